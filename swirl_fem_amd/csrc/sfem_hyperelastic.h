// Compressible neo-Hookean elasticity, total Lagrangian, on a collocated grid
// of P points per direction (the quadrature grid of the solve, reached by
// interpolation).  With F = I + H, H[c][j] = d u_c / d X_j, J = det F:
//
//   psi(F) = mu/2 (F:F - d) - mu ln J + lam/2 (ln J)^2
//   P(F)   = mu (F - F^-T) + lam ln J F^-T              (first Piola-Kirchhoff)
//   dP[dH] = mu dH + (mu - lam ln J) F^-T dH^T F^-T + lam tr(F^-1 dH) F^-T
//
// (plane strain in 2D: the 2 x 2 block).  hyperelastic_kernel is a sibling of
// elasticity_kernel (sfem_elasticity.h) and is made of its stages, the
// SFEM_ELAST_* macros there: the same lane mapping, derivative stages,
// DIM x DIM x P register lines per lane, mass term, stores and barriers.
// Only the pointwise stage is its own, per element and point with
// Kw[a][j] = w detJ d xi_a / d X_j (ElemCof, the reference mesh) and W = w detJ:
//
//   MODE = HYPER_RESIDUAL, out = R(u):
//     H = (1/W) Kw G,  F^-1 by the adjugate,  lnJ = log(det F)
//     g[c][a] = sum_j Kw[a][j] P[c][j]
//     state[e,q,:] = (F^-1 row-major, lnJ)     where `state` is given
//     psi[e,q] = W psi(F) + lambda0/2 rho W |u|^2   where `psi` is given
//   MODE = HYPER_TANGENT, out = T(u) w for the increment w in `u`:
//     dH = (1/W) Kw G_w,  F^-1 and lnJ loaded from `state` for the point
//     g[c][a] = sum_j Kw[a][j] dP[dH][c][j]
//
// The tangent takes no inverse and no logarithm: it runs once per CG iteration
// of a linearisation, the residual once.  F^-1, lnJ and the cofactors are
// transient inside the per-point loop.  J <= 0 (an inverted trial state) is
// arithmetic: log gives NaN or -inf and the element's outputs are non-finite;
// no address depends on a data value.  Points with W = 0 (the all -1 rows of
// a padded mesh) take H = 0.
#pragma once
#include "sfem_elasticity.h"

namespace sfem {

enum { HYPER_RESIDUAL = 0, HYPER_TANGENT = 1 };

template <typename T>
struct HyperelasticParams {
  ElasticityParams<T> el;   // u (the increment w in tangent mode), out, wdet,
                            // lam / mu / rho, lambda0 and the geometry
  T* state;                 // (E, N, DIM * DIM + 1): written by the residual
                            // where non-null, read by the tangent
  T* psi;                   // (E, N) or null; residual mode only
};

__device__ __forceinline__ double hyper_log(double x) { return ::log(x); }
__device__ __forceinline__ float hyper_log(float x) { return ::logf(x); }

// det and inverse of a DIM x DIM matrix by the adjugate.
template <typename T, int DIM>
__device__ __forceinline__ T hyper_inverse(const T (&F)[DIM][DIM],
                                           T (&Fi)[DIM][DIM]) {
  if constexpr (DIM == 2) {
    const T J = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    const T iJ = T(1) / J;
    Fi[0][0] = F[1][1] * iJ;
    Fi[0][1] = -F[0][1] * iJ;
    Fi[1][0] = -F[1][0] * iJ;
    Fi[1][1] = F[0][0] * iJ;
    return J;
  } else {
    T A[3][3];
    A[0][0] = F[1][1] * F[2][2] - F[1][2] * F[2][1];
    A[0][1] = F[0][2] * F[2][1] - F[0][1] * F[2][2];
    A[0][2] = F[0][1] * F[1][2] - F[0][2] * F[1][1];
    A[1][0] = F[1][2] * F[2][0] - F[1][0] * F[2][2];
    A[1][1] = F[0][0] * F[2][2] - F[0][2] * F[2][0];
    A[1][2] = F[0][2] * F[1][0] - F[0][0] * F[1][2];
    A[2][0] = F[1][0] * F[2][1] - F[1][1] * F[2][0];
    A[2][1] = F[0][1] * F[2][0] - F[0][0] * F[2][1];
    A[2][2] = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    const T J = F[0][0] * A[0][0] + F[0][1] * A[1][0] + F[0][2] * A[2][0];
    const T iJ = T(1) / J;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int jj = 0; jj < 3; ++jj) Fi[c][jj] = A[c][jj] * iJ;
    return J;
  }
}

template <typename T, int P, int DIM, int GM, int MODE>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (ElasticityBudget<T, P, DIM>::MINW))
hyperelastic_kernel(HyperelasticParams<T> hp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  const ElasticityParams<T>& ep = hp.el;
  const StokesParams<T>& prm = ep.geo;
  SFEM_LANE_PROLOGUE(prm);
  constexpr int NS = DIM * DIM + 1;
  ElemCof<T, P, DIM, GM> geom;
  geom.init(prm, dm, e, active, i, j, t);
  const T* ue = ep.u + e * N * DIM;
  T* oe = ep.out + e * N * DIM;

  // g[c][ax][a]: d u_c / d xi_ax at the lane's point of slice a, then the
  // folded Piola stress (or its increment)
  T g[DIM][DIM][P];
  SFEM_ELAST_INTAKE();

  // pointwise: reference derivatives -> H (or dH) -> P (or dP) -> fold
  if (active) {
    const T* wd = ep.wdet + e * N;
    const T* lame = ep.lam ? ep.lam + e * N : nullptr;
    const T* mue = ep.mu ? ep.mu + e * N : nullptr;
    const T* rhoe = ep.rho ? ep.rho + e * N : nullptr;
    T* se = hp.state ? hp.state + e * N * NS : nullptr;
    T* pe = hp.psi ? hp.psi + e * N : nullptr;
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int q = t + a * TPE;
      T K[DIM * DIM];
      geom.cof(dm, a, K);
      const T wq = wd[q];
      const T iw = wq != T(0) ? T(1) / wq : T(0);
      const T lq = lame ? lame[q] : ep.lam_const;
      const T mq = mue ? mue[q] : ep.mu_const;
      T H[DIM][DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) SFEM_ELAST_GRADIENT(c, a, iw, H);
      // what the rows of P(F), or of dP[dH], are made of; each row is folded
      // into g[c] as soon as it is formed (H holds what the later rows need)
      T Fi[DIM][DIM];
      T A[MODE == HYPER_TANGENT ? DIM : 1][DIM];   // tangent: F^-1 dH
      T c0, c1;
      if constexpr (MODE == HYPER_RESIDUAL) {
        T F[DIM][DIM];
        T ffd = T(0);   // F:F - d = 2 tr H + H:H, without the cancellation
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
#pragma unroll
          for (int jj = 0; jj < DIM; ++jj) {
            F[c][jj] = H[c][jj] + (c == jj ? T(1) : T(0));
            ffd += H[c][jj] * (H[c][jj] + (c == jj ? T(2) : T(0)));
          }
        }
        const T J = hyper_inverse<T, DIM>(F, Fi);
        const T lnJ = hyper_log(J);
        const T ll = lq * lnJ;
        c0 = T(0);
        c1 = ll;
        if (se) {
          T* sq = se + (int64_t)q * NS;
#pragma unroll
          for (int c = 0; c < DIM; ++c) {
#pragma unroll
            for (int jj = 0; jj < DIM; ++jj) sq[c * DIM + jj] = Fi[c][jj];
          }
          sq[DIM * DIM] = lnJ;
        }
        if (pe) {
          T w = mq * (T(0.5) * ffd - lnJ) + T(0.5) * ll * lnJ;
          if (ep.lambda0 != T(0)) {
            T uu = T(0);
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
              const T uc = ue[(int64_t)q * DIM + c];
              uu += uc * uc;
            }
            w += T(0.5) * ep.lambda0 * (rhoe ? rhoe[q] : ep.rho_const) * uu;
          }
          pe[q] = wq * w;
        }
      } else {
        const T* sq = se + (int64_t)q * NS;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
#pragma unroll
          for (int jj = 0; jj < DIM; ++jj) Fi[c][jj] = sq[c * DIM + jj];
        }
        const T lnJ = sq[DIM * DIM];
        // A = F^-1 dH, B = A F^-1; (F^-T dH^T F^-T)[c][j] = B[j][c]
        T tr = T(0);
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
#pragma unroll
          for (int jj = 0; jj < DIM; ++jj) {
            T s = T(0);
#pragma unroll
            for (int k = 0; k < DIM; ++k) s += Fi[c][k] * H[k][jj];
            A[c][jj] = s;
          }
          tr += A[c][c];
        }
        c0 = mq - lq * lnJ;
        c1 = lq * tr;
      }
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        T S[DIM];       // row c of P(F), or of dP[dH]
#pragma unroll
        for (int jj = 0; jj < DIM; ++jj) {
          if constexpr (MODE == HYPER_RESIDUAL) {
            S[jj] = mq * ((H[c][jj] + (c == jj ? T(1) : T(0))) - Fi[jj][c]) +
                    c1 * Fi[jj][c];
          } else {
            T b = T(0);
#pragma unroll
            for (int k = 0; k < DIM; ++k) b += A[jj][k] * Fi[k][c];
            S[jj] = mq * H[c][jj] + c0 * b + c1 * Fi[jj][c];
          }
        }
        SFEM_ELAST_FOLD(c, a, S);
      }
    }
  }

  SFEM_ELAST_OUTPUT();
}

template <typename T, int P, int DIM>
int launch_hyperelastic(const HyperelasticParams<T>& hp, int mode,
                        hipStream_t stream) {
  static_assert(HYPER_TANGENT == 1, "mode 1 of launch_two_mode");
  return launch_two_mode<T, P, DIM>(
      "hyperelastic", hp, mode, stream, [](auto gm, auto tangent) {
        return hyperelastic_kernel<T, P, DIM, decltype(gm)::value,
                                   decltype(tangent)::value>;
      });
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_hyperelastic(const HyperelasticParams<T>& hp, int P, int mode,
                          hipStream_t stream);

#define SFEM_DEFINE_HYPERELASTIC_DISPATCH(TYPE, DIMV)                        \
  template <>                                                                \
  int dispatch_hyperelastic<TYPE, DIMV>(const HyperelasticParams<TYPE>& hp,  \
                                        int P, int mode,                     \
                                        hipStream_t stream) {                \
    return with_order<2, 12>("hyperelastic", P, [&](auto p) {                \
      return launch_hyperelastic<TYPE, decltype(p)::value, DIMV>(hp, mode,   \
                                                                 stream);    \
    });                                                                      \
  }

}  // namespace sfem
