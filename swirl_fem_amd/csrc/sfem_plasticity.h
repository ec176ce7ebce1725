// Small-strain von Mises (J2) plasticity with linear isotropic hardening, on a
// collocated grid of P points per direction.  With H[c][j] = d u_c / d x_j,
// eps = sym(H) (plane strain in 2D: the 3 x 3 tensor with eps_zz = eps_xz =
// eps_yz = 0) and the committed history (eps_p, alpha) of the point:
//
//   e = eps - eps_p,  s_tr = 2 mu dev(e),  q = sqrt(3/2) |s_tr|
//   f = q - (sigma_y + Hh alpha)
//   f <= 0: sigma = lam tr(eps) I + 2 mu e,  history unchanged,
//           a = 2 mu, b = 0, n = 0
//   f >  0: dg = f / (3 mu + Hh),  n = s_tr / |s_tr|
//           eps_p' = eps_p + sqrt(3/2) dg n,  alpha' = alpha + dg
//           sigma  = (lam + 2 mu / 3) tr(eps) I + theta s_tr
//           theta  = 1 - 3 mu dg / q,  a = 2 mu theta
//           b      = 2 mu (1 / (1 + Hh / (3 mu)) - (1 - theta))
//   dsigma[deps] = lam tr(deps) I + 2 mu deps - (2 mu - a) dev(deps)
//                  - b (n : deps) n                   (the algorithmic tangent)
//
// plasticity_kernel is a sibling of elasticity_kernel (sfem_elasticity.h) and
// hyperelastic_kernel (sfem_hyperelastic.h) and is made of the same stages,
// the SFEM_ELAST_* macros of sfem_elasticity.h: the same lane mapping,
// derivative stages, DIM x DIM x P register lines per lane, mass term, stores
// and barriers.  Only the pointwise stage is its own, per element and point,
// with Kw[a][j] = w detJ d xi_a / d x_j (ElemCof) and W = w detJ:
//
//   MODE = PLAST_RESIDUAL, out = R(u):
//     H = (1/W) Kw G,  the return mapping from hist_in (null: virgin)
//     g[c][a] = sum_j Kw[a][j] sigma[c][j]
//     hist_out[e,q,:] = (eps_p', alpha')     where given
//     lin[e,q,:]      = (a, b, n)            where given
//     stress[e,q,:]   = sigma                where given
//   MODE = PLAST_TANGENT, out = T w for the increment w in `u`:
//     deps = sym((1/W) Kw G_w),  (a, b, n) loaded from `lin` for the point
//     g[c][a] = sum_j Kw[a][j] dsigma[deps][c][j]
//
// Voigt slots are those of elasticity_stress_kernel: 3D (xx, yy, zz, xy, xz,
// yz), 2D (xx, yy, xy) with zz last where it is stored.  Per point the history
// is NH = 7 reals in 3D (eps_p, alpha) and 4 in 2D (xx, yy, xy, alpha;
// eps_p,zz = -(xx + yy) is implied), `lin` is NL = 8 reals in 3D (a, b, n)
// and 5 in 2D (a, b, n_xx, n_yy, n_xy: deps_zz = 0, so nothing else enters
// n : deps), `stress` is 6 reals in 3D and 4 in 2D (xx, yy, xy, zz).
//
// The tangent takes no square root and no division: it runs once per CG
// iteration of a linearisation, the residual once.  History, `lin` and the
// cofactors are transient inside the per-point loop.  The yield test is a
// per-lane select over arithmetic that both sides can evaluate: no barrier
// and no address depends on it.  The elastic side never forms n, so
// |s_tr| = 0 does not divide.  Points with W = 0 (the all -1 rows of a padded
// mesh) take H = 0.
#pragma once
#include "sfem_elasticity.h"

namespace sfem {

enum { PLAST_RESIDUAL = 0, PLAST_TANGENT = 1 };

template <typename T>
struct PlasticityParams {
  ElasticityParams<T> el;   // u (the increment w in tangent mode), out, wdet,
                            // lam / mu / rho, lambda0 and the geometry
  const T* yield;           // (E, N) or null = yield_const
  const T* hard;            // (E, N) or null = hard_const
  T yield_const, hard_const;
  const T* hist_in;         // (E, N, NH) or null = virgin; residual only
  T* hist_out;              // (E, N, NH) or null; residual only
  T* lin;                   // (E, N, NL): written by the residual where
                            // non-null, read by the tangent
  T* stress;                // (E, N, NV) or null; residual only
};

template <int DIM>
struct PlasticityLayout {
  static constexpr int NV = DIM == 3 ? 6 : 4;   // stored stress slots
  static constexpr int NE = DIM == 3 ? 6 : 3;   // stored eps_p / n slots
  static constexpr int NH = NE + 1;
  static constexpr int NL = NE + 2;
};

__device__ __forceinline__ double plast_sqrt(double x) { return ::sqrt(x); }
__device__ __forceinline__ float plast_sqrt(float x) { return ::sqrtf(x); }

template <typename T, int P, int DIM, int GM, int MODE>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (ElasticityBudget<T, P, DIM>::MINW))
plasticity_kernel(PlasticityParams<T> pp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  const ElasticityParams<T>& ep = pp.el;
  const StokesParams<T>& prm = ep.geo;
  SFEM_LANE_PROLOGUE(prm);
  using Lay = PlasticityLayout<DIM>;
  constexpr int NV = Lay::NV, NE = Lay::NE, NH = Lay::NH, NL = Lay::NL;
  // where the in-plane and out-of-plane Voigt slots sit in a 6-array
  // (xx, yy, zz, xy, xz, yz) and in the stored NE-array
  constexpr int XY = DIM == 3 ? 3 : 2;
  ElemCof<T, P, DIM, GM> geom;
  geom.init(prm, dm, e, active, i, j, t);
  const T* ue = ep.u + e * N * DIM;
  T* oe = ep.out + e * N * DIM;

  // g[c][ax][a]: d u_c / d xi_ax at the lane's point of slice a, then the
  // folded stress (or its increment)
  T g[DIM][DIM][P];
  SFEM_ELAST_INTAKE();

  // pointwise: reference derivatives -> eps (or deps) -> sigma (or dsigma)
  // -> fold
  if (active) {
    const T* wd = ep.wdet + e * N;
    const T* lame = ep.lam ? ep.lam + e * N : nullptr;
    const T* mue = ep.mu ? ep.mu + e * N : nullptr;
    const T* yle = pp.yield ? pp.yield + e * N : nullptr;
    const T* hde = pp.hard ? pp.hard + e * N : nullptr;
    const T* hie = pp.hist_in ? pp.hist_in + e * N * NH : nullptr;
    T* hoe = pp.hist_out ? pp.hist_out + e * N * NH : nullptr;
    T* le = pp.lin ? pp.lin + e * N * NL : nullptr;
    T* ste = pp.stress ? pp.stress + e * N * NV : nullptr;
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
      // the strain (or its increment) in the stored slots; 2D: eps_zz = 0
      T ev[NE];
      ev[0] = H[0][0];
      ev[1] = H[1][1];
      ev[XY] = T(0.5) * (H[0][1] + H[1][0]);
      if constexpr (DIM == 3) {
        ev[2] = H[2][2];
        ev[4] = T(0.5) * (H[0][2] + H[2][0]);
        ev[5] = T(0.5) * (H[1][2] + H[2][1]);
      }
      T tr = ev[0] + ev[1];
      if constexpr (DIM == 3) tr += ev[2];
      // sg: sigma (or dsigma) in the stored eps slots; szz: its zz entry in 2D
      T sg[NE];
      T szz = T(0);
      if constexpr (MODE == PLAST_RESIDUAL) {
        const T yq = yle ? yle[q] : pp.yield_const;
        const T hq = hde ? hde[q] : pp.hard_const;
        T epv[NE];
        T al = T(0);
#pragma unroll
        for (int k = 0; k < NE; ++k) epv[k] = T(0);
        if (hie) {
          const T* hq_in = hie + (int64_t)q * NH;
#pragma unroll
          for (int k = 0; k < NE; ++k) epv[k] = hq_in[k];
          al = hq_in[NE];
        }
        // e = eps - eps_p; in 2D e_zz = -eps_p,zz = eps_p,xx + eps_p,yy
        T el[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) el[k] = ev[k] - epv[k];
        T ezz = T(0);
        if constexpr (DIM == 2) ezz = epv[0] + epv[1];
        T tre = el[0] + el[1] + (DIM == 3 ? el[2] : ezz);
        const T third = tre * T(1.0 / 3.0);
        const T m2 = T(2) * mq;
        // s_tr = 2 mu dev(e)
        T s[NE];
        s[0] = m2 * (el[0] - third);
        s[1] = m2 * (el[1] - third);
        s[XY] = m2 * el[XY];
        T s2;
        T s_zz = T(0);
        if constexpr (DIM == 3) {
          s[2] = m2 * (el[2] - third);
          s[4] = m2 * el[4];
          s[5] = m2 * el[5];
          s2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2] +
               T(2) * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]);
        } else {
          s_zz = m2 * (ezz - third);
          s2 = s[0] * s[0] + s[1] * s[1] + s_zz * s_zz + T(2) * s[2] * s[2];
        }
        const T sn = plast_sqrt(s2);
        const T r32 = T(1.2247448713915890491);   // sqrt(3/2)
        const T qv = r32 * sn;
        const T f = qv - (yq + hq * al);
        const bool plastic = f > T(0);
        // the elastic side keeps dg = 0 and never forms 1 / |s_tr|
        const T dg = plastic ? f / (T(3) * mq + hq) : T(0);
        const T isn = plastic ? T(1) / sn : T(0);
        const T theta = T(1) - T(3) * mq * dg * isn * (T(1) / r32);
        const T av = m2 * theta;
        const T bv = plastic
            ? m2 * (T(1) / (T(1) + hq / (T(3) * mq)) - (T(1) - theta))
            : T(0);
        // sigma: elastic lam tr(eps) I + 2 mu e; plastic (lam + 2 mu / 3)
        // tr(eps) I + theta s_tr
        const T vol_e = lq * tr;
        const T vol_p = (lq + m2 * T(1.0 / 3.0)) * tr;
        sg[0] = plastic ? vol_p + theta * s[0] : vol_e + m2 * el[0];
        sg[1] = plastic ? vol_p + theta * s[1] : vol_e + m2 * el[1];
        sg[XY] = plastic ? theta * s[XY] : m2 * el[XY];
        if constexpr (DIM == 3) {
          sg[2] = plastic ? vol_p + theta * s[2] : vol_e + m2 * el[2];
          sg[4] = plastic ? theta * s[4] : m2 * el[4];
          sg[5] = plastic ? theta * s[5] : m2 * el[5];
        } else {
          szz = plastic ? vol_p + theta * s_zz : vol_e + m2 * ezz;
        }
        const T step = r32 * dg * isn;   // eps_p' = eps_p + step s_tr
        if (hoe) {
          T* ho = hoe + (int64_t)q * NH;
#pragma unroll
          for (int k = 0; k < NE; ++k) ho[k] = epv[k] + step * s[k];
          ho[NE] = al + dg;
        }
        if (le) {
          T* lo = le + (int64_t)q * NL;
          lo[0] = av;
          lo[1] = bv;
#pragma unroll
          for (int k = 0; k < NE; ++k) lo[2 + k] = isn * s[k];
        }
        if (ste) {
          T* so = ste + (int64_t)q * NV;
#pragma unroll
          for (int k = 0; k < NE; ++k) so[k] = sg[k];
          if constexpr (DIM == 2) so[3] = szz;
        }
      } else {
        const T* lo = le + (int64_t)q * NL;
        const T av = lo[0];
        const T bv = lo[1];
        T nv[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) nv[k] = lo[2 + k];
        T nd = nv[0] * ev[0] + nv[1] * ev[1] + T(2) * nv[XY] * ev[XY];
        if constexpr (DIM == 3)
          nd += nv[2] * ev[2] + T(2) * (nv[4] * ev[4] + nv[5] * ev[5]);
        // dsigma = (lam + (2 mu - a) / 3) tr I + a deps - b (n : deps) n
        const T vol = (lq + (T(2) * mq - av) * T(1.0 / 3.0)) * tr;
        const T bn = bv * nd;
        sg[0] = vol + av * ev[0] - bn * nv[0];
        sg[1] = vol + av * ev[1] - bn * nv[1];
        sg[XY] = av * ev[XY] - bn * nv[XY];
        if constexpr (DIM == 3) {
          sg[2] = vol + av * ev[2] - bn * nv[2];
          sg[4] = av * ev[4] - bn * nv[4];
          sg[5] = av * ev[5] - bn * nv[5];
        }
      }
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        T S[DIM];       // row c of sigma, or of dsigma
        if constexpr (DIM == 3) {
          S[0] = c == 0 ? sg[0] : c == 1 ? sg[3] : sg[4];
          S[1] = c == 0 ? sg[3] : c == 1 ? sg[1] : sg[5];
          S[2] = c == 0 ? sg[4] : c == 1 ? sg[5] : sg[2];
        } else {
          S[0] = c == 0 ? sg[0] : sg[2];
          S[1] = c == 0 ? sg[2] : sg[1];
        }
        SFEM_ELAST_FOLD(c, a, S);
      }
    }
  }

  SFEM_ELAST_OUTPUT();
}

template <typename T, int P, int DIM>
int launch_plasticity(const PlasticityParams<T>& pp, int mode,
                      hipStream_t stream) {
  static_assert(PLAST_TANGENT == 1, "mode 1 of launch_two_mode");
  return launch_two_mode<T, P, DIM>(
      "plasticity", pp, mode, stream, [](auto gm, auto tangent) {
        return plasticity_kernel<T, P, DIM, decltype(gm)::value,
                                 decltype(tangent)::value>;
      });
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_plasticity(const PlasticityParams<T>& pp, int P, int mode,
                        hipStream_t stream);

#define SFEM_DEFINE_PLASTICITY_DISPATCH(TYPE, DIMV)                          \
  template <>                                                                \
  int dispatch_plasticity<TYPE, DIMV>(const PlasticityParams<TYPE>& pp,      \
                                      int P, int mode, hipStream_t stream) { \
    return with_order<2, 12>("plasticity", P, [&](auto p) {                  \
      return launch_plasticity<TYPE, decltype(p)::value, DIMV>(pp, mode,     \
                                                               stream);      \
    });                                                                      \
  }

}  // namespace sfem
