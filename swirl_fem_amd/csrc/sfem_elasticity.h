// Linear elasticity on a collocated grid of P points per direction (the
// quadrature grid of the solve, reached by interpolation):
//
//   out = K u + lambda0 M_rho u,   v^T K u = int sigma(u) : grad v,
//   sigma = lam tr(eps) I + 2 mu eps,  eps = (grad u + grad u^T) / 2
//
// per element and point, with Kw[a][j] = w detJ d xi_a / d x_j the weighted
// cofactors of ElemCof and W = w detJ (`wdet`):
//
//   G[c][a] = d u_c / d xi_a                          (derivative lines)
//   H[c][j] = (1/W) sum_a Kw[a][j] G[c][a]            (physical gradient)
//   S[c][j] = lam (tr H) delta_cj + mu (H[c][j] + H[j][c])
//   F[c][a] = sum_j Kw[a][j] S[c][j]
//   out[e,m,c] = sum_a sum_q D_a[q,m] F[c][a](q) + lambda0 rho W u_c(m)
//
// elasticity_kernel is a sibling of stokes_convect_kernel (sfem_stokes.h):
// ElemCof, and the lane mapping and LDS derivative stage shared through the
// macros of sfem_helmholtz.h (SFEM_PAIR_LINES_DM).  What differs:
//   * the pointwise stage couples the components: it needs all DIM x DIM
//     reference derivatives of a point at once.  The components pass one
//     after another through the one LDS tensor pair and every lane takes the
//     derivatives at its own points back into registers, DIM x DIM x P reals
//     per lane.  gfx950 has 512 VGPRs per lane and SIMD, and a tensor pair per
//     component would cost occupancy instead: three pairs at P = 8 fp64 are
//     27 KiB per one-wave workgroup, 5 waves per CU, where 9 P doubles in
//     registers still leave 8;
//   * F overwrites G in those registers, and the transposed derivative stage
//     then runs per component through the same tensor pair, as in
//     helmholtz_adv_kernel;
//   * the mass term re-reads u (the lines were not kept) where lambda0 != 0,
//     a kernel argument, so the test is uniform over the workgroup.
// All barriers stay outside the `active` / `lane_ok` branches.  Element-local
// in and out, (E, n, DIM) row-major; interpolation, its transpose, gather and
// scatter are separate kernels.
#pragma once
#include "sfem_stokes.h"

namespace sfem {

template <typename T>
struct ElasticityParams {
  StokesParams<T> geo;   // kfac / geo_elem / geo_index / elem_list /
                         // num_elements / geo_mode / *_host; the rest unused
  const T* u;            // (E, N, DIM)
  T* out;                // (E, N, DIM)
  const T* wdet;         // (E, N) w detJ
  const T* lam;          // (E, N) or null = lam_const
  const T* mu;           // (E, N) or null = mu_const
  const T* rho;          // (E, N) or null = rho_const
  T lam_const, mu_const, rho_const;
  T lambda0;             // 0 skips the mass term
};

// Waves per SIMD asked of the compiler: two (256 registers per lane) once
// the DIM x DIM lines alone take more than 40 registers.
template <typename T, int P, int DIM>
struct ElasticityBudget {
  static constexpr int LINE_REGS = DIM * DIM * P * (int)sizeof(T) / 4;
  static constexpr int MINW =
      LINE_REGS > 40 ? 2 : HelmholtzTile<T, P, DIM>::MINW;
};

template <typename T, int P, int DIM, int GM>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (ElasticityBudget<T, P, DIM>::MINW))
elasticity_kernel(ElasticityParams<T> ep, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  const StokesParams<T>& prm = ep.geo;
  SFEM_LANE_PROLOGUE(prm);
  ElemCof<T, P, DIM, GM> geom;
  geom.init(prm, dm, e, active, i, j, t);
  const T* ue = ep.u + e * N * DIM;
  T* oe = ep.out + e * N * DIM;

  // g[c][ax][a]: d u_c / d xi_ax at the lane's point of slice a, then F[c][ax]
  T g[DIM][DIM][P];
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    T ua[P];
#pragma unroll
    for (int a = 0; a < P; ++a)
      ua[a] = active ? ue[(int64_t)(t + a * TPE) * DIM + c] : T(0);
    line_apply<T, P, false>(dm, ua, g[c][0]);
    SFEM_PAIR_SPREAD(ua);
    __syncthreads();
    SFEM_PAIR_LINES_DM(false);
    __syncthreads();
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int o = a * SA + i * SB + j;
      g[c][1][a] = lane_ok ? s0[o] : T(0);
      if constexpr (DIM == 3) g[c][2][a] = lane_ok ? s1[o] : T(0);
    }
    __syncthreads();   // the next component overwrites the tensor pair
  }

  // pointwise: reference derivatives -> physical gradient -> stress -> F
  if (active) {
    const T* wd = ep.wdet + e * N;
    const T* lame = ep.lam ? ep.lam + e * N : nullptr;
    const T* mue = ep.mu ? ep.mu + e * N : nullptr;
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int q = t + a * TPE;
      T K[DIM * DIM];
      geom.cof(dm, a, K);
      const T iw = T(1) / wd[q];
      const T lq = lame ? lame[q] : ep.lam_const;
      const T mq = mue ? mue[q] : ep.mu_const;
      T H[DIM][DIM];
      T tr = T(0);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
#pragma unroll
        for (int jj = 0; jj < DIM; ++jj) {
          T h = T(0);
#pragma unroll
          for (int ax = 0; ax < DIM; ++ax) h += K[ax * DIM + jj] * g[c][ax][a];
          H[c][jj] = iw * h;
        }
        tr += H[c][c];
      }
      const T lt = lq * tr;
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        T S[DIM];
#pragma unroll
        for (int jj = 0; jj < DIM; ++jj)
          S[jj] = mq * (H[c][jj] + H[jj][c]) + (jj == c ? lt : T(0));
#pragma unroll
        for (int ax = 0; ax < DIM; ++ax) {
          T f = T(0);
#pragma unroll
          for (int jj = 0; jj < DIM; ++jj) f += K[ax * DIM + jj] * S[jj];
          g[c][ax][a] = f;
        }
      }
    }
  }

  const bool mass = ep.lambda0 != T(0);
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    if (lane_ok) {
#pragma unroll
      for (int a = 0; a < P; ++a) {
        const int o = a * SA + i * SB + j;
        s0[o] = g[c][1][a];
        if constexpr (DIM == 3) s1[o] = g[c][2][a];
      }
    }
    __syncthreads();
    SFEM_PAIR_LINES_DM(true);   // the transposed derivatives, in place
    T dt0[P];
    line_apply<T, P, true>(dm, g[c][0], dt0);
    __syncthreads();
    if (active) {
      const T* wd = ep.wdet + e * N;
      const T* rhoe = ep.rho ? ep.rho + e * N : nullptr;
#pragma unroll
      for (int a = 0; a < P; ++a) {
        const int o = a * SA + i * SB + j;
        const int q = t + a * TPE;
        T v = dt0[a] + s0[o];
        if (DIM == 3) v += s1[o];
        if (mass)
          v += ep.lambda0 * (rhoe ? rhoe[q] : ep.rho_const) * wd[q] *
               ue[(int64_t)q * DIM + c];
        oe[(int64_t)q * DIM + c] = v;
      }
    }
    __syncthreads();   // the next component overwrites the tensor pair
  }
}

template <typename T, int P, int DIM>
int launch_elasticity(const ElasticityParams<T>& ep, hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>("elasticity", ep.geo,
                                                        &L))
    return rc;
  with_geo_mode(ep.geo.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL((elasticity_kernel<T, P, DIM, decltype(gm)::value>),
                       L.grid, L.block, 0, stream, ep, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_elasticity(const ElasticityParams<T>& ep, int P,
                        hipStream_t stream);

#define SFEM_DEFINE_ELASTICITY_DISPATCH(TYPE, DIMV)                          \
  template <>                                                                \
  int dispatch_elasticity<TYPE, DIMV>(const ElasticityParams<TYPE>& ep,      \
                                      int P, hipStream_t stream) {           \
    return with_order<2, 12>("elasticity", P, [&](auto p) {                  \
      return launch_elasticity<TYPE, decltype(p)::value, DIMV>(ep, stream);  \
    });                                                                      \
  }

}  // namespace sfem
