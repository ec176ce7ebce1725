// Lame and density sensitivities of the linear-elasticity operator, element-
// local:  for A(lam, mu, rho) = K + lambda0 M_rho (sfem_elasticity.h) and two
// displacement fields u, v given on the collocated grid, per point q
//
//   dlam[q] = d(v . A u)/dlam[q] = W tr(H_u) tr(H_v)
//   dmu[q]  = d(v . A u)/dmu[q]  = W sum_{c,j} (H_u[c][j] + H_u[j][c]) H_v[c][j]
//   drho[q] = d(v . A u)/drho[q] = lambda0 W sum_c u_c v_c
//
// with H = (1/W) Kw G the physical gradient, Kw the weighted cofactors of
// ElemCof and W = w detJ (`wdet`), none with a coefficient folded in.  No
// gather, no scatter, no atomics: inputs are (E, N, DIM), outputs (E, N)
// arrays indexed by element id, in the layout the forward kernel reads its
// per-point coefficients in (lane t of slice a writes point a * TPE + t).
//
// elasticity_sens_kernel is a sibling of elasticity_kernel: ElemCof and the
// shared lane mapping and LDS derivative stage (sfem_helmholtz.h).  Holding
// the DIM x DIM reference derivatives of both fields would take 2 DIM^2 P
// reals per lane.  Row c of H depends on the DIM reference derivatives of
// component c alone, so the components pass one after another:
//   1. u, component by component: the symmetric E_u = H_u + H_u^T is
//      accumulated in registers (6 values per point in 3D, 3 in 2D; tr H_u is
//      half its diagonal sum);
//   2. v, component by component: dmu += E_u[c][j] H_v[c][j] and tr H_v.
// A lane then holds (6 + 2) P reals (3D) next to the P values of the
// component, its axis-0 derivative and the 2 P of a line product; the other
// derivatives are read from the LDS pair at the point.  ElemCof::cof is
// evaluated again per component.  SensBudget asks for fewer waves per SIMD
// where that does not fit.  An output pointer that is null skips its product
// and its stores; with dlam and dmu both null no derivative stage runs.  All
// barriers stay outside the `active` / `lane_ok` branches (`want_*` are
// kernel arguments, uniform over the grid).
#pragma once
#include "sfem_elasticity.h"

namespace sfem {

template <typename T>
struct ElasticitySensParams {
  StokesParams<T> geo;   // kfac / geo_elem / geo_index / elem_list /
                         // num_elements / geo_mode / *_host; the rest unused
  const T* u;            // (E, N, DIM)
  const T* v;            // (E, N, DIM)
  const T* wdet;         // (E, N) w detJ
  T* dlam;               // (E, N) or null
  T* dmu;                // (E, N) or null
  T* drho;               // (E, N) or null
  T lambda0;
};

// Waves per SIMD asked of the compiler.  LIVE_REGS: the per-point values a
// lane keeps across the component passes (E_u, dmu, tr H_v) plus one
// component's values, its axis-0 derivative and a line product.
template <typename T, int P, int DIM>
struct ElasticitySensBudget {
  static constexpr int NSYM = DIM * (DIM + 1) / 2;
  static constexpr int LIVE_REGS = (NSYM + 2 + 4) * P * (int)sizeof(T) / 4;
  static constexpr int MINW =
      LIVE_REGS > 200 ? 1
                      : (LIVE_REGS > 60 ? 2 : HelmholtzTile<T, P, DIM>::MINW);
};

template <typename T, int P, int DIM, int GM>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (ElasticitySensBudget<T, P, DIM>::MINW))
elasticity_sens_kernel(ElasticitySensParams<T> sp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  constexpr int NSYM = DIM * (DIM + 1) / 2;
  const StokesParams<T>& prm = sp.geo;
  SFEM_LANE_PROLOGUE(prm);
  const bool want_l = sp.dlam != nullptr;
  const bool want_m = sp.dmu != nullptr;
  const bool want_r = sp.drho != nullptr;
  const T* ue = sp.u + e * N * DIM;
  const T* ve = sp.v + e * N * DIM;
  const T* wd = sp.wdet + e * N;

  // es[s][a]: E_u = H_u + H_u^T at the lane's point of slice a; s = c on the
  // diagonal, DIM + c + j - 1 for c < j
  T es[NSYM][P] = {};
  T dm_acc[P] = {}, trv[P] = {};

  if (want_l || want_m) {   // uniform over the grid
    ElemCof<T, P, DIM, GM> geom;
    geom.init(prm, dm, e, active, i, j, t);

    // The shared stages, as lambdas: this kernel was written with lambdas, and
    // its register allocation follows their inlining (the macros alone move
    // registers in every instantiation).
    auto derivatives = [&](const T (&x)[P], T (&dx0)[P]) {
      SFEM_ELAST_DERIVATIVES(x, dx0);
    };
    auto gradient_row = [&](int a, T g0, T (&h)[DIM]) {
      SFEM_ELAST_GRADIENT_ROW(a, g0, h);
    };

#pragma unroll
    for (int c = 0; c < DIM; ++c) {   // pass 1: E_u
      T xa[P], g0[P];
#pragma unroll
      for (int a = 0; a < P; ++a)
        xa[a] = active ? ue[(int64_t)(t + a * TPE) * DIM + c] : T(0);
      derivatives(xa, g0);
      if (active) {
#pragma unroll
        for (int a = 0; a < P; ++a) {
          T h[DIM];
          gradient_row(a, g0[a], h);
#pragma unroll
          for (int jj = 0; jj < DIM; ++jj) {
            if (jj == c)
              es[c][a] += h[jj] + h[jj];
            else
              es[DIM + c + jj - 1][a] += h[jj];
          }
        }
      }
      __syncthreads();   // the next component overwrites the tensor pair
    }

#pragma unroll
    for (int c = 0; c < DIM; ++c) {   // pass 2: contraction with H_v
      T xa[P], g0[P];
#pragma unroll
      for (int a = 0; a < P; ++a)
        xa[a] = active ? ve[(int64_t)(t + a * TPE) * DIM + c] : T(0);
      derivatives(xa, g0);
      if (active) {
#pragma unroll
        for (int a = 0; a < P; ++a) {
          T h[DIM];
          gradient_row(a, g0[a], h);
          trv[a] += h[c];
          if (want_m) {
#pragma unroll
            for (int jj = 0; jj < DIM; ++jj)
              dm_acc[a] += es[jj == c ? c : DIM + c + jj - 1][a] * h[jj];
          }
        }
      }
      __syncthreads();   // the next component overwrites the tensor pair
    }
  }

  if (active) {
    T* lout = want_l ? sp.dlam + e * N : nullptr;
    T* mout = want_m ? sp.dmu + e * N : nullptr;
    T* rout = want_r ? sp.drho + e * N : nullptr;
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int q = t + a * TPE;
      const T w = wd[q];
      if (want_l) {
        T tru = es[0][a] + es[1][a];
        if constexpr (DIM == 3) tru += es[2][a];
        lout[q] = w * (T(0.5) * tru) * trv[a];
      }
      if (want_m) mout[q] = w * dm_acc[a];
      if (want_r) {
        T s = T(0);
#pragma unroll
        for (int c = 0; c < DIM; ++c)
          s += ue[(int64_t)q * DIM + c] * ve[(int64_t)q * DIM + c];
        rout[q] = sp.lambda0 * w * s;
      }
    }
  }
}

template <typename T, int P, int DIM>
int launch_elasticity_sens(const ElasticitySensParams<T>& sp,
                           hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>("elasticity_sens",
                                                        sp.geo, &L))
    return rc;
  with_geo_mode(sp.geo.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL(
        (elasticity_sens_kernel<T, P, DIM, decltype(gm)::value>), L.grid,
        L.block, 0, stream, sp, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_elasticity_sens(const ElasticitySensParams<T>& sp, int P,
                             hipStream_t stream);

#define SFEM_DEFINE_ELASTICITY_SENS_DISPATCH(TYPE, DIMV)                     \
  template <>                                                                \
  int dispatch_elasticity_sens<TYPE, DIMV>(                                  \
      const ElasticitySensParams<TYPE>& sp, int P, hipStream_t stream) {     \
    return with_order<2, 12>("elasticity_sens", P, [&](auto p) {             \
      return launch_elasticity_sens<TYPE, decltype(p)::value, DIMV>(sp,      \
                                                                    stream); \
    });                                                                      \
  }

}  // namespace sfem
