// Lame and density sensitivities of the neo-Hookean residual, element-local:
// for R(u; lam, mu, rho) of sfem_hyperelastic.h, a field v given on the
// collocated grid and the state (F^-1 row-major, ln J) that the residual launch
// stored at u, per point q
//
//   dlam[q] = d(v . R)/dlam[q] = W lnJ tr(F^-1 H_v)
//   dmu[q]  = d(v . R)/dmu[q]  = W (F : H_v - tr(F^-1 H_v))
//   drho[q] = d(v . R)/drho[q] = lambda0 W sum_c u_c v_c
//
// with H_v = (1/W) Kw G_v the physical gradient of v, tr(F^-1 H_v) =
// sum_{c,j} Fi[j][c] H_v[c][j] and W = w detJ (`wdet`): P(F) = mu (F - F^-T) +
// lam lnJ F^-T is linear in the coefficients.  No gather, no scatter, no
// atomics, and no address depends on a data value: inputs are (E, N, .),
// outputs (E, N) arrays indexed by element id, in the layout the forward
// kernel reads its per-point coefficients in.
//
// hyperelastic_sens_kernel is a sibling of elasticity_sens_kernel
// (sfem_elasticity_sens.h): ElemCof, the shared lane mapping and LDS
// derivative stage, one component at a time.  Only v is differentiated, in DIM
// passes.  Pass c forms row c of H_v and needs, at the point, column c of
// F^-1 (from the state) and row c of F, which is recovered from the state by
// the adjugate of F^-1 (hyper_inverse; the rows a pass does not use are dead
// code): u is not interpolated and differentiated a second time, and is read
// for drho alone.  Two accumulators per point stay live across the passes,
// tr(F^-1 H_v) and F : H_v, so a lane holds 2 P reals next to the P values of
// the component, its axis-0 derivative and the 2 P of a line product.  The
// state row of a point is read once per pass (DIM times; the repeats are
// served by the caches).  HyperelasticSensBudget asks for fewer waves per SIMD
// where that does not fit.
//
// A point with W = 0 (the all -1 rows of a padded mesh) stores exactly 0 in
// every output, whatever its state row holds: a zero F^-1 has no inverse, and
// the outputs are summed with the others for a scalar coefficient.  An output
// pointer that is null skips its product and its stores; with dlam and dmu
// both null no derivative stage runs.  All barriers stay outside the `active`
// / `lane_ok` branches (`want_*` are kernel arguments, uniform over the grid).
#pragma once
#include "sfem_hyperelastic.h"

namespace sfem {

template <typename T>
struct HyperelasticSensParams {
  StokesParams<T> geo;   // kfac / geo_elem / geo_index / elem_list /
                         // num_elements / geo_mode / *_host; the rest unused
  const T* v;            // (E, N, DIM)
  const T* state;        // (E, N, DIM * DIM + 1)
  const T* u;            // (E, N, DIM), or null where drho is null
  const T* wdet;         // (E, N) w detJ
  T* dlam;               // (E, N) or null
  T* dmu;                // (E, N) or null
  T* drho;               // (E, N) or null
  T lambda0;
};

// Waves per SIMD asked of the compiler.  LIVE_REGS: the two per-point
// accumulators a lane keeps across the component passes plus one component's
// values, its axis-0 derivative and a line product.  In 3D the adjugate of a
// 3 x 3 state and the cofactors of a curved element come on top: at 48 to 60
// registers of live state (double P = 4, 5; float P = 8 .. 10) the tile's own
// 4 waves per SIMD left 12 to 60 bytes of scratch in three instantiations, 3
// waves leave none.
template <typename T, int P, int DIM>
struct HyperelasticSensBudget {
  static constexpr int LIVE_REGS = (2 + 4) * P * (int)sizeof(T) / 4;
  static constexpr int TILE_MINW = HelmholtzTile<T, P, DIM>::MINW;
  static constexpr int MINW =
      LIVE_REGS > 200  ? 1
      : LIVE_REGS > 60 ? 2
      : (DIM == 3 && LIVE_REGS >= 48 && TILE_MINW > 3) ? 3
                                                       : TILE_MINW;
};

template <typename T, int P, int DIM, int GM>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (HyperelasticSensBudget<T, P, DIM>::MINW))
hyperelastic_sens_kernel(HyperelasticSensParams<T> sp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  constexpr int NS = DIM * DIM + 1;
  const StokesParams<T>& prm = sp.geo;
  SFEM_LANE_PROLOGUE(prm);
  const bool want_l = sp.dlam != nullptr;
  const bool want_m = sp.dmu != nullptr;
  const bool want_r = sp.drho != nullptr;
  const T* ve = sp.v + e * N * DIM;
  const T* se = sp.state + e * N * NS;
  const T* wd = sp.wdet + e * N;

  // at the lane's point of slice a: tr(F^-1 H_v) and F : H_v
  T tr_acc[P] = {}, fh_acc[P] = {};

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
    for (int c = 0; c < DIM; ++c) {
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
          const T* sq = se + (int64_t)(t + a * TPE) * NS;
          T Fi[DIM][DIM], F[DIM][DIM];
#pragma unroll
          for (int r = 0; r < DIM; ++r) {
#pragma unroll
            for (int jj = 0; jj < DIM; ++jj) Fi[r][jj] = sq[r * DIM + jj];
          }
#pragma unroll
          for (int jj = 0; jj < DIM; ++jj) tr_acc[a] += Fi[jj][c] * h[jj];
          if (want_m) {
            hyper_inverse<T, DIM>(Fi, F);   // F = (F^-1)^-1; row c is used
#pragma unroll
            for (int jj = 0; jj < DIM; ++jj) fh_acc[a] += F[c][jj] * h[jj];
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
    const T* ue = want_r ? sp.u + e * N * DIM : nullptr;
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int q = t + a * TPE;
      const T w = wd[q];
      // W = 0: the state row may hold anything (a zero F^-1 gives inf and
      // NaN above); the stores are exactly zero
      const bool live = w != T(0);
      if (want_l) {
        const T lnJ = se[(int64_t)q * NS + DIM * DIM];
        lout[q] = live ? w * lnJ * tr_acc[a] : T(0);
      }
      if (want_m) mout[q] = live ? w * (fh_acc[a] - tr_acc[a]) : T(0);
      if (want_r) {
        T s = T(0);
#pragma unroll
        for (int c = 0; c < DIM; ++c)
          s += ue[(int64_t)q * DIM + c] * ve[(int64_t)q * DIM + c];
        rout[q] = live ? sp.lambda0 * w * s : T(0);
      }
    }
  }
}

template <typename T, int P, int DIM>
int launch_hyperelastic_sens(const HyperelasticSensParams<T>& sp,
                             hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>("hyperelastic_sens",
                                                        sp.geo, &L))
    return rc;
  with_geo_mode(sp.geo.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL(
        (hyperelastic_sens_kernel<T, P, DIM, decltype(gm)::value>), L.grid,
        L.block, 0, stream, sp, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_hyperelastic_sens(const HyperelasticSensParams<T>& sp, int P,
                               hipStream_t stream);

#define SFEM_DEFINE_HYPERELASTIC_SENS_DISPATCH(TYPE, DIMV)                   \
  template <>                                                                \
  int dispatch_hyperelastic_sens<TYPE, DIMV>(                                \
      const HyperelasticSensParams<TYPE>& sp, int P, hipStream_t stream) {   \
    return with_order<2, 12>("hyperelastic_sens", P, [&](auto p) {           \
      return launch_hyperelastic_sens<TYPE, decltype(p)::value, DIMV>(       \
          sp, stream);                                                       \
    });                                                                      \
  }

}  // namespace sfem
