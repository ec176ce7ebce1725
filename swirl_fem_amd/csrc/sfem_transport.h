// Explicit right-hand side of BDFk/EXTk scalar transport,
//   dT/dt + u . grad T - div(k grad T) = s,
// on a collocated grid of P points per direction (the quadrature grid of the
// Helmholtz solve, reached by interpolation):
//
//   out[e,q] = W[e,q] (source[e,q] + sum_j mass_coef[j] T_j[e,q])
//            + sum_j conv_coef[j] sum_a (sum_c Kw[a][c] u_j,c[e,q]) d T_j / d xi_a
//
// for up to SFEM_TRANSPORT_LEVELS time levels j, with W = w detJ (`wdet`) and
// Kw[a][c] = w detJ d xi_a / d x_c the weighted cofactors of ElemCof.  The
// stepper passes mass_coef = -bdf[j] / dt and conv_coef = -ext[j].
//
// transport_rhs_kernel is a sibling of stokes_convect_kernel (sfem_stokes.h):
// ElemCof, and the lane mapping and LDS derivative stage shared through the
// macros of sfem_helmholtz.h (SFEM_PAIR_LINES_DM).  What differs:
//   * the differentiated field is a scalar and the advecting velocity is data
//     of its own, so a level's velocity is needed at the pointwise stage only
//     and is read there, DIM reals per point, instead of being held as
//     DIM x P registers across the derivative lines;
//   * the levels run one after another through the one LDS tensor pair into
//     one accumulator of P values per lane;
//   * a level without a velocity (null pointer) or with conv_coef = 0 skips
//     its derivative stage and its barriers.  Both are kernel arguments, so
//     the test is uniform over the workgroup and the barriers stay outside
//     the `active` / `lane_ok` branches.
// Element-local in and out; interpolation, its transpose, gather and scatter
// are separate kernels.
#pragma once
#include "sfem_stokes.h"

namespace sfem {

template <typename T>
struct TransportParams {
  StokesParams<T> geo;   // kfac / geo_elem / geo_index / elem_list /
                         // num_elements / geo_mode / *_host; the rest unused
  const T* scalar[SFEM_TRANSPORT_LEVELS];    // T_j (E, N)
  const T* velocity[SFEM_TRANSPORT_LEVELS];  // u_j (E, N, DIM) or null
  T mass_coef[SFEM_TRANSPORT_LEVELS];
  T conv_coef[SFEM_TRANSPORT_LEVELS];
  const T* source;       // (E, N) or null
  const T* wdet;         // (E, N) w detJ; null only without mass terms / source
  T* out;                // (E, N)
  int num_levels;
};

template <typename T, int P, int DIM, int GM>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (HelmholtzTile<T, P, DIM>::MINW))
transport_rhs_kernel(TransportParams<T> tp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  const StokesParams<T>& prm = tp.geo;
  SFEM_LANE_PROLOGUE(prm);
  ElemCof<T, P, DIM, GM> geom;
  geom.init(prm, dm, e, active, i, j, t);
  // per-point arrays of this element: lane t of slice a reads point
  // a * TPE + t (coalesced); a velocity holds DIM consecutive reals per point
  const T* wd = tp.wdet ? tp.wdet + e * N : nullptr;

  T acc[P];
#pragma unroll
  for (int a = 0; a < P; ++a) acc[a] = T(0);

#pragma unroll 1
  for (int lev = 0; lev < tp.num_levels; ++lev) {
    const T mc = tp.mass_coef[lev], cc = tp.conv_coef[lev];
    const T* ve = tp.velocity[lev];
    const bool conv = ve != nullptr && cc != T(0);
    if (!conv && mc == T(0)) continue;
    const T* te = tp.scalar[lev] + e * N;
    T ua[P];
#pragma unroll
    for (int a = 0; a < P; ++a) ua[a] = active ? te[t + a * TPE] : T(0);
    if (mc != T(0) && active) {
#pragma unroll
      for (int a = 0; a < P; ++a) acc[a] += mc * wd[t + a * TPE] * ua[a];
    }
    if (!conv) continue;
    ve += e * N * DIM;
    cof_fence(geom);
    T d0[P];
    line_apply<T, P, false>(dm, ua, d0);
    SFEM_PAIR_SPREAD(ua);
    __syncthreads();
    SFEM_PAIR_LINES_DM(false);
    __syncthreads();
    if (active) {
#pragma unroll
      for (int a = 0; a < P; ++a) {
        const int o = a * SA + i * SB + j;
        const T* vq = ve + (int64_t)(t + a * TPE) * DIM;
        T vel[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) vel[c] = vq[c];
        T K[DIM * DIM];
        geom.cof(dm, a, K);
        T v = T(0);
#pragma unroll
        for (int ax = 0; ax < DIM; ++ax) {
          T U = T(0);                 // contravariant velocity along xi_ax
#pragma unroll
          for (int c = 0; c < DIM; ++c) U += K[ax * DIM + c] * vel[c];
          const T g = ax == 0 ? d0[a] : (ax == 1 ? s0[o] : s1[o]);
          v += U * g;
        }
        acc[a] += cc * v;
      }
    }
    __syncthreads();   // the next level overwrites the tensor pair
  }

  if (active) {
    const T* se = tp.source ? tp.source + e * N : nullptr;
    T* oe = tp.out + e * N;
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int q = t + a * TPE;
      T v = acc[a];
      if (se) v += wd[q] * se[q];
      oe[q] = v;
    }
  }
}

template <typename T, int P, int DIM>
int launch_transport_rhs(const TransportParams<T>& tp, hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>("transport_rhs",
                                                        tp.geo, &L))
    return rc;
  with_geo_mode(tp.geo.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL((transport_rhs_kernel<T, P, DIM, decltype(gm)::value>),
                       L.grid, L.block, 0, stream, tp, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_transport_rhs(const TransportParams<T>& tp, int P,
                           hipStream_t stream);

#define SFEM_DEFINE_TRANSPORT_DISPATCH(TYPE, DIMV)                           \
  template <>                                                                \
  int dispatch_transport_rhs<TYPE, DIMV>(const TransportParams<TYPE>& tp,    \
                                         int P, hipStream_t stream) {        \
    return with_order<2, 12>("transport_rhs", P, [&](auto p) {               \
      return launch_transport_rhs<TYPE, decltype(p)::value, DIMV>(tp,        \
                                                                  stream);   \
    });                                                                      \
  }

}  // namespace sfem
