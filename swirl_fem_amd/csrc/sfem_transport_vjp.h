// Vector-Jacobian product of the scalar-transport right-hand side
// (sfem_transport.h).  The forward kernel computes per element
//
//   out[q] = W[q] (s[q] + sum_j m_j T_j[q])
//          + sum_j c_j sum_a U_j,a[q] (D_a T_j)[q],   U_j,a = sum_c Kw[a][c] u_j,c
//
// which is linear in s and bilinear in (T_j, u_j).  With lam the cotangent of
// `out`:
//
//   s_bar[q]      = W[q] lam[q]
//   T_bar_j[q]    = m_j W[q] lam[q] + c_j sum_a (D_a^T (U_j,a . lam))[q]
//   u_bar_j[q][c] = c_j lam[q] sum_a Kw[a][c][q] (D_a T_j)[q]
//
// transport_vjp_kernel is a sibling of transport_rhs_kernel: ElemCof with
// cof_fence, the shared lane mapping and LDS derivative stage
// (SFEM_PAIR_LINES_DM, sfem_helmholtz.h), the same AFFINE / MULTILINEAR /
// POINT launches.  Per level:
//   1. (u_bar wanted) load T_j and run the forward derivative stage: the
//      axis-0 derivative stays in registers, axes 1 and 2 are left in s0, s1;
//   2. pointwise, one cofactor evaluation per point: u_bar from the three
//      derivatives, stored as DIM consecutive reals; the fluxes
//      F_a = c_j U_a lam from the same K, F_0 in a register, F_1 and F_2 over
//      this lane's own words of s0 and s1 (the lane has just read them, no
//      other lane touches them between the two barriers);
//   3. (T_bar wanted) barrier, transposed lines in place along the last and
//      the middle axis, barrier, T_bar_j = D_0^T F_0 + s0 + s1 + m_j W lam;
//   4. barrier before the next level.
// Every output pointer is optional.  Without dvelocity[j] the level skips the
// load of T_j and stage 1, without dscalar[j] stage 3; a level with a null
// velocity or conv_coef = 0 does its mass term only.  All of these are kernel
// arguments, so the tests are uniform over the workgroup and every barrier
// stays outside the `active` / `lane_ok` branches.  Element-local in and out:
// no gather, no scatter, no atomics.
//
// A lane holds lam, a derivative line and a flux line (3 P values) next to the
// 2 P of a line product, one line more than the forward kernel, so in fp64 the
// kernel asks for fewer waves per SIMD than the parents (VjpTile::MINW, as
// SensTile does) rather than spill.
#pragma once
#include "sfem_stokes.h"

namespace sfem {

template <typename T>
struct TransportVjpParams {
  StokesParams<T> geo;   // as in TransportParams
  const T* lam;                               // cotangent of `out` (E, N)
  const T* scalar[SFEM_TRANSPORT_LEVELS];     // T_j (E, N); read for dvelocity
  const T* velocity[SFEM_TRANSPORT_LEVELS];   // u_j (E, N, DIM) or null
  T mass_coef[SFEM_TRANSPORT_LEVELS];
  T conv_coef[SFEM_TRANSPORT_LEVELS];
  const T* wdet;                              // (E, N) w detJ or null
  T* dscalar[SFEM_TRANSPORT_LEVELS];          // (E, N) or null
  T* dvelocity[SFEM_TRANSPORT_LEVELS];        // (E, N, DIM) or null
  T* dsource;                                 // (E, N) or null
  int num_levels;
};

template <typename T, int P>
struct VjpTile {
  // waves per SIMD asked of the register allocator: 3 P + 2 P live values
  static constexpr int MINW =
      sizeof(T) == 8 ? (P <= 5 ? 4 : 2) : (P <= 8 ? 4 : 2);
};

template <typename T, int P, int DIM, int GM>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (VjpTile<T, P>::MINW))
transport_vjp_kernel(TransportVjpParams<T> tp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  const StokesParams<T>& prm = tp.geo;
  SFEM_LANE_PROLOGUE(prm);
  ElemCof<T, P, DIM, GM> geom;
  geom.init(prm, dm, e, active, i, j, t);
  // per-point arrays of this element: lane t of slice a reads point
  // a * TPE + t (coalesced); a velocity holds DIM consecutive reals per point
  const T* wd = tp.wdet ? tp.wdet + e * N : nullptr;

  T la[P];
  {
    const T* le = tp.lam + e * N;
#pragma unroll
    for (int a = 0; a < P; ++a) la[a] = active ? le[t + a * TPE] : T(0);
  }
  if (tp.dsource && active) {
    T* se = tp.dsource + e * N;
#pragma unroll
    for (int a = 0; a < P; ++a) se[t + a * TPE] = wd[t + a * TPE] * la[a];
  }

#pragma unroll 1
  for (int lev = 0; lev < tp.num_levels; ++lev) {
    const T mc = tp.mass_coef[lev], cc = tp.conv_coef[lev];
    const T* ve = tp.velocity[lev];
    const bool conv = ve != nullptr && cc != T(0);
    T* dT = tp.dscalar[lev] ? tp.dscalar[lev] + e * N : nullptr;
    T* dU = tp.dvelocity[lev] ? tp.dvelocity[lev] + e * N * DIM : nullptr;
    if (!conv) {   // the mass term alone; a velocity without effect gets zero
      if (active) {
#pragma unroll
        for (int a = 0; a < P; ++a) {
          const int q = t + a * TPE;
          if (dT) dT[q] = mc != T(0) ? mc * wd[q] * la[a] : T(0);
          if (dU) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) dU[q * DIM + c] = T(0);
          }
        }
      }
      continue;
    }
    if (!dT && !dU) continue;
    ve += e * N * DIM;
    cof_fence(geom);
    T d0[P];
#pragma unroll
    for (int a = 0; a < P; ++a) d0[a] = T(0);
    if (dU) {   // the forward derivative stage of T_j
      const T* te = tp.scalar[lev] + e * N;
      T ua[P];
#pragma unroll
      for (int a = 0; a < P; ++a) ua[a] = active ? te[t + a * TPE] : T(0);
      line_apply<T, P, false>(dm, ua, d0);
      SFEM_PAIR_SPREAD(ua);
      __syncthreads();
      SFEM_PAIR_LINES_DM(false);
      __syncthreads();
    }
    // pointwise: u_bar out, the fluxes over the derivatives this lane read
    T f0[P];
    if (lane_ok) {
#pragma unroll
      for (int a = 0; a < P; ++a) {
        const int o = a * SA + i * SB + j;
        T F[DIM];
#pragma unroll
        for (int ax = 0; ax < DIM; ++ax) F[ax] = T(0);
        if (active) {
          const int q = t + a * TPE;
          const T* vq = ve + (int64_t)q * DIM;
          T K[DIM * DIM];
          geom.cof(dm, a, K);
          const T cl = cc * la[a];
          if (dU) {
            T g[DIM];
            g[0] = d0[a];
            g[1] = s0[o];
            if constexpr (DIM == 3) g[2] = s1[o];
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
              T v = T(0);
#pragma unroll
              for (int ax = 0; ax < DIM; ++ax) v += K[ax * DIM + c] * g[ax];
              dU[q * DIM + c] = cl * v;
            }
          }
          if (dT) {
            T vel[DIM];
#pragma unroll
            for (int c = 0; c < DIM; ++c) vel[c] = vq[c];
#pragma unroll
            for (int ax = 0; ax < DIM; ++ax) {
              T U = T(0);               // contravariant velocity along xi_ax
#pragma unroll
              for (int c = 0; c < DIM; ++c) U += K[ax * DIM + c] * vel[c];
              F[ax] = cl * U;
            }
          }
        }
        f0[a] = F[0];
        if (dT) {
          s0[o] = F[1];
          if constexpr (DIM == 3) s1[o] = F[2];
        }
      }
    } else {
#pragma unroll
      for (int a = 0; a < P; ++a) f0[a] = T(0);
    }
    if (dT) {
      __syncthreads();
      SFEM_PAIR_LINES_DM(true);   // the transposed derivatives, in place
      T dt0[P];
      line_apply<T, P, true>(dm, f0, dt0);
      __syncthreads();
      if (active) {
#pragma unroll
        for (int a = 0; a < P; ++a) {
          const int o = a * SA + i * SB + j;
          const int q = t + a * TPE;
          T v = dt0[a] + s0[o];
          if constexpr (DIM == 3) v += s1[o];
          if (mc != T(0)) v += mc * wd[q] * la[a];
          dT[q] = v;
        }
      }
    }
    __syncthreads();   // the next level overwrites the tensor pair
  }
}

template <typename T, int P, int DIM>
int launch_transport_vjp(const TransportVjpParams<T>& tp, hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>("transport_rhs_vjp",
                                                        tp.geo, &L))
    return rc;
  with_geo_mode(tp.geo.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL((transport_vjp_kernel<T, P, DIM, decltype(gm)::value>),
                       L.grid, L.block, 0, stream, tp, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_transport_vjp(const TransportVjpParams<T>& tp, int P,
                           hipStream_t stream);

#define SFEM_DEFINE_TRANSPORT_VJP_DISPATCH(TYPE, DIMV)                       \
  template <>                                                                \
  int dispatch_transport_vjp<TYPE, DIMV>(                                    \
      const TransportVjpParams<TYPE>& tp, int P, hipStream_t stream) {       \
    return with_order<2, 12>("transport_rhs_vjp", P, [&](auto p) {           \
      return launch_transport_vjp<TYPE, decltype(p)::value, DIMV>(tp,        \
                                                                  stream);   \
    });                                                                      \
  }

}  // namespace sfem
