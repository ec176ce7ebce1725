// Coefficient sensitivities of the Helmholtz operator with an advective term,
// element-local:  for A(k, c, beta) = lambda0 B_c + lambda1 A_k + C_beta and
// two fields u, lam given on the operator's point grid, per point q
//
//   dkappa[q]   = d(lam . A u)/dk[q]      = lambda1 g_lam(q) . G(q) g_u(q)
//   dsigma[q]   = d(lam . A u)/dc[q]      = lambda0 W(q) lam(q) u(q)
//   dbeta[q,d]  = d(lam . A u)/dbeta[q,d] = lam(q) (D_d u)(q)
//
// with g_u, g_lam the reference-space gradients and G, W the geometric factors
// WITHOUT any coefficient folded in.  No gather and no scatter: inputs and
// outputs are (E, N[, DIM]) arrays indexed by element id.
//
// helmholtz_sens_kernel is a sibling of helmholtz_adv_kernel: lane mapping and
// LDS derivative stage are the shared macros of sfem_helmholtz.h.
// The derivative stage runs once per field: the DIM * P derivatives of u are
// kept in registers while those of lam go through the LDS pair again, so a
// lane holds 6 P values (u, lam, three derivatives of u, the axis-0 derivative
// of lam) next to the 2 P of a line product.  That is more than the register
// budget of the operator kernels' launch bounds admits in fp64 from P = 7 on,
// so the kernel asks for fewer waves per SIMD there (SensTile::MINW).
// Outputs are written in the plane layout the per-point coefficients are read
// in: lane t of slice a writes point a * TPE + t (coalesced), dbeta as DIM
// consecutive reals.  An output pointer that is null skips its product and
// its stores.
#pragma once
#include "sfem_helmholtz.h"

namespace sfem {

template <typename T>
struct HelmholtzSensParams : HelmholtzParams<T> {
  const T* lam;          // second field (E, N); the first is `u`
  T* dkappa;             // (E, N) or null
  T* dsigma;             // (E, N) or null
  T* dbeta;              // (E, N, DIM) or null
};

template <typename T, int P>
struct SensTile {
  // waves per SIMD asked of the register allocator: 6 P + 2 P live values
  static constexpr int MINW =
      sizeof(T) == 8 ? (P <= 6 ? 4 : 2) : (P <= 8 ? 4 : 2);
};

template <typename T, int P, int DIM, int GM>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (SensTile<T, P>::MINW))
helmholtz_sens_kernel(HelmholtzSensParams<T> prm, DMat<T, P> dm) {
  using PRM = HelmholtzSensParams<T>;
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);

  SFEM_LANE_PROLOGUE(prm);
  const DMat<T, P>& dmat = dm;
  const bool want_k = prm.dkappa != nullptr;
  const bool want_c = prm.dsigma != nullptr;
  const bool want_b = prm.dbeta != nullptr;

  ElemGeom<T, P, DIM, GM> geom;
#if SFEM_KERNARG_PICK
  static_assert(sizeof(PRM) % alignof(DMat<T, P>) == 0, "");
  geom.template init<true>(prm, dm, e, active, i, j, t,
                           kernarg_dmat<T, P>(sizeof(PRM)));
#else
  geom.init(prm, dm, e, active, i, j, t);
#endif
  const uint32_t slot_off = (uint32_t)t;
  const T* up = prm.u + e * N;
  const T* lp = prm.lam + e * N;

  // derivative stage of one field: x[a] = the lane's values (a, i, j) in,
  // dx0[a] = its axis-0 derivative out; the axis-1 / axis-2 derivatives at
  // (a, i, j) are left in s0 / s1
  auto derivatives = [&](const T (&x)[P], T (&dx0)[P]) {
    SFEM_LINE_APPLY(PRM, false, x, dx0);
    SFEM_PAIR_SPREAD(x);
    __syncthreads();
    SFEM_PAIR_LINES(PRM, false);
    __syncthreads();
  };

  T ua[P], gu0[P], gu1[P];
  [[maybe_unused]] T gu2[DIM == 3 ? P : 1];
#pragma unroll
  for (int a = 0; a < P; ++a)
    ua[a] = active ? up[slot_off + a * TPE] : T(0);
  derivatives(ua, gu0);
#pragma unroll
  for (int a = 0; a < P; ++a) {
    const int o = a * SA + i * SB + j;
    gu1[a] = lane_ok ? s0[o] : T(0);
    if constexpr (DIM == 3) gu2[a] = lane_ok ? s1[o] : T(0);
  }
  __syncthreads();        // every lane has read u's derivatives: reuse the pair

  T la[P], gl0[P] = {};
#pragma unroll
  for (int a = 0; a < P; ++a)
    la[a] = active ? lp[slot_off + a * TPE] : T(0);
  // lam's derivatives feed dkappa only
  if (want_k) derivatives(la, gl0);

  if (active) {
    T* kout = want_k ? prm.dkappa + e * N : nullptr;
    T* sout = want_c ? prm.dsigma + e * N : nullptr;
    T* bout = want_b ? prm.dbeta + e * N * DIM : nullptr;
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int o = a * SA + i * SB + j;
      const uint32_t q = slot_off + a * TPE;
      if (want_b) {
        bout[q * DIM] = la[a] * gu0[a];
        bout[q * DIM + 1] = la[a] * gu1[a];
        if constexpr (DIM == 3) bout[q * DIM + 2] = la[a] * gu2[a];
      }
      if (!want_k && !want_c) continue;
      T Wm = T(0);
      if (want_k) {
        const T h0 = gl0[a], h1 = s0[o];
        T dk;
        if constexpr (GM == GEO_MULTILINEAR && DIM == 3) {
          T o0, o1, o2;
          geom.apply_multilinear3(dm, a, want_c, gu0[a], gu1[a], gu2[a], o0, o1,
                                  o2, Wm);
          dk = h0 * o0 + h1 * o1 + s1[o] * o2;
        } else {
          T G[6];
          geom.factors(dm, a, true, want_c, G, Wm);
          if constexpr (DIM == 3) {
            const T h2 = s1[o];
            dk = h0 * (G[0] * gu0[a] + G[1] * gu1[a] + G[2] * gu2[a]) +
                 h1 * (G[1] * gu0[a] + G[3] * gu1[a] + G[4] * gu2[a]) +
                 h2 * (G[2] * gu0[a] + G[4] * gu1[a] + G[5] * gu2[a]);
          } else {
            dk = h0 * (G[0] * gu0[a] + G[1] * gu1[a]) +
                 h1 * (G[1] * gu0[a] + G[3] * gu1[a]);
          }
        }
        kout[q] = prm.lambda1 * dk;
      } else {
        T G[6];
        geom.factors(dm, a, false, true, G, Wm);
      }
      if (want_c) sout[q] = prm.lambda0 * Wm * la[a] * ua[a];
    }
  }
}

template <typename T, int P, int DIM>
int launch_helmholtz_sens(const HelmholtzSensParams<T>& prm,
                          hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc =
          element_launch<HelmholtzTile<T, P, DIM>>("helmholtz_sens", prm, &L))
    return rc;
  with_geo_mode(prm.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL((helmholtz_sens_kernel<T, P, DIM, decltype(gm)::value>),
                       L.grid, L.block, 0, stream, prm, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_helmholtz_sens(const HelmholtzSensParams<T>& prm, int P,
                            hipStream_t stream);

#define SFEM_DEFINE_HELMHOLTZ_SENS_DISPATCH(TYPE, DIMV)                     \
  template <>                                                               \
  int dispatch_helmholtz_sens<TYPE, DIMV>(                                  \
      const HelmholtzSensParams<TYPE>& prm, int P, hipStream_t stream) {    \
    return with_order<2, 12>("helmholtz_sens", P, [&](auto p) {             \
      return launch_helmholtz_sens<TYPE, decltype(p)::value, DIMV>(prm,     \
                                                                   stream); \
    });                                                                     \
  }

}  // namespace sfem
