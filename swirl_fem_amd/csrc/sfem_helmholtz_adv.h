// Helmholtz operator with an advective term, index rows / element-local:
//
//   out = mask * scatter( (lambda0 B_c + lambda1 A_k + C_b)_local(g) ),
//   C_b[i,j] = sum_q W_q phi_i(q) b_q . grad phi_j(q)
//
// At a collocated point q the advective term is a dot product of the
// reference-space derivatives of u (the lines helmholtz_kernel computes for the
// stiffness term anyway) with the folded velocity
//   beta[e,q,d] = W[e,q] sum_j b[e,q,j] invjac[e,q,j,d],
// added to the pointwise (mass-like) contribution of q.  So the term does not
// depend on the geometry kind and costs DIM extra loads per point and no extra
// derivative line.
//
// helmholtz_adv_kernel is a sibling of helmholtz_kernel (sfem_helmholtz.h): the
// same lane mapping and LDS derivative stage (SFEM_TILE_PREAMBLE,
// SFEM_LANE_PROLOGUE, SFEM_PAIR_SPREAD, SFEM_PAIR_LINES there) and ElemGeom.
// It is kept apart so that the constant- and variable-coefficient
// instantiations compile from code this file never touches.
// Scalar fields, slot-order scatter; kappa / sigma per point or null
// (one form bounds the number of instantiations: Python expands scalars and
// per-element values).  The derivative lines are always computed (C_b needs
// them when lambda1 = 0 as well); lambda0 is tested at run time.
//
// TR: the transposed advective term.  B_c and A_k are symmetric, and
//   (C_b^T v)_i = sum_q (sum_d beta[q,d] D_d phi_i(q)) v(q),
// so at a point beta[q,d] * v(q) joins the reference-space flux of direction
// d ahead of the transposed derivative lines and nothing joins the mass-like
// accumulator.  For that the flux carries lambda1 from the pointwise stage on
// (lambda1 k G g) and the final accumulation adds the transposed-derivative
// sum unscaled.  A template argument, not a run-time flag: tested at run time
// (wave-uniform) the forward kernels lost registers to the three beta values
// and u that stay live across the geometry evaluation (fp64 3D affine, P = 8:
// 192 -> 348 bytes of scratch per lane; P = 12: 0 -> 180; P = 4: 102 -> 118
// VGPRs), so the forward instantiations compile from the code they always
// had.
#pragma once
#include "sfem_helmholtz.h"

namespace sfem {

template <typename T>
struct HelmholtzAdvParams : HelmholtzParams<T> {
  const T* kappa;        // diffusivity (E, N) slot order; null = 1
  const T* sigma;        // reaction (E, N); null = 1
  const T* beta;         // folded velocity (E, N, DIM), slot order
};

template <typename T, int P, int DIM, bool GS, int GM, bool TR = false>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (HelmholtzTile<T, P, DIM>::MINW))
helmholtz_adv_kernel(HelmholtzAdvParams<T> prm, DMat<T, P> dm) {
  using PRM = HelmholtzAdvParams<T>;
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);

  SFEM_LANE_PROLOGUE(prm);
  const DMat<T, P>& dmat = dm;
  const int64_t ns = prm.node_stride;
  const bool has_mass = prm.lambda0 != T(0);

  ElemGeom<T, P, DIM, GM> geom;
#if SFEM_KERNARG_PICK
  static_assert(sizeof(PRM) % alignof(DMat<T, P>) == 0, "");
  geom.template init<true>(prm, dm, e, active, i, j, t,
                           kernarg_dmat<T, P>(sizeof(PRM)));
#else
  geom.init(prm, dm, e, active, i, j, t);
#endif
  const uint32_t slot_off = (uint32_t)t;

  // per-point arrays of this element, read in the plane layout of the stored
  // factors: lane t of slice a reads point a * TPE + t (coalesced); beta holds
  // DIM consecutive reals per point, so a wave reads one contiguous strip
  const T* kpt = prm.kappa ? prm.kappa + e * N : nullptr;
  const T* cpt = prm.sigma ? prm.sigma + e * N : nullptr;
  const T* bpt = prm.beta + e * N * DIM;

  uint32_t enc[P];
  if (GS) {
    const int32_t* enc0 = prm.enc + e * N;
#pragma unroll
    for (int a = 0; a < P; ++a)
      enc[a] = active ? (uint32_t)__builtin_nontemporal_load(
                            &enc0[slot_off + a * TPE])
                      : (uint32_t)SFEM_IDX_PAD;
  }
  const T* ul0 = GS ? nullptr : prm.u + e * N * ns;
  T* ol0 = GS ? nullptr : prm.out + e * N * ns;
  const T* ug = prm.u;
  T* og = prm.out;

  T ua[P], acc[P];
#pragma unroll
  for (int a = 0; a < P; ++a) {
    if (GS) {
      const uint32_t id = enc[a] & SFEM_IDX_MASK;
      ua[a] = id == SFEM_IDX_PAD ? T(0) : ug[(int64_t)id * ns];
    } else {
      ua[a] = active ? ul0[(int64_t)(slot_off + a * TPE) * ns] : T(0);
    }
  }
  T d0[P];   // derivative along axis 0 at (a, i, j)
  SFEM_LINE_APPLY(PRM, false, ua, d0);
  SFEM_PAIR_SPREAD(ua);
  __syncthreads();
  SFEM_PAIR_LINES(PRM, false);
  __syncthreads();
  // pointwise: the advective and mass terms go to acc, w = k G * (reference
  // gradient) replaces the gradient
  T w0[P];
#pragma unroll
  for (int a = 0; a < P; ++a) { w0[a] = T(0); acc[a] = T(0); }
  if (active) {
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int o = a * SA + i * SB + j;
      const uint32_t q = slot_off + a * TPE;
      const T g0 = d0[a], g1 = s0[o];
      [[maybe_unused]] T g2 = T(0);
      if constexpr (DIM == 3) g2 = s1[o];
      T adv = T(0);
      if constexpr (!TR) {
        adv = bpt[q * DIM] * g0 + bpt[q * DIM + 1] * g1;
        if constexpr (DIM == 3) adv += bpt[q * DIM + 2] * g2;
      }
      const T kq = (TR ? prm.lambda1 : T(1)) * (kpt ? kpt[q] : T(1));
      T Wm;
      if constexpr (GM == GEO_MULTILINEAR && DIM == 3) {
        T o0, o1, o2;
        geom.apply_multilinear3(dm, a, has_mass, g0, g1, g2, o0, o1, o2, Wm);
        w0[a] = kq * o0; s0[o] = kq * o1; s1[o] = kq * o2;
      } else {
        T G[6];
        geom.factors(dm, a, true, has_mass, G, Wm);
        if constexpr (DIM == 3) {
          w0[a] = kq * (G[0] * g0 + G[1] * g1 + G[2] * g2);
          s0[o] = kq * (G[1] * g0 + G[3] * g1 + G[4] * g2);
          s1[o] = kq * (G[2] * g0 + G[4] * g1 + G[5] * g2);
        } else {
          w0[a] = kq * (G[0] * g0 + G[1] * g1);
          s0[o] = kq * (G[1] * g0 + G[3] * g1);
        }
      }
      if constexpr (TR) {     // beta * u joins the flux, after the geometry
        w0[a] += bpt[q * DIM] * ua[a];
        s0[o] += bpt[q * DIM + 1] * ua[a];
        if constexpr (DIM == 3) s1[o] += bpt[q * DIM + 2] * ua[a];
      }
      if (has_mass) {
        if (cpt) Wm *= cpt[q];
        adv += prm.lambda0 * Wm * ua[a];
      }
      acc[a] = adv;
    }
  }
  __syncthreads();
  SFEM_PAIR_LINES(PRM, true);   // the transposed derivatives, in place
  T dt0[P];
  SFEM_LINE_APPLY(PRM, true, w0, dt0);
  __syncthreads();
  if (lane_ok) {
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int o = a * SA + i * SB + j;
      T v = dt0[a] + s0[o];
      if (DIM == 3) v += s1[o];
      acc[a] += TR ? v : prm.lambda1 * v;   // TR: lambda1 rode in with the flux
    }
  }
  // direct-stiffness summation in slot order
#pragma unroll
  for (int a = 0; a < P; ++a) {
    if (GS) {
      const uint32_t ea = enc[a];
      const uint32_t id = ea & SFEM_IDX_MASK;
      if (id != SFEM_IDX_PAD) {
        T* dst = og + (int64_t)id * ns;
        const bool dirichlet = ea & SFEM_IDX_DIRICHLET;
        if (ea & SFEM_IDX_SHARED) {
          if (!dirichlet) {
            if (prm.colored) *dst = *dst + acc[a];
            else unsafeAtomicAdd(dst, acc[a]);
          }
        } else {
          *dst = dirichlet ? T(0) : acc[a];
        }
      }
    } else if (active) {
      ol0[(int64_t)(slot_off + a * TPE) * ns] = acc[a];
    }
  }
}

template <typename T, int P, int DIM, bool GS, bool TR>
int launch_helmholtz_adv(const HelmholtzAdvParams<T>& prm, hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>("helmholtz", prm, &L))
    return rc;
  with_geo_mode(prm.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL(
        (helmholtz_adv_kernel<T, P, DIM, GS, decltype(gm)::value, TR>), L.grid,
        L.block, 0, stream, prm, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_helmholtz_adv(const HelmholtzAdvParams<T>& prm, int P, bool gs,
                           bool transpose, hipStream_t stream);

#define SFEM_DEFINE_HELMHOLTZ_ADV_DISPATCH(TYPE, DIMV)                      \
  template <>                                                               \
  int dispatch_helmholtz_adv<TYPE, DIMV>(                                   \
      const HelmholtzAdvParams<TYPE>& prm, int P, bool gs, bool transpose,  \
      hipStream_t stream) {                                                 \
    return with_order<2, 12>("helmholtz", P, [&](auto p) {                  \
      return with_flag(gs, [&](auto g) {                                    \
        return with_flag(transpose, [&](auto tr) {                          \
          return launch_helmholtz_adv<TYPE, decltype(p)::value, DIMV,       \
                                      decltype(g)::value,                   \
                                      decltype(tr)::value>(prm, stream);    \
        });                                                                 \
      });                                                                   \
    });                                                                     \
  }

}  // namespace sfem
