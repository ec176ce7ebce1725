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

// What the entry points of this family copy out of their args struct of
// include/sfem.h (any of them: a template over the struct).  The geometry and
// launch fields, for `work` elements:
template <typename T, typename Args>
void fill_geometry(const Args* a, int64_t work, StokesParams<T>* g) {
  g->kfac = (const T*)a->kfac;
  g->geo_elem = (const T*)a->geo_elem;
  g->geo_index = a->geo_index;
  g->elem_list = a->elem_list;
  g->dmat_host = (const T*)a->dmat;
  g->weights_host = (const T*)a->weights;
  g->nodes_host = (const T*)a->nodes;
  g->num_elements = work;
  g->geo_mode = a->geo_mode;
}

// ... and with them every field of ElasticityParams.
template <typename T, typename Args>
void fill_elasticity(const Args* a, int64_t work, ElasticityParams<T>* ep) {
  fill_geometry<T>(a, work, &ep->geo);
  ep->u = (const T*)a->u;
  ep->out = (T*)a->out;
  ep->wdet = (const T*)a->wdet;
  ep->lam = (const T*)a->lam;
  ep->mu = (const T*)a->mu;
  ep->rho = (const T*)a->rho;
  ep->lam_const = (T)a->lam_const;
  ep->mu_const = (T)a->mu_const;
  ep->rho_const = (T)a->rho_const;
  ep->lambda0 = (T)a->lambda0;
}

// Waves per SIMD asked of the compiler: two (256 registers per lane) once
// the DIM x DIM lines alone take more than 40 registers.
template <typename T, int P, int DIM>
struct ElasticityBudget {
  static constexpr int LINE_REGS = DIM * DIM * P * (int)sizeof(T) / 4;
  static constexpr int MINW =
      LINE_REGS > 40 ? 2 : HelmholtzTile<T, P, DIM>::MINW;
};

// ---------------------------------------------------------------- stages ---
// The stages that the kernels of this family share (elasticity_kernel here,
// hyperelastic_kernel, plasticity_kernel, the two sensitivity kernels and the
// stress kernels).  Macros, for the reason given at SFEM_PAIR_LINES_WITH
// (sfem_helmholtz.h): as force-inlined function templates taking array
// references the gradient and fold stages moved registers in 13 of the 66
// kernels of sfem_hyperelastic_f32_2d; as macros every kernel is
// byte-identical to its open-coded text.  All of them expect T, P, DIM, the
// names of SFEM_TILE_PREAMBLE and SFEM_LANE_PROLOGUE and the DMat `dm` in
// scope; what else, each says itself.

// Derivative stage of one component: X[a] = the lane's values (a, i, j) in,
// DX0[a] = the axis-0 derivative out; the axis-1 / axis-2 derivatives at
// (a, i, j) are left in s0 / s1.  Barriers included, so not under a branch.
#define SFEM_ELAST_DERIVATIVES(X, DX0)                                        \
  do {                                                                        \
    line_apply<T, P, false>(dm, X, DX0);                                      \
    SFEM_PAIR_SPREAD(X);                                                      \
    __syncthreads();                                                          \
    SFEM_PAIR_LINES_DM(false);                                                \
    __syncthreads();                                                          \
  } while (0)

// Its transpose: G[ax][a] = the lane's values at (a, i, j) per axis in,
// DT0[a] = the transposed axis-0 derivative of G[0] out; those of G[1] / G[2]
// at (a, i, j) are left in s0 / s1 and the caller sums the three.  Barriers
// included, so not under a branch.
#define SFEM_ELAST_DERIVATIVES_T(G, DT0)                                      \
  do {                                                                        \
    if (lane_ok) {                                                            \
      _Pragma("unroll") for (int a_ = 0; a_ < P; ++a_) {                      \
        const int o_ = a_ * SA + i * SB + j;                                  \
        s0[o_] = (G)[1][a_];                                                  \
        if constexpr (DIM == 3) s1[o_] = (G)[2][a_];                          \
      }                                                                       \
    }                                                                         \
    __syncthreads();                                                          \
    SFEM_PAIR_LINES_DM(true);   /* in place */                                \
    line_apply<T, P, true>(dm, (G)[0], DT0);                                  \
    __syncthreads();                                                          \
  } while (0)

// Row c of the physical gradient at the lane's point of slice A, from the
// axis-0 derivative G0 and the LDS pair that SFEM_ELAST_DERIVATIVES left (the
// kernels that keep no DIM x DIM lines).  Expects the ElemCof `geom` and
// `wd` = the element's wdet; H is T[DIM].  W = 0 gives a zero row.
#define SFEM_ELAST_GRADIENT_ROW(A, G0, H)                                     \
  do {                                                                        \
    const int o_ = (A) * SA + i * SB + j;                                     \
    T K_[DIM * DIM];                                                          \
    geom.cof(dm, (A), K_);                                                    \
    const T wq_ = wd[t + (A) * TPE];                                          \
    const T iw_ = wq_ != T(0) ? T(1) / wq_ : T(0);                            \
    T g_[DIM];                                                                \
    g_[0] = (G0);                                                             \
    g_[1] = s0[o_];                                                           \
    if constexpr (DIM == 3) g_[2] = s1[o_];                                   \
    _Pragma("unroll") for (int jj_ = 0; jj_ < DIM; ++jj_) {                   \
      T s_ = T(0);                                                            \
      _Pragma("unroll") for (int ax_ = 0; ax_ < DIM; ++ax_)                   \
          s_ += K_[ax_ * DIM + jj_] * g_[ax_];                                \
      (H)[jj_] = iw_ * s_;                                                    \
    }                                                                         \
  } while (0)

// Intake: every component of `ue`, the element's (N, DIM) values, through the
// derivative stage into the lines T g[DIM][DIM][P]: g[c][ax][a] =
// d u_c / d xi_ax at the lane's point of slice a.  Barriers included, so not
// under a branch.
#define SFEM_ELAST_INTAKE()                                                   \
  _Pragma("unroll") for (int c_ = 0; c_ < DIM; ++c_) {                        \
    T ua_[P];                                                                 \
    _Pragma("unroll") for (int a_ = 0; a_ < P; ++a_)                          \
        ua_[a_] = active ? ue[(int64_t)(t + a_ * TPE) * DIM + c_] : T(0);     \
    SFEM_ELAST_DERIVATIVES(ua_, g[c_][0]);                                    \
    _Pragma("unroll") for (int a_ = 0; a_ < P; ++a_) {                        \
      const int o_ = a_ * SA + i * SB + j;                                    \
      g[c_][1][a_] = lane_ok ? s0[o_] : T(0);                                 \
      if constexpr (DIM == 3) g[c_][2][a_] = lane_ok ? s1[o_] : T(0);         \
    }                                                                         \
    __syncthreads();   /* the next component overwrites the tensor pair */    \
  }

// Physical gradient, row C at the lane's point of slice A: H[C][j] = IW
// sum_ax K[ax * DIM + j] g[C][ax][A], from the cofactors T K[DIM * DIM] and
// the lines g; H is T[DIM][DIM] and the caller loops over C (elasticity_kernel
// sums the trace between the rows).  IW = 1 / W is the caller's:
// elasticity_kernel divides without a guard, its siblings take 0 where W = 0
// (a padded mesh).
#define SFEM_ELAST_GRADIENT(C, A, IW, H)                                      \
  _Pragma("unroll") for (int jj = 0; jj < DIM; ++jj) {                        \
    T h = T(0);                                                               \
    _Pragma("unroll") for (int ax = 0; ax < DIM; ++ax)                        \
        h += K[ax * DIM + jj] * g[C][ax][A];                                  \
    (H)[C][jj] = (IW) * h;                                                    \
  }

// Fold of the stress row S[DIM] of component C at slice A into the lines:
// g[C][ax][A] = sum_j K[ax * DIM + j] S[j].
#define SFEM_ELAST_FOLD(C, A, S)                                              \
  _Pragma("unroll") for (int ax = 0; ax < DIM; ++ax) {                        \
    T f = T(0);                                                               \
    _Pragma("unroll") for (int jj = 0; jj < DIM; ++jj)                        \
        f += K[ax * DIM + jj] * (S)[jj];                                      \
    g[C][ax][A] = f;                                                          \
  }

// Output: per component the transposed derivative stage of the folded lines
// g, plus lambda0 rho W u, stored to `oe`, the element's (N, DIM) output.
// Expects the ElasticityParams `ep` and `ue`.  Barriers included, so not under
// a branch.
#define SFEM_ELAST_OUTPUT()                                                   \
  do {                                                                        \
    const bool mass = ep.lambda0 != T(0);                                     \
    _Pragma("unroll") for (int c_ = 0; c_ < DIM; ++c_) {                      \
      T dt0[P];                                                               \
      SFEM_ELAST_DERIVATIVES_T(g[c_], dt0);                                   \
      if (active) {                                                           \
        const T* wd = ep.wdet + e * N;                                        \
        const T* rhoe = ep.rho ? ep.rho + e * N : nullptr;                    \
        _Pragma("unroll") for (int a_ = 0; a_ < P; ++a_) {                    \
          const int o_ = a_ * SA + i * SB + j;                                \
          const int q = t + a_ * TPE;                                         \
          T v = dt0[a_] + s0[o_];                                             \
          if (DIM == 3) v += s1[o_];                                          \
          if (mass)                                                           \
            v += ep.lambda0 * (rhoe ? rhoe[q] : ep.rho_const) * wd[q] *       \
                 ue[(int64_t)q * DIM + c_];                                   \
          oe[(int64_t)q * DIM + c_] = v;                                      \
        }                                                                     \
      }                                                                       \
      __syncthreads();   /* the next component overwrites the tensor pair */  \
    }                                                                         \
  } while (0)

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
  SFEM_ELAST_INTAKE();

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
      const T iw = T(1) / wd[q];   // no W = 0 guard here, unlike the siblings
      const T lq = lame ? lame[q] : ep.lam_const;
      const T mq = mue ? mue[q] : ep.mu_const;
      T H[DIM][DIM];
      T tr = T(0);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        SFEM_ELAST_GRADIENT(c, a, iw, H);
        tr += H[c][c];
      }
      const T lt = lq * tr;
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        T S[DIM];
#pragma unroll
        for (int jj = 0; jj < DIM; ++jj)
          S[jj] = mq * (H[c][jj] + H[jj][c]) + (jj == c ? lt : T(0));
        SFEM_ELAST_FOLD(c, a, S);
      }
    }
  }

  SFEM_ELAST_OUTPUT();
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

// The launcher of a sibling with a residual (mode 0) and a tangent (mode 1)
// kernel: `prm.el` are its ElasticityParams and kernel_of(gm, tangent) is the
// kernel for the two compile-time constants.
template <typename T, int P, int DIM, typename PRM, typename F>
int launch_two_mode(const char* who, const PRM& prm, int mode,
                    hipStream_t stream, F&& kernel_of) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>(who, prm.el.geo, &L))
    return rc;
  with_geo_mode(prm.el.geo.geo_mode, [&](auto gm) {
    with_flag(mode == 1, [&](auto tangent) {
      auto kernel = kernel_of(gm, tangent);
      hipLaunchKernelGGL(kernel, L.grid, L.block, 0, stream, prm, L.dm);
    });
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
