// Stress recovery of linear elasticity on the collocated grid, element-local,
// and its vector-Jacobian product.  With H = (1/W) Kw G the physical gradient
// of the displacement (sfem_elasticity.h), t = tr H and per point q
//
//   sigma_cc = lam t + 2 mu H[c][c],   sigma_cj = mu (H[c][j] + H[j][c])
//   vm = sqrt(0.5 ((sxx-syy)^2 + (syy-szz)^2 + (szz-sxx)^2)
//             + 3 (sxy^2 + sxz^2 + syz^2))
//
// in Voigt slots: 3D (xx, yy, zz, xy, xz, yz), the `es` index of the
// sensitivity kernel; 2D (xx, yy, xy, zz) with sigma_zz = lam t (plane strain)
// or 0 (`plane_stress`, the caller passes the modified lambda).  No gather, no
// scatter, no atomics: u is (E, N, DIM), sigma (E, N, NV), vm (E, N), indexed
// by element id; lane t of slice a owns point a * TPE + t.
//
// elasticity_stress_kernel takes the register plan of elasticity_sens_kernel:
// the components of u pass one after another through the derivative stage and
// only E_u = H + H^T is kept (NSYM values per point); the axis-0 derivative of
// the current component sits in registers, the others are read from the LDS
// pair at the point.  ElemCof::cof is evaluated again per component.
//
// elasticity_stress_vjp_kernel, for a cotangent sbar (E, N, NV) and
// dbar = sum_c sbar_cc (+ sbar_zz in plane strain):
//
//   Hbar[c][j] = lam dbar delta_cj + mu (c == j ? 2 sbar_cc : sbar_cj)
//   Gbar[c][a] = (1/W) sum_j Kw[a][j] Hbar[c][j]
//   ubar[e,m,c] = sum_a sum_q D_a[q,m] Gbar[c][a](q)
//   dlam[q] = tr(H_u) dbar
//   dmu[q]  = sum_c 2 H_u[c][c] sbar_cc + sum_{c<j} (H_u[c][j] + H_u[j][c]) sbar_cj
//
// without a weight W (stress is a pointwise value, not an integral).  Row c of
// Hbar needs sbar at the point alone, so ubar runs per component like the
// transposed stage of elasticity_kernel, DIM P reals per lane; dlam and dmu
// are accumulated in a pass over the components of u (tr H_u and the
// contraction, 2 P reals), which is skipped when both are null.
//
// W = 0 (the all -1 rows of a padded mesh) gives zeros in every output.  An
// output pointer that is null skips its arithmetic and its stores.  All
// barriers stay outside the `active` / `lane_ok` branches (the `want_*` tests
// are kernel arguments, uniform over the grid).
#pragma once
#include "sfem_elasticity.h"

namespace sfem {

template <typename T>
struct ElasticityStressParams {
  StokesParams<T> geo;   // kfac / geo_elem / geo_index / elem_list /
                         // num_elements / geo_mode / *_host; the rest unused
  const T* u;            // (E, N, DIM)
  const T* wdet;         // (E, N) w detJ
  const T* lam;          // (E, N) or null = lam_const
  const T* mu;           // (E, N) or null = mu_const
  T* sigma;              // (E, N, NV) or null
  T* vm;                 // (E, N) or null
  T lam_const, mu_const;
  int plane_stress;      // 2D: sigma_zz = 0
};

template <typename T>
struct ElasticityStressVjpParams {
  StokesParams<T> geo;
  const T* sbar;         // (E, N, NV)
  const T* u;            // (E, N, DIM); read for dlam / dmu only
  const T* wdet;         // (E, N)
  const T* lam;          // (E, N) or null = lam_const
  const T* mu;           // (E, N) or null = mu_const
  T* ubar;               // (E, N, DIM) or null
  T* dlam;               // (E, N) or null
  T* dmu;                // (E, N) or null
  T lam_const, mu_const;
  int plane_stress;      // 2D: sbar_zz takes no part
};

// Waves per SIMD asked of the compiler.  LIVE_REGS: E_u, which a lane keeps
// across the component passes (the vjp kernel: the DIM lines of Gbar, fewer),
// plus one component's values, its axis-0 derivative and a line product.
// The thresholds are those of ElasticitySensBudget, which holds two values
// per point more and spills nowhere.
template <typename T, int P, int DIM>
struct ElasticityStressBudget {
  static constexpr int NSYM = DIM * (DIM + 1) / 2;
  static constexpr int LIVE_REGS = (NSYM + 4) * P * (int)sizeof(T) / 4;
  static constexpr int MINW =
      LIVE_REGS > 200 ? 1
                      : (LIVE_REGS > 60 ? 2 : HelmholtzTile<T, P, DIM>::MINW);
};

// The vjp kernel: its pointwise stages read sbar, lam, mu and W of every slice
// next to the stored cofactors, and the compiler keeps those loads in flight,
// so it asks for one wave earlier.  At the thresholds above the kernels on
// stored geometry spilled (fp64 3D P = 8, 9, 10: 140, 300, 468 bytes per
// lane; fp64 2D P = 12: 44 bytes).
template <typename T, int P, int DIM>
struct ElasticityStressVjpBudget {
  static constexpr int LIVE_REGS = ElasticityStressBudget<T, P, DIM>::LIVE_REGS;
  static constexpr int MINW =
      LIVE_REGS > 150 ? 1
                      : (LIVE_REGS > 60 ? 2 : HelmholtzTile<T, P, DIM>::MINW);
};

template <typename T, int P, int DIM, int GM>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (ElasticityStressBudget<T, P, DIM>::MINW))
elasticity_stress_kernel(ElasticityStressParams<T> sp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  constexpr int NSYM = DIM * (DIM + 1) / 2;
  constexpr int NV = DIM == 3 ? 6 : 4;
  const StokesParams<T>& prm = sp.geo;
  SFEM_LANE_PROLOGUE(prm);
  const bool want_s = sp.sigma != nullptr;
  const bool want_v = sp.vm != nullptr;
  const T* ue = sp.u + e * N * DIM;
  const T* wd = sp.wdet + e * N;

  ElemCof<T, P, DIM, GM> geom;
  geom.init(prm, dm, e, active, i, j, t);

  // es[s][a]: E_u = H + H^T at the lane's point of slice a; s = c on the
  // diagonal, DIM + c + j - 1 for c < j
  T es[NSYM][P] = {};
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    T xa[P], g0[P];
#pragma unroll
    for (int a = 0; a < P; ++a)
      xa[a] = active ? ue[(int64_t)(t + a * TPE) * DIM + c] : T(0);
    SFEM_ELAST_DERIVATIVES(xa, g0);
    if (active) {
#pragma unroll
      for (int a = 0; a < P; ++a) {
        T h[DIM];
        SFEM_ELAST_GRADIENT_ROW(a, g0[a], h);
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

  if (active) {
    const T* lame = sp.lam ? sp.lam + e * N : nullptr;
    const T* mue = sp.mu ? sp.mu + e * N : nullptr;
    T* sout = want_s ? sp.sigma + e * N * NV : nullptr;
    T* vout = want_v ? sp.vm + e * N : nullptr;
#pragma unroll
    for (int a = 0; a < P; ++a) {
      const int q = t + a * TPE;
      const T lq = lame ? lame[q] : sp.lam_const;
      const T mq = mue ? mue[q] : sp.mu_const;
      T tr = es[0][a] + es[1][a];
      if constexpr (DIM == 3) tr += es[2][a];
      const T lt = lq * (T(0.5) * tr);
      const T sxx = lt + mq * es[0][a];
      const T syy = lt + mq * es[1][a];
      T szz, sxy, sxz = T(0), syz = T(0);
      if constexpr (DIM == 3) {
        szz = lt + mq * es[2][a];
        sxy = mq * es[3][a];
        sxz = mq * es[4][a];
        syz = mq * es[5][a];
      } else {
        szz = sp.plane_stress ? T(0) : lt;
        sxy = mq * es[2][a];
      }
      if (want_s) {
        T* so = sout + (int64_t)q * NV;
        so[0] = sxx;
        so[1] = syy;
        if constexpr (DIM == 3) {
          so[2] = szz;
          so[3] = sxy;
          so[4] = sxz;
          so[5] = syz;
        } else {
          so[2] = sxy;
          so[3] = szz;
        }
      }
      if (want_v) {
        const T d0 = sxx - syy, d1 = syy - szz, d2 = szz - sxx;
        const T sh = sxy * sxy + sxz * sxz + syz * syz;
        vout[q] = sqrt(T(0.5) * (d0 * d0 + d1 * d1 + d2 * d2) + T(3) * sh);
      }
    }
  }
}

template <typename T, int P, int DIM, int GM>
__global__ void __launch_bounds__((HelmholtzTile<T, P, DIM>::BLOCK),
                                  (ElasticityStressVjpBudget<T, P, DIM>::MINW))
elasticity_stress_vjp_kernel(ElasticityStressVjpParams<T> sp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  constexpr int NV = DIM == 3 ? 6 : 4;
  const StokesParams<T>& prm = sp.geo;
  SFEM_LANE_PROLOGUE(prm);
  const bool want_u = sp.ubar != nullptr;
  const bool want_l = sp.dlam != nullptr;
  const bool want_m = sp.dmu != nullptr;
  const T* sbe = sp.sbar + e * N * NV;
  const T* wd = sp.wdet + e * N;
  // 2D plane strain: sigma_zz = lam t feeds sbar_zz into the trace
  const bool zz = DIM == 2 && !sp.plane_stress;

  ElemCof<T, P, DIM, GM> geom;
  geom.init(prm, dm, e, active, i, j, t);

  // the cotangent of sigma_cj at point q: slot c on the diagonal,
  // DIM + c + j - 1 off it (either order)
  auto sb = [&](int q, int c, int jj) {
    const int s = c == jj ? c : DIM + c + jj - 1;
    return sbe[(int64_t)q * NV + s];
  };
  auto dbar_at = [&](int q) {
    T d = sbe[(int64_t)q * NV] + sbe[(int64_t)q * NV + 1];
    if (DIM == 3) d += sbe[(int64_t)q * NV + 2];
    if (zz) d += sbe[(int64_t)q * NV + 3];
    return d;
  };

  if (want_l || want_m) {   // uniform over the grid
    const T* ue = sp.u + e * N * DIM;
    T tru[P] = {}, dm_acc[P] = {};
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      T xa[P], g0[P];
#pragma unroll
      for (int a = 0; a < P; ++a)
        xa[a] = active ? ue[(int64_t)(t + a * TPE) * DIM + c] : T(0);
      SFEM_ELAST_DERIVATIVES(xa, g0);
      if (active) {
#pragma unroll
        for (int a = 0; a < P; ++a) {
          T h[DIM];
          SFEM_ELAST_GRADIENT_ROW(a, g0[a], h);
          tru[a] += h[c];
          if (want_m) {
            const int q = t + a * TPE;
#pragma unroll
            for (int jj = 0; jj < DIM; ++jj)
              dm_acc[a] += (jj == c ? T(2) : T(1)) * sb(q, c, jj) * h[jj];
          }
        }
      }
      __syncthreads();   // the next component overwrites the tensor pair
    }
    if (active) {
      T* lout = want_l ? sp.dlam + e * N : nullptr;
      T* mout = want_m ? sp.dmu + e * N : nullptr;
#pragma unroll
      for (int a = 0; a < P; ++a) {
        const int q = t + a * TPE;
        if (want_l) lout[q] = tru[a] * dbar_at(q);
        if (want_m) mout[q] = dm_acc[a];
      }
    }
  }

  if (want_u) {   // uniform over the grid
    const T* lame = sp.lam ? sp.lam + e * N : nullptr;
    const T* mue = sp.mu ? sp.mu + e * N : nullptr;
    T* uo = sp.ubar + e * N * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      // g[ax][a]: Gbar[c][ax] at the lane's point of slice a
      T g[DIM][P] = {};
      if (active) {
#pragma unroll
        for (int a = 0; a < P; ++a) {
          const int q = t + a * TPE;
          T K[DIM * DIM];
          geom.cof(dm, a, K);
          const T wq = wd[q];
          const T iw = wq != T(0) ? T(1) / wq : T(0);
          const T lq = lame ? lame[q] : sp.lam_const;
          const T mq = mue ? mue[q] : sp.mu_const;
          const T ld = lq * dbar_at(q);
          T hb[DIM];
#pragma unroll
          for (int jj = 0; jj < DIM; ++jj)
            hb[jj] = jj == c ? ld + T(2) * mq * sb(q, c, c) : mq * sb(q, c, jj);
#pragma unroll
          for (int ax = 0; ax < DIM; ++ax) {
            T f = T(0);
#pragma unroll
            for (int jj = 0; jj < DIM; ++jj) f += K[ax * DIM + jj] * hb[jj];
            g[ax][a] = iw * f;
          }
        }
      }
      T dt0[P];
      SFEM_ELAST_DERIVATIVES_T(g, dt0);
      if (active) {
#pragma unroll
        for (int a = 0; a < P; ++a) {
          const int o = a * SA + i * SB + j;
          const int q = t + a * TPE;
          T v = dt0[a] + s0[o];
          if (DIM == 3) v += s1[o];
          uo[(int64_t)q * DIM + c] = v;
        }
      }
      __syncthreads();   // the next component overwrites the tensor pair
    }
  }
}

template <typename T, int P, int DIM>
int launch_elasticity_stress(const ElasticityStressParams<T>& sp,
                             hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>("elasticity_stress",
                                                        sp.geo, &L))
    return rc;
  with_geo_mode(sp.geo.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL(
        (elasticity_stress_kernel<T, P, DIM, decltype(gm)::value>), L.grid,
        L.block, 0, stream, sp, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

template <typename T, int P, int DIM>
int launch_elasticity_stress_vjp(const ElasticityStressVjpParams<T>& sp,
                                 hipStream_t stream) {
  ElementLaunch<T, P> L;
  if (int rc = element_launch<HelmholtzTile<T, P, DIM>>(
          "elasticity_stress_vjp", sp.geo, &L))
    return rc;
  with_geo_mode(sp.geo.geo_mode, [&](auto gm) {
    hipLaunchKernelGGL(
        (elasticity_stress_vjp_kernel<T, P, DIM, decltype(gm)::value>), L.grid,
        L.block, 0, stream, sp, L.dm);
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_elasticity_stress(const ElasticityStressParams<T>& sp, int P,
                               hipStream_t stream);
template <typename T, int DIM>
int dispatch_elasticity_stress_vjp(const ElasticityStressVjpParams<T>& sp,
                                   int P, hipStream_t stream);

#define SFEM_DEFINE_ELASTICITY_STRESS_DISPATCH(TYPE, DIMV)                   \
  template <>                                                                \
  int dispatch_elasticity_stress<TYPE, DIMV>(                                \
      const ElasticityStressParams<TYPE>& sp, int P, hipStream_t stream) {   \
    return with_order<2, 12>("elasticity_stress", P, [&](auto p) {           \
      return launch_elasticity_stress<TYPE, decltype(p)::value, DIMV>(       \
          sp, stream);                                                       \
    });                                                                      \
  }                                                                          \
  template <>                                                                \
  int dispatch_elasticity_stress_vjp<TYPE, DIMV>(                            \
      const ElasticityStressVjpParams<TYPE>& sp, int P,                      \
      hipStream_t stream) {                                                  \
    return with_order<2, 12>("elasticity_stress_vjp", P, [&](auto p) {       \
      return launch_elasticity_stress_vjp<TYPE, decltype(p)::value, DIMV>(   \
          sp, stream);                                                       \
    });                                                                      \
  }

}  // namespace sfem
