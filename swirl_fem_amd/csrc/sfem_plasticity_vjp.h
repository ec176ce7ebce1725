// Vector-Jacobian product of the radial return of sfem_plasticity.h on the
// collocated grid: the hot path of the path adjoint of a plasticity solve.
// The point map is (eps, eps_p, alpha; lam, mu, sigma_y, Hh) -> (sigma,
// eps_p', alpha').  With the cotangents S of sigma, Pb of eps_p' (symmetric
// 3 x 3 each) and ab of alpha', r32 = sqrt(3/2), e = eps - eps_p, s = 2 mu
// dev(e), sn = |s|, n = s / sn, f = r32 sn - sigma_y - Hh alpha, c = 1 / (3 mu
// + Hh), dg = c f:
//
//   common:   eps_b = lam tr(S) I + 2 mu S;  lam_b = tr(eps) tr(S);
//             Z = Pb - 2 mu S
//   f <= 0:   epsp_b = Z;  alpha_b = ab;  mu_b = 2 (eps - eps_p) : S;
//             sy_b = Hh_b = 0
//   f >  0:   mu_b   = 2 (eps - eps_p') : S
//             dg_b   = ab + r32 (n : Z);      n_b = r32 dg Z
//             f_b    = c dg_b;   mu_b -= 3 c dg dg_b
//             Hh_b   = -c dg dg_b - alpha f_b
//             sy_b   = -f_b;     alpha_b = ab - Hh f_b
//             s_b    = (n_b - (n : n_b) n) / sn + r32 f_b n
//             e_b    = 2 mu dev(s_b);   mu_b += (s : s_b) / mu
//             eps_b += e_b;   epsp_b = Z - e_b
//
// The yield test is a per-lane select, as in the forward kernel: with dg, 1 /
// sn and f_b taken as 0 on the elastic side the plastic expressions reduce to
// the elastic ones, so one sequence serves both, the elastic side never forms
// 1 / sn, and no barrier and no address depends on a data value.
//
// Cotangents of histories refer to the stored arrays (PlasticityLayout): a
// stored off-diagonal slot stands for two tensor entries, so Pb_xy = hbar[xy]
// / 2 on input and hbar_prev[xy] = 2 epsp_b_xy on output; in 2D eps_p,zz =
// -(xx + yy) is implied and eps_p',zz is not stored, so Pb_zz = 0 on input and
// hbar_prev[xx] = epsp_b_xx - epsp_b_zz on output, likewise for yy.
//
// plasticity_vjp_kernel is a sibling of plasticity_kernel: ElemCof, the lane
// mapping and the SFEM_ELAST_* stages of sfem_elasticity.h.  No gather, no
// scatter, no atomics.  It repeats the return mapping from `u` on the grid and
// `hist_in` (null: virgin) and reads nothing that a forward launch left.
//
//   MODE = PLAST_VJP_DISPLACEMENT, out (E, N, DIM) = d(hbar . Phi)/du with Phi
//     the history update: the point VJP with S = 0.  Intake, point stage,
//     fold, output as in the residual mode; the fold takes eps_b / W (no
//     quadrature weight: the history update has none), 0 where W = 0.
//   MODE = PLAST_VJP_STATE, for a second field w on the grid: the point VJP
//     with S = W sym(H_w), Pb and ab from `hbar` (null: zero).  Out, each where
//     non-null: hbar_prev (E, N, NH), the cotangent of hist_in, and dlam, dmu,
//     dyield, dhard (E, N), the derivatives of w . R(u) + hbar . Phi(u) by the
//     point's coefficients; drho = lambda0 W u . w.  No fold.  eps(u) and
//     sym(H_w) are formed one component at a time, as in elasticity_sens_kernel
//     (2 NE P reals per lane, not two DIM x DIM x P line sets).
//
// A point with W = 0 (the all -1 rows of a padded mesh) stores exact zeros in
// every output, whatever its rows of hist_in and hbar hold.  All barriers stay
// outside the `active` / `lane_ok` branches; which outputs are wanted is a
// kernel argument, uniform over the grid.
#pragma once
#include "sfem_plasticity.h"

namespace sfem {

enum { PLAST_VJP_DISPLACEMENT = 0, PLAST_VJP_STATE = 1 };

template <typename T>
struct PlasticityVjpParams {
  ElasticityParams<T> el;   // u, out (displacement mode), wdet, lam / mu and
                            // the geometry; rho unused and lambda0 = 0 there
  const T* w;               // (E, N, DIM); state mode
  const T* yield;           // (E, N) or null = yield_const
  const T* hard;            // (E, N) or null = hard_const
  T yield_const, hard_const;
  const T* hist_in;         // (E, N, NH) or null = virgin
  const T* hbar;            // (E, N, NH); null = zero in the state mode
  T* hbar_prev;             // (E, N, NH) or null; state mode
  T* dlam;                  // (E, N) or null; state mode, as the four below
  T* dmu;
  T* dyield;
  T* dhard;
  T* drho;
  T lambda0;                // of drho
};

// Waves per SIMD asked of the compiler in the state mode.  LIVE_REGS: eps(u)
// and sym(H_w) of the lane's P points plus one component's values, its axis-0
// derivative and a line product.  The displacement mode holds the DIM x DIM x
// P lines of the residual kernel and takes its ElasticityBudget.
template <typename T, int P, int DIM>
struct PlasticityVjpBudget {
  static constexpr int NE = PlasticityLayout<DIM>::NE;
  static constexpr int LIVE_REGS = (2 * NE + 4) * P * (int)sizeof(T) / 4;
  static constexpr int MINW =
      LIVE_REGS > 200 ? 1
                      : (LIVE_REGS > 60 ? 2 : HelmholtzTile<T, P, DIM>::MINW);
  template <int MODE>
  static constexpr int minw() {
    return MODE == PLAST_VJP_STATE ? MINW : ElasticityBudget<T, P, DIM>::MINW;
  }
};

// a : b of two symmetric tensors in the stored slots (off-diagonals twice);
// the zz entries of 2D are the caller's
template <typename T, int DIM>
__device__ __forceinline__ T plast_ddot(
    const T (&a)[PlasticityLayout<DIM>::NE],
    const T (&b)[PlasticityLayout<DIM>::NE]) {
  if constexpr (DIM == 3)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] +
           T(2) * (a[3] * b[3] + a[4] * b[4] + a[5] * b[5]);
  else
    return a[0] * b[0] + a[1] * b[1] + T(2) * a[2] * b[2];
}

// What the point VJP returns: eps_b as tensor entries in the stored slots,
// the cotangent of the stored committed history, and the four coefficient
// derivatives.
template <typename T, int DIM>
struct PlastPointVjp {
  T eps_b[PlasticityLayout<DIM>::NE];
  T hprev[PlasticityLayout<DIM>::NH];
  T lam_b, mu_b, sy_b, hh_b;
};

// The point VJP of the header comment.  ev: eps in the stored slots (2D:
// eps_zz = 0); epv, al: the committed history; Sv: the tensor entries of S in
// the stored slots (2D: S_zz = 0); hb: the cotangent of the stored trial
// history (eps_p' slots, alpha').
template <typename T, int DIM>
__device__ __forceinline__ void plast_point_vjp(
    const T (&ev)[PlasticityLayout<DIM>::NE],
    const T (&epv)[PlasticityLayout<DIM>::NE], T al,
    const T (&Sv)[PlasticityLayout<DIM>::NE],
    const T (&hb)[PlasticityLayout<DIM>::NH], T lq, T mq, T yq, T hq,
    PlastPointVjp<T, DIM>& o) {
  constexpr int NE = PlasticityLayout<DIM>::NE;
  constexpr int XY = DIM == 3 ? 3 : 2;
  constexpr int ND = DIM == 3 ? 3 : 2;   // stored diagonal slots: 0 .. ND - 1
  const T r32 = T(1.2247448713915890491);   // sqrt(3/2)
  const T m2 = T(2) * mq;
  // the forward return mapping, as in plasticity_kernel
  T el[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) el[k] = ev[k] - epv[k];
  T ezz = T(0);
  if constexpr (DIM == 2) ezz = epv[0] + epv[1];
  const T tre = el[0] + el[1] + (DIM == 3 ? el[XY - 1] : ezz);
  const T third = tre * T(1.0 / 3.0);
  T s[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) s[k] = m2 * (k < ND ? el[k] - third : el[k]);
  const T s_zz = DIM == 2 ? m2 * (ezz - third) : T(0);
  const T s2 = plast_ddot<T, DIM>(s, s) + s_zz * s_zz;
  const T sn = plast_sqrt(s2);
  const T f = r32 * sn - (yq + hq * al);
  const bool plastic = f > T(0);
  const T cc = T(1) / (T(3) * mq + hq);
  // the elastic side keeps dg = 0 and never forms 1 / |s|
  const T dg = plastic ? cc * f : T(0);
  const T isn = plastic ? T(1) / sn : T(0);
  T n[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) n[k] = isn * s[k];
  const T n_zz = isn * s_zz;

  // the cotangents as tensors: Pb from the stored slots, Z = Pb - 2 mu S
  T trS = Sv[0] + Sv[1];
  if constexpr (DIM == 3) trS += Sv[2];
  T tr = ev[0] + ev[1];
  if constexpr (DIM == 3) tr += ev[2];
  T Z[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k)
    Z[k] = (k < ND ? hb[k] : T(0.5) * hb[k]) - m2 * Sv[k];
  const T ab = hb[NE];
  o.lam_b = tr * trS;

  const T nZ = plast_ddot<T, DIM>(n, Z);   // Z_zz = 0 in 2D
  const T dg_b = ab + r32 * nZ;
  const T f_b = plastic ? cc * dg_b : T(0);
  const T nnb = r32 * dg * nZ;             // n : n_b with n_b = r32 dg Z
  // s_b = (n_b - (n : n_b) n) / sn + r32 f_b n
  const T along = r32 * f_b - nnb * isn;
  const T across = r32 * dg * isn;
  T sb[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) sb[k] = across * Z[k] + along * n[k];
  const T sb_zz = along * n_zz;
  T trsb = sb[0] + sb[1];
  if constexpr (DIM == 3) trsb += sb[2]; else trsb += sb_zz;
  const T tb3 = trsb * T(1.0 / 3.0);
  // e_b = 2 mu dev(s_b)
  T eb[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) eb[k] = m2 * (k < ND ? sb[k] - tb3 : sb[k]);
  const T eb_zz = DIM == 2 ? m2 * (sb_zz - tb3) : T(0);

  // mu_b = 2 (eps - eps_p') : S - 3 c dg dg_b + (s : s_b) / mu
  T en[NE];
  const T step = r32 * dg;
#pragma unroll
  for (int k = 0; k < NE; ++k) en[k] = el[k] - step * n[k];
  const T ssb = plast_ddot<T, DIM>(s, sb) + s_zz * sb_zz;
  o.mu_b = T(2) * plast_ddot<T, DIM>(en, Sv) - T(3) * cc * dg * dg_b +
           ssb / mq;
  o.hh_b = -cc * dg * dg_b - al * f_b;
  o.sy_b = -f_b;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    o.eps_b[k] = m2 * Sv[k] + (k < ND ? lq * trS : T(0)) + eb[k];
    // epsp_b = Z - e_b, to the stored slots: off-diagonals twice, and in 2D
    // eps_p,zz = -(xx + yy) carries epsp_b_zz = -e_b_zz
    const T pb = Z[k] - eb[k];
    o.hprev[k] = k < ND ? pb + eb_zz : T(2) * pb;
  }
  o.hprev[NE] = ab - hq * f_b;
}

template <typename T, int P, int DIM, int GM, int MODE>
__global__ void __launch_bounds__(
    (HelmholtzTile<T, P, DIM>::BLOCK),
    (PlasticityVjpBudget<T, P, DIM>::template minw<MODE>()))
plasticity_vjp_kernel(PlasticityVjpParams<T> pp, DMat<T, P> dm) {
  SFEM_TILE_PREAMBLE(HelmholtzTile<T, P, DIM>);
  const ElasticityParams<T>& ep = pp.el;
  const StokesParams<T>& prm = ep.geo;
  SFEM_LANE_PROLOGUE(prm);
  using Lay = PlasticityLayout<DIM>;
  constexpr int NE = Lay::NE, NH = Lay::NH;
  constexpr int XY = DIM == 3 ? 3 : 2;
  ElemCof<T, P, DIM, GM> geom;
  geom.init(prm, dm, e, active, i, j, t);
  const T* ue = ep.u + e * N * DIM;
  const T* wd = ep.wdet + e * N;
  const T* lame = ep.lam ? ep.lam + e * N : nullptr;
  const T* mue = ep.mu ? ep.mu + e * N : nullptr;
  const T* yle = pp.yield ? pp.yield + e * N : nullptr;
  const T* hde = pp.hard ? pp.hard + e * N : nullptr;
  const T* hie = pp.hist_in ? pp.hist_in + e * N * NH : nullptr;
  const T* hbe = pp.hbar ? pp.hbar + e * N * NH : nullptr;

  // the committed history and the cotangent of the trial history of point q
  auto load_point = [&](int q, T (&epv)[NE], T& al, T (&hb)[NH]) {
#pragma unroll
    for (int k = 0; k < NE; ++k) epv[k] = T(0);
    al = T(0);
    if (hie) {
      const T* hq_in = hie + (int64_t)q * NH;
#pragma unroll
      for (int k = 0; k < NE; ++k) epv[k] = hq_in[k];
      al = hq_in[NE];
    }
#pragma unroll
    for (int k = 0; k < NH; ++k) hb[k] = T(0);
    if (hbe) {
      const T* hq_b = hbe + (int64_t)q * NH;
#pragma unroll
      for (int k = 0; k < NH; ++k) hb[k] = hq_b[k];
    }
  };

  if constexpr (MODE == PLAST_VJP_DISPLACEMENT) {
    T* oe = ep.out + e * N * DIM;
    // g[c][ax][a]: d u_c / d xi_ax at the lane's point of slice a, then the
    // folded eps_b / W
    T g[DIM][DIM][P];
    SFEM_ELAST_INTAKE();

    if (active) {
#pragma unroll
      for (int a = 0; a < P; ++a) {
        const int q = t + a * TPE;
        T K[DIM * DIM];
        geom.cof(dm, a, K);
        const T wq = wd[q];
        const bool live = wq != T(0);
        const T iw = live ? T(1) / wq : T(0);
        T H[DIM][DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) SFEM_ELAST_GRADIENT(c, a, iw, H);
        T ev[NE];
        ev[0] = H[0][0];
        ev[1] = H[1][1];
        ev[XY] = T(0.5) * (H[0][1] + H[1][0]);
        if constexpr (DIM == 3) {
          ev[2] = H[2][2];
          ev[4] = T(0.5) * (H[0][2] + H[2][0]);
          ev[5] = T(0.5) * (H[1][2] + H[2][1]);
        }
        T epv[NE], al, hb[NH], Sv[NE];
        load_point(q, epv, al, hb);
#pragma unroll
        for (int k = 0; k < NE; ++k) Sv[k] = T(0);
        PlastPointVjp<T, DIM> o;
        plast_point_vjp<T, DIM>(ev, epv, al, Sv, hb,
                                lame ? lame[q] : ep.lam_const,
                                mue ? mue[q] : ep.mu_const,
                                yle ? yle[q] : pp.yield_const,
                                hde ? hde[q] : pp.hard_const, o);
        // eps_b / W, an exact zero where W = 0 whatever the rows hold
        T sg[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) sg[k] = live ? iw * o.eps_b[k] : T(0);
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          T S[DIM];
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

    SFEM_ELAST_OUTPUT();   // ep.lambda0 = 0: no mass term
  } else {
    const T* we = pp.w + e * N * DIM;
    // eu[k][a], sw[k][a]: eps(u) and sym(H_w) in the stored slots at the
    // lane's point of slice a
    T eu[NE][P] = {}, sw[NE][P] = {};
    auto derivatives = [&](const T (&x)[P], T (&dx0)[P]) {
      SFEM_ELAST_DERIVATIVES(x, dx0);
    };
    auto gradient_row = [&](int a, T g0, T (&h)[DIM]) {
      SFEM_ELAST_GRADIENT_ROW(a, g0, h);
    };
#pragma unroll
    for (int fld = 0; fld < 2; ++fld) {
      const T* xe = fld == 0 ? ue : we;
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        T xa[P], g0[P];
#pragma unroll
        for (int a = 0; a < P; ++a)
          xa[a] = active ? xe[(int64_t)(t + a * TPE) * DIM + c] : T(0);
        derivatives(xa, g0);
        if (active) {
#pragma unroll
          for (int a = 0; a < P; ++a) {
            T h[DIM];
            gradient_row(a, g0[a], h);
#pragma unroll
            for (int jj = 0; jj < DIM; ++jj) {
              const int k = jj == c ? c : (DIM == 3 ? c + jj + 2 : 2);
              const T v = jj == c ? h[jj] : T(0.5) * h[jj];
              if (fld == 0)
                eu[k][a] += v;
              else
                sw[k][a] += v;
            }
          }
        }
        __syncthreads();   // the next component overwrites the tensor pair
      }
    }

    if (active) {
      T* hpe = pp.hbar_prev ? pp.hbar_prev + e * N * NH : nullptr;
      T* lout = pp.dlam ? pp.dlam + e * N : nullptr;
      T* mout = pp.dmu ? pp.dmu + e * N : nullptr;
      T* yout = pp.dyield ? pp.dyield + e * N : nullptr;
      T* hout = pp.dhard ? pp.dhard + e * N : nullptr;
      T* rout = pp.drho ? pp.drho + e * N : nullptr;
#pragma unroll
      for (int a = 0; a < P; ++a) {
        const int q = t + a * TPE;
        const T wq = wd[q];
        const bool live = wq != T(0);
        T ev[NE], Sv[NE], epv[NE], al, hb[NH];
#pragma unroll
        for (int k = 0; k < NE; ++k) {
          ev[k] = eu[k][a];
          Sv[k] = wq * sw[k][a];
        }
        load_point(q, epv, al, hb);
        PlastPointVjp<T, DIM> o;
        plast_point_vjp<T, DIM>(ev, epv, al, Sv, hb,
                                lame ? lame[q] : ep.lam_const,
                                mue ? mue[q] : ep.mu_const,
                                yle ? yle[q] : pp.yield_const,
                                hde ? hde[q] : pp.hard_const, o);
        if (hpe) {
          T* ho = hpe + (int64_t)q * NH;
#pragma unroll
          for (int k = 0; k < NH; ++k) ho[k] = live ? o.hprev[k] : T(0);
        }
        if (lout) lout[q] = live ? o.lam_b : T(0);
        if (mout) mout[q] = live ? o.mu_b : T(0);
        if (yout) yout[q] = live ? o.sy_b : T(0);
        if (hout) hout[q] = live ? o.hh_b : T(0);
        if (rout) {
          T sdot = T(0);
#pragma unroll
          for (int c = 0; c < DIM; ++c)
            sdot += ue[(int64_t)q * DIM + c] * we[(int64_t)q * DIM + c];
          rout[q] = live ? pp.lambda0 * wq * sdot : T(0);
        }
      }
    }
  }
}

template <typename T, int P, int DIM>
int launch_plasticity_vjp(const PlasticityVjpParams<T>& pp, int mode,
                          hipStream_t stream) {
  static_assert(PLAST_VJP_STATE == 1, "mode 1 of launch_two_mode");
  return launch_two_mode<T, P, DIM>(
      "plasticity_vjp", pp, mode, stream, [](auto gm, auto state) {
        return plasticity_vjp_kernel<T, P, DIM, decltype(gm)::value,
                                     decltype(state)::value>;
      });
}

// Defined once per (dtype, ndim) translation unit, P = 2..12.
template <typename T, int DIM>
int dispatch_plasticity_vjp(const PlasticityVjpParams<T>& pp, int P, int mode,
                            hipStream_t stream);

#define SFEM_DEFINE_PLASTICITY_VJP_DISPATCH(TYPE, DIMV)                      \
  template <>                                                                \
  int dispatch_plasticity_vjp<TYPE, DIMV>(                                   \
      const PlasticityVjpParams<TYPE>& pp, int P, int mode,                  \
      hipStream_t stream) {                                                  \
    return with_order<2, 12>("plasticity_vjp", P, [&](auto p) {              \
      return launch_plasticity_vjp<TYPE, decltype(p)::value, DIMV>(pp, mode, \
                                                                   stream);  \
    });                                                                      \
  }

}  // namespace sfem
