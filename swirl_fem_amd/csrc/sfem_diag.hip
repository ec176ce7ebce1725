// Element diagonals of the Helmholtz operator (sfem_helmholtz_diag): the
// Jacobi preconditioner's setup kernel.
//
// For the operator  lambda0 B_e + lambda1 A_e  that sfem_helmholtz_apply /
// sfem_helmholtz_local apply, with the same geometric factors
// G = w detJ J^-1 J^-T and W = w detJ from the same sources (stored per point,
// or evaluated from the multilinear map of the element), node i = (i0, i1, i2)
// (axis 0 slowest) of an element has
//   diag(B_e)_i = sum_q W(q) prod_c B(q_c, i_c)^2
//   diag(A_e)_i = sum_q sum_ab G_ab(q) g_a(q) g_b(q),
//                 g_a = prod_c (c == a ? Dt(q_c, i_c) : B(q_c, i_c))
// with B the (Q, P) interpolation from the nodes to the quadrature points and
// Dt = D_q B its derivative.  The two parts come out separately, so one launch
// serves every (lambda0, lambda1).
//
// Collocated spaces (B = I, the fused operator) reduce to the points that
// share all but one coordinate with the node:
//   diag(B_e)_i = W(i)
//   diag(A_e)_i = sum_a sum_k G_aa(i; i_a -> k) D(k, i_a)^2
//               + 2 sum_{a<b} G_ab(i) D(i_a, i_a) D(i_b, i_b)
// -- d P + 1 geometry evaluations per node, O(P^(d+1)) per element.  The
// general form (two-grid operator) is a direct sum over the Q^d points per
// node.  One thread per (element, node); this runs once per operator.

#include "sfem_common.h"

namespace sfem {
namespace {

constexpr int GEO_POINT = 0, GEO_AFFINE = 1, GEO_MULTILINEAR = 3;

template <typename T>
struct DiagParams {
  T* mass_out;
  T* stiff_out;
  const T* geo;
  const T* geo_elem;
  const int32_t* geo_index;
  const int32_t* elem_list;
  const T* bmat;     // (Q, P) or null (collocated)
  const T* dtil;     // (Q, P)
  const T* weights;  // (Q,)
  const T* nodes;    // (Q,)
  int64_t num_listed;
  int P, Q, geo_mode;
  const T* kappa;    // coefficients (coef_mode SFEM_COEF_*), or null = 1
  const T* sigma;
  int coef_mode;
};

template <typename T, int DIM>
__device__ void geo_factors(const DiagParams<T>& prm, int64_t e,
                            int64_t slot, int q0, int q1, int q2,
                            bool want_g, T (&g)[3][3], T& W);

// G (upper triangle in g[a][b], a <= b) and W at point (q0, q1, q2), G scaled
// by the diffusivity k and W by the reaction coefficient c of the point.
template <typename T, int DIM>
__device__ void point_factors(const DiagParams<T>& prm, int64_t e,
                              int64_t slot, int q0, int q1, int q2,
                              bool want_g, T (&g)[3][3], T& W) {
  geo_factors<T, DIM>(prm, e, slot, q0, q1, q2, want_g, g, W);
  if (prm.coef_mode == SFEM_COEF_NONE) return;
  int64_t at = e;
  if (prm.coef_mode == SFEM_COEF_POINT) {
    const int Q = prm.Q;
    const int64_t NQ = DIM == 3 ? (int64_t)Q * Q * Q : (int64_t)Q * Q;
    at = e * NQ + (DIM == 3 ? ((int64_t)q0 * Q + q1) * Q + q2
                            : (int64_t)q0 * Q + q1);
  }
  if (prm.sigma) W *= prm.sigma[at];
  if (want_g && prm.kappa) {
    const T k = prm.kappa[at];
    for (int a = 0; a < DIM; ++a)
      for (int b = a; b < DIM; ++b) g[a][b] *= k;
  }
}

template <typename T, int DIM>
__device__ void geo_factors(const DiagParams<T>& prm, int64_t e,
                            int64_t slot, int q0, int q1, int q2,
                            bool want_g, T (&g)[3][3], T& W) {
  const int Q = prm.Q;
  if (prm.geo_mode == GEO_POINT) {
    const int64_t NQ = DIM == 3 ? (int64_t)Q * Q * Q : (int64_t)Q * Q;
    const int64_t q = DIM == 3 ? ((int64_t)q0 * Q + q1) * Q + q2
                               : (int64_t)q0 * Q + q1;
    const T* b = prm.geo + slot * (int64_t)(DIM == 3 ? 7 : 4) * NQ;
    // pairs (G00, G01) (G02, G11) (G12, G22), then W;  2D: (G00, G01) (G11, W)
    if (DIM == 3) {
      g[0][0] = b[q * 2];           g[0][1] = b[q * 2 + 1];
      g[0][2] = b[(NQ + q) * 2];    g[1][1] = b[(NQ + q) * 2 + 1];
      g[1][2] = b[(2 * NQ + q) * 2]; g[2][2] = b[(2 * NQ + q) * 2 + 1];
      W = b[6 * NQ + q];
    } else {
      g[0][0] = b[q * 2];        g[0][1] = b[q * 2 + 1];
      g[1][1] = b[(NQ + q) * 2]; W = b[(NQ + q) * 2 + 1];
    }
    return;
  }
  const T* A = prm.geo_elem + e * 24;
  const T* x = prm.nodes;
  const T* w = prm.weights;
  if (DIM == 3) {
    const T r = x[q0], s = x[q1], t = x[q2];
    const T wq = w[q0] * w[q1] * w[q2];
    T R0[3], R1[3], R2[3];
    for (int c = 0; c < 3; ++c) {
      const T A1 = A[c], A2 = A[3 + c], A3 = A[6 + c], A4 = A[9 + c],
              A5 = A[12 + c], A6 = A[15 + c], A7 = A[18 + c];
      R0[c] = A1 + A4 * s + (A6 + A7 * s) * t;
      R1[c] = (A2 + A5 * t) + r * (A4 + A7 * t);
      R2[c] = (A3 + A5 * s) + r * (A6 + A7 * s);
    }
    const T c0[3] = {R1[1] * R2[2] - R1[2] * R2[1],
                     R1[2] * R2[0] - R1[0] * R2[2],
                     R1[0] * R2[1] - R1[1] * R2[0]};
    const T det = R0[0] * c0[0] + R0[1] * c0[1] + R0[2] * c0[2];
    W = wq * det;
    if (!want_g) return;
    const T c1[3] = {R2[1] * R0[2] - R2[2] * R0[1],
                     R2[2] * R0[0] - R2[0] * R0[2],
                     R2[0] * R0[1] - R2[1] * R0[0]};
    const T c2[3] = {R0[1] * R1[2] - R0[2] * R1[1],
                     R0[2] * R1[0] - R0[0] * R1[2],
                     R0[0] * R1[1] - R0[1] * R1[0]};
    const T* cc[3] = {c0, c1, c2};
    const T sc = wq / det;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b)
        g[a][b] = sc * (cc[a][0] * cc[b][0] + cc[a][1] * cc[b][1] +
                        cc[a][2] * cc[b][2]);
  } else {
    const T r = x[q0], s = x[q1];
    const T wq = w[q0] * w[q1];
    T R0[2], R1[2];
    for (int c = 0; c < 2; ++c) {
      R0[c] = A[c] + A[4 + c] * s;        // d/dr
      R1[c] = A[2 + c] + r * A[4 + c];    // d/ds
    }
    const T det = R0[0] * R1[1] - R0[1] * R1[0];
    W = wq * det;
    if (!want_g) return;
    const T sc = wq / det;
    g[0][0] = sc * (R1[1] * R1[1] + R1[0] * R1[0]);
    g[0][1] = -sc * (R1[1] * R0[1] + R1[0] * R0[0]);
    g[1][1] = sc * (R0[1] * R0[1] + R0[0] * R0[0]);
  }
}

template <typename T, int DIM>
__global__ void __launch_bounds__(256)
helmholtz_diag_kernel(DiagParams<T> prm) {
  const int P = prm.P, Q = prm.Q;
  const int n = DIM == 3 ? P * P * P : P * P;
  const int64_t total = prm.num_listed * n;
  const bool want_m = prm.mass_out != nullptr;
  const bool want_a = prm.stiff_out != nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int64_t k = t / n;
    const int li = (int)(t - k * n);
    const int64_t e = prm.elem_list ? (int64_t)prm.elem_list[k] : k;
    const int64_t slot =
        prm.geo_mode == GEO_POINT && prm.geo_index ? prm.geo_index[e] : e;
    int ii[3] = {0, 0, 0};
    if (DIM == 3) {
      ii[0] = li / (P * P); ii[1] = (li / P) % P; ii[2] = li % P;
    } else {
      ii[0] = li / P; ii[1] = li % P;
    }
    T m = T(0), s = T(0);
    T g[3][3] = {};
    T W;
    if (prm.bmat == nullptr) {
      // collocated: node i is quadrature point i
      point_factors<T, DIM>(prm, e, slot, ii[0], ii[1], ii[2], want_a, g, W);
      m = W;
      if (want_a) {
        const T dd[3] = {prm.dtil[ii[0] * P + ii[0]], prm.dtil[ii[1] * P + ii[1]],
                         DIM == 3 ? prm.dtil[ii[2] * P + ii[2]] : T(0)};
        for (int a = 0; a < DIM; ++a)
          for (int b = a + 1; b < DIM; ++b)
            s += T(2) * g[a][b] * dd[a] * dd[b];
        for (int a = 0; a < DIM; ++a) {
          for (int kk = 0; kk < P; ++kk) {
            int q[3] = {ii[0], ii[1], ii[2]};
            q[a] = kk;
            T ga[3][3] = {};
            T Wa;
            point_factors<T, DIM>(prm, e, slot, q[0], q[1], q[2], true, ga, Wa);
            const T dk = prm.dtil[kk * P + ii[a]];
            s += ga[a][a] * dk * dk;
          }
        }
      }
    } else {
      const int q2n = DIM == 3 ? Q : 1;
      for (int q0 = 0; q0 < Q; ++q0) {
        const T b0 = prm.bmat[q0 * P + ii[0]], d0 = prm.dtil[q0 * P + ii[0]];
        for (int q1 = 0; q1 < Q; ++q1) {
          const T b1 = prm.bmat[q1 * P + ii[1]], d1 = prm.dtil[q1 * P + ii[1]];
          for (int q2 = 0; q2 < q2n; ++q2) {
            const T b2 = DIM == 3 ? prm.bmat[q2 * P + ii[2]] : T(1);
            const T d2 = DIM == 3 ? prm.dtil[q2 * P + ii[2]] : T(0);
            point_factors<T, DIM>(prm, e, slot, q0, q1, q2, want_a, g, W);
            const T bb = b0 * b1 * b2;
            m += W * bb * bb;
            if (want_a) {
              const T gv[3] = {d0 * b1 * b2, b0 * d1 * b2, b0 * b1 * d2};
              for (int a = 0; a < DIM; ++a) {
                s += g[a][a] * gv[a] * gv[a];
                for (int b = a + 1; b < DIM; ++b)
                  s += T(2) * g[a][b] * gv[a] * gv[b];
              }
            }
          }
        }
      }
    }
    if (want_m) prm.mass_out[e * n + li] = m;
    if (want_a) prm.stiff_out[e * n + li] = s;
  }
}

template <typename T>
int launch_diag(const sfem_diag_args* a, hipStream_t stream) {
  DiagParams<T> prm;
  prm.mass_out = (T*)a->mass_out;
  prm.stiff_out = (T*)a->stiff_out;
  prm.geo = (const T*)a->geo;
  prm.geo_elem = (const T*)a->geo_elem;
  prm.geo_index = a->geo_index;
  prm.elem_list = a->elem_list;
  prm.bmat = (const T*)a->bmat;
  prm.dtil = (const T*)a->dtil;
  prm.weights = (const T*)a->weights;
  prm.nodes = (const T*)a->nodes;
  prm.num_listed = a->elem_list ? a->num_listed : a->num_elements;
  prm.P = a->P;
  prm.Q = a->bmat ? a->Q : a->P;
  prm.geo_mode = a->geo_mode;
  prm.kappa = (const T*)a->kappa;
  prm.sigma = (const T*)a->sigma;
  prm.coef_mode = a->coef_mode;
  const int n = a->ndim == 3 ? a->P * a->P * a->P : a->P * a->P;
  const unsigned grid = stream_grid(prm.num_listed * n, 256);
  if (a->ndim == 3)
    hipLaunchKernelGGL((helmholtz_diag_kernel<T, 3>), dim3(grid), dim3(256), 0,
                       stream, prm);
  else
    hipLaunchKernelGGL((helmholtz_diag_kernel<T, 2>), dim3(grid), dim3(256), 0,
                       stream, prm);
  return SFEM_OK;
}

}  // namespace
}  // namespace sfem

using namespace sfem;

extern "C" {

int sfem_helmholtz_diag(const sfem_diag_args* a, sfem_stream_t stream) {
  SFEM_REQUIRE(a, "sfem_helmholtz_diag: null arguments");
  SFEM_REQUIRE(a->ndim == 2 || a->ndim == 3,
               "sfem_helmholtz_diag: ndim = %d (2 or 3)", a->ndim);
  SFEM_REQUIRE(a->P >= 2 && a->P <= 12,
               "sfem_helmholtz_diag: P = %d outside 2..12", a->P);
  SFEM_REQUIRE(a->bmat == nullptr || (a->Q >= a->P && a->Q <= 16),
               "sfem_helmholtz_diag: Q = %d outside P..16", a->Q);
  SFEM_REQUIRE(a->num_elements >= 0 && a->num_listed >= 0,
               "sfem_helmholtz_diag: negative sizes");
  SFEM_REQUIRE(a->mass_out || a->stiff_out,
               "sfem_helmholtz_diag: no output requested");
  SFEM_REQUIRE(a->dtil && a->weights,
               "sfem_helmholtz_diag: null 1D matrices");
  SFEM_REQUIRE(a->geo_mode == GEO_POINT || a->geo_mode == GEO_AFFINE ||
                   a->geo_mode == GEO_MULTILINEAR,
               "sfem_helmholtz_diag: geometry mode %d (stored, affine or "
               "multilinear)", a->geo_mode);
  SFEM_REQUIRE(a->geo_mode == GEO_POINT ? a->geo != nullptr
                                        : (a->geo_elem && a->nodes),
               "sfem_helmholtz_diag: missing geometry");
  SFEM_REQUIRE(a->coef_mode == SFEM_COEF_NONE ||
                   a->coef_mode == SFEM_COEF_ELEM ||
                   a->coef_mode == SFEM_COEF_POINT,
               "sfem_helmholtz_diag: unknown coef_mode %d", a->coef_mode);
  SFEM_REQUIRE(a->coef_mode == SFEM_COEF_NONE || a->kappa || a->sigma,
               "sfem_helmholtz_diag: coef_mode %d needs kappa or sigma",
               a->coef_mode);
  if ((a->elem_list ? a->num_listed : a->num_elements) == 0) return SFEM_OK;
  int rc;
  if (a->dtype == SFEM_F64)
    rc = launch_diag<double>(a, as_stream(stream));
  else if (a->dtype == SFEM_F32)
    rc = launch_diag<float>(a, as_stream(stream));
  else
    SFEM_REQUIRE(false, "sfem_helmholtz_diag: unknown dtype %d", a->dtype);
  if (rc != SFEM_OK) return rc;
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

}  // extern "C"
