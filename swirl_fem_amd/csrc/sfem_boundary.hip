// Boundary integrals over the facets of a physical group (core/fespace.py
// `boundary_points`, `boundary_covector`): each facet is a (d-1)-dimensional
// isoparametric element with its own (P+1)^(d-1) nodes, integrated with the
// space's 1D rule in each facet direction.  B (Q x (P+1)) interpolates the
// nodes to the points, D_q = B D differentiates.
//
// One wave per facet, the facet's values in LDS, one thread per LINE of the
// axis being contracted (the scheme of `tensor_interp_kernel` and the
// p-multigrid transfers).  Accepted: 2 <= P+1 <= 16 and 1 <= Q <= 16.  The 24
// (P+1, Q) pairs the solvers use, Q = P+1 (the GLL rule, a Gauss rule of P+1
// points) and Q = P+2 (the 3D Gauss rule of `solve_poisson`) for P+1 = 2..13,
// are compiled with their sizes fixed; any other pair (Q < P+1, Q > P+2,
// P+1 >= 14) runs the same code with run-time sizes and a register array of
// 16.  Every pair is launched by `tests/test_gpu_boundary_kernels.py`.
//
// sfem_boundary_geom: x_q = (B (x) B) X, the tangents (D_q (x) B) X and
//   (B (x) D_q) X, wJ_q = w_s w_t |x_s x x_t| (3D mesh, 2D facets) or
//   wJ_q = w_s |x_s| (2D mesh, 1D facets).
// sfem_boundary_covector: c_f = (B (x) B)^T (wJ g) with g given at the points,
//   or gathered at the facet nodes and interpolated by B (x) B here.  The
//   element-local c_f are summed per node by sfem_scatter_csr (no atomics).
// sfem_boundary_mass_apply: the facet mass operator of a Robin term,
//   r_f = scale (B (x) B)^T (aw (B (x) B) u_f), u_f gathered through the facet
//   rows; a slot stored as ~id (a Dirichlet node) reads 0 and writes 0.
// sfem_boundary_mass_diag: the facet-local diagonal of the same operator,
//   scale (B.B (x) B.B)^T aw (B.B the entrywise square), same slot rule.
// sfem_boundary_add_rows: out[rows[r]] += the facet-local values of the row's
//   slots, summed in slot order: touches the group's nodes only, no atomics.
#include "sfem_common.h"

namespace sfem {
namespace {

constexpr int BND_MAX_POINTS = 16;

constexpr int bnd_pow(int b, int e) { return e == 0 ? 1 : b * bnd_pow(b, e - 1); }

// One contraction pass: src [pre][ni][post] -> dst [pre][no][post] with
// m (no x ni, row-major).  NI / NO: compile-time sizes, or 0 for run-time.
template <typename T, int NI, int NO>
__device__ __forceinline__ void bnd_contract(const T* __restrict__ src,
                                             T* __restrict__ dst,
                                             const T* __restrict__ m, int ni_rt,
                                             int no_rt, int pre, int post,
                                             int lane) {
  constexpr int NIR = NI ? NI : BND_MAX_POINTS;
  const int ni = NI ? NI : ni_rt;
  const int no = NO ? NO : no_rt;
  const int lines = pre * post;
  for (int l = lane; l < lines; l += 64) {
    const int pi = l / post, qi = l - pi * post;
    const T* x0 = src + pi * ni * post + qi;
    T x[NIR];
#pragma unroll
    for (int i = 0; i < NIR; ++i)
      if (NI || i < ni) x[i] = x0[i * post];
    T* y0 = dst + pi * no * post + qi;
    for (int o = 0; o < no; ++o) {
      T acc = T(0);
#pragma unroll
      for (int i = 0; i < NIR; ++i)
        if (NI || i < ni) acc += m[o * ni + i] * x[i];
      y0[o * post] = acc;
    }
  }
}

// K contractions NI -> NO of a scalar tensor starting in buf0; returns the
// buffer that holds the result.
template <typename T, int K, int NI, int NO>
__device__ __forceinline__ T* bnd_tensor(T* buf0, T* buf1, const T* m, int ni,
                                         int no, int lane) {
  T* src = buf0;
  T* dst = buf1;
  int pre = 1;
  int post = 1;
  for (int a = 1; a < K; ++a) post *= ni;
  for (int a = 0; a < K; ++a) {
    bnd_contract<T, NI, NO>(src, dst, m, ni, no, pre, post, lane);
    __syncthreads();
    pre *= no;
    post /= ni;
    T* t = src;
    src = dst;
    dst = t;
  }
  return src;
}

// K: facet dimension (1 or 2); the mesh has K + 1 coordinates.
template <typename T, int K, int P1, int Q>
__global__ void __launch_bounds__(64)
boundary_geom_kernel(const T* __restrict__ coords,
                     const int32_t* __restrict__ facets,
                     const T* __restrict__ bmat, const T* __restrict__ dmat,
                     const T* __restrict__ weights, T* __restrict__ xq,
                     T* __restrict__ wj, int p1_rt, int q_rt) {
  constexpr int D = K + 1;
  const int p1 = P1 ? P1 : p1_rt;
  const int q = Q ? Q : q_rt;
  const int nf = K == 1 ? p1 : p1 * p1;
  const int nq = K == 1 ? q : q * q;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* b = reinterpret_cast<T*>(smem_raw);           // [q][p1]
  T* d = b + q * p1;                               // [q][p1]
  T* w = d + q * p1;                               // [q]
  T* X = w + q;                                    // [nf][D]
  T* T0 = X + nf * D;                              // [q][p1 or 1][D]
  T* T1 = T0 + q * (K == 1 ? 1 : p1) * D;
  T* XQ = T1 + q * (K == 1 ? 1 : p1) * D;          // K = 2: [q][q][D]
  T* TS = XQ + (K == 1 ? 0 : nq * D);
  T* TT = TS + (K == 1 ? 0 : nq * D);
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  for (int t = lane; t < q * p1; t += 64) {
    b[t] = bmat[t];
    d[t] = dmat[t];
  }
  for (int t = lane; t < q; t += 64) w[t] = weights[t];
  for (int t = lane; t < nf * D; t += 64) {
    const int i = t / D, c = t - i * D;
    X[t] = coords[(int64_t)facets[f * nf + i] * D + c];
  }
  __syncthreads();
  if (K == 1) {
    bnd_contract<T, P1, Q>(X, T0, b, p1, q, 1, D, lane);   // x
    bnd_contract<T, P1, Q>(X, T1, d, p1, q, 1, D, lane);   // dx/ds
    __syncthreads();
    for (int a = lane; a < q; a += 64) {
      T s2 = T(0);
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const T t = T1[a * D + c];
        s2 += t * t;
        xq[(f * nq + a) * D + c] = T0[a * D + c];
      }
      wj[f * nq + a] = w[a] * sqrt(s2);
    }
  } else {
    bnd_contract<T, P1, Q>(X, T0, b, p1, q, 1, p1 * D, lane);
    bnd_contract<T, P1, Q>(X, T1, d, p1, q, 1, p1 * D, lane);
    __syncthreads();
    bnd_contract<T, P1, Q>(T0, XQ, b, p1, q, q, D, lane);  // x
    bnd_contract<T, P1, Q>(T1, TS, b, p1, q, q, D, lane);  // dx/ds
    bnd_contract<T, P1, Q>(T0, TT, d, p1, q, q, D, lane);  // dx/dt
    __syncthreads();
    for (int pt = lane; pt < nq; pt += 64) {
      const int a = pt / q, c = pt - a * q;
      const T* s = TS + pt * D;
      const T* t = TT + pt * D;
      const T n0 = s[1] * t[2] - s[2] * t[1];
      const T n1 = s[2] * t[0] - s[0] * t[2];
      const T n2 = s[0] * t[1] - s[1] * t[0];
#pragma unroll
      for (int k = 0; k < D; ++k) xq[(f * nq + pt) * D + k] = XQ[pt * D + k];
      wj[f * nq + pt] = w[a] * w[c] * sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    }
  }
}

template <typename T, int K, int P1, int Q>
__global__ void __launch_bounds__(64)
boundary_covector_kernel(const T* __restrict__ g, int nodal,
                         const int32_t* __restrict__ facets,
                         const T* __restrict__ wj, const T* __restrict__ bmat,
                         T* __restrict__ out, int p1_rt, int q_rt) {
  const int p1 = P1 ? P1 : p1_rt;
  const int q = Q ? Q : q_rt;
  const int nf = K == 1 ? p1 : p1 * p1;
  const int nq = K == 1 ? q : q * q;
  const int big = p1 > q ? p1 : q;
  const int cap = K == 1 ? big : big * big;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* b = reinterpret_cast<T*>(smem_raw);           // [q][p1]
  T* bt = b + q * p1;                              // [p1][q]
  T* buf0 = bt + q * p1;
  T* buf1 = buf0 + cap;
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  for (int t = lane; t < q * p1; t += 64) {
    const int o = t / q, i = t - o * q;
    b[t] = bmat[t];
    bt[t] = bmat[i * p1 + o];
  }
  T* h;
  if (nodal) {
    for (int t = lane; t < nf; t += 64) buf0[t] = g[facets[f * nf + t]];
    __syncthreads();
    h = bnd_tensor<T, K, P1, Q>(buf0, buf1, b, p1, q, lane);
    for (int t = lane; t < nq; t += 64) h[t] *= wj[f * nq + t];
  } else {
    h = buf0;
    for (int t = lane; t < nq; t += 64) h[t] = g[f * nq + t] * wj[f * nq + t];
  }
  __syncthreads();
  T* other = h == buf0 ? buf1 : buf0;
  const T* res = bnd_tensor<T, K, Q, P1>(h, other, bt, q, p1, lane);
  for (int t = lane; t < nf; t += 64) out[f * nf + t] = res[t];
}

// Robin facet mass: one wave per facet, as boundary_covector_kernel.  diag:
// the transposed pass of B.B on scale aw instead (u unread).
template <typename T, int K, int P1, int Q>
__global__ void __launch_bounds__(64)
boundary_mass_kernel(const T* __restrict__ u,
                     const int32_t* __restrict__ facets,
                     const T* __restrict__ aw, const T* __restrict__ bmat,
                     T scale, int diag, T* __restrict__ out, int p1_rt,
                     int q_rt) {
  const int p1 = P1 ? P1 : p1_rt;
  const int q = Q ? Q : q_rt;
  const int nf = K == 1 ? p1 : p1 * p1;
  const int nq = K == 1 ? q : q * q;
  const int big = p1 > q ? p1 : q;
  const int cap = K == 1 ? big : big * big;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* b = reinterpret_cast<T*>(smem_raw);           // [q][p1]
  T* bt = b + q * p1;                              // [p1][q]
  T* buf0 = bt + q * p1;
  T* buf1 = buf0 + cap;
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  for (int t = lane; t < q * p1; t += 64) {
    const int o = t / q, i = t - o * q;
    const T v = bmat[i * p1 + o];
    b[t] = bmat[t];
    bt[t] = diag ? v * v : v;
  }
  T* h;
  if (diag) {
    h = buf0;
    for (int t = lane; t < nq; t += 64) h[t] = scale * aw[f * nq + t];
  } else {
    for (int t = lane; t < nf; t += 64) {
      const int32_t id = facets[f * nf + t];
      buf0[t] = id >= 0 ? u[id] : T(0);
    }
    __syncthreads();
    h = bnd_tensor<T, K, P1, Q>(buf0, buf1, b, p1, q, lane);
    for (int t = lane; t < nq; t += 64) h[t] *= scale * aw[f * nq + t];
  }
  __syncthreads();
  T* other = h == buf0 ? buf1 : buf0;
  const T* res = bnd_tensor<T, K, Q, P1>(h, other, bt, q, p1, lane);
  for (int t = lane; t < nf; t += 64)
    out[f * nf + t] = facets[f * nf + t] >= 0 ? res[t] : T(0);
}

template <typename T, int K, int P1, int Q>
int launch_mass(const void* u, const int32_t* facets, const void* aw,
                const void* bmat, double scale, int diag, void* out,
                int64_t F, int p1, int q, hipStream_t st) {
  const size_t big = p1 > q ? p1 : q;
  const size_t lds = (2 * (size_t)q * p1 + 2 * bnd_pow((int)big, K)) *
                     sizeof(T);
  if (lds > 64 * 1024) return SFEM_EUNSUPPORTED;
  hipLaunchKernelGGL((boundary_mass_kernel<T, K, P1, Q>), dim3((unsigned)F),
                     dim3(64), lds, st, (const T*)u, facets, (const T*)aw,
                     (const T*)bmat, (T)scale, diag, (T*)out, p1, q);
  return SFEM_OK;
}

// the compiled (P+1, Q) pairs of dispatch_boundary
template <typename T, int K>
int dispatch_mass(const void* u, const int32_t* facets, const void* aw,
                  const void* bmat, double scale, int diag, void* out,
                  int64_t F, int p1, int q, hipStream_t st) {
#define SFEM_MASS_PAIR(N)                                                    \
  if (p1 == N && q == N)                                                     \
    return launch_mass<T, K, N, N>(u, facets, aw, bmat, scale, diag, out, F, \
                                   p1, q, st);                               \
  if (p1 == N && q == N + 1)                                                 \
    return launch_mass<T, K, N, N + 1>(u, facets, aw, bmat, scale, diag,     \
                                       out, F, p1, q, st);
  SFEM_MASS_PAIR(2) SFEM_MASS_PAIR(3) SFEM_MASS_PAIR(4) SFEM_MASS_PAIR(5)
  SFEM_MASS_PAIR(6) SFEM_MASS_PAIR(7) SFEM_MASS_PAIR(8) SFEM_MASS_PAIR(9)
  SFEM_MASS_PAIR(10) SFEM_MASS_PAIR(11) SFEM_MASS_PAIR(12) SFEM_MASS_PAIR(13)
#undef SFEM_MASS_PAIR
  return launch_mass<T, K, 0, 0>(u, facets, aw, bmat, scale, diag, out, F, p1,
                                 q, st);
}

int boundary_mass(const void* u, const int32_t* facets, int64_t F,
                  const void* aw, const void* bmat, int ndim, int p1, int q,
                  double scale, int diag, void* out, int dtype,
                  sfem_stream_t stream) {
  const char* who = diag ? "sfem_boundary_mass_diag"
                         : "sfem_boundary_mass_apply";
  SFEM_REQUIRE(F >= 0 && F <= 0x7fffffff, "%s: bad facet count", who);
  SFEM_REQUIRE(ndim == 2 || ndim == 3, "%s: ndim=%d (2 or 3)", who, ndim);
  SFEM_REQUIRE(p1 >= 2 && p1 <= BND_MAX_POINTS && q >= 1 &&
                   q <= BND_MAX_POINTS,
               "%s: need 2 <= P+1 <= %d and 1 <= Q <= %d, got %d, %d", who,
               BND_MAX_POINTS, BND_MAX_POINTS, p1, q);
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,
               "%s: unknown dtype %d", who, dtype);
  if (F == 0) return SFEM_OK;
  SFEM_REQUIRE(facets && aw && bmat && out && (diag || u),
               "%s: null pointer", who);
  hipStream_t st = as_stream(stream);
  int rc;
  if (dtype == SFEM_F64)
    rc = ndim == 3 ? dispatch_mass<double, 2>(u, facets, aw, bmat, scale, diag,
                                              out, F, p1, q, st)
                   : dispatch_mass<double, 1>(u, facets, aw, bmat, scale, diag,
                                              out, F, p1, q, st);
  else
    rc = ndim == 3 ? dispatch_mass<float, 2>(u, facets, aw, bmat, scale, diag,
                                             out, F, p1, q, st)
                   : dispatch_mass<float, 1>(u, facets, aw, bmat, scale, diag,
                                             out, F, p1, q, st);
  if (rc != SFEM_OK) {
    set_error("%s: P+1=%d, Q=%d, ndim=%d does not fit in LDS", who, p1, q,
              ndim);
    return rc;
  }
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// One thread per listed row: the row's slots summed in order, then added.
template <typename T>
__global__ void __launch_bounds__(256)
boundary_add_rows_kernel(const T* __restrict__ local,
                         const int32_t* __restrict__ rows,
                         const int64_t* __restrict__ offsets,
                         const int32_t* __restrict__ slots,
                         T* __restrict__ out, int64_t num_rows) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rows) return;
  const int64_t s1 = offsets[r + 1];
  T acc = T(0);
  for (int64_t s = offsets[r]; s < s1; ++s) acc += local[slots[s]];
  const int32_t v = rows[r];
  out[v] = out[v] + acc;
}

template <typename T, int K, int P1, int Q>
int launch_boundary(bool covector, const void* in, int nodal,
                    const int32_t* facets, const void* bmat, const void* dmat,
                    const void* weights, const void* wj_in, void* xq, void* wj,
                    int64_t F, int p1, int q, hipStream_t st) {
  constexpr int D = K + 1;
  const size_t nf = bnd_pow(p1, K), nq = bnd_pow(q, K);
  const size_t big = p1 > q ? p1 : q;
  size_t lds;
  if (covector)
    lds = (2 * (size_t)q * p1 + 2 * bnd_pow((int)big, K)) * sizeof(T);
  else
    lds = (2 * (size_t)q * p1 + q + nf * D +
           2 * (size_t)q * (K == 1 ? 1 : p1) * D + (K == 1 ? 0 : 3 * nq * D)) *
          sizeof(T);
  if (lds > 64 * 1024) return SFEM_EUNSUPPORTED;
  const dim3 grid((unsigned)F), block(64);
  if (covector)
    hipLaunchKernelGGL((boundary_covector_kernel<T, K, P1, Q>), grid, block,
                       lds, st, (const T*)in, nodal, facets, (const T*)wj_in,
                       (const T*)bmat, (T*)xq, p1, q);
  else
    hipLaunchKernelGGL((boundary_geom_kernel<T, K, P1, Q>), grid, block, lds,
                       st, (const T*)in, facets, (const T*)bmat,
                       (const T*)dmat, (const T*)weights, (T*)xq, (T*)wj, p1,
                       q);
  return SFEM_OK;
}

// (P+1, Q): Q = P+1 (the GLL rule on the nodes, a Gauss rule of P+1 points)
// and Q = P+2 (the 3D Gauss rule of solve_poisson), P+1 = 2..13.
template <typename T, int K>
int dispatch_boundary(bool covector, const void* in, int nodal,
                      const int32_t* facets, const void* bmat,
                      const void* dmat, const void* weights, const void* wj_in,
                      void* xq, void* wj, int64_t F, int p1, int q,
                      hipStream_t st) {
#define SFEM_BND_PAIR(N)                                                      \
  if (p1 == N && q == N)                                                      \
    return launch_boundary<T, K, N, N>(covector, in, nodal, facets, bmat,     \
                                       dmat, weights, wj_in, xq, wj, F, p1,   \
                                       q, st);                                \
  if (p1 == N && q == N + 1)                                                  \
    return launch_boundary<T, K, N, N + 1>(covector, in, nodal, facets, bmat, \
                                           dmat, weights, wj_in, xq, wj, F,   \
                                           p1, q, st);
  SFEM_BND_PAIR(2) SFEM_BND_PAIR(3) SFEM_BND_PAIR(4) SFEM_BND_PAIR(5)
  SFEM_BND_PAIR(6) SFEM_BND_PAIR(7) SFEM_BND_PAIR(8) SFEM_BND_PAIR(9)
  SFEM_BND_PAIR(10) SFEM_BND_PAIR(11) SFEM_BND_PAIR(12) SFEM_BND_PAIR(13)
#undef SFEM_BND_PAIR
  return launch_boundary<T, K, 0, 0>(covector, in, nodal, facets, bmat, dmat,
                                     weights, wj_in, xq, wj, F, p1, q, st);
}

int boundary(bool covector, const void* in, int nodal, const int32_t* facets,
             const void* bmat, const void* dmat, const void* weights,
             const void* wj_in, void* xq, void* wj, int64_t F, int ndim,
             int p1, int q, int dtype, sfem_stream_t stream) {
  const char* who = covector ? "sfem_boundary_covector" : "sfem_boundary_geom";
  SFEM_REQUIRE(F >= 0 && F <= 0x7fffffff, "%s: bad facet count", who);
  SFEM_REQUIRE(ndim == 2 || ndim == 3, "%s: ndim=%d (2 or 3)", who, ndim);
  SFEM_REQUIRE(p1 >= 2 && p1 <= BND_MAX_POINTS && q >= 1 &&
                   q <= BND_MAX_POINTS,
               "%s: need 2 <= P+1 <= %d and 1 <= Q <= %d, got %d, %d", who,
               BND_MAX_POINTS, BND_MAX_POINTS, p1, q);
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,
               "%s: unknown dtype %d", who, dtype);
  if (F == 0) return SFEM_OK;
  SFEM_REQUIRE(in && facets && bmat && xq &&
                   (covector ? wj_in != nullptr
                             : (dmat && weights && wj)),
               "%s: null pointer", who);
  hipStream_t st = as_stream(stream);
  int rc;
  if (dtype == SFEM_F64)
    rc = ndim == 3 ? dispatch_boundary<double, 2>(covector, in, nodal, facets,
                                                  bmat, dmat, weights, wj_in,
                                                  xq, wj, F, p1, q, st)
                   : dispatch_boundary<double, 1>(covector, in, nodal, facets,
                                                  bmat, dmat, weights, wj_in,
                                                  xq, wj, F, p1, q, st);
  else
    rc = ndim == 3 ? dispatch_boundary<float, 2>(covector, in, nodal, facets,
                                                 bmat, dmat, weights, wj_in,
                                                 xq, wj, F, p1, q, st)
                   : dispatch_boundary<float, 1>(covector, in, nodal, facets,
                                                 bmat, dmat, weights, wj_in,
                                                 xq, wj, F, p1, q, st);
  if (rc != SFEM_OK) {
    set_error("%s: P+1=%d, Q=%d, ndim=%d does not fit in LDS", who, p1, q,
              ndim);
    return rc;
  }
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

}  // namespace
}  // namespace sfem

using namespace sfem;

extern "C" int sfem_boundary_geom(const void* coords, const int32_t* facets,
                                  int64_t num_facets, const void* bmat,
                                  const void* dmat, const void* weights,
                                  int ndim, int p1, int q, void* xq, void* wj,
                                  int dtype, sfem_stream_t stream) {
  return boundary(false, coords, 0, facets, bmat, dmat, weights, nullptr, xq,
                  wj, num_facets, ndim, p1, q, dtype, stream);
}

extern "C" int sfem_boundary_covector(const void* g, int nodal,
                                      const int32_t* facets,
                                      int64_t num_facets, const void* wj,
                                      const void* bmat, int ndim, int p1,
                                      int q, void* out_local, int dtype,
                                      sfem_stream_t stream) {
  return boundary(true, g, nodal, facets, bmat, nullptr, nullptr, wj,
                  out_local, nullptr, num_facets, ndim, p1, q, dtype, stream);
}

extern "C" int sfem_boundary_mass_apply(const void* u, const int32_t* facets,
                                        int64_t num_facets, const void* aw,
                                        const void* bmat, int ndim, int p1,
                                        int q, double scale, void* out_local,
                                        int dtype, sfem_stream_t stream) {
  return boundary_mass(u, facets, num_facets, aw, bmat, ndim, p1, q, scale, 0,
                       out_local, dtype, stream);
}

extern "C" int sfem_boundary_mass_diag(const int32_t* facets,
                                       int64_t num_facets, const void* aw,
                                       const void* bmat, int ndim, int p1,
                                       int q, double scale, void* out_local,
                                       int dtype, sfem_stream_t stream) {
  return boundary_mass(nullptr, facets, num_facets, aw, bmat, ndim, p1, q,
                       scale, 1, out_local, dtype, stream);
}

extern "C" int sfem_boundary_add_rows(const void* local, const int32_t* rows,
                                      const int64_t* offsets,
                                      const int32_t* slots, int64_t num_rows,
                                      void* out, int dtype,
                                      sfem_stream_t stream) {
  SFEM_REQUIRE(num_rows >= 0, "sfem_boundary_add_rows: bad row count");
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,
               "sfem_boundary_add_rows: unknown dtype %d", dtype);
  if (num_rows == 0) return SFEM_OK;
  SFEM_REQUIRE(local && rows && offsets && slots && out,
               "sfem_boundary_add_rows: null pointer");
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((num_rows + 255) / 256)), block(256);
  if (dtype == SFEM_F64)
    hipLaunchKernelGGL(boundary_add_rows_kernel<double>, grid, block, 0, st,
                       (const double*)local, rows, offsets, slots,
                       (double*)out, num_rows);
  else
    hipLaunchKernelGGL(boundary_add_rows_kernel<float>, grid, block, 0, st,
                       (const float*)local, rows, offsets, slots, (float*)out,
                       num_rows);
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}
