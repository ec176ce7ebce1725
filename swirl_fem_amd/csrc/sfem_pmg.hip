// p-multigrid kernels (linalg/pmg.py): transfers between two polynomial
// orders of the same elements, the fused Chebyshev-Jacobi smoother step, and
// the reproducible inner products of the CG that stops on r.r.
//
// Transfers: one wave per element, the element's values in LDS, one thread
// per LINE of the axis being contracted (NI values into registers, NO results
// out, the 1D matrix read as a wave-wide broadcast) -- the scheme of
// `tensor_interp_kernel` (sfem_interp.h).  The (P_c, P_f) pairs of the default
// order schedules are compiled with their sizes fixed; any other pair runs the
// same code with run-time sizes.
//
// P = K_f P_raw K_c:  the coarse values are gathered through the coarse index
// rows (K_c: a Dirichlet node, encoded ~id, reads 0), interpolated, and stored
// at the fine nodes the element OWNS (a per-element bitmask: every fine node
// has exactly one owner, so every fine node is written exactly once, no
// atomics; K_f: a Dirichlet fine node, encoded ~id, gets 0).  The restriction
// P^T gathers the owned fine values (K_f), contracts with the transposed
// matrix and stores the coarse element-local values with the coarse Dirichlet
// slots zeroed (K_c); `sfem_scatter_csr` sums them per node in slot order.
#include "sfem_common.h"
#include "sfem_pmg_tensor.h"

namespace sfem {
namespace {

// u_f = P u_c (ADD: u_f += P u_c).  mat: (pf, pc) row-major.
template <typename T, int D, int PC, int PF, bool ADD>
__global__ void __launch_bounds__(64)
pmg_prolong_kernel(const T* __restrict__ uc, T* __restrict__ uf,
                   const int32_t* __restrict__ cidx,
                   const int32_t* __restrict__ fidx,
                   const uint32_t* __restrict__ owner,
                   const T* __restrict__ mat, int pc_rt, int pf_rt) {
  const int pc = PC ? PC : pc_rt;
  const int pf = PF ? PF : pf_rt;
  int nc = 1, nf = 1;
  for (int a = 0; a < D; ++a) {
    nc *= pc;
    nf *= pf;
  }
  const int cap = nf;
  const int words = (nf + 31) >> 5;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* m = reinterpret_cast<T*>(smem_raw);           // [pf][pc]
  T* buf0 = m + pf * pc;
  T* buf1 = buf0 + cap;
  const int lane = threadIdx.x;
  const int64_t e = blockIdx.x;
  for (int t = lane; t < pf * pc; t += 64) m[t] = mat[t];
  for (int t = lane; t < nc; t += 64) {
    const int32_t k = cidx[e * nc + t];
    buf0[t] = k >= 0 ? uc[k] : T(0);
  }
  __syncthreads();
  const T* res = pmg_tensor<T, D, PC, PF>(buf0, buf1, m, pc, pf, lane);
  for (int t = lane; t < nf; t += 64) {
    if (!pmg_owned(owner, e, words, t)) continue;
    const int32_t k = fidx[e * nf + t];
    if (k >= 0) {
      if (ADD) uf[k] += res[t];
      else uf[k] = res[t];
    } else if (!ADD) {
      uf[~k] = T(0);
    }
  }
}

// rc_local[e] = K_c (J^T (x) .. (x) J^T) (owned K_f r_f)[e]
template <typename T, int D, int PC, int PF>
__global__ void __launch_bounds__(64)
pmg_restrict_kernel(const T* __restrict__ rf, T* __restrict__ rc_local,
                    const int32_t* __restrict__ cidx,
                    const int32_t* __restrict__ fidx,
                    const uint32_t* __restrict__ owner,
                    const T* __restrict__ mat, int pc_rt, int pf_rt) {
  const int pc = PC ? PC : pc_rt;
  const int pf = PF ? PF : pf_rt;
  int nc = 1, nf = 1;
  for (int a = 0; a < D; ++a) {
    nc *= pc;
    nf *= pf;
  }
  const int cap = nf;
  const int words = (nf + 31) >> 5;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* m = reinterpret_cast<T*>(smem_raw);           // [pc][pf] = J^T
  T* buf0 = m + pf * pc;
  T* buf1 = buf0 + cap;
  const int lane = threadIdx.x;
  const int64_t e = blockIdx.x;
  for (int t = lane; t < pf * pc; t += 64) {
    const int o = t / pf, i = t - o * pf;
    m[t] = mat[i * pc + o];
  }
  for (int t = lane; t < nf; t += 64) {
    T v = T(0);
    if (pmg_owned(owner, e, words, t)) {
      const int32_t k = fidx[e * nf + t];
      if (k >= 0) v = rf[k];
    }
    buf0[t] = v;
  }
  __syncthreads();
  const T* res = pmg_tensor<T, D, PF, PC>(buf0, buf1, m, pf, pc, lane);
  for (int t = lane; t < nc; t += 64)
    rc_local[e * nc + t] = cidx[e * nc + t] >= 0 ? res[t] : T(0);
}

template <typename T, int D, int PC, int PF>
int launch_transfer(bool restrict_, bool add, const void* in, void* out,
                    const int32_t* cidx, const int32_t* fidx,
                    const uint32_t* owner, const void* mat, int64_t E, int pc,
                    int pf, hipStream_t st) {
  const size_t lds =
      ((size_t)pf * pc + 2 * (size_t)pmg_pow(pf, D)) * sizeof(T);
  if (lds > 64 * 1024) return SFEM_EUNSUPPORTED;
  const dim3 grid((unsigned)E), block(64);
  if (restrict_)
    hipLaunchKernelGGL((pmg_restrict_kernel<T, D, PC, PF>), grid, block, lds,
                       st, (const T*)in, (T*)out, cidx, fidx, owner,
                       (const T*)mat, pc, pf);
  else if (add)
    hipLaunchKernelGGL((pmg_prolong_kernel<T, D, PC, PF, true>), grid, block,
                       lds, st, (const T*)in, (T*)out, cidx, fidx, owner,
                       (const T*)mat, pc, pf);
  else
    hipLaunchKernelGGL((pmg_prolong_kernel<T, D, PC, PF, false>), grid, block,
                       lds, st, (const T*)in, (T*)out, cidx, fidx, owner,
                       (const T*)mat, pc, pf);
  return SFEM_OK;
}

// (P_c, P_f) in points: the pairs of the default schedules p -> p / 2 for
// fine orders 2..12 (3 -> 2, 4 -> 2, 5 -> 3, 6 -> 3, 7 -> 4, 8 -> 4, 9 -> 5,
// 10 -> 5, 11 -> 6, 12 -> 6, 13 -> 7); anything else: run-time sizes.
template <typename T, int D>
int dispatch_transfer(bool restrict_, bool add, const void* in, void* out,
                      const int32_t* cidx, const int32_t* fidx,
                      const uint32_t* owner, const void* mat, int64_t E,
                      int pc, int pf, hipStream_t st) {
#define SFEM_PMG_PAIR(C, F)                                                  \
  if (pc == C && pf == F)                                                    \
    return launch_transfer<T, D, C, F>(restrict_, add, in, out, cidx, fidx, \
                                       owner, mat, E, pc, pf, st);
  SFEM_PMG_PAIR(2, 3) SFEM_PMG_PAIR(2, 4) SFEM_PMG_PAIR(3, 5)
  SFEM_PMG_PAIR(3, 6) SFEM_PMG_PAIR(4, 7) SFEM_PMG_PAIR(4, 8)
  SFEM_PMG_PAIR(5, 9) SFEM_PMG_PAIR(5, 10) SFEM_PMG_PAIR(6, 11)
  SFEM_PMG_PAIR(6, 12) SFEM_PMG_PAIR(7, 13)
#undef SFEM_PMG_PAIR
  return launch_transfer<T, D, 0, 0>(restrict_, add, in, out, cidx, fidx,
                                     owner, mat, E, pc, pf, st);
}

int transfer(bool restrict_, bool add, const void* in, void* out,
             const int32_t* cidx, const int32_t* fidx, const uint32_t* owner,
             const void* mat, int64_t E, int ndim, int pc, int pf, int dtype,
             sfem_stream_t stream) {
  SFEM_REQUIRE(E >= 0 && E <= 0x7fffffff, "pmg transfer: bad element count");
  SFEM_REQUIRE(ndim == 2 || ndim == 3, "pmg transfer: ndim=%d", ndim);
  SFEM_REQUIRE(pc >= 2 && pf > pc && pf <= PMG_MAX_POINTS,
               "pmg transfer: need 2 <= P_c < P_f <= %d points, got %d, %d",
               PMG_MAX_POINTS, pc, pf);
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,
               "pmg transfer: unknown dtype %d", dtype);
  if (E == 0) return SFEM_OK;
  SFEM_REQUIRE(in && out && cidx && fidx && owner && mat,
               "pmg transfer: null pointer");
  hipStream_t st = as_stream(stream);
  int rc;
  if (dtype == SFEM_F64)
    rc = ndim == 3 ? dispatch_transfer<double, 3>(restrict_, add, in, out,
                                                  cidx, fidx, owner, mat, E,
                                                  pc, pf, st)
                   : dispatch_transfer<double, 2>(restrict_, add, in, out,
                                                  cidx, fidx, owner, mat, E,
                                                  pc, pf, st);
  else
    rc = ndim == 3 ? dispatch_transfer<float, 3>(restrict_, add, in, out,
                                                 cidx, fidx, owner, mat, E,
                                                 pc, pf, st)
                   : dispatch_transfer<float, 2>(restrict_, add, in, out,
                                                 cidx, fidx, owner, mat, E,
                                                 pc, pf, st);
  if (rc != SFEM_OK) {
    set_error("pmg transfer: P_c=%d, P_f=%d, ndim=%d does not fit in LDS", pc,
              pf, ndim);
    return rc;
  }
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// ------------------------------------------------------- Chebyshev step ---
// 16-byte accesses per lane (as the sfem_cg_update_* kernels), the last
// n % VN values by a scalar tail in workgroup 0.
template <typename T>
struct PmgVec;
template <>
struct PmgVec<double> {
  typedef double type __attribute__((ext_vector_type(2)));
  static constexpr int N = 2;
};
template <>
struct PmgVec<float> {
  typedef float type __attribute__((ext_vector_type(4)));
  static constexpr int N = 4;
};

template <typename T, bool NT>
__device__ __forceinline__ typename PmgVec<T>::type pmg_ld(
    const typename PmgVec<T>::type* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}

template <typename T, bool NT>
__device__ __forceinline__ void pmg_st(const typename PmgVec<T>::type& v,
                                       typename PmgVec<T>::type* p) {
  if (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// MODE 0: d = a d + c dinv (b - Ax);  x += d
// MODE 1: d = c dinv b;               x  = d     (x = 0: Ax, x, d not read)
// MODE 2: r = b - Ax                             (residual before restriction)
// MODE 3: d = c dinv (b - Ax);        x += d     (restart: d not read)
template <typename T, int MODE>
__device__ __forceinline__ void cheb_point(T& x, T& d, T ax, T b, T dinv, T& r,
                                           T a, T c) {
  if (MODE == 2) {
    r = b - ax;
  } else if (MODE == 1) {
    d = c * dinv * b;
    x = d;
  } else {
    const T res = b - ax;
    d = (MODE == 0 ? a * d : T(0)) + c * dinv * res;
    x += d;
  }
}

template <typename T, int MODE, bool NT>
__global__ void __launch_bounds__(512)
cheb_step_kernel(T* __restrict__ x, T* __restrict__ d,
                 const T* __restrict__ ax, const T* __restrict__ b,
                 const T* __restrict__ dinv, T* __restrict__ r, T a, T c,
                 int64_t n) {
  using V = typename PmgVec<T>::type;
  constexpr int VN = PmgVec<T>::N;
  constexpr bool RX = MODE == 0 || MODE == 3;     // reads x
  constexpr bool RAX = MODE != 1;                 // reads Ax
  constexpr bool RD = MODE == 0;                  // reads d
  constexpr bool RDINV = MODE != 2;
  const int64_t nvec = n / VN;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += stride) {
    const V bb = pmg_ld<T, NT>(reinterpret_cast<const V*>(b) + i);
    V aa = V(0), xx = V(0), dd = V(0), di = V(0), rr = V(0);
    if (RAX) aa = pmg_ld<T, NT>(reinterpret_cast<const V*>(ax) + i);
    if (RX) xx = pmg_ld<T, NT>(reinterpret_cast<const V*>(x) + i);
    if (RD) dd = pmg_ld<T, NT>(reinterpret_cast<const V*>(d) + i);
    if (RDINV) di = pmg_ld<T, NT>(reinterpret_cast<const V*>(dinv) + i);
#pragma unroll
    for (int k = 0; k < VN; ++k) {
      T xe = xx[k], de = dd[k], re = rr[k];
      cheb_point<T, MODE>(xe, de, aa[k], bb[k], di[k], re, a, c);
      xx[k] = xe;
      dd[k] = de;
      rr[k] = re;
    }
    if (MODE == 2) {
      pmg_st<T, NT>(rr, reinterpret_cast<V*>(r) + i);
    } else {
      pmg_st<T, NT>(xx, reinterpret_cast<V*>(x) + i);
      pmg_st<T, NT>(dd, reinterpret_cast<V*>(d) + i);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < n - nvec * VN) {
    const int64_t i = nvec * VN + threadIdx.x;
    T xe = RX ? x[i] : T(0), de = RD ? d[i] : T(0), re = T(0);
    cheb_point<T, MODE>(xe, de, RAX ? ax[i] : T(0), b[i],
                        RDINV ? dinv[i] : T(0), re, a, c);
    if (MODE == 2) {
      r[i] = re;
    } else {
      x[i] = xe;
      d[i] = de;
    }
  }
}

template <typename T, bool NT>
void launch_cheb(int mode, T* x, T* d, const T* ax, const T* b, const T* dinv,
                 T* r, T a, T c, int64_t n, hipStream_t st) {
  const dim3 grid(stream_grid(n / PmgVec<T>::N + 1, 512)), block(512);
#define SFEM_CHEB_MODE(M)                                                     \
  case M:                                                                     \
    hipLaunchKernelGGL((cheb_step_kernel<T, M, NT>), grid, block, 0, st, x,   \
                       d, ax, b, dinv, r, a, c, n);                           \
    break;
  switch (mode) {
    SFEM_CHEB_MODE(0) SFEM_CHEB_MODE(1) SFEM_CHEB_MODE(2) SFEM_CHEB_MODE(3)
  }
#undef SFEM_CHEB_MODE
}

// ----------------------------------------- reproducible inner products ---
__device__ inline double pmg_block_sum(double v) {
  __shared__ double partial[16];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) partial[wave] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 0; w < nw; ++w) total += partial[w];
  }
  __syncthreads();
  return total;  // valid on thread 0
}

// partials[g] = sum over workgroup g's share of a.b, partials[G + g] of a.c:
// stored, never accumulated, so the sums depend on n and G only.
template <typename T>
__global__ void __launch_bounds__(256)
pmg_dot2_kernel(const T* __restrict__ a, const T* __restrict__ b,
                const T* __restrict__ c, int64_t n,
                double* __restrict__ partials) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double ab = 0.0, ac = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const double av = (double)a[i];
    ab += av * (double)b[i];
    if (c) ac += av * (double)c[i];
  }
  ab = pmg_block_sum(ab);
  if (c) ac = pmg_block_sum(ac);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = ab;
    if (c) partials[gridDim.x + blockIdx.x] = ac;
  }
}

// sum of v[0..n) in a fixed order (valid on thread 0)
__device__ inline double pmg_ordered_sum(const double* __restrict__ v,
                                         int64_t n) {
  double s = 0.0;
  for (int64_t q = threadIdx.x; q < n; q += blockDim.x) s += v[q];
  return pmg_block_sum(s);
}

__device__ __forceinline__ bool pmg_bad_gamma(double g) {
  return !(g >= 0.0) || !(g <= 1.7976931348623157e308);
}

__device__ __forceinline__ bool pmg_bad_pap(double v) {
  return v == 0.0 || !(v >= -1.7976931348623157e308) ||
         !(v <= 1.7976931348623157e308);
}

// The scalar bookkeeping of CG stopping on r.r (see include/sfem.h).
__global__ void __launch_bounds__(256)
pmg_cg_scalars_kernel(double* __restrict__ s, int phase,
                      const double* __restrict__ partials, int64_t n,
                      double maxiter, double tol, double atol) {
  const double first = pmg_ordered_sum(partials, n);
  const double second = (phase == 2 || phase == 4)
                            ? pmg_ordered_sum(partials + n, n) : 0.0;
  if (threadIdx.x != 0) return;
  if (phase == 3) {                  // b.b
    s[5] = first;
    return;
  }
  if (phase == 2) {                  // r.r, r.z of the start; stop rule
    const double a = tol * tol * s[5], b = atol * atol;
    s[6] = a > b ? a : b;
    s[0] = second;
    s[13] = first;
    s[1] = s[2] = s[8] = s[9] = s[11] = s[12] = 0.0;
    for (int q = 0; q < SFEM_CG_RR_SLOTS; ++q)
      s[SFEM_CG_NSCALARS_NAMED + q] = 0.0;
    s[10] = SFEM_CG_STATUS_RUNNING;
    s[7] = 0.0;
    if (pmg_bad_gamma(s[0])) {
      s[10] = SFEM_CG_STATUS_BAD_GAMMA;
      s[7] = 1.0;
    } else if (!(s[13] > s[6])) {
      s[10] = SFEM_CG_STATUS_CONVERGED;
      s[7] = 1.0;
    } else if (maxiter <= 0.0) {
      s[10] = SFEM_CG_STATUS_MAXITER;
      s[7] = 1.0;
    }
    return;
  }
  if (s[7] != 0.0) return;
  if (phase == 0) {                  // p.Ap; alpha
    s[1] = first;
    if (pmg_bad_pap(first)) {
      s[10] = SFEM_CG_STATUS_BAD_PAP;
      s[7] = 1.0;
      return;
    }
    s[3] = s[0] / first;
    s[2] = 0.0;
  } else if (phase == 4) {           // r.r, gamma_new = r.z
    s[13] = first;
    s[2] = second;
  } else if (phase == 1) {           // close the iteration, stop on r.r
    const double g = s[2];
    s[4] = g / s[0];
    s[0] = g;
    s[1] = 0.0;
    s[8] += 1.0;
    if (pmg_bad_gamma(g)) {
      s[10] = SFEM_CG_STATUS_BAD_GAMMA;
      s[7] = 1.0;
    } else if (!(s[13] > s[6])) {
      s[10] = SFEM_CG_STATUS_CONVERGED;
      s[7] = 1.0;
    } else if (s[8] >= maxiter) {
      s[10] = SFEM_CG_STATUS_MAXITER;
      s[7] = 1.0;
    }
  }
}


// ------------------------------------------------------ ELL product ---
// y = A x on some rows of the order-1 matrix in the column-major ELL layout
// of sfem_ell_chebyshev (entry k of row i at [k n + i]): the coarse step of
// the V-cycle on a partition, split into interface and interior rows so that
// the neighbour exchange overlaps the interior rows.  A row range runs VN
// consecutive rows per lane (16-byte loads of the values, 8- / 16-byte loads
// of the columns; a wave covers 128 (fp64) or 256 (fp32) rows); a row list or
// an unaligned range runs one row per lane.  x is gathered through the
// columns (order-1 stencils: the neighbours' values are close in memory).
template <typename T>
struct EllCols;
template <>
struct EllCols<double> {
  typedef int32_t type __attribute__((ext_vector_type(2)));
};
template <>
struct EllCols<float> {
  typedef int32_t type __attribute__((ext_vector_type(4)));
};

template <typename T>
__global__ void __launch_bounds__(256)
ell_spmv_vec_kernel(const int32_t* __restrict__ cols, const T* __restrict__ vals,
                    const T* __restrict__ x, T* __restrict__ y, int64_t n,
                    int width, int64_t row_begin, int64_t nvec) {
  using V = typename PmgVec<T>::type;
  using C = typename EllCols<T>::type;
  constexpr int VN = PmgVec<T>::N;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nvec) return;
  const int64_t i0 = row_begin + t * VN;
  V acc = V(0);
#pragma unroll 4
  for (int k = 0; k < width; ++k) {
    const int64_t at = (int64_t)k * n + i0;
    const C c = *reinterpret_cast<const C*>(cols + at);
    const V v = *reinterpret_cast<const V*>(vals + at);
#pragma unroll
    for (int j = 0; j < VN; ++j) acc[j] += v[j] * x[c[j]];
  }
  *reinterpret_cast<V*>(y + i0) = acc;
}

template <typename T>
__global__ void __launch_bounds__(256)
ell_spmv_row_kernel(const int32_t* __restrict__ cols, const T* __restrict__ vals,
                    const T* __restrict__ x, T* __restrict__ y, int64_t n,
                    int width, int64_t row_begin, const int32_t* __restrict__ rows,
                    int64_t count) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const int64_t i = rows ? (int64_t)rows[t] : row_begin + t;
  T acc = T(0);
#pragma unroll 4
  for (int k = 0; k < width; ++k) {
    const int64_t at = (int64_t)k * n + i;
    acc += vals[at] * x[cols[at]];
  }
  y[i] = acc;
}

template <typename T>
void launch_ell_spmv(const int32_t* cols, const T* vals, const T* x, T* y,
                     int64_t n, int width, int64_t row_begin, int64_t row_end,
                     const int32_t* rows, int64_t num_rows, hipStream_t st) {
  constexpr int VN = PmgVec<T>::N;
  const dim3 block(256);
  if (rows) {
    hipLaunchKernelGGL(ell_spmv_row_kernel<T>,
                       dim3((unsigned)((num_rows + 255) / 256)), block, 0, st,
                       cols, vals, x, y, n, width, (int64_t)0, rows, num_rows);
    return;
  }
  int64_t head = row_begin;
  const bool aligned = n % VN == 0 &&
                       reinterpret_cast<uintptr_t>(vals) % 16 == 0 &&
                       reinterpret_cast<uintptr_t>(cols) % (4 * VN) == 0 &&
                       reinterpret_cast<uintptr_t>(y) % 16 == 0;
  if (aligned) {
    // the unaligned head and the tail of the range run one row per lane
    const int64_t first = (row_begin + VN - 1) / VN * VN;
    const int64_t nvec = first < row_end ? (row_end - first) / VN : 0;
    if (nvec > 0) {
      if (first > row_begin)
        hipLaunchKernelGGL(ell_spmv_row_kernel<T>, dim3(1), block, 0, st,
                           cols, vals, x, y, n, width, row_begin,
                           (const int32_t*)nullptr, first - row_begin);
      hipLaunchKernelGGL(ell_spmv_vec_kernel<T>,
                         dim3((unsigned)((nvec + 255) / 256)), block, 0, st,
                         cols, vals, x, y, n, width, first, nvec);
      head = first + nvec * VN;
    }
  }
  if (row_end > head)
    hipLaunchKernelGGL(ell_spmv_row_kernel<T>,
                       dim3((unsigned)((row_end - head + 255) / 256)), block,
                       0, st, cols, vals, x, y, n, width, head,
                       (const int32_t*)nullptr, row_end - head);
}

}  // namespace
}  // namespace sfem

using namespace sfem;

extern "C" int sfem_pmg_prolong(const void* uc, void* uf, const int32_t* cidx,
                                const int32_t* fidx, const uint32_t* owner,
                                const void* mat, int64_t num_elements,
                                int ndim, int pc, int pf, int add, int dtype,
                                sfem_stream_t stream) {
  return transfer(false, add != 0, uc, uf, cidx, fidx, owner, mat,
                  num_elements, ndim, pc, pf, dtype, stream);
}

extern "C" int sfem_pmg_restrict(const void* rf, void* rc_local,
                                 const int32_t* cidx, const int32_t* fidx,
                                 const uint32_t* owner, const void* mat,
                                 int64_t num_elements, int ndim, int pc,
                                 int pf, int dtype, sfem_stream_t stream) {
  return transfer(true, false, rf, rc_local, cidx, fidx, owner, mat,
                  num_elements, ndim, pc, pf, dtype, stream);
}

extern "C" int sfem_cheb_step(void* x, void* d, const void* ax, const void* b,
                              const void* dinv, void* r, double a, double c,
                              int64_t n, int mode, int dtype,
                              sfem_stream_t stream) {
  SFEM_REQUIRE(n >= 0 && mode >= 0 && mode <= 3,
               "sfem_cheb_step: bad size or mode %d", mode);
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,
               "sfem_cheb_step: unknown dtype %d", dtype);
  if (n == 0) return SFEM_OK;
  SFEM_REQUIRE(b && (mode == 1 || ax) && (mode == 2 ? r != nullptr
                                                    : (x && d && dinv)),
               "sfem_cheb_step: null pointer");
  hipStream_t st = as_stream(stream);
  const size_t es = dtype == SFEM_F64 ? sizeof(double) : sizeof(float);
  const bool nt = streams_past_caches(n, es);
  if (dtype == SFEM_F64) {
    if (nt)
      launch_cheb<double, true>(mode, (double*)x, (double*)d,
                                (const double*)ax, (const double*)b,
                                (const double*)dinv, (double*)r, a, c, n, st);
    else
      launch_cheb<double, false>(mode, (double*)x, (double*)d,
                                 (const double*)ax, (const double*)b,
                                 (const double*)dinv, (double*)r, a, c, n, st);
  } else {
    if (nt)
      launch_cheb<float, true>(mode, (float*)x, (float*)d, (const float*)ax,
                               (const float*)b, (const float*)dinv, (float*)r,
                               (float)a, (float)c, n, st);
    else
      launch_cheb<float, false>(mode, (float*)x, (float*)d, (const float*)ax,
                                (const float*)b, (const float*)dinv,
                                (float*)r, (float)a, (float)c, n, st);
  }
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

extern "C" int sfem_pmg_dot2(const void* a, const void* b, const void* c,
                             int64_t n, double* partials, int groups,
                             int dtype, sfem_stream_t stream) {
  SFEM_REQUIRE(n >= 0 && groups >= 1, "sfem_pmg_dot2: bad sizes");
  SFEM_REQUIRE(a && b && partials, "sfem_pmg_dot2: null pointer");
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,
               "sfem_pmg_dot2: unknown dtype %d", dtype);
  hipStream_t st = as_stream(stream);
  if (dtype == SFEM_F64)
    hipLaunchKernelGGL(pmg_dot2_kernel<double>, dim3(groups), dim3(256), 0, st,
                       (const double*)a, (const double*)b, (const double*)c, n,
                       partials);
  else
    hipLaunchKernelGGL(pmg_dot2_kernel<float>, dim3(groups), dim3(256), 0, st,
                       (const float*)a, (const float*)b, (const float*)c, n,
                       partials);
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

extern "C" int sfem_pmg_cg_scalars(double* scalars, int phase,
                                   const double* partials, int64_t n,
                                   double maxiter, double tol, double atol,
                                   sfem_stream_t stream) {
  SFEM_REQUIRE(scalars && partials && n >= 0 && phase >= 0 && phase <= 4,
               "sfem_pmg_cg_scalars: bad arguments");
  hipLaunchKernelGGL(pmg_cg_scalars_kernel, dim3(1), dim3(256), 0,
                     as_stream(stream), scalars, phase, partials, n, maxiter,
                     tol, atol);
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

extern "C" int sfem_ell_spmv(const int32_t* cols, const void* vals,
                             const void* x, void* y, int64_t n, int width,
                             int64_t row_begin, int64_t row_end,
                             const int32_t* rows, int64_t num_rows, int dtype,
                             sfem_stream_t stream) {
  SFEM_REQUIRE(n >= 0 && width >= 1 && num_rows >= 0 &&
                   (rows || (0 <= row_begin && row_begin <= row_end &&
                             row_end <= n)),
               "sfem_ell_spmv: bad sizes or row range");
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,
               "sfem_ell_spmv: unknown dtype %d", dtype);
  if (rows ? num_rows == 0 : row_end == row_begin) return SFEM_OK;
  SFEM_REQUIRE(cols && vals && x && y, "sfem_ell_spmv: null pointer");
  hipStream_t st = as_stream(stream);
  if (dtype == SFEM_F64)
    launch_ell_spmv<double>(cols, (const double*)vals, (const double*)x,
                            (double*)y, n, width, row_begin, row_end, rows,
                            num_rows, st);
  else
    launch_ell_spmv<float>(cols, (const float*)vals, (const float*)x,
                           (float*)y, n, width, row_begin, row_end, rows,
                           num_rows, st);
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}
