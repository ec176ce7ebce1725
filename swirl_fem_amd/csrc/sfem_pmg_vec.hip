// p-multigrid transfers of nodal VECTOR fields (linalg/pmg_elasticity.py):
// D components per node, dense (N, D) -- the flat (N D,) vectors of the
// elasticity solve -- between two polynomial orders of the same elements.
//
// The scheme is that of the scalar kernels (sfem_pmg.hip): one wave per
// element, the element's values in LDS, one lane per line of the axis being
// contracted (`pmg_tensor`, sfem_pmg_tensor.h), the default (P_c, P_f) pairs
// compiled with their sizes fixed.  What differs:
// * fixed components are per COMPONENT, not per node (a roller fixes one, a
//   clamp all), so the index rows are plain ids and the flags travel as one
//   byte per coarse node and one per fine node, bit c set when component c
//   is fixed;
// * the D components go one after another through the same two LDS buffers
//   (all at once would not fit: 13^3 points x 3 components x 2 buffers in
//   fp64 is 105 KB), inside one launch: the matrix is loaded once, and the
//   index rows, owner words and flag bytes of an element come from memory
//   once and from cache for the other components, where D scalar launches
//   on component strips read them D times and need the strips copied.
//
// P = K_f P_raw K_c per component: a fixed coarse component reads 0, every
// fine node is written once, at the element that OWNS it (no atomics), a
// fixed fine component gets 0 (store) or is left alone (add).  The
// restriction gathers the owned, non-fixed fine values and stores the coarse
// element-local values (E, n_c, D) with the fixed coarse slots zeroed;
// `sfem_scatter_csr` (ncomp = D) sums them per node in slot order.
#include "sfem_common.h"
#include "sfem_pmg_tensor.h"

namespace sfem {
namespace {

__device__ __forceinline__ bool pmg_fixed(const uint8_t* __restrict__ flags,
                                          int32_t k, int c) {
  return (flags[k] >> c) & 1u;
}

// u_f = P u_c (ADD: u_f += P u_c).  mat: (pf, pc) row-major.
template <typename T, int D, int PC, int PF, bool ADD>
__global__ void __launch_bounds__(64)
pmg_prolong_vec_kernel(const T* __restrict__ uc, T* __restrict__ uf,
                       const int32_t* __restrict__ cidx,
                       const int32_t* __restrict__ fidx,
                       const uint32_t* __restrict__ owner,
                       const uint8_t* __restrict__ cfix,
                       const uint8_t* __restrict__ ffix,
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
  for (int c = 0; c < D; ++c) {
    for (int t = lane; t < nc; t += 64) {
      const int32_t k = cidx[e * nc + t];
      buf0[t] = pmg_fixed(cfix, k, c) ? T(0) : uc[(int64_t)k * D + c];
    }
    __syncthreads();
    const T* res = pmg_tensor<T, D, PC, PF>(buf0, buf1, m, pc, pf, lane);
    for (int t = lane; t < nf; t += 64) {
      if (!pmg_owned(owner, e, words, t)) continue;
      const int32_t k = fidx[e * nf + t];
      T* dst = uf + (int64_t)k * D + c;
      if (!pmg_fixed(ffix, k, c)) {
        if (ADD) *dst += res[t];
        else *dst = res[t];
      } else if (!ADD) {
        *dst = T(0);
      }
    }
    // the next component's gather overwrites the buffer `res` lives in
    __syncthreads();
  }
}

// rc_local[e] = K_c (J^T (x) .. (x) J^T) (owned K_f r_f)[e], per component
template <typename T, int D, int PC, int PF>
__global__ void __launch_bounds__(64)
pmg_restrict_vec_kernel(const T* __restrict__ rf, T* __restrict__ rc_local,
                        const int32_t* __restrict__ cidx,
                        const int32_t* __restrict__ fidx,
                        const uint32_t* __restrict__ owner,
                        const uint8_t* __restrict__ cfix,
                        const uint8_t* __restrict__ ffix,
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
  for (int c = 0; c < D; ++c) {
    for (int t = lane; t < nf; t += 64) {
      T v = T(0);
      if (pmg_owned(owner, e, words, t)) {
        const int32_t k = fidx[e * nf + t];
        if (!pmg_fixed(ffix, k, c)) v = rf[(int64_t)k * D + c];
      }
      buf0[t] = v;
    }
    __syncthreads();
    const T* res = pmg_tensor<T, D, PF, PC>(buf0, buf1, m, pf, pc, lane);
    for (int t = lane; t < nc; t += 64) {
      const int32_t k = cidx[e * nc + t];
      rc_local[(e * nc + t) * D + c] = pmg_fixed(cfix, k, c) ? T(0) : res[t];
    }
    __syncthreads();
  }
}

template <typename T, int D, int PC, int PF>
int launch_transfer_vec(bool restrict_, bool add, const void* in, void* out,
                        const int32_t* cidx, const int32_t* fidx,
                        const uint32_t* owner, const uint8_t* cfix,
                        const uint8_t* ffix, const void* mat, int64_t E,
                        int pc, int pf, hipStream_t st) {
  const size_t lds =
      ((size_t)pf * pc + 2 * (size_t)pmg_pow(pf, D)) * sizeof(T);
  if (lds > 64 * 1024) return SFEM_EUNSUPPORTED;
  const dim3 grid((unsigned)E), block(64);
  if (restrict_)
    hipLaunchKernelGGL((pmg_restrict_vec_kernel<T, D, PC, PF>), grid, block,
                       lds, st, (const T*)in, (T*)out, cidx, fidx, owner, cfix,
                       ffix, (const T*)mat, pc, pf);
  else if (add)
    hipLaunchKernelGGL((pmg_prolong_vec_kernel<T, D, PC, PF, true>), grid,
                       block, lds, st, (const T*)in, (T*)out, cidx, fidx,
                       owner, cfix, ffix, (const T*)mat, pc, pf);
  else
    hipLaunchKernelGGL((pmg_prolong_vec_kernel<T, D, PC, PF, false>), grid,
                       block, lds, st, (const T*)in, (T*)out, cidx, fidx,
                       owner, cfix, ffix, (const T*)mat, pc, pf);
  return SFEM_OK;
}

// the (P_c, P_f) pairs of `dispatch_transfer` (sfem_pmg.hip)
template <typename T, int D>
int dispatch_transfer_vec(bool restrict_, bool add, const void* in, void* out,
                          const int32_t* cidx, const int32_t* fidx,
                          const uint32_t* owner, const uint8_t* cfix,
                          const uint8_t* ffix, const void* mat, int64_t E,
                          int pc, int pf, hipStream_t st) {
#define SFEM_PMG_PAIR(C, F)                                                  \
  if (pc == C && pf == F)                                                    \
    return launch_transfer_vec<T, D, C, F>(restrict_, add, in, out, cidx,   \
                                           fidx, owner, cfix, ffix, mat, E, \
                                           pc, pf, st);
  SFEM_PMG_PAIR(2, 3) SFEM_PMG_PAIR(2, 4) SFEM_PMG_PAIR(3, 5)
  SFEM_PMG_PAIR(3, 6) SFEM_PMG_PAIR(4, 7) SFEM_PMG_PAIR(4, 8)
  SFEM_PMG_PAIR(5, 9) SFEM_PMG_PAIR(5, 10) SFEM_PMG_PAIR(6, 11)
  SFEM_PMG_PAIR(6, 12) SFEM_PMG_PAIR(7, 13)
#undef SFEM_PMG_PAIR
  return launch_transfer_vec<T, D, 0, 0>(restrict_, add, in, out, cidx, fidx,
                                         owner, cfix, ffix, mat, E, pc, pf,
                                         st);
}

int transfer_vec(bool restrict_, bool add, const void* in, void* out,
                 const int32_t* cidx, const int32_t* fidx,
                 const uint32_t* owner, const uint8_t* cfix,
                 const uint8_t* ffix, const void* mat, int64_t E, int ndim,
                 int pc, int pf, int dtype, sfem_stream_t stream) {
  SFEM_REQUIRE(E >= 0 && E <= 0x7fffffff,
               "pmg vector transfer: bad element count");
  SFEM_REQUIRE(ndim == 2 || ndim == 3, "pmg vector transfer: ndim=%d", ndim);
  SFEM_REQUIRE(pc >= 2 && pf > pc && pf <= PMG_MAX_POINTS,
               "pmg vector transfer: need 2 <= P_c < P_f <= %d points, got "
               "%d, %d", PMG_MAX_POINTS, pc, pf);
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,
               "pmg vector transfer: unknown dtype %d", dtype);
  if (E == 0) return SFEM_OK;
  SFEM_REQUIRE(in && out && cidx && fidx && owner && cfix && ffix && mat,
               "pmg vector transfer: null pointer");
  hipStream_t st = as_stream(stream);
  int rc;
  if (dtype == SFEM_F64)
    rc = ndim == 3
             ? dispatch_transfer_vec<double, 3>(restrict_, add, in, out, cidx,
                                                fidx, owner, cfix, ffix, mat,
                                                E, pc, pf, st)
             : dispatch_transfer_vec<double, 2>(restrict_, add, in, out, cidx,
                                                fidx, owner, cfix, ffix, mat,
                                                E, pc, pf, st);
  else
    rc = ndim == 3
             ? dispatch_transfer_vec<float, 3>(restrict_, add, in, out, cidx,
                                               fidx, owner, cfix, ffix, mat,
                                               E, pc, pf, st)
             : dispatch_transfer_vec<float, 2>(restrict_, add, in, out, cidx,
                                               fidx, owner, cfix, ffix, mat,
                                               E, pc, pf, st);
  if (rc != SFEM_OK) {
    set_error("pmg vector transfer: P_c=%d, P_f=%d, ndim=%d does not fit in "
              "LDS", pc, pf, ndim);
    return rc;
  }
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

}  // namespace
}  // namespace sfem

using namespace sfem;

extern "C" int sfem_pmg_prolong_vec(const void* uc, void* uf,
                                    const int32_t* cidx, const int32_t* fidx,
                                    const uint32_t* owner,
                                    const uint8_t* cfix, const uint8_t* ffix,
                                    const void* mat, int64_t num_elements,
                                    int ndim, int pc, int pf, int add,
                                    int dtype, sfem_stream_t stream) {
  return transfer_vec(false, add != 0, uc, uf, cidx, fidx, owner, cfix, ffix,
                      mat, num_elements, ndim, pc, pf, dtype, stream);
}

extern "C" int sfem_pmg_restrict_vec(const void* rf, void* rc_local,
                                     const int32_t* cidx, const int32_t* fidx,
                                     const uint32_t* owner,
                                     const uint8_t* cfix, const uint8_t* ffix,
                                     const void* mat, int64_t num_elements,
                                     int ndim, int pc, int pf, int dtype,
                                     sfem_stream_t stream) {
  return transfer_vec(true, false, rf, rc_local, cidx, fidx, owner, cfix, ffix,
                      mat, num_elements, ndim, pc, pf, dtype, stream);
}
