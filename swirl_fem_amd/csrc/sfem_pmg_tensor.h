// The tensor contraction of the p-multigrid transfers, shared by the scalar
// kernels (sfem_pmg.hip) and the vector ones (sfem_pmg_vec.hip): the element's
// values in LDS, one thread per LINE of the axis being contracted (NI values
// into registers, NO results out, the 1D matrix read as a wave-wide
// broadcast) -- the scheme of `tensor_interp_kernel` (sfem_interp.h).
#pragma once
#include "sfem_common.h"

namespace sfem {
namespace {

constexpr int PMG_MAX_POINTS = 13;

constexpr int pmg_pow(int b, int e) { return e == 0 ? 1 : b * pmg_pow(b, e - 1); }

// One contraction pass: src [pre][ni][post] -> dst [pre][no][post] with
// m (no x ni, row-major).  NI / NO: compile-time sizes, or 0 for run-time.
template <typename T, int NI, int NO>
__device__ __forceinline__ void pmg_contract(const T* __restrict__ src,
                                             T* __restrict__ dst,
                                             const T* __restrict__ m, int ni_rt,
                                             int no_rt, int pre, int post,
                                             int lane) {
  constexpr int NIR = NI ? NI : PMG_MAX_POINTS;
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

// D contractions NI -> NO starting in buf[0]; returns the buffer holding the
// result.
template <typename T, int D, int NI, int NO>
__device__ __forceinline__ T* pmg_tensor(T* buf0, T* buf1, const T* m,
                                         int ni, int no, int lane) {
  T* src = buf0;
  T* dst = buf1;
  int pre = 1;
  int post = 1;
  for (int a = 1; a < D; ++a) post *= ni;
  for (int a = 0; a < D; ++a) {
    pmg_contract<T, NI, NO>(src, dst, m, ni, no, pre, post, lane);
    __syncthreads();
    pre *= no;
    post /= ni;
    T* t = src;
    src = dst;
    dst = t;
  }
  return src;
}

__device__ __forceinline__ bool pmg_owned(const uint32_t* __restrict__ owner,
                                          int64_t e, int words, int t) {
  return (owner[e * words + (t >> 5)] >> (t & 31)) & 1u;
}

}  // namespace
}  // namespace sfem
