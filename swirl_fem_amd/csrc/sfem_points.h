// Fields at arbitrary points: evaluation at located points and
// its transpose.  The locator, which is setup and not templated, lives in
// sfem_points.hip.
//
// A point p in element e with reference coordinates xi sees
//   u(xi) = sum_n u[elements[e, n]] l_n(xi),   l_n = l_i(xi_0) l_j(xi_1) ...
// with the 1D Lagrange polynomials in the product form
//   l_i(x) = bary[i] prod_{k != i} (x - nodes[k]),
// finite at the nodes.  Both kernels are templated on the scalar type, the
// dimension and P1 = points per direction, so the DIM x P1 basis values of a
// point live in registers and every loop over them unrolls.
//
//   point_eval_kernel    one wave per chunk of at most 64 points of one
//                        element; the element's nodal values of a component
//                        are staged in LDS through the index row, lane = point
//                        contracts sum-factorised (every lane reads the same
//                        LDS word at the same time: broadcasts).
//   point_eval_t_kernel  one workgroup per touched element; lanes over points
//                        stage a chunk's basis values and weights in LDS,
//                        lanes over nodes accumulate them in point order into
//                        one element-local row.  No atomics: a call is
//                        bitwise reproducible.
// Barriers sit in loops whose trip counts are uniform over the workgroup.
#pragma once
#include "sfem_launch.h"

namespace sfem {

constexpr int POINT_CHUNK = SFEM_POINT_CHUNK;
constexpr int POINT_T_BLOCK = 256;

template <typename T, int P1>
struct PointBasis {
  T x[P1];   // 1D nodes
  T w[P1];   // 1 / prod_{k != i} (x[i] - x[k])
};

template <typename T, int P1>
inline PointBasis<T, P1> make_point_basis(const double* nodes,
                                          const double* bary) {
  PointBasis<T, P1> pb;
  for (int i = 0; i < P1; ++i) {
    pb.x[i] = (T)nodes[i];
    pb.w[i] = (T)bary[i];
  }
  return pb;
}

template <typename T>
struct PointParams {
  const T* field;
  T* values;
  T* rows;
  const int32_t* elements;
  const T* xi;
  const int64_t* perm;
  const int32_t* chunk_elem;
  const int64_t* chunk_start;
  const int32_t* chunk_count;
  const int32_t* seg_elem;
  const int64_t* seg_offsets;
  int64_t num_chunks, num_segments;
  int64_t node_stride, comp_stride;
  int ncomp;
};

// l[i] = w[i] prod_{k != i} (x - x[k]), all P1 of them
template <typename T, int P1>
__device__ __forceinline__ void lagrange_values(const PointBasis<T, P1>& pb,
                                                T x, T (&l)[P1]) {
  T d[P1];
#pragma unroll
  for (int k = 0; k < P1; ++k) d[k] = x - pb.x[k];
#pragma unroll
  for (int i = 0; i < P1; ++i) {
    T v = pb.w[i];
#pragma unroll
    for (int k = 0; k < P1; ++k)
      if (k != i) v *= d[k];
    l[i] = v;
  }
}

template <typename T, int DIM, int P1>
__global__ void __launch_bounds__(POINT_CHUNK)
point_eval_kernel(PointParams<T> pp, PointBasis<T, P1> pb) {
  constexpr int N = DIM == 3 ? P1 * P1 * P1 : P1 * P1;
  __shared__ T us[N];
  const int lane = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int64_t e = pp.chunk_elem[chunk];
  const int count = pp.chunk_count[chunk];
  const bool active = lane < count;
  const int64_t p = pp.chunk_start[chunk] + (active ? lane : 0);
  const int32_t* row = pp.elements + e * N;

  // axes 1.. in registers; in 3D axis 0 is walked by a rolled loop that forms
  // l_i(xi_0) from the differences d0 (a run-time index into a register
  // array would go to scratch, P1 unrolled planes hold too many LDS reads
  // in flight: float at P1 >= 9 took 256 VGPRs)
  T lb[DIM][P1];
#pragma unroll
  for (int a = DIM == 3 ? 1 : 0; a < DIM; ++a)
    lagrange_values<T, P1>(pb, pp.xi[p * DIM + a], lb[a]);
  T d0[P1];
#pragma unroll
  for (int k = 0; k < P1; ++k) d0[k] = pp.xi[p * DIM] - pb.x[k];
  const int64_t dst = pp.perm[p] * pp.ncomp;

#pragma unroll 1
  for (int c = 0; c < pp.ncomp; ++c) {
    __syncthreads();            // the previous component has been read
    for (int q = lane; q < N; q += POINT_CHUNK) {
      const int32_t k = row[q];
      us[q] = k >= 0 ? pp.field[(int64_t)k * pp.node_stride +
                                (int64_t)c * pp.comp_stride]
                     : T(0);
    }
    __syncthreads();
    T r = T(0);
    if (DIM == 3) {
#pragma unroll 1
      for (int i = 0; i < P1; ++i) {
        T l0 = T(1);            // w[i] prod_{k != i} d0[k]
#pragma unroll
        for (int k = 0; k < P1; ++k) l0 *= k == i ? pb.w[k] : d0[k];
        const T* plane = us + i * P1 * P1;
        T s = T(0);
#pragma unroll
        for (int j = 0; j < P1; ++j) {
          T t = T(0);
#pragma unroll
          for (int k = 0; k < P1; ++k) t += plane[j * P1 + k] * lb[DIM - 1][k];
          s += t * lb[1][j];
        }
        r += s * l0;
      }
    } else {
#pragma unroll
      for (int i = 0; i < P1; ++i) {
        T t = T(0);
#pragma unroll
        for (int k = 0; k < P1; ++k) t += us[i * P1 + k] * lb[1][k];
        r += t * lb[0][i];
      }
    }
    if (active) pp.values[dst + c] = r;
  }
}

template <typename T, int DIM, int P1>
__global__ void __launch_bounds__(POINT_T_BLOCK)
point_eval_t_kernel(PointParams<T> pp, PointBasis<T, P1> pb) {
  constexpr int N = DIM == 3 ? P1 * P1 * P1 : P1 * P1;
  constexpr int KN = (N + POINT_T_BLOCK - 1) / POINT_T_BLOCK;
  constexpr int LW = DIM * P1;          // basis words per point
  __shared__ T bas[POINT_CHUNK * LW];
  __shared__ T wgt[POINT_CHUNK];
  const int tid = threadIdx.x;
  const int64_t seg = blockIdx.x;
  const int64_t begin = pp.seg_offsets[seg], end = pp.seg_offsets[seg + 1];

  // node q = tid + m * BLOCK has the 1D indices (i, j, k), axis 0 slowest
  int o0[KN], o1[KN], o2[KN];
#pragma unroll
  for (int m = 0; m < KN; ++m) {
    const int q = tid + m * POINT_T_BLOCK;
    const int qq = q < N ? q : 0;
    if (DIM == 3) {
      o0[m] = qq / (P1 * P1);
      o1[m] = P1 + (qq / P1) % P1;
      o2[m] = 2 * P1 + qq % P1;
    } else {
      o0[m] = qq / P1;
      o1[m] = P1 + qq % P1;
      o2[m] = 0;
    }
  }

#pragma unroll 1
  for (int c = 0; c < pp.ncomp; ++c) {
    T acc[KN];
#pragma unroll
    for (int m = 0; m < KN; ++m) acc[m] = T(0);
#pragma unroll 1
    for (int64_t base = begin; base < end; base += POINT_CHUNK) {
      const int count =
          (int)(end - base < POINT_CHUNK ? end - base : (int64_t)POINT_CHUNK);
      __syncthreads();          // the previous chunk has been read
      if (tid < count) {
        const int64_t p = base + tid;
        T l[P1];
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          lagrange_values<T, P1>(pb, pp.xi[p * DIM + a], l);
#pragma unroll
          for (int i = 0; i < P1; ++i) bas[tid * LW + a * P1 + i] = l[i];
        }
        wgt[tid] = pp.values[pp.perm[p] * pp.ncomp + c];
      }
      __syncthreads();
#pragma unroll 1
      for (int t = 0; t < count; ++t) {
        const T* b = bas + t * LW;
        const T w = wgt[t];
#pragma unroll
        for (int m = 0; m < KN; ++m) {
          T v = w * b[o0[m]] * b[o1[m]];
          if (DIM == 3) v *= b[o2[m]];
          acc[m] += v;
        }
      }
    }
    T* out = pp.rows + seg * N * pp.ncomp;
#pragma unroll
    for (int m = 0; m < KN; ++m) {
      const int q = tid + m * POINT_T_BLOCK;
      if (q < N) out[(int64_t)q * pp.ncomp + c] = acc[m];
    }
  }
}

template <typename T, int DIM, int P1>
int launch_point_eval(const PointParams<T>& pp, const double* nodes,
                      const double* bary, bool transpose, hipStream_t stream) {
  const PointBasis<T, P1> pb = make_point_basis<T, P1>(nodes, bary);
  if (transpose) {
    hipLaunchKernelGGL((point_eval_t_kernel<T, DIM, P1>),
                       dim3((unsigned)pp.num_segments), dim3(POINT_T_BLOCK), 0,
                       stream, pp, pb);
  } else {
    hipLaunchKernelGGL((point_eval_kernel<T, DIM, P1>),
                       dim3((unsigned)pp.num_chunks), dim3(POINT_CHUNK), 0,
                       stream, pp, pb);
  }
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

// Defined once per (dtype, ndim) translation unit, P1 = 2..12.
template <typename T, int DIM>
int dispatch_point_eval(const PointParams<T>& pp, int P1, const double* nodes,
                        const double* bary, bool transpose,
                        hipStream_t stream);

#define SFEM_DEFINE_POINT_DISPATCH(TYPE, DIMV)                               \
  template <>                                                                \
  int dispatch_point_eval<TYPE, DIMV>(                                       \
      const PointParams<TYPE>& pp, int P1, const double* nodes,              \
      const double* bary, bool transpose, hipStream_t stream) {              \
    return with_order<2, 12>("point_eval", P1, [&](auto p) {                 \
      return launch_point_eval<TYPE, DIMV, decltype(p)::value>(              \
          pp, nodes, bary, transpose, stream);                               \
    });                                                                      \
  }

}  // namespace sfem
