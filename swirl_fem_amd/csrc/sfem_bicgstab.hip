// Right-preconditioned BiCGStab: the fused vector kernels and scalar phases
// behind linalg/bicgstab.py (include/sfem.h, "BiCGStab").  As in the CG core
// every scalar of the recurrence lives in a small device array that the
// kernels read, so an iteration needs no host synchronisation; once `done` is
// raised every kernel and every phase returns at once.
#include "sfem_common.h"

namespace sfem {

enum {
  BS_RHO = 0, BS_RHO_NEW = 1, BS_ALPHA = 2, BS_OMEGA = 3, BS_BETA = 4,
  BS_R0V = 5, BS_SS = 6, BS_TS = 7, BS_TT = 8, BS_RR = 9, BS_BB = 10,
  BS_THRESHOLD = 11, BS_DONE = 12, BS_ITERS = 13, BS_STATUS = 14,
  BS_HALF = 15, BS_RESIDUAL = 16
};

__device__ __forceinline__ double bs_block_sum(double v) {
  __shared__ double part[8];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();               // `part` may still be read by an earlier sum
  if ((threadIdx.x & 63) == 0) part[wave] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += part[w];
  return total;                  // valid in thread 0
}

__device__ __forceinline__ bool bs_finite(double v) {
  return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308;
}

// omega = t.s / t.t; 0 after a half-step stop and when t.t is zero or the
// quotient is not finite (the closing phase then reports the breakdown)
__device__ __forceinline__ double bs_omega(const double* scalars) {
  if (scalars[BS_HALF] != 0.0) return 0.0;
  const double tt = scalars[BS_TT];
  if (!(tt > 0.0)) return 0.0;
  const double w = scalars[BS_TS] / tt;
  return bs_finite(w) ? w : 0.0;
}

// slot[0] += a.b  (slot[1] += a.a when TWO)
template <typename T, bool TWO>
__global__ void __launch_bounds__(512)
bicgstab_dot_kernel(const T* __restrict__ a, const T* __restrict__ b,
                    int64_t count, double* __restrict__ scalars, int slot,
                    int skip_on_half) {
  if (scalars[BS_DONE] != 0.0) return;
  if (skip_on_half && scalars[BS_HALF] != 0.0) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double ab = 0.0, aa = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += stride) {
    const double x = (double)a[i];
    ab += x * (double)b[i];
    if (TWO) aa += x * x;
  }
  const double s0 = bs_block_sum(ab);
  if (threadIdx.x == 0) unsafeAtomicAdd(&scalars[slot], s0);
  if (TWO) {
    const double s1 = bs_block_sum(aa);
    if (threadIdx.x == 0) unsafeAtomicAdd(&scalars[slot + 1], s1);
  }
}

// 1.  p = r + beta (p - omega v);  phat = dinv p  (dinv null: phat is p)
template <typename T>
__global__ void __launch_bounds__(512)
bicgstab_update_p_kernel(T* __restrict__ p, T* __restrict__ phat,
                         const T* __restrict__ r, const T* __restrict__ v,
                         const T* __restrict__ dinv, int64_t count,
                         const double* __restrict__ scalars) {
  if (scalars[BS_DONE] != 0.0) return;
  const T beta = (T)scalars[BS_BETA], omega = (T)scalars[BS_OMEGA];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += stride) {
    const T pn = r[i] + beta * (p[i] - omega * v[i]);
    p[i] = pn;
    if (dinv) phat[i] = dinv[i] * pn;
  }
}

// 2.  s = r - alpha v;  shat = dinv s;  scalars[SS] += s.s
template <typename T>
__global__ void __launch_bounds__(512)
bicgstab_update_s_kernel(T* __restrict__ s, T* __restrict__ shat,
                         const T* __restrict__ r, const T* __restrict__ v,
                         const T* __restrict__ dinv, int64_t count,
                         double* __restrict__ scalars) {
  if (scalars[BS_DONE] != 0.0) return;
  const T alpha = (T)scalars[BS_ALPHA];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += stride) {
    const T sn = r[i] - alpha * v[i];
    s[i] = sn;
    if (dinv) shat[i] = dinv[i] * sn;
    acc += (double)sn * (double)sn;
  }
  const double total = bs_block_sum(acc);
  if (threadIdx.x == 0) unsafeAtomicAdd(&scalars[BS_SS], total);
}

// 4.  x += alpha phat + omega shat;  r = s - omega t;
//     scalars[RR] += r.r, scalars[RHO_NEW] += r0.r
template <typename T>
__global__ void __launch_bounds__(512)
bicgstab_update_xr_kernel(T* __restrict__ x, T* __restrict__ r,
                          const T* __restrict__ phat,
                          const T* __restrict__ shat, const T* __restrict__ s,
                          const T* __restrict__ t, const T* __restrict__ r0,
                          int64_t count, double* __restrict__ scalars) {
  if (scalars[BS_DONE] != 0.0) return;
  const T alpha = (T)scalars[BS_ALPHA];
  const T omega = (T)bs_omega(scalars);
  const bool half = omega == T(0);     // t may never have been written
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double rr = 0.0, rho = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += stride) {
    T xn = x[i] + alpha * phat[i];
    T rn = s[i];
    if (!half) {
      xn += omega * shat[i];
      rn -= omega * t[i];
    }
    x[i] = xn;
    r[i] = rn;
    rr += (double)rn * (double)rn;
    rho += (double)r0[i] * (double)rn;
  }
  const double a = bs_block_sum(rr);
  if (threadIdx.x == 0) unsafeAtomicAdd(&scalars[BS_RR], a);
  const double b = bs_block_sum(rho);
  if (threadIdx.x == 0) unsafeAtomicAdd(&scalars[BS_RHO_NEW], b);
}

__device__ __forceinline__ void bs_stop(double* scalars, double status) {
  scalars[BS_STATUS] = status;
  scalars[BS_DONE] = 1.0;
}

// One thread.  phase 0: start (BB, RR, RHO_NEW hold b.b, r.r, r0.r);
// 1: alpha from r0.v;  2: the half-step test on s.s;  3: closes the iteration.
__global__ void bicgstab_scalars_kernel(double* __restrict__ scalars, int phase,
                                        double maxiter, double tol,
                                        double atol) {
  if (phase != 0 && scalars[BS_DONE] != 0.0) return;
  if (phase == 0) {
    const double t2 = tol * tol * scalars[BS_BB], a2 = atol * atol;
    scalars[BS_THRESHOLD] = t2 > a2 ? t2 : a2;
    scalars[BS_RHO] = scalars[BS_RHO_NEW];
    scalars[BS_RHO_NEW] = 0.0;
    scalars[BS_ALPHA] = 1.0;
    scalars[BS_OMEGA] = 1.0;
    scalars[BS_BETA] = 0.0;
    scalars[BS_R0V] = 0.0; scalars[BS_SS] = 0.0;
    scalars[BS_TS] = 0.0; scalars[BS_TT] = 0.0;
    scalars[BS_RESIDUAL] = scalars[BS_RR];
    scalars[BS_DONE] = 0.0;
    scalars[BS_ITERS] = 0.0;
    scalars[BS_STATUS] = SFEM_BICGSTAB_STATUS_RUNNING;
    scalars[BS_HALF] = 0.0;
    const double rr = scalars[BS_RR], rho = scalars[BS_RHO];
    if (!(rr > scalars[BS_THRESHOLD]) && bs_finite(rr))
      bs_stop(scalars, SFEM_BICGSTAB_STATUS_CONVERGED);
    else if (rho == 0.0 || !bs_finite(rho))
      bs_stop(scalars, SFEM_BICGSTAB_STATUS_BAD_RHO);
    else if (maxiter <= 0.0)
      bs_stop(scalars, SFEM_BICGSTAB_STATUS_MAXITER);
  } else if (phase == 1) {
    const double r0v = scalars[BS_R0V];
    const double alpha = scalars[BS_RHO] / r0v;
    if (r0v == 0.0 || !bs_finite(alpha)) {
      bs_stop(scalars, SFEM_BICGSTAB_STATUS_BAD_ALPHA);
      return;
    }
    scalars[BS_ALPHA] = alpha;
    scalars[BS_SS] = 0.0;
  } else if (phase == 2) {
    const double ss = scalars[BS_SS];
    scalars[BS_HALF] = (!(ss > scalars[BS_THRESHOLD]) && bs_finite(ss)) ? 1.0
                                                                        : 0.0;
    scalars[BS_TS] = 0.0; scalars[BS_TT] = 0.0;
    scalars[BS_RR] = 0.0; scalars[BS_RHO_NEW] = 0.0;
  } else {
    const double omega = bs_omega(scalars);
    const double rr = scalars[BS_RR], rho_new = scalars[BS_RHO_NEW];
    const bool half = scalars[BS_HALF] != 0.0;
    scalars[BS_OMEGA] = omega;
    scalars[BS_RESIDUAL] = rr;
    scalars[BS_ITERS] += 1.0;
    scalars[BS_R0V] = 0.0;
    if (!bs_finite(rr)) {
      bs_stop(scalars, half || omega != 0.0 ? SFEM_BICGSTAB_STATUS_BAD_RHO
                                            : SFEM_BICGSTAB_STATUS_BAD_OMEGA);
    } else if (!(rr > scalars[BS_THRESHOLD])) {
      bs_stop(scalars, SFEM_BICGSTAB_STATUS_CONVERGED);
    } else if (omega == 0.0) {
      bs_stop(scalars, SFEM_BICGSTAB_STATUS_BAD_OMEGA);
    } else if (rho_new == 0.0 || !bs_finite(rho_new)) {
      bs_stop(scalars, SFEM_BICGSTAB_STATUS_BAD_RHO);
    } else if (scalars[BS_ITERS] >= maxiter) {
      bs_stop(scalars, SFEM_BICGSTAB_STATUS_MAXITER);
    } else {
      scalars[BS_BETA] = (rho_new / scalars[BS_RHO]) *
                         (scalars[BS_ALPHA] / omega);
      scalars[BS_RHO] = rho_new;
    }
  }
}

}  // namespace sfem

using namespace sfem;

#define SFEM_BS_DTYPE(who)                                                \
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64,                    \
               who ": unknown dtype %d", dtype)

extern "C" {

int sfem_bicgstab_scalars(double* scalars, int phase, double maxiter,
                          double tol, double atol, sfem_stream_t stream) {
  SFEM_REQUIRE(scalars && phase >= 0 && phase <= 3,
               "sfem_bicgstab_scalars: bad arguments");
  hipLaunchKernelGGL(bicgstab_scalars_kernel, dim3(1), dim3(1), 0,
                     as_stream(stream), scalars, phase, maxiter, tol, atol);
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

int sfem_bicgstab_dot(const void* a, const void* b, int64_t count,
                      double* scalars, int slot, int two, int dtype,
                      sfem_stream_t stream) {
  SFEM_REQUIRE(count >= 0 && scalars, "sfem_bicgstab_dot: bad arguments");
  SFEM_REQUIRE(slot >= 0 && slot + (two ? 1 : 0) < SFEM_BICGSTAB_NSCALARS,
               "sfem_bicgstab_dot: slot %d outside the scalar array", slot);
  SFEM_BS_DTYPE("sfem_bicgstab_dot");
  if (count == 0) return SFEM_OK;
  SFEM_REQUIRE(a && b, "sfem_bicgstab_dot: null pointer");
  const dim3 grid(reduce_grid(count, 512 * 4)), block(512);
  hipStream_t st = as_stream(stream);
  // the (t.s, t.t) pass is skipped after a half-step stop: t was not formed
  const int skip = two ? 1 : 0;
#define SFEM_BS_DOT(T, TWO)                                                  \
  hipLaunchKernelGGL((bicgstab_dot_kernel<T, TWO>), grid, block, 0, st,      \
                     (const T*)a, (const T*)b, count, scalars, slot, skip)
  if (dtype == SFEM_F64) { if (two) SFEM_BS_DOT(double, true); else SFEM_BS_DOT(double, false); }
  else { if (two) SFEM_BS_DOT(float, true); else SFEM_BS_DOT(float, false); }
#undef SFEM_BS_DOT
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

int sfem_bicgstab_update_p(void* p, void* phat, const void* r, const void* v,
                           const void* dinv, int64_t count, double* scalars,
                           int dtype, sfem_stream_t stream) {
  SFEM_REQUIRE(count >= 0 && scalars, "sfem_bicgstab_update_p: bad arguments");
  SFEM_BS_DTYPE("sfem_bicgstab_update_p");
  if (count == 0) return SFEM_OK;
  SFEM_REQUIRE(p && r && v && (!dinv || phat),
               "sfem_bicgstab_update_p: null pointer");
  const dim3 grid(stream_grid(count, 512 * 2)), block(512);
  if (dtype == SFEM_F64)
    hipLaunchKernelGGL(bicgstab_update_p_kernel<double>, grid, block, 0,
                       as_stream(stream), (double*)p, (double*)phat,
                       (const double*)r, (const double*)v, (const double*)dinv,
                       count, scalars);
  else
    hipLaunchKernelGGL(bicgstab_update_p_kernel<float>, grid, block, 0,
                       as_stream(stream), (float*)p, (float*)phat,
                       (const float*)r, (const float*)v, (const float*)dinv,
                       count, scalars);
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

int sfem_bicgstab_update_s(void* s, void* shat, const void* r, const void* v,
                           const void* dinv, int64_t count, double* scalars,
                           int dtype, sfem_stream_t stream) {
  SFEM_REQUIRE(count >= 0 && scalars, "sfem_bicgstab_update_s: bad arguments");
  SFEM_BS_DTYPE("sfem_bicgstab_update_s");
  if (count == 0) return SFEM_OK;
  SFEM_REQUIRE(s && r && v && (!dinv || shat),
               "sfem_bicgstab_update_s: null pointer");
  const dim3 grid(reduce_grid(count, 512 * 4)), block(512);
  if (dtype == SFEM_F64)
    hipLaunchKernelGGL(bicgstab_update_s_kernel<double>, grid, block, 0,
                       as_stream(stream), (double*)s, (double*)shat,
                       (const double*)r, (const double*)v, (const double*)dinv,
                       count, scalars);
  else
    hipLaunchKernelGGL(bicgstab_update_s_kernel<float>, grid, block, 0,
                       as_stream(stream), (float*)s, (float*)shat,
                       (const float*)r, (const float*)v, (const float*)dinv,
                       count, scalars);
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

int sfem_bicgstab_update_xr(void* x, void* r, const void* phat,
                            const void* shat, const void* s, const void* t,
                            const void* r0, int64_t count, double* scalars,
                            int dtype, sfem_stream_t stream) {
  SFEM_REQUIRE(count >= 0 && scalars, "sfem_bicgstab_update_xr: bad arguments");
  SFEM_BS_DTYPE("sfem_bicgstab_update_xr");
  if (count == 0) return SFEM_OK;
  SFEM_REQUIRE(x && r && phat && shat && s && t && r0,
               "sfem_bicgstab_update_xr: null pointer");
  const dim3 grid(reduce_grid(count, 512 * 4)), block(512);
  if (dtype == SFEM_F64)
    hipLaunchKernelGGL(bicgstab_update_xr_kernel<double>, grid, block, 0,
                       as_stream(stream), (double*)x, (double*)r,
                       (const double*)phat, (const double*)shat,
                       (const double*)s, (const double*)t, (const double*)r0,
                       count, scalars);
  else
    hipLaunchKernelGGL(bicgstab_update_xr_kernel<float>, grid, block, 0,
                       as_stream(stream), (float*)x, (float*)r,
                       (const float*)phat, (const float*)shat,
                       (const float*)s, (const float*)t, (const float*)r0,
                       count, scalars);
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

}  // extern "C"
