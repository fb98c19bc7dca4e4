// sg_scan.h -- the wave and workgroup scan helpers of the reduce-then-scan kernels: the u64 sums of
// sg_scan.hip and the (head flag, S, M) elements of the link queues (sg_queue.h).  Device code only.
//
// An element type T needs scan_shfl_up(T, d) (the value of the lane d below, anything where there
// is none) and an operator op(lower, upper) that is associative; it need not commute: the lower
// lane's value is always the left argument.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sg {

__device__ __forceinline__ unsigned long long scan_shfl_up(unsigned long long x, uint32_t d) {
  return __shfl_up(x, d, 64);
}

struct ScanPlus {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const {
    return a + b;
  }
};

template <class T, class Op>
__device__ __forceinline__ T wave_inclusive_op(T x, Op op) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const T y = scan_shfl_up(x, d);
    if (lane >= d) x = op(y, x);
  }
  return x;
}

__device__ __forceinline__ unsigned long long wave_inclusive(unsigned long long x) {
  return wave_inclusive_op(x, ScanPlus());
}

// The exclusive prefix of x over the workgroup's threads (blockDim.x a multiple of 64, at most
// 1024); *total = the sum.  s_wave: 16 words of LDS; every thread calls.
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long x, unsigned long long* s_wave,
                                                              unsigned long long* total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned long long inc = wave_inclusive(x);
  __syncthreads();  // (the last call's reads of s_wave)
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  unsigned long long before = 0ull, all = 0ull;
  for (uint32_t k = 0; k < nw; k++) {
    const unsigned long long t = s_wave[k];
    if (k < w) before += t;
    all += t;
  }
  *total = all;
  return before + inc - x;
}

// The same for any element and operator: the exclusive prefix (`identity` for thread 0), *total =
// the whole workgroup's.  s_wave: 16 elements of LDS.
template <class T, class Op>
__device__ __forceinline__ T block_exclusive_op(T x, T identity, T* s_wave, T* total, Op op) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const T inc = wave_inclusive_op(x, op);
  T ex = scan_shfl_up(inc, 1);
  if (lane == 0) ex = identity;
  __syncthreads();  // (the last call's reads of s_wave)
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  T before = identity, all = identity;
  for (uint32_t k = 0; k < nw; k++) {
    const T t = s_wave[k];
    if (k < w) before = op(before, t);
    all = op(all, t);
  }
  *total = all;
  return op(before, ex);
}

}  // namespace sg
