// sg_scan.hip -- the exclusive u64 scan of u32 counts, reduce-then-scan in three launches: the
// block sums of tiles of SCAN_TILE counts; one workgroup over the sums, which also writes off[n]
// and the total into a word of its own (the callers': pinned and mapped); the add.  No workgroup
// waits on another inside a launch.  Users: the hop counts of sg_paths.hip (off = out_off) and the
// link counters of sg_trace.hip (off = out_link_off).
#include <algorithm>

#include "sg_internal.h"
#include "sg_scan.h"

namespace sg {
namespace {

constexpr uint32_t SCAN_THREADS = 256;
constexpr uint32_t SCAN_PER = 8;  // counts per thread
constexpr uint32_t SCAN_TILE = SCAN_THREADS * SCAN_PER;
constexpr uint32_t SCAN_SUMS_THREADS = 1024;

// (wave_inclusive, block_exclusive: sg_scan.h)

__global__ void __launch_bounds__(SCAN_THREADS) k_scan_block_sums(const uint32_t* cnt, uint32_t n,
                                                                  unsigned long long* sums) {
  __shared__ unsigned long long s_wave[16];
  const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
  unsigned long long x = 0ull;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_PER; k++)
    if (base + k < n) x += cnt[base + k];
  unsigned long long total;
  block_exclusive(x, s_wave, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: the block sums to their exclusive prefix, in place; off[n] and the total.
__global__ void __launch_bounds__(SCAN_SUMS_THREADS) k_scan_sums(unsigned long long* sums, uint32_t n_blocks,
                                                                 uint32_t n, unsigned long long* off,
                                                                 unsigned long long* out_total) {
  __shared__ unsigned long long s_wave[16];
  unsigned long long carry = 0ull;
  for (uint32_t base = 0; base < n_blocks; base += blockDim.x) {
    const uint32_t b = base + threadIdx.x;
    const unsigned long long x = b < n_blocks ? sums[b] : 0ull;
    unsigned long long total;
    const unsigned long long ex = block_exclusive(x, s_wave, &total);
    if (b < n_blocks) sums[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    off[n] = carry;
    *out_total = carry;
  }
}

__global__ void __launch_bounds__(SCAN_THREADS) k_scan_add(const uint32_t* cnt, uint32_t n,
                                                           const unsigned long long* sums, unsigned long long* off) {
  __shared__ unsigned long long s_wave[16];
  const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
  uint32_t c[SCAN_PER];
  unsigned long long x = 0ull;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_PER; k++) {
    c[k] = base + k < n ? cnt[base + k] : 0u;
    x += c[k];
  }
  unsigned long long total;
  unsigned long long at = sums[blockIdx.x] + block_exclusive(x, s_wave, &total);
#pragma unroll
  for (uint32_t k = 0; k < SCAN_PER; k++) {
    if (base + k < n) off[base + k] = at;
    at += c[k];
  }
}

}  // namespace

void scan_counts(sg_ctx* ctx, const uint32_t* cnt, uint32_t n, unsigned long long* off, unsigned long long* total) {
  // (at least one block: n == 0 still writes off[0] and the total)
  const uint32_t n_blocks = std::max(1u, (uint32_t)(((size_t)n + SCAN_TILE - 1) / SCAN_TILE));
  unsigned long long* sums = ctx->p_sums.get<unsigned long long>(n_blocks);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_scan_block_sums, dim3(n_blocks), dim3(SCAN_THREADS), 0, st, cnt, n, sums);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_SUMS_THREADS), 0, st, sums, n_blocks, n, off, total);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_scan_add, dim3(n_blocks), dim3(SCAN_THREADS), 0, st, cnt, n, (const unsigned long long*)sums,
                     off);
  SG_CHECK_LAUNCH();
}

}  // namespace sg
