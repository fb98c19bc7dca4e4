// sg_segsort.h -- the three-tier segmented sort of 16-byte keys (time lo, time hi, tie word,
// payload word), ascending (time, tie word) inside every segment of an offset array.  Its users:
// the link trace (sg_trace.hip: segments are links, the tie word the packet, the payload the hop)
// and the carried link queues (sg_queue_carry.hip: a packet's records by input time, and every link's
// records by carried time once per iteration).
//   k_trace_sort_small  a wave per segment: up to 64 records are ranked in the wave's registers
//                       (keys are unique, so ranks are a permutation); a longer segment is cut
//                       into pieces of P records, work entry = (segment, piece);
//   k_trace_sort_lds    a workgroup per piece: bitonic sort of its keys in LDS (16 bytes a key,
//                       32 KiB at P = 2048); a segment of one piece is written out, a piece of a
//                       longer one goes sorted to the second staging array;
//   k_trace_merge       the pieces of a longer segment are merged by rank: a record's place is
//                       its index in its piece plus, for every other piece, the number of keys
//                       below its own (a binary search).
// Keys must be unique within a segment and no tie word may be UINT32_MAX (the LDS tier's padding).
// The kernels have internal linkage: each file that includes this header gets its own.
#pragma once

#include "sg_internal.h"
#include "sg_walks.h"

namespace sg {
namespace {

constexpr uint32_t TR_THREADS = 256;
constexpr uint32_t TR_RANK_MAX = 64;     // a segment up to one wave: rank sort in registers
constexpr uint32_t TR_PIECE_MAX = 2048;  // keys of one piece in LDS: 16 bytes x 2048 = 32 KiB

// (TraceOut: sg_walks.h)
struct TraceRec {
  unsigned long long enter, exit;
  uint32_t packet, hop;
};

__device__ __forceinline__ TraceRec trace_load(const uint4* key, const unsigned long long* exit, size_t at) {
  const uint4 k = key[at];
  return TraceRec{((unsigned long long)k.y << 32) | k.x, exit ? exit[at] : 0ull, k.z, k.w};
}

__device__ __forceinline__ void trace_store(uint4* key, unsigned long long* exit, size_t at, const TraceRec& r) {
  key[at] = make_uint4((uint32_t)r.enter, (uint32_t)(r.enter >> 32), r.packet, r.hop);
  if (exit) exit[at] = r.exit;
}

__device__ __forceinline__ void trace_emit(const TraceOut& o, size_t at, const TraceRec& r) {
  if (o.packet) o.packet[at] = r.packet;
  if (o.hop) o.hop[at] = r.hop;
  if (o.enter) o.enter[at] = r.enter;
  if (o.exit) o.exit[at] = r.exit;
}

__device__ __forceinline__ bool trace_less(unsigned long long ta, uint32_t pa, unsigned long long tb, uint32_t pb) {
  return ta < tb || (ta == tb && pa < pb);
}

// Tier 1, a wave per link.  n_work (one word, zeroed) counts the work entries of the longer segments.
__global__ void __launch_bounds__(TR_THREADS) k_trace_sort_small(const unsigned long long* off, uint32_t n_links,
                                                                const uint4* key, const unsigned long long* exit,
                                                                TraceOut out, uint32_t piece, uint2* work,
                                                                uint32_t work_cap, uint32_t* n_work) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * TR_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * TR_THREADS) >> 6;
  for (uint32_t lk = wave; lk < n_links; lk += n_waves) {
    const unsigned long long s0 = off[lk];
    const uint32_t n = __builtin_amdgcn_readfirstlane((uint32_t)(off[lk + 1] - s0));
    if (n == 0) continue;
    if (n <= TR_RANK_MAX) {
      TraceRec r = {};
      if (lane < n) r = trace_load(key, exit, (size_t)s0 + lane);
      uint32_t rank = 0;
      for (uint32_t j = 0; j < n; j++) {
        const unsigned long long tj = __shfl(r.enter, (int)j, 64);
        const uint32_t pj = __shfl(r.packet, (int)j, 64);
        rank += trace_less(tj, pj, r.enter, r.packet) ? 1u : 0u;
      }
      if (lane < n) trace_emit(out, (size_t)s0 + rank, r);
    } else {
      const uint32_t pieces = (n + piece - 1) / piece;
      uint32_t at = 0;
      if (lane == 0) at = atomicAdd(n_work, pieces);
      at = __shfl(at, 0, 64);
      for (uint32_t c = lane; c < pieces; c += 64)
        if (at + c < work_cap) work[at + c] = make_uint2(lk, c);
    }
  }
}

struct TraceKey {
  unsigned long long t;
  uint32_t p, idx;
};

// Tier 2, a workgroup per piece: bitonic sort of the keys in LDS.  A segment of one piece is
// final: written out.  A piece of a longer segment goes, sorted, to the second staging array.
__global__ void __launch_bounds__(TR_THREADS) k_trace_sort_lds(const unsigned long long* off, const uint4* key,
                                                              const unsigned long long* exit, uint4* key2,
                                                              unsigned long long* exit2, TraceOut out, uint32_t piece,
                                                              const uint2* work, uint32_t work_cap,
                                                              const uint32_t* n_work_p) {
  __shared__ TraceKey s_key[TR_PIECE_MAX];
  const uint32_t n_work = min(*n_work_p, work_cap);
  for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
    const uint2 we = work[wi];
    const unsigned long long s0 = off[we.x];
    const uint32_t n = (uint32_t)(off[we.x + 1] - s0);
    const uint32_t p0 = we.y * piece, m = min(n - p0, piece);
    uint32_t P = 64;
    while (P < m) P <<= 1;  // <= TR_PIECE_MAX: piece is
    for (uint32_t i = threadIdx.x; i < P; i += TR_THREADS) {
      TraceKey k = {~0ull, ~0u, ~0u};  // padding sorts last (no packet index is UINT32_MAX)
      if (i < m) {
        const uint4 q = key[(size_t)s0 + p0 + i];
        k = TraceKey{((unsigned long long)q.y << 32) | q.x, q.z, i};
      }
      s_key[i] = k;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t i = threadIdx.x; i < P; i += TR_THREADS) {
          const uint32_t x = i ^ j;
          if (x > i) {
            const TraceKey a = s_key[i], b = s_key[x];
            const bool up = (i & k) == 0;
            if (trace_less(b.t, b.p, a.t, a.p) == up) {
              s_key[i] = b;
              s_key[x] = a;
            }
          }
        }
        __syncthreads();
      }
    for (uint32_t i = threadIdx.x; i < m; i += TR_THREADS) {
      const uint32_t idx = s_key[i].idx;
      if (idx >= m) continue;  // (padding never sorts below a record)
      const TraceRec r = trace_load(key, exit, (size_t)s0 + p0 + idx);
      if (n <= piece)
        trace_emit(out, (size_t)s0 + i, r);
      else
        trace_store(key2, exit2, (size_t)s0 + p0 + i, r);
    }
    __syncthreads();
  }
}

// Tier 3, a hot link: the segment's sorted pieces are merged by rank -- a record's final position
// is its index in its own piece plus, for every other piece, the number of keys below its own (a
// binary search; unique keys, so no tie rule is needed).
__global__ void __launch_bounds__(TR_THREADS) k_trace_merge(const unsigned long long* off, const uint4* key2,
                                                           const unsigned long long* exit2, TraceOut out, uint32_t piece,
                                                           const uint2* work, uint32_t work_cap,
                                                           const uint32_t* n_work_p) {
  const uint32_t n_work = min(*n_work_p, work_cap);
  for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
    const uint2 we = work[wi];
    const unsigned long long s0 = off[we.x];
    const uint32_t n = (uint32_t)(off[we.x + 1] - s0);
    if (n <= piece) continue;
    const uint32_t pieces = (n + piece - 1) / piece;
    const uint32_t p0 = we.y * piece, m = min(n - p0, piece);
    for (uint32_t i = threadIdx.x; i < m; i += TR_THREADS) {
      const TraceRec r = trace_load(key2, exit2, (size_t)s0 + p0 + i);
      uint32_t rank = i;
      for (uint32_t c = 0; c < pieces; c++) {
        if (c == we.y) continue;
        const uint32_t q0 = c * piece, qm = min(n - q0, piece);
        uint32_t lo = 0, hi = qm;  // the first index of piece c whose key is not below r's
        for (int it = 0; it < 32 && lo < hi; it++) {
          const uint32_t mid = lo + (hi - lo) / 2;
          const uint4 q = key2[(size_t)s0 + q0 + mid];
          if (trace_less(((unsigned long long)q.y << 32) | q.x, q.z, r.enter, r.packet))
            lo = mid + 1;
          else
            hi = mid;
        }
        rank += lo;
      }
      if (rank < n) trace_emit(out, (size_t)s0 + rank, r);  // (always, with unique keys)
    }
  }
}

// The work entries `tot` records in segments can need: the pieces of the segments past TR_RANK_MAX.
inline uint64_t segsort_work_cap(uint64_t tot, uint32_t piece) { return tot / piece + tot / TR_RANK_MAX + 1; }

// The three tiers on the context stream: the segments of off (n_seg + 1 entries) of `key` (and
// `exit`, or null) sorted into `out`.  key2 / exit2: the second staging arrays, as long as the
// first; work: work_cap entries; n_work: one zeroed word.
inline void segsort_enqueue(sg_ctx* ctx, const unsigned long long* off, uint32_t n_seg, const uint4* key,
                            const unsigned long long* exit, uint4* key2, unsigned long long* exit2, const TraceOut& out,
                            uint32_t piece, uint2* work, uint32_t work_cap, uint32_t* n_work) {
  hipStream_t st = ctx->stream;
  const dim3 g_small(grid_for((size_t)n_seg * 64, TR_THREADS, 16u * (unsigned)ctx->n_cu));
  const dim3 g_work(grid_for(work_cap, 1, 8u * (unsigned)ctx->n_cu));
  hipLaunchKernelGGL(k_trace_sort_small, g_small, dim3(TR_THREADS), 0, st, off, n_seg, key, exit, out, piece, work,
                     work_cap, n_work);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_trace_sort_lds, g_work, dim3(TR_THREADS), 0, st, off, key, exit, key2, exit2, out, piece,
                     (const uint2*)work, work_cap, (const uint32_t*)n_work);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_trace_merge, g_work, dim3(TR_THREADS), 0, st, off, (const uint4*)key2,
                     (const unsigned long long*)exit2, out, piece, (const uint2*)work, work_cap,
                     (const uint32_t*)n_work);
  SG_CHECK_LAUNCH();
}

}  // namespace
}  // namespace sg
