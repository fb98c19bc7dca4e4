// sg_queue_series.hip -- link queues, the time series (SG_LINK_QUEUE_SERIES): under the rates, per slot of
// watched links and per time bin, the server's busy time, the time-integral of the waiting queue, the
// weight served and the weight dropped.  A layer over all others (sg_queue.h): it runs once the
// per-record outputs stand at the input indices and reads nothing else of theirs.
//
// Behind the per-link values of out_link_busy_ns lies M[plane 0..3][slot][B + 2] (include/shadow_gpu.h
// has the definition): columns 0 .. B - 1 the bins, B the time before t0, B + 1 the time at or after
// the last bin's end.  A record's state is read from the sentinels of the drop rule and of the windowed
// form; a served record has start = done - s and e' = start - wait.
//
// The cost of a record does not follow the bins its wait or its service spans: an interval [a, b)
// is clipped into before, middle and after; the two end bins of the middle, whole or partial, are
// added straight into M, and the whole bins between them are a +1 / -1 pair in a difference array
// D[plane 0..1][slot][B + 1], which the context owns and the call zeroes.
//   k_series_records  a lane per record: its link by binary search in link_off, the slot, the state,
//                     and up to fourteen cell adds.  A link's records are adjacent and mostly in time
//                     order, so neighbouring lanes hit the same cell: every add is first summed over
//                     the wave's runs of adjacent lanes with the same cell, and only a run's first
//                     lane issues the atomic.  An add no lane of the wave makes costs one ballot.
//                     (sg_queue.h's wave_run_reduce wants equal keys in one run per wave, as links
//                     are; cells come back -- shuffled segments, carried order, shared slots -- so
//                     the run's end is taken from a ballot of the run heads here.)
//   the row pass      the running sum along every row of D, count * bin_ns added into M:
//     k_series_rows        short rows: a group of L = 1 .. 64 lanes per row, L from B on the host;
//     k_series_chunk_sums  long rows, a workgroup per chunk of S_CHUNK cells: the chunk's sum;
//     k_series_chunk_rows  the chunk again behind the sums of its row's earlier chunks.
// Sums are integers and wrap: the result does not depend on the order of the adds.  No workgroup
// waits on another.  No index is formed from a value that was not checked: a column is always one
// of B + 2 whatever the times are, and a slot value is compared with S first.
#include <vector>

#include "sg_queue.h"

namespace sg {
namespace {

constexpr uint32_t S_NONE = 0xFFFFFFFFu;  // no cell
constexpr uint32_t S_PENDING = 0xFFFFFFFFu;  // a pending record's ahead
constexpr uint32_t S_PER = 8;
constexpr uint32_t S_CHUNK = Q_THREADS * S_PER;
constexpr uint32_t S_ROW_LONG = 2048;  // rows past this many bins take the chunked form

struct SArgs {
  const u64* off;
  uint32_t n_links;
  u64 n;
  const uint32_t* packet;
  const uint32_t* weight;
  uint32_t n_weights;
  const u64* cost;
  const u64* slot;  // one per link (all ones: not watched); null: the identity
  const u64* wait;  // the per-record outputs, at input indices
  const u64* done;
  const uint32_t* ahead;  // windowed: tells a pending record from a dropped one; else null
  uint32_t drop;  // the drop rule's sentinels tell a record's state
  u64 t0, bin;
  uint32_t n_bins, n_slots;
  u64* m;  // 4 planes of n_slots rows of n_bins + 2
  u64* d;  // 2 planes of n_slots rows of n_bins + 1
  u64* part;  // the chunked row pass: a sum per chunk
  uint32_t chunks;  // per row
  u64* flag;
};

// v into base[cell] (S_NONE: nothing), summed first over the wave's runs of adjacent lanes with the
// same cell.  Every lane of the wave calls.
__device__ __forceinline__ void wave_cell_add(u64* base, uint32_t cell, u64 v) {
  if (__ballot(cell != S_NONE) == 0ull) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t below = __shfl_up(cell, 1, 64);
  const bool head = lane == 0u || below != cell;
  const u64 heads = __ballot(head);
  const u64 above = lane == 63u ? 0ull : heads >> (lane + 1u);
  const uint32_t end = above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : 64u;  // one past the run
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const u64 y = __shfl_down(v, d, 64);
    if (lane + d < end) v += y;
  }
  if (head && cell != S_NONE && v) atomicAdd(&base[cell], v);
}

// |[a, b) ∩ T_c| into row `row` of a plane m (all ones: no row, the lane only takes part), the
// whole bins between the end bins into the same row of d.
__device__ __forceinline__ void interval_add(const SArgs& a, u64* m, u64* d, uint32_t row, u64 lo, u64 hi) {
  const uint32_t nb = a.n_bins;
  const u64 mrow = (u64)row * (nb + 2u), drow = (u64)row * (nb + 1u);
  uint32_t c_first = S_NONE, c_last = S_NONE, c_before = S_NONE, c_after = S_NONE, d_up = S_NONE, d_down = S_NONE;
  u64 v_first = 0ull, v_last = 0ull, v_before = 0ull, v_after = 0ull;
  if (row != S_NONE && lo < hi) {
    if (lo < a.t0) {
      v_before = min(hi, a.t0) - lo;
      c_before = (uint32_t)(mrow + nb);
      lo = a.t0;
    }
    if (hi > a.t0) {
      // (from here on relative to t0, x < y; the range's end nb * bin may pass 2^64: by the quotient)
      const u64 x = lo - a.t0;
      u64 y = hi - a.t0;
      const u64 qx = x / a.bin;
      if (qx >= nb) {
        v_after = y - x;
        c_after = (uint32_t)(mrow + nb + 1u);
      } else {
        u64 qy = y / a.bin;
        if (qy >= nb) {  // (nb * bin <= y: the product fits)
          const u64 e = (u64)nb * a.bin;
          if (y > e) {
            v_after = y - e;
            c_after = (uint32_t)(mrow + nb + 1u);
          }
          y = e;
          qy = nb;
        }
        if (qx == qy) {
          v_first = y - x;
          c_first = (uint32_t)(mrow + qx);
        } else {
          v_first = (qx + 1ull) * a.bin - x;  // (qx + 1 <= qy: the product is at most y)
          c_first = (uint32_t)(mrow + qx);
          v_last = y - qy * a.bin;
          if (v_last) c_last = (uint32_t)(mrow + qy);  // (a remainder: qy < nb)
          if (qy > qx + 1ull) {
            d_up = (uint32_t)(drow + qx + 1ull);
            d_down = (uint32_t)(drow + qy);  // (qy <= nb: the row has nb + 1 cells)
          }
        }
      }
    }
  }
  wave_cell_add(m, c_first, v_first);
  wave_cell_add(m, c_last, v_last);
  wave_cell_add(m, c_before, v_before);
  wave_cell_add(m, c_after, v_after);
  wave_cell_add(d, d_up, 1ull);
  wave_cell_add(d, d_down, ~0ull);  // (-1: the sums wrap)
}

// The column of the instant t.
__device__ __forceinline__ uint32_t column_of(const SArgs& a, u64 t) {
  if (t < a.t0) return a.n_bins;
  const u64 q = (t - a.t0) / a.bin;
  return q < a.n_bins ? (uint32_t)q : a.n_bins + 1u;
}

__global__ void __launch_bounds__(Q_THREADS) k_series_records(const SArgs a) {
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;  // (the same for every lane of the launch)
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  const u64 cells = (u64)a.n_slots * (a.n_bins + 2u), dcells = (u64)a.n_slots * (a.n_bins + 1u);
  uint32_t row = S_NONE, c_served = S_NONE, c_dropped = S_NONE;
  u64 w = 0ull, start = 0ull, done = 0ull, enter = 0ull;
  bool served = false;
  if (i < a.n) {
    const uint32_t lk = link_of(a.off, a.n_links, i);
    u64 s = lk;
    if (a.slot) {
      s = a.slot[lk];
      if (s != Q_MAX && s >= a.n_slots) {
        atomicMin(&a.flag[Q_BAD_SLOT], (u64)lk);
        s = Q_MAX;  // (treated as not watched)
      }
    }
    if (s < a.n_slots) {
      const u64 wt = a.wait[i];
      done = a.done[i];
      uint32_t wu = 1u;
      if (a.weight) {
        const uint32_t p = a.packet[i];
        wu = p < a.n_weights ? a.weight[p] : 0u;  // (flagged by the call itself)
      }
      const bool pending = a.ahead && wt == Q_MAX && a.ahead[i] == S_PENDING;
      if (pending) {
        // nothing
      } else if (!a.drop || wt != Q_MAX) {
        served = true;
        row = (uint32_t)s;
        w = wu;
        start = done - service_ns(wu, a.cost[lk]);
        enter = start - wt;
        c_served = (uint32_t)(s * (a.n_bins + 2u) + column_of(a, done));
      } else if (done != Q_MAX) {  // dropped at its (carried) enter time; else absent
        w = wu;
        c_dropped = (uint32_t)(s * (a.n_bins + 2u) + column_of(a, done));
      }
    }
  }
  // (a served record of a result without an overflow has enter <= start <= done; any other order is an
  // empty interval)
  interval_add(a, a.m, a.d, served && start <= done ? row : S_NONE, start, done);
  interval_add(a, a.m + cells, a.d + dcells, served && enter <= start ? row : S_NONE, enter, start);
  wave_cell_add(a.m + 2ull * cells, c_served, w);
  wave_cell_add(a.m + 3ull * cells, c_dropped, w);
}

// ---- the row pass.  Row r of the 2 n_slots rows of d lies at d + r (n_bins + 1); it belongs to row
// r % n_slots of plane r / n_slots of m.
__device__ __forceinline__ u64* m_row(const SArgs& a, u64 r) { return a.m + r * (a.n_bins + 2u); }

// Short rows: lanes_log2 = log2 of the lanes per row.
__global__ void __launch_bounds__(Q_THREADS) k_series_rows(const SArgs a, uint32_t lanes_log2) {
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const uint32_t L = 1u << lanes_log2, sub = threadIdx.x & (L - 1u);
  const u64 r = ((u64)blockIdx.x * Q_THREADS + threadIdx.x) >> lanes_log2;
  const bool live = r < 2ull * a.n_slots;  // (a whole group at once: L divides the workgroup)
  const u64* d = a.d + (live ? r : 0ull) * (a.n_bins + 1u);
  u64* m = m_row(a, live ? r : 0ull);
  u64 carry = 0ull;
  for (uint32_t base = 0; base < a.n_bins; base += L) {  // (the same trip count for every lane)
    const uint32_t j = base + sub;
    const bool in = live && j < a.n_bins;
    u64 x = in ? d[j] : 0ull;
    for (uint32_t k = 1; k < L; k <<= 1) {
      const u64 y = __shfl_up(x, k, L);
      if (sub >= k) x += y;
    }
    const u64 count = carry + x;
    if (in && count) m[j] += count * a.bin;
    carry += __shfl(x, L - 1u, L);
  }
}

__device__ __forceinline__ void chunk_of(const SArgs& a, u64& r, uint32_t& j0) {
  r = blockIdx.x / a.chunks;
  j0 = (blockIdx.x % a.chunks) * S_CHUNK + threadIdx.x * S_PER;
}

__global__ void __launch_bounds__(Q_THREADS) k_series_chunk_sums(const SArgs a) {
  __shared__ u64 s_wave[16];
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  u64 r;
  uint32_t j0;
  chunk_of(a, r, j0);
  const u64* d = a.d + r * (a.n_bins + 1u);
  u64 x = 0ull;
#pragma unroll
  for (uint32_t k = 0; k < S_PER; k++)
    if (j0 + k < a.n_bins) x += d[j0 + k];
  u64 total;
  block_exclusive(x, s_wave, &total);
  if (threadIdx.x == 0) a.part[blockIdx.x] = total;
}

__global__ void __launch_bounds__(Q_THREADS) k_series_chunk_rows(const SArgs a) {
  __shared__ u64 s_wave[16];
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  u64 r;
  uint32_t j0;
  chunk_of(a, r, j0);
  const uint32_t chunk = blockIdx.x % a.chunks;
  // the row's earlier chunks
  u64 before = 0ull, total;
  for (uint32_t c = threadIdx.x; c < chunk; c += Q_THREADS) before += a.part[blockIdx.x - chunk + c];
  block_exclusive(before, s_wave, &total);
  const u64 carry = total;
  const u64* d = a.d + r * (a.n_bins + 1u);
  u64* m = m_row(a, r);
  u64 v[S_PER], x = 0ull;
#pragma unroll
  for (uint32_t k = 0; k < S_PER; k++) {
    v[k] = j0 + k < a.n_bins ? d[j0 + k] : 0ull;
    x += v[k];
  }
  u64 count = carry + block_exclusive(x, s_wave, &total);
#pragma unroll
  for (uint32_t k = 0; k < S_PER; k++) {
    count += v[k];
    if (j0 + k < a.n_bins && count) m[j0 + k] += count * a.bin;
  }
}

}  // namespace

QSeries queue_series_plan(sg_ctx* ctx, const u64* cost_tail, bool dev, uint32_t n_links) {
  u64 h[4];
  if (dev)
    copy_to_host(ctx, h, cost_tail, sizeof(h));  // (one more synchronisation of a device-mode call)
  else
    std::copy(cost_tail, cost_tail + 4, h);
  if (h[1] == 0ull || h[2] == 0ull) throw Error(SG_ERR_INVALID_ARG, "SG_LINK_QUEUE_SERIES with bin_ns or n_bins zero");
  if (h[2] > 0xFFFFFFFFull || h[3] > 0xFFFFFFFFull) throw Error(SG_ERR_CAPACITY, "SG_LINK_QUEUE_SERIES: n_bins or n_slots past 2^32 - 1");
  QSeries s = {};
  s.t0 = h[0];
  s.bin = h[1];
  s.n_bins = (uint32_t)h[2];
  s.mapped = h[3] != 0ull;
  s.n_slots = s.mapped ? (uint32_t)h[3] : n_links;
  s.cells = (u64)s.n_slots * ((u64)s.n_bins + 2ull);
  if (s.cells > 0x80000000ull) throw Error(SG_ERR_CAPACITY, "SG_LINK_QUEUE_SERIES: more than 2^31 cells a plane");
  if (s.mapped && !dev) {
    const u64* slot = cost_tail + 4;
    for (uint32_t lk = 0; lk < n_links; lk++)
      if (slot[lk] != Q_MAX && slot[lk] >= s.n_slots)
        throw Error(SG_ERR_INVALID_ARG,
                    "SG_LINK_QUEUE_SERIES: link " + std::to_string(lk) + " has slot " + std::to_string(slot[lk]) +
                        ", not below n_slots and not 2^64 - 1",
                    lk, 0xFFFFFFFFu);
  }
  return s;
}

void queue_series(sg_ctx* ctx, const QArgs& a, const QSeries& s, bool drop, bool window) {
  // read_timer("link_queue_series_cells") = (0, n_slots (n_bins + 2), the call's records)
  timer_set_counter(ctx, "link_queue_series_cells", (double)a.n, s.cells, true);
  if (!a.n || !s.cells) return;
  hipStream_t st = ctx->stream;
  SArgs x = {};
  x.off = a.off;
  x.n_links = a.n_links;
  x.n = a.n;
  x.packet = a.packet;
  x.weight = a.weight;
  x.n_weights = a.n_weights;
  x.cost = a.cost;
  const size_t c0 = (drop ? 2 : 1) * (size_t)a.n_links;
  x.slot = s.mapped ? a.cost + c0 + 4 : nullptr;
  x.wait = a.out.wait;
  x.done = a.out.done;
  x.ahead = window ? a.out.ahead : nullptr;
  x.drop = drop ? 1u : 0u;
  x.t0 = s.t0;
  x.bin = s.bin;
  x.n_bins = s.n_bins;
  x.n_slots = s.n_slots;
  x.m = a.out.busy + c0;
  const size_t d_cells = 2 * (size_t)s.n_slots * ((size_t)s.n_bins + 1);
  x.d = ctx->qs_diff.get<u64>(d_cells);
  x.flag = a.flag;
  const u64 rows = 2ull * s.n_slots;
  const bool chunked = s.n_bins > S_ROW_LONG;
  if (chunked) {
    x.chunks = (s.n_bins + S_CHUNK - 1u) / S_CHUNK;
    // (rows * chunks <= 2 cells / S_ROW_LONG + rows: a grid's size)
    x.part = ctx->qs_part.get<u64>((size_t)(rows * x.chunks));
  }
  const dim3 blk(Q_THREADS);
  TimedLaunch tl(ctx, "link_queue_series", (double)a.n);
  SG_HIP(hipMemsetAsync(x.d, 0, d_cells * 8, st));
  hipLaunchKernelGGL(k_series_records, dim3(grid_for(a.n, Q_THREADS, 0x7FFFFFFFu)), blk, 0, st, x);
  SG_CHECK_LAUNCH();
  if (chunked) {
    const dim3 g((unsigned)(rows * x.chunks));
    hipLaunchKernelGGL(k_series_chunk_sums, g, blk, 0, st, x);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_series_chunk_rows, g, blk, 0, st, x);
    SG_CHECK_LAUNCH();
  } else {
    uint32_t lg = 0;
    while (lg < 6u && (1u << lg) < s.n_bins) lg++;
    hipLaunchKernelGGL(k_series_rows, dim3(grid_for((size_t)(rows << lg), Q_THREADS, 0x7FFFFFFFu)), blk, 0, st, x, lg);
    SG_CHECK_LAUNCH();
  }
}

}  // namespace sg
