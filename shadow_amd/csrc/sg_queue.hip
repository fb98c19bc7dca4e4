// sg_queue.hip -- link queues: the FIFO wait of every crossing of a link trace under a link rate.
//
// Input is a link trace (sg_trace.hip, sg_group_trace.hip): link L owns records [off[L], off[L + 1])
// in arrival order.  Per record, with `done` starting at the link's free_in value (include/
// shadow_gpu.h has the definition):
//   s = min(ceil(w cost / 1000), MAX);  start = max(enter, done);  done = min(start + s, MAX);
//   wait = start - enter;  ahead = #{earlier records of the segment with done > enter}.
//
// The recurrence is a segmented scan in the (max, saturating +) algebra: record i is the element
// (S, M) = (s, enter (+) s), the operator (S1, M1) o (S2, M2) = (S1 (+) S2, max(M1 (+) S2, M2)) with
// (+) saturating at MAX = 2^64 - 1; a segment's first record takes max(enter, free_in) for enter,
// so done_i is the M of its segment's prefix.  Saturating addition of non-negative values is
// associative and max distributes over it: any bracketing gives the serial loop's value, and
// done_i == MAX is the overflow test.
//
// Launches on the context stream, one flat scan over all records whatever the segment lengths:
//   k_queue_links   a lane per link_off entry: validates link_off (every later kernel returns at
//                   once when it is bad: no index is formed from a bad value), zeroes the per-link
//                   sums and gives an empty link its free_in value;
//   k_queue_agg     a tile of Q_TILE records per workgroup, Q_PER consecutive records per lane: the
//                   tile's aggregate (head flag, S, M).  A lane finds the link of its first record
//                   by binary search in link_off and advances through the offsets from there;
//   k_queue_carry   one workgroup over the tile aggregates, looping past its 1024 threads: the
//                   `done` that enters each tile;
//   k_queue_rescan  the tile again with that carry: wait, done, out_link_free from a segment's
//                   last record, and the per-link busy / wait sums.  A lane sums its own run of
//                   equal links first; lanes whose records all lie on one link are then summed
//                   across the wave by a segmented reduction keyed by the link, and only the
//                   first lane of a run issues the atomics: a link of 100k records gets one add
//                   per wave, not one per record;
//   k_queue_ahead   a lane per record: done is non-decreasing within a segment, so ahead is one
//                   binary search over the done values of the segment's prefix; the per-link
//                   maximum by the same wave reduction.
// No workgroup waits on another inside a launch.  SG_LINK_QUEUE_SERIAL = 1 replaces agg, carry
// and rescan by k_queue_serial, a lane per link looping over its segment.
//
// SG_LINK_QUEUE_CARRY carries every wait to the packet's later hops: a fixed point over the same
// scan, with every link sorted anew by the carried times in each iteration ("the carried form",
// below queue_run's helpers).
//
// SG_LINK_QUEUE_DROP gives every link a finite buffer and drops at its tail: the unlimited scan
// above only marks the busy periods, which are then walked from an idle server side by side
// ("finite buffers", below k_queue_ahead).
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_scan.h"
#include "sg_segsort.h"

namespace sg {
namespace {

using u64 = unsigned long long;

constexpr uint32_t Q_THREADS = 256;
constexpr uint32_t Q_PER = 8;  // consecutive records per lane
constexpr uint32_t Q_TILE = Q_THREADS * Q_PER;
constexpr uint32_t Q_CARRY_THREADS = 1024;
constexpr u64 Q_MAX = ~0ull;
constexpr uint32_t Q_NO_LINK = 0xFFFFFFFFu;

// flag words (all ones: nothing found; the smallest value wins)
// (the carried form adds Q_DUP, the smallest record with a twin in its packet's chain, and
// Q_CHANGED, 0 once an iteration moved an enter time)
enum { Q_BAD_OFF = 0, Q_BAD_PACKET = 1, Q_OVERFLOW = 2, Q_DUP = 3, Q_CHANGED = 4, Q_WORDS = 5 };

struct QArgs {
  const u64* off;
  uint32_t n_links;
  u64 n;
  const u64* enter;
  const uint32_t* packet;
  const uint32_t* weight;
  uint32_t n_weights;
  const u64* cost;
  const u64* free_in;
  u64* wait;
  u64* done;  // the caller's, or the scratch array k_queue_ahead reads, or null
  uint32_t* ahead;
  u64* link_free;
  u64* busy;
  u64* wmax;
  u64* wsum;
  uint32_t* amax;
  u64* flag;
  // the tile aggregates; agg_m becomes the `done` entering each tile
  u64* agg_s;
  u64* agg_m;
  uint32_t* agg_h;
};

__device__ __forceinline__ u64 sat_add(u64 a, u64 b) {
  const u64 r = a + b;
  return r < a ? Q_MAX : r;
}

// min(ceil(w cost / 1000), MAX), the product taken exactly (96 bits)
__device__ __forceinline__ u64 service_ns(uint32_t w, u64 cost) {
  const u64 lo = (u64)w * cost, hi = __umul64hi((u64)w, cost);
  u64 q, r;
  if (hi == 0ull) {
    q = lo / 1000ull;
    r = lo - q * 1000ull;
  } else {
    // hi < 2^32: long division of the limbs (hi, lo >> 32, lo & 2^32 - 1) by 1000
    if (hi >= 1000ull) return Q_MAX;  // the quotient is 2^64 or more
    const u64 t1 = (hi << 32) | (lo >> 32), q1 = t1 / 1000ull, r1 = t1 - q1 * 1000ull;
    const u64 t0 = (r1 << 32) | (lo & 0xFFFFFFFFull), q0 = t0 / 1000ull;
    r = t0 - q0 * 1000ull;
    if (q1 >> 32) return Q_MAX;
    q = (q1 << 32) | q0;
  }
  return r != 0ull && q != Q_MAX ? q + 1ull : q;
}

// The link that owns record i < n of a valid link_off: the L with off[L] <= i < off[L + 1].
__device__ __forceinline__ uint32_t link_of(const u64* __restrict__ off, uint32_t n_links, u64 i) {
  uint32_t lo = 1, hi = n_links;  // the first L' in [1, n_links] with off[L'] > i (off[n_links] = n > i)
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] > i)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo - 1;
}

// A lane's place in link_off while it steps through consecutive records.
struct QCursor {
  uint32_t link;
  u64 end;  // off[link + 1]
  __device__ __forceinline__ void seek(const QArgs& a, u64 i) {
    link = link_of(a.off, a.n_links, i);
    end = a.off[link + 1];
  }
  // to record i, one past the last; true when the link changed
  __device__ __forceinline__ bool step(const QArgs& a, u64 i) {
    if (i < end) return false;
    link++;  // (i == end: a later link starts here, and link + 1 <= n_links while i < n)
    end = a.off[link + 1];
    if (i >= end) seek(a, i);  // empty links in between
    return true;
  }
};

// The weight of record i; a packet index past the weights is flagged and counts 0.
__device__ __forceinline__ uint32_t record_weight(const QArgs& a, u64 i, bool flag) {
  if (!a.weight) return 1u;
  const uint32_t p = a.packet[i];
  if (p >= a.n_weights) {
    if (flag) atomicMin(&a.flag[Q_BAD_PACKET], i);
    return 0u;
  }
  return a.weight[p];
}

// ---- the scan's element
struct QElem {
  u64 s, m;
  uint32_t head;
};

__device__ __forceinline__ QElem scan_shfl_up(QElem x, uint32_t d) {
  return QElem{__shfl_up(x.s, d, 64), __shfl_up(x.m, d, 64), __shfl_up(x.head, d, 64)};
}

struct QOp {
  __device__ __forceinline__ QElem operator()(const QElem& a, const QElem& b) const {
    if (b.head) return b;
    return QElem{sat_add(a.s, b.s), max(sat_add(a.m, b.s), b.m), a.head};
  }
};

// (every element has m >= s, so this is the identity on both sides)
__device__ __forceinline__ QElem q_identity() { return QElem{0ull, 0ull, 0u}; }

// A lane's Q_PER records: service, enter time, link, and which are a segment's first and last.
struct QLane {
  u64 s[Q_PER], e[Q_PER];
  uint32_t link[Q_PER];
  uint32_t head, last, count;  // bit masks; the records the lane has
};

template <bool FLAG>
__device__ __forceinline__ QElem lane_load(const QArgs& a, u64 base, QLane& r) {
  QElem acc = q_identity();
  r.head = r.last = r.count = 0u;
  if (base >= a.n) return acc;
  QCursor c;
  c.seek(a, base);
  u64 cost = a.cost[c.link];
  bool head = base == a.off[c.link];
#pragma unroll
  for (uint32_t k = 0; k < Q_PER; k++) {
    const u64 i = base + k;
    r.s[k] = r.e[k] = 0ull;
    r.link[k] = Q_NO_LINK;
    if (i >= a.n) continue;
    if (k > 0 && c.step(a, i)) {
      head = true;
      cost = a.cost[c.link];
    }
    const u64 s = service_ns(record_weight(a, i, FLAG), cost), e = a.enter[i];
    r.s[k] = s;
    r.e[k] = e;
    r.link[k] = c.link;
    r.count = k + 1;
    if (head) {
      r.head |= 1u << k;
      const u64 x0 = a.free_in ? a.free_in[c.link] : 0ull;
      acc = QElem{s, sat_add(max(e, x0), s), 1u};
    } else {
      acc = QElem{sat_add(acc.s, s), sat_add(max(acc.m, e), s), acc.head};
    }
    if (i + 1 == c.end) r.last |= 1u << k;
    head = false;
  }
  return acc;
}

// ---- link_off's check, the per-link sums' zeroes, the empty links
__global__ void __launch_bounds__(Q_THREADS) k_queue_links(const QArgs a) {
  const u64 q = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (q > a.n_links) return;
  const uint32_t lk = (uint32_t)q;
  const u64 o = a.off[lk];
  if (lk == 0 && o != 0ull) atomicMin(&a.flag[Q_BAD_OFF], 0ull);
  if (lk == a.n_links) {
    if (o != a.n) atomicMin(&a.flag[Q_BAD_OFF], (u64)lk);
    return;
  }
  const u64 o1 = a.off[lk + 1];
  if (o1 < o) atomicMin(&a.flag[Q_BAD_OFF], (u64)lk);
  if (a.busy) a.busy[lk] = 0ull;
  if (a.wmax) a.wmax[lk] = 0ull;
  if (a.wsum) a.wsum[lk] = 0ull;
  if (a.amax) a.amax[lk] = 0u;
  if (a.link_free && o1 == o) a.link_free[lk] = a.free_in ? a.free_in[lk] : 0ull;
}

// ---- 1. the tile aggregates
__global__ void __launch_bounds__(Q_THREADS) k_queue_agg(const QArgs a) {
  __shared__ QElem s_wave[16];
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  QLane r;
  const QElem x = lane_load<true>(a, (u64)blockIdx.x * Q_TILE + (u64)threadIdx.x * Q_PER, r);
  QElem total;
  block_exclusive_op(x, q_identity(), s_wave, &total, QOp());
  if (threadIdx.x == 0) {
    a.agg_s[blockIdx.x] = total.s;
    a.agg_m[blockIdx.x] = total.m;
    a.agg_h[blockIdx.x] = total.head;
  }
}

// ---- 2. one workgroup: agg_m[t] = the M of everything before tile t (the `done` entering it)
__global__ void __launch_bounds__(Q_CARRY_THREADS) k_queue_carry(const QArgs a, uint32_t n_tiles) {
  __shared__ QElem s_wave[16];
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const QOp op;
  QElem carry = q_identity();
  for (uint32_t base = 0; base < n_tiles; base += Q_CARRY_THREADS) {
    const uint32_t b = base + threadIdx.x;
    const QElem x = b < n_tiles ? QElem{a.agg_s[b], a.agg_m[b], a.agg_h[b]} : q_identity();
    QElem total;
    const QElem ex = block_exclusive_op(x, q_identity(), s_wave, &total, op);
    if (b < n_tiles) a.agg_m[b] = op(carry, ex).m;
    carry = op(carry, total);
  }
}

// The segmented reduction of a wave's (key, busy, wait max, wait sum): equal keys sit in
// consecutive lanes (links rise with the record index); afterwards the first lane of a run of
// equal keys holds the run's sums.  Every lane calls.
struct QSums {
  u64 busy, wmax, wsum;
};

__device__ __forceinline__ bool wave_run_sums(uint32_t key, QSums& x) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t k2 = __shfl_down(key, d, 64);
    const u64 b = __shfl_down(x.busy, d, 64), m = __shfl_down(x.wmax, d, 64), s = __shfl_down(x.wsum, d, 64);
    if (lane + d < 64 && k2 == key) {
      x.busy += b;
      x.wmax = max(x.wmax, m);
      x.wsum += s;
    }
  }
  const uint32_t below = __shfl_up(key, 1, 64);
  return key != Q_NO_LINK && (lane == 0 || below != key);
}

__device__ __forceinline__ void link_sums_add(const QArgs& a, uint32_t link, const QSums& x) {
  if (a.busy && x.busy) atomicAdd(&a.busy[link], x.busy);
  if (a.wmax && x.wmax) atomicMax(&a.wmax[link], x.wmax);
  if (a.wsum && x.wsum) atomicAdd(&a.wsum[link], x.wsum);
}

// ---- 3. the tile again, with its carry
__global__ void __launch_bounds__(Q_THREADS) k_queue_rescan(const QArgs a) {
  __shared__ QElem s_wave[16];
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 base = (u64)blockIdx.x * Q_TILE + (u64)threadIdx.x * Q_PER;
  QLane r;
  const QElem x = lane_load<false>(a, base, r);
  QElem total;
  const QElem ex = block_exclusive_op(x, q_identity(), s_wave, &total, QOp());
  // (ex.head: a segment starts in the tile below this lane, the carry does not reach it)
  u64 done = ex.head ? ex.m : max(sat_add(a.agg_m[blockIdx.x], ex.s), ex.m);
  const bool sums = a.busy || a.wmax || a.wsum;
  QSums run = {0ull, 0ull, 0ull};
  uint32_t run_link = Q_NO_LINK;
#pragma unroll
  for (uint32_t k = 0; k < Q_PER; k++) {
    if (k >= r.count) continue;
    const uint32_t lk = r.link[k];
    if ((r.head >> k) & 1u) done = a.free_in ? a.free_in[lk] : 0ull;
    const u64 start = max(r.e[k], done), wait = start - r.e[k];
    done = sat_add(start, r.s[k]);
    if (done == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], base + k);
    if (a.wait) a.wait[base + k] = wait;
    if (a.done) a.done[base + k] = done;
    if (a.link_free && ((r.last >> k) & 1u)) a.link_free[lk] = done;
    if (sums) {
      if (lk != run_link) {
        if (run_link != Q_NO_LINK) link_sums_add(a, run_link, run);
        run_link = lk;
        run = QSums{0ull, 0ull, 0ull};
      }
      run.busy += r.s[k];
      run.wmax = max(run.wmax, wait);
      run.wsum += wait;
    }
  }
  if (sums) {  // (the same for every lane of the launch)
    // a lane whose records lie on one link joins the wave's reduction; any other adds its last run itself
    uint32_t key = Q_NO_LINK;
    if (r.count && r.link[0] == run_link) {
      key = run_link;
    } else if (run_link != Q_NO_LINK) {
      link_sums_add(a, run_link, run);
    }
    if (wave_run_sums(key, run)) link_sums_add(a, key, run);
  }
}

// ---- the lane-per-link form
__global__ void __launch_bounds__(Q_THREADS) k_queue_serial(const QArgs a) {
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 stride = (u64)gridDim.x * Q_THREADS;
  for (u64 q = (u64)blockIdx.x * Q_THREADS + threadIdx.x; q < a.n_links; q += stride) {
    const uint32_t lk = (uint32_t)q;
    const u64 i0 = a.off[lk], i1 = a.off[lk + 1];
    if (i0 == i1) continue;  // (k_queue_links wrote an empty link's outputs)
    const u64 cost = a.cost[lk];
    u64 done = a.free_in ? a.free_in[lk] : 0ull;
    QSums run = {0ull, 0ull, 0ull};
    for (u64 i = i0; i < i1; i++) {
      const u64 s = service_ns(record_weight(a, i, true), cost), e = a.enter[i];
      const u64 start = max(e, done), wait = start - e;
      done = sat_add(start, s);
      if (done == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], i);
      if (a.wait) a.wait[i] = wait;
      if (a.done) a.done[i] = done;
      run.busy += s;
      run.wmax = max(run.wmax, wait);
      run.wsum += wait;
    }
    if (a.link_free) a.link_free[lk] = done;
    if (a.busy) a.busy[lk] = run.busy;
    if (a.wmax) a.wmax[lk] = run.wmax;
    if (a.wsum) a.wsum[lk] = run.wsum;
  }
}

// ---- ahead: the records of the segment's prefix still in the system when record i arrives
__global__ void __launch_bounds__(Q_THREADS) k_queue_ahead(const QArgs a) {
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const uint32_t lane = threadIdx.x & 63u;
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  uint32_t key = Q_NO_LINK, ahead = 0u;
  if (i < a.n) {
    key = link_of(a.off, a.n_links, i);
    const u64 e = a.enter[i];
    u64 lo = a.off[key], hi = i;  // the first j of the prefix with done[j] > e
    while (lo < hi) {
      const u64 mid = lo + (hi - lo) / 2;
      if (a.done[mid] > e)
        hi = mid;
      else
        lo = mid + 1;
    }
    ahead = (uint32_t)min(i - lo, (u64)0xFFFFFFFFull);
    if (a.ahead) a.ahead[i] = ahead;
  }
  if (!a.amax) return;  // (the same for every lane)
  uint32_t m = ahead;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t k2 = __shfl_down(key, d, 64), m2 = __shfl_down(m, d, 64);
    if (lane + d < 64 && k2 == key) m = max(m, m2);
  }
  const uint32_t below = __shfl_up(key, 1, 64);
  if (key != Q_NO_LINK && (lane == 0 || below != key) && m) atomicMax(&a.amax[key], m);
}

// ---- finite buffers (SG_LINK_QUEUE_DROP): tail drop under a longest wait per link.
//
// The limited recurrence -- start = max(enter, done); start - enter > limit: dropped, done as it
// was; else done = start + s -- is no constant-size scan (the map of one record is not closed
// under composition), but its `done` never exceeds the unlimited queue's.  A record the unlimited
// scan serves without waiting therefore finds the limited server idle too: the limited queue
// restarts there, and a link's records fall into independent busy periods.
//   agg, carry       the unlimited scan's first two launches, as above;
//   k_drop_heads     the tile again with its carry: mark[i] = 1 where the unlimited wait is 0 or a
//                    segment starts.  No caller output, no overflow flag (the pass may saturate);
//   scan_counts      the marks' exclusive sums, and k_drop_starts: the period starts, compacted;
//   k_drop_lane      a lane per period: one of at most D_SHORT records is walked by its lane,
//                    a longer one is appended to the list of long periods;
//   k_drop_wave      a wave per long period: 64 records per coalesced load (the next 64 in flight
//                    meanwhile), the scalar `done` stepped through them by lane reads of a uniform
//                    lane; every lane keeps the `done` before its record and finishes it alone.
// A walk leaves per record wt (the wait; all ones: not served), run (the `done` after it: it never
// falls within a segment, a dropped record repeats the value before it) and mark (1: served).
// SG_LINK_QUEUE_SERIAL = 1: k_drop_serial, a lane per link, leaves the same three arrays.
//   k_drop_finish    a lane per record: the caller's wait, done and ahead (one binary search over
//                    run, then a difference of the served marks' exclusive sums), out_link_free,
//                    and the per-link sums by the wave reduction of k_queue_ahead.
// Carried (d.absent): a record whose enter time is all ones is absent: it sorts last on its link,
// is a period of its own in the unlimited pass, and is skipped by every walk.
constexpr uint32_t D_SHORT = 32;  // the longest period a lane walks

struct DArgs {
  QArgs q;           // the inputs, agg_*, flag; wait / done / ahead and the per-link arrays: k_drop_finish's
  const u64* limit;  // cost + n_links
  uint32_t absent;   // carried: enter == MAX is an absent record
  uint32_t lng_cap;
  uint32_t* mark;  // the period heads, then the served records
  u64* pos;        // n + 2: the exclusive sums of mark, the total twice
  uint32_t* start;  // the period starts
  uint32_t* lng;    // the long periods, in any order
  uint32_t* n_long;
  u64* run;
  u64* wt;
  uint32_t* drops;  // the second halves of out_link_ahead_max and out_link_busy_ns, or null
  u64* refused;
};

__global__ void __launch_bounds__(Q_THREADS) k_drop_links(const DArgs d) {
  const u64 q = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (q >= d.q.n_links) return;
  if (d.drops) d.drops[q] = 0u;
  if (d.refused) d.refused[q] = 0ull;
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_heads(const DArgs d) {
  __shared__ QElem s_wave[16];
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 base = (u64)blockIdx.x * Q_TILE + (u64)threadIdx.x * Q_PER;
  QLane r;
  const QElem x = lane_load<false>(a, base, r);
  QElem total;
  const QElem ex = block_exclusive_op(x, q_identity(), s_wave, &total, QOp());
  u64 done = ex.head ? ex.m : max(sat_add(a.agg_m[blockIdx.x], ex.s), ex.m);
#pragma unroll
  for (uint32_t k = 0; k < Q_PER; k++) {
    if (k >= r.count) continue;
    const bool head = (r.head >> k) & 1u;
    if (head) done = a.free_in ? a.free_in[r.link[k]] : 0ull;
    d.mark[base + k] = head || r.e[k] >= done ? 1u : 0u;
    done = sat_add(max(r.e[k], done), r.s[k]);
  }
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_starts(const DArgs d) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= d.q.n || d.q.flag[Q_BAD_OFF] != Q_MAX) return;
  if (!d.mark[i]) return;
  const u64 at = d.pos[i];
  if (at < d.q.n) d.start[at] = (uint32_t)i;
}

// One record under the drop rule: the wait (all ones: not served) and the new `done`.
__device__ __forceinline__ u64 drop_step(u64& done, u64 e, u64 s, u64 lim, bool absent) {
  if (absent && e == Q_MAX) return Q_MAX;
  const u64 start = max(e, done), w = start - e;
  if (w > lim) return Q_MAX;
  done = sat_add(start, s);
  return w;
}

// Records [i0, i1) of link lk, one after the other.
template <bool FLAG>
__device__ __forceinline__ void drop_walk(const DArgs& d, uint32_t lk, u64 i0, u64 i1, u64 done) {
  const QArgs& a = d.q;
  const u64 cost = a.cost[lk], lim = d.limit[lk];
  for (u64 i = i0; i < i1; i++) {
    const u64 s = service_ns(record_weight(a, i, FLAG), cost), e = a.enter[i];
    const u64 w = drop_step(done, e, s, lim, d.absent != 0u);
    if (w != Q_MAX && done == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], i);
    d.wt[i] = w;
    d.run[i] = done;
    d.mark[i] = w != Q_MAX ? 1u : 0u;
  }
}

// Period p's records [i0, i1) and link, and the `done` it starts from: the link's free_in at a
// segment's first record, else the head's own enter time (the server is idle there).  False: not
// a period of a valid compaction.
__device__ __forceinline__ bool drop_period(const DArgs& d, u64 p, u64 np, u64& i0, u64& i1, uint32_t& lk, u64& done) {
  const QArgs& a = d.q;
  i0 = d.start[p];
  i1 = p + 1 < np ? (u64)d.start[p + 1] : a.n;
  if (i0 >= i1 || i1 > a.n) return false;
  lk = link_of(a.off, a.n_links, i0);
  if (i1 > a.off[lk + 1]) return false;
  done = i0 == a.off[lk] ? (a.free_in ? a.free_in[lk] : 0ull) : a.enter[i0];
  return true;
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_lane(const DArgs d) {
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 p = (u64)blockIdx.x * Q_THREADS + threadIdx.x, np = min(d.pos[a.n], a.n);
  if (p >= np) return;
  u64 i0, i1, done;
  uint32_t lk;
  if (!drop_period(d, p, np, i0, i1, lk, done)) return;
  if (i1 - i0 > D_SHORT) {
    const uint32_t slot = atomicAdd(d.n_long, 1u);
    if (slot < d.lng_cap) d.lng[slot] = (uint32_t)p;
    return;
  }
  drop_walk<false>(d, lk, i0, i1, done);
}

__device__ __forceinline__ u64 uniform64(u64 v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 lane_read64(u64 v, uint32_t k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)k);
  return ((u64)hi << 32) | lo;
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_wave(const DArgs d) {
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const uint32_t lane = threadIdx.x & 63u, waves = Q_THREADS / 64u;
  const uint32_t n_long = min(*d.n_long, d.lng_cap);
  const u64 np = min(d.pos[a.n], a.n);
  const bool absent = d.absent != 0u;
  for (uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * waves + (threadIdx.x >> 6))); w < n_long;
       w += gridDim.x * waves) {
    const u64 p = d.lng[w];
    if (p >= np) continue;
    u64 i0, i1, done;
    uint32_t lk;
    if (!drop_period(d, p, np, i0, i1, lk, done)) continue;
    i0 = uniform64(i0);
    i1 = uniform64(i1);
    done = uniform64(done);
    lk = (uint32_t)__builtin_amdgcn_readfirstlane((int)lk);
    // (in scalar registers before the first load below is issued: the stepping loop waits for no memory)
    const u64 cost = uniform64(a.cost[lk]), lim = uniform64(d.limit[lk]);
    u64 e = 0ull, s = 0ull;
    if (i0 + lane < i1) {
      e = a.enter[i0 + lane];
      s = service_ns(record_weight(a, i0 + lane, false), cost);
    }
    for (u64 b = i0; b < i1; b += 64ull) {
      // the next 64 records, in flight while these are stepped through
      u64 e2 = 0ull, s2 = 0ull;
      if (b + 64ull + lane < i1) {
        e2 = a.enter[b + 64ull + lane];
        s2 = service_ns(record_weight(a, b + 64ull + lane, false), cost);
      }
      const uint32_t cnt = (uint32_t)min((u64)64ull, i1 - b);
      u64 before = 0ull;
      for (uint32_t k = 0; k < cnt; k++) {
        const u64 ek = lane_read64(e, k), sk = lane_read64(s, k);
        if (lane == k) before = done;
        drop_step(done, ek, sk, lim, absent);
      }
      if (lane < cnt) {
        const u64 i = b + lane;
        const u64 wt = drop_step(before, e, s, lim, absent);
        if (wt != Q_MAX && before == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], i);
        d.wt[i] = wt;
        d.run[i] = before;
        d.mark[i] = wt != Q_MAX ? 1u : 0u;
      }
      e = e2;
      s = s2;
    }
  }
}

// ---- the lane-per-link form under the drop rule
__global__ void __launch_bounds__(Q_THREADS) k_drop_serial(const DArgs d) {
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 stride = (u64)gridDim.x * Q_THREADS;
  for (u64 q = (u64)blockIdx.x * Q_THREADS + threadIdx.x; q < a.n_links; q += stride) {
    const uint32_t lk = (uint32_t)q;
    drop_walk<true>(d, lk, a.off[lk], a.off[lk + 1], a.free_in ? a.free_in[lk] : 0ull);
  }
}

// A wave's segmented reduction of x by f over runs of equal keys in consecutive lanes; the first
// lane of a run holds the run's value.  Every lane calls.
template <class T, class F>
__device__ __forceinline__ T wave_run_reduce(uint32_t key, T x, F f) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t k2 = __shfl_down(key, d, 64);
    const T y = __shfl_down(x, d, 64);
    if (lane + d < 64 && k2 == key) x = f(x, y);
  }
  return x;
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_finish(const DArgs d, uint32_t want_ahead) {
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const uint32_t lane = threadIdx.x & 63u;
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  uint32_t key = Q_NO_LINK, ahead = 0u, drops = 0u;
  u64 busy = 0ull, wmax = 0ull, wsum = 0ull, refused = 0ull;
  if (i < a.n) {
    key = link_of(a.off, a.n_links, i);
    const u64 i0 = a.off[key], i1 = a.off[key + 1];
    const u64 e = a.enter[i], w = d.wt[i], r = d.run[i];
    const bool absent = d.absent && e == Q_MAX, served = w != Q_MAX;
    if (want_ahead && !absent) {
      u64 lo = i0, hi = i;  // the first j of the prefix with run[j] > e: the served from there on are ahead
      while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (d.run[mid] > e)
          hi = mid;
        else
          lo = mid + 1;
      }
      ahead = (uint32_t)min(d.pos[i] - d.pos[lo], (u64)0xFFFFFFFFull);
    }
    if (a.wait) a.wait[i] = w;
    if (a.done) a.done[i] = served ? r : e;
    if (a.ahead) a.ahead[i] = ahead;
    if (a.link_free) {
      // run after the last record that arrives: the done of the record served last, or free_in
      if (absent) {
        if (i == i0) a.link_free[key] = a.free_in ? a.free_in[key] : 0ull;
      } else if (i + 1 == i1 || (d.absent && a.enter[i + 1] == Q_MAX)) {
        a.link_free[key] = r;
      }
    }
    if (!absent) {
      const u64 s = service_ns(record_weight(a, i, false), a.cost[key]);
      if (served) {
        busy = s;
        wmax = wsum = w;
      } else {
        refused = s;
        drops = 1u;
        ahead = 0u;  // (the maximum runs over served records)
      }
    }
  }
  if (!a.busy && !a.wmax && !a.wsum && !a.amax) return;  // (the same for every lane)
  const auto add64 = [](u64 x, u64 y) { return x + y; };
  const auto max64 = [](u64 x, u64 y) { return max(x, y); };
  const uint32_t below = __shfl_up(key, 1, 64);
  const bool first = key != Q_NO_LINK && (lane == 0 || below != key);
  if (a.busy) {
    busy = wave_run_reduce(key, busy, add64);
    refused = wave_run_reduce(key, refused, add64);
    if (first && busy) atomicAdd(&a.busy[key], busy);
    if (first && refused) atomicAdd(&d.refused[key], refused);
  }
  if (a.wmax) {
    wmax = wave_run_reduce(key, wmax, max64);
    if (first && wmax) atomicMax(&a.wmax[key], wmax);
  }
  if (a.wsum) {
    wsum = wave_run_reduce(key, wsum, add64);
    if (first && wsum) atomicAdd(&a.wsum[key], wsum);
  }
  if (a.amax) {
    ahead = wave_run_reduce(key, ahead, [](uint32_t x, uint32_t y) { return max(x, y); });
    drops = wave_run_reduce(key, drops, [](uint32_t x, uint32_t y) { return x + y; });
    if (first && ahead) atomicMax(&a.amax[key], ahead);
    if (first && drops) atomicAdd(&d.drops[key], drops);
  }
}

// the first bad link of a host link_off; all ones when it is good
u64 bad_link_off(const uint64_t* off, uint32_t n_links, uint64_t n) {
  if (off[0] != 0) return 0;
  for (uint32_t k = 0; k < n_links; k++)
    if (off[k + 1] < off[k]) return k;
  return off[n_links] != n ? (u64)n_links : Q_MAX;
}

[[noreturn]] void throw_bad_off(u64 link) {
  throw Error(SG_ERR_INVALID_ARG,
              "link_off is not an offset array of the records at link " + std::to_string(link) +
                  " (it starts at 0, never falls and ends at n_records)",
              (uint32_t)link, 0xFFFFFFFFu);
}

// The queue scan of a.enter / a.packet as they lie, in either form, on the context stream.
void launch_scan(sg_ctx* ctx, const QArgs& a, uint32_t n_tiles, bool serial) {
  hipStream_t st = ctx->stream;
  if (serial) {
    hipLaunchKernelGGL(k_queue_serial, dim3(grid_for(a.n_links, Q_THREADS, 16u * (unsigned)ctx->n_cu)), dim3(Q_THREADS),
                       0, st, a);
    SG_CHECK_LAUNCH();
  } else {
    hipLaunchKernelGGL(k_queue_agg, dim3(n_tiles), dim3(Q_THREADS), 0, st, a);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_queue_carry, dim3(1), dim3(Q_CARRY_THREADS), 0, st, a, n_tiles);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_queue_rescan, dim3(n_tiles), dim3(Q_THREADS), 0, st, a);
    SG_CHECK_LAUNCH();
  }
}

// The walk under the drop rule, in either form: wt, run and the served marks of every record.
void launch_drop(sg_ctx* ctx, const DArgs& d, uint32_t n_tiles, bool serial) {
  hipStream_t st = ctx->stream;
  const QArgs& a = d.q;
  const dim3 g_rec(grid_for(a.n, Q_THREADS, 0x7FFFFFFFu)), blk(Q_THREADS);
  if (serial) {
    hipLaunchKernelGGL(k_drop_serial, dim3(grid_for(a.n_links, Q_THREADS, 16u * (unsigned)ctx->n_cu)), blk, 0, st, d);
    SG_CHECK_LAUNCH();
    return;
  }
  hipLaunchKernelGGL(k_queue_agg, dim3(n_tiles), blk, 0, st, a);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_queue_carry, dim3(1), dim3(Q_CARRY_THREADS), 0, st, a, n_tiles);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_drop_heads, dim3(n_tiles), blk, 0, st, d);
  SG_CHECK_LAUNCH();
  scan_counts(ctx, d.mark, (uint32_t)a.n, d.pos, d.pos + a.n + 1);
  SG_HIP(hipMemsetAsync(d.n_long, 0, 4, st));
  hipLaunchKernelGGL(k_drop_starts, g_rec, blk, 0, st, d);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_drop_lane, g_rec, blk, 0, st, d);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_drop_wave, dim3(grid_for(d.lng_cap, Q_THREADS / 64u, 8u * (unsigned)ctx->n_cu)), blk, 0, st, d);
  SG_CHECK_LAUNCH();
}

// Every output the caller takes, from a walk's three arrays.
void launch_drop_finish(sg_ctx* ctx, const DArgs& d, bool want_ahead) {
  hipStream_t st = ctx->stream;
  const QArgs& a = d.q;
  if (want_ahead) scan_counts(ctx, d.mark, (uint32_t)a.n, d.pos, d.pos + a.n + 1);
  hipLaunchKernelGGL(k_drop_finish, dim3(grid_for(a.n, Q_THREADS, 0x7FFFFFFFu)), dim3(Q_THREADS), 0, st, d,
                     want_ahead ? 1u : 0u);
  SG_CHECK_LAUNCH();
}

// ---- the carried form (SG_LINK_QUEUE_CARRY): a wait moves the packet's later hops.
//
// Set-up, once: the records of every packet in ascending input (enter, record) order -- a
// histogram per packet (k_carry_count, which also checks packet[i] < n_packets), scan_counts, a
// fill with a cursor per packet (k_carry_fill) and the segmented sort of sg_segsort.h with packets
// for segments -- then k_carry_chain: next[i], gap[i] = enter[next] - enter[i] (0: two records of
// one packet at one time, flagged) and cur[i] = enter[i].
// An iteration: keys (cur[i], packet[i], i) (k_carry_keys), the segmented sort by link over the
// caller's link_off, the queue scan over the sorted order (done only), and k_carry_propagate, a
// lane per sorted record: cur[next] = done + gap, and the changed word when that moved it.  Every
// cur cell has one writer, and the sort copied the keys before: the update is in place.  The host
// reads the flag words once per iteration; when nothing changed, the scan runs once more over the
// same order with every output the caller takes, k_queue_ahead after it, and k_carry_scatter
// moves wait, done and ahead through the permutation to the input indices.
// No index is formed from a value that was not checked: a record index read from the sort's
// output is compared with n (two records of one packet on one link can meet at one carried time
// while the iteration is under way; the sort then ranks them alike and leaves a slot unwritten).
constexpr uint32_t Q_NO_NEXT = 0xFFFFFFFFu;

struct CArgs {
  u64 n;
  uint32_t n_packets;
  const u64* enter;  // the uncongested schedule
  const uint32_t* packet;
  uint32_t* cnt;   // records per packet
  uint32_t* fill;  // the fill's cursor per packet
  const u64* pkt_off;
  uint4* key;
  uint32_t* list;  // the records packet by packet, ascending (enter, record)
  uint32_t* next;
  u64* gap;
  u64* cur;
  // a link-sorted pass
  const uint32_t* perm;
  u64* s_done;
  u64* s_wait;
  uint32_t* s_ahead;
  u64* flag;
};

__device__ __forceinline__ bool carry_bad(const CArgs& c) {
  return c.flag[Q_BAD_OFF] != Q_MAX || c.flag[Q_BAD_PACKET] != Q_MAX;
}

__global__ void __launch_bounds__(Q_THREADS) k_carry_count(const CArgs c) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= c.n) return;
  const uint32_t p = c.packet[i];
  if (p >= c.n_packets)
    atomicMin(&c.flag[Q_BAD_PACKET], i);
  else
    atomicAdd(&c.cnt[p], 1u);
}

__global__ void __launch_bounds__(Q_THREADS) k_carry_fill(const CArgs c) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= c.n || carry_bad(c)) return;
  const uint32_t p = c.packet[i];
  if (p >= c.n_packets) return;
  const u64 at = c.pkt_off[p] + atomicAdd(&c.fill[p], 1u);
  const u64 e = c.enter[i];
  if (at < c.pkt_off[p + 1]) c.key[at] = make_uint4((uint32_t)e, (uint32_t)(e >> 32), (uint32_t)i, 0u);
}

__global__ void __launch_bounds__(Q_THREADS) k_carry_chain(const CArgs c) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= c.n || carry_bad(c)) return;
  const uint32_t i = c.list[j];
  if (i >= c.n) return;
  const uint32_t p = c.packet[i];
  if (p >= c.n_packets) return;
  const u64 e = c.enter[i];
  uint32_t nx = Q_NO_NEXT;
  u64 g = 0ull;
  if (j + 1 < c.pkt_off[p + 1]) {
    nx = c.list[j + 1];
    if (nx >= c.n) {
      nx = Q_NO_NEXT;
    } else {
      g = c.enter[nx] - e;  // (the list is ascending)
      if (g == 0ull) atomicMin(&c.flag[Q_DUP], (u64)i);  // (equal times lie in record order: i < nx)
    }
  }
  c.next[i] = nx;
  c.gap[i] = g;
  c.cur[i] = e;
}

__global__ void __launch_bounds__(Q_THREADS) k_carry_keys(const CArgs c) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= c.n) return;
  const u64 e = c.cur[i];
  c.key[i] = make_uint4((uint32_t)e, (uint32_t)(e >> 32), c.packet[i], (uint32_t)i);
}

__global__ void __launch_bounds__(Q_THREADS) k_carry_propagate(const CArgs c) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= c.n) return;
  const uint32_t i = c.perm[j];
  if (i >= c.n) return;
  const uint32_t nx = c.next[i];
  if (nx == Q_NO_NEXT) return;  // (else below n: k_carry_chain checked it)
  const u64 v = sat_add(c.s_done[j], c.gap[i]);
  if (v == Q_MAX) atomicMin(&c.flag[Q_OVERFLOW], j);
  if (v != c.cur[nx]) {
    c.cur[nx] = v;
    c.flag[Q_CHANGED] = 0ull;
  }
}

// The same under SG_LINK_QUEUE_DROP: the successor of a record that is not served (wt all ones:
// dropped or absent) is absent, cur = MAX; only a served record can carry past 2^64 - 1.
__global__ void __launch_bounds__(Q_THREADS) k_carry_propagate_drop(const CArgs c, const u64* wt) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= c.n) return;
  const uint32_t i = c.perm[j];
  if (i >= c.n) return;
  const uint32_t nx = c.next[i];
  if (nx == Q_NO_NEXT) return;
  u64 v = Q_MAX;
  if (wt[j] != Q_MAX) {
    v = sat_add(c.s_done[j], c.gap[i]);
    if (v == Q_MAX) atomicMin(&c.flag[Q_OVERFLOW], j);
  }
  if (v != c.cur[nx]) {
    c.cur[nx] = v;
    c.flag[Q_CHANGED] = 0ull;
  }
}

__global__ void __launch_bounds__(Q_THREADS) k_carry_scatter(const CArgs c, u64* wait, u64* done, uint32_t* ahead) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= c.n) return;
  const uint32_t i = c.perm[j];
  if (i >= c.n) return;
  if (wait) wait[i] = c.s_wait[j];
  if (done) done[i] = c.s_done[j];
  if (ahead) ahead[i] = c.s_ahead[j];
}

using PairOf = std::function<void(u64, uint32_t&, uint32_t&)>;

// read_timer("link_queue_iters") = (0, the iterations of the last carried call, its records).
// Kept whether or not the timers are on: the iterations are part of what a caller is told.
void set_iters(sg_ctx* ctx, u64 n, uint32_t iters) {
  KernelTimer* t = nullptr;
  for (auto& kv : ctx->timers)
    if (kv.first == "link_queue_iters") t = &kv.second;
  if (!t) {
    ctx->timers.emplace_back("link_queue_iters", KernelTimer());
    t = &ctx->timers.back().second;
  }
  t->work = (double)n;
  t->launches = iters;
}

// `a`: the call's arrays on the device (n > 0 records, agg_* set for the scan form, flag words all ones).
// `drop`: the call's DArgs under SG_LINK_QUEUE_DROP (its scratch arrays set), else null.
void queue_carry(sg_ctx* ctx, const QArgs& a, uint32_t n_tiles, bool serial, bool want_ahead, const PairOf& pair_of,
                 const std::function<void(u64)>& throw_bad_packet, const DArgs* drop) {
  hipStream_t st = ctx->stream;
  const u64 n = a.n;
  const uint32_t nl = a.n_links, np = a.n_weights;
  const int cap = knob_int("SG_LINK_QUEUE_CARRY_ITERS", 4096, 1, INT_MAX);
  const uint32_t piece = (uint32_t)knob_int("SG_LINK_TRACE_PIECE", (int)TR_PIECE_MAX, (int)TR_RANK_MAX, (int)TR_PIECE_MAX);
  const uint64_t work_cap64 = segsort_work_cap(n, piece);
  if (work_cap64 > 0xFFFFFFFFull) throw Error(SG_ERR_CAPACITY, "more records than one carried call sorts");
  const uint32_t work_cap = (uint32_t)work_cap64;
  const dim3 g_rec(grid_for(n, Q_THREADS, 0x7FFFFFFFu)), blk(Q_THREADS);

  // the counters and the cursors per packet and the sort's work counter: one block, zeroed
  uint32_t* ctr = ctx->qc_cnt.get<uint32_t>(2 * (size_t)np + 1);
  SG_HIP(hipMemsetAsync(ctr, 0, (2 * (size_t)np + 1) * 4, st));
  uint32_t* n_work = ctr + 2 * (size_t)np;
  u64* pkt_off = ctx->qc_off.get<u64>((size_t)np + 2);  // (the last word: the scan's total)
  uint4* key = ctx->tr_key.get<uint4>(n);
  uint4* key2 = ctx->tr_key2.get<uint4>(n);
  uint2* work = ctx->tr_work.get<uint2>(work_cap);
  u64* s_enter = ctx->qc_enter.get<u64>(n);
  uint32_t* s_packet = ctx->qc_packet.get<uint32_t>(n);
  uint32_t* perm = ctx->qc_perm.get<uint32_t>(n);
  CArgs c = {};
  c.n = n;
  c.n_packets = np;
  c.enter = a.enter;
  c.packet = a.packet;
  c.cnt = ctr;
  c.fill = ctr + np;
  c.pkt_off = pkt_off;
  c.key = key;
  c.list = ctx->qc_list.get<uint32_t>(n);
  c.next = ctx->qc_next.get<uint32_t>(n);
  c.gap = ctx->qc_gap.get<u64>(n);
  c.cur = ctx->qc_cur.get<u64>(n);
  c.perm = perm;
  c.s_done = ctx->qc_done.get<u64>(n);
  c.s_wait = a.wait ? ctx->qc_wait.get<u64>(n) : nullptr;
  c.s_ahead = a.ahead ? ctx->qc_ahead.get<uint32_t>(n) : nullptr;
  c.flag = a.flag;

  // link_off's check alone: no output is written before the last pass
  QArgs v = a;
  v.link_free = v.busy = v.wmax = v.wsum = nullptr;
  v.amax = nullptr;
  hipLaunchKernelGGL(k_queue_links, dim3(grid_for((size_t)nl + 1, Q_THREADS)), blk, 0, st, v);
  SG_CHECK_LAUNCH();
  {
    TimedLaunch tl(ctx, "link_queue_index", (double)n);
    hipLaunchKernelGGL(k_carry_count, g_rec, blk, 0, st, c);
    SG_CHECK_LAUNCH();
    scan_counts(ctx, c.cnt, np, pkt_off, pkt_off + np + 1);
    hipLaunchKernelGGL(k_carry_fill, g_rec, blk, 0, st, c);
    SG_CHECK_LAUNCH();
    const TraceOut chain = {c.list, nullptr, nullptr, nullptr};
    segsort_enqueue(ctx, pkt_off, np, (const uint4*)key, nullptr, key2, nullptr, chain, piece, work, work_cap, n_work);
    hipLaunchKernelGGL(k_carry_chain, g_rec, blk, 0, st, c);
    SG_CHECK_LAUNCH();
  }
  u64 h[Q_WORDS];
  copy_to_host(ctx, h, a.flag, sizeof(h));
  if (h[Q_BAD_OFF] != Q_MAX) throw_bad_off(h[Q_BAD_OFF]);
  if (h[Q_BAD_PACKET] != Q_MAX) throw_bad_packet(h[Q_BAD_PACKET]);
  if (h[Q_DUP] != Q_MAX) {
    uint32_t lk, at;
    pair_of(h[Q_DUP], lk, at);
    throw Error(SG_ERR_INVALID_ARG,
                "record " + std::to_string(h[Q_DUP]) + " (link " + std::to_string(lk) +
                    ") enters at the time of another record of its packet",
                lk, at);
  }

  // the scan's view of a sorted pass
  QArgs s = v;
  s.enter = s_enter;
  s.packet = s_packet;
  s.wait = nullptr;
  s.done = c.s_done;
  s.ahead = nullptr;
  const TraceOut sorted = {s_packet, perm, s_enter, nullptr};
  // under the drop rule a walk's `run` is the sorted pass's done
  DArgs ds = {};
  if (drop) {
    ds = *drop;
    ds.q = s;
    ds.absent = 1u;
    ds.run = c.s_done;
  }
  uint32_t iters = 0;
  bool settled = false;
  while (!settled && iters < (uint32_t)cap) {
    iters++;
    SG_HIP(hipMemsetAsync(a.flag + Q_CHANGED, 0xff, 8, st));
    SG_HIP(hipMemsetAsync(n_work, 0, 4, st));
    {
      TimedLaunch tl(ctx, "link_queue_sort", (double)n);
      hipLaunchKernelGGL(k_carry_keys, g_rec, blk, 0, st, c);
      SG_CHECK_LAUNCH();
      segsort_enqueue(ctx, a.off, nl, (const uint4*)key, nullptr, key2, nullptr, sorted, piece, work, work_cap, n_work);
    }
    {
      TimedLaunch tl(ctx, "link_queue", (double)n);
      if (drop)
        launch_drop(ctx, ds, n_tiles, serial);
      else
        launch_scan(ctx, s, n_tiles, serial);
    }
    {
      TimedLaunch tl(ctx, "link_queue_carry", (double)n);
      if (drop)
        hipLaunchKernelGGL(k_carry_propagate_drop, g_rec, blk, 0, st, c, (const u64*)ds.wt);
      else
        hipLaunchKernelGGL(k_carry_propagate, g_rec, blk, 0, st, c);
      SG_CHECK_LAUNCH();
    }
    copy_to_host(ctx, h, a.flag, sizeof(h));
    set_iters(ctx, n, iters);
    if (h[Q_OVERFLOW] != Q_MAX) {
      uint32_t lk, at;
      pair_of(h[Q_OVERFLOW], lk, at);
      throw Error(SG_ERR_TIME_OVERFLOW, "a record of link " + std::to_string(lk) + " is served or carried past 2^64 - 1 ns",
                  lk, at);
    }
    settled = h[Q_CHANGED] == Q_MAX;
  }
  if (!settled)
    throw Error(SG_ERR_CAPACITY,
                "the carried times still moved after " + std::to_string(iters) + " iterations (SG_LINK_QUEUE_CARRY_ITERS)",
                iters, 0xFFFFFFFFu);

  // the last pass, over the order the last iteration sorted: every output the caller takes
  s.wait = c.s_wait;
  s.ahead = c.s_ahead;
  s.link_free = a.link_free;
  s.busy = a.busy;
  s.wmax = a.wmax;
  s.wsum = a.wsum;
  s.amax = a.amax;
  hipLaunchKernelGGL(k_queue_links, dim3(grid_for((size_t)nl + 1, Q_THREADS)), blk, 0, st, s);
  SG_CHECK_LAUNCH();
  if (drop) {
    // (k_drop_finish reads run while it writes done: the sorted done of the last pass has an array of its own)
    s.done = a.done ? ctx->qd_done.get<u64>(n) : nullptr;
    c.s_done = s.done;
    ds.q = s;
    hipLaunchKernelGGL(k_drop_links, dim3(grid_for(nl, Q_THREADS)), blk, 0, st, ds);
    SG_CHECK_LAUNCH();
    // (no time moved: the last iteration's walk is this order's, wt, run and the marks stand)
    TimedLaunch tl(ctx, "link_queue_ahead", (double)n);
    launch_drop_finish(ctx, ds, want_ahead);
  } else {
    {
      TimedLaunch tl(ctx, "link_queue", (double)n);
      launch_scan(ctx, s, n_tiles, serial);
    }
    if (want_ahead) {
      TimedLaunch tl(ctx, "link_queue_ahead", (double)n);
      hipLaunchKernelGGL(k_queue_ahead, g_rec, blk, 0, st, s);
      SG_CHECK_LAUNCH();
    }
  }
  if (a.wait || a.done || a.ahead) {
    hipLaunchKernelGGL(k_carry_scatter, g_rec, blk, 0, st, c, a.wait, a.done, a.ahead);
    SG_CHECK_LAUNCH();
  }
}

struct QueueCall {
  sg_ctx* ctx;
  uint32_t flags, n_links;
  const uint64_t* link_off;
  uint64_t n;
  const uint64_t* enter;
  const uint32_t* packet;
  const uint32_t* weight;
  uint32_t n_weights;
  const uint64_t* cost;
  const uint64_t* free_in;
  uint64_t* wait;
  uint64_t* done;
  uint32_t* ahead;
  uint64_t* link_free;
  uint64_t* busy;
  uint64_t* wmax;
  uint64_t* wsum;
  uint32_t* amax;
};

void queue_run(const QueueCall& c) {
  sg_ctx* ctx = c.ctx;
  if (!c.link_off || !c.enter || !c.cost) throw Error(SG_ERR_INVALID_ARG, "null link_off, enter_ns or cost_ps");
  if (!c.wait && !c.done && !c.ahead && !c.link_free && !c.busy && !c.wmax && !c.wsum && !c.amax)
    throw Error(SG_ERR_INVALID_ARG, "no output");
  if (c.weight && !c.packet) throw Error(SG_ERR_INVALID_ARG, "weight without packet");
  if (c.link_free && c.link_free == c.free_in) throw Error(SG_ERR_INVALID_ARG, "out_link_free is link_free_in");
  const bool dev = (c.flags & SG_ROUTE_OUT_DEVICE) != 0;
  const uint32_t nl = c.n_links;
  const uint64_t n = c.n;
  if (c.flags & SG_LINK_QUEUE_CARRY) {
    if (!c.packet) throw Error(SG_ERR_INVALID_ARG, "SG_LINK_QUEUE_CARRY without packet");
    // (the record index is a word of the sort's key, and UINT32_MAX is its padding)
    if (n > 0xFFFFFFFEull) throw Error(SG_ERR_CAPACITY, "more records than one carried call takes");
  }
  const bool carry = (c.flags & SG_LINK_QUEUE_CARRY) != 0 && n != 0;  // (no record: nothing to carry)
  const bool drop = (c.flags & SG_LINK_QUEUE_DROP) != 0;
  // (the period starts are u32 record indices, and the marks are summed by scan_counts)
  if (drop && n > 0xFFFFFFFEull) throw Error(SG_ERR_CAPACITY, "more records than one call with SG_LINK_QUEUE_DROP takes");
  const size_t nl2 = drop ? 2 * (size_t)nl : (size_t)nl;  // cost_ps, out_link_busy_ns, out_link_ahead_max
  if (!dev) {
    const u64 bad = bad_link_off(c.link_off, nl, n);
    if (bad != Q_MAX) throw_bad_off(bad);
  }
  const uint64_t n_tiles64 = (n + Q_TILE - 1) / Q_TILE;
  if (n_tiles64 > 0x7FFFFFFFull) throw Error(SG_ERR_CAPACITY, "more records than one call scans");
  const uint32_t n_tiles = (uint32_t)n_tiles64;
  hipStream_t st = ctx->stream;

  QArgs a = {};
  a.n_links = nl;
  a.n = n;
  a.n_weights = c.n_weights;
  // host arrays in: device copies; host outputs: device arrays copied back at the end
  struct Back {
    void* host;
    const void* dev;
    size_t bytes;
  };
  std::vector<Back> back;
  int slot = 0;
  auto in = [&](const void* p, size_t bytes) -> const void* {
    sg::DevBuf& b = ctx->q_buf[slot++];
    if (!p || dev) return p;
    char* d = b.get<char>(bytes);
    if (bytes) SG_HIP(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, st));
    return d;
  };
  auto out = [&](void* p, size_t bytes) -> void* {
    sg::DevBuf& b = ctx->q_buf[slot++];
    if (!p || dev) return p;
    char* d = b.get<char>(bytes);
    back.push_back(Back{p, d, bytes});
    return d;
  };
  a.off = (const u64*)in(c.link_off, ((size_t)nl + 1) * 8);
  a.enter = (const u64*)in(c.enter, n * 8);
  a.packet = (const uint32_t*)in(c.packet, n * 4);
  a.weight = (const uint32_t*)in(c.weight, (size_t)c.n_weights * 4);
  a.cost = (const u64*)in(c.cost, nl2 * 8);
  a.free_in = (const u64*)in(c.free_in, (size_t)nl * 8);
  a.wait = (u64*)out(c.wait, n * 8);
  a.done = (u64*)out(c.done, n * 8);
  a.ahead = (uint32_t*)out(c.ahead, n * 4);
  a.link_free = (u64*)out(c.link_free, (size_t)nl * 8);
  a.busy = (u64*)out(c.busy, nl2 * 8);
  a.wmax = (u64*)out(c.wmax, (size_t)nl * 8);
  a.wsum = (u64*)out(c.wsum, (size_t)nl * 8);
  a.amax = (uint32_t*)out(c.amax, nl2 * 4);
  const bool want_ahead = (a.ahead || a.amax);
  if (want_ahead && !a.done && !carry && !drop) a.done = ctx->q_done.get<u64>(n);
  a.flag = ctx->q_flag.get<u64>(Q_WORDS);
  SG_HIP(hipMemsetAsync(a.flag, 0xff, Q_WORDS * 8, st));

  const bool serial = knob_int("SG_LINK_QUEUE_SERIAL", 0) != 0;
  // read_timer("link_queue_serial") = (0, 1 when the last call took the lane-per-link form, its records)
  timer_set_counter(ctx, "link_queue_serial", (double)n, serial ? 1u : 0u);
  if (!serial && n) {
    u64* agg = ctx->q_agg.get<u64>(3 * (size_t)n_tiles);
    a.agg_s = agg;
    a.agg_m = agg + n_tiles;
    a.agg_h = (uint32_t*)(agg + 2 * (size_t)n_tiles);
  }
  // the (link, record in the link) of record i: link_off is valid, the host's or a copy of the device's
  std::vector<uint64_t> hoff;
  auto pair_of = [&](u64 i, uint32_t& lk, uint32_t& at) {
    const uint64_t* off = c.link_off;
    if (dev) {
      if (hoff.empty()) {
        hoff.resize((size_t)nl + 1);
        SG_HIP(hipMemcpy(hoff.data(), c.link_off, hoff.size() * 8, hipMemcpyDeviceToHost));
      }
      off = hoff.data();
    }
    lk = (uint32_t)(std::upper_bound(off + 1, off + nl + 1, (uint64_t)i) - off - 1);
    at = (uint32_t)std::min<uint64_t>(i - off[lk], 0xFFFFFFFFull);
  };
  auto throw_bad_packet = [&](u64 i) {
    uint32_t lk, at;
    pair_of(i, lk, at);
    throw Error(SG_ERR_INVALID_ARG,
                "packet[" + std::to_string(i) + "] is not below n_weights (link " + std::to_string(lk) + ")", lk, at);
  };

  DArgs d = {};
  if (drop) {
    d.q = a;
    d.limit = a.cost + nl;
    d.drops = a.amax ? a.amax + nl : nullptr;
    d.refused = a.busy ? a.busy + nl : nullptr;
    if (n) {
      d.lng_cap = (uint32_t)(n / (D_SHORT + 1u) + 1u);
      d.mark = ctx->qd_mark.get<uint32_t>(n);
      d.pos = ctx->qd_pos.get<u64>((size_t)n + 2);
      d.start = ctx->qd_start.get<uint32_t>(n);
      d.lng = ctx->qd_long.get<uint32_t>((size_t)d.lng_cap + 1);
      d.n_long = d.lng + d.lng_cap;
      d.run = ctx->qd_run.get<u64>(n);
      d.wt = ctx->qd_wait.get<u64>(n);
    }
  }

  if (carry) {
    queue_carry(ctx, a, n_tiles, serial, want_ahead, pair_of, throw_bad_packet, drop ? &d : nullptr);
  } else {
    hipLaunchKernelGGL(k_queue_links, dim3(grid_for((size_t)nl + 1, Q_THREADS)), dim3(Q_THREADS), 0, st, a);
    SG_CHECK_LAUNCH();
    if (drop) {
      hipLaunchKernelGGL(k_drop_links, dim3(grid_for(nl, Q_THREADS)), dim3(Q_THREADS), 0, st, d);
      SG_CHECK_LAUNCH();
    }
    if (n && drop) {
      {
        TimedLaunch tl(ctx, "link_queue", (double)n);
        launch_drop(ctx, d, n_tiles, serial);
      }
      TimedLaunch tl(ctx, "link_queue_ahead", (double)n);
      launch_drop_finish(ctx, d, want_ahead);
    } else if (n) {
      TimedLaunch tl(ctx, "link_queue", (double)n);
      launch_scan(ctx, a, n_tiles, serial);
    }
    if (n && want_ahead && !drop) {
      TimedLaunch tl(ctx, "link_queue_ahead", (double)n);
      hipLaunchKernelGGL(k_queue_ahead, dim3(grid_for(n, Q_THREADS, 0x7FFFFFFFu)), dim3(Q_THREADS), 0, st, a);
      SG_CHECK_LAUNCH();
    }
    u64 h[Q_WORDS];
    copy_to_host(ctx, h, a.flag, sizeof(h));
    if (h[Q_BAD_OFF] != Q_MAX) throw_bad_off(h[Q_BAD_OFF]);
    if (h[Q_BAD_PACKET] != Q_MAX) throw_bad_packet(h[Q_BAD_PACKET]);
    if (h[Q_OVERFLOW] != Q_MAX) {
      const u64 i = h[Q_OVERFLOW];
      uint32_t lk, at;
      pair_of(i, lk, at);
      throw Error(SG_ERR_TIME_OVERFLOW,
                  "record " + std::to_string(i) + " of link " + std::to_string(lk) + " is served past 2^64 - 1 ns", lk, at);
    }
  }
  for (const Back& b : back)
    if (b.bytes) SG_HIP(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st));
  if (!back.empty()) SG_HIP(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace sg

extern "C" {

int32_t sg_link_queue(sg_ctx* ctx, uint32_t flags, uint32_t n_links, const uint64_t* link_off, uint64_t n_records,
                      const uint64_t* enter_ns, const uint32_t* packet, const uint32_t* weight, uint32_t n_weights,
                      const uint64_t* cost_ps, const uint64_t* link_free_in, uint64_t* out_wait_ns,
                      uint64_t* out_done_ns, uint32_t* out_ahead, uint64_t* out_link_free, uint64_t* out_link_busy_ns,
                      uint64_t* out_link_wait_max_ns, uint64_t* out_link_wait_sum_ns, uint32_t* out_link_ahead_max) {
  return sg::guarded(ctx, [&] {
    sg::queue_run(sg::QueueCall{ctx, flags, n_links, link_off, n_records, enter_ns, packet, weight, n_weights, cost_ps,
                                link_free_in, out_wait_ns, out_done_ns, out_ahead, out_link_free, out_link_busy_ns,
                                out_link_wait_max_ns, out_link_wait_sum_ns, out_link_ahead_max});
  });
}

}  // extern "C"
