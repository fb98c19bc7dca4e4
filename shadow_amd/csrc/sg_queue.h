// sg_queue.h -- what the three layers of the link queues share: the first-order scan (sg_queue.hip),
// finite buffers on top of it (sg_queue_drop.hip) and the carried form on top of both
// (sg_queue_carry.hip).  Device code, and the host entry points one layer calls in another: no
// kernel is launched across the files.
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
// The *tile carry* is the `done` that enters a tile of the scan (k_queue_carry); *carried* is the flag's form.
#pragma once

#include <cstddef>

#include "sg_internal.h"
#include "sg_scan.h"

namespace sg {

using u64 = unsigned long long;

constexpr uint32_t Q_THREADS = 256;
constexpr uint32_t Q_PER = 8;  // consecutive records per lane
constexpr uint32_t Q_TILE = Q_THREADS * Q_PER;
constexpr u64 Q_MAX = ~0ull;
constexpr uint32_t Q_NO_LINK = 0xFFFFFFFFu;

// flag words (all ones: nothing found; the smallest value wins)
// (the carried form adds Q_DUP, the smallest record with a twin in its packet's chain, and
// Q_CHANGED, 0 once an iteration moved an enter time; the packet pass adds Q_PKT_OVERFLOW, the
// smallest packet whose first-order arrival is past the range, and Q_LOST, a count from 0: the
// packets dropped; the windowed form adds Q_ACTIVE, no flag but a count: the records below the horizon
// as the last compaction found them, read with the others in the iteration's one read; the time series
// adds Q_BAD_SLOT, the smallest link whose slot is neither below the slots nor all ones)
enum { Q_BAD_OFF = 0, Q_BAD_PACKET = 1, Q_OVERFLOW = 2, Q_DUP = 3, Q_CHANGED = 4, Q_PKT_OVERFLOW = 5, Q_LOST = 6, Q_ACTIVE = 7, Q_BAD_SLOT = 8, Q_WORDS = 9 };

// The outputs of a pass (null: not written), per record in the view's order and per link.
struct QOuts {
  u64* wait;
  u64* done;  // the caller's, or the scratch array k_queue_ahead reads, or null
  uint32_t* ahead;
  u64* link_free;
  u64* busy;
  u64* wmax;
  u64* wsum;
  uint32_t* amax;
};

// One pass over the records.  Built once, by queue_pass(), and const from there on: a kernel sees
// the arrays its pass was built with.
struct QArgs {
  const u64* off;
  uint32_t n_links;
  u64 n;
  const u64* enter;  // the view (enter, packet): the input order, or the order a carried iteration sorted
  const uint32_t* packet;
  const uint32_t* weight;
  uint32_t n_weights;
  const u64* cost;
  const u64* free_in;
  QOuts out;
  u64* flag;
  // the tile aggregates (null: the lane-per-link form); agg_m becomes the `done` entering each tile
  u64* agg_s;
  u64* agg_m;
  uint32_t* agg_h;
};

// (the kernels of every layer take the struct by value: a field added here moves their arguments)
static_assert(sizeof(QArgs) == 168 && offsetof(QArgs, out) == 72 && offsetof(QArgs, flag) == 136, "QArgs keeps its layout");

// A pass of the call `call` over the view (enter, packet) that writes `outs`.
inline QArgs queue_pass(QArgs call, const u64* enter, const uint32_t* packet, const QOuts& outs) {
  call.enter = enter;
  call.packet = packet;
  call.out = outs;
  return call;
}
// (host side: the tiles of the scan form, and whether the pass takes the lane-per-link form)
inline uint32_t queue_tiles(const QArgs& a) { return (uint32_t)((a.n + Q_TILE - 1) / Q_TILE); }
inline bool queue_serial(const QArgs& a) { return !a.agg_s; }

// ---- host entry points across the layers: each queues on the context stream and waits for nothing
// unless it says so.  carried_run: a walk under the drop rule keeps `run`, the `done` after every
// record, in an array of the drop layer's own (null) or, carried, in the sorted pass's done array;
// the records whose enter time is all ones are then absent.  k_drop_finish reads run while it
// writes the pass's done: the two are never one array (sg_queue_carry.hip's sorted_outs).
struct QLocator;  // sg_queue.hip: the (link, record in the link) of a record, for an error's pair; the packets lost
// sg_queue.hip.  launch_links: link_off's check, the zeroes of the pass's per-link outputs.
// launch_walk (timer link_queue): wait, done and the per-link sums in the scan or the serial form, or
// under the drop rule the walk's three arrays, whose wt it returns.  queue_output_pass: the links,
// the walk unless `walk_stands` (the last walk was this view's and holds), ahead (timer
// link_queue_ahead).  queue_check_flags reads the flag words back -- it waits for the stream -- and
// throws the first error: with `inputs` a bad link_off, packet index or twin; an overflow
// (`carried`: its message), the packet pass's too.  True: no enter time moved.  active: Q_ACTIVE's value.
void launch_links(sg_ctx* ctx, const QArgs& a);
const u64* launch_walk(sg_ctx* ctx, const QArgs& a, bool drop, u64* carried_run);
void queue_output_pass(sg_ctx* ctx, const QArgs& a, bool drop, u64* carried_run, bool walk_stands);
bool queue_check_flags(sg_ctx* ctx, const u64* flag, QLocator& where, bool carried, bool inputs, u64* active = nullptr);
// sg_queue_drop.hip.  The walk expects the tile carries of `a` in a.agg_m (the scan form).
void drop_launch_links(sg_ctx* ctx, const QArgs& a);
const u64* drop_launch_walk(sg_ctx* ctx, const QArgs& a, u64* carried_run);  // the walk's waits
void drop_launch_finish(sg_ctx* ctx, const QArgs& a, u64* carried_run);
// sg_queue_carry.hip.  `a`: the call on the device (n > 0, flag words all ones), every output the caller takes.
// packets: the packet pass follows, and one more read of the flag words after it.
void queue_carry(sg_ctx* ctx, const QArgs& a, bool drop, bool packets, QLocator& where);
// The index step alone (timer link_queue_index; it also bounds packet[i] by a.n_weights): packet p's records
// are list[pkt_off[p]] .. list[pkt_off[p + 1]], in ascending input (enter, record) order.
struct QChains {
  const u64* pkt_off;
  const uint32_t* list;
};
QChains queue_packet_lists(sg_ctx* ctx, const QArgs& a);
// sg_queue_packets.hip (SG_LINK_QUEUE_PACKETS).  `a`: the call, its per-record outputs written at the input
// indices, n_weights packets behind the n records of enter, wait, done and ahead.  next: the carried
// form's chain successors at input indices, null first order.  prev: the windowed form's chain
// predecessors (null: not windowed): a record whose wait is all ones and whose ahead is 0xFFFFFFFF is
// pending, and its packet in flight.
void queue_packets(sg_ctx* ctx, const QArgs& a, bool drop, const uint32_t* next, const uint32_t* prev = nullptr);
// sg_queue_window.hip (SG_LINK_QUEUE_WINDOW over the carried form).  `a` as queue_carry's, a.free_in with
// the horizon behind the links' entries.
void queue_window(sg_ctx* ctx, const QArgs& a, bool drop, bool packets, QLocator& where);
// sg_queue_series.hip (SG_LINK_QUEUE_SERIES).  queue_series_plan: the four header words behind cost_ps'
// c0 entries (cost_tail; dev: device memory, read back, which waits for the stream), checked, and in
// host mode the slot map behind them.  queue_series (timer link_queue_series): `a` the call, its
// per-record outputs written at the input indices, the slot map behind the header in a.cost and the
// matrix behind the c0 entries of a.out.busy; it adds into the matrix and flags a bad slot value in
// Q_BAD_SLOT, which queue_check_flags reports after every other error.
struct QSeries {
  u64 t0, bin;
  uint32_t n_bins, n_slots;  // n_slots: S, n_links under the identity map
  bool mapped;               // a slot per link follows the header
  u64 cells;                 // S (n_bins + 2), a plane of the matrix
};
QSeries queue_series_plan(sg_ctx* ctx, const u64* cost_tail, bool dev, uint32_t n_links);
void queue_series(sg_ctx* ctx, const QArgs& a, const QSeries& s, bool drop, bool window);

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

// The first index in [lo, hi) whose value exceeds x, hi when there is none (p never falls there).
template <class I>
__device__ __forceinline__ I upper_bound(const u64* p, I lo, I hi, u64 x) {
  while (lo < hi) {
    const I mid = lo + (hi - lo) / 2;
    if (p[mid] > x)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// The link that owns record i < n of a valid link_off: the L with off[L] <= i < off[L + 1].
__device__ __forceinline__ uint32_t link_of(const u64* __restrict__ off, uint32_t n_links, u64 i) {
  // the first L' in [1, n_links] with off[L'] > i (off[n_links] = n > i)
  return upper_bound(off, 1u, n_links, i) - 1;
}

__device__ __forceinline__ u64 link_free_in(const QArgs& a, uint32_t lk) { return a.free_in ? a.free_in[lk] : 0ull; }

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
      acc = QElem{s, sat_add(max(e, link_free_in(a, c.link)), s), 1u};
    } else {
      acc = QElem{sat_add(acc.s, s), sat_add(max(acc.m, e), s), acc.head};
    }
    if (i + 1 == c.end) r.last |= 1u << k;
    head = false;
  }
  return acc;
}

// ---- the tile again, with its tile carry (a.agg_m, after k_queue_carry): the lane's records into r,
// then body(k, start, done) for each in order: the unlimited queue's start of record base + k (its
// link's free_in enters at a segment's first record) and its `done`, each computed once.  Every
// thread of the workgroup calls; s_wave: 16 elements of LDS.
template <class Body>
__device__ __forceinline__ void tile_rescan(const QArgs& a, QElem* s_wave, u64 base, QLane& r, const Body& body) {
  const QElem x = lane_load<false>(a, base, r);
  QElem total;
  const QElem ex = block_exclusive_op(x, q_identity(), s_wave, &total, QOp());
  // (ex.head: a segment starts in the tile below this lane, the tile carry does not reach it)
  u64 done = ex.head ? ex.m : max(sat_add(a.agg_m[blockIdx.x], ex.s), ex.m);
#pragma unroll
  for (uint32_t k = 0; k < Q_PER; k++) {
    if (k >= r.count) continue;
    if ((r.head >> k) & 1u) done = link_free_in(a, r.link[k]);
    const u64 start = max(r.e[k], done);
    done = sat_add(start, r.s[k]);
    body(k, start, done);
  }
}

// ---- a wave's segmented reduction by key: equal keys sit in consecutive lanes (links rise with
// the record index); afterwards the first lane of a run of equal keys holds op over the run.  As in
// sg_scan.h an element type T supplies its shuffle, run_shfl_down(T, d), and an operator.  Every
// lane calls.
template <class T>
__device__ __forceinline__ T run_shfl_down(T x, uint32_t d) { return __shfl_down(x, d, 64); }

// A link's (busy, wait max, wait sum) as one element: the key is shuffled once per step.
struct QSums {
  u64 busy, wmax, wsum;
};

__device__ __forceinline__ QSums run_shfl_down(QSums x, uint32_t d) {
  return QSums{__shfl_down(x.busy, d, 64), __shfl_down(x.wmax, d, 64), __shfl_down(x.wsum, d, 64)};
}

struct QSumsOp {
  __device__ __forceinline__ QSums operator()(const QSums& a, const QSums& b) const {
    return QSums{a.busy + b.busy, max(a.wmax, b.wmax), a.wsum + b.wsum};
  }
};

template <class T, class Op>
__device__ __forceinline__ T wave_run_reduce(uint32_t key, T x, Op op) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t k2 = __shfl_down(key, d, 64);
    const T y = run_shfl_down(x, d);
    const T z = op(x, y);
    if (lane + d < 64 && k2 == key) x = z;
  }
  return x;
}

// The first lane of a run whose key is a link.  Every lane calls.
__device__ __forceinline__ bool wave_run_first(uint32_t key) {
  const uint32_t below = __shfl_up(key, 1, 64);
  return key != Q_NO_LINK && ((threadIdx.x & 63u) == 0 || below != key);
}

}  // namespace sg
