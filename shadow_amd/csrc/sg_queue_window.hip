// sg_queue_window.hip -- link queues, the windowed form (SG_LINK_QUEUE_WINDOW): the carried form settled up
// to a horizon H = link_free_in[n_links], the rest handed back as pending.  A layer over the carried
// form's index step (sg_queue_carry.hip), the scan and, under SG_LINK_QUEUE_DROP, the drop walk (sg_queue.h).
//
// A link serves in (carried enter, packet) order, and a record's start, its drop decision and its done
// depend on earlier records of that order alone: the records below H are a fixed point of their own.
// Every iteration therefore sorts and scans a compact view, the records whose carried time is below H.
//
// Set-up, once: the packets' lists (queue_packet_lists), then k_window_chain: next, prev, gap and
// cur = enter.
// An iteration, a lane per record unless said otherwise:
//   k_window_mark       act[i] = cur[i] < H and the chain predecessor's cur (if any) is below H too.  It
//                       writes no time: every lane sees the times the iteration started from;
//   scan_counts         the marks' exclusive sums: the place of every active record, in input order, so
//                       the compact view is grouped by link as the input is;
//   k_window_fill       the compact keys (cur, packet, record) and the compact link offsets
//                       (pos[link_off[L]]), the count into the flag word Q_ACTIVE.  A record that is not
//                       active although its time is below H stands behind a record that left the
//                       window (moved to or past H, dropped, absent): its time is stale, and it becomes
//                       its predecessor's plus the gap, which is at or past H.  The predecessor's lane
//                       does not write in this launch (its time is not below H): one writer per cell;
//   the segmented sort by link over the compact offsets, launch_walk on the compact view;
//   k_window_propagate  a lane per compact record: cur[next] = done + gap, all ones behind a record
//                       that is not served.
// The host reads the flag words once per iteration, after the marks, the sums and the fill of the
// *next* one: they tell whether a time moved and how many records the next sort takes.  When none
// moved the compact view is the settled records, each with its closed-solution values:
//   queue_output_pass   over the compact view: the caller's per-link outputs run over settled records;
//   k_window_scatter    a lane per compact record: wait, done and ahead to the input index; where its
//                       successor is not in the view, the lane walks the rest of the chain: absent
//                       behind a dropped record, else pending with the re-based times r, r + gap, ...;
//   k_window_heads      a lane per record: a chain's first record at or past H walks its chain alike.
// Every record is written by one lane: a chain's settled records are a prefix of it.  A walk is a
// loop over a path's hops and is cut at n steps.
// No index is formed from a value that was not checked, as in the carried form.
#include "sg_knobs.h"
#include "sg_queue.h"
#include "sg_segsort.h"

namespace sg {
namespace {

constexpr uint32_t W_NONE = 0xFFFFFFFFu;  // no successor, no predecessor; a pending record's ahead

struct WArgs {
  u64 n;
  uint32_t n_packets, n_links;
  const u64* off;  // the caller's link_off
  const u64* enter;
  const uint32_t* packet;
  const u64* pkt_off;
  const uint32_t* list;
  const u64* horizon;
  uint32_t* next;
  uint32_t* prev;
  u64* gap;
  u64* cur;
  uint32_t* act;
  u64* pos;   // n + 2: the exclusive sums of act, the total twice
  u64* coff;  // the compact view's link offsets
  uint4* key;
  const uint32_t* perm;  // compact sorted place -> record
  u64* flag;
};

__device__ __forceinline__ bool window_bad(const WArgs& w) {
  return w.flag[Q_BAD_OFF] != Q_MAX || w.flag[Q_BAD_PACKET] != Q_MAX;
}

__global__ void __launch_bounds__(Q_THREADS) k_window_chain(const WArgs w) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= w.n || window_bad(w)) return;
  const uint32_t i = w.list[j];
  if (i >= w.n) return;
  const uint32_t p = w.packet[i];
  if (p >= w.n_packets) return;
  const u64 e = w.enter[i];
  uint32_t nx = W_NONE, pv = W_NONE;
  u64 g = 0ull;
  if (j + 1 < w.pkt_off[p + 1]) {
    nx = w.list[j + 1];
    if (nx >= w.n) {
      nx = W_NONE;
    } else {
      g = w.enter[nx] - e;  // (the list is ascending)
      if (g == 0ull) atomicMin(&w.flag[Q_DUP], (u64)i);
    }
  }
  if (j > w.pkt_off[p]) {
    pv = w.list[j - 1];
    if (pv >= w.n) pv = W_NONE;
  }
  w.next[i] = nx;
  w.prev[i] = pv;
  w.gap[i] = g;
  w.cur[i] = e;
}

__global__ void __launch_bounds__(Q_THREADS) k_window_mark(const WArgs w) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= w.n) return;
  uint32_t act = 0u;
  if (!window_bad(w)) {
    const u64 h = *w.horizon;
    const uint32_t pv = w.prev[i];
    act = w.cur[i] < h && (pv >= w.n || w.cur[pv] < h) ? 1u : 0u;  // (pv: W_NONE or below n)
  }
  w.act[i] = act;
}

// (the grid covers the records and the n_links + 1 compact offsets)
__global__ void __launch_bounds__(Q_THREADS) k_window_fill(const WArgs w) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (window_bad(w)) return;
  if (i <= w.n_links) {
    const u64 o = i < w.n_links ? w.off[i] : w.n;
    w.coff[i] = w.pos[min(o, w.n)];  // (link_off is valid: the min changes nothing)
    if (i == 0) w.flag[Q_ACTIVE] = w.pos[w.n];
  }
  if (i >= w.n) return;
  const u64 c = w.cur[i];
  if (w.act[i]) {
    const u64 at = w.pos[i];
    if (at < w.n) w.key[at] = make_uint4((uint32_t)c, (uint32_t)(c >> 32), w.packet[i], (uint32_t)i);
    return;
  }
  if (c >= *w.horizon) return;
  const uint32_t pv = w.prev[i];  // (below n, its time at or past H: k_window_mark found the record stale)
  if (pv >= w.n) return;
  w.cur[i] = sat_add(w.cur[pv], w.gap[pv]);
  w.flag[Q_CHANGED] = 0ull;
}

// done: the compact sorted pass's.  wt: null, or under SG_LINK_QUEUE_DROP the walk's waits (all ones: dropped).
__global__ void __launch_bounds__(Q_THREADS) k_window_propagate(const WArgs w, u64 n_view, const u64* done, const u64* wt) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= n_view) return;
  const bool served = !wt || wt[j] != Q_MAX;
  const uint32_t i = w.perm[j];
  if (i >= w.n) return;
  const uint32_t nx = w.next[i];
  if (nx >= w.n) return;
  const u64 old = w.cur[nx];
  u64 v = Q_MAX;
  if (served) {
    v = sat_add(done[j], w.gap[i]);
    if (v == Q_MAX) atomicMin(&w.flag[Q_OVERFLOW], j);
  }
  if (v != old) {
    w.cur[nx] = v;
    w.flag[Q_CHANGED] = 0ull;
  }
}

// The chain from record k on: absent, or pending with the re-based times r, r + gap, ...
__device__ __forceinline__ void window_tail(const WArgs& w, const QOuts& to, uint32_t k, u64 r, bool absent) {
  for (u64 steps = 0; k < w.n && steps < w.n; steps++) {
    if (!absent && r == Q_MAX) atomicMin(&w.flag[Q_OVERFLOW], (u64)k);
    if (to.wait) to.wait[k] = Q_MAX;
    if (to.done) to.done[k] = absent ? Q_MAX : r;
    if (to.ahead) to.ahead[k] = absent ? 0u : W_NONE;
    r = sat_add(r, w.gap[k]);
    k = w.next[k];
  }
}

__global__ void __launch_bounds__(Q_THREADS) k_window_scatter(const WArgs w, u64 n_view, const QOuts sorted, const QOuts to,
                                                             const u64* wt) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= n_view) return;
  const uint32_t i = w.perm[j];
  if (i >= w.n) return;
  if (to.wait) to.wait[i] = sorted.wait[j];
  if (to.done) to.done[i] = sorted.done[j];
  if (to.ahead) to.ahead[i] = sorted.ahead[j];
  const uint32_t nx = w.next[i];
  if (nx >= w.n) return;
  const u64 c = w.cur[nx];
  if (c < *w.horizon) return;  // (settled: a lane of its own)
  window_tail(w, to, nx, c, wt && wt[j] == Q_MAX);
}

__global__ void __launch_bounds__(Q_THREADS) k_window_heads(const WArgs w, const QOuts to) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= w.n || window_bad(w)) return;
  if (w.prev[i] < w.n) return;
  const u64 c = w.cur[i];
  if (c < *w.horizon) return;
  window_tail(w, to, (uint32_t)i, c, false);
}

}  // namespace

void queue_window(sg_ctx* ctx, const QArgs& a, bool drop, bool packets, QLocator& where) {
  hipStream_t st = ctx->stream;
  const u64 n = a.n;
  const uint32_t nl = a.n_links;
  const int cap = knob_int("SG_LINK_QUEUE_CARRY_ITERS", 4096, 1, INT_MAX);
  const dim3 blk(Q_THREADS), g_rec(grid_for(n, Q_THREADS, 0x7FFFFFFFu));
  const dim3 g_fill(grid_for(std::max<size_t>((size_t)n, (size_t)nl + 1), Q_THREADS, 0x7FFFFFFFu));

  const uint32_t piece = (uint32_t)knob_int("SG_LINK_TRACE_PIECE", (int)TR_PIECE_MAX, (int)TR_RANK_MAX, (int)TR_PIECE_MAX);
  const uint64_t work_cap64 = segsort_work_cap(n, piece);
  if (work_cap64 > 0xFFFFFFFFull) throw Error(SG_ERR_CAPACITY, "more records than one carried call sorts");
  const uint32_t work_cap = (uint32_t)work_cap64;

  u64* s_enter = ctx->qc_enter.get<u64>(n);
  uint32_t* s_packet = ctx->qc_packet.get<uint32_t>(n);
  uint32_t* perm = ctx->qc_perm.get<uint32_t>(n);
  const TraceOut sorted = {s_packet, perm, s_enter, nullptr};
  if (drop) {  // (the drop layer sizes its arrays by the view: at their largest now, none grows in the loop)
    ctx->qd_mark.get<uint32_t>(n);
    ctx->qd_pos.get<u64>((size_t)n + 2);
    ctx->qd_start.get<uint32_t>(n);
    ctx->qd_long.get<uint32_t>((size_t)n / 33 + 2);
    ctx->qd_wait.get<u64>(n);
  }

  launch_links(ctx, queue_pass(a, a.enter, a.packet, QOuts{}));  // (link_off's check alone)
  const QChains lists = queue_packet_lists(ctx, a);
  WArgs w = {};
  w.n = n;
  w.n_packets = a.n_weights;
  w.n_links = nl;
  w.off = a.off;
  w.enter = a.enter;
  w.packet = a.packet;
  w.pkt_off = lists.pkt_off;
  w.list = lists.list;
  w.horizon = a.free_in + nl;
  w.next = ctx->qc_next.get<uint32_t>(n);
  w.prev = ctx->qw_prev.get<uint32_t>(n);
  w.gap = ctx->qc_gap.get<u64>(n);
  w.cur = ctx->qc_cur.get<u64>(n);
  w.act = ctx->qw_act.get<uint32_t>(n);
  w.pos = ctx->qw_pos.get<u64>((size_t)n + 2);
  w.coff = ctx->qw_off.get<u64>((size_t)nl + 1);
  w.key = ctx->tr_key.get<uint4>(n);  // (the index step is done with the three: the stream orders the two)
  uint4* key2 = ctx->tr_key2.get<uint4>(n);
  uint2* work = ctx->tr_work.get<uint2>(work_cap);
  uint32_t* n_work = ctx->qw_ctr.get<uint32_t>(1);
  w.perm = perm;
  w.flag = a.flag;

  // the marks, their sums and the fill: the view of the iteration that follows
  const auto compact = [&] {
    hipLaunchKernelGGL(k_window_mark, g_rec, blk, 0, st, w);
    SG_CHECK_LAUNCH();
    scan_counts(ctx, w.act, (uint32_t)n, w.pos, w.pos + n + 1);
    hipLaunchKernelGGL(k_window_fill, g_fill, blk, 0, st, w);
    SG_CHECK_LAUNCH();
  };
  {
    TimedLaunch tl(ctx, "link_queue_index", (double)n);
    hipLaunchKernelGGL(k_window_chain, g_rec, blk, 0, st, w);
    SG_CHECK_LAUNCH();
    compact();
  }
  u64 n_view = 0;
  queue_check_flags(ctx, a.flag, where, true, true, &n_view);
  if (n_view > n) throw Error(SG_ERR_DEVICE, "the windowed form counted more active records than the call has");

  QArgs view = a;
  view.off = w.coff;
  QOuts iter_outs = {};
  iter_outs.done = ctx->qc_done.get<u64>(n);
  u64* run = drop ? iter_outs.done : nullptr;  // (sg_queue.h: carried_run)
  const u64* wt = nullptr;

  uint32_t iters = 0;
  u64 active = 0;
  bool settled = false;
  while (!settled && iters < (uint32_t)cap) {
    iters++;
    active += n_view;
    SG_HIP(hipMemsetAsync(a.flag + Q_CHANGED, 0xff, 8, st));
    if (n_view) {
      view.n = n_view;
      const QArgs iter = queue_pass(view, s_enter, s_packet, iter_outs);
      const dim3 g_view(grid_for(n_view, Q_THREADS, 0x7FFFFFFFu));
      SG_HIP(hipMemsetAsync(n_work, 0, 4, st));
      {
        TimedLaunch tl(ctx, "link_queue_sort", (double)n_view);
        segsort_enqueue(ctx, w.coff, nl, (const uint4*)w.key, nullptr, key2, nullptr, sorted, piece, work, work_cap, n_work);
      }
      wt = launch_walk(ctx, iter, drop, run);
      TimedLaunch tl(ctx, "link_queue_carry", (double)n_view);
      hipLaunchKernelGGL(k_window_propagate, g_view, blk, 0, st, w, n_view, (const u64*)iter_outs.done, wt);
      SG_CHECK_LAUNCH();
    }
    {
      TimedLaunch tl(ctx, "link_queue_window", (double)n);
      compact();
    }
    timer_set_counter(ctx, "link_queue_iters", (double)n, iters, true);
    timer_set_counter(ctx, "link_queue_active", (double)n, active, true);
    u64 n_next = 0;
    settled = queue_check_flags(ctx, a.flag, where, true, false, &n_next);
    if (n_next > n) throw Error(SG_ERR_DEVICE, "the windowed form counted more active records than the call has");
    if (!settled) n_view = n_next;  // (settled: nothing moved, the next view is this one)
  }
  if (!settled)
    throw Error(SG_ERR_CAPACITY,
                "the carried times still moved after " + std::to_string(iters) + " iterations (SG_LINK_QUEUE_CARRY_ITERS)",
                iters, 0xFFFFFFFFu);

  // the last pass over the compact view, as the carried form's over all records
  view.n = n_view;
  QOuts last_outs = a.out;  // (the per-link outputs are the caller's)
  last_outs.done = drop ? (a.out.done ? ctx->qd_done.get<u64>(n) : nullptr) : iter_outs.done;
  last_outs.wait = a.out.wait ? ctx->qc_wait.get<u64>(n) : nullptr;
  last_outs.ahead = a.out.ahead ? ctx->qc_ahead.get<uint32_t>(n) : nullptr;
  const QArgs last = queue_pass(view, s_enter, s_packet, last_outs);
  queue_output_pass(ctx, last, drop, run, drop);
  {
    TimedLaunch tl(ctx, "link_queue_window", (double)n);
    if (n_view) {
      hipLaunchKernelGGL(k_window_scatter, dim3(grid_for(n_view, Q_THREADS, 0x7FFFFFFFu)), blk, 0, st, w, n_view, last_outs,
                         a.out, drop ? wt : nullptr);
      SG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_window_heads, g_rec, blk, 0, st, w, a.out);
    SG_CHECK_LAUNCH();
  }
  if (packets) queue_packets(ctx, a, drop, w.next, w.prev);
  // (a re-based time past the range, and the packet pass's arrivals)
  queue_check_flags(ctx, a.flag, where, true, false);
}

}  // namespace sg
