// sg_queue_carry.hip -- link queues, the carried form (SG_LINK_QUEUE_CARRY): a wait moves the packet's
// later hops.  A layer over sg_queue.hip and, under SG_LINK_QUEUE_DROP, sg_queue_drop.hip (sg_queue.h).
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
#include "sg_knobs.h"
#include "sg_queue.h"
#include "sg_segsort.h"

namespace sg {
namespace {

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
  const uint32_t* perm;  // sorted place -> record, as the last sort by link left it
  u64* flag;
};

// (the kernels take the struct by value: a field added here moves their arguments)
static_assert(sizeof(CArgs) == 112 && offsetof(CArgs, next) == 72, "CArgs keeps its layout");

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

// done: the sorted pass's.  wt: null, or under SG_LINK_QUEUE_DROP the walk's waits: the successor
// of a record that is not served (wt all ones: dropped or absent) is absent, cur = MAX; only a
// served record can carry past 2^64 - 1.
__global__ void __launch_bounds__(Q_THREADS) k_carry_propagate(const CArgs c, const u64* done, const u64* wt) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= c.n) return;
  const bool served = !wt || wt[j] != Q_MAX;  // (wt: the same for every lane of the launch)
  const uint32_t i = c.perm[j];
  if (i >= c.n) return;
  const uint32_t nx = c.next[i];
  if (nx == Q_NO_NEXT) return;  // (else below n: k_carry_chain checked it)
  const u64 old = c.cur[nx];  // (in flight beside the loads below)
  u64 v = Q_MAX;
  if (served) {
    v = sat_add(done[j], c.gap[i]);
    if (v == Q_MAX) atomicMin(&c.flag[Q_OVERFLOW], j);
  }
  if (v != old) {
    c.cur[nx] = v;
    c.flag[Q_CHANGED] = 0ull;
  }
}

// The sorted pass's wait, done and ahead to the input indices (`to`: the caller's, null: not taken).
__global__ void __launch_bounds__(Q_THREADS) k_carry_scatter(const CArgs c, const QOuts sorted, const QOuts to) {
  const u64 j = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (j >= c.n) return;
  const uint32_t i = c.perm[j];
  if (i >= c.n) return;
  if (to.wait) to.wait[i] = sorted.wait[j];
  if (to.done) to.done[i] = sorted.done[j];
  if (to.ahead) to.ahead[i] = sorted.ahead[j];
}

// The chains of the call `a` (ctr: 2 n_packets zeroed words; pkt_off, key: the set-up's scratch) and
// the order `perm` every sort by link leaves.
CArgs carry_args(sg_ctx* ctx, const QArgs& a, uint32_t* ctr, const u64* pkt_off, uint4* key, const uint32_t* perm) {
  CArgs c = {};
  c.n = a.n;
  c.n_packets = a.n_weights;
  c.enter = a.enter;
  c.packet = a.packet;
  c.cnt = ctr;
  c.fill = ctr + a.n_weights;
  c.pkt_off = pkt_off;
  c.key = key;
  c.list = ctx->qc_list.get<uint32_t>(a.n);
  c.next = ctx->qc_next.get<uint32_t>(a.n);
  c.gap = ctx->qc_gap.get<u64>(a.n);
  c.cur = ctx->qc_cur.get<u64>(a.n);
  c.perm = perm;
  c.flag = a.flag;
  return c;
}

// What a link-sorted pass writes.  An iteration writes done alone, into the array that is also a
// walk's `run` under the drop rule.  The last pass writes every output the caller takes, per
// record in sorted order for k_carry_scatter; under the drop rule k_drop_finish reads run while it
// writes done, so there the last pass's done has an array of its own.
QOuts sorted_outs(sg_ctx* ctx, const QArgs& a, bool last, bool drop) {
  QOuts o = last ? a.out : QOuts{};  // (the per-link outputs are the caller's)
  o.done = ctx->qc_done.get<u64>(a.n);
  if (!last) return o;
  o.wait = a.out.wait ? ctx->qc_wait.get<u64>(a.n) : nullptr;
  o.ahead = a.out.ahead ? ctx->qc_ahead.get<uint32_t>(a.n) : nullptr;
  if (drop) o.done = a.out.done ? ctx->qd_done.get<u64>(a.n) : nullptr;
  return o;
}

// The index step (timer link_queue_index): every packet's records in ascending input (enter, record)
// order in c.list, packet p's at c.pkt_off[p] .. c.pkt_off[p + 1], and with `chain` next, gap and cur.
struct CIndex {
  CArgs c;
  uint4* key2;
  uint2* work;
  uint32_t work_cap, piece;
  uint32_t* n_work;
};

CIndex carry_index(sg_ctx* ctx, const QArgs& a, const uint32_t* perm, bool chain) {
  hipStream_t st = ctx->stream;
  const u64 n = a.n;
  const uint32_t np = a.n_weights;
  CIndex x = {};
  x.piece = (uint32_t)knob_int("SG_LINK_TRACE_PIECE", (int)TR_PIECE_MAX, (int)TR_RANK_MAX, (int)TR_PIECE_MAX);
  const uint64_t work_cap64 = segsort_work_cap(n, x.piece);
  if (work_cap64 > 0xFFFFFFFFull) throw Error(SG_ERR_CAPACITY, "more records than one carried call sorts");
  x.work_cap = (uint32_t)work_cap64;
  const dim3 g_rec(grid_for(n, Q_THREADS, 0x7FFFFFFFu)), blk(Q_THREADS);
  // the counters and the cursors per packet and the sort's work counter: one block, zeroed
  uint32_t* ctr = ctx->qc_cnt.get<uint32_t>(2 * (size_t)np + 1);
  SG_HIP(hipMemsetAsync(ctr, 0, (2 * (size_t)np + 1) * 4, st));
  x.n_work = ctr + 2 * (size_t)np;
  u64* pkt_off = ctx->qc_off.get<u64>((size_t)np + 2);  // (the last word: the scan's total)
  uint4* key = ctx->tr_key.get<uint4>(n);
  x.key2 = ctx->tr_key2.get<uint4>(n);
  x.work = ctx->tr_work.get<uint2>(x.work_cap);
  x.c = carry_args(ctx, a, ctr, pkt_off, key, perm);
  const CArgs& c = x.c;
  TimedLaunch tl(ctx, "link_queue_index", (double)n);
  hipLaunchKernelGGL(k_carry_count, g_rec, blk, 0, st, c);
  SG_CHECK_LAUNCH();
  scan_counts(ctx, c.cnt, np, pkt_off, pkt_off + np + 1);
  hipLaunchKernelGGL(k_carry_fill, g_rec, blk, 0, st, c);
  SG_CHECK_LAUNCH();
  const TraceOut lists = {c.list, nullptr, nullptr, nullptr};
  segsort_enqueue(ctx, pkt_off, np, (const uint4*)key, nullptr, x.key2, nullptr, lists, x.piece, x.work, x.work_cap, x.n_work);
  if (chain) {
    hipLaunchKernelGGL(k_carry_chain, g_rec, blk, 0, st, c);
    SG_CHECK_LAUNCH();
  }
  return x;
}

}  // namespace

QChains queue_packet_lists(sg_ctx* ctx, const QArgs& a) {
  const CIndex x = carry_index(ctx, a, nullptr, false);
  return QChains{x.c.pkt_off, x.c.list};
}

void queue_carry(sg_ctx* ctx, const QArgs& a, bool drop, bool packets, QLocator& where) {
  hipStream_t st = ctx->stream;
  const u64 n = a.n;
  const uint32_t nl = a.n_links;
  const int cap = knob_int("SG_LINK_QUEUE_CARRY_ITERS", 4096, 1, INT_MAX);
  const dim3 g_rec(grid_for(n, Q_THREADS, 0x7FFFFFFFu)), blk(Q_THREADS);

  u64* s_enter = ctx->qc_enter.get<u64>(n);
  uint32_t* s_packet = ctx->qc_packet.get<uint32_t>(n);
  uint32_t* perm = ctx->qc_perm.get<uint32_t>(n);
  const TraceOut sorted = {s_packet, perm, s_enter, nullptr};
  // link_off's check alone (no output is written before the last pass), an iteration's pass, the last pass
  const QArgs check = queue_pass(a, a.enter, a.packet, QOuts{});
  const QArgs iter = queue_pass(a, s_enter, s_packet, sorted_outs(ctx, a, false, drop));
  const QArgs last = queue_pass(a, s_enter, s_packet, sorted_outs(ctx, a, true, drop));
  u64* run = drop ? iter.out.done : nullptr;  // (sg_queue.h: carried_run)

  launch_links(ctx, check);
  const CIndex x = carry_index(ctx, a, perm, true);
  const CArgs& c = x.c;
  queue_check_flags(ctx, a.flag, where, true, true);

  uint32_t iters = 0;
  bool settled = false;
  while (!settled && iters < (uint32_t)cap) {
    iters++;
    SG_HIP(hipMemsetAsync(a.flag + Q_CHANGED, 0xff, 8, st));
    SG_HIP(hipMemsetAsync(x.n_work, 0, 4, st));
    {
      TimedLaunch tl(ctx, "link_queue_sort", (double)n);
      hipLaunchKernelGGL(k_carry_keys, g_rec, blk, 0, st, c);
      SG_CHECK_LAUNCH();
      segsort_enqueue(ctx, a.off, nl, (const uint4*)c.key, nullptr, x.key2, nullptr, sorted, x.piece, x.work, x.work_cap, x.n_work);
    }
    const u64* wt = launch_walk(ctx, iter, drop, run);  // (the walk's waits under the drop rule, else null)
    {
      TimedLaunch tl(ctx, "link_queue_carry", (double)n);
      hipLaunchKernelGGL(k_carry_propagate, g_rec, blk, 0, st, c, (const u64*)iter.out.done, wt);
      SG_CHECK_LAUNCH();
    }
    // read_timer("link_queue_iters") = (0, the last carried call's iterations, its records), timers on or off
    timer_set_counter(ctx, "link_queue_iters", (double)n, iters, true);
    settled = queue_check_flags(ctx, a.flag, where, true, false);
  }
  if (!settled)
    throw Error(SG_ERR_CAPACITY,
                "the carried times still moved after " + std::to_string(iters) + " iterations (SG_LINK_QUEUE_CARRY_ITERS)",
                iters, 0xFFFFFFFFu);

  // (under the drop rule no time moved: the last iteration's walk is this order's, wt, run and the marks stand)
  queue_output_pass(ctx, last, drop, run, drop);
  if (a.out.wait || a.out.done || a.out.ahead) {
    hipLaunchKernelGGL(k_carry_scatter, g_rec, blk, 0, st, c, last.out, a.out);
    SG_CHECK_LAUNCH();
  }
  if (packets) {
    // (the outputs stand at the input indices; only an arrival past the range is left to find)
    queue_packets(ctx, a, drop, c.next);
    queue_check_flags(ctx, a.flag, where, true, false);
  }
}

}  // namespace sg
