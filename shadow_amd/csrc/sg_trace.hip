// sg_trace.hip -- link trace: a round's packets per link, in time order.
//
// sg_tree_paths_packets (sg_paths.hip) keeps a round's hop records grouped by packet; this file
// gives the same crossings grouped by LINK and sorted by time.  A TRACE RECORD is one (counted
// packet p, link crossed).  Packet p has row i, source s = nodes[i], destination d and the tree
// path s = v0 .. vh = d of row i's pred row; cum(v) = latency_ns[i][pos[v]], cum(s) = 0.  d != s:
// hop k (1 <= k <= h) gives a record on link (v(k-1), vk) with (packet p, hop k, enter =
// send_time[p] + cum(v(k-1)), exit = send_time[p] + cum(vk)).  d == s: one record on the self-loop
// link (s, s), hop 1, enter = send_time[p], exit = send_time[p] + the diagonal cell.  Link L (in
// sg_net_links order) owns records [out_link_off[L], out_link_off[L + 1]) in ascending (enter,
// packet) order; a tree path crosses a link at most once, so the key is unique and the output a
// function of the inputs alone.  A link with watch[L] == 0 owns nothing; its crossings are
// walked and validated all the same.
//
// Steps on the context stream:
//   1. count (k_trace_count): a lane per packet, grid-stride; the count walk of sg_walks.h with
//      the link search (link_find, sg_links.h) per hop and a u32 add into the link's counter.
//      Writes the packet's hop count and every flag word: the walk is validated here once, whole.
//   2. scan (scan_counts, sg_scan.hip): the exclusive u64 scan of the link counters into
//      out_link_off, with out_link_off[n_links] and the total into a pinned, mapped word.
//   3. fill (k_trace_fill): the walk again; a record reserves its slot with an add on the link's
//      cursor and stores its staging record there: the key (enter, packet) with the hop in one
//      16-byte word, the exit time beside it when out_exit_ns is wanted.  The order inside a
//      segment is whatever the adds gave.
//   4. sort, per link, in three tiers after sg_wire.hip's segmented sort (sg_segsort.h):
//        k_trace_sort_small  a wave per link: up to 64 records are ranked in the wave's registers
//                            (keys are unique, so ranks are a permutation); a longer segment is
//                            cut into pieces of P records, work entry = (link, piece);
//        k_trace_sort_lds    a workgroup per piece: bitonic sort of its keys in LDS (16 bytes a
//                            key, 32 KiB at P = 2048); a segment of one piece is written out, a
//                            piece of a longer one goes sorted to the second staging array;
//        k_trace_merge       the pieces of a longer segment are merged by rank: a record's place
//                            is its index in its piece plus, for every other piece, the number of
//                            keys below its own (a binary search).
// The host reads the flag words and the total between 2 and 3 (total > cap: SG_ERR_CAPACITY, with
// out_link_off and *total complete and no record written) and waits for the stream after 4: two
// synchronisations.  Steps 1-2 and 3-4 are the halves of sg_walks.h (trace_enqueue_count /
// trace_finish_count / trace_enqueue_sort): sg_link_trace_packets runs them back to back, a
// device group (sg_group_trace.hip) runs them per member and merges the members' sorted segments.
#include <algorithm>
#include <string>
#include <vector>

#include "sg_device.h"
#include "sg_hosts.h"
#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_links.h"
#include "sg_segsort.h"
#include "sg_walks.h"

namespace sg {
namespace {

// (the item rule, the flag words and the walks: sg_walks.h; TR_THREADS, the sort's tiers and
// their limits: sg_segsort.h)

// (TraceArgs, TraceOut: sg_walks.h)

__device__ __forceinline__ bool watched(const TraceArgs& a, uint32_t link) { return !a.watch || a.watch[link] != 0; }

// ---- 1. count
__global__ void __launch_bounds__(TR_THREADS) k_trace_count(const TraceArgs a) {
  const LinkArgs& l = a.l;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < a.n_items; q += stride) {
    const uint32_t p = (uint32_t)q;
    uint32_t i, j, kind;
    const bool walk = packet_item(a.pk, l, p, i, j, kind);
    if (kind != LINK_NONE) flag_item(l, p, kind);
    uint32_t hops = 0;
    if (walk) {
      // the destination's time bounds every hop's: arc latency is at least 1 ns, cum rises along the path
      if (a.send_time[p] + a.lat[(size_t)(i - l.row_begin) * l.n + j] < a.send_time[p]) flag_item(l, p, ITEM_TIME);
      hops = count_walk<true>(l, i, j, [&](uint32_t link, uint32_t) {
        if (watched(a, link)) atomicAdd(&a.cnt[link], 1u);
      });
    }
    a.hops[p] = hops;
  }
}

// ---- 2. scan: scan_counts (sg_scan.hip)
// ---- 3. fill
__global__ void __launch_bounds__(TR_THREADS) k_trace_fill(const TraceArgs a) {
  const LinkArgs& l = a.l;
  const uint32_t n = l.n;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < a.n_items; q += stride) {
    const uint32_t p = (uint32_t)q;
    uint32_t k = a.hops[p];  // the hop number of the record at hand: the walk climbs from d
    uint32_t i, j, kind;
    if (k == 0 || !packet_item(a.pk, l, p, i, j, kind)) continue;
    const uint32_t s = l.nodes[i];
    const size_t r = (size_t)(i - l.row_begin) * n;
    const uint32_t* __restrict__ row = l.pred + r;
    const unsigned long long send = a.send_time[p];
    // v climbs from d; cv its column; pv = pred_i[v] (s itself for the self-loop's record),
    // gathered one hop ahead of the link search, and the cell of the hop's tail with it
    uint32_t v = l.nodes[j], cv = j;
    uint32_t pv = v == s ? s : row[j];
    unsigned long long exit = send + a.lat[r + cv];
    while (k > 0) {  // (the count's own bound)
      const uint32_t u = pv;
      if (u >= n) break;  // (the count walk reported it)
      uint32_t cu = 0u;
      unsigned long long enter = send;
      if (u != s) {
        cu = l.pos[u];
        pv = row[cu];
        enter = send + a.lat[r + cu];
      }
      const uint32_t link = link_find(l, u, v);
      if (link != LINK_NONE && watched(a, link)) {
        // (a slot past the segment cannot be reserved while the inputs are what the count walked;
        // the bound keeps the store inside the arrays whatever they are)
        const unsigned long long at = a.off[link] + atomicAdd(&a.cur[link], 1u);
        if (at < a.off[link + 1]) {
          a.key[at] = make_uint4((uint32_t)enter, (uint32_t)(enter >> 32), p, k);
          if (a.exit) a.exit[at] = exit;
        }
      }
      if (u == s) break;
      k--;
      v = u;
      cv = cu;
      exit = enter;
    }
  }
}

// ---- 4. sort: segsort_enqueue (sg_segsort.h)

}  // namespace

// ---- host: the halves of sg_walks.h, and the single-context call that runs them back to back
void trace_check(const TraceCall& c, bool check_nodes) {
  sg_ctx* ctx = c.ctx;
  sg_net* net = c.net;
  check_rows_call(ctx, net, c.nodes, c.n_nodes, c.row_begin, c.row_end);
  if (check_nodes) check_node_list(net, c.nodes, c.n_nodes);  // in range and none twice: with n_nodes entries, a permutation
  if (!c.hosts || c.hosts->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "host table belongs to another context");
  if (!c.packets) throw Error(SG_ERR_INVALID_ARG, "null packets");
  const uint32_t ni = c.packets->n_packets;
  if (ni && (!c.packets->src_host || !c.packets->dst_ipv4 || !c.packets->send_time_ns))
    throw Error(SG_ERR_INVALID_ARG, "null packet arrays");
  if (c.row_end > c.row_begin && (!c.pred || !c.lat)) throw Error(SG_ERR_INVALID_ARG, "null pred or latency_ns rows");
}

void trace_enqueue_count(const TraceCall& c, TraceJob& j) {
  sg_ctx* ctx = c.ctx;
  sg_net* net = c.net;
  hipStream_t st = ctx->stream;
  const uint32_t n = c.n_nodes, rows = c.row_end - c.row_begin, ni = c.packets->n_packets;
  ensure_links(ctx, net);
  const uint32_t nl = net->n_links;
  if (!ctx->paths_ret) SG_HIP(hipHostMalloc(&ctx->paths_ret, 16, hipHostMallocMapped | hipHostMallocCoherent));
  uint32_t* d_idx = link_node_index(ctx, c.nodes, n);
  unsigned long long* bad = ctx->l_flag.get<unsigned long long>(WALK_WORDS);
  SG_HIP(hipMemsetAsync(bad, 0xff, WALK_WORDS * 8, st));
  // the link counters, the fill's cursors and the work counter: one block, zeroed
  uint32_t* ctr = ctx->tr_cnt.get<uint32_t>(2 * (size_t)nl + 1);
  SG_HIP(hipMemsetAsync(ctr, 0, (2 * (size_t)nl + 1) * 4, st));
  TraceArgs& a = j.a;
  a.l = link_args(net, d_idx, n, c.row_begin, rows, c.pred, bad);
  a.pk = packet_args(c.hosts, c.packets, c.status);
  a.send_time = (const unsigned long long*)c.packets->send_time_ns;
  a.n_items = ni;
  a.hops = ctx->p_cnt.get<uint32_t>(ni);
  a.lat = (const unsigned long long*)c.lat;
  a.watch = c.watch;
  a.n_links = nl;
  a.cnt = ctr;
  a.cur = ctr + nl;
  a.off = (unsigned long long*)c.off;
  a.key = nullptr;
  a.exit = nullptr;
  j.n_work = ctr + 2 * (size_t)nl;
  j.grid = grid_for(ni, TR_THREADS, 16u * (unsigned)ctx->n_cu);
  j.total = 0;
  {
    // (work = the records, added once the total is read)
    TimedLaunch tl(ctx, "link_trace_count", 0.0);
    hipLaunchKernelGGL(k_trace_count, dim3(j.grid), dim3(TR_THREADS), 0, st, a);
    SG_CHECK_LAUNCH();
  }
  scan_counts(ctx, a.cnt, nl, a.off, ctx->paths_ret);
}

void trace_finish_count(const TraceCall& c, TraceJob& j) {
  sg_ctx* ctx = c.ctx;
  unsigned long long hw[WALK_WORDS];
  copy_to_host(ctx, hw, j.a.l.bad, sizeof(hw));
  const uint64_t tot = *ctx->paths_ret;
  timer_add_work(ctx, "link_trace_count", (double)tot);
  if (hw[WALK_BAD_ITEM] != ~0ull) throw_item_error(true, hw[WALK_BAD_ITEM]);
  if (hw[WALK_BAD_RANGE] != ~0ull || hw[WALK_BAD_CYCLE] != ~0ull) {
    const int kind = hw[WALK_BAD_RANGE] <= hw[WALK_BAD_CYCLE] ? WALK_BAD_RANGE : WALK_BAD_CYCLE;
    throw_pred_error(c.net, c.nodes, kind, hw[kind]);
  }
  if (hw[WALK_BAD_LINK] != ~0ull) throw_pred_error(c.net, c.nodes, WALK_BAD_LINK, hw[WALK_BAD_LINK]);
  j.total = tot;
}

void trace_enqueue_sort(const TraceCall& c, TraceJob& j, const TraceOut& out) {
  sg_ctx* ctx = c.ctx;
  hipStream_t st = ctx->stream;
  TraceArgs& a = j.a;
  const uint64_t tot = j.total;
  const uint32_t nl = a.n_links;
  const uint32_t piece = (uint32_t)knob_int("SG_LINK_TRACE_PIECE", (int)TR_PIECE_MAX, (int)TR_RANK_MAX, (int)TR_PIECE_MAX);
  const uint64_t work_cap64 = segsort_work_cap(tot, piece);  // pieces of the segments past TR_RANK_MAX, at most
  if (work_cap64 > 0xFFFFFFFFull) throw Error(SG_ERR_CAPACITY, "the trace holds more records than one call sorts");
  const uint32_t work_cap = (uint32_t)work_cap64;
  a.key = ctx->tr_key.get<uint4>(tot);
  uint4* key2 = ctx->tr_key2.get<uint4>(tot);
  unsigned long long* exit2 = nullptr;
  if (out.exit) {
    a.exit = ctx->tr_exit.get<unsigned long long>(tot);
    exit2 = ctx->tr_exit2.get<unsigned long long>(tot);
  }
  uint2* work = ctx->tr_work.get<uint2>(work_cap);
  {
    TimedLaunch tl(ctx, "link_trace_fill", (double)tot);
    hipLaunchKernelGGL(k_trace_fill, dim3(j.grid), dim3(TR_THREADS), 0, st, a);
    SG_CHECK_LAUNCH();
  }
  {
    TimedLaunch tl(ctx, "link_trace_sort", (double)tot);
    segsort_enqueue(ctx, a.off, nl, (const uint4*)a.key, (const unsigned long long*)a.exit, key2, exit2, out, piece, work,
                    work_cap, j.n_work);
  }
}

namespace {

// sg_link_trace_packets: host arrays staged around the halves; two synchronisations.
struct TraceRun {
  TraceCall c;  // (pred, lat, watch, off: the caller's, host or device by `flags`)
  uint32_t flags;
  uint32_t* out_packet;
  uint32_t* out_hop;
  uint64_t* out_enter;
  uint64_t* out_exit;
  uint64_t cap;
  uint64_t* total;
};

void trace_run(const TraceRun& r) {
  TraceCall c = r.c;
  sg_ctx* ctx = c.ctx;
  trace_check(c, true);
  if (!r.out_packet && !r.out_hop && !r.out_enter && !r.out_exit) throw Error(SG_ERR_INVALID_ARG, "no record output");
  if (!c.off || !r.total) throw Error(SG_ERR_INVALID_ARG, "null out_link_off or total");
  hipStream_t st = ctx->stream;
  const bool dev = (r.flags & SG_ROUTE_OUT_DEVICE) != 0;
  const uint32_t n = c.n_nodes, rows = c.row_end - c.row_begin, ni = c.packets->n_packets;
  ensure_links(ctx, c.net);
  const uint32_t nl = c.net->n_links;
  if (ni == 0) {
    if (dev) {
      SG_HIP(hipMemsetAsync(c.off, 0, ((size_t)nl + 1) * 8, st));
      SG_HIP(hipStreamSynchronize(st));
    } else {
      std::fill(c.off, c.off + nl + 1, (uint64_t)0);
    }
    *r.total = 0;
    return;
  }
  // host arrays in: device copies
  if (!dev) {
    const size_t cells = (size_t)rows * n;
    uint32_t* up = ctx->l_pred.get<uint32_t>(cells);
    uint64_t* ul = ctx->p_lat.get<uint64_t>(cells);
    if (cells) {
      SG_HIP(hipMemcpyAsync(up, r.c.pred, cells * 4, hipMemcpyHostToDevice, st));
      SG_HIP(hipMemcpyAsync(ul, r.c.lat, cells * 8, hipMemcpyHostToDevice, st));
    }
    c.pred = up;
    c.lat = ul;
    if (r.c.watch) {
      uint8_t* uw = ctx->tr_watch.get<uint8_t>(nl);
      if (nl) SG_HIP(hipMemcpyAsync(uw, r.c.watch, nl, hipMemcpyHostToDevice, st));
      c.watch = uw;
    }
    c.off = ctx->p_off.get<uint64_t>((size_t)nl + 1);
  }
  TraceJob j;
  trace_enqueue_count(c, j);
  if (!dev) SG_HIP(hipMemcpyAsync(r.c.off, c.off, ((size_t)nl + 1) * 8, hipMemcpyDeviceToHost, st));
  trace_finish_count(c, j);
  const uint64_t tot = j.total;
  *r.total = tot;
  if (tot > r.cap)
    throw Error(SG_ERR_CAPACITY,
                "the trace holds " + std::to_string(tot) + " records, the arrays " + std::to_string(r.cap));
  if (tot == 0) return;
  // the device copies of host outputs
  TraceOut out = {r.out_packet, r.out_hop, (unsigned long long*)r.out_enter, (unsigned long long*)r.out_exit};
  if (!dev) {
    if (r.out_packet) out.packet = ctx->p_node.get<uint32_t>(tot);
    if (r.out_hop) out.hop = ctx->p_link.get<uint32_t>(tot);
    if (r.out_enter) out.enter = ctx->p_olat.get<unsigned long long>(tot);
    if (r.out_exit) out.exit = ctx->tr_oexit.get<unsigned long long>(tot);
  }
  trace_enqueue_sort(c, j, out);
  if (!dev) {
    if (r.out_packet) SG_HIP(hipMemcpyAsync(r.out_packet, out.packet, tot * 4, hipMemcpyDeviceToHost, st));
    if (r.out_hop) SG_HIP(hipMemcpyAsync(r.out_hop, out.hop, tot * 4, hipMemcpyDeviceToHost, st));
    if (r.out_enter) SG_HIP(hipMemcpyAsync(r.out_enter, out.enter, tot * 8, hipMemcpyDeviceToHost, st));
    if (r.out_exit) SG_HIP(hipMemcpyAsync(r.out_exit, out.exit, tot * 8, hipMemcpyDeviceToHost, st));
  }
  SG_HIP(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace sg

extern "C" {

int32_t sg_link_trace_packets(sg_ctx* ctx, sg_net* net, sg_hosts* hosts, const uint32_t* nodes, uint32_t n_nodes,
                              uint32_t row_begin, uint32_t row_end, uint32_t flags, const uint32_t* pred,
                              const uint64_t* latency_ns, const sg_packets* packets, const uint8_t* status,
                              const uint8_t* watch, uint64_t* out_link_off, uint32_t* out_packet, uint32_t* out_hop,
                              uint64_t* out_enter_ns, uint64_t* out_exit_ns, uint64_t cap, uint64_t* total) {
  return sg::guarded(ctx, [&] {
    sg::trace_run(sg::TraceRun{sg::TraceCall{ctx, net, hosts, nodes, n_nodes, row_begin, row_end, pred, latency_ns,
                                             packets, status, watch, out_link_off},
                               flags, out_packet, out_hop, out_enter_ns, out_exit_ns, cap, total});
  });
}

}  // extern "C"
