// sg_group_trace.hip -- link loads and the link trace of a round across a device group.
//
// A group shards a round by source row block: member m holds rows [row_begin[m], row_end[m]) of
// the tree and the table, and packets[m] are the sends of its own sources.  The walks themselves
// are the single-context ones (sg_walks.h: the halves of sg_link_load_packets and
// sg_link_trace_packets); this file runs them on every member at once and combines the results on
// one member's device, `root`.  Everything is enqueued by the one calling thread.
//
// sg_group_link_load_packets
//   1. every member walks its batch on its own stream into a zeroed accumulator of its own
//      (context scratch: l_link, l_node); out_hops[m] is written in place;
//   2. the host reads every member's flag words (one wait per member, all walks in flight);
//   3. k_group_link_reduce on root's stream adds the n accumulators into the caller's arrays.
//      Because the add is deferred past 2, an error leaves the caller's arrays untouched.
//
// sg_group_link_series_packets: the same three steps with sg_link_series_packets' walk; the
// accumulators are a member's series matrix and outside cells (sr_series, sr_outside), the host
// slot map goes to every member (sr_slot), and k_group_flat_reduce adds on root.
//
// sg_group_link_trace_packets
//   1. every member counts and scans on its own stream: off_m (p_off) and total_m;
//   2. the host reads flags and totals;
//   3. k_group_off_sum on root: out_link_off[L] = the sum over m of off_m[L] -- a sum of prefix
//      sums is the prefix sum of the sums, so nothing is scanned again; the capacity check;
//   4. every member fills and sorts its own records (the three tiers of sg_trace.hip) into sorted
//      staging of its own (p_node, p_link, p_olat, tr_oexit), and records its "sent" event;
//   5. k_group_trace_merge on root, after every member's event: each record of member m on link L
//      goes to  out_link_off[L] + its index in m's segment + the records of the other members'
//      segments of L that come before it: those with enter <= its own for m' < m, enter < its own
//      for m' > m.  Each member's segment ascends in (enter, packet), so both counts are binary
//      searches on enter alone, and the result ascends in (enter, member, packet).
//   6. one wait on root's stream, which by then has waited for every member's.
//
// k_group_trace_merge: a thread per record, grid-stride, blockIdx.y = the member.  The thread
// finds its link by a binary search of its record index in off_m (log2 n_links steps), then makes
// n - 1 searches of log2(segment) steps.  Work goes with the records alone: a hot link's records
// spread over the whole grid, an empty link costs nothing, no launch per link.  Nothing is
// re-sorted.  Every loop has a fixed bound, no workgroup waits on another, plain vector loads and
// stores only.  The members' pointers travel by value in the argument block (sg_group.hip's
// PullArgs): indexed by the workgroup's member and a uniform loop counter, they are scalar loads
// from the argument segment; a member on another device is read through peer access, which
// sg_group_create enabled.  Bound by the latency of dependent loads (each search step waits for
// the one before), mostly served by L2: unmeasured on hardware beyond the timer's totals.
#include <algorithm>
#include <string>
#include <vector>

#include "sg_internal.h"
#include "sg_walks.h"

namespace sg {
namespace {

constexpr int GT_THREADS = 256;

struct ReduceArgs {
  const unsigned long long* link[GROUP_MAX];  // member m's accumulators, or null
  const unsigned long long* node[GROUP_MAX];
};

__global__ void __launch_bounds__(GT_THREADS) k_group_link_reduce(const ReduceArgs a, uint32_t n, uint32_t n_links,
                                                                 uint32_t n_nodes, unsigned long long* out_link,
                                                                 unsigned long long* out_node) {
  const uint32_t gtid = blockIdx.x * GT_THREADS + threadIdx.x, gsize = gridDim.x * GT_THREADS;
  if (out_link)
    for (uint32_t i = gtid; i < n_links; i += gsize) {
      unsigned long long s = 0ull;
      for (uint32_t m = 0; m < n; m++)
        if (a.link[m]) s += a.link[m][i];
      out_link[i] += s;
    }
  if (out_node)
    for (uint32_t i = gtid; i < n_nodes; i += gsize) {
      unsigned long long s = 0ull;
      for (uint32_t m = 0; m < n; m++)
        if (a.node[m]) s += a.node[m][i];
      out_node[i] += s;
    }
}

// The same sum over two flat arrays of any length (the series matrix and its outside cells).
__global__ void __launch_bounds__(GT_THREADS) k_group_flat_reduce(const ReduceArgs a, uint32_t n, size_t len_a,
                                                                 size_t len_b, unsigned long long* out_a,
                                                                 unsigned long long* out_b) {
  const size_t gtid = (size_t)blockIdx.x * GT_THREADS + threadIdx.x, gsize = (size_t)gridDim.x * GT_THREADS;
  for (size_t i = gtid; i < len_a; i += gsize) {
    unsigned long long s = 0ull;
    for (uint32_t m = 0; m < n; m++)
      if (a.link[m]) s += a.link[m][i];
    if (s) out_a[i] += s;
  }
  if (out_b)
    for (size_t i = gtid; i < len_b; i += gsize) {
      unsigned long long s = 0ull;
      for (uint32_t m = 0; m < n; m++)
        if (a.node[m]) s += a.node[m][i];
      if (s) out_b[i] += s;
    }
}

struct MergeArgs {
  const unsigned long long* off[GROUP_MAX];    // member m's offsets (n_links + 1), or null: no packets
  const unsigned long long* enter[GROUP_MAX];  // its sorted staging (null with no record)
  const unsigned long long* exit[GROUP_MAX];
  const uint32_t* packet[GROUP_MAX];
  const uint32_t* hop[GROUP_MAX];
  unsigned long long total[GROUP_MAX];
  uint32_t base[GROUP_MAX];
};

struct GroupTraceOut {
  uint32_t* packet;
  uint8_t* member;
  uint32_t* hop;
  unsigned long long* enter;
  unsigned long long* exit;
};

// out[i] = the sum of the members' off[i], i < n_entries.
__global__ void __launch_bounds__(GT_THREADS) k_group_off_sum(const MergeArgs a, uint32_t n, uint32_t n_entries,
                                                             unsigned long long* out) {
  const uint32_t gtid = blockIdx.x * GT_THREADS + threadIdx.x, gsize = gridDim.x * GT_THREADS;
  for (uint32_t i = gtid; i < n_entries; i += gsize) {
    unsigned long long s = 0ull;
    for (uint32_t m = 0; m < n; m++)
      if (a.off[m]) s += a.off[m][i];
    out[i] = s;
  }
}

__global__ void __launch_bounds__(GT_THREADS) k_group_trace_merge(const MergeArgs a, uint32_t n, uint32_t n_links,
                                                                 GroupTraceOut o, unsigned long long cap) {
  const uint32_t m = blockIdx.y;
  const unsigned long long tot = a.total[m];
  if (tot == 0) return;
  const unsigned long long* __restrict__ off = a.off[m];
  const unsigned long long stride = (unsigned long long)gridDim.x * GT_THREADS;
  for (unsigned long long r = (unsigned long long)blockIdx.x * GT_THREADS + threadIdx.x; r < tot; r += stride) {
    // the record's link: off[lo] <= r < off[hi] throughout (off[0] = 0, off[n_links] = tot)
    uint32_t lo = 0, hi = n_links;
    for (int it = 0; it < 32 && hi - lo > 1; it++) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (off[mid] <= r)
        lo = mid;
      else
        hi = mid;
    }
    const uint32_t link = lo;
    const unsigned long long t = a.enter[m][r];
    unsigned long long pos = r - off[link];
    for (uint32_t q = 0; q < n; q++) {
      const unsigned long long* __restrict__ qo = a.off[q];
      if (!qo) continue;
      const unsigned long long s0 = qo[link];
      pos += s0;  // (over every member: out_link_off[link])
      if (q == m) continue;
      // q's records on the link that come first: enter <= t for q < m, enter < t for q > m
      const unsigned long long* __restrict__ e = a.enter[q];
      unsigned long long l2 = s0, h2 = qo[link + 1];
      for (int it = 0; it < 64 && l2 < h2; it++) {
        const unsigned long long mid = l2 + ((h2 - l2) >> 1);
        const unsigned long long x = e[mid];
        if (q < m ? x <= t : x < t)
          l2 = mid + 1;
        else
          h2 = mid;
      }
      pos += l2 - s0;
    }
    if (pos >= cap) continue;  // (never, while the staging is what the members counted)
    if (o.packet) o.packet[pos] = a.base[m] + a.packet[m][r];
    if (o.member) o.member[pos] = (uint8_t)m;
    if (o.hop) o.hop[pos] = a.hop[m][r];
    if (o.enter) o.enter[pos] = t;
    if (o.exit) o.exit[pos] = a.exit[m][r];
  }
}

// ---- host
// What both calls take per member, checked: the nets (one graph, each on its member), the hosts,
// the row ranges.  Returns the members' count.
uint32_t group_check_members(sg_group* g, sg_net** nets, sg_hosts** hosts, const uint32_t* nodes, uint32_t n_nodes,
                             const uint32_t* row_begin, const uint32_t* row_end, const void* const* pred,
                             const sg_packets* packets, uint32_t root) {
  const uint32_t n = (uint32_t)g->ctxs.size();
  if (!nets || !hosts || !row_begin || !row_end || !pred || !packets) throw Error(SG_ERR_INVALID_ARG, "null argument");
  if (n_nodes && !nodes) throw Error(SG_ERR_INVALID_ARG, "null node list");
  if (root >= n) throw Error(SG_ERR_INVALID_ARG, "root is not a member");
  for (uint32_t m = 0; m < n; m++) {
    if (!nets[m] || nets[m]->ctx != g->ctxs[m])
      throw Error(SG_ERR_INVALID_ARG,
                  "nets[" + std::to_string(m) + "] was not created on member " + std::to_string(m) + "'s context");
    if (nets[m]->n_nodes != nets[0]->n_nodes || nets[m]->n_edges != nets[0]->n_edges ||
        nets[m]->directed != nets[0]->directed)
      throw Error(SG_ERR_INVALID_ARG, "nets[" + std::to_string(m) + "] is not the graph of nets[0]");
  }
  return n;
}

// A member's argument error, naming the member.
template <class F>
void member_check(uint32_t m, F&& fn) {
  try {
    fn();
  } catch (const Error& e) {
    throw Error(e.code, "member " + std::to_string(m) + ": " + e.what(), e.row, e.col);
  }
}

// Every member's links (built on first use), and that they number the same.
uint32_t group_links(sg_group* g, sg_net** nets) {
  const uint32_t n = (uint32_t)g->ctxs.size();
  for (uint32_t m = 0; m < n; m++) {
    set_device(g->ctxs[m]);
    ensure_links(g->ctxs[m], nets[m]);
    if (nets[m]->n_links != nets[0]->n_links)
      throw Error(SG_ERR_INVALID_ARG, "nets[" + std::to_string(m) + "] is not the graph of nets[0]");
  }
  return nets[0]->n_links;
}

// Waits for every member's stream and rethrows: an exit by exception leaves nothing in flight.
template <class F>
void drained_on_error(sg_group* g, F&& fn) {
  try {
    fn();
  } catch (...) {
    for (sg_ctx* c : g->ctxs)
      if (hipSetDevice(c->device) == hipSuccess) (void)hipStreamSynchronize(c->stream);
    throw;
  }
}

// The finish half of every active member (each waits for its own stream); the lowest-numbered
// failing member's error is the group's.
template <class F>
void finish_members(sg_group* g, const std::vector<uint8_t>& active, F&& finish) {
  const uint32_t n = (uint32_t)g->ctxs.size();
  std::vector<int32_t> rc(n, SG_OK);
  for (uint32_t m = 0; m < n; m++)
    if (active[m]) rc[m] = guarded(g->ctxs[m], [&] { finish(m); });
  for (uint32_t m = 0; m < n; m++) {
    if (rc[m] == SG_OK) continue;
    const sg_ctx* c = g->ctxs[m];
    g->err_member = m;
    throw Error(rc[m], "member " + std::to_string(m) + ": " + c->last_error, c->err_row, c->err_col);
  }
}

// "sent" on every active member's stream but root's own; root's stream waits for them all
// (exchange_ordered's steps 1 and 2, for one owner).
void root_waits(sg_group* g, uint32_t root, const std::vector<uint8_t>& active) {
  const uint32_t n = (uint32_t)g->ctxs.size();
  for (uint32_t m = 0; m < n; m++) {
    if (!active[m] || m == root) continue;
    set_device(g->ctxs[m]);
    SG_HIP(hipEventRecord(g->sent[m], g->ctxs[m]->stream));
  }
  set_device(g->ctxs[root]);
  for (uint32_t m = 0; m < n; m++)
    if (active[m] && m != root) SG_HIP(hipStreamWaitEvent(g->ctxs[root]->stream, g->sent[m], 0));
}

}  // namespace
}  // namespace sg

extern "C" {

int32_t sg_group_link_load_packets(sg_group* g, sg_net** nets, sg_hosts** hosts, const uint32_t* nodes,
                                   uint32_t n_nodes, const uint32_t* row_begin, const uint32_t* row_end,
                                   const uint32_t** pred, const sg_packets* packets, const uint8_t** status,
                                   const uint32_t** weight, uint32_t root, uint64_t* out_link_load,
                                   uint64_t* out_node_load, uint32_t** out_hops) {
  return sg::group_guarded(g, [&] {
    using namespace sg;
    const uint32_t n = group_check_members(g, nets, hosts, nodes, n_nodes, row_begin, row_end,
                                           (const void* const*)pred, packets, root);
    bool any_hops = false;
    for (uint32_t m = 0; out_hops && m < n; m++) any_hops |= out_hops[m] != nullptr;
    if (!out_link_load && !out_node_load && !any_hops) throw Error(SG_ERR_INVALID_ARG, "null output");
    std::vector<LinkPacketsCall> c(n);
    std::vector<uint8_t> active(n, 0);
    for (uint32_t m = 0; m < n; m++) {
      c[m] = LinkPacketsCall{g->ctxs[m], nets[m],    hosts[m],
                             nodes,      n_nodes,    row_begin[m],
                             row_end[m], pred[m],    &packets[m],
                             status ? status[m] : nullptr, weight ? weight[m] : nullptr,
                             nullptr,    nullptr,    out_hops ? out_hops[m] : nullptr};
      member_check(m, [&] { link_packets_check(c[m], false); });
      active[m] = packets[m].n_packets != 0;
    }
    check_node_list(nets[0], nodes, n_nodes);  // in range and none twice: with n_nodes entries, a permutation
    if (std::find(active.begin(), active.end(), 1) == active.end()) return;
    const uint32_t nl = group_links(g, nets);
    ReduceArgs ra{};
    drained_on_error(g, [&] {
      for (uint32_t m = 0; m < n; m++) {
        if (!active[m]) continue;
        sg_ctx* ctx = g->ctxs[m];
        set_device(ctx);
        if (out_link_load) {
          c[m].link_load = ctx->l_link.get<uint64_t>(nl);
          SG_HIP(hipMemsetAsync(c[m].link_load, 0, std::max<size_t>((size_t)nl * 8, 8), ctx->stream));
        }
        if (out_node_load) {
          c[m].node_load = ctx->l_node.get<uint64_t>(n_nodes);
          SG_HIP(hipMemsetAsync(c[m].node_load, 0, std::max<size_t>((size_t)n_nodes * 8, 8), ctx->stream));
        }
        ra.link[m] = (const unsigned long long*)c[m].link_load;
        ra.node[m] = (const unsigned long long*)c[m].node_load;
        link_packets_enqueue(c[m]);
      }
      finish_members(g, active, [&](uint32_t m) { link_packets_finish(c[m]); });
      if (!out_link_load && !out_node_load) return;
      root_waits(g, root, active);
      sg_ctx* rc = g->ctxs[root];
      {
        // work = the accumulator words read
        TimedLaunch tl(rc, "group_link_reduce",
                       (double)std::count(active.begin(), active.end(), 1) *
                           ((out_link_load ? (double)nl : 0.0) + (out_node_load ? (double)n_nodes : 0.0)));
        const unsigned grid = grid_for(std::max<size_t>(nl, n_nodes), GT_THREADS, 4u * (unsigned)rc->n_cu);
        hipLaunchKernelGGL(k_group_link_reduce, dim3(grid), dim3(GT_THREADS), 0, rc->stream, ra, n, nl, n_nodes,
                           (unsigned long long*)out_link_load, (unsigned long long*)out_node_load);
        SG_CHECK_LAUNCH();
      }
      SG_HIP(hipStreamSynchronize(rc->stream));
    });
  });
}

int32_t sg_group_link_series_packets(sg_group* g, sg_net** nets, sg_hosts** hosts, const uint32_t* nodes,
                                     uint32_t n_nodes, const uint32_t* row_begin, const uint32_t* row_end,
                                     const uint32_t** pred, const uint64_t** latency_ns, const sg_packets* packets,
                                     const uint8_t** status, const uint32_t** weight, const uint32_t* link_slot,
                                     uint32_t n_slots, uint32_t at, uint64_t t0_ns, uint64_t bin_ns, uint32_t n_bins,
                                     uint32_t root, uint64_t* out_series, uint64_t* out_outside) {
  return sg::group_guarded(g, [&] {
    using namespace sg;
    const uint32_t n = group_check_members(g, nets, hosts, nodes, n_nodes, row_begin, row_end,
                                           (const void* const*)pred, packets, root);
    if (!latency_ns) throw Error(SG_ERR_INVALID_ARG, "null argument");
    std::vector<SeriesCall> c(n);
    std::vector<uint8_t> active(n, 0);
    for (uint32_t m = 0; m < n; m++) {
      // (slot and series: the caller's, for the check alone, which reads neither; the member's
      // own copy and accumulator below)
      c[m] = SeriesCall{g->ctxs[m], nets[m],    hosts[m],   nodes,
                        n_nodes,    row_begin[m], row_end[m], pred[m],
                        latency_ns[m], &packets[m], status ? status[m] : nullptr, weight ? weight[m] : nullptr,
                        link_slot,  n_slots,    at,         t0_ns,
                        bin_ns,     n_bins,     out_series, nullptr};
      member_check(m, [&] {
        set_device(g->ctxs[m]);  // (the check builds the member's links)
        series_check(c[m], false);
      });
      c[m].slot = nullptr;
      active[m] = packets[m].n_packets != 0;
    }
    check_node_list(nets[0], nodes, n_nodes);  // in range and none twice: with n_nodes entries, a permutation
    const uint32_t nl = group_links(g, nets);
    if (link_slot)
      for (uint32_t k = 0; k < nl; k++)
        if (link_slot[k] >= n_slots && link_slot[k] != 0xFFFFFFFFu)
          throw Error(SG_ERR_INVALID_ARG,
                      "link_slot[" + std::to_string(k) + "] is neither below n_slots nor UINT32_MAX", k, 0xFFFFFFFFu);
    if (std::find(active.begin(), active.end(), 1) == active.end()) return;
    const size_t n_series = (size_t)n_slots * n_bins, n_out = out_outside ? 2 * (size_t)n_slots : 0;
    ReduceArgs ra{};
    drained_on_error(g, [&] {
      for (uint32_t m = 0; m < n; m++) {
        if (!active[m]) continue;
        sg_ctx* ctx = g->ctxs[m];
        set_device(ctx);
        if (link_slot) {
          uint32_t* us = ctx->sr_slot.get<uint32_t>(nl);
          if (nl) SG_HIP(hipMemcpyAsync(us, link_slot, (size_t)nl * 4, hipMemcpyHostToDevice, ctx->stream));
          c[m].slot = us;
        }
        c[m].series = ctx->sr_series.get<uint64_t>(n_series);
        SG_HIP(hipMemsetAsync(c[m].series, 0, n_series * 8, ctx->stream));
        if (out_outside) {
          c[m].outside = ctx->sr_outside.get<uint64_t>(n_out);
          SG_HIP(hipMemsetAsync(c[m].outside, 0, n_out * 8, ctx->stream));
        }
        ra.link[m] = (const unsigned long long*)c[m].series;
        ra.node[m] = (const unsigned long long*)c[m].outside;
        series_enqueue(c[m]);
      }
      finish_members(g, active, [&](uint32_t m) { series_finish(c[m]); });
      root_waits(g, root, active);
      sg_ctx* rc = g->ctxs[root];
      {
        // work = the accumulator words read
        TimedLaunch tl(rc, "group_link_reduce",
                       (double)std::count(active.begin(), active.end(), 1) * ((double)n_series + (double)n_out));
        const unsigned grid = grid_for(std::max(n_series, n_out), GT_THREADS, 4u * (unsigned)rc->n_cu);
        hipLaunchKernelGGL(k_group_flat_reduce, dim3(grid), dim3(GT_THREADS), 0, rc->stream, ra, n, n_series, n_out,
                           (unsigned long long*)out_series, (unsigned long long*)out_outside);
        SG_CHECK_LAUNCH();
      }
      SG_HIP(hipStreamSynchronize(rc->stream));
    });
  });
}

int32_t sg_group_link_trace_packets(sg_group* g, sg_net** nets, sg_hosts** hosts, const uint32_t* nodes,
                                    uint32_t n_nodes, const uint32_t* row_begin, const uint32_t* row_end,
                                    const uint32_t** pred, const uint64_t** latency_ns, const sg_packets* packets,
                                    const uint8_t** status, const uint8_t* watch, const uint32_t* packet_base,
                                    uint32_t root, uint64_t* out_link_off, uint32_t* out_packet, uint8_t* out_member,
                                    uint32_t* out_hop, uint64_t* out_enter_ns, uint64_t* out_exit_ns, uint64_t cap,
                                    uint64_t* total) {
  return sg::group_guarded(g, [&] {
    using namespace sg;
    const uint32_t n = group_check_members(g, nets, hosts, nodes, n_nodes, row_begin, row_end,
                                           (const void* const*)pred, packets, root);
    if (!latency_ns) throw Error(SG_ERR_INVALID_ARG, "null argument");
    if (!out_packet && !out_member && !out_hop && !out_enter_ns && !out_exit_ns)
      throw Error(SG_ERR_INVALID_ARG, "no record output");
    if (!out_link_off || !total) throw Error(SG_ERR_INVALID_ARG, "null out_link_off or total");
    std::vector<TraceCall> c(n);
    std::vector<TraceJob> job(n);
    std::vector<uint8_t> active(n, 0);
    MergeArgs ma{};
    uint64_t n_packets = 0;
    for (uint32_t m = 0; m < n; m++) {
      c[m] = TraceCall{g->ctxs[m], nets[m],       hosts[m],    nodes,
                       n_nodes,    row_begin[m],  row_end[m],  pred[m],
                       latency_ns[m], &packets[m], status ? status[m] : nullptr, nullptr, nullptr};
      member_check(m, [&] { trace_check(c[m], false); });
      active[m] = packets[m].n_packets != 0;
      ma.base[m] = packet_base ? packet_base[m] : (uint32_t)n_packets;
      n_packets += packets[m].n_packets;
    }
    if (!packet_base && n_packets > 0x100000000ull)
      throw Error(SG_ERR_INVALID_ARG, "more than 2^32 packets: the default packet_base does not number them");
    check_node_list(nets[0], nodes, n_nodes);  // in range and none twice: with n_nodes entries, a permutation
    const uint32_t nl = group_links(g, nets);
    sg_ctx* rc = g->ctxs[root];
    drained_on_error(g, [&] {
      // 1. count and scan, every member on its own stream
      for (uint32_t m = 0; m < n; m++) {
        if (!active[m]) continue;
        sg_ctx* ctx = g->ctxs[m];
        set_device(ctx);
        if (watch) {
          uint8_t* uw = ctx->tr_watch.get<uint8_t>(nl);
          if (nl) SG_HIP(hipMemcpyAsync(uw, watch, nl, hipMemcpyHostToDevice, ctx->stream));
          c[m].watch = uw;
        }
        c[m].off = ctx->p_off.get<uint64_t>((size_t)nl + 1);
        trace_enqueue_count(c[m], job[m]);
        ma.off[m] = (const unsigned long long*)c[m].off;
      }
      // 2. flags and totals
      finish_members(g, active, [&](uint32_t m) { trace_finish_count(c[m], job[m]); });
      uint64_t sum = 0, most = 0;
      for (uint32_t m = 0; m < n; m++) {
        ma.total[m] = active[m] ? job[m].total : 0;
        sum += ma.total[m];
        most = std::max<uint64_t>(most, ma.total[m]);
      }
      // 3. root's offsets (the members' streams are drained: no event is needed yet)
      set_device(rc);
      {
        TimedLaunch tl(rc, "group_trace_offsets", (double)sum);
        hipLaunchKernelGGL(k_group_off_sum, dim3(grid_for((size_t)nl + 1, GT_THREADS, 4u * (unsigned)rc->n_cu)),
                           dim3(GT_THREADS), 0, rc->stream, ma, n, nl + 1, (unsigned long long*)out_link_off);
        SG_CHECK_LAUNCH();
      }
      *total = sum;
      if (sum > cap || sum == 0) {
        SG_HIP(hipStreamSynchronize(rc->stream));
        if (sum > cap)
          throw Error(SG_ERR_CAPACITY,
                      "the trace holds " + std::to_string(sum) + " records, the arrays " + std::to_string(cap));
        return;
      }
      // 4. every member's fill and sort into its own sorted staging
      std::vector<uint8_t> sorting(n, 0);
      for (uint32_t m = 0; m < n; m++) {
        const uint64_t tot = ma.total[m];
        if (tot == 0) continue;
        sg_ctx* ctx = g->ctxs[m];
        set_device(ctx);
        TraceOut out = {out_packet ? ctx->p_node.get<uint32_t>(tot) : nullptr,
                        out_hop ? ctx->p_link.get<uint32_t>(tot) : nullptr,
                        ctx->p_olat.get<unsigned long long>(tot),  // (the merge's key: always)
                        out_exit_ns ? ctx->tr_oexit.get<unsigned long long>(tot) : nullptr};
        trace_enqueue_sort(c[m], job[m], out);
        ma.packet[m] = out.packet;
        ma.hop[m] = out.hop;
        ma.enter[m] = out.enter;
        ma.exit[m] = out.exit;
        sorting[m] = 1;
      }
      // 5. the merge on root, after every member's sort
      root_waits(g, root, sorting);
      {
        TimedLaunch tl(rc, "group_trace_merge", (double)sum);
        const dim3 grid(grid_for(most, GT_THREADS, 8u * (unsigned)rc->n_cu), n);
        hipLaunchKernelGGL(k_group_trace_merge, grid, dim3(GT_THREADS), 0, rc->stream, ma, n, nl,
                           GroupTraceOut{out_packet, out_member, out_hop, (unsigned long long*)out_enter_ns,
                                         (unsigned long long*)out_exit_ns},
                           (unsigned long long)sum);
        SG_CHECK_LAUNCH();
      }
      // 6. root's stream has waited for every member's
      SG_HIP(hipStreamSynchronize(rc->stream));
    });
  });
}

}  // extern "C"
