// sg_paths.hip -- batched tree paths: the hop list of every pair, or of every packet of a round.
//
// sg_link_load_packets (sg_link.hip) walks a packet's tree path and keeps sums; this file keeps
// the walk itself.  A HOP RECORD is one link crossed.  For source row i (s = nodes[i]) and
// destination column j (d = nodes[j]), d != s: the tree path s = v0, v1, ..., vh = d of row i's pred
// row gives h records in source-to-destination order, record k (1 <= k <= h) = (node vk, the link
// (v(k-1), vk) in sg_net_links order, latency[i][pos[vk]], packet_loss[i][pos[vk]]): the
// cumulative (latency, loss) at a hop is the row's own table cell of the intermediate node, bit
// for bit ("the fold along the tree path to v is key[v]").  d == s: one record, the
// self-loop link (s, s) with the diagonal cell, as sg_link_load_packets counts that case.  A
// packet that does not count has no record.
//
// The output is CSR and deterministic: out_off (n + 1 u64, out_off[0] = 0), pair or packet p owns
// records [out_off[p], out_off[p + 1]).  Three steps on the context stream:
//   1. count (k_paths_count): a lane per pair or packet, grid-stride; the count walk of
//      sg_walks.h without the link search: per hop pos[u] and pred_row[.], two dependent loads.
//      Writes the hop count, 0 for a packet that does not count.
//   2. scan (scan_counts, sg_scan.hip): the exclusive u64 scan of the counts into out_off, with
//      out_off[n] and the total into a pinned, mapped word.
//   3. fill (k_paths_fill): the walk again, records written backwards from out_off[p + 1], so the
//      order comes out source to destination; the next hop's gather is issued ahead of this hop's
//      link search (link_find, sg_links.h), which is skipped when out_link is NULL.
//      Direct form: every lane stores into its own region.  Staged form (SG_PATHS_STAGE=1): a
//      wave's 64 consecutive pairs own one contiguous span of the output; where the span is at
//      most SG_PATHS_STAGE_HOPS records the lanes put their records into the wave's part of the
//      LDS and the wave writes the span out with consecutive lanes on consecutive records; a
//      longer span (a path graph) takes the direct stores, per wave.
// The host reads the flag words and the total between 2 and 3 (total > cap: SG_ERR_CAPACITY, with
// out_off and *total complete and no record written) and the flag words again after 3 (a
// (pred, node) pair that is not a link is found there): two synchronisations.
#include <algorithm>
#include <string>
#include <vector>

#include "sg_device.h"
#include "sg_hosts.h"
#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_links.h"
#include "sg_walks.h"

namespace sg {

// (the item rule, the flag words and the walks: sg_walks.h)
constexpr uint32_t PA_THREADS = 256;
constexpr int PA_STAGE_HOPS = 640;      // records a wave stages (the default: 10 hops a lane)
constexpr int PA_STAGE_HOPS_MAX = 1536;  // 4 waves x 20 bytes x 1536 = 120 KiB of the CU's 160

struct PathArgs {
  LinkArgs l;  // (bad: WALK_WORDS words)
  // the packet form: the hosts' address map and the batch
  PacketArgs pk;
  // the pair form
  const uint32_t* pair_row;
  const uint32_t* pair_col;
  uint32_t n_items;  // pairs or packets
  uint32_t* cnt;     // hops per item
  unsigned long long* off;  // out_off
  // rows [row_begin, row_begin + rows) of the table, or null
  const unsigned long long* lat;
  const float* loss;
  uint32_t* out_node;
  uint32_t* out_link;
  unsigned long long* out_lat;
  float* out_loss;
  uint32_t stage_hops;
};

template <bool PACKETS>
__device__ __forceinline__ bool path_item(const PathArgs& a, uint32_t p, uint32_t& i, uint32_t& j, uint32_t& kind) {
  return PACKETS ? packet_item(a.pk, a.l, p, i, j, kind) : pair_item(a.pair_row, a.pair_col, a.l, p, i, j, kind);
}

// ---- 1. count
template <bool PACKETS>
__global__ void __launch_bounds__(PA_THREADS) k_paths_count(const PathArgs a) {
  const LinkArgs& l = a.l;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < a.n_items; q += stride) {
    const uint32_t p = (uint32_t)q;
    uint32_t i, j, kind;
    const bool walk = path_item<PACKETS>(a, p, i, j, kind);
    if (kind != LINK_NONE) flag_item(l, p, kind);
    a.cnt[p] = walk ? count_walk<false>(l, i, j, [] {}) : 0u;
  }
}

// ---- 2. scan: scan_counts (sg_scan.hip)
// ---- 3. fill
// The staged records of one wave: its part of the dynamic LDS, an array per requested output
// (latency first: 8-byte aligned).
struct PathStage {
  unsigned long long* lat;
  uint32_t* node;
  uint32_t* link;
  float* loss;
};

__host__ __device__ inline size_t path_stage_bytes(uint32_t hops, bool node, bool link, bool lat, bool loss) {
  const size_t b = (size_t)hops * ((lat ? 8u : 0u) + (node ? 4u : 0u) + (link ? 4u : 0u) + (loss ? 4u : 0u));
  return (b + 7) & ~(size_t)7;
}

template <bool PACKETS, bool STAGE>
__global__ void __launch_bounds__(PA_THREADS) k_paths_fill(const PathArgs a) {
  extern __shared__ __align__(16) unsigned char paths_smem[];
  const LinkArgs& l = a.l;
  const uint32_t n = l.n, lane = threadIdx.x & 63u;
  PathStage st = {nullptr, nullptr, nullptr, nullptr};
  if (STAGE) {
    const uint32_t H = a.stage_hops;
    unsigned char* at = paths_smem + (threadIdx.x >> 6) * path_stage_bytes(H, a.out_node, a.out_link, a.out_lat, a.out_loss);
    st.lat = (unsigned long long*)at;
    at += a.out_lat ? (size_t)H * 8 : 0;
    st.node = (uint32_t*)at;
    at += a.out_node ? (size_t)H * 4 : 0;
    st.link = (uint32_t*)at;
    at += a.out_link ? (size_t)H * 4 : 0;
    st.loss = (float*)at;
  }
  // (the trip count is the same for every thread of a workgroup: the staged form has a barrier)
  for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < a.n_items;
       base += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long q = base + threadIdx.x;
    // the wave's span of the output
    unsigned long long span_b = 0ull;
    bool staged = false;
    uint32_t span = 0;
    if (STAGE) {
      const unsigned long long ni = a.n_items;
      const unsigned long long w0 = q - lane < ni ? q - lane : ni;
      const unsigned long long w1 = w0 + 64 < ni ? w0 + 64 : ni;
      span_b = a.off[w0];
      const unsigned long long len = a.off[w1] - span_b;
      staged = len <= a.stage_hops;
      span = staged ? (uint32_t)len : 0u;
    }
    if (q < a.n_items) {
      const uint32_t p = (uint32_t)q;
      const unsigned long long begin = a.off[p];
      unsigned long long k = a.off[p + 1];
      uint32_t i, j, kind;
      if (k > begin && path_item<PACKETS>(a, p, i, j, kind)) {
        const uint32_t s = l.nodes[i];
        const size_t r = (size_t)(i - l.row_begin) * n;
        const uint32_t* __restrict__ row = l.pred + r;
        const unsigned long long cell = (unsigned long long)i << 32;
        // v climbs from d; cv its column; pv = pred_i[v] (s itself for the self-loop's record),
        // gathered one hop ahead
        uint32_t v = l.nodes[j], cv = j;
        uint32_t pv = v == s ? s : row[j];
        while (k > begin) {  // (the count's own bound: a lane never leaves its region)
          k--;
          const uint32_t u = pv;
          if (u >= n) break;  // (the count walk reported it)
          // the next hop's gather ahead of this hop's search: the search's dependent loads overlap it
          uint32_t cu = 0u;
          if (u != s) {
            cu = l.pos[u];
            pv = row[cu];
          }
          uint32_t link = LINK_NONE;
          if (a.out_link) {
            link = link_find(l, u, v);
            if (link == LINK_NONE) atomicMin(&l.bad[WALK_BAD_LINK], cell | cv);
          }
          if (STAGE && staged) {
            const uint32_t t = (uint32_t)(k - span_b);
            if (a.out_node) st.node[t] = v;
            if (a.out_link) st.link[t] = link;
            if (a.out_lat) st.lat[t] = a.lat[r + cv];
            if (a.out_loss) st.loss[t] = a.loss[r + cv];
          } else {
            if (a.out_node) a.out_node[k] = v;
            if (a.out_link) a.out_link[k] = link;
            if (a.out_lat) a.out_lat[k] = a.lat[r + cv];
            if (a.out_loss) a.out_loss[k] = a.loss[r + cv];
          }
          if (u == s) break;
          v = u;
          cv = cu;
        }
      }
    }
    if (STAGE) {
      __syncthreads();  // the wave's records are in its LDS
      for (uint32_t t = lane; t < span; t += 64) {
        if (a.out_node) a.out_node[span_b + t] = st.node[t];
        if (a.out_link) a.out_link[span_b + t] = st.link[t];
        if (a.out_lat) a.out_lat[span_b + t] = st.lat[t];
        if (a.out_loss) a.out_loss[span_b + t] = st.loss[t];
      }
      __syncthreads();  // read before the next trip's records overwrite it
    }
  }
}

// ---- host
struct PathCall {
  sg_ctx* ctx;
  sg_net* net;
  bool packet_form;  // hosts, packets, status; else the pair arrays
  sg_hosts* hosts;
  const uint32_t* nodes;
  uint32_t n_nodes, row_begin, row_end, flags;
  const uint32_t* pred;
  const uint64_t* lat;
  const float* loss;
  const sg_packets* packets;
  const uint8_t* status;
  uint32_t n_pairs;
  const uint32_t* pair_row;
  const uint32_t* pair_col;
  uint64_t* out_off;
  uint32_t* out_node;
  uint32_t* out_link;
  uint64_t* out_lat;
  float* out_loss;
  uint64_t cap;
  uint64_t* total;
};

static void paths_run(const PathCall& c) {
  sg_ctx* ctx = c.ctx;
  sg_net* net = c.net;
  const bool packets = c.packet_form;
  check_rows_call(ctx, net, c.nodes, c.n_nodes, c.row_begin, c.row_end);
  check_node_list(net, c.nodes, c.n_nodes);  // in range and none twice: with n_nodes entries, a permutation
  if (!c.out_node && !c.out_link && !c.out_lat && !c.out_loss) throw Error(SG_ERR_INVALID_ARG, "no record output");
  if (!c.out_off || !c.total) throw Error(SG_ERR_INVALID_ARG, "null out_off or total");
  if (c.out_lat && !c.lat) throw Error(SG_ERR_INVALID_ARG, "out_latency_ns needs the latency_ns rows");
  if (c.out_loss && !c.loss) throw Error(SG_ERR_INVALID_ARG, "out_packet_loss needs the packet_loss rows");
  uint32_t ni = c.n_pairs;
  if (packets) {
    if (!c.hosts || c.hosts->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "host table belongs to another context");
    if (!c.packets) throw Error(SG_ERR_INVALID_ARG, "null packets");
    ni = c.packets->n_packets;
    if (ni && (!c.packets->src_host || !c.packets->dst_ipv4)) throw Error(SG_ERR_INVALID_ARG, "null packet arrays");
  } else if (ni && (!c.pair_row || !c.pair_col)) {
    throw Error(SG_ERR_INVALID_ARG, "null pair arrays");
  }
  if (c.row_end > c.row_begin && !c.pred) throw Error(SG_ERR_INVALID_ARG, "null pred rows");
  hipStream_t st = ctx->stream;
  const bool dev = (c.flags & SG_ROUTE_OUT_DEVICE) != 0;
  const uint32_t n = c.n_nodes, rows = c.row_end - c.row_begin;
  if (ni == 0) {
    if (dev) {
      SG_HIP(hipMemsetAsync(c.out_off, 0, 8, st));
      SG_HIP(hipStreamSynchronize(st));
    } else {
      c.out_off[0] = 0;
    }
    *c.total = 0;
    return;
  }
  ensure_links(ctx, net);
  if (!ctx->paths_ret) SG_HIP(hipHostMalloc(&ctx->paths_ret, 16, hipHostMallocMapped | hipHostMallocCoherent));
  // host arrays in: device copies
  const uint32_t* d_pred = c.pred;
  const uint64_t* d_lat = c.out_lat ? c.lat : nullptr;
  const float* d_loss = c.out_loss ? c.loss : nullptr;
  const uint32_t* d_prow = c.pair_row;
  const uint32_t* d_pcol = c.pair_col;
  uint64_t* d_off = c.out_off;
  if (!dev) {
    const size_t cells = (size_t)rows * n;
    uint32_t* up = ctx->l_pred.get<uint32_t>(cells);
    if (cells) SG_HIP(hipMemcpyAsync(up, c.pred, cells * 4, hipMemcpyHostToDevice, st));
    d_pred = up;
    if (d_lat) {
      uint64_t* ul = ctx->p_lat.get<uint64_t>(cells);
      if (cells) SG_HIP(hipMemcpyAsync(ul, c.lat, cells * 8, hipMemcpyHostToDevice, st));
      d_lat = ul;
    }
    if (d_loss) {
      float* uf = ctx->p_loss.get<float>(cells);
      if (cells) SG_HIP(hipMemcpyAsync(uf, c.loss, cells * 4, hipMemcpyHostToDevice, st));
      d_loss = uf;
    }
    if (!packets) {
      uint32_t* pr = ctx->p_pair.get<uint32_t>(2 * (size_t)ni);
      SG_HIP(hipMemcpyAsync(pr, c.pair_row, (size_t)ni * 4, hipMemcpyHostToDevice, st));
      SG_HIP(hipMemcpyAsync(pr + ni, c.pair_col, (size_t)ni * 4, hipMemcpyHostToDevice, st));
      d_prow = pr;
      d_pcol = pr + ni;
    }
    d_off = ctx->p_off.get<uint64_t>((size_t)ni + 1);
  }
  uint32_t* d_idx = link_node_index(ctx, c.nodes, n);
  unsigned long long* bad = ctx->l_flag.get<unsigned long long>(WALK_WORDS);
  SG_HIP(hipMemsetAsync(bad, 0xff, WALK_WORDS * 8, st));
  PathArgs a;
  a.l = link_args(net, d_idx, n, c.row_begin, rows, d_pred, bad);
  a.pk = packets ? packet_args(c.hosts, c.packets, c.status) : PacketArgs{};
  a.pair_row = d_prow;
  a.pair_col = d_pcol;
  a.n_items = ni;
  a.cnt = ctx->p_cnt.get<uint32_t>(ni);
  a.off = (unsigned long long*)d_off;
  a.lat = (const unsigned long long*)d_lat;
  a.loss = d_loss;
  a.out_node = nullptr;
  a.out_link = nullptr;
  a.out_lat = nullptr;
  a.out_loss = nullptr;
  a.stage_hops = 0;
  const dim3 grid(grid_for(ni, PA_THREADS, 16u * (unsigned)ctx->n_cu));
  {
    // (work = the records, added below once the total is read)
    TimedLaunch tl(ctx, "tree_paths_count", 0.0);
    if (packets)
      hipLaunchKernelGGL(k_paths_count<true>, grid, dim3(PA_THREADS), 0, st, a);
    else
      hipLaunchKernelGGL(k_paths_count<false>, grid, dim3(PA_THREADS), 0, st, a);
    SG_CHECK_LAUNCH();
  }
  {
    TimedLaunch tl(ctx, "tree_paths_scan", (double)ni);
    scan_counts(ctx, a.cnt, ni, a.off, ctx->paths_ret);
  }
  if (!dev) SG_HIP(hipMemcpyAsync(c.out_off, d_off, ((size_t)ni + 1) * 8, hipMemcpyDeviceToHost, st));
  unsigned long long h[WALK_WORDS];
  copy_to_host(ctx, h, bad, sizeof(h));
  const uint64_t tot = *ctx->paths_ret;
  timer_add_work(ctx, "tree_paths_count", (double)tot);
  if (h[WALK_BAD_ITEM] != ~0ull) throw_item_error(packets, h[WALK_BAD_ITEM]);
  if (h[WALK_BAD_RANGE] != ~0ull || h[WALK_BAD_CYCLE] != ~0ull) {
    const int kind = h[WALK_BAD_RANGE] <= h[WALK_BAD_CYCLE] ? WALK_BAD_RANGE : WALK_BAD_CYCLE;
    throw_pred_error(net, c.nodes, kind, h[kind]);
  }
  *c.total = tot;
  if (tot > c.cap)
    throw Error(SG_ERR_CAPACITY, "the paths hold " + std::to_string(tot) + " hop records, the arrays " + std::to_string(c.cap));
  if (tot == 0) return;
  // host arrays out: device copies of the records
  a.out_node = c.out_node;
  a.out_link = c.out_link;
  a.out_lat = (unsigned long long*)c.out_lat;
  a.out_loss = c.out_loss;
  if (!dev) {
    if (c.out_node) a.out_node = ctx->p_node.get<uint32_t>(tot);
    if (c.out_link) a.out_link = ctx->p_link.get<uint32_t>(tot);
    if (c.out_lat) a.out_lat = ctx->p_olat.get<unsigned long long>(tot);
    if (c.out_loss) a.out_loss = ctx->p_oloss.get<float>(tot);
  }
  const bool stage = knob_int("SG_PATHS_STAGE", 1) != 0;
  a.stage_hops = (uint32_t)knob_int("SG_PATHS_STAGE_HOPS", PA_STAGE_HOPS, 1, PA_STAGE_HOPS_MAX);
  {
    TimedLaunch tl(ctx, "tree_paths_fill", (double)tot);
    if (stage) {
      const size_t dyn =
          (PA_THREADS / 64) * path_stage_bytes(a.stage_hops, a.out_node, a.out_link, a.out_lat, a.out_loss);
      const void* fn = packets ? (const void*)k_paths_fill<true, true> : (const void*)k_paths_fill<false, true>;
      SG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
      if (packets)
        hipLaunchKernelGGL((k_paths_fill<true, true>), grid, dim3(PA_THREADS), dyn, st, a);
      else
        hipLaunchKernelGGL((k_paths_fill<false, true>), grid, dim3(PA_THREADS), dyn, st, a);
    } else if (packets) {
      hipLaunchKernelGGL((k_paths_fill<true, false>), grid, dim3(PA_THREADS), 0, st, a);
    } else {
      hipLaunchKernelGGL((k_paths_fill<false, false>), grid, dim3(PA_THREADS), 0, st, a);
    }
    SG_CHECK_LAUNCH();
  }
  if (!dev) {
    if (c.out_node) SG_HIP(hipMemcpyAsync(c.out_node, a.out_node, tot * 4, hipMemcpyDeviceToHost, st));
    if (c.out_link) SG_HIP(hipMemcpyAsync(c.out_link, a.out_link, tot * 4, hipMemcpyDeviceToHost, st));
    if (c.out_lat) SG_HIP(hipMemcpyAsync(c.out_lat, a.out_lat, tot * 8, hipMemcpyDeviceToHost, st));
    if (c.out_loss) SG_HIP(hipMemcpyAsync(c.out_loss, a.out_loss, tot * 4, hipMemcpyDeviceToHost, st));
  }
  copy_to_host(ctx, h, bad, sizeof(h));
  if (h[WALK_BAD_LINK] != ~0ull) throw_pred_error(net, c.nodes, WALK_BAD_LINK, h[WALK_BAD_LINK]);
}

}  // namespace sg

extern "C" {

int32_t sg_tree_paths(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes, uint32_t row_begin,
                      uint32_t row_end, uint32_t flags, const uint32_t* pred, const uint64_t* latency_ns,
                      const float* packet_loss, uint32_t n_pairs, const uint32_t* pair_row, const uint32_t* pair_col,
                      uint64_t* out_off, uint32_t* out_node, uint32_t* out_link, uint64_t* out_latency_ns,
                      float* out_packet_loss, uint64_t cap, uint64_t* total) {
  return sg::guarded(ctx, [&] {
    sg::paths_run(sg::PathCall{ctx, net, false, nullptr, nodes, n_nodes, row_begin, row_end, flags, pred, latency_ns,
                               packet_loss, nullptr, nullptr, n_pairs, pair_row, pair_col, out_off, out_node, out_link,
                               out_latency_ns, out_packet_loss, cap, total});
  });
}

int32_t sg_tree_paths_packets(sg_ctx* ctx, sg_net* net, sg_hosts* hosts, const uint32_t* nodes, uint32_t n_nodes,
                              uint32_t row_begin, uint32_t row_end, uint32_t flags, const uint32_t* pred,
                              const uint64_t* latency_ns, const float* packet_loss, const sg_packets* packets,
                              const uint8_t* status, uint64_t* out_off, uint32_t* out_node, uint32_t* out_link,
                              uint64_t* out_latency_ns, float* out_packet_loss, uint64_t cap, uint64_t* total) {
  return sg::guarded(ctx, [&] {
    sg::paths_run(sg::PathCall{ctx, net, true, hosts, nodes, n_nodes, row_begin, row_end, flags, pred, latency_ns,
                               packet_loss, packets, status, 0, nullptr, nullptr, out_off, out_node, out_link,
                               out_latency_ns, out_packet_loss, cap, total});
  });
}

}  // extern "C"
