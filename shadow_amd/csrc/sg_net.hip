// sg_net.hip -- the device-resident network graph (sg_net): upload of the GML edge
// list, the out-arc CSR every search reads, the in-arc CSC built on first use, and
// the self-loop census for get_edge_weight(n, n).  Arcs run both directions when the
// graph is undirected (petgraph semantics, graph/mod.rs:137-152).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"

namespace sg {

// Two zero fills as one launch (the upload's degree counters and self-loop census; an unplanned
// LDS search's row flags and claim counters): two hipMemsetAsync calls cost ~16 us of host time
// and two fill dispatches on the device
__global__ void k_zero2(uint32_t* __restrict__ a, uint32_t na, uint32_t* __restrict__ b, uint32_t nb) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += gridDim.x * blockDim.x) {
    if (i < na) a[i] = 0u;
    else b[i - na] = 0u;
  }
}

void launch_zero2(sg_ctx* ctx, uint32_t* a, uint32_t na, uint32_t* b, uint32_t nb) {
  hipLaunchKernelGGL(k_zero2, dim3(grid_for((size_t)na + nb, 256, 1024)), dim3(256), 0, ctx->stream, a, na, b, nb);
  SG_CHECK_LAUNCH();
}

// One pass over the edges for both arc lists and the self-loop census (a graph
// upload is part of every one-shot build: three launches instead of six).
__global__ void k_net_count(const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst, uint32_t m,
                            int directed, uint32_t* __restrict__ indeg, uint32_t* __restrict__ outdeg,
                            uint32_t* __restrict__ self_cnt, uint32_t* __restrict__ self_edge) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < m; e += gridDim.x * blockDim.x) {
    const uint32_t s = src[e], d = dst[e];
    if (s == d) {
      atomicAdd(&self_cnt[s], 1u);
      self_edge[s] = e;  // meaningful only when the count ends at 1
      continue;
    }
    atomicAdd(&indeg[d], 1u);
    atomicAdd(&outdeg[s], 1u);
    if (!directed) {
      atomicAdd(&indeg[s], 1u);
      atomicAdd(&outdeg[d], 1u);
    }
  }
}

// Graphs of up to NET_LDS_NODES nodes (C2: a 1,200-node complete graph, 720k edges)
// count and place their arcs through per-block LDS counters: the global degree and
// cursor atomics of k_net_count / k_net_scatter all land on a few thousand words there
// (C2: 0.63 + 1.39 ms).  A block takes a contiguous run of edges; it adds its per-node
// counts to the global ones once, and reserves each node's range for its arcs with one
// returning atomic per node, then places them with LDS cursors.
constexpr uint32_t NET_LDS_NODES = 4096;
constexpr uint32_t NET_LDS_BLOCKS = 256;
__global__ void __launch_bounds__(256) k_net_count_lds(const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                                                       uint32_t m, uint32_t n, int directed,
                                                       uint32_t* __restrict__ indeg, uint32_t* __restrict__ outdeg,
                                                       uint32_t* __restrict__ self_cnt,
                                                       uint32_t* __restrict__ self_edge) {
  __shared__ uint32_t s_in[NET_LDS_NODES], s_out[NET_LDS_NODES];
  for (uint32_t v = threadIdx.x; v < n; v += 256) s_in[v] = s_out[v] = 0;
  __syncthreads();
  const uint32_t per = (m + gridDim.x - 1) / gridDim.x, e0 = blockIdx.x * per, e1 = min(e0 + per, m);
  for (uint32_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const uint32_t s = src[e], d = dst[e];
    if (s == d) {
      atomicAdd(&self_cnt[s], 1u);
      self_edge[s] = e;  // meaningful only when the count ends at 1
      continue;
    }
    atomicAdd(&s_in[d], 1u);
    atomicAdd(&s_out[s], 1u);
    if (!directed) {
      atomicAdd(&s_in[s], 1u);
      atomicAdd(&s_out[d], 1u);
    }
  }
  __syncthreads();
  for (uint32_t v = threadIdx.x; v < n; v += 256) {
    if (s_in[v]) atomicAdd(&indeg[v], s_in[v]);
    if (s_out[v]) atomicAdd(&outdeg[v], s_out[v]);
  }
}

// OUT: the out-arcs (out_arc, every search's input) -- the upload; CSC: the in-arcs (in_src,
// in_lat, in_om, in_rec: the slab and wide kernels' and a directed plan's input) -- built on
// first use (ensure_csc), so an upload writes 12 B per arc instead of 52.
template <bool OUT, bool CSC>
__global__ void __launch_bounds__(256) k_net_scatter_lds(const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                                                         const uint64_t* __restrict__ lat, const float* __restrict__ loss,
                                                         uint32_t m, uint32_t n, int directed,
                                                         uint32_t* __restrict__ cursor, uint32_t* __restrict__ in_src,
                                                         uint64_t* __restrict__ in_lat, float* __restrict__ in_om,
                                                         uint4* __restrict__ in_rec, uint32_t* __restrict__ ocursor,
                                                         uint32_t* __restrict__ out_arc) {
  __shared__ uint32_t s_in[NET_LDS_NODES], s_out[NET_LDS_NODES];  // counts, then the block's cursors
  for (uint32_t v = threadIdx.x; v < n; v += 256) s_in[v] = s_out[v] = 0;
  __syncthreads();
  const uint32_t per = (m + gridDim.x - 1) / gridDim.x, e0 = blockIdx.x * per, e1 = min(e0 + per, m);
  for (uint32_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const uint32_t s = src[e], d = dst[e];
    if (s == d) continue;
    if (CSC) atomicAdd(&s_in[d], 1u);
    if (OUT) atomicAdd(&s_out[s], 1u);
    if (!directed) {
      if (CSC) atomicAdd(&s_in[s], 1u);
      if (OUT) atomicAdd(&s_out[d], 1u);
    }
  }
  __syncthreads();
  for (uint32_t v = threadIdx.x; v < n; v += 256) {  // this block's ranges
    if (CSC && s_in[v]) s_in[v] = atomicAdd(&cursor[v], s_in[v]);
    if (OUT && s_out[v]) s_out[v] = atomicAdd(&ocursor[v], s_out[v]);
  }
  __syncthreads();
  for (uint32_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const uint32_t s = src[e], d = dst[e];
    if (s == d) continue;  // a self-loop never improves D[s][v] (latency >= 1)
    const float om = __fsub_rn(1.0f, loss[e]);
    const uint64_t l = lat[e];
    const uint32_t l32 = l < LAT32_SAT ? (uint32_t)l : LAT32_SAT;
    for (int dir = 0; dir < (directed ? 1 : 2); dir++) {
      const uint32_t a = dir ? d : s, b = dir ? s : d;  // the arc a -> b
      if (CSC) {
        const uint32_t p = atomicAdd(&s_in[b], 1u);
        in_src[p] = a;
        in_lat[p] = l;
        in_om[p] = om;
        in_rec[p] = make_uint4(a, b, l32, __float_as_uint(om));
      }
      if (OUT) {
        const uint32_t q = atomicAdd(&s_out[a], 1u);
        out_arc[3 * (size_t)q] = b;
        out_arc[3 * (size_t)q + 1] = l32;
        out_arc[3 * (size_t)q + 2] = __float_as_uint(om);
      }
    }
  }
}

// Exclusive scans of indeg and outdeg (n + 1 entries each, the last one the
// total) in one workgroup, each result written twice: the offsets and the
// scatter's cursors.  For graphs up to NET_SCAN_SMALL nodes.  Both arrays in one
// pass over chunks of 16 x 1024 consecutive entries (32 branch-free loads in flight
// per thread); a thread's running offset carries across chunks in a register, and
// the offsets go out through LDS as coalesced stores.  (The earlier form gave each
// thread 10+ strided entries, one array at a time: 22 us at C3; with 8 entries per
// thread and stores straight from registers, 28 us; through LDS, 14.7 us.)
constexpr uint32_t NET_SCAN_SMALL = 1u << 17;
__global__ void __launch_bounds__(1024) k_net_scan(const uint32_t* __restrict__ indeg, const uint32_t* __restrict__ outdeg,
                                                   uint32_t n, uint32_t* __restrict__ in_off, uint32_t* __restrict__ in_cur,
                                                   uint32_t* __restrict__ out_off, uint32_t* __restrict__ out_cur) {
  constexpr int PER = 16;  // one chunk up to 16,383 nodes
  __shared__ uint32_t s_w[2][16];
  __shared__ uint32_t s_x[2][PER * 1024];  // 128 KB
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // branch-free loads (past n: an out-of-range offset reads 0), so all 16 are in flight
  // at once; with a branch per element the compiler waited for each load in turn
  const __amdgpu_buffer_rsrc_t ri = __builtin_amdgcn_make_buffer_rsrc((void*)indeg, 0, (int)(n * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)outdeg, 0, (int)(n * 4u), 0x00020000);
  uint32_t carry_i = 0, carry_o = 0;
  for (uint32_t base = 0; base <= n; base += PER * 1024) {
    uint32_t xi[PER], xo[PER];
    uint32_t si = 0, so = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const uint32_t i = base + (uint32_t)tid * PER + k;
      xi[k] = __builtin_amdgcn_raw_buffer_load_b32(ri, i < n ? i * 4u : 0x80000000u, 0, 0);
      xo[k] = __builtin_amdgcn_raw_buffer_load_b32(ro, i < n ? i * 4u : 0x80000000u, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < PER; k++) {
      si += xi[k];
      so += xo[k];
    }
    const uint32_t ii = wave_incl_sum(si), io = wave_incl_sum(so);
    if (lane == 63) {
      s_w[0][wv] = ii;
      s_w[1][wv] = io;
    }
    __syncthreads();
    uint32_t pi = carry_i + ii - si, po = carry_o + io - so;
    for (int w = 0; w < 16; w++) {
      const uint32_t a = s_w[0][w], b = s_w[1][w];
      pi += w < wv ? a : 0u;
      po += w < wv ? b : 0u;
      carry_i += a;
      carry_o += b;
    }
    // the chunk's offsets through LDS, then stored coalesced (entry base + k * 1024 + tid)
#pragma unroll
    for (int k = 0; k < PER; k++) {
      s_x[0][tid * PER + k] = pi;
      s_x[1][tid * PER + k] = po;
      pi += xi[k];
      po += xo[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const uint32_t i = base + (uint32_t)k * 1024 + tid;
      const uint32_t a = s_x[0][k * 1024 + tid], b = s_x[1][k * 1024 + tid];
      if (i <= n) {
        in_off[i] = a;
        in_cur[i] = a;
        out_off[i] = b;
        out_cur[i] = b;
      }
    }
    __syncthreads();  // s_w and s_x are rewritten by the next chunk
  }
}

template <bool OUT, bool CSC>  // (as k_net_scatter_lds)
__global__ void k_net_scatter(const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                              const uint64_t* __restrict__ lat, const float* __restrict__ loss, uint32_t m,
                              int directed, uint32_t* __restrict__ cursor, uint32_t* __restrict__ in_src,
                              uint64_t* __restrict__ in_lat, float* __restrict__ in_om, uint4* __restrict__ in_rec,
                              uint32_t* __restrict__ ocursor, uint32_t* __restrict__ out_arc) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < m; e += gridDim.x * blockDim.x) {
    const uint32_t s = src[e], d = dst[e];
    if (s == d) continue;  // a self-loop never improves D[s][v] (latency >= 1)
    const float om = __fsub_rn(1.0f, loss[e]);
    const uint64_t l = lat[e];
    const uint32_t l32 = l < LAT32_SAT ? (uint32_t)l : LAT32_SAT;
    for (int dir = 0; dir < (directed ? 1 : 2); dir++) {
      const uint32_t a = dir ? d : s, b = dir ? s : d;  // the arc a -> b
      if (CSC) {
        const uint32_t p = atomicAdd(&cursor[b], 1u);
        in_src[p] = a;
        in_lat[p] = l;
        in_om[p] = om;
        in_rec[p] = make_uint4(a, b, l32, __float_as_uint(om));
      }
      if (OUT) {
        const uint32_t q = atomicAdd(&ocursor[a], 1u);
        out_arc[3 * (size_t)q] = b;
        out_arc[3 * (size_t)q + 1] = l32;
        out_arc[3 * (size_t)q + 2] = __float_as_uint(om);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Host orchestration
// ---------------------------------------------------------------------------
std::string node_name(const sg_net* net, uint32_t idx) {
  uint32_t id = net->gml_id.empty() ? idx : net->gml_id[idx];
  return std::to_string(id);
}

struct NetKnobs {
  bool trace;        // SG_NET_TRACE (diagnostics: host phases on stderr)
  uint32_t threads;  // SG_NET_THREADS (A/B diagnostics, 1 = one thread): staging threads of a large edge list
  bool lds;          // SG_NET_LDS (=0: A/B): per-block LDS counters up to NET_LDS_NODES nodes
  bool bucket;       // SG_APSP_BUCKET=1: the bucketed search takes this graph whatever its size
};
static NetKnobs net_knobs() {
  NetKnobs k;
  k.trace = knob_int("SG_NET_TRACE", 0) != 0;
  k.threads = (uint32_t)knob_int("SG_NET_THREADS", 4, 1, 4);
  k.lds = knob_int("SG_NET_LDS", 1) != 0;
  k.bucket = knob_int("SG_APSP_BUCKET", -1) == 1;
  return k;
}

// A fresh network per simulation (the reference builds its graph once and computes
// the table once, sim_config.rs:76-79, :137-141): one device allocation for every
// array, the arc count from the host edge list (no device round trip), and no
// stream synchronisation -- the build that follows orders after these launches.
static void build_net(sg_ctx* ctx, const sg_graph* g, sg_net* net) {
  const NetKnobs knobs = net_knobs();
  const uint32_t n = g->n_nodes, m = g->n_edges;
  if (m && (!g->edge_src || !g->edge_dst || !g->edge_latency_ns || !g->edge_packet_loss))
    throw Error(SG_ERR_INVALID_ARG, "null edge array");
  // Validation, in branch-free passes over the edge arrays (part of every one-shot
  // build).  One thread: the endpoints (and the self-loop count the sizes need) before
  // anything is allocated, the losses and latencies, which index nothing, after the
  // upload's launches, while the device runs them.  Large lists: every check in the
  // threaded staging pass below, before any launch.  Either way a bad edge is named by
  // the per-edge loop, which checks every rule edge by edge (the reference's order).
  const uint32_t* __restrict__ es = g->edge_src;
  const uint32_t* __restrict__ ed = g->edge_dst;
  const uint64_t* __restrict__ el = g->edge_latency_ns;
  const float* __restrict__ ef = g->edge_packet_loss;
  const bool trace = knobs.trace;
  auto now_us = []() {
    return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count() / 1e3;
  };
  const double tr0 = trace ? now_us() : 0.0;
  double tr[6] = {0, 0, 0, 0, 0, 0};
  auto name_bad_edge = [&]() {
    for (uint32_t e = 0; e < m; e++) {
      if (es[e] >= n || ed[e] >= n)
        throw Error(SG_ERR_INVALID_ARG, "edge " + std::to_string(e) + " endpoint out of range");
      const float l = ef[e];
      if (!(l >= 0.0f && l <= 1.0f))  // graph/mod.rs:101-103 (NaN rejected too)
        throw Error(SG_ERR_INVALID_ARG, "Edge 'packet_loss' is not in the range [0,1]");
      if (el[e] == 0)  // graph/mod.rs:105-107
        throw Error(SG_ERR_INVALID_ARG, "Edge 'latency' must not be 0");
    }
  };
  // one allocation, 256-B aligned sub-arrays; the edge arrays first (their offsets depend on m
  // only, so they can be staged before the self-loop count sizes the rest)
  size_t total = 0;
  constexpr size_t align = 256;
  auto carve = [&](size_t bytes) {
    const size_t o = total;
    total += (std::max<size_t>(bytes, 16) + align - 1) / align * align;
    return o;
  };
  const size_t o_esrc = carve(m * 4ull), o_edst = carve(m * 4ull), o_elat = carve(m * 8ull),
               o_eloss = carve(m * 4ull);
  const size_t eb = total;  // bytes of the edge arrays, up to the first derived array
  // Large edge lists (C2's 720k edges): validation and the copy into the pinned staging over
  // up to 4 host threads (one thread 349 us, 4 threads 134 us on the MI355X box's host;
  // tools/debug/stage_thread_probe.cpp), in two parts, each DMA'd as soon as it is staged:
  // (A) the endpoints -- checked, self-loops counted -- then (B) the latencies and losses --
  // checked -- while A's DMA runs.  The block is sized for no self-loops, since it is allocated
  // before the count is known (the arrays then have a little unused room).  Small lists
  // (C3's 50k edges: 22 us) take one thread, where the threads' start-up costs more than they
  // save, and check the losses and latencies after the upload's launches.
  const uint64_t arcs_cap = (uint64_t)m * (g->directed ? 1u : 2u);
  const uint32_t n_thr = m >= (1u << 18) && arcs_cap < (1ull << 32) ? knobs.threads : 1u;
  const bool threaded = n_thr > 1;
  uint64_t n_self = 0;
  if (!threaded) {
    uint32_t bad = 0, ns = 0;
    for (uint32_t e = 0; e < m; e++) {
      const uint32_t a = es[e], b = ed[e];
      bad |= (uint32_t)(a >= n) | (uint32_t)(b >= n);
      ns += a == b;
    }
    if (bad) name_bad_edge();
    n_self = ns;
  }
  if (trace) tr[0] = now_us();
  // arcs without self-loops, both directions when undirected (petgraph semantics, graph/mod.rs:137-152)
  const uint64_t arcs_sz = threaded ? arcs_cap : ((uint64_t)m - n_self) * (g->directed ? 1u : 2u);
  if (arcs_sz >= (1ull << 32)) throw Error(SG_ERR_INVALID_ARG, "too many arcs");
  const uint32_t n_arcs_sz = (uint32_t)arcs_sz;  // the layout's arc count (an upper bound when threaded)
  net->ctx = ctx;
  net->n_nodes = n;
  net->n_edges = m;
  net->directed = g->directed != 0;
  if (g->node_gml_id) net->gml_id.assign(g->node_gml_id, g->node_gml_id + n);
  hipStream_t st = ctx->stream;
  const size_t o_inoff = carve(((size_t)n + 1) * 4), o_scnt = carve((size_t)n * 4),
               o_sedge = carve((size_t)n * 4), o_insrc = carve(n_arcs_sz * 4ull),
               o_inlat = carve(n_arcs_sz * 8ull), o_inom = carve(n_arcs_sz * 4ull),
               o_inrec = carve(n_arcs_sz * 16ull), o_outoff = carve(((size_t)n + 1) * 4),
               o_outarc = carve(n_arcs_sz * 12ull);
  {  // a released block of the right size from the context's pool, else a new one
    size_t best = ~(size_t)0;
    for (size_t i = 0; i < ctx->net_pool.size(); i++) {
      const size_t b = ctx->net_pool[i].bytes;
      if (b >= total && b <= 2 * total + (1u << 20) && (best == ~(size_t)0 || b < ctx->net_pool[best].bytes)) best = i;
    }
    if (best != ~(size_t)0) {
      auto blk = ctx->net_pool[best];
      ctx->net_pool.erase(ctx->net_pool.begin() + best);
      SG_HIP(hipStreamWaitEvent(ctx->stream, blk.freed, 0));
      (void)hipEventDestroy(blk.freed);
      net->mem = blk.p;
      net->mem_bytes = blk.bytes;
    } else {
      SG_HIP(hipMalloc(&net->mem, total));
      net->mem_bytes = total;
    }
  }
  if (trace) tr[1] = now_us();
  char* base = (char*)net->mem;
  net->e_src = (uint32_t*)(base + o_esrc);
  net->e_dst = (uint32_t*)(base + o_edst);
  net->e_lat = (uint64_t*)(base + o_elat);
  net->e_loss = (float*)(base + o_eloss);
  net->in_off = (uint32_t*)(base + o_inoff);
  net->self_cnt = (uint32_t*)(base + o_scnt);
  net->self_edge = (uint32_t*)(base + o_sedge);
  net->in_src = (uint32_t*)(base + o_insrc);
  net->in_lat = (uint64_t*)(base + o_inlat);
  net->in_om = (float*)(base + o_inom);
  net->in_rec = (uint4*)(base + o_inrec);
  net->out_off = (uint32_t*)(base + o_outoff);
  net->out_arc = (uint32_t*)(base + o_outarc);
  // a bad edge found once the block is allocated: nothing may still run on the block when
  // the caller deletes the net, then the per-edge loop names it
  auto reject = [&]() {
    (void)hipStreamSynchronize(st);
    (void)hipFree(net->mem);
    net->mem = nullptr;
    name_bad_edge();
  };
  bool checked = false;  // losses and latencies checked (threaded: in part B)
  if (threaded) {
    char* staged = stage_acquire(ctx, 0, eb);
    std::vector<uint32_t> bad_t(n_thr, 0u), ns_t(n_thr, 0u);
    std::atomic<uint32_t> done_a{0u}, done_b{0u};
    auto range = [&](uint32_t t, uint32_t& e0, uint32_t& e1) {
      e0 = (uint32_t)((uint64_t)m * t / n_thr);
      e1 = (uint32_t)((uint64_t)m * (t + 1) / n_thr);
    };
    auto part_a = [&](uint32_t t) {  // endpoints: checked, self-loops counted, staged
      uint32_t e0, e1, bad = 0, ns = 0;
      range(t, e0, e1);
      for (uint32_t e = e0; e < e1; e++) {
        const uint32_t a = es[e], b = ed[e];
        bad |= (uint32_t)(a >= n) | (uint32_t)(b >= n);
        ns += a == b;
      }
      memcpy(staged + o_esrc + e0 * 4ull, es + e0, (e1 - e0) * 4ull);
      memcpy(staged + o_edst + e0 * 4ull, ed + e0, (e1 - e0) * 4ull);
      bad_t[t] = bad;
      ns_t[t] = ns;
      done_a.fetch_add(1u, std::memory_order_release);
    };
    auto part_b = [&](uint32_t t) {  // losses and latencies: checked, staged
      uint32_t e0, e1, bad = 0;
      range(t, e0, e1);
      for (uint32_t e = e0; e < e1; e++) bad |= (uint32_t)!(ef[e] >= 0.0f) | (uint32_t)!(ef[e] <= 1.0f);
      for (uint32_t e = e0; e < e1; e++) bad |= (uint32_t)(el[e] == 0);
      memcpy(staged + o_elat + e0 * 8ull, el + e0, (e1 - e0) * 8ull);
      memcpy(staged + o_eloss + e0 * 4ull, ef + e0, (e1 - e0) * 4ull);
      bad_t[t] |= bad;
      done_b.fetch_add(1u, std::memory_order_release);
    };
    std::vector<std::thread> pool;
    struct Joiner {  // every started thread is joined, whatever is thrown below
      std::vector<std::thread>& p;
      ~Joiner() {
        for (auto& th : p)
          if (th.joinable()) th.join();
      }
    } joiner{pool};
    uint32_t started = 1;  // threads 1 .. started-1 run their parts; this thread runs the others
    try {
      for (uint32_t t = 1; t < n_thr; t++, started++)
        pool.emplace_back([&, t] {
          part_a(t);
          part_b(t);
        });
    } catch (const std::system_error&) {
    }
    // each part's DMA once every thread has staged it: A's runs while part B is staged
    for (uint32_t t = 0; t < n_thr; t++)
      if (t == 0 || t >= started) part_a(t);
    while (done_a.load(std::memory_order_acquire) < n_thr) std::this_thread::yield();
    const hipError_t ea = hipMemcpyAsync(base, staged, o_elat, hipMemcpyHostToDevice, st);
    for (uint32_t t = 0; t < n_thr; t++)
      if (t == 0 || t >= started) part_b(t);
    while (done_b.load(std::memory_order_acquire) < n_thr) std::this_thread::yield();
    const hipError_t eb2 = ea == hipSuccess ? hipMemcpyAsync(base + o_elat, staged + o_elat, eb - o_elat,
                                                             hipMemcpyHostToDevice, st)
                                            : ea;
    for (auto& th : pool) th.join();
    SG_HIP(eb2);
    stage_release(ctx, 0);
    uint32_t bad = 0;
    for (uint32_t t = 0; t < n_thr; t++) {
      bad |= bad_t[t];
      n_self += ns_t[t];
    }
    if (bad) reject();
    checked = true;
    if (trace) tr[2] = now_us();
  } else if (m) {  // the edge arrays through the context's pinned staging, one copy (they are adjacent)
    char* h = stage_acquire(ctx, 0, eb);
    memcpy(h + o_esrc, g->edge_src, m * 4ull);
    memcpy(h + o_edst, g->edge_dst, m * 4ull);
    memcpy(h + o_elat, g->edge_latency_ns, m * 8ull);
    memcpy(h + o_eloss, g->edge_packet_loss, m * 4ull);
    if (trace) tr[2] = now_us();
    SG_HIP(hipMemcpyAsync(base, h, eb, hipMemcpyHostToDevice, st));
    stage_release(ctx, 0);
  }
  const uint32_t n_arcs = (uint32_t)(((uint64_t)m - n_self) * (g->directed ? 1u : 2u));
  net->n_arcs = n_arcs;
  if (trace) tr[3] = now_us();
  uint32_t* indeg = ctx->r_misc.get<uint32_t>(2 * ((size_t)n + 1));
  uint32_t* outdeg = indeg + n + 1;
  // the degree counters, and self_cnt with self_edge (adjacent): self_edge stays 0 where no
  // self-loop sets it, so a build that reads it before the self-loop check's error is raised
  // stays in bounds
  launch_zero2(ctx, indeg, 2 * (n + 1), net->self_cnt, (uint32_t)((o_insrc - o_scnt) / 4));
  const bool lds_up = n <= NET_LDS_NODES && knobs.lds;
  const uint32_t lds_blocks = std::max(1u, std::min(NET_LDS_BLOCKS, (m + 255) / 256));
  if (m) {
    if (lds_up)
      hipLaunchKernelGGL(k_net_count_lds, dim3(lds_blocks), dim3(256), 0, st, net->e_src, net->e_dst, m, n,
                         (int)net->directed, indeg, outdeg, net->self_cnt, net->self_edge);
    else
      hipLaunchKernelGGL(k_net_count, dim3(grid_for(m, 256, 8192)), dim3(256), 0, st, net->e_src, net->e_dst, m,
                         (int)net->directed, indeg, outdeg, net->self_cnt, net->self_edge);
    SG_CHECK_LAUNCH();
  }
  uint32_t* cursor = ctx->r_map.get<uint32_t>(2 * ((size_t)n + 1));
  uint32_t* ocursor = cursor + n + 1;
  if (n < NET_SCAN_SMALL) {
    hipLaunchKernelGGL(k_net_scan, dim3(1), dim3(1024), 0, st, indeg, outdeg, n, net->in_off, cursor, net->out_off,
                       ocursor);
    SG_CHECK_LAUNCH();
  } else {
    exclusive_scan_u32(ctx, indeg, net->in_off, n);
    exclusive_scan_u32(ctx, outdeg, net->out_off, n);
    SG_HIP(hipMemcpyAsync(cursor, net->in_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, st));
    SG_HIP(hipMemcpyAsync(ocursor, net->out_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, st));
  }
  if (n_arcs) {
    // the out-arcs only; the in-arcs wait for a search that reads them (ensure_csc)
    if (lds_up)
      hipLaunchKernelGGL((k_net_scatter_lds<true, false>), dim3(lds_blocks), dim3(256), 0, st, net->e_src, net->e_dst,
                         net->e_lat, net->e_loss, m, n, (int)net->directed, cursor, net->in_src, net->in_lat,
                         net->in_om, net->in_rec, ocursor, net->out_arc);
    else
      hipLaunchKernelGGL((k_net_scatter<true, false>), dim3(grid_for(m, 256, 8192)), dim3(256), 0, st, net->e_src,
                         net->e_dst, net->e_lat, net->e_loss, m, (int)net->directed, cursor, net->in_src, net->in_lat,
                         net->in_om, net->in_rec, ocursor, net->out_arc);
    SG_CHECK_LAUNCH();
  }
  {  // the losses and latencies, while the device runs the upload (threaded: checked already)
    uint32_t bad = 0;
    if (!checked) {
      for (uint32_t e = 0; e < m; e++) bad |= (uint32_t)!(ef[e] >= 0.0f) | (uint32_t)!(ef[e] <= 1.0f);
      for (uint32_t e = 0; e < m; e++) bad |= (uint32_t)(el[e] == 0);
    }
    // the arcs' latency statistics the bucketed search sizes its buckets from (graphs past the
    // LDS search, or SG_APSP_BUCKET=1): smallest and mean arc latency, self-loops excluded
    if (!bad && (!sssp_lds_fits(n) || knobs.bucket)) {
      uint64_t lo = LAT32_SAT;
      double sum = 0.0;
      uint64_t cnt = 0;
      for (uint32_t e = 0; e < m; e++) {
        if (es[e] == ed[e]) continue;
        const uint64_t l = std::min<uint64_t>(el[e], LAT32_SAT);
        lo = std::min(lo, l);
        sum += (double)l;
        cnt++;
      }
      net->arc_lat_min = (uint32_t)lo;
      net->arc_lat_mean = cnt ? sum / (double)cnt : 0.0;
    }
    if (trace) {
      tr[4] = now_us();
      fprintf(stderr, "[net] m=%u: endpoint check %.1f us, allocation %.1f, staging copy %.1f, H2D enqueue %.1f, "
              "kernels enqueue + loss/latency check %.1f\n", m, tr[0] - tr0, tr[1] - tr[0], tr[2] - tr[1],
              tr[3] - tr[2], tr[4] - tr[3]);
    }
    if (bad) reject();
  }
}

// The in-arc CSC (in_src, in_lat, in_om, in_rec), built on its first use: the scatter again,
// in-arcs only, from cursors set to in_off (the upload's scan wrote it).
void ensure_csc(sg_ctx* ctx, sg_net* net) {
  if (net->csc) return;
  const uint32_t n = net->n_nodes, m = net->n_edges;
  if (net->n_arcs) {
    hipStream_t st = ctx->stream;
    uint32_t* cursor = ctx->r_map.get<uint32_t>((size_t)n + 1);
    SG_HIP(hipMemcpyAsync(cursor, net->in_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (n <= NET_LDS_NODES && net_knobs().lds)
      hipLaunchKernelGGL((k_net_scatter_lds<false, true>), dim3(std::max(1u, std::min(NET_LDS_BLOCKS, (m + 255) / 256))),
                         dim3(256), 0, st, net->e_src, net->e_dst, net->e_lat, net->e_loss, m, n, (int)net->directed,
                         cursor, net->in_src, net->in_lat, net->in_om, net->in_rec, (uint32_t*)nullptr,
                         (uint32_t*)nullptr);
    else
      hipLaunchKernelGGL((k_net_scatter<false, true>), dim3(grid_for(m, 256, 8192)), dim3(256), 0, st, net->e_src,
                         net->e_dst, net->e_lat, net->e_loss, m, (int)net->directed, cursor, net->in_src,
                         net->in_lat, net->in_om, net->in_rec, (uint32_t*)nullptr, (uint32_t*)nullptr);
    SG_CHECK_LAUNCH();
  }
  net->csc = true;
}

}  // namespace sg

extern "C" {

int32_t sg_net_create(sg_ctx* ctx, const sg_graph* g, sg_net** out) {
  if (!g || !out) return SG_ERR_INVALID_ARG;
  *out = nullptr;
  sg_net* net = nullptr;
  int32_t rc = sg::guarded(ctx, [&] {
    net = new sg_net();
    net->serial = ++ctx->net_serial;
    sg::build_net(ctx, g, net);
  });
  if (rc != SG_OK) {
    delete net;
    return rc;
  }
  *out = net;
  return SG_OK;
}

void sg_net_destroy(sg_net* net) {
  if (!net) return;
  sg_ctx* ctx = net->ctx;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    hipEvent_t ev = nullptr;
    if (net->mem && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess &&
        hipEventRecord(ev, ctx->stream) == hipSuccess) {
      ctx->net_pool.push_back({net->mem, net->mem_bytes, ev});
      net->mem = nullptr;
      while (ctx->net_pool.size() > 4) {  // keep a few blocks; release the oldest
        auto& old = ctx->net_pool.front();
        (void)hipEventSynchronize(old.freed);
        (void)hipEventDestroy(old.freed);
        (void)hipFree(old.p);
        ctx->net_pool.erase(ctx->net_pool.begin());
      }
    } else if (ev) {
      (void)hipEventDestroy(ev);
    }
  }
  delete net;
}

}  // extern "C"
