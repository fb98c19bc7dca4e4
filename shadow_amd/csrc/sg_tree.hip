// sg_tree.hip -- shortest-path trees: predecessor and first-hop rows beside the routing table.
//
// The reference keeps no next-hop table (graph/mod.rs:297-303: a PathProperties is a latency
// and a loss), but its arithmetic pins one: a path is right exactly when the left fold
// default() + e1 + ... + ek (graph/mod.rs:322-331) over its edges gives the table's cell
// (graph/mod.rs:183-228), latency and loss bits alike.  The tree is therefore a function of the
// finished table and the graph; no search changes, this is one pass over finished rows.
//
// Definition.  For a source s let key[v] = (latency, loss bits) be the table's row of s, with
// key[s] = (0, +0.0f), the fold's default() -- not the diagonal cell, which holds the
// self-loop.  An in-arc u -> v (u != v, v != s; parallel edges each count) is TIGHT when
//     key[u].lat + w.lat == key[v].lat   and
//     fold_loss(key[u].loss, 1f32 - w.loss) has exactly key[v]'s loss bits
// (sg_device.h fold_loss / relax32, compiled under -ffp-contract=off).  A correct row has at
// least one tight in-arc per v != s: the fixed point every search computes.
//   pred[s][v]      = the SMALLEST petgraph node index u among v's tight in-arcs; pred[s][s] = s.
//                     By value, never by arc position: the CSC's arc order comes from atomics.
//                     Arc latency is at least 1 ns (graph/mod.rs:105-107), so latencies fall
//                     strictly towards s: every pred row is a tree rooted at s, and by
//                     induction the fold along the tree path to v is key[v], bit for bit.
//   first_hop[s][v] = the node after s on that tree path: v itself when pred[s][v] == s;
//                     first_hop[s][s] = s.
// Both are petgraph NodeIndex values and do not depend on the column order of `nodes`.
//
// A tree spans every graph node, so the rows must too: `nodes` is a permutation of
// 0 .. n_nodes-1 (a simulation with a used subset puts its used nodes first and builds rows
// [0, n_used)).  The f32 loss fold is not associative, so the suffix of s's canonical path
// from an intermediate node h need not be h's own canonical path: paths are expanded inside
// one source's pred row (sg_tree_path), never hop by hop across rows.
//
// Two paths, one definition:
//  * k_tree_lds: one workgroup per row; the row staged in LDS as packed keys
//    (lat32 << 32) | loss bits indexed by node, pred and first_hop as u16 beside it
//    (12 bytes per node: 120 KB at 10k nodes, one row per CU; several rows per CU on small
//    graphs).  The node limit comes from the device's LDS size (tree_lds_max).  A row
//    holding a latency at or past 2^32 - 1 ns leaves for the global path inside the kernel.
//  * k_tree_global: rows past that limit, SG_TREE_LDS=0, and the wide rows above: keys read
//    from the row in memory (u64 latency, the exact in_lat), first hops jumped in the output row.
// The tight test runs over the ARCS, a lane per arc record (coalesced 16-byte loads, four in
// flight per lane), and a tight arc lowers its head's pred with a u32 min -- in LDS, where the
// u32 words lie over the u16 pred and first_hop arrays until the test is done, or in the output
// row.  A thread per node with the wave sharing long arc lists measured 2.3x slower at C3
// (each lane's few loads wait for one another: DESIGN 3.6); by arcs a hub's list is spread over
// the workgroup like any other.  First hops come from pointer jumping in place:
// a[v] = a[a[v]] until a[v] is a child of s; entries that are children of s never change, so
// the unsynchronised form only ever reads an ancestor on v's own path.
// A cell without a tight in-arc means the rows are not this graph's table: the first such
// (row, col) in row-major order goes to a flag word read at the call's one synchronisation.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_links.h"

namespace sg {

constexpr uint32_t TREE_NONE = 0xFFFFFFFFu;
constexpr uint32_t TREE_NONE16 = 0xFFFFu;
constexpr int TREE_ARCS = 4;             // arc records in flight per lane
constexpr int TREE_PER_THREAD = 16;      // LDS path: nodes per thread at most (1,024 threads: 16,384 nodes)
constexpr size_t TREE_STATIC_LDS = 64;   // the kernels' __shared__ words, rounded up
constexpr size_t TREE_NODE_BYTES = 12;   // key u64 + pred u16 + first_hop u16

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct TreeArgs {
  // the net's in-arc CSC (sg_net.hip ensure_csc)
  const uint4* in_rec;  // (source, destination, latency32, bits(1f32 - loss))
  const uint64_t* in_lat;
  uint32_t n_arcs;
  // nodes[j] = the node of column j; pos = its inverse
  const uint32_t* nodes;
  const uint32_t* pos;
  uint32_t n, row_begin, rows;
  // rows [row_begin, row_begin + rows) of the table and of the outputs, row-major from row_begin
  const uint64_t* lat;
  const float* loss;
  uint32_t* pred;
  uint32_t* fh;
  unsigned long long* bad;  // min over untight cells of (row << 32) | col
  int vec;                  // 16-byte stores are aligned in every row
};

// Every arc record once, TREE_ARCS loads in flight per lane: fn(p, record).
template <class F>
__device__ __forceinline__ void for_each_arc(const TreeArgs& a, F fn) {
  const uint32_t T = blockDim.x, m = a.n_arcs;
  for (uint32_t p0 = threadIdx.x; p0 < m; p0 += TREE_ARCS * T) {
    uint4 rec[TREE_ARCS];
#pragma unroll
    for (int k = 0; k < TREE_ARCS; k++) {
      const uint32_t p = p0 + k * T;
      rec[k] = a.in_rec[p < m ? p : p0];
    }
#pragma unroll
    for (int k = 0; k < TREE_ARCS; k++) {
      const uint32_t p = p0 + k * T;
      if (p < m) fn(p, rec[k]);
    }
  }
}

// One row on the global path, by a whole workgroup: keys from the row in memory.
__device__ void tree_row_global(const TreeArgs& a, uint32_t r, uint32_t* s_bad) {
  const uint32_t tid = threadIdx.x, T = blockDim.x, n = a.n;
  const uint32_t s = a.nodes[a.row_begin + r];
  const uint64_t* __restrict__ lat = a.lat + (size_t)r * n;
  const float* __restrict__ loss = a.loss + (size_t)r * n;
  uint32_t* pred = a.pred + (size_t)r * n;
  uint32_t* fh = a.fh + (size_t)r * n;
  // (the mins are taken at the L2: written and read there)
  for (uint32_t j = tid; j < n; j += T)
    __hip_atomic_store(&pred[j], TREE_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  for_each_arc(a, [&](uint32_t p, const uint4& rec) {
    const uint32_t u = rec.x, v = rec.y;
    if (v == s) return;
    const uint64_t w = a.in_lat[p];
    uint64_t lu = 0;
    float fu = 0.0f;
    if (u != s) {
      const uint32_t pu = a.pos[u];
      lu = lat[pu];
      fu = loss[pu];
    }
    const uint32_t pv = a.pos[v];
    const uint64_t sum = lu + w;
    if (sum >= lu && sum == lat[pv] &&
        __float_as_uint(fold_loss(fu, __uint_as_float(rec.w))) == __float_as_uint(loss[pv]))
      atomicMin(&pred[pv], u);
  });
  __syncthreads();
  uint32_t bad = TREE_NONE;
  for (uint32_t j = tid; j < n; j += T) {
    const uint32_t v = a.nodes[j];
    const uint32_t best = __hip_atomic_load(&pred[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == s) {
      pred[j] = s;
      fh[j] = s;
    } else {
      if (best == TREE_NONE) bad = min(bad, j);
      // the jump's start: children of s (and cells without a tight arc) are fixed points
      fh[j] = best == s || best == TREE_NONE ? v : best;
    }
  }
  if (bad != TREE_NONE) atomicMin(s_bad, bad);
  __syncthreads();
  // pointer jumping in the output row (relaxed, workgroup scope: a stale read is an ancestor too)
  for (uint32_t j = tid; j < n; j += T) {
    for (uint32_t it = 0; it < n; it++) {  // (bounded: a graph with a 0 ns arc could tie in a cycle)
      const uint32_t x = __hip_atomic_load(&fh[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const uint32_t y = __hip_atomic_load(&fh[a.pos[x]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (y == x) break;
      __hip_atomic_store(&fh[j], y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (*s_bad != TREE_NONE) atomicMin(a.bad, ((unsigned long long)(a.row_begin + r) << 32) | *s_bad);
    *s_bad = TREE_NONE;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(1024) k_tree_global(const TreeArgs a) {
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0) s_bad = TREE_NONE;
  __syncthreads();
  for (uint32_t r = blockIdx.x; r < a.rows; r += gridDim.x) tree_row_global(a, r, &s_bad);
}

// One workgroup per row, the row in LDS: key[n] u64, then pred[n] u16 and first_hop[n] u16, by
// node; during the tight test the 4n bytes of the two u16 arrays hold min[n] u32 instead.
__global__ void __launch_bounds__(1024) k_tree_lds(const TreeArgs a) {
  extern __shared__ __align__(16) unsigned char tree_smem[];
  __shared__ uint32_t s_bad, s_wide;
  const uint32_t tid = threadIdx.x, T = blockDim.x, n = a.n;
  uint64_t* key = (uint64_t*)tree_smem;
  uint32_t* min32 = (uint32_t*)(key + n);
  uint16_t* pred = (uint16_t*)(key + n);
  volatile uint16_t* hop = (volatile uint16_t*)(pred + n);
  if (tid == 0) {
    s_bad = TREE_NONE;
    s_wide = 0u;
  }
  __syncthreads();
  for (uint32_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
    const uint32_t s = a.nodes[a.row_begin + r];
    const uint64_t* __restrict__ lat = a.lat + (size_t)r * n;
    const float* __restrict__ loss = a.loss + (size_t)r * n;
    // stage the row by node; key[s] = default()
    bool wide = false;
    for (uint32_t j = tid; j < n; j += T) {
      const uint32_t v = a.nodes[j];
      const uint64_t l = lat[j];
      const uint32_t f = __float_as_uint(loss[j]);
      if (v == s) {
        key[v] = 0ull;
      } else {
        wide |= l >= (uint64_t)LAT32_SAT;
        key[v] = (l << 32) | (uint64_t)f;
      }
      min32[j] = TREE_NONE;
    }
    if (wide) s_wide = 1u;
    __syncthreads();
    if (s_wide) {  // a latency of 2^32 - 1 ns or more: u64 keys, the exact in_lat
      __syncthreads();
      if (tid == 0) s_wide = 0u;
      tree_row_global(a, r, &s_bad);
      continue;
    }
    // every saturating add below is exact or ends at LAT32_SAT, which no key of this row holds
    for_each_arc(a, [&](uint32_t, const uint4& rec) {
      if (rec.y != s && relax32(key[rec.x], rec.z, __uint_as_float(rec.w)) == key[rec.y])
        atomicMin(&min32[rec.y], rec.x);
    });
    __syncthreads();
    // min[n] u32 -> pred[n] u16 + first_hop[n] u16 in the same bytes, through registers
    uint32_t best[TREE_PER_THREAD];
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; k++) {
      const uint32_t v = tid + k * T;
      best[k] = v < n ? min32[v] : TREE_NONE;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; k++) {
      const uint32_t v = tid + k * T;
      if (v < n) {
        if (v == s) {
          pred[v] = (uint16_t)s;
          hop[v] = (uint16_t)s;
        } else {
          pred[v] = (uint16_t)best[k];  // (TREE_NONE -> TREE_NONE16: n is below 65,535)
          hop[v] = (uint16_t)(best[k] == s || best[k] == TREE_NONE ? v : best[k]);
        }
      }
    }
    __syncthreads();
    for (uint32_t v = tid; v < n; v += T) {
      for (uint32_t it = 0; it < n; it++) {  // (bounded, as on the global path)
        const uint32_t x = hop[v];
        const uint32_t y = hop[x];
        if (y == x) break;
        hop[v] = (uint16_t)y;
      }
    }
    __syncthreads();
    // both rows in the caller's column order, 16 bytes a store
    uint32_t* o_pred = a.pred + (size_t)r * n;
    uint32_t* o_fh = a.fh + (size_t)r * n;
    uint32_t bad = TREE_NONE;
    auto one = [&](uint32_t j, uint32_t v, uint32_t& p, uint32_t& h) {
      p = pred[v];
      h = hop[v];
      if (p == TREE_NONE16 && v != s) {
        p = TREE_NONE;
        bad = min(bad, j);
      }
    };
    if (a.vec) {
      for (uint32_t j = tid * 4; j < n; j += T * 4) {
        const uint4 nd = *(const uint4*)&a.nodes[j];
        u32x4 p, h;
        uint32_t pp, hh;
        one(j, nd.x, pp, hh);
        p.x = pp;
        h.x = hh;
        one(j + 1, nd.y, pp, hh);
        p.y = pp;
        h.y = hh;
        one(j + 2, nd.z, pp, hh);
        p.z = pp;
        h.z = hh;
        one(j + 3, nd.w, pp, hh);
        p.w = pp;
        h.w = hh;
        __builtin_nontemporal_store(p, (u32x4*)&o_pred[j]);
        __builtin_nontemporal_store(h, (u32x4*)&o_fh[j]);
      }
    } else {
      for (uint32_t j = tid; j < n; j += T) {
        uint32_t pp, hh;
        one(j, a.nodes[j], pp, hh);
        __builtin_nontemporal_store(pp, &o_pred[j]);
        __builtin_nontemporal_store(hh, &o_fh[j]);
      }
    }
    if (bad != TREE_NONE) atomicMin(&s_bad, bad);
    __syncthreads();  // (and the next row reuses the LDS)
    if (tid == 0) {
      if (s_bad != TREE_NONE) atomicMin(a.bad, ((unsigned long long)(a.row_begin + r) << 32) | s_bad);
      s_bad = TREE_NONE;
    }
    __syncthreads();
  }
}

// The most nodes the LDS path takes on this device: 12 bytes a node in what a workgroup may
// allocate, u16 node indices with 0xFFFF spare, and TREE_PER_THREAD nodes per thread.
static uint32_t tree_lds_max(const sg_ctx* ctx) {
  int lds = 0;
  SG_HIP(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  if ((size_t)lds <= TREE_STATIC_LDS) return 0;
  const size_t n = ((size_t)lds - TREE_STATIC_LDS) / TREE_NODE_BYTES;
  return (uint32_t)std::min<size_t>(std::min<size_t>(n, TREE_NONE16 - 1), (size_t)TREE_PER_THREAD * 1024);
}

// Rows [row_begin, row_end) of pred / first_hop from the same rows of the table, all on the
// device (d_* row-major from row_begin).  Synchronises once, on the flag word.
static void tree_rows(sg_ctx* ctx, sg_net* net, const uint32_t* h_nodes, uint32_t row_begin, uint32_t row_end,
                      const uint64_t* d_lat, const float* d_loss, uint32_t* d_pred, uint32_t* d_fh) {
  hipStream_t st = ctx->stream;
  const uint32_t n = net->n_nodes, rows = row_end - row_begin;
  ensure_csc(ctx, net);
  // nodes, then its inverse
  uint32_t* d_idx = ctx->t_idx.get<uint32_t>(2 * (size_t)n);
  {
    char* hu = stage_acquire(ctx, 1, 2 * (size_t)n * 4);
    uint32_t* hn = (uint32_t*)hu;
    memcpy(hn, h_nodes, (size_t)n * 4);
    for (uint32_t j = 0; j < n; j++) hn[n + h_nodes[j]] = j;
    SG_HIP(hipMemcpyAsync(d_idx, hu, 2 * (size_t)n * 4, hipMemcpyHostToDevice, st));
    stage_release(ctx, 1);
  }
  unsigned long long* bad = ctx->t_flag.get<unsigned long long>(2);
  SG_HIP(hipMemsetAsync(bad, 0xff, 8, st));
  TreeArgs a;
  a.in_rec = net->in_rec;
  a.in_lat = net->in_lat;
  a.n_arcs = net->n_arcs;
  a.nodes = d_idx;
  a.pos = d_idx + n;
  a.n = n;
  a.row_begin = row_begin;
  a.rows = rows;
  a.lat = d_lat;
  a.loss = d_loss;
  a.pred = d_pred;
  a.fh = d_fh;
  a.bad = bad;
  a.vec = n % 4 == 0 && ((uintptr_t)d_pred & 15) == 0 && ((uintptr_t)d_fh & 15) == 0;
  const uint32_t n_max = tree_lds_max(ctx);
  const bool lds = knob_int("SG_TREE_LDS", 1) != 0 && n <= n_max;
  // small graphs: 256 threads, so that a CU holds several rows
  const unsigned threads = n <= 2048 ? 256u : 1024u;
  // bytes moved: the rows read (12 B a cell), both outputs written (8 B a cell)
  const double bytes = 20.0 * (double)rows * (double)n;
  {
    TimedLaunch tl(ctx, "tree", bytes);
    if (lds) {
      const size_t dyn = (size_t)n * TREE_NODE_BYTES;
      SG_HIP(hipFuncSetAttribute((const void*)k_tree_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
      hipLaunchKernelGGL(k_tree_lds, dim3(rows), dim3(threads), dyn, st, a);
    } else {
      hipLaunchKernelGGL(k_tree_global, dim3(rows), dim3(threads), 0, st, a);
    }
    SG_CHECK_LAUNCH();
  }
  // read_timer("tree_lds") = (0, rows launched on the LDS path, the LDS path's node limit)
  timer_set_counter(ctx, "tree_lds", (double)n_max, lds ? rows : 0u);
  unsigned long long h = 0;
  copy_to_host(ctx, &h, bad, 8);
  if (h != ~0ull) {
    const uint32_t i = (uint32_t)(h >> 32), j = (uint32_t)h;
    throw Error(SG_ERR_INVALID_ARG,
                "no tight in-arc for the path from node " + node_name(net, h_nodes[i]) + " to node " +
                    node_name(net, h_nodes[j]) + ": the rows are not this graph's shortest-path table",
                i, j);
  }
}

// The checks sg_routing_tree and sg_routing_build_tree share; none touches an output.
static void tree_check_args(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes, uint32_t row_begin,
                            uint32_t row_end) {
  check_rows_call(ctx, net, nodes, n_nodes, row_begin, row_end, "a tree");
  check_node_list(net, nodes, n_nodes);  // in range and none twice: with n_nodes entries, a permutation
}

// tree_rows with outputs that may be missing (dev_out) or on the host
static void tree_outputs(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t row_begin, uint32_t row_end,
                         bool dev_out, const uint64_t* d_lat, const float* d_loss, uint32_t* out_pred,
                         uint32_t* out_first_hop) {
  const size_t count = (size_t)(row_end - row_begin) * net->n_nodes;
  // (the kernels write both rows: a missing one goes to the workspace)
  uint32_t* d_pred = dev_out && out_pred ? out_pred : ctx->t_pred.get<uint32_t>(count);
  uint32_t* d_fh = dev_out && out_first_hop ? out_first_hop : ctx->t_fh.get<uint32_t>(count);
  tree_rows(ctx, net, nodes, row_begin, row_end, d_lat, d_loss, d_pred, d_fh);
  if (!dev_out) {
    hipStream_t st = ctx->stream;
    if (out_pred) SG_HIP(hipMemcpyAsync(out_pred, d_pred, count * 4, hipMemcpyDeviceToHost, st));
    if (out_first_hop) SG_HIP(hipMemcpyAsync(out_first_hop, d_fh, count * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
  }
}

}  // namespace sg

extern "C" {

int32_t sg_routing_tree(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes, uint32_t row_begin,
                        uint32_t row_end, uint32_t flags, const uint64_t* latency_ns, const float* packet_loss,
                        uint32_t* out_pred, uint32_t* out_first_hop) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    tree_check_args(ctx, net, nodes, n_nodes, row_begin, row_end);
    if (!out_pred && !out_first_hop) throw Error(SG_ERR_INVALID_ARG, "null output");
    if (row_end == row_begin) return;
    if (!latency_ns || !packet_loss) throw Error(SG_ERR_INVALID_ARG, "null table rows");
    const bool dev = flags & SG_ROUTE_OUT_DEVICE;
    const size_t count = (size_t)(row_end - row_begin) * n_nodes;
    const uint64_t* d_lat = latency_ns;
    const float* d_loss = packet_loss;
    if (!dev) {
      uint64_t* wl = ctx->r_out_lat.get<uint64_t>(count);
      float* wf = ctx->r_out_loss.get<float>(count);
      SG_HIP(hipMemcpyAsync(wl, latency_ns, count * 8, hipMemcpyHostToDevice, ctx->stream));
      SG_HIP(hipMemcpyAsync(wf, packet_loss, count * 4, hipMemcpyHostToDevice, ctx->stream));
      d_lat = wl;
      d_loss = wf;
    }
    tree_outputs(ctx, net, nodes, row_begin, row_end, dev, d_lat, d_loss, out_pred, out_first_hop);
  });
}

int32_t sg_routing_build_tree(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes, uint32_t row_begin,
                              uint32_t row_end, uint32_t flags, uint64_t* out_latency_ns, float* out_packet_loss,
                              uint32_t* out_pred, uint32_t* out_first_hop) {
  int32_t rc = sg::guarded(ctx, [&] {
    using namespace sg;
    tree_check_args(ctx, net, nodes, n_nodes, row_begin, row_end);
    if (!(flags & SG_ROUTE_SHORTEST_PATH))
      throw Error(SG_ERR_INVALID_ARG, "direct paths have no tree: SG_ROUTE_SHORTEST_PATH is required");
    if (row_end > row_begin && (!out_latency_ns || !out_packet_loss || !out_pred || !out_first_hop))
      throw Error(SG_ERR_INVALID_ARG, "null output");
  });
  if (rc != SG_OK) return rc;
  // the build, with its errors in its precedence
  rc = sg_routing_build(ctx, net, nodes, n_nodes, row_begin, row_end, flags, out_latency_ns, out_packet_loss);
  if (rc != SG_OK || row_end == row_begin) return rc;
  return sg::guarded(ctx, [&] {
    using namespace sg;
    const bool dev = flags & SG_ROUTE_OUT_DEVICE;
    // with host outputs the rows are still in the build's device workspace
    const uint64_t* d_lat = dev ? out_latency_ns : (const uint64_t*)ctx->r_out_lat.p;
    const float* d_loss = dev ? out_packet_loss : (const float*)ctx->r_out_loss.p;
    tree_outputs(ctx, net, nodes, row_begin, row_end, dev, d_lat, d_loss, out_pred, out_first_hop);
  });
}

int32_t sg_tree_path(const uint32_t* pred_row, const uint32_t* nodes, uint32_t n_nodes, uint32_t src, uint32_t dst,
                     uint32_t* out_path, uint32_t cap, uint32_t* len) {
  if (!pred_row || !len || src >= n_nodes || dst >= n_nodes) return SG_ERR_INVALID_ARG;
  try {
    std::vector<uint32_t> pos;
    if (nodes) {
      pos.assign(n_nodes, 0xFFFFFFFFu);
      for (uint32_t j = 0; j < n_nodes; j++) {
        if (nodes[j] >= n_nodes || pos[nodes[j]] != 0xFFFFFFFFu) return SG_ERR_INVALID_ARG;
        pos[nodes[j]] = j;
      }
    }
    // dst back to src: every step must stay in range, and n_nodes nodes is the longest path
    uint32_t count = 1;
    for (uint32_t cur = dst; cur != src; count++) {
      if (count >= n_nodes) return SG_ERR_INVALID_ARG;
      const uint32_t nxt = pred_row[nodes ? pos[cur] : cur];
      if (nxt >= n_nodes || nxt == cur) return SG_ERR_INVALID_ARG;
      cur = nxt;
    }
    *len = count;
    if (count > cap) return SG_ERR_CAPACITY;
    if (!out_path) return SG_ERR_INVALID_ARG;
    uint32_t k = count;
    for (uint32_t cur = dst;; cur = pred_row[nodes ? pos[cur] : cur]) {
      out_path[--k] = cur;
      if (cur == src) break;
    }
    return SG_OK;
  } catch (const std::bad_alloc&) {
    return SG_ERR_OOM;
  }
}

}  // extern "C"
