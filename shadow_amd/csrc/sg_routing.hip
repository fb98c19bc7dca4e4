// sg_routing.hip -- routing-table build on MI355X: the search dispatch and the C ABI.
//
// Replaces NetworkGraph::compute_shortest_paths (graph/mod.rs:183-228) and
// NetworkGraph::get_direct_paths (graph/mod.rs:230-252).
//
// Shortest paths.  The reference runs petgraph's Dijkstra per used source
// over (latency u64, loss f32) with the LEFT fold default() + e1 + e2 + ...
// (graph/mod.rs:195-200, 322-331).  Because edge latency >= 1 ns
// (graph/mod.rs:105-107) and the f32 fold is monotone, that result equals the
// fixed point of the source-rooted relaxation
//     D[s][v] = min(D[s][v], D[s][u] (+) w(u,v))
// under ANY relaxation order, as long as every update keeps the edge on the
// right (source-rooted) and the (latency, loss) pair is updated atomically.
// Floyd-Warshall would re-associate the f32 fold and is not bit-exact for loss.
//
// Every search computes that fixed point; shortest_paths below picks one by the graph:
//  * sg_sssp.hip k_sssp_lds (sparse graphs up to ~10.9k nodes): one workgroup per
//    source, the source's whole distance row in LDS, an asynchronous work queue,
//    rows bounded (and partly seeded exactly) by neighbour rows finished in earlier
//    phases (sg_plan.hip); about 1.1-1.6x Dijkstra's relaxations at C3.
//  * sg_bucket.hip (sparse graphs past the LDS search): delta-stepping per source.
//  * sg_dense.hip (dense graphs up to DENSE_MAX nodes): a register-resident search.
//  * sg_slab.hip k_relax_w2 (everything else): batched-source pull relaxation.
// All use the packed key (latency u32 << 32) | f32 bits(loss) (sg_device.h), so
// one u64 min is the lexicographic PathProperties comparison.  Latency adds
// saturate at LAT32_SAT = 2^32 - 1 ns; rows holding a saturated key (a path of
// 4.29 s or more, or an unreachable node) are redone by the wide (u64 latency,
// f32 loss) Jacobi kernel k_relax_wide (sg_slab.hip).  The graph itself is built
// by sg_net.hip.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"

namespace sg {

// ---------------------------------------------------------------------------
// Self-loop census over the used nodes (graph/mod.rs:210-217): first failing
// node in order, low bit = "more than one".
// ---------------------------------------------------------------------------
__global__ void k_self_check(const uint32_t* __restrict__ used, uint32_t n_used,
                             const uint32_t* __restrict__ self_cnt,
                             unsigned long long* __restrict__ first) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_used; j += gridDim.x * blockDim.x) {
    uint32_t c = self_cnt[used[j]];
    if (c != 1) atomicMin(first, ((unsigned long long)j << 1) | (c > 1 ? 1ull : 0ull));
  }
}

// The LDS search's last launch of a build: how many rows it flagged for the wide
// kernel, and (when sg_routing_build asked for it) the self-loop check's first
// failure as k_self_check encodes it, both into the mapped return block -- the
// build's end is one synchronisation and no copies.  One workgroup, branch-free loads.
// count_flags 0: the self-loop check alone (on the side stream, beside phase 0: the LDS search
// kernels then tell the host themselves that a row was flagged, and no kernel ends the build).
__global__ void __launch_bounds__(1024) k_build_finish(const uint32_t* __restrict__ sat, uint32_t rows,
                                                       const uint32_t* __restrict__ used, uint32_t n_used,
                                                       const uint32_t* __restrict__ self_cnt, uint32_t* __restrict__ ret,
                                                       int count_flags) {
  constexpr int G = 8;
  __shared__ uint32_t s_cnt[16];
  __shared__ unsigned long long s_min[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr uint32_t OOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)sat, 0, (int)(rows * 4u), 0x00020000);
  uint32_t cnt = 0;
  for (uint32_t r0 = tid; r0 < rows; r0 += G * 1024) {
    uint32_t x[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const uint32_t r = r0 + g * 1024;
      x[g] = __builtin_amdgcn_raw_buffer_load_b32(rs, r < rows ? r * 4u : OOB, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < G; g++) cnt += x[g] != 0u;
  }
  unsigned long long first = ~0ull;
  if (self_cnt) {
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)used, 0, (int)(n_used * 4u), 0x00020000);
    for (uint32_t j0 = tid; j0 < n_used; j0 += G * 1024) {
      uint32_t v[G], c[G];
#pragma unroll
      for (int g = 0; g < G; g++) {
        const uint32_t j = j0 + g * 1024;
        v[g] = __builtin_amdgcn_raw_buffer_load_b32(ru, j < n_used ? j * 4u : OOB, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < G; g++) c[g] = j0 + g * 1024 < n_used ? self_cnt[v[g]] : 1u;
#pragma unroll
      for (int g = 0; g < G; g++)
        if (c[g] != 1u) first = min(first, ((unsigned long long)(j0 + g * 1024) << 1) | (c[g] > 1u ? 1ull : 0ull));
    }
  }
  cnt = wave_incl_sum(cnt);
  for (int d = 32; d > 0; d >>= 1) first = min(first, (unsigned long long)__shfl_xor(first, d));
  if (lane == 63) s_cnt[wv] = cnt;
  if (lane == 0) s_min[wv] = first;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
    unsigned long long m = ~0ull;
    for (int w = 0; w < 16; w++) {
      t += s_cnt[w];
      m = min(m, s_min[w]);
    }
    if (count_flags) ret[4] = t;
    ((unsigned long long*)ret)[1] = m;
  }
}

// ---------------------------------------------------------------------------
// Direct paths (graph/mod.rs:230-252): per used pair, count the edges that
// petgraph's edges_connecting would yield.
// ---------------------------------------------------------------------------
__global__ void k_pair_count(const uint32_t* __restrict__ src, const uint32_t* __restrict__ dst,
                             uint32_t m, int directed, const uint32_t* __restrict__ map,
                             uint32_t n_used, uint32_t row_begin, uint32_t row_end,
                             uint32_t* __restrict__ cnt, uint32_t* __restrict__ edge) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < m; e += gridDim.x * blockDim.x) {
    uint32_t iu = map[src[e]], iv = map[dst[e]];
    if (iu == ~0u || iv == ~0u) continue;
    if (iu >= row_begin && iu < row_end) {
      size_t o = (size_t)(iu - row_begin) * n_used + iv;
      atomicAdd(&cnt[o], 1u);
      edge[o] = e;
    }
    if (!directed && iu != iv && iv >= row_begin && iv < row_end) {
      size_t o = (size_t)(iv - row_begin) * n_used + iu;
      atomicAdd(&cnt[o], 1u);
      edge[o] = e;
    }
  }
}

__global__ void k_pair_out(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ edge,
                           size_t count, uint32_t n_used, uint32_t row_begin,
                           const uint64_t* __restrict__ e_lat, const float* __restrict__ e_loss,
                           uint64_t* __restrict__ out_lat, float* __restrict__ out_loss,
                           unsigned long long* __restrict__ first) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (size_t)gridDim.x * blockDim.x) {
    uint32_t c = cnt[i];
    if (c != 1) {
      unsigned long long lin = (unsigned long long)row_begin * n_used + i;
      atomicMin(first, (lin << 1) | (c > 1 ? 1ull : 0ull));
      out_lat[i] = 0;
      out_loss[i] = 0.0f;
    } else {
      out_lat[i] = e_lat[edge[i]];
      out_loss[i] = e_loss[edge[i]];
    }
  }
}

// Two-stage minimum: per-block partials (plain stores), then one block.
__global__ void __launch_bounds__(256) k_min_u64(const uint64_t* __restrict__ x, size_t count,
                                                 unsigned long long* __restrict__ part) {
  __shared__ unsigned long long wm[4];
  unsigned long long m = ~0ull;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    m = min(m, (unsigned long long)x[i]);
  for (int d = 32; d > 0; d >>= 1) m = min(m, (unsigned long long)__shfl_xor(m, d, 64));
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = min(min(wm[0], wm[1]), min(wm[2], wm[3]));
}

__global__ void __launch_bounds__(256) k_min_final(const unsigned long long* __restrict__ part, uint32_t n,
                                                   unsigned long long* __restrict__ out) {
  __shared__ unsigned long long wm[4];
  unsigned long long m = ~0ull;
  for (uint32_t i = threadIdx.x; i < n; i += 256) m = min(m, part[i]);
  for (int d = 32; d > 0; d >>= 1) m = min(m, (unsigned long long)__shfl_xor(m, d, 64));
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) *out = min(min(wm[0], wm[1]), min(wm[2], wm[3]));
}

// sg_routing_info_fill: a block of (latency u64, loss f32) cells -> the host
// RoutingInfo's 8-byte cells (latency u32 << 32 | bits(loss); SG_CELL_WIDE in the
// latency half when the path takes 2^32 - 1 ns or more), the block's smallest
// latency (ctl[0], atomicMin) and its count of wide cells (ctl[1]).
__global__ void __launch_bounds__(256) k_pack_cells(const uint64_t* __restrict__ lat, const float* __restrict__ loss,
                                                    size_t cells, uint64_t* __restrict__ out,
                                                    unsigned long long* __restrict__ ctl) {
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  unsigned long long m = ~0ull;
  uint32_t nw = 0;
  auto pack = [&](uint64_t l, float f) -> uint64_t {
    m = min(m, (unsigned long long)l);
    const uint32_t hi = l < SG_CELL_WIDE ? (uint32_t)l : SG_CELL_WIDE;
    nw += hi == SG_CELL_WIDE;
    return ((uint64_t)hi << 32) | __float_as_uint(f);
  };
  const size_t pairs = cells / 2, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride) {
    const u64x2 l = __builtin_nontemporal_load((const u64x2*)lat + i);
    const f32x2 f = __builtin_nontemporal_load((const f32x2*)loss + i);
    __builtin_nontemporal_store((u64x2){pack(l.x, f.x), pack(l.y, f.y)}, (u64x2*)out + i);
  }
  if ((cells & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[cells - 1] = pack(lat[cells - 1], loss[cells - 1]);
  for (int d = 32; d > 0; d >>= 1) {
    m = min(m, (unsigned long long)__shfl_xor(m, d, 64));
    nw += __shfl_xor(nw, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (m != ~0ull) atomicMin(&ctl[0], m);
    if (nw) atomicAdd(&ctl[1], (unsigned long long)nw);
  }
}

// sg_routing_info_fill: the wide cells of a block: (cell index + off, u64 latency) pairs, in
// any order.  (Not part of the wide fallback of sg_slab.hip: it lists what k_pack_cells marked.)
__global__ void k_wide_list(const uint64_t* __restrict__ lat, size_t cells, uint64_t off,
                            unsigned long long* __restrict__ ctr, uint64_t* __restrict__ list) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += stride)
    if (lat[i] >= SG_CELL_WIDE) {
      const unsigned long long k = atomicAdd(ctr, 1ull);
      list[2 * k] = off + i;
      list[2 * k + 1] = lat[i];
    }
}

// ---------------------------------------------------------------------------
// Host orchestration
// ---------------------------------------------------------------------------
// The self-loop check of every used node (graph/mod.rs:210-217) runs ahead of the
// search without a host round trip; its result is read once the build has
// synchronised (raise_self_loops), and an error found there wins over any the
// search raised, as in the reference, where the self-loops are checked before the
// n^2 assertion (:219).  The search reads self_edge only at count 1 (and it is
// zeroed elsewhere), so it stays in bounds on a graph the check rejects.
static unsigned long long* launch_self_loops(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used) {
  flush_used(ctx);
  unsigned long long* first = ctx->r_self.get<unsigned long long>(4);  // (its own word: the build uses r_err)
  SG_HIP(hipMemsetAsync(first, 0xff, 8, ctx->stream));
  hipLaunchKernelGGL(k_self_check, dim3(grid_for(n_used, 256, 4096)), dim3(256), 0, ctx->stream,
                     d_used, n_used, net->self_cnt, first);
  SG_CHECK_LAUNCH();
  return first;
}

static void raise_self_value(sg_net* net, unsigned long long h, const uint32_t* h_used) {
  if (h != ~0ull) {
    uint32_t j = (uint32_t)(h >> 1);
    std::string id = node_name(net, h_used[j]);
    if (h & 1)
      throw Error(SG_ERR_MULTI_EDGE, "More than one edge connecting node " + id + " to " + id, j, j);
    throw Error(SG_ERR_NO_EDGE, "No edge connecting node " + id + " to " + id, j, j);
  }
}

static void raise_self_loops(sg_ctx* ctx, sg_net* net, const unsigned long long* first, const uint32_t* h_used) {
  unsigned long long h = 0;
  copy_to_host(ctx, &h, first, 8);
  raise_self_value(net, h, h_used);
}

// sg_routing_build's check: the value the LDS search's final kernel read, else a launch of its own
static void raise_self_check(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used,
                             const uint32_t* h_used) {
  const bool done = ctx->self_done;
  const unsigned long long v = ctx->self_first;
  ctx->self_used = nullptr;
  ctx->self_cnt = nullptr;
  ctx->self_done = false;
  if (done) raise_self_value(net, v, h_used);
  else raise_self_loops(ctx, net, launch_self_loops(ctx, net, d_used, n_used), h_used);
}

// The relaxation counters' sum (WORK_SHARDS shards, then `extra` words the caller reads from w)
static double read_work(sg_ctx* ctx, const unsigned long long* work, unsigned long long* w, int extra = 0) {
  copy_to_host(ctx, w, work, (size_t)(WORK_SHARDS + extra) * 8);
  double total = 0;
  for (int k = 0; k < WORK_SHARDS; k++) total += (double)w[k];
  return total;
}

// The build's end: the flagged rows' count and the self-loop check in one kernel,
// one synchronisation; the flags themselves are copied only when some row was
// flagged.  Returns the rows (absolute) that need the wide kernel.  told: no kernel -- the
// searches set the flagged word themselves and the self-loop check ran on the side stream.
static std::vector<uint32_t> finish_rows(sg_ctx* ctx, const uint32_t* sat, uint32_t row_begin, uint32_t rows,
                                         bool told = false) {
  hipStream_t st = ctx->stream;
  if (!told) {
    hipLaunchKernelGGL(k_build_finish, dim3(1), dim3(1024), 0, st, sat, rows, ctx->self_used, ctx->self_n,
                       ctx->self_cnt, ctx->apsp_ret, 1);
    SG_CHECK_LAUNCH();
  }
  SG_HIP(hipStreamSynchronize(st));
  const volatile uint32_t* ret = ctx->apsp_ret;
  const uint32_t n_flag = ret[4];
  if (ctx->self_used) {
    ctx->self_first = *(const volatile unsigned long long*)(ret + 2);
    ctx->self_done = true;
  }
  std::vector<uint32_t> wide_rows;
  if (n_flag) {
    std::vector<uint32_t> h_sat(rows);
    copy_to_host(ctx, h_sat.data(), sat, rows * 4ull);
    for (uint32_t r = 0; r < rows; r++)
      if (h_sat[r]) wide_rows.push_back(row_begin + r);
  }
  return wide_rows;
}

// Dense graphs (sg_dense.hip): one register-resident search per row, no plan.
static void shortest_paths_dense(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used,
                                 uint32_t row_begin, uint32_t row_end, uint64_t* out_lat, float* out_loss) {
  const uint32_t rows = row_end - row_begin;
  // (no fill: the dense kernels write every row's flag, sg_dense.hip dense_write_row)
  uint32_t* sat = ctx->r_flags.get<uint32_t>(std::max(rows, 1u));
  unsigned long long* work = ctx->count_work ? ctx->r_work.get<unsigned long long>(WORK_SHARDS) : nullptr;
  if (work) SG_HIP(hipMemsetAsync(work, 0, WORK_SHARDS * 8, ctx->stream));
  launch_sssp_dense(ctx, net, d_used, n_used, row_begin, row_end, out_lat, out_loss, sat, work);
  std::vector<uint32_t> wide_rows = finish_rows(ctx, sat, row_begin, rows);
  if (work) {
    unsigned long long w[WORK_SHARDS];
    timer_add_work(ctx, "sssp_dense", read_work(ctx, work, w));
  }
  if (!wide_rows.empty()) run_wide(ctx, net, d_used, n_used, wide_rows, row_begin, out_lat, out_loss);
}

// SG_BUCKET_DIAG: the bucketed search's per-row statistics (d: its 16 diagnostic words) on stderr
static void print_bucket_diag(const sg_net* net, uint32_t rows, const unsigned long long* d, double total) {
  const double nb = std::max(1.0, (double)d[0]);
  fprintf(stderr, "[bucket] %u rows: %.1f buckets, %.0f entries, %.2f far steps, %.0f pops in %.0f claims, "
          "%.0f relaxations (%.3f x arcs) per row\n", rows, d[0] / (double)rows, d[1] / (double)rows,
          d[2] / (double)rows, d[3] / (double)rows, d[8] / (double)rows, total / rows,
          total / rows / std::max(1u, net->n_arcs));
  fprintf(stderr, "[bucket] cycles per bucket (thread 0): phase 0 %.0f, phase 1 %.0f, phase 2 %.0f; output per row %.0f\n",
          d[4] / nb, d[5] / nb, d[6] / nb, d[7] / (double)rows);
  fprintf(stderr, "[bucket] band kernel, wave 0 per bucket: offsets %.0f, arcs (with appends) %.0f, appends %.0f, store wait %.0f; "
          "band splits per row %.2f\n", d[9] / nb, d[10] / nb, d[11] / nb, d[12] / nb, d[15] / (double)rows);
  fprintf(stderr, "[bucket] band kernel, thread 0 per bucket in the load step: entry loads %.0f, hash %.0f, barrier wait %.0f\n",
          d[8] / nb, d[13] / nb, d[14] / nb);
  const double ncl = std::max(1.0, (double)d[8]);
  fprintf(stderr, "[bucket] per wave and bucket: load step %.0f cyc, idle %.0f; per claim: to offsets %.0f, to "
          "arcs %.0f (sum over arc rounds), appends %.0f, claim total %.0f\n", d[9] / nb / 4, d[14] / nb / 4,
          d[10] / ncl, d[11] / ncl, d[12] / ncl, d[13] / ncl);
}

// Sparse graphs past the LDS search (sg_bucket.hip): one delta-stepping search per row, the
// band of each bucket in LDS, later buckets in a per-workgroup arena; no plan.
static void shortest_paths_bucket(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used,
                                  uint32_t row_begin, uint32_t row_end, uint64_t* out_lat, float* out_loss) {
  const bool diag_on = knob_int("SG_BUCKET_DIAG", 0) != 0;
  const uint32_t rows = row_end - row_begin;
  uint32_t* sat = ctx->r_flags.get<uint32_t>(std::max(rows, 1u));
  SG_HIP(hipMemsetAsync(sat, 0, std::max(rows, 1u) * 4ull, ctx->stream));
  unsigned long long* work = ctx->count_work ? ctx->r_work.get<unsigned long long>(WORK_SHARDS + 16) : nullptr;
  unsigned long long* diag = work ? work + WORK_SHARDS : nullptr;
  if (work) SG_HIP(hipMemsetAsync(work, 0, (WORK_SHARDS + 16) * 8, ctx->stream));
  {
    TimedLaunch tl(ctx, "sssp_bucket", 0.0);
    launch_sssp_bucket(ctx, net, d_used, n_used, row_begin, row_end, out_lat, out_loss, sat, work, diag);
  }
  std::vector<uint32_t> wide_rows = finish_rows(ctx, sat, row_begin, rows);
  if (work) {
    unsigned long long w[WORK_SHARDS + 16];
    const double total = read_work(ctx, work, w, 16);
    timer_add_work(ctx, "sssp_bucket", total);
    timer_add_work(ctx, "sssp_bucket_entries", (double)w[WORK_SHARDS + 1]);  // entries through the arena
    if (diag_on) print_bucket_diag(net, rows, w + WORK_SHARDS, total);
  }
  if (!wide_rows.empty()) run_wide(ctx, net, d_used, n_used, wide_rows, row_begin, out_lat, out_loss);
}

// The LDS search's knobs, and with them the launch shape of a row block.
struct LdsKnobs {
  // Bucket width: SG_APSP_DELTA (ns), else one bucket (chaotic relaxation over the
  // asynchronous queue): at C3 it measured fastest (5.10 ms against 5.6 ms at 100 ms
  // buckets and 6.2 ms at 50 ms), for 2.5x Dijkstra's relaxations against 1.06x at
  // 50 ms -- the search is bound by its critical path, not by its relaxation count.
  uint32_t delta;
  bool diag;  // SG_SSSP_DIAG=1 (with counting timers): per-row cycle and phase statistics on stderr
  // Phases and bounds (sg_sssp.hip "Bounds", sg_plan.hip): phase 0 runs from infinity, a
  // row of phase p >= 1 starts from bounds (and exact seeds) taken from neighbour rows of
  // earlier phases.  The plan is built on the device for every build (sg_plan.hip), so a
  // one-shot build pays it.
  bool flagged;  // the plan's rows in one launch, in phase order
  bool phased;   // one launch per phase: a kernel boundary publishes the rows the next phase reads
  int n_phase, kb, hops;
  bool exact;
  uint32_t n_land;
  // SG_SSSP_CHAIN (sg_sssp.hip "Chained rows"): a persistent workgroup's next row is one with an
  // arc to the row it just finished, seeded from the keys still in its LDS.  Undirected graphs,
  // the phased launches and the launch without a plan; 0 keeps the list order and the set-up.
  bool chain;
  bool overlap;  // SG_BUILD_FUSED: the phased plan's bound rows run beside phase 0
};
static LdsKnobs lds_knobs(const sg_ctx* ctx, const sg_net* net, uint32_t n_used, uint32_t rows) {
  LdsKnobs k;
  k.delta = (uint32_t)std::min(4294967295.0, std::max(1.0, knob_double("SG_APSP_DELTA", 4294967295.0)));
  k.diag = knob_int("SG_SSSP_DIAG", 0) != 0;
  // Phases (sg_plan.hip) from 8 rows per CU: with fewer, the phase boundaries cost
  // more than the bounds save (tools/sssp_ab.py, C3 graph: 1,250 rows 0.78 against
  // 0.76 ms unbounded, a 2,000-node build 0.45 against 0.43; 2,500 rows 1.30
  // against 1.38, a 4,000-node build 0.97 against 1.07).  SG_SSSP_SEEDS=0 never, =2 always.
  const int seeds_env = knob_int("SG_SSSP_SEEDS", 1);
  // Flagged rows (sg_sssp.hip): the plan's rows in ONE launch, in phase order, each row
  // taking the bound rows already published when it starts -- no phase boundaries, so the
  // bounds pay even with few rows per CU.  The default for a row block (a rank's share of a
  // sharded build, or a RoutingInfo fill block); the whole table keeps the phased launches,
  // which it builds as fast (one box, tools/sssp_ab.py, C3 graph, tables bit-identical:
  // 10k rows 3.187 against 3.185 ms; row blocks of 5,000 1.93 against 1.99, 2,500 1.13
  // against 1.20, 1,250 0.685 against 0.706).  SG_SSSP_FLAGGED=0 / 1 forces it.
  // Below 6 rows per CU neither pays: the plan and the seeding cost more than the bounds save
  // (r7i-r7j, C3 graph, the hybrid lane path, tables identical: 640 rows 0.351 ms unbounded against
  // 0.398 flagged, 1,250 rows 0.558 against 0.581; 2,500 rows 1.044 against 0.948 flagged)
  const int flag_env = knob_int("SG_SSSP_FLAGGED", -1);
  const bool few_rows = rows < 6u * (uint32_t)std::max(1, ctx->n_cu);
  k.flagged = seeds_env != 0 && (flag_env == 1 || (flag_env < 0 && rows < n_used && !few_rows));
  k.phased = !k.flagged && seeds_env != 0 && (seeds_env == 2 || rows >= 8u * (uint32_t)ctx->n_cu);
  // phases by rows per CU (one box, tools/sssp_ab.py --rows, C3 graph): 39 rows per CU
  // (10k rows) 4 phases; 19.5 (a half) 3 phases, 2.25 against 2.57 ms unbounded;
  // 9.8 (a quarter) 2 phases, 1.30 against 1.38 ms
  // With chained rows two phases: a chain bounds most of phase 0's rows, so a smaller phase 0
  // saves less than the third launch costs (C3, one box, interleaved, tables identical:
  // 2.60-2.62 ms at 2 phases against 2.67-2.71 at 3 and 2.75-2.77 at 4; unchained 2.82-2.85 at 2 or 3)
  const bool chain = !knob_off("SG_SSSP_CHAIN") && !net->directed && !k.flagged;
  const uint32_t per_cu = rows / std::max(1, ctx->n_cu);
  k.n_phase = knob_int("SG_SSSP_PHASES", per_cu >= 16 && !chain ? 3 : 2, 2, SSSP_PHASES_MAX);
  k.kb = knob_int("SG_SSSP_BOUNDS", 2, 1, SSSP_KB_MAX);
  // exact seeds need a column for every node (see sg_sssp.hip "Exact seeds")
  k.exact = knob_int("SG_SSSP_EXACT", 1) != 0 && n_used == net->n_nodes;
  k.hops = knob_int("SG_SSSP_HOPS", 3, 1, 3);
  // Landmarks (sg_plan.hip header; undirected graphs, the phased plan only): SG_SSSP_LANDMARKS
  // rows first, the rest of phase 0 bounded through them.  Off by default: at C3
  // (tools/sssp_ab.py, one box, tables bit-identical) 256 landmarks cut phase 0 from 1.30 to
  // 0.36 ms but the landmark-bounded rows took 113 us each against 129 unbounded and 66 for
  // rows bounded by a neighbour: the build took 3.53 ms against 3.43 (128: 3.54, 512: 3.67).
  const int land_env = knob_int("SG_SSSP_LANDMARKS", 0);
  k.n_land = net->directed || land_env <= 0 ? 0u : (uint32_t)land_env;
  k.chain = chain;
  k.overlap = build_fused();
  return k;
}

// SG_SSSP_DIAG: the LDS search's per-row statistics (SSSP_DIAG_WORDS per row) on stderr
static void print_sssp_diag(sg_ctx* ctx, const sg_net* net, const unsigned long long* diag, uint32_t n_diag,
                            uint32_t delta) {
  constexpr int DW = SSSP_DIAG_WORDS;
  std::vector<unsigned long long> h((size_t)n_diag * DW);
  copy_to_host(ctx, h.data(), diag, h.size() * 8);
  double a[DW] = {};
  double setup = 0;
  // chained against unchained rows (word 3, bit 22): rows, setup cycles, search cycles (set-up included)
  double cn[2] = {0, 0}, cs[2] = {0, 0}, cq[2] = {0, 0};
  // how the search begins (words 13-15, sg_sssp.hip E_T0), per chained row with bound-row stamps: early
  // rows (index 1) against the others: rows, cycles to the first and the fourth claim (rows with four),
  // waves that held a claim in the first 16k cycles, cycles to the end of the last merge, merges onto dirty keys
  double en[2] = {0, 0}, e1[2] = {0, 0}, e4[2] = {0, 0}, e4n[2] = {0, 0}, ew[2] = {0, 0}, em = 0, ed = 0;
  double parts_n = 0;  // rows whose words 11 and 12 hold load-round parts
  for (uint32_t r = 0; r < n_diag; r++) {
    for (int k = 0; k < 13; k++) a[k] += (double)h[(size_t)r * DW + k];
    const unsigned long long w3 = h[(size_t)r * DW + 3];
    if (h[(size_t)r * DW] != 0 && ((w3 >> 22) & 1)) {
      const unsigned long long w13 = h[(size_t)r * DW + 13], w14 = h[(size_t)r * DW + 14], w15 = h[(size_t)r * DW + 15];
      const int e = (int)((w15 >> 32) & 1);
      en[e] += 1;
      e1[e] += (double)(uint32_t)w14;
      if ((uint32_t)w13) {
        e4[e] += (double)(uint32_t)w13;
        e4n[e] += 1;
      }
      ew[e] += (double)(w13 >> 32);
      if (e) {
        em += (double)(w14 >> 32);
        ed += (double)(uint32_t)w15;
      }
    }
    if (!((h[(size_t)r * DW + 15] >> 32) & 1)) parts_n += 1;
    setup += (double)(w3 >> 24);
    a[3] -= (double)(w3 >> 22 << 22);
    if (h[(size_t)r * DW] == 0) continue;  // a row of the list past this launch's phase
    const int c = (int)((w3 >> 22) & 1);
    cn[c] += 1;
    cs[c] += (double)(w3 >> 24);
    cq[c] += (double)h[(size_t)r * DW];
  }
  for (int c = 0; c < 2; c++)
    fprintf(stderr, "[sssp] %s rows: %.0f, mean setup %.0f cyc, mean search %.0f cyc\n", c ? "chained" : "unchained",
            cn[c], cs[c] / std::max(1.0, cn[c]), cq[c] / std::max(1.0, cn[c]));
  fprintf(stderr, "[sssp] mean setup (init + bound rows) %.0f cyc of the search\n", setup / n_diag);
  // the set-up's parts, thread 0's stamps (words 8-12)
  // (the load-round parts over the rows that have them: an early row's loads run under its search)
  fprintf(stderr, "[sssp] setup parts: bound-row listing and load issue %.0f, LDS pass %.0f, barrier %.0f, first load "
          "round %.0f, later rounds and closing barrier %.0f cyc (%.0f rows)\n", a[9] / n_diag, a[8] / n_diag,
          a[10] / n_diag, a[11] / std::max(1.0, parts_n), a[12] / std::max(1.0, parts_n), parts_n);
  for (int e = 0; e < 2; e++)
    fprintf(stderr, "[sssp] chained rows %s: %.0f, from the search's start: first claim %.0f cyc, fourth claim %.0f cyc "
            "(%.0f rows), %.2f waves with a claim in the first 16k cyc\n", e ? "started under their loads" : "set up first",
            en[e], e1[e] / std::max(1.0, en[e]), e4[e] / std::max(1.0, e4n[e]), e4n[e], ew[e] / std::max(1.0, en[e]));
  fprintf(stderr, "[sssp] rows started under their loads: last wave merged %.0f cyc after the search's start, %.2f merges "
          "onto dirty keys per row\n", em / std::max(1.0, en[1]), ed / std::max(1.0, en[1]));
  fprintf(stderr, "[sssp] per-wave cycles summed over a row's 16 waves: claim+wait %.0f, pop %.0f, steps %.0f "
          "(per pop: %.0f, %.0f)\n", a[5] / n_diag, a[6] / n_diag, a[7] / n_diag, a[6] / std::max(1.0, a[2]),
          a[7] / std::max(1.0, a[2]));
  fprintf(stderr, "[sssp] delta %u ns, %u rows: mean search %.0f cyc, output %.0f cyc, %.1f wave pops, %.1f buckets, "
          "%.0f relaxations (%.2f x arcs)\n", delta, n_diag, a[0] / n_diag, a[1] / n_diag, a[2] / n_diag,
          a[3] / n_diag, a[4] / n_diag, a[4] / n_diag / std::max(1u, net->n_arcs));
}

// Per-source LDS-resident search (sg_sssp.hip) for sparse graphs that fit a CU's LDS.
static void shortest_paths_lds(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, uint32_t row_begin,
                               uint32_t row_end, uint64_t* out_lat, float* out_loss) {
  hipStream_t st = ctx->stream;
  const uint32_t rows = row_end - row_begin;
  const LdsKnobs k = lds_knobs(ctx, net, n_used, rows);
  // (the searches set it to 1 when they flag a row; no launch of an earlier build is in flight)
  *(volatile uint32_t*)(ctx->apsp_ret + 4) = 0u;
  bool told = false;  // the build needs no final kernel (the phased plan with its side stream)
  // However the build ends, nothing stays pending on the side stream: the build's last
  // synchronisation covers it once the context stream waits for the bound rows (side_busy is
  // cleared there); an error thrown before that leaves through this.
  struct SideDrain {
    sg_ctx* c;
    ~SideDrain() {
      if (c->side_busy) (void)hipStreamSynchronize(c->side_stream);
      c->side_busy = false;
    }
  } side_drain{ctx};
  // the row flags, then the chained rows' claim words: zeroed by the plan's first kernel, else here
  uint32_t* sat = ctx->r_flags.get<uint32_t>(2 * (size_t)rows);
  uint32_t* claim = k.chain ? sat + rows : nullptr;
  // the relaxation counters, then the chained rows' two: rows seeded in place, those with exact seeds
  // ... then the ring invariant's two: ring slots a row's end found non-empty, rows looked at
  // ... then, with SG_SSSP_DIAG, the pops by class (SSSP_POP_WORDS)
  // ... then the early rows' two: rows that started under their bound rows' loads, merges onto dirty keys
  constexpr int WORK_WORDS = WORK_SSSP_EARLY + 2;
  unsigned long long* work = ctx->count_work ? ctx->r_work.get<unsigned long long>(WORK_WORDS) : nullptr;
  if (work) SG_HIP(hipMemsetAsync(work, 0, WORK_WORDS * 8, st));
  // counting mode with SG_SSSP_DIAG: the pops of the launch just issued, by class (the counters run on)
  unsigned long long pops_seen[SSSP_POP_WORDS] = {};
  auto diag_pops = [&](const char* what, int ph) {
    if (!work || !k.diag) return;
    unsigned long long c[SSSP_POP_WORDS];
    copy_to_host(ctx, c, work + WORK_SHARDS + 4, sizeof(c));
    static const char* const cls[SSSP_POP_CLASSES] = {"0", "1", "2", "3-4", "5-8", ">8"};
    for (int i = 0; i < SSSP_POP_CLASSES; i++) {
      const unsigned long long p = c[3 * i] - pops_seen[3 * i], a = c[3 * i + 1] - pops_seen[3 * i + 1],
                               cy = c[3 * i + 2] - pops_seen[3 * i + 2];
      fprintf(stderr, "[sssp] %s %d pops of S %s: %llu pops, %llu arcs, %llu step cycles (%.0f per pop)\n", what, ph,
              cls[i], p, a, cy, (double)cy / (double)std::max(1ull, p));
    }
    for (int i = 0; i < SSSP_POP_WORDS; i++) pops_seen[i] = c[i];
  };
  unsigned long long chained_seen[2] = {0, 0};
  unsigned long long phase_chained[SSSP_PHASES_MAX] = {};
  // counting mode: the rows this launch chained (kept per phase; SG_SSSP_DIAG prints them)
  auto diag_chained = [&](const char* what, int ph) {
    if (!work) return;
    unsigned long long c[2];
    copy_to_host(ctx, c, work + WORK_SHARDS, 16);
    phase_chained[ph] = c[0] - chained_seen[0];
    if (k.diag)
      fprintf(stderr, "[sssp] %s %d: %llu chained rows, %llu with exact seeds\n", what, ph, c[0] - chained_seen[0],
              c[1] - chained_seen[1]);
    chained_seen[0] = c[0];
    chained_seen[1] = c[1];
  };
  // counting mode: read_timer("sssp_phase<p>") = (0, rows of the plan's phase p, rows chained in its launch)
  auto publish_phases = [&](const SsspDevPlan& plan) {
    if (!work) return;
    uint32_t h[2 * SSSP_PHASES_MAX];
    copy_to_host(ctx, h, plan.ctl, sizeof(h));
    for (int p = 0; p < SSSP_PHASES_MAX; p++) {
      char name[24];
      snprintf(name, sizeof(name), "sssp_phase%d", p);
      const bool on = p < plan.n_phase;  // (ctl past the plan's phases is not written)
      timer_set_counter(ctx, name, on ? (double)phase_chained[p] : 0.0, on ? h[2 * p + 1] : 0u);
    }
  };
  const uint32_t n_diag = std::min<uint32_t>(rows, 4096);
  unsigned long long* diag =
      work && k.diag ? ctx->r_misc.get<unsigned long long>((size_t)n_diag * SSSP_DIAG_WORDS) : nullptr;
  if (diag) SG_HIP(hipMemsetAsync(diag, 0, (size_t)n_diag * SSSP_DIAG_WORDS * 8, st));
  SsspLdsLaunch base;
  base.d_used = d_used;
  base.n_used = n_used;
  base.ident = ctx->used_ident;
  base.row_begin = row_begin;
  base.row_end = row_end;
  base.out_lat = out_lat;
  base.out_loss = out_loss;
  base.sat_row = sat;
  base.delta = k.delta;
  base.work = work;
  base.diag = diag;
  base.pops = work && k.diag ? work + WORK_SHARDS + 4 : nullptr;
  if (k.flagged) {
    uint32_t* done = ctx->r_done.get<uint32_t>(std::max(rows, 1u));
    const SsspDevPlan plan = sssp_device_plan(ctx, net, d_used, n_used, row_begin, row_end, k.n_phase, k.kb, k.exact,
                                              k.hops, 0u, sat, done);
    SsspLdsLaunch l = base;
    l.blk_rows = plan.list;
    l.n_blk = rows;
    l.ub_row = plan.ub_row;
    l.ub_w = plan.ub_w;
    l.plan_ctr = plan.ctr;
    l.done = done;
    {
      TimedLaunch tl(ctx, "sssp", 0.0);
      launch_sssp_lds(ctx, net, l);
    }
    diag_pops("launch", 0);
    publish_phases(plan);  // (the one launch chains no rows)
  } else if (k.phased) {
    // the plan's bound rows beside phase 0 (sssp_plan_bounds_side) -- not with timers on, where
    // read_timer("plan_bounds") times them on this stream, and not with landmarks
    const bool overlap = k.overlap && !ctx->timing && !k.n_land;
    const SsspDevPlan plan =
        sssp_device_plan(ctx, net, d_used, n_used, row_begin, row_end, k.n_phase, k.kb, k.exact, k.hops, k.n_land, sat,
                         claim, claim != nullptr, knob_int("SG_SSSP_EXACT", 1) != 0, overlap);
    for (int ph = 0; ph < plan.n_phase; ph++) {
      const bool bounded = ph > 0;
      SsspLdsLaunch l = base;
      l.diag = ph + 1 == plan.n_phase ? diag : nullptr;
      l.blk_rows = plan.list;
      l.n_blk = rows;  // (an upper bound: the phase's size is in plan_ctl, known to the device only)
      l.ub_row = bounded ? plan.ub_row : nullptr;
      l.ub_w = bounded ? plan.ub_w : nullptr;
      l.plan_ctl = plan.ctl;
      l.plan_ph = ph;
      l.plan_ctr = plan.ctr + 2 * ph;
      l.chain = plan.chain;
      {
        TimedLaunch tl(ctx, bounded ? "sssp_bounded" : "sssp", 0.0);
        launch_sssp_lds(ctx, net, l);
      }
      diag_chained("phase", ph);
      diag_pops("phase", ph);
      if (ph == 0 && plan.bounds_deferred) {
        sssp_plan_bounds_side(ctx, net, plan, d_used, row_begin, row_end, k.kb, k.exact, k.hops);
        // the build's self-loop check rides along; the bounded phases wait for both
        if (ctx->self_used) {
          hipLaunchKernelGGL(k_build_finish, dim3(1), dim3(1024), 0, ctx->side_stream, sat, 0u, ctx->self_used,
                             ctx->self_n, ctx->self_cnt, ctx->apsp_ret, 0);
          SG_CHECK_LAUNCH();
        }
        told = true;
        SG_HIP(hipEventRecord(ctx->plan_bounds, ctx->side_stream));
        SG_HIP(hipStreamWaitEvent(st, ctx->plan_bounds, 0));
      }
      if (ph == 0 && plan.landmarks) sssp_landmark_bounds(ctx, plan, n_used, row_begin, out_lat, sat, k.kb);
    }
    publish_phases(plan);
  } else {
    // without a plan: the row flags and the persistent workgroups' claim counters zeroed by one
    // launch (two fills cost two dispatches and ~10 us of host time in a one-shot block build)
    SsspLdsLaunch l = base;
    l.plan_ctr = ctx->r_items.get<uint32_t>(2);
    // (chained rows need persistent workgroups, as launch_sssp_lds decides them)
    if (claim && rows > (uint32_t)ctx->n_cu && !knob_off("SG_SSSP_PERSIST")) {
      l.chain = sssp_plain_rel(ctx, net, d_used, row_begin, row_end, sat, claim, l.plan_ctr,
                               knob_int("SG_SSSP_EXACT", 1) != 0);
    } else {
      flush_used(ctx);  // (k_plan_rel writes a pending identity list, here as in a plan; nothing else does)
      launch_zero2(ctx, sat, rows, l.plan_ctr, 2u);
    }
    {
      TimedLaunch tl(ctx, "sssp", 0.0);
      launch_sssp_lds(ctx, net, l);
    }
    diag_chained("launch", 0);
    diag_pops("launch", 0);
  }
  if (diag) print_sssp_diag(ctx, net, diag, n_diag, k.delta);
  std::vector<uint32_t> wide_rows = finish_rows(ctx, sat, row_begin, rows, told);
  ctx->side_busy = false;  // (the context stream waited for the side stream and was synchronised)
  if (work) {
    unsigned long long w[WORK_WORDS];
    timer_add_work(ctx, "sssp", read_work(ctx, work, w, WORK_WORDS - WORK_SHARDS));
    // with SG_SSSP_DIAG, read_timer("sssp_pop_s<class>") = (0, pops, arcs) and ("sssp_pop_s<class>_cyc") =
    // (0, pops, step cycles) of this build's pops of S = ceil(arcs / 64) slots per lane, the classes named
    // by their largest S (0, 1, 2, 4, 8, and "gt8"); ("sssp_pops") = (0, pops counted by the waves, those of
    // them that took the lane path)
    if (k.diag) {
      static const char* const cls[SSSP_POP_CLASSES] = {"0", "1", "2", "4", "8", "gt8"};
      const unsigned long long* pc = w + WORK_SHARDS + 4;
      for (int i = 0; i < SSSP_POP_CLASSES; i++) {
        char name[32];
        snprintf(name, sizeof(name), "sssp_pop_s%s", cls[i]);
        timer_set_counter(ctx, name, (double)pc[3 * i + 1], pc[3 * i]);
        snprintf(name, sizeof(name), "sssp_pop_s%s_cyc", cls[i]);
        timer_set_counter(ctx, name, (double)pc[3 * i + 2], pc[3 * i]);
      }
      timer_set_counter(ctx, "sssp_pops", (double)pc[3 * SSSP_POP_CLASSES], pc[SSSP_POP_WORDS - 1]);
    }
    // read_timer("sssp_chained"): (0, rows with exact chain seeds, chained rows) of this build
    timer_set_counter(ctx, "sssp_chained", (double)w[WORK_SHARDS], w[WORK_SHARDS + 1]);
    // read_timer("sssp_ring_left"): (0, rows whose ring was looked at, slots found non-empty: 0 by the invariant)
    timer_set_counter(ctx, "sssp_ring_left", (double)w[WORK_SHARDS + 2], w[WORK_SHARDS + 3]);
    // read_timer("sssp_early"): (0, rows whose search started under their bound rows' loads, merges of
    // theirs that landed on a dirty key) -- sg_sssp.hip "Late seeds"
    timer_set_counter(ctx, "sssp_early", (double)w[WORK_SSSP_EARLY + 1], w[WORK_SSSP_EARLY]);
    if (k.diag)
      fprintf(stderr, "[sssp] ring slots not empty at a row's end: %llu (%llu rows)\n", w[WORK_SHARDS + 2],
              w[WORK_SHARDS + 3]);
  }
  if (!wide_rows.empty()) run_wide(ctx, net, d_used, n_used, wide_rows, row_begin, out_lat, out_loss);
}

// Which search takes the graph.
static void shortest_paths(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, const uint32_t* h_used,
                           uint32_t n_used, uint32_t row_begin, uint32_t row_end, uint64_t* out_lat,
                           float* out_loss) {
  // (Round 3 also built a team search for graphs past one CU's LDS, K workgroups per
  // row: 1.5x Dijkstra's relaxations at C5 but 646 ms against the slab's 249 ms, so
  // it was removed in round 4; DESIGN.md, "Team search".)
  // SG_APSP_LDS=0 forces the batched-source slab kernel.  The LDS search takes
  // sparse graphs (mean out-degree <= 64); on dense ones the slab kernel shares
  // each arc record among 64 sources (C2, 1,200-node complete graph: 3.6 ms
  // against 6.8-9.2 ms for the LDS search).
  const bool per_source = knob_int("SG_APSP_LDS", 1) != 0;
  // SG_APSP_DENSE=0: dense graphs take the slab kernel too
  const bool dense_on = knob_int("SG_APSP_DENSE", 1) != 0;
  // SG_APSP_BUCKET: 1 forces the bucketed search on any sparse graph (tests), 0 keeps the slab
  // kernel past the LDS search
  const int bucket_env = knob_int("SG_APSP_BUCKET", -1);
  const bool sparse = net->n_nodes && net->n_arcs <= 64ull * net->n_nodes;
  const bool arcs_ok = (uint64_t)net->n_arcs * 12 < (1ull << 31);
  // Dense graphs up to DENSE_MAX nodes (C2): the register-resident search of sg_dense.hip,
  // Dijkstra's n^2 relaxations per row
  const bool dense = per_source && dense_on && !sparse && sssp_dense_fits(net->n_nodes);
  const bool bucket = !dense && per_source && sparse && arcs_ok && bucket_env != 0 && sssp_bucket_fits(net->n_nodes) &&
                      (bucket_env == 1 || !sssp_lds_fits(net->n_nodes));
  const bool lds = !dense && !bucket && per_source && sparse && sssp_lds_fits(net->n_nodes) && arcs_ok;
  if (!lds) flush_used(ctx);  // (the LDS search's plan writes a pending identity list itself)
  if (dense)
    shortest_paths_dense(ctx, net, d_used, n_used, row_begin, row_end, out_lat, out_loss);
  else if (bucket)
    shortest_paths_bucket(ctx, net, d_used, n_used, row_begin, row_end, out_lat, out_loss);
  else if (lds)
    shortest_paths_lds(ctx, net, d_used, n_used, row_begin, row_end, out_lat, out_loss);
  else
    shortest_paths_slab(ctx, net, d_used, n_used, row_begin, row_end, out_lat, out_loss);
}


static void direct_paths(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, const uint32_t* h_used,
                         uint32_t n_used, uint32_t row_begin, uint32_t row_end, uint64_t* out_lat,
                         float* out_loss) {
  hipStream_t st = ctx->stream;
  flush_used(ctx);
  const uint32_t n = net->n_nodes;
  std::vector<uint32_t> map(n, ~0u);
  for (uint32_t j = 0; j < n_used; j++) map[h_used[j]] = j;
  uint32_t* d_map = ctx->r_map.get<uint32_t>(n);
  SG_HIP(hipMemcpyAsync(d_map, map.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  size_t count = (size_t)(row_end - row_begin) * n_used;
  uint32_t* cnt = ctx->r_pair_cnt.get<uint32_t>(count);
  uint32_t* edge = ctx->r_pair_edge.get<uint32_t>(count);
  SG_HIP(hipMemsetAsync(cnt, 0, count * 4, st));
  if (net->n_edges)
    hipLaunchKernelGGL(k_pair_count, dim3(grid_for(net->n_edges, 256, 8192)), dim3(256), 0, st,
                       net->e_src, net->e_dst, net->n_edges, (int)net->directed, d_map, n_used,
                       row_begin, row_end, cnt, edge);
  unsigned long long* first = ctx->r_err.get<unsigned long long>(4);
  SG_HIP(hipMemsetAsync(first, 0xff, 8, st));
  hipLaunchKernelGGL(k_pair_out, dim3(grid_for(count, 256, 65536)), dim3(256), 0, st, cnt, edge,
                     count, n_used, row_begin, net->e_lat, net->e_loss, out_lat, out_loss, first);
  SG_CHECK_LAUNCH();
  unsigned long long h = 0;
  copy_to_host(ctx, &h, first, 8);
  if (h != ~0ull) {
    unsigned long long lin = h >> 1;
    uint32_t i = (uint32_t)(lin / n_used), j = (uint32_t)(lin % n_used);
    std::string a = node_name(net, h_used[i]), b = node_name(net, h_used[j]);
    if (h & 1) throw Error(SG_ERR_MULTI_EDGE, "More than one edge connecting node " + a + " to " + b, i, j);
    throw Error(SG_ERR_NO_EDGE, "No edge connecting node " + a + " to " + b, i, j);
  }
}

}  // namespace sg

namespace sg {
// The used-node list: every index in range, none twice.  One branch-free pass; only a bad
// list is walked again, entry by entry, for the first bad entry's error.
bool check_node_list(const sg_net* net, const uint32_t* nodes, uint32_t n_used) {
  const uint32_t n = net->n_nodes;
  std::vector<uint8_t> seen((size_t)n + 1, 0);  // the spare last byte takes out-of-range ids
  uint32_t bad = 0, moved = 0;
  for (uint32_t j = 0; j < n_used; j++) {
    const uint32_t v = nodes[j];
    const uint32_t out = v >= n;
    const uint32_t x = out ? n : v;
    bad |= out | (uint32_t)seen[x];
    moved |= v ^ j;
    seen[x] = 1;
  }
  if (!bad) return !moved;
  std::fill(seen.begin(), seen.end(), (uint8_t)0);
  for (uint32_t j = 0; j < n_used; j++) {
    if (nodes[j] >= n) throw Error(SG_ERR_INVALID_ARG, "node index out of range");
    if (seen[nodes[j]]++) throw Error(SG_ERR_INVALID_ARG, "duplicate node in node list");
  }
  return false;
}

// used[j] = j: the identity used list written on the device (sg_ctx::used_fill) where no plan
// kernel does it; one launch in place of a 40-KB copy at C3 and of the wait that follows a copy.
__global__ void k_used_identity(uint32_t* __restrict__ used, uint32_t n_used) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_used; j += gridDim.x * blockDim.x) used[j] = j;
}

void flush_used(sg_ctx* ctx) {
  uint32_t* used = ctx->used_fill;
  if (!used) return;
  ctx->used_fill = nullptr;
  hipLaunchKernelGGL(k_used_identity, dim3(grid_for(ctx->used_fill_n, 256, 1024)), dim3(256), 0, ctx->stream, used,
                     ctx->used_fill_n);
  SG_CHECK_LAUNCH();
}
}  // namespace sg

extern "C" {

int32_t sg_routing_build(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_used,
                         uint32_t row_begin, uint32_t row_end, uint32_t flags,
                         uint64_t* out_latency_ns, float* out_packet_loss) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (!net || net->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "network belongs to another context");
    if (row_begin > row_end || row_end > n_used) throw Error(SG_ERR_INVALID_ARG, "bad row range");
    if (n_used && !nodes) throw Error(SG_ERR_INVALID_ARG, "null node list");
    if (row_end > row_begin && (!out_latency_ns || !out_packet_loss))
      throw Error(SG_ERR_INVALID_ARG, "null output");
    const bool identity = check_node_list(net, nodes, n_used);
    if (n_used == 0) return;
    hipStream_t st = ctx->stream;
    uint32_t* d_used = ctx->r_used.get<uint32_t>(n_used);
    struct NoFill {  // however the build ends, no later call finds this list's fill pending
      sg_ctx* c;
      ~NoFill() {
        c->used_fill = nullptr;
        c->used_ident = false;
      }
    } no_fill{ctx};
    ctx->used_ident = identity;
    if (identity && build_fused()) {
      // every node used, in order (C3, C5, C2; Shadow whenever every graph node has a host): the
      // list is written by the first kernel that reads it (the plan's k_plan_rel, else flush_used)
      ctx->used_fill = d_used;
      ctx->used_fill_n = n_used;
    } else {
      char* hu = stage_acquire(ctx, 1, (size_t)n_used * 4);
      memcpy(hu, nodes, (size_t)n_used * 4);
      SG_HIP(hipMemcpyAsync(d_used, hu, (size_t)n_used * 4, hipMemcpyHostToDevice, st));
      stage_release(ctx, 1);
    }
    const bool shortest = flags & SG_ROUTE_SHORTEST_PATH;
    // The reference checks every used node's self-loop (graph/mod.rs:211-217),
    // whichever rows this call computes.
    if (row_end == row_begin) {
      if (shortest) raise_self_loops(ctx, net, launch_self_loops(ctx, net, d_used, n_used), nodes);
      return;
    }
    const size_t count = (size_t)(row_end - row_begin) * n_used;
    const bool dev_out = flags & SG_ROUTE_OUT_DEVICE;
    uint64_t* o_lat = dev_out ? out_latency_ns : ctx->r_out_lat.get<uint64_t>(count);
    float* o_loss = dev_out ? out_packet_loss : ctx->r_out_loss.get<float>(count);
    if (shortest) {
      // the check of every used node's self-loop (graph/mod.rs:210-217) rides on the LDS
      // search's final kernel (k_build_finish); the other kernels leave it to a launch of its own
      ctx->self_used = d_used;
      ctx->self_n = n_used;
      ctx->self_cnt = net->self_cnt;
      ctx->self_done = false;
      struct Clear {  // however the build ends, no later kernel reads this net's arrays for the check
        sg_ctx* c;
        ~Clear() {
          c->self_used = nullptr;
          c->self_cnt = nullptr;
          c->self_done = false;
        }
      } clear{ctx};
      try {
        shortest_paths(ctx, net, d_used, nodes, n_used, row_begin, row_end, o_lat, o_loss);
      } catch (const Error&) {
        ctx->self_done = false;  // (the search may have failed before its final kernel)
        raise_self_check(ctx, net, d_used, n_used, nodes);  // a self-loop error first (graph/mod.rs:210-219)
        throw;
      }
      raise_self_check(ctx, net, d_used, n_used, nodes);
    } else
      direct_paths(ctx, net, d_used, nodes, n_used, row_begin, row_end, o_lat, o_loss);
    if (!dev_out) {
      SG_HIP(hipMemcpyAsync(out_latency_ns, o_lat, count * 8, hipMemcpyDeviceToHost, st));
      SG_HIP(hipMemcpyAsync(out_packet_loss, o_loss, count * 4, hipMemcpyDeviceToHost, st));
    }
    SG_HIP(hipStreamSynchronize(st));
  });
}

}  // extern "C"

namespace sg {
// Rows [r0, r1) of the table into a host RoutingInfo's cells (sg_route_info.hip), on one
// context: row blocks are built into one of two device staging buffers, packed into 8-byte
// cells and copied to the object's pinned host array on a second stream while the next block
// builds.  The copy (8 bytes per cell over PCIe) is what binds.  The rows' smallest latency
// and their wide cells (unsorted) go to `out`, not into the object: sg_routing_info_fill runs
// this over [0, n), sg_group_routing_info_fill (sg_group.hip) over one row range per member,
// each on a thread of its own, and merges.  block_rows: the block size where
// SG_RI_BLOCK_ROWS is unset.  self_check: the self-loop check of every used node
// (graph/mod.rs:210-217) ahead of the first block.  copy_stream is synchronised on every
// path: no copy still writes into the object once this returns or throws.
void fill_rows(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t flags, sg_routing_info* ri, uint32_t r0,
               uint32_t r1, uint32_t block_rows, bool self_check, FillRows* out) {
  const uint32_t n_used = ri->n;
  out->min_lat = UINT64_MAX;
  out->wide.clear();
  hipStream_t st = ctx->stream;
  if (!ctx->copy_stream) {
    SG_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++) {
      SG_HIP(hipEventCreateWithFlags(&ctx->stage_done[b], hipEventDisableTiming));
      SG_HIP(hipEventCreateWithFlags(&ctx->stage_copied[b], hipEventDisableTiming));
    }
  }
  // an earlier fill that failed may have left copies in flight into its staging buffers
  SG_HIP(hipStreamSynchronize(ctx->copy_stream));
  uint32_t* d_used = ctx->r_used.get<uint32_t>(n_used);
  {
    char* hu = stage_acquire(ctx, 1, (size_t)n_used * 4);
    memcpy(hu, nodes, (size_t)n_used * 4);
    SG_HIP(hipMemcpyAsync(d_used, hu, (size_t)n_used * 4, hipMemcpyHostToDevice, st));
    stage_release(ctx, 1);
  }
  const bool shortest = flags & SG_ROUTE_SHORTEST_PATH;
  if (shortest && self_check) raise_self_loops(ctx, net, launch_self_loops(ctx, net, d_used, n_used), nodes);
  if (r1 <= r0) return;
  // at least 64 rows, whole 64-row batches
  uint32_t rows = (uint32_t)std::max(64, knob_int("SG_RI_BLOCK_ROWS", (int)block_rows));
  rows = std::min(r1 - r0, (rows + 63) / 64 * 64);
  uint64_t* slat[2];
  float* sloss[2];
  uint64_t* spack[2];
  for (int b = 0; b < 2; b++) {
    slat[b] = ctx->r_stage_lat[b].get<uint64_t>((size_t)rows * n_used);
    sloss[b] = ctx->r_stage_loss[b].get<float>((size_t)rows * n_used);
    spack[b] = ctx->r_stage_pack[b].get<uint64_t>((size_t)rows * n_used);
  }
  const unsigned nbp = grid_for((size_t)rows * n_used / 2, 256, 4096);
  uint64_t m = UINT64_MAX;
  int k = 0;
  try {
    for (uint32_t b0 = r0; b0 < r1; b0 += rows, k++) {
      const uint32_t b1 = std::min(r1, b0 + rows), b = k & 1;
      ctx->in_fill = true;
      try {
        if (shortest)
          shortest_paths(ctx, net, d_used, nodes, n_used, b0, b1, slat[b], sloss[b]);
        else
          direct_paths(ctx, net, d_used, nodes, n_used, b0, b1, slat[b], sloss[b]);
      } catch (...) {
        ctx->in_fill = false;
        throw;
      }
      ctx->in_fill = false;
      const size_t cells = (size_t)(b1 - b0) * n_used;
      // (workspace fetched after the build, which may grow these buffers)
      unsigned long long* ctl = ctx->r_err.get<unsigned long long>(4);
      SG_HIP(hipMemsetAsync(ctl, 0xff, 8, st));
      SG_HIP(hipMemsetAsync(ctl + 1, 0, 8, st));
      if (k >= 2) SG_HIP(hipStreamWaitEvent(st, ctx->stage_copied[b], 0));  // block k - 2 left spack[b]
      hipLaunchKernelGGL(k_pack_cells, dim3(nbp), dim3(256), 0, st, slat[b], sloss[b], cells, spack[b], ctl);
      SG_CHECK_LAUNCH();
      SG_HIP(hipEventRecord(ctx->stage_done[b], st));
      SG_HIP(hipStreamWaitEvent(ctx->copy_stream, ctx->stage_done[b], 0));
      SG_HIP(hipMemcpyAsync(ri->cell + (size_t)b0 * n_used, spack[b], cells * 8, hipMemcpyDeviceToHost,
                            ctx->copy_stream));
      SG_HIP(hipEventRecord(ctx->stage_copied[b], ctx->copy_stream));
      unsigned long long h[2] = {0, 0};
      copy_to_host(ctx, h, ctl, 16);  // (the next block's build starts after this sync; the copy runs on)
      m = std::min<uint64_t>(m, h[0]);
      if (h[1]) {  // paths of 4.29 s or more: their u64 latencies to the side table
        uint64_t* list = ctx->r_misc.get<uint64_t>(2 * h[1]);
        SG_HIP(hipMemsetAsync(ctl + 1, 0, 8, st));
        hipLaunchKernelGGL(k_wide_list, dim3(grid_for(cells, 256, 4096)), dim3(256), 0, st, slat[b], cells,
                           (uint64_t)b0 * n_used, ctl + 1, list);
        SG_CHECK_LAUNCH();
        std::vector<uint64_t> hl(2 * h[1]);
        copy_to_host(ctx, hl.data(), list, hl.size() * 8);
        for (size_t i = 0; i < h[1]; i++) out->wide.push_back({hl[2 * i], hl[2 * i + 1]});
      }
    }
  } catch (...) {
    (void)hipStreamSynchronize(ctx->copy_stream);  // no copy may still run into the object
    throw;
  }
  SG_HIP(hipStreamSynchronize(ctx->copy_stream));
  out->min_lat = m;
}

// A fill's start: the object as after sg_routing_info_create (not filled, no row set).
void fill_reset(sg_routing_info* ri) {
  ri->filled = false;
  ri->min_lat = UINT64_MAX;
  ri->wide.clear();
  std::fill(ri->row_set.begin(), ri->row_set.end(), 0);
  ri->rows_set = 0;
}

// A fill's end: every row written, the wide cells sorted by cell.
void fill_finish(sg_routing_info* ri, uint64_t min_lat, std::vector<sg_routing_info::Wide>&& wide) {
  ri->wide = std::move(wide);
  std::sort(ri->wide.begin(), ri->wide.end(),
            [](const sg_routing_info::Wide& x, const sg_routing_info::Wide& y) { return x.cell < y.cell; });
  std::fill(ri->row_set.begin(), ri->row_set.end(), 2);  // written; per-row minima not kept
  ri->rows_set = ri->n;
  ri->min_lat = min_lat;
  ri->filled = true;
}
}  // namespace sg

extern "C" {

// The whole table into a host RoutingInfo: fill_rows over every row.
int32_t sg_routing_info_fill(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t flags, sg_routing_info* ri) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (!net || net->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "network belongs to another context");
    if (!ri) throw Error(SG_ERR_INVALID_ARG, "null routing info");
    const uint32_t n_used = ri->n;
    if (n_used && !nodes) throw Error(SG_ERR_INVALID_ARG, "null node list");
    check_node_list(net, nodes, n_used);
    fill_reset(ri);
    if (n_used == 0) {
      ri->filled = true;
      return;
    }
    FillRows out;
    fill_rows(ctx, net, nodes, flags, ri, 0, n_used, (n_used + 7) / 8, true, &out);  // blocks of about 1/8 of the table
    fill_finish(ri, out.min_lat, std::move(out.wide));
  });
}

int32_t sg_routing_min_latency(sg_ctx* ctx, const uint64_t* d_latency_ns, size_t count,
                               uint64_t* out_min) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (!out_min || (count && !d_latency_ns)) throw Error(SG_ERR_INVALID_ARG, "null argument");
    unsigned long long* m = ctx->r_err.get<unsigned long long>(4);
    SG_HIP(hipMemsetAsync(m, 0xff, 8, ctx->stream));
    if (count) {
      const unsigned nb = grid_for(count, 256, 2048);
      unsigned long long* part = ctx->r_misc.get<unsigned long long>(nb);
      hipLaunchKernelGGL(k_min_u64, dim3(nb), dim3(256), 0, ctx->stream, d_latency_ns, count, part);
      hipLaunchKernelGGL(k_min_final, dim3(1), dim3(256), 0, ctx->stream, part, nb, m);
    }
    SG_CHECK_LAUNCH();
    unsigned long long h = 0;
    copy_to_host(ctx, &h, m, 8);
    *out_min = h;
  });
}

}  // extern "C"
