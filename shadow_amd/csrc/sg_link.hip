// sg_link.hip -- link loads: a per-pair traffic matrix folded onto the graph's links through
// pred rows.
//
// sg_routing_tree says which links a path uses (pred rows, sg_tree.hip); the delivery round
// counts delivered packets per (source row, destination column) (sg_ctx_set_packet_counters).
// This file joins the two: how much crossed each link, exactly, on the device, after the fact --
// the round's kernels are untouched and pay nothing.
//
// Definitions.  A LINK is a distinct ordered node pair (u, v) joined by at least one edge: an
// undirected edge {a, b} gives (a, b) and (b, a), a directed edge one link, a self-loop (a, a);
// parallel edges are ONE link (pred is defined by node).  The public order is ascending
// (head v, tail u): the links into one node are contiguous, which is the lookup the kernel needs.
// For row i of source s = nodes[i], its pred row and its counter row c[i][j], j < count_cols
// (columns at or past count_cols count zero), sub_i[v] = the sum of c[i][j] over the columns j
// whose node lies in v's subtree of the row's tree, v included, the diagonal column excluded.
//   link_load[(pred_i[v], v)] += sub_i[v]   for v != s
//   link_load[(s, s)]         += c[i][i]    (the diagonal cell's path is the self-loop)
//   node_load[v]              += sub_i[v]   for v != s (what arrives at or passes through v)
// All sums are u64 and wrap; they are ADDED to what the outputs hold, so row blocks, group
// members and successive intervals sum into one array.  Integer adds only: exact, any order.
//
// One row, one workgroup, persistent over rows.  Per node: sub u64, a child counter u32, parent
// u16 (14 bytes: 10k nodes in one CU's LDS; the limit comes from the device, link_lds_max).
//   1. Stage the row by node (16-byte loads where the rows are aligned), reduce "any counter
//      nonzero": an all-zero row ends here, its pred row not read any further (not validated).
//      A pred value >= n or pred[s] != s ends the row with an error before any index is formed.
//   2. Count children: one LDS add per node.  The first child adds one more, so a node with
//      children holds children + 1 and never reads 0 again; 0 means "leaf", for the whole row.
//   3. Every thread takes the leaves among its nodes and walks up, in the state alone: at v, one
//      LDS u64 add of sub[v] into sub[parent] (none when sub[v] == 0), then the decrement of the
//      parent's counter.  The decrement that finds 2 is the last child's: that thread goes on
//      with the parent, every other thread's walk ends.  O(n) LDS operations per row whatever
//      the depth, no barrier per level, and no queue: the releasing thread carries the released
//      node itself, so nothing spins or waits -- every loop is bounded by n.  The order that
//      matters -- a thread's add into sub[parent] before its decrement of the parent's counter --
//      is the order of two LDS operations of one wave, which the LDS executes in issue order; a
//      compiler fence keeps the issue order, and no global access is in flight in this step.
//   4. A node (other than s) whose counter still reads >= 2 was never released: the row is not a
//      tree (the nodes of a cycle are never released).
//   5. The nodes with sub != 0 are listed (one LDS add each, the list in the counters' words):
//      real traffic is sparse, 1M packets over 10^8 cells leave about 800 of 10k nodes per row.
//   6. A lane per listed node: the link by a binary search for parent[v] among
//      lk_tail[lk_off[v] .. lk_off[v + 1]) (L2 resident), one global u64 add each to link_load
//      and node_load.  A node with sub == 0 costs no lookup and no global atomic.  With the
//      lookups inside the walk of step 3 -- the first form measured -- every step of a wave
//      waited on some lane's dependent loads: 2.44 ms at C3 against this form's 1.02.
// Global path (rows past the LDS limit, SG_LINK_LDS=0): the same algorithm with sub, the counters
// and parent in a per-workgroup scratch row, every access an agent-scope atomic at the L2; there
// two addresses are two L2 channels, so the add into sub[parent] is drained (a release fence)
// before the decrement.
// Errors go through u64 mins into flag words, one per kind, read at the call's one
// synchronisation: the first (row, col) in row-major order.
//
// sg_link_load_packets (k_link_packets, below the fold): the same sums straight from a round's
// batch, without the counter matrix.  A lane per packet: the source's route row, the destination
// resolved through the hosts' address map, then the tree path walked from the destination up to
// the source, the packet's weight added to every link and node on the way.  Cost in proportion
// to packets x hops; no per-row state, so no node limit and one path for every graph size.
// Its host side is the halves of sg_walks.h (link_packets_check / _enqueue / _finish): the entry
// point runs them back to back, a device group (sg_group_trace.hip) per member.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sg_device.h"
#include "sg_hosts.h"
#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_links.h"
#include "sg_walks.h"

namespace sg {

constexpr size_t LINK_STATIC_LDS = 512;   // the kernels' static LDS (the flag words and __syncthreads_or's own: 288 bytes), rounded up
constexpr size_t LINK_NODE_BYTES = 14;   // sub u64 + child counter u32 + parent u16
constexpr size_t LINK_SCRATCH_BYTES = 16;  // global path: sub u64 + child counter u32 + parent u32
// flag words: the first (row << 32) | col of each kind
enum { LINK_BAD_RANGE = 0, LINK_BAD_ROOT = 1, LINK_BAD_LINK = 2, LINK_BAD_CYCLE = 3, LINK_BAD_KINDS = 4 };

// (LinkArgs, link_find and link_node_index: sg_links.h, shared with the walks of sg_walks.h)
// The tree rows and what the dense fold alone takes.
struct LinkFoldArgs : LinkArgs {  // (bad: LINK_BAD_KINDS words)
  uint32_t count_cols;
  const unsigned long long* counts;
  unsigned long long* link_load;  // or null
  unsigned long long* node_load;  // or null
  unsigned char* scratch;         // global path: LINK_SCRATCH_BYTES * n per workgroup
  int vec;                        // 16-byte loads are aligned in every row
};

// The per-node state of one row: in LDS (relaxed workgroup-scope accesses) or in the workgroup's
// scratch row (agent-scope accesses at the L2).
template <bool LDS>
struct LinkState {
  unsigned long long* sub;
  uint32_t* cnt;
  uint16_t* par16;  // LDS
  uint32_t* par32;  // global
  static constexpr int SCOPE = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  __device__ __forceinline__ void init(uint32_t v, uint32_t p, unsigned long long x) {
    if (LDS) {
      sub[v] = x;
      par16[v] = (uint16_t)p;
    } else {
      __hip_atomic_store(&sub[v], x, __ATOMIC_RELAXED, SCOPE);
      __hip_atomic_store(&par32[v], p, __ATOMIC_RELAXED, SCOPE);
    }
  }
  __device__ __forceinline__ void zero_cnt(uint32_t v) {
    if (LDS)
      cnt[v] = 0u;
    else
      __hip_atomic_store(&cnt[v], 0u, __ATOMIC_RELAXED, SCOPE);
  }
  __device__ __forceinline__ uint32_t parent(uint32_t v) const {
    return LDS ? (uint32_t)par16[v] : __hip_atomic_load(&par32[v], __ATOMIC_RELAXED, SCOPE);
  }
  __device__ __forceinline__ unsigned long long load_sub(uint32_t v) const {
    return __hip_atomic_load(&sub[v], __ATOMIC_RELAXED, SCOPE);
  }
  __device__ __forceinline__ uint32_t load_cnt(uint32_t v) const {
    return __hip_atomic_load(&cnt[v], __ATOMIC_RELAXED, SCOPE);
  }
  __device__ __forceinline__ void add_sub(uint32_t v, unsigned long long x) {
    __hip_atomic_fetch_add(&sub[v], x, __ATOMIC_RELAXED, SCOPE);
  }
  __device__ __forceinline__ uint32_t add_cnt(uint32_t v, uint32_t x) {
    return __hip_atomic_fetch_add(&cnt[v], x, __ATOMIC_RELAXED, SCOPE);
  }
  __device__ __forceinline__ uint32_t dec_cnt(uint32_t v) {
    return __hip_atomic_fetch_sub(&cnt[v], 1u, __ATOMIC_RELAXED, SCOPE);
  }
  // the list of step 5 lies in the counters' words
  __device__ __forceinline__ void set_list(uint32_t k, uint32_t v) {
    if (LDS)
      cnt[k] = v;
    else
      __hip_atomic_store(&cnt[k], v, __ATOMIC_RELAXED, SCOPE);
  }
  __device__ __forceinline__ uint32_t get_list(uint32_t k) const {
    return LDS ? cnt[k] : __hip_atomic_load(&cnt[k], __ATOMIC_RELAXED, SCOPE);
  }
};

template <bool LDS>
__global__ void __launch_bounds__(1024) k_link_load(const LinkFoldArgs a) {
  extern __shared__ __align__(16) unsigned char link_smem[];
  __shared__ uint32_t s_bad[LINK_BAD_KINDS], s_count;
  const uint32_t tid = threadIdx.x, T = blockDim.x, n = a.n;
  LinkState<LDS> st;
  if (LDS) {
    st.sub = (unsigned long long*)link_smem;
    st.cnt = (uint32_t*)(st.sub + n);
    st.par16 = (uint16_t*)(st.cnt + n);
    st.par32 = nullptr;
  } else {
    unsigned char* base = a.scratch + (size_t)blockIdx.x * n * LINK_SCRATCH_BYTES;
    st.sub = (unsigned long long*)base;
    st.cnt = (uint32_t*)(st.sub + n);
    st.par16 = nullptr;
    st.par32 = st.cnt + n;
  }
  if (tid < LINK_BAD_KINDS) s_bad[tid] = LINK_NONE;
  __syncthreads();
  for (uint32_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
    const uint32_t i = a.row_begin + r;  // the row's own column
    const uint32_t s = a.nodes[i];
    const uint32_t* __restrict__ pred = a.pred + (size_t)r * n;
    const unsigned long long* __restrict__ cnts = a.counts + (size_t)r * a.count_cols;
    // ---- 1. stage by node; any counter nonzero; values in range; pred[s] == s
    bool any = false;
    uint32_t bad_range = LINK_NONE, bad_root = LINK_NONE;
    unsigned long long diag = 0ull;
    auto one = [&](uint32_t j, uint32_t v, uint32_t p, unsigned long long c) {
      any |= c != 0ull;
      if (p >= n) {
        bad_range = min(bad_range, j);
        p = v;  // (never followed: the row ends below)
      }
      if (j == i) {
        diag = c;
        c = 0ull;
        if (p != s) bad_root = j;
      }
      st.init(v, p, c);
      st.zero_cnt(j);
    };
    if (a.vec) {
      for (uint32_t j = tid * 4; j < n; j += T * 4) {
        const uint4 nd = *(const uint4*)&a.nodes[j];
        const uint4 pr = *(const uint4*)&pred[j];
        ulonglong2 c01 = make_ulonglong2(0ull, 0ull), c23 = c01;
        if (j < a.count_cols) {  // (count_cols is a multiple of 4 here)
          c01 = *(const ulonglong2*)&cnts[j];
          c23 = *(const ulonglong2*)&cnts[j + 2];
        }
        one(j, nd.x, pr.x, c01.x);
        one(j + 1, nd.y, pr.y, c01.y);
        one(j + 2, nd.z, pr.z, c23.x);
        one(j + 3, nd.w, pr.w, c23.y);
      }
    } else {
      for (uint32_t j = tid; j < n; j += T) one(j, a.nodes[j], pred[j], j < a.count_cols ? cnts[j] : 0ull);
    }
    // (the barrier also ends the last row's use of the state)
    if (!__syncthreads_or(any)) continue;  // an all-zero row: nothing to add, its pred row not validated
    if (bad_range != LINK_NONE) atomicMin(&s_bad[LINK_BAD_RANGE], bad_range);
    if (bad_root != LINK_NONE) atomicMin(&s_bad[LINK_BAD_ROOT], bad_root);
    __syncthreads();
    if (s_bad[LINK_BAD_RANGE] != LINK_NONE || s_bad[LINK_BAD_ROOT] != LINK_NONE) {
      __syncthreads();
      if (tid < 2 && s_bad[tid] != LINK_NONE) {
        atomicMin(&a.bad[tid], ((unsigned long long)i << 32) | s_bad[tid]);
        s_bad[tid] = LINK_NONE;
      }
      __syncthreads();
      continue;
    }
    // ---- 2. children per node (+1 from the first child: a node with children never reads 0)
    for (uint32_t v = tid; v < n; v += T) {
      if (v == s) continue;
      const uint32_t p = st.parent(v);
      if (st.add_cnt(p, 1u) == 0u) st.add_cnt(p, 1u);
    }
    __syncthreads();
    // ---- 3. from every leaf upwards, in the state alone; the last child to arrive goes on
    // with the parent
    for (uint32_t v = tid; v < n; v += T) {
      if (v == s || st.load_cnt(v) != 0u) continue;
      uint32_t u = v;
      for (uint32_t step = 0; step < n; step++) {  // (bounded: a walk visits a node once)
        const uint32_t p = st.parent(u);
        if (p == s) break;
        const unsigned long long x = st.load_sub(u);
        if (x != 0ull) {
          st.add_sub(p, x);
          // the add before the decrement that may release p to another wave
          if (LDS)
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
          else
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
        if (st.dec_cnt(p) != 2u) break;
        __atomic_signal_fence(__ATOMIC_SEQ_CST);  // sub[p] is read after the decrement returned
        u = p;
      }
    }
    if (tid == 0) s_count = 0u;
    __syncthreads();
    // ---- 4. a node never released: not a tree
    uint32_t bad_cycle = LINK_NONE;
    for (uint32_t v = tid; v < n; v += T)
      if (v != s && st.load_cnt(v) >= 2u) bad_cycle = min(bad_cycle, a.pos[v]);
    if (bad_cycle != LINK_NONE) atomicMin(&s_bad[LINK_BAD_CYCLE], bad_cycle);
    __syncthreads();
    // ---- 5. the nodes that carry traffic, listed in the counters' words (their last use was 4.)
    for (uint32_t v = tid; v < n; v += T)
      if (v != s && st.load_sub(v) != 0ull) st.set_list(atomicAdd(&s_count, 1u), v);
    __syncthreads();
    // ---- 6. one lookup and the global adds per listed node, every lane its own
    uint32_t bad_link = LINK_NONE;
    if (diag != 0ull) {  // (this thread staged column i)
      const uint32_t k = link_find(a, s, s);
      if (k == LINK_NONE)
        bad_link = i;
      else if (a.link_load)
        atomicAdd(&a.link_load[k], diag);
    }
    const uint32_t listed = s_count;
    for (uint32_t q = tid; q < listed; q += T) {
      const uint32_t v = st.get_list(q);
      const unsigned long long x = st.load_sub(v);
      const uint32_t k = link_find(a, st.parent(v), v);
      if (k == LINK_NONE) {
        bad_link = min(bad_link, a.pos[v]);
      } else {
        if (a.link_load) atomicAdd(&a.link_load[k], x);
        if (a.node_load) atomicAdd(&a.node_load[v], x);
      }
    }
    if (bad_link != LINK_NONE) atomicMin(&s_bad[LINK_BAD_LINK], bad_link);
    __syncthreads();  // (and the next row reuses the state)
    if (tid >= 2 && tid < LINK_BAD_KINDS && s_bad[tid] != LINK_NONE) {
      atomicMin(&a.bad[tid], ((unsigned long long)i << 32) | s_bad[tid]);
      s_bad[tid] = LINK_NONE;
    }
    __syncthreads();
  }
}

// ---- sg_link_load_packets: a lane per packet walks its tree path
// (the item rule and the flag words: sg_walks.h; WALK_COUNTED = the packets counted)
// Hops walked between two flushes of the global adds.  A no-return atomic stays counted in vmcnt
// for hundreds of cycles, and the next dependent load waits for everything issued before it (every
// wait in the code object is vmcnt(0)): with the adds after every hop each hop would pay that
// wait; held back, LP_HOPS hops pay it once.  (The per-hop form was not measured.)
constexpr int LP_HOPS = 4;

// (LinkPacketArgs: sg_walks.h)

// One counted packet's walk: weight w from column j up row i's tree; returns its hops.
__device__ __forceinline__ uint32_t link_packet_walk(const LinkPacketArgs& a, uint32_t i, uint32_t j,
                                                     unsigned long long w) {
  const LinkArgs& l = a.l;
  const uint32_t n = l.n;
  const uint32_t s = l.nodes[i], d = l.nodes[j];
  const uint32_t* __restrict__ row = l.pred + (size_t)(i - l.row_begin) * n;
  const unsigned long long cell = (unsigned long long)i << 32;
  if (d == s) {  // the self-loop (get_edge_weight's rule), one hop
    const uint32_t k = link_find(l, s, s);
    if (k == LINK_NONE)
      atomicMin(&l.bad[WALK_BAD_LINK], cell | j);
    else if (a.link_load)
      atomicAdd(&a.link_load[k], w);
    return 1u;
  }
  // v climbs from d; cv its column; pv = pred_i[v], gathered one hop ahead
  uint32_t v = d, cv = j, pv = row[j], steps = 0;
  bool go = true;
  while (go) {
    uint32_t ks[LP_HOPS], vs[LP_HOPS];
#pragma unroll
    for (int q = 0; q < LP_HOPS; q++) {
      ks[q] = LINK_NONE;
      vs[q] = 0u;
      if (!go) continue;
      if (steps >= n) {  // n steps and not at s: a cycle
        atomicMin(&l.bad[WALK_BAD_CYCLE], cell | j);
        go = false;
        continue;
      }
      const uint32_t u = pv;
      if (u >= n) {
        atomicMin(&l.bad[WALK_BAD_RANGE], cell | cv);
        go = false;
        continue;
      }
      // the next hop's gather ahead of this hop's search: the search's dependent loads overlap it
      uint32_t cu = 0u;
      if (u != s) {
        cu = l.pos[u];
        pv = row[cu];
      }
      const uint32_t k = link_find(l, u, v);
      if (k == LINK_NONE) {
        atomicMin(&l.bad[WALK_BAD_LINK], cell | cv);
        go = false;
        continue;
      }
      ks[q] = k;
      vs[q] = v;
      steps++;
      v = u;
      cv = cu;
      go = u != s;
    }
#pragma unroll
    for (int q = 0; q < LP_HOPS; q++) {
      if (ks[q] == LINK_NONE) continue;
      if (a.link_load) atomicAdd(&a.link_load[ks[q]], w);
      if (a.node_load) atomicAdd(&a.node_load[vs[q]], w);
    }
  }
  return steps;
}

// COMBINE (the default; SG_LINK_COMBINE=0 is the plain form): a wave first sums the weights of its
// lanes' equal (row, column) pairs into the lowest such lane, which walks for all of them; the
// others take its hop count.  A batch grouped by source host repeats pairs among neighbours: at
// C3, 1M packets over 20,000 pairs took 0.112 ms against the plain form's 1.139; on uniform pairs,
// where nothing combines, it was no slower.
template <bool COMBINE>
__global__ void __launch_bounds__(256) k_link_packets(const LinkPacketArgs a) {
  __shared__ uint32_t s_counted;
  const LinkArgs& l = a.l;
  if (threadIdx.x == 0) s_counted = 0u;
  __syncthreads();
  uint32_t counted = 0;
  // (the trip count is the same for every lane of a workgroup: COMBINE exchanges across a wave)
  for (uint32_t base = blockIdx.x * blockDim.x; base < a.n_packets; base += gridDim.x * blockDim.x) {
    const uint32_t p = base + threadIdx.x;
    uint32_t hops = LINK_NONE, i = 0, j = 0;
    unsigned long long w = 0ull;
    bool walk = false;
    if (p < a.n_packets) {
      uint32_t kind;
      walk = packet_item(a.pk, l, p, i, j, kind);
      if (kind != LINK_NONE) flag_item(l, p, kind);
      if (walk) {
        counted++;
        w = a.weight ? (unsigned long long)a.weight[p] : 1ull;
      }
    }
    if (COMBINE) {
      const uint32_t lane = threadIdx.x & 63u;
      // (a lane that does not walk gets a key of its own: row ~0 is no row)
      const uint32_t ki = walk ? i : 0xFFFFFFFFu, kj = walk ? j : lane;
      uint32_t first = lane;
      unsigned long long sum = 0ull;
      for (int q = 63; q >= 0; q--) {
        const uint32_t qi = __builtin_amdgcn_readlane(ki, q), qj = __builtin_amdgcn_readlane(kj, q);
        const uint32_t wlo = __builtin_amdgcn_readlane((uint32_t)w, q);
        const uint32_t whi = __builtin_amdgcn_readlane((uint32_t)(w >> 32), q);
        if (qi == ki && qj == kj) {
          first = (uint32_t)q;
          sum += ((unsigned long long)whi << 32) | wlo;
        }
      }
      if (walk && first == lane) hops = link_packet_walk(a, i, j, sum);
      const uint32_t got = __shfl(hops, first);
      if (walk) hops = got;
    } else if (walk) {
      hops = link_packet_walk(a, i, j, w);
    }
    if (a.hops && p < a.n_packets) a.hops[p] = hops;
  }
  if (counted) atomicAdd(&s_counted, counted);
  __syncthreads();
  if (threadIdx.x == 0 && s_counted) atomicAdd(&l.bad[WALK_COUNTED], (unsigned long long)s_counted);
}

// The most nodes the LDS path takes on this device: 14 bytes a node in what a workgroup may
// allocate (lds_bytes), and u16 parents.
static uint32_t link_lds_max(const sg_ctx* ctx, size_t* lds_bytes) {
  int lds = 0;
  SG_HIP(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  *lds_bytes = (size_t)std::max(lds, 0);
  if (*lds_bytes <= LINK_STATIC_LDS) return 0;
  const size_t n = (*lds_bytes - LINK_STATIC_LDS) / LINK_NODE_BYTES;
  return (uint32_t)std::min<size_t>(n, 0xFFFFu);
}

// The net's links, built once: the edge list back from the device, sorted and made unique on the
// host by (head, tail), lk_off / lk_tail uploaded.  Off the hot path.
void ensure_links(sg_ctx* ctx, sg_net* net) {
  if (net->links) return;
  const uint32_t n = net->n_nodes, m = net->n_edges;
  std::vector<uint32_t> es(m), ed(m);
  if (m) {
    SG_HIP(hipMemcpyAsync(es.data(), net->e_src, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(ed.data(), net->e_dst, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  // keys (head << 32) | tail
  std::vector<uint64_t> keys;
  keys.reserve((size_t)m * (net->directed ? 1 : 2));
  for (uint32_t e = 0; e < m; e++) {
    keys.push_back(((uint64_t)ed[e] << 32) | es[e]);
    if (!net->directed) keys.push_back(((uint64_t)es[e] << 32) | ed[e]);
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  if (keys.size() >= 0xFFFFFFFFull) throw Error(SG_ERR_CAPACITY, "more than 2^32 - 2 links");
  const uint32_t nl = (uint32_t)keys.size();
  std::vector<uint32_t> tail(nl), head(nl), off((size_t)n + 1, 0u);
  for (uint32_t k = 0; k < nl; k++) {
    head[k] = (uint32_t)(keys[k] >> 32);
    tail[k] = (uint32_t)keys[k];
    off[head[k] + 1]++;
  }
  for (uint32_t v = 0; v < n; v++) off[v + 1] += off[v];
  auto find = [&](uint32_t t, uint32_t h) {
    return (uint32_t)(std::lower_bound(keys.begin(), keys.end(), ((uint64_t)h << 32) | t) - keys.begin());
  };
  std::vector<uint32_t> fwd(m), rev(m);
  for (uint32_t e = 0; e < m; e++) {
    fwd[e] = find(es[e], ed[e]);
    rev[e] = net->directed ? 0xFFFFFFFFu : find(ed[e], es[e]);
  }
  void* mem = nullptr;
  const size_t off_bytes = (((size_t)n + 1) * 4 + 15) & ~(size_t)15;
  SG_HIP(hipMalloc(&mem, off_bytes + std::max<size_t>((size_t)nl * 4, 16)));
  hipError_t e1 = hipMemcpy(mem, off.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice);
  hipError_t e2 = nl ? hipMemcpy((char*)mem + off_bytes, tail.data(), (size_t)nl * 4, hipMemcpyHostToDevice) : hipSuccess;
  if (e1 != hipSuccess || e2 != hipSuccess) {
    (void)hipFree(mem);
    SG_HIP(e1);
    SG_HIP(e2);
  }
  net->lk_mem = mem;
  net->lk_off = (uint32_t*)mem;
  net->lk_tail = (uint32_t*)((char*)mem + off_bytes);
  net->n_links = nl;
  net->lk_tail_h.swap(tail);
  net->lk_head_h.swap(head);
  net->e_fwd.swap(fwd);
  net->e_rev.swap(rev);
  net->links = true;
}

// What a pred row's error says, in the dense fold's decode and the walks' (throw_pred_error).
static const char WHY_RANGE[] = "holds a node index out of range";
static const char WHY_LINK[] = "names a predecessor that no link joins to the node (not a link)";

// Rows [row_begin, row_end) folded into the device outputs (d_* row-major from row_begin).
// Queues everything and synchronises once, on the flag words; `after` runs between the kernel
// and that synchronisation (the copies of host outputs).
template <class F>
static void link_rows(sg_ctx* ctx, sg_net* net, const uint32_t* h_nodes, uint32_t row_begin, uint32_t row_end,
                      const uint32_t* d_pred, const uint64_t* d_counts, uint32_t count_cols, uint64_t* d_link,
                      uint64_t* d_node, F after) {
  hipStream_t stq = ctx->stream;
  const uint32_t n = net->n_nodes, rows = row_end - row_begin;
  uint32_t* d_idx = link_node_index(ctx, h_nodes, n);
  unsigned long long* bad = ctx->l_flag.get<unsigned long long>(LINK_BAD_KINDS);
  SG_HIP(hipMemsetAsync(bad, 0xff, LINK_BAD_KINDS * 8, stq));
  LinkFoldArgs a;
  static_cast<LinkArgs&>(a) = link_args(net, d_idx, n, row_begin, rows, d_pred, bad);
  a.count_cols = count_cols;
  a.counts = (const unsigned long long*)d_counts;
  a.link_load = (unsigned long long*)d_link;
  a.node_load = (unsigned long long*)d_node;
  a.scratch = nullptr;
  a.vec = n % 4 == 0 && count_cols % 4 == 0 && ((uintptr_t)d_pred & 15) == 0 && ((uintptr_t)d_counts & 15) == 0;
  size_t lds_bytes = 0;
  const uint32_t n_max = link_lds_max(ctx, &lds_bytes);
  const bool lds = knob_int("SG_LINK_LDS", 1) != 0 && n <= n_max;
  // small graphs: 256 threads, so that a CU holds several rows
  const unsigned threads = n <= 2048 ? 256u : 1024u;
  // bytes read: the pred row and the counter row
  const double bytes = (double)rows * (4.0 * (double)n + 8.0 * (double)count_cols);
  {
    TimedLaunch tl(ctx, "link_load", bytes);
    if (lds) {
      const size_t dyn = (size_t)n * LINK_NODE_BYTES;
      // persistent: as many workgroups as the LDS holds rows, at most 8 per CU
      const size_t per_cu = std::max<size_t>(1, std::min<size_t>(8, lds_bytes / (dyn + LINK_STATIC_LDS)));
      const unsigned grid = (unsigned)std::min<size_t>(rows, per_cu * (size_t)ctx->n_cu);
      SG_HIP(hipFuncSetAttribute((const void*)k_link_load<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
      hipLaunchKernelGGL(k_link_load<true>, dim3(grid), dim3(threads), dyn, stq, a);
    } else {
      const unsigned grid = (unsigned)std::min<size_t>(rows, 2 * (size_t)ctx->n_cu);
      a.scratch = ctx->l_scratch.get<unsigned char>((size_t)grid * n * LINK_SCRATCH_BYTES);
      hipLaunchKernelGGL(k_link_load<false>, dim3(grid), dim3(threads), 0, stq, a);
    }
    SG_CHECK_LAUNCH();
  }
  // read_timer("link_lds") = (0, rows launched on the LDS path, the LDS path's node limit)
  timer_set_counter(ctx, "link_lds", (double)n_max, lds ? rows : 0u);
  after();
  unsigned long long h[LINK_BAD_KINDS];
  copy_to_host(ctx, h, bad, sizeof(h));
  int kind = -1;
  for (int k = 0; k < LINK_BAD_KINDS; k++)
    if (h[k] != ~0ull && (kind < 0 || h[k] < h[kind])) kind = k;
  if (kind >= 0) {
    const uint32_t i = (uint32_t)(h[kind] >> 32), j = (uint32_t)h[kind];
    static const char* const why[LINK_BAD_KINDS] = {
        WHY_RANGE, "does not have pred[source] == source", WHY_LINK,
        "is never released: the row has a cycle, it is not a tree"};
    throw Error(SG_ERR_INVALID_ARG,
                "the pred row of source node " + node_name(net, h_nodes[i]) + " at node " +
                    node_name(net, h_nodes[j]) + " " + why[kind],
                i, j);
  }
}

static void link_check_net(sg_ctx* ctx, sg_net* net) {
  if (!net || net->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "network belongs to another context");
}

// ---- the walks' host side (sg_walks.h)
PacketArgs packet_args(const sg_hosts* h, const sg_packets* packets, const uint8_t* status) {
  return PacketArgs{HostMap{h->ip_base, h->dense_span, h->n, h->dense, h->sorted_ip, h->sorted_host},
                    h->route,
                    h->n,
                    packets->src_host,
                    packets->dst_ipv4,
                    status};
}

void throw_item_error(bool packets, unsigned long long word) {
  const uint64_t p = word >> 3;
  const uint32_t kind = (uint32_t)(word & 7);
  static const char* const why_packet[ITEM_TIME + 1] = {
      "has a source host past the host table", "has a source host whose route row lies outside the row block",
      "counts and has a destination address that no host holds", "resolves to a route index that is not below n_nodes",
      "counts and has a send time plus path latency past 2^64 - 1 ns"};
  static const char* const why_pair[ITEM_TIME + 1] = {"", "has a row outside the row block", "",
                                                      "has a column that is not below n_nodes", ""};
  throw Error(kind == ITEM_TIME ? SG_ERR_TIME_OVERFLOW : SG_ERR_INVALID_ARG,
              std::string(packets ? "packet " : "pair ") + std::to_string(p) + " " +
                  (packets ? why_packet : why_pair)[kind],
              (uint32_t)p, 0xFFFFFFFFu);
}

void throw_pred_error(const sg_net* net, const uint32_t* nodes, int kind, unsigned long long word) {
  const uint32_t i = (uint32_t)(word >> 32), j = (uint32_t)word;
  const std::string why = kind == WALK_BAD_RANGE  ? std::string(WHY_RANGE) + " at node "
                          : kind == WALK_BAD_LINK ? std::string(WHY_LINK) + " at node "
                                                  : "does not reach its source within n_nodes steps (a cycle) from node ";
  throw Error(SG_ERR_INVALID_ARG,
              "the pred row of source node " + node_name(net, nodes[i]) + " " + why + node_name(net, nodes[j]), i, j);
}

// ---- sg_link_load_packets' halves (sg_walks.h)
void link_packets_check(const LinkPacketsCall& c, bool check_nodes) {
  link_check_net(c.ctx, c.net);  // (ahead of the host table's: the order of this call's errors)
  if (!c.hosts || c.hosts->ctx != c.ctx) throw Error(SG_ERR_INVALID_ARG, "host table belongs to another context");
  check_rows_call(c.ctx, c.net, c.nodes, c.n_nodes, c.row_begin, c.row_end);
  if (check_nodes) check_node_list(c.net, c.nodes, c.n_nodes);  // in range and none twice: with n_nodes entries, a permutation
  if (!c.packets) throw Error(SG_ERR_INVALID_ARG, "null packets");
  if (c.packets->n_packets && (!c.packets->src_host || !c.packets->dst_ipv4))
    throw Error(SG_ERR_INVALID_ARG, "null packet arrays");
  if (c.row_end > c.row_begin && !c.pred) throw Error(SG_ERR_INVALID_ARG, "null pred rows");
}

void link_packets_enqueue(const LinkPacketsCall& c) {
  sg_ctx* ctx = c.ctx;
  sg_net* net = c.net;
  hipStream_t st = ctx->stream;
  const uint32_t n = c.n_nodes, np = c.packets->n_packets;
  uint32_t* d_idx = link_node_index(ctx, c.nodes, n);
  unsigned long long* bad = ctx->l_flag.get<unsigned long long>(WALK_WORDS_COUNTED);
  SG_HIP(hipMemsetAsync(bad, 0xff, WALK_WORDS * 8, st));
  SG_HIP(hipMemsetAsync(bad + WALK_COUNTED, 0, 8, st));
  const LinkPacketArgs a{link_args(net, d_idx, n, c.row_begin, c.row_end - c.row_begin, c.pred, bad),
                         packet_args(c.hosts, c.packets, c.status),
                         np,
                         c.weight,
                         (unsigned long long*)c.link_load,
                         (unsigned long long*)c.node_load,
                         c.hops};
  // (work = the packets walked, added by the finish once the count is read)
  TimedLaunch tl(ctx, "link_packets", 0.0);
  const dim3 grid(grid_for(np, 256, 16u * (unsigned)ctx->n_cu));
  if (knob_int("SG_LINK_COMBINE", 1) != 0)
    hipLaunchKernelGGL(k_link_packets<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_link_packets<false>, grid, dim3(256), 0, st, a);
  SG_CHECK_LAUNCH();
}

void link_packets_finish(const LinkPacketsCall& c) {
  sg_ctx* ctx = c.ctx;
  unsigned long long h[WALK_WORDS_COUNTED];
  copy_to_host(ctx, h, ctx->l_flag.get<unsigned long long>(WALK_WORDS_COUNTED), sizeof(h));
  timer_add_work(ctx, "link_packets", (double)h[WALK_COUNTED]);
  // read_timer("link_packets_counted") = (0, the packets the last call counted, 0)
  timer_set_counter(ctx, "link_packets_counted", 0.0, h[WALK_COUNTED]);
  if (h[WALK_BAD_ITEM] != ~0ull) throw_item_error(true, h[WALK_BAD_ITEM]);
  int kind = -1;
  for (int k = WALK_BAD_RANGE; k <= WALK_BAD_CYCLE; k++)
    if (h[k] != ~0ull && (kind < 0 || h[k] < h[kind])) kind = k;
  if (kind >= 0) throw_pred_error(c.net, c.nodes, kind, h[kind]);
}

}  // namespace sg

extern "C" {

int32_t sg_net_links(sg_ctx* ctx, sg_net* net, uint32_t* n_links, uint32_t* out_tail, uint32_t* out_head,
                     uint32_t cap) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    link_check_net(ctx, net);
    if (!n_links) throw Error(SG_ERR_INVALID_ARG, "null link count");
    ensure_links(ctx, net);
    *n_links = net->n_links;
    if (net->n_links > cap) throw Error(SG_ERR_CAPACITY, "the link list needs " + std::to_string(net->n_links) + " entries");
    if (net->n_links && (!out_tail || !out_head)) throw Error(SG_ERR_INVALID_ARG, "null output");
    if (net->n_links) {
      memcpy(out_tail, net->lk_tail_h.data(), (size_t)net->n_links * 4);
      memcpy(out_head, net->lk_head_h.data(), (size_t)net->n_links * 4);
    }
  });
}

int32_t sg_net_edge_links(sg_ctx* ctx, sg_net* net, uint32_t* out_fwd, uint32_t* out_rev) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    link_check_net(ctx, net);
    if (net->n_edges && (!out_fwd || !out_rev)) throw Error(SG_ERR_INVALID_ARG, "null output");
    ensure_links(ctx, net);
    if (net->n_edges) {
      memcpy(out_fwd, net->e_fwd.data(), (size_t)net->n_edges * 4);
      memcpy(out_rev, net->e_rev.data(), (size_t)net->n_edges * 4);
    }
  });
}

int32_t sg_link_load(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes, uint32_t row_begin,
                     uint32_t row_end, uint32_t flags, const uint32_t* pred, const uint64_t* counts,
                     uint32_t count_cols, uint64_t* out_link_load, uint64_t* out_node_load) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    check_rows_call(ctx, net, nodes, n_nodes, row_begin, row_end);
    if (count_cols > n_nodes) throw Error(SG_ERR_INVALID_ARG, "count_cols is larger than n_nodes");
    check_node_list(net, nodes, n_nodes);  // in range and none twice: with n_nodes entries, a permutation
    if (!out_link_load && !out_node_load) throw Error(SG_ERR_INVALID_ARG, "null output");
    if (row_end == row_begin) return;
    if (!pred || (count_cols && !counts)) throw Error(SG_ERR_INVALID_ARG, "null pred or counter rows");
    ensure_links(ctx, net);
    hipStream_t st = ctx->stream;
    const uint32_t n = n_nodes, rows = row_end - row_begin, nl = net->n_links;
    if (flags & SG_ROUTE_OUT_DEVICE) {
      link_rows(ctx, net, nodes, row_begin, row_end, pred, counts, count_cols, out_link_load, out_node_load, [] {});
      return;
    }
    // host rows in, host sums out: the device sums start at zero and are added on the host
    uint32_t* d_pred = ctx->l_pred.get<uint32_t>((size_t)rows * n);
    uint64_t* d_cnt = ctx->l_cnt.get<uint64_t>((size_t)rows * count_cols);
    SG_HIP(hipMemcpyAsync(d_pred, pred, (size_t)rows * n * 4, hipMemcpyHostToDevice, st));
    if (count_cols) SG_HIP(hipMemcpyAsync(d_cnt, counts, (size_t)rows * count_cols * 8, hipMemcpyHostToDevice, st));
    uint64_t* d_link = out_link_load ? ctx->l_link.get<uint64_t>(nl) : nullptr;
    uint64_t* d_node = out_node_load ? ctx->l_node.get<uint64_t>(n) : nullptr;
    if (d_link) SG_HIP(hipMemsetAsync(d_link, 0, std::max<size_t>((size_t)nl * 8, 8), st));
    if (d_node) SG_HIP(hipMemsetAsync(d_node, 0, (size_t)n * 8, st));
    std::vector<uint64_t> h_link(d_link ? nl : 0), h_node(d_node ? n : 0);
    link_rows(ctx, net, nodes, row_begin, row_end, d_pred, d_cnt, count_cols, d_link, d_node, [&] {
      if (d_link && nl) SG_HIP(hipMemcpyAsync(h_link.data(), d_link, (size_t)nl * 8, hipMemcpyDeviceToHost, st));
      if (d_node) SG_HIP(hipMemcpyAsync(h_node.data(), d_node, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    });
    for (uint32_t k = 0; k < (d_link ? nl : 0u); k++) out_link_load[k] += h_link[k];
    for (uint32_t v = 0; v < (d_node ? n : 0u); v++) out_node_load[v] += h_node[v];
  });
}

int32_t sg_link_load_packets(sg_ctx* ctx, sg_net* net, sg_hosts* hosts, const uint32_t* nodes, uint32_t n_nodes,
                             uint32_t row_begin, uint32_t row_end, uint32_t flags, const uint32_t* pred,
                             const sg_packets* packets, const uint8_t* status, const uint32_t* weight,
                             uint64_t* out_link_load, uint64_t* out_node_load, uint32_t* out_hops) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    LinkPacketsCall c{ctx,     net,    hosts,  nodes,         n_nodes,       row_begin, row_end,
                      pred,    packets, status, weight,        out_link_load, out_node_load, out_hops};
    link_packets_check(c, true);
    if (!out_link_load && !out_node_load && !out_hops) throw Error(SG_ERR_INVALID_ARG, "null output");
    const uint32_t np = packets->n_packets;
    if (np == 0) return;
    ensure_links(ctx, net);
    hipStream_t st = ctx->stream;
    const uint32_t n = n_nodes, rows = row_end - row_begin, nl = net->n_links;
    const bool dev = (flags & SG_ROUTE_OUT_DEVICE) != 0;
    // host rows in, host sums out: the device sums start at zero and are added on the host
    if (!dev) {
      uint32_t* up = ctx->l_pred.get<uint32_t>((size_t)rows * n);
      if (rows) SG_HIP(hipMemcpyAsync(up, pred, (size_t)rows * n * 4, hipMemcpyHostToDevice, st));
      c.pred = up;
      c.link_load = out_link_load ? ctx->l_link.get<uint64_t>(nl) : nullptr;
      c.node_load = out_node_load ? ctx->l_node.get<uint64_t>(n) : nullptr;
      c.hops = out_hops ? ctx->l_hops.get<uint32_t>(np) : nullptr;
      if (c.link_load) SG_HIP(hipMemsetAsync(c.link_load, 0, std::max<size_t>((size_t)nl * 8, 8), st));
      if (c.node_load) SG_HIP(hipMemsetAsync(c.node_load, 0, (size_t)n * 8, st));
    }
    link_packets_enqueue(c);
    std::vector<uint64_t> h_link(!dev && c.link_load ? nl : 0), h_node(!dev && c.node_load ? n : 0);
    if (!dev) {
      if (c.link_load && nl) SG_HIP(hipMemcpyAsync(h_link.data(), c.link_load, (size_t)nl * 8, hipMemcpyDeviceToHost, st));
      if (c.node_load) SG_HIP(hipMemcpyAsync(h_node.data(), c.node_load, (size_t)n * 8, hipMemcpyDeviceToHost, st));
      if (c.hops) SG_HIP(hipMemcpyAsync(out_hops, c.hops, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    }
    link_packets_finish(c);
    for (uint32_t k = 0; k < (uint32_t)h_link.size(); k++) out_link_load[k] += h_link[k];
    for (uint32_t v = 0; v < (uint32_t)h_node.size(); v++) out_node_load[v] += h_node[v];
  });
}

}  // extern "C"
