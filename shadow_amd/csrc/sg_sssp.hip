// sg_sssp.hip -- per-source shortest paths with the distance row resident in LDS.
//
// Replaces, for graphs whose node count fits a CU's LDS (about 11k nodes), the
// per-source petgraph::algo::dijkstra of NetworkGraph::compute_shortest_paths
// (graph/mod.rs:190-208).  One workgroup owns one source row: its keys live in
// LDS for the whole search, the graph's out-arcs are read from L2 (one 12-B
// record per relaxation), and the finished row is written straight into the
// caller's row-major table.
//
// Why not the batched-source slab kernel (sg_slab.hip k_relax_w2) here: a
// 64-source batch gathers whole 512-B rows, and Bellman-Ford re-gathers a row
// whenever any of its 64 sources improved it -- about 10x the n_used * arcs
// relaxations of Dijkstra at C3.  A per-source search relaxes only what its own
// frontier improved: with delta-stepping buckets about 1.05-1.4x Dijkstra's
// relaxations (SG_SSSP_DIAG reports it).
//
// Exactness.  Edge latency >= 1 ns (graph/mod.rs:105-107) and the f32 loss fold
// is monotone, so petgraph's Dijkstra result is the unique fixed point of the
// source-rooted relaxation key[v] = min(key[v], key[u] (+) w(u, v)) with the
// edge applied on the right (sg_device.h fold_loss); any relaxation order
// reaches it.  Keys whose latency saturates at LAT32_SAT (>= 4.29 s, or
// unreachable) are never propagated and flag the row for the wide kernel
// (sg_slab.hip run_wide), as in the slab kernel.
//
// Flagged key.  key = (latency u32 << 32) | (bits(loss) << 1) | dirty.  Loss is
// in [0, 1], so bits(loss) < 2^31 and the 64-bit integer order of the key is the
// PathProperties order (latency, then loss), the flag ranking last.  A candidate
// carries dirty = 1, so one 64-bit LDS atomic min both relaxes and tests the
// flag: the node improved iff the returned key's (latency, loss) is larger, and
// it must be queued iff the returned key was clean.  An equal candidate never
// replaces a key (its flag is 1, the stored one 0 or 1), so "improved" means
// strictly better.  A pop clears the flag with one atomic AND whose return value
// is the key to relax with; an improvement that lands after it finds the flag
// clear and queues the node again.
//
// Work order: an asynchronous work queue per workgroup, with delta-stepping
// buckets (bucket width `delta`; one workgroup barrier per bucket, none per hop).
//   * A node is dirty from an improvement until it is popped; a node that
//     becomes dirty with latency below `split` is also appended to the queue,
//     so the queue never holds a node twice.
//   * The queue is an LDS ring of u16 node ids with head / tail counters.  A
//     wave claims up to 64 entries (CAS on head), relaxes their out-arcs and
//     appends what it improved (add on tail, then the slot writes; a claimed
//     slot not yet written reads as EMPTY and is waited for).  `busy` counts the
//     waves holding claimed entries; head and busy share one 64-bit LDS word,
//     so a claim is one CAS and a failed claim attempt changes nothing.
//   * Quiescence (busy == 0 and head == tail, read in that order) is stable: no
//     entry appears without a busy wave.  Every wave then meets at a barrier;
//     the dirty nodes left are those at or beyond `split`.  split = (smallest
//     dirty latency) + delta, the dirty nodes below it are queued, and the
//     waves go on.  No dirty node left: the search is done.
//   * Relaxing a popped node: a pop of at most step_arcs arcs (SG_SSSP_STEP_ARCS) is
//     expanded into consecutive slots (owner by scatter + max-scan) and relaxed in as
//     many chunks of 64 as it holds: one, two, or rounds of SSSP_K.  A larger pop: when
//     the largest out-degree among the wave's entries is at most LANE_DEG_MAX, each lane
//     walks its own node's arcs, eight loads in flight (no cross-lane bookkeeping on the
//     dependent chain); otherwise the expansion, SSSP_K chunks of 64 at once.
//
// Bounds (ub_row / ub_w).  For an arc s -> s' whose row D[s'] is already in the
// table, w(s, s') + D[s'][v] is the latency of a real path from s, so it bounds
// D[s][v] from above.  A bounded search starts key[v] at (that bound + 1, loss
// 1.0, clean) instead of infinity: still above the optimum, so the fixed point
// and the proof above are unchanged, but every candidate slower than the bound
// loses its first atomic min and is never queued.  sg_plan.hip sssp_device_plan
// orders the rows in phases, one launch each, so the bound rows of a phase are
// final (an earlier launch) before any search reads them.  A one-launch variant
// with per-row flags (searches reading rows other workgroups had just published)
// was tried: with an L2 write-back before each flag it matched bit for bit and
// saved 3 %, without it the table came out wrong, so it was dropped.
//
// Exact seeds.  When the arc s -> s' has zero loss (bits(1f32 - loss) == 1.0f),
// the left fold from s over s -> s' followed by any path P from s' gives exactly
// P's fold from s' (fold(0, 1.0) = 0, then the same sequence of f32 ops), so
// (w(s, s') + D[s'][v].lat, D[s'][v].loss) is the exact key of a real path.
// Such keys start CLEAN (never queued).  Still exact: every key is a real path's
// value (>= the optimum), and along an optimal path s = v0, .., vk every vi ends
// at its optimum by induction -- either v(i-1) was popped holding its optimum and
// relaxed vi, or v(i-1) held its optimum from the start, i.e. an exact seed via
// some s'; then vi's seed via the same s' is at most w + (D[s'][v(i-1)] (+)
// w(v(i-1), vi)) = opt(vi), so vi also starts at its optimum.  The induction needs
// a seed for every node, so the plan sets SSSP_UB_EXACT only when every node is a
// used node, and a bound row flagged for the wide kernel seeds bounds only.  A
// node reached optimally through an exactly seeded neighbour row is never
// popped: its subtree drops out of the search.
//
// Chained rows (SG_SSSP_CHAIN; persistent workgroups on an undirected graph, the phased
// launches and the launch without a plan, never the flagged one).  One bound row needs no
// publication: the row s the workgroup finished a moment ago, whose final keys are still in its
// LDS.  After the search's closing barrier, and before the output stores are issued (a load or
// a returning atomic issued after them would wait behind them), one wave reads s's out-arcs
// (up to 64), maps each head t through rel to its row, keeps the rows of this block and of this
// launch's phase whose claim word is 0, and tries them in the order (zero-loss arc, latency,
// row) with one relaxed device-scope CAS 0 -> 1 each; the undirected upload mirrors every
// edge (sg_net.hip), so the arc t -> s exists with the same latency w and loss.  The claim
// words only exclude -- no data passes through them, so no fence or cache policy goes with
// them -- and every row, listed or chained, belongs to whoever changed its word; a workgroup
// that finds no neighbour takes the next row of the list whose word it can change.  The loop
// is bounded by the candidates and waits for nothing another workgroup does.  Only a search
// that ended normally chains; the sweep of the last workgroup to give up flags only rows
// whose word is still 0 (a claimed row is its owner's to write or to flag).
//   The chained row's set-up rewrites key[] in place, for all n nodes: a saturated key, or
// one whose latency + w reaches LAT32_SAT - 1, becomes FKEY_INF; else (lat + w, loss, clean)
// when exact, (lat + w + 1, 1.0, clean) when not.  The bound rows the plan lists are then
// merged with min.  s's own key (0, 0.0) gives (w, 0.0), the arc itself.
//   Exactness of those seeds: "Bounds" covers the inexact form.  The exact form needs a
// zero-loss arc, SG_SSSP_EXACT, and an output pass of s that saw no saturated key.  It does
// NOT need every node to be a used node, as the plan's exact seeds do: the LDS row has a key
// for every node, which is the seed-for-every-node the induction above asks for.  A
// saturated key of an UNUSED node, which no output pass sees, does no harm either: latency
// only grows along a path, so an optimal path to a node whose optimum is below LAT32_SAT
// passes only through such nodes, and among them s's row is a fixed point (a popped node
// relaxed every arc, and a candidate is dropped only when it saturates) -- the induction runs
// over those nodes alone.  A node whose optimum from t reaches LAT32_SAT starts at FKEY_INF
// or above its optimum and ends saturated, which flags the row like any other.
//
// Late seeds (SG_SSSP_EARLY; the plain launches, a chained row that has bound rows and is not its
// workgroup's first).  Such a row has a complete start row in LDS once the chained rewrite is done; the
// plan's bound rows only lower keys further, and their 240 KB are bound by what one CU keeps in flight,
// not by anything the search uses.  So the order of its start is: the LDS pass (rewrite, ctl, hb) and
// its barrier; thread 0 writes the source's key, ring[0], TAIL and s_psat, and a barrier; then wave 0
// enters the claim loop while waves 1 .. 15 issue the bound rows' loads (11 columns per thread and
// round, every pair of bound rows) and merge them into key[].  A wave enters the claim loop only after
// its own merge is complete, and the search ends at a workgroup barrier every wave must reach (the
// quiescence barrier; a wave that arrives from its merge finds the queue quiescent or joins the
// search), so no row ends, and no bucket advances, with a bound row unmerged.  A wave that gives up
// leaves as before: the merging waves see ctl[ABORT] at their first claim and meet no barrier on the way.
//   The merge runs beside relaxations and pops, so it is a 64-bit LDS compare-and-swap loop that keeps
// the dirty bit: new = min(old & ~1, seed) | (old & 1), attempted only when the seed is below the key
// read, retried when the word changed.  A plain min with the clean seed over a dirty, queued key would
// clear the flag without a pop; a later improvement would append the node a second time, and the
// ring's capacity (at most n queued) would no longer hold.  With the flag kept, "dirty from an
// improvement until popped, queued exactly once" stands as written; a merge never queues (a clean key
// stays clean, a dirty one is queued already, or lies at or beyond `split` and is found by the next
// bucket advance like any dirty key a relaxation lowered below it).
//   Exactness.  Every key is still a real path's value or above one.  The induction of "Exact seeds"
// along an optimal path s = v0, .., vk now reads: (a) a node whose key reaches its optimum while dirty
// -- by a relaxation, or by a merge onto a dirty key -- is popped afterwards holding it and relaxes its
// successor; (b) a node that reaches its optimum clean did so by an exact seed through some s' (the
// chain's, in the start row, or a bound row's, merged late); its successor's seed through the same s'
// is at most the successor's optimum, and is in the start row or merged before the closing barrier,
// whichever of the two lands first; (c) bound-only seeds are strictly above the optimum, as before, so
// they never stand in for either.  The source's key (0, 0.0, dirty) survives its own column's merge:
// every seed for it is a path s -> s' -> s of latency at least w > 0, never below the key read.
// tests/test_sssp_late_seeds_cpu.py runs this argument as a model, merges at random points.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"

namespace sg {

constexpr int SSSP_THREADS = 1024;  // the largest workgroup (template NT; every launch uses 1024)
constexpr int SSSP_WAVES = SSSP_THREADS / 64;
constexpr int SSSP_K = 4;            // expansion path: chunks of 64 arc slots a wave handles at once
constexpr int SSSP_KB = SSSP_KB_MAX;  // bound rows per bounded search (sg_plan.hip sssp_device_plan)
// static LDS of k_sssp_lds: ctl[8] + red[SSSP_WAVES] (u32), hb (u64), own[SSSP_WAVES][64 * SSSP_K] (u8),
// sink[64] (u64), s_ub[SSSP_KB][3] + s_nub (u32); the slack holds s_item, s_sat, s_chain, s_cw, s_psat
// (4,832 B in every instantiation, by the compiler's resource report)
constexpr size_t SSSP_STATIC_LDS = 4 * (8 + SSSP_WAVES) + 16 + SSSP_WAVES * 64 * SSSP_K + 512 + 4 * (3 * SSSP_KB + 1) + 16;
// lane path: arcs a lane has in flight (template LA; every launch uses 8);
// used up to out-degree lane_deg_max (SG_SSSP_LANE_DEG, default 64; the arcs past LA arc-parallel)

constexpr size_t LDS_PER_CU = 160 * 1024;

constexpr uint64_t FKEY_INF = ((uint64_t)LAT32_SAT << 32) | ((uint64_t)0x3F800000u << 1);  // (SAT, 1.0), clean
__device__ __forceinline__ uint32_t fkey_lat(uint64_t k) { return (uint32_t)(k >> 32); }
__device__ __forceinline__ uint32_t fkey_loss_bits(uint64_t k) { return ((uint32_t)k >> 1) & 0x7FFFFFFFu; }
// key(u) (+) edge (graph/mod.rs:322-331), flagged dirty
// (the loss is in [0, 1], never -0.0: its bits are below 2^31, so the low word is one 32-bit
// shift-or and the high word is the latency itself -- no 64-bit shift, no carry)
__device__ __forceinline__ uint64_t frelax(uint64_t ku, uint32_t edge_lat, float edge_om) {
  const uint32_t lat = __builtin_elementwise_add_sat(fkey_lat(ku), edge_lat);
  const float loss = fold_loss(__uint_as_float(fkey_loss_bits(ku)), edge_om);
  return ((uint64_t)lat << 32) | (uint32_t)((__float_as_uint(loss) << 1) | 1u);
}

// Queue capacity: n + 1024 rounded up to 64.  At most n nodes are queued (one
// entry per dirty node) and at most 16 waves x 64 claimed slots are still being
// read, so a slot is never reused while its last entry is unread.  Slot of a
// counter c: c mod cap by a multiply-high and one correction (cap < 2^17).
__host__ __device__ inline uint32_t sssp_ring_cap(uint32_t n) { return (n + 1024 + 63) / 64 * 64; }
struct RingMod {
  uint32_t cap, m;  // m = floor(2^32 / cap)
  __device__ __forceinline__ uint32_t operator()(uint32_t c) const {
    uint32_t r = c - __umulhi(c, m) * cap;  // in [0, 2 cap)
    return r >= cap ? r - cap : r;
  }
};
constexpr uint16_t RING_EMPTY = 0xFFFF;

// Queue the flagged lanes' nodes (NK candidates per lane): one tail add per call.
// mq[c]: the wave's ballot of candidate c (wave-uniform masks, no per-lane bool kept)
template <int NK>
__device__ __forceinline__ void append_q(const uint64_t* mq, const uint32_t* v, uint16_t* ring, uint32_t* tail,
                                         const RingMod& slot_of, int lane) {
  const uint64_t lt = (1ull << lane) - 1;
  uint32_t tot = 0;
#pragma unroll
  for (int c = 0; c < NK; c++) tot += (uint32_t)__popcll(mq[c]);
  if (!tot) return;
  uint32_t b = 0;
  if (lane == 0) b = atomicAdd(tail, tot);
  b = __builtin_amdgcn_readfirstlane(b);
#pragma unroll
  for (int c = 0; c < NK; c++) {
    if ((mq[c] >> lane) & 1ull) ring[slot_of(b + (uint32_t)__popcll(mq[c] & lt))] = (uint16_t)v[c];
    b += (uint32_t)__popcll(mq[c]);
  }
}

// LDS bytes the kernel needs for n nodes (dynamic part): keys, staged out-arc
// offsets, the queue ring.
size_t sssp_lds_bytes(uint32_t n) {
  return (size_t)n * 8 + (((size_t)n + 1) * 4 + 7) / 8 * 8 + (size_t)sssp_ring_cap(n) * 2;
}

// One workgroup per source row i in [row_begin, row_end): source used[i].
// out_arc: 3 u32 per out-arc (destination, latency clamped to LAT32_SAT,
// bits(1f32 - loss)), grouped by tail node (out_off).
// PART: 0 for a routing build, 1 for sg_routing_info_fill's row blocks (the same
// code; a separate symbol so per-kernel profiles do not mix whole builds with blocks)
// FLAG: one launch for the whole plan (rows in phase order), bound rows taken
// only once published -- see "Flagged rows" below; `done` (per row, zeroed by the
// plan) is 1 for a final row, 2 for a final row with saturated keys (bounds only).
constexpr int SSSP_SC1 = 16;  // buffer cache-policy bits: sc1 (gfx950), MI355X_MICROARCH.md's hand-off
template <bool COUNT, int NT, int LA, int PART, bool FLAG = false>
__global__ void __launch_bounds__(NT)
    k_sssp_lds(const uint32_t* __restrict__ out_off, const uint32_t* __restrict__ out_arc, uint32_t n,
               uint32_t n_arcs, const uint32_t* __restrict__ used, uint32_t n_used, uint32_t row_begin,
               uint32_t out_row0, const uint32_t* __restrict__ self_edge, const uint64_t* __restrict__ e_lat,
               const float* __restrict__ e_loss, uint64_t* __restrict__ out_lat, float* __restrict__ out_loss,
               uint32_t* __restrict__ sat_row, uint32_t delta, int vec_out, unsigned long long* __restrict__ work,
               unsigned long long* __restrict__ diag, uint32_t claim, uint32_t idle_sleep,
               uint32_t lane_deg_max, const uint32_t* __restrict__ blk_rows,
               const uint32_t* __restrict__ ub_row, const uint32_t* __restrict__ ub_w,
               uint32_t* __restrict__ item_ctr, uint32_t n_items, uint32_t spin_max,
               const uint32_t* __restrict__ plan_ctl, int plan_ph, uint32_t* __restrict__ done,
               const SsspChainDesc* chain_desc, uint32_t* __restrict__ any_flag, int ident, uint32_t step_arcs,
               unsigned long long* __restrict__ popc, int early_on) {
  constexpr int NW = NT / 64;
  constexpr int AUX = FLAG ? SSSP_SC1 : 0;  // bound rows and the output: sc1 in the flagged launch
  // Chained rows: persistent workgroups, never the flagged launch.  The claim words and the maps
  // are read through the descriptor where they are used, from a copy of its address the compiler
  // cannot see through: as kernel arguments they stayed in registers across the whole search.
  if (FLAG || !item_ctr) chain_desc = nullptr;
  const bool chain_on = chain_desc != nullptr;
  auto chain_args = [&]() {
    const SsspChainDesc* d = chain_desc;
    asm volatile("" : "+s"(d));
    return d;
  };
  if (plan_ctl) {  // a device-built plan (sg_plan.hip): this phase's rows and bound rows, its row count
    const uint32_t base = plan_ctl[2 * plan_ph];
    n_items = plan_ctl[2 * plan_ph + 1];
    blk_rows += base;
    if (ub_row) {
      ub_row += (size_t)base * SSSP_KB;
      ub_w += (size_t)base * SSSP_KB;
    }
  }
  extern __shared__ __align__(16) unsigned char smem[];
  const uint32_t cap = sssp_ring_cap(n);
  const RingMod slot_of{cap, (uint32_t)(0x100000000ull / cap)};
  unsigned long long* key = (unsigned long long*)smem;
  uint32_t* off = (uint32_t*)(key + n);  // out_off staged in LDS (n + 1)
  uint16_t* ring = (uint16_t*)(smem + (size_t)n * 8 + (((size_t)n + 1) * 4 + 7) / 8 * 8);
  // counting build with SG_SSSP_DIAG (popc set): the workgroup's pops by class, behind the ring (cap is a
  // multiple of 64, so 8-byte aligned; the launch asks for SSSP_POP_WORDS more words of LDS)
  unsigned long long* s_popc = (unsigned long long*)(ring + cap);
  const bool pop_diag = COUNT && popc;
  __shared__ uint32_t ctl[8];  // TAIL
  constexpr int TAIL = 1;
  constexpr int E_DIRTY = 0, E_T0 = 3, E_POPS = 4, E_WAVES = 5, E_T4 = 6, E_T1 = 7;  // counting build: see the set-up
  // (head << 32) | busy in one word: a claim advances head and counts its wave
  // busy in one CAS, so a failed claim attempt never touches busy
  __shared__ unsigned long long hb;
  __shared__ uint8_t own[NW][64 * SSSP_K];
  __shared__ uint32_t red[NW];
  __shared__ unsigned long long sink[64];  // per-lane no-op target of offer_all
  __shared__ uint32_t s_ub[SSSP_KB][3];     // the row's usable bound rows: row, latency, exact
  __shared__ uint32_t s_nub;
  __shared__ uint32_t s_sat;  // FLAG: a wave saw a saturated key in the row's output
  if (FLAG && threadIdx.x == 0) s_sat = 0u;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // Every global read of the setup is a buffer load whose out-of-range lanes read
  // 0 without a branch, issued in groups so that a thread has a group's loads in
  // flight at once (one round trip per group, not per element).
  constexpr uint32_t OOB = 0x80000000u;
  {  // out_off staged in LDS, once per workgroup (a persistent one keeps it for all its rows)
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)out_off, 0, (int)((n + 1) * 4u),
                                                                        0x00020000);
    constexpr int GO = 12;  // entries per thread per group: one group up to 12,287 nodes
    for (uint32_t v0 = tid; v0 <= n; v0 += GO * NT) {
      uint32_t to[GO];
#pragma unroll
      for (int g = 0; g < GO; g++) {
        const uint32_t v = v0 + g * NT;
        to[g] = __builtin_amdgcn_raw_buffer_load_b32(ro, v <= n ? v * 4u : OOB, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < GO; g++)
        if (v0 + g * NT <= n) off[v0 + g * NT] = to[g];
    }
  }
  // Rows: one per workgroup, or (item_ctr set: persistent workgroups, one per
  // CU) claimed one after another from a counter the host zeroed
  // The next row is claimed while this one's output is written (its returning
  // atomic then overlaps the stores instead of starting the next row's setup);
  // give-ups happen only during a search, never with a claim outstanding.
  __shared__ uint32_t s_item;
  // Chained rows: s_chain = 1 (the row was claimed through an arc to the row just finished, whose
  // keys are still in key[]) | 2 (a zero-loss arc), s_cw the arc's latency; s_psat: the row just
  // finished had a saturated key in its output (it seeds bounds only)
  __shared__ uint32_t s_chain, s_cw, s_psat;
  // the next row of the list (one lane): with claim words, the next one whose word this
  // workgroup changes from 0 to 1 -- a row another workgroup chained to is skipped
  auto next_listed = [&]() -> uint32_t {
    uint32_t* claim_w = chain_on ? chain_args()->claim : nullptr;
    for (;;) {
      const uint32_t b = atomicAdd(item_ctr, 1u);
      if (!claim_w || b >= n_items) return b;
      const uint32_t r = blk_rows ? blk_rows[b] : row_begin + b;
      if (atomicCAS(&claim_w[r - row_begin], 0u, 1u) == 0u) return b;
    }
  };
  // The ring and own[] are reset here, once: a pop stores RING_EMPTY into its slot, and a search
  // that ended normally is quiescent (head == tail, no wave busy), so every slot written was
  // popped and the ring is all RING_EMPTY again; expand zeroes every own[] entry it reads, and
  // it reads every entry it wrote; a workgroup that gave up takes no further row.  (The row
  // loop's barriers order this ahead of the first search.)
  for (uint32_t i = tid; i < cap; i += NT) ring[i] = RING_EMPTY;
  for (int i = tid; i < NW * 64 * SSSP_K; i += NT) (&own[0][0])[i] = 0;
  if (pop_diag && tid < SSSP_POP_WORDS) s_popc[tid] = 0ull;
  if (item_ctr && tid == 0) {
    s_item = next_listed();
    s_chain = 0u;
    s_psat = 0u;
  }
  for (uint32_t it = 0;; it++) {
    uint32_t bi, chain = 0, chain_w = 0;
    if (item_ctr) {
      __syncthreads();  // s_item written (first row: above; later rows: in the previous row's output)
      bi = s_item;
      if (bi >= n_items) break;
      if (chain_on) {
        chain = s_chain;
        chain_w = s_cw;
        // exact seeds: a zero-loss arc, and the row in key[] a fixed point (no saturated key)
        if (chain > 1u && !(chain_args()->exact && !s_psat)) chain = 1u;
      }
    } else {
      if (it) break;
      bi = blockIdx.x;
      if (bi >= n_items) break;
    }
    // COUNT diagnostics of the first 4096 rows: cycle stamps, pops, bucket advances, relaxations
    const bool dg = COUNT && diag && bi < 4096 && tid == 0;
    const unsigned long long c_start = dg ? clock64() : 0;
    uint32_t n_adv = 0, n_pops = 0;
    unsigned long long cyc_claim = 0, cyc_pop = 0, cyc_steps = 0;  // per wave, COUNT diagnostics
    const uint32_t row = blk_rows ? blk_rows[bi] : row_begin + bi;
    const uint32_t src = ident ? row : used[row];  // (ident: the used list is the identity, column j is node j)
    // Setup.  Every global load of it is issued before the LDS pass, so the row pays one memory
    // round trip behind the bound-row listing instead of one per column group:
    //   1. the row's usable bound rows are listed (ub_row / ub_w, then their flags): for a
    //      persistent workgroup's later rows already at the claim, see list_bounds below;
    //   2. each thread issues its columns' node ids and the first two bound rows' latency and loss
    //      loads for its first GC columns (every column up to GC x NT = 10,240 of them);
    //   3. the keys become this row's start (infinity, or the chained rewrite) and ctl / hb are
    //      reset under those loads; a barrier, since with a used list other than the identity
    //      column j's node is another thread's to rewrite;
    //   4. the loads are merged into key[] with min, one bound row after the other (the map from a
    //      bound to its start key is monotone, so the min of the keys is the key of the min);
    //   5. columns past GC x NT and bound rows past the second (SG_SSSP_BOUNDS > 2, in pairs)
    //      take a load round each: the same loop, without the LDS pass.
    // An early row (see "Late seeds" in the header) runs step 3 alone here; steps 2, 4 and 5 are its
    // waves' way into the claim loop, under the search.
    // The ring and own[] are not reset: see the invariant ahead of the row loop.
    //
    // The usable bound rows of list place b, written to s_ub / s_nub by one whole wave: a row
    // whose search gave up (sat_row 2) was never written, so it gives no bounds; a saturated one
    // (1) holds real paths but not its optimum everywhere: bounds only.
    //   Phased launches: the flags are those of earlier launches, so they can be read at any
    // time.  A persistent workgroup's later rows are listed by the wave that claims them, ahead
    // of that wave's output stores (at the row's start the two dependent loads would wait behind
    // every wave's stores of the row before); s_ub is read during a set-up, or by an early
    // row's waves before they enter the claim loop, and the search's closing barrier separates that
    // from the claim.  A workgroup's first row is listed here by every wave for
    // itself (the same values into the same words), which waits for no other wave.
    //   Flagged launch: wave 0 polls here, at set-up time (an earlier poll would miss rows
    // published meanwhile), and alone: every column must see the same set of rows (the induction
    // of "Exact seeds" follows one bound row along a path).
    auto list_bounds = [&](uint32_t b) {
      const uint32_t e = lane < SSSP_KB ? ub_row[(size_t)b * SSSP_KB + lane] : ~0u;
      const uint32_t w = lane < SSSP_KB ? ub_w[(size_t)b * SSSP_KB + lane] : 0u;
      const uint32_t srow = e & ~SSSP_UB_EXACT;
      uint32_t sf;
      if constexpr (FLAG) {  // one sc1 poll per bound row, no wait: an unpublished row gives no bounds
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)done, 0, 0x7FFFFFFF, 0x00020000);
        const uint32_t dn = __builtin_amdgcn_raw_buffer_load_b32(rd, e != ~0u ? (srow - row_begin) * 4u : 0x80000000u,
                                                                 0, SSSP_SC1);
        sf = dn == 1u ? 0u : dn == 2u ? 1u : 2u;
      } else {
        sf = e != ~0u ? sat_row[srow - row_begin] : 2u;
      }
      const bool on = sf != 2u;
      const uint64_t mk = __ballot(on);
      if (on) {
        const int at = __popcll(mk & ((1ull << lane) - 1));
        s_ub[at][0] = srow;
        s_ub[at][1] = w;
        s_ub[at][2] = (e & SSSP_UB_EXACT) && sf == 0u;
      }
      if (lane == 0) s_nub = (uint32_t)__popcll(mk);
    };
    int nb = 0;
    if (ub_row && (FLAG ? tid < 64 : it == 0)) list_bounds(bi);
    if (ub_row) {
      if constexpr (FLAG) {
        __syncthreads();
      } else {  // this wave's own writes (or another's, the same values)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      nb = (int)s_nub;
    }
    unsigned long long c_list = 0, c_init = 0, c_bar = 0, c_g0 = 0;
    // the LDS pass: the keys become this row's start, ctl and hb are reset; then the barrier
    auto lds_pass = [&]() {
      if (dg) c_list = clock64();
      if (chain) {
        // Chained rows: key[] holds the finished row of a node this source has an arc to (latency
        // chain_w); every key becomes this row's start in place -- see the header
        const bool ex = (chain & 2u) != 0;
        for (uint32_t v = tid; v < n; v += NT) {
          const uint64_t kv = key[v];
          const uint64_t lw = (uint64_t)fkey_lat(kv) + chain_w;
          uint64_t nk = FKEY_INF;
          if (fkey_lat(kv) != LAT32_SAT && lw < LAT32_SAT - 1)
            nk = ex ? (lw << 32) | ((uint32_t)kv & ~1u) : ((lw + 1) << 32) | ((uint64_t)0x3F800000u << 1);
          key[v] = nk;
        }
        if (COUNT && tid == 0) {
          atomicAdd(&work[WORK_SHARDS], 1ull);
          if (ex) atomicAdd(&work[WORK_SHARDS + 1], 1ull);
        }
      } else {
        for (uint32_t v = tid; v < n; v += NT) key[v] = FKEY_INF;
      }
      if (tid < 8) ctl[tid] = 0;
      if (tid == 0) hb = 0;
      if (dg) c_init = clock64();
      __syncthreads();
      if (dg) c_bar = clock64();
    };
    // A bound-row pair's wave-uniform values, read into scalar registers (so the descriptors are scalar too)
    struct BoundPair {
      bool on[2], exact[2];
      uint32_t sr[2];
    };
    const __amdgpu_buffer_rsrc_t ru_set = __builtin_amdgcn_make_buffer_rsrc((void*)used, 0, (int)(n_used * 4u),
                                                                            0x00020000);
    // issue the loads of bound rows k, k + 1 for columns j0 + g * stride, g < GC
    auto bound_loads = [&](auto gc, int k, uint32_t j0, uint32_t stride, BoundPair& p, auto& l, auto& f, auto& vv) {
      constexpr int GC = decltype(gc)::value;
#pragma unroll
      for (int u = 0; u < 2; u++) {
        p.on[u] = k + u < nb;
        p.sr[u] = p.on[u] ? __builtin_amdgcn_readfirstlane(s_ub[k + u][0]) : 0u;
        p.exact[u] = p.on[u] && __builtin_amdgcn_readfirstlane(s_ub[k + u][2]);
        const size_t rb = p.on[u] ? (size_t)(p.sr[u] - out_row0) * n_used : 0;
        const __amdgpu_buffer_rsrc_t rl =
            __builtin_amdgcn_make_buffer_rsrc((void*)(out_lat + rb), 0, (int)(p.on[u] ? n_used * 8u : 0u), 0x00020000);
        const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(out_loss + rb), 0, (int)(p.exact[u] ? n_used * 4u : 0u), 0x00020000);
#pragma unroll
        for (int g = 0; g < GC; g++) {
          const uint32_t j = j0 + g * stride;
          const auto x = __builtin_amdgcn_raw_buffer_load_b64(rl, j < n_used ? j * 8u : OOB, 0, AUX);
          l[u][g] = ((uint64_t)x[1] << 32) | x[0];
          f[u][g] = __builtin_amdgcn_raw_buffer_load_b32(rf, j < n_used ? j * 4u : OOB, 0, AUX);
        }
      }
      if (!ident) {
#pragma unroll
        for (int g = 0; g < GC; g++) {
          const uint32_t j = j0 + g * stride;
          vv[g] = __builtin_amdgcn_raw_buffer_load_b32(ru_set, j < n_used ? j * 4u : OOB, 0, 0);
        }
      }
    };
    // column j's start key from the pair's rows: the smaller of their seeds, ~0 without one (the map from
    // a bound to its start key is monotone, so the min of the keys is the key of the min)
    auto bound_seed = [&](const BoundPair& p, const uint32_t* w, uint32_t j, uint64_t l0, uint64_t l1, uint32_t f0,
                          uint32_t f1) {
      uint64_t sd = ~0ull;
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const uint64_t ub = (u ? l1 : l0) + w[u];  // w < 2^32: a wrap means >= 2^64
        if (!p.on[u] || ub < w[u]) continue;
        if (ub < LAT32_SAT - 1) sd = min(sd, ((ub + 1) << 32) | ((uint64_t)0x3F800000u << 1));
        if (p.exact[u] && ub < LAT32_SAT && j != p.sr[u])  // exact: the path s -> s' then D[s'][v]
          sd = min(sd, (ub << 32) | ((uint64_t)(u ? f1 : f0) << 1));
      }
      return sd;
    };
    // Early rows (SG_SSSP_EARLY; see "Late seeds" in the header): a chained row with bound rows, not the
    // workgroup's first, starts its search behind the LDS pass; waves 1 .. NW - 1 load and merge the bound
    // rows, each on its way into the claim loop.
    const bool early = !FLAG && early_on && chain && nb > 0 && it > 0;
    if (!nb || early) {  // no bounds, or their loads issued under the search: the LDS pass alone
      lds_pass();
      if (COUNT && early && tid == 0) atomicAdd(&work[WORK_SSSP_EARLY], 1ull);
    } else {
      constexpr int GC = 10;  // columns per thread in flight (x 2 bound rows x 12 B)
      // load rounds: bound rows k, k + 1 for columns jb + tid + g NT, g < GC; the first round
      // carries the LDS pass between its loads and their merge
      int k = 0;
      uint32_t jb = 0;
      // (the column offsets come from an opaque copy of tid, per row: computed from tid itself they
      // are hoisted out of the row loop and kept, or spilled, across the whole search)
      uint32_t ts = (uint32_t)tid;
      asm volatile("" : "+v"(ts));
#pragma unroll 1
      do {
        const uint32_t j0 = jb + ts;
        uint32_t vv[GC];
        uint64_t l[2][GC];
        uint32_t f[2][GC];
        BoundPair p;
        bound_loads(std::integral_constant<int, GC>(), k, j0, (uint32_t)NT, p, l, f, vv);
        if (k == 0 && jb == 0) lds_pass();
        // one thread per column, so a plain read and write (a chained row's keys already hold its
        // first bound row, an earlier pair's its bounds: the smaller start wins)
        uint32_t w[2];
#pragma unroll
        for (int u = 0; u < 2; u++) w[u] = p.on[u] ? __builtin_amdgcn_readfirstlane(s_ub[k + u][1]) : 0u;
#pragma unroll
        for (int g = 0; g < GC; g++) {
          const uint32_t j = j0 + g * NT;
          if (j >= n_used) continue;
          const uint32_t v = ident ? j : vv[g];
          const uint64_t sd = bound_seed(p, w, j, l[0][g], l[1][g], f[0][g], f[1][g]);
          if (sd < key[v]) key[v] = sd;
        }
        if (dg && !c_g0) c_g0 = clock64();
        jb += GC * NT;
        if (jb >= n_used) {
          jb = 0;
          k += 2;
        }
      } while (k < nb);
    }
    if (ub_row && !early) __syncthreads();  // (an early row: the LDS pass's barrier)
    const unsigned long long c_setup = dg ? clock64() : 0;
    if (tid == 0) {
      key[src] = 1ull;  // PathProperties::default(), dirty and queued
      ring[0] = (uint16_t)src;
      ctl[TAIL] = 1;
      s_psat = 0u;  // (read by every thread before the set-up's barrier; set again in this row's output)
      // SG_SSSP_DIAG stamps shared by the waves, in ctl's free words (reset by the LDS pass): E_T0 the
      // search's start (clock, low word), E_POPS the row's wave-pops, E_WAVES the waves that held a
      // claim in its first 16k cycles, E_T4 / E_T1 the cycles to the fourth / first claim;
      // E_DIRTY (counting build) the merges that landed on a dirty key
      if (COUNT && diag) ctl[E_T0] = (uint32_t)clock64();
    }
    if (COUNT && diag && lane == 0) red[wv] = 0u;  // an early row: the cycles to the end of the wave's merge
    uint32_t split = delta;  // delta >= 1
    const __amdgpu_buffer_rsrc_t arcs = __builtin_amdgcn_make_buffer_rsrc((void*)out_arc, 0, (int)(n_arcs * 12u),
                                                                          0x00020000);
    uint32_t n_rel = 0;
    // a bound no correct search reaches (a bucket advance queues at least one
    // node, and a node is queued at most once per improvement); past it the row
    // is handed to the wide kernel instead of spinning
    const uint32_t max_adv = 4u * n + 64u;
    uint8_t* ow = own[wv];
    // spin budget per wave (sleeps of ~128 cycles): a safety valve against a
    // queue bug, never reached by a correct search; past it the wave leaves and
    // the row goes to the wide kernel
    uint32_t spins = 0;
    // Giving up (the safety valves below, never reached by a correct search):
    // the wave flags the row for the wide kernel, sets ctl[ABORT] and leaves the
    // kernel; every other wave of the workgroup leaves too, at its next claim or
    // after the quiescence barrier, so no wave waits at a barrier the others
    // will not reach, and a persistent workgroup takes no further rows (the
    // other workgroups claim them).
    constexpr int ABORT = 2;
    auto give_up = [&]() {
      if (lane == 0) {
        sat_row[row - row_begin] = 2u;  // never written: the wide kernel redoes it, and no search bounds by it
        *any_flag = 1u;                 // (host-visible: some row of the build was flagged)
        // the workgroup's first wave to give up counts it out; when every persistent
        // workgroup has given up (none left to claim the rest), the last one flags the
        // rows none claimed.  (A workgroup that ends normally has seen every row claimed.)
        if (atomicExch(&ctl[ABORT], 1u) == 0u && item_ctr) {
          __threadfence();
          if (atomicAdd(&item_ctr[1], 1u) == gridDim.x - 1) {
            const uint32_t c = __hip_atomic_load(&item_ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // (with claim words: only the rows no workgroup chained to -- a chained row is its
            // owner's to write or to flag)
            uint32_t* claim_w = chain_on ? chain_args()->claim : nullptr;
            for (uint32_t i = min(c, n_items); i < n_items; i++) {
              const uint32_t r = (blk_rows ? blk_rows[i] : row_begin + i) - row_begin;
              if (!claim_w || __hip_atomic_load(&claim_w[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
                sat_row[r] = 2u;
            }
          }
        }
      }
    };
    auto ld = [](uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    // relax NK candidates into key[v[c]]; app[c]: the ballot of the lanes whose v[c] became dirty below split (to
    // be queued).  Branch-free, so the NK LDS atomics issue back to back and share
    // one wait: a lane with no candidate (or a saturated one, never propagated)
    // offers ~0 to its own sink word, a no-op.  (With one branch per candidate the
    // compiler waited for each atomic's return before issuing the next.)
    auto offer_all = [&](auto nk, const bool* valid, const uint32_t* v, const uint64_t* cand, uint64_t* app) {
      constexpr int NK = decltype(nk)::value;
      uint64_t cd[NK], old[NK];
      bool okk[NK];
#pragma unroll
      for (int c = 0; c < NK; c++) {
        const bool ok = valid[c] && fkey_lat(cand[c]) != LAT32_SAT;
        okk[c] = ok;
        // (no select of the offered value: a lane without a candidate offers whatever it holds
        // to its own sink word, whose value nothing reads)
        cd[c] = cand[c];
        old[c] = __hip_atomic_fetch_min(ok ? &key[v[c]] : &sink[lane], (unsigned long long)cd[c], __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      // keep the scheduler from pulling a use of old[] between the atomics
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < NK; c++)
        // improved and was clean: a clean old key (flag 0) is above the candidate (flag 1) iff its
        // (latency, loss) is larger -- one 64-bit compare, no shifts
        // (the i1 ballot: the condition's lane mask as is, not a 0/1 VGPR compared back to a mask)
        app[c] = __builtin_amdgcn_ballot_w64(okk[c] && !((uint32_t)old[c] & 1u) && old[c] > cd[c] &&
                                             fkey_lat(cd[c]) < split);
    };
    __syncthreads();

    if (early && wv != 0) {
      // An early row's bound rows, under the search wave 0 has begun: the columns spread over the
      // other waves (GE per thread and round: one round up to 10,560 columns), every bound-row pair
      // loaded and merged before the wave enters the claim loop.  The search runs, so the merge is
      // a compare-and-swap that keeps the dirty bit (see "Late seeds").
      constexpr int GE = 11;
      constexpr uint32_t NM = NT - 64;
      uint32_t ts = (uint32_t)tid - 64u;
      asm volatile("" : "+v"(ts));  // (opaque, per row: see the set-up's load rounds)
      int k = 0;
      uint32_t jb = 0;
#pragma unroll 1
      do {
        const uint32_t j0 = jb + ts;
        uint32_t vv[GE];
        uint64_t l[2][GE];
        uint32_t f[2][GE];
        BoundPair p;
        bound_loads(std::integral_constant<int, GE>(), k, j0, NM, p, l, f, vv);
        uint32_t w[2];
#pragma unroll
        for (int u = 0; u < 2; u++) w[u] = p.on[u] ? __builtin_amdgcn_readfirstlane(s_ub[k + u][1]) : 0u;
#pragma unroll
        for (int g = 0; g < GE; g++) {
          const uint32_t j = j0 + g * NM;
          if (j >= n_used) continue;
          const uint32_t v = ident ? j : vv[g];
          const uint64_t sd = bound_seed(p, w, j, l[0][g], l[1][g], f[0][g], f[1][g]);
          unsigned long long old = __hip_atomic_load(&key[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          while (sd < (old & ~1ull)) {
            const unsigned long long prev = atomicCAS(&key[v], old, sd | (old & 1ull));
            if (prev == old) {
              if (COUNT && (old & 1ull)) atomicAdd(&ctl[E_DIRTY], 1u);
              break;
            }
            old = prev;
          }
        }
        jb += GE * NM;
        if (jb >= n_used) {
          jb = 0;
          k += 2;
        }
      } while (k < nb);
      if (COUNT && diag && lane == 0) red[wv] = (uint32_t)clock64() - ctl[E_T0];
    }

    for (;;) {
      // ---- claim up to `claim` queued entries
      const unsigned long long tc0 = (COUNT && diag) ? clock64() : 0;
      uint32_t h = 0, k = 0;
      if (lane == 0) {
        for (;;) {
          const unsigned long long w = __hip_atomic_load(&hb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          const uint32_t hh = (uint32_t)(w >> 32), t = ld(&ctl[TAIL]);
          if (t == hh) break;
          const uint32_t kk = min(claim, t - hh);
          const unsigned long long nw = ((unsigned long long)(hh + kk) << 32) | ((w & 0xFFFFFFFFull) + 1);
          if (atomicCAS(&hb, w, nw) == w) {
            h = hh;
            k = kk;
            break;
          }
        }
      }
      h = __builtin_amdgcn_readfirstlane(h);
      k = __builtin_amdgcn_readfirstlane(k);
      if (__builtin_amdgcn_readfirstlane(ld(&ctl[ABORT]))) goto wave_exit;  // another wave gave up
      if (!k) {
        uint32_t q = 0;
        if (lane == 0) {
          const unsigned long long w = __hip_atomic_load(&hb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __atomic_signal_fence(__ATOMIC_SEQ_CST);  // (head, busy) before tail (see header)
          q = (w & 0xFFFFFFFFull) == 0 && (uint32_t)(w >> 32) == ld(&ctl[TAIL]);
        }
        if (!__builtin_amdgcn_readfirstlane(q)) {
          if (++spins > spin_max) {
            give_up();
            goto wave_exit;
          }
          for (uint32_t z = 0; z < idle_sleep; z++) __builtin_amdgcn_s_sleep(8);  // ~512 cycles each
          __builtin_amdgcn_s_sleep(2);
          continue;
        }
        // ---- quiescent: every wave is here.  Next bucket, or done.
        __syncthreads();
        if (ld(&ctl[ABORT])) goto wave_exit;  // a wave gave up before this barrier (uniform: no wave is spinning now)
        // one bucket (split = LAT32_SAT, the default): every node that became dirty was
        // queued, so a quiescent queue means nothing is dirty -- no key scan needed
        if (split >= LAT32_SAT) break;
        uint32_t m = LAT32_SAT;
        for (uint32_t v = tid; v < n; v += NT) {
          const uint64_t kv = key[v];
          if (kv & 1ull) m = min(m, fkey_lat(kv));
        }
        for (int d = 32; d > 0; d >>= 1) m = min(m, (uint32_t)__shfl_xor(m, d));
        if (lane == 0) red[wv] = m;
        __syncthreads();
        m = red[0];
        for (int w = 1; w < NW; w++) m = min(m, red[w]);
        if (m == LAT32_SAT) break;  // nothing dirty (saturated keys are never marked dirty)
        if (++n_adv > max_adv) {  // every wave is here together
          give_up();
          goto wave_exit;
        }
        split = m + delta >= m ? min(m + delta, LAT32_SAT) : LAT32_SAT;
        for (uint32_t v0 = wv * 64; v0 < n; v0 += NT) {  // queue the dirty nodes below split
          const uint32_t v = v0 + lane;
          uint64_t kv = v < n ? key[v] : 0ull;
          const bool q2 = (kv & 1ull) && fkey_lat(kv) < split;
          const uint64_t m2 = __ballot(q2);
          append_q<1>(&m2, &v, ring, &ctl[TAIL], slot_of, lane);
        }
        __syncthreads();
        continue;
      }
      if (COUNT) n_pops++;
      const unsigned long long tc1 = (COUNT && diag) ? clock64() : 0;
      if (COUNT && diag && lane == 0) {  // how the search begins: see E_T0
        const uint32_t dt = (uint32_t)tc1 - ctl[E_T0], np = atomicAdd(&ctl[E_POPS], 1u);
        if (np == 0u) ctl[E_T1] = dt;
        if (np == 3u) ctl[E_T4] = dt;
        if (dt < 16384u) atomicOr(&ctl[E_WAVES], 1u << wv);
      }
      // ---- pop the claimed entries (a slot claimed before its writer stored it reads EMPTY)
      const bool on = lane < (int)k;
      uint32_t u = 0, a0 = 0, a1 = 0;
      uint64_t ku = 0;
      bool stuck = false;
      if (on) {
        // (relaxed workgroup-scope accesses, so the slot is read and written as LDS: through a
        // volatile pointer both were flat operations, the store with a wait for it behind it)
        uint16_t* slot = &ring[slot_of(h + lane)];
        uint16_t x;
        uint32_t sp = 0;
        while ((x = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == RING_EMPTY &&
               ++sp < spin_max)
          __builtin_amdgcn_s_sleep(0);
        stuck = x == RING_EMPTY;
        __hip_atomic_store(slot, RING_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        u = stuck ? src : x;
        a0 = off[u];
        a1 = off[u + 1];
        // clear the dirty flag; the returned key is the one to relax with (see header)
        ku = __hip_atomic_fetch_and(&key[u], ~1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & ~1ull;
      }
      if (__any(stuck)) {
        give_up();
        goto wave_exit;
      }
      const uint32_t deg = a1 - a0;
      // the pop's arcs: the scan the arc-parallel step needs anyway, taken once
      const uint32_t deg_incl = wave_incl_sum(deg);
      const uint32_t T = __builtin_amdgcn_readlane(deg_incl, 63);
      const unsigned long long tc2 = (COUNT && (diag || pop_diag)) ? clock64() : 0;
      // arcs [ea0, ea0 + edeg) of each lane's node, arc-parallel: the wave's arcs in consecutive
      // slots, KX chunks of 64 at once (owner lane by scatter + max-scan)
      // (incl: the inclusive scan of edeg over the wave)
      auto expand = [&](auto kx, uint32_t ea0, uint32_t edeg, uint32_t incl) {
        constexpr int KX = decltype(kx)::value;
        const uint32_t base = incl - edeg;
        const uint32_t T = __builtin_amdgcn_readlane(incl, 63);
        if (COUNT) n_rel += T;
        uint32_t carry = 0;  // 1 + the owner lane of the previous slot
        for (uint32_t t0 = 0; t0 < T; t0 += 64 * KX) {
          // owner lane of each slot: heads scatter 1 + their lane at their first slot, a max-scan fills the rest
          if (edeg && base >= t0 && base - t0 < 64u * KX) ow[base - t0] = (uint8_t)(lane + 1);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          uint32_t v[KX], lat[KX], om[KX], o[KX];
          bool valid[KX];
          uint64_t app[KX];
#pragma unroll
          for (int c = 0; c < KX; c++) {
            const uint32_t hd = ow[c * 64 + lane];
            ow[c * 64 + lane] = 0;
            const uint32_t mx = max(wave_incl_max(hd), carry);
            carry = __builtin_amdgcn_readlane(mx, 63);
            o[c] = mx - 1;
          }
#pragma unroll
          for (int c = 0; c < KX; c++) {
            const uint32_t sl = t0 + c * 64 + lane;
            valid[c] = sl < T;
            const uint32_t a = __shfl(ea0, (int)o[c]) + sl - __shfl(base, (int)o[c]);
            const auto r = __builtin_amdgcn_raw_buffer_load_b96(arcs, valid[c] ? a * 12u : 0x80000000u, 0, 0);
            v[c] = r[0];
            lat[c] = r[1];
            om[c] = r[2];
          }
          uint64_t cand[KX];
#pragma unroll
          for (int c = 0; c < KX; c++) {
            const uint32_t klo = __shfl((uint32_t)ku, (int)o[c]), khi = __shfl((uint32_t)(ku >> 32), (int)o[c]);
            cand[c] = frelax(((uint64_t)khi << 32) | klo, lat[c], __uint_as_float(om[c]));
          }
          offer_all(std::integral_constant<int, KX>(), valid, v, cand, app);
          append_q<KX>(app, v, ring, &ctl[TAIL], slot_of, lane);
        }
      };
      // ---- the step follows the arcs: a pop of at most step_arcs arcs goes arc-parallel whatever its
      // entries' degrees, in ceil(T / 64) slots per lane (1, 2, or rounds of SSSP_K) where the lane path
      // issues LA slots and its overflow round for every pop.  (A pop without arcs relaxes nothing.)
      const bool small = T <= step_arcs;
      // (the largest degree is only ever compared: a ballot each, no second scan)
      if (small && T <= 64u) {
        expand(std::integral_constant<int, 1>(), a0, deg, deg_incl);
      } else if (small && T <= 128u) {
        expand(std::integral_constant<int, 2>(), a0, deg, deg_incl);
      } else if (small || __builtin_amdgcn_ballot_w64(deg > lane_deg_max)) {
        // ---- expansion path (a small pop past 128 arcs, or a high out-degree): arcs of the 64 entries in
        // consecutive slots
        expand(std::integral_constant<int, SSSP_K>(), a0, deg, deg_incl);
      } else {
        // ---- lane path: each lane walks its node's first LA arcs (LA loads in flight); the arcs
        // past them (nodes of degree > LA only) go arc-parallel like the expansion path.  At C3
        // (mean degree 8, a wave's largest ~14) a second round of LA slots per lane was mostly
        // idle lanes: 3.10 -> 2.83 ms (profiles/r05/ab_sssp_hybrid_r6x.txt)
        if (COUNT) n_rel += __builtin_amdgcn_readlane(wave_incl_sum(min(deg, (uint32_t)LA)), 63);
        if (pop_diag && lane == 0) atomicAdd(&s_popc[3 * SSSP_POP_CLASSES], 1ull);
        {
          constexpr uint32_t j0 = 0;
          uint32_t v[LA], lat[LA], om[LA];
          bool valid[LA];
          uint64_t app[LA];
#pragma unroll
          for (int c = 0; c < LA; c++) {
            valid[c] = j0 + c < deg;
            const auto r = __builtin_amdgcn_raw_buffer_load_b96(arcs, valid[c] ? (a0 + j0 + c) * 12u : 0x80000000u,
                                                                0, 0);
            v[c] = r[0];
            lat[c] = r[1];
            om[c] = r[2];
          }
          uint64_t cand[LA];
#pragma unroll
          for (int c = 0; c < LA; c++) cand[c] = frelax(ku, lat[c], __uint_as_float(om[c]));
          offer_all(std::integral_constant<int, LA>(), valid, v, cand, app);
          append_q<LA>(app, v, ring, &ctl[TAIL], slot_of, lane);
        }
        if (__builtin_amdgcn_ballot_w64(deg > (uint32_t)LA)) {  // the arcs past each node's first LA, arc-parallel
          const uint32_t rest = deg > (uint32_t)LA ? deg - LA : 0u;
          expand(std::integral_constant<int, 1>(), a0 + LA, rest, wave_incl_sum(rest));
        }
      }
      // release the claim after this wave's appends (LDS keeps a wave's operations in order)
      if (lane == 0) atomicSub(&hb, 1ull);
      if (COUNT && (diag || pop_diag)) {
        const unsigned long long tc3 = clock64();
        if (diag) {
          cyc_claim += tc1 - tc0;
          cyc_pop += tc2 - tc1;
          cyc_steps += tc3 - tc2;
        }
        if (pop_diag && lane == 0) {  // the pop's class by S = ceil(T / 64): pops, arcs, step cycles
          const uint32_t S = (T + 63u) / 64u;
          const int cls = S <= 2u ? (int)S : S <= 4u ? 3 : S <= 8u ? 4 : 5;
          atomicAdd(&s_popc[3 * cls], 1ull);
          atomicAdd(&s_popc[3 * cls + 1], (unsigned long long)T);
          atomicAdd(&s_popc[3 * cls + 2], tc3 - tc2);
        }
      }
    }
    if (COUNT && lane == 0 && n_rel) atomicAdd(&work[bi & 63], (unsigned long long)n_rel);
    if (COUNT && diag && bi < 4096 && lane == 0) {
      if (n_rel) atomicAdd(&diag[bi * SSSP_DIAG_WORDS + 4], (unsigned long long)n_rel);
      if (n_pops) atomicAdd(&diag[bi * SSSP_DIAG_WORDS + 2], (unsigned long long)n_pops);
      atomicAdd(&diag[bi * SSSP_DIAG_WORDS + 5], cyc_claim);
      atomicAdd(&diag[bi * SSSP_DIAG_WORDS + 6], cyc_pop);
      atomicAdd(&diag[bi * SSSP_DIAG_WORDS + 7], cyc_steps);
    }
    const unsigned long long c_search = dg ? clock64() : 0;
    if (COUNT) {  // the ring invariant: slots a finished search left non-empty (0), rows looked at
      uint32_t left = 0;
      for (uint32_t i = tid; i < cap; i += NT) left += ring[i] != RING_EMPTY;
      if (left) atomicAdd(&work[WORK_SHARDS + 2], (unsigned long long)left);
      if (tid == 0) atomicAdd(&work[WORK_SHARDS + 3], 1ull);
      if (tid == 0 && early && ctl[E_DIRTY]) atomicAdd(&work[WORK_SSSP_EARLY + 1], (unsigned long long)ctl[E_DIRTY]);
    }

    // ---- write the row: columns in used order, diagonal = the raw self-loop (graph/mod.rs:210-217)
    __syncthreads();  // every thread has read s_item (at the row's start) before it is written again
    if (pop_diag) {  // (no wave is in a step: the row's classes move to the launch's counters)
      if (tid < SSSP_POP_WORDS - 1 && s_popc[tid]) {
        atomicAdd(&popc[tid], s_popc[tid]);
        s_popc[tid] = 0ull;
      }
      if (lane == 0 && n_pops) atomicAdd(&popc[SSSP_POP_WORDS - 1], (unsigned long long)n_pops);
    }
    if (item_ctr && !chain_on) {
      if (wv == 0) {  // the next row (see the row loop), and its bound rows (see list_bounds)
        uint32_t ni = 0;
        if (lane == 0) s_item = ni = atomicAdd(item_ctr, 1u);
        if (!FLAG && ub_row) {
          ni = __builtin_amdgcn_readfirstlane(ni);
          if (ni < n_items) list_bounds(ni);
        }
      }
    } else if (item_ctr && wv == NW - 1) {
      // Chained rows: one wave looks for the next row among the heads of this source's out-arcs
      // (up to 64, one per lane): a row of the block, of this launch's phase, not yet claimed;
      // zero-loss arcs first, then by latency, then by row.  The loop tries one claim per
      // candidate row at most and waits for nothing another workgroup does.  Four dependent
      // round trips (arc, rel, {phase, claim word, list place}, the claim) ahead of this wave's
      // share of the output, so the last wave takes it: its share is the smallest.
      uint32_t ll = (uint32_t)lane;  // an opaque copy: nothing here is kept across the search
      asm volatile("" : "+v"(ll));
      const SsspChainDesc* cd = chain_args();
      uint32_t* claim_w = cd->claim;
      const uint32_t* rel = cd->rel;
      const uint8_t* phase_of = cd->phase_of;
      const uint32_t* list_pos = cd->pos;
      const uint32_t a0 = off[src], nd = min(off[src + 1] - a0, 64u);
      const bool in = ll < nd;
      const auto r = __builtin_amdgcn_raw_buffer_load_b96(arcs, in ? (a0 + ll) * 12u : OOB, 0, 0);
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)rel, 0, (int)(n * 4u), 0x00020000);
      const uint32_t q = __builtin_amdgcn_raw_buffer_load_b32(rr, in ? r[0] * 4u : OOB, 0, 0);
      bool ok = in && q != ~0u;
      if (const uint32_t vr = cd->check_rows) {  // rel holds anything outside the block's rows: map q back
        const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)used, 0, (int)(n_used * 4u), 0x00020000);
        ok = ok && q < vr;
        const uint32_t back = __builtin_amdgcn_raw_buffer_load_b32(ru, ok ? (row_begin + q) * 4u : OOB, 0, 0);
        ok = ok && back == r[0];
      }
      // (branch-free, in flight together; the claim word past this XCD's L2, which may hold it stale)
      const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)phase_of, 0, phase_of ? 0x7FFFFFFF : 0, 0x00020000);
      const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)claim_w, 0, 0x7FFFFFFF, 0x00020000);
      const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc((void*)list_pos, 0, list_pos ? 0x7FFFFFFF : 0, 0x00020000);
      const uint32_t q_ph = __builtin_amdgcn_raw_buffer_load_b8(rp, ok ? q : OOB, 0, 0);
      const uint32_t q_cl = __builtin_amdgcn_raw_buffer_load_b32(rc, ok ? q * 4u : OOB, 0, SSSP_SC1);
      const uint32_t q_at = __builtin_amdgcn_raw_buffer_load_b32(rl, ok ? q * 4u : OOB, 0, 0);
      const uint32_t base = list_pos ? plan_ctl[2 * plan_ph] : 0u;
      ok = ok && q_cl == 0u && (!phase_of || q_ph == (uint32_t)plan_ph);
      // (zero-loss arcs rank first) | latency | row: the smallest is the best
      uint64_t sc = ok ? ((uint64_t)(r[2] != 0x3F800000u) << 63) | ((uint64_t)r[1] << 31) | q : ~0ull;
      uint32_t got = 0, nb = ~0u, cf = 0, cw = 0;
      for (;;) {
        uint64_t m = sc;
        for (int d = 32; d > 0; d >>= 1) m = min(m, (uint64_t)__shfl_xor((unsigned long long)m, d));
        if (m == ~0ull) break;
        const uint32_t mq = (uint32_t)m & 0x7FFFFFFFu;
        const int win = __ffsll((long long)__ballot(sc == m)) - 1;  // parallel arcs can tie
        uint32_t old = 1u;
        if ((int)ll == win) old = atomicCAS(&claim_w[mq], 0u, 1u);
        old = __shfl(old, win);
        if (old == 0u) {
          got = 1u;
          cf = 1u | ((m >> 63) ? 0u : 2u);
          cw = (uint32_t)(m >> 31);
          nb = list_pos ? __shfl(q_at, win) - base : mq;  // (a plan's list: its place in this phase)
          break;
        }
        if (ok && q == mq) sc = ~0ull;  // claimed by another workgroup: every arc to it drops out
      }
      uint32_t ni = 0;
      if (lane == 0) {
        s_item = ni = got ? nb : next_listed();
        s_chain = cf;
        s_cw = cw;
      }
      if (ub_row) {  // the claimed row's bound rows (see list_bounds)
        ni = __builtin_amdgcn_readfirstlane(ni);
        if (ni < n_items) list_bounds(ni);
      }
    }
    const size_t orow = (size_t)(row - out_row0) * n_used;
    bool sat = false;
    // the row's output: nontemporal 16-B stores; in the flagged launch sc1 (write-through) stores,
    // which the later rows' sc1 loads read across XCDs (MI355X_MICROARCH.md hand-off protocol)
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t wl = __builtin_amdgcn_make_buffer_rsrc((void*)(out_lat + orow), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t wf = __builtin_amdgcn_make_buffer_rsrc((void*)(out_loss + orow), 0, 0x7FFFFFFF, 0x00020000);
    auto st_lat2 = [&](uint32_t j, uint64_t a, uint64_t b) {
      if constexpr (FLAG) {
        typedef uint32_t v4 __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_raw_buffer_store_b128((v4){(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)},
                                               wl, j * 8u, 0, SSSP_SC1);
      } else {
        __builtin_nontemporal_store((u64x2){a, b}, (u64x2*)&out_lat[orow + j]);
      }
    };
    auto st_loss4 = [&](uint32_t j, float a, float b, float c, float d) {
      if constexpr (FLAG) {
        typedef uint32_t v4 __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_raw_buffer_store_b128((v4){__float_as_uint(a), __float_as_uint(b), __float_as_uint(c),
                                                    __float_as_uint(d)}, wf, j * 4u, 0, SSSP_SC1);
      } else {
        __builtin_nontemporal_store((f32x4){a, b, c, d}, (f32x4*)&out_loss[orow + j]);
      }
    };
    auto entry = [&](uint32_t j, uint64_t& l, float& f) {
      if (j == row) {
        const uint32_t e = self_edge[ident ? j : used[j]];
        l = e_lat[e];
        f = e_loss[e];
      } else {
        const uint64_t kk = key[ident ? j : used[j]];
        sat |= fkey_lat(kk) == LAT32_SAT;
        l = fkey_lat(kk);
        f = __uint_as_float(fkey_loss_bits(kk));
      }
    };
    if (vec_out) {  // n_used % 4 == 0, 16-B aligned rows: 16-B stores
      // Every global read of the output comes before its first store: the columns'
      // node ids (16-B loads, OU per thread) and the diagonal's raw self-loop.  (Read
      // inside the loop, each one waited behind the thread's earlier stores, since the
      // vector-memory counter covers both.)
      constexpr int OU = 4;
      const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)used, 0, (int)(n_used * 4u),
                                                                          0x00020000);
      // the column indices are computed here, per row, from an opaque copy of tid: hoisted
      // out of the row loop, the compiler kept (and spilled) them across the whole search
      uint32_t tt = (uint32_t)tid;
      asm volatile("" : "+v"(tt));
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      u32x4 uv[OU];
#pragma unroll
      for (int k = 0; k < OU; k++) {
        const uint32_t j = (tt + (uint32_t)k * NT) * 4;
        if (ident) uv[k] = (u32x4){j, j + 1, j + 2, j + 3};
        else uv[k] = __builtin_amdgcn_raw_buffer_load_b128(ru, j < n_used ? j * 4u : OOB, 0, 0);
      }
      const uint32_t de = self_edge[src];
      const uint64_t d_lat = e_lat[de];
      const float d_loss = e_loss[de];
      auto cell = [&](uint32_t j, uint32_t vj, uint64_t& l, float& f) {
        const uint64_t kk = key[vj];
        const bool diag = j == row;
        sat |= !diag && fkey_lat(kk) == LAT32_SAT;
        l = diag ? d_lat : (uint64_t)fkey_lat(kk);
        f = diag ? d_loss : __uint_as_float(fkey_loss_bits(kk));
      };
#pragma unroll
      for (int k = 0; k < OU; k++) {
        const uint32_t j = (tt + (uint32_t)k * NT) * 4;
        if (j < n_used) {
          uint64_t l0, l1, l2, l3;
          float f0, f1, f2, f3;
          cell(j, uv[k][0], l0, f0);
          cell(j + 1, uv[k][1], l1, f1);
          cell(j + 2, uv[k][2], l2, f2);
          cell(j + 3, uv[k][3], l3, f3);
          st_lat2(j, l0, l1);
          st_lat2(j + 2, l2, l3);
          st_loss4(j, f0, f1, f2, f3);
        }
      }
      for (uint32_t j = (tt + OU * NT) * 4; j < n_used; j += NT * 4) {  // past OU x NT x 4 columns
        uint64_t l0, l1, l2, l3;
        float f0, f1, f2, f3;
        entry(j, l0, f0);
        entry(j + 1, l1, f1);
        entry(j + 2, l2, f2);
        entry(j + 3, l3, f3);
        st_lat2(j, l0, l1);
        st_lat2(j + 2, l2, l3);
        st_loss4(j, f0, f1, f2, f3);
      }
    } else {
      for (uint32_t j = tid; j < n_used; j += NT) {
        uint64_t l;
        float f;
        entry(j, l, f);
        if constexpr (FLAG) {
          __builtin_amdgcn_raw_buffer_store_b64((uint32_t __attribute__((ext_vector_type(2)))){(uint32_t)l,
                                                                                              (uint32_t)(l >> 32)},
                                                wl, j * 8u, 0, SSSP_SC1);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(f), wf, j * 4u, 0, SSSP_SC1);
        } else {
          out_lat[orow + j] = l;
          out_loss[orow + j] = f;
        }
      }
    }
    if (__any(sat) && lane == 0) {
      sat_row[row - row_begin] = 1u;
      *any_flag = 1u;
      if (FLAG) s_sat = 1u;
      if (chain_on) s_psat = 1u;
    }
    if (dg) {
      diag[bi * SSSP_DIAG_WORDS + 0] = c_search - c_start;
      diag[bi * SSSP_DIAG_WORDS + 1] = clock64() - c_search;
      // bucket advances (< 2^22) | chained, exact (bits 22, 23) | setup cycles
      diag[bi * SSSP_DIAG_WORDS + 3] = n_adv | ((unsigned long long)chain << 22) | ((c_setup - c_start) << 24);
      // the set-up's parts: the listing up to the loads' issue, the LDS pass, the barrier, the
      // first load round's wait and merge, the later rounds with the closing barrier
      diag[bi * SSSP_DIAG_WORDS + 8] = c_init - c_list;
      diag[bi * SSSP_DIAG_WORDS + 9] = c_list - c_start;
      diag[bi * SSSP_DIAG_WORDS + 10] = c_bar - c_list;
      diag[bi * SSSP_DIAG_WORDS + 11] = early ? 0ull : c_g0 - c_bar;
      diag[bi * SSSP_DIAG_WORDS + 12] = early ? 0ull : c_setup - c_g0;
      // how the search began, from its start behind the set-up (E_T0): cycles to the fourth claim | waves
      // that held a claim in the first 16k cycles; cycles to the first claim | an early row's cycles to the
      // end of its last wave's merge (overwritten by a bucket advance: one bucket only); an early row's
      // merges onto dirty keys | early
      uint32_t last_merge = 0;
      for (int w = 1; w < NW; w++) last_merge = max(last_merge, red[w]);
      diag[bi * SSSP_DIAG_WORDS + 13] = ctl[E_T4] | ((unsigned long long)__popc(ctl[E_WAVES]) << 32);
      diag[bi * SSSP_DIAG_WORDS + 14] = ctl[E_T1] | ((unsigned long long)(early ? last_merge : 0u) << 32);
      diag[bi * SSSP_DIAG_WORDS + 15] = ctl[E_DIRTY] | ((unsigned long long)early << 32);
    }
    if constexpr (FLAG) {
      // Flagged rows: every wave waits for its sc1 stores, then one lane publishes the row
      // (sc1 flag store behind the barrier: MI355X_MICROARCH.md hand-off table, first row)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)done, 0, 0x7FFFFFFF, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(s_sat ? 2u : 1u, rd, (row - row_begin) * 4u, 0, SSSP_SC1);
        s_sat = 0u;
      }
    }
    __syncthreads();  // the next row reuses the LDS
  }
wave_exit:;
  // (An earlier version counted every wave out with one device atomic at exit: 4,096
  // atomics on one word at the end of each launch cost ~0.1 ms.)
}

bool sssp_lds_fits(uint32_t n) {
  if (n == 0 || n >= RING_EMPTY) return false;  // u16 queue entries
  return sssp_lds_bytes(n) + SSSP_STATIC_LDS <= LDS_PER_CU;
}

struct SsspKnobs {
  uint32_t claim;       // SG_SSSP_CLAIM: entries a wave claims at once (1..64)
  uint32_t idle_sleep;  // SG_SSSP_SLEEP: idle back-off, units of ~512 cycles
  // SG_SSSP_LANE_DEG (with the remainder arc-parallel, every wave takes the lane path unless
  // it is lowered: C3 2.83 ms at 16, 2.79 at 24 and 64)
  uint32_t lane_deg;
  // One persistent workgroup per CU claims rows from a counter: out_off is
  // staged once per CU instead of once per row, and no workgroup is launched and
  // torn down per row.  C3: 3.92 -> 3.54 ms (same box).  SG_SSSP_PERSIST=0: a
  // workgroup per row.
  bool persist;
  // spin budget per wave (sleeps of ~128 cycles): a safety valve against a queue
  // bug, never reached by a correct search; SG_SSSP_SPIN_MAX (tests) lowers it so
  // that searches give up and their rows take the wide kernel
  uint32_t spin_max;
  // SG_SSSP_STEP_ARCS: a pop of at most this many arcs takes the arc-parallel step sized to them
  // (0: the lane path unless an entry's degree is past lane_deg)
  uint32_t step_arcs;
  // SG_SSSP_EARLY: a chained row with bound rows starts its search behind the LDS pass, the bound rows
  // loaded and merged under it ("Late seeds"); 0: every row's set-up ends before its search begins
  bool early;
};
static SsspKnobs sssp_knobs() {
  SsspKnobs k;
  k.claim = (uint32_t)knob_int("SG_SSSP_CLAIM", 64, 1, 64);
  k.idle_sleep = (uint32_t)std::max(0, knob_int("SG_SSSP_SLEEP", 0));
  k.lane_deg = (uint32_t)std::max(0, knob_int("SG_SSSP_LANE_DEG", 64));
  k.persist = !knob_off("SG_SSSP_PERSIST");
  k.spin_max = sssp_spin_max();
  k.step_arcs = (uint32_t)std::max(0, knob_int("SG_SSSP_STEP_ARCS", 256));
  k.early = knob_int("SG_SSSP_EARLY", 1) != 0;
  return k;
}

void launch_sssp_lds(sg_ctx* ctx, const sg_net* net, const SsspLdsLaunch& l) {
  const SsspKnobs k = sssp_knobs();
  const uint32_t n = net->n_nodes;
  size_t lds = sssp_lds_bytes(n);
  if (!sssp_lds_fits(n)) throw Error(SG_ERR_INVALID_ARG, "graph too large for the LDS-resident search");
  if ((uint64_t)net->n_arcs * 12 >= (1ull << 31)) throw Error(SG_ERR_INVALID_ARG, "too many arcs for 32-bit offsets");
  const int vec = l.n_used % 4 == 0 && ((uintptr_t)l.out_lat & 15) == 0 && ((uintptr_t)l.out_loss & 15) == 0;
  // with a device plan (plan_ctl), n_blk bounds the phase's row count, which only the device knows
  const uint32_t rows = l.blk_rows ? l.n_blk : l.row_end - l.row_begin;
  if (!rows) return;
  const bool persist = l.done || (k.persist && (rows > (uint32_t)ctx->n_cu || l.plan_ctl));
  // [claims, waves done] (sg_sssp.hip wave_exit); a device plan's counters are zeroed by the plan kernel
  uint32_t* item_ctr = nullptr;
  if (persist && l.plan_ctr) {
    item_ctr = l.plan_ctr;
  } else if (persist) {
    item_ctr = ctx->r_items.get<uint32_t>(2);
    SG_HIP(hipMemsetAsync(item_ctr, 0, 8, ctx->stream));
  }
  const uint32_t grid = persist ? (uint32_t)ctx->n_cu : rows;
  // Chained rows: persistent workgroups on an undirected graph (the arc t -> s mirrors s -> t),
  // never the flagged launch (the caller passes claim words only with SG_SSSP_CHAIN on)
  const SsspChainDesc* chain = persist && !l.done && !net->directed ? l.chain : nullptr;
  // the pop classes (counting build): their LDS words behind the ring, where the CU has room for them
  unsigned long long* pops = l.work ? l.pops : nullptr;
  if (pops && lds + SSSP_POP_WORDS * 8 + SSSP_STATIC_LDS > LDS_PER_CU) pops = nullptr;
  if (pops) lds += SSSP_POP_WORDS * 8;
  auto go = [&](auto kern) {
    SG_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(LDS_PER_CU - SSSP_STATIC_LDS)));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(1024), lds, ctx->stream, net->out_off, net->out_arc, n, net->n_arcs,
                       l.d_used, l.n_used, l.row_begin, l.row_begin, net->self_edge, net->e_lat, net->e_loss,
                       l.out_lat, l.out_loss, l.sat_row, l.delta, vec, l.work, l.diag, k.claim, k.idle_sleep,
                       k.lane_deg, l.blk_rows, l.ub_row, l.ub_w, item_ctr, rows, k.spin_max, l.plan_ctl, l.plan_ph,
                       l.done, chain, ctx->apsp_ret + 4, (int)l.ident, k.step_arcs, pops, (int)k.early);
  };
  // <counting, threads, lane arcs, fill symbol, flagged>
  if (l.done) {  // the flagged one-launch plan
    if (l.work) go(k_sssp_lds<true, 1024, 8, 0, true>);
    else if (ctx->in_fill) go(k_sssp_lds<false, 1024, 8, 1, true>);
    else go(k_sssp_lds<false, 1024, 8, 0, true>);
  } else if (l.work) {
    go(k_sssp_lds<true, 1024, 8, 0>);
  } else if (ctx->in_fill) {
    go(k_sssp_lds<false, 1024, 8, 1>);
  } else {
    go(k_sssp_lds<false, 1024, 8, 0>);
  }
  SG_CHECK_LAUNCH();
}


}  // namespace sg
