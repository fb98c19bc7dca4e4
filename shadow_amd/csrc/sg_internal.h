// sg_internal.h -- host-side runtime shared by the HIP translation units:
// context, grow-only device workspace, error plumbing.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <new>
#include <stdexcept>
#include <string>
#include <atomic>
#include <deque>
#include <memory>
#include <vector>

#include "../../include/shadow_gpu.h"

namespace sg {

// Status-carrying exception; converted to a status code at the C boundary.
struct Error : std::runtime_error {
  int32_t code;
  uint32_t row, col;
  Error(int32_t c, const std::string& m, uint32_t r = 0, uint32_t k = 0)
      : std::runtime_error(m), code(c), row(r), col(k) {}
};

#define SG_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      if (e_ == hipErrorOutOfMemory) throw ::sg::Error(SG_ERR_OOM, std::string(#expr) + ": out of device memory"); \
      throw ::sg::Error(SG_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    }                                                                                       \
  } while (0)

#define SG_CHECK_LAUNCH() SG_HIP(hipGetLastError())

// Grow-only device buffer.  Growth is the only path that allocates, so a
// steady-state round never calls hipMalloc.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* get(size_t count) {
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    if (bytes > cap) {
      release();
      SG_HIP(hipMalloc(&p, bytes));
      cap = bytes;
    }
    return static_cast<T*>(p);
  }
};

// Per-kernel timer: HIP events recorded on the context stream around each
// launch of an instrumented kernel (bench.py reads the average launch time and
// the algorithmic work the launch site declares).
struct KernelTimer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0.0;
  double work = 0.0;  // algorithmic units (relaxations / bytes), summed over launches
  uint64_t launches = 0;
};


}  // namespace sg

struct sg_round_ret {
  unsigned long long stats[3];  // n_delivered, min deliver time, min used latency
  uint32_t err;
  uint32_t overflow;  // a bucketing region overflowed: the scan path must run
  // sg_deliver_bucket_padded: this rank's receive count from each rank, and the
  // largest count any rank sent any rank (over the padded capacity: exchange again)
  uint32_t recv_cnt[64];
  uint32_t pair_max;
  uint32_t pad_;
};

struct sg_ctx {
  int device = 0;
  unsigned long long* pair_count = nullptr;  // sg_ctx_set_packet_counters: per table cell (device), or null
  uint64_t pair_count_cells = 0;
  uint64_t net_serial = 0;   // the last sg_net serial handed out
  uint64_t dense_owner = 0;  // the net whose arcs r_dense holds sorted (0: none)
  uint32_t dense_gen = 0;    // stamp of the dense search's seed-row marks in r_dense (0: none valid)
  uint64_t band_owner = 0;   // the net whose degree-class numbering r_band holds (0: none)
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  int n_cu = 256;
  std::string last_error;
  uint32_t err_row = 0, err_col = 0;
  // routing workspace
  sg::DevBuf r_dist, r_dist2, r_flags, r_used, r_err, r_self, r_pair_cnt, r_pair_edge, r_map, r_out_lat,
      r_out_loss, r_misc, r_dirty, r_work, r_items, r_plan, r_dense, r_done, r_bucket, r_band;
  // delivery workspace
  sg::DevBuf d_seg, d_dst, d_cnt, d_cur, d_keys, d_vals, d_keys2, d_vals2, d_keys3, d_keys4, d_misc,
      d_scan, d_lists, d_lists2, d_ctr0, d_blk, d_spill;
  sg::DevBuf m_scratch;
  // shortest-path trees (sg_tree.hip): the node list and its inverse, the flag word, and the
  // device rows of outputs the caller takes on the host or not at all
  sg::DevBuf t_idx, t_flag, t_pred, t_fh;
  // link loads (sg_link.hip): the node list and its inverse, the flag words, the device copies of
  // host inputs and outputs (l_hops: sg_link_load_packets' per-packet hops), and the global
  // path's per-workgroup rows
  sg::DevBuf l_idx, l_flag, l_pred, l_cnt, l_link, l_node, l_scratch, l_hops;
  // (l_idx, l_flag and l_pred serve every walk up the tree rows: sg_link.hip, sg_paths.hip,
  // sg_trace.hip)
  // tree paths (sg_paths.hip): the hop count per pair, the device copies of host inputs (table
  // rows, pair arrays) and outputs, and the pinned, mapped word that receives the record total
  // (allocated on first use); p_sums: the block sums of scan_counts (sg_scan.hip), whoever calls
  sg::DevBuf p_cnt, p_sums, p_lat, p_loss, p_pair, p_off, p_node, p_link, p_olat, p_oloss;
  unsigned long long* paths_ret = nullptr;
  // link trace (sg_trace.hip; it shares p_cnt, p_lat, p_off, the p_* outputs and paths_ret, and
  // p_sums through scan_counts): the link counters with the fill's cursors and the work counter,
  // the two staging arrays (keys, exit times), the sort's work entries, the device copies of a
  // host watch array and of out_exit_ns
  sg::DevBuf tr_cnt, tr_key, tr_key2, tr_exit, tr_exit2, tr_work, tr_watch, tr_oexit;
  // link time series (sg_series.hip; it shares l_idx, l_flag, l_pred and p_lat): the device copy
  // of a host slot map, and the zeroed sums of a host-mode call or of a group member
  sg::DevBuf sr_slot, sr_series, sr_outside;
  // link queues (sg_queue.hip, sg_queue.h): the device copies of a host-mode call's six inputs and eight
  // outputs, the tile aggregates, the done times when the caller takes none, the flag words
  sg::DevBuf q_buf[14], q_agg, q_done, q_flag;
  // the carried form (SG_LINK_QUEUE_CARRY, sg_queue_carry.hip; it shares tr_key, tr_key2 and tr_work with the link
  // trace's sort, and p_sums through scan_counts): the per-packet counters with the fill's
  // cursors and the sort's work counter, the packet offsets, the records in chain order, next,
  // gap, the carried enter times, and a link-sorted pass: enter, packet, the permutation, done,
  // wait, ahead
  sg::DevBuf qc_cnt, qc_off, qc_list, qc_next, qc_gap, qc_cur, qc_enter, qc_packet, qc_perm, qc_done, qc_wait, qc_ahead;
  // finite buffers (SG_LINK_QUEUE_DROP, sg_queue_drop.hip; p_sums through scan_counts): the period heads and then
  // the served marks, their exclusive sums, the period starts, the long periods with their
  // counter, and per record the running done and the wait; the carried form's sorted done
  sg::DevBuf qd_mark, qd_pos, qd_start, qd_long, qd_run, qd_wait, qd_done;
  // the windowed form (SG_LINK_QUEUE_WINDOW, sg_queue_window.hip; over the carried form's arrays): the chain
  // predecessors, the active marks with their exclusive sums, the compact link offsets, the sort's
  // work counter
  sg::DevBuf qw_prev, qw_act, qw_pos, qw_off, qw_ctr;
  // the time series (SG_LINK_QUEUE_SERIES, sg_queue_series.hip): the difference array of a call, zeroed by it,
  // and the chunk sums of the row pass over long rows
  sg::DevBuf qs_diff, qs_part;
  // sg_routing_info_fill: double-buffered device row blocks, copied to the host
  // on copy_stream while the next block computes
  sg::DevBuf r_stage_lat[2], r_stage_loss[2], r_stage_pack[2];
  hipStream_t copy_stream = nullptr;
  bool in_fill = false;  // inside sg_routing_info_fill (selects the row-block kernel symbols)
  hipEvent_t stage_done[2] = {nullptr, nullptr}, stage_copied[2] = {nullptr, nullptr};
  // The phased plan's bound rows (sg_plan.hip k_plan_bounds) run beside phase 0 on a stream
  // of their own (created by the first build that needs it): plan_lists orders them after the
  // lists kernel, plan_bounds orders the first bounded launch after them.  side_busy: work was
  // queued there that the context stream's last synchronisation may not cover (an error exit
  // synchronises the side stream itself).
  hipStream_t side_stream = nullptr;
  hipEvent_t plan_lists = nullptr, plan_bounds = nullptr;
  bool side_busy = false;
  // sg_routing_build with the identity used list ("every node used", in order): no copy of the
  // list; the build's first kernel that reads it writes used_fill[j] = j, j < used_fill_n, first
  // (the plan's k_plan_rel, else a fill of its own: sg_routing.hip flush_used).  Null: nothing
  // is pending.
  uint32_t* used_fill = nullptr;
  uint32_t used_fill_n = 0;
  // ... and, copied or not, that the list of the build in progress is the identity (the LDS
  // search then reads no column ids); false outside sg_routing_build, so in sg_routing_info_fill
  bool used_ident = false;
  // Round control: round_err (device, zeroed at creation) collects the source
  // phase's error flags; the stats kernel hands them to the host and clears
  // them for the next round.  round_ret (pinned, mapped host memory) receives
  // the round's stats and error flags straight from that kernel: no copies.
  uint32_t* round_err = nullptr;
  sg_round_ret* round_ret = nullptr;
  // sg_deliver_source_padded does not synchronise: its flags sit in round_ret until a call that
  // does reads them (sg_deliver_bucket_padded, or sg_wire_pop on the wire's path); set until then.
  bool round_flags_pending = false;
  // Region bucketing counters, two parities of [SB_SUB x SB_MAX counts + overflow
  // flag] (zeroed at creation; each call's sort kernel clears the other parity),
  // then two parities for the coarse level of two-level scatters (cleared by the
  // second level's kernel).
  uint32_t* sb_ctl = nullptr;
  uint32_t sb_parity = 0, sb_parity_c = 0;
  sg::DevBuf d_cd, d_ct, d_ck, d_ci;  // coarse-level runs of a two-level scatter
  // APSP (pinned host-mapped, 32 B): [0] the slab's active-batch count of the next
  // pass (k_active_list, each pass-chunk end); [4] the flagged rows' count (k_build_finish, the
  // build's end) or, where no such kernel runs, nonzero once an LDS search flagged a row;
  // [2..3] the self-loop check's first failure (k_build_finish)
  uint32_t* apsp_ret = nullptr;
  // sg_routing_build's self-loop check (graph/mod.rs:210-217), folded into the LDS
  // search's final kernel when it runs: the inputs, and the result once read
  const uint32_t* self_used = nullptr;
  uint32_t self_n = 0;
  const uint32_t* self_cnt = nullptr;
  bool self_done = false;
  unsigned long long self_first = ~0ull;
  // sg_net device blocks released by sg_net_destroy, reused by the next sg_net_create
  // (a simulation that builds one graph and one table pays no hipMalloc / hipFree,
  // whose implicit device synchronisation cost ~0.2 ms each); `freed` orders the
  // reuse after the last work queued on the released block
  struct NetBlock {
    void* p;
    size_t bytes;
    hipEvent_t freed;
  };
  std::vector<NetBlock> net_pool;
  // pinned staging of a new graph's edge arrays (one H2D copy); `stage_used` marks
  // when the last copy out of it completed
  // (slot 0: edges; slot 1: a build's used-node list)
  void* h_stage[2] = {nullptr, nullptr};
  size_t h_stage_bytes[2] = {0, 0};
  hipEvent_t stage_used[2] = {nullptr, nullptr};
  // kernel timers (off unless sg_ctx_enable_timers)
  bool timing = false;
  bool count_work = false;  // SG_TIMERS_COUNT_WORK
  std::deque<std::pair<std::string, sg::KernelTimer>> timers;  // deque: stable addresses
  std::vector<hipEvent_t> event_pool;
};

// Device-resident network graph (sg_net.hip builds it).
struct sg_net {
  sg_ctx* ctx = nullptr;
  uint64_t serial = 0;  // unique per context: who owns the context's sorted-arc workspace (sg_dense.hip)
  uint32_t n_nodes = 0, n_edges = 0, n_arcs = 0;
  bool directed = false;
  // the arcs' smallest latency and mean latency (each clamped to LAT32_SAT), taken on the host
  // for graphs the bucketed search takes (sg_bucket.hip sizes its bucket width from them)
  uint32_t arc_lat_min = 0;
  double arc_lat_mean = 0.0;
  std::vector<uint32_t> gml_id;
  // GML edge list (device)
  uint32_t* e_src = nullptr;
  uint32_t* e_dst = nullptr;
  uint64_t* e_lat = nullptr;
  float* e_loss = nullptr;
  // in-arc CSC without self-loops (device)
  uint32_t* in_off = nullptr;  // n_nodes + 1
  uint32_t* in_src = nullptr;
  uint64_t* in_lat = nullptr;    // exact latency (wide kernel)
  float* in_om = nullptr;        // 1f32 - loss
  uint4* in_rec = nullptr;       // per in-arc (source, destination, latency32, bits(1f32 - loss))
  bool csc = false;              // the in-arc arrays above are built (ensure_csc, on first use)
  // out-arc CSR without self-loops (device), for the per-source LDS search
  // (sg_sssp.hip): out_arc = 3 u32 per arc (head node, latency32, bits(1f32 - loss))
  uint32_t* out_off = nullptr;  // n_nodes + 1
  uint32_t* out_arc = nullptr;
  // self-loops
  uint32_t* self_cnt = nullptr;
  uint32_t* self_edge = nullptr;
  void* mem = nullptr;  // one device block holding every array above (from the context's pool)
  size_t mem_bytes = 0;
  // links (sg_link.hip ensure_links, on first use): the distinct ordered node pairs joined by an
  // edge, ascending (head, tail).  Host: the list and each edge's link numbers; device (lk_mem, a
  // block of its own): lk_off[n_nodes + 1] by head, lk_tail[n_links]
  bool links = false;
  uint32_t n_links = 0;
  std::vector<uint32_t> lk_tail_h, lk_head_h, e_fwd, e_rev;
  uint32_t* lk_off = nullptr;
  uint32_t* lk_tail = nullptr;
  void* lk_mem = nullptr;
  ~sg_net() {
    if (mem) (void)hipFree(mem);  // (sg_net_destroy hands it back to the pool instead)
    if (lk_mem) (void)hipFree(lk_mem);
  }
};

// Host-resident dense RoutingInfo (sg_route_info.hip).
struct sg_routing_info {
  uint32_t n = 0;
  std::vector<uint32_t> node_ids;
  // n x n cells (latency << 32) | bits(loss), pinned when a device was present at
  // creation; a cell whose latency half is SG_CELL_WIDE has its u64 latency in
  // `wide` (sorted by cell index)
  uint64_t* cell = nullptr;
  bool pinned = false;
  struct Wide {
    uint64_t cell;
    uint64_t lat;
  };
  std::vector<Wide> wide;
  // per row: 0 not written, 1 written with its smallest latency in row_min, 2 written by a
  // fill (row_min not kept; computed once if set_rows later needs it); all written -> filled
  std::vector<uint8_t> row_set;
  std::vector<uint64_t> row_min;
  uint32_t rows_set = 0;
  bool filled = false;
  uint64_t min_lat = UINT64_MAX;
  // GML id -> row: dense window [id_base, id_base + id_span) or sorted (id, row) pairs
  uint32_t id_base = 0, id_span = 0;
  std::vector<uint32_t> id_dense;
  std::vector<std::pair<uint32_t, uint32_t>> id_sorted;
  // address (host byte order) -> row (IpAssignment::get_node, then the id map)
  uint32_t ip_base = 0, ip_span = 0;
  std::vector<uint32_t> ip_dense;
  std::vector<std::pair<uint32_t, uint32_t>> ip_sorted;
  // increment_packet_count: n x n saturating counters, allocated on first use
  std::atomic<uint64_t*> counters{nullptr};
  ~sg_routing_info();
};

// A device group (sg_group.hip; sg_group_trace.hip holds its link loads and link trace).
struct sg_group {
  std::vector<sg_ctx*> ctxs;
  std::vector<hipEvent_t> sent, pulled;  // one per member, created on the member's device
  std::string last_error;
  uint32_t err_row = 0, err_col = 0;
  uint32_t err_member = 0xFFFFFFFFu;  // the member whose error the last call reported, or UINT32_MAX
};

namespace sg {

constexpr uint32_t GROUP_MAX = 64;  // members of a group (sg_round_ret::recv_cnt)

inline void set_device(const sg_ctx* c) { SG_HIP(hipSetDevice(c->device)); }

// Map exceptions to a status and the group's last error (sg::guarded, for a group).  A call that
// reports a member's error sets err_member before it throws.
template <class F>
int32_t group_guarded(sg_group* g, F&& fn) {
  if (!g) return SG_ERR_INVALID_ARG;
  int prev = 0;
  (void)hipGetDevice(&prev);
  int32_t rc = SG_OK;
  g->err_member = 0xFFFFFFFFu;
  try {
    fn();
    g->last_error.clear();
    g->err_row = g->err_col = 0;
  } catch (const Error& e) {
    g->last_error = e.what();
    g->err_row = e.row;
    g->err_col = e.col;
    rc = e.code;
  } catch (const std::bad_alloc&) {
    g->last_error = "host out of memory";
    rc = SG_ERR_OOM;
  } catch (const std::exception& e) {
    g->last_error = e.what();
    rc = SG_ERR_DEVICE;
  }
  (void)hipSetDevice(prev);  // the calls walk over the members' devices
  return rc;
}

// Run `fn` with the context's device current; map exceptions to status codes.
template <class F>
int32_t guarded(sg_ctx* ctx, F&& fn) {
  if (!ctx) return SG_ERR_INVALID_ARG;
  try {
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (prev != ctx->device) SG_HIP(hipSetDevice(ctx->device));
    fn();
    ctx->last_error.clear();
    ctx->err_row = ctx->err_col = 0;
    return SG_OK;
  } catch (const Error& e) {
    ctx->last_error = e.what();
    ctx->err_row = e.row;
    ctx->err_col = e.col;
    return e.code;
  } catch (const std::bad_alloc&) {
    ctx->last_error = "host out of memory";
    return SG_ERR_OOM;
  } catch (const std::exception& e) {
    ctx->last_error = e.what();
    return SG_ERR_DEVICE;
  }
}

// sg_routing.hip: the host RoutingInfo fill over a row range of one context (what
// sg_routing_info_fill runs over every row and sg_group_routing_info_fill, sg_group.hip, over
// one range per member), the used-node list's check, and the object's state around a fill.
struct FillRows {
  uint64_t min_lat = UINT64_MAX;
  std::vector<sg_routing_info::Wide> wide;  // unsorted
};
// (returns whether the list is the identity: nodes[j] == j for every j)
bool check_node_list(const sg_net* net, const uint32_t* nodes, uint32_t n_used);
// The pending fill of an identity used list (sg_ctx::used_fill), launched now if still pending:
// ahead of the first kernel that reads the list, wherever the plan's first kernel does not run.
void flush_used(sg_ctx* ctx);
void fill_rows(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t flags, sg_routing_info* ri, uint32_t r0,
               uint32_t r1, uint32_t block_rows, bool self_check, FillRows* out);
void fill_reset(sg_routing_info* ri);
void fill_finish(sg_routing_info* ri, uint64_t min_lat, std::vector<sg_routing_info::Wide>&& wide);

// Region bucketing counters per parity: 8 sub-counters (one per XCD) x SB_MAX
// (4096) super-buckets + an overflow flag.
constexpr uint32_t SB_SUB = 8;
constexpr uint32_t SB_CTL_STRIDE = SB_SUB * 4096 + 1;

inline unsigned grid_for(size_t n, unsigned block, unsigned cap = 1u << 20) {
  size_t g = (n + block - 1) / block;
  if (g == 0) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

// Exclusive scan of n u32 values (device, in -> out, out has n+1 entries, out[n] = total).
void exclusive_scan_u32(sg_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, uint32_t n);
// sg_scan.hip: the exclusive u64 scan of n u32 counts (any n), three launches on the context
// stream: off[0 .. n] (off[n] = the sum) and *total = the sum (device-visible memory).  The
// block sums live in ctx->p_sums.
void scan_counts(sg_ctx* ctx, const uint32_t* cnt, uint32_t n, unsigned long long* off, unsigned long long* total);

// Group offsets of a key array grouped by ascending key (sg_deliver.hip's
// k_host_off): off[g] = first index whose key >= g, g = 0..n_groups.  err bit
// 1: not grouped ascending; bit 2: a key >= n_groups.
void launch_group_offsets(sg_ctx* ctx, const uint32_t* key, uint32_t n, uint32_t n_groups, uint32_t* off,
                          uint32_t* err);

// Read a few scalars back (blocking on the context stream).
void copy_to_host(sg_ctx* ctx, void* dst, const void* src, size_t bytes);

// Pinned staging for host-to-device copies (a pageable source costs the runtime's own
// staging and ~20 us): stage_acquire waits until the slot's previous copy has left it
// and returns it (grown to `bytes`); stage_release after the hipMemcpyAsync out of it.
char* stage_acquire(sg_ctx* ctx, int slot, size_t bytes);
void stage_release(sg_ctx* ctx, int slot);

// After a synchronisation of the context's stream: throws the error of a padded source phase
// whose flags no call has reported yet (sg_deliver.hip); otherwise nothing.
void report_round_flags(sg_ctx* ctx);

// Add algorithmic work to a timer after the fact (e.g. a device-side count).
void timer_add_work(sg_ctx* ctx, const char* name, double work);
// A counter pair of the last build under a timer's name: read_timer gives (0, n, work).  `always`:
// kept whether or not the timers are on.
void timer_set_counter(sg_ctx* ctx, const char* name, double work, uint64_t n, bool always = false);

// RAII bracket for one instrumented launch: `TimedLaunch t(ctx, "k_walk", work);`
// before the launch; the end event is recorded when `t` goes out of scope.
struct TimedLaunch {
  sg_ctx* ctx;
  KernelTimer* timer = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  TimedLaunch(sg_ctx* c, const char* name, double work);
  ~TimedLaunch();
};

// Per-source LDS-resident shortest paths (sg_sssp.hip).  Rows [row_begin,
// row_end) of the table, one workgroup each; or, with blk_rows, the n_blk rows
// listed there (absolute, within [row_begin, row_end)).  ub_row / ub_w (per
// workgroup, SSSP_KB_MAX each, optional): rows of out-neighbours s' already in
// the table (~0u: none) and the arc latencies s -> s'; the search starts every
// key at min over them of (w + D[s'][v]) + 1 instead of infinity.  A bound row
// whose ub_row entry carries SSSP_UB_EXACT (a zero-loss arc s -> s', every node a
// used node) also seeds exact keys (w + D[s'][v].lat, D[s'][v].loss); see
// sg_sssp.hip "Exact seeds".  The bound rows must be final before the launch
// (an earlier launch on the stream).
// Per-source search of dense graphs, settling by rounds and relaxing only the arcs
// below the round's largest unsettled latency (sg_dense.hip): rows [row_begin,
// row_end); sat_row (zeroed by the caller) receives 1 for rows needing the wide
// kernel.  Sorts every node's out-arcs by latency on the stream first.  work
// (optional, WORK_SHARDS counters): arcs relaxed.
constexpr uint32_t DENSE_MAX = 4096;
bool sssp_dense_fits(uint32_t n_nodes);
void launch_sssp_dense(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, uint32_t row_begin,
                       uint32_t row_end, uint64_t* out_lat, float* out_loss, uint32_t* sat_row,
                       unsigned long long* work);

// Per-source delta-stepping search of sparse graphs past the LDS search (sg_bucket.hip): rows
// [row_begin, row_end); sat_row (zeroed by the caller) receives 1 for rows needing the wide
// kernel, 2 for rows whose search gave up.  work / diag optional (relaxations; [buckets,
// entries, far steps, pops]).
bool sssp_bucket_fits(uint32_t n_nodes);
void launch_sssp_bucket(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, uint32_t row_begin,
                        uint32_t row_end, uint64_t* out_lat, float* out_loss, uint32_t* sat_row,
                        unsigned long long* work, unsigned long long* diag);

constexpr int SSSP_KB_MAX = 8;
constexpr uint32_t SSSP_UB_EXACT = 0x80000000u;  // bound rows per bounded search (sg_sssp.hip SSSP_KB)
bool sssp_lds_fits(uint32_t n_nodes);

// Chained rows (sg_sssp.hip), in device memory: claim, one word per row of the block (0: free);
// rel[node] its relative row (~0: not a row of the block); with a plan, phase_of / pos: a relative
// row's phase and its place in the plan's list (null without one); exact: SG_SSSP_EXACT;
// check_rows: 0, or the block's row count when rel was written for the block's rows only and
// holds anything elsewhere -- an entry then counts only if used[] maps it back to its node
// (a row block without a plan: no fill of rel on a one-shot build's path).
struct SsspChainDesc {
  uint32_t* claim;
  const uint32_t* rel;
  const uint8_t* phase_of;
  const uint32_t* pos;
  uint32_t exact, check_rows;
};

// One launch of the LDS search on a net (the graph arrays come from it).
constexpr int SSSP_DIAG_WORDS = 16;  // SG_SSSP_DIAG: u64 words per row (sg_sssp.hip writes, print_sssp_diag reads)
// SG_SSSP_DIAG, counting build: a launch's pops by class of S = ceil(arcs / 64): 0, 1, 2, 3-4, 5-8, > 8;
// (pops, arcs, step cycles) per class, then the pops that took the lane path and the pops every wave
// counted (u64 words)
constexpr int SSSP_POP_CLASSES = 6;
constexpr int SSSP_POP_WORDS = 3 * SSSP_POP_CLASSES + 2;
struct SsspLdsLaunch {
  // the row block: rows [row_begin, row_end) of the table (out_* device, row-major from
  // row_begin); sat_row (row_end - row_begin u32) receives 1 for rows needing the wide kernel;
  // delta the bucket width in ns; work / diag optional (relaxations; SSSP_DIAG_WORDS per row)
  const uint32_t* d_used = nullptr;
  uint32_t n_used = 0, row_begin = 0, row_end = 0;
  bool ident = false;  // d_used[j] == j for every j: the kernel takes column j's node as j and does not load the list
  uint64_t* out_lat = nullptr;
  float* out_loss = nullptr;
  uint32_t* sat_row = nullptr;
  uint32_t delta = 0;
  unsigned long long* work = nullptr;
  unsigned long long* diag = nullptr;
  unsigned long long* pops = nullptr;  // with work: SSSP_POP_WORDS counters the launch adds to (see above)
  // the plan (optional): the rows to run (blk_rows, n_blk) and their bound rows (ub_row, ub_w),
  // as described above; plan_ctl / plan_ph: the device plan's phase to run (n_blk then bounds
  // its row count, which only the device knows); plan_ctr: the launch's claim counters, zeroed
  // by the caller (null: the launch zeroes its own); done: per-row flags of the flagged
  // one-launch plan (sg_sssp.hip "Flagged rows")
  const uint32_t* blk_rows = nullptr;
  uint32_t n_blk = 0;
  const uint32_t* ub_row = nullptr;
  const uint32_t* ub_w = nullptr;
  const uint32_t* plan_ctl = nullptr;
  int plan_ph = 0;
  uint32_t* plan_ctr = nullptr;
  uint32_t* done = nullptr;
  // chained rows (sg_sssp.hip "Chained rows"; null: off): the device descriptor that
  // sssp_device_plan / sssp_plain_rel wrote, its claim words zeroed
  const SsspChainDesc* chain = nullptr;
};
void launch_sssp_lds(sg_ctx* ctx, const sg_net* net, const SsspLdsLaunch& l);

// sg_net.hip: the in-arc CSC of a net, built on its first use (the upload writes the out-arcs
// only); a node's GML id as text, for error messages; two zero fills as one launch on the
// context stream
void ensure_csc(sg_ctx* ctx, sg_net* net);
// sg_link.hip: the net's link list (sg_net::lk_*), built on its first use
void ensure_links(sg_ctx* ctx, sg_net* net);
std::string node_name(const sg_net* net, uint32_t idx);
void launch_zero2(sg_ctx* ctx, uint32_t* a, uint32_t na, uint32_t* b, uint32_t nb);

// sg_slab.hip: the batched-source slab search of rows [row_begin, row_end) (any graph whose
// slab offsets fit 32 bits), and the wide (u64 latency) recomputation of the listed rows
// (absolute row indices) every search falls back to
constexpr int WORK_SHARDS = 64;  // relaxation counter shards (measurement only)
// the LDS search's counters behind the shards: chained rows (2), the ring invariant (2), the pops by
// class, then SG_SSSP_EARLY's two: rows that started under their bound rows' loads, merges onto dirty keys
constexpr int WORK_SSSP_EARLY = WORK_SHARDS + 4 + SSSP_POP_WORDS;
void shortest_paths_slab(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, uint32_t row_begin,
                         uint32_t row_end, uint64_t* out_lat, float* out_loss);
void run_wide(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, const std::vector<uint32_t>& rows,
              uint32_t out_row0, uint64_t* out_lat, float* out_loss);

// The LDS search's phase plan, built on the device (sg_plan.hip) on the context
// stream: phase p's rows are list[ctl[2p] .. + ctl[2p + 1]) (absolute row indices),
// their SSSP_KB_MAX bound rows and latencies at the same list positions of ub_row /
// ub_w; ctr[2p .. 2p + 2) are the phase launch's claim counters (zeroed).
struct SsspDevPlan {
  int n_phase = 0;
  uint32_t* list = nullptr;
  uint32_t* ub_row = nullptr;
  uint32_t* ub_w = nullptr;
  uint32_t* ctl = nullptr;
  uint32_t* ctr = nullptr;
  const SsspChainDesc* chain = nullptr;  // written when the caller passed claim words
  bool landmarks = false;  // phase 0 = landmark rows; phase 1's bounds come from them (sssp_landmark_bounds)
  unsigned rows_grid = 0;  // sssp_landmark_bounds' grid (one thread per row of the block)
  // the bound rows were left to sssp_plan_bounds_side (its inputs in the plan's workspace)
  bool bounds_deferred = false;
  const uint32_t* rel = nullptr;
  const uint8_t* phase_of = nullptr;
};
constexpr int SSSP_PHASES_MAX = 6;
// defer_bounds: the plan ends at its lists (an event marks them on the context stream); the
// caller launches phase 0, which reads no bound row, and then sssp_plan_bounds_side.
SsspDevPlan sssp_device_plan(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, uint32_t row_begin,
                             uint32_t row_end, int n_phase, int kb, bool exact, int hops, uint32_t n_land,
                             uint32_t* zero_rows = nullptr, uint32_t* zero_rows2 = nullptr, bool chain = false,
                             bool chain_exact = false, bool defer_bounds = false);
// The deferred bound rows on the context's side stream, after the plan's lists.  Sets
// ctx->side_busy; the caller orders the context stream's next launch after the side stream.
void sssp_plan_bounds_side(sg_ctx* ctx, const sg_net* net, const SsspDevPlan& p, const uint32_t* d_used,
                           uint32_t row_begin, uint32_t row_end, int kb, bool exact, int hops);
// Without a plan: rel alone (in the plan's workspace) and the chained rows' descriptor, zeroing the
// row flags, the claim words and the two claim counters in the same launch.
const SsspChainDesc* sssp_plain_rel(sg_ctx* ctx, const sg_net* net, const uint32_t* d_used, uint32_t row_begin,
                                    uint32_t row_end, uint32_t* zero_rows, uint32_t* claim, uint32_t* zero_ctr,
                                    bool chain_exact);
// After phase 0 (the landmarks) ran: phase 1's bound rows from the landmark rows' columns.
void sssp_landmark_bounds(sg_ctx* ctx, const SsspDevPlan& p, uint32_t n_used, uint32_t row_begin,
                          const uint64_t* out_lat, const uint32_t* sat_row, int kb);

}  // namespace sg
