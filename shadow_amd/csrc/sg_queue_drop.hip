// sg_queue_drop.hip -- link queues, finite buffers (SG_LINK_QUEUE_DROP): tail drop under a longest
// wait per link.  A layer over the first-order scan (sg_queue.hip; sg_queue.h has what they share).
//
// The limited recurrence -- start = max(enter, done); start - enter > limit: dropped, done as it
// was; else done = start + s -- is no constant-size scan (the map of one record is not closed
// under composition), but its `done` never exceeds the unlimited queue's.  A record the unlimited
// scan serves without waiting therefore finds the limited server idle too: the limited queue
// restarts there, and a link's records fall into independent busy periods.
//   agg, tile carry  the unlimited scan's first two launches (sg_queue.hip's launch_walk);
//   k_drop_heads     the tile again with its tile carry: mark[i] = 1 where the unlimited wait is 0
//                    or a segment starts.  No caller output, no overflow flag (the pass may saturate);
//   scan_counts      the marks' exclusive sums, and k_drop_starts: the period starts, compacted;
//   k_drop_lane      a lane per period: one of at most D_SHORT records is walked by its lane,
//                    a longer one is appended to the list of long periods;
//   k_drop_wave      a wave per long period: 64 records per coalesced load (the next 64 in flight
//                    meanwhile), the scalar `done` stepped through them by lane reads of a uniform
//                    lane; every lane keeps the `done` before its record and finishes it alone.
// A walk leaves per record wt (the wait; all ones: not served), run (the `done` after it: it never
// falls within a segment, a dropped record repeats the value before it) and mark (1: served).
// SG_LINK_QUEUE_SERIAL = 1: k_drop_serial, a lane per link, leaves the same three arrays.
//   k_drop_finish    a lane per record: the caller's wait, done and ahead (one binary search over
//                    run, then a difference of the served marks' exclusive sums), out_link_free,
//                    and the per-link sums by the wave reduction of k_queue_ahead.
// Carried (d.absent): a record whose enter time is all ones is absent: it sorts last on its link,
// is a period of its own in the unlimited pass, and is skipped by every walk.
#include "sg_queue.h"

namespace sg {
namespace {

constexpr uint32_t D_SHORT = 32;  // the longest period a lane walks

struct DArgs {
  QArgs q;           // the inputs, agg_*, flag; wait / done / ahead and the per-link arrays: k_drop_finish's
  const u64* limit;  // cost + n_links
  uint32_t absent;   // carried: enter == MAX is an absent record
  uint32_t lng_cap;
  uint32_t* mark;  // the period heads, then the served records
  u64* pos;        // n + 2: the exclusive sums of mark, the total twice
  uint32_t* start;  // the period starts
  uint32_t* lng;    // the long periods, in any order
  uint32_t* n_long;
  u64* run;
  u64* wt;
  uint32_t* drops;  // the second halves of out_link_ahead_max and out_link_busy_ns, or null
  u64* refused;
};

// (the kernels take the struct by value: a field added here moves their arguments)
static_assert(sizeof(DArgs) == 256 && offsetof(DArgs, limit) == sizeof(QArgs), "DArgs keeps its layout");

// The pass `a` under the drop rule with the layer's scratch arrays (carried_run: sg_queue.h).
DArgs drop_args(sg_ctx* ctx, const QArgs& a, u64* carried_run) {
  DArgs d = {};
  d.q = a;
  d.limit = a.cost + a.n_links;
  d.absent = carried_run ? 1u : 0u;
  d.drops = a.out.amax ? a.out.amax + a.n_links : nullptr;
  d.refused = a.out.busy ? a.out.busy + a.n_links : nullptr;
  if (a.n) {
    d.lng_cap = (uint32_t)(a.n / (D_SHORT + 1u) + 1u);
    d.mark = ctx->qd_mark.get<uint32_t>(a.n);
    d.pos = ctx->qd_pos.get<u64>((size_t)a.n + 2);
    d.start = ctx->qd_start.get<uint32_t>(a.n);
    d.lng = ctx->qd_long.get<uint32_t>((size_t)d.lng_cap + 1);
    d.n_long = d.lng + d.lng_cap;
    d.run = carried_run ? carried_run : ctx->qd_run.get<u64>(a.n);
    d.wt = ctx->qd_wait.get<u64>(a.n);
  }
  return d;
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_links(const DArgs d) {
  const u64 q = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (q >= d.q.n_links) return;
  if (d.drops) d.drops[q] = 0u;
  if (d.refused) d.refused[q] = 0ull;
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_heads(const DArgs d) {
  __shared__ QElem s_wave[16];
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 base = (u64)blockIdx.x * Q_TILE + (u64)threadIdx.x * Q_PER;
  QLane r;
  tile_rescan(a, s_wave, base, r, [&](uint32_t k, u64 start, u64) {
    d.mark[base + k] = ((r.head >> k) & 1u) || start == r.e[k] ? 1u : 0u;  // (no wait: e >= the done before)
  });
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_starts(const DArgs d) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= d.q.n || d.q.flag[Q_BAD_OFF] != Q_MAX) return;
  if (!d.mark[i]) return;
  const u64 at = d.pos[i];
  if (at < d.q.n) d.start[at] = (uint32_t)i;
}

// One record under the drop rule: the wait (all ones: not served) and the new `done`.
__device__ __forceinline__ u64 drop_step(u64& done, u64 e, u64 s, u64 lim, bool absent) {
  if (absent && e == Q_MAX) return Q_MAX;
  const u64 start = max(e, done), w = start - e;
  if (w > lim) return Q_MAX;
  done = sat_add(start, s);
  return w;
}

// Records [i0, i1) of link lk, one after the other.
template <bool FLAG>
__device__ __forceinline__ void drop_walk(const DArgs& d, uint32_t lk, u64 i0, u64 i1, u64 done) {
  const QArgs& a = d.q;
  const u64 cost = a.cost[lk], lim = d.limit[lk];
  for (u64 i = i0; i < i1; i++) {
    const u64 s = service_ns(record_weight(a, i, FLAG), cost), e = a.enter[i];
    const u64 w = drop_step(done, e, s, lim, d.absent != 0u);
    if (w != Q_MAX && done == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], i);
    d.wt[i] = w;
    d.run[i] = done;
    d.mark[i] = w != Q_MAX ? 1u : 0u;
  }
}

// Period p's records [i0, i1) and link, and the `done` it starts from: the link's free_in at a
// segment's first record, else the head's own enter time (the server is idle there).  False: not
// a period of a valid compaction.
__device__ __forceinline__ bool drop_period(const DArgs& d, u64 p, u64 np, u64& i0, u64& i1, uint32_t& lk, u64& done) {
  const QArgs& a = d.q;
  i0 = d.start[p];
  i1 = p + 1 < np ? (u64)d.start[p + 1] : a.n;
  if (i0 >= i1 || i1 > a.n) return false;
  lk = link_of(a.off, a.n_links, i0);
  if (i1 > a.off[lk + 1]) return false;
  done = i0 == a.off[lk] ? link_free_in(a, lk) : a.enter[i0];
  return true;
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_lane(const DArgs d) {
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 p = (u64)blockIdx.x * Q_THREADS + threadIdx.x, np = min(d.pos[a.n], a.n);
  if (p >= np) return;
  u64 i0, i1, done;
  uint32_t lk;
  if (!drop_period(d, p, np, i0, i1, lk, done)) return;
  if (i1 - i0 > D_SHORT) {
    const uint32_t slot = atomicAdd(d.n_long, 1u);
    if (slot < d.lng_cap) d.lng[slot] = (uint32_t)p;
    return;
  }
  drop_walk<false>(d, lk, i0, i1, done);
}

__device__ __forceinline__ u64 uniform64(u64 v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 lane_read64(u64 v, uint32_t k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)k);
  return ((u64)hi << 32) | lo;
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_wave(const DArgs d) {
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const uint32_t lane = threadIdx.x & 63u, waves = Q_THREADS / 64u;
  const uint32_t n_long = min(*d.n_long, d.lng_cap);
  const u64 np = min(d.pos[a.n], a.n);
  const bool absent = d.absent != 0u;
  for (uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * waves + (threadIdx.x >> 6))); w < n_long;
       w += gridDim.x * waves) {
    const u64 p = d.lng[w];
    if (p >= np) continue;
    u64 i0, i1, done;
    uint32_t lk;
    if (!drop_period(d, p, np, i0, i1, lk, done)) continue;
    i0 = uniform64(i0);
    i1 = uniform64(i1);
    done = uniform64(done);
    lk = (uint32_t)__builtin_amdgcn_readfirstlane((int)lk);
    // (in scalar registers before the first load below is issued: the stepping loop waits for no memory)
    const u64 cost = uniform64(a.cost[lk]), lim = uniform64(d.limit[lk]);
    u64 e = 0ull, s = 0ull;
    if (i0 + lane < i1) {
      e = a.enter[i0 + lane];
      s = service_ns(record_weight(a, i0 + lane, false), cost);
    }
    for (u64 b = i0; b < i1; b += 64ull) {
      // the next 64 records, in flight while these are stepped through
      u64 e2 = 0ull, s2 = 0ull;
      if (b + 64ull + lane < i1) {
        e2 = a.enter[b + 64ull + lane];
        s2 = service_ns(record_weight(a, b + 64ull + lane, false), cost);
      }
      const uint32_t cnt = (uint32_t)min((u64)64ull, i1 - b);
      u64 before = 0ull;
      for (uint32_t k = 0; k < cnt; k++) {
        const u64 ek = lane_read64(e, k), sk = lane_read64(s, k);
        if (lane == k) before = done;
        drop_step(done, ek, sk, lim, absent);
      }
      if (lane < cnt) {
        const u64 i = b + lane;
        const u64 wt = drop_step(before, e, s, lim, absent);
        if (wt != Q_MAX && before == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], i);
        d.wt[i] = wt;
        d.run[i] = before;
        d.mark[i] = wt != Q_MAX ? 1u : 0u;
      }
      e = e2;
      s = s2;
    }
  }
}

// ---- the lane-per-link form under the drop rule
__global__ void __launch_bounds__(Q_THREADS) k_drop_serial(const DArgs d) {
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 stride = (u64)gridDim.x * Q_THREADS;
  for (u64 q = (u64)blockIdx.x * Q_THREADS + threadIdx.x; q < a.n_links; q += stride) {
    const uint32_t lk = (uint32_t)q;
    drop_walk<true>(d, lk, a.off[lk], a.off[lk + 1], link_free_in(a, lk));
  }
}

__global__ void __launch_bounds__(Q_THREADS) k_drop_finish(const DArgs d, uint32_t want_ahead) {
  const QArgs& a = d.q;
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  uint32_t key = Q_NO_LINK, ahead = 0u, drops = 0u;
  u64 busy = 0ull, wmax = 0ull, wsum = 0ull, refused = 0ull;
  if (i < a.n) {
    key = link_of(a.off, a.n_links, i);
    const u64 i0 = a.off[key], i1 = a.off[key + 1];
    const u64 e = a.enter[i], w = d.wt[i], r = d.run[i];
    const bool absent = d.absent && e == Q_MAX, served = w != Q_MAX;
    if (want_ahead && !absent) {
      // the first j of the prefix with run[j] > e: the served from there on are ahead
      ahead = (uint32_t)min(d.pos[i] - d.pos[upper_bound(d.run, i0, i, e)], (u64)0xFFFFFFFFull);
    }
    if (a.out.wait) a.out.wait[i] = w;
    if (a.out.done) a.out.done[i] = served ? r : e;
    if (a.out.ahead) a.out.ahead[i] = ahead;
    if (a.out.link_free) {
      // run after the last record that arrives: the done of the record served last, or free_in
      if (absent) {
        if (i == i0) a.out.link_free[key] = link_free_in(a, key);
      } else if (i + 1 == i1 || (d.absent && a.enter[i + 1] == Q_MAX)) {
        a.out.link_free[key] = r;
      }
    }
    if (!absent) {
      const u64 s = service_ns(record_weight(a, i, false), a.cost[key]);
      if (served) {
        busy = s;
        wmax = wsum = w;
      } else {
        refused = s;
        drops = 1u;
        ahead = 0u;  // (the maximum runs over served records)
      }
    }
  }
  if (!a.out.busy && !a.out.wmax && !a.out.wsum && !a.out.amax) return;  // (the same for every lane)
  const bool first = wave_run_first(key);
  const auto run_max = [](auto x, auto y) { return max(x, y); };
  if (a.out.busy) {
    busy = wave_run_reduce(key, busy, ScanPlus());
    refused = wave_run_reduce(key, refused, ScanPlus());
    if (first && busy) atomicAdd(&a.out.busy[key], busy);
    if (first && refused) atomicAdd(&d.refused[key], refused);
  }
  if (a.out.wmax) {
    wmax = wave_run_reduce(key, wmax, run_max);
    if (first && wmax) atomicMax(&a.out.wmax[key], wmax);
  }
  if (a.out.wsum) {
    wsum = wave_run_reduce(key, wsum, ScanPlus());
    if (first && wsum) atomicAdd(&a.out.wsum[key], wsum);
  }
  if (a.out.amax) {
    ahead = wave_run_reduce(key, ahead, run_max);
    drops = wave_run_reduce(key, drops, ScanPlus());
    if (first && ahead) atomicMax(&a.out.amax[key], ahead);
    if (first && drops) atomicAdd(&d.drops[key], drops);
  }
}

}  // namespace

void drop_launch_links(sg_ctx* ctx, const QArgs& a) {
  const DArgs d = drop_args(ctx, a, nullptr);
  hipLaunchKernelGGL(k_drop_links, dim3(grid_for(a.n_links, Q_THREADS)), dim3(Q_THREADS), 0, ctx->stream, d);
  SG_CHECK_LAUNCH();
}

// The walk under the drop rule, in either form: wt (returned), run and the served marks of every record.
const u64* drop_launch_walk(sg_ctx* ctx, const QArgs& a, u64* carried_run) {
  hipStream_t st = ctx->stream;
  const DArgs d = drop_args(ctx, a, carried_run);
  const dim3 g_rec(grid_for(a.n, Q_THREADS, 0x7FFFFFFFu)), blk(Q_THREADS);
  if (queue_serial(a)) {
    hipLaunchKernelGGL(k_drop_serial, dim3(grid_for(a.n_links, Q_THREADS, 16u * (unsigned)ctx->n_cu)), blk, 0, st, d);
    SG_CHECK_LAUNCH();
    return d.wt;
  }
  hipLaunchKernelGGL(k_drop_heads, dim3(queue_tiles(a)), blk, 0, st, d);
  SG_CHECK_LAUNCH();
  scan_counts(ctx, d.mark, (uint32_t)a.n, d.pos, d.pos + a.n + 1);
  SG_HIP(hipMemsetAsync(d.n_long, 0, 4, st));
  hipLaunchKernelGGL(k_drop_starts, g_rec, blk, 0, st, d);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_drop_lane, g_rec, blk, 0, st, d);
  SG_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_drop_wave, dim3(grid_for(d.lng_cap, Q_THREADS / 64u, 8u * (unsigned)ctx->n_cu)), blk, 0, st, d);
  SG_CHECK_LAUNCH();
  return d.wt;
}

// Every output the caller takes, from a walk's three arrays.
void drop_launch_finish(sg_ctx* ctx, const QArgs& a, u64* carried_run) {
  const DArgs d = drop_args(ctx, a, carried_run);
  const bool want_ahead = a.out.ahead || a.out.amax;
  if (want_ahead) scan_counts(ctx, d.mark, (uint32_t)a.n, d.pos, d.pos + a.n + 1);
  hipLaunchKernelGGL(k_drop_finish, dim3(grid_for(a.n, Q_THREADS, 0x7FFFFFFFu)), dim3(Q_THREADS), 0, ctx->stream, d,
                     want_ahead ? 1u : 0u);
  SG_CHECK_LAUNCH();
}

}  // namespace sg
