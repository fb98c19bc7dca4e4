// sg_queue_packets.hip -- link queues, the packet pass (SG_LINK_QUEUE_PACKETS): a call's result folded
// onto its packets.  A layer over all three others (sg_queue.h): it runs once the per-record outputs
// stand at the input indices -- first order after queue_output_pass, carried after k_carry_scatter --
// and reads nothing else of theirs but the carried form's chain successors.
//
// Per packet p of the n_packets the call counts, behind the n records of the per-record arrays
// (include/shadow_gpu.h has the definition): delay = out_wait_ns[n + p], arrive = out_done_ns[n + p],
// where = out_ahead[n + p]; base = enter_ns[n + p] is read only.  A record's state is read from the
// sentinels of the drop rule; without the rule every record is served.
//
// Carried, one writer per cell and no atomic on an output:
//   k_packets_init   a lane per packet: where = nothing, delay = 0, arrive = base;
//   k_packets_chain  a lane per record.  The chain is served up to its drop: a served record whose
//                    successor is none or not served is the packet's last served one and stores
//                    delay; when there is no successor the packet arrived and the same lane stores
//                    arrive and where; a dropped record (a chain has at most one, and nothing is
//                    served after it) stores where and arrive.
// Windowed (prev: the chain predecessors), a record whose wait is all ones and whose ahead is
// 0xFFFFFFFF is pending, out_done_ns its re-based enter time, and its packet is in flight: the
// served record before a pending one stores where, the delay so far and the re-based base, a
// pending record that is its chain's first stores where (delay 0 and the base are k_packets_init's).
// First order there is no chain, and a served crossing downstream of a drop does not count:
//   k_packets_init   as above, with arrive = all ones: the cell is t_drop until the last kernel;
//   k_packets_tdrop  under the drop rule, a lane per record: atomicMin(t_drop, enter) for a dropped one;
//   k_packets_fold   a lane per record: a served record with enter < t_drop adds done - enter to
//                    delay (wrapping) and lowers where to "arrived"; a dropped record at t_drop
//                    lowers where to its index.  The codes are ordered so that the minimum is the
//                    answer: a record index < arrived < nothing.  It also bounds packet[i] by
//                    n_packets where there are no weights to have done so;
//   k_packets_arrive a lane per packet: arrive from where, base and delay.
// SG_LINK_QUEUE_PACKETS_INDEX = 1 takes the first-order pass through the carried form's index step instead
// (sg_queue_carry.hip: every packet's records in ascending (enter, record) order):
//   k_packets_lists  a lane per packet sums its list up to its first dropped record; the served
//                    records at the drop's own enter time that precede it in the list do not count.
// No workgroup waits on another.  The packets lost are counted a wave at a time into a flag word.
#include "sg_knobs.h"
#include "sg_queue.h"

namespace sg {
namespace {

constexpr uint32_t P_NOTHING = 0xFFFFFFFFu;  // no record of the packet
constexpr uint32_t P_ARRIVED = 0xFFFFFFFEu;
constexpr uint32_t P_IN_FLIGHT = 0xFFFFFFFDu;  // windowed: a record of the packet is pending
constexpr uint32_t P_NO_NEXT = 0xFFFFFFFFu;

struct PArgs {
  u64 n;
  uint32_t n_packets;
  uint32_t drop;  // the drop rule's sentinels tell a record's state
  const u64* enter;
  const uint32_t* packet;
  const u64* wait;  // the per-record outputs, at input indices
  const u64* done;
  const uint32_t* next;  // the carried form's chain successors; null: first order
  const uint32_t* prev;  // the windowed form's chain predecessors; null: no record is pending
  const uint32_t* ahead;
  const u64* base;
  u64* delay;
  u64* arrive;
  uint32_t* where;
  u64* flag;
};

__device__ __forceinline__ bool packets_bad(const PArgs& a) {
  return a.flag[Q_BAD_OFF] != Q_MAX || a.flag[Q_BAD_PACKET] != Q_MAX;
}

// One add per wave of the lanes with `lost`.  Every lane of the wave calls.
__device__ __forceinline__ void count_lost(const PArgs& a, bool lost) {
  const u64 m = __ballot(lost);
  if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(&a.flag[Q_LOST], (u64)__popcll(m));
}

__global__ void __launch_bounds__(Q_THREADS) k_packets_init(const PArgs a) {
  const u64 p = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (p >= a.n_packets) return;
  a.where[p] = P_NOTHING;
  a.delay[p] = 0ull;
  a.arrive[p] = a.next ? a.base[p] : Q_MAX;
}

__global__ void __launch_bounds__(Q_THREADS) k_packets_chain(const PArgs a) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  bool lost = false;
  if (i < a.n && !packets_bad(a)) {
    const uint32_t p = a.packet[i];
    if (p < a.n_packets) {
      const u64 w = a.wait[i], d = a.done[i];
      if (a.prev && w == Q_MAX && a.ahead[i] == P_NO_NEXT) {
        if (a.prev[i] == P_NO_NEXT) a.where[p] = P_IN_FLIGHT;
      } else if (!a.drop || w != Q_MAX) {
        uint32_t nx = a.next[i];
        if (nx != P_NO_NEXT && nx >= a.n) nx = P_NO_NEXT;
        const u64 delay = d - a.enter[i];
        if (a.prev && nx != P_NO_NEXT && a.wait[nx] == Q_MAX && a.ahead[nx] == P_NO_NEXT) {
          const u64 at = sat_add(a.base[p], delay);
          if (at == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], i);
          a.delay[p] = delay;
          a.arrive[p] = at;
          a.where[p] = P_IN_FLIGHT;
        } else if (nx == P_NO_NEXT) {
          const u64 at = sat_add(a.base[p], delay);
          if (at == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], i);
          a.delay[p] = delay;
          a.arrive[p] = at;
          a.where[p] = P_ARRIVED;
        } else if (a.drop && a.wait[nx] == Q_MAX) {
          a.delay[p] = delay;
        }
      } else if (d != Q_MAX) {
        a.where[p] = (uint32_t)i;
        a.arrive[p] = Q_MAX;
        lost = true;
      }
    }
  }
  count_lost(a, lost);
}

__global__ void __launch_bounds__(Q_THREADS) k_packets_tdrop(const PArgs a) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= a.n || a.flag[Q_BAD_OFF] != Q_MAX) return;
  const uint32_t p = a.packet[i];
  if (p >= a.n_packets) return;
  if (a.wait[i] == Q_MAX && a.done[i] != Q_MAX) atomicMin(&a.arrive[p], a.enter[i]);
}

__global__ void __launch_bounds__(Q_THREADS) k_packets_fold(const PArgs a) {
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= a.n || a.flag[Q_BAD_OFF] != Q_MAX) return;
  const uint32_t p = a.packet[i];
  if (p >= a.n_packets) {
    atomicMin(&a.flag[Q_BAD_PACKET], i);
    return;
  }
  const u64 e = a.enter[i], d = a.done[i];
  if (!a.drop) {
    atomicAdd(&a.delay[p], d - e);
    atomicMin(&a.where[p], P_ARRIVED);
    return;
  }
  const u64 t_drop = a.arrive[p];  // (k_packets_tdrop's, complete: no lane of this launch writes it)
  if (a.wait[i] != Q_MAX) {
    if (e < t_drop) {
      atomicAdd(&a.delay[p], d - e);
      atomicMin(&a.where[p], P_ARRIVED);
    }
  } else if (d != Q_MAX && e == t_drop) {
    atomicMin(&a.where[p], (uint32_t)i);
  }
}

__global__ void __launch_bounds__(Q_THREADS) k_packets_arrive(const PArgs a) {
  const u64 p = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  bool lost = false;
  if (p < a.n_packets && !packets_bad(a)) {
    const uint32_t w = a.where[p];
    u64 at = a.base[p];
    if (w < P_ARRIVED) {
      at = Q_MAX;
      lost = true;
    } else if (w == P_ARRIVED) {
      at = sat_add(at, a.delay[p]);
      if (at == Q_MAX) atomicMin(&a.flag[Q_PKT_OVERFLOW], p);
    }
    a.arrive[p] = at;
  }
  count_lost(a, lost);
}

// First order through the index: lists.list holds packet p's records from lists.pkt_off[p] on.
__global__ void __launch_bounds__(Q_THREADS) k_packets_lists(const PArgs a, const QChains lists) {
  const u64 p = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  bool lost = false;
  if (p < a.n_packets && !packets_bad(a)) {
    const u64 j0 = lists.pkt_off[p], j1 = min(lists.pkt_off[p + 1], a.n);
    // total: the served records before the current enter time; run: the served ones at it
    u64 total = 0ull, run = 0ull, run_enter = 0ull, at = a.base[p];
    uint32_t where = j0 < j1 ? P_ARRIVED : P_NOTHING;
    for (u64 j = j0; j < j1; j++) {
      const uint32_t i = lists.list[j];
      if (i >= a.n) continue;
      const u64 e = a.enter[i], d = a.done[i];
      if (e != run_enter) {
        total += run;
        run = 0ull;
        run_enter = e;
      }
      if (!a.drop || a.wait[i] != Q_MAX) {
        run += d - e;
      } else if (d != Q_MAX) {
        where = i;  // (the list is ascending in (enter, record): the first dropped record is drop(p))
        run = 0ull;
        break;
      }
    }
    total += run;
    if (where < P_ARRIVED) {
      at = Q_MAX;
      lost = true;
    } else if (where == P_ARRIVED) {
      at = sat_add(at, total);
      if (at == Q_MAX) atomicMin(&a.flag[Q_PKT_OVERFLOW], p);
    }
    a.where[p] = where;
    a.delay[p] = total;
    a.arrive[p] = at;
  }
  count_lost(a, lost);
}

}  // namespace

void queue_packets(sg_ctx* ctx, const QArgs& a, bool drop, const uint32_t* next, const uint32_t* prev) {
  hipStream_t st = ctx->stream;
  PArgs p = {};
  p.n = a.n;
  p.n_packets = a.n_weights;
  p.drop = drop ? 1u : 0u;
  p.enter = a.enter;
  p.packet = a.packet;
  p.wait = a.out.wait;
  p.done = a.out.done;
  p.next = next;
  p.prev = prev;
  p.ahead = a.out.ahead;
  p.base = a.enter + a.n;
  p.delay = a.out.wait + a.n;
  p.arrive = a.out.done + a.n;
  p.where = a.out.ahead + a.n;
  p.flag = a.flag;
  const dim3 g_rec(grid_for(a.n, Q_THREADS, 0x7FFFFFFFu)), g_pkt(grid_for(a.n_weights, Q_THREADS, 0x7FFFFFFFu)), blk(Q_THREADS);
  SG_HIP(hipMemsetAsync(a.flag + Q_LOST, 0, 8, st));
  if (!next && a.n && knob_int("SG_LINK_QUEUE_PACKETS_INDEX", 0) != 0) {
    const QChains lists = queue_packet_lists(ctx, a);
    TimedLaunch tl(ctx, "link_queue_packets", (double)a.n);
    hipLaunchKernelGGL(k_packets_lists, g_pkt, blk, 0, st, p, lists);
    SG_CHECK_LAUNCH();
    return;
  }
  TimedLaunch tl(ctx, "link_queue_packets", (double)a.n);
  hipLaunchKernelGGL(k_packets_init, g_pkt, blk, 0, st, p);
  SG_CHECK_LAUNCH();
  if (next) {
    if (a.n) {
      hipLaunchKernelGGL(k_packets_chain, g_rec, blk, 0, st, p);
      SG_CHECK_LAUNCH();
    }
    return;
  }
  if (a.n) {
    if (drop) {
      hipLaunchKernelGGL(k_packets_tdrop, g_rec, blk, 0, st, p);
      SG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_packets_fold, g_rec, blk, 0, st, p);
    SG_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_packets_arrive, g_pkt, blk, 0, st, p);
  SG_CHECK_LAUNCH();
}

}  // namespace sg
