// sg_lanes.h -- what the lane-per-host kernels share (sg_codel.hip: the routers' CoDel queues;
// sg_inbound.hip: the inbound relay; sg_outbound.hip: the outbound pipeline's fifo interface;
// sg_qdisc.hip: its round-robin interface): the block shape, the contiguous chunk's staging, the
// two chunk layouts, the relay's token bucket, the per-block sums and their prefix, the outbound
// object, and the launch's choice of layout.  Each translation unit gets its own copy of the
// device code (an unnamed namespace).
#pragma once

#include <type_traits>

#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"

namespace sg {
namespace {

constexpr uint64_t CD_TARGET = 10000000ull;     // codel_queue.rs:23
constexpr uint64_t CD_INTERVAL = 100000000ull;  // codel_queue.rs:28
constexpr uint64_t CD_MTU = 1500ull;            // definitions.h:124
constexpr uint64_t EMU_MAX = ~0ull - 1;         // emulated_time.rs:30 EMUTIME_MAX
constexpr uint32_t CD_NONE = ~0u;
enum : uint8_t { F_DROP = 1, F_IEND = 2, F_DNEXT = 4 };
enum : uint32_t { E_UNSORTED = 1, E_HOST = 2, E_FULL = 16, E_PKT = 32, E_WINDOW = 64 };

__device__ __forceinline__ uint64_t sat_add(uint64_t t, uint64_t d) { return t > EMU_MAX - d ? EMU_MAX : t + d; }
__device__ __forceinline__ uint64_t since(uint64_t now, uint64_t t) { return now > t ? now - t : 0; }

// One wave per block: the walkers are the whole block.  The staging loads are
// unrolled (CD_UNROLL per array in flight per lane) so one wave moves a chunk
// in two rounds of latency.  Blocks with idle helper waves held occupancy
// (VGPRs) without walking: at C4 only 1024 of the 1563 blocks were resident,
// and the kernels ran in two rounds (SG_LANE_DIAG).
constexpr int CD_THREADS = 64;
constexpr int CD_UNROLL = 8;
constexpr int CD_HOSTS = 64;
constexpr int CD_CHUNK = 1024;
constexpr int CD_OUT_CHUNK = 896;  // k_outbound: 24 B per send, 21 KB, 7 blocks per CU
static_assert(CD_THREADS == CD_HOSTS, "a block is its walkers");

// s_waitcnt vmcnt(0) as the immediate of __builtin_amdgcn_s_waitcnt (gfx9: lgkmcnt and expcnt
// left at their maxima)
constexpr int VMCNT0 = 0x0F70;

// Chunk [c0, c1) staged by the block: ld(i, u) loads element i into slot u of
// the lane's registers, st(k, u) stores slot u to LDS index k.  Indices past
// c1 load element c1 - 1 (always valid, unconditional loads: no branch for the
// compiler to drain each load at) and are not stored.
template <typename LD, typename ST>
__device__ __forceinline__ void stage_chunk(uint32_t c0, uint32_t c1, LD&& ld, ST&& st) {
  const uint32_t t = threadIdx.x;
  for (uint32_t base = c0; base < c1; base += CD_THREADS * CD_UNROLL) {
#pragma unroll
    for (int u = 0; u < CD_UNROLL; u++) ld(min(base + u * CD_THREADS + t, c1 - 1), u);
#pragma unroll
    for (int u = 0; u < CD_UNROLL; u++) {
      const uint32_t i = base + u * CD_THREADS + t;
      if (i < c1) st(i - c0, u);
    }
  }
}

// A block's events in chunks of CH LDS positions.  Contiguous: chunk c is the
// block's events [p0 + c CH, ...), the hosts in order -- at C4 (~20 events per
// host) a chunk holds ~50 hosts' events and every lane walks.  With hundreds of
// events per host (C5: ~200) a contiguous chunk holds ~5 hosts: 5 lanes walk
// while 59 wait, and the block's time is the sum of its hosts' chains.
// Lane-major: chunk c holds events [c LK, (c + 1) LK) of every host, host l at
// positions [l LK, l LK + LK) (holes past a host's last event), so all 64 lanes
// walk every chunk and the block's time is its busiest host's chain.  A host's
// events stay contiguous in position order, so k_codel's push / pop ranks by
// ballot work unchanged (a hole counts as a non-push position: the pop slots
// stay disjoint from the push slots).
template <bool LM, uint32_t CH = CD_CHUNK>
struct ChunkMap {
  static constexpr uint32_t LK = CH / CD_THREADS;  // lane-major: events per host per chunk
  uint32_t p0, p1;                       // the block's event range
  const uint32_t *s_hb, *s_hn;           // lane-major: per host, first event and event count (LDS)
  // chunk c exists (a loop test, not a chunk count: a count's division was hoisted above the
  // walkers' state loads, and its wait for p0 / p1 put a round trip in front of them)
  __device__ bool has(uint32_t c, uint32_t max_n) const { return LM ? c * LK < max_n : p0 + c * CH < p1; }
  // chunk c's positions [0, len)
  __device__ uint32_t len(uint32_t c) const { return LM ? CH : min(CH, p1 - p0 - c * CH); }
  // the event at position k of chunk c (a valid index even when !ok: the loads are unconditional)
  __device__ uint32_t event(uint32_t c, uint32_t k, bool& ok) const {
    if (!LM) {
      const uint32_t i = p0 + c * CH + k;
      ok = i < p1;
      return ok ? i : p1 - 1;
    }
    const uint32_t l = k / LK, o = c * LK + (k % LK), hn = s_hn[l];
    ok = o < hn;
    return ok ? s_hb[l] + o : p0;
  }
  // host lane t's positions [kb, ke) in chunk c, given its events [hb, he); ib = the event at kb
  __device__ void host_range(uint32_t c, uint32_t t, uint32_t hb, uint32_t he, uint32_t& kb, uint32_t& ke,
                             uint32_t& ib) const {
    if (LM) {
      const uint32_t o = c * LK, n = he - hb;
      kb = t * LK;
      ke = kb + (n > o ? min(LK, n - o) : 0u);
      ib = hb + o;
    } else {
      const uint32_t c0 = p0 + c * CH, c1 = min(c0 + CH, p1);
      const uint32_t b = max(hb, c0), e = min(he, c1);
      kb = b < e ? b - c0 : 0;
      ke = b < e ? e - c0 : 0;
      ib = b;
    }
  }
};

// Lane-major when it walks the block in less estimated time: a chunk costs CHUNK_COST walk
// steps of staging and barriers, plus its walk -- contiguous, about one host's share of the
// chunk (the active hosts' mean, capped at CH: its hosts are walked side by side); lane-major,
// LK steps (every host's next LK events side by side).  C5: 13 contiguous chunks of ~200 steps
// against 18 lane-major ones of 16; a partial last block (32 hosts) the same.  A block that is
// mostly one host (5,000 of its 5,006 events) stays contiguous: 313 lane-major chunks.  r05q:
// the earlier rule (lane-major chunks at most twice the contiguous ones) kept the partial last
// block of the C5 round contiguous, and it set every lane kernel's time (k_outbound 592 us walk
// against a 256 us mean).
constexpr uint32_t CHUNK_COST = 10;
template <uint32_t CH = CD_CHUNK>
__device__ __forceinline__ bool lane_major_block(int mode, uint32_t n_ev, uint32_t max_n, uint32_t h_act) {
  if (mode != 2) return mode == 1;
  constexpr uint32_t LK = CH / CD_THREADS;
  if (n_ev <= 2u * CH) return false;  // C4-like blocks: one or two contiguous chunks
  const uint32_t mean = n_ev / max(h_act, 1u);
  const uint64_t c_cost = (uint64_t)((n_ev + CH - 1) / CH) * (CHUNK_COST + min(mean, CH));
  const uint64_t l_cost = (uint64_t)((max_n + LK - 1) / LK) * (CHUNK_COST + LK);
  return l_cost < c_cost;
}

template <bool ANY>
__device__ __forceinline__ uint32_t lane_major_setup(uint32_t hb, uint32_t hn, uint32_t* s_hb, uint32_t* s_hn,
                                                     uint32_t& h_act) {
  if constexpr (!ANY) {
    h_act = 0;
    return 0;
  } else {
    uint32_t max_n = hn;
    for (int o = 32; o > 0; o >>= 1) max_n = max(max_n, (uint32_t)__shfl_xor(max_n, o, 64));
    h_act = (uint32_t)__popcll(__ballot(hn > 0));  // hosts with events in this call
    s_hb[threadIdx.x] = hb;
    s_hn[threadIdx.x] = hn;
    __syncthreads();
    return max_n;
  }
}

// Runs body(ChunkMap<LM, CH>) with the block's layout as a compile-time choice (the
// contiguous path keeps its r04 code; a runtime flag cost C4 ~1.5 us per launch)
// ANY: the kernel was launched with lane-major blocks possible (lane_major_launch).  The
// kernels launched without it keep the r04 contiguous loop verbatim instead of this one:
// walking through ChunkMap<false> cost C4 5-7 % more walk time (k_inbound 22.2 -> 23.5 us
// busiest-lane mean, k_outbound 15.0 -> 16.1, same box, SG_LANE_DIAG)
template <bool ANY, uint32_t CH = CD_CHUNK, class F>
__device__ __forceinline__ void with_chunk_map(bool lm, uint32_t p0, uint32_t p1, const uint32_t* s_hb,
                                               const uint32_t* s_hn, F&& body) {
  if constexpr (ANY) {
    if (lm) {
      body(ChunkMap<true, CH>{p0, p1, s_hb, s_hn});
      return;
    }
  }
  body(ChunkMap<false, CH>{p0, p1, s_hb, s_hn});
}

// SG_LANE_DIAG: a block's start and end on the 100 MHz wall clock (comparable
// across CUs), the cycles its walkers spent walking, and its busiest lane's events
__device__ __forceinline__ void lane_diag_store(unsigned long long* d, uint64_t t0, uint64_t walk, uint32_t ev) {
  if (!d) return;
  if (threadIdx.x < 64) {
    for (int o = 32; o > 0; o >>= 1) {
      walk = max(walk, (uint64_t)__shfl_xor((unsigned long long)walk, o, 64));
      ev = max(ev, (uint32_t)__shfl_xor(ev, o, 64));
    }
    if (threadIdx.x == 0) {
      unsigned long long* q = d + 4 * (size_t)blockIdx.x;
      q[0] = t0;
      q[1] = wall_clock64();
      q[2] = walk;
      q[3] = ev;
    }
  }
}

// ---- the relays' forward task state (relay/mod.rs, relay/token_bucket.rs) ----
constexpr uint64_t TB_INTERVAL = 1000000ull;  // relay/mod.rs:297: refill every 1 ms
enum : uint8_t { R_PENDING = 1, R_NEVER = 2, R_CACHED = 4 };

struct Relay {
  uint8_t rf;
  uint64_t tt;  // pending task time
  uint32_t cp, cl;  // cached packet, its length
  uint64_t cap, bal, inc, last;  // token bucket (token_bucket.rs:6-12)
  uint64_t n_max;                 // u64::MAX / inc (inc != 0): the refill count past which tokens saturate
  uint64_t ctr0;                  // the host's event counter at the call's start (0 without event_ctr)
  uint64_t tid, tborn;            // the pending task's event id and creation time (Event::new_local)

  // forward_later: the task is a Local event created at `now` (host.rs:690-697); its id is the
  // host counter's next value (host.rs:649-653), taken even when it lands past sim_end
  __device__ void schedule(uint64_t now, uint64_t at, uint64_t sim_end, uint64_t& ctr_inc) {
    rf |= R_PENDING;
    tid = ctr0 + ctr_inc++;
    tborn = now;
    tt = at;
    if (at >= sim_end) rf |= R_NEVER;
  }

  // inc is fixed for the call: the one u64 division by it happens here, not on every refill
  __device__ void set_inc(uint64_t v) {
    inc = v;
    n_max = v ? ~0ull / v : ~0ull;
  }
  // lazy_refill (token_bucket.rs:124-158): the span to the next refill
  __device__ uint64_t lazy_refill(uint64_t now) {
    uint64_t span = now - last;
    if (span >= TB_INTERVAL) {
      const uint64_t n = span / TB_INTERVAL;
      const uint64_t tokens = (inc != 0 && n > n_max) ? ~0ull : inc * n;
      const uint64_t b = bal > ~0ull - tokens ? ~0ull : bal + tokens;
      bal = b > cap ? cap : b;
      last = sat_add(last, n > ~0ull / TB_INTERVAL ? ~0ull : TB_INTERVAL * n);
      span = now - last;
    }
    return TB_INTERVAL - span;
  }
  // conforming_remove (token_bucket.rs:76-118)
  __device__ bool remove(uint64_t dec, uint64_t now, uint64_t& wait) {
    const uint64_t next = lazy_refill(now);
    if (bal >= dec) {
      bal -= dec;
      return true;
    }
    const uint64_t need = dec - bal;
    const uint64_t qn = need / inc;
    const uint64_t nref = qn + (need - qn * inc ? 1 : 0);
    if (nref == 1) {
      wait = next;
    } else {
      const uint64_t m = nref - 1;
      const uint64_t extra = m > ~0ull / TB_INTERVAL ? ~0ull : TB_INTERVAL * m;
      wait = next > ~0ull - extra ? ~0ull : next + extra;
    }
    return false;
  }
};

// k_outbound / k_qdisc: a host's sends out of execution order
enum : uint32_t { E_ORDER = 128 };

// Sums the blocks' drop counts, ORs their error flags (and the grouping
// check's) into the pinned host-mapped return block.  (Not every file that includes this
// header launches it, nor k_blk_offsets: hence [[maybe_unused]].)
[[maybe_unused]] __global__ void __launch_bounds__(1024) k_codel_reduce(const unsigned long long* __restrict__ blk, uint32_t n,
                                                       const uint32_t* __restrict__ group_err,
                                                       unsigned long long* __restrict__ ret) {
  __shared__ unsigned long long r[2][16];
  unsigned long long d = 0, e = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 1024) {
    d += blk[2 * i];
    e |= blk[2 * i + 1];
  }
  for (int s = 32; s > 0; s >>= 1) {
    d += __shfl_xor(d, s, 64);
    e |= __shfl_xor(e, s, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    r[0][threadIdx.x >> 6] = d;
    r[1][threadIdx.x >> 6] = e;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 16; i++) {
      d += r[0][i];
      e |= r[1][i];
    }
    ret[0] = d;
    ret[1] = e | *group_err;
  }
}

// Exclusive prefix of the k_outbound blocks' sent counts (blk[2b]) -> boff[b]:
// where each block's slice of the sent batch starts; and k_codel_reduce's sums
// (the total sent, the error flags) into the mapped return block, in the same
// launch.  One block.
[[maybe_unused]] __global__ void __launch_bounds__(1024) k_blk_offsets(const unsigned long long* __restrict__ blk, uint32_t nb,
                                                      uint32_t* __restrict__ boff,
                                                      const uint32_t* __restrict__ group_err,
                                                      unsigned long long* __restrict__ ret) {
  __shared__ uint32_t wsum[16];
  __shared__ unsigned long long esum[16];
  __shared__ uint32_t carry;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) carry = 0;
  __syncthreads();
  unsigned long long e = 0;
  for (uint32_t c0 = 0; c0 < nb; c0 += 1024) {
    const uint32_t i = c0 + t;
    const uint32_t v = i < nb ? (uint32_t)blk[2 * i] : 0;
    if (i < nb) e |= blk[2 * i + 1];
    uint32_t x = v;  // inclusive wave scan
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t w = 0; w < wv; w++) before += wsum[w];
    if (i < nb) boff[i] = before + x - v;
    __syncthreads();
    if (t == 1023) carry = before + x;
    __syncthreads();
  }
  for (int s = 32; s > 0; s >>= 1) e |= __shfl_xor(e, s, 64);
  if (lane == 0) esum[wv] = e;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 16; w++) e |= esum[w];
    ret[0] = carry;  // the sent total (k_codel_reduce's sum)
    ret[1] = e | *group_err;
  }
}

}  // namespace
}  // namespace sg

struct sg_outbound {
  sg_ctx* ctx = nullptr;
  uint32_t n = 0, cap = 0;
  uint32_t *host_ip = nullptr, *head = nullptr, *tail = nullptr, *start = nullptr, *off = nullptr;
  uint4* ring = nullptr;
  uint8_t* rflags = nullptr;
  uint64_t *task_time = nullptr, *tb_cap = nullptr, *tb_bal = nullptr, *tb_inc = nullptr, *tb_last = nullptr;
  uint64_t *task_id = nullptr, *task_born = nullptr;
  unsigned long long* ret = nullptr;  // pinned host-mapped: [sent, error flags]
  // The round-robin qdisc (sg_qdisc.hip; null on a fifo object).  `ring` then holds two halves of
  // `cap` records per host: the half half[h] names is the host's record pool, the other one
  // receives the call's forwarded records in forward order.  Socket s of host h lives at
  // qd_slot(h, s): blocks of 64 hosts, socket-major inside a block.
  uint32_t qdisc = 0, n_sock = 1;
  uint32_t *nxt = nullptr;                        // per pool slot (both halves): the socket's next record
  uint32_t *sk_head = nullptr, *sk_tail = nullptr;  // per socket: first and last pool slot (head ~0u: empty)
  uint8_t* dq = nullptr;                          // per host: the deque's ring of n_sock socket ids
  uint32_t *dq_front = nullptr, *dq_n = nullptr;  // per host: the deque's front counter and length
  uint32_t *top = nullptr, *n_live = nullptr;     // per host: the pool's bump pointer, the records queued
  uint8_t* half = nullptr;
  uint4* cached = nullptr;                        // per host: the relay's cached record (while R_CACHED)
  ~sg_outbound() {
    void* ps[] = {host_ip, head, tail, start, off, ring, rflags, task_time, task_id, task_born,
                  tb_cap, tb_bal, tb_inc, tb_last, nxt, sk_head, sk_tail, dq, dq_front, dq_n, top, n_live, half,
                  cached};
    for (void* p : ps)
      if (p) (void)hipFree(p);
    if (ret) (void)hipHostFree(ret);
  }
};

namespace sg {
// Socket (or deque entry) s of host h on a round-robin object with n_sock sockets per host
__host__ __device__ inline size_t qd_slot(uint32_t h, uint32_t s, uint32_t n_sock) {
  return ((size_t)(h >> 6) * n_sock + s) * 64 + (h & 63);
}
}  // namespace sg

// sg_codel.hip: the chunk layout a launch may use (SG_LANE_MAJOR) and the per-block timing
// diagnostic (SG_LANE_DIAG) of the lane kernels
int lane_major_env();
int lane_major_launch(int mode, size_t n_events, uint32_t nb, uint32_t ch);
// lane_major_launch's result as a compile-time LM: f(std::integral_constant<int, LM>) launches the
// kernel instantiated for it
template <class F>
inline void with_lane_mode(int lm, F&& f) {
  if (lm == 2) f(std::integral_constant<int, 2>{});
  else if (lm == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 0>{});
}
unsigned long long* lane_diag_alloc(uint32_t nb);
void lane_diag_report(hipStream_t st, const char* name, unsigned long long* d, uint32_t nb);
