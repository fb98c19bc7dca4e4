// sg_codel.hip -- the routers' inbound CoDel queues, one per host, on the device.
//
// Router::inbound_packets (router/mod.rs:15-58) is a CoDelQueue
// (router/codel_queue.rs): RFC 8289 with Shadow's TARGET = 10 ms and
// INTERVAL = 100 ms, no LIMIT, "good state" while at most one MTU (1500 B,
// definitions.h:124) is stored.  A host's queue is a sequential state machine,
// but hosts are independent: a batch of push / pop events runs one lane per
// host, k_walk-style -- a block owns 64 consecutive hosts, whose events are one
// contiguous range staged through LDS in chunks (coalesced loads, per-host
// sequential processing, coalesced pop results).  The FIFO of each host is a
// ring of `cap` slots in HBM (packet id, enqueue time, length); the scalar
// CoDel state is kept in registers for the whole call.  The queue itself is
// sg_codel_queue.h (shared with the inbound pipeline, sg_inbound.hip).  Also
// here: the lane kernels' host helpers (SG_LANE_MAJOR, SG_LANE_DIAG).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_codel_queue.h"
#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_lanes.h"

namespace sg {
namespace {

// LM: the chunk layouts this launch may use (lane_major_launch): 0 contiguous only, 1 lane-major
// only, 2 per block (lane_major_block).  A template parameter, not an argument: a field added to
// the argument structs changed k_inbound's register allocation and cost C4 ~2 us.
template <int LM>
__global__ void __launch_bounds__(CD_THREADS) k_codel(CodelArgs a) {
  constexpr bool ANY = LM != 0;
  const uint64_t d_t0 = a.bdiag ? wall_clock64() : 0;
  uint64_t d_walk = 0;
  // Staged chunk, 18 KB (8 one-wave blocks fit a CU): the chunk's pushes in push order
  // from the front of s_t / s_p / s_l (time, packet, length), its pops in pop order from
  // the back (time, result, pushes before the pop), so a walk step reads its element and
  // its next pop's fields directly -- no index list between (r03: an index read, then the
  // data, at every pop and every push accounted)
  __shared__ uint64_t s_t[CD_CHUNK];
  __shared__ uint32_t s_p[CD_CHUNK];
  __shared__ uint32_t s_l[CD_CHUNK];
  __shared__ uint16_t s_pp[CD_CHUNK + 1];  // pushes before each staged event (kind k = s_pp[k + 1] - s_pp[k])
  auto pop_at = [](uint32_t r) { return (uint32_t)CD_CHUNK - 1u - r; };  // the r-th pop's slot
  const uint32_t h0 = blockIdx.x * CD_HOSTS, t = threadIdx.x;
  const uint32_t p0 = min(a.host_off[min(h0, a.H)], a.E);
  const uint32_t p1 = max(min(a.host_off[min(h0 + CD_HOSTS, a.H)], a.E), p0);
  const uint32_t h = h0 + t;
  const bool walker = t < CD_HOSTS && h < a.H;
  uint32_t hb = 0, he = 0;
  Q<LM != 0> q{};
  if (walker) {
    hb = min(a.host_off[h], a.E);
    he = max(min(a.host_off[h + 1], a.E), hb);
    q.flags = a.flags[h];
    q.iend = a.iend[h];
    q.dnext = a.dnext[h];
    q.cur = a.cur[h];
    q.prev = a.prev[h];
    q.bytes = a.bytes[h];
    q.head = a.head[h];
    q.tail = a.tail[h];
    q.ring = a.ring + (size_t)h * a.cap;
    q.mask = a.cap - 1;
    q.status = a.status;
    q.n_status = a.n_status;
    q.load_head();
  }
  const uint64_t lt = (1ull << t) - 1;  // lanes below this one
  // 2. each host's pops in order, over its staged positions [kb, ke) of the chunk in LDS (both
  // chunk loops below, after their staging barrier).  A host's pushes between two pops only
  // append (tail, bytes): they are accounted at the next pop, the elements
  // read from the staged window, and the ring is written at the chunk's end
  // for the elements still queued -- the walk's steps are the pops alone.
  // (The walk reads no field of `a`: a lambda that captures the argument struct keeps the
  // compiler from marking k_codel<0>'s argument loads unclobbered, and its hosts' offsets and
  // state then come through vector loads -- C4 busiest-lane walk 14.98 -> 15.16 us.)
  const bool diag = a.bdiag != nullptr;
  auto walk = [&](uint32_t kb, uint32_t ke) {
    const uint64_t d_w0 = diag ? clock64() : 0;
    const uint32_t pb = kb < ke ? s_pp[kb] : 0, pe = kb < ke ? s_pp[ke] : 0;
    const uint32_t rb = kb - pb, re = ke - pe;  // this host's pop ranks [rb, re)
    // the window's j-th push is push slot pb + j
    q.begin_window((lds_u32*)s_p, (lds_u32*)s_l, (lds_u64*)s_t, pb);
    uint32_t seen = 0;  // window pushes accounted
    auto account = [&](uint32_t upto) {  // the window's pushes [seen, upto) enter the queue
      for (; seen < upto; seen++) q.bytes += s_l[pb + seen];
      q.tail = q.t0 + upto;
      if (q.tail - q.head > q.mask + 1u) q.err |= E_FULL;  // a push found the ring full
      if (!q.hv) q.load_head();
    };
    // the next pop's fields are read a step ahead
    uint64_t t1 = rb < re ? s_t[pop_at(rb)] : 0;
    uint32_t pp1 = rb < re ? s_l[pop_at(rb)] : 0;
    for (uint32_t r = rb; r < re; r++) {
      const uint32_t k = pop_at(r), pp = pp1;
      const uint64_t now = t1;
      if (r + 1 < re) {
        t1 = s_t[pop_at(r + 1)];
        pp1 = s_l[pop_at(r + 1)];
      }
      account(pp - pb);
      const uint32_t res = q.pop(now);
      // a dequeued packet's status is written with the chunk's results (3. below): a
      // global store here made the walk's next vector-memory wait (the ring prefetch,
      // or a register the compiler shares with it) wait for the store too
      if (res != CD_NONE && res >= q.n_status) q.err |= E_PKT;
      s_p[k] = res;  // a pop's packet slot is read by no one else
    }
    account(pe - pb);
    // the window's elements still queued live on in the ring
    const uint32_t w0 = q.head - q.t0 <= q.tail - q.t0 ? q.head - q.t0 : 0;
    for (uint32_t j = w0; j < q.tail - q.t0; j++) {
      const uint32_t k = pb + j;
      const uint64_t tk = s_t[k];
      q.ring[(q.t0 + j) & q.mask] = make_uint4(s_p[k], s_l[k], (uint32_t)tk, (uint32_t)(tk >> 32));
    }
    if (diag) d_walk += clock64() - d_w0;
    q.win = false;  // the next chunk's staging overwrites the window (the head stays cached)
  };
  if constexpr (!ANY) {  // contiguous chunks only: the r04 loop as it was (see with_chunk_map)
  for (uint32_t c0 = p0; c0 < p1; c0 += CD_CHUNK) {
    const uint32_t c1 = min(c0 + CD_CHUNK, p1);
    {  // 1. coalesced staging, and the chunk's push and pop lists by ballot (the block is one wave)
      uint32_t run = 0;
      for (uint32_t base = c0; base < c1; base += CD_THREADS * CD_UNROLL) {
        uint64_t rt[CD_UNROLL];
        uint32_t rp[CD_UNROLL], rl[CD_UNROLL];
        uint8_t rk[CD_UNROLL];
#pragma unroll
        for (int u = 0; u < CD_UNROLL; u++) {
          const uint32_t i = min(base + u * CD_THREADS + t, c1 - 1);
          rt[u] = a.time[i];
          rp[u] = a.pkt[i];
          rl[u] = a.len[i];
          rk[u] = a.kind[i];
        }
#pragma unroll
        for (int u = 0; u < CD_UNROLL; u++) {
          const uint32_t i = base + u * CD_THREADS + t;
          const bool in = i < c1, push = in && rk[u] == SG_CODEL_PUSH;
          const uint64_t m = __ballot(push);
          const uint32_t rank = run + (uint32_t)__popcll(m & lt);
          if (in) {
            const uint32_t k = i - c0;
            const uint32_t slot = push ? rank : pop_at(k - rank);
            s_t[slot] = rt[u];
            s_p[slot] = rp[u];
            s_l[slot] = push ? rl[u] : rank;
            s_pp[k] = (uint16_t)rank;
          }
          run += (uint32_t)__popcll(m);
        }
      }
      if (t == 0) s_pp[c1 - c0] = (uint16_t)run;
    }
    __syncthreads();
    if (walker) {
      // this host's staged range [kb, ke) (empty when its events lie outside the chunk)
      const uint32_t b = max(hb, c0), e = min(he, c1);
      walk(b < e ? b - c0 : 0, b < e ? e - c0 : 0);
    }
    __syncthreads();
    for (uint32_t i = c0 + t; i < c1; i += CD_THREADS) {  // 3. coalesced results (CD_NONE for a push)
      const uint32_t k = i - c0;
      const uint32_t r = s_pp[k + 1] != s_pp[k] ? CD_NONE : s_p[pop_at(k - s_pp[k])];
      a.pop_result[i] = r;
      if (r < a.n_status) a.status[r] = SG_CODEL_DEQUEUED;  // (CD_NONE >= n_status)
    }
    __syncthreads();
  }
  } else {
  __shared__ uint32_t s_hb[CD_HOSTS], s_hn[CD_HOSTS];
  const uint32_t hn = he - hb;
  uint32_t h_act;
  const uint32_t max_n = lane_major_setup<ANY>(hb, hn, s_hb, s_hn, h_act);
  with_chunk_map<ANY>(ANY && lane_major_block(LM, p1 - p0, max_n, h_act), p0, p1, s_hb, s_hn, [&](auto cm) {
  // A chunk's events are loaded into registers a chunk ahead (CD_PF per lane, one round of
  // loads): the next chunk's loads are in flight during this chunk's walk.  At C5 a block walks
  // ~19 lane-major chunks, and each chunk's staging round trips sat in front of its walk.
  constexpr int CD_PF = CD_CHUNK / CD_THREADS;
  uint64_t rt[CD_PF];
  uint32_t rp[CD_PF], rl[CD_PF];
  uint8_t rk[CD_PF];
  bool ok[CD_PF];
  auto fetch = [&](uint32_t f) {
#pragma unroll
    for (int u = 0; u < CD_PF; u++) {
      const uint32_t i = cm.event(f, u * CD_THREADS + t, ok[u]);
      rt[u] = a.time[i];
      rp[u] = a.pkt[i];
      rl[u] = a.len[i];
      rk[u] = a.kind[i];
    }
  };
  if (cm.has(0, max_n)) fetch(0);
  for (uint32_t c = 0; cm.has(c, max_n); c++) {
    const uint32_t clen = cm.len(c);
    {  // 1. staging from the registers (the chunk's range, or 16-event runs per host), and the
       //    chunk's push and pop lists by ballot (the block is one wave)
      uint32_t run = 0;
#pragma unroll
      for (int u = 0; u < CD_PF; u++) {
        const uint32_t k = u * CD_THREADS + t;
        const bool in = k < clen, push = in && ok[u] && rk[u] == SG_CODEL_PUSH;
        const uint64_t m = __ballot(push);
        const uint32_t rank = run + (uint32_t)__popcll(m & lt);
        if (in) {
          const uint32_t slot = push ? rank : pop_at(k - rank);
          if (ok[u]) {
            s_t[slot] = rt[u];
            s_p[slot] = rp[u];
            s_l[slot] = push ? rl[u] : rank;
          }
          s_pp[k] = (uint16_t)rank;
        }
        run += (uint32_t)__popcll(m);
      }
      if (t == 0) s_pp[clen] = (uint16_t)run;
    }
    if (cm.has(c + 1, max_n)) fetch(c + 1);  // (uniform) in flight during the walk
    __syncthreads();
    if (walker) {
      // this host's staged positions [kb, ke) (empty when none of its events is in the chunk)
      uint32_t kb, ke, ib;
      cm.host_range(c, t, hb, he, kb, ke, ib);
      (void)ib;
      walk(kb, ke);
    }
    __syncthreads();
    for (uint32_t k = t; k < clen; k += CD_THREADS) {  // 3. results (CD_NONE for a push)
      bool ok;
      const uint32_t i = cm.event(c, k, ok);
      if (!ok) continue;
      const uint32_t r = s_pp[k + 1] != s_pp[k] ? CD_NONE : s_p[pop_at(k - s_pp[k])];
      a.pop_result[i] = r;
      if (r < a.n_status) a.status[r] = SG_CODEL_DEQUEUED;  // (CD_NONE >= n_status)
    }
    __syncthreads();
  }
  });
  }
  unsigned long long dropped = 0, err = 0;
  if (walker) {
    a.flags[h] = q.flags;
    a.iend[h] = q.iend;
    a.dnext[h] = q.dnext;
    a.cur[h] = q.cur;
    a.prev[h] = q.prev;
    a.bytes[h] = q.bytes;
    a.head[h] = q.head;
    a.tail[h] = q.tail;
    dropped = q.dropped;
    err = q.err;
  }
  lane_diag_store(a.bdiag, d_t0, d_walk, he - hb);
  if (t < 64) {
    for (int d = 32; d > 0; d >>= 1) {
      dropped += __shfl_xor(dropped, d, 64);
      err |= __shfl_xor(err, d, 64);
    }
    if (t == 0) {
      a.blk[2 * blockIdx.x] = dropped;
      a.blk[2 * blockIdx.x + 1] = err;
    }
  }
}

}  // namespace
}  // namespace sg

extern "C" {

int32_t sg_codel_create(sg_ctx* ctx, uint32_t n_hosts, uint32_t ring_cap, sg_codel** out) {
  if (!out) return SG_ERR_INVALID_ARG;
  *out = nullptr;
  sg_codel* q = nullptr;
  int32_t rc = sg::guarded(ctx, [&] {
    using namespace sg;
    if (ring_cap == 0 || ring_cap > (1u << 30)) throw Error(SG_ERR_INVALID_ARG, "ring_cap must be in [1, 2^30]");
    uint32_t cap = 1;
    while (cap < ring_cap) cap <<= 1;
    q = new sg_codel();
    q->ctx = ctx;
    q->n = n_hosts;
    q->cap = cap;
    const size_t n = std::max<uint32_t>(n_hosts, 1), r = n * cap;
    SG_HIP(hipMalloc(&q->flags, n));
    SG_HIP(hipMalloc(&q->iend, n * 8));
    SG_HIP(hipMalloc(&q->dnext, n * 8));
    SG_HIP(hipMalloc(&q->cur, n * 8));
    SG_HIP(hipMalloc(&q->prev, n * 8));
    SG_HIP(hipMalloc(&q->bytes, n * 8));
    SG_HIP(hipMalloc(&q->head, n * 4));
    SG_HIP(hipMalloc(&q->tail, n * 4));
    SG_HIP(hipMalloc(&q->ring, r * 16));
    SG_HIP(hipHostMalloc(&q->ret, 16, hipHostMallocMapped | hipHostMallocCoherent));
    hipStream_t st = ctx->stream;  // CoDelQueue::new (codel_queue.rs:85-95): empty, Store mode, no times
    SG_HIP(hipMemsetAsync(q->flags, 0, n, st));
    void* z8[] = {q->iend, q->dnext, q->cur, q->prev, q->bytes};
    for (void* p : z8) SG_HIP(hipMemsetAsync(p, 0, n * 8, st));
    SG_HIP(hipMemsetAsync(q->head, 0, n * 4, st));
    SG_HIP(hipMemsetAsync(q->tail, 0, n * 4, st));
    SG_HIP(hipStreamSynchronize(st));
  });
  if (rc != SG_OK) {
    delete q;
    return rc;
  }
  *out = q;
  return SG_OK;
}

void sg_codel_destroy(sg_codel* q) {
  if (!q) return;
  if (q->ctx) (void)hipSetDevice(q->ctx->device);
  delete q;
}

uint32_t sg_codel_ring_cap(const sg_codel* q) { return q ? q->cap : 0; }

}  // extern "C"

// SG_LANE_MAJOR: the chunk layout of the lane kernels (ChunkMap): 0 contiguous, 1 lane-major,
// unset / 2 by each block's event count (tests force both on the same events)
int lane_major_env() {
  return sg::knob_int("SG_LANE_MAJOR", 2, 0, 2);
}

// The lane-major layout is compiled into a launch when forced (SG_LANE_MAJOR=1) or when
// the blocks average more than two contiguous chunks of ch events (C5: ~12.8k codel events
// per block; C4: ~1.3k, which keeps the contiguous-only kernel)
int lane_major_launch(int mode, size_t n_events, uint32_t nb, uint32_t ch) {
  return mode == 1 ? 1 : (mode == 2 && n_events > 2ull * ch * nb) ? 2 : 0;
}

// SG_LANE_DIAG=1: per-block timing of the lane-per-host kernels on stderr (a
// diagnostic: a synchronous copy after the launch; never set in a measured run)
unsigned long long* lane_diag_alloc(uint32_t nb) {
  if (sg::knob_int("SG_LANE_DIAG", 0) == 0) return nullptr;
  unsigned long long* d = nullptr;
  SG_HIP(hipMalloc(&d, (size_t)nb * 32));
  SG_HIP(hipMemset(d, 0, (size_t)nb * 32));
  return d;
}
void lane_diag_report(hipStream_t st, const char* name, unsigned long long* d, uint32_t nb) {
  if (!d) return;
  std::vector<unsigned long long> h((size_t)nb * 4);
  SG_HIP(hipStreamSynchronize(st));
  SG_HIP(hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost));
  (void)hipFree(d);
  uint64_t t_min = ~0ull, t_max = 0, s_max = 0;
  std::vector<double> dur(nb), walk(nb), ev(nb);
  for (uint32_t b = 0; b < nb; b++) {
    t_min = std::min<uint64_t>(t_min, h[4 * b]);
    t_max = std::max<uint64_t>(t_max, h[4 * b + 1]);
  }
  for (uint32_t b = 0; b < nb; b++) {
    s_max = std::max<uint64_t>(s_max, h[4 * b] - t_min);
    dur[b] = (h[4 * b + 1] - h[4 * b]) * 0.01;  // 100 MHz -> us
    walk[b] = h[4 * b + 2] / 2400.0;              // shader clock cycles -> us at ~2.4 GHz
    ev[b] = (double)h[4 * b + 3];
  }
  auto q = [](std::vector<double> v, double f) {
    std::sort(v.begin(), v.end());
    return v[(size_t)std::min<double>(v.size() - 1, f * v.size())];
  };
  double mw = 0, me = 0;
  for (uint32_t b = 0; b < nb; b++) mw += walk[b] / nb, me += ev[b] / nb;
  uint32_t slow = 0;  // the slowest block (its hosts are [64 slow, 64 slow + 64))
  for (uint32_t b = 1; b < nb; b++)
    if (dur[b] > dur[slow]) slow = b;
  fprintf(stderr,
          "[lane] %s: %u blocks, span %.2f us, last start +%.2f us; block us p50 %.2f p90 %.2f max %.2f; "
          "walk us (busiest lane) mean %.2f max %.2f; busiest-lane events mean %.1f max %.0f; slowest block %u "
          "(walk %.2f us, busiest lane %.0f events)\n",
          name, nb, (t_max - t_min) * 0.01, s_max * 0.01, q(dur, 0.5), q(dur, 0.9), q(dur, 1.0), mw, q(walk, 1.0), me,
          q(ev, 1.0), slow, walk[slow], ev[slow]);
}

extern "C" {

int32_t sg_codel_run(sg_ctx* ctx, sg_codel* q, const sg_codel_events* ev, uint32_t* pop_result,
                     uint8_t* pkt_status, uint32_t n_packets, uint64_t* n_dropped) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (!q || q->ctx != ctx || !ev) throw Error(SG_ERR_INVALID_ARG, "null argument");
    const uint32_t E = ev->n_events, H = q->n;
    if (n_dropped) *n_dropped = 0;
    if (!E) return;
    if (!ev->host || !ev->kind || !ev->time_ns || !ev->packet || !ev->len || !pop_result ||
        (n_packets && !pkt_status))
      throw Error(SG_ERR_INVALID_ARG, "null event or output array");
    hipStream_t st = ctx->stream;
    uint32_t* ws = ctx->d_seg.get<uint32_t>((size_t)H + 8);  // [offsets H+1][grouping error]
    uint32_t* gerr = ws + (size_t)H + 1;
    SG_HIP(hipMemsetAsync(gerr, 0, 4, st));
    launch_group_offsets(ctx, ev->host, E, H, ws, gerr);
    const uint32_t nb = std::max<uint32_t>(1, (H + CD_HOSTS - 1) / CD_HOSTS);
    CodelArgs a{ws, H, E, ev->kind, ev->time_ns, ev->packet, ev->len, q->flags, q->iend, q->dnext, q->cur,
                q->prev, q->bytes, q->head, q->tail, q->ring, q->cap, pop_result,
                pkt_status, n_packets, ctx->d_blk.get<unsigned long long>(2 * (size_t)nb)};
    a.bdiag = lane_diag_alloc(nb);
    {
      // per event: 17 B in, 4 B result, ring slot 16 B written (push) or read (pop), 1 B status
      TimedLaunch tl(ctx, "codel", 38.0 * E + 56.0 * H);
      const int lm = lane_major_launch(lane_major_env(), E, nb, CD_CHUNK);
      with_lane_mode(lm, [&](auto m) {
        hipLaunchKernelGGL(k_codel<decltype(m)::value>, dim3(nb), dim3(CD_THREADS), 0, st, a);
      });
    }
    lane_diag_report(st, "k_codel", a.bdiag, nb);
    hipLaunchKernelGGL(k_codel_reduce, dim3(1), dim3(1024), 0, st, a.blk, nb, gerr, q->ret);
    SG_CHECK_LAUNCH();
    SG_HIP(hipStreamSynchronize(st));
    const volatile unsigned long long* r = q->ret;
    const uint64_t err = r[1];
    if (err & E_UNSORTED) throw Error(SG_ERR_UNSORTED, "CoDel events must be grouped by ascending host");
    if (err & E_HOST) throw Error(SG_ERR_INVALID_ARG, "CoDel event host out of range");
    if (err & E_FULL) throw Error(SG_ERR_CAPACITY, "a CoDel queue outgrew its ring (raise ring_cap)");
    if (err & E_PKT) throw Error(SG_ERR_INVALID_ARG, "CoDel packet id >= n_packets");
    if (n_dropped) *n_dropped = r[0];
  });
}

int32_t sg_codel_get_state(sg_codel* q, sg_codel_state* o) {
  if (!q || !o) return SG_ERR_INVALID_ARG;
  return sg::guarded(q->ctx, [&] {
    const size_t n = q->n, r = n * q->cap;
    hipStream_t st = q->ctx->stream;
    struct { void* h; const void* d; size_t b; } cp[] = {
        {o->flags, q->flags, n}, {o->interval_end, q->iend, n * 8}, {o->drop_next, q->dnext, n * 8},
        {o->cur_drops, q->cur, n * 8}, {o->prev_drops, q->prev, n * 8}, {o->bytes, q->bytes, n * 8},
        {o->head, q->head, n * 4}, {o->tail, q->tail, n * 4}};
    for (auto& c : cp)
      if (c.h && c.b) SG_HIP(hipMemcpyAsync(c.h, c.d, c.b, hipMemcpyDeviceToHost, st));
    std::vector<uint4> ring(r);
    if (r) SG_HIP(hipMemcpyAsync(ring.data(), q->ring, r * 16, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < r; i++) {
      if (o->ring_packet) o->ring_packet[i] = ring[i].x;
      if (o->ring_len) o->ring_len[i] = ring[i].y;
      if (o->ring_time) o->ring_time[i] = ((uint64_t)ring[i].w << 32) | ring[i].z;
    }
  });
}

int32_t sg_codel_set_state(sg_codel* q, const sg_codel_state* in) {
  if (!q || !in) return SG_ERR_INVALID_ARG;
  return sg::guarded(q->ctx, [&] {
    const size_t n = q->n, r = n * q->cap;
    hipStream_t st = q->ctx->stream;
    struct { void* d; const void* h; size_t b; } cp[] = {
        {q->flags, in->flags, n}, {q->iend, in->interval_end, n * 8}, {q->dnext, in->drop_next, n * 8},
        {q->cur, in->cur_drops, n * 8}, {q->prev, in->prev_drops, n * 8}, {q->bytes, in->bytes, n * 8},
        {q->head, in->head, n * 4}, {q->tail, in->tail, n * 4}};
    for (auto& c : cp)
      if (c.h && c.b) SG_HIP(hipMemcpyAsync(c.d, c.h, c.b, hipMemcpyHostToDevice, st));
    if (in->ring_packet && in->ring_time && in->ring_len && r) {
      std::vector<uint4> ring(r);
      for (size_t i = 0; i < r; i++)
        ring[i] = make_uint4(in->ring_packet[i], in->ring_len[i], (uint32_t)in->ring_time[i],
                             (uint32_t)(in->ring_time[i] >> 32));
      SG_HIP(hipMemcpyAsync(q->ring, ring.data(), r * 16, hipMemcpyHostToDevice, st));
      SG_HIP(hipStreamSynchronize(st));  // before `ring` goes out of scope
    }
    SG_HIP(hipStreamSynchronize(st));
  });
}

}  // extern "C"
