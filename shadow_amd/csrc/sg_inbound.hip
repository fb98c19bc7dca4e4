// sg_inbound.hip -- the inbound pipeline: each host's router CoDel queue (sg_codel_queue.h) and
// the inbound relay's token bucket behind it (sg_lanes.h), one lane per host over a window of
// simulated time.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

#include "sg_codel_queue.h"
#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_lanes.h"

namespace sg {
namespace {

// ---- inbound pipeline: router CoDel queue -> relay_inet_in ---------------
// Per host over a window of simulated time (relay/mod.rs:72-288,
// relay/token_bucket.rs, host.rs:781-786, :919-924): each arrival (a Packet
// event, in EventQueue order) pushes into the host's CoDel queue and notifies
// the inbound relay; an Idle relay schedules its forward task at that time (a
// Local event: after the Packet events of the same time, event.rs:103-112; it
// takes an event id, host.rs:649-653).  The task pops until the queue is empty
// or the token bucket blocks, then reschedules itself after the conforming
// duration.  Tasks at or after the window end stay pending for the next call.

struct InboundArgs {
  CodelArgs q;  // queues; q.kind unused (every event is an arrival)
  uint8_t* rflags;
  uint64_t* task_time;
  uint32_t *cached_pkt, *cached_len;
  uint64_t *tb_cap, *tb_bal, *tb_inc, *tb_last;
  uint64_t window_end, bootstrap_end, sim_end;
  uint64_t* event_ctr;  // per host, or null
  uint64_t* fwd_time;   // per packet
  uint64_t *task_id, *task_born;  // per host: the pending task's event id and creation time
  uint8_t* arr_status;  // ORD: per arrival
  uint64_t* arr_fwd;
};

// The relay's forward task at `now` (run_forward_task -> forward_until_blocked).
template <class QT>
__device__ void relay_task(QT& q, Relay& r, uint64_t now, uint64_t bootstrap_end, uint64_t sim_end,
                           uint64_t& ctr_inc, uint64_t* fwd_time) {
  r.rf &= (uint8_t)~R_PENDING;
  for (;;) {
    uint32_t p, l;
    if (r.rf & R_CACHED) {
      p = r.cp;
      l = r.cl;
      r.rf &= (uint8_t)~R_CACHED;
    } else {
      const uint32_t popped = q.pop(now);
      if (popped == CD_NONE) return;  // empty: Idle
      p = popped;
      l = q.last_len;  // the popped element is the last one pop_front returned
    }
    uint64_t wait;
    if (now >= bootstrap_end && !r.remove(l, now, wait)) {  // Worker::is_bootstrapping: no rate limit
      r.rf |= R_CACHED;  // RelayCached; forward_later(wait)
      r.cp = p;
      r.cl = l;
      r.schedule(now, now > ~0ull - wait ? ~0ull : now + wait, sim_end, ctr_inc);
      return;
    }
    if (QT::ord && (p & ARR_BIT)) {  // RelayForwarded, an arrival of this call: at its index
      if ((p & ~ARR_BIT) < q.n_arr) {
        q.astat[p & ~ARR_BIT] = SG_CODEL_DEQUEUED;
        q.afwd[p & ~ARR_BIT] = now;
      } else {
        q.err |= E_PKT;
      }
    } else if (p < q.n_status) {  // RelayForwarded: pushed to the internet interface
      q.status[p] = SG_CODEL_DEQUEUED;
      fwd_time[p] = now;
    } else {
      q.err |= E_PKT;
    }
  }
}

template <int LM, bool ORD = false>
__global__ void __launch_bounds__(CD_THREADS) k_inbound(InboundArgs ia) {
  constexpr bool ANY = LM != 0;
  const uint64_t d_t0 = ia.q.bdiag ? wall_clock64() : 0;
  uint64_t d_walk = 0;
  const CodelArgs& a = ia.q;
  __shared__ uint64_t s_t[CD_CHUNK];
  __shared__ uint32_t s_p[CD_CHUNK];
  __shared__ uint32_t s_l[CD_CHUNK];
  const uint32_t h0 = blockIdx.x * CD_HOSTS, t = threadIdx.x;
  const uint32_t p0 = min(a.host_off[min(h0, a.H)], a.E);
  const uint32_t p1 = max(min(a.host_off[min(h0 + CD_HOSTS, a.H)], a.E), p0);
  const uint32_t h = h0 + t;
  const bool walker = t < CD_HOSTS && h < a.H;
  uint32_t hb = 0, he = 0;
  Q<false, ORD> q{};
  Relay r{};
  uint64_t ctr_inc = 0;
  uint32_t tail0 = 0;  // ORD: the tail at the call's start (later elements carry arrival indices)
  bool id_bad = false;  // !ORD: a staged packet id at or past n_packets (refused when it is pushed: E_PKT)
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
    q.astat = ia.arr_status;
    q.afwd = ia.arr_fwd;
    q.n_arr = a.E;
    tail0 = q.tail;
    q.load_head();
    r.rf = ia.rflags[h];
    r.tt = ia.task_time[h];
    r.cp = ia.cached_pkt[h];
    r.cl = ia.cached_len[h];
    r.cap = ia.tb_cap[h];
    r.bal = ia.tb_bal[h];
    r.set_inc(ia.tb_inc[h]);
    r.last = ia.tb_last[h];
    r.ctr0 = ia.event_ctr ? ia.event_ctr[h] : 0;
    r.tid = ia.task_id[h];
    r.tborn = ia.task_born[h];
  }
  auto due = [&](uint64_t before) {  // a pending task earlier than `before` (Packet events go first)
    return (r.rf & R_PENDING) && !(r.rf & R_NEVER) && r.tt < before;
  };
  // The per-host walk under `if (walker)` stands twice, word for word: here and in the
  // with_chunk_map loop (an edit to one goes into the other).  k_codel calls one lambda from
  // both loops; here that form cost C4 time with the same registers.  As written, the lambda
  // turned `due`'s `&&` into a branch in the walk's loop and k_inbound<0> reloaded ~170 more
  // spilled scalars per pass: 42.4-43.3 us per launch with the two copies against 48.4-49.8 us,
  // busiest-lane walk mean 21.5 against 25.0 us.  With a branch-free `due` the spills matched
  // and it came to 43.2-44.4 us and 21.62-21.64 us over three sessions: still above the two
  // copies' own spread (21.45-21.52 us), so they stay (one MI355X, libraries alternated,
  // SG_LANE_DIAG apart; profiles/lane_walk_ab.json).
  if constexpr (!ANY) {  // contiguous chunks only: the r04 loop as it was (see with_chunk_map)
  for (uint32_t c0 = p0; c0 < p1; c0 += CD_CHUNK) {
    const uint32_t c1 = min(c0 + CD_CHUNK, p1);
    {
      uint64_t rt[CD_UNROLL];
      uint32_t rp[CD_UNROLL], rl[CD_UNROLL];
      stage_chunk(
          c0, c1,
          [&](uint32_t i, int u) {
            rt[u] = a.time[i];
            rp[u] = ORD ? (ARR_BIT | i) : a.pkt[i];
            if (!ORD) id_bad |= rp[u] >= a.n_status;
            rl[u] = a.len[i];
          },
          [&](uint32_t k, int u) {
            s_t[k] = rt[u];
            s_p[k] = rp[u];
            s_l[k] = rl[u];
          });
    }
    __syncthreads();
    if (walker) {
      const uint32_t b = max(hb, c0), e = min(he, c1);
      const uint64_t d_w0 = a.bdiag ? clock64() : 0;
      q.win = false;  // the tasks first run by this chunk pop the previous chunk's elements from HBM
      q.begin_window((lds_u32*)s_p, (lds_u32*)s_l, (lds_u64*)s_t, b - c0);
      uint64_t nt = b < e ? s_t[b - c0] : 0;  // the next arrival's fields, read ahead
      uint32_t np = b < e ? s_p[b - c0] : 0, nl = b < e ? s_l[b - c0] : 0;
      for (uint32_t i = b; i < e; i++) {
        const uint32_t k = i - c0;
        const uint64_t now = nt;
        const uint32_t pkt = np, len = nl;
        if (i + 1 < e) {
          nt = s_t[k + 1];
          np = s_p[k + 1];
          nl = s_l[k + 1];
        }
        if (now >= ia.window_end) q.err |= E_WINDOW;
        while (due(now)) relay_task(q, r, r.tt, ia.bootstrap_end, ia.sim_end, ctr_inc, ia.fwd_time);
        // Router::route_incoming_packet: the arrival is the window's next element (staged
        // slot k, read from LDS when it reaches the head); the ring receives the window's
        // still-queued elements at the chunk's end, as in k_codel -- a ring store per
        // arrival made the walk's next vector-memory wait include it
        (void)pkt;
        q.tail++;
        q.bytes += len;
        if (q.tail - q.head > q.mask + 1u) q.err |= E_FULL;  // an arrival found the ring full
        if (!q.hv) q.load_head();
        if (!(r.rf & R_PENDING)) r.schedule(now, now, ia.sim_end, ctr_inc);  // notify: Idle -> forward_later(ZERO)
      }
      // the window's elements still queued live on in the ring
      const uint32_t w0 = q.head - q.t0 <= q.tail - q.t0 ? q.head - q.t0 : 0;
      for (uint32_t j = w0; j < q.tail - q.t0; j++) {
        const uint32_t k = q.wb + j;
        const uint64_t tk = s_t[k];
        q.ring[(q.t0 + j) & q.mask] = make_uint4(s_p[k], s_l[k], (uint32_t)tk, (uint32_t)(tk >> 32));
      }
      q.win = false;  // the next chunk's staging overwrites the window
      if (a.bdiag) d_walk += clock64() - d_w0;
    }
    __syncthreads();
  }
  } else {
  __shared__ uint32_t s_hb[CD_HOSTS], s_hn[CD_HOSTS];
  uint32_t h_act;
  const uint32_t max_n = lane_major_setup<ANY>(hb, he - hb, s_hb, s_hn, h_act);
  with_chunk_map<ANY>(ANY && lane_major_block(LM, p1 - p0, max_n, h_act), p0, p1, s_hb, s_hn, [&](auto cm) {
  for (uint32_t c = 0; cm.has(c, max_n); c++) {
    const uint32_t clen = cm.len(c);
    for (uint32_t base = 0; base < clen; base += CD_THREADS * CD_UNROLL) {  // staging (see ChunkMap)
      uint64_t rt[CD_UNROLL];
      uint32_t rp[CD_UNROLL], rl[CD_UNROLL];
      bool ok[CD_UNROLL];
#pragma unroll
      for (int u = 0; u < CD_UNROLL; u++) {
        const uint32_t i = cm.event(c, base + u * CD_THREADS + t, ok[u]);
        rt[u] = a.time[i];
        rp[u] = ORD ? (ARR_BIT | i) : a.pkt[i];
        if (!ORD) id_bad |= rp[u] >= a.n_status;
        rl[u] = a.len[i];
      }
#pragma unroll
      for (int u = 0; u < CD_UNROLL; u++) {
        const uint32_t k = base + u * CD_THREADS + t;
        if (k < clen && ok[u]) {
          s_t[k] = rt[u];
          s_p[k] = rp[u];
          s_l[k] = rl[u];
        }
      }
    }
    __syncthreads();
    if (walker) {
      uint32_t kb, ke, ib;
      cm.host_range(c, t, hb, he, kb, ke, ib);
      (void)ib;
      const uint64_t d_w0 = a.bdiag ? clock64() : 0;
      q.win = false;  // the tasks first run by this chunk pop the previous chunk's elements from HBM
      q.begin_window((lds_u32*)s_p, (lds_u32*)s_l, (lds_u64*)s_t, kb);
      uint64_t nt = kb < ke ? s_t[kb] : 0;  // the next arrival's fields, read ahead
      uint32_t np = kb < ke ? s_p[kb] : 0, nl = kb < ke ? s_l[kb] : 0;
      for (uint32_t k = kb; k < ke; k++) {
        const uint64_t now = nt;
        const uint32_t pkt = np, len = nl;
        if (k + 1 < ke) {
          nt = s_t[k + 1];
          np = s_p[k + 1];
          nl = s_l[k + 1];
        }
        if (now >= ia.window_end) q.err |= E_WINDOW;
        while (due(now)) relay_task(q, r, r.tt, ia.bootstrap_end, ia.sim_end, ctr_inc, ia.fwd_time);
        // Router::route_incoming_packet: the arrival is the window's next element (staged
        // slot k, read from LDS when it reaches the head); the ring receives the window's
        // still-queued elements at the chunk's end, as in k_codel -- a ring store per
        // arrival made the walk's next vector-memory wait include it
        (void)pkt;
        q.tail++;
        q.bytes += len;
        if (q.tail - q.head > q.mask + 1u) q.err |= E_FULL;  // an arrival found the ring full
        if (!q.hv) q.load_head();
        if (!(r.rf & R_PENDING)) r.schedule(now, now, ia.sim_end, ctr_inc);  // notify: Idle -> forward_later(ZERO)
      }
      // the window's elements still queued live on in the ring
      const uint32_t w0 = q.head - q.t0 <= q.tail - q.t0 ? q.head - q.t0 : 0;
      for (uint32_t j = w0; j < q.tail - q.t0; j++) {
        const uint32_t k = q.wb + j;
        const uint64_t tk = s_t[k];
        q.ring[(q.t0 + j) & q.mask] = make_uint4(s_p[k], s_l[k], (uint32_t)tk, (uint32_t)(tk >> 32));
      }
      q.win = false;  // the next chunk's staging overwrites the window
      if (a.bdiag) d_walk += clock64() - d_w0;
    }
    __syncthreads();
  }
  });
  }
  unsigned long long err = 0, dropped = 0;
  if (walker) {
    while (due(ia.window_end)) relay_task(q, r, r.tt, ia.bootstrap_end, ia.sim_end, ctr_inc, ia.fwd_time);
    if constexpr (ORD) {
      // the elements this call pushed that are still queued (the last min(queued, pushed) of
      // the ring), and a cached one, go back to the caller's packet ids for the next call; an id
      // past n_packets would read as an index in a later call, so it fails this one (E_PKT).
      // After a ring overflow (E_FULL: the call fails with SG_ERR_CAPACITY) the ring no longer
      // holds those elements, and nothing is translated
      auto to_id = [&](uint32_t v) -> uint32_t {
        const uint32_t i = v & ~ARR_BIT;
        const uint32_t id = i < a.E ? a.pkt[i] : 0xFFFFFFFFu;
        if (id >= a.n_status) q.err |= E_PKT;
        return id;
      };
      if (!(q.err & E_FULL)) {
        const uint32_t pushed = q.tail - tail0, queued = q.tail - q.head;
        for (uint32_t j = q.tail - min(min(pushed, queued), q.mask + 1u); j != q.tail; j++) {
          uint32_t* x = (uint32_t*)&q.ring[j & q.mask];
          if (*x & ARR_BIT) *x = to_id(*x);
        }
        if ((r.rf & R_CACHED) && (r.cp & ARR_BIT)) r.cp = to_id(r.cp);
      }
    }
    a.flags[h] = q.flags;
    a.iend[h] = q.iend;
    a.dnext[h] = q.dnext;
    a.cur[h] = q.cur;
    a.prev[h] = q.prev;
    a.bytes[h] = q.bytes;
    a.head[h] = q.head;
    a.tail[h] = q.tail;
    ia.rflags[h] = r.rf;
    ia.task_time[h] = r.tt;
    ia.cached_pkt[h] = r.cp;
    ia.cached_len[h] = r.cl;
    ia.tb_bal[h] = r.bal;
    ia.tb_last[h] = r.last;
    ia.task_id[h] = r.tid;
    ia.task_born[h] = r.tborn;
    if (ia.event_ctr && ctr_inc) ia.event_ctr[h] += ctr_inc;
    err = q.err;
    dropped = q.dropped;
  }
  if (!ORD && id_bad) err |= E_PKT;  // (every lane staged ids)
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

struct sg_inbound {
  sg_codel* q = nullptr;
  uint8_t* rflags = nullptr;
  uint64_t* task_time = nullptr;
  uint64_t *task_id = nullptr, *task_born = nullptr;
  uint32_t *cached_pkt = nullptr, *cached_len = nullptr;
  uint64_t *tb_cap = nullptr, *tb_bal = nullptr, *tb_inc = nullptr, *tb_last = nullptr;
  ~sg_inbound() {
    void* ps[] = {rflags, task_time, task_id, task_born, cached_pkt, cached_len, tb_cap, tb_bal, tb_inc, tb_last};
    for (void* p : ps)
      if (p) (void)hipFree(p);
    sg_codel_destroy(q);
  }
};

extern "C" {

int32_t sg_inbound_create(sg_ctx* ctx, uint32_t n_hosts, const uint64_t* bw_down_bits, uint32_t ring_cap,
                          sg_inbound** out) {
  if (!out) return SG_ERR_INVALID_ARG;
  *out = nullptr;
  sg_inbound* ib = new (std::nothrow) sg_inbound();
  if (!ib) return SG_ERR_OOM;
  int32_t rc = sg_codel_create(ctx, n_hosts, ring_cap, &ib->q);
  if (rc == SG_OK)
    rc = sg::guarded(ctx, [&] {
      using namespace sg;
      if (n_hosts && !bw_down_bits) throw Error(SG_ERR_INVALID_ARG, "null bandwidth array");
      const size_t n = std::max<uint32_t>(n_hosts, 1);
      SG_HIP(hipMalloc(&ib->rflags, n));
      SG_HIP(hipMalloc(&ib->task_time, n * 8));
      SG_HIP(hipMalloc(&ib->task_id, n * 8));
      SG_HIP(hipMalloc(&ib->task_born, n * 8));
      SG_HIP(hipMalloc(&ib->cached_pkt, n * 4));
      SG_HIP(hipMalloc(&ib->cached_len, n * 4));
      SG_HIP(hipMalloc(&ib->tb_cap, n * 8));
      SG_HIP(hipMalloc(&ib->tb_bal, n * 8));
      SG_HIP(hipMalloc(&ib->tb_inc, n * 8));
      SG_HIP(hipMalloc(&ib->tb_last, n * 8));
      // Relay::new (relay/mod.rs:48-66): Idle, no cached packet, a full bucket
      std::vector<uint64_t> inc(n), cap(n), last(n, 946684800ull * 1000000000ull);  // EmulatedTime::SIMULATION_START
      for (uint32_t h = 0; h < n_hosts; h++) {
        inc[h] = std::max<uint64_t>(1, (bw_down_bits[h] / 8) / 1000);  // create_token_bucket (:296-304)
        cap[h] = inc[h] + CD_MTU;                                      // + get_burst_allowance (:306-309)
      }
      hipStream_t st = ctx->stream;
      SG_HIP(hipMemsetAsync(ib->rflags, 0, n, st));
      SG_HIP(hipMemsetAsync(ib->task_time, 0, n * 8, st));
      SG_HIP(hipMemsetAsync(ib->task_id, 0, n * 8, st));
      SG_HIP(hipMemsetAsync(ib->task_born, 0, n * 8, st));
      SG_HIP(hipMemsetAsync(ib->cached_pkt, 0, n * 4, st));
      SG_HIP(hipMemsetAsync(ib->cached_len, 0, n * 4, st));
      SG_HIP(hipMemcpyAsync(ib->tb_cap, cap.data(), n * 8, hipMemcpyHostToDevice, st));
      SG_HIP(hipMemcpyAsync(ib->tb_bal, cap.data(), n * 8, hipMemcpyHostToDevice, st));
      SG_HIP(hipMemcpyAsync(ib->tb_inc, inc.data(), n * 8, hipMemcpyHostToDevice, st));
      SG_HIP(hipMemcpyAsync(ib->tb_last, last.data(), n * 8, hipMemcpyHostToDevice, st));
      SG_HIP(hipStreamSynchronize(st));
    });
  if (rc != SG_OK) {
    delete ib;
    return rc;
  }
  *out = ib;
  return SG_OK;
}

void sg_inbound_destroy(sg_inbound* ib) {
  if (!ib) return;
  if (ib->q && ib->q->ctx) (void)hipSetDevice(ib->q->ctx->device);
  delete ib;
}

uint32_t sg_inbound_ring_cap(const sg_inbound* ib) { return ib ? ib->q->cap : 0; }

}  // extern "C"

namespace sg {
// sg_inbound_run / sg_inbound_run_ordered (arr_status set: outputs per arrival of this call)
static int32_t inbound_run(sg_ctx* ctx, sg_inbound* ib, const sg_inbound_arrivals* arr, uint64_t window_end_ns,
                           uint64_t bootstrap_end_ns, uint64_t sim_end_ns, uint64_t* event_ctr, uint64_t* fwd_time,
                           uint8_t* pkt_status, uint32_t n_packets, uint8_t* arr_status, uint64_t* arr_fwd,
                           uint64_t* n_dropped) {
  return sg::guarded(ctx, [&] {
    if (!ib || !arr || ib->q->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "null argument");
    sg_codel* q = ib->q;
    const uint32_t E = arr->n, H = q->n;
    const bool ord = arr_status != nullptr;
    if (n_dropped) *n_dropped = 0;
    if (E && (!arr->host || !arr->time_ns || !arr->packet || !arr->len))
      throw Error(SG_ERR_INVALID_ARG, "null arrival array");
    if (n_packets && (!pkt_status || !fwd_time)) throw Error(SG_ERR_INVALID_ARG, "null output array");
    if (ord && E && !arr_fwd) throw Error(SG_ERR_INVALID_ARG, "null arrival output array");
    if (ord && E >= ARR_BIT) throw Error(SG_ERR_INVALID_ARG, "too many arrivals for one ordered call");
    // packet ids stay below 2^31 (an ordered call tells its arrival indices by bit 31)
    if (n_packets > ARR_BIT) throw Error(SG_ERR_INVALID_ARG, "n_packets above 2^31");
    if (!H) return;
    hipStream_t st = ctx->stream;
    uint32_t* ws = ctx->d_seg.get<uint32_t>((size_t)H + 8);
    uint32_t* gerr = ws + (size_t)H + 1;
    SG_HIP(hipMemsetAsync(gerr, 0, 4, st));
    if (E) {
      launch_group_offsets(ctx, arr->host, E, H, ws, gerr);
    } else {
      SG_HIP(hipMemsetAsync(ws, 0, ((size_t)H + 1) * 4, st));  // no arrivals: pending tasks only
    }
    const uint32_t nb = (H + CD_HOSTS - 1) / CD_HOSTS;
    InboundArgs a;
    a.q = CodelArgs{ws, H, E, nullptr, arr->time_ns, arr->packet, arr->len, q->flags, q->iend, q->dnext, q->cur,
                    q->prev, q->bytes, q->head, q->tail, q->ring, q->cap, nullptr, pkt_status, n_packets,
                    ctx->d_blk.get<unsigned long long>(2 * (size_t)nb)};
    a.rflags = ib->rflags;
    a.task_time = ib->task_time;
    a.task_id = ib->task_id;
    a.task_born = ib->task_born;
    a.cached_pkt = ib->cached_pkt;
    a.cached_len = ib->cached_len;
    a.tb_cap = ib->tb_cap;
    a.tb_bal = ib->tb_bal;
    a.tb_inc = ib->tb_inc;
    a.tb_last = ib->tb_last;
    a.window_end = window_end_ns;
    a.bootstrap_end = bootstrap_end_ns;
    a.sim_end = sim_end_ns;
    a.event_ctr = event_ctr;
    a.fwd_time = fwd_time;
    a.arr_status = arr_status;
    a.arr_fwd = arr_fwd;
    {
      // per arrival: 16 B in, a 16-B ring record written and read, 9 B out (ordered: 12 B in, the
      // packet id read only for an element still queued at the end); per host: ~160 B of state
      a.q.bdiag = lane_diag_alloc(nb);
      TimedLaunch tl(ctx, "inbound", (ord ? 53.0 : 57.0) * E + 160.0 * H);
      const int lm = lane_major_launch(lane_major_env(), E, nb, CD_CHUNK);
      auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(nb), dim3(CD_THREADS), 0, st, a); };
      with_lane_mode(lm, [&](auto m) {
        constexpr int LM = decltype(m)::value;
        if (ord) go(k_inbound<LM, true>);
        else go(k_inbound<LM>);
      });
    }
    lane_diag_report(st, "k_inbound", a.q.bdiag, nb);
    hipLaunchKernelGGL(k_codel_reduce, dim3(1), dim3(1024), 0, st, a.q.blk, nb, gerr, q->ret);
    SG_CHECK_LAUNCH();
    SG_HIP(hipStreamSynchronize(st));
    const volatile unsigned long long* r = q->ret;
    const uint64_t err = r[1];
    if (err & E_UNSORTED) throw Error(SG_ERR_UNSORTED, "arrivals must be grouped by ascending host");
    if (err & E_HOST) throw Error(SG_ERR_INVALID_ARG, "arrival host out of range");
    if (err & E_FULL) throw Error(SG_ERR_CAPACITY, "a CoDel queue outgrew its ring (raise ring_cap)");
    if (err & E_PKT) throw Error(SG_ERR_INVALID_ARG, "packet id >= n_packets");
    if (err & E_WINDOW) throw Error(SG_ERR_INVALID_ARG, "an arrival is at or after window_end");
    if (n_dropped) *n_dropped = r[0];
  });
}
}  // namespace sg

extern "C" {

int32_t sg_inbound_run(sg_ctx* ctx, sg_inbound* ib, const sg_inbound_arrivals* arr, uint64_t window_end_ns,
                       uint64_t bootstrap_end_ns, uint64_t sim_end_ns, uint64_t* event_ctr, uint64_t* fwd_time,
                       uint8_t* pkt_status, uint32_t n_packets, uint64_t* n_dropped) {
  return sg::inbound_run(ctx, ib, arr, window_end_ns, bootstrap_end_ns, sim_end_ns, event_ctr, fwd_time, pkt_status,
                         n_packets, nullptr, nullptr, n_dropped);
}

int32_t sg_inbound_run_ordered(sg_ctx* ctx, sg_inbound* ib, const sg_inbound_arrivals* arr, uint64_t window_end_ns,
                               uint64_t bootstrap_end_ns, uint64_t sim_end_ns, uint64_t* event_ctr,
                               uint64_t* fwd_time, uint8_t* pkt_status, uint32_t n_packets, uint64_t* arr_fwd_time,
                               uint8_t* arr_status, uint64_t* n_dropped) {
  if (arr && arr->n && !arr_status) return SG_ERR_INVALID_ARG;
  // (no arrivals: nothing is written per arrival, and the two kernels agree)
  return sg::inbound_run(ctx, ib, arr, window_end_ns, bootstrap_end_ns, sim_end_ns, event_ctr, fwd_time, pkt_status,
                         n_packets, arr && arr->n ? arr_status : nullptr, arr_fwd_time, n_dropped);
}

int32_t sg_inbound_get_state(sg_inbound* ib, sg_codel_state* queue, sg_inbound_relay_state* o) {
  if (!ib) return SG_ERR_INVALID_ARG;
  if (queue) {
    const int32_t rc = sg_codel_get_state(ib->q, queue);
    if (rc != SG_OK) return rc;
  }
  if (!o) return SG_OK;
  return sg::guarded(ib->q->ctx, [&] {
    const size_t n = ib->q->n;
    hipStream_t st = ib->q->ctx->stream;
    struct { void* h; const void* d; size_t b; } cp[] = {
        {o->flags, ib->rflags, n}, {o->task_time, ib->task_time, n * 8}, {o->cached_packet, ib->cached_pkt, n * 4},
        {o->cached_len, ib->cached_len, n * 4}, {o->tb_capacity, ib->tb_cap, n * 8},
        {o->tb_balance, ib->tb_bal, n * 8}, {o->tb_increment, ib->tb_inc, n * 8},
        {o->tb_last_refill, ib->tb_last, n * 8}, {o->task_event_id, ib->task_id, n * 8},
        {o->task_created_ns, ib->task_born, n * 8}};
    for (auto& c : cp)
      if (c.h && c.b) SG_HIP(hipMemcpyAsync(c.h, c.d, c.b, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
  });
}

}  // extern "C"
