// sg_outbound.hip -- the outbound pipeline with the interface's fifo qdisc: a ring of send
// records per host and the outbound relay's token bucket behind it (sg_lanes.h), one lane per
// host over a window of simulated time; then the sent batch gathered from the rings.  The
// round-robin qdisc of the same object is sg_qdisc.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_lanes.h"

namespace sg {
namespace {

// ---- outbound pipeline: interface FIFO -> relay_inet_out -> router --------
// Per host: sends push {packet, len, dst, payload_len} records into a ring
// (the interface's fifo qdisc); the relay's forward task pops them in order.
// The packet a blocked relay caches is the slot at head - 1 (never
// overwritten: a call's pushes may not reach the oldest slot it has to keep),
// so the records a call forwarded are still in the ring afterwards and
// k_out_compact gathers the sent batch from there -- no staging copy.

struct OutboundArgs {
  const uint32_t* host_off;
  uint32_t H, E;
  const uint64_t* time;
  const uint32_t *pkt, *len, *payload, *dst;
  const uint32_t* host_ip;
  uint32_t *head, *tail;
  uint4* ring;  // {packet, len, dst, payload_len}
  uint32_t cap;
  uint8_t* rflags;
  uint64_t* task_time;
  uint64_t *tb_cap, *tb_bal, *tb_inc, *tb_last;
  uint64_t window_end, bootstrap_end, sim_end;
  uint64_t* event_ctr;
  uint64_t* fwd_time;
  uint8_t* status;
  uint32_t n_status;
  uint32_t* start;  // per host: the first ring slot this call forwarded from
  const uint64_t *ev_id, *ev_born;  // per send (KEYED): the sending event's id and creation time
  uint64_t *task_id, *task_born;    // per host: the pending task's event id and creation time
  unsigned long long* blk;
  unsigned long long* bdiag = nullptr;  // as CodelArgs::bdiag
};

struct OutQ {
  uint32_t head, tail, oldest, mask, ip;
  uint4* ring;
  uint4 hr;  // the head record (valid while head < tail), loaded ahead of its pop
  uint4 cr;  // the relay's cached record (valid while R_CACHED): the slot at head - 1
  uint32_t sent;
  uint32_t err;
  // Staged window: the records pushed since begin_window() are the chunk's
  // send records wb, wb + 1, ... in LDS, so a head pushed there is read from
  // LDS instead of being re-read from the ring this lane just wrote (a forward
  // task pops back to back: each HBM re-read was a full round trip on the chain).
  bool win;
  uint32_t t0, wb;
  const __attribute__((address_space(3))) uint4* wr;
  __device__ void begin_window(const __attribute__((address_space(3))) uint4* r, uint32_t first) {
    win = true;
    t0 = tail;
    wb = first;
    wr = r;
  }
  __device__ void load_head() {
    if (head == tail) return;
    const uint32_t j = head - t0;
    if (win && j < tail - t0) {
      const __attribute__((address_space(3))) uint32_t* w =
          (const __attribute__((address_space(3))) uint32_t*)(wr + wb + j);
      hr = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      hr = ring[head & mask];
    }
  }
};

// The relay's forward task at `now` (run_forward_task -> forward_until_blocked),
// the interface as its source.
__device__ void out_task(OutQ& q, Relay& r, uint64_t now, const OutboundArgs& a, uint64_t& ctr_inc) {
  r.rf &= (uint8_t)~R_PENDING;
  for (;;) {
    uint4 rec;
    if (r.rf & R_CACHED) {  // next_packet.take(): the slot at head - 1
      rec = q.cr;
      r.rf &= (uint8_t)~R_CACHED;
    } else {
      if (q.head == q.tail) return;  // the interface has nothing: Idle
      rec = q.hr;
      q.head++;
      q.load_head();
    }
    const bool local = rec.z == q.ip;
    uint64_t wait;
    if (!local && now >= a.bootstrap_end && !r.remove(rec.y, now, wait)) {
      r.rf |= R_CACHED;  // RelayCached; forward_later(wait)
      q.cr = rec;
      r.schedule(now, now > ~0ull - wait ? ~0ull : now + wait, a.sim_end, ctr_inc);
      return;
    }
    if (rec.x < a.n_status) {
      a.status[rec.x] = local ? SG_OUT_LOCAL : SG_OUT_SENT;
      a.fwd_time[rec.x] = now;
    } else {
      q.err |= E_PKT;
    }
    q.sent += local ? 0 : 1;
  }
}

// KEYED: the sends carry their event's (creation time, id), and a task due at
// a send's own time runs first iff it was created before the sending event
// (Local events run in id = creation order, event.rs:163-183; a Packet event's
// send, id UINT64_MAX, precedes every Local event, event.rs:103-112).  Without
// keys every send precedes a task at its time.  A Local send's id also moves
// the host counter past it, so the tasks it schedules are numbered after it.  The keys cost 16 B of LDS per
// staged send, so the keyed chunk is smaller (40 B per send, 20 KB).
template <bool KEYED, int LM>
__global__ void __launch_bounds__(CD_THREADS) k_outbound(OutboundArgs a) {
  constexpr bool ANY = LM != 0;
  constexpr uint32_t CH = KEYED ? 512 : CD_OUT_CHUNK;
  const uint64_t d_t0 = a.bdiag ? wall_clock64() : 0;
  uint64_t d_walk = 0;
  __shared__ uint64_t s_t[CH];
  __shared__ uint4 s_r[CH];
  __shared__ uint64_t s_id[KEYED ? CH : 1], s_born[KEYED ? CH : 1];
  const uint32_t h0 = blockIdx.x * CD_HOSTS, t = threadIdx.x;
  const uint32_t h = h0 + t;
  const bool walker = t < CD_HOSTS && h < a.H;
  uint32_t hb = 0, he = 0;
  OutQ q{};
  Relay r{};
  uint64_t ctr_inc = 0, last = 0, last_born = 0, last_id = 0;
  if (walker) {
    hb = min(a.host_off[h], a.E);
    he = max(min(a.host_off[h + 1], a.E), hb);
    q.head = a.head[h];
    q.tail = a.tail[h];
    q.mask = a.cap - 1;
    q.ip = a.host_ip[h];
    q.ring = a.ring + (size_t)h * a.cap;
    r.rf = a.rflags[h];
    r.tt = a.task_time[h];
    r.cap = a.tb_cap[h];
    r.bal = a.tb_bal[h];
    r.set_inc(a.tb_inc[h]);
    r.last = a.tb_last[h];
    r.ctr0 = a.event_ctr ? a.event_ctr[h] : 0;
    r.tid = a.task_id[h];
    r.tborn = a.task_born[h];
    q.oldest = q.head - ((r.rf & R_CACHED) ? 1u : 0u);
    if (r.rf & R_CACHED) q.cr = q.ring[(q.head - 1) & q.mask];
    q.load_head();
  }
  // the block's events [p0, p1): lane 0's first and the last host's end, read from the
  // walkers' registers (loads of their own were waited for ahead of the walkers' state
  // loads once the chunk loop used them as scalars: a round trip per block, C4 +2.4 us)
  const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)hb, 0);
  const uint32_t p1 = (uint32_t)__builtin_amdgcn_readlane((int)he, (int)min(CD_HOSTS - 1u, a.H - 1u - h0));
  auto due = [&](uint64_t before) { return (r.rf & R_PENDING) && !(r.rf & R_NEVER) && r.tt < before; };
  // a task at the send's own time that runs first: created before the sending Local event
  auto due_tie = [&](uint64_t now, uint64_t born, uint64_t id) {
    return KEYED && (r.rf & R_PENDING) && !(r.rf & R_NEVER) && r.tt == now && id != ~0ull &&
           (r.tborn < born || (r.tborn == born && r.tid < id));
  };
  // The per-host walk under `if (walker)` stands twice, word for word: here and in the
  // with_chunk_map loop (an edit to one goes into the other).  k_codel and k_inbound call one
  // lambda from both loops; here that form cost C4 time although it compiled to fewer
  // instructions with the same registers: k_outbound<false, 0> 32.3-32.6 us per launch with the
  // two copies against 33.7-35.0 us with the lambda, busiest-lane walk mean 14.90 against
  // 15.93-16.15 us (one MI355X, libraries alternated, SG_LANE_DIAG apart; the same step as
  // ChunkMap<false>'s in sg_lanes.h).  Calling it without the `if (walker)` or with a
  // branch-free `due` did not bring it back (profiles/lane_walk_ab.json).
  if constexpr (!ANY) {  // contiguous chunks only: the r04 loop as it was (see with_chunk_map)
  for (uint32_t c0 = p0; c0 < p1; c0 += CH) {
    const uint32_t c1 = min(c0 + CH, p1);
    {
      uint64_t rt[CD_UNROLL], ri[KEYED ? CD_UNROLL : 1], rb[KEYED ? CD_UNROLL : 1];
      uint4 rr[CD_UNROLL];
      stage_chunk(
          c0, c1,
          [&](uint32_t i, int u) {
            rt[u] = a.time[i];
            rr[u] = make_uint4(a.pkt[i], a.len[i], a.dst[i], a.payload[i]);
            if constexpr (KEYED) {
              ri[u] = a.ev_id[i];
              rb[u] = a.ev_born[i];
            }
          },
          [&](uint32_t k, int u) {
            s_t[k] = rt[u];
            s_r[k] = rr[u];
            if constexpr (KEYED) {
              s_id[k] = ri[u];
              s_born[k] = rb[u];
            }
          });
    }
    __syncthreads();
    if (walker) {
      const uint32_t b = max(hb, c0), e = min(he, c1);
      const uint64_t d_w0 = a.bdiag ? clock64() : 0;
      q.begin_window((const __attribute__((address_space(3))) uint4*)s_r, b - c0);
      for (uint32_t i = b; i < e; i++) {
        const uint32_t k = i - c0;
        const uint64_t now = s_t[k];
        if (now >= a.window_end) q.err |= E_WINDOW;
        if (now < last) q.err |= E_ORDER;
        if constexpr (KEYED) {
          // execution order within a time: Packet-event sends, then Local ones by (created, id)
          const uint64_t id = s_id[k], born = s_born[k];
          if (now == last && i > hb) {
            const bool pk = id == ~0ull, lpk = last_id == ~0ull;
            if ((pk && !lpk) || (!pk && !lpk && (born < last_born || (born == last_born && id < last_id))))
              q.err |= E_ORDER;
          }
          last_born = born;
          last_id = id;
          // The sending event exists from its creation on, so the host's counter is past its id
          // (a Lamport-clock step; a no-op when the caller's ids come from this counter): before
          // a task that runs after that creation time (it may reschedule itself; at the time itself
          // the order of the task and the creating event is unknown), and
          // before the send (a task the send schedules takes a later id)
          while (due(now) || due_tie(now, born, id)) {
            if (id != ~0ull && r.tt > born && id - r.ctr0 >= ctr_inc && id >= r.ctr0) ctr_inc = id + 1 - r.ctr0;
            out_task(q, r, r.tt, a, ctr_inc);
          }
          // a send whose key equals the pending task's is no event order (two events, one id)
          if (id != ~0ull && (r.rf & R_PENDING) && !(r.rf & R_NEVER) && r.tt == now && r.tborn == born && r.tid == id)
            q.err |= E_ORDER;
          if (id != ~0ull && id - r.ctr0 >= ctr_inc && id >= r.ctr0) ctr_inc = id + 1 - r.ctr0;
        } else {
          while (due(now)) out_task(q, r, r.tt, a, ctr_inc);
        }
        last = now;
        if (q.tail - q.oldest >= a.cap) {  // the push would overwrite a slot this call still needs
          q.err |= E_FULL;
          continue;
        }
        // NetworkInterface::add_data_source: the record is the window's next element (read
        // from LDS at the head); the ring receives the window's records at the chunk's end
        // (k_out_compact gathers the sent ones from there) -- a ring store per send made the
        // walk's next vector-memory wait include it
        if (q.head == q.tail) q.hr = s_r[k];
        q.tail++;
        if (!(r.rf & R_PENDING)) r.schedule(now, now, a.sim_end, ctr_inc);  // notify: Idle -> forward_later(ZERO)
      }
      for (uint32_t j = 0; j < q.tail - q.t0; j++) q.ring[(q.t0 + j) & q.mask] = s_r[q.wb + j];
      if (a.bdiag) d_walk += clock64() - d_w0;
      q.win = false;  // the next chunk's staging overwrites the window
    }
    __syncthreads();
  }
  } else {
  __shared__ uint32_t s_hb[CD_HOSTS], s_hn[CD_HOSTS];
  uint32_t h_act;
  const uint32_t max_n = lane_major_setup<ANY>(hb, he - hb, s_hb, s_hn, h_act);
  with_chunk_map<ANY, CH>(ANY && lane_major_block<CH>(LM, p1 - p0, max_n, h_act), p0, p1, s_hb, s_hn,
                          [&](auto cm) {
  for (uint32_t c = 0; cm.has(c, max_n); c++) {
    const uint32_t clen = cm.len(c);
    for (uint32_t base = 0; base < clen; base += CD_THREADS * CD_UNROLL) {  // staging (see ChunkMap)
      uint64_t rt[CD_UNROLL], ri[KEYED ? CD_UNROLL : 1], rb[KEYED ? CD_UNROLL : 1];
      uint4 rr[CD_UNROLL];
      bool ok[CD_UNROLL];
#pragma unroll
      for (int u = 0; u < CD_UNROLL; u++) {
        const uint32_t i = cm.event(c, base + u * CD_THREADS + t, ok[u]);
        rt[u] = a.time[i];
        rr[u] = make_uint4(a.pkt[i], a.len[i], a.dst[i], a.payload[i]);
        if constexpr (KEYED) {
          ri[u] = a.ev_id[i];
          rb[u] = a.ev_born[i];
        }
      }
#pragma unroll
      for (int u = 0; u < CD_UNROLL; u++) {
        const uint32_t k = base + u * CD_THREADS + t;
        if (k < clen && ok[u]) {
          s_t[k] = rt[u];
          s_r[k] = rr[u];
          if constexpr (KEYED) {
            s_id[k] = ri[u];
            s_born[k] = rb[u];
          }
        }
      }
    }
    __syncthreads();
    if (walker) {
      uint32_t kb, ke, ib;
      cm.host_range(c, t, hb, he, kb, ke, ib);
      const uint64_t d_w0 = a.bdiag ? clock64() : 0;
      q.begin_window((const __attribute__((address_space(3))) uint4*)s_r, kb);
      for (uint32_t k = kb; k < ke; k++) {
        const uint32_t i = ib + (k - kb);
        const uint64_t now = s_t[k];
        if (now >= a.window_end) q.err |= E_WINDOW;
        if (now < last) q.err |= E_ORDER;
        if constexpr (KEYED) {
          // execution order within a time: Packet-event sends, then Local ones by (created, id)
          const uint64_t id = s_id[k], born = s_born[k];
          if (now == last && i > hb) {
            const bool pk = id == ~0ull, lpk = last_id == ~0ull;
            if ((pk && !lpk) || (!pk && !lpk && (born < last_born || (born == last_born && id < last_id))))
              q.err |= E_ORDER;
          }
          last_born = born;
          last_id = id;
          // The sending event exists from its creation on, so the host's counter is past its id
          // (a Lamport-clock step; a no-op when the caller's ids come from this counter): before
          // a task that runs after that creation time (it may reschedule itself; at the time itself
          // the order of the task and the creating event is unknown), and
          // before the send (a task the send schedules takes a later id)
          while (due(now) || due_tie(now, born, id)) {
            if (id != ~0ull && r.tt > born && id - r.ctr0 >= ctr_inc && id >= r.ctr0) ctr_inc = id + 1 - r.ctr0;
            out_task(q, r, r.tt, a, ctr_inc);
          }
          // a send whose key equals the pending task's is no event order (two events, one id)
          if (id != ~0ull && (r.rf & R_PENDING) && !(r.rf & R_NEVER) && r.tt == now && r.tborn == born && r.tid == id)
            q.err |= E_ORDER;
          if (id != ~0ull && id - r.ctr0 >= ctr_inc && id >= r.ctr0) ctr_inc = id + 1 - r.ctr0;
        } else {
          while (due(now)) out_task(q, r, r.tt, a, ctr_inc);
        }
        last = now;
        if (q.tail - q.oldest >= a.cap) {  // the push would overwrite a slot this call still needs
          q.err |= E_FULL;
          continue;
        }
        // NetworkInterface::add_data_source: the record is the window's next element (read
        // from LDS at the head); the ring receives the window's records at the chunk's end
        // (k_out_compact gathers the sent ones from there) -- a ring store per send made the
        // walk's next vector-memory wait include it
        if (q.head == q.tail) q.hr = s_r[k];
        q.tail++;
        if (!(r.rf & R_PENDING)) r.schedule(now, now, a.sim_end, ctr_inc);  // notify: Idle -> forward_later(ZERO)
      }
      for (uint32_t j = 0; j < q.tail - q.t0; j++) q.ring[(q.t0 + j) & q.mask] = s_r[q.wb + j];
      if (a.bdiag) d_walk += clock64() - d_w0;
      q.win = false;  // the next chunk's staging overwrites the window
    }
    __syncthreads();
  }
  });
  }
  unsigned long long err = 0, sent = 0;
  if (walker) {
    while (due(a.window_end)) out_task(q, r, r.tt, a, ctr_inc);
    a.head[h] = q.head;
    a.tail[h] = q.tail;
    a.rflags[h] = r.rf;
    a.task_time[h] = r.tt;
    a.tb_bal[h] = r.bal;
    a.tb_last[h] = r.last;
    a.task_id[h] = r.tid;
    a.task_born[h] = r.tborn;
    a.start[h] = q.oldest;
    if (a.event_ctr && ctr_inc) a.event_ctr[h] += ctr_inc;
    err = q.err;
    sent = q.sent;
  }
  lane_diag_store(a.bdiag, d_t0, d_walk, he - hb);
  if (t < 64) {
    for (int d = 32; d > 0; d >>= 1) {
      sent += __shfl_xor(sent, d, 64);
      err |= __shfl_xor(err, d, 64);
    }
    if (t == 0) {
      a.blk[2 * blockIdx.x] = sent;
      a.blk[2 * blockIdx.x + 1] = err;
    }
  }
}


// The sent batch: block b owns hosts [64b, 64b + 64), whose forwarded records
// are ring slots [start, end) per host (end = head, less a packet cached at the
// end).  The block walks the hosts' slot ranges as one concatenated sequence,
// 256 slots per step (coalesced within a host's range), skips local packets
// (a ballot prefix gives each kept record its rank) and writes its slice
// [boff[b], boff[b] + sent) of the batch with coalesced stores.
__global__ void __launch_bounds__(256) k_out_compact(uint32_t H, const uint32_t* __restrict__ start,
                                                     const uint32_t* __restrict__ head,
                                                     const uint8_t* __restrict__ rflags,
                                                     const uint32_t* __restrict__ host_ip,
                                                     const uint4* __restrict__ ring, uint32_t cap,
                                                     const uint64_t* __restrict__ fwd_time, uint32_t n_status,
                                                     const uint32_t* __restrict__ boff, sg_outbound_sent out) {
  __shared__ uint32_t s_off[CD_HOSTS + 1], s_start[CD_HOSTS], s_ip[CD_HOSTS];
  __shared__ uint32_t wsum[4];
  const uint32_t h0 = blockIdx.x * CD_HOSTS, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < 64) {  // one wave: per-host slot counts and their exclusive prefix
    const uint32_t h = h0 + t;
    uint32_t len = 0;
    if (h < H) {
      const uint32_t st = start[h], end = head[h] - ((rflags[h] & R_CACHED) ? 1u : 0u);
      len = end - st;
      s_start[t] = st;
      s_ip[t] = host_ip[h];
    }
    uint32_t x = len;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (lane >= (uint32_t)d) x += y;
    }
    s_off[t + 1] = x;
    if (t == 0) s_off[0] = 0;
  }
  __syncthreads();
  const uint32_t S = s_off[CD_HOSTS], mask = cap - 1;
  uint32_t o = boff[blockIdx.x];
  // CU rounds of 256 records per step: every round's ring and forward-time loads are
  // issued (branch-free, clamped to a valid record) before the step's first store --
  // a load after a store waited for the store too
  constexpr int CU = 4;
  for (uint32_t j0 = 0; j0 < S; j0 += 256 * CU) {
    uint4 rec[CU];
    uint32_t kk[CU];
    bool keep[CU];
    uint64_t ft[CU];
#pragma unroll
    for (int u = 0; u < CU; u++) {
      const uint32_t j = j0 + u * 256 + t, jc = min(j, S - 1);
      uint32_t lo = 0, hi = CD_HOSTS;  // the host k with s_off[k] <= jc < s_off[k + 1]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_off[mid] <= jc) lo = mid;
        else hi = mid;
      }
      kk[u] = lo;
      rec[u] = ring[(size_t)(h0 + lo) * cap + ((s_start[lo] + (jc - s_off[lo])) & mask)];
    }
#pragma unroll
    for (int u = 0; u < CU; u++) {
      keep[u] = j0 + u * 256 + t < S && rec[u].z != s_ip[kk[u]];
      ft[u] = n_status ? fwd_time[rec[u].x < n_status ? rec[u].x : 0u] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < CU; u++) {
      if (j0 + u * 256 >= S) break;
      const uint64_t m = __ballot(keep[u]);
      if (lane == 0) wsum[wv] = (uint32_t)__popcll(m);
      __syncthreads();
      uint32_t pos = o + (uint32_t)__popcll(m & ((1ull << lane) - 1));
      for (uint32_t w = 0; w < wv; w++) pos += wsum[w];
      if (keep[u] && pos < out.cap) {
        out.src_host[pos] = h0 + kk[u];
        out.dst_ipv4[pos] = rec[u].z;
        out.payload_len[pos] = rec[u].w;
        out.send_time_ns[pos] = rec[u].x < n_status ? ft[u] : 0;
        out.packet[pos] = rec[u].x;
      }
      o += wsum[0] + wsum[1] + wsum[2] + wsum[3];
      __syncthreads();
    }
  }
}

}  // namespace
}  // namespace sg

extern "C" {

int32_t sg_outbound_create(sg_ctx* ctx, uint32_t n_hosts, const uint32_t* host_ipv4, const uint64_t* bw_up_bits,
                           uint32_t ring_cap, sg_outbound** out) {
  return sg_outbound_create_qdisc(ctx, n_hosts, host_ipv4, bw_up_bits, ring_cap, SG_QDISC_FIFO, 1, out);
}

int32_t sg_outbound_create_qdisc(sg_ctx* ctx, uint32_t n_hosts, const uint32_t* host_ipv4,
                                 const uint64_t* bw_up_bits, uint32_t ring_cap, uint32_t qdisc, uint32_t max_sockets,
                                 sg_outbound** out) {
  if (!out) return SG_ERR_INVALID_ARG;
  *out = nullptr;
  sg_outbound* ob = nullptr;
  int32_t rc = sg::guarded(ctx, [&] {
    using namespace sg;
    if (ring_cap == 0 || ring_cap > (1u << 30)) throw Error(SG_ERR_INVALID_ARG, "ring_cap must be in [1, 2^30]");
    if (n_hosts && (!host_ipv4 || !bw_up_bits)) throw Error(SG_ERR_INVALID_ARG, "null address or bandwidth array");
    if (qdisc != SG_QDISC_FIFO && qdisc != SG_QDISC_ROUND_ROBIN)
      throw Error(SG_ERR_INVALID_ARG, "qdisc must be SG_QDISC_FIFO or SG_QDISC_ROUND_ROBIN");
    if (max_sockets == 0 || max_sockets > SG_QDISC_MAX_SOCKETS)
      throw Error(SG_ERR_INVALID_ARG, "max_sockets must be in [1, SG_QDISC_MAX_SOCKETS]");
    const bool rr = qdisc == SG_QDISC_ROUND_ROBIN;
    uint32_t cap = 1, n_sock = 1;
    while (cap < ring_cap) cap <<= 1;
    while (n_sock < max_sockets) n_sock <<= 1;
    ob = new sg_outbound();
    ob->qdisc = qdisc;
    ob->n_sock = n_sock;
    ob->ctx = ctx;
    ob->n = n_hosts;
    ob->cap = cap;
    const size_t n = std::max<uint32_t>(n_hosts, 1);
    SG_HIP(hipMalloc(&ob->host_ip, n * 4));
    SG_HIP(hipMalloc(&ob->head, n * 4));
    SG_HIP(hipMalloc(&ob->tail, n * 4));
    SG_HIP(hipMalloc(&ob->start, n * 4));
    SG_HIP(hipMalloc(&ob->off, ((n + CD_HOSTS - 1) / CD_HOSTS + 1) * 4));  // per k_outbound block
    SG_HIP(hipMalloc(&ob->ring, n * cap * 16 * (rr ? 2 : 1)));
    SG_HIP(hipMalloc(&ob->rflags, n));
    const size_t n_slot = (n + CD_HOSTS - 1) / CD_HOSTS * CD_HOSTS * n_sock;  // sg_lanes.h qd_slot
    if (rr) {
      SG_HIP(hipMalloc(&ob->nxt, n * cap * 4 * 2));
      SG_HIP(hipMalloc(&ob->sk_head, n_slot * 4));
      SG_HIP(hipMalloc(&ob->sk_tail, n_slot * 4));
      SG_HIP(hipMalloc(&ob->dq, n_slot));
      SG_HIP(hipMalloc(&ob->dq_front, n * 4));
      SG_HIP(hipMalloc(&ob->dq_n, n * 4));
      SG_HIP(hipMalloc(&ob->top, n * 4));
      SG_HIP(hipMalloc(&ob->n_live, n * 4));
      SG_HIP(hipMalloc(&ob->half, n));
      SG_HIP(hipMalloc(&ob->cached, n * 16));
    }
    SG_HIP(hipMalloc(&ob->task_time, n * 8));
    SG_HIP(hipMalloc(&ob->task_id, n * 8));
    SG_HIP(hipMalloc(&ob->task_born, n * 8));
    SG_HIP(hipMalloc(&ob->tb_cap, n * 8));
    SG_HIP(hipMalloc(&ob->tb_bal, n * 8));
    SG_HIP(hipMalloc(&ob->tb_inc, n * 8));
    SG_HIP(hipMalloc(&ob->tb_last, n * 8));
    SG_HIP(hipHostMalloc(&ob->ret, 16, hipHostMallocMapped | hipHostMallocCoherent));
    // Relay::new (relay/mod.rs:91-109): Idle, nothing cached, a full bucket;
    // the interface's queue empty
    std::vector<uint64_t> inc(n), tcap(n), last(n, 946684800ull * 1000000000ull);  // EmulatedTime::SIMULATION_START
    for (uint32_t h = 0; h < n_hosts; h++) {
      inc[h] = std::max<uint64_t>(1, (bw_up_bits[h] / 8) / 1000);  // create_token_bucket (:278-315)
      tcap[h] = inc[h] + CD_MTU;                                   // + get_burst_allowance (:317-319)
    }
    hipStream_t st = ctx->stream;
    if (n_hosts) SG_HIP(hipMemcpyAsync(ob->host_ip, host_ipv4, (size_t)n_hosts * 4, hipMemcpyHostToDevice, st));
    SG_HIP(hipMemsetAsync(ob->head, 0, n * 4, st));
    SG_HIP(hipMemsetAsync(ob->tail, 0, n * 4, st));
    if (rr) {  // every socket empty, the deques empty, the pools unused
      SG_HIP(hipMemsetAsync(ob->sk_head, 0xff, n_slot * 4, st));
      SG_HIP(hipMemsetAsync(ob->sk_tail, 0xff, n_slot * 4, st));
      SG_HIP(hipMemsetAsync(ob->dq, 0, n_slot, st));
      SG_HIP(hipMemsetAsync(ob->dq_front, 0, n * 4, st));
      SG_HIP(hipMemsetAsync(ob->dq_n, 0, n * 4, st));
      SG_HIP(hipMemsetAsync(ob->top, 0, n * 4, st));
      SG_HIP(hipMemsetAsync(ob->n_live, 0, n * 4, st));
      SG_HIP(hipMemsetAsync(ob->half, 0, n, st));
      SG_HIP(hipMemsetAsync(ob->cached, 0, n * 16, st));
    }
    SG_HIP(hipMemsetAsync(ob->rflags, 0, n, st));
    SG_HIP(hipMemsetAsync(ob->task_time, 0, n * 8, st));
    SG_HIP(hipMemsetAsync(ob->task_id, 0, n * 8, st));
    SG_HIP(hipMemsetAsync(ob->task_born, 0, n * 8, st));
    SG_HIP(hipMemcpyAsync(ob->tb_cap, tcap.data(), n * 8, hipMemcpyHostToDevice, st));
    SG_HIP(hipMemcpyAsync(ob->tb_bal, tcap.data(), n * 8, hipMemcpyHostToDevice, st));
    SG_HIP(hipMemcpyAsync(ob->tb_inc, inc.data(), n * 8, hipMemcpyHostToDevice, st));
    SG_HIP(hipMemcpyAsync(ob->tb_last, last.data(), n * 8, hipMemcpyHostToDevice, st));
    SG_HIP(hipStreamSynchronize(st));
  });
  if (rc != SG_OK) {
    delete ob;
    return rc;
  }
  *out = ob;
  return SG_OK;
}

void sg_outbound_destroy(sg_outbound* ob) {
  if (!ob) return;
  if (ob->ctx) (void)hipSetDevice(ob->ctx->device);
  delete ob;
}

uint32_t sg_outbound_ring_cap(const sg_outbound* ob) { return ob ? ob->cap : 0; }
uint32_t sg_outbound_qdisc(const sg_outbound* ob) { return ob ? ob->qdisc : 0; }
uint32_t sg_outbound_max_sockets(const sg_outbound* ob) { return ob ? ob->n_sock : 0; }

int32_t sg_outbound_run(sg_ctx* ctx, sg_outbound* ob, const sg_outbound_sends* s, uint64_t window_end_ns,
                        uint64_t bootstrap_end_ns, uint64_t sim_end_ns, uint64_t* event_ctr, uint64_t* fwd_time,
                        uint8_t* pkt_status, uint32_t n_packets, sg_outbound_sent* sent, uint32_t* n_sent) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (!ob || !s || ob->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "null argument");
    if (ob->qdisc != SG_QDISC_FIFO)
      throw Error(SG_ERR_INVALID_ARG, "a round-robin interface takes its sends' sockets: sg_outbound_run_qdisc");
    const uint32_t E = s->n, H = ob->n;
    if (n_sent) *n_sent = 0;
    if (E && (!s->host || !s->time_ns || !s->packet || !s->len || !s->payload_len || !s->dst_ipv4))
      throw Error(SG_ERR_INVALID_ARG, "null send array");
    if (n_packets && (!pkt_status || !fwd_time)) throw Error(SG_ERR_INVALID_ARG, "null output array");
    const bool keyed = s->event_id != nullptr;
    if (keyed != (s->event_created_ns != nullptr))
      throw Error(SG_ERR_INVALID_ARG, "event_id and event_created_ns are given together or not at all");
    if (keyed && !event_ctr) throw Error(SG_ERR_INVALID_ARG, "send event ids need the hosts' event counters");
    if (sent && sent->cap && (!sent->src_host || !sent->dst_ipv4 || !sent->payload_len || !sent->send_time_ns ||
                              !sent->packet))
      throw Error(SG_ERR_INVALID_ARG, "null sent-batch array");
    if (!H) return;
    hipStream_t st = ctx->stream;
    uint32_t* ws = ctx->d_seg.get<uint32_t>((size_t)H + 8);
    uint32_t* gerr = ws + (size_t)H + 1;
    SG_HIP(hipMemsetAsync(gerr, 0, 4, st));
    if (E) {
      launch_group_offsets(ctx, s->host, E, H, ws, gerr);
    } else {
      SG_HIP(hipMemsetAsync(ws, 0, ((size_t)H + 1) * 4, st));  // no sends: pending tasks only
    }
    const uint32_t nb = (H + CD_HOSTS - 1) / CD_HOSTS;
    OutboundArgs a;
    a.host_off = ws;
    a.H = H;
    a.E = E;
    a.time = s->time_ns;
    a.pkt = s->packet;
    a.len = s->len;
    a.payload = s->payload_len;
    a.dst = s->dst_ipv4;
    a.host_ip = ob->host_ip;
    a.head = ob->head;
    a.tail = ob->tail;
    a.ring = ob->ring;
    a.cap = ob->cap;
    a.rflags = ob->rflags;
    a.task_time = ob->task_time;
    a.task_id = ob->task_id;
    a.task_born = ob->task_born;
    a.ev_id = s->event_id;
    a.ev_born = s->event_created_ns;
    a.tb_cap = ob->tb_cap;
    a.tb_bal = ob->tb_bal;
    a.tb_inc = ob->tb_inc;
    a.tb_last = ob->tb_last;
    a.window_end = window_end_ns;
    a.bootstrap_end = bootstrap_end_ns;
    a.sim_end = sim_end_ns;
    a.event_ctr = event_ctr;
    a.fwd_time = fwd_time;
    a.status = pkt_status;
    a.n_status = n_packets;
    a.start = ob->start;
    a.blk = ctx->d_blk.get<unsigned long long>(2 * (size_t)nb);
    {
      // per send: 24 B in, a 16-B ring record written and read, 9 B out; per host: ~90 B of state
      a.bdiag = lane_diag_alloc(nb);
        TimedLaunch tl(ctx, "outbound", 65.0 * E + 90.0 * H);
      const int lm = lane_major_launch(lane_major_env(), E, nb, keyed ? 512u : (uint32_t)CD_OUT_CHUNK);
      auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(nb), dim3(CD_THREADS), 0, st, a); };
      with_lane_mode(lm, [&](auto m) {
        constexpr int LM = decltype(m)::value;
        if (keyed && E) go(k_outbound<true, LM>);
        else go(k_outbound<false, LM>);
      });
    }
    lane_diag_report(st, "k_outbound", a.bdiag, nb);
    if (sent) {  // the blocks' offsets and the sums in one launch, then the compaction
      hipLaunchKernelGGL(k_blk_offsets, dim3(1), dim3(1024), 0, st, a.blk, nb, ob->off, gerr, ob->ret);
      sg_outbound_sent o = *sent;
      TimedLaunch tl(ctx, "out_compact", 0.0);
      hipLaunchKernelGGL(k_out_compact, dim3(nb), dim3(256), 0, st, H, ob->start, ob->head, ob->rflags, ob->host_ip,
                         ob->ring, ob->cap, fwd_time, n_packets, ob->off, o);
    } else {
      hipLaunchKernelGGL(k_codel_reduce, dim3(1), dim3(1024), 0, st, a.blk, nb, gerr, ob->ret);
    }
    SG_CHECK_LAUNCH();
    SG_HIP(hipStreamSynchronize(st));
    const volatile unsigned long long* r = ob->ret;
    const uint64_t err = r[1];
    if (err & E_UNSORTED) throw Error(SG_ERR_UNSORTED, "sends must be grouped by ascending host");
    if (err & E_HOST) throw Error(SG_ERR_INVALID_ARG, "send host out of range");
    if (err & E_ORDER)
      throw Error(SG_ERR_UNSORTED, "a host's sends must come in execution order (time; Packet events, then "
                                   "Local ones by creation time and id)");
    if (err & E_FULL) throw Error(SG_ERR_CAPACITY, "an interface queue outgrew its ring (raise ring_cap)");
    if (err & E_PKT) throw Error(SG_ERR_INVALID_ARG, "packet id >= n_packets");
    if (err & E_WINDOW) throw Error(SG_ERR_INVALID_ARG, "a send is at or after window_end");
    const uint64_t ns = r[0];
    if (n_sent) *n_sent = (uint32_t)ns;
    if (sent && ns > sent->cap) throw Error(SG_ERR_CAPACITY, "the sent batch exceeds sent->cap");
  });
}

int32_t sg_outbound_get_state(sg_outbound* ob, sg_outbound_queue_state* o, sg_inbound_relay_state* rl) {
  if (!ob) return SG_ERR_INVALID_ARG;
  return sg::guarded(ob->ctx, [&] {
    const size_t n = ob->n, r = n * ob->cap;
    hipStream_t st = ob->ctx->stream;
    const bool rr = ob->qdisc != SG_QDISC_FIFO;
    if (rr && o)
      throw sg::Error(SG_ERR_INVALID_ARG, "a round-robin interface has no ring: sg_outbound_get_qdisc_state");
    if (o) {
      struct { void* h; const void* d; size_t b; } cp[] = {{o->head, ob->head, n * 4}, {o->tail, ob->tail, n * 4}};
      for (auto& c : cp)
        if (c.h && c.b) SG_HIP(hipMemcpyAsync(c.h, c.d, c.b, hipMemcpyDeviceToHost, st));
    }
    if (rl) {
      struct { void* h; const void* d; size_t b; } cp[] = {
          {rl->flags, ob->rflags, n}, {rl->task_time, ob->task_time, n * 8}, {rl->tb_capacity, ob->tb_cap, n * 8},
          {rl->tb_balance, ob->tb_bal, n * 8}, {rl->tb_increment, ob->tb_inc, n * 8},
          {rl->tb_last_refill, ob->tb_last, n * 8}, {rl->task_event_id, ob->task_id, n * 8},
          {rl->task_created_ns, ob->task_born, n * 8}};
      for (auto& c : cp)
        if (c.h && c.b) SG_HIP(hipMemcpyAsync(c.h, c.d, c.b, hipMemcpyDeviceToHost, st));
    }
    std::vector<uint4> ring(o ? r : 0);
    if (o && r) SG_HIP(hipMemcpyAsync(ring.data(), ob->ring, r * 16, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (o)
      for (size_t i = 0; i < r; i++) {
        if (o->ring_packet) o->ring_packet[i] = ring[i].x;
        if (o->ring_len) o->ring_len[i] = ring[i].y;
        if (o->ring_dst) o->ring_dst[i] = ring[i].z;
        if (o->ring_payload_len) o->ring_payload_len[i] = ring[i].w;
      }
    // the relay's cached packet is the ring slot at head - 1 (no separate fields)
    if (rl && (rl->cached_packet || rl->cached_len)) {
      std::vector<uint32_t> head(n);
      std::vector<uint8_t> fl(n);
      SG_HIP(hipMemcpy(head.data(), ob->head, n * 4, hipMemcpyDeviceToHost));
      SG_HIP(hipMemcpy(fl.data(), ob->rflags, n, hipMemcpyDeviceToHost));
      for (size_t h = 0; h < n; h++) {
        uint4 rec = make_uint4(0, 0, 0, 0);
        if (rr && (fl[h] & sg::R_CACHED))  // (a record of its own: sg_lanes.h)
          SG_HIP(hipMemcpy(&rec, ob->cached + h, 16, hipMemcpyDeviceToHost));
        else if (fl[h] & sg::R_CACHED)
          SG_HIP(hipMemcpy(&rec, ob->ring + h * ob->cap + ((head[h] - 1) & (ob->cap - 1)), 16, hipMemcpyDeviceToHost));
        if (rl->cached_packet) rl->cached_packet[h] = rec.x;
        if (rl->cached_len) rl->cached_len[h] = rec.y;
      }
    }
  });
}

}  // extern "C"
