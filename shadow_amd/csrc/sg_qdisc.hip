// sg_qdisc.hip -- the outbound pipeline with the interface's round-robin qdisc.
//
// experimental.interface_qdisc: round-robin (QDiscMode::RoundRobin, configuration.rs:971-973)
// makes the interface a FIFO over *sockets* (NetworkQueueKind::FirstInFirstOut,
// host/network/interface.rs:97-108, queuing.rs): a deque of socket ids without duplicates and a
// FIFO of packets per socket.  A send appends to its socket's FIFO and pushes the socket to the
// deque's back unless it is queued already (add_data_source, interface.rs:168-181); pop()
// (:227-259) takes the front socket and its oldest packet and pushes the socket to the back if
// it still holds one.  The relay above it (relay/mod.rs:111-273) is k_outbound's.
//
// k_qdisc has k_outbound's shape (sg_outbound.hip): one wave per block, one lane per host, the
// block's sends staged through LDS in chunks of either layout (ChunkMap).  Per host:
//   pool     `cap` record slots, bump-allocated (slot = top++).  ring_cap bounds the packets
//            queued at a call's start plus the call's sends, so a pool that starts a call
//            compacted never overflows; a host compacts (QdQ::compact: its queued records, in
//            deque order, into the other half of its two-half pool) only when the call's sends
//            would not fit behind `top`, and an interface that drains frees its pool at once.
//   nxt      per slot, the next record of the same socket.
//   sockets  head and tail slot per socket (head ~0u: empty, i.e. not in the deque).
//   deque    a ring of n_sock socket ids with a front counter and a length.
//   log      the records the call forwarded to the router, in forward order, in the pool's idle
//            half (at most `cap`: every one was queued at the start or sent by the call);
//            k_qd_compact gathers the blocks' logs into the sent batch.
// A pop chains deque -> socket head -> record -> next link.  With up to QD_LDS_SOCKETS sockets
// per host the sockets' heads and tails and the deque live in LDS for the call (loaded by the
// lane that owns them, stored back at the end); the records and links of the chunk being
// walked are read from the staged chunk itself (the window, as OutQ's), so a pop that follows
// its push never leaves LDS.  Past QD_LDS_SOCKETS the socket state stays in global memory.
#include <algorithm>
#include <vector>

#include "sg_lanes.h"

namespace sg {
namespace {

constexpr uint32_t QD_NONE = ~0u;
constexpr uint32_t QD_LDS_SOCKETS = 16;
// 32 B of LDS per staged send (time, record, socket, link), 48 B keyed: 12 KB of chunk + 9 KB of
// socket state (16 sockets x 64 hosts x (4 + 4 + 1) B) + 0.5 KB = 21.5 KB, 7 blocks per CU
constexpr uint32_t QD_CHUNK = 384, QD_CHUNK_KEYED = 256;
enum : uint32_t { E_SOCKET = 256 };

typedef __attribute__((address_space(3))) const uint4 lds_rec;
typedef __attribute__((address_space(3))) uint32_t lds_link;

template <bool SL, class T>
struct SockPtr {
  typedef T* type;
};
template <class T>
struct SockPtr<true, T> {
  typedef __attribute__((address_space(3))) T* type;
};

struct QdiscArgs {
  const uint32_t* host_off;
  uint32_t H, E;
  const uint64_t* time;
  const uint32_t *pkt, *len, *payload, *dst, *sock;
  const uint32_t* host_ip;
  uint4* pool;    // 2 * cap records per host
  uint32_t* nxt;  // 2 * cap links per host
  uint32_t cap, n_sock;
  uint32_t *sk_head, *sk_tail;
  uint8_t* dq;
  uint32_t *dq_front, *dq_n, *top, *n_live;
  uint8_t* half;
  uint4* cached;
  uint32_t* n_fwd;  // per host: the records this call logged
  uint8_t* rflags;
  uint64_t* task_time;
  uint64_t *tb_cap, *tb_bal, *tb_inc, *tb_last;
  uint64_t window_end, bootstrap_end, sim_end;
  uint64_t* event_ctr;
  uint64_t* fwd_time;
  uint8_t* status;
  uint32_t n_status;
  const uint64_t *ev_id, *ev_born;
  uint64_t *task_id, *task_born;
  int lm;  // lane_major_launch's mode
  unsigned long long* blk;
  unsigned long long* bdiag = nullptr;
};

// One host's interface.  SL: the socket state is in LDS (column threadIdx.x of [s][64] arrays),
// else in global memory (qd_slot); either way socket s is hd[s * 64], deque entry j dq[j * 64].
template <bool SL>
struct QdQ {
  typename SockPtr<SL, uint32_t>::type hd, tl;
  typename SockPtr<SL, uint8_t>::type dq;
  uint32_t front, n, smask;
  uint4 *pool, *log;
  uint32_t* nxt;
  uint32_t top, live, room, ip, n_log, err;
  uint4 cr;  // the relay's cached record (valid while R_CACHED)
  // The record the next pop returns (valid while n != 0), read ahead of it as OutQ's hr is: a send
  // into an empty interface takes it from the staged chunk, so the pop that follows meets no
  // join of an LDS read with a global one -- at such a join the wave waits for every vector-
  // memory operation in flight (vmcnt counts loads and stores alike), the last forward's stores
  // included; a pop that leaves the interface busy reads the next one (and pays that wait)
  uint4 fr;
  // the staged window (OutQ's): slots [t0, top) are the chunk's records wb, wb + 1, ...
  bool win;
  uint32_t t0, wb;
  lds_rec* wr;
  lds_link* wn;

  __device__ void begin_window(lds_rec* r, lds_link* l, uint32_t first) {
    win = true;
    t0 = top;
    wb = first;
    wr = r;
    wn = l;
  }
  __device__ bool in_window(uint32_t slot) const { return win && slot - t0 < top - t0; }
  __device__ uint4 rec_at(uint32_t slot) const {
    if (in_window(slot)) {
      const __attribute__((address_space(3))) uint32_t* w =
          (const __attribute__((address_space(3))) uint32_t*)(wr + wb + (slot - t0));
      return make_uint4(w[0], w[1], w[2], w[3]);
    }
    // The global path waits for its own load where it issues it (as Q<PF>'s ring path does):
    // otherwise the wait lands where the two paths join and on every later use of the record,
    // and the walkers that read LDS wait there for the last forward's stores
    const uint4 r = pool[slot];
    __builtin_amdgcn_s_waitcnt(VMCNT0);
    return r;
  }
  __device__ uint32_t next_at(uint32_t slot) const {
    if (in_window(slot)) return wn[wb + (slot - t0)];
    const uint32_t v = nxt[slot];
    __builtin_amdgcn_s_waitcnt(VMCNT0);
    return v;
  }
  __device__ void load_front() {
    if (n) fr = rec_at(hd[(uint32_t)dq[(front & smask) * 64] * 64]);
  }
  __device__ void set_next(uint32_t slot, uint32_t v) {
    if (in_window(slot)) wn[wb + (slot - t0)] = v;
    else nxt[slot] = v;
  }
  // add_data_source: the record is the window's next one (the caller checked the socket and the room)
  __device__ void push(uint32_t s) {
    const uint32_t slot = top++;
    live++;
    room--;
    if (hd[s * 64] == QD_NONE) {  // not in the deque: to its back
      hd[s * 64] = slot;
      dq[((front + n) & smask) * 64] = (uint8_t)s;
      if (n == 0) {  // the new front: its record is the window's newest
        const __attribute__((address_space(3))) uint32_t* w =
            (const __attribute__((address_space(3))) uint32_t*)(wr + wb + (slot - t0));
        fr = make_uint4(w[0], w[1], w[2], w[3]);
      }
      n++;
    } else {
      set_next(tl[s * 64], slot);
    }
    tl[s * 64] = slot;
  }
  // NetworkInterface::pop
  __device__ bool pop(uint4& rec) {
    if (n == 0) return false;
    const uint32_t s = dq[(front & smask) * 64];
    const uint32_t slot = hd[s * 64];
    rec = fr;
    if (slot == tl[s * 64]) {  // drained: leaves the deque
      hd[s * 64] = QD_NONE;
      n--;
    } else {  // still holds a packet: to the back (the entry the front just left when the deque is full)
      hd[s * 64] = next_at(slot);
      dq[((front + n) & smask) * 64] = (uint8_t)s;
    }
    front++;
    live--;
    load_front();
    return true;
  }
  // The queued records, socket by socket in deque order, into the pool's other half (slots 0,
  // 1, ...); the halves swap.  Outside a window only.
  __device__ void compact() {
    uint32_t k = 0;
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t s = dq[((front + j) & smask) * 64];
      uint32_t slot = hd[s * 64];
      const uint32_t last = tl[s * 64];
      hd[s * 64] = k;
      for (;;) {
        log[k] = pool[slot];
        (nxt - (pool - log))[k] = k + 1;  // the other half's links lie as its records do
        k++;
        if (slot == last) break;
        slot = nxt[slot];
      }
      tl[s * 64] = k - 1;
    }
    nxt -= pool - log;
    uint4* p = pool;
    pool = log;
    log = p;
    top = k;
  }
};

// The relay's forward task at `now` (out_task, sg_outbound.hip), the round-robin interface as its
// source; the records handed to the router go to the log.
template <bool SL>
__device__ void qd_task(QdQ<SL>& q, Relay& r, uint64_t now, const QdiscArgs& a, uint64_t& ctr_inc) {
  r.rf &= (uint8_t)~R_PENDING;
  for (;;) {
    uint4 rec;
    if (r.rf & R_CACHED) {  // next_packet.take(): popped earlier, its socket has rotated
      rec = q.cr;
      r.rf &= (uint8_t)~R_CACHED;
    } else if (!q.pop(rec)) {
      return;  // the interface has nothing: Idle
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
    if (!local) q.log[q.n_log++] = rec;
  }
}

// KEYED as k_outbound's.  SL: n_sock <= QD_LDS_SOCKETS.
template <bool KEYED, bool SL>
__global__ void __launch_bounds__(CD_THREADS) k_qdisc(QdiscArgs a) {
  constexpr uint32_t CH = KEYED ? QD_CHUNK_KEYED : QD_CHUNK;
  const uint64_t d_t0 = a.bdiag ? wall_clock64() : 0;
  uint64_t d_walk = 0;
  __shared__ uint64_t s_t[CH];
  __shared__ uint4 s_r[CH];
  __shared__ uint32_t s_sk[CH], s_n[CH];
  __shared__ uint64_t s_id[KEYED ? CH : 1], s_born[KEYED ? CH : 1];
  __shared__ uint32_t s_head[SL ? QD_LDS_SOCKETS * CD_HOSTS : 1], s_tail[SL ? QD_LDS_SOCKETS * CD_HOSTS : 1];
  __shared__ uint8_t s_dq[SL ? QD_LDS_SOCKETS * CD_HOSTS : 1];
  __shared__ uint32_t s_hb[CD_HOSTS], s_hn[CD_HOSTS];
  const uint32_t h0 = blockIdx.x * CD_HOSTS, t = threadIdx.x;
  const uint32_t h = h0 + t, S = a.n_sock;
  const bool walker = h < a.H;
  uint32_t hb = 0, he = 0, n_start = 0;
  QdQ<SL> q{};
  Relay r{};
  uint64_t ctr_inc = 0, last = 0, last_born = 0, last_id = 0;
  const size_t g0 = qd_slot(h, 0, S);  // (allocated for whole blocks: a valid index past H too)
  if constexpr (SL) {
    q.hd = (typename SockPtr<SL, uint32_t>::type)s_head + t;
    q.tl = (typename SockPtr<SL, uint32_t>::type)s_tail + t;
    q.dq = (typename SockPtr<SL, uint8_t>::type)s_dq + t;
  } else {
    q.hd = a.sk_head + g0;
    q.tl = a.sk_tail + g0;
    q.dq = a.dq + g0;
  }
  if (walker) {
    hb = min(a.host_off[h], a.E);
    he = max(min(a.host_off[h + 1], a.E), hb);
    const uint32_t half = a.half[h];
    q.pool = a.pool + ((size_t)h * 2 + half) * a.cap;
    q.log = a.pool + ((size_t)h * 2 + (half ^ 1u)) * a.cap;
    q.nxt = a.nxt + ((size_t)h * 2 + half) * a.cap;
    q.front = a.dq_front[h];
    q.n = n_start = a.dq_n[h];
    q.smask = S - 1;
    q.top = a.top[h];
    q.live = a.n_live[h];
    q.ip = a.host_ip[h];
    r.rf = a.rflags[h];
    r.tt = a.task_time[h];
    r.cap = a.tb_cap[h];
    r.bal = a.tb_bal[h];
    r.set_inc(a.tb_inc[h]);
    r.last = a.tb_last[h];
    r.ctr0 = a.event_ctr ? a.event_ctr[h] : 0;
    r.tid = a.task_id[h];
    r.tborn = a.task_born[h];
    if (r.rf & R_CACHED) q.cr = a.cached[h];
    const uint32_t held = q.live + ((r.rf & R_CACHED) ? 1u : 0u);
    q.room = a.cap > held ? a.cap - held : 0;
  }
  if constexpr (SL) {  // the lane's own column: no barrier.  An empty interface has every socket empty
    for (uint32_t s = 0; s < S; s++) {
      const bool ld = walker && n_start != 0;
      s_head[s * 64 + t] = ld ? a.sk_head[g0 + s * 64] : QD_NONE;
      s_tail[s * 64 + t] = ld ? a.sk_tail[g0 + s * 64] : QD_NONE;
      s_dq[s * 64 + t] = ld ? a.dq[g0 + s * 64] : (uint8_t)0;
    }
  }
  // the call's sends must fit behind the bump pointer (they do once the pool is compacted)
  if (walker && q.top + (he - hb) > a.cap && q.top != q.live) q.compact();
  if (walker) q.load_front();
  const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)hb, 0);
  const uint32_t p1 = (uint32_t)__builtin_amdgcn_readlane((int)he, (int)min(CD_HOSTS - 1u, a.H - 1u - h0));
  auto due = [&](uint64_t before) { return (r.rf & R_PENDING) && !(r.rf & R_NEVER) && r.tt < before; };
  // a task at the send's own time that runs first: created before the sending Local event
  auto due_tie = [&](uint64_t now, uint64_t born, uint64_t id) {
    return KEYED && (r.rf & R_PENDING) && !(r.rf & R_NEVER) && r.tt == now && id != ~0ull &&
           (r.tborn < born || (r.tborn == born && r.tid < id));
  };
  uint32_t h_act;
  const uint32_t max_n = lane_major_setup<true>(hb, he - hb, s_hb, s_hn, h_act);
  with_chunk_map<true, CH>(lane_major_block<CH>(a.lm, p1 - p0, max_n, h_act), p0, p1, s_hb, s_hn, [&](auto cm) {
    for (uint32_t c = 0; cm.has(c, max_n); c++) {
      const uint32_t clen = cm.len(c);
      for (uint32_t base = 0; base < clen; base += CD_THREADS * CD_UNROLL) {  // staging (see ChunkMap)
        uint64_t rt[CD_UNROLL], ri[KEYED ? CD_UNROLL : 1], rb[KEYED ? CD_UNROLL : 1];
        uint4 rr[CD_UNROLL];
        uint32_t rs[CD_UNROLL];
        bool ok[CD_UNROLL];
#pragma unroll
        for (int u = 0; u < CD_UNROLL; u++) {
          const uint32_t i = cm.event(c, min(base + u * CD_THREADS + t, clen - 1), ok[u]);
          rt[u] = a.time[i];
          rr[u] = make_uint4(a.pkt[i], a.len[i], a.dst[i], a.payload[i]);
          rs[u] = a.sock[i];
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
            s_sk[k] = rs[u];
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
        q.begin_window((lds_rec*)s_r, (lds_link*)s_n, kb);
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
            // the counter steps past the sending event's id as in k_outbound: before a task that
            // runs after the event's creation, and before the send
            while (due(now) || due_tie(now, born, id)) {
              if (id != ~0ull && r.tt > born && id - r.ctr0 >= ctr_inc && id >= r.ctr0) ctr_inc = id + 1 - r.ctr0;
              qd_task(q, r, r.tt, a, ctr_inc);
            }
            // a send whose key equals the pending task's is no event order (two events, one id)
            if (id != ~0ull && (r.rf & R_PENDING) && !(r.rf & R_NEVER) && r.tt == now && r.tborn == born &&
                r.tid == id)
              q.err |= E_ORDER;
            if (id != ~0ull && id - r.ctr0 >= ctr_inc && id >= r.ctr0) ctr_inc = id + 1 - r.ctr0;
          } else {
            while (due(now)) qd_task(q, r, r.tt, a, ctr_inc);
          }
          last = now;
          const uint32_t s = s_sk[k];
          if (s >= S) {  // no such queue
            q.err |= E_SOCKET;
            continue;
          }
          if (q.room == 0) {  // more than ring_cap packets queued at the start or sent by the call
            q.err |= E_FULL;
            continue;
          }
          q.push(s);
          if (!(r.rf & R_PENDING)) r.schedule(now, now, a.sim_end, ctr_inc);  // notify: Idle -> forward_later(ZERO)
        }
        if (q.n == 0) {
          q.top = 0;  // nothing queued (a cached record is in q.cr): the pool starts over
        } else {      // the window's records and links to the pool: the next chunk's staging overwrites them
          for (uint32_t j = 0; j < q.top - q.t0; j++) {
            q.pool[q.t0 + j] = s_r[q.wb + j];
            q.nxt[q.t0 + j] = s_n[q.wb + j];
          }
        }
        if (a.bdiag) d_walk += clock64() - d_w0;
        q.win = false;
      }
      __syncthreads();
    }
  });
  unsigned long long err = 0, sent = 0;
  if (walker) {
    while (due(a.window_end)) qd_task(q, r, r.tt, a, ctr_inc);
    if (q.n == 0) q.top = 0;
    a.dq_front[h] = q.front;
    a.dq_n[h] = q.n;
    a.top[h] = q.top;
    a.n_live[h] = q.live;
    a.half[h] = (uint8_t)(q.pool == a.pool + ((size_t)h * 2 + 1) * a.cap ? 1 : 0);
    if (r.rf & R_CACHED) a.cached[h] = q.cr;
    a.n_fwd[h] = q.n_log;
    a.rflags[h] = r.rf;
    a.task_time[h] = r.tt;
    a.tb_bal[h] = r.bal;
    a.tb_last[h] = r.last;
    a.task_id[h] = r.tid;
    a.task_born[h] = r.tborn;
    if (a.event_ctr && ctr_inc) a.event_ctr[h] += ctr_inc;
    err = q.err;
    sent = q.n_log;
  }
  if constexpr (SL) {  // an interface empty before and after left its (all-empty) sockets as they were
    if (walker && (n_start != 0 || q.n != 0)) {
      for (uint32_t s = 0; s < S; s++) {
        a.sk_head[g0 + s * 64] = s_head[s * 64 + t];
        a.sk_tail[g0 + s * 64] = s_tail[s * 64 + t];
        a.dq[g0 + s * 64] = s_dq[s * 64 + t];
      }
    }
  }
  lane_diag_store(a.bdiag, d_t0, d_walk, he - hb);
  for (int d = 32; d > 0; d >>= 1) {
    sent += __shfl_xor(sent, d, 64);
    err |= __shfl_xor(err, d, 64);
  }
  if (t == 0) {
    a.blk[2 * blockIdx.x] = sent;
    a.blk[2 * blockIdx.x + 1] = err;
  }
}

// The sent batch: block b owns hosts [64b, 64b + 64), whose logs (n_fwd records each, in the
// idle half of the host's pool) it walks as one concatenated sequence, 256 records per step,
// into its slice [boff[b], ...) of the batch: loads coalesced within a host's log, stores
// coalesced throughout.  Locals were never logged, so a record's rank is its position.
__global__ void __launch_bounds__(256) k_qd_compact(uint32_t H, const uint32_t* __restrict__ n_fwd,
                                                    const uint8_t* __restrict__ half,
                                                    const uint4* __restrict__ pool, uint32_t cap,
                                                    const uint64_t* __restrict__ fwd_time, uint32_t n_status,
                                                    const uint32_t* __restrict__ boff, sg_outbound_sent out) {
  __shared__ uint32_t s_off[CD_HOSTS + 1], s_half[CD_HOSTS];
  const uint32_t h0 = blockIdx.x * CD_HOSTS, t = threadIdx.x, lane = t & 63;
  if (t < 64) {
    const uint32_t h = h0 + t;
    uint32_t x = h < H ? min(n_fwd[h], cap) : 0;
    s_half[t] = h < H ? (half[h] ^ 1u) : 0;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (lane >= (uint32_t)d) x += y;
    }
    s_off[t + 1] = x;
    if (t == 0) s_off[0] = 0;
  }
  __syncthreads();
  const uint32_t n = s_off[CD_HOSTS], o = boff[blockIdx.x];
  for (uint32_t j = t; j < n; j += 256) {
    uint32_t lo = 0, hi = CD_HOSTS;  // the host k with s_off[k] <= j < s_off[k + 1]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_off[mid] <= j) lo = mid;
      else hi = mid;
    }
    const uint4 rec = pool[((size_t)(h0 + lo) * 2 + s_half[lo]) * cap + (j - s_off[lo])];
    const uint32_t pos = o + j;
    if (pos < out.cap) {
      out.src_host[pos] = h0 + lo;
      out.dst_ipv4[pos] = rec.z;
      out.payload_len[pos] = rec.w;
      out.send_time_ns[pos] = rec.x < n_status ? fwd_time[rec.x] : 0;
      out.packet[pos] = rec.x;
    }
  }
}

// sg_outbound_get_qdisc_state: every host compacts (its queued records then lie in canonical
// order in its pool, slots [0, n_live)), and the deque and the sockets' counts are listed.
__global__ void __launch_bounds__(64) k_qd_canon(uint32_t H, uint32_t n_sock, uint32_t cap, uint4* pool, uint32_t* nxt,
                                                 uint32_t* sk_head, uint32_t* sk_tail, uint8_t* dq,
                                                 const uint32_t* dq_front, const uint32_t* dq_n, uint32_t* top,
                                                 uint8_t* half, uint32_t* active, uint32_t* count) {
  const uint32_t h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  QdQ<false> q{};
  const size_t g0 = qd_slot(h, 0, n_sock);
  const uint32_t hf = half[h];
  q.hd = sk_head + g0;
  q.tl = sk_tail + g0;
  q.dq = dq + g0;
  q.pool = pool + ((size_t)h * 2 + hf) * cap;
  q.log = pool + ((size_t)h * 2 + (hf ^ 1u)) * cap;
  q.nxt = nxt + ((size_t)h * 2 + hf) * cap;
  q.front = dq_front[h];
  q.n = dq_n[h];
  q.smask = n_sock - 1;
  if (q.n == 0) return;
  q.compact();
  top[h] = q.top;
  half[h] = (uint8_t)(hf ^ 1u);
  for (uint32_t j = 0; j < q.n; j++) {
    const uint32_t s = q.dq[((q.front + j) & q.smask) * 64];
    active[(size_t)h * n_sock + j] = s;
    count[(size_t)h * n_sock + j] = q.tl[s * 64] - q.hd[s * 64] + 1;
  }
}

}  // namespace
}  // namespace sg

extern "C" {

int32_t sg_outbound_run_qdisc(sg_ctx* ctx, sg_outbound* ob, const sg_outbound_sends* s, const uint32_t* socket,
                              uint64_t window_end_ns, uint64_t bootstrap_end_ns, uint64_t sim_end_ns,
                              uint64_t* event_ctr, uint64_t* fwd_time, uint8_t* pkt_status, uint32_t n_packets,
                              sg_outbound_sent* sent, uint32_t* n_sent) {
  if (ob && ob->qdisc == SG_QDISC_FIFO)  // the socket is irrelevant: host-wide creation order
    return sg_outbound_run(ctx, ob, s, window_end_ns, bootstrap_end_ns, sim_end_ns, event_ctr, fwd_time, pkt_status,
                           n_packets, sent, n_sent);
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (!ob || !s || ob->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "null argument");
    const uint32_t E = s->n, H = ob->n;
    if (n_sent) *n_sent = 0;
    if (E && (!s->host || !s->time_ns || !s->packet || !s->len || !s->payload_len || !s->dst_ipv4))
      throw Error(SG_ERR_INVALID_ARG, "null send array");
    if (E && !socket) throw Error(SG_ERR_INVALID_ARG, "a round-robin interface needs each send's socket");
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
    QdiscArgs a;
    a.host_off = ws;
    a.H = H;
    a.E = E;
    a.time = s->time_ns;
    a.pkt = s->packet;
    a.len = s->len;
    a.payload = s->payload_len;
    a.dst = s->dst_ipv4;
    a.sock = socket;
    a.host_ip = ob->host_ip;
    a.pool = ob->ring;
    a.nxt = ob->nxt;
    a.cap = ob->cap;
    a.n_sock = ob->n_sock;
    a.sk_head = ob->sk_head;
    a.sk_tail = ob->sk_tail;
    a.dq = ob->dq;
    a.dq_front = ob->dq_front;
    a.dq_n = ob->dq_n;
    a.top = ob->top;
    a.n_live = ob->n_live;
    a.half = ob->half;
    a.cached = ob->cached;
    a.n_fwd = ob->start;
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
    a.blk = ctx->d_blk.get<unsigned long long>(2 * (size_t)nb);
    const bool kd = keyed && E, sl = ob->n_sock <= QD_LDS_SOCKETS;
    {
      // per send: 28 B in, a 16-B record logged and gathered, 9 B out; per host: ~120 B of state
      a.bdiag = lane_diag_alloc(nb);
      TimedLaunch tl(ctx, "outbound", 69.0 * E + 120.0 * H);
      a.lm = lane_major_launch(lane_major_env(), E, nb, kd ? QD_CHUNK_KEYED : QD_CHUNK);
      auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(nb), dim3(CD_THREADS), 0, st, a); };
      if (kd)
        sl ? go(k_qdisc<true, true>) : go(k_qdisc<true, false>);
      else
        sl ? go(k_qdisc<false, true>) : go(k_qdisc<false, false>);
    }
    lane_diag_report(st, "k_qdisc", a.bdiag, nb);
    // the blocks' offsets and the sums in one launch, then the gather of the logs
    hipLaunchKernelGGL(k_blk_offsets, dim3(1), dim3(1024), 0, st, a.blk, nb, ob->off, gerr, ob->ret);
    if (sent) {
      sg_outbound_sent o = *sent;
      TimedLaunch tl(ctx, "out_compact", 0.0);
      hipLaunchKernelGGL(k_qd_compact, dim3(nb), dim3(256), 0, st, H, ob->start, ob->half, ob->ring, ob->cap,
                         fwd_time, n_packets, ob->off, o);
    }
    SG_CHECK_LAUNCH();
    SG_HIP(hipStreamSynchronize(st));
    const volatile unsigned long long* r = ob->ret;
    const uint64_t err = r[1];
    if (err & E_UNSORTED) throw Error(SG_ERR_UNSORTED, "sends must be grouped by ascending host");
    if (err & E_HOST) throw Error(SG_ERR_INVALID_ARG, "send host out of range");
    if (err & E_SOCKET) throw Error(SG_ERR_INVALID_ARG, "a send's socket is not below sg_outbound_max_sockets");
    if (err & E_ORDER)
      throw Error(SG_ERR_UNSORTED, "a host's sends must come in execution order (time; Packet events, then "
                                   "Local ones by creation time and id)");
    if (err & E_FULL) throw Error(SG_ERR_CAPACITY, "an interface's queues outgrew its pool (raise ring_cap)");
    if (err & E_PKT) throw Error(SG_ERR_INVALID_ARG, "packet id >= n_packets");
    if (err & E_WINDOW) throw Error(SG_ERR_INVALID_ARG, "a send is at or after window_end");
    const uint64_t ns = r[0];
    if (n_sent) *n_sent = (uint32_t)ns;
    if (sent && ns > sent->cap) throw Error(SG_ERR_CAPACITY, "the sent batch exceeds sent->cap");
  });
}

int32_t sg_outbound_get_qdisc_state(sg_outbound* ob, sg_outbound_qdisc_state* o, sg_inbound_relay_state* rl) {
  if (!ob) return SG_ERR_INVALID_ARG;
  if (rl) {
    const int32_t rc = sg_outbound_get_state(ob, nullptr, rl);
    if (rc != SG_OK) return rc;
  }
  if (!o) return SG_OK;
  return sg::guarded(ob->ctx, [&] {
    using namespace sg;
    if (ob->qdisc != SG_QDISC_ROUND_ROBIN)
      throw Error(SG_ERR_INVALID_ARG, "a fifo interface has one ring: sg_outbound_get_state");
    const size_t n = ob->n, S = ob->n_sock, cap = ob->cap;
    if (!n) return;
    hipStream_t st = ob->ctx->stream;
    uint32_t* d_act = ob->ctx->d_seg.get<uint32_t>(2 * n * S);
    hipLaunchKernelGGL(k_qd_canon, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (uint32_t)n, (uint32_t)S,
                       (uint32_t)cap, ob->ring, ob->nxt, ob->sk_head, ob->sk_tail, ob->dq, ob->dq_front, ob->dq_n,
                       ob->top, ob->half, d_act, d_act + n * S);
    SG_CHECK_LAUNCH();
    std::vector<uint32_t> act(2 * n * S), n_act(n), n_q(n);
    std::vector<uint8_t> half(n), fl(n);
    std::vector<uint4> pool(2 * n * cap), cached(n);
    SG_HIP(hipMemcpyAsync(act.data(), d_act, act.size() * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(n_act.data(), ob->dq_n, n * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(n_q.data(), ob->n_live, n * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(half.data(), ob->half, n, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(fl.data(), ob->rflags, n, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(pool.data(), ob->ring, pool.size() * 16, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(cached.data(), ob->cached, n * 16, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    for (size_t h = 0; h < n; h++) {
      if (o->n_active) o->n_active[h] = n_act[h];
      if (o->n_queued) o->n_queued[h] = n_q[h];
      for (size_t j = 0; j < n_act[h] && j < S; j++) {
        if (o->active) o->active[h * S + j] = act[h * S + j];
        if (o->active_count) o->active_count[h * S + j] = act[n * S + h * S + j];
      }
      const uint4* p = pool.data() + (h * 2 + half[h]) * cap;
      for (size_t i = 0; i < n_q[h] && i < cap; i++) {
        if (o->q_packet) o->q_packet[h * cap + i] = p[i].x;
        if (o->q_len) o->q_len[h * cap + i] = p[i].y;
        if (o->q_dst) o->q_dst[h * cap + i] = p[i].z;
        if (o->q_payload_len) o->q_payload_len[h * cap + i] = p[i].w;
      }
      const uint4 c = (fl[h] & R_CACHED) ? cached[h] : make_uint4(0, 0, 0, 0);
      if (o->cached_packet) o->cached_packet[h] = c.x;
      if (o->cached_len) o->cached_len[h] = c.y;
      if (o->cached_dst) o->cached_dst[h] = c.z;
      if (o->cached_payload_len) o->cached_payload_len[h] = c.w;
    }
  });
}

}  // extern "C"
