"""A per-host restatement of the network interface's two queueing disciplines and the
outbound relay's forward loop, in plain Python integers: the reference model of
sg_outbound_run_qdisc (tests/test_qdisc_gpu.py compares the library with it bit for bit,
tests/test_qdisc_ref_cpu.py compares it with the oracle where the two must agree).

The interface (host/network/interface.rs:97-108, :168-181, :227-259; queuing.rs):

  fifo          the sending sockets are kept by the priority of their next packet, which is
                host-wide creation order: a host's sends are one FIFO, the socket is irrelevant.
  round-robin   a deque of socket ids without duplicates (send_sockets and its membership
                set) and a FIFO of packets per socket.  A send appends to its socket's FIFO and
                pushes the socket to the deque's back unless it is already queued
                (add_data_source).  pop() takes the front socket and its oldest packet, and
                pushes the socket to the back if it still holds a packet.

The relay (relay/mod.rs:111-273) is the same for both: a forward task pops until the interface
is empty or the token bucket (relay/token_bucket.rs) blocks; the blocked packet is cached (it
was already popped, so its socket has already rotated) and the task reschedules itself after
the conforming duration.  Packets to the host's own address use no tokens.  The order of a
send against a task at the same nanosecond, the event-counter advances and the sim_end rule
follow oracle/sg_oracle.c outbound_impl line by line.
"""
from collections import deque

import numpy as np

U64 = 2**64 - 1
T0 = 946684800 * 10**9
TB_INTERVAL = 1_000_000  # relay/mod.rs:297
MTU = 1500               # definitions.h:124
RL_PENDING, RL_NEVER, RL_CACHED = 1, 2, 4
FIFO, ROUND_ROBIN = "fifo", "round-robin"
E_FULL, E_PKT, E_GROUP, E_WINDOW, E_ORDER, E_SOCKET = -2, -3, -4, -5, -6, -8


class QdiscError(ValueError):
    def __init__(self, code):
        super().__init__(f"qdisc_ref: error {code}")
        self.code = code


def _sat_add(a, b):
    return min(a + b, U64)


class _Bucket:
    """TokenBucket with lazy refills (token_bucket.rs:6-12, :76-158), u64 saturating."""

    def __init__(self, cap, inc, last):
        self.cap, self.bal, self.inc, self.last = cap, cap, inc, last

    def remove(self, dec, now):
        """conforming_remove: (True, 0), or (False, the conforming duration)."""
        span = now - self.last
        if span >= TB_INTERVAL:  # lazy_refill
            n = span // TB_INTERVAL
            self.bal = min(self.cap, _sat_add(self.bal, min(self.inc * n, U64)))
            self.last = min(_sat_add(self.last, min(TB_INTERVAL * n, U64)), U64 - 1)
            span = now - self.last
        nxt = TB_INTERVAL - span
        if self.bal >= dec:
            self.bal -= dec
            return True, 0
        need = dec - self.bal
        nref = -(-need // self.inc)
        return False, nxt if nref == 1 else _sat_add(nxt, min(TB_INTERVAL * (nref - 1), U64))


class _Host:
    def __init__(self, ip, bw, t0):
        inc = max(1, (int(bw) // 8) // 1000)  # create_token_bucket (relay/mod.rs:278-315)
        self.ip = int(ip)
        self.tb = _Bucket(inc + MTU, inc, t0)
        self.rf, self.tt, self.tid, self.tborn = 0, 0, 0, 0
        self.cached = None
        self.dq = deque()   # round-robin: socket ids; fifo: unused
        self.q = {}         # round-robin: socket -> deque of records; fifo: {0: deque}
        self.n = 0          # packets queued (the cached one not counted)


class Interfaces:
    """Every host's interface + outbound relay.  `cap` and `max_sockets` are rounded up to
    powers of two like the library's."""

    def __init__(self, host_ipv4, bw_up_bits, cap, qdisc=FIFO, max_sockets=1, t0=T0):
        assert qdisc in (FIFO, ROUND_ROBIN)
        self.qdisc = qdisc
        self.cap = 1 << max(0, int(cap) - 1).bit_length()
        self.S = 1 << max(0, int(max_sockets) - 1).bit_length()
        self.hosts = [_Host(ip, bw, t0) for ip, bw in zip(host_ipv4, bw_up_bits)]

    # -- the interface ---------------------------------------------------------------
    def _push(self, h, sock, rec):
        if self.qdisc == FIFO:
            h.q.setdefault(0, deque()).append(rec)
        else:
            q = h.q.setdefault(sock, deque())
            q.append(rec)
            if len(q) == 1:  # add_data_source: a socket already queued is ignored
                h.dq.append(sock)
        h.n += 1

    def _pop(self, h):
        if h.n == 0:
            return None
        h.n -= 1
        if self.qdisc == FIFO:
            return h.q[0].popleft()
        s = h.dq.popleft()
        rec = h.q[s].popleft()
        if h.q[s]:  # still holds a packet: back of the deque
            h.dq.append(s)
        return rec

    # -- one window ------------------------------------------------------------------
    def run(self, host, time, pkt, length, payload, dst, socket, window_end, bootstrap_end, sim_end,
            event_ctr, fwd_time, pkt_status, event_id=None, event_created=None):
        """Sends grouped by ascending host, each host's in execution order.  Updates event_ctr,
        fwd_time and pkt_status in place and returns the sent batch (send_packet order)."""
        assert (event_id is None) == (event_created is None)
        host = np.asarray(host, np.int64)
        n = len(host)
        if n and (np.any(np.diff(host) < 0) or host[0] < 0 or host[-1] >= len(self.hosts)):
            raise QdiscError(E_GROUP)
        tm = [int(x) for x in np.asarray(time, np.uint64)]
        recs = list(zip((int(x) for x in pkt), (int(x) for x in length), (int(x) for x in payload),
                        (int(x) for x in dst)))
        sock = [0] * n if socket is None else [int(x) for x in socket]
        if self.qdisc == ROUND_ROBIN and any(s >= self.S for s in sock):
            raise QdiscError(E_SOCKET)
        eid = None if event_id is None else [int(x) for x in np.asarray(event_id, np.uint64)]
        eborn = None if event_created is None else [int(x) for x in np.asarray(event_created, np.uint64)]
        off = np.searchsorted(host, np.arange(len(self.hosts) + 1))
        n_status = len(pkt_status)
        out = dict(src_host=[], dst_ipv4=[], payload_len=[], send_time=[], packet=[])
        for hi, h in enumerate(self.hosts):
            e, e1 = int(off[hi]), int(off[hi + 1])
            e_first, last = e, 0
            room = self.cap - h.n - (1 if h.rf & RL_CACHED else 0)  # ring_cap: queued at the start + sends
            ctr = int(event_ctr[hi])
            tb = h.tb
            while True:
                has_send = e < e1
                has_task = bool(h.rf & RL_PENDING) and not (h.rf & RL_NEVER) and h.tt < window_end
                if has_send and tm[e] >= window_end:
                    raise QdiscError(E_WINDOW)
                if has_send and tm[e] < last:
                    raise QdiscError(E_ORDER)
                if has_send and eid is not None and e > e_first and tm[e] == tm[e - 1]:
                    pk, ppk = eid[e] == U64, eid[e - 1] == U64
                    if (pk and not ppk) or (not pk and not ppk and (eborn[e], eid[e]) < (eborn[e - 1], eid[e - 1])):
                        raise QdiscError(E_ORDER)
                send_first = has_send and (not has_task or tm[e] < h.tt)
                if has_send and has_task and tm[e] == h.tt:
                    if eid is not None and eid[e] != U64 and (eborn[e], eid[e]) == (h.tborn, h.tid):
                        raise QdiscError(E_ORDER)
                    send_first = eid is None or eid[e] == U64 or (eborn[e], eid[e]) < (h.tborn, h.tid)
                if send_first:  # add_data_source + Relay::notify
                    now = last = tm[e]
                    if eid is not None and eid[e] != U64 and ctr <= eid[e]:
                        ctr = eid[e] + 1
                    if room <= 0:
                        raise QdiscError(E_FULL)
                    room -= 1
                    self._push(h, sock[e], recs[e])
                    if not h.rf & RL_PENDING:  # Idle -> forward_later(ZERO)
                        h.tid, h.tborn, h.tt = ctr, now, now
                        ctr = (ctr + 1) & U64
                        h.rf |= RL_PENDING | (RL_NEVER if now >= sim_end else 0)
                    e += 1
                elif has_task:  # run_forward_task -> forward_until_blocked
                    now = h.tt
                    if has_send and eid is not None and eid[e] != U64 and h.tt > eborn[e] and ctr <= eid[e]:
                        ctr = eid[e] + 1
                    h.rf &= ~RL_PENDING
                    while True:
                        if h.rf & RL_CACHED:  # next_packet.take()
                            rec, h.cached = h.cached, None
                            h.rf &= ~RL_CACHED
                        else:
                            rec = self._pop(h)
                            if rec is None:
                                break  # the interface is empty: Idle
                        p, ln, pay, d = rec
                        local = d == h.ip
                        if not local and now >= bootstrap_end:
                            ok, wait = tb.remove(ln, now)
                            if not ok:  # RelayCached; forward_later(wait)
                                h.cached = rec
                                h.rf |= RL_CACHED | RL_PENDING
                                h.tid, h.tborn = ctr, now
                                ctr = (ctr + 1) & U64
                                h.tt = _sat_add(now, wait)
                                if h.tt >= sim_end:
                                    h.rf |= RL_NEVER
                                break
                        if p >= n_status:
                            raise QdiscError(E_PKT)
                        pkt_status[p] = 2 if local else 1
                        fwd_time[p] = now
                        if not local:
                            out["src_host"].append(hi)
                            out["dst_ipv4"].append(d)
                            out["payload_len"].append(pay)
                            out["send_time"].append(now)
                            out["packet"].append(p)
                else:
                    break
            event_ctr[hi] = ctr
        dt = dict(src_host=np.uint32, dst_ipv4=np.uint32, payload_len=np.uint32, send_time=np.uint64, packet=np.uint32)
        return {k: np.array(v, dtype=dt[k]) for k, v in out.items()}

    # -- state -------------------------------------------------------------------------
    def relay_state(self):
        H = self.hosts
        u = lambda f: np.array([f(h) for h in H], np.uint64)
        return dict(rflags=np.array([h.rf for h in H], np.uint8), task_time=u(lambda h: h.tt),
                    task_id=u(lambda h: h.tid), task_born=u(lambda h: h.tborn), tb_cap=u(lambda h: h.tb.cap),
                    tb_bal=u(lambda h: h.tb.bal), tb_inc=u(lambda h: h.tb.inc), tb_last=u(lambda h: h.tb.last))

    def qdisc_state(self):
        """The canonical state (sg_outbound_qdisc_state): the deque front to back, each active
        socket's packet count, the queued packets socket by socket in deque order (each socket's
        in FIFO order), and the cached packet."""
        assert self.qdisc == ROUND_ROBIN
        n, S, c = len(self.hosts), self.S, self.cap
        st = dict(n_active=np.zeros(n, np.uint32), active=np.zeros(n * S, np.uint32),
                  active_count=np.zeros(n * S, np.uint32), n_queued=np.zeros(n, np.uint32),
                  q_packet=np.zeros(n * c, np.uint32), q_len=np.zeros(n * c, np.uint32),
                  q_payload_len=np.zeros(n * c, np.uint32), q_dst=np.zeros(n * c, np.uint32),
                  cached_packet=np.zeros(n, np.uint32), cached_len=np.zeros(n, np.uint32),
                  cached_payload_len=np.zeros(n, np.uint32), cached_dst=np.zeros(n, np.uint32))
        for hi, h in enumerate(self.hosts):
            st["n_active"][hi] = len(h.dq)
            st["n_queued"][hi] = h.n
            k = hi * c
            for j, s in enumerate(h.dq):
                st["active"][hi * S + j] = s
                st["active_count"][hi * S + j] = len(h.q[s])
                for p, ln, pay, d in h.q[s]:
                    st["q_packet"][k], st["q_len"][k], st["q_payload_len"][k], st["q_dst"][k] = p, ln, pay, d
                    k += 1
            if h.cached is not None:
                (st["cached_packet"][hi], st["cached_len"][hi], st["cached_payload_len"][hi],
                 st["cached_dst"][hi]) = h.cached
        return st
