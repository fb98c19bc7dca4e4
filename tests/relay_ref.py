"""The relays' forward task and its token bucket, restated per host on Python integers from the
reference's own functions -- not from the oracle's C and not from the kernels' header, which
share one shape (flag bits, one walk).  What is restated, function by function:

  relay/token_bucket.rs   new_inner :37-60, conforming_remove_inner :75-86,
                          compute_conforming_duration :94-120, lazy_refill :127-157
  relay/mod.rs            notify :111-136, forward_later :145-163, run_forward_task :166-178,
                          forward_now :181-187, forward_until_blocked :201-273,
                          create_token_bucket :278-288, get_burst_allowance :317-319
  host/host.rs            get_new_event_id :649-653, schedule_task_with_delay :695-697,
                          push_local_event :703-709 (an event at or past sim_end is never queued;
                          Event::new_local, core/work/event.rs:35-45, took its id before that)
  core/work/event.rs      :84-110: by time, then Packet events before Local ones, Local ones by id
  core/worker.rs          is_bootstrapping :476-478: now < bootstrap_end

Numbers: every count is a Python int.  The bucket's u64 arithmetic saturates where the reference's
does (saturating_mul, saturating_add); EmulatedTime saturates at EMU_MAX.  `now + delay` in
schedule_task_with_delay is a plain add in the reference (it panics past EMU_MAX); here it
saturates at 2^64 - 1 as the library documents, and no case goes there (relay_cases.py's header).

Two pipelines use the relay:

  Inbound   the source is the router's CoDel queue (codel_ref.Queue); an arrival is a Packet
            event that pushes and notifies (host.rs:781-786, :919-924); the forward task pops at
            its own time.  State in oracle.inbound_state's layout.
  Outbound  the source is the network interface (qdisc_ref.Interfaces' two disciplines); a send
            adds a data source and notifies (host.rs:930-945); a packet to the interface's own
            address is local: no tokens, no refill (relay/mod.rs:226-231).  A send may carry the
            key (created, id) of the Local event that made it: at the task's own nanosecond it
            runs first iff that key is below the task's (include/shadow_gpu.h, "Same-time order");
            the counter rules for keyed sends are that header's too.

trace    a dict the model counts into: one key per arm (ARMS) and one per side of every
         comparison ("<name>:lt", ":eq", ":gt", left against right; SIDES lists the sides that
         exist).
variant  one single-site mutation (VARIANTS): what a slip in a kernel would look like.
"""
import numpy as np

import codel_ref
import qdisc_ref

U64, M64 = 2**64 - 1, 2**64
EMU_MAX = codel_ref.EMU_MAX
T0 = 946684800 * 10**9       # EmulatedTime::SIMULATION_START (emulated_time.rs)
INTERVAL = 1_000_000         # relay/mod.rs:279 refill_interval = 1 ms
MTU = 1500                   # definitions.h:124 CONFIG_MTU, the burst allowance
RL_PENDING, RL_NEVER, RL_CACHED = 1, 2, 4
FORWARDED, DROPPED, LOCAL = 1, 2, 2   # packet statuses: inbound 1 / 2 (CoDel drop), outbound 1 / 2 (local)
PACKET_EVENT = U64           # a send's event id when a Packet event made it
E_FULL, E_PKT, E_GROUP, E_WINDOW, E_ORDER = -2, -3, -4, -5, -6
FIFO, ROUND_ROBIN = qdisc_ref.FIFO, qdisc_ref.ROUND_ROBIN

BUCKET_VARIANTS = (
    "span>I", "bal>dec", "nref-floor", "nref<=2", "clamp-dropped", "clamp-cap+1", "tokens-wrap", "bal+tokens-wraps",
    "last=now", "inc-without-max", "cap-without-mtu")
RELAY_VARIANTS = (
    "tt<=arrival", "tt<=window_end", "at>sim_end", "never-takes-no-id", "now>boot", "boot-pop-refills",
    "blocked-requeued", "wake-from-arrival", "group-id-per-arrival")
INBOUND_VARIANTS = ("codel-pop-at-arrival",)
OUTBOUND_VARIANTS = ("local-takes-tokens", "local-refills", "tie-ignores-id", "tie-created<=", "tie-ignores-created")
VARIANTS = BUCKET_VARIANTS + RELAY_VARIANTS + INBOUND_VARIANTS + OUTBOUND_VARIANTS

ARMS = ("refill:none", "refill:some", "tokens:plain", "tokens:saturated", "sum:plain", "sum:saturated", "remove:ok",
        "remove:short", "ceil:exact", "ceil:up", "wait:one-refill", "wait:more-refills", "notify:idle",
        "notify:pending", "later:queued", "later:never", "task:run", "next:cached", "next:popped", "loop:empty",
        "loop:blocked", "limit:bootstrapping", "limit:rate", "forward", "walk:arrival", "walk:task-before-arrival",
        "walk:task-before-window-end", "walk:carried", "walk:idle-end", "walk:never-end")
OUTBOUND_ARMS = ("limit:local", "tie:packet-event", "tie:local-event")
# the sides that exist: need > 0 after a short balance, so nref >= 1; a same-time Local send's
# key never equals the task's (the entry points refuse it: E_ORDER)
SIDES = {"span?I": "lt eq gt", "bal?dec": "lt eq gt", "sum?cap": "lt eq gt", "nref?1": "eq gt", "tt?arrival": "lt eq gt",
         "tt?wend": "lt eq gt", "at?sim_end": "lt eq gt", "now?boot": "lt eq gt"}
OUTBOUND_SIDES = {"born?tborn": "lt eq gt", "id?tid": "lt gt"}


class RelayError(ValueError):
    def __init__(self, code):
        super().__init__(f"relay_ref: error {code}")
        self.code = code


class _Tracer:
    def __init__(self, trace, variant):
        assert variant is None or variant in VARIANTS, variant
        self.trace, self.v = trace, variant

    def hit(self, key):
        if self.trace is not None:
            self.trace[key] = self.trace.get(key, 0) + 1

    def cmp(self, name, a, b):
        if self.trace is not None:
            self.hit(name + (":lt" if a < b else ":eq" if a == b else ":gt"))


class Bucket:
    """TokenBucket as create_token_bucket makes it (relay/mod.rs:278-288): refill max(1, B / 1000)
    bytes per millisecond, capacity refill + MTU, full, last refill at the simulation's start."""

    def __init__(self, bw_bits, tr, t0=T0):
        self.tr = tr
        per_second = int(bw_bits) // 8   # RateLimit::BytesPerSecond (host.rs: bandwidth bits / 8)
        inc = per_second // 1000
        if tr.v != "inc-without-max":
            inc = max(1, inc)
        self.inc = inc
        self.cap = inc + (0 if tr.v == "cap-without-mtu" else MTU)
        self.bal, self.last = self.cap, t0   # new_inner :50-56

    def lazy_refill(self, now):   # :127-157
        tr, v = self.tr, self.tr.v
        assert now >= self.last   # duration_since panics otherwise
        span = now - self.last
        tr.cmp("span?I", span, INTERVAL)
        if span > INTERVAL if v == "span>I" else span >= INTERVAL:
            tr.hit("refill:some")
            n = span // INTERVAL
            tokens = self.inc * n   # saturating_mul :136-138
            if tokens > U64:
                tr.hit("tokens:saturated")
                tokens = tokens % M64 if v == "tokens-wrap" else U64
            else:
                tr.hit("tokens:plain")
            s = self.bal + tokens   # saturating_add :141-143
            if s > U64:
                tr.hit("sum:saturated")
                s = s % M64 if v == "bal+tokens-wraps" else U64
            else:
                tr.hit("sum:plain")
            tr.cmp("sum?cap", s, self.cap)
            self.bal = s if v == "clamp-dropped" else min(s, self.cap + 1) if v == "clamp-cap+1" else min(s, self.cap)
            if v == "last=now":
                self.last = now
            else:
                self.last = min(self.last + min(INTERVAL * n, U64), EMU_MAX)   # :147-150
            span = now - self.last
        else:
            tr.hit("refill:none")
        return INTERVAL - span

    def conforming_remove(self, dec, now):   # :75-86: (True, 0), or (False, the conforming duration)
        tr, v = self.tr, self.tr.v
        nxt = self.lazy_refill(now)
        tr.cmp("bal?dec", self.bal, dec)
        if self.bal > dec if v == "bal>dec" else self.bal >= dec:   # checked_sub
            tr.hit("remove:ok")
            self.bal -= dec
            return True, 0
        tr.hit("remove:short")
        need = max(dec - self.bal, 0)   # compute_conforming_duration :94-120
        q, r = divmod(need, self.inc)   # (a mutant's inc = 0: ZeroDivisionError)
        tr.hit("ceil:up" if r else "ceil:exact")
        nref = q + (1 if r and v != "nref-floor" else 0)
        if v is None:
            assert nref >= 1
        nref = max(nref, 1)   # a mutant's zero refills would wake the task at its own time for ever
        tr.cmp("nref?1", nref, 1)
        if nref <= 2 if v == "nref<=2" else nref == 1:
            tr.hit("wait:one-refill")
            return False, nxt if v is None else max(nxt, 1)   # (a mutant's zero wait: the same, for ever)
        tr.hit("wait:more-refills")
        return False, min(nxt + min(INTERVAL * (nref - 1), U64), U64)


class Relay:
    """One Relay (relay/mod.rs:51-63) and what the host keeps of its forward task: the Local
    event's time, id and creation time, and whether it was queued at all."""

    def __init__(self, bw_bits, tr):
        self.tr = tr
        self.tb = Bucket(bw_bits, tr)
        self.pending = False     # RelayState::Pending (Forwarding exists only inside the loop)
        self.never = False       # push_local_event refused the task: the relay stays Pending for good
        self.tt = self.tid = self.tborn = 0
        self.cached = None       # next_packet
        self.ctr = 0             # the host's event_id_counter, for the call
        self.sim_end = self.boot = 0

    def new_event_id(self):   # host.rs:649-653
        res = self.ctr
        self.ctr = (self.ctr + 1) % M64
        return res

    def notify(self, now):   # :111-136
        if not self.pending:
            self.tr.hit("notify:idle")
            self.forward_later(0, now, now)
            return
        self.tr.hit("notify:pending")
        if self.tr.v == "group-id-per-arrival" and not self.never and self.tt == now and self.tborn == now:
            self.tid = self.new_event_id()

    def forward_later(self, delay, now, base):   # :145-163; base is `now` (a mutant takes another)
        tr = self.tr
        assert not self.pending
        self.pending = True
        at = min(base + delay, U64)   # schedule_task_with_delay host.rs:695-697
        tr.cmp("at?sim_end", at, self.sim_end)
        self.never = at > self.sim_end if tr.v == "at>sim_end" else at >= self.sim_end   # push_local_event :703-709
        tr.hit("later:never" if self.never else "later:queued")
        if self.never and tr.v == "never-takes-no-id":
            self.tid = self.ctr
        else:
            self.tid = self.new_event_id()   # Event::new_local, before the sim_end test
        self.tborn, self.tt = now, at

    def run_forward_task(self, src, before):   # :166-187; before: the event the task runs ahead of
        self.tr.hit("task:run")
        now = self.tt
        self.pending = False
        wait = self.forward_until_blocked(src, now, before)
        if wait is not None:
            base = before if self.tr.v == "wake-from-arrival" and before is not None else now
            self.forward_later(wait, now, base)

    def forward_until_blocked(self, src, now, before):   # :201-273
        tr, v = self.tr, self.tr.v
        tr.cmp("now?boot", now, self.boot)
        bootstrapping = now <= self.boot if v == "now>boot" else now < self.boot   # worker.rs:476-478
        pop_at = before if v == "codel-pop-at-arrival" and before is not None else now
        while True:
            if self.cached is not None:   # next_packet.take().or_else(|| src.pop()) :217
                tr.hit("next:cached")
                rec, self.cached = self.cached, None
            else:
                rec = src.pop(pop_at)
                if rec is None:
                    tr.hit("loop:empty")
                    return None
                tr.hit("next:popped")
            local = src.is_local(rec)
            if bootstrapping:   # :231
                tr.hit("limit:bootstrapping")
                if v == "boot-pop-refills":
                    self.tb.lazy_refill(now)
            elif local:
                tr.hit("limit:local")
                if v == "local-takes-tokens":
                    self.tb.conforming_remove(src.length(rec), now)
                elif v == "local-refills":
                    self.tb.lazy_refill(now)
            else:
                tr.hit("limit:rate")
                ok, wait = self.tb.conforming_remove(src.length(rec), now)   # :235
                if not ok:
                    tr.hit("loop:blocked")
                    if v == "blocked-requeued":
                        src.requeue(rec, now)
                    else:
                        self.cached = rec   # :250-253
                    return wait
            tr.hit("forward")
            src.forward(rec, now, local)   # :262-271

    # ---- the host's event loop over one window ------------------------------------------------
    def walk(self, src, events, window_end, arrive):
        """events: (time, key) in execution order, key None (made by a Packet event) or the
        (created, id) of the Local event that made it; arrive(i, now) pushes event i into the
        source.  Runs every event and every forward task before window_end."""
        tr, v = self.tr, self.tr.v
        e, last = 0, 0
        while True:
            runnable = self.pending and not self.never
            if e < len(events):
                t, key = events[e]
                if t >= window_end:
                    raise RelayError(E_WINDOW)
                if t < last:
                    raise RelayError(E_ORDER)
                task_first = False
                if runnable:
                    tr.cmp("tt?arrival", self.tt, t)
                    task_first = self.tt < t
                    if self.tt == t:   # event.rs:84-110
                        if key is None:
                            tr.hit("tie:packet-event")
                            task_first = v == "tt<=arrival"
                        else:
                            tr.hit("tie:local-event")
                            task_first = not self._send_first(key)
                if task_first:
                    tr.hit("walk:task-before-arrival")
                    if key is not None and self.tt > key[0] and self.ctr <= key[1]:
                        self.ctr = key[1] + 1   # the send's event exists by now: the counter is past its id
                    self.run_forward_task(src, t)
                    continue
                tr.hit("walk:arrival")
                last = t
                if key is not None and self.ctr <= key[1]:
                    self.ctr = key[1] + 1
                arrive(e, t)
                self.notify(t)
                e += 1
            elif runnable:
                tr.cmp("tt?wend", self.tt, window_end)
                if self.tt <= window_end if v == "tt<=window_end" else self.tt < window_end:
                    tr.hit("walk:task-before-window-end")
                    self.run_forward_task(src, None)
                else:
                    tr.hit("walk:carried")
                    return
            else:
                tr.hit("walk:never-end" if self.pending else "walk:idle-end")
                return

    def _send_first(self, key):
        """A Local event's send at the task's own time: first iff (created, id) < the task's."""
        tr, v = self.tr, self.tr.v
        born, eid = key
        if (born, eid) == (self.tborn, self.tid):
            raise RelayError(E_ORDER)   # two events with one id
        tr.cmp("born?tborn", born, self.tborn)
        if v == "tie-ignores-created":
            return eid < self.tid
        if born != self.tborn:
            return born < self.tborn
        tr.cmp("id?tid", eid, self.tid)
        if v == "tie-ignores-id":
            return False
        if v == "tie-created<=":
            return True
        return eid < self.tid

    def rflags(self):
        return (RL_PENDING if self.pending else 0) | (RL_NEVER if self.pending and self.never else 0) | (
            RL_CACHED if self.cached is not None else 0)


def _offsets(host, n_hosts):
    host = np.asarray(host, np.int64)
    if len(host) and (np.any(np.diff(host) < 0) or host[0] < 0 or host[-1] >= n_hosts):
        raise RelayError(E_GROUP)
    return np.searchsorted(host, np.arange(n_hosts + 1))


# ---- inbound: router CoDel queue -> relay_inet_in ---------------------------------------------------
class _Fates(dict):
    """What the CoDel queue tells of a packet: only a drop is a fate here (a dequeued packet is
    the relay's, forwarded or cached)."""

    def __setitem__(self, pkt, s):
        if s == codel_ref.DROPPED:
            super().__setitem__(pkt, s)


class _RouterSource:
    def __init__(self, cap, owner):
        self.fates = _Fates()
        self.q = codel_ref.Queue(cap, self.fates)
        self.o = owner

    def pop(self, now):
        p = self.q.pop(now)
        if p == codel_ref.NONE:
            return None
        return p, int(self.q.len[(self.q.head - 1) % self.q.cap])

    def is_local(self, rec):
        return False

    def length(self, rec):
        return rec[1]

    def requeue(self, rec, now):
        self.q.push(rec[0], rec[1], now)

    def forward(self, rec, now, local):
        self.o.fwd[rec[0]] = now


class Inbound:
    """Every host's router queue and inbound relay; run() has oracle.inbound_run's arguments
    after the state, state() returns oracle.inbound_state's layout."""

    def __init__(self, bw_down_bits, cap, trace=None, variant=None):
        self.tr = _Tracer(trace, variant)
        self.cap = cap
        self.relays = [Relay(b, self.tr) for b in bw_down_bits]
        self.srcs = [_RouterSource(cap, self) for _ in bw_down_bits]
        self.cp = [[0, 0] for _ in bw_down_bits]   # the cached fields keep their last value
        self.fwd = {}

    def run(self, host, time, pkt, length, window_end, bootstrap_end, sim_end, event_ctr, fwd_time, pkt_status):
        off = _offsets(host, len(self.relays))
        time, pkt, length = (np.asarray(a).tolist() for a in (time, pkt, length))
        n_status = len(pkt_status)
        self.fwd = {}
        for h, (r, s) in enumerate(zip(self.relays, self.srcs)):
            a, b = int(off[h]), int(off[h + 1])
            if a == b and not r.pending:
                continue
            r.ctr, r.sim_end, r.boot = int(event_ctr[h]), sim_end, bootstrap_end
            s.fates.clear()

            def arrive(i, now, a=a, s=s):
                try:
                    s.q.push(pkt[a + i], length[a + i], now)   # Router::route_incoming_packet
                except ValueError:
                    raise RelayError(E_FULL)

            r.walk(s, [(time[i], None) for i in range(a, b)], window_end, arrive)
            event_ctr[h] = r.ctr
            if r.cached is not None:
                self.cp[h] = list(r.cached)
            for p in s.fates:
                if p >= n_status:
                    raise RelayError(E_PKT)
                pkt_status[p] = DROPPED
        for p, t in self.fwd.items():
            if p >= n_status:
                raise RelayError(E_PKT)
            pkt_status[p], fwd_time[p] = FORWARDED, t

    def state(self):
        n, cap = len(self.relays), self.cap
        st = codel_ref.new_state(n, cap)
        for h, s in enumerate(self.srcs):
            for k in codel_ref.SCALARS:
                st[k][h] = getattr(s.q, k)
            for k, a in (("ring_pkt", s.q.pkt), ("ring_ts", s.q.ts), ("ring_len", s.q.len)):
                st[k][h * cap:(h + 1) * cap] = a
        st.update(relay_state(self.relays))
        st["cached_pkt"] = np.array([c[0] for c in self.cp], np.uint32)
        st["cached_len"] = np.array([c[1] for c in self.cp], np.uint32)
        return st


def relay_state(relays):
    u = lambda f: np.array([f(r) for r in relays], np.uint64)
    return dict(rflags=np.array([r.rflags() for r in relays], np.uint8), task_time=u(lambda r: r.tt),
                task_id=u(lambda r: r.tid), task_born=u(lambda r: r.tborn), tb_cap=u(lambda r: r.tb.cap),
                tb_bal=u(lambda r: r.tb.bal), tb_inc=u(lambda r: r.tb.inc), tb_last=u(lambda r: r.tb.last))


# ---- outbound: network interface -> relay_inet_out -> router -> send_packet -------------------------
class _InterfaceSource:
    """One host's interface: qdisc_ref's disciplines (its _push / _pop on its per-host object)."""

    def __init__(self, ifs, h, owner, hi):
        self.ifs, self.h, self.o, self.hi = ifs, h, owner, hi
        self.sock = {}   # packet -> its socket (a record is qdisc_ref's: packet, len, payload, dst)

    def pop(self, now):
        return self.ifs._pop(self.h)

    def is_local(self, rec):   # relay/mod.rs:226
        return rec[3] == self.h.ip

    def length(self, rec):
        return rec[1]

    def requeue(self, rec, now):
        self.ifs._push(self.h, self.sock[rec[0]], rec)

    def forward(self, rec, now, local):
        self.sock.pop(rec[0], None)
        self.o.fates.append((rec[0], LOCAL if local else FORWARDED, now))
        if not local:   # Router::push -> Worker::send_packet(now)
            self.o.sent.append((self.hi, rec[3], rec[2], now, rec[0]))


class Outbound:
    """Every host's interface and outbound relay; run() has qdisc_ref.Interfaces.run's arguments."""

    def __init__(self, host_ipv4, bw_up_bits, cap, qdisc=FIFO, max_sockets=1, trace=None, variant=None):
        self.tr = _Tracer(trace, variant)
        self.ifs = qdisc_ref.Interfaces(host_ipv4, bw_up_bits, cap, qdisc, max_sockets)
        self.cap, self.S, self.qdisc = self.ifs.cap, self.ifs.S, qdisc
        self.relays = [Relay(b, self.tr) for b in bw_up_bits]
        self.srcs = [_InterfaceSource(self.ifs, h, self, i) for i, h in enumerate(self.ifs.hosts)]
        self.fates, self.sent = [], []

    def run(self, host, time, pkt, length, payload, dst, socket, window_end, bootstrap_end, sim_end, event_ctr,
            fwd_time, pkt_status, event_id=None, event_created=None):
        assert (event_id is None) == (event_created is None)
        off = _offsets(host, len(self.relays))
        n = len(np.asarray(host))
        time, pkt, length, payload, dst = (np.asarray(a).tolist() for a in (time, pkt, length, payload, dst))
        sock = [0] * n if socket is None else np.asarray(socket).tolist()
        keys = [None] * n
        if event_id is not None:
            eid, born = np.asarray(event_id, np.uint64).tolist(), np.asarray(event_created, np.uint64).tolist()
            keys = [None if i == PACKET_EVENT else (b, i) for i, b in zip(eid, born)]
        self.fates, self.sent = [], []
        for h, (r, s) in enumerate(zip(self.relays, self.srcs)):
            a, b = int(off[h]), int(off[h + 1])
            if a == b and not r.pending:
                continue
            for i in range(a + 1, b):   # sends at one time come in execution order (shadow_gpu.h, sg_outbound_sends)
                if time[i] == time[i - 1] and keys[i - 1] is not None and (keys[i] is None or keys[i] < keys[i - 1]):
                    raise RelayError(E_ORDER)
            r.ctr, r.sim_end, r.boot = int(event_ctr[h]), sim_end, bootstrap_end
            room = [self.cap - s.h.n - (r.cached is not None)]   # ring_cap: queued at the start + the call's sends

            def arrive(i, now, a=a, s=s, room=room):
                if room[0] <= 0:
                    raise RelayError(E_FULL)
                room[0] -= 1
                j = a + i
                s.sock[pkt[j]] = sock[j]
                self.ifs._push(s.h, sock[j], (pkt[j], length[j], payload[j], dst[j]))   # add_data_source

            r.walk(s, [(time[i], keys[i]) for i in range(a, b)], window_end, arrive)
            event_ctr[h] = r.ctr
        for p, s, t in self.fates:
            if p >= len(pkt_status):
                raise RelayError(E_PKT)
            pkt_status[p], fwd_time[p] = s, t
        dt = (("src_host", np.uint32), ("dst_ipv4", np.uint32), ("payload_len", np.uint32), ("send_time", np.uint64),
              ("packet", np.uint32))
        return {k: np.array([x[j] for x in self.sent], d) for j, (k, d) in enumerate(dt)}

    def relay_state(self):
        return relay_state(self.relays)

    def queued(self, h):
        """Host h's packets still to go, in the order a fifo ring holds them: the cached one, then the queue."""
        r, q = self.relays[h], self.ifs.hosts[h].q.get(0, ())
        return ([r.cached] if r.cached is not None else []) + list(q)

    def qdisc_state(self):
        for r, h in zip(self.relays, self.ifs.hosts):
            h.cached = r.cached
        return self.ifs.qdisc_state()
