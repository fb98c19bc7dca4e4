"""The routers' CoDel queue, restated from the reference function by function
(router/codel_queue.rs) on Python integers.  Deliberately not the oracle's C and not the
kernel's header: those two share their shape (flags, one pop routine); this follows the
reference's own functions -- push (:303-317), pop (:125-148), drop_from_store_mode (:150-170),
drop_from_drop_mode (:172-201), codel_pop (:204-227), process_standing_delay (:231-262),
should_drop (:265-270), was_dropping_recently (:273-281), apply_control_law (:285-298).

Numbers: every time and counter is a Python int.  EmulatedTime saturates at EMU_MAX
(emulated_time.rs:30, as the oracle has it); the reference's usize counters wrap at 2^64 as
its release build does (one case goes there, for apply_control_law's count-0 arm).  The
reference's VecDeque is the ring of `cap` slots the oracle and the device use, head and tail
running u32 counters taken modulo 2^32 (slot = counter % cap, cap a power of two).  An Option
field is its flag bit plus the field's last value, which stays where it was when the Option
becomes None: the layout of oracle.codel_state / CoDelQueues.get_state, compared key by key.

`run` has oracle.codel_run's signature and two more arguments:

trace    a dict the model counts into: one key per arm of every branch (ARMS), three per
         comparison (COMPARISONS: "<name>:lt", ":eq", ":gt", left against right), and for
         drop_from_drop_mode "drops_per_pop:<k>" and "drop_exit:<why>" (DROP_EXITS).
variant  one single-site mutation (VARIANTS) -- what a slip in a kernel would look like; the
         case file has teeth when every variant changes some case's outcome.
"""
import math

import numpy as np

TARGET = 10_000_000          # codel_queue.rs:23
INTERVAL = 100_000_000       # codel_queue.rs:28
MTU = 1500                   # definitions.h:124 CONFIG_MTU
EMU_MAX = (1 << 64) - 2      # emulated_time.rs:30 EMUTIME_MAX
M32, M64 = 1 << 32, 1 << 64
F_DROP, F_IEND, F_DNEXT = 1, 2, 4   # mode == Drop, interval_end is Some, drop_next is Some
PUSH, POP = 0, 1
NONE = 0xFFFFFFFF
DEQUEUED, DROPPED = 1, 2
SCALARS = ("flags", "interval_end", "drop_next", "cur", "prev", "bytes", "head", "tail")

VARIANTS = (
    "sd<=T", "bytes<MTU", "bytes-before-subtract", "now>iend", "iend-not-cleared-on-good",
    "iend-not-cleared-on-empty", "drop-mode-kept-on-empty", "drop-mode-kept-on-good", "now>dnext", "recent<=16I",
    "recent-ignores-unset-dnext", "recent-false-when-now<dnext", "delta>=1", "delta>2", "delta-wraps",
    "prev-not-updated", "store-drop-law-from-dnext", "drop-law-from-now", "law-advances-on-last", "sojourn-of-next",
    "second-pop-skips-standing", "law-rint", "law-trunc", "law-f32-sqrt", "law-rcp-mul", "counters-not-modular")

# Mutations that no case can catch, and why (test_codel_ref_cpu.py asserts that exactly these survive)
UNCATCHABLE = {
    "delta>=1": "equivalent: it differs only at delta == 1, where resuming takes cur = delta = 1 and "
                "restarting takes cur = 1 -- the same drop_next, prev and mode",
    "law-rcp-mul": "no count found at which INTERVAL * (1 / sqrt) rounds to another step than INTERVAL / sqrt: at the "
                   "exact ties (sqrt = 512 * 5^j) the product rounds back onto the tie, and elsewhere the quotient "
                   "would have to lie within an ulp or two of a half-integer (searched: every count to 2^22, and "
                   "the counts around (INTERVAL / (m + 1/2))^2 for m < 2,000)",
}

COMPARISONS = ("sd?TARGET", "bytes?MTU", "now?iend", "now?dnext", "since?16I", "delta?1", "cur?prev", "bytes?len")
ARMS = ("push", "pop:empty", "pop:good", "pop:store-entry", "pop:drop-mode", "codel_pop:empty", "codel_pop:element",
        "standing:good", "standing:bad-interval-running", "standing:bad-interval-starts", "should_drop:unset",
        "should_drop:set", "recent:unset", "recent:set", "store:next-some", "store:next-none", "store:resume",
        "store:restart", "drop:law", "drop:leave", "law:count0", "law:count", "sat_add:plain", "sat_add:saturated")
DROP_EXITS = ("empty", "not-ok", "dnext-future")


def round_half_away(x: float) -> int:
    """f64::round for x >= 0: to the nearest integer, a tie away from zero.  x - floor(x) is
    exact (both below 2^52 here or x is an integer already)."""
    f = math.floor(x)
    return f + 1 if x - f >= 0.5 else f


def law_increment(count: int, variant=None) -> int:
    """apply_control_law's increment (:286-294): round(INTERVAL / sqrt(count as f64)), count 0 as 1."""
    interval = float(INTERVAL)
    if count == 0:
        s = 1.0
    elif variant == "law-f32-sqrt":
        s = float(np.sqrt(np.float32(count)))
    else:
        s = math.sqrt(float(count))   # int -> float rounds to nearest even, as `count as f64`
    div = interval * (1.0 / s) if variant == "law-rcp-mul" else interval / s
    if variant == "law-rint":
        return int(np.rint(div))
    if variant == "law-trunc":
        return int(div)
    return round_half_away(div)


def _nothing(*_):
    pass


class Queue:
    """One CoDelQueue (:65-81)."""

    def __init__(self, cap, status, trace=None, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.cap, self.status, self.trace, self.v = cap, status, trace, variant
        self.flags = self.interval_end = self.drop_next = self.cur = self.prev = self.bytes = 0   # new() :85-95
        self.head = self.tail = 0
        self.pkt, self.ts, self.len = [0] * cap, [0] * cap, [0] * cap
        if trace is None:   # nothing to count: the streams of 180k events run through here
            self._hit = self._cmp = _nothing

    # -- bookkeeping ---------------------------------------------------------------------------
    def _hit(self, key):
        self.trace[key] = self.trace.get(key, 0) + 1

    def _cmp(self, name, a, b):
        self._hit(name + (":lt" if a < b else ":eq" if a == b else ":gt"))

    def _count(self):   # elements.len()
        if self.v == "counters-not-modular":
            return max(self.tail - self.head, 0)
        return (self.tail - self.head) % M32

    def _sat_add(self, t, d):   # EmulatedTime::saturating_add
        if t > EMU_MAX - d:
            self._hit("sat_add:saturated")
            return EMU_MAX
        self._hit("sat_add:plain")
        return t + d

    def _drop_packet(self, pkt):   # :319-321 RouterDropped
        self.status[pkt] = DROPPED

    # -- the reference's functions --------------------------------------------------------------
    def push(self, pkt, length, now):   # :303-317 (LIMIT = usize::MAX: the ring's size is the caller's)
        if self._count() >= self.cap:
            raise ValueError("ring full")
        self._hit("push")
        self.bytes = (self.bytes + length) % M64
        s = self.tail % self.cap
        self.pkt[s], self.ts[s], self.len[s] = pkt, now, length
        self.tail = (self.tail + 1) % M32

    def pop(self, now):   # :125-148
        item = self.codel_pop(now)
        if item is None:
            self._hit("pop:empty")
            if self.v != "drop-mode-kept-on-empty":
                self.flags &= ~F_DROP   # :140
            return NONE
        pkt, ok = item
        if not ok:
            self._hit("pop:good")
            if self.v != "drop-mode-kept-on-good":
                self.flags &= ~F_DROP   # :134
            out = pkt
        elif not self.flags & F_DROP:
            self._hit("pop:store-entry")
            out = self.drop_from_store_mode(now, pkt)
        else:
            self._hit("pop:drop-mode")
            out = self.drop_from_drop_mode(now, pkt)
        if out != NONE:
            self.status[out] = DEQUEUED   # :145-147
        return out

    def drop_from_store_mode(self, now, pkt):   # :150-170
        self._drop_packet(pkt)
        nxt = self.codel_pop(now, second=True)
        self._hit("store:next-none" if nxt is None else "store:next-some")
        self.flags |= F_DROP
        self._cmp("cur?prev", self.cur, self.prev)
        if self.v == "delta-wraps":
            delta = (self.cur - self.prev) % M64
        else:
            delta = self.cur - self.prev if self.cur > self.prev else 0   # saturating_sub :159-161
        resume = self.was_dropping_recently(now)
        if resume:   # && short-circuits :162
            self._cmp("delta?1", delta, 1)
            resume = delta >= 1 if self.v == "delta>=1" else delta > 2 if self.v == "delta>2" else delta > 1
        self._hit("store:resume" if resume else "store:restart")
        self.cur = delta if resume else 1
        base = self.drop_next if self.v == "store-drop-law-from-dnext" else now
        self.drop_next = self.apply_control_law(base, self.cur)   # :166
        self.flags |= F_DNEXT
        if self.v != "prev-not-updated":
            self.prev = self.cur   # :167
        return NONE if nxt is None else nxt[0]

    def drop_from_drop_mode(self, now, pkt):   # :172-201
        item, drops = (pkt, True), 0
        while True:   # :181, in its order
            if item is None:
                why = "empty"
                break
            if not self.flags & F_DROP:
                why = "not-ok"
                break
            if not self.should_drop(now):
                why = "dnext-future"
                break
            self._drop_packet(item[0])
            self.cur = (self.cur + 1) % M64
            drops += 1
            item = self.codel_pop(now)
            if item is not None and item[1]:
                self._hit("drop:law")
                base = now if self.v == "drop-law-from-now" else self.drop_next
                self.drop_next = self.apply_control_law(base, self.cur)   # :191-194
            else:
                self._hit("drop:leave")
                self.flags &= ~F_DROP   # :196
                if self.v == "law-advances-on-last":
                    self.drop_next = self.apply_control_law(self.drop_next, self.cur)
        self._hit("drops_per_pop:%d" % drops)
        self._hit("drop_exit:" + why)
        return NONE if item is None else item[0]

    def codel_pop(self, now, second=False):   # :204-227
        skip = second and self.v == "second-pop-skips-standing"
        if self._count() == 0:
            self._hit("codel_pop:empty")
            if self.v != "iend-not-cleared-on-empty" and not skip:
                self.flags &= ~F_IEND   # :223
            return None
        self._hit("codel_pop:element")
        s = self.head % self.cap
        pkt, ts, length = int(self.pkt[s]), int(self.ts[s]), int(self.len[s])
        self.head = (self.head + 1) % M32
        before = self.bytes
        self._cmp("bytes?len", self.bytes, length)
        self.bytes = self.bytes - length if self.bytes > length else 0   # saturating_sub :209-210
        if self.v == "sojourn-of-next" and self._count():
            ts = int(self.ts[self.head % self.cap])
        standing_delay = now - ts if now > ts else 0   # saturating_duration_since :213
        if skip:
            return pkt, False
        stored = before if self.v == "bytes-before-subtract" else self.bytes
        return pkt, self.process_standing_delay(now, standing_delay, stored)

    def process_standing_delay(self, now, standing_delay, stored):   # :231-262
        self._cmp("sd?TARGET", standing_delay, TARGET)
        good = standing_delay <= TARGET if self.v == "sd<=T" else standing_delay < TARGET
        if not good:   # || short-circuits :236
            self._cmp("bytes?MTU", stored, MTU)
            good = stored < MTU if self.v == "bytes<MTU" else stored <= MTU
        if good:
            self._hit("standing:good")
            if self.v != "iend-not-cleared-on-good":
                self.flags &= ~F_IEND   # :240
            return False
        if self.flags & F_IEND:
            self._hit("standing:bad-interval-running")
            self._cmp("now?iend", now, self.interval_end)
            return now > self.interval_end if self.v == "now>iend" else now >= self.interval_end   # :250
        self._hit("standing:bad-interval-starts")
        self.interval_end = self._sat_add(now, INTERVAL)   # :257
        self.flags |= F_IEND
        return False

    def should_drop(self, now):   # :265-270
        if not self.flags & F_DNEXT:
            self._hit("should_drop:unset")
            return False
        self._hit("should_drop:set")
        self._cmp("now?dnext", now, self.drop_next)
        return now > self.drop_next if self.v == "now>dnext" else now >= self.drop_next

    def was_dropping_recently(self, now):   # :273-281
        if not self.flags & F_DNEXT and self.v != "recent-ignores-unset-dnext":
            self._hit("recent:unset")
            return False
        self._hit("recent:set")
        if self.v == "recent-false-when-now<dnext" and now < self.drop_next:
            return False
        since = now - self.drop_next if now > self.drop_next else 0   # saturating_duration_since :277
        self._cmp("since?16I", since, 16 * INTERVAL)
        return since <= 16 * INTERVAL if self.v == "recent<=16I" else since < 16 * INTERVAL

    def apply_control_law(self, time, count):   # :285-298
        self._hit("law:count0" if count == 0 else "law:count")
        return self._sat_add(time, law_increment(count, self.v))


def new_state(n_hosts, cap):
    """CoDelQueue::new per host, in oracle.codel_state's layout."""
    return dict(cap=cap, flags=np.zeros(n_hosts, np.uint8), interval_end=np.zeros(n_hosts, np.uint64),
                drop_next=np.zeros(n_hosts, np.uint64), cur=np.zeros(n_hosts, np.uint64),
                prev=np.zeros(n_hosts, np.uint64), bytes=np.zeros(n_hosts, np.uint64),
                head=np.zeros(n_hosts, np.uint32), tail=np.zeros(n_hosts, np.uint32),
                ring_pkt=np.zeros(n_hosts * cap, np.uint32), ring_ts=np.zeros(n_hosts * cap, np.uint64),
                ring_len=np.zeros(n_hosts * cap, np.uint32))


def copy_state(st):
    return {k: (v if k == "cap" else v.copy()) for k, v in st.items()}


def run(state, host, kind, time, pkt, length, pkt_status, trace=None, variant=None):
    """oracle.codel_run on the model: events grouped by ascending host, each host's in order;
    state and pkt_status updated in place; returns pop_result (NONE for a push)."""
    host, kind, time = [np.asarray(a).tolist() for a in (host, kind, time)]
    pkt, length = np.asarray(pkt).tolist(), np.asarray(length).tolist()
    cap, n = state["cap"], len(host)
    res = np.full(n, NONE, np.uint32)
    status = {}
    e = 0
    while e < n:
        h = host[e]
        if e and h < host[e - 1]:
            raise ValueError("events not grouped by ascending host")
        q = Queue(cap, status, trace, variant)
        for k in SCALARS:
            setattr(q, k, int(state[k][h]))
        lo = h * cap
        q.pkt, q.ts, q.len = (state[k][lo:lo + cap] for k in ("ring_pkt", "ring_ts", "ring_len"))   # views
        while e < n and host[e] == h:
            if kind[e] == PUSH:
                q.push(pkt[e], length[e], time[e])
            else:
                res[e] = q.pop(time[e])
            e += 1
        if variant == "counters-not-modular":   # what a u32 store keeps of them
            q.head, q.tail = q.head % M32, q.tail % M32
        for k in SCALARS:
            state[k][h] = getattr(q, k)
    for p, s in status.items():   # a packet has one fate per call: later writes win as in the oracle's array
        if p >= len(pkt_status):
            raise ValueError("packet id >= n_packets")
        pkt_status[p] = s
    return res


def live_slots(st):
    """Indices into the ring arrays of every live slot, [head, tail) modulo 2^32 per host."""
    cap = st["cap"]
    lo = st["head"].astype(np.int64)
    n = (st["tail"].astype(np.int64) - lo) % M32
    assert (n <= cap).all()
    hh = np.repeat(np.arange(len(n)), n)
    c = lo[hh] + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    return hh * cap + (c % cap)
