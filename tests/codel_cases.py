"""Boundary cases of the routers' CoDel queue (router/codel_queue.rs; the model is codel_ref.py):
every decision of the state machine at -1, 0 and +1 of its unit, the rest of the decision held
on the side that lets the threshold decide.  One case is one host: a pre-state (scalars and ring
elements), at most ~40 events, a name.  test_codel_ref_cpu.py proves the cases against the model,
the oracle and the model's mutations; test_codel_gpu.py runs them through k_codel, one lane each.

Families (the case's name starts with it): target, mtu, interval, entry (drop_from_store_mode),
drop (drop_from_drop_mode), law (apply_control_law's counts), ring (the u32 counters and the
ring's end), and twin/<family>: the same boundary reached from CoDelQueue::new by pushes and pops
alone, so that nothing rests on set_state.

Boundaries without an events-only twin, and why a consistent queue cannot stand there:
* cur < prev, delta = 1000, the control-law counts past a few dozen: counts only grow by drops
  (a thousand events); cur < prev never (prev = cur at every entry, cur only grows after it).
* drop_next unset with its field holding junk, drop mode without drop_next: drop_next is set
  when drop mode is first entered and never unset.
* drop_next in the future at a store-mode entry: a re-entry comes a full INTERVAL after a bad
  pop that follows the leaving pop, and drop_next is at most one INTERVAL past the pop before it.
* a head younger than the element behind it: pushes are in time order in a consistent queue.
* inflated / deflated byte counts (the store-mode entry and the drop loop finding the queue
  empty): the last element always leaves 0 <= MTU bytes, so its pop is "good" before the queue
  can run out under a drop.
* a pop on an empty queue with drop mode or the interval still set: the pop that empties a
  queue leaves 0 bytes, which is "good" and clears both.
* head / tail at 2^32: four billion pushes.
* times at EMU_MAX.
Reachable but left without a twin: multi-drop pops starting from cur = 2 and 7 (the twins start
from the cur = 1 of a first entry).

Forms (materialise): a case's elements are in the ring before the call ("ring": set through the
state, or for a twin pushed by an earlier call), pushed by the same call that pops them ("window":
the kernel reads them from its staged LDS window), or half and half ("mixed": a multi-drop pop
crosses from ring elements to window elements).
"""
import numpy as np

import codel_ref as ref

T0 = 946684800 * 10**9
T, I, MTU = ref.TARGET, ref.INTERVAL, ref.MTU
F_DROP, F_IEND, F_DNEXT = ref.F_DROP, ref.F_IEND, ref.F_DNEXT
N = T0 + 5 * 10**9     # the cases' "now"
OLD = N - 5 * T        # enqueue time of an element standing well past TARGET
L = 1000               # two such packets behind a pop are more than an MTU
FORMS = ("ring", "window", "mixed")

LAW_COUNTS = tuple(range(1, 65)) + (
    2**18 - 1, 2**18, 2**18 + 1, 6_553_600, (512 * 25)**2, 2**24 + 1, 2**32 - 1, 2**32, 2**32 + 1, 2**53 - 1, 2**53,
    2**53 + 1, 4 * 10**16, 4 * 10**16 + 2**40, 2**63)
# the counts whose quotient INTERVAL / sqrt(count) is an exact tie (test_codel_ref_cpu asserts it)
LAW_TIES = (2**18, 6_553_600, (512 * 25)**2, 4 * 10**16)

CASES = []


def old(n, ln=L, ts=OLD):
    return [(ts, ln)] * n


def pop(t):
    return (ref.POP, t, 0)


def push(t, ln=L):
    return (ref.PUSH, t, ln)


def case(name, events, ring=(), extra=0, cap=64, head=0, expect=None, **scalars):
    """ring: (enqueue time, length) per element, head first; extra: bytes beyond (or, negative,
    short of) what the ring holds; scalars: flags, interval_end, drop_next, cur, prev.  A twin
    has no pre-state: its leading pushes are its elements."""
    assert not set(scalars) - {"flags", "interval_end", "drop_next", "cur", "prev"}
    assert all(c["name"] != name for c in CASES), name
    ring, events = list(ring), list(events)
    twin = name.startswith("twin/")
    if twin:
        assert not ring and not scalars and not extra and not head
        while events and events[0][0] == ref.PUSH:
            ring.append((events[0][1], events[0][2]))
            events.pop(0)
    assert len(ring) <= cap and len(events) + len(ring) <= 48
    CASES.append(dict(name=name, family=name.split("/")[1 if twin else 0], twin=twin, ring=ring, events=events,
                      extra=extra, cap=cap, head=head, expect=expect or {}, scalars=scalars))


def law_steps(cur, k):
    """The k accumulated control-law steps a drop loop takes from drop count cur."""
    s, out = 0, []
    for j in range(1, k + 1):
        s += ref.law_increment(cur + j)
        out.append(s)
    return out


# ---- target -----------------------------------------------------------------------------------
for d in (-1, 0, 1):
    case(f"target/sd=T{d:+d}", [pop(N), pop(N + I)], ring=old(3, ts=N - (T + d)))
    case(f"target/sd=T{d:+d}/interval-due", [pop(N), pop(N)], ring=old(4, ts=N - (T + d)), flags=F_IEND,
         interval_end=N)
    case(f"twin/target/sd=T{d:+d}", [push(N - (T + d))] * 3 + [pop(N), pop(N + I)])
case("target/head=T+1,next=T-1", [pop(N), pop(N)], ring=[(N - (T + 1), L)] + old(3, ts=N - (T - 1)), flags=F_IEND,
     interval_end=N)
case("target/head=T-1,next=T+1", [pop(N), pop(N)], ring=[(N - (T - 1), L)] + old(3, ts=N - (T + 1)), flags=F_IEND,
     interval_end=N)
case("twin/target/head=T+1,next=T-1", [push(N - (T + 1))] + [push(N - (T - 1))] * 3 + [pop(N), pop(N + I)])

# ---- MTU --------------------------------------------------------------------------------------
for r in (MTU - 1, MTU, MTU + 1):
    for x in (1, L):   # x = 1: the byte counts before and after the pop fall on opposite sides at r = MTU
        case(f"mtu/left={r}/popped={x}", [pop(N), pop(N)], ring=[(OLD, x), (OLD, 750), (OLD, r - 750)], flags=F_IEND,
             interval_end=N)
        case(f"mtu/left={r}/popped={x}/interval-starts", [pop(N)], ring=[(OLD, x), (OLD, 750), (OLD, r - 750)])
        case(f"twin/mtu/left={r}/popped={x}", [push(OLD, x), push(OLD, 750), push(OLD, r - 750), pop(N)])
case("mtu/bytes-below-ring", [pop(N), pop(N), pop(N)], ring=old(3), extra=-1500, flags=F_IEND, interval_end=N)

# ---- interval ---------------------------------------------------------------------------------
for d in (-1, 0, 1):
    case(f"interval/now=iend{d:+d}", [pop(N), pop(N)], ring=old(4), flags=F_IEND, interval_end=N - d)
    case(f"twin/interval/now=iend{d:+d}", [push(OLD)] * 6 + [pop(OLD + T), pop(OLD + T + I + d), pop(OLD + T + I + d)])
# bad (interval_end = OLD + T + I), good (one MTU left), bad again past the first interval_end:
# the interval restarts, nothing drops
case("twin/interval/bad-good-bad",
     [push(OLD)] * 3 + [pop(OLD + T), pop(OLD + T + 1)] + [push(OLD + T + 2)] * 2 + [pop(OLD + T + I + 5),
                                                                                      pop(OLD + T + I + 6)])
case("interval/empty-pop-clears", [pop(N)], flags=F_IEND | F_DROP | F_DNEXT, interval_end=N - 1, drop_next=N - 1, cur=3,
     prev=2)
case("interval/empty-pop-then-traffic", [pop(N)] + [push(N)] * 4 + [pop(N + T + 1), pop(N + T + 2)],
     flags=F_IEND | F_DROP | F_DNEXT, interval_end=N - 1, drop_next=N - 1, cur=3, prev=2)
_end = ref.EMU_MAX - 10   # the interval's end saturates at EMU_MAX; no pop can reach it
case("interval/end-saturates", [pop(_end), pop(_end + 5)], ring=old(4, ts=_end - 2 * T))

# ---- entering drop mode -----------------------------------------------------------------------
_due = dict(flags=F_IEND, interval_end=N)
for n in (1, 2, 3):   # packets behind the dropped one (1,600 B each: one alone is more than an MTU)
    case(f"entry/behind={n}", [pop(N), pop(N + 1)], ring=old(1) + old(n, 1600), **_due)
    case(f"twin/entry/behind={n}", [push(OLD)] * 2 + [push(OLD, 1600)] * n + [pop(OLD + T), pop(OLD + T + I),
                                                                               pop(OLD + T + I + 1)])
case("entry/second-below-target", [pop(N), pop(N + 1)], ring=old(1) + old(3, ts=N - (T - 1)), **_due)
case("entry/second-below-target/alone", [pop(N)], ring=old(1) + old(3, ts=N - (T - 1)), **_due)
case("entry/second-above-target", [pop(N), pop(N + 1)], ring=old(4), **_due)
for r in (MTU, MTU + 1):
    case(f"entry/second-leaves={r}", [pop(N), pop(N + 1)], ring=[(OLD, L), (OLD, 1600), (OLD, r)], **_due)
for r in (MTU, MTU + 1):
    case(f"twin/entry/second-leaves={r}", [push(OLD)] * 2 + [push(OLD, 1600), push(OLD, r), pop(OLD + T),
                                                            pop(OLD + T + I), pop(OLD + T + I + 1)])
case("twin/entry/second-below-target",
     [push(OLD)] * 3 + [pop(OLD + T)] + [push(OLD + I + 1)] * 3 + [pop(OLD + T + I), pop(OLD + T + I + 1)])
# the byte count says more than the ring holds: the entry's second codel_pop finds the queue
# empty; the pop returns none and drop mode stays set
case("entry/queue-empty-after-drop", [pop(N), push(N + 1), pop(N + 2)], ring=old(1), extra=5000, **_due)
_deltas = {"0": (5, 5), "1": (6, 5), "2": (7, 5), "3": (8, 5), "1000": (1005, 5), "cur<prev": (3, 5)}
_dnexts = {"unset-junk": (0, N - 1), "future": (F_DNEXT, N + 5), "16I-1": (F_DNEXT, N - (16 * I - 1)),
           "16I": (F_DNEXT, N - 16 * I), "16I+1": (F_DNEXT, N - (16 * I + 1))}
for dk, (cur, prev) in _deltas.items():
    for nk, (fl, dn) in _dnexts.items():
        case(f"entry/delta={dk}/dnext={nk}", [pop(N), pop(N + 1)], ring=old(5), flags=F_IEND | fl, interval_end=N,
             drop_next=dn, cur=cur, prev=prev)


def _twin_reentry(name, m, off):
    """From new: enter drop mode at E (cur = prev = 1, drop_next = E + I), m more drops in one
    pop of the drop loop (cur = 1 + m), leave through a pop that leaves one MTU, stand bad again
    for an interval and re-enter at drop_next + off with delta = m."""
    n = 5 + m + (1 if m else 0)
    E = OLD + T + I
    ev = [push(OLD)] * n + [pop(OLD + T), pop(E)]
    dn, last = E + I, E
    if m:
        steps = law_steps(1, m)
        last = dn + (steps[-2] if m > 1 else 0)
        ev.append(pop(last))
        dn += steps[-1]
    ev.append(pop(last))      # leaves 1,000 B behind: good, Store mode
    R = dn + off              # the re-entry
    assert R - I - T > last
    ev += [push(R - I - T)] * 4 + [pop(R - I), pop(R), pop(R + 1)]
    case(name, ev, expect=dict(drops=2 + m))


for m in (0, 1, 2, 3):
    _twin_reentry(f"twin/entry/delta={m}/recent", m, 8 * I)
for d in (-1, 0, 1):
    _twin_reentry(f"twin/entry/delta=2/dnext=16I{d:+d}", 2, 16 * I + d)
_twin_reentry("twin/entry/delta=2/now=dnext+3I", 2, 3 * I)

# ---- drop mode --------------------------------------------------------------------------------
_drop = dict(flags=F_DROP | F_IEND | F_DNEXT, interval_end=N - 10 * I)
for d in (-1, 0, 1):
    case(f"drop/now=dnext{d:+d}", [pop(N), pop(N)], ring=old(5), drop_next=N - d, cur=3, prev=3, **_drop)
    case(f"twin/drop/now=dnext{d:+d}", [push(OLD)] * 8 + [pop(OLD + T), pop(OLD + T + I), pop(OLD + T + 2 * I + d),
                                                         pop(OLD + T + 2 * I + d)], expect=dict(drops=1 + (d >= 0)))
for c in (1, 2, 7):
    for k in (1, 2, 3, 5, 12):
        st = [0] + law_steps(c, k)
        # on the step that makes the k-th drop due, one ns before it, and one ns before the next
        for where, t, drops in (("on", st[k - 1], k), ("before", st[k - 1] - 1, k - 1), ("last", st[k] - 1, k)):
            case(f"drop/cur={c}/k={k}/{where}", [pop(N + t), pop(N + t)], ring=old(k + 4), drop_next=N, cur=c, prev=c,
                 expect=dict(drops=drops), **_drop)
for k in (1, 2, 3, 5, 12):   # from new: cur = 1 and drop_next = E + I after the entry at E
    st = [0] + law_steps(1, k)
    for where, t, drops in (("on", st[k - 1], k), ("before", st[k - 1] - 1, k - 1)):
        E = OLD + T + I
        case(f"twin/drop/cur=1/k={k}/{where}", [push(OLD)] * (k + 7) + [pop(OLD + T), pop(E), pop(E + I + t),
                                                                       pop(E + I + t)], expect=dict(drops=1 + drops))
_far = N + 100 * I
case("drop/ends-queue-empty", [pop(_far), pop(_far)], ring=old(3), extra=5000, drop_next=N, cur=2, prev=2,
     expect=dict(drops=3), **_drop)
case("drop/ends-at-mtu", [pop(_far), pop(_far)], ring=old(4), drop_next=N, cur=2, prev=2, expect=dict(drops=2), **_drop)
case("drop/ends-at-younger", [pop(N), pop(N)], ring=old(2) + [(N - 1, L)] + old(3, ts=N - 1), drop_next=N - 10 * I, cur=5,
     prev=5, expect=dict(drops=2), **_drop)
case("twin/drop/ends-at-mtu", [push(OLD)] * 6 + [pop(OLD + T), pop(OLD + T + I), pop(_far), pop(_far)],
     expect=dict(drops=2))
case("twin/drop/ends-at-younger", [push(OLD)] * 5 + [pop(OLD + T), pop(OLD + T + I)] + [push(_far - 1)] * 3 +
     [pop(_far), pop(_far)], expect=dict(drops=3))
case("drop/dnext-unset", [pop(N), pop(N)], ring=old(4), flags=F_DROP | F_IEND, interval_end=N - 1, drop_next=N - 1, cur=2,
     prev=2, expect=dict(drops=0))
case("drop/law-saturates", [pop(_end + 9)], ring=old(5, ts=_end - 5 * T), flags=F_DROP | F_IEND | F_DNEXT,
     interval_end=_end, drop_next=_end + 5, cur=2, prev=2, expect=dict(drops=1))

# ---- control law ------------------------------------------------------------------------------
for c in LAW_COUNTS:
    case(f"law/count={c}/entry", [pop(N)], ring=old(4), flags=F_IEND | F_DNEXT, interval_end=N, drop_next=N - 1, cur=c,
         prev=0)
    case(f"law/count={c}/loop", [pop(N)], ring=old(6), drop_next=N, cur=c - 1, prev=c - 1, **_drop)

# the drop count wraps at 2^64 as the reference's release build does: the law's count-0 arm
case("law/count=0/loop-wraps", [pop(N)], ring=old(6), drop_next=N, cur=2**64 - 1, prev=2**64 - 1, **_drop)

# ---- ring counters ----------------------------------------------------------------------------
for cap in (4, 64):
    for h in (2**32 - 2, 2**32 - 1, cap - 1, 2**31 + cap - 2):
        case(f"ring/cap={cap}/head={h}/fifo", [pop(N)] * 4, ring=old(3, ts=N - 1), cap=cap, head=h)
        case(f"ring/cap={cap}/head={h}/drops", [pop(_far), pop(_far)], ring=old(4), cap=cap, head=h, drop_next=N, cur=2,
             prev=2, expect=dict(drops=2), **_drop)
        case(f"ring/cap={cap}/head=tail={h}/push-pop", [push(N), push(N), pop(N + 1), push(N + 1), pop(N + 2),
                                                       pop(N + 2), pop(N + 2)], cap=cap, head=h)

NAMES = tuple(c["name"] for c in CASES)
BY_NAME = {c["name"]: c for c in CASES}


def of_cap(cap):
    return [c for c in CASES if c["cap"] == cap]


def has_form(c, form):
    n = len(c["ring"])
    if form == "ring":
        return True
    if c["extra"] < 0:   # the window's pushes cannot start below zero bytes
        return False
    return n >= 1 if form == "window" else n >= 2


def materialise(c, form):
    """(scalars incl. bytes / head / tail, ring elements [(pkt, ts, len)], [call 0, call 1]) with
    events (kind, time, pkt, len) and packet ids local to the case (elements first)."""
    assert has_form(c, form)
    n = len(c["ring"])
    m = n if form == "ring" else 0 if form == "window" else (n + 1) // 2
    el = [(i, ts, ln) for i, (ts, ln) in enumerate(c["ring"])]
    pushes = [(ref.PUSH, ts, i, ln) for i, ts, ln in el]
    ev, p = [], n
    for kind, t, ln in c["events"]:
        ev.append((kind, t, p if kind == ref.PUSH else 0, ln))
        p += kind == ref.PUSH
    sc = dict(flags=0, interval_end=0, drop_next=0, cur=0, prev=0)
    sc.update(c["scalars"])
    if c["twin"]:
        sc.update(bytes=0, head=0, tail=0)
        return sc, [], [pushes[:m], pushes[m:] + ev], p
    sc.update(bytes=sum(e[2] for e in el[:m]) + c["extra"], head=c["head"], tail=(c["head"] + m) % ref.M32)
    return sc, el[:m], [[], pushes[m:] + ev], p


def build(cases, form, cap, hosts=None, n_hosts=None, pkt0=0):
    """The cases as one batch: a state in oracle.codel_state's layout (host i holds cases[i], or
    hosts[i] of n_hosts), the two calls' event columns (host, kind, time, pkt, len; grouped by
    ascending host) and each case's first packet id (the last entry: the next free id)."""
    hosts = list(range(len(cases))) if hosts is None else [int(h) for h in hosts]
    forms = [form] * len(cases) if isinstance(form, str) else list(form)   # one form, or one per case
    st = ref.new_state(n_hosts or len(cases), cap)
    rows, base = ([], []), {}
    for h, c, f in sorted(zip(hosts, cases, forms), key=lambda x: x[0]):
        assert c["cap"] == cap
        sc, el, calls, npk = materialise(c, f)
        for k, v in sc.items():
            st[k][h] = v
        for j, (p, ts, ln) in enumerate(el):
            s = h * cap + (sc["head"] + j) % cap
            st["ring_pkt"][s], st["ring_ts"][s], st["ring_len"][s] = pkt0 + p, ts, ln
        for i in (0, 1):
            rows[i].extend((h, k, t, pkt0 + p if k == ref.PUSH else 0, ln) for k, t, p, ln in calls[i])
        base[h] = pkt0
        pkt0 += npk
    return st, [columns(r) for r in rows], [base[h] for h in hosts] + [pkt0]


def columns(rows):
    a = list(zip(*rows)) if rows else [[]] * 5
    return (np.array(a[0], np.uint32), np.array(a[1], np.uint8), np.array(a[2], np.uint64), np.array(a[3], np.uint32),
            np.array(a[4], np.uint32))


# ---- the random streams of test_codel_gpu.py (drawn here so that the CPU tests can run them) ----
MS = 10**6


def host_times(host, gaps, t0):
    """Per host (host sorted): t0 + the running sum of its own gaps (a segmented cumsum)."""
    c = np.cumsum(gaps.astype(np.int64))
    first = np.r_[True, host[1:] != host[:-1]]
    base = np.maximum.accumulate(np.where(first, c - gaps, 0))
    return (t0 + c - base).astype(np.uint64)


def stream(rng, H, E, t0, gap_ms, p_pop, n_pkt0=0):
    host = np.sort(rng.integers(0, H, E)).astype(np.uint32)
    kind = (rng.random(E) < p_pop).astype(np.uint8)
    t = host_times(host, rng.integers(0, gap_ms * MS, E), t0)
    pkt = (n_pkt0 + np.arange(E)).astype(np.uint32)
    ln = rng.integers(40, 1500, E).astype(np.uint32)
    return host, kind, t, pkt, ln
