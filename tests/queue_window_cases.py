"""Inputs of the windowed link-queue tests (test_queue_window_ref_cpu.py qualifies them on the CPU,
test_queue_window_gpu.py runs them), on queue_carry_cases and outcomes_cases.  A case is an
outcomes_cases case: a queue_carry_cases.case dict with limit_ns and base."""
import numpy as np

import outcomes_cases as OC
import queue_carry_cases as CC
import queue_drop_cases as DC
import queue_window_ref as WR

MAX = WR.MAX
MODES = ((False, False), (False, True), (True, False), (True, True))  # (drop, packets)
MODE_IDS = ("plain", "packets", "drop", "drop-packets")


def closed_enter(c, drop):
    """The closed solution's carried enter times (2^64 - 1: absent)."""
    rc, _, _, cur, _ = WR._closed(c, drop)
    assert rc == WR.OK
    return cur


def horizons(c, drop):
    """Below every record, equal to a record's carried time (strict: that record is pending), between
    two records, above every record, and 2^64 - 1."""
    t = np.unique(closed_enter(c, drop))
    t = [int(x) for x in t.tolist() if int(x) != MAX]
    mid = t[len(t) // 2]
    between = next((a + 1 for a, b in zip(t, t[1:]) if b - a > 1 and a >= mid), t[-1] + 1)
    return [t[0], mid, between, t[-1] + 1, MAX]


def hand():
    return OC.with_base(CC.hand()[0], 1000)


def staircase(k):
    return OC.with_base(CC.staircase(k), 1000)


def pushed_past():
    """Packet 1 enters link 0 at 105, below H = 110, behind packet 0 (served 100 .. 120): it waits and
    enters link 1 at 135 instead of 110.  Packet 2 enters link 1 at 108."""
    c = CC.build(2, [[(0, 100)], [(0, 101), (1, 106)], [(1, 108)]], [20, 5, 5], [1000] * 2)
    return OC.with_base(c, 500)


def drop_cases():
    """(case, H, what it is).  Packet 0 holds link 0 until 200; packet 1 finds no buffer there at
    110 and is dropped, its later hops (links 1, 2 at 130, 150) are absent; packet 2 crosses link 1."""
    c = CC.build(3, [[(0, 100)], [(0, 110), (1, 130), (2, 150)], [(1, 120), (2, 170)]], [100, 10, 10], [1000] * 3)
    c = OC.with_base(DC.with_limits(c, [0, MAX, MAX]), 900)
    return [(c, 125, "a settled drop, its later hops beyond H: absent, not pending"),
            (c, 105, "a drop beyond H: it and its later hops are pending"),
            (c, 111, "the drop just settled"), (c, 160, "H cuts packet 2")]


def segments(length, seed=31):
    """A link of `length` records among three others, chains of one to three records, and the
    horizon that leaves about half of every link active."""
    c = OC.with_base(DC.draw_limits(CC.from_lengths([length, 70, 3, 0], seed), seed + 1))
    return c


def rounds(c, k, seed):
    """The case cut into k rounds by the packets' first enter time at k - 1 random horizons; the
    last horizon is 2^64 - 1.  Returns (the case with its packets renumbered in (round, packet)
    order, [(the round's case, H, the original index of each of its records, of each packet)])."""
    rng = np.random.default_rng(seed)
    n, P = len(c["enter"]), c["n_packets"]
    ent = c["enter"].astype(np.int64) if n else np.zeros(0, np.int64)
    first = np.full(P, np.iinfo(np.int64).max)
    np.minimum.at(first, c["packet"].astype(np.int64), ent)
    lo, hi = (int(ent.min()), int(ent.max()) + 2) if n else (0, 2)
    cuts = sorted(int(x) for x in rng.integers(lo, hi, k - 1)) + [MAX]
    rnd = np.searchsorted(np.array(cuts[:-1], np.int64), np.where(first == np.iinfo(np.int64).max, lo, first), side="right")
    order = np.lexsort((np.arange(P), rnd))  # new number -> old packet
    renum = np.empty(P, np.int64)
    renum[order] = np.arange(P)
    whole = dict(c, packet=renum[c["packet"].astype(np.int64)].astype(np.uint32), weight=c["weight"][order], base=c["base"][order])
    link = np.repeat(np.arange(len(c["link_off"]) - 1), np.diff(c["link_off"].astype(np.int64)))
    out = []
    for r in range(k):
        pk = np.flatnonzero(rnd == r)  # (old numbers, ascending: the round's own order)
        local = np.full(P, -1, np.int64)
        local[pk] = np.arange(len(pk))
        idx = np.flatnonzero(local[c["packet"].astype(np.int64)] >= 0) if n else np.zeros(0, np.int64)
        rc = dict(link_off=np.searchsorted(link[idx], np.arange(len(c["link_off"]))).astype(np.uint64), enter=c["enter"][idx],
                  packet=local[c["packet"][idx].astype(np.int64)].astype(np.uint32), weight=c["weight"][pk], base=c["base"][pk],
                  n_packets=len(pk))
        out.append((rc, cuts[r], idx, renum[pk]))
    return whole, out


def run_session(c, k, seed, drop, solve=None):
    """A SessionRef over the case's k rounds and a flush: every settled record and packet at the
    whole case's indices: (wait, done per record; delay, arrive, lost, drop link per packet)."""
    whole, rs = rounds(c, k, seed)
    nl = len(c["link_off"]) - 1
    s = WR.SessionRef(nl, c["cost_ps"], c["limit_ns"] if drop else None, c["free_in"], solve)
    n, P = len(c["enter"]), c["n_packets"]
    wait, done = np.full(n, 7, np.uint64), np.full(n, 7, np.uint64)
    delay, arrive = np.full(P, 7, np.uint64), np.full(P, 7, np.uint64)
    lost, dlink = np.zeros(P, bool), np.full(P, -1, np.int64)
    seen_r, seen_p = np.zeros(n, int), np.zeros(P, int)
    for step in [(rc, H) for rc, H, _, _ in rs] + [(None, MAX)]:
        records, packets = s.advance(*step)
        for r, i, w, d in records:
            at = rs[r][2][i]
            wait[at], done[at] = w, d
            seen_r[at] += 1
        for r, p, dl, ar, lk, ls in packets:
            at = rs[r][3][p]
            delay[at], arrive[at], lost[at] = dl, ar, ls
            dlink[at] = -1 if lk is None else lk
            seen_p[at] += 1
    assert (seen_r == 1).all() and (seen_p == 1).all() and not s.rec and not s.pkt
    return whole, dict(wait=wait, done=done, delay=delay, arrive=arrive, lost=lost, drop_link=dlink, link_free=s.free, sums=s.sums)


def session_want(whole, drop):
    """What one carried call over the whole case gives, in run_session's form."""
    rc, out = WR.define(whole, MAX, drop, True)
    assert rc == WR.OK
    n, nl = len(whole["enter"]), len(whole["link_off"]) - 1
    where = out["ahead"][n:]
    lost = where < np.uint32(WR.IN_FLIGHT)
    link = np.repeat(np.arange(nl), np.diff(whole["link_off"].astype(np.int64)))
    dlink = np.full(len(where), -1, np.int64)
    dlink[lost] = link[where[lost].astype(np.int64)]
    sums = dict(busy=out["busy"][:nl], wait_sum=out["wait_sum"], wait_max=out["wait_max"],
                drops=out["ahead_max"][nl:].astype(np.uint64) if drop else np.zeros(nl, np.uint64))
    return dict(wait=out["wait"][:n], done=out["done"][:n], delay=out["wait"][n:], arrive=out["done"][n:], lost=lost,
                drop_link=dlink, link_free=out["link_free"], sums=sums)
