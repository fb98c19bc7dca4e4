"""Inputs of the finite-buffer link-queue tests (test_queue_drop_ref_cpu.py qualifies them on the
CPU, test_queue_drop_gpu.py runs them).  A case is a queue_carry_cases.case dict plus limit_ns."""
import bisect

import numpy as np

import queue_carry_cases as CC
import queue_cases as QC
import queue_drop_ref as DR

MAX = DR.MAX
TILE = QC.TILE
SHORT = 32  # the longest busy period a lane of the library walks alone; a longer one takes a wave
WAVE = 64  # records per load of a wave's walk
PERIODS = (1, 2, SHORT - 1, SHORT, SHORT + 1, 63, 64, 65, 2 * WAVE + SHORT, 2047, 2048, 2049, 3 * 2048 + 1)
LIMITS = (0, 5, 20, 60, 200, MAX)


def with_limits(c, limit_ns):
    nl = len(c["link_off"]) - 1
    lim = np.full(nl, int(limit_ns), np.uint64) if np.ndim(limit_ns) == 0 else np.asarray(limit_ns, np.uint64)
    assert lim.shape == (nl,)
    return dict(c, limit_ns=lim)


def draw_limits(c, seed, limits=LIMITS):
    nl = len(c["link_off"]) - 1
    return with_limits(c, np.random.default_rng(seed).choice(np.array(limits, np.uint64), nl))


def ref(c, **kw):
    """First order: queue_drop_ref.loop."""
    return DR.loop(c["link_off"], c["enter"], c["packet"], c["weight"], cost_ps=c["cost_ps"], limit_ns=c["limit_ns"],
                   free_in=c["free_in"], **kw)


def ref_carried(c, jacobi=False, **kw):
    f = DR.jacobi if jacobi else DR.event
    return f(c["link_off"], c["enter"], c["packet"], c["weight"], n_packets=c["n_packets"], cost_ps=c["cost_ps"],
             limit_ns=c["limit_ns"], free_in=c["free_in"], **kw)


def fast(c):
    """queue_drop_ref.loop's Result for a valid first-order case without overflow, `ahead` by
    bisection over the served done times (they never fall) instead of the direct count: the large
    cases' reference.  test_queue_drop_ref_cpu.py qualifies it against `loop`."""
    off = c["link_off"].astype(np.int64).tolist()
    nl, n = len(off) - 1, len(c["enter"])
    ent = c["enter"].tolist()
    if c["weight"] is None:
        w = np.ones(n, np.int64)
    else:
        w = c["weight"].astype(np.int64)[c["packet"].astype(np.int64)]
    per = np.repeat(c["cost_ps"].astype(np.int64), np.diff(off))
    assert n == 0 or (int(w.max()) < 1 << 31 and int(per.max()) < 1 << 31)
    s = (-((-w * per) // 1000)).tolist()
    wait, done, ahead = [MAX] * n, [0] * n, [0] * n
    link_free, busy, wmax, wsum, amax, drops, refused = ([0] * nl for _ in range(7))
    for lk in range(nl):
        d = 0 if c["free_in"] is None else int(c["free_in"][lk])
        lim = int(c["limit_ns"][lk])
        served = []
        for i in range(off[lk], off[lk + 1]):
            e = ent[i]
            a = len(served) - bisect.bisect_right(served, e)
            ahead[i] = a
            start = e if e > d else d
            if start - e > lim:
                done[i] = e
                drops[lk] += 1
                refused[lk] += s[i]
                continue
            d = start + s[i]
            assert d < MAX
            wait[i], done[i] = start - e, d
            served.append(d)
            busy[lk] += s[i]
            wsum[lk] += start - e
            if start - e > wmax[lk]:
                wmax[lk] = start - e
            if a > amax[lk]:
                amax[lk] = a
        link_free[lk] = d
    u = lambda x: np.array(x, np.uint64)  # noqa: E731
    return DR.Result(u(wait), u(done), np.array(ahead, np.uint32), u(link_free), u(busy), u(wmax), u(wsum),
                     np.array(amax, np.uint32), np.array(drops, np.uint32), u(refused))


def hand():
    """Three links at 1 ns a unit, four packets of weight 10 (a service of 10 ns everywhere), every
    buffer holds a wait of 5 ns:
         A = 0: link 0 at 102, link 1 at 107 (gap 5)
         B = 1: link 0 at 100, link 2 at 105 (gap 5)
         C = 2: link 1 at 126
         D = 3: link 2 at 118
    Link 0: B is served 100 .. 110; A would wait 8 and is dropped, so A is absent on link 1.
    Link 1: C (126) finds it idle and is served 126 .. 136.  Without limits A waits 8 on link 0,
    enters link 1 at 120 + 5 = 125, is served 125 .. 135, and C waits 9.
    Link 2: B enters at 110 + 5 = 115 and is served 115 .. 125; D (118) would wait 7 and is
    dropped.  The first-order flagged result takes link 2 at the input times, B 105 .. 115, and
    serves D at 118 without a wait (and serves A on link 1 at 107, though link 0 dropped it).
    Returns (case, Result, carried enter, the first-order flagged Result)."""
    c = CC.build(3, [[(0, 102), (1, 107)], [(0, 100), (2, 105)], [(1, 126)], [(2, 118)]], [10] * 4, [1000] * 3)
    assert c["packet"].tolist() == [1, 0, 0, 2, 1, 3] and c["enter"].tolist() == [100, 102, 107, 126, 105, 118]
    c = with_limits(c, 5)
    R, M = DR.Result, MAX
    want = R(wait=np.uint64([0, M, M, 0, 0, M]), done=np.uint64([110, 102, M, 136, 125, 118]),
             ahead=np.uint32([0, 1, 0, 0, 0, 1]), link_free=np.uint64([110, 136, 125]), busy=np.uint64([10, 10, 10]),
             wait_max=np.uint64([0, 0, 0]), wait_sum=np.uint64([0, 0, 0]), ahead_max=np.uint32([0, 0, 0]),
             drops=np.uint32([1, 0, 1]), refused=np.uint64([10, 0, 10]))
    first = R(wait=np.uint64([0, M, 0, 0, 0, 0]), done=np.uint64([110, 102, 117, 136, 115, 128]),
              ahead=np.uint32([0, 1, 0, 0, 0, 0]), link_free=np.uint64([110, 136, 128]), busy=np.uint64([10, 20, 20]),
              wait_max=np.uint64([0, 0, 0]), wait_sum=np.uint64([0, 0, 0]), ahead_max=np.uint32([0, 0, 0]),
              drops=np.uint32([1, 0, 0]), refused=np.uint64([10, 0, 0]))
    return c, want, np.uint64([100, 102, M, 126, 115, 118]), first


def periods(segments, seed, limit_ns=60, *, free=None, touch=False):
    """A first-order case whose busy periods under the UNLIMITED queue are exactly the given ones:
    segments[L] lists link L's period lengths (an empty list: an empty link).  Services are 10 ..
    30 ns (weights through a shuffled packet index at 1 ns a unit); inside a period arrivals rise
    by 0 .. 9 ns, so every record but the first finds the unlimited server busy; a period starts 0
    .. 5 ns after the unlimited server has drained (touch: exactly when it has).  A queue builds by
    about 15 ns a record, so a limit of 60 drops from the fifth record or so on and then serves
    and drops in turn.  free: free_in drawn within `free` ns of a segment's first arrival."""
    rng = np.random.default_rng(seed)
    lens = [np.asarray(p, np.int64) for p in segments]
    seg_len = np.array([int(p.sum()) for p in lens], np.int64)
    off = np.concatenate([[0], np.cumsum(seg_len)])
    n = int(off[-1])
    plen = np.concatenate(lens) if n else np.zeros(0, np.int64)
    pstart = np.concatenate([[0], np.cumsum(plen)])[:-1]
    per_of = np.repeat(np.arange(len(plen)), plen)
    weight = rng.integers(10, 31, n + 5)
    packet = rng.permutation(n + 5)[:n]
    s = weight[packet].astype(np.int64)
    step = rng.integers(0, 10, n)
    step[pstart] = 0
    rise = np.cumsum(step)
    rise -= rise[pstart][per_of] if n else 0
    total = np.add.reduceat(s, pstart) if n else np.zeros(0, np.int64)  # a period's unlimited busy time
    gap = np.zeros(len(plen), np.int64) if touch else rng.integers(0, 6, len(plen))
    # a period's start: 1000 for a segment's first, else the one before's start + its busy time + the gap
    seg_of_per = np.repeat(np.arange(len(lens)), [len(p) for p in lens])
    t0 = np.zeros(len(plen), np.int64)
    prev_seg, t = -1, 0
    for p in range(len(plen)):
        t = 1000 if seg_of_per[p] != prev_seg else t + int(total[p - 1]) + int(gap[p])
        t0[p], prev_seg = t, seg_of_per[p]
    enter = (t0[per_of] + rise).astype(np.uint64) if n else np.zeros(0, np.uint64)
    free_in = None
    if free:
        free_in = np.uint64(1000 - free) + rng.integers(0, 2 * free, len(lens)).astype(np.uint64)
    c = QC.case(off, enter, packet, weight, np.full(len(lens), 1000), free_in)
    c["n_packets"] = len(weight)
    return with_limits(c, limit_ns)


def period_heads(c):
    """The unlimited queue's busy-period heads of a first-order case (queue_ref.loop): a segment's
    first record, or a wait of 0."""
    rc, _, res = QC.ref(c)
    assert rc == DR.OK
    head = res.wait == 0
    off = c["link_off"].astype(np.int64)
    head[off[:-1][off[1:] > off[:-1]]] = True
    return head


def packed_periods():
    """Every length of PERIODS as a link's only period, an empty link between every two."""
    out = [[]]
    for n in PERIODS:
        out += [[n], []]
    return out


def shifted_periods(shift):
    """One link: `shift` one-record periods, then every length of PERIODS, so each meets the tile
    edges `shift` records later."""
    return [[1] * shift + list(PERIODS)]


def edge_periods():
    """Periods that end exactly on a tile edge and start there, across two links."""
    return [[TILE - 40, 40, TILE], [5, TILE - 5, 1, TILE - 1, 3]]


def mixed_periods(n, seed):
    """One segment of n records: period lengths drawn from 1 .. 3 (most), to 100, to 5,000."""
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left:
        kind = rng.random()
        k = int(rng.integers(1, 4) if kind < 0.6 else rng.integers(4, 101) if kind < 0.95 else rng.integers(101, 5001))
        k = min(k, left)
        out.append(k)
        left -= k
    return [out]
