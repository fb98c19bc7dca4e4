"""Inputs of the carried link-queue tests (test_queue_carry_ref_cpu.py qualifies them on the CPU,
test_queue_carry_gpu.py runs them): chains of records built by hand, and the real traces' costs.

A case is a queue_cases.case dict plus n_packets (the library's n_weights: len(weight) when there
are weights).  `build` takes chains -- a packet's (link, enter) pairs -- and lays the records out
as a link trace does: by link, ascending (enter, packet) inside a link."""
import numpy as np

import queue_carry_ref as CR
import queue_cases as QC

# The flag's name, in two parts: test_knobs_cpu.py takes every SG_LINK_* name written out in a file
# under tests/ for an environment knob of sg_knobs.h, and this one is a flag bit of the C ABI.
CARRY_FLAG = "SG_LINK_" + "QUEUE_CARRY"
PIECE = 2048  # records of one piece of the library's LDS sort, and of one tile of its scan
# link segments that cross every sort tier (1 .. 64 a wave, up to 2,048 one piece, past it the
# merge) and the scan's tile edges
SEGMENTS = (0, 1, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1)
STAIRS = (3, 6, 12)
# the real traces: the tie round under queue_cases.TIE_COST, and six sweep graphs under
# queue_cases.sweep_costs (test_queue_carry_ref_cpu.py asserts conditions() on each: of the 40
# graphs the 14 with at most 9 links give one-record chains, and two more settle in 2 iterations;
# these six take 5, 7, 9, 8, 32 and 10)
SWEEP_NAMES = ("k04", "k07", "k09", "k17", "k30", "k34")


def case(link_off, enter, packet, weight=None, cost_ps=None, free_in=None, n_packets=None):
    c = QC.case(link_off, enter, packet, weight, cost_ps, free_in)
    c["n_packets"] = len(c["weight"]) if weight is not None else int(n_packets)
    return c


def build(n_links, chains, weight=None, cost_ps=None, free_in=None, n_packets=None):
    """chains[p]: packet p's [(link, enter), ...]."""
    recs = sorted((lk, t, p) for p, ch in enumerate(chains) for lk, t in ch)
    off = np.searchsorted(np.array([r[0] for r in recs], np.int64), np.arange(n_links + 1))
    return case(off, [r[1] for r in recs], [r[2] for r in recs], weight, cost_ps, free_in,
                n_packets=len(chains) if n_packets is None else n_packets)


def ref(c, jacobi=False, **kw):
    f = CR.jacobi if jacobi else CR.event
    return f(c["link_off"], c["enter"], c["packet"], c["weight"], n_packets=c["n_packets"], cost_ps=c["cost_ps"],
             free_in=c["free_in"], **kw)


def first_order(c):
    return QC.ref(c)


def shuffled(c, seed):
    """The case with every link's records in a random order, and the permutation: record j of the
    result is record perm[j] of c."""
    rng = np.random.default_rng(seed)
    off = c["link_off"].astype(np.int64)
    perm = np.concatenate([off[k] + rng.permutation(off[k + 1] - off[k]) for k in range(len(off) - 1)] or [np.zeros(0, np.int64)])
    return dict(c, enter=c["enter"][perm], packet=c["packet"][perm]), perm


def hand():
    """Three links at 1 ns a unit, three packets of weight 10 (a service of 10 ns everywhere):
         A = 0: link 0 at 101, link 1 at 106 (gap 5)
         B = 1: link 0 at 100, link 2 at 107 (gap 7)
         C = 2: link 2 at 100, link 1 at 108 (gap 8)
    Link 0: B is served 100 .. 110, A waits 9 and is served 110 .. 120, so A enters link 1 at
    120 + 5 = 125.  Link 2: C is served 100 .. 110 and enters link 1 at 110 + 8 = 118; B enters at
    110 + 7 = 117 and is served 117 .. 127.  Link 1: C (118) is served ahead of A (125): C 118 ..
    128, A waits 3 and is served 128 .. 138.  The first-order result takes link 1 at the input
    times, A (106) ahead of C (108): A 106 .. 116, C waits 8 and is done at 126.
    Returns (case, Result, carried enter, the first-order Result)."""
    c = build(3, [[(0, 101), (1, 106)], [(0, 100), (2, 107)], [(2, 100), (1, 108)]], [10, 10, 10], [1000] * 3)
    assert c["packet"].tolist() == [1, 0, 0, 2, 2, 1] and c["enter"].tolist() == [100, 101, 106, 108, 100, 107]
    R = CR.Result
    want = R(wait=np.uint64([0, 9, 3, 0, 0, 0]), done=np.uint64([110, 120, 138, 128, 110, 127]),
             ahead=np.uint32([0, 1, 1, 0, 0, 0]), link_free=np.uint64([120, 138, 127]), busy=np.uint64([20, 20, 20]),
             wait_max=np.uint64([9, 3, 0]), wait_sum=np.uint64([9, 3, 0]), ahead_max=np.uint32([1, 1, 0]))
    first = R(wait=np.uint64([0, 9, 0, 8, 0, 3]), done=np.uint64([110, 120, 116, 126, 110, 120]),
              ahead=np.uint32([0, 1, 0, 1, 0, 1]), link_free=np.uint64([120, 126, 120]), busy=np.uint64([20, 20, 20]),
              wait_max=np.uint64([9, 8, 3]), wait_sum=np.uint64([9, 8, 3]), ahead_max=np.uint32([1, 1, 1]))
    return c, want, np.uint64([100, 101, 125, 118, 100, 117]), first


def staircase(k):
    """k packets, each on link j then link j + 1 five ns later, and a blocker (packet k) on link 0
    at time 0; services of 10 ns.  Packet 0 (link 0 at 1) waits for the blocker and reaches link 1
    at 25 instead of 6, just ahead of packet 1 (at 26), which therefore waits and reaches link 2
    late, just ahead of packet 2 (at 51), and so on: packet j's lateness is known only once packet
    j - 1's is, one iteration per step."""
    chains = [[(j, 1 + 25 * j), (j + 1, 6 + 25 * j)] for j in range(k)] + [[(0, 0)]]
    return build(k + 1, chains, [10] * (k + 1), [1000] * (k + 1))


def random_chains(seed, n_links=6, n_packets=40, hops=(1, 4), span=400, gap_max=30, wmax=40, costs=(0, 500, 1000, 2000),
                  free_max=0):
    """Packets on random routes of hops[0] .. hops[1] distinct links (a route never meets a link
    twice), entering within `span` ns, gaps of 1 .. gap_max ns."""
    rng = np.random.default_rng(seed)
    chains = []
    for _ in range(n_packets):
        h = int(rng.integers(hops[0], min(hops[1], n_links) + 1))
        links = rng.permutation(n_links)[:h]
        t = int(rng.integers(0, span + 1)) + np.concatenate([[0], np.cumsum(rng.integers(1, gap_max + 1, h - 1))])
        chains.append(list(zip(links.tolist(), t.tolist())))
    free = rng.integers(0, free_max + 1, n_links) if free_max else None
    return build(n_links, chains, rng.integers(0, wmax + 1, n_packets), rng.choice(np.asarray(costs), n_links), free)


def from_lengths(lengths, seed, hops=(1, 3), span=4000, gap_max=40, wmax=60, costs=(500, 1000, 1500), free_max=0):
    """Link L gets exactly lengths[L] records: the records' links are shuffled and cut into chains
    of hops[0] .. hops[1] records, a chain ending early where its next link is one it has."""
    rng = np.random.default_rng(seed)
    slots = rng.permutation(np.repeat(np.arange(len(lengths)), lengths)).tolist()
    chains, at = [], 0
    while at < len(slots):
        h = int(rng.integers(hops[0], hops[1] + 1))
        links = []
        while at < len(slots) and len(links) < h and slots[at] not in links:
            links.append(slots[at])
            at += 1
        t = int(rng.integers(0, span + 1)) + np.concatenate([[0], np.cumsum(rng.integers(1, gap_max + 1, len(links) - 1))])
        chains.append(list(zip(links, t.tolist())))
    free = rng.integers(0, free_max + 1, len(lengths)) if free_max else None
    c = build(len(lengths), chains, rng.integers(0, wmax + 1, len(chains)), rng.choice(np.asarray(costs), len(lengths)), free)
    assert np.array_equal(np.diff(c["link_off"].astype(np.int64)), np.asarray(lengths))
    return c


def long_chains(seed=21):
    """2,049 links.  Packet 0 crosses every one of them and packet 1 the first 65 (the packet sort's
    third and second tier); 300 packets of one to three records cross their paths."""
    rng = np.random.default_rng(seed)
    nl = PIECE + 1
    chains = [[(lk, 50 + 7 * lk) for lk in range(nl)], [(lk, 40 + 7 * lk) for lk in range(65)]]
    for _ in range(300):
        h = int(rng.integers(1, 4))
        lk0 = int(rng.integers(0, nl - 3))
        t0 = 7 * lk0 + int(rng.integers(0, 80))
        chains.append([(lk0 + d, t0 + 6 * d) for d in range(h)])
    return build(nl, chains, rng.integers(1, 30, len(chains)), np.full(nl, 1000))


def hot_link(seed=22, n=5000, feeders=50):
    """n packets, each over one of `feeders` slow links and then over one hot link: the feeders'
    queues reorder the hot link's 5,000 records from one iteration to the next."""
    rng = np.random.default_rng(seed)
    chains = []
    for p in range(n):
        t = int(rng.integers(0, 20000))
        chains.append([(1 + int(rng.integers(0, feeders)), t), (0, t + int(rng.integers(1, 50)))])
    cost = np.full(feeders + 1, 3000)
    cost[0] = 100
    return build(feeders + 1, chains, rng.integers(1, 60, n), cost)


def single_records(lengths, seed):
    """queue_cases.random_trace (a packet per record) with every segment in ascending (enter,
    packet) order, as a trace's are: the carried call must give the first-order result."""
    c = QC.random_trace(lengths, seed, free_max=100)
    link = np.repeat(np.arange(len(lengths)), lengths)
    order = np.lexsort((c["packet"], c["enter"], link))
    return dict(c, enter=c["enter"][order], packet=c["packet"][order], n_packets=len(c["weight"]))


def carry_overflow(slack):
    """One packet over link 0 (10 ns of service, free only at 2^64 - 16 - slack) and, 5 ns on, link
    1 (no service): it leaves link 0 at 2^64 - 6 - slack and enters link 1 at 2^64 - 1 - slack."""
    return build(2, [[(0, 100), (1, 105)]], [10], [1000, 0], np.uint64([CR.MAX - 15 - slack, 0]))


def conditions(c, cur, iters):
    """(some record's carried enter differs from the input's, some link's service order differs
    from the input order, at least 3 iterations)."""
    return (bool((cur != c["enter"]).any()), CR.order_changes(c["link_off"], c["enter"], cur, c["packet"]), iters >= 3)
