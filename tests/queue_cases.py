"""Inputs of the link-queue tests (test_queue_ref_cpu.py qualifies them on the CPU,
test_queue_gpu.py runs them): hand-made trace arrays, and the costs the real traces of
tests/trace_cases.py and tests/sweep_cases.py are queued under."""
import numpy as np

import queue_ref as QR

TILE = 2048  # records of one tile of the library's scan
SENT64 = np.uint64(0x5A5A5A5A5A5A5A5A)
SENT32 = np.uint32(0x5A5A5A5A)
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 1)
SECOND_TRIP = 1024 * TILE + 1  # one record past 1,024 tile aggregates
COSTS = (0, 80, 8000, 10**6)  # ps per byte: no time at all, 100 Gbit/s, 1 Gbit/s, 8 Mbit/s


def case(link_off, enter, packet=None, weight=None, cost_ps=None, free_in=None):
    nl = len(link_off) - 1
    return dict(link_off=np.asarray(link_off, np.uint64), enter=np.asarray(enter, np.uint64),
                packet=None if packet is None else np.asarray(packet, np.uint32),
                weight=None if weight is None else np.asarray(weight, np.uint32),
                cost_ps=np.full(nl, 1000, np.uint64) if cost_ps is None else np.asarray(cost_ps, np.uint64),
                free_in=None if free_in is None else np.asarray(free_in, np.uint64))


def ref(c, closed=False):
    f = QR.closed if closed else QR.loop
    return f(c["link_off"], c["enter"], c["packet"], c["weight"], cost_ps=c["cost_ps"], free_in=c["free_in"])


def hand():
    """Three links, every output written out.  Link 0 (1.5 ns a unit, free from 5): four records,
    two of them at one time; link 1 empty (free from 77); link 2 (1 ns a unit) free only at 100,
    after both its records arrive.  Weights [3, 1, 10] through packet."""
    c = case([0, 4, 4, 6], [10, 11, 30, 30, 40, 50], [2, 0, 1, 0, 2, 2], [3, 1, 10], [1500, 123, 1000], [5, 77, 100])
    # services: link 0: ceil(10 * 1.5) = 15, ceil(3 * 1.5) = 5, ceil(1.5) = 2, 5; link 2: 10, 10
    want = QR.Result(wait=np.uint64([0, 14, 0, 2, 60, 60]), done=np.uint64([25, 30, 32, 37, 110, 120]),
                     ahead=np.uint32([0, 1, 0, 1, 0, 1]), link_free=np.uint64([37, 77, 120]), busy=np.uint64([27, 0, 20]),
                     wait_max=np.uint64([14, 0, 60]), wait_sum=np.uint64([16, 0, 120]), ahead_max=np.uint32([1, 0, 1]))
    return c, want


def random_trace(lengths, seed, *, gap=40, wmax=60, costs=(0, 500, 1000, 1500), free_max=0, t0=1000, weighted=True):
    """Segments of the given lengths back to back (a length 0 is an empty link): arrivals rise by
    0 .. gap ns inside a segment, every segment starting over at t0; weights 0 .. wmax through a
    shuffled packet index, so with the default costs a record's service is about the mean gap:
    queues build and drain.  free_max: free_in drawn within free_max of t0 (not below 0), else None."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    n = int(lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)])
    step = rng.integers(0, gap + 1, n)
    run = np.cumsum(step)
    first = off[:-1][lengths > 0]
    seg = np.repeat(np.arange(len(first)), lengths[lengths > 0])
    enter = np.uint64(t0) + (run - run[first][seg]).astype(np.uint64) if n else np.zeros(0, np.uint64)
    packet = weight = None
    if weighted:
        packet = rng.permutation(n + 7)[:n]
        weight = rng.integers(0, wmax + 1, n + 7)
    cost = rng.choice(np.asarray(costs, np.uint64), len(lengths))
    free = None
    if free_max:
        lo = max(t0 - free_max, 0)
        free = np.uint64(lo) + rng.integers(0, t0 + free_max - lo, len(lengths)).astype(np.uint64)
    return case(off, enter, packet, weight, cost, free)


def packed_lengths():
    """LENGTHS back to back on one link array, an empty link between every two, an empty first
    and an empty last link."""
    out = [0]
    for n in LENGTHS:
        out += [n, 0]
    return out


def tile_edge_lengths():
    """A segment ending exactly at a tile edge with the next starting there; a one-record segment
    on either side of the next edge."""
    return [TILE - 5, 5, TILE - 1, 1, 1, TILE - 1, 3]


def second_trip(shape):
    """SECOND_TRIP records: "one" segment, "mid" 1,025 segments of 2,046 (and the rest), "three"
    segments of 3 (and the rest).  Small values: the closed form is the reference."""
    n = SECOND_TRIP
    size = dict(one=n, mid=2046, three=3)[shape]
    lengths = [size] * (n // size) + ([n % size] if n % size else [])
    return random_trace(lengths, 91, gap=20, wmax=30, costs=(500, 1000), free_max=50)


# ---- the real traces' costs.  No GPU case may be vacuous: test_queue_ref_cpu.py asserts that under
# these costs the reference alone shows a deep queue, a wait and an idle gap (conditions()).
def draw_costs(n_links, seed, costs=COSTS):
    return np.random.default_rng(seed).choice(np.asarray(costs, np.uint64), n_links)


def conditions(link_off, res):
    """(some record has ahead >= 64, some link has a positive wait, some link has an idle gap: a
    record with wait 0 after one with a positive wait)."""
    off = np.asarray(link_off).astype(np.int64)
    wait = res.wait
    gap = False
    for lk in np.flatnonzero(res.wait_max > 0):
        w = wait[off[lk]:off[lk + 1]]
        pos = np.flatnonzero(w > 0)
        if (w[pos[0]:] == 0).any():
            gap = True
            break
    return bool((res.ahead >= 64).any()), bool((res.wait_max > 0).any()), gap


# ---- the sweep graphs: a round of this module's own per graph, since the cases' own rounds put
# fewer than 65 records on any link of most graphs (no cost gives ahead >= 64 there)
SWEEP_PACKETS, SWEEP_BURST = 3000, 1500


def sweep_round(c):
    """For a case of sweep_cases: 3,000 packets from the hosts of the node of row 0 to hosts
    anywhere, mixed statuses; the first 1,500 are sent at one instant (a burst that queues on the
    sender's links), the others over the millisecond after it (they find the queue drained or
    draining).  Returns (packets, statuses)."""
    import link_round_cases as RC

    src_hosts = np.flatnonzero(c["hosts"]["route"] == 0)
    pk = RC.batch(SWEEP_PACKETS, c["hosts"], 77, src_hosts=src_hosts)
    pk["send_time"][:SWEEP_BURST] = RC.T0
    return pk, RC.mixed_status(SWEEP_PACKETS, 78)


# cost seeds under which conditions() holds on sweep_round's trace (found by trying 0, 1, ..: on a
# graph of one to four links most draws leave the busy link at cost 0)
SWEEP_SEED = {"k00": 1, "k01": 3, "k12": 4, "k26": 1, "k36": 3, "k38": 3}


def sweep_costs(name, n_links):
    """One cost per link drawn from COSTS."""
    import sweep_cases as WC

    return draw_costs(n_links, 1000 * WC.NAMES.index(name) + SWEEP_SEED.get(name, 0))


# the tie round (1 ms of sends, payloads to 1,448 bytes, whole-millisecond arcs) at 80 Mbit/s on
# every link; the wide round (8.6 s of sends on a 48-node ring) at 80 kbit/s
TIE_COST = 100_000
WIDE_COST = 10**8
GROUP_WORLDS = (1, 3)


def group_status(mixed):
    """The group case's statuses: the tie round's mixed ones with every drop turned into a
    delivery, so three packets of four count (a quarter leaves no link 65 records)."""
    return np.where(np.asarray(mixed) == 3, 3, 0).astype(np.uint8)
