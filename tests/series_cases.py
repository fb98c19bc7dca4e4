"""Inputs of the link-time-series tests (test_series_ref_cpu.py qualifies them on the CPU,
test_series_gpu.py and test_group_series_gpu.py run them).  Graphs, hosts and most batches are
those of tests/trace_cases.py, tests/link_round_cases.py and tests/link_cases.py."""
import numpy as np

from shadow_amd import synth

import link_round_cases as RC
import trace_cases as XC

T0 = RC.T0
MS = 1_000_000
BASE_SERIES = np.uint64(0x0101010101010101)  # what every output cell starts from
BASE_OUTSIDE = np.uint64(0x0202020202020202)

# the tie round's three bin sets (bin_ns, n_bins), all from t0 = T0 + 1 ms
TIE_T0 = T0 + MS
BIN_SETS = ((MS, 8), (250_000, 64), (333_333, 40))
# (before, inside, after, inside crossings on a bin's lower edge) of trace_cases.tie_round() with
# status = None at enter times, measured on the CPU; 42,172 crossings in all
TIE_CROSSINGS = 42_172
TIE_PLACES = {(MS, 8): (10_000, 32_024, 148, None), (250_000, 64): (10_000, 32_172, 0, 32_172),
              (333_333, 40): (10_000, 32_172, 0, 1_266)}

# the LDS budget of the form tests (cells), and (n_slots, n_bins) of 63, 64 and 65 cells
SMALL_BUDGET = 64
BUDGET_SHAPES = ((7, 7), (8, 6), (5, 11))


def hand_graph():
    """test_trace_ref_cpu.py's hand graph: the path 0 - 1 - 2 - 3 with 1 us arcs and self-loops,
    and the chord 0 - 2 of 1.5 us: from node 0, nodes 2 and 3 are reached over the chord."""
    edges = [(0, 1, 1000), (1, 2, 1000), (2, 3, 1000), (0, 2, 1500)]
    src = list(range(4)) + [e[0] for e in edges]
    dst = list(range(4)) + [e[1] for e in edges]
    lat = [1000] * 4 + [e[2] for e in edges]
    return dict(n=4, src=np.uint32(src), dst=np.uint32(dst), lat=np.uint64(lat), loss=np.zeros(8, np.float32),
                directed=False)


HAND_T = 10_000


def hand_round():
    """That test's six sends (host h on node h, host 4 on node 0), with payloads 1, 2, 4, ...:
    (hosts, packets, statuses)."""
    T = HAND_T
    sends = [(0, 3, T, 0),        # 0 - 2 - 3
             (1, 3, T + 500, 0),  # 1 - 2 - 3
             (0, 4, T + 7, 0),    # to its own node: the self-loop
             (3, 0, T + 100, 0),  # 3 - 2 - 0
             (0, 3, T, 1),        # dropped
             (0, 3, T - 200, 0)]  # 0 - 2 - 3 ahead of packet 0
    hosts = synth.make_hosts(5, 4)
    pk = dict(src=np.uint32([s[0] for s in sends]), dst_ip=hosts["ip"][[s[1] for s in sends]],
              payload=np.uint32([1 << k for k in range(len(sends))]), send_time=np.uint64([s[2] for s in sends]))
    return hosts, pk, np.uint8([s[3] for s in sends])


# ---- quotient edges: packets 0 -> 2 on trace_cases.tier_graph() (1 ms arcs): link (0, 1) is
# entered at the send time and left 1 ms later, link (1, 2) entered then and left at 2 ms
EDGE_T0 = 10 * MS
EDGE_BINS = (1, 3, 333_333, 1 << 20, (1 << 32) + 1)
EDGE_N_BINS = 4096
LAST = (1 << 64) - 1


def edge_offsets(bin_ns, n_bins=EDGE_N_BINS):
    """The values of t - t0 the case aims at (t the enter time of link (0, 1)): one below and at
    the lower edge of bins 1, 2, 63, 64, the last bin and the one past it; t0 - 1; 2^32 bins and k
    more, whose quotient truncated to 32 bits would land in bin k; 2^63 + 5.  Only those whose
    packet still arrives by 2^64 - 1."""
    xs = []
    for b in (1, 2, 63, 64, n_bins - 1, n_bins):
        xs += [b * bin_ns - 1, b * bin_ns]
    xs.append(-1)
    xs += [(1 << 32) * bin_ns + k * bin_ns for k in (0, 1, 77, n_bins - 1)]
    xs.append((1 << 63) + 5)
    return [x for x in xs if EDGE_T0 + x + 2 * MS <= LAST]


def edge_round(offsets, t0=EDGE_T0):
    """A host per node of the tier graph; packet k is sent from node 0 to node 2 at t0 +
    offsets[k], payload k + 1."""
    hosts = synth.make_hosts(3, 3)
    n = len(offsets)
    t = np.array([t0 + x for x in offsets], dtype=object)
    assert (t >= 0).all() and (t + 2 * MS <= LAST).all()
    return hosts, dict(src=np.zeros(n, np.uint32), dst_ip=np.full(n, hosts["ip"][2], np.uint32),
                       payload=np.arange(1, n + 1, dtype=np.uint32), send_time=t.astype(np.uint64))


# t0 + n_bins * bin_ns past 2^64: every crossing lies inside, whatever an end time would say
PAST_T0 = (1 << 64) - 4 * MS
PAST_BINS = ((1000, 4096), ((1 << 52) + 1, 4096))
PAST_OFFSETS = (-1, 0, 1, 999, 1000, 1_999_999)  # the last packet arrives at 2^64 - 1


def both_directions(tail, head):
    """(slot map, n_slots): links (u, v) and (v, u) share a slot, numbered by first appearance."""
    key = {}
    m = np.empty(len(tail), np.uint32)
    for k, (u, v) in enumerate(zip(np.asarray(tail).tolist(), np.asarray(head).tolist())):
        m[k] = key.setdefault((min(u, v), max(u, v)), len(key))
    return m, len(key)


def bases(n_slots, n_bins):
    return np.full((n_slots, n_bins), BASE_SERIES, np.uint64), np.full((n_slots, 2), BASE_OUTSIDE, np.uint64)


def enter_range_bins(enter, n_bins=16):
    """(t0, bin_ns) of n_bins bins over [min enter, max enter] of a view's crossings (lists of
    Python ints); one bin of 1 ns when there is no crossing."""
    if not enter:
        return 0, 1
    lo, hi = min(enter), max(enter)
    return lo, (hi - lo) // n_bins + 1
