"""Inputs of the link-queue series tests (test_queue_series_ref_cpu.py qualifies them on the CPU,
test_queue_series_gpu.py runs them), on queue_cases, queue_drop_cases, outcomes_cases and
queue_window_cases."""
import numpy as np

import outcomes_cases as OC
import queue_cases as QC
import queue_series_ref as SR
import queue_window_ref as WR

MAX = SR.MAX
T0, BIN, BINS = 1000, 10, 4  # the edge cases' range: [1000, 1040)
BIN_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 2049)  # (100,000 has a test of its own)
RECORD_COUNTS = (0, 1, 255, 256, 257)

# (what it is, e', start, service): one record on a link of its own, its wait [e', start) made by the
# link's free_in, its service [start, start + s) by its weight at 1 ns a unit
EDGES = (
    ("inside one bin", 1001, 1004, 4),
    ("across exactly two bins", 1005, 1015, 10),
    ("starting on a bin's first ns", 1010, 1013, 3),
    ("ending exactly on a bin edge", 1003, 1010, 10),
    ("of length 0, both", 1012, 1012, 0),
    ("of length 0 on a bin edge", 1020, 1020, 0),
    ("a wait of 0 and a whole bin", 1020, 1020, 10),
    ("wait across t0", 990, 1005, 2),
    ("service across t0", 980, 995, 10),
    ("wait across the end", 1030, 1045, 5),
    ("service across the end", 1030, 1035, 10),
    ("wholly before", 900, 950, 20),
    ("ending exactly at t0", 900, 950, 50),
    ("wholly after", 1100, 1150, 20),
    ("starting exactly at the end", 1040, 1050, 7),
    ("wait covering the whole range", 900, 1100, 3),
    ("service covering the whole range", 900, 950, 200),
    ("three whole bins between two partial ones", 1003, 1005, 33),
    ("whole bins only", 1000, 1010, 30),
)


def edges(pick=None):
    """The edge records, one per link (pick: only these), weights through packet."""
    rows = [EDGES[k] for k in (range(len(EDGES)) if pick is None else pick)]
    n = len(rows)
    return QC.case(np.arange(n + 1), [r[1] for r in rows], np.arange(n), [r[3] for r in rows], [1000] * n, [r[2] for r in rows])


def first_order_out(c, drop=False):
    """A first-order reference result as the call's arrays by name."""
    rc, res = OC.queue_ref(c, False, drop)
    assert rc == 0
    return OC.raw(res, drop)


def carried_out(c, H=MAX, drop=False, packets=False):
    """A carried reference result (windowed at H) as the call's arrays by name."""
    rc, out = WR.define(c, H, drop, packets)
    assert rc == 0
    return out


def matrix(c, out, hdr, *, drop=False, window=False, start=None, form=SR.diffs):
    """The matrix a call leaves: `start` (None: zeroes) plus the call's sums, wrapping."""
    nl = len(c["link_off"]) - 1
    M = form(SR.terms_of(c, out, hdr, drop=drop, window=window), hdr, nl)
    if start is not None:
        with np.errstate(over="ignore"):
            M = M + start
    return M


def pattern(shape, seed=3):
    """A non-zero start of the matrix with values near 2^64."""
    rng = np.random.default_rng(seed)
    M = rng.integers(0, 1 << 62, shape, dtype=np.uint64)
    M[rng.random(shape) < 0.25] = np.uint64(MAX)
    M[rng.random(shape) < 0.25] = np.uint64(MAX - 5)
    return M


def span_header(c, out, n_bins, slots=None, n_slots=None, margin=0):
    """A header whose bins cover the result's settled times, from `margin` bins inside on either side."""
    done = np.asarray(out["done"])[:len(c["enter"])]
    done = done[done != np.uint64(MAX)]
    lo = int(min(c["enter"].min(), done.min())) if len(done) else 0
    hi = int(done.max()) + 1 if len(done) else 1
    bin_ns = max((hi - lo) // max(n_bins - 2 * margin, 1), 1)
    return SR.header(lo + margin * bin_ns, bin_ns, n_bins, slots, n_slots)
