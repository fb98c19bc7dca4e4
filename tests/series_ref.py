"""The link time series, the definition restated in numpy (include/shadow_gpu.h, "link time
series") on top of trace_ref.unsorted_records, which test_trace_ref_cpu.py
qualifies against tree_ref and the oracle.  Deliberately not the library's algorithm: the crossings
are expanded on the host, every time is a Python int, the quotient is Python's own // on unbounded
integers (no reciprocal, no shift), and the cells are summed by one np.add.at per array (no
per-workgroup matrices).

For every crossing of a counted packet p on link L: s = slot[L] (None: the identity; 0xFFFFFFFF:
not watched); t = enter (at = 0) or exit (at = 1);
    t <  t0:                outside[2 s]     += w
    q = (t - t0) // bin:    series[s, q]     += w   when q < n_bins
                            outside[2 s + 1] += w   otherwise
w = weight[p], 1 without weights; sums are u64 and wrap, added to `base` when given."""
import numpy as np

import trace_ref as XR

UMAX = 0xFFFFFFFF
AT_ENTER, AT_EXIT = 0, 1


def identity_slots(g):
    return None, XR.n_links(g)


def list_slots(g, links):
    """The map of a list of link numbers: slot = position."""
    m = np.full(XR.n_links(g), UMAX, np.uint32)
    m[np.asarray(links, np.int64)] = np.arange(len(links), dtype=np.uint32)
    return m, len(links)


def crossings(g, nodes, rows, pred, tab_lat, hosts, pk, status=None, weight=None):
    """(link i64, weight u64, enter, exit) of every crossing; the times as lists of Python ints."""
    link, packet, _, enter, leave = XR.unsorted_records(g, nodes, rows, pred, tab_lat, hosts, pk, status)
    w = np.ones(len(link), np.uint64) if weight is None else np.asarray(weight)[packet].astype(np.uint64)
    return link, w, enter.tolist(), leave.tolist()


def bin_crossings(cross, slot, n_slots, at, t0, bin_ns, n_bins, base=None):
    """(series u64 [n_slots, n_bins], outside u64 [n_slots, 2]) from crossings()' result."""
    link, w, enter, leave = cross
    t0, bin_ns, n_bins = int(t0), int(bin_ns), int(n_bins)
    assert bin_ns > 0 and n_bins > 0 and n_slots > 0 and at in (AT_ENTER, AT_EXIT)
    s = link if slot is None else np.asarray(slot, np.int64)[link]
    assert ((s < n_slots) | (s == UMAX)).all(), "a slot value that is neither below n_slots nor UINT32_MAX"
    if base is None:
        series, outside = np.zeros((n_slots, n_bins), np.uint64), np.zeros((n_slots, 2), np.uint64)
    else:
        series, outside = base[0].copy(), base[1].copy()
    col = np.empty(len(link), np.int64)  # the bin; -1 before, -2 after
    for k, t in enumerate(enter if at == AT_ENTER else leave):
        if t < t0:
            col[k] = -1
        else:
            q = (t - t0) // bin_ns
            col[k] = q if q < n_bins else -2
    keep = s != UMAX
    inside, before, after = keep & (col >= 0), keep & (col == -1), keep & (col == -2)
    with np.errstate(over="ignore"):
        np.add.at(series, (s[inside], col[inside]), w[inside])
        np.add.at(outside, (s[before], np.zeros(int(before.sum()), np.int64)), w[before])
        np.add.at(outside, (s[after], np.ones(int(after.sum()), np.int64)), w[after])
    return series, outside


def series(g, nodes, rows, pred, tab_lat, hosts, pk, status=None, weight=None, slot=None, n_slots=None, at=AT_ENTER,
           t0=0, bin_ns=1, n_bins=1, base=None):
    cross = crossings(g, nodes, rows, pred, tab_lat, hosts, pk, status, weight)
    n_slots = XR.n_links(g) if n_slots is None else n_slots
    return bin_crossings(cross, slot, n_slots, at, t0, bin_ns, n_bins, base)


def slot_loads(link_load, slot, n_slots):
    """The identity's right-hand side: link loads summed per slot."""
    link_load = np.asarray(link_load, np.uint64)
    s = np.arange(len(link_load), dtype=np.int64) if slot is None else np.asarray(slot, np.int64)
    out = np.zeros(n_slots, np.uint64)
    keep = s != UMAX
    with np.errstate(over="ignore"):
        np.add.at(out, s[keep], link_load[keep])
    return out


def slot_totals(series, outside):
    """The identity's left-hand side: per slot, every bin and both outside cells (wrapping)."""
    with np.errstate(over="ignore"):
        return series.sum(axis=1, dtype=np.uint64) + outside.sum(axis=1, dtype=np.uint64)


def place_counts(cross, at, t0, bin_ns, n_bins):
    """(before, inside, after, inside crossings that lie exactly on a bin's lower edge), every link."""
    _, _, enter, leave = cross
    before = inside = after = edge = 0
    for t in (enter if at == AT_ENTER else leave):
        if t < t0:
            before += 1
        elif (t - t0) // bin_ns < n_bins:
            inside += 1
            edge += (t - t0) % bin_ns == 0
        else:
            after += 1
    return before, inside, after, edge
