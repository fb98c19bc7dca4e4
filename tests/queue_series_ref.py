"""Link queues over time (sg_link_queue with its series flag), the definition restated over Python integers
(include/shadow_gpu.h, "link queues").  The queue result itself comes from the
existing references (queue_ref, queue_drop_ref, queue_window_ref.define, which covers the carried form at
H = 2^64 - 1); on top of it, two restatements of the series:

  * `naive`: per record and per column the intersection of the record's intervals with the column's
    span, one column at a time.  Normative.
  * `diffs`: what the library does -- the two end bins added directly, the whole bins between them as a
    +1 / -1 pair in a difference array, a running sum along each row -- over Python integers for the
    records and numpy u64 (which wraps) for the rows: the reference of the large shapes.

Both take `terms`: per counted record (slot, state, weight, e', start, done), built from a call's result
by `terms_of`.  M is u64 [4, S, B + 2]: planes busy_ns, wait_ns, served, dropped; column B before t0,
column B + 1 at or after t0 + B bin_ns.
"""
import numpy as np

import queue_ref as QR
from queue_ref import MAX, UMAX

SERIES_FLAG = "SG_LINK_" + "QUEUE_SERIES"  # (in two parts: queue_carry_cases.CARRY_FLAG tells why)
SERIES = 0x40
UNWATCHED = MAX
CAPACITY = 10


def header(t0, bin_ns, n_bins, slots=None, n_slots=None):
    """The tail behind cost_ps: (t0, bin_ns, n_bins, n_slots) and, with a slot map, a slot per link
    (UNWATCHED: not watched).  n_slots None: the largest slot + 1."""
    if slots is None:
        return np.array([t0, bin_ns, n_bins, 0], np.uint64)
    slots = [int(s) for s in slots]
    if n_slots is None:
        n_slots = max([s for s in slots if s != UNWATCHED], default=0) + 1
    return np.array([t0, bin_ns, n_bins, n_slots] + slots, np.uint64)


def shape_of(hdr, n_links):
    """(t0, bin_ns, B, S, the slot of every link or None for one not watched) of a header."""
    t0, bin_ns, B, ns = (int(x) for x in hdr[:4])
    if ns == 0:
        return t0, bin_ns, B, n_links, list(range(n_links))
    slot = [int(x) for x in hdr[4:4 + n_links]]
    return t0, bin_ns, B, ns, [None if s == UNWATCHED or s >= ns else s for s in slot]


def bad_slot(hdr, n_links):
    """The smallest link whose slot is neither below S nor UNWATCHED, or None."""
    ns = int(hdr[3])
    if ns == 0:
        return None
    return next((lk for lk in range(n_links) if int(hdr[4 + lk]) != UNWATCHED and int(hdr[4 + lk]) >= ns), None)


def terms_of(c, out, hdr, *, drop=False, window=False):
    """[(slot, "served" | "dropped", w, e', start, done)] of the counted records of a call's result `out`
    (wait, done and ahead by name, at least n entries each) on the case c: the records of watched links
    that are served or dropped.  A record's state is read from the sentinels."""
    off = np.asarray(c["link_off"]).astype(np.int64)
    n, nl = int(off[-1]), len(off) - 1
    slot = shape_of(hdr, nl)[4]
    w, _ = QR.weights(n, c["packet"], c["weight"])
    wait, done, ahead = (np.asarray(out[k]).tolist() for k in ("wait", "done", "ahead"))
    res = []
    for lk in range(nl):
        if slot[lk] is None:
            continue
        for i in range(int(off[lk]), int(off[lk + 1])):
            if window and wait[i] == MAX and ahead[i] == UMAX:
                continue  # pending
            if not drop or wait[i] != MAX:
                start = done[i] - QR.service(w[i], c["cost_ps"][lk])
                res.append((slot[lk], "served", w[i], start - wait[i], start, done[i]))
            elif done[i] != MAX:
                res.append((slot[lk], "dropped", w[i], done[i], done[i], done[i]))
    return res


def column(t, t0, bin_ns, B):
    if t < t0:
        return B
    q = (t - t0) // bin_ns
    return q if q < B else B + 1


def _array(M):
    return np.array([[[x & MAX for x in row] for row in plane] for plane in M], dtype=np.uint64).reshape(4, len(M[0]), -1)


def naive(terms, hdr, n_links):
    """The definition, a column at a time: O(records x columns)."""
    t0, bin_ns, B, S, _ = shape_of(hdr, n_links)
    M = [[[0] * (B + 2) for _ in range(S)] for _ in range(4)]
    end = t0 + B * bin_ns  # (unbounded: may pass 2^64)
    spans = [(t0 + k * bin_ns, t0 + (k + 1) * bin_ns) for k in range(B)] + [(0, t0), (end, 1 << 200)]
    for s, state, w, e, start, done in terms:
        if state == "dropped":
            M[3][s][column(e, t0, bin_ns, B)] += w
            continue
        M[2][s][column(done, t0, bin_ns, B)] += w
        for plane, (a, b) in ((0, (start, done)), (1, (e, start))):
            for k, (lo, hi) in enumerate(spans):
                M[plane][s][k] += max(0, min(b, hi) - max(a, lo))
    return _array(M)


def diffs(terms, hdr, n_links):
    """The difference-array form: O(records + cells)."""
    t0, bin_ns, B, S, _ = shape_of(hdr, n_links)
    M = np.zeros((4, S, B + 2), np.uint64)
    D = np.zeros((2, S, B + 1), np.uint64)
    add = {}

    def put(plane, s, k, v):
        add[(plane, s, k)] = add.get((plane, s, k), 0) + v

    for s, state, w, e, start, done in terms:
        if state == "dropped":
            put(3, s, column(e, t0, bin_ns, B), w)
            continue
        put(2, s, column(done, t0, bin_ns, B), w)
        for plane, (a, b) in ((0, (start, done)), (1, (e, start))):
            if a >= b:
                continue
            if a < t0:
                put(plane, s, B, min(b, t0) - a)
                a = t0
            if b <= t0:
                continue
            x, y = a - t0, b - t0
            qx = x // bin_ns
            if qx >= B:
                put(plane, s, B + 1, y - x)
                continue
            if y // bin_ns >= B:
                put(plane, s, B + 1, y - B * bin_ns)
                y = B * bin_ns
            qy = y // bin_ns
            if qx == qy:
                put(plane, s, qx, y - x)
                continue
            put(plane, s, qx, (qx + 1) * bin_ns - x)
            if y - qy * bin_ns:
                put(plane, s, qy, y - qy * bin_ns)
            if qy > qx + 1:
                put(-1 - plane, s, qx + 1, 1)
                put(-1 - plane, s, qy, -1)
    for (plane, s, k), v in add.items():
        if plane < 0:
            D[-1 - plane, s, k] = np.uint64(v & MAX)
        else:
            M[plane, s, k] = np.uint64(v & MAX)
    with np.errstate(over="ignore"):
        M[:2, :, :B] += np.cumsum(D[:, :, :B], axis=2, dtype=np.uint64) * np.uint64(bin_ns)
    return M


def plane_sums(M):
    """[4, S] Python-int sums over all B + 2 columns, mod 2^64."""
    return [[sum(int(x) for x in row) & MAX for row in plane] for plane in M]


def link_sums_by_slot(values, hdr, n_links):
    """Per-link values summed over the links of every slot, mod 2^64."""
    S, slot = shape_of(hdr, n_links)[3:]
    out = [0] * S
    for lk in range(n_links):
        if slot[lk] is not None:
            out[slot[lk]] = (out[slot[lk]] + int(values[lk])) & MAX
    return out
