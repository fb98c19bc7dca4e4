"""Link queues, the definition restated (include/shadow_gpu.h, "link queues"; DESIGN.md section
3.14).  Deliberately not the library's algorithm: the library runs one flat segmented scan in the
(max, saturating +) algebra over all records and finds `ahead` by a binary search; `loop` here
takes the segments one at a time as a plain loop over Python integers and counts `ahead` directly.

Link L owns records [link_off[L], link_off[L + 1]); taking them in the order given, with `done`
starting at free_in[L]:
    s     = min(ceil(w * cost_ps[L] / 1000), 2^64 - 1)
    start = max(enter, done);  done = min(start + s, 2^64 - 1);  wait = start - enter
    ahead = #{earlier records of the segment with done > enter}

`closed` is the same for small values (nothing near 2^63) in numpy, all segments at once, for the
large cases: done = maximum.accumulate(enter - S_excl) + S_incl per segment.  test_queue_ref_cpu.py
qualifies it against `loop`.
"""
from collections import namedtuple

import numpy as np

MAX = (1 << 64) - 1
UMAX = 0xFFFFFFFF
OK, INVALID_ARG, TIME_OVERFLOW = 0, 5, 11

Result = namedtuple("Result", "wait done ahead link_free busy wait_max wait_sum ahead_max")
FIELDS = Result._fields
RECORD_FIELDS = FIELDS[:3]
DTYPES = dict(wait=np.uint64, done=np.uint64, ahead=np.uint32, link_free=np.uint64, busy=np.uint64, wait_max=np.uint64,
              wait_sum=np.uint64, ahead_max=np.uint32)


def service(w, cost):
    """min(ceil(w cost / 1000), 2^64 - 1) on Python integers."""
    return min(-((-int(w) * int(cost)) // 1000), MAX)


def bad_link_off(link_off, n_records):
    """The link a bad link_off is reported at, or None: link_off[0] != 0 is link 0, link_off[L + 1]
    < link_off[L] link L, link_off[n_links] != n_records link n_links; the smallest."""
    off = [int(x) for x in link_off]
    if off[0] != 0:
        return 0
    for k in range(len(off) - 1):
        if off[k + 1] < off[k]:
            return k
    return len(off) - 1 if off[-1] != n_records else None


def weights(n, packet, weight):
    """The weight of every record (Python ints), and the first record whose packet index is not
    below the weights' count (or None); such a record weighs 0."""
    if weight is None:
        return [1] * n, None
    w, bad = [], None
    for i, p in enumerate(np.asarray(packet).tolist()):
        if p >= len(weight):
            bad = i if bad is None else bad
            w.append(0)
        else:
            w.append(int(weight[p]))
    return w, bad


def _summaries(off, s, wait, done, ahead, free_in):
    nl = len(off) - 1
    link = np.repeat(np.arange(nl), np.diff(off))
    out = {k: np.zeros(nl, DTYPES[k]) for k in FIELDS[3:]}
    out["link_free"][:] = 0 if free_in is None else np.asarray(free_in, np.uint64)
    full = off[1:] > off[:-1]
    out["link_free"][full] = done[off[1:][full] - 1]
    with np.errstate(over="ignore"):
        np.add.at(out["busy"], link, s)
        np.add.at(out["wait_sum"], link, wait)  # wraps
    np.maximum.at(out["wait_max"], link, wait)
    np.maximum.at(out["ahead_max"], link, ahead)
    return out


def loop(link_off, enter, packet=None, weight=None, *, cost_ps, free_in=None):
    """(status, (link, record in the link) or None, Result): the definition, a segment at a time.
    A bad link_off is reported before anything is computed (Result None)."""
    n = len(enter)
    bad = bad_link_off(link_off, n)
    if bad is not None:
        return INVALID_ARG, (bad, UMAX), None
    off = np.asarray(link_off).astype(np.int64)
    ent = [int(x) for x in np.asarray(enter).tolist()]
    w, bad_packet = weights(n, packet, weight)
    s, wait, done, ahead = (np.zeros(n, np.uint64) for _ in range(4))
    overflow = None
    for lk in range(len(off) - 1):
        i0, i1 = int(off[lk]), int(off[lk + 1])
        d = 0 if free_in is None else int(free_in[lk])
        for i in range(i0, i1):
            si = service(w[i], cost_ps[lk])
            start = max(ent[i], d)
            d = min(start + si, MAX)
            if d == MAX and overflow is None:
                overflow = i
            s[i], wait[i], done[i] = si, start - ent[i], d
            ahead[i] = int((done[i0:i] > np.uint64(ent[i])).sum())
    res = Result(wait, done, ahead.astype(np.uint32), **_summaries(off, s, wait, done, ahead.astype(np.uint32), free_in))
    for code, i in ((INVALID_ARG, bad_packet), (TIME_OVERFLOW, overflow)):
        if i is not None:
            lk = int(np.searchsorted(off, i, side="right")) - 1
            return code, (lk, i - int(off[lk])), res
    return OK, None, res


def closed(link_off, enter, packet=None, weight=None, *, cost_ps, free_in=None):
    """Result for a valid input of small values (every time and sum far below 2^62), all segments
    at once: segmented prefix sums and a segmented running maximum."""
    off = np.asarray(link_off).astype(np.int64)
    nl, n = len(off) - 1, len(enter)
    link = np.repeat(np.arange(nl), np.diff(off))
    ent = np.asarray(enter).astype(np.int64)
    w = np.ones(n, np.int64) if weight is None else np.asarray(weight).astype(np.int64)[np.asarray(packet).astype(np.int64)]
    cost = np.asarray(cost_ps).astype(np.int64)[link]
    assert n == 0 or (w.max() < 1 << 31 and cost.max() < 1 << 31)
    s = -((-w * cost) // 1000)
    first = off[:-1][off[1:] > off[:-1]]  # the first record of every non-empty segment
    e1 = ent.copy()
    if free_in is not None:
        e1[first] = np.maximum(ent[first], np.asarray(free_in).astype(np.int64)[link[first]])
    seg = np.zeros(n, np.int64)
    seg[first] = 1
    seg = np.cumsum(seg) - 1  # the number of the record's segment among the non-empty ones
    s_incl = np.cumsum(s)
    s_incl -= (s_incl - s)[first][seg] if n else 0
    v = e1 - (s_incl - s)
    big = int(v.max() - v.min() + 1) if n else 1
    assert big * (len(first) + 1) < 1 << 62 and (n == 0 or int(ent.max()) + int(s_incl.max()) < 1 << 62)
    done = np.maximum.accumulate(v + seg * big) - seg * big + s_incl
    wait = done - s - ent
    # done is non-decreasing in a segment: the records ahead are those from the first done > enter on
    span = int(max(done.max(), ent.max()) + 1) if n else 1
    assert span * (len(first) + 1) < 1 << 62
    at = np.searchsorted(done + seg * span, ent + seg * span, side="right")
    ahead = (np.arange(n) - np.minimum(at, np.arange(n))).astype(np.uint32)
    u = lambda x: x.astype(np.uint64)  # noqa: E731
    return Result(u(wait), u(done), ahead, **_summaries(off, u(s), u(wait), u(done), ahead, free_in))
