"""The link-queue series on the card (sg_link_queue with its series flag, shadow_amd.LinkQueueSeries and the
series= keyword) against tests/queue_series_ref.py over the existing queue references.

Every output starts from sentinel values, the matrix from a pattern with values near 2^64, and every
comparison is np.array_equal.  Unless a test says otherwise a case runs in host and in device mode and
in both kernel forms of the scan.  test_queue_series_ref_cpu.py qualifies the reference and the cases."""
import numpy as np
import pytest

import outcomes_cases as OC
import queue_carry_cases as CC
import queue_cases as QC
import queue_drop_cases as DC
import queue_gpu_calls as QG
import queue_ref as QR
import queue_series_cases as SC
import queue_series_ref as SR
import queue_window_cases as WC
import queue_window_ref as WR
from queue_gpu_calls import CARRY, DROP, FORMS, VIEW, _batch, _form, _host_table, _net, _pair

pytestmark = pytest.mark.gpu

MAX = QR.MAX
RAW = QR.FIELDS
PACKETS, WINDOW, SERIES = 0x10, 0x20, SR.SERIES
INVALID_ARG, CAPACITY = QR.INVALID_ARG, SR.CAPACITY
INPUTS = ("link_off", "enter", "packet", "weight", "cost_ps", "free_in")


def _sizes(c, drop, packets):
    n, nl = len(c["enter"]), len(c["link_off"]) - 1
    P = c.get("n_packets", 0) if packets else 0
    return {k: n + P if k in QR.RECORD_FIELDS else (2 * nl if drop and k in ("busy", "ahead_max") else nl) for k in RAW}


def _call(ctx, c, hdr, *, dev, carry=False, drop=False, packets=False, H=None, series=True, start=None, null=(), nullout=(),
          n_records=None, handle=None):
    """One sg_link_queue call on a case's arrays with the header (and slot map) behind cost_ps and the matrix
    `start` (None: the pattern) behind out_link_busy_ns, every other output starting from sentinels.
    series False: the same arrays without the bit.  (status, outputs by name, the matrix afterwards)."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    nl = len(c["link_off"]) - 1
    S, B = SR.shape_of(hdr, nl)[3], int(hdr[2])
    if start is None:
        start = SC.pattern((4, S, B + 2))
    size = _sizes(c, drop, packets)
    outs = {k: np.full(size[k], QC.SENT32 if QR.DTYPES[k] == np.uint32 else QC.SENT64, QR.DTYPES[k]) for k in RAW}
    c0 = size["busy"]
    outs["busy"] = np.concatenate([outs["busy"], start.ravel()])
    free = np.zeros(nl, np.uint64) if c["free_in"] is None and H is not None else c["free_in"]
    arrays = dict(c, cost_ps=np.concatenate([c["cost_ps"]] + ([c["limit_ns"]] if drop else []) + [np.asarray(hdr, np.uint64)]),
                  free_in=free if H is None else np.concatenate([free, np.array([H], np.uint64)]))
    if packets:
        arrays["enter"] = np.concatenate([c["enter"], c["base"]])
    keep = []

    def ptr(a):
        if a is None:
            return None
        if not dev:
            keep.append((a, a if a.size else np.zeros(1, a.dtype)))
            return C.c_void_p(keep[-1][1].ctypes.data)
        t = torch.from_numpy(np.ascontiguousarray(a).view(VIEW[a.dtype]).copy() if a.size else np.zeros(1, VIEW[a.dtype])).cuda()
        keep.append((a, t))
        return C.c_void_p(t.data_ptr())

    ip = [None if k in null else ptr(arrays[k]) for k in INPUTS]
    n_in = len(keep)
    op = {k: None if k in nullout else ptr(outs[k]) for k in RAW}
    if dev:
        torch.cuda.synchronize()
    if "n_packets" in c:
        n_weights = c["n_packets"]
    else:
        n_weights = 0 if c["weight"] is None else len(c["weight"])
    flags = (_capi.SG_ROUTE_OUT_DEVICE if dev else 0) | (CARRY if carry else 0) | (DROP if drop else 0) | \
        (PACKETS if packets else 0) | (0 if H is None else WINDOW) | (SERIES if series else 0)
    rc = _capi.load().sg_link_queue((ctx if handle is None else handle).handle, flags, nl, ip[0],
                                    len(c["enter"]) if n_records is None else n_records, ip[1], ip[2], ip[3], n_weights,
                                    ip[4], ip[5], *[op[k] for k in RAW])
    if dev:
        torch.cuda.synchronize()
        for a, t in keep[n_in:]:
            if a.size:
                a[...] = t.cpu().numpy().view(a.dtype)
    M = outs["busy"][c0:].reshape(4, S, B + 2).copy()
    outs["busy"] = outs["busy"][:c0]
    return rc, outs, M


def _reference(c, *, carry, drop, packets, H):
    """The call's arrays without the bit, from the mode's reference."""
    if carry:
        return SC.carried_out(c, MAX if H is None else H, drop, packets)
    return OC.want(c, False, drop)[0] if packets else SC.first_order_out(c, drop)


def _untouched(outs, M, start):
    return QG._untouched(outs) and np.array_equal(M, start)


def _check(ctx, monkeypatch, c, hdrs, *, carry=False, drop=False, packets=False, H=None, devs=(True, False), forms=FORMS,
           want=None, names=RAW):
    """The case under every header in every array mode and form: the matrix against the reference's sums
    on top of the pattern, every other output against the call's reference.  Returns the last matrix's
    sums alone."""
    from shadow_amd import _capi

    want = _reference(c, carry=carry, drop=drop, packets=packets, H=H) if want is None else want
    nl = len(c["link_off"]) - 1
    sums = None
    for hdr in hdrs:
        sums = SC.matrix(c, want, hdr, drop=drop, window=H is not None)
        start = SC.pattern(sums.shape)
        with np.errstate(over="ignore"):
            expect = sums + start
        for form in forms:
            _form(monkeypatch, form)
            for dev in devs:
                rc, outs, M = _call(ctx, c, hdr, dev=dev, carry=carry, drop=drop, packets=packets, H=H, start=start)
                _capi.check(ctx.handle, rc)
                where = (hdr[:4].tolist(), form, "device" if dev else "host")
                assert np.array_equal(M, expect), \
                    f"M {where}: {int((M != expect).sum())} of {M.size} cells differ, first at {np.argwhere(M != expect)[0].tolist()}"
                for k in names:
                    assert outs[k].shape == want[k].shape and np.array_equal(outs[k], want[k]), (k, where)
                assert int(ctx.read_timer("link_queue_series_cells")[1]) == SR.shape_of(hdr, nl)[3] * (int(hdr[2]) + 2)
    return sums


# ---- 1. one interval in every position, for both planes
EDGE_HEADERS = ((SC.T0, SC.BIN, SC.BINS), (SC.T0, 1, 40), (SC.T0, 40, 1), (SC.T0 + 3, 7, 5), (0, 1 << 40, 2), (MAX - 20, 7, 5),
                (SC.T0, 1 << 62, 5))


def test_edges(ctx, monkeypatch):
    c = SC.edges()
    _check(ctx, monkeypatch, c, [SR.header(*h) for h in EDGE_HEADERS])
    # shared slots and links that are not watched: every third edge in slot 0, every third in none
    nl = len(SC.EDGES)
    slots = [(0, SR.UNWATCHED, 1)[k % 3] for k in range(nl)]
    _check(ctx, monkeypatch, c, [SR.header(SC.T0, SC.BIN, SC.BINS, slots, 2), SR.header(SC.T0, SC.BIN, SC.BINS, [0] * nl, 1),
                                 SR.header(SC.T0, SC.BIN, SC.BINS, [SR.UNWATCHED] * nl, 3)])


@pytest.mark.parametrize("k", range(len(SC.EDGES)), ids=[e[0] for e in SC.EDGES])
def test_edges_one_by_one(ctx, k):
    """A record alone in its call, from a zeroed matrix, device mode."""
    c = SC.edges([k])
    want = SC.first_order_out(c)
    for h in EDGE_HEADERS[:4]:
        hdr = SR.header(*h)
        expect = SC.matrix(c, want, hdr)
        rc, outs, M = _call(ctx, c, hdr, dev=True, start=np.zeros_like(expect))
        assert rc == 0 and np.array_equal(M, expect), (h, M.tolist(), expect.tolist())


def test_times_near_2_63_and_an_end_past_2_64(ctx, monkeypatch):
    c = QC.case([0, 2, 3], [(1 << 63) - 5, (1 << 63) + 1, MAX - 1000], None, None, [3000, 7000], [1 << 63, 0])
    hdrs = [SR.header((1 << 63) - 8, 1 << 62, 3), SR.header(1 << 63, 1 << 60, 16), SR.header((1 << 63) + 2, 3, 2),
            SR.header(MAX - 1005, 20, 65), SR.header(MAX, 1, 1)]
    assert all(int(h[0]) + int(h[1]) * int(h[2]) >= 1 << 64 for h in hdrs[:2] + hdrs[3:])
    _check(ctx, monkeypatch, c, hdrs)


# ---- 2. the row pass: bin counts on either side of a wave, a workgroup, a chunk
def _mixed_case(seed=12):
    """Five links with an empty one between full ones, queues that build and drain, weights."""
    return QC.random_trace([300, 0, 70, 1, 129], seed, free_max=30)


@pytest.mark.parametrize("B", SC.BIN_COUNTS)
def test_bin_counts(ctx, monkeypatch, B):
    c = _mixed_case()
    want = SC.first_order_out(c)
    slots = [1, 0, SR.UNWATCHED, 1, 2]
    span = int(want["done"].max()) - 1000
    hdrs = [SC.span_header(c, want, B), SC.span_header(c, want, B, slots, 3, margin=min(1, (B - 1) // 2)),
            SR.header(1000, span + 7, B, [0] * 5, 1), SR.header(1000, 1, B)]
    sums = _check(ctx, monkeypatch, c, hdrs, devs=(True,))
    _check(ctx, monkeypatch, c, hdrs[1:2], forms=FORMS[:1], devs=(False,))
    assert sums[:2].sum() > 0


def test_100000_bins_of_1_ns(ctx):
    """A wait across all 100,000 bins, a service across most of them, records inside: the cost of a
    record does not follow the bins it spans."""
    B = 100_000
    c = QC.case([0, 3, 4], [900, 50_000, 50_001, 10], None, None, [10**6, 95 * 10**6], [B + 2000, 5005])
    want = SC.first_order_out(c)
    assert int(want["wait"][0]) > B + 1000 and int(want["done"][3]) - int(want["wait"][3]) - 10 == 95_000
    hdr = SR.header(1000, 1, B, [1, 0], 2)
    expect = SC.matrix(c, want, hdr, start=SC.pattern((4, 2, B + 2)))
    rc, outs, M = _call(ctx, c, hdr, dev=True, start=SC.pattern((4, 2, B + 2)))
    assert rc == 0 and np.array_equal(M, expect)
    plain = SC.matrix(c, want, hdr)
    assert (plain[1, 1, :B] >= 1).all() and plain[0, 0, 4005:99005].tolist() == [1] * 95000 and not plain[0, 0, 99005:B].any()


# ---- 3. contention: a hot link, many one-record links, record counts
@pytest.mark.parametrize("B", (1, 4096))
def test_hot_link(ctx, monkeypatch, B):
    """100,000 records on one link between two small ones."""
    c = QC.random_trace([50, 100_000, 3], 77, gap=20, wmax=30, costs=(500, 1000))
    want = {k: v for k, v in QC.ref(c, closed=True)._asdict().items()}
    hdr = SC.span_header(c, want, B, [0, 1, 1], 2)
    sums = _check(ctx, monkeypatch, c, [hdr], devs=(True,), want=want)
    assert int(sums[2, 1].sum()) == int(c["weight"][c["packet"][50:]].sum())


def test_5000_one_record_links(ctx, monkeypatch):
    rng = np.random.default_rng(5)
    n = 5000
    c = QC.case(np.arange(n + 1), 1000 + rng.integers(0, 500, n), None, None, rng.integers(0, 40000, n), 1000 + rng.integers(0, 500, n))
    want = SC.first_order_out(c)
    _check(ctx, monkeypatch, c, [SR.header(1100, 60, 7), SR.header(1100, 60, 7, rng.integers(0, 9, n).tolist(), 9)], devs=(True,))
    assert want["wait"].any()


@pytest.mark.parametrize("n", SC.RECORD_COUNTS)
def test_record_counts(ctx, monkeypatch, n):
    c = QC.random_trace([n // 2, 0, n - n // 2], 3 + n, free_max=20)
    sums = _check(ctx, monkeypatch, c, [SR.header(1010, 50, 9), SR.header(1010, 50, 9, [0, 0, 0], 1)])
    assert (sums.sum() == 0) == (n == 0)  # (no record: the matrix is left as it is)


def test_shuffled_first_order_segments(ctx, monkeypatch):
    """The recurrence does not want a segment sorted: the same cell comes back in later lanes."""
    c = _mixed_case(14)
    rng = np.random.default_rng(1)
    off = c["link_off"].astype(np.int64)
    enter = c["enter"].copy()
    for k in range(len(off) - 1):
        enter[off[k]:off[k + 1]] = rng.permutation(enter[off[k]:off[k + 1]])
    c = dict(c, enter=enter)
    _check(ctx, monkeypatch, c, [SR.header(1005, 90, 40), SR.header(1005, 90, 40, [0, 1, 0, 1, 0], 2)])


# ---- 4. every form of the call
MODES = [(carry, drop, packets) for carry in (False, True) for drop in (False, True) for packets in (False, True)]
MODE_IDS = ["-".join(w for w, on in zip(("carry", "drop", "packets"), m) if on) or "first-order" for m in MODES]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_modes(ctx, monkeypatch, mode):
    """First order, carried, with limits (dropped counted, absent not), with the packet pass."""
    carry, drop, packets = mode
    c = OC.with_base(DC.draw_limits(CC.from_lengths([257, 70, 3, 0, 40], 31), 32, limits=(0, 5, 20, 60, MAX)))
    want = _reference(c, carry=carry, drop=drop, packets=packets, H=None)
    n = len(c["enter"])
    if drop:
        lost = want["wait"][:n] == np.uint64(MAX)
        assert lost.any() and (not carry or (lost & (want["done"][:n] == np.uint64(MAX))).any())
    hdrs = [SC.span_header(c, want, 33, margin=2), SC.span_header(c, want, 300, [0, 1, SR.UNWATCHED, 1, 0], 2)]
    sums = _check(ctx, monkeypatch, c, hdrs, carry=carry, drop=drop, packets=packets, want=want)
    assert (sums[3].sum() > 0) == drop


@pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)
def test_horizons(ctx, monkeypatch, mode):
    """A horizon below, on, between and above the records: pending records are not counted."""
    drop, packets = mode
    c = WC.segments(129)
    closed = SC.carried_out(c, MAX, drop)
    hdr = SC.span_header(c, closed, 40, [0, 1, 1, 0], 2, margin=1)
    seen = set()
    for H in WC.horizons(c, drop):
        want = SC.carried_out(c, H, drop, packets)
        seen.add(int(want["pending"].sum()))
        _check(ctx, monkeypatch, c, [hdr], carry=True, drop=drop, packets=packets, H=H, want=want, forms=FORMS[:1])
    assert 0 in seen and len(c["enter"]) in seen and len(seen) >= 4


# ---- 5. sums across calls
@pytest.mark.parametrize("drop", (False, True), ids=("plain", "drop"))
def test_re_feeding_through_raw_calls(ctx, drop):
    """queue_window_ref.SessionRef with the library answering every call into one matrix on the host's
    side: 2, 5 and 17 rounds and a flush sum to the single carried call's matrix."""
    from shadow_amd import _capi

    for k, seed in ((2, 0), (5, 1), (17, 2)):
        c = OC.random_case(100 + seed)
        hdr = SC.span_header(c, SC.carried_out(c, MAX, drop), 21, margin=2)
        nl = len(c["link_off"]) - 1
        box = [SC.pattern((4, nl, 23))]
        first = box[0].copy()

        def solve(rc, H, d):
            rc = dict(rc, limit_ns=rc.get("limit_ns"))
            st, outs, M = _call(ctx, rc, hdr, dev=True, carry=True, drop=d, packets=True, H=H, start=box[0])
            _capi.check(ctx.handle, st)
            box[0] = M
            return outs

        whole, _ = WC.run_session(c, k, seed, drop, solve)
        want = SC.matrix(whole, SC.carried_out(whole, MAX, drop), hdr, drop=drop, start=first)
        assert np.array_equal(box[0], want)


def test_two_calls_into_one_matrix(ctx):
    """Device mode adds to what the matrix holds; a call with limits and one without share the cells."""
    from shadow_amd import LinkQueueSeries, link_queue

    a, b = _mixed_case(20), DC.draw_limits(_mixed_case(21), 4, limits=(0, 5, 20))
    wa, wb = SC.first_order_out(a), SC.first_order_out(b, True)
    hdr = SC.span_header(a, wa, 50, [0, 1, 1, SR.UNWATCHED, 2], 3)
    s = LinkQueueSeries(ctx, int(hdr[0]), int(hdr[1]), 50, n_links=5, link_slot=[0, 1, 1, -1, 2])
    ra = link_queue(ctx, a["link_off"], a["enter"], a["packet"], a["weight"], cost_ps=a["cost_ps"], free_ns=a["free_in"], series=s)
    assert np.array_equal(s.planes(), SC.matrix(a, wa, hdr))
    rb = link_queue(ctx, b["link_off"], b["enter"], b["packet"], b["weight"], cost_ps=b["cost_ps"], free_ns=b["free_in"],
                    limit_ns=b["limit_ns"], series=s)
    both = SC.matrix(b, wb, hdr, drop=True, start=SC.matrix(a, wa, hdr))
    assert np.array_equal(s.planes(), both) and both[3].sum() > 0
    assert np.array_equal(ra.link_busy_ns, wa["busy"]) and ra.link_busy_ns.shape == (5,)
    assert np.array_equal(rb.link_busy_ns, wb["busy"][:5]) and np.array_equal(rb.link_refused_ns, wb["busy"][5:])
    assert np.array_equal(s.busy_ns, both[0, :, :50]) and np.array_equal(s.wait_ns, both[1, :, :50])
    assert np.array_equal(s.served, both[2, :, :50]) and np.array_equal(s.dropped, both[3, :, :50])
    assert np.array_equal(s.before, both[:, :, 50]) and np.array_equal(s.after, both[:, :, 51])
    assert np.array_equal(s.utilisation(), both[0, :, :50] / float(hdr[1])) and s.mean_waiting().shape == (3, 50)
    s.reset()
    assert not s.planes().any()


def test_a_slot_of_one_link_is_busy_at_most_bin_ns(ctx):
    c = QC.random_trace([3000, 0, 500], 5, free_max=10)
    want = {k: v for k, v in QC.ref(c, closed=True)._asdict().items()}
    for bin_ns, B in ((1, 3000), (13, 300), (1000, 5)):
        hdr = SR.header(990, bin_ns, B)
        rc, outs, M = _call(ctx, c, hdr, dev=True, start=np.zeros((4, 3, B + 2), np.uint64))
        assert rc == 0 and np.array_equal(M, SC.matrix(c, want, hdr))
        assert 0 < int(M[0, :, :B].max()) <= bin_ns
        sums = SR.plane_sums(M)
        assert sums[0] == [int(x) for x in outs["busy"]] and sums[1] == [int(x) for x in outs["wait_sum"]]


# ---- 6. the guard: the call without the bit, and the other outputs with it
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_the_unflagged_call_leaves_the_tail(ctx, monkeypatch, mode):
    """The same arrays without the bit: the matrix behind out_link_busy_ns keeps its pattern, and every
    output equals the flagged call's."""
    carry, drop, packets = mode
    c = OC.random_case(3)
    hdr = SR.header(0, 1, 1)  # (read by nobody)
    for form in FORMS:
        _form(monkeypatch, form)
        for dev in (True, False):
            start = SC.pattern((4, len(c["link_off"]) - 1, 3))
            rc, plain, M = _call(ctx, c, hdr, dev=dev, carry=carry, drop=drop, packets=packets, series=False, start=start)
            assert rc == 0 and np.array_equal(M, start)
            rc, flagged, M = _call(ctx, c, hdr, dev=dev, carry=carry, drop=drop, packets=packets, start=start)
            assert rc == 0 and not np.array_equal(M, start)
            for k in RAW:
                assert np.array_equal(plain[k], flagged[k]), k


# ---- 7. errors: codes, pairs, precedence, outputs untouched
@pytest.mark.parametrize("dev", (True, False), ids=("device", "host"))
def test_argument_errors(ctx, dev):
    c = OC.random_case(4)
    nl = len(c["link_off"]) - 1
    hdr = SR.header(1000, 10, 8)
    start = SC.pattern((4, nl, 10))

    def fails(code, pair=None, h=hdr, st=start, **kw):
        rc, outs, M = _call(ctx, c, h, dev=dev, start=st, **kw)
        assert rc == code and _untouched(outs, M, st), (rc, kw)
        assert pair is None or _pair(ctx) == pair

    # an output the pass reads is missing (a call without out_link_busy_ns has no matrix to look at)
    fails(INVALID_ARG, nullout=("wait",))
    fails(INVALID_ARG, nullout=("done",))
    assert _call(ctx, c, hdr, dev=dev, nullout=("busy",), start=start)[0] == INVALID_ARG
    fails(INVALID_ARG, carry=True, H=5000, nullout=("ahead",))
    fails(INVALID_ARG, h=SR.header(1000, 0, 8))
    fails(INVALID_ARG, h=SR.header(1000, 10, 0), st=np.zeros((4, nl, 2), np.uint64))
    # a count past the range; a zero comes before it, and a missing output before both
    fails(INVALID_ARG, h=SR.header(1000, 0, 8), nullout=("wait",))
    for h, code in ((np.array([0, 1, 1 << 32, 1] + [0] * nl, np.uint64), CAPACITY), (np.array([0, 1, 1, 1 << 32] + [0] * nl, np.uint64), CAPACITY),
                    (np.array([0, 1, (1 << 31) - 1, 2] + [0] * nl, np.uint64), CAPACITY), (np.array([0, 0, 1 << 32, 1] + [0] * nl, np.uint64), INVALID_ARG)):
        rc, outs, _ = _raw_header_call(ctx, c, h, dev)
        assert rc == code and QG._untouched(outs), (h[:4].tolist(), rc)
    # a bad slot: host mode finds it before anything runs; device mode after the call's own errors
    slots = [0, 9, SR.UNWATCHED, 1 << 40, 1, 0][:nl]
    hb = SR.header(1000, 10, 8, slots, 2)
    assert SR.bad_slot(hb, nl) == 1
    st2 = SC.pattern((4, 2, 10))
    if not dev:
        fails(INVALID_ARG, (1, 0xFFFFFFFF), h=hb, st=st2)
        # before link_off's check
        bad = dict(c, link_off=np.concatenate([[1], c["link_off"][1:]]).astype(np.uint64))
        rc, outs, M = _call(ctx, bad, hb, dev=False, start=st2)
        assert rc == INVALID_ARG and _pair(ctx) == (1, 0xFFFFFFFF)
    else:
        rc, outs, M = _call(ctx, c, hb, dev=True, start=st2)
        assert rc == INVALID_ARG and _pair(ctx) == (1, 0xFFFFFFFF)
        # treated as not watched: the other links' sums stand
        good = SR.header(1000, 10, 8, [0, SR.UNWATCHED, SR.UNWATCHED, SR.UNWATCHED, 1, 0][:nl], 2)
        assert np.array_equal(M, SC.matrix(c, SC.first_order_out(c), good, start=st2))
        # after the call's own errors: a packet index past the weights
        pk = c["packet"].copy()
        pk[7] = c["n_packets"] + 3
        rc, _, _ = _call(ctx, dict(c, packet=pk), hb, dev=True, start=st2)
        lk = int(np.searchsorted(c["link_off"], 7, side="right")) - 1
        assert rc == INVALID_ARG and _pair(ctx) == (lk, 7 - int(c["link_off"][lk]))
        for carry in (False, True):
            rc, _, _ = _call(ctx, dict(c, packet=pk), hb, dev=True, carry=carry, start=st2)
            assert rc == INVALID_ARG and _pair(ctx) == (lk, 7 - int(c["link_off"][lk]))
        rc, _, _ = _call(ctx, c, hb, dev=True, carry=True, drop=True, packets=True, H=MAX, start=st2)
        assert rc == INVALID_ARG and _pair(ctx) == (1, 0xFFFFFFFF)


def _raw_header_call(ctx, c, h, dev):
    """A call whose header cannot have a matrix: out_link_busy_ns has the per-link entries alone."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    nl = len(c["link_off"]) - 1
    outs = {k: np.full(_sizes(c, False, False)[k], QC.SENT32 if QR.DTYPES[k] == np.uint32 else QC.SENT64, QR.DTYPES[k]) for k in RAW}
    arrays = dict(c, cost_ps=np.concatenate([c["cost_ps"], h]))
    keep = []

    def ptr(a):
        if a is None:
            return None
        if not dev:
            keep.append(a)
            return C.c_void_p(a.ctypes.data)
        keep.append(torch.from_numpy(a.view(VIEW[a.dtype]).copy()).cuda())
        return C.c_void_p(keep[-1].data_ptr())

    ip = [ptr(arrays[k]) for k in INPUTS]
    k0 = len(keep)
    op = [ptr(outs[k]) for k in RAW]
    if dev:
        torch.cuda.synchronize()
    rc = _capi.load().sg_link_queue(ctx.handle, (_capi.SG_ROUTE_OUT_DEVICE if dev else 0) | SERIES, nl, ip[0], len(c["enter"]),
                                    ip[1], ip[2], ip[3], c["n_packets"], ip[4], ip[5], *op)
    if dev:
        torch.cuda.synchronize()
        for k, t in zip(RAW, keep[k0:]):
            outs[k][...] = t.cpu().numpy().view(outs[k].dtype)
    return rc, outs, None


# ---- 8. a non-blocking stream
def test_non_blocking_stream():
    """The flagged carried call with limits on a context whose stream is the caller's non-blocking stream
    S: inputs and the matrix reach the device on S behind a delay, so a launch, a memset or the
    header's read-back on any other stream would come before them."""
    import torch

    import stream_cases as STC
    from shadow_amd import Context, _capi

    C = _capi.C
    c = OC.with_base(DC.draw_limits(CC.random_chains(41, n_links=6, n_packets=700, hops=(1, 4), span=4000), 64, limits=(5, 20, 60)))
    want = SC.carried_out(c, MAX, True)
    hdr = SC.span_header(c, want, 2049, [0, 1, 2, SR.UNWATCHED, 1, 0], 3, margin=3)
    start = SC.pattern((4, 3, 2051))
    expect = SC.matrix(c, want, hdr, drop=True, start=start)
    arrays = dict(c, cost_ps=np.concatenate([c["cost_ps"], c["limit_ns"], hdr]))
    outs = {k: np.full(v, QC.SENT32 if QR.DTYPES[k] == np.uint32 else QC.SENT64, QR.DTYPES[k]) for k, v in _sizes(c, True, False).items()}
    outs["busy"] = np.concatenate([outs["busy"], start.ravel()])
    S = torch.cuda.Stream()
    sctx = Context(0, stream=S.cuda_stream)
    try:
        pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(VIEW[a.dtype]).copy()).pin_memory()  # noqa: E731
        h_in = [None if arrays[k] is None else pin(arrays[k]) for k in INPUTS]
        h_out = {k: pin(outs[k]) for k in RAW}
        with torch.cuda.stream(S):
            torch.cuda._sleep(STC.DELAY_CYCLES)
            d_in = [None if t is None else t.to("cuda", non_blocking=True) for t in h_in]
            d_out = {k: t.to("cuda", non_blocking=True) for k, t in h_out.items()}
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
            rc = _capi.load().sg_link_queue(sctx.handle, _capi.SG_ROUTE_OUT_DEVICE | CARRY | DROP | SERIES, 6, ptr(d_in[0]),
                                            len(c["enter"]), ptr(d_in[1]), ptr(d_in[2]), ptr(d_in[3]), c["n_packets"], ptr(d_in[4]),
                                            ptr(d_in[5]), *[ptr(d_out[k]) for k in RAW])
            for k in RAW:
                h_out[k].copy_(d_out[k], non_blocking=True)
            S.synchronize()
        _capi.check(sctx.handle, rc)
        got = h_out["busy"].numpy().view(np.uint64)
        assert np.array_equal(got[12:].reshape(4, 3, 2051), expect) and np.array_equal(got[:12], want["busy"])
        for k in RAW:
            if k != "busy":
                assert np.array_equal(h_out[k].numpy().view(outs[k].dtype), want[k]), k
    finally:
        S.synchronize()
        sctx.close()


# ---- 9. the Python surface over real traces
@pytest.fixture(scope="module")
def tie(ctx, oracle):
    r = OC.real_trace(oracle, "tie")
    net = _net(r["g"], ctx)
    return dict(r, net=net, tree=net.compute_shortest_path_tree())


def _series_for(ctx_or_net, c, closed, n_bins=48, **kw):
    from shadow_amd import LinkQueueSeries

    hdr = SC.span_header(c, closed, n_bins, margin=1)
    nl = len(c["link_off"]) - 1
    s = LinkQueueSeries(ctx_or_net, int(hdr[0]), int(hdr[1]), n_bins, **(dict(n_links=nl) if not hasattr(ctx_or_net, "links") else {}), **kw)
    return s, SR.header(int(hdr[0]), int(hdr[1]), n_bins, None if s.link_slot is None else s.link_slot.tolist(), s.n_slots)


def test_session_over_five_rounds_of_a_real_trace(ctx, oracle):
    """LinkQueueSession(series=) over the tie round cut into 5 rounds by send time, under the median limits,
    and flush(): the matrix of the single carried call, which shadow_amd.link_queue(series=) gives too."""
    import shadow_amd

    c = OC.real_trace(oracle, "tie")["case"]
    whole, rs = WC.rounds(c, 5, 7)
    closed = SC.carried_out(whole, MAX, True)
    nl = len(c["link_off"]) - 1
    watch = np.flatnonzero(np.diff(c["link_off"].astype(np.int64)) > 0)[::2]
    s, hdr = _series_for(ctx, whole, closed, watch=watch)
    sess = shadow_amd.LinkQueueSession(ctx, c["cost_ps"], c["limit_ns"], c["free_in"], n_links=nl, series=s)
    pend = []
    for rc, H, _, _ in rs:
        sess.advance(rc["link_off"], rc["enter"], rc["packet"], rc["weight"], rc["base"], H)
        pend.append(sess.pending)
    sess.flush()
    want = SC.matrix(whole, closed, hdr, drop=True)
    assert max(pend) > 0 and sess.pending == 0 and want[3].sum() > 0 and want[1].sum() > 0
    assert np.array_equal(s.planes(), want)
    s2, _ = _series_for(ctx, whole, closed, watch=watch)
    shadow_amd.link_queue(ctx, whole["link_off"], whole["enter"], whole["packet"], whole["weight"], cost_ps=whole["cost_ps"],
                          carry=True, limit_ns=whole["limit_ns"], series=s2)
    assert np.array_equal(s2.planes(), want)


def test_path_tree_round_tie(ctx, tie):
    """PathTree.link_queue_round(series=) on the tie round: first order, carried with limits and outcomes,
    and window by window; the result is the call's without the keyword."""
    t, c = tie["tree"], tie["case"]
    ht, pb = _host_table(tie["hosts"], ctx), _batch(tie["pk"])
    closed = SC.carried_out(c, MAX, True)
    kw = dict(cost_ps=QC.TIE_COST, limit_ns=c["limit_ns"], carry=True, outcomes=c["base"])
    plain = t.link_queue_round(ht, pb, tie["status"], "payload", **kw)
    s, hdr = _series_for(tie["net"], c, closed)
    got = t.link_queue_round(ht, pb, tie["status"], "payload", series=s, **kw)
    want = SC.matrix(c, closed, hdr, drop=True)
    assert np.array_equal(s.planes(), want) and want[3].sum() > 0
    assert type(got[5]) is type(plain[5])
    for f in got[5]._fields:
        assert np.array_equal(getattr(got[5], f), getattr(plain[5], f)), f
    nxt, _, gap, _ = WR._chains(c)
    s.reset()
    t.link_queue_round(ht, pb, tie["status"], "payload", series=s, window_ns=16 * min(g for g, k in zip(gap, nxt) if k != WR.NONE), **kw)
    assert np.array_equal(s.planes(), want)
    # first order, without limits, into the same cells
    s.reset()
    first = t.link_queue_round(ht, pb, tie["status"], "payload", cost_ps=QC.TIE_COST, series=s)
    fo = dict(wait=first[5].wait_ns, done=first[5].done_ns, ahead=first[5].ahead)
    assert np.array_equal(s.planes(), SC.matrix(c, fo, hdr)) and first[5].link_busy_ns.shape == (len(c["link_off"]) - 1,)


@pytest.mark.parametrize("name", ["k04", "k30"])
def test_path_tree_round_sweep(ctx, oracle, name):
    import sweep_cases as SWC

    w = SWC.case(name)
    pk, status = QC.sweep_round(w)
    net = _net(w["g"], ctx)
    t = net.compute_shortest_path_tree()
    nl = len(net.links()[0])
    cost = QC.sweep_costs(name, nl)
    ht, pb = _host_table(w["hosts"], ctx), _batch(pk)
    plain = t.link_queue_round(ht, pb, status, "payload", cost_ps=cost, carry=True)
    c = CC.case(plain[0], plain[3], plain[1], pk["payload"], cost)
    out = dict(wait=plain[5].wait_ns, done=plain[5].done_ns, ahead=plain[5].ahead)
    s, hdr = _series_for(net, c, out, n_bins=257)
    got = t.link_queue_round(ht, pb, status, "payload", cost_ps=cost, carry=True, series=s)
    assert np.array_equal(got[5].done_ns, plain[5].done_ns)
    M = s.planes()
    assert np.array_equal(M, SC.matrix(c, out, hdr))
    sums = SR.plane_sums(M)
    assert sums[0] == [int(x) for x in plain[5].link_busy_ns] and sums[1] == [int(x) for x in plain[5].link_wait_sum_ns]


@pytest.mark.parametrize("world", QC.GROUP_WORLDS)
def test_group_round(ctx, tie, world):
    """Group.link_queue_round(series=) over 1 and 3 members, on the root's device: the single call's matrix."""
    import group_trace_cases as GC
    from test_group_trace_gpu import members

    g, hosts, t = tie["g"], tie["hosts"], tie["tree"]
    parts = GC.split(hosts, tie["pk"], tie["status"], g["n"], world)
    cat, cstatus, _ = GC.concat(parts)
    single = t.link_queue_round(_host_table(hosts, ctx), _batch(cat), cstatus, "payload", cost_ps=QC.TIE_COST)
    c = CC.case(single[0], single[3], single[1], cat["payload"], np.full(len(single[0]) - 1, QC.TIE_COST, np.uint64))
    out = dict(wait=single[5].wait_ns, done=single[5].done_ns, ahead=single[5].ahead)
    s1, hdr = _series_for(tie["net"], c, out)
    t.link_queue_round(_host_table(hosts, ctx), _batch(cat), cstatus, "payload", cost_ps=QC.TIE_COST, series=s1)
    want = SC.matrix(c, out, hdr)
    assert np.array_equal(s1.planes(), want) and want[1].sum() > 0
    with members(world) as (ctxs, group, keep):
        graphs = [keep(_net(g, cx)) for cx in ctxs]
        hts = [keep(_host_table(hosts, cx)) for cx in ctxs]
        s, _ = _series_for(graphs[world - 1], c, out)
        got = group.link_queue_round(graphs, hts, t, [_batch(p[0]) for p in parts], [p[1] for p in parts], "payload",
                                     cost_ps=QC.TIE_COST, root=world - 1, series=s)
        assert np.array_equal(got[6].done_ns, single[5].done_ns) and np.array_equal(s.planes(), want)


def test_link_queue_device_series(ctx, tie):
    """NetworkGraph.link_queue_device(series=): the caller's busy array receives the per-link values."""
    import torch

    c = tie["case"]
    want = SC.carried_out(c, MAX, True)
    s, hdr = _series_for(tie["net"], c, want)
    nl = len(c["link_off"]) - 1
    up = lambda a: torch.from_numpy(a.view(VIEW[a.dtype]).copy()).cuda()  # noqa: E731
    d = {k: up(c[k]) for k in ("link_off", "enter", "packet", "weight", "cost_ps")}
    outs = {k: up(np.full(v, QC.SENT32 if QR.DTYPES[k] == np.uint32 else QC.SENT64, QR.DTYPES[k])) for k, v in _sizes(c, True, False).items()}
    torch.cuda.synchronize()
    tie["net"].link_queue_device(d["link_off"].data_ptr(), len(c["packet"]), d["enter"].data_ptr(), d["packet"].data_ptr(),
                                 d["weight"].data_ptr(), c["n_packets"], d["cost_ps"].data_ptr(), 0,
                                 **{k + "_ptr": outs[k].data_ptr() for k in RAW}, carry=True, limit_ns=c["limit_ns"], series=s)
    torch.cuda.synchronize()
    for k in RAW:
        assert np.array_equal(outs[k].cpu().numpy().view(want[k].dtype), want[k]), k
    assert np.array_equal(s.planes(), SC.matrix(c, want, hdr, drop=True)) and nl
