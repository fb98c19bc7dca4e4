"""The link time series on the GPU (sg_link_series_packets, NetworkGraph.link_series_packets_device,
PathTree.link_series_round).

As in test_trace_gpu.py, the pred and latency rows the library reads come from
sg_routing_build_tree on the same net; the reference (tests/series_ref.py) bins the crossings of
tests/trace_ref.py with Python integers and one np.add.at per array.  Every output starts from
non-zero base values, so that "added to" and "nothing else written" are both checked; every
comparison is exact (np.array_equal).  The inputs' own conditions are checked on the CPU in
test_series_ref_cpu.py.  Which form a call took is read from read_timer("link_series_lds")."""
import numpy as np
import pytest

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import series_cases as SC
import series_ref as SR
import sweep_cases as WC
import trace_cases as XC
import trace_ref as XR

pytestmark = pytest.mark.gpu

UMAX = 0xFFFFFFFF
VIEW = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
LDS_MAX = 8064  # the knob's largest value
ATS = (SR.AT_ENTER, SR.AT_EXIT)


def _net(g, ctx):
    from shadow_amd import NetworkGraph

    return NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)


def _tabs(net, nodes, r0, r1):
    """(pred, latency) rows [r0, r1) from sg_routing_build_tree (host outputs)."""
    from shadow_amd import _capi

    nodes = np.ascontiguousarray(nodes, np.uint32)
    n, k = len(nodes), r1 - r0
    lat, loss = np.zeros((k, n), np.uint64), np.zeros((k, n), np.float32)
    pred, hop = np.zeros((k, n), np.uint32), np.zeros((k, n), np.uint32)
    _capi.check(net.ctx.handle, _capi.load().sg_routing_build_tree(
        net.ctx.handle, net._ensure_net(), nodes.ctypes.data, n, r0, r1, _capi.SG_ROUTE_SHORTEST_PATH,
        lat.ctypes.data, loss.ctypes.data, pred.ctypes.data, hop.ctypes.data))
    return pred, lat


def _oracle_lat(O, g, nodes, r0, r1):
    rc, lat, _, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                     np.asarray(nodes, np.uint32), rows=(r0, r1), threads=8)
    assert rc == 0
    return lat


def _host_table(hosts, ctx):
    from shadow_amd.worker import HostTable

    return HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)


def _batch(pk):
    from shadow_amd.worker import PacketBatch

    n = len(pk["src"])
    return PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk.get("payload", np.zeros(n, np.uint32)), pk["send_time"])


def _dev(x):
    import torch

    if x is None:
        return None
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(VIEW[x.dtype]).copy()).cuda()


def _call(net, nodes, r0, r1, tabs, ht, pb, outs, *, status=None, weight=None, slot=None, n_slots, at=0, t0=0, bin_ns=1,
          n_bins=1, dev=False, n_nodes=None):
    """One call on numpy arrays: host-array mode, or (dev) pred, latency, the slot map and the
    outputs uploaded, SG_ROUTE_OUT_DEVICE, and the outputs copied back into `outs` = [series or
    None, outside or None].  status and weight are numpy arrays or None.  Returns the status code."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    nodes = np.ascontiguousarray(nodes, np.uint32)
    ins = [None if t is None else np.ascontiguousarray(t, dt) for t, dt in zip(tabs, (np.uint32, np.uint64))]
    ins.append(None if slot is None else np.ascontiguousarray(slot, np.uint32))
    d_status, d_weight = _dev(status), _dev(None if weight is None else np.asarray(weight, np.uint32))
    if dev:
        d_ins = [_dev(t) for t in ins]
        d_outs = [_dev(o) for o in outs]
        ip = [None if t is None else C.c_void_p(t.data_ptr()) for t in d_ins]
        op = [None if o is None else C.c_void_p(o.data_ptr()) for o in d_outs]
    else:
        ip = [None if t is None else t.ctypes.data for t in ins]
        op = [None if o is None else o.ctypes.data for o in outs]
    p = pb.c_struct()
    rc = _capi.load().sg_link_series_packets(
        net.ctx.handle, net._ensure_net(), ht.handle, nodes.ctypes.data, len(nodes) if n_nodes is None else n_nodes, r0, r1,
        _capi.SG_ROUTE_OUT_DEVICE if dev else 0, ip[0], ip[1], C.byref(p),
        None if d_status is None else C.c_void_p(d_status.data_ptr()),
        None if d_weight is None else C.c_void_p(d_weight.data_ptr()), ip[2], int(n_slots), int(at), int(t0), int(bin_ns),
        int(n_bins), op[0], op[1])
    if dev:
        torch.cuda.synchronize()
        for o, d in zip(outs, d_outs):
            if o is not None:
                o[...] = d.cpu().numpy().view(np.uint64).reshape(o.shape)
    return rc


def _error(ctx):
    from shadow_amd import _capi

    r, k = _capi.C.c_uint32(), _capi.C.c_uint32()
    _capi.load().sg_ctx_last_error_pair(ctx.handle, _capi.C.byref(r), _capi.C.byref(k))
    return (r.value, k.value), _capi.load().sg_ctx_last_error(ctx.handle).decode()


def _untouched(outs):
    return all(o is None or (o == (SC.BASE_SERIES if k == 0 else SC.BASE_OUTSIDE)).all() for k, o in enumerate(outs))


def _check(net, nodes, rows, tabs, ht, pb, cross, *, slot=None, n_slots, at, t0, bin_ns, n_bins, outside=True, **kw):
    """One call from the base values against the reference binned from `cross` (series_ref.crossings).
    Returns the sums without the base."""
    from shadow_amd import _capi

    base = SC.bases(n_slots, n_bins)
    want = SR.bin_crossings(cross, slot, n_slots, at, t0, bin_ns, n_bins, base)
    outs = [base[0].copy(), base[1].copy() if outside else None]
    rc = _call(net, nodes, rows[0], rows[1], tabs, ht, pb, outs, slot=slot, n_slots=n_slots, at=at, t0=t0, bin_ns=bin_ns,
               n_bins=n_bins, **kw)
    _capi.check(net.ctx.handle, rc)
    assert np.array_equal(outs[0], want[0]), f"series differs in {int((outs[0] != want[0]).sum())} of {want[0].size} cells"
    if outside:
        assert np.array_equal(outs[1], want[1]), f"outside differs in {int((outs[1] != want[1]).sum())} cells"
    return outs[0] - SC.BASE_SERIES, want[1] - SC.BASE_OUTSIDE


def _form(ctx):
    """(1 when the last call took the LDS form, its cells); timers on."""
    _, lds, cells = ctx.read_timer("link_series_lds")
    return int(lds), int(cells)


@pytest.fixture(scope="module")
def tie(ctx, oracle):
    """The tie graph's net, its rows from the library and the oracle's latencies, the tie round
    with its own statuses (the oracle's delivery round), and the crossings of each (status, weight)."""
    g = LC.tie_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    net = _net(g, ctx)
    hosts, pk, mixed = XC.tie_round()
    tabs = _tabs(net, nodes, 0, g["n"])
    rc, olat, oloss, _ = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                               rows=(0, g["n"]), threads=8)
    assert rc == 0 and np.array_equal(tabs[1], olat)
    rng = np.stack([oracle.xoshiro_seed(int(s)) for s in hosts["seed"]])
    own = oracle.deliver_round(RC.ROUND_END, 2**63, 0, pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"],
                               hosts["ip"], hosts["route"], olat, oloss, rng, np.zeros(hosts["n"], np.uint64))["status"]
    assert 0 < int((own == 0).sum()) < len(own)
    big = RC.big_weights(len(pk["src"]))
    combos = {"plain": (None, None), "own": (own, pk["payload"]), "mixed": (mixed, big)}
    cross = {k: SR.crossings(g, nodes, (0, 300), tabs[0], olat, hosts, pk, s, w) for k, (s, w) in combos.items()}
    tail, head, _ = LR.links(g)
    return dict(g=g, nodes=nodes, net=net, tabs=tabs, olat=olat, hosts=hosts, pk=pk, mixed=mixed, combos=combos, cross=cross,
                ht=_host_table(hosts, ctx), pb=_batch(pk), n_links=XR.n_links(g), tail=tail, head=head)


def _tie_check(t, combo, **kw):
    status, weight = t["combos"][combo]
    return _check(t["net"], t["nodes"], (0, 300), t["tabs"], t["ht"], t["pb"], t["cross"][combo], status=status,
                  weight=weight, **kw)


def _head(pk, n):
    return {k: v[:n] for k, v in pk.items()}


# ---- 1. the tie round
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_tie_round(ctx, tie, dev):
    """The three bin sets, both `at` values; no statuses, the round's own with payload weights,
    mixed ones with weights up to 2^32 - 1 (cells pass 2^32: an LDS add done in halves would lose
    the carry); a list of 16 links (the LDS form) and the identity (the global form); the identity
    with sg_link_load_packets on the device; the counted-packets timer."""
    import torch

    nl = tie["n_links"]
    load = XR.trace(tie["g"], tie["nodes"], (0, 300), tie["tabs"][0], tie["olat"], tie["hosts"], tie["pk"])[0]
    busiest = np.argsort(np.diff(load.astype(np.int64)))[-16:]
    some = SR.list_slots(tie["g"], busiest)
    dpred = _dev(tie["tabs"][0])
    ctx.enable_timers(True)
    try:
        for combo, (status, weight) in tie["combos"].items():
            dload = torch.zeros(nl, dtype=torch.int64, device="cuda")
            ds, dw = _dev(status), _dev(weight)  # (held until the call has run)
            tie["net"].link_load_packets_device(tie["ht"], tie["nodes"], 0, 300, dpred.data_ptr(), tie["pb"],
                                                0 if ds is None else ds.data_ptr(), 0 if dw is None else dw.data_ptr(),
                                                dload.data_ptr(), 0, 0)
            torch.cuda.synchronize()
            loads = dload.cpu().numpy().view(np.uint64)
            counted = len(tie["pk"]["src"]) if status is None else int((status == 0).sum())
            for (bin_ns, n_bins) in SC.BIN_SETS:
                for at in ATS:
                    for (slot, ns), lds in ((some, 1), ((None, nl), 0)):
                        ctx.enable_timers(True)  # (resets them)
                        got = _tie_check(tie, combo, slot=slot, n_slots=ns, at=at, t0=SC.TIE_T0, bin_ns=bin_ns,
                                         n_bins=n_bins, dev=dev)
                        assert _form(ctx) == (lds, ns * (n_bins + 2))
                        assert np.array_equal(SR.slot_totals(*got), SR.slot_loads(loads, slot, ns))
                        _, launches, work = ctx.read_timer("link_series")
                        assert launches == 1 and int(work) == counted
                        assert int(ctx.read_timer("link_series_counted")[1]) == counted
                        if combo == "mixed" and slot is not None:
                            assert int(got[0].max()) >= 1 << 32
    finally:
        ctx.enable_timers(False)


# ---- 2. both forms
def test_both_forms(ctx, tie, monkeypatch):
    """Every bin set of the tie round under SG_LINK_SERIES_LDS=0 and under a budget that admits
    it: equal, and equal to the reference.  A budget of 64 cells with shapes of 63, 64 and 65
    cells.  The identity (2,080 x 64 cells) takes the global form under any budget."""
    busiest = np.arange(100, 116)
    some = SR.list_slots(tie["g"], busiest)
    ctx.enable_timers(True)
    try:
        for (bin_ns, n_bins) in SC.BIN_SETS:
            got = {}
            for budget, lds in (("0", 0), (str(LDS_MAX), 1)):
                monkeypatch.setenv("SG_LINK_SERIES_LDS", budget)
                got[lds] = [_tie_check(tie, "mixed", slot=some[0], n_slots=16, at=at, t0=SC.TIE_T0, bin_ns=bin_ns,
                                       n_bins=n_bins, dev=True) for at in ATS]
                assert _form(ctx) == (lds, 16 * (n_bins + 2))
            for a, b in zip(got[0], got[1]):
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        monkeypatch.setenv("SG_LINK_SERIES_LDS", str(SC.SMALL_BUDGET))
        for (ns, n_bins), lds in zip(SC.BUDGET_SHAPES, (1, 1, 0)):
            slot = SR.list_slots(tie["g"], busiest[:ns])[0]
            _tie_check(tie, "own", slot=slot, n_slots=ns, at=SR.AT_ENTER, t0=SC.TIE_T0, bin_ns=12 * SC.MS // n_bins,
                       n_bins=n_bins, dev=True)
            assert _form(ctx) == (lds, ns * (n_bins + 2))
        assert tie["n_links"] == 2080
        for budget in ("0", str(LDS_MAX), None):
            if budget is None:
                monkeypatch.delenv("SG_LINK_SERIES_LDS")
            else:
                monkeypatch.setenv("SG_LINK_SERIES_LDS", budget)
            _tie_check(tie, "own", n_slots=2080, at=SR.AT_EXIT, t0=SC.TIE_T0, bin_ns=250_000, n_bins=64, dev=True)
            assert _form(ctx) == (0, 2080 * 66)
    finally:
        ctx.enable_timers(False)


# ---- 3. quotient edges
@pytest.fixture(scope="module")
def tier(ctx, oracle):
    g = XC.tier_graph()
    net = _net(g, ctx)
    nodes = np.arange(3, dtype=np.uint32)
    tabs = _tabs(net, nodes, 0, 1)
    olat = _oracle_lat(oracle, g, nodes, 0, 1)
    _, _, keys = LR.links(g)
    l01, l12 = (int(LR.link_index(keys, [u], [v])[0]) for u, v in ((0, 1), (1, 2)))
    shared = np.full(XR.n_links(g), UMAX, np.uint32)
    shared[[l01, l12]] = 0
    return dict(g=g, net=net, nodes=nodes, tabs=tabs, olat=olat, n_links=XR.n_links(g), l01=l01, l12=l12, shared=shared)


def _tier_check(ctx, t, hosts, pk, monkeypatch, **kw):
    """The identity (global form) and both links in one slot under the largest budget (LDS form)."""
    ht, pb = _host_table(hosts, ctx), _batch(pk)
    cross = SR.crossings(t["g"], t["nodes"], (0, 1), t["tabs"][0], t["olat"], hosts, pk, None, pk["payload"])
    out = []
    for at in ATS:
        monkeypatch.setenv("SG_LINK_SERIES_LDS", "0")
        out.append(_check(t["net"], t["nodes"], (0, 1), t["tabs"], ht, pb, cross, weight=pk["payload"], n_slots=t["n_links"],
                          at=at, dev=True, **kw))
        assert _form(ctx)[0] == 0
        monkeypatch.setenv("SG_LINK_SERIES_LDS", str(LDS_MAX))
        out.append(_check(t["net"], t["nodes"], (0, 1), t["tabs"], ht, pb, cross, weight=pk["payload"], slot=t["shared"],
                          n_slots=1, at=at, dev=True, **kw))
        assert _form(ctx)[0] == (1 if kw["n_bins"] + 2 <= LDS_MAX else 0)
    return out


@pytest.mark.parametrize("bin_ns", SC.EDGE_BINS)
def test_quotient_edges(ctx, tier, monkeypatch, bin_ns):
    """Crossings whose t - t0 is one below and at the lower edge of bins 1, 2, 63, 64, the last
    and the one past it; t0 - 1; 2^32 bins and k more (a quotient truncated to 32 bits would land
    in bin k: the right answer is "after"); 2^63 + 5.  4,096 bins; a divisor of 1, 3, 333,333,
    2^20 and 2^32 + 1."""
    xs = SC.edge_offsets(bin_ns)
    hosts, pk = SC.edge_round(xs)
    ctx.enable_timers(True)
    try:
        out = _tier_check(ctx, tier, hosts, pk, monkeypatch, t0=SC.EDGE_T0, bin_ns=bin_ns, n_bins=SC.EDGE_N_BINS)
    finally:
        ctx.enable_timers(False)
    # at enter, link (0, 1): t - t0 = the offsets themselves
    series, outside = out[0]
    row, n_bins = series[tier["l01"]], SC.EDGE_N_BINS
    weight = lambda cond: sum(k + 1 for k, x in enumerate(xs) if cond(x))  # noqa: E731  (packet k weighs k + 1)
    assert int(outside[tier["l01"], 0]) == weight(lambda x: x < 0) > 0
    assert int(outside[tier["l01"], 1]) == weight(lambda x: x >= 0 and x // bin_ns >= n_bins) > 0
    for b in (1, 2, 63, 64, n_bins - 1):
        assert int(row[b]) == weight(lambda x: x >= 0 and x // bin_ns == b) > 0


@pytest.mark.parametrize("bin_ns,n_bins", SC.PAST_BINS)
def test_bins_past_2_64(ctx, tier, monkeypatch, bin_ns, n_bins):
    """t0 + n_bins bin_ns passes 2^64: decided by the quotient, every crossing from t0 on lies
    inside; the last packet arrives at 2^64 - 1."""
    hosts, pk = SC.edge_round(list(SC.PAST_OFFSETS), SC.PAST_T0)
    ctx.enable_timers(True)
    try:
        out = _tier_check(ctx, tier, hosts, pk, monkeypatch, t0=SC.PAST_T0, bin_ns=bin_ns, n_bins=n_bins)
    finally:
        ctx.enable_timers(False)
    for series, outside in out:
        assert not outside[:, 1].any() and int(outside[:, 0].sum()) in (0, 1)  # (packet 0 enters link (0, 1) at t0 - 1)


# ---- 4. the hot cell
@pytest.mark.parametrize("n", [1, 64, 65, 2049, 100_000])
def test_hot_cell(ctx, tier, monkeypatch, n):
    """n packets at one send time: every crossing of a link in one cell, both forms."""
    hosts, pk = XC.tier_round(n, False)
    pk["payload"] = np.full(n, 0xFFFFFFF0, np.uint32)
    ctx.enable_timers(True)
    try:
        out = _tier_check(ctx, tier, hosts, pk, monkeypatch, t0=SC.T0 - 5, bin_ns=SC.MS, n_bins=64)
    finally:
        ctx.enable_timers(False)
    assert int(out[0][0][tier["l01"], 0]) == n * 0xFFFFFFF0 and int(out[1][0][0, 1]) == n * 0xFFFFFFF0


def test_star_hot_link(ctx, oracle, monkeypatch):
    """The 512-spoke star, 3,000 packets from one spoke: its link to the hub takes nearly all."""
    g = LC.star_graph(512)
    net = _net(g, ctx)
    nodes = np.arange(g["n"], dtype=np.uint32)
    hosts, pk = RC.star_round()
    tabs = _tabs(net, nodes, 0, 8)
    cross = SR.crossings(g, nodes, (0, 8), tabs[0], _oracle_lat(oracle, g, nodes, 0, 8), hosts, pk, None, pk["payload"])
    t0, bin_ns = SC.enter_range_bins(cross[2], 32)
    ht, pb = _host_table(hosts, ctx), _batch(pk)
    hot = int(np.bincount(cross[0]).argmax())
    assert int((cross[0] == hot).sum()) > 2048
    for budget in ("0", str(LDS_MAX)):
        monkeypatch.setenv("SG_LINK_SERIES_LDS", budget)
        for dev in (False, True):
            _check(net, nodes, (0, 8), tabs, ht, pb, cross, weight=pk["payload"], n_slots=XR.n_links(g), at=0, t0=t0,
                   bin_ns=bin_ns, n_bins=32, dev=dev)
            slot = SR.list_slots(g, [hot, (hot + 1) % XR.n_links(g), (hot + 2) % XR.n_links(g)])
            _check(net, nodes, (0, 8), tabs, ht, pb, cross, weight=pk["payload"], slot=slot[0], n_slots=3, at=1, t0=t0,
                   bin_ns=bin_ns, n_bins=32, dev=dev)


# ---- 5. slots
def test_slots(ctx, tie):
    """Both directions of every undirected edge in one slot; a list of five links; nothing
    watched adds nothing, and a corrupted crossed pred cell is still reported; a slot value >=
    n_slots in host mode (an argument error, the outputs untouched) and in device mode (its pair,
    ahead of a bad packet of the same call)."""
    from shadow_amd import _capi

    net, nodes, tabs, nl = tie["net"], tie["nodes"], tie["tabs"], tie["n_links"]
    both, ns = SC.both_directions(tie["tail"], tie["head"])
    assert ns < nl
    kw = dict(at=SR.AT_ENTER, t0=SC.TIE_T0, bin_ns=SC.MS, n_bins=8)
    for dev in (False, True):
        _tie_check(tie, "own", slot=both, n_slots=ns, dev=dev, **kw)
        five = SR.list_slots(tie["g"], [5, 17, 400, 401, nl - 1])
        _tie_check(tie, "own", slot=five[0], n_slots=5, dev=dev, **kw)
        none = np.full(nl, UMAX, np.uint32)
        got = _tie_check(tie, "own", slot=none, n_slots=3, dev=dev, **kw)
        assert not got[0].any() and not got[1].any()
    # a walked (pred, node) pair that is not a link, no link watched
    pk = _head(tie["pk"], 4000)
    pb = _batch(pk)
    pred = tabs[0]
    _, _, keys = LR.links(tie["g"])
    _, ri, cj = RR.counted_pairs(tie["hosts"], pk, None)
    k = int(np.flatnonzero((ri != cj) & (pred[ri, cj] != ri))[0])
    i, j = int(ri[k]), int(cj[k])
    p = pred.copy()
    p[i, j] = next(x for x in range(300) if x != j and LR.link_index(keys, [x], [j])[0] < 0)
    want = RR.first_bad_pred(tie["g"], nodes, (0, 300), p, tie["hosts"], pk)
    assert want is not None and want[0] == i
    outs = list(SC.bases(3, 8))
    rc = _call(net, nodes, 0, 300, (p, tabs[1]), tie["ht"], pb, outs, slot=none, n_slots=3, **kw)
    pair, msg = _error(ctx)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and "link" in msg, (pair, want, msg)
    # a bad slot value
    bad = five[0].copy()
    bad[[900, 33]] = 5, 77
    outs = list(SC.bases(5, 8))
    rc = _call(net, nodes, 0, 300, tabs, tie["ht"], pb, outs, slot=bad, n_slots=5, **kw)
    pair, msg = _error(ctx)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == (33, UMAX) and "link_slot[33]" in msg and _untouched(outs), (pair, msg)
    wrong = dict(pk, src=pk["src"].copy())
    wrong["src"][7] = tie["hosts"]["n"]  # a source host out of range
    for slot, first in ((bad, (33, UMAX)), (five[0], (7, UMAX))):
        rc = _call(net, nodes, 0, 300, tabs, tie["ht"], _batch(wrong), list(SC.bases(5, 8)), slot=slot, n_slots=5, dev=True, **kw)
        pair, msg = _error(ctx)
        assert rc == _capi.SG_ERR_INVALID_ARG and pair == first, (pair, first, msg)
    _tie_check(tie, "own", slot=five[0], n_slots=5, dev=True, **kw)  # and the context still works


# ---- 6. accumulation
def test_accumulation(ctx, tie, oracle):
    """A shuffled node order, rows [0, 60) and [60, 120) in two calls with their halves of the
    batch into one matrix; then the same round again: twice the sums."""
    from shadow_amd import _capi

    g, net = tie["g"], tie["net"]
    nodes, hosts, lo, hi = RC.shuffled_round()
    ht = _host_table(hosts, ctx)
    nl = tie["n_links"]
    kw = dict(n_slots=nl, at=SR.AT_EXIT, t0=SC.T0, bin_ns=700_000, n_bins=12)
    for dev in (False, True):
        want = SC.bases(nl, 12)
        outs = [want[0].copy(), want[1].copy()]
        first = None
        for again in range(2):
            if again:
                first = outs[0] - SC.BASE_SERIES
            for (r0, r1), pk in (((0, 60), lo), ((60, 120), hi)):
                tabs = _tabs(net, nodes, r0, r1)
                want = SR.series(g, nodes, (r0, r1), tabs[0], _oracle_lat(oracle, g, nodes, r0, r1), hosts, pk, None,
                                 pk["payload"], base=want, **kw)
                _capi.check(ctx.handle, _call(net, nodes, r0, r1, tabs, ht, _batch(pk), outs, weight=pk["payload"], dev=dev, **kw))
                assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[1])
        assert first.any() and np.array_equal(outs[0] - SC.BASE_SERIES, 2 * first)


# ---- 7. wider inputs
def test_wide_cells_and_overflow(ctx, oracle):
    """Latencies past 2^32 ns and times on both sides of 2^32, 1 s bins; a counted packet whose
    arrival passes 2^64 - 1 is SG_ERR_TIME_OVERFLOW with its index, the smallest such; one at
    2^64 - 1 exactly is not; the same packet not counted is no error."""
    from shadow_amd import _capi

    g = XC.wide_graph()
    n = g["n"]
    net = _net(g, ctx)
    nodes = np.arange(n, dtype=np.uint32)
    tabs = _tabs(net, nodes, 0, n)
    olat = _oracle_lat(oracle, g, nodes, 0, n)
    hosts, pk = XC.wide_round()
    ht = _host_table(hosts, ctx)
    nl = XR.n_links(g)
    kw = dict(n_slots=nl, t0=1 << 30, bin_ns=10**9, n_bins=48)
    for dev in (False, True):
        for at in ATS:
            cross = SR.crossings(g, nodes, (0, n), tabs[0], olat, hosts, pk, None, pk["payload"])
            got = _check(net, nodes, (0, n), tabs, ht, _batch(pk), cross, weight=pk["payload"], at=at, dev=dev, **kw)
            # (an exit is an arc of 1 s or more past the send: none lies before t0)
            assert got[0].any() and got[1][:, 0].any() == (at == SR.AT_ENTER) and got[1][:, 1].any()
    _, ri, cj = RR.counted_pairs(hosts, pk, None)
    cell = olat[ri, cj].astype(object)
    late = dict(pk, send_time=pk["send_time"].copy())
    late["send_time"][700] = np.uint64((1 << 64) - 1 - int(cell[700]))  # arrives at 2^64 - 1
    assert XR.first_overflow(nodes, (0, n), olat, hosts, late) is None
    cross = SR.crossings(g, nodes, (0, n), tabs[0], olat, hosts, late)
    assert max(cross[3]) == (1 << 64) - 1
    _check(net, nodes, (0, n), tabs, ht, _batch(late), cross, at=SR.AT_EXIT, dev=True, **kw)
    for q in (2000, 1300):
        late["send_time"][q] = np.uint64((1 << 64) - int(cell[q]))  # one past it
    for status, first in ((None, 1300), (np.where(np.arange(len(ri)) == 1300, RC.DROP_LOSS, 0).astype(np.uint8), 2000)):
        assert XR.first_overflow(nodes, (0, n), olat, hosts, late, status) == first
        rc = _call(net, nodes, 0, n, tabs, ht, _batch(late), list(SC.bases(nl, 48)), status=status, at=0, dev=True, **kw)
        pair, msg = _error(ctx)
        assert rc == _capi.SG_ERR_TIME_OVERFLOW and pair == (first, UMAX) and f"packet {first} " in msg, (rc, pair, msg)
    status = np.where(np.isin(np.arange(len(ri)), (1300, 2000)), RC.SIM_END, 0).astype(np.uint8)
    cross = SR.crossings(g, nodes, (0, n), tabs[0], olat, hosts, late, status)
    _check(net, nodes, (0, n), tabs, ht, _batch(late), cross, status=status, at=SR.AT_ENTER, dev=True, **kw)


@pytest.mark.parametrize("which", ["directed", "multi"])
def test_directed_and_multigraph(ctx, oracle, which):
    """Packets to the sender's own node cross its self-loop link: enter = the send time, exit =
    the send time plus the diagonal cell; a general batch beside them; parallel edges are one link."""
    g = LC.directed_graph() if which == "directed" else LC.multi_graph()
    n = g["n"]
    net = _net(g, ctx)
    nodes = np.arange(n, dtype=np.uint32)
    tabs = _tabs(net, nodes, 0, n)
    olat = _oracle_lat(oracle, g, nodes, 0, n)
    hosts, pk = RC.same_node_round(n)
    ht = _host_table(hosts, ctx)
    nl = XR.n_links(g)
    cross = SR.crossings(g, nodes, (0, n), tabs[0], olat, hosts, pk, None, pk["payload"])
    tail, head = net.links()
    assert len(cross[0]) == 2 * n and (tail[cross[0]] == head[cross[0]]).all()
    diag = int(olat.diagonal().min())
    for at in ATS:
        got = _check(net, nodes, (0, n), tabs, ht, _batch(pk), cross, weight=pk["payload"], n_slots=nl, at=at, t0=RC.T0,
                     bin_ns=diag, n_bins=2)
        # at enter every crossing lies in bin 0; its exit is a diagonal cell later, at least one bin
        assert got[0].any() and not got[0][:, 1 - at].any()
    pk2 = RC.batch(3000, hosts, 47)
    cross = SR.crossings(g, nodes, (0, n), tabs[0], olat, hosts, pk2, None, pk2["payload"])
    t0, bin_ns = SC.enter_range_bins(cross[2], 16)
    _check(net, nodes, (0, n), tabs, ht, _batch(pk2), cross, weight=pk2["payload"], n_slots=nl, at=0, t0=t0, bin_ns=bin_ns,
           n_bins=16, dev=True)


def test_sparse_addresses(ctx, tie):
    """The sorted address table resolves; packets to unknown addresses cross nothing."""
    hosts, pk, status = RC.sparse_address_round()
    cross = SR.crossings(tie["g"], tie["nodes"], (0, 300), tie["tabs"][0], tie["olat"], hosts, pk, status, pk["payload"])
    _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], _host_table(hosts, ctx), _batch(pk), cross, status=status,
           weight=pk["payload"], n_slots=tie["n_links"], at=SR.AT_EXIT, t0=SC.TIE_T0, bin_ns=SC.MS, n_bins=8)


# ---- 8. errors
def test_corrupted_pred(ctx, tie):
    """A 2-cycle, a value >= n and a non-link on a walked path, each with its (row, col), link
    loads' precedence (the smallest in row-major order whatever the kind); the same corruption in
    an unwalked cell succeeds."""
    from shadow_amd import _capi

    g, net, nodes, hosts = tie["g"], tie["net"], tie["nodes"], tie["hosts"]
    n, nl = g["n"], tie["n_links"]
    pred, lat = tie["tabs"]
    pk = _head(tie["pk"], 3000)
    pb = _batch(pk)
    _, _, keys = LR.links(g)
    _, ri, cj = RR.counted_pairs(hosts, pk, None)
    k = int(np.flatnonzero((ri != cj) & (pred[ri, cj] != ri))[0])
    i, j = int(ri[k]), int(cj[k])
    kw = dict(n_slots=nl, at=SR.AT_ENTER, t0=SC.TIE_T0, bin_ns=SC.MS, n_bins=8)

    def run(p, dev=False):
        rc = _call(net, nodes, 0, n, (p, lat), tie["ht"], pb, list(SC.bases(nl, 8)), dev=dev, **kw)
        return (rc,) + _error(ctx)

    def above(row, x):  # the nodes from x up to the row's source
        seen = [x]
        while seen[-1] != row:
            seen.append(int(pred[row, seen[-1]]))
        return seen

    cases = []
    p = pred.copy()  # a 2-cycle on that packet's path
    p[i, int(p[i, j])] = j
    cases.append((p, "cycle"))
    p = pred.copy()  # a value >= n
    p[i, j] = n
    cases.append((p, "range"))
    p = pred.copy()  # a pair that is not a link
    p[i, j] = next(x for x in range(n) if x != j and LR.link_index(keys, [x], [j])[0] < 0 and j not in above(i, x))
    cases.append((p, "link"))
    for p, word in cases:
        want = RR.first_bad_pred(g, nodes, (0, n), p, hosts, pk)
        assert want is not None and want[0] == i
        for dev in (False, True):
            rc, pair, msg = run(p, dev)
            assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and word in msg, (word, pair, want, msg)
    # precedence: a non-link in an earlier row wins over a value >= n in a later one
    later = int(np.flatnonzero((ri > i) & (ri != cj))[0])
    p = cases[2][0].copy()
    p[int(ri[later]), int(cj[later])] = n + 5
    want = RR.first_bad_pred(g, nodes, (0, n), p, hosts, pk)
    assert want == RR.first_bad_pred(g, nodes, (0, n), cases[2][0], hosts, pk) and want[0] == i
    rc, pair, msg = run(p)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and "link" in msg, (pair, want, msg)
    # the same corruption in a cell no path crosses succeeds
    crossed = np.zeros(n, bool)
    for c in cj[ri == i].tolist():
        if c != i:
            crossed[above(i, c)] = True
    free = int(np.flatnonzero(~crossed)[0])
    assert free != i
    for bad in (n, next(x for x in range(n) if x != free and LR.link_index(keys, [x], [free])[0] < 0)):
        p = pred.copy()
        p[i, free] = bad
        assert RR.first_bad_pred(g, nodes, (0, n), p, hosts, pk) is None
        assert run(p)[0] == _capi.SG_OK


def test_packet_and_argument_errors(ctx, tie):
    """Packet errors report their index; every argument error leaves the base values."""
    from shadow_amd import _capi

    g, net, nodes, hosts, ht = tie["g"], tie["net"], tie["nodes"], tie["hosts"], tie["ht"]
    n, nl = g["n"], tie["n_links"]
    pred, lat = tie["tabs"]
    base = {k: v[:2000].copy() for k, v in tie["pk"].items()}
    st = np.zeros(2000, np.uint8)
    st[700] = RC.DROP_NO_DST
    kw = dict(n_slots=nl, at=SR.AT_ENTER, t0=SC.TIE_T0, bin_ns=SC.MS, n_bins=8)

    def run(pk, status, r0=0, r1=n):
        rc = _call(net, nodes, r0, r1, (pred[r0:r1], lat[r0:r1]), ht, _batch(pk), list(SC.bases(nl, 8)), status=status, **kw)
        return (rc,) + _error(ctx)

    pk = dict(base, src=base["src"].copy())
    pk["src"][1234] = hosts["n"]
    rc, pair, msg = run(pk, st)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == (1234, UMAX) and "source host" in msg, (pair, msg)
    want = RR.first_bad_packet(hosts, base, st, (0, 40), n)
    assert want is not None and want > 0
    rc, pair, msg = run(base, st, 0, 40)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == (want, UMAX) and "row" in msg, (pair, want, msg)
    pk = dict(base, dst_ip=base["dst_ip"].copy())
    pk["dst_ip"][700] = pk["dst_ip"][900] = 0x0A090909
    rc, pair, msg = run(pk, st)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == (900, UMAX) and "address" in msg, (pair, msg)
    assert run(pk, None)[1] == (700, UMAX)
    # argument errors
    outs = list(SC.bases(nl, 8))
    pb = _batch(base)
    dup = nodes.copy()
    dup[5] = 6
    other = _net(LC.multi_graph(), ctx)
    tabs = (pred, lat)
    ident = np.arange(nl, dtype=np.uint32)
    high = ident.copy()
    high[11] = nl
    codes = [_call(net, dup, 0, n, tabs, ht, pb, outs, **kw),
             _call(net, nodes[:40], 0, 4, tabs, ht, pb, outs, **kw),
             _call(net, nodes, 3, 2, tabs, ht, pb, outs, **kw),
             _call(net, nodes, n - 1, n + 1, tabs, ht, pb, outs, **kw),
             _call(other, nodes, 0, n, tabs, ht, pb, outs, **kw),
             _call(net, nodes, 0, n, (None, lat), ht, pb, outs, **kw),
             _call(net, nodes, 0, n, (pred, None), ht, pb, outs, **kw),
             _call(net, nodes, 0, n, tabs, ht, pb, outs, **dict(kw, bin_ns=0)),
             _call(net, nodes, 0, n, tabs, ht, pb, outs, **dict(kw, n_bins=0)),
             _call(net, nodes, 0, n, tabs, ht, pb, outs, **dict(kw, n_slots=0)),
             _call(net, nodes, 0, n, tabs, ht, pb, outs, **dict(kw, at=2)),
             _call(net, nodes, 0, n, tabs, ht, pb, [None, outs[1]], **kw),
             _call(net, nodes, 0, n, tabs, ht, pb, outs, **dict(kw, n_slots=nl - 1)),
             _call(net, nodes, 0, n, tabs, ht, pb, outs, slot=high, **kw)]
    assert codes == [_capi.SG_ERR_INVALID_ARG] * len(codes)
    assert _error(ctx)[0] == (11, UMAX)
    L, h, nh, p = _capi.load(), ctx.handle, net._ensure_net(), pb.c_struct()
    B, Ns = _capi.C.byref(p), nodes.ctypes.data
    P, Tl = pred.ctypes.data, lat.ctypes.data
    tail = (None, None, None, nl, 0, SC.TIE_T0, SC.MS, 8, outs[0].ctypes.data, outs[1].ctypes.data)
    no_time = pb.c_struct()
    no_time.send_time_ns = None
    bad = [L.sg_link_series_packets(h, None, ht.handle, Ns, n, 0, n, 0, P, Tl, B, *tail),
           L.sg_link_series_packets(h, nh, None, Ns, n, 0, n, 0, P, Tl, B, *tail),
           L.sg_link_series_packets(h, nh, ht.handle, None, n, 0, n, 0, P, Tl, B, *tail),
           L.sg_link_series_packets(h, nh, ht.handle, Ns, n, 0, n, 0, P, Tl, None, *tail),
           L.sg_link_series_packets(h, nh, ht.handle, Ns, n, 0, n, 0, P, Tl, _capi.C.byref(no_time), *tail)]
    assert bad == [_capi.SG_ERR_INVALID_ARG] * len(bad)
    assert _untouched(outs)
    # no packets at all: nothing added; out_outside may be NULL
    for dev in (False, True):
        outs = list(SC.bases(nl, 8))
        assert _call(net, nodes, 0, n, tabs, ht, _batch(_head(base, 0)), outs, dev=dev, **kw) == _capi.SG_OK and _untouched(outs)
        cross = SR.crossings(g, nodes, (0, n), pred, tie["olat"], hosts, base)
        _check(net, nodes, (0, n), tabs, ht, _batch(base), cross, outside=False, dev=dev, **kw)


# ---- 9. the sweep
@pytest.mark.parametrize("name", WC.NAMES)
def test_sweep(oracle, ctx, name):
    """The 40 generated graphs, each row block's round with its mixed statuses, 16 bins over the
    view's own enter range."""
    c, rs = WC.case(name), WC.refs(oracle, name)
    net = _net(c["g"], ctx)
    ht = _host_table(c["hosts"], ctx)
    nl = XR.n_links(c["g"])
    for v, r in zip(c["views"], rs):
        cross = SR.crossings(c["g"], c["nodes"], v["rows"], r["pred"], r["lat"], c["hosts"], v["pk"], v["status"],
                             v["pk"]["payload"])
        t0, bin_ns = SC.enter_range_bins(cross[2], 16)
        for at in ATS:
            _check(net, c["nodes"], v["rows"], (r["pred"], r["lat"]), ht, _batch(v["pk"]), cross, status=v["status"],
                   weight=v["pk"]["payload"], n_slots=nl, at=at, t0=t0, bin_ns=bin_ns, n_bins=16, dev=True)


# ---- 10. the Python interface
def test_python_interface(ctx, tie):
    """PathTree.link_series_round from a round's Deliveries: `slots` in its three forms, weight =
    "payload", `out=` across two rounds."""
    import torch

    from shadow_amd.worker import DeviceTable, deliver_round

    g, net, hosts, pk = tie["g"], tie["net"], tie["hosts"], tie["pk"]
    t = net.compute_shortest_path_tree()
    assert np.array_equal(t.latency_ns, tie["olat"])
    dlat = torch.from_numpy(t.latency_ns.view(np.int64)).cuda()
    dloss = torch.from_numpy(t.packet_loss).cuda()
    out = deliver_round(_host_table(hosts, ctx), DeviceTable(dlat.ravel(), dloss.ravel(), 300), tie["pb"], RC.ROUND_END,
                        2**63, 0, ctx=ctx)
    status = out.status[:len(pk["src"])].cpu().numpy()
    assert 0 < int((status == 0).sum()) == out.n_delivered < len(status)
    nl = tie["n_links"]
    some = [5, 17, 400, 401, nl - 1]
    both, ns = SC.both_directions(tie["tail"], tie["head"])
    kw = dict(t0_ns=SC.TIE_T0, bin_ns=250_000, n_bins=64)
    cross = SR.crossings(g, t.nodes, (0, 300), t.pred, tie["olat"], hosts, pk, status, pk["payload"])
    for slots, (slot, n_slots) in ((None, (None, nl)), (some, SR.list_slots(g, some)), (both, (both, ns))):
        for at, code in (("enter", 0), ("exit", 1)):
            got = t.link_series_round(tie["ht"], tie["pb"], out, "payload", slots=slots, at=at, **kw)
            want = SR.bin_crossings(cross, slot, n_slots, code, SC.TIE_T0, 250_000, 64)
            assert got[0].dtype == got[1].dtype == np.uint64 and got[0].shape == (n_slots, 64) and got[1].shape == (n_slots, 2)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # a loop over rounds keeps one matrix
    ones = SR.crossings(g, t.nodes, (0, 300), t.pred, tie["olat"], hosts, pk)
    acc = t.link_series_round(tie["ht"], tie["pb"], status, pk["payload"], slots=some, **kw)
    again = t.link_series_round(tie["ht"], tie["pb"], out=acc, slots=some, **kw)
    assert again[0] is acc[0] and again[1] is acc[1]
    slot = SR.list_slots(g, some)[0]
    want = SR.bin_crossings(ones, slot, 5, 0, SC.TIE_T0, 250_000, 64, base=SR.bin_crossings(cross, slot, 5, 0, SC.TIE_T0, 250_000, 64))
    assert np.array_equal(acc[0], want[0]) and np.array_equal(acc[1], want[1])
    for bad in (dict(slots=[nl]), dict(at="middle"), dict(out=(acc[0][:3], acc[1]), slots=some)):
        with pytest.raises(ValueError):
            t.link_series_round(tie["ht"], tie["pb"], **dict(kw, **bad))
