"""The link time series of a round sharded over a device group, on the card
(sg_group_link_series_packets, Group.link_series_round).

The members are N contexts on device 0, built as test_group_trace_gpu.py builds them (never more
than 8 open).  The reference is tests/series_ref.py on the members' batches concatenated in member
order over all rows; the single-context call on that batch must give the same bits.  Root's arrays
start from non-zero base values; every comparison is exact (np.array_equal)."""
import numpy as np
import pytest

import group_trace_cases as GC
import link_cases as LC
import series_cases as SC
import series_ref as SR
import sweep_cases as WC
import trace_cases as XC
from shadow_amd import _capi
from test_group_trace_gpu import _common, _error, _full_tabs, _load_parts, _part, _ptrs, _shard, members
from test_series_gpu import _batch, _call, _dev, _host_table, _net, _oracle_lat

pytestmark = pytest.mark.gpu

C = _capi.C
UMAX = 0xFFFFFFFF
ATS = (SR.AT_ENTER, SR.AT_EXIT)


def _series(group, S, outs, *, weight=None, slot=None, n_slots, at, t0, bin_ns, n_bins, root=0, **kw):
    """sg_group_link_series_packets adding into outs = [series, outside or None] (uploaded to root's
    device, copied back).  weight: per-member numpy u32 arrays or None; slot: a host u32 map or None."""
    import torch

    d = [_dev(o) for o in outs]
    dw = None if weight is None else [_dev(np.ascontiguousarray(w, np.uint32)) for w in weight]
    sl = None if slot is None else np.ascontiguousarray(slot, np.uint32)
    torch.cuda.synchronize()
    rc = _capi.load().sg_group_link_series_packets(
        group.handle, *_common(S, **kw), _ptrs(S.lat), S._live[1], None if S.status is None else _ptrs(S.status),
        None if dw is None else _ptrs(dw), None if sl is None else sl.ctypes.data, int(n_slots), int(at), int(t0),
        int(bin_ns), int(n_bins), root, *[None if t is None else C.c_void_p(t.data_ptr()) for t in d])
    torch.cuda.synchronize()
    for o, t in zip(outs, d):
        if o is not None:
            o[...] = t.cpu().numpy().view(np.uint64).reshape(o.shape)
    return rc


def _check(group, S, hosts, pred, lat, *, weighted=True, slot=None, n_slots, root=0, **kw):
    """One call from the base values against the reference on the concatenated batch."""
    cat, status, _ = GC.concat(S.parts)
    rows = (S.ranges[0][0], S.ranges[-1][1])
    base = SC.bases(n_slots, kw["n_bins"])
    want = SR.series(S.g, S.nodes, rows, pred, lat, hosts, cat, status, cat["payload"] if weighted else None, slot=slot,
                     n_slots=n_slots, base=base, **kw)
    outs = [base[0].copy(), base[1].copy()]
    rc = _series(group, S, outs, weight=[p[0]["payload"] for p in S.parts] if weighted else None, slot=slot, n_slots=n_slots,
                 root=root, **kw)
    assert rc == _capi.SG_OK, _error(group)
    assert group.last_error_member() is None
    assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[1])
    return outs


def _untouched(outs):
    return (outs[0] == SC.BASE_SERIES).all() and (outs[1] == SC.BASE_OUTSIDE).all()


@pytest.fixture(scope="module")
def tie(oracle):
    g = LC.tie_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    hosts, pk, mixed = XC.tie_round()
    return dict(g=g, nodes=nodes, hosts=hosts, pk=pk, mixed=mixed, olat=_oracle_lat(oracle, g, nodes, 0, g["n"]))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_tie_round(ctx, tie, world):
    """The tie round over 1, 2, 3 and 8 members, mixed statuses and none, both `at` values, a
    list of links (the members' LDS form) and the identity: equal to the reference and, bit for
    bit, to the single-context call on the concatenated batch; root = W - 1."""
    g, nodes, hosts = tie["g"], tie["nodes"], tie["hosts"]
    with members(world) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(300, world))
        pred, lat = _full_tabs(S)
        assert np.array_equal(lat, tie["olat"])
        one = keep(_net(g, ctx))
        oht = keep(_host_table(hosts, ctx))
        some = SR.list_slots(g, np.arange(100, 116))
        for status in (tie["mixed"], None):
            _load_parts(S, GC.split(hosts, tie["pk"], status, 300, world))
            cat, cstatus, _ = GC.concat(S.parts)
            for at, (slot, ns), (bin_ns, n_bins) in ((0, some, SC.BIN_SETS[1]), (1, (None, S.n_links), SC.BIN_SETS[2])):
                kw = dict(slot=slot, n_slots=ns, at=at, t0=SC.TIE_T0, bin_ns=bin_ns, n_bins=n_bins)
                outs = _check(group, S, hosts, pred, tie["olat"], root=world - 1, **kw)
                single = list(SC.bases(ns, n_bins))
                rc = _call(one, nodes, 0, 300, (pred, lat), oht, _batch(cat), single, status=cstatus, weight=cat["payload"],
                           dev=True, **kw)
                assert rc == _capi.SG_OK and np.array_equal(outs[0], single[0]) and np.array_equal(outs[1], single[1])
        # without out_outside
        base = SC.bases(16, 8)
        outs = [base[0].copy(), None]
        assert _series(group, S, outs, slot=some[0], n_slots=16, at=0, t0=SC.TIE_T0, bin_ns=SC.MS, n_bins=8) == _capi.SG_OK
        cat, cstatus, _ = GC.concat(S.parts)
        want = SR.series(g, nodes, (0, 300), pred, tie["olat"], hosts, cat, cstatus, None, slot=some[0], n_slots=16, at=0,
                         t0=SC.TIE_T0, bin_ns=SC.MS, n_bins=8, base=base)
        assert np.array_equal(outs[0], want[0])


def test_empty_members(oracle):
    """3 nodes and 8 members, five of them without rows or packets; a member with rows and an
    empty batch; every batch empty: nothing added."""
    g = GC.tiny_graph()
    nodes = np.arange(3, dtype=np.uint32)
    olat = _oracle_lat(oracle, g, nodes, 0, 3)
    hosts, pk = GC.tiny_round()
    with members(8) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(3, 8))
        pred, lat = _full_tabs(S)
        parts = GC.split(hosts, pk, None, 3, 8)
        assert [len(p[2]) > 0 for p in parts] == [True] * 3 + [False] * 5
        lone = [p if m != 1 else ({k: v[:0] for k, v in p[0].items()}, None, p[2][:0]) for m, p in enumerate(parts)]
        kw = dict(n_slots=S.n_links, at=1, t0=SC.T0, bin_ns=100_000, n_bins=32)
        for ps, root in ((parts, 5), (lone, 2)):
            _load_parts(S, ps)
            _check(group, S, hosts, pred, olat, root=root, **kw)
        _load_parts(S, [({k: v[:0] for k, v in p[0].items()}, None, p[2][:0]) for p in parts])
        outs = list(SC.bases(S.n_links, 32))
        assert _series(group, S, outs, **kw) == _capi.SG_OK and _untouched(outs)


def test_errors(tie):
    """A bad packet in members 1 and 2: member 1 is reported and root's arrays are untouched; a
    time overflow; a corrupted crossed pred cell; a slot value >= n_slots and the other argument
    errors name no member."""
    import link_round_ref as RR

    g, nodes, hosts = tie["g"], tie["nodes"], tie["hosts"]
    W = 3
    pk = {k: v[:3000] for k, v in tie["pk"].items()}
    with members(W) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(300, W))
        pred, _ = _full_tabs(S)
        good = [_part(p[0]) for p in GC.split(hosts, pk, None, 300, W)]
        kw = dict(n_slots=S.n_links, at=0, t0=SC.TIE_T0, bin_ns=SC.MS, n_bins=8)

        def fails(parts, code, member, pair, word, **more):
            _load_parts(S, parts)
            outs = list(SC.bases(S.n_links, 8))
            rc = _series(group, S, outs, root=W - 1, **dict(kw, **more))
            who, got, msg = _error(group)
            assert (rc, who, got) == (code, member, pair) and word in msg, (rc, who, got, msg)
            assert (member is None or f"member {member}" in msg) and _untouched(outs)

        parts = [_part(p[0]) for p in good]
        parts[1][0]["src"][77] = hosts["n"]
        fails(parts, _capi.SG_ERR_INVALID_ARG, 1, (77, UMAX), "source host")
        parts[2][0]["src"][3] = hosts["n"] + 9
        fails(parts, _capi.SG_ERR_INVALID_ARG, 1, (77, UMAX), "source host")
        parts = [_part(p[0]) for p in good]
        parts[2][0]["send_time"][9] = np.uint64((1 << 64) - 1)
        fails(parts, _capi.SG_ERR_TIME_OVERFLOW, 2, (9, UMAX), "packet 9 ")
        # a crossed pred cell of member 1
        r0, r1 = S.ranges[1]
        block = S.tabs[1][0]
        _, ri, cj = RR.counted_pairs(hosts, good[1][0], None)
        k = int(np.flatnonzero((ri != cj) & (block[ri - r0, cj] != ri))[0])
        bad = block.copy()
        bad[int(ri[k]) - r0, int(cj[k])] = 300
        want = RR.first_bad_pred(g, nodes, (r0, r1), bad, hosts, good[1][0])
        rows = list(S.pred)
        rows[1] = _dev(bad)
        fails([_part(p[0]) for p in good], _capi.SG_ERR_INVALID_ARG, 1, want, "range", pred=rows)
        # argument errors: no member named
        high = np.arange(S.n_links, dtype=np.uint32)
        high[11] = S.n_links
        fails(good, _capi.SG_ERR_INVALID_ARG, None, (11, UMAX), "link_slot[11]", slot=high)
        for more in (dict(bin_ns=0), dict(n_bins=0), dict(n_slots=0), dict(at=2), dict(n_slots=S.n_links - 1)):
            _load_parts(S, good)
            outs = list(SC.bases(S.n_links, 8))
            assert _series(group, S, outs, **dict(kw, **more)) == _capi.SG_ERR_INVALID_ARG and _untouched(outs), more
        assert _series(group, S, outs, root=W, **kw) == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
        assert _series(group, S, [None, outs[1]], **kw) == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
        # and the group still works
        _check(group, S, hosts, pred, tie["olat"], **kw)


@pytest.mark.parametrize("name", WC.NAMES)
def test_sweep(oracle, name):
    """The 40 generated graphs over 3 members: the whole table's round with its mixed statuses,
    16 bins over the round's own enter range."""
    c, r = WC.case(name), WC.refs(oracle, name)[0]
    g, nodes, hosts, v = c["g"], c["nodes"], c["hosts"], c["views"][0]
    n = g["n"]
    with members(3) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(n, 3))
        _load_parts(S, GC.split(hosts, v["pk"], v["status"], n, 3))
        cat, status, _ = GC.concat(S.parts)
        enter = SR.crossings(g, nodes, (0, n), r["pred"], r["lat"], hosts, cat, status)[2]
        t0, bin_ns = SC.enter_range_bins(enter, 16)
        for at in ATS:
            _check(group, S, hosts, r["pred"], r["lat"], n_slots=S.n_links, at=at, t0=t0, bin_ns=bin_ns, n_bins=16, root=at)


def test_python_interface(tie):
    """Group.link_series_round: slots as a list, weight = "payload", `out=` across two rounds."""
    g, nodes, hosts, pk = tie["g"], tie["nodes"], tie["hosts"], tie["pk"]
    W = 3
    with members(W) as (ctxs, group, keep):
        graphs = [keep(_net(g, c)) for c in ctxs]
        tree = graphs[0].compute_shortest_path_tree()
        hts = [keep(_host_table(hosts, c)) for c in ctxs]
        parts = GC.split(hosts, pk, tie["mixed"], 300, W)
        batches = [_batch(p[0]) for p in parts]
        status = [p[1] for p in parts]
        cat, cstatus, _ = GC.concat(parts)
        some = [5, 17, 400, 401, len(graphs[0].links()[0]) - 1]
        slot = SR.list_slots(g, some)[0]
        kw = dict(t0_ns=SC.TIE_T0, bin_ns=250_000, n_bins=64)
        got = group.link_series_round(graphs, hts, tree, batches, status, "payload", slots=some, at="exit", root=1, **kw)
        want = SR.series(g, nodes, (0, 300), tree.pred, tie["olat"], hosts, cat, cstatus, cat["payload"], slot=slot, n_slots=5,
                         at=1, t0=SC.TIE_T0, bin_ns=250_000, n_bins=64)
        assert got[0].dtype == np.uint64 and got[0].shape == (5, 64) and got[1].shape == (5, 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        again = group.link_series_round(graphs, hts, tree, batches, status, "payload", slots=some, at="exit", out=got, **kw)
        assert again[0] is got[0] and np.array_equal(got[0], 2 * want[0]) and np.array_equal(got[1], 2 * want[1])
        every = group.link_series_round(graphs, hts, tree, batches, **kw)
        want = SR.series(g, nodes, (0, 300), tree.pred, tie["olat"], hosts, cat, None, None, at=0, t0=SC.TIE_T0, bin_ns=250_000,
                         n_bins=64)
        assert np.array_equal(every[0], want[0]) and np.array_equal(every[1], want[1])
        with pytest.raises(ValueError):
            group.link_series_round(graphs, hts, tree, batches, slots=[len(graphs[0].links()[0])], **kw)
