"""Link loads and the link trace of a round sharded over a device group, on the card
(sg_group_link_load_packets, sg_group_link_trace_packets, Group.link_load_round,
Group.link_trace_round).

The members are N contexts on device 0 (the `members()` pattern of test_group_gpu.py).  Member m
holds rows dist.row_range(n_rows, N, m): its pred and latency rows come from sg_routing_build_tree
on that block of its own net, its batch is the round's packets whose sender's row lies there
(tests/group_trace_cases.py).  The reference is tests/trace_ref.py / tests/link_round_ref.py on the
members' batches concatenated in member order over all rows; a record's member is recovered from
the packet bases.  Every output starts from sentinels, a few records longer than the total; every
comparison is exact (np.array_equal).  The inputs' own conditions are checked on the CPU in
test_group_trace_ref_cpu.py."""
import contextlib
import types

import numpy as np
import pytest

import group_trace_cases as GC
import link_cases as LC
import link_round_cases as RC
import link_round_ref as RR
import sweep_cases as SC
import trace_cases as XC
from shadow_amd import Context, Group, GroupDelivery, _capi, synth
from shadow_amd.dist import HostPartition
from test_trace_gpu import _batch, _call, _dev, _host_table, _net, _oracle_lat, _sentinels, _tabs

pytestmark = pytest.mark.gpu

C = _capi.C
UMAX = 0xFFFFFFFF
PAD = 3
NAMES = ("packet", "member", "hop", "enter", "exit")
KEYS = ("off",) + NAMES
DTYPES = dict(off=np.uint64, packet=np.uint32, member=np.uint8, hop=np.uint32, enter=np.uint64, exit=np.uint64)


@contextlib.contextmanager
def members(n):
    """n contexts on device 0 and their group; `keep(obj)` registers an object created on one of
    them, released (in reverse) before the group and the contexts close."""
    ctxs, made, group = [], [], None

    def keep(obj):
        made.append(obj)
        return obj

    try:
        for _ in range(n):
            ctxs.append(Context(device=0))
        group = Group(ctxs)
        yield ctxs, group, keep
    finally:
        for obj in reversed(made):
            (getattr(obj, "close", None) or obj.__del__)()
        if group is not None:
            group.close()
        for c in ctxs:
            c.close()


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None or t.numel() == 0 else t.data_ptr() for t in tensors])


def _shard(ctxs, keep, g, nodes, hosts, ranges):
    """The members' nets, host tables and rows (sg_routing_build_tree on each member's block)."""
    S = types.SimpleNamespace(n=len(ctxs), g=g, nodes=np.ascontiguousarray(nodes, np.uint32), ranges=list(ranges))
    S.nets = [keep(_net(g, c)) for c in ctxs]
    S.hts = [keep(_host_table(hosts, c)) for c in ctxs]
    n = len(S.nodes)
    S.tabs = [_tabs(S.nets[m], S.nodes, r0, r1) if r1 > r0 else (np.zeros((0, n), np.uint32), np.zeros((0, n), np.uint64))
              for m, (r0, r1) in enumerate(S.ranges)]
    S.pred, S.lat = [_dev(t[0]) for t in S.tabs], [_dev(t[1]) for t in S.tabs]
    S.n_links = len(S.nets[0].links()[0])
    return S


def _load_parts(S, parts):
    S.parts = parts
    S.pbs = [_batch(p[0]) for p in parts]
    S.status = None if parts[0][1] is None else [_dev(np.ascontiguousarray(p[1], np.uint8)) for p in parts]
    return S


def _common(S, nets=None, hts=None, nodes=None, ranges=None, pred=None):
    n = S.n
    nets = S.nets if nets is None else nets
    hts = S.hts if hts is None else hts
    ranges = S.ranges if ranges is None else ranges
    nodes = S.nodes if nodes is None else nodes
    S._live = (nodes, (_capi.sg_packets * n)(*[pb.c_struct() for pb in S.pbs]))
    return [(C.c_void_p * n)(*[None if x is None else x._ensure_net().value for x in nets]),
            (C.c_void_p * n)(*[None if h is None else getattr(h.handle, "value", h.handle) for h in hts]),
            nodes.ctypes.data, len(nodes), (C.c_uint32 * n)(*[r[0] for r in ranges]),
            (C.c_uint32 * n)(*[r[1] for r in ranges]), _ptrs(S.pred if pred is None else pred)]


def _sent(n_links, cap, which=NAMES):
    outs = dict(_sentinels(n_links, cap), member=np.full(cap, GC.SENT8, np.uint8))
    return {k: (outs[k] if k == "off" or k in which else None) for k in KEYS}


def _untouched(outs, off=True):
    cap = max(len(v) for k, v in outs.items() if k != "off" and v is not None)
    want = _sent(len(outs["off"]) - 1, cap)
    return all(v is None or (k == "off" and not off) or np.array_equal(v, want[k]) for k, v in outs.items())


def _trace(group, S, outs, cap, watch=None, bases=None, root=0, **kw):
    """sg_group_link_trace_packets from `outs` (uploaded to root's device, copied back).  Returns
    (status code, total)."""
    import torch

    d = {k: _dev(outs[k]) for k in KEYS}
    op = [None if d[k] is None else C.c_void_p(d[k].data_ptr()) for k in KEYS]
    total = C.c_uint64(0xDEAD)
    w = None if watch is None else np.ascontiguousarray(watch, np.uint8)
    b = None if bases is None else np.ascontiguousarray(bases, np.uint32)
    torch.cuda.synchronize()
    rc = _capi.load().sg_group_link_trace_packets(
        group.handle, *_common(S, **kw), _ptrs(S.lat), S._live[1], None if S.status is None else _ptrs(S.status),
        None if w is None else w.ctypes.data, None if b is None else b.ctypes.data, root, *op, cap, C.byref(total))
    torch.cuda.synchronize()
    for k in KEYS:
        if outs[k] is not None:
            outs[k][...] = d[k].cpu().numpy().view(outs[k].dtype)
    return rc, total.value


def _loads(group, S, link, node, weight=None, hops=True, root=0, **kw):
    """sg_group_link_load_packets adding into `link` / `node` (numpy u64 or None, updated in place).
    weight: per-member numpy u32 arrays or None.  Returns (status code, per-member hops)."""
    import torch

    dl, dn = _dev(link), _dev(node)
    dh = [_dev(np.full(max(len(p[0]["src"]), 1), RC.SENT32, np.uint32)) for p in S.parts] if hops else None
    dw = None if weight is None else [_dev(np.ascontiguousarray(w, np.uint32)) for w in weight]
    torch.cuda.synchronize()
    rc = _capi.load().sg_group_link_load_packets(
        group.handle, *_common(S, **kw), S._live[1], None if S.status is None else _ptrs(S.status),
        None if dw is None else _ptrs(dw), root, None if dl is None else C.c_void_p(dl.data_ptr()),
        None if dn is None else C.c_void_p(dn.data_ptr()), None if dh is None else _ptrs(dh))
    torch.cuda.synchronize()
    if link is not None:
        link[...] = dl.cpu().numpy().view(np.uint64)
    if node is not None:
        node[...] = dn.cpu().numpy().view(np.uint64)
    got = None if dh is None else [h.cpu().numpy().view(np.uint32)[:len(p[0]["src"])] for h, p in zip(dh, S.parts)]
    return rc, got


def _error(group):
    r, k = C.c_uint32(), C.c_uint32()
    L = _capi.load()
    L.sg_group_last_error_pair(group.handle, C.byref(r), C.byref(k))
    return group.last_error_member(), (r.value, k.value), L.sg_group_last_error(group.handle).decode()


def _same(outs, want, which=NAMES):
    off, total = want[0], int(want[0][-1])
    assert np.array_equal(outs["off"], off), f"offsets differ at {int((outs['off'] != off).sum())} entries"
    tail = _sent(0, PAD)
    for k, w in zip(NAMES, want[1:]):
        if k not in which:
            continue
        got = outs[k]
        assert got.dtype == DTYPES[k]
        assert np.array_equal(got[:total], w), f"{k} differs at {int((got[:total] != w).sum())} of {total} records"
        assert np.array_equal(got[total:], tail[k][:len(got) - total]), f"{k}: written past the total"


def _check(group, S, want, which=NAMES, **kw):
    """One call from sentinels at cap = the total against the reference."""
    total = int(want[0][-1])
    outs = _sent(S.n_links, total + PAD, which)
    rc, got = _trace(group, S, outs, total, **kw)
    assert rc == _capi.SG_OK, _error(group)
    assert got == total and group.last_error_member() is None
    _same(outs, want, which)
    return outs


def _full_tabs(S):
    """The members' rows stacked: all rows, as one context would hold them."""
    return np.concatenate([t[0] for t in S.tabs]), np.concatenate([t[1] for t in S.tabs])


def _want_loads(S, hosts, pred, weight, link0, node0):
    """(link, node, per-member hops) of link_round_ref on the concatenated batch, added to copies."""
    cat, status, bases = GC.concat(S.parts)
    n = len(S.nodes)
    w = None if weight is None else np.concatenate(weight)
    link, node, hops = RR.link_load_round(S.g, S.nodes, (S.ranges[0][0], S.ranges[-1][1]), pred, hosts, cat, status, w,
                                          link0.copy(), node0.copy())
    assert len(node) == n
    ends = list(bases[1:]) + [len(cat["src"])]
    return link, node, [hops[int(a):int(b)] for a, b in zip(bases, ends)]


@pytest.fixture(scope="module")
def tie(oracle):
    g = LC.tie_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    hosts, pk, mixed = XC.tie_round()
    return dict(g=g, nodes=nodes, hosts=hosts, pk=pk, mixed=mixed, olat=_oracle_lat(oracle, g, nodes, 0, g["n"]))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_tie_round(ctx, tie, world):
    """(1): the tie round over 1, 2, 3 and 8 members, mixed statuses and none: the trace and the
    loads equal the reference and the single-context calls on the concatenated batch; the loads
    are added onto non-zero contents, weight = payload, hops per member; diff(out_link_off) is the
    unit-weight link load.  The timers count the records."""
    g, nodes, hosts = tie["g"], tie["nodes"], tie["hosts"]
    rng = np.random.default_rng(world)
    with members(world) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(300, world))
        pred, lat = _full_tabs(S)
        assert np.array_equal(lat, tie["olat"])
        one = keep(_net(g, ctx))  # the single context: all rows, the concatenated batch
        oht = keep(_host_table(hosts, ctx))
        for status in (tie["mixed"], None):
            _load_parts(S, GC.split(hosts, tie["pk"], status, 300, world))
            want = GC.trace(g, nodes, 300, pred, tie["olat"], hosts, S.parts)
            total = int(want[0][-1])
            ctxs[0].enable_timers(True)
            try:
                outs = _check(group, S, want)
                _, launches, work = ctxs[0].read_timer("group_trace_merge")
                assert launches == 1 and int(work) == total
            finally:
                ctxs[0].enable_timers(False)
            cat, cstatus, _ = GC.concat(S.parts)
            single = _sentinels(S.n_links, total + PAD)
            rc, got = _call(one, nodes, 0, 300, (pred, lat), single, total, ht=oht, pb=_batch(cat), status=cstatus, dev=True)
            assert rc == _capi.SG_OK and got == total
            for k in ("off", "packet", "hop", "enter", "exit"):  # (world = 1: bit for bit that call's output)
                assert np.array_equal(outs[k], single[k]), k
            # the loads, onto non-zero contents, weight = payload
            link0 = rng.integers(1, 1 << 40, S.n_links).astype(np.uint64)
            node0 = rng.integers(1, 1 << 40, 300).astype(np.uint64)
            weight = [p[0]["payload"] for p in S.parts]
            wl, wn, wh = _want_loads(S, hosts, pred, weight, link0, node0)
            link, node = link0.copy(), node0.copy()
            rc, hops = _loads(group, S, link, node, weight)
            assert rc == _capi.SG_OK, _error(group)
            assert np.array_equal(link, wl) and np.array_equal(node, wn)
            assert all(np.array_equal(a, b) for a, b in zip(hops, wh))
            sl, sn = _dev(link0), _dev(node0)
            sh = _dev(np.zeros(len(cat["src"]), np.uint32))
            dp, ds, dw = _dev(pred), _dev(cstatus), _dev(cat["payload"])
            one.link_load_packets_device(oht, nodes, 0, 300, dp.data_ptr(), _batch(cat), 0 if ds is None else ds.data_ptr(),
                                         dw.data_ptr(), sl.data_ptr(), sn.data_ptr(), sh.data_ptr())
            assert np.array_equal(sl.cpu().numpy().view(np.uint64), link) and np.array_equal(sn.cpu().numpy().view(np.uint64), node)
            assert np.array_equal(sh.cpu().numpy().view(np.uint32), np.concatenate(hops))
            # unit weights from zero: the records per link
            unit = np.zeros(S.n_links, np.uint64)
            rc, _ = _loads(group, S, unit, None, None, hops=False)
            assert rc == _capi.SG_OK and np.array_equal(np.diff(outs["off"].astype(np.int64)).astype(np.uint64), unit)


@pytest.mark.parametrize("times", ["equal", "tied", "shuffled"])
def test_fan_in(oracle, times):
    """(2): one source per member, one destination: the last link holds a segment of every member,
    of 0, 1, 63, 64, 65 and 2049 records (2049: a member's own sort runs its merge tier), a member
    with none beside one with 2049; one enter time (the order is by member, then packet), and
    distinct, shuffled ones."""
    g, nodes = GC.fan_graph(), GC.fan_nodes()
    olat = _oracle_lat(oracle, g, nodes, 0, GC.FAN_N)
    with members(GC.FAN_W) as (ctxs, group, keep):
        S = None
        for lengths in GC.FAN_CASES:
            hosts, parts = GC.fan_round(lengths, times)
            if S is None:
                S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(GC.FAN_N, GC.FAN_W))
                pred, lat = _full_tabs(S)
                assert np.array_equal(lat, olat)
            _load_parts(S, parts)
            want = GC.trace(g, nodes, GC.FAN_N, pred, olat, hosts, parts)
            _check(group, S, want)
            zl, zn = np.zeros(S.n_links, np.uint64), np.zeros(GC.FAN_N, np.uint64)
            wl, wn, wh = _want_loads(S, hosts, pred, None, zl, zn)
            rc, hops = _loads(group, S, zl, zn)
            assert rc == _capi.SG_OK and np.array_equal(zl, wl) and np.array_equal(zn, wn)
            assert all(np.array_equal(a, b) for a, b in zip(hops, wh))


def test_empty_members(oracle):
    """(3): 3 nodes and 8 members, five of them without rows or packets; a member with rows and an
    empty batch; every batch empty: all offsets zero, total 0, no record written."""
    g = GC.tiny_graph()
    nodes = np.arange(3, dtype=np.uint32)
    olat = _oracle_lat(oracle, g, nodes, 0, 3)
    hosts, pk = GC.tiny_round()
    with members(8) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(3, 8))
        assert [r1 - r0 for r0, r1 in S.ranges] == [1, 1, 1, 0, 0, 0, 0, 0]
        pred, lat = _full_tabs(S)
        parts = GC.split(hosts, pk, None, 3, 8)
        assert [len(p[2]) > 0 for p in parts] == [True] * 3 + [False] * 5
        lone = [p if m != 1 else ({k: v[:0] for k, v in p[0].items()}, None, p[2][:0]) for m, p in enumerate(parts)]
        for ps in (parts, lone):
            _load_parts(S, ps)
            _check(group, S, GC.trace(g, nodes, 3, pred, olat, hosts, ps), root=5)
            link, node = np.full(S.n_links, 7, np.uint64), np.full(3, 9, np.uint64)
            wl, wn, wh = _want_loads(S, hosts, pred, None, link, node)
            rc, hops = _loads(group, S, link, node, root=2)
            assert rc == _capi.SG_OK and np.array_equal(link, wl) and np.array_equal(node, wn)
            assert all(np.array_equal(a, b) for a, b in zip(hops, wh))
        _load_parts(S, [({k: v[:0] for k, v in p[0].items()}, None, p[2][:0]) for p in parts])
        outs = _sent(S.n_links, PAD)
        rc, total = _trace(group, S, outs, PAD)
        assert rc == _capi.SG_OK and total == 0 and not outs["off"].any() and _untouched(outs, off=False)
        link = np.full(S.n_links, 7, np.uint64)
        rc, _ = _loads(group, S, link, None)
        assert rc == _capi.SG_OK and (link == 7).all()


def test_wide_latencies(oracle):
    """(4): latencies past 2^32 ns: enter times on both sides of 2^32 inside a segment."""
    g = XC.wide_graph()
    n = g["n"]
    nodes = np.arange(n, dtype=np.uint32)
    olat = _oracle_lat(oracle, g, nodes, 0, n)
    hosts, pk = XC.wide_round()
    with members(3) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(n, 3))
        pred, lat = _full_tabs(S)
        assert np.array_equal(lat, olat)
        _load_parts(S, GC.split(hosts, pk, None, n, 3))
        want = GC.trace(g, nodes, n, pred, olat, hosts, S.parts)
        assert int(want[4].min()) < 1 << 32 < int(want[4].max())
        _check(group, S, want)


def test_watch_capacity_outputs(tie):
    """(5): a watch mask; cap one below the total: SG_ERR_CAPACITY, offsets and total complete, the
    record arrays still sentinels; the sizing call; subsets of the record arrays; root = W - 1;
    explicit packet bases."""
    g, nodes, hosts = tie["g"], tie["nodes"], tie["hosts"]
    W = 3
    pk = {k: v[:4000] for k, v in tie["pk"].items()}
    with members(W) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(300, W))
        pred, _ = _full_tabs(S)
        _load_parts(S, GC.split(hosts, pk, tie["mixed"][:4000], 300, W))
        every = GC.trace(g, nodes, 300, pred, tie["olat"], hosts, S.parts)
        total = int(every[0][-1])
        masks = [np.zeros(S.n_links, np.uint8), (np.arange(S.n_links) % 2).astype(np.uint8)]
        for m in masks:
            want = GC.trace(g, nodes, 300, pred, tie["olat"], hosts, S.parts, watch=m)
            outs = _check(group, S, want, watch=m, root=W - 1)
            if not m.any():
                assert not outs["off"].any() and _untouched(outs, off=False)
        # capacity
        outs = _sent(S.n_links, total + PAD)
        rc, got = _trace(group, S, outs, total - 1)
        assert rc == _capi.SG_ERR_CAPACITY and got == total and group.last_error_member() is None
        assert np.array_equal(outs["off"], every[0]) and _untouched(outs, off=False)
        rc, got = _trace(group, S, outs, total)
        assert rc == _capi.SG_OK and got == total
        _same(outs, every)
        # the sizing call: one real record array, capacity 0
        outs = _sent(S.n_links, PAD, ("member",))
        rc, got = _trace(group, S, outs, 0)
        assert rc == _capi.SG_ERR_CAPACITY and got == total and np.array_equal(outs["off"], every[0])
        assert _untouched(outs, off=False)
        # subsets of the record arrays, on the last member
        for which in (("member",), ("packet", "exit"), ("hop", "enter"), ("packet", "member", "hop", "exit")):
            _check(group, S, every, which, root=W - 1)
        # explicit bases
        bases = np.array([1_000_000, 5, 70_000], np.uint32)
        want = GC.trace(g, nodes, 300, pred, tie["olat"], hosts, S.parts, bases=bases)
        assert not np.array_equal(want[1], every[1]) and np.array_equal(want[2], every[2])
        _check(group, S, want, bases=bases)


def _part(pk, status=None):
    return ({k: v.copy() for k, v in pk.items()}, None if status is None else status.copy(), None)


def test_device_found_errors(tie):
    """(6): a bad source host in member 1 only; bad packets in members 1 and 2 (member 1 is
    reported); a source outside its member's block; a time overflow; a corrupted crossed pred cell
    in one member, and the same corruption in an uncrossed cell succeeding.  Each: the code, the
    member, the pair (the packet index member-local), and root's outputs untouched."""
    g, nodes, hosts = tie["g"], tie["nodes"], tie["hosts"]
    W = 3
    pk = {k: v[:3000] for k, v in tie["pk"].items()}
    with members(W) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(300, W))
        pred, _ = _full_tabs(S)
        good = [_part(p[0]) for p in GC.split(hosts, pk, None, 300, W)]
        assert all(len(p[0]["src"]) > 100 for p in good)

        def fails(parts, code, member, pair, word, trace_only=False, pred_rows=None):
            _load_parts(S, parts)
            kw = {} if pred_rows is None else dict(pred=pred_rows)
            outs = _sent(S.n_links, 40000)
            rc, total = _trace(group, S, outs, 40000, **kw)
            who, got, msg = _error(group)
            assert (rc, who, got) == (code, member, pair) and f"member {member}" in msg and word in msg, (rc, who, got, msg)
            assert _untouched(outs) and total == 0xDEAD
            if trace_only:
                return
            link, node = np.full(S.n_links, 5, np.uint64), np.full(300, 6, np.uint64)
            rc, _ = _loads(group, S, link, node, **kw)
            who, got, msg = _error(group)
            assert (rc, who, got) == (code, member, pair) and f"member {member}" in msg and word in msg, (rc, who, got, msg)
            assert (link == 5).all() and (node == 6).all()

        # a source host past the host table, in member 1 only
        parts = [_part(p[0]) for p in good]
        parts[1][0]["src"][77] = hosts["n"]
        fails(parts, _capi.SG_ERR_INVALID_ARG, 1, (77, UMAX), "source host")
        # bad packets in members 1 and 2: the lowest-numbered member is reported
        parts[2][0]["src"][3] = hosts["n"] + 9
        fails(parts, _capi.SG_ERR_INVALID_ARG, 1, (77, UMAX), "source host")
        # a source outside its member's block: member 0's first sender in member 1's batch
        parts = [_part(p[0]) for p in good]
        parts[1][0]["src"][40] = good[0][0]["src"][0]
        fails(parts, _capi.SG_ERR_INVALID_ARG, 1, (40, UMAX), "row")
        # a time overflow in member 2
        parts = [_part(p[0]) for p in good]
        parts[2][0]["send_time"][9] = np.uint64((1 << 64) - 1)
        fails(parts, _capi.SG_ERR_TIME_OVERFLOW, 2, (9, UMAX), "packet 9 ", trace_only=True)
        # a crossed pred cell of member 1: a value out of range at the first two-hop packet's destination
        r0, r1 = S.ranges[1]
        block = S.tabs[1][0]
        _, ri, cj = RR.counted_pairs(hosts, good[1][0], None)
        k = int(np.flatnonzero((ri != cj) & (block[ri - r0, cj] != ri))[0])
        i, j = int(ri[k]), int(cj[k])
        bad = block.copy()
        bad[i - r0, j] = 300
        want = RR.first_bad_pred(g, nodes, (r0, r1), bad, hosts, good[1][0])
        assert want is not None and want[0] == i
        rows = list(S.pred)
        rows[1] = _dev(bad)
        fails([_part(p[0]) for p in good], _capi.SG_ERR_INVALID_ARG, 1, want, "range", pred_rows=rows)
        # the same corruption in a cell no path of the row crosses succeeds
        crossed = np.zeros(300, bool)
        for c in cj[ri == i].tolist():
            v = c
            while v != i:
                crossed[v] = True
                v = int(block[i - r0, v])
        free = int(np.flatnonzero(~crossed & (np.arange(300) != i))[0])
        ok = block.copy()
        ok[i - r0, free] = 300
        assert RR.first_bad_pred(g, nodes, (r0, r1), ok, hosts, good[1][0]) is None
        rows[1] = _dev(ok)
        _load_parts(S, good)
        _check(group, S, GC.trace(g, nodes, 300, pred, tie["olat"], hosts, good), pred=rows)
        link = np.zeros(S.n_links, np.uint64)
        rc, _ = _loads(group, S, link, None, pred=rows)
        assert rc == _capi.SG_OK and group.last_error_member() is None


def test_argument_errors(tie):
    """(6): NULL arguments, a net or hosts of another member, graphs that differ, root >= n, no
    output at all, `nodes` not a permutation, a bad row range: SG_ERR_INVALID_ARG, no member named,
    every output as it was."""
    g, nodes, hosts = tie["g"], tie["nodes"], tie["hosts"]
    W = 3
    pk = {k: v[:1000] for k, v in tie["pk"].items()}
    with members(W) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(300, W))
        _load_parts(S, GC.split(hosts, pk, None, 300, W))
        other = keep(_net(LC.multi_graph(), ctxs[2]))
        dup = nodes.copy()
        dup[5] = 6
        swap = lambda xs: [xs[1], xs[0], xs[2]]  # noqa: E731
        variants = [dict(nets=swap(S.nets)), dict(hts=swap(S.hts)), dict(nets=[S.nets[0], S.nets[1], other]),
                    dict(nets=[S.nets[0], None, S.nets[2]]), dict(hts=[S.hts[0], None, S.hts[2]]), dict(nodes=dup),
                    dict(ranges=[S.ranges[0], (S.ranges[1][1], S.ranges[1][0]), S.ranges[2]]),
                    dict(ranges=[S.ranges[0], S.ranges[1], (S.ranges[2][0], 301)]), dict(root=W), dict(root=UMAX),
                    dict(pred=[S.pred[0], None, S.pred[2]])]
        outs = _sent(S.n_links, 8000)
        link, node = np.full(S.n_links, 5, np.uint64), np.full(300, 6, np.uint64)
        for kw in variants:
            rc, total = _trace(group, S, outs, 8000, **kw)
            assert rc == _capi.SG_ERR_INVALID_ARG and total == 0xDEAD and group.last_error_member() is None, kw
            rc, _ = _loads(group, S, link, node, **kw)
            assert rc == _capi.SG_ERR_INVALID_ARG and group.last_error_member() is None, kw
        # no output at all; no offsets; no total
        none = dict(outs, **{k: None for k in NAMES})
        assert _trace(group, S, none, 8000)[0] == _capi.SG_ERR_INVALID_ARG
        assert _trace(group, S, dict(outs, off=None), 8000)[0] == _capi.SG_ERR_INVALID_ARG
        assert _loads(group, S, None, None, hops=False)[0] == _capi.SG_ERR_INVALID_ARG
        # NULL lists
        L, a = _capi.load(), _common(S)
        held = [_dev(outs[k]) for k in KEYS]
        op = [C.c_void_p(t.data_ptr()) for t in held]
        T = C.byref(C.c_uint64())
        for hole in (0, 1, 2, 4, 5, 6):
            b = list(a)
            b[hole] = None
            assert L.sg_group_link_trace_packets(group.handle, *b, _ptrs(S.lat), S._live[1], None, None, None, 0, *op, 8000,
                                                 T) == _capi.SG_ERR_INVALID_ARG, hole
            assert L.sg_group_link_load_packets(group.handle, *b, S._live[1], None, None, 0, op[0], None,
                                                None) == _capi.SG_ERR_INVALID_ARG, hole
        assert L.sg_group_link_trace_packets(group.handle, *a, None, S._live[1], None, None, None, 0, *op, 8000,
                                             T) == _capi.SG_ERR_INVALID_ARG
        assert L.sg_group_link_trace_packets(group.handle, *a, _ptrs(S.lat), None, None, None, None, 0, *op, 8000,
                                             T) == _capi.SG_ERR_INVALID_ARG
        assert L.sg_group_link_trace_packets(group.handle, *a, _ptrs(S.lat), S._live[1], None, None, None, 0, *op, 8000,
                                             None) == _capi.SG_ERR_INVALID_ARG
        assert L.sg_group_link_load_packets(None, *a, S._live[1], None, None, 0, op[0], None, None) == _capi.SG_ERR_INVALID_ARG
        assert L.sg_group_last_error_member(None) == UMAX
        assert _untouched(outs) and (link == 5).all() and (node == 6).all()
        # and the group still works
        pred, _ = _full_tabs(S)
        _check(group, S, GC.trace(g, nodes, 300, pred, tie["olat"], hosts, S.parts))


@pytest.mark.parametrize("name", SC.NAMES)
def test_sweep(oracle, name):
    """(7): the 40 generated graphs over 3 members: the whole table's round with its mixed statuses,
    trace and loads."""
    c, r = SC.case(name), SC.refs(oracle, name)[0]
    g, nodes, hosts, v = c["g"], c["nodes"], c["hosts"], c["views"][0]
    n = g["n"]
    with members(3) as (ctxs, group, keep):
        S = _shard(ctxs, keep, g, nodes, hosts, GC.blocks(n, 3))
        pred, lat = _full_tabs(S)
        assert np.array_equal(pred, r["pred"]) and np.array_equal(lat, r["lat"])
        _load_parts(S, GC.split(hosts, v["pk"], v["status"], n, 3))
        _check(group, S, GC.trace(g, nodes, n, r["pred"], r["lat"], hosts, S.parts))
        link, node = np.full(S.n_links, 11, np.uint64), np.full(n, 12, np.uint64)
        weight = [p[0]["payload"] for p in S.parts]
        wl, wn, wh = _want_loads(S, hosts, r["pred"], weight, link, node)
        rc, hops = _loads(group, S, link, node, weight)
        assert rc == _capi.SG_OK, _error(group)
        assert np.array_equal(link, wl) and np.array_equal(node, wn) and all(np.array_equal(a, b) for a, b in zip(hops, wh))


def test_python_interface(tie):
    """(8): Group.link_trace_round / link_load_round from a GroupDelivery round's inputs and
    statuses; a total past the first sizing guess."""
    import torch

    from shadow_amd.worker import DeviceTable

    g, nodes, hosts, pk = tie["g"], tie["nodes"], tie["hosts"], tie["pk"]
    W = 3
    with members(W) as (ctxs, group, keep):
        graphs = [keep(_net(g, c)) for c in ctxs]
        tree = graphs[0].compute_shortest_path_tree()
        assert np.array_equal(tree.nodes, nodes) and np.array_equal(tree.latency_ns, tie["olat"])
        hts = [keep(_host_table(hosts, c)) for c in ctxs]
        ranges = GC.blocks(300, W)
        tables = [DeviceTable(torch.from_numpy(tree.latency_ns[r0:r1].view(np.int64).ravel().copy()).cuda(),
                              torch.from_numpy(tree.packet_loss[r0:r1].ravel().copy()).cuda(), 300, r0) for r0, r1 in ranges]
        parts = GC.split(hosts, pk, None, 300, W)
        batches = [_batch(p[0]) for p in parts]
        gd = GroupDelivery(group, hts, tables, HostPartition(hosts["route"], 300, W))
        out = gd.round(batches, RC.ROUND_END, 2**63, 0)
        torch.cuda.synchronize()
        status = [out[m][0].status[:len(batches[m])] for m in range(W)]
        st = [s.cpu().numpy() for s in status]
        assert all(0 < int((s == 0).sum()) < len(s) for s in st)
        ref_parts = [(p[0], s, p[2]) for p, s in zip(parts, st)]
        some = [5, 17, 400, 401, len(graphs[0].links()[0]) - 1]
        for watch in (None, some):
            got = group.link_trace_round(graphs, hts, tree, batches, status, watch=watch, root=1)
            want = GC.trace(g, nodes, 300, tree.pred, tie["olat"], hosts, ref_parts, watch=watch)
            for a, w, k in zip(got, want, KEYS):
                assert a.dtype == DTYPES[k] and np.array_equal(a, w), k
        link, node, hops = group.link_load_round(graphs, hts, tree, batches, status, weight="payload", root=2)
        cat, cstatus, bases = GC.concat(ref_parts)
        wl, wn, wh = RR.link_load_round(g, nodes, (0, 300), tree.pred, hosts, cat, cstatus, cat["payload"])
        assert np.array_equal(link, wl) and np.array_equal(node, wn) and np.array_equal(np.concatenate(hops), wh)
        with pytest.raises(ValueError):
            group.link_trace_round(graphs, hts, tree, batches, watch=[len(graphs[0].links()[0])])
    # more records than the first call's guess: the second call at the reported total; device rows
    gp = LC.path_graph(64)
    hp = synth.make_hosts(64, 64)
    with members(2) as (ctxs, group, keep):
        graphs = [keep(_net(gp, c)) for c in ctxs]
        tp = graphs[0].compute_shortest_path_tree([0, 1])
        hts = [keep(_host_table(hp, c)) for c in ctxs]
        parts = [(dict(src=np.full(20, m, np.uint32), dst_ip=np.full(20, hp["ip"][63], np.uint32),
                       payload=np.zeros(20, np.uint32), send_time=np.arange(20, 0, -1).astype(np.uint64)), None, None)
                 for m in range(2)]
        batches = [_batch(p[0]) for p in parts]
        rows = (tp.nodes, [(m, m + 1, _dev(tp.pred[m:m + 1]), _dev(tp.latency_ns[m:m + 1])) for m in range(2)])
        got = group.link_trace_round(graphs, hts, rows, batches)
        assert int(got[0][-1]) == 20 * 63 + 20 * 62 > 8 * 40 + 64
        want = GC.trace(gp, tp.nodes, 2, tp.pred, tp.latency_ns, hp, parts)
        for a, w in zip(got, want):
            assert np.array_equal(a, w)
        link, _, hops = group.link_load_round(graphs, hts, tp, batches)
        assert int(link.sum()) == 20 * 63 + 20 * 62 and (hops[0] == 63).all() and (hops[1] == 62).all()
