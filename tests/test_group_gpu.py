"""The device group on the card: N contexts of this one process, all on device 0 (which is legal
and all one card allows; peer access between devices is not reached here).

  * sg_group_routing_info_fill against sg_routing_info_fill on one context and against the
    oracle table: cells byte-identical, the wide side table, the errors one context would report;
  * sg_group_exchange_padded / sg_group_alltoallv_records against tests/group_ref.py;
  * GroupDelivery: the closed loop of tests/wire_sharded_cases.py (source -> stamp -> the group's
    exchange -> push -> pop -> inbound on every member) against the oracle chain, as
    tests/test_wire_sharded_gpu.py checks it for ranks emulated on one context.

Every context is made in the test and closed in a `finally`, after the objects created on it."""
import contextlib

import numpy as np
import pytest

import group_ref
import wire_cases as wc
import wire_sharded_cases as ws
from shadow_amd import (Context, Group, GroupDelivery, NetworkGraph, RoutingInfo, ShadowGpuError, _capi, synth)
from shadow_amd.dist import RECORD_DTYPE, row_range
from shadow_amd.wire import PacketWire
from shadow_amd.worker import DeviceTable, HostTable, PacketBatch, deliver_round
from test_wire_sharded_gpu import CAPACITY, POP_KEYS, STATE_KEYS, Rank, _dev, _np

pytestmark = pytest.mark.gpu
SHORTEST = _capi.SG_ROUTE_SHORTEST_PATH
WIDE_NS = 4_300_000_000  # latencies from here on do not fit a cell's 32 bits (SG_CELL_WIDE)


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


def _graphs(g, ctxs, keep):
    return [keep(NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=c)) for c in ctxs]


def _single(g, used, flags):
    """sg_routing_info_fill on one context of its own."""
    with members(1) as (ctxs, _, keep):
        ri = RoutingInfo(used.tolist())
        ri.fill(_graphs(g, ctxs, keep)[0], used, bool(flags & SHORTEST))
        return ri


def _oracle_table(oracle, g, used, shortest):
    fn = oracle.shortest_paths if shortest else oracle.direct_paths
    rc, lat, loss, _ = fn(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], used,
                          **(dict(threads=8) if shortest else {}))
    assert rc == 0
    return lat, loss


_tables = {}


def _case(oracle, name):
    """(graph, used nodes, flags, single-context RoutingInfo, oracle latency, oracle loss), once per
    module: the references are computed once and never written."""
    if name not in _tables:
        if name == "sparse":  # 301 used nodes (not a multiple of 2, 3 or 8), LDS search, shuffled order
            g = synth.ring_chords_graph(301, 6.0, seed=11)
            used = np.random.default_rng(2).permutation(301).astype(np.uint32)
            flags = SHORTEST
        elif name == "dense":  # mean out-degree 69 > 64: the dense search
            g = synth.complete_graph(70, seed=5)
            used, flags = np.arange(70, dtype=np.uint32), SHORTEST
            assert 2 * (len(g["src"]) - 70) > 64 * 70  # arcs, self-loops aside
        elif name == "direct":
            g = synth.complete_graph(70, seed=5)
            used, flags = np.arange(70, dtype=np.uint32), 0
        elif name == "two_nodes":  # 2 used nodes of a 30-node graph: with 3 members the last has no row
            g = synth.ring_chords_graph(30, 4.0, seed=3)
            used, flags = np.array([17, 4], np.uint32), SHORTEST
        else:
            raise KeyError(name)
        lat, loss = _oracle_table(oracle, g, used, bool(flags))
        _tables[name] = (g, used, flags, _single(g, used, flags), lat, loss)
    return _tables[name]


def _same_table(ri, single, lat, loss):
    assert ri.pinned
    assert np.array_equal(ri.cells, single.cells)  # byte-identical 8-byte cells
    got_lat, got_loss = ri.rows()
    assert np.array_equal(got_lat, lat) and np.array_equal(got_loss.view(np.uint32), loss.view(np.uint32))
    assert ri.get_smallest_latency_ns() == single.get_smallest_latency_ns() == int(lat.min())
    assert ri._view().n_wide == single._view().n_wide


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["sparse", "dense", "direct"])
def test_fill_equals_the_single_fill(oracle, name, n):
    g, used, flags, single, lat, loss = _case(oracle, name)
    with members(n) as (ctxs, group, keep):
        assert len(group) == n
        ri = RoutingInfo(used.tolist())
        ri.cells[:] = np.uint64(0xA5A5A5A5A5A5A5A5)  # a row no member wrote cannot pass
        group.fill(ri, _graphs(g, ctxs, keep), used, flags)
        _same_table(ri, single, lat, loss)


def test_fill_with_a_member_without_rows(oracle):
    g, used, flags, single, lat, loss = _case(oracle, "two_nodes")
    assert [row_range(2, 3, m)[:2] for m in range(3)] == [(0, 1), (1, 2), (2, 2)]
    with members(3) as (ctxs, group, keep):
        ri = group.fill_routing_info(_graphs(g, ctxs, keep), used.tolist())
        _same_table(ri, single, lat, loss)
        assert ri.node_ids == [17, 4] and ri.path(17, 4).latency_ns == int(lat[0, 1])


def test_fill_in_small_blocks(oracle, monkeypatch):
    """SG_RI_BLOCK_ROWS still sets the block size: 64-row blocks, so the 151 rows of a member take
    three blocks and both staging buffers are reused."""
    monkeypatch.setenv("SG_RI_BLOCK_ROWS", "64")
    g, used, flags, single, lat, loss = _case(oracle, "sparse")
    with members(2) as (ctxs, group, keep):
        ri = RoutingInfo(used.tolist())
        group.fill(ri, _graphs(g, ctxs, keep), used, flags)
        _same_table(ri, single, lat, loss)


def test_wide_cells_across_members(oracle):
    """A 12-node ring of 1.1 s arcs: every row holds paths of 4.4 s and more (4 to 6 hops), so with 3
    members each block adds entries to the wide side table, the second and third's included."""
    n = 12
    g = synth.ring_chords_graph(n, 2.0, seed=1, lat_lo_us=1_100_000, lat_hi_us=1_100_000)
    used = np.arange(n, dtype=np.uint32)
    lat, loss = _oracle_table(oracle, g, used, True)
    wide = lat >= WIDE_NS
    assert wide[4:8].any() and wide[8:12].any() and not wide.all()
    single = _single(g, used, SHORTEST)
    with members(3) as (ctxs, group, keep):
        ri = RoutingInfo(used.tolist())
        group.fill(ri, _graphs(g, ctxs, keep), used, SHORTEST)
        _same_table(ri, single, lat, loss)
        assert ri._view().n_wide == int(wide.sum()) > 0
        assert (ri.cells[wide] >> np.uint64(32) == 0xFFFFFFFF).all()
        for a in range(n):
            for b in range(n):
                p, q = ri.path(a, b), single.path(a, b)
                assert p.latency_ns == q.latency_ns == int(lat[a, b])
                assert np.float32(p.packet_loss).view(np.uint32) == loss.view(np.uint32)[a, b]


def _two_sinks(n, sinks, seed):
    """A directed graph, strongly connected but for the nodes of `sinks`, which keep their in-arcs
    and self-loops only: from a sink nothing else is reachable, every other pair is."""
    g = synth.ring_chords_graph(n, 6.0, seed=seed)
    s, d = g["src"], g["dst"]
    loop = s == d
    fs, fd = np.concatenate([s, d[~loop]]), np.concatenate([d, s[~loop]])
    lat, loss = np.concatenate([g["lat"], g["lat"][~loop]]), np.concatenate([g["loss"], g["loss"][~loop]])
    keep = ~(np.isin(fs, sinks) & (fs != fd))
    return dict(n=n, src=fs[keep], dst=fd[keep], lat=lat[keep], loss=loss[keep], directed=True)


def _fill_error(fill):
    with pytest.raises(ShadowGpuError) as e:
        fill()
    return e.value.code, str(e.value), e.value.pair


def test_fill_errors_are_the_single_fill_s(oracle):
    n = 100
    good = synth.ring_chords_graph(n, 6.0, seed=13)
    used = np.arange(n, dtype=np.uint32)
    blocks = [row_range(n, 3, m)[:2] for m in range(3)]
    assert blocks == [(0, 34), (34, 68), (68, 100)]
    # a node without a self-loop whose row lies in member 2's block
    keep_e = ~((good["src"] == 80) & (good["dst"] == 80))
    no_loop = dict(good, src=good["src"][keep_e], dst=good["dst"][keep_e], lat=good["lat"][keep_e],
                   loss=good["loss"][keep_e])
    # unreachable pairs in members 1 and 2's blocks only: rows 40 and 80 (the oracle names the first)
    sinks = _two_sinks(n, [40, 80], 13)
    rc, _, _, first = oracle.shortest_paths(n, sinks["src"], sinks["dst"], sinks["lat"], sinks["loss"], True, used,
                                            threads=8)
    assert rc == _capi.SG_ERR_UNREACHABLE and first == (40, 0)
    with members(3) as (ctxs, group, keep):
        lone = keep(Context(device=0))
        ri = RoutingInfo(used.tolist())
        for bad, code, pair in ((no_loop, _capi.SG_ERR_NO_EDGE, (80, 80)),
                                (sinks, _capi.SG_ERR_UNREACHABLE, (40, 0))):
            one = keep(NetworkGraph(bad["n"], bad["src"], bad["dst"], bad["lat"], bad["loss"], bad["directed"],
                                    ctx=lone))
            want = _fill_error(lambda: RoutingInfo(used.tolist()).fill(one, used, True))
            assert want[0] == code and want[2] == pair
            graphs = _graphs(bad, ctxs, keep)
            got = _fill_error(lambda: group.fill(ri, graphs, used, SHORTEST))
            assert got == want  # status, message and pair
            assert ri.get_smallest_latency_ns() is None  # not filled
        # the same group and object go on working
        graphs = _graphs(good, ctxs, keep)
        group.fill(ri, graphs, used, SHORTEST)
        lat, loss = _oracle_table(oracle, good, used, True)
        assert np.array_equal(ri.latency_ns, lat) and ri.get_smallest_latency_ns() == int(lat.min())
        # nets in the wrong order: nets[m] must be the graph on member m
        code, msg, _ = _fill_error(lambda: group.fill(ri, [graphs[1], graphs[0], graphs[2]], used, SHORTEST))
        assert code == _capi.SG_ERR_INVALID_ARG and "member 0" in msg
        assert ri.get_smallest_latency_ns() == int(lat.min())  # rejected before the object was touched
        # a graph that differs from member 0's
        other = _graphs(synth.ring_chords_graph(n, 4.0, seed=1), ctxs[2:], keep)
        code, msg, _ = _fill_error(lambda: group.fill(ri, graphs[:2] + other, used, SHORTEST))
        assert code == _capi.SG_ERR_INVALID_ARG and "nets[2]" in msg


# ---- the exchange ---------------------------------------------------------------------------
def _records(rng, n):
    r = np.zeros(n, RECORD_DTYPE)
    for k in ("deliver_time_ns", "order_key", "event_id"):
        r[k] = rng.integers(0, 2**63, n).astype(np.uint64)
    r["packet"], r["dst_host"] = rng.integers(0, 2**32, n), rng.integers(0, 2**32, n)
    return r


def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _on(ctx):
    """torch work enqueued on the member's own stream (not the default stream, which would order
    itself against every member)."""
    import torch

    return torch.cuda.stream(torch.cuda.ExternalStream(ctx.stream))


def test_exchange_padded_against_the_reference():
    """3 members, cap 4, counts 0, 1, 4 and 7 in one matrix (empty, partial, full, overflowing).  Three
    rounds on the same buffers: after each call every source's blocks and row are overwritten with the
    next round's, and every owner's result is copied aside and poisoned again, all on the members' own
    streams with no host synchronisation until the end."""
    import torch

    n, cap, rounds = 3, 4, 3
    counts = np.array([[0, 1, 4], [7, 4, 1], [1, 0, 7]], np.uint64)
    assert {0, 1, cap, 7} <= set(counts.ravel().tolist()) and 7 > cap
    rng = np.random.default_rng(5)
    send = [[_records(rng, n * cap) for _ in range(n)] for _ in range(rounds)]
    xrow = [[np.concatenate([rng.integers(0, 2**63, 3).astype(np.uint64), np.roll(counts, k, axis=0)[b]])
             for b in range(n)] for k in range(rounds)]
    poison = np.full(n * cap * 4, 0x5A5A5A5A5A5A5A5A, np.uint64).view(RECORD_DTYPE)
    with members(n) as (ctxs, group, _):
        staged = [[(_to_dev(send[k][b]), _to_dev(xrow[k][b])) for b in range(n)] for k in range(rounds)]
        d_send = [torch.empty_like(staged[0][b][0]) for b in range(n)]
        d_xrow = [torch.empty_like(staged[0][b][1]) for b in range(n)]
        d_poison = _to_dev(poison)
        d_recv = [d_poison.clone() for _ in range(n)]
        d_xall = [torch.zeros(n * (3 + n), dtype=torch.int64, device="cuda") for _ in range(n)]
        out = [[(torch.empty_like(d_recv[r]), torch.empty_like(d_xall[r])) for r in range(n)] for _ in range(rounds)]
        torch.cuda.synchronize()
        for k in range(rounds):
            for b in range(n):  # this round's blocks: the "source phase" on the source's stream
                with _on(ctxs[b]):
                    d_send[b].copy_(staged[k][b][0])
                    d_xrow[b].copy_(staged[k][b][1])
            group.exchange_padded(d_send, d_recv, cap, d_xrow, d_xall)
            for r in range(n):
                with _on(ctxs[r]):
                    out[k][r][0].copy_(d_recv[r])
                    out[k][r][1].copy_(d_xall[r])
                    d_recv[r].copy_(d_poison)
        for c in ctxs:
            c.synchronize()
        for k in range(rounds):
            want_recv, want_xall = group_ref.exchange_padded(send[k], xrow[k], cap, [poison] * n)
            for r in range(n):
                got = out[k][r][0].cpu().numpy().view(RECORD_DTYPE)
                assert np.array_equal(got, want_recv[r]), (k, r)  # valid slots and the poison elsewhere
                assert np.array_equal(out[k][r][1].cpu().numpy().view(np.uint64), want_xall[r]), (k, r)
        assert sum(int((out[0][r][0].cpu().numpy().view(RECORD_DTYPE) == poison).sum()) for r in range(n)) > 0


def test_exchange_padded_rejects_short_lists():
    import torch

    with members(2) as (ctxs, group, _):
        t = torch.zeros(2 * 4 * 4, dtype=torch.int64, device="cuda")
        x = torch.zeros(2 * 5, dtype=torch.int64, device="cuda")
        with pytest.raises(ValueError):
            group.exchange_padded([t], [t, t], 4, [x, x], [x, x])
        code, msg, _ = _fill_error(lambda: group._check(_capi.load().sg_group_exchange_padded(
            group.handle, None, None, 4, None, None)))
        assert code == _capi.SG_ERR_INVALID_ARG and "null" in msg


def test_alltoallv_records_against_the_reference():
    """3 members; member 1 sends nothing (a zero row) and nobody sends to member 1 (a zero column)."""
    import torch

    counts = np.array([[2, 0, 3], [0, 0, 0], [5, 0, 1]])
    rng = np.random.default_rng(6)
    send = [_records(rng, int(counts[b].sum())) for b in range(3)]
    want = group_ref.alltoallv(send, counts)
    with members(3) as (ctxs, group, _):
        d_send = [_to_dev(s) if len(s) else None for s in send]
        d_recv = [torch.full((max(len(w), 1) * 4 + 4,), -1, dtype=torch.int64, device="cuda") for w in want]
        group.alltoallv_records(d_send, counts, d_recv)
        for c in ctxs:
            c.synchronize()
        for r in range(3):
            got = d_recv[r].cpu().numpy()
            assert np.array_equal(got[:len(want[r]) * 4].view(RECORD_DTYPE), want[r]), r
            assert (got[len(want[r]) * 4:] == -1).all(), r  # nothing past the records


# ---- the closed loop on real contexts -------------------------------------------------------
def _ranks(ctxs, sc, part, keep, inbound=True):
    ranks = [Rank(ctxs[m], sc, part, m, len(ctxs), inbound=inbound) for m in range(len(ctxs))]
    for R in ranks:
        keep(R.ht), keep(R.wire)
        if inbound:
            keep(R.ib)
    return ranks


def _round(gd, ranks, sc, k, check_status=True, **kw):
    rd = sc["rounds"][k]
    b = [R.batch(k) for R in ranks]  # (rows of the round's batch, PacketBatch, len, packet ids)
    out = gd.round([x[1] for x in b], rd["end"], wc.SIM_END, 0, wires=[R.wire for R in ranks],
                   lengths=[x[2] for x in b], packet_ids=[x[3] for x in b], **kw)
    if check_status:
        want = rd["want"]
        for (sel, _, _, _), (res, recv_counts, stats) in zip(b, out):
            assert np.array_equal(res.status[:len(sel)].cpu().numpy(), want["status"][sel])
            assert stats == (want["delivered"], want["min_deliver"], want["min_lat"])
    return out


def _final_state(ranks, sc):
    for R in ranks:
        assert len(R.wire.get_state()["host"]) == 0 and R.wire.count == 0
        rng, ctr = R.ht.get_state()
        assert np.array_equal(rng[R.mine], sc["rng_end"][R.mine])  # the hosts this member sends for
        assert np.array_equal(ctr[R.mine], sc["rounds"][-1]["ctr"][R.mine])


@pytest.mark.parametrize("W", [1, 2, 3])
def test_closed_loop_exact(oracle, W):
    """Every member's pops equal rank_pop; fates, forward times and event counters follow the oracle
    chain (Rank.pop / Rank.inbound assert them round by round); the streams end where the oracle's do."""
    sc = wc.scenario(oracle)
    part = ws.partition(sc, W)
    counts = ws.pair_counts(sc, part)
    with members(W) as (ctxs, group, keep):
        ranks = _ranks(ctxs, sc, part, keep)
        gd = GroupDelivery(group, [R.ht for R in ranks], [R.table for R in ranks], part)
        for k in range(wc.ROUNDS):
            if k < wc.SEND_ROUNDS:
                out = _round(gd, ranks, sc, k)
                assert gd.last_mode == "exact" and np.array_equal(gd.last_counts, counts[k])
                assert [o[1] for o in out] == [counts[k][:, d].tolist() for d in range(W)]
            for R in ranks:
                R.inbound(k, R.pop(k))
        _final_state(ranks, sc)


def test_closed_loop_padded(oracle):
    """Round 0 exact, then blocks of the cap tests/test_wire_sharded_cpu.py fixes: about half the
    rounds overflow it and go through alltoallv_records, the others through the pull alone."""
    W = ws.PADDED_W
    sc = wc.scenario(oracle)
    part = ws.partition(sc, W)
    cap, counts = ws.padded_cap(sc), ws.pair_counts(sc, part)
    modes = []
    with members(W) as (ctxs, group, keep):
        ranks = _ranks(ctxs, sc, part, keep)
        gd = GroupDelivery(group, [R.ht for R in ranks], [R.table for R in ranks], part, padded=True)
        for k in range(wc.ROUNDS):
            if k < wc.SEND_ROUNDS:
                if k:
                    gd.cap = cap
                _round(gd, ranks, sc, k)
                assert np.array_equal(gd.last_counts, counts[k])
                want = "exact" if k == 0 else "padded+exact" if counts[k].max() > cap else "padded"
                assert gd.last_mode == want, k
                modes.append(gd.last_mode)
            for R in ranks:
                R.inbound(k, R.pop(k))
        _final_state(ranks, sc)
    assert modes.count("padded") > 0 and modes.count("padded+exact") > 0


def test_one_member_equals_the_single_gpu_push(oracle):
    sc = wc.scenario(oracle)
    rd, h = sc["rounds"][0], sc["hosts"]
    pk = rd["pk"]
    with members(1) as (ctxs, group, keep):
        # path A: sg_deliver_round + sg_wire_push
        ht = keep(HostTable(h["ip"], h["route"], h["seed"], ctx=ctxs[0]))
        table = DeviceTable(_dev(sc["lat"].ravel(), np.uint64, np.int64),
                            _dev(sc["loss"].ravel(), np.float32, np.float32), wc.H)
        batch = PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"])
        out = deliver_round(ht, table, batch, rd["end"], wc.SIM_END, 0, ctx=ctxs[0])
        a = keep(PacketWire(wc.H, CAPACITY, wc.MS, 16, ctx=ctxs[0]))
        a.push(batch, out, _dev(pk["len"], np.uint32, np.int32), id_base=rd["id_base"] + 7)
        # path B: a group of one
        (R,) = _ranks(ctxs, sc, ws.partition(sc, 1), keep, inbound=False)
        gd = GroupDelivery(group, [R.ht], [R.table], R.part)
        sel, b, length, _ = R.batch(0)
        gd.round([b], rd["end"], wc.SIM_END, 0, wires=[R.wire], lengths=[length], id_bases=rd["id_base"] + 7)
        sa, sb = a.get_state(), R.wire.get_state()
        assert len(sa["host"]) == rd["want"]["delivered"] > 0
        for key in STATE_KEYS:
            assert np.array_equal(sa[key], sb[key]), key


def test_bucketing_without_a_wire(oracle):
    """Without wires the owners bucket what they received: every member's buckets hold the oracle's
    delivery order of the hosts it owns, in an exact round and in a padded one."""
    W = 3
    sc = wc.scenario(oracle)
    part = ws.partition(sc, W)
    with members(W) as (ctxs, group, keep):
        ranks = _ranks(ctxs, sc, part, keep, inbound=False)
        gd = GroupDelivery(group, [R.ht for R in ranks], [R.table for R in ranks], part, padded=True)
        for k in range(2):
            rd = sc["rounds"][k]
            b = [R.batch(k) for R in ranks]
            out = gd.round([x[1] for x in b], rd["end"], wc.SIM_END, 0)
            assert gd.last_mode == ("exact", "padded")[k]
            want = rd["want"]
            off, order = want["dst_offsets"].astype(np.int64), want["dst_order"].astype(np.int64)
            for d, (res, recv, recv_counts, got_order, got_off) in enumerate(out):
                rec = recv.cpu().numpy().view(RECORD_DTYPE).ravel()[got_order.cpu().numpy().astype(np.int64)]
                goff = got_off.cpu().numpy().astype(np.int64)
                assert goff[-1] == len(rec) == sum(recv_counts)
                for slot, host in enumerate(part.hosts_of[d]):
                    w = order[off[host]:off[host + 1]]
                    seg = rec[goff[slot]:goff[slot + 1]]
                    assert (seg["dst_host"] == host).all() and len(seg) == len(w), (k, d, host)
                    assert np.array_equal(seg["event_id"], want["event_id"][w])
                    assert np.array_equal(seg["deliver_time_ns"], want["deliver_time"][w])


def test_one_member_s_batch_error(oracle):
    """An unsorted batch on member 1 of 3 in a padded wire round: member 1's pop returns SG_ERR_UNSORTED
    once, nothing of its batch was delivered, and the other members' rounds are complete."""
    W = 3
    sc = wc.scenario(oracle)
    part = ws.partition(sc, W)
    counts = ws.pair_counts(sc, part)
    with members(W) as (ctxs, group, keep):
        ranks = _ranks(ctxs, sc, part, keep, inbound=False)
        gd = GroupDelivery(group, [R.ht for R in ranks], [R.table for R in ranks], part, padded=True)
        _round(gd, ranks, sc, 0)
        for R in ranks:
            R.pop(0)
        held = [len(R.wire.get_state()["host"]) for R in ranks]
        state1 = ranks[1].ht.get_state()
        rd = sc["rounds"][1]
        b = [R.batch(1) for R in ranks]
        sel1 = b[1][0][::-1].copy()  # member 1's rows of the batch, last host first
        assert (np.diff(rd["pk"]["src"][sel1].astype(np.int64)) < 0).any()
        pk = rd["pk"]
        b[1] = (sel1, PacketBatch.from_numpy(pk["src"][sel1], pk["dst_ip"][sel1], pk["payload"][sel1],
                                             pk["send_time"][sel1]),
                _dev(pk["len"][sel1], np.uint32, np.int32), _dev(rd["id_base"] + sel1, np.uint32, np.int32))
        out = gd.round([x[1] for x in b], rd["end"], wc.SIM_END, 0, wires=[R.wire for R in ranks],
                       lengths=[x[2] for x in b], packet_ids=[x[3] for x in b])
        assert gd.last_mode == "padded"  # no call has failed yet
        want_counts = counts[1].copy()
        want_counts[1] = 0
        assert np.array_equal(gd.last_counts, want_counts)
        for m in (0, 2):
            assert np.array_equal(out[m][0].status[:len(b[m][0])].cpu().numpy(), rd["want"]["status"][b[m][0]])
        popped = []
        for m, R in enumerate(ranks):
            want, nxt = ws.rank_pop(sc, part, m, 1)  # round 1 delivers at or after its end: round 0's events
            if m == 1:
                with pytest.raises(ShadowGpuError) as e:
                    R.wire.pop(rd["end"])
                assert e.value.code == _capi.SG_ERR_UNSORTED
                got = e.value.arrivals  # the pop itself was complete
            else:
                got = R.wire.pop(rd["end"])
            assert got["n"] == len(want["host"]) > 0
            for key in POP_KEYS:
                assert np.array_equal(_np(got[key], key), want[key]), (m, key)
            popped.append(got["n"])
        assert ranks[1].wire.pop(rd["end"])["n"] == 0  # reported once
        for a, b_ in zip(state1, ranks[1].ht.get_state()):
            assert np.array_equal(a, b_)  # the rejected batch drew nothing
        for d, R in enumerate(ranks):  # every owner holds the round's records of members 0 and 2
            assert len(R.wire.get_state()["host"]) == held[d] - popped[d] + int(want_counts[:, d].sum()), d
