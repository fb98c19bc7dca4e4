"""The generated family of tests/sweep_cases.py through every routing stage on the GPU, table to
hop records; the table builds on graphs that are not one strongly connected piece; and the
hop-record scan's second trip.

Every comparison is exact (np.array_equal, f32 losses by their bits) against references that
exist already: the oracle for tables, tests/tree_ref.py, tests/link_ref.py,
tests/link_round_ref.py and tests/paths_ref.py for the rest.  Each later stage reads the
references' rows, not the stage before it: a wrong table fails the table check alone.  The
inputs' own conditions are checked on the CPU in test_sweep_ref_cpu.py.

The six seam cases of sweep_cases.EXTRA (tests/seam_cases.py: optima of exactly 2^32 - 4 ..
2^32 + 1 ns, two of them dense graphs; test_seam_ref_cpu.py) run through the same stages; on an
MI355X each takes 0.07-0.23 s."""
import time

import numpy as np
import pytest

import link_ref as LR
import link_round_cases as RC
import paths_cases as PC
import paths_ref as PR
import sweep_cases as SC
import tree_cases as TC
import tree_ref as TR
from conftest import APSP_KERNELS, APSP_OPTIONS, set_apsp_kernel

pytestmark = pytest.mark.gpu

ALL_KERNELS = APSP_KERNELS + [k for k in APSP_OPTIONS if k not in APSP_KERNELS]
SENT64, SENT32 = RC.SENT64, RC.SENT32
PAD = 3  # sentinel records past the total
VIEW = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64,
        np.dtype(np.float32): np.float32}


def _net(g, ctx):
    from shadow_amd import NetworkGraph

    return NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)


def _d(x):
    import torch

    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(VIEW[x.dtype]).copy()).cuda()


def _h(t, dtype):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_table(got_lat, got_loss, lat, loss, what):
    assert np.array_equal(got_lat, lat), f"{what}: latency differs in {int((got_lat != lat).sum())} cells"
    assert np.array_equal(_bits(got_loss), _bits(loss)), f"{what}: loss differs in {int((_bits(got_loss) != _bits(loss)).sum())} cells"


def _rows_device(net, used, r0, r1):
    """Rows [r0, r1) through build_rows_device, copied back."""
    import torch

    dlat = torch.full((r1 - r0, len(used)), -1, dtype=torch.int64, device="cuda")
    dloss = torch.full((r1 - r0, len(used)), -7.5, dtype=torch.float32, device="cuda")
    net.build_rows_device(used, r0, r1, dlat.data_ptr(), dloss.data_ptr())
    return _h(dlat, np.uint64), _h(dloss, np.float32)


# ---- the stages of one case ---------------------------------------------------------------------
def _tables(net, c, rs, monkeypatch):
    g, nodes = c["g"], c["nodes"]
    variants = [(k, {}) for k in APSP_KERNELS] + ([("lds", {"SG_DENSE_LAZY": "0"})] if SC.dense(g) else [])
    for kernel, env in variants:
        set_apsp_kernel(monkeypatch, kernel)
        for k, x in env.items():
            monkeypatch.setenv(k, x)
        t = net.compute_shortest_paths(nodes)
        _same_table(t.latency_ns, t.packet_loss, rs[0]["lat"], rs[0]["loss"], f"table, {kernel} {env}")
        for v, r in zip(c["views"][1:], rs[1:]):
            lat, loss = _rows_device(net, nodes, *v["rows"])
            _same_table(lat, loss, r["lat"], r["loss"], f"rows {v['rows']}, {kernel} {env}")
        for k in env:
            monkeypatch.delenv(k)
    set_apsp_kernel(monkeypatch, "lds")


def _trees(net, c, v, r, d, monkeypatch):
    import torch

    (r0, r1), n = v["rows"], c["g"]["n"]
    for lds in ("1", "0"):
        monkeypatch.setenv("SG_TREE_LDS", lds)
        dpred = torch.full((r1 - r0, n), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        dhop = torch.full((r1 - r0, n), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        net.tree_rows_device(c["nodes"], r0, r1, d["lat"].data_ptr(), d["loss"].data_ptr(), dpred.data_ptr(), dhop.data_ptr())
        pred, hop = _h(dpred, np.uint32), _h(dhop, np.uint32)
        assert np.array_equal(pred, r["pred"]), f"trees, SG_TREE_LDS={lds}: pred differs in {int((pred != r['pred']).sum())} cells"
        assert np.array_equal(hop, r["hop"]), f"trees, SG_TREE_LDS={lds}: first_hop differs in {int((hop != r['hop']).sum())} cells"
    monkeypatch.delenv("SG_TREE_LDS")


def _link_loads(net, c, v, r, d, n_links, monkeypatch):
    import torch

    (r0, r1), n = v["rows"], c["g"]["n"]
    assert len(r["link"]) == n_links
    dcounts = _d(v["counts"])
    for lds in ("1", "0"):
        monkeypatch.setenv("SG_LINK_LDS", lds)
        dlink, dnode = _d(np.full(n_links, SENT64, np.uint64)), _d(np.full(n, SENT64, np.uint64))
        net.link_load_device(c["nodes"], r0, r1, d["pred"].data_ptr(), dcounts.data_ptr(), n, dlink.data_ptr(), dnode.data_ptr())
        with np.errstate(over="ignore"):
            assert np.array_equal(_h(dlink, np.uint64), r["link"] + SENT64), f"link loads, SG_LINK_LDS={lds}"
            assert np.array_equal(_h(dnode, np.uint64), r["node"] + SENT64), f"node loads, SG_LINK_LDS={lds}"
    monkeypatch.delenv("SG_LINK_LDS")


def _round_loads(net, c, v, r, d, n_links, monkeypatch):
    (r0, r1), n = v["rows"], c["g"]["n"]
    pk, npk = v["pk"], len(v["pk"]["src"])
    for weight in (None, pk["payload"]):
        for status in (None, v["status"]):
            wl, wn, wh = SC.round_refs(c, v, r, status, weight)
            for combine in ("1", "0"):
                monkeypatch.setenv("SG_LINK_COMBINE", combine)
                what = f"SG_LINK_COMBINE={combine}, weights {weight is not None}, status {status is not None}"
                dlink, dnode = _d(np.full(n_links, SENT64, np.uint64)), _d(np.full(n, SENT64, np.uint64))
                dhops = _d(np.full(npk, SENT32, np.uint32))
                net.link_load_packets_device(d["ht"], c["nodes"], r0, r1, d["pred"].data_ptr(), d["pb"],
                                             0 if status is None else d["status"].data_ptr(),
                                             0 if weight is None else d["pb"].payload_len.data_ptr(), dlink.data_ptr(),
                                             dnode.data_ptr(), dhops.data_ptr())
                with np.errstate(over="ignore"):
                    assert np.array_equal(_h(dlink, np.uint64), wl + SENT64), f"round link loads, {what}"
                    assert np.array_equal(_h(dnode, np.uint64), wn + SENT64), f"round node loads, {what}"
                assert np.array_equal(_h(dhops, np.uint32), wh), f"round hops, {what}"
    monkeypatch.delenv("SG_LINK_COMBINE")


def _records(call, n_items, want, what):
    """One hop-record call from sentinels at cap = the total: (off, node, link, lat, loss) equal
    the reference's and the tails past the total are still sentinels.  Returns the arrays."""
    total = int(want[0][-1])
    cap = total + PAD
    outs = [_d(np.full(n_items + 1, PC.SENT_OFF, np.uint64)), _d(np.full(cap, PC.SENT32, np.uint32)),
            _d(np.full(cap, PC.SENT32, np.uint32)), _d(np.full(cap, PC.SENT_LAT, np.uint64)),
            _d(np.full(cap, PC.SENT_LOSS, np.float32))]
    got_total = call(*[t.data_ptr() for t in outs], total)
    assert got_total == total, f"{what}: total {got_total}, want {total}"
    got = [_h(t, dt) for t, dt in zip(outs, (np.uint64, np.uint32, np.uint32, np.uint64, np.float32))]
    assert np.array_equal(got[0], want[0]), f"{what}: offsets differ"
    sent = (None, PC.SENT32, PC.SENT32, PC.SENT_LAT, PC.SENT_LOSS)
    for k, name in ((1, "node"), (2, "link"), (3, "latency"), (4, "loss")):
        a, w = got[k], want[k]
        assert np.array_equal(a[:total].view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), \
            f"{what}: {name} differs in {int((a[:total] != w).sum())} of {total} records"
        assert (a[total:].view(np.uint8) == np.full(PAD, sent[k]).view(np.uint8)).all(), f"{what}: {name} written past the total"
    return got


def _hop_records(net, c, v, r, d, monkeypatch):
    g, nodes, (r0, r1) = c["g"], c["nodes"], v["rows"]
    ri, cj = v["pairs"]
    dri, dcj = _d(ri), _d(cj)
    want_pk = PR.packet_records(g, nodes, v["rows"], r["pred"], r["lat"], r["loss"], c["hosts"], v["pk"], v["status"])
    tabs = (d["pred"].data_ptr(), d["lat"].data_ptr(), d["loss"].data_ptr())
    got = None
    for stage, hops in (("0", None), ("1", None), ("1", "64")):
        monkeypatch.setenv("SG_PATHS_STAGE", stage)
        if hops is None:
            monkeypatch.delenv("SG_PATHS_STAGE_HOPS", raising=False)
        else:
            monkeypatch.setenv("SG_PATHS_STAGE_HOPS", hops)
        what = f"SG_PATHS_STAGE={stage}, SG_PATHS_STAGE_HOPS={hops}"
        got = _records(lambda *o: net.tree_paths_device(nodes, r0, r1, *tabs, len(ri), dri.data_ptr(), dcj.data_ptr(), *o),
                       len(ri), r["records"], f"pair records, {what}")
        _records(lambda *o: net.tree_paths_packets_device(d["ht"], nodes, r0, r1, *tabs, d["pb"], d["status"].data_ptr(), *o),
                 len(v["pk"]["src"]), want_pk, f"packet records, {what}")
    monkeypatch.delenv("SG_PATHS_STAGE")
    monkeypatch.delenv("SG_PATHS_STAGE_HOPS")
    return got


def _folds(net, c, v, r, got):
    """Leaning on no reference's walk: along 200 sampled pairs' records, each (latency, loss) is
    the record before it folded with some arc of the record's link, from (0, +0.0); the last
    record is the table's cell.  A same-node pair's one record is its self-loop, the diagonal cell."""
    g, nodes, (r0, _) = c["g"], c["nodes"], v["rows"]
    off, node, link, lat, loss = got
    tail, head = net.links()
    idx = TR.build_arc_index(g)
    loops = {int(a): (int(w), f) for a, b, w, f in zip(g["src"], g["dst"], g["lat"], g["loss"]) if a == b}
    ri, cj = v["pairs"]
    for p in range(SC.SAMPLE):
        a, b = int(off[p]), int(off[p + 1])
        s, dst = int(nodes[ri[p]]), int(nodes[cj[p]])
        assert b > a and node[b - 1] == dst
        assert lat[b - 1] == r["lat"][ri[p] - r0, cj[p]] and _bits(loss[b - 1:b])[0] == _bits(r["loss"][ri[p] - r0, cj[p]:cj[p] + 1])[0]
        if s == dst:
            assert b - a == 1 and (tail[link[a]], head[link[a]]) == (s, s)
            assert (int(lat[a]), _bits(loss[a:b])[0]) == (loops[s][0], _bits(np.float32([loops[s][1]]))[0])
            continue
        at, cur_lat, cur_loss = s, 0, np.float32(0.0)
        for k in range(a, b):
            assert tail[link[k]] == at and head[link[k]] == node[k], (p, k)
            ok = [w for w, om in idx.get((at, int(node[k])), ())
                  if cur_lat + w == int(lat[k]) and _bits(np.float32([TR.fold(cur_loss, om)]))[0] == _bits(loss[k:k + 1])[0]]
            assert ok, f"pair {p}, record {k - a}: no arc of its link folds the record before it into it"
            at, cur_lat, cur_loss = int(node[k]), int(lat[k]), loss[k]


@pytest.mark.parametrize("name", SC.NAMES)
def test_table_to_hop_records(oracle, ctx, monkeypatch, name):
    from shadow_amd.worker import HostTable, PacketBatch

    c, rs = SC.case(name), SC.refs(oracle, name)
    net = _net(c["g"], ctx)
    n_links = len(net.links()[0])
    assert np.array_equal(np.stack(net.links()), np.stack(LR.links(c["g"])[:2]))
    _tables(net, c, rs, monkeypatch)
    hosts = c["hosts"]
    ht = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    for v, r in zip(c["views"], rs):
        pk = v["pk"]
        d = dict(lat=_d(r["lat"]), loss=_d(r["loss"]), pred=_d(r["pred"]), status=_d(v["status"]), ht=ht,
                 pb=PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"]))
        _trees(net, c, v, r, d, monkeypatch)
        _link_loads(net, c, v, r, d, n_links, monkeypatch)
        _round_loads(net, c, v, r, d, n_links, monkeypatch)
        got = _hop_records(net, c, v, r, d, monkeypatch)
        _folds(net, c, v, r, got)


# ---- graphs that are not one strongly connected piece -------------------------------------------
_ORACLE = {}


def _want(oracle, key, g, used, rows=None):
    if key not in _ORACLE:
        _ORACLE[key] = SC.oracle_rows(oracle, g, used, rows)
    return _ORACLE[key]


def _build(net, used, rows):
    """The whole table to host arrays, or a row block to device arrays: (latency, loss)."""
    if rows is None:
        t = net.compute_shortest_paths(used)
        return t.latency_ns, t.packet_loss
    return _rows_device(net, used, *rows)


def _succeeds(oracle, nets, name, g, used, rows, what):
    rc, lat, loss, _ = _want(oracle, name, g, used, rows)
    assert rc == 0
    _same_table(*_build(nets(g), used, rows), lat, loss, f"{name}, {what}")


def _fails_then_builds(oracle, nets, name, what):
    """The failing build `name` reports the oracle's first pair; the valid build after it, with a
    used list of the other kind, on the same net or a second one, equals the oracle."""
    from shadow_amd import RoutingInfo, ShadowGpuError, _capi

    g, used, rows = SC.error_cases()[name]
    rc, _, _, first = _want(oracle, name, g, used, rows)
    assert rc == oracle.ERR_UNREACHABLE
    builds = [lambda: _build(nets(g), used, rows)]
    if rows is None:
        builds.append(lambda: RoutingInfo(used.tolist()).fill(nets(g), used, True))
    g2, used2 = SC.follow_up(name)
    for build in builds:
        with pytest.raises(ShadowGpuError) as e:
            build()
        assert e.value.code == _capi.SG_ERR_UNREACHABLE and e.value.pair == first, (name, what, e.value.pair, first)
        _succeeds(oracle, nets, name + "_then", g2 or g, used2, None, what)


@pytest.fixture
def nets(ctx):
    """One net per graph on the shared context, kept for the test."""
    made = {}

    def get(g):
        if id(g) not in made:
            made[id(g)] = (g, _net(g, ctx))
        return made[id(g)][1]

    return get


@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_unused_nodes_out_of_reach(oracle, nets, monkeypatch, kernel):
    """S1, S2, D: unreachable nodes that no used pair needs, at sizes where the plan, its bound
    and chained rows, the landmarks, the dense search and the bucket ring run: the build succeeds."""
    set_apsp_kernel(monkeypatch, kernel)
    for name, (g, used, rows) in SC.split_cases().items():
        _succeeds(oracle, nets, name, g, used, rows, kernel)


@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_used_pairs_out_of_reach(oracle, nets, monkeypatch, kernel):
    """E1, E2, D: SG_ERR_UNREACHABLE with the oracle's pair, and a clean start for the build
    that follows on the same context."""
    set_apsp_kernel(monkeypatch, kernel)
    for name in SC.error_cases():
        _fails_then_builds(oracle, nets, name, kernel)


@pytest.mark.parametrize("env", [{}, {"SG_DENSE_LAZY": "0"}, {"SG_APSP_DENSE": "0"}], ids=["lazy", "tcut", "slab"])
def test_dense_blocks(oracle, nets, monkeypatch, env):
    """D under the default dense search, the T-cut search with seed rows, and without the dense
    search."""
    set_apsp_kernel(monkeypatch, "lds")
    for k, x in env.items():
        monkeypatch.setenv(k, x)
    for name, (g, used, rows) in SC.split_cases().items():
        if name.startswith("D_"):
            _succeeds(oracle, nets, name, g, used, rows, str(env))
    for name in ("D_identity", "D_shuffled"):
        _fails_then_builds(oracle, nets, name, str(env))


# ---- the hop-record scan's second trip ----------------------------------------------------------
@pytest.fixture(scope="module")
def scan(oracle):
    """The 64-node multigraph's pred rows and the vectorised walk of 1,024 x 2,048 + 1 pairs."""
    g = TC.multi_graph()
    nodes = np.arange(64, dtype=np.uint32)
    rc, lat, loss, _ = SC.oracle_rows(oracle, g, nodes)
    assert rc == 0
    pred, _, bad = TR.tree_ref(g, nodes, (0, 64), lat, loss)
    assert bad is None
    ri, cj = SC.scan_pairs(64)
    return dict(g=g, nodes=nodes, pred=pred, ri=ri, cj=cj, want=SC.walk_records(g, nodes, (0, 64), pred, ri, cj))


@pytest.mark.parametrize("stage", ["1", "0"])
def test_scan_second_trip(ctx, monkeypatch, scan, stage):
    """The scan's one-workgroup kernel over the block sums (k_scan_sums, sg_scan.hip; the link
    trace's scan too) carries its total from the first 1,024 block sums into the 1,025th tile,
    whose only item is the last pair (a same-node pair: one record)."""
    monkeypatch.setenv("SG_PATHS_STAGE", stage)
    off, node, link = scan["want"]
    total, n_pairs = int(off[-1]), len(scan["ri"])
    assert n_pairs == SC.SCAN_TRIP * SC.SCAN_TILE + 1 and total - int(off[-2]) == 1
    net = _net(scan["g"], ctx)
    dpred, dri, dcj = _d(scan["pred"]), _d(scan["ri"]), _d(scan["cj"])
    doff = _d(np.full(n_pairs + 1, PC.SENT_OFF, np.uint64))
    dnode, dlink = _d(np.full(total + PAD, PC.SENT32, np.uint32)), _d(np.full(total + PAD, PC.SENT32, np.uint32))
    t0 = time.perf_counter()
    got_total = net.tree_paths_device(scan["nodes"], 0, 64, dpred.data_ptr(), 0, 0, n_pairs, dri.data_ptr(), dcj.data_ptr(),
                                      doff.data_ptr(), dnode.data_ptr(), dlink.data_ptr(), 0, 0, total)
    got_off = _h(doff, np.uint64)
    print(f"scan: {n_pairs} pairs, {got_total} records, SG_PATHS_STAGE={stage}, {time.perf_counter() - t0:.3f} s")
    assert got_total == total
    assert np.array_equal(got_off, off), f"offsets differ, the first at item {int(np.flatnonzero(got_off != off)[:1].sum())}"
    for name, t, w in (("node", dnode, node), ("link", dlink, link)):
        a = _h(t, np.uint32)
        assert np.array_equal(a[:total], w), f"{name} differs in {int((a[:total] != w).sum())} of {total} records"
        assert (a[total:] == PC.SENT32).all(), f"{name}: written past the total"
