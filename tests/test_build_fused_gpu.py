"""The one-shot build's shortened launch chain (SG_BUILD_FUSED, default 1): an identity used
list written by the build's first kernel instead of copied (sg_routing.hip flush_used,
sg_plan.hip k_plan_rel), the phased plan's bound rows and the self-loop check launched beside
phase 0 on the context's side stream (sg_plan.hip sssp_plan_bounds_side; timers off, no
landmarks, not the flagged launch), and no kernel at the build's end there.

Every case is built into zero-poisoned device buffers with the switch on and with it off (the
launch chain as it was) and every cell of both tables compared with the CPU oracle (latency by
value, loss by bit), so the two tables are byte-identical; a graph the reference rejects must
raise the oracle's code and pair, and the same message, under both settings.
"""
import numpy as np
import pytest

import plan_cases as C
from conftest import set_apsp_kernel
from shadow_amd import NetworkGraph, ShadowGpuError, _capi, synth
from test_sssp_chain_gpu import _build, _same
from test_sssp_plan_gpu import KNOBS, PHASES_MAX, _check_plan, _graph

pytestmark = pytest.mark.gpu

NET_LDS_NODES = 4096  # sg_net.hip: up to here the upload counts in LDS (SG_NET_LDS=1)


def _g(n, src, dst, directed=False, seed=3):
    """A graph over the given endpoints: latencies of 1-4 us (equal-latency paths), 60 % zero-loss."""
    g = dict(n=n, src=np.asarray(src, dtype=np.uint32), dst=np.asarray(dst, dtype=np.uint32), directed=directed,
             lat=np.zeros(len(src), dtype=np.uint64), loss=np.zeros(len(src), dtype=np.float32))
    return C.ties(g, seed)


def _loops(n):
    return list(range(n))


def _env(monkeypatch, net_lds="1", seeds="1", **knobs):
    set_apsp_kernel(monkeypatch, "lds")
    monkeypatch.setenv("SG_SSSP_SEEDS", seeds)
    if seeds == "2":
        monkeypatch.setenv("SG_SSSP_FLAGGED", "0")
    monkeypatch.setenv("SG_NET_LDS", net_lds)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))


def _both(oracle, ctx, monkeypatch, g, used=None, rows=None):
    """The block under SG_BUILD_FUSED=1 and =0 against the oracle; an error the oracle raises must
    come out of both builds alike.  Returns the error (or None)."""
    used = np.arange(g["n"], dtype=np.uint32) if used is None else np.asarray(used, dtype=np.uint32)
    rows = rows or (0, len(used))
    rc, lat, loss, pair = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], used,
                                                rows=rows, threads=8)
    errs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("SG_BUILD_FUSED", fused)
        if rc == 0:
            _same(_build(g, used, rows, ctx), (lat, loss))
            continue
        with pytest.raises(ShadowGpuError) as e:
            _build(g, used, rows, ctx)
        assert (e.value.code, e.value.pair) == (rc, pair), (fused, e.value.code, e.value.pair, str(e.value))
        errs.append(str(e.value))
    if rc == 0:
        return None
    assert errs[0] == errs[1]
    return errs[0]


# ---- a. graphs of every upload path (every node used, in order: the identity list)

def _star65():
    return _g(65, _loops(65) + [0] * 64, _loops(65) + list(range(1, 65)), seed=65)


def _isolated():
    """Nodes 40..49 carry a self-loop and nothing else; the used nodes are the connected ones."""
    r = synth.ring_chords_graph(40, 5.0, seed=8)
    g = _g(50, list(r["src"]) + list(range(40, 50)), list(r["dst"]) + list(range(40, 50)), seed=8)
    return g, np.arange(40, dtype=np.uint32)


SMALL_GRAPHS = {
    "two_nodes": lambda: (_g(2, [0, 1, 0], [0, 1, 1]), None),
    "star65": lambda: (_star65(), None),  # hub degree 64: past one 8-arc group, at the lane path's edge
    "ring257": lambda: (C.ties(synth.ring_chords_graph(257, 6.0, seed=257), 257), None),
    "ring257_directed": lambda: (C.ties(synth.ring_chords_graph(257, 6.0, seed=258, directed=True), 258), None),
    "ring1025": lambda: (C.ties(synth.ring_chords_graph(1025, 7.0, seed=1025), 1025), None),
    "ring1025_directed": lambda: (C.ties(synth.ring_chords_graph(1025, 7.0, seed=1026, directed=True), 1026), None),
    "parallel": lambda: (C.ties(synth.ring_chords_graph(300, 6.0, seed=12, parallel=0.4), 12), None),
    "isolated": _isolated,
}


@pytest.mark.parametrize("net_lds", ["1", "0"])
@pytest.mark.parametrize("name", sorted(SMALL_GRAPHS))
def test_upload_small_graphs(oracle, ctx, monkeypatch, name, net_lds):
    """The upload with its LDS counters and (SG_NET_LDS=0) with global atomics; edge counts off
    the block sizes.  Too few rows for a plan: the identity list's own fill, or the plan-less
    k_plan_rel, writes it."""
    g, used = SMALL_GRAPHS[name]()
    if name.startswith("ring"):
        assert len(g["src"]) % 256 and len(g["src"]) % 1024
    _env(monkeypatch, net_lds)
    assert _both(oracle, ctx, monkeypatch, g, used) is None


@pytest.mark.parametrize("net_lds", ["1", "0"])
def test_upload_graphs_the_reference_rejects(oracle, ctx, monkeypatch, net_lds):
    """No edge at all (one node; five nodes), a directed path (node 0 unreachable from 2), a node
    without a self-loop, a node with two: the error, its pair and its text under both settings."""
    _env(monkeypatch, net_lds)
    cases = [
        (_g(1, [], []), _capi.SG_ERR_NO_EDGE, "No edge connecting node 0 to 0"),
        (_g(5, [], []), _capi.SG_ERR_NO_EDGE, "No edge connecting node 0 to 0"),
        (_g(3, [0, 1, 2, 0, 1], [0, 1, 2, 1, 2], directed=True), _capi.SG_ERR_UNREACHABLE, None),
        (_g(6, [0, 1, 2, 4, 5, 0, 1, 2, 3, 4], [0, 1, 2, 4, 5, 1, 2, 3, 4, 5]), _capi.SG_ERR_NO_EDGE,
         "No edge connecting node 3 to 3"),
        (_g(6, _loops(6) + [4, 0, 1, 2, 3, 4], _loops(6) + [4, 1, 2, 3, 4, 5]), _capi.SG_ERR_MULTI_EDGE,
         "More than one edge connecting node 4 to 4"),
    ]
    for g, code, text in cases:
        msg = _both(oracle, ctx, monkeypatch, g)
        assert msg is not None and (text is None or text in msg), msg
        err = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                    np.arange(g["n"], dtype=np.uint32))[0]
        assert err == code


@pytest.mark.parametrize("n", [NET_LDS_NODES, NET_LDS_NODES + 1])
def test_upload_both_sides_of_the_lds_counters(oracle, ctx, monkeypatch, n):
    """4,096 nodes count in LDS, 4,097 with global atomics; both take the phased plan (16 rows
    per CU): the whole table of each."""
    g = synth.ring_chords_graph(n, 6.0, seed=n)
    _env(monkeypatch)
    assert _both(oracle, ctx, monkeypatch, g) is None


# ---- b. the plan

def _plan_case(oracle, ctx, monkeypatch, name, knobs, used=None, rows=None, flagged="0"):
    """The table with the switch on and off (timers off: the overlapped bound rows, and the launch
    order as it was) and in counting mode (the serial path), whose phase sizes are returned."""
    g, lat, loss = _graph(oracle, name)
    used = np.arange(g["n"], dtype=np.uint32) if used is None else np.asarray(used, dtype=np.uint32)
    rows = rows or (0, len(used))
    sel = used[rows[0]:rows[1]]
    want = (lat[np.ix_(sel, used)], loss[np.ix_(sel, used)])
    _env(monkeypatch, seeds="2", **knobs)
    monkeypatch.setenv("SG_SSSP_FLAGGED", flagged)
    for fused in ("0", "1"):
        monkeypatch.setenv("SG_BUILD_FUSED", fused)
        _same(_build(g, used, rows, ctx), want)
    ctx.enable_timers(True, count_work=True)
    try:
        _same(_build(g, used, rows, ctx), want)
        per_phase = [ctx.read_timer(f"sssp_phase{p}") for p in range(PHASES_MAX)]
        c = dict(sizes=[int(n) for _, n, _ in per_phase], chained=[int(w) for _, _, w in per_phase],
                 unbounded=int(ctx.read_timer("sssp")[1]), bounded=int(ctx.read_timer("sssp_bounded")[1]), g=g,
                 used=used, rows=rows)
    finally:
        ctx.enable_timers(False)
    return c


@pytest.mark.parametrize("n_phase", [2, 3, 6])
@pytest.mark.parametrize("name", ["SMALL", "STAR", "BIG", "HUBS"])
def test_plan_whole_table(oracle, ctx, monkeypatch, name, n_phase):
    c = _plan_case(oracle, ctx, monkeypatch, name, {"SG_SSSP_PHASES": n_phase})
    _check_plan(c, n_phase)


@pytest.mark.parametrize("n_phase", [2, 3, 6])
@pytest.mark.parametrize("case", ["block", "subset", "subset_block"])
def test_plan_blocks_and_subsets(oracle, ctx, monkeypatch, case, n_phase):
    """Rows [600, 1900) of BIG (rel filled for the block's rows only), a shuffled used list of
    1,801 nodes, rows [300, 1500) of it."""
    used, rows = {"block": (None, (600, 1900)), "subset": (C.SUBSET, None), "subset_block": (C.SUBSET, (300, 1500))}[case]
    c = _plan_case(oracle, ctx, monkeypatch, "BIG", {"SG_SSSP_PHASES": n_phase}, used=used, rows=rows)
    _check_plan(c, n_phase)


def test_plan_directed(oracle, ctx, monkeypatch):
    """The in-arc CSC is built on the plan's path (ensure_csc), ahead of the overlapped launch."""
    c = _plan_case(oracle, ctx, monkeypatch, "DIRECTED", {"SG_SSSP_PHASES": 3})
    _check_plan(c, 3)


def test_plan_landmarks_stay_serial(oracle, ctx, monkeypatch):
    c = _plan_case(oracle, ctx, monkeypatch, "BIG", {"SG_SSSP_PHASES": 3, "SG_SSSP_LANDMARKS": 8})
    want = _check_plan(c, 3, 8)
    assert want[0] == 8


def test_plan_flagged_launch_stays_serial(oracle, ctx, monkeypatch):
    c = _plan_case(oracle, ctx, monkeypatch, "BIG", {"SG_SSSP_PHASES": 3}, flagged="1")
    _check_plan(c, 3, phased=False)


# ---- c. the used list: the identity is written on the device, any other list is copied

@pytest.mark.parametrize("which", ["identity", "permutation", "subset"])
@pytest.mark.parametrize("kernel", ["lds", "lds_bounded", "lds_flagged", "bucket", "slab"])
def test_used_lists(oracle, ctx, monkeypatch, kernel, which):
    """Every search family reads the list: the phased and the flagged plan (whose first kernel
    writes the identity), the unplanned LDS launch, the bucketed and the slab search (a fill of
    its own ahead of them).  Whole tables and a row block."""
    g, lat, loss = _graph(oracle, "SMALL")
    n = g["n"]
    used = {"identity": np.arange(n), "permutation": np.random.default_rng(5).permutation(n),
            "subset": np.random.default_rng(6).permutation(n)[:601]}[which].astype(np.uint32)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("SG_NET_LDS", raising=False)
    set_apsp_kernel(monkeypatch, kernel)
    for rows in ((0, len(used)), (128, 400)):
        sel = used[rows[0]:rows[1]]
        want = (lat[np.ix_(sel, used)], loss[np.ix_(sel, used)])
        for fused in ("1", "0"):
            monkeypatch.setenv("SG_BUILD_FUSED", fused)
            _same(_build(g, used, rows, ctx), want)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_used_identity_direct_paths_and_empty_block(oracle, ctx, monkeypatch, fused):
    """The identity list where no search runs: direct paths, and a build of no rows, which still
    checks every used node's self-loop."""
    _env(monkeypatch)
    monkeypatch.setenv("SG_BUILD_FUSED", fused)
    n = 6
    src = [a for a in range(n) for b in range(a, n)]
    dst = [b for a in range(n) for b in range(a, n)]
    g = _g(n, src, dst, seed=66)
    used = np.arange(n, dtype=np.uint32)
    net = _net(g, ctx)
    t = net.get_direct_paths(used)
    rc, dlat, dloss, _ = oracle.direct_paths(n, g["src"], g["dst"], g["lat"], g["loss"], False, used)
    assert rc == 0
    _same((t.latency_ns, t.packet_loss), (dlat, dloss))
    net.build_rows_device(used, 3, 3, 0, 0, True)
    net.close()
    keep = ~((g["src"] == 2) & (g["dst"] == 2))
    bad = _net(dict(g, **{k: g[k][keep] for k in ("src", "dst", "lat", "loss")}), ctx)
    with pytest.raises(ShadowGpuError, match="No edge connecting node 2 to 2"):
        bad.build_rows_device(used, 3, 3, 0, 0, True)
    bad.close()


# ---- d. the overlapped bound rows, build after build on one context

def _net(g, ctx):
    return NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)


def _table(net, n):
    import torch

    dl = torch.zeros(n * n, dtype=torch.int64, device="cuda")
    df = torch.zeros(n * n, dtype=torch.float32, device="cuda")
    net.build_rows_device(np.arange(n, dtype=np.uint32), 0, n, dl.data_ptr(), df.data_ptr(), True)
    return dl.cpu().numpy().view(np.uint64).reshape(n, n), df.cpu().numpy().reshape(n, n)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_builds_back_to_back(oracle, ctx, monkeypatch, fused):
    """Two graphs built back to back (the second plan reuses the first's workspace), a third after
    the first is destroyed (its device block is reused behind the first's last work)."""
    _env(monkeypatch, seeds="2")
    monkeypatch.setenv("SG_BUILD_FUSED", fused)
    gs = [_graph(oracle, name) for name in ("SMALL", "HUBS", "STAR")]
    a, b = _net(gs[0][0], ctx), _net(gs[1][0], ctx)
    ta, tb = _table(a, gs[0][0]["n"]), _table(b, gs[1][0]["n"])
    a.close()
    c = _net(gs[2][0], ctx)
    tc = _table(c, gs[2][0]["n"])
    tb2 = _table(b, gs[1][0]["n"])
    b.close()
    c.close()
    for got, (_, lat, loss) in zip((ta, tb, tc, tb2), (gs[0], gs[1], gs[2], gs[1])):
        _same(got, (lat, loss))


def test_timers_take_the_serial_path(oracle, ctx, monkeypatch):
    """The same graph with timers off (overlapped) and in counting mode (plan_bounds timed on the
    build's stream): equal tables, and the timer saw its launch."""
    _env(monkeypatch, seeds="2")
    monkeypatch.setenv("SG_BUILD_FUSED", "1")
    g, lat, loss = _graph(oracle, "SMALL")
    net = _net(g, ctx)
    plain = _table(net, g["n"])
    ctx.enable_timers(True, count_work=True)
    try:
        counted = _table(net, g["n"])
        assert int(ctx.read_timer("plan_bounds")[1]) == 1
    finally:
        ctx.enable_timers(False)
    again = _table(net, g["n"])
    net.close()
    for got in (plain, counted, again):
        _same(got, (lat, loss))


@pytest.mark.parametrize("fused", ["1", "0"])
def test_failed_build_between_two_good_ones(oracle, ctx, monkeypatch, fused):
    """A build that fails its self-loop check after its launches (the bound rows among them) have
    run; the next build on the context is right."""
    _env(monkeypatch, seeds="2")
    monkeypatch.setenv("SG_BUILD_FUSED", fused)
    g, lat, loss = _graph(oracle, "SMALL")
    keep = ~((g["src"] == 7) & (g["dst"] == 7))  # node 7 loses its self-loop
    bad = dict(g, **{k: g[k][keep] for k in ("src", "dst", "lat", "loss")})
    for _ in range(2):
        _same(_build(g, np.arange(g["n"], dtype=np.uint32), (0, g["n"]), ctx), (lat, loss))
        with pytest.raises(ShadowGpuError, match="No edge connecting node 7 to 7") as e:
            _build(bad, np.arange(g["n"], dtype=np.uint32), (0, g["n"]), ctx)
        assert e.value.code == _capi.SG_ERR_NO_EDGE and e.value.pair == (7, 7)
    _same(_build(g, np.arange(g["n"], dtype=np.uint32), (0, g["n"]), ctx), (lat, loss))


def test_flagged_rows_without_a_final_kernel(oracle, ctx, monkeypatch):
    """FAR with every node used: every row holds saturated keys, so every search flags its row.
    With the switch on no kernel counts the flags at the build's end: the searches tell the host
    themselves, and the wide kernel finishes the table as before."""
    g, lat, loss = _graph(oracle, "FAR")
    assert (lat >= 0xFFFFFFFF).any()
    c = _plan_case(oracle, ctx, monkeypatch, "FAR", {"SG_SSSP_PHASES": 3})
    _check_plan(c, 3)
    _env(monkeypatch, seeds="2")
    monkeypatch.setenv("SG_BUILD_FUSED", "1")
    ctx.enable_timers(True, count_work=True)
    try:
        _same(_build(g, np.arange(g["n"], dtype=np.uint32), (0, g["n"]), ctx), (lat, loss))
        assert int(ctx.read_timer("relax_wide")[1]) > 0
    finally:
        ctx.enable_timers(False)


@pytest.mark.parametrize("knobs", [{"SG_SSSP_SPIN_MAX": 24}, {"SG_SSSP_CHAIN": 0}], ids=["spin24", "chain0"])
def test_overlap_with_rows_that_give_up_and_without_chains(oracle, ctx, monkeypatch, knobs):
    """SG_SSSP_SPIN_MAX=24: rows give up and the wide kernel finishes the table behind the
    overlapped launch.  SG_SSSP_CHAIN=0: no descriptor, the list order."""
    g, lat, loss = _graph(oracle, "SMALL")
    _env(monkeypatch, seeds="2", **knobs)
    for fused in ("1", "0", "1"):
        monkeypatch.setenv("SG_BUILD_FUSED", fused)
        _same(_build(g, np.arange(g["n"], dtype=np.uint32), (0, g["n"]), ctx), (lat, loss))
