"""The LDS search's relaxation step sized to the pop's arcs (sg_sssp.hip "the step follows the arcs"):
a pop of at most SG_SSSP_STEP_ARCS arcs is relaxed arc-parallel in ceil(arcs / 64) slots per lane
(one, two, or rounds of four), any other pop on the lane path; and the pop's ring slot read and
cleared as LDS.

Every case builds into poisoned device buffers and compares every cell with the CPU oracle, bit for
bit.  An oracle result is computed once per graph and row block and shared by the settings that
build it.  The thresholds: 0 (the lane path for every pop), 64 and 128 (the one- and two-slot
steps alone), 256 (the default: one round of four), 1,000,000 (no pop on the lane path, rounds of
four looping); the claims: 1 entry (every pop one node), 5, 64.

Claims by share of the queue were measured and not kept, so there is no
share knob to cross with.
"""
import numpy as np
import pytest

from conftest import set_apsp_kernel
from shadow_amd import NetworkGraph, synth

pytestmark = pytest.mark.gpu

MODES = {
    "phased": {"SG_SSSP_SEEDS": "2", "SG_SSSP_FLAGGED": "0"},
    "flagged": {"SG_SSSP_SEEDS": "1", "SG_SSSP_FLAGGED": "1"},
    "plain": {"SG_SSSP_SEEDS": "0", "SG_SSSP_FLAGGED": "0"},
}
STEP_ARCS = ["0", "64", "128", "256", "1000000"]
CLAIMS = ["1", "5", "64"]
POP_CLASSES = ("0", "1", "2", "4", "8", "gt8")

_GRAPHS = {}
_WANT = {}


def _ties(g, seed, zero=0.6):
    """test_exact_seeds_with_ties' family: equal-latency paths, a share `zero` of zero-loss arcs."""
    g = dict(g)
    rng = np.random.default_rng(seed)
    g["lat"] = (rng.integers(1, 5, len(g["lat"])) * 1000).astype(np.uint64)
    loss = rng.uniform(0.01, 0.3, len(g["lat"])).astype(np.float32)
    loss[rng.random(len(loss)) < zero] = 0
    g["loss"] = loss
    return g


def _with_edges(g, src, dst, seed):
    """g plus the edges (src, dst), latencies and losses drawn like a chord's."""
    g = dict(g)
    rng = np.random.default_rng(seed)
    m = len(src)
    g["src"] = np.concatenate([g["src"], np.asarray(src, np.uint32)])
    g["dst"] = np.concatenate([g["dst"], np.asarray(dst, np.uint32)])
    g["lat"] = np.concatenate([g["lat"], (rng.integers(1000, 100000, m) * 1000).astype(np.uint64)])
    g["loss"] = np.concatenate([g["loss"], rng.uniform(0.0, 0.02, m).astype(np.float32)])
    return g


def _make(name):
    if name == "ring8":  # 1,025 nodes: more rows than CUs (persistent workgroups), a last column group of one
        return synth.ring_chords_graph(1025, 8.0, seed=12)
    if name == "ring3":  # no node past eight arcs: the lane path has no overflow round
        return synth.ring_chords_graph(1025, 3.0, seed=13)
    if name == "ties":
        return _ties(synth.ring_chords_graph(1000, 7.0, seed=5), 5)
    if name == "ties_directed":
        return _ties(synth.ring_chords_graph(1000, 7.0, seed=9, directed=True), 9)
    if name == "parallel":
        return synth.ring_chords_graph(1025, 8.0, seed=14, parallel=0.2)
    if name == "hub":
        # a ring of 600 plus node 0 joined to 300 others: one queue entry spans more than four
        # 64-slot chunks, so the owner carry crosses the rounds of the arc-parallel step
        g = synth.ring_chords_graph(600, 2.0, seed=15)
        others = np.random.default_rng(15).permutation(np.arange(2, 599))[:300]
        return _with_edges(g, np.zeros(300, np.uint32), others, 15)
    if name == "sink":
        # directed, and node 7 has no out-arc: a pop that holds node 7 alone holds no arc at all
        # (claims of one entry).  Nothing is reachable from node 7, and a used pair out of reach
        # fails the build, so node 7 is the one unused node (699 columns: scalar output stores).
        g = _ties(synth.ring_chords_graph(700, 7.0, seed=16, directed=True), 16)
        keep = g["src"] != 7
        return {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    if name == "two_parts":
        # two parts of 330 nodes.  With no path between them the build fails by contract (a used
        # pair out of reach), so one edge of 5 s joins them: every key across it is past the u32
        # latency, every row saturates and is finished by the wide kernel
        a = synth.ring_chords_graph(330, 6.0, seed=17)
        b = synth.ring_chords_graph(330, 6.0, seed=18)
        g = dict(a)
        g["n"] = 660
        g["src"] = np.concatenate([a["src"], b["src"] + np.uint32(330), [5]]).astype(np.uint32)
        g["dst"] = np.concatenate([a["dst"], b["dst"] + np.uint32(330), [400]]).astype(np.uint32)
        g["lat"] = np.concatenate([a["lat"], b["lat"], [5_000_000_000]]).astype(np.uint64)
        g["loss"] = np.concatenate([a["loss"], b["loss"], [0.01]]).astype(np.float32)
        return g
    raise KeyError(name)


def _used(name):
    n = _graph(name)["n"]
    used = np.arange(n, dtype=np.uint32)
    return used[used != 7] if name == "sink" else used


GRAPHS = ["ring8", "ring3", "ties", "ties_directed", "parallel", "hub", "sink", "two_parts"]


def _graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = _make(name)
    return _GRAPHS[name]


def _want(oracle, name):
    """The oracle's table of the graph, computed once and never written to."""
    if name not in _WANT:
        g = _graph(name)
        used = _used(name)
        rc, olat, oloss, _ = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                                   used, rows=(0, len(used)), threads=8)
        assert rc == 0
        olat.setflags(write=False)
        oloss.setflags(write=False)
        _WANT[name] = (olat, oloss)
    return _WANT[name]


def _env(monkeypatch, mode="phased", chain="1", step="256", **extra):
    set_apsp_kernel(monkeypatch, "lds")
    for k in ("SG_SSSP_CLAIM", "SG_SSSP_PERSIST", "SG_APSP_DELTA", "SG_SSSP_SPIN_MAX", "SG_SSSP_DIAG",
              "SG_SSSP_LANE_DEG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SG_SSSP_CHAIN", chain)
    monkeypatch.setenv("SG_SSSP_STEP_ARCS", step)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _check(name, ctx, want):
    import torch

    g = _graph(name)
    used = _used(name)
    n = len(used)
    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    dl = torch.full((n * n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    df = torch.full((n * n,), float("nan"), dtype=torch.float32, device="cuda")
    net.build_rows_device(used, 0, n, dl.data_ptr(), df.data_ptr(), True)
    lat = dl.cpu().numpy().view(np.uint64).reshape(n, n)
    loss = df.cpu().numpy().reshape(n, n)
    assert np.array_equal(lat, want[0])
    assert np.array_equal(loss.view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("claim", CLAIMS)
@pytest.mark.parametrize("step", STEP_ARCS)
@pytest.mark.parametrize("name", GRAPHS)
def test_step_by_arcs(oracle, ctx, monkeypatch, name, step, claim):
    want = _want(oracle, name)
    _env(monkeypatch, step=step, SG_SSSP_CLAIM=claim)
    _check(name, ctx, want)


@pytest.mark.parametrize("mode,chain", [("phased", "1"), ("phased", "0"), ("flagged", "1"), ("flagged", "0"),
                                        ("plain", "1"), ("plain", "0")])
def test_launch_shapes(oracle, ctx, monkeypatch, mode, chain):
    want = _want(oracle, "ring8")
    _env(monkeypatch, mode, chain)
    _check("ring8", ctx, want)


@pytest.mark.parametrize("mode", ["phased", "plain"])
def test_workgroup_per_row(oracle, ctx, monkeypatch, mode):
    want = _want(oracle, "ring8")
    _env(monkeypatch, mode, SG_SSSP_PERSIST="0")
    _check("ring8", ctx, want)


@pytest.mark.parametrize("claim", ["5", "64"])
def test_delta_buckets(oracle, ctx, monkeypatch, claim):
    """25-ms buckets: the step's appends are filtered by `split`, and the quiescence scan queues
    the dirty nodes again."""
    want = _want(oracle, "ring8")
    _env(monkeypatch, SG_APSP_DELTA="25000000", SG_SSSP_CLAIM=claim)
    _check("ring8", ctx, want)


@pytest.mark.parametrize("spin", ["1", "40"])
def test_give_up_takes_wide_kernel(oracle, ctx, monkeypatch, spin):
    """SG_SSSP_SPIN_MAX 1 and 40 (test_lds_give_up_takes_wide_kernel): searches give up, and the
    table still matches the oracle through the wide kernel."""
    want = _want(oracle, "ring8")
    _env(monkeypatch, SG_SSSP_SPIN_MAX=spin)
    _check("ring8", ctx, want)


def _counted(name, ctx, want):
    ctx.enable_timers(True, count_work=True)
    try:
        _check(name, ctx, want)
        cls = [ctx.read_timer(f"sssp_pop_s{c}")[1:] for c in POP_CLASSES]
        cyc = [ctx.read_timer(f"sssp_pop_s{c}_cyc") for c in POP_CLASSES]
        _, pops, lane_pops = ctx.read_timer("sssp_pops")
        rel = ctx.read_timer("sssp")[2]
    finally:
        ctx.enable_timers(False)
    print("pops, arcs per class:", cls, "pops:", pops, "on the lane path:", lane_pops, "relaxations:", rel)
    assert pops > 0
    assert sum(int(p) for p, _ in cls) == pops
    assert sum(int(a) for _, a in cls) == int(rel)
    for (p, _), (_, pc, c) in zip(cls, cyc):
        assert pc == p
        assert (c > 0) == (p > 0)
    return cls, pops, lane_pops


@pytest.mark.parametrize("mode", ["phased", "plain"])
def test_pop_classes_add_up(oracle, ctx, monkeypatch, mode):
    """One counting build: the classes' pops sum to the pops the waves counted and their arcs to the
    relaxation count.  With claims of one entry and no node past 64 arcs, no pop is past S = 1."""
    want = _want(oracle, "ring8")
    _env(monkeypatch, mode, SG_SSSP_DIAG="1")
    _, pops, lane_pops = _counted("ring8", ctx, want)
    assert 0 < lane_pops < pops  # the default threshold: pops on either side of it
    _env(monkeypatch, mode, SG_SSSP_DIAG="1", SG_SSSP_CLAIM="1")
    cls, pops, lane_pops = _counted("ring8", ctx, want)
    assert all(p == 0 for p, _ in cls[2:])
    assert lane_pops == 0  # a node's arcs are below the default threshold


def test_no_lane_path_past_the_threshold(oracle, ctx, monkeypatch):
    """SG_SSSP_STEP_ARCS=1000000: no pop takes the lane path; 0: every pop does, where no node is
    past SG_SSSP_LANE_DEG arcs (ring8), and every pop but those holding the hub (hub)."""
    for name in ("ring8", "hub"):
        want = _want(oracle, name)
        _env(monkeypatch, step="1000000", SG_SSSP_DIAG="1")
        cls, pops, lane_pops = _counted(name, ctx, want)
        assert lane_pops == 0
        _env(monkeypatch, step="0", SG_SSSP_DIAG="1")
        cls, pops, lane_pops = _counted(name, ctx, want)
        assert (lane_pops == pops) if name == "ring8" else (0 < lane_pops < pops)
    assert cls[4][0] > 0  # the hub's 300 arcs: pops of five slots per lane at least
