"""The LDS search's per-row set-up (sg_sssp.hip "Setup"): every global load issued ahead of the LDS
pass, ten columns per thread in flight and a loop past 10,240 columns; the bound rows listed by
every wave (phased launches) or polled by wave 0 (the flagged launch); no column-id loads with the
identity used list; the ring and own[] reset once per workgroup.

Every case builds into poisoned device buffers and compares every cell with the CPU oracle.  The
large graphs run as small row blocks; an oracle result is computed once per graph and row block and
shared by the configurations that build it.
"""
import numpy as np
import pytest

from conftest import set_apsp_kernel
from shadow_amd import NetworkGraph, synth

pytestmark = pytest.mark.gpu

# the launch shapes: one launch per phase, the one flagged launch, no plan at all
MODES = {
    "phased": {"SG_SSSP_SEEDS": "2", "SG_SSSP_FLAGGED": "0"},
    "flagged": {"SG_SSSP_SEEDS": "1", "SG_SSSP_FLAGGED": "1"},
    "plain": {"SG_SSSP_SEEDS": "0", "SG_SSSP_FLAGGED": "0"},
}

_GRAPHS = {}
_WANT = {}


def _env(monkeypatch, mode, chain="1", **extra):
    set_apsp_kernel(monkeypatch, "lds")
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SG_SSSP_CHAIN", chain)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _ring(n, degree=8.0, seed=1, **kw):
    key = (n, degree, seed, tuple(sorted(kw.items())))
    if key not in _GRAPHS:
        _GRAPHS[key] = synth.ring_chords_graph(n, degree, seed=seed, **kw)
    return _GRAPHS[key]


def _ties(n, degree, seed, zero=0.6, **kw):
    """test_exact_seeds_with_ties' family: equal-latency paths, a share `zero` of zero-loss arcs."""
    key = ("ties", n, degree, seed, zero, tuple(sorted(kw.items())))
    if key not in _GRAPHS:
        g = dict(synth.ring_chords_graph(n, degree, seed=seed, **kw))
        rng = np.random.default_rng(seed)
        g["lat"] = (rng.integers(1, 5, len(g["lat"])) * 1000).astype(np.uint64)
        loss = rng.uniform(0.01, 0.3, len(g["lat"])).astype(np.float32)
        loss[rng.random(len(loss)) < zero] = 0
        g["loss"] = loss
        _GRAPHS[key] = g
    return _GRAPHS[key]


def _want(oracle, name, g, used, rows):
    """The oracle's rows, computed once per (name, rows) and never written to."""
    key = (name, rows)
    if key not in _WANT:
        rc, olat, oloss, _ = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                                   used, rows=rows, threads=8)
        assert rc == 0
        olat.setflags(write=False)
        oloss.setflags(write=False)
        _WANT[key] = (olat, oloss)
    return _WANT[key]


def _build(g, used, rows, ctx):
    import torch

    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    r0, r1 = rows
    nu = len(used)
    dl = torch.full(((r1 - r0) * nu,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    df = torch.full(((r1 - r0) * nu,), float("nan"), dtype=torch.float32, device="cuda")
    net.build_rows_device(used, r0, r1, dl.data_ptr(), df.data_ptr(), True)
    return dl.cpu().numpy().view(np.uint64).reshape(r1 - r0, nu), df.cpu().numpy().reshape(r1 - r0, nu)


def _check(g, used, rows, ctx, want):
    got = _build(g, used, rows, ctx)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049, 6143, 6145])
def test_column_group_edges(oracle, ctx, monkeypatch, n, chain):
    """One, two, three and seven columns per thread with a last column group of 1,023, 1,024 or one
    thread; phases forced, so the bounded launch merges two bound rows per row."""
    g = _ring(n, 8.0, seed=n)
    used = np.arange(n, dtype=np.uint32)
    rows = (0, n) if n <= 1025 else (0, 520)
    want = _want(oracle, f"edges{n}", g, used, rows)
    _env(monkeypatch, "phased", chain)
    _check(g, used, rows, ctx, want)


@pytest.mark.parametrize("mode", ["phased", "flagged"])
@pytest.mark.parametrize("rows", [(0, 300), (5000, 5300)])
def test_loop_past_10240_columns(oracle, ctx, monkeypatch, rows, mode):
    """10,300 columns: the load rounds' loop runs twice, the second round for 60 columns."""
    g = _ring(10300, 8.0, seed=7)
    used = np.arange(10300, dtype=np.uint32)
    want = _want(oracle, "past10240", g, used, rows)
    _env(monkeypatch, mode)
    _check(g, used, rows, ctx, want)


@pytest.mark.parametrize("mode,chain", [("phased", "1"), ("phased", "0"), ("flagged", "1"), ("plain", "1")])
@pytest.mark.parametrize("n_used", [700, 701, 1000])
def test_used_lists(oracle, ctx, monkeypatch, n_used, mode, chain):
    """A shuffled subset of 700 (16-B output stores) and 701 (scalar ones) of 1,000 nodes: the column
    ids are loaded.  The identity list of the same graph: they are not."""
    g = _ties(1000, 7.0, seed=5)
    if n_used == 1000:
        used = np.arange(1000, dtype=np.uint32)
    else:
        used = np.random.default_rng(n_used).permutation(1000)[:n_used].astype(np.uint32)
    want = _want(oracle, f"used{n_used}", g, used, (0, n_used))
    _env(monkeypatch, mode, chain)
    _check(g, used, (0, n_used), ctx, want)


@pytest.mark.parametrize("mode", ["phased", "flagged"])
@pytest.mark.parametrize("kb", ["1", "2", "3", "8"])
def test_bound_row_counts(oracle, ctx, monkeypatch, kb, mode):
    """One bound row (half a pair), two, three (a second round with half a pair) and eight."""
    g = _ties(640, 8.0, seed=21)
    used = np.arange(640, dtype=np.uint32)
    want = _want(oracle, "bounds640", g, used, (0, 640))
    _env(monkeypatch, mode, SG_SSSP_BOUNDS=kb)
    _check(g, used, (0, 640), ctx, want)


@pytest.mark.parametrize("mode", ["phased", "flagged"])
def test_bound_rows_with_saturated_keys(oracle, ctx, monkeypatch, mode):
    """Every arc of 27 nodes is 5 s long (test_chain_behind_saturated_rows): each row holds
    saturated keys, so a bound row gives bounds only, and the wide kernel finishes the table."""
    n = 620
    g = dict(_ties(n, 6.0, seed=22))
    far_nodes = np.arange(0, n, 23)
    far = (np.isin(g["src"], far_nodes) | np.isin(g["dst"], far_nodes)) & (g["src"] != g["dst"])
    g["lat"] = g["lat"].copy()
    g["lat"][far] = np.uint64(5_000_000_000)
    used = np.arange(n, dtype=np.uint32)
    want = _want(oracle, "far620", g, used, (0, n))
    _env(monkeypatch, mode)
    _check(g, used, (0, n), ctx, want)


@pytest.mark.parametrize("mode", ["phased", "flagged"])
@pytest.mark.parametrize("spin", ["1", "40"])
def test_bound_rows_that_gave_up(oracle, ctx, monkeypatch, spin, mode):
    """SG_SSSP_SPIN_MAX 1 and 40: searches give up, their rows are never written and give no
    bounds; the table is still exact through the wide kernel."""
    g = _ring(700, 6.0, seed=33)
    used = np.arange(700, dtype=np.uint32)
    want = _want(oracle, "giveup700", g, used, (0, 700))
    _env(monkeypatch, mode, SG_SSSP_SPIN_MAX=spin)
    _check(g, used, (0, 700), ctx, want)


@pytest.mark.parametrize("mode,persist", [("phased", "1"), ("plain", "1"), ("phased", "0"), ("plain", "0")])
def test_directed_graph(oracle, ctx, monkeypatch, mode, persist):
    """No chain: thread 0 claims the next row.  SG_SSSP_PERSIST=0: one row per workgroup, so every
    row is a workgroup's first and the one reset of the ring is the only one."""
    g = _ties(700, 7.0, seed=9, directed=True)
    used = np.arange(700, dtype=np.uint32)
    want = _want(oracle, "directed700", g, used, (0, 700))
    _env(monkeypatch, mode, SG_SSSP_PERSIST=persist)
    _check(g, used, (0, 700), ctx, want)


@pytest.mark.parametrize("mode,chain", [("phased", "1"), ("phased", "0"), ("plain", "1"), ("flagged", "1")])
def test_delta_buckets(oracle, ctx, monkeypatch, mode, chain):
    """50-ms buckets on 900 nodes: the quiescence scan queues the dirty nodes again through the
    ring that no row resets."""
    g = _ring(900, 7.0, seed=31)
    used = np.arange(900, dtype=np.uint32)
    want = _want(oracle, "delta900", g, used, (0, 900))
    _env(monkeypatch, mode, chain, SG_APSP_DELTA="50000000")
    _check(g, used, (0, 900), ctx, want)


@pytest.mark.parametrize("delta", [None, "50000000"])
def test_ring_is_empty_at_every_rows_end(oracle, ctx, monkeypatch, delta):
    """The counting build looks at the whole ring after each search: every slot written was popped
    (read_timer("sssp_ring_left") = (0, rows looked at, slots found non-empty))."""
    g = _ring(900, 7.0, seed=31)
    used = np.arange(900, dtype=np.uint32)
    want = _want(oracle, "delta900", g, used, (0, 900))
    extra = {"SG_APSP_DELTA": delta} if delta else {}
    _env(monkeypatch, "phased", **extra)
    ctx.enable_timers(True, count_work=True)
    try:
        _check(g, used, (0, 900), ctx, want)
        _, n_rows, left = ctx.read_timer("sssp_ring_left")
    finally:
        ctx.enable_timers(False)
    print(f"sssp_ring_left: {left:.0f} slots in {n_rows} rows")
    assert n_rows == 900
    assert left == 0
