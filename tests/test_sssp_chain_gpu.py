"""Chained rows of the LDS search (sg_sssp.hip "Chained rows", SG_SSSP_CHAIN): a persistent
workgroup takes as its next row one that has an arc to the row it just finished, and rewrites the
keys still in its LDS into that row's start (bounds, or exact seeds over a zero-loss arc).

Every case compares every cell of a table built into zero-poisoned device buffers with the CPU
oracle, with the chain on and off, without a plan (SG_SSSP_SEEDS=0) and with the phases forced
(SG_SSSP_SEEDS=2).  The graphs have 600-1,200 nodes: 2-5 rows per CU, so chains form.

test_chains_at_the_seam runs tests/seam_cases.py's 603-node graphs, whose rows end exactly at the
largest latency a 32-bit key holds, also without exact seeds and with a workgroup per row
(measured on an MI355X: 0.07 and 0.03 s per case, twelve builds each; the counts vary a little
from run to run: under_ms600 chained about 270 rows, 200 of them with exact seeds, without a
plan and about 77 / 54 with the phases forced; under_unit600 about 232 / 137 and 22 / 9).
"""
import numpy as np
import pytest

from conftest import set_apsp_kernel
from shadow_amd import NetworkGraph, synth

pytestmark = pytest.mark.gpu

CONFIGS = [(chain, seeds) for chain in ("1", "0") for seeds in ("0", "2")]


def _env(monkeypatch, chain, seeds):
    set_apsp_kernel(monkeypatch, "lds")
    monkeypatch.setenv("SG_SSSP_FLAGGED", "0")
    monkeypatch.setenv("SG_SSSP_SEEDS", seeds)
    monkeypatch.setenv("SG_SSSP_CHAIN", chain)


def _oracle(oracle, g, used, rows):
    rc, olat, oloss, _ = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], used,
                                               rows=rows, threads=8)
    assert rc == 0
    return olat, oloss


def _build(g, used, rows, ctx):
    import torch

    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    r0, r1 = rows
    nu = len(used)
    dl = torch.zeros((r1 - r0) * nu, dtype=torch.int64, device="cuda")
    df = torch.zeros((r1 - r0) * nu, dtype=torch.float32, device="cuda")
    net.build_rows_device(used, r0, r1, dl.data_ptr(), df.data_ptr(), True)
    return dl.cpu().numpy().view(np.uint64).reshape(r1 - r0, nu), df.cpu().numpy().reshape(r1 - r0, nu)


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _counted(g, used, rows, ctx, want):
    """One build with the counting kernels: (chained rows, those with exact seeds)."""
    ctx.enable_timers(True, count_work=True)
    try:
        _same(_build(g, used, rows, ctx), want)
        _, n_exact, n_chained = ctx.read_timer("sssp_chained")
    finally:
        ctx.enable_timers(False)
    print(f"sssp_chained: {n_chained:.0f} rows, {n_exact} exact, of {rows[1] - rows[0]}")
    return int(n_chained), int(n_exact)


def _all_configs(oracle, ctx, monkeypatch, g, used, rows=None, counted=False):
    """The table under the four configurations; with counted, the chained-row counts per configuration."""
    used = np.asarray(used, dtype=np.uint32)
    rows = rows or (0, len(used))
    want = _oracle(oracle, g, used, rows)
    counts = {}
    for chain, seeds in CONFIGS:
        _env(monkeypatch, chain, seeds)
        _same(_build(g, used, rows, ctx), want)
        if counted:
            counts[(chain, seeds)] = _counted(g, used, rows, ctx, want)
    return counts


def _ties(g, seed, zero=0.6):
    """test_exact_seeds_with_ties' family: equal-latency paths, a share `zero` of zero-loss arcs."""
    rng = np.random.default_rng(seed)
    g["lat"] = (rng.integers(1, 5, len(g["lat"])) * 1000).astype(np.uint64)
    loss = rng.uniform(0.01, 0.3, len(g["lat"])).astype(np.float32)
    loss[rng.random(len(loss)) < zero] = 0
    g["loss"] = loss
    return g


def test_chains_form(oracle, ctx, monkeypatch):
    g = synth.ring_chords_graph(900, 7.0, seed=31)
    counts = _all_configs(oracle, ctx, monkeypatch, g, np.arange(900), counted=True)
    for (chain, seeds), (n_chained, n_exact) in counts.items():
        if chain == "1":
            assert n_chained > 0, (chain, seeds)
        else:
            assert n_chained == 0 and n_exact == 0, (chain, seeds)


@pytest.mark.parametrize("zero", [0.6, 0.0, 1.0])
def test_ties_and_loss_mixes(oracle, ctx, monkeypatch, zero):
    """Equal-latency paths with 60 % zero-loss arcs; every arc lossy (chains give bounds only);
    every arc zero-loss (every chain seeds exact keys)."""
    g = _ties(synth.ring_chords_graph(640, 8.0, seed=21), 21, zero)
    counts = _all_configs(oracle, ctx, monkeypatch, g, np.arange(640), counted=True)
    for seeds in ("0", "2"):
        n_chained, n_exact = counts[("1", seeds)]
        assert n_chained > 0
        if zero == 0.0:
            assert n_exact == 0
        if zero == 1.0:
            assert n_exact == n_chained


@pytest.mark.parametrize("n_used", [700, 701])
def test_used_subset_exact_chain_seeds(oracle, ctx, monkeypatch, n_used):
    """A shuffled used list of 700 (701: n_used % 4 != 0, the scalar output path) of 1,000 nodes: the
    LDS row seeds every node, used or not, so chains seed exact keys where the plan's bound rows
    (used columns only) cannot."""
    g = _ties(synth.ring_chords_graph(1000, 7.0, seed=5), 5)
    used = np.random.default_rng(n_used).permutation(1000)[:n_used]
    counts = _all_configs(oracle, ctx, monkeypatch, g, used, counted=True)
    for seeds in ("0", "2"):
        assert counts[("1", seeds)][1] > 0


def test_row_block_in_the_middle(oracle, ctx, monkeypatch):
    """Rows [200, 800) of 1,000: neighbours outside the block are never claimed, every row of the
    block is written (the buffer starts poisoned) and equals the oracle's."""
    g = _ties(synth.ring_chords_graph(1000, 7.0, seed=6), 6)
    counts = _all_configs(oracle, ctx, monkeypatch, g, np.arange(1000), rows=(200, 800), counted=True)
    for seeds in ("0", "2"):
        assert 0 < counts[("1", seeds)][0] < 600


@pytest.mark.parametrize("all_used", [True, False])
def test_chain_behind_saturated_rows(oracle, ctx, monkeypatch, all_used):
    """Every arc of 27 nodes is 5 s long (test_exact_seeds_next_to_wide_rows, undirected).  With
    every node used each row holds saturated keys: a row chained behind one takes no exact seeds,
    and the table is exact after the wide kernel.  With only the other nodes used, no output sees
    the saturated keys of the unused ones, and the exact chain seeds must still give the table."""
    n = 620
    g = _ties(synth.ring_chords_graph(n, 6.0, seed=22), 22)
    far_nodes = np.arange(0, n, 23)
    far = (np.isin(g["src"], far_nodes) | np.isin(g["dst"], far_nodes)) & (g["src"] != g["dst"])
    g["lat"][far] = np.uint64(5_000_000_000)
    used = np.arange(n) if all_used else np.setdiff1d(np.arange(n), far_nodes)
    counts = _all_configs(oracle, ctx, monkeypatch, g, used, counted=True)
    for seeds in ("0", "2"):
        n_chained, n_exact = counts[("1", seeds)]
        assert n_chained > 0
        if all_used:
            assert n_exact == 0
        else:
            assert n_exact > 0


@pytest.mark.parametrize("name", ["under_ms600", "under_unit600"])
def test_chains_at_the_seam(oracle, ctx, monkeypatch, name):
    """tests/seam_cases.py's 600-node graphs: 167 and 237 of 603 rows have a maximum of exactly
    2^32 - 2 ns, the largest latency a 32-bit key holds (a chain's `lw < LAT32_SAT - 1` and an exact
    seed's `ub < LAT32_SAT` are one off it), 149 and 117 rows hold cells past 2^32 and go to the
    wide kernel.  Every base arc of under_ms600 is lossless: its chains seed exact keys."""
    import sweep_cases as SC

    c = SC.case(name)
    counts = _all_configs(oracle, ctx, monkeypatch, c["g"], c["nodes"], counted=True)
    for (chain, seeds), (n_chained, n_exact) in counts.items():
        if chain == "0":
            assert n_chained == 0 and n_exact == 0, (chain, seeds)
            continue
        assert n_chained > 0, (chain, seeds)
        if name == "under_ms600":
            assert n_exact > 0, (chain, seeds)
    # The launch without a plan, 603 rows on fewer CUs: SG_SSSP_EXACT=0 chains with bounds only;
    # SG_SSSP_PERSIST=0 launches a workgroup per row, which chains nothing.
    used = np.asarray(c["nodes"], dtype=np.uint32)
    rows = (0, len(used))
    want = _oracle(oracle, c["g"], used, rows)
    for knob, chains in (("SG_SSSP_EXACT", True), ("SG_SSSP_PERSIST", False)):
        with monkeypatch.context() as m:
            _env(m, "1", "0")
            m.setenv(knob, "0")
            _same(_build(c["g"], used, rows, ctx), want)
            n_chained, n_exact = _counted(c["g"], used, rows, ctx, want)
            assert n_exact == 0 and (n_chained > 0) == chains, (knob, n_chained, n_exact)


@pytest.mark.parametrize("spin", ["1", "40"])
def test_give_ups_with_the_chain_on(oracle, ctx, monkeypatch, spin):
    """SG_SSSP_SPIN_MAX 1 and 40: workgroups give up; every row is still produced (by the search
    or by the wide kernel), none claimed and then lost."""
    monkeypatch.setenv("SG_SSSP_SPIN_MAX", spin)
    g = synth.ring_chords_graph(700, 6.0, seed=33)
    _all_configs(oracle, ctx, monkeypatch, g, np.arange(700))


def test_parallel_edges_hub_and_self_loops(oracle, ctx, monkeypatch):
    """Parallel edges with different weights, a hub with more than 64 arcs (the scan's cap), and
    the self-loops every node carries."""
    g = _ties(synth.ring_chords_graph(800, 7.0, seed=44, parallel=0.3), 44)
    rng = np.random.default_rng(44)
    spokes = rng.permutation(np.arange(1, 800))[:150].astype(np.uint32)
    g["src"] = np.concatenate([g["src"], np.zeros(150, dtype=np.uint32)])
    g["dst"] = np.concatenate([g["dst"], spokes])
    g["lat"] = np.concatenate([g["lat"], (rng.integers(1, 5, 150) * 1000).astype(np.uint64)])
    g["loss"] = np.concatenate([g["loss"], np.where(rng.random(150) < 0.5, 0, 0.1).astype(np.float32)])
    counts = _all_configs(oracle, ctx, monkeypatch, g, np.arange(800), counted=True)
    assert counts[("1", "0")][0] > 0 and counts[("1", "2")][0] > 0


def test_directed_graph_never_chains(oracle, ctx, monkeypatch):
    g = _ties(synth.ring_chords_graph(700, 7.0, seed=9, directed=True), 9)
    counts = _all_configs(oracle, ctx, monkeypatch, g, np.arange(700), counted=True)
    assert all(c == (0, 0) for c in counts.values())
