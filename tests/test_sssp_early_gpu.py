"""Early rows of the LDS search (sg_sssp.hip "Late seeds", SG_SSSP_EARLY): a chained row with bound
rows starts its search behind the LDS pass, and the other waves load and merge the bound rows
under it, each before it enters the claim loop.

Every case builds the table into zero-poisoned device buffers with SG_SSSP_EARLY 1 and 0 and
compares every cell of both with the CPU oracle (latency by value, loss by bit), so the two builds
are also equal to each other.  A third build with the counting kernels reads
read_timer("sssp_early") = (0, rows that started under their loads, merges onto dirty keys):
wherever a bounded launch chained rows the path must have run, and with the knob at 0, a workgroup
per row or the chain off it must not.  SG_SSSP_SEEDS=2 forces the phased plan at every size here.

The shapes are the smallest at which each thing can go wrong; the counts a case saw are printed.
"""
import functools

import numpy as np
import pytest

from conftest import set_apsp_kernel
from shadow_amd import NetworkGraph, synth

pytestmark = pytest.mark.gpu

PHASES_MAX = 6
KNOBS = ("SG_SSSP_BOUNDS", "SG_SSSP_EXACT", "SG_APSP_DELTA", "SG_SSSP_SPIN_MAX", "SG_SSSP_PERSIST", "SG_SSSP_CHAIN",
         "SG_SSSP_EARLY", "SG_SSSP_PHASES", "SG_SSSP_HOPS")


def _ties(g, seed, zero=0.6):
    """Equal-latency paths everywhere, a share `zero` of zero-loss arcs."""
    rng = np.random.default_rng(seed)
    g["lat"] = (rng.integers(1, 5, len(g["lat"])) * 1000).astype(np.uint64)
    loss = rng.uniform(0.01, 0.3, len(g["lat"])).astype(np.float32)
    loss[rng.random(len(loss)) < zero] = 0
    g["loss"] = loss
    return g


BLOCK = 1536  # the rows built of the 10k-node graphs


def _block_graph(n, seed):
    """Degree 4: self-loops, the ring, and a chord per node.  The first BLOCK nodes' chords end anywhere
    among those nodes, so a block of the first BLOCK rows has neighbours inside the block and far away
    in list order, as a whole table has, and its bounded launch chains rows without the oracle
    computing 10,000 of them (rows next to each other in the list are claimed at the same moment and
    never chain); the other nodes' chords end 2 to 48 places on."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    chord = np.where(i < BLOCK, rng.integers(0, BLOCK, n), (i + rng.integers(2, 49, n)) % n)
    keep = chord != i
    src = np.concatenate([i, i, i[keep]])
    dst = np.concatenate([i, (i + 1) % n, chord[keep]])
    g = dict(n=n, src=src.astype(np.uint32), dst=dst.astype(np.uint32), directed=False, lat=np.zeros(len(src)))
    return _ties(g, seed)


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name == "ties48":
        return _ties(synth.ring_chords_graph(48, 6.0, seed=48), 48)
    if name == "ties200":
        return _ties(synth.ring_chords_graph(200, 6.0, seed=200), 200)
    if name == "ties600":
        return _ties(synth.ring_chords_graph(600, 6.0, seed=600), 600)
    if name == "chords1500":
        return _ties(synth.ring_chords_graph(1500, 7.0, seed=15), 15)
    if name in ("deg4_10400", "deg4_10900"):  # (10,900: past one early round's 10,560 columns)
        return _block_graph(int(name[5:]), seed=int(name[5:]) // 100)
    if name == "far620":  # every arc of 27 nodes is 5 s long: rows with keys past 2^32 - 1 ns next to ordinary ones
        g = _ties(synth.ring_chords_graph(620, 6.0, seed=22), 22)
        far_nodes = np.arange(0, 620, 23)
        far = (np.isin(g["src"], far_nodes) | np.isin(g["dst"], far_nodes)) & (g["src"] != g["dst"])
        g["lat"][far] = np.uint64(5_000_000_000)
        return g
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _used(name, kind):
    n = _graph(name)["n"]
    if kind == "all":
        return np.arange(n, dtype=np.uint32)
    perm = np.random.default_rng(n).permutation(n).astype(np.uint32)
    return perm if kind == "shuffled" else perm[:2 * n // 3 // 4 * 4]  # "two_thirds"


_WANT = {}


def _want(oracle, name, kind, rows):
    """The oracle's rows, computed once per (graph, used list, rows) and never written to."""
    key = (name, kind, rows)
    if key not in _WANT:
        g = _graph(name)
        rc, lat, loss, _ = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                                 _used(name, kind), rows=rows, threads=8)
        assert rc == 0
        lat.setflags(write=False)
        loss.setflags(write=False)
        _WANT[key] = (lat, loss)
    return _WANT[key]


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


def _case(oracle, ctx, monkeypatch, name, kind="all", rows=None, **knobs):
    """Both builds against the oracle, then the counted one.  Returns (rows early, merges onto dirty
    keys, rows chained in the bounded launches)."""
    g, used = _graph(name), _used(name, kind)
    rows = rows or (0, len(used))
    want = _want(oracle, name, kind, rows)
    set_apsp_kernel(monkeypatch, "lds")
    monkeypatch.setenv("SG_SSSP_SEEDS", "2")
    monkeypatch.setenv("SG_SSSP_FLAGGED", "0")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    for early in ("1", "0"):
        monkeypatch.setenv("SG_SSSP_EARLY", early)
        _same(_build(g, used, rows, ctx), want)
        ctx.enable_timers(True, count_work=True)
        try:
            _same(_build(g, used, rows, ctx), want)
            _, n_early, n_dirty = ctx.read_timer("sssp_early")
            chained = sum(int(ctx.read_timer(f"sssp_phase{p}")[2]) for p in range(1, PHASES_MAX))
        finally:
            ctx.enable_timers(False)
        print(f"{name} {kind} {knobs} early={early}: {int(n_early)} early rows, {int(n_dirty)} merges onto dirty "
              f"keys, {chained} rows chained in bounded launches")
        if early == "0":
            assert n_early == 0 and n_dirty == 0
        else:
            out = (int(n_early), int(n_dirty), chained)
    return out


def _ran_where_chained(c):
    n_early, _, chained = c
    assert n_early <= chained
    if chained:
        assert n_early > 0


@pytest.mark.parametrize("name", ["ties48", "ties200", "ties600"])
def test_small_rows_end_before_their_merges(oracle, ctx, monkeypatch, name):
    """48, 200 and 600 nodes, ties and 60 % zero-loss arcs: a search of a few pops can end before a wave
    has merged, so the closing barrier must hold the row; with fewer columns than merging threads
    some waves have nothing to merge.  (A device with more CUs than the graph has rows claims every
    row at once and chains none: on an MI355X the first two check the tables and that nothing is
    counted; 600 nodes, the smallest of these that chains there, runs the path.)"""
    c = _case(oracle, ctx, monkeypatch, name)
    _ran_where_chained(c)
    if name == "ties600":
        assert c[0] > 0


@pytest.mark.parametrize("exact", ["0", "1"])
@pytest.mark.parametrize("bounds", ["1", "2", "4"])
def test_bound_row_pairs_and_exact_seeds(oracle, ctx, monkeypatch, bounds, exact):
    """1,500 nodes: one bound row, a pair, and two pairs (a second load round under the search); with
    and without exact seeds."""
    _ran_where_chained(_case(oracle, ctx, monkeypatch, "chords1500", SG_SSSP_BOUNDS=bounds, SG_SSSP_EXACT=exact))


@pytest.mark.parametrize("name", ["deg4_10400", "deg4_10900"])
def test_columns_past_one_round_and_a_full_lds(oracle, ctx, monkeypatch, name):
    """10,400 nodes (past the set-up's 10,240 columns a round) and 10,900 (past the early merge's
    10,560), degree 4: a second round of columns, and the LDS nearly full.  A block of BLOCK rows."""
    c = _case(oracle, ctx, monkeypatch, name, rows=(0, BLOCK))
    _ran_where_chained(c)
    assert c[0] > 0


@pytest.mark.parametrize("kind", ["shuffled", "two_thirds"])
def test_used_lists(oracle, ctx, monkeypatch, kind):
    """A shuffled used list (not the identity: the column to node map is loaded) and one of two thirds
    of the nodes (the plan's exact seeds off, the chain's on)."""
    _ran_where_chained(_case(oracle, ctx, monkeypatch, "chords1500", kind))


def test_bucket_advances_after_late_merges(oracle, ctx, monkeypatch):
    """SG_APSP_DELTA at a tenth of the largest path: a merge can leave a dirty key below the split
    that no wave queued; the next bucket advance finds it."""
    lat, _ = _want(oracle, "chords1500", "all", (0, 1500))
    _ran_where_chained(_case(oracle, ctx, monkeypatch, "chords1500", SG_APSP_DELTA=max(1, int(lat.max()) // 10)))


def test_saturated_keys_next_to_ordinary_rows(oracle, ctx, monkeypatch):
    """Paths past 2^32 - 1 ns: saturated keys in the rows, rows flagged for the wide kernel, and the
    row just finished demoting the next chain to bounds."""
    lat, _ = _want(oracle, "far620", "all", (0, 620))
    assert lat.max() >= (1 << 32) and np.median(lat) < (1 << 32)
    _ran_where_chained(_case(oracle, ctx, monkeypatch, "far620"))


@pytest.mark.parametrize("spin", ["1", "40"])
def test_give_ups_while_waves_merge(oracle, ctx, monkeypatch, spin):
    """SG_SSSP_SPIN_MAX 1 and 40 (test_lds_give_up_takes_wide_kernel's): waves give up while others
    still merge; the workgroup leaves, the wide kernel redoes the row, the table matches."""
    _case(oracle, ctx, monkeypatch, "chords1500", SG_SSSP_SPIN_MAX=spin)


@pytest.mark.parametrize("knob", ["SG_SSSP_PERSIST", "SG_SSSP_CHAIN"])
def test_no_early_rows_without_chains(oracle, ctx, monkeypatch, knob):
    """A workgroup per row, or the chain off: no row takes the new path."""
    n_early, n_dirty, _ = _case(oracle, ctx, monkeypatch, "chords1500", **{knob: "0"})
    assert n_early == 0 and n_dirty == 0
