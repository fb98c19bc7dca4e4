"""The LDS search's phase plan (sg_plan.hip) past two phases, its landmarks, and the plan and
search knobs no other test sets.

Every configuration is built twice into zero-poisoned device buffers and every cell compared with
the CPU oracle (latency by value, loss by bit): once plain (the production kernel) and once with
the counting timers, which run the counting instantiation and publish, per phase p of the plan,
read_timer("sssp_phase<p>") = (0, rows of the phase, rows chained in its launch).  The phase
sizes are a deterministic function of the graph and must equal the CPU model's (plan_ref.py)
exactly: a plan that is legal but not the specified one fails here, though its table is right.
test_plan_ref_cpu.py pins the properties of these graphs' plans that the assertions rely on.
"""
import numpy as np
import pytest

import plan_cases as C
import plan_ref
from conftest import set_apsp_kernel
from test_sssp_chain_gpu import _build, _same

pytestmark = pytest.mark.gpu

PHASES_MAX = plan_ref.PHASES_MAX
GRAPHS = {"BIG": C.big, "SMALL": C.small, "STAR": C.star, "HUBS": C.hubs, "FAR": C.far, "DIRECTED": C.directed,
          "STAR_Z": lambda: C.star(zero=1.0), "HUBS_Z": lambda: C.hubs(zero=1.0)}
# every knob a case may set: each configuration starts from all of them unset
KNOBS = ("SG_SSSP_PHASES", "SG_SSSP_CHAIN", "SG_SSSP_LANDMARKS", "SG_SSSP_HOPS", "SG_SSSP_EXACT", "SG_SSSP_BOUNDS",
         "SG_SSSP_CLAIM", "SG_SSSP_LANE_DEG", "SG_SSSP_SLEEP", "SG_SSSP_SPIN_MAX", "SG_APSP_DELTA")
_cache = {}


def _graph(oracle, name):
    """The graph and the oracle's whole table, computed once per graph and never changed."""
    if name not in _cache:
        g = GRAPHS[name]()
        rc, lat, loss, _ = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                                 np.arange(g["n"], dtype=np.uint32), threads=8)
        assert rc == 0
        lat.setflags(write=False)
        loss.setflags(write=False)
        _cache[name] = (g, lat, loss)
    return _cache[name]


def _run(oracle, ctx, monkeypatch, name, knobs, used=None, rows=None, seeds="2", flagged="0"):
    """The table under `knobs`, plain and counted; the counted build's counters."""
    g, lat, loss = _graph(oracle, name)
    used = np.arange(g["n"], dtype=np.uint32) if used is None else np.asarray(used, dtype=np.uint32)
    rows = rows or (0, len(used))
    # a cell depends on its source and destination only: the block of a subset is a slice of the whole table
    sel = used[rows[0]:rows[1]]
    want = (lat[np.ix_(sel, used)], loss[np.ix_(sel, used)])
    set_apsp_kernel(monkeypatch, "lds")
    monkeypatch.setenv("SG_SSSP_SEEDS", seeds)
    monkeypatch.setenv("SG_SSSP_FLAGGED", flagged)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    _same(_build(g, used, rows, ctx), want)
    ctx.enable_timers(True, count_work=True)
    try:
        _same(_build(g, used, rows, ctx), want)
        per_phase = [ctx.read_timer(f"sssp_phase{p}") for p in range(PHASES_MAX)]
        _, n_exact, n_chained = ctx.read_timer("sssp_chained")
        c = dict(sizes=[int(n) for _, n, _ in per_phase], chained=[int(w) for _, _, w in per_phase],
                 unbounded=int(ctx.read_timer("sssp")[1]), bounded=int(ctx.read_timer("sssp_bounded")[1]),
                 wide=int(ctx.read_timer("relax_wide")[1]), n_chained=int(n_chained), n_exact=int(n_exact), g=g,
                 used=used, rows=rows)
    finally:
        ctx.enable_timers(False)
    print(name, knobs, "rows", rows, {k: c[k] for k in ("sizes", "chained", "unbounded", "bounded", "wide", "n_exact")})
    if seeds != "0":  # (a build without a plan publishes no phase counters)
        assert sum(c["chained"]) == c["n_chained"]
    return c


def _check_plan(c, n_phase, n_land=0, phased=True):
    """The counters against the model: the plan's sizes exactly, one launch per phase."""
    n = plan_ref.n_launches(n_phase, n_land)
    want = plan_ref.sizes(plan_ref.phases(c["g"], c["used"], c["rows"], n_phase, n_land), n)
    assert c["sizes"] == want + [0] * (PHASES_MAX - n)
    assert sum(c["sizes"]) == c["rows"][1] - c["rows"][0]
    assert c["chained"][n:] == [0] * (PHASES_MAX - n)
    if phased:
        assert (c["unbounded"], c["bounded"]) == (1, n - 1)
    else:  # the flagged launch: one launch, no chains
        assert (c["unbounded"], c["bounded"]) == (1, 0)
        assert c["chained"] == [0] * PHASES_MAX
    return want


def _check_chain(c, chain, must_chain):
    """Chain off: no launch chains.  Chain on: the phases p >= 1 listed in must_chain do."""
    if chain == "0":
        assert c["chained"] == [0] * PHASES_MAX and c["n_exact"] == 0
    else:
        for p in must_chain:
            assert c["chained"][p] > 0, (p, c["chained"])


# ---- a. phase counts

@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("n_phase", [3, 4, 6])
def test_phases_whole_table(oracle, ctx, monkeypatch, n_phase, chain):
    """3, 4 and 6 phased launches.  At 3 and 4 every phase has more rows than the grid, so with the
    chain on rows chain inside bounded launches: chain seeds merged with bounds from several
    earlier phases.  At 6 the last phase is empty and the fifth has 32 rows."""
    c = _run(oracle, ctx, monkeypatch, "BIG", {"SG_SSSP_PHASES": n_phase, "SG_SSSP_CHAIN": chain})
    want = _check_plan(c, n_phase)
    if n_phase == 6:
        assert 0 in want
    if chain == "0":
        _check_chain(c, chain, [])
    elif n_phase in (3, 4):
        assert any(c["chained"][p] > 0 for p in range(1, n_phase)), c["chained"]
        assert all(c["chained"][p] <= want[p] for p in range(n_phase))


@pytest.mark.parametrize("n_phase", [3, 6])
def test_phases_flagged_launch(oracle, ctx, monkeypatch, n_phase):
    """The same plans in the one flagged launch: the counters give the plan's sizes, no row chains."""
    c = _run(oracle, ctx, monkeypatch, "BIG", {"SG_SSSP_PHASES": n_phase}, flagged="1")
    _check_plan(c, n_phase, phased=False)


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("name", ["SMALL", "STAR"])
def test_six_phases_small_and_empty(oracle, ctx, monkeypatch, name, chain):
    """SMALL: phases smaller than the grid (15 rows) and an empty one.  STAR: phase 0 is the hub
    alone, phase 1 every leaf, four empty launches."""
    c = _run(oracle, ctx, monkeypatch, name, {"SG_SSSP_PHASES": 6, "SG_SSSP_CHAIN": chain})
    want = _check_plan(c, 6)
    assert 0 in want
    if name == "STAR":
        assert want == [1, 599, 0, 0, 0, 0]
    _check_chain(c, chain, [])


# ---- b. blocks and subsets at 4 phases

@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("case", ["block", "subset", "subset_block"])
def test_four_phases_blocks_and_subsets(oracle, ctx, monkeypatch, case, chain):
    """Rows [600, 1900) of BIG; a shuffled used list of 1,801 nodes (n_used % 4 != 0: the scalar
    output path; the plan's exact seeds are off, the chain's stay on); rows [300, 1500) of it.  The
    plan sees the block's rows only."""
    used, rows = {"block": (None, (600, 1900)), "subset": (C.SUBSET, None), "subset_block": (C.SUBSET, (300, 1500))}[case]
    c = _run(oracle, ctx, monkeypatch, "BIG", {"SG_SSSP_PHASES": 4, "SG_SSSP_CHAIN": chain}, used=used, rows=rows)
    want = _check_plan(c, 4)
    assert all(want)
    _check_chain(c, chain, [1])  # phase 1 has more rows than the grid in each case
    if chain == "1" and case != "block":
        assert c["n_exact"] > 0


# ---- c. plan knobs at 3 phases

@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("knob", [{"SG_SSSP_HOPS": 1}, {"SG_SSSP_HOPS": 2}, {"SG_SSSP_EXACT": 0}, {"SG_SSSP_BOUNDS": 8}],
                         ids=lambda k: "-".join(f"{a[8:]}{b}" for a, b in k.items()))
@pytest.mark.parametrize("name", ["BIG", "HUBS"])
def test_plan_knobs(oracle, ctx, monkeypatch, name, knob, chain):
    """k_plan_bounds' hop levels, its exact seeds off (no chained row takes exact seeds either), and
    eight bound rows per row.  The phase sets do not depend on any of them."""
    c = _run(oracle, ctx, monkeypatch, name, dict(knob, SG_SSSP_PHASES=3, SG_SSSP_CHAIN=chain))
    _check_plan(c, 3)
    _check_chain(c, chain, [1] if name == "BIG" else [])
    if "SG_SSSP_EXACT" in knob:
        assert c["n_exact"] == 0
    elif chain == "1" and name == "BIG":
        assert c["n_exact"] > 0


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("name", ["STAR_Z", "HUBS_Z"])
def test_zero_loss_frontier_past_the_clamp(oracle, ctx, monkeypatch, name, chain):
    """Every arc zero-loss at SG_SSSP_HOPS=3: a leaf's second level is the hub's 599 arcs, past
    k_plan_bounds' frontier of 256 entries (the rest are dropped: fewer seeds, the same table)."""
    c = _run(oracle, ctx, monkeypatch, name, {"SG_SSSP_PHASES": 3, "SG_SSSP_HOPS": 3, "SG_SSSP_CHAIN": chain})
    _check_plan(c, 3)
    _check_chain(c, chain, [])


# ---- d. search knobs

@pytest.mark.parametrize("seeds", ["0", "2"])
@pytest.mark.parametrize("knob", [{"SG_SSSP_CLAIM": 1}, {"SG_SSSP_CLAIM": 5}, {"SG_SSSP_LANE_DEG": 0}, {"SG_SSSP_LANE_DEG": 3},
                                  {"SG_SSSP_LANE_DEG": 4096}, {"SG_SSSP_SLEEP": 1}],
                         ids=lambda k: "-".join(f"{a[8:]}{b}" for a, b in k.items()))
def test_search_knobs(oracle, ctx, monkeypatch, knob, seeds):
    """The claim width, the lane path against the expansion path (out-degrees 2..160: always the
    expansion path, the lane path below degree 4 only, always the lane path) and the idle back-off,
    without a plan and with three phases."""
    c = _run(oracle, ctx, monkeypatch, "HUBS", dict(knob, SG_SSSP_PHASES=3), seeds=seeds)
    if seeds == "2":
        _check_plan(c, 3)
    else:  # no plan: one launch, no phase counters
        assert (c["unbounded"], c["bounded"]) == (1, 0) and c["sizes"] == [0] * PHASES_MAX
        assert c["n_chained"] > 0


def test_delta_buckets_with_chain_and_phases(oracle, ctx, monkeypatch):
    """1 us buckets (the arcs are 1-4 us): the bucketed order with chained and bounded starts."""
    c = _run(oracle, ctx, monkeypatch, "HUBS", {"SG_APSP_DELTA": 1000, "SG_SSSP_PHASES": 3, "SG_SSSP_CHAIN": 1})
    _check_plan(c, 3)
    c = _run(oracle, ctx, monkeypatch, "BIG", {"SG_APSP_DELTA": 1000, "SG_SSSP_PHASES": 3, "SG_SSSP_CHAIN": 1})
    _check_plan(c, 3)
    _check_chain(c, "1", [1])


# ---- e. landmarks

@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("n_phase", [2, 5, 6])
@pytest.mark.parametrize("n_land", [8, 64])
def test_landmarks_whole_table(oracle, ctx, monkeypatch, n_land, n_phase, chain):
    """The landmark launch runs: phases + 1 launches (6 phases are clamped to 5, then 6 launches),
    phase 0 holds exactly the landmarks, and with the chain on rows chain inside the landmark-bounded
    phase (586 or 642 rows)."""
    c = _run(oracle, ctx, monkeypatch, "BIG",
             {"SG_SSSP_LANDMARKS": n_land, "SG_SSSP_PHASES": n_phase, "SG_SSSP_CHAIN": chain})
    want = _check_plan(c, n_phase, n_land)
    assert c["bounded"] == min(n_phase, 5)
    assert want[0] == n_land
    _check_chain(c, chain, [1])


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("name,n_land", [("STAR", 8), ("BIG", 100000)])
def test_more_landmarks_than_phase_0(oracle, ctx, monkeypatch, name, n_land, chain):
    """n_land >= |phase 0|: no row is a landmark, every phase moves one later and the first launch
    has no rows."""
    c = _run(oracle, ctx, monkeypatch, name, {"SG_SSSP_LANDMARKS": n_land, "SG_SSSP_CHAIN": chain})
    want = _check_plan(c, 2, n_land)
    assert want[0] == 0 and c["bounded"] == 2
    _check_chain(c, chain, [1] if name == "BIG" else [])


@pytest.mark.parametrize("chain", ["1", "0"])
def test_landmarks_with_saturated_rows(oracle, ctx, monkeypatch, chain):
    """FAR with every node used: landmark rows hold saturated keys and distances at or above
    2^32 - 1 ns (no bound through those), and the wide kernel finishes the table."""
    c = _run(oracle, ctx, monkeypatch, "FAR", {"SG_SSSP_LANDMARKS": 8, "SG_SSSP_CHAIN": chain})
    _check_plan(c, 2, 8)
    _check_chain(c, chain, [])
    assert (_graph(oracle, "FAR")[1] >= 0xFFFFFFFF).any() and c["wide"] > 0


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("spin", ["24", "40"])
def test_landmark_rows_that_gave_up(oracle, ctx, monkeypatch, spin, chain):
    """SG_SSSP_SPIN_MAX: searches give up and their rows take the wide kernel; a landmark row that
    gave up was never written (the buffer holds the poison) and must give no bounds.  How many give
    up depends on timing, so only the table is asserted: on one MI355X every row gave up at 16,
    about two thirds at 24 (rows bounded through landmarks next to landmark rows never written)
    and none at 40."""
    c = _run(oracle, ctx, monkeypatch, "SMALL",
             {"SG_SSSP_LANDMARKS": 64, "SG_SSSP_SPIN_MAX": spin, "SG_SSSP_CHAIN": chain})
    _check_plan(c, 2, 64)


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("kb", [1, 8])
def test_landmark_bound_counts(oracle, ctx, monkeypatch, kb, chain):
    """One bound row per row, and eight: more than the landmark bounds' four."""
    c = _run(oracle, ctx, monkeypatch, "BIG", {"SG_SSSP_LANDMARKS": 64, "SG_SSSP_BOUNDS": kb, "SG_SSSP_CHAIN": chain})
    _check_plan(c, 2, 64)
    _check_chain(c, chain, [1])


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("case", ["block", "subset", "subset_block"])
def test_landmarks_blocks_and_subsets(oracle, ctx, monkeypatch, case, chain):
    used, rows = {"block": (None, (600, 1900)), "subset": (C.SUBSET, None), "subset_block": (C.SUBSET, (300, 1500))}[case]
    c = _run(oracle, ctx, monkeypatch, "BIG", {"SG_SSSP_LANDMARKS": 16, "SG_SSSP_PHASES": 3, "SG_SSSP_CHAIN": chain},
             used=used, rows=rows)
    want = _check_plan(c, 3, 16)
    assert want[0] == 16
    _check_chain(c, chain, [1])


def test_directed_graph_takes_no_landmarks(oracle, ctx, monkeypatch):
    """SG_SSSP_LANDMARKS on a directed graph is ignored (D[L][s] is no bound on D[s][L]): the plan
    runs its phases without a landmark launch.  (The directed shapes of test_option_kernels
    therefore run the plain phased plan.)"""
    c = _run(oracle, ctx, monkeypatch, "DIRECTED", {"SG_SSSP_LANDMARKS": 8, "SG_SSSP_PHASES": 3})
    _check_plan(c, 3, 0)
    assert c["bounded"] == 2 and c["n_chained"] == 0
