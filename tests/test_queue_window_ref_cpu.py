"""The windowed link queues' reference (queue_window_ref.py) against itself, no GPU: the loop the
library runs equals the definition, keeps its two invariants (asserted inside `jacobi`) and its
iteration bound; re-feeding the pending records gives the closed solution, call by call and
through a session."""
import re
from pathlib import Path

import numpy as np
import pytest

import outcomes_cases as OC
import queue_carry_cases as CC
import queue_drop_cases as DC
import queue_window_cases as WC
import queue_window_ref as WR

ROOT = Path(__file__).resolve().parent.parent
ARRAYS = ("wait", "done", "ahead", "link_free", "busy", "wait_max", "wait_sum", "ahead_max", "pending")


def _same(a, b, what):
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"
    assert a["lost"] == b["lost"], what


def _both(c, H, drop, packets, what):
    rc, want = WR.define(c, H, drop, packets)
    assert rc == WR.OK
    rc, got = WR.jacobi(c, H, drop, packets, exact=WC.closed_enter(c, drop))
    assert rc == WR.OK
    _same(got, want, what)
    assert got["iters"] <= WR.iteration_bound(c, H), (what, got["iters"], WR.iteration_bound(c, H))
    assert got["active"] <= got["iters"] * len(c["enter"])
    return want, got


def test_the_flag_is_the_headers():
    h = (ROOT / "include" / "shadow_gpu.h").read_text()
    assert int(re.search(r"#define\s+" + WR.WINDOW_FLAG + r"\s+(0x[0-9A-Fa-f]+)u", h).group(1), 16) == WR.WINDOW


def test_hand_example():
    c = WC.hand()
    # H = 118: C's second record enters link 1 at 118, strict: pending; B's second (117) is settled
    rc, out = WR.define(c, 118, False, True)
    assert rc == WR.OK
    assert out["pending"].tolist() == [False, False, True, True, False, False]
    assert out["done"][:6].tolist() == [110, 120, 125, 118, 110, 127]
    assert out["wait"][6:].tolist() == [19, 20, 10] and out["ahead"][6:].tolist() == [WR.IN_FLIGHT, OR_ARRIVED, WR.IN_FLIGHT]
    assert out["done"][6:].tolist() == [1019, 1020, 1010]
    assert out["link_free"].tolist() == [120, 0, 127]
    for H in WC.horizons(c, False):
        _both(c, H, False, True, f"hand {H}")


OR_ARRIVED = 0xFFFFFFFE


@pytest.mark.parametrize("k", CC.STAIRS)
def test_staircases(k):
    c = WC.staircase(k)
    for H in WC.horizons(c, False):
        _both(c, H, False, True, f"staircase {k} at {H}")


def test_a_wait_pushes_a_record_past_the_horizon():
    c = WC.pushed_past()
    want, _ = _both(c, 110, False, True, "pushed past")
    i = int(np.flatnonzero((c["packet"] == 1) & (c["enter"] == 106))[0])
    assert want["pending"][i] and int(want["done"][i]) == 130  # (enter 106 < H, carried 125 + 5)
    assert want["pending"].sum() == 1


def test_drops_across_the_horizon():
    (c, H, _), (_, H2, _) = WC.drop_cases()[:2]
    want, _ = _both(c, H, True, True, "settled drop")
    p1 = np.flatnonzero(c["packet"] == 1)
    assert not want["pending"][p1].any() and want["lost"] == 1
    assert sorted(want["done"][p1].tolist()) == [110, WR.MAX, WR.MAX]
    want, _ = _both(c, H2, True, True, "drop beyond H")
    assert want["pending"][p1].all() and want["lost"] == 0
    for c, H, what in WC.drop_cases():
        for packets in (False, True):
            _both(c, H, True, packets, what)


@pytest.mark.parametrize("seed", range(12))
def test_jacobi_is_the_definition_on_random_instances(seed):
    c = OC.random_case(seed)
    for drop in (False, True):
        hs = WC.horizons(c, drop)
        for H in hs + [int(x) for x in np.random.default_rng(seed).integers(hs[0], hs[3] + 1, 3)]:
            _both(c, H, drop, True, f"seed {seed} drop {drop} H {H}")


def test_the_whole_range_is_the_unflagged_call():
    for seed in range(4):
        c = OC.random_case(seed)
        for carry_drop in (False, True):
            want, n = OC.want(c, True, carry_drop)
            rc, got = WR.define(c, WR.MAX, carry_drop, True)
            assert rc == WR.OK and not got["pending"].any() and got["lost"] == n
            for k in WR.QR.FIELDS:
                assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("drop", (False, True))
@pytest.mark.parametrize("k", (1, 2, 5, 17))
def test_rounds_by_re_feeding_are_one_carried_call(k, drop):
    for seed in range(4):
        c = OC.random_case(100 + seed)
        whole, got = WC.run_session(c, k, seed, drop)
        want = WC.session_want(whole, drop)
        for name in ("wait", "done", "delay", "arrive", "lost", "drop_link", "link_free"):
            assert np.array_equal(got[name], want[name]), (name, k, seed)
        for name, v in want["sums"].items():
            assert np.array_equal(got["sums"][name], v), (name, k, seed)


def test_re_feeding_keeps_the_tie_order():
    """In-flight packets are numbered before a round's new ones and keep their order: two records
    that meet on a link at one carried time in a later call are served in (round, packet) order,
    the order of the whole trace's packet numbers."""
    c = OC.random_case(3)
    whole, rs = WC.rounds(c, 5, 1)
    seen = -1
    for _, _, _, new in rs:
        assert (np.diff(new) > 0).all() and (len(new) == 0 or new[0] > seen)
        seen = int(new[-1]) if len(new) else seen


def test_longer_cases_qualify():
    c = WC.segments(65)
    hs = WC.horizons(c, True)
    for H in hs[1:3]:
        want, got = _both(c, H, True, True, "segments 65")
        assert 0 < want["pending"].sum() < len(c["enter"])
        assert got["active"] < got["iters"] * len(c["enter"])
