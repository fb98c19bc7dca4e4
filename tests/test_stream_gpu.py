"""Every single-context entry-point family on a context whose stream is a caller's non-blocking
stream (sg_ctx_set_stream), results bit-exact against the suite's references.  The harness, the
cases and what each step catches: tests/stream_cases.py; the cases' qualification on the CPU:
tests/test_stream_cases_cpu.py.

The two controls come first: without them a green run proves nothing."""
import numpy as np
import pytest

import stream_cases as ST
from conftest import set_apsp_kernel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h():
    """The module's context on S = torch.cuda.Stream(), closed at teardown."""
    import shadow_amd

    shadow_amd.load()
    hs = ST.Harness()
    yield hs
    hs.close()


@pytest.fixture(scope="module")
def reader(h):
    """(a second non-blocking stream that runs while S sits in the delay, or None; streams tried)."""
    return ST.find_reader(h)


def _compare(case, got):
    want = case.want()
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape)
        same = g.view(np.uint8) == w.view(np.uint8)
        if not same.all():
            bad = np.flatnonzero((g != w).ravel()) if g.dtype != np.float32 else np.flatnonzero(
                (g.view(np.uint32) != w.view(np.uint32)).ravel())
            stale = case.ref("A")[k]
            stale = ST.plus_poison(stale) if k in case.ADDS else stale
            what = "equals the stale set A's reference" if np.array_equal(g, stale) else (
                "is all poison" if (g.view(np.uint8) == ST.POISON_BYTE).all() else "is neither A's reference nor poison")
            raise AssertionError(f"{case.name}: {k} differs from B's reference in {len(bad)} of {w.size} entries, first at "
                                 f"{int(bad[0])} (got {g.ravel()[bad[0]]}, want {w.ravel()[bad[0]]}); the output {what}")


# ---- controls
def test_delay_opens_a_window(h, reader):
    """A copy on a second fresh non-blocking stream, issued while S sits in the delay with B's
    write queued behind it, reads A: the delay gives a misplaced kernel time to run first."""
    R, tried = reader
    assert R is not None, f"none of {tried} reader streams ran while S sat in the delay: the harness cannot be shown " \
                          "to detect anything"


def test_delay_outlasts_a_call(h):
    """The delay as torch events on S measure it, against 4 W (stream_cases.W_MS)."""
    import torch

    with h.on_stream():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h.S.synchronize()
        e0.record()
        h.delay()
        e1.record()
        h.S.synchronize()
    ms = e0.elapsed_time(e1)
    print(f"delay: {ms:.1f} ms for {h.cycles} cycles; W = {ST.W_MS} ms")
    assert ms >= 4 * ST.W_MS


def test_caller_side_violation_is_seen(h, reader):
    """The caller breaking the header's rule: a context on the reader stream, the inputs of
    sg_link_queue written on S behind the delay.  The call returns A's reference exactly: a stale
    read is visible in a real call's results (and safe: A is valid)."""
    import torch

    from shadow_amd import Context

    R, _ = reader
    assert R is not None, "no reader stream (test_delay_opens_a_window)"
    case = ST.LinkQueueCase()
    a, b = case.sets()
    want = case.ref("A")
    ctx2 = Context(0, stream=R.cuda_stream)
    try:
        with h.on_stream():
            din = {k: h.dev(v) for k, v in a.items()}
            d_b = {k: h.dev(v) for k, v in b.items()}
            dout = {k: h.dev(np.zeros_like(v)) for k, v in want.items()}
            h.S.synchronize()
        with torch.cuda.stream(R):
            for r in ("1", "2"):  # warm
                case.device_call(ctx2, din, dout, r)
            R.synchronize()
        with h.on_stream():
            h.delay()
            for k in din:
                din[k].copy_(d_b[k])
        with torch.cuda.stream(R):
            for r in ("1", "2"):
                case.device_call(ctx2, din, dout, r)
            R.synchronize()
            got = {k: dout[k].cpu().numpy().view(want[k].dtype)[:want[k].size] for k in want}
        h.S.synchronize()
    finally:
        ctx2.close()
    for k, w in want.items():
        assert np.array_equal(got[k], w), f"{k}: not A's reference"
    wb = case.ref("B")
    assert any(not np.array_equal(got[k], wb[k]) for k in wb)


# ---- table builds
@pytest.mark.parametrize("case", ST.BUILD_CASES, ids=lambda c: c.name)
def test_table_builds(h, case, monkeypatch):
    """sg_routing_build into device buffers (whole table, then a row block) under every kernel
    selection of test_routing_gpu.py and on the dense search; the one-shot build with
    SG_BUILD_FUSED 1 and 0; sg_routing_info_fill in blocks of 64 rows; sg_routing_min_latency.  "lds_bounded" runs the
    plan's side stream, the fill the copy stream (stream_cases.BuildCase, InfoFillCase)."""
    set_apsp_kernel(monkeypatch, getattr(case, "kernel", "lds"))
    for k, v in getattr(case, "env", {}).items():
        monkeypatch.setenv(k, v)
    _compare(case, case.gpu(h))


# ---- trees
@pytest.mark.parametrize("case", ST.TREE_CASES, ids=lambda c: c.name)
def test_trees(h, case, monkeypatch):
    """sg_routing_tree (device table in) and sg_routing_build_tree (device outputs), on the LDS
    path and with SG_TREE_LDS=0."""
    monkeypatch.setenv("SG_TREE_LDS", str(case.lds))
    _compare(case, case.gpu(h))


# ---- the link family
@pytest.mark.parametrize("case", ST.LINK_CASES, ids=lambda c: c.name)
def test_link_family(h, case):
    """The device forms of sg_link_load, sg_link_load_packets, sg_tree_paths,
    sg_tree_paths_packets, sg_link_trace_packets, sg_link_series_packets (two rounds into one
    accumulator) and sg_link_queue (two calls, link_free chained) on the tie graph's round."""
    _compare(case, case.gpu(h))


# ---- delivery
@pytest.mark.parametrize("case", ST.DELIVER_CASES, ids=lambda c: c.name)
def test_delivery(h, case):
    """sg_hosts_set_state and sg_hosts_skip, sg_table_pack, two rounds of sg_deliver_round with
    packet counters set on either table form, sg_hosts_get_state; and the rounds with
    stats == NULL (which synchronise as well: the header says so since this test found them
    waiting); the sharded halves sg_deliver_source, sg_deliver_bucket, sg_deliver_source_padded
    (must return while the delay still runs), sg_deliver_pad_to_compact, sg_deliver_bucket_padded."""
    _compare(case, case.gpu(h))


# ---- the packet wire
@pytest.mark.parametrize("case", ST.WIRE_CASES, ids=lambda c: c.name)
def test_wire(h, case):
    """sg_wire_push, sg_wire_stamp_records[_padded], sg_wire_push_records[_padded] (each must
    return while the delay still runs), sg_wire_pop after each round, sg_wire_get_state and
    sg_wire_set_state."""
    _compare(case, case.gpu(h))


# ---- lanes
@pytest.mark.parametrize("case", ST.LANE_CASES, ids=lambda c: c.name)
def test_lanes(h, case):
    """sg_codel_run, sg_inbound_run, sg_inbound_run_ordered, sg_outbound_run and
    sg_outbound_run_qdisc (fifo and round-robin) on the lane_cases shape, two calls each so that
    state carries over, then the state itself (sg_codel_get_state, sg_inbound_get_state,
    sg_outbound_get_state, sg_outbound_get_qdisc_state)."""
    _compare(case, case.gpu(h))
