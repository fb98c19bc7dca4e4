"""GPU parity of the routers' inbound CoDel queues (sg_codel_*) against the
oracle (router/codel_queue.rs restated; the oracle itself is pinned by the
reference's unit tests in tests/test_codel_cpu.py).  Bit-exact: pop results,
packet statuses and the whole per-host state, across consecutive calls."""
import numpy as np
import pytest

import codel_cases as cc
import codel_ref as ref
import lane_cases
from shadow_amd import ShadowGpuError, _capi
from shadow_amd.router import CoDelEvents, CoDelQueues

pytestmark = pytest.mark.gpu
T0 = 946684800 * 10**9
MS = 10**6
KEYS = ("flags", "interval_end", "drop_next", "cur", "prev", "bytes", "head", "tail")


def _status(n):
    import torch

    return torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")


def _same_state(O, got, want):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    # live ring slots only: [head, tail) per host, the counters taken modulo 2^32
    i = ref.live_slots(want)
    for k in ("ring_pkt", "ring_ts", "ring_len"):
        assert np.array_equal(got[k][i], want[k][i]), k


def _run_both(O, q, ostate, gstat, ostat, host, kind, t, pkt, ln):
    ev = CoDelEvents.from_numpy(host, kind, t, pkt, ln)
    res, nd = q.run(ev, gstat)
    before = (ostat == 2).sum()
    want = O.codel_run(ostate, host, kind, t, pkt, ln, ostat)
    assert np.array_equal(res.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(gstat.cpu().numpy()[: len(ostat)], ostat)
    assert nd == (ostat == 2).sum() - before
    return want


_host_times, _stream = cc.host_times, cc.stream   # drawn in codel_cases.py: the CPU tests run them too


def test_reference_drop_many_sequence(oracle, ctx):
    """codel_queue.rs:494-534 event by event: state equal after every event."""
    q = CoDelQueues(1, 64, ctx=ctx)
    os_ = oracle.codel_state(1, q.cap)
    gstat, ostat = _status(64), np.zeros(64, np.uint8)
    start, end = T0 + 1000 * MS, T0 + 1000000 * MS
    seq = [(0, start)] * 20 + [(1, start + 10 * MS), (1, start + 110 * MS), (1, end)]
    for i, (k, t) in enumerate(seq):
        _run_both(oracle, q, os_, gstat, ostat, [0], [k], [t], [i], [1028])
        _same_state(oracle, q.get_state(), os_)
    st = q.get_state()
    assert st["tail"][0] - st["head"][0] == 1 and st["cur"][0] == 16 and not st["flags"][0] & 1


@pytest.mark.parametrize("gap_ms,p_pop,layout", [(3, 0.45, ""), (1, 0.3, ""), (20, 0.5, ""), (3, 0.45, "0"),
                                                  (1, 0.3, "1")])
def test_random_streams_over_calls(oracle, ctx, monkeypatch, gap_ms, p_pop, layout):
    """500 hosts, three consecutive calls of 60k events: state carries over.  ~120 events
    per host: the blocks take lane-major chunks by default (sg_lanes.h ChunkMap); layout
    forces contiguous ("0") or lane-major ("1") chunks."""
    if layout:
        monkeypatch.setenv("SG_LANE_MAJOR", layout)
    rng = np.random.default_rng(gap_ms)
    H, E = 500, 60000
    q = CoDelQueues(H, 4096, ctx=ctx)
    os_ = oracle.codel_state(H, q.cap)
    gstat, ostat = _status(3 * E), np.zeros(3 * E, np.uint8)
    t0 = T0 + 10**9
    for c in range(3):
        ev = _stream(rng, H, E, t0, gap_ms, p_pop, n_pkt0=c * E)
        _run_both(oracle, q, os_, gstat, ostat, *ev)
        t0 = int(ev[2].max()) + 1
    _same_state(oracle, q.get_state(), os_)
    assert (ostat == 2).any() and (ostat == 1).any()


@pytest.mark.parametrize("layout", lane_cases.LAYOUTS)
def test_layout_matrix(oracle, ctx, monkeypatch, layout):
    """k_codel's four walk sites on one small shape (lane_cases.py: 128 hosts, 64 x 48 events,
    one host of 3,000, two of 3; E = 6,078).  CH = 1,024, LK = 16: unset launches LM = 2 (6,078 >
    2 x 1,024 x 2 = 4,096), where block 0 goes lane-major (3 x (10 + 16) = 78 against 3 x (10 + 48)
    = 174) and block 1 stays contiguous (188 x 26 = 4,888 against 3 x (10 + 1,002) = 3,036); "0"
    launches LM = 0 and "1" LM = 1.  Two calls (state carries over), drawn as _stream draws them."""
    lane_cases.set_layout(monkeypatch, layout)
    rng = np.random.default_rng(31)
    host = lane_cases.host_column()
    H, E = lane_cases.H, len(host)
    q = CoDelQueues(H, lane_cases.RING_CAP, ctx=ctx)
    os_ = oracle.codel_state(H, q.cap)
    gstat, ostat = _status(2 * E), np.zeros(2 * E, np.uint8)
    t0 = T0 + 10**9
    for c in range(2):
        kind = (rng.random(E) < 0.45).astype(np.uint8)
        t = _host_times(host, rng.integers(0, 3 * MS, E), t0)
        pkt = (c * E + np.arange(E)).astype(np.uint32)
        ln = rng.integers(40, 1500, E).astype(np.uint32)
        _run_both(oracle, q, os_, gstat, ostat, host, kind, t, pkt, ln)
        _same_state(oracle, q.get_state(), os_)
        t0 = int(t.max()) + 1
    assert (ostat == 2).any() and (ostat == 1).any()
    assert (os_["tail"] != os_["head"]).any()  # live ring slots were compared


@pytest.mark.parametrize("layout", ["", "1"])
def test_queue_deeper_than_a_chunk(oracle, ctx, monkeypatch, layout):
    """One host's queue grows past a staged chunk (1024 events) and drains in later
    chunks: its elements are read back from the ring in HBM, which the kernel
    writes only for what outlives each chunk.  Then push/pop cycles wrap the ring
    indices several times.  Neighbour hosts have a few events each.  layout "1":
    lane-major chunks of 16 events per host (the default keeps this block contiguous)."""
    if layout:
        monkeypatch.setenv("SG_LANE_MAJOR", layout)
    rng = np.random.default_rng(5)
    cap = 4096
    q = CoDelQueues(3, cap, ctx=ctx)
    os_ = oracle.codel_state(3, q.cap)
    n_pkt = 40000
    gstat, ostat = _status(n_pkt), np.zeros(n_pkt, np.uint8)
    t0 = T0 + 10**9
    # host 1: 2500 pushes 1 us apart, then 2500 pops 2 ms apart (drop mode), in one call
    h1_kind = np.r_[np.zeros(2500, np.uint8), np.ones(2500, np.uint8)]
    h1_t = np.r_[t0 + np.arange(2500) * 1000, t0 + 3 * MS + np.arange(2500) * 2 * MS].astype(np.uint64)
    host = np.r_[np.zeros(3, np.uint32), np.ones(5000, np.uint32), np.full(3, 2, np.uint32)]
    kind = np.r_[np.array([0, 1, 1], np.uint8), h1_kind, np.array([0, 0, 1], np.uint8)]
    t = np.r_[t0 + np.arange(3) * MS, h1_t, t0 + np.arange(3) * MS].astype(np.uint64)
    pkt = np.arange(len(host), dtype=np.uint32)
    ln = rng.integers(40, 1500, len(host)).astype(np.uint32)
    _run_both(oracle, q, os_, gstat, ostat, host, kind, t, pkt, ln)
    _same_state(oracle, q.get_state(), os_)
    # wrap: calls of bursts (push 600, pop 400) on host 1, queue depth stepping up and down
    tn, p0 = int(t.max()) + MS, len(host)
    for c in range(12):
        k = np.r_[np.zeros(600, np.uint8), np.ones(400 if c % 3 else 900, np.uint8)]
        tt = (tn + np.arange(len(k)) * 50_000).astype(np.uint64)
        hh = np.ones(len(k), np.uint32)
        pp = (p0 + np.arange(len(k))).astype(np.uint32)
        _run_both(oracle, q, os_, gstat, ostat, hh, k, tt, pp, rng.integers(40, 1500, len(k)).astype(np.uint32))
        tn, p0 = int(tt.max()) + MS, p0 + len(k)
    _same_state(oracle, q.get_state(), os_)
    st = q.get_state()
    assert int(st["tail"][1]) > 2 * cap  # the ring indices wrapped
    assert (ostat == 2).any() and (ostat == 1).any()


@pytest.mark.parametrize("layout", ["", "1"])
def test_large_single_call(oracle, ctx, monkeypatch, layout):
    """100k hosts, 1M events (the bench shape), one call; layout "1" forces lane-major chunks."""
    if layout:
        monkeypatch.setenv("SG_LANE_MAJOR", layout)
    rng = np.random.default_rng(11)
    H, E = 100000, 1000000
    q = CoDelQueues(H, 256, ctx=ctx)
    os_ = oracle.codel_state(H, q.cap)
    gstat, ostat = _status(E), np.zeros(E, np.uint8)
    _run_both(oracle, q, os_, gstat, ostat, *_stream(rng, H, E, T0 + 10**9, 30, 0.4))
    _same_state(oracle, q.get_state(), os_)


def test_many_events_per_host(oracle, ctx):
    """The C5 shape per block (~200 events per host, 1 ms round): 6,400 hosts, 1.28M events,
    two calls; the blocks take lane-major chunks."""
    rng = np.random.default_rng(12)
    H, E = 6400, 1280000
    q = CoDelQueues(H, 1024, ctx=ctx)
    os_ = oracle.codel_state(H, q.cap)
    gstat, ostat = _status(2 * E), np.zeros(2 * E, np.uint8)
    t0 = T0 + 10**9
    for c in range(2):
        ev = _stream(rng, H, E, t0, 0.01, 0.5, n_pkt0=c * E)
        _run_both(oracle, q, os_, gstat, ostat, *ev)
        t0 = int(ev[2].max()) + 1
    _same_state(oracle, q.get_state(), os_)


def test_state_roundtrip_and_empty_call(ctx):
    q = CoDelQueues(3, 8, ctx=ctx)
    st = q.get_state()
    st["flags"][1] = 1
    st["bytes"][2] = 77
    q.set_state(st)
    st2 = q.get_state()
    assert st2["flags"][1] == 1 and st2["bytes"][2] == 77
    res, nd = q.run(CoDelEvents.from_numpy([], [], [], [], []), _status(1))
    assert len(res) == 0 and nd == 0


def test_errors(ctx):
    q = CoDelQueues(4, 2, ctx=ctx)  # ring of 2
    with pytest.raises(ShadowGpuError) as e:
        q.run(CoDelEvents.from_numpy([0, 0, 0], [0, 0, 0], [T0] * 3, [0, 1, 2], [100] * 3), _status(8))
    assert e.value.code == _capi.SG_ERR_CAPACITY
    q = CoDelQueues(4, 8, ctx=ctx)
    with pytest.raises(ShadowGpuError) as e:
        q.run(CoDelEvents.from_numpy([2, 1], [0, 0], [T0] * 2, [0, 1], [100] * 2), _status(8))
    assert e.value.code == _capi.SG_ERR_UNSORTED
    with pytest.raises(ShadowGpuError) as e:
        q.run(CoDelEvents.from_numpy([0, 9], [0, 0], [T0] * 2, [0, 1], [100] * 2), _status(8))
    assert e.value.code == _capi.SG_ERR_INVALID_ARG


def test_good_state_mix(oracle, ctx):
    """Most hosts in CoDel's good state (microsecond gaps), a few with queues that
    stand past TARGET and enter drop mode, in the same blocks and chunks; four
    calls, so elements pushed in one call are popped from the ring in the next,
    and hosts cross chunk boundaries."""
    rng = np.random.default_rng(23)
    H, E = 20000, 200000
    q = CoDelQueues(H, 512, ctx=ctx)
    os_ = oracle.codel_state(H, q.cap)
    gstat, ostat = _status(4 * E), np.zeros(4 * E, np.uint8)
    t0 = T0 + 10**9
    slow = rng.random(H) < 0.02
    for c in range(4):
        host = np.sort(rng.integers(0, H, E)).astype(np.uint32)
        # a few hosts get long runs (several chunks' worth of events)
        host[: 3000] = 7
        host[3000: 5500] = 1000 + c
        host = np.sort(host)
        kind = (rng.random(E) < np.where(slow[host], 0.3, 0.5)).astype(np.uint8)
        t = _host_times(host, rng.integers(0, np.where(slow[host], 4 * MS, 2000)), t0)
        pkt = (c * E + np.arange(E)).astype(np.uint32)
        ln = rng.integers(40, 1500, E).astype(np.uint32)
        _run_both(oracle, q, os_, gstat, ostat, host, kind, t, pkt, ln)
        t0 = int(t.max()) + 1
    _same_state(oracle, q.get_state(), os_)
    assert (ostat == 2).any() and (ostat == 1).any()


def test_bytes_below_ring_contents(oracle, ctx):
    """A state whose byte count is below what its ring holds (set_state): pops
    saturate the count at zero (codel_queue.rs pop_front)."""
    H = 64
    q = CoDelQueues(H, 16, ctx=ctx)
    os_ = oracle.codel_state(H, q.cap)
    gstat, ostat = _status(1000), np.zeros(1000, np.uint8)
    t0 = T0 + 10**9
    host = np.repeat(np.arange(H, dtype=np.uint32), 4)
    kind = np.tile(np.array([0, 0, 0, 0], np.uint8), H)
    t = (t0 + np.tile(np.arange(4), H) * 1000).astype(np.uint64)
    pkt = np.arange(4 * H, dtype=np.uint32)
    ln = np.full(4 * H, 1000, np.uint32)
    _run_both(oracle, q, os_, gstat, ostat, host, kind, t, pkt, ln)
    st = q.get_state()
    st["bytes"][::2] = 1500  # below the 4000 queued
    q.set_state(st)
    os_["bytes"][:] = st["bytes"]
    host = np.repeat(np.arange(H, dtype=np.uint32), 3)
    kind = np.ones(3 * H, np.uint8)
    t = (t0 + 10**6 + np.tile(np.arange(3), H) * 1000).astype(np.uint64)
    _run_both(oracle, q, os_, gstat, ostat, host, kind, t, np.zeros(3 * H, np.uint32), np.zeros(3 * H, np.uint32))
    _same_state(oracle, q.get_state(), os_)


# ---- the boundary cases (codel_cases.py), one lane per case ---------------------------------------
def _run_three(oracle, q, sm, so, gstat, mstat, ostat, ev):
    """One call on the device, the oracle and the model (codel_ref.py): results, statuses, drops."""
    want = _run_both(oracle, q, so, gstat, ostat, *ev)
    assert np.array_equal(ref.run(sm, *ev, mstat), want)
    assert np.array_equal(mstat, ostat)


def _three_states(oracle, q, sm, so):
    _same_state(oracle, q.get_state(), so)
    _same_state(oracle, sm, so)
    _same_state(oracle, so, q.get_state())   # and the device's live slots are the oracle's


def _queues(ctx, st0):
    q = CoDelQueues(len(st0["flags"]), st0["cap"], ctx=ctx)
    assert q.cap == st0["cap"]
    q.set_state(st0)
    return q, ref.copy_state(st0), ref.copy_state(st0)


@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("layout", lane_cases.LAYOUTS)
def test_boundary_cases(oracle, ctx, monkeypatch, layout, form):
    """Every case of codel_cases.py in one form, one host per case, all of them in one call (two:
    a twin's ring form pushes its elements in a call of its own); rings of 64 and, for the ring
    family's other half, of 4.  Pop results, statuses, n_dropped and the whole state against the
    oracle and the model, after each call."""
    lane_cases.set_layout(monkeypatch, layout)
    for cap in (64, 4):
        cs = [c for c in cc.of_cap(cap) if cc.has_form(c, form)]
        st0, calls, base = cc.build(cs, form, cap)
        q, sm, so = _queues(ctx, st0)
        gstat, mstat, ostat = _status(base[-1]), np.zeros(base[-1], np.uint8), np.zeros(base[-1], np.uint8)
        for ev in calls:
            _run_three(oracle, q, sm, so, gstat, mstat, ostat, ev)
            _three_states(oracle, q, sm, so)
        assert (ostat == 2).any() and (ostat == 1).any()


def _by_host(*parts):
    """Event columns of several sources as one call: grouped by ascending host, each host's in order."""
    cols = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    o = np.argsort(cols[0], kind="stable")
    return tuple(c[o] for c in cols)


@pytest.mark.parametrize("layout", lane_cases.LAYOUTS)
def test_boundary_cases_among_traffic(oracle, ctx, monkeypatch, layout):
    """The cases of every form (rings of 64: ~1,000 hosts) in shuffled order on the even hosts,
    the odd hosts between them carrying _stream traffic (~70 events each, so that an unset layout
    launches the per-block choice: E > 2 x 1,024 events per block), and a last host with 1,500
    events.  Lane-major chunks hold 16 events per host: a case of more events is walked in
    several chunks, resumed from the state the last one left, its window's elements read back
    from the ring; the long host's block walks contiguous chunks with the cases behind it."""
    lane_cases.set_layout(monkeypatch, layout)
    rng = np.random.default_rng(64)
    cs, forms = zip(*[(c, f) for f in cc.FORMS for c in cc.of_cap(64) if cc.has_form(c, f)])
    nc = len(cs)
    H = 2 * nc + 1
    st0, calls, base = cc.build(cs, forms, 64, hosts=2 * rng.permutation(nc), n_hosts=H)
    E, p0 = 70 * nc, base[-1]
    n_pkt = p0 + 2 * (E + 1500)
    q, sm, so = _queues(ctx, st0)
    gstat, mstat, ostat = _status(n_pkt), np.zeros(n_pkt, np.uint8), np.zeros(n_pkt, np.uint8)
    t0 = T0 + 10**9
    for c, ev in enumerate(calls):
        h, kind, t, pkt, ln = _stream(rng, nc, E, t0, 3, 0.5, n_pkt0=p0)
        big = _stream(rng, 1, 1500, t0, 1, 0.6, n_pkt0=p0 + E)   # more pops than pushes: 64 slots hold it
        all_ev = _by_host(ev, (2 * h + 1, kind, t, pkt, ln), (big[0] + np.uint32(H - 1),) + big[1:])
        assert np.bincount(all_ev[0]).max() >= 1500 and len(all_ev[0]) > 2 * 1024 * ((H + 63) // 64)
        _run_three(oracle, q, sm, so, gstat, mstat, ostat, all_ev)
        _three_states(oracle, q, sm, so)
        t0, p0 = int(t.max()) + 1, p0 + E + 1500
    assert (ostat[base[-1]:] == 2).any() and (ostat[base[-1]:] == 1).any()   # the traffic reached drop mode


def test_boundary_cases_one_event_per_call(oracle, ctx):
    """The entry and drop families (their twins too), ring form, one event of every case per run:
    the state written back after every event is the state the next event starts from."""
    cs = [c for c in cc.of_cap(64) if c["family"] in ("entry", "drop")]
    st0, calls, base = cc.build(cs, "ring", 64)
    q, sm, so = _queues(ctx, st0)
    gstat, mstat, ostat = _status(base[-1]), np.zeros(base[-1], np.uint8), np.zeros(base[-1], np.uint8)
    steps = 0
    for ev in calls:
        rank = np.arange(len(ev[0])) - np.searchsorted(ev[0], ev[0])   # an event's index within its host
        for j in range(int(rank.max()) + 1 if len(rank) else 0):
            _run_three(oracle, q, sm, so, gstat, mstat, ostat, tuple(a[rank == j] for a in ev))
            steps += 1
    _three_states(oracle, q, sm, so)
    assert steps >= 20 and (ostat == 2).sum() >= sum(c["expect"].get("drops", 0) for c in cs)


def test_state_roundtrip_every_field(ctx):
    """set_state then get_state returns every field of every host and every ring slot bit for
    bit, and so after an empty run: times with the high word set, counts above 2^32, every flag
    combination, head / tail straddling 2^32."""
    H, cap = 200, 8
    rng = np.random.default_rng(8)
    q = CoDelQueues(H, cap, ctx=ctx)
    st = q.get_state()
    u64 = lambda n: rng.integers(0, 2**64, n, dtype=np.uint64) | np.uint64(1 << 63)
    st["flags"][:] = np.arange(H) % 8
    for k in ("interval_end", "drop_next", "cur", "prev", "bytes"):
        st[k][:] = u64(H)
    st["cur"][:4] = np.array([2**32, 2**32 + 1, 2**64 - 1, 0], np.uint64)
    st["prev"][:4] = np.array([2**32 + 1, 2**32, 0, 2**64 - 1], np.uint64)
    st["head"][:] = rng.integers(0, 2**32, H, dtype=np.uint32)
    st["head"][:6] = (2**32 - 1, 2**32 - 2, 2**32 - cap, 0, 2**31, 2**31 - 1)
    st["tail"][:] = st["head"] + rng.integers(0, cap + 1, H).astype(np.uint32)   # wraps past 2^32
    assert (st["tail"][:3] < st["head"][:3]).any()
    st["ring_pkt"][:] = rng.integers(0, 2**32, H * cap, dtype=np.uint32)
    st["ring_ts"][:] = u64(H * cap)
    st["ring_len"][:] = rng.integers(0, 2**32, H * cap, dtype=np.uint32)
    want = ref.copy_state(st)
    q.set_state(st)
    for _ in range(2):
        got = q.get_state()
        assert sorted(got) == sorted(want) and got["cap"] == cap
        for k in want:
            if k != "cap":
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        res, nd = q.run(CoDelEvents.from_numpy([], [], [], [], []), _status(1))
        assert len(res) == 0 and nd == 0
