"""GPU parity of the packet wire (sg_wire_*, shadow_amd.wire.PacketWire) against the reference
model tests/wire_ref.py, bit-exact: the closed loop deliver_round -> push -> pop -> inbound
against the oracle chain, ties across rounds, window edges, the three sort tiers, capacity
errors, degenerate geometries, geometry independence and the checkpoint."""
import numpy as np
import pytest

import wire_cases as wc
from shadow_amd import ShadowGpuError, _capi, wire
from shadow_amd.router import InboundPipeline
from shadow_amd.wire import PacketWire
from shadow_amd.worker import DeviceTable, HostTable, PacketBatch, deliver_round
from wire_ref import NEVER, WireRef

pytestmark = pytest.mark.gpu
T0, MS = wc.T0, wc.MS
POP_KEYS = ("host", "time_ns", "packet", "len", "src_host", "event_id")
STATE_KEYS = ("host", "src_host", "packet", "len", "time_ns", "event_id")
UNSIGNED = dict(host=np.uint32, packet=np.uint32, len=np.uint32, src_host=np.uint32, time_ns=np.uint64,
                event_id=np.uint64)


def _np(t, key):
    return t.cpu().numpy().view(UNSIGNED[key])


def _same_pop(got, want, nxt, where=""):
    assert got["n"] == len(want["host"]), (where, got["n"], len(want["host"]))
    assert got["next_time_ns"] == nxt, (where, got["next_time_ns"], nxt)
    for k in POP_KEYS:
        assert np.array_equal(_np(got[k], k), want[k]), (where, k)


def _same_state(w, ref, where=""):
    got, want = w.get_state(), ref if isinstance(ref, dict) else ref.state()
    for k in STATE_KEYS:
        assert np.array_equal(got[k], want[k]), (where, k)
    assert w.count == len(want["host"])


def _dev(a, np_dtype, view):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype).view(view)).cuda()


class Loop:
    """The device chain of the scenario: deliver_round -> push -> pop(round_end) -> run_ordered."""

    def __init__(self, ctx, sc):
        import torch

        self.ctx, self.sc = ctx, sc
        h = sc["hosts"]
        self.ht = HostTable(h["ip"], h["route"], h["seed"], ctx=ctx)
        self.table = DeviceTable(_dev(sc["lat"].ravel(), np.uint64, np.int64), _dev(sc["loss"].ravel(), np.float32,
                                                                                     np.float32), wc.H)
        self.ib = InboundPipeline(sc["bw"], wc.RING_CAP, ctx=ctx)
        self.fwd = torch.full((sc["n_pk"],), -1, dtype=torch.int64, device="cuda")
        self.st = torch.zeros(sc["n_pk"], dtype=torch.uint8, device="cuda")
        self.ctr_ptr = _capi.load().sg_hosts_event_ctr(self.ht.handle)

    def round(self, w, k):
        """Round k on the device, compared with the reference's round k."""
        import torch

        r = self.sc["rounds"][k]
        if r["pk"] is not None:
            pk = r["pk"]
            batch = PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"])
            out = deliver_round(self.ht, self.table, batch, r["end"], wc.SIM_END, 0, ctx=self.ctx)
            assert out.n_delivered == r["want"]["delivered"]
            w.push(batch, out, _dev(pk["len"], np.uint32, np.int32), id_base=r["id_base"])
        got = w.pop(r["end"])
        _same_pop(got, r["pop"], r["next"], f"round {k}")
        n = got["n"]
        a_st = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        a_fwd = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
        self.ib.run_ordered(got["host"], got["time_ns"], got["packet"], got["len"], r["end"], 0, wc.SIM_END, self.fwd,
                            self.st, a_fwd, a_st, self.ctr_ptr)
        if n:  # this call's arrivals report in arrival order: scatter them to their packet ids
            p = got["packet"].long()
            left = a_st[:n] != 0
            self.st[p[left]] = a_st[:n][left]
            done = left & (a_st[:n] == 1)
            self.fwd[p[done]] = a_fwd[:n][done]
        st = self.st.cpu().numpy()
        assert np.array_equal(st, r["st"]), f"round {k}: inbound fates"
        assert np.array_equal(self.fwd.cpu().numpy().view(np.uint64)[st == 1], r["fwd"][st == 1]), f"round {k}: fwd"
        assert np.array_equal(self.ht.get_state()[1], r["ctr"]), f"round {k}: event_ctr"

    def inbound_matches(self, oracle):
        got, want = self.ib.get_state(), self.sc["inbound"]
        for k in ("flags", "interval_end", "drop_next", "cur", "prev", "bytes", "head", "tail", "rflags", "task_time",
                  "tb_cap", "tb_bal", "tb_inc", "tb_last", "task_id", "task_born"):
            assert np.array_equal(got[k], want[k]), k


def _wire(ctx, bin_ns=MS, n_bins=16, capacity=wc.SEND_ROUNDS * wc.PER_ROUND):
    return PacketWire(wc.H, capacity, bin_ns, n_bins, ctx=ctx)


def test_closed_loop_matches_oracle_chain(oracle, ctx):
    """12 rounds of ~2,000 packets over 64 hosts, then quiet rounds until the 40 ms class has
    arrived; a 16 x 1 ms ring, so the 19 and 40 ms classes go through the far list."""
    sc = wc.scenario(oracle)
    loop, w = Loop(ctx, sc), _wire(ctx)
    for k in range(wc.ROUNDS):
        loop.round(w, k)
        if k in (wc.SEND_ROUNDS - 1, wc.ROUNDS - 1):
            _same_state(w, sc["rounds"][k]["held"], f"round {k}")
    assert w.count == 0
    loop.inbound_matches(oracle)
    rng, ctr = loop.ht.get_state()
    assert np.array_equal(rng, sc["rng_end"]) and np.array_equal(ctr, sc["rounds"][-1]["ctr"])


@pytest.mark.parametrize("bin_ns,n_bins", [(MS, 16), (250_000, 4), (10**9, 2)])
def test_geometry_never_shows(oracle, ctx, bin_ns, n_bins):
    """The first six rounds under three calendars: the same pops (each equals the reference's).  The
    inbound stage runs too: its forward tasks take event ids from the counters delivery uses."""
    sc = wc.scenario(oracle)
    loop, w = Loop(ctx, sc), _wire(ctx, bin_ns, n_bins)
    for k in range(6):
        loop.round(w, k)
    _same_state(w, sc["rounds"][5]["held"])


def test_checkpoint_resumes(oracle, ctx):
    """get_state after round 6 -> a fresh wire -> set_state with the events shuffled -> rounds 7-12 as uninterrupted."""
    sc = wc.scenario(oracle)
    loop, w = Loop(ctx, sc), _wire(ctx)
    for k in range(6):
        loop.round(w, k)
    st = w.get_state()
    assert len(st["host"]) == len(sc["rounds"][5]["held"]["host"]) > 0
    perm = np.random.default_rng(3).permutation(len(st["host"]))
    w2 = _wire(ctx, 500_000, 8)
    w2.set_state({k: v[perm] for k, v in st.items()})
    _same_state(w2, sc["rounds"][5]["held"])
    for k in range(6, wc.SEND_ROUNDS):
        loop.round(w2, k)
    _same_state(w2, sc["rounds"][wc.SEND_ROUNDS - 1]["held"])


def _small_net(oracle, ctx, n_hosts, lat):
    from shadow_amd import synth

    hosts = synth.make_hosts(n_hosts, n_hosts)
    lat = np.asarray(lat, np.uint64)
    loss = np.zeros((n_hosts, n_hosts), np.float32)
    ht = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    table = DeviceTable(_dev(lat.ravel(), np.uint64, np.int64), _dev(loss.ravel(), np.float32, np.float32), n_hosts)
    rng = np.stack([oracle.xoshiro_seed(int(s)) for s in hosts["seed"]]).astype(np.uint64)
    return dict(hosts=hosts, lat=lat, loss=loss, ht=ht, table=table, rng=rng, ctr=np.zeros(n_hosts, np.uint64))


def _send(oracle, ctx, net, w, ref, src, dst, t, round_end, id_base, tag=0, expect=None):
    """One round on both sides; returns the oracle's delivery."""
    h = net["hosts"]
    src, t = np.asarray(src, np.uint32), np.asarray(t, np.uint64)
    dst_ip = h["ip"][np.asarray(dst, np.int64)].astype(np.uint32) if len(src) else np.zeros(0, np.uint32)
    pay = np.full(len(src), 1448, np.uint32)
    ln = pay + 28
    want = oracle.deliver_round(round_end, wc.SIM_END, 0, src, dst_ip, pay, t, h["ip"], h["route"], net["lat"],
                                net["loss"], net["rng"], net["ctr"])
    batch = PacketBatch.from_numpy(src, dst_ip, pay, t)
    out = deliver_round(net["ht"], net["table"], batch, round_end, wc.SIM_END, 0, ctx=ctx)
    if expect is None:
        w.push(batch, out, _dev(ln, np.uint32, np.int32), id_base=id_base)
        ref.push(want, src, ln, id_base=id_base, tag=tag)
    else:
        with pytest.raises(ShadowGpuError) as e:
            w.push(batch, out, _dev(ln, np.uint32, np.int32), id_base=id_base)
        assert e.value.code == expect
    return want


def test_ties_and_the_ordering_trap(oracle, ctx):
    lat = np.full((8, 8), 5 * MS, np.uint64)
    lat[1, 0] = 1000     # (a) two sends of host 1 that both clamp to round_end
    lat[5, 0] = 2 * MS   # (b) round 1, source 5: sent at T0 + 0.5 ms, arrives T0 + 2.5 ms
    lat[3, 0] = 1 * MS   #     round 2, source 3: sent at T0 + 1.5 ms, arrives T0 + 2.5 ms
    net = _small_net(oracle, ctx, 8, lat)
    w, ref = PacketWire(8, 64, MS, 4, ctx=ctx), WireRef()
    a = _send(oracle, ctx, net, w, ref, [1, 1, 5], [0, 0, 0], [T0 + 100, T0 + 200, T0 + MS // 2], T0 + MS, 0, tag=1)
    assert a["deliver_time"][0] == a["deliver_time"][1] == T0 + MS and a["event_id"][0] < a["event_id"][1]
    b = _send(oracle, ctx, net, w, ref, [3], [0], [T0 + 3 * MS // 2], T0 + 2 * MS, 10, tag=2)
    assert b["deliver_time"][0] == a["deliver_time"][2] == T0 + 5 * MS // 2
    want, nxt = ref.pop(T0 + 3 * MS)
    # host 0's queue: the two clamped packets by event id, then source 3 (pushed later) before source 5
    assert want["packet"].tolist() == [0, 1, 10, 2] and want["tag"].tolist() == [1, 1, 2, 1]
    _same_pop(w.pop(T0 + 3 * MS), want, nxt)
    # (c) one host, time and source; event ids 2^40 + 1 and 7 given in that order
    w.set_state(dict(host=[2, 2], src_host=[4, 4], packet=[0, 1], len=[9, 9], time_ns=[T0, T0],
                     event_id=[2**40 + 1, 7]))
    got = w.pop(T0 + 1)
    assert _np(got["event_id"], "event_id").tolist() == [7, 2**40 + 1] and _np(got["packet"], "packet").tolist() == [1, 0]


def _state(rows):
    """rows of (host, time, src, event id, packet)."""
    c = list(zip(*rows))
    return dict(host=np.array(c[0], np.uint32), time_ns=np.array(c[1], np.uint64), src_host=np.array(c[2], np.uint32),
                event_id=np.array(c[3], np.uint64), packet=np.array(c[4], np.uint32), len=np.full(len(rows), 77, np.uint32))


def _both(w, ref, rows):
    st = _state(rows)
    cur = w.get_state()
    w.set_state({k: np.concatenate([cur[k], st[k]]) for k in STATE_KEYS})
    ref.add(**st)


def test_window_edges(oracle, ctx):
    T = T0 + 10 * MS + 400_000  # in the middle of a 1 ms bin
    w, ref = PacketWire(4, 64, MS, 8, ctx=ctx), WireRef()
    _both(w, ref, [(1, T - 1, 0, 0, 0), (1, T, 0, 1, 1), (1, T + 1, 0, 2, 2), (2, T + 300_000, 0, 3, 3),
                   (3, 2**63, 0, 4, 4), (3, 2**64 - 2, 0, 5, 5)])
    for end in (T, T, T + 1, T - 5 * MS, T + 2):  # the same window twice; one behind the last: nothing leaves
        want, nxt = ref.pop(end)
        _same_pop(w.pop(end), want, nxt, end)
    assert w.count == 3
    # events below the last window_end leave on the next pop.  By set_state: that replaces the whole store
    # and starts its calendar afresh, so it shows only that such a state is accepted.  By a push (a round
    # long past), after a pop has advanced the calendar: that one is clamped to the calendar's first bin.
    _both(w, ref, [(0, T - 7 * MS, 1, 9, 9)])
    want, nxt = ref.pop(T + 2)
    assert want["packet"].tolist() == [9]
    _same_pop(w.pop(T + 2), want, nxt)
    net = _small_net(oracle, ctx, 4, np.full((4, 4), MS, np.uint64))
    _send(oracle, ctx, net, w, ref, [2, 3], [0, 1], [T0 + 10, T0 + 20], T0 + MS, 100)
    want, nxt = ref.pop(T + 2)
    assert want["packet"].tolist() == [100, 101] and int(want["time_ns"].max()) < T - 9 * MS
    _same_pop(w.pop(T + 2), want, nxt)
    want, nxt = ref.pop(2**63)  # two pops inside one bin happened above; now the bin's last event
    assert want["packet"].tolist() == [3]
    _same_pop(w.pop(2**63), want, nxt)
    want, nxt = ref.pop(2**63 + 1)
    _same_pop(w.pop(2**63 + 1), want, nxt)
    assert nxt == 2**64 - 2
    want, nxt = ref.pop(NEVER)  # UINT64_MAX drains everything
    assert want["packet"].tolist() == [5] and nxt == NEVER
    _same_pop(w.pop(NEVER), want, nxt)
    assert w.count == 0


@pytest.mark.parametrize("n", [1, 33, wire.RANK_SORT_MAX + 1, wire.LDS_SORT_MAX + 1, 3 * wire.LDS_SORT_MAX + 5])
def test_sort_tiers_hot_destination(ctx, n):
    """All events to one host at one time: the order rests on (src_host, event_id) alone."""
    rng = np.random.default_rng(n)
    T = T0 + 3 * MS
    eid = rng.permutation(4 * n).astype(np.uint64)[:n] + (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(40))
    st = dict(host=np.full(n, 2, np.uint32), time_ns=np.full(n, T, np.uint64),
              src_host=rng.integers(0, 7, n).astype(np.uint32), event_id=eid, packet=np.arange(n, dtype=np.uint32),
              len=rng.integers(28, 1500, n).astype(np.uint32))
    one = _state([(5, T + 1, 3, 1, n)])  # a second host with a single event
    st = {k: np.concatenate([st[k], one[k]]) for k in STATE_KEYS}
    w, ref = PacketWire(8, n + 1, MS, 4, ctx=ctx), WireRef()
    w.set_state(st)
    ref.add(**st)
    want, nxt = ref.pop(T + 2)
    assert len(want["host"]) == n + 1 and nxt == NEVER
    _same_pop(w.pop(T + 2), want, nxt)


def test_capacity(oracle, ctx):
    n = 300
    net = _small_net(oracle, ctx, 16, np.full((16, 16), 3 * MS, np.uint64))  # loss 0: every packet is delivered
    rng = np.random.default_rng(5)
    src = np.sort(rng.integers(0, 16, n)).astype(np.uint32)
    dst = (src + 1 + rng.integers(0, 15, n)) % 16
    t = np.sort(rng.integers(T0, T0 + MS, n)).astype(np.uint64)
    t = t[np.lexsort((t, src))]
    w, ref = PacketWire(16, n, MS, 8, ctx=ctx), WireRef()
    want = _send(oracle, ctx, net, w, ref, src, dst, t, T0 + MS, 0)  # fills the store exactly
    assert want["delivered"] == n and w.count == n
    _send(oracle, ctx, net, w, ref, [0], [1], [T0 + MS + 5], T0 + 2 * MS, n, expect=_capi.SG_ERR_CAPACITY)
    assert w.count == n
    due = int((ref.ev["time_ns"] < T0 + 7 * MS // 2).sum())
    assert 1 < due < n
    with pytest.raises(ShadowGpuError) as e:
        w.pop(T0 + 7 * MS // 2, cap=due - 1)
    assert e.value.code == _capi.SG_ERR_CAPACITY and e.value.needed == due and w.count == n
    _same_state(w, ref)  # neither failure changed the store
    exp, nxt = ref.pop(T0 + 7 * MS // 2)
    _same_pop(w.pop(T0 + 7 * MS // 2, cap=due), exp, nxt)
    exp, nxt = ref.pop(NEVER)
    _same_pop(w.pop(NEVER), exp, nxt)


def test_empty_and_degenerate(oracle, ctx):
    w = PacketWire(4, 8, MS, 4, ctx=ctx)
    got = w.pop(T0)
    assert got["n"] == 0 and got["next_time_ns"] == NEVER
    got = w.pop(NEVER, cap=0)
    assert got["n"] == 0 and got["next_time_ns"] == NEVER
    # a batch with no delivered packet (every destination unknown)
    import torch

    from shadow_amd import ipv4_to_u32

    net = _small_net(oracle, ctx, 4, np.full((4, 4), MS, np.uint64))
    src, t = np.array([0, 1, 2], np.uint32), np.array([T0 + 1, T0 + 2, T0 + 3], np.uint64)
    batch = PacketBatch.from_numpy(src, np.full(3, ipv4_to_u32("10.9.9.9"), np.uint32), np.full(3, 100, np.uint32), t)
    out = deliver_round(net["ht"], net["table"], batch, T0 + MS, wc.SIM_END, 0, ctx=ctx)
    assert out.n_delivered == 0 and bool((out.status[:3] == _capi.SG_PKT_DROP_NO_DST).all())
    w.push(batch, out, torch.full((3,), 128, dtype=torch.int32, device="cuda"))
    got = w.pop(NEVER)
    assert got["n"] == 0 and got["next_time_ns"] == NEVER and w.count == 0
    # the smallest calendar: two bins of one nanosecond
    w, ref = PacketWire(4, 64, 1, 2, ctx=ctx), WireRef()
    net = _small_net(oracle, ctx, 4, np.array([[MS, 3, 7 * MS, 9], [5, MS, 1, 2 * MS], [4 * MS, 8, MS, 6],
                                               [2, 3 * MS, 11, MS]], np.uint64))
    for k in range(4):
        rng = np.random.default_rng(k)
        src = np.sort(rng.integers(0, 4, 12)).astype(np.uint32)
        t = np.sort(rng.integers(T0 + k * MS, T0 + (k + 1) * MS, 12)).astype(np.uint64)
        _send(oracle, ctx, net, w, ref, src, (src + 1 + rng.integers(0, 3, 12)) % 4, t[np.lexsort((t, src))],
              T0 + (k + 1) * MS, 100 * k, tag=k)
        for end in (T0 + (k + 1) * MS, T0 + (k + 1) * MS + 1, T0 + (k + 1) * MS + MS // 2):
            want, nxt = ref.pop(end)
            _same_pop(w.pop(end), want, nxt, (k, end))
    want, nxt = ref.pop(NEVER)
    _same_pop(w.pop(NEVER), want, nxt)


@pytest.mark.parametrize("bin_ns,n_bins", [(10**9, 2), (8 * MS, 2)])
def test_long_bins_do_not_use_up_the_store(oracle, ctx, bin_ns, n_bins):
    """Many rounds through bins far longer than a round, with a capacity just above the peak of events
    held and about ten times that pushed in all: the records popped from the bin that straddles the
    window must not keep their slots (the row is compacted), or the arena runs out.  Every pop and the
    final state equal the reference; the compaction is seen to run."""
    rounds, per = 96, 300
    lat = np.random.default_rng(1).integers(MS, 3 * MS, (16, 16)).astype(np.uint64)
    net = _small_net(oracle, ctx, 16, lat)
    batches, ref, peak = [], WireRef(), 0
    onet = dict(net, rng=net["rng"].copy(), ctr=net["ctr"].copy())  # a dry run of the reference for the peak
    for k in range(rounds):
        rng = np.random.default_rng(1000 + k)
        src = np.sort(rng.integers(0, 16, per)).astype(np.uint32)
        dst = (src + 1 + rng.integers(0, 15, per)) % 16
        t = np.sort(rng.integers(T0 + k * MS, T0 + (k + 1) * MS, per)).astype(np.uint64)
        batches.append((src, dst, t))
        h = net["hosts"]
        want = oracle.deliver_round(T0 + (k + 1) * MS, wc.SIM_END, 0, src, h["ip"][dst].astype(np.uint32),
                                    np.full(per, 1448, np.uint32), t, h["ip"], h["route"], net["lat"], net["loss"],
                                    onet["rng"], onet["ctr"])
        peak = max(peak, len(ref) + per)  # what sg_wire_push checks: the count before it + the batch
        ref.push(want, src, np.full(per, 1476, np.uint32))
        ref.pop(T0 + (k + 1) * MS)
    assert rounds * per >= 8 * peak
    w, ref = PacketWire(16, peak, bin_ns, n_bins, ctx=ctx), WireRef()
    ctx.enable_timers(True)
    for k, (src, dst, t) in enumerate(batches):
        _send(oracle, ctx, net, w, ref, src, dst, t, T0 + (k + 1) * MS, k * per, tag=k)
        want, nxt = ref.pop(T0 + (k + 1) * MS)
        _same_pop(w.pop(T0 + (k + 1) * MS), want, nxt, k)
        assert w.count == len(ref)
    compactions = ctx.read_timer("wire_compact")[1]
    ctx.enable_timers(False)
    assert compactions > 0
    _same_state(w, ref)
    want, nxt = ref.pop(NEVER)
    _same_pop(w.pop(NEVER), want, nxt)
