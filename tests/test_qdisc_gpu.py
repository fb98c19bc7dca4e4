"""GPU parity of the outbound pipeline under the interface's round-robin qdisc
(sg_outbound_create_qdisc / sg_outbound_run_qdisc, sg_qdisc.hip) against tests/qdisc_ref.py,
bit-exact: statuses, forward times, event-counter advances, the sent batch (forward order) and
the canonical interface + relay state, window after window."""
import numpy as np
import pytest

import qdisc_cases as qc
from qdisc_ref import FIFO, ROUND_ROBIN, Interfaces
from shadow_amd import ShadowGpuError, _capi, synth
from shadow_amd.router import OutboundPipeline
from shadow_amd.worker import DeviceTable, HostTable, deliver_round

pytestmark = pytest.mark.gpu
T0, MS = qc.T0, qc.MS
RELAY = ("rflags", "task_time", "task_id", "task_born", "tb_cap", "tb_bal", "tb_inc", "tb_last")
QKEYS = ("n_active", "n_queued", "cached_packet", "cached_len", "cached_payload_len", "cached_dst")
SIM_END = T0 + 10**12


def _dev(a, np_dtype, signed_dtype):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype).view(signed_dtype)).cuda()


def _i32(a):
    return _dev(a, np.uint32, np.int32)


def _i64(a):
    return _dev(a, np.uint64, np.int64)


def _same_state(got, want, S, cap):
    """The canonical state: the written part of every per-host list."""
    for k in QKEYS:
        assert np.array_equal(got[k], want[k]), k
    na, nq = want["n_active"].astype(np.int64), want["n_queued"].astype(np.int64)
    ia = np.repeat(np.arange(len(na)) * S, na) + np.arange(int(na.sum())) - np.repeat(np.cumsum(na) - na, na)
    iq = np.repeat(np.arange(len(nq)) * cap, nq) + np.arange(int(nq.sum())) - np.repeat(np.cumsum(nq) - nq, nq)
    for k in ("active", "active_count"):
        assert np.array_equal(got[k][ia], want[k][ia]), k
    for k in ("q_packet", "q_len", "q_payload_len", "q_dst"):
        assert np.array_equal(got[k][iq], want[k][iq]), k


class Pair:
    """A round-robin pipeline on the device and the reference model beside it."""

    def __init__(self, ctx, host_ip, bw, cap, S, n_pk, ctr0=0):
        import torch

        self.ob = OutboundPipeline(host_ip, bw, cap, ctx=ctx, qdisc="round-robin", max_sockets=S)
        self.ref = Interfaces(host_ip, bw, cap, ROUND_ROBIN, S)
        assert self.ob.cap == self.ref.cap and self.ob.max_sockets == self.ref.S
        H = len(bw)
        self.H = H
        self.fwd_g = torch.full((n_pk,), -1, dtype=torch.int64, device="cuda")
        self.st_g = torch.zeros(n_pk, dtype=torch.uint8, device="cuda")
        self.ctr_g = torch.full((H,), ctr0, dtype=torch.int64, device="cuda")
        self.fwd_r = np.full(n_pk, np.uint64(2**64 - 1))
        self.st_r = np.zeros(n_pk, np.uint8)
        self.ctr_r = np.full(H, ctr0, np.uint64)

    def step(self, host, t, pkt, ln, pay, dst, sock, t1, boot=0, sim_end=SIM_END, eid=None, born=None, state=True):
        keys = {} if eid is None else dict(event_id=_i64(eid), event_created_ns=_i64(born))
        keys["sent_cap"] = len(host) + sum(h.n for h in self.ref.hosts) + self.H  # the sends, the queued, the cached
        batch, ids = self.ob.run(_i32(host), _i64(t), _i32(pkt), _i32(ln), _i32(pay), _i32(dst), t1, boot, sim_end,
                                 self.fwd_g, self.st_g, self.ctr_g.data_ptr(), socket=_i32(sock), **keys)
        want = self.ref.run(host, t, pkt, ln, pay, dst, sock, t1, boot, sim_end, self.ctr_r, self.fwd_r, self.st_r,
                            event_id=eid, event_created=born)
        assert np.array_equal(self.st_g.cpu().numpy(), self.st_r)
        m = self.st_r != 0
        assert np.array_equal(self.fwd_g.cpu().numpy().view(np.uint64)[m], self.fwd_r[m])
        assert np.array_equal(self.ctr_g.cpu().numpy().view(np.uint64), self.ctr_r)
        assert len(batch) == len(want["packet"])
        assert np.array_equal(ids.cpu().numpy().view(np.uint32), want["packet"])
        assert np.array_equal(batch.src_host.cpu().numpy().view(np.uint32), want["src_host"])
        assert np.array_equal(batch.dst_ipv4.cpu().numpy().view(np.uint32), want["dst_ipv4"])
        assert np.array_equal(batch.payload_len.cpu().numpy().view(np.uint32), want["payload_len"])
        assert np.array_equal(batch.send_time_ns.cpu().numpy().view(np.uint64), want["send_time"])
        if state:
            self.same_state()
        return want

    def same_state(self):
        got, rs = self.ob.get_qdisc_state(), self.ref.relay_state()
        for k in RELAY:
            assert np.array_equal(got[k], rs[k]), k
        _same_state(got, self.ref.qdisc_state(), self.ref.S, self.ref.cap)


def _bw(H, bw_mbit, seed):
    return np.random.default_rng(seed).integers(bw_mbit * 10**6 // 2, bw_mbit * 10**6 + 1, H).astype(np.uint64)


@pytest.mark.parametrize("layout", ["", "1"])
@pytest.mark.parametrize("S", [4, 64])
@pytest.mark.parametrize("bw_mbit", [1000, 50, 10])
def test_windows_match_reference(ctx, monkeypatch, bw_mbit, S, layout):
    """130 hosts (two full blocks and a two-host tail), five windows of 2 ms, 3000 sends each over
    S sockets per host: 4 sockets keep the socket state in LDS, 64 in global memory.  At 50 and
    10 Mbit the reference's own forward order must differ from the fifo order of the same sends
    on at least half the hosts, or the test would pass on fifo behaviour."""
    if layout:
        monkeypatch.setenv("SG_LANE_MAJOR", layout)
    H, W, per = 130, 2 * MS, 3000
    hosts = synth.make_hosts(H, 64, exact_seeds=False)
    bw = _bw(H, bw_mbit, bw_mbit)
    p = Pair(ctx, hosts["ip"], bw, 1024, S, 5 * per)
    fifo = Interfaces(hosts["ip"], bw, 1024, FIFO)
    f_ctr, f_fwd, f_st = np.zeros(H, np.uint64), np.zeros(5 * per, np.uint64), np.zeros(5 * per, np.uint8)
    rr_all, fifo_all = [], []
    for w in range(5):
        t0, t1 = T0 + w * W, T0 + (w + 1) * W
        host, t, ln, pay, dst, sock = qc.sends(hosts, per, t0, t1, 100 * bw_mbit + w, S)
        pkt = np.arange(w * per, (w + 1) * per, dtype=np.uint32)
        rr_all.append(p.step(host, t, pkt, ln, pay, dst, sock, t1))
        fifo_all.append(fifo.run(host, t, pkt, ln, pay, dst, None, t1, 0, SIM_END, f_ctr, f_fwd, f_st))
    cat = lambda b: {k: np.concatenate([x[k] for x in b]) for k in ("src_host", "packet")}
    differ = qc.hosts_reordered(H, cat(rr_all), cat(fifo_all))
    if bw_mbit != 1000:
        assert differ >= H // 2, differ
        assert (p.st_r == 0).any() and (p.ref.relay_state()["rflags"] & 4).any()
    assert (p.st_r == 2).any()


@pytest.mark.parametrize("layout", ["", "1"])
@pytest.mark.parametrize("bw_mbit", [1000, 50])
def test_long_host_across_chunks(ctx, monkeypatch, bw_mbit, layout):
    """Host 70 sends 2500 packets in one window over 8 sockets -- more than any staged chunk, so its
    deque and sockets carry over chunk boundaries -- beside hosts with a few sends or none; then
    two windows of 800 (1000 Mbit) that do not fit behind its pool's bump pointer, so it compacts
    in the kernel (no state is read between the windows: reading it compacts too)."""
    if layout:
        monkeypatch.setenv("SG_LANE_MAJOR", layout)
    H, W, S, big = 130, 2 * MS, 8, 70
    hosts = synth.make_hosts(H, 64, exact_seeds=False)
    bw = _bw(H, bw_mbit, 3)
    counts = [2500, 800, 800] if bw_mbit == 1000 else [2500, 40, 0]
    p = Pair(ctx, hosts["ip"], bw, 4096, S, sum(counts) + 3 * 400)
    rng = np.random.default_rng(11)
    p0 = 0
    for w, n_big in enumerate(counts):
        t0, t1 = T0 + w * W, T0 + (w + 1) * W
        host, t, ln, pay, dst, sock = qc.sends(hosts, 400, t0, t1, 40 + w, S)
        keep = (host % 3 != 0) & (host != big)  # a third of the hosts send nothing
        host, t, ln, pay, dst, sock = (a[keep] for a in (host, t, ln, pay, dst, sock))
        host = np.r_[host, np.full(n_big, big, np.uint32)].astype(np.uint32)
        t = np.r_[t, np.sort(rng.integers(t0, t1, n_big)).astype(np.uint64)]
        ln = np.r_[ln, rng.integers(40, 1500, n_big).astype(np.uint32)]
        pay = np.r_[pay, np.full(n_big, 100, np.uint32)]
        dst = np.r_[dst, np.full(n_big, hosts["ip"][5], np.uint32)]
        sock = np.r_[sock, rng.integers(0, S, n_big).astype(np.uint32)]
        o = np.lexsort((t, host))
        host, t, ln, pay, dst, sock = (a[o] for a in (host, t, ln, pay, dst, sock))
        pkt = np.arange(p0, p0 + len(host), dtype=np.uint32)
        p0 += len(host)
        p.step(host, t, pkt, ln, pay, dst, sock, t1, state=False)
    p.same_state()
    assert p.ref.hosts[big].n > 1000 and len(p.ref.hosts[big].dq) == S


@pytest.mark.parametrize("bw_mbit,S,layout", [(10, 4, ""), (2, 4, "1"), (2, 64, "")])
def test_same_time_ties_match_reference(ctx, monkeypatch, bw_mbit, S, layout):
    """Wake-ups and sends on the same nanosecond, ordered by the sending event's (created, id)
    against the task's: keyed sends (k_qdisc<true>), four windows, task ids included.  The keys
    must matter: the model with every Local send created first, and with every one created
    last, disagrees."""
    if layout:
        monkeypatch.setenv("SG_LANE_MAJOR", layout)
    H, W, per = 130, 2 * MS, 3000
    hosts = synth.make_hosts(H, 64, exact_seeds=False)
    bw = np.full(H, bw_mbit * 10**6, np.uint64)
    p = Pair(ctx, hosts["ip"], bw, 1024, S, 4 * per)
    alt = {k: Interfaces(hosts["ip"], bw, 1024, ROUND_ROBIN, S) for k in ("early", "late")}
    ctr_alt = {k: np.zeros(H, np.uint64) for k in alt}
    for w in range(4):
        t0, t1 = T0 + w * W, T0 + (w + 1) * W
        host, t, ln, pay, dst, sock, eid, born = qc.keyed_sends(hosts, per, t0, t1, 50 * bw_mbit + w, S)
        pkt = np.arange(w * per, (w + 1) * per, dtype=np.uint32)
        p.step(host, t, pkt, ln, pay, dst, sock, t1, eid=eid, born=born)
        for k, shift in (("early", -10**12), ("late", 10**12)):
            b2 = np.where(eid == np.uint64(2**64 - 1), born, (born.astype(np.int64) + shift).astype(np.uint64))
            alt[k].run(host, t, pkt, ln, pay, dst, sock, t1, 0, SIM_END, ctr_alt[k], np.zeros(4 * per, np.uint64),
                       np.zeros(4 * per, np.uint8), event_id=eid, event_created=b2)
    for k in alt:
        assert not np.array_equal(ctr_alt[k], p.ctr_r), k


@pytest.mark.parametrize("S", [4, 64])
def test_locals_bootstrap_and_an_empty_window(ctx, S):
    """15 % local sends (SG_OUT_LOCAL, no tokens), a bootstrap end inside the second window, and a
    third window with no sends at all: pending tasks only."""
    H, W, per = 130, 2 * MS, 3000
    hosts = synth.make_hosts(H, 64, exact_seeds=False)
    p = Pair(ctx, hosts["ip"], _bw(H, 10, 9), 1024, S, 3 * per)
    boot, p0 = T0 + 3 * MS, 0
    for w in range(4):
        t0, t1 = T0 + w * W, T0 + (w + 1) * W
        n = 0 if w == 2 else per
        host, t, ln, pay, dst, sock = qc.sends(hosts, n, t0, t1, 300 + w, S, p_local=0.15)
        pkt = np.arange(p0, p0 + n, dtype=np.uint32)
        p0 += n
        before = (p.st_r != 0).sum()
        p.step(host, t, pkt, ln, pay, dst, sock, t1, boot=boot)
        if w == 2:
            assert (p.st_r != 0).sum() > before  # the empty window forwarded queued packets
    assert (p.st_r == 2).any() and (p.st_r == 1).any() and (p.st_r == 0).any()


@pytest.mark.parametrize("S", [4, 16, 64])
def test_full_deque_rotates(ctx, S):
    """Every socket slot of every host active behind a throttled relay: the deque is full and a
    pop's re-push lands on the entry the front just left.  16 sockets is the most the kernel keeps
    in LDS."""
    H, W = 70, 2 * MS
    hosts = synth.make_hosts(H, 64, exact_seeds=False)
    p = Pair(ctx, hosts["ip"], np.full(H, 10 * 10**6, np.uint64), 512, S, 2 * H * S * 3)
    rng = np.random.default_rng(S)
    p0 = 0
    for w in range(2):  # every socket in turn, three times over; then sockets at random
        n = H * S * 3
        host = np.repeat(np.arange(H, dtype=np.uint32), S * 3)
        sock = np.tile(np.arange(S, dtype=np.uint32), 3 * H) if w == 0 else rng.integers(0, S, n).astype(np.uint32)
        t = (T0 + w * W + np.tile(np.arange(S * 3), H) * 1000 + 5).astype(np.uint64)
        ln = rng.integers(200, 1500, n).astype(np.uint32)
        pay = (ln - 40).astype(np.uint32)
        dst = hosts["ip"][(host + 1) % H].astype(np.uint32)
        pkt = np.arange(p0, p0 + n, dtype=np.uint32)
        p0 += n
        p.step(host, t, pkt, ln, pay, dst, sock, T0 + (w + 1) * W)
        full = (p.ref.qdisc_state()["n_active"] == S).sum()
        assert full == H if w == 0 else full >= H // 2
    sent = (p.st_r == 1).sum()
    e = np.zeros(0, np.uint32)
    p.step(e, np.zeros(0, np.uint64), e, e, e, e, e, T0 + 50 * MS)  # 46 ms of wake-ups turn the full deques over
    assert (p.st_r == 1).sum() - sent > H * min(S, 32)


@pytest.mark.parametrize("name", sorted(qc.HAND_CASES))
def test_hand_worked_orders(ctx, name):
    """The orders worked by hand from the reference's rules (tests/qdisc_cases.py)."""
    case = qc.HAND_CASES[name]
    host, t, pkt, ln, pay, dst, sock, eid, born = qc.hand_arrays(case)
    p = Pair(ctx, [10], [8 * 10**6], 16, 4, len(pkt), ctr0=case.get("ctr0", 0))
    want = p.step(host, t, pkt, ln, pay, dst, sock, case["end"], eid=eid, born=born)
    assert list(want["packet"]) == case["order"]


def _one_host(ctx, cap=16, S=2, qdisc="round-robin", bw=10**9):
    import torch

    ob = OutboundPipeline(np.array([10, 11], np.uint32), np.array([bw, bw], np.uint64), cap, ctx=ctx, qdisc=qdisc,
                          max_sockets=S)
    return ob, torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda")


def test_errors(ctx):
    lib = _capi.load()
    args = [_i32([0, 0, 1]), _i64([T0 + 1, T0 + 2, T0 + 1]), _i32([0, 1, 2]), _i32([100] * 3), _i32([60] * 3),
            _i32([11, 11, 10])]
    ob, f, s = _one_host(ctx)
    with pytest.raises(ShadowGpuError) as e:  # a socket at max_sockets
        ob.run(*args, T0 + MS, 0, SIM_END, f, s, socket=_i32([0, 2, 1]))
    assert e.value.code == _capi.SG_ERR_INVALID_ARG and "socket" in str(e.value)
    ob, f, s = _one_host(ctx)
    with pytest.raises(ShadowGpuError) as e:  # no sockets at all
        ob.run(*args, T0 + MS, 0, SIM_END, f, s)
    assert e.value.code == _capi.SG_ERR_INVALID_ARG and "socket" in str(e.value)
    sends = _capi.sg_outbound_sends(3, *(a.data_ptr() for a in args), None, None)
    import ctypes as C

    rc = lib.sg_outbound_run(ctx.handle, ob.handle, C.byref(sends), T0 + MS, 0, SIM_END, None, f.data_ptr(),
                             s.data_ptr(), 8, None, None)  # the fifo entry point on a round-robin object
    assert rc == _capi.SG_ERR_INVALID_ARG
    with pytest.raises(ShadowGpuError) as e:  # ... and its queue state
        ob.get_state()
    assert e.value.code == _capi.SG_ERR_INVALID_ARG
    ob, f, s = _one_host(ctx)
    with pytest.raises(ShadowGpuError) as e:  # sent->cap too small
        ob.run(*args, T0 + MS, 0, SIM_END, f, s, socket=_i32([0, 1, 1]), sent_cap=2)
    assert e.value.code == _capi.SG_ERR_CAPACITY
    ob, f, s = _one_host(ctx, cap=2, bw=8000)  # 1 B per ms: the second packet blocks, the queue fills
    a3 = [_i32([0, 0, 0, 0]), _i64([T0 + 1] * 4), _i32([0, 1, 2, 3]), _i32([1500] * 4), _i32([60] * 4), _i32([11] * 4)]
    with pytest.raises(ShadowGpuError) as e:
        ob.run(*a3, T0 + MS, 0, SIM_END, f, s, socket=_i32([0, 1, 0, 1]))
    assert e.value.code == _capi.SG_ERR_CAPACITY
    ob, f, s = _one_host(ctx)
    with pytest.raises(ShadowGpuError) as e:  # sends out of time order
        ob.run(args[0], _i64([T0 + 2, T0 + 1, T0 + 1]), *args[2:], T0 + MS, 0, SIM_END, f, s, socket=_i32([0, 1, 1]))
    assert e.value.code == _capi.SG_ERR_UNSORTED
    for bad in (0, _capi.SG_QDISC_MAX_SOCKETS + 1):
        with pytest.raises(ShadowGpuError) as e:
            _one_host(ctx, S=bad)
        assert e.value.code == _capi.SG_ERR_INVALID_ARG
    ob, _, _ = _one_host(ctx, S=5)
    assert ob.max_sockets == 8 and lib.sg_outbound_qdisc(ob.handle) == _capi.SG_QDISC_ROUND_ROBIN
    fo, _, _ = _one_host(ctx, qdisc="fifo", S=1)
    assert fo.max_sockets == 1 and lib.sg_outbound_qdisc(fo.handle) == _capi.SG_QDISC_FIFO
    with pytest.raises(ShadowGpuError) as e:  # a fifo object has no qdisc state
        fo.get_qdisc_state()
    assert e.value.code == _capi.SG_ERR_INVALID_ARG


def test_fifo_object_through_the_new_entry_point(ctx):
    """sg_outbound_run_qdisc on a fifo object ignores the sockets (given or NULL) and is
    sg_outbound_run: the same outputs and state over three throttled windows."""
    import ctypes as C

    import torch

    H, W, per = 130, 2 * MS, 3000
    hosts = synth.make_hosts(H, 64, exact_seeds=False)
    bw = _bw(H, 10, 5)
    obs = [OutboundPipeline(hosts["ip"], bw, 512, ctx=ctx) for _ in range(3)]
    out = [(torch.full((3 * per,), -1, dtype=torch.int64, device="cuda"),
            torch.zeros(3 * per, dtype=torch.uint8, device="cuda"), torch.zeros(H, dtype=torch.int64, device="cuda"))
           for _ in range(3)]
    for w in range(3):
        t0, t1 = T0 + w * W, T0 + (w + 1) * W
        host, t, ln, pay, dst, sock = qc.sends(hosts, per, t0, t1, 700 + w, 4)
        pkt = np.arange(w * per, (w + 1) * per, dtype=np.uint32)
        args = (_i32(host), _i64(t), _i32(pkt), _i32(ln), _i32(pay), _i32(dst), t1, 0, SIM_END)
        b0, i0 = obs[0].run(*args, out[0][0], out[0][1], out[0][2].data_ptr())
        want = [x.cpu().numpy().copy() for x in (i0, b0.src_host, b0.dst_ipv4, b0.payload_len, b0.send_time_ns)]
        b1, i1 = obs[1].run(*args, out[1][0], out[1][1], out[1][2].data_ptr(), socket=_i32(sock))
        got = [x.cpu().numpy().copy() for x in (i1, b1.src_host, b1.dst_ipv4, b1.payload_len, b1.send_time_ns)]
        for a, b in zip(want, got):
            assert np.array_equal(a, b)
        # socket = NULL, straight through the C entry point
        s = _capi.sg_outbound_sends(per, *(a.data_ptr() for a in args[:6]), None, None)
        ns = C.c_uint32()
        rc = _capi.load().sg_outbound_run_qdisc(ctx.handle, obs[2].handle, C.byref(s), None, t1, 0, SIM_END,
                                                C.c_void_p(out[2][2].data_ptr()), out[2][0].data_ptr(),
                                                out[2][1].data_ptr(), 3 * per, None, C.byref(ns))
        assert rc == _capi.SG_OK and ns.value == len(i0)
        for k in (1, 2):
            for a, b in zip(out[0], out[k]):
                assert torch.equal(a, b)
            sa, sb = obs[0].get_state(), obs[k].get_state()
            for key in ("head", "tail") + RELAY:
                assert np.array_equal(sa[key], sb[key]), key


def test_sent_batch_feeds_delivery(oracle, ctx):
    """A round-robin window -> sg_deliver_round on its sent batch, against the oracle's delivery of
    the reference model's batch."""
    import torch

    from test_deliver_gpu import _world

    lat, loss, hosts = _world(n_hosts=300, seed=4)
    H, S = hosts["n"], 4
    bw = np.full(H, 20 * 10**6, np.uint64)
    start, end = T0 + 10**9, T0 + 10**9 + 3 * MS  # two refills inside the window: queued packets leave reordered
    host, t, ln, pay, dst, sock = qc.sends(hosts, 6000, start, end, 7, S)
    pkt = np.arange(len(host), dtype=np.uint32)
    ob = OutboundPipeline(hosts["ip"], bw, 256, ctx=ctx, qdisc="round-robin", max_sockets=S)
    ref = Interfaces(hosts["ip"], bw, 256, ROUND_ROBIN, S)
    fifo = Interfaces(hosts["ip"], bw, 256, FIFO)
    fwd_g = torch.zeros(len(pkt), dtype=torch.int64, device="cuda")
    st_g = torch.zeros(len(pkt), dtype=torch.uint8, device="cuda")
    ht = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    rng0, ctr0 = ht.get_state()
    ctr_o = ctr0.copy()
    batch, ids = ob.run(_i32(host), _i64(t), _i32(pkt), _i32(ln), _i32(pay), _i32(dst), end, 0, end + 10**9, fwd_g,
                        st_g, _capi.load().sg_hosts_event_ctr(ht.handle), socket=_i32(sock))
    z = lambda: (np.zeros(len(pkt), np.uint64), np.zeros(len(pkt), np.uint8))
    sent = ref.run(host, t, pkt, ln, pay, dst, sock, end, 0, end + 10**9, ctr_o, *z())
    other = fifo.run(host, t, pkt, ln, pay, dst, None, end, 0, end + 10**9, ctr0.copy(), *z())
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), sent["packet"])
    assert qc.hosts_reordered(H, sent, other) > H // 10  # not the fifo order
    lat_t = torch.from_numpy(np.ascontiguousarray(lat).view(np.int64).ravel()).cuda()
    table = DeviceTable(lat_t, torch.from_numpy(np.ascontiguousarray(loss).ravel()).cuda(), lat.shape[1])
    assert table.pack()
    out = deliver_round(ht, table, batch, end, end + 10**9, 0)
    got = out.to_numpy(len(batch))
    want = oracle.deliver_round(end, end + 10**9, 0, sent["src_host"], sent["dst_ipv4"], sent["payload_len"],
                                sent["send_time"], hosts["ip"], hosts["route"], lat, loss, rng0, ctr_o)
    for k in ("status", "deliver_time", "event_id", "dst_offsets", "dst_order"):
        assert np.array_equal(got[k], want[k]), k
    grng, gctr = ht.get_state()
    assert np.array_equal(grng, rng0) and np.array_equal(gctr, ctr_o)
    assert want["delivered"] > 0 and len(batch) < len(pkt)
