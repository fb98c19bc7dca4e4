"""GPU parity of the wire on the sharded path, bit-exact: sg_deliver_source[_padded] ->
sg_wire_stamp_records[_padded] -> exchange -> sg_wire_push_records[_padded] -> sg_wire_pop ->
sg_inbound_run_ordered on every owner rank, against the oracle chain of tests/wire_cases.py
restricted to the hosts that rank owns (tests/wire_sharded_cases.py).

W ranks are emulated in one process on one context; the exchange is a concatenation of each
sender's segment (tests/test_dist_gpu.py::_run does the same; the collectives move stamped records
as they move records: same 32 bytes).  tests/test_wire_sharded_cpu.py asserts that the scenario
has every rank receive from every rank, that pops mix three rounds, and that the padded block size
used here makes some rounds overflow and some fit."""
import numpy as np
import pytest

import wire_cases as wc
import wire_sharded_cases as ws
from shadow_amd import ShadowGpuError, _capi
from shadow_amd.dist import (RECORD_DTYPE, WIRE_RECORD_DTYPE, ShardedDelivery, gpu_pad_to_compact,
                             gpu_source_phase_padded, row_range)
from shadow_amd.router import InboundPipeline
from shadow_amd.wire import PacketWire, stamp_records, stamp_records_padded
from shadow_amd.worker import DeviceTable, HostTable, PacketBatch, deliver_round
from wire_ref import NEVER, WireRef

pytestmark = pytest.mark.gpu
T0, MS = wc.T0, wc.MS
POP_KEYS = ws.POP_KEYS
STATE_KEYS = ("host", "src_host", "packet", "len", "time_ns", "event_id")
UNSIGNED = dict(host=np.uint32, packet=np.uint32, len=np.uint32, src_host=np.uint32, time_ns=np.uint64,
                event_id=np.uint64)
CAPACITY = 2 * wc.SEND_ROUNDS * wc.PER_ROUND


def _np(t, key):
    return t.cpu().numpy().view(UNSIGNED[key])


def _same_pop(got, want, nxt, where=""):
    assert got["n"] == len(want["host"]), (where, got["n"], len(want["host"]))
    assert got["next_time_ns"] == nxt, (where, got["next_time_ns"], nxt)
    for k in POP_KEYS:
        assert np.array_equal(_np(got[k], k), want[k]), (where, k)


def _dev(a, np_dtype, view):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype).view(view)).cuda()


def _records(a):
    """A numpy array of 32-byte records as the [n, 4] int64 device tensor the library's phases use."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 4).copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype).ravel()


class Rank:
    """One emulated rank: its hosts table (streams and counters of the hosts it owns), its shard of
    the routing rows, its wire and, with inbound=True, its inbound queues."""

    def __init__(self, ctx, sc, part, r, W, local=False, inbound=True):
        import torch

        h = sc["hosts"]
        self.ctx, self.sc, self.part, self.r, self.W = ctx, sc, part, r, W
        self.ht = HostTable(h["ip"], h["route"], h["seed"], ctx=ctx)
        r0, r1, _ = row_range(wc.H, W, r)
        self.table = DeviceTable(_dev(sc["lat"][r0:r1].ravel(), np.uint64, np.int64),
                                 _dev(sc["loss"][r0:r1].ravel(), np.float32, np.float32), wc.H, r0)
        self.sd = ShardedDelivery(ctx, self.ht, self.table, part, r, W)
        self.local = local
        self.host_map = self.sd.local_dev if local else None
        self.wire = PacketWire(part.n_local(r) if local else wc.H, CAPACITY, MS, 16, ctx=ctx)
        self.mine = part.hosts_of[r]
        if inbound:
            self.ib = InboundPipeline(sc["bw"], wc.RING_CAP, ctx=ctx)
            self.fwd = torch.full((sc["n_pk"],), -1, dtype=torch.int64, device="cuda")
            self.st = torch.zeros(sc["n_pk"], dtype=torch.uint8, device="cuda")
            self.ctr_ptr = _capi.load().sg_hosts_event_ctr(self.ht.handle)
            self.to_me = part.owner[np.maximum(ws.dst_of_packet(sc), 0)] == r
            self.to_me &= ws.dst_of_packet(sc) >= 0

    def batch(self, k):
        """This rank's packets of round k: those its hosts sent (a run of the source-grouped batch)."""
        rd = self.sc["rounds"][k]
        pk = rd["pk"]
        sel = np.nonzero(self.part.owner[pk["src"]] == self.r)[0]
        assert len(sel) and (np.diff(sel) == 1).all()
        b = PacketBatch.from_numpy(pk["src"][sel], pk["dst_ip"][sel], pk["payload"][sel], pk["send_time"][sel])
        return sel, b, _dev(pk["len"][sel], np.uint32, np.int32), _dev(rd["id_base"] + sel, np.uint32, np.int32)

    def source(self, k):
        """sg_deliver_source + the stamp (packet id = the scenario's id, len = the packet's)."""
        rd = self.sc["rounds"][k]
        sel, b, length, ids = self.batch(k)
        src = self.sd.source_fn(self.ctx, self.ht, self.table, b, rd["end"], wc.SIM_END, 0, self.sd.owner_dev, self.W)
        assert np.array_equal(src.status[:len(sel)].cpu().numpy(), rd["want"]["status"][sel])
        stamp_records(src.send, sum(src.send_counts), length, len(sel), packet_id=ids, ctx=self.ctx)
        return src

    def pop(self, k):
        got = self.wire.pop(self.sc["rounds"][k]["end"])
        want, nxt = ws.rank_pop(self.sc, self.part, self.r, k, slots=self.local)
        _same_pop(got, want, nxt, f"rank {self.r} round {k}")
        return got

    def inbound(self, k, got):
        import torch

        rd, n = self.sc["rounds"][k], got["n"]
        a_st = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        a_fwd = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
        self.ib.run_ordered(got["host"], got["time_ns"], got["packet"], got["len"], rd["end"], 0, wc.SIM_END, self.fwd,
                            self.st, a_fwd, a_st, self.ctr_ptr)
        if n:
            p = got["packet"].long()
            left = a_st[:n] != 0
            self.st[p[left]] = a_st[:n][left]
            done = left & (a_st[:n] == 1)
            self.fwd[p[done]] = a_fwd[:n][done]
        where = f"rank {self.r} round {k}"
        st = self.st.cpu().numpy()
        # the fate of every packet that arrives at a host of this rank; no other packet shows up here
        assert np.array_equal(st, np.where(self.to_me, rd["st"], 0)), where
        ok = st == 1
        assert np.array_equal(self.fwd.cpu().numpy().view(np.uint64)[ok], rd["fwd"][ok]), where
        assert np.array_equal(self.ht.get_state()[1][self.mine], rd["ctr"][self.mine]), where


def _exchange(sends, d):
    """What rank d receives in the exact exchange: segment d of every sender, in sender order."""
    import torch

    parts = []
    for src in sends:
        off = int(sum(src.send_counts[:d]))
        parts.append(src.send[off:off + src.send_counts[d]])
    return torch.cat(parts).contiguous()


def _exact_round(ranks, k):
    sends = [R.source(k) for R in ranks]
    for d, R in enumerate(ranks):
        recv = _exchange(sends, d)
        R.wire.push_records(recv, recv.shape[0], R.host_map)


@pytest.mark.parametrize("W", [1, 2, 3])
def test_closed_loop_exact_exchange(oracle, ctx, W):
    sc = wc.scenario(oracle)
    part = ws.partition(sc, W)
    ranks = [Rank(ctx, sc, part, r, W) for r in range(W)]
    for k in range(wc.ROUNDS):
        if k < wc.SEND_ROUNDS:
            _exact_round(ranks, k)
        for R in ranks:
            R.inbound(k, R.pop(k))
    for R in ranks:
        assert len(R.wire.get_state()["host"]) == 0 and R.wire.count == 0


def test_local_slots(oracle, ctx):
    """Wires over each rank's own hosts (22, 22 and 20), host_map = the partition's local slots.
    Pops only: the inbound stage does not run, so the event ids its forward tasks would have taken
    are given to the hosts' counters from the scenario after every round."""
    sc = wc.scenario(oracle)
    part = ws.partition(sc, 3)
    ranks = [Rank(ctx, sc, part, r, 3, local=True, inbound=False) for r in range(3)]
    assert [R.wire.n for R in ranks] == [22, 22, 20]
    for k in range(wc.ROUNDS):
        if k < wc.SEND_ROUNDS:
            _exact_round(ranks, k)
        for R in ranks:
            R.pop(k)
            R.ht.set_state(ctr=sc["rounds"][k]["ctr"])
    assert all(R.wire.count == 0 for R in ranks)


def test_sharded_delivery_round_with_a_wire(oracle, ctx):
    """ShardedDelivery.round(wire=...) on one rank without a process group, through its three modes:
    round 0 exact, then padded, and -- with the block size forced below the round's count -- a padded
    round that overflows into the exact exchange.  Pops, fates and counters as in the closed loop."""
    sc = wc.scenario(oracle)
    R = Rank(ctx, sc, ws.partition(sc, 1), 0, 1)
    sd = ShardedDelivery(ctx, R.ht, R.table, R.part, 0, 1, padded=True,
                         exchange_fn=lambda send, counts: (send[:counts[0]], list(counts)))
    modes = []
    for k in range(wc.ROUNDS):
        rd = sc["rounds"][k]
        if k < wc.SEND_ROUNDS:
            sel, b, length, ids = R.batch(k)
            if k in (3, 7):
                sd.cap = 256  # far below the ~1,900 records of a round
            if k % 2:
                res, recv_counts, stats = sd.round(b, rd["end"], wc.SIM_END, 0, wire=R.wire, length=length,
                                                   packet_id=ids)
            else:
                res, recv_counts, stats = sd.round(b, rd["end"], wc.SIM_END, 0, wire=R.wire, length=length,
                                                   id_base=rd["id_base"])
            modes.append(sd.last_mode)
            want = rd["want"]
            assert recv_counts == [want["delivered"]] and stats == (want["delivered"], want["min_deliver"],
                                                                    want["min_lat"])
            assert np.array_equal(res.status[:len(sel)].cpu().numpy(), want["status"])
        R.inbound(k, R.pop(k))
    assert modes[0] == "exact" and modes[3] == modes[7] == "padded+exact" and modes.count("padded") == 9
    assert R.wire.count == 0


def test_padded_round_reports_an_unsorted_batch_at_the_pop(oracle, ctx):
    """sg_deliver_source_padded reads nothing back, and with a wire no sg_deliver_bucket_padded
    follows it: a batch that is not grouped by source host is reported by the round's
    synchronising call, the pop, once; nothing of it was delivered and the hosts are untouched."""
    sc = wc.scenario(oracle)
    R = Rank(ctx, sc, ws.partition(sc, 1), 0, 1, inbound=False)
    sd = ShardedDelivery(ctx, R.ht, R.table, R.part, 0, 1, padded=True,
                         exchange_fn=lambda send, counts: (send[:counts[0]], list(counts)))
    rd = sc["rounds"][0]
    sel, b, length, ids = R.batch(0)
    sd.round(b, rd["end"], wc.SIM_END, 0, wire=R.wire, length=length, packet_id=ids)  # exact: sizes the blocks
    assert sd.cap is not None
    R.pop(0)
    held = R.wire.get_state()
    rng0, ctr0 = R.ht.get_state()
    pk = sc["rounds"][1]["pk"]
    assert (np.diff(pk["src"][::-1].astype(np.int64)) < 0).any()
    bad = PacketBatch.from_numpy(pk["src"][::-1].copy(), pk["dst_ip"][::-1].copy(), pk["payload"][::-1].copy(),
                                 pk["send_time"][::-1].copy())
    res, recv_counts, stats = sd.round(bad, sc["rounds"][1]["end"], wc.SIM_END, 0, wire=R.wire,
                                       length=_dev(pk["len"][::-1].copy(), np.uint32, np.int32), id_base=5000)
    assert sd.last_mode == "padded" and recv_counts == [0] and stats[0] == 0  # no call has failed yet
    end1 = sc["rounds"][1]["end"]
    with pytest.raises(ShadowGpuError) as e:
        R.wire.pop(end1)
    assert e.value.code == _capi.SG_ERR_UNSORTED
    # the pop itself was complete: round 0's events due before end1 (the scenario's pop of round 1
    # holds exactly those: what round 1 delivers arrives at or after end1)
    got, want = e.value.arrivals, ws.rank_pop(sc, R.part, 0, 1)[0]
    assert got["n"] == len(want["host"]) > 0
    for key in POP_KEYS:
        assert np.array_equal(_np(got[key], key), want[key]), key
    again = R.wire.pop(end1)  # reported once; the rejected round left nothing behind
    assert again["n"] == 0
    rng1, ctr1 = R.ht.get_state()
    assert np.array_equal(rng0, rng1) and np.array_equal(ctr0, ctr1)
    assert len(R.wire.get_state()["host"]) == len(held["host"]) - got["n"]


def test_one_rank_equals_the_single_gpu_push(oracle, ctx):
    sc = wc.scenario(oracle)
    rd = sc["rounds"][0]
    pk = rd["pk"]
    # path A: sg_deliver_round + sg_wire_push
    h = sc["hosts"]
    ht = HostTable(h["ip"], h["route"], h["seed"], ctx=ctx)
    table = DeviceTable(_dev(sc["lat"].ravel(), np.uint64, np.int64), _dev(sc["loss"].ravel(), np.float32, np.float32),
                        wc.H)
    batch = PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"])
    out = deliver_round(ht, table, batch, rd["end"], wc.SIM_END, 0, ctx=ctx)
    a = PacketWire(wc.H, CAPACITY, MS, 16, ctx=ctx)
    a.push(batch, out, _dev(pk["len"], np.uint32, np.int32), id_base=rd["id_base"] + 7)
    # path B: sg_deliver_source + stamp + sg_wire_push_records
    R = Rank(ctx, sc, ws.partition(sc, 1), 0, 1, inbound=False)
    sel, b, length, _ = R.batch(0)
    src = R.sd.source_fn(ctx, R.ht, R.table, b, rd["end"], wc.SIM_END, 0, R.sd.owner_dev, 1)
    n = sum(src.send_counts)
    stamp_records(src.send, n, length, len(sel), id_base=rd["id_base"] + 7, ctx=ctx)
    R.wire.push_records(src.send, n)
    sa, sb = a.get_state(), R.wire.get_state()
    assert len(sa["host"]) == rd["want"]["delivered"] > 0
    for key in STATE_KEYS:
        assert np.array_equal(sa[key], sb[key]), key


def test_padded_protocol(oracle, ctx):
    """Round 0 exact, rounds 1 .. 11 through blocks of the cap test_wire_sharded_cpu.py fixes.  A round
    whose largest pair count exceeds cap: the padded push appends nothing, and after
    sg_deliver_pad_to_compact and the exact exchange the wire has gained exactly the round's records."""
    import torch

    W = ws.PADDED_W
    sc = wc.scenario(oracle)
    part = ws.partition(sc, W)
    cap = ws.padded_cap(sc)
    counts = ws.pair_counts(sc, part)
    ranks = [Rank(ctx, sc, part, r, W) for r in range(W)]
    ran = dict(padded=0, overflow=0)
    for k in range(wc.ROUNDS):
        rd = sc["rounds"][k]
        if k == 0:
            _exact_round(ranks, k)
        elif k < wc.SEND_ROUNDS:
            srcs = []
            for R in ranks:
                sel, b, length, ids = R.batch(k)
                s = gpu_source_phase_padded(ctx, R.ht, R.table, b, rd["end"], wc.SIM_END, 0, R.sd.owner_dev, W, cap)
                before = (_host(s.send_padded, RECORD_DTYPE).copy(), _host(s.send, RECORD_DTYPE).copy())
                stamp_records_padded(s.send_padded, s.send, W, cap, s.xrow, length, len(sel), packet_id=ids, ctx=ctx)
                _check_padded_stamp(before, s, counts[k][R.r], cap, rd, sel)
                srcs.append(s)
            xall = torch.cat([s.xrow for s in srcs]).contiguous()
            xa = xall.cpu().numpy().view(np.uint64).reshape(W, 3 + W)
            assert np.array_equal(xa[:, 3:], counts[k])
            overflow = int(xa[:, 3:].max()) > cap
            held = [len(R.wire.get_state()["host"]) for R in ranks]
            for d, R in enumerate(ranks):
                recv = torch.cat([s.send_padded[d * cap:(d + 1) * cap] for s in srcs]).contiguous()
                R.wire.push_records_padded(recv, W, cap, xall, d, R.host_map)
                assert R.wire.count == held[d] + W * cap  # conservative until the next pop / get_state
            if overflow:
                ran["overflow"] += 1
                for d, R in enumerate(ranks):
                    assert len(R.wire.get_state()["host"]) == held[d], (k, d)  # nothing was appended
                full = [gpu_pad_to_compact(ctx, s, W) for s in srcs]
                for d, R in enumerate(ranks):
                    parts = []
                    for s_, f in enumerate(full):
                        off = int(counts[k][s_, :d].sum())
                        parts.append(f[off:off + int(counts[k][s_, d])])
                    recv = torch.cat(parts).contiguous()
                    assert recv.shape[0] == int(counts[k][:, d].sum())
                    R.wire.push_records(recv, recv.shape[0], R.host_map)
            else:
                ran["padded"] += 1
            for d, R in enumerate(ranks):  # the round's records, once
                assert len(R.wire.get_state()["host"]) == held[d] + int(counts[k][:, d].sum()), (k, d)
        for R in ranks:
            R.inbound(k, R.pop(k))
    assert ran["padded"] > 0 and ran["overflow"] > 0 and ran["padded"] + ran["overflow"] == wc.SEND_ROUNDS - 1
    assert all(R.wire.count == 0 for R in ranks)


def _check_padded_stamp(before, s, row, cap, rd, sel):
    """After sg_wire_stamp_records_padded: the valid slots of the blocks and the spilled records at
    their compact positions carry (len, packet id) of their packet; every other byte is as before."""
    pk = rd["pk"]
    for arr0, t, valid in ((before[0], s.send_padded, _block_mask(row, cap)),
                           (before[1], s.send, _spill_mask(row, cap, len(before[1])))):
        now = _host(t, RECORD_DTYPE)
        assert np.array_equal(now[~valid], arr0[~valid])
        p = sel[arr0["packet"][valid]]
        w = now[valid].view(WIRE_RECORD_DTYPE)
        assert np.array_equal(w["len"], pk["len"][p]) and np.array_equal(w["packet_id"], rd["id_base"] + p)
        assert np.array_equal(w["src_host"], pk["src"][p]) and np.array_equal(w["src_host"],
                                                                               arr0["order_key"][valid] >> np.uint64(32))
        for key in ("deliver_time_ns", "event_id", "dst_host"):
            assert np.array_equal(w[key], arr0[key][valid]), key


def _block_mask(row, cap):
    m = np.zeros(len(row) * cap, bool)
    for r, c in enumerate(row):
        m[r * cap:r * cap + min(int(c), cap)] = True
    return m


def _spill_mask(row, cap, n):
    m = np.zeros(n, bool)
    start = 0
    for c in row:
        if c > cap:
            m[start + cap:start + int(c)] = True
        start += int(c)
    return m


def _synthetic(n, n_hosts, seed, span_ms=20):
    """n stamped records: times over span_ms (a 8 x 1 ms ring puts the later ones on the far list),
    with ties on (host, time); (src_host, event_id) unique."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, WIRE_RECORD_DTYPE)
    rec["deliver_time_ns"] = T0 + rng.integers(0, span_ms * MS, n).astype(np.uint64)
    rec["dst_host"] = rng.integers(0, n_hosts, n)
    tie = n // 10
    rec["deliver_time_ns"][tie:2 * tie] = rec["deliver_time_ns"][:tie]
    rec["dst_host"][tie:2 * tie] = rec["dst_host"][:tie]
    rec["src_host"] = rng.integers(0, n_hosts, n)
    rec["event_id"] = rng.permutation(n).astype(np.uint64) + (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(40))
    rec["len"] = rng.integers(28, 1500, n)
    rec["packet_id"] = rng.permutation(4 * n)[:n]
    return rec


def _ref_add(ref, rec):
    ref.add(host=rec["dst_host"], time_ns=rec["deliver_time_ns"], src_host=rec["src_host"], event_id=rec["event_id"],
            packet=rec["packet_id"], len=rec["len"])


def _drain_in_steps(w, ref):
    for end in (T0 + 3 * MS, T0 + 3 * MS + 1, T0 + 9 * MS, T0 + 14 * MS + 500, NEVER):
        want, nxt = ref.pop(end)
        _same_pop(w.pop(end), want, nxt, end)
    assert w.count == 0


def test_append_steps_and_workgroups(ctx):
    """5,000 records in one push: past the 2,048 of one workgroup step, so several workgroups append
    to the same rows; 20 ms of times through an 8 x 1 ms ring, so the far list is used."""
    n, H = 5000, 40
    rec = _synthetic(n, H, 1)
    pairs = np.stack([rec["dst_host"].astype(np.uint64), rec["deliver_time_ns"]])
    assert np.unique(pairs, axis=1).shape[1] <= n - n // 10  # ties on (host, time)
    assert int(rec["deliver_time_ns"].max() - T0) > 8 * MS
    w, ref = PacketWire(H, 8192, MS, 8, ctx=ctx), WireRef()
    w.push_records(_records(rec), n)
    _ref_add(ref, rec)
    st, want = w.get_state(), ref.state()
    for key in STATE_KEYS:
        assert np.array_equal(st[key], want[key]), key
    _drain_in_steps(w, ref)


def _padded_blocks(counts, cap, seed):
    """Blocks of cap slots holding counts[b] records each; the slots past the counts hold records
    that would show if read: time 0 and a host nobody owns."""
    blocks, good = [], []
    for b, c in enumerate(counts):
        blk = np.zeros(cap, WIRE_RECORD_DTYPE)
        blk["dst_host"] = 0xFFFFFFF0
        blk["packet_id"] = 0xDEAD
        r = _synthetic(c, 40, seed + b)
        r["event_id"] += np.uint64(b) << np.uint64(48)  # unique across blocks
        blk[:c] = r
        blocks.append(blk)
        good.append(r)
    return np.concatenate(blocks), np.concatenate(good)


def test_padded_blocks_with_stale_slots(ctx):
    import torch

    cap, rank, W = 1024, 1, 3
    counts = (1024, 0, 700)
    padded, good = _padded_blocks(counts, cap, 20)
    xa = np.full((W, 3 + W), 5, np.uint64)
    xa[:, 3 + rank] = counts
    xall = torch.from_numpy(xa.view(np.int64).ravel().copy()).cuda()
    w, ref = PacketWire(40, 8192, MS, 8, ctx=ctx), WireRef()
    w.push_records_padded(_records(padded), W, cap, xall, rank)
    assert w.count == W * cap
    _ref_add(ref, good)
    st, want = w.get_state(), ref.state()
    assert len(st["host"]) == sum(counts) and w.count == sum(counts)
    for key in STATE_KEYS:
        assert np.array_equal(st[key], want[key]), key
    # another pair of ranks outgrew its block: this rank, too, appends nothing
    xa[2, 3 + 0] = cap + 1
    w.push_records_padded(_records(padded), W, cap, torch.from_numpy(xa.view(np.int64).ravel().copy()).cuda(), rank)
    assert len(w.get_state()["host"]) == sum(counts)
    _drain_in_steps(w, ref)


@pytest.mark.parametrize("case", ["dst_past_n_hosts", "mapped_to_none"])
def test_bad_destination_is_reported_by_the_next_pop(ctx, case):
    import torch

    rec = _synthetic(300, 8, 3)
    if case == "dst_past_n_hosts":
        rec["dst_host"][137] = 8
        host_map = None
    else:  # the host belongs to another rank: its slot is UINT32_MAX (HostPartition.local's NONE)
        m = np.arange(8, dtype=np.uint32)
        m[5] = 0xFFFFFFFF
        rec["dst_host"][rec["dst_host"] == 5] = 4
        rec["dst_host"][137] = 5
        host_map = torch.from_numpy(m.view(np.int32)).cuda()
    w = PacketWire(8, 1024, MS, 8, ctx=ctx)
    w.push_records(_records(rec), len(rec), host_map)  # SG_OK: nothing is known on the host yet
    with pytest.raises(ShadowGpuError) as e:
        w.pop(NEVER)
    assert e.value.code == _capi.SG_ERR_INVALID_ARG and "sg_wire_push_records" in str(e.value)
    # an argument error reported late, not a fault: the context goes on working
    w2, ref = PacketWire(8, 1024, MS, 8, ctx=ctx), WireRef()
    good = _synthetic(300, 8, 4)
    w2.push_records(_records(good), len(good))
    _ref_add(ref, good)
    want, nxt = ref.pop(NEVER)
    _same_pop(w2.pop(NEVER), want, nxt)


def test_capacity_is_checked_before_any_launch(ctx):
    rec = _synthetic(300, 8, 5)
    w, ref = PacketWire(8, 400, MS, 8, ctx=ctx), WireRef()
    w.push_records(_records(rec), 300)
    _ref_add(ref, rec)
    with pytest.raises(ShadowGpuError) as e:
        w.push_records(_records(_synthetic(101, 8, 6)), 101)
    assert e.value.code == _capi.SG_ERR_CAPACITY and w.count == 300
    import torch

    xall = torch.zeros(2 * 5, dtype=torch.int64, device="cuda")
    with pytest.raises(ShadowGpuError) as e:
        w.push_records_padded(_records(np.zeros(2 * 51, WIRE_RECORD_DTYPE)), 2, 51, xall, 0)
    assert e.value.code == _capi.SG_ERR_CAPACITY and w.count == 300
    st, want = w.get_state(), ref.state()
    for key in STATE_KEYS:
        assert np.array_equal(st[key], want[key]), key
    w.push_records(_records(_synthetic(100, 8, 7)), 100)  # exactly full
    assert w.count == 400


@pytest.mark.parametrize("ids", ["array", "base"])
def test_stamp_leaves_the_rest_alone(ctx, ids):
    n, extra, n_packets = 3000, 100, 3500
    rng = np.random.default_rng(9)
    rec = np.zeros(n + extra, RECORD_DTYPE)
    rec["deliver_time_ns"] = rng.integers(0, 2**63, n + extra).astype(np.uint64)
    rec["order_key"] = (rng.integers(0, 2**32, n + extra).astype(np.uint64) << np.uint64(32)) | \
        rng.integers(0, 2**32, n + extra).astype(np.uint64)
    rec["event_id"] = rng.integers(0, 2**63, n + extra).astype(np.uint64)
    rec["packet"] = rng.permutation(n_packets)[:n + extra]
    rec["packet"][[5, 2999]] = [n_packets, 0xFFFFFFFF]  # not packets of the batch: left alone
    rec["dst_host"] = rng.integers(0, 2**32, n + extra)
    length = rng.integers(28, 65536, n_packets).astype(np.uint32)
    pid = rng.permutation(2**20)[:n_packets].astype(np.uint32)
    t = _records(rec)
    stamp_records(t, n, _dev(length, np.uint32, np.int32), n_packets,
                  packet_id=_dev(pid, np.uint32, np.int32) if ids == "array" else None, id_base=77, ctx=ctx)
    now = _host(t, RECORD_DTYPE)
    assert np.array_equal(now[n:], rec[n:])  # the slots past n_records: byte-identical
    ok = np.zeros(n + extra, bool)
    ok[:n] = rec["packet"][:n] < n_packets
    assert ok.sum() == n - 2 and np.array_equal(now[~ok], rec[~ok])
    w, p = now[ok].view(WIRE_RECORD_DTYPE), rec["packet"][ok]
    for key in ("deliver_time_ns", "event_id", "dst_host"):
        assert np.array_equal(w[key], rec[key][ok]), key
    assert np.array_equal(w["src_host"], rec["order_key"][ok] >> np.uint64(32))
    assert np.array_equal(w["len"], length[p])
    assert np.array_equal(w["packet_id"], pid[p] if ids == "array" else (77 + p).astype(np.uint32))
