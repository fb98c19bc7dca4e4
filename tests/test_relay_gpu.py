"""The relay boundary cases (relay_cases.py) through the lane kernels, one lane per case: the model
(relay_ref.py), the oracle (qdisc_ref.py for round-robin, which the oracle does not have) and the
library compared three ways and bit for bit after every call -- statuses and forward times, event
counters, task_time / task_id / task_born, tb_bal / tb_last, cached packets, the queue's scalars
and live ring slots, and for outbound the sent batch.

Entries: sg_inbound_run, sg_inbound_run_ordered (k_inbound), sg_outbound_run unkeyed and keyed
(k_outbound), sg_outbound_run_qdisc on a fifo object (keyed, k_outbound) and on a round-robin one,
unkeyed and keyed (k_qdisc).  A case runs where its family applies: codel inbound only; local, tie
and rr outbound only, tie through the keyed entries only.  Layout "0" runs every test through the
contiguous-only loop and "1" through the lane-major chunk map; the with_chunk_map loop with a
contiguous block beside a lane-major one needs E > 2 CH nb events in a call, which
test_boundary_cases_among_traffic brings and asserts for every call."""
import numpy as np
import pytest

import lane_cases
import qdisc_ref
import relay_cases as rc
import relay_ref as ref
from shadow_amd.router import InboundPipeline, OutboundPipeline

pytestmark = pytest.mark.gpu
T0, MS = rc.T0, rc.MS
S = 4   # sockets per host on the round-robin object
# entry: direction, keyed, qdisc, the chunk the chunk form aligns on (k_qdisc's chunks are 384, 256 keyed:
# a boundary at a multiple of 768 or 512 is one of its boundaries too)
ENTRIES = {"inbound": ("i", False, ref.FIFO, 1024), "inbound_ordered": ("i", False, ref.FIFO, 1024),
           "outbound": ("o", False, ref.FIFO, 896), "outbound_keyed": ("o", True, ref.FIFO, 512),
           "qdisc_fifo": ("o", True, ref.FIFO, 512), "qdisc_rr": ("o", False, ref.ROUND_ROBIN, 768),
           "qdisc_rr_keyed": ("o", True, ref.ROUND_ROBIN, 512)}
# the chunk each entry's launch and blocks reckon with (lane_major_launch, lane_major_block)
LAUNCH_CHUNK = {"inbound": 1024, "inbound_ordered": 1024, "outbound": 896, "outbound_keyed": 512, "qdisc_fifo": 512,
                "qdisc_rr": 384, "qdisc_rr_keyed": 256}
_refs = {}   # the model's and the oracle's snapshots of a batch, computed once and shared by the layouts


def _dev(a, np_dtype, torch_dtype):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype).view(torch_dtype)).cuda()


ring_cap = rc.ring_cap


class QdiscRefRun:
    """qdisc_ref.Interfaces on a batch, in ModelRun's shape: the round-robin entry's second reference."""

    def __init__(self, b, keyed, cap):
        self.b, self.keyed = b, keyed
        self.q = qdisc_ref.Interfaces(b["ip"], b["bw"], cap, ref.ROUND_ROBIN, S)
        n = b["n_pkt"]
        self.status, self.fwd, self.ctr = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(len(b["bw"]), np.uint64)

    def call(self, j):
        end, (host, t, pkt, ln, pay, dst, sock, eid, born) = self.b["calls"][j]
        k = (eid, born) if self.keyed else (None, None)
        sent = self.q.run(host, t, pkt, ln, pay, dst, sock, end, self.b["boot"], self.b["sim_end"], self.ctr, self.fwd,
                          self.status, *k)
        out = rc.qdisc_snapshot(self.q.qdisc_state(), self.q.relay_state(), self.q.S, self.q.cap)
        out.update({"sent_" + k: sent[k] for k in rc.SENT})
        out.update(rc.fates(self.status, self.fwd, self.ctr))
        return out


def references(oracle, key, b, entry, cap):
    """Per call the snapshot the model and the second reference agree on."""
    if key not in _refs:
        d, keyed, qdisc, _ = ENTRIES[entry]
        m = rc.ModelRun(b, d, qdisc=qdisc, keyed=keyed, cap=cap, S=S)
        o = QdiscRefRun(b, keyed, cap) if qdisc == ref.ROUND_ROBIN else rc.OracleRun(oracle, b, d, keyed, cap=cap)
        snaps = []
        for j in range(len(b["calls"])):
            snaps.append(m.call(j))
            rc.same(snaps[-1], o.call(j), ("model against oracle", entry, j))
        _refs[key] = snaps
    return _refs[key]


class DeviceRun:
    """The library on a batch, in ModelRun's shape."""

    def __init__(self, ctx, b, entry, cap):
        import torch

        self.b, self.entry = b, entry
        self.dir, self.keyed, self.qdisc, _ = ENTRIES[entry]
        H, n = len(b["bw"]), b["n_pkt"]
        if self.dir == "i":
            self.p = InboundPipeline(b["bw"], cap, ctx=ctx)
        elif self.qdisc == ref.ROUND_ROBIN:
            self.p = OutboundPipeline(b["ip"], b["bw"], cap, ctx=ctx, qdisc="round-robin", max_sockets=S)
            assert self.p.max_sockets == S
        else:
            self.p = OutboundPipeline(b["ip"], b["bw"], cap, ctx=ctx)
        assert self.p.cap == cap
        self.fwd = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.ctr = torch.zeros(H, dtype=torch.int64, device="cuda")

    def call(self, j):
        import torch

        end, (host, t, pkt, ln, pay, dst, sock, eid, born) = self.b["calls"][j]
        b, n, p = self.b, len(host), self.p
        i32, i64 = (lambda a: _dev(a, np.uint32, np.int32)), (lambda a: _dev(a, np.uint64, np.int64))
        if self.dir == "i":
            args = (i32(host), i64(t), i32(pkt), i32(ln), end, b["boot"], b["sim_end"])
            if self.entry == "inbound":
                p.run(*args, self.fwd, self.status, self.ctr.data_ptr())
            else:   # fates per arrival of this call, scattered to the packet ids here
                a_st = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
                a_fwd = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
                p.run_ordered(*args, self.fwd, self.status, a_fwd, a_st, self.ctr.data_ptr())
                if n:
                    ids = torch.from_numpy(np.asarray(pkt, np.int64)).cuda()
                    left = a_st[:n] != 0
                    self.status[ids[left]] = a_st[:n][left]
                    fw = a_st[:n] == 1
                    self.fwd[ids[fw]] = a_fwd[:n][fw]
            out = rc.inbound_snapshot(p.get_state())
        else:
            kw = dict(sent_cap=n + (p.cap + 1) * p.n)
            if self.keyed and n:
                kw.update(event_id=i64(eid), event_created_ns=i64(born))
            if self.entry.startswith("qdisc"):
                kw.update(socket=i32(sock))
            batch, ids = p.run(i32(host), i64(t), i32(pkt), i32(ln), i32(pay), i32(dst), end, b["boot"], b["sim_end"],
                               self.fwd, self.status, self.ctr.data_ptr(), **kw)
            if self.qdisc == ref.ROUND_ROBIN:
                st = p.get_qdisc_state()
                out = rc.qdisc_snapshot(st, st, p.max_sockets, p.cap)
            else:
                out = rc.fifo_snapshot(p.get_state())
            u = lambda x, dt: x.cpu().numpy().view(dt).copy()
            out.update(sent_src_host=u(batch.src_host, np.uint32), sent_dst_ipv4=u(batch.dst_ipv4, np.uint32),
                       sent_payload_len=u(batch.payload_len, np.uint32), sent_send_time=u(batch.send_time_ns, np.uint64),
                       sent_packet=u(ids, np.uint32))
        out.update(rc.fates(self.status.cpu().numpy(), self.fwd.cpu().numpy().view(np.uint64),
                            self.ctr.cpu().numpy().view(np.uint64)))
        return out


def _run_batch(oracle, ctx, key, b, entry, cap):
    want = references(oracle, key, b, entry, cap)
    dev = DeviceRun(ctx, b, entry, cap)
    for j in range(len(b["calls"])):
        got = dev.call(j)
        diff = rc.who_differs(got, want[j], b)
        assert not diff, "%s, call %d: the device differs in %s" % (entry, j, "; ".join(
            "%s (%s)" % (n, ", ".join(k)) for n, k in sorted(diff.items())))
        rc.same(got, want[j], (entry, "call", j))
    return want


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("form", rc.FORMS)
@pytest.mark.parametrize("layout", lane_cases.LAYOUTS)
def test_boundary_cases(oracle, ctx, monkeypatch, layout, form, entry):
    """Every case that applies to the entry, one host per case, environment by environment, spread
    over 130 hosts (two full blocks and a tail; the chunk form: behind 60 idle hosts, so that the
    cases and their fillers cross from the first block into the second).  These batches are small:
    an unset layout launches the contiguous-only loop as "0" does, except where the chunk form's
    fillers push E past 2 CH nb; the per-block choice is test_boundary_cases_among_traffic's."""
    lane_cases.set_layout(monkeypatch, layout)
    d, keyed, _, chunk = ENTRIES[entry]
    n_cases = 0
    for env in rc.ENVS:
        cs = rc.of(env, d, keyed)
        if form == "chunk":
            b = rc.build(cs, env, form, chunk=chunk, lead=60)
        else:
            b = rc.build(cs, env, form, hosts=rc.spread(len(cs)), n_hosts=130)
        assert 64 < len(b["bw"]) <= 256 and min(b["host"]) < 64 <= max(b["host"])   # more than one block
        want = _run_batch(oracle, ctx, (env, form, entry), b, entry, ring_cap(d, form))
        assert (want[-1]["pkt_status"] == 1).any()
        n_cases += len(cs)
    assert n_cases == len([c for c in rc.CASES if d in c["dirs"] and (keyed or not c["keyed"])])   # no case left out


# ---- among traffic: the launch and the blocks' layouts are the ones sg_lanes.h would choose ----------------
H_TRAFFIC, BUSY, LONG, CHUNK_COST = 256, 48, 255, 10


def lane_major_launch(E, nb, ch):
    """sg_codel.hip lane_major_launch under an unset SG_LANE_MAJOR (mode 2)."""
    return 2 if E > 2 * ch * nb else 0


def lane_major_block(counts, ch):
    """sg_lanes.h lane_major_block (mode 2) for one block's per-host event counts."""
    n_ev, max_n, h_act, lk = int(counts.sum()), int(counts.max()), int((counts > 0).sum()), ch // 64
    if n_ev <= 2 * ch:
        return False
    mean = n_ev // max(h_act, 1)
    c_cost = -(-n_ev // ch) * (CHUNK_COST + min(mean, ch))
    l_cost = -(-max_n // lk) * (CHUNK_COST + lk)
    return l_cost < c_cost


def _traffic(rng, cases_at, b, ch, per=8):
    """Every call gets, beside the cases: on the first block's other hosts BUSY small packets each at
    100 Mbit/s (the block goes lane-major), on the other blocks' hosts `per` packets each at
    1 Mbit/s (standing queues, CoDel drops, blocked relays), and on the last host, at 10 Gbit/s, as
    many 28-B packets 1 ns apart as bring the call past 2 CH nb events (its block stays
    contiguous).  A call that starts at or past sim_end gets the slow traffic only: its arrivals
    all stay queued.  Packet ids behind the cases'."""
    others = np.setdiff1d(np.arange(H_TRAFFIC - 1), cases_at)
    busy, slow = others[others < 64], others[others >= 64]
    b["bw"][busy], b["bw"][slow], b["bw"][LONG] = 10**8, 10**6, 10**10
    nb = H_TRAFFIC // 64
    calls, p, start = [], b["n_pkt"], T0
    for end, cols in b["calls"]:
        span = min(end, start + 50 * MS) - start
        live = start < b["sim_end"]   # past sim_end no task runs and every arrival stays queued: the slow traffic only
        host = np.r_[np.repeat(busy, BUSY if live else 0), np.repeat(slow, per)].astype(np.uint32)
        n = len(host)
        t = (start + rng.integers(0, span, n)).astype(np.uint64)
        ln = np.r_[np.full(len(busy) * (BUSY if live else 0), 28), rng.choice(np.array([28, 1476, 600]), len(slow) * per)].astype(np.uint32)
        n_long = 2 * ch * nb + 1 if live else 0
        host = np.r_[host, np.full(n_long, LONG)].astype(np.uint32)
        t = np.concatenate([t, (start + np.arange(n_long)).astype(np.uint64)])   # (np.r_ would go through float64)
        ln = np.r_[ln, np.full(n_long, 28)].astype(np.uint32)
        n += n_long
        o = np.lexsort((t, host))
        host, t, ln = host[o], t[o], ln[o]
        extra = (host, t, np.arange(p, p + n, dtype=np.uint32), ln, ln, np.full(n, rc.OTHER_IP, np.uint32),
                 rng.integers(0, S, n).astype(np.uint32), np.full(n, ref.U64, np.uint64), np.zeros(n, np.uint64))
        merged = [np.concatenate([a, x]) for a, x in zip(cols, extra)]
        o = np.argsort(merged[0], kind="stable")
        calls.append((end, tuple(a[o] for a in merged)))
        p, start = p + n, end
    return calls, p


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("layout", lane_cases.LAYOUTS)
def test_boundary_cases_among_traffic(oracle, ctx, monkeypatch, layout, entry):
    """The cases on scattered host ids of 256, random traffic on the hosts between them, so that the
    neighbours' lanes diverge -- and enough of it that every call of every environment launches
    the per-block choice under an unset layout (E > 2 CH nb), where the first block goes
    lane-major and the last, which is mostly one host, stays contiguous: with "0" and "1" beside
    it, both copies of each walk and both chunk maps run the cases here.  Inbound rings hold 64
    slots; an outbound ring bounds a call's sends, so the long host needs 16,384."""
    lane_cases.set_layout(monkeypatch, layout)
    d, keyed, _, chunk = ENTRIES[entry]
    ch = LAUNCH_CHUNK[entry]
    for env in rc.ENVS:
        key = (env, "traffic", entry)
        if key + ("batch",) not in _refs:
            rng = np.random.default_rng(len(env))
            cs = rc.of(env, d, keyed)
            at = np.sort(rng.choice(H_TRAFFIC - 1, len(cs), replace=False))
            b = rc.build(cs, env, "window", hosts=at, n_hosts=H_TRAFFIC)
            b["calls"], b["n_pkt"] = _traffic(rng, at, b, ch)
            _refs[key + ("batch",)] = b
        b = _refs[key + ("batch",)]
        starts = [T0] + [c[0] for c in b["calls"][:-1]]
        for start, (end, cols) in zip(starts, b["calls"]):   # what an unset layout launches, and what its blocks choose
            if start >= b["sim_end"]:
                continue   # (the end family's last call: nothing runs any more, see _traffic)
            counts = np.bincount(cols[0], minlength=H_TRAFFIC).reshape(-1, 64)
            assert lane_major_launch(len(cols[0]), len(counts), ch) == 2
            assert lane_major_block(counts[0], ch) and not lane_major_block(counts[-1], ch)
        want = _run_batch(oracle, ctx, key, b, entry, 64 if d == "i" else 16384)
        assert (want[-1]["pkt_status"] == 0).any() and (want[-1]["rflags"] & ref.RL_CACHED).any()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_boundary_cases_one_event_per_call(oracle, ctx, entry):
    """A call per distinct event time: every intermediate state goes through memory and get_state."""
    d, keyed, _, _ = ENTRIES[entry]
    calls = 0
    for env in rc.ENVS:
        cs = rc.of(env, d, keyed)
        b = rc.build(cs, env, "single", hosts=rc.spread(len(cs)), n_hosts=130)
        _run_batch(oracle, ctx, (env, "single", entry), b, entry, 64)
        calls += len(b["calls"])
    assert calls >= 60
