"""The stream contract of the C ABI on a caller's non-blocking stream: harness and cases
(test_stream_cases_cpu.py qualifies the cases on the CPU, test_stream_gpu.py runs them).

include/shadow_gpu.h, at sg_ctx_set_stream: "every entry point launches on this stream and reads
device inputs in stream order".  The session context of conftest.py keeps the context's own
stream, a blocking one, on which no ordering mistake is visible.  Here the context's stream is
S = torch.cuda.Stream() (torch's pool streams are non-blocking) and every case goes through
Harness.run:

  1. two input sets A and B of equal shapes go to the device; they share every index-valued array
     and differ in value arrays only, so any mixture of the two is a valid input;
  2. a warm-up call on A with outputs of their final sizes (no first-use allocation later);
  3. on S: a delay kernel, then B copied over the input buffers device to device, then every
     device output filled with the poison byte;
  4. the library call;
  5. on S, with no host synchronisation of the test's own: every output copied to pinned host
     memory, then S.synchronize();
  6. every output against the reference of B.

Work on a wrong stream reads A; an output written ahead of S's earlier work is poisoned; one
written on another stream and not joined back is read as poison.  A case of several calls repeats
steps 3 and 4 per call (Harness.run, "stages"): most calls synchronise, so one delay would cover
the first call only.  Stateful objects (host tables, wires, lane pipelines) exist twice: the
warm-up runs on the twin, so the checked run starts from the state the reference starts from.

The delay must outlast the host-side span of a whole library call, so that a misplaced kernel
anywhere in the call starts before B lands: at least 4 W, W the largest warm call's wall time on
the context's own blocking stream (Harness(blocking=True) runs the same cases there and keeps
each case's longest call in .wall).  Measured on an MI355X: torch.cuda._sleep counts 2.4 cycles
per nanosecond (10,000,000 cycles: 4.18 ms); the calls take 0.06 ms (sg_link_load) to 3.72 ms
(the largest seen in four runs: sg_codel_get_state's copy of every ring; the lane calls themselves
take 1.2 to 2.9 ms): W = 3.72 ms.  DELAY_CYCLES = 72,000,000 gives 30 ms, 8 W.  A case of k calls
sits through k delays: the longest, the wire's eleven, takes 0.35 s.
test_stream_gpu.py::test_delay_outlasts_a_call measures the delay again on every run and holds
it to 4 W_MS.
"""
import functools
import time

import numpy as np

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import paths_cases as PC
import paths_ref as PR
import queue_cases as QC
import queue_ref as QR
import series_ref as SR
import trace_cases as XC
import trace_ref as XR
import tree_cases as TC
import tree_ref as TR

# ---- the delay: W, the cycle count and the measured delay (MI355X; see the module docstring)
W_MS = 3.72
DELAY_CYCLES = 72_000_000
DELAY_MS = 30.0

POISON_BYTE = 0xA5
VIEW = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64,
        np.dtype(np.int32): np.int32, np.dtype(np.int64): np.int64, np.dtype(np.float32): np.float32}


def poison(dtype):
    """The value of one `dtype` element whose bytes are all POISON_BYTE."""
    return np.full(np.dtype(dtype).itemsize, POISON_BYTE, np.uint8).view(dtype)[0]


def has_poison(a):
    a = np.asarray(a)
    return bool((a.view(np.uint8).reshape(a.size, a.dtype.itemsize) == POISON_BYTE).all(axis=1).any()) if a.size else False


def plus_poison(want):
    """What an output the library adds into holds after a call that started from poison."""
    with np.errstate(over="ignore"):
        return (np.asarray(want) + poison(want.dtype)).astype(want.dtype)


# ---------------------------------------------------------------------------
# the harness (GPU)
# ---------------------------------------------------------------------------
class Harness:
    """A context on a caller's non-blocking stream S, the delay, and the six steps of a case.
    blocking=True keeps the context's own blocking stream instead (for measuring W only)."""

    def __init__(self, blocking=False, cycles=None):
        import torch

        from shadow_amd import Context

        self.torch = torch
        self.cycles = int(DELAY_CYCLES if cycles is None else cycles)
        if blocking:
            self.ctx = Context(0)
            self.S = torch.cuda.ExternalStream(self.ctx.stream)
        else:
            self.S = torch.cuda.Stream()
            self.ctx = Context(0, stream=self.S.cuda_stream)
        self.blocking = blocking
        self.wall = {}  # case name -> seconds of the second warm call (W's source)

    def close(self):
        self.S.synchronize()
        self.ctx.close()

    def on_stream(self):
        return self.torch.cuda.stream(self.S)

    def delay(self):
        """Enqueue on the current stream a kernel that does nothing for DELAY_MS."""
        self.torch.cuda._sleep(self.cycles)

    def dev(self, a):
        """A host array on the device, as the torch tensor of its bits."""
        a = np.ascontiguousarray(a)
        if a.size == 0:
            a = np.zeros(1, a.dtype)
        return self.torch.from_numpy(a.view(VIEW[a.dtype]).ravel().copy()).to("cuda")

    def run(self, name, ins_a, ins_b, outs, call, *, expect_async=False, measure=False):
        """The six steps.  ins_a / ins_b: name -> host array, the device inputs of A and B; outs:
        name -> host array giving the size and type of a device output; call(din, dout, X, warm)
        makes the library call on device tensors din / dout (X is "A" or "B"; warm tells a
        stateful case to use its twin objects) and returns the call's host results.

        A case of several calls gives `call` as a list of stages (in_keys, out_keys, fn): most
        entry points synchronise, so the calls after the first would find S idle.  Each stage
        then gets a delay of its own: its inputs are set back to A, and behind the delay B is
        copied over them and its outputs are poisoned, then fn runs.  expect_async, one value or
        one per stage: True for a call documented as not synchronising (S must still sit in the
        delay when it returns), "syncs" for one documented to synchronise (S must be idle).

        Returns (host results of the call on B -- a list with stages --, name -> output as a host
        array)."""
        torch = self.torch
        S = self.S
        assert set(ins_a) == set(ins_b)
        single = callable(call)
        stages = [(tuple(ins_a), tuple(outs), call)] if single else list(call)
        stages = [tuple(st) + ((),) * (4 - len(st)) for st in stages]  # (.., zero_keys): outputs the caller must zero
        want_async = [bool(expect_async)] * len(stages) if isinstance(expect_async, bool) else list(expect_async)
        differ = {k for k in ins_a if not np.array_equal(ins_a[k], ins_b[k])}
        with torch.cuda.stream(S):
            d_a = {k: self.dev(ins_a[k]) for k in differ}
            d_b = {k: self.dev(ins_b[k]) for k in differ}
            din = {k: self.dev(v) for k, v in ins_a.items()}
            dout = {k: self.dev(np.zeros_like(v)) for k, v in outs.items()}
            pinned = {k: torch.empty(t.shape, dtype=t.dtype, device="cpu").pin_memory() for k, t in dout.items()}
            S.synchronize()
            walls = []
            for _, _, fn, zero_keys in stages:
                for k in zero_keys:
                    dout[k].zero_()
                t0 = time.perf_counter()
                fn(din, dout, "A", True)
                S.synchronize()
                walls.append(time.perf_counter() - t0)
            self.wall[name] = max(walls)  # (W: a case run a second time has no first-use allocation in it)
            rets, self.span = [], []
            for (in_keys, out_keys, fn, zero_keys), no_sync in zip(stages, want_async):
                for k in in_keys:
                    if k in differ:
                        din[k].copy_(d_a[k])
                t0 = time.perf_counter()
                self.delay()
                for k in in_keys:
                    if k in differ:
                        din[k].copy_(d_b[k])
                for k in out_keys:
                    dout[k].view(torch.uint8).fill_(POISON_BYTE)
                for k in zero_keys:  # (where the entry point asks for zeroed memory: zeroed behind the delay)
                    dout[k].zero_()
                rets.append(fn(din, dout, "B", False))
                busy = not S.query()
                self.span.append(time.perf_counter() - t0)  # host seconds from the delay's enqueue to the return
                if no_sync == "syncs":
                    assert not busy, f"{name}: documented as synchronising, but S was busy when the call returned"
                elif no_sync and not self.blocking:  # (measuring W: next to no delay)
                    assert busy, f"{name}: documented as not synchronising, but S was idle when the call returned " \
                                 f"({self.span[-1] * 1e3:.2f} ms after the delay was enqueued)"
            for k, t in dout.items():
                pinned[k].copy_(t, non_blocking=True)
            S.synchronize()
        got = {k: pinned[k].numpy().view(outs[k].dtype)[:outs[k].size].reshape(outs[k].shape).copy() for k in outs}
        return (rets[0] if single else rets), got


def find_reader(h, candidates=4):
    """The first of up to `candidates` fresh non-blocking streams on which a copy runs while S sits
    in the delay (two streams may share a hardware queue): (stream, how many were tried), or
    (None, candidates)."""
    torch = h.torch
    a = np.arange(4096, dtype=np.int64)
    with h.on_stream():
        buf, other = h.dev(a), h.dev(a + 7)
        h.S.synchronize()
    host = torch.empty(4096, dtype=torch.int64).pin_memory()
    for k in range(candidates):
        R = torch.cuda.Stream()
        with h.on_stream():
            buf.copy_(h.dev(a))
            h.S.synchronize()
            h.delay()
            buf.copy_(other)
        with torch.cuda.stream(R):
            host.copy_(buf, non_blocking=True)
            R.synchronize()
        saw_a = bool(np.array_equal(host.numpy(), a))
        h.S.synchronize()
        if saw_a:
            return R, k + 1
    return None, candidates


# ---------------------------------------------------------------------------
# the shared world: the tie graph, its tables and trees, one round (CPU)
# ---------------------------------------------------------------------------
N = 300
NODES = np.arange(N, dtype=np.uint32)


def _oracle_table(g):
    from oracle import oracle as O

    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], NODES, threads=4)
    assert rc == 0
    return lat, loss


@functools.lru_cache(None)
def world():
    """Graph A = tree_cases.tie_graph(); graph B = its edge list under other latencies and losses
    (the index arrays src / dst shared).  For each: the oracle's table and tree_ref's trees.  The
    round: trace_cases.tie_round() (10,000 packets, mixed statuses), and for B other payloads,
    send times and statuses on the same (source, destination) arrays."""
    ga = TC.tie_graph()
    rng = np.random.default_rng(77)
    m = len(ga["src"])
    gb = dict(ga, lat=(rng.integers(1, 5, m).astype(np.uint64) * np.uint64(1_000_000)),
              loss=np.where(rng.random(m) < 0.5, np.float32(0.25), np.float32(0.0)).astype(np.float32))
    w = {}
    for x, g in (("A", ga), ("B", gb)):
        lat, loss = _oracle_table(g)
        pred, hop, bad = TR.tree_ref(g, NODES, (0, N), lat, loss)
        assert bad is None
        w[x] = dict(g=g, lat=lat, loss=loss, pred=pred, hop=hop)
    hosts, pk, status = XC.tie_round()
    npk = len(pk["src"])
    pkb = dict(pk, payload=((pk["payload"].astype(np.uint64) * 7 + 13) % 1400).astype(np.uint32),
               send_time=pk["send_time"] + np.uint64(125_000) + (np.arange(npk, dtype=np.uint64) % np.uint64(3)) * np.uint64(1000))
    w["hosts"] = hosts
    w["A"].update(pk=pk, status=status)
    w["B"].update(pk=pkb, status=np.repeat(RC.mixed_status(npk // 2, seed=43), 2))
    return w


class Case:
    """A case: sets() gives (A, B), two dicts of every input array; INDEX names the arrays both
    share; ref(X) gives every output the GPU test compares (name -> array) for X = A or B; ADDS
    names the outputs the library adds into (they start from poison and hold poison + value);
    gpu(h) runs the six steps and returns the outputs by the same names."""
    name = ""
    INDEX = ()
    ADDS = ()
    PADDED = {}   # output -> the output holding its record count: the rest of the array keeps the poison
    SAME = ()     # outputs that follow from the index arrays alone, so ref(A) == ref(B) there
    STALE = True  # the case has device inputs that differ between A and B
    PARTIAL = ()  # outputs indexed by packet id that the library writes only where a packet left: the rest keeps the poison
    HOST_SIZED = ()  # host results whose length is itself a result (it may differ between A and B)

    def sets(self):
        raise NotImplementedError

    def ref(self, x):
        raise NotImplementedError

    def gpu(self, h):
        raise NotImplementedError

    def want(self):
        """ref(B) as the device shows it: poison added where the library adds into."""
        return {k: plus_poison(v) if k in self.ADDS else v for k, v in self.ref("B").items()}


def _net(g, ctx):
    from shadow_amd import NetworkGraph

    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    net._ensure_net()
    return net


def _host_table(hosts, ctx):
    from shadow_amd.worker import HostTable

    return HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)


def _batch(din):
    from shadow_amd.worker import PacketBatch

    return PacketBatch(din["src"], din["dst_ip"], din["payload"], din["send_time"])


def _u64(x):
    return np.asarray([x], np.uint64)


# ---------------------------------------------------------------------------
# trees: sg_routing_tree (device table in, pred and first hop out)
# ---------------------------------------------------------------------------
class TreeCase(Case):
    """sg_routing_tree on the tie graph: the device table of graph X in, pred and first_hop out.
    A and B are two graphs on one edge list, so the net (uploaded before the delay, host arrays)
    is X's own and only the table is swapped behind the delay."""
    INDEX = ("src", "dst")

    def __init__(self, lds):
        self.lds = lds
        self.name = f"tree_lds{lds}"

    def sets(self):
        w = world()
        return tuple(dict(src=w[x]["g"]["src"], dst=w[x]["g"]["dst"], edge_lat=w[x]["g"]["lat"],
                          edge_loss=w[x]["g"]["loss"], lat=w[x]["lat"], loss=w[x]["loss"]) for x in "AB")

    def ref(self, x):
        w = world()[x]
        return dict(pred=w["pred"], hop=w["hop"])

    def gpu(self, h, measure=False):
        w = world()
        a, b = self.sets()
        with h.on_stream():
            nets = {x: _net(w[x]["g"], h.ctx) for x in "AB"}

        def call(din, dout, x, warm):
            nets[x].tree_rows_device(NODES, 0, N, din["lat"].data_ptr(), din["loss"].data_ptr(), dout["pred"].data_ptr(),
                                     dout["hop"].data_ptr())

        pick = lambda s: {k: s[k] for k in ("lat", "loss")}  # noqa: E731
        _, got = h.run(self.name, pick(a), pick(b), self.ref("B"), call, measure=measure)
        return got


class BuildTreeCase(Case):
    """sg_routing_build_tree with device outputs (table, pred, first hop): no device input, the
    poison and read-back half."""

    def __init__(self, lds):
        self.lds = lds
        self.name = f"build_tree_lds{lds}"

    def sets(self):
        return TreeCase(self.lds).sets()

    INDEX = ("src", "dst")

    def ref(self, x):
        w = world()[x]
        return dict(lat=w["lat"], loss=w["loss"], pred=w["pred"], hop=w["hop"])

    def gpu(self, h, measure=False):
        from shadow_amd import _capi

        w = world()
        with h.on_stream():
            nets = {x: _net(w[x]["g"], h.ctx) for x in "AB"}

        def call(din, dout, x, warm):
            p = lambda k: _capi.C.c_void_p(dout[k].data_ptr())  # noqa: E731
            _capi.check(h.ctx.handle, _capi.load().sg_routing_build_tree(
                h.ctx.handle, nets[x]._ensure_net(), NODES.ctypes.data, N, 0, N,
                _capi.SG_ROUTE_SHORTEST_PATH | _capi.SG_ROUTE_OUT_DEVICE, p("lat"), p("loss"), p("pred"), p("hop")))

        _, got = h.run(self.name, {}, {}, self.ref("B"), call, measure=measure)
        return got


# ---------------------------------------------------------------------------
# the link family on the tie graph's round, device forms
# ---------------------------------------------------------------------------
def _link_tables(x):
    """The table a link-family call looks its records' latencies and losses up in.  The pred rows
    are graph A's for both sets (an index array); B's table is A's under other values (the calls
    gather from it, they do not check it against the graph)."""
    w = world()["A"]
    if x == "A":
        return w["lat"], w["loss"]
    return w["lat"] * np.uint64(2) + np.uint64(5), (w["loss"] * np.float32(0.5)).astype(np.float32)


def _round(x):
    w = world()
    return w["hosts"], w[x]["pk"], w[x]["status"]


class LinkCase(Case):
    """Base of the link family: the round's arrays as device inputs."""
    INDEX = ("src", "dst_ip", "pred")

    def sets(self):
        out = []
        for x in "AB":
            _, pk, status = _round(x)
            lat, loss = _link_tables(x)
            out.append(dict(src=pk["src"], dst_ip=pk["dst_ip"], payload=pk["payload"], send_time=pk["send_time"],
                            status=status, pred=world()["A"]["pred"], lat=lat, loss=loss))
        return tuple(out)

    def _objects(self, h):
        w = world()
        with h.on_stream():
            net = _net(w["A"]["g"], h.ctx)
            net.links()
            ht = _host_table(w["hosts"], h.ctx)
        return net, ht

    def _args(self, x):
        w = world()
        hosts, pk, status = _round(x)
        lat, loss = _link_tables(x)
        return w["A"]["g"], NODES, (0, N), w["A"]["pred"], lat, loss, hosts, pk, status


class LinkLoadCase(LinkCase):
    """sg_link_load: a device u64 matrix of counts folded onto links and nodes (adds into)."""
    name = "link_load"
    INDEX = ("pred",)
    ADDS = ("link", "node")

    def sets(self):
        pred = world()["A"]["pred"]
        return dict(pred=pred, counts=LC.sparse_matrix(N, N, seed=12)), dict(pred=pred, counts=LC.dense_matrix(N, N, seed=11))

    def ref(self, x):
        s = self.sets()["AB".index(x)]
        link, node = LR.link_load(world()["A"]["g"], NODES, (0, N), s["pred"], s["counts"])
        return dict(link=link, node=node)

    def gpu(self, h, measure=False):
        net, _ = self._objects(h)
        a, b = self.sets()

        def call(din, dout, x, warm):
            net.link_load_device(NODES, 0, N, din["pred"].data_ptr(), din["counts"].data_ptr(), N, dout["link"].data_ptr(),
                                 dout["node"].data_ptr())

        return h.run(self.name, a, b, self.ref("B"), call, measure=measure)[1]


class LinkLoadPacketsCase(LinkCase):
    """sg_link_load_packets: statuses and payload weights on the device; link and node loads added
    into, hops written."""
    name = "link_load_packets"
    ADDS = ("link", "node")

    def ref(self, x):
        g, nodes, rows, pred, _, _, hosts, pk, status = self._args(x)
        link, node, hops = RR.link_load_round(g, nodes, rows, pred, hosts, pk, status, pk["payload"])
        return dict(link=link, node=node, hops=hops)

    def gpu(self, h, measure=False):
        net, ht = self._objects(h)
        a, b = self.sets()

        def call(din, dout, x, warm):
            net.link_load_packets_device(ht, NODES, 0, N, din["pred"].data_ptr(), _batch(din), din["status"].data_ptr(),
                                         din["payload"].data_ptr(), dout["link"].data_ptr(), dout["node"].data_ptr(),
                                         dout["hops"].data_ptr())

        drop = lambda s: {k: v for k, v in s.items() if k not in ("lat", "loss")}  # noqa: E731
        return h.run(self.name, drop(a), drop(b), self.ref("B"), call, measure=measure)[1]


PAD = 64  # records of room past a hop-record or trace total: they keep the poison


class _Records(LinkCase):
    """Outputs of `total` records in arrays of total + PAD: the reference pads with poison."""

    PADDED = {k: "total" for k in ("node", "link", "olat", "oloss", "packet", "hop", "enter", "exit")}

    def _padded(self, recs, cap):
        out = {}
        for k, v in recs.items():
            p = np.full(cap, poison(v.dtype), v.dtype)
            p[:len(v)] = v
            out[k] = p
        return out


class TreePathsCase(_Records):
    """sg_tree_paths: 257 pairs (device row / column indices) through device pred rows and table."""
    name = "tree_paths"
    INDEX = ("pred", "row", "col")
    SAME = ("off", "total", "node", "link")

    def sets(self):
        ri, cj = PC.tie_pairs(257)
        out = []
        for x in "AB":
            lat, loss = _link_tables(x)
            out.append(dict(pred=world()["A"]["pred"], row=ri.astype(np.uint32), col=cj.astype(np.uint32), lat=lat, loss=loss))
        return tuple(out)

    def _cap(self):
        return int(self._recs("A")[0][-1]) + PAD

    @functools.lru_cache(None)
    def _recs(self, x):
        s = self.sets()["AB".index(x)]
        return PR.records(world()["A"]["g"], NODES, (0, N), s["pred"], s["lat"], s["loss"], s["row"].astype(np.int64),
                          s["col"].astype(np.int64))

    def ref(self, x):
        off, node, link, lat, loss = self._recs(x)
        return dict(off=off, total=_u64(off[-1]), **self._padded(dict(node=node, link=link, olat=lat, oloss=loss), self._cap()))

    def gpu(self, h, measure=False):
        net, _ = self._objects(h)
        a, b = self.sets()
        cap = self._cap()

        def call(din, dout, x, warm):
            return net.tree_paths_device(NODES, 0, N, din["pred"].data_ptr(), din["lat"].data_ptr(), din["loss"].data_ptr(),
                                         len(a["row"]), din["row"].data_ptr(), din["col"].data_ptr(), dout["off"].data_ptr(),
                                         dout["node"].data_ptr(), dout["link"].data_ptr(), dout["olat"].data_ptr(),
                                         dout["oloss"].data_ptr(), cap)

        want = self.ref("B")
        total, got = h.run(self.name, a, b, {k: v for k, v in want.items() if k != "total"}, call, measure=measure)
        return dict(got, total=_u64(total))


class TreePathsPacketsCase(_Records):
    """sg_tree_paths_packets: the round's hop records, statuses on the device."""
    name = "tree_paths_packets"

    @functools.lru_cache(None)
    def _recs(self, x):
        g, nodes, rows, pred, lat, loss, hosts, pk, status = self._args(x)
        return PR.packet_records(g, nodes, rows, pred, lat, loss, hosts, pk, status)

    def _cap(self):
        return max(int(self._recs(x)[0][-1]) for x in "AB") + PAD

    def ref(self, x):
        off, node, link, lat, loss = self._recs(x)
        return dict(off=off, total=_u64(off[-1]), **self._padded(dict(node=node, link=link, olat=lat, oloss=loss), self._cap()))

    def gpu(self, h, measure=False):
        net, ht = self._objects(h)
        a, b = self.sets()
        cap = self._cap()

        def call(din, dout, x, warm):
            return net.tree_paths_packets_device(ht, NODES, 0, N, din["pred"].data_ptr(), din["lat"].data_ptr(),
                                                 din["loss"].data_ptr(), _batch(din), din["status"].data_ptr(),
                                                 dout["off"].data_ptr(), dout["node"].data_ptr(), dout["link"].data_ptr(),
                                                 dout["olat"].data_ptr(), dout["oloss"].data_ptr(), cap)

        want = self.ref("B")
        total, got = h.run(self.name, a, b, {k: v for k, v in want.items() if k != "total"}, call, measure=measure)
        return dict(got, total=_u64(total))


class LinkTraceCase(_Records):
    """sg_link_trace_packets: the round's crossings per link in time order."""
    name = "link_trace_packets"

    @functools.lru_cache(None)
    def _recs(self, x):
        g, nodes, rows, pred, lat, _, hosts, pk, status = self._args(x)
        return XR.trace(g, nodes, rows, pred, lat, hosts, pk, status)

    def _cap(self):
        return max(len(self._recs(x)[1]) for x in "AB") + PAD

    def ref(self, x):
        off, packet, hop, enter, leave = self._recs(x)
        return dict(link_off=off, total=_u64(off[-1]),
                    **self._padded(dict(packet=packet, hop=hop, enter=enter, exit=leave), self._cap()))

    def gpu(self, h, measure=False):
        from shadow_amd import _capi

        net, ht = self._objects(h)
        a, b = self.sets()
        cap = self._cap()

        def call(din, dout, x, warm):
            rc, total = net.link_trace_packets_device(
                ht, NODES, 0, N, din["pred"].data_ptr(), din["lat"].data_ptr(), _batch(din), din["status"].data_ptr(), 0,
                dout["link_off"].data_ptr(), dout["packet"].data_ptr(), dout["hop"].data_ptr(), dout["enter"].data_ptr(),
                dout["exit"].data_ptr(), cap)
            assert rc == _capi.SG_OK
            return total

        drop = lambda s: {k: v for k, v in s.items() if k != "loss"}  # noqa: E731
        want = self.ref("B")
        total, got = h.run(self.name, drop(a), drop(b), {k: v for k, v in want.items() if k != "total"}, call,
                           measure=measure)
        return dict(got, total=_u64(total))


class LinkSeriesCase(LinkCase):
    """sg_link_series_packets, two rounds into one accumulator: the round at its enter times under
    its statuses and payload weights, then every packet of it at its exit times, weight 1."""
    name = "link_series_packets"
    ADDS = ("series", "outside")
    BIN_NS, N_BINS = 250_000, 64

    def ref(self, x):
        g, nodes, rows, pred, lat, _, hosts, pk, status = self._args(x)
        kw = dict(t0=XC.T0, bin_ns=self.BIN_NS, n_bins=self.N_BINS)
        first = SR.series(g, nodes, rows, pred, lat, hosts, pk, status, pk["payload"], at=SR.AT_ENTER, **kw)
        series, outside = SR.series(g, nodes, rows, pred, lat, hosts, pk, None, None, at=SR.AT_EXIT, base=first, **kw)
        return dict(series=series, outside=outside)

    def gpu(self, h, measure=False):
        net, ht = self._objects(h)
        a, b = self.sets()
        nl = XR.n_links(world()["A"]["g"])

        def stage(at):
            def fn(din, dout, x, warm):
                status, weight = (din["status"].data_ptr(), din["payload"].data_ptr()) if at == 0 else (0, 0)
                net.link_series_packets_device(ht, NODES, 0, N, din["pred"].data_ptr(), din["lat"].data_ptr(), _batch(din),
                                               status, weight, 0, nl, at, XC.T0, self.BIN_NS, self.N_BINS,
                                               dout["series"].data_ptr(), dout["outside"].data_ptr())
            return fn

        drop = lambda s: {k: v for k, v in s.items() if k != "loss"}  # noqa: E731
        a, b = drop(a), drop(b)
        # (the second round adds into the first one's cells: they are not poisoned again)
        stages = [(tuple(a), ("series", "outside"), stage(0)), (tuple(a), (), stage(1))]
        return h.run(self.name, a, b, self.ref("B"), stages, measure=measure)[1]


class LinkQueueCase(Case):
    """sg_link_queue, device form, two chained calls: the tie round's trace (the reference's) at
    queue_cases.TIE_COST, then the same records again with link_free_in = the first call's
    out_link_free.  A and B share link_off and packet; B's arrival times, weights, costs and
    free_in are other values (arrivals still ascending inside a link)."""
    name = "link_queue"
    INDEX = ("link_off", "packet")

    @functools.lru_cache(None)
    def sets(self):
        off, packet, _, enter, _ = LinkTraceCase()._recs("A")
        w = world()
        nl = len(off) - 1
        n = len(enter)
        a = dict(link_off=off, packet=packet, enter=enter, weight=w["A"]["pk"]["payload"],
                 cost_ps=np.full(nl, QC.TIE_COST, np.uint64), free_in=np.full(nl, XC.T0 + 100_000, np.uint64))
        seg = XR.segment_links(off)
        place = np.arange(n, dtype=np.int64) - off.astype(np.int64)[seg]  # a record's place in its link
        b = dict(a, enter=enter + np.uint64(40_000) + (place.astype(np.uint64) * np.uint64(900)),
                 weight=w["B"]["pk"]["payload"], cost_ps=QC.draw_costs(nl, 5, (80, 8000, 250_000)),
                 free_in=np.uint64(XC.T0) + (np.arange(nl, dtype=np.uint64) % np.uint64(7)) * np.uint64(300_000))
        return a, b

    @functools.lru_cache(None)
    def ref(self, x):
        s = self.sets()["AB".index(x)]
        out = {}
        free = s["free_in"]
        for r in ("1", "2"):
            rc, _, res = QR.loop(s["link_off"], s["enter"], s["packet"], s["weight"], cost_ps=s["cost_ps"], free_in=free)
            assert rc == QR.OK
            out.update({k + r: getattr(res, k) for k in QR.FIELDS})
            free = res.link_free
        return out

    def device_call(self, ctx, din, dout, r):
        """Call r ("1" or "2") of the two chained sg_link_queue calls on ctx."""
        from shadow_amd import _capi

        p = lambda t: _capi.C.c_void_p(t.data_ptr())  # noqa: E731
        s = self.sets()[0]
        free = din["free_in"] if r == "1" else dout["link_free1"]
        _capi.check(ctx.handle, _capi.load().sg_link_queue(
            ctx.handle, _capi.SG_ROUTE_OUT_DEVICE, len(s["link_off"]) - 1, p(din["link_off"]), len(s["enter"]),
            p(din["enter"]), p(din["packet"]), p(din["weight"]), len(s["weight"]), p(din["cost_ps"]), p(free),
            *[p(dout[k + r]) for k in QR.FIELDS]))

    def gpu(self, h, measure=False):
        a, b = self.sets()
        stages = [(tuple(a) if r == "1" else tuple(k for k in a if k != "free_in"), tuple(k + r for k in QR.FIELDS),
                   lambda din, dout, x, warm, r=r: self.device_call(h.ctx, din, dout, r)) for r in ("1", "2")]
        return h.run(self.name, a, b, self.ref("B"), stages, measure=measure)[1]


# ---------------------------------------------------------------------------
# table builds: sg_routing_build (device outputs), sg_routing_info_fill
# ---------------------------------------------------------------------------
SWEEP_GRAPH = "k11"  # 300 nodes, sparse (tests/sweep_cases.py)
APSP_KERNELS = ("lds", "lds_bounded", "lds_flagged", "bucket", "slab")  # conftest.APSP_KERNELS


@functools.lru_cache(None)
def _build_world(which):
    """(graph, node order, row block, the oracle's whole table) of the sparse 300-node graph or of
    sweep_cases.dense_blocks() (132 nodes, the 66 of its first block used: the dense search)."""
    import sweep_cases as WC
    from oracle import oracle as O

    if which == "dense":
        g = WC.dense_blocks()
        nodes = np.arange(WC.HALF, dtype=np.uint32)  # (split_cases' "D_used_first": the second block is a dead end)
    else:
        c = WC.case(SWEEP_GRAPH)
        g, nodes = c["g"], c["nodes"]
    n = len(nodes)
    rc, lat, loss, _ = WC.oracle_rows(O, g, nodes)
    assert rc == 0
    return g, nodes, (n // 3, n - n // 4), lat, loss


class BuildCase(Case):
    """sg_routing_build through build_rows_device: the whole table, then a row block, into device
    buffers.  No device input: the poison and read-back half of the steps (STALE is off, A is B).
    one_shot: a new net per call, as test_build_fused_gpu.py builds (upload and build in one
    chain, SG_BUILD_FUSED = 1 or 0).

    The plan's side stream runs in the whole-table build of "lds_bounded" (SG_SSSP_SEEDS=2,
    SG_SSSP_FLAGGED=0: the phased plan) with SG_BUILD_FUSED unset or 1 and timers off:
    sg_routing.hip:571 (overlap), sg_plan.hip:577-585 (the side stream and its events are created
    there and nowhere else), sg_routing.hip:592-603 (k_plan_bounds and, in a one-shot build,
    k_build_finish launched on it; the context's stream waits for plan_bounds).  No timer reports
    it: the overlap is off while timers are on."""
    STALE = False
    INDEX = ("src", "dst")

    def __init__(self, kernel, which="sparse", one_shot=False, fused=None):
        self.kernel, self.which, self.one_shot, self.fused = kernel, which, one_shot, fused
        self.env = {} if fused is None else {"SG_BUILD_FUSED": fused}
        self.name = f"build_{which}_{kernel}" + (f"_one_shot_fused{fused}" if one_shot else "")

    def sets(self):
        g = _build_world(self.which)[0]
        s = dict(src=g["src"], dst=g["dst"], edge_lat=g["lat"], edge_loss=g["loss"])
        return s, s

    def ref(self, x):
        _, _, (r0, r1), lat, loss = _build_world(self.which)
        return dict(lat=lat, loss=loss, block_lat=lat[r0:r1], block_loss=loss[r0:r1])

    def gpu(self, h, measure=False):
        g, nodes, (r0, r1), _, _ = _build_world(self.which)
        with h.on_stream():
            kept = None if self.one_shot else _net(g, h.ctx)

        def stage(rows, lat, loss):
            def fn(din, dout, x, warm):
                net = kept or _net(g, h.ctx)
                net.build_rows_device(nodes, rows[0], rows[1], dout[lat].data_ptr(), dout[loss].data_ptr())
            return fn

        stages = [((), ("lat", "loss"), stage((0, len(nodes)), "lat", "loss")),
                  ((), ("block_lat", "block_loss"), stage((r0, r1), "block_lat", "block_loss"))]
        return h.run(self.name, {}, {}, self.ref("B"), stages, measure=measure)[1]


class InfoFillCase(Case):
    """sg_routing_info_fill with SG_RI_BLOCK_ROWS=64: five blocks of the 300-node table pass through
    the context's copy stream and its two event pairs (sg_routing.hip:906-913; every fill goes
    through copy_stream, fill_rows creates it).  The cells are pinned host memory: they start from
    poison and every one is compared with the oracle at return (the call synchronises)."""
    name = "routing_info_fill"
    STALE = False
    INDEX = ("src", "dst")
    env = {"SG_RI_BLOCK_ROWS": "64"}
    kernel = "lds"

    def sets(self):
        return BuildCase("lds").sets()

    def ref(self, x):
        _, _, _, lat, loss = _build_world("sparse")
        return dict(lat=lat, loss=loss, smallest=_u64(lat.min()))

    def gpu(self, h, measure=False):
        from shadow_amd import RoutingInfo

        g, nodes, _, _, _ = _build_world("sparse")
        with h.on_stream():
            net = _net(g, h.ctx)
        ri = RoutingInfo(nodes)
        got = {}

        def call(din, dout, x, warm):
            ri.cells[...] = poison(np.uint64)
            ri.fill(net, nodes)
            if not warm:
                lat, loss = ri.rows()
                got.update(lat=lat, loss=loss, smallest=_u64(ri.get_smallest_latency_ns()))

        h.run(self.name, {}, {}, {}, call, measure=measure)
        return got


class MinLatencyCase(Case):
    """sg_routing_min_latency: a device latency table in, its smallest entry back on the host."""
    name = "routing_min_latency"

    def sets(self):
        w = world()
        return dict(lat=w["A"]["lat"]), dict(lat=w["B"]["lat"] + np.uint64(17))

    def ref(self, x):
        return dict(smallest=_u64(self.sets()["AB".index(x)]["lat"].min()))

    def gpu(self, h, measure=False):
        from shadow_amd import _capi

        a, b = self.sets()

        def call(din, dout, x, warm):
            out = _capi.C.c_uint64()
            _capi.check(h.ctx.handle, _capi.load().sg_routing_min_latency(h.ctx.handle, _capi.C.c_void_p(din["lat"].data_ptr()),
                                                                          a["lat"].size, _capi.C.byref(out)))
            return out.value

        return dict(smallest=_u64(h.run(self.name, a, b, {}, call, measure=measure)[0]))


BUILD_CASES = [BuildCase(k) for k in APSP_KERNELS] + [BuildCase("lds", "dense")] + \
              [BuildCase(k, one_shot=True, fused=f) for k in ("lds", "lds_bounded") for f in ("1", "0")] + \
              [InfoFillCase(), MinLatencyCase()]


# ---------------------------------------------------------------------------
# delivery: sg_table_pack, sg_deliver_round, sg_hosts_*
# ---------------------------------------------------------------------------
T0 = RC.T0


@functools.lru_cache(None)
def _deliver_world():
    """test_deliver_gpu._world(n_hosts=800, seed=5) (a 64-node ring with chords, the oracle's table
    with some cells made lossy), and for B the same table under other latencies and losses."""
    from oracle import oracle as O
    from shadow_amd import synth

    g = synth.ring_chords_graph(64, 6.0, seed=5)
    rc, lat, loss, _ = O.shortest_paths(64, g["src"], g["dst"], g["lat"], g["loss"], False, np.arange(64, dtype=np.uint32),
                                        threads=4)
    assert rc == 0
    loss = loss.copy()
    loss[::2, 1::3] = np.float32(0.3)
    loss[5, :] = np.float32(1.0)
    hosts = synth.make_hosts(800, 64, general_seed=5)
    lat_b = lat + np.uint64(777)
    loss_b = loss.copy()
    loss_b[1::2, ::3] = np.float32(0.2)
    return hosts, dict(A=(lat, loss), B=(lat_b, loss_b))


class DeliverCase(Case):
    """Two consecutive rounds of 15,000 packets through sg_deliver_round (stats taken: the call
    synchronises once), packet counters set, on the two-array table or on the packed one
    (sg_table_pack, a stage of its own); before them sg_hosts_set_state and sg_hosts_skip, after
    them sg_hosts_get_state.  A and B share sources and destination addresses; payloads, send
    times and the table differ.  The hosts' streams are set from a state of the test's own at the
    start (sg_hosts_set_state), so the warm-up rounds leave nothing behind."""
    INDEX = ("src1", "dst_ip1", "src2", "dst_ip2")
    ADDS = ("counts",)
    SAME = ("rng", "packed")  # one draw per packet whatever its fate: the streams follow from the sources
    PADDED = {"dst_order1": "delivered1", "dst_order2": "delivered2"}
    NPK = 15000
    SKIP = (np.array([3, 5, 3, 799, 0], np.uint32), np.array([2, 1, 4, 10, 1], np.uint64))

    def __init__(self, packed, stats=True):
        self.packed, self.stats = packed, stats
        self.name = "deliver_" + ("path_key" if packed else "two_array") + ("" if stats else "_no_stats")

    @functools.lru_cache(None)
    def sets(self):
        from shadow_amd import synth

        hosts, tabs = _deliver_world()
        out = []
        for x in "AB":
            s = dict(lat=tabs[x][0], loss=tabs[x][1])
            for r in (1, 2):
                pk = synth.make_packets(self.NPK, hosts, T0 + (r - 1) * 10**6, T0 + r * 10**6, seed=20 + r)
                if x == "B":
                    pk = dict(pk, payload=((pk["payload"].astype(np.uint64) * 5 + 3) % 1400).astype(np.uint32),
                              send_time=np.minimum(pk["send_time"] + np.uint64(1234), np.uint64(T0 + r * 10**6 - 1)))
                s.update({f"src{r}": pk["src"], f"dst_ip{r}": pk["dst_ip"], f"payload{r}": pk["payload"],
                          f"send_time{r}": pk["send_time"]})
            out.append(s)
        return tuple(out)

    def _state0(self):
        from oracle import oracle as O

        hosts, _ = _deliver_world()
        rng = np.stack([O.xoshiro_seed(int(s) ^ 0x5DEECE66D) for s in hosts["seed"]]).astype(np.uint64)
        return rng, (np.arange(hosts["n"], dtype=np.uint64) * np.uint64(3) + np.uint64(1))

    @functools.lru_cache(None)
    def ref(self, x):
        from oracle import oracle as O

        hosts, _ = _deliver_world()
        s = self.sets()["AB".index(x)]
        rng, ctr = self._state0()
        for hh, k in zip(*self.SKIP):
            for _ in range(int(k)):
                O.xoshiro_next_u64(rng[hh])
        n = s["lat"].shape[0]
        counts = np.zeros(n * n, np.uint64)
        ip_to_host = {int(ip): i for i, ip in enumerate(hosts["ip"])}
        out = {}
        for r in (1, 2):
            w = O.deliver_round(T0 + r * 10**6, 2**63, 0, s[f"src{r}"], s[f"dst_ip{r}"], s[f"payload{r}"], s[f"send_time{r}"],
                                hosts["ip"], hosts["route"], s["lat"], s["loss"], rng, ctr)
            order = np.full(self.NPK, poison(np.uint32), np.uint32)
            order[:w["delivered"]] = w["dst_order"]
            out.update({f"status{r}": w["status"], f"deliver_time{r}": w["deliver_time"], f"event_id{r}": w["event_id"],
                        f"dst_order{r}": order, f"dst_offsets{r}": w["dst_offsets"], f"delivered{r}": _u64(w["delivered"])})
            if self.stats:
                out.update({f"min_deliver{r}": _u64(w["min_deliver"]), f"min_lat{r}": _u64(w["min_lat"])})
            dlv = np.flatnonzero(w["status"] == 0)
            dh = np.array([ip_to_host[int(v)] for v in s[f"dst_ip{r}"][dlv]], np.int64)
            cell = hosts["route"][s[f"src{r}"][dlv]].astype(np.int64) * n + hosts["route"][dh].astype(np.int64)
            np.add.at(counts, cell, np.uint64(1))
        out.update(counts=counts, rng=rng.copy(), ctr=ctr.copy())
        if self.packed:
            out.update(path_key=(s["lat"] << np.uint64(32)) | s["loss"].view(np.uint32).astype(np.uint64), packed=_u64(1))
        return out

    def gpu(self, h, measure=False):
        from shadow_amd import _capi
        from shadow_amd.worker import Deliveries, DeviceTable, PacketBatch, deliver_round

        hosts, _ = _deliver_world()
        a, b = self.sets()
        want = self.ref("B")
        host_keys = [k for k in want if k[:-1] in ("delivered", "min_deliver", "min_lat")] + ["rng", "ctr", "packed"]  # at return
        outs = {k: v for k, v in want.items() if k not in host_keys}
        with h.on_stream():
            ht = _host_table(hosts, h.ctx)
        n = a["lat"].shape[0]
        got = {}
        C = _capi.C

        def table(din, dout):
            t = DeviceTable(din["lat"], din["loss"], n)
            if self.packed:
                t.path_key = dout["path_key"]
            return t

        def pack(din, dout, x, warm):
            ok = C.c_uint32(0)
            t = DeviceTable(din["lat"], din["loss"], n).struct()
            _capi.check(h.ctx.handle, _capi.load().sg_table_pack(h.ctx.handle, C.byref(t), dout["path_key"].data_ptr(),
                                                                 C.byref(ok)))
            got["packed"] = _u64(ok.value)

        def set_up(din, dout, x, warm):
            ht.set_state(*self._state0())
            ht.skip(*self.SKIP)

        def round_(r):
            def fn(din, dout, x, warm):
                pb = PacketBatch(din[f"src{r}"], din[f"dst_ip{r}"], din[f"payload{r}"], din[f"send_time{r}"])
                out = Deliveries(dout[f"status{r}"], dout[f"deliver_time{r}"], dout[f"event_id{r}"], dout[f"dst_order{r}"],
                                 dout[f"dst_offsets{r}"])
                h.ctx.set_packet_counters(dout["counts"])
                try:
                    if self.stats:
                        deliver_round(ht, table(din, dout), pb, T0 + r * 10**6, 2**63, 0, out=out, ctx=h.ctx)
                        got.update({f"delivered{r}": _u64(out.n_delivered), f"min_deliver{r}": _u64(out.min_deliver_time_ns),
                                    f"min_lat{r}": _u64(out.min_used_latency_ns)})
                    else:  # stats == NULL (the wrapper always takes them)
                        t, p, d = table(din, dout).struct(), pb.c_struct(), out.c_struct()
                        rnd = _capi.sg_round(T0 + r * 10**6, 2**63, 0)
                        _capi.check(h.ctx.handle, _capi.load().sg_deliver_round(
                            h.ctx.handle, ht.handle, C.byref(t), C.byref(rnd), C.byref(p), C.byref(d), None))
                finally:
                    h.ctx.set_packet_counters(None)
            return fn

        def state(din, dout, x, warm):
            rng, ctr = ht.get_state()
            got.update(rng=rng, ctr=ctr)

        def keys(r):
            return tuple(k for k in a if k.endswith(str(r)))

        def okeys(r):
            return tuple(k for k in outs if k.endswith(str(r)))

        stages = [((), (), set_up)]
        if self.packed:
            # (the rounds then read the packed table alone: the two arrays stay B's)
            stages += [(("lat", "loss"), ("path_key",), pack), (keys(1), okeys(1) + ("counts",), round_(1)),
                       (keys(2), okeys(2), round_(2))]
        else:
            stages += [(keys(1) + ("lat", "loss"), okeys(1) + ("counts",), round_(1)),
                       (keys(2) + ("lat", "loss"), okeys(2), round_(2))]
        stages.append(((), (), state))
        # stats == NULL still synchronises once (the header says so since this test found it waiting)
        no_sync = ["syncs" if not self.stats and fn.__qualname__.endswith("round_.<locals>.fn") else False
                   for _, _, fn in stages]
        _, dev = h.run(self.name, a, b, outs, stages, measure=measure, expect_async=no_sync)
        got = dict(dev, **got)
        if not self.stats:  # the delivered counts from the bucket offsets
            got.update({f"delivered{r}": _u64(got[f"dst_offsets{r}"][-1]) for r in (1, 2)})
        return got


class ShardedCase(Case):
    """The sharded halves in one process, as test_dist_gpu.py runs them: one source rank that holds
    the whole table and every packet, two owner ranks (HostPartition over the 64 rows).
    sg_deliver_source (synchronises), sg_deliver_bucket on owner 0's records; then on a second
    host table sg_deliver_source_padded (must return while the delay still runs),
    sg_deliver_pad_to_compact and sg_deliver_bucket_padded for owner 0 (the other source rank's
    block empty).  Records are compared per owner group in packet order, and a bucketing by the
    packets it names, since neither entry point fixes the order inside a group."""
    name = "sharded_halves"
    INDEX = ("src", "dst_ip")
    SAME = ("rng",)  # one draw per packet whatever its fate
    NPK = 8000
    HOST_SIZED = ("send0", "send1", "padded0", "padded1", "compact0", "compact1", "bucket0", "bucket_padded0")

    @functools.lru_cache(None)
    def sets(self):
        from shadow_amd import synth

        hosts, tabs = _deliver_world()
        pk = synth.make_packets(self.NPK, hosts, T0, T0 + 10**6, seed=33, p_unknown_dst=0.01)
        a = dict(src=pk["src"], dst_ip=pk["dst_ip"], payload=pk["payload"], send_time=pk["send_time"], lat=tabs["A"][0],
                 loss=tabs["A"][1])
        b = dict(a, payload=((pk["payload"].astype(np.uint64) * 5 + 3) % 1400).astype(np.uint32),
                 send_time=np.minimum(pk["send_time"] + np.uint64(4321), np.uint64(T0 + 10**6 - 1)), lat=tabs["B"][0],
                 loss=tabs["B"][1])
        return a, b

    def _partition(self):
        from shadow_amd.dist import HostPartition

        hosts, _ = _deliver_world()
        return HostPartition(hosts["route"], 64, 2)

    @functools.lru_cache(None)
    def ref(self, x):
        from oracle import oracle as O

        hosts, _ = _deliver_world()
        part = self._partition()
        s = self.sets()["AB".index(x)]
        rng = np.stack([O.xoshiro_seed(int(v)) for v in hosts["seed"]]).astype(np.uint64)
        ctr = np.zeros(hosts["n"], np.uint64)
        w = O.deliver_round(T0 + 10**6, 2**63, 0, s["src"], s["dst_ip"], s["payload"], s["send_time"], hosts["ip"],
                            hosts["route"], s["lat"], s["loss"], rng, ctr)
        ip_to_host = {int(ip): i for i, ip in enumerate(hosts["ip"])}
        dlv = np.flatnonzero(w["status"] == 0)
        dst = np.array([ip_to_host[int(v)] for v in s["dst_ip"][dlv]], np.int64)
        src = s["src"][dlv].astype(np.uint64)
        k = np.arange(len(dlv)) - np.searchsorted(src, src)  # packets are grouped by source: the place among its delivered
        rec = np.zeros((len(dlv), 4), np.uint64)
        rec[:, 0], rec[:, 1], rec[:, 2] = w["deliver_time"][dlv], (src << np.uint64(32)) | k.astype(np.uint64), w["event_id"][dlv]
        rec[:, 3] = dlv.astype(np.uint64) | (dst.astype(np.uint64) << np.uint64(32))
        out = dict(status=w["status"], deliver_time=w["deliver_time"], event_id=w["event_id"], rng=rng, ctr=ctr,
                   stats=np.array([w["delivered"], w["min_deliver"], w["min_lat"]], np.uint64))
        counts = []
        for d in (0, 1):
            g = rec[part.owner[dst] == d]
            counts.append(len(g))
            out[f"send{d}"] = out[f"padded{d}"] = out[f"compact{d}"] = g
        out["counts"] = np.array(counts, np.uint64)
        mine = part.hosts_of[0].astype(np.int64)
        offs = w["dst_offsets"].astype(np.int64)
        out["bucket0"] = out["bucket_padded0"] = np.concatenate([w["dst_order"][offs[v]:offs[v + 1]] for v in mine]).astype(np.uint32)
        out["offsets0"] = out["offsets_padded0"] = np.concatenate([[0], np.cumsum(offs[mine + 1] - offs[mine])]).astype(np.uint32)
        return out

    def gpu(self, h, measure=False):
        from shadow_amd import _capi
        from shadow_amd.worker import DeviceTable, PacketBatch

        hosts, _ = _deliver_world()
        part = self._partition()
        a, b = self.sets()
        C, L, n, cap = _capi.C, _capi.load(), self.NPK, self.NPK
        H, n_local = hosts["n"], part.n_local(0)
        z = lambda k, dt: np.zeros(k, dt)  # noqa: E731
        outs = dict(status=z(n, np.uint8), deliver_time=z(n, np.uint64), event_id=z(n, np.uint64), send=z((n, 4), np.uint64),
                    order=z(n, np.uint32), offsets=z(n_local + 1, np.uint32),
                    status_p=z(n, np.uint8), deliver_time_p=z(n, np.uint64), event_id_p=z(n, np.uint64),
                    send_padded=z((2 * cap, 4), np.uint64), send_p=z((n, 4), np.uint64), xrow=z(5, np.uint64),
                    order_p=z(2 * cap, np.uint32), offsets_p=z(n_local + 1, np.uint32))
        with h.on_stream():
            hts = {(warm, k): _host_table(hosts, h.ctx) for warm in (True, False) for k in "ep"}
            owner, local = h.dev(part.owner), h.dev(part.local)
            other = h.dev(np.array([0, 2**64 - 1, 2**64 - 1, 0, 0], np.uint64))  # the second source rank: no packet
            recv_padded, xall = h.dev(z((2 * cap, 4), np.uint64)), h.dev(z(10, np.uint64))
        got = {}
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def args(din, warm, k):
            t = DeviceTable(din["lat"], din["loss"], 64).struct()
            p = PacketBatch(din["src"], din["dst_ip"], din["payload"], din["send_time"]).c_struct()
            return hts[(warm, k)].handle, t, _capi.sg_round(T0 + 10**6, 2**63, 0), p

        def source(din, dout, x, warm):
            hh, t, r, p = args(din, warm, "e")
            counts, st = (C.c_uint32 * 2)(), _capi.sg_round_stats()
            _capi.check(h.ctx.handle, L.sg_deliver_source(
                h.ctx.handle, hh, C.byref(t), C.byref(r), C.byref(p), vp(dout["status"]), vp(dout["deliver_time"]),
                vp(dout["event_id"]), vp(owner), 2, vp(dout["send"]), counts, C.byref(st)))
            got.update(counts=np.array(list(counts), np.uint64),
                       stats=np.array([st.n_delivered, st.min_deliver_time_ns, st.min_used_latency_ns], np.uint64))

        def bucket(din, dout, x, warm):
            _capi.check(h.ctx.handle, L.sg_deliver_bucket(h.ctx.handle, vp(dout["send"]), int(got["counts"][0]), vp(local), H,
                                                          n_local, vp(dout["order"]), vp(dout["offsets"])))

        def source_padded(din, dout, x, warm):
            hh, t, r, p = args(din, warm, "p")
            _capi.check(h.ctx.handle, L.sg_deliver_source_padded(
                h.ctx.handle, hh, C.byref(t), C.byref(r), C.byref(p), vp(dout["status_p"]), vp(dout["deliver_time_p"]),
                vp(dout["event_id_p"]), vp(owner), 2, cap, vp(dout["send_padded"]), vp(dout["send_p"]), vp(dout["xrow"])))

        def compact(din, dout, x, warm):
            _capi.check(h.ctx.handle, L.sg_deliver_pad_to_compact(h.ctx.handle, vp(dout["send_padded"]), 2, cap,
                                                                  vp(dout["xrow"]), vp(dout["send_p"])))

        def bucket_padded(din, dout, x, warm):
            # the exchange, for owner 0: its block from this source rank, an empty one from the other
            recv_padded[:cap * 4].copy_(dout["send_padded"][:cap * 4])
            xall[:5].copy_(dout["xrow"])
            xall[5:].copy_(other)
            st, rc, pm = _capi.sg_round_stats(), (C.c_uint32 * 2)(), C.c_uint32()
            _capi.check(h.ctx.handle, L.sg_deliver_bucket_padded(
                h.ctx.handle, vp(recv_padded), 2, cap, vp(xall), 0, vp(local), H, n_local, vp(dout["order_p"]),
                vp(dout["offsets_p"]), C.byref(st), rc, C.byref(pm)))
            if not warm:
                got.update(stats_p=np.array([st.n_delivered, st.min_deliver_time_ns, st.min_used_latency_ns], np.uint64),
                           recv_counts=list(rc), state=hts[(False, "p")].get_state())

        ins = tuple(a)
        stages = [(ins, ("status", "deliver_time", "event_id", "send"), source), ((), ("order", "offsets"), bucket),
                  (ins, ("status_p", "deliver_time_p", "event_id_p", "send_padded", "send_p", "xrow"), source_padded),
                  ((), (), compact), ((), ("order_p", "offsets_p"), bucket_padded)]
        _, dev = h.run(self.name, a, b, outs, stages, measure=measure, expect_async=[False, False, True, False, False])
        c0, c1 = (int(v) for v in got["counts"])
        assert [int(v) for v in dev["xrow"][3:]] == [c0, c1] and got["recv_counts"] == [c0, 0]
        assert np.array_equal(dev["xrow"][:3], got["stats"]) and np.array_equal(got["stats_p"], got["stats"])
        for k in ("status", "deliver_time", "event_id"):
            assert np.array_equal(dev[k], dev[k + "_p"]), f"{k}: the padded source phase differs from the exact one"
        canon = lambda r: r[np.argsort(r[:, 3] & np.uint64(0xFFFFFFFF), kind="stable")]  # noqa: E731
        out = {k: dev[k] for k in ("status", "deliver_time", "event_id")}
        out.update(send0=canon(dev["send"][:c0]), send1=canon(dev["send"][c0:c0 + c1]),
                   padded0=canon(dev["send_padded"][:c0]), padded1=canon(dev["send_padded"][cap:cap + c1]),
                   compact0=canon(dev["send_p"][:c0]), compact1=canon(dev["send_p"][c0:c0 + c1]),
                   counts=got["counts"], stats=got["stats"], rng=got["state"][0], ctr=got["state"][1])
        pkt = lambda r: (r[:, 3] & np.uint64(0xFFFFFFFF)).astype(np.uint32)  # noqa: E731
        out.update(bucket0=pkt(dev["send"])[dev["order"][:c0]], offsets0=dev["offsets"],
                   bucket_padded0=pkt(dev["send_padded"])[dev["order_p"][:c0]], offsets_padded0=dev["offsets_p"])
        return out


DELIVER_CASES = [DeliverCase(False), DeliverCase(True), DeliverCase(False, stats=False), ShardedCase()]

# ---------------------------------------------------------------------------
# the packet wire: sg_wire_push, the record forms, pop, the checkpoint
# ---------------------------------------------------------------------------
class WireCase(Case):
    """Four rounds of wire_cases.scenario on one wire, each pushed another way and popped two
    milliseconds past its round end: sg_wire_push; sg_wire_stamp_records + sg_wire_push_records; the padded pair (one
    rank, a block of cap records, the count in xall on the device); sg_wire_push with a packet id
    array.  Then sg_wire_get_state, and sg_wire_set_state of those events, shuffled, into a second
    wire.  The pushes take the oracle's deliveries (A) as device inputs: delivery has its own case.
    B keeps every index array (sources, destination buckets, the records' packet and destination)
    and has other times, event ids and lengths.  The five calls the header marks "does not
    synchronise" must return while the delay still runs."""
    name = "wire"
    ROUNDS = 4
    PAD = 16
    INDEX = tuple(f"{k}{r}" for r in range(4) for k in ("src", "dst_order", "dst_offsets")) + \
        tuple(f"{k}{r}" for r in (1, 2) for k in ("rec_key", "rec_packet", "rec_dst")) + ("packet_id3",)
    POP = ("host", "time_ns", "packet", "len", "src_host", "event_id")
    STATE = ("host", "src_host", "packet", "len", "time_ns", "event_id")
    PADDED = {k + str(r): "n" + str(r) for k in ("host", "time_ns", "packet", "len", "src_host", "event_id")
              for r in "0123"}
    SAME = ("stamp_key_hi",)
    HOST_SIZED = tuple("state_" + k for k in ("host", "src_host", "packet", "len", "time_ns", "event_id"))

    def _scenario(self):
        import wire_cases as WC
        from oracle import oracle as O

        return WC, WC.scenario(O)

    @functools.lru_cache(None)
    def sets(self):
        WC, sc = self._scenario()
        out = []
        for x in "AB":
            s = {}
            for r in range(self.ROUNDS):
                rd = sc["rounds"][r]
                pk, w = rd["pk"], rd["want"]
                time, eid, ln = w["deliver_time"], w["event_id"], pk["len"].astype(np.uint32)
                if x == "B":
                    dlv = w["status"] == 0
                    time = np.where(dlv, time + np.uint64(400_333 + 1000 * r), time)
                    eid = np.where(dlv, eid + np.uint64(5), eid)
                    ln = ((ln.astype(np.uint64) * 3 + 1) % 1500).astype(np.uint32)
                nd = w["delivered"]
                order = np.zeros(len(pk["src"]), np.uint32)
                order[:nd] = w["dst_order"]
                s.update({f"src{r}": pk["src"], f"dst_order{r}": order, f"dst_offsets{r}": w["dst_offsets"],
                          f"deliver_time{r}": time, f"event_id{r}": eid, f"len{r}": ln})
                if r in (1, 2):  # sg_record per delivered packet, as sg_deliver_source writes them for one rank
                    p = w["dst_order"].astype(np.int64)
                    dst = np.repeat(np.arange(WC.H, dtype=np.uint32), np.diff(w["dst_offsets"].astype(np.int64)))
                    src = pk["src"][p].astype(np.uint64)
                    first = np.searchsorted(pk["src"][np.sort(p)], pk["src"][p])
                    rank = np.searchsorted(np.sort(p), p) - first  # k: the place among the source's delivered packets
                    s.update({f"rec_time{r}": time[p], f"rec_key{r}": (src << np.uint64(32)) | rank.astype(np.uint64),
                              f"rec_eid{r}": eid[p], f"rec_packet{r}": p.astype(np.uint32), f"rec_dst{r}": dst})
            s["packet_id3"] = (np.arange(len(sc["rounds"][3]["pk"]["src"]), dtype=np.uint32) * np.uint32(7) + np.uint32(100_000))
            out.append(s)
        return tuple(out)

    def records(self, s, r, cap=None):
        """Round r's records as the [n, 4] u64 array of sg_record (cap: padded with zero records)."""
        n = len(s[f"rec_time{r}"])
        rec = np.zeros((cap or n, 4), np.uint64)
        rec[:n, 0], rec[:n, 1], rec[:n, 2] = s[f"rec_time{r}"], s[f"rec_key{r}"], s[f"rec_eid{r}"]
        rec[:n, 3] = s[f"rec_packet{r}"].astype(np.uint64) | (s[f"rec_dst{r}"].astype(np.uint64) << np.uint64(32))
        return rec

    def id_base(self, r):
        return 1000 * r + 7

    def window(self, sc, r):
        """Round r's pop: two milliseconds past its end, so that the first round's pop is not empty."""
        return int(sc["rounds"][r]["end"]) + 2 * 10**6

    def _cap(self, s, r):
        return len(s[f"rec_time{r}"]) + self.PAD

    @functools.lru_cache(None)
    def ref(self, x):
        import wire_ref as WR

        WC, sc = self._scenario()
        s = self.sets()["AB".index(x)]
        wire = WR.WireRef()
        cap = self.ROUNDS * WC.PER_ROUND
        out = {}
        for r in range(self.ROUNDS):
            nd = int(s[f"dst_offsets{r}"][-1])
            res = dict(dst_order=s[f"dst_order{r}"][:nd], dst_offsets=s[f"dst_offsets{r}"], deliver_time=s[f"deliver_time{r}"],
                       event_id=s[f"event_id{r}"])
            wire.push(res, s[f"src{r}"], s[f"len{r}"], packet_id=s["packet_id3"] if r == 3 else None, id_base=self.id_base(r))
            pop, nxt = wire.pop(self.window(sc, r))
            for k in self.POP:
                a = np.full(cap, poison(pop[k].dtype), pop[k].dtype)
                a[:len(pop[k])] = pop[k]
                out[f"{k}{r}"] = a
            out.update({f"n{r}": _u64(len(pop["host"])), f"next{r}": _u64(nxt)})
            if r in (1, 2):  # the stamped records: len in the key's low half, the packet id in place of the index
                rec = self.records(s, r)
                p = s[f"rec_packet{r}"].astype(np.int64)
                rec[:, 1] = (rec[:, 1] & np.uint64(0xFFFFFFFF00000000)) | s[f"len{r}"][p].astype(np.uint64)
                rec[:, 3] = (rec[:, 3] & np.uint64(0xFFFFFFFF00000000)) | (p + self.id_base(r)).astype(np.uint64)
                out[f"stamped{r}"] = rec
        st = wire.state()
        out.update({f"state_{k}": st[k] for k in self.STATE})
        out["stamp_key_hi"] = out["stamped1"][:, 1] >> np.uint64(32)
        return out

    def gpu(self, h, measure=False):
        import wire_cases as WC
        from shadow_amd import _capi, wire as W
        from shadow_amd.worker import Deliveries, PacketBatch

        _, sc = self._scenario()
        a, b = self.sets()
        want = self.ref("B")
        C = _capi.C
        cap = self.ROUNDS * WC.PER_ROUND
        ins = []
        for s in (a, b):
            d = {k: v for k, v in s.items() if not k.startswith("rec_")}
            d["rec1"] = self.records(s, 1)
            d["rec2"] = self.records(s, 2, self._cap(s, 2))
            d["xall2"] = np.array([0, 0, 0, len(s["rec_time2"])], np.uint64)
            ins.append(d)
        outs = {k: v for k, v in want.items() if k[:-1] in self.POP}
        with h.on_stream():
            # (room for the conservative counts of the pushes: a push adds its whole batch until the next pop)
            wires = {warm: W.PacketWire(WC.H, 4 * cap, WC.MS, 16, ctx=h.ctx) for warm in (True, False)}
            second = W.PacketWire(WC.H, 4 * cap, 500_000, 8, ctx=h.ctx)
            status = h.dev(np.zeros(WC.PER_ROUND, np.uint8))  # (not read by the push)
        got = {}
        L = _capi.load()
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def push(r):
            def fn(din, dout, x, warm):
                w = wires[warm]
                if r in (0, 3):
                    pb = PacketBatch(din[f"src{r}"], din[f"src{r}"], din[f"len{r}"], din[f"deliver_time{r}"])
                    out = Deliveries(status, din[f"deliver_time{r}"], din[f"event_id{r}"], din[f"dst_order{r}"],
                                     din[f"dst_offsets{r}"])
                    w.push(pb, out, din[f"len{r}"], packet_id=din["packet_id3"] if r == 3 else None, id_base=self.id_base(r))
                elif r == 1:
                    w.push_records(din["rec1"], len(a["rec_time1"]))
                else:
                    w.push_records_padded(din["rec2"], 1, self._cap(a, 2), din["xall2"], 0)
            return fn

        def stamp(r):
            def fn(din, dout, x, warm):
                npk = len(a[f"src{r}"])
                if r == 1:
                    W.stamp_records(din["rec1"], len(a["rec_time1"]), din["len1"], npk, id_base=self.id_base(1), ctx=h.ctx)
                else:  # (nothing past cap: `send` is the block itself)
                    W.stamp_records_padded(din["rec2"], din["rec2"], 1, self._cap(a, 2), din["xall2"], din["len2"], npk,
                                           id_base=self.id_base(2), ctx=h.ctx)
            return fn

        def pop(r):
            def fn(din, dout, x, warm):
                o = _capi.sg_wire_arrivals(cap, *(dout[f"{k}{r}"].data_ptr() for k in self.POP))
                n, nxt = C.c_uint32(), C.c_uint64()
                _capi.check(h.ctx.handle, L.sg_wire_pop(h.ctx.handle, wires[warm].handle, self.window(sc, r),
                                                        C.byref(o), C.byref(n), C.byref(nxt)))
                got.update({f"n{r}": _u64(n.value), f"next{r}": _u64(nxt.value)})
                if r in (1, 2) and not warm:  # (after the pop's synchronisation: the records as stamped)
                    got[f"stamped{r}"] = din[f"rec{r}"].cpu().numpy().view(np.uint64).reshape(-1, 4)[:len(a[f"rec_time{r}"])]
            return fn

        def checkpoint(din, dout, x, warm):
            st = wires[warm].get_state()
            perm = np.random.default_rng(3).permutation(len(st["host"]))
            second.set_state({k: v[perm] for k, v in st.items()})
            again = second.get_state()
            if not warm:
                got.update({f"state_{k}": st[k] for k in self.STATE})
                got["second"] = all(np.array_equal(st[k], again[k]) for k in self.STATE)

        stages, no_sync = [], []
        for r in range(self.ROUNDS):
            keys = tuple(f"{k}{r}" for k in ("deliver_time", "event_id", "len"))
            if r in (1, 2):
                stages.append((keys + (f"rec{r}",), (), stamp(r)))
                stages.append(((), (), push(r)))
                no_sync += [True, True]
            else:
                stages.append((keys, (), push(r)))
                no_sync.append(True)
            stages.append(((), tuple(f"{k}{r}" for k in self.POP), pop(r)))
            no_sync.append(False)
        stages.append(((), (), checkpoint))
        no_sync.append(False)
        _, dev = h.run(self.name, ins[0], ins[1], outs, stages, measure=measure, expect_async=no_sync)
        assert got.pop("second"), "the second wire's state after set_state differs from what was set"
        got = dict(dev, **got)
        got["stamp_key_hi"] = got["stamped1"][:, 1] >> np.uint64(32)
        return got


WIRE_CASES = [WireCase()]

# ---------------------------------------------------------------------------
# lanes: sg_codel_run, sg_inbound_run, sg_inbound_run_ordered
# ---------------------------------------------------------------------------
MS = 1_000_000


def _ascending(host, gaps, t0):
    """Per host (hosts grouped): t0 + the running sum of its own gaps."""
    c = np.cumsum(gaps.astype(np.int64))
    first = np.r_[True, host[1:] != host[:-1]]
    base = np.maximum.accumulate(np.where(first, c - gaps, 0))
    return (t0 + c - base).astype(np.uint64)


def _live(st):
    """The live ring slots [head, tail) of every host, host after host: (packets, times, lengths)."""
    cap = st["cap"]
    lo = st["head"].astype(np.int64)
    n = st["tail"].astype(np.int64) - lo
    hh = np.repeat(np.arange(len(n)), n)
    c = lo[hh] + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    i = hh * cap + (c % cap)
    return st["ring_pkt"][i], st["ring_ts"][i], st["ring_len"][i]


def _partial(a):
    """An output the library writes only where something happened (indexed by packet id): the
    zeros of the reference's own starting value are what the device leaves as poison."""
    return np.where(a == 0, poison(a.dtype), a).astype(a.dtype)


class CodelCase(Case):
    """sg_codel_run on the lane_cases shape (128 hosts, 6,078 events), two calls so that state
    carries over; then sg_codel_get_state.  A and B share hosts, kinds and packet ids; times (per
    host ascending in both) and lengths differ."""
    name = "codel_run"
    INDEX = ("host", "kind1", "kind2", "pkt1", "pkt2")
    PARTIAL = ("status",)
    SAME = ("state_tail",)  # a ring's tail counts its host's pushes
    HOST_SIZED = ("ring_pkt", "ring_ts", "ring_len")
    CODEL_KEYS = ("flags", "interval_end", "drop_next", "cur", "prev", "bytes", "head", "tail")

    @functools.lru_cache(None)
    def sets(self):
        import lane_cases

        host = lane_cases.host_column()
        E = len(host)
        out = []
        for x in "AB":
            rng = np.random.default_rng(31)
            vals = np.random.default_rng(31 if x == "A" else 32)
            s = dict(host=host)
            t0 = T0 + 10**9
            for c in (1, 2):
                s[f"kind{c}"] = (rng.random(E) < 0.45).astype(np.uint8)
                s[f"time{c}"] = _ascending(host, vals.integers(0, 3 * MS, E), t0)
                s[f"pkt{c}"] = ((c - 1) * E + np.arange(E)).astype(np.uint32)
                s[f"len{c}"] = vals.integers(40, 1500, E).astype(np.uint32)
                t0 += 3 * MS * 3001
            out.append(s)
        return tuple(out)

    @functools.lru_cache(None)
    def ref(self, x):
        import lane_cases
        from oracle import oracle as O

        s = self.sets()["AB".index(x)]
        E = len(s["host"])
        st = O.codel_state(lane_cases.H, lane_cases.RING_CAP)
        stat = np.zeros(2 * E, np.uint8)
        out = {}
        for c in (1, 2):
            before = int((stat == 2).sum())
            out[f"res{c}"] = O.codel_run(st, s["host"], s[f"kind{c}"], s[f"time{c}"], s[f"pkt{c}"], s[f"len{c}"], stat).copy()
            out[f"drops{c}"] = _u64(int((stat == 2).sum()) - before)
        out["status"] = _partial(stat)
        out.update({"state_" + k: st[k].copy() for k in self.CODEL_KEYS})
        out.update(zip(("ring_pkt", "ring_ts", "ring_len"), _live(st)))
        return out

    def gpu(self, h, measure=False):
        import lane_cases
        from shadow_amd.router import CoDelEvents, CoDelQueues

        a, b = self.sets()
        want = self.ref("B")
        with h.on_stream():
            qs = {warm: CoDelQueues(lane_cases.H, lane_cases.RING_CAP, ctx=h.ctx) for warm in (True, False)}
        got = {}
        E = len(a["host"])

        def run(c):
            def fn(din, dout, x, warm):
                ev = CoDelEvents(din["host"], din[f"kind{c}"], din[f"time{c}"], din[f"pkt{c}"], din[f"len{c}"])
                e = _capi_events(ev, E)
                from shadow_amd import _capi
                nd = _capi.C.c_uint64()
                _capi.check(h.ctx.handle, _capi.load().sg_codel_run(h.ctx.handle, qs[warm].handle, _capi.C.byref(e),
                                                                    dout[f"res{c}"].data_ptr(), dout["status"].data_ptr(),
                                                                    2 * E, _capi.C.byref(nd)))
                got[f"drops{c}"] = _u64(nd.value)
            return fn

        def state(din, dout, x, warm):
            st = qs[warm].get_state()
            got.update({"state_" + k: st[k] for k in self.CODEL_KEYS})
            got.update(zip(("ring_pkt", "ring_ts", "ring_len"), _live(st)))

        outs = {k: want[k] for k in ("res1", "res2", "status")}
        stages = [(("time1", "len1"), ("res1", "status"), run(1)), (("time2", "len2"), ("res2",), run(2)), ((), (), state)]
        _, dev = h.run(self.name, a, b, outs, stages, measure=measure)
        return dict(dev, **got)


def _capi_events(ev, n):
    from shadow_amd import _capi

    return _capi.sg_codel_events(n, ev.host.data_ptr(), ev.kind.data_ptr(), ev.time_ns.data_ptr(), ev.packet.data_ptr(),
                                 ev.length.data_ptr())


class InboundCase(Case):
    """sg_inbound_run / sg_inbound_run_ordered on the lane_cases shape: two windows of 60 ms through
    1 Mbit/s relays (200 Mbit/s at the long host), so queues stand, CoDel drops and forward tasks
    stay pending across the calls; event ids from a device counter array; then
    sg_inbound_get_state.  The ordered call's per-arrival fates are scattered to packet ids on
    the host, as test_inbound_gpu.py does on the device, so both forms compare with the oracle's
    arrays by packet id.  A and B share hosts and packet ids; times and lengths differ."""
    INDEX = ("host", "pkt1", "pkt2")
    PARTIAL = ("status", "fwd")
    # the tail counts the host's arrivals; the buckets' sizes follow from the bandwidths; every relay
    # ends the second window in the same mode under either set
    SAME = ("state_tail", "state_tb_cap", "state_tb_inc", "state_rflags")
    HOST_SIZED = ("ring_pkt", "ring_ts", "ring_len")
    KEYS = CodelCase.CODEL_KEYS + ("rflags", "task_time", "task_id", "task_born", "tb_cap", "tb_bal", "tb_inc", "tb_last")

    def __init__(self, ordered):
        self.ordered = ordered
        self.name = "inbound_run" + ("_ordered" if ordered else "")

    def _bw(self):
        import lane_cases

        bw = np.full(lane_cases.H, 10**6, np.uint64)
        bw[64] = 200 * 10**6
        return bw

    @functools.lru_cache(None)
    def sets(self):
        import lane_cases

        host = lane_cases.host_column()
        E = len(host)
        out = []
        for x in "AB":
            rng = np.random.default_rng(43 if x == "A" else 44)
            s = dict(host=host)
            for c in (1, 2):
                t = rng.integers(T0 + (c - 1) * 60 * MS, T0 + c * 60 * MS, E).astype(np.uint64)
                s[f"time{c}"] = t[np.lexsort((t, host))]
                s[f"pkt{c}"] = ((c - 1) * E + np.arange(E)).astype(np.uint32)
                s[f"len{c}"] = rng.choice(np.array([28, 1476, 600], np.uint32), E)
            out.append(s)
        return tuple(out)

    @functools.lru_cache(None)
    def ref(self, x):
        import lane_cases
        from oracle import oracle as O

        s = self.sets()["AB".index(x)]
        E = len(s["host"])
        st = O.inbound_state(self._bw(), lane_cases.RING_CAP)
        fwd, stat, ctr = np.full(2 * E, np.uint64(2**64 - 1)), np.zeros(2 * E, np.uint8), np.zeros(lane_cases.H, np.uint64)
        for c in (1, 2):
            O.inbound_run(st, s["host"], s[f"time{c}"], s[f"pkt{c}"], s[f"len{c}"], T0 + c * 60 * MS, 0, T0 + 10**12, ctr, fwd,
                          stat)
        out = dict(status=_partial(stat), fwd=np.where(stat == 1, fwd, poison(np.uint64)), ctr=ctr,
                   drops=_u64(int((stat == 2).sum())))
        out.update({"state_" + k: st[k].copy() for k in self.KEYS})
        out.update(zip(("ring_pkt", "ring_ts", "ring_len"), _live(st)))
        return out

    def gpu(self, h, measure=False):
        import lane_cases
        from shadow_amd.router import InboundPipeline

        a, b = self.sets()
        want = self.ref("B")
        E = len(a["host"])
        with h.on_stream():
            ibs = {warm: InboundPipeline(self._bw(), lane_cases.RING_CAP, ctx=h.ctx) for warm in (True, False)}
        got = {"drops": 0}

        def run(c):
            def fn(din, dout, x, warm):
                args = (din["host"], din[f"time{c}"], din[f"pkt{c}"], din[f"len{c}"], T0 + c * 60 * MS, 0, T0 + 10**12,
                        dout["fwd"], dout["status"])
                if self.ordered:
                    nd = ibs[warm].run_ordered(*args, dout[f"a_fwd{c}"], dout[f"a_st{c}"], dout["ctr"].data_ptr())
                else:
                    nd = ibs[warm].run(*args, dout["ctr"].data_ptr())
                if not warm:
                    got["drops"] += nd
            return fn

        def state(din, dout, x, warm):
            st = ibs[warm].get_state()
            got.update({"state_" + k: st[k] for k in self.KEYS})
            got.update(zip(("ring_pkt", "ring_ts", "ring_len"), _live(st)))

        outs = dict(status=want["status"], fwd=want["fwd"], ctr=want["ctr"])
        arr = {}
        if self.ordered:
            for c in (1, 2):
                arr[f"a_fwd{c}"], arr[f"a_st{c}"] = np.zeros(E, np.uint64), np.zeros(E, np.uint8)
        outs.update(arr)
        # the event counters are read and advanced: zeroed, not poisoned; a_st: "zeroed by the caller"
        stages = [(("time1", "len1"), ("status", "fwd") + (("a_fwd1",) if self.ordered else ()), run(1),
                   ("ctr",) + (("a_st1",) if self.ordered else ())),
                  (("time2", "len2"), ("a_fwd2",) if self.ordered else (), run(2), ("a_st2",) if self.ordered else ()),
                  ((), (), state)]
        _, dev = h.run(self.name, a, b, outs, stages, measure=measure)
        status, fwd = dev["status"], dev["fwd"]
        if self.ordered:  # this call's arrivals report in arrival order: scatter them to their packet ids
            for c in (1, 2):
                p = a[f"pkt{c}"].astype(np.int64)
                a_st, a_fwd = dev.pop(f"a_st{c}"), dev.pop(f"a_fwd{c}")
                left = a_st != 0
                status[p[left]] = a_st[left]
                done = left & (a_st == 1)
                fwd[p[done]] = a_fwd[done]
        dev["fwd"] = np.where(status == 1, fwd, poison(np.uint64))
        return dict(dev, drops=_u64(got.pop("drops")), **got)


class OutboundCase(Case):
    """sg_outbound_run, or sg_outbound_run_qdisc on a fifo pipeline made by
    sg_outbound_create_qdisc (the socket array is given and ignored), on the lane_cases shape: two
    windows of 60 ms through 2 Mbit/s relays (400 Mbit/s at the long host), so packets stay queued
    and cached and tasks pending; the sent batch into device arrays of the call's capacity; then
    sg_outbound_get_state.  A and B share hosts, packet ids and destination addresses; times,
    lengths and payloads differ."""
    INDEX = ("host", "pkt1", "pkt2", "dst1", "dst2", "socket")
    PARTIAL = ("status", "fwd")
    SENT = ("src_host", "dst_ipv4", "payload_len", "send_time", "packet")
    PADDED = {k + c: "n_sent" + c for k in ("src_host", "dst_ipv4", "payload_len", "send_time", "packet") for c in "12"}
    SAME = ("state_tail", "state_tb_cap", "state_tb_inc")
    HOST_SIZED = ("ring_pkt", "ring_len", "ring_pay", "ring_dst")
    KEYS = ("head", "tail", "rflags", "task_time", "task_id", "task_born", "tb_cap", "tb_bal", "tb_inc", "tb_last")

    QKEYS = ("n_active", "n_queued", "cached_packet", "cached_len", "cached_payload_len", "cached_dst")

    def __init__(self, qdisc):
        """qdisc: None (sg_outbound_create / sg_outbound_run), "fifo" or "round-robin" (the qdisc
        pair; the round-robin pipeline against tests/qdisc_ref.py, four sockets a host, its state
        through sg_outbound_get_qdisc_state in canonical form)."""
        self.qdisc = qdisc
        self.rr = qdisc == "round-robin"
        self.name = "outbound_run" + ("_qdisc_" + qdisc.replace("-", "_") if qdisc else "")
        if self.rr:
            # (every busy host ends with all four sockets queued under either set)
            self.SAME = ("state_tb_cap", "state_tb_inc", "state_n_active")
            self.HOST_SIZED = ("active", "active_count", "q_packet", "q_len", "q_payload_len", "q_dst")

    def _canon(self, st, S, cap):
        """The written part of every per-host list of a canonical qdisc state."""
        na, nq = st["n_active"].astype(np.int64), st["n_queued"].astype(np.int64)
        ia = np.repeat(np.arange(len(na)) * S, na) + np.arange(int(na.sum())) - np.repeat(np.cumsum(na) - na, na)
        iq = np.repeat(np.arange(len(nq)) * cap, nq) + np.arange(int(nq.sum())) - np.repeat(np.cumsum(nq) - nq, nq)
        out = {"state_" + k: st[k] for k in self.QKEYS}
        out.update({k: st[k][ia] for k in ("active", "active_count")})
        out.update({k: st[k][iq] for k in ("q_packet", "q_len", "q_payload_len", "q_dst")})
        return out

    def _world(self):
        import lane_cases
        from shadow_amd import synth

        hosts = synth.make_hosts(lane_cases.H, 64, exact_seeds=False)
        bw = np.full(lane_cases.H, 2 * 10**6, np.uint64)
        bw[64] = 400 * 10**6
        return hosts, bw

    @functools.lru_cache(None)
    def sets(self):
        import lane_cases
        from shadow_amd import synth

        hosts, _ = self._world()
        src = lane_cases.host_column()
        E = len(src)
        out = []
        for x in "AB":
            s = dict(host=src, socket=(np.arange(E, dtype=np.uint32) % np.uint32(4)))
            for c in (1, 2):
                pk = synth.make_packets(E, hosts, T0 + (c - 1) * 60 * MS, T0 + c * 60 * MS, seed=70 + c)
                pkv = pk if x == "A" else synth.make_packets(E, hosts, T0 + (c - 1) * 60 * MS, T0 + c * 60 * MS, seed=90 + c)
                loc = np.random.default_rng(1070 + c).random(E) < 0.05
                s[f"time{c}"] = pkv["send_time"][np.lexsort((pkv["send_time"], src))]
                s[f"pkt{c}"] = ((c - 1) * E + np.arange(E)).astype(np.uint32)
                s[f"payload{c}"] = pkv["payload"].astype(np.uint32)
                s[f"len{c}"] = (pkv["payload"] + 40).astype(np.uint32)
                s[f"dst{c}"] = np.where(loc, hosts["ip"][src], pk["dst_ip"]).astype(np.uint32)
            out.append(s)
        return tuple(out)

    def _live(self, st):
        c = st["cap"]
        lo = st["head"].astype(np.int64) - ((st["rflags"] & 4) != 0)
        n = st["tail"].astype(np.int64) - lo
        hh = np.repeat(np.arange(len(n)), n)
        k = lo[hh] + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
        i = hh * c + (k % c)
        return {key: st[key][i] for key in ("ring_pkt", "ring_len", "ring_pay", "ring_dst")}

    def _cap(self):
        import lane_cases

        return len(lane_cases.host_column()) * 2 + lane_cases.H * 4

    @functools.lru_cache(None)
    def ref(self, x):
        import lane_cases
        from oracle import oracle as O

        hosts, bw = self._world()
        s = self.sets()["AB".index(x)]
        E = len(s["host"])
        st = O.outbound_state(hosts["ip"], bw, lane_cases.RING_CAP)
        fwd, stat, ctr = np.full(2 * E, np.uint64(2**64 - 1)), np.zeros(2 * E, np.uint8), np.zeros(lane_cases.H, np.uint64)
        out = {}
        if self.rr:
            import qdisc_ref as QD

            model = QD.Interfaces(hosts["ip"], bw, lane_cases.RING_CAP, QD.ROUND_ROBIN, 4)
        for c in (1, 2):
            if self.rr:
                w = model.run(s["host"], s[f"time{c}"], s[f"pkt{c}"], s[f"len{c}"], s[f"payload{c}"], s[f"dst{c}"],
                              s["socket"], T0 + c * 60 * MS, 0, T0 + 10**12, ctr, fwd, stat)
            else:
                w = O.outbound_run(st, s["host"], s[f"time{c}"], s[f"pkt{c}"], s[f"len{c}"], s[f"payload{c}"],
                                   s[f"dst{c}"], T0 + c * 60 * MS, 0, T0 + 10**12, ctr, fwd, stat)
            out[f"n_sent{c}"] = _u64(len(w["packet"]))
            for k in self.SENT:
                a = np.full(self._cap(), poison(w[k].dtype), w[k].dtype)
                a[:len(w[k])] = w[k]
                out[f"{k}{c}"] = a
        out.update(status=_partial(stat), fwd=np.where(stat != 0, fwd, poison(np.uint64)), ctr=ctr)
        if self.rr:
            out.update({"state_" + k: v for k, v in model.relay_state().items()})
            out.update(self._canon(model.qdisc_state(), model.S, model.cap))
            return out
        out.update({"state_" + k: st[k].copy() for k in self.KEYS})
        out.update(self._live(st))
        return out

    def gpu(self, h, measure=False):
        import lane_cases
        from shadow_amd import _capi
        from shadow_amd.router import OutboundPipeline

        hosts, bw = self._world()
        a, b = self.sets()
        want = self.ref("B")
        E, cap = len(a["host"]), self._cap()
        C, L = _capi.C, _capi.load()
        kw = dict(qdisc=self.qdisc, max_sockets=4) if self.qdisc else {}
        with h.on_stream():
            obs = {warm: OutboundPipeline(hosts["ip"], bw, lane_cases.RING_CAP, ctx=h.ctx, **kw) for warm in (True, False)}
        got = {}

        def run(c):
            def fn(din, dout, x, warm):
                sends = _capi.sg_outbound_sends(E, din["host"].data_ptr(), din[f"time{c}"].data_ptr(), din[f"pkt{c}"].data_ptr(),
                                                din[f"len{c}"].data_ptr(), din[f"payload{c}"].data_ptr(),
                                                din[f"dst{c}"].data_ptr(), None, None)
                sent = _capi.sg_outbound_sent(cap, *(dout[f"{k}{c}"].data_ptr() for k in self.SENT))
                ns = C.c_uint32()
                rest = (T0 + c * 60 * MS, 0, T0 + 10**12, C.c_void_p(dout["ctr"].data_ptr()), dout["fwd"].data_ptr(),
                        dout["status"].data_ptr(), 2 * E, C.byref(sent), C.byref(ns))
                if self.qdisc:
                    rc = L.sg_outbound_run_qdisc(h.ctx.handle, obs[warm].handle, C.byref(sends),
                                                 C.c_void_p(din["socket"].data_ptr()), *rest)
                else:
                    rc = L.sg_outbound_run(h.ctx.handle, obs[warm].handle, C.byref(sends), *rest)
                _capi.check(h.ctx.handle, rc)
                got[f"n_sent{c}"] = _u64(ns.value)
            return fn

        def state(din, dout, x, warm):
            if self.rr:
                st = obs[warm].get_qdisc_state()
                got.update({"state_" + k: st[k] for k in self.KEYS if k not in ("head", "tail")})
                got.update(self._canon(st, obs[warm].max_sockets, obs[warm].cap))
                return
            st = obs[warm].get_state()
            got.update({"state_" + k: st[k] for k in self.KEYS})
            got.update(self._live(st))

        outs = {k: v for k, v in want.items() if k in ("status", "fwd", "ctr") or k[:-1] in self.SENT}
        sent = lambda c: tuple(k + str(c) for k in self.SENT)  # noqa: E731
        # (the event counters are read and advanced: zeroed, not poisoned)
        stages = [(("time1", "len1", "payload1"), ("status", "fwd") + sent(1), run(1), ("ctr",)),
                  (("time2", "len2", "payload2"), sent(2), run(2)), ((), (), state)]
        _, dev = h.run(self.name, a, b, outs, stages, measure=measure)
        dev["fwd"] = np.where(dev["status"] != ST_POISON8, dev["fwd"], poison(np.uint64))
        return dict(dev, **got)


ST_POISON8 = np.uint8(POISON_BYTE)

LANE_CASES = [CodelCase(), InboundCase(False), InboundCase(True), OutboundCase(None), OutboundCase("fifo"),
              OutboundCase("round-robin")]

LINK_CASES = [LinkLoadCase(), LinkLoadPacketsCase(), TreePathsCase(), TreePathsPacketsCase(), LinkTraceCase(),
              LinkSeriesCase(), LinkQueueCase()]
TREE_CASES = [TreeCase(1), TreeCase(0), BuildTreeCase(1), BuildTreeCase(0)]
ALL_CASES = BUILD_CASES + TREE_CASES + LINK_CASES + DELIVER_CASES + WIRE_CASES + LANE_CASES


# ---------------------------------------------------------------------------
# every entry point of include/shadow_gpu.h: the case that runs it on the caller's stream, or why
# none does (test_stream_cases_cpu.py holds this list against shadow_amd._capi.EXPORTED)
# ---------------------------------------------------------------------------
HOST_ONLY = "host only: no device work"
GROUP = "out of scope: a group owns several streams (test_group_gpu.py has the exchange's ordering test)"
COMM = "out of scope: sg_comm_* own their streams"
COVERAGE = {
    "sg_abi_version": HOST_ONLY, "sg_ctx_create": "every case (Harness)", "sg_ctx_destroy": "every case (Harness.close)",
    "sg_ctx_set_stream": "every case (Harness)", "sg_ctx_stream": HOST_ONLY,
    "sg_ctx_synchronize": "not called: the cases synchronise S itself", "sg_ctx_last_error": HOST_ONLY,
    "sg_ctx_last_error_pair": HOST_ONLY,
    "sg_ctx_enable_timers": "not run: timers turn the plan's side stream off (BuildCase); test_routing_gpu.py runs them",
    "sg_ctx_read_timer": "as sg_ctx_enable_timers",
    "sg_gml_parse": HOST_ONLY, "sg_gml_parse_threads": HOST_ONLY, "sg_gml_load": HOST_ONLY, "sg_gml_graph": HOST_ONLY,
    "sg_gml_node_index": HOST_ONLY, "sg_gml_destroy": HOST_ONLY,
    "sg_net_create": "build_sparse_lds_one_shot_fused1 (inside the call); every graph case (set-up)",
    "sg_net_destroy": "build_sparse_lds_one_shot_fused1", "sg_routing_build": "build_sparse_lds",
    "sg_routing_min_latency": "routing_min_latency",
    "sg_hosts_create": "deliver_two_array (set-up)", "sg_hosts_get_state": "deliver_two_array",
    "sg_hosts_set_state": "deliver_two_array", "sg_hosts_skip": "deliver_two_array", "sg_hosts_destroy": "deliver_two_array",
    "sg_deliver_round": "deliver_two_array", "sg_deliver_source": "sharded_halves", "sg_deliver_bucket": "sharded_halves",
    "sg_deliver_source_padded": "sharded_halves", "sg_deliver_bucket_padded": "sharded_halves",
    "sg_deliver_pad_to_compact": "sharded_halves", "sg_table_pack": "deliver_path_key",
    "sg_codel_create": "codel_run (set-up)", "sg_codel_destroy": "codel_run", "sg_codel_run": "codel_run",
    "sg_codel_ring_cap": HOST_ONLY, "sg_codel_get_state": "codel_run",
    "sg_codel_set_state": "not covered: a host-to-device copy of the state, left for a later case",
    "sg_inbound_create": "inbound_run (set-up)", "sg_inbound_destroy": "inbound_run", "sg_inbound_ring_cap": HOST_ONLY,
    "sg_inbound_run": "inbound_run", "sg_inbound_run_ordered": "inbound_run_ordered",
    "sg_ctx_set_packet_counters": "deliver_two_array", "sg_inbound_get_state": "inbound_run", "sg_hosts_event_ctr": HOST_ONLY,
    "sg_outbound_create": "outbound_run (set-up)", "sg_outbound_destroy": "outbound_run", "sg_outbound_ring_cap": HOST_ONLY,
    "sg_outbound_run": "outbound_run", "sg_outbound_get_state": "outbound_run",
    "sg_outbound_create_qdisc": "outbound_run_qdisc_fifo (set-up)", "sg_outbound_qdisc": HOST_ONLY,
    "sg_outbound_max_sockets": HOST_ONLY,
    "sg_outbound_run_qdisc": "outbound_run_qdisc_round_robin (and outbound_run_qdisc_fifo)",
    "sg_outbound_get_qdisc_state": "outbound_run_qdisc_round_robin",
    "sg_routing_info_create": HOST_ONLY, "sg_routing_info_destroy": HOST_ONLY, "sg_routing_info_fill": "routing_info_fill",
    "sg_routing_info_set_rows": HOST_ONLY, "sg_routing_info_view": HOST_ONLY, "sg_routing_info_rows": HOST_ONLY,
    "sg_routing_info_index": HOST_ONLY, "sg_routing_info_path": HOST_ONLY, "sg_routing_info_smallest_latency": HOST_ONLY,
    "sg_routing_info_increment_packet_count": HOST_ONLY, "sg_routing_info_packet_count": HOST_ONLY,
    "sg_routing_info_set_addresses": HOST_ONLY, "sg_worker_get_latency": HOST_ONLY, "sg_worker_get_reliability": HOST_ONLY,
    "sg_worker_is_routable": HOST_ONLY,
    "sg_comm_unique_id": COMM, "sg_comm_create": COMM, "sg_comm_destroy": COMM, "sg_comm_allgather_rows": COMM,
    "sg_comm_exchange_padded": COMM, "sg_comm_alltoallv_records": COMM, "sg_comm_allgather_u64": COMM,
    "sg_wire_create": "wire (set-up)", "sg_wire_destroy": "wire", "sg_wire_count": HOST_ONLY, "sg_wire_push": "wire",
    "sg_wire_pop": "wire", "sg_wire_get_state": "wire", "sg_wire_set_state": "wire", "sg_wire_stamp_records": "wire",
    "sg_wire_stamp_records_padded": "wire", "sg_wire_push_records": "wire", "sg_wire_push_records_padded": "wire",
    "sg_group_create": GROUP, "sg_group_destroy": GROUP, "sg_group_size": GROUP, "sg_group_last_error": GROUP,
    "sg_group_last_error_pair": GROUP, "sg_group_routing_info_fill": GROUP, "sg_group_exchange_padded": GROUP,
    "sg_group_alltoallv_records": GROUP, "sg_group_last_error_member": GROUP, "sg_group_link_load_packets": GROUP,
    "sg_group_link_trace_packets": GROUP, "sg_group_link_series_packets": GROUP,
    "sg_routing_tree": "tree_lds1", "sg_routing_build_tree": "build_tree_lds1", "sg_tree_path": HOST_ONLY,
    "sg_net_links": "link_load (set-up)", "sg_net_edge_links": "not covered: a device-to-host copy of link numbers",
    "sg_link_load": "link_load", "sg_link_load_packets": "link_load_packets", "sg_tree_paths": "tree_paths",
    "sg_tree_paths_packets": "tree_paths_packets", "sg_link_trace_packets": "link_trace_packets",
    "sg_link_series_packets": "link_series_packets", "sg_link_queue": "link_queue",
}
# the calls include/shadow_gpu.h marks "does not synchronise", each held to it by the case named
# (S.query() is false at return).  sg_deliver_round with stats == NULL was on this list until
# deliver_two_array_no_stats found it waiting; the header now says that it synchronises.
NO_SYNC = {"sg_deliver_source_padded": "sharded_halves", "sg_wire_push": "wire", "sg_wire_stamp_records": "wire",
           "sg_wire_stamp_records_padded": "wire", "sg_wire_push_records": "wire", "sg_wire_push_records_padded": "wire"}
