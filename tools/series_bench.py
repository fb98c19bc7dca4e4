"""A round's link time series at C3 (sg_link_series_packets) beside the walk that is its floor
(sg_link_load_packets, plain, link loads only) and the trace it replaces (sg_link_trace_packets:
count + fill + sort on the same batch and watch set).

    python tools/series_bench.py            # JSON to profiles/series_bench.json

One process on one GPU; any failure ends it, so nothing is started on the GPU after one.  The C3
table (10k x 10k) with its pred rows on the device, a host per node; per batch one delivery round
gives the statuses, weights are the payloads.  64 bins from the round's start; the legs:
  all        1M uniform packets, every link its own slot (n_links x 64 cells: the global form), a
             bin of 1,000,000 ns (the reciprocal) and of 2^20 ns (the shift);
  watch16    the same batch, the 16 busiest links in 16 slots: the LDS form and SG_LINK_SERIES_LDS=0;
  hot        the 512-spoke star, 100k packets from one spoke across the hub, that spoke's links among
             16 slots: both forms;
  small      10k and 100k uniform packets, every link and the 16 busiest, the default form.
The legs are alternated `--runs` times; inside a run every leg is timed `--reps` times with the
library's timers and gives its median.  Reported per leg: the median over the runs of each run's
median kernel time and the spread (max - min over the runs), the same for the link-load walk and
the trace's three kernels.  Every leg asserts that its forms agree, bit for bit, and that the
identity with sg_link_load_packets holds on the device.  Correctness is tests/test_series_gpu.py's;
bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T0 = 946684800 * 10**9
N_BINS = 64
TRACE_TIMERS = ("link_trace_count", "link_trace_fill", "link_trace_sort")


def star_graph(spokes=512):
    n = spokes + 1
    v, sp = np.arange(n), np.arange(1, n)
    return dict(n=n, src=np.concatenate([v, np.zeros(spokes, np.int64), sp]).astype(np.uint32),
                dst=np.concatenate([v, sp, np.where(sp == spokes, 1, sp + 1)]).astype(np.uint32),
                lat=np.concatenate([np.full(n, 1_000_000), np.full(spokes, 1_000_000), np.full(spokes, 5_000_000)]).astype(np.uint64),
                loss=np.zeros(n + 2 * spokes, np.float32), directed=False)


class World:
    """A graph with its table and pred rows on the device and a host per node."""

    def __init__(self, g, ctx):
        import torch

        from shadow_amd import NetworkGraph, synth
        from shadow_amd.worker import DeviceTable, HostTable

        self.ctx, self.n = ctx, g["n"]
        n = self.n
        self.net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
        self.nodes = np.arange(n, dtype=np.uint32)
        self.lat = torch.empty((n, n), dtype=torch.int64, device="cuda")
        self.loss = torch.empty((n, n), dtype=torch.float32, device="cuda")
        self.pred = torch.empty((n, n), dtype=torch.int32, device="cuda")
        self.net.build_rows_device(self.nodes, 0, n, self.lat.data_ptr(), self.loss.data_ptr())
        self.net.tree_rows_device(self.nodes, 0, n, self.lat.data_ptr(), self.loss.data_ptr(), self.pred.data_ptr(), 0)
        self.table = DeviceTable(self.lat.ravel(), self.loss.ravel(), n)
        self.hosts = synth.make_hosts(n, n, exact_seeds=False)
        self.ht = HostTable(self.hosts["ip"], self.hosts["route"], self.hosts["seed"], ctx=ctx)
        self.n_links = len(self.net.links()[0])


class Batch:
    """One round's packets with their statuses, the link loads (bytes) and the 16 busiest links."""

    def __init__(self, w, src, dst):
        import torch

        from shadow_amd.worker import Deliveries, PacketBatch, deliver_round

        n = w.n
        dst = np.where(dst == src, (dst + 1) % n, dst)  # (no host sends to itself)
        order = np.argsort(src, kind="stable")
        src, dst = src[order].astype(np.uint32), dst[order]
        self.w, self.P = w, len(src)
        rs = np.random.default_rng(5)
        self.pb = PacketBatch.from_numpy(src, w.hosts["ip"][dst], np.where(rs.random(self.P) < 0.2, 0, 1448).astype(np.uint32),
                                         np.sort(rs.integers(T0, T0 + 10**6, self.P)).astype(np.uint64))
        self.out = Deliveries.allocate(self.P, n)
        deliver_round(w.ht, w.table, self.pb, T0 + 10**6, 2**63, 0, out=self.out, ctx=w.ctx)
        self.st = self.out.status.data_ptr()
        self.wt = self.pb.payload_len.data_ptr()
        self.load = torch.zeros(w.n_links, dtype=torch.int64, device="cuda")
        self.walk()
        torch.cuda.synchronize()
        self.want = self.load.clone()
        busiest = torch.argsort(self.load, descending=True, stable=True)[:16]
        self.slot16 = torch.full((w.n_links,), -1, dtype=torch.int32, device="cuda")  # (0xFFFFFFFF)
        self.slot16[busiest] = torch.arange(16, dtype=torch.int32, device="cuda")
        self.watch16 = (self.slot16 >= 0).to(torch.uint8)
        self.cap = None

    def walk(self):
        """The floor: the plain per-packet walk with out_link_load only (SG_LINK_COMBINE=0 is set)."""
        w = self.w
        self.load.zero_()
        w.net.link_load_packets_device(w.ht, w.nodes, 0, w.n, w.pred.data_ptr(), self.pb, self.st, self.wt, self.load.data_ptr(), 0, 0)

    def series(self, watched, bin_ns, out):
        w = self.w
        out[0].zero_()
        out[1].zero_()
        w.net.link_series_packets_device(w.ht, w.nodes, 0, w.n, w.pred.data_ptr(), w.lat.data_ptr(), self.pb, self.st, self.wt,
                                         self.slot16.data_ptr() if watched else 0, 16 if watched else w.n_links, 0, T0, bin_ns,
                                         N_BINS, out[0].data_ptr(), out[1].data_ptr())

    def trace(self, watched, bufs):
        w = self.w
        return w.net.link_trace_packets_device(w.ht, w.nodes, 0, w.n, w.pred.data_ptr(), w.lat.data_ptr(), self.pb, self.st,
                                               self.watch16.data_ptr() if watched else 0, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                               bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), bufs[1].numel())[1]


def timed(ctx, call, timers):
    import torch

    torch.cuda.synchronize()
    ctx.enable_timers(True)
    try:
        call()
        got = [ctx.read_timer(k) for k in timers]
    finally:
        ctx.enable_timers(False)
    assert all(launches == 1 for _, launches, _ in got), got
    return sum(ms for ms, _, _ in got)


def main():
    import torch

    from shadow_amd import default_context, synth

    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_bench.json"))
    a = p.parse_args()
    assert a.runs >= 5 and a.reps >= 3
    os.environ["SG_LINK_COMBINE"] = "0"  # the floor is the plain walk
    ctx = default_context(0)
    c3 = World(synth.ring_chords_graph(a.nodes, 8.0, seed=1), ctx)
    star = World(star_graph(), ctx)
    rs = np.random.default_rng(4)
    n = c3.n
    batches = {P: Batch(c3, rs.integers(0, n, P), rs.integers(0, n, P)) for P in (10_000, 100_000, 1_000_000)}
    hot = Batch(star, np.ones(100_000, np.int64), rs.integers(3, 512, 100_000))

    # (name, batch, watched, bin_ns, SG_LINK_SERIES_LDS or None)
    legs = [("all, 1M, 1,000,000 ns bins (reciprocal)", batches[1_000_000], False, 1_000_000, None),
            ("all, 1M, 2^20 ns bins (shift)", batches[1_000_000], False, 1 << 20, None),
            ("watch16, 1M, LDS", batches[1_000_000], True, 1_000_000, None),
            ("watch16, 1M, global", batches[1_000_000], True, 1_000_000, "0"),
            ("hot link, 100k, LDS", hot, True, 1_000_000, None),
            ("hot link, 100k, global", hot, True, 1_000_000, "0")]
    for P in (10_000, 100_000):
        legs += [(f"all, {P}", batches[P], False, 1_000_000, None), (f"watch16, {P}, LDS", batches[P], True, 1_000_000, None),
                 (f"watch16, {P}, global", batches[P], True, 1_000_000, "0")]

    outs, tbufs, sums = {}, {}, {}
    for b in list(batches.values()) + [hot]:
        for watched in (False, True):
            ns = 16 if watched else b.w.n_links
            outs[id(b), watched] = (torch.zeros((ns, N_BINS), dtype=torch.int64, device="cuda"),
                                    torch.zeros((ns, 2), dtype=torch.int64, device="cuda"))
            one = torch.zeros(2, dtype=torch.int64, device="cuda")
            loff = torch.zeros(b.w.n_links + 1, dtype=torch.int64, device="cuda")
            total = b.w.net.link_trace_packets_device(b.w.ht, b.w.nodes, 0, b.w.n, b.w.pred.data_ptr(), b.w.lat.data_ptr(), b.pb,
                                                      b.st, b.watch16.data_ptr() if watched else 0, loff.data_ptr(), one.data_ptr(),
                                                      one.data_ptr(), one.data_ptr(), one.data_ptr(), 0)[1]
            tbufs[id(b), watched] = [loff] + [torch.zeros(max(total, 1), dtype=t, device="cuda")
                                              for t in (torch.int32, torch.int32, torch.int64, torch.int64)]

    def set_lds(v):
        if v is None:
            os.environ.pop("SG_LINK_SERIES_LDS", None)
        else:
            os.environ["SG_LINK_SERIES_LDS"] = v

    # warm-up (code objects, workspaces) and the checks: forms agree, the identity holds on the device
    for name, b, watched, bin_ns, lds in legs:
        set_lds(lds)
        out = outs[id(b), watched]
        b.series(watched, bin_ns, out)
        b.walk()
        b.trace(watched, tbufs[id(b), watched])
        torch.cuda.synchronize()
        assert torch.equal(b.load, b.want)
        total = out[0].sum(dim=1) + out[1].sum(dim=1)
        if watched:
            want = torch.zeros(16, dtype=torch.int64, device="cuda").index_add_(0, b.slot16[b.watch16 != 0].to(torch.int64),
                                                                                b.load[b.watch16 != 0])
        else:
            want = b.load
        assert torch.equal(total, want), f"{name}: the identity with sg_link_load_packets"
        key = (id(b), watched, bin_ns)
        if key in sums:
            assert torch.equal(sums[key][0], out[0]) and torch.equal(sums[key][1], out[1]), f"{name}: the forms differ"
        sums[key] = (out[0].clone(), out[1].clone())
    set_lds(None)

    per = {name: {"series": [], "walk": [], "trace": []} for name, *_ in legs}
    for _ in range(a.runs):
        for name, b, watched, bin_ns, lds in legs:
            set_lds(lds)
            out, bufs = outs[id(b), watched], tbufs[id(b), watched]
            ms = {"series": [], "walk": [], "trace": []}
            for _ in range(a.reps):
                ms["series"].append(timed(ctx, lambda: b.series(watched, bin_ns, out), ("link_series",)))
                ms["walk"].append(timed(ctx, b.walk, ("link_packets",)))
                ms["trace"].append(timed(ctx, lambda: b.trace(watched, bufs), TRACE_TIMERS))
            for k in ms:
                per[name][k].append(statistics.median(ms[k]))
    set_lds(None)

    def stat(xs):
        return {"runs_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
                "spread_ms": round(max(xs) - min(xs), 4)}

    cases = []
    for name, b, watched, bin_ns, lds in legs:
        r = {"leg": name, "nodes": b.w.n, "links": b.w.n_links, "packets": b.P, "delivered": int(b.out.n_delivered),
             "slots": 16 if watched else b.w.n_links, "bins": N_BINS, "bin_ns": bin_ns, "SG_LINK_SERIES_LDS": lds}
        r.update({k: stat(per[name][k]) for k in ("series", "walk", "trace")})
        print(json.dumps(r), flush=True)
        cases.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/series_bench.py", "runs": a.runs, "reps": a.reps, "cases": cases}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
