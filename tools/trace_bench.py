"""A round's link trace at C3 (sg_link_trace_packets) beside the same round's hop records
(sg_tree_paths_packets), a hot link, and a watched set.

    python tools/trace_bench.py            # JSON to profiles/trace_bench.json
    python tools/trace_bench.py --reps 9

The command starts one child process per leg, each under a time limit of its own, and stops at the
first leg that fails or runs out of time: nothing is started on the GPU after that.  A leg is one
process on one GPU:
  uniform    the C3 table (10k x 10k) with its pred rows on the device, a host per node; the
             batches of tools/paths_bench.py, uniform random (source host, destination host)
             pairs at 10k, 100k and 1M packets;
  repeated   the same sizes with every packet drawn from packets / 50 distinct pairs (1M packets
             over 20,000 pairs is paths_bench's);
  watch16    the 1M uniform batch with the 16 busiest links watched;
  hot_link   the 512-spoke star, 100k packets from one spoke to spokes across the hub: its link
             to the hub holds all of them (49 pieces of the merge tier).
Per batch one delivery round gives the statuses; then the trace (all four outputs, watch = NULL
unless the leg says otherwise) is alternated repetition by repetition with the hop records (node +
link + latency outputs) on the same inputs, the library's timers on, capacities from sizing calls.
Reported per batch: kernel ms as median (min .. max) per timer, the sums, and trace / hop
records.  Correctness is tests/test_trace_gpu.py's; every run here still checks the offsets against
the link loads and every segment's order.  bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T0 = 946684800 * 10**9
LEGS = {"uniform": 240, "repeated": 240, "watch16": 180, "hot_link": 120}  # name -> seconds
TRACE_TIMERS = ("link_trace_count", "link_trace_fill", "link_trace_sort")
PATHS_TIMERS = ("tree_paths_count", "tree_paths_scan", "tree_paths_fill")


def series(ms):
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def run_leg(a):
    import torch

    from shadow_amd import NetworkGraph, default_context, synth
    from shadow_amd.worker import Deliveries, DeviceTable, HostTable, PacketBatch, deliver_round

    ctx = default_context(0)
    star = a.leg == "hot_link"
    if star:
        spokes = 512
        n = spokes + 1
        v, sp = np.arange(n), np.arange(1, n)
        g = dict(n=n, src=np.concatenate([v, np.zeros(spokes, np.int64), sp]).astype(np.uint32),
                 dst=np.concatenate([v, sp, np.where(sp == spokes, 1, sp + 1)]).astype(np.uint32),
                 lat=np.concatenate([np.full(n, 1_000_000), np.full(spokes, 1_000_000), np.full(spokes, 5_000_000)]).astype(np.uint64),
                 loss=np.zeros(n + 2 * spokes, np.float32), directed=False)
    else:
        n = a.nodes
        g = synth.ring_chords_graph(n, 8.0, seed=1)
    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    nodes = np.arange(n, dtype=np.uint32)
    lat = torch.empty((n, n), dtype=torch.int64, device="cuda")
    loss = torch.empty((n, n), dtype=torch.float32, device="cuda")
    pred = torch.empty((n, n), dtype=torch.int32, device="cuda")
    net.build_rows_device(nodes, 0, n, lat.data_ptr(), loss.data_ptr())
    net.tree_rows_device(nodes, 0, n, lat.data_ptr(), loss.data_ptr(), pred.data_ptr(), 0)
    table = DeviceTable(lat.ravel(), loss.ravel(), n)
    hosts = synth.make_hosts(n, n, exact_seeds=False)
    ht = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    n_links = len(net.links()[0])

    def case(name, src, dst, watch16=False):
        dst = np.where(dst == src, (dst + 1) % n, dst)  # (no host sends to itself)
        order = np.argsort(src, kind="stable")
        src, dst = src[order].astype(np.uint32), dst[order]
        P = len(src)
        rs = np.random.default_rng(5)
        pb = PacketBatch.from_numpy(src, hosts["ip"][dst], np.where(rs.random(P) < 0.2, 0, 1448).astype(np.uint32),
                                    np.sort(rs.integers(T0, T0 + 10**6, P)).astype(np.uint64))
        out = Deliveries.allocate(P, n)
        deliver_round(ht, table, pb, T0 + 10**6, 2**63, 0, out=out, ctx=ctx)
        st = out.status.data_ptr()
        off = torch.zeros(P + 1, dtype=torch.int64, device="cuda")
        loff = torch.zeros(n_links + 1, dtype=torch.int64, device="cuda")
        load = torch.zeros(n_links, dtype=torch.int64, device="cuda")
        one = torch.zeros(2, dtype=torch.int64, device="cuda")
        net.link_load_packets_device(ht, nodes, 0, n, pred.data_ptr(), pb, st, 0, load.data_ptr(), 0, 0)
        torch.cuda.synchronize()
        watch = None
        if watch16:
            m = torch.zeros(n_links, dtype=torch.uint8, device="cuda")
            m[torch.argsort(load, descending=True, stable=True)[:16]] = 1
            watch = m

        def paths(bufs, cap):
            return net.tree_paths_packets_device(ht, nodes, 0, n, pred.data_ptr(), lat.data_ptr(), 0, pb, st, off.data_ptr(),
                                                 bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), 0, cap)

        def trace(bufs, cap):
            return net.link_trace_packets_device(ht, nodes, 0, n, pred.data_ptr(), lat.data_ptr(), pb, st,
                                                 0 if watch is None else watch.data_ptr(), loff.data_ptr(),
                                                 bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                                 bufs[3].data_ptr(), cap)[1]

        # the sizing calls: real record arrays, capacity 0
        p_total, t_total = paths([one, one, one], 0), trace([one, one, one, one], 0)
        assert watch16 or p_total == t_total
        pbufs = [torch.zeros(max(p_total, 1), dtype=t, device="cuda") for t in (torch.int32, torch.int32, torch.int64)]
        tbufs = [torch.zeros(max(t_total, 1), dtype=t, device="cuda") for t in (torch.int32, torch.int32, torch.int64, torch.int64)]

        def timed(call, bufs, total, timers):
            torch.cuda.synchronize()
            ctx.enable_timers(True)
            try:
                assert call(bufs, total) == total
                got = [ctx.read_timer(k) for k in timers]
            finally:
                ctx.enable_timers(False)
            assert all(launches == 1 for _, launches, _ in got)
            return [ms for ms, _, _ in got]

        timed(trace, tbufs, t_total, TRACE_TIMERS)  # warm-up: code objects, workspaces
        timed(paths, pbufs, p_total, PATHS_TIMERS)
        t = {"trace": {k: [] for k in TRACE_TIMERS + ("sum",)}, "paths": {k: [] for k in PATHS_TIMERS + ("sum",)}}
        for _ in range(a.reps):
            for which, call, bufs, total, timers in (("trace", trace, tbufs, t_total, TRACE_TIMERS),
                                                     ("paths", paths, pbufs, p_total, PATHS_TIMERS)):
                ms = timed(call, bufs, total, timers)
                for k, x in zip(timers, ms):
                    t[which][k].append(x)
                t[which]["sum"].append(sum(ms))
        torch.cuda.synchronize()
        # the offsets are the link loads (of the watched links), and every segment ascends in (enter, packet)
        cnt = torch.diff(loff)
        want = load if watch is None else load * watch
        assert torch.equal(cnt, want) and int(loff[-1]) == t_total
        seg = torch.repeat_interleave(torch.arange(n_links, device="cuda"), cnt)
        pk, en = tbufs[0][:t_total].to(torch.int64), tbufs[2][:t_total]
        inside = seg[1:] == seg[:-1]
        ascends = (en[1:] > en[:-1]) | ((en[1:] == en[:-1]) & (pk[1:] > pk[:-1]))
        assert bool(ascends[inside].all()), "a segment out of order"
        res = {"leg": a.leg, "case": name, "nodes": n, "links": n_links, "packets": P, "delivered": int(out.n_delivered),
               "hop_records": int(p_total), "trace_records": int(t_total), "longest_segment": int(cnt.max()),
               "segments_over_64": int((cnt > 64).sum()), "segments_over_2048": int((cnt > 2048).sum())}
        for which, timers in (("trace", TRACE_TIMERS), ("paths", PATHS_TIMERS)):
            res[which] = {k: series(t[which][k]) for k in timers + ("sum",)}
        res["trace_over_paths"] = round(res["trace"]["sum"]["median_ms"] / res["paths"]["sum"]["median_ms"], 3)
        res["trace_records_per_s"] = round(t_total / res["trace"]["sum"]["median_ms"] * 1e3)
        print(json.dumps(res), flush=True)
        return res

    rs = np.random.default_rng(4)
    sizes = [int(x) for x in a.sizes.split(",") if x]
    res = []
    if a.leg == "uniform":
        for P in sizes:
            res.append(case(f"{P} packets on uniform random pairs", rs.integers(0, n, P), rs.integers(0, n, P)))
    elif a.leg == "repeated":
        for P in sizes:
            K = max(P // 50, 1)
            ps, pd = rs.integers(0, n, K), rs.integers(0, n, K)
            pick = rs.integers(0, K, P)
            res.append(case(f"{P} packets over {K} distinct pairs", ps[pick], pd[pick]))
    elif a.leg == "watch16":
        P = sizes[-1]
        res.append(case(f"{P} packets on uniform random pairs, the 16 busiest links watched", rs.integers(0, n, P),
                        rs.integers(0, n, P), watch16=True))
    else:
        P = a.hot_packets  # from spoke 1 to spokes 3 .. 511: 1 - 0 - k
        res.append(case(f"{P} packets from one spoke of a 512-spoke star across the hub", np.ones(P, np.int64),
                        rs.integers(3, 512, P)))
    with open(a.leg_out, "w") as f:
        json.dump(res, f)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--sizes", default="10000,100000,1000000")
    p.add_argument("--hot-packets", type=int, default=100000)
    p.add_argument("--legs", default=",".join(LEGS))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench.json"))
    p.add_argument("--leg", help=argparse.SUPPRESS)  # (a child: run this leg, write --leg-out)
    p.add_argument("--leg-out", help=argparse.SUPPRESS)
    a = p.parse_args()
    assert a.reps >= 5, "at least five repetitions"
    if a.leg:
        return run_leg(a)
    cases, stopped = [], None
    for leg in [x for x in a.legs.split(",") if x]:
        tmp = a.out + f".{leg}.tmp"
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--leg-out", tmp, "--reps", str(a.reps), "--nodes",
               str(a.nodes), "--sizes", a.sizes, "--hot-packets", str(a.hot_packets)]
        try:
            rc = subprocess.run(cmd, timeout=LEGS[leg]).returncode
        except subprocess.TimeoutExpired:
            rc = "time limit"
        if rc != 0:
            stopped = f"leg {leg}: {rc}"
            print(stopped + "; nothing more is started", file=sys.stderr)
            break
        with open(tmp) as f:
            cases += json.load(f)
        os.remove(tmp)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/trace_bench.py", "reps": a.reps, "stopped": stopped, "cases": cases}, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
