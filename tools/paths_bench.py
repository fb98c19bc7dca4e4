"""A round's hop records at C3 (sg_tree_paths_packets): the count, scan and fill kernels in the
staged and the direct form of the fill, beside the walk that writes only a hop count
(sg_link_load_packets with only out_hops requested: one walk with its link searches, no atomics).

    python tools/paths_bench.py            # JSON to profiles/paths_bench.json
    python tools/paths_bench.py --reps 9

One process per run.  The C3 table (10k x 10k) is built once with its pred rows on the device; a
host per node.  Per batch one delivery round gives the statuses; then the three routes (staged
fill, direct fill, hops only) are alternated repetition by repetition with the library's timers
on, every record output requested (20 bytes a record), capacity = the total of a sizing call.
The batches are tools/link_round_bench.py's: uniform random (source host, destination host)
pairs, 10k, 100k and 1M packets, and 1M packets over 20,000 distinct pairs, each grouped by source
host.  Reported per batch: kernel ms as median (min .. max) per kernel and form, records per
second and output bytes per second of count + scan + fill, and the hops-only walk.  The two
forms' outputs are compared exactly; correctness itself is tests/test_paths_gpu.py's; bench.py
stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T0 = 946684800 * 10**9
RECORD_BYTES = 20  # node u32, link u32, latency u64, loss f32


def series(ms):
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--sizes", default="10000,100000,1000000")
    p.add_argument("--concentrated", default="1000000:20000", help="packets:distinct pairs")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "paths_bench.json"))
    a = p.parse_args()
    assert a.reps >= 5, "at least five repetitions"
    import torch

    from shadow_amd import NetworkGraph, default_context, synth
    from shadow_amd.worker import Deliveries, DeviceTable, HostTable, PacketBatch, deliver_round

    ctx = default_context(0)
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
    timers = ("tree_paths_count", "tree_paths_scan", "tree_paths_fill")

    def case(name, src, dst):
        dst = np.where(dst == src, (dst + 1) % n, dst)  # (no host sends to itself)
        order = np.argsort(src, kind="stable")
        src, dst = src[order].astype(np.uint32), dst[order]
        P = len(src)
        rs = np.random.default_rng(5)
        pb = PacketBatch.from_numpy(src, hosts["ip"][dst], np.where(rs.random(P) < 0.2, 0, 1448).astype(np.uint32),
                                    np.sort(rs.integers(T0, T0 + 10**6, P)).astype(np.uint64))
        out = Deliveries.allocate(P, n)
        deliver_round(ht, table, pb, T0 + 10**6, 2**63, 0, out=out, ctx=ctx)
        off = torch.zeros(P + 1, dtype=torch.int64, device="cuda")
        hops = torch.empty(P, dtype=torch.int32, device="cuda")
        one = torch.zeros(1, dtype=torch.int32, device="cuda")

        def paths(bufs, cap):
            return net.tree_paths_packets_device(ht, nodes, 0, n, pred.data_ptr(), lat.data_ptr(), loss.data_ptr(), pb,
                                                 out.status.data_ptr(), off.data_ptr(), bufs[0].data_ptr(),
                                                 bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), cap)

        # the sizing call: one real record array, capacity 0
        total = paths([one, one, one, one], 0)
        bufs = {f: [torch.zeros(total, dtype=t, device="cuda")
                    for t in (torch.int32, torch.int32, torch.int64, torch.float32)] for f in ("staged", "direct")}

        def form(f):
            os.environ["SG_PATHS_STAGE"] = "1" if f == "staged" else "0"
            torch.cuda.synchronize()
            ctx.enable_timers(True)
            try:
                assert paths(bufs[f], total) == total
                got = [ctx.read_timer(k) for k in timers]
            finally:
                ctx.enable_timers(False)
                os.environ.pop("SG_PATHS_STAGE", None)
            assert all(launches == 1 for _, launches, _ in got)
            return [ms for ms, _, _ in got]

        def hops_only():
            torch.cuda.synchronize()
            ctx.enable_timers(True)
            try:
                net.link_load_packets_device(ht, nodes, 0, n, pred.data_ptr(), pb, out.status.data_ptr(), 0, 0, 0,
                                             hops.data_ptr())
                ms, launches, _ = ctx.read_timer("link_packets")
            finally:
                ctx.enable_timers(False)
            assert launches == 1
            return ms

        for f in ("staged", "direct"):  # warm-up: code objects, workspaces
            form(f)
        hops_only()
        t = {f: {k: [] for k in timers + ("sum",)} for f in ("staged", "direct")}
        t["hops_only"] = []
        for _ in range(a.reps):
            for f in ("staged", "direct"):
                ms = form(f)
                for k, x in zip(timers, ms):
                    t[f][k].append(x)
                t[f]["sum"].append(sum(ms))
            t["hops_only"].append(hops_only())
        torch.cuda.synchronize()
        for x, y in zip(bufs["staged"], bufs["direct"]):
            assert torch.equal(x, y), "the two forms differ"
        h = hops.cpu().numpy()
        cnt = np.diff(off.cpu().numpy())
        assert np.array_equal(cnt, np.where(h == -1, 0, h)) and int(cnt.sum()) == total
        res = {"case": name, "nodes": n, "packets": P, "delivered": int(out.n_delivered), "records": int(total),
               "hops_mean": round(total / max(int(out.n_delivered), 1), 2), "output_bytes": total * RECORD_BYTES + 8 * (P + 1),
               "hops_only_kernel": series(t["hops_only"])}
        for f in ("staged", "direct"):
            med = statistics.median(t[f]["sum"])
            res[f] = {"count": series(t[f][timers[0]]), "scan": series(t[f][timers[1]]), "fill": series(t[f][timers[2]]),
                      "sum": series(t[f]["sum"]), "records_per_s": round(total / med * 1e3),
                      "output_bytes_per_s": round((total * RECORD_BYTES + 8 * (P + 1)) / med * 1e3),
                      "sum_over_hops_only": round(med / statistics.median(t["hops_only"]), 3)}
        print(json.dumps(res), flush=True)
        return res

    rs = np.random.default_rng(4)
    res = []
    for P in [int(x) for x in a.sizes.split(",") if x]:
        res.append(case(f"{P} packets on uniform random pairs", rs.integers(0, n, P), rs.integers(0, n, P)))
    if a.concentrated:
        P, K = (int(x) for x in a.concentrated.split(":"))
        ps, pd = rs.integers(0, n, K), rs.integers(0, n, K)
        pick = rs.integers(0, K, P)
        res.append(case(f"{P} packets over {K} distinct pairs", ps[pick], pd[pick]))
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/paths_bench.py", "reps": a.reps, "cases": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
