"""A round's link loads two ways, at C3: the dense fold of the round's counters (sg_link_load)
against the per-packet walk (sg_link_load_packets).

    python tools/link_round_bench.py            # JSON to profiles/link_round_bench.json
    python tools/link_round_bench.py --reps 9

One process per run.  The C3 table (10k x 10k, packed) is built once with its pred rows on the
device; a host per node.  Per batch the two routes are alternated repetition by repetition with
the library's timers on:
  dense:  a delivery round with device counters (read_timer("walk"), the round's wall time),
          then sg_link_load on the counters (read_timer("link_load"));
  direct: the same round without counters, then sg_link_load_packets on the round's own status
          (read_timer("link_packets")), under SG_LINK_COMBINE=0 (every packet walks on its own:
          "direct") and under SG_LINK_COMBINE=1 (the default: a wave sums its equal (row, column)
          pairs before the walk: "direct_combined").
Before every round the hosts' RNG streams and event counters are put back (not timed), so every
round of a batch delivers the same packets and the routes' outputs are compared exactly.  The
batches: uniform random (source host, destination host) pairs, 10k, 100k and 1M packets, and 1M
packets over 20,000 distinct pairs; each grouped by source host as a round's batch is.
Reported per batch: kernel ms as median (min .. max), packets x hops per second and global
atomics per second of the direct route (hops from out_hops; two u64 adds per hop, one for a
same-node packet).  Correctness itself is tests/test_link_round_gpu.py's; bench.py stays the
project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T0 = 946684800 * 10**9


def series(ms):
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--sizes", default="10000,100000,1000000")
    p.add_argument("--concentrated", default="1000000:20000", help="packets:distinct pairs")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_round_bench.json"))
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
    assert table.pack(ctx)
    n_links = len(net.links()[0])
    hosts = synth.make_hosts(n, n, exact_seeds=False)
    ht = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    rng0, ctr0 = ht.get_state()
    counts = torch.zeros(n * n, dtype=torch.int64, device="cuda")
    link = [torch.zeros(n_links, dtype=torch.int64, device="cuda") for _ in range(3)]
    node = [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(3)]

    def round_(pb, out, counting):
        """One delivery round from the hosts' initial state: (walk kernel ms, wall ms)."""
        ht.set_state(rng0, ctr0)
        if counting:
            counts.zero_()
        torch.cuda.synchronize()
        ctx.set_packet_counters(counts if counting else None)
        ctx.enable_timers(True)
        try:
            t0 = time.perf_counter()
            deliver_round(ht, table, pb, T0 + 10**6, 2**63, 0, out=out, ctx=ctx)
            wall = (time.perf_counter() - t0) * 1e3
            ms = ctx.read_timer("walk")[0]
        finally:
            ctx.enable_timers(False)
            ctx.set_packet_counters(None)
        return ms, wall

    def timed(name, call, k):
        link[k].zero_()
        node[k].zero_()
        torch.cuda.synchronize()
        ctx.enable_timers(True)
        try:
            t0 = time.perf_counter()
            call()
            wall = (time.perf_counter() - t0) * 1e3
            ms, launches, work = ctx.read_timer(name)
        finally:
            ctx.enable_timers(False)
        assert launches == 1
        return ms, wall, work

    def case(name, src, dst):
        dst = np.where(dst == src, (dst + 1) % n, dst)  # (no host sends to itself)
        order = np.argsort(src, kind="stable")
        src, dst = src[order].astype(np.uint32), dst[order]
        P = len(src)
        rs = np.random.default_rng(5)
        pb = PacketBatch.from_numpy(src, hosts["ip"][dst], np.where(rs.random(P) < 0.2, 0, 1448).astype(np.uint32),
                                    np.sort(rs.integers(T0, T0 + 10**6, P)).astype(np.uint64))
        out = Deliveries.allocate(P, n)
        hops = torch.empty(P, dtype=torch.int32, device="cuda")

        def dense():
            net.link_load_device(nodes, 0, n, pred.data_ptr(), counts.data_ptr(), n, link[0].data_ptr(),
                                 node[0].data_ptr())

        def direct(k):
            net.link_load_packets_device(ht, nodes, 0, n, pred.data_ptr(), pb, out.status.data_ptr(), 0,
                                         link[k].data_ptr(), node[k].data_ptr(), hops.data_ptr())

        def form(combine, k):
            os.environ["SG_LINK_COMBINE"] = combine
            try:
                direct(k)
            finally:
                os.environ.pop("SG_LINK_COMBINE", None)

        plain, combined = (lambda: form("0", 1)), (lambda: form("1", 2))

        # warm-up: code objects, the link list, workspaces
        round_(pb, out, True)
        timed("link_load", dense, 0)
        round_(pb, out, False)
        timed("link_packets", plain, 1)
        timed("link_packets", combined, 2)
        t = {k: [] for k in ("walk_cnt", "round_cnt_wall", "fold", "fold_wall", "walk", "round_wall", "direct",
                             "direct_wall", "combined")}
        for _ in range(a.reps):
            ms, wall = round_(pb, out, True)
            t["walk_cnt"].append(ms)
            t["round_cnt_wall"].append(wall)
            ms, wall, _ = timed("link_load", dense, 0)
            t["fold"].append(ms)
            t["fold_wall"].append(wall)
            ms, wall = round_(pb, out, False)
            t["walk"].append(ms)
            t["round_wall"].append(wall)
            ms, wall, walked = timed("link_packets", plain, 1)
            t["direct"].append(ms)
            t["direct_wall"].append(wall)
            t["combined"].append(timed("link_packets", combined, 2)[0])
        torch.cuda.synchronize()
        for k in (1, 2):
            assert torch.equal(link[0], link[k]) and torch.equal(node[0], node[k]), "the routes differ"
        h = hops.cpu().numpy()
        counted = h != -1
        assert int(counted.sum()) == out.n_delivered == int(walked)
        total_hops = int(h[counted].astype(np.int64).sum())
        same_node = int((hosts["route"][src] == hosts["route"][dst])[counted].sum())
        atomics = 2 * total_hops - same_node
        pairs = len(np.unique(src.astype(np.int64) * n + dst))
        d_ms, c_ms = statistics.median(t["direct"]), statistics.median(t["combined"])
        res = {"case": name, "nodes": n, "links": n_links, "packets": P, "distinct_pairs": pairs,
               "delivered": int(out.n_delivered), "hops_total": total_hops,
               "hops_mean": round(total_hops / max(int(counted.sum()), 1), 2), "atomics": atomics,
               "dense": {"walk_with_counters_kernel": series(t["walk_cnt"]), "round_wall": series(t["round_cnt_wall"]),
                         "link_load_kernel": series(t["fold"]), "link_load_wall": series(t["fold_wall"])},
               "direct": {"walk_kernel": series(t["walk"]), "round_wall": series(t["round_wall"]),
                          "link_packets_kernel": series(t["direct"]), "link_packets_wall": series(t["direct_wall"]),
                          "packet_hops_per_s": round(total_hops / d_ms * 1e3), "atomics_per_s": round(atomics / d_ms * 1e3)},
               "direct_combined": {"link_packets_kernel": series(t["combined"]),
                                   "packet_hops_per_s": round(total_hops / c_ms * 1e3)},
               "ratio_direct_over_fold": round(d_ms / statistics.median(t["fold"]), 3)}
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
        json.dump({"tool": "tools/link_round_bench.py", "reps": a.reps, "cases": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
