"""Link loads (sg_link_load) beside the tree pass (sg_routing_tree) of the same rows, at C3.

    python tools/link_load_bench.py            # JSON to profiles/link_load_bench.json
    python tools/link_load_bench.py --reps 9

One process per run.  The C3 table (10k x 10k) is built once with its pred rows on the device;
then, per traffic matrix, the tree pass and the link-load call are alternated repetition by
repetition with the library's timers on: read_timer("tree") and read_timer("link_load"), and the
calls' wall times.  Medians and ranges.  The matrices:
  (i)   C4-like: 1M packets on uniform random (source, destination) pairs;
  (ii)  dense: every cell 1;
  (iii) (i) under SG_LINK_LDS=0 (the global path).
Bytes per link-load launch = the pred row and the counter row of every row (12 B a cell); the link
lists (lk_off, lk_tail) and the node list are re-read from L2 and not counted.  The outputs are
zeroed before every repetition (not timed); per matrix the tool checks that the self-loop links
hold the diagonal's sum and that every repetition gives the same arrays (correctness itself is
tests/test_link_gpu.py's).  bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def series(ms):
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--packets", type=int, default=1_000_000)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_load_bench.json"))
    a = p.parse_args()
    assert a.reps >= 5, "at least five repetitions"
    import torch

    from shadow_amd import NetworkGraph, default_context, synth

    ctx = default_context(0)
    n = a.nodes
    g = synth.ring_chords_graph(n, 8.0, seed=1)
    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    nodes = np.arange(n, dtype=np.uint32)
    lat = torch.empty((n, n), dtype=torch.int64, device="cuda")
    loss = torch.empty((n, n), dtype=torch.float32, device="cuda")
    pred = torch.empty((n, n), dtype=torch.int32, device="cuda")
    hop = torch.empty((n, n), dtype=torch.int32, device="cuda")
    net.build_rows_device(nodes, 0, n, lat.data_ptr(), loss.data_ptr())
    tail, head = net.links()
    n_links = len(tail)
    loops = torch.from_numpy(np.flatnonzero(tail == head)).cuda()
    link = torch.zeros(n_links, dtype=torch.int64, device="cuda")
    node = torch.zeros(n, dtype=torch.int64, device="cuda")

    def tree():
        ctx.enable_timers(True)
        try:
            t0 = time.perf_counter()
            net.tree_rows_device(nodes, 0, n, lat.data_ptr(), loss.data_ptr(), pred.data_ptr(), hop.data_ptr())
            wall = (time.perf_counter() - t0) * 1e3
            ms = ctx.read_timer("tree")[0]
        finally:
            ctx.enable_timers(False)
        return ms, wall

    def load(counts):
        link.zero_()
        node.zero_()
        torch.cuda.synchronize()
        ctx.enable_timers(True)
        try:
            t0 = time.perf_counter()
            net.link_load_device(nodes, 0, n, pred.data_ptr(), counts.data_ptr(), n, link.data_ptr(), node.data_ptr())
            wall = (time.perf_counter() - t0) * 1e3
            ms, launches, work = ctx.read_timer("link_load")
            lds_rows, n_max = ctx.read_timer("link_lds")[1:]
        finally:
            ctx.enable_timers(False)
        assert launches == 1
        return ms, wall, work, int(lds_rows), int(n_max)

    def case(name, counts, lds_env=None):
        if lds_env is not None:
            os.environ["SG_LINK_LDS"] = lds_env
        try:
            tree()
            load(counts)  # warm-up: code objects, the link list, workspaces
            first = (link.clone(), node.clone())
            t, tw, k, kw = [], [], [], []
            for _ in range(a.reps):
                ms, wall = tree()
                t.append(ms)
                tw.append(wall)
                ms, wall, work, lds_rows, n_max = load(counts)
                k.append(ms)
                kw.append(wall)
            torch.cuda.synchronize()
        finally:
            os.environ.pop("SG_LINK_LDS", None)
        assert torch.equal(link, first[0]) and torch.equal(node, first[1]), "two repetitions differ"
        assert int(link[loops].sum()) == int(torch.diagonal(counts).sum()), "the diagonal is not on the self-loops"
        out = {"case": name, "nodes": n, "links": n_links, "rows": [0, n],
               "cells_nonzero": int((counts != 0).sum()), "count_total": int(counts.sum()),
               "link_load_total": int(link.sum()), "node_load_total": int(node.sum()),
               "path": "lds" if lds_rows else "global", "lds_node_limit": n_max,
               "tree_kernel": series(t), "tree_wall": series(tw), "link_kernel": series(k), "link_wall": series(kw),
               "bytes_per_launch": int(work), "link_gb_per_s": round(work / statistics.median(k) / 1e6, 1),
               "ratio_link_over_tree": round(statistics.median(k) / statistics.median(t), 3)}
        print(json.dumps(out), flush=True)
        return out

    rng = np.random.default_rng(4)
    flat = rng.integers(0, n, a.packets) * n + rng.integers(0, n, a.packets)
    sparse = torch.bincount(torch.from_numpy(flat).cuda(), minlength=n * n).reshape(n, n).contiguous()
    res = [case(f"(i) {a.packets} packets on uniform random pairs", sparse)]
    res.append(case("(iii) the same under SG_LINK_LDS=0", sparse, lds_env="0"))
    dense = torch.ones((n, n), dtype=torch.int64, device="cuda")
    res.append(case("(ii) dense, every cell 1", dense))
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/link_load_bench.py", "reps": a.reps, "cases": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
