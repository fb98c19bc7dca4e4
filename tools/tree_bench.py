"""The shortest-path tree pass (sg_routing_tree) beside the build of the same rows.

    python tools/tree_bench.py                 # C3 whole table and one C5 row block,
                                               # JSON to profiles/tree_bench.json
    python tools/tree_bench.py --no-c5 --reps 9

Per shape, in one process and alternated repetition by repetition: the wall time of
sg_routing_build over the rows (device outputs, timers off: the build as bench.py measures it),
then the tree pass over those rows with the library's timers on, read_timer("tree") and its wall
time.  Medians, spreads and the bytes a tree launch moves (12 B read and 8 B written per cell;
the arc records and the node list are re-read from L2 and not counted).  bench.py stays the
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


def series(ms):
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def shape(name, n, degree, r0, r1, reps, lds_env=None):
    import torch

    from shadow_amd import NetworkGraph, default_context, synth

    ctx = default_context(0)
    g = synth.ring_chords_graph(n, degree, seed=1)
    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    nodes = np.arange(n, dtype=np.uint32)
    rows = r1 - r0
    lat = torch.empty((rows, n), dtype=torch.int64, device="cuda")
    loss = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    pred = torch.empty((rows, n), dtype=torch.int32, device="cuda")
    hop = torch.empty((rows, n), dtype=torch.int32, device="cuda")
    if lds_env is not None:
        os.environ["SG_TREE_LDS"] = lds_env

    def build():
        t0 = time.perf_counter()
        net.build_rows_device(nodes, r0, r1, lat.data_ptr(), loss.data_ptr())
        return (time.perf_counter() - t0) * 1e3

    def tree():
        ctx.enable_timers(True)
        try:
            t0 = time.perf_counter()
            net.tree_rows_device(nodes, r0, r1, lat.data_ptr(), loss.data_ptr(), pred.data_ptr(), hop.data_ptr())
            wall = (time.perf_counter() - t0) * 1e3
            ms, launches, work = ctx.read_timer("tree")
            lds_rows, n_max = ctx.read_timer("tree_lds")[1:]
        finally:
            ctx.enable_timers(False)
        assert launches == 1
        return ms, wall, work, int(lds_rows), int(n_max)

    build()
    tree()  # warm-up: code objects, the in-arc CSC, workspaces
    b, t, tw = [], [], []
    for _ in range(reps):
        b.append(build())
        ms, wall, work, lds_rows, n_max = tree()
        t.append(ms)
        tw.append(wall)
    torch.cuda.synchronize()
    os.environ.pop("SG_TREE_LDS", None)
    out = {"shape": name, "nodes": n, "arcs": int(2 * (g["src"] != g["dst"]).sum()), "rows": [r0, r1],
           "path": "lds" if lds_rows else "global", "lds_node_limit": n_max,
           "build_wall": series(b), "tree_kernel": series(t), "tree_wall": series(tw),
           "bytes_per_launch": int(work), "tree_gb_per_s": round(work / statistics.median(t) / 1e6, 1),
           "ratio_tree_over_build": round(statistics.median(t) / statistics.median(b), 3)}
    print(json.dumps(out), flush=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--no-c5", action="store_true")
    p.add_argument("--no-global-c3", action="store_true", help="skip C3 with SG_TREE_LDS=0")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_bench.json"))
    a = p.parse_args()
    assert a.reps >= 5, "at least five repetitions"
    res = [shape("C3 whole table", 10000, 8.0, 0, 10000, a.reps)]
    if not a.no_global_c3:
        res.append(shape("C3 whole table, SG_TREE_LDS=0", 10000, 8.0, 0, 10000, a.reps, lds_env="0"))
    if not a.no_c5:
        res.append(shape("C5 row block", 50000, 8.0, 0, 6250, a.reps))
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/tree_bench.py", "reps": a.reps, "shapes": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
