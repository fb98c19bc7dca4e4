#!/usr/bin/env python3
"""Per-row statistics of the LDS-resident search (SG_SSSP_DIAG) on the C3 graph for
several bucket widths (whole table or a row block): cycles in the search and in the row write-out, phases, far
scans, relaxations per row; then the build's pops by class of S = ceil(arcs / 64) slots per lane
(pops, arcs, step cycles; SG_SSSP_STEP_ARCS=0 gives the lane step's).  python tools/sssp_diag.py [--nodes 10000] [--deltas 25e6,1e9]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# read_timer("sssp_pop_s<name>"): the class's name and the S values it holds
POP_CLASSES = (("0", "0"), ("1", "1"), ("2", "2"), ("4", "3-4"), ("8", "5-8"), ("gt8", ">8"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--degree", type=float, default=8.0)
    ap.add_argument("--deltas", default="25e6,50e6,4e9")
    ap.add_argument("--rows", default="", help="r0:r1, a rank's row block (default: every row)")
    a = ap.parse_args()
    import torch

    from shadow_amd import Context, NetworkGraph, synth

    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    g = synth.ring_chords_graph(a.nodes, a.degree, seed=1)
    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    n = a.nodes
    used = np.arange(n, dtype=np.uint32)
    r0, r1 = (int(x) for x in a.rows.split(":")) if a.rows else (0, n)
    lat = torch.empty((r1 - r0) * n, dtype=torch.int64, device="cuda")
    loss = torch.empty((r1 - r0) * n, dtype=torch.float32, device="cuda")
    os.environ["SG_SSSP_DIAG"] = "1"
    for d in a.deltas.split(","):
        os.environ["SG_APSP_DELTA"] = str(int(float(d)))
        net.build_rows_device(used, r0, r1, lat.data_ptr(), loss.data_ptr(), True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.build_rows_device(used, r0, r1, lat.data_ptr(), loss.data_ptr(), True)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        ctx.enable_timers(True, count_work=True)
        net.build_rows_device(used, r0, r1, lat.data_ptr(), loss.data_ptr(), True)
        # the build's pops by class of S = ceil(arcs / 64) slots per lane: pops, arcs, step cycles
        pops = []
        for name, label in POP_CLASSES:
            _, p, arcs = ctx.read_timer(f"sssp_pop_s{name}")
            _, _, cyc = ctx.read_timer(f"sssp_pop_s{name}_cyc")
            pops.append((label, int(p), int(arcs), int(cyc)))
        _, n_pops, _ = ctx.read_timer("sssp_pops")
        n_rel = ctx.read_timer("sssp")[2]
        ctx.enable_timers(False)
        print(f"delta {d}: {ms:.3f} ms/build", flush=True)
        tp, ta, tc = (max(1, sum(x[i] for x in pops)) for i in (1, 2, 3))
        print(f"pops by class, whole build ({r1 - r0} rows): {int(n_pops)} pops, {n_rel:.0f} relaxations")
        print(f"{'S':>4} {'pops':>10} {'share':>6} {'arcs':>12} {'share':>6} {'step cycles':>14} {'share':>6} {'cycles/pop':>10}")
        for label, p, arcs, cyc in pops:
            print(f"{label:>4} {p:>10} {p / tp:>6.1%} {arcs:>12} {arcs / ta:>6.1%} {cyc:>14} {cyc / tc:>6.1%} "
                  f"{cyc / max(1, p):>10.0f}", flush=True)


if __name__ == "__main__":
    main()
