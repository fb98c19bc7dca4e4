"""A round's carried link queues at C3 (sg_link_queue with SG_LINK_QUEUE_CARRY on the device trace
of sg_link_trace_packets) beside the first-order call on the same trace.

    python tools/queue_carry_bench.py      # JSON to profiles/queue_carry_bench.json

One process on one GPU; any failure ends it, so nothing is started on the GPU after one.  The
worlds, batches and legs are tools/queue_bench.py's: 8,000 ps a byte (1 Gbit/s) on every link,
payload weights, all eight outputs.  The legs are alternated `--runs` times; inside a run every
leg is timed `--reps` times and gives its median.  Reported per leg, as the median over the runs
of each run's median with the spread (max - min over the runs):
  first    the first-order call, "link_queue" + "link_queue_ahead";
  carried  the carried call's device time: the chains ("link_queue_index"), then per iteration
           the sort ("link_queue_sort"), the scan ("link_queue": the iterations' scans and the
           last pass) and the propagate step ("link_queue_carry"), and "link_queue_ahead";
  wall     the carried call on the host's clock, its synchronisation per iteration included;
and once per leg the iterations, the records whose carried enter time differs from the trace's
and the records that wait.  A leg whose fixed point does not settle within
SG_LINK_QUEUE_CARRY_ITERS is reported with its error and not timed.  Correctness is
tests/test_queue_carry_gpu.py's; bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from queue_bench import COST_PS, QUEUE_TIMERS, Queue  # noqa: E402
from series_bench import Batch, World, star_graph  # noqa: E402

CARRY_TIMERS = ("link_queue_index", "link_queue_sort", "link_queue", "link_queue_carry", "link_queue_ahead")


def call(q, carry):
    w, f, r, k = q.w, q.bufs, q.rec, q.lnk
    w.net.link_queue_device(f[0].data_ptr(), q.total, f[3].data_ptr(), f[1].data_ptr(), q.b.wt, q.b.P, q.cost.data_ptr(), 0,
                            wait_ptr=r[0].data_ptr(), done_ptr=r[1].data_ptr(), ahead_ptr=r[2].data_ptr(),
                            link_free_ptr=k[0].data_ptr(), busy_ptr=k[1].data_ptr(), wait_max_ptr=k[2].data_ptr(),
                            wait_sum_ptr=k[3].data_ptr(), ahead_max_ptr=k[4].data_ptr(), carry=carry)


def timed(ctx, fn, timers):
    """({timer: ms}, wall ms) of one call."""
    import torch

    torch.cuda.synchronize()
    ctx.enable_timers(True)
    try:
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        got = {k: ctx.read_timer(k)[0] for k in timers}
    finally:
        ctx.enable_timers(False)
    return got, wall


def main():
    import torch

    from shadow_amd import ShadowGpuError, default_context, synth

    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_carry_bench.json"))
    a = p.parse_args()
    assert a.runs >= 5 and a.reps >= 3
    os.environ["SG_LINK_COMBINE"] = "0"  # (series_bench's Batch times the plain walk)
    os.environ["SG_LINK_QUEUE_SERIAL"] = "0"
    ctx = default_context(0)
    c3 = World(synth.ring_chords_graph(a.nodes, 8.0, seed=1), ctx)
    star = World(star_graph(), ctx)
    rs = np.random.default_rng(4)
    n = c3.n
    batches = {P: Batch(c3, rs.integers(0, n, P), rs.integers(0, n, P)) for P in (10_000, 100_000, 1_000_000)}
    hot = Batch(star, np.ones(100_000, np.int64), rs.integers(3, 512, 100_000))
    legs = [("all, 1M", Queue(batches[1_000_000], False)), ("watch16, 1M", Queue(batches[1_000_000], True)),
            ("hot link, 100k", Queue(hot, True)), ("all, 100k", Queue(batches[100_000], False)),
            ("all, 10k", Queue(batches[10_000], False))]

    # warm-up (code objects, workspaces), the iterations and what moved
    info = {}
    for name, q in legs:
        q.trace()
        call(q, False)
        torch.cuda.synchronize()
        r = {"longest_segment": int(torch.diff(q.bufs[0]).max()), "first_order_waiting": int((q.rec[0][:q.total] > 0).sum())}
        try:
            call(q, True)
        except ShadowGpuError as e:
            r["error"] = str(e)
            info[name] = r
            print(json.dumps({"leg": name, **r}), flush=True)
            continue
        torch.cuda.synchronize()
        r["iterations"] = int(ctx.read_timer("link_queue_iters")[1])
        t = q.total
        pkt = q.bufs[1][:t].long()
        wt = q.b.pb.payload_len.view(torch.int32)[pkt].long()
        s = (wt * COST_PS + 999) // 1000
        enter = q.rec[1][:t] - s - q.rec[0][:t]
        r["records_moved"] = int((enter != q.bufs[3][:t]).sum())
        r["records_waiting"] = int((q.rec[0][:t] > 0).sum())
        r["hops_max"] = int(torch.bincount(pkt).max()) if t else 0
        info[name] = r

    keys = ("first", "index", "sort", "scan", "propagate", "ahead", "carried", "wall")
    per = {name: {k: [] for k in keys} for name, _ in legs}
    for _ in range(a.runs):
        for name, q in legs:
            if "error" in info[name]:
                continue
            ms = {k: [] for k in keys}
            for _ in range(a.reps):
                got, _ = timed(ctx, lambda: call(q, False), QUEUE_TIMERS)
                ms["first"].append(sum(got.values()))
                got, wall = timed(ctx, lambda: call(q, True), CARRY_TIMERS)
                for k, t in zip(keys[1:6], CARRY_TIMERS):
                    ms[k].append(got[t])
                ms["carried"].append(sum(got.values()))
                ms["wall"].append(wall)
            for k in keys:
                per[name][k].append(statistics.median(ms[k]))

    def stat(xs):
        return {"runs_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
                "spread_ms": round(max(xs) - min(xs), 4)}

    cases = []
    for name, q in legs:
        r = {"leg": name, "nodes": q.w.n, "links": q.w.n_links, "packets": q.b.P, "records": q.total, "cost_ps": COST_PS}
        r.update(info[name])
        if "error" not in r:
            r.update({k: stat(per[name][k]) for k in keys})
            it = r["iterations"]
            r["per_iteration_ms"] = {k: round(r[k]["median_ms"] / it, 4) for k in ("sort", "propagate")}
            # (the scan ran once more than the iterations: the last pass)
            r["per_iteration_ms"]["scan"] = round(r["scan"]["median_ms"] / (it + 1), 4)
            r["moved_fraction"] = round(r["records_moved"] / max(q.total, 1), 4)
        print(json.dumps(r), flush=True)
        cases.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/queue_carry_bench.py", "runs": a.runs, "reps": a.reps, "cases": cases}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
