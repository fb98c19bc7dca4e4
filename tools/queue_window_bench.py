"""The windowed link queues at C3 (sg_link_queue with SG_LINK_QUEUE_WINDOW) beside the carried call as it is.

    python tools/queue_window_bench.py       # JSON to profiles/queue_window_bench.json

One process on one GPU; any failure ends it, so nothing is started on the GPU after one.  The
worlds, batches and legs are tools/queue_bench.py's: 8,000 ps a byte (1 Gbit/s) on every link,
payload weights, all eight outputs.  Per leg, alternated `--runs` times, wall time with a device
synchronisation at both ends (a windowed solve is many calls and the torch merge between them,
which the library's timers do not see):
  carried    the carried call as it is (median of `--reps`), its iterations;
  window_x1, window_x4, window_x16
             the trace solved window by window by a LinkQueueSession (graph._step_windows, what
             PathTree.link_queue_round(window_ns=) runs) at 1, 4 and 16 times the trace's smallest gap,
             results left on the device: total ms, calls, the calls' summed iterations, and the records
             sorted and scanned (read_timer("link_queue_active"), summed) against records x iterations
             of the carried call.  A solve is cut at `--max-calls` calls and then reported as cut,
             with the records still pending.  The first run asserts that an uncut solve gives the
             carried call's wait and done at every record.
Reported as the median over the runs with the spread (max - min).  Nothing is fixed in advance:
whether the window cuts the time is what this measures.
Then a session over the 1M leg cut into 8 rounds by send time, each round a delivery round of its
own with its own device trace: per round the wall ms of the trace, and of advance()'s merge, solve
and keep, and the records pending after it; at the end a flush.
Correctness is tests/test_queue_window_gpu.py's; bench.py stays the project's headline benchmark."""
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

from queue_bench import COST_PS, Queue  # noqa: E402
from queue_carry_bench import call  # noqa: E402
from series_bench import T0, Batch, World, star_graph  # noqa: E402

MULTS = (1, 4, 16)


def wall(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def smallest_gap(q):
    """The smallest gap between two consecutive records of one packet, on the device."""
    import torch

    n = q.total
    enter, pkt = q.bufs[3][:n], q.bufs[1][:n].to(torch.int64)
    o = torch.argsort(enter, stable=True)
    o = o[torch.argsort(pkt[o], stable=True)]
    same = pkt[o][1:] == pkt[o][:-1]
    gaps = (enter[o][1:] - enter[o][:-1])[same]
    return int(gaps.min()) if gaps.numel() else 0


def windowed(ctx, q, window_ns, max_calls, check=None):
    """One windowed solve of the leg's trace: (ms, calls, iterations, active, pending left)."""
    import torch

    from shadow_amd.link_queue import _step_windows
    from shadow_amd.queue_session import LinkQueueSession

    n, P = q.total, q.b.P
    s = LinkQueueSession(ctx, COST_PS, n_links=q.w.n_links)
    s.on_host = False
    weight = q.b.pb.payload_len.view(torch.int32).reshape(-1)[:P]
    base = torch.zeros(P, dtype=torch.int64, device="cuda")
    wait = torch.zeros(n, dtype=torch.int64, device="cuda")
    done = torch.zeros(n, dtype=torch.int64, device="cuda")

    def settled(pk, rc):
        wait[rc.record], done[rc.record] = rc.wait_ns, rc.done_ns

    ms, calls = wall(lambda: _step_windows(s, q.bufs[0], n, q.bufs[3], q.bufs[1], weight, base, window_ns, settled, max_calls))
    if check is not None and not s.pending:
        assert torch.equal(wait, check[0]) and torch.equal(done, check[1]), "the windowed solve differs from the carried call"
    return ms, calls, s.iterations, s.active, s.pending


def main():
    import torch

    from shadow_amd import default_context, synth
    from shadow_amd.queue_session import LinkQueueSession
    from shadow_amd.worker import Deliveries, PacketBatch, deliver_round

    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--max-calls", type=int, default=100)
    p.add_argument("--legs", type=int, default=1, help="0: the session alone, merged into the file that is there")
    p.add_argument("--session", type=int, default=1)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_window_bench.json"))
    a = p.parse_args()
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

    info, want = {}, {}
    for name, q in legs:  # warm-up, the gap, the carried call's result
        q.trace()
        call(q, True)
        torch.cuda.synchronize()
        want[name] = (q.rec[0][:q.total].clone(), q.rec[1][:q.total].clone())
        info[name] = {"gap_ns": smallest_gap(q), "carried_iterations": int(ctx.read_timer("link_queue_iters")[1])}
        print(json.dumps({"leg": name, "records": q.total, **info[name]}), flush=True)

    keys = ["carried"] + [f"window_x{m}" for m in MULTS]
    per = {name: {k: [] for k in keys} for name, _ in legs}
    counts = {name: {} for name, _ in legs}
    for run in range(a.runs if a.legs else 0):
        for name, q in legs:
            per[name]["carried"].append(statistics.median(wall(lambda: call(q, True))[0] for _ in range(a.reps)))
            for m in MULTS:
                k = f"window_x{m}"
                if not q.total or not info[name]["gap_ns"]:
                    continue
                ms, calls, iters, active, left = windowed(ctx, q, m * info[name]["gap_ns"], a.max_calls, want[name] if run == 0 else None)
                per[name][k].append(ms)
                counts[name][k] = {"calls": calls, "iterations": iters, "active": active, "cut_with_pending": left}
            print(json.dumps({"run": run, "leg": name, **{k: round(v[-1], 3) for k, v in per[name].items() if v}}), flush=True)

    def stat(xs):
        return {"runs_ms": [round(x, 3) for x in xs], "median_ms": round(statistics.median(xs), 3),
                "spread_ms": round(max(xs) - min(xs), 3)}

    cases = []
    for name, q in legs if a.legs else []:
        r = {"leg": name, "nodes": q.w.n, "links": q.w.n_links, "packets": q.b.P, "records": q.total, "cost_ps": COST_PS}
        r.update(info[name])
        r["carried_records_x_iterations"] = q.total * info[name]["carried_iterations"]
        for k in keys:
            if per[name][k]:
                r[k] = dict(stat(per[name][k]), **counts[name].get(k, {}))
        cases.append(r)
        print(json.dumps(r), flush=True)

    # ---- a session over the 1M leg cut into 8 rounds by send time
    b = batches[1_000_000]
    send = b.pb.send_time_ns.cpu().numpy().view(np.uint64)
    rounds = []
    if a.session:
        src = b.pb.src_host.cpu().numpy().view(np.uint32)
        dst_ip = b.pb.dst_ipv4.cpu().numpy().view(np.uint32)
        pay = b.pb.payload_len.cpu().numpy().view(np.uint32)
        edges = (T0 + np.arange(1, 9) * (10**6 // 8)).astype(np.uint64)  # (u64 like send: no float promotion)
        which = np.searchsorted(edges, send, side="right")
        s = LinkQueueSession(ctx, COST_PS, n_links=c3.n_links)
        s.on_host, s.profile = False, {}
        for k in range(8):
            m = np.flatnonzero(which == k)  # (ascending: still grouped by source host)
            rb = Batch.__new__(Batch)
            rb.w, rb.P = c3, len(m)
            rb.pb = PacketBatch.from_numpy(src[m], dst_ip[m], pay[m], send[m])
            rb.out = Deliveries.allocate(rb.P, c3.n)
            deliver_round(c3.ht, c3.table, rb.pb, int(edges[k]), 2**63, 0, out=rb.out, ctx=ctx)
            rb.st, rb.wt = rb.out.status.data_ptr(), rb.pb.payload_len.data_ptr()
            rb.watch16 = b.watch16
            t_alloc, q = wall(lambda: Queue(rb, False))
            t_trace, _ = wall(q.trace)
            weight = rb.pb.payload_len.view(torch.int32).reshape(-1)[:rb.P]
            base = rb.out.deliver_time_ns.view(torch.int64).reshape(-1)[:rb.P]
            t_adv, _ = wall(lambda: s.advance(q.bufs[0], q.bufs[3][:q.total], q.bufs[1][:q.total], weight, base, int(edges[k])))
            rounds.append({"round": k, "packets": rb.P, "records": q.total, "trace_ms": round(t_trace, 3),
                           **{f"{x}_ms": round(v, 3) for x, v in s.profile.items()}, "advance_ms": round(t_adv, 3),
                           "pending": s.pending, "in_flight": s.in_flight})
            print(json.dumps(rounds[-1]), flush=True)
        t_adv, _ = wall(s.flush)
        rounds.append({"round": "flush", **{f"{x}_ms": round(v, 3) for x, v in s.profile.items()}, "advance_ms": round(t_adv, 3),
                       "pending": s.pending, "iterations": s.iterations, "active": s.active})
        print(json.dumps(rounds[-1]), flush=True)
    doc = {"tool": "tools/queue_window_bench.py", "runs": a.runs, "reps": a.reps, "max_calls": a.max_calls, "cases": cases,
           "session_8_rounds": rounds}
    if not a.legs and os.path.exists(a.out):
        with open(a.out) as f:
            doc = dict(json.load(f), session_8_rounds=rounds)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
