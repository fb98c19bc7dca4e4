"""A round's link queues with finite buffers at C3 (sg_link_queue with SG_LINK_QUEUE_DROP on the
device trace of sg_link_trace_packets) beside the unflagged calls on the same trace.

    python tools/queue_drop_bench.py       # JSON to profiles/queue_drop_bench.json

One process on one GPU; any failure ends it, so nothing is started on the GPU after one.  The
worlds, batches and legs are tools/queue_bench.py's: 8,000 ps a byte (1 Gbit/s) on every link,
payload weights, all eight outputs.  limit_ns[L] is the median positive wait on L in the unlimited
result of the same mode (of an even count the two middle values' mean, rounded down), 2^64 - 1 on
a link where nothing waits; the limits are computed once, outside the timed region.  The legs are
alternated `--runs` times; inside a run every leg is timed `--reps` times and gives its median.
Reported per leg, as the median over the runs of each run's median with the spread (max - min
over the runs), device time by the library's timers:
  first          the unflagged first-order call, "link_queue" + "link_queue_ahead";
  drop           the flagged first-order call, its busy periods walked in parallel;
  drop_serial    the flagged first-order call under SG_LINK_QUEUE_SERIAL = 1, a lane per link;
  carried        the unflagged carried call, all its timers;
  carried_drop   the flagged carried call, and its split: the chains, then per iteration the sort,
                 the walk ("link_queue") and the propagate step, and the outputs;
and once per leg the fraction of records dropped and absent in either mode and the iterations.
Every leg asserts that the two flagged first-order forms agree bit for bit.  Correctness is
tests/test_queue_drop_gpu.py's; bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from queue_bench import COST_PS, QUEUE_TIMERS, Queue  # noqa: E402
from queue_carry_bench import CARRY_TIMERS, timed  # noqa: E402
from series_bench import Batch, World, star_graph  # noqa: E402

UMAX = 0xFFFFFFFFFFFFFFFF


def median_limits(off, wait):
    """One u64 per link from a call's link_off and wait_ns (host arrays)."""
    nl = len(off) - 1
    lim = np.full(nl, UMAX, np.uint64)
    link = np.repeat(np.arange(nl), np.diff(off.astype(np.int64)))
    pos = wait > 0
    link, w = link[pos], wait[pos]
    order = np.lexsort((w, link))
    link, w = link[order], w[order]
    first = np.flatnonzero(np.r_[True, link[1:] != link[:-1]]) if len(link) else np.zeros(0, np.int64)
    count = np.diff(np.r_[first, len(link)])
    lo, hi = w[first + (count - 1) // 2], w[first + count // 2]
    lim[link[first]] = lo + (hi - lo) // np.uint64(2)
    return lim


class Drop:
    """A queue_bench.Queue with the doubled arrays of a flagged call."""

    def __init__(self, q):
        import torch

        self.q = q
        nl = q.w.n_links
        self.busy2 = torch.zeros(2 * nl, dtype=torch.int64, device="cuda")
        self.amax2 = torch.zeros(2 * nl, dtype=torch.int32, device="cuda")
        self.limits = {}

    def call(self, carry=False, drop=None):
        """drop: None (unflagged) or the mode whose limits to take ("first", "carried")."""
        q = self.q
        w, f, r, k = q.w, q.bufs, q.rec, q.lnk
        busy, amax = (k[1], k[4]) if drop is None else (self.busy2, self.amax2)
        w.net.link_queue_device(f[0].data_ptr(), q.total, f[3].data_ptr(), f[1].data_ptr(), q.b.wt, q.b.P, q.cost.data_ptr(), 0,
                                wait_ptr=r[0].data_ptr(), done_ptr=r[1].data_ptr(), ahead_ptr=r[2].data_ptr(),
                                link_free_ptr=k[0].data_ptr(), busy_ptr=busy.data_ptr(), wait_max_ptr=k[2].data_ptr(),
                                wait_sum_ptr=k[3].data_ptr(), ahead_max_ptr=amax.data_ptr(), carry=carry,
                                limit_ns=None if drop is None else self.limits[drop])

    def host(self, t):
        return t[:self.q.total].cpu().numpy().view(np.uint64)

    def fractions(self):
        wait, done = self.host(self.q.rec[0]), self.host(self.q.rec[1])
        out = wait == np.uint64(UMAX)
        absent = out & (done == np.uint64(UMAX))
        n = max(self.q.total, 1)
        return round(float((out & ~absent).sum()) / n, 4), round(float(absent.sum()) / n, 4)


def main():
    import torch

    from shadow_amd import default_context, synth

    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_drop_bench.json"))
    a = p.parse_args()
    assert a.runs >= 5 and a.reps >= 3
    os.environ["SG_LINK_COMBINE"] = "0"  # (series_bench's Batch times the plain walk)

    def set_form(serial):
        os.environ["SG_LINK_QUEUE_SERIAL"] = "1" if serial else "0"

    set_form(False)
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
    legs = [(name, Drop(q)) for name, q in legs]

    # warm-up (code objects, workspaces), the limits, the fractions, the forms' agreement
    info = {}
    for name, d in legs:
        q = d.q
        q.trace()
        off = q.bufs[0].cpu().numpy().view(np.uint64)
        r = {"longest_segment": int(np.diff(off.astype(np.int64)).max())}
        for mode, carry in (("first", False), ("carried", True)):
            d.call(carry)
            torch.cuda.synchronize()
            d.limits[mode] = median_limits(off, d.host(q.rec[0]))
            r[f"{mode}_links_limited"] = int((d.limits[mode] != np.uint64(UMAX)).sum())
        d.call(False, "first")
        torch.cuda.synchronize()
        r["first_dropped_fraction"] = d.fractions()[0]
        got = [t.clone() for t in q.rec + q.lnk[:1] + q.lnk[2:4] + [d.busy2, d.amax2]]
        set_form(True)
        d.call(False, "first")
        torch.cuda.synchronize()
        set_form(False)
        same = [t for t in q.rec + q.lnk[:1] + q.lnk[2:4] + [d.busy2, d.amax2]]
        assert all(torch.equal(x, y) for x, y in zip(got, same)), f"{name}: the forms differ"
        d.call(True, "carried")
        torch.cuda.synchronize()
        r["iterations"] = int(ctx.read_timer("link_queue_iters")[1])
        r["carried_dropped_fraction"], r["carried_absent_fraction"] = d.fractions()
        d.call(True)
        torch.cuda.synchronize()
        r["iterations_unlimited"] = int(ctx.read_timer("link_queue_iters")[1])
        info[name] = r
        print(json.dumps({"leg": name, **r}), flush=True)

    keys = ("first", "drop", "drop_serial", "carried", "carried_drop", "index", "sort", "walk", "propagate", "outputs")
    per = {name: {k: [] for k in keys} for name, _ in legs}
    for _ in range(a.runs):
        for name, d in legs:
            ms = {k: [] for k in keys}
            for _ in range(a.reps):
                ms["first"].append(sum(timed(ctx, lambda: d.call(), QUEUE_TIMERS)[0].values()))
                ms["drop"].append(sum(timed(ctx, lambda: d.call(False, "first"), QUEUE_TIMERS)[0].values()))
                set_form(True)
                ms["drop_serial"].append(sum(timed(ctx, lambda: d.call(False, "first"), QUEUE_TIMERS)[0].values()))
                set_form(False)
                ms["carried"].append(sum(timed(ctx, lambda: d.call(True), CARRY_TIMERS)[0].values()))
                got = timed(ctx, lambda: d.call(True, "carried"), CARRY_TIMERS)[0]
                ms["carried_drop"].append(sum(got.values()))
                for k, t in zip(keys[5:], CARRY_TIMERS):
                    ms[k].append(got[t])
            for k in keys:
                per[name][k].append(statistics.median(ms[k]))

    def stat(xs):
        return {"runs_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
                "spread_ms": round(max(xs) - min(xs), 4)}

    cases = []
    for name, d in legs:
        q = d.q
        r = {"leg": name, "nodes": q.w.n, "links": q.w.n_links, "packets": q.b.P, "records": q.total, "cost_ps": COST_PS}
        r.update(info[name])
        r.update({k: stat(per[name][k]) for k in keys})
        it = r["iterations"]
        r["per_iteration_ms"] = {k: round(r[k]["median_ms"] / it, 4) for k in ("sort", "walk", "propagate")}
        gain = r["drop_serial"]["median_ms"] - r["drop"]["median_ms"]
        r["parallel_beats_serial"] = bool(gain > max(r["drop"]["spread_ms"], r["drop_serial"]["spread_ms"]))
        print(json.dumps(r), flush=True)
        cases.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/queue_drop_bench.py", "runs": a.runs, "reps": a.reps, "cases": cases}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
