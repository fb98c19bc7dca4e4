"""A round's link queues at C3 (sg_link_queue on the device trace of sg_link_trace_packets) beside
the trace's own count + fill + sort on the same batch, which is what the queue step adds to, and
beside the lane-per-link form (SG_LINK_QUEUE_SERIAL = 1).

    python tools/queue_bench.py            # JSON to profiles/queue_bench.json

One process on one GPU; any failure ends it, so nothing is started on the GPU after one.  The
worlds, batches and timers are tools/series_bench.py's: the C3 table (10k x 10k) with its pred
rows on the device, a host per node, per batch one delivery round for the statuses; weights are
the payloads, every link costs 8,000 ps a byte (1 Gbit/s).  The legs:
  all, 1M      1M uniform packets, every link;
  watch16, 1M  the same batch, the 16 busiest links;
  hot          the 512-spoke star, 100k packets from one spoke across the hub (a link of 100k
               records);
  all, 100k / all, 10k.
The legs are alternated `--runs` times; inside a run every leg is timed `--reps` times with the
library's timers and gives its median.  Reported per leg: the median over the runs of each run's
median and the spread (max - min over the runs) of the trace's three kernels, of the scan form
("link_queue" + "link_queue_ahead", all eight outputs) and of the lane-per-link form; the bytes
the scan must move (enter_ns, packet and the gathered weight read twice, the outputs written once;
the ahead kernel's reads of done are not counted) and what fraction of 6.3 TB/s that is at the
measured time.  Every leg asserts that the two forms agree bit for bit.  Correctness is
tests/test_queue_gpu.py's; bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from series_bench import TRACE_TIMERS, Batch, World, star_graph, timed  # noqa: E402

COST_PS = 8000
HBM_BYTES_PER_S = 6.3e12
QUEUE_TIMERS = ("link_queue", "link_queue_ahead")


class Queue:
    """A batch's device trace and the arrays of one sg_link_queue call over it."""

    def __init__(self, b, watched):
        import torch

        w = self.w = b.w
        self.b, self.watched = b, watched
        one = torch.zeros(2, dtype=torch.int64, device="cuda")
        loff = torch.zeros(w.n_links + 1, dtype=torch.int64, device="cuda")
        args = (w.ht, w.nodes, 0, w.n, w.pred.data_ptr(), w.lat.data_ptr(), b.pb, b.st, b.watch16.data_ptr() if watched else 0)
        self.total = w.net.link_trace_packets_device(*args, loff.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(),
                                                     one.data_ptr(), 0)[1]
        t = max(self.total, 1)
        self.bufs = [loff] + [torch.zeros(t, dtype=d, device="cuda") for d in (torch.int32, torch.int32, torch.int64, torch.int64)]
        self.cost = torch.full((w.n_links,), COST_PS, dtype=torch.int64, device="cuda")
        self.rec = [torch.zeros(t, dtype=d, device="cuda") for d in (torch.int64, torch.int64, torch.int32)]
        self.lnk = [torch.zeros(w.n_links, dtype=d, device="cuda")
                    for d in (torch.int64, torch.int64, torch.int64, torch.int64, torch.int32)]
        self.longest = 0

    def trace(self):
        return self.b.trace(self.watched, self.bufs)

    def queue(self):
        w, f, r, k = self.w, self.bufs, self.rec, self.lnk
        w.net.link_queue_device(f[0].data_ptr(), self.total, f[3].data_ptr(), f[1].data_ptr(), self.b.wt, self.b.P,
                                self.cost.data_ptr(), 0, wait_ptr=r[0].data_ptr(), done_ptr=r[1].data_ptr(),
                                ahead_ptr=r[2].data_ptr(), link_free_ptr=k[0].data_ptr(), busy_ptr=k[1].data_ptr(),
                                wait_max_ptr=k[2].data_ptr(), wait_sum_ptr=k[3].data_ptr(), ahead_max_ptr=k[4].data_ptr())

    def bytes_moved(self):
        return self.total * (2 * (8 + 4 + 4) + 8 + 8 + 4) + self.w.n_links * (4 * 8 + 4)


def main():
    import torch

    from shadow_amd import default_context, synth

    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_bench.json"))
    a = p.parse_args()
    assert a.runs >= 5 and a.reps >= 3
    os.environ["SG_LINK_COMBINE"] = "0"  # (series_bench's Batch times the plain walk)
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

    def set_form(serial):
        os.environ["SG_LINK_QUEUE_SERIAL"] = "1" if serial else "0"

    # warm-up (code objects, workspaces) and the check: the forms agree bit for bit
    for name, q in legs:
        q.trace()
        got = []
        for serial in (False, True):
            set_form(serial)
            q.queue()
            torch.cuda.synchronize()
            got.append([t.clone() for t in q.rec + q.lnk])
        assert all(torch.equal(x, y) for x, y in zip(*got)), f"{name}: the forms differ"
        q.longest = int(torch.diff(q.bufs[0]).max())
        q.waiting = int((q.rec[0][:q.total] > 0).sum())
        q.deepest = int(q.lnk[4].max())

    per = {name: {"trace": [], "scan": [], "serial": []} for name, _ in legs}
    for _ in range(a.runs):
        for name, q in legs:
            ms = {"trace": [], "scan": [], "serial": []}
            for _ in range(a.reps):
                ms["trace"].append(timed(ctx, q.trace, TRACE_TIMERS))
                for serial in (False, True):
                    set_form(serial)
                    ms["serial" if serial else "scan"].append(timed(ctx, q.queue, QUEUE_TIMERS))
            for k in ms:
                per[name][k].append(statistics.median(ms[k]))
    set_form(False)

    def stat(xs):
        return {"runs_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
                "spread_ms": round(max(xs) - min(xs), 4)}

    cases = []
    for name, q in legs:
        r = {"leg": name, "nodes": q.w.n, "links": q.w.n_links, "packets": q.b.P, "records": q.total,
             "longest_segment": q.longest, "records_waiting": q.waiting, "deepest_queue": q.deepest, "cost_ps": COST_PS}
        r.update({k: stat(per[name][k]) for k in ("trace", "scan", "serial")})
        r["scan_bytes"] = q.bytes_moved()
        r["scan_hbm_fraction"] = round(r["scan_bytes"] / (r["scan"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
        print(json.dumps(r), flush=True)
        cases.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/queue_bench.py", "runs": a.runs, "reps": a.reps, "cases": cases}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
