"""The link-queue series at C3 (sg_link_queue with SG_LINK_QUEUE_SERIES) beside the call as it is.

    python tools/queue_series_bench.py      # JSON to profiles/queue_series_bench.json

One process on one GPU; any failure ends it, so nothing is started on the GPU after one.  The worlds,
batches and legs are tools/queue_bench.py's: 8,000 ps a byte (1 Gbit/s) on every link, payload
weights, all eight outputs.  Every leg runs first order, carried, and carried under the median limits
of tools/queue_drop_bench.py, each under four shapes of the matrix over the span of the leg's times:
  all links, 64 bins; all links, 1,024 bins (dropped where the matrix and its difference array pass
  `--max-gib`, and said so); 16 slots (the links with the most records), 64 bins; 16 slots, 65,536 bins.
Per (leg, form, shape), alternated `--runs` times, each the median of `--reps`: the call's wall time
without the bit and with it (a device synchronisation at both ends; both go through
NetworkGraph.link_queue_device, the timers off) and the pass alone by its timer, "link_queue_series",
in a third call.  Reported as
the median over the runs with the spread (max - min).  Further:
  pass_hbm_fraction   the pass's bytes (records x 24 B, the matrix and the difference array read and
                      written once) over its time, as a share of 6.3 TB/s.  An upper bound of the
                      traffic: a cell whose count is 0 is neither read nor written in the matrix, so
                      with many cells and few records the figure passes 1;
  extra_wall_ms       with - without - pass: the header's read-back (one more synchronisation in device
                      mode), the tail's copy behind cost_ps and the per-link values' copy, in Python;
  span_check          16 slots: the pass at 65,536 bins against 64 bins: the cost of a record must not
                      follow the bins its wait spans;
  host_route          at 1M packets, first order: wait_ns and done_ns downloaded and binned with numpy
                      (busy and waiting time per link and bin by a difference array), what the pass
                      replaces.
The first run asserts per shape that plane 0 and plane 1 sum to the call's per-link busy and wait sums.
Nothing is fixed in advance.  Correctness is tests/test_queue_series_gpu.py's; bench.py stays the
project's headline benchmark."""
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

from queue_bench import COST_PS, HBM_BYTES_PER_S, Queue  # noqa: E402
from queue_drop_bench import Drop, median_limits  # noqa: E402
from series_bench import Batch, World, star_graph  # noqa: E402

FORMS = ("first", "carried", "carried_limits")
SHAPES = (("all, 64", None, 64), ("all, 1024", None, 1024), ("16 slots, 64", 16, 64), ("16 slots, 65536", 16, 65536))


def wall(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


class Leg:
    def __init__(self, ctx, name, q):
        self.ctx, self.name, self.q, self.d = ctx, name, q, Drop(q)
        self.series = {}

    def call(self, form, series=None):
        import torch

        q, d = self.q, self.d
        w, f, r, k = q.w, q.bufs, q.rec, q.lnk
        drop = form == "carried_limits"
        busy, amax = (d.busy2, d.amax2) if drop else (k[1], k[4])
        w.net.link_queue_device(f[0].data_ptr(), q.total, f[3].data_ptr(), f[1].data_ptr(), q.b.wt, q.b.P, q.cost.data_ptr(), 0,
                                wait_ptr=r[0].data_ptr(), done_ptr=r[1].data_ptr(), ahead_ptr=r[2].data_ptr(),
                                link_free_ptr=k[0].data_ptr(), busy_ptr=busy.data_ptr(), wait_max_ptr=k[2].data_ptr(),
                                wait_sum_ptr=k[3].data_ptr(), ahead_max_ptr=amax.data_ptr(), carry=form != "first",
                                limit_ns=d.limits["carried"] if drop else None, series=series)
        torch.cuda.synchronize()

    def span(self):
        """(first enter, last done + 1) of the carried call without limits, the latest the leg sees."""
        import torch

        t = self.q.total
        sign = torch.tensor(-2**63, dtype=torch.int64, device="cuda")
        done = self.q.rec[1][:t]
        return int((self.q.bufs[3][:t] ^ sign).min() ^ sign), int((done ^ sign).max() ^ sign) + 1

    def make_series(self, shape, lo, hi, max_bytes):
        from shadow_amd import LinkQueueSeries

        name, slots, bins = shape
        nl = self.q.w.n_links
        S = nl if slots is None else slots
        size = (4 * S * (bins + 2) + 2 * S * (bins + 1)) * 8
        if size > max_bytes:
            return None, size
        watch = None
        if slots is not None:
            import torch

            watch = torch.argsort(torch.diff(self.q.bufs[0]), descending=True)[:slots].cpu().numpy()
        return LinkQueueSeries(self.q.w.net, lo, max((hi - lo + bins - 1) // bins, 1), bins, watch=watch), size


def host_route(leg, lo, bin_ns, bins):
    """Busy and waiting time per link and bin from downloaded wait_ns and done_ns, with numpy: (download ms,
    binning ms)."""
    import torch

    q = leg.q
    t = q.total
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wait = q.rec[0][:t].cpu().numpy().view(np.uint64)
    done = q.rec[1][:t].cpu().numpy().view(np.uint64)
    off = q.bufs[0].cpu().numpy().astype(np.int64)
    pkt = q.bufs[1][:t].cpu().numpy().astype(np.int64)
    wt = q.b.pb.payload_len.cpu().numpy().view(np.uint32).astype(np.uint64)
    t1 = time.perf_counter()
    nl = len(off) - 1
    link = np.repeat(np.arange(nl), np.diff(off))
    s = (wt[pkt] * np.uint64(COST_PS) + np.uint64(999)) // np.uint64(1000)
    start = done - s
    enter = start - wait
    out = []
    for a, b in ((start, done), (enter, start)):
        M = np.zeros((nl, bins + 1), np.int64)
        x, y = (a - np.uint64(lo)).astype(np.int64), (b - np.uint64(lo)).astype(np.int64)
        qx, qy = np.minimum(x // bin_ns, bins), np.minimum(y // bin_ns, bins)
        same = qx == qy
        np.add.at(M, (link[same], qx[same]), (y - x)[same])
        d = ~same
        np.add.at(M, (link[d], qx[d]), ((qx + 1) * bin_ns - x)[d])
        np.add.at(M, (link[d], qy[d]), (y - qy * bin_ns)[d])
        D = np.zeros((nl, bins + 2), np.int64)
        np.add.at(D, (link[d], qx[d] + 1), 1)
        np.add.at(D, (link[d], qy[d]), -1)
        M[:, :bins] += np.cumsum(D[:, :bins], axis=1) * bin_ns
        out.append(M)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, out


def main():
    import torch

    from shadow_amd import default_context, synth

    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--max-gib", type=float, default=8.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_series_bench.json"))
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
    legs = [Leg(ctx, "all, 1M", Queue(batches[1_000_000], False)), Leg(ctx, "watch16, 1M", Queue(batches[1_000_000], True)),
            Leg(ctx, "hot link, 100k", Queue(hot, True)), Leg(ctx, "all, 100k", Queue(batches[100_000], False)),
            Leg(ctx, "all, 10k", Queue(batches[10_000], False))]

    # warm-up, the limits, the span, the matrices and the identities
    skipped = {}
    for leg in legs:
        q = leg.q
        q.trace()
        leg.call("carried")
        off = q.bufs[0].cpu().numpy().view(np.uint64)
        leg.d.limits["carried"] = median_limits(off, leg.d.host(q.rec[0]))
        lo, hi = leg.span()
        for shape in SHAPES:
            s, size = leg.make_series(shape, lo, hi, a.max_gib * 2**30)
            if s is None:
                skipped[f"{leg.name} / {shape[0]}"] = f"matrix and difference array of {size / 2**30:.1f} GiB"
                continue
            leg.series[shape[0]] = s
            for form in FORMS:
                s.reset()
                leg.call(form, s)
                M = s.planes()
                slot = np.arange(q.w.n_links) if s.link_slot is None else s.link_slot
                watched = slot != np.uint64(0xFFFFFFFFFFFFFFFF)
                busy = (leg.d.busy2 if form == "carried_limits" else q.lnk[1])[:q.w.n_links].cpu().numpy().view(np.uint64)
                wsum = q.lnk[3].cpu().numpy().view(np.uint64)
                for plane, per_link in ((0, busy), (1, wsum)):
                    want = np.zeros(s.n_slots, np.uint64)
                    np.add.at(want, slot[watched].astype(np.int64), per_link[watched])
                    assert np.array_equal(M[plane].sum(axis=1, dtype=np.uint64), want), (leg.name, shape[0], form, plane)
    print(json.dumps({"skipped": skipped}), flush=True)

    keys = ("without", "with", "pass")
    per = {}
    for run in range(a.runs):
        for leg in legs:
            for form in FORMS:
                for shape, s in leg.series.items():
                    ms = {k: [] for k in keys}
                    for _ in range(a.reps):
                        ms["without"].append(wall(lambda: leg.call(form)))
                        ms["with"].append(wall(lambda: leg.call(form, s)))
                        ctx.enable_timers(True)  # (a call of its own: the timers' events cost wall time)
                        try:
                            leg.call(form, s)
                            ms["pass"].append(ctx.read_timer("link_queue_series")[0])
                        finally:
                            ctx.enable_timers(False)
                    for k in keys:
                        per.setdefault((leg.name, form, shape), {k: [] for k in keys})[k].append(statistics.median(ms[k]))
        print(json.dumps({"run": run}), flush=True)

    def stat(xs):
        return {"runs_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
                "spread_ms": round(max(xs) - min(xs), 4)}

    cases = []
    for leg in legs:
        for form in FORMS:
            for shape, s in leg.series.items():
                r = {"leg": leg.name, "form": form, "shape": shape, "records": leg.q.total, "links": leg.q.w.n_links,
                     "slots": s.n_slots, "bins": s.n_bins, "bin_ns": s.bin_ns}
                r.update({k: stat(v) for k, v in per[(leg.name, form, shape)].items()})
                r["pass_bytes"] = leg.q.total * 24 + 2 * 8 * (4 * s.cells + 2 * s.n_slots * (s.n_bins + 1))
                r["pass_hbm_fraction"] = round(r["pass_bytes"] / (max(r["pass"]["median_ms"], 1e-6) * 1e-3) / HBM_BYTES_PER_S, 4)
                r["extra_wall_ms"] = round(r["with"]["median_ms"] - r["without"]["median_ms"] - r["pass"]["median_ms"], 4)
                cases.append(r)
                print(json.dumps(r), flush=True)

    span_check = []
    for leg in legs:
        for form in FORMS:
            lo_, hi_ = per.get((leg.name, form, "16 slots, 64")), per.get((leg.name, form, "16 slots, 65536"))
            if lo_ and hi_:
                a64, a64k = stat(lo_["pass"]), stat(hi_["pass"])
                span_check.append({"leg": leg.name, "form": form, "pass_64_ms": a64["median_ms"], "pass_65536_ms": a64k["median_ms"],
                                   "spreads_ms": round(a64["spread_ms"] + a64k["spread_ms"], 4),
                                   "within_spreads": a64k["median_ms"] - a64["median_ms"] <= a64["spread_ms"] + a64k["spread_ms"]})
    leg = legs[0]
    leg.call("first")
    s = leg.series["all, 64"]
    down, binning, got = host_route(leg, s.t0_ns, s.bin_ns, s.n_bins)
    s.reset()
    leg.call("first", s)
    M = s.planes()
    assert np.array_equal(got[0][:, :64].astype(np.uint64), M[0, :, :64]) and np.array_equal(got[1][:, :64].astype(np.uint64), M[1, :, :64])
    host = {"leg": leg.name, "form": "first", "shape": "all, 64", "download_ms": round(down, 3), "numpy_binning_ms": round(binning, 3),
            "pass_ms": stat(per[(leg.name, "first", "all, 64")]["pass"])["median_ms"]}
    print(json.dumps({"span_check": span_check, "host_route": host}), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/queue_series_bench.py", "runs": a.runs, "reps": a.reps, "skipped": skipped, "cases": cases,
                   "span_check": span_check, "host_route": host}, f, indent=1)
        f.write("\n")
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
