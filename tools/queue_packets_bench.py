"""A round's link queues folded onto its packets at C3 (sg_link_queue with SG_LINK_QUEUE_PACKETS on the
device trace of sg_link_trace_packets) beside the same calls without the bit.

    python tools/queue_packets_bench.py       # JSON to profiles/queue_packets_bench.json

One process on one GPU; any failure ends it, so nothing is started on the GPU after one.  The
worlds, batches and legs are tools/queue_bench.py's: 8,000 ps a byte (1 Gbit/s) on every link,
payload weights, all eight outputs.  Base times are the delivery round's deliver_time_ns.  Three
modes: first order, carried, and carried with the median-wait limits of tools/queue_drop_bench.py
(computed once, outside the timed region).  The legs are alternated `--runs` times; inside a run
every column is timed `--reps` times and gives its median.  Reported per leg and mode, as the median
over the runs of each run's median with the spread (max - min over the runs), device time by the
library's timers:
  plain          the call without the bit, all its timers;
  packets        the call with the bit, all its timers ("link_queue_packets" among them);
  pass           "link_queue_packets" alone;
and first order also the pass through the carried form's index step (SG_LINK_QUEUE_PACKETS_INDEX = 1):
  packets_index  the call, and pass_index = "link_queue_index" + "link_queue_packets".
No cost is fixed in advance: the bit's cost is `packets` against `plain`.  pass_bytes is what the pass
must move (carried: 32 B a record -- packet, wait, done, enter, next -- first order 28 B a record and
12 B of atomics' operands; 28 B written and 8 B read a packet in either, twice where two kernels
visit the packets), and pass_hbm_fraction that over the pass's time as a fraction of 6.3 TB/s.
Every leg asserts that the two first-order forms agree bit for bit and that the bit leaves the
first n_records entries and the per-link arrays alone.  On the 1M-packet leg sg_wire_push is timed
with the delivery's own times and with the carried, limited arrive tail ("wire_push").
Correctness is tests/test_outcomes_gpu.py's; bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from queue_bench import COST_PS, HBM_BYTES_PER_S, Queue  # noqa: E402
from queue_carry_bench import CARRY_TIMERS, timed  # noqa: E402
from queue_drop_bench import UMAX, median_limits  # noqa: E402
from series_bench import Batch, World, star_graph  # noqa: E402

PASS = "link_queue_packets"
TIMERS = CARRY_TIMERS + (PASS,)
MODES = (("first", False, False), ("carried", True, False), ("carried_drop", True, True))


class Packets:
    """A queue_bench.Queue with the per-record arrays a call with the bit takes: the packets behind
    the records, the delivery's times behind enter's."""

    def __init__(self, q):
        import torch

        self.q = q
        n, P, nl = q.total, q.b.P, q.w.n_links
        self.enter = torch.zeros(n + P, dtype=torch.int64, device="cuda")
        self.rec = [torch.zeros(n + P, dtype=d, device="cuda") for d in (torch.int64, torch.int64, torch.int32)]
        self.busy2 = torch.zeros(2 * nl, dtype=torch.int64, device="cuda")
        self.amax2 = torch.zeros(2 * nl, dtype=torch.int32, device="cuda")
        self.limits = None

    def trace(self):
        q = self.q
        q.trace()
        self.enter[:q.total].copy_(q.bufs[3][:q.total])
        self.enter[q.total:].copy_(q.b.out.deliver_time_ns[:q.b.P])

    def call(self, carry, drop, bit):
        q = self.q
        w, f, r, k = q.w, q.bufs, self.rec, q.lnk
        busy, amax = (self.busy2, self.amax2) if drop else (k[1], k[4])
        w.net.link_queue_device(f[0].data_ptr(), q.total, self.enter.data_ptr(), f[1].data_ptr(), q.b.wt, q.b.P, q.cost.data_ptr(), 0,
                                wait_ptr=r[0].data_ptr(), done_ptr=r[1].data_ptr(), ahead_ptr=r[2].data_ptr(),
                                link_free_ptr=k[0].data_ptr(), busy_ptr=busy.data_ptr(), wait_max_ptr=k[2].data_ptr(),
                                wait_sum_ptr=k[3].data_ptr(), ahead_max_ptr=amax.data_ptr(), carry=carry,
                                limit_ns=self.limits if drop else None, outcomes=bit)

    def outputs(self, drop):
        k = self.q.lnk
        return self.rec + [k[0], k[2], k[3]] + ([self.busy2, self.amax2] if drop else [k[1], k[4]])


def pass_bytes(n, P, carry):
    per_packet = 28 + 8
    return n * 32 + P * per_packet + P * 20 if carry else n * (28 + 12) + 2 * P * per_packet


def main():
    import torch

    from shadow_amd import default_context, synth
    from shadow_amd.wire import PacketWire

    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_packets_bench.json"))
    a = p.parse_args()
    assert a.runs >= 5 and a.reps >= 3
    os.environ["SG_LINK_COMBINE"] = "0"  # (series_bench's Batch times the plain walk)
    os.environ["SG_LINK_QUEUE_SERIAL"] = "0"

    def set_index(on):
        os.environ["SG_LINK_QUEUE_PACKETS_INDEX"] = "1" if on else "0"

    set_index(False)
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
    legs = [(name, Packets(q)) for name, q in legs]

    # warm-up (code objects, workspaces), the limits, the agreement of the forms and of the bit
    info = {}
    for name, d in legs:
        q = d.q
        d.trace()
        nrec = q.total
        off = q.bufs[0].cpu().numpy().view(np.uint64)
        d.call(True, False, False)
        torch.cuda.synchronize()
        d.limits = median_limits(off, d.rec[0][:nrec].cpu().numpy().view(np.uint64))
        r = {"links_limited": int((d.limits != np.uint64(UMAX)).sum())}
        for mode, carry, drop in MODES:
            d.call(carry, drop, False)
            torch.cuda.synchronize()
            plain = [t.clone() for t in d.outputs(drop)]
            d.call(carry, drop, True)
            torch.cuda.synchronize()
            got = d.outputs(drop)
            assert all(torch.equal(x[:nrec] if k < 3 else x, y[:nrec] if k < 3 else y)
                       for k, (x, y) in enumerate(zip(got, plain))), f"{name}, {mode}: the bit changed an output"
            where = d.rec[2][nrec:]
            r[f"{mode}_lost"] = int(ctx.read_timer("link_queue_lost")[1])
            assert r[f"{mode}_lost"] == int((where.view(torch.int32) >= 0).sum())  # (a record index; the two codes are negative)
            r[f"{mode}_no_record"] = int((where == -1).sum())
            if carry:
                r[f"{mode}_iterations"] = int(ctx.read_timer("link_queue_iters")[1])
            else:
                tails = [t[nrec:].clone() for t in d.rec]
                set_index(True)
                d.call(carry, drop, True)
                torch.cuda.synchronize()
                set_index(False)
                assert all(torch.equal(t[nrec:], x) for t, x in zip(d.rec, tails)), f"{name}: the first-order forms differ"
        info[name] = r
        print(json.dumps({"leg": name, **r}), flush=True)

    cols = ["plain", "packets", "pass"]
    keys = [f"{m}_{c}" for m, _, _ in MODES for c in cols] + ["first_packets_index", "first_pass_index"]
    per = {name: {k: [] for k in keys} for name, _ in legs}
    for _ in range(a.runs):
        for name, d in legs:
            ms = {k: [] for k in keys}
            for _ in range(a.reps):
                for mode, carry, drop in MODES:
                    ms[f"{mode}_plain"].append(sum(timed(ctx, lambda: d.call(carry, drop, False), CARRY_TIMERS)[0].values()))
                    got = timed(ctx, lambda: d.call(carry, drop, True), TIMERS)[0]
                    ms[f"{mode}_packets"].append(sum(got.values()))
                    ms[f"{mode}_pass"].append(got[PASS])
                set_index(True)
                got = timed(ctx, lambda: d.call(False, False, True), TIMERS)[0]
                set_index(False)
                ms["first_packets_index"].append(sum(got.values()))
                ms["first_pass_index"].append(got[PASS] + got["link_queue_index"])
            for k in keys:
                per[name][k].append(statistics.median(ms[k]))

    def stat(xs):
        return {"runs_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
                "spread_ms": round(max(xs) - min(xs), 4)}

    # the wire on the 1M leg: the delivery's own times, then the carried, limited arrive tail
    d = legs[0][1]
    b = d.q.b
    d.call(True, True, True)
    torch.cuda.synchronize()
    arrive = d.rec[1][d.q.total:].clone()
    length = (b.pb.payload_len + 28).contiguous()
    wire = PacketWire(c3.n, 2 * b.P, 10**6, 64, ctx=ctx)
    push = {"plain": [], "rates": []}
    events = {}
    for _ in range(a.runs):
        for k, times in (("plain", None), ("rates", arrive)):
            ms = []
            for _ in range(a.reps):
                ms.append(timed(ctx, lambda: wire.push(b.pb, b.out, length, deliver_time_ns=times), ("wire_push",))[0]["wire_push"])
                events[k] = int(wire.pop(2**64 - 1)["n"])
                assert wire.count == 0
            push[k].append(statistics.median(ms))
    assert events["rates"] == events["plain"] - info["all, 1M"]["carried_drop_lost"]

    cases = []
    for name, d in legs:
        q = d.q
        r = {"leg": name, "nodes": q.w.n, "links": q.w.n_links, "packets": q.b.P, "records": q.total, "cost_ps": COST_PS}
        r.update(info[name])
        r.update({k: stat(per[name][k]) for k in keys})
        for mode, carry, _ in MODES:
            r[f"{mode}_bit_costs_ms"] = round(r[f"{mode}_packets"]["median_ms"] - r[f"{mode}_plain"]["median_ms"], 4)
            r[f"{mode}_pass_bytes"] = pass_bytes(q.total, q.b.P, carry)
            r[f"{mode}_pass_hbm_fraction"] = round(r[f"{mode}_pass_bytes"] / (r[f"{mode}_pass"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
        r["first_form"] = "atomics" if r["first_pass"]["median_ms"] <= r["first_pass_index"]["median_ms"] else "index"
        if name == "all, 1M":
            r["wire_push_plain"], r["wire_push_rates"] = stat(push["plain"]), stat(push["rates"])
            r["wire_events_plain"], r["wire_events_rates"] = events["plain"], events["rates"]
        print(json.dumps(r), flush=True)
        cases.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/queue_packets_bench.py", "runs": a.runs, "reps": a.reps, "cases": cases}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
