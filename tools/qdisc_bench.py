#!/usr/bin/env python3
"""Cost of the interface's round-robin qdisc (sg_qdisc.hip) against the fifo one (k_outbound) on
the C4 outbound leg's sends.

bench.py's outbound_leg volume: 100k hosts, 1M sends in one 1 ms window, every host's bandwidth
up 1 Gbit/s.  The same sends run, in one process on one device, through
  fifo    a fifo object (sg_outbound_run: k_outbound + k_out_compact), the baseline
  rr4     a round-robin object with 4 socket slots per host (socket state in LDS)
  rr64    a round-robin object with 64 (socket state in global memory)
alternating, a fresh object per step (the leg's steady state is an empty interface), and the
library's `outbound` and `out_compact` timers (HIP events on the context stream) are read after
every step.  The round-robin legs are reported as ratios to the fifo leg's mean.

    python tools/qdisc_bench.py --out profiles/qdisc_bench.json

--throttled BITS adds the three legs once more at that bandwidth up (queues build and drain,
the relays block), four consecutive windows on the same objects.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T0 = 946684800 * 10**9
MS = 10**6
BW_UP_BITS = 10**9
HDR_BYTES = 40
LEGS = (("fifo", "fifo", 1), ("rr4", "round-robin", 4), ("rr64", "round-robin", 64))


def stats(xs):
    a = np.asarray(xs, float)
    return dict(mean=float(a.mean()), median=float(np.median(a)), std=float(a.std()), min=float(a.min()),
                max=float(a.max()), n=int(a.size))


def timers(ctx):
    return {k: ctx.read_timer(k) for k in ("outbound", "out_compact")}


def run_leg(a, torch, ctx, hosts, bw_bits, windows):
    from shadow_amd import synth
    from shadow_amd.router import OutboundPipeline

    H = hosts["n"]
    dev = lambda x, dt, tv: torch.from_numpy(np.ascontiguousarray(x, dtype=dt).view(tv)).cuda()
    wins = []
    for w in range(windows):
        pk = synth.make_packets(a.packets, hosts, T0 + w * MS, T0 + (w + 1) * MS, seed=100 + w)
        n = len(pk["src"])
        rng = np.random.default_rng(7 + w)
        wins.append(dict(
            args=(dev(pk["src"], np.uint32, np.int32), dev(pk["send_time"], np.uint64, np.int64),
                  dev(np.arange(w * n, (w + 1) * n), np.uint32, np.int32),
                  dev(pk["payload"] + HDR_BYTES, np.uint32, np.int32), dev(pk["payload"], np.uint32, np.int32),
                  dev(pk["dst_ip"], np.uint32, np.int32)),
            sock={S: dev(rng.integers(0, S, n), np.uint32, np.int32) for _, _, S in LEGS},
            end=T0 + (w + 1) * MS, deepest=int(np.bincount(pk["src"], minlength=H).max(initial=0))))
    n_pk = a.packets * windows
    fwd = torch.full((n_pk,), -1, dtype=torch.int64, device="cuda")
    status = torch.zeros(n_pk, dtype=torch.uint8, device="cuda")
    cap = 64
    while cap < windows * max(w["deepest"] for w in wins):
        cap *= 2
    bw = np.full(H, bw_bits, np.uint64)
    rows = {name: dict(outbound=[], out_compact=[], sent=[]) for name, _, _ in LEGS}
    for k in range(a.warmup + a.steps):
        if k == a.warmup:
            ctx.enable_timers(True)
        for name, qdisc, S in LEGS:  # alternated: the legs share whatever the device does meanwhile
            ob = OutboundPipeline(hosts["ip"], bw, cap, ctx=ctx, qdisc=qdisc, max_sockets=S)
            ob.sent_buffers(a.packets + 4 * H, "cuda")
            status.zero_()
            t_out = t_cmp = 0.0
            sent = 0
            for w in wins:
                before = timers(ctx) if k >= a.warmup else None
                batch, _ = ob.run(*w["args"], w["end"], 0, 2**63, fwd, status,
                                  socket=None if qdisc == "fifo" else w["sock"][S])
                sent += len(batch)
                if before is not None:
                    after = timers(ctx)
                    t_out += after["outbound"][0] - before["outbound"][0]
                    t_cmp += after["out_compact"][0] - before["out_compact"][0]
            if k >= a.warmup:
                rows[name]["outbound"].append(t_out * 1e3)      # us per window set
                rows[name]["out_compact"].append(t_cmp * 1e3)
                rows[name]["sent"].append(sent)
            del ob
    ctx.enable_timers(False)
    res = dict(bw_up_bits=int(bw_bits), windows=windows, ring_cap=cap, hosts=H, sends_per_window=a.packets)
    for name, _, S in LEGS:
        r = rows[name]
        res[name] = dict(max_sockets=S, outbound_us=stats(r["outbound"]), out_compact_us=stats(r["out_compact"]),
                         sent=int(r["sent"][-1]))
    base = res["fifo"]["outbound_us"]["mean"]
    base_c = res["fifo"]["out_compact_us"]["mean"]
    for name in ("rr4", "rr64"):
        res[name]["outbound_ratio_to_fifo"] = round(res[name]["outbound_us"]["mean"] / base, 3)
        res[name]["out_compact_ratio_to_fifo"] = round(res[name]["out_compact_us"]["mean"] / max(base_c, 1e-9), 3)
        res[name]["both_ratio_to_fifo"] = round(
            (res[name]["outbound_us"]["mean"] + res[name]["out_compact_us"]["mean"]) / (base + base_c), 3)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--hosts", type=int, default=100000)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--packets", type=int, default=1000000)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--throttled", type=int, default=0, help="also run at this bandwidth up (bits/s), 4 windows")
    p.add_argument("--out", default="")
    a = p.parse_args()
    import torch

    import shadow_amd
    from shadow_amd import synth

    shadow_amd.load()
    ctx = shadow_amd.default_context(0)
    hosts = synth.make_hosts(a.hosts, a.nodes, general_seed=1, exact_seeds=True)
    res = dict(device=torch.cuda.get_device_name(0), timers="HIP events on the context stream",
               c4=run_leg(a, torch, ctx, hosts, BW_UP_BITS, 1))
    if a.throttled:
        res["throttled"] = run_leg(a, torch, ctx, hosts, a.throttled, 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
