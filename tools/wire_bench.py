#!/usr/bin/env python3
"""Steady-state cost of the packet wire (sg_wire_push / sg_wire_pop) under C4-shaped rounds.

100k hosts, 1M packets per 1 ms round; path latencies uniform in [1 ms, L]: the wire then
holds about packets x L / 2 ms events.  Three legs at the same batch size:
  P10M      L = 20 ms, 128 bins of 1 ms (the far list stays empty)
  P40M      L = 80 ms, 128 bins of 1 ms (the far list stays empty)
  P40M_far  L = 80 ms,  32 bins of 1 ms (most events wait on the far list, re-binned every 16 rounds)
Each leg warms up until the store is in steady state, then times rounds with the library's
per-kernel timers (HIP events on the context stream, read after every round): wire_push,
wire_pop, and the same round's delivery kernels (walk + bucketing) as the yardstick.  The design
condition under test: a round's wire time depends on what it pushes and pops, not on what the
store holds, so P40M / P10M should be 1 within the spread.

    python tools/wire_bench.py --out profiles/wire_bench.json

A fourth leg, not in the default list, compares the two ways into the wire on P10M's volume and
geometry with W = 1 (every record is local), both in every timed round of one run:
  P10M_records  old: sg_deliver_round + sg_wire_push
                new: sg_deliver_source + sg_wire_stamp_records + sg_wire_push_records
Each path has its own hosts table and wire, fed the same batches (so both hold the same events);
the wire_push timer is read around each path's push, wire_stamp around the stamp.

    python tools/wire_bench.py --legs P10M_records --out profiles/wire_bench_records.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T0 = 946684800 * 10**9
MS = 10**6
DELIVERY_TIMERS = ("walk", "scatter", "scatter2", "sort_small", "sort_big", "seg_bounds")
RECORD_BYTES = 32


def stats(xs):
    a = np.asarray(xs, float)
    return dict(mean=float(a.mean()), std=float(a.std()), min=float(a.min()), max=float(a.max()), n=int(a.size))


def leg(name, a, torch, ctx, lat_max_ms, n_bins, capacity):
    from shadow_amd import synth
    from shadow_amd.wire import PacketWire
    from shadow_amd.worker import DeviceTable, Deliveries, HostTable, PacketBatch, deliver_round

    rng = np.random.default_rng(11)
    hosts = synth.make_hosts(a.hosts, a.nodes, exact_seeds=False)
    lat = rng.integers(MS, lat_max_ms * MS + 1, (a.nodes, a.nodes)).astype(np.uint64)
    loss = (rng.random((a.nodes, a.nodes)) * 0.02).astype(np.float32)
    ht = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    table = DeviceTable(torch.from_numpy(lat.view(np.int64).ravel()).cuda(), torch.from_numpy(loss.ravel()).cuda(),
                        a.nodes)
    table.pack(ctx)
    # a few distinct batches, reused in turn with their send times moved to the round
    batches = []
    for s in range(4):
        pk = synth.make_packets(a.packets, hosts, 0, MS, seed=50 + s)
        batches.append((PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"]),
                        torch.from_numpy(pk["send_time"].view(np.int64)).cuda(),
                        torch.from_numpy((pk["payload"] + 28).astype(np.uint32).view(np.int32)).cuda()))
    out = Deliveries.allocate(a.packets, a.hosts)
    wire = PacketWire(a.hosts, capacity, MS, n_bins, ctx=ctx)
    warm = lat_max_ms + 8
    cap = 2 * a.packets
    rows = []
    names = ("wire_push", "wire_pop") + DELIVERY_TIMERS
    for k in range(warm + a.rounds):
        batch, rel, length = batches[k % len(batches)]
        batch.send_time_ns.copy_(rel + (T0 + k * MS))
        end = T0 + (k + 1) * MS
        if k == warm:
            ctx.enable_timers(True)
        prev = {n: ctx.read_timer(n) for n in names} if k >= warm else None
        t0 = time.perf_counter()
        deliver_round(ht, table, batch, end, 2**63, 0, out=out, ctx=ctx)
        t1 = time.perf_counter()
        wire.push(batch, out, length, id_base=0)
        got = wire.pop(end, cap=cap)
        t2 = time.perf_counter()
        if k >= warm:
            now = {n: ctx.read_timer(n) for n in names}
            d = {n: now[n][0] - prev[n][0] for n in names}
            rows.append(dict(round=k, delivered=int(out.n_delivered), popped=got["n"], held=wire.count,
                             push_ms=d["wire_push"], pop_ms=d["wire_pop"],
                             pushed_bytes=now["wire_push"][2] - prev["wire_push"][2],
                             popped_bytes=now["wire_pop"][2] - prev["wire_pop"][2],
                             delivery_kernels_ms=sum(d[n] for n in DELIVERY_TIMERS), walk_ms=d["walk"],
                             deliver_call_ms=(t1 - t0) * 1e3, wire_calls_ms=(t2 - t1) * 1e3))
    ctx.enable_timers(False)
    res = dict(name=name, lat_max_ms=lat_max_ms, n_bins=n_bins, bin_ns=MS, capacity=capacity, warmup_rounds=warm,
               held=stats([r["held"] for r in rows]), popped=stats([r["popped"] for r in rows]),
               push_ms=stats([r["push_ms"] for r in rows]), pop_ms=stats([r["pop_ms"] for r in rows]),
               wire_ms=stats([r["push_ms"] + r["pop_ms"] for r in rows]),
               delivery_kernels_ms=stats([r["delivery_kernels_ms"] for r in rows]),
               walk_ms=stats([r["walk_ms"] for r in rows]),
               wire_calls_host_ms=stats([r["wire_calls_ms"] for r in rows]),
               deliver_call_host_ms=stats([r["deliver_call_ms"] for r in rows]), rounds=rows)
    # bytes the wire's kernels move per event at the least: a record written on push; read, staged,
    # read again and written out as 36 B of arrays on pop
    res["push_ns_per_event"] = res["push_ms"]["mean"] * 1e6 / max(np.mean([r["delivered"] for r in rows]), 1)
    res["pop_ns_per_event"] = res["pop_ms"]["mean"] * 1e6 / max(res["popped"]["mean"], 1)
    del wire, ht, table, out, batches
    torch.cuda.empty_cache()
    return res


def leg_records(name, a, torch, ctx, lat_max_ms, n_bins, capacity):
    """The same rounds through both ways into the wire (see the module docstring)."""
    from shadow_amd import synth
    from shadow_amd.dist import HostPartition, ShardedDelivery
    from shadow_amd.wire import PacketWire, stamp_records
    from shadow_amd.worker import DeviceTable, Deliveries, HostTable, PacketBatch, deliver_round

    rng = np.random.default_rng(11)
    hosts = synth.make_hosts(a.hosts, a.nodes, exact_seeds=False)
    lat = rng.integers(MS, lat_max_ms * MS + 1, (a.nodes, a.nodes)).astype(np.uint64)
    loss = (rng.random((a.nodes, a.nodes)) * 0.02).astype(np.float32)
    table = DeviceTable(torch.from_numpy(lat.view(np.int64).ravel()).cuda(), torch.from_numpy(loss.ravel()).cuda(),
                        a.nodes)
    table.pack(ctx)
    ht_old = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    ht_new = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    sd = ShardedDelivery(ctx, ht_new, table, HostPartition(hosts["route"], a.nodes, 1), 0, 1)
    batches = []
    for s in range(4):
        pk = synth.make_packets(a.packets, hosts, 0, MS, seed=50 + s)
        batches.append((PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"]),
                        torch.from_numpy(pk["send_time"].view(np.int64)).cuda(),
                        torch.from_numpy((pk["payload"] + 28).astype(np.uint32).view(np.int32)).cuda()))
    out = Deliveries.allocate(a.packets, a.hosts)
    w_old = PacketWire(a.hosts, capacity, MS, n_bins, ctx=ctx)
    w_new = PacketWire(a.hosts, capacity, MS, n_bins, ctx=ctx)
    warm = lat_max_ms + 8
    cap = 2 * a.packets
    names = ("wire_push", "wire_stamp", "wire_pop")
    rows = []

    def read():
        return {n: ctx.read_timer(n)[0] for n in names}

    for k in range(warm + a.rounds):
        batch, rel, length = batches[k % len(batches)]
        batch.send_time_ns.copy_(rel + (T0 + k * MS))
        end = T0 + (k + 1) * MS
        if k == warm:
            ctx.enable_timers(True)
        timed = k >= warm
        # old: the single-GPU round and its push
        deliver_round(ht_old, table, batch, end, 2**63, 0, out=out, ctx=ctx)
        t0 = read() if timed else None
        w_old.push(batch, out, length, id_base=0)
        g_old = w_old.pop(end, cap=cap)
        t1 = read() if timed else None
        # new: the sharded round's source half, the stamp, the push from records
        src = sd.source_fn(ctx, ht_new, table, batch, end, 2**63, 0, sd.owner_dev, 1)
        n_rec = int(sum(src.send_counts))
        t2 = read() if timed else None
        stamp_records(src.send, n_rec, length, len(batch), id_base=0, ctx=ctx)
        w_new.push_records(src.send, n_rec)
        g_new = w_new.pop(end, cap=cap)
        t3 = read() if timed else None
        if g_old["n"] != g_new["n"] or w_old.count != w_new.count or int(out.n_delivered) != n_rec:
            sys.exit(f"{name}: the two paths disagree in round {k}")
        if timed:
            rows.append(dict(round=k, delivered=n_rec, popped=g_new["n"], held=w_new.count,
                             push_old_ms=t1["wire_push"] - t0["wire_push"], pop_old_ms=t1["wire_pop"] - t0["wire_pop"],
                             push_new_ms=t3["wire_push"] - t2["wire_push"], stamp_ms=t3["wire_stamp"] - t2["wire_stamp"],
                             pop_new_ms=t3["wire_pop"] - t2["wire_pop"]))
    ctx.enable_timers(False)
    # the last timed pops of both wires hold the same events in the same order
    same = all(bool(torch.equal(g_old[key], g_new[key])) for key in ("host", "time_ns", "packet", "len", "src_host",
                                                                      "event_id"))
    res = dict(name=name, lat_max_ms=lat_max_ms, n_bins=n_bins, bin_ns=MS, capacity=capacity, warmup_rounds=warm,
               ranks=1, last_pops_equal=same, held=stats([r["held"] for r in rows]),
               delivered=stats([r["delivered"] for r in rows]),
               push_old_ms=stats([r["push_old_ms"] for r in rows]), push_new_ms=stats([r["push_new_ms"] for r in rows]),
               stamp_ms=stats([r["stamp_ms"] for r in rows]), pop_old_ms=stats([r["pop_old_ms"] for r in rows]),
               pop_new_ms=stats([r["pop_new_ms"] for r in rows]), rounds=rows)
    res["ratio_push_new_over_old"] = res["push_new_ms"]["mean"] / res["push_old_ms"]["mean"]
    res["ratio_push_plus_stamp_over_old"] = (res["push_new_ms"]["mean"] + res["stamp_ms"]["mean"]) / \
        res["push_old_ms"]["mean"]
    res["regression_bound"] = 1.10  # the push's round-to-round spread is 4 %
    del w_old, w_new, ht_old, ht_new, table, out, batches, sd
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--hosts", type=int, default=100_000)
    p.add_argument("--nodes", type=int, default=1000)
    p.add_argument("--packets", type=int, default=1_000_000)
    p.add_argument("--rounds", type=int, default=24, help="timed steady-state rounds per leg (after the warm-up)")
    p.add_argument("--legs", default="P10M,P40M,P40M_far")
    p.add_argument("--out", default="")
    a = p.parse_args()

    import torch

    import shadow_amd

    if not torch.cuda.is_available():
        sys.exit("wire_bench.py measures on the GPU: no device found")
    shadow_amd.load()
    ctx = shadow_amd.default_context(0)
    per_ms = a.packets  # events entering per 1 ms round
    legs = {"P10M": (20, 128, per_ms * 14), "P40M": (80, 128, per_ms * 45),
            # the far list is written again beside itself when re-binned: room for a second copy
            "P40M_far": (80, 32, per_ms * 80)}
    res = {"config": dict(hosts=a.hosts, nodes=a.nodes, packets_per_round=a.packets, round_ns=MS,
                          timed_rounds=a.rounds, record_bytes=RECORD_BYTES,
                          device=torch.cuda.get_device_name(0)), "legs": {}}
    res["config"]["command"] = "python tools/wire_bench.py " + " ".join(sys.argv[1:])
    for name in a.legs.split(","):
        if name == "P10M_records":
            r = res["legs"][name] = leg_records(name, a, torch, ctx, *legs["P10M"])
            print(f"{name}: held {r['held']['mean'] / 1e6:.1f}M  push from deliveries {r['push_old_ms']['mean']:.3f} ms "
                  f"(sd {r['push_old_ms']['std']:.3f})  push from records {r['push_new_ms']['mean']:.3f} ms (sd "
                  f"{r['push_new_ms']['std']:.3f})  stamp {r['stamp_ms']['mean']:.3f} ms  ratio "
                  f"{r['ratio_push_new_over_old']:.3f} (with the stamp {r['ratio_push_plus_stamp_over_old']:.3f})  "
                  f"pops equal: {r['last_pops_equal']}", flush=True)
            continue
        res["legs"][name] = leg(name, a, torch, ctx, *legs[name])
        r = res["legs"][name]
        print(f"{name}: held {r['held']['mean'] / 1e6:.1f}M  push {r['push_ms']['mean']:.3f} ms (sd "
              f"{r['push_ms']['std']:.3f})  pop {r['pop_ms']['mean']:.3f} ms (sd {r['pop_ms']['std']:.3f}, max "
              f"{r['pop_ms']['max']:.3f})  delivery kernels {r['delivery_kernels_ms']['mean']:.3f} ms", flush=True)
    L = res["legs"]
    if "P10M" in L and "P40M" in L:
        res["ratio_40M_over_10M"] = dict(push=L["P40M"]["push_ms"]["mean"] / L["P10M"]["push_ms"]["mean"],
                                         pop=L["P40M"]["pop_ms"]["mean"] / L["P10M"]["pop_ms"]["mean"],
                                         wire=L["P40M"]["wire_ms"]["mean"] / L["P10M"]["wire_ms"]["mean"])
        print("P40M / P10M:", json.dumps(res["ratio_40M_over_10M"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    summary = {k: v for k, v in res.items() if k != "legs"}
    summary["legs"] = {n: {k: v for k, v in l.items() if k != "rounds"} for n, l in L.items()}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
