"""The device group on one card: the C3 host-table fill through sg_routing_info_fill and through
groups of 1, 2, 4 and 8 contexts on device 0, and the padded exchange of an 8-member round at C4
volume (k_group_pull beside the same rounds' delivery kernels).

    python tools/group_bench.py                  # everything, JSON to profiles/group_bench.json
    python tools/group_bench.py --single-only    # the single-context fill alone (works with an
                                                 # older library given via SHADOW_GPU_LIB: A/B of
                                                 # the fill's refactor)

On one card every member shares one PCIe link and one GPU: the group fill cannot be faster than
the single fill here, and the pull is a local copy.  What a group is for -- N links, xGMI -- needs
an N-GPU node and is not measured by this tool's device-0 runs (pass --devices to spread the
members over the devices of such a node).  Several contexts on one device also share the process's
hardware queues (GPU_MAX_HW_QUEUES, 4 by default): a member whose stream and copy stream land on one
queue loses the overlap of its copies with its builds (DESIGN 3.5 has the 4- and 16-queue series).
bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T0 = 946684800 * 10**9
PULL = "k_group_pull"
DELIVERY_KERNELS = ("walk", "pack", "scatter", "scatter2", "sort_small", "sort_big", "seg_bounds")


def series(ms):
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def timed_fills(fill, reps, sync):
    fill()  # warm-up: code objects, staging buffers, the pinned pages touched once
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fill()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--degree", type=float, default=8.0)
    p.add_argument("--hosts", type=int, default=100000)
    p.add_argument("--packets", type=int, default=1000000, help="packets each member sends per round")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--members", default="1,2,4,8")
    p.add_argument("--exchange-members", type=int, default=8)
    p.add_argument("--devices", default="0", help="devices the members are dealt over, e.g. 0,1,2,3")
    p.add_argument("--single-only", action="store_true")
    p.add_argument("--no-exchange", action="store_true")
    p.add_argument("--tag", default="")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_bench.json"))
    a = p.parse_args()

    import torch

    import shadow_amd
    from shadow_amd import Context, NetworkGraph, RoutingInfo, synth

    devices = [int(x) for x in a.devices.split(",")]
    g = synth.ring_chords_graph(a.nodes, a.degree, seed=1)
    used = np.arange(a.nodes, dtype=np.uint32)
    graph = lambda c: NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=c)
    res = {"tool": "group_bench", "tag": a.tag,
           "library": os.path.relpath(os.environ.get("SHADOW_GPU_LIB", shadow_amd.LIB_PATH), ROOT),
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "default"),
           "gpu": torch.cuda.get_device_name(0), "devices": devices,
           "workload": f"C3 table ({a.nodes} used nodes, {8 * a.nodes * a.nodes} bytes of cells) into the host "
                       "RoutingInfo; wall time of the call, one series entry per call"}

    # ---- the single-context fill ----
    ctx = Context(devices[0])
    net = graph(ctx)
    # one host object for every fill below: a second 0.8 GB pinned allocation may land on other
    # memory than the first, and the copy's speed follows the allocation, not the caller
    ri = RoutingInfo(used)
    res["single_fill"] = series(timed_fills(lambda: ri.fill(net, used, True), a.reps, ctx.synchronize))
    want_cells = ri.cells.copy()
    print(f"single fill: {res['single_fill']}", file=sys.stderr, flush=True)

    if not a.single_only:
        from shadow_amd import Group

        res["group_fill"] = {}
        for n in [int(x) for x in a.members.split(",")]:
            ctxs = [Context(devices[m % len(devices)]) for m in range(n)]
            graphs = [graph(c) for c in ctxs]
            group = Group(ctxs)
            ri.cells[:] = 0
            s = series(timed_fills(lambda: group.fill(ri, graphs, used), a.reps, lambda: [c.synchronize() for c in ctxs]))
            s["same_cells_as_single"] = bool(np.array_equal(ri.cells, want_cells))
            res["group_fill"][str(n)] = s
            print(f"group of {n}: {s}", file=sys.stderr, flush=True)
            for x in graphs:
                x.close()
            group.close()
            for c in ctxs:
                c.close()
        if not a.no_exchange:
            res["exchange"] = exchange(a, torch, devices, g, used)
    net.close()
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def exchange(a, torch, devices, g, used):
    """Padded rounds of a.exchange_members members, each sending a.packets from the hosts it owns:
    the pull's device time per launch beside the round's delivery kernels (HIP-event timers on each
    member's stream), and the round's wall time."""
    from shadow_amd import Context, Group, GroupDelivery, NetworkGraph, synth
    from shadow_amd.dist import HostPartition, row_range
    from shadow_amd.worker import DeviceTable, HostTable, PacketBatch

    n, nu = a.exchange_members, len(used)
    ctxs = [Context(devices[m % len(devices)]) for m in range(n)]
    group = Group(ctxs)
    hosts = synth.make_hosts(a.hosts, a.nodes, general_seed=1, exact_seeds=False)
    part = HostPartition(hosts["route"], nu, n)
    tables, hts, batches, nets = [], [], [], []
    for m, c in enumerate(ctxs):
        r0, r1, _ = row_range(nu, n, m)
        dev = torch.device("cuda", c.device)
        lat = torch.empty((r1 - r0) * nu, dtype=torch.int64, device=dev)
        loss = torch.empty((r1 - r0) * nu, dtype=torch.float32, device=dev)
        net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=c)
        net.build_rows_device(used, r0, r1, lat.data_ptr(), loss.data_ptr(), True)
        nets.append(net)
        tables.append(DeviceTable(lat, loss, nu, r0))
        hts.append(HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=c))
        pk = synth.make_packets(a.packets, hosts, T0 + 10**9, T0 + 10**9 + 10**6, seed=100 + m,
                                src_hosts=part.hosts_of[m])
        batches.append(PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"], device=dev))
    gd = GroupDelivery(group, hts, tables, part, padded=True)
    end, sim_end = T0 + 10**9 + 10**6, 2**63
    gd.round(batches, end, sim_end)  # exact: sizes the blocks
    gd.round(batches, end, sim_end)  # padded warm-up
    cap = gd.cap
    for c in ctxs:
        c.enable_timers(True)
    t0 = time.perf_counter()
    modes = []
    for _ in range(a.rounds):
        gd.round(batches, end, sim_end)
        modes.append(gd.last_mode)
    wall = (time.perf_counter() - t0) / a.rounds
    per = {}
    for name in (PULL,) + DELIVERY_KERNELS:
        ms, launches = 0.0, 0
        for c in ctxs:
            t, k, _ = c.read_timer(name)
            ms, launches = ms + t, launches + k
        if launches:
            per[name] = {"avg_launch_us": round(ms / launches * 1e3, 2), "launches_per_member_round":
                         round(launches / (n * a.rounds), 2)}
    for c in ctxs:
        c.enable_timers(False)
    counts = gd.last_counts
    out = {"members": n, "packets_per_member": a.packets, "hosts": a.hosts, "cap": int(cap), "modes": sorted(set(modes)),
           "records_per_owner": int(counts.sum(axis=0).mean()), "pair_max": int(counts.max()),
           "pull_bytes_per_owner": int(counts.sum(axis=0).mean()) * 32, "round_wall_ms": round(wall * 1e3, 3),
           "kernels": per,
           "what": "k_group_pull: one launch per owner per round, its HIP-event time beside the same rounds' "
                   "delivery kernels (source: walk, pack; bucketing: scatter, sort_*, seg_bounds); all members on "
                   "the listed devices"}
    print(f"exchange: {out}", file=sys.stderr, flush=True)
    for x in nets:
        x.close()
    del gd, hts, tables, batches
    group.close()
    for c in ctxs:
        c.close()
    return out


if __name__ == "__main__":
    main()
