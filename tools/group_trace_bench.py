"""A round's link trace and link loads across a device group at C3 (sg_group_link_trace_packets,
sg_group_link_load_packets) beside the single-context calls on the same round.

    python tools/group_trace_bench.py                 # JSON to profiles/group_trace_bench.json
    python tools/group_trace_bench.py --legs single   # the single-context calls alone (any ABI-7 library:
                                                      # SHADOW_GPU_LIB=<an older build> gives the A/B baseline)

The shape is tools/trace_bench.py's: the C3 graph (10k nodes), a host per node, 50,000 packets on
uniform random (source host, destination host) pairs, statuses from one delivery round.  A leg is one
child process on one GPU under a time limit of its own; the command stops at the first leg that
fails or runs out of time and starts nothing on the GPU after it.
  single   one context holding all rows: sg_link_trace_packets (all four outputs) and
           sg_link_load_packets (link and node loads, hops) on the whole batch;
  n1 .. n8 N contexts on device 0, member m holding rows row_range(10000, N, m) built on its own net
           and the packets of its own sources; the group's trace (all five outputs) and loads,
           alternated repetition by repetition with the single-context calls on the concatenated
           batch in the same process.
Per call the host clock runs around the call (each ends in a wait) and the library's timers give the
kernels: per member count, fill and sort (the slowest member and the sum over members), on root the
offsets, the merge and the reduce.  Every figure is a median with its min and max over --reps.
All members share one device here, so N > 1 shows the group's overhead, not scaling; timing across
devices and the peer-read path are not measured by this tool.  Correctness is
tests/test_group_trace_gpu.py's; every leg still compares the group's outputs with the single
context's.  bench.py stays the project's headline benchmark."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T0 = 946684800 * 10**9
LEGS = {"single": 150, "n1": 150, "n2": 150, "n4": 180, "n8": 210}  # name -> seconds
TRACE_TIMERS = ("link_trace_count", "link_trace_fill", "link_trace_sort")
ROOT_TIMERS = ("group_trace_offsets", "group_trace_merge")


def series(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def run_leg(a):
    import ctypes as C

    import torch

    from shadow_amd import Context, Group, NetworkGraph, _capi, synth
    from shadow_amd.dist import row_range
    from shadow_amd.worker import Deliveries, DeviceTable, HostTable, PacketBatch, deliver_round

    assert torch.cuda.is_available(), "this tool measures on a GPU"
    n, P = a.nodes, a.packets
    g = synth.ring_chords_graph(n, 8.0, seed=1)
    nodes = np.arange(n, dtype=np.uint32)
    hosts = synth.make_hosts(n, n, exact_seeds=False)
    rs = np.random.default_rng(4)
    src, dst = rs.integers(0, n, P), rs.integers(0, n, P)
    dst = np.where(dst == src, (dst + 1) % n, dst)
    order = np.argsort(src, kind="stable")  # grouped by source host: by source row, so by member
    src, dst = src[order].astype(np.uint32), dst[order]
    payload = np.where(rs.random(P) < 0.2, 0, 1448).astype(np.uint32)
    send = np.sort(rs.integers(T0, T0 + 10**6, P)).astype(np.uint64)

    def table(ctx, r0, r1):
        net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
        lat = torch.empty((r1 - r0, n), dtype=torch.int64, device="cuda")
        loss = torch.empty((r1 - r0, n), dtype=torch.float32, device="cuda")
        pred = torch.empty((r1 - r0, n), dtype=torch.int32, device="cuda")
        net.build_rows_device(nodes, r0, r1, lat.data_ptr(), loss.data_ptr())
        net.tree_rows_device(nodes, r0, r1, lat.data_ptr(), loss.data_ptr(), pred.data_ptr(), 0)
        return net, lat, loss, pred

    # the single context: all rows, the whole batch (sorted by source: the members' batches concatenated)
    ctx = Context(device=0)
    net, lat, loss, pred = table(ctx, 0, n)
    ht = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    pb = PacketBatch.from_numpy(src, hosts["ip"][dst], payload, send)
    out = Deliveries.allocate(P, n)
    deliver_round(ht, DeviceTable(lat.ravel(), loss.ravel(), n), pb, T0 + 10**6, 2**63, 0, out=out, ctx=ctx)
    torch.cuda.synchronize()
    status = out.status[:P].clone()
    n_links = len(net.links()[0])
    one = torch.zeros(2, dtype=torch.int64, device="cuda")
    loff = torch.zeros(n_links + 1, dtype=torch.int64, device="cuda")

    def s_trace(bufs, cap):
        return net.link_trace_packets_device(ht, nodes, 0, n, pred.data_ptr(), lat.data_ptr(), pb, status.data_ptr(), 0,
                                             loff.data_ptr(), *[b.data_ptr() for b in bufs], cap)[1]

    total = s_trace([one] * 4, 0)  # the sizing call
    sbufs = [torch.zeros(total, dtype=t, device="cuda") for t in (torch.int32, torch.int32, torch.int64, torch.int64)]
    sload = [torch.zeros(n_links, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"),
             torch.zeros(P, dtype=torch.int32, device="cuda")]

    def s_loads():
        net.link_load_packets_device(ht, nodes, 0, n, pred.data_ptr(), pb, status.data_ptr(), 0, *[b.data_ptr() for b in sload])

    def timed(c, call, timers):
        """(host ms, [ms per timer]) of one call."""
        torch.cuda.synchronize()
        c.enable_timers(True)
        try:
            t0 = time.perf_counter()
            call()
            wall = (time.perf_counter() - t0) * 1e3
            got = [c.read_timer(k) for k in timers]
        finally:
            c.enable_timers(False)
        assert all(launches == 1 for _, launches, _ in got), got
        return wall, [ms for ms, _, _ in got]

    res = {"leg": a.leg, "nodes": n, "links": n_links, "packets": P, "delivered": int((status == 0).sum()),
           "records": int(total), "abi": _capi.abi_version(), "library": os.environ.get("SHADOW_GPU_LIB", "in-tree")}
    t = {"single_trace": {k: [] for k in ("host",) + TRACE_TIMERS}, "single_loads": {"host": [], "link_packets": []}}
    world = 0 if a.leg == "single" else int(a.leg[1:])
    if world:
        ctxs = [Context(device=0) for _ in range(world)]
        group = Group(ctxs)
        mem = []
        for m, c in enumerate(ctxs):
            r0, r1, _ = row_range(n, world, m)
            mnet, mlat, mloss, mpred = table(c, r0, r1)
            idx = np.flatnonzero((hosts["route"][src] >= r0) & (hosts["route"][src] < r1))
            mem.append(dict(r0=r0, r1=r1, net=mnet, lat=mlat, pred=mpred, idx=idx,
                            ht=HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=c),
                            pb=PacketBatch.from_numpy(src[idx], hosts["ip"][dst[idx]], payload[idx], send[idx]),
                            status=status[torch.from_numpy(idx).cuda()].contiguous(),
                            hops=torch.zeros(max(len(idx), 1), dtype=torch.int32, device="cuda")))
        assert np.array_equal(np.concatenate([x["idx"] for x in mem]), np.arange(P))  # member order = batch order
        ptr = lambda ts: (C.c_void_p * world)(*[x.data_ptr() for x in ts])  # noqa: E731
        common = [group.handle, (C.c_void_p * world)(*[x["net"]._ensure_net().value for x in mem]),
                  (C.c_void_p * world)(*[getattr(x["ht"].handle, "value", x["ht"].handle) for x in mem]),
                  nodes.ctypes.data, n, (C.c_uint32 * world)(*[x["r0"] for x in mem]),
                  (C.c_uint32 * world)(*[x["r1"] for x in mem]), ptr([x["pred"] for x in mem])]
        packets = (_capi.sg_packets * world)(*[x["pb"].c_struct() for x in mem])
        goff = torch.zeros(n_links + 1, dtype=torch.int64, device="cuda")
        gbufs = [torch.zeros(total, dtype=d, device="cuda")
                 for d in (torch.int32, torch.uint8, torch.int32, torch.int64, torch.int64)]
        gload = [torch.zeros(n_links, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")]
        gtotal = C.c_uint64()
        L = _capi.load()

        def g_trace():
            group._check(L.sg_group_link_trace_packets(
                *common, ptr([x["lat"] for x in mem]), packets, ptr([x["status"] for x in mem]), None, None, 0,
                goff.data_ptr(), *[b.data_ptr() for b in gbufs], total, C.byref(gtotal)))

        def g_loads():
            group._check(L.sg_group_link_load_packets(
                *common, packets, ptr([x["status"] for x in mem]), None, 0, gload[0].data_ptr(), gload[1].data_ptr(),
                ptr([x["hops"] for x in mem])))

        def timed_group(call, member_timers, root_timers):
            torch.cuda.synchronize()
            for c in ctxs:
                c.enable_timers(True)
            try:
                t0 = time.perf_counter()
                call()
                wall = (time.perf_counter() - t0) * 1e3
                per = [[c.read_timer(k)[0] for k in member_timers] for c in ctxs]
                root = [ctxs[0].read_timer(k)[0] for k in root_timers]
            finally:
                for c in ctxs:
                    c.enable_timers(False)
            return wall, per, root

        t["group_trace"] = {k: [] for k in ("host",) + ROOT_TIMERS + tuple(f"{k}_slowest_member" for k in TRACE_TIMERS) +
                            tuple(f"{k}_sum_members" for k in TRACE_TIMERS)}
        t["group_loads"] = {k: [] for k in ("host", "group_link_reduce", "link_packets_slowest_member",
                                            "link_packets_sum_members")}

    def rep(record):
        wall, ms = timed(ctx, lambda: s_trace(sbufs, total), TRACE_TIMERS)
        if record:
            t["single_trace"]["host"].append(wall)
            for k, x in zip(TRACE_TIMERS, ms):
                t["single_trace"][k].append(x)
        for b in sload:
            b.zero_()
        wall, ms = timed(ctx, s_loads, ("link_packets",))
        if record:
            t["single_loads"]["host"].append(wall)
            t["single_loads"]["link_packets"].append(ms[0])
        if not world:
            return
        wall, per, root = timed_group(g_trace, TRACE_TIMERS, ROOT_TIMERS)
        if record:
            t["group_trace"]["host"].append(wall)
            for k, x in zip(ROOT_TIMERS, root):
                t["group_trace"][k].append(x)
            for i, k in enumerate(TRACE_TIMERS):
                t["group_trace"][f"{k}_slowest_member"].append(max(p[i] for p in per))
                t["group_trace"][f"{k}_sum_members"].append(sum(p[i] for p in per))
        for b in gload:
            b.zero_()
        wall, per, root = timed_group(g_loads, ("link_packets",), ("group_link_reduce",))
        if record:
            t["group_loads"]["host"].append(wall)
            t["group_loads"]["group_link_reduce"].append(root[0])
            t["group_loads"]["link_packets_slowest_member"].append(max(p[0] for p in per))
            t["group_loads"]["link_packets_sum_members"].append(sum(p[0] for p in per))

    for _ in range(2):  # warm-up: code objects, workspaces, every shape the timed repetitions use
        rep(False)
    for _ in range(a.reps):
        rep(True)
    torch.cuda.synchronize()
    if world:  # the group computed what the single context did
        assert gtotal.value == total and torch.equal(goff, loff)
        for gb, sb in zip([gbufs[0], gbufs[2], gbufs[3], gbufs[4]], sbufs):
            assert torch.equal(gb, sb)
        assert torch.equal(gload[0], sload[0]) and torch.equal(gload[1], sload[1])
        assert torch.equal(torch.cat([x["hops"][:len(x["idx"])] for x in mem]), sload[2])
        group.close()
    for which, d in t.items():
        res[which] = {k: series(v) for k, v in d.items()}
    print(json.dumps(res), flush=True)
    with open(a.leg_out, "w") as f:
        json.dump(res, f)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--nodes", type=int, default=10000)
    p.add_argument("--packets", type=int, default=50000)
    p.add_argument("--legs", default="n1,n2,n4,n8")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_trace_bench.json"))
    p.add_argument("--leg", help=argparse.SUPPRESS)  # (a child: run this leg, write --leg-out)
    p.add_argument("--leg-out", help=argparse.SUPPRESS)
    a = p.parse_args()
    assert a.reps >= 5, "at least five repetitions"
    if a.leg:
        return run_leg(a)
    cases, stopped = [], None
    for leg in [x for x in a.legs.split(",") if x]:
        tmp = a.out + f".{leg}.tmp"
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--leg-out", tmp, "--reps", str(a.reps), "--nodes",
               str(a.nodes), "--packets", str(a.packets)]
        try:
            rc = subprocess.run(cmd, timeout=LEGS[leg]).returncode
        except subprocess.TimeoutExpired:
            rc = "time limit"
        if rc != 0:
            stopped = f"leg {leg}: {rc}"
            print(stopped + "; nothing more is started", file=sys.stderr)
            break
        with open(tmp) as f:
            cases.append(json.load(f))
        os.remove(tmp)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/group_trace_bench.py", "reps": a.reps, "stopped": stopped, "cases": cases}, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
