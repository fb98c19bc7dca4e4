#!/usr/bin/env python3
"""A CPU model of the LDS search's work queue (sg_sssp.hip): an event simulation of one row.

Rules.  16 waves, a FIFO queue, the kernel's claim rule.  A free wave claims entries as soon as the
queue holds any; a pop's keys are read (and its nodes' dirty flags cleared) at claim time, its
candidates are applied when its step ends, and the nodes it improved that were clean are appended
then.  A pop costs a fixed part (claim + pop) and a step: the lane step walks eight slots per lane
plus an overflow round per 64 arcs past a node's eighth; the arc-parallel step costs a + b per slot
of 64 arcs.  Every row's final keys are checked against a plain fixed point (Dijkstra on the
(latency, loss) order with the f32 loss fold of sg_device.h).

A bounded row starts from the rows of its source's two lowest-latency neighbours: latency + arc + 1
with loss 1.0 as a bound, the exact key through a zero-loss arc; the start keys are clean.  There is
no chain and there are no three-arc seeds.

The cost constants default to the r07 counters and can be re-fitted from an SG_SSSP_DIAG file
(tools/sssp_diag.py's output): --diag FILE takes the fixed part from the "per pop" line and, where
the file holds the per-class table of a build that took the arc-parallel step, a and b from its
classes S = 1 and S = 2.

python tools/sssp_queue_model.py [--nodes 10000] [--degree 8] [--rows 16] [--diag FILE]
"""
import argparse
import heapq
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NW = 16
LA = 8
ONE = np.float32(1.0)
INF = np.uint64(0xFFFFFFFF) << np.uint64(31) | np.uint64(0x3F800000)  # (2^32 - 1, 1.0)
CLASSES = ("0", "1", "2", "3-4", "5-8", ">8")


class Costs:
    """Cycles: fixed per pop; the lane step l0 + LA * l1, its overflow round o0 + o1 per 64 arcs."""

    def __init__(self, fixed=1750.0, l0=500.0, l1=545.0, o0=400.0, o1=545.0):
        self.fixed, self.l0, self.l1, self.o0, self.o1 = fixed, l0, l1, o0, o1
        self.fit = None  # (a, b) measured for the arc-parallel step

    def lane(self, deg):
        over = int(np.maximum(deg.astype(np.int64) - LA, 0).sum())
        return self.l0 + LA * self.l1 + (-(-over // 64)) * (self.o0 + self.o1)

    @staticmethod
    def from_diag(path):
        c = Costs()
        text = open(path).read()
        m = re.search(r"claim\+wait (\d+), pop (\d+), steps (\d+) \(per pop: (\d+), (\d+)\)", text)
        pops = re.search(r"([\d.]+) wave pops", text)
        if m and pops:
            c.fixed = float(m.group(1)) / float(pops.group(1)) + float(m.group(4))
        per = {}
        for line in text.splitlines():
            f = line.split()
            if len(f) == 8 and f[0] in CLASSES and f[2].endswith("%"):
                per[f[0]] = float(f[7])
        if per.get("5-8"):  # pops of 5 to 8 slots per lane take the lane step in either build
            c.l1 = (per["5-8"] - c.l0) / LA
        if per.get("1") and per.get("2") and per["2"] > per["1"] and per["2"] < 0.6 * per.get("5-8", 1e9):
            c.fit = (2 * per["1"] - per["2"], per["2"] - per["1"])
        return c


class Policy:
    def __init__(self, name, share=0, claim=64, arc=None, step_arcs=None, lane=True):
        # arc: (a, b) of the arc-parallel step, None: the lane step only
        # step_arcs: None takes the cheaper step; a number the kernel's rule, arcs <= step_arcs, in
        #   one slot, two, or rounds of four
        self.name, self.share, self.claim, self.arc, self.step_arcs, self.lane = name, share, claim, arc, step_arcs, lane

    def take(self, avail):
        if not self.share:
            return min(self.claim, avail)
        return min(self.claim, avail, max(self.share, -(-avail // NW)))

    def step(self, costs, deg):
        t = int(deg.sum())
        lane = costs.lane(deg)
        if self.arc is None:
            return lane
        a, b = self.arc
        if self.step_arcs is None:
            return min(lane, a + b * (-(-t // 64)))
        if t > self.step_arcs:
            return lane
        return a + b * (-(-t // 64)) if t <= 128 else (-(-t // 256)) * (a + 4 * b)


def load_graph(g):
    """Out-arcs by tail node: off, head, latency, bits-exact f32 (1 - loss); an undirected edge both ways."""
    src, dst = g["src"].astype(np.int64), g["dst"].astype(np.int64)
    lat, om = g["lat"].astype(np.uint64), ONE - g["loss"].astype(np.float32)
    if not g["directed"]:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        lat, om = np.concatenate([lat, lat]), np.concatenate([om, om])
    keep = src != dst  # a self-loop relaxes nothing
    src, dst, lat, om = src[keep], dst[keep], lat[keep], om[keep]
    order = np.argsort(src, kind="stable")
    off = np.zeros(g["n"] + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=g["n"]), out=off[1:])
    return off, dst[order], lat[order], om[order]


def pack(lat, loss):
    return (lat.astype(np.uint64) << np.uint64(31)) | loss.astype(np.float32).view(np.uint32).astype(np.uint64)


def relax(keys, lat, om):
    """key (+) arc for arrays: latency add, loss' = 1 - (1 - loss) * (1 - e) in f32, three rounded ops."""
    kl = keys >> np.uint64(31)
    loss = (keys & np.uint64(0x7FFFFFFF)).astype(np.uint32).view(np.float32)
    nl = ONE - (ONE - loss) * om
    return pack(kl + lat, nl)


def fixed_point(graph, n, src):
    """Dijkstra on the packed (latency, loss) order: the unique fixed point of the relaxation."""
    off, head, lat, om = graph
    key = np.full(n, INF, np.uint64)
    key[src] = 0
    done = np.zeros(n, bool)
    heap = [(0, src)]
    while heap:
        k, u = heapq.heappop(heap)
        if done[u] or k != int(key[u]):
            continue
        done[u] = True
        a0, a1 = off[u], off[u + 1]
        cand = relax(np.full(a1 - a0, k, np.uint64), lat[a0:a1], om[a0:a1])
        for v, c in zip(head[a0:a1].tolist(), cand.tolist()):
            if c < int(key[v]):
                key[v] = c
                heapq.heappush(heap, (c, v))
    return key


def bounded_start(graph, n, src, rows):
    """The start keys of a bounded row: rows[s'] for the source's two lowest-latency neighbours."""
    off, head, lat, om = graph
    a0, a1 = off[src], off[src + 1]
    key = np.full(n, INF, np.uint64)
    seen = []
    for i in np.argsort(lat[a0:a1], kind="stable"):
        s2 = int(head[a0 + i])
        if s2 in seen:
            continue
        seen.append(s2)
        w = lat[a0 + i]
        d = rows(s2)
        bound = pack((d >> np.uint64(31)) + w + np.uint64(1), np.full(n, ONE))
        key = np.minimum(key, np.where(d == INF, INF, bound))
        if om[a0 + i] == ONE:  # a zero-loss arc: the exact key of the path src -> s' -> v
            exact = d + (w << np.uint64(31))
            exact[s2] = INF  # (the arc itself is relaxed from the source)
            key = np.minimum(key, np.where(d == INF, INF, exact))
        if len(seen) == 2:
            break
    key[src] = INF
    return key


def simulate(graph, n, src, policy, costs, start=None):
    """One row.  Returns (keys, stats): search cycles, pops, relaxations, busy cycles per wave, pops by class."""
    off, head, lat, om = graph
    key = np.full(n, INF, np.uint64) if start is None else start.copy()
    dirty = np.zeros(n, bool)
    key[src] = 0
    dirty[src] = True
    queue, qh = [src], 0
    events = []  # (end time, sequence, heads, candidates)
    idle = list(range(NW))
    now, seq, busy, pops, rel = 0.0, 0, 0.0, 0, 0
    cls = np.zeros(len(CLASSES), np.int64)
    while True:
        while idle and qh < len(queue):
            k = policy.take(len(queue) - qh)
            u = np.array(queue[qh:qh + k], np.int64)
            qh += k
            dirty[u] = False
            deg = off[u + 1] - off[u]
            arcs = np.concatenate([np.arange(off[x], off[x + 1]) for x in u]) if len(u) else np.zeros(0, np.int64)
            cand = relax(np.repeat(key[u], deg), lat[arcs], om[arcs])
            t = int(deg.sum())
            s = -(-t // 64)
            cls[s if s <= 2 else 3 if s <= 4 else 4 if s <= 8 else 5] += 1
            cost = costs.fixed + policy.step(costs, deg)
            idle.pop()
            heapq.heappush(events, (now + cost, seq, head[arcs], cand))
            seq += 1
            busy += cost
            pops += 1
            rel += t
        if not events:
            break
        now, _, v, cand = heapq.heappop(events)
        idle.append(0)
        old = key[v]  # (a node twice among the candidates: np.minimum.at keeps the smallest)
        np.minimum.at(key, v, cand)
        better = np.unique(v[cand < old])
        fresh = better[~dirty[better]]
        dirty[fresh] = True
        queue.extend(fresh.tolist())
    return key, dict(cycles=now, pops=pops, rel=rel, busy=busy / NW, cls=cls)


def policies(costs):
    fit = costs.fit or (1000.0, 600.0)
    return [
        Policy("parent"),
        Policy("parent's claims, step 600 + 650 S", arc=(600.0, 650.0)),
        Policy("parent's claims, step 1,000 + 1,000 S", arc=(1000.0, 1000.0)),
        Policy("share claims (min 16), step 600 + 650 S", share=16, arc=(600.0, 650.0)),
        Policy("share claims (min 32), step 1,000 + 1,000 S", share=32, arc=(1000.0, 1000.0)),
        Policy("share claims (min 8), lane step only", share=8),
        Policy(f"the kernel's rule: arcs <= 256, step {fit[0]:.0f} + {fit[1]:.0f} S", arc=fit, step_arcs=256),
    ]


def run(g, rows, costs, check=None, out=sys.stdout):
    """Every policy on the listed source rows, bounded and from infinity; each row's keys checked
    against the fixed point (and by check(src, keys), if given).  Returns {policy: (bounded, infinity)}."""
    n = g["n"]
    graph = load_graph(g)
    cache = {}

    def fp(s):
        if s not in cache:
            cache[s] = fixed_point(graph, n, s)
        return cache[s]

    res = {}
    for p in policies(costs):
        tot = [dict(cycles=0.0, pops=0, rel=0, busy=0.0, cls=np.zeros(len(CLASSES), np.int64)) for _ in range(2)]
        for s in rows:
            for b, start in ((0, bounded_start(graph, n, s, fp)), (1, None)):
                key, st = simulate(graph, n, s, p, costs, start)
                assert np.array_equal(key, fp(s)), f"{p.name}: row {s} is not the fixed point"
                if check:
                    check(s, key)
                for k in tot[b]:
                    tot[b][k] = tot[b][k] + st[k]
        res[p.name] = tot
    m = len(rows)
    arcs = len(graph[1])
    base = res["parent"]
    print(f"{m} rows, {n} nodes, {arcs} arcs; cycles of the search per row (fixed {costs.fixed:.0f} per pop, lane step "
          f"{costs.l0:.0f} + {LA} x {costs.l1:.0f})", file=out)
    print(f"{'policy':<58} {'bounded row':>20} {'row from infinity':>20}", file=out)
    for name, tot in res.items():
        cells = []
        for b in (0, 1):
            c, c0 = tot[b]["cycles"] / m, base[b]["cycles"] / m
            cells.append(f"{c / 1e3:.1f}k ({(c - c0) / c0:+.0%})")
        print(f"{name:<58} {cells[0]:>20} {cells[1]:>20}", file=out)
    for name in ("parent", list(res)[-1]):
        for b, what in ((0, "bounded row"), (1, "row from infinity")):
            t = res[name][b]
            share = t["cls"] / max(1, t["cls"].sum())
            print(f"{name}, {what}: {t['pops'] / m:.1f} wave pops, {t['rel'] / m / arcs:.2f} relaxations per arc, "
                  f"{t['busy'] / m / 1e3:.1f}k busy cycles per wave; pops by S "
                  + ", ".join(f"{c}: {x:.0%}" for c, x in zip(CLASSES, share)), file=out)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--degree", type=float, default=8.0)
    ap.add_argument("--rows", type=int, default=16, help="random source rows")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--diag", default=None, help="an SG_SSSP_DIAG file to take the cost constants from")
    a = ap.parse_args()
    from shadow_amd import synth

    g = synth.ring_chords_graph(a.nodes, a.degree, seed=1)
    rows = np.random.default_rng(a.seed).choice(a.nodes, a.rows, replace=False).tolist()
    run(g, rows, Costs.from_diag(a.diag) if a.diag else Costs())


if __name__ == "__main__":
    main()
