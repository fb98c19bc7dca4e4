"""Late seeds of the LDS search (sg_sssp.hip "Late seeds"): a plain-Python model of one chained,
bounded row whose bound rows are merged into key[] while the search already runs.

The model keeps the kernel's key (latency << 32 | bits(loss) << 1 | dirty) and its rules:
  * a FIFO queue; a relaxation is one atomic min with a dirty candidate, and the node is appended
    iff the key it replaced was clean and larger; a pop clears the flag with one atomic AND and
    relaxes with the key that AND returned;
  * the row starts from the chain's rewrite of the row of one out-neighbour t (exact through a
    zero-loss arc, latency + 1 and loss 1.0 otherwise, clean), the source at (0, 0.0, dirty), queued;
  * one or two further out-neighbours' rows give seeds as the kernel forms them: the bound
    (w + D[s'][v].lat + 1, 1.0) for every node, and through a zero-loss arc the exact key
    (w + D[s'][v].lat, D[s'][v].loss) for every node but s' itself (whose cell of the table is the
    raw self-loop);
  * the seeds are merged one node at a time at random points of the search, by the rule
    new = min(old & ~1, seed) | (old & 1), attempted only when the seed is below the key read;
  * up to three pops are in flight at once, and every arc of a pop is an event of its own, so
    merges land between a pop's AND and its relaxations, and between two relaxations;
  * the search ends when the queue is empty and no pop is in flight; the merges not yet applied
    land then (every wave finishes its merge before the closing barrier) and queue nothing.

Asserted: the final keys equal Dijkstra's over (latency, f32 loss) for every interleaving; no node
is ever appended while it is queued; and the same model with a plain clean min in place of the
dirty-preserving rule does queue a node twice for some interleaving, so the model can see the bug
the rule is there to prevent.
"""
import heapq
import random

import numpy as np

ONE = np.float32(1.0)
ONE_BITS = 0x3F800000
LATS = (1000, 2000, 3000)  # three values: equal-latency paths everywhere
SELF_LAT = 1000            # the diagonal cell of a bound row: the raw self-loop


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _fold(loss_bits, one_minus_e):
    """sg_device.h fold_loss: 1f32 - (1f32 - a) * (1f32 - e), every op rounded once."""
    a = np.uint32(loss_bits).view(np.float32)
    return _bits(ONE - (ONE - a) * one_minus_e)


def _key(lat, loss_bits, dirty=0):
    return (lat << 32) | (loss_bits << 1) | dirty


def _graph(n, rng, directed):
    """Ring plus n chords, 60 % zero-loss arcs; undirected: every edge mirrored with its weights."""
    edges = [(i, (i + 1) % n) for i in range(n)]
    while len(edges) < 2 * n:
        a, b = rng.randrange(n), rng.randrange(n)
        if a != b:
            edges.append((a, b))
    out = [[] for _ in range(n)]
    for a, b in edges:
        lat = rng.choice(LATS)
        loss = np.float32(0.0) if rng.random() < 0.6 else np.float32(rng.uniform(0.01, 0.3))
        arc = (lat, ONE - loss, bool(loss == 0))
        out[a].append((b,) + arc)
        if not directed:
            out[b].append((a,) + arc)
    return out


def _dijkstra(out, s):
    """(latency, bits(loss)) of every node from s, the loss folded from the left along the path."""
    n = len(out)
    best = [None] * n
    heap = [(0, 0, s)]
    while heap:
        lat, lb, u = heapq.heappop(heap)
        if best[u] is not None:
            continue
        best[u] = (lat, lb)
        for v, w, om, _ in out[u]:
            if best[v] is None:
                heapq.heappush(heap, (lat + w, _fold(lb, om), v))
    assert all(b is not None for b in best)
    return best


def _row_case(out, rows, s, rng):
    """The start keys of s's row chained behind its out-neighbour t, and the late seeds (node, key)
    from one or two other out-neighbours' rows."""
    n = len(out)
    arcs = out[s][:]
    rng.shuffle(arcs)
    t, w, _, zero = arcs[0]
    start = []
    for v in range(n):
        lat, lb = rows[t][v]
        start.append(_key(lat + w, lb) if zero else _key(lat + w + 1, ONE_BITS))
    seeds = []
    seen = {t}
    n_rows = rng.choice((1, 2))
    for sp, w, _, zero in arcs[1:]:
        if sp in seen or sp == s or len(seen) > n_rows:
            continue
        seen.add(sp)
        for v in range(n):
            lat, lb = rows[sp][v] if v != sp else (SELF_LAT, 0)
            sd = _key(lat + w + 1, ONE_BITS)
            if zero and v != sp:
                sd = min(sd, _key(lat + w, lb))
            seeds.append((v, sd))
    return start, seeds


def _run(out, s, start, seeds, rng, keep_dirty=True, workers=3):
    """One interleaving.  Returns (final keys, True if a node was appended while queued)."""
    key = start[:]
    key[s] = 1  # (0, 0.0), dirty
    queue = [s]
    queued = {s}
    twice = False
    merges = seeds[:]
    rng.shuffle(merges)
    busy = []  # pops in flight: [key popped with, arcs not yet relaxed]
    # how eager the merges are: from all ahead of the first pop to all behind the last
    p_merge = rng.choice((0.02, 0.2, 0.5, 0.9))
    while queue or busy or merges:
        search_on = bool(queue or busy)
        if merges and (not search_on or rng.random() < p_merge):
            v, sd = merges.pop()
            old = key[v]
            if keep_dirty:
                if sd < (old & ~1):
                    key[v] = sd | (old & 1)
            elif sd < old:
                key[v] = sd  # the bug: a clean seed over a dirty, queued key
            continue
        if queue and len(busy) < workers and (not busy or rng.random() < 0.5):
            u = queue.pop(0)
            queued.discard(u)
            ku = key[u] & ~1  # the AND's return value
            key[u] = ku
            busy.append([ku, out[u][:]])
            continue
        b = rng.choice(busy)
        if b[1]:
            v, w, om, _ = b[1].pop()
            cand = _key((b[0] >> 32) + w, _fold((b[0] >> 1) & 0x7FFFFFFF, om), 1)
            old = key[v]
            if cand < old:
                key[v] = cand
            if not (old & 1) and old > cand:  # improved, and was clean: append
                twice |= v in queued
                queue.append(v)
                queued.add(v)
        if not b[1]:
            busy.remove(b)
    return key, twice


def _cases():
    """(out, rows, s, start, seeds, rng) over graphs of 12 to 40 nodes, each directed and undirected."""
    for gi in range(28):
        n = 12 + gi
        for directed in (False, True):
            rng = random.Random(1000 * gi + directed)
            out = _graph(n, rng, directed)
            rows = [_dijkstra(out, v) for v in range(n)]
            sources = [v for v in range(n) if len({a[0] for a in out[v]} - {v}) >= 2]
            for s in rng.sample(sources, 2):
                start, seeds = _row_case(out, rows, s, rng)
                if seeds:
                    yield out, rows, s, start, seeds, rng


def test_late_seeds_keep_the_row_exact_and_queue_once():
    runs = 0
    for out, rows, s, start, seeds, rng in _cases():
        want = [_key(lat, lb) for lat, lb in rows[s]]
        for _ in range(12):
            key, twice = _run(out, s, start, seeds, rng)
            runs += 1
            assert not twice, f"a node of {len(out)} was queued twice (source {s})"
            assert all(not (k & 1) for k in key), "a node is dirty after the search ended"
            assert key == want, f"keys differ from Dijkstra's ({len(out)} nodes, source {s})"
    assert runs >= 1000


def test_every_start_and_seed_is_a_real_path_value():
    """What the argument rests on: no start key and no seed is below the node's optimum."""
    for out, rows, s, start, seeds, _ in _cases():
        for v, k in list(enumerate(start)) + seeds:
            if v != s:
                assert k >= _key(*rows[s][v])


def test_plain_min_merge_is_caught():
    caught = 0
    for out, rows, s, start, seeds, rng in _cases():
        for _ in range(12):
            caught += _run(out, s, start, seeds, rng, keep_dirty=False)[1]
    assert caught >= 1
