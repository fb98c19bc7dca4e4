"""CPU model of the LDS search's phase plan (sg_plan.hip), in plain numpy.

The header of sg_plan.hip is the specification; this restates it.  Phase sets by vote: for each
set, every row of the block not yet in a phase names the best candidate of its closed out-
neighbourhood (itself and the unassigned block rows it has an arc to), the one with the highest
gain (1 + its in-arcs from unassigned block rows, arcs counted), then the lowest row; every named
row joins the set.  The rows left after n_phase - 1 sets take the last phase.  Landmarks split
phase 0 (k_plan_landmarks).

Arcs are the device's (sg_net.hip): a self-loop is no arc, an undirected edge is one arc each
way, parallel edges stay parallel.
"""
import numpy as np

PHASES_MAX = 6  # SSSP_PHASES_MAX


def arcs(g):
    """(tail, head) of every arc of the uploaded graph."""
    s, d = np.asarray(g["src"], dtype=np.int64), np.asarray(g["dst"], dtype=np.int64)
    keep = s != d
    s, d = s[keep], d[keep]
    if not g["directed"]:
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
    return s, d


def n_launches(n_phase, n_land=0):
    """The plan's phases (one launch each) for SG_SSSP_PHASES = n_phase and n_land landmarks."""
    return max(2, min(PHASES_MAX - (1 if n_land else 0), n_phase)) + (1 if n_land else 0)


def phases(g, used, rows, n_phase, n_land=0):
    """The phase of every row of the block rows = (row_begin, row_end) of the used list."""
    used = np.asarray(used, dtype=np.int64)
    r0, r1 = rows
    nr = r1 - r0
    n_sets = n_launches(n_phase, 0) - 1 if not n_land else n_launches(n_phase, n_land) - 2
    rel = np.full(g["n"], -1, dtype=np.int64)
    rel[used[r0:r1]] = np.arange(nr)
    s, d = arcs(g)
    inside = (rel[s] >= 0) & (rel[d] >= 0)
    t, h = rel[s[inside]], rel[d[inside]]  # arcs between block rows, as relative rows
    jn = np.zeros(nr, dtype=np.int64)  # 0: in no phase yet, else phase + 1
    for ph in range(n_sets):
        is_open = jn == 0
        live = is_open[t] & is_open[h]
        lt, lh = t[live], h[live]
        gain = 1 + np.bincount(lh, minlength=nr)
        # every open row's best candidate by (gain, then lowest row): itself, then the heads of its arcs
        score = gain * (nr + 1) + (nr - np.arange(nr))
        best = np.where(is_open, score, 0)
        np.maximum.at(best, lt, score[lh])
        named = nr - best[is_open] % (nr + 1)
        jn[named] = ph + 1
    if n_land:
        p0 = np.flatnonzero(jn == 1)
        s0 = len(p0)
        land = np.zeros(nr, dtype=bool)
        if n_land < s0:
            i = np.arange(s0, dtype=np.int64)
            step = (i * n_land) // s0 != ((i - 1) * n_land) // s0
            step[0] = True
            land[p0[step]] = True
        jn = np.where(land, 1, np.where(jn > 0, jn + 1, 0))
    last = n_launches(n_phase, n_land) - 1
    return np.where(jn > 0, jn - 1, last)


def sizes(ph, n):
    """Rows per phase, for n phases."""
    return [int(c) for c in np.bincount(ph, minlength=n)[:n]]
