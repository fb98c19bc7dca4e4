"""Pair batches and sentinels of the batched tree-path tests (test_paths_ref_cpu.py qualifies
them on the CPU, test_paths_gpu.py runs them).  Graphs, hosts and packet batches are those of
tests/tree_cases.py, tests/link_cases.py and tests/link_round_cases.py."""
import numpy as np

PAIR_COUNTS = (1, 63, 64, 65, 257)  # (b): under, at and over one wave, and past one workgroup
SENT_OFF = np.uint64(0xA5A5A5A5A5A5A5A5)
SENT32 = np.uint32(0x5A5A5A5A)
SENT_LAT = np.uint64(0x5A5A5A5A00000000)
SENT_LOSS = np.float32(-7.5)


def tie_pairs(n_pairs, seed=61):
    """(b): uniform (row, column) pairs on the tie graph's 300 nodes; the first one a same-node
    pair (one record: the self-loop)."""
    rng = np.random.default_rng(seed)
    ri, cj = rng.integers(0, 300, n_pairs), rng.integers(0, 300, n_pairs)
    cj[0] = ri[0]
    return ri.astype(np.uint32), cj.astype(np.uint32)


def wave_spans(off):
    """Records per wave: the spans of 64 consecutive pairs."""
    off = np.asarray(off, np.int64)
    edges = off[np.minimum(np.arange(0, len(off) - 1 + 64, 64), len(off) - 1)]
    return np.diff(edges)


def stage_capacities(off):
    """(b): SG_PATHS_STAGE_HOPS values that put the first wave's span one record under the
    capacity, at it, and one over."""
    s = int(wave_spans(off)[0])
    return [h for h in (s + 1, s, s - 1) if h >= 1]
