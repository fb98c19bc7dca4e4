"""The wire_cases scenario seen from W ranks: what each owner rank's wire must return, and the
block size of the padded test.  Computed from the oracle's run alone (wire_cases.scenario), so
tests/test_wire_sharded_cpu.py can assert, without a GPU, that the sharded GPU tests cannot pass
vacuously, and tests/test_wire_sharded_gpu.py compares the device chain against it."""
import numpy as np

import wire_cases as wc
from shadow_amd.dist import HostPartition
from wire_ref import NEVER

POP_KEYS = ("host", "time_ns", "packet", "len", "src_host", "event_id")
PADDED_W = 3  # ranks of the padded test
_cache = {}


def partition(sc, W):
    """Hosts in W equal blocks of routing rows (host h sits on node h: rank d owns a run of hosts)."""
    return HostPartition(sc["hosts"]["route"], wc.H, W)


def delivered(r):
    """(index in the round's batch, destination host) of a sending round's delivered packets."""
    want = r["want"]
    off = want["dst_offsets"].astype(np.int64)
    return want["dst_order"].astype(np.int64), np.repeat(np.arange(len(off) - 1), np.diff(off))


def pair_counts(sc, part):
    """Per sending round the W x W matrix: records rank s sends rank d."""
    out = []
    for r in sc["rounds"][:wc.SEND_ROUNDS]:
        p, dst = delivered(r)
        m = np.zeros((part.world, part.world), np.int64)
        np.add.at(m, (part.owner[r["pk"]["src"][p]], part.owner[dst]), 1)
        out.append(m)
    return out


def padded_cap(sc):
    """Block size of the padded test: the median, over the sending rounds, of the round's largest
    pair count (W = PADDED_W).  About half of the rounds overflow it, about half fit."""
    return int(np.median([m.max() for m in pair_counts(sc, partition(sc, PADDED_W))]))


def dst_of_packet(sc):
    """Destination host of every packet id of the scenario (-1: never delivered)."""
    if _cache.get("dst_of") is not sc:  # one scenario at a time
        d = np.full(sc["n_pk"], -1, np.int64)
        for r in sc["rounds"][:wc.SEND_ROUNDS]:
            p, dst = delivered(r)
            d[r["id_base"] + p] = dst
        _cache["dst"], _cache["dst_of"] = d, sc
    return _cache["dst"]


def rank_pop(sc, part, d, k, slots=False):
    """(pop, next_time_ns) of rank d's wire in round k: the scenario's restricted to the hosts rank d
    owns (still grouped by ascending host, each host's in EventQueue order).  slots: hosts renumbered
    to the rank's local slots, for a wire over its own hosts."""
    r = sc["rounds"][k]
    m = part.owner[r["pop"]["host"]] == d
    pop = {key: r["pop"][key][m] for key in POP_KEYS + ("tag",)}
    held = r["held"]
    t = held["time_ns"][part.owner[held["host"]] == d]
    if slots:
        pop["host"] = part.local[pop["host"]]
    return pop, (int(t.min()) if len(t) else NEVER)
