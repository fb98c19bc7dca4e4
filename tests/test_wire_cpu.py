"""CPU-only checks of the packet wire: argument rejection of sg_wire_* without a device, the
reference model tests/wire_ref.py against hand-written cases, and that the closed-loop scenario
the GPU tests run (tests/wire_cases.py) exercises what it is meant to."""
import ctypes as C
import os
import re

import numpy as np

import shadow_amd
from shadow_amd import _capi, wire
from wire_ref import NEVER, WireRef

INVALID = _capi.SG_ERR_INVALID_ARG


def test_null_and_zero_arguments_rejected():
    L = shadow_amd.load()  # dlopen only: no device call is made below
    h = C.c_void_p()
    assert L.sg_wire_create(None, 4, 16, 1000, 8, C.byref(h)) == INVALID and not h.value
    assert L.sg_wire_create(None, 0, 0, 0, 0, C.byref(h)) == INVALID and not h.value
    assert L.sg_wire_create(None, 4, 16, 1000, 8, None) == INVALID
    p, d = _capi.sg_packets(), _capi.sg_deliveries()
    assert L.sg_wire_push(None, None, C.byref(p), C.byref(d), None, 0, None) == INVALID
    assert L.sg_wire_push(None, None, None, None, None, 0, None) == INVALID
    o, n = _capi.sg_wire_arrivals(), C.c_uint32()
    assert L.sg_wire_pop(None, None, 5, C.byref(o), C.byref(n), None) == INVALID
    assert L.sg_wire_pop(None, None, 5, None, None, None) == INVALID
    s, m = _capi.sg_wire_state(), C.c_uint64()
    assert L.sg_wire_get_state(None, 0, C.byref(s), C.byref(m)) == INVALID
    assert L.sg_wire_set_state(None, 0, C.byref(s)) == INVALID
    assert L.sg_wire_count(None) == 0
    L.sg_wire_destroy(None)
    assert L.sg_abi_version() == 7  # the wire is additive


def test_sort_limits_match_the_kernels():
    src = open(os.path.join(os.path.dirname(_capi.LIB_PATH), "csrc", "sg_wire.hip")).read()
    assert int(re.search(r"WR_RANK_SORT_MAX = (\d+);", src).group(1)) == wire.RANK_SORT_MAX
    assert int(re.search(r"WR_LDS_SORT_MAX = (\d+);", src).group(1)) == wire.LDS_SORT_MAX


def _ev(w, rows):
    cols = list(zip(*rows))
    w.add(host=cols[0], time_ns=cols[1], src_host=cols[2], event_id=cols[3], packet=cols[4],
          len=np.full(len(rows), 100))


def test_ref_boundary_time_equal_to_window_end_stays():
    w = WireRef()
    T = 10**9
    _ev(w, [(0, T - 1, 1, 0, 10), (0, T, 1, 1, 11), (0, T + 1, 1, 2, 12)])
    out, nxt = w.pop(T)
    assert out["packet"].tolist() == [10] and nxt == T and len(w) == 2
    out, nxt = w.pop(T)
    assert len(out["packet"]) == 0 and nxt == T
    out, nxt = w.pop(T + 1)
    assert out["packet"].tolist() == [11] and nxt == T + 1
    out, nxt = w.pop(NEVER)
    assert out["packet"].tolist() == [12] and nxt == NEVER and len(w) == 0


def test_ref_ties_by_source_then_event_id():
    w = WireRef()
    T = 5000
    # (host, time, src, event id, packet): appended against the order they must leave in
    _ev(w, [(2, T, 9, 0, 0), (1, T, 5, 2**40 + 1, 1), (1, T, 5, 7, 2), (1, T, 3, 99, 3), (1, T - 1, 8, 5, 4),
            (0, T + 5, 0, 0, 5)])
    out, nxt = w.pop(T + 1)
    assert out["host"].tolist() == [1, 1, 1, 1, 2]
    assert out["packet"].tolist() == [4, 3, 2, 1, 0]  # time, then source 3 < 5, then event id 7 < 2^40 + 1
    assert nxt == T + 5
    assert w.state()["packet"].tolist() == [5]


def test_ref_push_takes_hosts_from_the_buckets():
    res = dict(dst_order=np.array([2, 0, 3], np.uint32), dst_offsets=np.array([0, 1, 1, 3], np.uint32),
               deliver_time=np.array([50, 0, 60, 70], np.uint64), event_id=np.array([4, 2**64 - 1, 8, 9], np.uint64))
    w = WireRef()
    w.push(res, src_host=[1, 1, 2, 2], length=[10, 11, 12, 13], id_base=100)
    s = w.state()
    assert s["host"].tolist() == [0, 2, 2] and s["packet"].tolist() == [102, 100, 103]
    assert s["time_ns"].tolist() == [60, 50, 70] and s["len"].tolist() == [12, 10, 13]
    assert s["src_host"].tolist() == [2, 1, 2] and s["event_id"].tolist() == [8, 4, 9]


def test_scenario_exercises_what_it_claims(oracle):
    """Asserted on the reference side, so the GPU comparison cannot pass vacuously."""
    import wire_cases as wc

    sc = wc.scenario(oracle)
    rounds = sc["rounds"]
    # some pop returns events pushed in at least three different earlier rounds
    assert max(len(np.unique(r["pop"]["tag"])) for r in rounds) >= 3
    # some event waited more than 16 bins of 1 ms (it went through the far list of a 16-bin ring)
    waited = max(int(((r["end"] - wc.T0) // wc.MS - 1 - r["pop"]["tag"]).max()) for r in rounds if len(r["pop"]["tag"]))
    assert waited > 16
    # some pop leaves a host empty-handed while other hosts receive
    assert any(len(r["pop"]["host"]) and len(np.unique(r["pop"]["host"])) < wc.H for r in rounds)
    assert any(wc.QUIET_HOST in r["pop"]["host"] for r in rounds)
    # the reference inbound run raised no capacity error (scenario() would have thrown); packets were lost,
    # and the store still holds events when the sends stop and is empty at the end
    assert any((r["want"]["status"] == _capi.SG_PKT_DROP_LOSS).any() for r in rounds[:wc.SEND_ROUNDS])
    assert len(rounds[wc.SEND_ROUNDS - 1]["held"]["host"]) > 0 and len(rounds[-1]["held"]["host"]) == 0
    assert rounds[-1]["next"] == NEVER
