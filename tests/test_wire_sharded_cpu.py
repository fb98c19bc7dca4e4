"""CPU-only checks of the wire on the sharded path (sg_wire_stamp_records[_padded],
sg_wire_push_records[_padded]): the symbols and their argument rejection without a device, the
stamped record's layout, and -- on the oracle's run alone -- that the scenario the GPU tests of
tests/test_wire_sharded_gpu.py run exercises what they claim under W = 2 and 3 ranks, and that
the padded test's block size makes some rounds overflow and some fit."""
import ctypes as C

import numpy as np
import pytest

import shadow_amd
import wire_cases as wc
import wire_sharded_cases as ws
from shadow_amd import _capi
from shadow_amd.dist import RECORD_DTYPE, WIRE_RECORD_DTYPE

INVALID = _capi.SG_ERR_INVALID_ARG
NEW = ("sg_wire_stamp_records", "sg_wire_stamp_records_padded", "sg_wire_push_records", "sg_wire_push_records_padded")


def test_symbols_exported_and_null_arguments_rejected():
    L = shadow_amd.load()  # dlopen only: no device call is made below
    for name in NEW:
        assert hasattr(L, name) and name in _capi.EXPORTED, name
    buf = (C.c_uint64 * 8)()  # stands for any non-null array: nothing reads it
    p = C.addressof(buf)
    # no context
    assert L.sg_wire_stamp_records(None, p, 1, None, 0, p, 1) == INVALID
    assert L.sg_wire_stamp_records_padded(None, p, p, 2, 1, p, None, 0, p, 1) == INVALID
    # null records / len / xrow
    assert L.sg_wire_stamp_records(None, None, 1, None, 0, p, 1) == INVALID
    assert L.sg_wire_stamp_records(None, p, 1, None, 0, None, 1) == INVALID
    assert L.sg_wire_stamp_records_padded(None, None, p, 2, 1, p, None, 0, p, 1) == INVALID
    assert L.sg_wire_stamp_records_padded(None, p, None, 2, 1, p, None, 0, p, 1) == INVALID
    assert L.sg_wire_stamp_records_padded(None, p, p, 2, 1, None, None, 0, p, 1) == INVALID
    assert L.sg_wire_stamp_records_padded(None, p, p, 2, 1, p, None, 0, None, 1) == INVALID
    # no wire
    assert L.sg_wire_push_records(None, None, p, 1, None, 4) == INVALID
    assert L.sg_wire_push_records_padded(None, None, p, 2, 1, p, 0, None, 4) == INVALID
    assert L.sg_wire_push_records_padded(None, None, None, 2, 1, None, 0, None, 4) == INVALID
    assert L.sg_abi_version() == 7  # additive


def test_wire_record_is_a_second_reading_of_the_record():
    assert WIRE_RECORD_DTYPE.itemsize == RECORD_DTYPE.itemsize == 32
    off = {k: WIRE_RECORD_DTYPE.fields[k][1] for k in WIRE_RECORD_DTYPE.names}
    assert off == dict(deliver_time_ns=0, len=8, src_host=12, event_id=16, packet_id=24, dst_host=28)
    old = {k: RECORD_DTYPE.fields[k][1] for k in RECORD_DTYPE.names}
    assert off["deliver_time_ns"] == old["deliver_time_ns"] and off["event_id"] == old["event_id"]
    assert off["len"] == old["order_key"] and off["src_host"] == old["order_key"] + 4  # little-endian halves
    assert off["packet_id"] == old["packet"] and off["dst_host"] == old["dst_host"]
    # one record read both ways
    r = np.zeros(1, RECORD_DTYPE)
    r["deliver_time_ns"], r["order_key"], r["event_id"], r["packet"], r["dst_host"] = 11, (7 << 32) | 1476, 2**40, 99, 5
    w = r.view(WIRE_RECORD_DTYPE)
    assert (int(w["len"][0]), int(w["src_host"][0]), int(w["packet_id"][0]), int(w["dst_host"][0])) == (1476, 7, 99, 5)
    assert int(w["deliver_time_ns"][0]) == 11 and int(w["event_id"][0]) == 2**40


@pytest.mark.parametrize("W", [2, 3])
def test_scenario_conditions_under_a_partition(oracle, W):
    sc = wc.scenario(oracle)
    part = ws.partition(sc, W)
    assert sorted(part.n_local(d) for d in range(W)) == ([32, 32] if W == 2 else [20, 22, 22])
    counts = ws.pair_counts(sc, part)
    # every rank receives records from every rank in some round
    assert (np.max(counts, axis=0) > 0).all()
    # at least one pop on every rank holds events of three or more rounds
    for d in range(W):
        assert max(len(np.unique(ws.rank_pop(sc, part, d, k)[0]["tag"])) for k in range(wc.ROUNDS)) >= 3, d
    # the ranks' pops together are the scenario's pop, round by round
    for k in range(wc.ROUNDS):
        assert sum(len(ws.rank_pop(sc, part, d, k)[0]["host"]) for d in range(W)) == len(sc["rounds"][k]["pop"]["host"])


def test_padded_cap_makes_rounds_overflow_and_rounds_fit(oracle):
    """The padded GPU test runs round 0 exactly and rounds 1 .. SEND_ROUNDS - 1 through blocks of
    this cap: among those, some round's largest pair count must exceed it and some must not."""
    sc = wc.scenario(oracle)
    cap = ws.padded_cap(sc)
    pm = [int(m.max()) for m in ws.pair_counts(sc, ws.partition(sc, ws.PADDED_W))]
    assert len(pm) == wc.SEND_ROUNDS and cap > 0
    assert any(x > cap for x in pm[1:]), (cap, pm)
    assert any(x <= cap for x in pm[1:]), (cap, pm)
    # an overflowing round has blocks that are full and blocks that are not
    over = [m for m in ws.pair_counts(sc, ws.partition(sc, ws.PADDED_W))[1:] if m.max() > cap]
    assert any((m <= cap).any() for m in over)
