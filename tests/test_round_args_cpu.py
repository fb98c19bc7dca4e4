"""shadow_amd.round_args, the one home of the round entry points' argument marshalling, against
what the copies it replaced did (PathTree's to_dev and watch blocks, _base_times, LinkQueueSession.
_tensor, the capacity loops, Group's per-member weights).  On torch's CPU device: 5 packets, 6 links.
No GPU."""
import importlib
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from shadow_amd import _capi
from shadow_amd import round_args as RA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
NPK, NLINKS = 5, 6
KINDS = [(np.uint8, torch.uint8, np.int16, torch.uint8), (np.uint32, torch.int32, np.int64, torch.int32),
         (np.uint64, torch.int64, np.uint64, torch.int64)]  # (asked for, the view, a wider numpy dtype, a torch dtype)


def _values(np_dtype, n=NPK):
    return [(3 * i + 1) % 200 for i in range(n)] if np_dtype == np.uint8 else [1000 * i + 7 for i in range(n)]


@pytest.mark.parametrize("np_dtype,view,wider,t_dtype", KINDS)
def test_int_tensor_inputs_agree(np_dtype, view, wider, t_dtype):
    vals = _values(np_dtype)
    want = np.array(vals, np_dtype)
    for x in (vals, want, np.array(vals, wider), torch.tensor(vals, dtype=t_dtype), want.reshape(NPK, 1)):
        got = RA.int_tensor(x, np_dtype, NPK, CPU, "arg")
        assert got.dtype == view and got.dim() == 1 and got.is_contiguous() and got.device == CPU
        assert np.array_equal(got.numpy().view(np_dtype), want)
    strided = torch.tensor(_values(np_dtype, 2 * NPK), dtype=t_dtype)[::2]  # (a tensor that is not contiguous)
    got = RA.int_tensor(strided, np_dtype, NPK, CPU, "arg")
    assert got.is_contiguous() and np.array_equal(got.numpy().view(np_dtype), np.array(_values(np_dtype, 2 * NPK)[::2], np_dtype))


@pytest.mark.parametrize("np_dtype,view,wider,t_dtype", KINDS)
def test_int_tensor_counts(np_dtype, view, wider, t_dtype):
    with pytest.raises(ValueError) as e:
        RA.int_tensor(_values(np_dtype, 4), np_dtype, NPK, CPU, "the_arg")
    assert "the_arg" in str(e.value) and "5" in str(e.value)
    with pytest.raises(ValueError):
        RA.int_tensor(torch.tensor(_values(np_dtype, 4), dtype=t_dtype), np_dtype, NPK, CPU, "the_arg")
    # the rule for a longer input: at least `count`, all of it kept (PathTree's to_dev; _base_times and
    # LinkQueueSession._tensor slice the result themselves)
    for x in (_values(np_dtype, 7), torch.tensor(_values(np_dtype, 7), dtype=t_dtype)):
        got = RA.int_tensor(x, np_dtype, NPK, CPU, "arg")
        assert got.numel() == 7 and np.array_equal(got.numpy().view(np_dtype), np.array(_values(np_dtype, 7), np_dtype))


def test_int_tensor_rejects_other_tensors():
    with pytest.raises(ValueError):
        RA.int_tensor(torch.zeros(NPK, dtype=torch.float32), np.uint32, NPK, CPU, "weight")
    with pytest.raises(ValueError):
        RA.int_tensor(torch.zeros(NPK, dtype=torch.int16), np.uint32, NPK, CPU, "weight")
    with pytest.raises(ValueError):
        RA.int_tensor(torch.zeros(NPK, dtype=torch.float64), np.uint64, NPK, CPU, "outcomes")


def test_int_tensor_u64_top_bit():
    vals = np.array([1 << 63, (1 << 64) - 1, (1 << 63) + 12345, 0, 1], np.uint64)
    got = RA.int_tensor(vals, np.uint64, NPK, CPU, "outcomes")
    assert got.dtype == torch.int64 and got.tolist() == [-(1 << 63), -1, -(1 << 63) + 12345, 0, 1]
    assert np.array_equal(got.numpy().view(np.uint64), vals)
    again = RA.int_tensor(got, np.uint64, NPK, CPU, "outcomes")  # (the int64 view of one passes as it is)
    assert np.array_equal(again.numpy().view(np.uint64), vals)


def test_int_tensor_unwraps():
    st = np.array([1, 0, 1, 2, 1], np.uint8)
    times = np.array([5, 6, 7, 8, 1 << 63], np.uint64)
    deliveries = SimpleNamespace(status=torch.from_numpy(st), deliver_time_ns=torch.from_numpy(times.view(np.int64)))
    assert np.array_equal(RA.int_tensor(deliveries, np.uint8, NPK, CPU, "status", "status").numpy(), st)
    assert np.array_equal(RA.int_tensor(deliveries, np.uint64, NPK, CPU, "outcomes", "deliver_time_ns").numpy().view(np.uint64), times)
    assert np.array_equal(RA.int_tensor(st, np.uint8, NPK, CPU, "status", "status").numpy(), st)  # (a bare array passes)


def test_base_times_and_session_tensor_cut_to_count():
    """The two callers that cut a longer input to the count, as their parents did."""
    from shadow_amd.link_queue import _base_times
    from shadow_amd.queue_session import LinkQueueSession

    times = np.arange(7, dtype=np.uint64) + (1 << 63)
    got = _base_times(SimpleNamespace(deliver_time_ns=times), NPK, CPU)
    assert got.dtype == torch.int64 and got.is_contiguous() and np.array_equal(got.numpy().view(np.uint64), times[:NPK])
    with pytest.raises(ValueError, match="outcomes"):
        _base_times(times[:4], NPK, CPU)
    s = SimpleNamespace(dev=CPU)
    got = LinkQueueSession._tensor(s, list(range(7)), np.uint32, torch.int32, NPK, "packet")
    assert got.dtype == torch.int32 and got.tolist() == [0, 1, 2, 3, 4]
    assert LinkQueueSession._tensor(s, None, np.uint32, torch.int32, 0, "packet").numel() == 0
    with pytest.raises(ValueError):
        LinkQueueSession._tensor(s, None, np.uint32, torch.int32, NPK, "packet")


def test_weight_arg():
    batch = SimpleNamespace(payload_len=torch.arange(NPK, dtype=torch.int32))
    assert RA.weight_arg(None, batch) is None
    assert RA.weight_arg("payload", batch) is batch.payload_len
    w = [1, 2, 3, 4, 5]
    assert RA.weight_arg(w, batch) is w
    with pytest.raises(ValueError):
        RA.weight_arg("bytes", batch)


def test_watch_mask():
    assert RA.watch_mask(None, NLINKS) is None
    flags = np.array([1, 0, 0, 1, 1, 0], bool)
    got = RA.watch_mask(flags, NLINKS)
    assert got.dtype == np.uint8 and got.flags.c_contiguous and got.tolist() == [1, 0, 0, 1, 1, 0]
    with pytest.raises(ValueError):
        RA.watch_mask(np.ones(5, bool), NLINKS)
    u8 = np.array([0, 1, 0, 0, 0, 5], np.uint8)  # (one entry per link: a mask, not link numbers)
    got = RA.watch_mask(u8, NLINKS)
    assert got.dtype == np.uint8 and got.tolist() == [0, 1, 0, 0, 0, 5]
    assert RA.watch_mask(np.array([1, 4], np.uint8), NLINKS).tolist() == [0, 1, 0, 0, 1, 0]  # (another shape: link numbers)
    assert RA.watch_mask([0, 5, 5], NLINKS).tolist() == [1, 0, 0, 0, 0, 1]
    for bad in ([6], [-1]):
        with pytest.raises(ValueError):
            RA.watch_mask(bad, NLINKS)
    got = RA.watch_mask([], NLINKS)
    assert got.dtype == np.uint8 and got.tolist() == [0] * NLINKS


def _retry(answers):
    """with_capacity over a fake call that answers (rc, total) in turn; the caps and array lengths seen."""
    seen, answers = [], list(answers)

    def call(arrays, cap):
        seen.append((cap, [len(a) for a in arrays]))
        return answers.pop(0)

    rc, total, arrays = RA.with_capacity(1, lambda cap: [np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)], call)
    assert not answers and [len(a) for a in arrays] == seen[-1][1]
    return rc, total, seen


def test_with_capacity():
    CAP = _capi.SG_ERR_CAPACITY
    other = _capi.SG_ERR_INVALID_ARG
    assert _retry([(CAP, 100), (_capi.SG_OK, 100)]) == (_capi.SG_OK, 100, [(72, [72, 72]), (100, [100, 100])])
    assert _retry([(_capi.SG_OK, 72)]) == (_capi.SG_OK, 72, [(72, [72, 72])])
    assert _retry([(CAP, 72)]) == (CAP, 72, [(72, [72, 72])])  # (total <= cap: the status goes back)
    assert _retry([(CAP, 10)]) == (CAP, 10, [(72, [72, 72])])
    assert _retry([(other, 0)]) == (other, 0, [(72, [72, 72])])
    assert _retry([(other, 1000)]) == (other, 1000, [(72, [72, 72])])
    assert _retry([(_capi.SG_OK, 3)]) == (_capi.SG_OK, 3, [(72, [72, 72])])
    assert _retry([(CAP, 100), (CAP, 130), (_capi.SG_OK, 130)])[2] == [(72, [72, 72]), (100, [100, 100]), (130, [130, 130])]


class _Batch:
    """What the weight functions read of a PacketBatch: its length and its payload_len."""

    def __init__(self, payload_len):
        self.payload_len = payload_len

    def __len__(self):
        return len(self.payload_len)


def test_member_weights():
    batches = [_Batch(torch.arange(k, dtype=torch.int32) + 40 * k) for k in (2, 3, 5)]
    devs = [CPU] * 3
    assert RA.member_weights(None, batches, devs) is None
    got = RA.member_weights([np.array([7, 1 << 31], np.int64), None, torch.arange(7, dtype=torch.int32)], batches, devs)
    assert got[1] is None and got[0].dtype == got[2].dtype == torch.int32
    assert got[0].numpy().view(np.uint32).tolist() == [7, 1 << 31] and got[2].tolist() == list(range(7))
    with pytest.raises(ValueError):
        RA.member_weights([[1, 2], None], batches, devs)  # (two entries for three members)
    with pytest.raises(ValueError) as e:
        RA.member_weights([[1, 2], None, [1, 2, 3, 4]], batches, devs)  # (member 2 has 5 packets)
    assert "weight[2]" in str(e.value) and "5" in str(e.value)
    with pytest.raises(ValueError):
        RA.member_weights("bytes", batches, devs)
    got = RA.member_weights("payload", batches, devs)
    assert [g.tolist() for g in got] == [b.payload_len.tolist() for b in batches]
    # the concatenated form of Group.link_queue_round: ones for None, every part cut to its member's packets
    parts = RA.member_weights([[9, 8, 7], None, torch.arange(7, dtype=torch.int32)], batches, devs)
    cat = RA.concat_weights(parts, batches, CPU)
    assert cat.dtype == torch.int32 and cat.is_contiguous() and cat.tolist() == [9, 8, 1, 1, 1, 0, 1, 2, 3, 4]
    assert RA.concat_weights(None, batches, CPU) is None and RA.concat_weights([], [], CPU) is None


def test_series_out():
    series, outside = np.zeros((4, 3), np.uint64), np.zeros((4, 2), np.uint64)
    assert RA.series_out((series, outside), 4, 3)[0] is series
    for bad in ((series.astype(np.int64), outside), (series, outside.astype(np.int64)), (np.zeros((4, 2), np.uint64), outside),
                (series, np.zeros((3, 2), np.uint64)), (np.zeros((3, 4), np.uint64).T, outside)):
        with pytest.raises(ValueError):
            RA.series_out(bad, 4, 3)
    view = np.zeros((3, 4), np.uint64).T  # (the group copies a view in and writes it back: only PathTree needs it contiguous)
    assert RA.series_out((view, outside), 4, 3, contiguous=False)[0] is view


PUBLIC = ["series_slots", "LinkQueueResult", "LinkQueueCarried", "LinkQueueDropped", "LinkQueueCarriedDropped", "PacketOutcomes",
          "WHERE_ARRIVED", "WHERE_NOTHING", "WHERE_IN_FLIGHT", "link_queue_pending", "queue_limit_ns", "cost_ps_from_bandwidth",
          "link_queue"]


def test_graph_reexports_link_queue():
    import shadow_amd
    from shadow_amd import graph

    lq = importlib.import_module("shadow_amd.link_queue")  # (the package's attribute of that name is the function)
    for name in PUBLIC:
        assert getattr(graph, name) is getattr(lq, name), name
        if name != "series_slots":
            assert getattr(shadow_amd, name) is getattr(lq, name), name
    assert not hasattr(graph, "_link_queue_tensors") or graph._link_queue_tensors is lq._link_queue_tensors


def test_link_queue_imports_alone():
    code = ("import sys, shadow_amd.link_queue; m = sys.modules['shadow_amd.link_queue']; "
            "assert callable(m.link_queue) and callable(m._step_windows); print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
    # and without the package's __init__ having pulled in graph first: link_queue does not need it
    code = ("import sys, types, os; p = types.ModuleType('shadow_amd'); p.__path__ = [os.path.join(%r, 'shadow_amd')]; "
            "sys.modules['shadow_amd'] = p; import shadow_amd.link_queue; "
            "assert 'shadow_amd.graph' not in sys.modules; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
