"""What the link-queue tests on the card share (test_queue_gpu.py, test_queue_carry_gpu.py,
test_queue_drop_gpu.py): one raw sg_link_queue call on a case's arrays with every output starting
from sentinel values, the loop over modes and forms that compares it with a reference, and the
objects of a real round."""
import numpy as np

import queue_cases as QC
import queue_ref as QR

VIEW = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
FORMS = ("scan", "serial")
INPUTS = ("link_off", "enter", "packet", "weight", "cost_ps", "free_in")
CARRY, DROP = 4, 8  # (the flag bits, by value: the two reference test files hold the layers' constants to them)


def _sentinels(c, names, drop=False):
    """The outputs `names`; under the drop flag busy and ahead_max have two entries per link."""
    n, nl = len(c["enter"]), len(c["link_off"]) - 1
    size = lambda k: n if k in QR.RECORD_FIELDS else (2 * nl if drop and k in ("busy", "ahead_max") else nl)  # noqa: E731
    return {k: np.full(size(k), QC.SENT32 if QR.DTYPES[k] == np.uint32 else QC.SENT64, QR.DTYPES[k]) for k in names}


def _call(ctx, c, names=QR.FIELDS, *, dev, carry=False, drop=False, handle=True, alias_free=False, n_records=None):
    """One sg_link_queue call on a case's arrays, the outputs `names` starting from sentinels.
    Returns (status, outputs by name).  n_weights is the case's n_packets (the weights' length
    where the case has none; 0 under the drop flag alone when there are no weights to count)."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    outs = _sentinels(c, names, drop)
    keep = []

    def ptr(a):
        if a is None:
            return None
        if not dev:
            return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(np.zeros(1, a.dtype).ctypes.data)
        t = torch.from_numpy(np.ascontiguousarray(a).view(VIEW[a.dtype]).copy() if a.size else np.zeros(1, VIEW[a.dtype])).cuda()
        keep.append((a, t))
        return C.c_void_p(t.data_ptr())

    arrays = dict(c, cost_ps=np.concatenate([c["cost_ps"], c["limit_ns"]]) if drop else c["cost_ps"])
    ip = [ptr(arrays[k]) for k in INPUTS]
    n_in = len(keep)
    op = {k: ptr(outs[k]) if k in outs else None for k in QR.FIELDS}
    if alias_free:
        op["link_free"] = ip[5]
    if dev:
        torch.cuda.synchronize()
    if "n_packets" in c and (carry or not drop or c["weight"] is not None):
        n_weights = c["n_packets"]
    else:
        n_weights = 0 if c["weight"] is None else len(c["weight"])
    flags = (_capi.SG_ROUTE_OUT_DEVICE if dev else 0) | (CARRY if carry else 0) | (DROP if drop else 0)
    rc = _capi.load().sg_link_queue(ctx.handle if handle else None, flags, len(c["link_off"]) - 1, ip[0],
                                    len(c["enter"]) if n_records is None else n_records, ip[1], ip[2], ip[3], n_weights,
                                    ip[4], ip[5], *[op[k] for k in QR.FIELDS])
    if dev:
        torch.cuda.synchronize()
        for a, t in keep[n_in:]:
            if a.size:
                a[...] = t.cpu().numpy().view(a.dtype)
    return rc, outs


def _pair(ctx):
    from shadow_amd import _capi

    r, k = _capi.C.c_uint32(), _capi.C.c_uint32()
    _capi.load().sg_ctx_last_error_pair(ctx.handle, _capi.C.byref(r), _capi.C.byref(k))
    return r.value, k.value


def _untouched(outs):
    return all((a == (QC.SENT32 if a.dtype == np.uint32 else QC.SENT64)).all() for a in outs.values())


def _form(monkeypatch, form):
    monkeypatch.setenv("SG_LINK_QUEUE_SERIAL", "1" if form == "serial" else "0")


def _iters(ctx):
    return int(ctx.read_timer("link_queue_iters")[1])


def ctx_error(ctx):
    from shadow_amd import _capi

    return _capi.load().sg_ctx_last_error(ctx.handle).decode()


def _check_calls(ctx, monkeypatch, c, want, names, *, carry=False, drop=False, devs=(True, False), forms=FORMS, iters=None):
    """The case in every mode and form against `want`, the expected array per output name; iters:
    the iterations every carried call must have taken."""
    from shadow_amd import _capi

    ctx.enable_timers(True)  # (read_timer("link_queue_serial") tells the form the last call took)
    try:
        for form in forms:
            _form(monkeypatch, form)
            for dev in devs:
                rc, outs = _call(ctx, c, names, dev=dev, carry=carry, drop=drop)
                _capi.check(ctx.handle, rc)
                assert int(ctx.read_timer("link_queue_serial")[1]) == (form == "serial")
                assert iters is None or _iters(ctx) == iters
                for k in names:
                    w = want[k]
                    assert np.array_equal(outs[k], w), \
                        f"{k} ({form}, {'device' if dev else 'host'}): {int((outs[k] != w).sum())} of {w.size} differ, " \
                        f"first at {int(np.flatnonzero(outs[k] != w)[0])}"
    finally:
        ctx.enable_timers(False)


# ---- a real round's objects
def _net(g, ctx):
    from shadow_amd import NetworkGraph

    return NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)


def _host_table(hosts, ctx):
    from shadow_amd.worker import HostTable

    return HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)


def _batch(pk):
    from shadow_amd.worker import PacketBatch

    return PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"])


PY_FIELDS = dict(zip(("wait_ns", "done_ns", "ahead", "link_free", "link_busy_ns", "link_wait_max_ns", "link_wait_sum_ns",
                      "link_ahead_max"), QR.FIELDS))
