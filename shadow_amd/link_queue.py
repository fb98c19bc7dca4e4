"""Link queues: the FIFO queue of every link of a link trace under a link rate (sg_link_queue), on
host arrays (`link_queue`) and on a device trace (PathTree.link_queue_round, Group.link_queue_round
and LinkQueueSession call the helpers here), with the result tuples and their sentinels, and the
slot map of the link time series.  A Context is only passed through."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _capi
from ._capi import check, load
from .round_args import int_tensor


def series_slots(slots, n_links: int) -> Tuple[Optional[np.ndarray], int]:
    """(slot map or None, n_slots) of link_series_round's `slots`: None (the identity), a full map
    (a u32 numpy array of one entry per link; n_slots = its largest slot + 1, 0xFFFFFFFF not
    counted) or a list of link numbers (slot = position)."""
    if slots is None:
        return None, n_links
    if isinstance(slots, np.ndarray) and slots.dtype == np.uint32 and slots.shape == (n_links,):
        m = np.ascontiguousarray(slots)
        watched = m[m != 0xFFFFFFFF]
        return m, int(watched.max()) + 1 if len(watched) else 1
    idx = np.asarray(slots).astype(np.int64).ravel()
    if len(idx) == 0 or idx.min() < 0 or idx.max() >= n_links or len(np.unique(idx)) != len(idx):
        raise ValueError(f"slots: distinct link numbers below {n_links}, at least one")
    m = np.full(n_links, 0xFFFFFFFF, np.uint32)
    m[idx] = np.arange(len(idx), dtype=np.uint32)
    return m, len(idx)


class LinkQueueResult(NamedTuple):
    """What sg_link_queue gives: per record wait_ns, done_ns (u64) and ahead (u32, the records of
    the link still in the system on arrival); per link link_free (u64, when its server is free
    after the last record), link_busy_ns (the summed service), link_wait_max_ns, link_wait_sum_ns
    (u64) and link_ahead_max (u32)."""
    wait_ns: np.ndarray
    done_ns: np.ndarray
    ahead: np.ndarray
    link_free: np.ndarray
    link_busy_ns: np.ndarray
    link_wait_max_ns: np.ndarray
    link_wait_sum_ns: np.ndarray
    link_ahead_max: np.ndarray


class LinkQueueCarried(NamedTuple):
    """What sg_link_queue gives with SG_LINK_QUEUE_CARRY (carry=True): LinkQueueResult's eight
    fields over the carried schedule, at the input records' indices; enter_ns (u64), the carried
    enter time of every record, done - service - wait; and the iterations the fixed point took."""
    wait_ns: np.ndarray
    done_ns: np.ndarray
    ahead: np.ndarray
    link_free: np.ndarray
    link_busy_ns: np.ndarray
    link_wait_max_ns: np.ndarray
    link_wait_sum_ns: np.ndarray
    link_ahead_max: np.ndarray
    enter_ns: np.ndarray
    iterations: int


class LinkQueueDropped(NamedTuple):
    """What sg_link_queue gives with SG_LINK_QUEUE_DROP (limit_ns=...): LinkQueueResult's eight
    fields, the per-link arrays cut back to n_links entries and running over served records only;
    dropped (bool per record: wait_ns is then 2^64 - 1 and done_ns its enter time); per link
    link_drops (u32, the records dropped) and link_refused_ns (u64, their summed service)."""
    wait_ns: np.ndarray
    done_ns: np.ndarray
    ahead: np.ndarray
    link_free: np.ndarray
    link_busy_ns: np.ndarray
    link_wait_max_ns: np.ndarray
    link_wait_sum_ns: np.ndarray
    link_ahead_max: np.ndarray
    dropped: np.ndarray
    link_drops: np.ndarray
    link_refused_ns: np.ndarray


class LinkQueueCarriedDropped(NamedTuple):
    """What sg_link_queue gives with SG_LINK_QUEUE_CARRY and SG_LINK_QUEUE_DROP: LinkQueueDropped's
    fields over the carried schedule; absent (bool per record: a record after a dropped or absent
    one in its packet's chain, it enters no queue, wait_ns and done_ns are 2^64 - 1); enter_ns, the
    carried enter time (done - service - wait served, done_ns dropped, 2^64 - 1 absent); and the
    iterations the fixed point took."""
    wait_ns: np.ndarray
    done_ns: np.ndarray
    ahead: np.ndarray
    link_free: np.ndarray
    link_busy_ns: np.ndarray
    link_wait_max_ns: np.ndarray
    link_wait_sum_ns: np.ndarray
    link_ahead_max: np.ndarray
    dropped: np.ndarray
    link_drops: np.ndarray
    link_refused_ns: np.ndarray
    absent: np.ndarray
    enter_ns: np.ndarray
    iterations: int


class PacketOutcomes(NamedTuple):
    """What sg_link_queue gives per packet with SG_LINK_QUEUE_PACKETS (outcomes=...): delay_ns (u64,
    what the queues add to the packet: carried, its last served crossing's done - enter; first
    order, the sum over its served crossings up to its first drop), arrive_ns (u64, base + delay,
    2^64 - 1 when the packet was dropped), where (u32: the record that dropped it, WHERE_ARRIVED
    when it arrived, WHERE_NOTHING when it has no record: not counted, or no watched link on its
    path, and arrive_ns is then its base time); lost (bool); drop_link (u32, the link of `where`,
    2^32 - 1 when not dropped); arrive_dev, arrive_ns as an int64 device tensor for
    PacketWire.push(deliver_time_ns=...) where the call ran on device arrays, else None."""
    delay_ns: np.ndarray
    arrive_ns: np.ndarray
    where: np.ndarray
    lost: np.ndarray
    drop_link: np.ndarray
    arrive_dev: object


WHERE_ARRIVED = 0xFFFFFFFE
WHERE_NOTHING = 0xFFFFFFFF
WHERE_IN_FLIGHT = 0xFFFFFFFD  # with a horizon: a record of the packet is pending, arrive_ns is its re-based base
_UMAX = 0xFFFFFFFFFFFFFFFF


def link_queue_pending(wait_ns, ahead):
    """The pending records of a call with a horizon (SG_LINK_QUEUE_WINDOW), from the sentinels: wait_ns
    2^64 - 1 and ahead 2^32 - 1; done_ns is then the record's re-based enter time, the enter_ns a
    later call takes.  Host arrays or device tensors (a u64 / u32 array, or torch's int64 / int32
    views of one); a bool mask of the same kind."""
    if isinstance(wait_ns, np.ndarray):
        return (wait_ns.view(np.uint64) == np.uint64(_UMAX)) & (np.asarray(ahead).view(np.uint32) == np.uint32(0xFFFFFFFF))
    return (wait_ns == -1) & (ahead == -1)


def _outcomes(link_off, delay, arrive, where, arrive_dev=None, window: bool = False) -> PacketOutcomes:
    """PacketOutcomes from the three tails (host arrays) of a call that succeeded; window: a packet
    may be in flight, which is not lost."""
    lost = where < np.uint32(WHERE_IN_FLIGHT if window else WHERE_ARRIVED)
    link = np.full(len(where), 0xFFFFFFFF, np.uint32)
    if lost.any():
        link[lost] = np.searchsorted(np.asarray(link_off, np.uint64), where[lost].astype(np.uint64), side="right") - 1
    return PacketOutcomes(delay, arrive, where, lost, link, arrive_dev)


def queue_limit_ns(buffer_units, cost_ps):
    """sg_link_queue's limit_ns of a buffer of buffer_units weight units (bytes, with byte weights)
    in front of a link's server: min(ceil(buffer_units cost_ps / 1000), 2^64 - 1), exactly, on
    Python integers.  Sequences (one of them may be a single value) give a u64 array, one limit
    per link."""
    def one(b, c) -> int:
        b, c = int(b), int(c)
        if b < 0 or c < 0:
            raise ValueError("buffer_units, cost_ps: not negative")
        return min(-((-b * c) // 1000), _UMAX)
    if np.ndim(buffer_units) == 0 and np.ndim(cost_ps) == 0:
        return one(buffer_units, cost_ps)
    b, c = np.broadcast_arrays(np.asarray(buffer_units, dtype=object), np.asarray(cost_ps, dtype=object))
    return np.array([one(x, y) for x, y in zip(b.ravel().tolist(), c.ravel().tolist())], dtype=np.uint64)


def _service_ns(link_off, n: int, packet, weight, cost) -> np.ndarray:
    """s = ceil(weight cost / 1000) per record, exactly (host arrays; below 2^64 wherever a record
    was served, since its done is)."""
    off = np.asarray(link_off).astype(np.int64)
    per = np.repeat(np.asarray(cost, np.uint64), np.diff(off))
    w = np.ones(n, np.uint64) if weight is None else np.asarray(weight, np.uint32).astype(np.uint64)[np.asarray(packet).astype(np.int64)]
    if n == 0 or int(per.max()) < 1 << 32:  # (the product fits 64 bits)
        prod = w * per
        return prod // np.uint64(1000) + (prod % np.uint64(1000) != 0).astype(np.uint64)
    return np.array([min(-((-int(a) * int(b)) // 1000), _UMAX) for a, b in zip(w.tolist(), per.tolist())], dtype=np.uint64)


def _dropped(ctx: "Context", raw, n_links: int, link_off, packet, weight, cost, carry: bool):
    """The result of a flagged call that succeeded, from its eight raw arrays (busy and ahead max
    with 2 n_links entries): the states from the sentinels, the per-link arrays cut back."""
    wait, done, ahead, free, busy2, wmax, wsum, amax2 = raw
    out = wait == np.uint64(_UMAX)
    absent = out & (done == np.uint64(_UMAX))
    dropped = out & ~absent
    res = LinkQueueDropped(wait, done, ahead, free, busy2[:n_links], wmax, wsum, amax2[:n_links], dropped,
                           amax2[n_links:2 * n_links], busy2[n_links:2 * n_links])
    if not carry:
        return res
    n = len(done)
    enter = done.copy()
    srv = ~out
    if srv.any():
        s = _service_ns(link_off, n, packet, weight, cost)
        enter[srv] = done[srv] - s[srv] - wait[srv]
    return LinkQueueCarriedDropped(*res, absent, enter, int(ctx.read_timer("link_queue_iters")[1]) if n else 0)


def _exit_carried(exit_ns, enter_ns, queue):
    """The carried exit time per record of a round: exit + (done - enter), 2^64 - 1 at a dropped
    or absent hop."""
    out = exit_ns + (queue.done_ns - enter_ns)
    if isinstance(queue, LinkQueueCarriedDropped):
        out[queue.dropped | queue.absent] = np.uint64(_UMAX)
    return out


def _carried(ctx: "Context", res: LinkQueueResult, link_off, packet, weight, cost) -> LinkQueueCarried:
    """The carried result of a call that succeeded: enter' = done - s - wait, exactly (host arrays;
    s = ceil(weight cost / 1000) is below 2^64 here, since every done is)."""
    n = len(res.done_ns)
    s = _service_ns(link_off, n, packet, weight, cost)
    return LinkQueueCarried(*res, res.done_ns - s - res.wait_ns, int(ctx.read_timer("link_queue_iters")[1]) if n else 0)


def cost_ps_from_bandwidth(bits_per_second, unit_bytes: int = 1):
    """sg_link_queue's cost_ps of a link rate: the picoseconds one weight unit of unit_bytes bytes
    takes at bits_per_second, rounded up (1e9 gives 8,000, 100e9 gives 80).  A sequence of rates
    gives a u64 array, one cost per link."""
    def one(bps) -> int:
        bps = int(bps)
        if bps <= 0:
            raise ValueError("bits_per_second: a positive rate")
        return -((-8 * int(unit_bytes) * 10**12) // bps)
    if np.ndim(bits_per_second) == 0:
        return one(bits_per_second)
    return np.array([one(b) for b in np.asarray(bits_per_second).ravel()], dtype=np.uint64)


def _per_link_u64(x, n_links: int, what: str) -> np.ndarray:
    """One u64 per link from a scalar or an array of n_links entries."""
    if np.ndim(x) == 0:
        return np.full(n_links, int(x), np.uint64)
    a = np.ascontiguousarray(x, dtype=np.uint64)
    if a.shape != (n_links,):
        raise ValueError(f"{what}: one value, or {n_links} entries, one per link")
    return a


def link_queue(ctx: "Context", link_off, enter_ns, packet=None, weight=None, *, cost_ps, free_ns=None, carry=False,
               limit_ns=None, outcomes=None, horizon_ns=None, series=None):
    """The FIFO queue of every link of a link trace under a link rate, on host arrays: link L owns
    records link_off[L] .. link_off[L + 1] (u64 offsets) in arrival order, enter_ns (u64) their
    arrival times, packet (u32) their index into weight (u32; None: every record weighs 1).
    cost_ps: picoseconds of service per weight unit, one value or one per link
    (cost_ps_from_bandwidth); free_ns: when each link's server is free (None: 0).  A record starts
    at max(enter, the link's previous done), takes ceil(weight cost_ps / 1000) ns and waits start -
    enter.  First order, a LinkQueueResult: a wait is not carried to the packet's later hops
    (sg_link_queue).
    carry=True: every wait is carried (SG_LINK_QUEUE_CARRY), a LinkQueueCarried.  packet is then
    required, and without weight the packets number max(packet) + 1.  The records of one packet,
    in ascending enter_ns, are its chain; a record enters at the previous one's done plus the
    input's gap between the two, and every link serves in ascending (carried enter, packet)
    order.  Results stay at the input records' indices.
    limit_ns: one u64 per link, the longest wait the link's buffer holds (queue_limit_ns; 2^64 - 1:
    no limit) (SG_LINK_QUEUE_DROP).  A record that would wait longer is dropped: the server's time
    is unchanged, and with carry=True the packet's later records are absent, they enter no queue.
    A LinkQueueDropped, with carry=True a LinkQueueCarriedDropped.
    outcomes: a u64 array of one base time per packet, its arrival without the rates
    (SG_LINK_QUEUE_PACKETS).  packet is then required, the packets number len(outcomes), as many
    as weight has, and the call returns (the queue result as above, a PacketOutcomes).
    horizon_ns: with carry=True, settle only the records whose carried enter time is below it
    (SG_LINK_QUEUE_WINDOW).  Every other record is pending (link_queue_pending tells which): its wait_ns
    is 2^64 - 1, its ahead 2^32 - 1 and its done_ns, as its enter_ns in the result, the re-based
    enter time a later call takes; it is neither dropped nor absent.  The per-link arrays run over
    settled records, link_free is what the later call takes as free_ns, and a packet with a pending
    record has where == WHERE_IN_FLIGHT, delay_ns what the queues added so far and arrive_ns its
    re-based base (LinkQueueSession keeps all this from round to round).
    series: a LinkQueueSeries (SG_LINK_QUEUE_SERIES); the call's busy time, waiting time, weight served and
    weight dropped per slot and time bin are added into its matrix.  The result is unchanged."""
    if horizon_ns is not None and not carry:
        raise ValueError("horizon_ns: with carry=True")
    if (carry or outcomes is not None) and packet is None:
        raise ValueError("packet: required with carry=True and with outcomes")
    off = np.ascontiguousarray(link_off, dtype=np.uint64)
    n_links = len(off) - 1
    if n_links < 0:
        raise ValueError("link_off: n_links + 1 entries")
    enter = np.ascontiguousarray(enter_ns, dtype=np.uint64)
    n = len(enter)
    pkt = None if packet is None else np.ascontiguousarray(packet, dtype=np.uint32)
    if pkt is not None and len(pkt) != n:
        raise ValueError(f"packet: {n} entries, one per record")
    wt = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint32)
    cost = _per_link_u64(cost_ps, n_links, "cost_ps")
    free = None if free_ns is None else _per_link_u64(free_ns, n_links, "free_ns")
    drop = limit_ns is not None
    nl2 = 2 * n_links if drop else n_links
    cost2 = np.concatenate([cost, _per_link_u64(limit_ns, n_links, "limit_ns")]) if drop else cost
    flags = (_capi.SG_LINK_QUEUE_CARRY if carry else 0) | (_capi.SG_LINK_QUEUE_DROP if drop else 0)
    if horizon_ns is not None:
        if not 0 <= int(horizon_ns) <= _UMAX:
            raise ValueError("horizon_ns: a u64 time")
        flags |= _capi.SG_LINK_QUEUE_WINDOW  # (the horizon rides behind the links' free times)
        free = np.concatenate([np.zeros(n_links, np.uint64) if free is None else free, np.array([int(horizon_ns)], np.uint64)])
    if series is not None:
        series._check(n_links)
        flags |= _capi.SG_LINK_QUEUE_SERIES  # (the header and the slot map ride behind the costs, the matrix behind busy)
        cost2 = series.host_cost(cost2)
    base = None if outcomes is None else np.ascontiguousarray(outcomes, dtype=np.uint64).ravel()
    n_rec = n
    if base is not None:
        if wt is not None and len(wt) != len(base):
            raise ValueError(f"outcomes: {len(wt)} base times, one per packet as weight has them")
        flags |= _capi.SG_LINK_QUEUE_PACKETS
        n_rec = n + len(base)
        enter = np.concatenate([enter, base])
    res = LinkQueueResult(np.zeros(n_rec, np.uint64), np.zeros(n_rec, np.uint64), np.zeros(n_rec, np.uint32),
                          np.zeros(n_links, np.uint64), np.zeros(nl2, np.uint64) if series is None else series.host_busy(nl2),
                          np.zeros(n_links, np.uint64), np.zeros(n_links, np.uint64), np.zeros(nl2, np.uint32))
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    n_weights = 0 if wt is None else len(wt)
    if carry and wt is None:
        n_weights = int(pkt.max()) + 1 if n else 0
    if base is not None:
        n_weights = len(base)
    check(ctx.handle, load().sg_link_queue(
        ctx.handle, flags, n_links, ptr(off), n, ptr(enter if n_rec else np.zeros(1, np.uint64)),
        ptr(pkt if n or pkt is None else np.zeros(1, np.uint32)), ptr(wt), n_weights, ptr(cost2),
        ptr(free), *[ptr(a) for a in res]))
    if series is not None:
        series.add_host(res.link_busy_ns[nl2:])
        res = res._replace(link_busy_ns=res.link_busy_ns[:nl2])
    tails = None
    if base is not None:
        tails = _outcomes(off, res.wait_ns[n:], res.done_ns[n:], res.ahead[n:], window=horizon_ns is not None)
        res = res._replace(wait_ns=res.wait_ns[:n], done_ns=res.done_ns[:n], ahead=res.ahead[:n])
    if drop:
        queue = _dropped(ctx, res, n_links, off, pkt, wt, cost, carry)
    else:
        queue = _carried(ctx, res, off, pkt, wt, cost) if carry else res
    if horizon_ns is not None:
        queue = _windowed(queue)
    return queue if tails is None else (queue, tails)


def _windowed(queue):
    """A carried result of a call with a horizon: a pending record is neither dropped nor absent, and
    its enter_ns is its re-based enter time."""
    pend = link_queue_pending(queue.wait_ns, queue.ahead)
    if not pend.any():
        return queue
    enter = queue.enter_ns.copy()
    enter[pend] = queue.done_ns[pend]
    queue = queue._replace(enter_ns=enter)
    if isinstance(queue, LinkQueueCarriedDropped):
        queue = queue._replace(dropped=queue.dropped & ~pend, absent=queue.absent & ~pend)
    return queue


def _link_queue_tensors(ctx: "Context", dev, n_links: int, off, n_records: int, enter, packet, weight, cost_ps,
                        free_ns, carry: bool = False, n_packets: int = 0, limit_ns=None, base=None, series=None):
    """sg_link_queue on a device trace (torch tensors on `dev`: off, enter, packet; weight or
    None), every output taken and copied to the host.  carry: with SG_LINK_QUEUE_CARRY, a
    LinkQueueCarried; n_packets bounds the packet numbers when there is no weight.  limit_ns: with
    SG_LINK_QUEUE_DROP, a LinkQueueDropped or LinkQueueCarriedDropped.  base: an int64 tensor of
    n_packets base times on `dev` (SG_LINK_QUEUE_PACKETS); enter then has room for them behind
    its records, where a device-to-device copy places them, weight has n_packets entries, and the
    call returns (the queue result, a PacketOutcomes with arrive_dev).  series: a LinkQueueSeries on `dev`
    (SG_LINK_QUEUE_SERIES): the call adds into its matrix."""
    import torch

    up = lambda a: torch.from_numpy(a.view(np.int64)).to(dev)  # noqa: E731
    h_cost = _per_link_u64(cost_ps, n_links, "cost_ps")
    drop = limit_ns is not None
    nl2 = 2 * n_links if drop else n_links
    cost = up(np.concatenate([h_cost, _per_link_u64(limit_ns, n_links, "limit_ns")]) if drop else h_cost)
    free = None if free_ns is None else up(_per_link_u64(free_ns, n_links, "free_ns"))
    n_tail = 0
    if base is not None:
        n_tail = n_packets
        if enter.numel() < n_records + n_tail or base.numel() < n_tail or (weight is not None and weight.numel() != n_tail):
            raise ValueError("outcomes: one base time per packet, and room for them behind the records")
        enter[n_records:n_records + n_tail].copy_(base[:n_tail])
    rec = lambda dt: torch.zeros(max(n_records + n_tail, 1), dtype=dt, device=dev)  # noqa: E731
    lnk = lambda dt, k=n_links: torch.zeros(max(k, 1), dtype=dt, device=dev)  # noqa: E731
    outs = [rec(torch.int64), rec(torch.int64), rec(torch.int32), lnk(torch.int64), lnk(torch.int64, nl2), lnk(torch.int64),
            lnk(torch.int64), lnk(torch.int32, nl2)]
    if series is not None:
        series._check(n_links, dev)
        cost, outs[4] = series.device_cost(cost), series.device_busy(nl2)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize(dev)
    check(ctx.handle, load().sg_link_queue(
        ctx.handle, _capi.SG_ROUTE_OUT_DEVICE | (_capi.SG_LINK_QUEUE_CARRY if carry else 0) |
        (_capi.SG_LINK_QUEUE_DROP if drop else 0) | (0 if base is None else _capi.SG_LINK_QUEUE_PACKETS) |
        (0 if series is None else _capi.SG_LINK_QUEUE_SERIES),
        n_links, ptr(off), n_records,
        ptr(enter), None if weight is None and not carry and base is None else ptr(packet), ptr(weight),
        (n_packets if carry or base is not None else 0) if weight is None else weight.numel(), ptr(cost),
        ptr(free), *[ptr(t) for t in outs]))
    lens = [n_records + n_tail] * 3 + [n_links, nl2, n_links, n_links, nl2]
    dts = [np.uint64, np.uint64, np.uint32, np.uint64, np.uint64, np.uint64, np.uint64, np.uint32]
    res = LinkQueueResult(*[t[:max(k, 1)].cpu().numpy().view(dt)[:k] for t, dt, k in zip(outs, dts, lens)])
    h_off = off.cpu().numpy().view(np.uint64)
    tails = None
    if base is not None:
        tails = _outcomes(h_off, res.wait_ns[n_records:], res.done_ns[n_records:], res.ahead[n_records:],
                          outs[1][n_records:n_records + n_tail])
        res = res._replace(wait_ns=res.wait_ns[:n_records], done_ns=res.done_ns[:n_records], ahead=res.ahead[:n_records])
    if drop:
        queue = _dropped(ctx, res, n_links, h_off,
                         None if weight is None and not carry else packet[:n_records].cpu().numpy().view(np.uint32),
                         None if weight is None else weight.cpu().numpy().view(np.uint32), h_cost, carry)
    elif carry:
        queue = _carried(ctx, res, h_off, packet[:n_records].cpu().numpy().view(np.uint32),
                         None if weight is None else weight.cpu().numpy().view(np.uint32), h_cost)
    else:
        queue = res
    return queue if tails is None else (queue, tails)


def _ahead_again(link_off, enter, packet, done, served, present):
    """sg_link_queue's ahead of every present (served or dropped) record from a carried result on
    host arrays: the served records before it in its link's (carried enter, packet) order whose
    done is past its enter time.  A link's done times never fall along that order."""
    off = np.asarray(link_off).astype(np.int64)
    ahead = np.zeros(len(enter), np.uint32)
    for lk in np.flatnonzero(np.diff(off) > 0):
        idx = np.arange(off[lk], off[lk + 1])
        idx = idx[present[idx]]
        order = idx[np.lexsort((packet[idx], enter[idx]))]
        srv = served[order]
        before = np.cumsum(srv) - srv
        gone = np.minimum(np.searchsorted(done[order][srv], enter[order], side="right"), before)
        ahead[order] = (before - gone).astype(np.uint32)
    return ahead


def _step_windows(s, off, n: int, enter, packet, weight, base, window_ns: int, settled, max_calls=None) -> int:
    """One device trace through the session s window by window: the whole trace goes in with the
    first call, at the horizon (first enter time) + window_ns; every later call only steps the
    horizon by window_ns, from the earliest pending record where that lies past the last horizon.
    settled(SettledPackets, SettledRecords) takes every call's results.  Returns the calls made
    (max_calls: stop there, with records still pending)."""
    import torch

    sign = torch.tensor(-2**63, dtype=torch.int64, device=s.dev)
    umin = lambda t: int((t ^ sign).min() ^ sign) & _UMAX  # noqa: E731
    H = min(umin(enter[:n]) + window_ns, _UMAX) if n else _UMAX
    calls = 0
    while True:
        settled(*(s.advance(off, enter[:n], packet[:n], weight, base, H) if not calls else s.advance(None, None, None, None, None, H)))
        calls += 1
        if not s.pending or H == _UMAX or calls == max_calls:
            return calls
        H = min(max(H, umin(s._rec["enter"])) + window_ns, _UMAX)


def _link_queue_windows(ctx: "Context", dev, n_links: int, off, n: int, enter, packet, weight, cost_ps, free_ns, n_packets: int,
                        limit_ns, base, window_ns: int, series=None):
    """A device trace solved window by window through a LinkQueueSession (PathTree.link_queue_round,
    window_ns): _link_queue_tensors' result with carry."""
    import torch

    from .queue_session import LinkQueueSession

    s = LinkQueueSession(ctx, cost_ps, limit_ns, free_ns, n_links=n_links, device=dev, series=series)
    wait, done = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    delay, arrive, where = np.zeros(n_packets, np.uint64), np.zeros(n_packets, np.uint64), np.zeros(n_packets, np.uint32)
    arrive_dev = torch.zeros(n_packets, dtype=torch.int64, device=dev)
    ones = torch.ones(n_packets, dtype=torch.int32, device=dev) if weight is None else weight.reshape(-1)[:n_packets]
    zero = torch.zeros(n_packets, dtype=torch.int64, device=dev) if base is None else base

    def settled(pk, rc):
        wait[rc.record], done[rc.record] = rc.wait_ns, rc.done_ns
        delay[pk.packet], arrive[pk.packet], where[pk.packet] = pk.delay_ns, pk.arrive_ns, pk.where
        arrive_dev[torch.from_numpy(pk.packet).to(dev)] = pk.arrive_dev

    _step_windows(s, off, n, enter, packet, ones, zero, window_ns, settled)
    h_off = off.cpu().numpy().view(np.uint64)
    h_pkt = packet[:n].cpu().numpy().view(np.uint32)
    h_wt = None if weight is None else weight.cpu().numpy().view(np.uint32)
    h_cost = _per_link_u64(cost_ps, n_links, "cost_ps")
    sums = s.link_sums
    out = wait == np.uint64(_UMAX)
    present = ~(out & (done == np.uint64(_UMAX)))
    srv = ~out
    e = done.copy()  # (the carried enter time: a dropped record's done is its own)
    if srv.any():
        e[srv] = done[srv] - _service_ns(h_off, n, h_pkt, h_wt, h_cost)[srv] - wait[srv]
    ahead = _ahead_again(h_off, e, h_pkt, done, srv, present)
    amax = np.zeros(n_links, np.uint32)
    if srv.any():
        link = np.repeat(np.arange(n_links), np.diff(h_off.astype(np.int64)))
        np.maximum.at(amax, link[srv], ahead[srv])
    drop = limit_ns is not None
    res = LinkQueueResult(wait, done, ahead, s.link_free.copy(),
                          np.concatenate([sums["busy_ns"], sums["refused_ns"]]) if drop else sums["busy_ns"],
                          sums["wait_max_ns"], sums["wait_sum_ns"],
                          np.concatenate([amax, sums["drops"].astype(np.uint32)]) if drop else amax)
    queue = _dropped(ctx, res, n_links, h_off, h_pkt, h_wt, h_cost, True) if drop else _carried(ctx, res, h_off, h_pkt, h_wt, h_cost)
    queue = queue._replace(iterations=s.iterations)
    return queue if base is None else (queue, _outcomes(h_off, delay, arrive, where, arrive_dev))


def _base_times(x, n_packets: int, dev, what: str = "outcomes"):
    """One base time per packet as an int64 tensor on `dev`: a Deliveries (its deliver_time_ns), or
    a u64 array or tensor."""
    return int_tensor(x, np.uint64, n_packets, dev, what, "deliver_time_ns")[:n_packets]
