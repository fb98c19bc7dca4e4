"""Link queues across rounds: a session settles every round up to its end and feeds what is still
in flight into the next one (sg_link_queue with SG_LINK_QUEUE_WINDOW).  The state
between the rounds lives here, in device tensors; the library keeps none."""
import ctypes as C
import time
from typing import NamedTuple

import numpy as np

from . import _capi
from ._capi import check, load
from .link_queue import _base_times, _per_link_u64
from .round_args import int_tensor

_UMAX = 0xFFFFFFFFFFFFFFFF
_IN_FLIGHT = 0xFFFFFFFD


class SettledPackets(NamedTuple):
    """The packets a LinkQueueSession.advance settled, in (round, packet) order: the round that
    brought the packet and its number there; delay_ns (u64), what the queues added, against the
    packet's original base time; arrive_ns (u64, 2^64 - 1: dropped); drop_link (u32, 2^32 - 1: not
    dropped); lost (bool); arrive_dev, arrive_ns as an int64 device tensor; where (u32), as
    PacketOutcomes has it: the record that dropped the packet, its index in the trace of the
    packet's round, else WHERE_ARRIVED or WHERE_NOTHING."""
    round: np.ndarray
    packet: np.ndarray
    delay_ns: np.ndarray
    arrive_ns: np.ndarray
    drop_link: np.ndarray
    lost: np.ndarray
    arrive_dev: object
    where: np.ndarray


class SettledRecords(NamedTuple):
    """The records a LinkQueueSession.advance settled: the round that brought the record and its
    index in that round's trace; wait_ns and done_ns (u64) with sg_link_queue's sentinels: served;
    dropped (wait 2^64 - 1, done the carried enter time); absent (both 2^64 - 1)."""
    round: np.ndarray
    record: np.ndarray
    wait_ns: np.ndarray
    done_ns: np.ndarray


def _u64(x) -> int:
    return int(x) & _UMAX


class LinkQueueSession:
    """Rounds that queue behind one another.  graph_or_ctx: a NetworkGraph (its links and context) or
    a Context with n_links given; cost_ps, limit_ns, free_ns as in shadow_amd.link_queue (limit_ns:
    finite buffers, SG_LINK_QUEUE_DROP in every call).

    Kept on the device: the pending records grouped by link (re-based enter time, in-flight packet
    slot, origin round and record), the in-flight packets (weight, re-based base, original base,
    origin round and packet), the links' free times, the running per-link sums and the last
    horizon.  advance() merges the pending records with a round's trace link by link -- both are
    grouped by link already: offsets and a scatter, no sort -- and runs one call with
    SG_LINK_QUEUE_CARRY | SG_LINK_QUEUE_WINDOW | SG_LINK_QUEUE_PACKETS.  In-flight packets are numbered before the
    round's and keep their order, so (round, packet) order is the packet numbering of every call:
    a sequence of rounds followed by flush() equals one carried call over the concatenated trace.
    `ahead` is not kept: a call counts only its own settled records (include/shadow_gpu.h).
    series: a LinkQueueSeries over the same links (SG_LINK_QUEUE_SERIES in every call): every advance() adds
    the records it settles into the series' matrix, so the rounds and flush() sum to the matrix of the
    one carried call."""

    def __init__(self, graph_or_ctx, cost_ps, limit_ns=None, free_ns=None, *, n_links=None, device="cuda", series=None):
        import torch

        self.ctx = getattr(graph_or_ctx, "ctx", graph_or_ctx)
        self.n_links = int(len(graph_or_ctx.links()[0]) if hasattr(graph_or_ctx, "links") else n_links)
        nl, self.dev = self.n_links, torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(self.dev)  # noqa: E731
        cost = _per_link_u64(cost_ps, nl, "cost_ps")
        self.drop = limit_ns is not None
        self._cost = up(np.concatenate([cost, _per_link_u64(limit_ns, nl, "limit_ns")]) if self.drop else cost)
        self.series = series
        if series is not None:
            series._check(nl, self.dev)
            self._cost = series.device_cost(self._cost)  # (the header and the slot map behind the costs)
        # (the horizon rides behind the links' free times)
        self._free = up(np.concatenate([np.zeros(nl, np.uint64) if free_ns is None else _per_link_u64(free_ns, nl, "free_ns"),
                                        np.zeros(1, np.uint64)]))
        z = lambda dt=torch.int64: torch.zeros(0, dtype=dt, device=self.dev)  # noqa: E731
        self._rec = dict(link=z(), enter=z(), slot=z(), round=z(), record=z())
        self._pkt = dict(weight=z(torch.int32), base=z(), base0=z(), round=z(), packet=z())
        self._sums = dict(busy=torch.zeros(nl, dtype=torch.int64, device=self.dev), wait_sum=torch.zeros(nl, dtype=torch.int64, device=self.dev),
                          wait_max=torch.zeros(nl, dtype=torch.int64, device=self.dev), drops=torch.zeros(nl, dtype=torch.int64, device=self.dev),
                          refused=torch.zeros(nl, dtype=torch.int64, device=self.dev))
        self.last_horizon, self.rounds, self.iterations, self.active = 0, 0, 0, 0
        # on_host: advance() hands its results out as host arrays (False: as device tensors, the u64 fields
        # as int64 views); profile: a dict that takes the last advance()'s wall ms for "merge", "solve" and
        # "keep", each ended by a device synchronisation (None: not measured)
        self.on_host, self.profile = True, None

    # ---- what the session holds
    @property
    def in_flight(self) -> int:
        return int(self._pkt["base"].numel())

    @property
    def pending(self) -> int:
        return int(self._rec["enter"].numel())

    @property
    def link_free(self) -> np.ndarray:
        return self._free[:self.n_links].cpu().numpy().view(np.uint64)

    @property
    def link_sums(self) -> dict:
        """busy_ns, wait_sum_ns, refused_ns and drops (they add) and wait_max_ns (the maximum) per
        link, over every record settled so far."""
        return {k + ("" if k == "drops" else "_ns"): v.cpu().numpy().view(np.uint64) for k, v in self._sums.items()}

    def _tensor(self, x, np_dtype, t_dtype, count, what):
        import torch

        if x is None:
            if count:
                raise ValueError(f"{what}: {count} entries")
            return torch.zeros(0, dtype=t_dtype, device=self.dev)
        return int_tensor(x, np_dtype, count, self.dev, what)[:count]

    def advance(self, link_off, enter, packet, weight, base, horizon_ns):
        """One round: its trace (link_off: n_links + 1 u64 offsets; enter u64 and packet u32 per
        record, grouped by link), weight (u32) and base (u64: the arrival without the rates) per
        packet of the round -- host arrays or device tensors, all None for a round without
        records -- settled up to horizon_ns.  The horizon never goes back, and no new record
        enters before the last one.  Returns (SettledPackets, SettledRecords)."""
        import torch

        H = int(horizon_ns)
        if not self.last_horizon <= H <= _UMAX:
            raise ValueError(f"horizon_ns: a u64 time, not before the last horizon {self.last_horizon}")
        nl, dev, i64 = self.n_links, self.dev, torch.int64
        sign = torch.tensor(-2**63, dtype=i64, device=dev)  # (x ^ sign orders int64 views as u64)
        if link_off is None:
            off = torch.zeros(nl + 1, dtype=i64, device=dev)
        else:
            off = self._tensor(link_off, np.uint64, i64, nl + 1, "link_off")
        n_new = int(off[nl]) if link_off is not None else 0
        P_new = 0 if base is None else int(base.numel() if isinstance(base, torch.Tensor) else np.size(base))
        t_new = self._tensor(enter, np.uint64, i64, n_new, "enter")
        p_new = self._tensor(packet, np.uint32, torch.int32, n_new, "packet").to(i64) & 0xFFFFFFFF
        w_new = self._tensor(weight, np.uint32, torch.int32, P_new, "weight")
        b_new = self._tensor(base, np.uint64, i64, P_new, "base")
        if n_new:
            if _u64((t_new ^ sign).min() ^ sign) < self.last_horizon:
                raise ValueError(f"enter: a record enters before the last horizon {self.last_horizon}")
            if int(p_new.max()) >= P_new:
                raise ValueError(f"packet: numbers below {P_new}, the round's packets")
        rec, pkt, rnd = self._rec, self._pkt, self.rounds
        F, n_old = self.in_flight, self.pending
        clock = [time.perf_counter()]

        def lap(name):
            if self.profile is not None:
                torch.cuda.synchronize(dev)
                clock.append(time.perf_counter())
                self.profile[name] = (clock[-1] - clock[-2]) * 1e3

        n, P = n_old + n_new, F + P_new

        # ---- the merge, link by link: a link's pending records, then the round's
        old_cnt = torch.bincount(rec["link"], minlength=nl) if n_old else torch.zeros(nl, dtype=i64, device=dev)
        new_cnt = off[1:] - off[:-1]
        m_off = torch.zeros(nl + 1, dtype=i64, device=dev)
        m_off[1:] = torch.cumsum(old_cnt + new_cnt, 0)
        old_off = torch.cumsum(old_cnt, 0) - old_cnt
        new_link = torch.repeat_interleave(torch.arange(nl, device=dev), new_cnt, output_size=n_new) if n_new else \
            torch.zeros(0, dtype=i64, device=dev)
        at_old = m_off[rec["link"]] + (torch.arange(n_old, device=dev) - old_off[rec["link"]])
        at_new = m_off[new_link] + old_cnt[new_link] + (torch.arange(n_new, device=dev) - off[new_link])
        room = lambda k, dt=i64: torch.zeros(max(k, 1), dtype=dt, device=dev)  # noqa: E731
        m_enter, m_packet, m_link = room(n + P), room(n, torch.int32), room(n)
        m_round, m_record = room(n), room(n)
        for at, lk, t, p, r, i in ((at_old, rec["link"], rec["enter"], rec["slot"], rec["round"], rec["record"]),
                                   (at_new, new_link, t_new, p_new + F, torch.full((n_new,), rnd, dtype=i64, device=dev),
                                    torch.arange(n_new, device=dev))):
            m_enter[at], m_packet[at], m_link[at], m_round[at], m_record[at] = t, p.to(torch.int32), lk, r, i
        m_weight = torch.cat([pkt["weight"], w_new]).contiguous()
        m_base = torch.cat([pkt["base"], b_new])
        m_base0 = torch.cat([pkt["base0"], b_new])
        m_pround = torch.cat([pkt["round"], torch.full((P_new,), rnd, dtype=i64, device=dev)])
        m_ppacket = torch.cat([pkt["packet"], torch.arange(P_new, device=dev)])
        m_enter[n:n + P] = m_base

        # ---- the call
        nl2 = 2 * nl if self.drop else nl
        wait, done, ahead = room(n + P), room(n + P), room(n + P, torch.int32)
        free_out, busy, wmax, wsum, amax = room(nl), room(nl2), room(nl), room(nl), room(nl2, torch.int32)
        if self.series is not None:
            busy = self.series.device_busy(nl2)  # (the per-link values in front of the matrix the call adds into)
        self._free[nl] = torch.tensor(H - (1 << 64) if H >= 1 << 63 else H, dtype=i64)
        if not m_weight.numel():
            m_weight = room(0, torch.int32)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        torch.cuda.synchronize(dev)
        lap("merge")
        flags = _capi.SG_ROUTE_OUT_DEVICE | _capi.SG_LINK_QUEUE_CARRY | _capi.SG_LINK_QUEUE_WINDOW | _capi.SG_LINK_QUEUE_PACKETS | \
            (_capi.SG_LINK_QUEUE_DROP if self.drop else 0) | (0 if self.series is None else _capi.SG_LINK_QUEUE_SERIES)
        check(self.ctx.handle, load().sg_link_queue(
            self.ctx.handle, flags, nl, ptr(m_off), n, ptr(m_enter), ptr(m_packet), ptr(m_weight), P, ptr(self._cost),
            ptr(self._free), ptr(wait), ptr(done), ptr(ahead), ptr(free_out), ptr(busy), ptr(wmax), ptr(wsum), ptr(amax)))
        if n:
            self.iterations += int(self.ctx.read_timer("link_queue_iters")[1])
            self.active += int(self.ctx.read_timer("link_queue_active")[1])
        lap("solve")

        # ---- keep what is pending and in flight, with stable masks; hand out the rest
        pend = (wait[:n] == -1) & (ahead[:n] == -1)
        where = ahead[n:n + P].to(i64) & 0xFFFFFFFF
        flying = where == _IN_FLIGHT
        slot = torch.cumsum(flying.to(i64), 0) - 1
        lost = where < _IN_FLIGHT
        drop_link = torch.full((P,), 0xFFFFFFFF, dtype=i64, device=dev)
        drop_link[lost] = m_link[where[lost]]
        origin = where.clone()  # (a record of the call -> its index in its round's trace)
        origin[lost] = m_record[where[lost]]
        out_p = ~flying
        delay = wait[n:n + P] + (m_base - m_base0)  # (against the original base; int64 wraps as u64 does)
        arrive = done[n:n + P]
        if self.on_host:
            host = lambda t, dt: t.cpu().numpy().view(dt) if dt != np.bool_ else t.cpu().numpy()  # noqa: E731
        else:
            host = lambda t, dt: t  # noqa: E731
        packets = SettledPackets(host(m_pround[out_p], np.int64), host(m_ppacket[out_p], np.int64), host(delay[out_p], np.uint64),
                                 host(arrive[out_p], np.uint64), self._u32(host(drop_link[out_p], np.int64)),
                                 host(lost[out_p], np.bool_), arrive[out_p], self._u32(host(origin[out_p], np.int64)))
        out_r = ~pend
        records = SettledRecords(host(m_round[:n][out_r], np.int64), host(m_record[:n][out_r], np.int64),
                                 host(wait[:n][out_r], np.uint64), host(done[:n][out_r], np.uint64))
        self._rec = dict(link=m_link[:n][pend], enter=done[:n][pend], slot=slot[m_packet[:n][pend].to(i64)],
                         round=m_round[:n][pend], record=m_record[:n][pend])
        self._pkt = dict(weight=m_weight[:P][flying], base=arrive[flying], base0=m_base0[flying], round=m_pround[flying],
                         packet=m_ppacket[flying])
        self._free[:nl] = free_out[:nl]
        s = self._sums
        s["busy"] += busy[:nl]
        s["wait_sum"] += wsum[:nl]
        s["wait_max"] = torch.where((wmax[:nl] ^ sign) > (s["wait_max"] ^ sign), wmax[:nl], s["wait_max"])
        if self.drop:
            s["drops"] += amax[nl:2 * nl].to(i64) & 0xFFFFFFFF
            s["refused"] += busy[nl:2 * nl]
        self.last_horizon, self.rounds = H, rnd + 1
        lap("keep")
        return packets, records

    @staticmethod
    def _u32(x):
        return x.astype(np.uint32) if isinstance(x, np.ndarray) else x

    def round(self, tree, hosts, packets, deliveries, horizon_ns, weight="payload", watch=None):
        """A delivery round: its link trace (PathTree.link_trace_device: the trace stays on the
        device), then advance(); the records' indices are the trace's.  deliveries: the round's Deliveries (status and the base times),
        weight and watch as in PathTree.link_queue_round."""
        off, n, enter, pkt, weight = tree.link_trace_device(hosts, packets, deliveries, weight, watch)[:5]
        base = _base_times(deliveries, len(packets), self.dev)
        if weight is None:
            import torch

            weight = torch.ones(len(packets), dtype=torch.int32, device=self.dev)
        return self.advance(off, enter[:n], pkt[:n], weight.reshape(-1)[:len(packets)], base, horizon_ns)

    def flush(self):
        """Settle everything still in flight: advance() at 2^64 - 1 with no records."""
        return self.advance(None, None, None, None, None, _UMAX)
