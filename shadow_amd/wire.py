"""Packets in flight, on the device: host-side mirror of the per-host EventQueue
between WorkerShared::push_packet_to_host (src/main/core/worker.rs:597-607) and
Host::execute's pops (src/main/host/host.rs:753-757), restricted to Packet events.

`PacketWire.push` takes a delivery round's output (`deliver_round`), `pop` returns
the arrivals of a window grouped by host in EventQueue order (time, src_host,
event_id; core/work/event.rs:84-155) as device tensors, ready for
`InboundPipeline.run_ordered`.  Nothing crosses the bus while a packet waits.
On the sharded path (shadow_amd.dist) the source rank stamps its records (`stamp_records`)
and the owner rank pushes what it received (`PacketWire.push_records`).
Every computation is a HIP kernel in libshadow_gpu.so (csrc/sg_wire.hip).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _capi
from ._capi import check, load
from .graph import Context, default_context

# The sort tiers' limits (csrc/sg_wire.hip WR_RANK_SORT_MAX / WR_LDS_SORT_MAX): a host's due
# segment up to RANK_SORT_MAX events is rank-sorted in a wave, up to LDS_SORT_MAX sorted in one
# workgroup's LDS, beyond that cut into such pieces and merged.  tests/test_wire_cpu.py keeps
# them equal to the kernel's.
RANK_SORT_MAX = 64
LDS_SORT_MAX = 2048
NEVER = 2**64 - 1  # next_time_ns of an empty wire (UINT64_MAX)

_STATE_KEYS = ("host", "src_host", "packet", "len", "time_ns", "event_id")
_STATE_TYPES = (np.uint32, np.uint32, np.uint32, np.uint32, np.uint64, np.uint64)


def stamp_records(send, n_records: int, length, n_packets: int, packet_id=None, id_base: int = 0,
                  ctx: Optional[Context] = None) -> None:
    """On the source rank, after the source phase: write len and the packet id into the first
    n_records records of `send` (int64 device tensor [n, 4]), in place: they become
    dist.WIRE_RECORD_DTYPE records.  length / packet_id: int32 device tensors over the rank's
    n_packets packets (packet_id None: id_base + the packet's index).  Once per round: stamped
    records must not be bucketed (sg_deliver_bucket) or stamped again.  Asynchronous."""
    ctx = ctx or default_context()
    n = int(n_records)
    check(ctx.handle, load().sg_wire_stamp_records(
        ctx.handle, send.data_ptr() if n else None, n, packet_id.data_ptr() if packet_id is not None else None,
        int(id_base), length.data_ptr(), int(n_packets)))


def stamp_records_padded(send_padded, send, n_ranks: int, cap: int, xrow, length, n_packets: int, packet_id=None,
                         id_base: int = 0, ctx: Optional[Context] = None) -> None:
    """The same after a padded source phase (dist.SourcePadded's send_padded, send, cap, xrow): the
    valid slots of every block and the records past cap in `send`, counts read on the device."""
    ctx = ctx or default_context()
    check(ctx.handle, load().sg_wire_stamp_records_padded(
        ctx.handle, send_padded.data_ptr(), send.data_ptr(), int(n_ranks), int(cap), xrow.data_ptr(),
        packet_id.data_ptr() if packet_id is not None else None, int(id_base), length.data_ptr(), int(n_packets)))


class PacketWire:
    """Every host's in-flight Packet events (sg_wire_*).  capacity: events it may hold;
    bin_ns / n_bins: the calendar's geometry, which affects speed only."""

    def __init__(self, n_hosts: int, capacity: int, bin_ns: int, n_bins: int, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.n = int(n_hosts)
        self.capacity = int(capacity)
        h = C.c_void_p()
        check(self.ctx.handle, load().sg_wire_create(self.ctx.handle, self.n, self.capacity, int(bin_ns), int(n_bins),
                                                     C.byref(h)))
        self.handle = h
        self._out = None

    @property
    def count(self) -> int:
        """Events held as the host knows it (exact after pop / get_state / set_state; a push adds
        its whole batch, dropped packets included)."""
        return int(load().sg_wire_count(self.handle))

    def push(self, packets, out, length, packet_id=None, id_base: int = 0, deliver_time_ns=None) -> None:
        """One event per delivered packet of the round (`packets`: PacketBatch, `out`: its
        Deliveries).  length: int32 device tensor, PacketRc::len() per packet; packet_id: int32
        device tensor or None (then id_base + the packet's index).  deliver_time_ns: an int64
        device tensor of n_packets that replaces out.deliver_time_ns, e.g. the arrive_dev of a
        round under link rates (graph.PacketOutcomes); a packet whose time is 2^64 - 1 adds no
        event.  Asynchronous: the tensor must stay alive until the stream has run the push."""
        d = out.c_struct()
        if deliver_time_ns is not None:
            if deliver_time_ns.element_size() != 8 or deliver_time_ns.numel() < len(packets) or \
                    not deliver_time_ns.is_contiguous():
                raise ValueError(f"deliver_time_ns: a contiguous int64 device tensor of {len(packets)} entries")
            d = type(d)()  # (out's own struct is cached: a copy carries the other times)
            C.memmove(C.byref(d), C.byref(out.c_struct()), C.sizeof(d))
            d.deliver_time_ns = deliver_time_ns.data_ptr()
        check(self.ctx.handle, load().sg_wire_push(
            self.ctx.handle, self.handle, C.byref(packets.c_struct()), C.byref(d),
            packet_id.data_ptr() if packet_id is not None else None, int(id_base), length.data_ptr()))

    def push_records(self, recv, n_records: int, host_map=None) -> None:
        """The owner rank's push on the sharded path: one event per stamped record (see
        stamp_records) of `recv`, an int64 device tensor [n, 4] as the exchange delivers it.
        host_map: int32 device tensor over all hosts or None; the event's host is
        host_map[dst_host] (e.g. the partition's `local` for a wire over the rank's own hosts),
        else dst_host.  A destination outside the map or the wire is reported by the next pop
        (SG_ERR_INVALID_ARG).  Asynchronous."""
        n = int(n_records)
        check(self.ctx.handle, load().sg_wire_push_records(
            self.ctx.handle, self.handle, recv.data_ptr() if n else None, n,
            host_map.data_ptr() if host_map is not None else None,
            int(host_map.numel()) if host_map is not None else self.n))

    def push_records_padded(self, recv_padded, n_ranks: int, cap: int, xall, rank: int, host_map=None) -> None:
        """The same for the blocks of a fixed-split exchange ([n_ranks * cap, 4]; xall: the gathered
        [stats, counts] rows, on the device).  Appends nothing when a count in xall exceeds cap:
        the round is then exchanged again exactly and pushed with push_records.  `count` rises by
        n_ranks * cap until the next pop.  Asynchronous."""
        check(self.ctx.handle, load().sg_wire_push_records_padded(
            self.ctx.handle, self.handle, recv_padded.data_ptr(), int(n_ranks), int(cap), xall.data_ptr(), int(rank),
            host_map.data_ptr() if host_map is not None else None,
            int(host_map.numel()) if host_map is not None else self.n))

    def _buffers(self, cap: int):
        import torch

        if self._out is None or self._out["host"].numel() < cap:
            i32 = dict(dtype=torch.int32, device="cuda")
            i64 = dict(dtype=torch.int64, device="cuda")
            self._out = dict(host=torch.empty(cap, **i32), time_ns=torch.empty(cap, **i64),
                             packet=torch.empty(cap, **i32), len=torch.empty(cap, **i32),
                             src_host=torch.empty(cap, **i32), event_id=torch.empty(cap, **i64))
        return self._out

    def pop(self, window_end_ns: int, cap: Optional[int] = None) -> dict:
        """Every event with time < window_end_ns, removed: dict(n, next_time_ns, host, time_ns,
        packet, len, src_host, event_id), device tensors sliced to n (views of buffers the next
        pop reuses), grouped by ascending host, each host's in EventQueue order.  cap: the output
        capacity (default: the events held); with more due, ShadowGpuError(SG_ERR_CAPACITY)
        whose `needed` is their number, and the wire is unchanged.  After a padded sharded round
        (ShardedDelivery.round(wire=...)) the pop is the round's synchronisation and also raises
        that round's source-phase error (e.g. SG_ERR_UNSORTED for a batch not grouped by source
        host: nothing of it was delivered), once; the pop is then complete all the same, and the
        exception's `arrivals` holds what it returned."""
        cap = max(int(self.count if cap is None else cap), 0)
        b = self._buffers(max(cap, 1))
        o = _capi.sg_wire_arrivals(cap, *(b[k].data_ptr() for k in ("host", "time_ns", "packet", "len", "src_host",
                                                                    "event_id")))
        n, nxt = C.c_uint32(), C.c_uint64(NEVER)
        rc = load().sg_wire_pop(self.ctx.handle, self.handle, int(window_end_ns), C.byref(o), C.byref(n),
                                C.byref(nxt))
        k = int(n.value)
        res = dict(n=k, next_time_ns=int(nxt.value))
        res.update({key: b[key][:k] for key in ("host", "time_ns", "packet", "len", "src_host", "event_id")})
        try:
            check(self.ctx.handle, rc)
        except _capi.ShadowGpuError as e:
            e.needed = k
            # a source-phase error of the sharded round reported by this pop: the pop itself is
            # complete, and these are its arrivals (they have left the wire)
            e.arrivals = res if rc != _capi.SG_ERR_CAPACITY else None
            raise
        return res

    @staticmethod
    def _struct(st) -> _capi.sg_wire_state:
        return _capi.sg_wire_state(*(st[k].ctypes.data_as(C.c_void_p) for k in _STATE_KEYS))

    def get_state(self) -> dict:
        """All events in canonical order (host, time_ns, src_host, event_id): numpy arrays
        host, src_host, packet, len (uint32), time_ns, event_id (uint64)."""
        cap = max(self.count, 1)
        while True:
            st = {k: np.zeros(cap, t) for k, t in zip(_STATE_KEYS, _STATE_TYPES)}
            n = C.c_uint64()
            rc = load().sg_wire_get_state(self.handle, cap, C.byref(self._struct(st)), C.byref(n))
            if rc == _capi.SG_ERR_CAPACITY and n.value > cap:
                cap = int(n.value)
                continue
            check(self.ctx.handle, rc)
            return {k: v[:n.value] for k, v in st.items()}

    def set_state(self, st: dict) -> None:
        """Replace the contents with the events of `st` (get_state's keys), in any order."""
        a = {k: np.ascontiguousarray(st[k], dtype=t) for k, t in zip(_STATE_KEYS, _STATE_TYPES)}
        n = len(a["host"])
        assert all(len(v) == n for v in a.values())
        check(self.ctx.handle, load().sg_wire_set_state(self.handle, n, C.byref(self._struct(a))))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                load().sg_wire_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
