"""Host-side mirror of Shadow's network-graph interface over the HIP core.

Names, argument meaning and errors follow src/main/network/graph/mod.rs and
src/main/core/sim_config.rs so that a test written against the reference reads
the same here:

    graph = NetworkGraph.parse(gml_text)                       # graph/mod.rs:134
    n0 = graph.node_id_to_index(0)                             # graph/mod.rs:126
    paths = graph.compute_shortest_paths([n0, n1, n2])         # graph/mod.rs:183
    paths[(n0, n1)].latency_ns
    routing = generate_routing_info(graph, {0, 1, 2}, True)    # sim_config.rs:411
    routing.path(0, 1)                                         # graph/mod.rs:448

All computation runs in libshadow_gpu.so on the GPU; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from ._capi import ShadowGpuError, check, load
from .link_queue import (WHERE_ARRIVED, WHERE_IN_FLIGHT, WHERE_NOTHING, LinkQueueCarried, LinkQueueCarriedDropped,  # noqa: F401
                         LinkQueueDropped, LinkQueueResult, PacketOutcomes, cost_ps_from_bandwidth, link_queue,
                         link_queue_pending, queue_limit_ns, series_slots)
from .link_queue import _UMAX, _base_times, _exit_carried, _link_queue_tensors, _link_queue_windows, _per_link_u64
from .round_args import int_tensor, series_out, watch_mask, weight_arg, with_capacity


def _vp(x):
    """A device address for the library: 0 is NULL."""
    return C.c_void_p(x or None)


def _dev_ptr(t):
    """A tensor's address for the library: None is NULL."""
    return None if t is None else C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------
# Context
# ---------------------------------------------------------------------------
class Context:
    """One GPU (HIP device) + stream + workspace (sg_ctx)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        L = load()
        h = C.c_void_p()
        rc = L.sg_ctx_create(int(device), C.byref(h))
        if rc != _capi.SG_OK:
            why = (L.sg_ctx_last_error(None) or b"").decode(errors="replace")
            raise ShadowGpuError(rc, f"sg_ctx_create(device={device}) failed with status {rc}: {why}")
        self.handle = h
        self.device = int(device)
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream: Optional[int]) -> None:
        """Launch on `stream` (a hipStream_t as int, e.g. torch's cuda_stream); None = own stream."""
        check(self.handle, load().sg_ctx_set_stream(self.handle, C.c_void_p(stream or 0)))

    @property
    def stream(self) -> int:
        return load().sg_ctx_stream(self.handle) or 0

    def synchronize(self) -> None:
        check(self.handle, load().sg_ctx_synchronize(self.handle))

    def set_packet_counters(self, counts=None) -> None:
        """RoutingInfo::increment_packet_count on the device (sg_ctx_set_packet_counters): a
        zeroed int64 device tensor with a cell per routing-table cell; every delivered packet of
        this context's later rounds adds one at its path's cell.  None turns counting off."""
        if counts is None:
            check(self.handle, load().sg_ctx_set_packet_counters(self.handle, None, 0))
            return
        if counts.dtype.itemsize != 8 or not counts.is_cuda or not counts.is_contiguous():
            raise ValueError("packet counters: a contiguous 8-byte device tensor")
        self._packet_counts = counts  # kept alive while the library holds the pointer
        check(self.handle, load().sg_ctx_set_packet_counters(self.handle, counts.data_ptr(), counts.numel()))

    def enable_timers(self, enable: bool = True, count_work: bool = False) -> None:
        """Per-kernel HIP-event timers on this context's stream (resets them).

        count_work: run the counting variants of data-dependent kernels (the
        relaxation kernel's lane-relaxation count); time them in a separate run.
        """
        mode = (1 | (2 if count_work else 0)) if enable else 0
        check(self.handle, load().sg_ctx_enable_timers(self.handle, mode))

    def read_timer(self, kernel: str):
        """(total device ms, launches, declared algorithmic work) for one kernel."""
        t, n, w = C.c_double(), C.c_uint64(), C.c_double()
        check(self.handle, load().sg_ctx_read_timer(self.handle, kernel.encode(), C.byref(t), C.byref(n), C.byref(w)))
        return t.value, n.value, w.value

    def close(self) -> None:
        if getattr(self, "handle", None):
            load().sg_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: Dict[int, Context] = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


# ---------------------------------------------------------------------------
# PathProperties (graph/mod.rs:297-340)
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class PathProperties:
    latency_ns: int
    packet_loss: np.float32

    def _key(self):
        return (self.latency_ns, float(self.packet_loss))

    # graph/mod.rs:305-320: latency first, then packet loss
    def __lt__(self, other):
        return self._key() < other._key()

    def __le__(self, other):
        return self._key() <= other._key()

    def __eq__(self, other):
        return isinstance(other, PathProperties) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    # graph/mod.rs:322-331 (f32 ops, one rounding each)
    def __add__(self, other: "PathProperties") -> "PathProperties":
        one = np.float32(1.0)
        a, b = np.float32(self.packet_loss), np.float32(other.packet_loss)
        return PathProperties(self.latency_ns + other.latency_ns,
                              np.float32(one - np.float32(np.float32(one - a) * np.float32(one - b))))


DEFAULT_PATH = PathProperties(0, np.float32(0.0))


class PathTable:
    """Dense result of compute_shortest_paths / get_direct_paths.

    Behaves like the reference's HashMap<(NodeIndex, NodeIndex), PathProperties>
    (graph/mod.rs:186): keys are (src, dst) node indices from `nodes`; the
    arrays `latency_ns` (u64) and `packet_loss` (f32) are [n_used x n_used]
    with row = source in `nodes` order.
    """

    def __init__(self, nodes: Sequence[int], latency_ns: np.ndarray, packet_loss: np.ndarray):
        self.nodes = [int(x) for x in nodes]
        self.index = {n: i for i, n in enumerate(self.nodes)}
        self.latency_ns = latency_ns
        self.packet_loss = packet_loss

    def __len__(self) -> int:
        return len(self.nodes) ** 2

    def get(self, key: Tuple[int, int]) -> Optional[PathProperties]:
        i, j = self.index.get(key[0]), self.index.get(key[1])
        if i is None or j is None:
            return None
        return PathProperties(int(self.latency_ns[i, j]), np.float32(self.packet_loss[i, j]))

    def __getitem__(self, key: Tuple[int, int]) -> PathProperties:
        p = self.get(key)
        if p is None:
            raise KeyError(key)
        return p

    def __contains__(self, key) -> bool:
        return key[0] in self.index and key[1] in self.index

    def keys(self) -> Iterator[Tuple[int, int]]:
        for a in self.nodes:
            for b in self.nodes:
                yield (a, b)

    def items(self):
        for k in self.keys():
            yield k, self[k]


class PathTree:
    """Shortest-path trees beside their table rows (sg_routing_build_tree).

    `nodes` is a permutation of every graph node, the sources first; row i is source
    nodes[i], column j is node nodes[j].  `latency_ns` / `packet_loss` are the full-width
    rows [n_sources x n_nodes]; `pred` / `first_hop` hold petgraph node indices:
    pred[i, j] = the node before nodes[j] on the path from nodes[i] (the smallest index
    among the tight in-arcs), first_hop[i, j] = the node after nodes[i] on it.
    The f32 loss fold is not associative, so a path is expanded inside its source's pred
    row (`path`), never first hop by first hop across rows.
    """

    def __init__(self, graph: "NetworkGraph", nodes: np.ndarray, n_sources: int, latency_ns: np.ndarray,
                 packet_loss: np.ndarray, pred: np.ndarray, first_hop: np.ndarray):
        self._graph = graph
        self.nodes = nodes
        self.n_sources = int(n_sources)
        self.index = {int(v): j for j, v in enumerate(nodes)}
        self.latency_ns = latency_ns
        self.packet_loss = packet_loss
        self.pred = pred
        self.first_hop = first_hop

    def _row(self, src: int) -> int:
        i = self.index.get(int(src))
        if i is None or i >= self.n_sources:
            raise KeyError(f"node {src} is not a source of this tree")
        return i

    def _rows(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The pred, latency_ns and packet_loss rows as the library reads them (u32, u64, f32, contiguous)."""
        return (np.ascontiguousarray(self.pred, dtype=np.uint32), np.ascontiguousarray(self.latency_ns, dtype=np.uint64),
                np.ascontiguousarray(self.packet_loss, dtype=np.float32))

    def _call_prefix(self, pred: np.ndarray, hosts=None) -> tuple:
        """What every tree call on host rows starts with: the context, the net, the HostTable where the
        call takes a round's batch, the node order, all the source rows on the host, and `pred`."""
        g = self._graph
        return ((g.ctx.handle, g._ensure_net()) + (() if hosts is None else (hosts.handle,)) +
                (self.nodes.ctypes.data, len(self.nodes), 0, self.n_sources, 0, pred.ctypes.data))

    def _status_weight(self, packets, status, weight=None):
        """A round's status and weight as tensors (or None) on the packets' device."""
        npk, dev = len(packets), packets.src_host.device
        if status is not None:
            status = int_tensor(status, np.uint8, npk, dev, "status", "status")
        weight = weight_arg(weight, packets)
        return status, None if weight is None else int_tensor(weight, np.uint32, npk, dev, "weight")

    def path(self, src: int, dst: int) -> List[int]:
        """The node indices src ... dst of the tree path (sg_tree_path)."""
        row = np.ascontiguousarray(self.pred[self._row(src)])
        n = len(self.nodes)
        out = np.empty(n, np.uint32)
        ln = C.c_uint32()
        rc = load().sg_tree_path(row.ctypes.data, self.nodes.ctypes.data, n, int(src), int(dst), out.ctypes.data, n,
                                 C.byref(ln))
        if rc != _capi.SG_OK:
            raise ShadowGpuError(rc, f"sg_tree_path({src}, {dst}) failed with status {rc}")
        return out[:ln.value].tolist()

    def link_load(self, counts) -> Tuple[np.ndarray, np.ndarray]:
        """(link_load, node_load), both u64, of a host matrix counts[i, j] = what source nodes[i]
        sent to nodes[j] (n_sources rows, up to n_nodes columns; missing columns count zero):
        every cell added to each link of its tree path (in NetworkGraph.links() order) and to
        each node the path reaches after the source; a diagonal cell goes to its node's
        self-loop link (sg_link_load)."""
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        n = len(self.nodes)
        if c.ndim != 2 or c.shape[0] != self.n_sources or c.shape[1] > n:
            raise ValueError(f"counts: {self.n_sources} rows of at most {n} columns")
        g = self._graph
        n_links = len(g.links()[0])
        link, node = np.zeros(n_links, np.uint64), np.zeros(n, np.uint64)
        pred = self._rows()[0]
        check(g.ctx.handle, load().sg_link_load(
            *self._call_prefix(pred), c.ctypes.data, c.shape[1], link.ctypes.data, node.ctypes.data))
        return link, node

    def link_load_round(self, hosts, packets, status=None, weight=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(link_load, node_load, hops) of one round's batch: every counted packet of `packets`
        (a PacketBatch sent by hosts of `hosts`, a HostTable whose route indices are this tree's
        columns, every sender on a source row) adds its weight to each link of its tree path (in
        NetworkGraph.links() order) and to each node the path reaches after the source; a packet
        to its own node goes to the self-loop link.  hops[p] = the links packet p crossed,
        0xFFFFFFFF where it does not count.  status: the round's statuses (a Deliveries, or a
        torch / numpy u8 array of SG_PKT_*), a packet counting when delivered; None: every packet.
        weight: None (1 per packet), "payload" (the batch's payload_len) or a u32 array
        (sg_link_load_packets)."""
        status, weight = self._status_weight(packets, status, weight)
        g = self._graph
        link, node = np.zeros(len(g.links()[0]), np.uint64), np.zeros(len(self.nodes), np.uint64)
        hops = np.zeros(len(packets), np.uint32)
        pred = self._rows()[0]
        p = packets.c_struct()
        check(g.ctx.handle, load().sg_link_load_packets(
            *self._call_prefix(pred, hosts), C.byref(p), _dev_ptr(status), _dev_ptr(weight), link.ctypes.data,
            node.ctypes.data, hops.ctypes.data))
        return link, node, hops

    def _records(self, n_off: int, n_items: int, dtypes, call):
        """(off, one array per dtype cut to the record total) from call(the arrays' addresses ..., cap,
        total) on host arrays, off of n_off entries first, at a capacity with_capacity finds."""
        off = np.zeros(n_off, np.uint64)
        total = C.c_uint64()
        rc, t, arrays = with_capacity(
            n_items, lambda cap: [np.zeros(cap, dt) for dt in dtypes],
            lambda arrays, cap: (call(off.ctypes.data, *[a.ctypes.data for a in arrays], cap, C.byref(total)), total.value))
        check(self._graph.ctx.handle, rc)
        return (off,) + tuple(a[:t] for a in arrays)

    def _hop_records(self, n_items: int, call) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(off, node, link, latency_ns, packet_loss) from call(off, node, link, lat, loss, cap, total),
        one of the two sg_tree_paths entry points."""
        return self._records(n_items + 1, n_items, (np.uint32, np.uint32, np.uint64, np.float32), call)

    def paths(self, src, dst) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The tree paths of the pairs (src[p], dst[p]) (node indices, every src a source of this
        tree) as hop records, (off, node, link, latency_ns, packet_loss): pair p owns records
        off[p] .. off[p + 1], one per link crossed, source to destination: the node reached, the
        link (in NetworkGraph.links() order) and the table's (latency, loss) of that node in the
        source's row.  [src[p]] + node[off[p]:off[p + 1]] is path(src[p], dst[p]); a pair with
        src == dst has one record, its node's self-loop link and diagonal cell (sg_tree_paths)."""
        src, dst = np.atleast_1d(np.asarray(src)), np.atleast_1d(np.asarray(dst))
        if src.shape != dst.shape or src.ndim != 1:
            raise ValueError("paths: src and dst are two 1-d arrays of one length")
        rows = np.array([self._row(v) for v in src.tolist()], np.uint32)
        cols = np.array([self.index[int(v)] for v in dst.tolist()], np.uint32)
        pred, tlat, tloss = self._rows()

        def call(*out):
            return load().sg_tree_paths(*self._call_prefix(pred), tlat.ctypes.data, tloss.ctypes.data, len(rows),
                                        rows.ctypes.data, cols.ctypes.data, *out)

        return self._hop_records(len(rows), call)

    def trace_round(self, hosts, packets, status=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray,
                                                                 np.ndarray]:
        """The hop records of one round's batch, (off, node, link, latency_ns, packet_loss) as
        `paths` gives them: packet p of `packets` (a PacketBatch sent by hosts of `hosts`, a
        HostTable whose route indices are this tree's columns, every sender on a source row) owns
        records off[p] .. off[p + 1], none when it does not count.  status: the round's statuses (a
        Deliveries, or a torch / numpy u8 array of SG_PKT_*), a packet counting when delivered;
        None: every packet (sg_tree_paths_packets)."""
        status = self._status_weight(packets, status)[0]
        pred, tlat, tloss = self._rows()
        p = packets.c_struct()

        def call(*out):
            return load().sg_tree_paths_packets(*self._call_prefix(pred, hosts), tlat.ctypes.data, tloss.ctypes.data,
                                                C.byref(p), _dev_ptr(status), *out)

        return self._hop_records(len(packets), call)

    def link_trace_round(self, hosts, packets, status=None, watch=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray,
                                                                                 np.ndarray, np.ndarray]:
        """The link trace of one round's batch, (link_off, packet, hop, enter_ns, exit_ns): link L
        (in NetworkGraph.links() order) owns records link_off[L] .. link_off[L + 1], one per counted
        packet that crossed it, in ascending (enter_ns, packet) order; hop is the crossing's place
        on the packet's path (record off[packet] + hop - 1 of trace_round), enter_ns / exit_ns the
        packet's send time plus the table's latency of the link's tail / head in the sender's row.
        hosts, packets and status as in trace_round.  watch: None (every link), a u8 / bool mask
        of one entry per link, or a list of link numbers; a link not watched owns no record
        (sg_link_trace_packets)."""
        status = self._status_weight(packets, status)[0]
        n_links = len(self._graph.links()[0])
        watch = watch_mask(watch, n_links)
        pred, tlat, _ = self._rows()
        p = packets.c_struct()

        def call(*out):
            return load().sg_link_trace_packets(*self._call_prefix(pred, hosts), tlat.ctypes.data, C.byref(p),
                                                _dev_ptr(status), None if watch is None else watch.ctypes.data, *out)

        return self._records(n_links + 1, len(packets), (np.uint32, np.uint32, np.uint64, np.uint64), call)

    def link_series_round(self, hosts, packets, status=None, weight=None, *, t0_ns: int, bin_ns: int, n_bins: int,
                          slots=None, at: str = "enter", out=None) -> Tuple[np.ndarray, np.ndarray]:
        """The link time series of one round's batch, (series, outside): series[s, b] (u64, n_slots
        x n_bins) is the weight of the counted packets that crossed a link of slot s at a time t
        with t0_ns + b bin_ns <= t < t0_ns + (b + 1) bin_ns, t the crossing's enter_ns (at =
        "enter") or exit_ns ("exit") as link_trace_round gives them; outside[s] = (the weight
        before t0_ns, the weight at or past the last bin's end).  hosts, packets and status as in
        trace_round, weight as in link_load_round.  slots: None (a slot per link, in
        NetworkGraph.links() order), a list of link numbers (slot = position in the list) or a
        full u32 map of one entry per link (0xFFFFFFFF: not watched; links may share a slot).
        out: a previous result to add into, so that a loop over rounds keeps one matrix
        (sg_link_series_packets)."""
        if at not in ("enter", "exit"):
            raise ValueError('at: "enter" or "exit"')
        status, weight = self._status_weight(packets, status, weight)
        g = self._graph
        slot_map, n_slots = series_slots(slots, len(g.links()[0]))
        if out is None:
            series, outside = np.zeros((n_slots, int(n_bins)), np.uint64), np.zeros((n_slots, 2), np.uint64)
        else:
            series, outside = series_out(out, n_slots, int(n_bins))
        pred, tlat, _ = self._rows()
        p = packets.c_struct()
        check(g.ctx.handle, load().sg_link_series_packets(
            *self._call_prefix(pred, hosts), tlat.ctypes.data, C.byref(p), _dev_ptr(status), _dev_ptr(weight),
            None if slot_map is None else slot_map.ctypes.data, n_slots, 0 if at == "enter" else 1, int(t0_ns),
            int(bin_ns), int(n_bins), series.ctypes.data, outside.ctypes.data))
        return series, outside

    def link_trace_device(self, hosts, packets, status=None, weight=None, watch=None, tail: int = 0):
        """The link trace of one round's batch, left on the device (sg_link_trace_packets): (link_off,
        the number of records t, enter, packet, weight, hop, exit) as torch tensors of at least t
        entries -- int64 / int32 views of the u64 / u32 arrays; enter with `tail` more entries
        behind its capacity; weight per packet, None where every crossing weighs 1.  hosts,
        packets, status, weight and watch as in link_queue_round."""
        import torch

        npk = len(packets)
        dev = packets.src_host.device
        status, weight = self._status_weight(packets, status, weight)
        if weight is not None and tail:
            weight = weight[:npk]
        g = self._graph
        n_links = len(g.links()[0])
        watch = watch_mask(watch, n_links)
        if watch is not None:
            watch = torch.from_numpy(watch).to(dev)
        pred, tlat = (torch.from_numpy(a.view(dt)).to(dev) for a, dt in zip(self._rows(), (np.int32, np.int64)))
        off = torch.zeros(n_links + 1, dtype=torch.int64, device=dev)

        def alloc(cap):  # (pkt, hop, enter with room for the base times behind the records, leave)
            return [torch.zeros(cap + k, dtype=dt, device=dev) for dt, k in
                    ((torch.int32, 0), (torch.int32, 0), (torch.int64, tail), (torch.int64, 0))]

        def call(arrays, cap):
            torch.cuda.synchronize(dev)
            return g.link_trace_packets_device(
                hosts, self.nodes, 0, self.n_sources, pred.data_ptr(), tlat.data_ptr(), packets,
                0 if status is None else status.data_ptr(), 0 if watch is None else watch.data_ptr(), off.data_ptr(),
                *[a.data_ptr() for a in arrays], cap)

        _, t, (pkt, hop, enter, leave) = with_capacity(npk, alloc, call)
        return off, t, enter, pkt, weight, hop, leave

    def link_queue_round(self, hosts, packets, status=None, weight=None, *, cost_ps, watch=None, free_ns=None,
                         carry=False, limit_ns=None, outcomes=None, window_ns=None, series=None):
        """The link trace of one round's batch and the FIFO queue of every link under a link rate,
        (link_off, packet, hop, enter_ns, exit_ns, queue): the first five as link_trace_round
        gives them, queue a LinkQueueResult over the same records.  The trace stays on the device
        between the two calls (sg_link_trace_packets, then sg_link_queue).  weight as in
        link_load_round: None (every crossing weighs 1), "payload" or a u32 array per packet;
        cost_ps and free_ns as in shadow_amd.link_queue; hosts, packets, status and watch as in
        link_trace_round.  First order: a crossing's wait is not added to the packet's later hops.
        carry=True: it is (SG_LINK_QUEUE_CARRY).  queue is then a LinkQueueCarried, and a seventh
        entry follows it: the carried exit_ns per record, exit_ns + (done_ns - enter_ns), when the
        crossing leaves its link under the rates; a packet's last hop's value is its arrival.  An
        unwatched link is crossed at its latency, as a link of infinite rate.
        limit_ns: one u64 per link, the longest wait its buffer holds (SG_LINK_QUEUE_DROP, as in
        shadow_amd.link_queue).  queue is then a LinkQueueDropped or, with carry=True, a
        LinkQueueCarriedDropped, and the carried exit_ns is 2^64 - 1 at a dropped or absent hop.
        outcomes: the round's Deliveries, or a u64 array or tensor of one base time per packet
        (SG_LINK_QUEUE_PACKETS).  A PacketOutcomes is then the tuple's last entry: every packet's
        delay and arrival under the rates and where it was dropped, folded on the device; its
        arrive_dev is what PacketWire.push(deliver_time_ns=...) takes.
        window_ns: with carry=True, solve the trace window by window: a LinkQueueSession takes the
        whole trace and its horizon steps by window_ns from the first record on (past a stretch in
        which nothing is pending it jumps to the next pending record), every call sorting and
        scanning only the records below its horizon.  The result is the one carry=True gives, but
        for `iterations`, the calls' sum.  A call counts `ahead` over its own settled records
        only, so ahead and link_ahead_max are counted again here on the host, from the settled
        carried enter and done times.
        series: a LinkQueueSeries over the graph's links (SG_LINK_QUEUE_SERIES): the round's busy time,
        waiting time, weight served and weight dropped per slot and time bin are added into its
        matrix on the device, with window_ns= by every window's call.  The result is unchanged."""
        import torch  # noqa: F401

        if window_ns is not None and (not carry or int(window_ns) < 1):
            raise ValueError("window_ns: a positive number of ns, with carry=True")

        npk = len(packets)
        dev = packets.src_host.device
        base = None if outcomes is None else _base_times(outcomes, npk, dev)
        off, t, enter, pkt, weight, hop, leave = self.link_trace_device(hosts, packets, status, weight, watch,
                                                                        0 if base is None else npk)
        g = self._graph
        n_links = off.numel() - 1
        if window_ns is not None:
            queue = _link_queue_windows(g.ctx, dev, n_links, off, t, enter, pkt, weight, cost_ps, free_ns, npk, limit_ns, base,
                                        int(window_ns), series)
        else:
            queue = _link_queue_tensors(g.ctx, dev, n_links, off, t, enter, pkt, weight, cost_ps, free_ns, carry, npk,
                                        limit_ns, base, series)
        tails = ()
        if base is not None:
            queue, tails = queue[0], (queue[1],)
        out = (off.cpu().numpy().view(np.uint64), pkt[:t].cpu().numpy().view(np.uint32),
               hop[:t].cpu().numpy().view(np.uint32), enter[:t].cpu().numpy().view(np.uint64),
               leave[:t].cpu().numpy().view(np.uint64), queue)
        return (out + (_exit_carried(out[4], out[3], queue),) if carry else out) + tails

    def path_properties(self, src: int, dst: int) -> PathProperties:
        """The left fold default() + e1 + ... + ek over the tree path's edges (graph/mod.rs:322-331),
        taking at each step any arc that is tight: one whose fold gives the table's cell of the
        step's head, latency and loss bits.  Equals the table's cell for (src, dst); for
        src == dst it is default(), not the self-loop the table's diagonal holds."""
        i = self._row(src)
        arcs = self._graph._arcs_between()
        acc = DEFAULT_PATH
        nodes = self.path(src, dst)
        for u, v in zip(nodes[:-1], nodes[1:]):
            j = self.index[v]
            want = (int(self.latency_ns[i, j]), np.float32(self.packet_loss[i, j]).view(np.uint32))
            for e in arcs.get((u, v), ()):
                got = acc + PathProperties(int(self._graph.edge_latency_ns[e]), self._graph.edge_packet_loss[e])
                if (got.latency_ns, np.float32(got.packet_loss).view(np.uint32)) == want:
                    acc = got
                    break
            else:
                raise ShadowGpuError(_capi.SG_ERR_INVALID_ARG, f"no tight arc {u} -> {v} on the path {src} -> {dst}",
                                     (i, j))
        return acc


# ---------------------------------------------------------------------------
# NetworkGraph (graph/mod.rs:113-294)
# ---------------------------------------------------------------------------
class NetworkGraph:
    def __init__(self, n_nodes: int, edge_src, edge_dst, edge_latency_ns, edge_packet_loss,
                 directed: bool, node_ids: Optional[Sequence[int]] = None, ctx: Optional[Context] = None):
        self._ctx = ctx
        self.n_nodes = int(n_nodes)
        self.directed = bool(directed)
        self.edge_src = np.ascontiguousarray(edge_src, dtype=np.uint32)
        self.edge_dst = np.ascontiguousarray(edge_dst, dtype=np.uint32)
        self.edge_latency_ns = np.ascontiguousarray(edge_latency_ns, dtype=np.uint64)
        self.edge_packet_loss = np.ascontiguousarray(edge_packet_loss, dtype=np.float32)
        # GML node ids; None: each node's index (built only if asked for, and not passed to
        # sg_net_create, which then names nodes by index -- a one-shot build skips both)
        self._node_ids = None if node_ids is None else np.ascontiguousarray(node_ids, dtype=np.uint32)
        self._id_to_index = None  # built on first lookup
        self._net = None

    @property
    def node_ids(self) -> np.ndarray:
        """The GML node id of each node index."""
        if self._node_ids is None:
            self._node_ids = np.arange(self.n_nodes, dtype=np.uint32)
        return self._node_ids

    @property
    def ctx(self) -> Context:
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def _graph_struct(self) -> _capi.sg_graph:
        g = _capi.sg_graph()
        g.n_nodes = self.n_nodes
        g.n_edges = len(self.edge_src)
        # (the arrays' addresses straight from the array interface: ndarray.ctypes builds a helper
        # object per call, and this runs in every one-shot build)
        ptr = lambda a, t: C.cast(a.__array_interface__["data"][0], C.POINTER(t))
        g.edge_src = ptr(self.edge_src, C.c_uint32)
        g.edge_dst = ptr(self.edge_dst, C.c_uint32)
        g.edge_latency_ns = ptr(self.edge_latency_ns, C.c_uint64)
        g.edge_packet_loss = ptr(self.edge_packet_loss, C.c_float)
        g.node_gml_id = None if self._node_ids is None else ptr(self._node_ids, C.c_uint32)
        g.directed = 1 if self.directed else 0
        return g

    def _ensure_net(self):
        """Upload the edge list once (sg_net_create) on first use of the device."""
        if self._net is None:
            self._upload()
        return self._net

    def _upload(self) -> None:
        L = load()
        g = self._graph_struct()
        h = C.c_void_p()
        check(self.ctx.handle, L.sg_net_create(self.ctx.handle, C.byref(g), C.byref(h)))
        self._net = h

    def close(self) -> None:
        """Release the device graph (sg_net_destroy) now rather than at garbage collection."""
        if self._net:
            load().sg_net_destroy(self._net)
            self._net = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def parse(cls, graph_text, ctx: Optional[Context] = None, threads: int = 0) -> "NetworkGraph":
        """NetworkGraph::parse (graph/mod.rs:134-181); raises ShadowGpuError(SG_ERR_PARSE).
        graph_text: str or bytes (UTF-8).  threads: host threads for the parse (0 = min(cores, 16))."""
        L = load()
        raw = graph_text.encode() if isinstance(graph_text, str) else bytes(graph_text)
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = L.sg_gml_parse_threads(raw, len(raw), int(threads), C.byref(h), err, len(err))
        if rc != _capi.SG_OK:
            raise ShadowGpuError(rc, err.value.decode(errors="replace") or f"parse status {rc}")
        return cls._from_handle(h, ctx)

    @classmethod
    def _from_handle(cls, h, ctx) -> "NetworkGraph":
        L = load()
        try:
            g = _capi.sg_graph()
            check(None, L.sg_gml_graph(h, C.byref(g)))
            n, m = g.n_nodes, g.n_edges
            arr = lambda p, cnt, dt: np.ctypeslib.as_array(p, shape=(cnt,)).astype(dt) if cnt else np.zeros(0, dt)
            return cls(n, arr(g.edge_src, m, np.uint32), arr(g.edge_dst, m, np.uint32),
                       arr(g.edge_latency_ns, m, np.uint64), arr(g.edge_packet_loss, m, np.float32),
                       bool(g.directed), arr(g.node_gml_id, n, np.uint32), ctx)
        finally:
            L.sg_gml_destroy(h)

    @classmethod
    def from_file(cls, path, compression: Optional[str] = None, ctx: Optional[Context] = None,
                  threads: int = 0) -> "NetworkGraph":
        """load_network_graph + NetworkGraph::parse (graph/mod.rs:483-513) in the native
        library (sg_gml_load): a GML file, plain or xz-compressed (compression="xz", read_xz
        :484-496; decompressed by the system liblzma), checked to be UTF-8
        (String::from_utf8), then parsed on `threads` threads."""
        if compression not in (None, "xz"):
            raise ValueError(f"unknown compression {compression!r} (configuration.rs:985-988: xz)")
        L = load()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = L.sg_gml_load(str(path).encode(), 1 if compression == "xz" else 0, int(threads), C.byref(h), err,
                           len(err))
        if rc != _capi.SG_OK:
            raise ShadowGpuError(rc, err.value.decode(errors="replace") or f"load status {rc}")
        return cls._from_handle(h, ctx)

    def node_id_to_index(self, node_id: int) -> Optional[int]:
        if self._id_to_index is None:  # graph/mod.rs:155-162: a later duplicate id wins
            self._id_to_index = {int(i): k for k, i in enumerate(self.node_ids)}
        return self._id_to_index.get(int(node_id))

    def node_index_to_id(self, index: int) -> Optional[int]:
        return int(self.node_ids[index]) if 0 <= index < self.n_nodes else None

    # -- routing ------------------------------------------------------------
    def _build(self, nodes: Sequence[int], shortest: bool) -> PathTable:
        L = load()
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        nu = len(used)
        lat = np.zeros((nu, nu), np.uint64)
        loss = np.zeros((nu, nu), np.float32)
        flags = _capi.SG_ROUTE_SHORTEST_PATH if shortest else 0
        check(self.ctx.handle, L.sg_routing_build(self.ctx.handle, self._ensure_net(), used.ctypes.data, nu, 0, nu, flags,
                                                  lat.ctypes.data, loss.ctypes.data))
        return PathTable(used.tolist(), lat, loss)

    def compute_shortest_paths(self, nodes: Sequence[int]) -> PathTable:
        """graph/mod.rs:183-228 (bit-exact latency and f32 loss)."""
        return self._build(nodes, True)

    def get_direct_paths(self, nodes: Sequence[int]) -> PathTable:
        """graph/mod.rs:230-252."""
        return self._build(nodes, False)

    def build_rows_device(self, nodes: Sequence[int], row_begin: int, row_end: int, out_latency_ptr: int,
                          out_loss_ptr: int, shortest: bool = True) -> None:
        """Rows [row_begin, row_end) into caller-owned device buffers (sharded build)."""
        L = load()
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        flags = (_capi.SG_ROUTE_SHORTEST_PATH if shortest else 0) | _capi.SG_ROUTE_OUT_DEVICE
        check(self.ctx.handle, L.sg_routing_build(self.ctx.handle, self._ensure_net(), used.ctypes.data, len(used),
                                                  int(row_begin), int(row_end), flags, C.c_void_p(out_latency_ptr),
                                                  C.c_void_p(out_loss_ptr)))

    # -- shortest-path trees -------------------------------------------------
    def _arcs_between(self):
        """(u, v) -> the edges that give an arc u -> v (self-loops left out), built once."""
        if getattr(self, "_arc_index", None) is None:
            idx: Dict[Tuple[int, int], List[int]] = {}
            for e, (a, b) in enumerate(zip(self.edge_src.tolist(), self.edge_dst.tolist())):
                if a == b:
                    continue
                idx.setdefault((a, b), []).append(e)
                if not self.directed:
                    idx.setdefault((b, a), []).append(e)
            self._arc_index = idx
        return self._arc_index

    def tree_permutation(self, sources: Optional[Sequence[int]] = None) -> np.ndarray:
        """Every graph node once, `sources` first (in their order), the rest ascending."""
        if sources is None:
            return np.arange(self.n_nodes, dtype=np.uint32)
        first = np.ascontiguousarray(sources, dtype=np.uint32)
        rest = np.setdiff1d(np.arange(self.n_nodes, dtype=np.uint32), first)
        return np.ascontiguousarray(np.concatenate([first, rest]), dtype=np.uint32)

    def compute_shortest_path_tree(self, sources: Optional[Sequence[int]] = None) -> PathTree:
        """compute_shortest_paths (graph/mod.rs:183-228) from `sources` (petgraph indices, default
        all) to every graph node, with the predecessor and first-hop rows of those paths
        (sg_routing_build_tree).  The sources come first in the result's node order, so its
        leading len(sources) columns are compute_shortest_paths(sources)."""
        nodes = self.tree_permutation(sources)
        n, k = len(nodes), self.n_nodes if sources is None else len(sources)
        lat = np.zeros((k, n), np.uint64)
        loss = np.zeros((k, n), np.float32)
        pred = np.zeros((k, n), np.uint32)
        hop = np.zeros((k, n), np.uint32)
        check(self.ctx.handle, load().sg_routing_build_tree(
            self.ctx.handle, self._ensure_net(), nodes.ctypes.data, n, 0, k, _capi.SG_ROUTE_SHORTEST_PATH,
            lat.ctypes.data, loss.ctypes.data, pred.ctypes.data, hop.ctypes.data))
        return PathTree(self, nodes, k, lat, loss, pred, hop)

    def tree_rows_device(self, nodes: Sequence[int], row_begin: int, row_end: int, latency_ptr: int, loss_ptr: int,
                         out_pred_ptr: int, out_first_hop_ptr: int) -> None:
        """Rows [row_begin, row_end) of pred / first_hop from the same rows of a device table
        (as build_rows_device wrote them for the same `nodes`, a permutation of every node), into
        caller-owned device buffers; either output pointer may be 0 (sg_routing_tree)."""
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        check(self.ctx.handle, load().sg_routing_tree(
            self.ctx.handle, self._ensure_net(), used.ctypes.data, len(used), int(row_begin), int(row_end),
            _capi.SG_ROUTE_OUT_DEVICE, C.c_void_p(latency_ptr), C.c_void_p(loss_ptr), _vp(out_pred_ptr),
            _vp(out_first_hop_ptr)))

    # -- link loads -----------------------------------------------------------
    def links(self) -> Tuple[np.ndarray, np.ndarray]:
        """(tail, head) of every link: the distinct ordered node pairs joined by an edge (an
        undirected edge gives both directions, parallel edges one link), ascending (head, tail)
        (sg_net_links).  link_load arrays are in this order."""
        L, n = load(), C.c_uint32()
        net = self._ensure_net()
        rc = L.sg_net_links(self.ctx.handle, net, C.byref(n), None, None, 0)
        if rc not in (_capi.SG_OK, _capi.SG_ERR_CAPACITY):
            check(self.ctx.handle, rc)
        tail, head = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        check(self.ctx.handle, L.sg_net_links(self.ctx.handle, net, C.byref(n), tail.ctypes.data, head.ctypes.data,
                                              n.value))
        return tail, head

    def edge_links(self) -> Tuple[np.ndarray, np.ndarray]:
        """(fwd, rev): per edge, the link (src -> dst) and the link (dst -> src), the latter
        0xFFFFFFFF on a directed graph (sg_net_edge_links).  Parallel edges share a link."""
        m = len(self.edge_src)
        fwd, rev = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        check(self.ctx.handle, load().sg_net_edge_links(self.ctx.handle, self._ensure_net(), fwd.ctypes.data,
                                                        rev.ctypes.data))
        return fwd, rev

    def link_load_device(self, nodes: Sequence[int], row_begin: int, row_end: int, pred_ptr: int, counts_ptr: int,
                         count_cols: int, link_ptr: int, node_ptr: int) -> None:
        """Rows [row_begin, row_end) of a device u64 matrix (count_cols columns) added onto the
        links and nodes of their tree paths through the same rows of device pred rows (as
        tree_rows_device wrote them for the same `nodes`); the device outputs (u64, one per
        link in links() order / one per node) are added to, and either may be 0 (sg_link_load)."""
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        check(self.ctx.handle, load().sg_link_load(
            self.ctx.handle, self._ensure_net(), used.ctypes.data, len(used), int(row_begin), int(row_end),
            _capi.SG_ROUTE_OUT_DEVICE, C.c_void_p(pred_ptr), _vp(counts_ptr), int(count_cols), _vp(link_ptr),
            _vp(node_ptr)))

    def link_load_packets_device(self, hosts, nodes: Sequence[int], row_begin: int, row_end: int, pred_ptr: int,
                                 packets, status_ptr: int, weight_ptr: int, link_ptr: int, node_ptr: int,
                                 hops_ptr: int) -> None:
        """One round's batch (a PacketBatch from hosts of `hosts`, a HostTable) added onto the links
        and nodes of its packets' tree paths through device pred rows [row_begin, row_end): a
        packet counts when its status (device u8, 0: every packet) is SG_PKT_DELIVERED and adds
        its weight (device u32, 0: 1); the device outputs (u64 per link / per node, added to; u32
        hops per packet, written) may be 0, not all three (sg_link_load_packets)."""
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        p = packets.c_struct()
        check(self.ctx.handle, load().sg_link_load_packets(
            self.ctx.handle, self._ensure_net(), hosts.handle, used.ctypes.data, len(used), int(row_begin),
            int(row_end), _capi.SG_ROUTE_OUT_DEVICE, C.c_void_p(pred_ptr), C.byref(p), _vp(status_ptr), _vp(weight_ptr),
            _vp(link_ptr), _vp(node_ptr), _vp(hops_ptr)))

    def tree_paths_device(self, nodes: Sequence[int], row_begin: int, row_end: int, pred_ptr: int, latency_ptr: int,
                          loss_ptr: int, n_pairs: int, pair_row_ptr: int, pair_col_ptr: int, off_ptr: int,
                          node_ptr: int, link_ptr: int, out_latency_ptr: int, out_loss_ptr: int, cap: int) -> int:
        """The hop records of n_pairs pairs (device u32 row / column indices in `nodes` order)
        through device pred rows [row_begin, row_end) and the same rows of the device table, into
        caller-owned device arrays: off (u64, n_pairs + 1), then per record node u32, link u32,
        latency u64, loss f32, each of `cap` records; any record array may be 0, not all four,
        and a table pointer may be 0 when its output is.  Returns the record total; when it
        exceeds `cap`, off is complete and no record was written (sg_tree_paths)."""
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        total = C.c_uint64()
        rc = load().sg_tree_paths(
            self.ctx.handle, self._ensure_net(), used.ctypes.data, len(used), int(row_begin), int(row_end),
            _capi.SG_ROUTE_OUT_DEVICE, C.c_void_p(pred_ptr), _vp(latency_ptr), _vp(loss_ptr), int(n_pairs),
            _vp(pair_row_ptr), _vp(pair_col_ptr), _vp(off_ptr), _vp(node_ptr), _vp(link_ptr), _vp(out_latency_ptr),
            _vp(out_loss_ptr), int(cap), C.byref(total))
        if rc != _capi.SG_ERR_CAPACITY:
            check(self.ctx.handle, rc)
        return total.value

    def tree_paths_packets_device(self, hosts, nodes: Sequence[int], row_begin: int, row_end: int, pred_ptr: int,
                                  latency_ptr: int, loss_ptr: int, packets, status_ptr: int, off_ptr: int,
                                  node_ptr: int, link_ptr: int, out_latency_ptr: int, out_loss_ptr: int,
                                  cap: int) -> int:
        """tree_paths_device for one round's batch (a PacketBatch from hosts of `hosts`, a
        HostTable): packet p owns records off[p] .. off[p + 1], none unless its status (device u8,
        0: every packet) is SG_PKT_DELIVERED; the pairs are link_load_packets_device's
        (sg_tree_paths_packets)."""
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        total = C.c_uint64()
        p = packets.c_struct()
        rc = load().sg_tree_paths_packets(
            self.ctx.handle, self._ensure_net(), hosts.handle, used.ctypes.data, len(used), int(row_begin),
            int(row_end), _capi.SG_ROUTE_OUT_DEVICE, C.c_void_p(pred_ptr), _vp(latency_ptr), _vp(loss_ptr), C.byref(p),
            _vp(status_ptr), _vp(off_ptr), _vp(node_ptr), _vp(link_ptr), _vp(out_latency_ptr), _vp(out_loss_ptr),
            int(cap), C.byref(total))
        if rc != _capi.SG_ERR_CAPACITY:
            check(self.ctx.handle, rc)
        return total.value

    def link_trace_packets_device(self, hosts, nodes: Sequence[int], row_begin: int, row_end: int, pred_ptr: int,
                                  latency_ptr: int, packets, status_ptr: int, watch_ptr: int, link_off_ptr: int,
                                  packet_ptr: int, hop_ptr: int, enter_ptr: int, exit_ptr: int,
                                  cap: int) -> Tuple[int, int]:
        """The link trace of one round's batch (a PacketBatch from hosts of `hosts`, a HostTable)
        through device pred rows [row_begin, row_end) and the same rows of the device latency
        table, into caller-owned device arrays: link_off (u64, one entry per link of links() and
        one more), then per record packet u32, hop u32, enter_ns u64, exit_ns u64, each of `cap`
        records and sorted by (enter_ns, packet) inside a link's segment; any record array may be
        0, not all four.  status (device u8, 0: every packet) as in tree_paths_packets_device;
        watch (device u8 per link, 0: every link) empties the segments of the links it marks 0.
        Returns (status code, record total): SG_OK, or SG_ERR_CAPACITY when the total exceeds
        `cap` (link_off is complete then and no record was written); any other status raises
        (sg_link_trace_packets)."""
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        total = C.c_uint64()
        p = packets.c_struct()
        rc = load().sg_link_trace_packets(
            self.ctx.handle, self._ensure_net(), hosts.handle, used.ctypes.data, len(used), int(row_begin),
            int(row_end), _capi.SG_ROUTE_OUT_DEVICE, C.c_void_p(pred_ptr), _vp(latency_ptr), C.byref(p), _vp(status_ptr),
            _vp(watch_ptr), _vp(link_off_ptr), _vp(packet_ptr), _vp(hop_ptr), _vp(enter_ptr), _vp(exit_ptr), int(cap),
            C.byref(total))
        if rc != _capi.SG_ERR_CAPACITY:
            check(self.ctx.handle, rc)
        return rc, total.value

    def link_series_packets_device(self, hosts, nodes: Sequence[int], row_begin: int, row_end: int, pred_ptr: int,
                                   latency_ptr: int, packets, status_ptr: int, weight_ptr: int, slot_ptr: int,
                                   n_slots: int, at: int, t0_ns: int, bin_ns: int, n_bins: int, series_ptr: int,
                                   outside_ptr: int) -> None:
        """One round's batch (a PacketBatch from hosts of `hosts`, a HostTable) added into a device
        matrix of n_slots x n_bins u64 cells through device pred rows [row_begin, row_end) and the
        same rows of the device latency table: every crossing of a counted packet adds the packet's
        weight (device u32, 0: 1) to the cell (slot[link], (t - t0_ns) // bin_ns), t its enter
        (at = 0) or exit (at = 1) time; crossings before t0_ns or past the last bin go to
        outside[2 s] / outside[2 s + 1] (device u64, 2 n_slots, or 0).  slot: device u32 per link of
        links(), 0xFFFFFFFF for a link not watched, or 0: the identity, with n_slots the link
        count.  status as in link_load_packets_device (sg_link_series_packets)."""
        used = np.ascontiguousarray(nodes, dtype=np.uint32)
        p = packets.c_struct()
        check(self.ctx.handle, load().sg_link_series_packets(
            self.ctx.handle, self._ensure_net(), hosts.handle, used.ctypes.data, len(used), int(row_begin),
            int(row_end), _capi.SG_ROUTE_OUT_DEVICE, C.c_void_p(pred_ptr), _vp(latency_ptr), C.byref(p), _vp(status_ptr),
            _vp(weight_ptr), _vp(slot_ptr), int(n_slots), int(at), int(t0_ns), int(bin_ns), int(n_bins), _vp(series_ptr),
            _vp(outside_ptr)))

    def link_queue_device(self, link_off_ptr: int, n_records: int, enter_ptr: int, packet_ptr: int, weight_ptr: int,
                          n_weights: int, cost_ptr: int, free_in_ptr: int = 0, *, wait_ptr: int = 0, done_ptr: int = 0,
                          ahead_ptr: int = 0, link_free_ptr: int = 0, busy_ptr: int = 0, wait_max_ptr: int = 0,
                          wait_sum_ptr: int = 0, ahead_max_ptr: int = 0, carry: bool = False, limit_ns=None,
                          outcomes: bool = False, horizon_ns=None, series=None) -> None:
        """The FIFO queue of every link of a device link trace under a link rate, into caller-owned
        device arrays: link_off (u64, one entry per link of links() and one more), enter (u64) and
        packet (u32) of n_records records as link_trace_packets_device wrote them; weight (device
        u32, n_weights entries indexed by packet; 0: every record weighs 1, packet may be 0 too);
        cost (device u64 per link, picoseconds per weight unit); free_in (device u64 per link, 0:
        all zero).  Outputs, any of them 0 but not all: per record wait u64, done u64, ahead u32;
        per link link_free u64 (not free_in's array), busy u64, wait_max u64, wait_sum u64,
        ahead_max u32 (sg_link_queue).  carry: every wait is carried to the packet's later hops
        (SG_LINK_QUEUE_CARRY: packet is required and n_weights bounds it); the call then
        synchronises once per iteration, read_timer("link_queue_iters") tells how many it took.
        limit_ns: a host array of one u64 per link, the longest wait its buffer holds
        (SG_LINK_QUEUE_DROP).  cost is then copied, with the limits behind it, into the doubled
        array the call takes; busy and ahead_max must have two entries per link (the second
        halves: the refused service and the drops per link), and the per-record outputs carry
        the states as sentinels (sg_link_queue).
        outcomes: the result per packet as well (SG_LINK_QUEUE_PACKETS).  enter, wait, done and
        ahead then have n_records + n_weights entries and all three outputs are required: the
        caller puts every packet's base time behind enter's records and finds its delay, its
        arrival and the record that dropped it behind the records of wait, done and ahead.
        horizon_ns: with carry, settle only the records whose carried enter time is below it
        (SG_LINK_QUEUE_WINDOW; link_queue tells what the pending ones get).  free_in is then copied, with the
        horizon behind it, into the array of one more entry the call takes.
        series: a LinkQueueSeries over the graph's links (SG_LINK_QUEUE_SERIES); wait and done are then
        required, with horizon_ns ahead as well.  cost is copied, with the series' header and slot
        map behind it, the call writes its per-link busy values in front of the series' matrix and
        adds into the matrix, and busy (if given) receives a copy of the per-link values."""
        n_links = len(self.links()[0])
        flags = _capi.SG_ROUTE_OUT_DEVICE | (_capi.SG_LINK_QUEUE_CARRY if carry else 0) | \
            (_capi.SG_LINK_QUEUE_PACKETS if outcomes else 0)
        if horizon_ns is not None:
            import torch

            if not carry or not 0 <= int(horizon_ns) <= _UMAX:
                raise ValueError("horizon_ns: a u64 time, with carry")
            h = np.array([int(horizon_ns)], np.uint64).view(np.int64)
            if free_in_ptr:
                class _Free:  # the n_links u64 at free_in_ptr, for torch
                    __cuda_array_interface__ = {"shape": (n_links,), "typestr": "<i8", "data": (int(free_in_ptr), False),
                                                "version": 2}
                old_free = torch.as_tensor(_Free(), device="cuda")
            else:
                old_free = torch.zeros(n_links, dtype=torch.int64, device="cuda")
            free2 = torch.cat([old_free, torch.from_numpy(h).to(old_free.device)]).contiguous()
            torch.cuda.synchronize(old_free.device)
            free_in_ptr = free2.data_ptr()
            flags |= _capi.SG_LINK_QUEUE_WINDOW
        if limit_ns is not None:
            import torch

            class _View:  # the n_links u64 at cost_ptr, for torch
                __cuda_array_interface__ = {"shape": (n_links,), "typestr": "<i8", "data": (int(cost_ptr), False),
                                            "version": 2}
            old = torch.as_tensor(_View(), device="cuda")
            lim = torch.from_numpy(_per_link_u64(limit_ns, n_links, "limit_ns").view(np.int64)).to(old.device)
            cost2 = torch.cat([old, lim]).contiguous()
            torch.cuda.synchronize(old.device)
            cost_ptr = cost2.data_ptr()
            flags |= _capi.SG_LINK_QUEUE_DROP
        own_busy = 0
        if series is not None:
            import torch

            series._check(n_links)
            c0 = 2 * n_links if limit_ns is not None else n_links

            class _Cost:  # the c0 u64 at cost_ptr, for torch
                __cuda_array_interface__ = {"shape": (c0,), "typestr": "<i8", "data": (int(cost_ptr), False), "version": 2}
            cost3 = series.device_cost(torch.as_tensor(_Cost(), device="cuda"))
            busy3 = series.device_busy(c0)
            torch.cuda.synchronize(cost3.device)
            cost_ptr, own_busy, busy_ptr = cost3.data_ptr(), busy_ptr, busy3.data_ptr()
            flags |= _capi.SG_LINK_QUEUE_SERIES
        check(self.ctx.handle, load().sg_link_queue(
            self.ctx.handle, flags, n_links, _vp(link_off_ptr), int(n_records), _vp(enter_ptr), _vp(packet_ptr),
            _vp(weight_ptr), int(n_weights), _vp(cost_ptr), _vp(free_in_ptr),
            *[_vp(x) for x in (wait_ptr, done_ptr, ahead_ptr, link_free_ptr, busy_ptr, wait_max_ptr, wait_sum_ptr,
                               ahead_max_ptr)]))
        if own_busy and c0:
            class _Busy:  # the caller's c0 u64 at busy_ptr
                __cuda_array_interface__ = {"shape": (c0,), "typestr": "<i8", "data": (int(own_busy), False), "version": 2}
            torch.as_tensor(_Busy(), device="cuda").copy_(busy3[:c0])
            torch.cuda.synchronize(busy3.device)

    def min_latency_device(self, latency_ptr: int, count: int) -> int:
        out = C.c_uint64()
        check(self.ctx.handle, load().sg_routing_min_latency(self.ctx.handle, C.c_void_p(latency_ptr), count,
                                                             C.byref(out)))
        return out.value


# ---------------------------------------------------------------------------
# RoutingInfo (graph/mod.rs:432-481) keyed by GML node id: a dense host table
# owned by libshadow_gpu (sg_routing_info, sg_route_info.hip)
# ---------------------------------------------------------------------------
class RoutingInfo:
    """RoutingInfo<u32>: path(start, end), get_smallest_latency_ns and the packet
    counters, over a dense table of 8-byte (latency, loss) cells in pinned host
    memory (row = source, in `node_ids` order).  `latency_ns` / `packet_loss` /
    `rows()` decode copies; `cells` is the zero-copy packed view.  With addresses attached
    (set_addresses) it also answers WorkerShared::latency / reliability /
    is_routable (worker.rs:517-555)."""

    def __init__(self, node_ids: Sequence[int], latency_ns: Optional[np.ndarray] = None,
                 packet_loss: Optional[np.ndarray] = None):
        L = load()
        ids = np.ascontiguousarray(node_ids, dtype=np.uint32)
        h = C.c_void_p()
        rc = L.sg_routing_info_create(len(ids), ids.ctypes.data, C.byref(h))
        if rc != _capi.SG_OK:
            raise ShadowGpuError(rc, "sg_routing_info_create failed (duplicate node id?)")
        self.handle = h
        self.node_ids = [int(x) for x in ids]
        self.n = len(ids)
        if latency_ns is not None:
            self.set_rows(0, np.asarray(latency_ns, np.uint64), np.asarray(packet_loss, np.float32))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            load().sg_routing_info_destroy(h)
            self.handle = None

    def fill(self, graph: "NetworkGraph", nodes: Sequence[int], use_shortest_paths: bool = True) -> None:
        """sg_routing_info_fill: the whole table from the GPU (nodes = petgraph indices of node_ids)."""
        idx = np.ascontiguousarray(nodes, dtype=np.uint32)
        assert len(idx) == self.n
        flags = _capi.SG_ROUTE_SHORTEST_PATH if use_shortest_paths else 0
        check(graph.ctx.handle, load().sg_routing_info_fill(graph.ctx.handle, graph._ensure_net(), idx.ctypes.data,
                                                             flags, self.handle))

    def set_rows(self, row_begin: int, latency_ns: np.ndarray, packet_loss: np.ndarray) -> None:
        lat = np.ascontiguousarray(latency_ns, np.uint64).reshape(-1, self.n)
        loss = np.ascontiguousarray(packet_loss, np.float32).reshape(-1, self.n)
        rc = load().sg_routing_info_set_rows(self.handle, int(row_begin), int(row_begin) + lat.shape[0],
                                             lat.ctypes.data, loss.ctypes.data)
        if rc != _capi.SG_OK:
            raise ShadowGpuError(rc, "sg_routing_info_set_rows: bad row range")

    def _view(self):
        v = _capi.sg_routing_view()
        load().sg_routing_info_view(self.handle, C.byref(v))
        return v

    def rows(self, row_begin: int = 0, row_end: Optional[int] = None):
        """Rows [row_begin, row_end) decoded from the 8-byte cells (sg_routing_info_rows): a
        (latency u64, loss f32) pair of new arrays."""
        _capi.require_abi(5, "RoutingInfo.rows")
        row_end = self.n if row_end is None else int(row_end)
        k = max(0, row_end - int(row_begin))
        lat = np.empty((k, self.n), np.uint64)
        loss = np.empty((k, self.n), np.float32)
        rc = load().sg_routing_info_rows(self.handle, int(row_begin), row_end, lat.ctypes.data, loss.ctypes.data)
        if rc != _capi.SG_OK:
            raise ShadowGpuError(rc, "sg_routing_info_rows: bad row range")
        return lat, loss

    @property
    def latency_ns(self) -> np.ndarray:
        """[n x n] latencies (a copy, decoded from the cells)."""
        return self.rows()[0]

    @property
    def packet_loss(self) -> np.ndarray:
        """[n x n] losses (a copy)."""
        return self.rows()[1]

    @property
    def cells(self) -> np.ndarray:
        """Zero-copy [n x n] view of the packed cells (latency << 32 | bits(loss); SG_CELL_WIDE in the
        upper half for paths of 2^32 - 1 ns or more).  The array keeps this object alive."""
        _capi.require_abi(5, "RoutingInfo.cells")
        v = self._view()
        if not self.n:
            return np.zeros((0, 0), np.uint64)
        buf = (C.c_uint64 * (self.n * self.n)).from_address(v.cells)
        buf._owner = self  # the frombuffer base chain keeps the table alive
        return np.frombuffer(buf, dtype=np.uint64).reshape(self.n, self.n)

    @property
    def pinned(self) -> bool:
        return bool(self._view().pinned)

    def index(self, node_id: int) -> Optional[int]:
        r = C.c_uint32()
        return int(r.value) if load().sg_routing_info_index(self.handle, int(node_id), C.byref(r)) == 0 else None

    def path(self, start: int, end: int) -> Optional[PathProperties]:
        """graph/mod.rs:448-450."""
        lat, loss = C.c_uint64(), C.c_float()
        if not load().sg_routing_info_path(self.handle, int(start), int(end), C.byref(lat), C.byref(loss)):
            return None
        return PathProperties(int(lat.value), np.float32(loss.value))

    def increment_packet_count(self, start: int, end: int) -> None:
        """graph/mod.rs:453-460 (saturating; the reference's caller unwraps an unknown pair)."""
        rc = load().sg_routing_info_increment_packet_count(self.handle, int(start), int(end))
        if rc != _capi.SG_OK:
            raise KeyError((start, end))

    def packet_count(self, start: int, end: int) -> int:
        return int(load().sg_routing_info_packet_count(self.handle, int(start), int(end)))

    def get_smallest_latency_ns(self) -> Optional[int]:
        """graph/mod.rs:478-480: min over every entry, self pairs included."""
        out = C.c_uint64()
        return int(out.value) if load().sg_routing_info_smallest_latency(self.handle, C.byref(out)) else None

    # -- WorkerShared lookups (worker.rs:517-555), addresses as host-order u32 ----
    def set_addresses(self, ipv4: Sequence[int], node_ids: Sequence[int]) -> None:
        ips = np.ascontiguousarray(ipv4, np.uint32)
        ids = np.ascontiguousarray(node_ids, np.uint32)
        rc = load().sg_routing_info_set_addresses(self.handle, len(ips), ips.ctypes.data, ids.ctypes.data)
        if rc != _capi.SG_OK:
            raise ShadowGpuError(rc, "IP address has already been assigned")

    @staticmethod
    def _be(ip: int) -> int:
        return int.from_bytes(int(ip).to_bytes(4, "big"), "little")  # in_addr_t: network byte order

    def latency(self, src_ip: int, dst_ip: int) -> Optional[int]:
        out = C.c_uint64()
        rc = load().sg_worker_get_latency(self.handle, self._be(src_ip), self._be(dst_ip), C.byref(out))
        return int(out.value) if rc == _capi.SG_OK else None

    def reliability(self, src_ip: int, dst_ip: int) -> Optional[np.float32]:
        out = C.c_float()
        rc = load().sg_worker_get_reliability(self.handle, self._be(src_ip), self._be(dst_ip), C.byref(out))
        return np.float32(out.value) if rc == _capi.SG_OK else None

    def is_routable(self, src_ip: int, dst_ip: int) -> bool:
        return bool(load().sg_worker_is_routable(self.handle, self._be(src_ip), self._be(dst_ip)))


def generate_routing_info(graph: NetworkGraph, node_ids: Iterable[int], use_shortest_paths: bool) -> RoutingInfo:
    """sim_config.rs:411-448: used GML ids -> petgraph indices, build straight into
    the dense host RoutingInfo keyed by the ids (no HashMap, no remap pass)."""
    ids = list(node_ids)
    idx = []
    for x in ids:
        i = graph.node_id_to_index(x)
        if i is None:
            raise KeyError(f"node id {x} not in graph")
        idx.append(i)
    # an id that maps to an index twice collapses in the reference's HashMap; ids are unique here
    ri = RoutingInfo([graph.node_index_to_id(i) for i in idx])
    try:
        ri.fill(graph, idx, use_shortest_paths)
    except ShadowGpuError as e:
        what = "shortest paths" if use_shortest_paths else "the direct paths"
        raise ShadowGpuError(e.code, f"Failed to compute {what} between graph nodes: {e}", e.pair) from None
    return ri


# ---------------------------------------------------------------------------
# IpAssignment (graph/mod.rs:352-430)
# ---------------------------------------------------------------------------
def ipv4_to_u32(s: str) -> int:
    a, b, c, d = (int(x) for x in s.split("."))
    return (a << 24) | (b << 16) | (c << 8) | d


def u32_to_ipv4(x: int) -> str:
    return f"{(x >> 24) & 255}.{(x >> 16) & 255}.{(x >> 8) & 255}.{x & 255}"


class IpAssignment:
    def __init__(self):
        self.map: Dict[int, int] = {}
        self.last_assigned_addr = ipv4_to_u32("11.0.0.0")

    @staticmethod
    def increment_address(addr: int) -> int:
        inc = 1
        while True:
            nxt = (addr + inc) & 0xFFFFFFFF
            if (nxt & 0xFF) in (0, 255):  # skip .0 and .255 (graph/mod.rs:414-417)
                inc += 1
                continue
            return nxt

    def assign(self, node_id: int) -> int:
        while True:
            ip = self.increment_address(self.last_assigned_addr)
            self.last_assigned_addr = ip
            if ip not in self.map:
                self.map[ip] = node_id
                return ip

    def assign_ip(self, node_id: int, ip: int) -> None:
        if ip in self.map:
            raise ShadowGpuError(_capi.SG_ERR_DUPLICATE_IP, "IP address has already been assigned")
        self.map[ip] = node_id

    def get_node(self, ip: int) -> Optional[int]:
        return self.map.get(ip)

    def get_nodes(self) -> set:
        return set(self.map.values())
