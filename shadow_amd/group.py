"""A device group: N contexts of one process (sg_group_*, csrc/sg_group.hip).

Shadow is one process whose Manager owns every host (manager.rs:254-261); the sharded paths of
shadow_amd.dist assume one process per GPU and RCCL between them.  A `Group` binds N `Context`s
of the calling process instead -- usually one per GPU; all on device 0 works too and is what the
tests use -- and "member m" plays the part "rank m" plays there:

    ctxs = [Context(d) for d in range(n_gpus)]
    group = Group(ctxs)
    graphs = [NetworkGraph(..., ctx=c) for c in ctxs]             # the same graph on every member
    routing = group.fill_routing_info(graphs, used_ids)            # one host RoutingInfo, N links
    gd = GroupDelivery(group, hosts, tables, partition, padded=True)
    gd.round(batches, round_end, sim_end, wires=wires, lengths=lengths)   # every member's round

`Group.exchange_padded` / `Group.alltoallv_records` are the round's exchange inside the process
(a pull kernel per owner, device copies for the exact form), ordered against the members' streams
by events; nothing is synchronised and no count leaves the device.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _capi
from ._capi import ShadowGpuError, load
from .dist import (HostPartition, SourceResult, Workspace, _stream_wait, gpu_bucket_phase, gpu_bucket_phase_padded,
                   gpu_pad_to_compact, gpu_source_phase, gpu_source_phase_padded, next_cap)
from .graph import Context, NetworkGraph, RoutingInfo
from .round_args import concat_weights, int_tensor, member_weights, series_out, watch_mask, with_capacity

GROUP_MAX = 64  # members of one group (sg_group_create)


def _ptrs(tensors) -> C.Array:
    """An array of device pointers, one per member (None: NULL)."""
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class Group:
    """N contexts of this process as one object (sg_group).  The contexts must outlive it."""

    def __init__(self, contexts: Sequence[Context]):
        self.contexts = list(contexts)
        n = len(self.contexts)
        arr = (C.c_void_p * max(n, 1))(*[getattr(c.handle, "value", c.handle) for c in self.contexts])
        h = C.c_void_p()
        rc = load().sg_group_create(arr, n, C.byref(h))
        if rc != _capi.SG_OK:
            why = (load().sg_group_last_error(None) or b"").decode(errors="replace")
            raise ShadowGpuError(rc, why or f"sg_group_create failed with status {rc}")
        self.handle = h

    def __len__(self) -> int:
        return int(load().sg_group_size(self.handle)) if self.handle else 0

    def _check(self, rc: int) -> None:
        if rc == _capi.SG_OK:
            return
        L = load()
        msg = (L.sg_group_last_error(self.handle) or b"").decode(errors="replace")
        r, c = C.c_uint32(), C.c_uint32()
        L.sg_group_last_error_pair(self.handle, C.byref(r), C.byref(c))
        raise ShadowGpuError(rc, msg or f"status {rc}", (r.value, c.value))

    def close(self) -> None:
        if getattr(self, "handle", None):
            load().sg_group_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- start-up: one host RoutingInfo from all members ------------------------------------
    def fill(self, ri: RoutingInfo, graphs: Sequence[NetworkGraph], nodes: Sequence[int],
             flags: int = _capi.SG_ROUTE_SHORTEST_PATH) -> None:
        """sg_group_routing_info_fill into an existing RoutingInfo: graphs[m] is the graph on member
        m's context, nodes the petgraph indices of ri's node ids.  Member m builds and copies the
        rows dist.row_range(ri.n, len(group), m), all members at once."""
        if len(graphs) != len(self.contexts):
            raise ValueError(f"{len(graphs)} graphs for {len(self.contexts)} members")
        idx = np.ascontiguousarray(nodes, dtype=np.uint32)
        assert len(idx) == ri.n
        nets = (C.c_void_p * len(graphs))(*[g._ensure_net().value for g in graphs])
        self._check(load().sg_group_routing_info_fill(self.handle, nets, idx.ctypes.data, int(flags), ri.handle))

    def fill_routing_info(self, graphs: Sequence[NetworkGraph], node_ids: Sequence[int],
                          flags: int = _capi.SG_ROUTE_SHORTEST_PATH) -> RoutingInfo:
        """generate_routing_info (sim_config.rs:411-448) on all members: the used GML ids -> one
        dense host RoutingInfo keyed by them."""
        idx = []
        for x in node_ids:
            i = graphs[0].node_id_to_index(x)
            if i is None:
                raise KeyError(f"node id {x} not in graph")
            idx.append(i)
        ri = RoutingInfo([graphs[0].node_index_to_id(i) for i in idx])
        self.fill(ri, graphs, idx, flags)
        return ri

    # -- the round's exchange -----------------------------------------------------------------
    def exchange_padded(self, send_padded, recv_padded, cap: int, xrow, xall) -> None:
        """sg_group_exchange_padded: lists of one device tensor per member (records as int64
        [n * cap, 4]; xrow int64 [3 + n]; xall int64 [n * (3 + n)]).  Enqueued on the members'
        streams; does not synchronise."""
        n = len(self.contexts)
        for name, lst in (("send_padded", send_padded), ("recv_padded", recv_padded), ("xrow", xrow), ("xall", xall)):
            if len(lst) != n:
                raise ValueError(f"{name}: {len(lst)} tensors for {n} members")
        for s, r in zip(send_padded, recv_padded):
            if cap and (s.numel() < n * cap * 4 or r.numel() < n * cap * 4):
                raise ValueError("a record buffer holds fewer than members x cap records")
        for a, b in zip(xrow, xall):
            if a.numel() < 3 + n or b.numel() < n * (3 + n):
                raise ValueError("xrow holds 3 + n words, xall n x (3 + n)")
        self._check(load().sg_group_exchange_padded(self.handle, _ptrs(send_padded), _ptrs(recv_padded), int(cap),
                                                    _ptrs(xrow), _ptrs(xall)))

    def alltoallv_records(self, send, counts, recv) -> None:
        """sg_group_alltoallv_records: counts[b][r] = records member b holds for member r (host);
        send[b] grouped by r, recv[r] receives them source after source.  Does not synchronise."""
        n = len(self.contexts)
        cnt = np.ascontiguousarray(counts, dtype=np.uint32).reshape(n, n)
        for m in range(n):
            if (send[m] is None or send[m].numel() < int(cnt[m].sum()) * 4) and cnt[m].sum():
                raise ValueError(f"send[{m}] holds fewer records than its counts")
            if (recv[m] is None or recv[m].numel() < int(cnt[:, m].sum()) * 4) and cnt[:, m].sum():
                raise ValueError(f"recv[{m}] holds fewer records than its counts")
        self._check(load().sg_group_alltoallv_records(self.handle, _ptrs(send), cnt.ctypes.data, _ptrs(recv)))

    # -- a sharded round's link loads and link trace ------------------------------------------
    def last_error_member(self) -> int | None:
        """The member whose device-found error the last call reported (sg_group_last_error_member)."""
        m = int(load().sg_group_last_error_member(self.handle))
        return None if m == 0xFFFFFFFF else m

    def _round_inputs(self, graphs, hosts, rows, packets, status, need_latency):
        """The per-member arguments both calls share.  rows: a PathTree over all the group's
        source rows (member m takes rows dist.row_range(tree.n_sources, n, m), uploaded to its
        device), or (nodes, [(row_begin, row_end, pred, latency_ns or None), ...]) with one entry
        per member of device tensors on that member's device.  Returns the C arguments and what
        they point into."""
        import torch

        from .dist import row_range

        n = len(self.contexts)
        for name, lst in (("graphs", graphs), ("hosts", hosts), ("packets", packets)):
            if len(lst) != n:
                raise ValueError(f"{name}: {len(lst)} entries for {n} members")
        devs = [torch.device("cuda", c.device) for c in self.contexts]
        if isinstance(rows, (tuple, list)):
            nodes, blocks = rows
            if len(blocks) != n:
                raise ValueError(f"rows: {len(blocks)} blocks for {n} members")
            blocks = [(int(b[0]), int(b[1]), b[2], b[3] if len(b) > 3 else None) for b in blocks]
        else:  # a PathTree
            nodes, blocks = rows.nodes, []
            for m in range(n):
                r0, r1, _ = row_range(rows.n_sources, n, m)
                pred = torch.from_numpy(np.ascontiguousarray(rows.pred[r0:r1], dtype=np.uint32).view(np.int32)).to(devs[m])
                lat = None
                if need_latency:
                    lat = torch.from_numpy(np.ascontiguousarray(rows.latency_ns[r0:r1], dtype=np.uint64).view(np.int64)).to(devs[m])
                blocks.append((r0, r1, pred, lat))
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        for m, (r0, r1, pred, lat) in enumerate(blocks):
            cells = (r1 - r0) * len(nodes)
            if r1 > r0 and (pred is None or pred.numel() < cells or (need_latency and (lat is None or lat.numel() < cells))):
                raise ValueError(f"rows[{m}]: {r1 - r0} rows of {len(nodes)} cells")
        st = [None] * n
        if status is not None:
            if len(status) != n:
                raise ValueError(f"status: {len(status)} entries for {n} members")
            for m, s in enumerate(status):
                if s is not None:
                    st[m] = int_tensor(s, np.uint8, len(packets[m]), devs[m], f"status[{m}]", "status")
        pk = (_capi.sg_packets * n)(*[p.c_struct() for p in packets])
        u32s = lambda v: (C.c_uint32 * n)(*v)  # noqa: E731
        args = dict(nets=(C.c_void_p * n)(*[g._ensure_net().value for g in graphs]),
                    hosts=(C.c_void_p * n)(*[getattr(h.handle, "value", h.handle) for h in hosts]),
                    nodes=nodes, row_begin=u32s([b[0] for b in blocks]), row_end=u32s([b[1] for b in blocks]),
                    pred=_ptrs([b[2] for b in blocks]), lat=_ptrs([b[3] for b in blocks]), packets=pk,
                    status=None if status is None else _ptrs(st))
        for d in devs:  # what wrote the inputs on torch's streams
            torch.cuda.synchronize(d)
        return args, devs, (blocks, st)

    def link_load_round(self, graphs, hosts, rows, packets, status=None, weight=None, root: int = 0):
        """(link_load, node_load, hops) of one sharded round: PathTree.link_load_round over every
        member's batch at once (sg_group_link_load_packets).  graphs[m], hosts[m], packets[m]
        (a PacketBatch of member m's own sources) and status[m] (or None) live on member m's
        context; rows as in _round_inputs; weight: None (1 per packet), "payload", or one u32
        array per member.  link_load and node_load (u64, summed over the members on member
        `root`'s device) equal the single call's on the concatenated batch; hops is one u32 array
        per member."""
        import torch

        a, devs, keep = self._round_inputs(graphs, hosts, rows, packets, status, False)
        wt = member_weights(weight, packets, devs)
        if wt is not None:
            for d in devs:
                torch.cuda.synchronize(d)
        n_links = len(graphs[root].links()[0])
        link = torch.zeros(max(n_links, 1), dtype=torch.int64, device=devs[root])
        node = torch.zeros(max(len(a["nodes"]), 1), dtype=torch.int64, device=devs[root])
        hops = [torch.zeros(max(len(p), 1), dtype=torch.int32, device=d) for p, d in zip(packets, devs)]
        for d in devs:
            torch.cuda.synchronize(d)
        self._check(load().sg_group_link_load_packets(
            self.handle, a["nets"], a["hosts"], a["nodes"].ctypes.data, len(a["nodes"]), a["row_begin"], a["row_end"],
            a["pred"], a["packets"], a["status"], None if wt is None else _ptrs(wt), int(root), link.data_ptr(),
            node.data_ptr(), _ptrs(hops)))
        for c in self.contexts:
            c.synchronize()
        del keep
        return (link.cpu().numpy().view(np.uint64)[:n_links], node.cpu().numpy().view(np.uint64)[:len(a["nodes"])],
                [h.cpu().numpy().view(np.uint32)[:len(p)] for h, p in zip(hops, packets)])

    def link_trace_round(self, graphs, hosts, rows, packets, status=None, watch=None, root: int = 0):
        """The link trace of one sharded round, (link_off, packet, member, hop, enter_ns, exit_ns):
        PathTree.link_trace_round over every member's batch, the members' records merged on member
        `root`'s device (sg_group_link_trace_packets).  Link L owns records link_off[L] ..
        link_off[L + 1] in ascending (enter_ns, member, member-local packet) order; packet is the
        index in the members' batches concatenated in member order, member the batch it came from.
        rows needs the latency rows; watch as in PathTree.link_trace_round.  A first call at a
        guessed capacity, a second at the total the first reported when that was too small."""
        return self._trace_to_host(*self._link_trace_tensors(graphs, hosts, rows, packets, status, watch, root))

    @staticmethod
    def _trace_to_host(off, pkt, mem, hop, enter, leave, t):
        return (off.cpu().numpy().view(np.uint64), pkt[:t].cpu().numpy().view(np.uint32), mem[:t].cpu().numpy(),
                hop[:t].cpu().numpy().view(np.uint32), enter[:t].cpu().numpy().view(np.uint64),
                leave[:t].cpu().numpy().view(np.uint64))

    def _link_trace_tensors(self, graphs, hosts, rows, packets, status, watch, root):
        """link_trace_round's arrays as they lie on root's device, and the record total."""
        import torch

        a, devs, keep = self._round_inputs(graphs, hosts, rows, packets, status, True)
        n_links = len(graphs[root].links()[0])
        watch = watch_mask(watch, n_links)
        d = devs[root]
        off = torch.zeros(n_links + 1, dtype=torch.int64, device=d)
        total = C.c_uint64()

        def alloc(cap):  # (pkt, hop, mem, enter, leave)
            return [torch.zeros(cap, dtype=dt, device=d) for dt in (torch.int32, torch.int32, torch.uint8, torch.int64, torch.int64)]

        def call(arrays, cap):
            pkt, hop, mem, enter, leave = arrays
            torch.cuda.synchronize(d)
            rc = load().sg_group_link_trace_packets(
                self.handle, a["nets"], a["hosts"], a["nodes"].ctypes.data, len(a["nodes"]), a["row_begin"], a["row_end"],
                a["pred"], a["lat"], a["packets"], a["status"], None if watch is None else watch.ctypes.data, None,
                int(root), off.data_ptr(), pkt.data_ptr(), mem.data_ptr(), hop.data_ptr(), enter.data_ptr(),
                leave.data_ptr(), cap, C.byref(total))
            return rc, total.value

        rc, t, (pkt, hop, mem, enter, leave) = with_capacity(sum(len(p) for p in packets), alloc, call)
        self._check(rc)
        del keep
        return off, pkt, mem, hop, enter, leave, t

    def link_queue_round(self, graphs, hosts, rows, packets, status=None, weight=None, *, cost_ps, watch=None,
                         free_ns=None, root: int = 0, carry=False, limit_ns=None, outcomes=None, series=None):
        """The link trace of one sharded round and the FIFO queue of every link under a link rate,
        (link_off, packet, member, hop, enter_ns, exit_ns, queue): the first six as
        link_trace_round gives them, queue a graph.LinkQueueResult over the same records
        (PathTree.link_queue_round for a group).  The merged trace stays on member `root`'s device,
        where sg_link_queue runs on root's context with the members' weights concatenated in
        member order, as the trace's packet numbers are.  weight: None, "payload" or one u32
        array per member (as in link_load_round); cost_ps, free_ns as in shadow_amd.link_queue.
        carry=True: every wait is carried to the packet's later hops (SG_LINK_QUEUE_CARRY), on
        root's merged trace as well; queue is then a graph.LinkQueueCarried, and the carried
        exit_ns per record follows it (PathTree.link_queue_round).
        limit_ns: one u64 per link, the longest wait its buffer holds (SG_LINK_QUEUE_DROP), on
        root's merged trace as well; queue is then a graph.LinkQueueDropped or
        graph.LinkQueueCarriedDropped (PathTree.link_queue_round).
        outcomes: one Deliveries, or u64 array or tensor of base times, per member
        (SG_LINK_QUEUE_PACKETS); they are concatenated in member order on root's device, as the
        packet numbers are, and a graph.PacketOutcomes over all members' packets is the tuple's
        last entry (PathTree.link_queue_round).
        series: a LinkQueueSeries on root's device (SG_LINK_QUEUE_SERIES): the round's busy time, waiting
        time, weight served and weight dropped per slot and time bin are added into its matrix there."""
        import torch

        from .link_queue import _base_times, _exit_carried, _link_queue_tensors

        tr = self._link_trace_tensors(graphs, hosts, rows, packets, status, watch, root)
        off, pkt, _, _, enter, _, t = tr
        dev = off.device
        # (every member's weights straight onto root's device, where the queue runs)
        wt = concat_weights(member_weights(weight, packets, [dev] * len(packets)), packets, dev)
        npk = sum(len(p) for p in packets)
        base, tails = None, ()
        if outcomes is not None:
            if len(outcomes) != len(packets):
                raise ValueError(f"outcomes: {len(outcomes)} entries for {len(packets)} members")
            parts = [_base_times(o, len(packets[m]), dev, f"outcomes[{m}]") for m, o in enumerate(outcomes)]
            base = torch.cat(parts).contiguous() if parts else torch.zeros(0, dtype=torch.int64, device=dev)
            if enter.numel() < t + npk:  # (room for the base times behind the records)
                enter = torch.cat([enter[:t], torch.zeros(npk, dtype=torch.int64, device=dev)])
        queue = _link_queue_tensors(self.contexts[root], dev, off.numel() - 1, off, t, enter, pkt, wt, cost_ps, free_ns,
                                    carry, npk, limit_ns, base, series)
        if base is not None:
            queue, tails = queue[0], (queue[1],)
        host = self._trace_to_host(*tr)
        return (host + (queue, _exit_carried(host[5], host[4], queue)) if carry else host + (queue,)) + tails

    def link_series_round(self, graphs, hosts, rows, packets, status=None, weight=None, *, t0_ns: int, bin_ns: int,
                          n_bins: int, slots=None, at: str = "enter", out=None, root: int = 0):
        """The link time series of one sharded round, (series, outside): PathTree.link_series_round
        over every member's batch at once, the members' sums added on member `root`'s device
        (sg_group_link_series_packets).  graphs, hosts, rows (with the latency rows), packets and
        status as in link_trace_round, weight as in link_load_round; t0_ns, bin_ns, n_bins, slots,
        at and out as in PathTree.link_series_round.  Equals the single call on the concatenated
        batch."""
        import torch

        from .link_queue import series_slots

        if at not in ("enter", "exit"):
            raise ValueError('at: "enter" or "exit"')
        a, devs, keep = self._round_inputs(graphs, hosts, rows, packets, status, True)
        wt = member_weights(weight, packets, devs)
        n_links = len(graphs[root].links()[0])
        slot_map, n_slots = series_slots(slots, n_links)
        n_bins = int(n_bins)
        if out is not None:
            # (a view that is not contiguous passes here: it is copied in below and written back at the end)
            series, outside = series_out(out, n_slots, n_bins, contiguous=False)
            d_series = torch.from_numpy(np.ascontiguousarray(series).view(np.int64)).to(devs[root])
            d_out = torch.from_numpy(np.ascontiguousarray(outside).view(np.int64)).to(devs[root])
        else:
            d_series = torch.zeros((n_slots, max(n_bins, 1)), dtype=torch.int64, device=devs[root])
            d_out = torch.zeros((n_slots, 2), dtype=torch.int64, device=devs[root])
        for d in devs:
            torch.cuda.synchronize(d)
        self._check(load().sg_group_link_series_packets(
            self.handle, a["nets"], a["hosts"], a["nodes"].ctypes.data, len(a["nodes"]), a["row_begin"], a["row_end"],
            a["pred"], a["lat"], a["packets"], a["status"], None if wt is None else _ptrs(wt),
            None if slot_map is None else slot_map.ctypes.data, n_slots, 0 if at == "enter" else 1, int(t0_ns),
            int(bin_ns), n_bins, int(root), d_series.data_ptr(), d_out.data_ptr()))
        del keep
        got = (d_series.cpu().numpy().view(np.uint64).reshape(n_slots, -1)[:, :n_bins],
               d_out.cpu().numpy().view(np.uint64).reshape(n_slots, 2))
        if out is None:
            return got
        series[...], outside[...] = got
        return series, outside


class GroupDelivery:
    """The single-process driver of a sharded delivery round: dist.ShardedDelivery.round for all
    members of a group at once, with the group's exchange in place of the collectives.

    hosts[m] / tables[m]: member m's HostTable and its DeviceTable shard (rows
    dist.row_range(n_used, n, m)), both on member m's context; partition: the HostPartition over n
    members.  A round runs the source phase on every member, one exchange, and on every owner either
    the bucketing or -- with `wires` -- the wire's push (stamp -> exchange -> push -> the caller's
    pop).  Its three modes are ShardedDelivery's: "exact" (the first round, or padded=False),
    "padded", and "padded+exact" when a pair count outgrew the block (pair_max > cap): all members
    then exchange again exactly through alltoallv_records."""

    def __init__(self, group: Group, hosts, tables, partition: HostPartition, padded: bool = False):
        import torch

        n = len(group.contexts)
        if not (len(hosts) == len(tables) == n == partition.world):
            raise ValueError("one HostTable and one DeviceTable per member, and a partition over the members")
        self.group, self.hosts, self.tables, self.part, self.padded = group, list(hosts), list(tables), partition, padded
        self.n = n
        self.ws = [Workspace() for _ in range(n)]
        self.devices = [torch.device("cuda", c.device) for c in group.contexts]
        self.owner_dev = [torch.from_numpy(partition.owner.view(np.int32)).to(d) for d in self.devices]
        self.local_dev = [torch.from_numpy(partition.local.view(np.int32)).to(d) for d in self.devices]
        self.cap = None        # block size of the next padded round (None: the next round is exact)
        self.last_mode = None  # "exact", "padded" or "padded+exact"
        self.last_stats = None
        self.last_counts = None  # the round's n x n matrix: records member b sent member r

    # the members' streams against torch's current stream (which wrote the inputs / reads the outputs)
    def _join_in(self) -> None:
        import torch

        for c, d in zip(self.group.contexts, self.devices):
            _stream_wait(int(c.stream), int(torch.cuda.current_stream(d).cuda_stream))

    def _join_out(self) -> None:
        import torch

        for c, d in zip(self.group.contexts, self.devices):
            _stream_wait(int(torch.cuda.current_stream(d).cuda_stream), int(c.stream))

    def _synchronize(self) -> None:
        for c in self.group.contexts:
            c.synchronize()

    def _wire_map(self, wire, m):
        if wire.n == len(self.part.local):
            return None
        if wire.n == self.part.n_local(m):
            return self.local_dev[m]
        raise ValueError(f"member {m}'s wire holds {wire.n} hosts: neither all {len(self.part.local)} nor its own "
                         f"{self.part.n_local(m)}")

    def round(self, packets, round_end_ns: int, sim_end_ns: int, bootstrap_end_ns: int = 0, wires=None, lengths=None,
              packet_ids=None, id_bases=0):
        """One round of every member.  packets[m]: member m's PacketBatch.  Without wires returns,
        per member, (source result, recv, recv_counts, order, offsets) as ShardedDelivery.round;
        with wires[m] (a PacketWire on member m's context; lengths[m] int32 device tensor,
        packet_ids[m] or None, id_bases an int or one per member) returns per member (source result,
        recv_counts, stats) and the arrivals come out of wires[m].pop, which also raises a padded
        source phase's batch error of that member."""
        n = self.n
        if len(packets) != n:
            raise ValueError(f"{len(packets)} batches for {n} members")
        if wires is not None and lengths is None:
            raise ValueError("round(wires=...) needs lengths")
        ids = list(packet_ids) if packet_ids is not None else [None] * n
        bases = list(id_bases) if isinstance(id_bases, (list, tuple)) else [int(id_bases)] * n
        self._join_in()
        clock = (round_end_ns, sim_end_ns, bootstrap_end_ns)
        if self.padded and self.cap is not None:
            out = self._round_padded(packets, clock, wires, lengths, ids, bases)
        else:
            out = self._round_exact(packets, clock, wires, lengths, ids, bases)
            if self.padded:  # the first round sizes the blocks
                self.cap = next_cap(int(self.last_counts.max()))
        self._join_out()
        return out

    def _exchange_exact(self, sends, counts):
        import torch

        recv = [self.ws[m].get("x_recv", max(int(counts[:, m].sum()), 1), torch.int64, self.devices[m], cols=4)
                for m in range(self.n)]
        self.group.alltoallv_records(sends, counts, recv)
        return recv

    def _owner_phase(self, m, recv, n_records, wires):
        """The destination half on member m for a compact `recv`: the wire's push, or the bucketing."""
        c = self.group.contexts[m]
        if wires is not None:
            wires[m].push_records(recv, n_records, self._wire_map(wires[m], m))
            return None
        return gpu_bucket_phase(c, recv, n_records, self.local_dev[m], len(self.part.local), self.part.n_local(m),
                                ws=self.ws[m])

    def _round_exact(self, packets, clock, wires, lengths, ids, bases):
        from . import wire as _wire

        n, ctxs = self.n, self.group.contexts
        self.last_mode = "exact"
        srcs = [gpu_source_phase(ctxs[m], self.hosts[m], self.tables[m], packets[m], *clock, self.owner_dev[m], n,
                                 ws=self.ws[m]) for m in range(n)]
        counts = np.array([s.send_counts for s in srcs], dtype=np.int64).reshape(n, n)
        if wires is not None:
            for m, s in enumerate(srcs):
                _wire.stamp_records(s.send, int(counts[m].sum()), lengths[m], len(packets[m]), ids[m], bases[m],
                                    ctx=ctxs[m])
        recv = self._exchange_exact([s.send for s in srcs], counts)
        self.last_counts = counts
        self.last_stats = (int(sum(s.n_delivered for s in srcs)), int(min(s.min_deliver_time_ns for s in srcs)),
                           int(min(s.min_used_latency_ns for s in srcs)))
        out = []
        for m in range(n):
            rc = [int(x) for x in counts[:, m]]
            res = self._owner_phase(m, recv[m], sum(rc), wires)
            out.append((srcs[m], rc, self.last_stats) if wires is not None else (srcs[m], recv[m][:sum(rc)], rc, *res))
        return out

    def _round_padded(self, packets, clock, wires, lengths, ids, bases):
        import torch

        from . import wire as _wire

        n, ctxs, cap = self.n, self.group.contexts, self.cap
        srcs = [gpu_source_phase_padded(ctxs[m], self.hosts[m], self.tables[m], packets[m], *clock,
                                        self.owner_dev[m], n, cap, ws=self.ws[m]) for m in range(n)]
        if wires is not None:
            for m, s in enumerate(srcs):
                _wire.stamp_records_padded(s.send_padded, s.send, n, cap, s.xrow, lengths[m], len(packets[m]), ids[m],
                                           bases[m], ctx=ctxs[m])
        recv = [self.ws[m].get("recv_padded", n * cap, torch.int64, self.devices[m], cols=4) for m in range(n)]
        xall = [self.ws[m].get("xall", n * (3 + n), torch.int64, self.devices[m]) for m in range(n)]
        self.group.exchange_padded([s.send_padded for s in srcs], recv, cap, [s.xrow for s in srcs], xall)
        bucketed = [None] * n
        for m in range(n):
            if wires is not None:  # appends nothing if the round overflowed
                wires[m].push_records_padded(recv[m], n, cap, xall[m], m, self._wire_map(wires[m], m))
            else:  # synchronises member m and raises its source phase's batch error
                bucketed[m] = gpu_bucket_phase_padded(ctxs[m], recv[m], cap, xall[m], m, self.local_dev[m],
                                                      len(self.part.local), self.part.n_local(m), ws=self.ws[m])
        # The gathered [stats, counts] rows, n x (3 + n) words: all this round copies to the host
        # (every member holds the same rows; the C loop of INTEGRATION 2.8 reads them after the pop).
        self._synchronize()
        xa = xall[0].cpu().numpy().view(np.uint64).reshape(n, 3 + n)
        counts = xa[:, 3:].astype(np.int64)
        pair_max = int(counts.max())
        self.last_counts = counts
        self.last_stats = (int(xa[:, 0].sum()), int(xa[:, 1].min()), int(xa[:, 2].min()))
        self.cap = next_cap(pair_max)
        overflow = pair_max > cap
        self.last_mode = "padded+exact" if overflow else "padded"
        if overflow:  # some pair outgrew its block: every member exchanges again, exactly
            sends = [gpu_pad_to_compact(ctxs[m], srcs[m], n) for m in range(n)]
            xrecv = self._exchange_exact(sends, counts)
        out = []
        for m in range(n):
            rc = [int(x) for x in counts[:, m]]
            res = SourceResult(srcs[m].status, srcs[m].deliver_time_ns, srcs[m].event_id,
                               srcs[m].send if overflow else None, [int(x) for x in counts[m]], *self.last_stats,
                               send_padded=srcs[m].send_padded)
            if overflow:
                b = self._owner_phase(m, xrecv[m], sum(rc), wires)
                out.append((res, rc, self.last_stats) if wires is not None else (res, xrecv[m][:sum(rc)], rc, *b))
            elif wires is not None:
                out.append((res, rc, self.last_stats))
            else:
                order, offsets = bucketed[m][0], bucketed[m][1]
                out.append((res, recv[m], rc, order, offsets))
        return out


__all__ = ["Group", "GroupDelivery", "GROUP_MAX"]
