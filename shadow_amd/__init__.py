"""shadow_amd -- MI355X-native network core for the Shadow simulator.

Two stages of Shadow's network core run as HIP kernels for gfx950 behind the
C ABI in include/shadow_gpu.h (libshadow_gpu.so):

* routing-table build (NetworkGraph::compute_shortest_paths / get_direct_paths,
  src/main/network/graph/mod.rs:183-252) -> `graph.NetworkGraph`, with the paths' trees
  (`graph.PathTree`) and the traffic they carried per link (`PathTree.link_load` from per-pair
  counters, `PathTree.link_load_round` from a round's packets, `NetworkGraph.links`), and what
  a link rate would make each crossing wait (`link_queue`, `PathTree.link_queue_round`; the module
  link_queue.py, which the function of that name hides as an attribute here), also per link and
  time bin (`LinkQueueSeries`);
* per-round packet delivery (Worker::send_packet, src/main/core/worker.rs:322-397)
  -> `worker.deliver_round`;
* the packets in flight between a delivery round and their arrival (the per-host
  EventQueue, worker.rs:597-607 / host.rs:753-757) -> `wire.PacketWire`.

There is no CPU fallback: if libshadow_gpu.so is missing, `load()` raises.
"""
from ._capi import LIB_PATH, ShadowGpuError, ShadowGpuUnavailable, load  # noqa: F401
from .graph import (Context, IpAssignment, LinkQueueCarried, LinkQueueCarriedDropped, LinkQueueDropped, LinkQueueResult, NetworkGraph, PacketOutcomes, PathProperties, PathTable,  # noqa: F401
                    PathTree, RoutingInfo, cost_ps_from_bandwidth, default_context, generate_routing_info,
                    ipv4_to_u32, link_queue, link_queue_pending, queue_limit_ns, u32_to_ipv4,
                    WHERE_ARRIVED, WHERE_IN_FLIGHT, WHERE_NOTHING)
from .queue_session import LinkQueueSession, SettledPackets, SettledRecords  # noqa: F401
from .queue_series import LinkQueueSeries  # noqa: F401
from .wire import PacketWire  # noqa: F401
from .group import Group, GroupDelivery  # noqa: F401

__all__ = ["Context", "NetworkGraph", "PathProperties", "PathTable", "PathTree", "RoutingInfo", "IpAssignment",
           "generate_routing_info", "default_context", "load", "ShadowGpuError", "ShadowGpuUnavailable",
           "ipv4_to_u32", "u32_to_ipv4", "LIB_PATH", "PacketWire", "Group", "GroupDelivery", "LinkQueueResult", "LinkQueueCarried",
           "link_queue", "link_queue_pending", "LinkQueueSession", "SettledPackets", "SettledRecords", "WHERE_ARRIVED",
           "WHERE_IN_FLIGHT", "WHERE_NOTHING", "cost_ps_from_bandwidth", "LinkQueueDropped", "LinkQueueCarriedDropped", "queue_limit_ns",
           "PacketOutcomes", "LinkQueueSeries"]
