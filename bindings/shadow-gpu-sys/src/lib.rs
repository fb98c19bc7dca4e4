//! Raw bindings to `libshadow_gpu.so`, the MI355X network core for Shadow 3.2.0.
//!
//! Every declaration mirrors `include/shadow_gpu.h` (ABI 7) one to one: the 80 entry
//! points, the 17 `#[repr(C)]` structs, the opaque handles and the constants.
//! `tests/test_rust_binding_cpu.py` parses both files and fails on any difference in
//! names, argument counts, argument and field types, or constant values, and on any
//! export of the built library that this file does not declare.
//!
//! Conventions (as the header's): every fallible call returns an `i32` status
//! (`SG_OK` or `SG_ERR_*`, never unwinds); pointers the header documents as "device"
//! are HIP device pointers on the context's device, everything else is host memory.
//! The safe wrappers Shadow would use (`src/main/network/gpu.rs` in INTEGRATION.md)
//! sit on top of these and keep the reference's own types at their call sites:
//! `NetworkGraph` (`src/main/network/graph/mod.rs:116-252`), `RoutingInfo`
//! (`graph/mod.rs:432-481`), `Worker::send_packet` (`src/main/core/worker.rs:322-397`)
//! and the exported `worker_getLatency` / `worker_isRoutable`
//! (`worker.rs:619-684`, whose `extern "C-unwind"` conventions these follow in reverse:
//! plain integers and pointers, no Rust types across the boundary).
#![allow(non_camel_case_types)]
#![no_std]

use core::ffi::{c_char, c_void};

// ---------------------------------------------------------------------------
// Opaque handles
// ---------------------------------------------------------------------------
/// One HIP device, stream and workspace.
#[repr(C)]
pub struct sg_ctx {
    _private: [u8; 0],
}
/// A device-resident network graph (the petgraph `Graph` of `NetworkGraph`, graph/mod.rs:116-119).
#[repr(C)]
pub struct sg_net {
    _private: [u8; 0],
}
/// Device-resident host table: addresses, routes, Xoshiro streams, event-id counters.
#[repr(C)]
pub struct sg_hosts {
    _private: [u8; 0],
}
/// A host-side parsed GML graph (`NetworkGraph::parse`, graph/mod.rs:134-181).
#[repr(C)]
pub struct sg_gml {
    _private: [u8; 0],
}
/// The dense host-side `RoutingInfo<u32>` (graph/mod.rs:432-481).
#[repr(C)]
pub struct sg_routing_info {
    _private: [u8; 0],
}
/// One RCCL communicator bound to an `sg_ctx` (ABI 7).
#[repr(C)]
pub struct sg_comm {
    _private: [u8; 0],
}
/// N `sg_ctx` of this one process (the `Manager` owns them all) behind one object.
#[repr(C)]
pub struct sg_group {
    _private: [u8; 0],
}
/// Every host's in-flight Packet events (the per-host `EventQueue`, on the device).
#[repr(C)]
pub struct sg_wire {
    _private: [u8; 0],
}
/// Every host's router `CoDelQueue` (router/codel_queue.rs).
#[repr(C)]
pub struct sg_codel {
    _private: [u8; 0],
}
/// Router queue + `relay_inet_in` per host (relay/mod.rs:72-288).
#[repr(C)]
pub struct sg_inbound {
    _private: [u8; 0],
}
/// Interface FIFO + `relay_inet_out` per host (relay/mod.rs:111-275).
#[repr(C)]
pub struct sg_outbound {
    _private: [u8; 0],
}

// ---------------------------------------------------------------------------
// Structs
// ---------------------------------------------------------------------------
/// Edge list in GML edge order; node indices are petgraph `NodeIndex` values.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_graph {
    pub n_nodes: u32,
    pub n_edges: u32,
    pub edge_src: *const u32,
    pub edge_dst: *const u32,
    pub edge_latency_ns: *const u64,
    pub edge_packet_loss: *const f32,
    /// optional (null): GML ids, for messages
    pub node_gml_id: *const u32,
    pub directed: u8,
}

/// Zero-copy view of an `sg_routing_info`: cells `(latency_ns << 32) | bits(loss)`.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_routing_view {
    pub n: u32,
    pub node_ids: *const u32,
    pub cells: *const u64,
    pub n_wide: u64,
    pub pinned: u32,
}

/// A routing-table shard resident on the device (rows `[row_begin, row_begin + n_rows)`).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_table {
    pub latency_ns: *const u64,
    pub packet_loss: *const f32,
    pub n_cols: u32,
    pub row_begin: u32,
    pub n_rows: u32,
    /// null = the two-array form
    pub path_key: *const u64,
}

/// Round clock (EmulatedTime ns): the worker's barrier (worker.rs:262-268), sim end, bootstrap end.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct sg_round {
    pub round_end_ns: u64,
    pub sim_end_ns: u64,
    pub bootstrap_end_ns: u64,
}

/// One round's sent packets (device SoA, grouped by ascending source host, send order).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_packets {
    pub n_packets: u32,
    pub src_host: *const u32,
    pub dst_ipv4: *const u32,
    pub payload_len: *const u32,
    pub send_time_ns: *const u64,
    /// null = none: other consumers' steps of the host's RNG stream (host.rs:645-647)
    pub rng_skip: *const u32,
}

/// Device outputs of `sg_deliver_round`.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_deliveries {
    pub status: *mut u8,
    pub deliver_time_ns: *mut u64,
    pub event_id: *mut u64,
    pub dst_order: *mut u32,
    pub dst_offsets: *mut u32,
}

/// The round minima `Manager::run` folds (worker.rs:372,388).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct sg_round_stats {
    pub n_delivered: u64,
    pub min_deliver_time_ns: u64,
    pub min_used_latency_ns: u64,
}

/// One delivered packet on its way to the destination's owner rank (32 bytes).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct sg_record {
    pub deliver_time_ns: u64,
    /// (src_host << 32) | k, k = rank among src_host's delivered packets this round
    pub order_key: u64,
    pub event_id: u64,
    pub packet: u32,
    pub dst_host: u32,
}

/// A batch of CoDel push / pop events (device arrays, grouped by ascending host).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_codel_events {
    pub n_events: u32,
    pub host: *const u32,
    /// `SG_CODEL_PUSH` | `SG_CODEL_POP`
    pub kind: *const u8,
    pub time_ns: *const u64,
    pub packet: *const u32,
    pub len: *const u32,
}

/// Per-host CoDel state (host arrays) for checkpoints and tests.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_codel_state {
    pub flags: *mut u8,
    pub interval_end: *mut u64,
    pub drop_next: *mut u64,
    pub cur_drops: *mut u64,
    pub prev_drops: *mut u64,
    pub bytes: *mut u64,
    pub head: *mut u32,
    pub tail: *mut u32,
    pub ring_packet: *mut u32,
    pub ring_time: *mut u64,
    pub ring_len: *mut u32,
}

/// A window's Packet events (device arrays, grouped by ascending host, EventQueue order).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_inbound_arrivals {
    pub n: u32,
    pub host: *const u32,
    pub time_ns: *const u64,
    pub packet: *const u32,
    pub len: *const u32,
}

/// Per-host relay and token-bucket state (host arrays).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_inbound_relay_state {
    pub flags: *mut u8,
    pub task_time: *mut u64,
    pub cached_packet: *mut u32,
    pub cached_len: *mut u32,
    pub tb_capacity: *mut u64,
    pub tb_balance: *mut u64,
    pub tb_increment: *mut u64,
    pub tb_last_refill: *mut u64,
    /// ABI 6, may be null: the pending forward task's event id (host.rs:649-653)
    pub task_event_id: *mut u64,
    /// ABI 6, may be null: the time that task was scheduled at
    pub task_created_ns: *mut u64,
}

/// A window's sends (device arrays, grouped by ascending host, interface order).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_outbound_sends {
    pub n: u32,
    pub host: *const u32,
    pub time_ns: *const u64,
    pub packet: *const u32,
    pub len: *const u32,
    pub payload_len: *const u32,
    pub dst_ipv4: *const u32,
    /// ABI 6, optional (null, or both): the sending event's id (u64::MAX: a Packet event)
    pub event_id: *const u64,
    pub event_created_ns: *const u64,
}

/// The packets an outbound window handed to `send_packet` (a delivery round's `sg_packets`).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_outbound_sent {
    pub cap: u32,
    pub src_host: *mut u32,
    pub dst_ipv4: *mut u32,
    pub payload_len: *mut u32,
    pub send_time_ns: *mut u64,
    pub packet: *mut u32,
}

/// Per-host interface FIFO (host arrays); a cached packet is the slot at head - 1.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_outbound_queue_state {
    pub head: *mut u32,
    pub tail: *mut u32,
    pub ring_packet: *mut u32,
    pub ring_len: *mut u32,
    pub ring_payload_len: *mut u32,
    pub ring_dst: *mut u32,
}

/// A round-robin object's interfaces in canonical form (host arrays, any may be null): per host
/// the deque front to back with each socket's packet count, the queued packets socket by socket
/// in deque order, and the relay's cached packet.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_outbound_qdisc_state {
    pub n_active: *mut u32,
    pub active: *mut u32,
    pub active_count: *mut u32,
    pub n_queued: *mut u32,
    pub q_packet: *mut u32,
    pub q_len: *mut u32,
    pub q_payload_len: *mut u32,
    pub q_dst: *mut u32,
    pub cached_packet: *mut u32,
    pub cached_len: *mut u32,
    pub cached_payload_len: *mut u32,
    pub cached_dst: *mut u32,
}

/// A window's arrivals out of the wire (device arrays of capacity `cap`): the first four
/// arrays are an `sg_inbound_arrivals`; `src_host` / `event_id` both, or both null.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_wire_arrivals {
    pub cap: u32,
    pub host: *mut u32,
    pub time_ns: *mut u64,
    pub packet: *mut u32,
    pub len: *mut u32,
    pub src_host: *mut u32,
    pub event_id: *mut u64,
}

/// The wire's events (host arrays), in canonical order (host, time, src_host, event_id).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct sg_wire_state {
    pub host: *mut u32,
    pub src_host: *mut u32,
    pub packet: *mut u32,
    pub len: *mut u32,
    pub time_ns: *mut u64,
    pub event_id: *mut u64,
}

/// An `sg_record` after `sg_wire_stamp_records[_padded]`: same size, same offsets; the low half
/// of `order_key` carries `len`, `packet` the caller's packet id.  It travels through the
/// exchanges as an `sg_record`; never hand one to `sg_deliver_bucket[_padded]`.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct sg_wire_record {
    pub deliver_time_ns: u64,
    pub len: u32,
    pub src_host: u32,
    pub event_id: u64,
    pub packet_id: u32,
    pub dst_host: u32,
}

// ---------------------------------------------------------------------------
// Constants
// ---------------------------------------------------------------------------
/// Checked against `sg_abi_version()` at startup.
pub const SG_ABI_VERSION: i32 = 7;

// sg_status
pub const SG_OK: i32 = 0;
/// graph/mod.rs:266-268 "No edge connecting node {} to {}"
pub const SG_ERR_NO_EDGE: i32 = 1;
/// graph/mod.rs:269-275 "More than one edge connecting node {} to {}"
pub const SG_ERR_MULTI_EDGE: i32 = 2;
/// graph/mod.rs:219 (a panic in the reference)
pub const SG_ERR_UNREACHABLE: i32 = 3;
pub const SG_ERR_OOM: i32 = 4;
pub const SG_ERR_INVALID_ARG: i32 = 5;
pub const SG_ERR_DEVICE: i32 = 6;
/// NetworkGraph::parse / ShadowEdge::try_from (graph/mod.rs:72-181)
pub const SG_ERR_PARSE: i32 = 7;
pub const SG_ERR_UNSORTED: i32 = 8;
/// IpAssignment::assign_ip (graph/mod.rs:383-394)
pub const SG_ERR_DUPLICATE_IP: i32 = 9;
pub const SG_ERR_CAPACITY: i32 = 10;
/// EmulatedTime + SimulationTime past EMUTIME_MAX (a panic in the reference, emulated_time.rs:121-126)
pub const SG_ERR_TIME_OVERFLOW: i32 = 11;
/// sg_comm_*: RCCL could not be opened; sg_group_create: a pair of devices without peer access
pub const SG_ERR_UNSUPPORTED: i32 = 12;

/// sg_link_series_packets' `at`: the time of a crossing that chooses its bin
pub const SG_SERIES_AT_ENTER: u32 = 0;
pub const SG_SERIES_AT_EXIT: u32 = 1;
pub const SG_TIMERS_ON: u32 = 1;
pub const SG_TIMERS_COUNT_WORK: u32 = 2;
/// network.use_shortest_path (configuration.rs:315-326)
pub const SG_ROUTE_SHORTEST_PATH: u32 = 1;
pub const SG_ROUTE_OUT_DEVICE: u32 = 2;
/// sg_link_queue: carry each wait to the packet's later hops
pub const SG_LINK_QUEUE_CARRY: u32 = 4;
/// sg_link_queue: cost_ps carries a longest wait per link in its second half; tail drop
pub const SG_LINK_QUEUE_DROP: u32 = 8;
/// sg_link_queue: enter_ns and the per-record outputs carry n_weights packets behind the records:
/// each packet's base time in, its delay, arrival and the record that dropped it out
pub const SG_LINK_QUEUE_PACKETS: u32 = 16;
/// sg_link_queue: with SG_LINK_QUEUE_CARRY, link_free_in carries a horizon behind the links: records whose
/// carried enter time is below it are settled, the rest come back pending with their re-based times
pub const SG_LINK_QUEUE_WINDOW: u32 = 32;
/// sg_link_queue: cost_ps carries (t0_ns, bin_ns, n_bins, n_slots) and a slot per link behind its entries, and
/// out_link_busy_ns a matrix behind its own: busy time, waiting time, weight served and weight dropped per
/// slot and time bin, added on the device
pub const SG_LINK_QUEUE_SERIES: u32 = 64;
pub const SG_CELL_WIDE: u32 = 0xFFFF_FFFF;
pub const SG_COMM_ID_BYTES: usize = 128;

// sg_deliveries.status
pub const SG_PKT_DELIVERED: u8 = 0;
pub const SG_PKT_DROP_LOSS: u8 = 1;
pub const SG_PKT_DROP_NO_DST: u8 = 2;
pub const SG_PKT_SIM_END: u8 = 3;
// sg_codel_events.kind
pub const SG_CODEL_PUSH: u8 = 0;
pub const SG_CODEL_POP: u8 = 1;
// router / relay packet fates
pub const SG_CODEL_QUEUED: u8 = 0;
pub const SG_CODEL_DEQUEUED: u8 = 1;
/// PacketStatus::RouterDropped
pub const SG_CODEL_DROPPED: u8 = 2;
pub const SG_OUT_QUEUED: u8 = 0;
/// to the router: Worker::send_packet
pub const SG_OUT_SENT: u8 = 1;
/// dst == own address: back to the interface
pub const SG_OUT_LOCAL: u8 = 2;
/// experimental.interface_qdisc (QDiscMode, configuration.rs:971-973)
pub const SG_QDISC_FIFO: u32 = 0;
pub const SG_QDISC_ROUND_ROBIN: u32 = 1;
/// the most socket slots per host of a round-robin object
pub const SG_QDISC_MAX_SOCKETS: u32 = 256;

// ---------------------------------------------------------------------------
// Entry points (in the header's order)
// ---------------------------------------------------------------------------
unsafe extern "C" {
    pub fn sg_abi_version() -> i32;

    // ---- context -------------------------------------------------------------
    pub fn sg_ctx_create(device: i32, out: *mut *mut sg_ctx) -> i32;
    pub fn sg_ctx_destroy(ctx: *mut sg_ctx);
    /// An existing hipStream_t (e.g. the caller's), or null for the context's own stream.
    pub fn sg_ctx_set_stream(ctx: *mut sg_ctx, hip_stream: *mut c_void) -> i32;
    pub fn sg_ctx_stream(ctx: *const sg_ctx) -> *mut c_void;
    pub fn sg_ctx_synchronize(ctx: *mut sg_ctx) -> i32;
    pub fn sg_ctx_last_error(ctx: *const sg_ctx) -> *const c_char;
    pub fn sg_ctx_last_error_pair(ctx: *const sg_ctx, row: *mut u32, col: *mut u32);
    pub fn sg_ctx_enable_timers(ctx: *mut sg_ctx, enable: i32) -> i32;
    pub fn sg_ctx_read_timer(ctx: *mut sg_ctx, kernel: *const c_char, total_ms: *mut f64, launches: *mut u64,
                             work: *mut f64) -> i32;

    // ---- GML ingest: load_network_graph + NetworkGraph::parse (graph/mod.rs:134-181, 483-513) ----
    pub fn sg_gml_parse(text: *const c_char, len: usize, out: *mut *mut sg_gml, err: *mut c_char, err_len: usize)
        -> i32;
    pub fn sg_gml_parse_threads(text: *const c_char, len: usize, threads: u32, out: *mut *mut sg_gml,
                                err: *mut c_char, err_len: usize) -> i32;
    pub fn sg_gml_load(path: *const c_char, compression: u32, threads: u32, out: *mut *mut sg_gml, err: *mut c_char,
                       err_len: usize) -> i32;
    /// The parsed edge list, borrowed until sg_gml_destroy.
    pub fn sg_gml_graph(g: *const sg_gml, out: *mut sg_graph) -> i32;
    /// NetworkGraph::node_id_to_index (graph/mod.rs:126-128).
    pub fn sg_gml_node_index(g: *const sg_gml, gml_id: u32, out_index: *mut u32) -> i32;
    pub fn sg_gml_destroy(g: *mut sg_gml);

    // ---- routing-table build: compute_shortest_paths / get_direct_paths (graph/mod.rs:183-252) ----
    pub fn sg_net_create(ctx: *mut sg_ctx, g: *const sg_graph, out: *mut *mut sg_net) -> i32;
    pub fn sg_net_destroy(net: *mut sg_net);
    pub fn sg_routing_build(ctx: *mut sg_ctx, net: *mut sg_net, nodes: *const u32, n_used: u32, row_begin: u32,
                            row_end: u32, flags: u32, out_latency_ns: *mut u64, out_packet_loss: *mut f32) -> i32;
    /// RoutingInfo::get_smallest_latency_ns (graph/mod.rs:478-480) over device latencies.
    pub fn sg_routing_min_latency(ctx: *mut sg_ctx, d_latency_ns: *const u64, count: usize, out_min: *mut u64)
        -> i32;

    // ---- shortest-path trees: which links a path uses (graph/mod.rs:183-228, 322-331) ----
    /// pred / first_hop rows (petgraph indices) from finished table rows; `nodes` is a permutation.
    pub fn sg_routing_tree(ctx: *mut sg_ctx, net: *mut sg_net, nodes: *const u32, n_nodes: u32, row_begin: u32,
                           row_end: u32, flags: u32, latency_ns: *const u64, packet_loss: *const f32,
                           out_pred: *mut u32, out_first_hop: *mut u32) -> i32;
    /// sg_routing_build over those rows, then the tree pass; needs SG_ROUTE_SHORTEST_PATH.
    pub fn sg_routing_build_tree(ctx: *mut sg_ctx, net: *mut sg_net, nodes: *const u32, n_nodes: u32,
                                 row_begin: u32, row_end: u32, flags: u32, out_latency_ns: *mut u64,
                                 out_packet_loss: *mut f32, out_pred: *mut u32, out_first_hop: *mut u32) -> i32;
    /// Host only: the node sequence src ... dst from one host pred row (the row of `src`).
    pub fn sg_tree_path(pred_row: *const u32, nodes: *const u32, n_nodes: u32, src: u32, dst: u32,
                        out_path: *mut u32, cap: u32, len: *mut u32) -> i32;

    // ---- link loads: a per-pair u64 matrix folded onto the graph's links through pred rows ----
    /// The link list (distinct ordered node pairs joined by an edge), ascending (head, tail).
    pub fn sg_net_links(ctx: *mut sg_ctx, net: *mut sg_net, n_links: *mut u32, out_tail: *mut u32,
                        out_head: *mut u32, cap: u32) -> i32;
    /// Each edge's link numbers: (src -> dst), and (dst -> src) or u32::MAX on a directed graph.
    pub fn sg_net_edge_links(ctx: *mut sg_ctx, net: *mut sg_net, out_fwd: *mut u32, out_rev: *mut u32) -> i32;
    /// Adds rows [row_begin, row_end) of `counts` onto the links and nodes of their tree paths.
    pub fn sg_link_load(ctx: *mut sg_ctx, net: *mut sg_net, nodes: *const u32, n_nodes: u32, row_begin: u32,
                        row_end: u32, flags: u32, pred: *const u32, counts: *const u64, count_cols: u32,
                        out_link_load: *mut u64, out_node_load: *mut u64) -> i32;
    /// The same sums from one round's batch: every counted packet walks its tree path, adding its
    /// weight (1 when `weight` is null) to each link and node on it; `out_hops[p]` = its hop count.
    pub fn sg_link_load_packets(ctx: *mut sg_ctx, net: *mut sg_net, hosts: *mut sg_hosts, nodes: *const u32,
                                n_nodes: u32, row_begin: u32, row_end: u32, flags: u32, pred: *const u32,
                                packets: *const sg_packets, status: *const u8, weight: *const u32,
                                out_link_load: *mut u64, out_node_load: *mut u64, out_hops: *mut u32) -> i32;

    // ---- batched tree paths: hop records (node, link, cumulative latency and loss) in CSR ----
    /// The hop records of the pairs (pair_row[p], pair_col[p]), source to destination; pair p owns
    /// records [out_off[p], out_off[p + 1]).  SG_ERR_CAPACITY with out_off and *total complete
    /// when *total > cap.
    pub fn sg_tree_paths(ctx: *mut sg_ctx, net: *mut sg_net, nodes: *const u32, n_nodes: u32, row_begin: u32,
                         row_end: u32, flags: u32, pred: *const u32, latency_ns: *const u64,
                         packet_loss: *const f32, n_pairs: u32, pair_row: *const u32, pair_col: *const u32,
                         out_off: *mut u64, out_node: *mut u32, out_link: *mut u32, out_latency_ns: *mut u64,
                         out_packet_loss: *mut f32, cap: u64, total: *mut u64) -> i32;
    /// The same for the counted packets of one round's batch (pairs as in sg_link_load_packets).
    pub fn sg_tree_paths_packets(ctx: *mut sg_ctx, net: *mut sg_net, hosts: *mut sg_hosts, nodes: *const u32,
                                 n_nodes: u32, row_begin: u32, row_end: u32, flags: u32, pred: *const u32,
                                 latency_ns: *const u64, packet_loss: *const f32, packets: *const sg_packets,
                                 status: *const u8, out_off: *mut u64, out_node: *mut u32, out_link: *mut u32,
                                 out_latency_ns: *mut u64, out_packet_loss: *mut f32, cap: u64,
                                 total: *mut u64) -> i32;
    /// Link trace: the same crossings grouped by link (sg_net_links order) and sorted by
    /// (enter_ns, packet); link L owns records [out_link_off[L], out_link_off[L + 1]).  `watch`
    /// (NULL or n_links u8) empties the segments of links it marks 0.  SG_ERR_CAPACITY with
    /// out_link_off and *total complete when *total > cap.
    pub fn sg_link_trace_packets(ctx: *mut sg_ctx, net: *mut sg_net, hosts: *mut sg_hosts, nodes: *const u32,
                                 n_nodes: u32, row_begin: u32, row_end: u32, flags: u32, pred: *const u32,
                                 latency_ns: *const u64, packets: *const sg_packets, status: *const u8,
                                 watch: *const u8, out_link_off: *mut u64, out_packet: *mut u32,
                                 out_hop: *mut u32, out_enter_ns: *mut u64, out_exit_ns: *mut u64, cap: u64,
                                 total: *mut u64) -> i32;
    /// Link time series: every crossing of the trace adds its packet's weight to the cell
    /// (link_slot[link], (t - t0_ns) / bin_ns) of out_series (n_slots x n_bins u64, ADDED to), t the
    /// enter or the exit time by `at` (SG_SERIES_AT_*); crossings before t0_ns or past the last bin
    /// go to out_outside[2 s] / [2 s + 1] (or NULL).  link_slot NULL: the identity.
    pub fn sg_link_series_packets(ctx: *mut sg_ctx, net: *mut sg_net, hosts: *mut sg_hosts, nodes: *const u32,
                                  n_nodes: u32, row_begin: u32, row_end: u32, flags: u32, pred: *const u32,
                                  latency_ns: *const u64, packets: *const sg_packets, status: *const u8,
                                  weight: *const u32, link_slot: *const u32, n_slots: u32, at: u32, t0_ns: u64,
                                  bin_ns: u64, n_bins: u32, out_series: *mut u64, out_outside: *mut u64) -> i32;
    /// Link queues: the FIFO wait of every record of a link trace (link_off, enter_ns, packet) under a
    /// per-link service cost (cost_ps picoseconds per unit of weight[packet[i]], NULL weight: 1), the
    /// server free from link_free_in[L] (NULL: 0).  Per record wait, done and the records ahead; per
    /// link the new free time, the busy time, the largest and the summed wait, the deepest queue.
    /// First order: a wait is not propagated to the packet's later hops, unless flags carries
    /// SG_LINK_QUEUE_CARRY: then packet is required, n_weights bounds it, every link serves in
    /// ascending (carried enter, packet) order and the call iterates until no time moves.
    /// With SG_LINK_QUEUE_PACKETS enter_ns, out_wait_ns, out_done_ns and out_ahead (all required) have
    /// n_records + n_weights entries: a base time per packet in, its delay, arrival (u64::MAX: dropped)
    /// and the record that dropped it out (0xFFFF_FFFE: arrived, 0xFFFF_FFFF: no record).
    pub fn sg_link_queue(ctx: *mut sg_ctx, flags: u32, n_links: u32, link_off: *const u64, n_records: u64,
                         enter_ns: *const u64, packet: *const u32, weight: *const u32, n_weights: u32,
                         cost_ps: *const u64, link_free_in: *const u64, out_wait_ns: *mut u64,
                         out_done_ns: *mut u64, out_ahead: *mut u32, out_link_free: *mut u64,
                         out_link_busy_ns: *mut u64, out_link_wait_max_ns: *mut u64,
                         out_link_wait_sum_ns: *mut u64, out_link_ahead_max: *mut u32) -> i32;

    // ---- host-side dense RoutingInfo: generate_routing_info (sim_config.rs:411-448) ----
    pub fn sg_routing_info_create(n_used: u32, node_ids: *const u32, out: *mut *mut sg_routing_info) -> i32;
    pub fn sg_routing_info_destroy(ri: *mut sg_routing_info);
    pub fn sg_routing_info_fill(ctx: *mut sg_ctx, net: *mut sg_net, nodes: *const u32, flags: u32,
                                ri: *mut sg_routing_info) -> i32;
    /// Rows all-gathered from other ranks' sg_routing_build (sg_comm_allgather_rows).
    pub fn sg_routing_info_set_rows(ri: *mut sg_routing_info, row_begin: u32, row_end: u32, latency_ns: *const u64,
                                    packet_loss: *const f32) -> i32;
    pub fn sg_routing_info_view(ri: *const sg_routing_info, out: *mut sg_routing_view) -> i32;
    pub fn sg_routing_info_rows(ri: *const sg_routing_info, row_begin: u32, row_end: u32, latency_ns: *mut u64,
                                packet_loss: *mut f32) -> i32;
    pub fn sg_routing_info_index(ri: *const sg_routing_info, node_id: u32, row: *mut u32) -> i32;
    /// RoutingInfo::path (graph/mod.rs:448-450): 1 = Some, 0 = None.
    pub fn sg_routing_info_path(ri: *const sg_routing_info, start: u32, end: u32, latency_ns: *mut u64,
                                packet_loss: *mut f32) -> i32;
    pub fn sg_routing_info_smallest_latency(ri: *const sg_routing_info, out: *mut u64) -> i32;
    /// RoutingInfo::increment_packet_count (graph/mod.rs:453-460).
    pub fn sg_routing_info_increment_packet_count(ri: *mut sg_routing_info, start: u32, end: u32) -> i32;
    pub fn sg_routing_info_packet_count(ri: *const sg_routing_info, start: u32, end: u32) -> u64;
    /// IpAssignment (graph/mod.rs:354-430).
    pub fn sg_routing_info_set_addresses(ri: *mut sg_routing_info, n_addrs: u32, ipv4: *const u32,
                                         node_id: *const u32) -> i32;
    /// worker_getLatency / worker_isRoutable (worker.rs:651-684): network-order addresses.
    pub fn sg_worker_get_latency(ri: *const sg_routing_info, src_be: u32, dst_be: u32, latency_ns: *mut u64) -> i32;
    pub fn sg_worker_get_reliability(ri: *const sg_routing_info, src_be: u32, dst_be: u32, reliability: *mut f32)
        -> i32;
    pub fn sg_worker_is_routable(ri: *const sg_routing_info, src_be: u32, dst_be: u32) -> i32;

    // ---- packet delivery: Worker::send_packet + push_packet_to_host (worker.rs:322-397, 597-607) ----
    pub fn sg_hosts_create(ctx: *mut sg_ctx, n_hosts: u32, host_ipv4: *const u32, host_route_idx: *const u32,
                           host_seed: *const u64, out: *mut *mut sg_hosts) -> i32;
    pub fn sg_hosts_get_state(hosts: *mut sg_hosts, rng_state: *mut u64, event_ctr: *mut u64) -> i32;
    pub fn sg_hosts_set_state(hosts: *mut sg_hosts, rng_state: *const u64, event_ctr: *const u64) -> i32;
    pub fn sg_hosts_skip(hosts: *mut sg_hosts, n: u32, host_ids: *const u32, steps: *const u64) -> i32;
    pub fn sg_hosts_destroy(hosts: *mut sg_hosts);
    /// RoutingInfo::increment_packet_count on the device (ABI 7); null turns counting off.
    pub fn sg_ctx_set_packet_counters(ctx: *mut sg_ctx, counts: *mut u64, n_cells: u64) -> i32;
    pub fn sg_table_pack(ctx: *mut sg_ctx, table: *const sg_table, out_key: *mut u64, out_packable: *mut u32) -> i32;
    pub fn sg_deliver_round(ctx: *mut sg_ctx, hosts: *mut sg_hosts, table: *const sg_table, round: *const sg_round,
                            packets: *const sg_packets, out: *mut sg_deliveries, stats: *mut sg_round_stats) -> i32;

    // ---- sharded delivery: source half, exchange, destination half ----
    pub fn sg_deliver_source(ctx: *mut sg_ctx, hosts: *mut sg_hosts, table: *const sg_table, round: *const sg_round,
                             packets: *const sg_packets, status: *mut u8, deliver_time_ns: *mut u64,
                             event_id: *mut u64, host_owner: *const u32, n_ranks: u32, send: *mut sg_record,
                             send_counts: *mut u32, stats: *mut sg_round_stats) -> i32;
    pub fn sg_deliver_bucket(ctx: *mut sg_ctx, recv: *const sg_record, n_records: u32, host_local: *const u32,
                             n_hosts: u32, n_local_hosts: u32, dst_order: *mut u32, dst_offsets: *mut u32) -> i32;
    // the fixed-split exchange (one host synchronisation per round)
    pub fn sg_deliver_source_padded(ctx: *mut sg_ctx, hosts: *mut sg_hosts, table: *const sg_table,
                                    round: *const sg_round, packets: *const sg_packets, status: *mut u8,
                                    deliver_time_ns: *mut u64, event_id: *mut u64, host_owner: *const u32,
                                    n_ranks: u32, cap: u32, send_padded: *mut sg_record, send: *mut sg_record,
                                    xrow: *mut u64) -> i32;
    pub fn sg_deliver_bucket_padded(ctx: *mut sg_ctx, recv_padded: *const sg_record, n_ranks: u32, cap: u32,
                                    xall: *const u64, rank: u32, host_local: *const u32, n_hosts: u32,
                                    n_local_hosts: u32, dst_order: *mut u32, dst_offsets: *mut u32,
                                    stats: *mut sg_round_stats, recv_counts: *mut u32, pair_max: *mut u32) -> i32;
    pub fn sg_deliver_pad_to_compact(ctx: *mut sg_ctx, send_padded: *const sg_record, n_ranks: u32, cap: u32,
                                     xrow: *const u64, send: *mut sg_record) -> i32;

    // ---- collectives of the sharded path over RCCL (ABI 7, on the context's stream) ----
    pub fn sg_comm_unique_id(id: *mut u8) -> i32;
    pub fn sg_comm_create(ctx: *mut sg_ctx, id: *const u8, n_ranks: u32, rank: u32, out: *mut *mut sg_comm) -> i32;
    pub fn sg_comm_destroy(comm: *mut sg_comm);
    pub fn sg_comm_allgather_rows(comm: *mut sg_comm, lat: *mut u64, loss: *mut f32, rows_per_rank: u32,
                                  n_used: u32) -> i32;
    pub fn sg_comm_exchange_padded(comm: *mut sg_comm, send_padded: *const sg_record, recv_padded: *mut sg_record,
                                   cap: u32, xrow: *const u64, xall: *mut u64) -> i32;
    pub fn sg_comm_alltoallv_records(comm: *mut sg_comm, send: *const sg_record, send_counts: *const u32,
                                     recv: *mut sg_record, recv_counts: *const u32) -> i32;
    pub fn sg_comm_allgather_u64(comm: *mut sg_comm, mine: *const u64, all: *mut u64, n: u32) -> i32;

    // ---- router inbound CoDel queues (router/mod.rs:15-58, codel_queue.rs) ----
    pub fn sg_codel_create(ctx: *mut sg_ctx, n_hosts: u32, ring_cap: u32, out: *mut *mut sg_codel) -> i32;
    pub fn sg_codel_destroy(q: *mut sg_codel);
    pub fn sg_codel_run(ctx: *mut sg_ctx, q: *mut sg_codel, ev: *const sg_codel_events, pop_result: *mut u32,
                        pkt_status: *mut u8, n_packets: u32, n_dropped: *mut u64) -> i32;
    pub fn sg_codel_ring_cap(q: *const sg_codel) -> u32;
    pub fn sg_codel_get_state(q: *mut sg_codel, out: *mut sg_codel_state) -> i32;
    pub fn sg_codel_set_state(q: *mut sg_codel, input: *const sg_codel_state) -> i32;

    // ---- inbound pipeline: router queue -> relay_inet_in (host.rs:781-786, relay/mod.rs:72-288) ----
    pub fn sg_inbound_create(ctx: *mut sg_ctx, n_hosts: u32, bw_down_bits: *const u64, ring_cap: u32,
                             out: *mut *mut sg_inbound) -> i32;
    pub fn sg_inbound_destroy(ib: *mut sg_inbound);
    pub fn sg_inbound_ring_cap(ib: *const sg_inbound) -> u32;
    pub fn sg_inbound_run(ctx: *mut sg_ctx, ib: *mut sg_inbound, arr: *const sg_inbound_arrivals, window_end_ns: u64,
                          bootstrap_end_ns: u64, sim_end_ns: u64, event_ctr: *mut u64, fwd_time: *mut u64,
                          pkt_status: *mut u8, n_packets: u32, n_dropped: *mut u64) -> i32;
    /// ABI 7: this call's arrivals' fates in arrival order.
    pub fn sg_inbound_run_ordered(ctx: *mut sg_ctx, ib: *mut sg_inbound, arr: *const sg_inbound_arrivals,
                                  window_end_ns: u64, bootstrap_end_ns: u64, sim_end_ns: u64, event_ctr: *mut u64,
                                  fwd_time: *mut u64, pkt_status: *mut u8, n_packets: u32, arr_fwd_time: *mut u64,
                                  arr_status: *mut u8, n_dropped: *mut u64) -> i32;
    pub fn sg_inbound_get_state(ib: *mut sg_inbound, queue: *mut sg_codel_state, relay: *mut sg_inbound_relay_state)
        -> i32;

    // ---- outbound pipeline: interface -> relay_inet_out -> router (relay/mod.rs:111-275) ----
    pub fn sg_outbound_create(ctx: *mut sg_ctx, n_hosts: u32, host_ipv4: *const u32, bw_up_bits: *const u64,
                              ring_cap: u32, out: *mut *mut sg_outbound) -> i32;
    pub fn sg_outbound_destroy(ob: *mut sg_outbound);
    pub fn sg_outbound_ring_cap(ob: *const sg_outbound) -> u32;
    pub fn sg_outbound_run(ctx: *mut sg_ctx, ob: *mut sg_outbound, sends: *const sg_outbound_sends,
                           window_end_ns: u64, bootstrap_end_ns: u64, sim_end_ns: u64, event_ctr: *mut u64,
                           fwd_time: *mut u64, pkt_status: *mut u8, n_packets: u32, sent: *mut sg_outbound_sent,
                           n_sent: *mut u32) -> i32;
    pub fn sg_outbound_get_state(ob: *mut sg_outbound, queue: *mut sg_outbound_queue_state,
                                 relay: *mut sg_inbound_relay_state) -> i32;

    // ---- the interface's qdisc (interface.rs:97-108, :168-181, :227-259; queuing.rs) ----
    pub fn sg_outbound_create_qdisc(ctx: *mut sg_ctx, n_hosts: u32, host_ipv4: *const u32, bw_up_bits: *const u64,
                                    ring_cap: u32, qdisc: u32, max_sockets: u32, out: *mut *mut sg_outbound) -> i32;
    pub fn sg_outbound_qdisc(ob: *const sg_outbound) -> u32;
    pub fn sg_outbound_max_sockets(ob: *const sg_outbound) -> u32;
    pub fn sg_outbound_run_qdisc(ctx: *mut sg_ctx, ob: *mut sg_outbound, sends: *const sg_outbound_sends,
                                 socket: *const u32, window_end_ns: u64, bootstrap_end_ns: u64, sim_end_ns: u64,
                                 event_ctr: *mut u64, fwd_time: *mut u64, pkt_status: *mut u8, n_packets: u32,
                                 sent: *mut sg_outbound_sent, n_sent: *mut u32) -> i32;
    pub fn sg_outbound_get_qdisc_state(ob: *mut sg_outbound, q: *mut sg_outbound_qdisc_state,
                                       relay: *mut sg_inbound_relay_state) -> i32;

    /// The device array of the hosts' event-id counters (Host::event_id_counter).
    pub fn sg_hosts_event_ctr(hosts: *mut sg_hosts) -> *mut u64;

    // ---- packets in flight: push_packet_to_host -> Host::execute's pops (worker.rs:597-607, host.rs:753-757) ----
    pub fn sg_wire_create(ctx: *mut sg_ctx, n_hosts: u32, capacity: u64, bin_ns: u64, n_bins: u32,
                          out: *mut *mut sg_wire) -> i32;
    pub fn sg_wire_destroy(w: *mut sg_wire);
    pub fn sg_wire_count(w: *const sg_wire) -> u64;
    /// One event per delivered packet of a round; does not synchronise.
    pub fn sg_wire_push(ctx: *mut sg_ctx, w: *mut sg_wire, packets: *const sg_packets, out: *const sg_deliveries,
                        packet_id: *const u32, id_base: u32, len: *const u32) -> i32;
    /// Every event with time < window_end_ns, grouped by host in EventQueue order; synchronises.
    pub fn sg_wire_pop(ctx: *mut sg_ctx, w: *mut sg_wire, window_end_ns: u64, out: *mut sg_wire_arrivals,
                       n_out: *mut u32, next_time_ns: *mut u64) -> i32;
    pub fn sg_wire_get_state(w: *mut sg_wire, cap: u64, out: *mut sg_wire_state, n: *mut u64) -> i32;
    pub fn sg_wire_set_state(w: *mut sg_wire, n: u64, input: *const sg_wire_state) -> i32;

    // ---- the wire on the sharded path: stamp on the source rank, push on the owner ----
    /// After sg_deliver_source: len and the caller's packet id into the records, in place.
    pub fn sg_wire_stamp_records(ctx: *mut sg_ctx, send: *mut sg_record, n_records: u32, packet_id: *const u32,
                                 id_base: u32, len: *const u32, n_packets: u32) -> i32;
    /// After sg_deliver_source_padded: the valid slots of every block and the spilled records.
    pub fn sg_wire_stamp_records_padded(ctx: *mut sg_ctx, send_padded: *mut sg_record, send: *mut sg_record,
                                        n_ranks: u32, cap: u32, xrow: *const u64, packet_id: *const u32,
                                        id_base: u32, len: *const u32, n_packets: u32) -> i32;
    /// One event per stamped record received; does not synchronise.
    pub fn sg_wire_push_records(ctx: *mut sg_ctx, w: *mut sg_wire, recv: *const sg_record, n_records: u32,
                                host_map: *const u32, n_hosts: u32) -> i32;
    /// The valid records of every block of a fixed-split exchange; nothing when the round overflowed.
    pub fn sg_wire_push_records_padded(ctx: *mut sg_ctx, w: *mut sg_wire, recv_padded: *const sg_record,
                                       n_ranks: u32, cap: u32, xall: *const u64, rank: u32, host_map: *const u32,
                                       n_hosts: u32) -> i32;

    // ---- device group: the one Shadow process owns N contexts (manager.rs:254-261) ----
    /// 1 <= n <= 64 distinct contexts; peer access is enabled between distinct devices.
    /// The pointer arrays of these calls are only read.
    pub fn sg_group_create(ctxs: *mut *mut sg_ctx, n: u32, out: *mut *mut sg_group) -> i32;
    pub fn sg_group_destroy(g: *mut sg_group);
    pub fn sg_group_size(g: *const sg_group) -> u32;
    pub fn sg_group_last_error(g: *const sg_group) -> *const c_char;
    pub fn sg_group_last_error_pair(g: *const sg_group, row: *mut u32, col: *mut u32);
    /// One host RoutingInfo from all members: member m builds and copies its block of rows.
    pub fn sg_group_routing_info_fill(g: *mut sg_group, nets: *mut *mut sg_net, nodes: *const u32, flags: u32,
                                      ri: *mut sg_routing_info) -> i32;
    /// The fixed-split round's exchange for all members: one pull kernel per owner, no RCCL.
    pub fn sg_group_exchange_padded(g: *mut sg_group, send_padded: *mut *const sg_record,
                                    recv_padded: *mut *mut sg_record, cap: u32, xrow: *mut *const u64,
                                    xall: *mut *mut u64) -> i32;
    /// The exact exchange: counts is the host n x n matrix (member b's records for member r).
    pub fn sg_group_alltoallv_records(g: *mut sg_group, send: *mut *const sg_record, counts: *const u32,
                                      recv: *mut *mut sg_record) -> i32;

    // ---- link loads and link trace across a group: a round sharded by source row block ----
    /// The member whose device-found error the group's last call reported, or u32::MAX.
    pub fn sg_group_last_error_member(g: *const sg_group) -> u32;
    /// sg_link_load_packets on every member at once; the members' sums are added into root's
    /// arrays by one kernel, after every member validated: any error leaves them untouched.
    pub fn sg_group_link_load_packets(g: *mut sg_group, nets: *mut *mut sg_net, hosts: *mut *mut sg_hosts,
                                      nodes: *const u32, n_nodes: u32, row_begin: *const u32, row_end: *const u32,
                                      pred: *mut *const u32, packets: *const sg_packets, status: *mut *const u8,
                                      weight: *mut *const u32, root: u32, out_link_load: *mut u64,
                                      out_node_load: *mut u64, out_hops: *mut *mut u32) -> i32;
    /// sg_link_trace_packets on every member at once, the members' sorted segments merged on root:
    /// link L's records ascend in (enter_ns, member, member-local packet); out_packet = packet_base[m] + p.
    pub fn sg_group_link_trace_packets(g: *mut sg_group, nets: *mut *mut sg_net, hosts: *mut *mut sg_hosts,
                                       nodes: *const u32, n_nodes: u32, row_begin: *const u32, row_end: *const u32,
                                       pred: *mut *const u32, latency_ns: *mut *const u64,
                                       packets: *const sg_packets, status: *mut *const u8, watch: *const u8,
                                       packet_base: *const u32, root: u32, out_link_off: *mut u64,
                                       out_packet: *mut u32, out_member: *mut u8, out_hop: *mut u32,
                                       out_enter_ns: *mut u64, out_exit_ns: *mut u64, cap: u64,
                                       total: *mut u64) -> i32;
    /// sg_link_series_packets on every member at once; `link_slot` is a HOST map.  The members'
    /// sums are added into root's arrays by one kernel: any error leaves them untouched.
    pub fn sg_group_link_series_packets(g: *mut sg_group, nets: *mut *mut sg_net, hosts: *mut *mut sg_hosts,
                                        nodes: *const u32, n_nodes: u32, row_begin: *const u32, row_end: *const u32,
                                        pred: *mut *const u32, latency_ns: *mut *const u64,
                                        packets: *const sg_packets, status: *mut *const u8,
                                        weight: *mut *const u32, link_slot: *const u32, n_slots: u32, at: u32,
                                        t0_ns: u64, bin_ns: u64, n_bins: u32, root: u32, out_series: *mut u64,
                                        out_outside: *mut u64) -> i32;
}
