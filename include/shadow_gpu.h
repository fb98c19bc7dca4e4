/*
 * shadow_gpu.h -- C ABI of the MI355X network core for Shadow (gfx950 / HIP).
 *
 * This is the drop-in boundary for two stages of Shadow 3.2.0's network core:
 *
 *   1. Routing-table build.  Replaces
 *        NetworkGraph::compute_shortest_paths   src/main/network/graph/mod.rs:183-228
 *        NetworkGraph::get_direct_paths         src/main/network/graph/mod.rs:230-252
 *      and the id remap of generate_routing_info (src/main/core/sim_config.rs:411-448).
 *      The result is a dense table instead of HashMap<(u32,u32),PathProperties>
 *      (RoutingInfo, graph/mod.rs:434-481): row i / column j = nodes[i] / nodes[j].
 *
 *   2. Inter-host packet delivery for one scheduling round.  Replaces the
 *      per-packet body of Worker::send_packet (src/main/core/worker.rs:322-397)
 *      and WorkerShared::push_packet_to_host (worker.rs:597-607): destination
 *      resolution (Dns::addr_to_host_id, network/dns.rs:174-176), path lookup
 *      (WorkerShared::latency/reliability, worker.rs:517-531), the per-host
 *      Xoshiro256++ loss draw (host/host.rs:221,645-647), arrival time, event
 *      ids (host.rs:649-653) and the destination EventQueue order
 *      (core/work/event.rs:84-155).
 *
 * Conventions: plain C, int32_t status codes (sg_status), never unwinds.
 * Pointers documented "device" are HIP device pointers on the context's
 * device; everything else is host memory.  The reference's panics
 * (unreachable pair, graph/mod.rs:219; unit overflow, graph/mod.rs:336) become
 * status codes.  Calls on one context are not thread-safe (the reference makes
 * these calls from one thread: sim_config.rs:137 and the manager's round loop).
 */
#ifndef SHADOW_GPU_H
#define SHADOW_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_ABI_VERSION 7

typedef enum sg_status {
  SG_OK = 0,
  SG_ERR_NO_EDGE = 1,       /* graph/mod.rs:266-268  "No edge connecting node {} to {}" */
  SG_ERR_MULTI_EDGE = 2,    /* graph/mod.rs:269-275  "More than one edge connecting node {} to {}" */
  SG_ERR_UNREACHABLE = 3,   /* graph/mod.rs:219      assert_eq!(paths.len(), n^2) (panic) */
  SG_ERR_OOM = 4,
  SG_ERR_INVALID_ARG = 5,
  SG_ERR_DEVICE = 6,        /* HIP runtime error */
  SG_ERR_PARSE = 7,         /* NetworkGraph::parse / ShadowEdge::try_from (graph/mod.rs:72-181) */
  SG_ERR_UNSORTED = 8,      /* sg_deliver_round: packets not grouped by ascending source host */
  SG_ERR_DUPLICATE_IP = 9,  /* two hosts with one address (IpAssignment::assign_ip, graph/mod.rs:383-394) */
  SG_ERR_CAPACITY = 10,     /* a CoDel queue outgrew its ring (sg_codel_create ring_cap) */
  SG_ERR_UNSUPPORTED = 12,  /* sg_comm_*: RCCL (librccl.so.1) could not be opened (ABI 7);
                               sg_group_create: a pair of devices without peer access */
  SG_ERR_TIME_OVERFLOW = 11 /* send time + latency past EMUTIME_MAX: EmulatedTime + SimulationTime
                               panics in the reference (emulated_time.rs:121-126, worker.rs:381) */
} sg_status;

typedef struct sg_ctx sg_ctx;     /* one HIP device + stream + workspace */
typedef struct sg_net sg_net;     /* device-resident network graph */
typedef struct sg_hosts sg_hosts; /* device-resident host table: addresses, routes, RNG, event ids */
typedef struct sg_gml sg_gml;     /* host-side parsed GML graph */

int32_t sg_abi_version(void);

/* ---- context ------------------------------------------------------------ */
int32_t sg_ctx_create(int32_t device, sg_ctx** out);
void sg_ctx_destroy(sg_ctx* ctx);
/* Use an existing hipStream_t (e.g. torch's current stream); NULL = the context's own
 * stream, a blocking stream (ordered with work on the legacy default stream, which is
 * torch's default stream).  Every entry point launches on this stream and reads
 * device inputs in stream order: inputs written on some other non-blocking stream
 * must be complete (or waited for) before the call.
 * tests/test_stream_gpu.py holds every single-context entry point to this on a
 * caller's non-blocking stream: behind a delay kernel on that stream the inputs are
 * overwritten with a second valid set and the outputs with a poison byte, then the
 * call runs and its results must be the second set's, bit for bit; the calls marked
 * "does not synchronise" below must return while the delay still runs. */
int32_t sg_ctx_set_stream(sg_ctx* ctx, void* hip_stream);
void* sg_ctx_stream(const sg_ctx* ctx);
int32_t sg_ctx_synchronize(sg_ctx* ctx);
/* Message and (row, col) of the last failing call on this context. */
const char* sg_ctx_last_error(const sg_ctx* ctx);
void sg_ctx_last_error_pair(const sg_ctx* ctx, uint32_t* row, uint32_t* col);
/* Measurement hooks (bench.py): with bit 0 of `enable` set, every launch of an
 * instrumented kernel is bracketed by HIP events on the context stream;
 * bit 1 (SG_TIMERS_COUNT_WORK) additionally runs the counting variant of kernels
 * whose work is data-dependent (the relaxation kernel counts the lane-
 * relaxations it performs; slower, so time and count in separate runs).
 * read_timer returns the summed device time, the launch count and the
 * algorithmic work ("relax": lane-relaxations; delivery kernels: bytes).
 * Enabling or disabling resets all timers. */
#define SG_TIMERS_ON 1
#define SG_TIMERS_COUNT_WORK 2
int32_t sg_ctx_enable_timers(sg_ctx* ctx, int32_t enable);
int32_t sg_ctx_read_timer(sg_ctx* ctx, const char* kernel, double* total_ms, uint64_t* launches,
                          double* work);

/* ---- GML ingest (NetworkGraph::parse, graph/mod.rs:134-181) -------------- */
/* Edge list in GML edge order; node indices are petgraph NodeIndex values
 * (GML node order).  Latency in integer ns (units.rs:377-438), loss f32. */
typedef struct sg_graph {
  uint32_t n_nodes;
  uint32_t n_edges;
  const uint32_t* edge_src;
  const uint32_t* edge_dst;
  const uint64_t* edge_latency_ns;
  const float* edge_packet_loss;
  const uint32_t* node_gml_id; /* optional (may be NULL): GML ids, for messages */
  uint8_t directed;
} sg_graph;

/* Parse GML text.  On failure returns SG_ERR_PARSE and writes a message into
 * err (if err_len > 0).  Latency unit overflow is reported here. */
int32_t sg_gml_parse(const char* text, size_t len, sg_gml** out, char* err, size_t err_len);
/* The same parse on `threads` host threads (0: min(cores, 16), or SG_GML_THREADS).
 * Results and the error reported are those of the single-threaded parse
 * (load_network_graph feeds it, graph/mod.rs:498-513). */
int32_t sg_gml_parse_threads(const char* text, size_t len, uint32_t threads, sg_gml** out, char* err,
                             size_t err_len);
/* load_network_graph + NetworkGraph::parse (graph/mod.rs:483-513): read the GML
 * file at `path` ("~/" expanded, tilde_expansion), xz-decompress it when
 * compression = 1 (read_xz, :484-496: the system liblzma.so.5, opened at run
 * time), check it is UTF-8 (String::from_utf8 / read_to_string), and parse it
 * on `threads` threads as sg_gml_parse_threads.  compression 0 = plain text.
 * Read, decompression and UTF-8 failures are SG_ERR_PARSE with a message. */
int32_t sg_gml_load(const char* path, uint32_t compression, uint32_t threads, sg_gml** out, char* err,
                    size_t err_len);
/* Borrow the parsed edge list (valid until sg_gml_destroy). */
int32_t sg_gml_graph(const sg_gml* g, sg_graph* out);
/* NetworkGraph::node_id_to_index (graph/mod.rs:126-128); SG_ERR_INVALID_ARG if absent. */
int32_t sg_gml_node_index(const sg_gml* g, uint32_t gml_id, uint32_t* out_index);
void sg_gml_destroy(sg_gml* g);

/* ---- routing-table build ------------------------------------------------- */
/* Upload a graph to the device and build its in-arc (CSC) form. */
int32_t sg_net_create(sg_ctx* ctx, const sg_graph* g, sg_net** out);
void sg_net_destroy(sg_net* net);

#define SG_ROUTE_SHORTEST_PATH 0x1u /* network.use_shortest_path (configuration.rs:315-326) */
#define SG_ROUTE_OUT_DEVICE 0x2u    /* out_* are device pointers (else host) */

/*
 * Rows [row_begin, row_end) of the routing table over `nodes` (petgraph
 * indices of the used nodes, n_used of them; the caller's order defines the
 * table's row/column order):
 *   out_latency_ns [(i-row_begin)*n_used + j] = path(nodes[i] -> nodes[j]).latency_ns
 *   out_packet_loss[(i-row_begin)*n_used + j] = path(nodes[i] -> nodes[j]).packet_loss
 * With SG_ROUTE_SHORTEST_PATH: the lexicographic (latency, loss) optimum of
 * the left fold PathProperties::default() + e1 + ... + ek over every path,
 * bit-exact (petgraph::algo::dijkstra semantics), diagonal = the node's single
 * self-loop.  Without: the single direct edge of every pair.
 * Errors as the reference: missing/duplicate self-loop (first node in order),
 * missing/duplicate direct edge (first pair in row-major order), unreachable
 * pair (first pair in row-major order); sg_ctx_last_error_pair gives (i, j).
 * Rows may be sharded across devices by calling with disjoint row ranges.
 */
int32_t sg_routing_build(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_used,
                         uint32_t row_begin, uint32_t row_end, uint32_t flags,
                         uint64_t* out_latency_ns, float* out_packet_loss);

/* RoutingInfo::get_smallest_latency_ns (graph/mod.rs:478-480) over `count`
 * device latencies; UINT64_MAX when count == 0. */
int32_t sg_routing_min_latency(sg_ctx* ctx, const uint64_t* d_latency_ns, size_t count,
                               uint64_t* out_min);

/* ---- shortest-path trees: predecessor and first-hop rows (additive to ABI 7) --
 * Which links a path uses.  The reference keeps no such table (a PathProperties
 * is a latency and a loss, graph/mod.rs:297-303), but compute_shortest_paths
 * (graph/mod.rs:183-228) and the left fold PathProperties::add
 * (graph/mod.rs:322-331) pin one: a path is right exactly when default() + e1 +
 * ... + ek over its edges gives the table's cell, latency and loss bits alike.
 *
 * For a source s let key[v] = (latency, loss bits) be s's row of the table, with
 * key[s] = (0, +0.0f), the fold's default() (the diagonal cell holds the
 * self-loop and is not read).  An in-arc u -> v (u != v, v != s; parallel edges
 * each count) is tight when key[u].lat + w.lat == key[v].lat and the f32 fold
 * 1 - (1 - key[u].loss) * (1 - w.loss), one rounding per operation, has exactly
 * key[v]'s loss bits.  Then
 *   pred[s][v]      = the smallest petgraph node index u among v's tight in-arcs
 *                     (by value, never by arc position); pred[s][s] = s.  Arc
 *                     latency is at least 1 ns, so every pred row is a tree rooted
 *                     at s, and the fold along the tree path to v is key[v].
 *   first_hop[s][v] = the node after s on that tree path (v itself when
 *                     pred[s][v] == s); first_hop[s][s] = s.
 * Both hold petgraph NodeIndex values, whatever the column order of `nodes`:
 *   out_pred     [(i-row_begin)*n_nodes + j] = pred[nodes[i]][nodes[j]]
 *   out_first_hop[(i-row_begin)*n_nodes + j] = first_hop[nodes[i]][nodes[j]]
 *
 * A tree spans every graph node, so the rows it is computed from must: n_nodes is
 * the net's node count and `nodes` a permutation of 0 .. n_nodes-1.  A simulation
 * with a used subset puts its used nodes first and takes rows [0, n_used): its
 * used x used table is the leading n_used columns of those rows.
 * The f32 fold is not associative: the rest of s's tree path from an
 * intermediate node h need not be h's own tree path.  Expand a path inside one
 * source's pred row (sg_tree_path), never first hop by first hop across rows.
 *
 * sg_routing_tree: rows [row_begin, row_end) of both outputs from the same rows
 * of the table (latency_ns / packet_loss, row-major from row_begin, as
 * sg_routing_build wrote them for the same `nodes`).  SG_ROUTE_OUT_DEVICE applies
 * to inputs and outputs alike.  Either output may be NULL, not both.
 * SG_ERR_INVALID_ARG, the outputs untouched, for n_nodes other than the net's node
 * count, `nodes` not a permutation, a bad row range, NULL arguments.  A cell
 * without a tight in-arc means the rows are not this graph's table:
 * SG_ERR_INVALID_ARG with a message, sg_ctx_last_error_pair = the first such
 * (row, col) in row-major order; the outputs are then undefined.  Synchronises.
 * Row ranges shard across contexts exactly as the build's do.
 *
 * sg_routing_build_tree: sg_routing_build over those rows, then the tree pass;
 * all four outputs are required.  The build's errors in the build's precedence;
 * SG_ERR_INVALID_ARG (before anything is written) without SG_ROUTE_SHORTEST_PATH:
 * direct paths have no tree. */
int32_t sg_routing_tree(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes,
                        uint32_t row_begin, uint32_t row_end, uint32_t flags,
                        const uint64_t* latency_ns, const float* packet_loss,
                        uint32_t* out_pred, uint32_t* out_first_hop);
int32_t sg_routing_build_tree(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes,
                              uint32_t row_begin, uint32_t row_end, uint32_t flags,
                              uint64_t* out_latency_ns, float* out_packet_loss,
                              uint32_t* out_pred, uint32_t* out_first_hop);
/* Host only, no device: the node sequence src ... dst (petgraph indices) of the
 * tree path, from one host pred row -- the row of source src, in the column
 * order of `nodes` (NULL: the identity order).  *len = its length in nodes (1
 * when src == dst).  SG_ERR_CAPACITY with *len set when cap is too small
 * (nothing is written to out_path); SG_ERR_INVALID_ARG for src or dst out of
 * range, `nodes` not a permutation, or a row that does not reach src within
 * n_nodes steps: a garbage row ends, it never loops. */
int32_t sg_tree_path(const uint32_t* pred_row, const uint32_t* nodes, uint32_t n_nodes, uint32_t src, uint32_t dst,
                     uint32_t* out_path, uint32_t cap, uint32_t* len);

/* ---- link loads: per-pair counters folded onto graph links (additive to ABI 7) --
 * How much crossed each link: a u64 matrix per (source row, destination column)
 * -- the packet counters of sg_ctx_set_packet_counters, or bytes a caller
 * accumulates -- attributed to the links of each cell's tree path through the
 * pred rows of sg_routing_tree.  Exact (integer adds only) and independent of
 * order; the delivery round itself is not touched.
 *
 * A link is a distinct ordered node pair (u, v) joined by at least one edge: an
 * undirected edge {a, b} gives (a, b) and (b, a), a directed edge one link, a
 * self-loop (a, a).  Parallel edges between one pair are ONE link (pred is
 * defined by node).  Link order: ascending (head v, tail u), so the links into
 * one node are contiguous.
 *
 * sg_net_links: the link list to host arrays; *n_links is always set.
 * SG_ERR_CAPACITY, nothing written, when cap < *n_links.  Built once per net on
 * first use (a device-to-host copy of the edge list and a host sort).
 * sg_net_edge_links: host arrays of n_edges entries; out_fwd[e] = the link of
 * edge e as (src -> dst), out_rev[e] = the link (dst -> src) on an undirected
 * graph, UINT32_MAX on a directed one; for a self-loop both name the same link.
 * Parallel edges share their link's number: load_of_edge[e] =
 * link_load[out_fwd[e]] (+ link_load[out_rev[e]]) is the pair's load.
 *
 * sg_link_load: rows [row_begin, row_end), row i of source s = nodes[i]; `pred`
 * (as sg_routing_tree writes it: petgraph indices, columns in `nodes` order) and
 * `counts` (u64, count_cols <= n_nodes columns; columns at or past count_cols
 * count zero) are row-major from row_begin.  With sub_i[v] = the sum of
 * counts[i][j] over the columns j != i whose node nodes[j] lies in v's subtree of
 * row i's tree, v included:
 *   out_link_load[link (pred_i[v], v)] += sub_i[v]      for every v != s
 *   out_link_load[link (s, s)]         += counts[i][i]  (the diagonal cell's path
 *                                          is the self-loop, get_edge_weight's rule)
 *   out_node_load[v]                   += sub_i[v]      for v != s: what arrives at
 *                                          or passes through v
 * out_link_load has *n_links entries in link order, out_node_load n_nodes entries
 * by petgraph index.  All sums are u64 and WRAP on overflow.  They are ADDED to
 * what the arrays hold: the caller zeroes them, and row blocks, group members and
 * successive measurement intervals sum into one array.  Either output may be
 * NULL, not both.  SG_ROUTE_OUT_DEVICE applies to pred, counts and both outputs
 * alike.  `nodes` is a permutation of 0 .. n_nodes-1, as for the tree; a
 * simulation with a used subset puts its used nodes first and passes count_cols =
 * n_used when its delivery table is n_used wide.  Synchronises once.
 * SG_ERR_INVALID_ARG, the outputs untouched, for NULL arguments, a bad row range,
 * n_nodes other than the net's, `nodes` not a permutation, count_cols > n_nodes,
 * both outputs NULL.  SG_ERR_INVALID_ARG with a message and
 * sg_ctx_last_error_pair = the first (row, col) in row-major order, the outputs
 * then undefined, for a pred row that holds a value >= n_nodes, does not have
 * pred[s] == s, names a pair that is not a link, or leaves nodes unreleased (a
 * cycle: not a tree); never a trap, never a loop.  Within one row the first two
 * kinds are reported ahead of the others.  A row whose counters are all zero is
 * skipped: its pred row is not validated.  A node whose subtree sum is zero is
 * not looked up: a pair that is not a link is reported only where traffic
 * crosses it.
 *
 * sg_link_load_packets gives the same sums straight from one round's batch,
 * without the counter matrix and with a weight per packet; it takes the
 * delivery types, so it is declared after them ("link loads from a round's
 * packets", below sg_deliver_bucket). */
int32_t sg_net_links(sg_ctx* ctx, sg_net* net, uint32_t* n_links, uint32_t* out_tail, uint32_t* out_head,
                     uint32_t cap);
int32_t sg_net_edge_links(sg_ctx* ctx, sg_net* net, uint32_t* out_fwd, uint32_t* out_rev);
int32_t sg_link_load(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes,
                     uint32_t row_begin, uint32_t row_end, uint32_t flags,
                     const uint32_t* pred, const uint64_t* counts, uint32_t count_cols,
                     uint64_t* out_link_load, uint64_t* out_node_load);

/* ---- host-side dense RoutingInfo (graph/mod.rs:432-481) ------------------
 * RoutingInfo<u32> keyed by GML node id, as generate_routing_info builds it
 * (sim_config.rs:411-448), stored dense: row-major latency / loss arrays in
 * pinned host memory owned by the object and an id -> row map.  It replaces the
 * reference's two n_used^2 HashMaps (compute_shortest_paths', graph/mod.rs:190-208,
 * and the id remap's, sim_config.rs:423-445) and answers RoutingInfo::path and
 * the WorkerShared lookups with array reads.  Lookups are read-only and safe
 * from any number of threads; packet counters are atomic.                    */
typedef struct sg_routing_info sg_routing_info;
/* node_ids: the used GML node ids (the table's row / column order).  Allocates
 * the n_used^2 table of 8-byte cells (pinned when a HIP device is present).  SG_ERR_INVALID_ARG
 * for a duplicate id. */
int32_t sg_routing_info_create(uint32_t n_used, const uint32_t* node_ids, sg_routing_info** out);
void sg_routing_info_destroy(sg_routing_info* ri);
/* Build the whole table: nodes[i] = the petgraph index of node_ids[i]
 * (NetworkGraph::node_id_to_index, graph/mod.rs:126-128).  Results and errors
 * are sg_routing_build's over all rows; row blocks are built on the device and
 * copied into the object while the next block builds.  Also computes
 * get_smallest_latency_ns. */
int32_t sg_routing_info_fill(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t flags, sg_routing_info* ri);
/* Rows [row_begin, row_end) from host arrays (e.g. row shards gathered from
 * other ranks' sg_routing_build).  get_smallest_latency_ns is Some once every row
 * has been set (by fill or by these calls), over the whole table. */
int32_t sg_routing_info_set_rows(sg_routing_info* ri, uint32_t row_begin, uint32_t row_end,
                                 const uint64_t* latency_ns, const float* packet_loss);
/* Zero-copy view: cell (i, j) = path(node_ids[i] -> node_ids[j]) packed as
 * (latency_ns << 32) | bits(packet_loss), 8 bytes, while the latency is below
 * SG_CELL_WIDE; a cell whose upper half is SG_CELL_WIDE holds its loss bits only,
 * and its u64 latency is one of the n_wide entries that sg_routing_info_rows and
 * the lookups below resolve (paths of 4.29 s or more are rare: the whole table
 * moves and lives at 8 bytes per cell instead of 12). */
#define SG_CELL_WIDE 0xFFFFFFFFu
typedef struct sg_routing_view {
  uint32_t n;
  const uint32_t* node_ids;
  const uint64_t* cells;
  uint64_t n_wide;
  uint32_t pinned;
} sg_routing_view;
int32_t sg_routing_info_view(const sg_routing_info* ri, sg_routing_view* out);
/* Rows [row_begin, row_end) decoded into caller arrays (latency u64, loss f32, row-major). */
int32_t sg_routing_info_rows(const sg_routing_info* ri, uint32_t row_begin, uint32_t row_end, uint64_t* latency_ns,
                             float* packet_loss);
/* Row of a GML node id (SG_ERR_INVALID_ARG if absent). */
int32_t sg_routing_info_index(const sg_routing_info* ri, uint32_t node_id, uint32_t* row);
/* RoutingInfo::path(start, end) (graph/mod.rs:448-450): 1 = Some (outputs
 * written when non-NULL), 0 = None. */
int32_t sg_routing_info_path(const sg_routing_info* ri, uint32_t start, uint32_t end, uint64_t* latency_ns,
                             float* packet_loss);
/* RoutingInfo::get_smallest_latency_ns (graph/mod.rs:478-480): 1 = Some, 0 = None. */
int32_t sg_routing_info_smallest_latency(const sg_routing_info* ri, uint64_t* out);
/* RoutingInfo::increment_packet_count (graph/mod.rs:453-460): saturating, thread
 * safe; SG_ERR_INVALID_ARG for an unknown pair (its caller unwraps, worker.rs:538-542). */
int32_t sg_routing_info_increment_packet_count(sg_routing_info* ri, uint32_t start, uint32_t end);
uint64_t sg_routing_info_packet_count(const sg_routing_info* ri, uint32_t start, uint32_t end);
/* IpAssignment (graph/mod.rs:354-430): the assigned addresses (host byte order,
 * u32::from(Ipv4Addr)) and their GML node ids; SG_ERR_DUPLICATE_IP for a repeat. */
int32_t sg_routing_info_set_addresses(sg_routing_info* ri, uint32_t n_addrs, const uint32_t* ipv4,
                                      const uint32_t* node_id);
/* WorkerShared::latency / reliability / is_routable (worker.rs:517-555) as the C
 * exports worker_getLatency / worker_isRoutable take them (worker.rs:651-684):
 * addresses in network byte order.  latency / reliability return SG_OK, or
 * SG_ERR_INVALID_ARG where the reference's Option is None (worker_getLatency
 * unwraps it: a panic).  reliability = 1f32 - loss.  is_routable: 1 when both
 * addresses are assigned (the graph is connected), else 0. */
int32_t sg_worker_get_latency(const sg_routing_info* ri, uint32_t src_be, uint32_t dst_be, uint64_t* latency_ns);
int32_t sg_worker_get_reliability(const sg_routing_info* ri, uint32_t src_be, uint32_t dst_be, float* reliability);
int32_t sg_worker_is_routable(const sg_routing_info* ri, uint32_t src_be, uint32_t dst_be);

/* ---- packet delivery ------------------------------------------------------ */
/*
 * Host table.  host_ipv4[h] = the host's address (host byte order, as
 * u32::from(Ipv4Addr)); host_route_idx[h] = index of the host's graph node in
 * the routing table's node list; host_seed[h] = HostInfo.seed (node_seed):
 * the RNG is Xoshiro256PlusPlus::seed_from_u64(seed) (host.rs:221).  HostId =
 * h (hosts sorted by name, configuration.rs:107).  Addresses must be unique.
 */
int32_t sg_hosts_create(sg_ctx* ctx, uint32_t n_hosts, const uint32_t* host_ipv4,
                        const uint32_t* host_route_idx, const uint64_t* host_seed,
                        sg_hosts** out);
/* Copy RNG state (4 u64 per host, Xoshiro s[0..3]) and event-id counters
 * (Host::event_id_counter) out of / into the device (host memory). */
int32_t sg_hosts_get_state(sg_hosts* hosts, uint64_t* rng_state, uint64_t* event_ctr);
int32_t sg_hosts_set_state(sg_hosts* hosts, const uint64_t* rng_state, const uint64_t* event_ctr);
/* Advance hosts' device RNG streams by steps[i] next_u64 steps each (host
 * arrays, n entries, host_ids[i] < n_hosts; a host may repeat): the steps other
 * consumers took (see sg_packets.rng_skip) that no later packet has carried to
 * the device yet -- e.g. before sg_hosts_get_state for a checkpoint. */
int32_t sg_hosts_skip(sg_hosts* hosts, uint32_t n, const uint32_t* host_ids, const uint64_t* steps);
void sg_hosts_destroy(sg_hosts* hosts);

/* Routing-table shard resident on the device (rows [row_begin, row_begin+n_rows)).
 * path_key (optional, from sg_table_pack) holds each cell as one u64,
 * (latency_ns << 32) | bits(packet_loss): the delivery walk then gathers one
 * 8-byte word per packet instead of two scattered words.  When path_key is
 * set, latency_ns / packet_loss are not read by the delivery calls and may be
 * NULL.  NULL = use the two arrays. */
typedef struct sg_table {
  const uint64_t* latency_ns; /* device, n_rows x n_cols */
  const float* packet_loss;   /* device, n_rows x n_cols */
  uint32_t n_cols;
  uint32_t row_begin;
  uint32_t n_rows;
  const uint64_t* path_key;   /* device, n_rows x n_cols, or NULL */
} sg_table;

/* ABI 7: per-pair packet counters on the device.  RoutingInfo::increment_packet_count
 * (graph/mod.rs:451-459), which Worker::send_packet calls for every delivered
 * packet (worker.rs:373): with counters set, every sg_deliver_round /
 * sg_deliver_source on this context adds one to counts[cell] for each packet it
 * delivers, cell = the path's cell of the table it was given ((route row -
 * row_begin) * n_cols + destination column).  counts: device u64, n_cells >=
 * the table's n_rows * n_cols, zeroed by the caller (the reference's counters
 * start empty); NULL turns counting off (the default).  The reference
 * saturates its u64; a u64 count of packets cannot reach it. */
int32_t sg_ctx_set_packet_counters(sg_ctx* ctx, uint64_t* counts, uint64_t n_cells);

/* Pack a table's (latency_ns, packet_loss) cells into path_key form
 * (out_key: device, n_rows x n_cols u64).  *out_packable (host) = 1 if every
 * latency is below 2^32 ns, else 0 and out_key must not be used (latencies of
 * 4.29 s and more keep the two-array form).  Synchronises.  Done once per
 * routing table (the table is immutable for the simulation, network_graph.rs
 * IpPreviewTable / RoutingInfo are built once in Manager::run). */
int32_t sg_table_pack(sg_ctx* ctx, const sg_table* table, uint64_t* out_key, uint32_t* out_packable);

/* Round clock (EmulatedTime ns).  round_end = the worker's barrier
 * (worker.rs:262-268); sim_end / bootstrap_end from WorkerShared. */
typedef struct sg_round {
  uint64_t round_end_ns;
  uint64_t sim_end_ns;
  uint64_t bootstrap_end_ns;
} sg_round;

/* One round's sent packets, device SoA, grouped by ascending source host and
 * in each host's send order (the order Worker::send_packet saw them).
 *
 * rng_skip (optional, NULL = none): the host's Xoshiro stream is shared with
 * other consumers on the CPU -- Host::random_mut() (host.rs:645-647) is also
 * drawn by getrandom (syscall/handler/random.rs:40), socket port choices
 * (socket.rs:179-858), host_rngDouble / host_rngNextNBytes (host.rs:1288-1300)
 * and the auxv random bytes (managed_thread.rs:248).  rng_skip[i] = the number
 * of next_u64 steps those consumers took on packet i's source host since the
 * previous packet of that host handed to the device (in this batch or an
 * earlier one).  The device advances the host's stream by that many steps
 * before packet i (whatever its status), so every packet draws at exactly the
 * stream position Worker::send_packet (worker.rs:360) drew from.  The CPU keeps
 * its own copy of the stream in step by taking one step per packet that draws
 * (now < sim_end and the destination resolves, worker.rs:332-360): no state
 * crosses the bus per round. */
typedef struct sg_packets {
  uint32_t n_packets;
  const uint32_t* src_host;     /* HostId of the sending host */
  const uint32_t* dst_ipv4;     /* destination address (host byte order) */
  const uint32_t* payload_len;  /* PacketRc::payload_len (packet.rs:394-396) */
  const uint64_t* send_time_ns; /* Worker::current_time() at the send */
  const uint32_t* rng_skip;     /* device, n_packets, or NULL (see above) */
} sg_packets;

enum {
  SG_PKT_DELIVERED = 0,  /* PacketStatus::InetSent; pushed to the destination queue */
  SG_PKT_DROP_LOSS = 1,  /* InetDropped by the reliability draw (worker.rs:365-368) */
  SG_PKT_DROP_NO_DST = 2,/* InetDropped: unknown destination, no draw (worker.rs:341-351) */
  SG_PKT_SIM_END = 3     /* now >= sim_end: ignored, no draw (worker.rs:332-335) */
};

/* Device outputs. */
typedef struct sg_deliveries {
  uint8_t* status;           /* n_packets, SG_PKT_* */
  uint64_t* deliver_time_ns; /* n_packets (0 unless delivered) */
  uint64_t* event_id;        /* n_packets, src_host_event_id (UINT64_MAX unless delivered) */
  uint32_t* dst_order;       /* n_packets capacity: delivered packet indices bucketed by
                                destination, each bucket in EventQueue pop order */
  uint32_t* dst_offsets;     /* n_hosts + 1 */
} sg_deliveries;

typedef struct sg_round_stats {
  uint64_t n_delivered;
  uint64_t min_deliver_time_ns; /* Worker::update_next_event_time input min (worker.rs:388) */
  uint64_t min_used_latency_ns; /* Worker::update_lowest_used_latency input min (worker.rs:372) */
} sg_round_stats;

/* Run one round.  Updates the hosts' RNG streams and event counters on the
 * device.  `stats` (host) may be NULL.  The call synchronises once either way: it
 * reads the round's error flags and whether a destination overfilled its region
 * (then it sorts again and synchronises a second time).
 * A batch that is not grouped by ascending source host (SG_ERR_UNSORTED), names
 * a host out of range, or comes from a host whose route row is outside the
 * table shard (SG_ERR_INVALID_ARG) is rejected whole: no host's RNG stream or
 * event counter changes and no output is written.  SG_ERR_TIME_OVERFLOW (the
 * reference panics) leaves the hosts' state undefined. */
int32_t sg_deliver_round(sg_ctx* ctx, sg_hosts* hosts, const sg_table* table,
                         const sg_round* round, const sg_packets* packets, sg_deliveries* out,
                         sg_round_stats* stats);

/* ---- sharded delivery (one process per GPU, exchange between the calls) ---
 * Hosts are partitioned over ranks; a rank sends for the hosts whose routing
 * rows it holds and receives for the hosts it owns.
 *   1. sg_deliver_source: the send_packet half for this rank's packets
 *      (same per-packet outputs and RNG/counter updates as sg_deliver_round),
 *      plus one sg_record per delivered packet, grouped by the destination's
 *      owner rank host_owner[dst] (send_counts[r] records for rank r, in rank
 *      order).  Synchronises (the counts are needed for the exchange).
 *   2. the caller exchanges records (all-to-all, e.g. RCCL over xGMI).
 *   3. sg_deliver_bucket: the push_packet_to_host half on the owner: bucket
 *      the received records by local destination slot host_local[dst] and
 *      order each bucket as the EventQueue pops it (deliver time, src host,
 *      event id).  dst_order holds indices into `recv`.                     */
typedef struct sg_record {
  uint64_t deliver_time_ns;
  uint64_t order_key; /* (src_host << 32) | k, k = rank among src_host's delivered packets this round */
  uint64_t event_id;  /* src_host_event_id */
  uint32_t packet;    /* index in the source rank's sg_packets */
  uint32_t dst_host;  /* HostId of the destination */
} sg_record;

int32_t sg_deliver_source(sg_ctx* ctx, sg_hosts* hosts, const sg_table* table, const sg_round* round,
                          const sg_packets* packets, uint8_t* status, uint64_t* deliver_time_ns,
                          uint64_t* event_id, const uint32_t* host_owner, uint32_t n_ranks,
                          sg_record* send, uint32_t* send_counts, sg_round_stats* stats);
int32_t sg_deliver_bucket(sg_ctx* ctx, const sg_record* recv, uint32_t n_records,
                          const uint32_t* host_local, uint32_t n_hosts, uint32_t n_local_hosts,
                          uint32_t* dst_order, uint32_t* dst_offsets);

/* ---- link loads from a round's packets (additive to ABI 7) ------------------
 * What sg_link_load gives for a run's counter matrix, for one round's batch and
 * with a weight per packet: every counted packet walks its tree path through the
 * pred rows of sg_routing_tree and adds its weight to each link and node on it.
 * Cost in proportion to packets x hops; no n x n matrix, no node limit.  Links
 * and their order are those of sg_net_links.
 *
 * `nodes` / n_nodes as for sg_link_load (a permutation of the net's nodes);
 * `pred` holds rows [row_begin, row_end) as sg_routing_tree writes them,
 * row-major from row_begin.  packets->src_host and packets->dst_ipv4 are read:
 * device arrays as for sg_deliver_round, but no grouping by source host is
 * required.  `status`: device, n_packets SG_PKT_* values, what sg_deliver_round
 * or sg_deliver_source wrote; a packet counts iff its status is
 * SG_PKT_DELIVERED; NULL: every packet counts.  `weight`: device u32 per packet
 * (payload_len, or a total size the caller computed); NULL: 1.  Every counted
 * packet is walked, whatever its weight.  Per counted packet p: row i =
 * host_route_idx[src_host[p]], column j = the route index of the host that
 * dst_ipv4[p] resolves to (the delivery walk's address map), s = nodes[i], d =
 * nodes[j], w = its weight:
 *   d == s:  out_link_load[link (s, s)] += w, hops = 1 (get_edge_weight's
 *            self-loop rule, as sg_link_load treats the diagonal)
 *   else, for every v on the tree path from d up to (excluding) s in row i:
 *            out_link_load[link (pred_i[v], v)] += w, out_node_load[v] += w;
 *            hops = the number of such v
 *   out_hops[p] = hops; UINT32_MAX for a packet that does not count.
 * All sums are u64, WRAP, and are ADDED to what the arrays hold: row blocks,
 * ranks, group members and successive rounds sum into one array.  Any output may
 * be NULL, but not all three.  SG_ROUTE_OUT_DEVICE applies to pred and the three
 * outputs, as in sg_link_load; without it they are host arrays (the library
 * uploads pred and adds the device sums into the host arrays).  The packet
 * arrays, status and weight are always device memory.  Synchronises once.
 * For weight == NULL, out_link_load and out_node_load equal what sg_link_load
 * gives on the counters sg_ctx_set_packet_counters collected for the same round.
 * SG_ERR_INVALID_ARG, the outputs untouched, for NULL arguments, hosts or net of
 * another context, n_nodes other than the net's, `nodes` not a permutation, a bad
 * row range, no output at all.  Found on the device (SG_ERR_INVALID_ARG with a
 * message, the outputs then undefined; never a trap, never a loop: every walk is
 * bounded by n_nodes steps), packet kinds first, sg_ctx_last_error_pair =
 * (smallest failing packet index, UINT32_MAX): a source host >= the host count,
 * a source whose route row lies outside [row_begin, row_end) (both for every
 * packet, counted or not), a counted packet whose address does not resolve, a
 * resolved route index >= n_nodes.  Then pred kinds, sg_ctx_last_error_pair =
 * the smallest (row, col) in row-major order over all failing packets: a value
 * >= n_nodes or a (pred, node) pair that is not a link (col = the column of the
 * node at which the walk failed), a walk that has not reached s after n_nodes
 * steps (a cycle; col = the packet's destination column).  Only cells that some
 * counted packet's path crosses are validated; pred[s] is not read.
 * Timers: "link_packets" (work = packets walked); read_timer(
 * "link_packets_counted") gives the packets the last call counted. */
int32_t sg_link_load_packets(sg_ctx* ctx, sg_net* net, sg_hosts* hosts,
                             const uint32_t* nodes, uint32_t n_nodes,
                             uint32_t row_begin, uint32_t row_end, uint32_t flags,
                             const uint32_t* pred,
                             const sg_packets* packets, const uint8_t* status,
                             const uint32_t* weight,
                             uint64_t* out_link_load, uint64_t* out_node_load,
                             uint32_t* out_hops);

/* ---- batched tree paths: per-pair and per-packet hop lists (additive to ABI 7) --
 * The links a path crosses, kept instead of summed: the device batch form of
 * sg_tree_path.  A HOP RECORD is one link crossed.  For source row i (s =
 * nodes[i]) and destination column j (d = nodes[j]):
 *   d != s: the tree path s = v0, v1, ..., vh = d in row i's pred row gives h
 *           records in SOURCE-TO-DESTINATION order; record k (1 <= k <= h) holds
 *             node        = vk (petgraph index)
 *             link        = the number of link (v(k-1), vk) in sg_net_links order
 *             latency_ns  = latency_ns [i][pos[vk]]   (pos = the inverse of nodes)
 *             packet_loss = packet_loss[i][pos[vk]]
 *           the cumulative (latency, loss) at a hop is the row's own table cell
 *           of the intermediate node, bit for bit.  The source itself is implicit.
 *   d == s: one record, as sg_link_load_packets counts that case: node = s, link =
 *           the self-loop link (s, s), latency_ns / packet_loss = the diagonal
 *           cell (get_edge_weight's rule).
 * A packet that does not count (status other than SG_PKT_DELIVERED) has no record.
 * So a counted packet's record count is sg_link_load_packets' out_hops[p], and for
 * d != s, s followed by the pair's out_node entries is what sg_tree_path returns.
 *
 * Output (CSR, deterministic): out_off has n + 1 u64 entries (n = n_pairs or
 * packets->n_packets), out_off[0] = 0; pair or packet p owns records
 * [out_off[p], out_off[p + 1]).  out_node u32, out_link u32, out_latency_ns u64,
 * out_packet_loss f32, each of capacity `cap` records; any may be NULL, not all
 * four.  out_latency_ns needs the latency_ns rows [row_begin, row_end) as the
 * build wrote them (row-major from row_begin), out_packet_loss the packet_loss
 * rows; an output requested without its input is SG_ERR_INVALID_ARG, and an input
 * whose output is NULL is not read.  With out_link == NULL no link is looked up
 * and a (pred, node) pair that is not a link is not reported.  *total always
 * receives the record count.  total > cap: SG_ERR_CAPACITY, out_off and *total
 * complete, nothing written to the record arrays; grow them and call again.  A
 * sizing call passes at least one real record array and takes that error.
 *
 * sg_tree_paths: the pairs as (pair_row[p], pair_col[p]), row and column indices
 * in `nodes` order.  SG_ROUTE_OUT_DEVICE applies to pred, the table rows, the
 * pair arrays and every output alike; without it all of them are host arrays,
 * which the library stages as sg_link_load_packets does.
 * sg_tree_paths_packets: the pairs of a round's packets exactly as in
 * sg_link_load_packets (row = host_route_idx[src_host[p]], column through the
 * hosts' address map); the packet arrays and status are always device memory.
 * `total` is a host pointer in either form.  Synchronises twice.
 *
 * SG_ERR_INVALID_ARG, every output untouched, for NULL arguments, a net or hosts
 * of another context, n_nodes other than the net's, `nodes` not a permutation, a
 * bad row range, no record output.  Found on the device (SG_ERR_INVALID_ARG with
 * a message, the outputs then undefined; never a trap, never a loop: every walk
 * ends after n_nodes steps, a value >= n_nodes is caught before it forms an
 * index): pair or packet kinds first, sg_ctx_last_error_pair = (smallest failing
 * index, UINT32_MAX): a source host >= the host count, a row outside
 * [row_begin, row_end), a column or route index >= n_nodes, a counted packet
 * whose address does not resolve.  Then pred kinds, the smallest (row, col) in
 * row-major order: a value >= n_nodes (col = the column of the node at which the
 * walk failed) or a walk that has not reached s after n_nodes steps (a cycle; col
 * = the destination column), both found while counting, ahead of a (pred, node)
 * pair that is not a link (col = the node's column), found while filling.  Only
 * cells that some path crosses are validated; pred[s] is not read.
 * Timers: "tree_paths_count" and "tree_paths_fill" (work = records), and
 * "tree_paths_scan" (work = pairs or packets). */
int32_t sg_tree_paths(sg_ctx* ctx, sg_net* net, const uint32_t* nodes, uint32_t n_nodes,
                      uint32_t row_begin, uint32_t row_end, uint32_t flags,
                      const uint32_t* pred, const uint64_t* latency_ns, const float* packet_loss,
                      uint32_t n_pairs, const uint32_t* pair_row, const uint32_t* pair_col,
                      uint64_t* out_off, uint32_t* out_node, uint32_t* out_link,
                      uint64_t* out_latency_ns, float* out_packet_loss,
                      uint64_t cap, uint64_t* total);
int32_t sg_tree_paths_packets(sg_ctx* ctx, sg_net* net, sg_hosts* hosts,
                              const uint32_t* nodes, uint32_t n_nodes,
                              uint32_t row_begin, uint32_t row_end, uint32_t flags,
                              const uint32_t* pred, const uint64_t* latency_ns, const float* packet_loss,
                              const sg_packets* packets, const uint8_t* status,
                              uint64_t* out_off, uint32_t* out_node, uint32_t* out_link,
                              uint64_t* out_latency_ns, float* out_packet_loss,
                              uint64_t cap, uint64_t* total);

/* ---- link trace: a round's packets per link, in time order (additive to ABI 7) --
 * The crossings of sg_tree_paths_packets grouped by LINK and sorted by time: which
 * packets crossed a link, and when.  Pairs, counting rule, `nodes`, `pred`, the
 * latency_ns rows, the row block and the address resolution are exactly as in
 * sg_tree_paths_packets; latency_ns is always required (the order depends on it),
 * packet_loss is not taken, packets->send_time_ns is read.
 * A TRACE RECORD is one (counted packet p, link crossed).  Packet p has row i,
 * source s, destination d and the tree path s = v0, ..., vh = d; cum(v) =
 * latency_ns[i][pos[v]], cum(s) = 0:
 *   d != s: hop k (1 <= k <= h) gives one record on link (v(k-1), vk):
 *             packet   = p
 *             hop      = k
 *             enter_ns = send_time_ns[p] + cum(v(k-1))
 *             exit_ns  = send_time_ns[p] + cum(vk)
 *   d == s: one record on the self-loop link (s, s): hop = 1, enter_ns =
 *           send_time_ns[p], exit_ns = send_time_ns[p] + the diagonal cell.
 * So record out_off[p] + hop - 1 of sg_tree_paths_packets is the same crossing.
 *
 * Output: links are numbered in sg_net_links order.  out_link_off (required) has
 * n_links + 1 u64 entries, out_link_off[0] = 0; link L owns records
 * [out_link_off[L], out_link_off[L + 1]) in ascending (enter_ns, packet) order.  A
 * tree path crosses a link at most once, so the key is unique and the output is a
 * function of the inputs alone.  out_packet u32, out_hop u32, out_enter_ns u64,
 * out_exit_ns u64, each of capacity `cap` records; any may be NULL, not all four.
 * watch: NULL, or n_links u8; a link with watch[L] == 0 gets an empty segment and
 * counts nothing towards *total, its crossings are still walked and validated.
 * total > cap: SG_ERR_CAPACITY, out_link_off and *total complete, nothing written
 * to the record arrays (the contract of sg_tree_paths, its sizing call included).
 * With no packets out_link_off is all zero and *total = 0.
 *
 * SG_ROUTE_OUT_DEVICE applies to pred, latency_ns, watch and every output alike;
 * without it they are host arrays, staged as the sibling calls stage theirs.  The
 * packet arrays and status are always device memory, `total` a host pointer.
 * Synchronises twice.
 *
 * Errors: precedence and sg_ctx_last_error_pair as in sg_tree_paths_packets.
 * Argument errors (those of sg_tree_paths_packets; NULL latency_ns or
 * send_time_ns) leave every output untouched.  Packet kinds come first, the
 * smallest failing packet as (packet, UINT32_MAX); to its kinds one is added, the
 * last of them: a counted packet whose send_time_ns + latency_ns[i][j] passes
 * 2^64 - 1 gives SG_ERR_TIME_OVERFLOW (no earlier hop can overflow when the
 * destination's sum does not: arc latency is at least 1 ns, cum rises along the
 * path).  Then the pred kinds: a value >= n_nodes or a cycle, ahead of a (pred,
 * node) pair that is not a link; every crossing is looked up, so a non-link is
 * reported whichever outputs are NULL and whether or not a link is watched.  Every
 * walk ends after n_nodes steps: never a trap, never a loop.
 * Timers: "link_trace_count", "link_trace_fill", "link_trace_sort" (work =
 * records). */
int32_t sg_link_trace_packets(sg_ctx* ctx, sg_net* net, sg_hosts* hosts,
                              const uint32_t* nodes, uint32_t n_nodes,
                              uint32_t row_begin, uint32_t row_end, uint32_t flags,
                              const uint32_t* pred, const uint64_t* latency_ns,
                              const sg_packets* packets, const uint8_t* status,
                              const uint8_t* watch,
                              uint64_t* out_link_off,
                              uint32_t* out_packet, uint32_t* out_hop,
                              uint64_t* out_enter_ns, uint64_t* out_exit_ns,
                              uint64_t cap, uint64_t* total);

/* ---- link time series: bytes per link per time bin (additive to ABI 7) ---------
 * How busy each link was over time: the crossings of sg_link_trace_packets, each
 * adding its packet's weight into one (slot, time bin) cell of a matrix that stays
 * on the device across rounds.  No record is kept and nothing is sorted.  Pairs,
 * counting rule, `nodes`, `pred`, the latency_ns rows, the row block, address
 * resolution, link numbering, the crossings and their enter_ns / exit_ns are exactly
 * those of sg_link_trace_packets; `weight` is sg_link_load_packets' (device u32 per
 * packet; NULL: 1).  For every crossing of a counted packet p (weight w) on link L:
 *   slot  s = link_slot[L].  link_slot has n_links u32 entries; NULL is the
 *         identity, and n_slots must then equal n_links.  UINT32_MAX: the link is
 *         not watched; its crossing is walked and validated all the same.  Several
 *         links may share a slot (both directions of an edge, a cut set).
 *   time  t = enter_ns for at == SG_SERIES_AT_ENTER, exit_ns for SG_SERIES_AT_EXIT.
 *   cell  t < t0_ns:  out_outside[2 s] += w.  Else q = (t - t0_ns) / bin_ns, the
 *         exact u64 quotient (bins closed below, open above):
 *         q < n_bins:  out_series[s * n_bins + q] += w;
 *         otherwise:   out_outside[2 s + 1] += w.
 *         q is compared as a 64-bit value, and the decision is by the quotient, not
 *         by an end time: t0_ns + n_bins * bin_ns may pass 2^64.
 * All sums are u64, WRAP, and are ADDED to what the arrays hold: row blocks, group
 * members and successive rounds sum into one matrix.  out_series (n_slots * n_bins
 * u64) is required; out_outside (2 * n_slots u64) may be NULL.
 * IDENTITY: for every slot s, the sum over b of out_series[s][b], plus
 * out_outside[2 s] + out_outside[2 s + 1], equals the sum of sg_link_load_packets'
 * out_link_load[L] over the links L of that slot, for either value of `at`.
 *
 * SG_ROUTE_OUT_DEVICE applies to pred, latency_ns, link_slot and both outputs;
 * without it they are host arrays, staged as sg_link_load_packets stages its own
 * (the device sums start at zero and are added into the host arrays).  The packet
 * arrays, status and weight are always device memory.  Synchronises once.
 *
 * SG_ERR_INVALID_ARG, every output untouched: the argument errors of
 * sg_link_trace_packets; bin_ns, n_bins or n_slots zero; at > 1; NULL out_series;
 * NULL link_slot with n_slots != n_links; in host mode a slot value >= n_slots
 * other than UINT32_MAX, sg_ctx_last_error_pair = (link, UINT32_MAX).  Found on the
 * device (the outputs then undefined, as in sg_link_load_packets; never a trap,
 * never a loop, and no index is ever formed from a bad value): first a bad slot
 * value in device mode, the smallest such link of the whole map as (link,
 * UINT32_MAX), which the walk treats as not watched; then the packet kinds of
 * sg_link_trace_packets, SG_ERR_TIME_OVERFLOW the last of them; then the pred kinds
 * with sg_link_load_packets' precedence: the smallest (row, col) in row-major order
 * among a value >= n_nodes, a non-link and a cycle.
 * Timers: "link_series" (work = packets walked); read_timer("link_series_counted")
 * gives the packets the last call counted, read_timer("link_series_lds") whether
 * it summed in per-workgroup LDS matrices (1) or straight into memory (0), and
 * n_slots * (n_bins + 2), the cells that choice is made by (SG_LINK_SERIES_LDS). */
#define SG_SERIES_AT_ENTER 0
#define SG_SERIES_AT_EXIT 1
int32_t sg_link_series_packets(sg_ctx* ctx, sg_net* net, sg_hosts* hosts,
                               const uint32_t* nodes, uint32_t n_nodes,
                               uint32_t row_begin, uint32_t row_end, uint32_t flags,
                               const uint32_t* pred, const uint64_t* latency_ns,
                               const sg_packets* packets, const uint8_t* status,
                               const uint32_t* weight,
                               const uint32_t* link_slot, uint32_t n_slots, uint32_t at,
                               uint64_t t0_ns, uint64_t bin_ns, uint32_t n_bins,
                               uint64_t* out_series, uint64_t* out_outside);

/* ---- link queues: FIFO wait per crossing under a link rate (additive to ABI 7) --
 * What a link trace would look like if each link served only so many bytes a
 * second: how long every crossing waits, when it is done, how deep the queue is
 * when it arrives, and which links cannot keep up.  Input is a link trace in the
 * format of sg_link_trace_packets and sg_group_link_trace_packets: link_off has
 * n_links + 1 u64 entries, enter_ns n_records u64, packet n_records u32.  Further:
 *   weight        u32, n_weights entries, indexed by packet[i]; NULL: 1 per record,
 *                 and packet may then be NULL too.
 *   cost_ps       u64, n_links entries: picoseconds of service per weight unit
 *                 (with byte weights 1 Gbit/s is 8,000 and 100 Gbit/s is 80); 0: the
 *                 link serves in no time.
 *   link_free_in  u64, n_links entries, or NULL (all 0): the time each link's
 *                 server becomes free.
 * Link L owns records [link_off[L], link_off[L + 1]).  Taking them in the order
 * given, with `done` starting at link_free_in[L]:
 *   s_i     = min(ceil(w_i * cost_ps[L] / 1000), 2^64 - 1)   (the product exact)
 *   start_i = max(enter_i, done)
 *   done    = min(start_i + s_i, 2^64 - 1)                   -> done_i
 *   wait_i  = start_i - enter_i
 *   ahead_i = #{ j < i in the segment : done_j > enter_i }   (the records still in
 *             the system when i arrives)
 * The recurrence does not require a segment to be sorted: the result is a function
 * of the arrays as given (a trace's segments are in ascending (enter_ns, packet)
 * order, which is a FIFO queue's arrival order).
 * Outputs, all optional, at least one required.  Per record: out_wait_ns u64,
 * out_done_ns u64, out_ahead u32.  Per link, n_links entries each:
 *   out_link_free         u64: done of the link's last record, link_free_in[L] for
 *                         an empty segment; it must not alias link_free_in
 *   out_link_busy_ns      u64: the sum of s_i
 *   out_link_wait_max_ns  u64
 *   out_link_wait_sum_ns  u64, wraps
 *   out_link_ahead_max    u32
 * An empty segment has 0 in the last four.  n_records == 0 is legal.
 * FIRST ORDER, unless SG_LINK_QUEUE_CARRY is set (below): a wait is not propagated
 * to the packet's later hops; enter_ns downstream is the trace's.
 * CHAINING out_link_free into a later call's
 * link_free_in equals one call over both calls' records only when every record of
 * the later call arrives after every record of the earlier one on its link.
 *
 * SG_ROUTE_OUT_DEVICE applies to every array argument alike; without it all
 * arrays are host arrays, staged.  Synchronises once.
 *
 * SG_ERR_INVALID_ARG, every output untouched: NULL ctx, link_off, enter_ns or
 * cost_ps; no output; weight without packet; out_link_free == link_free_in; in
 * host mode a bad link_off, sg_ctx_last_error_pair = (link, UINT32_MAX), the
 * smallest such link: link_off[0] != 0 is link 0, link_off[L + 1] < link_off[L]
 * is link L, link_off[n_links] != n_records is link n_links.
 * Found on the device (the outputs then undefined; never a trap, and no index is
 * ever formed from a bad value), in this order: a bad link_off in device mode, as
 * above; packet[i] >= n_weights, SG_ERR_INVALID_ARG with the pair (link, i -
 * link_off[link]) of the smallest such i; done_i reaching 2^64 - 1,
 * SG_ERR_TIME_OVERFLOW with the same kind of pair, the smallest i.
 * Timers: "link_queue" (work = records), "link_queue_ahead".
 *
 * SG_LINK_QUEUE_CARRY in flags: every wait is carried to the packet's later hops.
 * Without the flag the call is what it was, bit for bit, with the same launches.
 * Inputs.  packet is required.  n_weights is the number of packets: it bounds
 * packet[i] whether or not weight is NULL.  enter_ns is the uncongested schedule;
 * the library only reads it.
 * A packet's chain.  The records with equal packet value, taken in ascending input
 * enter_ns, are that packet's chain.  gap_i = enter_ns[next(i)] - enter_ns[i] is the
 * uncongested time from entering record i's link to entering the link of the
 * packet's next record; it must be at least 1 (in a real trace it is the link
 * latency; with `watch` it is the link latency plus the latencies of the unwatched
 * links in between, so an unwatched link behaves as a link of infinite rate with
 * no extra work).  No hop or exit_ns argument is needed.
 * Carried times.  enter'_i = enter_ns[i] for the first record of a chain,
 * enter'_next(i) = done_i + gap_i otherwise: store and forward, service is paid on
 * every link.
 * Each link's queue.  Link L serves its records in ascending (enter', packet)
 * order, not in the order given.  The recurrence is unchanged, starting from
 * link_free_in[L]: start = max(enter', done), done = start + s, wait = start -
 * enter'; ahead is the number of records earlier in that order with done_j >
 * enter'_i; s is exactly the value above.  (A packet's chain visits a link once, as
 * a tree path does: two records of one packet on one link have no order here.)
 * Outputs.  The result is the unique solution of these equations: what an
 * event-driven simulation yields when it processes arrivals in global (time,
 * packet) order.  Outputs keep their meaning and their index: out_wait_ns[i],
 * out_done_ns[i] and out_ahead[i] belong to input record i, so the result does not
 * depend on the order in which a link's records are given.  out_link_free[L] is the
 * done of the record served last; the per-link sums are over the carried
 * schedule.  With every cost_ps 0 and no link_free_in, enter' = enter_ns and all
 * waits are 0; a chain of one record per packet gives the result above for sorted
 * segments.  The carried enter time of record i is done_i - s_i - wait_i.
 * The call iterates (sort every link by the carried times, scan, carry done + gap
 * to the next record) until no time moves, and SYNCHRONISES ONCE PER ITERATION; an
 * iteration settles at least the smallest gap of simulated time.
 * SG_LINK_QUEUE_CARRY_ITERS (default 4096) bounds the iterations: reaching it is an
 * error, never a partial answer.
 * Errors with the flag.  Every output untouched: NULL packet, SG_ERR_INVALID_ARG;
 * n_records > 2^32 - 2, SG_ERR_CAPACITY.  Found on the device (outputs undefined,
 * never a trap, no index formed from a bad value), in this order: a bad link_off;
 * packet[i] >= n_weights, both as above; two records of one packet with equal
 * enter_ns, SG_ERR_INVALID_ARG with the pair (link, i - link_off[link]) of the
 * smallest such record index i; done or done + gap reaching 2^64 - 1,
 * SG_ERR_TIME_OVERFLOW, pair unspecified; not converged within the bound,
 * SG_ERR_CAPACITY with the pair (iterations run, UINT32_MAX).
 * Timers with the flag: "link_queue_index" (the chains), "link_queue_sort",
 * "link_queue" (the scan), "link_queue_carry" (the propagate step),
 * "link_queue_ahead"; read_timer("link_queue_iters") gives the iterations of the
 * last carried call.
 *
 * SG_LINK_QUEUE_DROP in flags: every link has a finite buffer and drops at its tail.
 * Without the flag the call is what it was, bit for bit, with the same launches.
 * Inputs.  cost_ps has 2 * n_links entries: limit_ns[L] = cost_ps[n_links + L] is the
 * longest wait link L's buffer holds, the unfinished work a record may find, measured
 * in service time.  2^64 - 1: no limit; 0: a record is dropped whenever it would wait
 * at all.  With byte weights a buffer of B bytes in front of the server is
 * min(ceil(B * cost_ps[L] / 1000), 2^64 - 1).  In host mode 2 * n_links entries are
 * staged.
 * Each link's queue, in the order served (the order given; with SG_LINK_QUEUE_CARRY
 * ascending (enter', packet) over the records that arrive), `done` starting at
 * link_free_in[L]:
 *   start_i = max(enter_i, done)
 *   start_i - enter_i > limit_ns[L]:  record i is DROPPED, done is unchanged
 *   otherwise record i is SERVED:     done = min(start_i + s_i, 2^64 - 1) -> done_i,
 *                                     wait_i = start_i - enter_i
 * with s_i exactly the value above.  ahead_i counts served records only: the earlier
 * served records of the link's order with done_j > enter_i.
 * With SG_LINK_QUEUE_CARRY the chain successor of a dropped or absent record is
 * ABSENT: it enters no queue.  Apart from that the equations are the carried ones,
 * and the result is what an event-driven simulation in global (time, packet) order
 * yields.
 * Outputs.  There is no new array: a record's state is read from values a served
 * record cannot produce.
 *   state     out_wait_ns   out_done_ns               out_ahead
 *   served    as above      as above                  as above (served only)
 *   dropped   2^64 - 1      its (carried) enter time  the served records it found
 *   absent    2^64 - 1      2^64 - 1                  0
 * out_link_free[L] is the done of the record served last, link_free_in[L] when none
 * was served.  Busy, wait max, wait sum and ahead max run over served records only.
 * out_link_ahead_max then has 2 * n_links entries: [n_links + L] is the number of
 * records dropped on L (u32).  out_link_busy_ns then has 2 * n_links entries:
 * [n_links + L] is the sum of s_i over the records dropped on L (wraps).  Absent
 * records count nowhere; an empty link has 0 in both second halves.
 * With every limit 2^64 - 1 the flagged call equals the unflagged one in every
 * first-half output, with or without SG_LINK_QUEUE_CARRY, and the second halves are 0.
 * The carried enter time of a served record is done_i - s_i - wait_i, of a dropped
 * record out_done_ns[i], of an absent record 2^64 - 1.
 * Errors with the flag are unchanged in kind and order, and n_records > 2^32 - 2 is
 * SG_ERR_CAPACITY, every output untouched.  SG_ERR_TIME_OVERFLOW is raised by served
 * records only: a served done, or with SG_LINK_QUEUE_CARRY done + gap, reaching
 * 2^64 - 1; a dropped record never overflows.  SG_LINK_QUEUE_CARRY_ITERS bounds the
 * iterations as above.
 * Timers with the flag: "link_queue" (the walk), "link_queue_ahead" (the outputs).
 *
 * SG_LINK_QUEUE_PACKETS in flags: the result is folded onto the packets -- each packet's
 * delay under the rates, its arrival, and the record where it was dropped.  The bit
 * composes with SG_ROUTE_OUT_DEVICE, SG_LINK_QUEUE_CARRY and SG_LINK_QUEUE_DROP in every
 * combination.  Without it the call is what it was, bit for bit, with the same
 * launches; with it the first n_records entries of the per-record outputs and every
 * per-link output equal the call without it.
 * Inputs.  packet is required.  n_weights is the number of packets P: it bounds
 * packet[i] whether or not weight is NULL.  enter_ns has n_records + P entries:
 * enter_ns[n_records + p] = base_p is packet p's uncongested arrival time (a delivery
 * round's deliver_time_ns[p]); the library only reads it.  In host mode n_records + P
 * entries are staged.
 * Outputs.  out_wait_ns, out_done_ns and out_ahead are all required and have
 * n_records + P entries each; behind the records:
 *   out_wait_ns[n_records + p] = delay(p)
 *   out_done_ns[n_records + p] = arrive(p)
 *   out_ahead[n_records + p]   = where(p)
 * Definition.  R(p) is the set of records with packet[i] == p.  A record's state is
 * read as above: served; dropped (wait 2^64 - 1, done not); absent (both 2^64 - 1);
 * without SG_LINK_QUEUE_DROP every record is served.  All times here are the input
 * enter_ns, not the carried ones.
 *   drop(p)   the dropped record of R(p) with the smallest enter_ns, the smallest index
 *             among equals; t_drop its enter_ns, +infinity when R(p) has none.
 *   S(p)      the served records of R(p) with enter_ns < t_drop: what a first-order
 *             result serves downstream of a drop does not count.
 *   where(p)  the record index of drop(p); 0xFFFFFFFE when p arrived (R(p) is not empty
 *             and nothing of it was dropped); 0xFFFFFFFF when R(p) is empty (the packet
 *             was not counted, or it crossed no watched link).
 *   delay(p)  with SG_LINK_QUEUE_CARRY done_l - enter_ns[l] for the record l of S(p)
 *             with the largest enter_ns (the chain's waits and services telescope into
 *             it); without, the sum over S(p) of done_i - enter_ns[i], wrapping: the
 *             first-order sum of what each link adds.  0 when S(p) is empty.
 *   arrive(p) 2^64 - 1 when p was dropped, else base_p + delay(p).  A packet with no
 *             record keeps base_p whatever its value.
 * Errors with the bit.  Every output untouched: a NULL packet, out_wait_ns,
 * out_done_ns or out_ahead, SG_ERR_INVALID_ARG; n_records > 2^32 - 2, SG_ERR_CAPACITY
 * (the two codes of where are the top two u32 values).  Found on the device, after
 * the errors above and in their order, with their pairs: packet[i] >= n_weights (now
 * also without weight); base_p + delay(p) of a packet that arrived reaching 2^64 - 1,
 * SG_ERR_TIME_OVERFLOW, the pair names a record of that packet, which one is
 * unspecified.  No index is formed from a flagged value.
 * The packet pass runs after the outputs stand and before the flag words are read; with
 * SG_LINK_QUEUE_CARRY they are read once more after it.
 * Timers with the bit: "link_queue_packets" (work = records);
 * read_timer("link_queue_lost") gives the packets the last such call found dropped,
 * and P.
 *
 * SG_LINK_QUEUE_WINDOW in flags: the carried form is settled up to a horizon H only, and the
 * rest comes back as pending, in the form a later call takes as input: rounds queue
 * behind one another.  The bit requires SG_LINK_QUEUE_CARRY and composes with
 * SG_LINK_QUEUE_DROP, SG_LINK_QUEUE_PACKETS and SG_ROUTE_OUT_DEVICE in every combination.
 * Without it the call is what it was, bit for bit, with the same launches.
 * Input.  link_free_in is required and has n_links + 1 entries:
 * link_free_in[n_links] = H (host mode stages n_links + 1 entries).
 * n_records <= 2^32 - 3.
 * Definition.  The closed solution is the result of the same call without the bit
 * (the carried form, with the drop rule if flagged); e'_i is record i's carried enter
 * time there.  A record is settled when it is served or dropped in the closed solution
 * and e'_i < H (strict), or when it is absent and the dropped record of its chain is
 * itself settled.  Every other record is pending: e'_i >= H, or absent behind a drop
 * that is not settled.  A packet's settled records are a prefix of its chain.  A link
 * serves in (e', packet) order, and a record's start, its drop decision and its done
 * depend on earlier records of that order alone: the settled records' values depend
 * neither on the pending records nor on any record a later call adds at or after H,
 * and the library never computes the closed solution past H.
 * Outputs.  A settled record gets the values it gets without the bit.  A pending
 * record gets out_wait_ns = 2^64 - 1, out_ahead = 0xFFFFFFFF and out_done_ns = r_i, its
 * re-based enter time: for the first pending record h of a chain r_h = enter_ns[h]
 * when h is the chain's first record, else e'_h = done + gap of its predecessor (exact:
 * the predecessor is settled and served); for every later one r_next(i) = r_i + gap_i.
 * The per-link outputs run over settled records only, the second halves under
 * SG_LINK_QUEUE_DROP too; out_link_free[L] is the done of the last settled served record
 * of L, link_free_in[L] when there is none.  out_ahead counts this call's settled
 * served records only: a crossing still in service from an earlier call is seen
 * through link_free_in alone, so out_ahead and out_link_ahead_max of a sequence of
 * calls are lower bounds of the closed solution's.
 * With SG_LINK_QUEUE_PACKETS a packet with a pending record is in flight: where(p) =
 * 0xFFFFFFFD, delay(p) = r_h - enter_ns[h] for its first pending record h (what the
 * queues have added so far; 0 when h is its chain's first) and arrive(p) = base_p +
 * delay(p), the re-based base.  Every other packet is as without the bit;
 * read_timer("link_queue_lost") counts settled drops only.
 * Two identities.  (1) With H = 2^64 - 1 the call equals the one without the bit in
 * every output.  (2) Re-feeding: call 1 runs over records R at H1; call 2 runs at H2
 * >= H1 over call 1's pending records (enter_ns = r, base = call 1's re-based base,
 * their weights), the in-flight packets renumbered in their old relative order, new
 * records N, all with enter_ns >= H1, their packets numbered after the in-flight
 * ones, and link_free_in = call 1's out_link_free.  The settled outputs of both calls
 * together are then the closed solution's values for every record of R and N with e' <
 * H2, the packets of N numbered after those of R.  By induction a sequence of rounds
 * that ends at H = 2^64 - 1 equals one carried call over the concatenated trace.
 * Errors keep their kinds, order and pairs.  Every output untouched: the bit without
 * SG_LINK_QUEUE_CARRY, or a NULL link_free_in, SG_ERR_INVALID_ARG; n_records > 2^32 - 3,
 * SG_ERR_CAPACITY (after the two).  A re-based time or an in-flight packet's
 * re-based base reaching 2^64 - 1 is SG_ERR_TIME_OVERFLOW, pair unspecified; an
 * overflow of the closed solution past H is not found.  No index is formed from an
 * unchecked value.
 * The call synchronises once per iteration, as the carried form does; an iteration
 * sorts and scans only the records whose carried time is below H.  With t_min the
 * smallest enter_ns below H and g_min the smallest gap, iterations <= ceil((H -
 * t_min) / g_min) + 1.  Timers with the bit: the carried form's, over the records
 * sorted, and "link_queue_window" (the compaction and the scatter);
 * read_timer("link_queue_iters") as before; read_timer("link_queue_active") gives the
 * records sorted and scanned, summed over the call's iterations, and n_records.
 *
 * SG_LINK_QUEUE_SERIES in flags: the result gets a time axis -- under the rates, per slot of
 * watched links and per time bin, the server's busy time, the time-integral of the waiting
 * queue, the weight served and the weight dropped, summed on the device into a matrix that
 * stays there across calls and rounds.  The bit composes with SG_ROUTE_OUT_DEVICE,
 * SG_LINK_QUEUE_CARRY, SG_LINK_QUEUE_DROP, SG_LINK_QUEUE_PACKETS and SG_LINK_QUEUE_WINDOW in every
 * combination.  Without it the call is what it was, bit for bit, with the same launches;
 * with it every other output equals the call without it.
 * Input.  Let c0 = n_links (2 * n_links with SG_LINK_QUEUE_DROP).  cost_ps has four more u64
 * entries: cost_ps[c0] = t0_ns, cost_ps[c0 + 1] = bin_ns, cost_ps[c0 + 2] = n_bins (B),
 * cost_ps[c0 + 3] = n_slots.  n_slots == 0 is the identity map, S = n_links.  Otherwise S =
 * n_slots and n_links more entries follow: cost_ps[c0 + 4 + L] is link L's slot, a value
 * below S, or 2^64 - 1 for a link that is not watched; several links may share a slot.
 * Host mode stages the tail too.
 * Output.  out_wait_ns, out_done_ns and out_link_busy_ns are required, with
 * SG_LINK_QUEUE_WINDOW out_ahead as well (it tells a pending record from a dropped one).
 * out_link_busy_ns has c0 + 4 * S * (B + 2) entries; behind the per-link values lies
 * M[k][s][c] = out_link_busy_ns[c0 + (k * S + s) * (B + 2) + c]: plane k in 0..3, slot s,
 * column c in 0..B-1 for the bin T_c = [t0 + c * bin_ns, t0 + (c + 1) * bin_ns), column B for
 * the time before t0_ns, column B + 1 for the time at or after t0 + B * bin_ns.  All interval
 * arithmetic is as if unbounded: t0 + B * bin_ns may pass 2^64, and the decision is by the
 * quotient, as in sg_link_series_packets.
 * For every record i of a watched link with slot s the pass reads the call's own result;
 * w_i = weight[packet[i]] (1 when weight is NULL), s_i the service time as above.
 *   served   start_i = done_i - s_i, e'_i = start_i - wait_i (first order: enter_ns[i]).
 *            plane 0, busy_ns:  column c gets |[start_i, done_i) ∩ T_c|
 *            plane 1, wait_ns:  column c gets |[e'_i, start_i) ∩ T_c|
 *            plane 2, served:   the column of done_i gets w_i
 *   dropped  plane 3, dropped:  the column of e'_i (= out_done_ns[i]) gets w_i
 *   absent, pending: nothing.
 * Plane 0 divided by bin_ns is the link's utilisation in that bin, plane 1 divided by bin_ns
 * its mean number waiting.  All sums are u64 and wrap.  In device mode they are ADDED to what M
 * holds; in host mode the device sums start at zero and are added into the host array's tail
 * (the head is written as before).  n_records == 0 is legal and leaves M as it is.
 * IDENTITIES.  For every slot, summed over its links and over all B + 2 columns: plane 0
 * equals out_link_busy_ns[L]; plane 1 equals out_link_wait_sum_ns[L] mod 2^64; with unit
 * weights plane 3 equals the drop counts out_link_ahead_max[n_links + L] and plane 2 the
 * number served.  From a zeroed matrix a slot of one link has M[0][s][c] <= bin_ns for c < B.
 * With SG_LINK_QUEUE_WINDOW only settled records count, each with the closed solution's values:
 * the matrices of a sequence of re-fed calls that ends at H = 2^64 - 1 sum to the matrix of
 * one carried call over the concatenated trace, bit for bit.
 * Errors with the bit.  Found on the host, every output untouched, after the argument errors
 * above and before link_off's check, in this order: the bit without out_wait_ns, out_done_ns
 * or out_link_busy_ns, or with SG_LINK_QUEUE_WINDOW and no out_ahead, SG_ERR_INVALID_ARG;
 * bin_ns == 0 or n_bins == 0, SG_ERR_INVALID_ARG; n_bins or n_slots >= 2^32, or S * (B + 2) >
 * 2^31, SG_ERR_CAPACITY; in host mode a slot value >= S other than 2^64 - 1,
 * SG_ERR_INVALID_ARG with the pair (link, UINT32_MAX), the smallest such link.  In device
 * mode the four header words are READ BACK BEFORE THE FIRST LAUNCH: one more synchronisation.
 * Found on the device, after every error the call has without the bit: a bad slot value of
 * a link that has a record, reported as above; it is treated as not watched, and no index is
 * formed from it.
 * The pass runs after the outputs stand at the input indices and before the flag words are
 * read; with SG_LINK_QUEUE_CARRY they are read once more after it.  Its cost per record does
 * not depend on the bins a wait or a service spans.
 * Timers with the bit: "link_queue_series" (work = records);
 * read_timer("link_queue_series_cells") gives S * (B + 2). */
#define SG_LINK_QUEUE_CARRY 0x4u
#define SG_LINK_QUEUE_DROP 0x8u
#define SG_LINK_QUEUE_PACKETS 0x10u
#define SG_LINK_QUEUE_WINDOW 0x20u
#define SG_LINK_QUEUE_SERIES 0x40u
int32_t sg_link_queue(sg_ctx* ctx, uint32_t flags, uint32_t n_links,
                      const uint64_t* link_off, uint64_t n_records,
                      const uint64_t* enter_ns, const uint32_t* packet,
                      const uint32_t* weight, uint32_t n_weights,
                      const uint64_t* cost_ps, const uint64_t* link_free_in,
                      uint64_t* out_wait_ns, uint64_t* out_done_ns, uint32_t* out_ahead,
                      uint64_t* out_link_free, uint64_t* out_link_busy_ns,
                      uint64_t* out_link_wait_max_ns, uint64_t* out_link_wait_sum_ns,
                      uint32_t* out_link_ahead_max);

/* ---- sharded delivery with a fixed-split exchange (no host round trip) ----
 * The same round as sg_deliver_source / sg_deliver_bucket, with every rank's
 * records for rank r in a block of `cap` slots, so the exchange is one
 * equal-split all-to-all the host need not size (RCCL over xGMI), and the round
 * synchronises once, at its end.  `cap` must be the same on every rank (e.g.
 * derived from the largest pair count of the round before).
 *   1. sg_deliver_source_padded: the source half; rank r's k-th record goes to
 *      send_padded[r * cap + k] if k < cap, else to its compact position in
 *      `send` (n_packets records, as sg_deliver_source's).  xrow (device,
 *      3 + n_ranks u64) = [delivered, min deliver time, min used latency,
 *      records for rank 0, 1, ...].  Does not synchronise.
 *   2. the caller all-gathers xrow into xall (n_ranks x (3 + n_ranks)) and
 *      all-to-alls send_padded (cap records per rank pair) into recv_padded.
 *   3. sg_deliver_bucket_padded: buckets the valid records of every block (block
 *      b holds min(xall[b][3 + rank], cap)); dst_order indexes recv_padded.
 *      stats = the round's global values; recv_counts[b] = records rank b sent
 *      this rank; pair_max = the largest count any rank sent any rank.  If
 *      pair_max > cap, some records did not fit: every rank sees the same xall,
 *      so all of them then run sg_deliver_pad_to_compact (the complete compact
 *      `send`), the exact exchange of sg_deliver_source's protocol with the
 *      counts from xall, and sg_deliver_bucket.                                */
int32_t sg_deliver_source_padded(sg_ctx* ctx, sg_hosts* hosts, const sg_table* table, const sg_round* round,
                                 const sg_packets* packets, uint8_t* status, uint64_t* deliver_time_ns,
                                 uint64_t* event_id, const uint32_t* host_owner, uint32_t n_ranks, uint32_t cap,
                                 sg_record* send_padded, sg_record* send, uint64_t* xrow);
int32_t sg_deliver_bucket_padded(sg_ctx* ctx, const sg_record* recv_padded, uint32_t n_ranks, uint32_t cap,
                                 const uint64_t* xall, uint32_t rank, const uint32_t* host_local, uint32_t n_hosts,
                                 uint32_t n_local_hosts, uint32_t* dst_order, uint32_t* dst_offsets,
                                 sg_round_stats* stats, uint32_t* recv_counts, uint32_t* pair_max);
int32_t sg_deliver_pad_to_compact(sg_ctx* ctx, const sg_record* send_padded, uint32_t n_ranks, uint32_t cap,
                                  const uint64_t* xrow, sg_record* send);

/* ---- collectives of the sharded path over RCCL (ABI 7) --------------------
 * One communicator per rank (one process per GPU), bound to an sg_ctx: every call
 * is enqueued on the context's stream, after the library's kernels, and returns
 * without synchronising.  They replace the hand-offs between the reference's
 * worker threads (Worker::push_packet_to_host, worker.rs:597-607, run from the
 * manager's round loop, manager.rs:415-501) and the routing table every worker
 * reads (NetworkGraph::compute_shortest_paths, graph/mod.rs:183-228, computed once,
 * sim_config.rs:137-141) once rows and hosts are sharded over GPUs.  RCCL is
 * opened at run time (librccl.so.1); without it these return SG_ERR_UNSUPPORTED
 * and everything else works.
 *   sg_comm_unique_id: on one rank; the caller passes the bytes to every rank.
 *   sg_comm_allgather_rows: in place, rank r's rows [r rows_per_rank, (r + 1)
 *     rows_per_rank) of the n_used-column table (device lat u64 / loss f32; either
 *     may be NULL) to every rank.
 *   sg_comm_exchange_padded: step 2 of the fixed-split round above: xrow (3 +
 *     n_ranks u64, device) all-gathered into xall, and cap records per rank pair
 *     from send_padded to recv_padded (n_ranks blocks each).
 *   sg_comm_alltoallv_records: the exact exchange of sg_deliver_source's records
 *     (grouped by rank: send_counts[r] for rank r), received rank after rank;
 *     send_counts / recv_counts are host arrays of n_ranks.
 *   sg_comm_allgather_u64: n u64 per rank (device) into all (n_ranks x n).   */
typedef struct sg_comm sg_comm;
#define SG_COMM_ID_BYTES 128
int32_t sg_comm_unique_id(uint8_t* id /* SG_COMM_ID_BYTES */);
int32_t sg_comm_create(sg_ctx* ctx, const uint8_t* id, uint32_t n_ranks, uint32_t rank, sg_comm** out);
void sg_comm_destroy(sg_comm* comm);
int32_t sg_comm_allgather_rows(sg_comm* comm, uint64_t* lat, float* loss, uint32_t rows_per_rank, uint32_t n_used);
int32_t sg_comm_exchange_padded(sg_comm* comm, const sg_record* send_padded, sg_record* recv_padded, uint32_t cap,
                                const uint64_t* xrow, uint64_t* xall);
int32_t sg_comm_alltoallv_records(sg_comm* comm, const sg_record* send, const uint32_t* send_counts,
                                  sg_record* recv, const uint32_t* recv_counts);
int32_t sg_comm_allgather_u64(sg_comm* comm, const uint64_t* mine, uint64_t* all, uint32_t n);

/* ---- router inbound CoDel queues (one per host) ---------------------------
 * Router::inbound_packets (router/mod.rs:15-58): each host's CoDelQueue
 * (router/codel_queue.rs), RFC 8289 with Shadow's TARGET = 10 ms,
 * INTERVAL = 100 ms, no LIMIT, MTU = 1500 (definitions.h:124).  The queues
 * and their CoDel state live on the device across calls.  A call runs a batch
 * of push / pop events: each host's events in its order (hosts are
 * independent, so the batch runs one device lane per host).
 *   push(packet, len, now)  = CoDelQueue::push (codel_queue.rs:303-317)
 *   pop(now) -> packet|none = CoDelQueue::pop  (codel_queue.rs:125-148),
 *                             dropping as the control law dictates.      */
typedef struct sg_codel sg_codel;
enum { SG_CODEL_PUSH = 0, SG_CODEL_POP = 1 };
enum { SG_CODEL_QUEUED = 0, SG_CODEL_DEQUEUED = 1, SG_CODEL_DROPPED = 2 /* PacketStatus::RouterDropped */ };

/* ring_cap: packets a host's queue may hold (rounded up to a power of two);
 * a push beyond it fails the call with SG_ERR_CAPACITY (the reference has no
 * limit, so size it for the workload). */
int32_t sg_codel_create(sg_ctx* ctx, uint32_t n_hosts, uint32_t ring_cap, sg_codel** out);
void sg_codel_destroy(sg_codel* q);

typedef struct sg_codel_events { /* device arrays, grouped by ascending host */
  uint32_t n_events;
  const uint32_t* host;
  const uint8_t* kind;     /* SG_CODEL_PUSH | SG_CODEL_POP */
  const uint64_t* time_ns; /* EmulatedTime of the operation (Worker::current_time) */
  const uint32_t* packet;  /* push: the caller's packet id (< n_packets below) */
  const uint32_t* len;     /* push: PacketRc::len() (packet.rs:388-390) */
} sg_codel_events;

/* pop_result (device, n_events): the popped packet id, UINT32_MAX for an
 * empty pop and for pushes.  pkt_status (device, n_packets): set to
 * SG_CODEL_DEQUEUED / SG_CODEL_DROPPED when a packet leaves its queue.
 * n_dropped (host, may be NULL): packets CoDel dropped in this call. */
int32_t sg_codel_run(sg_ctx* ctx, sg_codel* q, const sg_codel_events* ev, uint32_t* pop_result,
                     uint8_t* pkt_status, uint32_t n_packets, uint64_t* n_dropped);

/* Copy the per-host state out of / into the device (host arrays, n_hosts
 * each; ring_* n_hosts * ring_cap): flags (bit 0 drop mode, bit 1
 * interval_end set, bit 2 drop_next set), interval_end, drop_next, current /
 * previous drop count, bytes stored, ring head / tail counters, and the ring
 * (packet, enqueue time, len).  For checkpoints and tests. */
typedef struct sg_codel_state {
  uint8_t* flags;
  uint64_t *interval_end, *drop_next, *cur_drops, *prev_drops, *bytes;
  uint32_t *head, *tail;
  uint32_t* ring_packet;
  uint64_t* ring_time;
  uint32_t* ring_len;
} sg_codel_state;
uint32_t sg_codel_ring_cap(const sg_codel* q);
int32_t sg_codel_get_state(sg_codel* q, sg_codel_state* out);
int32_t sg_codel_set_state(sg_codel* q, const sg_codel_state* in);

/* ---- inbound pipeline: router CoDel queue -> relay_inet_in (token bucket) --
 * Host::execute on a Packet event (host.rs:781-786): the packet enters the
 * router's CoDel queue and the inbound relay is notified; the relay
 * (relay/mod.rs:72-288) forwards from the queue to the host's internet
 * interface as its token bucket allows (relay/token_bucket.rs: refill
 * max(1, bw_down_bytes / 1000) every 1 ms, capacity refill + MTU,
 * relay/mod.rs:296-309), rescheduling itself when blocked.  A call processes
 * one host's arrivals (a delivery round's buckets, in EventQueue order) and the
 * relay's forward tasks up to window_end; later tasks stay pending.  Assumes
 * Shadow's CPU-delay model is off (host.rs:758-775; its default).           */
typedef struct sg_inbound sg_inbound;
/* bw_down_bits (host, n_hosts): each host's bandwidth down (HostInfo, bits/s). */
int32_t sg_inbound_create(sg_ctx* ctx, uint32_t n_hosts, const uint64_t* bw_down_bits, uint32_t ring_cap,
                          sg_inbound** out);
void sg_inbound_destroy(sg_inbound* ib);
uint32_t sg_inbound_ring_cap(const sg_inbound* ib);

typedef struct sg_inbound_arrivals { /* device arrays, grouped by ascending host, EventQueue order */
  uint32_t n;
  const uint32_t* host;
  const uint64_t* time_ns; /* the Packet event's time (the delivery's arrival), < window_end */
  const uint32_t* packet;  /* the caller's packet id (< n_packets) */
  const uint32_t* len;     /* PacketRc::len() */
} sg_inbound_arrivals;

/* Packet ids are below n_packets <= 2^31: SG_ERR_INVALID_ARG otherwise, for an id at or past
 * n_packets as soon as it enters a queue (sg_inbound_run) or would stay queued past the call
 * (sg_inbound_run_ordered).
 * event_ctr (device, n_hosts, may be NULL): each host's event-id counter,
 * advanced by one per forward task the relay schedules (host.rs:649-653) --
 * e.g. sg_hosts_event_ctr(hosts).  fwd_time (device, n_packets): the time the
 * relay pushed the packet to the interface; pkt_status (device, n_packets):
 * SG_CODEL_DEQUEUED once forwarded, SG_CODEL_DROPPED if CoDel dropped it.
 * n_dropped (host, may be NULL): CoDel drops in this call. */
int32_t sg_inbound_run(sg_ctx* ctx, sg_inbound* ib, const sg_inbound_arrivals* arr, uint64_t window_end_ns,
                       uint64_t bootstrap_end_ns, uint64_t sim_end_ns, uint64_t* event_ctr, uint64_t* fwd_time,
                       uint8_t* pkt_status, uint32_t n_packets, uint64_t* n_dropped);

/* ABI 7: the same call with each arrival's fate written in arrival order
 * (RelayForwarded / drop_packet of relay/mod.rs:201-273 and
 * codel_queue.rs:125-148, at the arrival's index instead of its packet id, so
 * a host's outputs are consecutive).  arr_status (device, arr->n): set to
 * SG_CODEL_DEQUEUED / SG_CODEL_DROPPED when arrival i of this call leaves its
 * queue in this call, untouched while it stays queued (the caller zeroes it:
 * SG_CODEL_QUEUED); arr_fwd_time (device, arr->n): the forward time of a
 * DEQUEUED arrival, untouched otherwise.  Packets that arrived in earlier calls
 * and leave in this one still go to pkt_status / fwd_time by packet id
 * (n_packets covers every id).  arr->n < 2^31. */
int32_t sg_inbound_run_ordered(sg_ctx* ctx, sg_inbound* ib, const sg_inbound_arrivals* arr, uint64_t window_end_ns,
                               uint64_t bootstrap_end_ns, uint64_t sim_end_ns, uint64_t* event_ctr,
                               uint64_t* fwd_time, uint8_t* pkt_status, uint32_t n_packets, uint64_t* arr_fwd_time,
                               uint8_t* arr_status, uint64_t* n_dropped);

typedef struct sg_inbound_relay_state { /* host arrays, n_hosts each */
  uint8_t* flags;          /* bit 0 a forward task is pending, bit 1 it was never queued (>= sim_end),
                              bit 2 a packet is cached (RelayCached) */
  uint64_t* task_time;
  uint32_t *cached_packet, *cached_len;
  uint64_t *tb_capacity, *tb_balance, *tb_increment, *tb_last_refill;
  /* ABI 6 (may be NULL): the pending forward task's Local event id
     (Host::get_new_event_id, host.rs:649-653, taken from event_ctr when the
     task was scheduled) and the time it was scheduled at (its creation). */
  uint64_t *task_event_id, *task_created_ns;
} sg_inbound_relay_state;
int32_t sg_inbound_get_state(sg_inbound* ib, sg_codel_state* queue, sg_inbound_relay_state* relay);

/* ---- outbound pipeline: network interface -> relay_inet_out -> router ------
 * The send side of the relay.  A socket with data joins
 * its interface's sending queue and relay_inet_out is notified
 * (Host::notify_socket_has_packets, host.rs:930-945; interface.rs:168-182).
 * Under the default fifo qdisc the interface pops the socket whose next packet
 * has the smallest priority (interface.rs:225-260, queuing.rs:16-36), so
 * packets leave in creation order: a host's sends are one FIFO.  The relay
 * (relay/mod.rs:111-275) pops and forwards while its token bucket allows
 * (bw_up: refill max(1, bw_up_bytes / 1000) every 1 ms, capacity refill + MTU,
 * relay/mod.rs:278-319; no limit while bootstrapping).  A packet addressed to
 * the host's own address goes back to the interface without using tokens
 * (is_local, :222-226, :259-264); any other one goes to the router, whose push
 * is Worker::send_packet at the forward task's time (router/mod.rs:41-43).
 * Those packets form an sg_packets batch for sg_deliver_round.
 *
 * A call processes each host's sends (times < window_end, nondecreasing per
 * host) and the relay's forward tasks before window_end; later tasks stay
 * pending.  Assumes Shadow's CPU-delay model is off (host.rs:758-775; its
 * default).
 *
 * Same-time order.  A send happens while the host runs some event E; the
 * relay's forward task is a Local event (relay/mod.rs:145-157).  At one
 * EmulatedTime the host runs Packet events first, then Local events by event
 * id (event.rs:84-155, :163-183), and ids grow in creation order
 * (host.rs:649-653).  With sends->event_id given, a task at time t runs before
 * a send at t iff E is a Local event created after the task:
 * (event_created_ns, event_id) > (task created, task id), the task's id taken
 * from event_ctr when it is scheduled.  event_id = UINT64_MAX marks E as a
 * Packet event (it precedes every Local one).  Creation time decides first
 * because ids are monotone in creation order, so the comparison is exact
 * whenever the two were created at different times, whatever numbering the
 * caller's own ids use within a window; at one creation time it falls back
 * to the ids.  Without event_id (NULL) every send at t
 * precedes a task at t (all sends treated as Packet-event sends).          */
typedef struct sg_outbound sg_outbound;
/* host_ipv4, bw_up_bits (host, n_hosts): each host's address and bandwidth up
 * (HostInfo, bits/s).  ring_cap bounds, per host and call, the packets queued
 * at the start (a cached one included) plus the call's sends; more fails the
 * call with SG_ERR_CAPACITY. */
int32_t sg_outbound_create(sg_ctx* ctx, uint32_t n_hosts, const uint32_t* host_ipv4, const uint64_t* bw_up_bits,
                           uint32_t ring_cap, sg_outbound** out);
void sg_outbound_destroy(sg_outbound* ob);
uint32_t sg_outbound_ring_cap(const sg_outbound* ob);

typedef struct sg_outbound_sends { /* device arrays, grouped by ascending host, interface order */
  uint32_t n;
  const uint32_t* host;
  const uint64_t* time_ns;      /* when the socket handed the packet to the interface, < window_end */
  const uint32_t* packet;       /* the caller's packet id (< n_packets) */
  const uint32_t* len;          /* PacketRc::len() (packet.rs:388-390): the bucket's cost */
  const uint32_t* payload_len;  /* PacketRc::payload_len(): carried into the sent batch */
  const uint32_t* dst_ipv4;
  /* ABI 6, optional (NULL, or both): the sending event's id and the time it was
     created (scheduled).  event_id UINT64_MAX: a Packet event.  Sends at one time
     come in the host's execution order: Packet-event sends first, then by
     (event_created_ns, event_id).  Requires event_ctr in sg_outbound_run. */
  const uint64_t* event_id;
  const uint64_t* event_created_ns;
} sg_outbound_sends;

enum { SG_OUT_QUEUED = 0, SG_OUT_SENT = 1 /* to the router: Worker::send_packet */,
       SG_OUT_LOCAL = 2 /* dst == own address: back to the interface */ };

/* The packets this call handed to send_packet, device arrays of capacity
 * `cap`, grouped by ascending host and in each host's send order: the
 * sg_packets of a delivery round (src_host, dst_ipv4, payload_len,
 * send_time_ns), plus the caller's packet id. */
typedef struct sg_outbound_sent {
  uint32_t cap;
  uint32_t *src_host, *dst_ipv4, *payload_len;
  uint64_t* send_time_ns;
  uint32_t* packet;
} sg_outbound_sent;

/* event_ctr (device, n_hosts, may be NULL): advanced by one per forward task
 * scheduled (host.rs:649-653).  fwd_time / pkt_status (device, n_packets): the
 * forward time and SG_OUT_SENT / SG_OUT_LOCAL of each packet the relay
 * forwarded (untouched otherwise).  sent may be NULL; n_sent (host, may be
 * NULL) receives the count.  SG_ERR_CAPACITY if sent->cap is too small. */
int32_t sg_outbound_run(sg_ctx* ctx, sg_outbound* ob, const sg_outbound_sends* sends, uint64_t window_end_ns,
                        uint64_t bootstrap_end_ns, uint64_t sim_end_ns, uint64_t* event_ctr, uint64_t* fwd_time,
                        uint8_t* pkt_status, uint32_t n_packets, sg_outbound_sent* sent, uint32_t* n_sent);

/* Host arrays: per host the ring head / tail counters and n_hosts * ring_cap
 * slots (packet, len, payload_len, dst).  A cached packet (relay flags bit 2)
 * is the slot at head - 1. */
typedef struct sg_outbound_queue_state {
  uint32_t *head, *tail;
  uint32_t *ring_packet, *ring_len, *ring_payload_len, *ring_dst;
} sg_outbound_queue_state;
int32_t sg_outbound_get_state(sg_outbound* ob, sg_outbound_queue_state* queue, sg_inbound_relay_state* relay);

/* ---- the interface's queueing discipline (additive to ABI 7) ----------------
 * experimental.interface_qdisc (QDiscMode, configuration.rs:971-973) selects how
 * the interface picks the next sending socket (host/network/interface.rs:97-108):
 * fifo, above, or round-robin, a NetworkQueueKind::FirstInFirstOut over sockets
 * (host/network/queuing.rs).  Per host, round-robin keeps a deque of socket ids
 * without duplicates (send_sockets and its membership set) and a FIFO of packets
 * per socket:
 *   a send of packet p on socket s   appends p to s's FIFO; pushes s to the deque's
 *                                    back unless s is already in it (add_data_source,
 *                                    interface.rs:168-181); notifies the relay as
 *                                    under fifo;
 *   pop() (interface.rs:227-259)     takes s from the deque's front and s's oldest
 *                                    packet; pushes s to the back if it still holds a
 *                                    packet (counting the sends processed before this
 *                                    pop in the host's execution order); an empty
 *                                    deque is an idle interface.
 * The relay's forward loop, its cached packet (already popped: its socket has
 * already rotated), the token bucket and the bootstrap exemption, local packets,
 * the sim_end rule, the event-counter advances and the keyed same-time order are
 * those of sg_outbound_run (relay/mod.rs:111-273).  With one socket per host, or a
 * socket per packet, round-robin is the fifo order.
 *
 * max_sockets: the socket slots per host, rounded up to a power of two
 * (sg_outbound_max_sockets returns that); 0 or more than SG_QDISC_MAX_SOCKETS is
 * SG_ERR_INVALID_ARG, as is an unknown qdisc.  ring_cap keeps sg_outbound_create's
 * contract.  sg_outbound_create(...) is sg_outbound_create_qdisc(..., SG_QDISC_FIFO, 1). */
enum { SG_QDISC_FIFO = 0, SG_QDISC_ROUND_ROBIN = 1 };
enum { SG_QDISC_MAX_SOCKETS = 256 };
int32_t sg_outbound_create_qdisc(sg_ctx* ctx, uint32_t n_hosts, const uint32_t* host_ipv4,
                                 const uint64_t* bw_up_bits, uint32_t ring_cap, uint32_t qdisc, uint32_t max_sockets,
                                 sg_outbound** out);
uint32_t sg_outbound_qdisc(const sg_outbound* ob);
uint32_t sg_outbound_max_sockets(const sg_outbound* ob);

/* sg_outbound_run with each send's socket: socket (device, sends->n) is the
 * caller's per-host slot index of the sending socket, below
 * sg_outbound_max_sockets(ob) (SG_ERR_INVALID_ARG with a message of its own
 * otherwise).  A slot is only a queue index: it may be given to another socket
 * once it has drained.  On a fifo object `socket` is ignored (it may be NULL) and
 * the call is sg_outbound_run; on a round-robin object sg_outbound_run itself is
 * SG_ERR_INVALID_ARG.  Every other argument and error is sg_outbound_run's, in
 * the same precedence (the socket check comes after the host checks).  The sent
 * batch has sg_outbound_run's layout: grouped by ascending host, each host's
 * packets in forward order, send_time_ns the forward time. */
int32_t sg_outbound_run_qdisc(sg_ctx* ctx, sg_outbound* ob, const sg_outbound_sends* sends, const uint32_t* socket,
                              uint64_t window_end_ns, uint64_t bootstrap_end_ns, uint64_t sim_end_ns,
                              uint64_t* event_ctr, uint64_t* fwd_time, uint8_t* pkt_status, uint32_t n_packets,
                              sg_outbound_sent* sent, uint32_t* n_sent);

/* A round-robin object's interfaces in a canonical form that does not depend on
 * how the library stores them (host arrays, any may be NULL).  Per host h: the
 * deque front to back is active[h * max_sockets + j], j < n_active[h], and
 * active_count[...] the packets each of those sockets holds; the n_queued[h]
 * queued packets are q_*[h * ring_cap + i], listed socket by socket in deque
 * order, each socket's in FIFO order; cached_*[h] is the relay's cached packet
 * (zeros unless relay flags bit 2).  Entries past n_active / n_queued are not
 * written.  On a round-robin object sg_outbound_get_state's queue half is
 * SG_ERR_INVALID_ARG (its relay half works as before); on a fifo object this
 * call's queue half is. */
typedef struct sg_outbound_qdisc_state {
  uint32_t *n_active, *active, *active_count;
  uint32_t* n_queued;
  uint32_t *q_packet, *q_len, *q_payload_len, *q_dst;
  uint32_t *cached_packet, *cached_len, *cached_payload_len, *cached_dst;
} sg_outbound_qdisc_state;
int32_t sg_outbound_get_qdisc_state(sg_outbound* ob, sg_outbound_qdisc_state* q, sg_inbound_relay_state* relay);

/* The device array of the hosts' event-id counters (Host::event_id_counter). */
uint64_t* sg_hosts_event_ctr(sg_hosts* hosts);

/* ---- packets in flight: every host's Packet events between delivery and arrival ----
 * The reference's per-host EventQueue restricted to Packet events, on the device:
 * WorkerShared::push_packet_to_host (worker.rs:597-607) puts a delivered packet
 * into its destination's queue; Host::execute(until) pops every event with
 * time < until (host.rs:753-757) in the order of event.rs:84-155, which for
 * Packet events of one host is (time, src_host, event_id).  A delivery round's
 * output goes in with sg_wire_push, a window's arrivals come out with
 * sg_wire_pop in the form sg_inbound_run_ordered takes, and no packet crosses
 * the bus while it waits (a 50 ms latency under a 1 ms runahead: ~50 rounds).
 * The key (host, time, src_host, event_id) is unique, so what a pop returns
 * depends only on the set of events held, never on the order they were pushed
 * in.  On the sharded path (one rank per GPU) the owner rank pushes the records
 * it received: see "the wire on the sharded path" below.  Additive to ABI 7. */
typedef struct sg_wire sg_wire; /* every host's in-flight Packet events, on the device */

/* capacity: events the store may hold (at most 2^31).  bin_ns >= 1 and n_bins
 * (rounded up to a power of two, at least 2, at most 1024): the geometry of the
 * store's calendar -- a ring of n_bins bins of bin_ns each, later events on a far
 * list that is re-binned as the ring advances; they affect speed only, never
 * results (fastest with n_bins * bin_ns past the largest latency, the far list
 * empty, and bin_ns about a round).  One exception, which only a calendar
 * shorter than the latencies can meet: re-binning writes the far list again
 * beside itself, and the store's memory is 1.25 x capacity records, so a pop
 * that must re-bin (window_end has reached the ring's end) while events held +
 * events on the far list exceed about 1.1 x capacity fails with
 * SG_ERR_CAPACITY, the store unchanged; size capacity for both then.
 * SG_ERR_INVALID_ARG for a zero n_hosts, capacity or bin_ns. */
int32_t sg_wire_create(sg_ctx* ctx, uint32_t n_hosts, uint64_t capacity, uint64_t bin_ns, uint32_t n_bins,
                       sg_wire** out);
void sg_wire_destroy(sg_wire* w);
/* Events held, as the host knows it without a device call: exact after
 * sg_wire_pop / get_state / set_state; each push since adds its n_packets. */
uint64_t sg_wire_count(const sg_wire* w);

/* WorkerShared::push_packet_to_host for a whole delivery round: one event per
 * packet i with out->status[i] == SG_PKT_DELIVERED, i.e. per entry of
 * out->dst_order: (destination host = the bucket of out->dst_order /
 * dst_offsets holding i, time = out->deliver_time_ns[i], src_host =
 * packets->src_host[i], event_id = out->event_id[i], packet = packet_id ?
 * packet_id[i] : id_base + i, len = len[i]).  packet_id (device, n_packets, may
 * be NULL); len (device, n_packets): PacketRc::len() (packet.rs:388-390).
 * A packet whose out->deliver_time_ns[i] is 2^64 - 1 adds no event (no event
 * carries that time: EMUTIME_MAX is 2^64 - 2).  That is how a round under link
 * rates leaves out the packets its queues dropped: out->deliver_time_ns is then
 * sg_link_queue's arrive tail (SG_LINK_QUEUE_PACKETS).  sg_wire_count counts such a
 * packet until the next pop, as it counts dropped packets.
 * w was created for the hosts table's n_hosts.  SG_ERR_INVALID_ARG for NULL
 * arguments; SG_ERR_CAPACITY when sg_wire_count + packets->n_packets exceeds
 * the capacity (checked on the host, so dropped packets count: conservative);
 * on either the store is unchanged.  Does not synchronise. */
int32_t sg_wire_push(sg_ctx* ctx, sg_wire* w, const sg_packets* packets, const sg_deliveries* out,
                     const uint32_t* packet_id, uint32_t id_base, const uint32_t* len);

typedef struct sg_wire_arrivals { /* device arrays of capacity cap */
  uint32_t cap;
  uint32_t* host;
  uint64_t* time_ns;
  uint32_t* packet;
  uint32_t* len;      /* host, time_ns, packet, len: an sg_inbound_arrivals */
  uint32_t* src_host; /* src_host and event_id: both, or both NULL */
  uint64_t* event_id;
} sg_wire_arrivals;

/* Host::execute(until)'s pops, for every host: removes every event with
 * time < window_end_ns (one at window_end_ns stays) and writes them grouped by
 * ascending host, each host's in EventQueue order (time, src_host, event_id).
 * window_end_ns need not grow from call to call; UINT64_MAX drains the store.
 * *n_out (host): their number.  *next_time_ns (host, may be NULL): the smallest
 * time left in the store, UINT64_MAX when empty (EventQueue::next_event_time
 * over all hosts: an input of the manager's min_next_event_time).  With more
 * due events than out->cap: SG_ERR_CAPACITY, *n_out = the number needed, the
 * store unchanged.  SG_ERR_CAPACITY with a message in sg_ctx_last_error also
 * when the store's arena has no room left.  Synchronises.
 * On the sharded path this is the round's synchronising call, so it also
 * reports what sg_deliver_source_padded could not: if that call's batch was
 * rejected (SG_ERR_UNSORTED, SG_ERR_INVALID_ARG for a source host or route row
 * out of range: nothing was delivered, no record sent) or overflowed
 * (SG_ERR_TIME_OVERFLOW), and no sg_deliver_bucket_padded has reported it, the
 * first pop on the context afterwards returns that error, once.  The pop itself
 * is then complete: *n_out, *next_time_ns and out are as on SG_OK. */
int32_t sg_wire_pop(sg_ctx* ctx, sg_wire* w, uint64_t window_end_ns, sg_wire_arrivals* out, uint32_t* n_out,
                    uint64_t* next_time_ns);

/* Checkpoint: all events in canonical order (host, time, src_host, event_id)
 * into host arrays of capacity cap (SG_ERR_CAPACITY, *n = the number needed,
 * if too small); set_state replaces the contents with n events given in any
 * order.  Both synchronise. */
typedef struct sg_wire_state {
  uint32_t *host, *src_host, *packet, *len;
  uint64_t *time_ns, *event_id;
} sg_wire_state;
int32_t sg_wire_get_state(sg_wire* w, uint64_t cap, sg_wire_state* out, uint64_t* n);
int32_t sg_wire_set_state(sg_wire* w, uint64_t n, const sg_wire_state* in);

/* ---- the wire on the sharded path (additive to ABI 7) ----------------------
 * With hosts partitioned over ranks, WorkerShared::push_packet_to_host
 * (worker.rs:597-607) runs on the destination's owner, which holds only the
 * sg_records it received.  The wire needs, per event, (time, src_host, event
 * id, destination, len, packet id).  Of an sg_record's 32 bytes the owner has
 * no use for two words: k, the low half of order_key (it restarts every round;
 * the wire orders by the real, unique (time, src_host, event_id)), and
 * `packet` (an index into the SOURCE rank's batch).  The source rank writes
 * len and the caller's packet id there -- "stamps" the record -- and the record
 * then reads as an sg_wire_record.  Size and every other field are unchanged, so
 * sg_comm_exchange_padded, sg_comm_alltoallv_records and
 * sg_deliver_pad_to_compact move stamped records exactly as they move records.
 * A stamped record MUST NOT be given to sg_deliver_bucket[_padded]: its
 * order_key is no longer an order key.  A round is
 *   source rank: sg_deliver_source[_padded], sg_wire_stamp_records[_padded]
 *   exchange:    as before
 *   owner rank:  sg_wire_push_records[_padded], sg_wire_pop,
 *                sg_inbound_run_ordered
 * sg_deliver_source_padded's batch errors, which sg_deliver_bucket_padded
 * reports on the path without a wire, are returned by sg_wire_pop here.       */
typedef struct sg_wire_record {
  uint64_t deliver_time_ns;
  uint32_t len;       /* PacketRc::len() (packet.rs:388-390); was the low half of order_key */
  uint32_t src_host;  /* the high half of order_key, unchanged */
  uint64_t event_id;  /* src_host_event_id */
  uint32_t packet_id; /* the caller's packet id; was `packet` */
  uint32_t dst_host;  /* HostId of the destination */
} sg_wire_record;

/* Stamp, in place, the n_records records sg_deliver_source wrote to `send`: for
 * record k with p = send[k].packet, the low 32 bits of order_key become len[p]
 * and packet becomes packet_id ? packet_id[p] : id_base + p.  packet_id (may be
 * NULL) and len: device arrays of n_packets, as sg_wire_push's.  A record with
 * p >= n_packets is left alone.  Stamp once: a second call would read packet
 * ids as indices.  On the context's stream; does not synchronise. */
int32_t sg_wire_stamp_records(sg_ctx* ctx, sg_record* send, uint32_t n_records, const uint32_t* packet_id,
                              uint32_t id_base, const uint32_t* len, uint32_t n_packets);
/* The same after sg_deliver_source_padded, with its send_padded, send, n_ranks,
 * cap and xrow: stamps the valid slots of every block, [r cap, r cap +
 * min(xrow[3 + r], cap)), and the records past cap at their compact positions
 * in `send` (n_packets records), so that a later sg_deliver_pad_to_compact
 * yields a compact array stamped throughout.  No slot is stamped twice and none
 * outside those is touched.  The counts are read on the device: does not
 * synchronise. */
int32_t sg_wire_stamp_records_padded(sg_ctx* ctx, sg_record* send_padded, sg_record* send, uint32_t n_ranks,
                                     uint32_t cap, const uint64_t* xrow, const uint32_t* packet_id, uint32_t id_base,
                                     const uint32_t* len, uint32_t n_packets);

/* WorkerShared::push_packet_to_host (worker.rs:597-607) on the owner rank: one
 * event per stamped record of recv (device, n_records).  The event's host is
 * host_map ? host_map[dst_host] : dst_host; host_map (device, n_hosts entries,
 * may be NULL) is e.g. the partition's host_local for a wire over the rank's own
 * hosts.  Errors as sg_wire_push: SG_ERR_CAPACITY when sg_wire_count + n_records
 * exceeds the capacity, the store unchanged.  A bad destination (dst_host >=
 * n_hosts, or a host that is UINT32_MAX or not below the wire's n_hosts) cannot
 * be reported without a synchronisation: the call returns SG_OK, the store is
 * incomplete from then on, and the next sg_wire_pop (or get_state) returns
 * SG_ERR_INVALID_ARG with a message naming this call; sg_wire_set_state starts
 * the store afresh.  Does not synchronise. */
int32_t sg_wire_push_records(sg_ctx* ctx, sg_wire* w, const sg_record* recv, uint32_t n_records,
                             const uint32_t* host_map, uint32_t n_hosts);
/* The same for the blocks of a fixed-split exchange: the valid records of every
 * block of recv_padded (block b holds min(xall[b][3 + rank], cap)), xall read on
 * the device.  If the largest count in xall exceeds cap the call appends
 * NOTHING: every rank sees the same xall and runs the exact exchange, whose
 * sg_wire_push_records carries all the round's records.  The caller learns that
 * from its own copy of xall; the round's one synchronisation remains the pop's.
 * sg_wire_count rises by n_ranks * cap whatever the blocks hold (conservative,
 * as sg_wire_push's count of dropped packets; the next pop makes it exact), and
 * SG_ERR_CAPACITY is returned when that would pass the capacity. */
int32_t sg_wire_push_records_padded(sg_ctx* ctx, sg_wire* w, const sg_record* recv_padded, uint32_t n_ranks,
                                    uint32_t cap, const uint64_t* xall, uint32_t rank, const uint32_t* host_map,
                                    uint32_t n_hosts);

/* ---- device group: one process, N contexts (additive to ABI 7) --------------
 * Shadow is one process: Manager::run spawns worker threads (manager.rs:254-261) and
 * a packet crosses hosts through an in-process push (worker.rs:597-607).  A group
 * binds N contexts of that one process, usually one per GPU, so the sharded paths
 * above need neither one process per GPU nor RCCL: "member m" (the m-th context
 * given) plays the part "rank m" plays there.  Calls on one group are not
 * thread-safe, and no other call may run on a member's context meanwhile.
 *
 * create: 1 <= n <= 64 distinct contexts (64: the per-rank receive counts of a padded
 * round); devices may repeat (all members on device 0 is legal).  For every pair of
 * distinct devices peer access is checked and enabled: SG_ERR_UNSUPPORTED, naming the
 * pair, if the platform refuses.  SG_ERR_INVALID_ARG for NULL, n == 0, n > 64, a NULL
 * or repeated context.  The contexts must outlive the group.  The arrays of pointers
 * these calls take are only read.
 * last_error[_pair]: message and (row, col) of the group's last failing call, as the
 * context's; with NULL, the reason the last create on this thread failed. */
typedef struct sg_group sg_group;
int32_t sg_group_create(sg_ctx** ctxs, uint32_t n, sg_group** out);
void sg_group_destroy(sg_group* g);
uint32_t sg_group_size(const sg_group* g);
const char* sg_group_last_error(const sg_group* g);
void sg_group_last_error_pair(const sg_group* g, uint32_t* row, uint32_t* col);

/* One host RoutingInfo from all members at once: nets[m] is the same graph created
 * on member m.  With per = ceil(ri->n / n), member m builds rows [min(m per, ri->n),
 * min((m + 1) per, ri->n)) and copies them into ri's pinned cells, each member on a
 * host thread of its own, in blocks of half its rows (whole 64-row batches); a
 * member whose range is empty does nothing.  ri ends exactly as after the single
 * fill of one context, and so do the errors: the self-loop check runs first (on member 0), and of
 * the members' search errors the one at the smallest (row, col) is reported.  After
 * a failure ri is not filled, and no copy still writes into it.
 * SG_ERR_INVALID_ARG when nets[m] was not created on member m or the graphs differ in
 * node count, edge count or directedness. */
int32_t sg_group_routing_info_fill(sg_group* g, sg_net** nets, const uint32_t* nodes, uint32_t flags,
                                   sg_routing_info* ri);

/* Step 2 of the fixed-split round ("sharded delivery with a fixed-split exchange"
 * above) for all members in one call.  Arrays of n device pointers, entry m on member
 * m's device.  Afterwards, for every owner r and source b:
 *   xall[r] = xrow[0] | xrow[1] | ... | xrow[n-1]            (n x (3 + n) u64)
 *   recv_padded[r][b*cap + k] = send_padded[b][r*cap + k]    for k < min(xrow[b][3 + r], cap)
 * Slots past that count in recv_padded are left as they were.  Each owner pulls its
 * blocks with one kernel on its own stream; no count leaves the device.  Ordering is
 * by events: every owner's pull waits for what every member had enqueued on its stream
 * before the call, and what the caller enqueues on any member's stream after the call
 * waits for every pull (so the next round may overwrite send_padded at once).
 * Stamped records move as plain ones.  Does not synchronise. */
int32_t sg_group_exchange_padded(sg_group* g, const sg_record** send_padded, sg_record** recv_padded, uint32_t cap,
                                 const uint64_t** xrow, uint64_t** xall);
/* The exact exchange (the contract of sg_comm_alltoallv_records): counts is a host
 * n x n array, counts[b*n + r] = records member b holds for member r, grouped by r in
 * send[b]; recv[r] receives them source after source.  Device copies behind the same
 * event ordering.  Does not synchronise. */
int32_t sg_group_alltoallv_records(sg_group* g, const sg_record** send, const uint32_t* counts, sg_record** recv);

/* ---- link loads and link trace across a group (additive to ABI 7) -----------
 * sg_link_load_packets and sg_link_trace_packets for a round that a group shards by
 * source row block: member m holds rows [row_begin[m], row_end[m]) of the tree (and,
 * for the trace, of the table), and packets[m] are the sends of its own sources.
 * Rounds, packets, the counting rule, address resolution, link numbering, the record
 * and the error kinds are those calls'; nothing is redefined here.  Every member
 * walks its own batch on its own stream, all members at once, and the results are
 * combined on the device of member `root`.  (sg_tree_paths[_packets] needs no group
 * form: its output is per packet and a member's packets are its own, so n calls, one
 * per member, are the answer.)
 *
 * Per member, arrays of n entries, entry m on member m's context and device (always
 * device memory; there is no host-array mode): nets[m], the same graph on every
 * member, checked as in sg_group_routing_info_fill; hosts[m]; pred[m] (and
 * latency_ns[m]), rows [row_begin[m], row_end[m]) row-major from row_begin[m];
 * packets[m], an sg_packets in the host array `packets` whose pointers are device
 * memory of member m; status[m], or NULL (`status` itself may be NULL: every packet of
 * every member counts).  row_begin and row_end are host arrays; the ranges need not be
 * row_range's, an empty one is legal, and so is n_packets == 0.  `nodes` (n_nodes
 * entries, host) is one permutation for all members.
 *
 * sg_group_link_load_packets: weight[m] as `weight` of sg_link_load_packets (NULL, or
 * a NULL `weight`: 1).  out_link_load (n_links u64) and out_node_load (n_nodes u64)
 * lie on root's device and are ADDED to; out_hops[m] (n_packets of m, u32) lies on
 * member m's device.  Any may be NULL (out_hops itself, or single entries), not all.
 * Each member sums into a zeroed accumulator of its own; after every member's flags
 * have been read, one kernel on root's stream adds the n accumulators into the
 * caller's arrays, and the call returns when it has finished.  The result equals
 * sg_link_load_packets on one context holding all rows and the members' batches
 * concatenated in member order.  Because the add is deferred, ANY error leaves
 * out_link_load and out_node_load untouched (stronger than the single call);
 * out_hops is undefined after a device-found error.
 *
 * sg_group_link_trace_packets: `watch` is a HOST mask of n_links u8, or NULL; the
 * library uploads it to every member.  packet_base: host, n u32, or NULL = the
 * exclusive prefix sums of the members' n_packets (the packet's index in the
 * concatenated batch).  Outputs on root's device: out_link_off (n_links + 1 u64,
 * required), out_packet u32, out_member u8, out_hop u32, out_enter_ns u64,
 * out_exit_ns u64, each of capacity `cap` records; any record array may be NULL, not
 * all five.  `total` is a host pointer.  Link L owns records
 * [out_link_off[L], out_link_off[L + 1]) in ascending (enter_ns, member, member-local
 * packet index) order; out_member = m, out_packet = packet_base[m] + p.  The key is
 * unique whatever the bases are.  With the default bases the output equals
 * sg_link_trace_packets on one context with all rows and the concatenated batch, and
 * out_member tells where each record came from; with n = 1 it is that call's output,
 * bit for bit.  total > cap: SG_ERR_CAPACITY, out_link_off and *total complete, no
 * record array written; the sizing call works as there (a real record array, cap 0).
 * With no packet in any member out_link_off is all zero and *total = 0.  Every member
 * counts and scans; the host reads flags and totals; root sums the members' offsets
 * (no second scan); every member fills and sorts its own segments; one kernel on root
 * places each record by rank among the members' sorted segments of its link (binary
 * searches on enter_ns alone); the call ends with one wait on root's stream.
 *
 * Errors.  SG_ERR_INVALID_ARG with every output untouched: NULL arguments; a net or
 * hosts not of its member's context; graphs that differ; root >= n; no output at all;
 * `nodes` not a permutation; a bad row range; NULL pred (or latency_ns) rows of a
 * non-empty range; NULL packet arrays of a non-empty batch.  Found on the device: the
 * single call's kinds with its precedence inside a member (packet kinds, then the
 * time overflow, then pred kinds); across members the LOWEST-NUMBERED failing member
 * is reported: sg_group_last_error names it ("member 2: packet 17 ..."),
 * sg_group_last_error_pair gives its pair (a packet index there is member-local) and
 * sg_group_last_error_member the member.  out_link_off, the record arrays and the
 * load arrays are untouched after a device-found error.
 * sg_group_last_error_member: the member whose device-found error the group's last
 * call reported; UINT32_MAX when that call succeeded, failed for another reason, or g
 * is NULL.
 * Timers, on root's context: "group_link_reduce" (work = accumulator words read),
 * "group_trace_offsets" and "group_trace_merge" (work = records); the members' own
 * timers are the single calls' ("link_packets", "link_trace_count",
 * "link_trace_fill", "link_trace_sort").
 *
 * sg_group_link_series_packets: sg_link_series_packets for the same sharding, with
 * sg_group_link_load_packets' argument shape.  latency_ns[m] as in the group trace;
 * weight[m] as in the group link loads; link_slot is a HOST map of n_links u32, or
 * NULL (the identity), uploaded to every member as `watch` is and validated on the
 * host; n_slots, at, t0_ns, bin_ns and n_bins as in the single call.  out_series and
 * out_outside (or NULL) lie on root's device and are ADDED to.  Each member sums into
 * a zeroed accumulator of its own; after every member's flags have been read, one
 * kernel on root's stream adds the accumulators into the caller's arrays.  ANY error
 * leaves the caller's arrays untouched; the lowest-numbered failing member is
 * reported.  The result equals the single call on all rows with the batches
 * concatenated; with n = 1 it is that call's, bit for bit.  Timers: "link_series" on
 * the members, "group_link_reduce" on root. */
uint32_t sg_group_last_error_member(const sg_group* g);
int32_t sg_group_link_series_packets(sg_group* g, sg_net** nets, sg_hosts** hosts,
                                     const uint32_t* nodes, uint32_t n_nodes,
                                     const uint32_t* row_begin, const uint32_t* row_end,
                                     const uint32_t** pred, const uint64_t** latency_ns,
                                     const sg_packets* packets, const uint8_t** status,
                                     const uint32_t** weight,
                                     const uint32_t* link_slot, uint32_t n_slots, uint32_t at,
                                     uint64_t t0_ns, uint64_t bin_ns, uint32_t n_bins,
                                     uint32_t root,
                                     uint64_t* out_series, uint64_t* out_outside);
int32_t sg_group_link_load_packets(sg_group* g, sg_net** nets, sg_hosts** hosts,
                                   const uint32_t* nodes, uint32_t n_nodes,
                                   const uint32_t* row_begin, const uint32_t* row_end,
                                   const uint32_t** pred, const sg_packets* packets,
                                   const uint8_t** status, const uint32_t** weight,
                                   uint32_t root,
                                   uint64_t* out_link_load, uint64_t* out_node_load,
                                   uint32_t** out_hops);
int32_t sg_group_link_trace_packets(sg_group* g, sg_net** nets, sg_hosts** hosts,
                                    const uint32_t* nodes, uint32_t n_nodes,
                                    const uint32_t* row_begin, const uint32_t* row_end,
                                    const uint32_t** pred, const uint64_t** latency_ns,
                                    const sg_packets* packets, const uint8_t** status,
                                    const uint8_t* watch, const uint32_t* packet_base,
                                    uint32_t root,
                                    uint64_t* out_link_off,
                                    uint32_t* out_packet, uint8_t* out_member, uint32_t* out_hop,
                                    uint64_t* out_enter_ns, uint64_t* out_exit_ns,
                                    uint64_t cap, uint64_t* total);

#ifdef __cplusplus
}
#endif
#endif /* SHADOW_GPU_H */
