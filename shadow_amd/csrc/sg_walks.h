// sg_walks.h -- the per-packet tree walks of a round (link loads from packets, sg_link.hip; link
// trace, sg_trace.hip) as ENQUEUE and FINISH halves.  The single-context entry points run the
// halves back to back; a device group (sg_group_trace.hip) enqueues every member's first half,
// then finishes them one by one, so that all members are in flight at once.
//
// Every pointer of a call is device memory of the call's context, except `nodes` (host).  The
// halves run with the context's device current.  A check throws sg::Error for an argument error
// and touches nothing; an enqueue queues work on the context stream and does not wait; a finish
// waits for the stream, reads the flag words and throws the call's device-found error, if any.
#pragma once

#include "sg_hosts.h"
#include "sg_internal.h"
#include "sg_links.h"

namespace sg {

// ---- link loads from a round's packets (sg_link.hip)
struct LinkPacketArgs {
  LinkArgs l;  // (counts, count_cols, scratch and vec unused; bad = LP_WORDS words)
  HostMap map;
  const uint32_t* route;  // host -> route index
  uint32_t n_hosts, n_packets;
  const uint32_t* src_host;
  const uint32_t* dst_ipv4;
  const uint8_t* status;   // or null: every packet counts
  const uint32_t* weight;  // or null: 1
  uint32_t* hops;          // or null
};

struct LinkPacketsCall {
  sg_ctx* ctx;
  sg_net* net;
  sg_hosts* hosts;
  const uint32_t* nodes;
  uint32_t n_nodes, row_begin, row_end;
  const uint32_t* pred;
  const sg_packets* packets;
  const uint8_t* status;
  const uint32_t* weight;
  uint64_t* link_load;  // the three outputs, any of them null (the caller checks "not all")
  uint64_t* node_load;
  uint32_t* hops;
};

// The argument errors of sg_link_load_packets but "no output at all"; `nodes` is checked when
// check_nodes is set (a group checks its one list once).
void link_packets_check(const LinkPacketsCall& c, bool check_nodes);
// The walk of c.packets (n_packets > 0) on the context stream.
void link_packets_enqueue(const LinkPacketsCall& c);
void link_packets_finish(const LinkPacketsCall& c);

// ---- link trace (sg_trace.hip)
struct TraceArgs {
  LinkArgs l;  // (counts, count_cols, link_load, node_load, scratch and vec unused; bad = TR_WORDS words)
  HostMap map;
  const uint32_t* route;  // host -> route index
  uint32_t n_hosts;
  const uint32_t* src_host;
  const uint32_t* dst_ipv4;
  const unsigned long long* send_time;
  const uint8_t* status;  // or null: every packet counts
  uint32_t n_items;       // packets
  uint32_t* hops;         // per packet, from the count walk
  const unsigned long long* lat;  // rows [row_begin, row_begin + rows) of the table
  const uint8_t* watch;           // per link, or null: every link
  uint32_t n_links;
  uint32_t* cnt;  // records per link
  uint32_t* cur;  // the fill's cursor per link
  unsigned long long* sums;  // the scan's block sums, then their exclusive prefix
  unsigned long long* off;   // out_link_off
  unsigned long long* total;  // the mapped word
  // staging: (enter lo, enter hi, packet, hop) and the exit time (or null)
  uint4* key;
  unsigned long long* exit;
};

// The four record arrays, any of them null.
struct TraceOut {
  uint32_t* packet;
  uint32_t* hop;
  unsigned long long* enter;
  unsigned long long* exit;
};

struct TraceCall {
  sg_ctx* ctx;
  sg_net* net;
  sg_hosts* hosts;
  const uint32_t* nodes;
  uint32_t n_nodes, row_begin, row_end;
  const uint32_t* pred;
  const uint64_t* lat;
  const sg_packets* packets;
  const uint8_t* status;
  const uint8_t* watch;
  uint64_t* off;  // n_links + 1 entries
};

// A trace between its halves.
struct TraceJob {
  TraceArgs a;
  uint32_t* n_work = nullptr;
  unsigned grid = 0;
  uint64_t total = 0;  // set by trace_finish_count
};

// The argument errors of sg_link_trace_packets that concern the inputs (not the outputs).
void trace_check(const TraceCall& c, bool check_nodes);
// Count and scan of c.packets (n_packets > 0): c.off and the total, on the context stream.
void trace_enqueue_count(const TraceCall& c, TraceJob& j);
// Waits; throws the device-found error; else j.total = the records.
void trace_finish_count(const TraceCall& c, TraceJob& j);
// Fill and the three sort tiers into `out` (j.total > 0 records each; null arrays are skipped).
void trace_enqueue_sort(const TraceCall& c, TraceJob& j, const TraceOut& out);

}  // namespace sg
