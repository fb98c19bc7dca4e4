// sg_walks.h -- the walk up a row's predecessor tree, from a destination column to the row's
// source, and what its users share: sg_link_load_packets (sg_link.hip), sg_tree_paths and
// sg_tree_paths_packets (sg_paths.hip), sg_link_trace_packets (sg_trace.hip),
// sg_link_series_packets (sg_series.hip) and the group forms on top of them (sg_group_trace.hip).
//   - the item rule: a packet or a pair to its (row, column), or the kind of its error;
//   - the flag words a call's kernels report through, and the host's decode of them;
//   - the count walk;
//   - the per-packet walks of a round (link loads, link trace, link series) as ENQUEUE and FINISH halves.  The
//     single-context entry points run the halves back to back; a device group enqueues every
//     member's first half, then finishes them one by one, so that all members are in flight at once.
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

// ---- flag words (LinkArgs::bad): the smallest failing (item << 3) | ITEM_*; the first
// (row << 32) | col of each pred kind; link loads' fifth word, the packets counted
enum {
  WALK_BAD_ITEM = 0,
  WALK_BAD_RANGE = 1,
  WALK_BAD_LINK = 2,
  WALK_BAD_CYCLE = 3,
  WALK_WORDS = 4,
  WALK_COUNTED = 4,
  WALK_WORDS_COUNTED = 5
};
enum { ITEM_SRC = 0, ITEM_ROW = 1, ITEM_DST = 2, ITEM_COL = 3, ITEM_TIME = 4 };

// ---- the item rule
struct PacketArgs {
  HostMap map;
  const uint32_t* route;  // host -> route index
  uint32_t n_hosts;
  const uint32_t* src_host;
  const uint32_t* dst_ipv4;
  const uint8_t* status;  // or null: every packet counts
};

__device__ __forceinline__ void flag_item(const LinkArgs& l, uint32_t p, uint32_t kind) {
  atomicMin(&l.bad[WALK_BAD_ITEM], ((unsigned long long)p << 3) | kind);
}

// Packet p's (row, column); returns whether it is walked.  kind: ITEM_* when the packet is in
// error, else LINK_NONE.  A packet that does not count is still in error for a bad source host;
// its destination is not resolved (sg_hosts.h).
__device__ __forceinline__ bool packet_item(const PacketArgs& a, const LinkArgs& l, uint32_t p, uint32_t& i,
                                            uint32_t& j, uint32_t& kind) {
  kind = LINK_NONE;
  i = j = 0;
  const uint32_t h = a.src_host[p];
  const bool counts = !a.status || a.status[p] == SG_PKT_DELIVERED;
  if (h >= a.n_hosts) {
    kind = ITEM_SRC;
    return false;
  }
  i = a.route[h];
  if (i < l.row_begin || i - l.row_begin >= l.rows) {
    kind = ITEM_ROW;
    return false;
  }
  if (!counts) return false;
  const uint2 r = a.map.resolve(a.dst_ipv4[p]);
  j = r.y;
  if (r.x == NONE) {
    kind = ITEM_DST;
    return false;
  }
  if (j >= l.n) {
    kind = ITEM_COL;
    return false;
  }
  return true;
}

// Pair p's, the same way.
__device__ __forceinline__ bool pair_item(const uint32_t* pair_row, const uint32_t* pair_col, const LinkArgs& l,
                                          uint32_t p, uint32_t& i, uint32_t& j, uint32_t& kind) {
  kind = LINK_NONE;
  i = pair_row[p];
  j = pair_col[p];
  if (i < l.row_begin || i - l.row_begin >= l.rows)
    kind = ITEM_ROW;
  else if (j >= l.n)
    kind = ITEM_COL;
  return kind == LINK_NONE;
}

// ---- the walk.  Row i (source s = nodes[i]) from column j (d = nodes[j]); v is the node the walk
// stands on, cv its column, u = pred_i[v].  A value >= n is caught before it forms an index, a
// walk ends after n steps (a cycle); errors go to the flag words as (i << 32) | column.

// The count walk: the hops of the path, 0 when the row is in error; d == s is one hop, the
// self-loop (get_edge_weight's rule).  LINKS: every hop's link is searched and hop(link, cv)
// called with it; one that is no link is flagged and not passed.  Else hop is not called.
template <bool LINKS, class F>
__device__ __forceinline__ uint32_t count_walk(const LinkArgs& l, uint32_t i, uint32_t j, F&& hop) {
  const uint32_t n = l.n, s = l.nodes[i], d = l.nodes[j];
  const unsigned long long cell = (unsigned long long)i << 32;
  auto cross = [&](uint32_t u, uint32_t v, uint32_t cv) {
    if constexpr (LINKS) {
      const uint32_t link = link_find(l, u, v);
      if (link == LINK_NONE)
        atomicMin(&l.bad[WALK_BAD_LINK], cell | cv);
      else
        hop(link, cv);
    }
  };
  if (d == s) {
    cross(s, s, j);
    return 1u;
  }
  const uint32_t* __restrict__ row = l.pred + (size_t)(i - l.row_begin) * n;
  uint32_t v = d, cv = j, pv = row[j], steps = 0;
  for (;;) {
    if (steps >= n) {  // n steps and not at s: a cycle
      atomicMin(&l.bad[WALK_BAD_CYCLE], cell | j);
      return 0u;
    }
    if (pv >= n) {
      atomicMin(&l.bad[WALK_BAD_RANGE], cell | cv);
      return 0u;
    }
    steps++;
    cross(pv, v, cv);
    if (pv == s) return steps;
    v = pv;
    cv = l.pos[pv];
    pv = row[cv];
  }
}

// (The fills climb the same way, the next hop's gather issued ahead of the link search, but each
// keeps its own loop: a shared climb with a functor per hop cost k_trace_fill 2 to 4 % at C3, its
// latency cell no longer loaded beside the gather.)

// ---- host: the set-up and the decode of the flag words (sg_link.hip)
PacketArgs packet_args(const sg_hosts* hosts, const sg_packets* packets, const uint8_t* status);
// word: a WALK_BAD_ITEM word that is set.  ITEM_TIME is SG_ERR_TIME_OVERFLOW.
[[noreturn]] void throw_item_error(bool packets, unsigned long long word);
// word: the WALK_BAD_RANGE / _LINK / _CYCLE word (`kind`) that is set.  The entry point chooses
// which of its words wins.
[[noreturn]] void throw_pred_error(const sg_net* net, const uint32_t* nodes, int kind, unsigned long long word);

// ---- link loads from a round's packets (sg_link.hip)
struct LinkPacketArgs {
  LinkArgs l;  // (bad: WALK_WORDS_COUNTED words)
  PacketArgs pk;
  uint32_t n_packets;
  const uint32_t* weight;         // or null: 1
  unsigned long long* link_load;  // the three outputs, or null
  unsigned long long* node_load;
  uint32_t* hops;
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
  LinkArgs l;  // (bad: WALK_WORDS words)
  PacketArgs pk;
  const unsigned long long* send_time;
  uint32_t n_items;  // packets
  uint32_t* hops;    // per packet, from the count walk
  const unsigned long long* lat;  // rows [row_begin, row_begin + rows) of the table
  const uint8_t* watch;           // per link, or null: every link
  uint32_t n_links;
  uint32_t* cnt;  // records per link
  uint32_t* cur;  // the fill's cursor per link
  unsigned long long* off;  // out_link_off
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

// ---- link time series (sg_series.hip)
// Flag words: the walks' four, the packets counted, and the smallest link whose slot value is
// neither below n_slots nor UINT32_MAX.
enum { SERIES_BAD_SLOT = 5, SERIES_WORDS = 6 };

struct SeriesCall {
  sg_ctx* ctx;
  sg_net* net;
  sg_hosts* hosts;
  const uint32_t* nodes;
  uint32_t n_nodes, row_begin, row_end;
  const uint32_t* pred;
  const uint64_t* lat;
  const sg_packets* packets;
  const uint8_t* status;
  const uint32_t* weight;
  const uint32_t* slot;  // n_links entries, or null: the identity
  uint32_t n_slots, at;
  uint64_t t0, bin;
  uint32_t n_bins;
  uint64_t* series;   // n_slots x n_bins, added to
  uint64_t* outside;  // 2 n_slots, added to, or null
};

// The argument errors of sg_link_series_packets but those of the slot values; builds the net's
// links (a null slot map needs their count).
void series_check(const SeriesCall& c, bool check_nodes);
// The walk of c.packets (n_packets > 0) on the context stream.
void series_enqueue(const SeriesCall& c);
void series_finish(const SeriesCall& c);

}  // namespace sg
