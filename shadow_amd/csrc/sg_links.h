// sg_links.h -- the tree rows of a call (LinkArgs), the link lookup and the node index, shared by
// the translation units that turn a (pred, node) pair into a link number on the device: the dense
// fold and the packet walk of sg_link.hip, sg_paths.hip and sg_trace.hip (the latter three through
// the walks of sg_walks.h).  check_rows_call also serves sg_tree.hip, which writes the rows.
#pragma once

#include <cstring>

#include "sg_internal.h"

namespace sg {

constexpr uint32_t LINK_NONE = 0xFFFFFFFFu;

// What link_find and every walk up a pred row need.
struct LinkArgs {
  // the net's links by head (ensure_links)
  const uint32_t* lk_off;
  const uint32_t* lk_tail;
  // nodes[j] = the node of column j; pos = its inverse
  const uint32_t* nodes;
  const uint32_t* pos;
  uint32_t n, row_begin, rows;
  // rows [row_begin, row_begin + rows), row-major from row_begin
  const uint32_t* pred;
  unsigned long long* bad;  // the call's flag words
};

// The link (tail -> head): its index, or LINK_NONE.
__device__ __forceinline__ uint32_t link_find(const LinkArgs& a, uint32_t tail, uint32_t head) {
  uint32_t lo = a.lk_off[head], hi = a.lk_off[head + 1];
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint32_t t = a.lk_tail[mid];
    if (t == tail) return mid;
    if (t < tail)
      lo = mid + 1;
    else
      hi = mid;
  }
  return LINK_NONE;
}

// `nodes`, then its inverse, on the device (queued on the context stream).
static inline uint32_t* link_node_index(sg_ctx* ctx, const uint32_t* h_nodes, uint32_t n) {
  uint32_t* d_idx = ctx->l_idx.get<uint32_t>(2 * (size_t)n);
  char* hu = stage_acquire(ctx, 1, 2 * (size_t)n * 4);
  uint32_t* hn = (uint32_t*)hu;
  memcpy(hn, h_nodes, (size_t)n * 4);
  for (uint32_t j = 0; j < n; j++) hn[n + h_nodes[j]] = j;
  SG_HIP(hipMemcpyAsync(d_idx, hu, 2 * (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  stage_release(ctx, 1);
  return d_idx;
}

// d_idx: link_node_index's.
static inline LinkArgs link_args(const sg_net* net, const uint32_t* d_idx, uint32_t n, uint32_t row_begin,
                                 uint32_t rows, const uint32_t* pred, unsigned long long* bad) {
  return LinkArgs{net->lk_off, net->lk_tail, d_idx, d_idx + n, n, row_begin, rows, pred, bad};
}

// The argument checks every call over tree rows starts with (`what` spans every graph node).
static inline void check_rows_call(const sg_ctx* ctx, const sg_net* net, const uint32_t* nodes, uint32_t n_nodes,
                                   uint32_t row_begin, uint32_t row_end, const char* what = "a pred row") {
  if (!net || net->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "network belongs to another context");
  if (n_nodes != net->n_nodes)
    throw Error(SG_ERR_INVALID_ARG,
                std::string(what) + " spans every graph node: n_nodes must be the network's node count");
  if (n_nodes && !nodes) throw Error(SG_ERR_INVALID_ARG, "null node list");
  if (row_begin > row_end || row_end > n_nodes) throw Error(SG_ERR_INVALID_ARG, "bad row range");
}

}  // namespace sg
