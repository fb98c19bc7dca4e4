// sg_links.h -- the link lookup and the node index, shared by the translation units that turn a
// (pred, node) pair into a link number on the device (sg_link.hip, sg_paths.hip).
#pragma once

#include <cstring>

#include "sg_internal.h"

namespace sg {

constexpr uint32_t LINK_NONE = 0xFFFFFFFFu;

struct LinkArgs {
  // the net's links by head (ensure_links)
  const uint32_t* lk_off;
  const uint32_t* lk_tail;
  // nodes[j] = the node of column j; pos = its inverse
  const uint32_t* nodes;
  const uint32_t* pos;
  uint32_t n, row_begin, rows, count_cols;
  // rows [row_begin, row_begin + rows), row-major from row_begin
  const uint32_t* pred;
  const unsigned long long* counts;
  unsigned long long* link_load;  // or null
  unsigned long long* node_load;  // or null
  unsigned long long* bad;        // LINK_BAD_KINDS words
  unsigned char* scratch;         // global path: LINK_SCRATCH_BYTES * n per workgroup
  int vec;                        // 16-byte loads are aligned in every row
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

}  // namespace sg
