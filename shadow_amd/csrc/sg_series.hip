// sg_series.hip -- link time series: bytes per link per time bin, summed on the device.
//
// The link trace (sg_trace.hip) keeps one record per crossing and sorts them; what is plotted from
// a simulation is a histogram of those records, which needs neither the records nor their order.
// This file walks a round's packets once and adds each packet's weight into one cell per link
// crossed, in a matrix that stays on the device across rounds.  Crossings, their enter / exit
// times, pairs and validation are the trace's; the weight is sg_link_load_packets'.
//
// For a crossing of link L at time t (the enter or the exit time, by `at`): s = slot[L] (the
// identity without a map; UINT32_MAX: not watched, walked and validated all the same);
//   t <  t0:                 outside[2 s]     += w
//   q = (t - t0) / bin_ns:   series[s][q]     += w   when q < n_bins
//                            outside[2 s + 1] += w   otherwise
// q is the exact u64 quotient and is compared as such: t0 + n_bins * bin_ns may pass 2^64.
//
// The quotient (SeriesDiv): a shift when bin_ns is a power of two; else the multiply-high form of
// Granlund and Montgomery (1994, fig. 4.1) at N = 64: with l = ceil(log2 d) and
// m = floor(2^64 (2^l - d) / d) + 1,  q = (t1 + ((n - t1) >> 1)) >> (l - 1),  t1 = mulhi(m, n),
// which is floor(n / d) for EVERY n below 2^64 (n - t1 never borrows: t1 <= n).  One 64 x 64 high
// multiply, two shifts, an add and a subtract per crossing instead of a division loop.
//
// One kernel, a lane per packet, grid-stride, in two forms:
//   LDS     n_slots (n_bins + 2) cells fit the budget (SG_LINK_SERIES_LDS): the workgroup zeroes a
//           matrix of its own in LDS, adds with LDS u64 atomics (ds_add_u64: one operation, the
//           carry inside it), and at its end adds its non-zero cells to the caller's matrix.  The
//           watched-links case: what would serialise on a few L2 lines stays on the CU.  The grid
//           is bounded (the workgroups resident at once, by the occupancy query: 7 per CU at 16 x
//           64 cells), so the flush is grid x cells LDS reads and at most as many global adds as
//           there were crossings, small beside packets x hops dependent loads.
//   global  u64 adds straight into the matrix, held back and issued SR_HOPS at a time as
//           link_packet_walk's are (sg_link.hip, LP_HOPS: a no-return atomic stays counted in
//           vmcnt and every wait the compiler emits is vmcnt(0)).
// The climb is k_trace_fill's -- the next hop's gather issued ahead of the link search, enter and
// exit in registers -- with the count walk's validation in the same pass: a value >= n_nodes is
// caught before it forms an index, a walk ends after n_nodes steps, a slot value >= n_slots never
// forms an index.  Errors go through u64 mins into the flag words, read at the one synchronisation.
// The slot map is validated whole ahead of the walk, by the same kernel: the smallest link with a
// bad value is what the call reports, crossed or not.
#include <algorithm>
#include <string>
#include <vector>

#include "sg_device.h"
#include "sg_hosts.h"
#include "sg_internal.h"
#include "sg_knobs.h"
#include "sg_links.h"
#include "sg_walks.h"

namespace sg {
namespace {

constexpr uint32_t SR_THREADS = 256;
constexpr int SR_HOPS = 4;  // global form: hops walked between two flushes of the adds
constexpr int SR_LDS_DEFAULT = 4096;  // cells: 32 KiB, so that a CU holds five workgroups
constexpr int SR_LDS_MAX = 8064;      // what fits beside the static words below 64 KiB

struct SeriesDiv {
  unsigned long long mul;
  uint32_t sh2;  // l - 1
  int shift;     // >= 0: bin_ns = 1 << shift, the other two unused
};

SeriesDiv series_div(uint64_t d) {
  SeriesDiv v{0ull, 0u, -1};
  if ((d & (d - 1)) == 0) {
    v.shift = __builtin_ctzll(d);
    return v;
  }
  const uint32_t l = 64u - (uint32_t)__builtin_clzll(d - 1);  // 2 .. 64
  // floor(2^64 r / d) for r = 2^l - d < d, by long division: a bit of the quotient per step
  uint64_t r = l == 64 ? (uint64_t)0 - d : ((uint64_t)1 << l) - d, q = 0;
  for (int b = 0; b < 64; b++) {
    const bool carry = (r >> 63) != 0;
    r <<= 1;
    q <<= 1;
    if (carry || r >= d) {
      r -= d;
      q |= 1;
    }
  }
  v.mul = q + 1;
  v.sh2 = l - 1;
  return v;
}

__device__ __forceinline__ unsigned long long series_quot(const SeriesDiv& v, unsigned long long n) {
  if (v.shift >= 0) return n >> v.shift;
  const unsigned long long t1 = __umul64hi(v.mul, n);
  return (t1 + ((n - t1) >> 1)) >> v.sh2;
}

struct SeriesArgs {
  LinkArgs l;  // (bad: SERIES_WORDS words)
  PacketArgs pk;
  const unsigned long long* send_time;
  uint32_t n_items;
  const unsigned long long* lat;
  const uint32_t* weight;  // or null: 1
  const uint32_t* slot;    // or null: the identity
  uint32_t n_links, n_slots, at, n_bins;
  unsigned long long t0;
  SeriesDiv div;
  unsigned long long* series;
  unsigned long long* outside;  // or null
};

// The crossing's (slot, column): columns [0, n_bins) the bins, n_bins "before", n_bins + 1
// "after".  False: the link is not watched (or its slot value is bad: reported by the check).
__device__ __forceinline__ bool series_cell(const SeriesArgs& a, uint32_t link, unsigned long long t, uint32_t& s,
                                            uint32_t& col) {
  s = a.slot ? a.slot[link] : link;
  if (s >= a.n_slots) return false;
  if (t < a.t0) {
    col = a.n_bins;
  } else {
    const unsigned long long q = series_quot(a.div, t - a.t0);
    col = q < (unsigned long long)a.n_bins ? (uint32_t)q : a.n_bins + 1;
  }
  return true;
}

// The caller's cell of (slot, column), or null where `outside` is not taken.
__device__ __forceinline__ unsigned long long* series_target(const SeriesArgs& a, uint32_t s, uint32_t col) {
  if (col < a.n_bins) return a.series + (size_t)s * a.n_bins + col;
  return a.outside ? a.outside + 2 * (size_t)s + (col - a.n_bins) : nullptr;
}

template <bool LDS>
__global__ void __launch_bounds__(SR_THREADS) k_link_series(const SeriesArgs a) {
  extern __shared__ unsigned long long s_cell[];
  __shared__ uint32_t s_counted;
  const LinkArgs& l = a.l;
  const uint32_t n = l.n, width = a.n_bins + 2;
  const uint32_t cells = LDS ? a.n_slots * width : 0u;  // (within the budget: no overflow)
  if (LDS)
    for (uint32_t c = threadIdx.x; c < cells; c += SR_THREADS) s_cell[c] = 0ull;
  if (threadIdx.x == 0) s_counted = 0u;
  // the slot map, whole
  if (a.slot) {
    uint32_t bad = LINK_NONE;
    for (uint32_t k = blockIdx.x * SR_THREADS + threadIdx.x; k < a.n_links; k += gridDim.x * SR_THREADS) {
      const uint32_t s = a.slot[k];
      if (s >= a.n_slots && s != LINK_NONE) bad = min(bad, k);
    }
    if (bad != LINK_NONE) atomicMin(&l.bad[SERIES_BAD_SLOT], (unsigned long long)bad);
  }
  __syncthreads();
  uint32_t counted = 0;
  const unsigned long long stride = (unsigned long long)gridDim.x * SR_THREADS;
  for (unsigned long long pq = (unsigned long long)blockIdx.x * SR_THREADS + threadIdx.x; pq < a.n_items; pq += stride) {
    const uint32_t p = (uint32_t)pq;
    uint32_t i, j, kind;
    const bool walk = packet_item(a.pk, l, p, i, j, kind);
    if (kind != LINK_NONE) flag_item(l, p, kind);
    if (!walk) continue;
    counted++;
    const unsigned long long w = a.weight ? (unsigned long long)a.weight[p] : 1ull;
    const unsigned long long send = a.send_time[p];
    const size_t r = (size_t)(i - l.row_begin) * n;
    // the destination's time bounds every hop's: arc latency is at least 1 ns, cum rises along the path
    unsigned long long exit = send + a.lat[r + j];
    if (exit < send) {
      flag_item(l, p, ITEM_TIME);
      continue;
    }
    const uint32_t s = l.nodes[i], d = l.nodes[j];
    const unsigned long long cell = (unsigned long long)i << 32;
    auto add = [&](uint32_t sl, uint32_t col) {
      if (LDS) {
        atomicAdd(&s_cell[sl * width + col], w);
      } else {
        unsigned long long* tgt = series_target(a, sl, col);
        if (tgt) atomicAdd(tgt, w);
      }
    };
    if (d == s) {  // the self-loop (get_edge_weight's rule), one crossing: enter = send
      const uint32_t k = link_find(l, s, s);
      uint32_t sl, col;
      if (k == LINK_NONE)
        atomicMin(&l.bad[WALK_BAD_LINK], cell | j);
      else if (series_cell(a, k, a.at ? exit : send, sl, col))
        add(sl, col);
      continue;
    }
    const uint32_t* __restrict__ row = l.pred + r;
    // v climbs from d; cv its column; pv = pred_i[v], gathered one hop ahead, and the cell of
    // the hop's tail with it
    uint32_t v = d, cv = j, pv = row[j], steps = 0;
    bool go = true;
    while (go) {
      uint32_t ss[SR_HOPS], cs[SR_HOPS];
#pragma unroll
      for (int q = 0; q < SR_HOPS; q++) {
        ss[q] = LINK_NONE;
        cs[q] = 0u;
        if (!go) continue;
        if (steps >= n) {  // n steps and not at s: a cycle
          atomicMin(&l.bad[WALK_BAD_CYCLE], cell | j);
          go = false;
          continue;
        }
        const uint32_t u = pv;
        if (u >= n) {
          atomicMin(&l.bad[WALK_BAD_RANGE], cell | cv);
          go = false;
          continue;
        }
        uint32_t cu = 0u;
        unsigned long long enter = send;
        if (u != s) {
          cu = l.pos[u];
          pv = row[cu];
          enter = send + a.lat[r + cu];
        }
        const uint32_t k = link_find(l, u, v);
        if (k == LINK_NONE) {
          atomicMin(&l.bad[WALK_BAD_LINK], cell | cv);
          go = false;
          continue;
        }
        uint32_t sl, col;
        if (series_cell(a, k, a.at ? exit : enter, sl, col)) {
          if (LDS) {
            add(sl, col);
          } else {
            ss[q] = sl;
            cs[q] = col;
          }
        }
        steps++;
        v = u;
        cv = cu;
        exit = enter;
        go = u != s;
      }
      if (!LDS) {
#pragma unroll
        for (int q = 0; q < SR_HOPS; q++)
          if (ss[q] != LINK_NONE) add(ss[q], cs[q]);
      }
    }
  }
  if (counted) atomicAdd(&s_counted, counted);
  __syncthreads();
  if (threadIdx.x == 0 && s_counted) atomicAdd(&l.bad[WALK_COUNTED], (unsigned long long)s_counted);
  if (LDS)
    for (uint32_t c = threadIdx.x; c < cells; c += SR_THREADS) {
      const unsigned long long x = s_cell[c];
      if (x == 0ull) continue;
      const uint32_t sl = c / width;
      unsigned long long* tgt = series_target(a, sl, c - sl * width);
      if (tgt) atomicAdd(tgt, x);
    }
}

}  // namespace

// ---- host: the halves of sg_walks.h
void series_check(const SeriesCall& c, bool check_nodes) {
  trace_check(TraceCall{c.ctx, c.net, c.hosts, c.nodes, c.n_nodes, c.row_begin, c.row_end, c.pred, c.lat, c.packets,
                        c.status, nullptr, nullptr},
              check_nodes);
  if (c.bin == 0 || c.n_bins == 0 || c.n_slots == 0) throw Error(SG_ERR_INVALID_ARG, "bin_ns, n_bins or n_slots is zero");
  if (c.at > SG_SERIES_AT_EXIT) throw Error(SG_ERR_INVALID_ARG, "at is neither SG_SERIES_AT_ENTER nor SG_SERIES_AT_EXIT");
  if (!c.series) throw Error(SG_ERR_INVALID_ARG, "null out_series");
  ensure_links(c.ctx, c.net);
  if (!c.slot && c.n_slots != c.net->n_links)
    throw Error(SG_ERR_INVALID_ARG, "link_slot is null: n_slots must be the link count, " + std::to_string(c.net->n_links));
}

void series_enqueue(const SeriesCall& c) {
  sg_ctx* ctx = c.ctx;
  sg_net* net = c.net;
  hipStream_t st = ctx->stream;
  const uint32_t n = c.n_nodes, ni = c.packets->n_packets;
  uint32_t* d_idx = link_node_index(ctx, c.nodes, n);
  unsigned long long* bad = ctx->l_flag.get<unsigned long long>(SERIES_WORDS);
  SG_HIP(hipMemsetAsync(bad, 0xff, SERIES_WORDS * 8, st));
  SG_HIP(hipMemsetAsync(bad + WALK_COUNTED, 0, 8, st));
  SeriesArgs a;
  a.l = link_args(net, d_idx, n, c.row_begin, c.row_end - c.row_begin, c.pred, bad);
  a.pk = packet_args(c.hosts, c.packets, c.status);
  a.send_time = (const unsigned long long*)c.packets->send_time_ns;
  a.n_items = ni;
  a.lat = (const unsigned long long*)c.lat;
  a.weight = c.weight;
  a.slot = c.slot;
  a.n_links = net->n_links;
  a.n_slots = c.n_slots;
  a.at = c.at;
  a.n_bins = c.n_bins;
  a.t0 = c.t0;
  a.div = series_div(c.bin);
  a.series = (unsigned long long*)c.series;
  a.outside = (unsigned long long*)c.outside;
  const uint64_t cells = (uint64_t)c.n_slots * ((uint64_t)c.n_bins + 2);
  const bool lds = cells <= (uint64_t)knob_int("SG_LINK_SERIES_LDS", SR_LDS_DEFAULT, 0, SR_LDS_MAX);
  // (work = the packets walked, added by the finish once the count is read)
  TimedLaunch tl(ctx, "link_series", 0.0);
  if (lds) {
    // persistent, every workgroup the same share: as many as are resident at once, and no more --
    // one more per CU would run alone after the others, a second round for an eighth of the work
    int per_cu = 0;
    SG_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_link_series<true>, (int)SR_THREADS, (size_t)cells * 8));
    const dim3 grid(grid_for(ni, SR_THREADS, (unsigned)std::max(per_cu, 1) * (unsigned)ctx->n_cu));
    hipLaunchKernelGGL(k_link_series<true>, grid, dim3(SR_THREADS), (size_t)cells * 8, st, a);
  } else {
    const dim3 grid(grid_for(ni, SR_THREADS, 16u * (unsigned)ctx->n_cu));
    hipLaunchKernelGGL(k_link_series<false>, grid, dim3(SR_THREADS), 0, st, a);
  }
  SG_CHECK_LAUNCH();
  // read_timer("link_series_lds") = (0, 1 when the last call took the LDS form, its cells)
  timer_set_counter(ctx, "link_series_lds", (double)cells, lds ? 1u : 0u);
}

void series_finish(const SeriesCall& c) {
  sg_ctx* ctx = c.ctx;
  unsigned long long h[SERIES_WORDS];
  copy_to_host(ctx, h, ctx->l_flag.get<unsigned long long>(SERIES_WORDS), sizeof(h));
  timer_add_work(ctx, "link_series", (double)h[WALK_COUNTED]);
  // read_timer("link_series_counted") = (0, the packets the last call counted, 0)
  timer_set_counter(ctx, "link_series_counted", 0.0, h[WALK_COUNTED]);
  if (h[SERIES_BAD_SLOT] != ~0ull)
    throw Error(SG_ERR_INVALID_ARG,
                "link_slot[" + std::to_string(h[SERIES_BAD_SLOT]) + "] is neither below n_slots nor UINT32_MAX",
                (uint32_t)h[SERIES_BAD_SLOT], 0xFFFFFFFFu);
  if (h[WALK_BAD_ITEM] != ~0ull) throw_item_error(true, h[WALK_BAD_ITEM]);
  int kind = -1;
  for (int k = WALK_BAD_RANGE; k <= WALK_BAD_CYCLE; k++)
    if (h[k] != ~0ull && (kind < 0 || h[k] < h[kind])) kind = k;
  if (kind >= 0) throw_pred_error(c.net, c.nodes, kind, h[kind]);
}

}  // namespace sg

extern "C" {

int32_t sg_link_series_packets(sg_ctx* ctx, sg_net* net, sg_hosts* hosts, const uint32_t* nodes, uint32_t n_nodes,
                               uint32_t row_begin, uint32_t row_end, uint32_t flags, const uint32_t* pred,
                               const uint64_t* latency_ns, const sg_packets* packets, const uint8_t* status,
                               const uint32_t* weight, const uint32_t* link_slot, uint32_t n_slots, uint32_t at,
                               uint64_t t0_ns, uint64_t bin_ns, uint32_t n_bins, uint64_t* out_series,
                               uint64_t* out_outside) {
  return sg::guarded(ctx, [&] {
    using namespace sg;
    SeriesCall c{ctx,    net,    hosts,     nodes,   n_nodes, row_begin, row_end, pred,       latency_ns,  packets,
                 status, weight, link_slot, n_slots, at,      t0_ns,     bin_ns,  n_bins,     out_series,  out_outside};
    series_check(c, true);
    const bool dev = (flags & SG_ROUTE_OUT_DEVICE) != 0;
    const uint32_t n = n_nodes, rows = row_end - row_begin, nl = net->n_links, ni = packets->n_packets;
    if (!dev && link_slot)
      for (uint32_t k = 0; k < nl; k++)
        if (link_slot[k] >= n_slots && link_slot[k] != 0xFFFFFFFFu)
          throw Error(SG_ERR_INVALID_ARG,
                      "link_slot[" + std::to_string(k) + "] is neither below n_slots nor UINT32_MAX", k, 0xFFFFFFFFu);
    if (ni == 0) return;
    hipStream_t st = ctx->stream;
    // host rows in, host sums out: the device sums start at zero and are added on the host
    const size_t n_series = (size_t)n_slots * n_bins, n_out = out_outside ? 2 * (size_t)n_slots : 0;
    if (!dev) {
      const size_t cells = (size_t)rows * n;
      uint32_t* up = ctx->l_pred.get<uint32_t>(cells);
      uint64_t* ul = ctx->p_lat.get<uint64_t>(cells);
      if (cells) {
        SG_HIP(hipMemcpyAsync(up, pred, cells * 4, hipMemcpyHostToDevice, st));
        SG_HIP(hipMemcpyAsync(ul, latency_ns, cells * 8, hipMemcpyHostToDevice, st));
      }
      c.pred = up;
      c.lat = ul;
      if (link_slot) {
        uint32_t* us = ctx->sr_slot.get<uint32_t>(nl);
        if (nl) SG_HIP(hipMemcpyAsync(us, link_slot, (size_t)nl * 4, hipMemcpyHostToDevice, st));
        c.slot = us;
      }
      c.series = ctx->sr_series.get<uint64_t>(n_series);
      SG_HIP(hipMemsetAsync(c.series, 0, n_series * 8, st));
      if (out_outside) {
        c.outside = ctx->sr_outside.get<uint64_t>(n_out);
        SG_HIP(hipMemsetAsync(c.outside, 0, n_out * 8, st));
      }
    }
    series_enqueue(c);
    std::vector<uint64_t> h_series(dev ? 0 : n_series), h_out(dev ? 0 : n_out);
    if (!dev) {
      SG_HIP(hipMemcpyAsync(h_series.data(), c.series, n_series * 8, hipMemcpyDeviceToHost, st));
      if (n_out) SG_HIP(hipMemcpyAsync(h_out.data(), c.outside, n_out * 8, hipMemcpyDeviceToHost, st));
    }
    series_finish(c);
    for (size_t k = 0; k < h_series.size(); k++) out_series[k] += h_series[k];
    for (size_t k = 0; k < h_out.size(); k++) out_outside[k] += h_out[k];
  });
}

}  // extern "C"
