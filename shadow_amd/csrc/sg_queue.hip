// sg_queue.hip -- link queues: the FIFO wait of every crossing of a link trace under a link rate.
// The first-order scan, the host side of a call and the C entry; sg_queue.h has the definition,
// the algebra and what the layers share.
//
// Launches on the context stream, one flat scan over all records whatever the segment lengths:
//   k_queue_links   a lane per link_off entry: validates link_off (every later kernel returns at
//                   once when it is bad: no index is formed from a bad value), zeroes the per-link
//                   sums and gives an empty link its free_in value;
//   k_queue_agg     a tile of Q_TILE records per workgroup, Q_PER consecutive records per lane: the
//                   tile's aggregate (head flag, S, M).  A lane finds the link of its first record
//                   by binary search in link_off and advances through the offsets from there;
//   k_queue_carry   the tile carry: one workgroup over the tile aggregates, looping past its 1024
//                   threads: the `done` that enters each tile;
//   k_queue_rescan  the tile again with that tile carry: wait, done, out_link_free from a segment's
//                   last record, and the per-link busy / wait sums.  A lane sums its own run of
//                   equal links first; lanes whose records all lie on one link are then summed
//                   across the wave by a segmented reduction keyed by the link, and only the
//                   first lane of a run issues the atomics: a link of 100k records gets one add
//                   per wave, not one per record;
//   k_queue_ahead   a lane per record: done is non-decreasing within a segment, so ahead is one
//                   binary search over the done values of the segment's prefix; the per-link
//                   maximum by the same wave reduction.
// No workgroup waits on another inside a launch.  SG_LINK_QUEUE_SERIAL = 1 replaces agg, the tile
// carry and rescan by k_queue_serial, a lane per link looping over its segment.
//
// SG_LINK_QUEUE_CARRY carries every wait to the packet's later hops: a fixed point over the same
// scan, with every link sorted anew by the carried times in each iteration (the carried form,
// sg_queue_carry.hip).
//
// SG_LINK_QUEUE_DROP gives every link a finite buffer and drops at its tail: the unlimited scan
// above only marks the busy periods, which are then walked from an idle server side by side
// (finite buffers, sg_queue_drop.hip).
//
// SG_LINK_QUEUE_WINDOW settles the carried form up to a horizon only and hands the rest back as pending,
// in the form a later call takes as input (the windowed form, sg_queue_window.hip).
//
// SG_LINK_QUEUE_PACKETS folds the result onto the packets, behind the records of the per-record
// arrays: each packet's delay, its arrival and where it was dropped (the packet pass,
// sg_queue_packets.hip).
//
// SG_LINK_QUEUE_SERIES sums the result per slot of watched links and per time bin into a matrix behind
// out_link_busy_ns: busy time, waiting time, weight served, weight dropped (the time series,
// sg_queue_series.hip).
#include <algorithm>
#include <string>
#include <vector>

#include "sg_knobs.h"
#include "sg_queue.h"

namespace sg {

// (link_off is valid: the host's array, or a copy of the device's made when the first error asks)
struct QLocator {
  const u64* link_off;
  uint32_t n_links;
  bool dev;
  std::vector<u64> host;
  const uint32_t* packet;  // the caller's, n entries
  u64 n;
  u64 lost;  // the packet pass's count, as the last read of the flag words found it
  u64 bad_slot = Q_MAX;  // the time series' flag word, likewise
  // a record of packet p (an error's path: the whole array is read)
  u64 record_of(uint32_t p) {
    std::vector<uint32_t> h;
    const uint32_t* pk = packet;
    if (dev) {
      h.resize((size_t)n);
      if (n) SG_HIP(hipMemcpy(h.data(), packet, (size_t)n * 4, hipMemcpyDeviceToHost));
      pk = h.data();
    }
    const uint32_t* at = std::find(pk, pk + n, p);
    return at == pk + n ? 0ull : (u64)(at - pk);
  }
  void locate(u64 i, uint32_t& lk, uint32_t& at) {
    const u64* off = link_off;
    if (dev) {
      if (host.empty()) {
        host.resize((size_t)n_links + 1);
        SG_HIP(hipMemcpy(host.data(), link_off, host.size() * 8, hipMemcpyDeviceToHost));
      }
      off = host.data();
    }
    lk = (uint32_t)(std::upper_bound(off + 1, off + n_links + 1, i) - off - 1);
    at = (uint32_t)std::min<uint64_t>(i - off[lk], 0xFFFFFFFFull);
  }
};

namespace {

constexpr uint32_t Q_CARRY_THREADS = 1024;

// ---- link_off's check, the per-link sums' zeroes, the empty links
__global__ void __launch_bounds__(Q_THREADS) k_queue_links(const QArgs a) {
  const u64 q = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  if (q > a.n_links) return;
  const uint32_t lk = (uint32_t)q;
  const u64 o = a.off[lk];
  if (lk == 0 && o != 0ull) atomicMin(&a.flag[Q_BAD_OFF], 0ull);
  if (lk == a.n_links) {
    if (o != a.n) atomicMin(&a.flag[Q_BAD_OFF], (u64)lk);
    return;
  }
  const u64 o1 = a.off[lk + 1];
  if (o1 < o) atomicMin(&a.flag[Q_BAD_OFF], (u64)lk);
  if (a.out.busy) a.out.busy[lk] = 0ull;
  if (a.out.wmax) a.out.wmax[lk] = 0ull;
  if (a.out.wsum) a.out.wsum[lk] = 0ull;
  if (a.out.amax) a.out.amax[lk] = 0u;
  if (a.out.link_free && o1 == o) a.out.link_free[lk] = link_free_in(a, lk);
}

// ---- 1. the tile aggregates
__global__ void __launch_bounds__(Q_THREADS) k_queue_agg(const QArgs a) {
  __shared__ QElem s_wave[16];
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  QLane r;
  const QElem x = lane_load<true>(a, (u64)blockIdx.x * Q_TILE + (u64)threadIdx.x * Q_PER, r);
  QElem total;
  block_exclusive_op(x, q_identity(), s_wave, &total, QOp());
  if (threadIdx.x == 0) {
    a.agg_s[blockIdx.x] = total.s;
    a.agg_m[blockIdx.x] = total.m;
    a.agg_h[blockIdx.x] = total.head;
  }
}

// ---- 2. the tile carry, one workgroup: agg_m[t] = the M of everything before tile t (the `done` entering it)
__global__ void __launch_bounds__(Q_CARRY_THREADS) k_queue_carry(const QArgs a, uint32_t n_tiles) {
  __shared__ QElem s_wave[16];
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const QOp op;
  QElem carry = q_identity();
  for (uint32_t base = 0; base < n_tiles; base += Q_CARRY_THREADS) {
    const uint32_t b = base + threadIdx.x;
    const QElem x = b < n_tiles ? QElem{a.agg_s[b], a.agg_m[b], a.agg_h[b]} : q_identity();
    QElem total;
    const QElem ex = block_exclusive_op(x, q_identity(), s_wave, &total, op);
    if (b < n_tiles) a.agg_m[b] = op(carry, ex).m;
    carry = op(carry, total);
  }
}

__device__ __forceinline__ void link_sums_add(const QArgs& a, uint32_t link, const QSums& x) {
  if (a.out.busy && x.busy) atomicAdd(&a.out.busy[link], x.busy);
  if (a.out.wmax && x.wmax) atomicMax(&a.out.wmax[link], x.wmax);
  if (a.out.wsum && x.wsum) atomicAdd(&a.out.wsum[link], x.wsum);
}

// ---- 3. the tile again, with its tile carry
__global__ void __launch_bounds__(Q_THREADS) k_queue_rescan(const QArgs a) {
  __shared__ QElem s_wave[16];
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 base = (u64)blockIdx.x * Q_TILE + (u64)threadIdx.x * Q_PER;
  const bool sums = a.out.busy || a.out.wmax || a.out.wsum;
  QSums run = {0ull, 0ull, 0ull};
  uint32_t run_link = Q_NO_LINK;
  QLane r;
  tile_rescan(a, s_wave, base, r, [&](uint32_t k, u64 start, u64 done) {
    const uint32_t lk = r.link[k];
    const u64 wait = start - r.e[k];
    if (done == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], base + k);
    if (a.out.wait) a.out.wait[base + k] = wait;
    if (a.out.done) a.out.done[base + k] = done;
    if (a.out.link_free && ((r.last >> k) & 1u)) a.out.link_free[lk] = done;
    if (sums) {
      if (lk != run_link) {
        if (run_link != Q_NO_LINK) link_sums_add(a, run_link, run);
        run_link = lk;
        run = QSums{0ull, 0ull, 0ull};
      }
      run.busy += r.s[k];
      run.wmax = max(run.wmax, wait);
      run.wsum += wait;
    }
  });
  if (sums) {  // (the same for every lane of the launch)
    // a lane whose records lie on one link joins the wave's reduction; any other adds its last run itself
    uint32_t key = Q_NO_LINK;
    if (r.count && r.link[0] == run_link) {
      key = run_link;
    } else if (run_link != Q_NO_LINK) {
      link_sums_add(a, run_link, run);
    }
    run = wave_run_reduce(key, run, QSumsOp());
    if (wave_run_first(key)) link_sums_add(a, key, run);
  }
}

// ---- the lane-per-link form
__global__ void __launch_bounds__(Q_THREADS) k_queue_serial(const QArgs a) {
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 stride = (u64)gridDim.x * Q_THREADS;
  for (u64 q = (u64)blockIdx.x * Q_THREADS + threadIdx.x; q < a.n_links; q += stride) {
    const uint32_t lk = (uint32_t)q;
    const u64 i0 = a.off[lk], i1 = a.off[lk + 1];
    if (i0 == i1) continue;  // (k_queue_links wrote an empty link's outputs)
    const u64 cost = a.cost[lk];
    u64 done = link_free_in(a, lk);
    QSums run = {0ull, 0ull, 0ull};
    for (u64 i = i0; i < i1; i++) {
      const u64 s = service_ns(record_weight(a, i, true), cost), e = a.enter[i];
      const u64 start = max(e, done), wait = start - e;
      done = sat_add(start, s);
      if (done == Q_MAX) atomicMin(&a.flag[Q_OVERFLOW], i);
      if (a.out.wait) a.out.wait[i] = wait;
      if (a.out.done) a.out.done[i] = done;
      run.busy += s;
      run.wmax = max(run.wmax, wait);
      run.wsum += wait;
    }
    if (a.out.link_free) a.out.link_free[lk] = done;
    if (a.out.busy) a.out.busy[lk] = run.busy;
    if (a.out.wmax) a.out.wmax[lk] = run.wmax;
    if (a.out.wsum) a.out.wsum[lk] = run.wsum;
  }
}

// ---- ahead: the records of the segment's prefix still in the system when record i arrives
__global__ void __launch_bounds__(Q_THREADS) k_queue_ahead(const QArgs a) {
  if (a.flag[Q_BAD_OFF] != Q_MAX) return;
  const u64 i = (u64)blockIdx.x * Q_THREADS + threadIdx.x;
  uint32_t key = Q_NO_LINK, ahead = 0u;
  if (i < a.n) {
    key = link_of(a.off, a.n_links, i);
    // the first j of the prefix with done[j] > enter[i]
    ahead = (uint32_t)min(i - upper_bound(a.out.done, a.off[key], i, a.enter[i]), (u64)0xFFFFFFFFull);
    if (a.out.ahead) a.out.ahead[i] = ahead;
  }
  if (!a.out.amax) return;  // (the same for every lane)
  const uint32_t m = wave_run_reduce(key, ahead, [](uint32_t x, uint32_t y) { return max(x, y); });
  if (wave_run_first(key) && m) atomicMax(&a.out.amax[key], m);
}

// the first bad link of a host link_off; all ones when it is good
u64 bad_link_off(const u64* off, uint32_t n_links, u64 n) {
  if (off[0] != 0) return 0;
  for (uint32_t k = 0; k < n_links; k++)
    if (off[k + 1] < off[k]) return k;
  return off[n_links] != n ? (u64)n_links : Q_MAX;
}

[[noreturn]] void throw_bad_off(u64 link) {
  throw Error(SG_ERR_INVALID_ARG,
              "link_off is not an offset array of the records at link " + std::to_string(link) +
                  " (it starts at 0, never falls and ends at n_records)",
              (uint32_t)link, 0xFFFFFFFFu);
}

// c: the caller's arrays as given, on the host or on the device.
void queue_run(sg_ctx* ctx, uint32_t flags, const QArgs& c) {
  if (!c.off || !c.enter || !c.cost) throw Error(SG_ERR_INVALID_ARG, "null link_off, enter_ns or cost_ps");
  if (!c.out.wait && !c.out.done && !c.out.ahead && !c.out.link_free && !c.out.busy && !c.out.wmax && !c.out.wsum && !c.out.amax)
    throw Error(SG_ERR_INVALID_ARG, "no output");
  if (c.weight && !c.packet) throw Error(SG_ERR_INVALID_ARG, "weight without packet");
  if (c.out.link_free && c.out.link_free == c.free_in) throw Error(SG_ERR_INVALID_ARG, "out_link_free is link_free_in");
  const bool dev = (flags & SG_ROUTE_OUT_DEVICE) != 0;
  const uint32_t nl = c.n_links;
  const uint64_t n = c.n;
  if (flags & SG_LINK_QUEUE_CARRY) {
    if (!c.packet) throw Error(SG_ERR_INVALID_ARG, "SG_LINK_QUEUE_CARRY without packet");
    // (the record index is a word of the sort's key, and UINT32_MAX is its padding)
    if (n > 0xFFFFFFFEull) throw Error(SG_ERR_CAPACITY, "more records than one carried call takes");
  }
  const bool window = (flags & SG_LINK_QUEUE_WINDOW) != 0;
  if (window) {
    if (!(flags & SG_LINK_QUEUE_CARRY)) throw Error(SG_ERR_INVALID_ARG, "SG_LINK_QUEUE_WINDOW without SG_LINK_QUEUE_CARRY");
    if (!c.free_in) throw Error(SG_ERR_INVALID_ARG, "SG_LINK_QUEUE_WINDOW without link_free_in (the horizon is its last entry)");
    // (0xFFFFFFFD in where is "in flight": a record index stays below it)
    if (n > 0xFFFFFFFDull) throw Error(SG_ERR_CAPACITY, "more records than one call with SG_LINK_QUEUE_WINDOW takes");
  }
  const bool carry = (flags & SG_LINK_QUEUE_CARRY) != 0 && n != 0;  // (no record: nothing to carry)
  const bool drop = (flags & SG_LINK_QUEUE_DROP) != 0;
  const bool packets = (flags & SG_LINK_QUEUE_PACKETS) != 0;
  if (packets) {
    if (!c.packet) throw Error(SG_ERR_INVALID_ARG, "SG_LINK_QUEUE_PACKETS without packet");
    if (!c.out.wait || !c.out.done || !c.out.ahead)
      throw Error(SG_ERR_INVALID_ARG, "SG_LINK_QUEUE_PACKETS without out_wait_ns, out_done_ns or out_ahead");
    // (a record index shares out_ahead's tail with the two codes)
    if (n > 0xFFFFFFFEull) throw Error(SG_ERR_CAPACITY, "more records than one call with SG_LINK_QUEUE_PACKETS takes");
  }
  const size_t n_rec = (size_t)n + (packets ? (size_t)c.n_weights : 0);  // enter_ns and the per-record outputs
  // (the period starts are u32 record indices, and the marks are summed by scan_counts)
  if (drop && n > 0xFFFFFFFEull) throw Error(SG_ERR_CAPACITY, "more records than one call with SG_LINK_QUEUE_DROP takes");
  const size_t nl2 = drop ? 2 * (size_t)nl : (size_t)nl;  // cost_ps, out_link_busy_ns, out_link_ahead_max
  // the time series: the header and the slot map behind cost_ps, the matrix behind out_link_busy_ns
  const bool series = (flags & SG_LINK_QUEUE_SERIES) != 0;
  QSeries sr = {};
  size_t cost_tail = 0, busy_tail = 0;
  if (series) {
    if (!c.out.wait || !c.out.done || !c.out.busy || (window && !c.out.ahead))
      throw Error(SG_ERR_INVALID_ARG,
                  "SG_LINK_QUEUE_SERIES without out_wait_ns, out_done_ns or out_link_busy_ns (with SG_LINK_QUEUE_WINDOW: or out_ahead)");
    sr = queue_series_plan(ctx, c.cost + nl2, dev, nl);
    cost_tail = 4 + (sr.mapped ? (size_t)nl : 0);
    busy_tail = 4 * (size_t)sr.cells;
  }
  if (!dev) {
    const u64 bad = bad_link_off(c.off, nl, n);
    if (bad != Q_MAX) throw_bad_off(bad);
  }
  const uint64_t n_tiles64 = (n + Q_TILE - 1) / Q_TILE;
  if (n_tiles64 > 0x7FFFFFFFull) throw Error(SG_ERR_CAPACITY, "more records than one call scans");
  hipStream_t st = ctx->stream;

  // host arrays in: device copies; host outputs: device arrays copied back at the end
  struct Back {
    void* host;
    const void* dev;
    size_t bytes;
  };
  std::vector<Back> back;
  int slot = 0;
  auto in = [&](const void* p, size_t bytes) -> const void* {
    sg::DevBuf& b = ctx->q_buf[slot++];
    if (!p || dev) return p;
    char* d = b.get<char>(bytes);
    if (bytes) SG_HIP(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, st));
    return d;
  };
  // (tail: bytes of the device copy behind the output's own, not copied back here)
  auto out = [&](void* p, size_t bytes, size_t tail = 0) -> void* {
    sg::DevBuf& b = ctx->q_buf[slot++];
    if (!p || dev) return p;
    char* d = b.get<char>(bytes + tail);
    back.push_back(Back{p, d, bytes});
    return d;
  };
  QArgs call = {};
  call.n_links = nl;
  call.n = n;
  call.n_weights = c.n_weights;
  call.off = (const u64*)in(c.off, ((size_t)nl + 1) * 8);
  const u64* enter = (const u64*)in(c.enter, n_rec * 8);
  const uint32_t* packet = (const uint32_t*)in(c.packet, n * 4);
  call.weight = (const uint32_t*)in(c.weight, (size_t)c.n_weights * 4);
  call.cost = (const u64*)in(c.cost, (nl2 + cost_tail) * 8);
  call.free_in = (const u64*)in(c.free_in, ((size_t)nl + (window ? 1 : 0)) * 8);  // (windowed: the horizon behind the links)
  QOuts outs = {};
  outs.wait = (u64*)out(c.out.wait, n_rec * 8);
  outs.done = (u64*)out(c.out.done, n_rec * 8);
  outs.ahead = (uint32_t*)out(c.out.ahead, n_rec * 4);
  outs.link_free = (u64*)out(c.out.link_free, (size_t)nl * 8);
  outs.busy = (u64*)out(c.out.busy, nl2 * 8, busy_tail * 8);
  // (host mode: the matrix's device sums start at zero and are added into the host array's tail)
  if (series && !dev && busy_tail) SG_HIP(hipMemsetAsync(outs.busy + nl2, 0, busy_tail * 8, st));
  outs.wmax = (u64*)out(c.out.wmax, (size_t)nl * 8);
  outs.wsum = (u64*)out(c.out.wsum, (size_t)nl * 8);
  outs.amax = (uint32_t*)out(c.out.amax, nl2 * 4);
  // (k_queue_ahead searches the done times: a scratch array where the caller takes none)
  if ((outs.ahead || outs.amax) && !outs.done && !carry && !drop) outs.done = ctx->q_done.get<u64>(n);
  call.flag = ctx->q_flag.get<u64>(Q_WORDS);
  SG_HIP(hipMemsetAsync(call.flag, 0xff, Q_WORDS * 8, st));

  const bool serial = knob_int("SG_LINK_QUEUE_SERIAL", 0) != 0;
  // read_timer("link_queue_serial") = (0, 1 when the last call took the lane-per-link form, its records)
  timer_set_counter(ctx, "link_queue_serial", (double)n, serial ? 1u : 0u);
  if (!serial && n) {
    u64* agg = ctx->q_agg.get<u64>(3 * (size_t)n_tiles64);
    call.agg_s = agg;
    call.agg_m = agg + n_tiles64;
    call.agg_h = (uint32_t*)(agg + 2 * (size_t)n_tiles64);
  }
  const QArgs a = queue_pass(call, enter, packet, outs);
  QLocator where = {c.off, nl, dev, {}, c.packet, n, 0};

  // read_timer("link_queue_active") = (0, the records the last windowed call sorted and scanned, summed over its
  // iterations, its records)
  if (window) timer_set_counter(ctx, "link_queue_active", (double)n, 0u, true);
  if (carry && window) {
    queue_window(ctx, a, drop, packets, where);
  } else if (carry) {
    queue_carry(ctx, a, drop, packets, where);
  } else {
    queue_output_pass(ctx, a, drop, nullptr, false);
    if (packets) queue_packets(ctx, a, drop, nullptr);
    if (series) queue_series(ctx, a, sr, drop, false);
    queue_check_flags(ctx, a.flag, where, false, true);
  }
  if (series) {
    // (carried, the outputs stand at the input indices now, and the flag words are read once more)
    if (carry) {
      queue_series(ctx, a, sr, drop, window);
      queue_check_flags(ctx, a.flag, where, true, false);
    }
    if (where.bad_slot != Q_MAX)
      throw Error(SG_ERR_INVALID_ARG,
                  "SG_LINK_QUEUE_SERIES: the slot of link " + std::to_string(where.bad_slot) + " is not below n_slots and not 2^64 - 1",
                  (uint32_t)where.bad_slot, 0xFFFFFFFFu);
  }
  // read_timer("link_queue_lost") = (0, the packets the last call with SG_LINK_QUEUE_PACKETS found dropped, its packets)
  if (packets) timer_set_counter(ctx, "link_queue_lost", (double)c.n_weights, where.lost, true);
  for (const Back& b : back)
    if (b.bytes) SG_HIP(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st));
  std::vector<u64> sums;
  if (series && !dev && busy_tail) {
    sums.resize(busy_tail);
    SG_HIP(hipMemcpyAsync(sums.data(), outs.busy + nl2, busy_tail * 8, hipMemcpyDeviceToHost, st));
  }
  if (!back.empty()) SG_HIP(hipStreamSynchronize(st));
  for (size_t k = 0; k < sums.size(); k++) c.out.busy[nl2 + k] += sums[k];
}

}  // namespace

bool queue_check_flags(sg_ctx* ctx, const u64* flag, QLocator& where, bool carried, bool inputs, u64* active) {
  u64 h[Q_WORDS];
  copy_to_host(ctx, h, flag, sizeof(h));
  if (active) *active = h[Q_ACTIVE];
  uint32_t lk, at;
  if (inputs) {
    if (h[Q_BAD_OFF] != Q_MAX) throw_bad_off(h[Q_BAD_OFF]);
    if (h[Q_BAD_PACKET] != Q_MAX) {
      where.locate(h[Q_BAD_PACKET], lk, at);
      throw Error(SG_ERR_INVALID_ARG,
                  "packet[" + std::to_string(h[Q_BAD_PACKET]) + "] is not below n_weights (link " + std::to_string(lk) + ")",
                  lk, at);
    }
    if (h[Q_DUP] != Q_MAX) {
      where.locate(h[Q_DUP], lk, at);
      throw Error(SG_ERR_INVALID_ARG,
                  "record " + std::to_string(h[Q_DUP]) + " (link " + std::to_string(lk) +
                      ") enters at the time of another record of its packet",
                  lk, at);
    }
  }
  if (h[Q_OVERFLOW] != Q_MAX) {
    where.locate(h[Q_OVERFLOW], lk, at);
    throw Error(SG_ERR_TIME_OVERFLOW,
                carried ? "a record of link " + std::to_string(lk) + " is served or carried past 2^64 - 1 ns"
                        : "record " + std::to_string(h[Q_OVERFLOW]) + " of link " + std::to_string(lk) +
                              " is served past 2^64 - 1 ns",
                lk, at);
  }
  if (h[Q_PKT_OVERFLOW] != Q_MAX) {
    where.locate(where.record_of((uint32_t)h[Q_PKT_OVERFLOW]), lk, at);
    throw Error(SG_ERR_TIME_OVERFLOW,
                "packet " + std::to_string(h[Q_PKT_OVERFLOW]) + " (a record of link " + std::to_string(lk) +
                    ") arrives past 2^64 - 1 ns",
                lk, at);
  }
  where.lost = h[Q_LOST];
  where.bad_slot = h[Q_BAD_SLOT];
  return h[Q_CHANGED] == Q_MAX;
}

const u64* launch_walk(sg_ctx* ctx, const QArgs& a, bool drop, u64* carried_run) {
  hipStream_t st = ctx->stream;
  TimedLaunch tl(ctx, "link_queue", (double)a.n);
  const bool serial = queue_serial(a);
  if (!serial) {
    hipLaunchKernelGGL(k_queue_agg, dim3(queue_tiles(a)), dim3(Q_THREADS), 0, st, a);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_queue_carry, dim3(1), dim3(Q_CARRY_THREADS), 0, st, a, queue_tiles(a));
    SG_CHECK_LAUNCH();
  }
  if (drop) return drop_launch_walk(ctx, a, carried_run);
  if (serial) {
    hipLaunchKernelGGL(k_queue_serial, dim3(grid_for(a.n_links, Q_THREADS, 16u * (unsigned)ctx->n_cu)), dim3(Q_THREADS),
                       0, st, a);
    SG_CHECK_LAUNCH();
  } else {
    hipLaunchKernelGGL(k_queue_rescan, dim3(queue_tiles(a)), dim3(Q_THREADS), 0, st, a);
    SG_CHECK_LAUNCH();
  }
  return nullptr;
}

void launch_links(sg_ctx* ctx, const QArgs& a) {
  hipLaunchKernelGGL(k_queue_links, dim3(grid_for((size_t)a.n_links + 1, Q_THREADS)), dim3(Q_THREADS), 0, ctx->stream, a);
  SG_CHECK_LAUNCH();
}

void queue_output_pass(sg_ctx* ctx, const QArgs& a, bool drop, u64* carried_run, bool walk_stands) {
  launch_links(ctx, a);
  if (drop) drop_launch_links(ctx, a);
  if (!a.n) return;
  if (!walk_stands) launch_walk(ctx, a, drop, carried_run);
  if (!drop && !a.out.ahead && !a.out.amax) return;
  TimedLaunch tl(ctx, "link_queue_ahead", (double)a.n);
  if (drop) {
    drop_launch_finish(ctx, a, carried_run);
  } else {
    hipLaunchKernelGGL(k_queue_ahead, dim3(grid_for(a.n, Q_THREADS, 0x7FFFFFFFu)), dim3(Q_THREADS), 0, ctx->stream, a);
    SG_CHECK_LAUNCH();
  }
}

}  // namespace sg

extern "C" {

int32_t sg_link_queue(sg_ctx* ctx, uint32_t flags, uint32_t n_links, const uint64_t* link_off, uint64_t n_records,
                      const uint64_t* enter_ns, const uint32_t* packet, const uint32_t* weight, uint32_t n_weights,
                      const uint64_t* cost_ps, const uint64_t* link_free_in, uint64_t* out_wait_ns,
                      uint64_t* out_done_ns, uint32_t* out_ahead, uint64_t* out_link_free, uint64_t* out_link_busy_ns,
                      uint64_t* out_link_wait_max_ns, uint64_t* out_link_wait_sum_ns, uint32_t* out_link_ahead_max) {
  return sg::guarded(ctx, [&] {
    using sg::u64;
    sg::queue_run(ctx, flags,
                  sg::QArgs{(const u64*)link_off, n_links, n_records, (const u64*)enter_ns, packet, weight, n_weights,
                            (const u64*)cost_ps, (const u64*)link_free_in,
                            sg::QOuts{(u64*)out_wait_ns, (u64*)out_done_ns, out_ahead, (u64*)out_link_free,
                                      (u64*)out_link_busy_ns, (u64*)out_link_wait_max_ns, (u64*)out_link_wait_sum_ns,
                                      out_link_ahead_max}});
  });
}

}  // extern "C"
