// sg_slab.hip -- the shortest-path searches that work in global memory.
//
//  * The batched-source slab search (k_relax_w2; graphs past the per-source searches,
//    or SG_APSP_LDS=0): pull relaxation to the fixed point sg_routing.hip's header
//    describes.  A wave owns a few destination nodes of one 64-source batch; lane =
//    source.  The batch's distance slab is laid out [node][64 sources], so each in-arc
//    (u -> v) costs one coalesced 512-B read of D[u][0..63] and 64 independent
//    relaxations.  Keys are packed (latency u32 << 32) | f32 bits(loss) (sg_device.h).
//  * The wide fallback (k_relax_wide, run_wide): rows in which some search met a
//    saturated key (a path of 4.29 s or more, or an unreachable node) are redone with
//    u64 latency and f32 loss, Jacobi.
//
// In-place (Gauss-Seidel) updates in k_relax_w2.  A flush writes a lane's two
// keys with one 16-B store while other waves may gather the same row with 16-B
// loads.  Each key is one aligned 8-B half of that store.  MI355X_MICROARCH.md
// records untorn 16-B halves on gfx950 as observed, not architecturally
// guaranteed; the exactness argument needs only that each aligned 8-B key is
// read whole (a 64-bit access), which is how the vector memory path moves
// aligned dwordx2 halves.  Dense graphs (arc segments) flush with 64-bit
// atomicMin instead.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sg_device.h"
#include "sg_internal.h"
#include "sg_knobs.h"

namespace sg {

constexpr int BATCH = 64;         // sources per batch = wave width
constexpr int RELAX_WAVES = 4;    // waves per block (wide kernel)
constexpr int RELAX_BLOCK = RELAX_WAVES * 64;

// ---------------------------------------------------------------------------
// Batched-source relaxation (the hot kernel).
//
// B sources per batch (lane = source).  A batch's distance slab is laid out
// D[node][B] (u64 keys, 8 B x B per node), so one in-arc u -> v costs one
// coalesced row read of D[u][0..B-1] and B independent relaxations.
//
// k_relax_w: one wave per work item (active batch, NPW consecutive destination
// nodes); see the kernel's comment.  XCD-aware 1-D grid: dispatch deals blocks
// round-robin over the 8 XCDs (MI355X_MICROARCH.md, "Workgroup dispatch"), so
// block L runs on XCD L % 8, and the items of one batch all go to blocks of one
// residue: the waves of an XCD share a slab in its L2.  Placement changes speed
// only, never results.
//
// Frontier (FRONT): stamp[batch][node] = p + 2 when the node's key changed in
// pass p (sources start at 1).  In pass p an arc is relaxed only when its
// source's stamp >= p + 1, i.e. the source changed in pass p - 1 or earlier in
// pass p.  Exactness: a value written in pass p is re-read by every out-arc in
// pass p + 1 (a kernel boundary, so visible), and iteration stops only after a
// pass with no change anywhere -- then every arc satisfies D[v] <= D[u] (+) w,
// the fixed point, which is petgraph's Dijkstra result (see header).
// ---------------------------------------------------------------------------
constexpr int RELAX_THREADS = 256;
constexpr uint32_t FLAG_STRIDE = 32;  // per-batch pass flags 128 B apart: no two batches share a cache line

// One 8-B key through a buffer descriptor (32-bit per-lane byte offset).  An
// offset of OOB lies outside every slab: the load returns 0 and moves no data.
constexpr uint32_t OOB = 0x80000000u;
constexpr uint32_t PREFETCH_MIN = 16;  // dirty arcs from which an item prefetches all its rows
__device__ __forceinline__ uint64_t load_key(__amdgpu_buffer_rsrc_t rsrc, uint32_t off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0);
  return ((uint64_t)v[1] << 32) | v[0];
}

// Slab init: every key KEY_INF (16-B stores, no per-element index arithmetic),
// every stamp 0; k_stamp_sources then marks the sources.  (An earlier version
// tested each element against its batch's sources with 64-bit divisions and
// ran at about 0.3 TB/s.)
template <int B>
__global__ void k_init_batch(uint64_t* __restrict__ D, uint32_t* __restrict__ stamp, uint32_t n,
                             uint32_t n_batches) {
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const size_t pairs = (size_t)n_batches * n * (B / 2), stride = (size_t)gridDim.x * blockDim.x;
  const u64x2 inf = {KEY_INF, KEY_INF};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride)
    __builtin_nontemporal_store(inf, (u64x2*)D + i);
  const size_t ns = (size_t)n_batches * n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += stride) stamp[i] = 0;
}

// Sources: key 0 (PathProperties::default()) and stamp 1, one thread per row.
template <int B>
__global__ void k_stamp_sources(uint64_t* __restrict__ D, uint32_t* __restrict__ stamp, uint32_t n,
                                const uint32_t* __restrict__ used, uint32_t first_row, uint32_t row_end,
                                uint32_t n_batches) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_batches * B) return;
  const uint32_t row = first_row + t;
  if (row >= row_end) return;
  const size_t bv = (size_t)(t / B) * n + used[row];
  stamp[bv] = 1;
  D[bv * B + (t % B)] = 0ull;
}

// Active-batch list for the next pass: alist[0] = count, alist[1 + i] = the
// i-th batch (ascending) whose flag is set.  One block.  Also zeroes the flag
// slot the pass will set (`clear`, gb x FLAG_STRIDE words) and, if count_out
// (pinned host-mapped) is given, reports the count there: no fill and no copy
// per pass.
__global__ void __launch_bounds__(1024) k_active_list(const uint32_t* __restrict__ flags, uint32_t gb,
                                                      uint32_t* __restrict__ alist, uint32_t* __restrict__ clear,
                                                      uint32_t* __restrict__ count_out) {
  for (uint32_t i = threadIdx.x; i < gb * FLAG_STRIDE; i += 1024) clear[i] = 0;
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t base;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (uint32_t b0 = 0; b0 < gb; b0 += 1024) {
    const uint32_t b = b0 + threadIdx.x;
    const bool on = b < gb && flags[b * FLAG_STRIDE] != 0;
    const uint64_t m = __ballot(on);
    if (lane == 0) wsum[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = base;
    for (int i = 0; i < wv; i++) off += wsum[i];
    if (on) alist[1 + off + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = b;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < 16; i++) base += wsum[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    alist[0] = base;
    if (count_out) *count_out = base;
  }
}

// B = sources per batch (64: one row per wave instruction; 32: two rows, one
// per half-wave, and a 2.5 MB slab at 10k nodes that stays in one XCD's L2).
template <int B, int NPW, int K, int GROUP, bool FRONT, bool COUNT>
__global__ void __launch_bounds__(RELAX_THREADS)
    k_relax_w(const uint32_t* __restrict__ in_off, const uint4* __restrict__ in_rec, uint64_t* __restrict__ D,
              uint32_t n, const uint32_t* __restrict__ alist, uint32_t* __restrict__ changed,
              uint32_t* __restrict__ stamp, uint32_t pass, unsigned long long* __restrict__ work) {
  constexpr int WAVES = RELAX_THREADS / 64;
  constexpr int STG_W = 64 * K;
  constexpr int G = 64 / B;  // rows per wave instruction
  static_assert(NPW % G == 0, "NPW must be a multiple of the rows per instruction");
  __shared__ uint4 lists[WAVES][STG_W];  // (source row byte offset, destination slot, latency, 1 - loss)
  __shared__ unsigned long long bests[WAVES][NPW * B];
  const int lane = threadIdx.x & 63;
  const uint32_t gh = lane / B, sl = lane % B;  // row group within the instruction, source lane
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lane8 = sl * 8;
  uint4* list = lists[w];
  unsigned long long* best = bests[w];
  // Work items (active batch, wave chunk): the active batches with list index
  // i = x (mod 8) go to the blocks L = x (mod 8), i.e. to XCD x under
  // round-robin dispatch, so the remaining work stays spread over all XCDs as
  // batches converge; consecutive items are consecutive chunks of one batch, so
  // an XCD's resident waves share a slab.
  const uint32_t x = blockIdx.x & 7;
  const uint32_t nwc = (n + NPW - 1) / NPW;
  const uint32_t n_act = alist[0];
  const uint32_t nbx = n_act > x ? (n_act - x + 7) / 8 : 0;
  constexpr uint32_t nseg = 1;  // (segments: k_relax_w2 only)
  // nseg > 1 (dense graphs): an item is one of nseg segments of a node chunk's
  // in-arcs, so a chunk's thousands of arcs are relaxed by nseg waves at once;
  // the segments' waves share rows and merge by 64-bit atomic min (the packed
  // key's order is the PathProperties order)
  const uint32_t items = nbx * nwc * nseg;
  const uint32_t stride = (gridDim.x >> 3) * WAVES;
  uint32_t n_rel = 0, flagged = ~0u;
  for (uint32_t it = (blockIdx.x >> 3) * WAVES + w; it < items; it += stride) {
    const uint32_t b = alist[1 + x + 8 * (it / (nwc * nseg))];
    const uint32_t ci = it % (nwc * nseg);
    const uint32_t vw = (ci / nseg) * NPW, seg = ci % nseg;
    const uint32_t vw1 = min(vw + NPW, n);
    uint64_t* Db = D + (size_t)b * n * B;
    const uint32_t* St = stamp + (size_t)b * n;
    const __amdgpu_buffer_rsrc_t slab = __builtin_amdgcn_make_buffer_rsrc(Db, 0, (int)(n * B * 8u), 0x00020000);
    uint32_t a0 = in_off[vw], a1 = in_off[vw1];
    if (nseg > 1) {
      const uint32_t per = (a1 - a0 + nseg - 1) / nseg;
      a0 = min(a1, a0 + seg * per);
      a1 = min(a1, a0 + per);
    }
    uint32_t n_cand = 0;
    uint32_t run_slot = 0;  // per row group: records of one destination form a run
    uint64_t run = KEY_INF;
    bool prefetched = false;
    uint64_t cur[NPW / G];
    for (uint32_t c0 = a0; c0 < a1; c0 += STG_W) {
      const uint32_t c1 = min(c0 + STG_W, a1);
      uint4 ra[K];
      bool dirty[K];
#pragma unroll
      for (int i = 0; i < K; i++) ra[i] = in_rec[min(c0 + lane + 64 * i, c1 - 1)];
#pragma unroll
      for (int i = 0; i < K; i++) dirty[i] = c0 + lane + 64 * i < c1 && (!FRONT || St[ra[i].x] > pass);
      uint32_t cnt = 0;
#pragma unroll
      for (int i = 0; i < K; i++) {
        const uint64_t m = __ballot(dirty[i]);
        if (dirty[i])
          list[cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1))] =
              make_uint4(ra[i].x * (B * 8), ra[i].y - vw, ra[i].z, ra[i].w);
        cnt += (uint32_t)__popcll(m);
      }
      if (cnt && !n_cand) {  // first candidates of this item: reset its LDS rows
#pragma unroll
        for (int i = 0; i < NPW * B / 64; i++) best[i * 64 + lane] = KEY_INF;
      }
      n_cand += cnt;
      if (cnt >= PREFETCH_MIN && !prefetched) {  // dense item: fetch its rows now, under the relax loop
        prefetched = true;
#pragma unroll
        for (int i = 0; i < NPW / G; i++)
          cur[i] = load_key(slab, min(vw + i * G + gh, vw1 - 1) * (B * 8) + lane8);
      }
      // Records arrive in destination order (CSC order, compaction keeps it);
      // row group gh takes records gh, gh + G, ..., so each destination's
      // candidates form one run per group, folded in registers and merged into
      // the destination's LDS row (ds_min) when the destination changes.
      uint32_t g = 0;
      for (; g + GROUP * G <= cnt; g += GROUP * G) {
        uint4 r[GROUP];
        uint64_t k[GROUP];
#pragma unroll
        for (int j = 0; j < GROUP; j++) r[j] = list[g + j * G + gh];
#pragma unroll
        for (int j = 0; j < GROUP; j++) k[j] = load_key(slab, r[j].x + lane8);
#pragma unroll
        for (int j = 0; j < GROUP; j++) {
          const uint32_t slot = G == 1 ? __builtin_amdgcn_readfirstlane(r[j].y) : r[j].y;
          if (slot != run_slot) {
            atomicMin(&best[run_slot * B + sl], (unsigned long long)run);
            run_slot = slot;
            run = KEY_INF;
          }
          run = min(run, relax32(k[j], r[j].z, __uint_as_float(r[j].w)));
        }
      }
      for (; g < cnt; g += G) {
        const uint32_t idx = g + gh;
        if (idx < cnt) {
          const uint4 r = list[idx];
          if (r.y != run_slot) {
            atomicMin(&best[run_slot * B + sl], (unsigned long long)run);
            run_slot = r.y;
            run = KEY_INF;
          }
          run = min(run, relax32(load_key(slab, r.x + lane8), r.z, __uint_as_float(r.w)));
        }
      }
    }
    if (COUNT) n_rel += n_cand;
    if (!n_cand) continue;
    atomicMin(&best[run_slot * B + sl], (unsigned long long)run);
    // flush: improved keys are written in place (one untorn 64-bit update each).
    // A sparse item reads only the lanes that received a candidate (the others
    // take an out-of-range offset: no memory traffic, value 0, no change).
    uint64_t nbv[NPW / G];
#pragma unroll
    for (int i = 0; i < NPW / G; i++) nbv[i] = best[(i * G + gh) * B + sl];
    if (!prefetched) {
#pragma unroll
      for (int i = 0; i < NPW / G; i++)
        cur[i] = load_key(slab, nbv[i] != KEY_INF ? min(vw + i * G + gh, vw1 - 1) * (B * 8) + lane8 : OOB);
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < NPW / G; i++) {
      const uint32_t v = vw + i * G + gh;
      const uint64_t nb = nbv[i];
      const bool ch = v < vw1 && nb < cur[i];
      if (ch) Db[(size_t)v * B + sl] = nb;
      const uint64_t m = __ballot(ch);
      if (m) {
        any = true;
        if (FRONT && sl == 0 && ((m >> (gh * B)) & (B == 64 ? ~0ull : ((1ull << B) - 1))))
          stamp[(size_t)b * n + v] = pass + 2;
      }
    }
    // one flag store per wave and batch (a wave's items run batch by batch)
    if (any && b != flagged) {
      if (lane == 0) changed[b * FLAG_STRIDE] = 1u;
      flagged = b;
    }
  }
  if (COUNT && lane == 0 && n_rel) atomicAdd(&work[blockIdx.x & (WORK_SHARDS - 1)], (unsigned long long)n_rel * B);
}

// Two 8-B keys (16 B) through the buffer descriptor; OOB -> zeros, no traffic.
__device__ __forceinline__ void load_key2(__amdgpu_buffer_rsrc_t rsrc, uint32_t off, uint64_t& k0, uint64_t& k1) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
  k0 = ((uint64_t)v[1] << 32) | v[0];
  k1 = ((uint64_t)v[3] << 32) | v[2];
}

// k_relax_w2: the B = 64 relaxation with two sources per lane.  A row (64 keys,
// 512 B) is read by 32 lanes with 16-B loads, so one wave instruction reads
// two rows (two arcs, one per half-wave): half the vector-memory instructions
// per relaxation.  The texture-address unit, 80 % busy in k_relax_w (PMC
// TA_TA_BUSY), processes one instruction's 64 addresses whatever their width.
// Same work items, frontier, LDS merge and flush as k_relax_w; a flush writes
// both keys of a lane with one 16-B store (the row's only writer is this wave,
// so the unchanged half is rewritten with the value it holds).
// B = 32 (SG_APSP_B=32): 16 lanes per row, four rows per wave instruction, and
// a 2.5 MB slab at 10k nodes that fits one XCD's 4 MB L2.
template <int B, int NPW, int K, int GROUP, bool FRONT, bool COUNT>
__global__ void __launch_bounds__(RELAX_THREADS)
    k_relax_w2(const uint32_t* __restrict__ in_off, const uint4* __restrict__ in_rec, uint64_t* __restrict__ D,
               uint32_t n, const uint32_t* __restrict__ alist, uint32_t* __restrict__ changed,
               uint32_t* __restrict__ stamp, uint32_t pass, unsigned long long* __restrict__ work, uint32_t nseg) {
  static_assert(B == 64 || B == 32, "B = 64 or 32");
  constexpr int WAVES = RELAX_THREADS / 64;
  constexpr int STG_W = 64 * K;
  constexpr int LPR = B / 2;   // lanes per row
  constexpr int G = 64 / LPR;  // rows per wave instruction
  constexpr uint64_t ROW_MASK = LPR == 64 ? ~0ull : (1ull << LPR) - 1;
  static_assert(NPW % G == 0, "NPW must be a multiple of the rows per instruction");
  __shared__ uint4 lists[WAVES][STG_W];
  __shared__ unsigned long long bests[WAVES][NPW * B];
  const int lane = threadIdx.x & 63;
  const uint32_t gh = lane / LPR, sl = lane % LPR;  // row group; the lane's sources 2 sl, 2 sl + 1
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lane16 = sl * 16;
  uint4* list = lists[w];
  unsigned long long* best = bests[w];
  const uint32_t x = blockIdx.x & 7;
  const uint32_t nwc = (n + NPW - 1) / NPW;
  const uint32_t n_act = alist[0];
  const uint32_t nbx = n_act > x ? (n_act - x + 7) / 8 : 0;
  // nseg > 1 (dense graphs): an item is one of nseg segments of a node chunk's
  // in-arcs, so a chunk's thousands of arcs are relaxed by nseg waves at once;
  // the segments' waves share rows and merge by 64-bit atomic min (the packed
  // key's order is the PathProperties order)
  const uint32_t items = nbx * nwc * nseg;
  const uint32_t stride = (gridDim.x >> 3) * WAVES;
  uint32_t n_rel = 0, flagged = ~0u;
  for (uint32_t it = (blockIdx.x >> 3) * WAVES + w; it < items; it += stride) {
    const uint32_t b = alist[1 + x + 8 * (it / (nwc * nseg))];
    const uint32_t ci = it % (nwc * nseg);
    const uint32_t vw = (ci / nseg) * NPW, seg = ci % nseg;
    const uint32_t vw1 = min(vw + NPW, n);
    uint64_t* Db = D + (size_t)b * n * B;
    const uint32_t* St = stamp + (size_t)b * n;
    const __amdgpu_buffer_rsrc_t slab = __builtin_amdgcn_make_buffer_rsrc(Db, 0, (int)(n * B * 8u), 0x00020000);
    uint32_t a0 = in_off[vw], a1 = in_off[vw1];
    if (nseg > 1) {
      const uint32_t per = (a1 - a0 + nseg - 1) / nseg;
      a0 = min(a1, a0 + seg * per);
      a1 = min(a1, a0 + per);
    }
    uint32_t n_cand = 0;
    uint32_t run_slot = 0;
    uint64_t run0 = KEY_INF, run1 = KEY_INF;
    bool prefetched = false;
    uint64_t cur0[NPW / G], cur1[NPW / G];
    for (uint32_t c0 = a0; c0 < a1; c0 += STG_W) {
      const uint32_t c1 = min(c0 + STG_W, a1);
      uint4 ra[K];
      bool dirty[K];
#pragma unroll
      for (int i = 0; i < K; i++) ra[i] = in_rec[min(c0 + lane + 64 * i, c1 - 1)];
#pragma unroll
      for (int i = 0; i < K; i++) dirty[i] = c0 + lane + 64 * i < c1 && (!FRONT || St[ra[i].x] > pass);
      uint32_t cnt = 0;
#pragma unroll
      for (int i = 0; i < K; i++) {
        const uint64_t m = __ballot(dirty[i]);
        if (dirty[i])
          list[cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1))] =
              make_uint4(ra[i].x * (B * 8), ra[i].y - vw, ra[i].z, ra[i].w);
        cnt += (uint32_t)__popcll(m);
      }
      if (cnt && !n_cand) {
#pragma unroll
        for (int i = 0; i < NPW * B / 64; i++) best[i * 64 + lane] = KEY_INF;
      }
      n_cand += cnt;
      if (cnt >= PREFETCH_MIN && !prefetched) {
        prefetched = true;
#pragma unroll
        for (int i = 0; i < NPW / G; i++)
          load_key2(slab, min(vw + i * G + gh, vw1 - 1) * (B * 8) + lane16, cur0[i], cur1[i]);
      }
      // half-wave gh takes records gh, gh + 2, ...: each destination's candidates
      // form one run per half-wave (CSC order)
      auto fold = [&](const uint4& r, uint64_t k0, uint64_t k1) {
        if (r.y != run_slot) {
          atomicMin(&best[run_slot * B + 2 * sl], (unsigned long long)run0);
          atomicMin(&best[run_slot * B + 2 * sl + 1], (unsigned long long)run1);
          run_slot = r.y;
          run0 = run1 = KEY_INF;
        }
        const float om = __uint_as_float(r.w);
        run0 = min(run0, relax32(k0, r.z, om));
        run1 = min(run1, relax32(k1, r.z, om));
      };
      uint32_t g = 0;
      for (; g + GROUP * G <= cnt; g += GROUP * G) {
        uint4 r[GROUP];
        uint64_t k0[GROUP], k1[GROUP];
#pragma unroll
        for (int j = 0; j < GROUP; j++) r[j] = list[g + j * G + gh];
#pragma unroll
        for (int j = 0; j < GROUP; j++) load_key2(slab, r[j].x + lane16, k0[j], k1[j]);
#pragma unroll
        for (int j = 0; j < GROUP; j++) fold(r[j], k0[j], k1[j]);
      }
      for (; g < cnt; g += G) {
        const uint32_t idx = g + gh;
        if (idx < cnt) {
          const uint4 r = list[idx];
          uint64_t k0, k1;
          load_key2(slab, r.x + lane16, k0, k1);
          fold(r, k0, k1);
        }
      }
    }
    if (COUNT) n_rel += n_cand;
    if (!n_cand) continue;
    atomicMin(&best[run_slot * B + 2 * sl], (unsigned long long)run0);
    atomicMin(&best[run_slot * B + 2 * sl + 1], (unsigned long long)run1);
    uint64_t nb0[NPW / G], nb1[NPW / G];
#pragma unroll
    for (int i = 0; i < NPW / G; i++) {
      nb0[i] = best[(i * G + gh) * B + 2 * sl];
      nb1[i] = best[(i * G + gh) * B + 2 * sl + 1];
    }
    if (!prefetched) {
#pragma unroll
      for (int i = 0; i < NPW / G; i++)
        load_key2(slab,
                  nb0[i] != KEY_INF || nb1[i] != KEY_INF ? min(vw + i * G + gh, vw1 - 1) * (B * 8) + lane16 : OOB,
                  cur0[i], cur1[i]);
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < NPW / G; i++) {
      const uint32_t v = vw + i * G + gh;
      bool c0 = v < vw1 && nb0[i] < cur0[i];
      bool c1 = v < vw1 && nb1[i] < cur1[i];
      if (nseg > 1) {  // other segments' waves write this row too
        unsigned long long* k = (unsigned long long*)&Db[(size_t)v * B + 2 * sl];
        if (c0) c0 = nb0[i] < atomicMin(k, (unsigned long long)nb0[i]);
        if (c1) c1 = nb1[i] < atomicMin(k + 1, (unsigned long long)nb1[i]);
      } else if (c0 || c1) {
        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
        *(u64x2*)&Db[(size_t)v * B + 2 * sl] = (u64x2){c0 ? nb0[i] : cur0[i], c1 ? nb1[i] : cur1[i]};
      }
      const uint64_t m = __ballot(c0 || c1);
      if (m) {
        any = true;
        if (FRONT && sl == 0 && ((m >> (gh * LPR)) & ROW_MASK)) stamp[(size_t)b * n + v] = pass + 2;
      }
    }
    if (any && b != flagged) {
      if (lane == 0) changed[b * FLAG_STRIDE] = 1u;
      flagged = b;
    }
  }
  if (COUNT && lane == 0 && n_rel) atomicAdd(&work[blockIdx.x & (WORK_SHARDS - 1)], (unsigned long long)n_rel * B);
}

// Transposed write-out of [B rows x 64 cols] tiles.  Diagonal = the raw
// self-loop (graph/mod.rs:210-217).  Saturated keys flag their batch.
// VEC: 16-B stores (two latencies / four losses per lane); needs n_used % 4 == 0
// so every row starts 16-B aligned.
__device__ __forceinline__ void out_entry(uint64_t kk, uint32_t row, uint32_t j, const uint32_t* __restrict__ used,
                                          const uint32_t* __restrict__ self_edge, const uint64_t* __restrict__ e_lat,
                                          const float* __restrict__ e_loss, uint64_t& lat, float& loss, bool& sflag) {
  if (row == j) {
    const uint32_t e = self_edge[used[j]];
    lat = e_lat[e];
    loss = e_loss[e];
  } else {
    const uint32_t l = key_lat(kk);
    sflag |= l == LAT32_SAT;
    lat = l;
    loss = __uint_as_float(key_loss_bits(kk));
  }
}

// TPB column tiles per block: the global loads of tile t + 1 are issued into
// registers before tile t is written out, so a block's reads and writes overlap.
template <int B, bool VEC, int TPB>
__global__ void __launch_bounds__(256)
    k_out_batch(const uint64_t* __restrict__ D, uint32_t n, const uint32_t* __restrict__ used, uint32_t n_used,
                uint32_t first_row, uint32_t row_end, uint32_t out_row0, const uint32_t* __restrict__ self_edge,
                const uint64_t* __restrict__ e_lat, const float* __restrict__ e_loss,
                uint64_t* __restrict__ out_lat, float* __restrict__ out_loss, uint32_t* __restrict__ sat) {
  constexpr int G = 64 / B;
  constexpr int CPW = 64 / (4 * G);  // tile columns (nodes) each lane loads
  __shared__ uint64_t tile[64][B + 1];
  const uint32_t b = blockIdx.y;
  const uint64_t* __restrict__ Db = D + (size_t)b * n * B;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gh = lane / B, sl = lane % B;
  uint64_t pre[CPW];
  auto load_tile = [&](uint32_t j0) {
    uint32_t node[CPW];
#pragma unroll
    for (int k = 0; k < CPW; k++) {
      const uint32_t j = j0 + wave * G + gh + k * 4 * G;
      node[k] = j < n_used ? used[j] : ~0u;
    }
#pragma unroll
    for (int k = 0; k < CPW; k++) pre[k] = node[k] != ~0u ? Db[(size_t)node[k] * B + sl] : 0ull;
  };
  bool sflag = false;
  const uint32_t rbase = first_row + b * B;
  const uint32_t jb = blockIdx.x * TPB * 64;
  load_tile(jb);
  for (int t = 0; t < TPB; t++) {
    const uint32_t j0 = jb + t * 64;
    if (j0 >= n_used) break;
    if (t) __syncthreads();  // the previous tile's write-out has read the LDS tile
#pragma unroll
    for (int k = 0; k < CPW; k++) tile[wave * G + gh + k * 4 * G][sl] = pre[k];
    __syncthreads();
    if (t + 1 < TPB && j0 + 64 < n_used) load_tile(j0 + 64);
    if (VEC && j0 + 64 <= n_used) {
      // lane = (row quarter, 4 columns): each key is read from LDS once, and the
      // lane stores 32 B of latencies and 16 B of losses
      for (int r = wave * 4 + (lane >> 4); r < B; r += 16) {
        const uint32_t row = rbase + r;
        if (row >= row_end) continue;
        const uint32_t c = (lane & 15) * 4;
        uint64_t l0, l1, l2, l3;
        float4 f;
        out_entry(tile[c][r], row, j0 + c, used, self_edge, e_lat, e_loss, l0, f.x, sflag);
        out_entry(tile[c + 1][r], row, j0 + c + 1, used, self_edge, e_lat, e_loss, l1, f.y, sflag);
        out_entry(tile[c + 2][r], row, j0 + c + 2, used, self_edge, e_lat, e_loss, l2, f.z, sflag);
        out_entry(tile[c + 3][r], row, j0 + c + 3, used, self_edge, e_lat, e_loss, l3, f.w, sflag);
        const size_t o = (size_t)(row - out_row0) * n_used + j0 + c;
        // write-once streaming output (1.2 GB at 10k): nontemporal 16-B stores
        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store((u64x2){l0, l1}, (u64x2*)&out_lat[o]);
        __builtin_nontemporal_store((u64x2){l2, l3}, (u64x2*)&out_lat[o + 2]);
        __builtin_nontemporal_store((f32x4){f.x, f.y, f.z, f.w}, (f32x4*)&out_loss[o]);
      }
    } else {
      const uint32_t j = j0 + lane;
      for (int r = wave; r < B; r += 4) {
        const uint32_t row = rbase + r;
        if (row >= row_end || j >= n_used) continue;
        const size_t o = (size_t)(row - out_row0) * n_used + j;
        uint64_t l;
        float f;
        out_entry(tile[lane][r], row, j, used, self_edge, e_lat, e_loss, l, f, sflag);
        out_lat[o] = l;
        out_loss[o] = f;
      }
    }
  }
  if (__any(sflag) && lane == 0) atomicOr(&sat[b], 1u);
}

// ---------------------------------------------------------------------------
// Wide fallback: u64 latency + f32 loss, Jacobi (double-buffered) so a reader
// never sees a torn pair.  UINT64_MAX latency = no path yet.
// ---------------------------------------------------------------------------
__global__ void k_init_wide(uint64_t* __restrict__ L, float* __restrict__ F, uint32_t n,
                            const uint32_t* __restrict__ used, const uint32_t* __restrict__ rows,
                            uint32_t n_rows_total, uint32_t n_batches) {
  size_t total = (size_t)n_batches * n * BATCH;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    uint32_t lane = (uint32_t)(i & (BATCH - 1));
    size_t bv = i / BATCH;
    uint32_t v = (uint32_t)(bv % n);
    uint32_t b = (uint32_t)(bv / n);
    uint32_t slot = b * BATCH + lane;
    bool src = slot < n_rows_total && used[rows[slot]] == v;
    L[i] = src ? 0ull : ~0ull;
    F[i] = 0.0f;
  }
}

__global__ void __launch_bounds__(RELAX_BLOCK)
    k_relax_wide(const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ in_src,
                 const uint64_t* __restrict__ in_lat, const float* __restrict__ in_om,
                 const uint64_t* __restrict__ Lc, const float* __restrict__ Fc,
                 uint64_t* __restrict__ Ln, float* __restrict__ Fn, uint32_t n,
                 uint32_t* __restrict__ changed) {
  const uint32_t b = blockIdx.y;
  const size_t base = (size_t)b * n * BATCH;
  const int lane = threadIdx.x & 63;
  const uint32_t v = __builtin_amdgcn_readfirstlane(blockIdx.x * RELAX_WAVES + (threadIdx.x >> 6));
  if (v >= n) return;
  uint64_t bl = Lc[base + (size_t)v * BATCH + lane];
  float bf = Fc[base + (size_t)v * BATCH + lane];
  const uint64_t l_in = bl;
  const float f_in = bf;
  for (uint32_t a = in_off[v]; a < in_off[v + 1]; a++) {
    uint32_t u = in_src[a];
    uint64_t lu = Lc[base + (size_t)u * BATCH + lane];
    if (lu == ~0ull) continue;
    float fu = Fc[base + (size_t)u * BATCH + lane];
    uint64_t cl = lu + in_lat[a];
    float cf = fold_loss(fu, in_om[a]);
    if (cl < bl || (cl == bl && cf < bf)) {
      bl = cl;
      bf = cf;
    }
  }
  Ln[base + (size_t)v * BATCH + lane] = bl;
  Fn[base + (size_t)v * BATCH + lane] = bf;
  bool ch = bl != l_in || __float_as_uint(bf) != __float_as_uint(f_in);
  if (__any(ch) && lane == 0) *changed = 1u;  // plain store: the line stays in L2
}

__global__ void k_out_wide(const uint64_t* __restrict__ L, const float* __restrict__ F, uint32_t n,
                           const uint32_t* __restrict__ used, uint32_t n_used,
                           const uint32_t* __restrict__ rows, uint32_t n_rows_total, uint32_t out_row0,
                           const uint32_t* __restrict__ self_edge, const uint64_t* __restrict__ e_lat,
                           const float* __restrict__ e_loss, uint64_t* __restrict__ out_lat,
                           float* __restrict__ out_loss, unsigned long long* __restrict__ first_unreach) {
  const uint32_t slot = blockIdx.y * BATCH + (threadIdx.x & 63);
  if (slot >= n_rows_total) return;
  const uint32_t row = rows[slot];
  const size_t base = (size_t)blockIdx.y * n * BATCH + (threadIdx.x & 63);
  for (uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < n_used; j += gridDim.x * 4) {
    size_t o = (size_t)(row - out_row0) * n_used + j;
    if (row == j) {
      uint32_t e = self_edge[used[j]];
      out_lat[o] = e_lat[e];
      out_loss[o] = e_loss[e];
      continue;
    }
    uint64_t l = L[base + (size_t)used[j] * BATCH];
    out_lat[o] = l;
    out_loss[o] = F[base + (size_t)used[j] * BATCH];
    if (l == ~0ull) atomicMin(first_unreach, (unsigned long long)row * n_used + j);
  }
}

// Wide recomputation of the listed rows (absolute row indices).
void run_wide(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, const std::vector<uint32_t>& rows,
              uint32_t out_row0, uint64_t* out_lat, float* out_loss) {
  ensure_csc(ctx, net);
  hipStream_t st = ctx->stream;
  const uint32_t n = net->n_nodes;
  const uint32_t nr = (uint32_t)rows.size();
  const uint32_t nb = (nr + BATCH - 1) / BATCH;
  uint32_t* d_rows = ctx->r_misc.get<uint32_t>(nr);
  SG_HIP(hipMemcpyAsync(d_rows, rows.data(), nr * 4ull, hipMemcpyHostToDevice, st));
  size_t slab = (size_t)nb * n * BATCH;
  char* buf = ctx->r_dist2.get<char>(slab * 24);
  uint64_t* L0 = (uint64_t*)buf;
  uint64_t* L1 = L0 + slab;
  float* F0 = (float*)(L1 + slab);
  float* F1 = F0 + slab;
  hipLaunchKernelGGL(k_init_wide, dim3(grid_for(slab, 256, 65536)), dim3(256), 0, st, L0, F0, n,
                     d_used, d_rows, nr, nb);
  uint32_t* changed = ctx->r_flags.get<uint32_t>(4);
  for (uint32_t pass = 0;; pass++) {
    if (pass > n + 2) throw Error(SG_ERR_DEVICE, "wide relaxation did not converge");
    SG_HIP(hipMemsetAsync(changed, 0, 4, st));
    TimedLaunch tl(ctx, "relax_wide", (double)nb * BATCH * net->n_arcs);
    hipLaunchKernelGGL(k_relax_wide, dim3((n + RELAX_WAVES - 1) / RELAX_WAVES, nb), dim3(RELAX_BLOCK),
                       0, st, net->in_off, net->in_src, net->in_lat, net->in_om, L0, F0, L1, F1, n,
                       changed);
    SG_CHECK_LAUNCH();
    std::swap(L0, L1);
    std::swap(F0, F1);
    uint32_t h = 0;
    copy_to_host(ctx, &h, changed, 4);
    if (!h) break;
  }
  unsigned long long* first = ctx->r_err.get<unsigned long long>(4);
  SG_HIP(hipMemsetAsync(first, 0xff, 8, st));
  hipLaunchKernelGGL(k_out_wide, dim3(grid_for(n_used, 4, 1024), nb), dim3(256), 0, st, L0, F0, n,
                     d_used, n_used, d_rows, nr, out_row0, net->self_edge, net->e_lat, net->e_loss,
                     out_lat, out_loss, first);
  SG_CHECK_LAUNCH();
  unsigned long long h = 0;
  copy_to_host(ctx, &h, first, 8);
  if (h != ~0ull) {
    uint32_t i = (uint32_t)(h / n_used), j = (uint32_t)(h % n_used);
    throw Error(SG_ERR_UNREACHABLE, "no path from node index " + std::to_string(i) + " to " +
                                        std::to_string(j) + " (graph must be connected)",
                i, j);
  }
}

// The slab search's knobs, read once per search (shortest_paths_slab).  The first six pick
// the kernel instantiation (the SG_SP / SG_SP2 tables); their defaults are the fastest
// measured configuration of each kernel (tools/apsp_variants.py).
struct SlabKnobs {
  bool front;          // SG_APSP_FRONTIER (=0 relaxes every arc every pass)
  int bsz;             // SG_APSP_B: sources per batch (32 | 64)
  int spl;             // SG_APSP_SPL: sources per lane, 2 = k_relax_w2 (the default)
  int npw, stg, gr;    // SG_APSP_NPW nodes per wave item, SG_APSP_STAGE arcs staged per wave step,
                       // SG_APSP_GROUP row reads in flight
  size_t group_bytes;  // SG_APSP_GROUP_MB: device memory of the batches whose slabs are live together
  uint32_t chunk;      // SG_APSP_PASS_CHUNK: passes issued per host read of the convergence flags
  uint32_t nseg;       // SG_APSP_SEG: in-arc segments per relaxation item (k_relax_w2)
  int out_tpb;         // SG_APSP_OUT_TPB: column tiles per write-out block: 1 | 2 | 4 (1 measured best)
  bool trace;          // SG_APSP_TRACE: per-pass diagnostics on stderr
};
static SlabKnobs slab_knobs(const sg_net* net) {
  SlabKnobs k;
  k.front = knob_int("SG_APSP_FRONTIER", 1) != 0;
  // dense graphs (more than ~600 in-arcs per node: C2's complete graph) relax
  // faster in 32-source batches with arc segments (3.49 vs 3.66 ms at C2)
  const bool dense = net->n_nodes && (double)net->n_arcs / net->n_nodes > 600.0;
  k.bsz = knob_int("SG_APSP_B", dense ? 32 : 64);
  k.spl = knob_int("SG_APSP_SPL", 2);
  k.npw = knob_int("SG_APSP_NPW", k.spl == 2 ? 4 : 8);
  k.stg = knob_int("SG_APSP_STAGE", k.spl == 2 ? 64 : 128);
  k.gr = knob_int("SG_APSP_GROUP", k.spl == 2 ? 3 : 8);
  k.group_bytes = (size_t)knob_int("SG_APSP_GROUP_MB", 4096) << 20;
  k.chunk = (uint32_t)std::max(1, knob_int("SG_APSP_PASS_CHUNK", 4));
  // one segment per ~SEG_ARCS arcs of a node chunk, so dense graphs (C2: ~4800 arcs per
  // chunk) fill the chip
  constexpr uint32_t SEG_ARCS = 1200;  // C2 (1,200-node complete graph): 4 segments, measured best (of 1-16)
  const double chunk_arcs = net->n_nodes ? (double)net->n_arcs * k.npw / net->n_nodes : 0.0;
  k.nseg = k.spl == 2 ? (uint32_t)knob_int("SG_APSP_SEG", (int)std::lround(chunk_arcs / SEG_ARCS), 1, 16) : 1u;
  const int tpb = knob_int("SG_APSP_OUT_TPB", 1);
  k.out_tpb = tpb == 4 ? 4 : tpb == 2 ? 2 : 1;
  k.trace = knob_int("SG_APSP_TRACE", 0) != 0;
  return k;
}

// B sources per batch, NPW destination nodes per wave item, STG arcs staged per
// wave step, FRONT = stamp frontier.
template <int B, int NPW, int STG, int GR, bool FRONT, int SPL = 1>
static void shortest_paths_t(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, uint32_t row_begin,
                             uint32_t row_end, uint64_t* out_lat, float* out_loss, const SlabKnobs& knobs) {
  ensure_csc(ctx, net);  // the slab kernel gathers in-arcs
  hipStream_t st = ctx->stream;
  const uint32_t n = net->n_nodes;
  const uint32_t n_rows = row_end - row_begin;
  const uint32_t n_batches = (n_rows + B - 1) / B;
  // slab byte offsets are 32-bit (buffer descriptors; OOB = 0x80000000)
  if ((uint64_t)n * B * 8 >= 0x80000000ull)
    throw Error(SG_ERR_INVALID_ARG, "graph too large for the slab kernel's 32-bit slab offsets (" +
                                        std::to_string(n) + " nodes)");
  // Group: batches whose slabs are live together (bounded device memory).
  const size_t slab_bytes = (size_t)n * B * 8;
  const size_t budget = knobs.group_bytes;
  const uint32_t group = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_batches, budget / slab_bytes));
  uint64_t* D = ctx->r_dist.get<uint64_t>((size_t)group * n * B);
  uint32_t* stamp = ctx->r_dirty.get<uint32_t>((size_t)group * n);
  // per-batch flags: a 3-slot ring of "changed in pass p" arrays, the
  // saturation flags, the active-batch list
  const size_t fs = (size_t)group * FLAG_STRIDE;
  uint32_t* flags = ctx->r_flags.get<uint32_t>(fs * 3 + 2 * (size_t)group + 8);
  uint32_t* ring[3] = {flags, flags + fs, flags + 2 * fs};
  uint32_t* sat = flags + 3 * fs;
  uint32_t* alist = sat + group;
  unsigned long long* work = ctx->count_work ? ctx->r_work.get<unsigned long long>(WORK_SHARDS) : nullptr;
  if (work) SG_HIP(hipMemsetAsync(work, 0, WORK_SHARDS * 8, st));
  // Passes are issued in chunks; the host reads the convergence flags once per
  // chunk.  A pass issued after its batch converged finds it off the active list.
  const uint32_t chunk = knobs.chunk;
  const bool trace = knobs.trace;
  const uint32_t nseg = knobs.nseg;
  const int out_tpb = knobs.out_tpb;
  std::vector<uint32_t> h_sat(group);
  std::vector<uint32_t> wide_rows;
  for (uint32_t g0 = 0; g0 < n_batches; g0 += group) {
    const uint32_t gb = std::min(group, n_batches - g0);
    const uint32_t first_row = row_begin + g0 * B;
    hipLaunchKernelGGL(k_init_batch<B>, dim3(grid_for((size_t)gb * n * (B / 2), 256, 8192)), dim3(256), 0, st, D,
                       stamp, n, gb);
    hipLaunchKernelGGL(k_stamp_sources<B>, dim3(grid_for((size_t)gb * B, 256)), dim3(256), 0, st, D, stamp, n,
                       d_used, first_row, row_end, gb);
    SG_CHECK_LAUNCH();
    SG_HIP(hipMemsetAsync(ring[2], 1, gb * FLAG_STRIDE * 4ull, st));  // "changed in pass -1": every batch active
    // one wave per work item (active batch, NPW-node chunk); 4 waves per block,
    // a multiple of 8 blocks (XCD mapping)
    const uint32_t ncw = (n + 4 * NPW - 1) / (4 * NPW);
    // Sized for the active batches the host last saw (every batch at first; a
    // converged batch never becomes active again, so it is an upper bound for
    // the chunk): a tail pass with few active batches launches few blocks.
    uint32_t n_act_seen = gb;
    hipEvent_t te0 = nullptr, te1 = nullptr;
    if (trace) {
      SG_HIP(hipEventCreate(&te0));
      SG_HIP(hipEventCreate(&te1));
    }
    double trace_prev = 0;
    // the active list of pass p (from the flags of pass p - 1) is built by the
    // pass before it, or at a chunk end, where its count also goes to the host
    hipLaunchKernelGGL(k_active_list, dim3(1), dim3(1024), 0, st, ring[2], gb, alist, ring[0], nullptr);
    for (uint32_t pass = 0;;) {
      const uint32_t grid = 8 * ncw * ((n_act_seen + 7) / 8);
      for (uint32_t c = 0; c < chunk; c++, pass++) {
        if (pass > n + 2 + chunk) throw Error(SG_ERR_DEVICE, "relaxation did not converge");
        if (trace) SG_HIP(hipEventRecord(te0, st));
        uint32_t* changed = ring[pass % 3];
        if (c > 0)
          hipLaunchKernelGGL(k_active_list, dim3(1), dim3(1024), 0, st, ring[(pass + 2) % 3], gb, alist, changed,
                             nullptr);
        {
          TimedLaunch tl(ctx, "relax", 0.0);
          if constexpr (SPL == 2) {
            if (work)
              hipLaunchKernelGGL((k_relax_w2<B, NPW, STG / 64, GR, FRONT, true>), dim3(grid * nseg),
                                 dim3(RELAX_THREADS), 0, st, net->in_off, net->in_rec, D, n, alist, changed, stamp,
                                 pass, work, nseg);
            else
              hipLaunchKernelGGL((k_relax_w2<B, NPW, STG / 64, GR, FRONT, false>), dim3(grid * nseg),
                                 dim3(RELAX_THREADS), 0, st, net->in_off, net->in_rec, D, n, alist, changed, stamp,
                                 pass, work, nseg);
          } else {
            if (work)
              hipLaunchKernelGGL((k_relax_w<B, NPW, STG / 64, GR, FRONT, true>), dim3(grid), dim3(RELAX_THREADS), 0,
                                 st, net->in_off, net->in_rec, D, n, alist, changed, stamp, pass, work);
            else
              hipLaunchKernelGGL((k_relax_w<B, NPW, STG / 64, GR, FRONT, false>), dim3(grid), dim3(RELAX_THREADS), 0,
                                 st, net->in_off, net->in_rec, D, n, alist, changed, stamp, pass, work);
          }
        }
        SG_CHECK_LAUNCH();
        if (trace) {
          SG_HIP(hipEventRecord(te1, st));
          SG_HIP(hipEventSynchronize(te1));
          float ms = 0;
          SG_HIP(hipEventElapsedTime(&ms, te0, te1));
          unsigned long long w[WORK_SHARDS] = {};
          if (work) copy_to_host(ctx, w, work, sizeof(w));
          double tot = 0;
          for (int k = 0; k < WORK_SHARDS; k++) tot += (double)w[k];
          uint32_t na = 0;
          copy_to_host(ctx, &na, alist, 4);
          fprintf(stderr, "[apsp] group %u pass %u: %.3f ms, %u active batches, %.3f G lane-relaxations\n", g0, pass,
                  ms, na, (tot - trace_prev) / 1e9);
          trace_prev = tot;
        }
      }
      // active list of the next pass (= batches changed in the last one), its count to the host
      hipLaunchKernelGGL(k_active_list, dim3(1), dim3(1024), 0, st, ring[(pass + 2) % 3], gb, alist,
                         ring[pass % 3], ctx->apsp_ret);
      SG_CHECK_LAUNCH();
      SG_HIP(hipStreamSynchronize(st));
      n_act_seen = *(volatile uint32_t*)ctx->apsp_ret;
      if (n_act_seen == 0) break;
    }
    if (trace) {
      SG_HIP(hipEventDestroy(te0));
      SG_HIP(hipEventDestroy(te1));
    }
    SG_HIP(hipMemsetAsync(sat, 0, gb * 4ull, st));
    {
      TimedLaunch tl(ctx, "out", 12.0 * std::min<uint32_t>(gb * B, row_end - first_row) * n_used);
      const bool vec = n_used % 4 == 0 && ((uintptr_t)out_lat & 15) == 0 && ((uintptr_t)out_loss & 15) == 0;
      const uint32_t tpb = out_tpb;
      const dim3 og((n_used + 64 * tpb - 1) / (64 * tpb), gb);
#define SG_OUT(V_, T_)                                                                                          \
  hipLaunchKernelGGL((k_out_batch<B, V_, T_>), og, dim3(256), 0, st, D, n, d_used, n_used, first_row, row_end, \
                     row_begin, net->self_edge, net->e_lat, net->e_loss, out_lat, out_loss, sat)
      // (the grid above is sized for tpb: every branch launches TPB = tpb)
      if (vec && tpb == 4) SG_OUT(true, 4);
      else if (vec && tpb == 2) SG_OUT(true, 2);
      else if (vec) SG_OUT(true, 1);
      else if (tpb == 4) SG_OUT(false, 4);
      else if (tpb == 2) SG_OUT(false, 2);
      else SG_OUT(false, 1);
#undef SG_OUT
    }
    SG_CHECK_LAUNCH();
    copy_to_host(ctx, h_sat.data(), sat, gb * 4ull);
    for (uint32_t b = 0; b < gb; b++)
      if (h_sat[b])
        for (uint32_t r = 0; r < B; r++) {
          uint32_t row = first_row + b * B + r;
          if (row < row_end) wide_rows.push_back(row);
        }
  }
  if (work) {  // relaxations actually performed (relaxed arcs x lanes), for the roofline
    unsigned long long w[WORK_SHARDS];
    copy_to_host(ctx, w, work, sizeof(w));
    double total = 0;
    for (int k = 0; k < WORK_SHARDS; k++) total += (double)w[k];
    timer_add_work(ctx, "relax", total);
  }
  if (!wide_rows.empty()) run_wide(ctx, net, d_used, n_used, wide_rows, row_begin, out_lat, out_loss);
}

// The slab search of rows [row_begin, row_end): the instantiation the knobs name.
void shortest_paths_slab(sg_ctx* ctx, sg_net* net, const uint32_t* d_used, uint32_t n_used, uint32_t row_begin,
                         uint32_t row_end, uint64_t* out_lat, float* out_loss) {
  const SlabKnobs k = slab_knobs(net);
#define SG_SP_(B_, NPW_, STG_, GR_, SPL_)                                                                        \
  if (k.bsz == B_ && k.npw == NPW_ && k.stg == STG_ && k.gr == GR_) {                                            \
    if (k.front)                                                                                                 \
      shortest_paths_t<B_, NPW_, STG_, GR_, true, SPL_>(ctx, net, d_used, n_used, row_begin, row_end, out_lat,   \
                                                        out_loss, k);                                            \
    else                                                                                                         \
      shortest_paths_t<B_, NPW_, STG_, GR_, false, SPL_>(ctx, net, d_used, n_used, row_begin, row_end, out_lat,  \
                                                         out_loss, k);                                           \
    return;                                                                                                      \
  }
#define SG_SP2(B_, NPW_, STG_, GR_) SG_SP_(B_, NPW_, STG_, GR_, 2)
#define SG_SP(B_, NPW_, STG_, GR_) SG_SP_(B_, NPW_, STG_, GR_, 1)
  if (k.spl == 2) {
    SG_SP2(64, 8, 128, 8)
    SG_SP2(64, 8, 128, 4)
    SG_SP2(64, 8, 128, 2)
    SG_SP2(64, 8, 128, 6)
    SG_SP2(64, 8, 64, 4)
    SG_SP2(64, 4, 64, 4)
    SG_SP2(64, 4, 128, 4)
    SG_SP2(64, 2, 64, 4)
    SG_SP2(64, 4, 64, 3)
    SG_SP2(64, 4, 64, 5)
    SG_SP2(64, 16, 128, 4)
    SG_SP2(32, 4, 64, 3)
    SG_SP2(32, 4, 64, 2)
    SG_SP2(32, 8, 64, 3)
    SG_SP2(32, 8, 128, 3)
    SG_SP2(32, 4, 128, 3)
    throw Error(SG_ERR_INVALID_ARG, "unsupported SG_APSP_SPL=2 configuration");
  }
  SG_SP(64, 8, 128, 8)
  SG_SP(64, 8, 128, 16)
  SG_SP(64, 16, 128, 8)
  SG_SP(64, 4, 64, 8)
  SG_SP(32, 8, 128, 8)
  SG_SP(32, 16, 128, 8)
#undef SG_SP
#undef SG_SP2
#undef SG_SP_
  throw Error(SG_ERR_INVALID_ARG, "unsupported SG_APSP_B / SG_APSP_NPW / SG_APSP_STAGE / SG_APSP_GROUP");
}

}  // namespace sg
