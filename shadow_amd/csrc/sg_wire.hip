// sg_wire.hip -- every host's in-flight Packet events, resident on the device.
//
// The reference keeps one EventQueue per host (core/work/event_queue.rs); a
// delivered packet enters its destination's queue in
// WorkerShared::push_packet_to_host (worker.rs:597-607) and leaves it when
// Host::execute(until) pops every event with time < until (host.rs:753-757), in
// the order of event.rs:84-155: (time, Packet < Local, src_host_id,
// src_host_event_id).  sg_wire is those queues restricted to Packet events: a
// delivery round's buckets go in (sg_wire_push), a window's arrivals come out
// grouped by host in that order (sg_wire_pop), ready for sg_inbound_run_ordered.
//
// The key (host, time, src_host, event_id) is unique (a source's event ids are,
// host.rs:649-653), so what a pop returns is a function of the SET of events
// held: the order records were appended in never shows.  That frees the store
// from keeping any order at all until a record leaves:
//
//   record   32 B: time, event id, src host, dst host, packet, len
//   arena    chunks of WR_CHUNK records handed out from a free list
//   rows     n_bins ring rows + 2 far rows, each an append-only list of records:
//            a count and a table of the chunks holding slots [0, count)
//   calendar bin = time / bin_ns; bins [base, hz) live in ring row bin & mask,
//            later ones in the live far row, earlier ones clamp to bin `base`
//
// A push appends (count, allocate chunks, scatter: three launches over the batch).
// A pop scans only the rows whose bins end at or before window_end, plus the one
// row that straddles it: rows wholly due hand their chunks back; in the
// straddling row a record that leaves is overwritten with a tombstone (time =
// UINT64_MAX, which no event carries: EMUTIME_MAX = UINT64_MAX - 1,
// emulated_time.rs:30) and the row goes whole when the window has passed it; a
// row that straddles for long (bin_ns far above a round) is compacted in place
// whenever its tombstones reach an eighth of its live records.
// The due records are bucketed by destination (counts, scan, scatter into a
// staging array) and each host's segment is sorted by (time, src_host, event_id)
// -- the real event id: events of different rounds meet here, so the rank a
// packet had inside its own round (sg_deliver.hip's bucket key) says nothing.
// No grid and no loop below depends on the number of events held: only on the
// batch, the records of the scanned rows, n_hosts and n_bins.
//
// The far rows hold what lies past the ring's horizon hz.  When the ring has
// advanced half its length past the last re-binning (or the window reaches hz)
// the live far row is read once: due records leave, the others are appended
// again under the new (base, hz), to ring rows or to the other far row.
//
//   push: k_wire_count, k_wire_alloc, k_wire_scatter
//         from a delivery round's buckets (sg_wire_push), or on an owner rank of the sharded
//         path from the records it received (sg_wire_push_records[_padded]): the source rank
//         has written len and the caller's packet id into the two words of the 32-byte
//         sg_record the owner does not need (k_wire_stamp, sg_wire_stamp_records[_padded]), so
//         the exchange moves what it always moved and the append reads one record per event
//         k_wire_stamp (source rank), k_wire_padded_valid (the blocks' record counts, from xall)
//   pop:  k_wire_plan      the rows to scan, the new base / horizon
//         k_wire_popcount  due records per destination host (and the far records' new rows)
//         (scan)           host offsets
//         k_wire_commit    the verdict: fits out->cap, arena has room -- nothing moved before it
//         k_wire_move<0>   ring rows: due records -> staging by host, tombstones
//         k_wire_mid       frees the drained rows, advances base / hz, allocates for the far records
//         k_wire_move<1>   far row (when re-binning): due -> staging, the rest appended again
//         k_wire_final     frees the old far row, next_time, the result block
//         k_wire_sort_small / k_wire_sort_lds / k_wire_merge   the three sort tiers
//         k_wire_compact_list / _move / _finish   after the pop, when the straddling row needs it
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "sg_device.h"
#include "sg_internal.h"

namespace sg {
namespace {

constexpr uint32_t WR_CHUNK = 1024;      // records per arena chunk (32 KB)
constexpr uint32_t WR_MAX_BINS = 1024;   // ring rows at most (the per-row LDS histograms: 16 KB)
constexpr uint32_t WR_ROWS = WR_MAX_BINS + 2;
constexpr uint32_t WR_RANK_SORT_MAX = 64;   // a segment up to one wave: rank sort in registers
constexpr uint32_t WR_LDS_SORT_MAX = 2048;  // up to one workgroup's LDS (24-B keys: 48 KB): bitonic sort
constexpr int WR_THREADS = 256;
constexpr int WR_ITEMS = 8;             // records per thread and step of the append
constexpr uint64_t WR_TOMB = ~0ull;      // time of a record that has left its row
constexpr uint32_t WR_DEAD_SHARE = 8;    // a row is compacted when its tombstones reach live / 8 (and a chunk)
constexpr uint64_t WR_CAP_MAX = 1ull << 31;
constexpr uint32_t WR_MAX_RANKS = 64;    // ranks of a fixed-split exchange at most (sg_deliver.hip's MAX_RANKS)

// A stamped record travels as an sg_record: through every sg_comm_* exchange and
// sg_deliver_pad_to_compact unchanged.
static_assert(sizeof(sg_wire_record) == sizeof(sg_record) && sizeof(sg_record) == 32, "sg_wire_record");
static_assert(offsetof(sg_wire_record, deliver_time_ns) == offsetof(sg_record, deliver_time_ns) &&
                  offsetof(sg_wire_record, len) == offsetof(sg_record, order_key) &&
                  offsetof(sg_wire_record, src_host) == offsetof(sg_record, order_key) + 4 &&
                  offsetof(sg_wire_record, event_id) == offsetof(sg_record, event_id) &&
                  offsetof(sg_wire_record, packet_id) == offsetof(sg_record, packet) &&
                  offsetof(sg_wire_record, dst_host) == offsetof(sg_record, dst_host),
              "sg_wire_record is a second reading of sg_record");

// WireCtl::err (sticky).  WE_BADDST: a pushed record named a destination outside the hosts
enum : uint32_t { WE_ARENA = 1, WE_CORRUPT = 2, WE_BADDST = 4 };
enum : uint32_t { WV_OK = 0, WV_CAP = 1, WV_ERR = 2, WV_ARENA = 3 };  // WirePlan::verdict

struct WireCtl {
  unsigned long long base, hz;  // ring bins [base, hz), hz - base <= n_bins
  unsigned long long held;      // events in the store
  unsigned long long pushed;    // events appended by pushes since the last pop reported them
  uint32_t far;                 // the live far row (n_bins or n_bins + 1)
  uint32_t nfree;               // chunks on the free list
  uint32_t err;                 // WE_*: a push found no room; the store is no longer whole
  // Set while a push's count pass runs, by records with no host here; k_wire_alloc, alone on the
  // device, moves it into err: err itself never changes under a kernel that branches on it.
  uint32_t bad;
};

struct WirePlan {
  unsigned long long W, newbase, newhz;
  uint32_t n_ring;   // ring entries; entry n_ring is the far row when rebin
  uint32_t rebin, newfar, verdict;
  uint32_t due;      // records with time < W in the scanned rows
  uint32_t n_work;   // sort work-list entries
  uint32_t ent_row[WR_ROWS];
  uint32_t ent_kind[WR_ROWS];     // 0 wholly due (drained), 1 straddles W, 2 far
  uint32_t ent_off[WR_ROWS + 1];  // slot offsets of the entries (exclusive scan of the rows' counts)
};

struct WireRet {  // pinned, written by k_wire_final
  uint32_t verdict, due;
  unsigned long long next, held, pushed;
  // the straddling row, when its tombstones have reached an eighth of its live records (and a
  // chunk): compact it (row = ~0u: nothing to do); its slots in use and its live records
  uint32_t compact_row, compact_cnt, compact_keep;
  uint32_t err;  // WireCtl::err
};

struct WireDev {
  WireCtl* ctl;
  uint32_t *cnt, *add, *cur;    // per row: slots used, appends counted for the next allocation, scatter cursor
  uint32_t* dead;               // per row: tombstones among its slots
  unsigned long long* rmin;     // per row: smallest time appended since the row was last reset / filtered
  uint32_t* tbl;                // R x M: chunk of each CHUNK slots of a row
  uint32_t* freel;              // M
  uint4* arena;                 // M x CHUNK x 2
  unsigned long long bin_ns;
  uint32_t n_bins, mask, R, M;
};

struct Rec {
  unsigned long long time, eid;
  uint32_t src, dst, packet, len;
};

__device__ __forceinline__ Rec rec_load(const uint4* p, size_t i) {
  const uint4 a = p[2 * i], b = p[2 * i + 1];
  Rec r;
  r.time = ((unsigned long long)a.y << 32) | a.x;
  r.eid = ((unsigned long long)a.w << 32) | a.z;
  r.src = b.x;
  r.dst = b.y;
  r.packet = b.z;
  r.len = b.w;
  return r;
}
__device__ __forceinline__ void rec_store(uint4* p, size_t i, const Rec& r) {
  p[2 * i] = make_uint4((uint32_t)r.time, (uint32_t)(r.time >> 32), (uint32_t)r.eid, (uint32_t)(r.eid >> 32));
  p[2 * i + 1] = make_uint4(r.src, r.dst, r.packet, r.len);
}

// event.rs:84-155 inside one host's queue, Packet events only: time, then source host, then its event id
__device__ __forceinline__ bool key_less(unsigned long long ta, uint32_t sa, unsigned long long ea,
                                         unsigned long long tb, uint32_t sb, unsigned long long eb) {
  if (ta != tb) return ta < tb;
  if (sa != sb) return sa < sb;
  return ea < eb;
}

// The row of an event time under a calendar geometry.  One u64 division; no sum that could overflow.
__device__ __forceinline__ uint32_t wire_row(const WireDev& w, unsigned long long t, unsigned long long base,
                                             unsigned long long hz, uint32_t far) {
  unsigned long long b = t / w.bin_ns;
  if (b < base) b = base;
  if (b >= hz) return far;
  return (uint32_t)b & w.mask;
}

__device__ __forceinline__ size_t wire_slot(const WireDev& w, uint32_t row, uint32_t slot) {
  const uint32_t chunk = w.tbl[(size_t)row * w.M + slot / WR_CHUNK];
  return (size_t)chunk * WR_CHUNK + slot % WR_CHUNK;
}

// Exclusive scan over the block (blockDim.x a multiple of 64, <= 1024); s_w: 17 words.
__device__ __forceinline__ uint32_t wire_block_scan(uint32_t v, uint32_t* s_w, uint32_t* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint32_t inc = wave_incl_sum(v);
  if (lane == 63) s_w[wid] = inc;
  __syncthreads();
  if (wid == 0) {
    const uint32_t s = lane < nw ? s_w[lane] : 0;
    const uint32_t si = wave_incl_sum(s);
    if (lane < nw) s_w[lane] = si - s;
    if (lane == nw - 1) s_w[16] = si;
  }
  __syncthreads();
  const uint32_t r = inc - v + s_w[wid];
  *total = s_w[16];
  __syncthreads();
  return r;
}

__device__ __forceinline__ uint32_t chunks_of(unsigned long long n) {
  return (uint32_t)((n + WR_CHUNK - 1) / WR_CHUNK);
}

// ---- sources of records to append -------------------------------------------
// A delivery round's buckets (sg_deliveries): position i of dst_order names packet p, delivered to
// the host whose [dst_offsets[h], dst_offsets[h + 1]) holds i.
struct SrcDelivery {
  const uint32_t *dst_order, *dst_offsets;
  const unsigned long long *dtime, *eid;
  const uint32_t *src_host, *packet_id, *len;
  uint32_t n_hosts, n_packets, id_base;
  __device__ uint32_t n() const { return min(dst_offsets[n_hosts], n_packets); }
  __device__ bool time(uint32_t i, unsigned long long* t) const {
    const uint32_t p = dst_order[i];
    if (p >= n_packets) return false;
    *t = dtime[p];
    return *t != WR_TOMB;
  }
  __device__ bool load(uint32_t i, Rec* r) const {
    const uint32_t p = dst_order[i];
    if (p >= n_packets) return false;
    r->time = dtime[p];
    if (r->time == WR_TOMB) return false;
    // the first h in [1, n_hosts] with dst_offsets[h] > i; the packet's destination is h - 1
    uint32_t lo = 1, hi = n_hosts;
    for (int it = 0; it < 32 && lo < hi; it++) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (dst_offsets[mid] > i) hi = mid;
      else lo = mid + 1;
    }
    r->dst = lo - 1;
    r->eid = eid[p];
    r->src = src_host[p];
    r->packet = packet_id ? packet_id[p] : id_base + p;
    r->len = len[p];
    return true;
  }
};

// Records already in the store's form (sg_wire_set_state).
struct SrcArray {
  const uint4* recs;
  uint32_t count;
  __device__ uint32_t n() const { return count; }
  __device__ bool time(uint32_t i, unsigned long long* t) const {
    const uint4 a = recs[2 * (size_t)i];
    *t = ((unsigned long long)a.y << 32) | a.x;
    return true;
  }
  __device__ bool load(uint32_t i, Rec* r) const {
    *r = rec_load(recs, i);
    return true;
  }
};

// Received records of the sharded path, stamped on their source rank (sg_wire_record: time |
// len, src_host | event id | packet id, dst_host).  The destination stands in the record: no
// search, and no gather but host_map's.  A destination outside host_map, or mapped to no host of
// this wire, is left out by both passes and flagged (WireCtl::bad, then WE_BADDST: the next pop
// reports it).
struct SrcRecords {
  const uint4* recs;
  const uint32_t* host_map;  // may be null: the destination is the wire's host
  uint32_t* bad;             // &WireCtl::bad
  uint32_t count, n_map, n_hosts;
  __device__ uint32_t n() const { return count; }
  __device__ bool host(uint32_t d, uint32_t* h) const {
    if (d >= n_map) return false;
    *h = host_map ? host_map[d] : d;
    return *h < n_hosts;  // (UINT32_MAX, a host of another rank, included)
  }
  __device__ bool time(uint32_t i, unsigned long long* t) const {
    const uint4 a = recs[2 * (size_t)i];
    *t = ((unsigned long long)a.y << 32) | a.x;
    if (*t == WR_TOMB) return false;
    uint32_t h;
    if (host(recs[2 * (size_t)i + 1].w, &h)) return true;
    atomicOr(bad, 1u);
    return false;
  }
  __device__ bool load(uint32_t i, Rec* r) const {
    const uint4 a = recs[2 * (size_t)i], b = recs[2 * (size_t)i + 1];
    r->time = ((unsigned long long)a.y << 32) | a.x;
    if (r->time == WR_TOMB || !host(b.w, &r->dst)) return false;
    r->len = a.z;
    r->src = a.w;
    r->eid = ((unsigned long long)b.y << 32) | b.x;
    r->packet = b.z;
    return true;
  }
};

// The blocks of a fixed-split exchange: slot i is record i % cap of block i / cap, a record when
// that is below valid[block] (k_wire_padded_valid: all zero when the round overflowed its blocks).
struct SrcPaddedRecords {
  SrcRecords recs;
  const uint32_t* valid;
  uint32_t cap;
  __device__ uint32_t n() const { return recs.count; }
  __device__ bool time(uint32_t i, unsigned long long* t) const {
    return i % cap < valid[i / cap] && recs.time(i, t);
  }
  __device__ bool load(uint32_t i, Rec* r) const { return i % cap < valid[i / cap] && recs.load(i, r); }
};

// One wave: valid[b] = the records block b of recv_padded holds for `rank`, min(xall[b][3 + rank],
// cap); or 0 for every block when any pair's count exceeds cap: the round is then exchanged again
// exactly (every rank sees the same xall), and that exchange's push carries all its records.
__global__ void __launch_bounds__(64) k_wire_padded_valid(const unsigned long long* xall, uint32_t n_ranks,
                                                          uint32_t rank, uint32_t cap, uint32_t* valid) {
  const uint32_t b = threadIdx.x, wd = 3 + n_ranks;
  unsigned long long pm = 0;
  if (b < n_ranks)
    for (uint32_t r = 0; r < n_ranks; r++) pm = max(pm, xall[(size_t)b * wd + 3 + r]);
  for (int d = 32; d > 0; d >>= 1) pm = max(pm, (unsigned long long)__shfl_xor(pm, d, 64));
  if (b < n_ranks) valid[b] = pm > cap ? 0u : (uint32_t)min(xall[(size_t)b * wd + 3 + rank], (unsigned long long)cap);
}

// ---- stamp (on the source rank) -----------------------------------------------
// len and the caller's packet id into the two words of a record its owner does not read: the low
// half of order_key and `packet` (until now the index p into this rank's batch).  Not idempotent
// (the second word is its own input), so every slot is visited once.
struct WireStamp {
  const uint32_t *packet_id, *len;
  uint32_t id_base, n_packets;
};

__device__ __forceinline__ void wire_stamp(uint32_t* recs, size_t i, const WireStamp& s) {
  const uint32_t p = recs[8 * i + 6];
  if (p >= s.n_packets) return;
  recs[8 * i + 2] = s.len[p];
  recs[8 * i + 6] = s.packet_id ? s.packet_id[p] : s.id_base + p;
}

// PADDED 0: records [0, n) of `recs`.  PADDED 1: the layout k_owner_scatter writes and
// k_pad_to_compact reads (sg_deliver.hip): the first min(count_r, cap) records for rank r in block
// r of `recs`, the others at their compact positions start_r + k (k >= cap) of `spill`, an array
// of s.n_packets records; the counts are xrow[3 + r], read here, on the device.
template <int PADDED>
__global__ void __launch_bounds__(WR_THREADS) k_wire_stamp(uint32_t* recs, uint32_t* spill, uint32_t n,
                                                          uint32_t n_ranks, uint32_t cap,
                                                          const unsigned long long* xrow, WireStamp s) {
  const size_t t0 = (size_t)blockIdx.x * WR_THREADS + threadIdx.x, step = (size_t)gridDim.x * WR_THREADS;
  if (!PADDED) {
    for (size_t i = t0; i < n; i += step) wire_stamp(recs, i, s);
    return;
  }
  __shared__ unsigned long long s_cnt[WR_MAX_RANKS], s_start[WR_MAX_RANKS], s_spill[WR_MAX_RANKS + 1];
  if (threadIdx.x == 0) {
    unsigned long long a = 0, sp = 0;
    for (uint32_t r = 0; r < n_ranks; r++) {
      const unsigned long long c = min(xrow[3 + r], (unsigned long long)s.n_packets);
      s_cnt[r] = c;
      s_start[r] = a;
      s_spill[r] = sp;
      a += c;
      sp += c > cap ? c - cap : 0;
    }
    s_spill[n_ranks] = sp;
  }
  __syncthreads();
  const size_t blocks = (size_t)n_ranks * cap, total = blocks + (size_t)s_spill[n_ranks];
  for (size_t e = t0; e < total; e += step) {
    if (e < blocks) {
      const uint32_t r = (uint32_t)(e / cap);
      if (e - (size_t)r * cap < s_cnt[r]) wire_stamp(recs, e, s);
    } else {
      const unsigned long long j = e - blocks;
      uint32_t r = 0;  // the rank whose spilled records [s_spill[r], s_spill[r + 1]) hold j
      while (s_spill[r + 1] <= j) r++;
      const unsigned long long pos = s_start[r] + cap + (j - s_spill[r]);
      if (pos < s.n_packets) wire_stamp(spill, (size_t)pos, s);
    }
  }
}

// ---- append ------------------------------------------------------------------
// Pass 1: records per row, in LDS first, one global add per (block, row).
template <class S>
__global__ void __launch_bounds__(WR_THREADS) k_wire_count(WireDev w, S src) {
  __shared__ uint32_t s_hist[WR_ROWS];
  if (w.ctl->err) return;
  for (uint32_t r = threadIdx.x; r < w.R; r += WR_THREADS) s_hist[r] = 0;
  __syncthreads();
  const uint32_t n = src.n();
  const unsigned long long base = w.ctl->base, hz = w.ctl->hz;
  const uint32_t far = w.ctl->far;
  for (size_t i = (size_t)blockIdx.x * WR_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * WR_THREADS) {
    unsigned long long t;
    if (src.time((uint32_t)i, &t)) atomicAdd(&s_hist[wire_row(w, t, base, hz, far)], 1u);
  }
  __syncthreads();
  for (uint32_t r = threadIdx.x; r < w.R; r += WR_THREADS)
    if (s_hist[r]) atomicAdd(&w.add[r], s_hist[r]);
}

// Pass 2 (one block): the chunks every row needs for its counted appends, taken from the free
// list; the rows' counts grow, cur = the first new slot.  Fails whole (false, nothing changed but
// add[] cleared) when the free list or a row's table is too short.  *s_nfree: the free count
// (LDS, maintained here).  s_off / s_first: WR_ROWS + 1 / WR_ROWS words of LDS.
__device__ bool wire_alloc(const WireDev& w, uint32_t* s_nfree, uint32_t* s_off, uint32_t* s_first, uint32_t* s_w,
                           unsigned long long* added) {
  __shared__ uint32_t s_bad;
  __shared__ unsigned long long s_added;
  if (threadIdx.x == 0) {
    s_bad = 0;
    s_added = 0;
  }
  __syncthreads();
  uint32_t carry = 0;
  for (uint32_t r0 = 0; r0 < w.R; r0 += blockDim.x) {
    const uint32_t r = r0 + threadIdx.x;
    uint32_t need = 0;
    if (r < w.R) {
      const unsigned long long c0 = w.cnt[r], c1 = c0 + w.add[r];
      const uint32_t f = chunks_of(c0), l = chunks_of(c1);
      if (l > w.M || c1 > 0xFFFFFFFFull) atomicOr(&s_bad, 1u);
      need = l - f;
      s_first[r] = f;
      if (w.add[r]) atomicAdd(&s_added, (unsigned long long)w.add[r]);
    }
    uint32_t total;
    const uint32_t ex = wire_block_scan(need, s_w, &total);
    if (r < w.R) s_off[r] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) s_off[w.R] = carry;
  __syncthreads();
  const uint32_t T = s_off[w.R], nfree = *s_nfree;
  const bool ok = !s_bad && T <= nfree;
  if (ok) {
    for (uint32_t j = threadIdx.x; j < T; j += blockDim.x) {
      // the last row whose offset is <= j (rows that need nothing have empty ranges)
      uint32_t lo = 0, hi = w.R - 1;
      for (int it = 0; it < 32 && lo < hi; it++) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (s_off[mid] <= j) lo = mid;
        else hi = mid - 1;
      }
      w.tbl[(size_t)lo * w.M + s_first[lo] + (j - s_off[lo])] = w.freel[nfree - 1 - j];
    }
  }
  for (uint32_t r = threadIdx.x; r < w.R; r += blockDim.x) {
    if (ok) {
      const uint32_t c0 = w.cnt[r];
      w.cur[r] = c0;
      w.cnt[r] = c0 + w.add[r];
    }
    w.add[r] = 0;
  }
  __syncthreads();
  if (threadIdx.x == 0 && ok) *s_nfree = nfree - T;
  *added = ok ? s_added : 0;
  __syncthreads();
  return ok;
}

__global__ void __launch_bounds__(1024) k_wire_alloc(WireDev w) {
  __shared__ uint32_t s_off[WR_ROWS + 1], s_first[WR_ROWS], s_w[17], s_nfree;
  // With `bad` set the batch is left out whole, and its counts stay in add[]: harmless only because
  // err is sticky and every append kernel returns on it until k_wire_reset (sg_wire_set_state)
  // clears add[] too.  A way to clear err without a reset would have to clear add[] as well.
  if (threadIdx.x == 0 && w.ctl->bad) w.ctl->err |= WE_BADDST;
  __syncthreads();
  if (w.ctl->err) return;
  if (threadIdx.x == 0) s_nfree = w.ctl->nfree;
  __syncthreads();
  unsigned long long added;
  const bool ok = wire_alloc(w, &s_nfree, s_off, s_first, s_w, &added);
  if (threadIdx.x == 0) {
    if (ok) {
      w.ctl->nfree = s_nfree;
      w.ctl->held += added;
      w.ctl->pushed += added;
    } else {
      w.ctl->err |= WE_ARENA;
    }
  }
}

// Pass 3, for up to WR_ITEMS records per thread: ranks inside the block through LDS, one global
// reservation per (block, row), then the stores.  Called by every thread of the block.  A
// workgroup covers WR_THREADS x WR_ITEMS records per step so that the reservations -- global
// atomics on as many addresses as the batch touches rows, a few dozen -- stay in the hundreds
// per address for a 1M batch.  The row minimum is lowered only when it moves (a stale read
// can only be too large, which costs one atomic more).
template <int N>
__device__ __forceinline__ void wire_append(const WireDev& w, const bool (&has)[N], const uint32_t (&row)[N],
                                            const Rec (&rec)[N], uint32_t* s_hist, uint32_t* s_base,
                                            unsigned long long* s_min) {
  for (uint32_t r = threadIdx.x; r < w.R; r += WR_THREADS) {
    s_hist[r] = 0;
    s_min[r] = ~0ull;
  }
  __syncthreads();
  uint32_t rank[N];
#pragma unroll
  for (int k = 0; k < N; k++) {
    rank[k] = 0;
    if (has[k]) {
      rank[k] = atomicAdd(&s_hist[row[k]], 1u);
      atomicMin(&s_min[row[k]], rec[k].time);
    }
  }
  __syncthreads();
  for (uint32_t r = threadIdx.x; r < w.R; r += WR_THREADS)
    if (s_hist[r]) {
      s_base[r] = atomicAdd(&w.cur[r], s_hist[r]);
      if (s_min[r] < w.rmin[r]) atomicMin(&w.rmin[r], s_min[r]);
    }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++)
    if (has[k]) {
      const uint32_t slot = s_base[row[k]] + rank[k];
      if (slot / WR_CHUNK < w.M) rec_store(w.arena, wire_slot(w, row[k], slot), rec[k]);
    }
}

template <class S>
__global__ void __launch_bounds__(WR_THREADS) k_wire_scatter(WireDev w, S src) {
  __shared__ uint32_t s_hist[WR_ROWS], s_base[WR_ROWS];
  __shared__ unsigned long long s_min[WR_ROWS];
  if (w.ctl->err) return;
  const uint32_t n = src.n();
  const unsigned long long base = w.ctl->base, hz = w.ctl->hz;
  const uint32_t far = w.ctl->far;
  constexpr size_t STEP = (size_t)WR_THREADS * WR_ITEMS;
  for (size_t b0 = (size_t)blockIdx.x * STEP; b0 < n; b0 += (size_t)gridDim.x * STEP) {
    bool has[WR_ITEMS];
    uint32_t row[WR_ITEMS];
    Rec rec[WR_ITEMS];
#pragma unroll
    for (int k = 0; k < WR_ITEMS; k++) {
      const size_t i = b0 + (size_t)k * WR_THREADS + threadIdx.x;
      rec[k] = Rec{};
      has[k] = i < n && src.load((uint32_t)i, &rec[k]);
      row[k] = has[k] ? wire_row(w, rec[k].time, base, hz, far) : 0;
    }
    wire_append<WR_ITEMS>(w, has, row, rec, s_hist, s_base, s_min);
  }
}

// Block-wide: hand a row's chunks back and empty it.
__device__ __forceinline__ void wire_free_row(const WireDev& w, uint32_t row, uint32_t* s_nfree) {
  const uint32_t nc = chunks_of(w.cnt[row]), nf = *s_nfree;
  for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x)
    if (nf + k < w.M) w.freel[nf + k] = w.tbl[(size_t)row * w.M + k];
  __syncthreads();
  if (threadIdx.x == 0) {
    *s_nfree = min(nf + nc, w.M);
    w.cnt[row] = 0;
    w.rmin[row] = ~0ull;
    w.dead[row] = 0;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(1024) k_wire_reset(WireDev w) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < w.M; i += gridDim.x * blockDim.x) w.freel[i] = i;
  if (blockIdx.x == 0) {
    for (uint32_t r = threadIdx.x; r < w.R; r += blockDim.x) {
      w.cnt[r] = w.add[r] = w.cur[r] = w.dead[r] = 0;
      w.rmin[r] = ~0ull;
    }
    if (threadIdx.x == 0) {
      WireCtl c = {};
      c.base = 0;
      c.hz = w.n_bins;
      c.far = w.n_bins;
      c.nfree = w.M;
      *w.ctl = c;
    }
  }
}

// ---- pop -----------------------------------------------------------------------
// The rows a window touches.  With wb = W / bin_ns: ring bins [base, min(wb, hz)) are wholly due
// (every time in bin b is below (b + 1) bin_ns <= W; what clamped into bin `base` is earlier
// still); bin max(wb, base), if in the ring, straddles W.  base advances to wb, kept n_bins short
// of the top so that base + n_bins cannot overflow (bins in [newbase, wb) are then empty ring rows
// like any other).  The horizon follows base at once while the far row is empty; otherwise only
// when the window reaches it or half a ring has gone by, and the far row is re-binned.
__global__ void __launch_bounds__(1024) k_wire_plan(WireDev w, WirePlan* pl, unsigned long long W) {
  __shared__ uint32_t s_w[17];
  const unsigned long long base = w.ctl->base, hz = w.ctl->hz, wb = W / w.bin_ns;
  const uint32_t far = w.ctl->far;
  const unsigned long long top = max(wb, base);
  const unsigned long long bend = min(top, hz - 1);  // hz > base always
  const uint32_t n_ring = (uint32_t)(bend - base) + 1;
  const unsigned long long newbase = min(top, ~0ull - w.n_bins);
  const unsigned long long cand = newbase + w.n_bins;
  const bool far_empty = w.cnt[far] == 0;
  // Re-binning writes the far records again beside the old row: when the window has not reached
  // hz it can wait, and does while the free list could not hold a copy (every record into a chunk
  // of its own row at worst: the row's chunks + one per row)
  const bool room = w.ctl->nfree >= chunks_of(w.cnt[far]) + w.R;
  const bool rebin = !far_empty && (wb >= hz || (cand - hz >= w.n_bins / 2 && room));
  const uint32_t n_ent = n_ring + (rebin ? 1 : 0);
  uint32_t carry = 0;
  for (uint32_t e0 = 0; e0 < n_ent; e0 += blockDim.x) {
    const uint32_t e = e0 + threadIdx.x;
    uint32_t c = 0;
    if (e < n_ent) {
      const unsigned long long b = base + e;
      const uint32_t row = e < n_ring ? ((uint32_t)b & w.mask) : far;
      c = w.cnt[row];
      pl->ent_row[e] = row;
      pl->ent_kind[e] = e < n_ring ? (b < wb ? 0u : 1u) : 2u;
    }
    uint32_t total;
    const uint32_t ex = wire_block_scan(c, s_w, &total);
    if (e < n_ent) pl->ent_off[e] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    pl->ent_off[n_ent] = carry;
    if (!rebin) pl->ent_off[n_ent + 1] = carry;  // (the far range is empty)
    pl->W = W;
    pl->newbase = newbase;
    pl->newhz = (far_empty || rebin) ? cand : hz;
    pl->n_ring = n_ring;
    pl->rebin = rebin;
    pl->newfar = rebin ? (far == w.n_bins ? w.n_bins + 1 : w.n_bins) : far;
    pl->verdict = WV_OK;
    pl->due = 0;
    pl->n_work = 0;
  }
}

// Entry and slot of scan position g; s_off holds the plan's offsets.
__device__ __forceinline__ uint32_t wire_entry(const uint32_t* s_off, uint32_t n_ent, uint32_t g) {
  uint32_t lo = 0, hi = n_ent - 1;
  for (int it = 0; it < 32 && lo < hi; it++) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (s_off[mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Due records per destination host; the records of a far row being re-binned that stay are
// counted into the rows of the new geometry (pass 1 of their append).
__global__ void __launch_bounds__(WR_THREADS) k_wire_popcount(WireDev w, WirePlan* pl, uint32_t* hcnt,
                                                             uint32_t n_hosts) {
  __shared__ uint32_t s_off[WR_ROWS + 1], s_hist[WR_ROWS], s_due;
  const uint32_t n_ent = pl->n_ring + pl->rebin;
  const bool rebin = pl->rebin != 0;
  for (uint32_t e = threadIdx.x; e <= n_ent; e += WR_THREADS) s_off[e] = pl->ent_off[e];
  if (rebin)
    for (uint32_t r = threadIdx.x; r < w.R; r += WR_THREADS) s_hist[r] = 0;
  if (threadIdx.x == 0) s_due = 0;
  __syncthreads();
  const uint32_t total = s_off[n_ent];
  const unsigned long long W = pl->W;
  uint32_t due = 0;
  for (size_t g = (size_t)blockIdx.x * WR_THREADS + threadIdx.x; g < total; g += (size_t)gridDim.x * WR_THREADS) {
    const uint32_t e = wire_entry(s_off, n_ent, (uint32_t)g);
    const Rec r = rec_load(w.arena, wire_slot(w, pl->ent_row[e], (uint32_t)g - s_off[e]));
    if (r.time == WR_TOMB) continue;
    if (r.time < W) {
      if (r.dst < n_hosts) {
        atomicAdd(&hcnt[r.dst], 1u);
        due++;
      }
    } else if (pl->ent_kind[e] == 2) {
      atomicAdd(&s_hist[wire_row(w, r.time, pl->newbase, pl->newhz, pl->newfar)], 1u);  // (only when rebin)
    }
  }
  if (due) atomicAdd(&s_due, due);
  __syncthreads();
  if (threadIdx.x == 0 && s_due) atomicAdd(&pl->due, s_due);
  if (rebin)
    for (uint32_t r = threadIdx.x; r < w.R; r += WR_THREADS)
      if (s_hist[r]) atomicAdd(&w.add[r], s_hist[r]);
}

// The verdict, before anything moves ("rejected whole", as k_host_off / ERR_BATCH in
// sg_deliver.hip): the due records fit out->cap, and -- when a far row is re-binned -- the free
// list, with the drained rows' chunks back on it, covers the chunks its records need.
__global__ void __launch_bounds__(1024) k_wire_commit(WireDev w, WirePlan* pl, uint32_t cap) {
  __shared__ uint32_t s_drained[WR_ROWS], s_need, s_freed, s_bad;
  for (uint32_t r = threadIdx.x; r < w.R; r += blockDim.x) s_drained[r] = 0;
  if (threadIdx.x == 0) s_need = s_freed = s_bad = 0;
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < pl->n_ring; e += blockDim.x)
    if (pl->ent_kind[e] == 0) s_drained[pl->ent_row[e]] = 1;
  __syncthreads();
  if (pl->rebin) {
    for (uint32_t r = threadIdx.x; r < w.R; r += blockDim.x) {
      const unsigned long long c0 = s_drained[r] ? 0 : w.cnt[r], c1 = c0 + w.add[r];
      if (chunks_of(c1) > w.M || c1 > 0xFFFFFFFFull) atomicOr(&s_bad, 1u);
      atomicAdd(&s_need, chunks_of(c1) - chunks_of(c0));
      if (s_drained[r]) atomicAdd(&s_freed, chunks_of(w.cnt[r]));
    }
  }
  __syncthreads();
  uint32_t v = WV_OK;
  if (w.ctl->err) v = WV_ERR;
  else if (pl->due > cap) v = WV_CAP;
  else if (pl->rebin && (s_bad || s_need > w.ctl->nfree + s_freed)) v = WV_ARENA;
  __syncthreads();
  if (v != WV_OK) {
    for (uint32_t r = threadIdx.x; r < w.R; r += blockDim.x) w.add[r] = 0;
  } else {
    // the straddling row is filtered: its minimum is taken again over what stays
    for (uint32_t e = threadIdx.x; e < pl->n_ring; e += blockDim.x)
      if (pl->ent_kind[e] == 1) w.rmin[pl->ent_row[e]] = ~0ull;
  }
  if (threadIdx.x == 0) pl->verdict = v;
}

// PHASE 0: the ring entries.  A due record goes to the staging array at its host's next position;
// in the straddling row it leaves a tombstone, and the records that stay give the row's new
// minimum.  PHASE 1: the far row being re-binned: due records likewise, the others are appended
// under the new geometry (k_wire_mid has allocated their chunks).
template <int PHASE>
__global__ void __launch_bounds__(WR_THREADS) k_wire_move(WireDev w, const WirePlan* pl, const uint32_t* hoff,
                                                         uint32_t* hcur, uint32_t n_hosts, uint4* stage,
                                                         uint32_t cap) {
  __shared__ uint32_t s_off[WR_ROWS + 1], s_hist[PHASE ? WR_ROWS : 1], s_base[PHASE ? WR_ROWS : 1];
  __shared__ unsigned long long s_min[PHASE ? WR_ROWS : 1];
  if (pl->verdict != WV_OK || (PHASE == 1 && !pl->rebin)) return;
  const uint32_t n_ring = pl->n_ring, n_ent = n_ring + pl->rebin;
  for (uint32_t e = threadIdx.x; e <= n_ent; e += WR_THREADS) s_off[e] = pl->ent_off[e];
  __shared__ uint32_t s_tomb;
  if (PHASE == 0 && threadIdx.x == 0) {
    s_min[0] = ~0ull;
    s_tomb = 0;
  }
  __syncthreads();
  const unsigned long long W = pl->W;
  const uint32_t begin = PHASE ? s_off[n_ring] : 0, end = PHASE ? s_off[n_ent] : s_off[n_ring];
  constexpr int N = PHASE ? WR_ITEMS : 1;
  constexpr size_t STEP = (size_t)WR_THREADS * N;
  for (size_t b0 = (size_t)begin + (size_t)blockIdx.x * STEP; b0 < end; b0 += (size_t)gridDim.x * STEP) {
    bool stays[N];
    uint32_t row[N];
    Rec rec[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
      const size_t g = b0 + (size_t)k * WR_THREADS + threadIdx.x;
      stays[k] = false;
      row[k] = 0;
      rec[k] = Rec{};
      if (g >= end) continue;
      const uint32_t e = PHASE ? n_ring : wire_entry(s_off, n_ring, (uint32_t)g);
      const size_t at = wire_slot(w, pl->ent_row[e], (uint32_t)g - s_off[e]);
      const Rec r = rec_load(w.arena, at);
      if (r.time == WR_TOMB) continue;
      if (r.time < W) {
        if (r.dst < n_hosts) {
          const uint32_t pos = hoff[r.dst] + atomicAdd(&hcur[r.dst], 1u);
          if (pos < cap) rec_store(stage, pos, r);
        }
        if (PHASE == 0 && pl->ent_kind[e] == 1) {
          w.arena[2 * at] = make_uint4(~0u, ~0u, ~0u, ~0u);
          atomicAdd(&s_tomb, 1u);
        }
      } else {
        stays[k] = true;
        rec[k] = r;
        if (PHASE == 0) atomicMin(&s_min[0], r.time);  // only the straddling row has records that stay
        else row[k] = wire_row(w, r.time, pl->newbase, pl->newhz, pl->newfar);
      }
    }
    if (PHASE == 1) wire_append<N>(w, stays, row, rec, s_hist, s_base, s_min);
  }
  if (PHASE == 0) {
    __syncthreads();
    const uint32_t e = n_ring - 1;  // the straddling entry is the last one (n_ring >= 1)
    if (threadIdx.x == 0 && pl->ent_kind[e] == 1) {
      if (s_min[0] != ~0ull) atomicMin(&w.rmin[pl->ent_row[e]], s_min[0]);
      if (s_tomb) atomicAdd(&w.dead[pl->ent_row[e]], s_tomb);
    }
  }
}

// Between the two moves (one block): the drained rows' chunks go back, the calendar advances, and
// the far records that stay get their chunks (the commit checked the room).
__global__ void __launch_bounds__(1024) k_wire_mid(WireDev w, WirePlan* pl) {
  __shared__ uint32_t s_off[WR_ROWS + 1], s_first[WR_ROWS], s_w[17], s_nfree;
  if (pl->verdict != WV_OK) return;
  if (threadIdx.x == 0) s_nfree = w.ctl->nfree;
  __syncthreads();
  const uint32_t n_ring = pl->n_ring;
  for (uint32_t e = 0; e < n_ring; e++)
    if (pl->ent_kind[e] == 0 && w.cnt[pl->ent_row[e]]) wire_free_row(w, pl->ent_row[e], &s_nfree);
  if (pl->rebin) {
    unsigned long long added;
    if (!wire_alloc(w, &s_nfree, s_off, s_first, s_w, &added) && threadIdx.x == 0) w.ctl->err |= WE_ARENA;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    w.ctl->nfree = s_nfree;
    w.ctl->base = pl->newbase;
    w.ctl->hz = pl->newhz;
  }
}

// One block: the old far row goes back, the counters settle, next_time = the smallest row minimum.
__global__ void __launch_bounds__(1024) k_wire_final(WireDev w, WirePlan* pl, WireRet* ret) {
  __shared__ uint32_t s_nfree;
  __shared__ unsigned long long s_min;
  if (threadIdx.x == 0) {
    s_nfree = w.ctl->nfree;
    s_min = ~0ull;
  }
  __syncthreads();
  const uint32_t v = pl->verdict;
  if (v == WV_OK && pl->rebin) {
    wire_free_row(w, w.ctl->far, &s_nfree);
    if (threadIdx.x == 0) {
      w.ctl->nfree = s_nfree;
      w.ctl->far = pl->newfar;
    }
  }
  unsigned long long m = ~0ull;
  for (uint32_t r = threadIdx.x; r < w.R; r += blockDim.x) m = min(m, w.rmin[r]);
  if (m != ~0ull) atomicMin(&s_min, m);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (v == WV_OK) w.ctl->held -= min((unsigned long long)pl->due, w.ctl->held);
    ret->verdict = w.ctl->err && v == WV_OK ? WV_ERR : v;
    ret->due = pl->due;
    ret->next = s_min;
    ret->held = w.ctl->held;
    ret->pushed = w.ctl->pushed;
    w.ctl->pushed = 0;
    ret->err = w.ctl->err;
    ret->compact_row = ~0u;
    const uint32_t e = pl->n_ring - 1;
    if (v == WV_OK && !w.ctl->err && pl->ent_kind[e] == 1) {
      const uint32_t row = pl->ent_row[e], c = w.cnt[row], d = min(w.dead[row], c), live = c - d;
      if (d >= max(live / WR_DEAD_SHARE, WR_CHUNK)) {
        ret->compact_row = row;
        ret->compact_cnt = c;
        ret->compact_keep = live;
      }
    }
  }
}

// ---- compaction of a straddling row ----------------------------------------------
// A row that straddles window after window (bin_ns longer than a round) keeps its popped records
// as tombstones until the window has passed the whole bin.  To keep the slots in use within
// 9/8 of the events held (+ a chunk per row), the row is compacted in place as soon as a pop
// leaves it with tombstones >= live / 8: with `keep` live records among `cnt` slots, the live
// records in slots [keep, cnt) (movers) go into the tombstones in slots [0, keep) (holes) -- there
// are equally many -- and the chunks past `keep` go back.  Only holes are written and only
// movers read, so any pairing is safe.  Launched after the pop's synchronisation, when the host
// knows the sizes: grids over the row's slots, amortised against the pops that made the holes.
__global__ void __launch_bounds__(WR_THREADS) k_wire_compact_list(WireDev w, uint32_t row, uint32_t cnt, uint32_t keep,
                                                                 uint32_t* ctr, uint32_t* holes, uint32_t* movers,
                                                                 uint32_t h_max) {
  for (size_t s = (size_t)blockIdx.x * WR_THREADS + threadIdx.x; s < cnt; s += (size_t)gridDim.x * WR_THREADS) {
    const uint4 a = w.arena[2 * wire_slot(w, row, (uint32_t)s)];
    const bool tomb = (a.x & a.y) == ~0u;
    if (s < keep && tomb) {
      const uint32_t i = atomicAdd(&ctr[0], 1u);
      if (i < h_max) holes[i] = (uint32_t)s;
    } else if (s >= keep && !tomb) {
      const uint32_t i = atomicAdd(&ctr[1], 1u);
      if (i < h_max) movers[i] = (uint32_t)s;
    }
  }
}

__global__ void __launch_bounds__(WR_THREADS) k_wire_compact_move(WireDev w, uint32_t row, const uint32_t* ctr,
                                                                 const uint32_t* holes, const uint32_t* movers,
                                                                 uint32_t h_max) {
  const uint32_t n = ctr[0];
  if (n != ctr[1] || n > h_max) return;  // (k_wire_compact_finish reports it)
  for (size_t i = (size_t)blockIdx.x * WR_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * WR_THREADS)
    rec_store(w.arena, wire_slot(w, row, holes[i]), rec_load(w.arena, wire_slot(w, row, movers[i])));
}

__global__ void __launch_bounds__(1024) k_wire_compact_finish(WireDev w, uint32_t row, uint32_t cnt, uint32_t keep,
                                                             const uint32_t* ctr, uint32_t h_max) {
  if (ctr[0] != ctr[1] || ctr[0] > h_max || w.cnt[row] != cnt) {  // the row is not what the pop reported
    if (threadIdx.x == 0) w.ctl->err |= WE_CORRUPT;
    return;
  }
  const uint32_t c0 = chunks_of(keep), c1 = chunks_of(cnt), nf = w.ctl->nfree;
  for (uint32_t k = c0 + threadIdx.x; k < c1; k += blockDim.x)
    if (nf + (k - c0) < w.M) w.freel[nf + (k - c0)] = w.tbl[(size_t)row * w.M + k];
  __syncthreads();
  if (threadIdx.x == 0) {
    w.ctl->nfree = min(nf + (c1 - c0), w.M);
    w.cnt[row] = keep;
    w.dead[row] = 0;
  }
}

// sg_wire_get_state: every live record of every row into one contiguous array (any order; the
// host sorts).  off: the rows' slot offsets.  A checkpoint path: its grid covers the whole store.
__global__ void __launch_bounds__(WR_THREADS) k_wire_gather(WireDev w, const uint32_t* off, uint4* out, uint32_t* ctr,
                                                           uint32_t cap) {
  const uint32_t total = off[w.R];
  for (size_t g = (size_t)blockIdx.x * WR_THREADS + threadIdx.x; g < total; g += (size_t)gridDim.x * WR_THREADS) {
    const uint32_t row = wire_entry(off, w.R, (uint32_t)g);
    const Rec r = rec_load(w.arena, wire_slot(w, row, (uint32_t)g - off[row]));
    if (r.time == WR_TOMB) continue;
    const uint32_t pos = atomicAdd(ctr, 1u);
    if (pos < cap) rec_store(out, pos, r);
  }
}

// ---- the sort tiers ------------------------------------------------------------
struct WireOut {
  uint32_t* host;
  unsigned long long* time_ns;
  uint32_t *packet, *len, *src_host;
  unsigned long long* event_id;
};

__device__ __forceinline__ void wire_emit(const WireOut& o, size_t pos, const Rec& r) {
  o.host[pos] = r.dst;
  o.time_ns[pos] = r.time;
  o.packet[pos] = r.packet;
  o.len[pos] = r.len;
  if (o.src_host) {
    o.src_host[pos] = r.src;
    o.event_id[pos] = r.eid;
  }
}

// Tier 1, a wave per host: a segment of up to 64 records is ranked in registers (each lane counts
// the keys below its own; keys are unique, so ranks are a permutation).  A longer one is cut into
// pieces of WR_LDS_SORT_MAX for the next two kernels: work entry = (host, piece).
__global__ void __launch_bounds__(WR_THREADS) k_wire_sort_small(WirePlan* pl, const uint32_t* hoff, uint32_t n_hosts,
                                                               const uint4* stage, WireOut out, uint2* work,
                                                               uint32_t work_cap) {
  if (pl->verdict != WV_OK) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * WR_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * WR_THREADS) >> 6;
  for (uint32_t h = wave; h < n_hosts; h += n_waves) {
    const uint32_t s0 = hoff[h];
    const uint32_t n = __builtin_amdgcn_readfirstlane(hoff[h + 1] - s0);
    if (n == 0) continue;
    if (n <= WR_RANK_SORT_MAX) {
      Rec r = {};
      if (lane < n) r = rec_load(stage, (size_t)s0 + lane);
      uint32_t rank = 0;
      for (uint32_t j = 0; j < n; j++) {
        const unsigned long long tj = __shfl(r.time, (int)j, 64), ej = __shfl(r.eid, (int)j, 64);
        const uint32_t sj = __shfl(r.src, (int)j, 64);
        rank += key_less(tj, sj, ej, r.time, r.src, r.eid) ? 1u : 0u;
      }
      if (lane < n) wire_emit(out, (size_t)s0 + rank, r);
    } else {
      const uint32_t pieces = (n + WR_LDS_SORT_MAX - 1) / WR_LDS_SORT_MAX;
      uint32_t at = 0;
      if (lane == 0) at = atomicAdd(&pl->n_work, pieces);
      at = __shfl(at, 0, 64);
      for (uint32_t c = lane; c < pieces; c += 64)
        if (at + c < work_cap) work[at + c] = make_uint2(h, c);
    }
  }
}

struct WireKey {
  unsigned long long t, e;
  uint32_t s, idx;
};

// Tier 2, a workgroup per piece: bitonic sort of the keys in LDS.  A segment of one piece is
// final: written out.  A piece of a longer segment goes, sorted, to the second staging array.
__global__ void __launch_bounds__(WR_THREADS) k_wire_sort_lds(const WirePlan* pl, const uint32_t* hoff,
                                                             const uint4* stage, uint4* stage2, WireOut out,
                                                             const uint2* work, uint32_t work_cap) {
  __shared__ WireKey s_key[WR_LDS_SORT_MAX];
  if (pl->verdict != WV_OK) return;
  const uint32_t n_work = min(pl->n_work, work_cap);
  for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
    const uint2 we = work[wi];
    const uint32_t s0 = hoff[we.x], n = hoff[we.x + 1] - s0;
    const uint32_t p0 = we.y * WR_LDS_SORT_MAX, m = min(n - p0, WR_LDS_SORT_MAX);
    uint32_t P = 64;
    while (P < m) P <<= 1;  // <= WR_LDS_SORT_MAX
    for (uint32_t i = threadIdx.x; i < P; i += WR_THREADS) {
      WireKey k = {~0ull, ~0ull, ~0u, ~0u};  // padding sorts last (no event is at UINT64_MAX)
      if (i < m) {
        const Rec r = rec_load(stage, (size_t)s0 + p0 + i);
        k = WireKey{r.time, r.eid, r.src, i};
      }
      s_key[i] = k;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t i = threadIdx.x; i < P; i += WR_THREADS) {
          const uint32_t x = i ^ j;
          if (x > i) {
            const WireKey a = s_key[i], b = s_key[x];
            const bool up = (i & k) == 0;
            if (key_less(b.t, b.s, b.e, a.t, a.s, a.e) == up) {
              s_key[i] = b;
              s_key[x] = a;
            }
          }
        }
        __syncthreads();
      }
    for (uint32_t i = threadIdx.x; i < m; i += WR_THREADS) {
      const Rec r = rec_load(stage, (size_t)s0 + p0 + s_key[i].idx);
      if (n <= WR_LDS_SORT_MAX) wire_emit(out, (size_t)s0 + i, r);
      else rec_store(stage2, (size_t)s0 + p0 + i, r);
    }
    __syncthreads();
  }
}

// Tier 3, a hot destination: the segment's sorted pieces are merged by rank -- a record's final
// position is its index in its own piece plus, for every other piece, the number of keys below
// its own (a binary search; unique keys, so no tie rule is needed).
__global__ void __launch_bounds__(WR_THREADS) k_wire_merge(const WirePlan* pl, const uint32_t* hoff,
                                                          const uint4* stage2, WireOut out, const uint2* work,
                                                          uint32_t work_cap) {
  if (pl->verdict != WV_OK) return;
  const uint32_t n_work = min(pl->n_work, work_cap);
  for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
    const uint2 we = work[wi];
    const uint32_t s0 = hoff[we.x], n = hoff[we.x + 1] - s0;
    if (n <= WR_LDS_SORT_MAX) continue;
    const uint32_t pieces = (n + WR_LDS_SORT_MAX - 1) / WR_LDS_SORT_MAX;
    const uint32_t p0 = we.y * WR_LDS_SORT_MAX, m = min(n - p0, WR_LDS_SORT_MAX);
    for (uint32_t i = threadIdx.x; i < m; i += WR_THREADS) {
      const Rec r = rec_load(stage2, (size_t)s0 + p0 + i);
      uint32_t rank = i;
      for (uint32_t c = 0; c < pieces; c++) {
        if (c == we.y) continue;
        const uint32_t q0 = c * WR_LDS_SORT_MAX, qm = min(n - q0, WR_LDS_SORT_MAX);
        uint32_t lo = 0, hi = qm;  // the first index of piece c whose key is not below r's
        for (int it = 0; it < 32 && lo < hi; it++) {
          const uint32_t mid = lo + (hi - lo) / 2;
          const Rec q = rec_load(stage2, (size_t)s0 + q0 + mid);
          if (key_less(q.time, q.src, q.eid, r.time, r.src, r.eid)) lo = mid + 1;
          else hi = mid;
        }
        rank += lo;
      }
      wire_emit(out, (size_t)s0 + rank, r);
    }
  }
}

}  // namespace
}  // namespace sg

struct sg_wire {
  sg_ctx* ctx = nullptr;
  uint32_t n_hosts = 0;
  uint64_t capacity = 0, count = 0;
  sg::WireDev d = {};
  sg::WirePlan* plan = nullptr;
  uint32_t* hbuf = nullptr;  // hcnt [n_hosts + 1], hcur [n_hosts], hoff [n_hosts + 1], valid [WR_MAX_RANKS]
  sg::WireRet* ret = nullptr;
  ~sg_wire() {
    void* ps[] = {d.ctl, d.cnt, d.rmin, d.tbl, d.freel, d.arena, plan, hbuf};
    for (void* p : ps)
      if (p) (void)hipFree(p);
    if (ret) (void)hipHostFree(ret);
  }
};

namespace sg {
namespace {

template <class S>
void wire_append_launch(sg_ctx* ctx, sg_wire* w, const S& src, uint32_t n) {
  hipStream_t st = ctx->stream;
  // a workgroup flushes its per-row counts with one global atomic per row it touched: few, fat
  // workgroups (2 per CU) keep those at a few hundred per row and launch
  const unsigned grid = grid_for(n, WR_THREADS * WR_ITEMS, (unsigned)ctx->n_cu * 2);
  hipLaunchKernelGGL(k_wire_count<S>, dim3(grid), dim3(WR_THREADS), 0, st, w->d, src);
  hipLaunchKernelGGL(k_wire_alloc, dim3(1), dim3(1024), 0, st, w->d);
  hipLaunchKernelGGL(k_wire_scatter<S>, dim3(grid), dim3(WR_THREADS), 0, st, w->d, src);
  SG_CHECK_LAUNCH();
}

void wire_reset(sg_ctx* ctx, sg_wire* w) {
  hipLaunchKernelGGL(k_wire_reset, dim3(grid_for(w->d.M, 1024, 256)), dim3(1024), 0, ctx->stream, w->d);
  SG_CHECK_LAUNCH();
  w->count = 0;
}

}  // namespace
}  // namespace sg

extern "C" {

int32_t sg_wire_create(sg_ctx* ctx, uint32_t n_hosts, uint64_t capacity, uint64_t bin_ns, uint32_t n_bins,
                       sg_wire** out) {
  if (!out) return SG_ERR_INVALID_ARG;
  *out = nullptr;
  if (!ctx) return SG_ERR_INVALID_ARG;
  sg_wire* w = nullptr;
  int32_t rc = sg::guarded(ctx, [&] {
    using namespace sg;
    if (!n_hosts || !capacity || !bin_ns) throw Error(SG_ERR_INVALID_ARG, "n_hosts, capacity and bin_ns must be >= 1");
    if (capacity > WR_CAP_MAX) throw Error(SG_ERR_INVALID_ARG, "capacity above 2^31 events");
    // the geometry is free (results never depend on it): a power of two in [2, WR_MAX_BINS]
    uint32_t nb = 2;
    while (nb < n_bins && nb < WR_MAX_BINS) nb <<= 1;
    w = new sg_wire();
    w->ctx = ctx;
    w->n_hosts = n_hosts;
    w->capacity = capacity;
    WireDev& d = w->d;
    d.bin_ns = bin_ns;
    d.n_bins = nb;
    d.mask = nb - 1;
    d.R = nb + 2;
    // Every row may end in a partly filled chunk and hold up to a chunk of tombstones; of the quarter
    // of the capacity on top, an eighth covers the tombstones compaction allows, the rest lets a far
    // row be written again beside itself.
    const uint64_t c = (capacity + WR_CHUNK - 1) / WR_CHUNK;
    d.M = (uint32_t)(c + c / 4 + 2 * (uint64_t)d.R + 4);
    const size_t R = d.R, M = d.M;
    SG_HIP(hipMalloc(&d.ctl, sizeof(WireCtl)));
    SG_HIP(hipMalloc(&d.cnt, 4 * R * 4));
    d.add = d.cnt + R;
    d.cur = d.add + R;
    d.dead = d.cur + R;
    SG_HIP(hipMalloc(&d.rmin, R * 8));
    SG_HIP(hipMalloc(&d.tbl, R * M * 4));
    SG_HIP(hipMalloc(&d.freel, M * 4));
    SG_HIP(hipMalloc(&d.arena, M * WR_CHUNK * 32));
    SG_HIP(hipMalloc(&w->plan, sizeof(WirePlan)));
    SG_HIP(hipMalloc(&w->hbuf, (3 * (size_t)n_hosts + 2 + WR_MAX_RANKS) * 4));
    SG_HIP(hipHostMalloc(&w->ret, sizeof(WireRet), hipHostMallocMapped | hipHostMallocCoherent));
    wire_reset(ctx, w);
    SG_HIP(hipStreamSynchronize(ctx->stream));
  });
  if (rc != SG_OK) {
    delete w;
    return rc;
  }
  *out = w;
  return SG_OK;
}

void sg_wire_destroy(sg_wire* w) {
  if (!w) return;
  if (w->ctx) {
    (void)hipSetDevice(w->ctx->device);
    if (w->ctx->stream) (void)hipStreamSynchronize(w->ctx->stream);
  }
  delete w;
}

uint64_t sg_wire_count(const sg_wire* w) { return w ? w->count : 0; }

int32_t sg_wire_push(sg_ctx* ctx, sg_wire* w, const sg_packets* packets, const sg_deliveries* out,
                     const uint32_t* packet_id, uint32_t id_base, const uint32_t* len) {
  if (!w || !packets || !out || !len) return SG_ERR_INVALID_ARG;
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (w->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "the wire belongs to another context");
    const uint32_t n = packets->n_packets;
    if (!n) return;
    if (!packets->src_host || !out->deliver_time_ns || !out->event_id || !out->dst_order || !out->dst_offsets)
      throw Error(SG_ERR_INVALID_ARG, "null delivery array");
    // conservative (dropped packets count too), so that no device value is needed: the call stays
    // asynchronous; sg_wire_pop brings the count back to the events really held
    if (w->count + n > w->capacity)
      throw Error(SG_ERR_CAPACITY, "sg_wire_push: count + n_packets exceeds the wire's capacity");
    SrcDelivery s{out->dst_order, out->dst_offsets, (const unsigned long long*)out->deliver_time_ns,
                  (const unsigned long long*)out->event_id, packets->src_host, packet_id, len,
                  w->n_hosts, n, id_base};
    {
      TimedLaunch tl(ctx, "wire_push", 0.0);  // the work (events x 32 B) is known at the next pop
      wire_append_launch(ctx, w, s, n);
    }
    w->count += n;
  });
}

int32_t sg_wire_stamp_records(sg_ctx* ctx, sg_record* send, uint32_t n_records, const uint32_t* packet_id,
                              uint32_t id_base, const uint32_t* len, uint32_t n_packets) {
  if (!len || (n_records && !send)) return SG_ERR_INVALID_ARG;
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (!n_records) return;
    TimedLaunch tl(ctx, "wire_stamp", 32.0 * n_records);
    hipLaunchKernelGGL(k_wire_stamp<0>, dim3(grid_for(n_records, WR_THREADS, (unsigned)ctx->n_cu * 8)),
                       dim3(WR_THREADS), 0, ctx->stream, (uint32_t*)send, (uint32_t*)nullptr, n_records, 0u, 0u,
                       (const unsigned long long*)nullptr, WireStamp{packet_id, len, id_base, n_packets});
    SG_CHECK_LAUNCH();
  });
}

int32_t sg_wire_stamp_records_padded(sg_ctx* ctx, sg_record* send_padded, sg_record* send, uint32_t n_ranks,
                                     uint32_t cap, const uint64_t* xrow, const uint32_t* packet_id, uint32_t id_base,
                                     const uint32_t* len, uint32_t n_packets) {
  if (!send_padded || !send || !xrow || !len) return SG_ERR_INVALID_ARG;
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (n_ranks == 0 || n_ranks > WR_MAX_RANKS || cap == 0 || (uint64_t)n_ranks * cap > 0xFFFFFFFFull)
      throw Error(SG_ERR_INVALID_ARG, "bad n_ranks / cap");
    // the counts are on the device: the grid covers the blocks and, at most, a spilled record per packet
    const size_t most = (size_t)n_ranks * cap + n_packets;
    TimedLaunch tl(ctx, "wire_stamp", 32.0 * n_ranks * cap);  // (the slots scanned)
    hipLaunchKernelGGL(k_wire_stamp<1>, dim3(grid_for(most, WR_THREADS, (unsigned)ctx->n_cu * 8)), dim3(WR_THREADS), 0,
                       ctx->stream, (uint32_t*)send_padded, (uint32_t*)send, 0u, n_ranks, cap,
                       (const unsigned long long*)xrow, WireStamp{packet_id, len, id_base, n_packets});
    SG_CHECK_LAUNCH();
  });
}

int32_t sg_wire_push_records(sg_ctx* ctx, sg_wire* w, const sg_record* recv, uint32_t n_records,
                             const uint32_t* host_map, uint32_t n_hosts) {
  if (!w || (n_records && !recv)) return SG_ERR_INVALID_ARG;
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (w->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "the wire belongs to another context");
    if (!n_records) return;
    if (w->count + n_records > w->capacity)
      throw Error(SG_ERR_CAPACITY, "sg_wire_push_records: count + n_records exceeds the wire's capacity");
    SrcRecords s{(const uint4*)recv, host_map, &w->d.ctl->bad, n_records, n_hosts, w->n_hosts};
    {
      TimedLaunch tl(ctx, "wire_push", 0.0);  // the work (events x 32 B) is known at the next pop
      wire_append_launch(ctx, w, s, n_records);
    }
    w->count += n_records;
  });
}

int32_t sg_wire_push_records_padded(sg_ctx* ctx, sg_wire* w, const sg_record* recv_padded, uint32_t n_ranks,
                                    uint32_t cap, const uint64_t* xall, uint32_t rank, const uint32_t* host_map,
                                    uint32_t n_hosts) {
  if (!w || !recv_padded || !xall) return SG_ERR_INVALID_ARG;
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (w->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "the wire belongs to another context");
    if (n_ranks == 0 || n_ranks > WR_MAX_RANKS || rank >= n_ranks || cap == 0 ||
        (uint64_t)n_ranks * cap > 0xFFFFFFFFull)
      throw Error(SG_ERR_INVALID_ARG, "bad n_ranks / rank / cap");
    const uint32_t n = n_ranks * cap;
    // the counts stay on the device: every slot counts (conservative, as sg_wire_push's dropped packets)
    if (w->count + n > w->capacity)
      throw Error(SG_ERR_CAPACITY, "sg_wire_push_records_padded: count + n_ranks x cap exceeds the wire's capacity");
    uint32_t* valid = w->hbuf + 3 * (size_t)w->n_hosts + 2;
    SrcPaddedRecords s{SrcRecords{(const uint4*)recv_padded, host_map, &w->d.ctl->bad, n, n_hosts, w->n_hosts}, valid,
                       cap};
    {
      TimedLaunch tl(ctx, "wire_push", 0.0);
      hipLaunchKernelGGL(k_wire_padded_valid, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long*)xall,
                         n_ranks, rank, cap, valid);
      wire_append_launch(ctx, w, s, n);
    }
    w->count += n;
  });
}

int32_t sg_wire_pop(sg_ctx* ctx, sg_wire* w, uint64_t window_end_ns, sg_wire_arrivals* out, uint32_t* n_out,
                    uint64_t* next_time_ns) {
  if (!w || !out || !n_out) return SG_ERR_INVALID_ARG;
  return sg::guarded(ctx, [&] {
    using namespace sg;
    if (w->ctx != ctx) throw Error(SG_ERR_INVALID_ARG, "the wire belongs to another context");
    *n_out = 0;
    const uint32_t cap = out->cap, H = w->n_hosts;
    if (cap && (!out->host || !out->time_ns || !out->packet || !out->len))
      throw Error(SG_ERR_INVALID_ARG, "null arrival array");
    if ((out->src_host == nullptr) != (out->event_id == nullptr))
      throw Error(SG_ERR_INVALID_ARG, "src_host and event_id go together");
    hipStream_t st = ctx->stream;
    uint32_t *hcnt = w->hbuf, *hcur = hcnt + H + 1, *hoff = hcur + H;
    const size_t scap = std::max<uint32_t>(cap, 1);
    uint4* stage = ctx->d_keys.get<uint4>(2 * scap);
    uint4* stage2 = ctx->d_keys2.get<uint4>(2 * scap);
    const uint32_t work_cap = cap / WR_RANK_SORT_MAX + 1;
    uint2* work = ctx->d_lists.get<uint2>(work_cap);
    WireOut o{out->host, (unsigned long long*)out->time_ns, out->packet, out->len, out->src_host,
              (unsigned long long*)out->event_id};
    const unsigned G = (unsigned)ctx->n_cu * 4;
    {
      TimedLaunch tl(ctx, "wire_pop", 0.0);
      SG_HIP(hipMemsetAsync(hcnt, 0, (2 * (size_t)H + 1) * 4, st));
      hipLaunchKernelGGL(k_wire_plan, dim3(1), dim3(1024), 0, st, w->d, w->plan, (unsigned long long)window_end_ns);
      hipLaunchKernelGGL(k_wire_popcount, dim3(G), dim3(WR_THREADS), 0, st, w->d, w->plan, hcnt, H);
      exclusive_scan_u32(ctx, hcnt, hoff, H);
      hipLaunchKernelGGL(k_wire_commit, dim3(1), dim3(1024), 0, st, w->d, w->plan, cap);
      hipLaunchKernelGGL(k_wire_move<0>, dim3(G), dim3(WR_THREADS), 0, st, w->d, w->plan, hoff, hcur, H, stage, cap);
      hipLaunchKernelGGL(k_wire_mid, dim3(1), dim3(1024), 0, st, w->d, w->plan);
      hipLaunchKernelGGL(k_wire_move<1>, dim3(G), dim3(WR_THREADS), 0, st, w->d, w->plan, hoff, hcur, H, stage, cap);
      hipLaunchKernelGGL(k_wire_final, dim3(1), dim3(1024), 0, st, w->d, w->plan, w->ret);
      hipLaunchKernelGGL(k_wire_sort_small, dim3(grid_for((size_t)H * 64, WR_THREADS, (unsigned)ctx->n_cu * 16)),
                         dim3(WR_THREADS), 0, st, w->plan, hoff, H, stage, o, work, work_cap);
      hipLaunchKernelGGL(k_wire_sort_lds, dim3(G), dim3(WR_THREADS), 0, st, w->plan, hoff, stage, stage2, o, work,
                         work_cap);
      hipLaunchKernelGGL(k_wire_merge, dim3(G), dim3(WR_THREADS), 0, st, w->plan, hoff, stage2, o, work, work_cap);
      SG_CHECK_LAUNCH();
    }
    SG_HIP(hipStreamSynchronize(st));
    const volatile WireRet* r = w->ret;
    const uint32_t v = r->verdict, due = r->due, err = r->err;
    timer_add_work(ctx, "wire_push", 32.0 * (double)r->pushed);
    if (v == WV_ERR && (err & WE_BADDST))
      throw Error(SG_ERR_INVALID_ARG, "sg_wire_push_records: a record's dst_host is outside host_map (n_hosts), or "
                                      "maps to no host of this wire; the store is incomplete");
    if (v == WV_ERR) throw Error(SG_ERR_CAPACITY, "sg_wire: an earlier push found the arena without room; "
                                                  "the store is incomplete (raise capacity or n_bins)");
    w->count = r->held;
    if (v == WV_CAP) {
      *n_out = due;
      throw Error(SG_ERR_CAPACITY, "sg_wire_pop: " + std::to_string(due) + " events are due, out->cap is " +
                                       std::to_string(cap));
    }
    if (v == WV_ARENA)
      throw Error(SG_ERR_CAPACITY, "sg_wire_pop: no room in the arena to re-bin the far list "
                                   "(raise capacity, or n_bins x bin_ns past the largest latency)");
    *n_out = due;
    if (next_time_ns) *next_time_ns = r->next;
    timer_add_work(ctx, "wire_pop", 32.0 * due);
    if (r->compact_row != ~0u) {
      // the straddling row has gathered tombstones: fill them from its tail (asynchronous)
      const uint32_t row = r->compact_row, c = r->compact_cnt, keep = r->compact_keep;
      const uint32_t h_max = std::min(keep, c - keep);
      uint32_t* ws = ctx->d_lists2.get<uint32_t>(2 * (size_t)h_max + 2);
      uint32_t *holes = ws + 2, *movers = holes + h_max;
      TimedLaunch tc(ctx, "wire_compact", 32.0 * h_max);
      SG_HIP(hipMemsetAsync(ws, 0, 8, st));
      hipLaunchKernelGGL(k_wire_compact_list, dim3(grid_for(c, WR_THREADS, G)), dim3(WR_THREADS), 0, st, w->d, row, c,
                         keep, ws, holes, movers, h_max);
      hipLaunchKernelGGL(k_wire_compact_move, dim3(grid_for(h_max, WR_THREADS, G)), dim3(WR_THREADS), 0, st, w->d, row,
                         ws, holes, movers, h_max);
      hipLaunchKernelGGL(k_wire_compact_finish, dim3(1), dim3(1024), 0, st, w->d, row, c, keep, ws, h_max);
      SG_CHECK_LAUNCH();
    }
    // The sharded round's synchronisation is this one: a padded source phase's batch errors
    // (sg_deliver_source_padded reads nothing back) are reported here, as sg_deliver_bucket_padded
    // reports them on the path without a wire.  The pop itself is complete: *n_out and out hold.
    report_round_flags(ctx);
  });
}

int32_t sg_wire_get_state(sg_wire* w, uint64_t cap, sg_wire_state* out, uint64_t* n) {
  if (!w || !n) return SG_ERR_INVALID_ARG;
  return sg::guarded(w->ctx, [&] {
    using namespace sg;
    sg_ctx* ctx = w->ctx;
    hipStream_t st = ctx->stream;
    const WireDev& d = w->d;
    WireCtl ctl;
    std::vector<uint32_t> cnt(d.R);
    SG_HIP(hipMemcpyAsync(&ctl, d.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(cnt.data(), d.cnt, (size_t)d.R * 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (ctl.err & WE_BADDST)
      throw Error(SG_ERR_INVALID_ARG, "sg_wire_push_records: a record's dst_host is outside host_map (n_hosts), or "
                                      "maps to no host of this wire; the store is incomplete");
    if (ctl.err) throw Error(SG_ERR_CAPACITY, "sg_wire: an earlier push found the arena without room");
    w->count = ctl.held;
    *n = ctl.held;
    if (ctl.held > cap) throw Error(SG_ERR_CAPACITY, "sg_wire_get_state: the arrays are too small");
    if (!ctl.held) return;
    if (!out || !out->host || !out->src_host || !out->packet || !out->len || !out->time_ns || !out->event_id)
      throw Error(SG_ERR_INVALID_ARG, "null state array");
    struct HRec {
      uint64_t time, eid;
      uint32_t src, dst, packet, len;
    };
    // one gather on the device into a contiguous buffer (tombstones left behind), one copy
    std::vector<uint32_t> off(d.R + 1, 0);
    for (uint32_t r = 0; r < d.R; r++) off[r + 1] = off[r] + cnt[r];
    DevBuf ws, dense;
    uint32_t* d_off = ws.get<uint32_t>((size_t)d.R + 2);
    uint4* d_out = dense.get<uint4>(2 * (size_t)ctl.held);
    SG_HIP(hipMemcpyAsync(d_off + 1, off.data(), ((size_t)d.R + 1) * 4, hipMemcpyHostToDevice, st));
    SG_HIP(hipMemsetAsync(d_off, 0, 4, st));
    hipLaunchKernelGGL(k_wire_gather, dim3(grid_for(off[d.R], WR_THREADS, (unsigned)ctx->n_cu * 4)), dim3(WR_THREADS),
                       0, st, d, d_off + 1, d_out, d_off, (uint32_t)ctl.held);
    SG_CHECK_LAUNCH();
    std::vector<HRec> all(ctl.held);
    uint32_t got = 0;
    SG_HIP(hipMemcpyAsync(all.data(), d_out, (size_t)ctl.held * 32, hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(&got, d_off, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (got != ctl.held) all.clear();
    if (all.size() != ctl.held) throw Error(SG_ERR_DEVICE, "sg_wire: the rows do not hold the counted events");
    std::sort(all.begin(), all.end(), [](const HRec& a, const HRec& b) {
      if (a.dst != b.dst) return a.dst < b.dst;
      if (a.time != b.time) return a.time < b.time;
      if (a.src != b.src) return a.src < b.src;
      return a.eid < b.eid;
    });
    for (size_t i = 0; i < all.size(); i++) {
      out->host[i] = all[i].dst;
      out->src_host[i] = all[i].src;
      out->packet[i] = all[i].packet;
      out->len[i] = all[i].len;
      out->time_ns[i] = all[i].time;
      out->event_id[i] = all[i].eid;
    }
  });
}

int32_t sg_wire_set_state(sg_wire* w, uint64_t n, const sg_wire_state* in) {
  if (!w) return SG_ERR_INVALID_ARG;
  return sg::guarded(w->ctx, [&] {
    using namespace sg;
    sg_ctx* ctx = w->ctx;
    hipStream_t st = ctx->stream;
    if (n > w->capacity) throw Error(SG_ERR_CAPACITY, "sg_wire_set_state: more events than the wire's capacity");
    if (n && (!in || !in->host || !in->src_host || !in->packet || !in->len || !in->time_ns || !in->event_id))
      throw Error(SG_ERR_INVALID_ARG, "null state array");
    std::vector<uint4> recs(2 * (size_t)n);
    for (uint64_t i = 0; i < n; i++) {
      if (in->host[i] >= w->n_hosts) throw Error(SG_ERR_INVALID_ARG, "event host out of range");
      if (in->time_ns[i] == WR_TOMB) throw Error(SG_ERR_INVALID_ARG, "event time past EMUTIME_MAX");
      const uint64_t t = in->time_ns[i], e = in->event_id[i];
      recs[2 * i] = make_uint4((uint32_t)t, (uint32_t)(t >> 32), (uint32_t)e, (uint32_t)(e >> 32));
      recs[2 * i + 1] = make_uint4(in->src_host[i], in->host[i], in->packet[i], in->len[i]);
    }
    wire_reset(ctx, w);
    if (n) {
      DevBuf tmp;
      uint4* d_recs = tmp.get<uint4>(2 * (size_t)n);
      SG_HIP(hipMemcpyAsync(d_recs, recs.data(), (size_t)n * 32, hipMemcpyHostToDevice, st));
      wire_append_launch(ctx, w, SrcArray{d_recs, (uint32_t)n}, (uint32_t)n);
      SG_HIP(hipStreamSynchronize(st));
    }
    WireCtl ctl;
    SG_HIP(hipMemcpyAsync(&ctl, w->d.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (ctl.err) throw Error(SG_ERR_CAPACITY, "sg_wire_set_state: no room in the arena");
    w->count = ctl.held;
  });
}

}  // extern "C"
