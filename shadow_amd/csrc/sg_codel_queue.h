// sg_codel_queue.h -- one host's CoDel queue as the lane kernels walk it (sg_codel.hip: k_codel;
// sg_inbound.hip: k_inbound, with the relay behind it): the queue object, the per-host state in
// registers with its ring in HBM and its staged window in LDS (Q), and the kernels' arguments.
// Each translation unit gets its own copy of the device code (an unnamed namespace).
#pragma once

#include <cmath>

#include "sg_lanes.h"

struct sg_codel {
  sg_ctx* ctx = nullptr;
  uint32_t n = 0, cap = 0;
  uint8_t* flags = nullptr;
  uint64_t *iend = nullptr, *dnext = nullptr, *cur = nullptr, *prev = nullptr, *bytes = nullptr;
  uint32_t *head = nullptr, *tail = nullptr;
  uint4* ring = nullptr;  // per slot {packet, len, time lo, time hi}: one 16-B access per push / pop
  unsigned long long* ret = nullptr;  // pinned host-mapped: [dropped, error flags]
  ~sg_codel() {
    void* ps[] = {flags, iend, dnext, cur, prev, bytes, head, tail, ring};
    for (void* p : ps)
      if (p) (void)hipFree(p);
    if (ret) (void)hipHostFree(ret);
  }
};

namespace sg {
namespace {

// apply_control_law (codel_queue.rs:285-298): time + round(INTERVAL / sqrt(count)), f64
__device__ __forceinline__ uint64_t control_law(uint64_t t, uint64_t count) {
  const double s = count == 0 ? 1.0 : sqrt((double)count);
  return sat_add(t, (uint64_t)round((double)CD_INTERVAL / s));
}

// One host's queue (registers) + its ring (HBM).  The head element is also
// cached in registers (hp/ht/hl, valid while head < tail): a pop consumes the
// cache and issues the load of the next element right away, so its latency
// hides behind the events in between instead of stalling the next pop.
// LDS views (address space 3: ds_* instructions, not flat ones)
typedef __attribute__((address_space(3))) const uint32_t lds_u32;
typedef __attribute__((address_space(3))) const uint64_t lds_u64;

// PF: the kernel keeps the next chunk's loads in flight during the walk (k_codel<LM != 0>); the
// ring path then waits for its own load where it issues it -- where the ring and window paths
// join, the compiler otherwise waits for every vector-memory operation in flight (vmcnt(0)), the
// next chunk's loads included
// ORD (k_inbound<LM, true>, sg_inbound_run_ordered): an element pushed by this call carries
// ARR_BIT | its arrival index instead of the caller's packet id, and its fate is written at that
// index (arrival order: a host's outputs are consecutive) instead of at the packet id.  That is
// unambiguous because no packet id reaches a ring with the bit set: packet ids are below
// n_packets <= 2^31 (the host checks), an id at or past n_packets is refused when it is pushed
// (E_PKT) by the by-id call and when it would be left queued by the ordered one, and an index is
// checked against the call's arrivals before a fate is written at it (after a failed call, e.g.
// a ring overflow, the queue state is undefined but no write leaves the outputs)
constexpr uint32_t ARR_BIT = 0x80000000u;

template <bool PF = false, bool ORD = false>
struct Q {
  uint8_t flags;
  uint64_t iend, dnext, cur, prev, bytes;
  uint32_t head, tail;
  uint32_t hp, hl;
  uint64_t ht;
  bool hv;            // hp/hl/ht hold the element at head
  uint32_t last_len;  // length of the element pop_front returned last
  uint4* ring;
  uint32_t mask;
  // Staged window: the elements this host pushed since begin_window() are the
  // push events of its staged range, in order, so the head element is read
  // from LDS there instead of from the ring in HBM (the ring is still written:
  // what is left at the end of the window lives on in HBM).
  bool win;
  uint32_t t0, wb;  // tail at window start; host's first staged event
  lds_u32 *wp, *wl;
  lds_u64* wt;
  __device__ void begin_window(lds_u32* p, lds_u32* l, lds_u64* t, uint32_t first) {
    win = true;
    t0 = tail;
    wb = first;
    wp = p;
    wl = l;
    wt = t;
  }
  uint8_t* status;
  uint32_t n_status;
  uint64_t dropped;
  uint32_t err;
  uint8_t* astat;  // ORD: per arrival of this call
  uint64_t* afwd;
  uint32_t n_arr;  // ORD: the call's arrivals (the bound of astat / afwd)

  __device__ void drop(uint32_t pkt) {  // drop_packet -> RouterDropped
    if constexpr (ORD) {
      if (pkt & ARR_BIT) {
        if ((pkt & ~ARR_BIT) < n_arr) astat[pkt & ~ARR_BIT] = SG_CODEL_DROPPED;
        else err |= E_PKT;
        dropped++;
        return;
      }
    }
    if (pkt < n_status) status[pkt] = SG_CODEL_DROPPED;
    else err |= E_PKT;
    dropped++;
  }
  // process_standing_delay (codel_queue.rs:231-262)
  __device__ bool standing(uint64_t now, uint64_t sd) {
    if (sd < CD_TARGET || bytes <= CD_MTU) {
      flags &= (uint8_t)~F_IEND;
      return false;
    }
    if (flags & F_IEND) return now >= iend;
    iend = sat_add(now, CD_INTERVAL);
    flags |= F_IEND;
    return false;
  }
  // codel_pop / dodequeue (codel_queue.rs:204-227)
  __device__ bool pop_front(uint64_t now, uint32_t& pkt, bool& ok) {
    if (head == tail) {
      flags &= (uint8_t)~F_IEND;
      return false;
    }
    pkt = hp;
    last_len = hl;
    const uint64_t len = hl, ts = ht;
    head++;
    load_head();
    bytes = bytes > len ? bytes - len : 0;
    ok = standing(now, since(now, ts));
    return true;
  }
  __device__ void load_head() {
    hv = head != tail;
    if (!hv) return;
    const uint32_t j = head - t0;  // the j-th push of the window (modular)
    if (win && j < tail - t0) {
      const uint32_t k = wb + j;
      hp = wp[k];
      hl = wl[k];
      ht = wt[k];
      return;
    }
    const uint32_t slot = head & mask;
    const uint4 r = ring[slot];
    if constexpr (PF) __builtin_amdgcn_s_waitcnt(VMCNT0);
    hp = r.x;
    hl = r.y;
    ht = ((uint64_t)r.w << 32) | r.z;
  }
  static constexpr bool ord = ORD;
  __device__ bool should_drop(uint64_t now) const { return (flags & F_DNEXT) && now >= dnext; }
  __device__ bool dropping_recently(uint64_t now) const {
    return (flags & F_DNEXT) && since(now, dnext) < 16 * CD_INTERVAL;
  }
  // pop (codel_queue.rs:125-148), drop_from_store_mode (:150-170), drop_from_drop_mode (:172-201)
  __device__ uint32_t pop(uint64_t now) {
    uint32_t pkt;
    bool ok;
    if (!pop_front(now, pkt, ok)) {
      flags &= (uint8_t)~F_DROP;
      return CD_NONE;
    }
    if (!ok) {
      flags &= (uint8_t)~F_DROP;
      return pkt;
    }
    if (!(flags & F_DROP)) {
      drop(pkt);
      uint32_t nxt;
      bool nok;
      const bool has = pop_front(now, nxt, nok);
      flags |= F_DROP;
      const uint64_t delta = cur > prev ? cur - prev : 0;
      cur = (dropping_recently(now) && delta > 1) ? delta : 1;
      dnext = control_law(now, cur);
      flags |= F_DNEXT;
      prev = cur;
      return has ? nxt : CD_NONE;
    }
    bool has = true;
    while (has && (flags & F_DROP) && should_drop(now)) {
      drop(pkt);
      cur++;
      has = pop_front(now, pkt, ok);
      if (has && ok)
        dnext = control_law(dnext, cur);
      else
        flags &= (uint8_t)~F_DROP;
    }
    return has ? pkt : CD_NONE;
  }
};

struct CodelArgs {
  const uint32_t* host_off;
  uint32_t H, E;
  const uint8_t* kind;
  const uint64_t* time;
  const uint32_t* pkt;
  const uint32_t* len;
  uint8_t* flags;
  uint64_t *iend, *dnext, *cur, *prev, *bytes;
  uint32_t *head, *tail;
  uint4* ring;
  uint32_t cap;
  uint32_t* pop_result;
  uint8_t* status;
  uint32_t n_status;
  unsigned long long* blk;  // per block: [dropped, error flags]
  unsigned long long* bdiag = nullptr;  // SG_LANE_DIAG: per block [start, end, walk cycles, most events of a lane]
};

}  // namespace
}  // namespace sg
