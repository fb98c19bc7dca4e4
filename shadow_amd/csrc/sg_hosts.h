// sg_hosts.h -- the device-resident host table and its address map, shared by the translation
// units that resolve a packet's destination on the device (sg_deliver.hip; packet_item of
// sg_walks.h for sg_link.hip, sg_paths.hip and sg_trace.hip).
#pragma once

#include "sg_internal.h"

struct sg_hosts {
  sg_ctx* ctx = nullptr;
  uint32_t n = 0;
  uint32_t* route = nullptr;  // host -> routing-table index
  uint64_t* rng = nullptr;    // SoA [4][n]
  uint64_t* ctr = nullptr;    // n
  // address -> (host, routing index): dense window or sorted table (the pair
  // in one 8-byte entry, so resolving a destination is one dependent load)
  uint32_t ip_base = 0, dense_span = 0;
  uint2* dense = nullptr;
  uint32_t* sorted_ip = nullptr;
  uint2* sorted_host = nullptr;
  uint32_t max_route = 0;  // largest routing-table index of any host
  uint32_t min_route = 0;  // smallest (with max_route: a table shard holding every host's row needs no per-round check)
  ~sg_hosts() {
    void* ps[] = {route, rng, ctr, dense, sorted_ip, sorted_host};
    for (void* p : ps)
      if (p) (void)hipFree(p);
  }
};

namespace sg {

constexpr uint32_t NONE = ~0u;

struct HostMap {
  uint32_t ip_base, dense_span, n_sorted;
  const uint2* dense;
  const uint32_t* sorted_ip;
  const uint2* sorted_host;
  // Dns::addr_to_host_id (dns.rs:174-176): (host, its routing index), host = NONE if unknown
  __device__ __forceinline__ uint2 resolve(uint32_t ip) const {
    if (dense) {
      uint32_t off = ip - ip_base;
      return off < dense_span ? dense[off] : make_uint2(NONE, 0);
    }
    uint32_t lo = 0, hi = n_sorted;
    while (lo < hi) {
      uint32_t mid = (lo + hi) >> 1;
      if (sorted_ip[mid] < ip)
        lo = mid + 1;
      else
        hi = mid;
    }
    return (lo < n_sorted && sorted_ip[lo] == ip) ? sorted_host[lo] : make_uint2(NONE, 0);
  }
};

}  // namespace sg
