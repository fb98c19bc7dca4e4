// sg_group.hip -- a device group: N contexts of ONE process behind one object.
//
// Shadow is one process.  Manager::run spawns worker threads (manager.rs:254-261), a packet
// crosses hosts through an in-process push (worker.rs:597-607), and running as several
// processes is a TODO in the reference (worker.rs:375-376).  sg_comm.hip's collectives need one
// process per GPU and a channel between them for the RCCL id; a group needs neither: its
// members are sg_ctx of the calling process ("member m" = "rank m" of the sharded paths), and
//   * sg_group_routing_info_fill builds one host RoutingInfo from all members at once: member
//     m runs sg_routing.hip's fill_rows over its row range on a host thread of its own (each
//     with its member's device current), every member copying into its own rows of the
//     object's pinned cells -- N PCIe links instead of one when the members sit on N devices;
//   * sg_group_exchange_padded is the fixed-split round's exchange as a pull: one launch of
//     k_group_pull per owner, on the owner's stream, reads block r of every member's
//     send_padded (peer memory when the member sits on another device) and every member's
//     [stats, counts] row; no count leaves the device and the host sizes nothing;
//   * sg_group_alltoallv_records is the exact exchange as n x n device copies.
//
// Ordering of an exchange: events only, all enqueued by the one calling thread.
//   1. "sent" is recorded on every member's stream;
//   2. every owner's stream waits for all n of them, runs its pull (or copies), records "pulled";
//   3. every member's stream waits for all n "pulled": what the caller enqueues next on a
//      source's stream (the next round's source phase, which overwrites send_padded) runs after
//      every peer has read the blocks.
// Every event is recorded before any wait on it is enqueued, so the dependence graph has no
// cycle whatever the members' order.  The events are created with hipEventDisableTiming alone:
// no flag that drops the release at the record, which is what makes a source kernel's stores
// visible to a pull on another device.
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "sg_internal.h"

// (struct sg_group, group_guarded and set_device: sg_internal.h, shared with sg_group_trace.hip)

namespace sg {

// (GROUP_MAX: sg_internal.h)
constexpr int PULL_THREADS = 256;
constexpr int PULL_UNROLL = 4;  // 16-byte loads in flight per thread

// The members' pointers, by value in the kernel's argument block (1 KiB).  The kernel indexes
// them by a run-time member number straight out of the argument segment, which is memory: no
// local copy exists that could go to scratch, and the loads through them stay global loads.
struct PullArgs {
  const uint4* send[GROUP_MAX];     // member b's send_padded
  const uint64_t* xrow[GROUP_MAX];  // member b's [stats, counts] row (3 + n u64)
};

// Owner r's side of the fixed-split exchange.  Every workgroup reads the n counts for r into
// LDS (clamped to cap); the grid then copies the n rows into xall and the valid records of
// block r of every member into recv, two 16-byte words per 32-byte record.  Plain vector loads
// and stores; slots past a block's count are not touched.  2 cap < 2^31 (checked by the host).
__global__ void __launch_bounds__(PULL_THREADS) k_group_pull(PullArgs a, uint32_t n, uint32_t r, uint32_t cap,
                                                             uint4* __restrict__ recv, uint64_t* __restrict__ xall) {
  __shared__ uint32_t s_words[GROUP_MAX];  // 16-byte words to copy from member b: 2 min(count, cap)
  const uint32_t tid = threadIdx.x;
  if (tid < n) {
    const uint64_t c = a.xrow[tid][3 + r];
    s_words[tid] = 2u * (uint32_t)(c < cap ? c : cap);
  }
  __syncthreads();
  const uint32_t w = 3 + n;
  const uint32_t gtid = blockIdx.x * PULL_THREADS + tid, gsize = gridDim.x * PULL_THREADS;
  for (uint32_t i = gtid; i < n * w; i += gsize) xall[i] = a.xrow[i / w][i % w];
  for (uint32_t b = 0; b < n; b++) {
    const uint4* __restrict__ src = a.send[b] + 2ull * r * cap;
    uint4* __restrict__ dst = recv + 2ull * b * cap;
    const uint32_t words = s_words[b];
    uint32_t i = gtid;
    for (; i + (PULL_UNROLL - 1) * gsize < words; i += PULL_UNROLL * gsize) {  // PULL_UNROLL loads in flight
      uint4 v[PULL_UNROLL];
#pragma unroll
      for (int u = 0; u < PULL_UNROLL; u++) v[u] = src[i + u * gsize];
#pragma unroll
      for (int u = 0; u < PULL_UNROLL; u++) dst[i + u * gsize] = v[u];
    }
    for (; i < words; i += gsize) dst[i] = src[i];
  }
}

static thread_local std::string g_group_create_error;

// Steps 1 and 2's waits, then `work(r)` on every owner's stream, then steps 2's record and 3.
template <class F>
static void exchange_ordered(sg_group* g, F&& work) {
  const uint32_t n = (uint32_t)g->ctxs.size();
  for (uint32_t m = 0; m < n; m++) {
    set_device(g->ctxs[m]);
    SG_HIP(hipEventRecord(g->sent[m], g->ctxs[m]->stream));
  }
  for (uint32_t r = 0; r < n; r++) {
    sg_ctx* c = g->ctxs[r];
    set_device(c);
    for (uint32_t m = 0; m < n; m++)
      if (m != r) SG_HIP(hipStreamWaitEvent(c->stream, g->sent[m], 0));  // (its own: stream order)
    work(r);
    SG_HIP(hipEventRecord(g->pulled[r], c->stream));
  }
  for (uint32_t m = 0; m < n; m++) {
    sg_ctx* c = g->ctxs[m];
    set_device(c);
    for (uint32_t r = 0; r < n; r++)
      if (r != m) SG_HIP(hipStreamWaitEvent(c->stream, g->pulled[r], 0));
  }
}

static void destroy_group(sg_group* g) {
  for (size_t m = 0; m < g->ctxs.size(); m++) {
    (void)hipSetDevice(g->ctxs[m]->device);
    if (m < g->sent.size() && g->sent[m]) (void)hipEventDestroy(g->sent[m]);
    if (m < g->pulled.size() && g->pulled[m]) (void)hipEventDestroy(g->pulled[m]);
  }
  delete g;
}

}  // namespace sg

extern "C" {

int32_t sg_group_create(sg_ctx** ctxs, uint32_t n, sg_group** out) {
  using namespace sg;
  if (out) *out = nullptr;
  if (!ctxs || !out || n == 0 || n > GROUP_MAX) {
    g_group_create_error = "sg_group_create: null argument, or a member count outside 1 .. 64";
    return SG_ERR_INVALID_ARG;
  }
  for (uint32_t m = 0; m < n; m++) {
    if (!ctxs[m]) {
      g_group_create_error = "sg_group_create: member " + std::to_string(m) + " is NULL";
      return SG_ERR_INVALID_ARG;
    }
    for (uint32_t k = 0; k < m; k++)
      if (ctxs[k] == ctxs[m]) {
        g_group_create_error = "sg_group_create: members " + std::to_string(k) + " and " + std::to_string(m) +
                               " are the same context";
        return SG_ERR_INVALID_ARG;
      }
  }
  sg_group* g = new (std::nothrow) sg_group();
  if (!g) return SG_ERR_OOM;
  int prev = 0;
  (void)hipGetDevice(&prev);
  int32_t rc = SG_OK;
  try {
    g->ctxs.assign(ctxs, ctxs + n);
    g->sent.assign(n, nullptr);
    g->pulled.assign(n, nullptr);
    // peer access between every pair of distinct devices, both ways
    std::vector<int> devs;
    for (uint32_t m = 0; m < n; m++)
      if (std::find(devs.begin(), devs.end(), ctxs[m]->device) == devs.end()) devs.push_back(ctxs[m]->device);
    for (int a : devs)
      for (int b : devs) {
        if (a == b) continue;
        int can = 0;
        SG_HIP(hipDeviceCanAccessPeer(&can, a, b));
        if (!can)
          throw Error(SG_ERR_UNSUPPORTED,
                      "device " + std::to_string(a) + " cannot access device " + std::to_string(b) + "'s memory",
                      (uint32_t)a, (uint32_t)b);
        SG_HIP(hipSetDevice(a));
        const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
        if (e == hipErrorPeerAccessAlreadyEnabled)
          (void)hipGetLastError();
        else if (e != hipSuccess)
          throw Error(SG_ERR_UNSUPPORTED,
                      "device " + std::to_string(a) + " could not enable access to device " + std::to_string(b) +
                          ": " + hipGetErrorString(e),
                      (uint32_t)a, (uint32_t)b);
      }
    for (uint32_t m = 0; m < n; m++) {
      SG_HIP(hipSetDevice(ctxs[m]->device));
      SG_HIP(hipEventCreateWithFlags(&g->sent[m], hipEventDisableTiming));
      SG_HIP(hipEventCreateWithFlags(&g->pulled[m], hipEventDisableTiming));
    }
  } catch (const Error& e) {
    g_group_create_error = e.what();
    rc = e.code;
  } catch (const std::exception& e) {
    g_group_create_error = e.what();
    rc = SG_ERR_OOM;
  }
  (void)hipSetDevice(prev);
  if (rc != SG_OK) {
    destroy_group(g);
    return rc;
  }
  *out = g;
  return SG_OK;
}

void sg_group_destroy(sg_group* g) {
  if (!g) return;
  int prev = 0;
  (void)hipGetDevice(&prev);
  // the members' streams may still wait on the group's events
  for (sg_ctx* c : g->ctxs) {
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
  }
  sg::destroy_group(g);
  (void)hipSetDevice(prev);
}

uint32_t sg_group_size(const sg_group* g) { return g ? (uint32_t)g->ctxs.size() : 0; }

const char* sg_group_last_error(const sg_group* g) {
  return g ? g->last_error.c_str() : sg::g_group_create_error.c_str();
}

void sg_group_last_error_pair(const sg_group* g, uint32_t* row, uint32_t* col) {
  if (row) *row = g ? g->err_row : 0;
  if (col) *col = g ? g->err_col : 0;
}

uint32_t sg_group_last_error_member(const sg_group* g) { return g ? g->err_member : 0xFFFFFFFFu; }

int32_t sg_group_routing_info_fill(sg_group* g, sg_net** nets, const uint32_t* nodes, uint32_t flags,
                                   sg_routing_info* ri) {
  return sg::group_guarded(g, [&] {
    using namespace sg;
    const uint32_t n = (uint32_t)g->ctxs.size();
    if (!nets) throw Error(SG_ERR_INVALID_ARG, "null network list");
    if (!ri) throw Error(SG_ERR_INVALID_ARG, "null routing info");
    const uint32_t n_used = ri->n;
    if (n_used && !nodes) throw Error(SG_ERR_INVALID_ARG, "null node list");
    for (uint32_t m = 0; m < n; m++) {
      if (!nets[m] || nets[m]->ctx != g->ctxs[m])
        throw Error(SG_ERR_INVALID_ARG, "nets[" + std::to_string(m) + "] was not created on member " +
                                            std::to_string(m) + "'s context");
      if (nets[m]->n_nodes != nets[0]->n_nodes || nets[m]->n_edges != nets[0]->n_edges ||
          nets[m]->directed != nets[0]->directed)
        throw Error(SG_ERR_INVALID_ARG, "nets[" + std::to_string(m) + "] is not the graph of nets[0]");
    }
    check_node_list(nets[0], nodes, n_used);
    fill_reset(ri);
    if (n_used == 0) {
      ri->filled = true;
      return;
    }
    // a member's failure, as its context recorded it
    auto raise = [&](uint32_t m, int32_t rc) {
      const sg_ctx* c = g->ctxs[m];
      throw Error(rc, c->last_error, c->err_row, c->err_col);
    };
    // The self-loop check of every used node (graph/mod.rs:210-217), once, before any thread
    // starts: its error wins over any search's, as in the single fill.
    if (flags & SG_ROUTE_SHORTEST_PATH) {
      FillRows none;
      const int32_t rc = guarded(g->ctxs[0], [&] { fill_rows(g->ctxs[0], nets[0], nodes, flags, ri, 0, 0, 64, true, &none); });
      if (rc != SG_OK) raise(0, rc);
    }
    // member m's rows: shadow_amd.dist.row_range
    const uint64_t per = ((uint64_t)n_used + n - 1) / n;
    struct Member {
      uint32_t r0 = 0, r1 = 0;
      int32_t rc = SG_OK;
      FillRows out;
    };
    std::vector<Member> mem(n);
    uint32_t active = 0;
    for (uint32_t m = 0; m < n; m++) {
      mem[m].r0 = (uint32_t)std::min<uint64_t>(m * per, n_used);
      mem[m].r1 = (uint32_t)std::min<uint64_t>((m + 1) * per, n_used);
      active += mem[m].r1 > mem[m].r0;
    }
    // blocks of half the member's rows: the pack and the copy of one overlap the next one's build
    auto run = [&](uint32_t m) {
      Member& x = mem[m];
      x.rc = guarded(g->ctxs[m], [&] {
        fill_rows(g->ctxs[m], nets[m], nodes, flags, ri, x.r0, x.r1, (x.r1 - x.r0 + 1) / 2, false, &x.out);
      });
    };
    std::vector<std::thread> threads;
    struct Join {  // every thread is joined on every path
      std::vector<std::thread>& t;
      ~Join() {
        for (auto& th : t)
          if (th.joinable()) th.join();
      }
    };
    {
      Join join{threads};
      threads.reserve(n);
      for (uint32_t m = 0; m < n; m++) {
        if (mem[m].r1 <= mem[m].r0) continue;
        if (active == 1)
          run(m);  // one member with rows: on the calling thread
        else
          threads.emplace_back(run, m);
      }
    }
    // The error one context would have reported: the first failing pair in row-major order.
    int bad = -1;
    for (uint32_t m = 0; m < n; m++) {
      if (mem[m].rc == SG_OK) continue;
      const sg_ctx* c = g->ctxs[m];
      if (bad < 0 || std::make_pair(c->err_row, c->err_col) <
                         std::make_pair(g->ctxs[bad]->err_row, g->ctxs[bad]->err_col))
        bad = (int)m;
    }
    if (bad >= 0) raise((uint32_t)bad, mem[bad].rc);
    uint64_t min_lat = UINT64_MAX;
    std::vector<sg_routing_info::Wide> wide;
    for (const Member& x : mem) {
      min_lat = std::min(min_lat, x.out.min_lat);
      wide.insert(wide.end(), x.out.wide.begin(), x.out.wide.end());
    }
    fill_finish(ri, min_lat, std::move(wide));
  });
}

int32_t sg_group_exchange_padded(sg_group* g, const sg_record** send_padded, sg_record** recv_padded, uint32_t cap,
                                 const uint64_t** xrow, uint64_t** xall) {
  return sg::group_guarded(g, [&] {
    using namespace sg;
    static_assert(sizeof(sg_record) == 32, "k_group_pull moves a record as two 16-byte words");
    const uint32_t n = (uint32_t)g->ctxs.size();
    if (!xrow || !xall || (cap && (!send_padded || !recv_padded))) throw Error(SG_ERR_INVALID_ARG, "null argument");
    // (k_group_pull indexes a block's 2 cap 16-byte words, a few grid strides ahead, in 32 bits)
    if (cap >= (1u << 30)) throw Error(SG_ERR_INVALID_ARG, "cap must stay below 2^30");
    PullArgs a{};
    for (uint32_t m = 0; m < n; m++) {
      if (!xrow[m] || !xall[m] || (cap && (!send_padded[m] || !recv_padded[m])))
        throw Error(SG_ERR_INVALID_ARG, "null buffer of member " + std::to_string(m));
      a.send[m] = cap ? (const uint4*)send_padded[m] : nullptr;
      a.xrow[m] = xrow[m];
    }
    exchange_ordered(g, [&](uint32_t r) {
      sg_ctx* c = g->ctxs[r];
      // one launch per owner: at most two workgroups per CU, each thread PULL_UNROLL words per step
      const size_t items = std::max<size_t>((size_t)2 * n * cap, (size_t)n * (3 + n));
      const unsigned grid = grid_for((items + PULL_UNROLL - 1) / PULL_UNROLL, PULL_THREADS, 2u * (unsigned)c->n_cu);
      TimedLaunch t(c, "k_group_pull", 2.0 * 32.0 * n * cap);  // (bytes, at most)
      hipLaunchKernelGGL(k_group_pull, dim3(grid), dim3(PULL_THREADS), 0, c->stream, a, n, r, cap,
                         cap ? (uint4*)recv_padded[r] : nullptr, xall[r]);
      SG_CHECK_LAUNCH();
    });
  });
}

int32_t sg_group_alltoallv_records(sg_group* g, const sg_record** send, const uint32_t* counts, sg_record** recv) {
  return sg::group_guarded(g, [&] {
    using namespace sg;
    const uint32_t n = (uint32_t)g->ctxs.size();
    if (!send || !counts || !recv) throw Error(SG_ERR_INVALID_ARG, "null argument");
    std::vector<uint64_t> row(n, 0), col(n, 0);
    for (uint32_t b = 0; b < n; b++)
      for (uint32_t r = 0; r < n; r++) {
        row[b] += counts[(size_t)b * n + r];
        col[r] += counts[(size_t)b * n + r];
      }
    for (uint32_t m = 0; m < n; m++)
      if ((row[m] && !send[m]) || (col[m] && !recv[m]))
        throw Error(SG_ERR_INVALID_ARG, "null record buffer of member " + std::to_string(m));
    exchange_ordered(g, [&](uint32_t r) {
      sg_ctx* c = g->ctxs[r];
      size_t ro = 0;
      for (uint32_t b = 0; b < n; b++) {
        const size_t cnt = counts[(size_t)b * n + r];
        if (cnt) {
          size_t so = 0;
          for (uint32_t q = 0; q < r; q++) so += counts[(size_t)b * n + q];
          const int src_dev = g->ctxs[b]->device;
          if (src_dev == c->device)
            SG_HIP(hipMemcpyAsync(recv[r] + ro, send[b] + so, cnt * sizeof(sg_record), hipMemcpyDeviceToDevice,
                                  c->stream));
          else
            SG_HIP(hipMemcpyPeerAsync(recv[r] + ro, c->device, send[b] + so, src_dev, cnt * sizeof(sg_record),
                                      c->stream));
        }
        ro += cnt;
      }
    });
  });
}

}  // extern "C"
