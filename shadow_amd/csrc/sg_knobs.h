// sg_knobs.h -- every SG_* environment knob of the library, and the only getenv calls for them.
//
// Plain C++ (sg_gml.cpp is built with g++).  A knob is read on every call that uses it: the
// tests change knobs between calls in one process, so nothing here or at a call site is cached.
// Each search reads its knobs into one small struct at the top of its launch function; the code
// below that point takes values, not names.
//
// The list: name | default | range | kind | what it is for.  Kinds: test = a hook the tests set
// to reach a path small graphs would not take; tune = a measured choice kept for A/B runs;
// diag = prints or times, never changes a result.  A default written as a formula depends on
// run-time values and is computed where the knob is read.  DESIGN.md's "Knobs" appendix has one
// row per entry (tests/test_knobs_cpu.py keeps the two, and the tests' own use, in step).
//
//   SG_APSP_LDS | 1 | 0, 1 | test | 0: every graph takes the batched-source slab search
//   SG_APSP_DENSE | 1 | 0, 1 | tune | 0: dense graphs skip the register-resident dense search
//   SG_APSP_BUCKET | -1 | -1, 0, 1 | test | 1: the bucketed search on any sparse graph; 0: never; -1: past the LDS search
//   SG_APSP_DELTA | 4294967295 | 1 .. 2^32-1 ns | test | bucket width of the LDS search (default: one bucket)
//   SG_APSP_FRONTIER | 1 | 0, 1 | test | slab: 0 relaxes every arc every pass
//   SG_APSP_B | dense ? 32 : 64 | 32, 64 | test | slab: sources per batch
//   SG_APSP_SPL | 2 | 1, 2 | test | slab: sources per lane (2: k_relax_w2)
//   SG_APSP_NPW | spl == 2 ? 4 : 8 | table | test | slab: destination nodes per wave item
//   SG_APSP_STAGE | spl == 2 ? 64 : 128 | table | test | slab: arcs staged per wave step
//   SG_APSP_GROUP | spl == 2 ? 3 : 8 | table | test | slab: row reads in flight
//   SG_APSP_GROUP_MB | 4096 | MiB | test | slab: device memory for the batches live together
//   SG_APSP_PASS_CHUNK | 4 | >= 1 | test | slab: passes issued per host read of the convergence flags
//   SG_APSP_SEG | arcs per node chunk / 1200 | 1 .. 16 | test | slab (spl 2): in-arc segments per relaxation item
//   SG_APSP_OUT_TPB | 1 | 1, 2, 4 | test | slab: column tiles per write-out block
//   SG_APSP_TRACE | 0 | 0, 1 | diag | slab: per-pass times on stderr
//   SG_SSSP_SEEDS | 1 | 0, 1, 2 | test | LDS search: 0 never plans, 2 always takes the phased plan
//   SG_SSSP_FLAGGED | -1 | -1, 0, 1 | test | LDS search: the one-launch flagged plan off / on (-1: row blocks of 6+ rows per CU)
//   SG_SSSP_PHASES | rows per CU >= 16 and no chained rows ? 3 : 2 | 2 .. 6 | tune | plan: phases
//   SG_SSSP_BOUNDS | 2 | 1 .. 8 | test | plan: bound rows per bounded search
//   SG_SSSP_EXACT | 1 | 0, 1 | tune | plan: exact seeds through zero-loss arcs
//   SG_SSSP_HOPS | 3 | 1 .. 3 | tune | plan: hops searched for bound rows
//   SG_SSSP_LANDMARKS | 0 | >= 0 | test | plan: landmark rows ahead of phase 0 (undirected graphs)
//   SG_SSSP_DIAG | 0 | 0, 1 | diag | LDS search: per-row cycle statistics on stderr (with counting timers)
//   SG_SSSP_CLAIM | 64 | 1 .. 64 | tune | LDS search: queue entries a wave claims at once
//   SG_SSSP_SLEEP | 0 | >= 0 | tune | LDS search: idle back-off, units of ~512 cycles
//   SG_SSSP_LANE_DEG | 64 | >= 0 | tune | LDS search: out-degree up to which a wave takes the lane path
//   SG_SSSP_STEP_ARCS | 256 | >= 0 | tune | LDS search: arcs up to which a pop takes the arc-parallel step sized to them (0: never)
//   SG_SSSP_PERSIST | 1 | 0, 1 | test | LDS search: 0 launches a workgroup per row
//   SG_SSSP_CHAIN | 1 | 0, 1 | tune | LDS search: 0 takes rows in list order, none seeded from the row the workgroup just finished
//   SG_SSSP_EARLY | 1 | 0, 1 | tune | LDS search: 0 ends every row's set-up before its search; 1 starts a chained row's search behind the LDS pass, its bound rows merged under it
//   SG_SSSP_SPIN_MAX | 4194304 | >= 1 | test | LDS and bucketed searches: spin budget per wave; small values make searches give up
//   SG_PLAN_DIAG | 0 | 0, 1 | diag | plan: phase sizes on stderr
//   SG_DENSE_LAZY | 1 | 0, 1 | test | dense: 0 takes the T-cut search with seed rows
//   SG_DENSE_THREADS | lazy ? 256 : 1024 | lazy: 256, 384, 512; T-cut: 512, 1024 | test | dense: threads per row
//   SG_DENSE_SW | lazy ? 8 : 64 | lazy: 4, 8, 16; T-cut: 8, 16, 32, 64 | test | dense: lanes per settled row
//   SG_DENSE_G | 2 | 2, 4 | test | dense (lazy): rows in flight per lane group
//   SG_DENSE_SPEC | 1 | 0, 1 | test | dense (lazy): relax whole chunks
//   SG_DENSE_RTN | 1 | 0, 1 | test | dense (lazy): the atomic's returned key instead of a settled-bit read
//   SG_DENSE_SPLIT | waves per row | 0 .. waves per row | test | dense (T-cut): rounds with fewer settled rows split each row over several waves
//   SG_DENSE_SEED | one level of n_cu rows | comma list of rows; 0: none | test | dense (T-cut): rows of the seed launches
//   SG_DENSE_SEED_THREADS | 512 | 512, 1024 | test | dense (T-cut): threads per row of the seeded launches
//   SG_DENSE_SEED_SW | 8 | 8, 16, 32, 64 | test | dense (T-cut): lanes per settled row of the seeded launches
//   SG_BUCKET_THREADS | 256 | 256, 1024 | test | bucketed search: threads per workgroup
//   SG_BUCKET_HASH | 1024 threads ? 12 : 11 | 6 .. 14 | test | bucketed / banded search: log2 of the hash slots; small tables give up
//   SG_BUCKET_CHUNKS | banded ? 384 : 1024 | 4 .. 65534 | test | bucketed / banded search: arena chunks per workgroup; small arenas give up
//   SG_BUCKET_DELTA | max(smallest arc, mean arc / 128) | 2 .. 2^32-1 ns | test | bucketed search: bucket width; a set value below 2 is taken as 2 (at 1 ns the bucket of latency 2^32 - 2 is the kernel's far-step sentinel)
//   SG_BUCKET_RING | 128 | 2 .. 128, a power of two | test | bucketed search: ring slots; small rings use the far lists
//   SG_BUCKET_MODE | unset | queue | test | bucketed search: queue forces the general kernel over the exact-band one
//   SG_BUCKET_PER_CU | 8 | >= 1 | tune | bucketed / banded search: workgroups per CU, at most
//   SG_BUCKET_STAGE | banded ? 0 : what the LDS leaves | bucketed: >= 0; banded: 0 .. 16 | test | bucketed / banded search: entries staged in LDS
//   SG_BUCKET_DIAG | 0 | 0, 1 | diag | bucketed search: per-row statistics on stderr (with counting timers)
//   SG_BAND_NPW | 448 / mean out-degree, in 16 .. 64 | 1 .. 64 | test | banded search: band nodes per wave
//   SG_BAND_FILTER | 0 | 0, 1 | test | banded search: the append filter
//   SG_BUCKET_REGION | 1 | 0, 1 | test | delivery: 0 keeps the scan path instead of region bucketing
//   SG_BUCKET_TWO_LEVEL | -1 | -1, 0, 1 | test | delivery: two-level scatter never / always (-1: past 512 super-buckets)
//   SG_LANE_MAJOR | 2 | 0, 1, 2 | test | lane kernels' chunk layout: contiguous, lane-major, by event count
//   SG_LANE_DIAG | 0 | 0, 1 | diag | lane kernels: per-block timing on stderr
//   SG_NET_THREADS | 4 | 1 .. 4 | test | graph upload: host threads staging a large edge list
//   SG_NET_LDS | 1 | 0, 1 | tune | graph upload: 0 counts and places arcs with global atomics at any size
//   SG_NET_TRACE | 0 | 0, 1 | diag | graph upload: host phases on stderr
//   SG_BUILD_FUSED | 1 | 0, 1 | tune | one-shot build: 0 copies an identity used list and keeps the plan's bound rows ahead of phase 0
//   SG_TREE_LDS | 1 | 0, 1 | test | shortest-path trees: 0 takes every row on the global path (keys read from the row in memory)
//   SG_LINK_LDS | 1 | 0, 1 | test | link loads: 0 takes every row on the global path (subtree sums and child counters in a scratch row)
//   SG_LINK_COMBINE | 1 | 0, 1 | tune | link loads from packets: 0 walks every packet on its own; 1 sums a wave's equal (row, column) pairs first, one lane walking per distinct pair
//   SG_LINK_TRACE_PIECE | 2048 | 64 .. 2048 | test | link trace: records of one piece of the LDS sort; small pieces take a few hundred records on a link to the merge tier
//   SG_LINK_SERIES_LDS | 4096 | 0 .. 8064 cells | tune | link time series: the most cells, n_slots x (n_bins + 2), a workgroup sums in an LDS matrix of its own; 0: never, every add goes to the matrix in memory
//   SG_LINK_QUEUE_SERIAL | 0 | 0, 1 | tune | link queues: 1 takes a lane per link looping over its segment instead of the flat segmented scan
//   SG_LINK_QUEUE_CARRY_ITERS | 4096 | 1 .. 2^31-1 | tune | link queues, carried form: the most iterations of the fixed point; reaching it is SG_ERR_CAPACITY
//   SG_LINK_QUEUE_PACKETS_INDEX | 0 | 0, 1 | tune | link queues, the first-order packet pass: 0 folds the records onto their packets with atomics; 1 builds the carried form's index of every packet's records first and sums each packet's list in one lane
//   SG_PATHS_STAGE | 1 | 0, 1 | tune | tree paths: 0 stores every hop record from its lane; 1 stages a wave's records in LDS and writes its span of the output with consecutive lanes
//   SG_PATHS_STAGE_HOPS | 640 | 1 .. 1536 | tune | tree paths: records a wave stages; a wave whose span is longer stores from its lanes
//   SG_RI_BLOCK_ROWS | n_used / 8; a group member: half its rows | >= 64, whole 64-row batches | test | RoutingInfo fill: rows per block
//   SG_GML_THREADS | min(hardware threads, 16) | >= 1 | tune | GML parser: threads
#pragma once

#include <climits>
#include <cstdlib>

namespace sg {

// the raw string, or null when unset
inline const char* knob_str(const char* name) { return getenv(name); }

// unset or empty: the default
inline int knob_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return s && *s ? atoi(s) : dflt;
}

// the value (or the default) clamped to [lo, hi]
inline int knob_int(const char* name, int dflt, int lo, int hi) {
  const int v = knob_int(name, dflt);
  return v < lo ? lo : v > hi ? hi : v;
}

inline double knob_double(const char* name, double dflt) {
  const char* s = getenv(name);
  return s && *s ? atof(s) : dflt;
}

// a set value raised to lo; unset or empty: the default as it is
inline double knob_double(const char* name, double dflt, double lo) {
  const char* s = getenv(name);
  if (!s || !*s) return dflt;
  const double v = atof(s);
  return v < lo ? lo : v;
}

// a knob whose value starts with '0' (off switches that were never parsed as numbers)
inline bool knob_off(const char* name) {
  const char* s = getenv(name);
  return s && s[0] == '0';
}

// SG_BUILD_FUSED (sg_routing.hip: the used list's upload, the LDS search's dispatch)
inline bool build_fused() { return knob_int("SG_BUILD_FUSED", 1) != 0; }

// SG_SSSP_SPIN_MAX, which the LDS and the bucketed search share
inline unsigned sssp_spin_max() { return (unsigned)knob_int("SG_SSSP_SPIN_MAX", 1 << 22, 1, INT_MAX); }

}  // namespace sg
