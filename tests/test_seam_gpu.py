"""The table builds at the 2^32 ns seam of the searches' 32-bit keys (tests/seam_cases.py), under
the variants of each search that test_sweep_gpu.py does not set.  S = 2^32 - 1: a row whose
largest optimum is S - 1 or S - 2 must come exact out of the 32-bit search, a row with a cell of
exactly S, S + 1, ... must be redone in 64 bits.

Every variant builds the whole table and the case's qualified row block (test_seam_ref_cpu.py)
into poisoned device buffers, in an environment of its own, and every cell is compared with the
oracle (np.array_equal, losses by their bits).  The six small cases also run through every stage
in test_sweep_gpu.py, the two 600-node ones in test_sssp_chain_gpu.py.

SG_BUCKET_DELTA stays at 2 or more here: see the knob's row in sg_knobs.h.

Measured on an MI355X: the module's 11 tests take 3 s together, 1.6 s of it the context's set-up;
each test is under 0.1 s, but for 0.6 s where a test is the first of its process to launch the
bucketed search.
"""
import time

import numpy as np
import pytest

import seam_cases as SM
import sweep_cases as SC
from conftest import set_apsp_kernel

pytestmark = pytest.mark.gpu

SPARSE = [k for k in SM.SMALL if k not in SM.DENSE]
UNDIRECTED = [k for k in SM.SMALL if not SM.CASES[k][2]]


def _unit(name):
    return str(SM.UNIT[SM.CASES[name][4]])


def _lds_variants(name):
    """(kernel, environment, identity used list).  The small cases have 73-210 rows, fewer than a
    device has CUs: under "lds" they get no plan and a workgroup per row, so the knobs of the plan
    and of the launch shape are set under "lds_bounded" (SG_SSSP_SEEDS=2, SG_SSSP_FLAGGED=0: the
    phased plan, persistent workgroups claiming each phase's rows), where they act:
      SG_SSSP_BOUNDS 4, 8   bound rows per bounded search, in pairs past the second
      SG_SSSP_EXACT=0       the plan seeds bounds only, no exact keys through zero-loss arcs
      SG_SSSP_PERSIST=0     a workgroup per row under the plan (plan_ctl set, grid = rows)
      SG_BUILD_FUSED=0      the plan's bound rows ahead of phase 0, not beside it
    (The launch without a plan takes SG_SSSP_EXACT=0 and SG_SSSP_PERSIST=0 only past one row per
    CU: test_sssp_chain_gpu.py sets them on the 603-node cases.)  SG_APSP_DELTA acts on any launch.
    With an identity used list the output pass indexes the keys by column, not through the list,
    and a fused build leaves the list to the first kernel that reads it; SG_BUILD_FUSED=0 copies it."""
    v = [("lds_bounded", {"SG_SSSP_BOUNDS": "4"}, False), ("lds_bounded", {"SG_SSSP_BOUNDS": "8"}, False),
         ("lds_bounded", {"SG_SSSP_EXACT": "0"}, False), ("lds_bounded", {"SG_SSSP_PERSIST": "0"}, False),
         ("lds_bounded", {"SG_BUILD_FUSED": "0"}, False),
         ("lds", {"SG_APSP_DELTA": "1000"}, False),
         ("lds", {"SG_APSP_DELTA": "4194304"}, False),  # m + delta crosses 2^32 from the last 4 ms below it
         ("lds", {}, True), ("lds", {"SG_BUILD_FUSED": "0"}, True),
         ("lds_bounded", {}, True), ("lds_bounded", {"SG_BUILD_FUSED": "0"}, True)]
    return ([("lds_landmarks", {}, False)] if name in UNDIRECTED else []) + v


def _bucket_variants(name):
    """The default width is max(smallest arc, mean arc / 128).  On the "us" spur cases that is the
    mean's share (the 4.29 s spur arcs lift the mean to about 0.1-0.2 s), wider than the 1 us self-loops:
    the general kernel k_sssp_bucket.  On under_ms129 and across_ms129 the mean's share is
    0.2-0.4 ms, so the default is the smallest arc, 1 ms, and takes the exact-band kernel
    k_sssp_band as SG_BUCKET_DELTA = u does; there the general kernel runs under the widths of
    4,096 ns and 30 ms and under SG_BUCKET_MODE=queue."""
    u = _unit(name)
    return [("bucket", env, False) for env in (
        {},  # the default width
        {"SG_BUCKET_DELTA": u},  # exact bands
        {"SG_BUCKET_DELTA": "4096"}, {"SG_BUCKET_DELTA": "30000000"}, {"SG_BUCKET_MODE": "queue"},
        {"SG_BUCKET_RING": "2"}, {"SG_BAND_FILTER": "1", "SG_BUCKET_DELTA": u})]


def _dense_variants(name):
    return [("lds", env, False) for env in ({}, {"SG_DENSE_LAZY": "0"}, {"SG_APSP_DENSE": "0"}, {"SG_DENSE_SW": "4"})]


def _rows_device(net, used, r0, r1):
    import torch

    dlat = torch.full((r1 - r0, len(used)), -1, dtype=torch.int64, device="cuda")
    dloss = torch.full((r1 - r0, len(used)), -7.5, dtype=torch.float32, device="cuda")
    net.build_rows_device(used, r0, r1, dlat.data_ptr(), dloss.data_ptr())
    torch.cuda.synchronize()
    return dlat.cpu().numpy().view(np.uint64), dloss.cpu().numpy()


def _differences(got, r, nodes, rows):
    """The cells where a build differs from the oracle's rows, as text ('' when none)."""
    lat, loss = got
    bad = (lat != r["lat"]) | (loss.view(np.uint32) != r["loss"].view(np.uint32))
    if not bad.any():
        return ""
    i, j = (int(x[0]) for x in np.nonzero(bad))
    return (f"{int(bad.sum())} cells in {int(bad.any(1).sum())} rows, the first ({int(nodes[rows[0] + i])} -> {int(nodes[j])}): "
            f"({int(lat[i, j])}, {loss[i, j]!r}), want ({int(r['lat'][i, j])}, {r['loss'][i, j]!r}) = S{int(r['lat'][i, j]) - SM.S:+d}")


def _identity_views(n, nodes, r):
    """The whole table and the last third of its rows for the used list 0 .. n - 1, from the
    oracle's table over `nodes`: (used, rows, reference) each.  The added nodes are the last ones,
    so the block holds rows with a cell >= S beside rows without any."""
    at = nodes.astype(np.int64)
    lat, loss = np.empty_like(r["lat"]), np.empty_like(r["loss"])
    lat[np.ix_(at, at)], loss[np.ix_(at, at)] = r["lat"], r["loss"]
    used = np.arange(n, dtype=np.uint32)
    r0 = n - n // 3
    off = used[None, :] != used[r0:, None]
    wide = ((lat[r0:] >= SM.S) & off).any(1)
    assert wide.any() and not wide.all()
    return [(used, (0, n), dict(lat=lat, loss=loss)), (used, (r0, n), dict(lat=lat[r0:], loss=loss[r0:]))]


def _run(oracle, ctx, monkeypatch, name, variants):
    from shadow_amd import NetworkGraph

    c, rs = SC.case(name), SC.refs(oracle, name)
    g, nodes = c["g"], c["nodes"]
    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    views = [(nodes, v["rows"], r) for v, r in zip(c["views"], rs)]
    if any(ident for _, _, ident in variants):
        views_ident = _identity_views(g["n"], nodes, rs[0])
    failed = []
    t0 = time.perf_counter()
    for kernel, env, ident in variants:
        with monkeypatch.context() as m:  # a fresh environment per variant
            set_apsp_kernel(m, kernel)
            for k, x in env.items():
                m.setenv(k, x)
            for used, rows, r in (views_ident if ident else views):
                why = _differences(_rows_device(net, used, *rows), r, used, rows)
                if why:
                    failed.append(f"{kernel} {env}{', identity list' if ident else ''}, rows {rows}: {why}")
    print(f"{name}: {len(variants)} variants x 2 views in {time.perf_counter() - t0:.2f} s")
    assert not failed, "\n".join([name] + failed)


@pytest.mark.parametrize("name", SPARSE)
def test_lds_search_variants(oracle, ctx, monkeypatch, name):
    """The LDS search under the phased plan with landmarks (undirected), 4 and 8 bound rows, no
    exact seeds, a workgroup per row, and the bound rows ahead of phase 0; without a plan at
    bucket widths of 1 us and 4.19 ms; and on an identity used list, fused and not, with and
    without the plan.  _lds_variants says which path each reaches."""
    _run(oracle, ctx, monkeypatch, name, _lds_variants(name))


@pytest.mark.parametrize("name", SPARSE)
def test_bucketed_search_variants(oracle, ctx, monkeypatch, name):
    """The bucketed search at its default width, the banded one at the regime's unit (with and
    without the append filter), widths of 4,096 ns and 30 ms, the general kernel forced, a ring
    of two slots."""
    _run(oracle, ctx, monkeypatch, name, _bucket_variants(name))


@pytest.mark.parametrize("name", SM.DENSE)
def test_dense_search_variants(oracle, ctx, monkeypatch, name):
    """The lazy dense search, the T-cut search, no dense search, four lanes per settled row."""
    assert SC.dense(SC.case(name)["g"])
    _run(oracle, ctx, monkeypatch, name, _dense_variants(name))


def test_host_table_fill(oracle, ctx, monkeypatch):
    """RoutingInfo.fill on spur_us63: the host table's 8-byte cells mark paths of S or more as
    wide; every cell decodes to the oracle's."""
    from shadow_amd import NetworkGraph, RoutingInfo

    set_apsp_kernel(monkeypatch, "lds")
    c, r = SC.case("spur_us63"), SC.refs(oracle, "spur_us63")[0]
    g, nodes = c["g"], c["nodes"]
    net = NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)
    ri = RoutingInfo(nodes.tolist())
    ri.cells[...] = np.uint64(0x5A5A5A5A5A5A5A5A)
    ri.fill(net, nodes, True)
    why = _differences(ri.rows(), r, nodes, (0, g["n"]))
    assert not why, why
    assert ri.get_smallest_latency_ns() == int(r["lat"].min())
