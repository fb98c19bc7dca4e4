"""tools/sssp_queue_model.py, the CPU model of the LDS search's work queue: whatever the policy
(claim rule, lane or arc-parallel step, the kernel's threshold), a row ends at the oracle's keys,
from infinity and from its bounded start."""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_every_policy_ends_at_the_oracles_rows(oracle):
    import sssp_queue_model as M
    from shadow_amd import synth

    n = 300
    g = synth.ring_chords_graph(n, 6.0, seed=3)
    used = np.arange(n, dtype=np.uint32)
    rc, olat, oloss, _ = oracle.shortest_paths(n, g["src"], g["dst"], g["lat"], g["loss"], g["directed"], used,
                                               rows=(0, n), threads=4)
    assert rc == 0
    seen = []

    def check(s, key):
        other = np.arange(n) != s  # (the diagonal is the raw self-loop, not a key)
        assert np.array_equal((key >> np.uint64(31))[other], olat[s][other])
        assert np.array_equal((key & np.uint64(0x7FFFFFFF)).astype(np.uint32)[other], oloss[s].view(np.uint32)[other])
        seen.append(s)

    rows = [0, 7, 150, 299]
    out = io.StringIO()
    res = M.run(g, rows, M.Costs(), check=check, out=out)
    print(out.getvalue())
    assert len(res) == 7 and len(seen) == 7 * 2 * len(rows)
    # the same relaxations whatever the step costs: a policy changes the schedule, never the work rule
    for tot in res.values():
        assert tot[0]["pops"] > 0 and tot[1]["rel"] >= tot[0]["rel"]


def test_costs_from_a_diag_file(tmp_path):
    import sssp_queue_model as M

    p = tmp_path / "diag.txt"
    p.write_text("[sssp] per-wave cycles summed over a row's 16 waves: claim+wait 150000, pop 114000, steps 659000 "
                 "(per pop: 900, 5152)\n[sssp] delta 1 ns, 4096 rows: mean search 120621 cyc, output 15498 cyc, "
                 "128.0 wave pops, 0.0 buckets, 50044 relaxations (0.63 x arcs)\n"
                 "   1     161059   9.3%      4485648   0.6%      255151424   2.7%       1600\n"
                 "   2      71355   4.1%      6647196   0.9%      156907684   1.6%       2200\n"
                 " 5-8     779939  44.8%    373071800  50.2%     4505379300  47.2%       5780\n")
    c = M.Costs.from_diag(str(p))
    assert abs(c.fixed - (150000 / 128.0 + 900)) < 1e-6
    assert c.fit == (1000.0, 600.0)
    assert abs(c.l1 - (5780 - 500) / 8) < 1e-6
