"""The relay model (relay_ref.py) and the boundary cases (relay_cases.py), checked on the CPU: the
model equals the oracle on every case in every form and on the random streams the GPU tests use,
and qdisc_ref.py where the two must agree; the cases reach every arm and every side of every
comparison; every single-site mutation of the model is caught by a named case in the output the
case names; and a few cases are worked by hand."""
import numpy as np
import pytest

import qdisc_cases as qc
import qdisc_ref
import relay_cases as rc
import relay_ref as ref
from shadow_amd import synth

T0, MS, I = rc.T0, rc.MS, rc.I
CH = {("i", False): 1024, ("o", False): 896, ("o", True): 512}   # the kernels' contiguous chunks
RUNS = [(env, d, keyed) for env in rc.ENVS for d, keyed in (("i", False), ("o", False), ("o", True))]


ring_cap = rc.ring_cap


# ---- 1. the model equals the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("form", rc.FORMS + ("single",))
@pytest.mark.parametrize("env,direction,keyed", RUNS)
def test_model_equals_oracle_on_cases(oracle, env, direction, keyed, form):
    """Fates, forward times, counters, the sent batch and the whole queue and relay state after every call."""
    cs = rc.of(env, direction, keyed)
    assert cs and (keyed or direction == "i" or len(cs) == len([c for c in rc.of(env, "o") if not c["keyed"]]))
    b = rc.build(cs, env, form, chunk=CH[direction, keyed])
    cap = ring_cap(direction, form)
    m, o = rc.ModelRun(b, direction, keyed=keyed, cap=cap), rc.OracleRun(oracle, b, direction, keyed, cap=cap)
    for j in range(len(b["calls"])):
        rc.same(m.call(j), o.call(j), (form, j))
    assert (m.status == 1).any()


def test_no_case_is_left_out():
    seen = {c["name"] for env, d, keyed in RUNS for c in rc.of(env, d, keyed)}
    assert seen == set(rc.NAMES) and len(rc.CASES) == len(rc.NAMES)
    fam = {c["family"] for c in rc.CASES}
    assert fam == {"refill", "remove", "wait", "inc", "sat", "due", "window", "end", "boot", "codel", "local", "tie", "rr"}
    assert sum(c["chunk"] for c in rc.CASES) >= 5


@pytest.mark.parametrize("env,direction,keyed", [r for r in RUNS if r[1] == "o"])
def test_model_equals_qdisc_ref_on_cases(env, direction, keyed):
    """Under both disciplines: fates, counters, the sent batch, the relay and the canonical interface state."""
    cs = rc.of(env, "o", keyed)
    b = rc.build(cs, env, "window")
    for qdisc in (ref.FIFO, ref.ROUND_ROBIN):
        m = rc.ModelRun(b, "o", qdisc=qdisc, keyed=keyed)
        q = qdisc_ref.Interfaces(b["ip"], b["bw"], 64, qdisc, 4)
        st, fw, ctr = np.zeros(b["n_pkt"], np.uint8), np.zeros(b["n_pkt"], np.uint64), np.zeros(len(b["bw"]), np.uint64)
        for j, (end, (host, t, pkt, ln, pay, dst, sock, eid, born)) in enumerate(b["calls"]):
            got = m.call(j)
            k = (eid, born) if keyed else (None, None)
            sent = q.run(host, t, pkt, ln, pay, dst, sock, end, b["boot"], b["sim_end"], ctr, fw, st, *k)
            want = rc.fates(st, fw, ctr)
            want.update({"sent_" + k: sent[k] for k in rc.SENT})
            want.update(q.relay_state())
            for k in want:
                assert np.array_equal(got[k], want[k]), (qdisc, j, k)
            if qdisc == ref.ROUND_ROBIN:
                assert got["queue"] == rc.qdisc_snapshot(q.qdisc_state(), q.relay_state(), q.S, q.cap)["queue"]


def test_round_robin_differs_from_fifo_where_the_case_says():
    c = rc.BY_NAME["rr/cached-socket-rotated"]
    b = rc.build([c], "main", "window")
    order = {}
    for qdisc in (ref.FIFO, ref.ROUND_ROBIN):
        m = rc.ModelRun(b, "o", qdisc=qdisc)
        order[qdisc] = [int(p) for j in range(len(b["calls"])) for p in m.call(j)["sent_packet"]]
    assert order[ref.FIFO] == [0, 1, 2, 3] and order[ref.ROUND_ROBIN] == [0, 1, 3, 2]


# ---- the random streams of the GPU tests (test_inbound_gpu.py, test_outbound_gpu.py), smaller ----------
def inbound_stream(bw_mbit, boot_ms, H=30, per=1200, windows=5):
    """test_inbound_gpu.py::test_windows_match_oracle's draw (there: 300 hosts, 12,000 per window)."""
    rng = np.random.default_rng(bw_mbit + boot_ms)
    W = 60 * MS
    bw = rng.integers(bw_mbit * 10**6 // 2, bw_mbit * 10**6 + 1, H).astype(np.uint64)
    calls = []
    for w in range(windows):
        t0, t1 = T0 + w * W, T0 + (w + 1) * W
        host = np.sort(rng.integers(0, H, per)).astype(np.uint32)
        t = np.sort(rng.integers(t0, t1, per)).astype(np.uint64)
        o = np.lexsort((t, host))
        host, t = host[o], t[o]
        ln = rng.choice(np.array([28, 1476, 600], np.uint32), per)
        pkt = np.arange(w * per, (w + 1) * per, dtype=np.uint32)
        z = np.zeros(per, np.uint32)
        calls.append((t1, (host, t, pkt, ln, z, z, z, np.zeros(per, np.uint64), np.zeros(per, np.uint64))))
    return dict(bw=bw, ip=np.zeros(H, np.uint32), calls=calls, n_pkt=windows * per, boot=T0 + boot_ms * MS,
                sim_end=T0 + 10**12)


def outbound_stream(bw_mbit, boot_ms, keyed, H=150, per=3000, windows=4):
    """test_outbound_gpu.py::test_windows_match_oracle's and test_same_time_ties_match_oracle's
    draws (there: 2,000 / 1,500 hosts, 40,000 / 30,000 sends per window of 2 ms)."""
    hosts = synth.make_hosts(H, 64, exact_seeds=False)
    rng = np.random.default_rng(bw_mbit + boot_ms)
    bw = rng.integers(bw_mbit * 10**6 // 2, bw_mbit * 10**6 + 1, H).astype(np.uint64)
    W, calls = 2 * MS, []
    for w in range(windows):
        t0, t1 = T0 + w * W, T0 + (w + 1) * W
        if keyed:
            host, t, ln, pay, dst, sock, eid, born = qc.keyed_sends(hosts, per, t0, t1, 50 * bw_mbit + w, 1)
        else:
            host, t, ln, pay, dst, sock = qc.sends(hosts, per, t0, t1, 100 * bw_mbit + w, 1)
            eid, born = np.full(per, ref.U64, np.uint64), np.zeros(per, np.uint64)
        pkt = np.arange(w * per, (w + 1) * per, dtype=np.uint32)
        calls.append((t1, (host, t, pkt, ln, pay, dst, sock, eid, born)))
    return dict(bw=bw, ip=hosts["ip"], calls=calls, n_pkt=windows * per, boot=T0 + boot_ms * MS, sim_end=T0 + 10**12)


STREAMS = [("i", False, (1000, 0)), ("i", False, (10, 0)), ("i", False, (1, 0)), ("i", False, (10, 40)),
           ("o", False, (1000, 0)), ("o", False, (10, 0)), ("o", False, (2, 0)), ("o", False, (10, 3)),
           ("o", True, (10, 0)), ("o", True, (2, 0))]


def _stream(direction, keyed, par):
    return inbound_stream(*par) if direction == "i" else outbound_stream(*par, keyed)


@pytest.mark.parametrize("direction,keyed,par", STREAMS)
def test_model_equals_oracle_on_random_streams(oracle, direction, keyed, par):
    b = _stream(direction, keyed, par)
    cap = 4096 if direction == "i" else 1024
    m, o = rc.ModelRun(b, direction, keyed=keyed, cap=cap), rc.OracleRun(oracle, b, direction, keyed, cap=cap)
    for j in range(len(b["calls"])):
        rc.same(m.call(j), o.call(j), j)
    assert (m.status == 1).any()


# ---- 2. coverage is a condition -----------------------------------------------------------------------
def test_cases_reach_every_arm_and_every_side():
    tin, tout = {}, {}
    for env, d, keyed in RUNS:
        cs = rc.of(env, d, keyed)
        b = rc.build(cs, env, "window")
        m = rc.ModelRun(b, d, keyed=keyed, trace=tin if d == "i" else tout)
        for j in range(len(b["calls"])):
            m.call(j)
    sides = lambda table: [n + ":" + s for n, ss in table.items() for s in ss.split()]
    want = list(ref.ARMS) + sides(ref.SIDES)
    assert [k for k in want if not tin.get(k)] == [], "inbound"
    want_out = want + list(ref.OUTBOUND_ARMS) + sides(ref.OUTBOUND_SIDES)
    assert [k for k in want_out if not tout.get(k)] == [], "outbound"
    assert [k for k in list(tin) + list(tout) if k not in want_out] == []   # ARMS and SIDES are complete


# ---- 3. the cases have teeth ----------------------------------------------------------------------------
def _outcome(c, variant, direction=None, qdisc=ref.FIFO):
    """One case alone, window form: the relay state as created, then its snapshot after every call
    (up to the call in which a mutant dies: a zero increment divides by zero)."""
    d = direction or ("i" if "i" in c["dirs"] else "o")
    b = rc.build([c], c["env"], "window")
    m = rc.ModelRun(b, d, qdisc=qdisc, keyed=c["keyed"], variant=variant)
    out = [m.created()]
    try:
        for j in range(len(b["calls"])):
            out.append(m.call(j))
    except (ValueError, ZeroDivisionError, AssertionError):
        pass
    return out


def _differs(a, b, key=None):
    """Some output (or the named one) differs after some call both lived through; without a name,
    dying early counts too."""
    if a is None or b is None:
        return a is not b
    if key is None and len(a) != len(b):
        return True
    for x, y in zip(a, b):
        for k in ([key] if key else x):
            if k not in x:
                continue
            if not (np.array_equal(x[k], y[k]) if isinstance(x[k], np.ndarray) else x[k] == y[k]):
                return True
    return False


def test_every_variant_is_killed_by_the_case_that_names_it():
    """A case's `kills` names the mutations it is there for and the output that shows each: that
    output differs (as created, or after some call) between the mutated model and the model -- an
    output the device has too, never the mutant's own failure.  Every entry of VARIANTS is named
    by some case."""
    named, blunt = {}, []
    for c in rc.CASES:
        want = _outcome(c, None)
        for v, key in c["kills"].items():
            if not _differs(_outcome(c, v), want, key):
                blunt.append((c["name"], v, key))
            named.setdefault(v, []).append(c["name"])
    assert blunt == []
    assert [v for v in ref.VARIANTS if v not in named] == []


def test_every_variant_changes_some_case():
    """The whole table: per variant the cases (either direction) whose outcome it changes."""
    print()
    alive = []
    truth = {(c["name"], d): _outcome(c, None, d) for c in rc.CASES for d in c["dirs"]}
    for v in ref.VARIANTS:
        killers = sorted({c["name"] for c in rc.CASES for d in c["dirs"] if _differs(_outcome(c, v, d), truth[c["name"], d])})
        print("%-24s killed by %3d cases, first %s" % (v, len(killers), killers[0] if killers else "-"))
        if not killers:
            alive.append(v)
    assert alive == []


def _stream_ends(b, direction, keyed, variant):
    cap = 4096 if direction == "i" else 1024
    try:
        m = rc.ModelRun(b, direction, keyed=keyed, cap=cap, variant=variant)
        return [m.call(j) for j in range(len(b["calls"]))]
    except (ValueError, ZeroDivisionError, AssertionError):
        return None


WINDOW_STREAMS = [x for x in STREAMS if not x[1]]   # test_windows_match_oracle's, inbound and outbound
TIE_STREAMS = [x for x in STREAMS if x[1]]          # test_same_time_ties_match_oracle's


def stream_survivors(which, scale=1, show=False):
    """The variants that the streams `which` do not notice, the mutated model against the model.
    scale 1 is a tenth of the GPU tests' hosts at their events per host, scale 10 their own size."""
    streams = []
    for d, keyed, par in which:
        b = _stream(d, keyed, par) if scale == 1 else (
            inbound_stream(*par, H=30 * scale, per=1200 * scale) if d == "i" else
            outbound_stream(*par, keyed, H=150 * scale, per=3000 * scale))
        streams.append((d, keyed, b, _stream_ends(b, d, keyed, None)))
    survive = []
    for v in ref.VARIANTS:
        hit = any(_differs(_stream_ends(b, d, keyed, v), truth) for d, keyed, b, truth in streams)
        if show:
            print("%-24s %s" % (v, "killed" if hit else "SURVIVES"))
        if not hit:
            survive.append(v)
    return survive


# What random traffic does not notice, at scale 1 (a tenth of the GPU tests' hosts, their events per host).
# test_windows_match_oracle's streams alone: the saturating arithmetic, the increment's floor of 1, sim_end
# (never inside a stream), a refill at a local packet, the keyed tie (they carry no keys) -- and, their times
# being drawn in ns, also Packet-before-Local at an arrival, now >= bootstrap_end and one id per same-time
# group.  The keyed streams of test_same_time_ties_match_oracle snap half their sends onto the refill grid
# and notice those three and two sides of the tie.  At the GPU tests' own size (scale 10, `python
# tests/test_relay_ref_cpu.py`, minutes) the window streams also notice tt<=arrival and group-id-per-arrival,
# and the set with the tie streams gains tie-ignores-id: AT_FULL_SIZE, not asserted here.
WINDOW_STREAMS_MISS = ("tokens-wrap", "bal+tokens-wraps", "inc-without-max", "tt<=arrival", "at>sim_end",
                       "never-takes-no-id", "now>boot", "group-id-per-arrival", "local-refills", "tie-ignores-id",
                       "tie-created<=", "tie-ignores-created")
ALL_STREAMS_MISS = ("tokens-wrap", "bal+tokens-wraps", "inc-without-max", "at>sim_end", "never-takes-no-id",
                    "local-refills", "tie-created<=")
AT_FULL_SIZE = {
    "windows": ("tokens-wrap", "bal+tokens-wraps", "inc-without-max", "at>sim_end", "never-takes-no-id", "now>boot",
                "local-refills", "tie-ignores-id", "tie-created<=", "tie-ignores-created"),
    "windows and ties": ALL_STREAMS_MISS + ("tie-ignores-id",)}


def test_which_variants_the_random_streams_miss():
    """For the record, exactly, at scale 1: the streams of test_windows_match_oracle, inbound and
    outbound, with the mutated model against the model; then with the keyed tie streams added.
    Every variant in either set is killed by a named case all the same."""
    assert tuple(stream_survivors(WINDOW_STREAMS)) == WINDOW_STREAMS_MISS
    assert tuple(stream_survivors(STREAMS)) == ALL_STREAMS_MISS
    assert set(ALL_STREAMS_MISS) <= set(WINDOW_STREAMS_MISS) <= set(ref.VARIANTS)


# ---- 4. a few cases by hand -----------------------------------------------------------------------------
def _hand(name, direction="i"):
    c = rc.BY_NAME[name]
    b = rc.build([c], c["env"], "window")
    m = rc.ModelRun(b, direction, keyed=c["keyed"])
    return [m.call(j) for j in range(len(b["calls"]))]


def _row(s, *keys):
    return tuple(int(s[k][0]) for k in keys)


@pytest.mark.parametrize("direction", ["i", "o"])
def test_by_hand_the_one_millisecond_span(direction):
    """refill/span=I-1, +0, +1.  inc 1,000, capacity 2,500, last = T0.  1,500 B at T0 + 5: span 5, no
    refill, 1,000 left.  Two 1,500-B packets at T0 + 1 ms + d.
    d = -1: span 999,999 < INTERVAL: no refill; 1,000 < 1,500: 500 short = one refill, 1 ns away:
    cached, task at T0 + 1 ms.  There span = 1,000,000: one refill, 2,000; the cached packet leaves
    500; the next is 1,000 short = one refill, INTERVAL - 0 away: task at T0 + 2 ms; there 1,500,
    it leaves 0.  Tasks: 0 (first packet), 1 (the group), 2 and 3 (wake-ups): counter 4.
    d = 0: span = INTERVAL exactly refills: the second leaves at T0 + 1 ms at once.  Counter 3.
    d = +1: the same at T0 + 1 ms + 1; the third waits INTERVAL - 1: T0 + 2 ms."""
    for d, fwd, ctr in ((-1, (T0 + 5, T0 + I, T0 + 2 * I), 4), (0, (T0 + 5, T0 + I, T0 + 2 * I), 3),
                        (1, (T0 + 5, T0 + I + 1, T0 + 2 * I), 3)):
        s = _hand(f"refill/span=I{d:+d}", direction)[0]
        assert tuple(s["fwd_time"].tolist()) == fwd and s["pkt_status"].tolist() == [1, 1, 1]
        assert _row(s, "event_ctr", "tb_bal", "tb_last", "rflags") == (ctr, 0, T0 + 2 * I, 0)


@pytest.mark.parametrize("direction", ["i", "o"])
def test_by_hand_the_ceiling(direction):
    """wait/need=100 and 101.  inc 100, capacity 1,600, emptied at T0 + 5; the packet at T0 + 10 is
    all deficit.  100 / 100 = 1 refill exactly: wait = the 999,990 ns to T0 + 1 ms, where 100 arrive
    and suffice.  101 = 1 refill and 1 B more: 2 refills, wait = 999,990 + 1,000,000: T0 + 2 ms,
    where 200 arrive and 99 stay.  Tasks 0, 1 and the wake-up: counter 3."""
    for need, at, left in ((100, T0 + I, 0), (101, T0 + 2 * I, 99)):
        s = _hand(f"wait/need={need}", direction)[0]
        assert s["fwd_time"].tolist() == [T0 + 5, at]
        assert _row(s, "event_ctr", "tb_bal", "tb_last", "task_time", "task_born", "task_id") == (3, left, at, at, T0 + 10, 2)


@pytest.mark.parametrize("direction", ["i", "o"])
def test_by_hand_the_task_at_the_window_end(direction):
    """window/task=wend+0.  inc 1,000.  2,500 B at T0 + 9 ms + 5: nine refills clamp to 2,500, all
    taken, last = T0 + 9 ms.  1,000 B at T0 + 9 ms + 6: 1,000 short = one refill, 999,994 ns away:
    the task is at T0 + 10 ms = window_end.  tt < window_end is false: the first call leaves it
    pending and the packet cached; the second call (no arrivals) runs it: forwarded at T0 + 10 ms."""
    a, b = _hand("window/task=wend+0", direction)[:2]
    assert a["pkt_status"].tolist() == [1, 0] and _row(a, "rflags", "task_time", "task_id") == (1 | 4, T0 + 10 * MS, 2)
    assert b["pkt_status"].tolist() == [1, 1] and b["fwd_time"].tolist() == [T0 + 9 * MS + 5, T0 + 10 * MS]
    assert _row(b, "rflags", "tb_bal", "tb_last", "event_ctr") == (0, 0, T0 + 10 * MS, 3)


@pytest.mark.parametrize("direction", ["i", "o"])
def test_by_hand_the_saturated_product(direction):
    """sat/inc=2^51/n=8191 and 8192.  inc = 2^51, capacity 2^51 + 1,500; 1,500 B at T0 + 5 leave 2^51.
    8,191 ms later: 2^51 * 8,191 = 2^64 - 2^51 fits; balance + tokens = 2^64 saturates to 2^64 - 1,
    clamped to the capacity; 28 B leave capacity - 28.  At 8,192 ms the product is 2^64: saturated
    itself.  A wrapping product would give 2^51 + 0 -> 2^51 - 28."""
    cap = 2**51 + 1500
    for n in (8191, 8192):
        s = _hand(f"sat/inc=2^51/n={n}", direction)[1]
        assert s["pkt_status"].tolist() == [1, 1] and s["fwd_time"].tolist() == [T0 + 5, T0 + n * I + 7]
        assert _row(s, "tb_cap", "tb_inc", "tb_bal", "tb_last") == (cap, 2**51, cap - 28, T0 + n * I)
    assert rc.N_MAX == 8000 and rc.INC_MAX == 2305843009213693 and 2**51 * 8000 < 2**64


def test_by_hand_the_codel_drop_inside_a_task():
    """codel/drop-then-blocked-pop.  inc 100; packet 0 (1,600 B) at T0 + 5 empties the bucket;
    packets 1-15 (1,000 B) at T0 + 6.  1,000 B are ten refills: packet k leaves at T0 + 10 k ms, the
    task that forwards it popping packet k + 1, which blocks.  The pop at T0 + 10 ms finds 9,999,994 ns
    < TARGET; the one at T0 + 20 ms 19,999,994 >= TARGET with 12,000 B behind: interval_end = T0 +
    120 ms.  At T0 + 120 ms = interval_end the task forwards packet 12 and pops 13: ok to drop, Store
    mode: dropped; 14 is popped behind it (1,000 B left: good, the interval is cleared) and returned,
    Drop mode, cur = 1, drop_next = T0 + 220 ms; it blocks: cached, task at T0 + 130 ms.  The call
    ending at T0 + 125 ms shows that state."""
    s = _hand("codel/drop-then-blocked-pop")[3]
    assert s["pkt_status"].tolist() == [1] * 13 + [2, 0, 0] and s["cached"][0] == (14, 1000)
    assert _row(s, "flags", "drop_next", "cur", "rflags", "task_time") == (1 | 4, T0 + 220 * MS, 1, 1 | 4, T0 + 130 * MS)
    assert s["fwd_time"].tolist()[:13] == [T0 + 5] + [T0 + 10 * k * MS for k in range(1, 13)]


def test_equal_key_is_an_error_in_the_model_too():
    """The error test_tie_task_after_later_event_and_equal_key pins on the device."""
    c = dict(rc.BY_NAME["tie/id-1"])
    c["events"] = c["events"][:2] + [rc.ev(T0 + I, 100, key=(T0 + 2, 2))]
    b = rc.build([c], "main", "window")
    with pytest.raises(ref.RelayError) as e:
        rc.ModelRun(b, "o", keyed=True).call(0)
    assert e.value.code == ref.E_ORDER


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name, which in (("test_windows_match_oracle", WINDOW_STREAMS), ("... and test_same_time_ties", STREAMS)):
        for scale in (1, 10):
            print("== the streams of %s, scale %d" % (name, scale))
            stream_survivors(which, scale, show=True)
