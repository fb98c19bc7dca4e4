"""Boundary cases of the relays' forward task and token bucket (relay/mod.rs, relay/token_bucket.rs;
the model is relay_ref.py): every decision at -1, 0 and +1 of its unit, the rest of the decision
held on the side that lets the threshold decide.  One case is one host: a bandwidth, a few events
(time, length; outbound: own-address flag, socket, the sending event's key), a name.  Every case
starts from a fresh pipeline object and reaches its boundary by events alone: a fresh bucket has
last = T0 (a whole millisecond) and last moves by whole intervals, so the refill grid is T0 + k ms
and an event's offset from it is free; the balance starts at inc + 1,500; inc = max(1, bw / 8,000)
is free per host.  test_relay_ref_cpu.py proves the cases against the model, the oracle and the
model's mutations; test_relay_gpu.py runs them through k_inbound, k_outbound and k_qdisc, one lane
each.

The window ends, bootstrap_end and sim_end are arguments of a call, shared by every host in it, so
the cases come in four environments (ENVS), and a case puts its events around its environment's
fixed times: "main" (window ends on the refill grid, one ns past it and one ns before it), "boot"
(bootstrap_end = T0 + 5 ms), "end" (sim_end = T0 + 15 ms), "sat" (a window of 9 s).

Families (a name's first part): refill, remove, wait, inc, sat, due, window, end, boot, codel
(inbound only), local, tie, rr (outbound only).  Length 0 is accepted by the entry points and the
oracle (remove/len=0).

Boundaries of the model that events alone cannot reach, and why:
* the wait's own saturation (INTERVAL * (nref - 1) past 2^64): nref <= need <= len < 2^32 since
  inc >= 1, so the product stays below 2^52.
* now + wait past 2^64, and last's saturation at EMU_MAX: wait < 2^52, so now would have to lie
  within 52 days of the year 2554; there the reference's own `now + delay` panics
  (host.rs:695-697), and last <= now always (last only advances by the whole intervals of now -
  last), while EMU_MAX is not on the refill grid (2^64 - 2 = 551,614 mod 10^6, T0 = 0 mod 10^6).
* bal + tokens past 2^64 without inc * n having saturated first, at a small increment: it needs
  inc * (n + 1) >= 2^64 - 1,500 while n <= (EMU_MAX - T0) / 10^6 < 2^44, so inc > 2^20 -- reachable
  only with bandwidths above 8 Gbit/s idle for years.  The sat family reaches it the short way, at
  inc = 2^51 after 8,191 ms (sat/sum=2^64-1, +0, +1), and the saturated product one ms later.
* a wake-up that falls one token short: the conforming duration always suffices (nref refills
  bring at least `need` tokens) unless the packet is longer than the bucket holds; that case is
  wait/len=cap+1, which blocks again at every wake-up.
* a wake-up (a task made by a blocked pop) off the refill grid or at bootstrap_end exactly: the
  conforming duration ends on the grid, and nothing blocks while bootstrapping; tasks 1 ns off a
  fixed time are made by arrivals (delay 0) or by the window ends 1 ns off the grid.
* a Local send whose key equals the pending task's: the entry points refuse it
  (test_tie_task_after_later_event_and_equal_key pins the error; test_relay_ref_cpu.py checks the
  model raises it too).

Forms (build): "window" -- a call per window of the environment, everything of a window in one
staged chunk; "call" -- the windows cut at every case's boundary time (its `split` event), so that
the events before a boundary go in an earlier call and the state passes through memory; "chunk" --
as "window", with a filler host in front of each case marked chunk=True (at least one of every family
but sat, in every environment but "sat"), sized so that the kernel's contiguous chunk boundary falls
on the case's split event: the task pops the previous chunk's elements from the ring.  The other
cases ride along at whatever position they fall.  "single" cuts at every event time: one event per host and call at most.
"""
import numpy as np

import relay_ref as ref

T0, MS, I, MTU, U64 = ref.T0, 10**6, ref.INTERVAL, ref.MTU, ref.U64
FAR = T0 + 10**12
ENVS = {
    # window ends: on the grid, one ns past it, one ns before it, inside the codel family's drop, then far
    # enough for every task
    "main": dict(windows=(T0 + 10 * MS, T0 + 20 * MS + 1, T0 + 30 * MS - 1, T0 + 125 * MS, T0 + 400 * MS), boot=0, sim_end=FAR),
    "boot": dict(windows=(T0 + 3 * MS, T0 + 10 * MS, T0 + 40 * MS), boot=T0 + 5 * MS, sim_end=FAR),
    "end": dict(windows=(T0 + 10 * MS, T0 + 20 * MS, T0 + 40 * MS), boot=0, sim_end=T0 + 15 * MS),
    "sat": dict(windows=(T0 + 10 * MS, T0 + 9000 * MS, T0 + 9010 * MS), boot=0, sim_end=FAR),
}
FORMS = ("call", "window", "chunk")
BE, SE = ENVS["boot"]["boot"], ENVS["end"]["sim_end"]
W = ENVS["main"]["windows"]
OTHER_IP, FILLER_BW = 0x0B000001, 10**9
CASES = []


def ip_of(h):
    return 0x0A000001 + h


def ev(t, ln, local=False, sock=0, key=None):
    return (t, ln, local, sock, key)


def case(name, bw, events, env="main", dirs="io", split=None, chunk=False, expect="", kills=None):
    """dirs: "i" inbound, "o" outbound; split: the index of the boundary event (the last one by
    default); kills: {variant: the output that shows it}; expect: what the case pins, in words."""
    assert all(c["name"] != name for c in CASES), name
    events = [e if len(e) == 5 else ev(*e) for e in events]
    assert len(events) <= 48 and all(a[0] <= b[0] for a, b in zip(events, events[1:]))
    assert all(e[0] < ENVS[env]["windows"][-1] for e in events)
    keyed = any(e[4] is not None for e in events)
    outbound_only = keyed or any(e[2] or e[3] for e in events)
    assert not (outbound_only and "i" in dirs), name
    assert all(k in ref.VARIANTS for k in (kills or {})), name
    CASES.append(dict(name=name, family=name.split("/")[0], bw=bw, events=events, env=env, dirs=dirs, keyed=keyed,
                      split=len(events) - 1 if split is None else split, chunk=chunk, expect=expect, kills=kills or {}))


BW = lambda inc: inc * 8000
A = T0 + 5   # a first event's time: 5 ns into the first interval

# ---- refill ---------------------------------------------------------------------------------------
# inc 1,000, capacity 2,500.  A 1,500-B packet at T0 + 5 leaves 1,000; two more at T0 + 1 ms + d
for d in (-1, 0, 1):
    case(f"refill/span=I{d:+d}", BW(1000), [(A, 1500), (T0 + I + d, 1500), (T0 + I + d, 1500)], split=1, chunk=d == 0,
         expect="the second packet leaves at T0 + 1 ms + max(d, 0); at d = -1 a wake-up after 1 ns forwards it; the "
                "third waits INTERVAL - span: the task at T0 + 2 ms",
         kills={"span>I": "fwd_time"} if d == 0 else {} if d < 0 else {"last=now": "fwd_time"})
# inc 100, capacity 1,600: 100 left, then 300 B at T0 + 2 ms + d need two refills
for d in (-1, 0, 1):
    case(f"refill/span=2I{d:+d}", BW(100), [(A, 1500), (T0 + 2 * I + d, 300)],
         expect="n = 1 at d = -1 (blocked for 1 ns), n = 2 from d = 0 on: forwarded at T0 + 2 ms + max(d, 0)")
case("refill/n=7", BW(100), [(A, 1500), (T0 + 7 * I + 3, 800)], expect="seven refills bring exactly the 800 B")
# tokens landing at capacity - 1, capacity, capacity + 1: 2,500 - L1 left, one refill of 1,000
for d in (-1, 0, 1):
    case(f"refill/sum=cap{d:+d}", BW(1000), [(A, 1000 - d), (T0 + I, 1500), (T0 + I, 1001)],
         expect="balance 2,499 / 2,500 / 2,500 after the refill: the 1,001-B packet is 2 / 1 / 1 B short",
         kills={"clamp-dropped": "fwd_time", "clamp-cap+1": "fwd_time"} if d == 1 else {})

# ---- remove ---------------------------------------------------------------------------------------
for d in (-1, 0, 1):
    case(f"remove/bal=len{d:+d}", BW(1000), [(A, 1500), (A + 5, 1000 - d)],
         expect="1,000 B in the bucket against 1,001 / 1,000 / 999: blocked, forwarded to 0, forwarded to 1",
         kills={"bal>dec": "fwd_time"} if d == 0 else {})
case("remove/len=cap", BW(1000), [(A, 2500), (A + 1, 1)], expect="the whole bucket in one packet, the next 1 B short")
case("remove/len=0", BW(1000), [(A, 2500), (A + 1, 0), (A + 2, 1)], expect="a 0-B packet passes an empty bucket")

# ---- wait -----------------------------------------------------------------------------------------
# inc 100: the bucket emptied at T0 + 5, then a packet of the deficit's size
for need, nref in ((99, 1), (100, 1), (101, 2), (200, 2), (201, 3)):
    case(f"wait/need={need}", BW(100), [(A, 1600), (A + 5, need)], chunk=need == 101,
         expect=f"ceil({need} / 100) = {nref} refills: forwarded at T0 + {nref} ms, exactly sufficing at 100 and 200",
         kills={"nref-floor": "event_ctr", "nref<=2": "event_ctr"} if need == 101 else {})
case("wait/len=cap+1", BW(1000), [(A, 2501)], expect="never fits: a wake-up every ms, each 1 B short, blocks again")

# ---- inc ------------------------------------------------------------------------------------------
for bw in (0, 7999, 8000, 15999, 16000):
    case(f"inc/bw={bw}", bw, [(A, 1500), (A + 1, 3)],
         expect="inc 1 (2 at 16,000): 1 (2) B left, the 3-B packet waits 2 refills (1)",
         kills={"inc-without-max": "tb_inc", "cap-without-mtu": "tb_cap"} if bw == 7999 else {})

# ---- sat ------------------------------------------------------------------------------------------
P51 = 2**51   # inc 2^51: n_max = 8,191; the capacity is 2^51 + 1,500
for n in (8191, 8192, 8193):
    case(f"sat/inc=2^51/n={n}", BW(P51), [(A, 1500), (T0 + n * I + 7, 28)], env="sat",
         expect="shows in tb_bal = capacity - 28 and tb_last = T0 + n ms, in no fate: inc * n = 2^64 - 2^51, then "
                "saturated; balance + tokens = 2^64 saturates already at 8,191",
         kills={"bal+tokens-wraps": "tb_bal"} if n == 8191 else {"tokens-wrap": "tb_bal"} if n == 8192 else {})
for d in (-1, 0, 1):
    case(f"sat/sum=2^64{d:+d}", BW(P51), [(A, 1500 - d), (T0 + 8191 * I + 7, 28)], env="sat",
         expect="balance + tokens = 2^64 - 1 (fits), 2^64, 2^64 + 1 (saturate): tb_bal = capacity - 28 in all three")
BW_MAX = U64
INC_MAX = max(1, BW_MAX // 8 // 1000)
N_MAX = U64 // INC_MAX
for d in (-1, 0, 1):
    case(f"sat/bw=max/n=n_max{d:+d}", BW_MAX, [(A, 1500), (T0 + (N_MAX + d) * I + 7, 28)], env="sat",
         expect=f"the largest bandwidth: inc {INC_MAX}, n_max {N_MAX}; tb_bal = capacity - 28, tb_last on the grid")

# ---- due ------------------------------------------------------------------------------------------
K = T0 + I   # the wake-up of a packet blocked in the first interval
for d in (-1, 0, 1):
    case(f"due/arrival=task{d:+d}", BW(1000), [(A, 1500), (A + 5, 1500), (K + d, 100)], chunk=d == 0,
         expect="d <= 0: the arrival is queued before the wake-up runs (Packet first at d = 0), both leave at K "
                "through one task; d = +1: the wake-up runs first, the arrival makes a task of its own at K + 1",
         kills={"tt<=arrival": "event_ctr"} if d == 0 else {})
case("due/same-time-group", BW(1000), [(A, 100)] * 3, expect="one task, one id: the counter advances by 1",
     kills={"group-id-per-arrival": "event_ctr"})
case("due/queued-behind-cached", BW(1000), [(A, 1500), (A + 5, 1500), (A + 5, 1000)],
     expect="the blocked packet is cached, not queued again: it leaves first at K, the 1,000-B one behind it a ms later",
     kills={"blocked-requeued": "fwd_time"})
case("due/wake-blocks-again", BW(1000), [(A, 1500), (A + 5, 1500), (A + 6, 1500), (K + 7, 28)], chunk=True,
     expect="the wake-up at K forwards one and blocks on the next: the new wake-up is K + 1 ms, counted from the "
            "task's time and not from the arrival at K + 7 that made it due",
     kills={"wake-from-arrival": "fwd_time"})

# ---- window ---------------------------------------------------------------------------------------
# a wake-up on the grid against window ends on it (W[0]), one ns past it (W[1]) and one ns before it (W[2])
for j, d in ((0, 0), (1, -1), (2, 1)):
    g = (10, 20, 30)[j] * MS + T0   # the wake-up
    for tail in ("", "/then-arrival"):
        evs = [(g - MS + 5, 2500), (g - MS + 6, 1000)] + ([(g + 5, 28)] if tail else [])
        case(f"window/task=wend{d:+d}{tail}", BW(1000), evs, split=1,
             expect="d = -1: runs in the call; d = 0, +1: carried over, run by the next call (before its first "
                    "arrival, or with none); forwarded at the wake-up's time either way",
             kills={"tt<=window_end": "rflags"} if d == 0 and not tail else {})
case("window/arrival=wend-1", BW(1000), [(W[0] - 1, 100)], expect="the task at window_end - 1 runs in its call")

# ---- end ------------------------------------------------------------------------------------------
for d in (-1, 0, 1):
    case(f"end/arrival=sim_end{d:+d}", BW(1000), [(SE + d, 100), (SE + d + 5, 100), (SE + MS, 100)], env="end",
         expect="d = -1: forwarded at sim_end - 1, the later arrivals make tasks that never run; d >= 0: the task "
                "takes an id and never runs (R_NEVER), later arrivals schedule nothing and queue up",
         kills={"at>sim_end": "pkt_status", "never-takes-no-id": "event_ctr"} if d == 0 else {})
case("end/wake=sim_end", BW(1000), [(SE - MS + 5, 2500), (SE - MS + 6, 1000), (SE + 5, 100)], env="end",
     expect="the wake-up lands on sim_end: it takes an id, never runs, the cached packet stays")
case("end/wake=sim_end-1ms", BW(1000), [(SE - 2 * MS + 5, 2500), (SE - 2 * MS + 6, 1000)], env="end",
     expect="a wake-up one interval before sim_end runs")

# ---- boot -----------------------------------------------------------------------------------------
for d in (-1, 0, 1):
    case(f"boot/task=boot{d:+d}", BW(1000), [(BE + d, 2500), (BE + d, 1)], env="boot",
         expect="d = -1: both forwarded, the bucket untouched; d >= 0: five refills clamp to 2,500, the 1-B packet "
                "blocks", kills={"now>boot": "fwd_time"} if d == 0 else {})
case("boot/run-then-limited", BW(1000),
     [(T0 + 1 * MS + 5, 1500), (T0 + 2 * MS + 5, 1500), (T0 + 2 * MS + 500005, 1500), (T0 + 4 * MS, 1500), (BE + 7, 1500)],
     env="boot", expect="four unlimited pops leave balance and last_refill as created (seen after the first call, "
                        "which ends while bootstrapping); the first limited one refills five intervals at once",
     kills={"boot-pop-refills": "tb_last"})

# ---- codel (inbound) ------------------------------------------------------------------------------
# inc 100: 1,100 B blocked at T0 + 1 ms + 6 wake at KC = T0 + 12 ms; three 1,000-B packets queued so
# that the head's sojourn at KC is TARGET + d; the arrival that makes the task due comes 5 ns later
KC, TARGET = T0 + 12 * MS, 10 * MS
for d in (-1, 0, 1):
    ts = KC - TARGET - d
    case(f"codel/sojourn-at-task=T{d:+d}", BW(100),
         [(T0 + MS + 5, 1600), (T0 + MS + 6, 1100)] + [(ts, 1000)] * 3 + [(KC + 5, 28)], dirs="i", chunk=d == -1,
         expect="the pop happens at the task's time: at d = -1 the head is below TARGET there and past it at the "
                "arrival's; d >= 0 start the interval (flags, interval_end)",
         kills={"codel-pop-at-arrival": "flags"} if d == -1 else {})
case("codel/drop-then-blocked-pop", BW(100), [(A, 1600)] + [(A + 1, 1000)] * 15, dirs="i",
     expect="a packet per 10 ms; the interval starts at T0 + 20 ms; at T0 + 120 ms = interval_end the task's pop "
            "drops the head and returns the next, which blocks: one drop, a cached packet, Drop mode (seen at the "
            "window end T0 + 125 ms)")

# ---- local (outbound) -----------------------------------------------------------------------------
case("local/between", BW(1000), [ev(A, 1500), ev(A + 1, 500, local=True), ev(A + 2, 1000), ev(T0 + I + 5, 100, local=True)],
     dirs="o", expect="own-address packets take no tokens (the 1,000-B packet finds 1,000) and do not refill: "
                      "tb_last stays T0 after the local packet at T0 + 1 ms + 5",
     kills={"local-takes-tokens": "fwd_time", "local-refills": "tb_last"})
case("local/behind-cached", BW(1000), [ev(A, 1500), ev(A + 1, 1500), ev(A + 2, 100, local=True)], dirs="o",
     expect="a local packet queues behind the cached one and leaves with it at the wake-up")

# ---- tie (outbound, keyed) --------------------------------------------------------------------------
# Packet-event sends at T0 + 1 and T0 + 2: tasks 0 and 1, the blocked one's wake-up is task 2, created at T0 + 2
for nm, key, first in (("created-1", (T0 + 1, 50), "send"), ("created+1", (T0 + 3, 1), "task"),
                       ("id-1", (T0 + 2, 1), "send"), ("id+1", (T0 + 2, 3), "task")):
    case(f"tie/{nm}", BW(1000), [ev(T0 + 1, 1500), ev(T0 + 2, 1500), ev(K, 100, key=key)], dirs="o",
         expect=f"a Local event's send at the wake-up's nanosecond, key {nm} of the task's (T0 + 2, 2; 51 at "
                f"created-1, whose event exists when the blocked task runs): the {first} goes first (send first: one "
                "task forwards both; task first: the send makes a task of its own, one more id)",
         kills={"created-1": {}, "created+1": {"tie-ignores-created": "event_ctr"},
                "id-1": {"tie-ignores-id": "event_ctr"}, "id+1": {"tie-created<=": "event_ctr"}}[nm])

# ---- rr (outbound, sockets) -------------------------------------------------------------------------
case("rr/cached-socket-rotated", BW(1000),
     [ev(T0 + 1, 1500, sock=2), ev(T0 + 2, 1500, sock=0), ev(T0 + 2, 100, sock=0), ev(T0 + 2, 100, sock=1)], dirs="o",
     expect="round-robin: the blocked packet's socket went behind the other when it was popped, so the wake-up "
            "forwards the cached packet, then socket 1's, then socket 0's second; fifo keeps the send order")

# the chunk form puts a chunk boundary inside one case of every family whose boundary event has events of the
# same call before it (the sat family's two events lie 8 s and a call apart: nothing to straddle)
for _n in ("remove/bal=len-1", "inc/bw=8000", "window/task=wend+0/then-arrival", "end/wake=sim_end", "boot/task=boot+0",
           "local/behind-cached", "tie/id-1", "rr/cached-socket-rotated"):
    [c for c in CASES if c["name"] == _n][0]["chunk"] = True
NAMES = tuple(c["name"] for c in CASES)
BY_NAME = {c["name"]: c for c in CASES}


def of(env, direction, keyed=None):
    """The cases of one environment that run in one direction ("i" / "o"); keyed=False leaves out those with keys."""
    return [c for c in CASES if c["env"] == env and direction in c["dirs"] and (keyed is None or keyed or not c["keyed"])]


def _cuts(cases, env, form):
    """The calls' ends: the environment's window ends and, between them, the form's cut times."""
    ends = set(ENVS[env]["windows"])
    if form == "call":
        ends |= {c["events"][c["split"]][0] for c in cases if c["split"] > 0}
    elif form == "single":
        ends |= {e[0] for c in cases for e in c["events"]}
    return sorted(t for t in ends if t > T0)


def ring_cap(direction, form):
    """64 slots: the rings wrap.  An outbound ring bounds a call's sends, so the chunk form's filler needs 1,024."""
    return 1024 if direction == "o" and form == "chunk" else 64


def spread(n, n_hosts=130):
    """n host ids spread evenly over n_hosts: two full blocks of 64 lanes and a tail."""
    return [i * (n_hosts - 1) // max(n - 1, 1) for i in range(n)]


def build(cases, env, form, chunk=1024, hosts=None, n_hosts=None, lead=0):
    """The cases as one batch of hosts: dict(bw, ip, calls, n_pkt, host, ctr0) with calls a list of
    (window_end, columns) and columns host, time, pkt, len, payload, dst, socket, event_id,
    event_created (grouped by ascending host, each host's in order; event_id UINT64_MAX: made by
    a Packet event); host[i] is cases[i]'s host.  form "chunk" puts a filler host in front of each
    case marked chunk (hosts given: not allowed; lead: idle hosts in front), `chunk` events being the kernel's
    contiguous chunk."""
    ends = _cuts(cases, env, form)
    call_of = lambda t: int(np.searchsorted(ends, t, side="right"))
    plan = []   # (case or None, filler events, filler call)
    if form == "chunk":
        assert hosts is None
        plan = [(None, 0, 0)] * lead   # hosts without events in front: the cases cross into the next block
        cum = {}   # (block, call) -> events so far
        for c in cases:
            if c["chunk"]:
                h, j = len(plan), call_of(c["events"][c["split"]][0])
                if (h + 1) // 64 != h // 64:   # the filler and its case in one block
                    plan.append((None, 0, 0))
                    h += 1
                before = sum(1 for e in c["events"][:c["split"]] if call_of(e[0]) == j)
                n = (-(cum.get((h // 64, j), 0) + before)) % chunk or chunk
                plan.append((None, n, j))
                cum[(h // 64, j)] = cum.get((h // 64, j), 0) + n
            h = len(plan)
            plan.append((c, 0, 0))
            for e in c["events"]:
                k = (h // 64, call_of(e[0]))
                cum[k] = cum.get(k, 0) + 1
        hosts = list(range(len(plan)))
    else:
        hosts = list(range(len(cases))) if hosts is None else [int(h) for h in hosts]
        slots = dict(zip(hosts, cases))
        plan = [(slots.get(h), 0, 0) for h in range(n_hosts or (max(hosts) + 1 if hosts else 0))]
    H = len(plan)
    bw = np.full(H, FILLER_BW, np.uint64)
    rows = [[] for _ in ends]
    host_of, p, pkt_host = {}, 0, []
    for h, (c, n_fill, j_fill) in enumerate(plan):
        if c is None:
            start = ends[j_fill - 1] if j_fill else T0
            assert start + n_fill < ends[j_fill]
            for i in range(n_fill):
                rows[j_fill].append((h, start + i, p, 28, 0, OTHER_IP, 0, U64, 0))
                p += 1
            pkt_host += [h] * n_fill
            continue
        bw[h] = c["bw"]
        host_of[c["name"]] = h
        for t, ln, local, sock, key in c["events"]:
            born, eid = key if key is not None else (0, U64)
            rows[call_of(t)].append((h, t, p, ln, max(ln, 28) - 28, ip_of(h) if local else OTHER_IP, sock, eid, born))
            p += 1
        pkt_host += [h] * len(c["events"])
    dts = (np.uint32, np.uint64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint64, np.uint64)
    calls = []
    for end, r in zip(ends, rows):
        cols = list(zip(*r)) if r else [[]] * 9
        calls.append((end, tuple(np.array(a, d) for a, d in zip(cols, dts))))
    return dict(bw=bw, ip=np.array([ip_of(h) for h in range(H)], np.uint32), calls=calls, n_pkt=max(p, 1),
                host=[host_of[c["name"]] for c in cases], boot=ENVS[env]["boot"], sim_end=ENVS[env]["sim_end"],
                names={h: n for n, h in host_of.items()}, pkt_host=np.array(pkt_host, np.int64))


# ---- running a batch: the model, the oracle, and what is compared after every call ------------------
RELAY = ("rflags", "task_time", "task_id", "task_born", "tb_cap", "tb_bal", "tb_inc", "tb_last")
SENT = ("src_host", "dst_ipv4", "payload_len", "send_time", "packet")
CODEL = ("flags", "interval_end", "drop_next", "cur", "prev", "bytes", "head", "tail")


def fates(status, fwd, ctr):
    """Statuses, forward times where a packet has a fate, counters."""
    status, fwd = np.asarray(status, np.uint8), np.asarray(fwd, np.uint64)
    return dict(pkt_status=status.copy(), fwd_time=np.where(status != 0, fwd, 0).astype(np.uint64),
                event_ctr=np.asarray(ctr, np.uint64).copy())


def inbound_snapshot(st):
    """oracle.inbound_state's layout (the model's and the library's too): relay and queue scalars,
    the cached packet where one is cached, the live ring slots."""
    out = {k: np.asarray(st[k]).copy() for k in RELAY + CODEL}
    c = (st["rflags"] & ref.RL_CACHED) != 0
    out["cached"] = [(int(p), int(n)) if m else None for m, p, n in zip(c, st["cached_pkt"], st["cached_len"])]
    cap, ring = st["cap"], []
    for h in range(len(c)):
        n = (int(st["tail"][h]) - int(st["head"][h])) % 2**32
        assert n <= cap
        s = [h * cap + (int(st["head"][h]) + j) % cap for j in range(n)]
        ring.append([(int(st["ring_pkt"][i]), int(st["ring_ts"][i]), int(st["ring_len"][i])) for i in s])
    out["ring"] = ring
    return out


def fifo_snapshot(st):
    """oracle.outbound_state's layout: the relay, and per host the packets still to go (the cached
    one at head - 1, then the queue) as (packet, len, payload, dst)."""
    out = {k: np.asarray(st[k]).copy() for k in RELAY}
    cap, q = st["cap"], []
    for h in range(len(st["head"])):
        lo = int(st["head"][h]) - (1 if st["rflags"][h] & ref.RL_CACHED else 0)
        s = [h * cap + (lo + j) % cap for j in range((int(st["tail"][h]) - lo) % 2**32)]
        q.append([(int(st["ring_pkt"][i]), int(st["ring_len"][i]), int(st["ring_pay"][i]), int(st["ring_dst"][i]))
                  for i in s])
    out["queue"] = q
    return out


def qdisc_snapshot(st, relay, S, cap):
    """The canonical round-robin state (sg_outbound_qdisc_state) per host: the deque with each
    socket's count, the queued packets in its order, the cached packet."""
    out = {k: np.asarray(relay[k]).copy() for k in RELAY}
    q = []
    for h in range(len(st["n_active"])):
        na, nq = int(st["n_active"][h]), int(st["n_queued"][h])
        rec = lambda pre, i: tuple(int(st[pre + k][i]) for k in ("packet", "len", "payload_len", "dst"))
        q.append(([(int(st["active"][h * S + j]), int(st["active_count"][h * S + j])) for j in range(na)],
                  [rec("q_", h * cap + j) for j in range(nq)],
                  rec("cached_", h) if relay["rflags"][h] & ref.RL_CACHED else None))
    out["queue"] = q
    return out


def same(a, b, what=""):
    """Two snapshots key by key; names the first key that differs."""
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        eq = np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
        assert eq, (what, k)


def who_differs(a, b, batch):
    """The names of the cases (or "host <h>") whose lane differs between two snapshots, and in which keys."""
    H, out = len(batch["bw"]), {}
    for k in a:
        x, y = a[k], b[k]
        if k in ("pkt_status", "fwd_time"):
            n = len(batch["pkt_host"])
            hosts = set(batch["pkt_host"][np.nonzero(np.asarray(x[:n]) != np.asarray(y[:n]))[0]].tolist())
            if not np.array_equal(x[n:], y[n:]):
                hosts.add(-1)   # a packet of the traffic beside the cases
        elif len(x) == H and len(y) == H:
            hosts = {h for h in range(H) if not (x[h] == y[h])}
        else:
            hosts = set() if np.array_equal(x, y) else {-1}
        for h in hosts:
            out.setdefault(batch["names"].get(h, "host %d" % h), []).append(k)
    return out


class ModelRun:
    """relay_ref on a batch: call(j) runs call j and returns its snapshot."""

    def __init__(self, b, direction, qdisc=ref.FIFO, keyed=False, cap=64, S=4, trace=None, variant=None):
        self.b, self.dir, self.keyed, self.qdisc = b, direction, keyed, qdisc
        if direction == "i":
            self.m = ref.Inbound(b["bw"], cap, trace, variant)
        else:
            self.m = ref.Outbound(b["ip"], b["bw"], cap, qdisc, S, trace, variant)
        n = b["n_pkt"]
        self.status, self.fwd, self.ctr = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(len(b["bw"]), np.uint64)

    def created(self):
        """The relay state as the objects are created, before any call."""
        return {k: np.asarray(v).copy() for k, v in ref.relay_state(self.m.relays).items()}

    def call(self, j):
        end, (host, t, pkt, ln, pay, dst, sock, eid, born) = self.b["calls"][j]
        b, out = self.b, {}
        if self.dir == "i":
            self.m.run(host, t, pkt, ln, end, b["boot"], b["sim_end"], self.ctr, self.fwd, self.status)
            out = inbound_snapshot(self.m.state())
        else:
            k = (eid, born) if self.keyed else (None, None)
            sent = self.m.run(host, t, pkt, ln, pay, dst, sock, end, b["boot"], b["sim_end"], self.ctr, self.fwd,
                              self.status, *k)
            if self.qdisc == ref.FIFO:
                out = {k: v for k, v in self.m.relay_state().items()}
                out["queue"] = [self.m.queued(h) for h in range(len(b["bw"]))]
            else:
                out = qdisc_snapshot(self.m.qdisc_state(), self.m.relay_state(), self.m.S, self.m.cap)
            out.update({"sent_" + k: sent[k] for k in SENT})
        out.update(fates(self.status, self.fwd, self.ctr))
        return out


class OracleRun:
    """oracle.inbound_run / outbound_run (fifo) on a batch, the same way."""

    def __init__(self, O, b, direction, keyed=False, cap=64):
        self.O, self.b, self.dir, self.keyed = O, b, direction, keyed
        self.st = O.inbound_state(b["bw"], cap) if direction == "i" else O.outbound_state(b["ip"], b["bw"], cap)
        n = b["n_pkt"]
        self.status, self.fwd, self.ctr = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(len(b["bw"]), np.uint64)

    def call(self, j):
        end, (host, t, pkt, ln, pay, dst, sock, eid, born) = self.b["calls"][j]
        b = self.b
        if self.dir == "i":
            self.O.inbound_run(self.st, host, t, pkt, ln, end, b["boot"], b["sim_end"], self.ctr, self.fwd, self.status)
            out = inbound_snapshot(self.st)
        else:
            k = dict(event_id=eid, event_created=born) if self.keyed else {}
            sent = self.O.outbound_run(self.st, host, t, pkt, ln, pay, dst, end, b["boot"], b["sim_end"], self.ctr,
                                       self.fwd, self.status, **k)
            out = fifo_snapshot(self.st)
            out.update({"sent_" + k: sent[k] for k in SENT})
        out.update(fates(self.status, self.fwd, self.ctr))
        return out
