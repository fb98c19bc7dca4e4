"""Inputs of the packet-outcome tests (test_outcomes_ref_cpu.py qualifies them on the CPU,
test_outcomes_gpu.py runs them).  A case is a queue_drop_cases case -- a queue_carry_cases.case dict
plus limit_ns -- plus base, one uncongested arrival time per packet.  A mode is (carry, drop)."""
import numpy as np

import outcomes_ref as OR
import queue_carry_cases as CC
import queue_cases as QC
import queue_drop_cases as DC
import queue_drop_ref as DR
import queue_ref as QR

MAX = QR.MAX
MODES = ((False, False), (True, False), (False, True), (True, True))
MODE_IDS = ("first", "carried", "first-drop", "carried-drop")
RECORDS = (0, 1, 255, 256, 257, 2 * 2048 + 1)  # around a block of lanes, and past two tiles of the scan
PACKETS = (0, 1, 255, 256, 257)
BASE0 = 10**9


def with_base(c, base=None, seed=5):
    """The case with base times: `base` (one value or an array), else drawn above BASE0."""
    P = c["n_packets"]
    if base is None:
        base = np.uint64(BASE0) + np.random.default_rng(seed).integers(0, 10**6, P).astype(np.uint64)
    b = np.full(P, int(base), np.uint64) if np.ndim(base) == 0 else np.asarray(base, np.uint64)
    assert b.shape == (P,)
    if "limit_ns" not in c:
        c = DC.with_limits(c, MAX)
    return dict(c, base=b)


def queue_ref(c, carry, drop):
    """(status, Result) of the queue reference of a mode; a Result without the drop rule has no
    drops and no refused field."""
    if drop:
        r = DC.ref_carried(c) if carry else DC.ref(c)
    else:
        r = CC.ref(c) if carry else QC.ref(c)
    return r[0], r[2]


def raw(res, drop):
    """A reference Result as the call's eight arrays."""
    out = {k: getattr(res, k) for k in QR.FIELDS}
    if drop:
        out["busy"] = np.concatenate([res.busy, res.refused])
        out["ahead_max"] = np.concatenate([res.ahead_max, res.drops])
    return out


def ref(c, carry, drop, res=None):
    """(status, records, delay, arrive, where) of outcomes_ref over the mode's queue reference."""
    if res is None:
        rc, res = queue_ref(c, carry, drop)
        assert rc == QR.OK
    return OR.outcomes(c["link_off"], c["enter"], c["packet"], res.wait, res.done, c["n_packets"], carry, c["base"])


def want(c, carry, drop):
    """The call's eight arrays with the tails behind the records, and the number of packets lost."""
    rc, res = queue_ref(c, carry, drop)
    assert rc == QR.OK
    rc, _, delay, arrive, where = ref(c, carry, drop, res)
    assert rc == QR.OK
    out = raw(res, drop)
    out["wait"] = np.concatenate([out["wait"], delay])
    out["done"] = np.concatenate([out["done"], arrive])
    out["ahead"] = np.concatenate([out["ahead"], where])
    return out, int((where < OR.ARRIVED).sum())


def with_empty(c):
    """The case with three more packets that have no record: one at index 0, one in the middle and
    one last."""
    P = c["n_packets"]
    mid = P // 2 + 1  # (its new index)
    new = np.arange(P) + 1
    new[new >= mid] += 1
    weight = None
    if c["weight"] is not None:
        weight = np.zeros(P + 3, np.uint32)
        weight[new] = c["weight"]
        weight[[0, mid, P + 2]] = 7
    out = dict(c, packet=new.astype(np.uint32)[c["packet"].astype(np.int64)] if len(c["packet"]) else c["packet"],
               weight=weight, n_packets=P + 3)
    if "base" in c:
        base = np.full(P + 3, 12345, np.uint64)
        base[new] = c["base"]
        out["base"] = base
    return out, (0, mid, P + 2)


def split(n, k=5):
    """n records over k links, uneven, an empty link among them."""
    cuts = sorted({0, n // 7, n // 3, n // 3, (2 * n) // 3, n})
    lengths = np.diff(cuts).tolist()
    return (lengths + [0] * k)[:max(k, len(lengths))]


def by_records(n, seed=3):
    """Exactly n records in chains of 1 to 3, limits drawn."""
    c = CC.from_lengths(split(n), seed) if n else CC.build(5, [], np.zeros(0, np.uint32), [1000] * 5)
    return with_base(DC.draw_limits(c, seed + 100))


def by_packets(P, seed=4):
    """Exactly P packets on routes of 1 to 4 links, limits drawn, free_in too."""
    c = CC.random_chains(seed, n_links=6, n_packets=P, span=40 * max(P, 1), free_max=30)
    return with_base(DC.draw_limits(c, seed + 100))


def random_case(seed):
    """The instances the definition's two carried facts were checked on."""
    return with_base(DC.draw_limits(CC.random_chains(seed), seed), seed=seed)


def hand():
    """queue_drop_cases.hand() with base 0: (case, the carried (where, delay), the first-order pair)."""
    c = with_base(DC.hand()[0], 0)
    A = OR.ARRIVED
    return c, ([1, A, A, 5], [0, 20, 10, 0]), ([1, A, A, A], [0, 20, 10, 10])


def all_dropped(seed=6):
    """Every link busy until long after the round and no buffer at all: every packet is dropped on
    its first hop."""
    c = CC.random_chains(seed, n_links=6, n_packets=60)
    return with_base(DC.with_limits(dict(c, free_in=np.full(6, 10**6, np.uint64)), 0))


def none_dropped(seed=7):
    return with_base(DC.with_limits(CC.random_chains(seed, n_links=6, n_packets=60, free_max=40), MAX))


def last_hop_drop():
    """Packet 0 crosses links 0, 1 and 2 and finds link 2 busy and without a buffer; packet 1 queues
    behind it on link 0; packet 2 crosses link 2 alone, later, and is dropped there too."""
    c = CC.build(3, [[(0, 100), (1, 120), (2, 140)], [(0, 105)], [(2, 500)]], [10, 10, 10], [1000] * 3,
                 np.uint64([0, 0, 10**6]))
    return with_base(DC.with_limits(c, [MAX, MAX, 0]))


def long_chains(cut):
    """queue_carry_cases.long_chains(): chains of 2,049 and 65 records among short ones.  cut: link 0,
    packet 0's first, is busy and has no buffer: carried, packet 0 has one dropped and 2,048 absent
    records; first order, one dropped and 2,048 served ones that do not count."""
    c = CC.long_chains()
    nl = len(c["link_off"]) - 1
    if not cut:
        return with_base(DC.with_limits(c, MAX))
    lim = np.full(nl, MAX, np.uint64)
    lim[0] = 0
    free = np.zeros(nl, np.uint64)
    free[0] = 10**6
    return with_base(DC.with_limits(dict(c, free_in=free), lim))


def ties():
    """First order only (carried, two records of a packet at one time are an error): packet 0
    crosses link 3 at 90 and links 0, 1 and 2 at 100, and link 1, busy and without a buffer, drops
    it: the crossings of links 0 and 2, served at the drop's own time, do not count, one listed
    before the dropped record and one after it.  Packet 1 is dropped twice at one time: the smaller
    record index is its `where`."""
    c = CC.build(5, [[(0, 100), (1, 100), (2, 100), (3, 90)], [(1, 200), (4, 200), (3, 150)]], [10, 10], [1000] * 5,
                 np.uint64([0, 10**6, 0, 0, 10**6]))
    return with_base(DC.with_limits(c, [MAX, 0, MAX, MAX, 0]))


def shuffled(c, seed=8):
    """The case with every link's records in a random order (the carried result stays at the input
    records; the first-order result is that of the order given)."""
    return CC.shuffled(c, seed)[0]


def edge_base(c, carry, drop, slack):
    """The case with one arrived, delayed packet's base such that base + delay = 2^64 - 1 - slack,
    and that packet."""
    rc, _, delay, _, where = ref(c, carry, drop)
    assert rc == QR.OK
    p = int(np.flatnonzero((where == OR.ARRIVED) & (delay > 0))[0])
    base = c["base"].copy()
    base[p] = np.uint64(MAX - slack - int(delay[p]))
    return dict(c, base=base), p


# ---- the real traces
_REAL = {}


def table(O, g):
    """(nodes, latency rows, predecessor rows) of every node of g, by the oracle and tree_ref."""
    import tree_ref as R

    nodes = np.arange(g["n"], dtype=np.uint32)
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                        rows=(0, g["n"]), threads=4)
    assert rc == 0
    pred, _, bad = R.tree_ref(g, nodes, (0, g["n"]), lat, loss)
    assert bad is None
    return nodes, lat, pred


def real_trace(O, name):
    """A fully watched real trace with the median rule's limits of its unlimited carried result:
    the tie round under queue_cases.TIE_COST (name "tie"), or queue_cases.sweep_round on a sweep
    graph under sweep_costs.  base is the trace's last exit per packet: its arrival without the
    rates (0 for a packet without a record).  Computed once per process."""
    if name in _REAL:
        return _REAL[name]
    import link_cases as LC
    import sweep_cases as WC
    import trace_cases as XC
    import trace_ref as XR

    if name == "tie":
        g = LC.tie_graph()
        nodes, lat, pred = table(O, g)
        hosts, pk, mixed = XC.tie_round()
        status = QC.group_status(mixed)  # (a quarter of the packets is not counted: no record)
        cost = np.full(XR.n_links(g), QC.TIE_COST, np.uint64)
    else:
        w, r = WC.case(name), WC.refs(O, name)[0]
        g, nodes, lat, pred, hosts, mixed = w["g"], w["nodes"], r["lat"], r["pred"], w["hosts"], None
        pk, status = QC.sweep_round(w)
        cost = QC.sweep_costs(name, XR.n_links(g))
    tr = XR.trace(g, nodes, (0, g["n"]), pred, lat, hosts, pk, status)
    c = CC.case(tr[0], tr[3], tr[1], pk["payload"], cost)
    _REAL[name] = dict(g=g, hosts=hosts, pk=pk, mixed=mixed, status=status, tr=tr, **real(c, tr))
    return _REAL[name]


def real(c, tr):
    """A real trace's case with the median limits and exit-time bases, its carried reference."""
    rc, _, unl = CC.ref(c)[:3]
    assert rc == QR.OK
    c = DC.with_limits(c, DR.median_limits(c["link_off"], unl.wait))
    rc, _, res, cur, _ = DC.ref_carried(c)
    assert rc == QR.OK
    c = with_base(c, last_exit(tr, c["n_packets"]))
    return dict(case=c, res=res, cur=cur, unl=unl)


def last_exit(tr, P):
    """Per packet the trace's exit time of its last record: its arrival without the rates."""
    base = np.zeros(P, np.uint64)
    order = np.argsort(tr[3], kind="stable")
    base[tr[1][order].astype(np.int64)] = tr[4][order]
    return base
