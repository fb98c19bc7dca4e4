"""The closed-loop scenario of the wire tests, computed on the CPU by the oracle chain
oracle.deliver_round -> wire_ref.WireRef -> oracle.inbound_run.  A plain module: the GPU tests
compare the device chain against it round by round, and tests/test_wire_cpu.py checks that the
scenario exercises what it is meant to (far list, several rounds meeting in one pop, ...)."""
import numpy as np

from shadow_amd import synth
from wire_ref import WireRef

T0 = 946684800 * 10**9  # EmulatedTime::SIMULATION_START
MS = 10**6
H = 64
PER_ROUND = 2000
SEND_ROUNDS = 12   # rounds with sends
ROUNDS = 56        # then quiet rounds until the 40 ms class has arrived
SIM_END = T0 + 10**12
LAT_CLASSES_NS = (300_000, 1_000_000, 2_500_000, 7_000_000, 19_000_000, 40_000_000)
RING_CAP = 4096
QUIET_HOST = H - 1  # receives only what round 5 sends it
_cache = {}


def network(seed=7, loss_hi=0.05):
    """64 hosts, host h on node h, and a synthetic 64 x 64 table: latencies from the six classes."""
    rng = np.random.default_rng(seed)
    hosts = synth.make_hosts(H, H)
    lat = rng.choice(np.array(LAT_CLASSES_NS, np.uint64), (H, H))
    loss = (rng.random((H, H)) * loss_hi).astype(np.float32)
    bw = rng.choice(np.array([50, 200, 1000], np.uint64), H) * np.uint64(10**6)
    return hosts, lat, loss, bw


def round_packets(hosts, k, n=PER_ROUND):
    """Round k's sends (grouped by source, send order); only round 5 sends to QUIET_HOST."""
    pk = synth.make_packets(n, hosts, T0 + k * MS, T0 + (k + 1) * MS, seed=100 + k)
    if k != 5:
        quiet = pk["dst_ip"] == hosts["ip"][QUIET_HOST]
        other = np.where(pk["src"] == 0, hosts["ip"][1], hosts["ip"][0]).astype(np.uint32)
        pk["dst_ip"] = np.where(quiet, other, pk["dst_ip"]).astype(np.uint32)
    pk["len"] = (pk["payload"] + 28).astype(np.uint32)
    return pk


def scenario(oracle):
    """The reference run: per round the packets, the delivery, the pop, the inbound outputs."""
    if "sc" in _cache:
        return _cache["sc"]
    hosts, lat, loss, bw = network()
    rng_state = np.stack([oracle.xoshiro_seed(int(s)) for s in hosts["seed"]]).astype(np.uint64)
    rng0 = rng_state.copy()
    ctr = np.zeros(H, np.uint64)
    n_pk = SEND_ROUNDS * PER_ROUND
    ost = oracle.inbound_state(bw, RING_CAP)
    fwd = np.full(n_pk, np.uint64(2**64 - 1))
    st = np.zeros(n_pk, np.uint8)
    wire = WireRef()
    rounds = []
    for k in range(ROUNDS):
        end = T0 + (k + 1) * MS
        r = dict(end=end, pk=None)
        if k < SEND_ROUNDS:
            pk = round_packets(hosts, k)
            want = oracle.deliver_round(end, SIM_END, 0, pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"],
                                        hosts["ip"], hosts["route"], lat, loss, rng_state, ctr)
            wire.push(want, pk["src"], pk["len"], id_base=k * PER_ROUND, tag=k)
            r.update(pk=pk, want=want, id_base=k * PER_ROUND)
        pop, nxt = wire.pop(end)
        oracle.inbound_run(ost, pop["host"], pop["time_ns"], pop["packet"], pop["len"], end, 0, SIM_END, ctr, fwd, st)
        r.update(pop=pop, next=nxt, fwd=fwd.copy(), st=st.copy(), ctr=ctr.copy(), held=wire.state())
        rounds.append(r)
    sc = dict(hosts=hosts, lat=lat, loss=loss, bw=bw, rng0=rng0, rounds=rounds, n_pk=n_pk, inbound=ost,
              rng_end=rng_state)
    _cache["sc"] = sc
    return sc
