"""Reference model of the packet wire (shadow_amd.wire.PacketWire / sg_wire_*): the per-host
EventQueue restricted to Packet events, as a plain list of events.  It restates
core/work/event.rs:84-155 (order: time, source host, source event id) and
host/host.rs:753-757 (Host::execute pops while time < until) and is its own specification."""
import numpy as np

KEYS = ("host", "time_ns", "src_host", "event_id", "packet", "len", "tag")
TYPES = (np.uint32, np.uint64, np.uint32, np.uint64, np.uint32, np.uint32, np.int64)
NEVER = 2**64 - 1


class WireRef:
    def __init__(self):
        self.ev = {k: np.zeros(0, t) for k, t in zip(KEYS, TYPES)}

    def __len__(self):
        return len(self.ev["host"])

    def add(self, **cols):
        """Append events given as equal-length columns (tag: the caller's label, e.g. the round)."""
        n = len(cols["host"])
        cols.setdefault("tag", np.zeros(n, np.int64))
        self.ev = {k: np.concatenate([self.ev[k], np.asarray(cols[k]).astype(t)]) for k, t in zip(KEYS, TYPES)}

    def push(self, res, src_host, length, packet_id=None, id_base=0, tag=0):
        """The delivered packets of an oracle.deliver_round result: packet dst_order[i] goes to the
        host whose [dst_offsets[h], dst_offsets[h + 1]) holds i."""
        p = res["dst_order"].astype(np.int64)
        host = np.repeat(np.arange(len(res["dst_offsets"]) - 1), np.diff(res["dst_offsets"].astype(np.int64)))
        pkt = np.asarray(packet_id)[p] if packet_id is not None else id_base + p
        self.add(host=host, time_ns=res["deliver_time"][p], src_host=np.asarray(src_host)[p],
                 event_id=res["event_id"][p], packet=pkt, len=np.asarray(length)[p], tag=np.full(len(p), tag))

    def pop(self, window_end):
        """(events with time < window_end, in (host, time, src_host, event_id) order; the smallest
        time left, NEVER when empty).  The events leave."""
        due = self.ev["time_ns"] < np.uint64(window_end)
        out = {k: v[due] for k, v in self.ev.items()}
        o = np.lexsort((out["event_id"], out["src_host"], out["time_ns"], out["host"]))
        self.ev = {k: v[~due] for k, v in self.ev.items()}
        return {k: v[o] for k, v in out.items()}, (int(self.ev["time_ns"].min()) if len(self) else NEVER)

    def state(self):
        """What is held, in canonical order."""
        o = np.lexsort((self.ev["event_id"], self.ev["src_host"], self.ev["time_ns"], self.ev["host"]))
        return {k: v[o] for k, v in self.ev.items()}
