"""Link queues over time: busy time, waiting time, weight served and weight dropped per slot of watched
links and per time bin, summed on the device by sg_link_queue with SG_LINK_QUEUE_SERIES (DESIGN.md section
3.19).  The matrix lives here, in one device tensor that every call with series= adds into."""
import numpy as np

_UMAX = 0xFFFFFFFFFFFFFFFF


class LinkQueueSeries:
    """The time axis of link_queue's result.  ctx_or_graph: a NetworkGraph (its links and context) or a
    Context with n_links given.  Bin c < n_bins is [t0_ns + c bin_ns, t0_ns + (c + 1) bin_ns).
    Slots: none of link_slot, watch (every link its own slot, S = n_links); watch: link numbers, which
    take the slots 0, 1, .. in ascending link order, every other link is not watched; link_slot: one
    slot per link (negative, 2^32 - 1 or 2^64 - 1: not watched; several links may share a slot) with
    n_slots slots (None: the largest slot + 1).
    Pass the object as series= to shadow_amd.link_queue, NetworkGraph.link_queue_device,
    PathTree.link_queue_round, Group.link_queue_round or LinkQueueSession: every such call ADDS
    into the matrix, with or without limit_ns (the matrix lies behind 2 n_links entries of the buffer, and
    a call's per-link busy values end where it begins)."""

    def __init__(self, ctx_or_graph, t0_ns, bin_ns, n_bins, *, n_links=None, link_slot=None, n_slots=None, watch=None,
                 device="cuda"):
        if hasattr(ctx_or_graph, "links"):
            n_links = len(ctx_or_graph.links()[0])
        if n_links is None or int(n_links) < 0:
            raise ValueError("n_links: the number of links, with a Context")
        self.ctx = getattr(ctx_or_graph, "ctx", ctx_or_graph)
        self.n_links = nl = int(n_links)
        self.t0_ns, self.bin_ns, self.n_bins = int(t0_ns), int(bin_ns), int(n_bins)
        if not 0 <= self.t0_ns <= _UMAX:
            raise ValueError("t0_ns: a u64 time")
        if not 1 <= self.bin_ns <= _UMAX:
            raise ValueError("bin_ns: a positive u64 number of ns")
        if not 1 <= self.n_bins < 1 << 32:
            raise ValueError("n_bins: at least 1, below 2^32")
        if watch is not None and link_slot is not None:
            raise ValueError("watch, link_slot: one of them")
        slot = None
        if watch is not None:
            idx = np.unique(np.asarray(watch).astype(np.int64).ravel())
            if len(idx) != np.size(watch) or len(idx) == 0 or idx[0] < 0 or idx[-1] >= nl:
                raise ValueError(f"watch: distinct link numbers below {nl}, at least one")
            slot = np.full(nl, _UMAX, np.uint64)
            slot[idx] = np.arange(len(idx), dtype=np.uint64)
            n_slots = len(idx) if n_slots is None else n_slots
        elif link_slot is not None:
            raw = np.asarray(link_slot).ravel()
            if raw.shape != (nl,):
                raise ValueError(f"link_slot: {nl} entries, one per link")
            off = [int(x) < 0 or int(x) in (0xFFFFFFFF, _UMAX) for x in raw.tolist()]
            slot = np.array([_UMAX if o else int(x) for o, x in zip(off, raw.tolist())], dtype=np.uint64)
            top = max((int(x) for x, o in zip(slot.tolist(), off) if not o), default=0)
            n_slots = top + 1 if n_slots is None else n_slots
            if not 1 <= int(n_slots) < 1 << 32 or top >= int(n_slots):
                raise ValueError("n_slots: above every slot of link_slot, below 2^32")
        elif n_slots is not None and int(n_slots) != nl:
            raise ValueError("n_slots: with link_slot")
        self.link_slot = slot
        self.n_slots = nl if slot is None else int(n_slots)
        if self.n_slots * (self.n_bins + 2) > 1 << 31:
            raise ValueError("n_slots * (n_bins + 2): at most 2^31 cells a plane")
        hdr = np.array([self.t0_ns, self.bin_ns, self.n_bins, 0 if slot is None else self.n_slots], np.uint64)
        self._tail_host = hdr if slot is None else np.concatenate([hdr, slot])
        self._device = device
        self._buf = self._tail = None

    # ---- what a call takes
    @property
    def cells(self) -> int:
        """The cells of one plane, n_slots * (n_bins + 2)."""
        return self.n_slots * (self.n_bins + 2)

    def _ensure(self):
        import torch

        if self._buf is None:
            self.dev = torch.device(self._device)
            self._buf = torch.zeros(2 * self.n_links + 4 * self.cells, dtype=torch.int64, device=self.dev)
            self._tail = torch.from_numpy(self._tail_host.view(np.int64)).to(self.dev)

    def _check(self, n_links: int, dev=None):
        import torch

        if int(n_links) != self.n_links:
            raise ValueError(f"series: made for {self.n_links} links, the call has {n_links}")
        self._ensure()
        d = None if dev is None else torch.device(dev)
        if d is not None and d.type == "cuda" and d.index is not None and d.index != self._buf.device.index:
            raise ValueError(f"series: its matrix is on {self._buf.device}, the call runs on {d}")

    def host_cost(self, cost: np.ndarray) -> np.ndarray:
        """A host-mode call's cost_ps (n_links entries, or 2 n_links with the limits): the header and the slot
        map behind it."""
        return np.concatenate([np.ascontiguousarray(cost, np.uint64), self._tail_host])

    def host_busy(self, c0: int) -> np.ndarray:
        """A host-mode call's zeroed out_link_busy_ns, c0 per-link entries and the matrix."""
        return np.zeros(c0 + 4 * self.cells, np.uint64)

    def add_host(self, tail: np.ndarray) -> None:
        """What a host-mode call summed (the tail of its out_link_busy_ns), added into the matrix."""
        import torch

        self._ensure()
        self._buf[2 * self.n_links:] += torch.from_numpy(np.ascontiguousarray(tail, np.uint64).view(np.int64)).to(self.dev)

    def device_cost(self, cost):
        """A device-mode call's cost_ps from its int64 tensor of c0 entries: a copy with the tail."""
        import torch

        self._ensure()
        return torch.cat([cost.reshape(-1).to(self.dev), self._tail]).contiguous()

    def device_busy(self, c0: int):
        """A device-mode call's out_link_busy_ns, an int64 view of the buffer: c0 per-link entries, which the
        call overwrites, and the matrix, which it adds into."""
        self._ensure()
        if c0 not in (self.n_links, 2 * self.n_links):
            raise ValueError("series: n_links or 2 n_links per-link entries")
        return self._buf[2 * self.n_links - c0:]

    # ---- the result
    def planes(self) -> np.ndarray:
        """The whole matrix on the host, u64 [4, n_slots, n_bins + 2]: planes busy_ns, wait_ns, served,
        dropped; column n_bins before t0_ns, n_bins + 1 at or after the last bin's end."""
        if self._buf is None:
            return np.zeros((4, self.n_slots, self.n_bins + 2), np.uint64)
        return self._buf[2 * self.n_links:].cpu().numpy().view(np.uint64).reshape(4, self.n_slots, self.n_bins + 2)

    @property
    def busy_ns(self) -> np.ndarray:
        return self.planes()[0, :, :self.n_bins]

    @property
    def wait_ns(self) -> np.ndarray:
        return self.planes()[1, :, :self.n_bins]

    @property
    def served(self) -> np.ndarray:
        return self.planes()[2, :, :self.n_bins]

    @property
    def dropped(self) -> np.ndarray:
        return self.planes()[3, :, :self.n_bins]

    @property
    def before(self) -> np.ndarray:
        """[4, n_slots]: what fell before t0_ns, per plane."""
        return self.planes()[:, :, self.n_bins]

    @property
    def after(self) -> np.ndarray:
        """[4, n_slots]: what fell at or after t0_ns + n_bins bin_ns, per plane."""
        return self.planes()[:, :, self.n_bins + 1]

    def utilisation(self) -> np.ndarray:
        """busy_ns / bin_ns per slot and bin (float64): a slot of one link stays within [0, 1]."""
        return self.busy_ns.astype(np.float64) / float(self.bin_ns)

    def mean_waiting(self) -> np.ndarray:
        """wait_ns / bin_ns per slot and bin (float64): the mean number of records waiting."""
        return self.wait_ns.astype(np.float64) / float(self.bin_ns)

    def reset(self) -> None:
        if self._buf is not None:
            self._buf.zero_()
