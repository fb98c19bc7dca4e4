"""What a round's Python entry points do to their arguments before the library sees them: integer
arrays onto the packets' device, the weight, the watch mask, the capacity retry and the series' out=.
One home for PathTree, Group, LinkQueueSession and link_queue.py; plain functions, no state."""
import numpy as np

from . import _capi

_TORCH_VIEW = {1: "uint8", 4: "int32", 8: "int64"}  # torch has no u32 / u64 arithmetic: the signed views


def int_tensor(x, np_dtype, count: int, dev, what: str, attr: str = None):
    """x, an array-like or a tensor of the unsigned `np_dtype` (uint8, uint32, uint64), as a flat
    contiguous tensor on `dev`, viewed as torch.uint8 / int32 / int64, of at least `count` entries
    (all of x: a caller that wants exactly `count` slices).  attr: unwrap x.attr first (a
    Deliveries' status or deliver_time_ns).  A non-tensor is cast through np.ascontiguousarray; a
    tensor must be non-floating and of the dtype's item size."""
    import torch

    if attr is not None:
        x = getattr(x, attr, x)
    np_dtype = np.dtype(np_dtype)
    t_dtype = getattr(torch, _TORCH_VIEW[np_dtype.itemsize])
    if isinstance(x, torch.Tensor):
        if x.is_floating_point() or x.element_size() != np_dtype.itemsize:
            raise ValueError(f"{what}: a {np_dtype.name} array")
        x = x.to(device=dev).reshape(-1).contiguous().view(t_dtype)
    else:
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np_dtype).ravel().view(_TORCH_VIEW[np_dtype.itemsize])).to(dev)
    if x.numel() < count:
        raise ValueError(f"{what}: a {np_dtype.name} array of {count} entries")
    return x


def weight_arg(weight, packets):
    """A round's `weight`: None, "payload" (the batch's payload_len) or an array, which passes."""
    if isinstance(weight, str):
        if weight != "payload":
            raise ValueError('weight: None, "payload" or an array')
        return packets.payload_len
    return weight


def member_weights(weight, packets, devs):
    """A group round's `weight` (None, "payload" or one array or None per member) as None or a list
    of `u32 tensor on devs[m], or None`, each of at least len(packets[m]) entries."""
    if weight is None:
        return None
    if isinstance(weight, str):
        weight = [weight_arg(weight, p) for p in packets]
    if len(weight) != len(packets):
        raise ValueError(f"weight: {len(weight)} entries for {len(packets)} members")
    return [None if w is None else int_tensor(w, np.uint32, len(packets[m]), devs[m], f"weight[{m}]")
            for m, w in enumerate(weight)]


def concat_weights(parts, packets, dev):
    """member_weights' list as one tensor on `dev` of a weight per packet of the batches in member
    order: each part cut to its member's packets, ones where a member gave None."""
    import torch

    if not parts:
        return None
    return torch.cat([torch.ones(len(p), dtype=torch.int32, device=dev) if w is None else w[:len(p)].to(dev)
                      for w, p in zip(parts, packets)]).contiguous()


def watch_mask(watch, n_links: int):
    """`watch` as a u8 numpy mask of one entry per link, or None: a bool array or a u8 array of
    shape (n_links,) is the mask; anything else is a list of link numbers."""
    if watch is None:
        return None
    w = np.asarray(watch)
    if w.dtype == np.bool_ or (w.dtype == np.uint8 and w.shape == (n_links,)):
        if w.shape != (n_links,):
            raise ValueError(f"watch: a mask of {n_links} entries, one per link")
        return np.ascontiguousarray(w.astype(np.uint8))
    idx = w.astype(np.int64).ravel()
    if len(idx) and (idx.min() < 0 or idx.max() >= n_links):
        raise ValueError(f"watch: link numbers below {n_links}")
    mask = np.zeros(n_links, np.uint8)
    mask[idx] = 1
    return mask


def with_capacity(n_items: int, alloc, call):
    """(rc, total, arrays) of call(arrays, cap) -> (rc, total) on arrays = alloc(cap): a first call at
    a guessed capacity, another at the total the last one reported while that was too small.  The
    caller checks rc."""
    cap = 8 * n_items + 64
    while True:
        arrays = alloc(cap)
        rc, total = call(arrays, cap)
        if rc != _capi.SG_ERR_CAPACITY or total <= cap:
            return rc, total, arrays
        cap = total


def series_out(out, n_slots: int, n_bins: int, contiguous: bool = True):
    """link_series_round's out=, a previous (series, outside), checked against this call's shape."""
    series, outside = out
    if (series.dtype != np.uint64 or outside.dtype != np.uint64 or series.shape != (n_slots, n_bins)
            or outside.shape != (n_slots, 2) or (contiguous and not (series.flags.c_contiguous and outside.flags.c_contiguous))):
        raise ValueError(f"out: a previous result of this shape, u64 ({n_slots}, {n_bins}) and ({n_slots}, 2)")
    return series, outside
