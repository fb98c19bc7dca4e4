"""The exchange of a device group (sg_group_exchange_padded / sg_group_alltoallv_records,
include/shadow_gpu.h) stated in numpy: the two equations of the header and the concatenation of
the exact form.  Records are opaque 32-byte items (any dtype of that size); nothing looks inside
one.  tests/test_group_cpu.py checks these against hand cases, tests/test_group_gpu.py compares
the device against them."""
import numpy as np


def exchange_padded(send_padded, xrow, cap, recv_padded):
    """For n members: send_padded[b] holds n blocks of cap records (block r for member r), xrow[b]
    = [3 stats, count for member 0, 1, ...] (u64), recv_padded[r] is what member r's buffer held
    before.  Returns (recv, xall), one array per member:
        xall[r] = xrow[0] | xrow[1] | ... | xrow[n-1]
        recv[r][b*cap + k] = send_padded[b][r*cap + k]   for k < min(xrow[b][3 + r], cap)
    and every other slot of recv[r] as it was."""
    n = len(send_padded)
    assert len(xrow) == len(recv_padded) == n
    gathered = np.concatenate([np.asarray(x, np.uint64).reshape(3 + n) for x in xrow])
    recv = [np.array(r, copy=True) for r in recv_padded]
    for r in range(n):
        assert len(recv[r]) == n * cap
        for b in range(n):
            assert len(send_padded[b]) == n * cap
            k = min(int(xrow[b][3 + r]), cap)
            recv[r][b * cap:b * cap + k] = send_padded[b][r * cap:r * cap + k]
    return recv, [gathered.copy() for _ in range(n)]


def alltoallv(send, counts):
    """counts[b][r] = records member b holds for member r, grouped by r in send[b].  Returns what
    each member receives: its segment of every source, source after source."""
    counts = np.asarray(counts, np.int64)
    n = counts.shape[0]
    assert counts.shape == (n, n) and len(send) == n
    off = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(counts, axis=1)], axis=1)
    return [np.concatenate([send[b][off[b, r]:off[b, r + 1]] for b in range(n)]) for r in range(n)]
