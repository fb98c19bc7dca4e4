"""The device group without a device: the arguments sg_group_* rejects before it touches a
context, the new names in the header, the ctypes binding and the package, and the numpy statement
of the exchange (tests/group_ref.py) against hand cases.  tests/test_group_gpu.py runs the group
itself."""
import ctypes as C
import re

import numpy as np
import pytest

import group_ref
import shadow_amd
from shadow_amd import _capi
from shadow_amd.dist import RECORD_DTYPE, row_range

NEW = ["sg_group_create", "sg_group_destroy", "sg_group_size", "sg_group_last_error", "sg_group_last_error_pair",
       "sg_group_routing_info_fill", "sg_group_exchange_padded", "sg_group_alltoallv_records"]


@pytest.fixture(scope="module")
def L():
    return shadow_amd.load()  # dlopen and symbol lookup only


def _fake(n, repeat=None):
    """n distinct non-NULL `contexts` (addresses of a scratch buffer; the calls under test return
    before they would read one); repeat = (i, j): entry j is entry i again."""
    buf = (C.c_uint8 * (64 * max(n, 1)))()
    a = [C.addressof(buf) + 64 * i for i in range(n)]
    if repeat:
        a[repeat[1]] = a[repeat[0]]
    arr = (C.c_void_p * max(n, 1))(*a)
    arr._buf = buf
    return arr


def test_names_everywhere(L):
    hdr = open(_capi.HEADER_PATH).read()
    for name in NEW:
        assert name in _capi.EXPORTED and hasattr(L, name), name
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert getattr(L, name).argtypes is not None, name
    assert "typedef struct sg_group sg_group;" in hdr
    assert L.sg_abi_version() == 7  # additive
    from shadow_amd import Group, GroupDelivery  # noqa: F401
    from shadow_amd.group import GROUP_MAX

    assert GROUP_MAX == 64 and "Group" in shadow_amd.__all__ and "GroupDelivery" in shadow_amd.__all__


def test_create_rejects_bad_arguments(L):
    h = C.c_void_p(0xDEAD)
    assert L.sg_group_create(None, 2, C.byref(h)) == _capi.SG_ERR_INVALID_ARG
    assert h.value is None  # *out is cleared on failure
    assert L.sg_group_create(_fake(2), 2, None) == _capi.SG_ERR_INVALID_ARG
    for n in (0, 65):
        h = C.c_void_p(0xDEAD)
        assert L.sg_group_create(_fake(n), n, C.byref(h)) == _capi.SG_ERR_INVALID_ARG, n
        assert h.value is None
        assert b"1 .. 64" in L.sg_group_last_error(None)
    # a NULL member, a repeated member: found before any member is read
    arr = _fake(3)
    arr[1] = None
    assert L.sg_group_create(arr, 3, C.byref(h)) == _capi.SG_ERR_INVALID_ARG
    assert b"member 1 is NULL" in L.sg_group_last_error(None)
    assert L.sg_group_create(_fake(64, repeat=(5, 63)), 64, C.byref(h)) == _capi.SG_ERR_INVALID_ARG
    assert b"members 5 and 63 are the same context" in L.sg_group_last_error(None)
    assert h.value is None


def test_null_group(L):
    assert L.sg_group_size(None) == 0
    L.sg_group_destroy(None)
    r, c = C.c_uint32(7), C.c_uint32(7)
    L.sg_group_last_error_pair(None, C.byref(r), C.byref(c))
    assert (r.value, c.value) == (0, 0)
    assert L.sg_group_routing_info_fill(None, None, None, 0, None) == _capi.SG_ERR_INVALID_ARG
    assert L.sg_group_exchange_padded(None, None, None, 4, None, None) == _capi.SG_ERR_INVALID_ARG
    assert L.sg_group_alltoallv_records(None, None, None, None) == _capi.SG_ERR_INVALID_ARG


def test_python_group_reports_the_create_error():
    class NoContext:
        handle = None

    with pytest.raises(shadow_amd.ShadowGpuError) as e:
        shadow_amd.Group([])
    assert e.value.code == _capi.SG_ERR_INVALID_ARG and "1 .. 64" in str(e.value)
    with pytest.raises(shadow_amd.ShadowGpuError) as e:
        shadow_amd.Group([NoContext(), NoContext()])
    assert e.value.code == _capi.SG_ERR_INVALID_ARG and "member 0 is NULL" in str(e.value)


def _rec(tag, n):
    """n records whose every field names (tag, index): a misplaced record cannot pass."""
    r = np.zeros(n, RECORD_DTYPE)
    r["deliver_time_ns"] = tag * 1000 + np.arange(n)
    r["order_key"] = (np.uint64(tag) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    r["event_id"] = tag * 7 + np.arange(n)
    r["packet"] = np.arange(n)
    r["dst_host"] = tag
    return r


def test_ref_exchange_padded_by_hand():
    """2 members, cap 2: counts 0, 1 / 3 (over cap), 2."""
    cap = 2
    send = [_rec(10, 4), _rec(20, 4)]
    xrow = [np.array([5, 6, 7, 0, 1], np.uint64), np.array([8, 9, 10, 3, 2], np.uint64)]
    poison = _rec(99, 4)
    recv, xall = group_ref.exchange_padded(send, xrow, cap, [poison, poison])
    want_x = np.array([5, 6, 7, 0, 1, 8, 9, 10, 3, 2], np.uint64)
    assert all(np.array_equal(x, want_x) for x in xall) and len(xall) == 2
    # member 0: nothing from member 0 (count 0), min(3, 2) = 2 from member 1's block 0
    assert np.array_equal(recv[0][:2], poison[:2]) and np.array_equal(recv[0][2:], send[1][0:2])
    # member 1: one record of member 0's block 1 (slot 1 stays), two of member 1's block 1
    assert np.array_equal(recv[1][0], send[0][2]) and np.array_equal(recv[1][1], poison[1])
    assert np.array_equal(recv[1][2:], send[1][2:4])
    assert np.array_equal(poison, _rec(99, 4))  # the inputs are not written


def test_ref_alltoallv_by_hand():
    counts = [[2, 0, 1], [0, 0, 0], [1, 0, 3]]  # a zero row and a zero column
    send = [_rec(1, 3), _rec(2, 0), _rec(3, 4)]
    recv = group_ref.alltoallv(send, counts)
    assert np.array_equal(recv[0], np.concatenate([send[0][:2], send[2][:1]]))
    assert len(recv[1]) == 0
    assert np.array_equal(recv[2], np.concatenate([send[0][2:3], send[2][1:4]]))


def test_member_rows_are_dist_row_range():
    """The split the header restates in C for sg_group_routing_info_fill: per = ceil(n_used / n),
    member m = [min(m per, n_used), min((m + 1) per, n_used)).  301 rows over 2, 3 and 8 members end
    in a short block; 2 rows over 3 members leave the last member none."""
    for n_used, n in ((301, 1), (301, 2), (301, 3), (301, 8), (2, 3), (0, 4)):
        per = -(-n_used // n)
        got = [row_range(n_used, n, m)[:2] for m in range(n)]
        assert got == [(min(m * per, n_used), min((m + 1) * per, n_used)) for m in range(n)]
        assert got[0][0] == 0 and got[-1][1] == n_used and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    assert row_range(2, 3, 2)[:2] == (2, 2) and row_range(301, 8, 7)[:2] == (266, 301)
