"""The cases of tests/stream_cases.py, qualified on the CPU: a green GPU run means something only
if a stale read (input set A where B was written behind the delay) or an unwritten output (the
poison) cannot equal the expected result.  For every case:

  - A and B have equal shapes and share their index-valued arrays bit for bit, so any mixture of
    the two is a valid input;
  - ref(A) != ref(B) in every output the GPU test compares;
  - the poison pattern occurs in no reference output (an output the library adds into starts
    from poison, so there the reference must be non-zero somewhere instead)."""
import numpy as np
import pytest

import stream_cases as ST

CASES = {c.name: c for c in ST.ALL_CASES}


def test_poison_values():
    assert ST.poison(np.uint8) == 0xA5 and ST.poison(np.uint32) == 0xA5A5A5A5
    assert ST.poison(np.uint64) == 0xA5A5A5A5A5A5A5A5 and np.isfinite(ST.poison(np.float32))
    assert ST.has_poison(np.uint32([1, 0xA5A5A5A5])) and not ST.has_poison(np.uint32([0xA5A5A500, 0xA5]))
    assert np.array_equal(ST.plus_poison(np.uint64([1, 1 << 63])), np.uint64([0xA5A5A5A5A5A5A5A6, 0x25A5A5A5A5A5A5A5]))


def test_every_case_has_a_name_of_its_own():
    assert len(CASES) == len(ST.ALL_CASES) and all(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_sets_share_shapes_and_index_arrays(name):
    c = CASES[name]
    a, b = c.sets()
    assert set(a) == set(b)
    differ = 0
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, k
        if k in c.INDEX:
            assert np.array_equal(x, y), f"{k}: an index array differs between A and B"
        else:
            differ += not np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert all(k in a for k in c.INDEX)
    assert differ or not c.STALE, "A and B are the same input"


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_stale_read_or_the_poison_cannot_pass(name):
    c = CASES[name]
    ra, rb = c.ref("A"), c.ref("B")
    assert set(ra) == set(rb) and rb
    for k in rb:
        assert ra[k].dtype == rb[k].dtype and (ra[k].shape == rb[k].shape or k in c.HOST_SIZED), k
        if c.STALE and k not in c.SAME and ra[k].shape == rb[k].shape:
            assert not np.array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8)), f"{k}: ref(A) == ref(B)"
        if k in c.PARTIAL:
            assert (rb[k] != ST.poison(rb[k].dtype)).any() and ST.has_poison(rb[k]), k
        elif k in c.ADDS:
            assert rb[k].any(), f"{k}: the library adds nothing into it"
        elif k in c.PADDED:
            n = int(rb[c.PADDED[k]][0])
            assert not ST.has_poison(rb[k][:n]) and ST.has_poison(rb[k][n:]), k
        else:
            assert not ST.has_poison(rb[k]), f"{k}: the poison occurs in the reference"


def test_every_entry_point_is_accounted_for():
    """stream_cases.COVERAGE names, for every exported entry point, the case that runs it on the
    caller's stream or the reason none does; a name given as a case is one."""
    from shadow_amd import _capi

    assert sorted(ST.COVERAGE) == sorted(_capi.EXPORTED)
    for fn, what in list(ST.COVERAGE.items()) + list(ST.NO_SYNC.items()):
        first = what.split(" ")[0]
        assert first in CASES or not first.replace("_", "").isalnum() or first in ("every", "host", "out", "not", "as"), (fn, what)
    assert all(ST.COVERAGE[fn].startswith(case) for fn, case in ST.NO_SYNC.items())
