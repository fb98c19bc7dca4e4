"""The group's link loads and link trace through the layers: the export list, the built library's
symbols and the two Group methods.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_group_link_load_packets", "sg_group_link_trace_packets", "sg_group_last_error_member")


def test_exports_listed():
    from shadow_amd import _capi

    assert all(name in _capi.EXPORTED for name in NEW)


def test_symbols_exported():
    so = os.path.join(ROOT, "shadow_amd", "libshadow_gpu.so")
    assert os.path.exists(so), "libshadow_gpu.so is not built"
    if not shutil.which("nm"):
        pytest.skip("nm missing")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert all(name in have for name in NEW), [name for name in NEW if name not in have]


def test_python_methods():
    from shadow_amd import Group

    assert callable(getattr(Group, "link_load_round", None))
    assert callable(getattr(Group, "link_trace_round", None))
    assert callable(getattr(Group, "last_error_member", None))
