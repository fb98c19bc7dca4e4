"""The link trace's entry point through the layers: the export list, the built library's symbol
and the two Python methods.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_listed():
    from shadow_amd import _capi

    assert "sg_link_trace_packets" in _capi.EXPORTED


def test_symbol_exported():
    so = os.path.join(ROOT, "shadow_amd", "libshadow_gpu.so")
    assert os.path.exists(so), "libshadow_gpu.so is not built"
    if not shutil.which("nm"):
        pytest.skip("nm missing")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "sg_link_trace_packets" in {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def test_python_methods():
    from shadow_amd import NetworkGraph
    from shadow_amd.graph import PathTree

    assert callable(getattr(PathTree, "link_trace_round", None))
    assert callable(getattr(NetworkGraph, "link_trace_packets_device", None))
