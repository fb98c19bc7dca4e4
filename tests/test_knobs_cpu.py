"""The SG_* environment knobs, mechanically: shadow_amd/csrc/sg_knobs.h lists every knob once
and holds the only getenv calls for them; DESIGN.md's "Knobs" appendix has one row per knob.

Text only (nothing is built or loaded):
  * no other file of shadow_amd/csrc calls getenv with an SG_ name, and every knob a source
    file reads through the header's readers is in the header's list;
  * every knob the tests, tests/conftest.py or bench.py name (the routing, build, tree, link-load,
    tree-path, delivery, lane and parser prefixes below) is in the list: a test cannot set a knob the library dropped;
  * the list and the appendix name the same knobs.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shadow_amd", "csrc")
HEADER = os.path.join(CSRC, "sg_knobs.h")
DESIGN = os.path.join(ROOT, "DESIGN.md")

PREFIXES = ("SG_APSP_", "SG_SSSP_", "SG_DENSE_", "SG_BUCKET_", "SG_BAND_", "SG_NET_", "SG_PLAN_", "SG_LANE_",
            "SG_RI_", "SG_GML_", "SG_TREE_", "SG_LINK_", "SG_PATHS_", "SG_BUILD_")
NAME = r"SG_[A-Z0-9]+(?:_[A-Z0-9]+)+"
KINDS = {"test", "tune", "diag"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _header_knobs():
    """name -> (default, range, kind, what) from the header's list."""
    knobs = {}
    for line in _read(HEADER).splitlines():
        m = re.match(rf"^//\s+({NAME}) \| (.+?) \| (.+?) \| (\w+) \| (.+)$", line)
        if m:
            assert m.group(1) not in knobs, f"{m.group(1)} is listed twice in sg_knobs.h"
            knobs[m.group(1)] = m.groups()[1:]
    return knobs


def _design_rows():
    text = _read(DESIGN)
    m = re.search(r"^## Appendix: Knobs\n(.*?)(?=^## |\Z)", text, flags=re.S | re.M)
    assert m, "DESIGN.md has no '## Appendix: Knobs' section"
    rows = re.findall(rf"^\| `({NAME})` \|", m.group(1), flags=re.M)
    assert len(rows) == len(set(rows)), "a knob has two rows in DESIGN.md's appendix"
    return set(rows)


def test_header_lists_knobs():
    knobs = _header_knobs()
    assert len(knobs) >= 40
    for name, (dflt, rng, kind, what) in knobs.items():
        assert kind in KINDS, f"{name}: kind {kind!r}"
        assert dflt.strip() and rng.strip() and what.strip(), name


def test_getenv_only_in_header():
    knobs = _header_knobs()
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not path.endswith((".hip", ".cpp", ".h")) or path == HEADER:
            continue
        src = _read(path)
        bad = re.findall(r"getenv\s*\(\s*\"(SG_[A-Z0-9_]*)\"", src)
        assert not bad, f"{os.path.basename(path)} calls getenv for {bad}: read it through sg_knobs.h"
        for name in re.findall(rf"knob_(?:int|double|str|off)\s*\(\s*\"({NAME})\"", src):
            assert name in knobs, f"{os.path.basename(path)} reads {name}, which sg_knobs.h does not list"
    # the header's readers are the only getenv calls there are for SG_ names; they take the name
    assert re.search(r"getenv\(name\)", _read(HEADER))


def test_knobs_the_tests_set_exist():
    knobs = _header_knobs()
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) + [os.path.join(ROOT, "bench.py")]
    assert os.path.join(ROOT, "tests", "conftest.py") in files
    me = os.path.abspath(__file__)
    for path in files:
        if os.path.abspath(path) == me:
            continue
        for name in set(re.findall(NAME, _read(path))):
            if name.startswith(PREFIXES):
                assert name in knobs, f"{os.path.relpath(path, ROOT)} names {name}, which sg_knobs.h does not list"


def test_design_appendix_matches_header():
    knobs, rows = set(_header_knobs()), _design_rows()
    assert knobs - rows == set(), f"no row in DESIGN.md's Knobs appendix: {sorted(knobs - rows)}"
    assert rows - knobs == set(), f"rows in DESIGN.md's Knobs appendix without a knob: {sorted(rows - knobs)}"
