"""The environment variables the library reads are exactly those that
DESIGN.md's "Runtime switches" table lists: a new switch is a visible decision,
and a retired one leaves the table with its code."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_switches():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "dlsm_amd", "csrc", "*")):
        names.update(re.findall(r'getenv\(\s*"(DLSM_[A-Z0-9_]+)"', open(path).read()))
    return names


def documented_switches():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"\*\*Runtime switches\.\*\*.*?\n((?:\|[^\n]*\n)+)", txt, flags=re.S)
    assert m, "DESIGN.md has no Runtime switches table"
    rows = m.group(1).splitlines()[2:]  # past the header and its rule
    return {re.match(r"\|\s*`(DLSM_[A-Z0-9_]+)`", r).group(1) for r in rows}


def test_runtime_switches_match_design_table():
    src, doc = source_switches(), documented_switches()
    assert len(src) >= 5
    assert src == doc, f"only in the sources: {sorted(src - doc)}; only in DESIGN.md: {sorted(doc - src)}"
