"""The environment switches of the library: what the sources read, what docs/SWITCHES.md lists and what the tree exercises are one set.

A switch selects a path; a path that no test, benchmark or tool runs is code nobody has executed since it was measured.  So a switch
exists only while something in the tree sets it, and the list in the document is the list in the sources."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]
PKG = ROOT / "gfdl_atmos_cubed_sphere_amd"
TOKEN = re.compile(r"FV3_MI355X_[A-Z0-9_]+")

# Switches nothing under tests/, tools/ or in bench.py names, each with the reason it may stay.
EXEMPT = {
    "FV3_MI355X_DEBUG_SEGMENTS": "a diagnostic print on stderr, not a path",
    "FV3_MI355X_FACE_GROUP": "Python host: the tests turn the face group off through cubed_dyn's argument, not the environment",
}


def _tokens(paths):
    found = set()
    for p in paths:
        found |= set(TOKEN.findall(p.read_text(errors="replace")))
    return found


def _source_switches():
    files = [p for p in PKG.rglob("*") if p.suffix in (".py", ".hip", ".h") and p.is_file()]
    return _tokens(files)


def _documented_switches():
    # the first cell of a table row: | `FV3_MI355X_NAME` ... | default | what it does |
    rows = re.findall(r"^\|\s*`(FV3_MI355X_[A-Z0-9_]+)`[^|]*\|", (ROOT / "docs" / "SWITCHES.md").read_text(), flags=re.M)
    assert len(rows) == len(set(rows)), "a switch has two rows in docs/SWITCHES.md"
    return set(rows)


def test_sources_and_document_list_the_same_switches():
    src, doc = _source_switches(), _documented_switches()
    assert src == doc, f"only in the sources: {sorted(src - doc)}; only in docs/SWITCHES.md: {sorted(doc - src)}"


def test_every_switch_is_exercised():
    users = [p for d in ("tests", "tools") for p in (ROOT / d).rglob("*") if p.is_file() and p.suffix in (".py", ".sh", ".hip", ".h", ".md")]
    users = [p for p in users if p.resolve() != pathlib.Path(__file__).resolve()]
    used = _tokens(users + [ROOT / "bench.py"])
    src = _source_switches()
    idle = src - used - set(EXEMPT)
    assert not idle, f"switches that no test, tool or bench.py names (retire them, or exercise them): {sorted(idle)}"
    stale = set(EXEMPT) - src
    assert not stale, f"exempted switches that no longer exist: {sorted(stale)}"
    assert not (set(EXEMPT) & used), f"exempted switches that are exercised after all: {sorted(set(EXEMPT) & used)}"
