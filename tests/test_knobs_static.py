"""A machine check of the library's environment knobs: csrc/ reads the environment in one function only
(read_knobs in cdhip.hip, called once per handle by cdh_create), the variables it reads are exactly those the
LAB_NOTES.md table "Tuning knobs" lists, and the retired knobs, now fixed at their measured defaults, are gone
from the sources."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")
LAB_NOTES = os.path.join(ROOT, "LAB_NOTES.md")

RETIRED = ["CDH_NT", "CDH_STEP_GRID_PER_CU", "CDH_BLOCK_GRID_PER_CU", "CDH_GRAM_GRID_PER_CU", "CDH_GRAM32_GRID_PER_CU",
           "CDH_LT_PER_CU", "CDH_SMALL_ZEROCOPY", "CDH_CROSS_GX", "CDH_CROSS_BATCH", "CDH_CS_TABLE", "CDH_CS_FULL_CAP",
           "CDH_CS_FOLD_LIMIT", "CDH_COV_SOLVE_CLOCK"]


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".h", ".cpp")):
            yield name, open(os.path.join(CSRC, name)).read()


def _read_knobs_span():
    """(start, end) character offsets of read_knobs' definition in cdhip.hip, and its text."""
    txt = open(os.path.join(CSRC, "cdhip.hip")).read()
    m = re.search(r"^Knobs read_knobs\(\) \{$", txt, flags=re.M)
    assert m, "read_knobs() is not defined in cdhip.hip"
    end = txt.index("\n}\n", m.end()) + 3
    return m.start(), end, txt[m.start():end]


def _lab_notes_knobs():
    txt = open(LAB_NOTES).read()
    sec = txt[txt.index("### Tuning knobs"):]
    sec = sec[:sec.index("\n\nRetired")]
    names = set()
    for row in re.findall(r"^\| (`[^|]*) \|", sec, flags=re.M):
        names |= set(re.findall(r"\bCDH_[A-Z0-9_]+\b", row))
    return names


def test_getenv_only_in_read_knobs():
    start, end, _ = _read_knobs_span()
    stray = []
    for name, txt in _sources():
        for m in re.finditer(r"\bgetenv\b", txt):
            if not (name == "cdhip.hip" and start <= m.start() < end):
                stray.append(f"{name}:{txt.count(chr(10), 0, m.start()) + 1}")
    assert not stray, f"getenv outside read_knobs: {stray}"


def test_knobs_read_match_lab_notes_table():
    _, _, body = _read_knobs_span()
    read = set(re.findall(r'"(CDH_[A-Z0-9_]+)"', body))
    listed = _lab_notes_knobs()
    assert read, "read_knobs reads no CDH_* variable"
    assert read == listed, f"read but not in the table: {sorted(read - listed)}; in the table but not read: {sorted(listed - read)}"


def test_retired_knobs_are_gone():
    found = [(name, k) for name, txt in _sources() for k in RETIRED if re.search(r"\b%s\b" % k, txt)]
    assert not found, f"retired knobs still named in csrc/: {found}"
    assert not set(RETIRED) & _lab_notes_knobs()
