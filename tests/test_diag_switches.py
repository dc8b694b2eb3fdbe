"""The diagnostic switches are named in three places that nothing else ties together: the reads in the sources (diag_env / diag_env_int), the
list that decides which GNNCCA_* variable is reported as stale (csrc/pack.cpp: kDiagSwitches) and the table of DESIGN.md section 11.  Source
text only: no GPU, no library.
"""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "gnn-cca_amd", "csrc")
NOT_READ_IN_CSRC = {"GNNCCA_DIAG", "GNNCCA_LIB", "GNNCCA_STAMPS"}   # the gate itself (getenv), the Python side's, a build define's name


def _listed():
    text = open(os.path.join(CSRC, "pack.cpp")).read()
    body = re.search(r"kDiagSwitches\[\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    names = re.findall(r'"(GNNCCA_[A-Z0-9_]+)"', body)
    assert names and len(names) == len(set(names)), "kDiagSwitches is empty or names a switch twice"
    return set(names)


def _read():
    """name -> files, for every string literal handed to diag_env / diag_env_int; a call with anything else as its first argument fails."""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        text = open(path).read()
        for m in re.finditer(r"\bdiag_env(?:_int)?\s*\(\s*([^,)]*)", text):
            arg = m.group(1).strip()
            if arg.startswith("const char*"):   # the declarations and definitions
                continue
            if arg == "name" and os.path.basename(path) == "pack.cpp":   # diag_env_int hands its own parameter on
                continue
            lit = re.fullmatch(r'"(GNNCCA_[A-Z0-9_]+)"', arg)
            assert lit, f"{os.path.basename(path)}: diag_env called with {arg!r}, not a literal switch name"
            found.setdefault(lit.group(1), set()).add(os.path.basename(path))
    return found


def _documented():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("\n## 11. Diagnostic switches"):]
    nxt = sec.find("\n## ", 1)
    sec = sec if nxt < 0 else sec[:nxt]
    rows = [ln for ln in sec.splitlines() if ln.startswith("|")]
    assert rows[0].replace(" ", "") == "|variable|effect|" and set(rows[1]) <= set("|-"), "section 11 does not open with its table"
    # one table: every table row of the section is contiguous (a blank line inside would end the table for a renderer)
    lines = sec.splitlines()
    first = lines.index(rows[0])
    assert lines[first:first + len(rows)] == rows, "the table of section 11 is broken in two"
    names = []
    for ln in rows[2:]:
        names += re.findall(r"`(GNNCCA_[A-Z0-9_]+)`", ln.split("|")[1])
    assert len(names) == len(set(names)), "a switch is documented twice"
    return set(names)


def test_every_switch_the_sources_read_is_listed():
    listed, read = _listed(), _read()
    assert read, "no diag_env call found"
    missing = {n: sorted(f) for n, f in read.items() if n not in listed}
    assert not missing, f"read but not in kDiagSwitches (would be reported as stale when set): {missing}"


def test_every_listed_switch_is_read():
    dead = _listed() - NOT_READ_IN_CSRC - set(_read())
    assert not dead, f"in kDiagSwitches but read nowhere under csrc/: {sorted(dead)}"
    assert NOT_READ_IN_CSRC <= _listed()


def test_design_table_is_the_list():
    listed, documented = _listed(), _documented()
    assert documented == listed, f"only in DESIGN.md: {sorted(documented - listed)}; only in kDiagSwitches: {sorted(listed - documented)}"
