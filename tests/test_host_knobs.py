"""The library's environment switches live in ONE place: immesh_amd/csrc/host_knobs.hpp parses them when a context is created, nothing else under
csrc/ looks at the environment, and INTEGRATION.md's table lists exactly the switches parsed there.  Source-level checks: no GPU, no library."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "immesh_amd", "csrc")
KNOBS = os.path.join(CSRC, "host_knobs.hpp")

LISTED = {"IMMESH_DEBUG", "IMMESH_DEBUG_WAITS", "IMMESH_TRACE_FILE", "IMMESH_SPLIT_GENERAL", "IMMESH_NO_PRIORITY", "IMMESH_MESH_CUS", "IMMESH_RP_BLOCKS",
          "IMMESH_RP_FORCE_ABORT", "IMMESH_MATCH_SEQ", "IMMESH_HOST_EKF", "IMMESH_SERIAL_SAFE", "IMMESH_SERIAL_ORDER", "IMMESH_DS_RADIX", "IMMESH_DS_NO_GATE",
          "IMMESH_NO_GRAPH", "IMMESH_NO_SPLIT", "IMMESH_SPLIT", "IMMESH_MESH_ROOM", "IMMESH_NO_PIPELINE", "IMMESH_TRI_STREAM", "IMMESH_FUSED_WGS", "IMMESH_LIST_DIV",
          "IMMESH_MESH_GRID_DIV"}


def _parsed_switches():
    """the names handed to the parser: every quoted "IMMESH_*" literal of host_knobs.hpp (its comments name switches unquoted)"""
    return set(re.findall(r'"(IMMESH_[A-Z0-9_]+)"', open(KNOBS).read()))


def _documented_switches():
    """first column of the table that follows INTEGRATION.md's 'Environment switches' bullet; every row must say that the switch is read at create"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("* Environment switches of `libimmesh_hip.so`"):]
    names = set()
    started = False
    for line in table.splitlines()[1:]:
        row = line.strip()
        if not row.startswith("|"):
            if started:
                break
            continue
        started = True
        m = re.match(r"\|\s*`(IMMESH_[A-Z0-9_]+)`\s*\|", row)
        if m:
            assert row.rstrip("|").rstrip().endswith("at create"), row
            names.add(m.group(1))
    return names


def test_getenv_occurs_in_one_file_only():
    hits = []
    for d, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".cpp", ".hpp", ".hip", ".inc", ".h")) and "getenv(" in open(os.path.join(d, f), errors="replace").read():
                hits.append(os.path.relpath(os.path.join(d, f), CSRC))
    assert hits == ["host_knobs.hpp"], hits


def test_parsed_switches_are_the_documented_ones():
    assert _parsed_switches() == _documented_switches()


def test_no_switch_was_dropped():
    assert LISTED <= _parsed_switches(), sorted(LISTED - _parsed_switches())
