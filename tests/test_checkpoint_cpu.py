"""Checkpoints without a device (include/immesh_checkpoint.h): the header is plain C, its symbols are exported, the binding's structs match the
compiler's, and immesh_checkpoint_probe accepts what tests/checkpoint_checker.py builds and names the fault of every file it refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import checkpoint_checker as ck
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_checkpoint.h")


@pytest.fixture(scope="module")
def lib():
    return capi.load_hip_library()


def _write(tmp_path, name, header, table, payloads, cut=0):
    raw = ck.assemble(header, table, payloads)
    p = tmp_path / name
    p.write_bytes(raw[:len(raw) - cut] if cut else raw)
    return str(p)


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "immesh_checkpoint.h"\nint main(void) { immesh_checkpoint_info i; immesh_checkpoint_section s; (void)i; (void)s; '
                   'return IMMESH_E_IO == -6 && IMMESH_E_FORMAT == -7 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_symbols_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    assert fns == ["immesh_checkpoint_load", "immesh_checkpoint_probe", "immesh_checkpoint_save"]
    assert not [f for f in fns if not hasattr(lib, f)]


def test_struct_layouts_match_the_compiler(tmp_path):
    fields = {"immesh_checkpoint_section": [n for n, _ in capi.CheckpointSection._fields_], "immesh_checkpoint_info": [n for n, _ in capi.CheckpointInfo._fields_]}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "immesh_checkpoint.h"', "int main(void) {"]
    for st, names in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        prog += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, n, st, n) for n in names]
    prog.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for st, cls in (("immesh_checkpoint_section", capi.CheckpointSection), ("immesh_checkpoint_info", capi.CheckpointInfo)):
        assert int(got[st]) == C.sizeof(cls)
        for n in fields[st]:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)
    assert C.sizeof(capi.CheckpointSection) == ck.SECTION_DTYPE.itemsize == 56 and C.sizeof(capi.CheckpointInfo) == 440
    assert (capi.E_IO, capi.E_FORMAT, capi.CHECKPOINT_VERSION) == (-6, -7, ck.VERSION)


def test_checksum_known_answer():
    """the definition, spelled out with Python integers on a 19-byte buffer (two words and a 3-byte tail), and its value"""
    data = bytes(range(1, 20))
    m = (1 << 64) - 1

    def mix(k):
        k ^= k >> 30; k = k * 0xbf58476d1ce4e5b9 & m
        k ^= k >> 27; k = k * 0x94d049bb133111eb & m
        return k ^ (k >> 31)

    words = [int.from_bytes(data[i:i + 8].ljust(8, b"\0"), "little") for i in range(0, len(data), 8)]
    want = sum(mix(w ^ (i * 0x9E3779B97F4A7C15 & m)) for i, w in enumerate(words)) & m
    assert ck.checksum(data) == want == 0xD692D23CF9BE3B3A
    assert ck.checksum(b"") == 0
    assert ck.checksum(data[8:], first_word=1) == (want - mix(words[0])) & m
    assert ck.checksum(np.frombuffer(data + b"\0" * 5, np.uint8)) == want   # zero padding of the tail is the definition


@pytest.mark.parametrize("regions,colour", [(False, False), (True, True)])
def test_probe_accepts_a_built_file(lib, tmp_path, regions, colour):
    cfg = capi.avia_config(cap_root_voxels=1 << 16, mesh_region=2.0)
    header, table, payloads = ck.build(cfg=cfg, has_regions=regions, has_colour=colour)
    path = _write(tmp_path, "ok.ckpt", header, table, payloads)
    info, secs = capi.checkpoint_probe(lib, path)
    assert (info["version"], info["n_sections"], info["has_regions"], info["has_colour"]) == (1, len(table), int(regions), int(colour))
    assert info["file_bytes"] == os.path.getsize(path) == int(header["file_bytes"])
    assert bytes(info["cfg"]) == bytes(cfg)
    assert (info["n_root_voxels"], info["n_nodes"], info["n_point_chunks"], info["n_free_chunks"], info["n_ext_tables"], info["n_leaf_chunks"]) == (3, 4, 5, 2, 1, 2)
    assert (info["n_vertices"], info["n_mesh_voxels"], info["n_triangles_pool"], info["n_triangles_live"], info["n_adj_chunks"], info["n_regions"]) == (7, 2, 5, 4, 3, int(regions))
    assert (info["scans_meshed"], info["map_updates"]) == (2, 2)
    assert [(s["name"], s["offset"], s["bytes"], s["records"], s["checksum"]) for s in secs] == \
        [(t["name"].decode(), int(t["offset"]), int(t["bytes"]), int(t["records"]), int(t["checksum"])) for t in table]
    names = [s["name"] for s in secs]
    assert ("rg.hash.ent" in names) == regions and ("cl.n_obs" in names) == colour and {"reg.nodes", "mesh.thash.slot", "host.state"} <= set(names)
    ck.read(path)   # the numpy reader agrees: every section's checksum, the header's


def _refused(lib, path, rc, pattern):
    with pytest.raises(capi.CheckpointError) as e:
        capi.checkpoint_probe(lib, path)
    assert e.value.rc == rc, (e.value.rc, e.value.msg)
    assert re.search(pattern, e.value.msg), e.value.msg


def test_probe_names_the_fault(lib, tmp_path):
    def variant(name, edit, rc=capi.E_FORMAT, pattern="", cut=0):
        header, table, payloads = ck.build()
        header, table = header.copy(), table.copy()
        edit(header, table)
        header["header_checksum"] = ck.header_checksum(header, table)   # (the fault is the edit, not a stale checksum)
        _refused(lib, _write(tmp_path, name, header, table, payloads, cut), rc, pattern)

    def magic(h, t): h["magic"] = b"IMMESHXX"
    def version(h, t): h["version"] = 2
    def record(h, t): h["rec"][0] += 1
    def past_end(h, t): t["offset"][-1] = h["file_bytes"] - 8
    def overlap(h, t): t["offset"][4] = t["offset"][3]   # reg.nodes onto reg.hash.ent

    variant("magic.ckpt", magic, pattern="magic")
    variant("version.ckpt", version, pattern="version 2")
    variant("record.ckpt", record, pattern=r"record size sizeof\(NodeRec\): file 385, library 384")
    variant("short.ckpt", lambda h, t: None, pattern="file length", cut=1)
    variant("past_end.ckpt", past_end, pattern="host.state runs past the end")
    variant("overlap.ckpt", overlap, pattern="reg.hash.ent and reg.nodes overlap")
    # further inconsistencies of the table and a stale header checksum
    variant("count.ckpt", lambda h, t: h["counts"].__setitem__(1, 5), pattern="sections inconsistent.*reg.nodes")
    header, table, payloads = ck.build()
    header = header.copy(); header["counts"][15] += 1
    _refused(lib, _write(tmp_path, "sum.ckpt", header, table, payloads), capi.E_FORMAT, "checksum mismatch in the header")
    (tmp_path / "tiny.ckpt").write_bytes(b"IMMESHCK")
    _refused(lib, str(tmp_path / "tiny.ckpt"), capi.E_FORMAT, "shorter than a checkpoint header")


def test_probe_missing_file(lib, tmp_path):
    _refused(lib, str(tmp_path / "nothing_here.ckpt"), capi.E_IO, "cannot open")
