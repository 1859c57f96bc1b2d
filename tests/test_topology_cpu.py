"""CPU tier of the mesh topology (include/immesh_topology.h): the header as plain C99, the library's new symbols, immesh_topology_stats' layout, and
the checker (tests/topology_checker.py) against closed forms, against an independent O(F^2) adjacency closure on random small soups, and against
scipy's connected components where scipy is installed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import topology_checker as tc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_topology.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_topology.h"\nint main(void) { immesh_topology_stats s; s.euler = IMMESH_EDGE_BOUNDARY; '
                   'return (int)s.euler + IMMESH_EDGE_NONMANIFOLD + IMMESH_EDGE_INCONSISTENT + IMMESH_E_INTERNAL + IMMESH_RAY_NEAREST; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_no_header_includes_it():
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "immesh_topology.h":
            assert "immesh_topology.h" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert '#include "immesh_raycast.h"' in open(HEADER).read()


def test_error_code_is_its_own():
    codes = {}
    for name in os.listdir(os.path.join(ROOT, "include")):
        for k, v in re.findall(r"#define (IMMESH_E_\w+)\s+\((-\d+)\)", open(os.path.join(ROOT, "include", name)).read()):
            codes[k] = int(v)
    assert codes["IMMESH_E_INTERNAL"] == capi.E_INTERNAL and list(codes.values()).count(codes["IMMESH_E_INTERNAL"]) == 1, codes


def test_library_exports_every_declared_symbol(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    for must in ("immesh_topology_analyse", "immesh_topology_faces", "immesh_topology_components", "immesh_topology_edges", "immesh_topology_select",
                 "immesh_topology_last_timing"):
        assert must in fns
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_stats_layout(tmp_path):
    names = [n for n, _ in capi.TopologyStats._fields_]
    assert tuple(names) == tc.STAT_NAMES
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_topology.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_topology_stats));\n'
                    + "".join('  printf(" %%zu", offsetof(immesh_topology_stats, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.TopologyStats)] + [getattr(capi.TopologyStats, n).offset for n in names]
    assert got == [112] + [8 * i for i in range(14)]
    declared = re.findall(r"int64_t (\w+);", re.search(r"typedef struct immesh_topology_stats \{(.*?)\}", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S), re.S).group(1))
    assert declared == names
    assert (capi.EDGE_BOUNDARY, capi.EDGE_NONMANIFOLD, capi.EDGE_INCONSISTENT) == (tc.EDGE_BOUNDARY, tc.EDGE_NONMANIFOLD, tc.EDGE_INCONSISTENT)
    for name, val in (("IMMESH_EDGE_BOUNDARY", 0), ("IMMESH_EDGE_NONMANIFOLD", 1), ("IMMESH_EDGE_INCONSISTENT", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), open(HEADER).read())


# ---- closed forms (CLOSED_FORMS is shared with the device tier: every case is run there too) ------------------------------------------------------
def _two_tetrahedra(shared):
    """two tetrahedra with `shared` common vertices (1: a vertex, 2: an edge)"""
    v0, f0 = tc.tetrahedron()
    v1, f1 = tc.tetrahedron((3.0, 0.0, 0.0))
    remap = np.arange(4) + 4
    remap[:shared] = np.arange(shared)                                                 # the second one's first vertices are the first one's
    return np.concatenate([v0, v1]), np.concatenate([f0, remap[f1].astype(np.int32)])


HOLES = [(1, 1), (3, 2), (5, 5), (1, 6)]                                                # separate: no two share a vertex
CLOSED_FORMS = {
    "one face": (lambda: (np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], np.int32)),
                 dict(n_counting=1, n_vertices_used=3, n_edges=3, n_boundary=3, n_interior=0, n_components=1, n_boundary_loops=1, largest_loop_edges=3, euler=1)),
    "two faces wound against each other": (lambda: (np.zeros((4, 3), np.float32), np.array([[0, 1, 2], [1, 2, 3]], np.int32)),
                                           dict(n_inconsistent=1, n_interior=1, n_boundary=4, n_components=1, euler=1)),
    "two faces wound alike": (lambda: (np.zeros((4, 3), np.float32), np.array([[0, 1, 2], [2, 1, 3]], np.int32)),
                              dict(n_inconsistent=0, n_interior=1, n_boundary=4, n_components=1, euler=1)),
    "tetrahedron": (tc.tetrahedron, dict(euler=2, n_boundary=0, n_components=1, n_inconsistent=0, n_nonmanifold=0, n_boundary_loops=0, n_edges=6)),
    "grid sheet 7 x 5": (lambda: tc.grid_sheet(7, 5), dict(n_vertices_used=8 * 6, n_edges=3 * 35 + 12, n_boundary=2 * 12, euler=1, n_boundary_loops=1,
                                                           largest_loop_edges=24, n_components=1, n_inconsistent=0, n_counting=70)),
    "grid sheet 8 x 8 with 4 holes": (lambda: tc.grid_sheet(8, 8, HOLES), dict(euler=1 - 4, n_boundary_loops=1 + 4, n_boundary=32 + 16, largest_loop_edges=32,
                                                                               n_components=1, n_inconsistent=0, n_vertices_used=81)),
    "torus 16 x 16": (lambda: tc.torus(16, 16), dict(euler=0, n_boundary=0, n_components=1, n_inconsistent=0, n_nonmanifold=0, n_counting=512)),
    "moebius band": (lambda: tc.moebius(9), dict(n_components=1, n_boundary_loops=1, n_nonmanifold=0, euler=0)),
    "two tetrahedra sharing a vertex": (lambda: _two_tetrahedra(1), dict(n_components=2, n_vertices_used=7, n_boundary=0, euler=3)),
    "two tetrahedra sharing an edge": (lambda: _two_tetrahedra(2), dict(n_components=1, n_nonmanifold=1, n_vertices_used=6, n_edges=11, n_boundary=0)),
}


def check_closed_form(name, st, edges):
    """st: a dict of the stats; edges: kind -> (uv, uses)"""
    want = CLOSED_FORMS[name][1]
    assert {k: st[k] for k in want} == want, (name, st)
    assert st["n_edges"] == st["n_boundary"] + st["n_interior"] + st["n_nonmanifold"] and st["n_inconsistent"] <= st["n_interior"]
    assert st["euler"] == st["n_vertices_used"] - st["n_edges"] + st["n_counting"] and st["n_degenerate"] == st["n_faces"] - st["n_counting"]
    if name == "moebius band":
        assert st["n_inconsistent"] >= 1
    if name == "two tetrahedra sharing an edge":
        assert edges[tc.EDGE_NONMANIFOLD][0].tolist() == [[0, 1]] and edges[tc.EDGE_NONMANIFOLD][1].tolist() == [4]
    if name == "two faces wound against each other":
        assert edges[tc.EDGE_INCONSISTENT][0].tolist() == [[1, 2]] and edges[tc.EDGE_INCONSISTENT][1].tolist() == [2]
    if name == "one face":
        assert edges[tc.EDGE_BOUNDARY][0].tolist() == [[0, 1], [0, 2], [1, 2]] and edges[tc.EDGE_BOUNDARY][1].tolist() == [1, 1, 1]


@pytest.mark.parametrize("name", list(CLOSED_FORMS))
def test_checker_closed_forms(name):
    vtx, faces = CLOSED_FORMS[name][0]()
    res = tc.analyse(vtx, faces)
    check_closed_form(name, res["stats"], res["edges"])
    assert res["comp"].min() >= 0 and res["n_faces"].sum() == len(faces) and res["n_boundary"].sum() == res["stats"]["n_boundary"]


def test_checker_degenerate_duplicate_and_boxes():
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 5, -0.0], [7, np.inf, 2], [1, 1, 1], [2, 2, 2], [3, 3, 3]], np.float32)
    faces = np.array([[0, 1, 1], [0, 1, 2], [0, 1, 2], [5, 5, 5], [3, 4, 5], [6, 7, 6]], np.int32)
    res = tc.analyse(vtx, faces)
    st = res["stats"]
    assert (st["n_counting"], st["n_degenerate"], st["n_components"], st["n_vertices_used"]) == (3, 3, 2, 6)
    assert res["comp"].tolist() == [-1, 0, 0, -1, 1, -1] and res["first_face"].tolist() == [1, 4] and res["n_faces"].tolist() == [2, 1]
    assert st["n_edges"] == 6 and st["n_interior"] == 3 and st["n_inconsistent"] == 3 and st["n_boundary"] == 3     # the duplicate: three edges used twice, alike
    assert res["box"][0].tolist() == [0, 0, 0, 1, 1, 0]
    assert res["box"][1].tolist() == [1, 1, 0, 7, 5, 2]                                  # the finite floats of (nan, 5, -0), (7, inf, 2), (1, 1, 1)
    keep, kept = tc.select(res, faces, min_faces=2)
    assert keep.tolist() == [0, 1, 1, 0, 0, 0] and kept.tolist() == [[0, 1, 2], [0, 1, 2]]
    assert tc.select(res, faces, keep_largest=1)[0].tolist() == [0, 1, 1, 0, 0, 0]
    assert tc.select(res, faces, min_diagonal=1.25)[0].tolist() == [0, 1, 1, 0, 1, 0]
    assert tc.select(res, faces, min_diagonal=1.5)[0].tolist() == [0, 0, 0, 0, 1, 0]
    # a component without a finite float in some coordinate fails any positive diagonal, passes a zero one
    vtx2 = np.array([[np.nan, 0, 0], [np.nan, 1, 0], [np.inf, 0, 1]], np.float32)
    res2 = tc.analyse(vtx2, [[0, 1, 2]])
    assert res2["box"][0].tolist() == [np.inf, 0, 0, -np.inf, 1, 1]
    assert tc.select(res2, [[0, 1, 2]], min_diagonal=1e-30)[0].tolist() == [0] and tc.select(res2, [[0, 1, 2]])[0].tolist() == [1]
    # nothing at all
    empty = tc.analyse(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert all(v == 0 for v in empty["stats"].values()) and len(empty["comp"]) == 0


# ---- independent cross-checks ----------------------------------------------------------------------------------------------------------------------
def _closure(faces):
    """O(F^2): the adjacency matrix of counting faces by a shared edge, closed under composition -> the smallest face index of every class (-1)"""
    F = [tuple(int(x) for x in f) for f in faces]
    n = len(F)
    counting = [len(set(f)) == 3 for f in F]
    sets = [{frozenset((f[k], f[(k + 1) % 3])) for k in range(3)} for f in F]
    adj = np.eye(n, dtype=bool)
    for i in range(n):
        for j in range(i + 1, n):
            if counting[i] and counting[j] and sets[i] & sets[j]:
                adj[i, j] = adj[j, i] = True
    while True:
        nxt = (adj.astype(np.int32) @ adj.astype(np.int32)) > 0
        if np.array_equal(nxt, adj):
            break
        adj = nxt
    return np.array([int(np.argmax(adj[i])) if counting[i] else -1 for i in range(n)])


@pytest.mark.parametrize("seed", range(6))
def test_checker_against_adjacency_closure(seed):
    rng = np.random.default_rng(300 + seed)
    vtx, faces = tc.random_soup(rng, int(rng.integers(1, 120)), n_vtx=int(rng.integers(5, 40)))
    res = tc.analyse(vtx, faces)
    label = _closure(faces)
    want = np.array([-1 if l < 0 else sorted(set(label[label >= 0].tolist())).index(l) for l in label])
    assert np.array_equal(res["comp"], want)
    assert res["first_face"].tolist() == sorted(set(label[label >= 0].tolist()))
    # the edge classes by a dictionary of uses
    uses = {}
    for f in faces.tolist():
        if len(set(f)) == 3:
            for k in range(3):
                a, b = f[k], f[(k + 1) % 3]
                uses.setdefault((min(a, b), max(a, b)), []).append(a < b)
    st = res["stats"]
    assert st["n_edges"] == len(uses) and st["n_boundary"] == sum(len(u) == 1 for u in uses.values()) and st["n_nonmanifold"] == sum(len(u) >= 3 for u in uses.values())
    assert st["n_inconsistent"] == sum(len(u) == 2 and u[0] == u[1] for u in uses.values())
    assert res["edges"][tc.EDGE_NONMANIFOLD][0].tolist() == [list(e) for e in sorted(uses) if len(uses[e]) >= 3]
    assert res["edges"][tc.EDGE_NONMANIFOLD][1].tolist() == [len(uses[e]) for e in sorted(uses) if len(uses[e]) >= 3]


def test_checker_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(77)
    vtx, faces = tc.sheet_with_fragments(rng, 40, 30, 25, 60)
    faces = np.concatenate([faces, tc.random_soup(rng, 50, 30)[1] + 100]).astype(np.int32)
    res = tc.analyse(vtx, faces)
    # faces and edges as one bipartite graph
    F = faces.astype(np.int64)
    cf = np.nonzero((F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2]))[0]
    a, b = F[cf].reshape(-1), F[cf][:, [1, 2, 0]].reshape(-1)
    _, eid = np.unique(np.minimum(a, b) * (1 << 32) + np.maximum(a, b), return_inverse=True)
    n = len(faces) + eid.max() + 1
    g = sp.coo_matrix((np.ones(len(eid)), (np.repeat(cf, 3), len(faces) + eid)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    lab = lab[:len(faces)]
    assert len(set(lab[cf].tolist())) == res["stats"]["n_components"] > 60
    for c in range(res["stats"]["n_components"]):
        assert len(set(lab[res["comp"] == c].tolist())) == 1
    # the loops: the boundary edges' graph
    bu = res["edges"][tc.EDGE_BOUNDARY][0]
    nv = int(bu.max()) + 1
    n_all, lab_v = connected_components(sp.coo_matrix((np.ones(len(bu)), (bu[:, 0], bu[:, 1])), shape=(nv, nv)), directed=False)
    assert len(set(lab_v[bu[:, 0]].tolist())) == res["stats"]["n_boundary_loops"]
    assert np.bincount(lab_v[bu[:, 0]]).max() == res["stats"]["largest_loop_edges"]
