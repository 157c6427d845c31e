"""The host side of the boundary faces on the CPU (csrc/sem_faces_plan.cpp,
Mesh.exterior_faces / tag_boundary / boundary_faces).

tools/faces_check.cpp links the planner alone: the face-order index tables
against the reference's node_ind (tests/golden/faces.npz) and against numpy
transposes written out from the convention, the node CSR of the Neumann
assembly, and the validation of (element, face) lists.  The float64 twin
(tests/faces_twin.py), the yardstick of the GPU tests, meets the reference's
goldens to 1e-12 relative, the bar of test_geometry_fields_golden."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden, rel_l2

import faces_twin
from spectralelementmethod_amd import _build, discrete, faces, grid_importers, meshgen

SEM_E_INVALID, SEM_E_NOTIMPL = -1, -2
CASES = ["sq_p2", "sq_p4", "sq_p8", "ann_p6", "sq_p4_rcm"]


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    """tools/faces_check.cpp + csrc/sem_faces_plan.cpp, built once with the library's compiler"""
    exe = str(tmp_path_factory.mktemp("faces_check") / "faces_check")
    subprocess.run([_build.hipcc(), "-std=c++17", "-O1", "-Wall", "-I" + _build.CSRC,
                    os.path.join(ROOT, "tools", "faces_check.cpp"),
                    os.path.join(_build.CSRC, "sem_faces_plan.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    res = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True)
    return json.loads(res.stdout)


def tables(exe, ndim, n):
    return np.array(run(exe, "tables", ndim, n)["table"]).reshape(2 * ndim, -1)


@pytest.fixture(scope="module")
def golden():
    return load_golden("faces.npz")


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_tables_give_the_reference_node_ind(checker, golden, name):
    e2n = golden[name + "_e2n"].astype(np.int64)
    E, n = e2n.shape[0], e2n.shape[1]
    t = tables(checker, 2, n)
    got = e2n.reshape(E, -1)[:, t].reshape(4 * E, n)   # (element, face) order
    assert np.array_equal(got, golden[name + "_face_node_ind"])


@pytest.mark.parametrize("n", [2, 3, 5, 17])
def test_tables_3d_are_the_stated_transposes(checker, n):
    lin = np.arange(n ** 3).reshape(n, n, n)
    # side 1: axes (axis+1, axis+2) mod 3; side 0: the reverse order
    expect = [lin[0, :, :].T,      # face 0: (xi2, xi1)
              lin[-1, :, :],       # face 1: (xi1, xi2)
              lin[:, 0, :],        # face 2: (xi0, xi2)
              lin[:, -1, :].T,     # face 3: (xi2, xi0)
              lin[:, :, 0].T,      # face 4: (xi1, xi0)
              lin[:, :, -1]]       # face 5: (xi0, xi1)
    t = tables(checker, 3, n)
    for f in range(6):
        assert np.array_equal(t[f], expect[f].ravel()), f
    assert np.array_equal(t, faces.face_index_table(3, n))
    assert np.array_equal(t, faces_twin.index_table(3, n))


@pytest.mark.parametrize("n", [2, 4, 9, 17])
def test_tables_2d_run_counter_clockwise(checker, n):
    lin = np.arange(n * n).reshape(n, n)
    expect = [lin[0, ::-1], lin[-1, :], lin[:, 0], lin[::-1, -1]]
    t = tables(checker, 2, n)
    for f in range(4):
        assert np.array_equal(t[f], expect[f]), f
    assert np.array_equal(t, faces.face_index_table(2, n))
    assert np.array_equal(t, faces_twin.index_table(2, n))
    # the end of each face is the start of the next one round the element
    for a, b in ((2, 1), (1, 3), (3, 0), (0, 2)):
        assert t[a][-1] == t[b][0]


def _csr_case(kind):
    if kind == "corner2d":      # element 0 of a square lists its two exterior sides
        _, e2n = meshgen.structured_square(3, 2, 3)
        elem, face = [0, 0], [0, 2]
    elif kind == "corner3d":    # a corner hexahedron lists its three exterior faces
        _, e2n = meshgen.structured_cube(2, 2, 2, 2)
        elem, face = [0, 0, 0], [0, 2, 4]
    elif kind == "duplicate":   # one face twice, and a neighbour's
        _, e2n = meshgen.structured_square(3, 2, 3)
        elem, face = [0, 1, 0], [0, 0, 0]
    else:
        _, e2n = meshgen.structured_square(3, 2, 3)
        elem, face = [], []
    ndim = e2n.ndim - 1
    t = faces.face_index_table(ndim, e2n.shape[1])
    flat = e2n.reshape(e2n.shape[0], -1)
    node = np.array([flat[e][t[f]] for e, f in zip(elem, face)], dtype="<u4").reshape(-1)
    return node


@pytest.mark.parametrize("kind,max_row", [("corner2d", 2), ("corner3d", 3), ("duplicate", 3),
                                          ("empty", 0)])
def test_csr_covers_every_entry_once(checker, tmp_path, kind, max_row):
    node = _csr_case(kind)
    path = str(tmp_path / "nodes.bin")
    node.tofile(path)
    out = run(checker, "csr", path)
    nd, ptr, ent = np.array(out["node"]), np.array(out["ptr"]), np.array(out["entry"])
    assert np.array_equal(np.sort(ent), np.arange(node.size))        # every (face, q) once
    assert np.array_equal(nd, np.unique(node))                       # sorted, distinct
    assert ptr[0] == 0 and ptr[-1] == node.size and ptr.size == nd.size + 1
    for r in range(nd.size):
        row = ent[ptr[r]:ptr[r + 1]]
        assert row.size >= 1 and np.all(np.diff(row) > 0)            # ascending (face, q)
        assert np.all(node[row] == nd[r])
    assert out["max_row"] == max_row
    if kind == "duplicate":
        # the node the two elements share on the doubled side gets 3 entries
        assert np.bincount(np.diff(ptr)).tolist()[1:] == [3, 3, 1]


def test_check_refuses_bad_pairs(checker, tmp_path):
    def call(ndim, p, n_elem, elem, face):
        a, b = str(tmp_path / "elem.bin"), str(tmp_path / "face.bin")
        np.asarray(elem, dtype="<i4").tofile(a)
        np.asarray(face, dtype=np.uint8).tofile(b)
        return run(checker, "check", ndim, p, n_elem, a, b)
    assert call(2, 4, 6, [0, 5, 5], [0, 3, 3])["rc"] == 0
    assert call(3, 16, 8, [7], [5])["rc"] == 0
    assert call(2, 4, 6, [], [])["rc"] == 0
    for bad in (call(2, 4, 6, [0, 6], [0, 0]), call(2, 4, 6, [-1], [0]),
                call(2, 4, 6, [0], [4]), call(3, 4, 6, [0], [6]), call(4, 4, 6, [0], [0]),
                call(2, 0, 6, [0], [0])):
        assert bad["rc"] == SEM_E_INVALID and bad["error"], bad
    assert call(2, 17, 6, [0], [0])["rc"] == SEM_E_NOTIMPL


# ---------------------------------------------------------------------------
def test_exterior_faces_square_and_cube():
    nex, ney = 5, 3
    mesh = discrete.Mesh.from_arrays(*meshgen.structured_square(nex, ney, 2))
    elem, face = mesh.exterior_faces()
    assert elem.size == 2 * (nex + ney)
    assert elem.dtype == np.int32 and face.dtype == np.uint8
    # element (ex, ey) = ex * ney + ey: face 0 at ex = 0, 1 at ex = nex - 1, 2 / 3 in y
    ex, ey = elem // ney, elem % ney
    on = np.where(face == 0, ex == 0, np.where(face == 1, ex == nex - 1,
                                               np.where(face == 2, ey == 0, ey == ney - 1)))
    assert on.all()
    a, b, c = 2, 3, 4
    mesh = discrete.Mesh.from_arrays(*meshgen.structured_cube(a, b, c, 2))
    elem, face = mesh.exterior_faces()
    assert elem.size == 2 * (a * b + b * c + c * a)
    assert np.bincount(face, minlength=6).tolist() == [b * c, b * c, a * c, a * c, a * b, a * b]
    # a single cell: all of its sides
    mesh = discrete.Mesh.from_arrays(*meshgen.structured_cube(1, 1, 1, 1))
    assert mesh.exterior_faces()[1].tolist() == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("name", ["sq_p2", "sq_p4", "sq_p8"])
def test_exterior_faces_are_the_tagged_sides_of_a_msh(name):
    mesh = grid_importers.load_msh(os.path.join(GOLDEN, "mesh_%s.msh" % name), 2)
    tagged = set()
    for b in ("ebc", "nbc"):
        e, f = mesh.boundary_faces(b)
        assert e.size and np.all(np.diff(e) >= 0)
        tagged |= set(zip(e.tolist(), f.tolist()))
    e, f = mesh.exterior_faces()
    assert set(zip(e.tolist(), f.tolist())) == tagged and e.size == len(tagged)


def test_tag_boundary_round_trip():
    mesh = discrete.Mesh.from_arrays(*meshgen.structured_square(3, 2, 2))
    elem, face = mesh.exterior_faces()
    top = face == 3
    mesh.tag_boundary("top", elem[top][::-1], face[top][::-1])     # any order in
    mesh.tag_boundary("rest", elem[~top], face[~top])
    e, f = mesh.boundary_faces("top")
    assert e.tolist() == sorted(elem[top].tolist()) and set(f.tolist()) == {3}
    e, f = mesh.boundary_faces("rest")                             # cells ascending, then
    assert list(zip(e.tolist(), f.tolist())) == \
        list(zip(elem[~top].tolist(), face[~top].tolist()))        # each cell's recorded order
    assert [c.node_ind_lexicographic.shape for c in mesh.cells_on_boundary("top")] == [(3, 3)] * 3
    with pytest.raises(ValueError):
        mesh.tag_boundary("top", [6], [0])
    with pytest.raises(ValueError):
        mesh.tag_boundary("top", [0], [4])


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_twin_meets_the_reference(golden, gll, name):
    from spectralelementmethod_amd.operators import _basis_arrays
    p = int(golden[name + "_p"])
    _, D, w, _ = _basis_arrays(p, None, 2)
    x_phys, e2n = golden[name + "_x_phys"], golden[name + "_e2n"]
    E = x_phys.shape[0]
    tw = faces_twin.Twin(x_phys, D, w, np.repeat(np.arange(E), 4), np.tile(np.arange(4), E))
    assert np.array_equal(tw.node_ind(e2n), golden[name + "_face_node_ind"])
    for key in ("x_phys", "n_dS", "dS", "dSxW", "unit_normal"):
        e = rel_l2(getattr(tw, key), golden[name + "_face_" + key])
        print("%s %s: twin to reference %.2e" % (name, key, e))
        assert e <= 1e-12, (key, e)
    g, _ = tw.gradient(golden[name + "_u"], e2n)
    assert rel_l2(g, golden[name + "_face_gradient"]) <= 1e-12
    assert rel_l2(tw.integrate(np.ones_like(tw.dS))[0], golden[name + "_face_integrate"]) <= 1e-12
    # the subface slice of the facade is the twin's
    for f in range(4):
        assert np.array_equal(faces.subface_slice(f, x_phys[0], 2),
                              faces_twin.face_slice(f, x_phys[0], 2))
