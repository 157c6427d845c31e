"""The hexahedral scatter planner on the CPU (csrc/sem_hex_plan.cpp, DESIGN.md
§5).

tools/hex_plan_check.cpp links the planner alone, plans a map from a file and
replays the plan thread by thread the way k_hex_poisson, k_hex_rows or
k_hex_mfma execute it, every value carrying its global node and the number of
(element, local node) pairs in it: every node must end at its reference count
after the plain stores and the seam sums, no node may have two plain stores or
a plain store and a slot, no slot two writers, every written slot must stand
in exactly one seam list, every hand-over in LDS (carry, z-merge, y-merge)
must have both its sides and they must name the same node.  Its JSON line also
carries a digest of every array sem_set_map uploads;
tests/golden/hex_plan_digests.json holds the digests of the planner as it was
when it still lived in sem_hex.hip, so a change of any plan shows up here,
without a GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from hex_meshes import permute_local

from spectralelementmethod_amd import _build, meshgen

SEM_E_INVALID, SEM_E_NOTIMPL = -1, -2  # include/sem_hip.h
PLAN_ENV = ["SEM_HEX_CHAIN", "SEM_HEX_CHAIN_START", "SEM_HEX_ROWS", "SEM_HEX_ZMERGE",
            "SEM_HEX_YMERGE", "SEM_HEX_TMAP"]
RESIDENT = 2  # few resident workgroups: the rule prefers whole chains (several steps, carries)
GRIDS = [(1, 8, 8), (2, 4, 7), (3, 4, 4), (4, 2, 5), (7, 2, 2)]  # p, slot grid rows x columns
# (z-merge, y-merge, form)
ZY, Z, PLAIN, ROWS_Z = (1, 1, "three_block"), (1, 0, "three_block"), (0, 0, "three_block"), \
    (1, 0, "rows")


def cube(nex, ney, nez, p):
    return meshgen.structured_cube(nex, ney, nez, p)[1]


def broken(kind, p):
    """the numberings of test_hex_broken_chains_vs_oracle (tests/test_gpu_hex.py)"""
    nodes, e2n = meshgen.structured_cube(4, 3, 3, p, warp=0.05)
    rng = np.random.default_rng(5)
    if kind in ("shuffle_elements", "reoriented_shuffled"):
        e2n = meshgen.shuffle_elements(e2n, seed=3)
    if kind == "shuffle_nodes":
        nodes, e2n = meshgen.shuffle_nodes(nodes, e2n, seed=4)
    if kind.startswith("reoriented"):
        e2n = permute_local(e2n, rng)
    return e2n


def periodic(p):
    """structured_cube(3, 2, 2, p), the nodes of the face x = hi replaced by
    those of x = lo: every xi0 chain is a cycle (the face x = hi holds the
    last ids, so the numbering stays dense)"""
    e2n = cube(3, 2, 2, p).astype(np.int64)
    plane = (2 * p + 1) ** 2
    return np.where(e2n >= 3 * p * plane, e2n - 3 * p * plane, e2n).astype(np.uint32)


def cases():
    """(id, mesh thunk, dict(flags, resident, env, extra_nodes), checks on the JSON)"""
    out = []

    def add(name, mesh, flags, resident=RESIDENT, env=None, extra_nodes=0, **expect):
        out.append((name, mesh, dict(flags=flags, resident=resident, env=env or {},
                                     extra_nodes=extra_nodes), expect))

    def tag(flags):
        return "%s-z%d-y%d" % (flags[2], flags[0], flags[1])

    # full slot grids, a grid cut short at the mesh edge and the 1-D fallback
    for p, gy, gz in GRIDS:
        mesh = lambda p=p, gy=gy, gz=gz: cube(3, 2 * gy + 1, gz + 1, p)
        for flags in (ZY, Z, PLAIN, ROWS_Z):
            add("grid-p%d-%s" % (p, tag(flags)), mesh, flags, tmap=True,
                **({"min_grid_wgs": 1} if flags is ZY else {"grid_wgs": 0}))
        # one layer fewer along xi1 and xi2: rows and grids end early
        add("short-grid-p%d-%s" % (p, tag(ZY)), lambda p=p, gy=gy, gz=gz: cube(3, 2 * gy, gz, p), ZY,
            tmap=True)
    # S = 3 (prime) and S = 2: no grid, the y-merge asked for or not
    for p in (8, 10):
        for flags in (ZY, ROWS_Z):
            add("nogrid-p%d-%s" % (p, tag(flags)), lambda p=p: cube(4, 3, 3, p), flags, grid_wgs=0,
                tmap=True)
    # one slot per workgroup; at n = 17 the last boundary column is bit 63
    for p in (11, 13, 16):
        for form in ("mfma", "rows"):
            add("oneslot-p%d-%s" % (p, form), lambda p=p: cube(3, 2, 2, p), (1, 0, form), tmap=True,
                **({"bit63": True} if p == 16 else {}))
    for kind in ("shuffle_elements", "shuffle_nodes", "reoriented", "reoriented_shuffled"):
        for p in (2, 5):
            expect = {"tmap": False} if kind == "shuffle_nodes" else {}
            add("%s-p%d" % (kind, p), lambda kind=kind, p=p: broken(kind, p), ZY if p == 2 else Z,
                **expect)
    # the sub-chain length: the rule at three device sizes, a forced cap, and
    # a mesh on which the rule reaches its own cap of 16 (16 chains of 32
    # elements, one resident workgroup: 2 generations x (16 + 1) is the minimum)
    for resident in (1, 4, 10 ** 6):
        add("chain-7x2x2-p3-resident%d" % resident, lambda: cube(7, 2, 2, 3), ZY, resident=resident,
            max_sub=16, tmap=True)
    for cap in (1, 2):
        add("chain-7x2x2-p3-cap%d" % cap, lambda: cube(7, 2, 2, 3), ZY,
            env={"SEM_HEX_CHAIN": str(cap)}, max_sub=cap, lc=cap, tmap=True)
    add("chain-32x4x4-p3-resident1", lambda: cube(32, 4, 4, 3), ZY, resident=1, max_sub=16, lc=16,
        tmap=True)
    add("chain-32x4x4-p3-cap5", lambda: cube(32, 4, 4, 3), ZY, env={"SEM_HEX_CHAIN": "5"}, max_sub=5,
        lc=5, tmap=True)
    # periodic along xi0: chains without a head, cut by the planner's second walk
    for p in (2, 4):
        add("cycle-p%d" % p, lambda p=p: periodic(p), ZY if p == 2 else Z, chains=4)
        add("cycle-p%d-cap2" % p, lambda p=p: periodic(p), ZY if p == 2 else Z,
            env={"SEM_HEX_CHAIN": "2"}, chains=4, max_sub=2, lc=2)
    add("unreferenced-p3", lambda: cube(3, 2, 2, 3), ZY, extra_nodes=6, n_zero=6, tmap=True)
    return out


CASES = cases()


def build_checker(exe, planner=None):
    """tools/hex_plan_check.cpp + csrc/sem_hex_plan.cpp with the library's compiler"""
    subprocess.run([_build.hipcc(), "-std=c++17", "-O2", "-Wall", "-I" + _build.CSRC,
                    os.path.join(ROOT, "tools", "hex_plan_check.cpp"),
                    planner or os.path.join(_build.CSRC, "sem_hex_plan.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("hex_plan_check") / "hex_plan_check"))


def run_checker(exe, workdir, e2n, n_node, flags=ZY, resident=RESIDENT, env=None):
    e2n = np.ascontiguousarray(e2n, dtype="<u4")
    path = os.path.join(str(workdir), "hex_map.bin")
    e2n.tofile(path)
    cmd = [exe, path, str(e2n.shape[1]), str(e2n.shape[0]), str(n_node), str(resident),
           str(flags[0]), str(flags[1]), flags[2]]
    full = {k: v for k, v in os.environ.items() if k not in PLAN_ENV}
    full.update(env or {})
    res = subprocess.run(cmd, env=full, check=True, capture_output=True, text=True)
    return json.loads(res.stdout)


def plan_case(exe, workdir, mesh, opts):
    e2n = mesh()
    return run_checker(exe, workdir, e2n, int(e2n.max()) + 1 + opts["extra_nodes"], opts["flags"],
                       opts["resident"], opts["env"])


@pytest.fixture(scope="session")
def golden_digests():
    with open(os.path.join(GOLDEN, "hex_plan_digests.json")) as f:
        return json.load(f)


_RESULTS = {}  # the slotted writes of the cases run so far, by name


@pytest.mark.parametrize("name,mesh,opts,expect", CASES, ids=[c[0] for c in CASES])
def test_hex_plan(checker, tmp_path, golden_digests, name, mesh, opts, expect):
    out = plan_case(checker, tmp_path, mesh, opts)
    assert out["rc"] == 0, out
    assert out["errors"] == [], out["errors"]
    _RESULTS[name] = out["n_seam_writes"]
    if "tmap" in expect:
        assert out["template_map"] == expect["tmap"], out
    if "grid_wgs" in expect:
        assert out["grid_wgs"] == expect["grid_wgs"], out
    if "min_grid_wgs" in expect:
        assert out["grid_wgs"] >= expect["min_grid_wgs"], out
    if expect.get("bit63"):
        assert out["cmask_bit63"] > 0, out
    if "max_sub" in expect:
        assert out["sub_len_max"] <= min(expect["max_sub"], out["lc"]), out
    if "lc" in expect:
        assert out["lc"] == expect["lc"], out
    if "chains" in expect:
        assert out["n_chains"] == expect["chains"], out
    if "n_zero" in expect:
        top = int(mesh().max()) + 1
        assert out["zero"] == list(range(top, top + expect["n_zero"])), out
    # cuts are near-equal
    assert out["sub_len_spread"] <= 1, out
    assert out["digests"] == golden_digests[name], "the plan of %s changed" % name


@pytest.mark.parametrize("p,gy,gz", GRIDS)
def test_hex_merges_save_slots(checker, tmp_path, p, gy, gz):
    """fewer slotted writes with each merge than without"""
    writes = []
    for flags in (ZY, Z, PLAIN):
        name = "grid-p%d-%s-z%d-y%d" % (p, flags[2], flags[0], flags[1])
        if name not in _RESULTS:
            case = next(c for c in CASES if c[0] == name)
            _RESULTS[name] = plan_case(checker, tmp_path, case[1], case[2])["n_seam_writes"]
        writes.append(_RESULTS[name])
    assert writes[0] < writes[1] < writes[2], writes


def test_hex_node_past_n_node(checker, tmp_path):
    e2n = cube(3, 2, 2, 3)
    out = run_checker(checker, tmp_path, e2n, int(e2n.max()))  # one node short
    assert out["rc"] == SEM_E_INVALID, out
    assert out["error"] == "element map entry >= n_node", out


def test_hex_repeated_element(checker, tmp_path):
    e2n = cube(3, 2, 2, 3)
    e2n = np.concatenate([e2n, e2n[-1:]])
    out = run_checker(checker, tmp_path, e2n, int(e2n.max()) + 1)
    assert out["rc"] == SEM_E_NOTIMPL, out
    assert out["error"] == ("hex plan: a node inside an element column is shared "
                            "(non-conforming mesh)"), out
