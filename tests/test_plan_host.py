"""The 2-D scatter planner on the CPU (csrc/sem_plan.cpp).

tools/plan_check.cpp links the planner alone, plans a map from a file and
replays the plan in integers the way the kernels execute it: every node must
end at its reference count, no node may be written by two chains of a launch
or two waves of a round, no seam slot twice, the 16-bit map and its pattern
table must decode to the 32-bit map, and the bookkeeping (element positions,
zero list, owners) must be consistent.  Its JSON line also carries a digest of
every array the library uploads; tests/golden/plan_digests.json holds the
digests of the planner as it was first moved out of sem_device.hip, so a
change of any plan shows up here, without a GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from spectralelementmethod_amd import _build, meshgen

SEM_NODE_PRIOR, SEM_NODE_OTHER = 1, 2  # include/sem_hip.h
SEM_E_INVALID = -1
ORDERS = [2, 4, 8, 12, 16]
PLAN_ENV = ["SEM_CHAIN_ROUNDS", "SEM_BLOCK_ROUNDS", "SEM_SEAM", "SEM_PLAN", "SEM_MAP16",
            "SEM_MAP_PATTERNS", "SEM_CHAIN_SWIZZLE_MAX"]


def unstructured(kind, p):
    """make_mesh of tests/test_gpu_unstructured.py"""
    if kind.startswith("split_tri"):
        nodes, e2n = meshgen.quads_from_triangles(14, 11, p, seed=3)
        if kind != "split_tri":
            nodes, e2n = meshgen.shuffle_nodes(nodes, meshgen.shuffle_elements(e2n, 1), 2)
        if kind == "split_tri_rcm":
            nodes, e2n = meshgen.rcm_renumber(nodes, e2n)
        return e2n
    nodes, e2n = meshgen.structured_square(40, 30, p, warp=0.05)
    if kind == "shuffled_elems":
        return meshgen.shuffle_elements(e2n, 5)
    return meshgen.shuffle_nodes(nodes, e2n, 6)[1]


def square(nex, ney, p):
    return meshgen.structured_square(nex, ney, p)[1]


def strip_with_states():
    """structured_strip(7, 3, 4, 3, 7): its first node column holds a prior
    value; six unreferenced nodes follow, two of them another operator's"""
    nodes, e2n, _ = meshgen.structured_strip(7, 3, 4, 3, 7)
    n_ref = nodes.shape[1]
    state = np.zeros(n_ref + 6, dtype=np.uint8)
    state[:3 * 4 + 1] = SEM_NODE_PRIOR
    state[n_ref + 1] = state[n_ref + 4] = SEM_NODE_OTHER
    return e2n, state


def cases():
    """(id, mesh thunk, dict(dpn, mfma, env), checks on the JSON)"""
    out = []

    def add(name, mesh, env=None, dpn=1, mfma=0, **expect):
        out.append((name, mesh, dict(dpn=dpn, mfma=mfma, env=env or {}), expect))

    # 37 x 9: element lines of 9, shorter than a chain, so the chain patterns
    # break unless the block layout is forced; 9 x 37: lines of 37 (no multiple
    # of 4 * EPW), 9 of them (no multiple of 4 rounds): chains with merges,
    # carries and partly filled groups
    for nex, ney in ((37, 9), (9, 37)):
        for p in ORDERS:
            tag = "sq%dx%d-p%d" % (nex, ney, p)
            mesh = lambda nex=nex, ney=ney, p=p: square(nex, ney, p)
            for seam in ("0", "1", None):
                for br in ("0", "4", None):
                    env = {k: v for k, v in (("SEM_SEAM", seam), ("SEM_BLOCK_ROUNDS", br)) if v}
                    expect = {"atomic": 0}
                    chains = ney == 37 and p >= 8  # a chain is shorter than a line
                    if seam == "0" or (seam == "1" and chains):
                        expect["seam"] = int(seam)
                    if br == "0" or chains:
                        expect["blocks"] = int(br == "4")
                    if chains:
                        expect["ecol"] = 0
                    add("%s-seam%s-blocks%s" % (tag, seam, br), mesh, env, **expect)
            add(tag + "-rounds2", mesh, {"SEM_CHAIN_ROUNDS": "2"}, atomic=0)
    # 16 or more chains in one seam launch: chain_swizzle applies (lines of 64;
    # with lines of 16 and no blocks the plan is element-coloured instead)
    for nex, ney in ((64, 16), (24, 64)):
        for br in ("0", "4"):
            for swz in (None, "0"):
                env = {"SEM_SEAM": "1", "SEM_BLOCK_ROUNDS": br}
                if swz:
                    env["SEM_CHAIN_SWIZZLE_MAX"] = swz
                expect = {"seam": 1} if ney == 64 or br == "4" else {}
                add("sq%dx%d-p8-blocks%s-swizzle%s" % (nex, ney, br, swz),
                    lambda nex=nex, ney=ney: square(nex, ney, 8), env, atomic=0, min_chains=16,
                    **expect)
    for kind in ("split_tri", "split_tri_shuffled", "split_tri_rcm", "shuffled_elems",
                 "shuffled_nodes"):
        for p in (2, 4, 8):
            expect = {}
            if kind in ("split_tri", "split_tri_shuffled", "shuffled_elems"):
                expect = dict(ecol=1, atomic=0)
            if kind == "shuffled_nodes" and p == 8:
                expect = dict(map16=0)
            add("%s-p%d" % (kind, p), lambda kind=kind, p=p: unstructured(kind, p), **expect)
    for kind in ("shuffled_elems", "split_tri"):
        for plan in ("0", "1"):
            add("%s-p4-plan%s" % (kind, plan), lambda kind=kind: unstructured(kind, 4),
                {"SEM_PLAN": plan}, ecol=int(plan))
    for p in (4, 12):
        add("mfma-split_tri-p%d" % p, lambda p=p: unstructured("split_tri", p), mfma=1, atomic=0)
    for seam in ("0", "1"):
        add("mfma-sq9x7-p16-seam%s" % seam, lambda: square(9, 7, 16), {"SEM_SEAM": seam}, mfma=1,
            seam=int(seam), atomic=0)
    for seam in (None, "1"):
        env = {"SEM_SEAM": seam} if seam else {}
        add("dpn2-annulus-p6-seam%s" % seam, lambda: meshgen.annulus(4, 8, 6)[1], env, dpn=2,
            atomic=0)
        add("dpn2-sq37x9-p6-seam%s" % seam, lambda: square(37, 9, 6), env, dpn=2, atomic=0)
        add("dpn2-sq9x37-p6-seam%s" % seam, lambda: square(9, 37, 6), env, dpn=2, atomic=0,
            **({"seam": 1} if seam else {}))
    add("strip-states", strip_with_states, states=True)
    # a repeated element: every chain of the chain plan is atomic; left to
    # itself the planner then prefers the element-coloured plan, which puts the
    # two copies in different colours and needs no atomics
    twice = lambda: np.concatenate([square(6, 5, 4), square(6, 5, 4)[-1:]])
    add("nonconforming-chains", twice, {"SEM_PLAN": "0"}, conforming=0, min_atomic=1, ecol=0)
    add("nonconforming", twice, conforming=0, ecol=1)
    return out


CASES = cases()


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    """tools/plan_check.cpp + csrc/sem_plan.cpp, built once with the library's compiler"""
    exe = str(tmp_path_factory.mktemp("plan_check") / "plan_check")
    subprocess.run([_build.hipcc(), "-std=c++17", "-O2", "-Wall", "-I" + _build.CSRC,
                    os.path.join(ROOT, "tools", "plan_check.cpp"),
                    os.path.join(_build.CSRC, "sem_plan.cpp"), "-o", exe], check=True)
    return exe


def run_checker(exe, workdir, e2n, n_node, dpn=1, mfma=0, env=None, state=None):
    e2n = np.ascontiguousarray(e2n, dtype="<u4")
    path = os.path.join(str(workdir), "map.bin")
    e2n.tofile(path)
    cmd = [exe, path, str(e2n.shape[1]), str(e2n.shape[0]), str(n_node), str(dpn), str(mfma)]
    if state is not None:
        spath = os.path.join(str(workdir), "state.bin")
        np.ascontiguousarray(state, dtype=np.uint8).tofile(spath)
        cmd.append(spath)
    full = {k: v for k, v in os.environ.items() if k not in PLAN_ENV}
    full.update(env or {})
    res = subprocess.run(cmd, env=full, check=True, capture_output=True, text=True)
    return json.loads(res.stdout)


def plan_case(exe, workdir, mesh, opts):
    m = mesh()
    e2n, state = m if isinstance(m, tuple) else (m, None)
    n_node = int(e2n.max()) + 1 if state is None else state.size
    return run_checker(exe, workdir, e2n, n_node, state=state, **opts), state


@pytest.fixture(scope="session")
def golden_digests():
    with open(os.path.join(GOLDEN, "plan_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name,mesh,opts,expect", CASES, ids=[c[0] for c in CASES])
def test_plan(checker, tmp_path, golden_digests, name, mesh, opts, expect):
    out, state = plan_case(checker, tmp_path, mesh, opts)
    assert out["rc"] == 0, out
    assert out["errors"] == [], out["errors"]
    for key in ("seam", "blocks", "ecol", "map16", "conforming"):
        if key in expect:
            assert out[key] == expect[key], (key, out)
    if "atomic" in expect:
        assert out["n_atomic_groups"] == expect["atomic"], out
    if "min_atomic" in expect:
        assert out["n_atomic_groups"] >= expect["min_atomic"], out
    if "min_chains" in expect:  # enough chains for chain_swizzle to apply
        assert out["n_chains"] >= expect["min_chains"], out
    if opts["env"].get("SEM_CHAIN_ROUNDS") == "2" and not out["blocks"]:
        assert out["rounds"] == 2, out
    if expect.get("states"):
        # unreferenced nodes: the unmarked ones are zeroed, the marked ones are not
        free = np.flatnonzero(state == 0)
        free = free[free >= state.size - 6]
        assert out["zero"] == free.tolist() and len(free) == 4, out
    assert out["digests"] == golden_digests[name], "the plan of %s changed" % name


def test_node_past_n_node(checker, tmp_path):
    e2n = square(6, 5, 4)
    out = run_checker(checker, tmp_path, e2n, int(e2n.max()))  # one node short
    assert out["rc"] == SEM_E_INVALID, out
    assert out["error"] == "element map references node >= n_node", out
