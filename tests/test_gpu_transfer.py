"""GPU tests of the order transfer (transfer.Transfer, sem_transfer_* in
include/sem_hip.h) against the np.longdouble twin of the
stated definition (tests/transfer_twin.py, itself checked on the CPU in
tests/test_transfer_host.py) and against identities: polynomial exactness,
conservation of the load, round trips, repeatability, renumbering.

The meshes are 3 x 2 quadrilaterals and 2 x 2 x 2 hexahedra with warp 0.05,
the "to" nodes shuffled, on hexahedra the local axes of half the elements
re-oriented the same way on both sides (tests/transfer_twin.mesh_pair).
The bar against the twin is the project's parity bar, 1e-12 relative L2."""
import numpy as np
import pytest

from conftest import rel_l2

import transfer_twin as tw
from transfer_twin import mesh, mesh_pair

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL_PARITY = 1e-12
PAIRS_2D = [(1, 2), (2, 1), (3, 16), (16, 15), (4, 8), (8, 4), (7, 7)]
PAIRS_3D = [(1, 2), (2, 4), (4, 3), (8, 16), (16, 16)]
CASES = [(2, a, b) for a, b in PAIRS_2D] + [(3, a, b) for a, b in PAIRS_3D]


@pytest.fixture(scope="module")
def tmod():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from spectralelementmethod_amd import transfer
    return transfer


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def make(tmod, ndim, p_from, p_to, warp=0.05, pad=(0, 0)):
    """(Transfer, twin, n_node_from, n_node_to) of a mesh pair; ``pad`` adds
    nodes no element references to either side."""
    (nf, ef), (nt, et) = mesh_pair(ndim, p_from, p_to, warp=warp)
    nnf, nnt = nf.shape[1] + pad[0], nt.shape[1] + pad[1]
    return tmod.Transfer(ef, nnf, et, nnt), tw.Twin(ef, nnf, et, nnt), nnf, nnt


# --------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("ndim,p_from,p_to", CASES)
def test_prolong_and_restrict_match_the_twin(tmod, ndim, p_from, p_to):
    t, twin, nnf, nnt = make(tmod, ndim, p_from, p_to)
    rng = np.random.default_rng(11)
    u, r = rng.standard_normal(nnf), rng.standard_normal(nnt)
    e_p = rel_l2(t.prolong(u), twin.prolong(u).astype(np.float64))
    e_r = rel_l2(t.restrict(r), twin.restrict(r).astype(np.float64))
    print("ndim %d p %d -> %d: prolong to twin %.2e, restrict to twin %.2e"
          % (ndim, p_from, p_to, e_p, e_r))
    assert e_p <= TOL_PARITY and e_r <= TOL_PARITY, (e_p, e_r)
    info = t.info()
    assert (info["ndim"], info["p_from"], info["p_to"]) == (ndim, p_from, p_to)
    assert info["owned_entries"] == nnt and info["max_contributions"] == 2 ** ndim
    assert info["scratch_bytes"] == 2 * 8 * info["elements"] * (p_from + 1) ** ndim


# --------------------------------------------------------------------------- identities
@pytest.mark.parametrize("ndim,p_from,p_to", [(d, a, b) for d in (2, 3)
                                              for a, b in ((1, 2), (2, 1), (4, 8), (16, 15))])
def test_polynomials_are_prolonged_exactly(tmod, ndim, p_from, p_to):
    (nf, ef), (nt, et) = mesh_pair(ndim, p_from, p_to)          # unwarped
    deg = min(p_from, p_to)
    u = tw.product_polynomial(tw.gll_points(nf, ef), deg).astype(np.float64)
    ref = tw.product_polynomial(tw.gll_points(nt, et), deg).astype(np.float64)
    t = tmod.Transfer(ef, nf.shape[1], et, nt.shape[1])
    err = rel_l2(t.prolong(u), ref)
    print("ndim %d p %d -> %d: polynomial of degree %d prolonged to %.2e"
          % (ndim, p_from, p_to, deg, err))
    assert err <= TOL_PARITY


@pytest.mark.parametrize("ndim,p_from,p_to", [(2, 1, 2), (2, 4, 8), (3, 1, 2), (3, 4, 8)])
def test_restrict_conserves_the_load(tmod, ndim, p_from, p_to):
    """P^T of the assembled order-p_to detJxW is the assembled order-p_from
    detJxW: both quadratures integrate a degree-p_from basis function
    exactly.  Operators, their own geometry and transfer_to."""
    from spectralelementmethod_amd.operators import SEMOperator
    ops = [SEMOperator(p, *mesh(ndim, p)[::-1], device="cuda:0") for p in (p_from, p_to)]
    loads = [op.assemble(op.geometry_fields()["detJxW"]) for op in ops]
    t = ops[0].transfer_to(ops[1])
    err = rel_l2(t.restrict(loads[1]).cpu().numpy(), loads[0].cpu().numpy())
    print("ndim %d p %d -> %d: load restricted to %.2e" % (ndim, p_from, p_to, err))
    assert err <= TOL_PARITY
    assert abs(float(loads[0].sum()) - 2.0 ** ndim) <= 1e-12


@pytest.mark.parametrize("ndim,p,q", [(2, 4, 8), (2, 3, 16), (3, 2, 4)])
def test_round_trip_returns_the_input(tmod, ndim, p, q):
    (nf, ef), (nt, et) = mesh_pair(ndim, p, q, warp=0.05)
    up = tmod.Transfer(ef, nf.shape[1], et, nt.shape[1])
    down = tmod.Transfer(et, nt.shape[1], ef, nf.shape[1])
    u = np.random.default_rng(2).standard_normal(nf.shape[1])
    err = rel_l2(down.prolong(up.prolong(u)), u)
    print("ndim %d p %d -> %d -> %d: %.2e" % (ndim, p, q, p, err))
    assert err <= TOL_PARITY


# --------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("ndim,p_from,p_to", [(2, 4, 8), (3, 2, 4)])
def test_components_and_repeatability(tmod, ndim, p_from, p_to):
    t, _, nnf, nnt = make(tmod, ndim, p_from, p_to)
    rng = np.random.default_rng(4)
    for call, n_in in ((t.prolong, nnf), (t.restrict, nnt)):
        v = dev(rng.standard_normal((2, n_in)))
        single = torch.stack([call(v[0]), call(v[1])])
        assert torch.equal(call(v), single)                         # component-major
        inter = call(v.T.contiguous().reshape(-1), dofs_per_node=2)
        assert torch.equal(inter.reshape(-1, 2).T, single)          # interleaved
        v3 = dev(rng.standard_normal((3, n_in)))                    # more than the scratch holds
        assert torch.equal(call(v3), torch.stack([call(v3[k]) for k in range(3)]))
        assert torch.equal(call(v), call(v))                        # two runs, the same bits
        host = call(v.cpu().numpy())                                # host in, host out
        assert isinstance(host, np.ndarray) and np.array_equal(host, single.cpu().numpy())


@pytest.mark.parametrize("ndim,p_from,p_to", [(2, 4, 8), (3, 2, 4)])
def test_accumulate_and_unreferenced_nodes(tmod, ndim, p_from, p_to):
    t, twin, nnf, nnt = make(tmod, ndim, p_from, p_to, pad=(2, 3))
    rng = np.random.default_rng(6)
    r, pre = dev(rng.standard_normal(nnt)), dev(rng.standard_normal(nnf))
    plain = t.restrict(r)
    assert torch.equal(plain[-2:], torch.zeros_like(plain[-2:]))    # overwrite: 0 where unreferenced
    out = pre.clone()
    assert t.restrict(r, out=out, accumulate=True) is out
    assert torch.equal(out, pre + plain)
    out = pre.clone()
    t.restrict(r, out=out)                                          # overwrite mode
    assert torch.equal(out, plain)
    # prolong leaves "to" nodes no element references untouched
    u = dev(rng.standard_normal(nnf))
    out = torch.full((nnt,), 7.0, dtype=torch.float64, device="cuda")
    t.prolong(u, out=out)
    assert torch.equal(out[-3:], torch.full_like(out[-3:], 7.0))
    assert torch.equal(out[:-3], t.prolong(u)[:-3])
    ref = twin.prolong(u.cpu().numpy())[:-3].astype(np.float64)
    assert rel_l2(out[:-3].cpu().numpy(), ref) <= TOL_PARITY


@pytest.mark.parametrize("ndim,p_from,p_to", [(2, 4, 8), (3, 2, 4)])
def test_graph_capture(tmod, ndim, p_from, p_to):
    t, _, nnf, nnt = make(tmod, ndim, p_from, p_to)
    rng = np.random.default_rng(8)
    u, r = dev(rng.standard_normal((2, nnf))), dev(rng.standard_normal((2, nnt)))
    eager = t.prolong(u).clone(), t.restrict(r).clone()
    out_p, out_r = torch.zeros_like(eager[0]), torch.zeros_like(eager[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        t.prolong(u, out=out_p, stream=s)
        t.restrict(r, out=out_r, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t.prolong(u, out=out_p)
        t.restrict(r, out=out_r)
    out_p.zero_()
    out_r.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_p, eager[0]) and torch.equal(out_r, eager[1])


# --------------------------------------------------------------------------- renumbering
def test_equal_orders_between_two_numberings_is_the_permutation(tmod):
    from spectralelementmethod_amd import meshgen
    p = 5
    nodes, e2n = meshgen.structured_square(3, 2, p, warp=0.05)
    nodes_r, e2n_r = meshgen.rcm_renumber(nodes, e2n)
    # rcm_renumber also sorts the elements: bring the lexicographic side into
    # that element order (by the elements' first corner)

    def key(nd, m):
        c = np.round(nd[:, m.astype(np.int64)[:, 0, 0]], 9)
        return np.lexsort(c)
    e2n_l = np.empty_like(e2n)
    e2n_l[key(nodes_r, e2n_r)] = e2n[key(nodes, e2n)]
    new_id = np.empty(nodes.shape[1], dtype=np.int64)
    new_id[e2n_l.astype(np.int64).ravel()] = e2n_r.astype(np.int64).ravel()
    assert np.array_equal(nodes_r[:, new_id], nodes)
    assert not np.array_equal(new_id, np.arange(new_id.size))
    t = tmod.Transfer(e2n_l, nodes.shape[1], e2n_r, nodes.shape[1])
    rng = np.random.default_rng(9)
    u, r = rng.standard_normal(nodes.shape[1]), rng.standard_normal(nodes.shape[1])
    assert np.array_equal(t.prolong(u)[new_id], u)
    assert np.array_equal(t.restrict(r), r[new_id])                 # the inverse gather


def test_dof_managers_transfer(tmod):
    from spectralelementmethod_amd import meshgen
    from spectralelementmethod_amd.basis_functions import gll_basis_2d
    from spectralelementmethod_amd.discrete import DOFManager, Mesh
    dms = [DOFManager(Mesh.from_arrays(*meshgen.structured_square(3, 2, p, warp=0.05)), 1,
                      gll_basis_2d(p), device="cuda:0") for p in (3, 6)]       # RCM numberings
    t = dms[0].transfer_to(dms[1])
    maps = [dm.mesh.element_map() for dm in dms]
    twin = tw.Twin(maps[0], dms[0].ndof, maps[1], dms[1].ndof)
    u = np.random.default_rng(10).standard_normal(dms[0].ndof)
    assert rel_l2(t.prolong(u), twin.prolong(u).astype(np.float64)) <= TOL_PARITY


# --------------------------------------------------------------------------- errors
def test_argument_errors_are_raised_on_the_host(tmod):
    from spectralelementmethod_amd import meshgen
    from spectralelementmethod_amd.operators import SEMOperator
    t, _, nnf, nnt = make(tmod, 2, 2, 3)
    with pytest.raises(ValueError):
        t.prolong(np.zeros(nnf + 1))
    with pytest.raises(ValueError):
        t.prolong(np.zeros(nnt))
    with pytest.raises(ValueError):
        t.restrict(np.zeros(nnf))
    with pytest.raises(ValueError):
        t.prolong(np.zeros(2 * nnf + 1), dofs_per_node=2)
    with pytest.raises(ValueError):
        t.restrict(np.zeros(nnt), out=torch.zeros(nnf + 1, dtype=torch.float64, device="cuda"))
    (nf, ef), (nt, et) = mesh_pair(2, 2, 3)
    with pytest.raises(ValueError):
        tmod.Transfer(ef, nf.shape[1], et[:-1], nt.shape[1])        # mismatched n_elem
    with pytest.raises(ValueError):
        tmod.Transfer(ef, nf.shape[1] - 1, et, nt.shape[1])         # an id >= n_node
    with pytest.raises(ValueError):
        tmod.Transfer(ef, nf.shape[1], et, int(et.max()))
    with pytest.raises(NotImplementedError):
        tmod.Transfer(ef, nf.shape[1], np.zeros((len(ef), 18, 18), dtype=np.uint32), 1)
    # operators: another element count, and one element's local axes swapped
    # on one side only
    a = SEMOperator(2, ef, nf, device="cuda:0")
    na, ea = meshgen.structured_square(3, 3, 3)
    with pytest.raises(ValueError):
        a.transfer_to(SEMOperator(3, ea, na, device="cuda:0"))
    nb, eb = meshgen.structured_square(3, 2, 3)
    swapped = eb.copy()
    swapped[4] = eb[4, ::-1, ::-1]            # a half turn: detJ stays positive
    b = SEMOperator(3, swapped, nb, device="cuda:0")
    with pytest.raises(ValueError):
        a.transfer_to(b)
    assert a.transfer_to(b, check=False).n_elem == 6
    assert a.transfer_to(SEMOperator(3, eb, nb, device="cuda:0")).info()["elements"] == 6
