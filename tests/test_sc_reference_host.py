"""Host checks of tests/sc_reference.py, the yardstick of
tests/test_gpu_condensation.py: the extended-precision results are right, and
the seeded inputs meet the conditions its bound rests on, at every shape of
the GPU tests.  No device is needed.

* the extended elimination solves its system (residual in longdouble);
* S and s agree with the float64 formula of
  test_compute_local_sc_system_matches_dense to bound(kappa, nl);
* kappa_2 <= 1e6 everywhere (bound <= 5e-10); `general` blocks and the square
  bands with n >= 9 interchange rows at least n / 10 times;
* the bound is fair: float64 LAPACK alone (linalg.solve, solve_banded) stays
  within a quarter of it, measured against the extended result.

A case that breaks a condition gets another seed in sc_reference, not a skip."""
import numpy as np
import pytest

import sc_reference as ref

LD = np.longdouble
pytestmark = pytest.mark.skipif(not ref.have_extended(), reason=ref.NO_EXTENDED)

SCHUR = [(k, ne, ni) for k in ("general", "spd_skew") for ne, ni in ref.SCHUR_SHAPES]
SCHUR.append(ref.DISPLACED)


def test_extended_type_and_bound():
    assert np.finfo(LD).eps <= 2e-19
    assert ref.bound(1e6, 1000) <= 5e-10
    assert ref.bound(0.0, 1) == 2 * 2.22e-16


@pytest.mark.parametrize("kind,ne,ni", SCHUR)
def test_schur_case(kind, ne, ni):
    c = ref.schur_case(kind, ne, ni)
    A, b = c["mats"].astype(LD), c["rhs"].astype(LD)
    assert c["kappa"].max() <= 1e6
    assert c["bound"].max() <= 5e-10
    if kind == "general" and ni >= 9:  # one row cannot interchange
        assert c["swaps"].min() >= ni / 10.0
    if kind == "displaced":  # the pivot of column k starts 5 ni / 8 rows below it
        assert c["swaps"].min() >= ni / 2
        assert np.all(np.abs(c["mats"][:, ne:, ne:]).argmax(axis=1)
                      == (np.arange(ni) + 5 * ni // 8) % ni)
    for e in range(A.shape[0]):
        # the reference is right: A_ii X = [A_ie | b_i]
        R = np.concatenate([A[e, ne:, :ne], b[e, ne:, None]], axis=1)
        res = np.abs(A[e, ne:, ne:] @ c["X"][e] - R).max() / np.abs(R).max()
        assert res <= 1e-17 * c["kappa"][e], (res, c["kappa"][e])
        # float64 LAPACK meets a quarter of the bound
        Sl, sl, Xl = ref.lapack_schur(c["mats"][e], c["rhs"][e], ne)
        errs = (ref.err(Sl, c["S"][e]), ref.err(sl, c["s"][e]), ref.err(Xl, c["X"][e]))
        print("%s ne=%d ni=%d e=%d: kappa %.2e swaps %d bound %.2e lapack S %.2e s %.2e X %.2e"
              % ((kind, ne, ni, e, c["kappa"][e], c["swaps"][e], c["bound"][e]) + errs))
        assert max(errs) <= c["bound"][e] / 4


def test_many_elements_case():
    kind, E, ne, ni = ref.MANY
    c = ref.schur_case(kind, ne, ni, E)
    assert c["mats"].shape == (E, ne + ni, ne + ni)
    assert c["kappa"].max() <= 1e6
    # every element is different
    assert np.unique(c["mats"][:, 0, 0]).size == E
    worst = 0.0
    for e in range(0, E, 97):
        Sl, sl, Xl = ref.lapack_schur(c["mats"][e], c["rhs"][e], ne)
        errs = (ref.err(Sl, c["S"][e]), ref.err(sl, c["s"][e]), ref.err(Xl, c["X"][e]))
        worst = max(worst, max(errs) / c["bound"][e])
    assert worst <= 0.25, worst


def test_schur_ext_matches_solve_ext_and_backsolve():
    c = ref.schur_case("general", 12, 65)
    ne = 12
    A, b = c["mats"][1], c["rhs"][1]
    x, swaps = ref.solve_ext(A[ne:, ne:], b[ne:])
    assert swaps == c["swaps"][1]
    assert ref.err(x, c["X"][1][:, ne]) <= 1e-17 * c["kappa"][1]
    # the condensed system and the back-solve reproduce the full solve
    xe, _ = ref.solve_ext(c["S"][1], c["s"][1])
    xi = ref.backsolve_ext(c["X"][1:2], xe[None, :])[0]
    full, _ = ref.solve_ext(A, b)
    assert ref.err(np.concatenate([xe, xi]), full) <= 1e-15 * np.linalg.cond(A)


BANDS = [s + (None,) for s in ref.BAND_SHAPES] + ref.BAND_UNEVEN_SMALL


@pytest.mark.parametrize("n,kl,ku,small_every", BANDS)
def test_band_case(n, kl, ku, small_every):
    c = ref.band_case(n, kl, ku, small_every)
    A, b = c["A"], c["b"]
    assert c["kappa"] <= 1e6 and c["bound"] <= 5e-10
    if kl == ku and kl > 0 and n >= 9:  # a diagonal matrix cannot interchange
        assert c["swaps"] >= n / 10.0
    if small_every:  # one interchange or more at each small diagonal entry
        assert c["swaps"] >= len(range(3, n, small_every))
    res = np.abs(A.astype(LD) @ c["x"] - b).max() / np.abs(b).max()
    assert res <= 1e-17 * c["kappa"]
    e = ref.err(ref.lapack_banded(A, kl, ku, b), c["x"])
    print("band n=%d kl=%d ku=%d: kappa %.2e swaps %d bound %.2e lapack %.2e"
          % (n, kl, ku, c["kappa"], c["swaps"], c["bound"], e))
    assert e <= c["bound"] / 4
    # the CSR the device gets holds the band and nothing else
    rp, ci, va = ref.band_csr(A, kl, ku)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.all(rows - ci <= kl) and np.all(ci - rows <= ku)
    D = np.zeros((n, n))
    D[rows, ci] = va
    assert np.array_equal(D, A)


def test_uneven_band_that_interchanges():
    n, kl, ku = ref.BAND_PIVOTING_UNEVEN
    c = ref.band_case(n, kl, ku, 7)
    assert c["swaps"] >= n / 10.0
    assert np.isfinite(c["kappa"])
    assert ref.backward_error(c["A"], c["x"], c["b"]) <= 1e-18


def test_split_csr_is_the_same_matrix():
    A, _ = ref.band(33, 3, 3)
    rp, ci, va = ref.band_csr(A, 3, 3)
    rp2, ci2, va2 = ref.split_csr(rp, ci, va, shuffle_seed=1)
    assert rp2[-1] == 2 * rp[-1]
    D = np.zeros_like(A)
    np.add.at(D, (np.repeat(np.arange(33), np.diff(rp2)), ci2), va2)
    assert np.array_equal(D, A)


@pytest.mark.parametrize("n", ref.PCG_SIZES)
@pytest.mark.parametrize("which", ref.PCG_MASKS)
def test_pcg_case(n, which):
    c = ref.pcg_case(n, which)
    A = c["A"]
    assert np.array_equal(A, A.T)
    assert np.linalg.eigvalsh(A).min() > 0
    assert np.linalg.cond(A) <= 1e3 and c["kappa"] <= 1e3
    assert np.count_nonzero(A) <= 5 * n
    assert which != "all" or not c["free"].any()
    f = c["free"]
    if not f.any():
        return
    Aff = A[np.ix_(f, f)].astype(LD)
    res = np.abs(Aff @ c["xf"] - c["r0"]).max() / np.abs(c["r0"]).max()
    assert res <= 1e-17 * c["kappa"]
    # the extended solution has residual 0 by the measure of the GPU test
    x = c["x0"].astype(LD)
    x[f] = c["xf"]
    assert ref.pcg_residual(c, x) <= 1e-17 * c["kappa"]
