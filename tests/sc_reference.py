"""Plain high-precision statement of the condensation operations
(include/sem_hip.h "Static condensation"): the element Schur complement, the
interior back-solve, a dense direct solve, and the seeded matrices they are
tested on.  NumPy only, np.longdouble where it matters.  The yardstick of
tests/test_sc_reference_host.py (which proves the conditions the bound rests
on, without a device) and of tests/test_gpu_condensation.py.

A local system in hierarchical order has its ne exterior DOFs first:
    S = A_ee - A_ei A_ii^-1 A_ie,  s = b_e - A_ei A_ii^-1 b_i,
    X = A_ii^-1 [A_ie | b_i],      x_i = X[:, ne] - X[:, :ne] x_e.

Errors are max-abs differences over the max-abs of the extended result; the
bar is bound(kappa, n) = 2 eps64 (kappa + n): the first-order forward error
of a backward-stable solve with 2-norm condition number kappa, plus the
accumulation of an n-term dot product."""
import functools

import numpy as np

EPS64 = 2.22e-16
LD = np.longdouble
NO_EXTENDED = "np.longdouble is not an 80-bit extended type on this platform"


def have_extended():
    return bool(np.finfo(LD).eps <= 2e-19)


def bound(kappa, n):
    return 2.0 * EPS64 * (kappa + n)


def err(got, ref):
    """max |got - ref| / max |ref|, evaluated in longdouble."""
    ref = np.asarray(ref, dtype=LD)
    if ref.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, dtype=LD) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------- eliminations
def _gauss_jordan(M, n):
    """Gauss-Jordan with partial pivoting (first row on ties) of the left
    n columns of M [B, n, n + m] in place, all B systems at once; the right m
    columns end as A^-1 R.  Returns the row interchanges of each system."""
    B = M.shape[0]
    ar = np.arange(B)
    swaps = np.zeros(B, dtype=np.int64)
    for k in range(n):
        p = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        swaps += p != k
        rk, rp = M[ar, k, k:].copy(), M[ar, p, k:].copy()
        M[ar, p, k:] = rk
        M[ar, k, k:] = rp / rp[:, :1]
        f = M[:, :, k].copy()
        f[:, k] = 0
        M[:, :, k:] -= f[:, :, None] * M[:, k, None, k:]
    return swaps


def schur_ext(mats, rhs, ne):
    """(S, s, X, interchanges) of the systems mats [E, nl, nl], rhs [E, nl] in
    np.longdouble."""
    A = np.asarray(mats, dtype=LD)
    b = np.asarray(rhs, dtype=LD)
    E, nl = b.shape
    ni = nl - ne
    M = np.concatenate([A[:, ne:, ne:], A[:, ne:, :ne], b[:, ne:, None]], axis=2)
    swaps = _gauss_jordan(M, ni)
    X = np.ascontiguousarray(M[:, :, ni:])
    Y = np.matmul(A[:, :ne, ne:], X)
    return A[:, :ne, :ne] - Y[:, :, :ne], b[:, :ne] - Y[:, :, ne], X, swaps


def backsolve_ext(X, xe):
    """x_i [E, ni] from X [E, ni, ne + 1] and the exterior values xe [E, ne]."""
    X = np.asarray(X, dtype=LD)
    xe = np.asarray(xe, dtype=LD)
    ne = xe.shape[1]
    return X[:, :, ne] - np.matmul(X[:, :, :ne], xe[:, :, None])[:, :, 0]


def solve_ext(A, b):
    """x = A^-1 b in np.longdouble by LU with partial pivoting (first row on
    ties) and back substitution, and the number of row interchanges.  Exactly
    zero multipliers and pivot-row entries are skipped (they change nothing),
    which keeps banded and sparse systems cheap."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    M = np.concatenate([A, np.asarray(b, dtype=LD).reshape(n, 1)], axis=1)
    swaps = 0
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            swaps += 1
        rows = k + 1 + np.nonzero(M[k + 1:, k])[0]
        if rows.size:
            cols = k + 1 + np.nonzero(M[k, k + 1:])[0]
            f = M[rows, k] / M[k, k]
            M[np.ix_(rows, cols)] -= f[:, None] * M[k, cols][None, :]
            M[rows, k] = 0
    x = np.zeros(n, dtype=LD)
    for k in range(n - 1, -1, -1):
        cols = k + 1 + np.nonzero(M[k, k + 1:n])[0]
        x[k] = (M[k, n] - M[k, cols] @ x[cols]) / M[k, k]
    return x, swaps


# ------------------------------------------- float64 LAPACK, for comparison
def lapack_schur(A, b, ne):
    """S, s of one system by the reference's float64 formula (scipy
    linalg.solve on the transposed interior block), and X by linalg.solve."""
    from scipy import linalg
    ext, itr = slice(None, ne), slice(ne, None)
    if A.shape[0] == ne:
        return A.copy(), b.copy(), np.zeros((0, ne + 1))
    tmp = linalg.solve(A[itr, itr].T, A[ext, itr].T).T
    X = linalg.solve(A[itr, itr], np.concatenate([A[itr, ext], b[itr, None]], axis=1))
    return A[ext, ext] - tmp @ A[itr, ext], b[ext] - tmp @ b[itr], X


def lapack_banded(A, kl, ku, b):
    """x by scipy linalg.solve_banded (gbsv) on the band of the dense A."""
    from scipy import linalg
    n = A.shape[0]
    l, u = min(kl, n - 1), min(ku, n - 1)
    ab = np.zeros((l + u + 1, n))
    for k in range(-l, u + 1):
        j = np.arange(max(0, k), min(n, n + k))
        ab[u - k, j] = A[j - k, j]
    return linalg.solve_banded((l, u), ab, b)


# ----------------------------------------------------------------- matrices
def general(nl, n_elem=3, seed=0, ne=0):
    """i.i.d. normal entries, non-symmetric: interchanges at nearly every step."""
    rng = np.random.default_rng([seed, nl, 1])
    return rng.standard_normal((n_elem, nl, nl)), rng.standard_normal((n_elem, nl))


def spd_skew(nl, n_elem=3, seed=0, ne=0):
    """B B^T / nl + I + (C - C^T) / 2, the shape of the facade tests' matrices."""
    rng = np.random.default_rng([seed, nl, 2])
    B = rng.standard_normal((n_elem, nl, nl))
    C = rng.standard_normal((n_elem, nl, nl))
    A = B @ B.transpose(0, 2, 1) / nl + np.eye(nl) + 0.5 * (C - C.transpose(0, 2, 1))
    return A, rng.standard_normal((n_elem, nl))


def displaced(nl, n_elem=3, seed=0, ne=0):
    """Small noise N(0, 1) / (4 sqrt(nl)) plus, in the interior block, +-2 at
    row (k + 5 ni / 8) mod ni of column k: a row permutation of a dominant
    diagonal, so kappa_2 is small, every step interchanges, and the pivot of
    column k lies 5 ni / 8 rows below the diagonal.  A pivot search that stops
    short of that row is left with the noise and its growth."""
    rng = np.random.default_rng([seed, nl, 6])
    A = rng.standard_normal((n_elem, nl, nl)) * (0.25 / np.sqrt(nl))
    ni = nl - ne
    k = np.arange(ni)
    A[:, ne + (k + 5 * ni // 8) % ni, ne + k] += np.where(rng.random((n_elem, ni)) < 0.5, 2.0, -2.0)
    return A, rng.standard_normal((n_elem, nl))


GENERATORS = {"general": general, "spd_skew": spd_skew, "displaced": displaced}
# pivots displaced by 320 rows, past one round of the kernel's 256 threads
DISPLACED = ("displaced", 64, 512)

# (ne, ni) of the Schur tests; every shape runs with both generators
SCHUR_SHAPES = [(8, 1), (16, 9), (12, 63), (12, 64), (12, 65), (64, 255), (64, 256), (64, 257),
                (128, 450), (64, 512)]
# a case that breaks a condition of tests/test_sc_reference_host.py gets
# another seed here, not a skip
SCHUR_SEEDS = {}
# more elements than workgroups: (kind, n_elem, ne, ni)
MANY = ("general", 4096 * 2 + 37, 12, 4)


def band(n, kl, ku, seed=0, small_every=None):
    """Dense [n, n] matrix of lower / upper bandwidth kl / ku and a right-hand
    side.  Square bands (kl == ku): off-diagonals N(0, 1) / (kl + ku + 1), the
    diagonal +-(1..2) with every 7th entry from row 3 scaled by 1e-3, so that
    partial pivoting interchanges.  Other bands: off-diagonals
    N(0, 1) / 2 / (kl + ku + 1), the diagonal unscaled (dominant), unless
    small_every = m scales every m-th entry from row 3 as in the square bands."""
    rng = np.random.default_rng([seed, n, kl, ku])
    w = kl + ku + 1
    A = np.zeros((n, n))
    for k in range(-min(kl, n - 1), min(ku, n - 1) + 1):
        if k:
            A += np.diag(rng.standard_normal(n - abs(k)), k) * ((1.0 if kl == ku else 0.5) / w)
    d = np.where(rng.random(n) < 0.5, 1.0, -1.0) * (1.0 + rng.random(n))
    if small_every is None:
        small_every = 7 if kl == ku else 0
    if small_every:
        d[3::small_every] *= 1e-3
    A[np.arange(n), np.arange(n)] = d
    return A, rng.standard_normal(n)


# (n, kl, ku) of the band tests; the declared band may be wider than the matrix
BAND_SHAPES = [(1, 0, 0), (1, 3, 3), (2, 1, 1), (5, 8, 8), (9, 8, 8), (300, 0, 5), (300, 5, 0),
               (300, 0, 0), (257, 37, 3), (257, 3, 37), (1025, 2, 2), (400, 64, 64),
               (130, 129, 129)]
BAND_SEEDS = {}
# the uneven band that interchanges, with every 7th diagonal entry small: a
# chain of 36 small pivots below a 37-wide lower band, kappa_2 = 3e17, so it
# is judged by its backward error
BAND_PIVOTING_UNEVEN = (257, 37, 3)
# uneven bands that interchange and stay well conditioned (n, kl, ku,
# small_every): judged like every other band, against solve_ext
BAND_UNEVEN_SMALL = [(257, 37, 3, 48), (257, 3, 37, 48)]


def band_csr(A, kl, ku):
    """CSR (int64 row pointers, int32 columns, values) holding every entry of
    A inside the band, zeros included, and nothing outside it."""
    n = A.shape[0]
    i, j = np.indices((n, n))
    keep = (i - j <= kl) & (j - i <= ku)
    assert not np.any(A[~keep]), "entry outside the declared band"
    return dense_csr(A, keep)


def dense_csr(A, keep=None):
    keep = (A != 0) if keep is None else keep
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    r, c = np.nonzero(keep)
    return rp, c.astype(np.int32), np.ascontiguousarray(A[r, c], dtype=np.float64)


def split_csr(rp, ci, va, shuffle_seed=None):
    """Every stored entry a as the two entries a/2 + a/2 (exact in binary);
    with a seed, the entries of each row in shuffled order."""
    n = rp.size - 1
    rng = None if shuffle_seed is None else np.random.default_rng(shuffle_seed)
    cols, vals = [], []
    for r in range(n):
        c = np.repeat(ci[rp[r]:rp[r + 1]], 2)
        v = np.repeat(va[rp[r]:rp[r + 1]] * 0.5, 2)
        if rng is not None:
            o = rng.permutation(c.size)
            c, v = c[o], v[o]
        cols.append(c)
        vals.append(v)
    return (2 * rp).astype(np.int64), np.concatenate(cols).astype(np.int32), np.concatenate(vals)


PCG_SIZES = [1, 2, 31, 33, 1001]
PCG_MASKS = ["none", "random", "all"]


def laplace_spd(n, seed=0):
    """Leading n x n block of D (L + 0.1 I) D: L the five-point Laplacian of
    the smallest m x m grid with m^2 >= n, D a random diagonal in [0.5, 2].
    Symmetric bit for bit."""
    m = int(np.ceil(np.sqrt(n)))
    N = m * m
    L = np.zeros((N, N))
    idx = np.arange(N).reshape(m, m)
    L[np.arange(N), np.arange(N)] = 4.1
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        L[a.ravel(), b.ravel()] = -1.0
        L[b.ravel(), a.ravel()] = -1.0
    d = np.random.default_rng([seed, n, 3]).uniform(0.5, 2.0, N)
    return (L * np.multiply.outer(d, d))[:n, :n].copy()


def pcg_mask(n, which, seed=0):
    if which == "none":
        return np.zeros(n, dtype=bool)
    if which == "all":
        return np.ones(n, dtype=bool)
    return np.random.default_rng([seed, n, 4]).random(n) < 0.2


# ------------------------------------------------ cases, computed once a run
@functools.lru_cache(maxsize=None)
def schur_case(kind, ne, ni, n_elem=3):
    """Inputs, extended results and condition numbers of one Schur case
    (read-only: shared by every test of a run)."""
    nl = ne + ni
    mats, rhs = GENERATORS[kind](nl, n_elem, SCHUR_SEEDS.get((kind, ne, ni), 0), ne)
    S, s, X, swaps = schur_ext(mats, rhs, ne)
    kappa = np.array([np.linalg.cond(m[ne:, ne:]) if ni else 1.0 for m in mats])
    case = dict(kind=kind, ne=ne, ni=ni, nl=nl, mats=mats, rhs=rhs, S=S, s=s, X=X, swaps=swaps,
                kappa=kappa, bound=bound(kappa, nl))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def band_case(n, kl, ku, small_every=None):
    A, b = band(n, kl, ku, BAND_SEEDS.get((n, kl, ku), 0), small_every)
    x, swaps = solve_ext(A, b)
    kappa = float(np.linalg.cond(A))
    case = dict(n=n, kl=kl, ku=ku, A=A, b=b, x=x, swaps=swaps, kappa=kappa, bound=bound(kappa, n))
    for v in (A, b, x):
        v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def pcg_case(n, which):
    """A, b, the mask, the start vector (0 on free DOFs, the fixed values on
    masked ones), r0 = b_f - (A x0)_f, the extended solution on the free
    block and kappa_2(A_ff)."""
    A = laplace_spd(n)
    rng = np.random.default_rng([n, PCG_MASKS.index(which), 5])
    b = rng.standard_normal(n)
    mask = pcg_mask(n, which)
    x0 = np.where(mask, rng.standard_normal(n), 0.0)
    free = ~mask
    r0 = (b.astype(LD) - A.astype(LD) @ x0.astype(LD))[free]
    case = dict(n=n, which=which, A=A, b=b, mask=mask, x0=x0, free=free, r0=r0)
    if free.any():
        Aff = A[np.ix_(free, free)]
        case["xf"], _ = solve_ext(Aff, r0)
        case["kappa"] = float(np.linalg.cond(Aff))
    else:
        case["xf"], case["kappa"] = np.zeros(0, dtype=LD), 1.0
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def pcg_residual(case, x):
    """||b_f - (A x)_f||_2 / ||r0||_2 in longdouble."""
    f = case["free"]
    r = (case["b"].astype(LD) - case["A"].astype(LD) @ np.asarray(x, dtype=LD))[f]
    return float(np.sqrt(r @ r) / np.sqrt(case["r0"] @ case["r0"]))


def backward_error(A, x, b):
    """||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), residual in longdouble."""
    A = np.asarray(A, dtype=LD)
    x = np.asarray(x, dtype=LD)
    b = np.asarray(b, dtype=LD)
    r = b - A @ x
    return float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))
