"""GPU: the direct eigensolver (Householder tridiagonalisation with workgroup
hand-off, bisection, twisted factorisation or inverse iteration, three
back-transformations) at the level of eigenpairs, through scc_diag_eigen_topk
with SCC_EIG_SI=0 and SCC_EIG_FSI=0 (path 0), against numpy.linalg.eigh.

Every case asserts, with w the LAPACK eigenvalues (descending), v its vectors
and theta_q = z_q^T H z_q formed on the host:
  * W descending, columns >= k of Z zero;
  * |W_q - w_q| <= 1e-12 w_1 (the bar of test_small_syev_matches_lapack; it also
    catches correct eigenpairs that are not the top ones);
  * |W_q - theta_q| <= 1e-12 w_1;
  * max_q |H z_q - W_q z_q|_2 <= 1e-11 w_1;
  * max |Z^T Z - I| <= 1e-11 (the project's SI_TOL / FSI_TOL and the small
    solver's bar: nothing in the pipeline may be looser than what replaces it);
  * Davis-Kahan from the residual bar: with P the projector onto LAPACK's
    vectors of the eigenvalue's cluster (eigenvalues chained by gaps
    <= 1e-3 w_1; a single vector when it is isolated) and gap the distance from
    w_q to the rest of the spectrum (the (k+1)-th included),
    |(I - P) z_q| <= 4 * 1e-11 * w_1 / gap.

Thresholds of eig_plan (scc_eigen.hip), one n on each side:
  * tri_nj: register row slots 6 / 8 / 14 at n <= 384 / 512 / 896 -> 384, 385,
    512, 513, 896; n = 897: no register rows, every own row in LDS;
  * rows in LDS while tri_lds_bytes(n, R) <= 160 KB - 64 B (the kernel's static
    shared variables); with R = 10 rows per workgroup ((n + 9) / 10 workgroups,
    at most one per CU) that is 120 n + 2560 <= 163776, n <= 1343 -> 1343 (LDS),
    1344 and 2100 (global rows).  n = 1344 asked for exactly 160 KB of dynamic
    LDS beside 12 static bytes before the plan kept that margin: an invalid
    dispatch;
  * the LU of T - lambda I in LDS while 80 n <= 160 KB - 2 KB, n <= 2022 -> 1344
    and 2100 (global LU slots, inverse iteration for every pair).
SCC_EIG_NWG=8 at n = 323 / 400 puts 29 / 38 rows per workgroup in LDS beside
the 12 in registers.

Each case prints one "EIGPAIR" line with the measured residual and
orthogonality and LAPACK's on the same matrix (profiles/pca_stage_tests.md).
"""
import ctypes

import numpy as np
import pytest
import torch

from scconsensus_amd import _native as nat

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VAL_TOL = 1e-12
RES_TOL = 1e-11
ORTH_TOL = 1e-11
CLUSTER = 1e-3


@pytest.fixture(autouse=True)
def _direct_only(monkeypatch):
    monkeypatch.setenv("SCC_EIG_SI", "0")
    monkeypatch.setenv("SCC_EIG_FSI", "0")


@pytest.fixture(scope="module")
def lib():
    L = nat.load()
    L.scc_diag_eigen_topk.restype = ctypes.c_int
    return L


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ matrices
def _from_spectrum(lam, seed):
    rng = np.random.default_rng(seed)
    V, _ = np.linalg.qr(rng.standard_normal((len(lam), len(lam))))
    H = (V * lam) @ V.T
    return 0.5 * (H + H.T)


def _wishart(n, seed):
    A = np.random.default_rng(seed).standard_normal((n, 2 * n))
    return A @ A.T


def _repeated(n, seed):  # multiplicities 3, 4, 2, 6 inside the top 15
    lam = np.array([81.0] * 3 + [49.0] * 4 + [25.0] * 2 + [16.0] * 6 + [1.0] * max(n - 15, 0))[:n]
    return _from_spectrum(lam, seed)


def _near_pair(n, seed):  # a near-degenerate pair, relative gap 1e-9
    lam = np.sort(np.random.default_rng(seed).uniform(1.0, 10.0, n))[::-1].copy()
    lam[1] = lam[0] * (1.0 - 1e-9)
    return _from_spectrum(lam, seed)


def _graded(n, seed):
    return _from_spectrum(np.logspace(0, -12, n), seed)


def _rank5(n, seed):
    lam = np.zeros(n)
    lam[:min(5, n)] = np.array([5.0, 4.0, 3.0, 2.0, 1.0])[:min(5, n)]
    return _from_spectrum(lam, seed)


def _diagonal(n, seed):  # every reflector has tau = 0
    return np.diag(np.random.default_rng(seed).permutation(np.linspace(1.0, 10.0, n)))


def _mixed(n, seed):
    """Isolated values, an exact triple, a near pair and a bulk: the twisted
    factorisation, inverse iteration and the cluster Gram-Schmidt all run."""
    top = np.array([100.0, 81.0, 81.0, 81.0, 64.0, 49.0, 49.0 * (1 - 1e-9), 36.0, 25.0, 16.0, 9.0, 8.0, 7.0, 6.0, 5.0])
    bulk = np.sort(np.random.default_rng(seed).uniform(0.1, 1.0, max(n - 15, 0)))[::-1]
    return _from_spectrum(np.concatenate([top, bulk])[:n], seed)


def _b_like(n, seed):  # the spectrum shape of tests/test_gpu_fsi.py
    rng = np.random.default_rng(seed)
    top = np.array([15.14, 10.09, 8.97, 7.95, 6.82, 6.22, 3.59, 2.21, 1.655, 1.469, 1.055, 1.021, 1.009, 1.0045, 1.0])
    bulk = np.sort(rng.uniform(0.184, 0.996, n - 15))[::-1]
    bulk[0] = 0.996
    bulk[49] = 0.877
    return _from_spectrum(np.concatenate([top, np.sort(bulk)[::-1]]) * 4.1e4, seed)


SPECTRA = {"wishart": _wishart, "repeated": _repeated, "near_pair": _near_pair, "graded": _graded, "rank5": _rank5,
           "diagonal": _diagonal, "mixed": _mixed, "b_like": _b_like}


# ------------------------------------------------------------------ solve and check
def _solve(lib, H, k, padded=True):
    n = H.shape[0]
    lda = (n + 63) & ~63 if padded else n
    A = np.zeros((lda if padded else n, lda))
    A[:n, :n] = H
    Ad = torch.tensor(A, dtype=torch.float64, device=DEV)
    Z = torch.full((n * 16,), float("nan"), dtype=torch.float64, device=DEV)
    W = torch.full((16,), float("nan"), dtype=torch.float64, device=DEV)
    path = ctypes.c_int(-1)
    rc = lib.scc_diag_eigen_topk(_p(Ad), n, lda, k, _p(Z), _p(W), ctypes.byref(path))
    assert rc == 0
    return Z.cpu().numpy().reshape(n, 16), W.cpu().numpy()[:k], path.value


def _measure(H, Z, W):
    k = Z.shape[1]
    res = float(np.max(np.linalg.norm(H @ Z - Z * W, axis=0)))
    orth = float(np.max(np.abs(Z.T @ Z - np.eye(k))))
    return res, orth


def _check(tag, H, w, V, Z16, W, k):
    """The assertions of the module docstring; w, V: numpy.linalg.eigh, descending."""
    n = H.shape[0]
    w1 = abs(w[0])
    Z = Z16[:, :k]
    assert np.isfinite(Z16).all() and np.isfinite(W).all(), tag
    assert np.all(Z16[:, k:] == 0.0), tag
    res, orth = _measure(H, Z, W)
    lres, lorth = _measure(H, V[:, :k], w[:k])
    print(f"EIGPAIR {tag} n={n} k={k} res/w1={res / w1:.2e} orth={orth:.2e} "
          f"lapack_res/w1={lres / w1:.2e} lapack_orth={lorth:.2e} val={np.max(np.abs(W - w[:k])) / w1:.2e}")
    assert np.all(np.diff(W) <= 0.0), tag
    assert np.max(np.abs(W - w[:k])) <= VAL_TOL * w1, tag
    theta = np.einsum("iq,ij,jq->q", Z, H, Z)
    assert np.max(np.abs(W - theta)) <= VAL_TOL * w1, tag
    assert res <= RES_TOL * w1, tag
    assert orth <= ORTH_TOL, tag
    # clusters of the whole LAPACK spectrum: chained by gaps <= 1e-3 w_1
    start = np.concatenate([[0], np.nonzero(-np.diff(w) > CLUSTER * w1)[0] + 1, [n]])
    for a, b in zip(start[:-1], start[1:]):
        if a >= k or (a == 0 and b == n):
            continue
        P = V[:, a:b]
        for q in range(a, min(b, k)):
            outside = np.concatenate([w[:a], w[b:]])
            gap = np.min(np.abs(outside - w[q]))
            off = np.linalg.norm(Z[:, q] - P @ (P.T @ Z[:, q]))
            assert off <= 4.0 * RES_TOL * w1 / gap, (tag, q, off, gap)


def _eigh(H):
    w, V = np.linalg.eigh(H)
    return w[::-1].copy(), V[:, ::-1].copy()


def _ks(n):
    return sorted({k for k in (1, 2, 15, 16) if k <= n} | ({n} if n <= 16 else set()))


# ------------------------------------------------------------------ sizes x spectra
SIZES = [2, 3, 16, 17, 63, 64, 65, 128, 255, 256, 257, 400]


@pytest.mark.parametrize("spectrum", ["wishart", "repeated", "near_pair", "graded", "rank5", "diagonal"])
@pytest.mark.parametrize("n", SIZES)
def test_direct_eigenpairs(lib, n, spectrum):
    """rank5 at k >= 15 asks for ten pairs inside the null space: eigenvalues
    that agree to rounding, where the cluster's inverse iterations must still
    return independent vectors (n = 255 gave a residual of 1.03e-11 w_1 and an
    orthogonality of 9.9e-7 before the solves moved their shift 64 eps ||T||
    off the bisected one and the cluster Gram-Schmidt made two passes)."""
    H = SPECTRA[spectrum](n, seed=n)
    w, V = _eigh(H)
    for k in _ks(n):
        Z, W, path = _solve(lib, H, k)
        assert path == 0
        _check(spectrum, H, w, V, Z, W, k)


def test_unpadded_leading_dimension(lib):
    """lda = n (the diagnostic's other layout; production pads to 64)."""
    n, k = 65, 15
    H = _wishart(n, seed=3)
    w, V = _eigh(H)
    Z, W, path = _solve(lib, H, k, padded=False)
    assert path == 0
    _check("wishart_lda_n", H, w, V, Z, W, k)


@pytest.mark.parametrize("n", [384, 385, 512, 513, 896, 897, 1343, 1344])
def test_direct_eigenpairs_at_plan_thresholds(lib, n):
    """Register row slots 6 / 8 / 14 / none, the largest n with LDS rows and the
    first with global rows."""
    H = _wishart(n, seed=n)
    w, V = _eigh(H)
    Z, W, path = _solve(lib, H, 15)
    assert path == 0
    _check("wishart_plan", H, w, V, Z, W, 15)


def test_direct_eigenpairs_global_rows(lib):
    """n = 2100: own rows in global memory and the LU slots too (one case, one
    2100 x 2100 eigh on the host)."""
    n = 2100
    H = _wishart(n, seed=n)
    w, V = _eigh(H)
    Z, W, path = _solve(lib, H, 15)
    assert path == 0
    _check("wishart_global", H, w, V, Z, W, 15)


def test_identity(lib):
    n = 40
    H = np.eye(n)
    w, V = _eigh(H)
    for k in (1, 15, 16):
        Z, W, path = _solve(lib, H, k)
        assert path == 0
        _check("identity", H, w, V, Z, W, k)


def test_zero_matrix(lib):
    """W = 0 (the bisection's bracket is +-1e-300 around a zero Gershgorin
    interval) and Z finite and orthonormal."""
    n = 40
    H = np.zeros((n, n))
    for k in (1, 15, 16):
        Z, W, path = _solve(lib, H, k)
        assert path == 0
        assert np.all(np.abs(W) <= 2e-300)
        assert np.isfinite(Z).all()
        assert np.all(Z[:, k:] == 0.0)
        orth = float(np.max(np.abs(Z[:, :k].T @ Z[:, :k] - np.eye(k))))
        print(f"EIGPAIR zero n={n} k={k} orth={orth:.2e}")
        assert orth <= ORTH_TOL


# ------------------------------------------------------------------ routes
@pytest.mark.parametrize("twist", ["1", "0"])
@pytest.mark.parametrize("bt", ["0", "1", "2"])
@pytest.mark.parametrize("n", [17, 150, 323, 400])
def test_direct_routes(lib, monkeypatch, n, bt, twist):
    """Back-transformation per eigenpair / one workgroup / explicit Q, twisted
    factorisation on / off, 8 or 32 tridiagonalisation workgroups, on one XCD
    or anywhere: the same bars on every route."""
    monkeypatch.setenv("SCC_EIG_BT", bt)
    monkeypatch.setenv("SCC_EIG_TWIST", twist)
    H = _mixed(n, seed=n)
    w, V = _eigh(H)
    for nwg in ("8", "32"):
        for xcd in ("0", "1"):
            monkeypatch.setenv("SCC_EIG_NWG", nwg)
            monkeypatch.setenv("SCC_EIG_XCD", xcd)
            Z, W, path = _solve(lib, H, 15)
            assert path == 0
            _check(f"mixed_bt{bt}_tw{twist}_nwg{nwg}_xcd{xcd}", H, w, V, Z, W, 15)


def test_rerun_after_forced_timeout(lib, monkeypatch):
    """SCC_EIG_FORCE_TIMEOUT=1 (a flag, nothing is provoked): the one-workgroup
    rerun without cooperative waits answers (path 4) and meets the same bars."""
    monkeypatch.setenv("SCC_EIG_FORCE_TIMEOUT", "1")
    n = 150
    H = _mixed(n, seed=4)
    w, V = _eigh(H)
    Z, W, path = _solve(lib, H, 15)
    assert path == 4
    _check("mixed_rerun", H, w, V, Z, W, 15)


@pytest.mark.parametrize("n", [130, 323, 500])
def test_default_route_meets_the_same_bars(lib, monkeypatch, n):
    """Switches unset: whichever solver answers (the filtered iteration or the
    direct fallback) meets the bars of the direct solver."""
    monkeypatch.delenv("SCC_EIG_SI")
    monkeypatch.delenv("SCC_EIG_FSI")
    H = _b_like(n, seed=n)
    w, V = _eigh(H)
    Z, W, path = _solve(lib, H, 15)
    assert path in (0, 1, 2, 3)
    _check(f"b_like_default_path{path}", H, w, V, Z, W, 15)
