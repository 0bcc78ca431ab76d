"""The cases, the reference and the restatement of tests/pg_linear_cases.py hold what tests/test_gpu_pg_linear.py relies on (CPU only):
every case compared by value is solvable by the float64 restatement and its long-double reference is at least 64 times better than the
forward bar; solve_ref agrees with mpmath at 40 digits; chol64 agrees with numpy.linalg.solve; the indefinite builder fails at the
pivot it names and not before."""
import numpy as np
import pytest

import pg_linear_cases as pc


@pytest.mark.parametrize("fam,n", pc.dense_cases())
def test_every_dense_case_meets_the_condition(fam, n):
    A = pc.family(fam, n)
    assert np.array_equal(A, A.T)
    names, B = pc.rhs_set(A)
    assert pc.chol64(A, B) is not None, (fam, n)
    bar = pc.bars(A, B)
    ok, ratio = pc.reference_is_good(A, B, bar)
    print("%s n=%d: restatement forward %.2e residual %.2e, reference error / forward bar %.2e" %
          (fam, n, bar["forward64"].max(), bar["residual64"].max(), ratio))
    assert ok, (fam, n, ratio)
    assert (bar["forward"] >= pc.BAR_MIN).all() and (bar["residual"] >= pc.BAR_MIN).all()
    assert (bar["forward"] < 1e-2).all(), "a bar that wide checks nothing: lower k"


@pytest.mark.parametrize("n", pc.ORDERS_ALL_FAMILIES)
def test_the_bars_catch_a_solve_wrong_at_1e_7(n):
    """What Levenberg-Marquardt forgives: one component of x off by 1e-7 of max|x| (every unit-vector column included) is over the
    forward bar in four of the six families at every order; the spectra of condition 1e10 and 1e12 cannot see it in the forward error
    (their own restatement is that far off) and are there for the residual, where 1e-7 of the largest component is over the bar too."""
    for fam in pc.FAMILIES:
        A = pc.family(fam, n)
        names, B = pc.rhs_set(A)
        bar = pc.bars(A, B)
        wrong = np.array(bar["x64"])
        k = np.abs(wrong).argmax(axis=0)
        wrong[k, np.arange(B.shape[1])] *= 1.0 + 1e-7
        if fam not in ("spectrum10", "spectrum12"):
            over = pc.forward_error(wrong, bar["x_ref"]) > bar["forward"]
            if fam == "graded":   # x = ones out of entries 1e-8 .. 1e8 apart: the restatement itself is 1e-8 off there
                over = over[[j for j, nm in enumerate(names) if nm != "A@ones"]]
            assert over.all(), fam
        if fam != "graded":   # (graded: the largest component of x sits on the smallest rows of A, far under ||A||_inf)
            assert (pc.scaled_residual(A, wrong, B) > bar["residual"]).any(), fam


def test_solve_ref_matches_mpmath():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    for A in (pc.spectrum(12, 10, 1), pc.graded(9, 1), pc.block_chain(18, 1)):
        n = A.shape[0]
        b = np.random.default_rng(n).normal(size=n)
        x = pc.solve_ref(A, b)
        xm = mpmath.lu_solve(mpmath.matrix(A.tolist()), mpmath.matrix(b.tolist()))
        xm = np.array([pc.LD(mpmath.nstr(v, 30)) for v in xm], dtype=pc.LD)
        err = float(np.abs(x - xm).max() / np.abs(xm).max())
        # long double carries 2^-64; the solution of a system of condition c is known to about c 2^-64 after one refinement step
        c = np.linalg.cond(A / np.sqrt(np.outer(np.diag(A), np.diag(A))))
        assert err <= 64 * c * 2.0 ** -64, (n, err, c)
        assert err <= float(pc.ref_error(A, x, b)[0]) * 4 + 2.0 ** -60


@pytest.mark.parametrize("n", [1, 37, 64, 65, 200])
def test_chol64_matches_numpy_on_the_well_conditioned_family(n):
    A = pc.wellcond(n, 7)
    b = np.random.default_rng(n).normal(size=n)
    x, ref = pc.chol64(A, b), np.linalg.solve(A, b)
    assert np.abs(x - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    X = pc.chol64(A, np.stack([b, 2.0 * b], axis=1))                 # several right-hand sides: the same bits per column
    assert np.array_equal(X[:, 0], x) and np.array_equal(X[:, 1], 2.0 * x)
    assert pc.chol64(-A, b) is None


@pytest.mark.parametrize("n", [128, 130, 192])
def test_indefinite_fails_at_the_named_pivot_and_not_before(n):
    for k in (0, 1, 62, 63, 64, 65, 127, 128, n - 1):
        if k >= n:
            continue
        A = pc.indefinite(n, k, 0)
        assert np.array_equal(A, A.T)
        if k:
            assert np.linalg.eigvalsh(A[:k, :k]).min() > 1e-3, (n, k)     # leading minors 1 .. k positive, with room
        sign, _ = np.linalg.slogdet(A[:k + 1, :k + 1])
        assert sign == -1.0 and np.linalg.eigvalsh(A[:k + 1, :k + 1]).min() < -1e-3, (n, k)
        # the float64 restatement meets the pivot -1 there
        W = np.array(A)
        for j in range(k + 1):
            assert (W[j, j] > 0) == (j < k), (n, k, j)
            if j < k:
                W[j:, j] /= np.sqrt(W[j, j])
                W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j], W[j + 1:, j])
        assert abs(W[k, k] + 1.0) <= 1e-9
        assert pc.chol64(A, np.ones(n)) is None
