"""Cases, an extended-precision reference, a float64 restatement and the bars for the pose graph's linear solves: the blocked Cholesky of
csrc/k_posegraph.hip (k_potrf64 / k_trsm64 / k_syrk64 / k_trisolve_pipe), the chain-segment elimination (pg_seg_elim_wave /
pg_seg_backsub_wave) and the 256-thread Cholesky of csrc/k_pg_chol_body.inc.  CPU only, numpy only.

  solve_ref(A, b)   right-looking Cholesky and both triangular solves in numpy.longdouble (64-bit significand) with one step of iterative
                    refinement; A and b are float64 inputs taken as exact.  b may hold several right-hand sides as columns.
  chol64(A, b)      the same algorithm in float64, a plain column loop: the restatement whose error sets the bars.  None when a pivot is
                    not positive (or not finite).
  bars(A, b)        forward bar = 16 x the restatement's max|x - x_ref| / max|x_ref|, residual bar = 16 x its
                    max|A x - b| / (||A||_inf max|x| + max|b|) with the residual formed in long double; each at least 64 u.  The factor 16
                    is the margin for a summation order other than the restatement's (blocked, MFMA, rsqrt), as in marg_eig_cases.py.
  ref_error(...)    a bound of the reference's own forward error from its long-double residual and numpy.linalg.cond; every case that
                    is compared by value keeps it under 1/64 of the forward bar (tests/test_pg_linear_cases.py).
Every builder draws from a numpy.random.default_rng of its own; the references are computed at run time, so nothing depends on the
generator's bits."""
import numpy as np

U = 2.0 ** -53
BAR_FACTOR, BAR_MIN = 16.0, 64 * U
REF_MARGIN = 64.0
LD = np.longdouble

# the dense orders of the issue: k_potrf64 alone, one to four trailing block rows, an off-diagonal k_syrk64 tile (> 128), 1..63 padding
# rows, a five-stage k_trisolve_pipe
ORDERS_ALL_FAMILIES = (64, 65, 129, 257)
ORDERS_ONE_SPECTRUM = (1, 2, 63, 127, 128, 193)
FAMILIES = ("spectrum6", "spectrum10", "spectrum12", "graded", "block_chain", "wellcond")


# ---------------------------------------------------------------------------------------------------------------- reference
def _have_longdouble():
    return np.finfo(LD).nmant >= 63


def _chol_solve(A, B, dtype):
    """(X, L) of the right-looking Cholesky A = L L^T and L y = b, L^T x = y in `dtype`; L is None when a pivot is not positive and
    finite"""
    W = np.array(A, dtype=dtype)
    n = W.shape[0]
    for k in range(n):
        piv = W[k, k]
        if not (piv > 0) or not np.isfinite(piv):
            return None, None
        W[k:, k] = W[k:, k] / np.sqrt(piv)
        if k + 1 < n:
            c = W[k + 1:, k]
            W[k + 1:, k + 1:] -= c[:, None] * c[None, :]
    X = _tri_solves(W, np.array(B, dtype=dtype))
    return X, W


def _tri_solves(W, X):
    n = W.shape[0]
    for k in range(n):                       # L y = b, a column per step
        X[k] = X[k] / W[k, k]
        if k + 1 < n:
            X[k + 1:] -= W[k + 1:, k, None] * X[k][None, :]
    for k in range(n - 1, -1, -1):           # L^T x = y
        X[k] = X[k] / W[k, k]
        if k > 0:
            X[:k] -= W[k, :k, None] * X[k][None, :]
    return X


def _as_columns(b):
    b = np.asarray(b, dtype=np.float64)
    return (b[:, None], True) if b.ndim == 1 else (b, False)


def _solve_mp(A, B):
    import mpmath
    mpmath.mp.dps = 40
    Am = mpmath.matrix(A.tolist())
    cols = []
    for j in range(B.shape[1]):
        x = mpmath.cholesky_solve(Am, mpmath.matrix(B[:, j].tolist()))
        cols.append([LD(mpmath.nstr(v, 25)) for v in x])
    return np.array(cols, dtype=LD).T


def solve_ref(A, b):
    """x [n] (or [n, m]) as numpy.longdouble"""
    A = np.asarray(A, dtype=np.float64)
    B, vec = _as_columns(b)
    if not _have_longdouble():
        try:
            import mpmath  # noqa: F401
        except ImportError:
            raise AssertionError("numpy.longdouble has fewer than 63 mantissa bits and mpmath is not importable: no reference")
        X = _solve_mp(A, B)
        return X[:, 0] if vec else X
    assert np.finfo(LD).nmant >= 63
    X, W = _chol_solve(A, B, LD)
    assert W is not None, "solve_ref: the matrix is not positive definite"
    R = B.astype(LD) - A.astype(LD) @ X      # one step of iterative refinement, residual in long double
    X = X + _tri_solves(W, R)
    return X[:, 0] if vec else X


def chol64(A, b):
    """the float64 restatement: x [n] (or [n, m]) float64, or None when a pivot is not positive"""
    B, vec = _as_columns(b)
    with np.errstate(all="ignore"):
        X, W = _chol_solve(np.asarray(A, dtype=np.float64), B, np.float64)
    if W is None:
        return None
    return X[:, 0] if vec else X


# ------------------------------------------------------------------------------------------------------------------ measures
def forward_error(x, x_ref):
    """max|x - x_ref| / max|x_ref| per right-hand side, formed in long double"""
    x, x_ref = np.asarray(x, dtype=LD), np.asarray(x_ref, dtype=LD)
    d = np.abs(x - x_ref).max(axis=0)
    m = np.abs(x_ref).max(axis=0)
    return np.asarray(d / np.where(m > 0, m, 1), dtype=np.float64)


def scaled_residual(A, x, b):
    """max|A x - b| / (||A||_inf max|x| + max|b|) per right-hand side, the residual formed in long double"""
    Al, xl, bl = np.asarray(A, dtype=LD), np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    r = np.abs(Al @ xl - bl).max(axis=0)
    den = np.abs(Al).sum(axis=1).max() * np.abs(xl).max(axis=0) + np.abs(bl).max(axis=0)
    return np.asarray(r / np.where(den > 0, den, 1), dtype=np.float64)


def ref_error(A, x_ref, b):
    """the smaller of the two bounds of ref_error_bounds, per right-hand side"""
    e_norm, e_comp = ref_error_bounds(A, x_ref, b)
    return np.minimum(e_norm, e_comp)


def ref_error_bounds(A, x_ref, b):
    """(norm bound, componentwise bound) of max|x_ref - x| / max|x| per right-hand side.  With r = b - A x_ref (long double) the error is A^-1 r.  In the
    variables of the unit-diagonal matrix A^ = S^-1 A S^-1, S = sqrt(diag A) — the scaling under which Cholesky's error is measured
    (van der Sluis), and without which a graded matrix D M D would be charged the condition of D^2 —
        |e_i| <= ||A^^-1||_2 ||S^-1 r||_2 / s_i,    ||A^^-1||_2 = cond_2(A^) / ||A^||_2.
    That bound charges every component the worst direction of A^^-1 and a factor sqrt(n) for the norms; the componentwise bound of the
    same quantities, |e| <= S^-1 |A^^-1| S^-1 |r| with the float64 inverse of A^ (known to cond_2(A^) u of its norm: cases up to 1e12
    leave four digits, and a bound needs one), is never worse in exact arithmetic.
    Which cases need the second: none of the dense cases (worst ratio to the forward bar 1.1e-2 with the norm bound alone, under 1/64 =
    1.6e-2) and 85 of the 86 step-probe systems of tests/test_gpu_pg_linear.py, which prints both per system.  The one that does is the
    anisotropic configuration on n97_sep11 at radius 1e16: norm bound 2.5e-2 of the forward bar, componentwise 1.5e-3.  The condition
    (1/64) is the same for every case; this is a sharper bound of the same residual, not a wider admission."""
    A = np.asarray(A, dtype=np.float64)
    s = np.sqrt(np.diag(A))
    Ah = A / np.outer(s, s)
    inv_norm = np.linalg.cond(Ah) / np.linalg.norm(Ah, 2)
    xl = np.asarray(x_ref, dtype=LD)
    r = np.asarray(b, dtype=LD) - A.astype(LD) @ xl
    if r.ndim == 1:
        r, xl = r[:, None], xl[:, None]
    rs = np.abs(r) / s.astype(LD)[:, None]
    e_norm = inv_norm * np.sqrt((rs * rs).sum(axis=0)) / s.min()
    e_comp = ((np.abs(np.linalg.inv(Ah)).astype(LD) @ rs) / s.astype(LD)[:, None]).max(axis=0)
    xmax = np.abs(xl).max(axis=0)
    return np.asarray(e_norm / xmax, dtype=np.float64), np.asarray(e_comp / xmax, dtype=np.float64)


def bars(A, b):
    """dict(x_ref, x64, forward, residual, forward64, residual64): the bars per right-hand side, from the restatement's own error"""
    x_ref = solve_ref(A, b)
    x64 = chol64(A, b)
    assert x64 is not None, "bars: the float64 restatement meets a pivot that is not positive"
    f64, r64 = forward_error(x64, x_ref), scaled_residual(A, x64, b)
    return dict(x_ref=x_ref, x64=x64, forward64=f64, residual64=r64, forward=np.maximum(BAR_FACTOR * f64, BAR_MIN),
                residual=np.maximum(BAR_FACTOR * r64, BAR_MIN))


def reference_is_good(A, b, bar=None):
    """the condition on a case that is compared by value: (ok, worst ref_error / forward bar), ok when the ratio is <= 1/64"""
    bar = bars(A, b) if bar is None else bar
    ratio = float(np.max(ref_error(A, bar["x_ref"], b) / bar["forward"]))
    return ratio <= 1.0 / REF_MARGIN, ratio


# --------------------------------------------------------------------------------------------------------------------- cases
def _orth(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.where(np.diag(r) < 0, -1.0, 1.0)


def sym_from_lower(A):
    """exactly symmetric, from the lower triangle (the triangle the device reads)"""
    return np.tril(A) + np.tril(A, -1).T


def spectrum(n, k, seed):
    """Q diag(logspace(0, -k, n)) Q^T: condition 10^k (n > 1)"""
    rng = np.random.default_rng([n, k, seed, 1])
    q = _orth(rng, n)
    return sym_from_lower((q * np.logspace(0.0, -float(k), n)) @ q.T)


def wellcond(n, seed):
    """M M^T + n I, the family of test_dense_spd_solve_matches_numpy"""
    rng = np.random.default_rng([n, seed, 2])
    M = rng.normal(size=(n, n))
    return sym_from_lower(M @ M.T + n * np.eye(n))


def graded(n, seed):
    """D M D, M well conditioned and D = logspace(-4, 4, n) shuffled: metres against radians, what the Jacobi scaling is there for"""
    rng = np.random.default_rng([n, seed, 3])
    q = _orth(rng, n)
    M = (q * np.linspace(1.0, 3.0, n)) @ q.T
    d = rng.permutation(np.logspace(-4.0, 4.0, n))
    return sym_from_lower(d[:, None] * M * d[None, :])


def block_chain(n, seed):
    """The pose graph's shape: 6 x 6 blocks, block tridiagonal (chain edges), a few loop blocks and an arrow onto the first block, as a
    sum of W_e^T W_e over edges plus a weak prior; the leading n x n part of ceil(n / 6) blocks"""
    rng = np.random.default_rng([n, seed, 4])
    nb = (n + 5) // 6
    A = 1e-3 * np.eye(6 * nb)
    edges = [(i, i + 1, 1.0) for i in range(nb - 1)]
    edges += [(0, j, 0.1) for j in range(2, nb, 3)]                                     # the arrow
    for _ in range(min(4, max(nb - 3, 0))):                                            # loops
        i, j = sorted(rng.choice(nb, size=2, replace=False))
        if j - i > 1:
            edges.append((int(i), int(j), 3.0))
    for i, j, w in edges:
        W = w * rng.normal(size=(6, 12)) * np.array([1.0, 1.0, 1.0, 10.0, 10.0, 10.0] * 2)[None, :]
        idx = np.r_[6 * i:6 * i + 6, 6 * j:6 * j + 6]
        A[np.ix_(idx, idx)] += W.T @ W
    return sym_from_lower(A[:n, :n])


def indefinite(n, k, seed):
    """L diag(s) L^T with L unit lower triangular, s = 1 except s_k = -1: the leading minors are positive up to order k and the one of
    order k + 1 is not, so a Cholesky fails at pivot k (where it meets -1) and not before"""
    rng = np.random.default_rng([n, k, seed, 5])
    Lw = np.eye(n) + np.tril(rng.uniform(-1.0, 1.0, size=(n, n)), -1) / np.sqrt(n)
    s = np.ones(n)
    s[k] = -1.0
    return sym_from_lower((Lw * s) @ Lw.T)


def family(name, n, seed=0):
    if name.startswith("spectrum"):
        return spectrum(n, int(name[len("spectrum"):]), seed)
    return {"graded": graded, "block_chain": block_chain, "wellcond": wellcond}[name](n, seed)


def dense_cases():
    """[(family, n)]: every family at ORDERS_ALL_FAMILIES, one spectrum case at each of the remaining orders"""
    out = [(f, n) for n in ORDERS_ALL_FAMILIES for f in FAMILIES]
    out += [("spectrum%d" % (6, 10, 12)[i % 3], n) for i, n in enumerate(ORDERS_ONE_SPECTRUM)]
    return out


def rhs_set(A, seed=0):
    """(names, B [n, m]): a random vector, A @ ones, and the unit vectors e_k, k in {0, 63, 64, n - 1} where they exist — a unit
    vector returns one column of the inverse, so an error confined to one tile shows undiluted"""
    n = A.shape[0]
    rng = np.random.default_rng([n, seed, 6])
    names, cols = ["random", "A@ones"], [rng.normal(size=n), A @ np.ones(n)]
    for k in sorted({0, 63, 64, n - 1}):
        if 0 <= k < n:
            e = np.zeros(n)
            e[k] = 1.0
            names.append("e%d" % k)
            cols.append(e)
    return names, np.stack(cols, axis=1)
