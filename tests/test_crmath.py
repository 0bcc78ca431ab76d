"""csrc/liw_crmath.hpp — the correctly rounded sin / cos / atan2 of the tracking glue — compiled for the host alone
(tests/cpp/crmath_driver.cpp) and replayed over tests/golden/crmath_cases.npz without a GPU: every main-domain family must give the
bits of the correctly rounded result (tests/crmath_cases.py states the bar and its one exemption), the fallback family the special
values of the plain functions.  The device compile of the same header: tests/test_gpu_crmath.py.

The header as it was before it reduced its argument modulo pi/2 (|x| halved down to 0.25, then up to 22 double-angle steps) fails two
families here: near_multiple, 78 of 2 754 records off by up to 6.7 ulp, and big_multiple, 217 of 500 off by up to 2 862 ulp."""
import importlib.util
import math
import os

import numpy as np
import pytest

import crmath_cases as cc

D = cc.load()
MAIN = [f for f in D["families"] if not f.startswith("fallback")]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host build's results over the whole fixture, computed once"""
    run = cc.host_build(tmp_path_factory.mktemp("crmath"))
    got = run(D["op"], D["a"], D["b"])
    got.setflags(write=False)
    return got


def test_fixture_shape():
    n = len(D["op"])
    assert 4500 <= n <= 6500 and os.path.getsize(cc.PATH) <= 256 * 1024
    assert D["dropped"] <= 1e-3 * n
    for f in D["families"]:
        assert int((D["family"] == f).sum()) >= 20, f
    assert (np.abs(D["frac"]) <= 0.5).all()
    # the enumerated neighbours: 17 multiples x 81 doubles x 2 functions
    if D["dropped"] == 0:
        assert int((D["family"] == "near_multiple").sum()) == 17 * 81 * 2
    # each launch of the device test takes one op's records
    assert max(int((D["op"] == op).sum()) for op in (0, 1, 2)) <= 5000


@pytest.mark.parametrize("family", MAIN)
def test_main_domain_is_correctly_rounded(host, family):
    sel = D["family"] == family
    bad = cc.main_domain_failures(D, host, sel)
    worst = float(cc.ulp_error(host[sel], D["want"][sel], D["frac"][sel]).max())
    print("%s: %d records, %d off the correctly rounded result, worst error %.3f ulp" % (family, int(sel.sum()), len(bad), worst))
    assert len(bad) == 0, cc.describe(D, host, bad)


def test_fallback_special_values(host):
    sel = D["family"] == "fallback_special"
    bad = cc.special_failures(D, host, sel)
    assert len(bad) == 0, cc.describe(D, host, bad)
    # the fixture's special records are math.atan2's on this machine too, and NaN for sin / cos of an infinity
    f = lambda s, c: cc.u64([math.atan2(s, c)])[0]
    rec = {(int(o), int(a), int(b)): int(w) for o, a, b, w in zip(D["op"][sel], D["a"][sel], D["b"][sel], D["want"][sel])}
    for s in (0.0, -0.0):
        for c in (0.0, -0.0, float("inf"), -float("inf")):
            assert rec[(2, int(cc.u64([s])[0]), int(cc.u64([c])[0]))] == int(f(s, c))
    inf = int(cc.u64([float("inf")])[0])
    for op in (0, 1):
        assert cc.is_nan(np.uint64(rec[(op, inf, 0)])) and cc.is_nan(np.uint64(rec[(op, inf | (1 << 63), 0)]))


def test_sign_of_zero(host):
    run_sel = (D["op"] == cc.SIN) & (D["a"] == np.uint64(1 << 63))
    assert run_sel.any() and (host[run_sel] == np.uint64(1 << 63)).all()          # cr_sin(-0.0) is -0.0
    pos = (D["op"] == cc.SIN) & (D["a"] == np.uint64(0))
    assert pos.any() and (host[pos] == np.uint64(0)).all()


def test_fallback_finite_on_the_host(host):
    """host libm answers here: no bar of this project's (glibc states 1 ulp for these); the figure is printed"""
    sel = D["family"] == "fallback_finite"
    err = cc.ulp_error(host[sel], D["want"][sel], D["frac"][sel])
    print("fallback_finite on the host: %d records, %d not correctly rounded, worst %.3f ulp" % (int(sel.sum()), int((host[sel] != D["want"][sel]).sum()), float(err.max())))
    assert not cc.is_nan(host[sel]).any()


def test_the_bar_has_teeth():
    """The comparison is on bits: a result one ulp from the fixture's value fails, in either direction, for every enumerated
    neighbour of a multiple of pi/2 (so a result merely within 2 ulp fails).  And the fixture is not a record of the code's own
    output: it holds the two values every text on argument reduction quotes."""
    sel = D["family"] == "near_multiple"
    want = D["want"][sel]
    finite_nonzero = (want & ~cc.SIGN) != 0
    for delta in (1, -1):
        off = np.where(finite_nonzero, (want.astype(np.int64) + delta).astype(np.uint64), want ^ np.uint64(1))   # 0 -> the smallest subnormal
        assert (off != want).all()
        got = D["want"].copy()
        got[sel] = off
        assert len(cc.main_domain_failures(D, got, sel)) == int(sel.sum())
    rec = {(int(o), int(a)): int(w) for o, a, w in zip(D["op"][sel], D["a"][sel], D["want"][sel])}
    for op, x, value in cc.sin_of_pi_and_cos_of_half_pi():
        assert rec[(op, int(cc.u64([x])[0]))] == int(cc.u64([value])[0]), (op, x)


def test_fixture_regenerates():
    """with mpmath at hand: the committed generator's case list is the file's, and 200 records recomputed equal the file's"""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_golden_crmath", os.path.join(cc.ROOT, "tests", "golden", "make_golden_crmath.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.FAMILIES == D["families"]
    cases = gen.build_cases()
    assert len(cases) == len(D["op"]) + D["dropped"]
    if D["dropped"] == 0:
        assert [c[0] for c in cases] == list(D["family"])
        assert np.array_equal(np.array([c[1] for c in cases], dtype=np.uint8), D["op"])
        assert np.array_equal(np.array([gen.bits(c[2]) for c in cases], dtype=np.uint64), D["a"])
        assert np.array_equal(np.array([gen.bits(c[3]) for c in cases], dtype=np.uint64), D["b"])
    n = len(D["op"])
    for i in range(0, n, max(1, n // 200)):
        a, b = gen.from_bits(D["a"][i]), gen.from_bits(D["b"][i])
        if D["family"][i] == "fallback_special":
            want, frac = gen.special(int(D["op"][i]), a, b), 0.0
        else:
            want, frac, dist = gen.record(int(D["op"][i]), a, b)
            assert dist >= gen.DROP_BELOW or D["family"][i] == "fallback_finite"
        if math.isnan(want):
            assert cc.is_nan(D["want"][i])
        else:
            assert gen.bits(want) == int(D["want"][i]) and frac == float(D["frac"][i]), i
