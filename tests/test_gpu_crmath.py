"""The device compile of csrc/liw_crmath.hpp — the sin / cos / atan2 k_lfe_track_begin evaluates — through the diagnostic entry
liw_lfe_crmath_eval (laser_batch.BatchFrontEnd.crmath_eval), over tests/golden/crmath_cases.npz: one launch per function, and per
family the conditions tests/test_crmath.py puts on the host compile (tests/crmath_cases.py states them).  The correctly-rounded bar
holds on the device in full: the Newton start of cr_atan2 is the device library's atan2, a few ulp off, which is what the correction
is for.  Where the plain device functions answer (fallback_finite: |x| > 2^20, atan2 outside the 1e+-300 guards) the error is
measured against the fixture; the figures are in DESIGN.md section 3.  Then the entry itself: sizes around the wave and the
work-group with guard bands, out aliasing a, a non-default stream, two runs, every LIW_EINVAL."""
import ctypes as C

import numpy as np
import pytest

import crmath_cases as cc

pytestmark = pytest.mark.gpu

D = cc.load()
MAIN = [f for f in D["families"] if not f.startswith("fallback")]
G, FILL = 256, -7.25
# the plain device functions, measured on an MI355X: worst error from the exact value in fallback_finite 0.572 ulp (sin / cos of
# 2^20 < |x| <= 1e15) and 1.022 ulp (atan2 outside the guards); the bar is the worst figure rounded up to a whole ulp, plus one
FALLBACK_BAR_ULP = 3.0


def _dev(torch, u):
    return torch.from_numpy(np.ascontiguousarray(u, dtype=np.uint64).view(np.int64).copy()).cuda().view(torch.float64)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def fe(liw):
    f = liw.laser_batch.BatchFrontEnd(liw.laser.office_laser_params(), dict(B=1, slots=1, max_points=8, max_lines=4, max_cell_entries=16))
    yield f
    f.close()


@pytest.fixture(scope="module")
def device(fe):
    """the device build's results over the whole fixture: one launch per function"""
    import torch
    got = np.zeros(len(D["op"]), dtype=np.uint64)
    for op in (cc.SIN, cc.COS, cc.ATAN2):
        idx = np.nonzero(D["op"] == op)[0]
        assert 0 < len(idx) <= 5000
        out = fe.crmath_eval(op, _dev(torch, D["a"][idx]), _dev(torch, D["b"][idx]) if op == cc.ATAN2 else None)
        got[idx] = _bits(out)
    torch.cuda.synchronize()
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("family", MAIN)
def test_main_domain_is_correctly_rounded(device, family):
    sel = D["family"] == family
    bad = cc.main_domain_failures(D, device, sel)
    with np.errstate(invalid="ignore"):
        worst = float(np.nanmax(cc.ulp_error(device[sel], D["want"][sel], D["frac"][sel])))
    print("%s on the device: %d records, %d off the correctly rounded result, worst error %.3f ulp" % (family, int(sel.sum()), len(bad), worst))
    assert len(bad) == 0, cc.describe(D, device, bad)


def test_fallback_special_values(device):
    sel = D["family"] == "fallback_special"
    bad = cc.special_failures(D, device, sel)
    assert len(bad) == 0, cc.describe(D, device, bad)
    neg0 = (D["op"] == cc.SIN) & (D["a"] == np.uint64(1 << 63))
    assert neg0.any() and (device[neg0] == np.uint64(1 << 63)).all()   # cr_sin(-0.0) is -0.0


def test_fallback_finite_within_its_measured_bar(device):
    sel = D["family"] == "fallback_finite"
    assert not cc.is_nan(device[sel]).any()
    err = cc.ulp_error(device[sel], D["want"][sel], D["frac"][sel])
    for name, m in (("sin / cos of 2^20 < |x| <= 1e15", D["op"][sel] != cc.ATAN2), ("atan2 outside the 1e+-300 guards", D["op"][sel] == cc.ATAN2)):
        print("fallback_finite on the device, %s: %d records, %d not correctly rounded, worst %.3f ulp" % (name, int(m.sum()), int((device[sel][m] != D["want"][sel][m]).sum()),
                                                                                                           float(err[m].max())))
    worst = int(np.argmax(err))
    assert float(err.max()) <= FALLBACK_BAR_ULP, cc.describe(D, device, np.nonzero(sel)[0][[worst]])


def test_host_and_device_builds_differ_in(device, tmp_path):
    """recorded, not asserted: the number of fixture records on which the two compiles of the header differ
    bitwise, outside the fallback families, whose functions are different libraries"""
    host = cc.host_build(tmp_path)(D["op"], D["a"], D["b"])
    main = ~np.char.startswith(D["family"], "fallback")
    diff = main & (host != device)
    print("host and device builds of liw_crmath.hpp: %d of %d main-domain records differ bitwise (fallback records: %d of %d)"
          % (int(diff.sum()), int(main.sum()), int((~main & (host != device) & ~(cc.is_nan(host) & cc.is_nan(device))).sum()), int((~main).sum())))
    assert len(host) == len(device)


# ----------------------------------------------------------------------------------------------------------- the entry itself
def _records(n, op):
    """the first n records of op among the neighbours of the multiples of pi/2 (atan2: the random directions and the axes)"""
    fams = ("near_multiple",) if op != cc.ATAN2 else ("atan2_random", "atan2_axis")
    idx = np.nonzero((D["op"] == op) & np.isin(D["family"], fams))[0][:n]
    assert len(idx) == n
    return idx


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 257])
@pytest.mark.parametrize("op", [cc.SIN, cc.ATAN2])
def test_sizes_and_guard_bands(fe, n, op):
    import torch
    idx = _records(n, op)
    buf = torch.full((n + 2 * G,), FILL, dtype=torch.float64, device="cuda")
    out = buf[G:G + n]
    fe.crmath_eval(op, _dev(torch, D["a"][idx]), _dev(torch, D["b"][idx]) if op == cc.ATAN2 else None, out=out)
    torch.cuda.synchronize()
    assert bool((buf[:G] == FILL).all()) and bool((buf[-G:] == FILL).all())
    assert np.array_equal(_bits(out), D["want"][idx])


@pytest.mark.parametrize("op", [cc.COS, cc.ATAN2])
def test_out_may_alias_a(fe, op):
    import torch
    idx = _records(257, op)
    a = _dev(torch, D["a"][idx])
    r = fe.crmath_eval(op, a, _dev(torch, D["b"][idx]) if op == cc.ATAN2 else None, out=a)
    torch.cuda.synchronize()
    assert r.data_ptr() == a.data_ptr() and np.array_equal(_bits(a), D["want"][idx])


def test_non_default_stream(fe):
    import torch
    idx = _records(130, cc.COS)
    a = _dev(torch, D["a"][idx])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = fe.crmath_eval(cc.COS, a)
    s.synchronize()
    assert np.array_equal(_bits(out), D["want"][idx])


def test_two_runs_are_bit_identical(fe):
    import torch
    sel = np.nonzero(D["op"] == cc.ATAN2)[0]
    a, b = _dev(torch, D["a"][sel]), _dev(torch, D["b"][sel])
    r1, r2 = fe.crmath_eval(cc.ATAN2, a, b), fe.crmath_eval(cc.ATAN2, a, b)
    torch.cuda.synchronize()
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64))


def test_einval_and_empty(fe):
    import torch
    L, h = fe.L, fe.h
    idx = _records(8, cc.SIN)
    a = _dev(torch, D["a"][idx])
    b, out = a.clone(), torch.full((8,), FILL, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    E = -22
    assert L.liw_lfe_crmath_eval(None, 0, 8, p(a), p(b), p(out), None) == E
    for op in (-1, 3, 7):
        assert L.liw_lfe_crmath_eval(h, op, 8, p(a), p(b), p(out), None) == E
    assert L.liw_lfe_crmath_eval(h, 0, -1, p(a), p(b), p(out), None) == E
    for op in (0, 1, 2):
        assert L.liw_lfe_crmath_eval(h, op, 8, None, p(b), p(out), None) == E
        assert L.liw_lfe_crmath_eval(h, op, 8, p(a), p(b), None, None) == E
    assert L.liw_lfe_crmath_eval(h, 2, 8, p(a), None, p(out), None) == E
    for op in (0, 1, 2):
        assert L.liw_lfe_crmath_eval(h, op, 0, p(a), p(b), p(out), None) == 0   # n = 0: LIW_OK, nothing launched
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # b may be null for sin and cos
    assert L.liw_lfe_crmath_eval(h, 0, 8, p(a), None, p(out), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), D["want"][idx])
