"""The fixture of the eigen square root tests (tests/golden/marg_eig_cases.npz) and the float64 restatement of the kernels' algorithm
(tests/marg_eig_cases.py), without a GPU: the conditions the generator asserted hold on the committed file, the restatement meets
every assertion tests/test_gpu_marg_eig.py makes of the device with the same bars, and it runs into the 60-sweep cap on rank-deficient
input.  Also: the hook's argument checks that need no device."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import marg_eig_cases as mc


@pytest.fixture(scope="module")
def fx():
    return mc.load()


@pytest.fixture(scope="module")
def restated(fx):
    return [mc.restate(fx["dH"][i], fx["dg"][i]) for i in range(len(mc.NAMES))]


def test_fixture_layout(fx):
    N, M = len(mc.NAMES), len(mc.MEASURES)
    shapes = dict(dH=(N, 15, 15), dg=(N, 15), lam=(N, 15), vec=(N, 15, 15), sweeps=(N,), restate=(N, M), bars=(M,))
    assert sorted(fx) == sorted(shapes)
    for k, s in shapes.items():
        assert fx[k].shape == s and fx[k].dtype == np.float64, k
    assert os.path.getsize(mc.PATH) < 150 * 1000
    assert np.isfinite(fx["dH"]).all() and np.isfinite(fx["dg"]).all()
    assert np.all(np.diff(fx["lam"], axis=1) >= 0.0)
    # unit eigenvectors, largest |component| positive
    assert np.abs(np.linalg.norm(fx["vec"], axis=2) - 1.0).max() <= 4 * mc.U
    big = np.take_along_axis(fx["vec"], np.abs(fx["vec"]).argmax(axis=2)[..., None], axis=2)
    assert (big > 0.0).all()
    assert np.array_equal(fx["bars"], mc.bars_from(fx["restate"])) and (fx["bars"] >= mc.BAR_MIN).all()


def test_case_conditions(fx):
    for i, name in enumerate(mc.NAMES):
        H = fx["dH"][i]
        if name not in mc.EXACT:
            mc.assert_floor_margin(name, H, fx["lam"][i])
        if name != "skew":
            assert np.array_equal(H, H.T), name
    # what the cases are there for
    kept = {name: int(mc.kept_of(fx["lam"][i]).sum()) for i, name in enumerate(mc.NAMES)}
    assert (kept["rank12"], kept["rank8"], kept["rank1"], kept["zero"], kept["zero_rows"]) == (12, 8, 1, 0, 13)
    assert (kept["indef"], kept["small_norm"], kept["diag_floor"], kept["scale_down"], kept["scale_up"]) == (13, 10, 11, 0, 15)
    assert np.array_equal(np.diag(fx["dH"][mc.case_index("diag_floor")]), np.array(mc.DIAG_FLOOR))
    pr = fx["dH"][mc.case_index("pairs")]
    assert sum(1 for p in range(15) for q in range(p + 1, 15) if pr[p, q] != 0.0 and pr[p, p] == pr[q, q]) == 7   # d == 0 rotations
    i, j = mc.case_index("skew"), mc.case_index("skew_sym")
    S = fx["dH"][i]
    assert not np.array_equal(S, S.T) and np.array_equal(0.5 * (S + S.T), fx["dH"][j]) and np.array_equal(fx["dg"][i], fx["dg"][j])
    assert np.abs(S - S.T).max() / 2 <= 4.0 and np.array_equal(S * 2.0 ** 30, np.round(S * 2.0 ** 30))


def test_restatement_meets_every_bar(fx, restated):
    for i, name in enumerate(mc.NAMES):
        J, R, _ = restated[i]
        fig = mc.measures(name, fx["dH"][i], fx["dg"][i], fx["lam"][i], fx["vec"][i], J, R)
        print("%-14s " % name + "  ".join("%s %.1e" % (m, fig[m]) for m in mc.MEASURES + ["eig_rel"]))
        mc.check_bars(name, fig, fx["bars"])
        if name in mc.EXACT:
            assert fig["exact_ulp"] == 0.0
    print("bars           " + "  ".join("%s %.1e" % (m, b) for m, b in zip(mc.MEASURES, fx["bars"])))


def test_restatement_sweeps(fx, restated):
    sweeps = {name: restated[i][2] for i, name in enumerate(mc.NAMES)}
    assert [sweeps[n] for n in mc.NAMES] == [int(s) for s in fx["sweeps"]]
    assert sweeps["diag_floor"] == 0 and sweeps["ident"] == 0 and sweeps["zero"] == 0
    # a numerical null space of three and more dimensions never meets the stop test: the sweep cap ends the iteration
    assert sweeps["rank8"] == mc.SWEEP_CAP and sweeps["rank1"] == mc.SWEEP_CAP
    assert 3 <= sweeps["dense"] <= 10 and 3 <= sweeps["graded"] <= 10
    # the stop test is normwise: one sweep, and the 1e-6 block is left far from converged on its own scale
    i = mc.case_index("big_plus_tiny")
    assert sweeps["big_plus_tiny"] == 1
    J = restated[i][0]
    rel = np.abs((J * J).sum(axis=1) - fx["lam"][i]) / fx["lam"][i]
    assert rel[:5].max() > 1e-3 and rel[5:].max() <= fx["bars"][0]


def test_skew_restatement_is_bit_identical_to_its_symmetric_twin(fx, restated):
    i, j = mc.case_index("skew"), mc.case_index("skew_sym")
    assert np.array_equal(restated[i][0], restated[j][0]) and np.array_equal(restated[i][1], restated[j][1])


def test_two_cases_recomputed_with_mpmath(fx):
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_golden_marg_eig", os.path.join(mc.HERE, "golden", "make_golden_marg_eig.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for name in ("graded_perm", "rank8"):
        i = mc.case_index(name)
        lam, vec = gen.eigsy(fx["dH"][i])
        assert np.array_equal(lam, fx["lam"][i]), name
        simple = mc.gaps(fx["lam"][i]) > 1e-3
        assert np.array_equal(vec[simple], fx["vec"][i][simple]), name


def test_probe_argument_checks_without_a_device(liw, synth):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = liw.lib()
    ps = liw.params_struct(synth.office_params(), 0)
    h = C.c_void_p(L.liw_create(C.byref(ps)))
    assert h
    try:
        b = liw.BatchC()
        b.B, b.n = 1, 2
        buf = (C.c_double * 225)()
        p, null = C.cast(buf, C.c_void_p), C.c_void_p(None)
        call = lambda variant, dH, dg: L.liw_batch_marg_eig_probe(h, C.byref(b), null, C.c_int(variant), dH, dg, null, null, null)
        assert call(0, null, p) == liw.LIW_EINVAL and call(0, p, null) == liw.LIW_EINVAL
        assert call(-1, p, p) == liw.LIW_EINVAL and call(3, p, p) == liw.LIW_EINVAL
        for variant in (0, 1, 2):
            assert call(variant, p, p) == liw.LIW_ENODEV      # no CPU fallback
    finally:
        L.liw_destroy(h)
