"""csrc/liw_lm_rules.hpp — the Ceres trust-region rules every LM loop of the library calls — compiled for the host alone
(tests/cpp/lm_rules_driver.cpp) and checked without a GPU: against the iteration records of the oracle's INIT solves, and
against a table of hand-written cases for the rules those solves never reach."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """ask(list of query lines) -> list of answer lines, each split into words"""
    src = os.path.join(ROOT, "tests", "cpp", "lm_rules_driver.cpp")
    exe = str(tmp_path_factory.mktemp("lm_rules") / "lm_rules_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])

    def ask(queries):
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, check=True)
        out = [l.split() for l in r.stdout.splitlines()]
        assert len(out) == len(queries), r.stderr
        return out
    return ask


def q(op, *args):
    return op + "".join(" " + (float(a).hex() if isinstance(a, float) else str(int(a))) for a in args)


def test_constants_are_ceres_defaults(rules):
    c = rules(["const"])[0]
    got = [float.fromhex(v) for v in c[:9]] + [int(c[9]), float.fromhex(c[10])]
    assert got == [1e-6, 1e32, 1e-3, 1e-6, 1e-10, 1e-8, 1e16, 1e-32, 1e4, 5, 1.7976931348623157e308]


WINDOWS = [(2, 50), (3, 20), (5, 20), (7, 50)]   # (frames, iteration cap), five windows each


def test_replay_of_oracle_iteration_records(rules, synth, pyoracle):
    """Every iteration record of 20 oracle INIT solves goes through the header: rho equals the recorded relative decrease and a
    rejected step's radius the recorded radius exactly, accept equals `successful`, an accepted step's radius is within 8 ulp
    (the oracle cubes with pow(), the header with two multiplications: <= 2 ulp apart, amplified <= 2x by 1 - c where the
    max(1/3, .) clamp is inactive, then one division), the terminating record of a function-tolerance solve gives 2 and every
    earlier one 0, and the cap exits are lm_cap_reached's."""
    failed_cost = float.fromhex(rules(["const"])[0][10])
    prm = synth.office_params()
    orc = pyoracle.Oracle(prm)
    queries, checks = [], []   # one check per query: f(answer words)
    total = replayed = rejected = func_exits = cap_exits = 0

    def expect(query, f):
        queries.append(query)
        checks.append((query, f))

    def eq(want):
        return lambda a: a == [str(v) for v in want]

    for n, cap in WINDOWS:
        for k in range(5):
            d = synth.make_window(orc, prm, seed=4100 + 17 * n + k, n=n, L=20 * n + 37 * k)
            orc.set_max_iterations(cap)
            orc.init_solve(pyoracle.Window(d))
            recs, term = orc.iterations(), orc.summary()["termination"]
            total += len(recs) - 1                       # record 0 is the starting point, not a step
            dec = 2.0
            for i in range(1, len(recs)):
                prev, r = recs[i - 1], recs[i]
                expect(q("cap", i - 1, cap, i == 1), eq([0]))        # the step of iteration i was taken: no cap before it
                expect(q("valid", 1, r["model_cost_change"]), eq([int(r["valid"])]))
                if not r["valid"]:
                    def chk_invalid(a, r=r, dec=dec):
                        assert float.fromhex(a[2]) == r["radius"] and float.fromhex(a[3]) == 2.0 * dec and a[4] == "1"
                        return True
                    expect(q("step", 0.0, 0.0, 1.0, prev["radius"], dec), chk_invalid)   # rho = 0: StepIsInvalid -> StepRejected
                    dec *= 2.0
                    replayed += 1
                    continue
                cc = r["candidate_cost"] if math.isfinite(r["candidate_cost"]) else failed_cost
                if i == len(recs) - 1 and term in (2, 3):
                    assert term == 2, "a parameter-tolerance exit: its step norm is not in the records"
                    expect(q("cand", INF, 1.0, prev["cost"], cc), eq([2]))
                    func_exits += 1
                    replayed += 1
                    continue
                expect(q("cand", INF, 1.0, prev["cost"], cc), eq([0]))

                def chk_step(a, r=r, dec=dec):
                    rho, acc, radius, dec2, reuse = float.fromhex(a[0]), a[1] == "1", float.fromhex(a[2]), float.fromhex(a[3]), int(a[4])
                    assert rho == r["relative_decrease"]
                    assert acc == r["successful"]
                    if acc:
                        assert abs(radius - r["radius"]) <= 8 * math.ulp(r["radius"]), (radius, r["radius"])
                        assert dec2 == 2.0 and reuse == 0
                    else:
                        assert radius == r["radius"]
                        assert dec2 == 2.0 * dec and reuse == 1
                    return True
                expect(q("step", prev["cost"], cc, r["model_cost_change"], prev["radius"], dec), chk_step)
                dec = 2.0 if r["successful"] else 2.0 * dec
                rejected += 0 if r["successful"] else 1
                replayed += 1
            if term == 4:
                assert len(recs) - 1 == cap
                expect(q("cap", len(recs) - 1, cap, 0), eq([1]))
                cap_exits += 1
            else:
                assert term == 2, term
    answers = rules(queries)
    for (query, f), a in zip(checks, answers):
        assert f(a), (query, a)
    print("records %d, rejected %d, function-tolerance exits %d, cap exits %d" % (total, rejected, func_exits, cap_exits))
    assert replayed == total
    assert total >= 300 and rejected >= 50 and func_exits >= 10


DBL_MAX = 1.7976931348623157e308   # what the callers pass for a candidate that failed to evaluate (kFailedEvalCost)
# (query, expected answer, the Ceres rule it states)
TABLE = [
    (q("grad", 1, 1, 1e-10, 1), "1", "GradientToleranceReached after iteration zero: max norm <= gradient_tolerance"),
    (q("grad", 1, 1, 1.0000001e-10, 1), "0", "... and not above it"),
    (q("grad", 0, 1, 5e-11, 1), "1", "GradientToleranceReached after a successful step"),
    (q("grad", 0, 0, 5e-11, 1), "0", "an unsuccessful step does not re-test the gradient it left unchanged"),
    (q("grad", 0, 0, 1.0, 0), "5", "MinTrustRegionRadiusReached: radius <= min_trust_region_radius"),
    (q("grad", 0, 1, 1.0, 1), "0", "a radius above the minimum goes on"),
    (q("grad", 0, 1, 5e-11, 0), "1", "the gradient test comes before the radius test"),
    (q("grad", 0, 1, NAN, 1), "0", "a NaN gradient norm meets no tolerance"),
    (q("cand", 1e-8 * (3.0 + 1e-8), 3.0, 10.0, 5.0), "3", "ParameterToleranceReached: |step| <= parameter_tolerance (|x| + parameter_tolerance)"),
    (q("cand", 3.1e-8, 3.0, 10.0, 5.0), "0", "... and not above it"),
    (q("cand", 0.0, 3.0, 10.0, 10.0), "3", "the parameter test comes before the function test"),
    (q("cand", 1.0, 3.0, 8.0, 8.0 - 2.0 ** -17), "2", "FunctionToleranceReached: |cost change| <= function_tolerance * cost"),
    (q("cand", 1.0, 3.0, 8.0, 8.0 + 2.0 ** -17), "2", "... for a cost increase of that size as well"),
    (q("cand", 1.0, 3.0, 8.0, 8.0 - 2.0 ** -16), "0", "... and not above it (2^-17 < 8e-6 < 2^-16)"),
    (q("cand", 1.0, 3.0, 10.0, DBL_MAX), "0", "a failed evaluation (cost = max double) is no termination ..."),
    (q("step", 10.0, DBL_MAX, 2.0, 1e4, 2.0), ((10.0 - DBL_MAX) / 2.0, 0, 5e3, 4.0, 1), "... it is rejected: StepRejected divides the radius and doubles the factor"),
    (q("step", 10.0, 9.0, 1.0, 1e16, 2.0), (1.0, 1, 1e16, 2.0, 0), "StepAccepted: the radius is capped at max_trust_region_radius"),
    (q("step", 10.0, 9.0, 1.0, 1e4, 8.0), (1.0, 1, 1e4 / (1.0 / 3.0), 2.0, 0), "StepAccepted at rho = 1: radius / max(1/3, 1 - 1) = 3 radius, factor reset"),
    (q("step", 10.0, 9.5, 1.0, 9.0, 2.0), (0.5, 1, 9.0, 2.0, 0), "StepAccepted at rho = 1/2: radius / max(1/3, 1 - 0) unchanged"),
    (q("step", 1e-3, 0.0, 1.0, 8.0, 4.0), (1e-3, 0, 2.0, 8.0, 1), "IsStepSuccessful needs rho > min_relative_decrease, not >="),
    (q("valid", 1, 0.0), "0", "a zero model cost change makes the step invalid"),
    (q("valid", 1, -1e-3), "0", "a negative model cost change makes the step invalid"),
    (q("valid", 1, NAN), "0", "a NaN model cost change makes the step invalid"),
    (q("valid", 1, INF), "0", "an infinite model cost change makes the step invalid"),
    (q("valid", 0, 1.0), "0", "a failed linear solve makes the step invalid"),
    (q("valid", 1, 1e-300), "1", "any finite positive model cost change is valid"),
    (q("gives", 3), "0", "the fourth consecutive invalid step is survived"),
    (q("gives", 4), "1", "max_num_consecutive_invalid_steps = 5: the fifth is FAILURE"),
    (q("cap", 0, 0, 1), "0", "the pass that evaluates iteration zero does not stop at the cap"),
    (q("cap", 12, 12, 0), "1", "MaxSolverIterationsReached: iteration >= max_num_iterations"),
    (q("cap", 11, 12, 0), "0", "... and not below it"),
]


def test_table_of_rules(rules):
    answers = rules([t[0] for t in TABLE])
    for (query, want, rule), a in zip(TABLE, answers):
        if isinstance(want, str):
            assert a == [want], (rule, query, a)
        else:
            got = tuple(float.fromhex(v) if isinstance(w, float) else int(v) for v, w in zip(a, want))
            assert len(a) == len(want) and got == want, (rule, query, got)
