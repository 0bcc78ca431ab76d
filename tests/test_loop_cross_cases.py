"""Guards of the cross-robot loop cases (tests/loop_cross_cases.py) on the host restatement alone, on any machine: every decision the
cases are there for occurs, and none of them is made within round-off of a threshold, so that "the device decides what the
restatement decides" (tests/test_gpu_loop_cross.py) is a statement about the kernels and not about rounding.

Sizes are integers and the device computes them with the bodies whose parity tests/test_gpu_loop.py establishes, so "where a size
decides" is read as: the chosen candidate of a found query is above min_match by at least 2, and a query that launched candidates
and found nothing has no size above min_match - 2."""
import numpy as np
import pytest

import loop_cross_cases as xc


@pytest.mark.parametrize("name", xc.FLEETS)
def test_no_decision_is_close_to_a_threshold(name):
    """loop_cross_cases.check: chosen sizes at least 2 above min_match and unique among the passing candidates (except in the tie
    case), not-found queries far below, no rms within 1e-6 relative of max_rms, no angle within 1e-9 of a bin boundary, and every
    T_w1_w2 closer to the truth than the bound derived from the injected noise."""
    assert xc.check(name) == []


def _passing(r):
    return {i: c for i, c in r["cands"].items() if "rms" in c and not c["rms"] > xc.MAX_RMS}


@pytest.mark.parametrize("name", ("s3", "s1"))
def test_expected_decisions_occur(name):
    F = xc.fleet(name)
    S, mm = xc.SUBMAP[name], xc.MIN_MATCH[name]
    main, odd, claim = [xc.restated(name, c) for c in ("main", "odd", "claim")]
    assert all(k <= 14 for k in F["K"]) and F["dims"]["B"] == 8
    # a pair that links, with several passing candidates of different size
    assert main[1]["found"] and main[1]["edge"][1] == 0 and len({c["match"]["size"] for c in _passing(main[1]).values()}) >= 3
    # a size tie, settled by index
    p5 = _passing(main[5])
    ties = sorted(i for i, c in p5.items() if c["match"]["size"] == main[5]["edge"][3])
    assert len(ties) >= 2 and main[5]["edge"][2] == ties[0] and main[5]["edge"][3] == max(c["match"]["size"] for c in p5.values())
    # a candidate accepted by size and rejected by max_rms: the key frame with the rotated corners
    c4 = main[5]["cands"][4]
    assert c4["match"]["size"] > mm + 1 and c4["rms"] > 1.5 * xc.MAX_RMS and 4 not in p5
    assert all(c["rms"] < 0.5 * xc.MAX_RMS for c in p5.values())
    # a partner in another building
    assert not main[4]["found"] and main[4]["stats"][1] > 0 and main[4]["stats"][4] == 0
    # partner -1, self, out of range, negative; an empty partner; a masked-out robot; key clear
    for a in (0, 1, 2, 3, 4, 7):
        assert odd[a]["found"] == 0 and odd[a]["stats"] == [0] * 6 and odd[a]["edge"] == [-1, -1, -1, 0]
    assert xc.CALLS["odd"][1][:5] == [-1, 1, 8, 6, -7] and F["K"][6] == 0
    assert odd[5] is None and odd[6] == dict(found=0, key=0) and main[6] == dict(found=0, key=0)
    # an invalid query
    D = xc.features(name)
    assert not D[7].features[-1].valid and main[7]["found"] == 0 and main[7]["stats"] == [0] * 6
    if S == 3:
        assert len(D[7].features[-1].points) > xc.MAX_POINTS and all(len(f[2]) <= xc.MAX_KF_CORNERS for f in F["frames"][7])
    else:
        assert len(F["frames"][7][-1][2]) > xc.MAX_KF_CORNERS
    # mutual queries
    assert xc.CALLS["main"][1][0] == 1 and xc.CALLS["main"][1][1] == 0 and main[0]["found"] and main[1]["found"]
    # at least two pairs with K_a = K_b + submap_count
    for a, b in xc.KA_KB_PAIRS:
        assert F["K"][a] == F["K"][b] + S and xc.CALLS["main"][1][a] == b and main[a]["found"]
    # two linked robots claim the unlinked robot 2 in one call; the lowest wins
    assert claim[0]["found"] and claim[1]["found"] and claim[0]["edge"][1] == claim[1]["edge"][1] == 2
    first, second = xc.link_scenarios(name)
    assert second["steps"][0]["linked"] == [1, 1, 1, 0, 1, 0, 0, 0] and second["steps"][0]["via"][2][0] == 0
    # the chain 0 -> 3 -> 5 needs two calls; robot 7 is in no group, robot 6 has nothing to link with
    s1, s2 = first["steps"]
    assert s1["linked"] == [1, 1, 1, 1, 1, 0, 0, 0] and s2["linked"] == [1, 1, 1, 1, 1, 1, 0, 0]
    assert s1["via"][5] == [-1] * 4 and s2["via"][5][0] == 3 and s2["via"][3][0] == 0
    assert s2["group_linked"] == [0, 0, 0, 0, 1, 0, -1, -1]
    # the linked transforms are the truth up to the noise: T_g_w[r] maps r's world into robot 0's
    for r in (1, 2, 3, 5):
        assert np.abs(s2["T_g_w"][r] - xc.truth(name, 0, r)).max() < 0.05


def test_more_than_64_candidates():
    F = xc.fleet("long")
    r = xc.restated("long", "long")[1]
    assert F["K"][0] == 70 and r["stats"][0] == 70 and r["stats"][1] > 64 and r["found"] and r["edge"][2] < 64
    n = [len(f.points) for f in xc.features("long")[0].features]
    assert 6 <= min(n) and max(n) <= 14
    # candidates beyond the first 64 lanes are launched too, and some are accepted ones' neighbours
    assert all(not r["cands"][i]["gate"] for i in range(64, 70))


def test_partner_choice_restated():
    g = xc.GROUP_OF
    assert xc.choose_partners(g, [1, 0, 0, 1, 1, 0, 0, 0], 0) == [-1, 0, 0, -1, -1, 0, 0, -1]
    assert xc.choose_partners(g, [1, 0, 0, 1, 1, 0, 0, 0], 1) == [-1, 3, 3, -1, -1, 3, 3, -1]
    assert xc.choose_partners(g, [0, 0, 0, 0, 1, 0, 0, 0], 5) == [-1] * 8          # group 0 has no linked member; robot 4 is linked


@pytest.mark.parametrize("name", xc.FLEETS)
def test_deviation_from_the_truth(name):
    """The restatement's T_w1_w2 against W_a W_b^-1: below the bound that follows from the +-1 mm corner noise
    (loop_cross_cases.deviation_bound).  The device test uses twice the deviation as its sanity bar against the truth."""
    worst = 0.0
    for call in (["long"] if name == "long" else list(xc.CALLS)):
        for a, r in enumerate(xc.restated(name, call)):
            if r and r["found"]:
                dev = float(np.abs(r["T"] - xc.truth(name, a, r["edge"][1])).max())
                bound = xc.deviation_bound(r["cands"][r["edge"][2]])
                print("%s %s robot %d -> %d: |T_w1_w2 - truth| = %.3e (bound %.3e)" % (name, call, a, r["edge"][1], dev, bound))
                assert 1e-7 < dev < bound
                worst = max(worst, dev)
    assert worst > 0
