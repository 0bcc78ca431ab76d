"""CPU guards of the second parameter set of the front half (tests/second_config.py: laser_params, loop_params, skewed_params), which
tests/test_gpu_laser_second_config.py, tests/test_gpu_loop.py, tests/test_gpu_loop_batch.py, tests/test_gpu_map.py and
tests/test_gpu_map_batch.py run the kernels at:

  * the host front-end equals the oracle at the laser set, at the bars of tests/test_laser_frontend.py (lines 1e-9, discrete outputs exact);
  * the inputs of the GPU tests reach the arms the office set never reaches (points outside the grid in rows only and in columns only,
    grid coordinates in (-1, 0), lines partly outside the grid, gaps and lengths between the office thresholds and these);
  * they DISCRIMINATE: each single mistake of second_config.laser_mutations changes a discrete output of the oracle on them;
  * no decision sits on a threshold: every discrete output is unchanged when a threshold is scaled by 1 +- 1e-6;
  * the same for the loop detector's sets with tests/loop_reference.py, and for the map's extrinsic with tests/map_reference.py."""
import math

import numpy as np
import pytest

import loop_batch_cases as cases
import loop_reference as ref
import map_batch_cases as mc
import map_reference
import second_config as sc
import test_gpu_loop as tgl
from test_laser_frontend import same_lines

MARGIN = 1e-9           # tests/test_gpu_loop.py
SCALE = 1e-6            # the relative change of a threshold that must not change a decision
B = len(sc.ROOMS) * sc.POSES_PER_ROOM
ROOM_ROBOTS = tuple(range(0, B, sc.POSES_PER_ROOM))    # one robot per room: the six rooms of tests/test_laser_frontend.py
MATCH_ROBOTS = ((1, 0), (6, 0), (11, 1), (20, 1))        # (robot, kk) of the do_match cases


@pytest.fixture(scope="module")
def scene(liw, synth):
    return sc.laser_scene(liw, synth)


@pytest.fixture(scope="module")
def env(scene, pyoracle):
    return scene["lp"], pyoracle.LaserOracle(scene["lp"])


# ---------------------------------------------------------------------------------------------------------------- the laser set
def test_laser_set_has_the_properties_the_guards_rely_on(liw, synth, scene):
    lp, off = scene["lp"], liw.laser.office_laser_params()
    res = lp["laser_resolution"]
    for k in ("w_laser_each_scan", "h_laser_each_scan"):
        assert 0.25 <= (lp[k] / res) % 1.0 <= 0.75, k                  # (int)(x / res + 1) rests on no rounding
    w, h = int(lp["w_laser_each_scan"] / res + 1), int(lp["h_laser_each_scan"] / res + 1)
    assert (w, h) == (sc.LASER_W, sc.LASER_H) and w != h and (w % 2) != (h % 2)
    scalars = [lp[k] for k in sc.LASER]
    assert len(set(scalars)) == len(scalars) and all(lp[k] != off[k] for k in sc.LASER)
    assert lp["ref_n_accumulation"] % 2 == 1 and lp["ref_n_accumulation"] >= 5
    narrower = 0
    for seed in sc.ROOMS:                                              # rooms: (9 +- 1) m x (7 +- 1) m
        segs = np.array(liw.laser.room_segments(seed)[:4])
        W, H = np.ptp(segs[:, :, 0]), np.ptp(segs[:, :, 1])
        assert lp["w_laser_each_scan"] > max(W, H)
        narrower += lp["h_laser_each_scan"] < min(W, H)
    assert narrower >= 3                                               # rooms are (7 +- 1) m deep; the arms test counts what falls outside
    assert lp["T_imu_to_laser"] == list(scene["prm"]["T_imu_to_laser"]) != list(off["T_imu_to_laser"])
    print("walks drawn per robot until the floors were met:", scene["tries"])


# ---------------------------------------------------------------------------------------------------------------- host against oracle
def _same_cells(s, so, pts):
    n = 0
    for x, y, _z in pts:
        ka, ia = s.cell_lines(x, y, 64)
        kb, ib = so.cell_lines(x, y, 64)
        assert ka == kb and np.array_equal(ia, ib), (x, y, ka, kb)
        n += 1
    return n


@pytest.mark.parametrize("b", ROOM_ROBOTS + ("low edge",))
def test_spawn_matches_oracle(liw, scene, env, b):
    lp, orc = env
    pts = scene["low_edge"] if b == "low edge" else scene["points"][b][0]
    s, so = liw.laser.Scan.spawn(lp, pts, 1.0), orc.spawn_scan(pts, 1.0)
    la, lb = s.lines(), so.lines()
    assert la.shape[0] >= (1 if b == "low edge" else sc.MIN_LINES)
    same_lines(la, lb)
    ca, cb = s.concers(), so.concers()
    assert ca.shape == cb.shape and (ca.shape[0] == 0 or np.abs(ca - cb).max() <= 1e-9)
    cells = _same_cells(s, so, pts)                                    # the grid under every scan point, inside the grid or not
    print("spawn %s: %d lines, %d corners, %d cells equal" % (b, la.shape[0], ca.shape[0], cells))
    assert np.all(la[:, 9] >= lp["line_min_len"])


def test_segment_rasterisation_matches_oracle(liw, scene, env):
    lp, orc = env
    s, so = liw.laser.Scan.empty(lp), orc.empty_scan()
    rng = np.random.default_rng(5)
    on, registered = [], 0
    for _ in range(60):
        a = np.append(rng.uniform(-7, 7, 2), 0.0)                      # the grid is +-5.5 m x +-3.3 m: many segments leave it
        b = a + np.append(rng.uniform(-2, 2, 2), 0.0) * rng.choice([0.01, 1.0])
        got = s.add_segment(a, b, False)
        assert got == so.add_segment(a, b, False)                      # 0 also for an accepted segment that touches no valid cell
        registered += got
        on += [a[:2] + t * (b[:2] - a[:2]) for t in (0.0, 0.25, 0.5, 0.75, 1.0)]
    same_lines(s.lines(), so.lines())
    assert registered == s.lines().shape[0]
    probes = np.concatenate([rng.uniform(-7.5, 7.5, (1200, 2)), np.array(on)])   # anywhere, and on the segments
    gx, gy, w, h = sc.grid_coordinates(lp, probes)
    inside = (gx > -1) & (gx < w) & (gy > -1) & (gy < h)
    hit = 0
    for (x, y), ok in zip(probes, inside):
        ka, ia = s.cell_lines(x, y, 64)
        kb, ib = so.cell_lines(x, y, 64)
        assert ka == kb and np.array_equal(ia, ib)
        assert (ka >= 0) == bool(ok)
        hit += ka > 0
    print("rasterisation: %d lines, probes %d inside / %d outside the grid, %d on a line" % (s.lines().shape[0], inside.sum(), (~inside).sum(), hit))
    assert inside.sum() > 200 and (~inside).sum() > 200 and hit > 20


@pytest.mark.parametrize("b,kk", MATCH_ROBOTS)
def test_do_match_matches_oracle(liw, scene, env, b, kk):
    lp, orc = env
    (p1, p2), (pts1, pts2) = scene["poses"][b, :2], scene["points"][b][:2]
    s1, s2 = liw.laser.Scan.spawn(lp, pts1), liw.laser.Scan.spawn(lp, pts2)
    o1, o2 = orc.spawn_scan(pts1), orc.spawn_scan(pts2)
    p2g = p2 + sc.MATCH_GUESS
    m = liw.laser.do_match(lp, s1, s2, p1[:3], p1[3:], p2g[:3], p2g[3:], kk)
    mo = orc.do_match(o1, o2, p1[:3], p1[3:], p2g[:3], p2g[3:], kk)
    print("do_match robot %d kk %d: %d pairs" % (b, kk, len(m)))
    assert len(m) == len(mo) and len(m) >= sc.MIN_BACK_MATCHES
    assert np.array_equal(m.idx1, mo.idx1) and np.array_equal(m.idx2, mo.idx2)
    assert np.abs(m.pts - mo.pts).max() <= 1e-9 and np.array_equal(m.pose, mo.pose)


def test_manager_sequence_matches_oracle(liw, scene, pyoracle):
    """16 add_scans of robot 0 at ref_n_accumulation = 5: the first reference, a spawning sub-map at count 2, hand-overs at count 5 and
    then every third kept scan; frame F_SMALL_P is dropped by the motion filter, frame F_SMALL_Q is kept.  The hand-overs happen in
    the frames a numpy restatement of the state machine names."""
    from test_gpu_laser_add_scan_wave import _host_machine
    lb = liw.laser_batch
    lp = scene["lp"]
    orc, mgr = pyoracle.LaserOracle(lp), liw.laser.LaserManager(lp)
    flags, _, margin = _host_machine(lb, scene["poses"][0], lp["ref_n_accumulation"], lp["ref_motion_filter_p"], lp["ref_motion_filter_q"])
    ref_poses, ref_lines, offered, registered = [], [], 0, 0
    for k in range(sc.FRAMES):
        pose, pts = scene["poses"][0, k], scene["points"][0][k]
        p, q = pose[:3], pose[3:]
        s, o = liw.laser.Scan.spawn(lp, pts, float(k)), orc.spawn_scan(pts, float(k))
        for fn in ("match_with_front", "match_with_back", "match_with_ref"):
            m, mo = getattr(mgr, fn)(s, p, q), getattr(orc, fn)(o, p, q)
            assert len(m) == len(mo), (k, fn)
            assert np.array_equal(m.idx1, mo.idx1) and np.array_equal(m.idx2, mo.idx2), (k, fn)
            assert len(m) == 0 or np.abs(m.pts - mo.pts).max() <= 1e-9
            assert np.array_equal(m.pose, mo.pose)
            assert k == 0 or fn != "match_with_back" or len(m) >= sc.MIN_BACK_MATCHES
        mgr.add_scan(s, p, q)
        orc.add_scan(o, p, q)
        assert mgr.num_keyframes() == orc.num_keyframes() == k + 1
        ra, rb = mgr.ref_scan(), orc.ref_scan()
        assert ra is not None and rb is not None, k
        same_lines(ra[0].lines(), rb[0].lines())
        assert np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
        _same_cells(ra[0], rb[0], pts[::5])
        ref_poses.append(ra[1].tobytes() + ra[2].tobytes())
        ref_lines.append(ra[0].lines())
        if k and flags[k] == lb.ADD_ADDED:                             # accumulated into the same reference: what it offered, what registered
            offered += s.lines().shape[0]
            registered += ref_lines[-1].shape[0] - ref_lines[-2].shape[0]
    swapped = [k for k in range(1, sc.FRAMES) if ref_poses[k] != ref_poses[k - 1]]
    print("manager: %d of %d scans kept, reference handed over in frames %s; %d of the %d lines offered to a standing reference registered "
          "(the others lie outside the sub-map's grid)"
          % (sum(f != 0 for f in flags), sc.FRAMES, swapped, registered, offered))
    assert swapped == [k for k in range(sc.FRAMES) if flags[k] & lb.ADD_SWAPPED] and len(swapped) >= 3
    assert flags[sc.F_SMALL_P] == 0 and flags[sc.F_SMALL_Q] & lb.ADD_ADDED and margin > SCALE
    k = sc.F_SMALL_P                                                   # dropped: the reference is what it was
    assert ref_poses[k] == ref_poses[k - 1] and np.array_equal(ref_lines[k], ref_lines[k - 1])
    assert 0 < registered < offered


# ---------------------------------------------------------------------------------------------------------------- arms
def test_arms_that_the_office_set_never_reaches_occur(liw, scene, env, pyoracle):
    lp, orc = env
    off = liw.laser.office_laser_params()
    n = dict(rows_only=0, cols_only=0, low_edge=0, low_edge_on_a_line=0, partly_outside=0, gaps_between=0, short_lines=0)
    robots = dict(rows_only=set(), cols_only=set(), low_edge=set(), partly_outside=set())
    lax = pyoracle.LaserOracle(dict(lp, line_min_len=off["line_min_len"]))
    for b in range(B):
        pts = scene["points"][b][0]
        gx, gy, w, h = sc.grid_coordinates(lp, pts)
        in_c, in_r = (gx > -1) & (gx < w), (gy > -1) & (gy < h)          # truncation toward zero: (-1, 0) lands in cell 0
        low = ((gx > -1) & (gx < 0) & in_r) | ((gy > -1) & (gy < 0) & in_c)
        s = liw.laser.Scan.spawn(lp, pts)
        for x, y, _z in pts[low]:
            k, _ = s.cell_lines(x, y, 64)
            assert k >= 0                                                # a valid cell
            n["low_edge_on_a_line"] += k > 0
        for key, mask in (("rows_only", in_c & ~in_r), ("cols_only", in_r & ~in_c), ("low_edge", low)):
            n[key] += int(mask.sum())
            if mask.any():
                robots[key].add(b)
        la = s.lines()
        ends = []
        for e in (0, 3):
            ex, ey, _, _ = sc.grid_coordinates(lp, la[:, e:e + 3])
            ends.append((ex > -1) & (ex < w) & (ey > -1) & (ey < h))
        part = int((ends[0] != ends[1]).sum())
        n["partly_outside"] += part
        if part:
            robots["partly_outside"].add(b)
        gaps = np.linalg.norm(np.diff(pts, axis=0), axis=1)
        n["gaps_between"] += int(((gaps > off["line_continuous_threshold"]) & (gaps <= lp["line_continuous_threshold"])).sum())
        ll = lax.spawn_scan(pts).lines()
        n["short_lines"] += int(((ll[:, 9] >= off["line_min_len"]) & (ll[:, 9] < lp["line_min_len"])).sum())
    print("arms over the %d spawn scans: %s; robots %s" % (B, n, {k: sorted(v) for k, v in robots.items()}))
    assert n["rows_only"] >= 100 and n["cols_only"] >= 10 and n["low_edge"] >= 10 and n["low_edge_on_a_line"] >= 1
    assert n["partly_outside"] >= 5
    assert n["gaps_between"] >= 5      # runs the second value joins and the office value would have split
    assert n["short_lines"] >= 1       # lines the office line_min_len accepts and this one rejects
    gx, gy, w, h = sc.grid_coordinates(lp, scene["low_edge"])
    assert np.all((gx > -1) & (gx < 0) & (gy > 0) & (gy < h))          # the hand-placed wall: every point in column 0 through (-1, 0)
    s = liw.laser.Scan.spawn(lp, scene["low_edge"])
    assert all(s.cell_lines(x, y, 64)[0] >= 1 for x, y, _ in scene["low_edge"])


# ---------------------------------------------------------------------------------------------------------------- mutations, margins
def oracle_outputs(pyoracle, scene, lp):
    """every discrete output of the oracle on the inputs of tests/test_gpu_laser_second_config.py: per robot the line count of each
    scan, the cell under every second point of the spawn scan, the index lists of do_match (frame 0 against frame 1, kk 0 and 1)
    and of match_with_ref in every frame, and the reference sub-map after every add_scan (pose bytes, line count)"""
    out = dict(lines=[], cells=[], match=[], ref_match=[], ref=[])
    for b in range(B):
        orc = pyoracle.LaserOracle(lp)
        poses, scans = scene["poses"][b], [orc.spawn_scan(p) for p in scene["points"][b]]
        out["lines"].append(tuple(s.lines().shape[0] for s in scans))
        cells = []
        for x, y, _z in scene["points"][b][0][::2]:
            k, ids = scans[0].cell_lines(x, y, 16)
            cells.append((k,) + tuple(ids))
        out["cells"].append(tuple(cells))
        for kk in (0, 1):
            for p2 in (poses[1], poses[1] + sc.MATCH_GUESS):          # test_match's guess, and the exact pose of the back matches
                m = orc.do_match(scans[0], scans[1], poses[0, :3], poses[0, 3:], p2[:3], p2[3:], kk)
                out["match"].append((tuple(m.idx1), tuple(m.idx2)))
        for k in range(sc.FRAMES):
            m = orc.match_with_ref(scans[k], poses[k, :3], poses[k, 3:])
            out["ref_match"].append((tuple(m.idx1), tuple(m.idx2)))
            orc.add_scan(scans[k], poses[k, :3], poses[k, 3:])
            r = orc.ref_scan()
            out["ref"].append(None if r is None else (r[1].tobytes(), r[2].tobytes(), r[0].lines().shape[0]))
    return out


def moved(a, b):
    """per kind of output: how many entries differ (cells: per probed cell)"""
    d = {k: sum(x != y for x, y in zip(a[k], b[k])) for k in ("match", "ref_match", "ref")}
    d["lines"] = sum(x != y for ra, rb in zip(a["lines"], b["lines"]) for x, y in zip(ra, rb))
    d["cells"] = sum(x != y for ra, rb in zip(a["cells"], b["cells"]) for x, y in zip(ra, rb))
    return d


@pytest.fixture(scope="module")
def base_outputs(pyoracle, scene):
    return oracle_outputs(pyoracle, scene, scene["lp"])


# what each single mistake must move, and by how much at the least: (kind of output, entries).  There are 24 x 16 = 384 scans and
# reference sub-maps, 96 do_match lists and 11 690 probed cells.  A floor is what the mistake must reach by its nature (one entry per robot,
# a quarter of the frames, a hundred cells a scan), far below what it does reach (docs/WIDENING.md).
MUTATION_FLOORS = {
    "w and h exchanged": ("cells", 2400),                 # rows beyond +-3.3 m become valid, columns beyond it invalid: > 100 a scan
    "motion filters exchanged": ("ref", 24),              # every robot has a frame that each order of the two thresholds treats differently
    "ref_n_accumulation = 4": ("ref", 96),                # another hand-over cycle from the fourth kept scan on
    "laser rotation transposed": ("ref_match", 96),
    "office line_min_len": ("lines", 20),
    "office line_max_dis": ("lines", 5),                  # 0.03 against 0.021: only fits with a worst point between the two differ
    "office line_continuous_threshold": ("lines", 5),     # 0.1 against 0.14: only gaps between the two differ (the arms test counts them)
    "office line_max_tolerance_angle": ("lines", 20),
}


@pytest.mark.parametrize("name", sorted(MUTATION_FLOORS))
def test_single_mistakes_move_the_oracle(liw, pyoracle, scene, base_outputs, name):
    kind, floor = MUTATION_FLOORS[name]
    lpm = sc.laser_mutations(liw, scene["lp"])[name]
    d = moved(base_outputs, oracle_outputs(pyoracle, scene, lpm))
    print("%s: entries moved %s (asserted: %s >= %d)" % (name, d, kind, floor))
    assert d[kind] >= floor


def test_mutation_list_is_the_one_of_the_guards(liw, scene):
    assert set(sc.laser_mutations(liw, scene["lp"])) == set(MUTATION_FLOORS)


@pytest.mark.parametrize("key", sc.LASER_THRESHOLDS)
def test_no_decision_sits_on_a_threshold(pyoracle, scene, base_outputs, key):
    lp = scene["lp"]
    for f in (1.0 - SCALE, 1.0 + SCALE):
        lpm = dict(lp, **{key: lp[key] * f})
        res = lpm["laser_resolution"]
        assert (int(lpm["w_laser_each_scan"] / res + 1), int(lpm["h_laser_each_scan"] / res + 1)) == (sc.LASER_W, sc.LASER_H)   # w and h held
        d = moved(base_outputs, oracle_outputs(pyoracle, scene, lpm))
        assert not any(d.values()), (key, f, d)


# ---------------------------------------------------------------------------------------------------------------- loop detector
def _walk(p, feats, stride=2):
    """loop_reference over the ordered pairs the GPU test compares -> (results per pair, margins, best sizes, quick counts)"""
    fs = [ref.Feature(ref.dedup([F.tolist()], p["d_res"]), np.eye(4), p, 64) for F in feats]
    ref.QUICK_COUNTS.clear()
    margins, out, sizes = [], {}, set()
    for q in range(len(fs)):
        for c in range(len(fs)):
            if q == c or (q + c) % stride:
                continue
            m = ref.match_map(fs[q], fs[c], q, c, p, margins)
            out[(q, c)] = (m["gate"], m["size"], m["row"], m["query_row"], m["bin"], tuple(m["p1"]), tuple(m["p2"]))
            if m["gate"] in (0, 4):
                sizes.add(m["size"])
    return out, margins, sizes, set(ref.QUICK_COUNTS)


@pytest.mark.parametrize("cfg,thr,stride", [("fine", 5, 2), ("fine", 7, 2), ("coarse", 5, 2), ("coarse", 7, 2), ("edge", 5, 3)])
def test_match_cases_discriminate_at_the_loop_sets(cfg, thr, stride):
    p, feats = tgl.match_case(cfg, thr)
    out, margins, sizes, quick = _walk(p, feats, stride)
    accepted = sum(v[0] == 0 for v in out.values())
    swapped = dict(p, a_res=p["d_res"], d_res=p["a_res"])
    alt, _, _, _ = _walk(swapped, feats, stride)
    changed = sum(out[k] != alt[k] for k in out)
    print("%s set, threshold %d: %d pairs, %d accepted, smallest bin margin %.3e, a_res <-> d_res changes %d pairs"
          % (cfg, thr, len(out), accepted, min(margins), changed))
    assert min(margins) > MARGIN
    assert thr in sizes and thr + 1 in sizes and thr - 1 in quick and thr in quick
    if cfg != "edge":
        assert accepted > 100
        assert changed > 0.1 * len(out)
    else:
        assert len(out) > 300 and accepted > 20


def test_loop_sizes_at_the_three_sets(liw):
    want = dict(fine=(79, 253), coarse=(15, 91), edge=(79, 255))
    for cfg, wn in want.items():
        p = sc.loop_params(cfg)
        assert liw.loop.sizes(p) == ref.sizes(p) == wn, cfg
    assert len({sc.LOOP_SETS["fine"][k] for k in ("a_res", "d_res", "max_dis", "max_tf_p", "max_tf_q")}) == 5
    assert want["fine"][0] > 64 > want["coarse"][0]                   # more / fewer quick words than lanes
    with pytest.raises(ValueError):
        liw.loop.sizes(sc.loop_params("edge", a_res=2.0 * math.pi / 254.0))   # nAngle + 1 = 257 > kMaxBins
    with pytest.raises(ValueError):
        liw.loop.sizes(sc.loop_params("edge", a_res=2.0 * math.pi / 253.5))   # 255.5 + 1 > kMaxBins: check_params compares before truncating


@pytest.mark.parametrize("cfg", tgl.SECOND_SETS)
def test_detect_sequences_reach_between_the_gates(liw, cfg):
    res = cases.restatement(cfg)
    p = sc.loop_params(cfg)
    assert p["max_tf_q"] < p["max_tf_p"] < p["max_dis"]
    found = [[e is not None for e in r["edges"]] for r in res]
    assert not any(found[1]) and not any(found[7]) and all(any(found[r]) for r in (0, 2, 3, 4, 5, 6))
    assert res[0]["later_passes"] and all(e["index1"] >= 20 for e in res[0]["edges"] if e)
    accepted = [c for r in res for c in r["per_candidate"] if "tf_p" in c and c["tf_p"] <= p["max_tf_p"] and c["tf_q"] <= p["max_tf_q"]]
    dis_between = [c["dis"] for c in accepted if p["max_tf_p"] < c["dis"] < p["max_dis"]]
    tfp_between = [c["tf_p"] for c in accepted if p["max_tf_q"] < c["tf_p"] < p["max_tf_p"]]
    tfq_above = [c["tf_q"] for c in res[4]["per_candidate"] if c.get("tf_q", 0.0) > p["max_tf_q"]]
    print("%s set: %d edges; accepted candidates with max_tf_p < dis < max_dis: %d, with max_tf_q < tf_p < max_tf_p: %d; spin0 rejections: %d; "
          "smallest bin margin %.3e" % (cfg, sum(map(sum, found)), len(dis_between), len(tfp_between), len(tfq_above), min(r["min_margin"] for r in res)))
    assert sum(map(sum, found)) == 60 and len(accepted) == 60
    assert len(dis_between) >= 5 and len(tfp_between) >= 10 and len(tfq_above) >= 5
    assert any(found[4]) and all(e["index2"] != 0 for e in res[4]["edges"] if e)
    for r in res:
        assert [(k, v, t) for k, v, t in r["gates"] if k != "size" and abs(v - t) <= SCALE] == []
        assert r["min_margin"] > MARGIN
    dis = [(v, t) for r in res for k, v, t in r["gates"] if k == "dis"]
    sz = [(v, t) for r in res for k, v, t in r["gates"] if k == "size"]
    assert any(v > t for v, t in dis) and any(v <= t for v, t in dis) and any(v > t for v, t in sz) and any(v <= t for v, t in sz)
    # T_imu_to_wheel transposed in the restatement alone: the edges move
    Tiw = cases.T_imu_to_wheel(cfg)
    Tt = Tiw.copy()
    Tt[:3, :3] = Tiw[:3, :3].T
    alt = cases.restatement(cfg, tuple(Tt.reshape(16)))
    move = [float(np.abs(a["tf12"] - b["tf12"]).max()) for ra, rb in zip(res, alt) for a, b in zip(ra["edges"], rb["edges"]) if a is not None and b is not None]
    lost = sum((a is None) != (b is None) for ra, rb in zip(res, alt) for a, b in zip(ra["edges"], rb["edges"]))
    print("%s set, T_imu_to_wheel transposed: tf12 moves by up to %.3e over %d common edges, %d decisions change" % (cfg, max(move, default=0.0), len(move), lost))
    assert lost > 0 or max(move) > 1e-6


def test_second_set_detectors_get_a_generic_wheel_extrinsic(liw, synth):
    R = cases.T_imu_to_wheel("fine")[:3, :3]
    assert np.abs(R).min() >= 0.1 and np.abs(R).max() <= 0.97 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-6
    assert np.array_equal(cases.T_imu_to_wheel("fine"), sc.held_extrinsic(liw, sc.skewed_params(synth), "T_imu_to_wheel"))
    assert not np.array_equal(cases.T_imu_to_wheel("fine"), cases.T_imu_to_wheel())


# ---------------------------------------------------------------------------------------------------------------- map extrinsic
def _known(r):
    """known cells of a map_reference.render result -> dict (world cell) -> value"""
    g = r["grid"]
    ox, oy = int(round(r["origin_x"] / r["resolution"])), int(round(r["origin_y"] / r["resolution"]))
    ys, xs = np.nonzero(g != -1)
    return {(ox + int(x), oy + int(y)): int(g[y, x]) for y, x in zip(ys, xs)}


def test_map_case_exposes_a_transposed_laser_rotation(liw, synth):
    import test_gpu_map as tgm
    prm = sc.skewed_params(synth)
    subs, poses = tgm._poses_case()
    Til = mc.til12(liw, prm)
    Tt = Til.copy()
    Tt[:9] = Til[:9].reshape(3, 3).T.reshape(9)
    base = map_reference.render(mc.host_tf(liw, poses, Til), subs, 0.05)
    alt = map_reference.render(mc.host_tf(liw, poses, Tt), subs, 0.05)
    a, b = _known(base), _known(alt)
    diff = sum(b.get(k) != v for k, v in a.items())
    print("map: %d known cells, %d differ with the laser rotation transposed (%.1f %%)" % (len(a), diff, 100.0 * diff / len(a)))
    assert diff > 0.01 * len(a)
    off = mc.til12(liw, synth.office_params())
    assert np.abs(Til - off).max() > 0.1
