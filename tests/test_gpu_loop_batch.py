"""The fleet's key-frame sink and loop detector on the MI355X (include/liw_loop_batch.h) against one single-robot LoopDetector per
robot fed the same key frames: features bit-identical, every detection decision, edge and statistic equal in every robot-frame,
capacity, determinism and tiling at 512 robots, the detector behind a free-running FleetTracker, and the LIW_EINVAL cases."""
import ctypes as C

import numpy as np
import pytest

import loop_batch_cases as cases
import test_gpu_loop as tgl

pytestmark = pytest.mark.gpu
GUARD = 256
TF_BAR = 1e-9      # the bar of the single detector's own detect tests: host libm against liw_crmath, pose -> tf12


def _fleet(liw, synth, p, B, K, P, Cc, guard=0, cfg="office"):
    return liw.FleetLoopDetector(tgl._set_prm(synth, cfg), p, dict(B=B, max_keyframes=K, max_points=P, max_kf_corners=Cc), guard=guard)


def _single(liw, synth, p, K, P, cfg="office"):
    return liw.loop.LoopDetector(tgl._set_prm(synth, cfg), p, dict(max_keyframes=K, max_points=P))


def _upload(torch, B, stride, items):
    """items: per robot None or (pose6, corners [n][3]) -> dict(key, pose, acc, n_acc) as FleetTracker.step returns them"""
    key, pose, acc, n = np.zeros(B, np.uint8), np.zeros((B, 6)), np.zeros((B, stride, 3)), np.zeros(B, np.int32)
    for b, it in enumerate(items):
        if it is None:
            continue
        key[b], pose[b] = 1, it[0]
        c = np.asarray(it[1], dtype=np.float64).reshape(-1, 3)
        n[b] = len(c)
        acc[b, :len(c)] = c
    return {k: torch.from_numpy(v).cuda() for k, v in dict(key=key, pose=pose, acc=acc, n_acc=n).items()}


def _same_feature(liw, fl, b, det, k):
    """key frame k of robot b against key frame k of its detector: state, n_points, origin, points, every row; -> rows compared"""
    st, sd = fl.status(b, k), det.status(k)
    assert st["state"] == sd["state"] and st["n_points"] == sd["n_points"], (b, k, st, sd)
    assert np.array_equal(st["origin"], sd["origin"]), (b, k)
    if st["state"] == liw.loop.OVER_CAP:
        return 0
    pts = fl.get_points(b, k)
    assert pts.tobytes() == det.get_points(k).tobytes(), (b, k)
    if st["state"] != liw.loop.VALID:
        return 0
    for i in range(len(pts)):
        g, w = fl.get_row(b, k, i), det.get_row(k, i)
        assert np.array_equal(g["dij"], w["dij"]) and np.array_equal(g["j"], w["j"]) and np.array_equal(g["quick"], w["quick"]), (b, k, i)
        assert g["aij"].tobytes() == w["aij"].tobytes(), (b, k, i)     # same device acos, same operations
    return len(pts)


# --------------------------------------------------------------------------------------------------------------------- 1
def test_features_bit_identical(liw, synth):
    """Measured on an MI355X: 1 629 descriptor rows of 53 key frames, every byte equal."""
    _check_features_bit_identical(liw, synth, "office")


@pytest.mark.parametrize("cfg", tgl.SECOND_SETS)
def test_features_bit_identical_second_sets(liw, synth, cfg):
    """k_floop_gather's near = d_res / 2 and far = 5 d_res and the shared descriptor body at a_res != d_res.  The hand-placed corners
    of the office case are scaled by d_res / 0.03 where their distances are what the case is about."""
    _check_features_bit_identical(liw, synth, cfg)


def _check_features_bit_identical(liw, synth, cfg):
    import torch
    rng = np.random.default_rng(101)
    B, F, K, P, Cc, stride = 6, 14, 16, 64, 40, 48
    p = tgl._set_params(cfg, submap_count=3)
    sc_ = p["d_res"] / 0.03                 # 1.0 at the office set
    fl = _fleet(liw, synth, p, B, K, P, Cc, guard=GUARD, cfg=cfg)
    dets = [_single(liw, synth, p, K, P, cfg=cfg) for _ in range(B)]
    L = tgl._landmarks(rng)
    keyed = [lambda t: True, lambda t: t % 2 == 0, lambda t: t % 3 != 0, lambda t: t >= 2, lambda t: t not in (1, 5, 6), lambda t: False]
    count = [0] * B
    over_corner_kf, states_seen, rows, inputs0 = set(), set(), 0, []

    def corners_of(b, t, j):
        """corners of robot b's key frame j (given in frame t)"""
        T = tgl._pose(0.1 * t + b, 0.05 * t, 0.02 * t)
        Cn = tgl._seen(L, T, r=2.5)
        if b == 0:      # blends (inside d_res / 2), duplicates (inside 5 d_res), z that is blended too; later key frames see the same landmarks
            Cn = np.concatenate([Cn, Cn[:5] + [0.004, -0.003, 0.01 * j], Cn[5:9] + [0.06, 0.05, 0.0]])
        if b == 1 and j in (1, 4):
            Cn = np.zeros((0, 3))                                            # a key frame with no corners
        if b == 2:      # exact sizes: sub-map of key frames 4, 5, 6 has 22 + 22 + 21 = max_points + 1 points
            n = 22 if j in (4, 5) else (21 if j == 6 else 10)
            Cn = np.stack([np.arange(n) * 1.0 + 100.0, np.full(n, 1.0 * j), np.zeros(n)], axis=1)
        if b == 3 and j == 3:
            Cn = np.concatenate([Cn, [[40000.0 * sc_, 0.0, 0.0]]])           # dij = 1 333 333 >= 2^20 - 1
        if b == 4 and j == 2:
            Cn = np.concatenate([Cn, np.stack([np.arange(Cc + 1 - len(Cn)) * 1.0 + 50.0, np.full(Cc + 1 - len(Cn), -30.0), np.zeros(Cc + 1 - len(Cn))], axis=1)])
            assert len(Cn) == Cc + 1                                         # one key frame over max_kf_corners
        assert len(Cn) <= stride
        return T, Cn

    for t in range(F):
        items = []
        for b in range(B):
            if not keyed[b](t):
                items.append(None)
                continue
            T, Cn = corners_of(b, t, count[b])
            pose = np.array([T[0, 3], T[1, 3], 0.0, 0.0, 0.0, 0.02 * t])
            items.append((pose, Cn))
        snap = fl.robot_regions().clone()
        inp = _upload(torch, B, stride, items)
        fl.add_keyframes(inp["key"], inp["pose"], inp["acc"], inp["n_acc"])
        torch.cuda.synchronize()
        regions = fl.robot_regions()
        for b, it in enumerate(items):
            if it is None:
                assert torch.equal(regions[b], snap[b]), (t, b)              # key clear: no byte of the robot changes
                continue
            k = dets[b].add_keyframe(cases.make_tf(it[0]), it[1])
            assert k == count[b] and fl.num_keyframes(b) == k + 1
            count[b] += 1
            if b == 0:
                inputs0.append(it[1])
            if b == 4 and 2 <= k <= 4:                                       # every sub-map that contains key frame 2
                st = fl.status(b, k)
                assert st["state"] == liw.loop_batch.OVER_CORNERS and st["n_points"] == 0
                over_corner_kf.add(k)
                continue
            rows += _same_feature(liw, fl, b, dets[b], k)
            states_seen.add((b, fl.status(b, k)["state"]))
    # the candidate slots (k % 2 == 0) keep their features while later key frames come in
    for b in range(B):
        assert fl.num_keyframes(b) == count[b] == dets[b].num_keyframes() if count[b] else fl.num_keyframes(b) == 0
        for k in range(0, count[b], 2):
            if not (b == 4 and 2 <= k <= 4):
                rows += _same_feature(liw, fl, b, dets[b], k)
    assert count[5] == 0 and len(set(count)) >= 5
    assert over_corner_kf == {2, 3, 4}
    assert (2, liw.loop.OVER_CAP) in states_seen and fl.status(2, 6)["n_points"] == P + 1
    assert {k for k in range(count[3]) if fl.status(3, k)["state"] == liw.loop.DIJ_OVERFLOW} == {3, 4, 5}
    assert fl.status(1, 1)["n_points"] > 0 and dets[1].status(1)["n_points"] == fl.status(1, 1)["n_points"]
    # blended points exist: kept points of robot 0's newest sub-map that are no input corner
    flat = np.concatenate(inputs0)
    assert sum(1 for q in fl.get_points(0, count[0] - 1) if not (flat == q).all(axis=1).any()) >= 5
    assert rows > 1000
    buf = fl._buf
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())
    assert not bool(fl.full().any())
    print("features at the %s set: %d rows of %d key frames bit-identical (keys, j, aij, quick_des, points, origins)" % (cfg, rows, sum(count)))
    fl.close()


@pytest.mark.parametrize("n", tgl.DESCRIBE_EDGE_N)
def test_features_bit_identical_at_sort_and_lane_edges(liw, synth, n):
    """Sub-maps of n points, where the shared descriptor body's sort padding and lane strides change (tgl.DESCRIBE_EDGE_N), for two
    robots against the single detector: every byte of keys, aij and quick_des.  With max_points = 130 the describe grid has 128
    blocks per robot, so at n = 129 one wave also runs a second point in the same LDS."""
    _check_features_at_edges(liw, synth, n, "office")


@pytest.mark.parametrize("cfg", tgl.SECOND_SETS)
@pytest.mark.parametrize("n", tgl.DESCRIBE_EDGE_N)
def test_features_bit_identical_at_sort_and_lane_edges_second_sets(liw, synth, n, cfg):
    _check_features_at_edges(liw, synth, n, cfg)


def _check_features_at_edges(liw, synth, n, cfg):
    import torch
    C_, _ = tgl.describe_edge_case(n, cfg)
    B, P = 2, tgl.DESCRIBE_EDGE_CAP
    p = tgl._set_params(cfg)
    fl, det = _fleet(liw, synth, p, B, 2, P, P, guard=GUARD, cfg=cfg), _single(liw, synth, p, 2, P, cfg=cfg)
    inp = _upload(torch, B, P, [(np.zeros(6), C_)] * B)
    assert fl.add_keyframes(inp["key"], inp["pose"], inp["acc"], inp["n_acc"]).tolist() == [1] * B
    assert det.add_keyframe(cases.make_tf(np.zeros(6)), C_) == 0
    for b in range(B):
        assert _same_feature(liw, fl, b, det, 0) == n
    buf = fl._buf
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())
    fl.close()


# --------------------------------------------------------------------------------------------------------------------- 2
def _frame_items(robots, t, cfg="office"):
    seqs = cases.sequences(cfg)
    items = []
    for r in robots:
        off = cases.robots(cfg)[r][4]
        if off <= t < off + cases.KEYFRAMES:
            pose, _, Cn = seqs[r][t - off]
            items.append((pose, Cn))
        else:
            items.append(None)
    return items


def _stats_row(d):
    return [d[k] for k in ("candidates", "launched", "tasks", "quick_pass", "accepted", "icp_checked")]


def test_detection_equals_the_single_detectors(liw, synth):
    """Measured on an MI355X: 320 robot-frames, 60 edges, index pair, size and stats equal, tf12 max difference 3.9e-16 (bar 1e-9)."""
    _check_detection(liw, synth, "office")


@pytest.mark.parametrize("cfg", tgl.SECOND_SETS)
def test_detection_equals_the_single_detectors_second_sets(liw, synth, cfg):
    """the sequences of loop_batch_cases.ROBOTS_SECOND with detectors created from skewed_params: a generic T_imu_to_wheel through the
    Tiw, inv_iw conjugation of the tf gate, max_dis != max_tf_p with gate values between the two, a_res != d_res"""
    _check_detection(liw, synth, cfg)


def _check_detection(liw, synth, cfg):
    import torch
    res = cases.restatement(cfg)
    for r in res:
        assert cases.near_threshold(r["gates"]) == []       # no decision within 1e-6 relative of its threshold
    worst, edges, compared = 0.0, 0, 0
    for S, robots in cases.SETS.items():
        p, P = cases.params(S, cfg), cases.MAX_POINTS[S]
        B, K, stride = len(robots), 32, 256
        fl = _fleet(liw, synth, p, B, K, P, stride, cfg=cfg)
        dets = [_single(liw, synth, p, K, P, cfg=cfg) for _ in robots]
        first_detect = set()
        for t in range(cases.FRAMES):
            items = _frame_items(robots, t, cfg)
            out = fl.push(_upload(torch, B, stride, items))
            found, edge, tf12, stats = [out[k].cpu().numpy() for k in ("found", "edge", "tf12", "stats")]
            for b, it in enumerate(items):
                compared += 1
                if it is None:
                    assert found[b] == 0, (S, t, b)
                    continue
                r, kf = robots[b], t - cases.robots(cfg)[robots[b]][4]
                assert dets[b].add_keyframe(cases.make_tf(it[0]), it[1]) == kf
                want = dets[b].detect()
                ws = dets[b].last_stats()
                assert stats[b].tolist() == _stats_row(ws), (S, t, b, stats[b], ws)
                if ws["candidates"] and r not in first_detect:
                    first_detect.add(r)
                    assert kf == p["min_interval"]                          # reached at fleet frame offset + min_interval
                host = res[r]["edges"][kf]
                assert bool(found[b]) == (want is not None) == (host is not None), (S, t, b)
                if want is None:
                    assert edge[b].tolist() == [-1, -1, 0]
                    continue
                assert edge[b].tolist() == [want["index1"], want["index2"], want["size"]] == [host["index1"], host["index2"], host["size"]]
                d = float(np.abs(liw.loop.tf12_to_mat(tf12[b]) - want["tf12"]).max())
                worst = max(worst, d, float(np.abs(want["tf12"] - host["tf12"]).max()))
                assert d <= TF_BAR, (S, t, b, d)
                edges += 1
        for b, r in enumerate(robots):
            assert fl.num_keyframes(b) == cases.KEYFRAMES
            assert [fl.status(b, k)["n_points"] for k in range(cases.KEYFRAMES)] == res[r]["n_points"]
        fl.close()
    assert compared == 8 * cases.FRAMES and edges >= 40
    print("detection at the %s set: %d robot-frames, %d edges equal (index1, index2, size, stats); tf12 max difference %.3e" % (cfg, compared, edges, worst))
    assert worst <= TF_BAR


# --------------------------------------------------------------------------------------------------------------------- 3
def test_capacity_full_flag(liw, synth):
    import torch
    p = cases.params(1, min_interval=2)
    B, K, P, stride = 3, 12, 128, 64
    fl = _fleet(liw, synth, p, B, K, P, stride)
    dets = [_single(liw, synth, p, K if b == 0 else 32, P) for b in range(B)]
    seqs = cases.sequences()
    src, n_in = [5, 6, 4], [0, 0, 0]
    after12 = frozen = None
    for t in range(15):
        items = []
        for b in range(B):
            if b == 0 or (t + b) % 2 == 0:
                pose, _, Cn = seqs[src[b]][n_in[b]]
                items.append((pose, Cn))
            else:
                items.append(None)
        out = fl.push(_upload(torch, B, stride, items))
        found, edge = out["found"].cpu().numpy(), out["edge"].cpu().numpy()
        full = fl.full().cpu().numpy()
        stored = [int(it is not None and not (b == 0 and n_in[0] >= K)) for b, it in enumerate(items)]
        assert fl.added.cpu().numpy().tolist() == stored, t          # add_keyframes' own report of what it stored
        for b, it in enumerate(items):
            if it is None:
                assert found[b] == 0
                continue
            n_in[b] += 1
            if b == 0 and n_in[0] > K:
                with pytest.raises(liw.LiwError) as ei:
                    dets[0].add_keyframe(cases.make_tf(it[0]), it[1])
                assert ei.value.code == -12
                assert full[0] and found[0] == 0 and fl.num_keyframes(0) == K
                continue
            dets[b].add_keyframe(cases.make_tf(it[0]), it[1])
            want = dets[b].detect()
            assert bool(found[b]) == (want is not None), (t, b)
            if want is not None:
                assert edge[b].tolist() == [want["index1"], want["index2"], want["size"]]
        assert full.tolist() == [n_in[0] > K, False, False], t
        region = fl.robot_regions()[0].clone()
        if n_in[0] == K:
            after12 = region
        elif n_in[0] == K + 1:       # the 13th: the flag, and nothing else
            diff = (region != after12).nonzero().flatten().cpu().numpy()
            assert len(diff) and set(diff.tolist()) <= {4, 5, 6, 7}
            frozen = region
        elif n_in[0] > K + 1:
            assert torch.equal(region, frozen)
    assert n_in[0] == 15 and fl.is_full(0) and not fl.is_full(1)
    for b in (1, 2):
        assert fl.num_keyframes(b) == dets[b].num_keyframes() == n_in[b]
        _same_feature(liw, fl, b, dets[b], n_in[b] - 1)
    fl.close()


# --------------------------------------------------------------------------------------------------------------------- 4
def test_determinism_and_tiling_512(liw, synth):
    import torch
    tiles = 64
    total_edges = 0
    for S, robots in cases.SETS.items():
        p, P = cases.params(S), cases.MAX_POINTS[S]
        n, K, stride = len(robots), 32, 256
        B = n * tiles                                                        # 256 per parameter set, 512 in all
        frames = []
        for t in range(cases.FRAMES):
            inp = _upload(torch, n, stride, _frame_items(robots, t))
            frames.append({k: v.repeat(*([tiles] + [1] * (v.dim() - 1))).contiguous() for k, v in inp.items()})   # robot b = sequence b mod n
        runs = []
        for _ in range(2):
            fl = _fleet(liw, synth, p, B, K, P, stride)
            outs = []
            for inp in frames:
                o = fl.push(inp)
                outs.append({k: v.clone() for k, v in o.items()})
            torch.cuda.synchronize()
            runs.append((fl, outs))
        (fa, oa), (fb, ob) = runs
        for t in range(cases.FRAMES):
            for k in ("found", "edge", "tf12", "stats"):
                assert torch.equal(oa[t][k], ob[t][k]), (S, t, k)            # run to run
                v = oa[t][k].view(tiles, n, -1)
                assert torch.equal(v, v[0:1].expand_as(v)), (S, t, k)        # robot b against robot b mod n
            total_edges += int(oa[t]["found"].sum())
        assert torch.equal(fa._buf, fb._buf)                                 # the whole store, scratch included
        reg = fa.robot_regions().view(tiles, n, -1)
        for i in range(1, tiles):
            assert torch.equal(reg[i], reg[0]), (S, i)
        # and the tiled fleet found what the eight-robot fleet finds
        want = sum(e is not None for r in robots for e in cases.restatement()[r]["edges"])
        assert sum(int(o["found"].sum()) for o in oa) == tiles * want
        fa.close()
        fb.close()
        del runs, fa, fb, oa, ob, reg
        torch.cuda.empty_cache()
    assert total_edges >= tiles * 40


# --------------------------------------------------------------------------------------------------------------------- 5
def test_behind_the_tracker(liw, synth):
    """FleetLoopDetector.push(step_out) behind a free-running FleetTracker (the scene of tests/test_gpu_laser_track.py, 16 robots,
    ref_n_accumulation = 4) against a host sink that reads key / pose / acc / n_acc back and drives one LoopDetector per robot."""
    import torch
    import test_gpu_laser_track as tlt
    prm = synth.office_params()
    lp = dict(liw.laser.office_laser_params(prm), ref_n_accumulation=4)
    tp = dict(liw.laser_batch.office_track_params(prm), key_frame_p_motion_threshold=0.1)   # 0.15 m a frame: every frame can be a key frame
    nb, F, B = 8, 6, 16
    hp = liw.HostPreint(prm)
    trajs = [synth.make_window(hp, prm, seed=7100 + j, n=F + 1, L=0) for j in range(nb)]
    truth = np.stack([np.asarray(t["truth_states"]).reshape(F + 1, 15) for t in trajs])
    ranges = np.stack([[tlt._cast(liw, synth, lp, 3000 + j, truth[j, k, 0:6], seed=j * 10 + k) for k in range(F + 1)] for j in range(nb)])
    sc = dict(prm=prm, lp=lp, tp=tp, nb=nb, F=F, trajs=trajs, truth=truth, ranges=ranges, times=np.stack([t["times"] for t in trajs]))
    rob = np.arange(B) % nb
    ft = tlt._fleet(liw, sc, B)
    tlt._seed(torch, sc, ft.fe, rob)
    ft.start(truth[rob, 0])
    p = tgl._params(min_interval=2, submap_count=3)
    K, P, Cc = 16, 256, 256
    fl = _fleet(liw, synth, p, B, K, P, Cc)
    dets = [_single(liw, synth, p, K, P) for _ in range(B)]
    nk, worst, edges, corners = [0] * B, 0.0, 0, 0
    for k in range(1, F + 1):
        r, st = tlt._frame(torch, sc, rob, k)
        o = ft.step(r, st, tlt._interval(torch, sc, rob, k))
        out = fl.push(o)
        key, pose, acc, n_acc = [o[x].cpu().numpy() for x in ("key", "pose", "acc", "n_acc")]
        found, edge, tf12 = [out[x].cpu().numpy() for x in ("found", "edge", "tf12")]
        assert int(n_acc.max()) <= Cc
        for b in range(B):
            if not key[b]:
                assert found[b] == 0
                continue
            dets[b].add_keyframe(cases.make_tf(pose[b]), acc[b, :n_acc[b]])
            nk[b] += 1
            corners += int(n_acc[b])
            want = dets[b].detect()
            assert bool(found[b]) == (want is not None), (k, b)
            if want is not None:
                assert edge[b].tolist() == [want["index1"], want["index2"], want["size"]]
                d = float(np.abs(liw.loop.tf12_to_mat(tf12[b]) - want["tf12"]).max())
                worst = max(worst, d)
                assert d <= TF_BAR
                edges += 1
    rows = 0
    for b in range(B):
        assert fl.num_keyframes(b) == nk[b] >= 3, (b, nk)
        for kf in sorted(set(range(0, nk[b], 2)) | {nk[b] - 1}):
            rows += _same_feature(liw, fl, b, dets[b], kf)
    assert corners > 0 and rows > 0
    print("behind the tracker: %d key frames of %d robots, %d corners, %d descriptor rows bit-identical, %d edges (tf12 max difference %.3e)"
          % (sum(nk), B, corners, rows, edges, worst))
    fl.close()
    ft.close()


# --------------------------------------------------------------------------------------------------------------------- 6
def test_einval_writes_nothing(liw, synth):
    import torch
    p = cases.params(1, min_interval=2)
    B, K, P, stride = 2, 8, 64, 64
    fl = _fleet(liw, synth, p, B, K, P, stride, guard=GUARD)
    seqs = cases.sequences()
    for k in range(3):
        fl.push(_upload(torch, B, stride, [(seqs[5][k][0], seqs[5][k][2]), (seqs[6][k][0], seqs[6][k][2])]))
    inp = _upload(torch, B, stride, [(seqs[5][3][0], seqs[5][3][2]), (seqs[6][3][0], seqs[6][3][2])])
    torch.cuda.synchronize()
    outs = dict(found=fl.found, edge=fl.edge, tf12=fl.tf12, stats=fl.stats, added=fl.added)
    snap = fl._buf.clone()
    osnap = {k: v.clone() for k, v in outs.items()}
    L, h = fl.L, fl.h
    vp = lambda t: C.c_void_p(t.data_ptr())
    st, key, pose, acc, n = vp(fl.store), vp(inp["key"]), vp(inp["pose"]), vp(inp["acc"]), vp(inp["n_acc"])
    odd, ad = C.c_void_p(fl.store.data_ptr() + 4), vp(fl.added)
    calls = [
        L.liw_floop_reset(h, None, None, None), L.liw_floop_reset(h, odd, None, None),
        L.liw_floop_add_keyframes(h, None, key, pose, acc, stride, n, None, ad, None),
        L.liw_floop_add_keyframes(h, odd, key, pose, acc, stride, n, None, ad, None),
        L.liw_floop_add_keyframes(h, st, None, pose, acc, stride, n, None, ad, None),
        L.liw_floop_add_keyframes(h, st, key, None, acc, stride, n, None, ad, None),
        L.liw_floop_add_keyframes(h, st, key, pose, None, stride, n, None, ad, None),
        L.liw_floop_add_keyframes(h, st, key, pose, acc, stride, None, None, ad, None),
        L.liw_floop_add_keyframes(h, st, key, pose, acc, 0, n, None, ad, None),
        L.liw_floop_add_keyframes(h, st, key, pose, acc, -3, n, None, ad, None),
    ]
    o = [vp(outs[k]) for k in ("found", "edge", "tf12", "stats")]
    calls += [L.liw_floop_detect(h, None, key, None, *o, None), L.liw_floop_detect(h, odd, key, None, *o, None),
              L.liw_floop_detect(h, st, None, None, *o, None)]
    for i in range(4):
        a = list(o)
        a[i] = None
        calls.append(L.liw_floop_detect(h, st, key, None, *a, None))
    calls += [L.liw_floop_num_keyframes(h, st, -1), L.liw_floop_num_keyframes(h, st, B), L.liw_floop_full(h, None, 0),
              L.liw_floop_status(h, st, 0, 3, None, None, None), L.liw_floop_status(h, st, 0, -1, None, None, None),
              L.liw_floop_get_points(h, st, 0, 7, 0, None), L.liw_floop_get_row(h, st, 0, 0, 9999, 0, None, None, None, None)]
    torch.cuda.synchronize()
    assert calls == [-22] * len(calls), calls
    assert torch.equal(fl._buf, snap)
    for k, v in outs.items():
        assert torch.equal(v, osnap[k]), k
    # and the detector still works: the fourth key frame goes in
    fl.push(inp)
    assert fl.num_keyframes(0) == fl.num_keyframes(1) == 4
    assert bool((fl._buf[:GUARD] == 0xA5).all()) and bool((fl._buf[-GUARD:] == 0xA5).all())
    fl.close()
