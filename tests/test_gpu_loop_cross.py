"""Cross-robot loop detection and group alignment on the MI355X (include/liw_loop_cross.h) against the host restatement of
tests/loop_cross_cases.py: every decision, edge and statistic equal, tf12 / T_w1_w2 / rms within 1e-9 and T_w1_w2 within twice the
restatement's own deviation from the known truth W_a W_b^-1; the pair summaries and correspondence lists equal to the single
detector's match (the parent's kernels) where K_a = K_b + submap_count; T_w1_w2 and T_g_w bit-equal to liw_lie_mul of the device's
own inputs; the link rules including the double claim and the two-call chain; determinism and tiling; the store untouched; and the
pipeline FleetLoopDetector.push -> FleetGroupAligner.push -> FleetGroupMap.render_all end to end."""
import ctypes as C

import numpy as np
import pytest

import loop_cross_cases as xc
import map_batch_cases as mc
import map_group_cases as gc
import map_reference as mref
import test_gpu_loop as tgl
import test_gpu_loop_batch as tlb

pytestmark = pytest.mark.gpu
GUARD = 256
BAR = 1e-9         # the bar tests/test_gpu_loop_batch.py uses for tf12: host libm against liw_crmath
ULP_BAR = 4.0      # the group map's bar for a composed transform; 0 is expected


def _fed(liw, synth, name, tiles=1, guard=0):
    """a FleetLoopDetector holding the key frames of fleet `name`, `tiles` times over (robot b = robot b mod B of the cases)"""
    import torch
    F = xc.fleet(name)
    d = dict(F["dims"])
    n = d["B"]
    d["B"] = n * tiles
    fl = liw.FleetLoopDetector(synth.office_params(), F["params"], d, guard=guard)
    for t in range(max(F["K"])):
        items = [(F["frames"][r][t][0], F["frames"][r][t][2]) if t < F["K"][r] else None for r in range(n)]
        inp = tlb._upload(torch, n, 48, items)
        inp = {k: v.repeat(*([tiles] + [1] * (v.dim() - 1))).contiguous() for k, v in inp.items()}
        fl.add_keyframes(inp["key"], inp["pose"], inp["acc"], inp["n_acc"])
    return fl


def _aligner(liw, fl, name, group_of=None, anchors=(0, 4)):
    """anchors: robots of the eight (repeated in every tile), or a dict robot -> 4x4"""
    B = fl.B
    if group_of is None:
        group_of = (xc.GROUP_OF * (B // 8)) if B % 8 == 0 else [0] * B
    if not hasattr(anchors, "items"):
        anchors = [a + 8 * t for t in range(max(B // 8, 1)) for a in anchors if a + 8 * t < B]
    return liw.FleetGroupAligner(fl, group_of, anchors, xc.MIN_MATCH[name], xc.MAX_RMS)


def _calls(name):
    return {"long": xc.LONG_CALL} if name == "long" else xc.CALLS


def _sentinels(al):
    al.found.fill_(7); al.edge.fill_(-9); al.tf12.fill_(123.0); al.T_w1_w2.fill_(-55.0); al.rms.fill_(77.0); al.stats.fill_(-3)


def _lie(liw):
    L = liw.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def inv(A):
        A, out = np.ascontiguousarray(A, dtype=np.float64), np.zeros(12)
        L.liw_lie_inverse(pd(A), pd(out))
        return out
    return (lambda A, B: gc.lie_mul(liw, A, B)), inv


def _host(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


# --------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", xc.FLEETS)
def test_detect_equals_the_restatement(liw, synth, name):
    """Measured on an MI355X: 7 / 7 / 1 edges equal in found, edge and stats; tf12, T_w1_w2 and rms at most 8.9e-16 from the restatement
    (bar 1e-9); T_w1_w2 at most 7.0e-4 from the truth."""
    import torch
    fl = _fed(liw, synth, name, guard=GUARD)
    al = _aligner(liw, fl, name)
    mul, inv = _lie(liw)
    B = fl.B
    ones = torch.ones(B, dtype=torch.uint8, device="cuda")
    own_before = _host(fl.detect(ones))
    torch.cuda.synchronize()
    nreg = B * fl.lay["robot_bytes"]
    snap = fl._buf[:GUARD + nreg].clone()
    worst, worst_truth, edges = 0.0, 0.0, 0
    for call, (key, partner, mask) in _calls(name).items():
        want = xc.restated(name, call if name != "long" else "long")
        _sentinels(al)
        out = _host(al.detect_cross(np.array(key, np.uint8), np.array(partner, np.int32), None if mask is None else np.array(mask, np.uint8)))
        for a, w in enumerate(want):
            got = {k: v[a] for k, v in out.items()}
            if w is None:                                  # masked out: nothing is written
                assert got["found"] == 7 and (got["edge"] == -9).all() and (got["stats"] == -3).all() and got["rms"] == 77.0, (call, a)
                continue
            if not w["key"]:                               # key clear: found = 0 and nothing else
                assert got["found"] == 0 and (got["edge"] == -9).all() and (got["stats"] == -3).all() and (got["tf12"] == 123.0).all(), (call, a)
                continue
            assert got["found"] == w["found"] and got["edge"].tolist() == w["edge"] and got["stats"].tolist() == w["stats"], (name, call, a, got, w)
            if not w["found"]:                             # tf12, T_w1_w2 and rms are written only when found
                assert (got["tf12"] == 123.0).all() and (got["T_w1_w2"] == -55.0).all() and got["rms"] == 77.0
                continue
            edges += 1
            q, b, i, _ = w["edge"]
            T = liw.loop.tf12_to_mat(got["T_w1_w2"])
            d = max(float(np.abs(liw.loop.tf12_to_mat(got["tf12"]) - w["tf12"]).max()), float(np.abs(T - w["T"]).max()), abs(got["rms"] - w["rms"]))
            worst = max(worst, d)
            assert d <= BAR, (name, call, a, d)
            truth = xc.truth(name, a, b)
            dev, dev_host = float(np.abs(T - truth).max()), float(np.abs(w["T"] - truth).max())
            worst_truth = max(worst_truth, dev)
            assert dev <= 2 * dev_host, (name, call, a, dev, dev_host)
            # T_w1_w2 = (tf_a[q] tf12) inverse(tf_b[i]) with liw_lie_mul's arithmetic, from the device's own tf and tf12
            tfa, tfb = liw.loop.mat_to_tf12(fl.status(a, q)["tf"]), liw.loop.mat_to_tf12(fl.status(b, i)["tf"])
            assert mul(mul(tfa, got["tf12"]), inv(tfb)).tobytes() == got["T_w1_w2"].tobytes(), (name, call, a)
    torch.cuda.synchronize()
    assert torch.equal(fl._buf[:GUARD + nreg], snap)                                  # the robot regions and the guard in front are only read
    assert bool((fl._buf[-GUARD:] == 0xA5).all())
    own_after = _host(fl.detect(ones))
    for k in own_before:
        assert np.array_equal(own_before[k], own_after[k]), k                         # own detection on the same store gives what it gave
    assert edges >= (1 if name == "long" else 7)       # main: robots 0, 1, 2, 3, 5; claim: robots 0, 1
    print("cross detection, fleet %s: %d edges equal (found, edge, stats); tf12 / T_w1_w2 / rms max difference %.3e; from the truth %.3e"
          % (name, edges, worst, worst_truth))
    fl.close()


# --------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ("s3", "s1"))
def test_pairs_equal_the_single_detectors_match(liw, synth, name):
    """For the pairs with K_a = K_b + S one single-robot LoopDetector (the parent's kernels) is fed b's key frames and then a's last S:
    its key frame K_b + S - 1 holds a's newest sub-map, match(K_b + S - 1, i) draws with the same (q, c), and its size, draw, row,
    bin, query row and both index lists must equal the fleet's pair summary and list."""
    F = xc.fleet(name)
    S, s = xc.SUBMAP[name], xc.SUBMAP[name] // 3 + 1
    fl = _fed(liw, synth, name)
    al = _aligner(liw, fl, name)
    key, partner, mask = xc.CALLS["main"]
    al.detect_cross(np.array(key, np.uint8), np.array(partner, np.int32))
    want = xc.restated(name, "main")
    pairs = accepted = 0
    for a, b in xc.KA_KB_PAIRS:
        Ka, Kb = F["K"][a], F["K"][b]
        assert Ka == Kb + S
        det = liw.loop.LoopDetector(synth.office_params(), dict(F["params"], max_dis=1e30), dict(max_keyframes=Ka, max_points=xc.MAX_POINTS))
        for pose, T, Cn in F["frames"][b] + F["frames"][a][Ka - S:]:
            det.add_keyframe(T, Cn)
        assert det.get_points(Ka - 1).tobytes() == fl.get_points(a, Ka - 1).tobytes()
        for i in range(0, Kb, s):
            m, g = det.match(Ka - 1, i), al.get_pair(a, i)
            assert m["gate"] in (0, 4)
            assert (g["size"], g["draw"], g["row"], g["bin"], g["quick_pass"]) == (m["size"], m["draw"], m["row"], m["bin"], m["quick_pass"]), (a, i, g, m)
            w = want[a]["cands"][i]["match"]
            assert (g["size"], g["draw"], g["row"], g["bin"]) == (w["size"], w["draw"], w["row"], w["bin"])
            if m["size"] > F["params"]["min_match_threshold"]:
                assert g["query_row"] == m["query_row"] and np.array_equal(g["p1"], m["p1"]) and np.array_equal(g["p2"], m["p2"]), (a, i)
                assert g["p1"].tolist() == w["p1"] and g["p2"].tolist() == w["p2"]
                accepted += 1
            pairs += 1
    assert pairs >= 10 and accepted >= 8
    with pytest.raises(liw.LiwError):
        al.get_pair(6, 0)               # robot 6 launched nothing
    fl.close()


# --------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ("s3", "s1"))
def test_partner_and_link_equal_the_restatement(liw, synth, name):
    import torch
    fl = _fed(liw, synth, name)
    mul, inv = _lie(liw)
    worst = 0.0
    for sc in xc.link_scenarios(name):
        anchors = {r: xc.anchor_T(r) for r in sc["anchors"]}
        al = _aligner(liw, fl, name, anchors=anchors)
        assert al.group_linked.cpu().tolist() == [xc.GROUP_OF[r] if r in anchors else -1 for r in range(8)]
        for rnd in range(3):            # the partner kernel against its restatement, on the flags of the scenario's start
            assert al.choose_partners(rnd).cpu().tolist() == xc.choose_partners(xc.GROUP_OF, [int(r in anchors) for r in range(8)], rnd)
        for st in sc["steps"]:
            key, partner, mask = xc.CALLS[st["call"]]
            det = _host(al.detect_cross(np.array(key, np.uint8), np.array(partner, np.int32)))
            before = dict(linked=al.linked.cpu().numpy().copy(), T_g_w=al.T_g_w.cpu().numpy().copy(), via=al.via.cpu().numpy().copy())
            out = _host(al.link(partner=np.array(partner, np.int32)))
            assert out["linked"].tolist() == st["linked"] and out["via"].tolist() == st["via"] and out["group_linked"].tolist() == st["group_linked"], (name, st["call"], out)
            for r in range(8):
                if before["linked"][r] or not out["linked"][r]:
                    assert out["T_g_w"][r].tobytes() == before["T_g_w"][r].tobytes()              # nothing is re-linked; unlinked robots untouched
                    assert out["via"][r].tolist() == before["via"][r].tolist()
                    continue
                src = int(out["via"][r][0])
                own_edge = partner[r] == src and det["found"][r] and before["linked"][src]
                want = mul(before["T_g_w"][src], inv(det["T_w1_w2"][r])) if own_edge else mul(before["T_g_w"][src], det["T_w1_w2"][src])
                assert mc.ulps(out["T_g_w"][r], want) <= ULP_BAR, (name, r)
                worst = max(worst, float(np.abs(liw.loop.tf12_to_mat(out["T_g_w"][r]) - st["T_g_w"][r]).max()))
        # anchors keep what they were given
        T = al.T_g_w.cpu().numpy()
        for r in anchors:
            assert np.array_equal(liw.loop.tf12_to_mat(T[r]), anchors[r])
    assert worst <= 1e-8                # two composed edges of the 1e-9 bar
    print("link, fleet %s: linked / via / group_linked equal; T_g_w max difference from the restatement %.3e" % (name, worst))
    # push: partner -> detect -> link with the round counter; the chain 0 -> 3 -> 5 links in three rounds of partner choice at most
    al = _aligner(liw, fl, name, anchors=(0, 4))
    added = torch.tensor(xc.CALLS["main"][0], dtype=torch.uint8, device="cuda")
    linked, Tg, via = [1, 0, 0, 0, 1, 0, 0, 0], [xc.anchor_T(r) if r in (0, 4) else np.eye(4) for r in range(8)], [[-1] * 4 for _ in range(8)]
    for rnd in range(3):
        partner = xc.choose_partners(xc.GROUP_OF, linked, rnd)
        res = xc.detect(name, xc.CALLS["main"][0], partner)
        gl = xc.link(xc.GROUP_OF, partner, [x["found"] for x in res], [x.get("edge", [-1, -1, -1, 0]) for x in res], [x.get("T") for x in res], linked, Tg, via)
        out = _host(al.push(dict(added=added)))
        assert out["partner"].tolist() == partner and out["linked"].tolist() == linked and out["via"].tolist() == via and out["group_linked"].tolist() == gl, rnd
    assert al.round == 3 and linked == [1, 1, 1, 1, 1, 1, 0, 0]
    fl.close()


# --------------------------------------------------------------------------------------------------------------------- 4
def test_determinism_and_tiling(liw, synth):
    """two runs bit-equal, and 32 tiled copies of the eight robots (partners offset per tile) give what the eight give"""
    import torch
    name, tiles = "s3", 32
    key, partner, mask = xc.CALLS["main"]
    B = 8 * tiles
    pt = np.array([p + 8 * t if 0 <= p < 8 else (B if p >= 8 else p) for t in range(tiles) for p in partner], np.int32)
    kt = np.tile(np.array(key, np.uint8), tiles)
    runs = []
    for _ in range(2):
        fl = _fed(liw, synth, name, tiles=tiles)
        al = _aligner(liw, fl, name)
        out = {k: v.clone() for k, v in al.detect_cross(kt, pt).items()}
        out.update({k: v.clone() for k, v in al.link(partner=pt).items()})
        torch.cuda.synchronize()
        runs.append((fl, al, out))
    (fa, aa, oa), (fb, ab, ob) = runs
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(fa._buf, fb._buf)                    # the whole store, scratch included
    one = xc.restated(name, "main")
    off = (8 * torch.arange(tiles, device="cuda", dtype=torch.int32)).view(tiles, 1)
    for k in ("found", "tf12", "T_w1_w2", "rms", "stats", "linked", "T_g_w", "group_linked"):
        v = oa[k].view(tiles, 8, -1)
        if k in ("tf12", "T_w1_w2", "rms"):                  # written only when found
            v = v[:, [a for a in range(8) if one[a] and one[a]["found"]]]
        assert torch.equal(v, v[0:1].expand_as(v)), k
    e = oa["edge"].view(tiles, 8, 4).clone()
    e[:, :, 1] = torch.where(oa["found"].view(tiles, 8) != 0, e[:, :, 1] - off, e[:, :, 1])      # the partner's index, where an edge was written
    assert torch.equal(e, e[0:1].expand_as(e))
    assert e[0].cpu().tolist() == [w["edge"] if w and w["key"] else [0, 0, 0, 0] for w in one]
    vv = oa["via"].view(tiles, 8, 4).clone()
    vv[:, :, 0] = torch.where(vv[:, :, 0] >= 0, vv[:, :, 0] - off, vv[:, :, 0])
    assert torch.equal(vv, vv[0:1].expand_as(vv))
    assert oa["linked"].view(tiles, 8)[5].cpu().tolist() == xc.link_scenarios(name)[0]["steps"][0]["linked"]
    fa.close()
    fb.close()


# --------------------------------------------------------------------------------------------------------------------- 5
def test_einval_writes_nothing(liw, synth):
    import torch
    name = "s1"
    fl = _fed(liw, synth, name, guard=GUARD)
    al = _aligner(liw, fl, name)
    key, partner, mask = xc.CALLS["main"]
    al.detect_cross(np.array(key, np.uint8), np.array(partner, np.int32))
    al.link()
    torch.cuda.synchronize()
    tens = dict(found=al.found, edge=al.edge, tf12=al.tf12, T=al.T_w1_w2, rms=al.rms, stats=al.stats, linked=al.linked, Tg=al.T_g_w, via=al.via,
                gl=al.group_linked, partner=al.partner)
    snap, osnap = fl._buf.clone(), {k: v.clone() for k, v in tens.items()}
    L, h = al.L, fl.h
    vp = lambda t: C.c_void_p(t.data_ptr())
    X = liw.loop_cross.XloopParamsC
    st, odd = vp(fl.store), C.c_void_p(fl.store.data_ptr() + 4)
    kt, pt = torch.tensor(key, dtype=torch.uint8, device="cuda"), torch.tensor(partner, dtype=torch.int32, device="cuda")
    k, p = vp(kt), vp(pt)
    good = X(xc.MIN_MATCH[name], xc.MAX_RMS)
    o = [vp(al.found), vp(al.edge), vp(al.tf12), vp(al.T_w1_w2), vp(al.rms), vp(al.stats)]
    calls = [L.liw_xloop_detect(h, None, k, p, C.byref(good), None, *o, None), L.liw_xloop_detect(h, odd, k, p, C.byref(good), None, *o, None),
             L.liw_xloop_detect(h, st, None, p, C.byref(good), None, *o, None), L.liw_xloop_detect(h, st, k, None, C.byref(good), None, *o, None),
             L.liw_xloop_detect(h, st, k, p, None, None, *o, None),
             L.liw_xloop_detect(h, st, k, p, C.byref(X(fl.params["min_match_threshold"] - 1, 0.01)), None, *o, None),
             L.liw_xloop_detect(h, st, k, p, C.byref(X(9, -0.5)), None, *o, None)]
    for i in range(6):
        a = list(o)
        a[i] = None
        calls.append(L.liw_xloop_detect(h, st, k, p, C.byref(good), None, *a, None))
    g, lk = vp(al.group_of), vp(al.linked)
    calls += [L.liw_xloop_partner(h, None, lk, 0, vp(al.partner), None), L.liw_xloop_partner(h, g, None, 0, vp(al.partner), None),
              L.liw_xloop_partner(h, g, lk, 0, None, None), L.liw_xloop_partner(h, g, lk, -2, vp(al.partner), None)]
    la = [g, p, vp(al.found), vp(al.edge), vp(al.T_w1_w2), lk, vp(al.T_g_w), vp(al.via), vp(al.group_linked)]
    for i in range(9):
        a = list(la)
        a[i] = None
        calls.append(L.liw_xloop_link(h, *a, None))
    info = np.zeros(8, np.int32)
    ip = info.ctypes.data_as(C.POINTER(C.c_int))
    calls += [L.liw_xloop_get_pair(h, None, 0, 0, 0, ip, None, None), L.liw_xloop_get_pair(h, st, 8, 0, 0, ip, None, None),
              L.liw_xloop_get_pair(h, st, 1, 1, 0, None, None, None), L.liw_xloop_get_pair(h, st, 6, 0, 0, ip, None, None)]
    torch.cuda.synchronize()
    assert calls == [-22] * len(calls), calls
    assert torch.equal(fl._buf, snap)
    for kk, v in tens.items():
        assert torch.equal(v, osnap[kk]), kk
    fl.close()


# --------------------------------------------------------------------------------------------------------------------- 6
def test_end_to_end_two_robots_one_room(liw, synth):
    """FleetLoopDetector.push -> FleetGroupAligner.push -> FleetGroupMap.render_all(backend, group_linked, T_g_w) for two robots of one
    room with world frames of their own: robot 1 links to the anchor through a cross edge, the group grid equals the serial walk
    fed the read-back T_g_l, it has twice-hit cells that neither robot has on the same lattice, and none of the three calls copies
    anything to the host."""
    import math
    import torch
    import loop_batch_cases as lbc
    import loop_reference as lref
    prm = synth.office_params()
    rng = np.random.default_rng(5)
    pose_of, _ = lbc._lie()
    Tiw, Til = lbc.T_imu_to_wheel(), liw.loop.tf12_to_mat(mc.til12(liw, prm))
    Lm = tgl._landmarks(np.random.default_rng(900))
    room = mc._replay().replay_room()                     # its outer box holds the paths; the landmarks stand for the corners of its furniture
    W = [xc._world(0, 21), xc._world(1, 21)]
    bases = [xc._line(-2.0, 0.0, 0.0, 5), xc._line(-0.8, -1.2, math.pi / 2, 5)]       # robot 1 ends on robot 0's path
    B, K, cap, n_rays = 2, 5, 8, 90
    fl = liw.FleetLoopDetector(prm, tgl._params(submap_count=1, min_interval=2), dict(B=B, max_keyframes=cap, max_points=64, max_kf_corners=32))
    fb = liw.FleetBackEnd(prm, liw.posegraph.office_pg_params(), dict(B=B, max_keyframes=cap, max_loops=4), solve_period=1e9)
    fm = mc.mapper(liw, synth, B, cap, cap * n_rays, 1 << 19, 2048, prm=prm)
    gm = liw.FleetGroupMap(fm, 1, 1 << 21)
    al = liw.FleetGroupAligner(fl, [0, 0], [0], 9, xc.MAX_RMS)
    subs_of, frames, poses = [[], []], [], [[], []]
    for t in range(K):
        items = []
        for r in range(B):
            Cn = tgl._seen(Lm, bases[r][t], r=2.5)
            Cn[:, :2] += rng.uniform(-xc.NOISE, xc.NOISE, (len(Cn), 2))
            pose = pose_of(W[r] @ bases[r][t] @ lref.iso_inv(Tiw))
            items.append((pose, Cn @ W[r][:3, :3].T + W[r][:3, 3]))
            poses[r].append(pose)
            Tl = bases[r][t] @ lref.iso_inv(Tiw) @ Til                               # the laser in the room
            subs_of[r].append(mc.scan(room, Tl[0, 3], Tl[1, 3], math.atan2(Tl[1, 0], Tl[0, 0]), n_rays, rng))
        frames.append(tlb._upload(torch, B, 48, items))
    stamps = torch.zeros(B, dtype=torch.float64, device="cuda")
    reads = []
    for o, names in ((gm, ("_sync", "infos", "info_of", "grid", "members")), (fm, ("_sync", "infos", "tf", "info_of", "grid")), (fl, ("_sync",)),
                     (fb, ("_sync", "_read_n_due"))):
        for nm in names:
            setattr(o, nm, (lambda real, nm: lambda *a, **k: reads.append(nm) or real(*a, **k))(getattr(o, nm), nm))
    for t in range(K):
        loop_out = fl.push(frames[t])
        fb.add_keyframes(loop_out["added"], frames[t]["pose"], stamps + t)
        fm.add_keyframes(*mc.frame(subs_of, t, n_rays))
        al.push(loop_out)
    gm.render_all(fb, al.group_linked, al.T_g_w)
    assert not reads                                                                 # no device -> host copy in the three calls
    assert al.linked.cpu().tolist() == [1, 1] and al.group_linked.cpu().tolist() == [0, 0] and int(al.via[1, 0]) == 0
    assert np.allclose(fb.keyframes(1)["poses"], np.array(poses[1]), rtol=0, atol=1e-9)              # the back-end holds the poses it was given
    Tg = al.T_g_w.cpu().numpy()
    assert np.array_equal(liw.loop.tf12_to_mat(Tg[0]), np.eye(4))
    assert np.abs(liw.loop.tf12_to_mat(Tg[1]) - W[0] @ lref.iso_inv(W[1])).max() < 0.02
    status, rows = gm.gstatus.cpu().numpy(), gm.infos()
    assert status.tolist() == [0]
    T_g_l = [fm.tf(b) for b in range(B)]
    assert T_g_l[0].shape == T_g_l[1].shape == (K, 12)
    want = mref.render(*gc.concat(T_g_l, subs_of, [0, 1]), mc.RES)
    gc.assert_group(gm, 0, want, rows[0])
    # twice-hit cells of the group grid in which neither robot alone has two hits (its own render on this lattice shows 50 at most)
    grid = gm.grid(0).reshape(-1)
    hits = np.zeros((B, grid.size), np.int32)
    for b in range(B):
        for T, pts in zip(T_g_l[b], subs_of[b]):
            for pt in pts:
                P = mref.world_point([float(v) for v in T], pt)
                idx = mref._cell(P[0], P[1], want["origin_x"], want["origin_y"], mc.RES, want["width"], want["height"])
                if idx > -1:
                    hits[b, idx] += 1
    shared = int(((grid == 100) & (hits[0] < 2) & (hits[1] < 2)).sum())
    print("end to end: %d cells of value 100, %d of them hit once by each robot" % (int((grid == 100).sum()), shared))
    assert shared > 0
    for o in (fl, fb, fm, gm):
        o.close()
