"""The wave-per-robot add_scan kernel of the batched laser front-end (k_lfe_add_scan_wave behind liw_lfe_add_scan,
liw_lfe_add_scan_flags and the one-launch liw_lfe_rebuild), and the flags that tell what a call did.  References: the
lane-per-robot kernel kept behind LIW_LFE_ADD_SCAN=lane for the store bytes, a numpy state machine and the host LaserManager
for the flags; never the new kernel's own output.

What is compared between the two kernels (the contract of include/liw_laser_batch.h): the 256-byte manager record, every scan
slot as a whole, and of each sub-map slot the header, lines[0 .. n_lines) and entries[0 .. n_entries), as bytes.  A sub-map with a
capacity bit (LINES / CELLS) is compared in its status word only; bytes past n_lines / n_entries are nobody's."""
import numpy as np
import pytest

from test_gpu_laser_batch import ANG_INC, ANG_MIN, N_RAYS, T_INC, Scene, _pose, _T
from test_gpu_laser_spawn_wave import slot_parts, zigzag_scan

pytestmark = pytest.mark.gpu

HDR, MGR = 32, 256
B0, F0 = 24, 6
R_ZIGZAG, R_EMPTY, R_WALL_A, R_INVALID, R_WALL_B = 0, 1, 3, 4, 8
NEW_CAP = 2048          # new entries of one target the wave kernel holds in LDS (kAddNewCap); beyond it one lane runs the serial code
LDS_MAX = 64 * 1024


@pytest.fixture(scope="module")
def env(liw):
    import torch
    lp = liw.laser.office_laser_params()
    return liw, lp, Scene(liw, lp), torch


def _dims(B, slots, max_points=N_RAYS, max_lines=512, max_cell_entries=8192):
    return dict(B=B, slots=slots, max_points=max_points, max_lines=max_lines, max_cell_entries=max_cell_entries)


def _regions(dims):
    sb = (HDR + 80 * dims["max_lines"] + 8 * dims["max_cell_entries"] + 255) // 256 * 256
    return MGR + (dims["slots"] + 2) * sb, sb


def _wall(rng, n=40):
    return np.stack([np.linspace(-0.5, 0.5, n), np.full(n, 1.5) + rng.normal(0, 0.002, n), np.zeros(n)], 1)


@pytest.fixture(scope="module")
def scen(env):
    """24 robots x 6 frames: rooms seen along a random walk (steps up to 0.4 m and 12 degrees, and on a third of the steps exactly
    the pose before, which the motion filter drops), the zig-zag ring (robot 0: 90 lines a scan), a scan without points (robot 1,
    frame 2), two one-wall robots (3 and 8), a slot made invalid at spawn (robot 4, frame 1); robots 2, 7, 12, 17, 22 are masked
    out of every call."""
    liw, lp, sc, torch = env
    rng = np.random.default_rng(5100)
    poses = np.zeros((B0, F0, 6))
    for b in range(B0):
        poses[b, 0] = _pose(rng)
        for k in range(1, F0):
            poses[b, k] = poses[b, k - 1] if (k + b) % 3 == 0 else _pose(rng, poses[b, k - 1], 0.4, np.deg2rad(12))
    zz = zigzag_scan(liw)
    lists = []
    for b in range(B0):
        if b == R_ZIGZAG:
            lists.append([zz] * F0)
        elif b in (R_WALL_A, R_WALL_B):
            lists.append([_wall(rng) for _ in range(F0)])
        else:
            lists.append([sc.points(300 + b, poses[b, k], seed=10 * b + k)[0] for k in range(F0)])
    lists[R_EMPTY][2] = np.zeros((0, 3))
    for k in range(1, F0):   # the ring is cast at the laser origin: small real steps, none of them filtered
        poses[R_ZIGZAG, k] = _pose(rng, poses[R_ZIGZAG, k - 1], 0.05, np.deg2rad(2))
    mask = np.array([0 if b % 5 == 2 else 1 for b in range(B0)], dtype=np.uint8)
    return dict(poses=poses, lists=lists, mask=mask, invalid={(R_INVALID, 1)})


def _front_end(env, lp, dims, guard=0):
    liw, _, _, torch = env
    fe = liw.laser_batch.BatchFrontEnd(lp, dims)
    big = None
    if guard:
        n = fe.store.numel()
        big = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        fe.store = big[guard:guard + n]
        fe.reset()
    return fe, big


def _spawn_all(env, fe, lists, frames, first_slot, invalid=()):
    liw, _, _, torch = env
    mp = fe.max_points
    for k in frames:
        P, n = liw.laser_batch.pad_points([l[k] for l in lists], mp)
        for (b, kk) in invalid:
            if kk == k:
                n[b] = mp + 1
        fe.spawn(first_slot + k, torch.from_numpy(P).cuda(), torch.from_numpy(n).cuda())


def _snap(torch, fe):
    torch.cuda.synchronize()
    return fe.store.cpu().numpy().copy()


def _run(env, lp, dims, lists, poses, kernel, frames, first_slot=0, mask=None, invalid=(), guard=0, keep=False):
    """spawn the frames' scans, then one add_scan per frame under the given kernel ("wave": the default, "lane": the knob) ->
    dict(snaps: the store after the spawns and after every call, flags [F, B], paths)"""
    liw, _, _, torch = env
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("LIW_LFE_SPAWN", raising=False)
        if kernel == "lane":
            mp.setenv("LIW_LFE_ADD_SCAN", "lane")     # read per call
        else:
            mp.delenv("LIW_LFE_ADD_SCAN", raising=False)
        fe, big = _front_end(env, lp, dims, guard)
        _spawn_all(env, fe, lists, frames, first_slot, invalid)
        snaps, flags, paths = [_snap(torch, fe)], [], []
        for k in frames:
            fl = fe.add_scan(first_slot + k, poses[:, k], mask=mask, flags=True)
            paths.append(fe.add_scan_path())
            snaps.append(_snap(torch, fe))
            flags.append(fl.cpu().numpy().copy())
        out = dict(snaps=snaps, flags=np.stack(flags), paths=paths, dims=dims)
        if keep:
            out["fe"], out["big"] = fe, big
        return out


def _mgr(store, dims, b):
    rb, _ = _regions(dims)
    raw = store[b * rb:b * rb + MGR]
    i = raw[:32].view(np.int32)
    d = raw[32:32 + 8 * 24].view(np.float64)
    return dict(raw=raw, status=int(i[0]), has_ref=int(i[1]), has_spawn=int(i[2]), ref_sub=int(i[3]), count=int(i[4]), sub_p=d[0:6].reshape(2, 3),
                sub_q=d[6:12].reshape(2, 3))


def _hdr(h):
    v = h[:12].view(np.int32)
    return int(v[0]), int(v[1]), int(v[2])


CAPACITY = 2 | 4   # ST_LINES | ST_CELLS


def _assert_same_state(sw, sl, dims, what, robots=None):
    """the contract, for every robot: manager record and scan slots as bytes; sub-maps header + lines[:n_lines] + entries[:n_entries],
    or the status word alone when the lane kernel flagged the sub-map with a capacity bit.  -> number of sub-maps compared in full"""
    rb, sb = _regions(dims)
    S = dims["slots"]
    full = 0
    for b in (range(dims["B"]) if robots is None else robots):
        rw, rl = sw[b * rb:(b + 1) * rb], sl[b * rb:(b + 1) * rb]
        assert np.array_equal(rw[:MGR], rl[:MGR]), (what, b, "manager record", rw[:32].view(np.int32), rl[:32].view(np.int32))
        assert np.array_equal(rw[MGR:MGR + S * sb], rl[MGR:MGR + S * sb]), (what, b, "scan slots")
        for sub in (S, S + 1):
            hw, lw, ew = slot_parts(sw, dims, b, sub)
            hl, ll, el = slot_parts(sl, dims, b, sub)
            st, nl, ne = _hdr(hl)
            if st & CAPACITY:
                assert _hdr(hw)[0] == st, (what, b, sub, "status of an overflowed sub-map", _hdr(hw), _hdr(hl))
                continue
            assert np.array_equal(hw, hl), (what, b, sub, "header", _hdr(hw), _hdr(hl))
            assert 0 <= nl <= dims["max_lines"] and 0 <= ne <= dims["max_cell_entries"]
            assert np.array_equal(lw[:nl].view(np.uint64), ll[:nl].view(np.uint64)), (what, b, sub, "lines")
            assert np.array_equal(ew[:ne], el[:ne]), (what, b, sub, "entries")
            full += 1
    return full


_light = {}


def _pair(env, scen, n_acc, wh):
    """the scenario under both kernels; the flags and manager states of the wave run are kept for the tests that need no more"""
    lp = dict(env[1], ref_n_accumulation=n_acc, w_laser_each_scan=float(wh), h_laser_each_scan=float(wh))
    dims = _dims(B0, F0 + 1)
    args = dict(frames=range(F0), first_slot=1, mask=scen["mask"], invalid=scen["invalid"])
    w = _run(env, lp, dims, scen["lists"], scen["poses"], "wave", **args)
    l = _run(env, lp, dims, scen["lists"], scen["poses"], "lane", **args)
    states = [[tuple(_mgr(w["snaps"][k + 1], dims, b)[f] for f in ("has_ref", "has_spawn", "count")) for b in range(B0)] for k in range(F0)]
    _light[(n_acc, wh)] = dict(lp=lp, flags=w["flags"].copy(), states=states, paths=list(w["paths"]))
    return lp, dims, w, l


def _lines_outside(lp, m, src_lines, pose, half):
    """source lines that lie wholly outside the grid of the reference sub-map after the transform of an accumulating call, by a
    margin of two cells, and are long enough to be accepted: (count, of them longer than 0.1 m)"""
    Til = np.asarray(lp["T_imu_to_laser"], dtype=np.float64).reshape(4, 4)
    rs = m["ref_sub"] & 1
    Tl = np.linalg.inv(Til) @ np.linalg.inv(_T(m["sub_p"][rs], m["sub_q"][rs])) @ _T(pose[:3], pose[3:]) @ Til
    out = 0
    for ln in src_lines:
        a, c = Tl[:3, :3] @ ln[0:3] + Tl[:3, 3], Tl[:3, :3] @ ln[3:6] + Tl[:3, 3]
        lim = half + 0.1
        side = (min(a[0], c[0]) > lim) or (max(a[0], c[0]) < -lim) or (min(a[1], c[1]) > lim) or (max(a[1], c[1]) < -lim)
        if side and ln[9] > 0.1:
            out += 1
    return out


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n_acc,wh", [(2, 100), (4, 100), (2, 6), (4, 6)])
def test_store_bytes_equal_lane_kernel(env, scen, n_acc, wh):
    liw, lp0, sc, torch = env
    lb = liw.laser_batch
    lp, dims, w, l = _pair(env, scen, n_acc, wh)
    assert w["paths"] == [1] * F0 and l["paths"] == [0] * F0
    mask, poses = scen["mask"], scen["poses"]
    rb, sb = _regions(dims)
    assert np.array_equal(w["snaps"][0], l["snaps"][0])            # the same scans in the same slots
    assert slot_parts(w["snaps"][0], dims, R_ZIGZAG, 1)[0][4:8].view(np.int32)[0] > 64
    assert slot_parts(w["snaps"][0], dims, R_EMPTY, 3)[0][4:8].view(np.int32)[0] == 0
    assert slot_parts(w["snaps"][0], dims, R_WALL_A, 1)[0][4:8].view(np.int32)[0] in (1, 2)    # one wall (its noise may split it)
    assert slot_parts(w["snaps"][0], dims, R_INVALID, 2)[0][:4].view(np.int32)[0] & lb.ST_POINTS
    seen = dict(filtered=0, first=0, two=0, swap_sp=0, swap_quirk=0, spawned=0, outside=0)
    full = 0
    for k in range(F0):
        sw, sl = w["snaps"][k + 1], l["snaps"][k + 1]
        full += _assert_same_state(sw, sl, dims, (n_acc, wh, "frame", k))
        assert np.array_equal(w["flags"][k], l["flags"][k]), (k, w["flags"][k], l["flags"][k])
        for b in range(B0):
            fl = int(l["flags"][k][b])
            if not mask[b]:
                assert fl == 0
                for s in (w, l):                          # a masked robot's region never changes
                    assert np.array_equal(s["snaps"][k + 1][b * rb:(b + 1) * rb], s["snaps"][0][b * rb:(b + 1) * rb]), (b, k)
                continue
            before = _mgr(l["snaps"][k], dims, b)
            seen["filtered"] += fl == 0
            seen["first"] += bool(fl & lb.ADD_FIRST)
            seen["spawned"] += bool(fl & lb.ADD_SPAWNED)
            seen["two"] += bool(fl & lb.ADD_ADDED) and not fl & lb.ADD_FIRST and before["has_ref"] == 1 and before["has_spawn"] == 1
            seen["swap_sp"] += bool(fl & lb.ADD_SWAPPED) and before["has_spawn"] == 1
            seen["swap_quirk"] += bool(fl & lb.ADD_SWAPPED) and before["has_spawn"] == 0
            if wh == 6 and fl & lb.ADD_ADDED and not fl & lb.ADD_FIRST:
                _, src, _ = slot_parts(l["snaps"][0], dims, b, 1 + k)
                nsrc = _hdr(slot_parts(l["snaps"][0], dims, b, 1 + k)[0])[1]
                out = _lines_outside(lp, before, src[:nsrc], poses[b, k], 3.0)
                if out:
                    ref = dims["slots"] + (before["ref_sub"] & 1)
                    grown = _hdr(slot_parts(l["snaps"][k + 1], dims, b, ref)[0])[1] - _hdr(slot_parts(l["snaps"][k], dims, b, ref)[0])[1]
                    assert grown <= nsrc - out, (b, k, grown, nsrc, out)   # they took no id in the reference sub-map
                    seen["outside"] += out
    st = [_mgr(l["snaps"][-1], dims, b)["status"] for b in range(B0)]
    print("add_scan wave == lane, n_acc=%d grid=%d m: %d sub-maps compared in full over %d calls; %s; robot words %s"
          % (n_acc, wh, full, F0, seen, sorted(set(st))))
    assert all(not (s & CAPACITY) for s in st)                       # nothing overflowed: everything above was compared in full
    assert st[R_INVALID] & lb.ST_INVALID
    assert seen["filtered"] and seen["first"] and seen["two"] and seen["swap_sp"]
    if n_acc == 2:
        assert seen["swap_quirk"]
    else:
        assert seen["spawned"] and not seen["swap_quirk"]
    if wh == 6:
        assert seen["outside"] >= 1                                  # accepted lines without a valid cell


# ------------------------------------------------------------------------------------------------------------------ 2
def _angle(R):
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(v) / 2, (np.trace(R) - 1) / 2))


def _host_machine(lb, poses, n_acc, mf_p, mf_q):
    """laser_manager::add_scan's state machine for one robot -> (flags per frame, (has_ref, has_spawn, count) per frame, the
    smallest distance of a step's translation / rotation from the filter's thresholds)"""
    has_ref = has_spawn = count = 0
    last, flags, states, margin = None, [], [], np.inf
    for pose in poses:
        T = _T(pose[:3], pose[3:])
        fl = 0
        if has_ref:
            d = np.linalg.inv(last) @ T
            tn, an = float(np.linalg.norm(d[:3, 3])), _angle(d[:3, :3])
            margin = min(margin, abs(tn - mf_p), abs(an - mf_q))
            if not (tn < mf_p and an < mf_q):
                fl = lb.ADD_ADDED
                count += 1
                if not has_spawn and count == n_acc // 2:
                    has_spawn, fl = 1, fl | lb.ADD_SPAWNED
                if count == n_acc:
                    has_ref, has_spawn, count, fl = has_spawn, 1, n_acc // 2, fl | lb.ADD_SWAPPED
                last = T
        else:
            has_ref, count, last, fl = 1, 1, T, lb.ADD_ADDED | lb.ADD_FIRST
        flags.append(fl)
        states.append((has_ref, has_spawn, count))
    return flags, states, margin


@pytest.mark.parametrize("n_acc", [2, 4])
def test_flags_equal_host_state_machine(env, scen, n_acc):
    liw, lp0, sc, torch = env
    lb = liw.laser_batch
    if (n_acc, 100) not in _light:
        _pair(env, scen, n_acc, 100)
    w = _light[(n_acc, 100)]
    lp = w["lp"]
    assert w["paths"] == [1] * F0
    margin, nz = np.inf, 0
    for b in range(B0):
        if not scen["mask"][b]:
            assert not w["flags"][:, b].any()
            continue
        flags, states, m = _host_machine(lb, scen["poses"][b], n_acc, lp["ref_motion_filter_p"], lp["ref_motion_filter_q"])
        margin = min(margin, m)
        mgr = liw.laser.LaserManager(lp)
        for k in range(F0):
            assert int(w["flags"][k, b]) == flags[k], (b, k, int(w["flags"][k, b]), flags[k])
            d = dict(zip(("has_ref", "has_spawn", "count"), w["states"][k][b]))
            assert w["states"][k][b] == states[k], (b, k, d, states[k])
            mgr.add_scan(liw.laser.Scan.spawn(lp, scen["lists"][b][k]), scen["poses"][b, k, :3], scen["poses"][b, k, 3:])
            assert (mgr.ref_scan() is not None) == bool(d["has_ref"]), (b, k)
            nz += flags[k] != 0
    print("flags n_acc=%d: %d added scans; closest margin of a step to the motion filter's thresholds %.3e" % (n_acc, nz, margin))
    assert margin > 1e-6
    assert nz > B0


# ------------------------------------------------------------------------------------------------------------------ 3
def test_overflowing_submaps(env, scen):
    """ref_n_accumulation 4, three adds: the reference accumulates every one of them.  max_lines comes from the host's line counts
    of the scans (every scan slot fits, twice or three times a rich room's lines do not), max_cell_entries from the entry counts
    of the scan slots as spawn wrote them and of the first reference in the large store under the lane kernel (the host exposes no
    entry count)."""
    liw, lp0, sc, torch = env
    lb = liw.laser_batch
    lp = dict(lp0, ref_n_accumulation=4)
    F, G = 3, 4096
    lists = [scen["lists"][5] if b == R_ZIGZAG else scen["lists"][b] for b in range(B0)]   # rooms and the two one-wall robots
    poses = scen["poses"].copy()
    poses[R_ZIGZAG] = scen["poses"][5]
    for b in range(B0):                                     # no filtered step: three adds for everybody
        for k in range(1, F):
            if np.array_equal(poses[b, k], poses[b, k - 1]):
                poses[b, k, 0] += 0.2
    host_lines = np.array([[liw.laser.Scan.spawn(lp, lists[b][k]).lines().shape[0] for k in range(F)] for b in range(B0)])
    dL = _dims(B0, F)
    large = _run(env, lp, dL, lists, poses, "lane", range(F), keep=True)
    assert all(_mgr(large["snaps"][-1], dL, b)["status"] == 0 for b in range(B0))
    ents = np.array([[_hdr(slot_parts(large["snaps"][0], dL, b, k)[0])[2] for k in range(F)] for b in range(B0)])
    assert np.array_equal(host_lines, np.array([[_hdr(slot_parts(large["snaps"][0], dL, b, k)[0])[1] for k in range(F)] for b in range(B0)]))
    first_ref = max(_hdr(slot_parts(large["snaps"][1], dL, b, F + (_mgr(large["snaps"][1], dL, b)["ref_sub"] & 1))[0])[2] for b in range(B0))
    max_ents = max(int(ents.max()), first_ref)              # the first reference (one scan rasterised) fits as well
    mL = _np_match(large["fe"].match_with_ref(F - 1, poses[:, F - 1]))
    walls = (R_WALL_A, R_WALL_B)
    seen_bits = 0
    for max_lines, max_cells, bit in ((int(host_lines.max()) + 1, 8192, lb.ST_LINES), (512, max_ents + 8, lb.ST_CELLS)):
        dS = _dims(B0, F, max_lines=max_lines, max_cell_entries=max_cells)
        w = _run(env, lp, dS, lists, poses, "wave", range(F), guard=G, keep=True)
        l = _run(env, lp, dS, lists, poses, "lane", range(F), guard=G, keep=True)
        assert w["paths"] == [1] * F and l["paths"] == [0] * F
        for r in (w, l):
            torch.cuda.synchronize()
            assert (r["big"][:G] == 0xA5).all() and (r["big"][-G:] == 0xA5).all()
        assert np.array_equal(w["flags"], l["flags"]) and np.array_equal(w["flags"], large["flags"])
        mw, ml = _np_match(w["fe"].match_with_ref(F - 1, poses[:, F - 1])), _np_match(l["fe"].match_with_ref(F - 1, poses[:, F - 1]))
        for b in range(B0):                                 # every scan slot fits
            for k in range(F):
                assert _hdr(slot_parts(l["snaps"][0], dS, b, k)[0])[0] == 0, (b, k)
        flagged, first_at = [], {}
        for k in range(F):
            _assert_same_state(w["snaps"][k + 1], l["snaps"][k + 1], dS, ("overflow", bit, "call", k))
            for b in range(B0):
                if _mgr(l["snaps"][k + 1], dS, b)["status"] and b not in first_at:
                    first_at[b] = k
        sw, sl = w["snaps"][-1], l["snaps"][-1]
        for b in range(B0):
            gw, gl, gL = _mgr(sw, dS, b), _mgr(sl, dS, b), _mgr(large["snaps"][-1], dL, b)
            assert np.array_equal(gw["raw"], gl["raw"]), b
            if gl["status"]:
                flagged.append(b)
                assert gl["status"] & bit and gw["status"] == gl["status"], (b, gw["status"], gl["status"])
                for sub in (F, F + 1):
                    assert _hdr(slot_parts(sw, dS, b, sub)[0])[0] == _hdr(slot_parts(sl, dS, b, sub)[0])[0], (b, sub)
                assert mw["count"][b] == 0 and ml["count"][b] == 0, b
                continue
            assert np.array_equal(gw["raw"], gL["raw"]), b
            for s in (sw, sl):
                for sub in (F, F + 1):
                    hS, lS, eS = slot_parts(s, dS, b, sub)
                    hB, lB, eB = slot_parts(large["snaps"][-1], dL, b, sub)
                    st, nl, ne = _hdr(hB)
                    # status, n_lines, n_entries and time: the header's pad words keep the store's background (guard pattern)
                    assert np.array_equal(hS[:12], hB[:12]) and np.array_equal(hS[16:24], hB[16:24]) and st == 0, (b, sub)
                    assert np.array_equal(lS[:nl].view(np.uint64), lB[:nl].view(np.uint64)) and np.array_equal(eS[:ne], eB[:ne]), (b, sub)
            for m in (mw, ml):
                n = int(mL["count"][b])
                assert m["count"][b] == n
                for key in ("recs", "idx1", "idx2"):
                    assert np.array_equal(m[key][b, :n], mL[key][b, :n]), (b, key)
                assert np.array_equal(m["match_pose"][b], mL["match_pose"][b]), b
        print("overflow bit %d at max_lines=%d max_cell_entries=%d: flagged %s (first at call %s)" % (bit, max_lines, max_cells, flagged, first_at))
        assert flagged and len(flagged) < B0 and set(flagged).isdisjoint(walls)
        assert all(k in (1, 2) for k in first_at.values())            # at the second or the third add, never the first
        seen_bits |= bit
    assert seen_bits == lb.ST_LINES | lb.ST_CELLS


def _np_match(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()}


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("n_acc", [2, 4])
def test_rebuild_in_one_launch(env, scen, n_acc):
    liw, lp0, sc, torch = env
    lp = dict(lp0, ref_n_accumulation=n_acc)
    S = F0 + 2
    dims = _dims(B0, S)
    mask, poses = scen["mask"], scen["poses"]
    assert int((mask == 0).sum()) == 5
    rb, sb = _regions(dims)
    x = torch.zeros(B0, S, 15, dtype=torch.float64, device="cuda")     # the poses as frames 1 .. 6 of a states array
    x[:, 1:1 + F0, :6] = torch.from_numpy(poses).cuda()
    x[:, :, 6:] = 7.0

    def prepared(mp, kernel):
        mp.delenv("LIW_LFE_SPAWN", raising=False)
        mp.delenv("LIW_LFE_ADD_SCAN", raising=False)
        fe, _ = _front_end(env, lp, dims)
        _spawn_all(env, fe, scen["lists"], range(F0), 1, scen["invalid"])
        for s in (5, 2, 4):                                             # a manager state from before, under the reference kernel
            mp.setenv("LIW_LFE_ADD_SCAN", "lane")
            fe.add_scan(s, poses[:, ::-1][:, s - 1].copy())
        if kernel == "lane":
            mp.setenv("LIW_LFE_ADD_SCAN", "lane")
        else:
            mp.delenv("LIW_LFE_ADD_SCAN", raising=False)
        return fe, _snap(torch, fe)

    with pytest.MonkeyPatch.context() as mp:
        few, before = prepared(mp, "wave")
        few.rebuild(1, F0, x[:, 1:1 + F0], mask=mask)
        assert few.add_scan_path() == 1
        one = _snap(torch, few)
        fel, before_l = prepared(mp, "lane")
        fel.rebuild(1, F0, x[:, 1:1 + F0], mask=mask)
        assert fel.add_scan_path() == 0
        lane = _snap(torch, fel)
        # k_lfe_reset_mgr by hand (manager record zero; status, n_lines, n_entries and time of both sub-maps zero), then six calls
        fes, before_s = prepared(mp, "wave")
        st = fes.store.view(B0, rb)
        for b in np.nonzero(mask)[0]:
            st[b, :MGR] = 0
            for sub in (S, S + 1):
                o = MGR + sub * sb
                st[b, o:o + 12] = 0
                st[b, o + 16:o + 24] = 0
        for k in range(F0):
            fes.add_scan(1 + k, poses[:, k], mask=mask)
            assert fes.add_scan_path() == 1
        six = _snap(torch, fes)
    assert np.array_equal(before, before_l) and np.array_equal(before, before_s)
    assert any(_mgr(before, dims, b)["has_ref"] for b in range(B0))
    n1 = _assert_same_state(one, lane, dims, ("rebuild: one launch vs lane", n_acc))
    n2 = _assert_same_state(one, six, dims, ("rebuild: one launch vs six calls", n_acc))
    for b in range(B0):
        r0, r1 = before[b * rb:(b + 1) * rb], one[b * rb:(b + 1) * rb]
        assert np.array_equal(r0[MGR:MGR + S * sb], r1[MGR:MGR + S * sb]), ("scan slots", b)
        if not mask[b]:
            assert np.array_equal(r0, r1), ("masked robot", b)
        else:
            assert not np.array_equal(r0[:MGR], r1[:MGR]), b
    print("rebuild n_acc=%d: %d / %d sub-maps equal the lane rebuild / six single calls" % (n_acc, n1, n2))
    assert n1 == n2 == 2 * B0


# ------------------------------------------------------------------------------------------------------------------ 5
def _corridor(spacing=0.09):
    """corridor walls one, two and three metres to either side of the laser, 240 m of them in twelve stretches of 20 m with a
    doorway in the middle, as points 9 cm apart: twelve lines of about 400 cells a scan"""
    runs = []
    for y in (1.0, 2.0, 3.0, -1.0, -2.0, -3.0):
        for x0 in (-22.0, 2.0):
            xs = np.arange(x0, x0 + 20.0, spacing)
            runs.append(np.stack([xs, np.full_like(xs, y), np.zeros_like(xs)], 1))
    return np.concatenate(runs)


def test_beyond_the_wave_paths_limits(env, scen):
    liw, lp0, sc, torch = env
    lp = dict(lp0, ref_n_accumulation=4)
    F, B = 3, 3
    cor = _corridor()
    lists = [[cor] * F, scen["lists"][5][:F], scen["lists"][6][:F]]
    poses = np.stack([np.stack([[0.1 * k, 0.02 * k, 0, 0, 0, 0.01 * k] for k in range(F)]), scen["poses"][5, :F], scen["poses"][6, :F]])
    for b in range(B):
        for k in range(1, F):
            if np.array_equal(poses[b, k], poses[b, k - 1]):
                poses[b, k, 0] += 0.2
    # a: more new entries in a call than the wave holds in LDS -> the wave kernel runs, one lane builds that robot's sub-maps
    dims = _dims(B, F, max_points=cor.shape[0] + 8, max_lines=256, max_cell_entries=16384)
    w = _run(env, lp, dims, lists, poses, "wave", range(F))
    l = _run(env, lp, dims, lists, poses, "lane", range(F))
    assert w["paths"] == [1] * F and l["paths"] == [0] * F
    assert np.array_equal(w["flags"], l["flags"]) and (l["flags"] != 0).all()
    for k in range(F):
        _assert_same_state(w["snaps"][k + 1], l["snaps"][k + 1], dims, ("corridor", k))
    ref = [_hdr(slot_parts(l["snaps"][k + 1], dims, 0, F)[0]) for k in range(F)]   # ref_n_accumulation 4: sub-map 0 is the reference throughout
    print("corridor: the reference after each add (status, lines, entries) %s" % ref)
    assert all(r[0] == 0 for r in ref)
    assert ref[0][2] > NEW_CAP                                        # the fresh sub-map is beyond the LDS buffer,
    assert ref[1][2] - ref[0][2] > NEW_CAP and ref[2][2] - ref[1][2] > NEW_CAP   # and so is each accumulating call
    assert all(_mgr(l["snaps"][-1], dims, b)["status"] == 0 for b in range(B))
    # b: dimensions whose LDS need (12 bytes per held entry + 8 per line of max_lines) exceeds a work-group's -> the lane kernel
    big_lines = 6000
    assert 12 * NEW_CAP + 8 * big_lines > LDS_MAX
    dims = _dims(B, F, max_lines=big_lines, max_cell_entries=8192)
    rooms = [scen["lists"][9][:F], scen["lists"][5][:F], scen["lists"][6][:F]]
    poses[0] = scen["poses"][9, :F]
    for k in range(1, F):
        if np.array_equal(poses[0, k], poses[0, k - 1]):
            poses[0, k, 0] += 0.2
    w = _run(env, lp, dims, rooms, poses, "wave", range(F))
    l = _run(env, lp, dims, rooms, poses, "lane", range(F))
    assert w["paths"] == [0] * F and l["paths"] == [0] * F           # the default dispatch went to the lane kernel
    assert np.array_equal(w["flags"], l["flags"])
    for k in range(F + 1):
        assert np.array_equal(w["snaps"][k], l["snaps"][k]), k       # the same kernel: the same store, every byte
    assert _hdr(slot_parts(l["snaps"][-1], dims, 0, F)[0])[1] > 0


# ------------------------------------------------------------------------------------------------------------------ 6
def test_second_run_is_bit_identical(env, scen):
    liw, lp0, sc, torch = env
    lp = dict(lp0, ref_n_accumulation=4)
    B, F = 4096, 3
    src = [0, 5, 6, 9, 10, 11, R_WALL_A, R_INVALID]
    rob = np.array(src)[np.arange(B) % len(src)]
    poses = scen["poses"][rob][:, :F].copy()
    for k in range(1, F):
        same = (poses[:, k] == poses[:, k - 1]).all(1)
        poses[same, k, 0] += 0.2
    dims = _dims(B, F, max_lines=256, max_cell_entries=4096)
    P = []
    for k in range(F):
        Pk, nk = liw.laser_batch.pad_points([scen["lists"][s][k] for s in src], N_RAYS)
        nk[src.index(R_INVALID)] = N_RAYS + 1 if k == 1 else nk[src.index(R_INVALID)]
        idx = torch.from_numpy(np.arange(B) % len(src)).cuda()
        P.append((torch.from_numpy(Pk).cuda()[idx].contiguous(), torch.from_numpy(nk).cuda()[idx].contiguous()))
    dp = torch.from_numpy(poses).cuda()

    def once():
        fe = liw.laser_batch.BatchFrontEnd(lp, dims)
        fl = []
        for k in range(F):
            fe.spawn(k, *P[k])
        for k in range(F):
            fl.append(fe.add_scan(k, dp[:, k].contiguous(), flags=True))
            assert fe.add_scan_path() == 1
        torch.cuda.synchronize()
        return fe, torch.stack(fl)

    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("LIW_LFE_ADD_SCAN", raising=False)
        fe1, f1 = once()
        fe2, f2 = once()
    assert torch.equal(f1, f2) and torch.equal(fe1.store, fe2.store)
    assert (f1 != 0).all() and int((f1[2] & 1).sum()) == B
    st = sorted(set(int(fe1.status(b)) for b in range(len(src))))
    print("determinism: %d robots x %d frames, store %.2f GB, robot words %s" % (B, F, fe1.store.numel() / 1e9, st))
