"""Localisation of fleet robots in a held occupancy grid on the MI355X (include/liw_map_locate.h).  Every comparison with the numpy
restatement of tests/map_locate_cases.py is exact: np.array_equal on the field's bytes and counts and on found, best and stats, and
T_m_l bit for bit.  The restatement is fed the grids read back from the device, so that it answers for the search alone; the grids
have their own tests (test_gpu_map_batch.py, test_gpu_map_group.py)."""
import ctypes as C

import numpy as np
import pytest

import map_batch_cases as mc
import map_group_cases as gc
import map_locate_cases as lc
import map_reference as ref

pytestmark = pytest.mark.gpu
RES = mc.RES
LIW_EINVAL = -22
SENT = 0x5A


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _host(out):
    """host copies of a match's outputs"""
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _same(got, want):
    for k in ("found", "best", "stats"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert got["T_m_l"].tobytes() == np.ascontiguousarray(want["T_m_l"]).tobytes()


def _guards(o):
    return o.guard >= 64 and bool((o._buf[:o.guard] == 0xA5).all()) and bool((o._buf[-o.guard:] == 0xA5).all())


def _assert_field(loc, m, grid, info):
    want = lc.field_of(grid)
    got = loc.field(m)
    assert got.shape == want.shape and np.array_equal(got, want)
    fi = loc.field_info(m)
    assert (fi["status"], fi["occupied"], fi["near"]) == (lc.FIELD_OK, int((want == 2).sum()), int((want == 1).sum()))
    for k in ("width", "height", "resolution", "origin_x", "origin_y"):
        assert fi[k] == info[k]
    return want


# ------------------------------------------------------------------------------------------------------------------ the real sources
_REAL = {}
GROUP_OF = [1, 2, 0]      # robot b's grid is group GROUP_OF[b]'s


def _real(liw, synth):
    """one FleetMapper with the maps of the three room seeds and one FleetGroupMap holding the same grids under other indices;
    rendered once, shared and left unchanged"""
    if not _REAL:
        cells = 1 << 17
        maps = [lc.room_map(s) for s in lc.ROOM_SEEDS]
        fm = mc.mapper(liw, synth, 3, 6, 6 * 180, cells, 2048)
        mc.load(fm, [c["subs"] for c in maps])
        T = mc.pad_tfs([c["tfs"] for c in maps], 6)
        fm.render_tf(T)
        assert fm.status.cpu().tolist() == [0, 0, 0]
        gm = liw.FleetGroupMap(fm, 3, cells, guard=64)
        gm.render_tf(T, np.array(GROUP_OF, np.int32))
        assert gm.gstatus.cpu().tolist() == [0, 0, 0]
        grids = [fm.grid(b) for b in range(3)]
        infos = [fm.info_of(b) for b in range(3)]
        queries = [q for s in lc.ROOM_SEEDS for q in lc.room_queries(s)]
        _REAL.update(fm=fm, gm=gm, grids=grids, infos=infos, fields=[lc.field_of(g) for g in grids], queries=queries,
                     seed_of=np.repeat(np.arange(3), lc.TRIALS).astype(np.int32))
    return _REAL


def test_field_of_real_sources(liw, synth):
    r = _real(liw, synth)
    fm, gm = r["fm"], r["gm"]
    before = fm._buf.cpu().numpy().copy(), gm._buf.cpu().numpy().copy()
    loc = liw.FleetLocalizer(fm, 4, guard=64)
    assert [loc.field_info(m)["status"] for m in range(3)] == [lc.FIELD_EMPTY] * 3 and loc.field(0).shape == (0, 0)
    loc.build()
    for b in range(3):
        assert r["grids"][b].shape[0] > 200
        _assert_field(loc, b, r["grids"][b], r["infos"][b])
        assert loc.device_field(b) == loc.store.data_ptr() + b * loc.lay["map_bytes"] + loc.lay["field_off"]
    gloc = liw.FleetLocalizer(gm, 4, guard=64)
    gloc.build()
    for b in range(3):
        assert np.array_equal(gm.grid(GROUP_OF[b]), r["grids"][b])
        _assert_field(gloc, GROUP_OF[b], r["grids"][b], r["infos"][b])
    # equal grids leave equal regions, whichever source and index they came from
    a, g = loc.map_regions().cpu().numpy(), gloc.map_regions().cpu().numpy()
    assert all(a[b].tobytes() == g[GROUP_OF[b]].tobytes() for b in range(3))
    # the sources are only read
    assert fm._buf.cpu().numpy().tobytes() == before[0].tobytes() and gm._buf.cpu().numpy().tobytes() == before[1].tobytes()
    assert _guards(loc) and _guards(gloc)
    loc.close()
    gloc.close()


# ------------------------------------------------------------------------------------------------------------------ hand-made sources
def _hand_grids():
    rng = np.random.default_rng(3)
    border = np.zeros((9, 21), np.int8)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = 100
    corners = np.full((7, 18), -1, np.int8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 50
    rand = lambda h, w: rng.choice(np.array([-1, 0, 49, 50, 100], np.int8), size=(h, w), p=[0.3, 0.5, 0.05, 0.1, 0.05])
    return [np.array([[100]], np.int8), np.array([[0]], np.int8), rand(70, 3), rand(3, 70), border, corners, rand(13, 17), rand(31, 33), rand(40, 5),
            rand(50, 47)]


def _hand_source(liw, grids, max_cells, extra_infos=()):
    """a hand-made source on the device with one region per grid and one grid-less region per extra info -> (dict for FleetLocalizer,
    infos, the device tensor with 64 guard bytes on either side)"""
    import torch
    infos = [lc.hand_info(g.shape[1], g.shape[0], 0.25 * m, -0.5 * m) for m, g in enumerate(grids)] + list(extra_infos)
    blank = [np.zeros((0, 0), np.int8)] * len(extra_infos)
    buf, region_bytes, grid_off = lc.make_source(list(grids) + blank, infos, max_cells)
    t = torch.full((len(buf) + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    t[64:-64] = _dev(buf)
    return dict(store=t[64:-64], M=len(infos), region_bytes=region_bytes, grid_off=grid_off, max_cells=max_cells), infos, t


def test_field_of_hand_made_sources(liw, synth):
    grids = _hand_grids()
    max_cells = 50 * 47
    assert all(g.size <= max_cells for g in grids) and sum(g.shape[1] % 16 != 0 for g in grids) >= 8
    n = len(grids)
    src, infos, raw = _hand_source(liw, grids, max_cells, [lc.hand_info(0, 0), lc.hand_info(0, 7), lc.hand_info(50, 48), lc.hand_info(1 << 20, 1 << 20)])
    M = src["M"]
    assert M == n + 4 and infos[n + 2]["width"] * infos[n + 2]["height"] == max_cells + 50
    snap_src = raw.cpu().numpy().copy()
    loc = liw.FleetLocalizer(src, 2, guard=64)
    loc.build()
    for m, g in enumerate(grids):
        _assert_field(loc, m, g, infos[m])
    want_status = [lc.FIELD_EMPTY, lc.FIELD_EMPTY, lc.FIELD_OVER, lc.FIELD_OVER]
    for k in range(4):
        fi = loc.field_info(n + k)
        assert (fi["status"], fi["occupied"], fi["near"], fi["width"], fi["height"]) == (want_status[k], 0, 0, infos[n + k]["width"], infos[n + k]["height"])
        assert loc.field(n + k).shape == (0, 0)
    first = loc.map_regions().cpu().numpy().copy()
    fo = loc.lay["field_off"]
    assert not first[n + 2][fo:].any()                                 # OVER: no field
    # a second build: the maps move to other sources; map 3 is not selected; map 4 gets the OVER source, map 5 none, map 6 the 0 x 0 one
    src_of = np.roll(np.arange(M), 1).astype(np.int32)
    src_of[4], src_of[5], src_of[6] = n + 2, -1, n
    msel = np.ones(M, np.uint8)
    msel[3] = 0
    loc.build(src_of=src_of, msel=msel)
    second = loc.map_regions().cpu().numpy().copy()
    assert second[3].tobytes() == first[3].tobytes()                   # not selected: no byte
    for m in (1, 2, 7, 8, 9):
        _assert_field(loc, m, grids[src_of[m]], infos[src_of[m]])
    for m, st in ((4, lc.FIELD_OVER), (5, lc.FIELD_EMPTY), (6, lc.FIELD_EMPTY)):
        assert second[m][fo:].tobytes() == first[m][fo:].tobytes()     # no field byte is written
        assert second[m][:12].view(np.int32).tolist() == [st, 0, 0]
    assert not second[5][32:112].any() and second[4][32:112].tobytes() == first[n + 2][32:112].tobytes()
    assert raw.cpu().numpy().tobytes() == snap_src.tobytes() and _guards(loc)
    loc.close()


# ------------------------------------------------------------------------------------------------------------------ the room trials
@pytest.mark.parametrize("source", ["mapper", "group"])
def test_room_trials(liw, synth, source):
    r = _real(liw, synth)
    Q = len(r["queries"])
    loc = liw.FleetLocalizer(r["fm"] if source == "mapper" else r["gm"], Q, max_theta=17, guard=64)
    loc.build()
    map_of = r["seed_of"] if source == "mapper" else np.array(GROUP_OF, np.int32)[r["seed_of"]]
    fields, infos = [None] * 3, [None] * 3
    for b in range(3):
        m = b if source == "mapper" else GROUP_OF[b]
        fields[m], infos[m] = r["fields"][b], r["infos"][b]
    pts, n, T0 = lc.pack_queries(r["queries"], 120)
    table = lc.room_table()
    assert np.array_equal(loc.angle_table(np.radians(lc.ROOM_HALF_DEG), np.radians(lc.ROOM_STEP_DEG)), table)
    if "want" not in r:
        r["want"] = lc.match_rows(r["fields"], r["infos"], r["seed_of"], pts, n, T0, table, lc.ROOM_W, 600)
    got = _host(loc.match(map_of, pts, n, T0, table, lc.ROOM_W, min_permille=600))
    _same(got, r["want"])
    assert 0 < got["found"].sum() < Q                                   # the threshold splits the trials
    for k, q in enumerate(r["queries"]):
        assert max(lc.room_errors(q, got["best"][k])) <= 1.0 and got["stats"][k].tolist()[::2] == [lc.OK, 1]
    r["last_" + source] = got
    assert _guards(loc)
    loc.close()


# ------------------------------------------------------------------------------------------------------------------ the hand-made cases
_HAND = {}


def _hand(liw):
    """one hand-made source: the tie, edge and threshold grids, a 0 x 0 region and one that is too large; rows of every kind"""
    if not _HAND:
        rng = np.random.default_rng(9)
        tie, edge, thr = lc.tie_case(), lc.edge_case(), lc.threshold_case()
        grids = [tie["grid"], edge["grid"], thr["grid"]]
        max_cells = 80 * 24
        src, infos, raw = _hand_source(liw, grids, max_cells, [lc.hand_info(0, 0), lc.hand_info(50, 50)])
        infos[0], infos[1], infos[2] = tie["info"], edge["info"], thr["info"]
        buf, _, _ = lc.make_source(grids + [np.zeros((0, 0), np.int8)] * 2, infos, max_cells)
        raw[64:-64] = _dev(buf)
        stride = 700
        many = np.stack([rng.uniform(-1.0, 5.0, stride), rng.uniform(-1.0, 2.2, stride), rng.uniform(-0.2, 0.2, stride)], axis=1)
        odd = np.array([[np.nan, 0.2, 0.0], [0.5, np.inf, 0.0], [2e6, 0.1, 0.0]])
        rows = [(0, tie["pts"], tie["T0"]), (1, edge["pts"], edge["T0"]), (2, thr["pts"], thr["T0"]),
                (0, many, mc.tf12(0.3, 0.1, 0.2, 0.05, 0.02, -0.03)),              # 700 points: two LDS chunks, a tilted prior
                (2, np.zeros((0, 3)), lc.IDENT), (2, np.concatenate([odd, thr["pts"]]), lc.IDENT), (2, odd, lc.IDENT),
                (-1, thr["pts"], lc.IDENT), (3, thr["pts"], lc.IDENT), (4, thr["pts"], lc.IDENT), (5, thr["pts"], lc.IDENT),
                (2, thr["pts"], np.where(np.arange(12) == 1, np.inf, lc.IDENT)), (2, thr["pts"], np.where(np.arange(12) == 10, -1.5e6, lc.IDENT)),
                (1, many[:300], mc.tf12(-0.2, 0.3, -2.0))]
        Q = len(rows)
        pts, n, T0 = np.zeros((Q, stride, 3)), np.zeros(Q, np.int32), np.zeros((Q, 12))
        for k, (_, p, T) in enumerate(rows):
            n[k] = len(p)
            pts[k, :n[k]] = p
            T0[k] = T
        pts[4, :10] = thr["pts"]      # behind a count of 0
        n[4] = -3                     # reads as 0
        n[3] = 9999                   # reads as the stride
        _HAND.update(src=src, raw=raw, fields=[lc.field_of(g) for g in grids] + [None, None], infos=infos, map_of=np.array([r[0] for r in rows], np.int32),
                     pts=pts, n=n, T0=T0, Q=Q, tie=tie, edge=edge, thr=thr)
    return _HAND


def _hand_want(h, table, W, permille=0):
    return lc.match_rows(h["fields"], h["infos"], h["map_of"], h["pts"], h["n"], h["T0"], table, W, permille)


def _hand_loc(liw, h, max_theta=64):
    loc = liw.FleetLocalizer(h["src"], h["Q"], max_theta=max_theta, guard=64)
    loc.build()
    assert [loc.field_info(m)["status"] for m in range(5)] == [0, 0, 0, lc.FIELD_EMPTY, lc.FIELD_OVER]
    return loc


@pytest.mark.parametrize("n_theta,W", [(1, 0), (1, 5), (17, 8), (64, 2), (3, 31)])
def test_hand_made_rows(liw, synth, n_theta, W):
    h = _hand(liw)
    loc = _hand_loc(liw, h)
    a = (np.arange(n_theta) - (n_theta - 1) // 2) * np.radians(1.5)
    table = np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))
    want = _hand_want(h, table, W)
    got = _host(loc.match(h["map_of"], h["pts"], h["n"], h["T0"], table, W))
    _same(got, want)
    S = lc.OK, lc.NO_MAP, lc.NO_POINTS, lc.BAD_PRIOR
    assert got["stats"][:, 0].tolist() == [S[0]] * 4 + [S[2], S[0], S[2]] + [S[1]] * 4 + [S[3]] * 2 + [S[0]]
    assert got["stats"][3, 1] == 700 and got["stats"][5, 1] == 10
    assert got["found"].tolist() == [1, 1, 1, 1, 0, 1] + [0] * 7 + [1]
    assert got["T_m_l"][11].tobytes() == h["T0"][11].tobytes()         # a non-finite prior comes back bit for bit
    if (n_theta, W) == (1, 5):      # every ix of the best row ties, and the shortest shift wins
        assert tuple(got["best"][0]) == h["tie"]["want_best"] and got["stats"][0, 2] == h["tie"]["want_ties"] > 1
    if (n_theta, W) == (1, 0):      # the quotients in (-1, 0) are outside: truncation would score 12 more
        trunc = lc.match_one(h["fields"][1], h["infos"][1], h["edge"]["pts"], h["edge"]["T0"], table, 0, cell=np.trunc)
        assert got["best"][1, 3] == 4 and trunc["best"][3] == 16
    assert _guards(loc)
    loc.close()


def test_threshold_and_masked_rows(liw, synth):
    import torch
    h = _hand(liw)
    loc = _hand_loc(liw, h, max_theta=1)
    table = np.array([[1.0, 0.0]])
    p = h["thr"]["permille"]
    at = _host(loc.match(h["map_of"], h["pts"], h["n"], h["T0"], table, 0, min_permille=p))
    _same(at, _hand_want(h, table, 0, p))
    assert at["found"][2] == 1 and at["best"][2, 3] * 1000 == p * 2 * at["stats"][2, 1]          # met exactly
    # one above, on the rows of a mask: the other rows keep every byte, their scratch included
    for t in (loc.found, loc.best, loc.stats):
        t.fill_(SENT)
    loc.T_m_l.fill_(-7.25)
    mask = (np.arange(h["Q"]) % 3 != 1).astype(np.uint8)
    assert mask[2] == 1 and mask[1] == 0 and mask[7] == 0
    rows = lambda: loc.store[loc.lay["partial_off"]:].view(h["Q"], loc.lay["row_bytes"]).cpu().numpy().copy()
    torch.cuda.synchronize()
    scratch = rows()
    maps = loc.map_regions().cpu().numpy().copy()
    above = _host(loc.match(h["map_of"], h["pts"], h["n"], h["T0"], table, 0, min_permille=p + 1, mask=mask))
    want = _hand_want(h, table, 0, p + 1)
    on = mask != 0
    _same({k: v[on] for k, v in above.items()}, {k: v[on] for k, v in want.items()})
    assert above["found"][2] == 0 and above["best"][2].tolist() == at["best"][2].tolist()
    assert (above["found"][~on] == SENT).all() and (above["best"][~on] == SENT).all() and (above["stats"][~on] == SENT).all()
    assert (above["T_m_l"][~on] == -7.25).all()
    after = rows()
    assert after[~on].tobytes() == scratch[~on].tobytes() and loc.map_regions().cpu().numpy().tobytes() == maps.tobytes()
    assert _guards(loc)
    loc.close()


def test_tiled_copies_and_a_second_run(liw, synth):
    """32 copies of three queries at other query indices, against four maps built from one source region: every copy's rows are
    byte-equal, and a second run leaves the same store and outputs"""
    h = _hand(liw)
    base = [0, 3, 13]
    reps = 32
    Q = reps * len(base)
    M = 4
    src = dict(h["src"], M=M)
    loc = liw.FleetLocalizer(src, Q, max_theta=17, guard=64)
    table = lc.angle_table(12.0, 1.5)
    runs = []
    for src_region in (0, 1):
        loc.build(src_of=np.full(M, src_region, np.int32))
        idx = np.array([base[k % 3] for k in range(Q)])
        map_of = (np.arange(Q) // 3 % M).astype(np.int32)
        args = (map_of, h["pts"][idx], h["n"][idx], h["T0"][idx], table, 6)
        one = _host(loc.match(*args))
        store = loc.store.cpu().numpy().copy()
        two = _host(loc.match(*args))
        assert all(one[k].tobytes() == two[k].tobytes() for k in one) and loc.store.cpu().numpy().tobytes() == store.tobytes()
        want = lc.match_rows([h["fields"][src_region]], [h["infos"][src_region]], np.zeros(3, np.int32), h["pts"][base], h["n"][base], h["T0"][base], table, 6)
        for k in one:
            assert all(one[k][3 * c:3 * c + 3].tobytes() == np.ascontiguousarray(want[k]).tobytes() for c in range(reps)), k
        regs = loc.map_regions().cpu().numpy()
        assert all(regs[m].tobytes() == regs[0].tobytes() for m in range(M))
        runs.append(one)
    assert runs[0]["best"].tobytes() != runs[1]["best"].tobytes()
    loc.close()


# ------------------------------------------------------------------------------------------------------------------ bad calls
def test_bad_calls_write_nothing(liw, synth):
    import torch
    h = _hand(liw)
    loc = _hand_loc(liw, h, max_theta=8)
    for t in (loc.found, loc.best, loc.stats):
        t.fill_(SENT)
    for t in (loc.T_m_l, loc.T_w_l, loc.T_g_w):
        t.fill_(-7.25)
    torch.cuda.synchronize()
    outs = (loc.found, loc.best, loc.stats, loc.T_m_l, loc.T_w_l, loc.T_g_w)
    snap = [loc._buf.cpu().numpy().copy(), h["raw"].cpu().numpy().copy()] + [t.cpu().numpy().copy() for t in outs]
    L, hd = loc.L, loc.h
    vp = lambda t: C.c_void_p(t.data_ptr())
    Q = h["Q"]
    ls, ss = vp(loc.store), vp(h["src"]["store"])
    mis, smis = C.c_void_p(loc.store.data_ptr() + 4), C.c_void_p(h["src"]["store"].data_ptr() + 4)
    rb, go = h["src"]["region_bytes"], h["src"]["grid_off"]
    so = torch.zeros(5, dtype=torch.int32, device="cuda")
    build = lambda **k: L.liw_floc_build(hd, k.get("ls", ls), k.get("ss", ss), k.get("rb", rb), k.get("go", go), k.get("so", vp(so)), None, None)
    mo, pts, n, T0, tab = _dev(h["map_of"]), _dev(h["pts"]), _dev(h["n"]), _dev(h["T0"]), _dev(lc.angle_table(6.0, 1.5))
    assert tab.shape[0] == 9      # one more than max_theta
    base = dict(ls=ls, mo=vp(mo), pts=vp(pts), stride=700, n=vp(n), T0=vp(T0), tab=vp(tab), nt=8, W=4, mp=0, found=vp(loc.found), best=vp(loc.best),
                stats=vp(loc.stats), T=vp(loc.T_m_l))

    def match(**k):
        a = dict(base, **k)
        return L.liw_floc_match(hd, a["ls"], a["mo"], a["pts"], a["stride"], a["n"], a["T0"], a["tab"], a["nt"], a["W"], a["mp"], None, a["found"], a["best"],
                                a["stats"], a["T"], None)
    poses = torch.zeros(Q, 6, dtype=torch.float64, device="cuda")
    lbase = dict(T=vp(loc.T_m_l), poses=vp(poses), stride=6, found=vp(loc.found), Tw=vp(loc.T_w_l), Tg=vp(loc.T_g_w))

    def link(**k):
        a = dict(lbase, **k)
        return L.liw_floc_link_tf(hd, a["T"], a["poses"], a["stride"], a["found"], None, a["Tw"], a["Tg"], None)
    calls = [lambda: build(ls=None), lambda: build(ls=mis), lambda: build(ss=None), lambda: build(ss=smis), lambda: build(so=None),
             lambda: build(rb=104), lambda: build(rb=rb + 4), lambda: build(go=111), lambda: build(go=rb), lambda: build(go=rb + 256)]
    calls += [lambda k=k: match(**{k: None}) for k in ("ls", "mo", "pts", "n", "T0", "tab", "found", "best", "stats", "T")]
    calls += [lambda: match(ls=mis), lambda: match(stride=0), lambda: match(stride=-1), lambda: match(stride=(1 << 20) + 1), lambda: match(nt=0),
              lambda: match(nt=9), lambda: match(nt=-1), lambda: match(W=-1), lambda: match(W=32), lambda: match(mp=-1)]
    calls += [lambda k=k: link(**{k: None}) for k in ("T", "poses", "found", "Tw", "Tg")] + [lambda: link(stride=-1)]
    for k, call in enumerate(calls):
        assert call() == LIW_EINVAL, k
    for m in (-1, 5):
        assert L.liw_floc_field_info(hd, ls, m, None, None, None, None) == LIW_EINVAL and L.liw_floc_get_field(hd, ls, m, None, 0) == LIW_EINVAL
        assert L.liw_floc_device_field(hd, ls, m) is None
    assert L.liw_floc_field_info(hd, None, 0, None, None, None, None) == LIW_EINVAL and L.liw_floc_get_field(hd, ls, 0, None, 5) == LIW_EINVAL
    torch.cuda.synchronize()
    now = [loc._buf.cpu().numpy(), h["raw"].cpu().numpy()] + [t.cpu().numpy() for t in outs]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(now, snap))
    # and the same calls with good arguments succeed
    assert build() == 0 and match() == 0 and link() == 0
    torch.cuda.synchronize()
    loc.close()


# ------------------------------------------------------------------------------------------------------------------ link_tf
def _lie_inverse(liw, A):
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    A = np.ascontiguousarray(A, dtype=np.float64)
    out = np.zeros(12)
    liw.lib().liw_lie_inverse(pd(A), pd(out))
    return out


def test_link_tf(liw, synth):
    r = _real(liw, synth)
    rng = np.random.default_rng(12)
    prm = synth.office_params()
    Q = len(r["queries"])
    loc = liw.FleetLocalizer(r["fm"], Q, max_theta=17, prm=prm)
    loc.build()
    pts, n, T0 = lc.pack_queries(r["queries"], 120)
    m = _host(loc.match(r["seed_of"], pts, n, T0, lc.room_table(), lc.ROOM_W, min_permille=600))
    found = m["found"] != 0
    assert 0 < found.sum() < Q
    poses = np.zeros((Q, 6))
    for q in range(Q):
        poses[q] = [rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-3, 3)]
    loc.T_w_l.fill_(-7.25)
    loc.T_g_w.fill_(-7.25)
    mask = np.ones(Q, np.uint8)
    off = int(np.flatnonzero(found)[0])
    mask[off] = 0                          # a found row that the mask leaves out
    out = _host(loc.link_tf(poses, mask=mask))
    want_w = mc.host_tf(liw, poses, mc.til12(liw, prm))
    written = found & (mask != 0)
    assert written.sum() >= 1
    worst = mc.ulps(out["T_w_l"][written], want_w[written])
    print("device make_tf * T_imu_to_laser against the host's: %.2f ulp at most" % worst)
    assert worst <= 4.0
    for q in np.flatnonzero(written):
        want = gc.lie_mul(liw, m["T_m_l"][q], _lie_inverse(liw, out["T_w_l"][q]))
        assert out["T_g_w"][q].tobytes() == want.tobytes()
        # and it does what it is for: it carries the robot's laser pose onto the found one (liw_lie_inverse transposes, and the
        # office extrinsic's rotation is orthonormal to about 1e-7 only)
        assert np.allclose(gc.mul12(out["T_g_w"][q], out["T_w_l"][q]), m["T_m_l"][q], atol=1e-6)
    assert (out["T_w_l"][~written] == -7.25).all() and (out["T_g_w"][~written] == -7.25).all()
    # without a mask the left-out row is written too
    out = _host(loc.link_tf(poses))
    assert out["T_g_w"][off].tobytes() == gc.lie_mul(liw, m["T_m_l"][off], _lie_inverse(liw, out["T_w_l"][off])).tobytes()
    loc.close()


# ------------------------------------------------------------------------------------------------------------------ end to end
def _pose_of(T12, Til12):
    """the IMU pose (p, rotation vector) whose make_tf(p, q) * T_imu_to_laser is T12 (numpy: good to an ulp or so)"""
    T = gc.mul12(T12, gc.inv12(Til12))
    R = T[:9].reshape(3, 3)
    ang = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2.0 * np.sin(ang))
    return np.concatenate([T[9:], axis * ang])


def test_a_robot_joins_a_group(liw, synth):
    import torch
    c = lc.group_case()
    prm = synth.office_params()
    Til = mc.til12(liw, prm)
    B, K, cells = 2, 6, 1 << 17
    fm = mc.mapper(liw, synth, B, K, K * 90, cells, 2048, prm=prm)
    mc.load(fm, c["subs_of"])
    poses = np.zeros((B, K, 6))
    for b in range(B):
        for k, T in enumerate(c["tfs_of"][b]):
            poses[b, k] = _pose_of(T, Til)
    poses_d = _dev(poses)
    gm = liw.FleetGroupMap(fm, 1, cells)
    T_g_w = c["T_g_w"].copy()
    gm.render(poses_d, np.array([0, -1], np.int32), T_g_w)                 # robot 0 alone has mapped the room
    assert gm.gstatus.cpu().tolist() == [0] and gm.members(0) == (1, 6)
    loc = liw.FleetLocalizer(gm, B, max_theta=17, prm=prm)
    scan = np.zeros((B, 90, 3))
    n1 = len(c["subs_of"][1][0])
    scan[1, :n1] = c["subs_of"][1][0]
    args = [_dev(a) for a in (np.array([0, 0], np.int32), scan, np.array([0, n1], np.int32), np.stack([lc.IDENT, c["T0"]]), c["table"],
                              np.array([0, 1], np.uint8), poses[:, 0])]
    torch.cuda.synchronize()
    reads = []
    for name in ("_sync", "field", "field_info"):
        setattr(loc, name, (lambda real, name: lambda *a, **k: reads.append(name) or real(*a, **k))(getattr(loc, name), name))
    loc.build()
    loc.match(args[0], args[1], args[2], args[3], args[4], lc.GROUP_W, min_permille=300, mask=args[5])
    link = loc.link_tf(args[6])
    assert not reads                                                        # no device -> host copy in build, match or link_tf
    m = _host(dict(found=loc.found, best=loc.best, stats=loc.stats, T_m_l=loc.T_m_l))
    # the search itself, against the restatement on the group's grid
    info = gm.info_of(0)
    want = lc.match_one(lc.field_of(gm.grid(0)), info, scan[1, :n1], c["T0"], c["table"], lc.GROUP_W, 300)
    assert m["found"][1] == want["found"] == 1 and np.array_equal(m["best"][1], want["best"]) and np.array_equal(m["stats"][1], want["stats"])
    assert m["T_m_l"][1].tobytes() == want["T_m_l"].tobytes() and not m["T_m_l"][0].any()
    # the found T_g_w of robot 1 against the case's
    found = link["T_g_w"].cpu().numpy()[1]
    T_w_l1 = link["T_w_l"].cpu().numpy()[1]
    ex, ey, et = lc.group_errors(gc.mul12(found, T_w_l1), gc.mul12(c["T_g_w"][1], T_w_l1))
    print("joining robot: best %s, laser origin off by %.2f %.2f cells, yaw by %.2f table steps" % (m["best"][1].tolist(), ex, ey, et))
    assert ex <= 1.0 and ey <= 1.0 and et <= 1.0
    # the merged map with the found transform
    T_g_w[1] = found
    gm.render(poses_d, np.array([0, 0], np.int32), T_g_w)
    assert gm.gstatus.cpu().tolist() == [0] and gm.members(0) == (2, 7)
    rows = gm.infos()
    gc.assert_group(gm, 0, ref.render(*gc.concat([fm.tf(b) for b in range(B)], c["subs_of"], [0, 1]), RES), rows[0])
    for o in (loc, gm, fm):
        o.close()
