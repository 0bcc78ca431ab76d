"""The localisation in a held occupancy grid (include/liw_map_locate.h) restated in numpy, and its cases: tests/test_map_locate_cases.py
guards them on the restatement alone, tests/test_gpu_map_locate.py runs them on the device.  The restatement is literal and
exhaustive: every candidate (angle, row shift, column shift) gets its score, and the best one is the first under a sort key.  numpy
float64 arithmetic rounds every product, sum and quotient on its own (no FMA), which is what the header asks for."""
import numpy as np

import map_batch_cases as mc
import map_reference as ref

RES = mc.RES
FIELD_OK, FIELD_EMPTY, FIELD_OVER = 0, 1, 2
OK, NO_MAP, NO_POINTS, BAD_PRIOR = 0, 1, 2, 3
MARGIN = 32


# ---------------------------------------------------------------------------------------------------------------- the restatement
def field_of(grid):
    """2 where grid >= 50, 1 where one of the 8 neighbours inside the grid is, 0 elsewhere; uint8 [height][width]"""
    occ = np.asarray(grid) >= 50
    h, w = occ.shape
    p = np.pad(occ, 1)
    near = np.zeros_like(occ)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                near |= p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return np.where(occ, 2, np.where(near, 1, 0)).astype(np.uint8)


def tf_of(T0, c, s, ix, iy, res):
    """T_m_l of the candidate: the table's rotation in front of R0's rows 0 and 1, the shift added to t0"""
    T0 = np.asarray(T0, dtype=np.float64)
    out = T0.copy()
    out[0:3] = c * T0[0:3] - s * T0[3:6]
    out[3:6] = s * T0[0:3] + c * T0[3:6]
    out[9] = T0[9] + float(ix) * res
    out[10] = T0[10] + float(iy) * res
    return out


def scores(field, info, pts, T0, table, W, cell=np.floor):
    """(S [n_theta][2 W + 1][2 W + 1] int64 indexed [j][iy + W][ix + W], n_valid); `cell` is the quotient -> cell rule (np.floor: the
    definition; np.trunc: the map's own rule, for the case that shows the difference)"""
    T0 = np.asarray(T0, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    h, w = field.shape
    res, ox, oy = info["resolution"], info["origin_x"], info["origin_y"]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        Qx = (T0[0] * x + T0[1] * y) + T0[2] * z
        Qy = (T0[3] * x + T0[4] * y) + T0[5] * z
        valid = np.isfinite(Qx) & np.isfinite(Qy) & (np.abs(Qx) <= 1e6) & (np.abs(Qy) <= 1e6)
    Qx, Qy = Qx[valid], Qy[valid]
    pad = 2 * MARGIN
    pf = np.zeros((h + 2 * pad, w + 2 * pad), dtype=np.int64)       # cells outside the grid count 0
    pf[pad:pad + h, pad:pad + w] = field
    ixs = np.arange(-W, W + 1)
    S = np.zeros((len(table), 2 * W + 1, 2 * W + 1), dtype=np.int64)
    for j, (c, s) in enumerate(np.asarray(table, dtype=np.float64)):
        U = c * Qx - s * Qy
        V = s * Qx + c * Qy
        cx = cell(((U + T0[9]) - ox) / res)
        cy = cell(((V + T0[10]) - oy) / res)
        inside = (cx >= -MARGIN) & (cx < w + MARGIN) & (cy >= -MARGIN) & (cy < h + MARGIN)
        cxi, cyi = cx[inside].astype(np.int64), cy[inside].astype(np.int64)
        for iy in range(-W, W + 1):
            S[j, iy + W] = pf[(cyi + iy + pad)[:, None], (cxi + pad)[:, None] + ixs[None, :]].sum(axis=0)
    return S, int(valid.sum())


def match_one(field, info, pts, T0, table, W, min_permille=0, cell=np.floor):
    """One query against one field (None: no usable map) -> dict(found, best [4], stats [4], T_m_l [12], S)"""
    T0 = np.asarray(T0, dtype=np.float64).reshape(12)
    table = np.asarray(table, dtype=np.float64).reshape(-1, 2)

    def fail(status):
        return dict(found=0, best=np.zeros(4, np.int32), stats=np.array([status, 0, 0, 0], np.int32), T_m_l=T0.copy(), S=None)
    if field is None:
        return fail(NO_MAP)
    if not np.isfinite(T0).all() or (np.abs(T0[9:12]) > 1e6).any():
        return fail(BAD_PRIOR)
    S, n_valid = scores(field, info, pts, T0, table, W, cell)
    if n_valid == 0:
        return fail(NO_POINTS)
    n_theta = len(table)
    J, IY, IX = np.meshgrid(np.arange(n_theta), np.arange(-W, W + 1), np.arange(-W, W + 1), indexing="ij")
    J, IY, IX, Sf = J.ravel(), IY.ravel(), IX.ravel(), S.ravel()
    # the sort key, last key first: score (descending), ix^2 + iy^2, |j - centre|, j, iy, ix
    first = np.lexsort((IX, IY, J, np.abs(J - (n_theta - 1) // 2), IX * IX + IY * IY, -Sf))[0]
    j, iy, ix, score = int(J[first]), int(IY[first]), int(IX[first]), int(Sf[first])
    ties = int((Sf == score).sum())
    found = int(score * 1000 >= int(min_permille) * 2 * n_valid)
    return dict(found=found, best=np.array([j, ix, iy, score], np.int32), stats=np.array([OK, n_valid, ties, 0], np.int32),
                T_m_l=tf_of(T0, table[j, 0], table[j, 1], ix, iy, info["resolution"]), S=S)


def match_rows(fields, infos, map_of, points, n_points, T0, table, W, min_permille=0):
    """Q queries: fields / infos per map (a field of None: EMPTY or OVER) -> dict(found [Q] uint8, best [Q, 4], stats [Q, 4], T_m_l [Q, 12])"""
    Q = len(map_of)
    points = np.asarray(points, dtype=np.float64)
    out = dict(found=np.zeros(Q, np.uint8), best=np.zeros((Q, 4), np.int32), stats=np.zeros((Q, 4), np.int32), T_m_l=np.zeros((Q, 12)))
    for q in range(Q):
        m = int(map_of[q])
        fld = fields[m] if 0 <= m < len(fields) else None
        n = min(max(int(n_points[q]), 0), points.shape[1])
        r = match_one(fld, infos[m] if fld is not None else None, points[q, :n], T0[q], table, W, min_permille)
        for k in out:
            out[k][q] = r[k]
    return out


def angle_table(half_width_deg, step_deg):
    """(cos, sin) of -half .. half in whole steps, as FleetLocalizer.angle_table"""
    n = int(np.floor(half_width_deg / step_deg + 1e-9))
    a = np.arange(-n, n + 1, dtype=np.float64) * np.radians(step_deg)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


# ---------------------------------------------------------------------------------------------------------------- room trials
ROOM_SEEDS = (5, 6, 7)
TRIALS = 4
ROOM_W, ROOM_STEP_DEG, ROOM_HALF_DEG = 8, 1.0, 8.0
_ROOMS = {}


def room_map(seed):
    """the map of a room trial: 6 scans of 180 rays of rooms(4)[1] from flat poses -> dict(tfs [6, 12], subs, room)"""
    if seed not in _ROOMS:
        rng = np.random.default_rng(seed)
        room = mc.rooms(4)[1]
        tfs, subs = mc.room_case(rng, 6, 180, tilt=0.0, room=room)
        _ROOMS[seed] = dict(tfs=tfs, subs=subs, room=room, rng=rng, queries=None, render=None)
    return _ROOMS[seed]


def room_render(seed):
    """the serial walk's render of the room's map (slow; once per seed)"""
    c = room_map(seed)
    if c["render"] is None:
        c["render"] = ref.render(c["tfs"], c["subs"], RES)
    return c["render"]


def room_queries(seed):
    """TRIALS queries in the room: a scan of 120 rays from a true pose and a prior off by up to 0.3 m and 6 degrees ->
    list of dict(pts [n, 3], truth (x, y, yaw), off (dx, dy, dyaw), T0 [12])"""
    c = room_map(seed)
    if c["queries"] is None:
        rng, out = c["rng"], []
        for _ in range(TRIALS):
            a = rng.uniform(-np.pi, np.pi)
            x, y, yaw = 4.0 * np.cos(a), 5.0 + 4.0 * np.sin(a), rng.uniform(-np.pi, np.pi)
            pts = mc.scan(c["room"], x, y, yaw, 120, rng)
            dx, dy, dyaw = rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), np.radians(rng.uniform(-6.0, 6.0))
            out.append(dict(pts=pts, truth=(x, y, yaw), off=(dx, dy, dyaw), T0=mc.tf12(x + dx, y + dy, yaw + dyaw)))
        c["queries"] = out
    return c["queries"]


def room_table():
    return angle_table(ROOM_HALF_DEG, ROOM_STEP_DEG)


def info_of(render):
    return {k: render[k] for k in ("width", "height", "resolution", "origin_x", "origin_y")}


def room_errors(q, best, res=RES):
    """(|x error| in cells, |y error| in cells, |yaw error| in table steps) of a best candidate against the query's truth"""
    dx, dy, dyaw = q["off"]
    j, ix, iy = int(best[0]), int(best[1]), int(best[2])
    delta = np.radians((j - int(ROOM_HALF_DEG / ROOM_STEP_DEG)) * ROOM_STEP_DEG)
    return abs(ix * res + dx) / res, abs(iy * res + dy) / res, abs(delta + dyaw) / np.radians(ROOM_STEP_DEG)


def pack_queries(queries, stride):
    """list of queries -> points [Q, stride, 3], n [Q] int32, T0 [Q, 12]"""
    Q = len(queries)
    pts, n, T0 = np.zeros((Q, stride, 3)), np.zeros(Q, np.int32), np.zeros((Q, 12))
    for k, q in enumerate(queries):
        n[k] = len(q["pts"])
        pts[k, :n[k]] = q["pts"]
        T0[k] = q["T0"]
    return pts, n, T0


# ---------------------------------------------------------------------------------------------------------------- hand-made cases
def hand_info(w, h, ox=0.0, oy=0.0, res=RES):
    return dict(width=w, height=h, resolution=res, origin_x=ox, origin_y=oy)


def cell_points(cells, ox=0.0, oy=0.0, res=RES, frac=0.5):
    """laser-frame points (z = 0) at the fraction `frac` of the cells (x, y), for an identity prior"""
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    return np.stack([ox + (c[:, 0] + frac) * res, oy + (c[:, 1] + frac) * res, np.zeros(len(c))], axis=1)


IDENT = mc.tf12(0.0, 0.0, 0.0)


def tie_case():
    """One wall along x through the whole grid, a scan of 20 points on a line parallel to it, two rows above: every column shift
    of the best row ties, and the shortest shift wins.  -> dict(grid, info, pts, T0, table, W, want_best, want_ties)"""
    w, h, W = 80, 24, 5
    grid = np.zeros((h, w), np.int8)
    grid[10, :] = 100
    pts = cell_points([(30 + k, 12) for k in range(20)])
    return dict(grid=grid, info=hand_info(w, h), pts=pts, T0=IDENT.copy(), table=np.array([[1.0, 0.0]]), W=W,
                want_best=(0, 0, -2, 40), want_ties=2 * W + 1)


def edge_case():
    """A 12 x 9 grid whose border cells are all occupied, at an origin that is no multiple of the resolution, and a cross of
    points that leaves it on every side, past the margin of 32 cells too.  Six of the points sit a quarter or half a cell OUTSIDE
    the left column and the bottom row (four extra ones, and one of either arm of the cross): quotients in (-1, 0), which floor
    puts outside (cell -1) and truncation into the border.  W = 0, one angle."""
    w, h = 12, 9
    ox, oy = -0.31, 0.17
    grid = np.zeros((h, w), np.int8)
    grid[0, :] = grid[-1, :] = 50
    grid[:, 0] = grid[:, -1] = 100
    cross = [(x, 4) for x in range(-40, 50, 3)] + [(5, y) for y in range(-40, 50, 3)]
    pts = np.concatenate([cell_points(cross, ox, oy), cell_points([(-1, 3), (-1, 5), (4, -1), (7, -1)], ox, oy, frac=0.75)])
    return dict(grid=grid, info=hand_info(w, h, ox, oy), pts=pts, T0=IDENT.copy(), table=np.array([[1.0, 0.0]]), W=0)


def threshold_case():
    """10 valid points, 7 on a wall (2 each) and 3 in free space: the score is 14 of 20, so min_permille = 700 is met exactly and
    701 is not.  W = 0, one angle."""
    w, h = 20, 20
    grid = np.zeros((h, w), np.int8)
    grid[5, 2:9] = 50
    pts = cell_points([(x, 5) for x in range(2, 9)] + [(3, 15), (9, 15), (15, 15)])
    return dict(grid=grid, info=hand_info(w, h), pts=pts, T0=IDENT.copy(), table=np.array([[1.0, 0.0]]), W=0, score=14, n_valid=10,
                permille=700)


# ---------------------------------------------------------------------------------------------------------------- joining a group
GROUP_SEED = 21
GROUP_W, GROUP_STEP_DEG, GROUP_HALF_DEG = 8, 1.0, 8.0
_GROUP = {}


def yaw_then(T, dyaw, dx, dy):
    """the transform T turned by dyaw about its own origin (a rotation about z in front of R) and moved by (dx, dy)"""
    T = np.asarray(T, dtype=np.float64)
    c, s = np.cos(dyaw), np.sin(dyaw)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.concatenate([(Rz @ T[:9].reshape(3, 3)).reshape(9), T[9:] + np.array([dx, dy, 0.0])])


def yaw_of(T):
    return float(np.arctan2(T[3], T[0]))


def group_case():
    """map_group_cases.shared_room with sub-map counts [6, 1]: robot 0 has mapped the room, robot 1 holds one scan and joins.
    -> the room's dict with T_g_l_true [12] of robot 1's scan and the prior T0 [12], off by a few cells and degrees"""
    import map_group_cases as gc
    if not _GROUP:
        rng = np.random.default_rng(GROUP_SEED)
        c = gc.shared_room(rng, [6, 1])
        true = gc.mul12(c["T_g_w"][1], c["tfs_of"][1][0])
        off = (rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), np.radians(rng.uniform(-5.0, 5.0)))
        _GROUP.update(c, T_g_l_true=true, off=off, T0=yaw_then(true, off[2], off[0], off[1]), table=angle_table(GROUP_HALF_DEG, GROUP_STEP_DEG))
    return _GROUP


def group_errors(T_m_l, true, res=RES):
    """(|x|, |y| error of the laser origin in cells, |yaw| error in table steps) of a found map <- laser transform"""
    d = np.asarray(T_m_l)[9:11] - np.asarray(true)[9:11]
    dyaw = (yaw_of(T_m_l) - yaw_of(true) + np.pi) % (2 * np.pi) - np.pi
    return abs(d[0]) / res, abs(d[1]) / res, abs(dyaw) / np.radians(GROUP_STEP_DEG)


# ---------------------------------------------------------------------------------------------------------------- hand-made sources
def make_source(grids, infos, max_cells):
    """M hand-made source regions in one uint8 array: a liw_map_info at byte 32 and the int8 grid at grid_off = 256 of each ->
    (bytes [M * region_bytes] uint8, region_bytes, grid_off)"""
    grid_off = 256
    region_bytes = (grid_off + max(max_cells, max(g.size for g in grids)) + 255) // 256 * 256
    buf = np.zeros(len(grids) * region_bytes, np.uint8)
    for m, (g, i) in enumerate(zip(grids, infos)):
        base = m * region_bytes
        buf[base + 32:base + 40] = np.array([i["width"], i["height"]], np.int32).view(np.uint8)
        buf[base + 40:base + 64] = np.array([i["resolution"], i["origin_x"], i["origin_y"]], np.float64).view(np.uint8)
        buf[base + grid_off:base + grid_off + g.size] = np.ascontiguousarray(g, dtype=np.int8).reshape(-1).view(np.uint8)
    return buf, region_bytes, grid_off
