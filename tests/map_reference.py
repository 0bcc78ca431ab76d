"""The occupancy-grid map as a literal serial walk (checker only; nothing in the product uses it), written from the
semantics of reference src/utilies/visualization.cpp:33-75 and :369-451 as include/liw_map.h states them: world points with
the sum order ((R0 x + R1 y) + R2 z) + t, the bounding box, and per ray `for (tr = 0; tr <= len; tr += step)` with an
ACCUMULATED tr, a division by the resolution and a conversion that truncates toward zero.  Plain Python floats: IEEE double,
every operation rounded on its own, no BLAS and no FMA.  Slow: for small cases (tests/cpp/map_serial.cpp is the same walk
in C++ for large ones, and build_serial() / render_serial() here compile and call it)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def world_point(T, pt):
    x, y, z = float(pt[0]), float(pt[1]), float(pt[2])
    return [((T[3 * i] * x + T[3 * i + 1] * y) + T[3 * i + 2] * z) + T[9 + i] for i in range(3)]


def step_table(res, n):
    step = res / 2
    out, tr = [], 0.0
    for _ in range(n):
        out.append(tr)
        tr += step
    return np.array(out)


def _cell(cx, cy, ox, oy, res, w, h):
    x = int((cx - ox) / res)   # int() truncates toward zero
    y = int((cy - oy) / res)
    if x < 0 or x >= w or y < 0 or y >= h:
        return -1
    return y * w + x


def render(tfs, subs, res=0.05):
    """tfs: [K][12] world <- laser (R row-major, t); subs: K arrays [n][3] of laser-frame points.  Returns a dict: grid
    (int8 [height][width]), width, height, origin_x, origin_y, rays, samples, counts {-1, 0, 50, 100}, and the number of
    samples that landed in column 0 / row 0 through a NEGATIVE quotient (neg_col0, neg_row0: the truncation quirk)."""
    tfs = [[float(v) for v in np.asarray(T).reshape(12)] for T in tfs]
    world = []
    for T, pts in zip(tfs, subs):
        for pt in np.asarray(pts, dtype=np.float64).reshape(-1, 3):
            P = world_point(T, pt)
            O = T[9:12]
            d = [P[i] - O[i] for i in range(3)]
            ln = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if all(math.isfinite(v) for v in P) and math.isfinite(ln):
                world.append((O, P, d, ln))
    out = dict(rays=len(world), samples=0, neg_col0=0, neg_row0=0, resolution=res)
    if not world:
        out.update(grid=np.zeros((0, 0), dtype=np.int8), width=0, height=0, origin_x=0.0, origin_y=0.0, counts={-1: 0, 0: 0, 50: 0, 100: 0})
        return out
    min_x = min(w[1][0] for w in world)
    max_x = max(w[1][0] for w in world)
    min_y = min(w[1][1] for w in world)
    max_y = max(w[1][1] for w in world)
    w = int((max_x - min_x) / res + 1)
    h = int((max_y - min_y) / res + 1)
    data = [-1] * (w * h)
    step = res / 2
    for O, P, d, ln in world:
        if ln > 0.0:
            unit = [d[i] / ln for i in range(3)]
            tr = 0.0
            while tr <= ln:
                cx, cy = O[0] + unit[0] * tr, O[1] + unit[1] * tr
                idx = _cell(cx, cy, min_x, min_y, res, w, h)
                if idx > -1:
                    if (cx - min_x) / res < 0:
                        out["neg_col0"] += 1
                    if (cy - min_y) / res < 0:
                        out["neg_row0"] += 1
                    if data[idx] == -1:
                        data[idx] = 0
                out["samples"] += 1
                tr += step
        idx = _cell(P[0], P[1], min_x, min_y, res, w, h)
        if idx > -1:
            data[idx] = 50 if data[idx] in (-1, 0) else 100
    g = np.array(data, dtype=np.int8).reshape(h, w)
    out.update(grid=g, width=w, height=h, origin_x=min_x, origin_y=min_y, counts={v: int((g == v).sum()) for v in (-1, 0, 50, 100)})
    return out


# ---------------------------------------------------------------------------------------------- the C++ walk (map_serial.cpp)
def build_serial(out_dir):
    """compile tests/cpp/map_serial.cpp with the host compiler (-O2 -ffp-contract=off) into out_dir; returns the CDLL"""
    so = os.path.join(str(out_dir), "libmap_serial.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "cpp", "map_serial.cpp"), "-o", so])
    L = C.CDLL(so)
    L.map_serial_render.restype = C.c_longlong
    L.map_serial_render.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int),
                                    C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_byte), C.c_longlong]
    return L


def render_serial(L, tfs, subs, res=0.05):
    """the same dict as render() (without neg_col0 / neg_row0) from the C++ walk"""
    tf = np.ascontiguousarray(np.asarray(tfs, dtype=np.float64).reshape(-1, 12))
    K = tf.shape[0]
    n = np.array([np.asarray(s).reshape(-1, 3).shape[0] for s in subs], dtype=np.int32)
    pts = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in subs] + [np.zeros((1, 3))]))
    wh, org, cnt = (C.c_int * 2)(), (C.c_double * 2)(), (C.c_longlong * 2)()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    args = (K, pd(tf), n.ctypes.data_as(C.POINTER(C.c_int)), pd(pts), float(res), wh, org, cnt)
    cells = L.map_serial_render(*args, None, 0)
    g = np.zeros(max(cells, 1), dtype=np.int8)
    assert L.map_serial_render(*args, g.ctypes.data_as(C.POINTER(C.c_byte)), cells) == cells
    g = g[:cells].reshape(wh[1], wh[0])
    return dict(grid=g, width=wh[0], height=wh[1], origin_x=org[0], origin_y=org[1], rays=cnt[0], samples=cnt[1], resolution=res,
                counts={v: int((g == v).sum()) for v in (-1, 0, 50, 100)})
