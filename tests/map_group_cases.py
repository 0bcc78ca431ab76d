"""Cases for the shared map of a group of fleet robots (tests/test_map_group_cases.py guards them on the serial reference alone,
tests/test_gpu_map_group.py runs them on the device): robots that scan ONE room, each with a world frame of its own, the rigid
transforms T_g_w that bring them into the group's frame, the merged reference render, and the comparison helpers."""
import ctypes as C

import numpy as np

import map_batch_cases as mc
import map_reference as ref

RES = mc.RES


def mul12(A, B):
    """A * B for transforms of 12 doubles (R row-major 9, then t); numpy, for building cases (the device's product is checked
    against liw_lie_mul)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    Ra, Rb = A[:9].reshape(3, 3), B[:9].reshape(3, 3)
    return np.concatenate([(Ra @ Rb).reshape(9), Ra @ B[9:] + A[9:]])


def inv12(A):
    A = np.asarray(A, dtype=np.float64)
    Rt = A[:9].reshape(3, 3).T
    return np.concatenate([Rt.reshape(9), -(Rt @ A[9:])])


def lie_mul(liw, A, B):
    """liw_lie_mul(A, B): the host's product, whose product and sum order the device follows"""
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    out = np.zeros(12)
    liw.lib().liw_lie_mul(pd(A), pd(B), pd(out))
    return out


def group_frames(rng, B, tilt=0.02):
    """T_g_w [B, 12]: group <- robot world, a yaw, a small tilt and an offset of its own per robot"""
    return np.array([mc.tf12(rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(-np.pi, np.pi), rng.uniform(-0.05, 0.05),
                             rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt)) for _ in range(B)])


def shared_room(rng, counts, n_rays=90, room=None):
    """len(counts) robots in one room (replay_room when None) with counts[b] sub-maps of n_rays rays each.  Every robot keeps its
    poses in a world frame of its own: T_w_l[b][k] = T_g_w[b]^-1 * (the scan's pose in the room).  -> dict(tfs_of, subs_of, T_g_w)"""
    B = len(counts)
    T_g_w = group_frames(rng, B)
    tfs_of, subs_of = [], []
    for b, K in enumerate(counts):
        t, s = mc.room_case(rng, K, n_rays, room=room)
        back = inv12(T_g_w[b])
        tfs_of.append(np.array([mul12(back, T) for T in t]).reshape(K, 12))
        subs_of.append(s)
    return dict(tfs_of=tfs_of, subs_of=subs_of, T_g_w=T_g_w)


def concat(tfs_of, subs_of, members):
    """the members' transforms [n, 12] and sub-maps in (robot, sub-map) order: what ONE map is fed"""
    tfs = [np.asarray(tfs_of[b], dtype=np.float64).reshape(-1, 12) for b in members]
    subs = [s for b in members for s in subs_of[b]]
    return (np.concatenate(tfs) if tfs else np.zeros((0, 12))), subs


def compose(tfs_of, T_g_w, mul=mul12):
    """T_g_l per robot: T_g_w[b] * T_w_l[b][k]"""
    return [np.array([mul(T_g_w[b], T) for T in np.asarray(t).reshape(-1, 12)]).reshape(-1, 12) for b, t in enumerate(tfs_of)]


# two robots that hold one point each (T_g_w = None: the transforms are the group's own)
def one_point_same_cell():
    """both robots see the point (1, 0.5) of the group frame, from different places: 50 in either robot's grid, 100 merged"""
    subs_of = [[np.array([[1.0, 0.0, 0.0]])], [np.array([[0.0, 0.8, 0.0]])]]
    tfs_of = [np.array([mc.tf12(0.0, 0.5, 0.0)]), np.array([mc.tf12(1.0, -0.3, 0.0)])]
    return tfs_of, subs_of


def one_point_disjoint():
    """two points 2.42 m / 2.31 m apart, each seen along a short ray from inside the box: a 49 x 47 grid, mostly unknown"""
    subs_of = [[np.array([[0.35, 0.0, 0.0]])], [np.array([[0.3, 0.0, 0.0]])]]
    tfs_of = [np.array([mc.tf12(0.35, 0.01, np.pi)]), np.array([mc.tf12(2.12, 2.32, 0.0)])]
    return tfs_of, subs_of


def assert_group(gm, g, want, row=None):
    """group g's held grid and info equal the reference render `want` exactly; row: its info row of the render, equal too"""
    info = gm.info_of(g)
    assert info.pop("status") == (1 if want["rays"] == 0 else 0)
    mc.assert_info(info, want)
    if row is not None:
        assert row == info
    grid = gm.grid(g)
    assert grid.shape == want["grid"].shape
    assert int((grid != want["grid"]).sum()) == 0


def gregions(gm):
    """[G, group_bytes] uint8 host copy of the group regions"""
    gm._sync()
    return gm.group_regions().cpu().numpy().copy()
