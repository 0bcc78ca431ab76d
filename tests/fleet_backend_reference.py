"""Host restatement of what a robot of the fleet pose-graph back-end (include/liw_posegraph_batch.h) keeps around a solve, over the
exported liw_lie_* routines: add_keyframes, add_loops, due, the commit after a solve and correct, with the capacity and bad-edge
rules of the fleet.  The solve itself is a callable: tests/test_fleet_backend_reference.py delegates it to pyoracle.posegraph_solve
and compares the whole with pyoracle.backend_run; tests/test_gpu_posegraph_batch.py hands it the device's solved poses."""
import numpy as np

from track_glue_reference import Lie

IDENTITY12 = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


class RobotBackEnd:
    def __init__(self, lie, max_keyframes, max_loops, solve_period):
        self.lie, self.K, self.ML, self.period = lie, int(max_keyframes), int(max_loops), float(solve_period)
        self.reset()

    def reset(self):
        self.stamps, self.tfs, self.poses, self.seq = [], [], [], []
        self.loop_idx, self.loop_tf = [], []
        self.full = self.loops_full = self.bad_edge = self.pending = False
        self.solves, self.last_solve_time, self.modify = 0, -1e300, IDENTITY12.copy()

    def add_keyframe(self, pose, stamp):
        """-> added"""
        if len(self.tfs) >= self.K:
            self.full = True
            return False
        pose = np.asarray(pose, dtype=np.float64)
        tf = self.lie.make_tf(pose[:3], pose[3:])
        p, q = self.lie.log_SE3(self.lie.mul(self.modify, tf))
        if self.tfs:
            self.seq.append(self.lie.mul(self.lie.inverse(self.tfs[-1]), tf))
        self.tfs.append(tf)
        self.poses.append(np.concatenate([p, q]))
        self.stamps.append(float(stamp))
        return True

    def add_loop(self, edge, tf12):
        i1, i2, n = int(edge[0]), int(edge[1]), len(self.tfs)
        if i1 < 0 or i1 >= n or i2 < 0 or i2 >= n or i1 == i2:
            self.bad_edge = True
            return
        if len(self.loop_idx) >= self.ML:
            self.loops_full = True
            return
        self.loop_idx.append((i1, i2))
        self.loop_tf.append(np.asarray(tf12, dtype=np.float64).copy())
        self.pending = True

    def due(self, key, stamp):
        return bool(key) and self.pending and float(stamp) - self.last_solve_time > self.period

    def graph(self):
        n = len(self.tfs)
        return dict(poses=np.array(self.poses).reshape(n, 6), seq_idx=np.array([(k, k + 1) for k in range(n - 1)], dtype=np.int32).reshape(-1, 2),
                    seq_tf12=np.array(self.seq).reshape(-1, 12), loop_idx=np.array(self.loop_idx, dtype=np.int32).reshape(-1, 2),
                    loop_tf12=np.array(self.loop_tf).reshape(-1, 12))

    def commit(self, solved_poses, stamp):
        """after keyframe_manager::solve: the poses, modify_delta_tf = make_tf(p_last, q_last) * tfs_tracking.last^-1, the flags"""
        solved_poses = np.asarray(solved_poses, dtype=np.float64).reshape(-1, 6)
        self.poses = [x.copy() for x in solved_poses]
        cur = self.lie.make_tf(solved_poses[-1, :3], solved_poses[-1, 3:])
        self.modify = self.lie.mul(cur, self.lie.inverse(self.tfs[-1]))
        self.pending = False
        self.last_solve_time = float(stamp)
        self.solves += 1

    def correct(self, pose):
        pose = np.asarray(pose, dtype=np.float64)
        p, q = self.lie.log_SE3(self.lie.mul(self.modify, self.lie.make_tf(pose[:3], pose[3:])))
        return np.concatenate([p, q])


def run_schedule(liw, solve, times, poses, loops, solve_period, max_keyframes=None, max_loops=None):
    """oracle/keyframe_manager.h's add_keyframe loop on the restatement: loops = [(trigger, older, tf12)], at most one per trigger;
    solve(graph dict) -> (poses, iterations).  -> (RobotBackEnd, iterations of the last solve)"""
    rb = RobotBackEnd(Lie(liw), max_keyframes or len(times), max_loops if max_loops is not None else len(loops), solve_period)
    iterations = 0
    for k, (t, x) in enumerate(zip(times, poses)):
        added = rb.add_keyframe(x, t)
        for trig, older, tf in loops:
            if trig == k and added:
                rb.add_loop((k, older), tf)
                break
        if rb.due(added, t):
            if len(rb.tfs) >= 2:
                xs, its = solve(rb.graph())
                iterations = its
            else:
                xs = np.array(rb.poses)
            rb.commit(xs, t)
    return rb, iterations
