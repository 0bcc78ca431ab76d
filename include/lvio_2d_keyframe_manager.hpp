// lvio_2d_keyframe_manager.hpp — C++ host mirror of the reference's back-end bookkeeping around the pose-graph solve
// (BASELINE config C5), header-only over liw_posegraph.h / liw_lie.h / liw_io.h.  Same member names as
// reference src/trajectory/keyframe_manager.{h,cpp}:
//   add_keyframe / do_add_keyframe     :400-407, :419-482   key-frame queue, tracking poses, sequential edges, corrected pose
//   update_other_frame                 :408-418             current front-end pose carried into the corrected map frame
//   solve                              :722-838             -> liw_posegraph_solve (the MI355X relinearisation)
//   is_time_to_solve                   :839-848             "a loop is pending and 10 s have passed since the last solve"
//   ~keyframe_manager                  :370-397             back_end.txt (TUM) of every key frame
//   laser_loop_detect                  :642-712             opt-in built-in detector (enable_loop_detection -> include/lvio_2d_loop.hpp,
//                                                           the MI355X descriptor match), fed here because it needs tfs_tracking
//   show_laser_map                     :483-511             opt-in occupancy-grid map (enable_laser_map -> liw_map.h, the MI355X ray
//                                                           caster): every laser key frame with a laser_match_ptr gives its scan2
//                                                           points (uploaded once, when the key frame arrives) and its current p, q
// A detector may instead be a callback: when key frame `index` arrives it may return an edge (index1 = index, index2 = an older key
// frame, tf12) — the shape laser_loop_detect returns (:664-665, :702); a callback, when set, takes precedence.  When the built-in
// detector holds max_keyframes key frames, detection stops (loop_stopped) and the back-end goes on.  Two deliberate differences of
// this offline form: the back-end runs on the caller's thread (the reference has its own thread, keyframe_manager.cpp:859-881) and
// is_time_to_solve compares key-frame STAMPS instead of ros::WallTime, so that a replay is deterministic.  For the same reason
// show_laser_map is called after every back-end solve and by the caller at the end of a log, not every 10 s of wall time; when the map
// store is full (max_submaps / max_points) later key frames are left out of it (map_stopped) and the back-end goes on.
#pragma once
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "liw_io.h"
#include "liw_lie.h"
#include "liw_map.h"
#include "liw_posegraph.h"
#include "lvio_2d_laser.hpp"
#include "lvio_2d_loop.hpp"
#include "lvio_2d_solver.hpp"

namespace lvio_2d {

struct edge {   // reference src/trajectory/keyframe_type.h:12-32
    int index1, index2;
    double tf12[12];   // R (row-major 9) then t
};

struct keyframe_manager_params {
    liw_pg_params pg{};                // loop_sigma_p / _q, loop_edge_k, use_ground_{p,q}_factor (config/office.yaml:106-115)
    double solve_period = 10.0;        // seconds between back-end solves (is_time_to_solve, :843); key-frame time here
    int max_iterations = 0;            // <= 0: Ceres default (50), as :813-818
    bool output_tum = false;
    std::string output_dir;
};

class keyframe_manager {
public:
    // detector(index of the new key frame, the queue so far) -> true and an edge (index1 = index, index2 = older) if a loop closes
    using loop_detector = std::function<bool(int, const std::deque<frame_info::ptr>&, edge*)>;

    keyframe_manager(const liw_params& prm, const keyframe_manager_params& kp) : prm_(prm), kp_(kp), ctx_(liw_create(&prm)) {
        liw_lie_make_tf(zero3_, zero3_, modify_delta_tf);
    }
    ~keyframe_manager() {
        if (kp_.output_tum) write_tum((kp_.output_dir + "back_end.txt").c_str());
        loop_.reset();   // the detector is bound to ctx_
        liw_map_destroy(map_);   // and so is the map
        liw_destroy(ctx_);
    }
    keyframe_manager(const keyframe_manager&) = delete;
    keyframe_manager& operator=(const keyframe_manager&) = delete;

    void set_loop_detector(loop_detector d) { detector_ = std::move(d); }
    // the built-in laser loop detector (liw_loop.h) on this manager's ctx; false if the parameters or dims are rejected
    bool enable_loop_detection(const liw_loop_params& p, const liw_loop_dims& d) {
        loop_.reset(new laser_loop_detector(ctx_, p, d));
        if (!loop_->ok()) { loop_.reset(); return false; }
        return true;
    }

    // the occupancy-grid map (liw_map.h) on this manager's ctx; false if the parameters or dims are rejected.  Needs scans that keep
    // their points (trajectory_params::enable_laser_vis).
    bool enable_laser_map(const liw_map_params& p, const liw_map_dims& d) {
        liw_map_destroy(map_);
        map_ = liw_map_create(ctx_, &p, &d);
        map_keyframes.clear();
        map_stopped = false;
        return map_ != nullptr;
    }

    // show_laser_map (:483-511): the map of every laser key frame's scan at its current (corrected) pose; the points are on the
    // device already, only the poses are sent.  Returns the liw_map_render status (also kept in map_status).
    int show_laser_map() {
        if (!map_) return map_status = LIW_ESTATE;
        std::vector<double> poses(map_keyframes.size() * 6);
        for (size_t k = 0; k < map_keyframes.size(); ++k) {
            std::memcpy(&poses[k * 6], keyframe_queue[(size_t)map_keyframes[k]]->p, 24);
            std::memcpy(&poses[k * 6 + 3], keyframe_queue[(size_t)map_keyframes[k]]->q, 24);
        }
        map_status = liw_map_render(map_, (int)map_keyframes.size(), poses.data(), &last_map_info);
        if (map_status >= 0) { ++map_renders; map_poses = poses; }
        return map_status;
    }

    // the exact input of the last render: int32 K, then per sub-map float64 pose[6] (p, q), int32 n, float64 points[n][3]
    bool write_map_input(const char* path) const {
        FILE* f = fopen(path, "wb");
        if (!f) return false;
        const int K = (int)(map_poses.size() / 6);
        fwrite(&K, sizeof(int), 1, f);
        for (int k = 0; k < K; ++k) {
            const std::vector<double>& pts = keyframe_queue[(size_t)map_keyframes[(size_t)k]]->laser_match_ptr->scan2->points;
            const int n = (int)(pts.size() / 3);
            fwrite(&map_poses[(size_t)k * 6], sizeof(double), 6, f);
            fwrite(&n, sizeof(int), 1, f);
            if (n) fwrite(pts.data(), sizeof(double), (size_t)n * 3, f);
        }
        return fclose(f) == 0;
    }

    // add_keyframe (:400-407) + do_add_keyframe (:419-482) in one call: no worker thread in the offline form
    void add_keyframe(const frame_info::ptr& frame_ptr) {
        keyframe_queue.push_back(frame_ptr);
        tfs_tracking.emplace_back();
        double* tr = tfs_tracking.back().v;
        liw_lie_make_tf(frame_ptr->p, frame_ptr->q, tr);
        double corrected[12];
        liw_lie_mul(modify_delta_tf, tr, corrected);
        liw_lie_log_SE3(corrected, frame_ptr->p, frame_ptr->q);
        if (map_ && !map_stopped && frame_ptr->type == frame_info::laser && frame_ptr->laser_match_ptr && frame_ptr->laser_match_ptr->scan2) {
            const std::vector<double>& pts = frame_ptr->laser_match_ptr->scan2->points;
            const int r = liw_map_add_submap(map_, (int)(pts.size() / 3), pts.data());
            if (r >= 0) map_keyframes.push_back((int)keyframe_queue.size() - 1);
            else if (r == LIW_ENOMEM) map_stopped = true;
            else map_status = r;
        }
        int loop_status = 0;
        bool detect_now = false;
        if (loop_ && !detector_ && !loop_stopped) {   // the laser map feature of every key frame (:428-437)
            if (loop_->full()) loop_stopped = true;   // capacity reached: detection ends, the back-end goes on with the loops it has
            else {
                const int r = loop_->add_keyframe(frame_ptr->type == frame_info::laser, tr, frame_ptr->laser_concers);
                if (r < 0) loop_status = r;
                else detect_now = true;
            }
        }
        if (keyframe_queue.size() > 1) {
            const int index1 = (int)keyframe_queue.size() - 2, index2 = index1 + 1;
            edge e{index1, index2, {}};
            double inv1[12];
            liw_lie_inverse(tfs_tracking[index1].v, inv1);
            liw_lie_mul(inv1, tfs_tracking[index2].v, e.tf12);
            seq_edges.push_back(e);
        }
        if (frame_ptr->type == frame_info::laser && detector_) {
            edge lp{};
            if (detector_((int)keyframe_queue.size() - 1, keyframe_queue, &lp)) {
                loop_edges.push_back(lp);
                has_loop_wait_for_solve = true;
                last_loop_index = (int)keyframe_queue.size() - 1;
            }
        } else if (frame_ptr->type == frame_info::laser && detect_now) {
            liw_loop_edge le{};
            const int r = loop_->detect(&le);
            if (r < 0) loop_status = r;
            else if (r == 1) {
                edge lp{le.index1, le.index2, {}};
                std::memcpy(lp.tf12, le.tf12, sizeof lp.tf12);
                loop_edges.push_back(lp);
                has_loop_wait_for_solve = true;
                last_loop_index = (int)keyframe_queue.size() - 1;
            }
        }
        if (loop_status) {   // a detector error stops the back-end like a failed solve
            last_status = loop_status;
            loop_error_ = loop_->last_error();
            return;
        }
        double last_frame_tf[12];
        std::memcpy(last_frame_tf, tr, sizeof last_frame_tf);
        if (is_time_to_solve(frame_ptr->time)) {
            last_solve_time = frame_ptr->time;
            solve();
            if (last_status == 0) {
                double current_frame_tf[12], inv_last[12];
                liw_lie_make_tf(frame_ptr->p, frame_ptr->q, current_frame_tf);
                liw_lie_inverse(last_frame_tf, inv_last);
                liw_lie_mul(current_frame_tf, inv_last, modify_delta_tf);   // :468-473
            }
            has_loop_wait_for_solve = false;
            ++solves;
            if (map_ && last_status == 0) show_laser_map();   // every pose moved: the map is rendered again from all of them
        }
    }

    // update_other_frame (:408-418): the front-end's newest pose expressed in the corrected map frame (what the reference shows)
    void update_other_frame(const std::deque<frame_info::ptr>& frame_infos, double* p3, double* q3) const {
        if (frame_infos.empty()) return;
        double tf[12], cur[12];
        liw_lie_make_tf(frame_infos.back()->p, frame_infos.back()->q, tf);
        liw_lie_mul(modify_delta_tf, tf, cur);
        liw_lie_log_SE3(cur, p3, q3);
    }

    // keyframe_manager::solve (:722-838) on the MI355X
    void solve() {
        const int N = (int)keyframe_queue.size();
        if (N < 2) return;
        std::vector<double> poses((size_t)N * 6);
        for (int i = 0; i < N; ++i) {
            std::memcpy(&poses[(size_t)i * 6], keyframe_queue[i]->p, 24);
            std::memcpy(&poses[(size_t)i * 6 + 3], keyframe_queue[i]->q, 24);
        }
        std::vector<int> si, li;
        std::vector<double> st, lt;
        for (const edge& e : seq_edges) { si.push_back(e.index1); si.push_back(e.index2); st.insert(st.end(), e.tf12, e.tf12 + 12); }
        for (const edge& e : loop_edges) { li.push_back(e.index1); li.push_back(e.index2); lt.insert(lt.end(), e.tf12, e.tf12 + 12); }
        last_status = liw_posegraph_solve(ctx_, &kp_.pg, N, poses.data(), (int)seq_edges.size(), si.data(), st.data(), (int)loop_edges.size(),
                                          li.empty() ? nullptr : li.data(), lt.empty() ? nullptr : lt.data(), kp_.max_iterations, &last_summary);
        if (last_status) return;
        for (int i = 0; i < N; ++i) {
            std::memcpy(keyframe_queue[i]->p, &poses[(size_t)i * 6], 24);
            std::memcpy(keyframe_queue[i]->q, &poses[(size_t)i * 6 + 3], 24);
        }
    }

    bool write_tum(const char* path) const {   // (:370-397) every key frame's base pose, 10 decimals
        liw_tum_writer* w = liw_tum_open(path, &prm_);
        if (!w) return false;
        for (const auto& f : keyframe_queue) liw_tum_append(w, f->time, f->p, f->q);
        liw_tum_close(w);
        return true;
    }

    liw_map* laser_map() const { return map_; }
    const laser_loop_detector* laser_loop() const { return loop_.get(); }
    const char* last_error() const { return loop_error_.empty() ? liw_last_error(ctx_) : loop_error_.c_str(); }

    std::deque<frame_info::ptr> keyframe_queue;
    struct tf12 { double v[12]; };
    std::vector<tf12> tfs_tracking;
    std::vector<edge> seq_edges, loop_edges;
    double modify_delta_tf[12];
    bool has_loop_wait_for_solve = false;
    bool loop_stopped = false;   // the built-in detector held max_keyframes key frames: no detection after that
    int last_loop_index = -1, solves = 0;
    double last_solve_time = -1e300;
    int last_status = 0;
    liw_summary last_summary{};
    std::vector<int> map_keyframes;    // key-frame index of sub-map k of the map
    std::vector<double> map_poses;     // [K][6] the poses of the last render
    liw_map_info last_map_info{};
    bool map_stopped = false;          // the map store is full: later key frames are not in the map
    int map_status = 0, map_renders = 0;

private:
    bool is_time_to_solve(double time_now) const { return has_loop_wait_for_solve && time_now - last_solve_time > kp_.solve_period; }
    liw_params prm_;
    keyframe_manager_params kp_;
    liw_ctx* ctx_;
    loop_detector detector_;
    std::unique_ptr<laser_loop_detector> loop_;
    liw_map* map_ = nullptr;
    std::string loop_error_;
    double zero3_[3] = {0, 0, 0};
};

}  // namespace lvio_2d
