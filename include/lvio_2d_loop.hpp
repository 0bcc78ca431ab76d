// lvio_2d_loop.hpp — C++ host mirror of the reference's laser loop detection (keyframe_manager::laser_loop_detect and the
// laser_map_feature code behind it, reference src/trajectory/keyframe_manager.cpp:642-712, :898-1184), header-only over
// include/liw_loop.h.  The detector's device store belongs to the library (this mirror is built with g++ against the .so);
// keyframe_manager (include/lvio_2d_keyframe_manager.hpp) feeds it from add_keyframe when enable_loop_detection is called.
#pragma once
#include <vector>

#include "liw_loop.h"

namespace lvio_2d {

// config/office.yaml:98-108
inline liw_loop_params office_loop_params(unsigned long long seed = 0) {
    liw_loop_params p{};
    p.a_res = 0.03;
    p.d_res = 0.03;
    p.submap_count = 30;
    p.min_match_threshold = 5;
    p.min_interval = 100;
    p.max_dis = 1.0;
    p.max_tf_p = 1.0;
    p.max_tf_q = 0.5;
    p.seed = seed;
    return p;
}

class laser_loop_detector {
public:
    laser_loop_detector(liw_ctx* ctx, const liw_loop_params& p, const liw_loop_dims& d) : h_(liw_loop_create(ctx, &p, &d)), dims_(d) {}
    ~laser_loop_detector() { liw_loop_destroy(h_); }
    laser_loop_detector(const laser_loop_detector&) = delete;
    laser_loop_detector& operator=(const laser_loop_detector&) = delete;

    bool ok() const { return h_ != nullptr; }
    // every key-frame slot is taken: a further add_keyframe returns LIW_ENOMEM
    bool full() const { return h_ && liw_loop_num_keyframes(h_) >= dims_.max_keyframes; }
    // the key frame's tracking pose (world <- IMU, T12) and, for a laser key frame, its world-frame corners [k][3]
    int add_keyframe(bool is_laser, const double* tf_tracking12, const std::vector<double>& corners) {
        if (!h_) return LIW_EINVAL;
        return liw_loop_add_keyframe(h_, is_laser ? 1 : 0, tf_tracking12, (int)(corners.size() / 3), corners.empty() ? nullptr : corners.data());
    }
    // laser_loop_detect for the newest key frame: 1 and *e filled if a loop closes, 0 if not, < 0 on error
    int detect(liw_loop_edge* e) { return h_ ? liw_loop_detect(h_, e) : LIW_EINVAL; }
    const char* last_error() const { return h_ ? liw_loop_last_error(h_) : "liw_loop_create failed (bad params or dims)"; }
    liw_loop* handle() const { return h_; }

private:
    liw_loop* h_;
    liw_loop_dims dims_;
};

}  // namespace lvio_2d
