// k_lfe.hpp — interface between the fleet laser front-end's host code (liw_laser_batch.cpp) and its kernels (k_lfe_lines.hip,
// k_lfe_submap.hip, k_lfe_match.hip, k_lfe_state.hip): the parameter blocks and layouts passed by value, the records a getter
// reads back, the LDS planners of the wave kernels, and one launch_* per kernel launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/liw_laser_batch.h"

namespace lfe {

typedef unsigned long long u64;

constexpr double kPi = 3.14159265358979323846;
constexpr int kBlock = 64;

struct DP {                // laser parameters as the kernels use them
    double res, cont_thr, min_len, max_dis, tol, mf_p, mf_q;
    int w, h, n_acc;
    double Til_R[9], Til_t[3];
};
struct Lay {
    size_t robot_bytes, slot_bytes;
    int B, slots, max_points, max_lines, max_entries;
};
struct Mgr {               // laser_manager state of one robot (256 bytes in the store)
    int status, has_ref, has_spawn, ref_sub;
    int count, pad0, pad1, pad2;
    double sub_p[2][3], sub_q[2][3];
    double last_R[9], last_t[3];
};
struct SlotHdr { int status, n_lines, n_entries, pad; double time, pad2; };
constexpr size_t kMgrBytes = 256, kHdrBytes = 32;
static_assert(sizeof(Mgr) <= kMgrBytes, "manager record");
static_assert(sizeof(SlotHdr) == kHdrBytes, "slot header");

// store: robot-major; robot b = [Mgr | slot 0 .. slots-1 | sub-map 0 | sub-map 1]; slot = [SlotHdr | lines [max_lines][10] | entries]
// (make_lay of liw_laser_batch.cpp fills a Lay)
__host__ __device__ inline char* robot_ptr(void* store, const Lay& L, int b) { return (char*)store + (size_t)b * L.robot_bytes; }
__host__ __device__ inline size_t slot_off(const Lay& L, int phys) { return kMgrBytes + (size_t)phys * L.slot_bytes; }

__host__ __device__ inline void xy_to_index(const DP& P, double x, double y, int& c, int& r) {
    c = (int)(x / P.res + (double)(P.w / 2));
    r = (int)(y / P.res + (double)(P.h / 2));
}
__host__ __device__ inline bool valid(const DP& P, int r, int c) { return r >= 0 && r < P.h && c >= 0 && c < P.w; }
// first entry with key >= k (entries sorted)
__host__ __device__ inline int lower_bound(const u64* a, int n, u64 k) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < k) lo = mid + 1; else hi = mid; }
    return lo;
}

// LDS of k_lfe_spawn_wave: one work-group of one wave per (robot, scan); everything a step reads more than once lives in LDS
// (offsets in bytes):
//   X     [max_points][3] doubles   the scan's points; after the last add_line the same bytes are the hash set / sort buffer of the entries
//   brk   bit i: a continuous run starts at point i          mx   bit i: point i is a strict local maximum of the response
//   misc  counters, then per candidate of a chunk max_dis (bit pattern of a non-negative double, LDS atomic max) and `has a cell`
//   lbase / lcnt [max_lines]       where line id keeps its cells in `cell`, and how many
//   U     resp [max_points] doubles, until the maxima are known; afterwards
//         cell [max_points * 3 / 2 + 2] (first the `ends` lists of the runs; then a candidate i1 .. i2 with index j owns
//         cell[i1 + j ..]: ranges of consecutive candidates share at most one point) and cand [max_points / 2 + 1] (i1, i2) of
//         the candidate segments with i2 - i1 >= 2
struct WaveLds { unsigned x, brk, mx, misc, lbase, lcnt, u, cand; int tcap; size_t total; };
__host__ __device__ inline size_t up8(size_t x) { return (x + 7) / 8 * 8; }
inline WaveLds wave_lds(const Lay& L) {
    const size_t MP = (size_t)L.max_points, W = (MP + 63) / 64, ML = (size_t)L.max_lines;
    WaveLds O;
    size_t o = 0;
    O.x = (unsigned)o; o += 24 * MP;
    O.brk = (unsigned)o; o += 8 * W;
    O.mx = (unsigned)o; o += 8 * W;
    O.misc = (unsigned)o; o += 16 + 12 * kBlock;
    O.lbase = (unsigned)o; o += up8(4 * ML);
    O.lcnt = (unsigned)o; o += up8(4 * ML);
    O.u = (unsigned)o;
    const size_t cells = up8(4 * (MP + MP / 2 + 2)), cands = 8 * (MP / 2 + 1);
    O.cand = (unsigned)(o + cells);
    const size_t u = cells + cands > 8 * MP ? cells + cands : 8 * MP;
    O.total = o + u;
    O.tcap = 1;   // slots of the hash set in X's bytes: the largest power of two <= 3 * max_points, more than the 1.5 * max_points
    while ((size_t)O.tcap * 2 <= 3 * MP) O.tcap *= 2;   // (cell, line) pairs the candidates' points can make
    return O;
}
constexpr size_t kWaveLdsMax = 64 * 1024;   // a work-group's limit (two of them still share a CU); larger dimensions go to the lane kernel

// LDS of k_lfe_add_scan_wave: the new entries of one target (nw), their final positions (pos), id and entry offset per source line
struct AddLds { unsigned nw, pos, lid, loff; int ecap; size_t total; };
constexpr int kAddNewCap = 2048;   // new entries of one target held in LDS (24 KiB with pos); beyond it the serial escape
inline AddLds add_lds(const Lay& L) {
    AddLds O;
    O.ecap = L.max_entries < kAddNewCap ? L.max_entries : kAddNewCap;
    size_t o = 0;
    O.nw = (unsigned)o; o += 8 * (size_t)O.ecap;
    O.pos = (unsigned)o; o += up8(4 * (size_t)O.ecap);
    O.lid = (unsigned)o; o += up8(4 * (size_t)L.max_lines);
    O.loff = (unsigned)o; o += up8(4 * (size_t)L.max_lines);
    O.total = o;
    return O;
}
inline size_t match_lds(const Lay& L) { return 12 * (size_t)L.max_lines; }   // k_lfe_match_wave: best and d per line of the frame's scan
inline size_t pack_init_lds(int n) { return 4 * ((size_t)n + 1); }            // k_lfe_pack_init: the frames' offsets inside a window

struct Trk {               // tracking record of one robot (256 bytes, caller-owned, apart from the store)
    double kf_R[9], kf_t[3];   // last_keyframe_tf
    double ang[3];             // current_angular_local
    double stamp;              // of the last accepted frame
    int tracked, keys, skipped, pad;
};
constexpr size_t kTrkBytes = 256;
static_assert(sizeof(Trk) <= kTrkBytes, "tracking record");
struct TP { double Tiw_R[9], Tiw_t[3], min_dt, p_thr, q_thr; };

struct Ini {               // initialisation record of one robot (256 bytes, caller-owned, apart from the store and the tracking record)
    double p[3], q[3], v[3], bs[6];   // current_p / q / v / bs
    double ang[3];                    // current_angular_local
    int status, n_frames;             // LIW_LFE_INITIALIZING / _TRACKING; frames in the window being filled
    int inits, failed, dropped, pad;  // initialisations, failed windows, dropped frames
};
constexpr size_t kIniBytes = 256;
static_assert(sizeof(Ini) <= kIniBytes, "initialisation record");
struct IP { double Tiw_R[9], Tiw_t[3], p_thr, q_thr; int N; };

// Each launches one kernel on s and returns LIW_OK, or LIW_EHIP with the HIP error left for the caller to read.
inline int blocks(size_t n, int bs) { return (int)((n + bs - 1) / bs); }
inline int launched() { return hipPeekAtLastError() == hipSuccess ? LIW_OK : LIW_EHIP; }
// k_lfe_lines.hip
int launch_ranges(void* store, const Lay& L, const float* ranges, int n_rays, const float2* cs, float tinc, const double* stamps, double* pts,
                  double* times, int* n_pts, hipStream_t s);
int launch_deskew(const Lay& L, double* pts, const double* times, const int* n_pts, const double* stamps, const double* lin, const double* ang,
                  hipStream_t s);
int launch_spawn(void* store, const Lay& L, const DP& P, int slot, const double* pts, const int* n_pts, const double* times, hipStream_t s);
int launch_spawn_wave(void* store, const Lay& L, const DP& P, const WaveLds& O, int slot, const double* pts, const int* n_pts, const double* times,
                      int max_corners, double* corners, int* n_corners, hipStream_t s);
int launch_corners_world(void* store, const Lay& L, const DP& P, int max_corners, const double* corners, const int* n_corners, const double* pose,
                         const unsigned char* mask, const unsigned char* clear, int acc_cap, double* acc, int* n_acc, hipStream_t s);
// k_lfe_submap.hip
int launch_reset(void* store, const Lay& L, const unsigned char* mask, hipStream_t s);
int launch_reset_mgr(void* store, const Lay& L, const unsigned char* mask, hipStream_t s);
int launch_add_scan(void* store, const Lay& L, const DP& P, int src_slot, const double* pose, long long pose_stride, const unsigned char* mask,
                    unsigned char* flags, hipStream_t s);
int launch_add_scan_wave(void* store, const Lay& L, const DP& P, const AddLds& O, int first_slot, int F, int reset, const double* pose,
                         long long robot_stride, long long frame_stride, const unsigned char* mask, unsigned char* flags, hipStream_t s);
int launch_slot_copy(void* store, const Lay& L, const int* dst_slot, const unsigned char* mask, hipStream_t s);
// k_lfe_match.hip; sel == nullptr: every robot (k_lfe_scan_init, k_lfe_pack_init), else the listed ones (the _sel kernels)
int launch_match(void* store, const Lay& L, const DP& P, int slot1, int slot2, const double* pose1, const double* pose2, int kk, int cap, int* count,
                 double* recs, int* idx1, int* idx2, double* match_pose, hipStream_t s);
int launch_match_wave(void* store, const Lay& L, const DP& P, int front_slot, int first_slot, int F, const double* pose_front, const double* poses,
                      long long rs, long long fs, int kk, int cap, int* count, double* recs, int* idx1, int* idx2, double* match_pose, hipStream_t s);
int launch_scan_init(int R, int F, int cap, const int* count, const int* sel, int* off, hipStream_t s);
int launch_pack(int B, int n, int frame, int cap, int Ltot, const int* off, const double* recs, const double* match_pose, int* laser_frame,
                double* laser_pts, double* mp_out, unsigned char* has_match, hipStream_t s);
int launch_pack_init(int R, int n, int cap, int Ltot, const int* off, const int* count, const double* recs, const double* match_pose,
                     const double* pose_front, long long front_stride, const int* sel, int* laser_frame, double* laser_pts, double* mp_out,
                     unsigned char* has_match, unsigned char* init_ok, hipStream_t s);
// k_lfe_state.hip
int launch_track_init(int B, void* track, const double* x, long long robot_stride, const double* ang, const unsigned char* mask, hipStream_t s);
int launch_track_begin(int B, const DP& P, const TP& tp, void* track, double* x, const double* imu_X, const double* imu_Dt, const double* wheel_T,
                       const double* stamps, const unsigned char* mask, double* linear, double* angular, double* pose_new, unsigned char* skip,
                       hipStream_t s);
int launch_track_end(const void* store, const Lay& L, const DP& P, const TP& tp, void* track, int slot, const double* x, const int* count,
                     const unsigned char* mask, unsigned char* key, double* pose, hipStream_t s);
int launch_init_reset(int B, const IP& ip, void* init, const unsigned char* mask, hipStream_t s);
int launch_init_begin(int B, const DP& P, const IP& ip, void* init, const double* imu_X, const double* imu_Dt, const double* wheel_T,
                      const unsigned char* mask, double* x_init, unsigned char* drop, int* slot_of, int* rows, hipStream_t s);
int launch_init_rows(int B, int F, const int* rows, const double* imu_X, const double* imu_J, const double* imu_sqrtP, const double* imu_Dt,
                     const double* wheel_T, const double* wheel_sqrtP, double* w_imu_X, double* w_imu_J, double* w_imu_sqrtP, double* w_imu_Dt,
                     double* w_wheel_T, double* w_wheel_sqrtP, hipStream_t s);
int launch_init_select(int B, int N, const void* init, unsigned char* ready, int* sel, int* n_sel, hipStream_t s);
int launch_init_commit(int R, const IP& ip, void* init, void* track, const int* sel, const unsigned char* init_ok, const double* x_sol, double* x_init,
                       double* x_track, hipStream_t s);
int launch_crmath(int op, int n, const double* a, const double* b, double* out, hipStream_t s);

}  // namespace lfe
