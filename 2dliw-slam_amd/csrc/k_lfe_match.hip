// k_lfe_match.hip — fleet laser front-end, matching and packing (C ABI include/liw_laser_batch.h, host side liw_laser_batch.cpp):
// laser_manager::do_match lane-per-robot, match_with_front of a whole INIT window wave-per-(robot, frame), and the packs that turn
// match records into the laser arrays liw_batch takes.  The mean match distance is summed in match order, as on the host.
#pragma clang fp contract(off)   // the x86-64 host build of liw_laser.cpp does not contract; hipcc contracts device code by default

#include <hip/hip_runtime.h>

#include "k_lfe.hpp"
#include "k_lfe_dev.hpp"

namespace lfe {

// match_pair, the search of do_match for line i of s2, with T12 = (pose1 * Til)^-1 * (pose2 * Til): candidates of the (2a + 1)^2 cells
// around the transformed mid point by binary search of s1's sorted entries (dr, dc, push order), strict-< argmin of the angle, 10
// degree gate.  -> best line of s1 and the pair's distance d; false when the host skips the line (d is then left as it was).
// A struct of references with a call operator and not a function of ten arguments: that is what the lambda it replaces in k_lfe_match
// was, and only so does that kernel compile to the code it had.
struct MatchPair {
    const DP& P; const Slot& s1; const Slot& s2; const Iso<double>& T12; const int& a; const int& n1; const int& ne;
    __device__ __forceinline__ bool operator()(int i, int& best, double& d) const {
        const double* l2 = s2.lines + 10 * (size_t)i;
        const Vec l2p1 = ld3(l2), l2p2 = ld3(l2 + 3);
        const Vec mid((l2p1.x + l2p2.x) / 2, (l2p1.y + l2p2.y) / 2, (l2p1.z + l2p2.z) / 2);
        const Vec tm = apply(T12, mid);
        int c, r;
        xy_to_index(P, tm.x, tm.y, c, r);
        best = -1;
        bool any = false;
        double best_angle = kPi * 2;
        const Vec v2 = vsub(apply(T12, l2p2), apply(T12, l2p1));
        for (int dr = -a; dr <= a; ++dr)
            for (int dc = -a; dc <= a; ++dc) {
                const int rr = r + dr, cc = c + dc;
                if (!valid(P, rr, cc)) continue;
                const u64 key = (u64)(unsigned)(rr * P.w + cc);
                for (int j = lower_bound(s1.ent, ne, key << 32); j < ne && (s1.ent[j] >> 32) == key; ++j) {
                    const unsigned id = (unsigned)(s1.ent[j] & 0xffffffffull);
                    if (id >= (unsigned)n1) continue;   // only a store that was never reset holds such an entry
                    any = true;
                    const double* l1 = s1.lines + 10 * (size_t)id;
                    const double angle = acos(fabs(vdot(vunit_div(vsub(ld3(l1 + 3), ld3(l1))), vunit_div(v2))));
                    if (angle < best_angle) { best = (int)id; best_angle = angle; }
                }
            }
        if (!any) return false;
        if (best_angle / kPi * 180 > 10) return false;
        const double* l1 = s1.lines + 10 * (size_t)best;
        const Vec a1 = ld3(l1), a2 = ld3(l1 + 3);
        d = 0.5 * (dis_from_line(apply(T12, l2p1), a1, a2) + dis_from_line(apply(T12, l2p2), a1, a2));
        return true;
    }
};

// laser_manager::do_match (:244-348) for one robot, per line of s2 in scan::lines order; two passes (mean, then keep)
__global__ void __launch_bounds__(kBlock) k_lfe_match(void* store, Lay L, DP P, int slot1, int slot2, const double* pose1, const double* pose2, int kk,
                                                     int cap, int* count, double* recs, int* idx1, int* idx2, double* match_pose) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B) return;
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    const double* p2 = pose2 + 6 * (size_t)b;
    double* mp = match_pose + 12 * (size_t)b;
    double p1[6];
    int phys1 = slot1;
    if (slot1 == LIW_LFE_REF) {
        if (!m->has_ref) {   // empty_match(p, q)
            for (int k = 0; k < 6; ++k) { mp[k] = p2[k]; mp[6 + k] = p2[k]; }
            count[b] = 0;
            return;
        }
        const int rs = m->ref_sub & 1;
        phys1 = L.slots + rs;
        for (int k = 0; k < 3; ++k) { p1[k] = m->sub_p[rs][k]; p1[3 + k] = m->sub_q[rs][k]; }
    } else {
        for (int k = 0; k < 6; ++k) p1[k] = pose1[6 * (size_t)b + k];
    }
    for (int k = 0; k < 6; ++k) { mp[k] = p1[k]; mp[6 + k] = p2[k]; }
    count[b] = 0;
    const Slot s1 = slot_at(store, L, b, phys1), s2 = slot_at(store, L, b, slot2);
    if (s1.h->status || s2.h->status) { m->status |= LIW_LFE_ST_INVALID; return; }
    const Iso<double> Ti = til(P);
    const Iso<double> T12 = liw::mul(liw::inverse(liw::mul(tf6(p1), Ti)), liw::mul(tf6(p2), Ti));
    const int n2 = n_lines(s2, L), ne = n_entries(s1, L), n1 = n_lines(s1, L);
    const int a = 1 + kk;
    const MatchPair match_pair{P, s1, s2, T12, a, n1, ne};
    double aver = 0;
    int nm = 0;
    for (int i = 0; i < n2; ++i) {
        int best; double d;
        if (match_pair(i, best, d)) { aver += d; ++nm; }
    }
    aver /= (double)nm;
    int n = 0;
    for (int i = 0; i < n2; ++i) {
        int best; double d;
        if (!match_pair(i, best, d)) continue;
        if (!(d < aver * 1.2)) continue;
        if (n >= cap) { m->status |= LIW_LFE_ST_MATCH; count[b] = 0; return; }
        const double* l1 = s1.lines + 10 * (size_t)best;
        const double* l2 = s2.lines + 10 * (size_t)i;
        double* o = recs + ((size_t)b * cap + n) * 12;
        for (int k = 0; k < 6; ++k) { o[k] = l1[k]; o[6 + k] = l2[k]; }
        if (idx1) idx1[(size_t)b * cap + n] = best;
        if (idx2) idx2[(size_t)b * cap + n] = i;
        ++n;
    }
    count[b] = n;
}

// laser_manager::match_with_front for a whole INIT window: one wavefront per (robot, frame) task, task (b, k) =
// k_lfe_match(front_slot, first_slot + k) with frame k's pose at poses + b * rs + k * fs.  Lanes stride over the lines of the
// frame's scan; a lane runs match_pair for its line once (best and d stay in LDS: 12 bytes per line of max_lines).  Two
// steps stay ordered so that the result equals the lane kernel's bit for bit (tests/test_gpu_laser_init.py): the mean
// distance is summed in increasing line order (every lane walks the d values in LDS, so no broadcast is needed), and the kept
// pairs are written in increasing line order by a ballot / prefix count per 64-line chunk on a running base, to which the cap
// test applies.  Outputs are indexed by task: count [B][F], recs [B][F][cap][12], idx1 / idx2 [B][F][cap], match_pose [B][F][12].
__global__ void __launch_bounds__(kBlock) k_lfe_match_wave(void* store, Lay L, DP P, int front_slot, int first_slot, int F, const double* pose_front,
                                                          const double* poses, long long rs, long long fs, int kk, int cap, int* count, double* recs,
                                                          int* idx1, int* idx2, double* match_pose) {
    extern __shared__ __align__(16) unsigned char lds[];
    double* dL = (double*)lds;
    int* bestL = (int*)(lds + 8 * (size_t)L.max_lines);
    const int lane = threadIdx.x;
    const size_t task = blockIdx.x;
    const int b = (int)(task / (unsigned)F), k = (int)(task % (unsigned)F);
    if (b >= L.B) return;
    Mgr* m = (Mgr*)robot_ptr(store, L, b);
    const double* p1 = pose_front + 6 * (size_t)b;
    const double* p2 = poses + (long long)b * rs + (long long)k * fs;
    double* mp = match_pose + 12 * task;
    if (lane < 6) { mp[lane] = p1[lane]; mp[6 + lane] = p2[lane]; }
    const Slot s1 = slot_at(store, L, b, front_slot), s2 = slot_at(store, L, b, first_slot + k);
    if (s1.h->status || s2.h->status) {
        if (lane == 0) { atomicOr(&m->status, LIW_LFE_ST_INVALID); count[task] = 0; }
        return;
    }
    const Iso<double> Ti = til(P);
    const Iso<double> T12 = liw::mul(liw::inverse(liw::mul(tf6(p1), Ti)), liw::mul(tf6(p2), Ti));
    const int n2 = n_lines(s2, L), ne = n_entries(s1, L), n1 = n_lines(s1, L);
    const int a = 1 + kk;
    const MatchPair match_pair{P, s1, s2, T12, a, n1, ne};
    for (int i = lane; i < n2; i += kBlock) {
        int best;
        double d = 0.0;
        if (!match_pair(i, best, d)) best = -1;
        bestL[i] = best;
        dL[i] = d;
    }
    __syncthreads();
    double aver = 0;   // in line order, as the lane kernel sums it
    int nm = 0;
    for (int i = 0; i < n2; ++i)
        if (bestL[i] >= 0) { aver += dL[i]; ++nm; }
    aver /= (double)nm;
    const double thr = aver * 1.2;
    int base = 0;
    for (int c0 = 0; c0 < n2; c0 += kBlock) {
        const int i = c0 + lane;
        const int best = i < n2 ? bestL[i] : -1;
        const bool keep = best >= 0 && dL[i] < thr;
        const u64 mask = __ballot(keep);
        const int n = base + __popcll(mask & ((1ull << lane) - 1));
        if (keep && n < cap) {   // a pair past cap is never written: the match then counts 0
            const double* l1 = s1.lines + 10 * (size_t)best;
            const double* l2 = s2.lines + 10 * (size_t)i;
            double* o = recs + (task * cap + n) * 12;
            for (int q = 0; q < 6; ++q) { o[q] = l1[q]; o[6 + q] = l2[q]; }
            if (idx1) idx1[task * cap + n] = best;
            if (idx2) idx2[task * cap + n] = i;
        }
        base += __popcll(mask);
    }
    if (lane == 0) {
        if (base > cap) { atomicOr(&m->status, LIW_LFE_ST_MATCH); base = 0; }
        count[task] = base;
    }
}

// the component-major laser arrays of a tracking frame from the records of k_lfe_match and the offsets of k_lfe_scan_init (F = 1):
// a thread per (robot, record)
__global__ void __launch_bounds__(256) k_lfe_pack(int B, int n, int frame, int cap, int Ltot, const int* off, const double* recs, const double* match_pose,
                                                 int* laser_frame, double* laser_pts, double* mp_out, unsigned char* has_match) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)B * cap) return;
    const int b = (int)(g / cap), j = (int)(g % cap);
    if (j == 0) {
        for (int k = 0; k < 12; ++k) mp_out[((size_t)b * n + frame) * 12 + k] = match_pose[12 * (size_t)b + k];
        has_match[(size_t)b * n + frame] = 1;
    }
    const int o0 = off[b], cnt = off[b + 1] - o0;
    if (j >= cnt) return;
    const int o = o0 + j;
    laser_frame[o] = frame;
    const double* r = recs + g * 12;
    for (int k = 0; k < 12; ++k) laser_pts[(size_t)k * Ltot + o] = r[k];
}

// laser_off of B windows = exclusive scan over the robots of their F counts, each clamped to [0, cap]; one block of 1024, a
// thread sums a run of consecutive robots.  An INIT window has F = n - 1 (frame 0 has no blocks, so the offset of (b, frame 0) is
// the window's), a tracking frame F = 1 (liw_lfe_pack_track).  With `sel` window r is robot sel[r] (count stays robot-major):
// liw_lfe_pack_init_sel
template <bool SEL> __device__ __forceinline__ void scan_init_body(int B, int F, int cap, const int* count, const int* sel, int* off) {
    __shared__ long long part[1024];
    const int t = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int lo = t * per, hi = lo + per < B ? lo + per : B;
    auto total = [&](int b) {
        const size_t rb = SEL ? (size_t)sel[b] : (size_t)b;
        long long s = 0;
        for (int k = 0; k < F; ++k) { const int c = count[rb * F + k]; s += c < 0 ? 0 : (c > cap ? cap : c); }
        return s;
    };
    long long s = 0;
    for (int b = lo; b < hi; ++b) s += total(b);
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - s;
    for (int b = lo; b < hi; ++b) {
        off[b] = (int)run;
        run += total(b);
    }
    if (t == 1023) off[B] = (int)part[1023];
}
__global__ void __launch_bounds__(1024) k_lfe_scan_init(int B, int F, int cap, const int* count, int* off) {
    scan_init_body<false>(B, F, cap, count, nullptr, off);
}
__global__ void __launch_bounds__(1024) k_lfe_scan_init_sel(int R, int F, int cap, const int* count, const int* sel, int* off) {
    scan_init_body<true>(R, F, cap, count, sel, off);
}

// one work-group per window: the frames' offsets inside the window in LDS (fo [n + 1], frame 0 empty), then a thread per block of
// the window, ascending by owning frame; match_pose / has_match rows of all n frames and init_ok.  With `sel` window b of the output
// is robot sel[b] of the inputs, and the front pose is read at pose_front + robot * front_stride (liw_lfe_pack_init_sel)
template <bool SEL> __device__ __forceinline__ void pack_init_body(int B, int n, int cap, int Ltot, const int* off, const int* count, const double* recs,
                                                                   const double* match_pose, const double* pose_front, long long front_stride,
                                                                   const int* sel, int* laser_frame, double* laser_pts, double* mp_out,
                                                                   unsigned char* has_match, unsigned char* init_ok) {
    extern __shared__ __align__(16) unsigned char lds[];
    int* fo = (int*)lds;
    const int b = blockIdx.x, t = threadIdx.x, F = n - 1;
    if (b >= B) return;
    const size_t rb = SEL ? (size_t)sel[b] : (size_t)b;
    const int* cnt = count + rb * F;
    const double* pf = SEL ? pose_front + (long long)rb * front_stride : pose_front + 6 * rb;
    if (t == 0) {
        int run = 0, ok = 1;
        fo[0] = 0;
        for (int f = 1; f <= F; ++f) {
            fo[f] = run;
            const int c = cnt[f - 1];
            if (c < 2) ok = 0;
            run += c < 0 ? 0 : (c > cap ? cap : c);
        }
        fo[n] = run;
        if (init_ok) init_ok[b] = (unsigned char)ok;
    }
    for (int e = t; e < n * 12; e += 256) {
        const int f = e / 12, q = e % 12;
        mp_out[(size_t)b * n * 12 + e] = f == 0 ? pf[q % 6] : match_pose[(rb * F + f - 1) * 12 + q];
    }
    for (int f = t; f < n; f += 256) has_match[(size_t)b * n + f] = 1;
    __syncthreads();
    const int o0 = off[b], tot = fo[n];
    for (int j = t; j < tot; j += 256) {
        int lo = 1, hi = F;   // the last frame f in 1 .. F with fo[f] <= j
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (fo[mid] <= j) lo = mid; else hi = mid - 1; }
        const int f = lo, o = o0 + j;
        laser_frame[o] = f;
        const double* r = recs + ((rb * F + f - 1) * cap + (j - fo[f])) * 12;
        for (int q = 0; q < 12; ++q) laser_pts[(size_t)q * Ltot + o] = r[q];
    }
}
__global__ void __launch_bounds__(256) k_lfe_pack_init(int B, int n, int cap, int Ltot, const int* off, const int* count, const double* recs,
                                                      const double* match_pose, const double* pose_front, int* laser_frame, double* laser_pts,
                                                      double* mp_out, unsigned char* has_match, unsigned char* init_ok) {
    pack_init_body<false>(B, n, cap, Ltot, off, count, recs, match_pose, pose_front, 6, nullptr, laser_frame, laser_pts, mp_out, has_match, init_ok);
}
__global__ void __launch_bounds__(256) k_lfe_pack_init_sel(int R, int n, int cap, int Ltot, const int* off, const int* count, const double* recs,
                                                          const double* match_pose, const double* pose_front, long long front_stride, const int* sel,
                                                          int* laser_frame, double* laser_pts, double* mp_out, unsigned char* has_match,
                                                          unsigned char* init_ok) {
    pack_init_body<true>(R, n, cap, Ltot, off, count, recs, match_pose, pose_front, front_stride, sel, laser_frame, laser_pts, mp_out, has_match, init_ok);
}

int launch_match(void* store, const Lay& L, const DP& P, int slot1, int slot2, const double* pose1, const double* pose2, int kk, int cap, int* count,
                 double* recs, int* idx1, int* idx2, double* match_pose, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_match, dim3(blocks(L.B, kBlock)), dim3(kBlock), 0, s, store, L, P, slot1, slot2, pose1, pose2, kk, cap, count, recs, idx1, idx2,
                       match_pose);
    return launched();
}

int launch_match_wave(void* store, const Lay& L, const DP& P, int front_slot, int first_slot, int F, const double* pose_front, const double* poses,
                      long long rs, long long fs, int kk, int cap, int* count, double* recs, int* idx1, int* idx2, double* match_pose, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_match_wave, dim3((unsigned)((size_t)L.B * F)), dim3(kBlock), match_lds(L), s, store, L, P, front_slot, first_slot, F,
                       pose_front, poses, rs, fs, kk, cap, count, recs, idx1, idx2, match_pose);
    return launched();
}

int launch_scan_init(int R, int F, int cap, const int* count, const int* sel, int* off, hipStream_t s) {
    if (sel) hipLaunchKernelGGL(k_lfe_scan_init_sel, dim3(1), dim3(1024), 0, s, R, F, cap, count, sel, off);
    else hipLaunchKernelGGL(k_lfe_scan_init, dim3(1), dim3(1024), 0, s, R, F, cap, count, off);
    return launched();
}

int launch_pack(int B, int n, int frame, int cap, int Ltot, const int* off, const double* recs, const double* match_pose, int* laser_frame,
                double* laser_pts, double* mp_out, unsigned char* has_match, hipStream_t s) {
    hipLaunchKernelGGL(k_lfe_pack, dim3(blocks((size_t)B * cap, 256)), dim3(256), 0, s, B, n, frame, cap, Ltot, off, recs, match_pose, laser_frame,
                       laser_pts, mp_out, has_match);
    return launched();
}

int launch_pack_init(int R, int n, int cap, int Ltot, const int* off, const int* count, const double* recs, const double* match_pose,
                     const double* pose_front, long long front_stride, const int* sel, int* laser_frame, double* laser_pts, double* mp_out,
                     unsigned char* has_match, unsigned char* init_ok, hipStream_t s) {
    if (sel)
        hipLaunchKernelGGL(k_lfe_pack_init_sel, dim3(R), dim3(256), pack_init_lds(n), s, R, n, cap, Ltot, off, count, recs, match_pose, pose_front,
                           front_stride, sel, laser_frame, laser_pts, mp_out, has_match, init_ok);
    else
        hipLaunchKernelGGL(k_lfe_pack_init, dim3(R), dim3(256), pack_init_lds(n), s, R, n, cap, Ltot, off, count, recs, match_pose, pose_front,
                           laser_frame, laser_pts, mp_out, has_match, init_ok);
    return launched();
}

}  // namespace lfe
