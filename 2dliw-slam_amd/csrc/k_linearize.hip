// k_linearize.hip — factor residual/Jacobian evaluation + J^T J block partial sums (gfx950, fp64).
//
// One linearisation = three role kernels over every residual block of every window of a batch (or ONE kernel for small
// batches), one wavefront (64-thread work-group) per work item; the roles write disjoint partial slots and run concurrently:
//   (frame transforms: rows 0,1 of make_tf(p,theta) * T_imu_to_laser and d/dtheta_k per (window, frame), dual numbers with a
//                 direction per lane — every exp_so3 of the laser path is hoisted out of the blocks and computed once per wave for
//                 the wave's frames; a separate k_frame_tf launch writing them to HBM was 3 % slower, round 2)
//   k_lin_laser : G (window, owning frame) groups per wave; a LANE is one laser_factor block (reference
//                 src/factor/laser_factor.h:45-89, two point-to-line rows), 64 blocks per pass, coalesced reads of the
//                 component-major end-point arrays, closed-form Jacobian, register accumulation of the pair products
//                 and ONE butterfly reduction per group.
//   k_lin_imu   : six imu_factor blocks per wave (src/factor/imu_factor.h:13-89): 9 dual directions + value lane per
//                 block, closed forms for the linear columns, whitening and Y^T Y on the fp64 matrix cores.
//   k_lin_small : wheel_odom_factor (src/factor/wheel_factor.h:12-73, six blocks per wave, 9 dual directions) and
//                 ground_factor_p/q (src/factor/ground_factor.h:27-82, eight frames per wave); the n-fold duplication
//                 of solver.cpp:142-159 is applied as an integer weight n.
// Every role reduces G = Y^T Y with Y = [J | r] deterministically (no atomics).  G blocks go to the partial-sum slots
// described in liw_kernels.hpp; k_lm.hip assembles them.  Jacobians here are w.r.t. the AMBIENT parameters, exactly like
// auto_diff::compute_res_and_jacobi (src/utilies/common.h:201-217); the so3 local parameterisation is applied at assembly.
#include <type_traits>
#include <cstring>
#include "liw_kernels.hpp"

namespace liw {

// ------------------------------------------------------------------------------------------- laser
// Frame transform record (FTF doubles): rows 0,1 of  make_tf(p,theta) * T_imu_to_laser  and d/dtheta_k, k = 0..2:
//   [0..5] M[2][3]   [6..7] t[2]   [8+6k .. 8+6k+5] dM_k[2][3]   [26+2k .. 26+2k+1] dt_k[2]
// Two records per (window, frame): slot 0 at the frame's own pose, slot 1 at the constant laser_match pose (p1,q1) the
// tracking / marginalisation topologies tie the frame to.  4 lanes per record: 3 derivative directions + the value.
__device__ __forceinline__ void frame_tf_record(const DevParams& P, const double* pose6, int dir, double* o) {
    V3<LJ> p = cast_v3<LJ>(pose6);
    V3<LJ> th(LJ(pose6[3], dir == 0 ? 1.0 : 0.0), LJ(pose6[4], dir == 1 ? 1.0 : 0.0), LJ(pose6[5], dir == 2 ? 1.0 : 0.0));
    Iso<LJ> Twl = mul(make_tf(p, th), cast_iso<LJ>(P.Ril, P.til));
    const LJ tt[2] = {Twl.t.x, Twl.t.y};
    if (dir == 3) {
        for (int r = 0; r < 2; ++r) { for (int c = 0; c < 3; ++c) o[r * 3 + c] = Twl.R(r, c).v; o[6 + r] = tt[r].v; }
    } else {
        for (int r = 0; r < 2; ++r) { for (int c = 0; c < 3; ++c) o[8 + 6 * dir + r * 3 + c] = Twl.R(r, c).d; o[26 + 2 * dir + r] = tt[r].d; }
    }
}
// Wave-wide sums of V per-lane values (V = 32 or 16) in V-1 pair exchanges + log2(64/V) plain steps: each step pairs
// value j with value j + V/2 across the lane bit BIT, halving the values a lane still owns.  Afterwards every lane
// holds the total of value  lane >> log2(64/V).
template <int V, int BIT>
__device__ __forceinline__ void bfly_step(double* v, int lane) {
    if constexpr (V > 1) {
        const bool up = (lane & BIT) != 0;
#pragma unroll
        for (int j = 0; j < V / 2; ++j) {
            const double send = up ? v[j] : v[j + V / 2];
            const double keep = up ? v[j + V / 2] : v[j];
            v[j] = keep + __shfl_xor(send, BIT, 64);
        }
        if constexpr (BIT > 1) bfly_step<V / 2, BIT / 2>(v, lane);
    } else {
        v[0] += __shfl_xor(v[0], BIT, 64);
        if constexpr (BIT > 1) bfly_step<1, BIT / 2>(v, lane);
    }
}

#ifdef LIW_CLK
__device__ long long g_clk_lin[512];
// stamps of one wave in the middle of the grid (so that it runs under load), every memory operation drained first
#define LSTAMP(id) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); if (blockIdx.x == gridDim.x / 2 && lane == 0 && (id) < 512) g_clk_lin[(id)] = clock64(); } while (0)
#else
#define LSTAMP(id) do { } while (0)
#endif
constexpr int LASER_GMAX = 8;   // (window, frame) groups one wave may own

// Laser group kernel.  Columns of a block's two Jacobian rows: the translation columns of the two poses differ only
// in sign (d s/d p_b = - d s/d p_a), so the unique columns are  BOTH: [a_x a_y a_th0..2 b_th0..2 r] (9, 45 pairs),
// one free pose: [b_x b_y b_th0..2 r] (6, 21 pairs).  Every lane accumulates its blocks' pair products in
// registers over all passes; one butterfly per group reduces them across the wave.
template <bool BOTH>
__device__ __forceinline__ void laser_wave_local(const LinArgs& A, const DevParams& P, int G, int vblock) {
    constexpr bool kCostCopy = false;   // (k_lin_all: a few windows, never the per-frame format the compact cost array belongs to)
#include "k_lin_laser_body.inc"
}
template <bool BOTH>
__global__ __launch_bounds__(64, 2) void k_lin_laser(LinArgs A, DevParams P, int G) {
    const int vblock = (int)blockIdx.x;
    constexpr bool kCostCopy = true;
#include "k_lin_laser_body.inc"
}

// ------------------------------------------------------------------------------------------- imu
typedef double d4 __attribute__((ext_vector_type(4)));
typedef LJN<3> J3;
// IMU role.  Only the rotation vectors theta_i, theta_j and the gyro bias bw_i enter the residual (imu_factor.h:41-83) non-linearly:
// 9 derivative directions on THREE lanes per block (3 directions each), 21 blocks per wave, blocks indexed over the whole batch.
// The rotation chain of the gamma rows is  E = exp(-gamma(bw_i)) * exp(-theta_i) * exp(theta_j), and each lane differentiates exactly
// one of the three factors (lane 0: theta_i, lane 1: theta_j, lane 2: bw_i through gamma): the three VALUES are plain doubles, one
// factor per lane carries its 3 derivative directions (exp_so3 on LJN<3>), dE_e = L * dM_e * R with lane-selected double matrices —
// so every sqrt / sin / cos / division of the chain is evaluated once per three directions, and the three derivative chains of a lane
// are independent instructions that hide each other's fp64 latency.  The remaining 21 Jacobian columns are closed forms of R_i^T, Dt
// and the pre-integration Jacobian; they are never materialised: the MFMA operand of the whitening  Y = sqrt_info [J_raw | r_raw]
// (imu_factor.h:85-86) is composed per lane from the compact block record below, and  G = Y^T Y  follows on the matrix cores
// (8 + 12 v_mfma_f64_16x16x4_f64 per block, the accumulator layout of Y being the operand layout of Y^T Y).
// Blocks per wave: 16 (48 of the 64 lanes in the dual-number part) x 135 doubles of LDS each (+ the chain kernel's output staging area)
// = 19.2 kB per wave, so that EIGHT waves fit a CU (two per SIMD, the register limit).  The role is bound by the fp64 pipe its matrix-core and
// vector instructions share (~80 % busy with two waves per SIMD, tools/clk_probe_imu.py), not by HBM: with 21 blocks x 188 doubles
// (31.6 kB, five waves per CU) the kernel took 563 us per 12 288 C2 windows, with the packed inputs alone 3 % less.
constexpr int IMU_PER_WAVE = 16;    // (18 until the chain kernel's output staging area took the room of two blocks)
constexpr int IMU_STAGE = 244;      // k_lin_imu_chain: one frame record's larger part (ij | g_j: 240 doubles) on its way out
constexpr int IMU_SBUF = 128;       // LDS copy of one block's packed sqrt-information triangle (COAL in imu_blocks): 19 232 -> 20 256 B, still eight waves per CU
// compact block record in LDS (doubles): Xc[9][10] = rows alpha, beta, gamma: the 9 derivative columns (theta_i 0-2, theta_j 3-5,
// bw_i 6-8) + r_raw (9); Rb[6] = r_raw of the bias rows (their derivative columns are constants); Rt[9] = R_i^T; RtDt[9];
// Jb[18] = alpha_J_ba (9), beta_J_ba (9)
constexpr int IR_XS = 10, IR_RB = 90, IR_RT = 96, IR_RTDT = 105, IR_JB = 114, IR_K0 = 132, IR_K1 = 133, IR_KM1 = 134, IMU_REC = 135;
// (IR_K0 / IR_K1 / IR_KM1: the constants 0, 1, -1 of the Jacobian as words of the record, so that EVERY operand entry of the matrix-core part is
// one LDS read at a per-lane offset — as (record entry or constant) selects they were ~20 v_cndmask per block; 19.2 kB per wave: still eight per CU)

// column `col` (0..30: x_i 15 | r_raw | x_j 15) of row kk of [J_raw | r_raw] as a record offset (bit 30 = negated); the constant entries
// (0, +-1) are words of the record too (imu_entry_code0 maps the -1-with-constant form of this function onto them)
__host__ __device__ constexpr int imu_entry_code(int kk, int col, double* cst) {
    *cst = 0.0;
    if (kk >= 15 || col > 30) return -1;
    const int rg = kk / 3, rr = kk % 3;
    if (col == 15) return kk < 9 ? kk * IR_XS + 9 : IR_RB + kk - 9;
    const bool second = col > 15;
    const int c = second ? col - 16 : col, grp = c / 3, cc = c % 3;
    if (!second) {
        switch (grp) {
        case 0: return rg == 0 ? IR_RT + rr * 3 + cc : -1;                                            // d r_alpha / d p_i = R_i^T
        case 1: return kk < 9 ? kk * IR_XS + cc : -1;                                                // theta_i
        case 2: return rg == 0 ? IR_RTDT + rr * 3 + cc : (rg == 1 ? IR_RT + rr * 3 + cc : -1);       // v_i
        case 3: if (rg == 0) return IR_JB + rr * 3 + cc; if (rg == 1) return IR_JB + 9 + rr * 3 + cc;
                if (rg == 3 && rr == cc) *cst = -1.0; return -1;                                     // ba_i
        default: if (kk < 9) return kk * IR_XS + 6 + cc;
                 if (rg == 4 && rr == cc) *cst = -1.0; return -1;                                    // bw_i (d res_bw / d bw_i = -I)
        }
    }
    switch (grp) {
    case 0: return rg == 0 ? ((IR_RT + rr * 3 + cc) | (1 << 30)) : -1;                                // p_j: -R_i^T
    case 1: return kk < 9 ? kk * IR_XS + 3 + cc : -1;                                                // theta_j
    case 2: return rg == 1 ? ((IR_RT + rr * 3 + cc) | (1 << 30)) : -1;                                // v_j: -R_i^T
    case 3: if (rg == 3 && rr == cc) *cst = 1.0; return -1;                                          // ba_j
    default: if (rg == 4 && rr == cc) *cst = 1.0; return -1;                                         // bw_j
    }
}

// The operand entry codes of a lane of the matrix-core part (lane = 16 mk + ml: x0 = column ml of [J_raw wrt x_i | r_raw], x1 = column ml
// of [J_raw wrt x_j], rows kk = mk + 4 c) are constants of the lane: a table in constant memory, fetched with the block's inputs.
// Evaluated per wave they were 2.5 k of the 19.8 k cycles of the IMU wave a tracking frame waits for (tools/clk_probe_track.py).
__host__ __device__ constexpr int imu_entry_code0(int kk, int col) {   // always a record offset (| negate flag)
    double k = 0.0;
    const int c = imu_entry_code(kk, col, &k);
    return c >= 0 ? c : (k == 0.0 ? IR_K0 : (k > 0.0 ? IR_K1 : IR_KM1));
}
struct ImuLaneOps { int code0[4], code1[4]; };
struct ImuOpTab { ImuLaneOps lane[64]; };
constexpr ImuOpTab make_imu_optab() {
    ImuOpTab t{};
    for (int l = 0; l < 64; ++l) {
        const int ml = l & 15, mk = l >> 4;
        for (int c = 0; c < 4; ++c) {
            t.lane[l].code0[c] = imu_entry_code0(mk + 4 * c, ml);
            t.lane[l].code1[c] = imu_entry_code0(mk + 4 * c, ml < 15 ? 16 + ml : 31);
        }
    }
    return t;
}
__constant__ ImuOpTab c_imu_optab = make_imu_optab();

__device__ __forceinline__ V3<double> mulc(const double* m, int ld, const V3<double>& v) {   // 3x3 block of a row-major matrix times v
    return V3<double>(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[ld] * v.x + m[ld + 1] * v.y + m[ld + 2] * v.z,
                      m[2 * ld] * v.x + m[2 * ld + 1] * v.y + m[2 * ld + 2] * v.z);
}

// ND = derivative directions per lane: 3 (three lanes per block, 21 blocks per wave: the batched kernels — the value part of the chain
// is evaluated once per three directions) or 1 (nine lanes per block, small batches: a lane's instruction stream is what a single
// window waits for, and one direction instead of three shortens it by ~40 %).  f = the factor of the rotation chain this lane
// differentiates (0: theta_i, 1: theta_j, 2: bw_i through gamma), eg = e0 + e its global direction.
// PK: the block's inputs come from the packed records of the solve in progress (WsView::imu_pk, 1 536 B per block instead of the 3 728 B
// of the caller's X / J / sqrt_inverse_P / Dt arrays: the role is HBM-bound, and those arrays are constant over the LM iterations).
// CHAIN (large batches, per-frame records PIF_*, liw_kernels.hpp): a wave walks CONSECUTIVE blocks of ONE window; the jj tile of block k
// stays in the accumulator registers and enters block k+1's ii product as its MFMA C operand, so every frame's COMPLETE diagonal tile
// is written once and the consumers no longer add a neighbour block's share.  A window of more than IMU_PER_WAVE blocks is split over
// several waves; a wave that starts in the middle of a window evaluates the block in front of its first one once more, for that block's
// jj tile only (a "ghost": nothing of it is stored) — one block in 15 for the 29 blocks of a 30-frame window.
__host__ __device__ inline int imu_chain_parts(int nb) { return nb <= IMU_PER_WAVE ? 1 : (nb + IMU_PER_WAVE - 2) / (IMU_PER_WAVE - 1); }
// MULTI (round 6; CHAIN only, nb <= IMU_PER_WAVE / 2): SEVERAL windows per wave, imu_chain_windows(nb) of them — a two-frame tracking window
// has ONE IMU block, and a wave per window left 15 of its 16 block slots (and 45 of the 48 dual-number lanes) empty: 0.20 ms per 49 152
// two-frame windows against the 0.075 ms the role takes per 49 152 blocks of a C2 batch.  Slot blk = window blk / nb of the wave, block
// blk % nb; the jj -> ii hand-over starts from zero at every window's first block; the window of a block is a lane value, its record
// addresses are formed from scalars read off the block's first lane.  No ghosts (a window never straddles two waves).
__host__ __device__ inline int imu_chain_windows(int nb) { return (nb >= 1 && 2 * nb <= IMU_PER_WAVE) ? IMU_PER_WAVE / nb : 1; }
template <int ND, bool PK = false, bool CHAIN = false, bool MULTI = false>
__device__ __forceinline__ void imu_blocks(const LinArgs& A, const DevParams& P, int wave, double* lds, const int* const act) {
    constexpr int LPB = 9 / ND;
    constexpr int MAXB = 63 / LPB;
    typedef LJN<ND> JN;
    const int lane = threadIdx.x & 63, blk = lane / LPB, g = lane % LPB;
    LSTAMP(299);
    ImuLaneOps ops;
    if constexpr (ND == 1) ops = c_imu_optab.lane[lane];      // a wave per block (latency): in flight with the block's inputs; used by the matrix-core part
    const int f = g / (LPB / 3), e0 = ND == 3 ? 0 : g % 3;
    const int n = A.n, nb = n - 1, ipw = A.imu_per_wave;   // blocks per wave: IMU_PER_WAVE for throughput, fewer for latency
    // blocks are indexed over the windows that are still iterating (compacted list), so finished windows cost no lanes
    // act: the compacted list of the windows still iterating, or null (index by window); the kernel checks that the list is complete
    const long total = (long)(act ? act[0] : A.B) * nb, gb0 = CHAIN ? 0 : (long)wave * ipw;
    int chain_b = 0, chain_k0 = 0, chain_nblk = 0, ghost = 0;
    int multi_w0 = 0;                                      // MULTI: first position of this wave in the list of windows (compacted or all)
    if constexpr (CHAIN && MULTI) {
        if (nb < 1) return;
        const int wpw = imu_chain_windows(nb), cnt = act ? act[0] : A.B;
        multi_w0 = wave * wpw;
        if (multi_w0 >= cnt) return;
        chain_nblk = min(wpw, cnt - multi_w0) * nb;
    } else if constexpr (CHAIN) {
        if (nb < 1) return;
        const int npw = imu_chain_parts(nb), bpw = (nb + npw - 1) / npw;
        const int wiw = wave / npw, part = wave % npw;
        if (wiw >= (act ? act[0] : A.B)) return;
        chain_b = __builtin_amdgcn_readfirstlane(act ? act[1 + wiw] : wiw);
        if (!act && !window_live(A, chain_b)) return;
        const int kfirst = part * bpw, kend = min(nb, kfirst + bpw);
        if (kfirst >= kend) return;
        ghost = part > 0 ? 1 : 0;
        chain_k0 = kfirst - ghost;
        chain_nblk = kend - chain_k0;
    } else {
        if (gb0 >= total) return;
    }
    const long gb = gb0 + blk;
    bool on = CHAIN ? blk < chain_nblk : (blk < ipw && gb < total);
    const int wi = (CHAIN && MULTI) ? (on ? multi_w0 + blk / nb : 0) : ((!CHAIN && on) ? (int)(gb / nb) : 0);
    const int k = (CHAIN && MULTI) ? (on ? blk % nb : 0) : (CHAIN ? (on ? chain_k0 + blk : 0) : (on ? (int)(gb % nb) : 0));
    const int b = (CHAIN && !MULTI) ? chain_b : (act ? act[1 + wi] : wi);
    if ((!CHAIN || MULTI) && on && !act) on = window_live(A, b);
    double* rec = lds + (blk < MAXB ? blk : 0) * IMU_REC;
    const int sel_lane = (on && A.lm) ? (A.candidate ? 1 - A.lm[b].cur : A.lm[b].cur) : 0;   // partial buffer of this lane's block
    const int fk_lane = on ? b * nb + k : 0;                                                   // its record in the input / partial arrays
    // sqrt_info operands of the matrix-core part below (A[i = ml][k = mk + 4c]) are fetched for a whole group of blocks at once, the next
    // group's fetch in flight while this group runs on the matrix cores: three memory round trips per wave instead of one per block.
    // The one-direction instantiation (a wave per block: latency) issues its fetch HERE, ahead of the dual-number part.
    const int ml = lane & 15, mk = lane >> 4;
    const int nblk = CHAIN ? chain_nblk : (int)min((long)ipw, total - gb0);
    // blocks per operand group.  Round 6: 8 (was 7) and BOTH groups of a 16-block wave are fetched in ONE batch in front of the matrix-core loop.
    // As "group g + 1 is fetched while group g runs" every group's fetch was a load-and-wait — the compiler drains vmcnt before the first MFMA
    // of a group (the blocks' conditional stores make the count of outstanding operations unknowable across the loop) —, i.e. three exposed
    // memory round trips per wave: 0.6 of the role's 2.15 ms (probe build with constant operands: 1.56 ms).  One batch = one round trip.
    constexpr int GRP = ND == 3 ? 8 : 1;
    auto load_sop = [&](int gq, double* o) {
        const int fq = __shfl(fk_lane, gq < nblk ? LPB * gq : 0, 64);
        const double* S = PK ? A.imu_pk + (size_t)fq * IMU_PK + IPK_S : A.imu_sqrtP + (size_t)fq * 225;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int kk = mk + 4 * c;
            const bool in = ml < 15 && kk < 15 && (!PK || kk >= ml);          // (packed: row ml of the upper triangle)
            if constexpr (PK) {
                // Round 6: entries outside the triangle READ the record's zero word (IPK_S + 120: k_imu_pack writes 0.0 behind the 120 entries) instead
                // of being selected to 0.0 behind the load.  The select made every prefetched group a load-and-wait: the scheduling fences
                // around the prefetch keep it next to its load, so the NEXT group's 28 loads were waited for before the current group's first
                // MFMA — three exposed memory round trips per 16-block wave, 0.6 of the role's 2.15 ms (probe with constant operands: 1.56 ms).
                o[c] = S[in ? ml * 15 - (ml * (ml - 1)) / 2 + (kk - ml) : 120];
            } else {
                const double v = S[in ? ml * 15 + kk : 0];
                o[c] = in ? v : 0.0;
            }
        }
    };
    static_assert(IPK_S + 120 < IMU_PK, "the packed record's zero word behind the sqrt-information triangle");
    // COAL (round 6, the chain kernels on packed records): a block's sqrt-information triangle is fetched as ONE coalesced 16-byte-per-lane load (61 lanes:
    // 120 entries + the zero word) instead of four gathers of 8 bytes per lane, parked in registers (4 per block) and spread into the MFMA operand
    // layout through a 1-KiB LDS buffer right before the block's products (one ds_write_b128 + four ds_read_b64 at per-lane offsets).
    constexpr bool COAL = CHAIN && PK && ND == 3;
    typedef double __attribute__((ext_vector_type(2))) sraw_t;
    auto load_raw = [&](int gq) -> sraw_t {
        const int fq = __shfl(fk_lane, gq < nblk ? LPB * gq : 0, 64);
        const double* S = A.imu_pk + (size_t)fq * IMU_PK + IPK_S;
        return *reinterpret_cast<const sraw_t*>(S + 2 * (lane < 61 ? lane : 60));
    };
    static_assert((IPK_S * 8) % 16 == 0 && (IMU_PK * 8) % 16 == 0 && IPK_S + 122 <= IMU_PK, "16-byte pieces of the packed sqrt-information triangle");
    sraw_t sraw[COAL ? GRP : 1], srawn[COAL ? GRP : 1];
    int sidx[4];                                       // COAL: this lane's four operand entries as offsets into the LDS copy of the triangle
#pragma unroll
    for (int c = 0; c < 4; ++c) { const int kk = mk + 4 * c; sidx[c] = (ml < 15 && kk < 15 && kk >= ml) ? ml * 15 - (ml * (ml - 1)) / 2 + (kk - ml) : 120; }
    double sop[GRP][4], sopn[GRP][4];
    if constexpr (ND == 1) {
#pragma unroll
        for (int q = 0; q < GRP; ++q) load_sop(q, sop[q]);
    }
    LSTAMP(300);
    if (on) {
        const size_t fk = (size_t)b * nb + k;   // record of this block in the (uncompacted) input / partial arrays
        const double* si_ = A.x + ((size_t)b * n + k) * 15;
        const double* sj_ = si_ + 15;
        // Jp[r * JLD + c], r < 9, 9 <= c < 15: the bias blocks of the pre-integration Jacobian (the only entries the factor reads)
        constexpr int JLD = PK ? 6 : 15;
        const double* pkr = PK ? A.imu_pk + fk * IMU_PK : nullptr;
        const double* Jp = PK ? pkr + IPK_J - 9 : A.imu_J + fk * 225;
        const double* X0 = PK ? pkr : A.imu_X + fk * 15;
        const double Dt = PK ? pkr[IPK_DT] : A.imu_Dt[fk];
        const V3<double> thi = cast_v3<double>(si_ + 3), thj = cast_v3<double>(sj_ + 3);
        const V3<double> dba = cast_v3<double>(si_ + 9) - cast_v3<double>(X0 + 9), dbw = cast_v3<double>(si_ + 12) - cast_v3<double>(X0 + 12);
        const V3<double> gam = cast_v3<double>(X0 + 6) + mulc(Jp + 6 * JLD + 12, JLD, dbw);
        // this lane's differentiated rotation: f = 0 exp(-theta_i), 1 exp(theta_j), 2 exp(-gamma); seeds = d(arg)/d(direction)
        V3<JN> arg;
        {
            const double av[3] = {f == 0 ? -thi.x : (f == 1 ? thj.x : -gam.x), f == 0 ? -thi.y : (f == 1 ? thj.y : -gam.y),
                                  f == 0 ? -thi.z : (f == 1 ? thj.z : -gam.z)};
            JN* ac[3] = {&arg.x, &arg.y, &arg.z};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ac[c]->v = av[c];
#pragma unroll
                for (int e = 0; e < ND; ++e) {
                    const int eg = e0 + e;
                    ac[c]->d[e] = f == 0 ? (c == eg ? -1.0 : 0.0) : (f == 1 ? (c == eg ? 1.0 : 0.0) : -Jp[(6 + c) * JLD + 12 + eg]);
                }
            }
        }
        const M3<JN> Md = exp_so3(arg);
        // The three rotations of the chain as VALUES are the value parts of the three lanes' differentiated factors: fetched from the
        // first lane of each factor (two ds_bpermute per entry) instead of three more exp_so3 per lane (~750 instructions).
        M3<double> Rt, Rj, Eg;                                                    // exp(-theta_i) = bk_R_w, exp(theta_j), exp(-gamma)
        {
            const int l0 = lane - g;                                              // first lane of this block
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                const double mv = Md.m[q].v;
                Rt.m[q] = __shfl(mv, l0, 64);
                Rj.m[q] = __shfl(mv, l0 + LPB / 3, 64);
                Eg.m[q] = __shfl(mv, l0 + 2 * (LPB / 3), 64);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- alpha, beta, ba, bw rows
        {
            const V3<double> pi = cast_v3<double>(si_), vi = cast_v3<double>(si_ + 6), pj = cast_v3<double>(sj_), vj = cast_v3<double>(sj_ + 6);
            const double gD = P.g * Dt;
            const V3<double> va(pj.x - pi.x - vi.x * Dt, pj.y - pi.y - vi.y * Dt, pj.z - pi.z + 0.5 * gD * Dt - vi.z * Dt);
            const V3<double> vb(vj.x - vi.x, vj.y - vi.y, vj.z + gD - vi.z);
            const V3<double> ra = cast_v3<double>(X0) + mulc(Jp + 9, JLD, dba) + mulc(Jp + 12, JLD, dbw) - mul(Rt, va);
            const V3<double> rb = cast_v3<double>(X0 + 3) + mulc(Jp + 3 * JLD + 9, JLD, dba) + mulc(Jp + 3 * JLD + 12, JLD, dbw) - mul(Rt, vb);
#pragma unroll
            for (int e = 0; e < ND; ++e) {
                // f = 0: -(dR_i^T / d theta_i_e) v ; f = 2: the bias Jacobian column ; f = 1: nothing
                const int eg = e0 + e;
                M3<double> dM;
#pragma unroll
                for (int q = 0; q < 9; ++q) dM.m[q] = Md.m[q].d[e];
                const V3<double> da = mul(dM, va), db = mul(dM, vb);
                const double ca[3] = {f == 0 ? -da.x : (f == 2 ? Jp[0 * JLD + 12 + eg] : 0.0), f == 0 ? -da.y : (f == 2 ? Jp[1 * JLD + 12 + eg] : 0.0),
                                      f == 0 ? -da.z : (f == 2 ? Jp[2 * JLD + 12 + eg] : 0.0)};
                const double cb[3] = {f == 0 ? -db.x : (f == 2 ? Jp[3 * JLD + 12 + eg] : 0.0), f == 0 ? -db.y : (f == 2 ? Jp[4 * JLD + 12 + eg] : 0.0),
                                      f == 0 ? -db.z : (f == 2 ? Jp[5 * JLD + 12 + eg] : 0.0)};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    rec[r * IR_XS + 3 * f + eg] = ca[r];
                    rec[(3 + r) * IR_XS + 3 * f + eg] = cb[r];
                    // (res_ba has no non-linear direction, d res_bw / d bw_i = -I: constants of imu_entry_code)
                }
            }
            if (g == 0) {
                const double r3[3][3] = {{ra.x, ra.y, ra.z}, {rb.x, rb.y, rb.z}, {0.0, 0.0, 0.0}};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    rec[r * IR_XS + 9] = r3[0][r];
                    rec[(3 + r) * IR_XS + 9] = r3[1][r];
                    rec[IR_RB + r] = sj_[9 + r] - si_[9 + r];                                 // res_ba
                    rec[IR_RB + 3 + r] = sj_[12 + r] - si_[12 + r];                           // res_bw
                }
                rec[IR_K0] = 0.0; rec[IR_K1] = 1.0; rec[IR_KM1] = -1.0;
#pragma unroll
                for (int q = 0; q < 9; ++q) {
                    rec[IR_RT + q] = Rt.m[q];
                    rec[IR_RTDT + q] = Rt.m[q] * Dt;
                    rec[IR_JB + q] = Jp[(q / 3) * JLD + 9 + q % 3];                             // alpha_J_ba
                    rec[IR_JB + 9 + q] = Jp[(3 + q / 3) * JLD + 9 + q % 3];                     // beta_J_ba
                }
            }
        }
        LSTAMP(302);
        __builtin_amdgcn_sched_barrier(0);
        // ---- gamma rows: log( exp(-gamma^) R_i^T R_j )
        {
            const M3<double> RtRj = mul(Rt, Rj), EgRt = mul(Eg, Rt);
            M3<double> Lm, Rm;   // dE_e = Lm * dM_e * Rm
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                const double id = (q % 4 == 0) ? 1.0 : 0.0;
                Lm.m[q] = f == 2 ? id : (f == 1 ? EgRt.m[q] : Eg.m[q]);
                Rm.m[q] = f == 0 ? Rj.m[q] : (f == 1 ? id : RtRj.m[q]);
            }
            const M3<double> Ev = mul(Eg, RtRj);
            M3<JN> E;
#pragma unroll
            for (int q = 0; q < 9; ++q) E.m[q].v = Ev.m[q];
#pragma unroll
            for (int e = 0; e < ND; ++e) {
                M3<double> dM;
#pragma unroll
                for (int q = 0; q < 9; ++q) dM.m[q] = Md.m[q].d[e];
                const M3<double> dE = mul(mul(Lm, dM), Rm);
#pragma unroll
                for (int q = 0; q < 9; ++q) E.m[q].d[e] = dE.m[q];
            }
            __builtin_amdgcn_sched_barrier(0);
            const V3<JN> rg = log_SO3(E);
            const JN* rr[3] = {&rg.x, &rg.y, &rg.z};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int e = 0; e < ND; ++e) rec[(6 + r) * IR_XS + 3 * f + e0 + e] = rr[r]->d[e];
                if (g == 0) rec[(6 + r) * IR_XS + 9] = rr[r]->v;
            }
        }
        LSTAMP(303);
    }
    lds_sync();
    LSTAMP(304);
    // ---- matrix-core part, one block at a time (the whole wave cooperates).  Operand entry codes of this lane: x0 = column ml of
    // [J_raw wrt x_i | r_raw], x1 = column ml of [J_raw wrt x_j] for the four k-chunks (row kk = mk + 4c)
    if constexpr (ND != 1) ops = c_imu_optab.lane[lane];      // (throughput kernels: 24 registers that must not live across the dual-number part)
    int off0[4], off1[4], sgn1[4];    // record offsets of this lane's eight operand entries; sign bit of the x_j entries that are -R_i^T
#pragma unroll
    for (int c = 0; c < 4; ++c) { off0[c] = ops.code0[c] & 0xffff; off1[c] = ops.code1[c] & 0xffff; sgn1[c] = (ops.code1[c] >> 30) << 31; }
    const unsigned long long onmask = __ballot(on);           // lane LPB q = block q is live (in range, window still iterating)
    d4 chain11 = {0.0, 0.0, 0.0, 0.0};                         // CHAIN: the jj tile of the block before (zero in front of a window's first block)
    // CHAIN: staging offsets of this lane's accumulator entries (row = mk + 4 r, column ml): ij | g_j image at row * 15 + ml (row 15 = the
    // gradient row g_j at 225 + ml), diagonal image at the packed-triangle index (column 15 = g_i at 120 + row); no word: the spare one
    constexpr int IMU_SPARE = 242;                             // (a pad word of the 244-double staging area)
    int so_ij[4], so_d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = mk + 4 * r;
        so_ij[r] = ml < 15 ? row * 15 + ml : IMU_SPARE;        // (row <= 15)
        so_d[r] = row < 15 ? (ml == 15 ? 120 + row : (ml >= row ? row * 15 - (row * (row - 1)) / 2 + (ml - row) : IMU_SPARE)) : IMU_SPARE;
    }
    if constexpr (COAL) {
#pragma unroll
        for (int q = 0; q < GRP; ++q) sraw[q] = load_raw(q);
#pragma unroll
        for (int q = 0; q < GRP; ++q) srawn[q] = load_raw(GRP + q);
    } else if constexpr (ND == 3) {
        static_assert(2 * 8 >= IMU_PER_WAVE, "two operand groups cover a wave's blocks");
#pragma unroll
        for (int q = 0; q < GRP; ++q) load_sop(q, sop[q]);
#pragma unroll
        for (int q = 0; q < GRP; ++q) load_sop(GRP + q, sopn[q]);      // (a slot beyond nblk re-reads block 0's record: a valid address, never used)
    }
    for (int g0 = 0; g0 < nblk; g0 += GRP) {
        LSTAMP(305 + g0 / GRP);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ND != 3) {
            if (g0 + GRP < nblk) {
#pragma unroll
                for (int q = 0; q < GRP; ++q) load_sop(g0 + GRP + q, sopn[q]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < GRP; ++q) {
            const int gq = g0 + q;
            if (gq >= nblk || !((onmask >> (LPB * gq)) & 1ull)) continue;
            const double* R_ = lds + gq * IMU_REC;
            d4 y0 = {0.0, 0.0, 0.0, 0.0}, y1 = {0.0, 0.0, 0.0, 0.0};
            double sq[4];
            if constexpr (COAL) {
                double* const sbuf = lds + IMU_PER_WAVE * IMU_REC + IMU_STAGE;      // 128 doubles behind the output staging area
                *reinterpret_cast<sraw_t*>(sbuf + 2 * lane) = sraw[q];
                lds_sync();
#pragma unroll
                for (int c = 0; c < 4; ++c) sq[c] = sbuf[sidx[c]];
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) sq[c] = sop[q][c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double x0v = R_[off0[c]], l1 = R_[off1[c]];
                const double x1v = __hiloint2double(__double2hiint(l1) ^ sgn1[c], __double2loint(l1));
                y0 = __builtin_amdgcn_mfma_f64_16x16x4f64(sq[c], x0v, y0, 0, 0, 0);
                y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(sq[c], x1v, y1, 0, 0, 0);
            }
            // y_t[r] = Y[mk + 4r][ml + 16t]  ==  operand chunk r of Y^T Y
            d4 g00 = {0.0, 0.0, 0.0, 0.0}, g01 = g00, g11 = g00;
            if constexpr (CHAIN && MULTI) { if (gq % nb == 0) chain11 = d4{0.0, 0.0, 0.0, 0.0}; }   // a window's first block: no block before it
            if constexpr (CHAIN) g00 = chain11;   // + jj of the block before: frame k's diagonal tile is complete when this product is
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                g00 = __builtin_amdgcn_mfma_f64_16x16x4f64(y0[c], y0[c], g00, 0, 0, 0);
                g01 = __builtin_amdgcn_mfma_f64_16x16x4f64(y0[c], y1[c], g01, 0, 0, 0);
                g11 = __builtin_amdgcn_mfma_f64_16x16x4f64(y1[c], y1[c], g11, 0, 0, 0);
            }
            // (the block's record index and partial buffer are the same in every lane: as SCALARS, so that the output addresses below are a
            // scalar base + a 32-bit lane offset — as lane values every store paid a 64-bit select between the two buffers and a 64-bit
            // shift-and-add: ~1 400 of the kernel's 11 600 instructions)
            const size_t fg = (size_t)__builtin_amdgcn_readfirstlane(__shfl(fk_lane, LPB * gq, 64));
            const int sel = __builtin_amdgcn_readfirstlane(__shfl(sel_lane, LPB * gq, 64));
            if constexpr (CHAIN) {
                chain11 = g11;
                if (ghost && gq == 0) continue;   // evaluated for its jj tile only
                // frame kq's record: diagonal tile (upper triangle), gradient part of block (kq, kq+1); frame kq+1's: coupling, gradient
                // part and cost of the block; behind a window's last block the jj tile is frame n-1's diagonal
                const int kq = MULTI ? gq % nb : chain_k0 + gq;
                const int bq = MULTI ? (int)(fg / (size_t)nb) : b;            // the block's window (fg = window * nb + block: scalar)
                double* rf = (sel ? A.PI[1] : A.PI[0]) + ((size_t)bq * n + kq) * PIFS;
                const bool lastb = kq == nb - 1;
                // The tiles leave through LDS: in the accumulator layout a store instruction covers four 15-double row segments of a tile
                // (~8 lines, ~20 masked instructions and ~160 line writes per block for a 3-kB record: 0.22 of the kernel's 1.10 ms per
                // 24 576 windows went into them); staged, the same doubles go out as 16 bytes per lane on consecutive addresses — ij | g_j
                // (240 doubles, slots 120 .. 359 of frame kq+1's record) in two instructions, the diagonal triangle (120) in one, g_i in one.
                double* const img = lds + IMU_PER_WAVE * IMU_REC;
                typedef double __attribute__((ext_vector_type(2))) dbl2;
                auto flush = [&](double* dst, int nd) {          // nd doubles (even) from img to dst, 16 bytes per lane
                    lds_sync();
                    for (int e = 2 * lane; e < nd; e += 128) nt_store(reinterpret_cast<dbl2*>(dst + e), *reinterpret_cast<const dbl2*>(img + e));
                    lds_sync();
                };
                // staging writes are UNCONDITIONAL: every lane's four (tile row group -> staging word) offsets are constants of the wave
                // (so_ij / so_d below, built once), lanes without a word of theirs write a spare word.  As `if (row < 15 && ml < 15 ...)` each of the
                // ~20 writes of a block sat under its own exec mask: ~150 scalar mask / branch instructions per block (round 5, ISA count)
#pragma unroll
                for (int r = 0; r < 4; ++r) img[so_ij[r]] = g01[r];
                flush(rf + PIFS + PIF_IJ, 240);
                static_assert(PIF_GJ == PIF_IJ + 225 && PIF_IJ % 2 == 0 && PIFS % 2 == 0 && PIF_GI % 2 == 0, "staged ranges");
                auto diag_out = [&](const d4& gd, double* rec, bool with_gi) {   // upper triangle of a diagonal tile -> slots 0 .. 119, its column 15 -> g_i
#pragma unroll
                    for (int r = 0; r < 4; ++r) img[so_d[r]] = (ml == 15 && !with_gi) ? 0.0 : gd[r];
                    lds_sync();
                    if (lane < 60) nt_store(reinterpret_cast<dbl2*>(rec + PIF_D + 2 * lane), *reinterpret_cast<const dbl2*>(img + 2 * lane));
                    if (lane < 15) rec[PIF_GI + lane] = img[120 + lane];
                    lds_sync();
                };
                diag_out(g00, rf, true);
                if (lastb) diag_out(g11, rf + PIFS, false);
                if (mk == 3 && ml == 15) { rf[PIFS + PIF_C] = g00[3]; if (A.CS[0]) (sel ? A.CS[1] : A.CS[0])[cs_index(n, bq, CS_IMU, kq)] = g00[3]; }
                continue;
            }
            double* out = (sel ? A.PI[1] : A.PI[0]) + fg * PIS;   // (a select, not an indexed load: an indexed kernel argument sends the whole struct through scratch)
            // tile (0,0) = [ii | gradient_i ; . | cost], tile (0,1) = [ij ; gradient_j], tile (1,1) = jj: one masked store per tile row group
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mk + 4 * r;
                if (row < 15 && ml < 15) {
                    out[PI_IJ + row * 15 + ml] = g01[r];
                    if (ml >= row) {   // symmetric blocks: upper triangle only
                        const int tq = row * 15 - (row * (row - 1)) / 2 + (ml - row);
                        out[PI_II + tq] = g00[r];
                        out[PI_JJ + tq] = g11[r];
                    }
                }
                if (row < 15 && ml == 15) out[PI_G + row] = g00[r];
                if (r == 3) {
                    if (row == 15 && ml < 15) out[PI_G + 15 + ml] = g01[r];
                    if (row == 15 && ml == 15) out[PI_C] = g00[r];
                }
                if (A.dbg_imu_res && ml == 15 && row < 15) A.dbg_imu_res[fg * 15 + row] = y0[r];
                if (A.dbg_imu_jac && row < 15 && ml < 15) {
                    A.dbg_imu_jac[(fg * 15 + row) * 30 + ml] = y0[r];
                    A.dbg_imu_jac[(fg * 15 + row) * 30 + 15 + ml] = y1[r];
                }
            }
        }
        if constexpr (COAL) {
#pragma unroll
            for (int q = 0; q < GRP; ++q) sraw[q] = srawn[q];
        } else {
#pragma unroll
            for (int q = 0; q < GRP; ++q)
#pragma unroll
                for (int c = 0; c < 4; ++c) sop[q][c] = sopn[q][c];
        }
    }
    LSTAMP(311);
}

// ------------------------------------------------------------------------------------------- wheel
// 21 blocks per wave, three lanes each: lane 0 the 3 directions of theta_i, lane 1 theta_j, lane 2 the RELATIVE translation.
// The positions enter the residual only through p = R_wi^T (p_j - p_i) + c(theta), R_wi = R_i R_imu_to_wheel, so
// d res / d p_j = (d res / d p) R_wi^T and d res / d p_i = -(d res / d p_j): three directions instead of six.
// As in the IMU role every lane differentiates ONE rotation (lane 0 R_i, lane 1 R_j; lane 2 none) and the relative pose
//   R_rel = R_iw^T R_i^T R_j R_iw,   t_rel = R_iw^T R_i^T (R_j t_iw + p_j - p_i) - R_iw^T t_iw      (wheel_factor.h:29-34)
// gets its derivative parts as  L * dM_e * R  with lane-selected double matrices; only log_SO3 and the scalar tail of the residual
// run on LJN<3>.
constexpr int WHEEL_PER_WAVE = 21;
// record entry e -> columns (r, c) of Y = [J (3 x 12) | r] as (r << 8) | c: ii | ij | jj | gradient | cost (liw_kernels.hpp); -1 = padding.
// A table in constant memory (built per wave in LDS until round 5: divisions and searches, ~20 of the ~45 instructions of an output element
// before that).
struct WheelRcTab { int e[PWS]; };
constexpr WheelRcTab make_wheel_rc() {
    WheelRcTab t{};
    for (int e = 0; e < PWS; ++e) {
        int r = 12, c = 12;                                   // e == PW_C: sum r^2
        if (e < PW_IJ(0, 0) || (e >= PW_JJ(0, 0) && e < PW_G(0))) {   // packed upper triangles of ii / jj: row r has 6 - r entries
            const int jj = e >= PW_JJ(0, 0);
            int q = e - (jj ? PW_JJ(0, 0) : 0);
            r = 0;
            while (q >= 6 - r) { q -= 6 - r; ++r; }
            c = r + q + (jj ? 6 : 0); r += jj ? 6 : 0;
        } else if (e < PW_JJ(0, 0)) { r = (e - PW_IJ(0, 0)) / 6; c = 6 + (e - PW_IJ(0, 0)) % 6; }
        else if (e < PW_C) { r = e - PW_G(0); c = 12; }
        t.e[e] = e <= PW_C ? (r << 8) | c : -1;
    }
    return t;
}
__constant__ WheelRcTab c_wheel_rc = make_wheel_rc();
template <int ND, bool COSTCOPY>   // directions per lane: 3 (three lanes per block) or 1 (nine lanes per block, small batches), as in imu_blocks; COSTCOPY: see CS in LinArgs
__device__ __forceinline__ void wheel_blocks(const LinArgs& A, const DevParams& P, int wave, double* lds, const int* const act) {
    constexpr int LPB = 9 / ND;
    constexpr int MAXB = 63 / LPB;
    typedef LJN<ND> JN;
    const int lane = threadIdx.x & 63, blk = lane / LPB, g = lane % LPB;
    const int f = g / (LPB / 3), e0 = ND == 3 ? 0 : g % 3;   // f: 0 theta_i, 1 theta_j, 2 the relative translation; eg = e0 + e
    const int n = A.n, nb = n - 1;
    const long total = (long)(act ? act[0] : A.B) * nb, gb = (long)wave * A.small_per_wave + blk;   // over the windows still iterating
    bool on = blk < A.small_per_wave && gb < total;
    const int wi = on ? (int)(gb / nb) : 0, k = on ? (int)(gb % nb) : 0;
    const int b = act ? act[1 + wi] : wi;
    if (on && !act) on = window_live(A, b);
    double* Y = lds + (blk < MAXB ? blk : 0) * 64;   // [3][13] then Dp [3][3] at 40, R_wi [3][3] at 49
    const size_t fk = on ? (size_t)b * nb + k : 0;
    if (on) {
        const double* si_ = A.x + ((size_t)b * n + k) * 15;
        const double* sj_ = si_ + 15;
        const double* T12 = A.wheel_T + fk * 12;
        const double* sq9 = A.wheel_sqrtP + fk * 9;
        const V3<double> thi = cast_v3<double>(si_ + 3), thj = cast_v3<double>(sj_ + 3);
        V3<JN> arg;   // the rotation this lane differentiates (f = 2: R_i with zero seeds)
        {
            JN* ac[3] = {&arg.x, &arg.y, &arg.z};
            const double av[3] = {f == 1 ? thj.x : thi.x, f == 1 ? thj.y : thi.y, f == 1 ? thj.z : thi.z};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                *ac[c] = JN(av[c]);
#pragma unroll
                for (int e = 0; e < ND; ++e) if (f < 2 && c == e0 + e) ac[c]->d[e] = 1.0;
            }
        }
        const M3<JN> Md = exp_so3(arg);
        // R_i, R_j as values = the value parts of the differentiated rotations of the f = 0 (and f = 2: same argument) / f = 1 lanes
        M3<double> Ri, Rj;
        {
            const int l0 = lane - g;
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                const double mv = Md.m[q].v;
                Ri.m[q] = __shfl(mv, l0, 64);
                Rj.m[q] = __shfl(mv, l0 + LPB / 3, 64);
            }
        }
        const M3<double> Riw = cast_m3<double>(P.Riw);
        const V3<double> tiw(P.tiw[0], P.tiw[1], P.tiw[2]);
        const M3<double> Rwi = mul(Ri, Riw);                      // tf_i.R
        const M3<double> Am = transpose(Rwi);                     // R_iw^T R_i^T
        const M3<double> RjRiw = mul(Rj, Riw);
        const V3<double> Rjt = mul(Rj, tiw);
        const V3<double> w(Rjt.x + sj_[0] - si_[0], Rjt.y + sj_[1] - si_[1], Rjt.z + sj_[2] - si_[2]);
        const M3<double> Rrel = mul(Am, RjRiw);
        const V3<double> trel = mul(Am, w) - mulT(Riw, tiw);
        M3<JN> E;
        V3<JN> p;
#pragma unroll
        for (int q = 0; q < 9; ++q) E.m[q] = JN(Rrel.m[q]);
        p.x = JN(trel.x); p.y = JN(trel.y); p.z = JN(trel.z);
        {
            const M3<double> RiwT = transpose(Riw);
            M3<double> Lm, Rm;
#pragma unroll
            for (int q = 0; q < 9; ++q) { Lm.m[q] = f == 0 ? RiwT.m[q] : Am.m[q]; Rm.m[q] = f == 0 ? RjRiw.m[q] : Riw.m[q]; }
            const V3<double> wv(f == 0 ? w.x : tiw.x, f == 0 ? w.y : tiw.y, f == 0 ? w.z : tiw.z);
#pragma unroll
            for (int e = 0; e < ND; ++e) {
                const int eg = e0 + e;
                M3<double> X;   // f = 0: (dR_i / d theta_i_e)^T, f = 1: dR_j / d theta_j_e
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) X(r, c) = f == 0 ? Md(c, r).d[e] : Md(r, c).d[e];
                const M3<double> LX = mul(Lm, X);
                const M3<double> dR = mul(LX, Rm);
                const V3<double> dt = mul(LX, wv);
#pragma unroll
                for (int q = 0; q < 9; ++q) E.m[q].d[e] = f < 2 ? dR.m[q] : 0.0;
                p.x.d[e] = f < 2 ? dt.x : (eg == 0 ? 1.0 : 0.0);
                p.y.d[e] = f < 2 ? dt.y : (eg == 1 ? 1.0 : 0.0);
                p.z.d[e] = f < 2 ? dt.z : (eg == 2 ? 1.0 : 0.0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // wheel_odom_factor::operator() from (p, q) on (wheel_factor.h:36-70)
        const V3<JN> q = log_SO3(E);
        const V3<double> oq = log_SO3(cast_m3<double>(T12));      // log_SE3 of the constant odometry increment: plain doubles
        const double opx = T12[9], opy = T12[10];
        const double o_len = sqrt(opx * opx + opy * opy);
        const JN len = dsqrt(p.x * p.x + p.y * p.y);
        JN res[3];
        JN angle(0.0);
        if (o_len > 0.0001 && len.v > 0.0001) {
            const double odx = opx / o_len, ody = opy / o_len;     // normalized(o_dir)
            const JN dx = p.x / len, dy = p.y / len;
            // |cross(o_dir, dir)| with both in the plane: |o_x d_y - o_y d_x| through norm() = sqrt(z^2), as the reference computes it
            const JN cz = dy * odx - dx * ody;
            angle = dasin(dsqrt(cz * cz));
        } else {
            angle = len;
        }
        if (len.v < 0.0001 || o_len < 0.0001) res[0] = len * sq9[0];
        else res[0] = (JN(o_len) - len) * sq9[0];
        res[1] = angle * sq9[4];
        const JN nq = norm(q);
        const double noq = sqrt(oq.x * oq.x + oq.y * oq.y + oq.z * oq.z);
        if (nq.v < 0.001 || noq < 0.001) res[2] = nq * sq9[8];
        else res[2] = (JN(noq) - nq) * sq9[8];
#pragma unroll
        for (int e = 0; e < ND; ++e) {
            // f = 0 -> columns theta_i (3..5), f = 1 -> theta_j (9..11), f = 2 -> Dp
            const int eg = e0 + e;
            const int col = f == 0 ? 3 + eg : (f == 1 ? 9 + eg : 0);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                if (f < 2) Y[r * 13 + col] = res[r].d[e];
                else Y[40 + r * 3 + eg] = res[r].d[e];
            }
        }
        if (g == 0) {
#pragma unroll
            for (int r = 0; r < 3; ++r) Y[r * 13 + 12] = res[r].v;
#pragma unroll
            for (int qq = 0; qq < 9; ++qq) Y[49 + qq] = Rwi.m[qq];
        }
    }
    lds_sync();
    if (on && g < 3) {   // position columns: Y[r][p_j c] = sum_k Dp[r][k] R_wi[c][k],  Y[r][p_i c] = -Y[r][p_j c]   (row r = g of this lane)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = Y[40 + g * 3] * Y[49 + c * 3] + Y[40 + g * 3 + 1] * Y[49 + c * 3 + 1] + Y[40 + g * 3 + 2] * Y[49 + c * 3 + 2];
            Y[g * 13 + 6 + c] = v;
            Y[g * 13 + c] = -v;
        }
    }
    lds_sync();
    if (on && g == 0 && A.dbg_wheel_res)
        for (int r = 0; r < 3; ++r) A.dbg_wheel_res[fk * 3 + r] = Y[r * 13 + 12];
    if (on && A.dbg_wheel_jac)
        for (int e = g; e < 36; e += LPB) A.dbg_wheel_jac[fk * 36 + e] = Y[(e / 12) * 13 + e % 12];
    // G = Y^T Y (13 x 13 per block), written with consecutive lanes on consecutive addresses: the blocks of a wave are consecutive
    // records of the partial buffer, so the wave's output is one contiguous region (a lane-per-pair scatter doubled the HBM write
    // traffic of this role)
    int* meta = reinterpret_cast<int*>(lds + WHEEL_PER_WAVE * 64);   // per block: partial buffer (0 / 1) or -1 = skip; then its record index
    if (g == 0 && blk < MAXB) {
        meta[blk] = on ? (A.lm ? (A.candidate ? 1 - A.lm[b].cur : A.lm[b].cur) : 0) : -1;
        meta[32 + blk] = (int)fk;
        meta[64 + blk] = (int)cs_index(n, b, CS_WHEEL, k);   // its slot of the compact cost array
    }
    lds_sync();
    {   // a record (PWS = 92 doubles) leaves as 46 lanes x 16 bytes, one store per block; a lane's two (r, c) pairs are fixed for the
        // wave and the block meta words sit in registers (lane q holds block q's, read by v_readlane), so a block costs twelve LDS reads
        // at addresses known up front instead of four dependent LDS round trips per element (block meta -> (r, c) -> Y -> record index)
        const long gb0 = (long)wave * A.small_per_wave;
        const int nblk = (int)min((long)A.small_per_wave, total - gb0);
        const int ml = lane < MAXB ? lane : 0;
        const int selv = meta[ml], fkv = meta[32 + ml], csv = meta[64 + ml];
        const bool all_on = __builtin_amdgcn_ballot_w64(lane < nblk && selv < 0) == 0;   // (uniform; false only without the list of live windows)
        if (lane < PWS / 2) {
            const int rc0 = c_wheel_rc.e[2 * lane], rc1 = c_wheel_rc.e[2 * lane + 1];
            const int r0 = rc0 >> 8, c0 = rc0 & 255;
            const int r1 = rc1 >= 0 ? rc1 >> 8 : 0, c1 = rc1 >= 0 ? rc1 & 255 : 0;
            auto block = [&](int q) {
                const double* Yq = lds + q * 64;
                double2 v;
                v.x = __builtin_fma(Yq[26 + r0], Yq[26 + c0], __builtin_fma(Yq[r0], Yq[c0], Yq[13 + r0] * Yq[13 + c0]));
                const double w1 = __builtin_fma(Yq[26 + r1], Yq[26 + c1], __builtin_fma(Yq[r1], Yq[c1], Yq[13 + r1] * Yq[13 + c1]));
                v.y = rc1 >= 0 ? w1 : 0.0;                     // entry 91 is padding
                return v;
            };
            auto put = [&](int q, const double2& v) {
                const int sel = __builtin_amdgcn_readlane(selv, q);
                *reinterpret_cast<double2*>(&(sel ? A.PW[1] : A.PW[0])[(size_t)__builtin_amdgcn_readlane(fkv, q) * PWS + 2 * lane]) = v;
            };
            int q = 0;
            if (all_on)
                for (; q + 3 <= nblk; q += 3) {                // three blocks' LDS reads in flight (21 blocks per wave)
                    const double2 va = block(q), vb = block(q + 1), vc = block(q + 2);
                    put(q, va); put(q + 1, vb); put(q + 2, vc);
                }
            for (; q < nblk; ++q) {
                const double2 v = block(q);
                if (__builtin_amdgcn_readlane(selv, q) >= 0) put(q, v);
            }
        }
        if (COSTCOPY && A.CS[0] && lane < nblk && selv >= 0) {   // compact cost array: lane q writes block q's sum r^2, the same operations as record entry PW_C
            const double* Yq = lds + lane * 64;
            (selv ? A.CS[1] : A.CS[0])[csv] = __builtin_fma(Yq[38], Yq[38], __builtin_fma(Yq[12], Yq[12], Yq[25] * Yq[25]));
        }
    }
}

// ------------------------------------------------------------------------------------------- ground
// ground_factor_p / ground_factor_q, src/factor/ground_factor.h:27-48, :59-82: height of the wheel-frame origin and tilt of its z axis,
// tf_w_o = make_tf(p, theta) * T_imu_to_wheel
// 32 frames per wave, two lanes each: lane 0 the 3 directions of p, lane 1 of theta
constexpr int GROUND_PER_WAVE = 32;
struct GroundRcTab { int e[PGS]; };   // record entry e -> (r << 8) | c of the packed upper triangle of the 7 x 7 G (PG_H / PG_G / PG_C)
constexpr GroundRcTab make_ground_rc() {
    GroundRcTab t{};
    for (int e = 0; e < PGS; ++e) {
        int r = 0, c = e;
        while (c >= 7 - r) { c -= 7 - r; ++r; }               // row r has 7 - r entries
        t.e[e] = (r << 8) | (c + r);
    }
    return t;
}
__constant__ GroundRcTab c_ground_rc = make_ground_rc();
template <bool COSTCOPY>
__device__ __forceinline__ void ground_frames(const LinArgs& A, const DevParams& P, int wave, double* lds, const int* const act) {
    const int lane = threadIdx.x & 63, sub = lane >> 1, g = lane & 1;
    const int n = A.n;
    const long total = (long)(act ? act[0] : A.B) * n, gf = (long)wave * GROUND_PER_WAVE + sub;
    bool on = gf < total;
    const int wi = on ? (int)(gf / n) : 0;
    const int b = act ? act[1 + wi] : wi;
    if (on && !act) on = window_live(A, b);
    double* Y = lds + sub * 16;   // [2][7]
    const size_t fi = on ? (size_t)b * n + (size_t)(gf % n) : 0;
    if (on) {
        const double* s_ = A.x + fi * 15;
        J3 res[2];
        {
            V3<J3> q;
            q.x = seed<3>(s_[3], 0, g == 1); q.y = seed<3>(s_[4], 1, g == 1); q.z = seed<3>(s_[5], 2, g == 1);
            const M3<J3> R = exp_so3(q);
            const J3 pz = seed<3>(s_[2], 2, g == 0);
            res[0] = (R(2, 0) * P.tiw[0] + R(2, 1) * P.tiw[1] + R(2, 2) * P.tiw[2] + pz) * P.ground_p_info;
            // z axis of the wheel frame in the world; |z x e3| = sqrt(z_x^2 + z_y^2)
            const J3 zx = R(0, 0) * P.Riw[2] + R(0, 1) * P.Riw[5] + R(0, 2) * P.Riw[8];
            const J3 zy = R(1, 0) * P.Riw[2] + R(1, 1) * P.Riw[5] + R(1, 2) * P.Riw[8];
            res[1] = dasin(dsqrt(zy * zy + zx * zx)) * P.ground_q_info;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) { Y[3 * g + e] = res[0].d[e]; Y[7 + 3 * g + e] = res[1].d[e]; }
        if (g == 0) { Y[6] = res[0].v; Y[13] = res[1].v; }
        if (g == 0 && A.dbg_ground_res) { A.dbg_ground_res[fi * 2] = res[0].v; A.dbg_ground_res[fi * 2 + 1] = res[1].v; }
        if (A.dbg_ground_jac)
            for (int e = 0; e < 3; ++e) { A.dbg_ground_jac[(fi * 2) * 6 + 3 * g + e] = res[0].d[e]; A.dbg_ground_jac[(fi * 2 + 1) * 6 + 3 * g + e] = res[1].d[e]; }
    }
    int* meta = reinterpret_cast<int*>(lds + GROUND_PER_WAVE * 16);
    if (g == 0) { meta[sub] = on ? (A.lm ? (A.candidate ? 1 - A.lm[b].cur : A.lm[b].cur) : 0) : -1; meta[32 + sub] = (int)fi; meta[64 + sub] = (int)cs_index(n, b, CS_GROUND, (int)(gf % n)); }
    lds_sync();
    {   // n * Y^T Y (7 x 7 per frame; the block set is added once per outer frame index, solver.cpp:142-159): a record (PGS = 28 doubles)
        // leaves as 14 lanes x 16 bytes, four frames per store instruction; (r, c) pairs fixed per lane as in the wheel role
        const long gf0 = (long)wave * GROUND_PER_WAVE;
        const int nfr = (int)min((long)GROUND_PER_WAVE, total - gf0);
        const double mult = (double)n;
        constexpr int LPF = PGS / 2;                           // lanes per frame
        const int j = lane / LPF, pr = lane - j * LPF;
        const bool all_on = __builtin_amdgcn_ballot_w64(lane < nfr && meta[lane & 31] < 0) == 0;   // (uniform)
        if (j < 4) {
            const int rc0 = c_ground_rc.e[2 * pr], rc1 = c_ground_rc.e[2 * pr + 1];
            const int r0 = rc0 >> 8, c0 = rc0 & 255, r1 = rc1 >> 8, c1 = rc1 & 255;
            auto frame = [&](int q) {
                const double* Yq = lds + q * 16;
                double2 v;
                v.x = mult * __builtin_fma(Yq[7 + r0], Yq[7 + c0], Yq[r0] * Yq[c0]);
                v.y = mult * __builtin_fma(Yq[7 + r1], Yq[7 + c1], Yq[r1] * Yq[c1]);
                return v;
            };
            auto put = [&](int sel, int fq, const double2& v) { *reinterpret_cast<double2*>(&(sel ? A.PG[1] : A.PG[0])[(size_t)fq * PGS + 2 * pr]) = v; };
            int q = j;
            if (all_on)
                for (; q + 4 < nfr; q += 8) {                  // two rounds of four frames in flight
                    const int sa = meta[q], fa = meta[32 + q], sb = meta[q + 4], fb = meta[36 + q];
                    const double2 va = frame(q), vb = frame(q + 4);
                    put(sa, fa, va); put(sb, fb, vb);
                }
            for (; q < nfr; q += 4) {
                const int sel = meta[q], fq = meta[32 + q];
                const double2 v = frame(q);
                if (sel >= 0) put(sel, fq, v);
            }
        }
        if (COSTCOPY && A.CS[0] && lane < nfr && meta[lane & 31] >= 0) {   // compact cost array: lane q writes frame q's entry, the same operations as record entry PG_C
            const double* Yq = lds + lane * 16;
            (meta[lane] ? A.CS[1] : A.CS[0])[meta[64 + lane]] = mult * __builtin_fma(Yq[13], Yq[13], Yq[6] * Yq[6]);
        }
    }
}

// ------------------------------------------------------------------------------------------- wheel + ground, two lanes per block
// The batched form of the two small roles (k_lin_small; k_lin_all keeps the lane layouts above).  A wheel block (b, k) is two lanes:
// lane 0 differentiates R_k, lane 1 R_{k+1} (three directions each, as above); the three directions of the RELATIVE translation, which
// took a third lane with an idle exp_so3, ride along as three more dual parts of the scalar tail only (p -> length / direction angle: the
// rotation magnitude does not depend on p; its translation derivative is the chain's slopes times a zero seed, kept as ONE more dual
// part so that the NaN of norm() at an exactly stationary increment, wheel_factor.h:52-63, comes out as the reference's Jets give it).
// 31 blocks per wave instead of 21.  The lane that holds exp_so3(theta) of a frame with its three derivatives also evaluates that
// frame's ground factors (ground_factor.h:27-48, :59-82: frame k+1 by lane 1, frame k by lane 0 — stored for k = 0 only), so the ground
// role costs no exp_so3 of its own and no waves: 0.141 of the kernel's 0.708 ms per 49 152 C2 windows were its waves.
constexpr int WG_PER_WAVE = 31, WG_REC = 68;   // LDS doubles per block: Y [3][13] | ground of frame k+1 [2][7] at 39 | of frame k [2][7] at 53
constexpr int WG_LDS = WG_PER_WAVE * WG_REC + 96;   // + six meta words per block
__device__ __forceinline__ LJN<4> ext4(const J3& a) { LJN<4> r; r.v = a.v; r.d[0] = a.d[0]; r.d[1] = a.d[1]; r.d[2] = a.d[2]; r.d[3] = 0.0; return r; }
template <bool COSTCOPY>
__device__ __forceinline__ void wheel_ground2_blocks(const LinArgs& A, const DevParams& P, int wave, double* lds, const int* const act) {
    typedef LJN<4> J4;
    typedef LJN<6> J6;
    const int lane = threadIdx.x & 63, blk = lane >> 1, f = lane & 1;
    const int n = A.n, nb = n - 1;
    const long total = (long)(act ? act[0] : A.B) * nb, gb = (long)wave * A.small_per_wave + blk;   // over the windows still iterating
    bool on = blk < A.small_per_wave && blk < WG_PER_WAVE && gb < total;
    const int wi = on ? (int)(gb / nb) : 0, k = on ? (int)(gb % nb) : 0;
    const int b = act ? act[1 + wi] : wi;
    if (on && !act) on = window_live(A, b);
    double* Y = lds + (blk < WG_PER_WAVE ? blk : 0) * WG_REC;
    const size_t fk = on ? (size_t)b * nb + k : 0, fi0 = on ? (size_t)b * n + k : 0;
    if (on) {
        const double* si_ = A.x + fi0 * 15;
        const double* sj_ = si_ + 15;
        const double* T12 = A.wheel_T + fk * 12;
        const double* sq9 = A.wheel_sqrtP + fk * 9;
        const V3<double> thi = cast_v3<double>(si_ + 3), thj = cast_v3<double>(sj_ + 3);
        V3<J3> arg;   // the rotation this lane differentiates
        arg.x = seed<3>(f ? thj.x : thi.x, 0, true); arg.y = seed<3>(f ? thj.y : thi.y, 1, true); arg.z = seed<3>(f ? thj.z : thi.z, 2, true);
        const M3<J3> Md = exp_so3(arg);
        M3<double> Ri, Rj;   // the two rotations as values: the value parts of the two lanes' differentiated rotations
        {
            const int l0 = lane - f;
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                const double mv = Md.m[q].v;
                Ri.m[q] = __shfl(mv, l0, 64);
                Rj.m[q] = __shfl(mv, l0 + 1, 64);
            }
        }
        // ---- ground factors of this lane's frame (k + f) from the same exp_so3: height of the wheel-frame origin, tilt of its z axis
        {
            const double pz = f ? sj_[2] : si_[2];
            const J3 r0 = (Md(2, 0) * P.tiw[0] + Md(2, 1) * P.tiw[1] + Md(2, 2) * P.tiw[2] + J3(pz)) * P.ground_p_info;
            // (fourth dual part: a zero seed = any of the three position directions, whose derivative of the tilt is slope * 0 — NaN when
            //  the axis is exactly level, as the reference's Jets give it)
            const J4 zx = ext4(Md(0, 0)) * P.Riw[2] + ext4(Md(0, 1)) * P.Riw[5] + ext4(Md(0, 2)) * P.Riw[8];
            const J4 zy = ext4(Md(1, 0)) * P.Riw[2] + ext4(Md(1, 1)) * P.Riw[5] + ext4(Md(1, 2)) * P.Riw[8];
            const J4 r1 = dasin(dsqrt(zy * zy + zx * zx)) * P.ground_q_info;
            double* Yg = Y + (f ? 39 : 53);
            Yg[0] = 0.0; Yg[1] = 0.0; Yg[2] = P.ground_p_info;   // d (R(2,:) t + p_z) / d p, scaled
#pragma unroll
            for (int e = 0; e < 3; ++e) { Yg[3 + e] = r0.d[e]; Yg[7 + e] = r1.d[3]; Yg[10 + e] = r1.d[e]; }
            Yg[6] = r0.v; Yg[13] = r1.v;
            const size_t fi = fi0 + f;
            if ((f || k == 0) && A.dbg_ground_res) { A.dbg_ground_res[fi * 2] = r0.v; A.dbg_ground_res[fi * 2 + 1] = r1.v; }
            if ((f || k == 0) && A.dbg_ground_jac)
                for (int e = 0; e < 6; ++e) { A.dbg_ground_jac[(fi * 2) * 6 + e] = Yg[e]; A.dbg_ground_jac[(fi * 2 + 1) * 6 + e] = Yg[7 + e]; }
        }
        __builtin_amdgcn_sched_barrier(0);
        const M3<double> Riw = cast_m3<double>(P.Riw);
        const V3<double> tiw(P.tiw[0], P.tiw[1], P.tiw[2]);
        const M3<double> Rwi = mul(Ri, Riw);                      // tf_i.R
        const M3<double> Am = transpose(Rwi);                     // R_iw^T R_i^T
        const M3<double> RjRiw = mul(Rj, Riw);
        const V3<double> Rjt = mul(Rj, tiw);
        const V3<double> w(Rjt.x + sj_[0] - si_[0], Rjt.y + sj_[1] - si_[1], Rjt.z + sj_[2] - si_[2]);
        const M3<double> Rrel = mul(Am, RjRiw);
        const V3<double> trel = mul(Am, w) - mulT(Riw, tiw);
        M3<J4> E;      // relative rotation: parts 0..2 this lane's rotation directions, part 3 the zero seed of the translation directions
        V3<J6> p;      // relative translation: parts 0..2 this lane's rotation directions, 3..5 the translation directions
#pragma unroll
        for (int q = 0; q < 9; ++q) E.m[q] = J4(Rrel.m[q]);
        p.x = J6(trel.x); p.y = J6(trel.y); p.z = J6(trel.z);
        p.x.d[3] = 1.0; p.y.d[4] = 1.0; p.z.d[5] = 1.0;
        {
            const M3<double> RiwT = transpose(Riw);
            M3<double> Lm, Rm;
#pragma unroll
            for (int q = 0; q < 9; ++q) { Lm.m[q] = f == 0 ? RiwT.m[q] : Am.m[q]; Rm.m[q] = f == 0 ? RjRiw.m[q] : Riw.m[q]; }
            const V3<double> wv(f == 0 ? w.x : tiw.x, f == 0 ? w.y : tiw.y, f == 0 ? w.z : tiw.z);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                M3<double> X;   // f = 0: (dR_i / d theta_i_e)^T, f = 1: dR_j / d theta_j_e
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) X(r, c) = f == 0 ? Md(c, r).d[e] : Md(r, c).d[e];
                const M3<double> LX = mul(Lm, X);
                const M3<double> dR = mul(LX, Rm);
                const V3<double> dt = mul(LX, wv);
#pragma unroll
                for (int q = 0; q < 9; ++q) E.m[q].d[e] = dR.m[q];
                p.x.d[e] = dt.x; p.y.d[e] = dt.y; p.z.d[e] = dt.z;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // wheel_odom_factor::operator() from (p, q) on (wheel_factor.h:36-70)
        const V3<J4> q = log_SO3(E);
        const V3<double> oq = log_SO3(cast_m3<double>(T12));      // log_SE3 of the constant odometry increment: plain doubles
        const double opx = T12[9], opy = T12[10];
        const double o_len = sqrt(opx * opx + opy * opy);
        const J6 len = dsqrt(p.x * p.x + p.y * p.y);
        J6 res0, res1, angle(0.0);
        if (o_len > 0.0001 && len.v > 0.0001) {
            const double odx = opx / o_len, ody = opy / o_len;     // normalized(o_dir)
            const J6 dx = p.x / len, dy = p.y / len;
            const J6 cz = dy * odx - dx * ody;                     // |cross(o_dir, dir)| through norm() = sqrt(z^2), as the reference computes it
            angle = dasin(dsqrt(cz * cz));
        } else {
            angle = len;
        }
        if (len.v < 0.0001 || o_len < 0.0001) res0 = len * sq9[0];
        else res0 = (J6(o_len) - len) * sq9[0];
        res1 = angle * sq9[4];
        const J4 nq = norm(q);
        const double noq = sqrt(oq.x * oq.x + oq.y * oq.y + oq.z * oq.z);
        J4 res2;
        if (nq.v < 0.001 || noq < 0.001) res2 = nq * sq9[8];
        else res2 = (J4(noq) - nq) * sq9[8];
        // rotation columns of this lane: theta_i (3..5) or theta_j (9..11)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int col = f ? 9 + e : 3 + e;
            Y[col] = res0.d[e]; Y[13 + col] = res1.d[e]; Y[26 + col] = res2.d[e];
        }
        if (f == 0) {
            // position columns: Y[r][p_j c] = sum_k Dp[r][k] R_wi[c][k],  Y[r][p_i c] = -Y[r][p_j c];  residual column
            const double Dp[3][3] = {{res0.d[3], res0.d[4], res0.d[5]}, {res1.d[3], res1.d[4], res1.d[5]}, {res2.d[3], res2.d[3], res2.d[3]}};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double v = Dp[r][0] * Rwi.m[c * 3] + Dp[r][1] * Rwi.m[c * 3 + 1] + Dp[r][2] * Rwi.m[c * 3 + 2];
                    Y[r * 13 + 6 + c] = v;
                    Y[r * 13 + c] = -v;
                }
            }
            Y[12] = res0.v; Y[25] = res1.v; Y[38] = res2.v;
        }
    }
    lds_sync();
    if (on && f == 0 && A.dbg_wheel_res)
        for (int r = 0; r < 3; ++r) A.dbg_wheel_res[fk * 3 + r] = Y[r * 13 + 12];
    if (on && A.dbg_wheel_jac)
        for (int e = f; e < 36; e += 2) A.dbg_wheel_jac[fk * 36 + e] = Y[(e / 12) * 13 + e % 12];
    // per block: partial buffer (0 / 1) or -1 = skip | wheel record | wheel cost slot | ground record of frame k | its cost slot | k
    int* meta = reinterpret_cast<int*>(lds + WG_PER_WAVE * WG_REC);
    if (f == 0 && blk < WG_PER_WAVE) {
        meta[blk] = on ? (A.lm ? (A.candidate ? 1 - A.lm[b].cur : A.lm[b].cur) : 0) : -1;
        meta[32 + blk] = (int)fk;
        meta[64 + blk] = (int)cs_index(n, b, CS_WHEEL, k);
        meta[96 + blk] = (int)fi0;
        meta[128 + blk] = (int)cs_index(n, b, CS_GROUND, k);
        meta[160 + blk] = k;
    }
    lds_sync();
    const long gb0 = (long)wave * A.small_per_wave;
    const int nblk = (int)min((long)min(A.small_per_wave, WG_PER_WAVE), total - gb0);
    const int ml = lane < WG_PER_WAVE ? lane : 0;
    const int selv = meta[ml], fkv = meta[32 + ml], csv = meta[64 + ml], fiv = meta[96 + ml], cgv = meta[128 + ml], kv = meta[160 + ml];
    const bool all_on = __builtin_amdgcn_ballot_w64(lane < nblk && selv < 0) == 0;   // (uniform; false only without the list of live windows)
    // ---- wheel records (PWS = 92 doubles): 46 lanes x 16 bytes, one store per block
    if (lane < PWS / 2) {
        const int rc0 = c_wheel_rc.e[2 * lane], rc1 = c_wheel_rc.e[2 * lane + 1];
        const int r0 = rc0 >> 8, c0 = rc0 & 255;
        const int r1 = rc1 >= 0 ? rc1 >> 8 : 0, c1 = rc1 >= 0 ? rc1 & 255 : 0;
        auto block = [&](int q) {
            const double* Yq = lds + q * WG_REC;
            double2 v;
            v.x = __builtin_fma(Yq[26 + r0], Yq[26 + c0], __builtin_fma(Yq[r0], Yq[c0], Yq[13 + r0] * Yq[13 + c0]));
            const double w1 = __builtin_fma(Yq[26 + r1], Yq[26 + c1], __builtin_fma(Yq[r1], Yq[c1], Yq[13 + r1] * Yq[13 + c1]));
            v.y = rc1 >= 0 ? w1 : 0.0;                         // entry 91 is padding
            return v;
        };
        auto put = [&](int q, const double2& v) {
            const int sel = __builtin_amdgcn_readlane(selv, q);
            *reinterpret_cast<double2*>(&(sel ? A.PW[1] : A.PW[0])[(size_t)__builtin_amdgcn_readlane(fkv, q) * PWS + 2 * lane]) = v;
        };
        int q = 0;
        if (all_on)
            for (; q + 3 <= nblk; q += 3) {
                const double2 va = block(q), vb = block(q + 1), vc = block(q + 2);
                put(q, va); put(q + 1, vb); put(q + 2, vc);
            }
        for (; q < nblk; ++q) {
            const double2 v = block(q);
            if (__builtin_amdgcn_readlane(selv, q) >= 0) put(q, v);
        }
    }
    // ---- ground records (PGS = 28 doubles): 14 lanes x 16 bytes, four frames per store; pass 0 = frame k+1 of every block, pass 1 = frame k
    // of the blocks with k = 0 (a window's first)
    {
        const double mult = (double)n;
        constexpr int LPF = PGS / 2;
        const int j = lane / LPF, pr = lane - j * LPF;
        const bool any_k0 = __builtin_amdgcn_ballot_w64(lane < nblk && kv == 0) != 0;   // (uniform)
        if (j < 4) {
            const int rc0 = c_ground_rc.e[2 * pr], rc1 = c_ground_rc.e[2 * pr + 1];
            const int r0 = rc0 >> 8, c0 = rc0 & 255, r1 = rc1 >> 8, c1 = rc1 & 255;
            for (int pass = 0; pass < (any_k0 ? 2 : 1); ++pass) {
                const int yo = pass ? 53 : 39;
                for (int q = j; q < nblk; q += 4) {
                    const int sel = meta[q], fq = meta[96 + q] + (pass ? 0 : 1), kq = meta[160 + q];
                    const double* Yq = lds + q * WG_REC + yo;
                    double2 v;
                    v.x = mult * __builtin_fma(Yq[7 + r0], Yq[7 + c0], Yq[r0] * Yq[c0]);
                    v.y = mult * __builtin_fma(Yq[7 + r1], Yq[7 + c1], Yq[r1] * Yq[c1]);
                    if (sel >= 0 && (pass == 0 || kq == 0))
                        *reinterpret_cast<double2*>(&(sel ? A.PG[1] : A.PG[0])[(size_t)fq * PGS + 2 * pr]) = v;
                }
            }
        }
        // compact cost array: lane q writes block q's three entries, the same operations as the records' cost entries
        if (COSTCOPY && A.CS[0] && lane < nblk && selv >= 0) {
            const double* Yq = lds + lane * WG_REC;
            double* CSb = selv ? A.CS[1] : A.CS[0];
            CSb[csv] = __builtin_fma(Yq[38], Yq[38], __builtin_fma(Yq[12], Yq[12], Yq[25] * Yq[25]));
            CSb[cgv + 1] = mult * __builtin_fma(Yq[39 + 13], Yq[39 + 13], Yq[39 + 6] * Yq[39 + 6]);
            if (kv == 0) CSb[cgv] = mult * __builtin_fma(Yq[53 + 13], Yq[53 + 13], Yq[53 + 6] * Yq[53 + 6]);
        }
        (void)fiv;
    }
}

// ------------------------------------------------------------------------------------------- dispatch
// The IMU / wheel / ground roles index their blocks over the whole batch (21 / 21 / 32 per wave), so no wave is partly empty
// because of window boundaries; `done` windows are skipped lane by lane.
__host__ __device__ inline int imu_wave_count(int B, int n, int per_wave) { return n > 1 ? (int)(((long)B * (n - 1) + per_wave - 1) / per_wave) : 0; }
__host__ __device__ inline int wheel_wave_count(int B, int n, int per_wave) { return imu_wave_count(B, n, per_wave); }
__host__ __device__ inline int ground_wave_count(int B, int n) { return (int)(((long)B * n + GROUND_PER_WAVE - 1) / GROUND_PER_WAVE); }
template <int ND, bool COSTCOPY>
__device__ __forceinline__ void small_role(const LinArgs& A, const DevParams& P, int vblock, double* lds, const int* const act) {
    const int nw = wheel_wave_count(A.B, A.n, A.small_per_wave);
    if (vblock < nw) wheel_blocks<ND, COSTCOPY>(A, P, vblock, lds, act);
    else ground_frames<COSTCOPY>(A, P, vblock - nw, lds, act);
}
constexpr int SMALL_LDS = WHEEL_PER_WAVE * 64 + 32 + 16 + 64;   // + 64 per-block meta words + the (r, c) table of the wheel / ground record; >= GROUND_PER_WAVE * 16 + 32
__global__ __launch_bounds__(64, 2) void k_lin_imu(LinArgs A, DevParams P) {
    __shared__ double lds[IMU_PER_WAVE * IMU_REC];
    const int* const act = usable_active_list(A.active, A.B);
    if (A.imu_pk && *A.imu_pk_bad == 0) imu_blocks<3, true>(A, P, (int)blockIdx.x, lds, act);   // (uniform)
    else imu_blocks<3>(A, P, (int)blockIdx.x, lds, act);
}
__global__ __launch_bounds__(64, 2) void k_lin_imu_chain(LinArgs A, DevParams P) {   // consecutive blocks of one window per wave: per-frame IMU records
    __shared__ __attribute__((aligned(16))) double lds[IMU_PER_WAVE * IMU_REC + IMU_STAGE + IMU_SBUF];
    const int* const act = usable_active_list(A.active, A.B);
    if (A.imu_pk && *A.imu_pk_bad == 0) imu_blocks<3, true, true>(A, P, (int)blockIdx.x, lds, act);   // (uniform)
    else imu_blocks<3, false, true>(A, P, (int)blockIdx.x, lds, act);
}
// windows of at most IMU_PER_WAVE / 2 blocks (two-frame tracking windows: one block): several windows per wave.  A kernel of its own, so that
// its per-lane window bookkeeping does not enter the register allocation of the 30-frame kernel above (249 of 256)
__global__ __launch_bounds__(64, 2) void k_lin_imu_chain_multi(LinArgs A, DevParams P) {
    __shared__ __attribute__((aligned(16))) double lds[IMU_PER_WAVE * IMU_REC + IMU_STAGE + IMU_SBUF];
    const int* const act = usable_active_list(A.active, A.B);
    if (A.imu_pk && *A.imu_pk_bad == 0) imu_blocks<3, true, true, true>(A, P, (int)blockIdx.x, lds, act);   // (uniform)
    else imu_blocks<3, false, true, true>(A, P, (int)blockIdx.x, lds, act);
}
// Packed IMU block records of a solve (IMU_PK doubles per block, liw_kernels.hpp): one thread per entry; `bad` is raised when a
// sqrt_inverse_P has a non-zero entry below its diagonal (not what imu_preintegraption.h:149 produces: the role then reads the full arrays).
__global__ void k_imu_pack(long blocks, const double* X, const double* J, const double* S, const double* Dt, double* pk, int* bad) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= blocks * 256) return;
    const long fk = t >> 8;
    const int e = (int)(t & 255);
    if (e < IMU_PK) {
        double v = 0.0;
        if (e < 15) v = X[fk * 15 + e];
        else if (e == IPK_DT) v = Dt[fk];
        else if (e < IPK_S) { const int q = e - IPK_J; v = J[fk * 225 + (q / 6) * 15 + 9 + q % 6]; }
        else if (e < IPK_S + 120) {
            int r = 0, q = e - IPK_S;
            while (q >= 15 - r) { q -= 15 - r; ++r; }
            v = S[fk * 225 + r * 15 + r + q];
        }
        pk[fk * IMU_PK + e] = v;
    }
    if (e < 225 && e % 15 < e / 15 && S[fk * 225 + e] != 0.0) atomicOr(bad, 1);
}
// *flag = 1 when any laser end point has a non-zero z component (planes 2, 5, 8, 11 of the [12][Ltot] block array); 2-D scans have none
// (src/utilies/common.cpp:22-24) and the laser role then skips those planes.  Once per solve.
__global__ void k_laser_z_scan(long Ltot, const double* pts, int* flag) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool nz = false;
    for (long j = t; j < Ltot; j += (long)gridDim.x * blockDim.x)
        nz = nz || pts[2 * Ltot + j] != 0.0 || pts[5 * Ltot + j] != 0.0 || pts[8 * Ltot + j] != 0.0 || pts[11 * Ltot + j] != 0.0;
    if (__any(nz) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
void launch_laser_z_scan(long Ltot, const double* laser_pts, int* flag, hipStream_t s) {
    (void)hipMemsetAsync(flag, 0, sizeof(int), s);
    if (Ltot <= 0) return;
    const long blocks = (Ltot + 1023) / 1024;
    hipLaunchKernelGGL(k_laser_z_scan, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, Ltot, laser_pts, flag);
}
void launch_imu_pack(int B, int n, const double* imu_X, const double* imu_J, const double* imu_sqrtP, const double* imu_Dt, double* pk, int* bad, hipStream_t s) {
    (void)hipMemsetAsync(bad, 0, sizeof(int), s);
    const long blocks = (long)B * (n - 1);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_imu_pack, dim3((unsigned)blocks), dim3(256), 0, s, blocks, imu_X, imu_J, imu_sqrtP, imu_Dt, pk, bad);
}
constexpr int SMALL_OCC = 2;   // (two waves per SIMD: 17.6 kB of LDS per wave, no scratch; two and three waves tied before the roles were merged)
__global__ __launch_bounds__(64, SMALL_OCC) void k_lin_small(LinArgs A, DevParams P) {
    __shared__ double lds[WG_LDS > SMALL_LDS ? WG_LDS : SMALL_LDS];
    static_assert(sizeof(double) * (WG_LDS > SMALL_LDS ? WG_LDS : SMALL_LDS) * 4 * SMALL_OCC <= 160 * 1024, "LDS of the waves of a CU");
    const int* const act = usable_active_list(A.active, A.B);
    if (A.n > 1) wheel_ground2_blocks<true>(A, P, (int)blockIdx.x, lds, act);   // wheel blocks; the ground frames ride along
    else ground_frames<true>(A, P, (int)blockIdx.x, lds, act);                   // a one-frame window has no wheel block
}
__global__ void k_lm_reset(int B, LmState* lm, int max_iters) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) lm_reset(lm[b], max_iters);
}
// Small batches (a single tracking window): every role in ONE launch, the role of a wave follows from its block index —
// one kernel and no fork / join events per linearisation, which is what a latency-bound 2-frame window pays for.
template <bool BOTH>
__global__ __launch_bounds__(64, 2) void k_lin_all(LinArgs A, DevParams P, int G, int n_laser, int n_imu, int n_roles) {
    __shared__ double lds[IMU_PER_WAVE * IMU_REC];   // IMU / small roles (>= SMALL_LDS); the laser role brings its own static LDS
    const int v = (int)blockIdx.x;
    if (v >= n_roles) {   // the extra work-group of a solve's first linearisation: LM state reset (the role waves of this launch do not read it)
        for (int b = threadIdx.x; b < A.B; b += 64) lm_reset(A.reset_lm[b], A.reset_iters);
        return;
    }
#ifdef LIW_CLK
    if ((threadIdx.x & 63) == 0 && v < 40) g_clk_lin[400 + 2 * v] = clock64();
#endif
    if (v < n_laser) laser_wave_local<BOTH>(A, P, G, v);
    else if (A.small_nd == 1) {   // (uniform) one direction per lane: the short instruction stream a single window waits for
        if (v < n_laser + n_imu) imu_blocks<1>(A, P, v - n_laser, lds, nullptr); else small_role<1, false>(A, P, v - n_laser - n_imu, lds, nullptr);
    } else {
        if (v < n_laser + n_imu) imu_blocks<3>(A, P, v - n_laser, lds, nullptr); else small_role<3, false>(A, P, v - n_laser - n_imu, lds, nullptr);
    }
#ifdef LIW_CLK
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if ((threadIdx.x & 63) == 0 && v < 40) g_clk_lin[401 + 2 * v] = clock64();
#endif
}

// ids of the windows that are still iterating, in window order (deterministic): active[0] = count, active[1 ..] = ids; behind the list:
// a ticket word and one 64-bit publication word per work-group.  Small work-groups (256 windows each: one cache line per window, LmState is
// 15 kB): a group counts its live windows, PUBLISHES the count, adds up the counts of the groups in front of it as they appear (they were
// dispatched earlier and are a few microseconds of work each) and writes its ids at that offset; the group that finishes last clears
// the publication words for the next launch.  History: (1) ONE 1 024-thread group with 68 kB of LDS waited up to 0.9 ms for a CU to drain
// behind the laser kernel; (2) small groups + a scan by the last group alone: 44 us per 24 576 windows (96 flag bytes per thread, serially).
constexpr int COMPACT_MAX = 1 << 20;
__host__ __device__ inline size_t compact_pub_offset(int B) { return (sizeof(int) * ((size_t)B + 3) + 7) & ~(size_t)7; }   // list, ticket, status
__host__ __device__ inline size_t compact_list_bytes(int B) { return compact_pub_offset(B) + 8 * (((size_t)B + 255) / 256); }
__global__ __launch_bounds__(256) void k_compact_active(int B, const LmState* lm, int* active) {
    unsigned long long* pub = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(active) + compact_pub_offset(B));
    int* ticket = active + B + 1;
    int* status = active + B + 2;     // compact_status(): 1 = the list is complete, bit 1 = a group gave up waiting (consumers index by window)
    __shared__ int wcnt[4];
    __shared__ int part[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, blk = (int)blockIdx.x, nblk = (int)gridDim.x;
    const int b0 = blk * 256 + t;
    const bool live = b0 < B && !lm[b0].done;
    const unsigned long long m = __ballot(live);
    const int before = __popcll(m & ((1ull << lane) - 1ull));       // live windows of this wave in front of this lane
    if (lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    const int bc = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (t == 0) __hip_atomic_store(pub + blk, ((unsigned long long)bc << 1) | 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    // counts of the groups in front (bounded wait: a group that never shows up ends in a short list, not in a hung GPU)
    int sum = 0;
    for (int j = t; j < blk; j += 256) {
        unsigned long long v = 0;
        for (long polls = 0; polls < (1l << 24); ++polls) {
            v = __hip_atomic_load(pub + j, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (v & 1ull) break;
            __builtin_amdgcn_s_sleep(2);
        }
        if (!(v & 1ull)) atomicOr(status, 2);   // this group's offset is wrong: the list is marked unusable, nobody reads it
        sum += (int)(v >> 1);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) part[wv] = sum;
    __syncthreads();
    const int offset = part[0] + part[1] + part[2] + part[3];
    int wbase = 0;
    for (int q = 0; q < wv; ++q) wbase += wcnt[q];
    if (live) active[1 + offset + wbase + before] = b0;
    if (blk == nblk - 1 && t == 0) { active[0] = offset + bc; atomicOr(status, 1); }
    __syncthreads();
    if (t == 0 && __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nblk - 1) {
        for (int j = 0; j < nblk; ++j) __hip_atomic_store(pub + j, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ticket, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// laser block range of every (window, frame): first block of window b owned by a frame >= i
__global__ void k_group_offsets(int B, int n, const int* laser_off, const int* laser_frame, int* group_off) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * (n + 1)) return;
    const int b = t / (n + 1), i = t % (n + 1);
    int lo = laser_off[b], hi = laser_off[b + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (laser_frame[mid] < i) lo = mid + 1; else hi = mid;
    }
    group_off[t] = lo;
}

// One linearisation.  Large batches: the laser, IMU and wheel+ground role kernels write disjoint partial-sum slots, so
// they run concurrently (main stream + two side streams joined by events); the matrix-core phase of the IMU kernel then
// overlaps the fp64 VALU work of the laser kernel on the same CUs.  Small batches: one launch for everything (k_lin_all).
// defer_join: the laser role stays on `s`, the IMU / small roles on the side streams, and the join is left to launch_linearize_join —
// a factor-sharded driver puts its exchange of the laser partial sums on `s` in between, so that it overlaps the small roles.
size_t compact_list_bytes_host(int B) { return compact_list_bytes(B); }
bool lin_builds_active_list(int B, int eval_small) {
    static const bool no_compact = getenv("LIW_NO_COMPACT") != nullptr;   // profiling aid: index the small roles over all windows
    return eval_small && B >= 512 && B <= COMPACT_MAX && !no_compact;
}
void launch_linearize(const LinArgs& A_, const DevParams& P, hipStream_t s, const LinFork* fk, bool defer_join) {
    LinArgs A = A_;
    const int n = A.n, B = A.B;
    // IMU / wheel blocks per wave: 21 (all 63 lanes) once the batch fills the chip; small batches spread their blocks over more,
    // shorter waves (the matrix-core stage of a wave is serial over its blocks); a few windows (everything in ONE k_lin_all launch
    // with a wave per block) also switch to one derivative direction per lane
    A.small_nd = 3;
    {
        const long blocks = (long)B * (n > 1 ? n - 1 : 0);
        int pw = WHEEL_PER_WAVE;
        while (pw > 3 && (blocks + pw - 1) / pw < 512) pw = (pw + 1) / 2;   // 21 -> 11 -> 6 -> 3
        const bool nd3 = getenv("LIW_SMALL_ND3") != nullptr;                 // profiling / test aid (read per launch): three directions per lane everywhere
        if (A.eval_small && !nd3 && !A.pi_frame && A.role_mask == 0 && (long)B * n + 2 * blocks + ground_wave_count(B, n) <= 256) { pw = 1; A.small_nd = 1; }
        A.small_per_wave = pw;
        A.imu_per_wave = pw < IMU_PER_WAVE ? pw : IMU_PER_WAVE;
    }
    // groups per wave: one for small batches (latency), up to LASER_GMAX for large ones (no ragged last pass per group)
    int G = 1;
    if (A.mode != LIW_MODE_TRACK) while (G < LASER_GMAX && (long)B * ((n + 2 * G - 1) / (2 * G)) >= 4096) G *= 2;
    const int laser_waves = B * ((n + G - 1) / G);
    const int imu_waves = A.eval_small ? imu_wave_count(B, n, A.imu_per_wave) : 0;
    const int small_waves = A.eval_small ? wheel_wave_count(B, n, A.small_per_wave) + ground_wave_count(B, n) : 0;
    // large batches only: a single window gains nothing from the list and would pay one more launch per LM iteration
    const bool have_list = A.lm && A.active && lin_builds_active_list(B, A.eval_small);
    const bool compact = have_list && (A.role_mask == 0 || (A.role_mask & 8));   // (a single timed role re-uses the list built in front of it)
    if (!have_list) A.active = nullptr;
    // (also without the small roles — the older-frames laser evaluation of a marginalisation enqueued behind a tracking solve: the SAME
    // compiled body as the one-launch linearisation it must agree with bit for bit; the stand-alone k_lin_laser is a second compilation of
    // the body, whose FMA contraction may differ in the last bit)
    // (a single timed role, role_mask != 0, always takes the stand-alone kernels: the one-launch form cannot run a role alone)
    if (!A.pi_frame && A.role_mask == 0 && laser_waves + imu_waves + small_waves <= 256) {   // (per-frame IMU records come from k_lin_imu_chain only)
        const int roles = laser_waves + imu_waves + small_waves;
        const unsigned tot = (unsigned)(roles + (A.reset_lm ? 1 : 0));
        if (A.mode == LIW_MODE_INIT) hipLaunchKernelGGL(k_lin_all<true>, dim3(tot), dim3(64), 0, s, A, P, G, laser_waves, imu_waves, roles);
        else hipLaunchKernelGGL(k_lin_all<false>, dim3(tot), dim3(64), 0, s, A, P, G, laser_waves, imu_waves, roles);
        return;
    }
    if (A.reset_lm) hipLaunchKernelGGL(k_lm_reset, dim3((B + 63) / 64), dim3(64), 0, s, B, A.reset_lm, A.reset_iters);
    const bool fork = fk && fk->side[0] && A.eval_small;
    // the list of windows still iterating (read by the IMU / wheel / ground roles and by the next step kernel) is built IN FRONT of the
    // fork: on a side stream its work-groups queued behind the laser kernel, whose waves hold every register of the chip, and the roles
    // waiting for the list started up to 0.9 ms late
    if (compact) hipLaunchKernelGGL(k_compact_active, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, A.lm, A.active);
    if (fork) {
        hipEventRecord(fk->ev_fork, s);
        hipStreamWaitEvent(fk->side[0], fk->ev_fork, 0);
        hipStreamWaitEvent(fk->side[1], fk->ev_fork, 0);
    }
    hipStream_t s_imu = fork ? fk->side[0] : s, s_small = fork ? fk->side[1] : s;
    const int rm = A.role_mask ? A.role_mask : 7;
    auto role_laser = [&]() {
        if (!(rm & 1)) return;
        if (A.laser_pk) launch_lin_laser_slab(A, P, s);   // large 2-D batches: a lane per (window, frame) group (both poses free: INIT; one: MARG / TRACK)
        else if (A.mode == LIW_MODE_INIT) hipLaunchKernelGGL(k_lin_laser<true>, dim3((unsigned)laser_waves), dim3(64), 0, s, A, P, G);
        else hipLaunchKernelGGL(k_lin_laser<false>, dim3((unsigned)laser_waves), dim3(64), 0, s, A, P, G);
    };
    auto role_imu = [&]() {
        const bool no_multi = getenv("LIW_NO_IMU_MULTI") != nullptr;      // A/B / test aid (read per launch): a wave per window whatever n
        if (imu_waves && (rm & 2) && A.pi_frame && imu_chain_windows(n - 1) > 1 && !no_multi) {
            const int wpw = imu_chain_windows(n - 1);
            hipLaunchKernelGGL(k_lin_imu_chain_multi, dim3((unsigned)((B + wpw - 1) / wpw)), dim3(64), 0, s_imu, A, P);
        } else if (imu_waves && (rm & 2) && A.pi_frame) hipLaunchKernelGGL(k_lin_imu_chain, dim3((unsigned)(B * imu_chain_parts(n - 1))), dim3(64), 0, s_imu, A, P);
        else if (imu_waves && (rm & 2)) hipLaunchKernelGGL(k_lin_imu, dim3((unsigned)imu_waves), dim3(64), 0, s_imu, A, P);
    };
    auto role_small = [&]() {
        if (!(small_waves && (rm & 4))) return;
        // k_lin_small: two lanes per wheel block (31 per wave once the batch fills the chip), the ground frames evaluated by the wheel lanes
        if (A.small_per_wave == WHEEL_PER_WAVE) A.small_per_wave = WG_PER_WAVE;
        const int waves = n > 1 ? wheel_wave_count(B, n, A.small_per_wave) : ground_wave_count(B, n);
        hipLaunchKernelGGL(k_lin_small, dim3((unsigned)waves), dim3(64), 0, s_small, A, P);
    };
    // submission order of the three role kernels (they sit on three streams and drain roughly in this order).  LIW_LIN_ORDER (read once):
    // a permutation of "lis" (laser, IMU, small) — A/B aid, tools/bracket_time.py
    static const char* order_env = getenv("LIW_LIN_ORDER");
    const char* order = (order_env && strlen(order_env) == 3) ? order_env : "lis";
    for (int k = 0; k < 3; ++k) {
        if (order[k] == 'l') role_laser();
        else if (order[k] == 'i') role_imu();
        else if (order[k] == 's') role_small();
    }
    if (fork) {
        hipEventRecord(fk->ev_join[0], fk->side[0]);
        hipEventRecord(fk->ev_join[1], fk->side[1]);
        if (!defer_join) {
            hipStreamWaitEvent(s, fk->ev_join[0], 0);
            hipStreamWaitEvent(s, fk->ev_join[1], 0);
        }
    }
}
void launch_linearize_join(hipStream_t s, const LinFork* fk) {
    if (!fk || !fk->side[0]) return;
    hipStreamWaitEvent(s, fk->ev_join[0], 0);   // events never recorded count as complete
    hipStreamWaitEvent(s, fk->ev_join[1], 0);
}

// ------------------------------------------------------------------------------------------- factor-sharded exchange
// A laser group record (LP = 128 slots) is a signed expansion of NP pair totals (45 with both poses free, 21 with one): the
// exchange between ranks moves the NP totals only.  pack: record -> totals (128-slot records: representative slot and sign per total,
// table built on the host from laser_slot_code; compact records of the large-batch format hold the totals themselves: a plain copy);
// unpack: sum over `world` gathered copies in rank order -> record.
__global__ void k_exchange_pack(int groups, int n, int np, int compact, LaserPackTable tb, const double* PL0, const double* PL1, int candidate, const LmState* lm, double* buf) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= groups * np) return;
    const int grp = t / np, p = t % np;
    const bool dead = lm && lm[grp / n].done;   // finished windows are not re-linearised: their stale sums must not accumulate
    const int sel = lm ? (candidate ? 1 - lm[grp / n].cur : lm[grp / n].cur) : 0;
    const double* PL = sel ? PL1 : PL0;
    double v;
    if (compact) v = PL[(size_t)grp * LPC + p];
    else { v = PL[(size_t)grp * LP + tb.slot[p]]; v = tb.neg[p] ? -v : v; }
    buf[t] = dead ? 0.0 : v;
}
template <bool BOTH>
__global__ void k_exchange_unpack(int groups, int n, int np, int compact, int world, size_t stride, const double* buf, double* PL0, double* PL1, double* CS0, double* CS1, int candidate, const LmState* lm, int sysload) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int lps = laser_stride(compact);
    if (t >= groups * lps) return;
    const int grp = t / lps, s = t % lps;
    const int sel = lm ? (candidate ? 1 - lm[grp / n].cur : lm[grp / n].cur) : 0;
    double* PL = sel ? PL1 : PL0;
    const int code = compact ? (s < np ? s : -1) : laser_slot_code<BOTH>(s);   // compact: slot s IS pair total s, zeros behind the totals
    double v = 0.0;
    if (code >= 0) {
        const double* src = buf + (size_t)grp * np + (code & 63);
        // fixed rank order: every rank forms the same bits.  sysload: the images were written by OTHER devices (peer-write exchange):
        // system-scope loads, which do not trust lines this device's caches may still hold from the exchange two steps back
        for (int r = 0; r < world; ++r)
            v += sysload ? __hip_atomic_load(src + (size_t)r * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : src[(size_t)r * stride];
        if (code & 64) v = -v;
    }
    PL[t] = v;
    // the compact cost array of the large-batch format (liw_kernels.hpp, cs_index) holds the record's sum r^2 a second time: the prologue of
    // k_lm_step_quad reads ONLY that copy, so it has to carry the cross-rank total like the record does (else every rank would accept or
    // reject on its own shard's laser cost and the ranks would part ways)
    if (s == (compact ? np - 1 : 120) && CS0) (sel ? CS1 : CS0)[cs_index(n, grp / n, CS_LASER, grp % n)] = v;   // (the last pair total is sum r^2)
}
// records of either format -> 128-slot records (what a caller that inspects the records reads: 2dliw-slam_amd/batch.py)
template <bool BOTH>
__global__ void k_laser_expand(int groups, int compact, const double* PL, double* out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)groups * LP) return;
    out[t] = laser_slot<BOTH>(PL + (t / LP) * laser_stride(compact), (int)(t % LP), compact);
}
void launch_laser_expand(int B, int n, bool both, int compact, const double* PL, double* out, hipStream_t s) {
    const int groups = B * n;
    const unsigned blocks = (unsigned)(((size_t)groups * LP + 255) / 256);
    if (both) hipLaunchKernelGGL(k_laser_expand<true>, dim3(blocks), dim3(256), 0, s, groups, compact, PL, out);
    else hipLaunchKernelGGL(k_laser_expand<false>, dim3(blocks), dim3(256), 0, s, groups, compact, PL, out);
}
__global__ void k_count_active(int B, const LmState* lm, double* out) {
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int c = 0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) c += lm[b].done ? 0 : 1;
    atomicAdd(&cnt, c);   // integer: order-independent
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (double)cnt;
}
void launch_exchange_pack(int B, int n, bool both, int compact, const double* PL0, const double* PL1, int candidate, const LmState* lm, double* buf, hipStream_t s) {
    const int np = both ? 45 : 21, groups = B * n;
    LaserPackTable tb{};
    for (int p = 0; p < np; ++p) tb.slot[p] = -1;
    for (int sl = 0; sl < LP; ++sl) {
        const int code = both ? laser_slot_code<true>(sl) : laser_slot_code<false>(sl);
        if (code >= 0 && tb.slot[code & 63] < 0) { tb.slot[code & 63] = sl; tb.neg[code & 63] = (code & 64) ? 1 : 0; }
    }
    hipLaunchKernelGGL(k_exchange_pack, dim3((groups * np + 255) / 256), dim3(256), 0, s, groups, n, np, compact, tb, PL0, PL1, candidate, lm, buf);
    if (lm) hipLaunchKernelGGL(k_count_active, dim3(1), dim3(256), 0, s, B, lm, buf + (size_t)groups * np);
}
void launch_exchange_unpack(int B, int n, bool both, int compact, int world, size_t stride, const double* buf, double* PL0, double* PL1, double* CS0, double* CS1, int candidate, const LmState* lm, hipStream_t s, bool sysload) {
    const int np = both ? 45 : 21, groups = B * n, lps = laser_stride(compact);
    if (both) hipLaunchKernelGGL(k_exchange_unpack<true>, dim3((groups * lps + 255) / 256), dim3(256), 0, s, groups, n, np, compact, world, stride, buf, PL0, PL1, CS0, CS1, candidate, lm, sysload ? 1 : 0);
    else hipLaunchKernelGGL(k_exchange_unpack<false>, dim3((groups * lps + 255) / 256), dim3(256), 0, s, groups, n, np, compact, world, stride, buf, PL0, PL1, CS0, CS1, candidate, lm, sysload ? 1 : 0);
}

// ---- native one-shot exchange: instead of an all-gather collective every rank WRITES its packed record
// straight into its slot of every peer's receive area (P-1 pushes over the P-1 dedicated xGMI links, one hop), raises its flag there, and
// waits for the P flags of its own area before the rank-order sum.  Receive area of a rank: [2 parities][world images][nd doubles] +
// [world] 64-bit flags; peers map each other's areas with hipIpc (one process per GPU) or share pointers (one process).  Exchange e uses
// parity e & 1: a peer can only push exchange e + 2 after it has received this rank's e + 1, which this rank sends after it has summed e.
__global__ void k_p2p_push(size_t nd, const double* buf, P2pPeers peers, int rank, int world, int parity) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nd) return;
    const double v = buf[t];
    for (int p = 0; p < world; ++p)   // system-scope (write-through) stores: the payload leaves this device's caches as it is written
        __hip_atomic_store(peers.area[p] + ((size_t)(parity * world + rank)) * nd + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_p2p_signal(P2pPeers peers, int rank, int world, unsigned long long epoch) {   // launched behind k_p2p_push: its stores are complete
    const int p = threadIdx.x;
    if (p >= world) return;
    __atomic_thread_fence(__ATOMIC_RELEASE);   // (system scope by default)
    __hip_atomic_store(peers.flags[p] + rank, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// ONE small work-group polls (a spinning grid could keep a peer's push off a shared device); bounded: a peer that never arrives ends
// in an error word, not in a hung GPU
__global__ void k_p2p_wait(const unsigned long long* flags, int world, unsigned long long epoch, long long max_polls, int* err) {
    const int r = threadIdx.x;
    if (r < world && *(volatile int*)err == 0) {   // (an exchange that already failed is not waited for again)
        long long polls = 0;
        while (__hip_atomic_load(flags + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
            __builtin_amdgcn_s_sleep(32);
            if (++polls > max_polls) { atomicExch(err, 1 + r); break; }
        }
    }
    __syncthreads();
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
}
void launch_p2p_exchange(size_t nd, const double* buf, const P2pPeers& peers, int rank, int world, unsigned long long epoch, int* err, hipStream_t s) {
    const int parity = (int)(epoch & 1ull);
    hipLaunchKernelGGL(k_p2p_push, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, s, nd, buf, peers, rank, world, parity);
    hipLaunchKernelGGL(k_p2p_signal, dim3(1), dim3(64), 0, s, peers, rank, world, epoch);
    hipLaunchKernelGGL(k_p2p_wait, dim3(1), dim3(64), 0, s, (const unsigned long long*)peers.flags[rank], world, epoch, (long long)4000000, err);
}
#ifdef LIW_CLK
extern "C" void liw_debug_clk_lin(long long* out, int nn) { hipMemcpyFromSymbol(out, HIP_SYMBOL(g_clk_lin), sizeof(long long) * nn); }
#endif
void launch_group_offsets(int B, int n, const int* laser_off, const int* laser_frame, int* group_off, hipStream_t s) {
    const int tot = B * (n + 1);
    hipLaunchKernelGGL(k_group_offsets, dim3((tot + 255) / 256), dim3(256), 0, s, B, n, laser_off, laser_frame, group_off);
}

}  // namespace liw
