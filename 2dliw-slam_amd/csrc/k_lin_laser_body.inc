// k_lin_laser_body.inc — body of the laser role, included twice by k_linearize.hip: as the __global__ kernel k_lin_laser
// and as the device function the single-launch kernel k_lin_all calls.  Textual inclusion instead of a shared
// function template: the register allocation of this 250-VGPR body is sensitive to the calling context, and the stand-alone
// kernel is the one the roofline number is measured on.  Expects: A (LinArgs), P (DevParams), G, vblock, template bool BOTH.
    constexpr int NC = BOTH ? 9 : 6;
    constexpr int NP = NC * (NC + 1) / 2;
    const int lane = threadIdx.x & 63;
    const int n = A.n;
    const int wpw = (n + G - 1) / G;                     // waves per window
    const int b = vblock / wpw, i0 = (vblock % wpw) * G;
    if (b >= A.B) return;
    if (!window_live(A, b)) return;
    const int psel = A.lm ? (A.candidate ? 1 - A.lm[b].cur : A.lm[b].cur) : 0;   // partial buffer of this window
    const int i1 = min(n, i0 + G);   // this wave owns the groups of frames i0 .. i1-1
    if (i0 >= i1) return;
    __shared__ double tf[LASER_GMAX * 2 * FTF];   // frame transform records of the wave's frames (a | b per frame)
    __shared__ int goff[LASER_GMAX + 1];
    __shared__ double red[24 * 65];      // lane-transpose buffer of the group reduction
    __shared__ double tl[48];            // pair totals of the group being written
    __shared__ int slot_src[128];
    __shared__ int fon_lds[LASER_GMAX];

    // frame transforms of the wave's frames in LDS, re-read close to each use, which keeps 64 doubles per frame out of the
    // VGPRs.  Per frame: a = frame 0 (init) or the constant laser_match pose, b = own pose; computed by this wave, 4 lanes per record.
    {
        const int rec = lane >> 2, dir = lane & 3, g = rec >> 1, which = rec & 1;
        if (g < i1 - i0) {
            const int i = i0 + g;
            const double* pose6 = which ? (A.x + ((size_t)b * n + i) * 15)
                                        : (BOTH ? (A.x + (size_t)b * n * 15) : (A.match_pose + ((size_t)b * n + i) * 12));
            frame_tf_record(P, pose6, dir, tf + g * 64 + which * FTF);
        }
    }
    // slot -> (pair index | 64 if negated), -1 = structural zero, of the 128-slot group record (laser_slot_code, liw_kernels.hpp)
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) slot_src[lane + 64 * qq] = laser_slot_code<BOTH>(lane + 64 * qq);
    LSTAMP(0);
    if (lane < i1 - i0) fon_lds[lane] = (A.has_match[b * n + i0 + lane] && (A.mode != LIW_MODE_TRACK || i0 + lane == n - 1 || A.marg_older)) ? 1 : 0;
    if (lane <= i1 - i0) goff[lane] = A.group_off[b * (n + 1) + i0 + lane];
    lds_sync();
    LSTAMP(1);
    int pass_dbg = 0; (void)pass_dbg;
    const int J0 = goff[0], J1 = goff[i1 - i0];

    // 2-D scans: every end point has z = 0 in its laser frame (the reference builds them that way, src/utilies/common.cpp:22-24).  When the
    // solve in progress found no non-zero z (launch_laser_z_scan, per solve), the four z planes are not read (a third of the role's
    // HBM reads) and their terms are left out (exact: they are products with 0).  No flag (single windows, other callers): full path.
    const bool hz = A.laser_hz == nullptr || __builtin_amdgcn_readfirstlane(*A.laser_hz) != 0;
    constexpr int NACC = BOTH ? 48 : 32;   // 45 / 21 pair accumulators, padded to 32 (+16)
    double acc[NACC];
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] = 0.0;
    const size_t Lt = (size_t)A.Ltot;
    int cf = i0;                           // group being accumulated (uniform)
    double q[12];                          // this lane's block record (end points of the two matched segments)
    // the 12 component planes as wave-uniform base pointers + an unsigned 32-bit block index per lane: one global_load with scalar base
    // per component instead of a 64-bit vector address each (the block index is below Ltot < 2^31)
    const double* plane[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) plane[c] = A.laser_pts + (size_t)c * Lt;
    if (J0 + lane < J1) {
#pragma unroll
        for (int c = 0; c < 12; ++c) if (c % 3 != 2) q[c] = plane[c][(unsigned)(J0 + lane)];
        if (hz) {
#pragma unroll
            for (int c = 2; c < 12; c += 3) q[c] = plane[c][(unsigned)(J0 + lane)];
        }
    }
    if (!hz) { q[2] = 0.0; q[5] = 0.0; q[8] = 0.0; q[11] = 0.0; }
    // group boundaries of the wave's frames as scalars (they were re-read from LDS and compared per lane in every pass: 108 instructions)
    int gbound[LASER_GMAX];
#pragma unroll
    for (int g = 1; g < LASER_GMAX; ++g) gbound[g] = __builtin_amdgcn_readfirstlane(g < i1 - i0 ? goff[g] : 0x7fffffff);
    for (int base = J0;; base += 64) {
        const int j = base + lane;
        asm volatile("" ::: "memory");   // keeps the LDS reads of the transforms inside the pass (no loop-invariant hoisting)
        // owning frame of this lane's block = number of group boundaries at or below j
        int fl = i0;
#pragma unroll
        for (int g = 1; g < LASER_GMAX; ++g) fl += (j >= gbound[g]) ? 1 : 0;
        const bool fon = fon_lds[fl - i0] != 0;
        const bool valid = j < J1 && fon;
        double rows[2][NC];
        LSTAMP(8 + pass_dbg * 8 + 0);
        auto block_rows = [&](auto HZ_) {   // the block's two whitened Jacobian rows + residuals; HZ: the end points have z components
            constexpr bool HZ = decltype(HZ_)::value;
            const double* tfl = tf + (fl - i0) * 64;
#define TA(k) tfl[(k)]
#define TB(k) tfl[FTF + (k)]
            // laser_factor ctor: len1, len2, sum   (laser_factor.h:30-43)
            const double d1x = q[0] - q[3], d1y = q[1] - q[4], d1z = HZ ? q[2] - q[5] : 0.0;
            const double d2x = q[6] - q[9], d2y = q[7] - q[10], d2z = HZ ? q[8] - q[11] : 0.0;
            // min(len1, len2) = sqrt(min(len1^2, len2^2)) exactly (sqrt is monotone and correctly rounded): one sqrt
            // sum = sqrt(lmin / 2 / 0.02) = (625 min(len1, len2)^2)^(1/4): two square roots as x * rsqrt(x) on the hardware estimate + two
            // Newton steps each (the IEEE sqrt / division expansions were 70 of this lane's ~900 instructions per block)
            const double l2 = HZ ? fmin(d1x * d1x + d1y * d1y + d1z * d1z, d2x * d2x + d2y * d2y + d2z * d2z)
                                 : fmin(d1x * d1x + d1y * d1y, d2x * d2x + d2y * d2y);
            const double lmin25 = l2 > 0.0 ? 25.0 * (l2 * fast_rsqrt(l2)) : 0.0;
            const double sum = lmin25 > 0.0 ? lmin25 * fast_rsqrt(lmin25) : 0.0;
            // world points, z dropped (laser_factor.h:67-77).  (sums start with their additive constant: t + a b + c d contracts into two FMAs,
            // a b + c d + t into a multiplication, an FMA and an addition)
            double Ap[2], Bp[2], C[2][2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if constexpr (HZ) {
                    Ap[r] = TA(6 + r) + TA(r * 3) * q[0] + TA(r * 3 + 1) * q[1] + TA(r * 3 + 2) * q[2];
                    Bp[r] = TA(6 + r) + TA(r * 3) * q[3] + TA(r * 3 + 1) * q[4] + TA(r * 3 + 2) * q[5];
                    C[0][r] = TB(6 + r) + TB(r * 3) * q[6] + TB(r * 3 + 1) * q[7] + TB(r * 3 + 2) * q[8];
                    C[1][r] = TB(6 + r) + TB(r * 3) * q[9] + TB(r * 3 + 1) * q[10] + TB(r * 3 + 2) * q[11];
                } else {
                    Ap[r] = TA(6 + r) + TA(r * 3) * q[0] + TA(r * 3 + 1) * q[1];
                    Bp[r] = TA(6 + r) + TA(r * 3) * q[3] + TA(r * 3 + 1) * q[4];
                    C[0][r] = TB(6 + r) + TB(r * 3) * q[6] + TB(r * 3 + 1) * q[7];
                    C[1][r] = TB(6 + r) + TB(r * 3) * q[9] + TB(r * 3 + 1) * q[10];
                }
            }
            const double ux = Bp[0] - Ap[0], uy = Bp[1] - Ap[1];
            const double zz = ux * ux + uy * uy;
            const bool regular = zz > 0.0;
            const double rlen = regular ? fast_rsqrt(zz) : 1.0;   // one reciprocal square root instead of eight divisions by the length
            const double lx = ux * rlen, ly = uy * rlen;   // degenerate: stays the (zero) difference vector
            double dBx[3], dBy[3], dlx[3], dly[3];
            __builtin_amdgcn_sched_barrier(0);
            if (BOTH) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    __builtin_amdgcn_sched_barrier(0);
                    const int dMo = 8 + 6 * k, dto = 26 + 2 * k;
                    const double m0 = TA(dMo), m1 = TA(dMo + 1), m3 = TA(dMo + 3), m4 = TA(dMo + 4);
                    const double t0 = TA(dto), t1 = TA(dto + 1);
                    double dAx, dAy;
                    if constexpr (HZ) {
                        const double m2 = TA(dMo + 2), m5 = TA(dMo + 5);
                        dAx = t0 + m0 * q[0] + m1 * q[1] + m2 * q[2];
                        dAy = t1 + m3 * q[0] + m4 * q[1] + m5 * q[2];
                        dBx[k] = t0 + m0 * q[3] + m1 * q[4] + m2 * q[5];
                        dBy[k] = t1 + m3 * q[3] + m4 * q[4] + m5 * q[5];
                    } else {
                        dAx = t0 + m0 * q[0] + m1 * q[1];
                        dAy = t1 + m3 * q[0] + m4 * q[1];
                        dBx[k] = t0 + m0 * q[3] + m1 * q[4];
                        dBy[k] = t1 + m3 * q[3] + m4 * q[4];
                    }
                    const double dux = dBx[k] - dAx, duy = dBy[k] - dAy;
                    const double pr = lx * dux + ly * duy;
                    dlx[k] = (dux - lx * pr) * rlen;
                    dly[k] = (duy - ly * pr) * rlen;
                }
            }
            const double w = sum * P.laser_sqrt_info;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                __builtin_amdgcn_sched_barrier(0);
                const double* pt = q + 6 + 3 * k;
                const double ex = C[k][0] - Bp[0], ey = C[k][1] - Bp[1];
                double dCx[3], dCy[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const int dMo = 8 + 6 * m, dto = 26 + 2 * m;
                    if constexpr (HZ) {
                        dCx[m] = TB(dto) + TB(dMo) * pt[0] + TB(dMo + 1) * pt[1] + TB(dMo + 2) * pt[2];
                        dCy[m] = TB(dto + 1) + TB(dMo + 3) * pt[0] + TB(dMo + 4) * pt[1] + TB(dMo + 5) * pt[2];
                    } else {
                        dCx[m] = TB(dto) + TB(dMo) * pt[0] + TB(dMo + 1) * pt[1];
                        dCy[m] = TB(dto + 1) + TB(dMo + 3) * pt[0] + TB(dMo + 4) * pt[1];
                    }
                }
                // jc: [a_x a_y a_th0..2 b_th0..2]; b_x = -a_x, b_y = -a_y
                // (the sign of the distance rides on the weight: w * (sg * x) == (w * sg) * x exactly, eight multiplications per row less)
                double dist, jc[8], ws = w;
                if (regular) {
                    const double s = lx * ey - ly * ex;
                    ws = s < 0.0 ? -w : w;
                    dist = fabs(s);
                    // A point EXACTLY on the line: the reference takes norm() of the zero Jet p2p - (l.p2p) l (common.h:94), whose derivative is
                    // 0 * inf = NaN -> Ceres rejects the evaluation (IsEvaluationValid).  The cross product above has a finite derivative
                    // there, so the rejected vector is formed as the reference forms it and a zero poisons the block's rows (the residual
                    // itself stays 0, as in the Jet's value part).
                    {
                        const double prj = lx * ex + ly * ey;
                        const double vx = ex - prj * lx, vy = ey - prj * ly;
                        if (vx * vx + vy * vy == 0.0) ws = __builtin_nan("");
                    }
                    jc[0] = ly; jc[1] = -lx;
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        jc[2 + m] = BOTH ? (dlx[m] * ey - dly[m] * ex - lx * dBy[m] + ly * dBx[m]) : 0.0;
                        jc[5 + m] = lx * dCy[m] - ly * dCx[m];
                    }
                } else {  // zero-length reference segment: distance to the point B (Jet semantics of normalized(0))
                    dist = sqrt(ex * ex + ey * ey);
                    const double nx = ex / dist, ny = ey / dist;
                    jc[0] = -nx; jc[1] = -ny;
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        jc[2 + m] = BOTH ? -(nx * dBx[m] + ny * dBy[m]) : 0.0;
                        jc[5 + m] = nx * dCx[m] + ny * dCy[m];
                    }
                }
                const double res = sum * (P.laser_sqrt_info * dist);
                if (BOTH) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) rows[k][c] = ws * jc[c];
                } else {
                    rows[k][0] = -ws * jc[0]; rows[k][1] = -ws * jc[1];
#pragma unroll
                    for (int c = 0; c < 3; ++c) rows[k][2 + c] = ws * jc[5 + c];
                }
                rows[k][NC - 1] = res;
                if (A.dbg_laser_res) A.dbg_laser_res[(size_t)j * 2 + k] = res;
                if (A.dbg_laser_jac) {
                    double* dj = A.dbg_laser_jac + ((size_t)j * 2 + k) * 12;
                    dj[0] = ws * jc[0]; dj[1] = ws * jc[1]; dj[2] = 0.0;
                    dj[3] = ws * jc[2]; dj[4] = ws * jc[3]; dj[5] = ws * jc[4];
                    dj[6] = -ws * jc[0]; dj[7] = -ws * jc[1]; dj[8] = 0.0;
                    dj[9] = ws * jc[5]; dj[10] = ws * jc[6]; dj[11] = ws * jc[7];
                }
            }
#undef TA
#undef TB
        };
        if (valid) {
            if (hz) block_rows(std::true_type{}); else block_rows(std::false_type{});
        }
        LSTAMP(8 + pass_dbg * 8 + 1);
        // software pipeline: the record of the next chunk is in flight during the pair products and the group reduction
        __builtin_amdgcn_sched_barrier(0);
        if (j + 64 < J1) {
#pragma unroll
            for (int c = 0; c < 12; ++c) if (c % 3 != 2) q[c] = plane[c][(unsigned)(j + 64)];
            if (hz) {
#pragma unroll
                for (int c = 2; c < 12; c += 3) q[c] = plane[c][(unsigned)(j + 64)];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- accumulate / flush: a 64-block chunk may straddle group boundaries; the lanes of group cf add their pair
        //      products, and every group that ends inside (or before) this chunk is reduced and written.  The wave
        //      therefore makes ceil(blocks/64) passes over its G groups instead of one ceil per group.
        bool more = true;
        int fl_dbg = 0; (void)fl_dbg;
        while (more) {
            LSTAMP(8 + pass_dbg * 8 + 2 + 2 * fl_dbg);
            if (valid && fl == cf) {
                // (the rows are laundered per round of this loop: as loop invariants their 90 products were hoisted in front of it and every
                // round then ADDED them under its mask — 90 multiplications + 90 additions per round instead of 90 FMAs)
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int c = 0; c < NC; ++c) asm volatile("" : "+v"(rows[k][c]));
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int c1 = 0; c1 < NC; ++c1)
#pragma unroll
                        for (int c2 = c1; c2 < NC; ++c2) acc[c1 * NC - c1 * (c1 - 1) / 2 + (c2 - c1)] += rows[k][c1] * rows[k][c2];
            }
            more = goff[cf + 1 - i0] <= base + 64;       // group cf is complete (uniform)
            LSTAMP(8 + pass_dbg * 8 + 3 + 2 * fl_dbg);
            fl_dbg = fl_dbg < 2 ? fl_dbg + 1 : 2;
            if (more) {
                double* out = (psel ? A.PL[1] : A.PL[0]) + ((size_t)b * n + cf) * laser_stride(A.pl_compact);
                // totals of the NP pair accumulators over the 64 lanes.  Stage 1, in registers: v_permlane32_swap folds the upper
                // half-wave onto the lower one for TWO accumulators at a time (A' = [A_lo | B_lo], B' = [A_hi | B_hi], A' + B' =
                // [A's 32 half-sums | B's 32 half-sums]) -> NPK = ceil(NP / 2) packed registers.  Stage 2: ONE transpose through LDS
                // (lane (p, h) sums the 32 entries of half h of packed register p = the total of accumulator 2p + h).  A further
                // v_permlane16_swap stage (12 registers, 16 entries per reader) measured 3 % slower than this; the two-round
                // transpose of all 45 accumulators it replaces was 4 % slower.
                constexpr int NPK = (NP + 1) / 2;
                static_assert(NPK <= 24, "one transpose round");
                double pk[NPK];
#pragma unroll
                for (int e = 0; e < NPK; ++e) {
                    const double a = acc[2 * e], bq = (2 * e + 1 < NP) ? acc[2 * e + 1] : 0.0;
                    const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(a), __double2loint(bq), false, false);
                    const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(a), __double2hiint(bq), false, false);
                    pk[e] = __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
                }
                lds_sync();
#pragma unroll
                for (int e = 0; e < NPK; ++e) red[e * 65 + lane] = pk[e];
                lds_sync();
                {
                    const int pp = lane < 2 * NPK ? lane >> 1 : 0, hh = lane & 1;
                    const double* rp = red + pp * 65 + 32 * hh;
                    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
                    for (int k = 0; k < 32; k += 4) { s0 += rp[k]; s1 += rp[k + 1]; s2 += rp[k + 2]; s3 += rp[k + 3]; }
                    const double tot = (s0 + s1) + (s2 + s3);
                    if (lane < 2 * NPK && lane < NP) tl[lane] = tot;   // lane = 2 pp + hh = accumulator index
                    if (kCostCopy && lane == NP - 1 && A.CS[0]) (psel ? A.CS[1] : A.CS[0])[cs_index(n, b, CS_LASER, cf)] = tot;   // (the last pair total is sum r^2)
                }
                lds_sync();
                (void)NP;
                if (A.pl_compact) {
                    // large-batch format: the pair totals themselves, zeros behind them
                    if (lane < LPC) out[lane] = lane < NP ? tl[lane] : 0.0;
                } else {
                    // compose the 128-slot record from the pair totals (source pair and sign per slot: table built once per wave)
#pragma unroll
                    for (int qq = 0; qq < 2; ++qq) {
                        const int s = lane + 64 * qq;
                        const int src = slot_src[s];
                        out[s] = src < 0 ? 0.0 : (src & 64 ? -tl[src & 63] : tl[src & 63]);
                    }
                }
#pragma unroll
                for (int e = 0; e < NACC; ++e) acc[e] = 0.0;
                ++cf;
                more = cf < i1;
            }
        }
        ++pass_dbg;
        if (cf >= i1) break;
    }
    LSTAMP(2);
