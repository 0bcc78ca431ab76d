// k_map_locate.hip — localisation of fleet robots in a held occupancy grid (C ABI include/liw_map_locate.h, host side
// liw_map_locate.cpp): the whole-cell correlative scan match.  The grid of a fleet-map or group-map region becomes a dilated
// field of small integers once (a snapshot in the localiser's own store); a query rotates its scan once per candidate angle into
// cells and scores every whole-cell shift of a window by summing field bytes.  Integer decisions on cells that come from
// + - * / floor in double, each rounded on its own: the outputs are defined bit for bit.
//
//   kernel          mapping                                   work
//   k_floc_head     a lane per map                            status, zeroed counts and the source's liw_map_info into the header
//   k_floc_field    4 cells per lane, a work-group per        grid -> 2 / 1 / 0, one 4-byte store per lane; the two counts go by
//                   (map, chunk)                              wave sums and integer adds into the header
//   k_floc_match    a work-group of 256 per (query, angle)    the scan's cells of the angle go into LDS in chunks of 512 points
//                                                             (int2; a point outside the margin is a skip mark); a lane scores
//                                                             four neighbouring column shifts from ONE 4-byte load of a field row,
//                                                             16 lanes span a row of the window, the 16 lane groups of the block
//                                                             16 rows, a lane takes every 16th row; the sums are packed four to a
//                                                             word and widened every 120 points; the scores stay in registers
//                                                             across chunks; lanes and waves fold by a 64-bit key into one
//                                                             partial record per (query, angle)
//   k_floc_pick     a wave per query                          status, the fold of the n_theta records by the same order, the sum
//                                                             of the ties, and the output rows
//   k_floc_link     a lane per query                          T_w_l = make_tf(p, q) * T_imu_to_laser (compose_twl of the fleet
//                                                             map), T_g_w = T_m_l * inverse(T_w_l)
//
// No floating-point atomics and no order-dependent result: the only atomics are integer adds of counts.
#pragma clang fp contract(off)   // every product and sum rounds on its own, as in k_map_batch.hip and k_map_group.hip

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/liw_map_locate.h"
#include "k_map_batch_dev.hpp"
#include "k_map_locate.hpp"

namespace liw_floc_dev {

using liw_map_dev::wave_sum;

constexpr int kBlk = 256;            // threads of k_floc_match: four waves
constexpr int kChunk = 512;          // points per LDS chunk
constexpr int kSlots = 4;            // window rows per lane: 16 lane groups of 16 lanes take 16 rows at a time, 4 * 16 >= 2 * 31 + 1
constexpr int kFlush = 120;          // points between two flushes of the packed sums: 120 * 2 < 256
constexpr int kSkip = INT_MIN / 2;   // cx of a point that contributes to no candidate; kSkip + 31 is still negative
constexpr int kMargin = 32;          // cells around the grid in which a point still reaches it by a shift

__device__ __forceinline__ char* map_region(char* lstore, const FLay& L, int m) { return lstore + (size_t)m * L.map_bytes; }
__device__ __forceinline__ int* record(char* lstore, const FLay& L, int q, int j) {
    return (int*)(lstore + L.s_partial + (size_t)q * L.row_bytes) + (size_t)j * kRecInts;
}

// an entry of T0 that is not finite, or a component of t0 above 1e6 in magnitude
__device__ __forceinline__ bool bad_prior(const double* __restrict__ T0) {
    bool bad = false;
    for (int e = 0; e < 12; ++e) bad |= !isfinite(T0[e]);
    for (int e = 9; e < 12; ++e) bad |= !(fabs(T0[e]) <= 1e6);
    return bad;
}

// the field of map m when it can be matched against, else nullptr
__device__ __forceinline__ char* usable_map(char* lstore, const FLay& L, int m) {
    if (m < 0 || m >= L.M) return nullptr;
    char* MR = map_region(lstore, L, m);
    return ((const int*)MR)[FH_STATUS] == LIW_FLOC_FIELD_OK ? MR : nullptr;
}

__device__ __forceinline__ void put4(int* o, int a, int b, int c, int d) { o[0] = a; o[1] = b; o[2] = c; o[3] = d; }
__device__ __forceinline__ unsigned long long umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v = umax(v, __shfl_xor(v, o));
    return v;
}

// Larger key = better candidate of one angle: score, then the smaller ix^2 + iy^2, then the lower iy, then the lower ix.
// Always > 0, so 0 stands for "no candidate".  ix, iy in -31 .. 31, score below 2^22.
__device__ __forceinline__ unsigned long long angle_key(int score, int ix, int iy) {
    return ((unsigned long long)(unsigned)score << 24) | ((unsigned long long)(4095 - (ix * ix + iy * iy)) << 12) |
           ((unsigned long long)(31 - iy) << 6) | (unsigned long long)(31 - ix);
}
// The same over the angles: the smaller |j - centre| and the lower j come between the distance and iy.
__device__ __forceinline__ unsigned long long query_key(int score, int ix, int iy, int j, int centre) {
    const int dj = j > centre ? j - centre : centre - j;
    return ((unsigned long long)(unsigned)score << 40) | ((unsigned long long)(4095 - (ix * ix + iy * iy)) << 28) |
           ((unsigned long long)(255 - dj) << 20) | ((unsigned long long)(255 - j) << 12) | ((unsigned long long)(31 - iy) << 6) |
           (unsigned long long)(31 - ix);
}

// ------------------------------------------------------------------------------------------------------------------ grid -> field
__global__ __launch_bounds__(256) void k_floc_head(char* lstore, FLay L, const char* __restrict__ src_store, size_t region_bytes,
                                                   const int* __restrict__ src_of, const unsigned char* __restrict__ msel) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= L.M || (msel && !msel[m])) return;
    char* MR = map_region(lstore, L, m);
    int* hdr = (int*)MR;
    unsigned long long* info = (unsigned long long*)(MR + HB_INFO);
    const int src = src_of[m];
    int st = LIW_FLOC_FIELD_EMPTY;
    if (src < 0) {
        for (int k = 0; k < (int)(sizeof(liw_map_info) / 8); ++k) info[k] = 0ull;
    } else {
        const char* SR = src_store + (size_t)src * region_bytes;
        const unsigned long long* si = (const unsigned long long*)(SR + HB_INFO);
        for (int k = 0; k < (int)(sizeof(liw_map_info) / 8); ++k) info[k] = si[k];
        const liw_map_info* mi = (const liw_map_info*)(SR + HB_INFO);
        const int w = mi->width, h = mi->height;
        if (w > 0 && h > 0) st = (long long)w * h > (long long)L.C ? LIW_FLOC_FIELD_OVER : LIW_FLOC_FIELD_OK;
    }
    for (int k = 0; k < 8; ++k) hdr[k] = 0;
    hdr[FH_STATUS] = st;
}

__global__ __launch_bounds__(256) void k_floc_field(char* lstore, FLay L, const char* __restrict__ src_store, size_t region_bytes, size_t grid_off,
                                                    const int* __restrict__ src_of, const unsigned char* __restrict__ msel) {
    const int m = blockIdx.x / L.cchunk, c = blockIdx.x % L.cchunk;
    if (msel && !msel[m]) return;
    char* MR = map_region(lstore, L, m);
    int* hdr = (int*)MR;
    if (hdr[FH_STATUS] != LIW_FLOC_FIELD_OK) return;       // k_floc_head of this build has set it: src_of[m] >= 0, the cells fit
    const liw_map_info* mi = (const liw_map_info*)(MR + HB_INFO);
    const int w = mi->width, h = mi->height;
    const int n = w * h;
    const signed char* grid = (const signed char*)(src_store + (size_t)src_of[m] * region_bytes + grid_off);
    unsigned* field = (unsigned*)(MR + L.m_field);
    const int words = (n + 3) / 4;                          // n <= max_cells <= 2^31 - 16
    unsigned long long occ = 0, near_cells = 0;
    for (int k = c * 256 + threadIdx.x; k < words; k += L.cchunk * 256) {
        unsigned out = 0;
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * k + e;
            if (i >= n) break;
            unsigned v = 0;
            if (grid[i] >= 50) {
                v = 2;
                ++occ;
            } else {
                const int y = i / w, x = i - y * w;
                bool any = false;
                for (int dy = -1; dy <= 1; ++dy) {
                    const int yy = y + dy;
                    if (yy < 0 || yy >= h) continue;
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int xx = x + dx;
                        if (xx >= 0 && xx < w) any |= grid[yy * w + xx] >= 50;
                    }
                }
                if (any) {
                    v = 1;
                    ++near_cells;
                }
            }
            out |= v << (8 * e);
        }
        field[k] = out;
    }
    occ = wave_sum(occ);
    near_cells = wave_sum(near_cells);
    if ((threadIdx.x & 63) == 0) {
        if (occ) atomicAdd(&hdr[FH_OCC], (int)occ);
        if (near_cells) atomicAdd(&hdr[FH_NEAR], (int)near_cells);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the search
__global__ __launch_bounds__(kBlk) void k_floc_match(char* lstore, FLay L, MatchArgs a) {
    __shared__ int2 cells[kChunk];
    __shared__ unsigned long long wkey[kBlk / 64];
    __shared__ int wties[kBlk / 64];
    __shared__ int nvalid;
    const int q = blockIdx.x / a.n_theta, j = blockIdx.x % a.n_theta, t = threadIdx.x;
    if (a.mask && !a.mask[q]) return;
    // rows that k_floc_pick reports with another status than OK or NO_POINTS leave no record: it reads none of them
    char* MR = usable_map(lstore, L, a.map_of[q]);
    if (!MR) return;
    const double* T0 = a.T0 + (size_t)q * 12;
    if (bad_prior(T0)) return;
    const liw_map_info* mi = (const liw_map_info*)(MR + HB_INFO);
    const int w = mi->width, h = mi->height;
    const double res = mi->resolution, ox = mi->origin_x, oy = mi->origin_y;
    const double R00 = T0[0], R01 = T0[1], R02 = T0[2], R10 = T0[3], R11 = T0[4], R12 = T0[5], t0x = T0[9], t0y = T0[10];
    const double cj = a.table[2 * j], sj = a.table[2 * j + 1];
    const double xlim = (double)w + kMargin, ylim = (double)h + kMargin;
    int n = a.n_points[q];
    n = n < 0 ? 0 : (n > a.point_stride ? a.point_stride : n);
    const double* pts = a.points + (size_t)q * a.point_stride * 3;
    const unsigned char* fld = (const unsigned char*)(MR + L.m_field);

    // A lane holds 4 columns by kSlots rows of the window: the columns ix0 .. ix0 + 3 are the four bytes of ONE 4-byte load from a
    // field row, the rows are iy0 + 16 r.  16 lanes span 64 columns, the 16 lane groups of the four waves 16 rows.
    const int wave = t >> 6, lane = t & 63;
    const int W = a.W;
    const int ix0 = -W + 4 * (lane & 15);
    const int iy0 = -W + 4 * wave + (lane >> 4);
    const bool lane_on = ix0 <= W;
    int acc[kSlots][4];
    unsigned pk[kSlots];                                            // four 8-bit sums per word, emptied every kFlush points
#pragma unroll
    for (int r = 0; r < kSlots; ++r) {
        pk[r] = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] = 0;
    }
    if (t == 0) nvalid = 0;
    __syncthreads();

    for (int base = 0; base < n; base += kChunk) {
        const int cnt = n - base < kChunk ? n - base : kChunk;
        unsigned long long nv = 0;
        for (int p = t; p < cnt; p += kBlk) {
            const double* P = pts + (size_t)(base + p) * 3;
            const double x = P[0], y = P[1], z = P[2];
            const double Qx = (R00 * x + R01 * y) + R02 * z;
            const double Qy = (R10 * x + R11 * y) + R12 * z;
            int2 cell = make_int2(kSkip, 0);
            if (isfinite(Qx) && isfinite(Qy) && fabs(Qx) <= 1e6 && fabs(Qy) <= 1e6) {
                ++nv;
                const double U = cj * Qx - sj * Qy;
                const double V = sj * Qx + cj * Qy;
                const double fx = floor(((U + t0x) - ox) / res);
                const double fy = floor(((V + t0y) - oy) / res);
                if (fx >= -(double)kMargin && fx < xlim && fy >= -(double)kMargin && fy < ylim) cell = make_int2((int)fx, (int)fy);
            }
            cells[p] = cell;
        }
        nv = wave_sum(nv);
        if (lane == 0 && nv) atomicAdd(&nvalid, (int)nv);
        __syncthreads();
        for (int p0 = 0; p0 < cnt; p0 += kFlush) {
            const int p1 = p0 + kFlush < cnt ? p0 + kFlush : cnt;
            for (int p = p0; p < p1; ++p) {
                const int2 cell = cells[p];                         // one address for the whole wave: a broadcast
                if (cell.x == kSkip) continue;
                const int x0 = cell.x + ix0;
                unsigned keep = 0u;                                 // byte e is column x0 + e: kept where that lies in the grid
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((unsigned)(x0 + e) < (unsigned)w) keep |= 0xFFu << (8 * e);
                if (!lane_on || keep == 0u) continue;
                // The word may begin up to 3 bytes in front of its row and end up to 3 bytes behind it.  In front of row 0 lies
                // the region's header, behind the last row the field's padding, the next region or the rows of partial records:
                // every byte read is inside the store, and `keep` drops what is not a cell of this row.
                const unsigned char* at = fld + x0;
                const int y0 = cell.y + iy0;
#pragma unroll
                for (int r = 0; r < kSlots; ++r) {
                    const int y = y0 + 16 * r;
                    if (iy0 + 16 * r <= W && (unsigned)y < (unsigned)h) {
                        unsigned v;
                        __builtin_memcpy(&v, at + y * w, 4);        // y * w + x0 + 3 < width * height + 3 < 2^31
                        pk[r] += v & keep;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < kSlots; ++r) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r][e] += (int)((pk[r] >> (8 * e)) & 0xFFu);
                pk[r] = 0u;
            }
        }
        __syncthreads();
    }

    unsigned long long key = 0;
    if (lane_on) {
#pragma unroll
        for (int r = 0; r < kSlots; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (iy0 + 16 * r <= W && ix0 + e <= W) key = umax(key, angle_key(acc[r][e], ix0 + e, iy0 + 16 * r));
    }
    key = wave_max(key);
    if (lane == 0) wkey[wave] = key;
    __syncthreads();
    const unsigned long long bk = umax(umax(wkey[0], wkey[1]), umax(wkey[2], wkey[3]));   // wave 0, lane 0 always holds a candidate
    const int bs = (int)(bk >> 24);
    unsigned long long ties = 0;
    if (lane_on) {
#pragma unroll
        for (int r = 0; r < kSlots; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (iy0 + 16 * r <= W && ix0 + e <= W && acc[r][e] == bs) ++ties;
    }
    ties = wave_sum(ties);
    if (lane == 0) wties[wave] = (int)ties;
    __syncthreads();
    if (t == 0) {
        int* rec = record(lstore, L, q, j);
        rec[REC_SCORE] = bs;
        rec[REC_IX] = 31 - (int)(bk & 63);
        rec[REC_IY] = 31 - (int)((bk >> 6) & 63);
        rec[REC_TIES] = wties[0] + wties[1] + wties[2] + wties[3];
        rec[REC_NVALID] = nvalid;
        rec[5] = rec[6] = rec[7] = 0;
    }
}

__global__ __launch_bounds__(256) void k_floc_pick(char* lstore, FLay L, MatchArgs a) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= L.Q || (a.mask && !a.mask[q])) return;
    const double* T0 = a.T0 + (size_t)q * 12;
    double* out = a.T_m_l + (size_t)q * 12;
    char* MR = usable_map(lstore, L, a.map_of[q]);
    int status = LIW_FLOC_OK, n_valid = 0;
    if (!MR) status = LIW_FLOC_NO_MAP;
    else if (bad_prior(T0)) status = LIW_FLOC_BAD_PRIOR;
    else {
        n_valid = record(lstore, L, q, 0)[REC_NVALID];              // every angle counted the same points
        if (n_valid == 0) status = LIW_FLOC_NO_POINTS;
    }
    if (status != LIW_FLOC_OK) {
        if (lane < 12) out[lane] = T0[lane];
        if (lane == 0) {
            a.found[q] = 0;
            put4(a.best + (size_t)q * 4, 0, 0, 0, 0);
            put4(a.stats + (size_t)q * 4, status, 0, 0, 0);
        }
        return;
    }
    const int centre = (a.n_theta - 1) / 2;
    unsigned long long key = 0;
    for (int j = lane; j < a.n_theta; j += 64) {
        const int* r = record(lstore, L, q, j);
        key = umax(key, query_key(r[REC_SCORE], r[REC_IX], r[REC_IY], j, centre));
    }
    key = wave_max(key);
    const int score = (int)(key >> 40);
    unsigned long long ties = 0;
    for (int j = lane; j < a.n_theta; j += 64) {
        const int* r = record(lstore, L, q, j);
        if (r[REC_SCORE] == score) ties += (unsigned long long)r[REC_TIES];
    }
    ties = wave_sum(ties);
    const int j = 255 - (int)((key >> 12) & 255), iy = 31 - (int)((key >> 6) & 63), ix = 31 - (int)(key & 63);
    const double c = a.table[2 * j], s = a.table[2 * j + 1];
    const double res = ((const liw_map_info*)(MR + HB_INFO))->resolution;
    if (lane < 3) out[lane] = c * T0[lane] - s * T0[3 + lane];
    else if (lane < 6) out[lane] = s * T0[lane - 3] + c * T0[lane];
    else if (lane < 9) out[lane] = T0[lane];
    else if (lane == 9) out[9] = T0[9] + (double)ix * res;
    else if (lane == 10) out[10] = T0[10] + (double)iy * res;
    else if (lane == 11) out[11] = T0[11];
    if (lane == 0) {
        a.found[q] = (long long)score * 1000 >= (long long)a.min_permille * 2 * (long long)n_valid ? 1 : 0;
        put4(a.best + (size_t)q * 4, j, ix, iy, score);
        put4(a.stats + (size_t)q * 4, LIW_FLOC_OK, n_valid, (int)ties, 0);
    }
}

// ------------------------------------------------------------------------------------------------------------------ hand-over
__global__ __launch_bounds__(256) void k_floc_link(int Q, const double* __restrict__ T_m_l, const double* __restrict__ poses, long long robot_stride,
                                                   liw_fmap_dev::Til12 til, const unsigned char* __restrict__ found, const unsigned char* __restrict__ mask,
                                                   double* __restrict__ T_w_l, double* __restrict__ T_g_w) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q || !found[q] || (mask && !mask[q])) return;
    double w[12];
    liw_fmap_dev::compose_twl(poses + (size_t)q * robot_stride, til, w);
    const double* a = T_m_l + (size_t)q * 12;
    const liw::Iso<double> T = liw::mul(liw::cast_iso<double>(a, a + 9), liw::inverse(liw::cast_iso<double>(w, w + 9)));
    double* ow = T_w_l + (size_t)q * 12;
    double* og = T_g_w + (size_t)q * 12;
    for (int e = 0; e < 12; ++e) ow[e] = w[e];
    for (int e = 0; e < 9; ++e) og[e] = T.R.m[e];
    og[9] = T.t.x; og[10] = T.t.y; og[11] = T.t.z;
}

static int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

int launch_build(char* lstore, const FLay& L, const char* src_store, size_t region_bytes, size_t grid_off, const int* src_of,
                 const unsigned char* msel, hipStream_t s) {
    hipLaunchKernelGGL(k_floc_head, dim3((L.M + 255) / 256), dim3(256), 0, s, lstore, L, src_store, region_bytes, src_of, msel);
    hipLaunchKernelGGL(k_floc_field, dim3((unsigned)L.M * L.cchunk), dim3(256), 0, s, lstore, L, src_store, region_bytes, grid_off, src_of, msel);
    return launched();
}

int launch_match(char* lstore, const FLay& L, const MatchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_floc_match, dim3((unsigned)L.Q * a.n_theta), dim3(kBlk), 0, s, lstore, L, a);
    hipLaunchKernelGGL(k_floc_pick, dim3((L.Q + 3) / 4), dim3(256), 0, s, lstore, L, a);
    return launched();
}

int launch_link_tf(int Q, const double* T_m_l, const double* poses, long long robot_stride, const double* Til, const unsigned char* found,
                   const unsigned char* mask, double* T_w_l, double* T_g_w, hipStream_t s) {
    liw_fmap_dev::Til12 til;
    for (int k = 0; k < 12; ++k) til.v[k] = Til[k];
    hipLaunchKernelGGL(k_floc_link, dim3((Q + 255) / 256), dim3(256), 0, s, Q, T_m_l, poses, robot_stride, til, found, mask, T_w_l, T_g_w);
    return launched();
}

}  // namespace liw_floc_dev
