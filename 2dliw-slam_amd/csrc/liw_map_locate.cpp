// liw_map_locate.cpp — host side of the localisation in a held occupancy grid (C ABI include/liw_map_locate.h; kernels in
// k_map_locate.hip): the store's layout, argument checks, the launches and the synchronous getters.  No per-query work happens here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/liw_lie.h"
#include "../../include/liw_map_locate.h"
#include "k_map_locate.hpp"
#include "liw_host_common.hpp"

namespace {

using liw_floc_dev::FLay;

bool make_flay(const liw_floc_dims* d, FLay* L) {
    if (!d || d->Q < 1 || d->M < 1 || d->max_cells < 1 || d->max_cells > 0x7FFFFFF0 || d->max_theta < 1 || d->max_theta > LIW_FLOC_MAX_THETA) return false;
    L->Q = d->Q; L->M = d->M; L->C = d->max_cells; L->T = d->max_theta;
    L->Cn = ((size_t)L->C + 15) & ~(size_t)15;
    // work-groups per map of the field kernel (4 cells per lane), as the fleet map sizes its cell kernels per robot
    const int per = std::max(64, 2048 / L->M);
    L->cchunk = (int)std::min<size_t>((L->Cn / 4 + 255) / 256, (size_t)per);
    if ((long long)L->M * L->cchunk >= (1ll << 31) || (long long)L->Q * L->T >= (1ll << 31)) return false;   // the kernels' grids
    L->m_field = 256;
    L->map_bytes = al256(L->m_field + L->Cn);
    L->s_partial = (size_t)L->M * L->map_bytes;
    L->row_bytes = al256((size_t)L->T * liw_floc_dev::kRecInts * 4);
    L->bytes = L->s_partial + (size_t)L->Q * L->row_bytes;
    return true;
}

}  // namespace

struct liw_floc_ctx : liw_fleet_ctx_base {
    FLay L{};
    double Til[12];
};

namespace {

// header words of a map region; < 0 on error
int map_header(liw_floc_ctx* c, const void* lstore, int map, int* hdr) {
    if (bad_store(lstore) || map < 0 || map >= c->L.M) return fail(c, LIW_EINVAL, "liw_floc: lstore or map");
    if (!pull(lstore, (size_t)map * c->L.map_bytes, hdr, 8)) return fail(c, LIW_EHIP, "liw_floc: hipMemcpy");
    return 0;
}

}  // namespace

extern "C" {

int liw_floc_layout(const liw_floc_dims* dims, liw_floc_layout_info* out) {
    FLay L{};
    if (!out || !make_flay(dims, &L)) return LIW_EINVAL;
    out->bytes = L.bytes;
    out->map_bytes = L.map_bytes;
    out->field_bytes = L.Cn;
    out->field_off = L.m_field;
    out->partial_off = L.s_partial;
    out->row_bytes = L.row_bytes;
    out->cell_chunks = L.cchunk;
    return LIW_OK;
}

int liw_floc_store_bytes(const liw_floc_dims* dims, size_t* bytes) {
    FLay L{};
    if (!bytes || !make_flay(dims, &L)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

liw_floc_ctx* liw_floc_create(const liw_floc_dims* dims, const double* T_imu_to_laser16, int normalize_extrinsics, int device) {
    FLay L{};
    if (!T_imu_to_laser16 || !make_flay(dims, &L)) return nullptr;
    liw_floc_ctx* c = new liw_floc_ctx();
    c->L = L;
    c->device = device;
    liw_lie_from_matrix16(T_imu_to_laser16, normalize_extrinsics, c->Til);
    c->have_device = liw_probe_gfx950(device, &c->err);
    return c;
}

void liw_floc_destroy(liw_floc_ctx* c) { delete c; }
const char* liw_floc_last_error(liw_floc_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_floc_build(liw_floc_ctx* c, void* lstore, const void* src_store, size_t region_bytes, size_t grid_off, const int* src_of,
                   const unsigned char* msel, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(lstore) || bad_store(src_store) || !src_of || region_bytes < 112 || (region_bytes & 7) != 0 || grid_off < 112 || grid_off >= region_bytes)
        return fail(c, LIW_EINVAL, "liw_floc_build: bad argument");
    if (liw_floc_dev::launch_build((char*)lstore, c->L, (const char*)src_store, region_bytes, grid_off, src_of, msel, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_floc_build: kernel launch failed");
    return LIW_OK;
}

int liw_floc_match(liw_floc_ctx* c, void* lstore, const int* map_of, const double* points, int point_stride, const int* n_points,
                   const double* T0, const double* table, int n_theta, int W, int min_permille, const unsigned char* mask,
                   unsigned char* found, int* best, int* stats, double* T_m_l, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(lstore) || !map_of || !points || !n_points || !T0 || !table || !found || !best || !stats || !T_m_l || point_stride < 1 ||
        point_stride > LIW_FLOC_MAX_STRIDE || n_theta < 1 || n_theta > c->L.T || W < 0 || W > LIW_FLOC_MAX_W || min_permille < 0)
        return fail(c, LIW_EINVAL, "liw_floc_match: bad argument");
    const liw_floc_dev::MatchArgs a{map_of, points, point_stride, n_points, T0, table, n_theta, W, min_permille, mask, found, best, stats, T_m_l};
    if (liw_floc_dev::launch_match((char*)lstore, c->L, a, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_floc_match: kernel launch failed");
    return LIW_OK;
}

int liw_floc_link_tf(liw_floc_ctx* c, const double* T_m_l, const double* poses, long long robot_stride, const unsigned char* found,
                     const unsigned char* mask, double* T_w_l, double* T_g_w, void* stream) {
    LIW_FLEET_DEV(c);
    if (!T_m_l || !poses || robot_stride < 0 || !found || !T_w_l || !T_g_w) return fail(c, LIW_EINVAL, "liw_floc_link_tf: bad argument");
    if (liw_floc_dev::launch_link_tf(c->L.Q, T_m_l, poses, robot_stride, c->Til, found, mask, T_w_l, T_g_w, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_floc_link_tf: kernel launch failed");
    return LIW_OK;
}

int liw_floc_field_info(liw_floc_ctx* c, const void* lstore, int map, liw_map_info* info, int* status, int* occupied, int* near_cells) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = map_header(c, lstore, map, hdr)) return r;
    if (status) *status = hdr[liw_floc_dev::FH_STATUS];
    if (occupied) *occupied = hdr[liw_floc_dev::FH_OCC];
    if (near_cells) *near_cells = hdr[liw_floc_dev::FH_NEAR];
    if (info && !pull(lstore, (size_t)map * c->L.map_bytes + liw_floc_dev::HB_INFO, info, 1)) return fail(c, LIW_EHIP, "liw_floc_field_info: hipMemcpy");
    return LIW_OK;
}

long long liw_floc_get_field(liw_floc_ctx* c, const void* lstore, int map, unsigned char* out, long long cap) {
    LIW_FLEET_DEV(c);
    liw_map_info mi;
    int st = 0;
    if (int r = liw_floc_field_info(c, lstore, map, &mi, &st, nullptr, nullptr)) return r;
    if (cap < 0 || (cap > 0 && !out)) return fail(c, LIW_EINVAL, "liw_floc_get_field: bad argument");
    const long long n = st == LIW_FLOC_FIELD_OK ? (long long)mi.width * mi.height : 0;
    if (!pull(lstore, (size_t)map * c->L.map_bytes + c->L.m_field, out, (size_t)std::min(n, cap))) return fail(c, LIW_EHIP, "liw_floc_get_field: hipMemcpy");
    return n;
}

const unsigned char* liw_floc_device_field(liw_floc_ctx* c, const void* lstore, int map) {
    if (!c || !lstore || map < 0 || map >= c->L.M) return nullptr;
    return (const unsigned char*)lstore + (size_t)map * c->L.map_bytes + c->L.m_field;
}

}  // extern "C"
