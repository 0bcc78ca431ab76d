// liw_map_batch.cpp — host side of the fleet's occupancy-grid maps (C ABI include/liw_map_batch.h; kernels in k_map_batch.hip): the
// store layout, argument checks, the launches and the synchronous getters.  No per-robot work happens here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_lie.h"
#include "../../include/liw_map_batch.h"
#include "k_map_batch.hpp"
#include "k_map_group.hpp"   // fmap_view: what a group map (liw_map_group.cpp) borrows from a ctx
#include "liw_host_common.hpp"

namespace {

using liw_fmap_dev::Lay;

bool make_lay(const liw_map_params* p, const liw_fmap_dims* d, Lay* L) {
    if (!p || !(p->resolution > 0) || !std::isfinite(p->resolution)) return false;
    if (!d || d->B < 1 || d->max_submaps < 1 || d->max_points < 1 || d->max_cells < 1 || d->max_steps < 4 || d->max_steps > (1 << 22)) return false;
    if (d->max_cells > 0x7FFFFFF0 || d->max_points > 0x7FFFFFF0 || (long long)d->B * d->max_submaps >= (1ll << 31)) return false;
    L->B = d->B; L->K = d->max_submaps; L->P = d->max_points; L->C = d->max_cells; L->S = d->max_steps;
    L->res = p->resolution;
    const size_t B = (size_t)L->B, K = (size_t)L->K, P = (size_t)L->P;
    L->Cn = ((size_t)L->C + 15) & ~(size_t)15;
    L->nchunk = (int)std::min<size_t>((P + 255) / 256, (size_t)liw_fmap_dev::kMaxChunks);   // of P alone: the partials are part of the region
    // work-groups per robot of the ray and cell kernels: enough that a few selected robots of a large fleet still fill the chip (the
    // others' work-groups exit at once), each with at least two rounds of rays behind the 12 kB table it stages
    const int per = std::max(64, 2048 / L->B);
    L->rchunk = (int)std::min<size_t>((P + 31) / 32, (size_t)per);
    L->cchunk = (int)std::min<size_t>((L->Cn / 16 + 255) / 256, (size_t)per);
    if ((long long)L->B * std::max(L->nchunk, std::max(L->rchunk, L->cchunk)) >= (1ll << 31)) return false;
    size_t o = 256;
    L->r_off = o; o = al256(o + (K + 1) * 4);
    L->r_pts = o; o = al256(o + P * 24);
    L->r_sub = o; o = al256(o + P * 4);
    L->r_tf = o; o = al256(o + K * 96);
    L->r_partial = o; o = al256(o + (size_t)L->nchunk * 48);
    L->r_bits = o; o = al256(o + L->Cn);
    L->r_grid = o; o = al256(o + L->Cn);
    L->robot_bytes = o;
    L->s_table = B * L->robot_bytes;
    L->shared_bytes = al256((size_t)L->S * 8);
    L->bytes = L->s_table + L->shared_bytes;
    return true;
}

}  // namespace

struct liw_fmap_ctx : liw_fleet_ctx_base {
    Lay L{};
    double Til[12];
};

liw_fmap_dev::FmapView liw_fmap_dev::fmap_view(const liw_fmap_ctx* c) {
    FmapView v;
    v.L = c->L;
    std::memcpy(v.Til, c->Til, sizeof(v.Til));
    v.device = c->device;
    v.have_device = c->have_device;
    return v;
}

namespace {

// header words of a robot; < 0 on error
int robot_header(liw_fmap_ctx* c, const void* store, int robot, int* hdr) {
    if (bad_store(store) || robot < 0 || robot >= c->L.B) return fail(c, LIW_EINVAL, "liw_fmap: store or robot");
    if (!pull(store, (size_t)robot * c->L.robot_bytes, hdr, 8)) return fail(c, LIW_EHIP, "liw_fmap: hipMemcpy");
    return 0;
}

}  // namespace

extern "C" {

int liw_fmap_layout(const liw_map_params* params, const liw_fmap_dims* dims, liw_fmap_layout_info* out) {
    Lay L{};
    if (!out || !make_lay(params, dims, &L)) return LIW_EINVAL;
    out->bytes = L.bytes;
    out->robot_bytes = L.robot_bytes;
    out->shared_off = L.s_table;
    out->shared_bytes = L.shared_bytes;
    out->cell_bytes = L.Cn;
    out->offsets_off = L.r_off;
    out->points_off = L.r_pts;
    out->index_off = L.r_sub;
    out->tf_off = L.r_tf;
    out->partial_off = L.r_partial;
    out->bits_off = L.r_bits;
    out->grid_off = L.r_grid;
    out->partials = L.nchunk;
    return LIW_OK;
}

int liw_fmap_store_bytes(const liw_map_params* params, const liw_fmap_dims* dims, size_t* bytes) {
    Lay L{};
    if (!bytes || !make_lay(params, dims, &L)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

liw_fmap_ctx* liw_fmap_create(const liw_map_params* params, const liw_fmap_dims* dims, const double* T_imu_to_laser16, int normalize_extrinsics,
                              int device) {
    Lay L{};
    if (!T_imu_to_laser16 || !make_lay(params, dims, &L)) return nullptr;
    liw_fmap_ctx* c = new liw_fmap_ctx();
    c->L = L;
    c->device = device;
    liw_lie_from_matrix16(T_imu_to_laser16, normalize_extrinsics, c->Til);
    c->have_device = liw_probe_gfx950(device, &c->err);
    return c;
}

void liw_fmap_destroy(liw_fmap_ctx* c) { delete c; }
const char* liw_fmap_last_error(liw_fmap_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_fmap_reset(liw_fmap_ctx* c, void* store, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store)) return fail(c, LIW_EINVAL, "liw_fmap_reset: store");
    if (liw_fmap_dev::launch_reset((char*)store, c->L, mask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_fmap_reset: kernel launch failed");
    return LIW_OK;
}

int liw_fmap_add_keyframes(liw_fmap_ctx* c, void* store, const unsigned char* key, const double* points, int point_stride, const int* n_points,
                           const unsigned char* mask, unsigned char* added, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !key || !points || !n_points || point_stride < 1) return fail(c, LIW_EINVAL, "liw_fmap_add_keyframes: bad argument");
    if (liw_fmap_dev::launch_add((char*)store, c->L, key, points, point_stride, n_points, mask, added, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_fmap_add_keyframes: kernel launch failed");
    return LIW_OK;
}

int liw_fmap_render_tf(liw_fmap_ctx* c, void* store, const double* T_w_l, long long robot_stride, const unsigned char* sel, int* status,
                       liw_map_info* info, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !T_w_l || robot_stride < 0 || !status || !info) return fail(c, LIW_EINVAL, "liw_fmap_render_tf: bad argument");
    if (liw_fmap_dev::launch_render((char*)store, c->L, T_w_l, nullptr, c->Til, robot_stride, sel, status, info, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_fmap_render_tf: kernel launch failed");
    return LIW_OK;
}

int liw_fmap_render(liw_fmap_ctx* c, void* store, const double* poses, long long robot_stride, const unsigned char* sel, int* status,
                    liw_map_info* info, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !poses || robot_stride < 0 || !status || !info) return fail(c, LIW_EINVAL, "liw_fmap_render: bad argument");
    if (liw_fmap_dev::launch_render((char*)store, c->L, nullptr, poses, c->Til, robot_stride, sel, status, info, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_fmap_render: kernel launch failed");
    return LIW_OK;
}

int liw_fmap_num_submaps(liw_fmap_ctx* c, const void* store, int robot) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    return hdr[liw_fmap_dev::H_NSUB];
}

int liw_fmap_full(liw_fmap_ctx* c, const void* store, int robot) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    return hdr[liw_fmap_dev::H_FULL] != 0;
}

int liw_fmap_get_submap(liw_fmap_ctx* c, const void* store, int robot, int k, int cap, double* points) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (k < 0 || k >= hdr[liw_fmap_dev::H_NSUB] || cap < 0 || (cap > 0 && !points)) return fail(c, LIW_EINVAL, "liw_fmap_get_submap: no such sub-map or bad argument");
    const size_t base = (size_t)robot * c->L.robot_bytes;
    int off[2];
    if (!pull(store, base + c->L.r_off + (size_t)k * 4, off, 2)) return fail(c, LIW_EHIP, "liw_fmap_get_submap: hipMemcpy");
    const int n = off[1] - off[0];
    if (!pull(store, base + c->L.r_pts + (size_t)off[0] * 24, points, (size_t)std::min(n, cap) * 3)) return fail(c, LIW_EHIP, "liw_fmap_get_submap: hipMemcpy");
    return n;
}

int liw_fmap_get_tf(liw_fmap_ctx* c, const void* store, int robot, int cap, double* tf12) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (cap < 0 || (cap > 0 && !tf12)) return fail(c, LIW_EINVAL, "liw_fmap_get_tf: bad argument");
    const int n = hdr[liw_fmap_dev::H_NTF];
    if (!pull(store, (size_t)robot * c->L.robot_bytes + c->L.r_tf, tf12, (size_t)std::min(n, cap) * 12)) return fail(c, LIW_EHIP, "liw_fmap_get_tf: hipMemcpy");
    return n;
}

int liw_fmap_last_info(liw_fmap_ctx* c, const void* store, int robot, liw_map_info* info, int* status) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = robot_header(c, store, robot, hdr)) return r;
    if (status) *status = hdr[liw_fmap_dev::H_STATUS];
    if (info && !pull(store, (size_t)robot * c->L.robot_bytes + liw_fmap_dev::HB_INFO, info, 1)) return fail(c, LIW_EHIP, "liw_fmap_last_info: hipMemcpy");
    return LIW_OK;
}

long long liw_fmap_get(liw_fmap_ctx* c, const void* store, int robot, signed char* out, long long cap) {
    LIW_FLEET_DEV(c);
    liw_map_info mi;
    if (int r = liw_fmap_last_info(c, store, robot, &mi, nullptr)) return r;
    if (cap < 0 || (cap > 0 && !out)) return fail(c, LIW_EINVAL, "liw_fmap_get: bad argument");
    const long long n = (long long)mi.width * mi.height;
    if (!pull(store, (size_t)robot * c->L.robot_bytes + c->L.r_grid, out, (size_t)std::min(n, cap))) return fail(c, LIW_EHIP, "liw_fmap_get: hipMemcpy");
    return n;
}

const signed char* liw_fmap_device_data(liw_fmap_ctx* c, const void* store, int robot) {
    if (!c || !store || robot < 0 || robot >= c->L.B) return nullptr;
    return (const signed char*)store + (size_t)robot * c->L.robot_bytes + c->L.r_grid;
}

int liw_fmap_write_pgm(liw_fmap_ctx* c, const void* store, int robot, const char* path_stem, const unsigned char* palette4) {
    LIW_FLEET_DEV(c);
    liw_map_info mi;
    if (int r = liw_fmap_last_info(c, store, robot, &mi, nullptr)) return r;
    const long long n = (long long)mi.width * mi.height;
    std::vector<signed char> g((size_t)(n > 0 ? n : 1));
    const long long r = liw_fmap_get(c, store, robot, g.data(), n);
    if (r < 0) return (int)r;
    if (liw_map_write_pgm_grid(path_stem, g.data(), mi.width, mi.height, mi.resolution, mi.origin_x, mi.origin_y, palette4))
        return fail(c, LIW_EINVAL, "liw_fmap_write_pgm: cannot write the files");
    return LIW_OK;
}

}  // extern "C"
