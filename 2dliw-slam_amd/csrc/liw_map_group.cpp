// liw_map_group.cpp — host side of the shared occupancy-grid map of a group of fleet robots (C ABI include/liw_map_group.h; kernels
// in k_map_group.hip): the group store's layout, argument checks, the launches and the synchronous getters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_map_group.h"
#include "k_map_group.hpp"
#include "liw_host_common.hpp"

namespace {

using liw_fmap_dev::GLay;
using liw_fmap_dev::Lay;

bool make_glay(const liw_gmap_dims* d, GLay* GL) {
    if (!d || d->G < 1 || d->max_cells < 1 || d->max_cells > 0x7FFFFFF0) return false;
    GL->G = d->G; GL->C = d->max_cells;
    GL->Cn = ((size_t)GL->C + 15) & ~(size_t)15;
    // work-groups per group of the cell kernels, as the fleet map sizes them per robot
    const int per = std::max(64, 2048 / GL->G);
    GL->cchunk = (int)std::min<size_t>((GL->Cn / 16 + 255) / 256, (size_t)per);
    if ((long long)GL->G * GL->cchunk >= (1ll << 31)) return false;
    size_t o = 256;
    GL->g_bits = o; o = al256(o + GL->Cn);
    GL->g_grid = o; o = al256(o + GL->Cn);
    GL->group_bytes = o;
    GL->bytes = (size_t)GL->G * GL->group_bytes;
    return true;
}

}  // namespace

struct liw_gmap_ctx : liw_fleet_ctx_base {
    Lay L{};        // of the fleet map
    GLay GL{};
    double Til[12];
};

namespace {

// header words of a group; < 0 on error
int group_header(liw_gmap_ctx* c, const void* gstore, int group, int* hdr) {
    if (bad_store(gstore) || group < 0 || group >= c->GL.G) return fail(c, LIW_EINVAL, "liw_gmap: gstore or group");
    if (!pull(gstore, (size_t)group * c->GL.group_bytes, hdr, 8)) return fail(c, LIW_EHIP, "liw_gmap: hipMemcpy");
    return 0;
}

int render(liw_gmap_ctx* c, const char* what, void* store, void* gstore, const double* T_w_l, const double* poses, long long robot_stride,
           const int* group_of, const double* T_g_w, const unsigned char* gsel, int* gstatus, liw_map_info* ginfo, void* stream) {
    if (bad_store(store) || bad_store(gstore) || (!T_w_l && !poses) || robot_stride < 0 || !group_of || !gstatus || !ginfo) return fail(c, LIW_EINVAL, what);
    if (liw_fmap_dev::launch_group_render((char*)store, c->L, (char*)gstore, c->GL, T_w_l, poses, c->Til, robot_stride, group_of, T_g_w, gsel, gstatus,
                                          ginfo, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_gmap_render: kernel launch failed");
    return LIW_OK;
}

}  // namespace

extern "C" {

int liw_gmap_layout(const liw_gmap_dims* dims, liw_gmap_layout_info* out) {
    GLay GL{};
    if (!out || !make_glay(dims, &GL)) return LIW_EINVAL;
    out->bytes = GL.bytes;
    out->group_bytes = GL.group_bytes;
    out->cell_bytes = GL.Cn;
    out->bits_off = GL.g_bits;
    out->grid_off = GL.g_grid;
    out->cell_chunks = GL.cchunk;
    return LIW_OK;
}

int liw_gmap_store_bytes(const liw_gmap_dims* dims, size_t* bytes) {
    GLay GL{};
    if (!bytes || !make_glay(dims, &GL)) return LIW_EINVAL;
    *bytes = GL.bytes;
    return LIW_OK;
}

liw_gmap_ctx* liw_gmap_create(const liw_fmap_ctx* fleet, const liw_gmap_dims* dims) {
    GLay GL{};
    if (!fleet || !make_glay(dims, &GL)) return nullptr;
    const liw_fmap_dev::FmapView v = liw_fmap_dev::fmap_view(fleet);
    liw_gmap_ctx* c = new liw_gmap_ctx();
    c->L = v.L;
    c->GL = GL;
    std::memcpy(c->Til, v.Til, sizeof(c->Til));
    c->device = v.device;
    c->have_device = v.have_device;
    if (!c->have_device) c->err = "no usable gfx950 device (no CPU fallback)";
    return c;
}

void liw_gmap_destroy(liw_gmap_ctx* c) { delete c; }
const char* liw_gmap_last_error(liw_gmap_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_gmap_reset(liw_gmap_ctx* c, void* gstore, const unsigned char* gmask, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(gstore)) return fail(c, LIW_EINVAL, "liw_gmap_reset: gstore");
    if (liw_fmap_dev::launch_group_reset((char*)gstore, c->GL, c->L.res, gmask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_gmap_reset: kernel launch failed");
    return LIW_OK;
}

int liw_gmap_render_tf(liw_gmap_ctx* c, void* store, void* gstore, const double* T_w_l, long long robot_stride, const int* group_of,
                       const double* T_g_w, const unsigned char* gsel, int* gstatus, liw_map_info* ginfo, void* stream) {
    LIW_FLEET_DEV(c);
    return render(c, "liw_gmap_render_tf: bad argument", store, gstore, T_w_l, nullptr, robot_stride, group_of, T_g_w, gsel, gstatus, ginfo, stream);
}

int liw_gmap_render(liw_gmap_ctx* c, void* store, void* gstore, const double* poses, long long robot_stride, const int* group_of,
                    const double* T_g_w, const unsigned char* gsel, int* gstatus, liw_map_info* ginfo, void* stream) {
    LIW_FLEET_DEV(c);
    return render(c, "liw_gmap_render: bad argument", store, gstore, nullptr, poses, robot_stride, group_of, T_g_w, gsel, gstatus, ginfo, stream);
}

int liw_gmap_last_info(liw_gmap_ctx* c, const void* gstore, int group, liw_map_info* info, int* status) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = group_header(c, gstore, group, hdr)) return r;
    if (status) *status = hdr[liw_fmap_dev::GH_STATUS];
    if (info && !pull(gstore, (size_t)group * c->GL.group_bytes + liw_fmap_dev::HB_INFO, info, 1)) return fail(c, LIW_EHIP, "liw_gmap_last_info: hipMemcpy");
    return LIW_OK;
}

int liw_gmap_members(liw_gmap_ctx* c, const void* gstore, int group, int* robots, int* submaps) {
    LIW_FLEET_DEV(c);
    int hdr[8];
    if (int r = group_header(c, gstore, group, hdr)) return r;
    if (robots) *robots = hdr[liw_fmap_dev::GH_MEMBERS];
    if (submaps) *submaps = hdr[liw_fmap_dev::GH_SUBMAPS];
    return LIW_OK;
}

long long liw_gmap_get(liw_gmap_ctx* c, const void* gstore, int group, signed char* out, long long cap) {
    LIW_FLEET_DEV(c);
    liw_map_info mi;
    if (int r = liw_gmap_last_info(c, gstore, group, &mi, nullptr)) return r;
    if (cap < 0 || (cap > 0 && !out)) return fail(c, LIW_EINVAL, "liw_gmap_get: bad argument");
    const long long n = (long long)mi.width * mi.height;
    if (!pull(gstore, (size_t)group * c->GL.group_bytes + c->GL.g_grid, out, (size_t)std::min(n, cap))) return fail(c, LIW_EHIP, "liw_gmap_get: hipMemcpy");
    return n;
}

const signed char* liw_gmap_device_data(liw_gmap_ctx* c, const void* gstore, int group) {
    if (!c || !gstore || group < 0 || group >= c->GL.G) return nullptr;
    return (const signed char*)gstore + (size_t)group * c->GL.group_bytes + c->GL.g_grid;
}

int liw_gmap_write_pgm(liw_gmap_ctx* c, const void* gstore, int group, const char* path_stem, const unsigned char* palette4) {
    LIW_FLEET_DEV(c);
    liw_map_info mi;
    if (int r = liw_gmap_last_info(c, gstore, group, &mi, nullptr)) return r;
    const long long n = (long long)mi.width * mi.height;
    std::vector<signed char> g((size_t)(n > 0 ? n : 1));
    const long long r = liw_gmap_get(c, gstore, group, g.data(), n);
    if (r < 0) return (int)r;
    if (liw_map_write_pgm_grid(path_stem, g.data(), mi.width, mi.height, mi.resolution, mi.origin_x, mi.origin_y, palette4))
        return fail(c, LIW_EINVAL, "liw_gmap_write_pgm: cannot write the files");
    return LIW_OK;
}

}  // extern "C"
