// liw_map.cpp — host side of the occupancy-grid map (C ABI include/liw_map.h; kernels in k_map.hip).
//
// The host keeps the sub-map offsets, composes T_w_l = make_tf(p, q) * T_imu_to_laser with the liw_lie_* routines, reads the
// bounds of a render back (six doubles: the one read-back before the ray kernel), derives width / height with the reference's
// arithmetic (visualization.cpp:412-413), checks the capacity, extends the accumulated step table (uploaded once per growth)
// and reads the counters back at the end.  The PGM / YAML writer works on a plain array.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liw_lie.h"
#include "../../include/liw_map.h"
#include "k_map.hpp"
#include "liw_host_common.hpp"

struct liw_ctx;
hipStream_t liw_ctx_stream(liw_ctx* c);
int liw_ctx_device(liw_ctx* c);
bool liw_ctx_has_device(liw_ctx* c);

namespace {

using liw_map_dev::Grid;
using liw_map_dev::kBlock;
using liw_map_dev::kCounters;

constexpr long long kMaxSteps = 1ll << 22;   // step-table entries at most (32 MB)

struct Layout {
    size_t pts, sub, tf, partial, bounds, counters, bits, grid, bytes;
};


int layout(const liw_map_params* p, const liw_map_dims* d, Layout* L) {
    if (!p || !(p->resolution > 0) || !std::isfinite(p->resolution)) return LIW_EINVAL;
    if (!d || d->max_submaps < 1 || d->max_points < 1 || d->max_cells < 1) return LIW_EINVAL;
    if (d->max_cells > 0x7FFFFFF0ll || d->max_points > 0x7FFFFFF0ll) return LIW_EINVAL;   // cell and block indices are 32-bit
    const size_t K = (size_t)d->max_submaps, P = (size_t)d->max_points, Cn = ((size_t)d->max_cells + 15) & ~(size_t)15;
    size_t o = 0;
    L->pts = o; o = al256(o + P * 24);
    L->sub = o; o = al256(o + P * 4);
    L->tf = o; o = al256(o + K * 96);
    L->partial = o; o = al256(o + ((P + kBlock - 1) / kBlock) * 48);
    L->bounds = o; o = al256(o + 48);
    L->counters = o; o = al256(o + kCounters * 8);
    L->bits = o; o = al256(o + Cn);
    L->grid = o; o = al256(o + Cn);
    L->bytes = o;
    return LIW_OK;
}

const unsigned char kDefaultPalette[4] = {205, 254, 0, 0};

}  // namespace

struct liw_map {
    liw_ctx* ctx = nullptr;
    liw_map_params p{};
    liw_map_dims dims{};
    Layout L{};
    bool have_device = false;
    bool store_failed = false;
    char* store = nullptr;
    double* dT = nullptr;        // device step table
    size_t dT_cap = 0, dT_n = 0; // entries allocated / uploaded
    std::vector<double> T;       // host step table
    double Til[12];              // T_imu_to_laser
    std::vector<long long> off{0};   // sub-map k holds points off[k] .. off[k + 1]
    liw_map_info cur{};          // of the grid held
    long long probe[3] = {0, 0, 0}; // SAMPLED atomics / cell visits / HIT atomics of the last render
    std::string err;

    int fail(int code, const char* what) { err = what; return code; }
    template <class T_> T_* dev(size_t o) const { return (T_*)(store + o); }
};

namespace {

#define MAP_NEED_DEVICE(h)                                                                                   \
    do {                                                                                                     \
        if (!(h)) return LIW_EINVAL;                                                                         \
        if ((h)->store_failed) return LIW_ENOMEM;   /* err keeps the hipMalloc message */                  \
        if (!(h)->have_device) return (h)->fail(LIW_ENODEV, "no usable gfx950 device (no CPU fallback)"); \
        (void)hipSetDevice(liw_ctx_device((h)->ctx));                                                        \
    } while (0)

void extend_table(std::vector<double>& T, double step, size_t n) {
    if (T.empty()) T.push_back(0.0);
    T.reserve(n);
    while (T.size() < n) T.push_back(T.back() + step);   // the accumulated tr of `for (tr = 0; ...; tr += step)`
}

}  // namespace

extern "C" {

int liw_map_store_bytes(const liw_map_params* params, const liw_map_dims* dims, size_t* bytes) {
    Layout L{};
    if (!bytes || layout(params, dims, &L)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

int liw_map_step_table(double resolution, int n, double* T) {
    if (!(resolution > 0) || !std::isfinite(resolution) || n < 0 || (n > 0 && !T)) return LIW_EINVAL;
    const double step = resolution / 2;
    double tr = 0;
    for (int k = 0; k < n; ++k, tr += step) T[k] = tr;
    return LIW_OK;
}

liw_map* liw_map_create(liw_ctx* ctx, const liw_map_params* params, const liw_map_dims* dims) {
    Layout L{};
    if (!ctx || layout(params, dims, &L)) return nullptr;
    liw_map* h = new liw_map();
    h->ctx = ctx;
    h->p = *params;
    h->dims = *dims;
    h->L = L;
    h->cur.resolution = params->resolution;
    double Mw[16], Ml[16];
    liw_get_extrinsics(ctx, Mw, Ml);
    liw_lie_from_matrix16(Ml, 0, h->Til);
    if (liw_ctx_has_device(ctx)) {
        (void)hipSetDevice(liw_ctx_device(ctx));
        if (hipMalloc((void**)&h->store, L.bytes) == hipSuccess) h->have_device = true;
        else {
            h->store = nullptr;
            h->store_failed = true;
            h->err = "liw_map_create: hipMalloc of the " + std::to_string(L.bytes) + "-byte store failed (dims too large)";
        }
    } else {
        h->err = "no usable gfx950 device (no CPU fallback)";
    }
    return h;
}

void liw_map_destroy(liw_map* h) {
    if (!h) return;
    if (h->store) (void)hipFree(h->store);
    if (h->dT) (void)hipFree(h->dT);
    delete h;
}

const char* liw_map_last_error(liw_map* h) { return h ? h->err.c_str() : "null handle"; }
int liw_map_num_submaps(liw_map* h) { return h ? (int)h->off.size() - 1 : LIW_EINVAL; }

int liw_map_add_submap(liw_map* h, int n_points, const double* points) {
    MAP_NEED_DEVICE(h);
    if (n_points < 0 || (n_points > 0 && !points)) return h->fail(LIW_EINVAL, "liw_map_add_submap: bad argument");
    const int k = (int)h->off.size() - 1;
    if (k >= h->dims.max_submaps) return h->fail(LIW_ENOMEM, "liw_map_add_submap: max_submaps sub-maps held");
    const long long base = h->off.back();
    if (base + n_points > h->dims.max_points) return h->fail(LIW_ENOMEM, "liw_map_add_submap: max_points points would be exceeded");
    if (n_points) {
        const std::vector<int> ids((size_t)n_points, k);
        if (hipMemcpy(h->dev<double>(h->L.pts) + base * 3, points, sizeof(double) * 3 * (size_t)n_points, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->dev<int>(h->L.sub) + base, ids.data(), sizeof(int) * (size_t)n_points, hipMemcpyHostToDevice) != hipSuccess)
            return h->fail(LIW_EHIP, "liw_map_add_submap: hipMemcpy");
    }
    h->off.push_back(base + n_points);
    return k;
}

int liw_map_clear(liw_map* h) {
    if (!h) return LIW_EINVAL;
    h->off.assign(1, 0);
    h->cur = liw_map_info{};
    h->cur.resolution = h->p.resolution;
    return LIW_OK;
}

int liw_map_render_tf(liw_map* h, int K, const double* T_w_l, liw_map_info* info) {
    MAP_NEED_DEVICE(h);
    if (K < 0 || K > (int)h->off.size() - 1 || (K > 0 && !T_w_l)) return h->fail(LIW_EINVAL, "liw_map_render_tf: bad argument");
    hipStream_t s = liw_ctx_stream(h->ctx);
    const long long npts = h->off[(size_t)K];
    const double res = h->p.resolution, step = res / 2;
    liw_map_info mi{};
    mi.resolution = res;
    double b[6] = {0, 0, 0, 0, 0, 0};
    if (npts > 0) {
        (void)hipMemcpyAsync(h->dev<double>(h->L.tf), T_w_l, sizeof(double) * 12 * (size_t)K, hipMemcpyHostToDevice, s);
        if (liw_map_dev::launch_bounds(h->dev<double>(h->L.pts), h->dev<int>(h->L.sub), h->dev<double>(h->L.tf), npts, h->dev<double>(h->L.partial),
                                       h->dev<double>(h->L.bounds), s))
            return h->fail(LIW_EHIP, "liw_map_render_tf: kernel launch failed");
        (void)hipMemcpyAsync(b, h->dev<double>(h->L.bounds), sizeof b, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) return h->fail(LIW_EHIP, "liw_map_render_tf: hipStreamSynchronize");
    }
    mi.rays = (long long)b[5];
    if (mi.rays == 0) {   // no valid point: a 0 x 0 map
        h->cur = mi;
        if (info) *info = mi;
        return LIW_OK;
    }
    const double wd = (b[1] - b[0]) / res + 1, hd = (b[3] - b[2]) / res + 1;   // visualization.cpp:412-413
    mi.origin_x = b[0];
    mi.origin_y = b[2];
    if (!(wd < 2147483647.0) || !(hd < 2147483647.0)) {
        mi.width = mi.height = 2147483647;
        if (info) *info = mi;
        return h->fail(LIW_ENOMEM, "liw_map_render_tf: the bounding box needs more than max_cells cells");
    }
    mi.width = (int)wd;
    mi.height = (int)hd;
    if (info) *info = mi;
    const long long ncell = (long long)mi.width * mi.height;
    if (ncell > h->dims.max_cells) return h->fail(LIW_ENOMEM, "liw_map_render_tf: the bounding box needs more than max_cells cells");
    const double nsteps = b[4] / step;
    if (!(nsteps < (double)(kMaxSteps - 3))) return h->fail(LIW_EINVAL, "liw_map_render_tf: a ray is longer than 2^22 - 3 steps");
    const size_t need = (size_t)nsteps + 3;   // k_map_rays looks one entry past int(len / step)
    if (need > h->dT_n) {
        size_t n = h->T.size() > 2048 ? h->T.size() : 2048;
        while (n < need) n *= 2;
        extend_table(h->T, step, n);
        if (n > h->dT_cap) {
            if (h->dT) (void)hipFree(h->dT);
            h->dT = nullptr;
            h->dT_cap = h->dT_n = 0;
            if (hipMalloc((void**)&h->dT, sizeof(double) * n) != hipSuccess) return h->fail(LIW_ENOMEM, "liw_map_render_tf: hipMalloc of the step table");
            h->dT_cap = n;
        }
        if (hipMemcpyAsync(h->dT, h->T.data(), sizeof(double) * n, hipMemcpyHostToDevice, s) != hipSuccess)
            return h->fail(LIW_EHIP, "liw_map_render_tf: hipMemcpy of the step table");
        h->dT_n = n;
    }
    const Grid g{mi.width, mi.height, mi.origin_x, mi.origin_y, res, step};
    unsigned long long* cnt = h->dev<unsigned long long>(h->L.counters);
    unsigned long long c[kCounters];
    if (liw_map_dev::launch_clear(h->dev<uint8_t>(h->L.bits), ncell, cnt, s) ||
        liw_map_dev::launch_rays(h->dev<double>(h->L.pts), h->dev<int>(h->L.sub), h->dev<double>(h->L.tf), npts, h->dT, (int)h->dT_n, g,
                                 h->dev<uint8_t>(h->L.bits), cnt, s) ||
        liw_map_dev::launch_finish(h->dev<uint8_t>(h->L.bits), ncell, h->dev<signed char>(h->L.grid), cnt, s))
        return h->fail(LIW_EHIP, "liw_map_render_tf: kernel launch failed");
    (void)hipMemcpyAsync(c, cnt, sizeof c, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) return h->fail(LIW_EHIP, "liw_map_render_tf: hipStreamSynchronize");
    mi.samples = (long long)c[0];
    mi.free_cells = (long long)c[1];
    mi.hit_once = (long long)c[2];
    mi.hit_more = (long long)c[3];
    mi.unknown = ncell - mi.free_cells - mi.hit_once - mi.hit_more;
    h->cur = mi;
    h->probe[0] = (long long)c[4];
    h->probe[1] = (long long)c[5];
    h->probe[2] = (long long)c[6];
    if (info) *info = mi;
    return LIW_OK;
}

int liw_map_render(liw_map* h, int K, const double* poses, liw_map_info* info) {
    MAP_NEED_DEVICE(h);
    if (K < 0 || (K > 0 && !poses)) return h->fail(LIW_EINVAL, "liw_map_render: bad argument");
    std::vector<double> tf((size_t)K * 12);
    for (int k = 0; k < K; ++k) {
        double A[12];
        liw_lie_make_tf(poses + (size_t)k * 6, poses + (size_t)k * 6 + 3, A);
        liw_lie_mul(A, h->Til, &tf[(size_t)k * 12]);
    }
    return liw_map_render_tf(h, K, tf.data(), info);
}

int liw_map_last_info(liw_map* h, liw_map_info* info) {
    if (!h || !info) return LIW_EINVAL;
    *info = h->cur;
    return LIW_OK;
}

long long liw_map_get(liw_map* h, signed char* out, long long cap) {
    MAP_NEED_DEVICE(h);
    if (cap < 0 || (cap > 0 && !out)) return h->fail(LIW_EINVAL, "liw_map_get: bad argument");
    const long long n = (long long)h->cur.width * h->cur.height, m = n < cap ? n : cap;
    if (m > 0 && hipMemcpy(out, h->dev<signed char>(h->L.grid), (size_t)m, hipMemcpyDeviceToHost) != hipSuccess)
        return h->fail(LIW_EHIP, "liw_map_get: hipMemcpy");
    return n;
}

int liw_map_probe_counts(liw_map* h, long long* atomics, long long* visits, long long* hit_atomics) {
    if (!h) return LIW_EINVAL;
    if (atomics) *atomics = h->probe[0];
    if (visits) *visits = h->probe[1];
    if (hit_atomics) *hit_atomics = h->probe[2];
    return LIW_OK;
}

const signed char* liw_map_device_data(liw_map* h) { return h && h->have_device ? h->dev<signed char>(h->L.grid) : nullptr; }

int liw_map_write_pgm_grid(const char* path_stem, const signed char* data, int width, int height, double resolution, double origin_x,
                           double origin_y, const unsigned char* palette4) {
    if (!path_stem || width < 0 || height < 0 || ((long long)width * height > 0 && !data)) return LIW_EINVAL;
    const unsigned char* pal = palette4 ? palette4 : kDefaultPalette;
    const std::string stem(path_stem);
    std::vector<unsigned char> row((size_t)width);
    FILE* f = fopen((stem + ".pgm").c_str(), "wb");
    if (!f) return LIW_EINVAL;
    fprintf(f, "P5\n%d %d\n255\n", width, height);
    for (int y = height - 1; y >= 0; --y) {   // top row of the image = highest y
        for (int x = 0; x < width; ++x) {
            const int v = data[(size_t)y * width + x];
            const int e = v == -1 ? 0 : v == 0 ? 1 : v == 50 ? 2 : v == 100 ? 3 : -1;
            if (e < 0) { fclose(f); return LIW_EINVAL; }
            row[(size_t)x] = pal[e];
        }
        if (width && fwrite(row.data(), 1, (size_t)width, f) != (size_t)width) { fclose(f); return LIW_EINVAL; }
    }
    if (fclose(f)) return LIW_EINVAL;
    const size_t slash = stem.find_last_of('/');
    FILE* y = fopen((stem + ".yaml").c_str(), "w");
    if (!y) return LIW_EINVAL;
    fprintf(y, "image: %s.pgm\nresolution: %.17g\norigin: [%.17g, %.17g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n",
            stem.substr(slash == std::string::npos ? 0 : slash + 1).c_str(), resolution, origin_x, origin_y);
    return fclose(y) ? LIW_EINVAL : LIW_OK;
}

int liw_map_write_pgm(liw_map* h, const char* path_stem, const unsigned char* palette4) {
    MAP_NEED_DEVICE(h);
    const long long n = (long long)h->cur.width * h->cur.height;
    std::vector<signed char> g((size_t)(n > 0 ? n : 1));
    const long long r = liw_map_get(h, g.data(), n);
    if (r < 0) return (int)r;
    if (liw_map_write_pgm_grid(path_stem, g.data(), h->cur.width, h->cur.height, h->cur.resolution, h->cur.origin_x, h->cur.origin_y, palette4))
        return h->fail(LIW_EINVAL, "liw_map_write_pgm: cannot write the files");
    return LIW_OK;
}

}  // extern "C"
