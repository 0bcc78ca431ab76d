// map_serial — the occupancy-grid map as the literal serial walk in C++ (checker and the bench's 1-core baseline; nothing in
// the product uses it), written from the semantics of reference src/utilies/visualization.cpp:33-75 and :369-451 as
// include/liw_map.h states them.  Build with the host compiler, -O2 -ffp-contract=off (tests/map_reference.py build_serial).
#include <cmath>
#include <vector>

namespace {

struct ray { double O[3], P[3], d[3], len; };

long long cell_of(double cx, double cy, double ox, double oy, double res, int w, int h) {
    const double qx = (cx - ox) / res, qy = (cy - oy) / res;
    if (!(qx > -2147483648.0 && qx < 2147483648.0 && qy > -2147483648.0 && qy < 2147483648.0)) return -1;   // int() would overflow
    const int x = (int)qx, y = (int)qy;   // truncates toward zero
    if (x < 0 || x >= w || y < 0 || y >= h) return -1;
    return (long long)y * w + x;
}

}  // namespace

// K sub-maps: tf [K][12] (R row-major, t), n [K] point counts, pts [sum n][3].  Writes wh = {width, height}, origin = {x, y},
// counts = {rays, samples}; the grid [height][width] only if cap >= width * height.  Returns width * height.
extern "C" long long map_serial_render(int K, const double* tf, const int* n, const double* pts, double res, int* wh, double* origin,
                                       long long* counts, signed char* out, long long cap) {
    std::vector<ray> rays;
    const double* p = pts;
    for (int k = 0; k < K; ++k) {
        const double* T = tf + (long long)k * 12;
        for (int j = 0; j < n[k]; ++j, p += 3) {
            ray r;
            for (int i = 0; i < 3; ++i) {
                r.O[i] = T[9 + i];
                r.P[i] = ((T[3 * i] * p[0] + T[3 * i + 1] * p[1]) + T[3 * i + 2] * p[2]) + T[9 + i];
                r.d[i] = r.P[i] - r.O[i];
            }
            r.len = std::sqrt((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]);
            if (std::isfinite(r.P[0]) && std::isfinite(r.P[1]) && std::isfinite(r.P[2]) && std::isfinite(r.len)) rays.push_back(r);
        }
    }
    counts[0] = (long long)rays.size();
    counts[1] = 0;
    wh[0] = wh[1] = 0;
    origin[0] = origin[1] = 0.0;
    if (rays.empty()) return 0;
    double min_x = rays[0].P[0], max_x = min_x, min_y = rays[0].P[1], max_y = min_y;
    for (const ray& r : rays) {
        if (r.P[0] > max_x) max_x = r.P[0];
        if (r.P[0] < min_x) min_x = r.P[0];
        if (r.P[1] > max_y) max_y = r.P[1];
        if (r.P[1] < min_y) min_y = r.P[1];
    }
    const int w = (int)((max_x - min_x) / res + 1), h = (int)((max_y - min_y) / res + 1);
    wh[0] = w;
    wh[1] = h;
    origin[0] = min_x;
    origin[1] = min_y;
    const long long cells = (long long)w * h;
    if (cap < cells || !out) return cells;
    for (long long i = 0; i < cells; ++i) out[i] = -1;
    const double step = res / 2;
    for (const ray& r : rays) {
        if (r.len > 0.0) {
            const double ux = r.d[0] / r.len, uy = r.d[1] / r.len;
            for (double tr = 0; tr <= r.len; tr += step) {
                const long long idx = cell_of(r.O[0] + ux * tr, r.O[1] + uy * tr, min_x, min_y, res, w, h);
                if (idx > -1 && out[idx] == -1) out[idx] = 0;
                ++counts[1];
            }
        }
        const long long idx = cell_of(r.P[0], r.P[1], min_x, min_y, res, w, h);
        if (idx > -1) out[idx] = (out[idx] == -1 || out[idx] == 0) ? 50 : 100;
    }
    return cells;
}
