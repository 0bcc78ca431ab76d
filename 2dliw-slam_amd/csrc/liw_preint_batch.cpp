// liw_preint_batch.cpp — host side of the fleet's pre-integration (C ABI include/liw_preint_batch.h; kernels in k_preint_batch.hip):
// the store layout, argument checks, the launches and the synchronous getter.  No per-robot work happens here.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/liw_preint_batch.h"
#include "k_preint_batch.hpp"
#include "liw_host_common.hpp"

namespace {

using namespace liw_fpre_dev;

bool make_lay(const liw_fpre_dims* d, Lay* L) {
    if (!d || d->B < 1 || d->B > (1 << 20)) return false;
    L->B = d->B;
    L->robot_bytes = (size_t)kRobotDoubles * 8;
    L->s_P = (size_t)L->B * L->robot_bytes;
    L->shared_bytes = al256((size_t)L->B * 225 * 8);
    L->bytes = L->s_P + L->shared_bytes;
    return true;
}

}  // namespace

struct liw_fpre_ctx : liw_fleet_ctx_base {
    Lay L{};
    liw::PreintNoise N{};
};

extern "C" {

int liw_fpre_layout(const liw_fpre_dims* dims, liw_fpre_layout_info* out) {
    Lay L{};
    if (!out || !make_lay(dims, &L)) return LIW_EINVAL;
    out->bytes = L.bytes;
    out->robot_bytes = L.robot_bytes;
    out->shared_off = L.s_P;
    out->shared_bytes = L.shared_bytes;
    out->X_off = (size_t)R_X * 8;
    out->J_off = (size_t)R_J * 8;
    out->P_off = (size_t)R_P * 8;
    out->imu_last_off = (size_t)R_LACC * 8;
    out->wheel_off = (size_t)R_WDELTA * 8;
    out->pending_off = (size_t)R_STAMP * 8;
    out->latch_off = (size_t)R_LATCH * 8;
    out->mat_pitch = kPitch;
    return LIW_OK;
}

int liw_fpre_store_bytes(const liw_fpre_dims* dims, size_t* bytes) {
    Lay L{};
    if (!bytes || !make_lay(dims, &L)) return LIW_EINVAL;
    *bytes = L.bytes;
    return LIW_OK;
}

liw_fpre_ctx* liw_fpre_create(const liw_params* prm, const liw_fpre_dims* dims) {
    Lay L{};
    if (!prm || !make_lay(dims, &L)) return nullptr;
    liw_fpre_ctx* c = new liw_fpre_ctx();
    c->L = L;
    c->device = prm->device;
    for (int k = 0; k < 3; ++k) {   // as liw_imu_preint_create / liw_wheel_preint_create
        c->N.q_na[k] = prm->imu_noise_acc_sigma[k] * prm->imu_noise_acc_sigma[k];
        c->N.q_nw[k] = prm->imu_noise_gyro_sigma[k] * prm->imu_noise_gyro_sigma[k];
        c->N.q_nba[k] = prm->imu_bias_acc_sigma[k] * prm->imu_bias_acc_sigma[k];
        c->N.q_nbw[k] = prm->imu_bias_gyro_sigma[k] * prm->imu_bias_gyro_sigma[k];
        c->N.wheel_cov[k] = prm->wheel_sigma[k] * prm->wheel_sigma[k];
    }
    c->have_device = liw_probe_gfx950(c->device, &c->err);
    return c;
}

void liw_fpre_destroy(liw_fpre_ctx* c) { delete c; }
const char* liw_fpre_last_error(liw_fpre_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int liw_fpre_reset(liw_fpre_ctx* c, void* store, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store)) return fail(c, LIW_EINVAL, "liw_fpre_reset: store");
    if (launch_reset((char*)store, c->L, mask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_fpre_reset: kernel launch failed");
    return LIW_OK;
}

int liw_fpre_push(liw_fpre_ctx* c, void* store, const int* imu_off, const double* imu, const int* wheel_off, const double* wheel,
                  const double* stamps, const double* bias, const unsigned char* mask, double* imu_X, double* imu_J, double* imu_sqrtP,
                  double* imu_Dt, double* wheel_T, double* wheel_sqrtP, double* wheel_Dt, unsigned char* ready, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !imu_off || !imu || !wheel_off || !wheel || !stamps || !bias || !imu_X || !imu_J || !imu_sqrtP || !imu_Dt || !wheel_T ||
        !wheel_sqrtP || !wheel_Dt || !ready)
        return fail(c, LIW_EINVAL, "liw_fpre_push: bad argument");
    const Rows out{imu_X, imu_J, imu_sqrtP, imu_Dt, wheel_T, wheel_sqrtP, wheel_Dt, ready};
    if (launch_push((char*)store, c->L, c->N, imu_off, imu, wheel_off, wheel, stamps, bias, mask, out, (hipStream_t)stream))
        return fail(c, LIW_EHIP, "liw_fpre_push: kernel launch failed");
    return LIW_OK;
}

int liw_fpre_commit(liw_fpre_ctx* c, void* store, const unsigned char* taken, const unsigned char* mask, void* stream) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || !taken) return fail(c, LIW_EINVAL, "liw_fpre_commit: bad argument");
    if (launch_commit((char*)store, c->L, taken, mask, (hipStream_t)stream)) return fail(c, LIW_EHIP, "liw_fpre_commit: kernel launch failed");
    return LIW_OK;
}

int liw_fpre_get(liw_fpre_ctx* c, const void* store, int robot, liw_fpre_state* out) {
    LIW_FLEET_DEV(c);
    if (bad_store(store) || robot < 0 || robot >= c->L.B || !out) return fail(c, LIW_EINVAL, "liw_fpre_get: store, robot or out");
    double R[R_USED];
    if (!pull(store, (size_t)robot * c->L.robot_bytes, R, (size_t)R_USED)) return fail(c, LIW_EHIP, "liw_fpre_get: hipMemcpy");
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->X, R + R_X, sizeof(out->X));
    for (int r = 0; r < 15; ++r)
        for (int k = 0; k < 15; ++k) { out->J[r * 15 + k] = R[R_J + r * kPitch + k]; out->P[r * 15 + k] = R[R_P + r * kPitch + k]; }
    std::memcpy(out->last_acc, R + R_LACC, sizeof(out->last_acc));
    std::memcpy(out->last_gyro, R + R_LGYR, sizeof(out->last_gyro));
    out->last_add_imu_time = R[R_ILAST];
    out->imu_Dt = R[R_IDT];
    std::memcpy(out->delta_Tij, R + R_WDELTA, sizeof(out->delta_Tij));
    std::memcpy(out->last_pose, R + R_WPOSE, sizeof(out->last_pose));
    std::memcpy(out->v, R + R_WV, sizeof(out->v));
    std::memcpy(out->omega, R + R_WOM, sizeof(out->omega));
    out->last_update_time = R[R_WUPD];
    out->last_add_time = R[R_WADD];
    out->wheel_Dt = R[R_WDT];
    out->pending_stamp = R[R_STAMP];
    std::memcpy(out->pending_bias, R + R_BIAS, sizeof(out->pending_bias));
    const unsigned char* latch = (const unsigned char*)(R + R_LATCH);
    out->imu_inited = latch[0];
    out->wheel_odom_inited = latch[1];
    return LIW_OK;
}

}  // extern "C"
