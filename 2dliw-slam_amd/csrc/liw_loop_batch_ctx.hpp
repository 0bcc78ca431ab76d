// liw_loop_batch_ctx.hpp — the fleet loop detector's handle, private to its host files: liw_loop_batch.cpp creates and destroys it,
// liw_loop_cross.cpp (include/liw_loop_cross.h) reads its layout and parameters.
#pragma once
#include "k_loop_batch.hpp"
#include "liw_host_common.hpp"

struct liw_floop_ctx : liw_fleet_ctx_base {
    liw_floop_dev::Lay L{};
    liw_floop_dev::Prm P{};
};
