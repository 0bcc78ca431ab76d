// k_map_rays_body.inc — the body of a fleet ray kernel, included into k_fmap_rays (k_map_batch.hip: a robot's rays into its own grid)
// and k_gmap_rays (k_map_group.hip: into its group's).  In scope: store, L, R (the robot region the rays come from), c (its chunk of
// L.rchunk), sT (kLdsSteps doubles of LDS), and the macros RAYS_INFO (the held liw_map_info whose grid is drawn), RAYS_BITS (its cell
// bits), RAYS_TF (the transforms of R's sub-maps), RAYS_ROW (the info row).  The samples go into the held info and the row.
    const double* T = (const double*)(store + L.s_table);
    const int nl = L.S < kLdsSteps ? L.S : kLdsSteps;
    for (int e = threadIdx.x; e < nl; e += kBlock) sT[e] = T[e];
    __syncthreads();
    liw_map_info* hi = RAYS_INFO;
    const Grid g{hi->width, hi->height, hi->origin_x, hi->origin_y, L.res, L.res / 2};
    const int npts = ((const int*)R)[H_NPTS];
    const double* pts = (const double*)(R + L.r_pts);
    const int* sub = (const int*)(R + L.r_sub);
    const double* tf = RAYS_TF;
    uint8_t* bits = (uint8_t*)(RAYS_BITS);
    const int group = threadIdx.x / kRayLanes, s = threadIdx.x % kRayLanes;
    constexpr int kGroups = kBlock / kRayLanes;
    unsigned long long samples = 0, visits = 0, atomics = 0, hit_atomics = 0;   // the last three depend on the arrival order: not kept
    for (int ray = c * kGroups + group; ray < npts; ray += L.rchunk * kGroups) {
        const Ray r = liw_map_dev::make_ray(pts, sub, tf, ray);
        if (!r.valid) continue;
        liw_map_dev::walk_ray(r, g, sT, T, nl, s, bits, samples, visits, atomics, hit_atomics);
    }
    samples = liw_map_dev::wave_sum(samples);
    if ((threadIdx.x & 63) == 0 && samples) {
        atomicAdd((unsigned long long*)&hi->samples, samples);
        atomicAdd((unsigned long long*)&(RAYS_ROW).samples, samples);
    }
