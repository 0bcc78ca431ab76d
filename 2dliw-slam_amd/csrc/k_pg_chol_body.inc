// k_pg_chol_body.inc — right-looking Cholesky of a packed lower triangle and both triangular solves, by a work-group of 256 threads:
// the text that k_fpg_reduced (k_posegraph_batch.hip), k_gj_reduced (k_group_joint.hip) and k_ggraph_solve (k_group_graph.hip) share, so
// that all run the same instructions.  In scope where it is included: double* A (the triangle, order nr), double* rhs, int nr, int tid; it defines
// bool ok (false when a pivot is not positive and finite) and leaves rhs <- A^-1 rhs.
    // right-looking Cholesky, a column per step; every thread reads the same pivot
    bool ok = true;
    for (int k = 0; k < nr; ++k) {
        const double piv = A[tri(k, k)];
        if (!(piv > 0.0) || !isfinite(piv)) ok = false;
        const double inv = 1.0 / sqrt(piv);
        __syncthreads();
        for (int i = k + tid; i < nr; i += 256) A[tri(i, k)] *= inv;   // i = k: sqrt(piv)
        __syncthreads();
        const int m = nr - k - 1;
        for (int e = tid; e < m * m; e += 256) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i) A[tri(i, j)] -= A[tri(i, k)] * A[tri(j, k)];
        }
        __syncthreads();
    }
    for (int k = 0; k < nr; ++k) {          // L y = b
        const double xk = rhs[k] / A[tri(k, k)];
        __syncthreads();
        if (tid == 0) rhs[k] = xk;
        for (int i = k + 1 + tid; i < nr; i += 256) rhs[i] -= A[tri(i, k)] * xk;
        __syncthreads();
    }
    for (int k = nr - 1; k >= 0; --k) {     // L^T x = y
        const double xk = rhs[k] / A[tri(k, k)];
        __syncthreads();
        if (tid == 0) rhs[k] = xk;
        for (int i = tid; i < k; i += 256) rhs[i] -= A[tri(k, i)] * xk;
        __syncthreads();
    }
