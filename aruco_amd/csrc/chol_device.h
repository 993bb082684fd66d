// Cholesky solve of a reduced Levenberg-Marquardt system by one workgroup, for any dimension: the marker steps of marker mapping
// (k_map.hip, up to 378 unknowns) and the camera steps of a camera rig (k_rig.hip, up to 90).
#pragma once
#include "internal.h"

namespace ah {

// All T threads of the one workgroup call it. S = L L^T in place (right-looking; the matrix, N x N with its lower triangle filled,
// stays in HBM, the current column in s_col), L y = b, L^T x = y; s_b holds b on entry (the threads may have filled it just before
// the call: the first barrier in here makes it visible to all) and x on return. s_col and s_b: N doubles of LDS each, s_piv and s_fail
// one each. Returns whether the solve failed, on every thread: a pivot that is not positive or a solution that is not finite; s_b is
// then undefined.
template <int T>
__device__ __forceinline__ int chol_solve_block(double* S, int N, double* s_col, double* s_b, double* s_piv, int* s_fail, int tid) {
    if (tid == 0) *s_fail = 0;
    __syncthreads();
    for (int k = 0; k < N; k++) {
        if (tid == 0) {
            const double v = S[(size_t)k * N + k];
            if (!(v > 0) || !isfinite(v)) *s_fail = 1;
            *s_piv = sqrt(v);
            S[(size_t)k * N + k] = *s_piv;
        }
        __syncthreads();
        if (*s_fail) break;
        const double piv = *s_piv;
        for (int i = k + 1 + tid; i < N; i += T) {
            const double l = S[(size_t)i * N + k] / piv;
            S[(size_t)i * N + k] = l, s_col[i] = l;
        }
        __syncthreads();
        const int n = N - k - 1;
        for (int e = tid; e < n * n; e += T) {
            const int i = k + 1 + e / n, j = k + 1 + e % n;
            if (j <= i) S[(size_t)i * N + j] -= s_col[i] * s_col[j];
        }
        __syncthreads();
    }
    if (!*s_fail) {
        for (int k = 0; k < N; k++) {
            if (tid == 0) s_b[k] /= S[(size_t)k * N + k];
            __syncthreads();
            const double y = s_b[k];
            for (int i = k + 1 + tid; i < N; i += T) s_b[i] -= S[(size_t)i * N + k] * y;
            __syncthreads();
        }
        for (int k = N - 1; k >= 0; k--) {
            if (tid == 0) s_b[k] /= S[(size_t)k * N + k];
            __syncthreads();
            const double x = s_b[k];
            for (int i = tid; i < k; i += T) s_b[i] -= S[(size_t)k * N + i] * x;
            __syncthreads();
        }
        int bad = 0;
        for (int i = tid; i < N; i += T) bad |= !isfinite(s_b[i]);
        if (__syncthreads_or(bad) && tid == 0) *s_fail = 1;
    }
    __syncthreads();
    return *s_fail;
}

}  // namespace ah
