// The device pieces marker mapping (k_map.hip) and camera rigs (k_rig.hip) share: the scan that lists a view's observations, the
// damped 6 x 6 solve that eliminates a pose, and the step of the shared blocks from the reduced Levenberg-Marquardt system, a Cholesky
// solve by one workgroup for any dimension (up to 378 marker unknowns, up to 90 camera unknowns).
#pragma once
#include "internal.h"
#include "pnp_device.h"

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

// The body of the one-workgroup solve kernels, all T threads: delta holds the reduced right-hand side of nblocks blocks of 6 unknowns
// and gets the step, zero when the solve failed (a rejected step: st->solve_failed, which an elimination may have set already).
// pose is [2][nblocks + 1][6], block 0 the gauge: pose[other] = pose[cur] - step. Thread 0 leaves |step|^2 and |parameters|^2 in st.
template <int T>
__device__ __forceinline__ void reduced_step_block(double* S, double* delta, double* pose, int nblocks, LmCtl* st, double* s_col, double* s_b,
                                                   double* s_piv, int* s_fail) {
    const int N = 6 * nblocks, n = nblocks + 1, tid = threadIdx.x;
    for (int i = tid; i < N; i += T) s_b[i] = delta[i];
    const int fail = chol_solve_block<T>(S, N, s_col, s_b, s_piv, s_fail, tid);
    const int cur = st->cur;
    for (int i = tid; i < N; i += T) {
        const double dl = fail ? 0. : s_b[i];
        s_b[i] = dl, delta[i] = dl;
        pose[((size_t)(1 - cur) * n + 1) * 6 + i] = pose[((size_t)cur * n + 1) * 6 + i] - dl;
    }
    __syncthreads();
    if (tid == 0) {
        double dn = 0, pn = 0;
        for (int i = 0; i < N; i++) {
            const double v = pose[((size_t)cur * n + 1) * 6 + i];
            dn += s_b[i] * s_b[i], pn += v * v;
        }
        st->sdn = dn, st->spn = pn, st->solve_failed |= fail;
    }
}

// One lane: bc = U^-1 bc for the damped 6 x 6 block U of an eliminated pose. A U that cannot be solved gives a zero bc and sets
// *solve_failed: the step is rejected (lm_decide).
__device__ __forceinline__ void solve_damped6(const double* U, double* bc, int32_t* solve_failed) {
    double Uc[36];
#pragma unroll
    for (int a = 0; a < 36; a++) Uc[a] = U[a];
    if (!solve_static<6>(Uc, bc)) {
        atomicOr(solve_failed, 1);
#pragma unroll
        for (int a = 0; a < 6; a++) bc[a] = 0;
    }
}

// One wave. The observations [lo, hi) that belong to `owner` (obs_owner null: all of them) and carry one of the nlisted <= 128 listed
// ids, in detection order, the first of a repeated id: s_m[k] = the id's place in the list, s_o[k] = the observation. Returns their
// number, on every lane; the lists are lane 0's writes, visible after the caller's barrier.
__device__ __forceinline__ int listed_scan(const int32_t* obs_owner, int owner, const int32_t* obs_id, int lo, int hi, const int32_t* ids, int nlisted,
                                           int lane, int* s_m, int* s_o) {
    int n = 0;
    unsigned long long seen0 = 0, seen1 = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        int bi = -1;
        if (i < hi && (!obs_owner || obs_owner[i] == owner)) {
            const int id = obs_id[i];
            for (int j = 0; j < nlisted; j++)
                if (ids[j] == id) {
                    bi = j;
                    break;
                }
        }
        unsigned long long mask = __ballot(bi >= 0);
        while (mask) {
            const int j = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int b = __shfl(bi, j, 64);
            unsigned long long& seen = b < 64 ? seen0 : seen1;
            if ((seen >> (b & 63)) & 1) continue;
            seen |= 1ull << (b & 63);
            if (lane == 0) s_m[n] = b, s_o[n] = base + j;
            n++;   // n <= nlisted: every listed id enters once
        }
    }
    return n;
}

}  // namespace ah
