// What the Schur-complement Levenberg-Marquardt solvers share on the device (k_calib.hip, k_map.hip, k_rig.hip): the control block
// at the head of every solver state, and the rule that decides about a candidate. The host drives it with lm_drive (handle.h).
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ah {

struct LmCtl {
    double cost;       // sum of squared residuals at the parameters in buffer `cur`
    double sdn, spn;   // |step|^2 and |parameters|^2 of the shared block, left by the solve of the reduced system
    int32_t lg;        // lambda = 10^lg (lm_lambda)
    int32_t cur;       // which of the two parameter buffers holds the accepted parameters
    int32_t done, iters, max_iter, attempts;
    int32_t err;       // the solver's own *_ERR_* bits, set by its start kernels
    int32_t solve_failed;   // a system of this attempt could not be solved: the candidate is rejected
};

// whether lm_decide will take a candidate of cost c: its error is not larger and every system of the attempt could be solved
__device__ inline bool lm_takes(const LmCtl& s, double c) { return !s.solve_failed && isfinite(c) && c <= s.cost; }

// CvLevMarq's rule, by one thread: a candidate that lm_takes is taken (returns true; the candidate's buffer becomes `cur`) and lambda
// falls tenfold, else lambda rises tenfold (stop above 1e16). Stop after max_iter accepted steps or when |step| / |params| <
// DBL_EPSILON; dn, pn: their squares over all blocks, read only for a candidate that is taken (a caller need not sum them for another).
__device__ inline bool lm_decide(LmCtl& s, double c, double dn, double pn) {
    s.attempts++;
    const bool take = lm_takes(s, c);
    if (take) {
        s.cur = 1 - s.cur, s.cost = c;
        s.lg = max(s.lg - 1, -16);
        s.iters++;
        if (s.iters >= s.max_iter || sqrt(dn) < DBL_EPSILON * sqrt(pn)) s.done = 1;
    } else if (++s.lg > 16) {
        s.done = 1;
    }
    s.solve_failed = 0;
    return take;
}

}  // namespace ah
