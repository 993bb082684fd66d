// The run rule of one border-start candidate on the 16 pixels at hand (candidates_sparse_kernel, k_contours.hip). Plain C++ without HIP
// types, so that tests/cpp/cand_rule_check.cpp can compare it on the CPU with a loop that looks at one pixel at a time.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CAND_RULE_FN __host__ __device__ __forceinline__
#else
#define CAND_RULE_FN inline
#endif

namespace ah {

enum { CAND_DROP = 0, CAND_KEEP = 1, CAND_LONG = 2 };   // CAND_LONG: the run leaves the 16 pixels, the 64-pixel test (run_rule_tiles) decides

// rows: bits 0..15 = the row above the candidate's, bits 16..31 = its own row, each the 8 pixels of the candidate's tile followed by the 8 of the
// right neighbour tile; j = the candidate's column in its tile. A start-rule pixel that is clear is a hole start (*kind = 1), one that is set an
// outer start (*kind = 0). With avail = 16 - j pixels from the candidate on:
//   outer - Lr = its run of set pixels (at most avail); no set pixel in the row above at columns 2 .. min(Lr, avail - 1) of the run
//   hole  - Lr = its run of clear pixels;               no clear pixel in the row above at columns 1 .. min(Lr - 1, avail - 1)
CAND_RULE_FN int cand_rule16(uint32_t rows, uint32_t j, uint32_t* kind_out) {
    const int avail = 16 - (int)j;
    const uint32_t up = (rows & 0xFFFFu) >> j, mid = rows >> (16 + j);
    const uint32_t kind = ~mid & 1u;
    const uint32_t runbits = (kind ? mid : ~mid) | (1u << avail);
    const int Lr = __builtin_ctz(runbits);
    const int last = Lr - (int)kind;                                  // hole: Lr - 1, outer: Lr
    const int hi = last < avail - 1 ? last : avail - 1;
    const uint32_t span = ((2u << hi) - 1u) & ~(3u >> kind);         // hole: columns 1 .. hi, outer: columns 2 .. hi
    *kind_out = kind;
    if ((up ^ (0u - kind)) & span) return CAND_DROP;                  // hole: a clear pixel above, outer: a set one
    return Lr < avail ? CAND_KEEP : CAND_LONG;
}

}  // namespace ah
