// cand_rule16 (aruco_amd/csrc/cand_rule.h) against a loop that looks at one pixel at a time: every own row x every column of the tile x
// structured and random rows above, both kinds (the kind is the candidate pixel's own bit). Host C++ only.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../aruco_amd/csrc/cand_rule.h"

static int scalar_rule(uint32_t mid16, uint32_t up16, int j, uint32_t* kind) {
    const int avail = 16 - j;
    bool mid[16], up[16];
    for (int k = 0; k < avail; k++) mid[k] = (mid16 >> (j + k)) & 1u, up[k] = (up16 >> (j + k)) & 1u;
    const bool hole = !mid[0];
    *kind = hole ? 1u : 0u;
    int run = 0;
    while (run < avail && mid[run] != hole) run++;       // outer: set pixels, hole: clear pixels
    const int last = hole ? run - 1 : run;
    const int hi = last < avail - 1 ? last : avail - 1;
    for (int k = hole ? 1 : 2; k <= hi; k++)
        if (up[k] != hole) return ah::CAND_DROP;         // outer: a set pixel above, hole: a clear one
    return run < avail ? ah::CAND_KEEP : ah::CAND_LONG;
}

int main() {
    std::vector<uint32_t> ups = {0x0000u, 0xFFFFu, 0x5555u, 0xAAAAu, 0x00FFu, 0xFF00u};
    for (int b = 0; b < 16; b++) ups.push_back(1u << b), ups.push_back(0xFFFFu ^ (1u << b));              // one blocker at every column
    for (int b = 1; b < 16; b++) ups.push_back((1u << b) - 1u), ups.push_back(0xFFFFu ^ ((1u << b) - 1u)); // runs from column 0 / up to column 15
    uint32_t s = 12345u;
    for (int i = 0; i < 64; i++) s = s * 1664525u + 1013904223u, ups.push_back((s >> 11) & 0xFFFFu);
    long checked = 0, by_result[2][3] = {};
    for (uint32_t mid = 0; mid < 65536u; mid++)
        for (uint32_t up : ups)
            for (int j = 0; j < 8; j++) {
                uint32_t k0 = 9, k1 = 9;
                const int want = scalar_rule(mid, up, j, &k0), got = ah::cand_rule16(up | (mid << 16), (uint32_t)j, &k1);
                if (want != got || k0 != k1) {
                    printf("mismatch: mid %04x up %04x j %d: kind %u / %u, result %d / %d\n", mid, up, j, k0, k1, want, got);
                    return 1;
                }
                by_result[k0][want]++;
                checked++;
            }
    for (int k = 0; k < 2; k++)
        for (int r = 0; r < 3; r++)
            if (!by_result[k][r]) {
                printf("kind %d never gave result %d\n", k, r);
                return 1;
            }
    printf("cand_rule16: %ld cases equal\n", checked);
    return 0;
}
