/* rtr_mirrored.h — the mirrored bit of an instance, ONE function for the host (rtr_api.cpp, set_mirrored_word) and the device
 * (kernels/rtr_bvh.hip, k_write_instances) so that the two cannot drift.  Not part of include/rtr_math.h: that header is the fp32
 * numerical contract and its probe (tests/math_probe) holds every function of it; this is one double-precision expression. */
#pragma once
#include <stdint.h>
#include "../../../include/rtr_math.h"

/* 1 iff the determinant of the 3x3 part of the row-major 3x4 `m` is negative.  Evaluated in double, in exactly this expression and
 * operation order; the float -> double conversions are exact and, with no step fused (-ffp-contract=off), every product, difference
 * and sum is one IEEE operation on the host and on gfx950 alike: the same bit on both sides, whatever the magnitude of det. */
RTR_HD uint32_t rtr_mirrored_bit(const float* m) {
    const double det = (double)m[0] * ((double)m[5] * m[10] - (double)m[6] * m[9]) - (double)m[1] * ((double)m[4] * m[10] - (double)m[6] * m[8]) +
                       (double)m[2] * ((double)m[4] * m[9] - (double)m[5] * m[8]);
    return det < 0.0 ? 1u : 0u;
}
