/* rtr_tree_sah.h — the SAH cost of a tree from its eleven integer sums, ONE function for the host (rtr_api.cpp: rtr_host_tree_cost,
 * rtr_scene_tree_cost) and the device (kernels/rtr_bvh.hip: the decide and close kernels of rtr_scene_rebuild_if_async) so that the two
 * cannot drift.  Like rtr_mirrored.h it is not part of include/rtr_math.h, the fp32 contract: this is one double-precision expression. */
#pragma once
#include <stdint.h>
#include "../../../include/rtr_math.h"

/* w: the words of k_tree_cost — innerArea[3], leafArea[3], rootArea[3], numInner, numLeafRefs — each area triple (dx dy, dy dz, dz dx) in
 * grid steps; sx, sy, sz: RtrBvhGrid::scale.  Evaluated in double, in exactly this order: the uint64 -> double and float -> double
 * conversions are correctly rounded (the second exact) and, with no step fused (-ffp-contract=off), every product, sum and the quotient
 * is one IEEE operation on the host and on gfx950 alike: the same bits on both sides. */
RTR_HD double rtr_tree_sah(const uint64_t* w, float scaleX, float scaleY, float scaleZ) {
    const double sx = scaleX, sy = scaleY, sz = scaleZ;
    const double inner = (double)w[0] * sx * sy + (double)w[1] * sy * sz + (double)w[2] * sz * sx;
    const double leaf = (double)w[3] * sx * sy + (double)w[4] * sy * sz + (double)w[5] * sz * sx;
    const double root = (double)w[6] * sx * sy + (double)w[7] * sy * sz + (double)w[8] * sz * sx;
    return root > 0.0 ? (inner * 1.0 + leaf * 1.0) / root : 0.0;
}
