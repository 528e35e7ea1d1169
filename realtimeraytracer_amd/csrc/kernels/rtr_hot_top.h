/* rtr_hot_top.h — which 4-wide records k_shadow_trace4 finds in LDS: the PRIORITY of a record, ONE function for the host
 * (bvh_build.cpp: hot_top_positions) and the device (kernels/rtr_bvh.hip: k_hot_top_select) so that the two cannot drift.
 *
 * The any-hit kernel keeps the first kTopNodes records of DeviceScene::nodes4 in LDS.  Shadow rays converge on the area lights and
 * enter the child nearest the light first, so the records they visit most are a few chains towards the lights, not the first levels.
 * The resident order therefore starts with a BEST-FIRST top: from the root, the inner child with the highest priority of any record
 * already in the set is appended, ties to the lower breadth-first index, until the set has `top` records; everything else follows in
 * breadth-first order.  Record 0 stays the root and a record still precedes its children.
 *
 * The priority of a record is the share of the sphere its box (the child box in its parent's record) covers as seen from the lights'
 * centres: sum over the area lights of min(1, box area / (4 pi d^2)), d the distance from the light's centre (the image of its frame's
 * origin: transform[12..14]) to the box, 1 where the centre is inside.  No lights: every priority is 0 and the order is breadth-first.
 *
 * fp32 + - * / and comparisons alone, every step one IEEE operation on both sides (-ffp-contract=off); the planes are decoded to
 * integers, exactly. */
#pragma once
#include <stdint.h>
#include "../../../include/rtr_math.h"
#include "../../../include/rtr_types.h"

/* the largest best-first top either side makes (k_hot_top_select's LDS arrays); kTopNodes of rtr_kernels.hip is at most 160 */
#define RTR_HOT_TOP_MAX 256u

/* a plane of a 4-wide record (IEEE binary16 bits: an integer number of grid steps about the wide centre, or an infinity) as fp32,
 * exact; infinities become +-65536 */
RTR_HD float rtr_hot_plane(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    float mag;
    if (e == 31u) mag = 65536.0f;
    else if (e == 0u) mag = (float)m * 5.9604644775390625e-08f;                /* 2^-24 */
    else mag = (float)(1024u + m) * rtr_u2f((e + 102u) << 23);                  /* 2^(e - 25) */
    return (h & 0x8000u) ? -mag : mag;
}

/* w: the three plane words of a child slot (xmin | ymin << 16, xmax | ymax << 16, zmin | zmax << 16); centres: 3 floats per light */
RTR_HD float rtr_hot_score(uint32_t w0, uint32_t w1, uint32_t w2, const RtrBvhGrid* g, const float* centres, uint32_t numLights, uint32_t stride) {
    const float c[3] = {(float)(g->wideCentreXY & 0xffffu), (float)(g->wideCentreXY >> 16), (float)(g->wideCentreZ & 0xffffu)};
    const uint32_t hlo[3] = {w0 & 0xffffu, w0 >> 16, w2 & 0xffffu}, hhi[3] = {w1 & 0xffffu, w1 >> 16, w2 >> 16};
    float lo[3], hi[3], d[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = (rtr_hot_plane(hlo[k]) + c[k]) * g->scale[k] + g->origin[k];
        hi[k] = (rtr_hot_plane(hhi[k]) + c[k]) * g->scale[k] + g->origin[k];
        d[k] = rtr_max(hi[k] - lo[k], 0.0f);
    }
    const float area = 2.0f * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
    float score = 0.0f;
    for (uint32_t l = 0; l < numLights; ++l) {
        float d2 = 0.0f;
        for (int k = 0; k < 3; ++k) {
            const float p = centres[(size_t)l * stride + k];
            const float out = rtr_max(rtr_max(lo[k] - p, p - hi[k]), 0.0f);
            d2 = d2 + out * out;
        }
        const float sphere = 12.566370614359172f * d2;
        score = score + (sphere > area ? area / sphere : 1.0f);
    }
    return score;
}
