/* rtr_pick.h — the pick contract of rtr_light_rays_picked: which of a hit's area-light slots are sampled.
 *
 * One definition for the host (rtr_host_pick_slots) and the device (k_light_rays_picked), in the terms of rtr_math.h: 32-bit integer
 * words, one rtr_random, one binary32 product and one conversion, so that the kernel's slots can be held to the host's words
 * (tests/test_gpu_light_pick.py).  Uses rtr_math.h and rtr_types.h only; the render kernels do not include this header.
 *
 * SLOTS.  A hit has A = Ttot * ns area slots, Ttot = the triangles of the first numAreaLights lights, ns = numShadowRays: the first
 * Q - 1 slots of rtr_light_slots under the same numbers, slot j = sample j % ns of light triangle j / ns.
 * PICK p of a hit with seed base b (seeds[k], or the pixel's px * 733 + py * 1933: rtr_light_rays' rule) draws
 *     u = rtr_random(b + frame + 7919 * (depth + 1) + 400 + 100 * p)                                     in 32-bit words
 *     j = (uint32_t)(u * (float)A), clamped to A - 1        rtr_random can return exactly 1.0 (quirk Q2); RTR_PICK_NONE when A == 0
 * A <= RTR_PICK_MAX_SLOTS = 2^24: (float)A is exact and u, a multiple of 2^-32 rounded to 24 bits, reaches every slot.
 * SEEDS.  The offsets go on with the vertex's numbering: rtr_bounce_rays took + 0, + 100, + 200 and the roulette + 300 behind
 * b + frame + 7919 * (depth + 1); the RTR_PICK_MAX = 30 picks take + 400 ... + 3300.  The light samples of the same hit are seeded
 * s + b + frame and s + b + frame + 100 with s < ns <= 1024 (light_sample_pos), offsets 0 ... 1123 from b + frame; a pick's offset is
 * at least 7919 + 400 = 8319 and at most 7919 * (depth + 1) + 3300, which does not wrap around to 1123 or below while
 * depth + 1 <= 542 000 (7919 * 542 000 + 3300 < 2^32).  So no pick of a hit reads the number one of its light samples reads.
 * WEIGHT.  j is uniform over the A slots, so for the contribution c_j of slot j: E[Ttot * c_j] = Ttot / A * sum_j c_j =
 * sum_t (1 / ns) sum_s c_{t,s}, the area sum of the light loops.  P picks are averaged: the default weight of a pick is
 * (float)Ttot / (float)P.
 *
 * Used by: kernels/rtr_query.hip (device), rtr_pick_host.cpp (host).
 */
#ifndef RTR_PICK_H
#define RTR_PICK_H

#include "rtr_math.h"
#include "rtr_types.h"

/* the slot of the number u in [0, 1] among A slots */
RTR_HD uint32_t rtr_pick_slot_of(float u, uint32_t A) {
    if (A == 0u) return RTR_PICK_NONE;
    const uint32_t j = (uint32_t)(u * (float)A);
    return j < A ? j : A - 1u;
}

/* the seed of pick p of a vertex whose seed base + frame is baseFrame */
RTR_HD uint32_t rtr_pick_seed(uint32_t baseFrame, uint32_t depth, uint32_t p) {
    return baseFrame + 7919u * (depth + 1u) + 400u + 100u * p;
}

RTR_HD uint32_t rtr_pick_slot(uint32_t baseFrame, uint32_t depth, uint32_t p, uint32_t A) {
    return rtr_pick_slot_of(rtr_random(rtr_pick_seed(baseFrame, depth, p)), A);
}

/* the seed base of hit k: the caller's, or its pixel's (hit k is sample k % spp of pixel k / spp of a frame width pixels wide) */
RTR_HD uint32_t rtr_pick_base(const uint32_t* seeds, uint32_t k, uint32_t width, uint32_t spp) {
    if (seeds) return seeds[k];
    const uint32_t pix = k / spp;
    return (pix % width) * 733u + (pix / width) * 1933u;
}

#endif /* RTR_PICK_H */
