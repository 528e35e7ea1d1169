/* rtr_accum.h — the accumulation contract of rtr_accumulate_paths and the gather rule of rtr_gather_records: what one vertex of a
 * path adds to its pixel, and the throughput the path goes on with.
 *
 * One definition for the host (rtr_host_accumulate_paths, rtr_host_gather_records) and the device (k_accumulate_paths,
 * k_gather_records), in IEEE-754 binary32 multiplications and additions alone, compiled with -ffp-contract=off on both sides, so that
 * the kernel's words can be held to the host's bits (tests/test_gpu_accum.py) and both to a sum formed one operation at a time
 * (api.path_trace*).  Uses rtr_math.h and rtr_types.h only; the render kernels (kernels/rtr_device.h) do not include this header.
 *
 * ROW k < numPaths, per channel, every operation rounded once and in this order:
 *   1. kind = radiance[k].kind; rad = radiance[k].shadowed.
 *   2. kind == RTR_SURFACE_LIGHT with RTR_ACCUM_LIGHTS_FROM_EMITTERS: rad = emitters ? emitters[k].radiance : 0.
 *   3. kind == RTR_SURFACE_MISS with RTR_ACCUM_MISSES_FROM_ESCAPES:   rad = escapes ? escapes[k].radiance : 0.
 *   4. term = T[k] * rad.
 *   5. with skySums (rtr_shade_sky's 16-B rows): term = term + T[k] * skySums[4k .. 4k + 2].
 *   6. id = pathIds ? pathIds[k] : k.
 *   7. id < numSlots: accum[id] = accum[id] + term; outTerm[id] = term when outTerm is given.  RTR_PATH_NONE, the id rtr_compact_paths
 *      writes behind the survivors, is never below numSlots: such a row touches neither image.
 *   8. with bounces and outThroughput: outThroughput[3k ..] = T[k] * bounces[k].weight, for EVERY k.
 * Without the flags a light hit or a miss adds `shadowed` (the light's colour, the sky): the camera vertex's rule.  A term of zero is
 * still added.  The ids below numSlots must be distinct: there are no atomics, and an image row named twice ends up holding one of
 * the two results.
 *
 * GATHER: out[j] = src[rows[j]] when rows[j] < numSrc, else a record of zero bytes.
 *
 * Used by: kernels/rtr_accum.hip (device), rtr_accum_host.cpp (host).
 */
#ifndef RTR_ACCUM_H
#define RTR_ACCUM_H

#include "rtr_math.h"
#include "rtr_types.h"

/* steps 2 and 3: does a row of this kind take its radiance from the emitter (escape) records? */
RTR_HD int rtr_accum_from_emitters(uint32_t kind, uint32_t flags) { return (kind == RTR_SURFACE_LIGHT) & ((flags & RTR_ACCUM_LIGHTS_FROM_EMITTERS) != 0u); }
RTR_HD int rtr_accum_from_escapes(uint32_t kind, uint32_t flags) { return (kind == RTR_SURFACE_MISS) & ((flags & RTR_ACCUM_MISSES_FROM_ESCAPES) != 0u); }

/* steps 4 and 5; sky: the row's three sky-sum floats, read only with hasSky */
RTR_HD void rtr_accum_term(const float T[3], const float rad[3], int hasSky, const float sky[3], float term[3]) {
    for (int c = 0; c < 3; ++c) term[c] = T[c] * rad[c];
    if (hasSky)
        for (int c = 0; c < 3; ++c) {
            const float s = T[c] * sky[c];
            term[c] = term[c] + s;
        }
}

/* step 7's test */
RTR_HD int rtr_accum_slot_ok(uint32_t id, uint32_t numSlots) { return id < numSlots; }

/* step 8 */
RTR_HD void rtr_accum_next_throughput(const float T[3], const float weight[3], float outT[3]) {
    for (int c = 0; c < 3; ++c) outT[c] = T[c] * weight[c];
}

/* the gather's test */
RTR_HD int rtr_gather_row_ok(uint32_t row, uint32_t numSrc) { return row < numSrc; }

#endif /* RTR_ACCUM_H */
