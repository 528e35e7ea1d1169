/* rtr_paths.h — the survival contract of rtr_compact_paths: which paths of a wavefront go on, and with what throughput.
 *
 * One definition for the host (rtr_host_compact_paths) and the device (k_compact_count, k_compact_scatter), in the terms of
 * rtr_math.h: comparisons, one rtr_random and IEEE-754 binary32 divisions, compiled with -ffp-contract=off on both sides, so that the
 * kernels' records can be held to the host's bits (tests/test_gpu_compact.py).  Uses rtr_math.h and rtr_types.h only; the render
 * kernels (kernels/rtr_device.h) do not include this header.
 *
 * LIVE: the path's ray would cost a walk — origin and direction finite, direction not zero, tmax > tmin: what rtr_trace_rays documents
 * for a miss without a walk, negated — every channel of its throughput T is finite and >= 0, and the largest channel is > 0.
 * ROULETTE (RTR_COMPACT_ROULETTE, live paths only): p = max(max3(T), survivalFloor); with p >= 1 the path goes on with T unchanged and
 * no number is drawn; else it goes on iff rtr_random(seed + frame + 7919 * (depth + 1) + 300) < p, with T / p.  rtr_random can return
 * exactly 1.0: that path dies for every p < 1.  E[outT] = p * T / p = T: the estimator keeps its mean.
 *
 * Used by: kernels/rtr_paths.hip (device), rtr_paths_host.cpp (host).
 */
#ifndef RTR_PATHS_H
#define RTR_PATHS_H

#include "rtr_math.h"
#include "rtr_types.h"

RTR_HD int rtr_path_finite(float x) { return (rtr_f2u(x) & 0x7f800000u) != 0x7f800000u; }

/* would this ray cost a walk? */
RTR_HD int rtr_path_ray_walks(const RtrRay* r) {
    const int finite = rtr_path_finite(r->origin[0]) & rtr_path_finite(r->origin[1]) & rtr_path_finite(r->origin[2]) &
                       rtr_path_finite(r->direction[0]) & rtr_path_finite(r->direction[1]) & rtr_path_finite(r->direction[2]);
    const int nonzero = (r->direction[0] != 0.0f) | (r->direction[1] != 0.0f) | (r->direction[2] != 0.0f);
    return finite & nonzero & (r->tmax > r->tmin);       /* a NaN tmin or tmax compares false */
}

/* 1 and outT (the throughput the path goes on with) when the path survives; 0 and outT = 0 when it does not.  seed is read only when
 * a number is drawn (the flag set, the path live, p < 1). */
RTR_HD int rtr_path_survive(const RtrRay* ray, const float T[3], uint32_t seed, const rtr_compact_params* p, float outT[3]) {
    outT[0] = 0.0f; outT[1] = 0.0f; outT[2] = 0.0f;
    if (!rtr_path_ray_walks(ray)) return 0;
    const float t0 = T[0], t1 = T[1], t2 = T[2];
    if (!(rtr_path_finite(t0) & rtr_path_finite(t1) & rtr_path_finite(t2) & (t0 >= 0.0f) & (t1 >= 0.0f) & (t2 >= 0.0f))) return 0;
    float m = t0 > t1 ? t0 : t1;
    m = m > t2 ? m : t2;
    if (!(m > 0.0f)) return 0;
    if (p->flags & RTR_COMPACT_ROULETTE) {
        const float q = m < p->survivalFloor ? p->survivalFloor : m;
        if (q < 1.0f) {
            const float u = rtr_random(seed + p->frame + 7919u * (p->depth + 1u) + 300u);
            if (!(u < q)) return 0;
            outT[0] = t0 / q; outT[1] = t1 / q; outT[2] = t2 / q;
            return 1;
        }
    }
    outT[0] = t0; outT[1] = t1; outT[2] = t2;
    return 1;
}

#endif /* RTR_PATHS_H */
