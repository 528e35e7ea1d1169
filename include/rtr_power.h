/* rtr_power.h — the power-proportional pick contract of rtr_pick_slots_power, rtr_mis_pick_weights_power and rtr_emitter_hits_power:
 * a path vertex's P light picks drawn in proportion to the emitted power of the light triangles instead of uniformly over them
 * (include/rtr_pick.h), their weights, and the balance heuristic between them and the vertex's one bounce (include/rtr_mis.h).
 *
 * One definition for the host (rtr_host_light_power, rtr_host_pick_slots_power, rtr_host_mis_weights_power,
 * rtr_host_emitter_hits_power) and the device (kernels/rtr_power.hip, and the power forms of k_mis_pick_weights and k_emitter_hits), in
 * the terms of rtr_math.h, compiled with -ffp-contract=off on both sides, so that the kernels' words can be held to the host's
 * (tests/test_gpu_power.py).  Uses rtr_math.h, rtr_types.h, rtr_pick.h, rtr_bounce.h and rtr_mis.h only; the render kernels do not
 * include this header.
 *
 * POWER.  Light triangle t of light l has pw_t = (max(max3(color_l), 0) * intensity_l) * area_t in binary32, in that order, area_t the
 * word of its light-triangle record; 0 where that is not finite or not positive.  The renderer's emitted radiance is
 * 10 col I / (pdfrec area) with pdfrec = 1 / (0.7 area): independent of the area, so the flux of a triangle is proportional to pw_t.
 * Two-sidedness does not enter: a vertex sees one side.
 * THE TABLE covers all light triangles of all lights, in rtr_scene_export_light_tris' order.  pwMax = the largest
 * pw_t (a float maximum does not depend on the order it is formed in); weight_t = 0 when pw_t == 0, else
 * max(1, (uint32_t)((pw_t / pwMax) * 1048576.0f)): at most 2^20, and no triangle that emits is ever left out.  cdf[t]: the inclusive
 * prefix sums, uint64_t.  INTEGERS, so the sums do not depend on the order they are formed in and the device's table equals the host's
 * word for word.  One table serves every numAreaLights: with Ttot the triangles of the first numAreaLights lights, total =
 * cdf[Ttot - 1] (at most 2^24 * 2^20 = 2^44).
 *
 * PICK p of a vertex with seed base + frame bf draws, with seed = rtr_pick_seed(bf, depth, p) — the uniform pick's seed: the two rules
 * are alternatives, a vertex uses one of them —
 *     u = rtr_random(seed)        target = min((uint64_t)((double)u * (double)total), total - 1)
 *     t = the first index in [0, Ttot) with cdf[t] > target (binary search)
 *     s = rtr_pick_slot_of(rtr_random(seed + 50), ns)        slot = t * ns + s
 * and RTR_PICK_NONE when total == 0.  A double holds the 24-bit u and any total below 2^53 exactly; their product is one IEEE rounding
 * on either compiler (the precedent is rtr_sky_target).  A triangle of weight 0 is never drawn: cdf[t] > target >= cdf[t - 1] needs
 * cdf[t] > cdf[t - 1].
 * SEEDS.  Behind s0 = bf + 7919 * (depth + 1) a vertex's draws take the offsets 0, 100, 200 (rtr_bounce_rays), 300 (the roulette),
 * 400 + 100 p for p < 30 (the picks: 400 ... 3300) and 3400 + 200 j, 3500 + 200 j for j < 8 (the sky: 3400 ... 4900): every one a
 * multiple of 100.  The sample numbers take 450 + 100 p (450 ... 3350), 50 modulo 100, so none of them is any of those; all offsets
 * stay below 7919, so the draws of depth + 1 begin behind them.  The light samples of the same hit read offsets 0 ... 1123 from bf
 * (rtr_pick.h), below 7919 + 450, and the sum does not wrap around to them while depth + 1 <= 542 000, as there.  The resampled picks
 * (rtr_ris.h) go on behind the sky: candidate j >= 1 of pick p takes 5000 + 48 p + 3 j and that + 1, and the reservoir number of any
 * candidate 5000 + 48 p + 3 j + 2 — 5002 ... 6439 for p < 30 and j < 16, above 4900 and 3350 and below 7919; candidate 0 is the pick
 * above, seeds and all.
 * RESOLUTION.  rtr_random gives 24-bit numbers k / 2^24 (and 1.0).  A table whose total is above 2^24 — more than 16 triangles of full
 * weight — has targets no draw can reach: the 2^24 numbers fall total / 2^24 weight units apart, so that a triangle of weight w is met
 * by about w 2^24 / total of them, and a triangle lighter than total / 2^24 by one or none.  The numbers are evenly spaced, so the
 * shares stay right to within one number per triangle, and the weight below divides by the table's share, not by the share of the
 * numbers; the error of the expectation is bounded by Ttot / 2^24 of the largest contribution.
 *
 * WEIGHT.  pTri_t = (float)weight_t / (float)total is the probability of triangle t, and a slot of it has pdf_slot = pTri_t / ns.
 * rtr_shade_hits_picked's rule 1 / (P pdf_slot ns) is then
 *     wPow = (float)total / ((float)P * (float)weight_t)
 * UNBIASED: with c_{t,s} the contribution of sample s of triangle t, E[wPow c] = sum_{t: weight_t > 0} pTri_t (1 / ns) sum_s
 * c_{t,s} / (P pTri_t) = (1 / P) sum_t (1 / ns) sum_s c_{t,s}, and P picks are summed: the area sum of the light loops over the
 * triangles that emit.  A triangle of weight 0 has pw_t == 0: col I <= 0 (or not finite), or no area — it contributes nothing to the
 * loops either (a negative radiance is not light; DESIGN.md section 3 has the exception).
 * MIS.  The balance heuristic of rtr_mis.h with pTri in place of 1 / Ttot:
 *     a = P * ((pTri * d^2) / area)      b = pb |cosL|      wPick = a / (a + b)      wBounce = b / (a + b)
 *     lightPdf = ((pTri * d^2) / area) / |cosL|
 * evaluated by ONE function on both sides (rtr_power_mis_weights): the pick side for the triangle it drew, the bounce side for the
 * triangle its ray met.  A hit triangle with index >= Ttot or weight 0 is the bounce's alone (pTri = 0: a = 0).  No double division
 * anywhere.
 *
 * Used by: kernels/rtr_power.hip, kernels/rtr_query.hip, kernels/rtr_mis.hip (device), rtr_power_host.cpp (host).
 */
#ifndef RTR_POWER_H
#define RTR_POWER_H

#include "rtr_math.h"
#include "rtr_types.h"
#include "rtr_pick.h"
#include "rtr_bounce.h"
#include "rtr_mis.h"

#define RTR_POWER_SCALE 1048576.0f          /* 2^20: the weight of the strongest triangle */
#define RTR_POWER_SAMPLE_OFFSET 50u         /* behind a pick's seed: the number that chooses the sample within the triangle */

/* pw_t from the light's words and the record's area */
RTR_HD float rtr_power_of(const float* color, float intensity, float area) {
    const float m = rtr_max(rtr_bounce_max3(rtr_ld3(color)), 0.0f);
    const float pw = (m * intensity) * area;
    if (!(pw > 0.0f) || !rtr_bounce_finite(pw)) return 0.0f;
    return pw;
}

/* weight_t: pwMax is the largest pw of the table (pw <= pwMax, so the quotient is at most 1) */
RTR_HD uint32_t rtr_power_weight(float pw, float pwMax) {
    if (!(pw > 0.0f)) return 0u;
    const float q = (pw / pwMax) * RTR_POWER_SCALE;
    return q >= 1.0f ? (uint32_t)q : 1u;
}

/* weight_t read back from the sums */
RTR_HD uint32_t rtr_power_weight_at(const uint64_t* cdf, uint32_t t) { return (uint32_t)(cdf[t] - (t ? cdf[t - 1u] : 0u)); }

RTR_HD uint64_t rtr_power_total(const uint64_t* cdf, uint32_t Ttot) { return Ttot ? cdf[Ttot - 1u] : 0u; }

/* u in [0, 1] -> floor(u * total), at most total - 1 (u == 1.0 stays in range); total != 0 */
RTR_HD uint64_t rtr_power_target(float u, uint64_t total) {
    double s = (double)u * (double)total;
    if (!(s >= 0.0)) s = 0.0;
    const uint64_t k = (uint64_t)s;
    return k < total ? k : total - 1u;
}

/* the first t in [0, Ttot) with cdf[t] > target; target < cdf[Ttot - 1] */
RTR_HD uint32_t rtr_power_search(const uint64_t* cdf, uint32_t Ttot, uint64_t target) {
    uint32_t lo = 0u, hi = Ttot - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

/* pTri_t; 0 for t >= Ttot, weight 0 or an empty table */
RTR_HD float rtr_power_ptri(const uint64_t* cdf, uint32_t Ttot, uint32_t t) {
    if (t >= Ttot) return 0.0f;
    const uint64_t total = cdf[Ttot - 1u];
    const uint32_t w = rtr_power_weight_at(cdf, t);
    if (total == 0u || w == 0u) return 0.0f;
    return (float)w / (float)total;
}

/* wPow of a pick that drew a triangle of weight w > 0 */
RTR_HD float rtr_power_pick_weight(uint64_t total, uint32_t P, uint32_t w) { return (float)total / ((float)P * (float)w); }

/* pick p of the vertex: its slot and its plain weight; RTR_PICK_NONE and 0 when the table's total over Ttot triangles is 0 */
RTR_HD uint32_t rtr_power_pick(const uint64_t* cdf, uint32_t Ttot, uint32_t ns, uint32_t baseFrame, uint32_t depth, uint32_t p, uint32_t P, float* weight) {
    *weight = 0.0f;
    const uint64_t total = rtr_power_total(cdf, Ttot);
    if (total == 0u || ns == 0u) return RTR_PICK_NONE;
    const uint32_t seed = rtr_pick_seed(baseFrame, depth, p);
    const uint32_t t = rtr_power_search(cdf, Ttot, rtr_power_target(rtr_random(seed), total));
    const uint32_t s = rtr_pick_slot_of(rtr_random(seed + RTR_POWER_SAMPLE_OFFSET), ns);
    *weight = rtr_power_pick_weight(total, P, rtr_power_weight_at(cdf, t));
    return t * ns + s;
}

/* rtr_mis_terms with pTri in place of 1 / Ttot.  Roundings: d * d, its product by pTri, the quotient by area and the product by (float)P
 * make a (4); b has 1. */
RTR_HD void rtr_power_mis_terms(float pb, float dist, float cosLight, float area, float pTri, uint32_t P, float* a, float* b) {
    *a = (pTri > 0.0f && P != 0u) ? (float)P * ((pTri * (dist * dist)) / area) : 0.0f;
    *b = pb > 0.0f ? pb * rtr_abs(cosLight) : 0.0f;
}

/* rtr_mis_weights with these terms, guard for guard: an input that is not finite, or a negative distance or area, gives three zeros;
 * a + b == 0 gives 0 and 0; a sum that overflows with finite inputs is all the pick's (1 and 0); lightPdf is 0 where it is not finite
 * and where nobody picks the triangle (pTri == 0).  No output is ever a NaN or an infinity. */
RTR_HD void rtr_power_mis_weights(float pb, float dist, float cosLight, float area, float pTri, uint32_t P, float* lightPdf, float* wPick, float* wBounce) {
    *lightPdf = 0.0f; *wPick = 0.0f; *wBounce = 0.0f;
    if (!(rtr_bounce_finite(pb) & rtr_bounce_finite(dist) & rtr_bounce_finite(cosLight) & rtr_bounce_finite(area) & rtr_bounce_finite(pTri))) return;
    if (dist < 0.0f || area < 0.0f || pTri < 0.0f) return;
    float a, b;
    rtr_power_mis_terms(pb, dist, cosLight, area, pTri, P, &a, &b);
    const float sum = a + b;
    if (!(sum > 0.0f)) return;                            /* 0, or a NaN from 0 / 0 (d == 0 on a triangle without area) */
    if (pTri > 0.0f) {
        const float q = ((pTri * (dist * dist)) / area) / rtr_abs(cosLight);
        if (rtr_bounce_finite(q)) *lightPdf = q;
    }
    if (!rtr_bounce_finite(sum)) {                        /* b is finite (pb and cosLight are): a overflowed */
        if (rtr_bounce_finite(b)) *wPick = 1.0f;
        return;
    }
    *wPick = a / sum;
    *wBounce = b / sum;
}

/* The pick side in one piece, for a pick that sends a ray to triangle t < Ttot: wPow * wPick, with what it was made from.  A triangle of
 * weight 0 — only a caller's slot can name one — has no wPow: weight 0, and lightPdf = wPick = 0. */
RTR_HD float rtr_power_mis_pick(const uint64_t* cdf, uint32_t Ttot, uint32_t t, uint32_t P, float pb, float dist, float cosLight, float area,
                                float* lightPdf, float* wPick) {
    float wBounce;
    const float pTri = rtr_power_ptri(cdf, Ttot, t);
    rtr_power_mis_weights(pb, dist, cosLight, area, pTri, P, lightPdf, wPick, &wBounce);
    if (!(pTri > 0.0f)) { *lightPdf = 0.0f; *wPick = 0.0f; return 0.0f; }
    return rtr_power_pick_weight(cdf[Ttot - 1u], P, rtr_power_weight_at(cdf, t)) * *wPick;
}

/* rtr_mis_emitter with these terms: the measurement and the record are rtr_mis.h's.  pTri: rtr_power_ptri of the hit triangle (0 for a
 * light the picks cannot reach). */
RTR_HD void rtr_power_mis_emitter(const RtrRay* ray, float t, const RtrSurface* prev, const RtrBounce* bounce, const float* rec, uint32_t lightTri,
                                  const float* lightColor, float intensity, uint32_t twoSided, float pTri, uint32_t P, RtrEmitter* e) {
    rtr_mis_emitter_zero(e);
    rtr_mis_emitter_geom m;
    if (!rtr_mis_emitter_measure(ray, t, prev, bounce, rec, twoSided, &m)) return;
    float a, b;
    rtr_power_mis_terms(m.pb, m.d, m.cosL, m.area, pTri, P, &a, &b);
    float lightPdf, wPick, wBounce;
    rtr_power_mis_weights(m.pb, m.d, m.cosL, m.area, pTri, P, &lightPdf, &wPick, &wBounce);
    rtr_mis_emitter_record(&m, a, b, lightPdf, wBounce, lightTri, lightColor, intensity, e);
}

#endif /* RTR_POWER_H */
