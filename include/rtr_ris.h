/* rtr_ris.h — the resampling contract of rtr_pick_slots_ris: a path vertex's P light picks each chosen among M candidates of the
 * light-power table (include/rtr_power.h) in proportion to what the candidate would contribute at THIS vertex — resampled importance
 * sampling (RIS; Talbot et al. 2005) through a streaming weighted reservoir.  The table knows the lights; the target knows the vertex:
 * its BRDF, both cosines, the distance, the light's colour and its one-sidedness.  One shadow ray per pick, as before.
 *
 * One definition for the host (rtr_host_ris_candidates, rtr_host_ris_select) and the device (k_pick_slots_ris, kernels/rtr_query.hip),
 * in the terms of rtr_math.h, compiled with -ffp-contract=off on both sides, so that the kernel's words can be held to the host's
 * (tests/test_gpu_ris.py).  Everything of the rule is here EXCEPT the evaluation of a contribution, which is the device's
 * area_sample_contrib (kernels/rtr_device.h): the target is a float the caller of the rule supplies.  Uses rtr_power.h and what it
 * includes; the render kernels do not include this header.
 *
 * With Ttot, ns, A = Ttot * ns, total, weight_t and bf as in rtr_power.h, M = numCandidates (1 ... RTR_RIS_MAX_CANDIDATES) and
 * s0 = bf + 7919 * (depth + 1):
 * CANDIDATES.  Candidate j of pick p is a slot t * ns + s drawn exactly as rtr_power_pick draws: the triangle by a search of the table
 * for rtr_power_target(rtr_random(seedT)), the sample by rtr_pick_slot_of(rtr_random(seedS), ns).  j = 0 takes the power pick's own two
 * seeds, seedT = rtr_pick_seed(bf, depth, p) and seedS = seedT + 50: M = 1 IS the power pick.  j >= 1 takes seedT = s0 + 5000 + 48 p +
 * 3 j and seedS = seedT + 1.  The reservoir number of candidate j (any j) is u_j = rtr_random(s0 + 5000 + 48 p + 3 j + 2).  The largest
 * offset is 5000 + 48 * 29 + 47 = 6439 < 7919, the smallest is above the sky's 4900 and the sample numbers' 3350 (the SEEDS paragraph
 * of rtr_power.h): no draw of the vertex is reused.  total == 0 or ns == 0 gives RTR_PICK_NONE for every candidate.
 * TARGET.  phat_j, the caller's: for the kernel the largest channel of the unshadowed contribution rtr_shade_hits_picked would evaluate
 * at the slot (times wPick_j under RTR_RIS_MIS).  A value that is not finite or not > 0 counts as 0.
 *     r_j = phat_j * rtr_power_pick_weight(total, 1, weight_{t_j})          phat / q up to the constant ns; 0 where it is not finite
 * SELECTION, a streaming weighted reservoir without any per-lane array: W = 0 and nothing held; for j = 0 ... M - 1 in order, if
 * r_j > 0:  W = W + r_j, and the candidate is taken when nothing is held yet or when u_j * W < r_j.  Candidate j ends up held with
 * probability r_j / W.  The result is the held candidate's (slot, phat).
 * WEIGHT, for rtr_shade_hits_picked(weights):
 *     w = (W / phat_y) / (float)(M * P)          times wPick_y under RTR_RIS_MIS
 * RTR_PICK_NONE and weight 0 when nothing is held or w is not finite (a W that overflowed).  No output word is ever a NaN or an
 * infinity.
 * UNBIASED (DESIGN.md section 3 has the derivation).  The candidates are i.i.d. from q(slot) = pTri / ns.  With F(slot) = c_slot / ns,
 * E[F(y) / phat(y) * (1 / M) sum_j phat_j / q_j] = sum_slots F wherever phat > 0 on the support of F, which is the area sum of the
 * light loops over the triangles that emit; the P picks carry 1 / P each.  A slot whose contribution has no positive channel has
 * target 0 and is dropped — the "negative radiance is not light" exception of rtr_power.h — and the 24-bit RESOLUTION note there
 * applies unchanged.
 * MIS (RTR_RIS_MIS).  The pick side estimates the integral of F * wPick, wPick the function rtr_power_mis_weights gives for the
 * candidate's triangle, distance, cosine, bounce density and P: the target is max3(c) * wPick and the weight carries wPick_y.  The
 * bounce side stays rtr_emitter_hits_power; wPick + wBounce = 1 at every point, so the pair is unbiased.  It is NOT the balance
 * heuristic of the RIS density, which has no closed form.
 *
 * Used by: kernels/rtr_query.hip (device), rtr_ris_host.cpp (host).
 */
#ifndef RTR_RIS_H
#define RTR_RIS_H

#include "rtr_power.h"

#define RTR_RIS_SEED_OFFSET 5000u            /* behind s0: the first of the resampling draws */
#define RTR_RIS_PICK_STRIDE 48u              /* 3 numbers for each of 16 candidates */
#define RTR_RIS_CANDIDATE_STRIDE 3u          /* the triangle, the sample, the reservoir number */

/* the first of the three seeds of candidate j of pick p (for j = 0 only the third, the reservoir number's, is read) */
RTR_HD uint32_t rtr_ris_seed(uint32_t baseFrame, uint32_t depth, uint32_t p, uint32_t j) {
    return baseFrame + 7919u * (depth + 1u) + RTR_RIS_SEED_OFFSET + RTR_RIS_PICK_STRIDE * p + RTR_RIS_CANDIDATE_STRIDE * j;
}

/* candidate j of pick p: its slot and the weight of its triangle; RTR_PICK_NONE and 0 when the table's total over Ttot triangles is 0 */
RTR_HD uint32_t rtr_ris_candidate(const uint64_t* cdf, uint32_t Ttot, uint32_t ns, uint32_t baseFrame, uint32_t depth, uint32_t p, uint32_t j,
                                  uint32_t* weightT) {
    *weightT = 0u;
    const uint64_t total = rtr_power_total(cdf, Ttot);
    if (total == 0u || ns == 0u) return RTR_PICK_NONE;
    uint32_t seedT, seedS;
    if (j == 0u) { seedT = rtr_pick_seed(baseFrame, depth, p); seedS = seedT + RTR_POWER_SAMPLE_OFFSET; }
    else { seedT = rtr_ris_seed(baseFrame, depth, p, j); seedS = seedT + 1u; }
    const uint32_t t = rtr_power_search(cdf, Ttot, rtr_power_target(rtr_random(seedT), total));
    const uint32_t s = rtr_pick_slot_of(rtr_random(seedS), ns);
    *weightT = rtr_power_weight_at(cdf, t);
    return t * ns + s;
}

/* u_j */
RTR_HD float rtr_ris_number(uint32_t baseFrame, uint32_t depth, uint32_t p, uint32_t j) {
    return rtr_random(rtr_ris_seed(baseFrame, depth, p, j) + 2u);
}

/* the target as the rule uses it */
RTR_HD float rtr_ris_target(float phat) { return (phat > 0.0f && rtr_bounce_finite(phat)) ? phat : 0.0f; }

/* a pick's loop state: four scalars */
typedef struct rtr_ris_reservoir {
    float W;                 /* the sum of the r_j so far */
    uint32_t slot;           /* the held candidate, RTR_PICK_NONE while nothing is held */
    float phat, wPick;       /* its target, and what the caller handed in beside it (wPick under RTR_RIS_MIS) */
} rtr_ris_reservoir;

RTR_HD void rtr_ris_begin(rtr_ris_reservoir* r) { r->W = 0.0f; r->slot = RTR_PICK_NONE; r->phat = 0.0f; r->wPick = 0.0f; }

/* one candidate: slot (RTR_PICK_NONE: none), the weight of its triangle, its target as rtr_ris_target gives it, wPick and u_j */
RTR_HD void rtr_ris_step(rtr_ris_reservoir* r, uint64_t total, uint32_t weightT, uint32_t slot, float target, float wPick, float u) {
    if (slot == RTR_PICK_NONE || weightT == 0u || !(target > 0.0f)) return;
    const float rj = target * rtr_power_pick_weight(total, 1u, weightT);
    if (!(rj > 0.0f) || !rtr_bounce_finite(rj)) return;
    r->W = r->W + rj;
    if (r->slot == RTR_PICK_NONE || u * r->W < rj) { r->slot = slot; r->phat = target; r->wPick = wPick; }
}

/* the pick: its slot and its weight; mis: the weight carries the held wPick */
RTR_HD uint32_t rtr_ris_finish(const rtr_ris_reservoir* r, uint32_t M, uint32_t P, uint32_t mis, float* weight) {
    *weight = 0.0f;
    if (r->slot == RTR_PICK_NONE) return RTR_PICK_NONE;
    float w = (r->W / r->phat) / (float)(M * P);
    if (mis) w = w * r->wPick;
    if (!rtr_bounce_finite(w)) return RTR_PICK_NONE;
    *weight = w;
    return r->slot;
}

#endif /* RTR_RIS_H */
