/* rtr_ris_host.cpp — rtr_host_ris_candidates, rtr_host_ris_select and the argument checks rtr_pick_slots_ris shares with them.  Pure
 * host C++ with no HIP in it: include/rtr_ris.h compiled for the host cores with the kernels' flags (-ffp-contract=off, no fast-math),
 * so that the device's words can be held to these; a translation unit of its own (with rtr_power_host.cpp, rtr_pick_host.cpp and
 * rtr_mis_host.cpp, whose checks it calls) so that a stand-alone program (tools/ris_host_check.cpp) can run it under the host
 * sanitizers. */
#include "rtr_ris_host.h"
#include "rtr_pick_host.h"
#include "rtr_power_host.h"
#include "../../include/rtr_ris.h"

#include <cstdint>

namespace rtrdev {

int ris_check_candidates(const char* who, uint32_t numCandidates) {
    return numCandidates == 0u || numCandidates > RTR_RIS_MAX_CANDIDATES
               ? refusef("%s: numCandidates %u (1 ... %u)", who, numCandidates, RTR_RIS_MAX_CANDIDATES) : RTR_OK;
}

int ris_check_params(const char* who, const rtr_ris_params* ris) {
    if (!ris) return refusef("%s: ris params is null", who);
    if (const int rc = ris_check_candidates(who, ris->numCandidates)) return rc;
    if (ris->flags & ~RTR_RIS_MIS) return refusef("%s: unknown flag bits 0x%x of ris params", who, ris->flags);
    if (ris->flags & RTR_RIS_MIS) {
        if (const int rc = check_lobes(who, ris->lobes)) return rc;
    } else if (ris->lobes != 0u) {
        return refusef("%s: lobes 0x%x without RTR_RIS_MIS (0: the lobes are the bounce's the picks are weighted against)", who, ris->lobes);
    }
    return check_reserved(who, ris->_reserved, 5, "ris params");
}

int ris_check_count(const char* who, uint32_t n, uint32_t picks, uint32_t candidates) {
    if (const int rc = check_fits_32(who, n, "hits", picks, "picks")) return rc;
    return check_fits_32(who, n * picks, "picks", candidates, "candidates");
}

int ris_check_call(const char* who, const RisCall& c) {
    if (!c.outCandidates != !c.outTargets)
        return refusef("%s: %s is null: outCandidates and outTargets come together", who, c.outCandidates ? "outTargets" : "outCandidates");
    if (c.n == 0u) return RTR_OK;
    const uint32_t P = c.pick->numPicks, M = c.ris->numCandidates;
    if (const int rc = ris_check_count(who, c.n, P, M)) return rc;
    const size_t picks = (size_t)c.n * P * 4u, cands = picks * M;
    const Arg in[3] = {{c.rays, "rays", 16, true, (size_t)c.n * sizeof(RtrRay)}, {c.hits, "hits", 16, true, (size_t)c.n * sizeof(RtrHit)},
                       {c.seeds, "seeds", 4, false, (size_t)c.n * 4u}};
    const Arg out[4] = {{c.outSlots, "outSlots", 4, true, picks}, {c.outWeights, "outWeights", 4, true, picks},
                        {c.outCandidates, "outCandidates", 4, false, cands}, {c.outTargets, "outTargets", 4, false, cands}};
    if (const int rc = check_ptrs(who, in)) return rc;
    if (const int rc = check_ptrs(who, out)) return rc;
    if (const int rc = check_pixel_seeds(who, c.seeds, c.light->width, c.light->spp)) return rc;
    return check_overlaps(who, in, 3, out, 4);
}

}  // namespace rtrdev

extern "C" int rtr_host_ris_candidates(const uint64_t* cdf, uint32_t tris, const uint32_t* seeds, uint32_t n, const rtr_light_params* p,
                                       const rtr_pick_params* pick, uint32_t numCandidates, uint32_t* outCandidates) {
    const char* who = "rtr_host_ris_candidates";
    if (const int rc = rtrdev::pick_check_params(who, p, pick, false)) return rc;
    if (const int rc = rtrdev::ris_check_candidates(who, numCandidates)) return rc;
    if (const int rc = rtrdev::power_check_table(who, cdf, tris)) return rc;
    if (const int rc = rtrdev::pick_check_area(who, (uint64_t)tris * p->numShadowRays)) return rc;
    if (n == 0u) return RTR_OK;
    const uint32_t P = pick->numPicks, M = numCandidates;
    if (const int rc = rtrdev::ris_check_count(who, n, P, M)) return rc;
    const rtrdev::Arg args[2] = {{outCandidates, "outCandidates", 4, true}, {seeds, "seeds", 4, false}};
    if (const int rc = rtrdev::check_ptrs(who, args)) return rc;
    if (const int rc = rtrdev::check_pixel_seeds(who, seeds, p->width, p->spp)) return rc;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t baseFrame = rtr_pick_base(seeds, k, p->width, p->spp) + p->frame;
        for (uint32_t q = 0; q < P; ++q)
            for (uint32_t j = 0; j < M; ++j) {
                uint32_t w;
                outCandidates[((size_t)k * P + q) * M + j] = rtr_ris_candidate(cdf, tris, p->numShadowRays, baseFrame, pick->depth, q, j, &w);
            }
    }
    return RTR_OK;
}

extern "C" int rtr_host_ris_select(const uint64_t* cdf, uint32_t tris, const uint32_t* seeds, uint32_t n, const rtr_light_params* p,
                                   const rtr_pick_params* pick, const rtr_ris_params* ris, const uint32_t* candidates, const float* targets,
                                   const float* wPick, uint32_t* outSlots, float* outWeights) {
    const char* who = "rtr_host_ris_select";
    if (const int rc = rtrdev::pick_check_params(who, p, pick, false)) return rc;
    if (const int rc = rtrdev::ris_check_params(who, ris)) return rc;
    if (const int rc = rtrdev::power_check_table(who, cdf, tris)) return rc;
    if (const int rc = rtrdev::pick_check_area(who, (uint64_t)tris * p->numShadowRays)) return rc;
    if (n == 0u) return RTR_OK;
    const uint32_t P = pick->numPicks, M = ris->numCandidates, ns = p->numShadowRays;
    const bool mis = (ris->flags & RTR_RIS_MIS) != 0u;
    if (const int rc = rtrdev::ris_check_count(who, n, P, M)) return rc;
    const rtrdev::Arg args[6] = {{candidates, "candidates", 4, true}, {targets, "targets", 4, true}, {wPick, "wPick", 4, mis},
                                 {outSlots, "outSlots", 4, true}, {outWeights, "outWeights", 4, true}, {seeds, "seeds", 4, false}};
    if (const int rc = rtrdev::check_ptrs(who, args)) return rc;
    if (const int rc = rtrdev::check_pixel_seeds(who, seeds, p->width, p->spp)) return rc;
    const uint64_t total = rtr_power_total(cdf, tris);
    const uint64_t area = (uint64_t)tris * ns;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t baseFrame = rtr_pick_base(seeds, k, p->width, p->spp) + p->frame;
        for (uint32_t q = 0; q < P; ++q) {
            rtr_ris_reservoir r;
            rtr_ris_begin(&r);
            for (uint32_t j = 0; j < M; ++j) {
                const size_t at = ((size_t)k * P + q) * M + j;
                const uint32_t slot = candidates[at];
                if (total == 0u || slot >= area) continue;           /* RTR_PICK_NONE, or no slot of this table */
                if (mis && rtr_ris_target(wPick[at]) == 0.0f) continue;      /* the device's target, a product by wPick, is 0 there */
                rtr_ris_step(&r, total, rtr_power_weight_at(cdf, slot / ns), slot, rtr_ris_target(targets[at]), mis ? wPick[at] : 0.0f,
                             rtr_ris_number(baseFrame, pick->depth, q, j));
            }
            outSlots[(size_t)k * P + q] = rtr_ris_finish(&r, M, P, mis ? 1u : 0u, &outWeights[(size_t)k * P + q]);
        }
    }
    return RTR_OK;
}
