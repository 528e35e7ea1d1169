/* rtr_ris_host.h — what rtr_pick_slots_ris and the rtr_host_* forms of include/rtr_ris.h share (internal to librtr_hip.so). */
#pragma once
#include "rtr_arg_check.h"

namespace rtrdev {

/* the rtr_ris_params alone: not null, numCandidates 1 ... RTR_RIS_MAX_CANDIDATES, known flags, lobes as the flag wants them, _reserved 0 */
int ris_check_params(const char* who, const rtr_ris_params* ris);
/* 1 ... RTR_RIS_MAX_CANDIDATES */
int ris_check_candidates(const char* who, uint32_t numCandidates);
/* numHits x P x M fits 32 bits (behind pick_check_params: P is in range) */
int ris_check_count(const char* who, uint32_t n, uint32_t picks, uint32_t candidates);

/* every array of one rtr_pick_slots_ris call */
struct RisCall {
    const RtrRay* rays; const RtrHit* hits; uint32_t n;
    const rtr_light_params* light; const rtr_pick_params* pick; const rtr_ris_params* ris; const uint32_t* seeds;
    const uint32_t* outSlots; const float* outWeights; const uint32_t* outCandidates; const float* outTargets;
};
/* behind pick_check_params and ris_check_params: outCandidates and outTargets come together (for every n); for n > 0 the count, the
 * pointers, the pixel rule's width and spp, and no output over an input or another output */
int ris_check_call(const char* who, const RisCall& c);

}  // namespace rtrdev
