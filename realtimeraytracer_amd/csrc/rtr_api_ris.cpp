/* rtr_api_ris.cpp — rtr_pick_slots_ris of the C ABI (include/rtr.h; the rule is include/rtr_ris.h, the kernel k_pick_slots_ris of
 * kernels/rtr_query.hip, the host forms and the argument checks rtr_ris_host.cpp).  It takes the scene's light-power table from
 * rtr_api_power.cpp and the picked calls' scene checks and launch arguments from rtr_api_paths.cpp. */
#include "../../include/rtr.h"
#include "kernels/rtr_query.h"
#include "rtr_pick_host.h"
#include "rtr_ris_host.h"
#include "rtr_api_internal.h"

#include <hip/hip_runtime.h>

using namespace rtrapi;

static int enqueue_pick_slots_ris(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                  const rtr_pick_params* pick, const rtr_ris_params* ris, const uint32_t* seeds, uint32_t* outSlots, float* outWeights,
                                  uint32_t* outCandidates, float* outTargets, const char* who) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::pick_check_params(who, p, pick, true)) return rc;
    if (const int rc = rtrdev::ris_check_params(who, ris)) return rc;
    const rtrdev::RisCall call{rays, hits, n, p, pick, ris, seeds, outSlots, outWeights, outCandidates, outTargets};
    if (const int rc = rtrdev::ris_check_call(who, call)) return rc;
    uint32_t areaSlots = 0, tris = 0;
    if (const int rc = picked_scene_checks(c, s, p, who, &areaSlots, &tris)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = ensure_light_power(s, c->stream, who)) return rc;
    rtrdev::RisArgs a{};
    fill_pick_args(a.ma.pa, s, rays, hits, n, p, pick, seeds, nullptr, areaSlots, tris);
    a.ma.pa.outSlots = outSlots; a.ma.outWeights = outWeights; a.ma.lobes = ris->lobes; a.ma.tris = tris; a.ma.cdf = s->powerCdf.p;
    a.candidates = ris->numCandidates; a.mis = ris->flags & RTR_RIS_MIS; a.outCandidates = outCandidates; a.outTargets = outTargets;
    return launched(rtrdev::launch_pick_slots_ris(s->dev, a, c->stream), who);
}

extern "C" {

int rtr_pick_slots_ris_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                             const rtr_pick_params* pick, const rtr_ris_params* ris, const uint32_t* seeds, uint32_t* outSlots, float* outWeights,
                             uint32_t* outCandidates, float* outTargets) {
    return enqueue_pick_slots_ris(c, s, rays, hits, n, p, pick, ris, seeds, outSlots, outWeights, outCandidates, outTargets, "rtr_pick_slots_ris_async");
}

int rtr_pick_slots_ris(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                       const rtr_pick_params* pick, const rtr_ris_params* ris, const uint32_t* seeds, uint32_t* outSlots, float* outWeights,
                       uint32_t* outCandidates, float* outTargets) {
    return join_if_enqueued(c, enqueue_pick_slots_ris(c, s, rays, hits, n, p, pick, ris, seeds, outSlots, outWeights, outCandidates, outTargets,
                                                      "rtr_pick_slots_ris"), n);
}

}  // extern "C"
