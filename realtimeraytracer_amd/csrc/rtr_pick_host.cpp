/* rtr_pick_host.cpp — rtr_host_pick_slots and the argument checks rtr_light_rays_picked / rtr_shade_hits_picked share with it.
 * Pure host C++ with no HIP in it: include/rtr_pick.h compiled for the host cores with the kernels' flags (-ffp-contract=off, no
 * fast-math), so that the device's slots can be held to these words; a translation unit of its own so that a stand-alone program
 * (tools/pick_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_pick_host.h"
#include "../../include/rtr_pick.h"

#include <cstdint>

namespace rtrdev {

static int pick_params_ok(const char* who, const rtr_pick_params* pick) {
    if (!pick) return refusef("%s: pick params is null", who);
    if (const int rc = check_num_picks(who, pick->numPicks)) return rc;
    return check_reserved(who, pick->_reserved, 6, "pick params");
}

int pick_check_params(const char* who, const rtr_light_params* p, const rtr_pick_params* pick, bool shade) {
    if (!p) return refusef("%s: params is null", who);
    if (const int rc = pick_params_ok(who, pick)) return rc;
    /* what rtr_light_slots refuses of the params alone; numAreaLights is held to the scene's lights once there is a scene */
    if (const int rc = check_shadow_rays(who, p->numShadowRays)) return rc;
    if (const int rc = check_light_outputs(who, p->outputs)) return rc;
    if (shade && (p->outputs & RTR_LIGHT_ANALYTIC)) {
        refusef("%s: RTR_LIGHT_ANALYTIC has no per-sample form (the LTC term integrates whole lights): use rtr_shade_hits", who);
        return RTR_ERR_UNSUPPORTED;
    }
    return RTR_OK;
}

int pick_check_arrays(const char* who, const PickCall& c) {
    if (const int rc = check_fits_32(who, c.n, "hits", c.pick->numPicks + 1u, "slots")) return rc;
    const Arg light[6] = {{c.rays, "rays", 16, true}, {c.hits, "hits", 16, true}, {c.seeds, "seeds", 4, false}, {c.slots, "slotsIn", 4, false},
                          {c.outRays, "outRays", 16, true}, {c.outSlots, "outSlots", 4, true}};
    const Arg shade[7] = {{c.rays, "rays", 16, true}, {c.hits, "hits", 16, true}, {c.seeds, "seeds", 4, false}, {c.slots, "slots", 4, true},
                          {c.weights, "weights", 4, false}, {c.occluded, "occluded", 1, true}, {c.out, "out", 16, true}};
    if (const int rc = c.shade ? check_ptrs(who, shade) : check_ptrs(who, light)) return rc;
    return check_pixel_seeds(who, c.seeds, c.light->width, c.light->spp);
}

int pick_check_area(const char* who, uint64_t areaSlots) {
    if (areaSlots > RTR_PICK_MAX_SLOTS)
        return refusef("%s: %llu area slots per hit are more than RTR_PICK_MAX_SLOTS = 2^24", who, (unsigned long long)areaSlots);
    return RTR_OK;
}

}  // namespace rtrdev

extern "C" int rtr_host_pick_slots(const uint32_t* seeds, uint32_t n, uint32_t frame, uint32_t width, uint32_t spp, const rtr_pick_params* pick,
                                   uint32_t areaSlots, uint32_t* outSlots) {
    const char* who = "rtr_host_pick_slots";
    if (const int rc = rtrdev::pick_params_ok(who, pick)) return rc;
    if (const int rc = rtrdev::pick_check_area(who, areaSlots)) return rc;
    if (n == 0) return RTR_OK;
    const uint32_t P = pick->numPicks;
    if (const int rc = rtrdev::check_fits_32(who, n, "hits", P, "picks")) return rc;
    const rtrdev::Arg a[2] = {{outSlots, "outSlots", 4, true}, {seeds, "seeds", 4, false}};
    if (const int rc = rtrdev::check_ptrs(who, a)) return rc;
    if (const int rc = rtrdev::check_pixel_seeds(who, seeds, width, spp)) return rc;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t baseFrame = rtr_pick_base(seeds, k, width, spp) + frame;
        for (uint32_t p = 0; p < P; ++p) outSlots[(size_t)k * P + p] = rtr_pick_slot(baseFrame, pick->depth, p, areaSlots);
    }
    return RTR_OK;
}
