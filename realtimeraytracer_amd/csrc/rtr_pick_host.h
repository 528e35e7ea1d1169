/* rtr_pick_host.h — what rtr_light_rays_picked / rtr_shade_hits_picked and rtr_host_pick_slots share (internal to librtr_hip.so). */
#pragma once
#include "rtr_arg_check.h"

namespace rtrdev {

/* every array of one picked call; shade: rtr_shade_hits_picked (slots, weights, occluded, out), else rtr_light_rays_picked (slotsIn,
 * outRays, outSlots) */
struct PickCall {
    const RtrRay* rays; const RtrHit* hits; uint32_t n;
    const rtr_light_params* light; const rtr_pick_params* pick; const uint32_t* seeds;
    bool shade;
    const uint32_t* slots;       /* slotsIn (may be null), or the shade call's slots (needed) */
    const RtrRay* outRays; const uint32_t* outSlots;
    const float* weights; const uint8_t* occluded; const RtrRadiance* out;
};

/* The checks that need no handle (as rtr_arg_check.h returns them; RTR_ERR_UNSUPPORTED for the analytic sum of a shade call).  The
 * params are checked for every n, the arrays for n > 0. */
int pick_check_params(const char* who, const rtr_light_params* light, const rtr_pick_params* pick, bool shade);
int pick_check_arrays(const char* who, const PickCall& c);
/* A <= RTR_PICK_MAX_SLOTS */
int pick_check_area(const char* who, uint64_t areaSlots);

}  // namespace rtrdev
