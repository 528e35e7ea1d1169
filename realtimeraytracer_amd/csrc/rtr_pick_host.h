/* rtr_pick_host.h — what rtr_light_rays_picked / rtr_shade_hits_picked and rtr_host_pick_slots share (internal to librtr_hip.so). */
#pragma once
#include <stddef.h>
#include "../../include/rtr.h"

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

/* The checks that need no handle: true when the call may go on, else the refusal's message (it names `who` and the argument) in msg and
 * its status in rc.  The params are checked for every n, the arrays for n > 0. */
bool pick_check_params(const char* who, const rtr_light_params* light, const rtr_pick_params* pick, bool shade, char* msg, size_t msgBytes, int* rc);
bool pick_check_arrays(const char* who, const PickCall& c, char* msg, size_t msgBytes);
/* A <= RTR_PICK_MAX_SLOTS */
bool pick_check_area(const char* who, uint64_t areaSlots, char* msg, size_t msgBytes);

/* rtr_last_error's text for this thread; defined by rtr_api.cpp (a stand-alone program around rtr_pick_host.cpp brings its own) */
void set_last_error(const char* msg);

}  // namespace rtrdev
