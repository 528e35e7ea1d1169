/* rtr_power_host.h — what rtr_pick_slots_power and the rtr_host_* forms of include/rtr_power.h share (internal to librtr_hip.so). */
#pragma once
#include "rtr_arg_check.h"

namespace rtrdev {

/* rtr_pick_slots_power and rtr_host_pick_slots_power, behind pick_check_params (rtr_pick_host.h): numHits x P fits 32 bits, outSlots
 * and outWeights are needed and 4-B aligned, seeds may be null — then the hits are pixel-samples of a frame */
int power_check_pick_call(const char* who, const rtr_light_params* light, const rtr_pick_params* pick, uint32_t n, const uint32_t* seeds,
                          const uint32_t* outSlots, const float* outWeights);
/* a table over `tris` triangles: cdf is needed when there are any, 8-B aligned; tris <= RTR_PICK_MAX_SLOTS */
int power_check_table(const char* who, const uint64_t* cdf, uint32_t tris);

}  // namespace rtrdev
