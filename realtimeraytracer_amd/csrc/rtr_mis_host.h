/* rtr_mis_host.h — what rtr_mis_pick_weights / rtr_emitter_hits and the rtr_host_* forms of include/rtr_mis.h share (internal to
 * librtr_hip.so). */
#pragma once
#include <stddef.h>
#include "../../include/rtr.h"

namespace rtrdev {

/* The checks that need no handle: true when the call may go on, else the refusal's message (it names `who` and the argument) in msg.
 * The params are checked for every n, the arrays for n > 0. */
bool mis_check_params(const char* who, const rtr_mis_params* mis, char* msg, size_t msgBytes);
/* rtr_mis_pick_weights: the mis params against the light and pick params they must repeat, then the arrays (seeds, slots, outSamples may
 * be null) */
bool mis_check_pick_call(const char* who, const rtr_light_params* light, const rtr_pick_params* pick, const rtr_mis_params* mis, const RtrRay* rays,
                         const RtrHit* hits, uint32_t n, const uint32_t* seeds, const uint32_t* slots, const float* outWeights,
                         const RtrMisSample* outSamples, char* msg, size_t msgBytes);
/* rtr_emitter_hits and rtr_host_emitter_hits: every array is needed and 16-B aligned */
bool mis_check_emitter_arrays(const char* who, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                              const RtrEmitter* out, char* msg, size_t msgBytes);

/* rtr_last_error's text for this thread; defined by rtr_api.cpp (a stand-alone program around rtr_mis_host.cpp brings its own) */
void set_last_error(const char* msg);

}  // namespace rtrdev
