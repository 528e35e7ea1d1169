/* rtr_mis_host.h — what rtr_mis_pick_weights / rtr_emitter_hits and the rtr_host_* forms of include/rtr_mis.h share (internal to
 * librtr_hip.so). */
#pragma once
#include "rtr_arg_check.h"

namespace rtrdev {

/* The checks that need no handle (as rtr_arg_check.h returns them).  The params are checked for every n, the arrays for n > 0. */
int mis_check_params(const char* who, const rtr_mis_params* mis);
/* rtr_mis_pick_weights: the mis params against the light and pick params they must repeat, then the arrays (seeds, slots, outSamples may
 * be null) */
int mis_check_pick_call(const char* who, const rtr_light_params* light, const rtr_pick_params* pick, const rtr_mis_params* mis, const RtrRay* rays,
                        const RtrHit* hits, uint32_t n, const uint32_t* seeds, const uint32_t* slots, const float* outWeights,
                        const RtrMisSample* outSamples);
/* rtr_emitter_hits and rtr_host_emitter_hits: every array is needed and 16-B aligned */
int mis_check_emitter_arrays(const char* who, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                             const RtrEmitter* out);

}  // namespace rtrdev
