/* rtr_bounce_host.h — what rtr_bounce_rays' device and host entry points share (internal to librtr_hip.so). */
#pragma once
#include "rtr_arg_check.h"

namespace rtrdev {

/* The argument checks of rtr_bounce_rays[_async] and rtr_host_bounce_rays, which need no device (as rtr_arg_check.h returns them).  Not
 * called for numHits == 0. */
int bounce_check_args(const char* who, const RtrRay* rays, const RtrSurface* surfaces, uint32_t numHits, const rtr_bounce_params* params,
                      const uint32_t* seeds, const RtrRay* outRays, const RtrBounce* outBounce);

}  // namespace rtrdev
