/* rtr_bounce_host.h — what rtr_bounce_rays' device and host entry points share (internal to librtr_hip.so). */
#pragma once
#include <stddef.h>
#include "../../include/rtr.h"

namespace rtrdev {

/* The argument checks of rtr_bounce_rays[_async] and rtr_host_bounce_rays, which need no device: true when the call may go on, else
 * the refusal's message (it names `who` and the argument) in msg.  Not called for numHits == 0. */
bool bounce_check_args(const char* who, const RtrRay* rays, const RtrSurface* surfaces, uint32_t numHits, const rtr_bounce_params* params,
                       const uint32_t* seeds, const RtrRay* outRays, const RtrBounce* outBounce, char* msg, size_t msgBytes);

/* rtr_last_error's text for this thread; defined by rtr_api.cpp (a stand-alone program around rtr_bounce_host.cpp brings its own) */
void set_last_error(const char* msg);

}  // namespace rtrdev
