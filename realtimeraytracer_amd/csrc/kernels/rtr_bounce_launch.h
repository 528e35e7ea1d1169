/* rtr_bounce_launch.h — host-callable launcher of the continuation-ray kernel (kernels/rtr_bounce.hip; internal to librtr_hip.so). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/rtr_types.h"

namespace rtrdev {

struct BounceArgs {
    const float4* rays;          /* RtrRay as 2 x float4: {origin, tmin} {direction, tmax} */
    const float4* surfaces;      /* RtrSurface as 5 x float4 */
    const uint32_t* seeds;       /* per hit: the base of its seeds, or null (then the pixel's: px * 733 + py * 1933) */
    float4* outRays;             /* RtrRay as 2 x float4 */
    float4* outBounce;           /* RtrBounce as 2 x float4 */
    rtr_bounce_params params;
    uint32_t n;
};

/* one next ray and one RtrBounce per hit: rtr_bounce_sample (include/rtr_bounce.h) */
hipError_t launch_bounce_rays(const BounceArgs& a, hipStream_t stream);

}  // namespace rtrdev
