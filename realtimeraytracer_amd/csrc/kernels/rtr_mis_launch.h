/* rtr_mis_launch.h — host-callable launcher of the emitter-hit kernel (kernels/rtr_mis.hip; internal to librtr_hip.so). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/rtr_types.h"

namespace rtrdev {

struct EmitterArgs {
    const float4* rays;              /* the bounce rays: RtrRay as 2 x float4 */
    const float4* hits;              /* their closest hits: RtrHit as 2 x float4 */
    const float4* prevSurfaces;      /* RtrSurface of the vertex each ray left, 5 x float4 (the first two pieces are read) */
    const float4* bounces;           /* that vertex's RtrBounce, 2 x float4 (pdf is read) */
    float4* out;                     /* RtrEmitter as 2 x float4 */
    const float4* lightTris;         /* DeviceScene::lightTris: 4 x float4 per light triangle */
    const uint32_t* lightTriFirst;   /* DeviceScene::lightTriFirst */
    const RtrAreaLightInfo* lights;
    uint32_t numLights;
    uint32_t numAreaLights;          /* the lights the picks can reach */
    uint32_t tris;                   /* Ttot: their triangles */
    uint32_t picks;                  /* P */
    uint32_t n;
    const uint64_t* cdf;             /* null: the uniform rule; else the scene's power table (include/rtr_power.h) */
};

/* one RtrEmitter per ray: rtr_mis_emitter (include/rtr_mis.h) where the hit is a triangle of a light, zeros elsewhere; with a.cdf rtr_power_mis_emitter
 * (include/rtr_power.h) */
hipError_t launch_emitter_hits(const EmitterArgs& a, hipStream_t stream);

}  // namespace rtrdev
