/* rtr_sky_launch.h — host-callable launchers of the sky kernels (kernels/rtr_sky.hip; internal to librtr_hip.so). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/rtr_sky.h"

namespace rtrdev {

/* the marginal sums of a table up to this many rows are staged in LDS by k_sky_rays (8 B per row: 32 KiB); a taller table is searched
 * in global memory.  -DRTR_SKY_LDS_ROWS=0 is the build-time variant that always searches global memory (`make sky_global_variant`,
 * profiles/sky_rate.py --lib: the measurement behind DESIGN.md section 3) */
#ifndef RTR_SKY_LDS_ROWS
#define RTR_SKY_LDS_ROWS 4096
#endif
constexpr uint32_t kSkyLdsRows = RTR_SKY_LDS_ROWS;

/* the scene's sky on the device: sky.pixels, table.rows and table.marginal are DEVICE pointers */
struct SkyDevice {
    rtr_sky_source sky;
    rtr_sky_table table;
};

struct SkyRaysArgs {
    SkyDevice sd;
    const float4* rays;              /* the rays that found the hits: RtrRay as 2 x float4 */
    const float4* surfaces;          /* RtrSurface as 5 x float4 */
    const uint32_t* seeds;           /* or null: the pixel rule */
    float4* outRays;                 /* n x S rays */
    float4* outSamples;              /* n x S RtrSkySample as 2 x float4 */
    rtr_sky_params params;
    uint32_t n;
};

struct SkyShadeArgs {
    const float4* samples;           /* n x S RtrSkySample (the first piece of each is read) */
    const uint8_t* occluded;         /* n x S bytes */
    float4* out;                     /* n x {sum, 0} */
    uint32_t numSamples;
    uint32_t n;
};

struct SkyHitsArgs {
    SkyDevice sd;
    const float4* rays;              /* the bounce rays */
    const float4* hits;              /* their closest hits: RtrHit as 2 x float4 */
    const float4* prevSurfaces;      /* RtrSurface of the vertex each ray left (the first piece is read, at a miss) */
    const float4* bounces;           /* that vertex's RtrBounce (pdf is read, at a miss) */
    float4* out;                     /* RtrSkyEscape as 2 x float4 */
    uint32_t numSamples, flags;
    uint32_t n;
};

/* the three launches of the table build: the cell weights into rows, each row's inclusive scan in place, the 64-bit scan of the row totals */
hipError_t launch_sky_table(const rtr_sky_source& sky, uint32_t* rows, uint64_t* marginal, hipStream_t stream);
/* ldsMarginal: stage the marginal sums in LDS (height <= kSkyLdsRows) */
hipError_t launch_sky_rays(const SkyRaysArgs& a, bool ldsMarginal, hipStream_t stream);
hipError_t launch_shade_sky(const SkyShadeArgs& a, hipStream_t stream);
hipError_t launch_sky_hits(const SkyHitsArgs& a, hipStream_t stream);

}  // namespace rtrdev
