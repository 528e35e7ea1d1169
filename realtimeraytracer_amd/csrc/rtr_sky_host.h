/* rtr_sky_host.h — what rtr_sky_rays / rtr_shade_sky / rtr_sky_hits and the rtr_host_* forms of include/rtr_sky.h share (internal to
 * librtr_hip.so). */
#pragma once
#include "rtr_arg_check.h"

namespace rtrdev {

/* The checks that need no handle (as rtr_arg_check.h returns them).  The params are checked for every n, the arrays for n > 0.
 * zeroSamples: numSamples == 0 is allowed (rtr_sky_hits: a vertex that drew no sky sample) */
int sky_check_params(const char* who, const rtr_sky_params* p, bool zeroSamples);
/* rtr_sky_rays and rtr_host_sky_rays: the arrays (seeds may be null), the pixel rule, numHits x S in 32 bits, the overlaps */
int sky_check_rays_call(const char* who, const rtr_sky_params* p, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const uint32_t* seeds,
                        const RtrRay* outRays, const RtrSkySample* outSamples);
/* rtr_shade_sky */
int sky_check_shade_call(const char* who, const RtrSkySample* samples, const uint8_t* occluded, uint32_t n, uint32_t numSamples, const float* out);
/* rtr_sky_hits and rtr_host_sky_hits: every array is needed and 16-B aligned */
int sky_check_hits_arrays(const char* who, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces, uint32_t n,
                          const RtrSkyEscape* out);
/* an HDRI (null: the constant sky) a table can be made of */
int sky_check_texture(const char* who, const rtr_texture* hdri);

}  // namespace rtrdev
