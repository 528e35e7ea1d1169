/* rtr_bounce_host.cpp — rtr_host_bounce_rays and the argument checks it shares with rtr_bounce_rays.  Pure host C++ with no HIP in it:
 * include/rtr_bounce.h compiled for the host cores with the kernels' flags (-ffp-contract=off, no fast-math), so that the device's
 * records can be held to these bits; a translation unit of its own so that a stand-alone program (tools/bounce_host_check.cpp) can run
 * it under the host sanitizers. */
#include "rtr_bounce_host.h"
#include "../../include/rtr_bounce.h"

#include <cstdint>

namespace rtrdev {

int bounce_check_args(const char* who, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p,
                      const uint32_t* seeds, const RtrRay* outRays, const RtrBounce* outBounce) {
    if (!p) return refusef("%s: params is null", who);
    const Arg a[5] = {{rays, "rays", 16, true, sizeof(RtrRay) * (size_t)n}, {surfaces, "surfaces", 16, true, sizeof(RtrSurface) * (size_t)n},
                      {outRays, "outRays", 16, true, sizeof(RtrRay) * (size_t)n}, {outBounce, "outBounce", 16, true, sizeof(RtrBounce) * (size_t)n},
                      {seeds, "seeds", 4, false, sizeof(uint32_t) * (size_t)n}};
    if (const int rc = check_ptrs(who, a)) return rc;
    if (const int rc = check_lobes(who, p->lobes)) return rc;
    if (const int rc = check_pixel_seeds(who, seeds, p->width, p->spp)) return rc;
    if (!rtr_bounce_finite(p->normalOffset)) return refusef("%s: normalOffset is not finite", who);
    if (!rtr_bounce_finite(p->tmin)) return refusef("%s: tmin is not finite", who);
    if (!rtr_bounce_finite(p->tmax)) return refusef("%s: tmax is not finite", who);
    if (!(p->tmax > p->tmin)) return refusef("%s: tmax %g is not above tmin %g", who, (double)p->tmax, (double)p->tmin);
    const Arg in[3] = {a[0], a[1], a[4]};
    return check_overlaps(who, in, 3, a + 2, 2);
}

}  // namespace rtrdev

extern "C" int rtr_host_sincos_turn(const float* u, uint32_t n, float* outSin, float* outCos) {
    if (n == 0) return RTR_OK;
    const rtrdev::Arg a[3] = {{u, "u", 1, true}, {outSin, "outSin", 1, true}, {outCos, "outCos", 1, true}};
    if (const int rc = rtrdev::check_ptrs("rtr_host_sincos_turn", a)) return rc;
    for (uint32_t k = 0; k < n; ++k) rtr_sincos_turn(u[k], &outSin[k], &outCos[k]);
    return RTR_OK;
}

extern "C" int rtr_host_bounce_rays(const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p, const uint32_t* seeds,
                                    RtrRay* outRays, RtrBounce* outBounce) {
    if (n == 0) return RTR_OK;
    if (const int rc = rtrdev::bounce_check_args("rtr_host_bounce_rays", rays, surfaces, n, p, seeds, outRays, outBounce)) return rc;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t base = seeds ? seeds[k] : rtr_bounce_pixel_seed(k, p->width, p->spp);
        rtr_bounce_sample(&rays[k], &surfaces[k], base, p, &outRays[k], &outBounce[k]);
    }
    return RTR_OK;
}
