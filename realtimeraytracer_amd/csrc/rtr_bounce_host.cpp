/* rtr_bounce_host.cpp — rtr_host_bounce_rays and the argument checks it shares with rtr_bounce_rays.  Pure host C++ with no HIP in it:
 * include/rtr_bounce.h compiled for the host cores with the kernels' flags (-ffp-contract=off, no fast-math), so that the device's
 * records can be held to these bits; a translation unit of its own so that a stand-alone program (tools/bounce_host_check.cpp) can run
 * it under the host sanitizers. */
#include "rtr_bounce_host.h"
#include "../../include/rtr_bounce.h"

#include <cstdint>
#include <cstdio>

namespace rtrdev {

static bool overlaps(const void* a, size_t aBytes, const void* b, size_t bBytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bBytes && b0 < a0 + aBytes;
}

bool bounce_check_args(const char* who, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p,
                       const uint32_t* seeds, const RtrRay* outRays, const RtrBounce* outBounce, char* msg, size_t msgBytes) {
    if (!p) { snprintf(msg, msgBytes, "%s: params is null", who); return false; }
    const struct { const void* ptr; const char* name; size_t stride; bool out; } arr[4] = {
        {rays, "rays", sizeof(RtrRay), false}, {surfaces, "surfaces", sizeof(RtrSurface), false},
        {outRays, "outRays", sizeof(RtrRay), true}, {outBounce, "outBounce", sizeof(RtrBounce), true}};
    for (const auto& a : arr)
        if (!a.ptr) { snprintf(msg, msgBytes, "%s: %s is null", who, a.name); return false; }
    for (const auto& a : arr)
        if ((uintptr_t)a.ptr & 15u) { snprintf(msg, msgBytes, "%s: %s is not 16-B aligned", who, a.name); return false; }
    if (seeds && ((uintptr_t)seeds & 3u)) { snprintf(msg, msgBytes, "%s: seeds is not 4-B aligned", who); return false; }
    if (p->lobes == 0u || (p->lobes & ~(RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR))) {
        snprintf(msg, msgBytes, "%s: lobes 0x%x (RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR, at least one)", who, p->lobes);
        return false;
    }
    if (!seeds && (p->width == 0u || p->spp == 0u)) {
        snprintf(msg, msgBytes, "%s: width %u, spp %u: without seeds the hits are pixel-samples of a frame", who, p->width, p->spp);
        return false;
    }
    if (!rtr_bounce_finite(p->normalOffset)) { snprintf(msg, msgBytes, "%s: normalOffset is not finite", who); return false; }
    if (!rtr_bounce_finite(p->tmin)) { snprintf(msg, msgBytes, "%s: tmin is not finite", who); return false; }
    if (!rtr_bounce_finite(p->tmax)) { snprintf(msg, msgBytes, "%s: tmax is not finite", who); return false; }
    if (!(p->tmax > p->tmin)) { snprintf(msg, msgBytes, "%s: tmax %g is not above tmin %g", who, (double)p->tmax, (double)p->tmin); return false; }
    for (int o = 2; o < 4; ++o) {
        for (int i = 0; i < 2; ++i)
            if (overlaps(arr[o].ptr, arr[o].stride * n, arr[i].ptr, arr[i].stride * n)) {
                snprintf(msg, msgBytes, "%s: %s overlaps %s", who, arr[o].name, arr[i].name);
                return false;
            }
        if (seeds && overlaps(arr[o].ptr, arr[o].stride * n, seeds, sizeof(uint32_t) * (size_t)n)) {
            snprintf(msg, msgBytes, "%s: %s overlaps seeds", who, arr[o].name);
            return false;
        }
    }
    if (overlaps(outRays, sizeof(RtrRay) * (size_t)n, outBounce, sizeof(RtrBounce) * (size_t)n)) {
        snprintf(msg, msgBytes, "%s: outRays overlaps outBounce", who);
        return false;
    }
    return true;
}

}  // namespace rtrdev

extern "C" int rtr_host_sincos_turn(const float* u, uint32_t n, float* outSin, float* outCos) {
    if (n == 0) return RTR_OK;
    if (!u || !outSin || !outCos) {
        rtrdev::set_last_error(!u ? "rtr_host_sincos_turn: u is null" : (!outSin ? "rtr_host_sincos_turn: outSin is null" : "rtr_host_sincos_turn: outCos is null"));
        return RTR_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t k = 0; k < n; ++k) rtr_sincos_turn(u[k], &outSin[k], &outCos[k]);
    return RTR_OK;
}

extern "C" int rtr_host_bounce_rays(const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p, const uint32_t* seeds,
                                    RtrRay* outRays, RtrBounce* outBounce) {
    if (n == 0) return RTR_OK;
    char msg[256];
    if (!rtrdev::bounce_check_args("rtr_host_bounce_rays", rays, surfaces, n, p, seeds, outRays, outBounce, msg, sizeof msg)) {
        rtrdev::set_last_error(msg);
        return RTR_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t base = seeds ? seeds[k] : rtr_bounce_pixel_seed(k, p->width, p->spp);
        rtr_bounce_sample(&rays[k], &surfaces[k], base, p, &outRays[k], &outBounce[k]);
    }
    return RTR_OK;
}
