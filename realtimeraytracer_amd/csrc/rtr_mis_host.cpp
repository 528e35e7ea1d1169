/* rtr_mis_host.cpp — rtr_host_bounce_pdf, rtr_host_mis_weights, rtr_host_emitter_hits and the argument checks rtr_mis_pick_weights /
 * rtr_emitter_hits share with them.  Pure host C++ with no HIP in it: include/rtr_mis.h compiled for the host cores with the kernels'
 * flags (-ffp-contract=off, no fast-math), so that the device's records can be held to these bits; a translation unit of its own so
 * that a stand-alone program (tools/mis_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_mis_host.h"
#include "../../include/rtr_mis.h"

#include <cstdint>
#include <cstdio>

namespace rtrdev {

bool mis_check_params(const char* who, const rtr_mis_params* mis, char* msg, size_t msgBytes) {
    if (!mis) { snprintf(msg, msgBytes, "%s: mis params is null", who); return false; }
    if (mis->numPicks == 0u || mis->numPicks > RTR_PICK_MAX) {
        snprintf(msg, msgBytes, "%s: numPicks %u (1 ... %u)", who, mis->numPicks, RTR_PICK_MAX);
        return false;
    }
    if (mis->numShadowRays == 0u || mis->numShadowRays > 1024u) {
        snprintf(msg, msgBytes, "%s: numShadowRays %u (1 ... 1024)", who, mis->numShadowRays);
        return false;
    }
    if (mis->lobes == 0u || (mis->lobes & ~(RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR))) {
        snprintf(msg, msgBytes, "%s: lobes 0x%x (RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR, at least one)", who, mis->lobes);
        return false;
    }
    if (mis->_reserved[0] | mis->_reserved[1] | mis->_reserved[2] | mis->_reserved[3]) {
        snprintf(msg, msgBytes, "%s: _reserved words of mis params are not 0", who);
        return false;
    }
    return true;
}

struct MisArg { const void* ptr; const char* name; unsigned align; bool needed; };

static bool check_ptrs(const char* who, const MisArg* args, int count, char* msg, size_t msgBytes) {
    for (int i = 0; i < count; ++i)
        if (args[i].needed && !args[i].ptr) { snprintf(msg, msgBytes, "%s: %s is null", who, args[i].name); return false; }
    for (int i = 0; i < count; ++i)
        if (args[i].ptr && ((uintptr_t)args[i].ptr & (args[i].align - 1u))) {
            snprintf(msg, msgBytes, "%s: %s is not %u-B aligned", who, args[i].name, args[i].align);
            return false;
        }
    return true;
}

bool mis_check_pick_call(const char* who, const rtr_light_params* light, const rtr_pick_params* pick, const rtr_mis_params* mis, const RtrRay* rays,
                         const RtrHit* hits, uint32_t n, const uint32_t* seeds, const uint32_t* slots, const float* outWeights,
                         const RtrMisSample* outSamples, char* msg, size_t msgBytes) {
    if (mis->numPicks != pick->numPicks) {
        snprintf(msg, msgBytes, "%s: numPicks %u of the mis params is not the pick params' %u", who, mis->numPicks, pick->numPicks);
        return false;
    }
    if (mis->numAreaLights != light->numAreaLights || mis->numShadowRays != light->numShadowRays) {
        snprintf(msg, msgBytes, "%s: numAreaLights %u, numShadowRays %u of the mis params are not the light params' %u, %u", who, mis->numAreaLights,
                 mis->numShadowRays, light->numAreaLights, light->numShadowRays);
        return false;
    }
    if (n == 0u) return true;
    if ((uint64_t)n * mis->numPicks > 0xffffffffull) { snprintf(msg, msgBytes, "%s: %u hits x %u picks do not fit 32 bits", who, n, mis->numPicks); return false; }
    const MisArg args[6] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, {seeds, "seeds", 4, false}, {slots, "slots", 4, false},
                            {outWeights, "outWeights", 4, true}, {outSamples, "outSamples", 16, false}};
    if (!check_ptrs(who, args, 6, msg, msgBytes)) return false;
    if (!seeds && (light->width == 0u || light->spp == 0u)) {
        snprintf(msg, msgBytes, "%s: width %u, spp %u: without seeds the hits are pixel-samples of a frame", who, light->width, light->spp);
        return false;
    }
    return true;
}

bool mis_check_emitter_arrays(const char* who, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                              const RtrEmitter* out, char* msg, size_t msgBytes) {
    const MisArg args[5] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, {prevSurfaces, "prevSurfaces", 16, true}, {bounces, "bounces", 16, true},
                            {out, "out", 16, true}};
    return check_ptrs(who, args, 5, msg, msgBytes);
}

static int refuse(const char* msg) {
    set_last_error(msg);
    return RTR_ERR_INVALID_ARGUMENT;
}

}  // namespace rtrdev

extern "C" int rtr_host_bounce_pdf(const RtrRay* rays, const RtrSurface* surfaces, const float* dirs, uint32_t n, uint32_t lobes, float* outPdf) {
    const char* who = "rtr_host_bounce_pdf";
    char msg[256];
    if (lobes == 0u || (lobes & ~(RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR))) {
        snprintf(msg, sizeof msg, "%s: lobes 0x%x (RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR, at least one)", who, lobes);
        return rtrdev::refuse(msg);
    }
    if (n == 0) return RTR_OK;
    const rtrdev::MisArg args[4] = {{rays, "rays", 4, true}, {surfaces, "surfaces", 4, true}, {dirs, "dirs", 4, true}, {outPdf, "outPdf", 4, true}};
    if (!rtrdev::check_ptrs(who, args, 4, msg, sizeof msg)) return rtrdev::refuse(msg);
    for (uint32_t k = 0; k < n; ++k) outPdf[k] = rtr_mis_bounce_pdf(&rays[k], &surfaces[k], rtr_ld3(dirs + 3 * (size_t)k), lobes);
    return RTR_OK;
}

extern "C" int rtr_host_mis_weights(uint32_t n, const float* pb, const float* dist, const float* cosLight, const float* area, uint32_t Ttot, uint32_t P,
                                    RtrMisSample* outSamples, float* outWBounce) {
    const char* who = "rtr_host_mis_weights";
    char msg[256];
    if (P > RTR_PICK_MAX) { snprintf(msg, sizeof msg, "%s: P %u (0 ... %u)", who, P, RTR_PICK_MAX); return rtrdev::refuse(msg); }
    if (Ttot > RTR_PICK_MAX_SLOTS) { snprintf(msg, sizeof msg, "%s: Ttot %u is more than RTR_PICK_MAX_SLOTS = 2^24", who, Ttot); return rtrdev::refuse(msg); }
    if (n == 0) return RTR_OK;
    const rtrdev::MisArg args[6] = {{pb, "pb", 4, true}, {dist, "dist", 4, true}, {cosLight, "cosLight", 4, true}, {area, "area", 4, true},
                                    {outSamples, "outSamples", 4, true}, {outWBounce, "outWBounce", 4, false}};
    if (!rtrdev::check_ptrs(who, args, 6, msg, sizeof msg)) return rtrdev::refuse(msg);
    for (uint32_t k = 0; k < n; ++k) {
        RtrMisSample* o = &outSamples[k];
        float wBounce;
        rtr_mis_weights(pb[k], dist[k], cosLight[k], area[k], Ttot, P, &o->lightPdf, &o->wPick, &wBounce);
        o->bouncePdf = pb[k]; o->cosLight = cosLight[k]; o->dist = dist[k]; o->area = area[k]; o->lightTri = 0u; o->_r = 0u;
        if (outWBounce) outWBounce[k] = wBounce;
    }
    return RTR_OK;
}

extern "C" int rtr_host_emitter_hits(const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces, uint32_t n,
                                     const float* lightTris, const uint32_t* lightTriFirst, const RtrAreaLightInfo* lights, uint32_t numLights,
                                     const rtr_mis_params* mis, RtrEmitter* out) {
    const char* who = "rtr_host_emitter_hits";
    char msg[256];
    if (!rtrdev::mis_check_params(who, mis, msg, sizeof msg)) return rtrdev::refuse(msg);
    if (mis->numAreaLights > numLights) {
        snprintf(msg, sizeof msg, "%s: numAreaLights %u > lights %u", who, mis->numAreaLights, numLights);
        return rtrdev::refuse(msg);
    }
    if (numLights && (!lightTris || !lightTriFirst || !lights)) {
        snprintf(msg, sizeof msg, "%s: %s is null", who, !lightTris ? "lightTris" : (!lightTriFirst ? "lightTriFirst" : "lights"));
        return rtrdev::refuse(msg);
    }
    if (n == 0) return RTR_OK;
    if (!rtrdev::mis_check_emitter_arrays(who, rays, hits, prevSurfaces, bounces, out, msg, sizeof msg)) return rtrdev::refuse(msg);
    uint64_t tris = 0;
    for (uint32_t l = 0; l < mis->numAreaLights; ++l) tris += lights[l].numTriangles;
    if (tris > RTR_PICK_MAX_SLOTS) { snprintf(msg, sizeof msg, "%s: %llu light triangles are more than 2^24", who, (unsigned long long)tris); return rtrdev::refuse(msg); }
    for (uint32_t k = 0; k < n; ++k) {
        rtr_mis_emitter_zero(&out[k]);
        const uint32_t l = hits[k].customIndex, prim = hits[k].primitiveId;
        if (l >= numLights || prim >= lights[l].numTriangles) continue;       /* a miss (0xffffffff), an object, ids out of range */
        const uint32_t t = lightTriFirst[l] + prim;
        rtr_mis_emitter(&rays[k], hits[k].t, &prevSurfaces[k], &bounces[k], lightTris + 16 * (size_t)t, t, lights[l].color, lights[l].intensity,
                        lights[l].isTwoSided, l < mis->numAreaLights, (uint32_t)tris, mis->numPicks, &out[k]);
    }
    return RTR_OK;
}
