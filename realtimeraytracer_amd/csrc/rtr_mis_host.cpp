/* rtr_mis_host.cpp — rtr_host_bounce_pdf, rtr_host_mis_weights, rtr_host_emitter_hits and the argument checks rtr_mis_pick_weights /
 * rtr_emitter_hits share with them.  Pure host C++ with no HIP in it: include/rtr_mis.h compiled for the host cores with the kernels'
 * flags (-ffp-contract=off, no fast-math), so that the device's records can be held to these bits; a translation unit of its own so
 * that a stand-alone program (tools/mis_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_mis_host.h"
#include "../../include/rtr_mis.h"

#include <cstdint>

namespace rtrdev {

int mis_check_params(const char* who, const rtr_mis_params* mis) {
    if (!mis) return refusef("%s: mis params is null", who);
    if (const int rc = check_num_picks(who, mis->numPicks)) return rc;
    if (const int rc = check_shadow_rays(who, mis->numShadowRays)) return rc;
    if (const int rc = check_lobes(who, mis->lobes)) return rc;
    return check_reserved(who, mis->_reserved, 4, "mis params");
}

int mis_check_pick_call(const char* who, const rtr_light_params* light, const rtr_pick_params* pick, const rtr_mis_params* mis, const RtrRay* rays,
                        const RtrHit* hits, uint32_t n, const uint32_t* seeds, const uint32_t* slots, const float* outWeights,
                        const RtrMisSample* outSamples) {
    if (mis->numPicks != pick->numPicks) return refusef("%s: numPicks %u of the mis params is not the pick params' %u", who, mis->numPicks, pick->numPicks);
    if (mis->numAreaLights != light->numAreaLights || mis->numShadowRays != light->numShadowRays)
        return refusef("%s: numAreaLights %u, numShadowRays %u of the mis params are not the light params' %u, %u", who, mis->numAreaLights,
                       mis->numShadowRays, light->numAreaLights, light->numShadowRays);
    if (n == 0u) return RTR_OK;
    if (const int rc = check_fits_32(who, n, "hits", mis->numPicks, "picks")) return rc;
    const Arg args[6] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, {seeds, "seeds", 4, false}, {slots, "slots", 4, false},
                         {outWeights, "outWeights", 4, true}, {outSamples, "outSamples", 16, false}};
    if (const int rc = check_ptrs(who, args)) return rc;
    return check_pixel_seeds(who, seeds, light->width, light->spp);
}

int mis_check_emitter_arrays(const char* who, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                             const RtrEmitter* out) {
    const Arg args[5] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, {prevSurfaces, "prevSurfaces", 16, true}, {bounces, "bounces", 16, true},
                         {out, "out", 16, true}};
    return check_ptrs(who, args);
}

}  // namespace rtrdev

extern "C" int rtr_host_bounce_pdf(const RtrRay* rays, const RtrSurface* surfaces, const float* dirs, uint32_t n, uint32_t lobes, float* outPdf) {
    const char* who = "rtr_host_bounce_pdf";
    if (const int rc = rtrdev::check_lobes(who, lobes)) return rc;
    if (n == 0) return RTR_OK;
    const rtrdev::Arg args[4] = {{rays, "rays", 4, true}, {surfaces, "surfaces", 4, true}, {dirs, "dirs", 4, true}, {outPdf, "outPdf", 4, true}};
    if (const int rc = rtrdev::check_ptrs(who, args)) return rc;
    for (uint32_t k = 0; k < n; ++k) outPdf[k] = rtr_mis_bounce_pdf(&rays[k], &surfaces[k], rtr_ld3(dirs + 3 * (size_t)k), lobes);
    return RTR_OK;
}

extern "C" int rtr_host_mis_weights(uint32_t n, const float* pb, const float* dist, const float* cosLight, const float* area, uint32_t Ttot, uint32_t P,
                                    RtrMisSample* outSamples, float* outWBounce) {
    const char* who = "rtr_host_mis_weights";
    if (P > RTR_PICK_MAX) return rtrdev::refusef("%s: P %u (0 ... %u)", who, P, RTR_PICK_MAX);
    if (Ttot > RTR_PICK_MAX_SLOTS) return rtrdev::refusef("%s: Ttot %u is more than RTR_PICK_MAX_SLOTS = 2^24", who, Ttot);
    if (n == 0) return RTR_OK;
    const rtrdev::Arg args[6] = {{pb, "pb", 4, true}, {dist, "dist", 4, true}, {cosLight, "cosLight", 4, true}, {area, "area", 4, true},
                                 {outSamples, "outSamples", 4, true}, {outWBounce, "outWBounce", 4, false}};
    if (const int rc = rtrdev::check_ptrs(who, args)) return rc;
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
    if (const int rc = rtrdev::mis_check_params(who, mis)) return rc;
    if (mis->numAreaLights > numLights) return rtrdev::refusef("%s: numAreaLights %u > lights %u", who, mis->numAreaLights, numLights);
    const bool lit = numLights != 0u;
    const rtrdev::Arg table[3] = {{lightTris, "lightTris", 1, lit}, {lightTriFirst, "lightTriFirst", 1, lit}, {lights, "lights", 1, lit}};
    if (const int rc = rtrdev::check_ptrs(who, table)) return rc;
    if (n == 0) return RTR_OK;
    if (const int rc = rtrdev::mis_check_emitter_arrays(who, rays, hits, prevSurfaces, bounces, out)) return rc;
    uint64_t tris = 0;
    for (uint32_t l = 0; l < mis->numAreaLights; ++l) tris += lights[l].numTriangles;
    if (tris > RTR_PICK_MAX_SLOTS) return rtrdev::refusef("%s: %llu light triangles are more than 2^24", who, (unsigned long long)tris);
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
