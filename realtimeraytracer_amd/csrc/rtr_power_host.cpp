/* rtr_power_host.cpp — rtr_host_light_power, rtr_host_pick_slots_power, rtr_host_mis_weights_power, rtr_host_emitter_hits_power and the
 * argument check rtr_pick_slots_power shares with them.  Pure host C++ with no HIP in it: include/rtr_power.h compiled for the host
 * cores with the kernels' flags (-ffp-contract=off, no fast-math), so that the device's words can be held to these; a translation unit
 * of its own (with rtr_pick_host.cpp and rtr_mis_host.cpp, whose checks it calls) so that a stand-alone program
 * (tools/power_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_power_host.h"
#include "rtr_pick_host.h"
#include "rtr_mis_host.h"
#include "../../include/rtr_power.h"

#include <cstdint>

namespace rtrdev {

int power_check_pick_call(const char* who, const rtr_light_params* light, const rtr_pick_params* pick, uint32_t n, const uint32_t* seeds,
                          const uint32_t* outSlots, const float* outWeights) {
    if (n == 0u) return RTR_OK;
    if (const int rc = check_fits_32(who, n, "hits", pick->numPicks, "picks")) return rc;
    const Arg args[3] = {{outSlots, "outSlots", 4, true}, {outWeights, "outWeights", 4, true}, {seeds, "seeds", 4, false}};
    if (const int rc = check_ptrs(who, args)) return rc;
    return check_pixel_seeds(who, seeds, light->width, light->spp);
}

int power_check_table(const char* who, const uint64_t* cdf, uint32_t tris) {
    if (tris > RTR_PICK_MAX_SLOTS) return refusef("%s: tris %u is more than RTR_PICK_MAX_SLOTS = 2^24", who, tris);
    const Arg args[1] = {{cdf, "cdf", 8, tris != 0u}};
    return check_ptrs(who, args);
}

}  // namespace rtrdev

extern "C" int rtr_host_light_power(const float* lightTris, const uint32_t* lightTriFirst, const RtrAreaLightInfo* lights, uint32_t numLights,
                                    uint32_t* outWeights, uint64_t* outCdf) {
    const char* who = "rtr_host_light_power";
    if (numLights == 0u) return RTR_OK;
    const rtrdev::Arg table[2] = {{lightTriFirst, "lightTriFirst", 4, true}, {lights, "lights", 4, true}};
    if (const int rc = rtrdev::check_ptrs(who, table)) return rc;
    uint64_t total = 0;
    for (uint32_t l = 0; l < numLights; ++l) total += lights[l].numTriangles;
    if (total == 0u) return RTR_OK;
    if (total > 0xffffffffull) return rtrdev::refusef("%s: %llu light triangles do not fit 32 bits", who, (unsigned long long)total);
    const rtrdev::Arg arrays[3] = {{lightTris, "lightTris", 4, true}, {outWeights, "outWeights", 4, true}, {outCdf, "outCdf", 8, true}};
    if (const int rc = rtrdev::check_ptrs(who, arrays)) return rc;
    for (uint32_t l = 0; l < numLights; ++l)
        if ((uint64_t)lightTriFirst[l] + lights[l].numTriangles > total)
            return rtrdev::refusef("%s: lightTriFirst[%u] = %u with %u triangles leaves the table's %llu", who, l, lightTriFirst[l], lights[l].numTriangles,
                                   (unsigned long long)total);
    /* pw_t as float bits first, as the device keeps them, then the weights against their maximum, then the sums */
    float pwMax = 0.0f;
    for (uint32_t t = 0; t < (uint32_t)total; ++t) outWeights[t] = 0u;
    for (uint32_t l = 0; l < numLights; ++l)
        for (uint32_t i = 0; i < lights[l].numTriangles; ++i) {
            const uint32_t t = lightTriFirst[l] + i;
            const float pw = rtr_power_of(lights[l].color, lights[l].intensity, lightTris[16 * (size_t)t + 3]);
            outWeights[t] = rtr_f2u(pw);
            pwMax = rtr_max(pwMax, pw);
        }
    uint64_t sum = 0;
    for (uint32_t t = 0; t < (uint32_t)total; ++t) {
        const uint32_t w = rtr_power_weight(rtr_u2f(outWeights[t]), pwMax);
        outWeights[t] = w;
        sum += w;
        outCdf[t] = sum;
    }
    return RTR_OK;
}

extern "C" int rtr_host_pick_slots_power(const uint64_t* cdf, uint32_t tris, const uint32_t* seeds, uint32_t n, const rtr_light_params* p,
                                         const rtr_pick_params* pick, uint32_t* outSlots, float* outWeights) {
    const char* who = "rtr_host_pick_slots_power";
    if (const int rc = rtrdev::pick_check_params(who, p, pick, false)) return rc;
    if (const int rc = rtrdev::power_check_pick_call(who, p, pick, n, seeds, outSlots, outWeights)) return rc;
    if (const int rc = rtrdev::power_check_table(who, cdf, tris)) return rc;
    if (const int rc = rtrdev::pick_check_area(who, (uint64_t)tris * p->numShadowRays)) return rc;
    const uint32_t P = pick->numPicks;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t baseFrame = rtr_pick_base(seeds, k, p->width, p->spp) + p->frame;
        for (uint32_t q = 0; q < P; ++q)
            outSlots[(size_t)k * P + q] = rtr_power_pick(cdf, tris, p->numShadowRays, baseFrame, pick->depth, q, P, &outWeights[(size_t)k * P + q]);
    }
    return RTR_OK;
}

extern "C" int rtr_host_mis_weights_power(uint32_t n, const float* pb, const float* dist, const float* cosLight, const float* area, const uint32_t* lightTri,
                                          const uint64_t* cdf, uint32_t tris, uint32_t P, RtrMisSample* outSamples, float* outWBounce, float* outWeights) {
    const char* who = "rtr_host_mis_weights_power";
    if (P > RTR_PICK_MAX) return rtrdev::refusef("%s: P %u (0 ... %u)", who, P, RTR_PICK_MAX);
    if (const int rc = rtrdev::power_check_table(who, cdf, tris)) return rc;
    if (n == 0) return RTR_OK;
    const rtrdev::Arg args[8] = {{pb, "pb", 4, true}, {dist, "dist", 4, true}, {cosLight, "cosLight", 4, true}, {area, "area", 4, true},
                                 {lightTri, "lightTri", 4, true}, {outSamples, "outSamples", 4, true}, {outWBounce, "outWBounce", 4, false},
                                 {outWeights, "outWeights", 4, false}};
    if (const int rc = rtrdev::check_ptrs(who, args)) return rc;
    for (uint32_t k = 0; k < n; ++k) {
        RtrMisSample* o = &outSamples[k];
        const uint32_t t = lightTri[k];
        float wBounce;
        rtr_power_mis_weights(pb[k], dist[k], cosLight[k], area[k], rtr_power_ptri(cdf, tris, t), P, &o->lightPdf, &o->wPick, &wBounce);
        o->bouncePdf = pb[k]; o->cosLight = cosLight[k]; o->dist = dist[k]; o->area = area[k]; o->lightTri = t; o->_r = 0u;
        if (outWBounce) outWBounce[k] = wBounce;
        if (outWeights) {                                  /* what rtr_mis_pick_weights_power gives a pick on that triangle */
            float lightPdf, wPick;
            outWeights[k] = (t < tris && P != 0u) ? rtr_power_mis_pick(cdf, tris, t, P, pb[k], dist[k], cosLight[k], area[k], &lightPdf, &wPick) : 0.0f;
        }
    }
    return RTR_OK;
}

extern "C" int rtr_host_emitter_hits_power(const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces, uint32_t n,
                                           const float* lightTris, const uint32_t* lightTriFirst, const RtrAreaLightInfo* lights, uint32_t numLights,
                                           const uint64_t* cdf, const rtr_mis_params* mis, RtrEmitter* out) {
    const char* who = "rtr_host_emitter_hits_power";
    if (const int rc = rtrdev::mis_check_params(who, mis)) return rc;
    if (mis->numAreaLights > numLights) return rtrdev::refusef("%s: numAreaLights %u > lights %u", who, mis->numAreaLights, numLights);
    const bool lit = numLights != 0u;
    const rtrdev::Arg table[3] = {{lightTris, "lightTris", 1, lit}, {lightTriFirst, "lightTriFirst", 1, lit}, {lights, "lights", 1, lit}};
    if (const int rc = rtrdev::check_ptrs(who, table)) return rc;
    uint64_t tris = 0;
    for (uint32_t l = 0; l < mis->numAreaLights; ++l) tris += lights[l].numTriangles;
    if (tris > RTR_PICK_MAX_SLOTS) return rtrdev::refusef("%s: %llu light triangles are more than 2^24", who, (unsigned long long)tris);
    if (const int rc = rtrdev::power_check_table(who, cdf, (uint32_t)tris)) return rc;
    if (n == 0) return RTR_OK;
    if (const int rc = rtrdev::mis_check_emitter_arrays(who, rays, hits, prevSurfaces, bounces, out)) return rc;
    for (uint32_t k = 0; k < n; ++k) {
        rtr_mis_emitter_zero(&out[k]);
        const uint32_t l = hits[k].customIndex, prim = hits[k].primitiveId;
        if (l >= numLights || prim >= lights[l].numTriangles) continue;       /* a miss (0xffffffff), an object, ids out of range */
        const uint32_t t = lightTriFirst[l] + prim;
        rtr_power_mis_emitter(&rays[k], hits[k].t, &prevSurfaces[k], &bounces[k], lightTris + 16 * (size_t)t, t, lights[l].color, lights[l].intensity,
                              lights[l].isTwoSided, rtr_power_ptri(cdf, (uint32_t)tris, t), mis->numPicks, &out[k]);
    }
    return RTR_OK;
}
