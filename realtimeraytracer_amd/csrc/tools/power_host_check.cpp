/* power_host_check — the host forms of include/rtr_power.h under the host sanitizers: a stand-alone program around rtr_power_host.cpp
 * (with rtr_pick_host.cpp and rtr_mis_host.cpp, whose checks it calls), built with -fsanitize=address,undefined by
 * `make power_host_check` (never part of a library, never loaded into Python).  It runs rtr_host_light_power,
 * rtr_host_pick_slots_power, rtr_host_mis_weights_power and rtr_host_emitter_hits_power on exactly sized heap arrays, so that a read or
 * write past an array is caught: light tables of 1 ... 4099 triangles whose intensities, colours and areas include zeros, negatives, NaNs,
 * infinities and denormals, tables whose total is 0, every numAreaLights, 1 ... 20000 hits with P = 1, 2 and 30; checks that the sums
 * are those of the weights, that no triangle of weight 0 is ever drawn, that every slot is in range, that no output word is a NaN or an
 * infinity, that the weights add up to 1 where either is set, and every kind of refusal.  Exit status 0 and "ok" when nothing was
 * reported. */
#include "../rtr_power_host.h"
#include "host_check.h"
#include "../../../include/rtr_power.h"

#include <cmath>
#include <cstring>

static const float kOdd[8] = {0.0f, 1e-40f, NAN, INFINITY, -INFINITY, 1e30f, -1.0f, 1e-30f};

int main() {
    int bad = 0;
    size_t picks = 0, records = 0;
    uint32_t s = 4242u;
    const uint32_t lightCounts[5] = {1, 2, 3, 7, 64};
    const uint32_t triCounts[6] = {1, 5, 255, 256, 257, 4099};
    for (uint32_t numLights : lightCounts)
        for (uint32_t total : triCounts)
            for (int mode = 0; mode < 3; ++mode) {      /* 0: plain, 1: odd words, 2: nothing emits */
                if (total < numLights) continue;
                RtrAreaLightInfo* lights = static_cast<RtrAreaLightInfo*>(malloc(numLights * sizeof(RtrAreaLightInfo)));
                uint32_t* first = static_cast<uint32_t*>(malloc(numLights * sizeof(uint32_t)));
                float* rec = static_cast<float*>(malloc((size_t)total * 16 * sizeof(float)));
                uint32_t* w = static_cast<uint32_t*>(malloc(total * sizeof(uint32_t)));
                uint64_t* cdf = static_cast<uint64_t*>(malloc(total * sizeof(uint64_t)));
                memset(lights, 0, numLights * sizeof(RtrAreaLightInfo));
                uint32_t at = 0;
                for (uint32_t l = 0; l < numLights; ++l) {
                    first[l] = at;
                    const uint32_t left = total - at, lightsLeft = numLights - l;
                    lights[l].numTriangles = lightsLeft == 1u ? left : (l % 3u == 1u ? 0u : 1u + lcg(s) % (left - lightsLeft + 1u > 8u ? 8u : left - lightsLeft + 1u));
                    at += lights[l].numTriangles;
                    lights[l].color[0] = unit(s); lights[l].color[1] = unit(s); lights[l].color[2] = unit(s);
                    lights[l].intensity = mode == 2 ? 0.0f : (l % 4u == 2u ? 0.0f : unit(s) * 1000.0f);
                    lights[l].isTwoSided = l & 1u;
                    if (mode == 1 && l % 2u == 0u) lights[l].intensity = kOdd[lcg(s) >> 29];
                    if (mode == 1 && l % 5u == 1u) lights[l].color[lcg(s) % 3u] = kOdd[lcg(s) >> 29];
                }
                for (uint32_t t = 0; t < total; ++t) {
                    float* r = rec + 16 * (size_t)t;
                    memset(r, 0, 16 * sizeof(float));
                    r[0] = -1.0f + (float)(t % 7u); r[1] = -1.0f; r[2] = 2.0f; r[4] = 1.0f + (float)(t % 7u); r[5] = -1.0f; r[6] = 2.0f; r[8] = (float)(t % 7u); r[9] = 1.0f; r[10] = 2.0f;
                    r[3] = t % 9u == 4u ? 0.0f : unit(s) * 4.0f;
                    if (mode == 1 && t % 6u == 1u) r[3] = kOdd[lcg(s) >> 29];
                    r[7] = 1.0f / (0.7f * 2.0f); r[14] = t & 1u ? 1.0f : -1.0f;
                }
                memset(w, 0xA5, total * sizeof(uint32_t)); memset(cdf, 0xA5, total * sizeof(uint64_t));
                if (rtr_host_light_power(rec, first, lights, numLights, w, cdf) != RTR_OK) { fprintf(stderr, "rtr_host_light_power: %s\n", g_err.c_str()); return 1; }
                uint64_t sum = 0;
                uint32_t wMax = 0;
                for (uint32_t t = 0; t < total; ++t) {
                    sum += w[t];
                    wMax = w[t] > wMax ? w[t] : wMax;
                    if (cdf[t] != sum || w[t] > (1u << 20)) { ++bad; break; }
                }
                if (sum != 0u && wMax != (1u << 20)) ++bad;          /* the strongest triangle has the full weight */
                if (mode == 2 && sum != 0u) ++bad;

                for (uint32_t areaLights = 0; areaLights <= numLights; areaLights += (numLights > 7u ? 21u : 1u)) {
                    uint32_t tris = 0;
                    for (uint32_t l = 0; l < areaLights; ++l) tris += lights[l].numTriangles;
                    const uint32_t hitCounts[4] = {1, 65, 257, total == 4099u ? 20000u : 1000u};
                    for (uint32_t n : hitCounts)
                        for (uint32_t P : {1u, 2u, 30u}) {
                            for (int explicitSeeds = 0; explicitSeeds < 2; ++explicitSeeds) {
                                rtr_light_params lp{};
                                lp.numAreaLights = areaLights; lp.numShadowRays = 1u + (n % 3u); lp.frame = n; lp.width = 17; lp.spp = 2; lp.outputs = RTR_LIGHT_SHADOWED;
                                rtr_pick_params pp{};
                                pp.numPicks = P; pp.depth = n % 5u;
                                uint32_t* seeds = static_cast<uint32_t*>(malloc(n * sizeof(uint32_t)));
                                uint32_t* slots = static_cast<uint32_t*>(malloc((size_t)n * P * sizeof(uint32_t)));
                                float* wt = static_cast<float*>(malloc((size_t)n * P * sizeof(float)));
                                for (uint32_t k = 0; k < n; ++k) seeds[k] = lcg(s);
                                memset(slots, 0xA5, (size_t)n * P * sizeof(uint32_t)); memset(wt, 0xA5, (size_t)n * P * sizeof(float));
                                if (rtr_host_pick_slots_power(cdf, tris, explicitSeeds ? seeds : nullptr, n, &lp, &pp, slots, wt) != RTR_OK) {
                                    fprintf(stderr, "rtr_host_pick_slots_power: %s\n", g_err.c_str()); return 1;
                                }
                                const uint64_t tot = tris ? cdf[tris - 1u] : 0u;
                                for (size_t i = 0; i < (size_t)n * P; ++i) {
                                    ++picks;
                                    if (tot == 0u) { if (slots[i] != RTR_PICK_NONE || rtr_f2u(wt[i]) != 0u) { ++bad; break; } continue; }
                                    const uint32_t t = slots[i] / lp.numShadowRays;
                                    if (slots[i] >= tris * lp.numShadowRays || w[t] == 0u || !std::isfinite(wt[i]) || !(wt[i] > 0.0f)) { ++bad; break; }
                                    if (wt[i] != (float)tot / ((float)P * (float)w[t])) { ++bad; break; }
                                }
                                free(seeds); free(slots); free(wt);
                            }
                        }
                    /* the heuristic and the emitter records over this table */
                    const uint32_t n = 2000u;
                    float* col[4];
                    for (float*& c : col) c = static_cast<float*>(malloc(n * sizeof(float)));
                    uint32_t* lt = static_cast<uint32_t*>(malloc(n * sizeof(uint32_t)));
                    RtrMisSample* ms = static_cast<RtrMisSample*>(malloc(n * sizeof(RtrMisSample)));
                    float* wb = static_cast<float*>(malloc(n * sizeof(float)));
                    float* pw = static_cast<float*>(malloc(n * sizeof(float)));
                    for (uint32_t k = 0; k < n; ++k) {
                        col[0][k] = unit(s) * 3.0f; col[1][k] = unit(s) * 10.0f; col[2][k] = unit(s) * 2.0f - 1.0f; col[3][k] = unit(s) * 4.0f;
                        lt[k] = k % 13u == 0u ? total + k : lcg(s) % total;          /* past the table now and then */
                        if (mode == 1) col[k % 4u][k] = kOdd[lcg(s) >> 29];
                    }
                    for (uint32_t P : {0u, 1u, 30u}) {
                        memset(ms, 0xA5, n * sizeof(RtrMisSample)); memset(wb, 0xA5, n * sizeof(float)); memset(pw, 0xA5, n * sizeof(float));
                        if (rtr_host_mis_weights_power(n, col[0], col[1], col[2], col[3], lt, cdf, tris, P, ms, wb, pw) != RTR_OK) {
                            fprintf(stderr, "rtr_host_mis_weights_power: %s\n", g_err.c_str()); return 1;
                        }
                        for (uint32_t k = 0; k < n; ++k) {
                            const float a = ms[k].wPick, b = wb[k];
                            if (!std::isfinite(ms[k].lightPdf) || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite(pw[k]) || ms[k].lightTri != lt[k] || ms[k]._r) { ++bad; break; }
                            if ((a != 0.0f || b != 0.0f) && fabsf(a + b - 1.0f) > 2.4e-7f) { ++bad; break; }
                            const bool unpicked = lt[k] >= tris || w[lt[k]] == 0u;      /* P == 0 keeps lightPdf, as rtr_host_mis_weights does */
                            if ((unpicked || P == 0u) && (a != 0.0f || pw[k] != 0.0f || (unpicked && ms[k].lightPdf != 0.0f))) { ++bad; break; }
                        }
                    }
                    RtrRay* rays = aligned<RtrRay>(n);
                    RtrHit* hits = aligned<RtrHit>(n);
                    RtrSurface* sf = aligned<RtrSurface>(n);
                    RtrBounce* bo = aligned<RtrBounce>(n);
                    RtrEmitter* em = aligned<RtrEmitter>(n);
                    memset(rays, 0, n * sizeof(RtrRay)); memset(hits, 0, n * sizeof(RtrHit)); memset(sf, 0, n * sizeof(RtrSurface)); memset(bo, 0, n * sizeof(RtrBounce));
                    for (uint32_t k = 0; k < n; ++k) {
                        RtrSurface& f = sf[k];
                        f.kind = (k % 17u == 3u) ? RTR_SURFACE_LIGHT : RTR_SURFACE_OBJECT;
                        f.position[0] = unit(s) - 0.5f; f.position[1] = unit(s) - 0.5f; f.normal[2] = 1.0f;
                        float d[3] = {unit(s) - 0.5f, unit(s) - 0.5f, unit(s) * 1.2f - 0.2f};
                        for (int i = 0; i < 3; ++i) { rays[k].origin[i] = f.position[i] + 0.01f * f.normal[i]; rays[k].direction[i] = d[i]; }
                        rays[k].tmin = 0.001f; rays[k].tmax = 10000.0f;
                        bo[k].pdf = unit(s) * 3.0f;
                        hits[k].t = d[2] > 0.0f ? (2.0f - 0.01f) / d[2] : 10000.0f;
                        hits[k].customIndex = k % 11u == 0u ? 0xffffffffu : lcg(s) % (numLights + 2u);
                        hits[k].primitiveId = lcg(s) % 9u;
                        if (mode == 1 && k % 7u == 2u) bo[k].pdf = kOdd[lcg(s) >> 29];
                        if (mode == 1 && k % 7u == 4u) hits[k].t = kOdd[lcg(s) >> 29];
                    }
                    rtr_mis_params mp{};
                    mp.numPicks = 1u + areaLights % 30u; mp.numAreaLights = areaLights; mp.numShadowRays = 3; mp.lobes = 3;
                    memset(em, 0xA5, n * sizeof(RtrEmitter));
                    if (rtr_host_emitter_hits_power(rays, hits, sf, bo, n, rec, first, lights, numLights, cdf, &mp, em) != RTR_OK) {
                        fprintf(stderr, "rtr_host_emitter_hits_power: %s\n", g_err.c_str()); return 1;
                    }
                    for (uint32_t k = 0; k < n; ++k) {
                        const RtrEmitter& e = em[k];
                        const float f[6] = {e.radiance[0], e.radiance[1], e.radiance[2], e.wBounce, e.lightPdf, e.dist};
                        bool zero = e.lightTri == 0u && e.kind == 0u;
                        for (float x : f) { if (!std::isfinite(x)) { ++bad; } zero = zero && rtr_f2u(x) == 0u; }
                        if (e.kind != 0u && (e.kind != RTR_SURFACE_LIGHT || e.lightTri >= total || hits[k].customIndex >= numLights)) ++bad;
                        if (e.kind == 0u && !zero) ++bad;
                        const float area = e.kind != 0u ? rec[16 * (size_t)e.lightTri + 3] : 0.0f;      /* an area that is negative or not finite gives weights of 0 */
                        if (e.kind != 0u && std::isfinite(area) && area >= 0.0f && (e.lightTri >= tris || w[e.lightTri] == 0u) && e.wBounce != 1.0f) ++bad;
                        ++records;
                    }
                    free(rays); free(hits); free(sf); free(bo); free(em); free(lt); free(ms); free(wb); free(pw);
                    for (float* c : col) free(c);
                }
                free(lights); free(first); free(rec); free(w); free(cdf);
            }

    /* u == 1.0 stays in range, and the first index past the target is found at both ends */
    {
        const uint64_t c[4] = {5u, 5u, 9u, 1048585u};
        if (rtr_power_search(c, 4, rtr_power_target(1.0f, c[3])) != 3u || rtr_power_search(c, 4, rtr_power_target(0.0f, c[3])) != 0u) ++bad;
        if (rtr_power_search(c, 4, 5u) != 2u || rtr_power_search(c, 4, 4u) != 0u || rtr_power_search(c, 4, 9u) != 3u) ++bad;
        if (rtr_power_target(1.0f, 1u) != 0u || rtr_power_target(NAN, 7u) != 0u) ++bad;
    }

    /* refusals */
    alignas(16) static RtrRay rays[2];
    alignas(16) static RtrHit hits[2];
    alignas(16) static RtrSurface sf[2];
    alignas(16) static RtrBounce bo[2];
    alignas(16) static RtrEmitter em[2];
    static RtrMisSample ms[2];
    RtrAreaLightInfo lights[1];
    memset(lights, 0, sizeof lights);
    lights[0].numTriangles = 2; lights[0].intensity = 1.0f; lights[0].color[0] = 1.0f;
    const uint32_t first[1] = {0};
    alignas(16) float rec[32] = {0};
    rec[3] = 1.0f; rec[19] = 2.0f;
    uint32_t w[2], slots[4], lt[2] = {0, 1};
    uint64_t cdf[2];
    float x[4] = {1, 1, 1, 1}, wt[4];
    rtr_light_params lp{};
    lp.numAreaLights = 1; lp.numShadowRays = 1; lp.width = 8; lp.spp = 1; lp.outputs = RTR_LIGHT_SHADOWED;
    rtr_pick_params pp{};
    pp.numPicks = 2;
    rtr_mis_params mp{};
    mp.numPicks = 1; mp.numAreaLights = 1; mp.numShadowRays = 1; mp.lobes = 3;
    int refusals = 0;
    if (rtr_host_light_power(rec, first, lights, 1, w, cdf) != RTR_OK || w[0] != (1u << 19) || w[1] != (1u << 20) || cdf[1] != 3u * (1u << 19)) ++bad;
    REFUSED(rtr_host_light_power(nullptr, first, lights, 1, w, cdf), "rtr_host_light_power", "lightTris is null");
    REFUSED(rtr_host_light_power(rec, nullptr, lights, 1, w, cdf), "rtr_host_light_power", "lightTriFirst is null");
    REFUSED(rtr_host_light_power(rec, first, lights, 1, nullptr, cdf), "rtr_host_light_power", "outWeights is null");
    REFUSED(rtr_host_light_power(rec, first, lights, 1, w, reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(cdf) + 4)), "rtr_host_light_power", "outCdf is not 8-B aligned");
    { const uint32_t far[1] = {1}; REFUSED(rtr_host_light_power(rec, far, lights, 1, w, cdf), "rtr_host_light_power", "leaves the table"); }
    if (rtr_host_light_power(nullptr, nullptr, nullptr, 0, nullptr, nullptr) != RTR_OK) ++bad;
    REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, nullptr, &pp, slots, wt), "rtr_host_pick_slots_power", "params is null");
    REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, &lp, nullptr, slots, wt), "rtr_host_pick_slots_power", "pick params is null");
    { rtr_pick_params q = pp; q.numPicks = 0; REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, &lp, &q, slots, wt), "rtr_host_pick_slots_power", "numPicks 0"); }
    { rtr_pick_params q = pp; q.numPicks = 31; REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, &lp, &q, slots, wt), "rtr_host_pick_slots_power", "numPicks 31"); }
    { rtr_pick_params q = pp; q._reserved[5] = 1; REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, &lp, &q, slots, wt), "rtr_host_pick_slots_power", "_reserved"); }
    { rtr_light_params q = lp; q.width = 0; REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, &q, &pp, slots, wt), "rtr_host_pick_slots_power", "width 0"); }
    { rtr_light_params q = lp; q.numShadowRays = 0; REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, &q, &pp, slots, wt), "rtr_host_pick_slots_power", "numShadowRays 0"); }
    { rtr_light_params q = lp; q.numShadowRays = 1024; REFUSED(rtr_host_pick_slots_power(cdf, 1u << 24, nullptr, 2, &q, &pp, slots, wt), "rtr_host_pick_slots_power", "RTR_PICK_MAX_SLOTS"); }
    REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, &lp, &pp, nullptr, wt), "rtr_host_pick_slots_power", "outSlots is null");
    REFUSED(rtr_host_pick_slots_power(cdf, 2, nullptr, 2, &lp, &pp, slots, nullptr), "rtr_host_pick_slots_power", "outWeights is null");
    REFUSED(rtr_host_pick_slots_power(nullptr, 2, nullptr, 2, &lp, &pp, slots, wt), "rtr_host_pick_slots_power", "cdf is null");
    REFUSED(rtr_host_pick_slots_power(cdf, 2, reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(slots) + 2), 2, &lp, &pp, slots, wt), "rtr_host_pick_slots_power", "seeds is not 4-B aligned");
    if (rtr_host_pick_slots_power(nullptr, 0, nullptr, 2, &lp, &pp, slots, wt) != RTR_OK || slots[3] != RTR_PICK_NONE) ++bad;
    REFUSED(rtr_host_mis_weights_power(2, x, x, x, x, lt, cdf, 2, 31, ms, nullptr, nullptr), "rtr_host_mis_weights_power", "P 31");
    REFUSED(rtr_host_mis_weights_power(2, x, x, x, x, nullptr, cdf, 2, 1, ms, nullptr, nullptr), "rtr_host_mis_weights_power", "lightTri is null");
    REFUSED(rtr_host_mis_weights_power(2, x, x, x, x, lt, nullptr, 2, 1, ms, nullptr, nullptr), "rtr_host_mis_weights_power", "cdf is null");
    REFUSED(rtr_host_mis_weights_power(2, x, x, x, x, lt, cdf, 2, 1, nullptr, nullptr, nullptr), "rtr_host_mis_weights_power", "outSamples is null");
    REFUSED(rtr_host_emitter_hits_power(rays, hits, sf, bo, 2, rec, first, lights, 1, cdf, nullptr, em), "rtr_host_emitter_hits_power", "mis params is null");
    REFUSED(rtr_host_emitter_hits_power(rays, hits, sf, bo, 2, rec, first, lights, 1, nullptr, &mp, em), "rtr_host_emitter_hits_power", "cdf is null");
    { rtr_mis_params q = mp; q.numAreaLights = 2; REFUSED(rtr_host_emitter_hits_power(rays, hits, sf, bo, 2, rec, first, lights, 1, cdf, &q, em), "rtr_host_emitter_hits_power", "numAreaLights 2 > lights 1"); }
    { rtr_mis_params q = mp; q._reserved[0] = 1; REFUSED(rtr_host_emitter_hits_power(rays, hits, sf, bo, 2, rec, first, lights, 1, cdf, &q, em), "rtr_host_emitter_hits_power", "_reserved"); }
    REFUSED(rtr_host_emitter_hits_power(rays, hits, sf, nullptr, 2, rec, first, lights, 1, cdf, &mp, em), "rtr_host_emitter_hits_power", "bounces is null");
    if (rtr_host_emitter_hits_power(nullptr, nullptr, nullptr, nullptr, 0, rec, first, lights, 1, cdf, &mp, nullptr) != RTR_OK) ++bad;

    if (bad) { fprintf(stderr, "%d problems\n", bad); return 1; }
    printf("ok: %zu picks, %zu emitter records, %d refusals\n", picks, records, refusals);
    return 0;
}
