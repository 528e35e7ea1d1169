/* mis_host_check — the host forms of include/rtr_mis.h under the host sanitizers: a stand-alone program around rtr_mis_host.cpp, built
 * with -fsanitize=address,undefined by `make mis_host_check` (never part of a library, never loaded into Python).  It runs
 * rtr_host_bounce_pdf, rtr_host_mis_weights and rtr_host_emitter_hits for 1 ... 20000 records on exactly sized heap arrays, so that a
 * read or write past an array is caught, with inputs that reach every early return (surfaces that are not objects, views from behind
 * the shading normal and along the surface, the direction -V, NaN and infinite
 * words, zero and denormal densities, distances and areas, ids out of range, one-sided lights from behind); checks that no output word is
 * a NaN or an infinity, that the weights add up to 1 where either is set, and every kind of refusal.  Exit status 0 and "ok" when
 * nothing was reported. */
#include "../rtr_mis_host.h"
#include "host_check.h"
#include "../../../include/rtr_mis.h"

#include <cmath>
#include <cstring>

static const float kOdd[8] = {0.0f, 1e-40f, NAN, INFINITY, -INFINITY, 1e30f, -1.0f, 1e-30f};

int main() {
    const uint32_t sizes[7] = {1, 63, 64, 65, 257, 4099, 20000};
    int bad = 0;
    size_t records = 0;
    /* a light table: three lights of 2 + 1 + 2 triangles, the second one-sided */
    const uint32_t numLights = 3, first[3] = {0, 2, 3};
    RtrAreaLightInfo lights[3];
    memset(lights, 0, sizeof lights);
    float* rec = static_cast<float*>(malloc(5 * 16 * sizeof(float)));
    uint32_t s = 99u;
    for (uint32_t l = 0; l < numLights; ++l) {
        lights[l].color[0] = 1.0f; lights[l].color[1] = 0.8f; lights[l].color[2] = 0.6f; lights[l].intensity = 5.0f;
        lights[l].numTriangles = l == 1 ? 1u : 2u; lights[l].isTwoSided = l == 1 ? 0u : 1u;
    }
    for (uint32_t t = 0; t < 5; ++t) {
        float* r = rec + 16 * t;
        memset(r, 0, 16 * sizeof(float));
        r[0] = -1.0f + t; r[1] = -1.0f; r[2] = 2.0f; r[4] = 1.0f + t; r[5] = -1.0f; r[6] = 2.0f; r[8] = 0.0f + t; r[9] = 1.0f; r[10] = 2.0f;
        r[3] = 2.0f; r[7] = 1.0f / (0.7f * 2.0f); r[14] = t & 1u ? 1.0f : -1.0f;
    }
    for (uint32_t n : sizes)
        for (int odd = 0; odd < 2; ++odd) {
            RtrRay* rays = static_cast<RtrRay*>(aligned_alloc(16, n * sizeof(RtrRay)));
            RtrHit* hits = static_cast<RtrHit*>(aligned_alloc(16, n * sizeof(RtrHit)));
            RtrSurface* sf = static_cast<RtrSurface*>(aligned_alloc(16, n * sizeof(RtrSurface)));
            RtrBounce* bo = static_cast<RtrBounce*>(aligned_alloc(16, n * sizeof(RtrBounce)));
            RtrEmitter* em = static_cast<RtrEmitter*>(aligned_alloc(16, n * sizeof(RtrEmitter)));
            RtrMisSample* ms = static_cast<RtrMisSample*>(malloc(n * sizeof(RtrMisSample)));
            float* dirs = static_cast<float*>(malloc((size_t)n * 3 * sizeof(float)));
            float* pdf = static_cast<float*>(malloc(n * sizeof(float)));
            float* col[4];
            for (float*& c : col) c = static_cast<float*>(malloc(n * sizeof(float)));
            float* wb = static_cast<float*>(malloc(n * sizeof(float)));
            memset(rays, 0, n * sizeof(RtrRay)); memset(hits, 0, n * sizeof(RtrHit)); memset(sf, 0, n * sizeof(RtrSurface)); memset(bo, 0, n * sizeof(RtrBounce));
            for (uint32_t k = 0; k < n; ++k) {
                RtrSurface& f = sf[k];
                f.kind = (k % 17u == 3u) ? RTR_SURFACE_LIGHT : RTR_SURFACE_OBJECT;
                f.position[0] = unit(s) - 0.5f; f.position[1] = unit(s) - 0.5f; f.position[2] = 0.0f;
                f.normal[2] = 1.0f; f.color[0] = unit(s); f.color[1] = unit(s); f.color[2] = unit(s);
                f.roughness = (k % 5u) * 0.25f; f.metallic = (k % 3u) * 0.5f;
                rays[k].origin[0] = f.position[0] + 0.3f; rays[k].origin[1] = f.position[1] - 0.2f; rays[k].origin[2] = 3.0f;
                if (k % 4u == 1u) rays[k].origin[2] = -3.0f;                     /* seen from behind the shading normal */
                if (k % 23u == 7u) rays[k].origin[2] = 0.0f;                     /* dot(N, V) exactly 0 */
                float d[3] = {unit(s) - 0.5f, unit(s) - 0.5f, unit(s) * 1.2f - 0.2f};
                if (k % 31u == 9u) for (int i = 0; i < 3; ++i) d[i] = f.position[i] - rays[k].origin[i];      /* L = -V: V + L cancels */
                const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-20f;
                for (int i = 0; i < 3; ++i) dirs[3 * (size_t)k + i] = d[i] / len;
                /* the bounce ray of this vertex: from 0.01 above it along dirs, ending on the plane z = 2 when it goes up */
                RtrRay& b = rays[k];
                b.tmin = 0.001f; b.tmax = 10000.0f;
                bo[k].pdf = unit(s) * 3.0f;
                hits[k].t = d[2] > 0.0f ? (2.0f - 0.01f) / (d[2] / len) : 10000.0f;
                hits[k].customIndex = k % 11u == 0u ? 0xffffffffu : k % 5u;      /* misses, the three lights, ids past them */
                hits[k].primitiveId = k % 3u;                                    /* past a light's triangles now and then */
                col[0][k] = bo[k].pdf; col[1][k] = unit(s) * 10.0f; col[2][k] = unit(s) * 2.0f - 1.0f; col[3][k] = unit(s) * 4.0f;
                if (odd) {                     /* odd words wherever a float is read */
                    const float o = kOdd[lcg(s) >> 29];
                    switch (k % 9u) {
                        case 0: f.normal[1] = o; break;
                        case 1: f.position[0] = o; break;
                        case 2: dirs[3 * (size_t)k + 2] = o; break;
                        case 3: bo[k].pdf = o; col[0][k] = o; break;
                        case 4: hits[k].t = o; col[1][k] = o; break;
                        case 5: f.roughness = o; col[2][k] = o; break;
                        case 6: rays[k].origin[2] = o; col[3][k] = o; break;
                        default: break;
                    }
                }
            }
            /* the emitter form reads rays as the BOUNCE rays: origin above the surface, direction dirs */
            RtrRay* brays = static_cast<RtrRay*>(aligned_alloc(16, n * sizeof(RtrRay)));
            for (uint32_t k = 0; k < n; ++k) {
                brays[k] = rays[k];
                for (int i = 0; i < 3; ++i) { brays[k].origin[i] = sf[k].position[i] + 0.01f * sf[k].normal[i]; brays[k].direction[i] = dirs[3 * (size_t)k + i]; }
            }
            for (uint32_t lobes = 1; lobes <= 3; ++lobes) {
                memset(pdf, 0xA5, n * sizeof(float));
                if (rtr_host_bounce_pdf(rays, sf, dirs, n, lobes, pdf) != RTR_OK) { fprintf(stderr, "rtr_host_bounce_pdf: %s\n", g_err.c_str()); return 1; }
                for (uint32_t k = 0; k < n; ++k) if (!std::isfinite(pdf[k]) || pdf[k] < 0.0f) { ++bad; break; }
            }
            const uint32_t tp[5][2] = {{0, 1}, {1, 0}, {1, 1}, {5, 2}, {1u << 24, 30}};
            for (const auto& c : tp) {
                memset(ms, 0xA5, n * sizeof(RtrMisSample)); memset(wb, 0xA5, n * sizeof(float));
                if (rtr_host_mis_weights(n, col[0], col[1], col[2], col[3], c[0], c[1], ms, wb) != RTR_OK) { fprintf(stderr, "rtr_host_mis_weights: %s\n", g_err.c_str()); return 1; }
                for (uint32_t k = 0; k < n; ++k) {
                    const float w = ms[k].wPick, b = wb[k];
                    if (!std::isfinite(ms[k].lightPdf) || !std::isfinite(w) || !std::isfinite(b) || ms[k].lightTri || ms[k]._r) { ++bad; break; }
                    if ((w != 0.0f || b != 0.0f) && fabsf(w + b - 1.0f) > 2.4e-7f) { ++bad; break; }
                }
            }
            for (uint32_t areaLights = 0; areaLights <= numLights; ++areaLights) {
                rtr_mis_params mp{};
                mp.numPicks = 1u + areaLights; mp.numAreaLights = areaLights; mp.numShadowRays = 3; mp.lobes = 3;
                memset(em, 0xA5, n * sizeof(RtrEmitter));
                if (rtr_host_emitter_hits(brays, hits, sf, bo, n, rec, first, lights, numLights, &mp, em) != RTR_OK) { fprintf(stderr, "rtr_host_emitter_hits: %s\n", g_err.c_str()); return 1; }
                for (uint32_t k = 0; k < n; ++k) {
                    const RtrEmitter& e = em[k];
                    const float f[6] = {e.radiance[0], e.radiance[1], e.radiance[2], e.wBounce, e.lightPdf, e.dist};
                    bool zero = e.lightTri == 0u && e.kind == 0u;
                    for (float x : f) { if (!std::isfinite(x)) { ++bad; } zero = zero && rtr_f2u(x) == 0u; }
                    if (e.kind != 0u && (e.kind != RTR_SURFACE_LIGHT || e.lightTri >= 5u || hits[k].customIndex >= numLights)) ++bad;
                    if (e.kind == 0u && !zero) ++bad;
                    if (e.kind != 0u && hits[k].customIndex >= areaLights && e.wBounce != 1.0f) ++bad;
                    ++records;
                }
            }
            free(rays); free(brays); free(hits); free(sf); free(bo); free(em); free(ms); free(dirs); free(pdf); free(wb);
            for (float* c : col) free(c);
        }

    /* refusals */
    alignas(16) static RtrRay rays[2];
    alignas(16) static RtrHit hits[2];
    alignas(16) static RtrSurface sf[2];
    alignas(16) static RtrBounce bo[2];
    alignas(16) static RtrEmitter em[2];
    static RtrMisSample ms[2];
    float x[6] = {1, 1, 1, 1, 1, 1}, out[2];
    rtr_mis_params mp{};
    mp.numPicks = 1; mp.numAreaLights = 1; mp.numShadowRays = 1; mp.lobes = 3;
    rtr_mis_params q = mp;
    int refusals = 0;
    REFUSED(rtr_host_bounce_pdf(rays, sf, x, 2, 0, out), "rtr_host_bounce_pdf", "lobes 0x0");
    REFUSED(rtr_host_bounce_pdf(rays, sf, x, 2, 4, out), "rtr_host_bounce_pdf", "lobes 0x4");
    REFUSED(rtr_host_bounce_pdf(nullptr, sf, x, 2, 3, out), "rtr_host_bounce_pdf", "rays is null");
    REFUSED(rtr_host_bounce_pdf(rays, sf, x, 2, 3, nullptr), "rtr_host_bounce_pdf", "outPdf is null");
    REFUSED(rtr_host_bounce_pdf(rays, sf, reinterpret_cast<float*>(reinterpret_cast<char*>(x) + 2), 1, 3, out), "rtr_host_bounce_pdf", "dirs is not 4-B aligned");
    REFUSED(rtr_host_mis_weights(2, x, x, x, x, 1, 31, ms, nullptr), "rtr_host_mis_weights", "P 31");
    REFUSED(rtr_host_mis_weights(2, x, x, x, x, (1u << 24) + 1u, 1, ms, nullptr), "rtr_host_mis_weights", "Ttot");
    REFUSED(rtr_host_mis_weights(2, x, nullptr, x, x, 1, 1, ms, nullptr), "rtr_host_mis_weights", "dist is null");
    REFUSED(rtr_host_mis_weights(2, x, x, x, x, 1, 1, nullptr, nullptr), "rtr_host_mis_weights", "outSamples is null");
    REFUSED(rtr_host_emitter_hits(rays, hits, sf, bo, 2, rec, first, lights, 3, nullptr, em), "rtr_host_emitter_hits", "mis params is null");
    q = mp; q.numPicks = 0; REFUSED(rtr_host_emitter_hits(rays, hits, sf, bo, 2, rec, first, lights, 3, &q, em), "rtr_host_emitter_hits", "numPicks 0");
    q = mp; q.lobes = 0; REFUSED(rtr_host_emitter_hits(rays, hits, sf, bo, 2, rec, first, lights, 3, &q, em), "rtr_host_emitter_hits", "lobes 0x0");
    q = mp; q._reserved[3] = 1; REFUSED(rtr_host_emitter_hits(rays, hits, sf, bo, 2, rec, first, lights, 3, &q, em), "rtr_host_emitter_hits", "_reserved");
    q = mp; q.numAreaLights = 4; REFUSED(rtr_host_emitter_hits(rays, hits, sf, bo, 2, rec, first, lights, 3, &q, em), "rtr_host_emitter_hits", "numAreaLights 4 > lights 3");
    REFUSED(rtr_host_emitter_hits(rays, hits, sf, bo, 2, nullptr, first, lights, 3, &mp, em), "rtr_host_emitter_hits", "lightTris is null");
    REFUSED(rtr_host_emitter_hits(rays, hits, sf, nullptr, 2, rec, first, lights, 3, &mp, em), "rtr_host_emitter_hits", "bounces is null");
    REFUSED(rtr_host_emitter_hits(rays, hits, sf, bo, 2, rec, first, lights, 3, &mp, reinterpret_cast<RtrEmitter*>(reinterpret_cast<char*>(em) + 8)), "rtr_host_emitter_hits", "out is not 16-B aligned");
    if (rtr_host_emitter_hits(nullptr, nullptr, nullptr, nullptr, 0, rec, first, lights, 3, &mp, nullptr) != RTR_OK) ++bad;
    if (rtr_host_bounce_pdf(nullptr, nullptr, nullptr, 0, 3, nullptr) != RTR_OK || rtr_host_mis_weights(0, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr) != RTR_OK) ++bad;

    /* the checks the device entry points share */
    rtr_light_params lp{};
    lp.numAreaLights = 1; lp.numShadowRays = 1; lp.width = 8; lp.spp = 1; lp.outputs = RTR_LIGHT_SHADOWED;
    rtr_pick_params pp{};
    pp.numPicks = 1;
    float w[2];
    if (rtrdev::mis_check_params("f", &mp) != RTR_OK) ++bad;
    if (rtrdev::mis_check_pick_call("f", &lp, &pp, &mp, rays, hits, 2, nullptr, nullptr, w, nullptr) != RTR_OK) ++bad;
    bad += expect_refused(rtrdev::mis_check_pick_call("f", &lp, &pp, &mp, rays, hits, 2, nullptr, nullptr, nullptr, nullptr), "f", "outWeights is null");
    pp.numPicks = 2;
    bad += expect_refused(rtrdev::mis_check_pick_call("f", &lp, &pp, &mp, rays, hits, 2, nullptr, nullptr, w, nullptr), "f", "is not the pick params'");
    if (rtrdev::mis_check_emitter_arrays("f", rays, hits, sf, bo, em) != RTR_OK) ++bad;
    bad += expect_refused(rtrdev::mis_check_emitter_arrays("f", rays, hits, nullptr, bo, em), "f", "prevSurfaces is null");

    free(rec);
    if (bad) { fprintf(stderr, "%d problems\n", bad); return 1; }
    printf("ok: %zu emitter records, %d refusals\n", records, refusals);
    return 0;
}
