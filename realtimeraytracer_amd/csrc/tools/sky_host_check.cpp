/* sky_host_check — the host forms of include/rtr_sky.h under the host sanitizers: a stand-alone program around rtr_sky_host.cpp, built
 * with -fsanitize=address,undefined by `make sky_host_check` (never part of a library, never loaded into Python).  It builds the table
 * of HDRIs of 1 x 1 ... 257 x 33 texels (RGBA8 and R8, random, black, one bright texel in a corner) and of the constant sky on exactly
 * sized heap arrays, so that a read or write past an array is caught; runs rtr_host_sky_rays, rtr_host_sky_hits, rtr_host_sky_pdf and
 * rtr_host_sky_radiance for 1 ... 20000 records with inputs that reach every early return (surfaces that are not objects, views from
 * behind the shading normal, NaN and infinite words, null rays, random numbers of 1.0 through the seeds); checks that no output word is
 * a NaN or an infinity, that a dead sample is the null ray and zero bytes, that the sums are prefix sums, and every kind of refusal.
 * Exit status 0 and "ok" when nothing was reported. */
#include "../rtr_sky_host.h"
#include "host_check.h"
#include "../../../include/rtr_sky.h"

#include <cmath>
#include <cstring>

static const float kOdd[8] = {0.0f, 1e-40f, NAN, INFINITY, -INFINITY, 1e30f, -1.0f, 1e-30f};

static bool all_zero(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) if (b[i]) return false;
    return true;
}

int main() {
    int bad = 0;
    size_t records = 0;
    uint32_t s = 4242u;
    const uint32_t extents[6][2] = {{1, 1}, {2, 1}, {3, 5}, {64, 32}, {65, 7}, {257, 33}};
    const uint32_t sizes[6] = {1, 63, 64, 65, 257, 20000};
    const float skyColor[3] = {0.2f, 0.5f, 0.9f};
    for (int kindOfSky = 0; kindOfSky < 4; ++kindOfSky)          /* random, black, one corner texel, the constant sky */
        for (const auto& ext : extents)
            for (uint32_t ch = 1; ch <= 4; ch += 3) {
                if (kindOfSky == 3 && (ext[0] != 1 || ch != 1)) continue;
                const uint32_t W = ext[0], H = ext[1];
                uint8_t* px = static_cast<uint8_t*>(malloc((size_t)W * H * ch));
                for (size_t i = 0; i < (size_t)W * H * ch; ++i) px[i] = kindOfSky == 0 ? (uint8_t)(lcg(s) >> 24) : 0;
                if (kindOfSky == 2) px[(size_t)(W - 1) * ch] = 200;
                rtr_texture tex{px, W, H, ch};
                const rtr_texture* hdri = kindOfSky == 3 ? nullptr : &tex;
                uint32_t tw = 0, th = 0;
                if (rtr_host_sky_table(hdri, skyColor, &tw, &th, nullptr, 0, nullptr, 0) != RTR_ERR_INVALID_ARGUMENT) ++bad;
                uint32_t* rows = static_cast<uint32_t*>(malloc((size_t)tw * th * sizeof(uint32_t)));
                uint64_t* marg = static_cast<uint64_t*>(malloc(th * sizeof(uint64_t)));
                if (rtr_host_sky_table(hdri, skyColor, &tw, &th, rows, (size_t)tw * th, marg, th) != RTR_OK) { fprintf(stderr, "rtr_host_sky_table: %s\n", g_err.c_str()); return 1; }
                uint64_t sum = 0;
                for (uint32_t y = 0; y < th; ++y) {
                    for (uint32_t x = 1; x < tw; ++x) if (rows[(size_t)y * tw + x] < rows[(size_t)y * tw + x - 1]) ++bad;
                    sum += rows[(size_t)y * tw + tw - 1];
                    if (marg[y] != sum) ++bad;
                }
                if ((kindOfSky == 1) != (sum == 0)) ++bad;
                const rtr_sky_table table{rows, marg, tw, th};
                for (uint32_t n : sizes) {
                    if (n > 300 && W * H > 64) continue;
                    for (uint32_t S = 1; S <= RTR_SKY_MAX_SAMPLES; S += 7) {
                        RtrRay* rays = aligned<RtrRay>(n);
                        RtrSurface* sf = aligned<RtrSurface>(n);
                        RtrHit* hits = aligned<RtrHit>(n);
                        RtrBounce* bo = aligned<RtrBounce>(n);
                        uint32_t* seeds = static_cast<uint32_t*>(malloc(n * sizeof(uint32_t)));
                        RtrRay* outRays = aligned<RtrRay>((size_t)n * S);
                        RtrSkySample* outS = aligned<RtrSkySample>((size_t)n * S);
                        RtrSkyEscape* esc = aligned<RtrSkyEscape>(n);
                        float* pdf = static_cast<float*>(malloc(n * sizeof(float)));
                        float* rad = static_cast<float*>(malloc((size_t)n * 3 * sizeof(float)));
                        float* dirs = static_cast<float*>(malloc((size_t)n * 3 * sizeof(float)));
                        memset(rays, 0, n * sizeof(RtrRay)); memset(sf, 0, n * sizeof(RtrSurface)); memset(hits, 0, n * sizeof(RtrHit)); memset(bo, 0, n * sizeof(RtrBounce));
                        for (uint32_t k = 0; k < n; ++k) {
                            RtrSurface& f = sf[k];
                            f.kind = (k % 17u == 3u) ? RTR_SURFACE_LIGHT : RTR_SURFACE_OBJECT;
                            f.position[0] = unit(s) - 0.5f; f.position[1] = unit(s) - 0.5f;
                            f.normal[k % 3u] = (k & 8u) ? -1.0f : 1.0f;
                            f.color[0] = unit(s); f.color[1] = unit(s); f.color[2] = unit(s);
                            f.roughness = (k % 5u) * 0.25f; f.metallic = (k % 3u) * 0.5f;
                            rays[k].origin[0] = 3.0f * (unit(s) - 0.5f); rays[k].origin[1] = 3.0f * (unit(s) - 0.5f); rays[k].origin[2] = 3.0f * (unit(s) - 0.5f);
                            for (int i = 0; i < 3; ++i) dirs[3 * (size_t)k + i] = unit(s) - 0.5f;
                            if (k % 13u == 5u) for (int i = 0; i < 3; ++i) dirs[3 * (size_t)k + i] = 0.0f;      /* the null ray */
                            if (k % 13u == 6u) { dirs[3 * (size_t)k] = 0.0f; dirs[3 * (size_t)k + 2] = 0.0f; }  /* a pole */
                            const float o = kOdd[lcg(s) >> 29];
                            switch (k % 19u) {
                                case 0: f.normal[1] = o; break;
                                case 1: f.position[0] = o; break;
                                case 2: dirs[3 * (size_t)k + 2] = o; break;
                                case 3: bo[k].pdf = o; break;
                                case 4: f.roughness = o; break;
                                case 5: rays[k].origin[2] = o; break;
                                default: bo[k].pdf = unit(s) * 3.0f; break;
                            }
                            seeds[k] = lcg(s);
                            hits[k].customIndex = k % 4u == 0u ? 7u : 0xffffffffu;
                        }
                        for (uint32_t flags = 0; flags <= 1; ++flags) {
                            rtr_sky_params p{};
                            p.numSamples = S; p.depth = n % 5u; p.frame = n; p.width = 16; p.spp = 1; p.lobes = 3; p.flags = flags;
                            memset(outRays, 0xA5, (size_t)n * S * sizeof(RtrRay)); memset(outS, 0xA5, (size_t)n * S * sizeof(RtrSkySample));
                            if (rtr_host_sky_rays(hdri, skyColor, &table, rays, sf, n, &p, flags ? seeds : nullptr, outRays, outS) != RTR_OK) { fprintf(stderr, "rtr_host_sky_rays: %s\n", g_err.c_str()); return 1; }
                            for (size_t i = 0; i < (size_t)n * S; ++i) {
                                const float* w = reinterpret_cast<const float*>(&outRays[i]);
                                const float* v = reinterpret_cast<const float*>(&outS[i]);
                                for (int q = 0; q < 8; ++q) if (!std::isfinite(w[q])) ++bad;
                                for (int q = 0; q < 6; ++q) if (!std::isfinite(v[q]) || v[q] < 0.0f) ++bad;
                                const bool dead = outRays[i].tmax == 0.0f;
                                if (dead != all_zero(&outS[i], sizeof(RtrSkySample)) || (dead && !all_zero(&outRays[i], sizeof(RtrRay)))) ++bad;
                                if (!dead && (sf[i / S].kind != RTR_SURFACE_OBJECT || sum == 0 || outS[i].cell >= tw * th || !(outS[i].skyPdf > 0.0f))) ++bad;
                                ++records;
                            }
                            p.numSamples = S == 1 ? 0u : S;
                            for (uint32_t k = 0; k < n; ++k) memcpy(rays[k].direction, dirs + 3 * (size_t)k, 12);
                            memset(esc, 0xA5, n * sizeof(RtrSkyEscape));
                            if (rtr_host_sky_hits(hdri, skyColor, &table, rays, hits, sf, bo, n, &p, esc) != RTR_OK) { fprintf(stderr, "rtr_host_sky_hits: %s\n", g_err.c_str()); return 1; }
                            for (uint32_t k = 0; k < n; ++k) {
                                const float* v = reinterpret_cast<const float*>(&esc[k]);
                                for (int q = 0; q < 6; ++q) if (!std::isfinite(v[q]) || v[q] < 0.0f) ++bad;
                                if (hits[k].customIndex != 0xffffffffu && !all_zero(&esc[k], sizeof(RtrSkyEscape))) ++bad;
                                if (esc[k].wBounce > 1.0f || esc[k].kind != 0u || esc[k].cell >= tw * th) ++bad;
                                if ((flags == 0 || p.numSamples == 0) && hits[k].customIndex == 0xffffffffu && esc[k].wBounce != 1.0f) ++bad;
                            }
                        }
                        memset(pdf, 0xA5, n * sizeof(float)); memset(rad, 0xA5, (size_t)n * 3 * sizeof(float));
                        if (rtr_host_sky_pdf(&table, dirs, n, pdf) != RTR_OK || rtr_host_sky_radiance(hdri, skyColor, dirs, n, rad) != RTR_OK) { fprintf(stderr, "pdf / radiance: %s\n", g_err.c_str()); return 1; }
                        for (uint32_t k = 0; k < n; ++k) if (!std::isfinite(pdf[k]) || pdf[k] < 0.0f || !std::isfinite(rad[3 * (size_t)k]) || !std::isfinite(rad[3 * (size_t)k + 1]) || !std::isfinite(rad[3 * (size_t)k + 2])) ++bad;
                        free(rays); free(sf); free(hits); free(bo); free(seeds); free(outRays); free(outS); free(esc); free(pdf); free(rad); free(dirs);
                    }
                }
                free(px); free(rows); free(marg);
            }

    /* refusals */
    alignas(16) static RtrRay rays[4];
    alignas(16) static RtrSurface sf[2];
    alignas(16) static RtrHit hits[2];
    alignas(16) static RtrBounce bo[2];
    alignas(16) static RtrRay outRays[4];
    alignas(16) static RtrSkySample outS[4];
    alignas(16) static RtrSkyEscape esc[2];
    uint32_t rows[32 * 16], tw, th;
    uint64_t marg[16];
    float x[6] = {1, 1, 1, 1, 1, 1}, out[6];
    int refusals = 0;
    if (rtr_host_sky_table(nullptr, skyColor, &tw, &th, rows, 512, marg, 16) != RTR_OK || tw != 32 || th != 16) ++bad;
    const rtr_sky_table table{rows, marg, tw, th};
    rtr_sky_params p{};
    p.numSamples = 2; p.width = 4; p.spp = 1; p.lobes = 3; p.flags = RTR_SKY_MIS;
    rtr_sky_params q = p;
    uint8_t byte[4] = {1, 2, 3, 4};
    rtr_texture wide{byte, 65536, 1, 1}, odd{byte, 1, 1, 3}, none{nullptr, 1, 1, 1};
    REFUSED(rtr_host_sky_table(&wide, skyColor, &tw, &th, rows, 512, marg, 16), "rtr_host_sky_table", "65536 texels wide");
    REFUSED(rtr_host_sky_table(&odd, skyColor, &tw, &th, rows, 512, marg, 16), "rtr_host_sky_table", "bad extent or channels");
    REFUSED(rtr_host_sky_table(&none, skyColor, &tw, &th, rows, 512, marg, 16), "rtr_host_sky_table", "no pixels");
    REFUSED(rtr_host_sky_table(nullptr, nullptr, &tw, &th, rows, 512, marg, 16), "rtr_host_sky_table", "skyColor is null");
    REFUSED(rtr_host_sky_table(nullptr, skyColor, &tw, &th, rows, 511, marg, 16), "rtr_host_sky_table", "capacity 511 cells");
    REFUSED(rtr_host_sky_table(nullptr, skyColor, &tw, &th, rows, 512, marg, 15), "rtr_host_sky_table", "15 rows");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, nullptr, nullptr, outRays, outS), "rtr_host_sky_rays", "params is null");
    q = p; q.numSamples = 0; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &q, nullptr, outRays, outS), "rtr_host_sky_rays", "numSamples 0");
    q = p; q.numSamples = 9; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &q, nullptr, outRays, outS), "rtr_host_sky_rays", "numSamples 9");
    q = p; q.lobes = 0; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &q, nullptr, outRays, outS), "rtr_host_sky_rays", "lobes 0x0");
    q = p; q.lobes = 4; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &q, nullptr, outRays, outS), "rtr_host_sky_rays", "lobes 0x4");
    q = p; q.flags = 2; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &q, nullptr, outRays, outS), "rtr_host_sky_rays", "unknown flags bits 0x2");
    q = p; q._reserved = 1; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &q, nullptr, outRays, outS), "rtr_host_sky_rays", "_reserved");
    q = p; q.width = 0; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &q, nullptr, outRays, outS), "rtr_host_sky_rays", "width 0");
    q = p; q.spp = 0; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &q, nullptr, outRays, outS), "rtr_host_sky_rays", "spp 0");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, nullptr, sf, 2, &p, nullptr, outRays, outS), "rtr_host_sky_rays", "rays is null");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, nullptr, 2, &p, nullptr, outRays, outS), "rtr_host_sky_rays", "surfaces is null");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &p, nullptr, nullptr, outS), "rtr_host_sky_rays", "outRays is null");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &p, nullptr, outRays, nullptr), "rtr_host_sky_rays", "outSamples is null");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &p, nullptr, outRays, reinterpret_cast<RtrSkySample*>(reinterpret_cast<char*>(outS) + 8)), "rtr_host_sky_rays", "outSamples is not 16-B aligned");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 2, &p, nullptr, rays, outS), "rtr_host_sky_rays", "outRays overlaps rays");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, &table, rays, sf, 0x80000000u, &p, nullptr, outRays, outS), "rtr_host_sky_rays", "do not fit 32 bits");
    REFUSED(rtr_host_sky_rays(nullptr, skyColor, nullptr, rays, sf, 2, &p, nullptr, outRays, outS), "rtr_host_sky_rays", "table is null");
    { const rtr_sky_table t2{rows, marg, 16, 16}; REFUSED(rtr_host_sky_rays(nullptr, skyColor, &t2, rays, sf, 2, &p, nullptr, outRays, outS), "rtr_host_sky_rays", "the sky's is 32 x 16"); }
    q = p; q.numSamples = 9; REFUSED(rtr_host_sky_hits(nullptr, skyColor, &table, rays, hits, sf, bo, 2, &q, esc), "rtr_host_sky_hits", "numSamples 9 (0 ... 8)");
    REFUSED(rtr_host_sky_hits(nullptr, skyColor, &table, rays, hits, sf, nullptr, 2, &p, esc), "rtr_host_sky_hits", "bounces is null");
    REFUSED(rtr_host_sky_hits(nullptr, skyColor, &table, rays, nullptr, sf, bo, 2, &p, esc), "rtr_host_sky_hits", "hits is null");
    REFUSED(rtr_host_sky_hits(nullptr, skyColor, &table, rays, hits, sf, bo, 2, &p, reinterpret_cast<RtrSkyEscape*>(bo)), "rtr_host_sky_hits", "out overlaps bounces");
    REFUSED(rtr_host_sky_pdf(nullptr, x, 2, out), "rtr_host_sky_pdf", "table is null");
    REFUSED(rtr_host_sky_pdf(&table, nullptr, 2, out), "rtr_host_sky_pdf", "dirs is null");
    REFUSED(rtr_host_sky_pdf(&table, x, 2, nullptr), "rtr_host_sky_pdf", "outPdf is null");
    REFUSED(rtr_host_sky_radiance(nullptr, skyColor, nullptr, 2, out), "rtr_host_sky_radiance", "dirs is null");
    REFUSED(rtr_host_sky_radiance(nullptr, nullptr, x, 2, out), "rtr_host_sky_radiance", "skyColor is null");
    REFUSED(rtr_host_sky_radiance(&odd, skyColor, x, 2, out), "rtr_host_sky_radiance", "bad extent or channels");
    if (rtr_host_sky_rays(nullptr, skyColor, &table, nullptr, nullptr, 0, &p, nullptr, nullptr, nullptr) != RTR_OK) ++bad;
    if (rtr_host_sky_hits(nullptr, skyColor, &table, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr) != RTR_OK) ++bad;
    if (rtr_host_sky_pdf(&table, nullptr, 0, nullptr) != RTR_OK || rtr_host_sky_radiance(nullptr, skyColor, nullptr, 0, nullptr) != RTR_OK) ++bad;

    /* the checks the device entry points share */
    float o4[8];
    alignas(16) static float o16[8];
    if (rtrdev::sky_check_shade_call("f", outS, byte, 2, 2, o16) != RTR_OK) ++bad;
    bad += expect_refused(rtrdev::sky_check_shade_call("f", outS, byte, 2, 0, o16), "f", "numSamples 0");
    bad += expect_refused(rtrdev::sky_check_shade_call("f", outS, nullptr, 2, 2, o16), "f", "occluded is null");
    bad += expect_refused(rtrdev::sky_check_shade_call("f", outS, byte, 2, 2, reinterpret_cast<float*>(outS)), "f", "out overlaps samples");
    (void)o4;

    if (bad) { fprintf(stderr, "%d problems\n", bad); return 1; }
    printf("ok: %zu sky samples, %d refusals\n", records, refusals);
    return 0;
}
