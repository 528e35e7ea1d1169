/* bounce_host_check — rtr_host_bounce_rays under the host sanitizers: a stand-alone program around rtr_bounce_host.cpp, built with
 * -fsanitize=address,undefined by `make bounce_host_check` (never part of a library, never loaded into Python).  It runs a few hundred
 * records — live ones over the whole material range, views from behind the shading normal and along the surface, every kind of dead one, seeds whose random number is exactly 1.0, exactly sized
 * heap arrays so that a read or write past a record is caught — and every refusal.  Exit status 0 and "ok" when nothing was reported. */
#include "../rtr_bounce_host.h"
#include "host_check.h"

#include <cmath>
#include <cstring>
#include <limits>

int main() {
    const uint32_t n = 640;
    RtrRay* rays = aligned<RtrRay>(n);
    RtrSurface* sf = aligned<RtrSurface>(n);
    uint32_t* seeds = aligned<uint32_t>(n);
    RtrRay* outRays = aligned<RtrRay>(n);
    RtrBounce* outBounce = aligned<RtrBounce>(n);
    const float rough[5] = {0.0f, 1e-3f, 0.05f, 0.3f, 1.0f}, metal[3] = {0.0f, 0.5f, 1.0f};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    uint32_t s = 12345u;
    for (uint32_t k = 0; k < n; ++k) {
        memset(&sf[k], 0, sizeof sf[k]); memset(&rays[k], 0, sizeof rays[k]);
        float nx = unit(s) * 2 - 1, ny = unit(s) * 2 - 1, nz = unit(s) * 2 - 1;
        const float len = std::sqrt(nx * nx + ny * ny + nz * nz) + 1e-9f;
        nx /= len; ny /= len; nz /= len;
        if (k % 97 == 0) { nx = 0; ny = 0; nz = -1; }                     /* the basis' pole */
        sf[k].kind = RTR_SURFACE_OBJECT;
        sf[k].normal[0] = nx; sf[k].normal[1] = ny; sf[k].normal[2] = nz;
        for (int a = 0; a < 3; ++a) { sf[k].position[a] = unit(s) * 20 - 10; sf[k].color[a] = (k % 11 == 0) ? 0.0f : unit(s); }
        sf[k].roughness = rough[k % 5]; sf[k].metallic = metal[(k / 5) % 3];
        for (int a = 0; a < 3; ++a) rays[k].origin[a] = sf[k].position[a] + sf[k].normal[a] * (0.5f + unit(s)) + (unit(s) - 0.5f);
        if (k % 7 == 2) for (int a = 0; a < 3; ++a) rays[k].origin[a] = 2.0f * sf[k].position[a] - rays[k].origin[a];      /* seen from behind the normal */
        if (k % 43 == 5) {                                                  /* dot(N, V) exactly 0 */
            sf[k].normal[0] = 0; sf[k].normal[1] = 0; sf[k].normal[2] = (k & 1u) ? 1.0f : -1.0f;
            rays[k].origin[2] = sf[k].position[2];
        }
        rays[k].tmax = 10000.0f;
        seeds[k] = lcg(s);
        if (k % 13 == 1) seeds[k] = 60418823u - 7919u - 3u - 100u * (k % 3);   /* rtr_random == 1.0 for u1, u2 or uLobe */
        switch (k % 29) {                                                   /* the dead ones */
            case 1: sf[k].kind = RTR_SURFACE_MISS; break;
            case 2: sf[k].kind = RTR_SURFACE_LIGHT; break;
            case 3: sf[k].kind = RTR_SURFACE_INVALID; break;
            case 4: sf[k].kind = 0xdeadbeefu; break;
            case 5: sf[k].normal[1] = nan; break;
            case 6: sf[k].position[2] = inf; break;
            case 7: sf[k].color[0] = -inf; break;
            case 8: sf[k].roughness = nan; break;
            case 9: rays[k].origin[0] = inf; break;
            case 10: sf[k].metallic = 1.0f; sf[k].color[0] = sf[k].color[1] = sf[k].color[2] = 0.0f; sf[k].roughness = 0.0f; break;
            case 11: for (int a = 0; a < 3; ++a) rays[k].origin[a] = sf[k].position[a]; break;      /* no view vector */
            case 12: sf[k].normal[0] = sf[k].normal[1] = sf[k].normal[2] = 0.0f; break;
            case 13: sf[k].position[0] = 3.0e38f; sf[k].normal[0] = 1.0f; break;
            case 14: sf[k].color[1] = -0.5f; break;
            case 15: sf[k].roughness = 1e-30f; break;                                                 /* alpha2 underflows to 0 */
            case 16: sf[k].metallic = nan; break;
            default: break;
        }
    }
    int bad = 0;
    const uint32_t lobeSets[3] = {RTR_BOUNCE_DIFFUSE, RTR_BOUNCE_SPECULAR, RTR_BOUNCE_DIFFUSE | RTR_BOUNCE_SPECULAR};
    size_t live = 0;
    for (uint32_t lobes : lobeSets)
        for (int withSeeds = 0; withSeeds < 2; ++withSeeds) {
            rtr_bounce_params p{};
            p.frame = 3; p.depth = 0; p.width = 31; p.spp = 2; p.lobes = lobes; p.normalOffset = 0.01f; p.tmin = 0.001f; p.tmax = 10000.0f;
            memset(outRays, 0xA5, n * sizeof *outRays); memset(outBounce, 0xA5, n * sizeof *outBounce);
            const int rc = rtr_host_bounce_rays(rays, sf, n, &p, withSeeds ? seeds : nullptr, outRays, outBounce);
            if (rc != RTR_OK) { fprintf(stderr, "rtr_host_bounce_rays: %d %s\n", rc, g_err.c_str()); return 1; }
            for (uint32_t k = 0; k < n; ++k) {
                const float* f = reinterpret_cast<const float*>(&outRays[k]);
                const float* g = reinterpret_cast<const float*>(&outBounce[k]);
                bool finite = true;
                for (int a = 0; a < 8; ++a) finite = finite && std::isfinite(f[a]);
                for (int a = 0; a < 4; ++a) finite = finite && std::isfinite(g[a]);
                finite = finite && std::isfinite(outBounce[k].pSpecular);
                if (!finite) { fprintf(stderr, "record %u (lobes %u): a word is not finite\n", k, lobes); ++bad; }
                const bool dead = outBounce[k].lobe == 0u;
                const uint32_t c = k % 29;
                if (withSeeds && c >= 1 && c <= 16 && c != 13 && c != 14 && c != 15 && !dead) { fprintf(stderr, "record %u (case %u) should be dead\n", k, c); ++bad; }
                if (dead) {
                    static const unsigned char zero[32] = {0};
                    if (memcmp(&outRays[k], zero, 32) || memcmp(&outBounce[k], zero, 32)) { fprintf(stderr, "dead record %u is not zeros\n", k); ++bad; }
                } else ++live;
            }
        }
    if (live < 1000) { fprintf(stderr, "only %zu live records\n", live); ++bad; }

    rtr_bounce_params p{};
    p.width = 8; p.spp = 1; p.lobes = 3; p.normalOffset = 0.01f; p.tmin = 0.001f; p.tmax = 10000.0f;
    rtr_bounce_params q = p;
    const char* who = "rtr_host_bounce_rays";
    bad += expect_refused(rtr_host_bounce_rays(nullptr, sf, n, &p, seeds, outRays, outBounce), who, "rays is null");
    bad += expect_refused(rtr_host_bounce_rays(rays, sf, n, nullptr, seeds, outRays, outBounce), who, "params is null");
    bad += expect_refused(rtr_host_bounce_rays(rays, sf, n, &p, seeds, reinterpret_cast<RtrRay*>(reinterpret_cast<char*>(outRays) + 4), outBounce), who, "outRays is not 16-B aligned");
    q = p; q.lobes = 0; bad += expect_refused(rtr_host_bounce_rays(rays, sf, n, &q, seeds, outRays, outBounce), who, "lobes");
    q = p; q.width = 0; bad += expect_refused(rtr_host_bounce_rays(rays, sf, n, &q, nullptr, outRays, outBounce), who, "width");
    q = p; q.tmax = nan; bad += expect_refused(rtr_host_bounce_rays(rays, sf, n, &q, seeds, outRays, outBounce), who, "tmax");
    q = p; q.tmin = 5.0f; q.tmax = 5.0f; bad += expect_refused(rtr_host_bounce_rays(rays, sf, n, &q, seeds, outRays, outBounce), who, "tmax");
    bad += expect_refused(rtr_host_bounce_rays(rays, sf, n, &p, seeds, rays, outBounce), who, "outRays overlaps rays");
    if (rtr_host_bounce_rays(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != RTR_OK) ++bad;

    free(rays); free(sf); free(seeds); free(outRays); free(outBounce);
    if (bad) { fprintf(stderr, "%d problems\n", bad); return 1; }
    printf("ok: %u records x 6 runs, %zu live, 9 refusals\n", n, live);
    return 0;
}
