/* ris_host_check — the host forms of include/rtr_ris.h under the host sanitizers: a stand-alone program around rtr_ris_host.cpp (with
 * rtr_power_host.cpp, rtr_pick_host.cpp and rtr_mis_host.cpp, whose checks it calls), built with -fsanitize=address,undefined by
 * `make ris_host_check` (never part of a library, never loaded into Python).  It runs rtr_host_ris_candidates and rtr_host_ris_select on
 * exactly sized heap arrays, so that a read or write past an array is caught: tables of 1 ... 4099 triangles some of weight 0, tables
 * whose total is 0, 1 ... 3000 hits with P = 1, 2 and 30 and M = 1, 2, 5 and 16, with seeds and with the pixel rule, targets that
 * include zeros, negatives, NaNs, infinities, denormals and values whose sum overflows, candidates that are RTR_PICK_NONE or past the
 * table; checks that candidate 0 is rtr_host_pick_slots_power's slot, that every candidate is a slot of a triangle that emits, that a
 * pick is one of its candidates with a positive finite target, that no output word is a NaN or an infinity, and every kind of refusal.
 * Exit status 0 and "ok" when nothing was reported. */
#include "../rtr_ris_host.h"
#include "host_check.h"
#include "../../../include/rtr_ris.h"

#include <cmath>
#include <cstring>

static const float kOdd[8] = {0.0f, 1e-40f, NAN, INFINITY, -INFINITY, 3e38f, -1.0f, 1e-30f};

int main() {
    int bad = 0;
    size_t picks = 0, held = 0;
    uint32_t s = 777u;
    const uint32_t triCounts[6] = {1, 5, 255, 256, 257, 4099};
    for (uint32_t total : triCounts)
        for (int mode = 0; mode < 3; ++mode) {      /* 0: plain targets, 1: odd targets and candidates, 2: nothing emits */
            uint64_t* cdf = static_cast<uint64_t*>(malloc(total * sizeof(uint64_t)));
            uint32_t* w = static_cast<uint32_t*>(malloc(total * sizeof(uint32_t)));
            uint64_t sum = 0;
            for (uint32_t t = 0; t < total; ++t) {
                w[t] = mode == 2 || t % 4u == 1u ? 0u : 1u + lcg(s) % (1u << 20);
                sum += w[t];
                cdf[t] = sum;
            }
            const uint32_t hitCounts[3] = {1, 65, total == 4099u ? 3000u : 300u};
            for (uint32_t n : hitCounts)
                for (uint32_t P : {1u, 2u, 30u})
                    for (uint32_t M : {1u, 2u, 5u, 16u})
                        for (int explicitSeeds = 0; explicitSeeds < 2; ++explicitSeeds)
                            for (uint32_t mis = 0; mis < 2u; ++mis) {
                                const uint32_t tris = n % 2u ? total : (total + 1u) / 2u;
                                rtr_light_params lp{};
                                lp.numAreaLights = 1; lp.numShadowRays = 1u + (n % 3u); lp.frame = n; lp.width = 17; lp.spp = 2; lp.outputs = RTR_LIGHT_SHADOWED;
                                rtr_pick_params pp{};
                                pp.numPicks = P; pp.depth = n % 5u;
                                rtr_ris_params rp{};
                                rp.numCandidates = M; rp.flags = mis ? RTR_RIS_MIS : 0u; rp.lobes = mis ? 3u : 0u;
                                const size_t np = (size_t)n * P, nc = np * M;
                                uint32_t* seeds = static_cast<uint32_t*>(malloc(n * sizeof(uint32_t)));
                                uint32_t* cand = static_cast<uint32_t*>(malloc(nc * sizeof(uint32_t)));
                                float* tg = static_cast<float*>(malloc(nc * sizeof(float)));
                                float* wp = static_cast<float*>(malloc(nc * sizeof(float)));
                                uint32_t* slots = static_cast<uint32_t*>(malloc(np * sizeof(uint32_t)));
                                uint32_t* pslots = static_cast<uint32_t*>(malloc(np * sizeof(uint32_t)));
                                float* wt = static_cast<float*>(malloc(np * sizeof(float)));
                                float* pwt = static_cast<float*>(malloc(np * sizeof(float)));
                                for (uint32_t k = 0; k < n; ++k) seeds[k] = lcg(s);
                                const uint32_t* sd = explicitSeeds ? seeds : nullptr;
                                memset(cand, 0xA5, nc * sizeof(uint32_t)); memset(slots, 0xA5, np * sizeof(uint32_t)); memset(wt, 0xA5, np * sizeof(float));
                                if (rtr_host_ris_candidates(cdf, tris, sd, n, &lp, &pp, M, cand) != RTR_OK || rtr_host_pick_slots_power(cdf, tris, sd, n, &lp, &pp, pslots, pwt) != RTR_OK) {
                                    fprintf(stderr, "rtr_host_ris_candidates: %s\n", g_err.c_str()); return 1;
                                }
                                const uint64_t tot = cdf[tris - 1u];
                                for (size_t i = 0; i < nc; ++i) {
                                    if (tot == 0u) { if (cand[i] != RTR_PICK_NONE) { ++bad; break; } continue; }
                                    if (cand[i] >= tris * lp.numShadowRays || w[cand[i] / lp.numShadowRays] == 0u) { ++bad; break; }
                                    if (i % M == 0u && cand[i] != pslots[i / M]) { ++bad; break; }
                                }
                                for (size_t i = 0; i < nc; ++i) {
                                    tg[i] = unit(s) < 0.25f ? 0.0f : unit(s) * 4.0f;
                                    wp[i] = 0.01f + 0.99f * unit(s);
                                    if (mode == 1 && i % 3u == 0u) tg[i] = kOdd[lcg(s) >> 29];
                                    if (mode == 1 && i % 7u == 3u) cand[i] = i % 2u ? RTR_PICK_NONE : tris * lp.numShadowRays + (uint32_t)(i % 5u);
                                    if (mode == 1 && i % 11u == 5u) wp[i] = kOdd[lcg(s) >> 29];
                                }
                                if (rtr_host_ris_select(cdf, tris, sd, n, &lp, &pp, &rp, cand, tg, mis ? wp : nullptr, slots, wt) != RTR_OK) {
                                    fprintf(stderr, "rtr_host_ris_select: %s\n", g_err.c_str()); return 1;
                                }
                                for (size_t i = 0; i < np; ++i) {
                                    ++picks;
                                    if (!std::isfinite(wt[i]) || wt[i] < 0.0f) { ++bad; break; }
                                    if (slots[i] == RTR_PICK_NONE) { if (rtr_f2u(wt[i]) != 0u) { ++bad; break; } continue; }
                                    ++held;
                                    bool found = false, any = false;
                                    for (uint32_t j = 0; j < M; ++j) {
                                        const bool live = cand[i * M + j] < tris * lp.numShadowRays && tg[i * M + j] > 0.0f && std::isfinite(tg[i * M + j]);
                                        any = any || live;
                                        found = found || (live && cand[i * M + j] == slots[i]);
                                    }
                                    if (!found || !any || tot == 0u) { ++bad; break; }
                                    /* M == 1, a plain target: the power pick and, to a few roundings, its weight */
                                    if (M == 1u && !mis && tg[i] > 1e-3f && (slots[i] != pslots[i] || fabsf(wt[i] - pwt[i]) > 8.0f * 5.9604645e-8f * pwt[i])) { ++bad; break; }
                                }
                                free(seeds); free(cand); free(tg); free(wp); free(slots); free(pslots); free(wt); free(pwt);
                            }
            free(cdf); free(w);
        }

    /* a W that overflows gives no pick; a single huge target is still a pick */
    {
        const uint64_t c[2] = {1u, 1u << 20};
        rtr_light_params lp{};
        lp.numAreaLights = 1; lp.numShadowRays = 1; lp.width = 4; lp.spp = 1; lp.outputs = RTR_LIGHT_SHADOWED;
        rtr_pick_params pp{};
        pp.numPicks = 1;
        rtr_ris_params rp{};
        rp.numCandidates = 16;
        uint32_t cand[16], slot[1];
        float tg[16], wt[1];
        for (int j = 0; j < 16; ++j) { cand[j] = 1u; tg[j] = 3e38f; }
        if (rtr_host_ris_select(c, 2, nullptr, 1, &lp, &pp, &rp, cand, tg, nullptr, slot, wt) != RTR_OK || slot[0] != RTR_PICK_NONE || rtr_f2u(wt[0]) != 0u) ++bad;
        for (int j = 1; j < 16; ++j) tg[j] = 0.0f;
        if (rtr_host_ris_select(c, 2, nullptr, 1, &lp, &pp, &rp, cand, tg, nullptr, slot, wt) != RTR_OK || slot[0] != 1u || !std::isfinite(wt[0]) || !(wt[0] > 0.0f)) ++bad;
    }

    /* refusals */
    const uint64_t cdf[2] = {5u, 9u};
    uint32_t cand[8] = {0}, slots[4];
    float tg[8] = {0}, wt[4];
    rtr_light_params lp{};
    lp.numAreaLights = 1; lp.numShadowRays = 1; lp.width = 8; lp.spp = 1; lp.outputs = RTR_LIGHT_SHADOWED;
    rtr_pick_params pp{};
    pp.numPicks = 2;
    rtr_ris_params rp{};
    rp.numCandidates = 2;
    int refusals = 0;
    REFUSED(rtr_host_ris_candidates(cdf, 2, nullptr, 2, nullptr, &pp, 2, cand), "rtr_host_ris_candidates", "params is null");
    REFUSED(rtr_host_ris_candidates(cdf, 2, nullptr, 2, &lp, nullptr, 2, cand), "rtr_host_ris_candidates", "pick params is null");
    REFUSED(rtr_host_ris_candidates(cdf, 2, nullptr, 2, &lp, &pp, 0, cand), "rtr_host_ris_candidates", "numCandidates 0");
    REFUSED(rtr_host_ris_candidates(cdf, 2, nullptr, 2, &lp, &pp, 17, cand), "rtr_host_ris_candidates", "numCandidates 17");
    REFUSED(rtr_host_ris_candidates(nullptr, 2, nullptr, 2, &lp, &pp, 2, cand), "rtr_host_ris_candidates", "cdf is null");
    REFUSED(rtr_host_ris_candidates(cdf, 2, nullptr, 2, &lp, &pp, 2, nullptr), "rtr_host_ris_candidates", "outCandidates is null");
    REFUSED(rtr_host_ris_candidates(cdf, 2, reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(cand) + 2), 2, &lp, &pp, 2, cand), "rtr_host_ris_candidates", "seeds is not 4-B aligned");
    { rtr_light_params q = lp; q.width = 0; REFUSED(rtr_host_ris_candidates(cdf, 2, nullptr, 2, &q, &pp, 2, cand), "rtr_host_ris_candidates", "width 0"); }
    { rtr_light_params q = lp; q.numShadowRays = 1024; REFUSED(rtr_host_ris_candidates(cdf, 1u << 24, nullptr, 2, &q, &pp, 2, cand), "rtr_host_ris_candidates", "RTR_PICK_MAX_SLOTS"); }
    { rtr_pick_params q = pp; q.numPicks = 30; REFUSED(rtr_host_ris_candidates(cdf, 2, nullptr, 0xffffffffu, &lp, &q, 16, cand), "rtr_host_ris_candidates", "do not fit 32 bits"); }
    if (rtr_host_ris_candidates(nullptr, 0, nullptr, 2, &lp, &pp, 2, cand) != RTR_OK || cand[7] != RTR_PICK_NONE) ++bad;
    REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, nullptr, cand, tg, nullptr, slots, wt), "rtr_host_ris_select", "ris params is null");
    { rtr_ris_params q = rp; q.flags = 2; REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &q, cand, tg, nullptr, slots, wt), "rtr_host_ris_select", "unknown flag bits"); }
    { rtr_ris_params q = rp; q.lobes = 1; REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &q, cand, tg, nullptr, slots, wt), "rtr_host_ris_select", "lobes 0x1 without RTR_RIS_MIS"); }
    { rtr_ris_params q = rp; q.flags = RTR_RIS_MIS; REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &q, cand, tg, tg, slots, wt), "rtr_host_ris_select", "lobes 0x0"); }
    { rtr_ris_params q = rp; q.flags = RTR_RIS_MIS; q.lobes = 3; REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &q, cand, tg, nullptr, slots, wt), "rtr_host_ris_select", "wPick is null"); }
    { rtr_ris_params q = rp; q._reserved[4] = 1; REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &q, cand, tg, nullptr, slots, wt), "rtr_host_ris_select", "_reserved words of ris params"); }
    REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &rp, nullptr, tg, nullptr, slots, wt), "rtr_host_ris_select", "candidates is null");
    REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &rp, cand, nullptr, nullptr, slots, wt), "rtr_host_ris_select", "targets is null");
    REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &rp, cand, tg, nullptr, nullptr, wt), "rtr_host_ris_select", "outSlots is null");
    REFUSED(rtr_host_ris_select(cdf, 2, nullptr, 2, &lp, &pp, &rp, cand, tg, nullptr, slots, nullptr), "rtr_host_ris_select", "outWeights is null");
    if (rtr_host_ris_select(nullptr, 0, nullptr, 2, &lp, &pp, &rp, cand, tg, nullptr, slots, wt) != RTR_OK || slots[3] != RTR_PICK_NONE || rtr_f2u(wt[3]) != 0u) ++bad;

    if (bad) { fprintf(stderr, "%d problems\n", bad); return 1; }
    printf("ok: %zu picks, %zu held, %d refusals\n", picks, held, refusals);
    return 0;
}
