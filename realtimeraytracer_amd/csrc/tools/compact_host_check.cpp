/* compact_host_check — rtr_host_compact_paths under the host sanitizers: a stand-alone program around rtr_paths_host.cpp, built with
 * -fsanitize=address,undefined by `make compact_host_check` (never part of a library, never loaded into Python).  It runs the liveness
 * patterns of tests/test_compact_host.py — all live, all dead, only the first, only the last, alternating, one whole 256-block dead,
 * random at 0.5 and at 0.05 — at the sizes around the wave and workgroup boundaries, with and without seeds, ids and the roulette, at
 * stride 12 and 32, on exactly sized heap arrays so that a read or write past a record is caught; checks the count, the stable order
 * and the cleared tail; and every kind of refusal.  Exit status 0 and "ok" when nothing was reported. */
#include "../rtr_paths_host.h"
#include "host_check.h"

#include <cstring>
#include <limits>
#include <vector>

static bool wanted_live(int pattern, uint32_t k, uint32_t n, uint32_t& s) {
    switch (pattern) {
        case 0: return true;
        case 1: return false;
        case 2: return k == 0;
        case 3: return k == n - 1;
        case 4: return (k & 1u) == 0;
        case 5: return k / 256u != 1u;
        case 6: return unit(s) < 0.5f;
        default: return unit(s) < 0.05f;
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const uint32_t sizes[8] = {1, 63, 64, 65, 255, 256, 257, 20000};
    int bad = 0;
    size_t runs = 0, survivors = 0;
    for (uint32_t n : sizes)
        for (int pattern = 0; pattern < 8; ++pattern)
            for (int variant = 0; variant < 4; ++variant) {
                const uint32_t strideWords = (variant & 1) ? 8u : 3u;
                const bool withSeeds = variant < 3, withIds = (variant & 2) != 0, roulette = variant == 2;
                RtrRay* rays = aligned<RtrRay>(n);
                float* thr = aligned<float>((size_t)(n - 1) * strideWords + 3);          /* exactly the bytes the call may read */
                uint32_t* seeds = aligned<uint32_t>(n);
                uint32_t* ids = aligned<uint32_t>(n);
                RtrRay* outRays = aligned<RtrRay>(n);
                float* outT = aligned<float>((size_t)n * 3);
                uint32_t* outSeeds = aligned<uint32_t>(n);
                uint32_t* outIds = aligned<uint32_t>(n);
                std::vector<char> live(n);
                uint32_t s = 99u + n + 7u * (uint32_t)pattern, dead = 0;
                for (uint32_t k = 0; k < n; ++k) {
                    live[k] = wanted_live(pattern, k, n, s);
                    RtrRay& r = rays[k];
                    for (int a = 0; a < 3; ++a) { r.origin[a] = unit(s) * 20 - 10; r.direction[a] = unit(s) + 0.01f; }
                    r.tmin = 0.001f; r.tmax = 10000.0f;
                    float* T = thr + (size_t)k * strideWords;
                    for (int a = 0; a < 3; ++a) T[a] = (roulette ? 2.0f : 1.0f) * (unit(s) + 0.001f);
                    if (!live[k]) switch (dead++ % 9) {
                        case 0: memset(&r, 0, sizeof r); break;
                        case 1: r.tmax = r.tmin; break;
                        case 2: r.origin[1] = nan; break;
                        case 3: r.direction[0] = inf; break;
                        case 4: r.direction[0] = r.direction[1] = 0.0f; r.direction[2] = -0.0f; break;
                        case 5: T[2] = nan; break;
                        case 6: T[0] = inf; break;
                        case 7: T[1] = -1e-30f; break;
                        default: T[0] = T[1] = T[2] = 0.0f; break;
                    }
                    else if (k % 11 == 3) { T[0] = -0.0f; T[1] = 0.0f; T[2] = 1.0f; }     /* live */
                    seeds[k] = lcg(s); ids[k] = 1000u + (n - 1 - k);
                }
                rtr_compact_params p{};
                p.frame = 3; p.depth = 1; p.flags = roulette ? RTR_COMPACT_ROULETTE : 0u; p.survivalFloor = 0.1f; p.throughputStrideBytes = 4u * strideWords;
                memset(outRays, 0xA5, n * sizeof *outRays); memset(outT, 0xA5, (size_t)n * 12); memset(outSeeds, 0xA5, n * 4u); memset(outIds, 0xA5, n * 4u);
                uint32_t count = 0xA5A5A5A5u;
                const int rc = rtr_host_compact_paths(rays, thr, withSeeds ? seeds : nullptr, withIds ? ids : nullptr, n, &p, outRays, outT,
                                                      withSeeds ? outSeeds : nullptr, outIds, &count);
                ++runs;
                if (rc != RTR_OK) { fprintf(stderr, "rtr_host_compact_paths: %d %s\n", rc, g_err.c_str()); return 1; }
                uint32_t expect = 0;
                for (uint32_t k = 0; k < n; ++k) expect += live[k] ? 1u : 0u;
                if (roulette ? count > expect : count != expect) { fprintf(stderr, "n %u pattern %d variant %d: count %u, %u live\n", n, pattern, variant, count, expect); ++bad; }
                survivors += count;
                /* the survivors are live inputs in their order, each with its own ray; the tail is cleared */
                uint32_t k = 0;
                for (uint32_t j = 0; j < count && j < n; ++j) {
                    const uint32_t src = withIds ? (n - 1 - (outIds[j] - 1000u)) : outIds[j];
                    if (src >= n || src < k || !live[src] || memcmp(&outRays[j], &rays[src], 32) || (withSeeds && outSeeds[j] != seeds[src])) {
                        fprintf(stderr, "n %u pattern %d variant %d: slot %u is not a live input after slot %u's\n", n, pattern, variant, j, j ? j - 1 : 0);
                        ++bad;
                        break;
                    }
                    if (!roulette && memcmp(outT + 3 * (size_t)j, thr + (size_t)src * strideWords, 12)) { fprintf(stderr, "slot %u: throughput changed\n", j); ++bad; break; }
                    k = src + 1;
                }
                static const unsigned char zero[32] = {0};
                for (uint32_t j = count; j < n; ++j)
                    if (memcmp(&outRays[j], zero, 32) || memcmp(outT + 3 * (size_t)j, zero, 12) || (withSeeds && outSeeds[j] != 0u) || outIds[j] != RTR_PATH_NONE) {
                        fprintf(stderr, "n %u pattern %d variant %d: tail slot %u is not cleared\n", n, pattern, variant, j);
                        ++bad;
                        break;
                    }
                free(rays); free(thr); free(seeds); free(ids); free(outRays); free(outT); free(outSeeds); free(outIds);
            }

    const uint32_t n = 64;
    RtrRay* rays = aligned<RtrRay>(n); float* thr = aligned<float>(3 * n); uint32_t* seeds = aligned<uint32_t>(n); uint32_t* ids = aligned<uint32_t>(n);
    RtrRay* outRays = aligned<RtrRay>(n); float* outT = aligned<float>(3 * n); uint32_t* outSeeds = aligned<uint32_t>(n); uint32_t* outIds = aligned<uint32_t>(n);
    memset(rays, 0, n * sizeof *rays); memset(thr, 0, 12 * n); memset(seeds, 0, 4 * n); memset(ids, 0, 4 * n);
    uint32_t count = 0;
    rtr_compact_params p{};
    p.throughputStrideBytes = 12; p.survivalFloor = 0.05f;
    rtr_compact_params q = p;
    int refusals = 0;
    const char* who = "rtr_host_compact_paths";
    REFUSED(rtr_host_compact_paths(nullptr, thr, seeds, ids, n, &p, outRays, outT, outSeeds, outIds, &count), who, "rays is null");
    REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, nullptr, outRays, outT, outSeeds, outIds, &count), who, "params is null");
    REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &p, outRays, outT, outSeeds, outIds, nullptr), who, "outCount is null");
    REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &p, outRays, outT, nullptr, outIds, &count), who, "outSeeds is null");
    REFUSED(rtr_host_compact_paths(rays, thr, nullptr, ids, n, &p, outRays, outT, outSeeds, outIds, &count), who, "outSeeds without seeds");
    REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &p, reinterpret_cast<RtrRay*>(reinterpret_cast<char*>(outRays) + 4), outT, outSeeds, outIds, &count), who, "outRays is not 16-B aligned");
    q = p; q.throughputStrideBytes = 8; REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &q, outRays, outT, outSeeds, outIds, &count), who, "throughputStrideBytes");
    q = p; q.flags = 2; REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &q, outRays, outT, outSeeds, outIds, &count), who, "flags");
    q = p; q.flags = 1; REFUSED(rtr_host_compact_paths(rays, thr, nullptr, ids, n, &q, outRays, outT, nullptr, outIds, &count), who, "needs seeds");
    q = p; q.flags = 1; q.survivalFloor = nan; REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &q, outRays, outT, outSeeds, outIds, &count), who, "survivalFloor");
    q = p; q.flags = 1; q.survivalFloor = 0.0f; REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &q, outRays, outT, outSeeds, outIds, &count), who, "survivalFloor");
    q = p; q._reserved[2] = 1; REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &q, outRays, outT, outSeeds, outIds, &count), who, "_reserved");
    REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &p, rays, outT, outSeeds, outIds, &count), who, "outRays overlaps rays");
    REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &p, outRays, outT, outSeeds, outSeeds, &count), who, "outSeeds overlaps outPathIds");
    REFUSED(rtr_host_compact_paths(rays, thr, seeds, ids, n, &p, outRays, outT, outSeeds, outIds, outIds + 5), who, "outPathIds overlaps outCount");
    size_t bytes = 1, last = 0;
    if (rtr_compact_scratch_bytes(7, nullptr) != RTR_ERR_INVALID_ARGUMENT) ++bad;
    for (uint32_t m = 0; m < 5000; ++m) {
        if (rtr_compact_scratch_bytes(m, &bytes) != RTR_OK || bytes % 16 || bytes < last) { fprintf(stderr, "scratch bytes of %u: %zu after %zu\n", m, bytes, last); ++bad; }
        last = bytes;
    }
    if (rtr_compact_scratch_bytes(0xffffffffu, &bytes) != RTR_OK || bytes % 16 || bytes < last) ++bad;
    count = 5;
    if (rtr_host_compact_paths(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &count) != RTR_OK || count != 0) ++bad;
    if (rtr_host_compact_paths(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != RTR_OK) ++bad;

    free(rays); free(thr); free(seeds); free(ids); free(outRays); free(outT); free(outSeeds); free(outIds);
    if (bad) { fprintf(stderr, "%d problems\n", bad); return 1; }
    printf("ok: %zu runs, %zu survivors, %d refusals\n", runs, survivors, refusals);
    return 0;
}
