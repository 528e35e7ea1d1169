/* accum_host_check — rtr_host_accumulate_paths and rtr_host_gather_records under the host sanitizers: a stand-alone program around
 * rtr_accum_host.cpp, built with -fsanitize=address,undefined by `make accum_host_check` (never part of a library, never loaded into
 * Python).  It runs the optional-array, flag, stride and id combinations of tests/test_accum_host.py at the sizes around the wave and
 * workgroup boundaries on exactly sized heap arrays, so that a read or write past a record is caught; checks every word against a
 * loop of its own; the gather at record sizes 4 ... 256 with rows in and out of range; and every kind of refusal.  Exit status 0 and
 * "ok" when nothing was reported. */
#include "../rtr_accum_host.h"
#include "host_check.h"

#include <cstring>
#include <vector>

static float value(uint32_t& s) {
    const uint32_t pick = lcg(s) >> 28;
    if (pick == 0u) return 0.0f;
    if (pick == 1u) return -0.0f;
    if (pick == 2u) return 1e-22f;
    return unit(s) * 3.0f - 1.0f;
}

int main() {
    const uint32_t sizes[8] = {1, 63, 64, 65, 255, 256, 257, 20000};
    int bad = 0;
    size_t runs = 0, added = 0, skipped = 0;
    for (uint32_t n : sizes)
        for (int variant = 0; variant < 64; ++variant) {
            const bool withEm = variant & 1, withEs = variant & 2, withSky = variant & 4, withB = variant & 8, withTerm = variant & 16, withIds = variant & 32;
            const uint32_t flags = (uint32_t)(variant + n) & 3u;
            const uint32_t tWords = variant % 3 == 0 ? 3u : (variant % 3 == 1 ? 4u : 8u), iWords = (variant & 4) ? 4u : 3u;
            const bool inplace = withB && tWords == 3u && (variant & 16);
            const uint32_t S = variant % 5 == 0 ? n + 9u : (variant % 5 == 1 && n > 7u ? n - 7u : n);
            uint32_t s = 17u + n + 31u * (uint32_t)variant;
            RtrRadiance* rad = aligned<RtrRadiance>(n);
            float* T = aligned<float>((size_t)(n - 1) * tWords + 3);                  /* exactly the bytes the call may read */
            uint32_t* ids = aligned<uint32_t>(n);
            RtrEmitter* em = aligned<RtrEmitter>(n);
            RtrSkyEscape* es = aligned<RtrSkyEscape>(n);
            float* sky = aligned<float>((size_t)n * 4);
            RtrBounce* bo = aligned<RtrBounce>(n);
            float* acc = aligned<float>((size_t)(S - 1) * iWords + 3);
            float* term = aligned<float>((size_t)(S - 1) * iWords + 3);
            float* outT = aligned<float>((size_t)n * 3);
            const size_t imgWords = (size_t)(S - 1) * iWords + 3;
            for (size_t i = 0; i < (size_t)(n - 1) * tWords + 3; ++i) T[i] = unit(s) * 1.5f;
            for (uint32_t k = 0; k < n; ++k) {
                memset(&rad[k], 0x5B, sizeof rad[k]); memset(&em[k], 0x5B, sizeof em[k]); memset(&es[k], 0x5B, sizeof es[k]); memset(&bo[k], 0x5B, sizeof bo[k]);
                rad[k].kind = lcg(s) >> 30;
                for (int a = 0; a < 3; ++a) { rad[k].shadowed[a] = value(s); em[k].radiance[a] = value(s) + 4.0f; es[k].radiance[a] = value(s) + 8.0f; bo[k].weight[a] = value(s); }
                for (int a = 0; a < 4; ++a) sky[4 * (size_t)k + a] = value(s);
                /* a permutation of 0 ... max(n, S) - 1 cut to n, with ids that name no slot put in */
                const uint32_t m = n > S ? n : S;
                ids[k] = (uint32_t)(((uint64_t)k * 7919u + 13u) % m);
                if (m % 7919u == 0u) ids[k] = k;
                if (k % 11u == 5u) ids[k] = k % 3u == 0u ? RTR_PATH_NONE : (k % 3u == 1u ? S : S + 5u);
            }
            for (size_t i = 0; i < imgWords; ++i) { acc[i] = value(s); term[i] = 9.0f; }
            std::vector<float> acc0(acc, acc + imgWords), T0(T, T + (size_t)(n - 1) * tWords + 3);
            memset(outT, 0xA5, (size_t)n * 12);
            rtr_accum_params p{};
            p.flags = flags; p.numSlots = S; p.throughputStrideBytes = 4u * tWords; p.imageStrideBytes = 4u * iWords;
            const int rc = rtr_host_accumulate_paths(rad, T, withIds ? ids : nullptr, withEm ? em : nullptr, withEs ? es : nullptr, withSky ? sky : nullptr,
                                                     withB ? bo : nullptr, n, &p, acc, withTerm ? term : nullptr, withB ? (inplace ? T : outT) : nullptr);
            ++runs;
            if (rc != RTR_OK) { fprintf(stderr, "rtr_host_accumulate_paths: %d %s\n", rc, g_err.c_str()); return 1; }
            std::vector<float> wantAcc(acc0), wantTerm(imgWords, 9.0f);
            int wrong = 0;
            for (uint32_t k = 0; k < n; ++k) {
                const float* t = &T0[(size_t)k * tWords];
                float r[3];
                for (int a = 0; a < 3; ++a) {
                    r[a] = rad[k].shadowed[a];
                    if (rad[k].kind == RTR_SURFACE_LIGHT && (flags & RTR_ACCUM_LIGHTS_FROM_EMITTERS)) r[a] = withEm ? em[k].radiance[a] : 0.0f;
                    if (rad[k].kind == RTR_SURFACE_MISS && (flags & RTR_ACCUM_MISSES_FROM_ESCAPES)) r[a] = withEs ? es[k].radiance[a] : 0.0f;
                }
                const uint32_t id = withIds ? ids[k] : k;
                for (int a = 0; a < 3; ++a) {
                    volatile float x = t[a] * r[a];
                    if (withSky) { volatile float y = t[a] * sky[4 * (size_t)k + a]; x = x + y; }
                    if (id < S) { wantAcc[(size_t)id * iWords + a] = acc0[(size_t)id * iWords + a] + x; wantTerm[(size_t)id * iWords + a] = x; }
                    if (withB) { volatile float w = t[a] * bo[k].weight[a]; const float got = (inplace ? T : outT)[3 * (size_t)k + a]; wrong += memcmp(&got, (const float*)&w, 4) != 0; }
                }
                if (id < S) ++added; else ++skipped;
            }
            wrong += memcmp(acc, wantAcc.data(), imgWords * 4) != 0;
            if (withTerm) wrong += memcmp(term, wantTerm.data(), imgWords * 4) != 0;
            if (!inplace) wrong += memcmp(T, T0.data(), T0.size() * 4) != 0;
            if (wrong) { fprintf(stderr, "n %u variant %d: %d differences\n", n, variant, wrong); ++bad; }
            free(rad); free(T); free(ids); free(em); free(es); free(sky); free(bo); free(acc); free(term); free(outT);
        }

    /* the gather: records of every size class, rows in range, RTR_PATH_NONE, numSrc and past it; a base 4 B past a multiple of 16 */
    const uint32_t recordSizes[6] = {4, 12, 32, 48, 80, 256};
    for (uint32_t bytes : recordSizes)
        for (uint32_t n : sizes)
            for (int shift = 0; shift < 2; ++shift) {
                const uint32_t w = bytes / 4u, numSrc = n > 3u ? n - 3u : 1u;
                uint32_t s = bytes + n;
                uint32_t* srcBase = aligned<uint32_t>((size_t)numSrc * w + 1);
                uint32_t* outBase = aligned<uint32_t>((size_t)n * w + 1);
                uint32_t* rows = aligned<uint32_t>(n);
                uint32_t* src = srcBase + shift; uint32_t* out = outBase + shift;
                for (size_t i = 0; i < (size_t)numSrc * w; ++i) src[i] = lcg(s) | 1u;
                for (uint32_t j = 0; j < n; ++j) rows[j] = j % 7u == 0u ? (j % 3u == 0u ? RTR_PATH_NONE : (j % 3u == 1u ? numSrc : numSrc + 5u)) : lcg(s) % numSrc;
                memset(out, 0xA5, (size_t)n * bytes);
                const int rc = rtr_host_gather_records(src, bytes, numSrc, rows, n, out);
                ++runs;
                if (rc != RTR_OK) { fprintf(stderr, "rtr_host_gather_records: %d %s\n", rc, g_err.c_str()); return 1; }
                for (uint32_t j = 0; j < n; ++j)
                    for (uint32_t c = 0; c < w; ++c) {
                        const uint32_t want = rows[j] < numSrc ? src[(size_t)rows[j] * w + c] : 0u;
                        if (out[(size_t)j * w + c] != want) { fprintf(stderr, "gather %u B, n %u, shift %d: row %u word %u\n", bytes, n, shift, j, c); ++bad; j = n; break; }
                    }
                free(srcBase); free(outBase); free(rows);
            }

    const uint32_t n = 64;
    RtrRadiance* rad = aligned<RtrRadiance>(n); float* T = aligned<float>(3 * n); uint32_t* ids = aligned<uint32_t>(n); RtrEmitter* em = aligned<RtrEmitter>(n);
    RtrSkyEscape* es = aligned<RtrSkyEscape>(n); float* sky = aligned<float>(4 * n); RtrBounce* bo = aligned<RtrBounce>(n);
    float* acc = aligned<float>(3 * n); float* term = aligned<float>(3 * n); float* outT = aligned<float>(3 * n);
    memset(rad, 0, n * sizeof *rad); memset(T, 0, 12 * n); memset(em, 0, n * sizeof *em); memset(es, 0, n * sizeof *es); memset(sky, 0, 16 * n);
    memset(bo, 0, n * sizeof *bo); memset(acc, 0, 12 * n); memset(term, 0, 12 * n); memset(outT, 0, 12 * n);
    for (uint32_t k = 0; k < n; ++k) ids[k] = k;
    rtr_accum_params p{};
    p.numSlots = n; p.throughputStrideBytes = 12; p.imageStrideBytes = 12;
    rtr_accum_params q = p;
    int refusals = 0;
    const char* who = "rtr_host_accumulate_paths";
    REFUSED(rtr_host_accumulate_paths(nullptr, T, ids, em, es, sky, bo, n, &p, acc, term, outT), who, "radiance is null");
    REFUSED(rtr_host_accumulate_paths(rad, nullptr, ids, em, es, sky, bo, n, &p, acc, term, outT), who, "throughput is null");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &p, nullptr, term, outT), who, "accum is null");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, nullptr, acc, term, outT), who, "params is null");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &p, acc, term, nullptr), who, "bounces without outThroughput");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, nullptr, n, &p, acc, term, outT), who, "outThroughput without bounces");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, reinterpret_cast<RtrEmitter*>(reinterpret_cast<char*>(em) + 4), es, sky, bo, n, &p, acc, term, outT), who, "emitters is not 16-B aligned");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky + 1, bo, n, &p, acc, term, outT), who, "skySums is not 16-B aligned");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &p, reinterpret_cast<float*>(reinterpret_cast<char*>(acc) + 2), term, outT), who, "accum is not 4-B aligned");
    q = p; q.throughputStrideBytes = 8; REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &q, acc, term, outT), who, "throughputStrideBytes");
    q = p; q.imageStrideBytes = 14; REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &q, acc, term, outT), who, "imageStrideBytes");
    q = p; q.flags = 4; REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &q, acc, term, outT), who, "flags");
    q = p; q._reserved[3] = 1; REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &q, acc, term, outT), who, "_reserved");
    q = p; q.numSlots = 0; REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &q, acc, term, outT), who, "numSlots is 0");
    q = p; q.numSlots = 0xffffffffu; q.imageStrideBytes = 0xfffffffcu; REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &q, acc, term, outT), who, "does not fit");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &p, sky, term, outT), who, "accum overlaps skySums");
    q = p; q.numSlots = n / 2; REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &q, acc, acc + 3 * (n / 2 - 1), outT), who, "accum overlaps outTerm");
    REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &p, acc, term, T + 3), who, "outThroughput overlaps throughput");
    q = p; q.throughputStrideBytes = 16; REFUSED(rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, 48, &q, acc, term, T), who, "outThroughput overlaps throughput");
    if (rtr_host_accumulate_paths(rad, T, ids, em, es, sky, bo, n, &p, acc, term, T) != RTR_OK) { fprintf(stderr, "in place: %s\n", g_err.c_str()); ++bad; }
    if (rtr_host_accumulate_paths(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != RTR_OK) ++bad;
    who = "rtr_host_gather_records";
    REFUSED(rtr_host_gather_records(rad, 0, n, ids, n, acc), who, "recordBytes");
    REFUSED(rtr_host_gather_records(rad, 6, n, ids, n, acc), who, "recordBytes");
    REFUSED(rtr_host_gather_records(rad, 260, n, ids, n, acc), who, "recordBytes");
    REFUSED(rtr_host_gather_records(nullptr, 12, n, ids, n, acc), who, "src is null");
    REFUSED(rtr_host_gather_records(T, 12, n, nullptr, n, acc), who, "rows is null");
    REFUSED(rtr_host_gather_records(T, 12, n, ids, n, nullptr), who, "out is null");
    REFUSED(rtr_host_gather_records(T, 12, n, ids, n, T + 3 * (n - 1) + 2), who, "out overlaps src");
    REFUSED(rtr_host_gather_records(T, 4, n, ids, n, ids), who, "out overlaps rows");
    if (rtr_host_gather_records(nullptr, 12, 0, ids, n, acc) != RTR_OK || rtr_host_gather_records(nullptr, 0, 0, nullptr, 0, nullptr) != RTR_OK) ++bad;

    free(rad); free(T); free(ids); free(em); free(es); free(sky); free(bo); free(acc); free(term); free(outT);
    if (bad) { fprintf(stderr, "%d problems\n", bad); return 1; }
    printf("ok: %zu runs, %zu rows added, %zu skipped, %d refusals\n", runs, added, skipped, refusals);
    return 0;
}
