/* rtr_paths_host.cpp — rtr_host_compact_paths, rtr_compact_scratch_bytes and the argument checks rtr_compact_paths shares with them.
 * Pure host C++ with no HIP in it: include/rtr_paths.h compiled for the host cores with the kernels' flags (-ffp-contract=off, no
 * fast-math), so that the device's words can be held to these bits; a translation unit of its own so that a stand-alone program
 * (tools/compact_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_paths_host.h"
#include "../../include/rtr_paths.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

namespace rtrdev {

static bool overlaps(const void* a, size_t aBytes, const void* b, size_t bBytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bBytes && b0 < a0 + aBytes;
}

size_t compact_scratch_bytes(uint32_t numPaths) {
    const size_t groups = ((size_t)numPaths + 255u) / 256u;
    return groups * 32u + (groups * 4u + 15u) / 16u * 16u;
}

bool compact_check_args(const char* who, const CompactCall& c, char* msg, size_t msgBytes) {
    const rtr_compact_params* p = c.params;
    if (!p) { snprintf(msg, msgBytes, "%s: params is null", who); return false; }
    const size_t n = c.n;
    struct Range { const void* ptr; const char* name; size_t bytes; unsigned align; bool needed; };
    const size_t stride = p->throughputStrideBytes;
    const Range in[4] = {{c.rays, "rays", n * sizeof(RtrRay), 16, true}, {c.throughput, "throughput", (n - 1) * stride + 12u, 4, true},
                         {c.seeds, "seeds", n * 4u, 4, false}, {c.pathIds, "pathIds", n * 4u, 4, false}};
    const Range out[6] = {{c.outRays, "outRays", n * sizeof(RtrRay), 16, true}, {c.outThroughput, "outThroughput", n * 12u, 4, true},
                          {c.outSeeds, "outSeeds", n * 4u, 4, c.seeds != nullptr}, {c.outPathIds, "outPathIds", n * 4u, 4, true},
                          {c.outCount, "outCount", 4u, 4, true}, {c.scratch, "scratch", c.scratchBytes, 16, c.wantsScratch}};
    for (int i = 0; i < 10; ++i) {
        const Range& r = i < 4 ? in[i] : out[i - 4];
        if (r.needed && !r.ptr) { snprintf(msg, msgBytes, "%s: %s is null", who, r.name); return false; }
    }
    for (int i = 0; i < 10; ++i) {
        const Range& r = i < 4 ? in[i] : out[i - 4];
        if (r.ptr && ((uintptr_t)r.ptr & (r.align - 1u))) { snprintf(msg, msgBytes, "%s: %s is not %u-B aligned", who, r.name, r.align); return false; }
    }
    if (!c.seeds && c.outSeeds) { snprintf(msg, msgBytes, "%s: outSeeds without seeds (seeds is null)", who); return false; }
    if (c.wantsScratch && c.scratchBytes < c.scratchNeed) {
        snprintf(msg, msgBytes, "%s: scratchBytes %zu is below rtr_compact_scratch_bytes(%u) = %zu", who, c.scratchBytes, c.n, c.scratchNeed);
        return false;
    }
    if (stride < 12u || (stride & 3u)) {
        snprintf(msg, msgBytes, "%s: throughputStrideBytes %u (a multiple of 4, at least 12)", who, p->throughputStrideBytes);
        return false;
    }
    if (p->flags & ~RTR_COMPACT_ROULETTE) { snprintf(msg, msgBytes, "%s: flags 0x%x (RTR_COMPACT_ROULETTE or 0)", who, p->flags); return false; }
    if (p->flags & RTR_COMPACT_ROULETTE) {
        if (!c.seeds) { snprintf(msg, msgBytes, "%s: RTR_COMPACT_ROULETTE needs seeds (seeds is null)", who); return false; }
        if (!(p->survivalFloor > 0.0f && p->survivalFloor <= 1.0f)) {
            snprintf(msg, msgBytes, "%s: survivalFloor %g is not in (0, 1]", who, (double)p->survivalFloor);
            return false;
        }
    }
    if (p->_reserved[0] | p->_reserved[1] | p->_reserved[2]) { snprintf(msg, msgBytes, "%s: _reserved words of params are not 0", who); return false; }
    for (int o = 0; o < 6; ++o) {
        if (!out[o].ptr) continue;
        for (int i = 0; i < 4; ++i)
            if (in[i].ptr && overlaps(out[o].ptr, out[o].bytes, in[i].ptr, in[i].bytes)) {
                snprintf(msg, msgBytes, "%s: %s overlaps %s", who, out[o].name, in[i].name);
                return false;
            }
        for (int q = 0; q < o; ++q)
            if (out[q].ptr && overlaps(out[o].ptr, out[o].bytes, out[q].ptr, out[q].bytes)) {
                snprintf(msg, msgBytes, "%s: %s overlaps %s", who, out[q].name, out[o].name);
                return false;
            }
    }
    return true;
}

}  // namespace rtrdev

extern "C" int rtr_compact_scratch_bytes(uint32_t numPaths, size_t* bytes) {
    if (!bytes) { rtrdev::set_last_error("rtr_compact_scratch_bytes: bytes is null"); return RTR_ERR_INVALID_ARGUMENT; }
    *bytes = rtrdev::compact_scratch_bytes(numPaths);
    return RTR_OK;
}

extern "C" int rtr_host_compact_paths(const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds,
                                      uint32_t n, const rtr_compact_params* p,
                                      RtrRay* outRays, float* outThroughput, uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount) {
    if (n == 0) {
        if (outCount) *outCount = 0u;
        return RTR_OK;
    }
    char msg[256];
    const rtrdev::CompactCall c{rays, throughput, seeds, pathIds, n, p, nullptr, 0, 0, false, outRays, outThroughput, outSeeds, outPathIds, outCount};
    if (!rtrdev::compact_check_args("rtr_host_compact_paths", c, msg, sizeof msg)) {
        rtrdev::set_last_error(msg);
        return RTR_ERR_INVALID_ARGUMENT;
    }
    uint32_t count = 0;
    for (uint32_t k = 0; k < n; ++k) {
        float T[3], outT[3];
        memcpy(T, reinterpret_cast<const char*>(throughput) + (size_t)k * p->throughputStrideBytes, 12);
        if (!rtr_path_survive(&rays[k], T, seeds ? seeds[k] : 0u, p, outT)) continue;
        outRays[count] = rays[k];
        memcpy(outThroughput + 3 * (size_t)count, outT, 12);
        if (outSeeds) outSeeds[count] = seeds[k];
        outPathIds[count] = pathIds ? pathIds[k] : k;
        ++count;
    }
    for (uint32_t j = count; j < n; ++j) {
        memset(&outRays[j], 0, sizeof(RtrRay));
        memset(outThroughput + 3 * (size_t)j, 0, 12);
        if (outSeeds) outSeeds[j] = 0u;
        outPathIds[j] = RTR_PATH_NONE;
    }
    *outCount = count;
    return RTR_OK;
}
