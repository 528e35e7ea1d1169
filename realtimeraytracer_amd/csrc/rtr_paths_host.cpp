/* rtr_paths_host.cpp — rtr_host_compact_paths, rtr_compact_scratch_bytes and the argument checks rtr_compact_paths shares with them.
 * Pure host C++ with no HIP in it: include/rtr_paths.h compiled for the host cores with the kernels' flags (-ffp-contract=off, no
 * fast-math), so that the device's words can be held to these bits; a translation unit of its own so that a stand-alone program
 * (tools/compact_host_check.cpp) can run it under the host sanitizers. */
#include "rtr_paths_host.h"
#include "../../include/rtr_paths.h"

#include <cstdint>
#include <cstring>

namespace rtrdev {

size_t compact_scratch_bytes(uint32_t numPaths) {
    const size_t groups = ((size_t)numPaths + 255u) / 256u;
    return groups * 32u + (groups * 4u + 15u) / 16u * 16u;
}

int compact_check_args(const char* who, const CompactCall& c) {
    const rtr_compact_params* p = c.params;
    if (!p) return refusef("%s: params is null", who);
    const size_t n = c.n, stride = p->throughputStrideBytes;
    const Arg a[10] = {{c.rays, "rays", 16, true, n * sizeof(RtrRay)}, {c.throughput, "throughput", 4, true, (n - 1) * stride + 12u},
                       {c.seeds, "seeds", 4, false, n * 4u}, {c.pathIds, "pathIds", 4, false, n * 4u},
                       {c.outRays, "outRays", 16, true, n * sizeof(RtrRay)}, {c.outThroughput, "outThroughput", 4, true, n * 12u},
                       {c.outSeeds, "outSeeds", 4, c.seeds != nullptr, n * 4u}, {c.outPathIds, "outPathIds", 4, true, n * 4u},
                       {c.outCount, "outCount", 4, true, 4u}, {c.scratch, "scratch", 16, c.wantsScratch, c.scratchBytes}};
    if (const int rc = check_ptrs(who, a)) return rc;
    if (!c.seeds && c.outSeeds) return refusef("%s: outSeeds without seeds (seeds is null)", who);
    if (c.wantsScratch && c.scratchBytes < c.scratchNeed)
        return refusef("%s: scratchBytes %zu is below rtr_compact_scratch_bytes(%u) = %zu", who, c.scratchBytes, c.n, c.scratchNeed);
    if (stride < 12u || (stride & 3u)) return refusef("%s: throughputStrideBytes %u (a multiple of 4, at least 12)", who, p->throughputStrideBytes);
    if (p->flags & ~RTR_COMPACT_ROULETTE) return refusef("%s: flags 0x%x (RTR_COMPACT_ROULETTE or 0)", who, p->flags);
    if (p->flags & RTR_COMPACT_ROULETTE) {
        if (!c.seeds) return refusef("%s: RTR_COMPACT_ROULETTE needs seeds (seeds is null)", who);
        if (!(p->survivalFloor > 0.0f && p->survivalFloor <= 1.0f)) return refusef("%s: survivalFloor %g is not in (0, 1]", who, (double)p->survivalFloor);
    }
    if (const int rc = check_reserved(who, p->_reserved, 3, "params")) return rc;
    return check_overlaps(who, a, 4, a + 4, 6);       /* the four inputs, then the six outputs */
}

}  // namespace rtrdev

extern "C" int rtr_compact_scratch_bytes(uint32_t numPaths, size_t* bytes) {
    if (!bytes) return rtrdev::refuse("rtr_compact_scratch_bytes: bytes is null");
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
    const rtrdev::CompactCall c{rays, throughput, seeds, pathIds, n, p, nullptr, 0, 0, false, outRays, outThroughput, outSeeds, outPathIds, outCount};
    if (const int rc = rtrdev::compact_check_args("rtr_host_compact_paths", c)) return rc;
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
