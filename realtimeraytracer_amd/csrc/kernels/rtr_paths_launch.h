/* rtr_paths_launch.h — host-callable launcher of the path-compaction kernels (kernels/rtr_paths.hip; internal to librtr_hip.so). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/rtr_types.h"

namespace rtrdev {

struct CompactArgs {
    const float4* rays;              /* RtrRay as 2 x float4 */
    const char* throughput;          /* path k's three floats at throughput + k * params.throughputStrideBytes */
    const uint32_t* seeds;           /* or null (no roulette then) */
    const uint32_t* pathIds;         /* or null: path k has id k */
    unsigned long long* ballots;     /* scratch: one 64-bit survivor mask per wave, four per workgroup (the last workgroup's too) */
    uint32_t* groupTotals;           /* scratch: survivors per 256-path workgroup; k_compact_scan turns them into exclusive offsets */
    float4* outRays;
    float* outThroughput;            /* packed, stride 12 */
    uint32_t* outSeeds;              /* or null, with seeds */
    uint32_t* outPathIds;
    uint32_t* outCount;
    rtr_compact_params params;
    uint32_t n;
};

/* k_compact_count, k_compact_scan, k_compact_scatter on the stream, n > 0.  The scratch layout: ballots at scratch, groupTotals at
 * scratch + 32 * ceil(n / 256) (rtr_paths_host.cpp: compact_scratch_bytes). */
hipError_t launch_compact_paths(const CompactArgs& a, hipStream_t stream);

}  // namespace rtrdev
