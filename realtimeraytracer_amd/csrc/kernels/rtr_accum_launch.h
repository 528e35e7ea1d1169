/* rtr_accum_launch.h — host-callable launchers of the path-accumulation and record-gather kernels (kernels/rtr_accum.hip; internal to
 * librtr_hip.so). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/rtr_types.h"

namespace rtrdev {

struct AccumArgs {
    const float4* radiance;          /* RtrRadiance as 3 x float4, of which the first is read */
    const char* throughput;          /* path k's three floats at throughput + k * params.throughputStrideBytes */
    const uint32_t* pathIds;         /* or null: path k has id k */
    const float4* emitters;          /* RtrEmitter as 2 x float4, or null */
    const float4* escapes;           /* RtrSkyEscape as 2 x float4, or null */
    const float4* skySums;           /* rtr_shade_sky's rows, or null */
    const float4* bounces;           /* RtrBounce as 2 x float4, or null, with outThroughput */
    char* accum;                     /* slot id's three floats at accum + id * params.imageStrideBytes */
    char* outTerm;                   /* the same layout, or null */
    float* outThroughput;            /* packed, stride 12; may be the input itself when that is packed too */
    rtr_accum_params params;
    uint32_t n;
};

struct GatherArgs {
    const char* src;
    const uint32_t* rows;
    char* out;
    uint32_t recordBytes, numSrc, numRows;
};

/* k_accumulate_paths on the stream, n > 0: one launch */
hipError_t launch_accumulate_paths(const AccumArgs& a, hipStream_t stream);

/* k_gather_records on the stream, numRows > 0: one launch, a lane per 16-B chunk when recordBytes, src and out allow it, else per word */
hipError_t launch_gather_records(const GatherArgs& a, hipStream_t stream);

}  // namespace rtrdev
