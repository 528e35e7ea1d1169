/* rtr_paths_host.h — what rtr_compact_paths' device and host entry points share (internal to librtr_hip.so). */
#pragma once
#include "rtr_arg_check.h"

namespace rtrdev {

/* every array of one rtr_compact_paths call; scratch / scratchNeed are null / 0 for the host form, which has none */
struct CompactCall {
    const RtrRay* rays; const float* throughput; const uint32_t* seeds; const uint32_t* pathIds;
    uint32_t n; const rtr_compact_params* params;
    const void* scratch; size_t scratchBytes, scratchNeed; bool wantsScratch;
    const RtrRay* outRays; const float* outThroughput; const uint32_t* outSeeds; const uint32_t* outPathIds; const uint32_t* outCount;
};

/* The argument checks of rtr_compact_paths[_async] and rtr_host_compact_paths, which need no device (as rtr_arg_check.h returns them).
 * Not called for numPaths == 0. */
int compact_check_args(const char* who, const CompactCall& c);

/* what rtr_compact_scratch_bytes returns: per 256-path workgroup four 64-bit ballots and one 32-bit total, each array rounded to 16 B */
size_t compact_scratch_bytes(uint32_t numPaths);

}  // namespace rtrdev
