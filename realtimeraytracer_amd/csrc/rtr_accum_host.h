/* rtr_accum_host.h — what the device and host entry points of rtr_accumulate_paths and rtr_gather_records share (internal to
 * librtr_hip.so). */
#pragma once
#include "rtr_arg_check.h"

namespace rtrdev {

/* every array of one rtr_accumulate_paths call */
struct AccumCall {
    const RtrRadiance* radiance; const float* throughput; const uint32_t* pathIds; const RtrEmitter* emitters; const RtrSkyEscape* escapes;
    const float* skySums; const RtrBounce* bounces; uint32_t n; const rtr_accum_params* params;
    const float* accum; const float* outTerm; const float* outThroughput;
};

/* The argument checks of rtr_accumulate_paths[_async] and rtr_host_accumulate_paths, which need no device (as rtr_arg_check.h returns
 * them).  Not called for numPaths == 0. */
int accum_check_args(const char* who, const AccumCall& c);

/* The same for rtr_gather_records[_async] and rtr_host_gather_records.  Not called for numRows == 0. */
int gather_check_args(const char* who, const void* src, uint32_t recordBytes, uint32_t numSrc, const uint32_t* rows, uint32_t numRows, const void* out);

}  // namespace rtrdev
