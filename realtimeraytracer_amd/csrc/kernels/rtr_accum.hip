/* rtr_accum.hip — rtr_accumulate_paths and rtr_gather_records: a vertex's radiance added to the image at the paths' ids with the
 * throughput after its bounce, and records gathered by row.
 *
 * One launch each, streaming kernels like k_compact_scatter: 256-lane workgroups, no LDS, no atomics, no scene memory.
 *   k_accumulate_paths  one path per lane.  A lane reads the FIRST 16 B of its RtrRadiance (shadowed, kind), the first 16 B of its
 *                       RtrEmitter / RtrSkyEscape only when its kind and the flags ask for it, the 16-B sky sum and the first 16 B of
 *                       its RtrBounce, each as one float4 load; its throughput and its image rows as words at their strides.  The rule
 *                       is include/rtr_accum.h, which the host restatement (rtr_host_accumulate_paths) compiles too.  Which optional
 *                       arrays there are is a UNIFORM branch on a kernel argument (a scalar compare and branch per wave), not a
 *                       template parameter: five optional arrays would be 32 instantiations of a kernel that waits for memory.
 *   k_gather_records    one lane per 16-B chunk of an output record (the record size a multiple of 16, src and out 16-B aligned), else
 *                       one lane per word.  The lanes of a workgroup cover consecutive units of consecutive records, so the stores
 *                       coalesce; the loads are whole records wherever rows[] points.
 * About 130 B per path with every optional array (rtr_accumulate_paths), 2 x recordBytes + 4 per row (rtr_gather_records).
 */
#include <hip/hip_runtime.h>
#include "rtr_accum_launch.h"
#include "../../../include/rtr_accum.h"

namespace rtrdev {

constexpr int kAccumBlock = 256;

__global__ __launch_bounds__(kAccumBlock) void k_accumulate_paths(AccumArgs a) {
    const uint32_t k = blockIdx.x * kAccumBlock + threadIdx.x;
    if (k >= a.n) return;
    const float4 r = a.radiance[3 * (size_t)k];
    const uint32_t kind = __float_as_uint(r.w), flags = a.params.flags;
    float rad[3] = {r.x, r.y, r.z};
    if (rtr_accum_from_emitters(kind, flags)) {
        rad[0] = 0.0f; rad[1] = 0.0f; rad[2] = 0.0f;
        if (a.emitters) { const float4 e = a.emitters[2 * (size_t)k]; rad[0] = e.x; rad[1] = e.y; rad[2] = e.z; }
    }
    if (rtr_accum_from_escapes(kind, flags)) {
        rad[0] = 0.0f; rad[1] = 0.0f; rad[2] = 0.0f;
        if (a.escapes) { const float4 e = a.escapes[2 * (size_t)k]; rad[0] = e.x; rad[1] = e.y; rad[2] = e.z; }
    }
    const float* tp = reinterpret_cast<const float*>(a.throughput + (size_t)k * a.params.throughputStrideBytes);
    const float T[3] = {tp[0], tp[1], tp[2]};         /* read before outThroughput, which may be this array, is written */
    float sky[3] = {0.0f, 0.0f, 0.0f}, term[3];
    if (a.skySums) { const float4 s = a.skySums[k]; sky[0] = s.x; sky[1] = s.y; sky[2] = s.z; }
    rtr_accum_term(T, rad, a.skySums != nullptr, sky, term);
    const uint32_t id = a.pathIds ? a.pathIds[k] : k;
    if (rtr_accum_slot_ok(id, a.params.numSlots)) {
        const size_t at = (size_t)id * a.params.imageStrideBytes;
        float* ap = reinterpret_cast<float*>(a.accum + at);
        const float s0 = ap[0] + term[0], s1 = ap[1] + term[1], s2 = ap[2] + term[2];
        ap[0] = s0; ap[1] = s1; ap[2] = s2;
        if (a.outTerm) {
            float* op = reinterpret_cast<float*>(a.outTerm + at);
            op[0] = term[0]; op[1] = term[1]; op[2] = term[2];
        }
    }
    if (a.bounces) {                                   /* with outThroughput: the entry points check the pair */
        const float4 b = a.bounces[2 * (size_t)k];
        const float w[3] = {b.x, b.y, b.z};
        float outT[3];
        rtr_accum_next_throughput(T, w, outT);
        float* otp = a.outThroughput + 3 * (size_t)k;
        otp[0] = outT[0]; otp[1] = outT[1]; otp[2] = outT[2];
    }
}

/* Unit: float4 (16-B chunks) or uint32_t (words).  unitsPerRecord <= 64; the workgroup's first unit is found once per wave in scalar
 * registers, a lane's row and unit from it with 32-bit arithmetic. */
template <class Unit>
__global__ __launch_bounds__(kAccumBlock) void k_gather_records(GatherArgs a, uint32_t unitsPerRecord) {
    const uint64_t first = (uint64_t)blockIdx.x * kAccumBlock;
    const uint64_t row0 = first / unitsPerRecord;
    const uint32_t t = (uint32_t)(first - row0 * unitsPerRecord) + threadIdx.x;       /* < 64 + 256 */
    const uint64_t j = row0 + t / unitsPerRecord;
    const uint32_t u = t % unitsPerRecord;
    if (j >= a.numRows) return;
    const uint32_t row = a.rows[j];
    Unit v{};
    if (rtr_gather_row_ok(row, a.numSrc)) v = reinterpret_cast<const Unit*>(a.src + (size_t)row * a.recordBytes)[u];
    reinterpret_cast<Unit*>(a.out + (size_t)j * a.recordBytes)[u] = v;
}

hipError_t launch_accumulate_paths(const AccumArgs& a, hipStream_t s) {
    const uint32_t groups = (uint32_t)(((uint64_t)a.n + kAccumBlock - 1) / kAccumBlock);
    hipLaunchKernelGGL(k_accumulate_paths, dim3(groups), dim3(kAccumBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gather_records(const GatherArgs& a, hipStream_t s) {
    const bool wide = (a.recordBytes & 15u) == 0u && (((uintptr_t)a.src | (uintptr_t)a.out) & 15u) == 0u;
    const uint32_t units = a.recordBytes / (wide ? 16u : 4u);
    const uint32_t groups = (uint32_t)(((uint64_t)a.numRows * units + kAccumBlock - 1) / kAccumBlock);     /* at most 2^30 */
    if (wide) hipLaunchKernelGGL(k_gather_records<float4>, dim3(groups), dim3(kAccumBlock), 0, s, a, units);
    else hipLaunchKernelGGL(k_gather_records<uint32_t>, dim3(groups), dim3(kAccumBlock), 0, s, a, units);
    return hipGetLastError();
}

}  // namespace rtrdev
