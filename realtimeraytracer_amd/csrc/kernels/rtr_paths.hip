/* rtr_paths.hip — rtr_compact_paths: the live paths of a wavefront gathered to the front in their order, the rest cleared.
 *
 * Three launches on the stream, and no workgroup ever waits for another (no look-back, no flag, no atomic):
 *   k_compact_count    one path per lane, 256-lane workgroups.  A lane decides rtr_path_survive of include/rtr_paths.h, the definition
 *                      the host restatement (rtr_host_compact_paths) compiles too; the wave's __ballot goes to the scratch, 1 bit per
 *                      path, its popcount to LDS and the workgroup's total to the scratch.
 *   k_compact_scan     ONE workgroup: the exclusive scan of the workgroup totals, in place, 1024 totals per turn of a loop with a running
 *                      carry — right for every numPaths below 2^32 (2^24 totals then).  Writes *outCount.
 *   k_compact_scatter  a survivor's slot = its workgroup's offset + the popcounts of the waves before its own + its mbcnt prefix in the
 *                      STORED ballot: who lives is decided once, by k_compact_count.  A survivor moves its ray as two 16-B loads and two
 *                      16-B stores, its throughput (rtr_path_survive again: the same bits), seed and id as words.  Lane k with
 *                      k >= count clears tail slot k; survivors' slots are below count, so no slot is written twice.
 * Streaming kernels: no scene memory, about 150 B per path between them.
 */
#include <hip/hip_runtime.h>
#include "rtr_paths_launch.h"
#include "../../../include/rtr_paths.h"

namespace rtrdev {

constexpr int kCompactBlock = 256;
constexpr int kCompactWaves = kCompactBlock / 64;
constexpr int kScanPerThread = 4;
constexpr uint32_t kScanChunk = kCompactBlock * kScanPerThread;

/* path k's survival and, for a survivor, its outgoing throughput */
__device__ __forceinline__ int compact_decide(const CompactArgs& a, uint32_t k, float4* r0, float4* r1, float outT[3]) {
    const float4* __restrict__ rp = a.rays + 2 * (size_t)k;
    *r0 = rp[0]; *r1 = rp[1];
    const float* __restrict__ tp = reinterpret_cast<const float*>(a.throughput + (size_t)k * a.params.throughputStrideBytes);
    const float T[3] = {tp[0], tp[1], tp[2]};
    const uint32_t seed = a.seeds ? a.seeds[k] : 0u;
    RtrRay ray;
    ray.origin[0] = r0->x; ray.origin[1] = r0->y; ray.origin[2] = r0->z; ray.tmin = r0->w;
    ray.direction[0] = r1->x; ray.direction[1] = r1->y; ray.direction[2] = r1->z; ray.tmax = r1->w;
    return rtr_path_survive(&ray, T, seed, &a.params, outT);
}

__global__ __launch_bounds__(kCompactBlock) void k_compact_count(CompactArgs a) {
    __shared__ uint32_t waveTotal[kCompactWaves];
    const uint32_t k = blockIdx.x * kCompactBlock + threadIdx.x;
    int live = 0;
    if (k < a.n) {
        float4 r0, r1;
        float outT[3];
        live = compact_decide(a, k, &r0, &r1, outT);
    }
    const unsigned long long b = __ballot(live);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0u) {
        a.ballots[(size_t)blockIdx.x * kCompactWaves + wave] = b;      /* every wave of every workgroup writes its own, the padding of the last too */
        waveTotal[wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0u) a.groupTotals[blockIdx.x] = waveTotal[0] + waveTotal[1] + waveTotal[2] + waveTotal[3];
}

__global__ __launch_bounds__(kCompactBlock) void k_compact_scan(uint32_t* __restrict__ totals, uint32_t numGroups, uint32_t* __restrict__ outCount) {
    __shared__ uint32_t waveSum[kCompactWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t carry = 0u;                                               /* survivors before this chunk: at most numPaths, fits */
    for (uint32_t base = 0u; base < numGroups; base += kScanChunk) {   /* numGroups <= 2^24: base cannot wrap */
        const uint32_t i0 = base + threadIdx.x * kScanPerThread;
        uint32_t v[kScanPerThread], s = 0u;
        for (int j = 0; j < kScanPerThread; ++j) {
            v[j] = i0 + j < numGroups ? totals[i0 + j] : 0u;
            s += v[j];
        }
        uint32_t inc = s;                                              /* inclusive scan over the wave */
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63u) waveSum[wave] = inc;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0u; w < (uint32_t)kCompactWaves; ++w) {
            const uint32_t x = waveSum[w];
            before += w < wave ? x : 0u;
            total += x;
        }
        uint32_t ex = carry + before + (inc - s);
        for (int j = 0; j < kScanPerThread; ++j)
            if (i0 + j < numGroups) { totals[i0 + j] = ex; ex += v[j]; }
        carry += total;
        __syncthreads();                                               /* waveSum is written again by the next turn */
    }
    if (threadIdx.x == 0u) *outCount = carry;
}

__global__ __launch_bounds__(kCompactBlock) void k_compact_scatter(CompactArgs a) {
    const uint32_t k = blockIdx.x * kCompactBlock + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long* __restrict__ gb = a.ballots + (size_t)blockIdx.x * kCompactWaves;
    const unsigned long long b0 = gb[0], b1 = gb[1], b2 = gb[2], b3 = gb[3];
    const unsigned long long mine = wave == 0u ? b0 : (wave == 1u ? b1 : (wave == 2u ? b2 : b3));
    const uint32_t count = *a.outCount;
    if ((mine >> lane) & 1ull) {
        uint32_t slot = a.groupTotals[blockIdx.x];
        slot += wave > 0u ? (uint32_t)__popcll(b0) : 0u;
        slot += wave > 1u ? (uint32_t)__popcll(b1) : 0u;
        slot += wave > 2u ? (uint32_t)__popcll(b2) : 0u;
        slot += __builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
        float4 r0, r1;
        float outT[3];
        compact_decide(a, k, &r0, &r1, outT);                          /* the stored ballot decided; this is the survivor's outT */
        if (slot < count) {                                            /* always: the guard keeps a store inside the arrays whatever the scratch held */
            float4* __restrict__ orp = a.outRays + 2 * (size_t)slot;
            orp[0] = r0; orp[1] = r1;
            float* __restrict__ otp = a.outThroughput + 3 * (size_t)slot;
            otp[0] = outT[0]; otp[1] = outT[1]; otp[2] = outT[2];
            if (a.outSeeds) a.outSeeds[slot] = a.seeds[k];
            a.outPathIds[slot] = a.pathIds ? a.pathIds[k] : k;
        }
    }
    if (k >= count) {
        float4* __restrict__ orp = a.outRays + 2 * (size_t)k;
        orp[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); orp[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float* __restrict__ otp = a.outThroughput + 3 * (size_t)k;
        otp[0] = 0.0f; otp[1] = 0.0f; otp[2] = 0.0f;
        if (a.outSeeds) a.outSeeds[k] = 0u;
        a.outPathIds[k] = RTR_PATH_NONE;
    }
}

hipError_t launch_compact_paths(const CompactArgs& a, hipStream_t s) {
    const uint32_t groups = (uint32_t)(((uint64_t)a.n + kCompactBlock - 1) / kCompactBlock);
    hipLaunchKernelGGL(k_compact_count, dim3(groups), dim3(kCompactBlock), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(kCompactBlock), 0, s, a.groupTotals, groups, a.outCount);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compact_scatter, dim3(groups), dim3(kCompactBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace rtrdev
