/* rtr_power.hip — power-proportional light picks for path vertices: the table build and rtr_pick_slots_power.  The rule is
 * include/rtr_power.h, the definition the host restatement (rtr_power_host.cpp) compiles too.  The power forms of the two MIS kernels
 * are instantiations of k_mis_pick_weights (kernels/rtr_query.hip) and k_emitter_hits (kernels/rtr_mis.hip), beside the helpers they call.
 *
 * THE TABLE BUILD, two plain launches, again whenever the light triangles or the light infos are rewritten.  k_power_weights, one lane
 * per light triangle: finds the triangle's light in lightTriFirst (the search picked_sample makes), writes pw_t as the bits of a float
 * and folds them into one word with an atomic maximum — non-negative floats order as their bits do, and a maximum does not depend on
 * the order it is formed in.  k_power_scan, ONE workgroup: quantises kPowerScanChunk triangles at a time against that maximum and
 * scans them in 64 bits through LDS, carrying the sum of the chunks before; it puts the maximum's word back to 0 for the next build.
 * Light tables are small (the bench scene has twelve triangles), and the sums are integers: any order of adding gives these words.
 *
 * k_pick_slots_power: one hit per lane, P picks in a loop, each one binary search of at most log2 Ttot dependent 8-B loads of cdf and
 * two more for the weight.  The table stays in global memory: the first steps of every lane's search read the same few words (one
 * request per wave), the rest of a table of the sizes above sits in the vector L1, and the kernel reads only its seeds beside them.
 * The slots and the weights go out as the lane draws them, P words each at the 4 P-byte lane stride.  No LDS, no atomics, no scratch.
 */
#include <hip/hip_runtime.h>
#include "rtr_power_launch.h"
#include "../../../include/rtr_power.h"

namespace rtrdev {

constexpr int kPowerBlock = 256;
static_assert(kPowerScanChunk == (uint32_t)kPowerBlock, "the scan covers one triangle per lane and pass");

__global__ __launch_bounds__(kPowerBlock) void k_power_weights(const float4* __restrict__ lightTris, const uint32_t* __restrict__ lightTriFirst,
                                                               const RtrAreaLightInfo* __restrict__ lights, uint32_t numLights, PowerTable tb) {
    const uint32_t t = blockIdx.x * kPowerBlock + threadIdx.x;
    if (t >= tb.numTris) return;
    uint32_t lo = 0u, hi = numLights;                      /* the last l with lightTriFirst[l] <= t: a light without triangles is passed over */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lightTriFirst[mid] <= t) lo = mid; else hi = mid;
    }
    const RtrAreaLightInfo* __restrict__ L = lights + lo;
    const float col[3] = {L->color[0], L->color[1], L->color[2]};
    const float pw = rtr_power_of(col, L->intensity, lightTris[4 * (size_t)t].w);
    const uint32_t bits = __float_as_uint(pw);             /* pw >= +0: the bits order as the floats do */
    tb.weights[t] = bits;
    if (bits != 0u) atomicMax(tb.maxBits, bits);
}

__global__ __launch_bounds__(kPowerBlock) void k_power_scan(PowerTable tb) {
    __shared__ uint64_t buf[kPowerBlock];
    const uint32_t tid = threadIdx.x;
    const float pwMax = __uint_as_float(*tb.maxBits);
    __syncthreads();                                       /* every lane has read the maximum before lane 0 clears it below */
    uint64_t carry = 0u;
    for (uint32_t base = 0u; base < tb.numTris; base += kPowerBlock) {
        const uint32_t t = base + tid;
        uint32_t w = 0u;
        if (t < tb.numTris) {
            w = rtr_power_weight(__uint_as_float(tb.weights[t]), pwMax);
            tb.weights[t] = w;
        }
        buf[tid] = w;
        __syncthreads();
        for (uint32_t off = 1u; off < (uint32_t)kPowerBlock; off <<= 1) {
            const uint64_t v = tid >= off ? buf[tid - off] : 0u;
            __syncthreads();
            buf[tid] += v;
            __syncthreads();
        }
        if (t < tb.numTris) tb.cdf[t] = carry + buf[tid];
        carry += buf[kPowerBlock - 1];
        __syncthreads();
    }
    if (tid == 0u) *tb.maxBits = 0u;
}

hipError_t launch_light_power(const float4* lightTris, const uint32_t* lightTriFirst, const RtrAreaLightInfo* lights, uint32_t numLights,
                              const PowerTable& t, hipStream_t s) {
    if (t.numTris == 0u || numLights == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_power_weights, dim3((t.numTris + kPowerBlock - 1) / kPowerBlock), dim3(kPowerBlock), 0, s, lightTris, lightTriFirst, lights, numLights, t);
    hipLaunchKernelGGL(k_power_scan, dim3(1), dim3(kPowerBlock), 0, s, t);
    return hipGetLastError();
}

__global__ __launch_bounds__(kPowerBlock) void k_pick_slots_power(PowerPickArgs a) {
    const uint32_t k = blockIdx.x * kPowerBlock + threadIdx.x;
    if (k >= a.n) return;
    const uint64_t* __restrict__ cdf = a.cdf;
    const uint32_t baseFrame = rtr_pick_base(a.seeds, k, a.width, a.spp) + a.frame;
    const uint32_t P = a.picks;
    for (uint32_t p = 0u; p < P; ++p) {
        const size_t at = (size_t)k * P + p;
        float w;
        a.outSlots[at] = rtr_power_pick(cdf, a.tris, a.numShadowRays, baseFrame, a.depth, p, P, &w);
        a.outWeights[at] = w;
    }
}

hipError_t launch_pick_slots_power(const PowerPickArgs& a, hipStream_t s) {
    if (a.picks == 0u || a.picks > RTR_PICK_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pick_slots_power, dim3((uint32_t)(((uint64_t)a.n + kPowerBlock - 1) / kPowerBlock)), dim3(kPowerBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace rtrdev
