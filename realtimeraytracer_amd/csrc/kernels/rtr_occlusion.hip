/* rtr_occlusion.hip — the queued occlusion query (include/rtr.h: rtr_trace_occlusion): the renderer's any-hit machinery for rays the
 * caller supplies.
 *
 * rtr_trace_rays(RTR_QUERY_ANY) answers an occlusion ray with one lane of a one-shot launch over the BVH2 (k_query).  The renderer
 * answers its own shadow rays with k_shadow_trace4: persistent waves that refill finished lanes from a queue binned by direction
 * octant, over the 4-wide records, the top of the tree in LDS, the far-exit-first child order.  This file opens that walk to RtrRay
 * arrays, in the renderer's three stages:
 *   k_occlusion_gen   (here) classifies every ray — a null ray, a ray whose origin or direction is not finite or whose direction is
 *                     zero, a ray with !(tmax > tmin) is "not occluded" now and costs no walk — and appends the INDEX of every other
 *                     ray to the queue, laid out octant by octant inside the workgroup's chunk and cut into batches for the
 *                     per-(octant, XCD) batch lists, as k_shadow_gen_oct does (one reservation per workgroup and list).  Indices, not
 *                     rays: the rays are already in memory as 32-B records, which the walk gathers at refill;
 *   k_shadow_trace4   (rtr_kernels.hip, its CALLER form: launch_occlusion_walk) drains the lists;
 *   k_query_tail      (rtr_query.hip) finishes over the BVH2 the rays that outgrew the LDS stack.
 * Any-hit is a pure function of the ray and the triangles and the 4-wide boxes are conservative, so the bytes are rtr_trace_rays'.
 */
#include "rtr_query.h"

namespace rtrdev {

constexpr uint32_t kOccGenBlock = 512;                                     /* as k_shadow_gen_oct: two workgroups per CU */
constexpr uint32_t kOccGenPerLane = kOcclusionGenRays / kOccGenBlock;      /* rays per lane, kOccGenBlock apart: a wave's loads stay contiguous */
static_assert(kOccGenPerLane == 8 && kOccGenPerLane * kOccGenBlock == kOcclusionGenRays, "a lane keeps its rays' 4-bit codes in one register");
constexpr uint32_t kOccNoWalk = 8u;                                        /* code of a ray that is not queued (octants are 0..7) */

/* ray k's code: its direction octant (signs of the direction as given: the octant only sorts the queue, the walk takes its own from the
 * ray it loads), or kOccNoWalk.  wellFormed: origin and direction finite, direction not zero — query_ray()'s rule (rtr_query_device.h). */
__device__ __forceinline__ uint32_t occlusion_code(const float4* __restrict__ rays, uint64_t k, bool& wellFormed) {
    const float4 a = rays[2 * k], b = rays[2 * k + 1];
    wellFormed = __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) &&
                 __builtin_isfinite(b.x) && __builtin_isfinite(b.y) && __builtin_isfinite(b.z) && (b.x != 0.0f || b.y != 0.0f || b.z != 0.0f);
    if (!wellFormed || !(b.w > a.w)) return kOccNoWalk;
    return (b.x < 0.f ? 1u : 0u) | (b.y < 0.f ? 2u : 0u) | (b.z < 0.f ? 4u : 0u);
}

/* STATS: the well-formed rays that are not queued (an empty interval) are counted here; the walk counts the ones it takes, so the
 * query's numRays is what the renderer's counters call shadow rays — every ray that was sent, null slots excluded.
 * MASKED (rtr_trace_occlusion_masked): a ray whose effective cull mask — rm.cullMask & its byte of rm.rayMasks — is 0 sees no instance:
 * it is "not occluded" now, is not queued, and is counted as a ray with an empty interval is. */
template <bool STATS, bool MASKED = false>
__global__ __launch_bounds__(kOccGenBlock) void k_occlusion_gen(OcclusionArgs oa, Counters* stats, RayMaskArgs rm) {
    constexpr uint32_t kWaves = kOccGenBlock / 64;
    __shared__ uint32_t s_tot[kWaves][8], s_run[kWaves][8];
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t k0 = (uint64_t)blockIdx.x * kOcclusionGenRays + threadIdx.x;
    uint32_t codes = 0, unqueued = 0;
    unsigned long long lo = 0ull, hi = 0ull;          /* eight 16-bit counters: octants 0-3, 4-7 (a wave's total is at most 512) */
#pragma unroll
    for (uint32_t j = 0; j < kOccGenPerLane; ++j) {
        const uint64_t k = k0 + (uint64_t)j * kOccGenBlock;
        uint32_t code = kOccNoWalk;
        if (k < oa.n) {
            bool wellFormed;
            code = occlusion_code(oa.rays, k, wellFormed);
            if (MASKED && (rm.cullMask & (rm.rayMasks ? (uint32_t)rm.rayMasks[k] : 0xffu)) == 0u) code = kOccNoWalk;
            if (STATS && wellFormed && code == kOccNoWalk) ++unqueued;
        }
        codes |= code << (4u * j);
        if (code < 4u) lo += 1ull << (code * 16u);
        else if (code < 8u) hi += 1ull << ((code - 4u) * 16u);
    }
    unsigned long long tlo = lo, thi = hi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { tlo += __shfl_xor(tlo, o); thi += __shfl_xor(thi, o); }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (uint32_t o = 0; o < 8; ++o) s_tot[wave][o] = (uint32_t)(((o < 4 ? tlo : thi) >> ((o & 3u) * 16u)) & 0xffffull);
    }
    if (STATS) {
        uint32_t u = unqueued;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o);
        if ((threadIdx.x & 63u) == 0 && u) { atomicAdd(&stats->rays, (unsigned long long)u); atomicAdd(&stats->shadow, (unsigned long long)u); }
    }
    __syncthreads();
    if (threadIdx.x < kQueueLists) {
        /* the first wave, one lane per (octant, list): the workgroup's chunk of the queue (lane 0) and the places of its batches in the 64
         * lists are reserved together — one device-scope round trip — then the runs are laid inside the chunk (k_shadow_gen_oct's scheme) */
        const uint32_t o = threadIdx.x / kQueueRegions, x = threadIdx.x % kQueueRegions;
        uint32_t before = 0, len = 0, total = 0;
#pragma unroll
        for (uint32_t oo = 0; oo < 8; ++oo) {
            uint32_t t = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) t += s_tot[w][oo];
            before += oo < o ? t : 0u;
            len = oo == o ? t : len;
            total += t;
        }
        const uint32_t kB = oa.batch;
        const uint32_t nb = (len + kB - 1) / kB;
        const uint32_t b0 = (x + kQueueRegions - blockIdx.x % kQueueRegions) % kQueueRegions;     /* first batch that goes to list x */
        const uint32_t cnt = b0 < nb ? (nb - b0 + kQueueRegions - 1) / kQueueRegions : 0u;
        uint32_t at = 0, pos = 0;
        if (threadIdx.x == 0 && total) at = atomicAdd(oa.ctrl + kQueueLenWord, total);
        if (cnt) pos = atomicAdd(oa.ctrl + kQueueListLens + threadIdx.x, cnt);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)at) + before;
        if (x == 0) {
            uint32_t c = first;
            for (uint32_t w = 0; w < kWaves; ++w) { s_run[w][o] = c; c += s_tot[w][o]; }
        }
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t f = (b0 + j * kQueueRegions) * kB;
            if (pos + j < oa.listStride)              /* occlusion_list_stride() bounds it; never past the list whatever the bound */
                oa.lists[(size_t)threadIdx.x * oa.listStride + pos + j] = make_uint2(first + f, len - f < kB ? len - f : kB);
        }
    }
    __syncthreads();
    typedef volatile __attribute__((address_space(3))) uint32_t* lds_word;      /* keeps the accesses ds_read / ds_write */
    const lds_word run = (lds_word)&s_run[wave][0];
#pragma unroll
    for (uint32_t j = 0; j < kOccGenPerLane; ++j) {
        const uint32_t code = (codes >> (4u * j)) & 15u;
        const uint64_t k = k0 + (uint64_t)j * kOccGenBlock;
        unsigned long long rem = __ballot(code < kOccNoWalk);
        while (rem != 0ull) {                            /* one round per octant present among the wave's 64 consecutive rays */
            const uint32_t oo = (uint32_t)__builtin_amdgcn_readlane((int)code, (int)__ffsll((long long)rem) - 1);
            const unsigned long long mo = __ballot(code == oo);
            if (code == oo) {
                const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(mo >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mo, 0u));
                const uint32_t at = run[oo];
                if (prefix == 0) run[oo] = at + (uint32_t)__popcll(mo);
                if (at + prefix < oa.n) oa.queue[at + prefix] = (uint32_t)k;
            }
            rem &= ~mo;
        }
    }
}

hipError_t launch_occlusion(const DeviceScene& sc, const OcclusionArgs& oa, const Tunables& tun, bool alpha, int32_t* spill, Counters* stats,
                            hipStream_t s, uint32_t numCus, const RayMaskArgs& rm) {
    const uint32_t genBlocks = (uint32_t)(((uint64_t)oa.n + kOcclusionGenRays - 1) / kOcclusionGenRays);
    if (rm.masked) {
        if (stats) hipLaunchKernelGGL((k_occlusion_gen<true, true>), dim3(genBlocks), dim3(kOccGenBlock), 0, s, oa, stats, rm);
        else hipLaunchKernelGGL((k_occlusion_gen<false, true>), dim3(genBlocks), dim3(kOccGenBlock), 0, s, oa, stats, rm);
    } else if (stats) hipLaunchKernelGGL(k_occlusion_gen<true>, dim3(genBlocks), dim3(kOccGenBlock), 0, s, oa, stats, rm);
    else hipLaunchKernelGGL(k_occlusion_gen<false>, dim3(genBlocks), dim3(kOccGenBlock), 0, s, oa, stats, rm);
    hipError_t e = launch_occlusion_walk(sc, oa, tun, alpha, stats, s, numCus, rm);
    if (e != hipSuccess) return e;
    QueryArgs qa{};
    qa.rays = oa.rays; qa.occluded = oa.occluded; qa.n = oa.n;
    qa.redoCap = oa.overflowCap; qa.ctrl = oa.overflow; qa.redoList = oa.overflow + 1; qa.spill = spill;
    static_assert(kQueryRedoWord == 0, "the walk's overflow count is the tail's redo count");
    return launch_query_tail_any(sc, qa, alpha, stats, s, rm);
}

}  // namespace rtrdev
