/* rtr_query_device.h — device helpers the ray-query kernels share (kernels/rtr_query.hip, kernels/rtr_multihit.hip): how a ray and its
 * cull mask are read, and how a wave appends its abandoned rays to the context's redo list. */
#pragma once
#include "rtr_query.h"

namespace rtrdev {

/* ray k: two 16-B loads.  false: a degenerate ray (origin or direction not finite, or a zero direction), which is a miss */
__device__ __forceinline__ bool query_ray(const float4* __restrict__ rays, uint32_t k, rtr_v3& o, rtr_v3& d, float& tmin, float& tmax) {
    const float4 a = rays[2 * (size_t)k], b = rays[2 * (size_t)k + 1];
    o = rtr_mk(a.x, a.y, a.z); tmin = a.w;
    d = rtr_mk(b.x, b.y, b.z); tmax = b.w;
    const bool finite = __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) &&
                        __builtin_isfinite(b.x) && __builtin_isfinite(b.y) && __builtin_isfinite(b.z);
    return finite && (b.x != 0.0f || b.y != 0.0f || b.z != 0.0f);
}

/* ray k's effective cull mask, in the bits the records keep theirs in (trace()'s rayMask8); 0: nothing exists for the ray */
__device__ __forceinline__ uint32_t query_ray_mask8(const RayMaskArgs& rm, uint32_t k) {
    return (rm.cullMask & (rm.rayMasks ? (uint32_t)rm.rayMasks[k] : 0xffu)) << kTriMaskShift;
}

/* the abandoned rays of the wave (over: this lane's ray k is one) take consecutive entries of the redo list: one atomic per wave.  The
 * count in ctrl may pass redoCap; the tail kernels then find the rays by their sentinel */
__device__ __forceinline__ void redo_append(uint32_t* ctrl, uint32_t* redoList, uint32_t redoCap, bool over, uint32_t k) {
    const unsigned long long m = __ballot(over);
    if (m != 0ull) {
        const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        uint32_t base = 0;
        if (over && prefix == 0u) base = atomicAdd(ctrl + kQueryRedoWord, (uint32_t)__popcll(m));
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, __ffsll((long long)m) - 1);
        if (over && base + prefix < redoCap) redoList[base + prefix] = k;
    }
}

}  // namespace rtrdev
