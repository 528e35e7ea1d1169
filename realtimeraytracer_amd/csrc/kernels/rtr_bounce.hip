/* rtr_bounce.hip — rtr_bounce_rays: the BRDF-sampled continuation ray of each ray-query hit and its throughput weight.
 *
 * k_bounce_rays: one hit per lane, and its body is rtr_bounce_sample of include/rtr_bounce.h, the definition the host restatement
 * (rtr_host_bounce_rays) compiles too.  A streaming kernel: a lane reads its 80-B RtrSurface as five 16-B loads and its 32-B RtrRay as
 * two, and writes the next ray and the RtrBounce as four 16-B stores — 176 B per hit, no LDS, no atomics, no scratch, nothing of the
 * scene.  The records of neighbouring lanes are adjacent, so the loads and stores of a wave cover whole cache lines between them.
 * Every slot of every hit is written: a dead lane stores its zero records.
 */
#include <hip/hip_runtime.h>
#include "rtr_bounce_launch.h"
#include "../../../include/rtr_bounce.h"

namespace rtrdev {

constexpr int kBounceBlock = 256;

__global__ __launch_bounds__(kBounceBlock) void k_bounce_rays(BounceArgs a) {
    const uint32_t k = blockIdx.x * kBounceBlock + threadIdx.x;
    if (k >= a.n) return;
    const float4* __restrict__ rp = a.rays + 2 * (size_t)k;
    const float4* __restrict__ sp = a.surfaces + 5 * (size_t)k;
    const float4 r0 = rp[0], r1 = rp[1];
    const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3], s4 = sp[4];
    /* The sample reads 15 of the 28 words; left alone the compiler fetches just those, as dwordx3, dword and a dwordx4 at byte 44 of the
     * surface that straddles two 16-B pieces.  Every word counts as used here, so the records move as seven aligned 16-B loads; the
     * cache lines fetched are the same either way (the records are adjacent). */
    asm volatile("" ::"v"(r0.w), "v"(r1.x), "v"(r1.y), "v"(r1.z), "v"(r1.w), "v"(s1.w), "v"(s2.x), "v"(s2.y), "v"(s2.z), "v"(s4.x), "v"(s4.y), "v"(s4.z), "v"(s4.w));
    uint32_t base;
    if (a.seeds) base = a.seeds[k];
    else base = rtr_bounce_pixel_seed(k, a.params.width, a.params.spp);

    RtrRay ray;
    ray.origin[0] = r0.x; ray.origin[1] = r0.y; ray.origin[2] = r0.z; ray.tmin = r0.w;
    ray.direction[0] = r1.x; ray.direction[1] = r1.y; ray.direction[2] = r1.z; ray.tmax = r1.w;
    RtrSurface sf;
    sf.position[0] = s0.x; sf.position[1] = s0.y; sf.position[2] = s0.z; sf.kind = __float_as_uint(s0.w);
    sf.normal[0] = s1.x; sf.normal[1] = s1.y; sf.normal[2] = s1.z; sf.objectIndex = __float_as_uint(s1.w);
    sf.geomNormal[0] = s2.x; sf.geomNormal[1] = s2.y; sf.geomNormal[2] = s2.z; sf.metallic = s2.w;
    sf.color[0] = s3.x; sf.color[1] = s3.y; sf.color[2] = s3.z; sf.roughness = s3.w;
    sf.uv[0] = s4.x; sf.uv[1] = s4.y; sf._reserved[0] = 0u; sf._reserved[1] = 0u;

    RtrRay next;
    RtrBounce b;
    rtr_bounce_sample(&ray, &sf, base, &a.params, &next, &b);

    float4* __restrict__ orp = a.outRays + 2 * (size_t)k;
    float4* __restrict__ obp = a.outBounce + 2 * (size_t)k;
    orp[0] = make_float4(next.origin[0], next.origin[1], next.origin[2], next.tmin);
    orp[1] = make_float4(next.direction[0], next.direction[1], next.direction[2], next.tmax);
    obp[0] = make_float4(b.weight[0], b.weight[1], b.weight[2], b.pdf);
    obp[1] = make_float4(__uint_as_float(b.lobe), b.pSpecular, 0.0f, 0.0f);
}

hipError_t launch_bounce_rays(const BounceArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_bounce_rays, dim3((uint32_t)(((uint64_t)a.n + kBounceBlock - 1) / kBounceBlock)), dim3(kBounceBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace rtrdev
