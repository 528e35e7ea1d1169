/* rtr_mis.hip — rtr_emitter_hits: what a BRDF-sampled bounce ray that ends on a light contributes under the balance heuristic.
 *
 * k_emitter_hits: one ray per lane, and its body is rtr_mis_emitter of include/rtr_mis.h, the definition the host restatement
 * (rtr_host_emitter_hits) compiles too.  A streaming kernel: a lane reads its RtrRay and RtrHit as two 16-B pieces each, the first two
 * pieces of the RtrSurface of the vertex the ray left (position, kind, normal) and the first piece of that vertex's RtrBounce (pdf), and
 * writes its RtrEmitter as two 16-B stores — no LDS, no atomics, no scratch.  Only a lane whose hit is a triangle of a light goes on to
 * gather that triangle's record (four 16-B pieces of the scene's light-triangle table, found at lightTriFirst[customIndex] +
 * primitiveId as k_hit_surfaces finds it) and 32 B of its light's info; the ids are checked against the light table before anything is
 * read there.  Every record is written: a lane without a light hit stores 32 zero bytes.
 * POWER (rtr_emitter_hits_power; include/rtr_power.h): the pick density of the hit triangle comes from the scene's power table, two
 * 8-B gathers of a.cdf and its total, read only by a lane that has a light hit.  The uniform instantiation reads nothing of the table.
 */
#include <hip/hip_runtime.h>
#include "rtr_mis_launch.h"
#include "../../../include/rtr_mis.h"
#include "../../../include/rtr_power.h"

namespace rtrdev {

constexpr int kEmitterBlock = 256;

template <bool POWER>
__global__ __launch_bounds__(kEmitterBlock) void k_emitter_hits(EmitterArgs a) {
    const uint32_t k = blockIdx.x * kEmitterBlock + threadIdx.x;
    if (k >= a.n) return;
    const float4* __restrict__ hp = a.hits + 2 * (size_t)k;
    const float4 h0 = hp[0], h1 = hp[1];
    const uint32_t l = __float_as_uint(h0.w), prim = __float_as_uint(h1.x);
    RtrEmitter e;
    rtr_mis_emitter_zero(&e);
    if (l < a.numLights) {                                 /* a miss is 0xffffffff */
        const RtrAreaLightInfo* __restrict__ li = a.lights + l;
        if (prim < li->numTriangles) {
            const float4* __restrict__ rp = a.rays + 2 * (size_t)k;
            const float4* __restrict__ sp = a.prevSurfaces + 5 * (size_t)k;
            const float4 r0 = rp[0], r1 = rp[1];
            const float4 s0 = sp[0], s1 = sp[1];
            const float4 b0 = a.bounces[2 * (size_t)k];
            const uint32_t t = a.lightTriFirst[l] + prim;
            const float4* __restrict__ rec = a.lightTris + 4 * (size_t)t;
            const float4 c0 = rec[0], c1 = rec[1], c2 = rec[2], c3 = rec[3];
            RtrRay ray;
            ray.origin[0] = r0.x; ray.origin[1] = r0.y; ray.origin[2] = r0.z; ray.tmin = r0.w;
            ray.direction[0] = r1.x; ray.direction[1] = r1.y; ray.direction[2] = r1.z; ray.tmax = r1.w;
            RtrSurface sf{};
            sf.position[0] = s0.x; sf.position[1] = s0.y; sf.position[2] = s0.z; sf.kind = __float_as_uint(s0.w);
            sf.normal[0] = s1.x; sf.normal[1] = s1.y; sf.normal[2] = s1.z;
            RtrBounce b{};
            b.pdf = b0.w;
            const float recf[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
            const float col[3] = {li->color[0], li->color[1], li->color[2]};
            if (POWER) rtr_power_mis_emitter(&ray, h0.x, &sf, &b, recf, t, col, li->intensity, li->isTwoSided, rtr_power_ptri(a.cdf, a.tris, t), a.picks, &e);
            else rtr_mis_emitter(&ray, h0.x, &sf, &b, recf, t, col, li->intensity, li->isTwoSided, l < a.numAreaLights, a.tris, a.picks, &e);
        }
    }
    float4* __restrict__ o = a.out + 2 * (size_t)k;
    o[0] = make_float4(e.radiance[0], e.radiance[1], e.radiance[2], e.wBounce);
    o[1] = make_float4(e.lightPdf, e.dist, __uint_as_float(e.lightTri), __uint_as_float(e.kind));
}

hipError_t launch_emitter_hits(const EmitterArgs& a, hipStream_t s) {
    const dim3 grid((uint32_t)(((uint64_t)a.n + kEmitterBlock - 1) / kEmitterBlock));
    if (a.cdf) hipLaunchKernelGGL(k_emitter_hits<true>, grid, dim3(kEmitterBlock), 0, s, a);
    else hipLaunchKernelGGL(k_emitter_hits<false>, grid, dim3(kEmitterBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace rtrdev
