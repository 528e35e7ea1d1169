/* rtr_sky.hip — sky importance sampling for path vertices: the table build, rtr_sky_rays, rtr_shade_sky and rtr_sky_hits.  The rule is
 * include/rtr_sky.h, the definition the host restatement (rtr_sky_host.cpp) compiles too.
 *
 * THE TABLE BUILD, once per scene, three plain launches: k_sky_weights, one lane per cell, reads the 3 x 3 neighbourhood of texels and
 * writes the cell's integer weight (rtr_sky_weight); k_sky_rows, one wave per row, scans the row in place, 64 cells at a time with the
 * carry of the pieces before; k_sky_marginal, one workgroup, scans the row totals in 64 bits.  The sums are integers: any order of
 * adding gives these words.
 *
 * k_sky_rays: one hit per lane, S samples in a loop, each two dependent binary searches.  The row search goes through the marginal sums,
 * which the workgroup stages in LDS once (8 B per row, up to kSkyLdsRows rows = 32 KiB; the reads stay ds_read through an address-space-3
 * pointer); a taller table is searched in global memory (LDS == false).  The column search is at most log2 W dependent 4-B loads of one
 * row's sums, 4 B per texel of L2.  A lane reads its RtrRay and RtrSurface as seven 16-B pieces and writes each sample's ray and record as
 * four 16-B stores; every slot of every hit is written.
 *
 * k_shade_sky and k_sky_hits are streaming kernels, one record per lane, no LDS, no atomics.  k_sky_hits reads the surface and bounce
 * records only at a miss, as k_emitter_hits gathers only at a light.
 */
#include <hip/hip_runtime.h>
#include "rtr_sky_launch.h"

namespace rtrdev {

constexpr int kSkyBlock = 256;

__global__ __launch_bounds__(kSkyBlock) void k_sky_weights(rtr_sky_source sky, uint32_t* __restrict__ rows, uint32_t W, uint32_t H) {
    const uint64_t i = (uint64_t)blockIdx.x * kSkyBlock + threadIdx.x;
    if (i >= (uint64_t)W * H) return;
    rows[i] = rtr_sky_weight(&sky, (uint32_t)(i % W), (uint32_t)(i / W));
}

__global__ __launch_bounds__(kSkyBlock) void k_sky_rows(uint32_t* __restrict__ rows, uint32_t W, uint32_t H) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t y = blockIdx.x * (kSkyBlock / 64) + (threadIdx.x >> 6);
    if (y >= H) return;                                    /* the whole wave */
    uint32_t* __restrict__ row = rows + (size_t)y * W;
    uint32_t carry = 0u;
    for (uint32_t x0 = 0u; x0 < W; x0 += 64u) {
        const uint32_t x = x0 + lane;
        uint32_t v = x < W ? row[x] : 0u;
        for (uint32_t off = 1u; off < 64u; off <<= 1) {
            const uint32_t t = __shfl_up(v, off, 64);
            if (lane >= off) v += t;
        }
        v += carry;
        if (x < W) row[x] = v;
        carry = __shfl(v, 63, 64);
    }
}

__global__ __launch_bounds__(kSkyBlock) void k_sky_marginal(const uint32_t* __restrict__ rows, uint64_t* __restrict__ marginal, uint32_t W, uint32_t H) {
    __shared__ uint64_t buf[kSkyBlock];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0u;
    for (uint32_t base = 0u; base < H; base += kSkyBlock) {
        const uint32_t y = base + tid;
        buf[tid] = y < H ? (uint64_t)rows[(size_t)y * W + (W - 1u)] : 0u;
        __syncthreads();
        for (uint32_t off = 1u; off < kSkyBlock; off <<= 1) {
            const uint64_t t = tid >= off ? buf[tid - off] : 0u;
            __syncthreads();
            buf[tid] += t;
            __syncthreads();
        }
        if (y < H) marginal[y] = carry + buf[tid];
        carry += buf[kSkyBlock - 1];
        __syncthreads();
    }
}

hipError_t launch_sky_table(const rtr_sky_source& sky, uint32_t* rows, uint64_t* marginal, hipStream_t s) {
    const uint32_t W = rtr_sky_table_width(&sky), H = rtr_sky_table_height(&sky);
    const uint64_t cells = (uint64_t)W * H;
    hipLaunchKernelGGL(k_sky_weights, dim3((uint32_t)((cells + kSkyBlock - 1) / kSkyBlock)), dim3(kSkyBlock), 0, s, sky, rows, W, H);
    hipLaunchKernelGGL(k_sky_rows, dim3((H + kSkyBlock / 64 - 1) / (kSkyBlock / 64)), dim3(kSkyBlock), 0, s, rows, W, H);
    hipLaunchKernelGGL(k_sky_marginal, dim3(1), dim3(kSkyBlock), 0, s, rows, marginal, W, H);
    return hipGetLastError();
}

template <bool LDS>
__global__ __launch_bounds__(kSkyBlock) void k_sky_rays(SkyRaysArgs a) {
    extern __shared__ uint64_t s_marginal[];
    typedef __attribute__((address_space(3))) uint64_t* lds_u64;      /* keeps the accesses ds_read / ds_write */
    const lds_u64 staged = (lds_u64)s_marginal;
    const rtr_sky_table& t = a.sd.table;
    const uint32_t H = t.height;
    if (LDS) {
        for (uint32_t y = threadIdx.x; y < H; y += kSkyBlock) staged[y] = t.marginal[y];
        __syncthreads();
    }
    const uint32_t k = blockIdx.x * kSkyBlock + threadIdx.x;
    if (k >= a.n) return;
    const float4* __restrict__ rp = a.rays + 2 * (size_t)k;
    const float4* __restrict__ sp = a.surfaces + 5 * (size_t)k;
    const float4 r0 = rp[0];
    const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
    RtrRay ray;
    ray.origin[0] = r0.x; ray.origin[1] = r0.y; ray.origin[2] = r0.z; ray.tmin = r0.w;
    ray.direction[0] = ray.direction[1] = ray.direction[2] = 0.0f; ray.tmax = 0.0f;      /* the view vector comes from the origin */
    RtrSurface sf{};
    sf.position[0] = s0.x; sf.position[1] = s0.y; sf.position[2] = s0.z; sf.kind = __float_as_uint(s0.w);
    sf.normal[0] = s1.x; sf.normal[1] = s1.y; sf.normal[2] = s1.z; sf.objectIndex = __float_as_uint(s1.w);
    sf.geomNormal[0] = s2.x; sf.geomNormal[1] = s2.y; sf.geomNormal[2] = s2.z; sf.metallic = s2.w;
    sf.color[0] = s3.x; sf.color[1] = s3.y; sf.color[2] = s3.z; sf.roughness = s3.w;

    const uint32_t base = a.seeds ? a.seeds[k] : rtr_bounce_pixel_seed(k, a.params.width, a.params.spp);
    const uint32_t s0seed = rtr_sky_seed(base, a.params.frame, a.params.depth);
    const uint32_t S = a.params.numSamples;
    const uint64_t total = LDS ? staged[H - 1u] : t.marginal[H - 1u];
    const bool live = sf.kind == RTR_SURFACE_OBJECT && total != 0u;
    for (uint32_t j = 0u; j < S; ++j) {
        RtrRay out;
        RtrSkySample rec;
        rtr_sky_dead(&out, &rec);
        if (live) {
            float u1, u2;
            rtr_sky_randoms(s0seed, j, &u1, &u2);
            double sRow;
            const uint64_t target = rtr_sky_target(u1, total, &sRow);
            uint32_t y;
            uint64_t prevRows, upTo;
            if (LDS) {
                RTR_SKY_SEARCH(staged, H, target, y);
                prevRows = y ? staged[y - 1u] : 0u; upTo = staged[y];
            } else {
                RTR_SKY_SEARCH(t.marginal, H, target, y);
                prevRows = y ? t.marginal[y - 1u] : 0u; upTo = t.marginal[y];
            }
            const rtr_v3 L = rtr_sky_sample_in_row(&t, y, prevRows, upTo - prevRows, sRow, u2);
            rtr_sky_vertex_dir(&ray, &sf, &a.sd.sky, &t, L, S, a.params.flags, a.params.lobes, &out, &rec);
        }
        const size_t at = (size_t)k * S + j;
        float4* __restrict__ orp = a.outRays + 2 * at;
        float4* __restrict__ osp = a.outSamples + 2 * at;
        orp[0] = make_float4(out.origin[0], out.origin[1], out.origin[2], out.tmin);
        orp[1] = make_float4(out.direction[0], out.direction[1], out.direction[2], out.tmax);
        osp[0] = make_float4(rec.contrib[0], rec.contrib[1], rec.contrib[2], rec.skyPdf);
        osp[1] = make_float4(rec.bouncePdf, rec.wSky, __uint_as_float(rec.cell), 0.0f);
    }
}

hipError_t launch_sky_rays(const SkyRaysArgs& a, bool ldsMarginal, hipStream_t s) {
    const dim3 grid((uint32_t)(((uint64_t)a.n + kSkyBlock - 1) / kSkyBlock));
    if (ldsMarginal) hipLaunchKernelGGL(k_sky_rays<true>, grid, dim3(kSkyBlock), (size_t)a.sd.table.height * sizeof(uint64_t), s, a);
    else hipLaunchKernelGGL(k_sky_rays<false>, grid, dim3(kSkyBlock), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(kSkyBlock) void k_shade_sky(SkyShadeArgs a) {
    const uint32_t k = blockIdx.x * kSkyBlock + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t S = a.numSamples;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    for (uint32_t j = 0u; j < S; ++j) {
        const size_t at = (size_t)k * S + j;
        const float4 c = a.samples[2 * at];
        if (a.occluded[at] == 0u) { x = x + c.x; y = y + c.y; z = z + c.z; }
    }
    a.out[k] = make_float4(x, y, z, 0.0f);
}

hipError_t launch_shade_sky(const SkyShadeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_shade_sky, dim3((uint32_t)(((uint64_t)a.n + kSkyBlock - 1) / kSkyBlock)), dim3(kSkyBlock), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(kSkyBlock) void k_sky_hits(SkyHitsArgs a) {
    const uint32_t k = blockIdx.x * kSkyBlock + threadIdx.x;
    if (k >= a.n) return;
    const float4 h0 = a.hits[2 * (size_t)k];
    RtrSkyEscape e;
    rtr_sky_escape_zero(&e);
    if (__float_as_uint(h0.w) == 0xffffffffu) {            /* a miss */
        const float4 r1 = a.rays[2 * (size_t)k + 1];
        const float4 s0 = a.prevSurfaces[5 * (size_t)k];
        const float4 b0 = a.bounces[2 * (size_t)k];
        RtrRay ray;
        ray.origin[0] = ray.origin[1] = ray.origin[2] = 0.0f; ray.tmin = 0.0f;
        ray.direction[0] = r1.x; ray.direction[1] = r1.y; ray.direction[2] = r1.z; ray.tmax = r1.w;
        rtr_sky_escape(&ray, __float_as_uint(s0.w), b0.w, &a.sd.sky, &a.sd.table, a.numSamples, a.flags, &e);
    }
    float4* __restrict__ o = a.out + 2 * (size_t)k;
    o[0] = make_float4(e.radiance[0], e.radiance[1], e.radiance[2], e.wBounce);
    o[1] = make_float4(e.skyPdf, e.bouncePdf, __uint_as_float(e.cell), __uint_as_float(e.kind));
}

hipError_t launch_sky_hits(const SkyHitsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_sky_hits, dim3((uint32_t)(((uint64_t)a.n + kSkyBlock - 1) / kSkyBlock)), dim3(kSkyBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace rtrdev
