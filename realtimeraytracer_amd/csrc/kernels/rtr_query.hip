/* rtr_query.hip — ray queries: the renderer's BVH2 walk for rays the caller supplies (include/rtr.h: rtr_trace_rays).
 *
 * What traceRayEXT does for the reference's ray-gen shader, without the fixed shaders: closest hit (gl_RayFlagsNoneEXT, the camera
 * rays of raygen.rgen:99-107) or terminate-on-first-hit (the shadow rays of raygen.rgen:226-231, :299-303), with or without the
 * opacity-map any-hit test.  The walk is trace() of rtr_device.h, the one the camera-ray kernel k_primary runs, so a camera ray
 * (rtr_camera_rays_async) traced here gets the renderer's primary hit bit for bit and is counted as the renderer counts it:
 *   k_query       one ray per lane, one-wave workgroups (RTR_PRIMARY_BLOCK, what k_primary measured best), 16-entry interleaved
 *                 LDS stack; a wave whose rays share their direction signs runs the octant form of the slab test.  A ray that
 *                 needs more stack is abandoned: its output gets a sentinel and it is appended to a bounded redo list, one atomic
 *                 per wave (ballot + mbcnt prefix: redo_append() of rtr_query_device.h, which k_multihit shares);
 *   k_query_tail  walks those rays again with a full-depth stack in global memory (as k_primary_tail does); if the redo list
 *                 overflowed it finds them by their sentinel in the outputs.
 * k_hit_surfaces (rtr_hit_surfaces) takes the hits further: the surface the closest-hit shader computes for each, by fetch_surface().
 * k_light_rays / k_shade_hits / k_tonemap_pack (rtr_light_rays, rtr_shade_hits, rtr_tonemap_pack) take them to the framebuffer: what the
 * ray-gen shader does after the closest hit, by the renderer's own light_loops() with every query at a fixed slot of its hit.
 * k_light_rays_picked / k_shade_hits_picked (rtr_light_rays_picked, rtr_shade_hits_picked) do the same for a few picked area-light slots
 * of each hit (include/rtr_pick.h) and the directional light: the light loops' sample functions, called per picked slot.
 * k_mis_pick_weights (rtr_mis_pick_weights) gives those picks their balance-heuristic weights against the vertex's bounce (include/rtr_mis.h).
 * k_pick_slots_ris (rtr_pick_slots_ris) chooses each pick among candidates of the power table by what they would contribute (include/rtr_ris.h).
 * Compiled with the library's flags (-ffp-contract=off): the numerical contract of include/rtr_math.h.
 */
#include "rtr_query_device.h"
#include "../../../include/rtr.h"
#include "../../../include/rtr_pick.h"
#include "../../../include/rtr_mis.h"
#include "../../../include/rtr_power.h"
#include "../../../include/rtr_ris.h"

namespace rtrdev {

#ifndef RTR_PRIMARY_BLOCK
#define RTR_PRIMARY_BLOCK 64
#endif
constexpr int kQueryBlock = RTR_PRIMARY_BLOCK;
static_assert(kQueryBlock % 64 == 0 && kQueryBlock >= 64 && kQueryBlock <= 1024, "RTR_PRIMARY_BLOCK: a multiple of 64");
constexpr int kQueryTailBlock = 256;
constexpr int kQueryTailBlocks = 64;         /* the spill area holds 64 entries for each of these 64 x 256 lanes */
static_assert((size_t)64 * kQueryTailBlocks * kQueryTailBlock == kSpillInts, "the tail kernel's stacks fill the spill area");
constexpr uint8_t kOccludedRedo = 0xffu;     /* sentinel of an abandoned any-hit ray (its hit record's sentinel: customIndex = RTR_STACK_OVERFLOW) */

/* RtrHit as two 16-B stores: {t, u, v, customIndex} {primitiveId, 0, 0, 0} */
__device__ __forceinline__ void query_store_hit(float4* __restrict__ hits, uint32_t k, const HitRec& h) {
    hits[2 * (size_t)k] = make_float4(h.t, h.u, h.v, __uint_as_float(h.custom));
    hits[2 * (size_t)k + 1] = make_float4(__uint_as_float(h.prim), 0.0f, 0.0f, 0.0f);
}

/* the call's RTR_QUERY_CULL_* flags (wave-uniform; 0: none), which travel in RayMaskArgs::masked beside the bit that selects these forms */
__device__ __forceinline__ uint32_t query_cull(const RayMaskArgs& rm) { return rm.masked & kCullAll; }
static_assert(kCullBackFacing == RTR_QUERY_CULL_BACK_FACING && kCullFrontFacing == RTR_QUERY_CULL_FRONT_FACING && kCullOpaque == RTR_QUERY_CULL_OPAQUE &&
              kCullNoOpaque == RTR_QUERY_CULL_NO_OPAQUE && (kCullAll & 1u) == 0u, "the kernels' cull bits are the interface's");

/* MASKED (rtr_trace_rays_masked): the ray's mask byte is read beside the ray; a ray whose effective mask is 0 is a miss that walks nothing,
 * like a degenerate ray.  The masks are the LAST kernel argument, behind everything the forms without MASKED read: those compile to the
 * instructions they had (compared function by function in the disassembly); only their kernel-argument segment is 16 B longer, which moves
 * the offset of the one hidden argument k_query_tail loads (the grid size).  Giving the MASKED forms kernels of their own instead kept the
 * segment and lost that: the inlined bodies were register-allocated differently (k_query 9 instructions longer). */
template <bool ANY, bool ALPHA, bool STATS, bool MASKED = false>
__global__ __launch_bounds__(kQueryBlock) void k_query(DeviceScene sc, QueryArgs qa, Counters* stats, RayMaskArgs rm) {
    __shared__ int32_t s_stack[16 * kQueryBlock];
    int32_t* stack = s_stack + threadIdx.x;
    const uint32_t k = blockIdx.x * kQueryBlock + threadIdx.x;
    if (k >= qa.n) return;
    LocalStats st;
    rtr_v3 o, d;
    float tmin, tmax;
    const uint32_t rm8 = MASKED ? query_ray_mask8(rm, k) : 0u;
    const uint32_t cull = MASKED ? query_cull(rm) : 0u;
    const bool ok = query_ray(qa.rays, k, o, d, tmin, tmax) && (!MASKED || rm8 != 0u);
    const float limit = ok ? tmax : tmin;                 /* a degenerate ray walks nothing (!(limit > tmin)) but is counted like any other */
    HitRec h;
    if (STATS) trace<ANY, true, kQueryBlock, 16, 8, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull);
    else {
        /* as in k_primary: the traversal compiled for the wave's direction signs when all its rays share them */
        const uint32_t oct = ray_octant(sc, o, d);
        const uint32_t woct = (uint32_t)__builtin_amdgcn_readfirstlane((int)oct);
        switch (__ballot(oct != woct) != 0ull ? 8u : woct) {
            case 0: trace<ANY, false, kQueryBlock, 16, 0, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
            case 1: trace<ANY, false, kQueryBlock, 16, 1, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
            case 2: trace<ANY, false, kQueryBlock, 16, 2, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
            case 3: trace<ANY, false, kQueryBlock, 16, 3, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
            case 4: trace<ANY, false, kQueryBlock, 16, 4, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
            case 5: trace<ANY, false, kQueryBlock, 16, 5, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
            case 6: trace<ANY, false, kQueryBlock, 16, 6, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
            case 7: trace<ANY, false, kQueryBlock, 16, 7, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
            default: trace<ANY, false, kQueryBlock, 16, 8, ALPHA, true, MASKED>(sc, stack, o, d, tmin, limit, h, st, rm8, cull); break;
        }
    }
    /* the walk's outcome is read from the record alone (as k_primary reads it), not from trace()'s return value */
    const bool over = h.custom == RTR_STACK_OVERFLOW, found = h.custom != RTR_MISS && !over;
    if (!ok) h.t = tmax;                                  /* a miss reports the ray's own tmax */
    if (ANY) qa.occluded[k] = over ? kOccludedRedo : (found ? 1u : 0u);
    else query_store_hit(qa.hits, k, h);                  /* an abandoned ray's record carries customIndex = RTR_STACK_OVERFLOW */
    redo_append(qa.ctrl, qa.redoList, qa.redoCap, over, k);
    if (STATS) st.flush(stats);
}

/* The rays k_query abandoned, walked from the root with a full-depth stack in global memory (no LDS, so it can always run).  From the
 * redo list, or — when more rays were abandoned than the list holds — from a scan of the outputs for their sentinel.  STATS: the
 * counting form (the ray itself was counted by k_query; this walk's visits and tests are added to it). */
template <bool ANY, bool ALPHA, bool STATS, bool MASKED = false>
__global__ __launch_bounds__(kQueryTailBlock) void k_query_tail(DeviceScene sc, QueryArgs qa, Counters* stats, RayMaskArgs rm) {
    const uint32_t count = qa.ctrl[kQueryRedoWord];
    if (count == 0u) return;
    const bool scan = count > qa.redoCap;
    const uint64_t m = scan ? qa.n : count;
    int32_t* stack = qa.spill + blockIdx.x * kQueryTailBlock + threadIdx.x;
    LocalStats st;
    for (uint64_t j = (uint64_t)blockIdx.x * kQueryTailBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kQueryTailBlock) {
        uint32_t k = (uint32_t)j;
        if (!scan) k = qa.redoList[j];
        else if (ANY ? qa.occluded[k] != kOccludedRedo : __float_as_uint(qa.hits[2 * (size_t)k].w) != RTR_STACK_OVERFLOW) continue;
        rtr_v3 o, d;
        float tmin, tmax;
        query_ray(qa.rays, k, o, d, tmin, tmax);          /* an abandoned ray is never degenerate: it walked past 16 stacked nodes */
        const uint32_t rm8 = MASKED ? query_ray_mask8(rm, k) : 0u;      /* re-read like the ray: never 0 here, such a ray walked nothing */
        HitRec h;
        trace<ANY, STATS, kQueryTailBlocks * kQueryTailBlock, 0, 8, ALPHA, true, MASKED>(sc, stack, o, d, tmin, tmax, h, st, rm8, MASKED ? query_cull(rm) : 0u);
        const bool found = h.custom != RTR_MISS;
        if (STATS) { st.rays--; if (ANY) st.shadow--; else st.primary--; }
        if (ANY) qa.occluded[k] = found ? 1u : 0u;
        else query_store_hit(qa.hits, k, h);
    }
    if (STATS) st.flush(stats);
}

template <bool ANY, bool ALPHA, bool STATS, bool MASKED>
static hipError_t query_t(const DeviceScene& sc, const QueryArgs& qa, Counters* stats, hipStream_t s, const RayMaskArgs& rm) {
    const uint32_t blocks = (uint32_t)(((uint64_t)qa.n + kQueryBlock - 1) / kQueryBlock);
    hipLaunchKernelGGL((k_query<ANY, ALPHA, STATS, MASKED>), dim3(blocks), dim3(kQueryBlock), 0, s, sc, qa, stats, rm);
    hipLaunchKernelGGL((k_query_tail<ANY, ALPHA, STATS, MASKED>), dim3(kQueryTailBlocks), dim3(kQueryTailBlock), 0, s, sc, qa, stats, rm);
    return hipGetLastError();
}

template <bool ANY, bool ALPHA, bool MASKED>
static hipError_t query_s(const DeviceScene& sc, const QueryArgs& qa, Counters* stats, hipStream_t s, const RayMaskArgs& rm) {
    return stats ? query_t<ANY, ALPHA, true, MASKED>(sc, qa, stats, s, rm) : query_t<ANY, ALPHA, false, MASKED>(sc, qa, stats, s, rm);
}

template <bool MASKED>
static hipError_t query_f(const DeviceScene& sc, const QueryArgs& qa, uint32_t flags, Counters* stats, hipStream_t s, const RayMaskArgs& rm) {
    const bool any = (flags & RTR_QUERY_ANY) != 0u, alpha = (flags & RTR_QUERY_OPAQUE) == 0u;
    if (any) return alpha ? query_s<true, true, MASKED>(sc, qa, stats, s, rm) : query_s<true, false, MASKED>(sc, qa, stats, s, rm);
    return alpha ? query_s<false, true, MASKED>(sc, qa, stats, s, rm) : query_s<false, false, MASKED>(sc, qa, stats, s, rm);
}

hipError_t launch_query(const DeviceScene& sc, const QueryArgs& qa, uint32_t flags, Counters* stats, hipStream_t s, const RayMaskArgs& rm) {
    return rm.masked ? query_f<true>(sc, qa, flags, stats, s, rm) : query_f<false>(sc, qa, flags, stats, s, rm);
}

template <bool MASKED>
static hipError_t query_tail_any(const DeviceScene& sc, const QueryArgs& qa, bool alpha, Counters* stats, hipStream_t s, const RayMaskArgs& rm) {
    if (alpha) {
        if (stats) hipLaunchKernelGGL((k_query_tail<true, true, true, MASKED>), dim3(kQueryTailBlocks), dim3(kQueryTailBlock), 0, s, sc, qa, stats, rm);
        else hipLaunchKernelGGL((k_query_tail<true, true, false, MASKED>), dim3(kQueryTailBlocks), dim3(kQueryTailBlock), 0, s, sc, qa, stats, rm);
    } else {
        if (stats) hipLaunchKernelGGL((k_query_tail<true, false, true, MASKED>), dim3(kQueryTailBlocks), dim3(kQueryTailBlock), 0, s, sc, qa, stats, rm);
        else hipLaunchKernelGGL((k_query_tail<true, false, false, MASKED>), dim3(kQueryTailBlocks), dim3(kQueryTailBlock), 0, s, sc, qa, stats, rm);
    }
    return hipGetLastError();
}

hipError_t launch_query_tail_any(const DeviceScene& sc, const QueryArgs& qa, bool alpha, Counters* stats, hipStream_t s, const RayMaskArgs& rm) {
    return rm.masked ? query_tail_any<true>(sc, qa, alpha, stats, s, rm) : query_tail_any<false>(sc, qa, alpha, stats, s, rm);
}

/* one lane per pixel-sample: the camera ray k_primary traces for it (primary_dir, tmin 0.001, tmax 10000) */
constexpr int kCameraRaysBlock = 256;
__global__ __launch_bounds__(kCameraRaysBlock) void k_camera_rays(RenderArgs ra, uint32_t n, float4* __restrict__ out) {
    const uint32_t k = blockIdx.x * kCameraRaysBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = k % ra.spp, pix = k / ra.spp;
    const uint32_t px = pix % ra.width, py = pix / ra.width;
    const rtr_v3 d = primary_dir(ra, px, py, i);
    out[2 * (size_t)k] = make_float4(ra.cam.position[0], ra.cam.position[1], ra.cam.position[2], 0.001f);
    out[2 * (size_t)k + 1] = make_float4(d.x, d.y, d.z, 10000.0f);
}

hipError_t launch_camera_rays(const RtrCameraData& cam, uint32_t width, uint32_t height, uint32_t spp, float4* out, hipStream_t s) {
    RenderArgs ra{};
    ra.cam = cam; ra.width = width; ra.height = height; ra.spp = spp;
    const uint32_t n = width * height * spp;
    hipLaunchKernelGGL(k_camera_rays, dim3((uint32_t)(((uint64_t)n + kCameraRaysBlock - 1) / kCameraRaysBlock)), dim3(kCameraRaysBlock), 0, s, ra, n, out);
    return hipGetLastError();
}

/* One lane per hit: what the closest-hit shader computes for it (rtr_hit_surfaces).  The surface is fetch_surface<true>'s, the one the
 * renderer shades with, called without the LTC lookups (wantAnalytic = false): hit point, shading normal, linear colour and material
 * for an object; the light's colour at a light hit and the sky radiance at a miss, read from the Accum it adds them to.  uv and the
 * geometric normal come next to it, in the same rtr_math.h forms.  Ids out of range are INVALID and read nothing of the scene. */
constexpr int kSurfaceBlock = 256;
__global__ __launch_bounds__(kSurfaceBlock) void k_hit_surfaces(DeviceScene sc, SurfaceArgs sa) {
    const uint32_t k = blockIdx.x * kSurfaceBlock + threadIdx.x;
    if (k >= sa.n) return;
    const float4 rb = sa.rays[2 * (size_t)k + 1];                                   /* {direction, tmax}: the origin is not needed */
    const float4 ha = sa.hits[2 * (size_t)k], hb = sa.hits[2 * (size_t)k + 1];
    HitRec h;
    h.t = ha.x; h.u = ha.y; h.v = ha.z; h.custom = __float_as_uint(ha.w); h.prim = __float_as_uint(hb.x); h.leaf = 0;
    const rtr_v3 dir = f4xyz(rb);
    uint32_t kind = RTR_SURFACE_INVALID, index = 0xffffffffu;
    if (h.custom == RTR_MISS) kind = RTR_SURFACE_MISS;
    else if (h.custom < sa.numInstances && h.prim < sa.triCount[h.custom]) {
        kind = h.custom < sc.numLights ? RTR_SURFACE_LIGHT : RTR_SURFACE_OBJECT;
        index = h.custom < sc.numLights ? h.custom : h.custom - sc.numLights;
    }
    const rtr_v3 zero = rtr_mk(0, 0, 0);
    rtr_v3 position = zero, normal = zero, geomNormal = zero, color = zero;
    float metallic = 0.0f, roughness = 0.0f, uu = 0.0f, vv = 0.0f;
    if (kind != RTR_SURFACE_INVALID) {
        RenderArgs ra{};                     /* fetch_surface reads only the camera position, for a view vector this kernel does not output */
        Accum acc;
        acc.analytic = acc.shadowed = acc.unshadowed = acc.avgNormal = acc.avgPosition = zero;
        Surface sf;
        LocalStats st;
        fetch_surface<true, false>(sc, ra, h, dir, false, acc, sf, st);
        const float b0 = 1.0f - h.u - h.v, b1 = h.u, b2 = h.v;
        if (kind == RTR_SURFACE_OBJECT) {
            position = sf.hitPoint; normal = sf.hitNormal; color = sf.color; metallic = sf.metallic; roughness = sf.roughness;
            const RtrObjectInfo* oi = sc.objects + index;
            const uint32_t vOff = oi->vertexOffset, iOff = oi->indexOffset;
            const float4* va = reinterpret_cast<const float4*>(sc.vertices + (sc.indices[3u * h.prim + 0u + iOff] + vOff));
            const float4* vb = reinterpret_cast<const float4*>(sc.vertices + (sc.indices[3u * h.prim + 1u + iOff] + vOff));
            const float4* vc = reinterpret_cast<const float4*>(sc.vertices + (sc.indices[3u * h.prim + 2u + iOff] + vOff));
            const rtr_v3 p0 = f4xyz(va[0]), p1 = f4xyz(vb[0]), p2 = f4xyz(vc[0]);
            const rtr_v3 g = rtr_cross(rtr_sub(p1, p0), rtr_sub(p2, p0));
            geomNormal = rtr_normalize(rtr_mul33(sc.nmats + 12u * h.custom, rtr_normalize(g)));
            const float4 ta = va[2], tb = vb[2], tc = vc[2];                       /* uv in floats 8,9 of the 48-B vertex */
            uu = rtr_fma(tc.x, b2, rtr_fma(tb.x, b1, ta.x * b0));
            vv = rtr_fma(tc.y, b2, rtr_fma(tb.y, b1, ta.y * b0));
        } else {
            color = acc.shadowed;                                                    /* the sky at a miss, the light's colour at a light */
            if (kind == RTR_SURFACE_LIGHT) {
                /* k_light_tris writes light l's records at lightTriFirst[l] + primitiveId (triangle ti of the light's index range) */
                const float4* rec = sc.lightTris + (size_t)(sc.lightTriFirst[index] + h.prim) * kLightTriRecord;
                position = rtr_madd(rtr_madd(rtr_scale(f4xyz(rec[0]), b0), f4xyz(rec[1]), b1), f4xyz(rec[2]), b2);
                normal = geomNormal = f4xyz(rec[3]);
            }
        }
    }
    float4* o = sa.out + 5 * (size_t)k;
    o[0] = make_float4(position.x, position.y, position.z, __uint_as_float(kind));
    o[1] = make_float4(normal.x, normal.y, normal.z, __uint_as_float(index));
    o[2] = make_float4(geomNormal.x, geomNormal.y, geomNormal.z, metallic);
    o[3] = make_float4(color.x, color.y, color.z, roughness);
    o[4] = make_float4(uu, vv, 0.0f, 0.0f);
}

hipError_t launch_hit_surfaces(const DeviceScene& sc, const SurfaceArgs& sa, hipStream_t s) {
    hipLaunchKernelGGL(k_hit_surfaces, dim3((uint32_t)(((uint64_t)sa.n + kSurfaceBlock - 1) / kSurfaceBlock)), dim3(kSurfaceBlock), 0, s, sc, sa);
    return hipGetLastError();
}

/* ---- the triangle -> leaf table (rtr_hit_leaves, rtr_light_rays_hinted) --------------------------------------------------------------
 * One lane per BVH2 node: each of its two children that is a leaf writes its code at the (customIndex, primitiveId) of its up to 8
 * records.  A record sits in one leaf, so no entry is written with two values (a scene of a single leaf stores it as both children of
 * the root: the same value twice); slots of the node array that are not part of a device-built tree hold child codes 0, 0.  The ids are
 * checked against the table's extent and the leaf against the record array before anything is read or written there: the degenerate
 * record of an empty scene (customIndex 0xffffffff) writes nothing. */
constexpr int kLeafTableBlock = 256;
__global__ __launch_bounds__(kLeafTableBlock) void k_leaf_table(const uint4* __restrict__ nodes, uint32_t numNodes, const float4* __restrict__ tris,
                                                                uint32_t numTris, const uint32_t* __restrict__ triCount, const uint32_t* __restrict__ base,
                                                                uint32_t numInstances, int32_t* __restrict__ table, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;                               /* a gated launch (rtr_scene_rebuild_if_async) whose decision word says no */
    const uint32_t i = blockIdx.x * kLeafTableBlock + threadIdx.x;
    if (i >= numNodes) return;
    const uint4 w = nodes[2 * (size_t)i + 1];                  /* {z planes, child[0], child[1]} */
    const int32_t child[2] = {(int32_t)w.z, (int32_t)w.w};
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        if (child[sl] >= 0) continue;
        const uint32_t code = (uint32_t)~child[sl];
        const uint32_t first = code >> 3, cnt = (code & 7u) + 1u;
        if (first + cnt > numTris) continue;
        for (uint32_t j = first; j < first + cnt; ++j) {
            const uint32_t custom = __float_as_uint(tris[3 * (size_t)j].w), prim = __float_as_uint(tris[3 * (size_t)j + 1].w);
            if (custom < numInstances && prim < triCount[custom]) table[base[custom] + prim] = child[sl];
        }
    }
}

hipError_t launch_leaf_table(const uint4* nodes, uint32_t numNodes, const float4* tris, uint32_t numTris, const uint32_t* triCount,
                             const uint32_t* base, uint32_t numInstances, int32_t* table, hipStream_t s, const uint32_t* go) {
    if (numNodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_leaf_table, dim3((numNodes + kLeafTableBlock - 1) / kLeafTableBlock), dim3(kLeafTableBlock), 0, s, nodes, numNodes, tris, numTris,
                       triCount, base, numInstances, table, go);
    return hipGetLastError();
}

/* ---- instance cull masks (rtr_scene_set_instance_masks) ---------------------------------------------------------------------------------
 * One lane per record of the leaf-ordered triangle array: bits 8..15 of its flags word (kTriMaskBits) become maskBits[customIndex] — the
 * complement of its instance's mask, so the default 0xff is the zero the builders write — by one 4-byte store; bit 0 (alpha-tested) and
 * every other byte of the record stay.  A customIndex past the table (the dummy record of an empty scene) is left alone. */
constexpr int kSetMasksBlock = 256;
__global__ __launch_bounds__(kSetMasksBlock) void k_set_instance_masks(float4* __restrict__ tris, uint32_t numTris, const uint32_t* __restrict__ maskBits,
                                                                       uint32_t numInstances) {
    const uint32_t j = blockIdx.x * kSetMasksBlock + threadIdx.x;
    if (j >= numTris) return;
    const uint32_t custom = __float_as_uint(tris[3 * (size_t)j].w);
    if (custom >= numInstances) return;
    uint32_t* const flags = reinterpret_cast<uint32_t*>(&tris[3 * (size_t)j + 2].w);
    *flags = (*flags & ~kTriMaskBits) | (maskBits[custom] & kTriMaskBits);
}

hipError_t launch_set_instance_masks(float4* tris, uint32_t numTris, const uint32_t* maskBits, uint32_t numInstances, hipStream_t s) {
    if (numTris == 0 || numInstances == 0) return hipSuccess;
    hipLaunchKernelGGL(k_set_instance_masks, dim3((numTris + kSetMasksBlock - 1) / kSetMasksBlock), dim3(kSetMasksBlock), 0, s, tris, numTris, maskBits, numInstances);
    return hipGetLastError();
}

/* the table entry of a hit's ids, or 0 (a miss, RTR_STACK_OVERFLOW and anything else out of range: nothing is read for them) */
__device__ __forceinline__ int32_t leaf_of(const uint32_t* __restrict__ triCount, const uint32_t* __restrict__ base, const int32_t* __restrict__ table,
                                           uint32_t numInstances, uint32_t custom, uint32_t prim) {
    if (custom >= numInstances || prim >= triCount[custom]) return 0;
    return table[base[custom] + prim];
}

constexpr int kHitLeavesBlock = 256;
__global__ __launch_bounds__(kHitLeavesBlock) void k_hit_leaves(LeafArgs a) {
    const uint32_t k = blockIdx.x * kHitLeavesBlock + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t custom = __float_as_uint(a.hits[2 * (size_t)k].w), prim = __float_as_uint(a.hits[2 * (size_t)k + 1].x);
    a.leaves[k] = leaf_of(a.triCount, a.base, a.table, a.numInstances, custom, prim);
}

hipError_t launch_hit_leaves(const LeafArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_hit_leaves, dim3((uint32_t)(((uint64_t)a.n + kHitLeavesBlock - 1) / kHitLeavesBlock)), dim3(kHitLeavesBlock), 0, s, a);
    return hipGetLastError();
}

/* ---- direct lighting for caller hits (rtr_light_rays, rtr_shade_hits, rtr_tonemap_pack) ------------------------------------------------
 * What raygen.rgen:110-338 does with a closest hit, cut where the renderer's staged pipeline cuts it: the shadow rays of a hit, and —
 * once the caller has had them answered (rtr_trace_rays, RTR_QUERY_ANY) — the sums.  Both kernels run light_loops(), the loops
 * k_shadow_gen_oct and k_resolve run, with a policy that takes each query's place from slots_at(): hit k owns la.slots (Q) consecutive
 * slots, sample s of light triangle T_l + ti at (T_l + ti) * numShadowRays + s, the directional light last (include/rtr.h). */
typedef float rtr_q4 __attribute__((ext_vector_type(4)));

/* What a hit is, as k_hit_surfaces decides it; the hit record, the ray's direction and the RenderArgs the device functions read:
 * the view vector's origin (the ray's), numAreaLights, numShadowRays and the frame word.  light_sample_pos forms a sample's seed as
 * s + px * 733 + py * 1933 + frame in 32-bit words, so handing it px = py = 0 and frame + base gives the seed s + base + frame of
 * include/rtr.h whatever base is: the caller's seeds[k], or the pixel's px * 733 + py * 1933 (the renderer's seed for a camera ray). */
__device__ __forceinline__ uint32_t light_hit(const DeviceScene& sc, const LightArgs& la, uint32_t k, HitRec& h, rtr_v3& dir, RenderArgs& ra) {
    const float4 ro = la.rays[2 * (size_t)k], rb = la.rays[2 * (size_t)k + 1];
    const float4 ha = la.hits[2 * (size_t)k], hb = la.hits[2 * (size_t)k + 1];
    h.t = ha.x; h.u = ha.y; h.v = ha.z; h.custom = __float_as_uint(ha.w); h.prim = __float_as_uint(hb.x); h.leaf = 0;
    dir = f4xyz(rb);
    uint32_t base;
    if (la.seeds) base = la.seeds[k];
    else { const uint32_t pix = k / la.spp; base = (pix % la.width) * 733u + (pix / la.width) * 1933u; }
    ra.cam.position[0] = ro.x; ra.cam.position[1] = ro.y; ra.cam.position[2] = ro.z;
    ra.info.numAreaLights = la.numAreaLights; ra.info.frame = la.frame + base;
    ra.numShadowRays = la.numShadowRays; ra.spp = 1u;
    if (h.custom == RTR_MISS) return RTR_SURFACE_MISS;
    if (h.custom < la.numInstances && h.prim < la.triCount[h.custom]) return h.custom < sc.numLights ? RTR_SURFACE_LIGHT : RTR_SURFACE_OBJECT;
    return RTR_SURFACE_INVALID;
}

/* the query's ray into its slot of the hit's row: {origin, tmin 0.001} {direction, tmax}, two 16-B stores (LDS or global) */
template <class Row>
struct RayEmitPolicy {
    static constexpr bool kShade = false;
    Row row; uint32_t slot, last;
    __device__ __forceinline__ void slots_at(uint32_t first) { slot = first == kDirectionalSlot ? last : first; }
    __device__ __forceinline__ bool occluded(rtr_v3 o, rtr_v3 d, float tmax, rtr_v3, bool) {
        row[2u * slot] = rtr_q4{o.x, o.y, o.z, 0.001f};
        row[2u * slot + 1u] = rtr_q4{d.x, d.y, d.z, tmax};
        ++slot;
        return false;
    }
};

/* RayEmitPolicy and, beside each ray, its start hint for the queued occlusion query (rtr_light_rays_hinted): the leaf of the hit's own
 * triangle where the ray leaves INTO the surface — light_loops' intoSurface, the mark the renderer's queue build sets — else 0.  The
 * hints have a row of their own, one word per slot. */
template <class Row, class HintRow>
struct RayHintEmitPolicy {
    static constexpr bool kShade = false;
    Row row; HintRow hints; int32_t leaf; uint32_t slot, last;
    __device__ __forceinline__ void slots_at(uint32_t first) { slot = first == kDirectionalSlot ? last : first; }
    __device__ __forceinline__ bool occluded(rtr_v3 o, rtr_v3 d, float tmax, rtr_v3, bool into) {
        row[2u * slot] = rtr_q4{o.x, o.y, o.z, 0.001f};
        row[2u * slot + 1u] = rtr_q4{d.x, d.y, d.z, tmax};
        hints[slot] = into ? leaf : 0;
        ++slot;
        return false;
    }
};

/* One lane per hit, one wave per workgroup.  A hit's Q rays are 32 B apiece and 32 Q bytes from the next lane's: stored where the light
 * loops make them, every store instruction of the wave touches 64 different cache lines, half of each.  STAGED (Q <= kLightStagedSlots):
 * the wave's rays are made in LDS — lane l's row at l * (2 Q + 1) 16-B pieces: the odd pitch spreads the eight lanes a ds_write_b128
 * serves together over eight different 16-B bank slots, where the dense pitch 2 Q puts them all on one whenever Q is a multiple of 4 —
 * pre-filled with zeros, which ARE the null rays of the slots the loops skip; then the wave stores its contiguous 64 * Q * 32-byte block
 * with lane i on the i-th consecutive 16-B piece, 1 KiB per store instruction, every line written whole.  !STAGED is the form it was
 * compared with and the one left for light tables whose rows outgrow a workgroup's 64 KiB of LDS: zeros and rays stored straight from
 * the loops at the 32 Q-byte lane stride.  (The pre-fill cannot be a memset ahead of the kernel in either form without writing the
 * buffer twice.)  Both forms write the same bytes; tests/test_gpu_direct_light.py runs both against one another.  Measured on the bench
 * frame's camera hits (1920x1080, Q = 13, 863 MB of rays): staged 0.277 ms (3.1 TB/s written), direct 0.596 ms
 * (profiles/direct_light_rate.py, profiles/direct_light/).
 * HINTS (rtr_light_rays_hinted): the rays as before and la.outLeaves, one word per slot.  STAGED, the wave's hints are made in LDS behind
 * the rays — lane l's row at l * (Q | 1) words, zeros first: the 0 of every slot without a mark — and stored as the wave's contiguous
 * 64 * Q * 4-byte block, lane i on the i-th word, 256 B per store instruction; !STAGED, zeros and hints go straight to the 4 Q-byte lane
 * stride.  The forms without HINTS compile to what they were. */
constexpr int kLightRaysBlock = 64;
constexpr uint32_t kLightStagedSlots = 31;       /* 64 lanes x (2 * 31 + 1) pieces x 16 B = 63 KiB */
constexpr uint32_t kLightStagedLds = 64u << 10;  /* what a workgroup's stage may take: rays, and hints behind them */
__host__ __device__ constexpr uint32_t light_hint_pitch(uint32_t q) { return q | 1u; }      /* odd, as the rays' pitch: the lanes that write one slot spread over the banks */
template <bool STAGED, bool HINTS = false>
__global__ __launch_bounds__(kLightRaysBlock) void k_light_rays(DeviceScene sc, LightArgs la) {
    extern __shared__ rtr_q4 s_stage[];
    typedef __attribute__((address_space(3))) rtr_q4* lds_q4;      /* keeps the accesses ds_read / ds_write */
    typedef __attribute__((address_space(3))) int32_t* lds_i32;
    const lds_q4 stage = (lds_q4)s_stage;
    const uint32_t lane = threadIdx.x;
    const uint64_t k0 = (uint64_t)blockIdx.x * kLightRaysBlock;
    const bool live = k0 + lane < la.n;
    const uint32_t k = (uint32_t)(k0 + lane);
    const uint32_t Q = la.slots, pieces = 2u * Q, pitch = pieces + 1u;
    rtr_q4* __restrict__ out = reinterpret_cast<rtr_q4*>(la.outRays) + k0 * pieces;          /* the wave's block */
    const rtr_q4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t hpitch = light_hint_pitch(Q);
    const lds_i32 hstage = (lds_i32)(stage + kLightRaysBlock * pitch);                         /* HINTS && STAGED: behind the rays */
    int32_t* __restrict__ outHints = HINTS ? la.outLeaves + k0 * Q : nullptr;                /* the wave's block */
    if (STAGED) {
        for (uint32_t i = lane; i < kLightRaysBlock * pitch; i += kLightRaysBlock) stage[i] = zero;
        if (HINTS) for (uint32_t i = lane; i < kLightRaysBlock * hpitch; i += kLightRaysBlock) hstage[i] = 0;
        __syncthreads();
    } else if (live) {
        for (uint32_t j = 0; j < pieces; ++j) out[(size_t)lane * pieces + j] = zero;
        if (HINTS) for (uint32_t j = 0; j < Q; ++j) outHints[(size_t)lane * Q + j] = 0;
    }
    if (live) {
        HitRec h;
        rtr_v3 dir;
        RenderArgs ra{};
        if (light_hit(sc, la, k, h, dir, ra) == RTR_SURFACE_OBJECT) {
            Accum acc;
            Surface sf;
            LocalStats st;
            fetch_surface<false, false>(sc, ra, h, dir, false, acc, sf, st);
            if (HINTS) {
                const int32_t leaf = leaf_of(la.triCount, la.leafBase, la.leafTable, la.numInstances, h.custom, h.prim);
                if (STAGED) {
                    RayHintEmitPolicy<lds_q4, lds_i32> pol{stage + lane * pitch, hstage + lane * hpitch, leaf, 0u, Q - 1u};
                    light_loops<RayHintEmitPolicy<lds_q4, lds_i32>, false>(sc, ra, 0u, 0u, sf, 0u, acc, pol, st);
                } else {
                    RayHintEmitPolicy<rtr_q4*, int32_t*> pol{out + (size_t)lane * pieces, outHints + (size_t)lane * Q, leaf, 0u, Q - 1u};
                    light_loops<RayHintEmitPolicy<rtr_q4*, int32_t*>, false>(sc, ra, 0u, 0u, sf, 0u, acc, pol, st);
                }
            } else if (STAGED) {
                RayEmitPolicy<lds_q4> pol{stage + lane * pitch, 0u, Q - 1u};
                light_loops<RayEmitPolicy<lds_q4>, false>(sc, ra, 0u, 0u, sf, 0u, acc, pol, st);
            } else {
                RayEmitPolicy<rtr_q4*> pol{out + (size_t)lane * pieces, 0u, Q - 1u};
                light_loops<RayEmitPolicy<rtr_q4*>, false>(sc, ra, 0u, 0u, sf, 0u, acc, pol, st);
            }
        }
    }
    if (STAGED) {
        __syncthreads();
        const uint64_t left = la.n - k0;
        const uint32_t total = (uint32_t)(left < (uint64_t)kLightRaysBlock ? left : (uint64_t)kLightRaysBlock) * pieces;
        /* piece p of the block belongs to row p / pieces: kept as (row, rest) and stepped by 64 pieces, one division per lane */
        const uint32_t stepRow = (uint32_t)kLightRaysBlock / pieces, stepRest = (uint32_t)kLightRaysBlock % pieces;
        uint32_t row = lane / pieces, rest = lane % pieces;
        for (uint32_t p = lane; p < total; p += kLightRaysBlock) {
            out[p] = stage[row * pitch + rest];
            row += stepRow; rest += stepRest;
            if (rest >= pieces) { rest -= pieces; ++row; }
        }
        if (HINTS) {      /* the same walk over the hint words: word p belongs to row p / Q */
            const uint32_t words = total / 2u;
            const uint32_t hStepRow = (uint32_t)kLightRaysBlock / Q, hStepRest = (uint32_t)kLightRaysBlock % Q;
            uint32_t hrow = lane / Q, hrest = lane % Q;
            for (uint32_t p = lane; p < words; p += kLightRaysBlock) {
                outHints[p] = hstage[hrow * hpitch + hrest];
                hrow += hStepRow; hrest += hStepRest;
                if (hrest >= Q) { hrest -= Q; ++hrow; }
            }
        }
    }
}

hipError_t launch_light_rays(const DeviceScene& sc, const LightArgs& la, hipStream_t s) {
    const uint32_t blocks = (uint32_t)(((uint64_t)la.n + kLightRaysBlock - 1) / kLightRaysBlock);
    if (la.outLeaves) {      /* staged while rays and hints both fit the stage */
        const size_t lds = (size_t)kLightRaysBlock * ((2u * (size_t)la.slots + 1u) * sizeof(rtr_q4) + light_hint_pitch(la.slots) * sizeof(int32_t));
        if (la.slots <= kLightStagedSlots && lds <= kLightStagedLds && !la.direct)
            hipLaunchKernelGGL((k_light_rays<true, true>), dim3(blocks), dim3(kLightRaysBlock), lds, s, sc, la);
        else hipLaunchKernelGGL((k_light_rays<false, true>), dim3(blocks), dim3(kLightRaysBlock), 0, s, sc, la);
    } else if (la.slots <= kLightStagedSlots && !la.direct) {
        const size_t lds = (size_t)kLightRaysBlock * (2u * la.slots + 1u) * sizeof(rtr_q4);
        hipLaunchKernelGGL(k_light_rays<true>, dim3(blocks), dim3(kLightRaysBlock), lds, s, sc, la);
    } else hipLaunchKernelGGL(k_light_rays<false>, dim3(blocks), dim3(kLightRaysBlock), 0, s, sc, la);
    return hipGetLastError();
}

/* the visibility byte of the query's slot (the caller's RTR_QUERY_ANY answers for the rays k_light_rays made) */
struct SlotLookupPolicy {
    static constexpr bool kShade = true;
    const uint8_t* occ; uint32_t slot, last;
    __device__ __forceinline__ void slots_at(uint32_t first) { slot = first == kDirectionalSlot ? last : first; }
    __device__ __forceinline__ bool occluded(rtr_v3, rtr_v3, float, rtr_v3, bool) { return occ[slot++] != 0; }
};

/* One lane per hit: shade_sample() — fetch_surface<true> and the light loops, as k_resolve calls them for one sample of a pixel — into
 * a zeroed Accum; `want` is the renderer's (bit 0 analytic, bit 1 unshadowed), so the same work is skipped under the same rule.  A sum
 * that was not asked for is written as zeros. */
constexpr int kShadeBlock = 256;
__global__ __launch_bounds__(kShadeBlock) void k_shade_hits(DeviceScene sc, LightArgs la) {
    const uint32_t k = blockIdx.x * kShadeBlock + threadIdx.x;
    if (k >= la.n) return;
    HitRec h;
    rtr_v3 dir;
    RenderArgs ra{};
    const uint32_t kind = light_hit(sc, la, k, h, dir, ra);
    const bool wantUnshadowed = (la.outputs & RTR_LIGHT_UNSHADOWED) != 0u, wantAnalytic = (la.outputs & RTR_LIGHT_ANALYTIC) != 0u;
    const rtr_v3 zero = rtr_mk(0, 0, 0);
    Accum acc;
    acc.analytic = acc.shadowed = acc.unshadowed = acc.avgNormal = acc.avgPosition = zero;
    if (kind != RTR_SURFACE_INVALID) {
        LocalStats st;
        SlotLookupPolicy pol{la.occluded + (size_t)k * la.slots, 0u, la.slots - 1u};
        shade_sample<SlotLookupPolicy, false>(sc, ra, 0u, 0u, h, dir, (wantAnalytic ? 1u : 0u) | (wantUnshadowed ? 2u : 0u), acc, pol, st);
    }
    if (!wantUnshadowed) acc.unshadowed = zero;
    if (!wantAnalytic) acc.analytic = zero;
    float4* o = la.out + 3 * (size_t)k;
    o[0] = make_float4(acc.shadowed.x, acc.shadowed.y, acc.shadowed.z, __uint_as_float(kind));
    o[1] = make_float4(acc.unshadowed.x, acc.unshadowed.y, acc.unshadowed.z, 0.0f);
    o[2] = make_float4(acc.analytic.x, acc.analytic.y, acc.analytic.z, 0.0f);
}

hipError_t launch_shade_hits(const DeviceScene& sc, const LightArgs& la, hipStream_t s) {
    hipLaunchKernelGGL(k_shade_hits, dim3((uint32_t)(((uint64_t)la.n + kShadeBlock - 1) / kShadeBlock)), dim3(kShadeBlock), 0, s, sc, la);
    return hipGetLastError();
}

/* one lane per value: raygen.rgen:345-357 (ACES, sRGB, bytes B, G, R, 255) of the three floats at radiance + k * strideWords */
constexpr int kTonemapBlock = 256;
__global__ __launch_bounds__(kTonemapBlock) void k_tonemap_pack(const float* __restrict__ radiance, uint32_t strideWords, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * kTonemapBlock + threadIdx.x;
    if (k >= n) return;
    const float* r = radiance + (size_t)k * strideWords;
    out[k] = tonemap_pack(rtr_mk(r[0], r[1], r[2]));
}

hipError_t launch_tonemap_pack(const float* radiance, uint32_t strideWords, uint32_t n, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_tonemap_pack, dim3((uint32_t)(((uint64_t)n + kTonemapBlock - 1) / kTonemapBlock)), dim3(kTonemapBlock), 0, s, radiance, strideWords, n, out);
    return hipGetLastError();
}

/* ---- picked light samples (rtr_light_rays_picked, rtr_shade_hits_picked) -----------------------------------------------------------
 * The same rays and the same sums for P of a hit's A area slots (include/rtr_pick.h) and the directional light: hit k owns R = P + 1
 * slots, the picks first.  Slot j is sample j % ns of light triangle t = j / ns, and t differs from lane to lane: where light_loops reads
 * a triangle's record and its light's colour, intensity and sidedness through wave-uniform addresses (scalar loads), these are per-lane
 * gathers from the same small tables — four 16-B pieces of sc.lightTris, 32 B of sc.lights.  The light of t is found in sc.lightTriFirst
 * by a binary search over the first numAreaLights entries: the last l with lightTriFirst[l] <= t, at most ceil(log2(numAreaLights))
 * steps (a light without triangles shares its entry with the next one and is passed over).  The sample's point, the cull of a one-sided
 * triangle, direction, distance and BRDF are light_sample_pos, the test of light_loops and area_sample_contrib: called, not restated. */
struct PickedSample { rtr_v3 dir; float dist; rtr_v3 lcol; float lintensity, pdf; };

/* what light_loops computes for area slot j < A of a surface point; false where it sends no ray (a one-sided triangle facing away) */
__device__ __forceinline__ bool picked_sample(const DeviceScene& sc, const PickArgs& pa, const RenderArgs& ra, rtr_v3 hitPoint, uint32_t j, PickedSample& ps) {
    const uint32_t t = j / pa.la.numShadowRays, s = j - t * pa.la.numShadowRays;
    uint32_t lo = 0u, hi = pa.la.numAreaLights;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sc.lightTriFirst[mid] <= t) lo = mid; else hi = mid;
    }
    const RtrAreaLightInfo* L = sc.lights + lo;
    const float4* rec = sc.lightTris + (size_t)t * kLightTriRecord;
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    rtr_v3 P[3];
    P[0] = rtr_mk(r0.x, r0.y, r0.z); P[1] = rtr_mk(r1.x, r1.y, r1.z); P[2] = rtr_mk(r2.x, r2.y, r2.z);
    if (L->isTwoSided == 0u) {
        if (rtr_dot(rtr_mk(r3.x, r3.y, r3.z), rtr_sub(hitPoint, P[0])) < 0.0f) return false;
    }
    const rtr_v3 lightVec = rtr_sub(light_sample_pos(P, s, 0u, 0u, ra.info.frame), hitPoint);
    ps.dir = rtr_normalize(lightVec);
    ps.dist = rtr_length(lightVec);
    ps.lcol = rtr_ld3(L->color); ps.lintensity = L->intensity; ps.pdf = r1.w;
    return true;
}

/* One lane per hit, one wave per workgroup, as k_light_rays<STAGED>: the wave's 64 * R rays are made in LDS at the odd pitch 2 R + 1
 * pieces over zeros — the null rays of every slot without a ray — and stored as one contiguous block, lane i on the i-th 16-B piece.
 * R <= RTR_PICK_MAX + 1 = 31 always fits the stage (63 KiB), so there is no unstaged form.  The slots go out as the lane draws them,
 * P words at the 4 P-byte lane stride: 8 B per hit beside 64 B of rays at P = 1. */
__global__ __launch_bounds__(kLightRaysBlock) void k_light_rays_picked(DeviceScene sc, PickArgs pa) {
    extern __shared__ rtr_q4 s_pick_stage[];
    typedef __attribute__((address_space(3))) rtr_q4* lds_q4;
    const lds_q4 stage = (lds_q4)s_pick_stage;
    const LightArgs& la = pa.la;
    const uint32_t lane = threadIdx.x;
    const uint64_t k0 = (uint64_t)blockIdx.x * kLightRaysBlock;
    const bool live = k0 + lane < la.n;
    const uint32_t k = (uint32_t)(k0 + lane);
    const uint32_t P = pa.picks, R = P + 1u, pieces = 2u * R, pitch = pieces + 1u;
    rtr_q4* __restrict__ out = reinterpret_cast<rtr_q4*>(la.outRays) + k0 * pieces;          /* the wave's block */
    const rtr_q4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t i = lane; i < kLightRaysBlock * pitch; i += kLightRaysBlock) stage[i] = zero;
    __syncthreads();
    if (live) {
        HitRec h;
        rtr_v3 dir;
        RenderArgs ra{};
        const bool object = light_hit(sc, la, k, h, dir, ra) == RTR_SURFACE_OBJECT;
        Accum acc;
        Surface sf;
        LocalStats st;
        rtr_v3 shadowOrigin = rtr_mk(0, 0, 0);
        if (object) {
            fetch_surface<false, false>(sc, ra, h, dir, false, acc, sf, st);
            shadowOrigin = rtr_madd(sf.hitPoint, sf.hitNormal, 0.01f);
        }
        const lds_q4 row = stage + lane * pitch;
        for (uint32_t p = 0; p < P; ++p) {
            const size_t at = (size_t)k * P + p;
            /* ra.info.frame is la.frame + the hit's seed base (light_hit) */
            const uint32_t j = pa.slotsIn ? pa.slotsIn[at] : rtr_pick_slot(ra.info.frame, pa.depth, p, pa.areaSlots);
            pa.outSlots[at] = j;
            PickedSample ps;
            if (object && j < pa.areaSlots && picked_sample(sc, pa, ra, sf.hitPoint, j, ps)) {
                row[2u * p] = rtr_q4{shadowOrigin.x, shadowOrigin.y, shadowOrigin.z, 0.001f};
                row[2u * p + 1u] = rtr_q4{ps.dir.x, ps.dir.y, ps.dir.z, ps.dist - 0.5f};
            }
        }
        const rtr_v3 directLightDir = directional_light_dir();
        if (object && !(rtr_dot(sf.hitNormal, directLightDir) <= 0.0f)) {
            row[2u * P] = rtr_q4{shadowOrigin.x, shadowOrigin.y, shadowOrigin.z, 0.001f};
            row[2u * P + 1u] = rtr_q4{directLightDir.x, directLightDir.y, directLightDir.z, 10000.0f};
        }
    }
    __syncthreads();
    const uint64_t left = la.n - k0;
    const uint32_t total = (uint32_t)(left < (uint64_t)kLightRaysBlock ? left : (uint64_t)kLightRaysBlock) * pieces;
    /* piece p of the block belongs to row p / pieces: kept as (row, rest) and stepped by 64 pieces, one division per lane */
    const uint32_t stepRow = (uint32_t)kLightRaysBlock / pieces, stepRest = (uint32_t)kLightRaysBlock % pieces;
    uint32_t row = lane / pieces, rest = lane % pieces;
    for (uint32_t p = lane; p < total; p += kLightRaysBlock) {
        out[p] = stage[row * pitch + rest];
        row += stepRow; rest += stepRest;
        if (rest >= pieces) { rest -= pieces; ++row; }
    }
}

hipError_t launch_light_rays_picked(const DeviceScene& sc, const PickArgs& pa, hipStream_t s) {
    const uint32_t blocks = (uint32_t)(((uint64_t)pa.la.n + kLightRaysBlock - 1) / kLightRaysBlock);
    const size_t lds = (size_t)kLightRaysBlock * (2u * (pa.picks + 1u) + 1u) * sizeof(rtr_q4);
    if (pa.picks == 0u || pa.picks + 1u > kLightStagedSlots || lds > kLightStagedLds) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_light_rays_picked, dim3(blocks), dim3(kLightRaysBlock), lds, s, sc, pa);
    return hipGetLastError();
}

/* One lane per hit: k_shade_hits' record from the picks.  The sky, a light's colour and kind are fetch_surface<true>'s; at an object
 * acc = 0, then acc = fma(contrib_p, occluded ? 0 : w_p, acc) for p = 0 ... P - 1 in order, then the directional term as light_loops adds
 * it.  An occluded sample's BRDF is skipped unless the unshadowed sum is wanted (light_loops' rule, divergence D6).  With one light
 * triangle, one sample and one pick of weight 1 every operation is the full loops' (x * 1, x / 1 and 0 + x give x back). */
__global__ __launch_bounds__(kShadeBlock) void k_shade_hits_picked(DeviceScene sc, PickArgs pa) {
    const LightArgs& la = pa.la;
    const uint32_t k = blockIdx.x * kShadeBlock + threadIdx.x;
    if (k >= la.n) return;
    HitRec h;
    rtr_v3 dir;
    RenderArgs ra{};
    const uint32_t kind = light_hit(sc, la, k, h, dir, ra);
    const bool wantUnshadowed = (la.outputs & RTR_LIGHT_UNSHADOWED) != 0u;
    const rtr_v3 zero = rtr_mk(0, 0, 0);
    const uint32_t P = pa.picks, R = P + 1u;
    Accum acc;
    acc.analytic = acc.shadowed = acc.unshadowed = acc.avgNormal = acc.avgPosition = zero;
    Surface sf;
    LocalStats st;
    if (kind != RTR_SURFACE_INVALID && fetch_surface<true, false>(sc, ra, h, dir, false, acc, sf, st)) {
        const rtr_v3 currDiffuse = sf.diffuse;
        const uint8_t* occ = la.occluded + (size_t)k * R;
        rtr_v3 sumShadowed = zero, sumUnshadowed = zero;
        for (uint32_t p = 0; p < P; ++p) {
            const size_t at = (size_t)k * P + p;
            const uint32_t j = pa.slotsIn[at];
            PickedSample ps;
            if (j >= pa.areaSlots || !picked_sample(sc, pa, ra, sf.hitPoint, j, ps)) continue;
            const bool occluded = occ[p] != 0;
            if (wantUnshadowed || !occluded) {
                const float w = pa.weights ? pa.weights[at] : pa.defaultWeight;
                const rtr_v3 contrib = area_sample_contrib(sf.hitNormal, sf.viewDir, sf.roughness, sf.mSpecular, currDiffuse, ps.lcol, ps.lintensity, ps.pdf, ps.dir, ps.dist);
                sumShadowed = rtr_madd(sumShadowed, contrib, occluded ? 0.0f : w);
                sumUnshadowed = rtr_madd(sumUnshadowed, contrib, w);
            }
        }
        acc.shadowed = rtr_add(acc.shadowed, sumShadowed);
        acc.unshadowed = rtr_add(acc.unshadowed, sumUnshadowed);
        if (!(rtr_dot(sf.hitNormal, directional_light_dir()) <= 0.0f)) {      /* raygen.rgen:289-338, as light_loops */
            const bool occluded = occ[P] != 0;
            if (wantUnshadowed || !occluded) {
                const rtr_v3 contrib = directional_contrib(sf.hitNormal, sf.viewDir, sf.roughness, sf.mSpecular, currDiffuse);
                acc.shadowed = rtr_madd(acc.shadowed, contrib, occluded ? 0.0f : 1.0f);
                acc.unshadowed = rtr_add(acc.unshadowed, contrib);
            }
        }
    }
    if (!wantUnshadowed) acc.unshadowed = zero;
    float4* o = la.out + 3 * (size_t)k;
    o[0] = make_float4(acc.shadowed.x, acc.shadowed.y, acc.shadowed.z, __uint_as_float(kind));
    o[1] = make_float4(acc.unshadowed.x, acc.unshadowed.y, acc.unshadowed.z, 0.0f);
    o[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

hipError_t launch_shade_hits_picked(const DeviceScene& sc, const PickArgs& pa, hipStream_t s) {
    hipLaunchKernelGGL(k_shade_hits_picked, dim3((uint32_t)(((uint64_t)pa.la.n + kShadeBlock - 1) / kShadeBlock)), dim3(kShadeBlock), 0, s, sc, pa);
    return hipGetLastError();
}

/* ---- MIS weights of the picks (rtr_mis_pick_weights; the rule is include/rtr_mis.h) -------------------------------------------------
 * One lane per hit: for each pick the weight rtr_shade_hits_picked is to give it when the vertex's bounce ray counts the lights it
 * meets (rtr_emitter_hits) — the default weight times the balance heuristic's wPick.  The hit, the surface and the sample are
 * light_hit, fetch_surface and picked_sample, called as k_shade_hits_picked calls them, so the direction and the distance are the ones
 * its contribution is evaluated at; the triangle's area and normal are words of the record picked_sample reads.  The bounce density of
 * the pick's direction is rtr_mis_bounce_pdf on the words of the RtrSurface k_hit_surfaces writes for this hit (position, normal,
 * colour, roughness, metallic) and the ray's origin.  A slot is the caller's (pa.slotsIn) or drawn by the rule k_light_rays_picked
 * draws by.  Every weight and, when asked for, every RtrMisSample is written: zeros for a pick without a ray.
 * POWER (rtr_mis_pick_weights_power; the rule is include/rtr_power.h): the slots are always the caller's, and the weight is wPow * wPick
 * with the probability of the slot's triangle read from the scene's power table (ma.cdf, two 8-B gathers per pick).  The uniform
 * instantiation reads nothing of the table and computes what it computed. */
template <bool POWER>
__global__ __launch_bounds__(kShadeBlock) void k_mis_pick_weights(DeviceScene sc, MisPickArgs ma) {
    const PickArgs& pa = ma.pa;
    const LightArgs& la = pa.la;
    const uint32_t k = blockIdx.x * kShadeBlock + threadIdx.x;
    if (k >= la.n) return;
    HitRec h;
    rtr_v3 dir;
    RenderArgs ra{};
    const bool object = light_hit(sc, la, k, h, dir, ra) == RTR_SURFACE_OBJECT;
    const uint32_t P = pa.picks;
    Accum acc;
    Surface sf;
    LocalStats st;
    RtrRay ray{};
    RtrSurface rs{};
    if (object) {
        /* <true>: with the colour and the material, which the density reads (acc is only written at a miss or a light) */
        fetch_surface<true, false>(sc, ra, h, dir, false, acc, sf, st);
        ray.origin[0] = ra.cam.position[0]; ray.origin[1] = ra.cam.position[1]; ray.origin[2] = ra.cam.position[2];
        rs.position[0] = sf.hitPoint.x; rs.position[1] = sf.hitPoint.y; rs.position[2] = sf.hitPoint.z; rs.kind = RTR_SURFACE_OBJECT;
        rs.normal[0] = sf.hitNormal.x; rs.normal[1] = sf.hitNormal.y; rs.normal[2] = sf.hitNormal.z;
        rs.color[0] = sf.color.x; rs.color[1] = sf.color.y; rs.color[2] = sf.color.z;
        rs.roughness = sf.roughness; rs.metallic = sf.metallic;
    }
    for (uint32_t p = 0; p < P; ++p) {
        const size_t at = (size_t)k * P + p;
        /* ra.info.frame is la.frame + the hit's seed base (light_hit) */
        const uint32_t j = pa.slotsIn ? pa.slotsIn[at] : rtr_pick_slot(ra.info.frame, pa.depth, p, pa.areaSlots);
        float w = 0.0f;
        float4 m0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m1 = m0;
        PickedSample ps;
        if (object && j < pa.areaSlots && picked_sample(sc, pa, ra, sf.hitPoint, j, ps)) {
            const uint32_t t = j / la.numShadowRays;
            const float4* rec = sc.lightTris + (size_t)t * kLightTriRecord;
            const float area = rec[0].w;
            const float cosLight = rtr_dot(f4xyz(rec[3]), rtr_neg(ps.dir));
            const float pb = rtr_mis_bounce_pdf(&ray, &rs, ps.dir, ma.lobes);
            float lightPdf, wPick, wBounce, wt;
            if (POWER) {
                wt = rtr_power_mis_pick(ma.cdf, ma.tris, t, P, pb, ps.dist, cosLight, area, &lightPdf, &wPick);
            } else {
                rtr_mis_weights(pb, ps.dist, cosLight, area, ma.tris, P, &lightPdf, &wPick, &wBounce);
                wt = pa.defaultWeight * wPick;
            }
            if (rtr_bounce_finite(wt) & rtr_bounce_finite(ps.dist) & rtr_bounce_finite(cosLight) & rtr_bounce_finite(area) & rtr_bounce_finite3(ps.dir)) {
                w = wt;
                m0 = make_float4(lightPdf, pb, wPick, cosLight);
                m1 = make_float4(ps.dist, area, __uint_as_float(t), 0.0f);
            }
        }
        ma.outWeights[at] = w;
        if (ma.outSamples) { ma.outSamples[2 * at] = m0; ma.outSamples[2 * at + 1] = m1; }
    }
}

hipError_t launch_mis_pick_weights(const DeviceScene& sc, const MisPickArgs& ma, hipStream_t s) {
    if (ma.pa.picks == 0u || ma.pa.picks > RTR_PICK_MAX) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)(((uint64_t)ma.pa.la.n + kShadeBlock - 1) / kShadeBlock));
    if (ma.cdf) {
        if (!ma.pa.slotsIn) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_mis_pick_weights<true>, grid, dim3(kShadeBlock), 0, s, sc, ma);
    } else {
        hipLaunchKernelGGL(k_mis_pick_weights<false>, grid, dim3(kShadeBlock), 0, s, sc, ma);
    }
    return hipGetLastError();
}

/* ---- resampled light picks (rtr_pick_slots_ris; the rule is include/rtr_ris.h) -------------------------------------------------------
 * One lane per hit: light_hit and fetch_surface<true> once, then for each of the P picks M candidates from the scene's power table
 * (ma.cdf: the two searches of k_pick_slots_power), each given its target — picked_sample and area_sample_contrib called as
 * k_shade_hits_picked calls them, so the target is the largest channel of the very bits the shader multiplies later; MIS: times the
 * wPick k_mis_pick_weights<true> computes for the slot, by the same calls under the same guard — and passed through the header's
 * reservoir.  The loop state of a pick is the reservoir's four scalars: nothing is indexed by j, so nothing goes to scratch.  Every
 * slot and weight of every hit is written: RTR_PICK_NONE and 0 at a hit that is not an object.  SAMPLES: the candidates and their
 * targets as used go out too, the candidates for every hit (they are functions of the seeds alone), 0 targets where the hit is no
 * object; the forms without SAMPLES contain none of these stores. */
template <bool MIS, bool SAMPLES>
__global__ __launch_bounds__(kShadeBlock) void k_pick_slots_ris(DeviceScene sc, RisArgs a) {
    const MisPickArgs& ma = a.ma;
    const PickArgs& pa = ma.pa;
    const LightArgs& la = pa.la;
    const uint32_t k = blockIdx.x * kShadeBlock + threadIdx.x;
    if (k >= la.n) return;
    HitRec h;
    rtr_v3 dir;
    RenderArgs ra{};
    const bool object = light_hit(sc, la, k, h, dir, ra) == RTR_SURFACE_OBJECT;
    const uint32_t P = pa.picks, M = a.candidates;
    const uint64_t* __restrict__ cdf = ma.cdf;
    Accum acc;
    Surface sf;
    LocalStats st;
    RtrRay ray{};
    RtrSurface rs{};
    if (object) {
        fetch_surface<true, false>(sc, ra, h, dir, false, acc, sf, st);
        if (MIS) {      /* the words of the RtrSurface k_hit_surfaces writes for this hit, as k_mis_pick_weights fills them */
            ray.origin[0] = ra.cam.position[0]; ray.origin[1] = ra.cam.position[1]; ray.origin[2] = ra.cam.position[2];
            rs.position[0] = sf.hitPoint.x; rs.position[1] = sf.hitPoint.y; rs.position[2] = sf.hitPoint.z; rs.kind = RTR_SURFACE_OBJECT;
            rs.normal[0] = sf.hitNormal.x; rs.normal[1] = sf.hitNormal.y; rs.normal[2] = sf.hitNormal.z;
            rs.color[0] = sf.color.x; rs.color[1] = sf.color.y; rs.color[2] = sf.color.z;
            rs.roughness = sf.roughness; rs.metallic = sf.metallic;
        }
    }
    const uint64_t total = rtr_power_total(cdf, ma.tris);
    for (uint32_t p = 0; p < P; ++p) {
        const size_t at = (size_t)k * P + p;
        rtr_ris_reservoir res;
        rtr_ris_begin(&res);
        if (object || SAMPLES) {
            for (uint32_t j = 0; j < M; ++j) {
                /* ra.info.frame is la.frame + the hit's seed base (light_hit) */
                uint32_t weightT;
                const uint32_t slot = rtr_ris_candidate(cdf, ma.tris, la.numShadowRays, ra.info.frame, pa.depth, p, j, &weightT);
                float target = 0.0f, wPick = 0.0f;
                PickedSample ps;
                if (object && slot != RTR_PICK_NONE && picked_sample(sc, pa, ra, sf.hitPoint, slot, ps)) {
                    const rtr_v3 contrib = area_sample_contrib(sf.hitNormal, sf.viewDir, sf.roughness, sf.mSpecular, sf.diffuse, ps.lcol, ps.lintensity, ps.pdf, ps.dir, ps.dist);
                    float phat = rtr_bounce_max3(contrib);
                    if (MIS) {
                        const uint32_t t = slot / la.numShadowRays;
                        const float4* rec = sc.lightTris + (size_t)t * kLightTriRecord;
                        const float area = rec[0].w;
                        const float cosLight = rtr_dot(f4xyz(rec[3]), rtr_neg(ps.dir));
                        const float pb = rtr_mis_bounce_pdf(&ray, &rs, ps.dir, ma.lobes);
                        float lightPdf, wp;
                        const float wt = rtr_power_mis_pick(cdf, ma.tris, t, P, pb, ps.dist, cosLight, area, &lightPdf, &wp);
                        if (rtr_bounce_finite(wt) & rtr_bounce_finite(ps.dist) & rtr_bounce_finite(cosLight) & rtr_bounce_finite(area) & rtr_bounce_finite3(ps.dir)) wPick = wp;
                        phat = phat * wPick;
                    }
                    target = rtr_ris_target(phat);
                    rtr_ris_step(&res, total, weightT, slot, target, wPick, rtr_ris_number(ra.info.frame, pa.depth, p, j));
                }
                if (SAMPLES) { a.outCandidates[at * M + j] = slot; a.outTargets[at * M + j] = target; }
            }
        }
        float w;
        pa.outSlots[at] = rtr_ris_finish(&res, M, P, MIS ? 1u : 0u, &w);
        ma.outWeights[at] = w;
    }
}

hipError_t launch_pick_slots_ris(const DeviceScene& sc, const RisArgs& a, hipStream_t s) {
    if (a.ma.pa.picks == 0u || a.ma.pa.picks > RTR_PICK_MAX || a.candidates == 0u || a.candidates > RTR_RIS_MAX_CANDIDATES || !a.ma.cdf ||
        !a.outCandidates != !a.outTargets)
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)(((uint64_t)a.ma.pa.la.n + kShadeBlock - 1) / kShadeBlock));
    const bool samples = a.outCandidates != nullptr;
    if (a.mis) {
        if (samples) hipLaunchKernelGGL((k_pick_slots_ris<true, true>), grid, dim3(kShadeBlock), 0, s, sc, a);
        else hipLaunchKernelGGL((k_pick_slots_ris<true, false>), grid, dim3(kShadeBlock), 0, s, sc, a);
    } else {
        if (samples) hipLaunchKernelGGL((k_pick_slots_ris<false, true>), grid, dim3(kShadeBlock), 0, s, sc, a);
        else hipLaunchKernelGGL((k_pick_slots_ris<false, false>), grid, dim3(kShadeBlock), 0, s, sc, a);
    }
    return hipGetLastError();
}

}  // namespace rtrdev
