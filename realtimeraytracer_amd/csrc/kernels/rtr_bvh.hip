/* rtr_bvh.hip — BVH build and refit ON the device.
 *
 * Replaces what the reference leaves to the driver: vkCmdBuildAccelerationStructuresKHR for BLAS/TLAS
 * (src/vulkan/raytracing/blas.cppm:113-160, tlas.cppm:112-149) and TLAS::updateTransform / refit
 * (tlas.cppm:151-207 — present in the reference, never called by its app).
 *
 *   build  : LBVH (Karras 2012).  k_world_prims flattens instances to world space (same arithmetic as the host
 *            packer) and reduces centroid bounds; 30-bit Morton code | primitive index as a unique 64-bit key;
 *            rocPRIM/hipCUB radix sort (a plain library sort, the one step that is not hand-written);
 *            k_karras builds the radix tree, one lane per internal node; subtrees of <= 4 primitives collapse into
 *            leaves (Morton-sorted primitives of a subtree are contiguous, so a leaf is (first,count) as in the
 *            host builder); k_fit fits the child boxes bottom-up.
 *   refit  : k_world_prims again with new transforms into the existing leaf order, then k_fit on the unchanged
 *            topology (works for host-SAH-built and device-LBVH-built trees alike).
 *
 * k_fit: one lane per inner node fills the slots of its leaf children, then climbs: an agent-scope
 * fence + atomic counter per node lets exactly the second arriver continue with both child boxes visible
 * (cdna guide G16: visibility comes from the release/acquire pair, not from placement).  Every climb ends at the
 * root or at a node whose sibling has not arrived, so all waves exit.
 * Output layout = RTR_BVH_LAYOUT_VERSION 2 (64-B children-in-parent nodes, 48-B {v0,e1,e2} records), boxes padded
 * outwards by 2^-18 of the largest coordinate like the host builder, so traversal results are identical whichever
 * builder made the tree.
 */
#include "rtr_bvh.h"

#include <hipcub/hipcub.hpp>

#include "../../../include/rtr_math.h"
#include "rtr_mirrored.h"
#include "rtr_tree_sah.h"
#include "rtr_hot_top.h"

namespace rtrdev {

constexpr int kB = 256;
constexpr uint32_t kLeafMax = 4;

__device__ __forceinline__ uint32_t f2ord(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline float ord2f(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f; memcpy(&f, &u, 4); return f;
}

/* scene reduction words: [0..2] centroid min (ordered uint), [3..5] centroid max, [6] max |coordinate| (float bits, >= 0) */
__global__ __launch_bounds__(kB) void k_world_prims(BvhInputs in, uint32_t n, const uint32_t* __restrict__ slotOfPrim,
                                                    float4* __restrict__ triOut, float4* __restrict__ boxMin, float4* __restrict__ boxMax,
                                                    uint32_t* __restrict__ red, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;                         /* a gated launch whose decision word says no: nothing is read or written */
    const uint32_t p = blockIdx.x * kB + threadIdx.x;
    float cmin[3] = {3.0e38f, 3.0e38f, 3.0e38f}, cmax[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, mabs = 0.f;
    if (p < n) {
        const PrimRef pr = in.prims[p];
        const InstanceRef ir = in.instances[pr.customIndex];
        rtr_v3 w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t idx = in.indices[ir.indexOffset + 3u * pr.primitiveId + k] + ir.vertexOffset;
            w[k] = rtr_xform_point34(ir.transform, rtr_ld3(in.vertices[idx].position));
        }
        const rtr_v3 e1 = rtr_sub(w[1], w[0]), e2 = rtr_sub(w[2], w[0]);
        const uint32_t s = slotOfPrim ? slotOfPrim[p] : p;          /* refit writes straight into leaf order */
        triOut[(size_t)s * 3 + 0] = make_float4(w[0].x, w[0].y, w[0].z, __uint_as_float(pr.customIndex));
        triOut[(size_t)s * 3 + 1] = make_float4(e1.x, e1.y, e1.z, __uint_as_float(pr.primitiveId));
        triOut[(size_t)s * 3 + 2] = make_float4(e2.x, e2.y, e2.z, __uint_as_float(pr.flags));
        const float mn[3] = {fminf(fminf(w[0].x, w[1].x), w[2].x), fminf(fminf(w[0].y, w[1].y), w[2].y), fminf(fminf(w[0].z, w[1].z), w[2].z)};
        const float mx[3] = {fmaxf(fmaxf(w[0].x, w[1].x), w[2].x), fmaxf(fmaxf(w[0].y, w[1].y), w[2].y), fmaxf(fmaxf(w[0].z, w[1].z), w[2].z)};
        boxMin[s] = make_float4(mn[0], mn[1], mn[2], 0.f);
        boxMax[s] = make_float4(mx[0], mx[1], mx[2], 0.f);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = 0.5f * (mn[k] + mx[k]);
            cmin[k] = c; cmax[k] = c;
            mabs = fmaxf(mabs, fmaxf(fabsf(mn[k]), fabsf(mx[k])));
        }
    }
    /* wave reduction, then one atomic per wave and word */
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { cmin[k] = fminf(cmin[k], __shfl_xor(cmin[k], o)); cmax[k] = fmaxf(cmax[k], __shfl_xor(cmax[k], o)); }
        mabs = fmaxf(mabs, __shfl_xor(mabs, o));
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&red[k], f2ord(cmin[k])); atomicMax(&red[3 + k], f2ord(cmax[k])); }
        atomicMax(&red[6], __float_as_uint(mabs));
    }
}

__device__ __forceinline__ uint32_t expand10(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__global__ __launch_bounds__(kB) void k_morton(uint32_t n, const float4* __restrict__ boxMin, const float4* __restrict__ boxMax,
                                               const uint32_t* __restrict__ red, unsigned long long* __restrict__ keys, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t p = blockIdx.x * kB + threadIdx.x;
    if (p >= n) return;
    const float4 a = boxMin[p], b = boxMax[p];
    const float c[3] = {0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z)};
    uint32_t q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = ord2f(red[k]), hi = ord2f(red[3 + k]);
        const float ext = hi - lo;
        float t = ext > 0.f ? (c[k] - lo) / ext : 0.f;
        t = fminf(fmaxf(t * 1024.0f, 0.0f), 1023.0f);
        q[k] = (uint32_t)t;
    }
    const uint32_t m = (expand10(q[0]) << 2) | (expand10(q[1]) << 1) | expand10(q[2]);
    keys[p] = ((unsigned long long)m << 32) | p;
}

/* gather the canonical-order records into Morton order and remember where every canonical primitive went */
__global__ __launch_bounds__(kB) void k_gather(uint32_t n, const unsigned long long* __restrict__ keys,
                                               const float4* __restrict__ triIn, const float4* __restrict__ minIn, const float4* __restrict__ maxIn,
                                               float4* __restrict__ triOut, float4* __restrict__ minOut, float4* __restrict__ maxOut,
                                               uint32_t* __restrict__ slotOfPrim, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = (uint32_t)(keys[i] & 0xffffffffull);
    triOut[(size_t)i * 3 + 0] = triIn[(size_t)p * 3 + 0];
    triOut[(size_t)i * 3 + 1] = triIn[(size_t)p * 3 + 1];
    triOut[(size_t)i * 3 + 2] = triIn[(size_t)p * 3 + 2];
    minOut[i] = minIn[p]; maxOut[i] = maxIn[p];
    slotOfPrim[p] = i;
}

/* Karras 2012: longest common prefix of the (unique) keys i and j, -1 outside [0,n) */
__device__ __forceinline__ int lcp(const unsigned long long* __restrict__ keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    return __clzll((long long)(keys[i] ^ keys[j]));
}

__device__ __forceinline__ int32_t leaf_code(uint32_t first, uint32_t count) { return (int32_t)~((first << 3) | (count - 1u)); }

/* one lane per internal node: range, split, children; child codes with <=4-primitive subtrees collapsed to leaves */
__global__ __launch_bounds__(kB) void k_karras(int n, const unsigned long long* __restrict__ keys, int2* __restrict__ range,
                                               int2* __restrict__ rawChild /* index, with bit 31 = primitive leaf */, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n - 1) return;
    const int d = (lcp(keys, n, i, i + 1) - lcp(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = lcp(keys, n, i, i - d);
    int lmax = 2;
    while (lcp(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (lcp(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = lcp(keys, n, i, j);
    int s = 0;
    for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
        if (lcp(keys, n, i, i + (s + t) * d) > dnode) s += t;
        if (t == 1) break;
    }
    const int gamma = i + s * d + (d < 0 ? -1 : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    range[i] = make_int2(lo, hi);
    rawChild[i] = make_int2(lo == gamma ? (gamma | (int)0x80000000) : gamma, hi == gamma + 1 ? ((gamma + 1) | (int)0x80000000) : gamma + 1);
}

__global__ __launch_bounds__(kB) void k_mark_unused(uint32_t numNodes, int32_t* __restrict__ parent, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i < numNodes) parent[i] = -2;
}

/* child codes in the final node array + parent links for the climb */
__global__ __launch_bounds__(kB) void k_emit(int n, const int2* __restrict__ range, const int2* __restrict__ rawChild,
                                             float4* __restrict__ nodes, int32_t* __restrict__ parent, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n - 1) return;
    const int2 r = range[i];
    if ((uint32_t)(r.y - r.x + 1) <= kLeafMax && i != 0) return;        /* inside / root of a collapsed subtree: never referenced */
    const int2 rc = rawChild[i];
    int32_t code[2];
    const int raw[2] = {rc.x, rc.y};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (raw[s] < 0) code[s] = leaf_code((uint32_t)(raw[s] & 0x7fffffff), 1u);
        else {
            const int2 cr = range[raw[s]];
            const uint32_t cnt = (uint32_t)(cr.y - cr.x + 1);
            if (cnt <= kLeafMax) code[s] = leaf_code((uint32_t)cr.x, cnt);
            else { code[s] = raw[s]; parent[raw[s]] = (i << 1) | s; }
        }
    }
    int4 w = make_int4(code[0], code[1], 0, 0);
    nodes[(size_t)i * 4 + 3] = *reinterpret_cast<float4*>(&w);
    if (i == 0) parent[0] = -1;
}

/* bottom-up fit (build and refit).  counters must be zero on entry; depth[] gets the inner-node height. */
__global__ __launch_bounds__(kB) void k_fit(uint32_t numNodes, float4* nodes, const float4* __restrict__ boxMin, const float4* __restrict__ boxMax,
                                            const int32_t* __restrict__ parent, uint32_t* counters, uint32_t* depth, const uint32_t* __restrict__ red,
                                            uint32_t* maxDepthOut, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= numNodes) return;
    const int32_t par0 = parent[i];
    if (par0 == -2) return;                                   /* slot of the node array that is not part of the tree */
    const float pad = fmaxf(__uint_as_float(red[6]), 1e-6f) * 3.814697265625e-06f;
    float* nf = reinterpret_cast<float*>(nodes + (size_t)i * 4);
    const int2 ch = *reinterpret_cast<const int2*>(nodes + (size_t)i * 4 + 3);
    uint32_t filled = 0;
    const int32_t code[2] = {ch.x, ch.y};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (code[s] >= 0) continue;
        const uint32_t c = (uint32_t)~code[s];
        const uint32_t first = c >> 3, cnt = (c & 7u) + 1u;
        float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        for (uint32_t k = 0; k < cnt; ++k) {
            const float4 a = boxMin[first + k], b = boxMax[first + k];
            mn[0] = fminf(mn[0], a.x); mn[1] = fminf(mn[1], a.y); mn[2] = fminf(mn[2], a.z);
            mx[0] = fmaxf(mx[0], b.x); mx[1] = fmaxf(mx[1], b.y); mx[2] = fmaxf(mx[2], b.z);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { nf[6 * s + k] = mn[k] - pad; nf[6 * s + 3 + k] = mx[k] + pad; }
        ++filled;
    }
    if (filled == 0) return;                                  /* two inner children: their climbs complete this node */
    uint32_t cur = i;
    uint32_t add = filled;
    for (;;) {
        __threadfence();                                      /* release my slot writes (agent scope) */
        const uint32_t before = atomicAdd(&counters[cur], add);
        if (before + add < 2u) return;                        /* sibling subtree not finished: its lane will continue */
        __threadfence();                                      /* acquire the sibling's writes */
        float* cf = reinterpret_cast<float*>(nodes + (size_t)cur * 4);
        const int2 cc = *reinterpret_cast<const int2*>(nodes + (size_t)cur * 4 + 3);
        const uint32_t dl = cc.x >= 0 ? __hip_atomic_load(&depth[cc.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const uint32_t dr = cc.y >= 0 ? __hip_atomic_load(&depth[cc.y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const uint32_t dcur = 1u + (dl > dr ? dl : dr);
        __hip_atomic_store(&depth[cur], dcur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int32_t p = parent[cur];
        if (p < 0) { *maxDepthOut = dcur; return; }           /* root done */
        const uint32_t pi = (uint32_t)p >> 1, ps = (uint32_t)p & 1u;
        float* pf = reinterpret_cast<float*>(nodes + (size_t)pi * 4);
        /* my box = union of my two child boxes (volatile-style loads through the agent-scope path) */
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = __hip_atomic_load(&cf[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float b = __hip_atomic_load(&cf[6 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float c = __hip_atomic_load(&cf[3 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float d = __hip_atomic_load(&cf[9 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&pf[6 * ps + k], fminf(a, b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&pf[6 * ps + 3 + k], fmaxf(c, d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        cur = pi; add = 1u;
    }
}

/* scene grid from the root's two child boxes (one lane) */
__global__ void k_grid(const float4* __restrict__ nodesF, RtrBvhGrid* grid, const uint32_t* __restrict__ go) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (go && *go == 0u) return;
    const float* f = reinterpret_cast<const float*>(nodesF);
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) { mn[k] = fminf(f[k], f[6 + k]); mx[k] = fmaxf(f[3 + k], f[9 + k]); }
    RtrBvhGrid g = {};
    rtr_grid_from_bounds(mn, mx, g.origin, g.scale);
    *grid = g;
}

/* fp32 planes -> 16-bit grid coordinates, rounded outward (same arithmetic as rtr::quantize_nodes on the host) */
__global__ __launch_bounds__(kB) void k_quantize(uint32_t numNodes, const float4* __restrict__ nodesF, const int32_t* __restrict__ parent,
                                                 const RtrBvhGrid* __restrict__ grid, uint4* __restrict__ nodes, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= numNodes) return;
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = make_uint4(0, 0, 0, 0);
    if (parent[i] != -2) {
        const float4 a = nodesF[(size_t)i * 4], b = nodesF[(size_t)i * 4 + 1], c = nodesF[(size_t)i * 4 + 2];
        const int4 d = *reinterpret_cast<const int4*>(nodesF + (size_t)i * 4 + 3);
        const float ox = grid->origin[0], oy = grid->origin[1], oz = grid->origin[2];
        const float sx = grid->scale[0], sy = grid->scale[1], sz = grid->scale[2];
        /* a = (lminx,lminy,lminz,lmaxx)  b = (lmaxy,lmaxz,rminx,rminy)  c = (rminz,rmaxx,rmaxy,rmaxz) */
        w0.x = rtr_quant_lo(a.x, ox, sx) | (rtr_quant_lo(a.y, oy, sy) << 16);
        w0.y = rtr_quant_hi(a.w, ox, sx) | (rtr_quant_hi(b.x, oy, sy) << 16);
        w0.z = rtr_quant_lo(b.z, ox, sx) | (rtr_quant_lo(b.w, oy, sy) << 16);
        w0.w = rtr_quant_hi(c.y, ox, sx) | (rtr_quant_hi(c.z, oy, sy) << 16);
        w1.x = rtr_quant_lo(a.z, oz, sz) | (rtr_quant_hi(b.y, oz, sz) << 16);
        w1.y = rtr_quant_lo(c.x, oz, sz) | (rtr_quant_hi(c.w, oz, sz) << 16);
        w1.z = (uint32_t)d.x; w1.w = (uint32_t)d.y;
    }
    nodes[(size_t)i * 2] = w0; nodes[(size_t)i * 2 + 1] = w1;
}

/* f16 bits of a signed plane offset v (scene-grid steps from the scene's wide centre, |v| <= 65535), rounded towards -inf / +inf to
 * the 11 significant bits of a half float; a magnitude past the largest half float (65504) rounds away from zero to infinity and
 * towards zero to 65504.  Integer arithmetic, so a host restatement agrees bit for bit. */
__host__ __device__ inline uint32_t rtr_f16_bits_of_int(uint32_t a) {      /* a has at most 11 significant bits; a > 65504 (only 65536 can arrive) -> inf */
    if (a == 0) return 0u;
    if (a > 65504u) return 0x7c00u;
    const int e = 31 - __builtin_clz(a);                                   /* a = 1.m * 2^e, e <= 15 */
    const uint32_t m = (e >= 10) ? (a >> (e - 10)) : (a << (10 - e));      /* 11 bits, leading one at bit 10 */
    return ((uint32_t)(e + 15) << 10) | (m & 0x3ffu);
}
__host__ __device__ inline uint32_t rtr_f16_mag_down(uint32_t a) {          /* largest representable <= a */
    if (a <= 2048u) return a;
    if (a > 65504u) return 65504u;
    const int sh = (31 - __builtin_clz(a)) - 10;
    return (a >> sh) << sh;
}
__host__ __device__ inline uint32_t rtr_f16_mag_up(uint32_t a) {            /* smallest representable >= a */
    if (a <= 2048u) return a;
    const int sh = (31 - __builtin_clz(a)) - 10;
    return ((a + (1u << sh) - 1u) >> sh) << sh;
}
__host__ __device__ inline uint32_t rtr_f16_floor_bits(int32_t v) {         /* towards -inf */
    return v >= 0 ? rtr_f16_bits_of_int(rtr_f16_mag_down((uint32_t)v)) : (0x8000u | rtr_f16_bits_of_int(rtr_f16_mag_up((uint32_t)(-v))));
}
__host__ __device__ inline uint32_t rtr_f16_ceil_bits(int32_t v) {          /* towards +inf */
    return v >= 0 ? rtr_f16_bits_of_int(rtr_f16_mag_up((uint32_t)v)) : (0x8000u | rtr_f16_bits_of_int(rtr_f16_mag_down((uint32_t)(-v))));
}

/* The wide centre of a tree: the grid coordinate c (per axis) the 4-wide records' half-float planes are offsets from.  Half floats
 * are exact within 2048 steps of c and lose a bit per doubling beyond, so c decides where the boxes stay tight.  Two candidates per
 * axis, both from the tree's leaf boxes (integer sums in 64-bit atomics: the same bytes on every run):
 *   mean : the mean midpoint of the leaf boxes — tight where most leaves are;
 *   flat : the 4096-step window holding the most face area of leaves that are FLAT on this axis (extent <= 2 steps: floors, walls).
 *          A flat leaf whose planes move outward by more than the 0.01 a shadow ray is lifted off its surface swallows the origin
 *          of every ray leaving that surface; on the bunny-class scene (a small object on a large ground plane, planes about the
 *          grid's own centre) that cost +47 % node visits and +125 % triangle tests per shadow ray.
 * The flat candidate is taken on an axis where it cuts the area-weighted relative inflation of the leaf boxes (capped at the
 * box's own extent) to a quarter or less of the mean candidate's — measured choices and counts in profiles/r02/wide_centre.log. */
constexpr uint32_t kCentreBins = 512;                 /* of 128 grid steps */
constexpr uint32_t kCentreWindow = 32;                /* bins: the +-2048 steps a half float holds exactly */
constexpr uint32_t kCentreWords = 4 + 3 * kCentreBins + 6 + 6;    /* sums[4], flat-area histograms, candidates [axis][2], costs [axis][2] */

struct LeafBox { uint32_t lo[3], hi[3]; };
__device__ __forceinline__ int leaf_boxes(uint32_t i, uint32_t numNodes, const uint4* __restrict__ nodes, const int32_t* __restrict__ parent, LeafBox out[2]) {
    int n = 0;
    if (i < numNodes && (!parent || parent[i] != -2)) {
        const uint4 a = nodes[(size_t)i * 2], b = nodes[(size_t)i * 2 + 1];
        if ((int32_t)b.z < 0) { LeafBox& l = out[n++]; l.lo[0] = a.x & 0xffffu; l.lo[1] = a.x >> 16; l.lo[2] = b.x & 0xffffu; l.hi[0] = a.y & 0xffffu; l.hi[1] = a.y >> 16; l.hi[2] = b.x >> 16; }
        if ((int32_t)b.w < 0) { LeafBox& l = out[n++]; l.lo[0] = a.z & 0xffffu; l.lo[1] = a.z >> 16; l.lo[2] = b.y & 0xffffu; l.hi[0] = a.w & 0xffffu; l.hi[1] = a.w >> 16; l.hi[2] = b.y >> 16; }
    }
    return n;
}
__device__ __forceinline__ unsigned long long wave_total(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

__global__ __launch_bounds__(kB) void k_wide_centre_sum(uint32_t numNodes, const uint4* __restrict__ nodes, const int32_t* __restrict__ parent,
                                                        unsigned long long* __restrict__ w, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    LeafBox lb[2];
    const int nl = leaf_boxes(i, numNodes, nodes, parent, lb);
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int j = 0; j < nl; ++j) {
        for (int k = 0; k < 3; ++k) {
            s[k] += lb[j].lo[k] + lb[j].hi[k];
            if (lb[j].hi[k] - lb[j].lo[k] <= 2u) {          /* flat on axis k: its face area goes to the bins of its two planes */
                const int a = (k + 1) % 3, b = (k + 2) % 3;
                const unsigned long long area = (((unsigned long long)(lb[j].hi[a] - lb[j].lo[a]) * (lb[j].hi[b] - lb[j].lo[b])) >> 8) + 1ull;
                atomicAdd(w + 4 + k * kCentreBins + (lb[j].lo[k] >> 7), area);
                atomicAdd(w + 4 + k * kCentreBins + (lb[j].hi[k] >> 7), area);
            }
        }
        s[3] += 2;
    }
    for (int k = 0; k < 4; ++k) { const unsigned long long t = wave_total(s[k]); if ((threadIdx.x & 63u) == 0 && t) atomicAdd(w + k, t); }
}
__global__ void k_wide_centre_candidates(unsigned long long* __restrict__ w, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const unsigned long long n = w[3];
    unsigned long long* cand = w + 4 + 3 * kCentreBins;
    for (int k = 0; k < 3; ++k) {
        unsigned long long mean = 32768ull;
        if (n) { mean = (w[k] + n / 2) / n; if (mean > 65535ull) mean = 65535ull; }
        const unsigned long long* h = w + 4 + k * kCentreBins;
        unsigned long long run = 0, best = 0; uint32_t bestStart = 0;
        for (uint32_t b = 0; b < kCentreBins; ++b) {
            run += h[b];
            if (b >= kCentreWindow) run -= h[b - kCentreWindow];
            if (b + 1 >= kCentreWindow && run > best) { best = run; bestStart = b + 1 - kCentreWindow; }      /* ties: the lowest window */
        }
        cand[2 * k] = mean;
        cand[2 * k + 1] = best ? (unsigned long long)(bestStart * 128u + 2048u) : mean;
    }
}
/* outward movement of a plane q stored as a half float about c, in grid steps */
__device__ __forceinline__ uint32_t plane_slack_lo(uint32_t q, uint32_t c) { const int32_t v = (int32_t)q - (int32_t)c; return v >= 0 ? (uint32_t)v - rtr_f16_mag_down((uint32_t)v) : rtr_f16_mag_up((uint32_t)(-v)) - (uint32_t)(-v); }
__device__ __forceinline__ uint32_t plane_slack_hi(uint32_t q, uint32_t c) { const int32_t v = (int32_t)q - (int32_t)c; return v >= 0 ? rtr_f16_mag_up((uint32_t)v) - (uint32_t)v : (uint32_t)(-v) - rtr_f16_mag_down((uint32_t)(-v)); }
__global__ __launch_bounds__(kB) void k_wide_centre_cost(uint32_t numNodes, const uint4* __restrict__ nodes, const int32_t* __restrict__ parent,
                                                         unsigned long long* __restrict__ w, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    const unsigned long long* cand = w + 4 + 3 * kCentreBins;
    LeafBox lb[2];
    const int nl = leaf_boxes(i, numNodes, nodes, parent, lb);
    unsigned long long cost[6] = {0, 0, 0, 0, 0, 0};
    for (int j = 0; j < nl; ++j)
        for (int k = 0; k < 3; ++k) {
            const int a = (k + 1) % 3, b = (k + 2) % 3;
            const unsigned long long area = (((unsigned long long)(lb[j].hi[a] - lb[j].lo[a]) * (lb[j].hi[b] - lb[j].lo[b])) >> 8) + 1ull;
            const uint32_t ext = lb[j].hi[k] - lb[j].lo[k] + 1u;
            for (int c = 0; c < 2; ++c) {
                const uint32_t cc = (uint32_t)cand[2 * k + c];
                const uint32_t slack = plane_slack_lo(lb[j].lo[k], cc) + plane_slack_hi(lb[j].hi[k], cc);
                uint32_t rel = (slack << 8) / ext;                /* relative inflation in 1/256, capped at the box's own extent */
                if (rel > 256u) rel = 256u;
                cost[2 * k + c] += area * rel;
            }
        }
    for (int q = 0; q < 6; ++q) { const unsigned long long t = wave_total(cost[q]); if ((threadIdx.x & 63u) == 0 && t) atomicAdd(w + 4 + 3 * kCentreBins + 6 + q, t); }
}
__global__ void k_wide_centre_set(const unsigned long long* __restrict__ w, RtrBvhGrid* grid, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const unsigned long long* cand = w + 4 + 3 * kCentreBins;
    const unsigned long long* cost = cand + 6;
    uint32_t c[3];
    for (int k = 0; k < 3; ++k) c[k] = (uint32_t)((cost[2 * k + 1] * 4ull <= cost[2 * k]) ? cand[2 * k + 1] : cand[2 * k]);
    grid->wideCentreXY = c[0] | (c[1] << 16);
    grid->wideCentreZ = c[2];
}

/* ---- the SAH cost of the tree the kernels walk (rtr_scene_tree_cost) -------------------------------------------------
 * Integer sums over the quantised BVH2, one lane per node slot; slots that are not part of the tree (parent == -2) are skipped.
 * A child box's extents d = max(0, qmax - qmin) in grid steps give the area triple (dx dy, dy dz, dz dx); the scale factors are
 * applied once, on the host, to the finished sums (rtr_api.cpp, finish_tree_cost), so the words are exact and the same bytes on every
 * run: d <= 65535, count <= 8 and at most 2^25 nodes keep every sum below 2^61.
 *   w[0..2] innerArea : every child slot that holds an inner node, plus the root's own box (the union of its two child boxes)
 *   w[3..5] leafArea  : every child slot that holds a leaf, times its triangle count
 *   w[6..8] rootArea  : the root's box (written by lane 0 of block 0: the root is node 0)
 *   w[9] numInner (the root included)   w[10] numLeafRefs (child slots that hold a leaf)
 * The words are zero on entry.  rtr_host_tree_cost restates the sums on the host. */
constexpr uint32_t kTreeCostWords = 11;
__device__ __forceinline__ void area_triple(const uint32_t lo[3], const uint32_t hi[3], unsigned long long t[3]) {
    unsigned long long d[3];
    for (int k = 0; k < 3; ++k) d[k] = hi[k] > lo[k] ? (unsigned long long)(hi[k] - lo[k]) : 0ull;
    t[0] = d[0] * d[1]; t[1] = d[1] * d[2]; t[2] = d[2] * d[0];
}
__global__ __launch_bounds__(kB) void k_tree_cost(uint32_t numNodes, const uint4* __restrict__ nodes, const int32_t* __restrict__ parent,
                                                  unsigned long long* __restrict__ w, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    unsigned long long s[8] = {0, 0, 0, 0, 0, 0, 0, 0};      /* inner[3], leaf[3], numInner, numLeafRefs */
    if (i < numNodes && (!parent || parent[i] != -2)) {
        const uint4 a = nodes[(size_t)i * 2], b = nodes[(size_t)i * 2 + 1];      /* the 32-byte node: two 16-byte loads */
        const uint32_t lo[2][3] = {{a.x & 0xffffu, a.x >> 16, b.x & 0xffffu}, {a.z & 0xffffu, a.z >> 16, b.y & 0xffffu}};
        const uint32_t hi[2][3] = {{a.y & 0xffffu, a.y >> 16, b.x >> 16}, {a.w & 0xffffu, a.w >> 16, b.y >> 16}};
        const int32_t code[2] = {(int32_t)b.z, (int32_t)b.w};
        unsigned long long t[3];
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) {
            area_triple(lo[sd], hi[sd], t);
            if (code[sd] >= 0) { s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[6] += 1ull; }
            else {
                const unsigned long long cnt = ((uint32_t)~code[sd] & 7u) + 1u;
                s[3] += cnt * t[0]; s[4] += cnt * t[1]; s[5] += cnt * t[2]; s[7] += 1ull;
            }
        }
        if (i == 0) {
            uint32_t rlo[3], rhi[3];
            for (int k = 0; k < 3; ++k) { rlo[k] = lo[0][k] < lo[1][k] ? lo[0][k] : lo[1][k]; rhi[k] = hi[0][k] > hi[1][k] ? hi[0][k] : hi[1][k]; }
            area_triple(rlo, rhi, t);
            s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[6] += 1ull;
            w[6] = t[0]; w[7] = t[1]; w[8] = t[2];               /* no other lane writes these words */
        }
    }
    for (int q = 0; q < 8; ++q) {
        const unsigned long long tot = wave_total(s[q]);
        if ((threadIdx.x & 63u) == 0 && tot) atomicAdd(w + (q < 6 ? q : q + 3), tot);
    }
}

/* 4-wide view of the tree for the any-hit kernel (rtr_kernels.hip, k_shadow_trace4): entry n starts from the two children of
 * BVH2 node n and, while a slot is free, opens the inner entry with the largest box into its own two children; boxes are
 * copied from the BVH2 nodes that own them and child codes keep BVH2 node ids, so entry 0 roots a complete 4-wide tree.
 * Word layout (16 words = RtrWideNode): per child (xmin|ymin<<16) (xmax|ymax<<16) (zmin|zmax<<16) as half floats about the scene's wide centre (RtrBvhGrid::wideCentreXY / Z),
 * then the four child codes; an empty slot has the code 0x80000000 and an inside-out infinite box. */
__global__ __launch_bounds__(kB) void k_wide_nodes(uint32_t numNodes, const uint4* __restrict__ nodes, const int32_t* __restrict__ parent,
                                                   const RtrBvhGrid* __restrict__ grid, const uint8_t* __restrict__ shape, uint4* __restrict__ wide, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= numNodes) return;
    uint32_t o[16];
    /* an empty slot: the code RTR_WIDE_EMPTY and an inside-out box with infinite planes (min = +inf, max = -inf as half floats),
     * which no ray enters in the kernel's octant forms: those forms skip the test of the code */
    for (int k = 0; k < 4; ++k) { o[k * 3] = 0x7c007c00u; o[k * 3 + 1] = 0xfc00fc00u; o[k * 3 + 2] = 0xfc007c00u; }
    for (int k = 12; k < 16; ++k) o[k] = 0x80000000u;
    if (!parent || parent[i] != -2) {
        const float sx = grid->scale[0], sy = grid->scale[1], sz = grid->scale[2];
        const int32_t cx = (int32_t)(grid->wideCentreXY & 0xffffu), cy = (int32_t)(grid->wideCentreXY >> 16), cz = (int32_t)(grid->wideCentreZ & 0xffffu);
        /* an entry = (owner node, side); its three plane words and its code come from the owner */
        uint32_t own[4]; int side[4]; int k = 2;
        own[0] = own[1] = i; side[0] = 0; side[1] = 1;
        auto words = [&](uint32_t n, int sd, uint32_t& wmin, uint32_t& wmax, uint32_t& wz, int32_t& code) {
            const uint4 a = nodes[(size_t)n * 2], b = nodes[(size_t)n * 2 + 1];
            wmin = sd ? a.z : a.x; wmax = sd ? a.w : a.y; wz = sd ? b.y : b.x; code = (int32_t)(sd ? b.w : b.z);
        };
        auto area = [&](uint32_t wmin, uint32_t wmax, uint32_t wz) {
            const float dx = (float)((wmax & 0xffffu) - (wmin & 0xffffu)) * sx, dy = (float)((wmax >> 16) - (wmin >> 16)) * sy;
            const float dz = (float)((wz >> 16) - (wz & 0xffffu)) * sz;
            return dx * dy + dy * dz + dz * dx;
        };
        if (shape) {
            /* the host builder chose, by cost, which entries this record opens (bvh_build.cpp collapse_wide): open1 | open2 << 2,
             * each the slot to open + 1 (0 = none); an open replaces the entry by its left child and appends its right child */
            const uint32_t sh = shape[i];
            for (int step = 0; step < 2; ++step) {
                const uint32_t o = (sh >> (2 * step)) & 3u;
                if (o == 0u || (int)o > k) break;
                uint32_t wmin, wmax, wz; int32_t code;
                words(own[o - 1u], side[o - 1u], wmin, wmax, wz, code);
                if (code < 0 || (uint32_t)code >= numNodes) break;
                own[o - 1u] = (uint32_t)code; side[o - 1u] = 0;
                own[k] = (uint32_t)code; side[k] = 1; ++k;
            }
        } else
        while (k < 4) {
            int best = -1; float bestA = -1.0f; int32_t bestCode = 0;
            for (int j = 0; j < k; ++j) {
                uint32_t wmin, wmax, wz; int32_t code;
                words(own[j], side[j], wmin, wmax, wz, code);
                if (code >= 0 && (uint32_t)code < numNodes) { const float a = area(wmin, wmax, wz); if (a > bestA) { bestA = a; best = j; bestCode = code; } }
            }
            if (best < 0) break;
            own[best] = (uint32_t)bestCode; side[best] = 0;
            own[k] = (uint32_t)bestCode; side[k] = 1; ++k;
        }
        for (int j = 0; j < k; ++j) {
            uint32_t wmin, wmax, wz; int32_t code;
            words(own[j], side[j], wmin, wmax, wz, code);
            /* planes leave here as HALF FLOATS: the offset from the scene's wide centre (q - c), rounded outward to 11 significant
             * bits, so the kernel's slab test needs no conversion (one v_fma_mix_f32 per plane).  Exact within 2048 steps of the centre,
             * 2^-11 of the distance from it beyond: +0.7 % node visits, +6 % triangle tests on the bench frame (profiles/r02/wide_sim_f16.log)
             * for 12 % fewer vector instructions per visit */
            const int32_t xmin = (int32_t)(wmin & 0xffffu) - cx, ymin = (int32_t)(wmin >> 16) - cy, zmin = (int32_t)(wz & 0xffffu) - cz;
            const int32_t xmax = (int32_t)(wmax & 0xffffu) - cx, ymax = (int32_t)(wmax >> 16) - cy, zmax = (int32_t)(wz >> 16) - cz;
            o[j * 3] = rtr_f16_floor_bits(xmin) | (rtr_f16_floor_bits(ymin) << 16);
            o[j * 3 + 1] = rtr_f16_ceil_bits(xmax) | (rtr_f16_ceil_bits(ymax) << 16);
            o[j * 3 + 2] = rtr_f16_floor_bits(zmin) | (rtr_f16_ceil_bits(zmax) << 16);
            o[12 + j] = (uint32_t)code;
        }
    }
    for (int q = 0; q < 4; ++q) wide[(size_t)i * 4 + q] = make_uint4(o[q * 4], o[q * 4 + 1], o[q * 4 + 2], o[q * 4 + 3]);
}

/* Moves the 4-wide entries into the resident order (breadth-first from the root — rtr_api.cpp make_wide_nodes or k_wide_order — with
 * the best-first top of bvh_hot_top in front), so entries 0..K-1 are the part k_shadow_trace4 keeps in LDS.  Inner child codes are renumbered with it. */
__global__ __launch_bounds__(kB) void k_permute_wide(uint32_t numNodes, const uint4* __restrict__ in, const uint32_t* __restrict__ remap,
                                                     uint4* __restrict__ out, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= numNodes) return;
    const size_t dst = (size_t)remap[i] * 4;
    for (int q = 0; q < 3; ++q) out[dst + q] = in[(size_t)i * 4 + q];
    uint4 c = in[(size_t)i * 4 + 3];
    if ((int32_t)c.x >= 0) c.x = remap[c.x];
    if ((int32_t)c.y >= 0) c.y = remap[c.y];
    if ((int32_t)c.z >= 0) c.z = remap[c.z];
    if ((int32_t)c.w >= 0) c.w = remap[c.w];
    out[dst + 3] = c;
}

/* ---- vertex updates (rtr_scene_update_vertices) ---------------------------------------------------------------------
 * Lane i of the launch is vertex i of the concatenation of the ranges.  Its range is the last r with prefix[r] <= i (empty ranges
 * repeat a count and are skipped by that rule), found by bisection over the prefix counts, which every block first copies to LDS.
 * The source is read as strided dwords — whatever the caller's layout is: packed float3, a float4 column, RtrVertex records — and the
 * destination written as dword stores into the 48-B vertex, so uv and the pad words keep their bytes. */
static_assert(sizeof(RtrVertex) == 48 && sizeof(VertexRange) == 24, "layout");

__device__ __forceinline__ uint32_t vertex_range_of(const uint32_t* sPrefix, uint32_t numRanges, uint32_t i) {
    uint32_t lo = 0, hi = numRanges;                     /* sPrefix[lo] <= i < sPrefix[hi] */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sPrefix[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kB) void k_check_vertices(const VertexRange* __restrict__ ranges, const uint32_t* __restrict__ prefix, uint32_t numRanges,
                                                       uint32_t strideWords, uint32_t concatBase, uint32_t* __restrict__ firstBad) {
    __shared__ uint32_t sPrefix[kVertexRangesPerLaunch + 1];
    for (uint32_t j = threadIdx.x; j <= numRanges; j += kB) sPrefix[j] = prefix[j];
    __syncthreads();
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= sPrefix[numRanges]) return;
    const uint32_t r = vertex_range_of(sPrefix, numRanges, i);
    const uint32_t* src = ranges[r].positions + (size_t)(i - sPrefix[r]) * strideWords;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = __uint_as_float(src[k]);
        ok = ok && (x > -3.0e38f && x < 3.0e38f);        /* the rule of the scene builders: NaN fails both comparisons */
    }
    if (!ok) atomicMin(firstBad, concatBase + i);        /* rare: no wave reduction in front of it */
}

__global__ __launch_bounds__(kB) void k_write_vertices(const VertexRange* __restrict__ ranges, const uint32_t* __restrict__ prefix, uint32_t numRanges,
                                                       uint32_t positionStrideWords, uint32_t normalStrideWords, RtrVertex* __restrict__ vertices) {
    __shared__ uint32_t sPrefix[kVertexRangesPerLaunch + 1];
    for (uint32_t j = threadIdx.x; j <= numRanges; j += kB) sPrefix[j] = prefix[j];
    __syncthreads();
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= sPrefix[numRanges]) return;
    const uint32_t r = vertex_range_of(sPrefix, numRanges, i);
    const uint32_t v = i - sPrefix[r];
    const VertexRange vr = ranges[r];
    uint32_t* dst = reinterpret_cast<uint32_t*>(vertices + ((size_t)vr.firstVertex + v));
    const uint32_t* p = vr.positions + (size_t)v * positionStrideWords;
    const uint32_t p0 = p[0], p1 = p[1], p2 = p[2];
    dst[0] = p0; dst[1] = p1; dst[2] = p2;
    if (vr.normals) {
        const uint32_t* q = vr.normals + (size_t)v * normalStrideWords;
        const uint32_t n0 = q[0], n1 = q[1], n2 = q[2];
        dst[4] = n0; dst[5] = n1; dst[6] = n2;
    }
}

/* ---- the enqueued vertex update (rtr_scene_update_vertices_async) ----------------------------------------------------
 * The same two kernels with nothing between them and the host: the table of ranges and its prefix counts travel as KERNEL ARGUMENTS
 * (a launch copies them when it is enqueued, so no host buffer has to outlive the call), the check reduces the smallest offending
 * SCENE vertex index into *firstBad, and the write is predicated on that word: set, no lane writes anything — all ranges of the update
 * land or none does.  Ranges do not overlap (checked on the host), so the smallest scene index is one fixed vertex. */
__device__ __forceinline__ uint32_t arg_range_of(const VertexRangeArgs& t, uint32_t i) {
    uint32_t lo = 0, hi = t.numRanges;                   /* t.prefix[lo] <= i < t.prefix[hi] */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (t.prefix[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kB) void k_check_vertices_args(VertexRangeArgs t, uint32_t strideWords, uint32_t* __restrict__ firstBad) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= t.prefix[t.numRanges]) return;
    const uint32_t r = arg_range_of(t, i);
    const uint32_t v = i - t.prefix[r];
    const uint32_t* src = t.ranges[r].positions + (size_t)v * strideWords;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = __uint_as_float(src[k]);
        ok = ok && (x > -3.0e38f && x < 3.0e38f);
    }
    if (!ok) atomicMin(firstBad, t.ranges[r].firstVertex + v);
}

__global__ __launch_bounds__(kB) void k_write_vertices_args(VertexRangeArgs t, uint32_t positionStrideWords, uint32_t normalStrideWords,
                                                            RtrVertex* __restrict__ vertices, const uint32_t* __restrict__ firstBad) {
    if (*firstBad != 0xffffffffu) return;                /* a refused update: the vertex array keeps its bytes */
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= t.prefix[t.numRanges]) return;
    const uint32_t r = arg_range_of(t, i);
    const uint32_t v = i - t.prefix[r];
    const VertexRange vr = t.ranges[r];
    uint32_t* dst = reinterpret_cast<uint32_t*>(vertices + ((size_t)vr.firstVertex + v));
    const uint32_t* p = vr.positions + (size_t)v * positionStrideWords;
    const uint32_t p0 = p[0], p1 = p[1], p2 = p[2];
    dst[0] = p0; dst[1] = p1; dst[2] = p2;
    if (vr.normals) {
        const uint32_t* q = vr.normals + (size_t)v * normalStrideWords;
        const uint32_t n0 = q[0], n1 = q[1], n2 = q[2];
        dst[4] = n0; dst[5] = n1; dst[6] = n2;
    }
}

/* folds the update's word into the scene's sticky status: st[0] refused updates so far, st[1] the serial of the first refused update
 * since the host last looked (0xffffffff: none), st[2] its first bad scene vertex */
__global__ void k_fold_update_status(const uint32_t* __restrict__ firstBad, uint32_t* __restrict__ st, uint32_t serial) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t bad = *firstBad;
    if (bad == 0xffffffffu) return;
    st[0] += 1u;
    if (st[1] == 0xffffffffu) { st[1] = serial; st[2] = bad; }
}

/* ---- the enqueued instance update (rtr_scene_update_instances_async) -------------------------------------------------
 * The instance and light tables of a refit made ON THE DEVICE from the caller's device arrays.  One lane per ELEMENT of the update:
 * lanes 0 .. numInstances-1 are the records (instance firstInstance + lane, in instance order), the numLights lanes after them the
 * light infos.  The check reduces the smallest offending element index — instance index, or sceneInstances + light — into *firstBad;
 * the write is predicated on that word, as the vertex update's: set, no lane writes anything. */
struct InstanceUpdateArgs {
    const uint32_t* transforms;          /* numInstances records of 12 words, strideWords apart; null with numInstances == 0 */
    const uint32_t* lights;              /* numLights x 24 words (RtrAreaLightInfo), or null: no light lanes */
    uint32_t strideWords, firstInstance, numInstances, numLights, sceneInstances;
};

__global__ __launch_bounds__(kB) void k_check_instances(InstanceUpdateArgs a, const RtrAreaLightInfo* __restrict__ sceneLights, uint32_t* __restrict__ firstBad) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i < a.numInstances) {
        const uint32_t* src = a.transforms + (size_t)i * a.strideWords;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const float x = __uint_as_float(src[k]);
            ok = ok && (x > -3.0e38f && x < 3.0e38f);        /* the rule of rtr_scene_update_instances: NaN fails both comparisons */
        }
        if (!ok) atomicMin(firstBad, a.firstInstance + i);
    } else if (i - a.numInstances < a.numLights) {
        const uint32_t l = i - a.numInstances;
        const uint32_t* mine = a.lights + (size_t)l * 24u;
        const RtrAreaLightInfo& cur = sceneLights[l];
        if (mine[4] != cur.vertexOffset || mine[5] != cur.indexOffset || mine[6] != cur.numTriangles) atomicMin(firstBad, a.sceneInstances + l);
    }
}

__global__ __launch_bounds__(kB) void k_write_instances(InstanceUpdateArgs a, const uint32_t* __restrict__ customOf, uint32_t mirroredWord,
                                                        uint32_t* __restrict__ xforms, uint32_t* __restrict__ nmats, InstanceRef* __restrict__ refs,
                                                        uint32_t* __restrict__ sceneLights, const uint32_t* __restrict__ firstBad) {
    if (*firstBad != 0xffffffffu) return;                /* a refused update: every table keeps its bytes */
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i < a.numInstances) {
        const uint32_t* src = a.transforms + (size_t)i * a.strideWords;
        const uint32_t ci = customOf[a.firstInstance + i];
        float m[12], nm[9];
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = __uint_as_float(src[k]);
        rtr_normal_matrix(m, nm);
        const uint32_t bit = rtr_mirrored_bit(m);
        uint32_t* xf = xforms + 12u * (size_t)ci;
        uint32_t* nd = nmats + 12u * (size_t)ci;
        uint32_t* rf = reinterpret_cast<uint32_t*>(refs[ci].transform);
#pragma unroll
        for (int k = 0; k < 12; ++k) { const uint32_t w = __float_as_uint(m[k]); xf[k] = w; rf[k] = w; }
#pragma unroll
        for (int k = 0; k < 9; ++k) nd[k] = __float_as_uint(nm[k]);
        nd[mirroredWord] = bit;                          /* the other words of the slot keep their bytes */
    } else if (i - a.numInstances < a.numLights) {
        const uint32_t l = i - a.numInstances;
        const uint32_t* mine = a.lights + (size_t)l * 24u;
        uint32_t* dst = sceneLights + (size_t)l * 24u;
#pragma unroll
        for (int k = 0; k < 24; ++k) dst[k] = mine[k];
    }
}

/* the reduction words of a refit as bvh_refit's host array sets them, without a host array */
__global__ void k_refit_init(uint32_t* __restrict__ red) {
    const uint32_t i = threadIdx.x;
    if (blockIdx.x == 0 && i < 8u) red[i] = i < 3u ? 0xffffffffu : 0u;
}

/* ---- the breadth-first order of the 4-wide view, on the device (rtr_api.cpp, make_wide_nodes' host loop restated) ----------------
 * remap[] of k_permute_wide and the number of entries the tree reaches, bit for bit what the host loop gives: entry 0 gets id 0; the
 * entries are numbered in queue order — level by level, inside a level by their parent's new id, then by child slot; a code counts when
 * it is in 0 .. numNodes-1; an entry is numbered ONCE, where it first appears in that order; what the tree does not reach takes the ids
 * after them in ascending index order.
 * ONE workgroup of 1024 lanes walks the levels.  Why one: a level depends on the scan of the one before it, so a grid would need a
 * device-wide join per level — either a launch per level and phase (the refit keeps the topology, so stats.maxDepth bounds them: some
 * sixty launches of mostly idle grids, each as long as this kernel's whole step) or a grid sync, which the project does not use.  One
 * workgroup joins with s_barrier, keeps the level bounds in registers and LDS, needs no bound on the depth, and nothing is read back.
 * Its price is one CU's memory rate: profiles/refit_async_rate.py measures it on the bench scene.
 * A step takes kOrderE x 1024 queue entries, lane-consecutive (entry j = base + e * 1024 + tid: four independent loads in flight per
 * lane):
 *   claim : every inner code c of entry j (whose new id IS j: order[j] is the entry with id j) does atomicMin(claim[c], 4 j + slot + 1).
 *           Keys grow in queue order, so the minimum over all time is the first appearance: the host loop's `remap[c] == none` guard.
 *           claim[0] = 0 keeps the root from ever being numbered again.
 *   scan  : after a barrier the (entry, slot) pairs that hold their child's claim are counted — ballot + mbcnt inside a wave, one LDS
 *           word per (e, wave), which wave 0 scans (64 words: one per lane) — and the children take ids `next + rank` in that order.
 * What a lane reads back of the words this kernel wrote — claim[] (written by atomics, which work in L2), order[] and remap[] (stores of
 * other waves, one barrier earlier) — it reads with agent-scope loads, from L2: a line of order[] is read while its tail is still being
 * written, and nothing here depends on what the CU's L1 does with such a line. */
constexpr uint32_t kOrderB = 1024, kOrderE = 4, kOrderWaves = kOrderB / 64;
static_assert(kOrderE * kOrderWaves == 64, "wave 0 scans one (e, wave) total per lane");

__device__ __forceinline__ uint32_t lanes_before(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(kOrderB) void k_wide_order(const uint4* __restrict__ wide, uint32_t numNodes, uint32_t* __restrict__ remap,
                                                        uint32_t* __restrict__ claim, uint32_t* __restrict__ order, uint32_t* __restrict__ reachedOut, const uint32_t* __restrict__ go) {
    __shared__ uint32_t sTot[64];
    __shared__ uint32_t sAll;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (blockIdx.x != 0 || numNodes == 0) return;
    if (go && *go == 0u) return;                         /* the same word in every lane: the whole workgroup leaves before any barrier */
    for (uint32_t i = tid; i < numNodes; i += kOrderB) { remap[i] = i ? 0xffffffffu : 0u; claim[i] = i ? 0xffffffffu : 0u; }
    if (tid == 0) order[0] = 0;
    __syncthreads();
    uint32_t begin = 0, end = 1;                          /* the level in order[]: the same in every lane */
    while (begin < end) {
        uint32_t next = end;                              /* ids handed out so far */
        for (uint32_t base = begin; base < end; base += kOrderB * kOrderE) {
            /* every load below is unconditional (a lane past the level's end reads entry `begin` and drops it): the loads of a lane's
             * four entries, and later of its sixteen claim words, are in flight together instead of one after the other */
            uint32_t code[kOrderE][4];                    /* inner codes; 0xffffffff: not one */
            uint32_t node[kOrderE];
#pragma unroll
            for (uint32_t e = 0; e < kOrderE; ++e) {
                const uint32_t j = base + e * kOrderB + tid;
                node[e] = __hip_atomic_load(&order[j < end ? j : begin], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (uint32_t e = 0; e < kOrderE; ++e) {
                const uint32_t j = base + e * kOrderB + tid;
                const uint4 c = wide[(size_t)node[e] * 4 + 3];
                code[e][0] = j < end ? c.x : 0xffffffffu; code[e][1] = j < end ? c.y : 0xffffffffu;
                code[e][2] = j < end ? c.z : 0xffffffffu; code[e][3] = j < end ? c.w : 0xffffffffu;
            }
#pragma unroll
            for (uint32_t e = 0; e < kOrderE; ++e) {
                const uint32_t j = base + e * kOrderB + tid;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    if (code[e][k] < numNodes) atomicMin(&claim[code[e][k]], 4u * j + k + 1u);      /* (int32_t)code < 0 is >= numNodes as unsigned */
                    else code[e][k] = 0xffffffffu;
                }
            }
            __syncthreads();
            uint32_t won[kOrderE], before[kOrderE], seen[kOrderE][4];
#pragma unroll
            for (uint32_t e = 0; e < kOrderE; ++e)
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    seen[e][k] = __hip_atomic_load(&claim[code[e][k] != 0xffffffffu ? code[e][k] : 0u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (uint32_t e = 0; e < kOrderE; ++e) {
                const uint32_t j = base + e * kOrderB + tid;
                won[e] = 0; before[e] = 0;
                uint32_t total = 0;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const bool w = code[e][k] != 0xffffffffu && seen[e][k] == 4u * j + k + 1u;
                    const unsigned long long m = __ballot(w);
                    won[e] |= (w ? 1u : 0u) << k;
                    before[e] += lanes_before(m);
                    total += (uint32_t)__popcll(m);
                }
                if (lane == 0) sTot[e * kOrderWaves + wave] = total;
            }
            __syncthreads();
            if (wave == 0) {                              /* exclusive scan of the 64 totals, in (e, wave) order = queue order */
                const uint32_t v = sTot[lane];
                uint32_t incl = v;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const uint32_t up = __shfl_up(incl, o); if ((int)lane >= o) incl += up; }
                sTot[lane] = incl - v;
                if (lane == 63u) sAll = incl;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t e = 0; e < kOrderE; ++e) {
                uint32_t id = next + sTot[e * kOrderWaves + wave] + before[e];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (won[e] & (1u << k)) { remap[code[e][k]] = id; order[id] = code[e][k]; ++id; }
            }
            next += sAll;
            __syncthreads();                              /* sTot / sAll are free again; order[] of the next level is written */
        }
        begin = end; end = next;
    }
    const uint32_t reached = end;
    if (tid == 0) *reachedOut = reached;
    if (reached == numNodes) return;
    /* the rest, in ascending index order */
    uint32_t run = reached;
    for (uint32_t base = 0; base < numNodes; base += kOrderB) {
        const uint32_t i = base + tid;
        const bool un = i < numNodes && __hip_atomic_load(&remap[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0xffffffffu;
        const unsigned long long m = __ballot(un);
        if (lane == 0) sTot[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t pre = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kOrderWaves; ++w) { const uint32_t t = sTot[w]; if (w < wave) pre += t; all += t; }
        if (un) remap[i] = run + pre + lanes_before(m);
        run += all;
        __syncthreads();
    }
}

/* ---- the best-first top of the resident order (rtr_hot_top.h; bvh_build.cpp hot_top_positions restated) ---------------------------
 * k_hot_top_select: ONE wave grows the set from the root.  wide[] is still in BVH2-id order (child codes are BVH2 ids) and remap[]
 * holds every record's breadth-first id.  The candidates — the inner children of the records in the set — sit in LDS as (priority
 * bits, breadth-first id, BVH2 id); a step takes the one with the greatest key (priority << 32 | ~id: the highest priority, then the
 * lower breadth-first id; of equal keys the first in the list), moves the list's last entry into its place, and appends the taken
 * record's own inner children, whose priorities lanes 0..3 compute from the record's four child boxes.  A priority is >= 0, so its
 * bits order as it does.  The list holds at most 3 x set + 1 entries.  sel[0] = the size of the set, sel[1..] = its breadth-first ids
 * in the order they were taken.
 * k_hot_top_apply turns remap[] from breadth-first ids into resident positions: a member of the set goes to its rank, every other
 * record moves up by the number of members after it (breadth-first id b -> size + b - members below b). */
constexpr uint32_t kHotCand = 3u * RTR_HOT_TOP_MAX + 4u;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
        const unsigned long long u = ((unsigned long long)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}

__global__ __launch_bounds__(64) void k_hot_top_select(const uint4* __restrict__ wide, uint32_t numNodes, const uint32_t* __restrict__ remap,
                                                       const RtrBvhGrid* __restrict__ grid, const RtrAreaLightInfo* __restrict__ lights, uint32_t numLights,
                                                       uint32_t top, uint32_t* __restrict__ sel, const uint32_t* __restrict__ go) {
    __shared__ uint32_t cScore[kHotCand], cId[kHotCand], cNode[kHotCand], sSel[RTR_HOT_TOP_MAX];
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x != 0 || numNodes == 0) return;
    if (go && *go == 0u) return;                         /* the same word in every lane */
    if (top > RTR_HOT_TOP_MAX) top = RTR_HOT_TOP_MAX;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(wide);
    const float* centres = reinterpret_cast<const float*>(lights) + 20;      /* transform[12..14] */
    uint32_t nc = 0, ns = 1;                              /* the same in every lane */
    auto add_children = [&](uint32_t node) {              /* entered by all 64 lanes */
        const uint32_t* w = words + (size_t)node * 16;
        uint32_t code = 0xffffffffu, score = 0;
        if (lane < 4u) {
            code = w[12 + lane];
            if (code < numNodes) score = rtr_f2u(rtr_hot_score(w[3 * lane], w[3 * lane + 1], w[3 * lane + 2], grid, centres, numLights, 24u));
        }
        const bool inner = code < numNodes;               /* (int32_t)code < 0 is >= numNodes as unsigned */
        const unsigned long long m = __ballot(inner);
        const uint32_t at = nc + lanes_before(m);
        if (inner && at < kHotCand) { cScore[at] = score; cId[at] = remap[code]; cNode[at] = code; }
        nc += (uint32_t)__popcll(m);
        if (nc > kHotCand) nc = kHotCand;                 /* cannot happen: 3 x set + 1 entries at the most */
    };
    if (lane == 0) sSel[0] = 0u;
    add_children(0u);
    __syncthreads();
    while (ns < top && nc > 0u) {
        unsigned long long best = 0ull; uint32_t bi = 0xffffffffu;
        for (uint32_t i = lane; i < nc; i += 64u) {
            const unsigned long long key = ((unsigned long long)cScore[i] << 32) | (0xffffffffu - cId[i]);
            if (bi == 0xffffffffu || key > best) { best = key; bi = i; }
        }
        const unsigned long long all = wave_max_u64(bi == 0xffffffffu ? 0ull : best);
        const uint32_t win = wave_min_u32(bi != 0xffffffffu && best == all ? bi : 0xffffffffu);      /* < nc: some lane holds the maximum */
        const uint32_t id = cId[win], node = cNode[win];
        bool dup = false;
        for (uint32_t i = lane; i < ns; i += 64u) dup = dup || sSel[i] == id;
        const bool met = __ballot(dup) != 0ull;           /* a record met twice (never in a tree) is taken once */
        __syncthreads();
        --nc;
        if (lane == 0) { cScore[win] = cScore[nc]; cId[win] = cId[nc]; cNode[win] = cNode[nc]; if (!met) sSel[ns] = id; }
        __syncthreads();
        if (!met) { ++ns; add_children(node); __syncthreads(); }
    }
    if (lane == 0) sel[0] = ns;
    for (uint32_t i = lane; i < ns; i += 64u) sel[1 + i] = sSel[i];
}

__global__ __launch_bounds__(kB) void k_hot_top_apply(uint32_t numNodes, uint32_t* __restrict__ remap, const uint32_t* __restrict__ sel, const uint32_t* __restrict__ go) {
    __shared__ uint32_t sSel[RTR_HOT_TOP_MAX];
    if (go && *go == 0u) return;
    const uint32_t ns = sel[0] < RTR_HOT_TOP_MAX ? sel[0] : RTR_HOT_TOP_MAX;
    for (uint32_t i = threadIdx.x; i < ns; i += kB) sSel[i] = sel[1 + i];
    __syncthreads();
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= numNodes) return;
    const uint32_t b = remap[i];
    uint32_t below = 0, rank = 0xffffffffu;
    for (uint32_t r = 0; r < ns; ++r) { const uint32_t s = sSel[r]; below += s < b ? 1u : 0u; if (s == b) rank = r; }
    remap[i] = rank != 0xffffffffu ? rank : ns + b - below;
}

/* ---- the commit of an enqueued rebuild (rtr_scene_rebuild_async) ------------------------------------------------------------------
 * The device build wrote a STAGE, a second set of the tree's arrays nothing else reads; this kernel decides, on the device, whether the
 * staged tree replaces the live one.  The decision is one word every lane reads before anything else: the staged depth (red[7] of the
 * stage).  Above `limit` — the stack class the scene's render kernels are specialised for, which the host cannot raise without a join —
 * lane 0 writes the depth into *word (the update word the status fold reads) and NO lane copies anything; otherwise every array of the
 * table is copied over its live twin: all of it lands or none of it does.
 * One launch over all arrays: the table travels as a kernel argument; a lane moves 16 bytes per trip, the grid is capped
 * (kCommitMaxBlocks) and strides over an array's 16-byte chunks; the up to three words after an array's last whole chunk (4 (n - 1)-byte
 * arrays) are moved by the first lanes of the grid.  Every base is a hipMalloc'd one (256-B aligned), every size a multiple of 4.
 * The gated form (rtr_scene_rebuild_if_async): with *go == 0 nothing was staged, so nothing is copied and nothing is set.  committed, where
 * given, gets 1 when the arrays are copied and 0 when they are not (skipped or refused): the word the close of the policy is gated by. */
__global__ __launch_bounds__(kB) void k_commit_tree(CommitTable t, const uint32_t* __restrict__ stagedRed, uint32_t limit, uint32_t* __restrict__ word,
                                                    const uint32_t* __restrict__ go, uint32_t* __restrict__ committed) {
    const uint32_t g = blockIdx.x * kB + threadIdx.x;
    if (go && *go == 0u) {
        if (g == 0 && committed) *committed = 0u;
        return;
    }
    const uint32_t depth = stagedRed[7];
    if (g == 0 && committed) *committed = depth > limit ? 0u : 1u;
    if (depth > limit) {                                 /* the class would have to rise: refused, and the live tree keeps its bytes */
        if (g == 0) *word = depth;
        return;
    }
    const uint32_t stride = gridDim.x * kB;
    for (uint32_t k = 0; k < t.count; ++k) {
        const uint4* __restrict__ src = static_cast<const uint4*>(t.a[k].src);
        uint4* __restrict__ dst = static_cast<uint4*>(t.a[k].dst);
        const uint64_t chunks = t.a[k].bytes >> 4;
        for (uint64_t i = g; i < chunks; i += stride) dst[i] = src[i];
        const uint32_t tailWords = (uint32_t)(t.a[k].bytes & 15u) >> 2;
        if (g < tailWords) reinterpret_cast<uint32_t*>(dst + chunks)[g] = reinterpret_cast<const uint32_t*>(src + chunks)[g];
    }
}

/* ---- the rebuild policy on the device (rtr_scene_rebuild_if_async) -----------------------------------------------------------------
 * The record the policy keeps on the device: the fields of rtr_rebuild_if_status in its order, with the two words the chain is gated by
 * in the first two pad words.  go: this call builds (the gate of the build, the commit and the tail); committed: its commit copied the
 * stage (the gate of the close).  One lane each: the kernels between them are ordered by the stream. */
static_assert(sizeof(RebuildIfRecord) == 48, "layout");

/* decide: sah of the LIVE tree from the words k_tree_cost just summed and the live grid's scale, by the host's function; the comparison
 * is Scene.update_vertices_or_rebuild's, in double (rebuildAbove = +inf against a zero baseline is NaN, which compares false: never) */
__global__ void k_rebuild_if_decide(const unsigned long long* __restrict__ words, const RtrBvhGrid* __restrict__ grid, RebuildIfRecord* __restrict__ rec,
                                    double rebuildAbove) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "layout");
    uint64_t w[kTreeCostWords];
    for (uint32_t k = 0; k < kTreeCostWords; ++k) w[k] = words[k];
    const double sah = rtr_tree_sah(w, grid->scale[0], grid->scale[1], grid->scale[2]);
    const uint32_t go = sah > rebuildAbove * rec->builtSah ? 1u : 0u;
    rec->lastSah = sah;
    rec->evaluated += 1ull;
    rec->lastDecision = go;
    rec->go = go;
    rec->committed = 0u;
}

/* close: after a commit that copied, the words hold the sums of the NEW live tree (k_tree_cost gated by the same word): its sah is the
 * baseline from here on.  countRebuilt: 1 for rtr_scene_rebuild_if_async; 0 for rtr_scene_rebuild_async, which moves the baseline only. */
__global__ void k_rebuild_if_close(const unsigned long long* __restrict__ words, const RtrBvhGrid* __restrict__ grid, RebuildIfRecord* __restrict__ rec,
                                   uint32_t countRebuilt) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (rec->committed == 0u) return;
    uint64_t w[kTreeCostWords];
    for (uint32_t k = 0; k < kTreeCostWords; ++k) w[k] = words[k];
    rec->builtSah = rtr_tree_sah(w, grid->scale[0], grid->scale[1], grid->scale[2]);
    rec->rebuilt += countRebuilt;
}

/* a memset that a decision word can switch off (the leaf table's clearing: it must not run without the kernel that refills the table) */
__global__ __launch_bounds__(kB) void k_clear_words(uint32_t* __restrict__ p, uint64_t n, const uint32_t* __restrict__ go) {
    if (go && *go == 0u) return;
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < n; i += stride) p[i] = 0u;
}

/* ---- host-side drivers ------------------------------------------------------------------------------ */
#define BV_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)
static constexpr const uint32_t* kAlways = nullptr;      /* the gate of a launch that is not gated */

hipError_t launch_check_vertices(const VertexRange* ranges, const uint32_t* prefix, uint32_t numRanges, uint32_t total, uint32_t positionStrideWords,
                                 uint32_t concatBase, uint32_t* firstBad, hipStream_t s) {
    if (total == 0 || numRanges == 0) return hipSuccess;
    if (numRanges > kVertexRangesPerLaunch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_check_vertices, dim3((uint32_t)(((uint64_t)total + kB - 1) / kB)), dim3(kB), 0, s, ranges, prefix, numRanges, positionStrideWords, concatBase, firstBad);
    return hipGetLastError();
}

hipError_t launch_write_vertices(const VertexRange* ranges, const uint32_t* prefix, uint32_t numRanges, uint32_t total, uint32_t positionStrideWords,
                                 uint32_t normalStrideWords, RtrVertex* vertices, hipStream_t s) {
    if (total == 0 || numRanges == 0) return hipSuccess;
    if (numRanges > kVertexRangesPerLaunch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_write_vertices, dim3((uint32_t)(((uint64_t)total + kB - 1) / kB)), dim3(kB), 0, s, ranges, prefix, numRanges, positionStrideWords, normalStrideWords, vertices);
    return hipGetLastError();
}

hipError_t bvh_refit(const BvhInputs& in, uint32_t numPrims, uint32_t numNodes, const BvhDeviceArrays& a, hipStream_t s) {
    BV_TRY(hipMemsetAsync(a.counters, 0, (size_t)numNodes * sizeof(uint32_t), s));
    BV_TRY(hipMemsetAsync(a.depth, 0, (size_t)numNodes * sizeof(uint32_t), s));
    uint32_t init[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    BV_TRY(hipMemcpyAsync(a.red, init, sizeof init, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_world_prims, dim3((numPrims + kB - 1) / kB), dim3(kB), 0, s, in, numPrims, a.slotOfPrim, a.tris, a.boxMin, a.boxMax, a.red, kAlways);
    hipLaunchKernelGGL(k_fit, dim3((numNodes + kB - 1) / kB), dim3(kB), 0, s, numNodes, a.nodesF, a.boxMin, a.boxMax, a.parent, a.counters, a.depth, a.red, a.red + 7, kAlways);
    hipLaunchKernelGGL(k_grid, dim3(1), dim3(64), 0, s, a.nodesF, a.grid, kAlways);
    hipLaunchKernelGGL(k_quantize, dim3((numNodes + kB - 1) / kB), dim3(kB), 0, s, numNodes, a.nodesF, a.parent, a.grid, a.nodes, kAlways);
    return hipGetLastError();
}

/* the enqueued forms: nothing here waits, allocates or copies from host memory */
hipError_t launch_check_vertices_args(const VertexRangeArgs& t, uint32_t positionStrideWords, uint32_t* firstBad, hipStream_t s) {
    const uint32_t total = t.prefix[t.numRanges];
    if (total == 0 || t.numRanges == 0) return hipSuccess;
    if (t.numRanges > kVertexRangesPerArgs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_check_vertices_args, dim3((uint32_t)(((uint64_t)total + kB - 1) / kB)), dim3(kB), 0, s, t, positionStrideWords, firstBad);
    return hipGetLastError();
}

hipError_t launch_write_vertices_args(const VertexRangeArgs& t, uint32_t positionStrideWords, uint32_t normalStrideWords, RtrVertex* vertices,
                                      const uint32_t* firstBad, hipStream_t s) {
    const uint32_t total = t.prefix[t.numRanges];
    if (total == 0 || t.numRanges == 0) return hipSuccess;
    if (t.numRanges > kVertexRangesPerArgs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_write_vertices_args, dim3((uint32_t)(((uint64_t)total + kB - 1) / kB)), dim3(kB), 0, s, t, positionStrideWords, normalStrideWords, vertices, firstBad);
    return hipGetLastError();
}

hipError_t launch_fold_update_status(const uint32_t* firstBad, uint32_t* status, uint32_t serial, hipStream_t s) {
    hipLaunchKernelGGL(k_fold_update_status, dim3(1), dim3(64), 0, s, firstBad, status, serial);
    return hipGetLastError();
}

hipError_t launch_check_instances(const void* transforms, uint32_t strideWords, uint32_t firstInstance, uint32_t numInstances, const void* lights,
                                  uint32_t numLights, uint32_t sceneInstances, const RtrAreaLightInfo* sceneLights, uint32_t* firstBad, hipStream_t s) {
    const InstanceUpdateArgs a{static_cast<const uint32_t*>(transforms), static_cast<const uint32_t*>(lights), strideWords, firstInstance, numInstances,
                               lights ? numLights : 0u, sceneInstances};
    const uint64_t total = (uint64_t)a.numInstances + a.numLights;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_check_instances, dim3((uint32_t)((total + kB - 1) / kB)), dim3(kB), 0, s, a, sceneLights, firstBad);
    return hipGetLastError();
}

hipError_t launch_write_instances(const void* transforms, uint32_t strideWords, uint32_t firstInstance, uint32_t numInstances, const void* lights,
                                  uint32_t numLights, const uint32_t* customOf, uint32_t mirroredWord, float* xforms, float* nmats, InstanceRef* refs,
                                  RtrAreaLightInfo* sceneLights, const uint32_t* firstBad, hipStream_t s) {
    const InstanceUpdateArgs a{static_cast<const uint32_t*>(transforms), static_cast<const uint32_t*>(lights), strideWords, firstInstance, numInstances,
                               lights ? numLights : 0u, 0u};
    const uint64_t total = (uint64_t)a.numInstances + a.numLights;
    if (total == 0) return hipSuccess;
    if (mirroredWord < 9u || mirroredWord > 11u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_write_instances, dim3((uint32_t)((total + kB - 1) / kB)), dim3(kB), 0, s, a, customOf, mirroredWord, reinterpret_cast<uint32_t*>(xforms),
                       reinterpret_cast<uint32_t*>(nmats), refs, reinterpret_cast<uint32_t*>(sceneLights), firstBad);
    return hipGetLastError();
}

hipError_t bvh_refit_enqueued(const BvhInputs& in, uint32_t numPrims, uint32_t numNodes, const BvhDeviceArrays& a, hipStream_t s) {
    BV_TRY(hipMemsetAsync(a.counters, 0, (size_t)numNodes * sizeof(uint32_t), s));
    BV_TRY(hipMemsetAsync(a.depth, 0, (size_t)numNodes * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_refit_init, dim3(1), dim3(64), 0, s, a.red);
    hipLaunchKernelGGL(k_world_prims, dim3((numPrims + kB - 1) / kB), dim3(kB), 0, s, in, numPrims, a.slotOfPrim, a.tris, a.boxMin, a.boxMax, a.red, kAlways);
    hipLaunchKernelGGL(k_fit, dim3((numNodes + kB - 1) / kB), dim3(kB), 0, s, numNodes, a.nodesF, a.boxMin, a.boxMax, a.parent, a.counters, a.depth, a.red, a.red + 7, kAlways);
    hipLaunchKernelGGL(k_grid, dim3(1), dim3(64), 0, s, a.nodesF, a.grid, kAlways);
    hipLaunchKernelGGL(k_quantize, dim3((numNodes + kB - 1) / kB), dim3(kB), 0, s, numNodes, a.nodesF, a.parent, a.grid, a.nodes, kAlways);
    return hipGetLastError();
}

/* bvh_build_lbvh without its host array and with the nodesF memset inside: the same kernels in the same order.  go: every kernel of its
 * own returns at once when the word is 0, and the three clearings (stage and fit scratch) are gated kernels instead of memsets; the sort
 * (a library's twenty launches over the build scratch, which a device word cannot switch off) runs regardless: nothing else reads what
 * it writes */
hipError_t bvh_build_lbvh_enqueued(const BvhInputs& in, uint32_t numPrims, const BvhDeviceArrays& a, const BvhScratch& t, hipStream_t s, const uint32_t* go) {
    const uint32_t n = numPrims, numNodes = n - 1;
    if (go) {      /* gated, the three clearings are kernels too: 18 MB of memsets were a tenth of a skipped chain on the bench scene */
        BV_TRY(bvh_clear_words(reinterpret_cast<uint32_t*>(a.nodesF), (uint64_t)numNodes * 16, s, go));
        hipLaunchKernelGGL(k_refit_init, dim3(1), dim3(64), 0, s, a.red);
        BV_TRY(bvh_clear_words(a.counters, numNodes, s, go));
        BV_TRY(bvh_clear_words(a.depth, numNodes, s, go));
    } else {
        BV_TRY(hipMemsetAsync(a.nodesF, 0, (size_t)numNodes * 64, s));
        hipLaunchKernelGGL(k_refit_init, dim3(1), dim3(64), 0, s, a.red);
        BV_TRY(hipMemsetAsync(a.counters, 0, (size_t)numNodes * sizeof(uint32_t), s));
        BV_TRY(hipMemsetAsync(a.depth, 0, (size_t)numNodes * sizeof(uint32_t), s));
    }
    const dim3 gp((n + kB - 1) / kB), gn((numNodes + kB - 1) / kB);
    hipLaunchKernelGGL(k_world_prims, gp, dim3(kB), 0, s, in, n, (const uint32_t*)nullptr, t.trisCanon, t.minCanon, t.maxCanon, a.red, go);
    hipLaunchKernelGGL(k_morton, gp, dim3(kB), 0, s, n, t.minCanon, t.maxCanon, a.red, t.keysIn, go);
    size_t tempBytes = t.sortTempBytes;
    BV_TRY(hipcub::DeviceRadixSort::SortKeys(t.sortTemp, tempBytes, t.keysIn, t.keysOut, (int)n, 0, 64, s));
    hipLaunchKernelGGL(k_gather, gp, dim3(kB), 0, s, n, t.keysOut, t.trisCanon, t.minCanon, t.maxCanon, a.tris, a.boxMin, a.boxMax, a.slotOfPrim, go);
    hipLaunchKernelGGL(k_karras, gn, dim3(kB), 0, s, (int)n, t.keysOut, t.range, t.rawChild, go);
    hipLaunchKernelGGL(k_mark_unused, gn, dim3(kB), 0, s, numNodes, a.parent, go);
    hipLaunchKernelGGL(k_emit, gn, dim3(kB), 0, s, (int)n, t.range, t.rawChild, a.nodesF, a.parent, go);
    hipLaunchKernelGGL(k_fit, gn, dim3(kB), 0, s, numNodes, a.nodesF, a.boxMin, a.boxMax, a.parent, a.counters, a.depth, a.red, a.red + 7, go);
    hipLaunchKernelGGL(k_grid, dim3(1), dim3(64), 0, s, a.nodesF, a.grid, go);
    hipLaunchKernelGGL(k_quantize, gn, dim3(kB), 0, s, numNodes, a.nodesF, a.parent, a.grid, a.nodes, go);
    return hipGetLastError();
}

hipError_t bvh_commit_tree(const CommitTable& t, const uint32_t* stagedRed, uint32_t limit, uint32_t* word, hipStream_t s, const uint32_t* go, uint32_t* committed) {
    if (t.count > kCommitArrays) return hipErrorInvalidValue;
    uint64_t chunks = 1;
    for (uint32_t k = 0; k < t.count; ++k) {
        if ((t.a[k].bytes & 3u) || ((uintptr_t)t.a[k].src & 15u) || ((uintptr_t)t.a[k].dst & 15u)) return hipErrorInvalidValue;
        chunks = t.a[k].bytes >> 4 > chunks ? t.a[k].bytes >> 4 : chunks;
    }
    const uint64_t blocks = (chunks + kB - 1) / kB;
    hipLaunchKernelGGL(k_commit_tree, dim3((uint32_t)(blocks < kCommitMaxBlocks ? blocks : kCommitMaxBlocks)), dim3(kB), 0, s, t, stagedRed, limit, word, go, committed);
    return hipGetLastError();
}

hipError_t bvh_wide_order(const uint4* wide, uint32_t numNodes, uint32_t* remap, uint32_t* scratch, uint32_t* reached, hipStream_t s, const uint32_t* go) {
    if (numNodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_wide_order, dim3(1), dim3(kOrderB), 0, s, wide, numNodes, remap, scratch, scratch + numNodes, reached, go);
    return hipGetLastError();
}

size_t bvh_hot_top_words() { return RTR_HOT_TOP_MAX + 1u; }

hipError_t bvh_hot_top(const uint4* wide, uint32_t numNodes, uint32_t* remap, uint32_t* sel, const RtrBvhGrid* grid, const RtrAreaLightInfo* lights, uint32_t numLights,
                       uint32_t top, hipStream_t s, const uint32_t* go) {
    if (numNodes == 0 || numLights == 0 || !lights || top <= 1u) return hipSuccess;
    hipLaunchKernelGGL(k_hot_top_select, dim3(1), dim3(64), 0, s, wide, numNodes, remap, grid, lights, numLights, top, sel, go);
    hipLaunchKernelGGL(k_hot_top_apply, dim3((numNodes + kB - 1) / kB), dim3(kB), 0, s, numNodes, remap, sel, go);
    return hipGetLastError();
}

hipError_t bvh_build_lbvh(const BvhInputs& in, uint32_t numPrims, const BvhDeviceArrays& a, const BvhScratch& t, hipStream_t s) {
    const uint32_t* const go = kAlways;
    const uint32_t n = numPrims, numNodes = n - 1;
    uint32_t init[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    BV_TRY(hipMemcpyAsync(a.red, init, sizeof init, hipMemcpyHostToDevice, s));
    BV_TRY(hipMemsetAsync(a.counters, 0, (size_t)numNodes * sizeof(uint32_t), s));
    BV_TRY(hipMemsetAsync(a.depth, 0, (size_t)numNodes * sizeof(uint32_t), s));
    const dim3 gp((n + kB - 1) / kB), gn((numNodes + kB - 1) / kB);
    hipLaunchKernelGGL(k_world_prims, gp, dim3(kB), 0, s, in, n, (const uint32_t*)nullptr, t.trisCanon, t.minCanon, t.maxCanon, a.red, go);
    hipLaunchKernelGGL(k_morton, gp, dim3(kB), 0, s, n, t.minCanon, t.maxCanon, a.red, t.keysIn, go);
    size_t tempBytes = t.sortTempBytes;
    BV_TRY(hipcub::DeviceRadixSort::SortKeys(t.sortTemp, tempBytes, t.keysIn, t.keysOut, (int)n, 0, 64, s));
    hipLaunchKernelGGL(k_gather, gp, dim3(kB), 0, s, n, t.keysOut, t.trisCanon, t.minCanon, t.maxCanon, a.tris, a.boxMin, a.boxMax, a.slotOfPrim, go);
    hipLaunchKernelGGL(k_karras, gn, dim3(kB), 0, s, (int)n, t.keysOut, t.range, t.rawChild, go);
    hipLaunchKernelGGL(k_mark_unused, gn, dim3(kB), 0, s, numNodes, a.parent, go);
    hipLaunchKernelGGL(k_emit, gn, dim3(kB), 0, s, (int)n, t.range, t.rawChild, a.nodesF, a.parent, go);
    hipLaunchKernelGGL(k_fit, gn, dim3(kB), 0, s, numNodes, a.nodesF, a.boxMin, a.boxMax, a.parent, a.counters, a.depth, a.red, a.red + 7, go);
    hipLaunchKernelGGL(k_grid, dim3(1), dim3(64), 0, s, a.nodesF, a.grid, go);
    hipLaunchKernelGGL(k_quantize, gn, dim3(kB), 0, s, numNodes, a.nodesF, a.parent, a.grid, a.nodes, go);
    return hipGetLastError();
}

hipError_t bvh_make_wide(const uint4* nodes, uint32_t numNodes, const int32_t* parentOrNull, RtrBvhGrid* grid, const uint8_t* shapeOrNull, uint4* wide, unsigned long long* sums4, hipStream_t s, const uint32_t* go) {
    BV_TRY(hipMemsetAsync(sums4, 0, kCentreWords * sizeof(unsigned long long), s));
    const dim3 gn((numNodes + kB - 1) / kB);
    hipLaunchKernelGGL(k_wide_centre_sum, gn, dim3(kB), 0, s, numNodes, nodes, parentOrNull, sums4, go);
    hipLaunchKernelGGL(k_wide_centre_candidates, dim3(1), dim3(1), 0, s, sums4, go);
    hipLaunchKernelGGL(k_wide_centre_cost, gn, dim3(kB), 0, s, numNodes, nodes, parentOrNull, sums4, go);
    hipLaunchKernelGGL(k_wide_centre_set, dim3(1), dim3(1), 0, s, sums4, grid, go);
    hipLaunchKernelGGL(k_wide_nodes, dim3((numNodes + kB - 1) / kB), dim3(kB), 0, s, numNodes, nodes, parentOrNull, grid, shapeOrNull, wide, go);
    return hipGetLastError();
}

hipError_t bvh_permute_wide(const uint4* in, uint32_t numNodes, const uint32_t* remap, uint4* out, hipStream_t s, const uint32_t* go) {
    hipLaunchKernelGGL(k_permute_wide, dim3((numNodes + kB - 1) / kB), dim3(kB), 0, s, numNodes, in, remap, out, go);
    return hipGetLastError();
}

size_t bvh_wide_scratch_words() { return kCentreWords; }

size_t bvh_tree_cost_words() { return kTreeCostWords; }

hipError_t bvh_tree_cost(const uint4* nodes, uint32_t numNodes, const int32_t* parentOrNull, unsigned long long* words, hipStream_t s, const uint32_t* go) {
    BV_TRY(hipMemsetAsync(words, 0, kTreeCostWords * sizeof(unsigned long long), s));
    if (numNodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tree_cost, dim3((numNodes + kB - 1) / kB), dim3(kB), 0, s, numNodes, nodes, parentOrNull, words, go);
    return hipGetLastError();
}

hipError_t bvh_rebuild_if_decide(const unsigned long long* words, const RtrBvhGrid* grid, RebuildIfRecord* rec, double rebuildAbove, hipStream_t s) {
    hipLaunchKernelGGL(k_rebuild_if_decide, dim3(1), dim3(64), 0, s, words, grid, rec, rebuildAbove);
    return hipGetLastError();
}

hipError_t bvh_rebuild_if_close(const unsigned long long* words, const RtrBvhGrid* grid, RebuildIfRecord* rec, uint32_t countRebuilt, hipStream_t s) {
    hipLaunchKernelGGL(k_rebuild_if_close, dim3(1), dim3(64), 0, s, words, grid, rec, countRebuilt);
    return hipGetLastError();
}

hipError_t bvh_clear_words(uint32_t* p, uint64_t n, hipStream_t s, const uint32_t* go) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + kB - 1) / kB;
    hipLaunchKernelGGL(k_clear_words, dim3((uint32_t)(blocks < kCommitMaxBlocks ? blocks : kCommitMaxBlocks)), dim3(kB), 0, s, p, n, go);
    return hipGetLastError();
}

size_t bvh_sort_temp_bytes(uint32_t numPrims) {
    size_t bytes = 0;
    unsigned long long* nul = nullptr;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, nul, nul, (int)numPrims, 0, 64, (hipStream_t)0);
    return bytes;
}

}  // namespace rtrdev
