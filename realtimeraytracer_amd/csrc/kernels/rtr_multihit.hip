/* rtr_multihit.hip — multi-hit ray queries: the first K hits along a ray, in order, resumable (include/rtr.h: rtr_trace_rays_multi).
 *
 * What a Vulkan caller builds with an any-hit shader that records and ignores: every surface along the ray, not only the nearest.  The
 * accepted set of a ray is the closest-hit query's (rtr_trace_rays_masked: cull mask, opacity cull, rtr_mt_intersect with the ray's
 * tmin, t < tmax, facing cull, opacity-map test — in that order, counted the same way); the result is its min(K, |set|) smallest members
 * by the total order trace() of rtr_device.h already uses, (t, customIndex, primitiveId), ascending.
 *   k_multihit       one ray per lane, one-wave workgroups, 16-entry interleaved LDS stack: the closest-hit walk of trace() — near child
 *                    first, ties to child 0, far child pushed, a leaf's records in storage order — with ONE change: the far limit of the
 *                    slab test stays tmax until the lane's list holds K entries and is then the list's LAST t.  The slab test keeps a
 *                    box whose entry equals the limit (and widens: RTR_BOX_WIDEN), so candidates that tie the K-th t are still met and
 *                    can win on their ids.  With K = 1 this is the closest-hit walk visit for visit.  A ray that needs more stack is
 *                    abandoned and redone from scratch: sentinel in slot 0's customIndex, one atomic per wave onto the redo list;
 *   k_multihit_tail  walks those rays again with the full-depth stacks in global memory (the spill area k_query_tail uses, cut into
 *                    one-wave workgroups so that the list code is the same); if the redo list overflowed it finds them by the sentinel.
 * The per-lane list is sorted, holds (t, customIndex, primitiveId, u, v) and lives in LDS, interleaved per lane like the stack: word
 * (5 j + f) * 64 + lane, so every access of a wave is conflict-free and nothing is a dynamically indexed private array (scratch 0).  At
 * K = 8 a wave holds 4 KiB of stack and 10 KiB of list; the launch asks for the LDS its K needs.  Insertion: find the place from the
 * end (keys compared without short-circuit branches: the FLAT_TAKE note of rtr_device.h), shift, store.
 * Resume: only candidates whose key is strictly greater than after[k]'s enter the list (one comparison, ahead of the opacity-map test).
 * Compiled with the library's flags (-ffp-contract=off): the numerical contract of include/rtr_math.h.
 */
#include "rtr_query_device.h"
#include "../../../include/rtr.h"

namespace rtrdev {

constexpr int kMultiBlock = 64;                 /* one wave: the list's and the stack's interleave */
constexpr int kMultiStack = 16;                 /* LDS stack entries per lane, as k_query */
constexpr uint32_t kMultiFields = 5;            /* t, customIndex, primitiveId, u, v */
constexpr int kMultiTailBlocks = (int)(kSpillInts / 64 / kMultiBlock);      /* 256 one-wave workgroups share the spill area: 64 entries per lane */
static_assert((size_t)64 * kMultiTailBlocks * kMultiBlock == kSpillInts, "the tail kernel's stacks fill the spill area");
static_assert(RTR_MULTIHIT_MAX == 8u, "the LDS budget below is worked out for 8 entries");
static_assert((kCullAll & 1u) == 0u && kCullAll == (RTR_QUERY_CULL_BACK_FACING | RTR_QUERY_CULL_FRONT_FACING | RTR_QUERY_CULL_OPAQUE | RTR_QUERY_CULL_NO_OPAQUE),
              "the kernels' cull bits are the interface's");

typedef __attribute__((address_space(3))) uint32_t* lds_u32;      /* keeps the accesses ds_read / ds_write */
typedef __attribute__((address_space(3))) int32_t* lds_i32;

__host__ __device__ constexpr uint32_t multihit_lds_bytes(uint32_t maxHits) {
    return (uint32_t)kMultiBlock * ((uint32_t)kMultiStack + kMultiFields * maxHits) * 4u;
}

/* (t, customIndex, primitiveId) < (et, ec, ep), evaluated without short-circuit branches */
__device__ __forceinline__ bool key_less(float t, uint32_t c, uint32_t p, float et, uint32_t ec, uint32_t ep) {
    const bool idLess = (c < ec) | ((c == ec) & (p < ep));
    return (t < et) | ((t == et) & idLess);
}

/* the resume key of ray k: (-inf, 0, 0) without `after` — every candidate is greater.  false: the ray is exhausted (a miss record) */
__device__ __forceinline__ bool multi_after(const float4* __restrict__ after, uint32_t k, float& at, uint32_t& ac, uint32_t& ap) {
    at = -__builtin_inff(); ac = 0u; ap = 0u;
    if (!after) return true;
    const float4 a = after[2 * (size_t)k], b = after[2 * (size_t)k + 1];
    at = a.x; ac = __float_as_uint(a.w); ap = __float_as_uint(b.x);
    return ac != RTR_MISS;
}

/* The walk.  stack: this lane's slot 0, consecutive depths STRIDE ints apart (LDS, or the spill area: LIMIT = 0).  list: this lane's
 * word 0 of the wave's list.  cnt: entries the list holds (0 on entry).  Returns true iff the ray outgrew LIMIT stack entries. */
template <bool STATS, int STRIDE, int LIMIT, int OCT, bool ALPHA, class StackPtr>
__device__ __forceinline__ bool multihit_walk(const DeviceScene& sc, StackPtr stack, lds_u32 list, const uint32_t K, rtr_v3 o, rtr_v3 d, float tmin, float tmax,
                                              const float at, const uint32_t ac, const uint32_t ap, const uint32_t rayMask8, const uint32_t cull,
                                              uint32_t& cnt, LocalStats& st) {
    cnt = 0u;
    if (!(tmax > tmin)) return false;
    const rtr_v3 idir = rtr_mk(rtr_safe_rcp_dir(d.x), rtr_safe_rcp_dir(d.y), rtr_safe_rcp_dir(d.z));
    rtr_v3 ga, gb;                                        /* t(q) = q * ga + gb (rtr_math.h) */
    rtr_ray_grid(o, idir, sc.grid->origin, sc.grid->scale, &ga, &gb);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t nodeBuf = __builtin_amdgcn_make_buffer_rsrc((void*)sc.nodes, 0, 0xffffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t triBuf = __builtin_amdgcn_make_buffer_rsrc((void*)sc.tris, 0, 0xffffffff, 0x00020000);
    /* the list's last key while it is full; until then the far limit is the ray's */
    float limit = tmax;
    uint32_t lastC = RTR_MISS, lastP = RTR_MISS;
    int sp = 0;
    int32_t cur = 0;
    constexpr int32_t kWalkEnd = (int32_t)0x80000000;     /* not a leaf code */
    bool over = false;
    for (;;) {
        while (cur >= 0) {
            const int32_t nodeOff = cur << 5;
            const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(nodeBuf, nodeOff, 0, 0);
            const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(nodeBuf, nodeOff + 16, 0, 0);
            const int2 ch = make_int2((int)b.z, (int)b.w);
            if (STATS) st.nodes++;
            float tl, tr;
            const bool hl = slab_oct<OCT>(a.x, a.y, b.x, ga, gb, tmin, limit, tl);
            const bool hr = slab_oct<OCT>(a.z, a.w, b.y, ga, gb, tmin, limit, tr);
            if (hl && hr) {
                const bool swap = tr < tl;                /* the nearer child first (ties: child 0) */
                const int32_t nearC = swap ? ch.y : ch.x;
                const int32_t farC = swap ? ch.x : ch.y;
                if (LIMIT > 0 && sp >= LIMIT) { over = true; cur = kWalkEnd; }
                else { stack[sp * STRIDE] = farC; ++sp; cur = nearC; }
            } else if (hl) cur = ch.x;
            else if (hr) cur = ch.y;
            else if (sp == 0) cur = kWalkEnd;
            else { --sp; cur = stack[sp * STRIDE]; }
        }
        if (cur == kWalkEnd) break;
        {
            const uint32_t code = (uint32_t)~cur;
            const uint32_t first = code >> 3, count = (code & 7u) + 1u;
            for (uint32_t i = 0; i < count; ++i) {
                const int32_t triOff = (int32_t)((first + i) * 48u);
                const u32x4 r0 = __builtin_amdgcn_raw_buffer_load_b128(triBuf, triOff, 0, 0);
                const u32x4 r1 = __builtin_amdgcn_raw_buffer_load_b128(triBuf, triOff + 16, 0, 0);
                const u32x4 r2 = __builtin_amdgcn_raw_buffer_load_b128(triBuf, triOff + 32, 0, 0);
                const float4 q0 = make_float4(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w));
                const float4 q1 = make_float4(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z), __uint_as_float(r1.w));
                const float4 q2 = make_float4(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z), __uint_as_float(r2.w));
                if (STATS) st.tris++;
                if ((rayMask8 & ~r2.w) == 0u) continue;                               /* the instance does not exist for this ray */
                if (cull != 0u && cull_by_opacity(cull, r2.w, ALPHA)) continue;       /* culled before the any-hit test, as in Vulkan */
                float t, u, v;
                if (!rtr_mt_intersect(o, d, f4xyz(q0), f4xyz(q1), f4xyz(q2), tmin, &t, &u, &v)) continue;
                if (!(t < tmax)) continue;
                const uint32_t cu = __float_as_uint(q0.w), pr = __float_as_uint(q1.w);
                if (cull != 0u && cull_by_facing(sc, cull, d, f4xyz(q1), f4xyz(q2), cu)) continue;
                if (!key_less(at, ac, ap, t, cu, pr)) continue;                       /* resume: reported by an earlier call of the chain */
                if (ALPHA && (__float_as_uint(q2.w) & 1u) && !alpha_pass<STATS>(sc, cu, pr, u, v, st)) continue;
                const bool full = cnt == K;
                if (full & !key_less(t, cu, pr, limit, lastC, lastP)) continue;       /* not among the first K */
                /* its place, from the end; a record met twice (a one-leaf tree names its leaf in both children of the root) is dropped */
                uint32_t pos = cnt;
                bool dup = false;
                while (pos > 0u) {
                    const uint32_t e = (pos - 1u) * kMultiFields * kMultiBlock;
                    const float et = __uint_as_float(list[e]);
                    const uint32_t ec = list[e + kMultiBlock], ep = list[e + 2 * kMultiBlock];
                    if (!key_less(t, cu, pr, et, ec, ep)) { dup = (t == et) & (cu == ec) & (pr == ep); break; }
                    --pos;
                }
                if (dup) continue;
                const uint32_t end = full ? K - 1u : cnt;                             /* a full list drops its last entry */
                for (uint32_t j = end; j > pos; --j) {
                    const uint32_t to = j * kMultiFields * kMultiBlock, from = to - kMultiFields * kMultiBlock;
#pragma unroll
                    for (uint32_t f = 0; f < kMultiFields; ++f) list[to + f * kMultiBlock] = list[from + f * kMultiBlock];
                }
                const uint32_t e = pos * kMultiFields * kMultiBlock;
                list[e] = __float_as_uint(t); list[e + kMultiBlock] = cu; list[e + 2 * kMultiBlock] = pr;
                list[e + 3 * kMultiBlock] = __float_as_uint(u); list[e + 4 * kMultiBlock] = __float_as_uint(v);
                cnt = end + 1u;
                if (cnt == K) {
                    const uint32_t l = (K - 1u) * kMultiFields * kMultiBlock;
                    limit = __uint_as_float(list[l]); lastC = list[l + kMultiBlock]; lastP = list[l + 2 * kMultiBlock];
                }
            }
        }
        if (sp == 0) break;
        --sp; cur = stack[sp * STRIDE];
    }
    if (LIMIT > 0 && over) cnt = 0u;
    return LIMIT > 0 && over;
}

/* ray k's K records, ray-major: the list's cnt entries, then miss records (t = the ray's own tmax, ids 0xffffffff); RtrHit as two 16-B
 * stores.  sentinel: slot 0's customIndex becomes RTR_STACK_OVERFLOW (an abandoned ray: cnt is 0). */
__device__ __forceinline__ void multi_store(const MultiHitArgs& ma, lds_u32 list, uint32_t k, uint32_t cnt, float tmax, bool sentinel) {
    float4* __restrict__ out = ma.hits + 2 * (size_t)k * ma.maxHits;
    for (uint32_t j = 0; j < ma.maxHits; ++j) {
        float t = tmax, u = 0.0f, v = 0.0f;
        uint32_t cu = (sentinel && j == 0u) ? RTR_STACK_OVERFLOW : RTR_MISS, pr = RTR_MISS;
        if (j < cnt) {
            const uint32_t e = j * kMultiFields * kMultiBlock;
            t = __uint_as_float(list[e]); cu = list[e + kMultiBlock]; pr = list[e + 2 * kMultiBlock];
            u = __uint_as_float(list[e + 3 * kMultiBlock]); v = __uint_as_float(list[e + 4 * kMultiBlock]);
        }
        out[2 * j] = make_float4(t, u, v, __uint_as_float(cu));
        out[2 * j + 1] = make_float4(__uint_as_float(pr), 0.0f, 0.0f, 0.0f);
    }
    if (ma.counts) ma.counts[k] = cnt;
}

template <bool ALPHA, bool STATS>
__global__ __launch_bounds__(kMultiBlock) void k_multihit(DeviceScene sc, MultiHitArgs ma, Counters* stats, RayMaskArgs rm) {
    extern __shared__ uint32_t s_multi[];
    const lds_i32 stack = (lds_i32)s_multi + threadIdx.x;
    const lds_u32 list = (lds_u32)s_multi + kMultiStack * kMultiBlock + threadIdx.x;
    const uint32_t k = blockIdx.x * kMultiBlock + threadIdx.x;
    if (k >= ma.n) return;
    LocalStats st;
    rtr_v3 o, d;
    float tmin, tmax, at;
    uint32_t ac, ap;
    const uint32_t rm8 = query_ray_mask8(rm, k), cull = rm.masked & kCullAll;
    bool ok = query_ray(ma.rays, k, o, d, tmin, tmax) && rm8 != 0u;
    ok = multi_after(ma.after, k, at, ac, ap) && ok;
    const float tfar = ok ? tmax : tmin;                   /* a degenerate, masked-out or exhausted ray walks nothing but is counted like any other */
    if (STATS) { st.rays++; st.primary++; }
    uint32_t cnt = 0u;
    bool over;
    if (STATS) over = multihit_walk<true, kMultiBlock, kMultiStack, 8, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st);
    else {
        /* as in k_query: the traversal compiled for the wave's direction signs when all its rays share them */
        const uint32_t oct = ray_octant(sc, o, d);
        const uint32_t woct = (uint32_t)__builtin_amdgcn_readfirstlane((int)oct);
        switch (__ballot(oct != woct) != 0ull ? 8u : woct) {
            case 0: over = multihit_walk<false, kMultiBlock, kMultiStack, 0, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
            case 1: over = multihit_walk<false, kMultiBlock, kMultiStack, 1, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
            case 2: over = multihit_walk<false, kMultiBlock, kMultiStack, 2, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
            case 3: over = multihit_walk<false, kMultiBlock, kMultiStack, 3, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
            case 4: over = multihit_walk<false, kMultiBlock, kMultiStack, 4, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
            case 5: over = multihit_walk<false, kMultiBlock, kMultiStack, 5, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
            case 6: over = multihit_walk<false, kMultiBlock, kMultiStack, 6, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
            case 7: over = multihit_walk<false, kMultiBlock, kMultiStack, 7, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
            default: over = multihit_walk<false, kMultiBlock, kMultiStack, 8, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tfar, at, ac, ap, rm8, cull, cnt, st); break;
        }
    }
    multi_store(ma, list, k, cnt, tmax, over);            /* a miss reports the ray's own tmax */
    redo_append(ma.ctrl, ma.redoList, ma.redoCap, over, k);
    if (STATS) st.flush(stats);
}

/* The rays k_multihit abandoned, walked from the root with a full-depth stack in global memory and an empty list.  From the redo list,
 * or — when more rays were abandoned than it holds — from a scan of slot 0 of every ray for the sentinel.  STATS: the ray itself was
 * counted by k_multihit; this walk's visits and tests are added to it. */
template <bool ALPHA, bool STATS>
__global__ __launch_bounds__(kMultiBlock) void k_multihit_tail(DeviceScene sc, MultiHitArgs ma, Counters* stats, RayMaskArgs rm) {
    extern __shared__ uint32_t s_multi[];
    const uint32_t count = ma.ctrl[kQueryRedoWord];
    if (count == 0u) return;
    const lds_u32 list = (lds_u32)s_multi + threadIdx.x;
    const bool scan = count > ma.redoCap;
    const uint64_t m = scan ? ma.n : count;
    int32_t* stack = ma.spill + blockIdx.x * kMultiBlock + threadIdx.x;
    LocalStats st;
    for (uint64_t j = (uint64_t)blockIdx.x * kMultiBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kMultiBlock) {
        uint32_t k = (uint32_t)j;
        if (!scan) k = ma.redoList[j];
        else if (__float_as_uint(ma.hits[2 * (size_t)k * ma.maxHits].w) != RTR_STACK_OVERFLOW) continue;
        rtr_v3 o, d;
        float tmin, tmax, at;
        uint32_t ac, ap;
        query_ray(ma.rays, k, o, d, tmin, tmax);          /* an abandoned ray is never degenerate, masked out or exhausted: it walked past 16 stacked nodes */
        multi_after(ma.after, k, at, ac, ap);
        uint32_t cnt = 0u;
        multihit_walk<STATS, kMultiTailBlocks * kMultiBlock, 0, 8, ALPHA>(sc, stack, list, ma.maxHits, o, d, tmin, tmax, at, ac, ap, query_ray_mask8(rm, k),
                                                                           rm.masked & kCullAll, cnt, st);
        multi_store(ma, list, k, cnt, tmax, false);
    }
    if (STATS) st.flush(stats);
}

template <bool ALPHA, bool STATS>
static hipError_t multihit_t(const DeviceScene& sc, const MultiHitArgs& ma, Counters* stats, hipStream_t s, const RayMaskArgs& rm) {
    const uint32_t blocks = (uint32_t)(((uint64_t)ma.n + kMultiBlock - 1) / kMultiBlock);
    hipLaunchKernelGGL((k_multihit<ALPHA, STATS>), dim3(blocks), dim3(kMultiBlock), multihit_lds_bytes(ma.maxHits), s, sc, ma, stats, rm);
    hipLaunchKernelGGL((k_multihit_tail<ALPHA, STATS>), dim3(kMultiTailBlocks), dim3(kMultiBlock), (size_t)kMultiBlock * kMultiFields * ma.maxHits * 4u, s, sc, ma,
                       stats, rm);
    return hipGetLastError();
}

hipError_t launch_multihit(const DeviceScene& sc, const MultiHitArgs& ma, bool alpha, Counters* stats, hipStream_t s, const RayMaskArgs& rm) {
    if (ma.maxHits == 0u || ma.maxHits > RTR_MULTIHIT_MAX) return hipErrorInvalidValue;      /* the LDS the kernels index is sized by it */
    if (alpha) return stats ? multihit_t<true, true>(sc, ma, stats, s, rm) : multihit_t<true, false>(sc, ma, stats, s, rm);
    return stats ? multihit_t<false, true>(sc, ma, stats, s, rm) : multihit_t<false, false>(sc, ma, stats, s, rm);
}

}  // namespace rtrdev
