/* rtr_query.h — host-callable launchers of the ray-query kernels (kernels/rtr_query.hip; internal to librtr_hip.so). */
#pragma once
#include <hip/hip_runtime.h>
#include "rtr_kernels.h"

namespace rtrdev {

/* Entries of a context's redo list: the rays of one query that outgrew the 16-entry LDS stack.  Past it the tail kernel finds them by
 * their sentinel in the outputs instead, so the scratch does not grow with the number of rays. */
constexpr uint32_t kQueryRedoCap = 1u << 16;
constexpr uint32_t kQueryRedoWord = 0;       /* word of the control block: rays appended to the redo list (may exceed its capacity) */
constexpr uint32_t kQueryCtrlWords = 16;

struct QueryArgs {
    const float4* rays;          /* RtrRay as 2 x float4: {origin, tmin} {direction, tmax} */
    float4* hits;                /* RtrHit as 2 x float4 (closest hit), or null */
    uint8_t* occluded;           /* any hit: 1 = occluded, or null */
    uint32_t n;
    uint32_t redoCap;            /* entries of redoList the query may use */
    uint32_t* ctrl;              /* kQueryCtrlWords words, zeroed before the launch */
    uint32_t* redoList;
    int32_t* spill;              /* kSpillInts: the tail kernel's full-depth stacks */
};

/* Arguments of the hit-surface kernel (rtr_hit_surfaces).  The triangle counts live here, not in DeviceScene, which every other kernel
 * takes by value. */
struct SurfaceArgs {
    const float4* rays;          /* RtrRay as 2 x float4: {origin, tmin} {direction, tmax} */
    const float4* hits;          /* RtrHit as 2 x float4: {t, u, v, customIndex} {primitiveId, -, -, -} */
    float4* out;                 /* RtrSurface as 5 x float4 */
    const uint32_t* triCount;    /* per customIndex: the triangles of the light (customIndex < numLights) or of the instance's mesh */
    uint32_t numInstances;       /* entries of triCount */
    uint32_t n;
};

/* Arguments of the direct-lighting kernels (rtr_light_rays, rtr_shade_hits): rtr_light_params and the slots per hit the host derived
 * from the scene's light table (rtr_light_slots). */
struct LightArgs {
    const float4* rays;          /* RtrRay as 2 x float4 */
    const float4* hits;          /* RtrHit as 2 x float4 */
    const uint32_t* seeds;       /* per hit: the base of its sample seeds, or null (then the pixel's: px * 733 + py * 1933) */
    const uint32_t* triCount;    /* as SurfaceArgs */
    uint32_t numInstances;
    uint32_t n;
    uint32_t slots;              /* Q: numShadowRays x the triangles of the first numAreaLights lights, + 1 */
    uint32_t numAreaLights, numShadowRays, frame, width, spp;
    uint32_t outputs;            /* RTR_LIGHT_* mask (shade) */
    uint32_t direct;             /* light rays: 1 = the unstaged form of the kernel whatever the slot count (the test build's switch) */
    float4* outRays;             /* light rays: n * slots RtrRay */
    int32_t* outLeaves;          /* hinted light rays: n * slots start hints (LeafTable below), or null */
    const int32_t* leafTable;    /* hinted light rays: the scene's triangle -> leaf table and its per-customIndex bases */
    const uint32_t* leafBase;
    const uint8_t* occluded;     /* shade: n * slots visibility bytes */
    float4* out;                 /* shade: RtrRadiance as 3 x float4 */
};

/* Arguments of the picked direct-lighting kernels (rtr_light_rays_picked, rtr_shade_hits_picked): LightArgs as those of the full forms,
 * with la.slots = R = picks + 1 (the picks, then the directional light), and what include/rtr_pick.h needs. */
struct PickArgs {
    LightArgs la;
    uint32_t picks;              /* P: 1 ... RTR_PICK_MAX */
    uint32_t depth;              /* enters the picks' seeds */
    uint32_t areaSlots;          /* A: numShadowRays x the triangles of the first numAreaLights lights (la.numAreaLights > 0 whenever A > 0) */
    float defaultWeight;         /* shade: (float)triangles / (float)P */
    const uint32_t* slotsIn;     /* rays: n * P slots of the caller's choosing, or null (drawn by the rule); shade: the slots the rays were made for */
    uint32_t* outSlots;          /* rays: n * P slots used */
    const float* weights;        /* shade: n * P weights, or null (defaultWeight) */
};

/* Arguments of the MIS-weight kernel (rtr_mis_pick_weights): PickArgs as rtr_shade_hits_picked's (slotsIn may be null: drawn by the rule;
 * defaultWeight = (float)tris / (float)P), and what include/rtr_mis.h needs. */
struct MisPickArgs {
    PickArgs pa;
    float* outWeights;           /* n * P weights for rtr_shade_hits_picked */
    float4* outSamples;          /* n * P RtrMisSample as 2 x float4, or null */
    uint32_t lobes;              /* rtr_bounce_params::lobes of the vertex's bounce */
    uint32_t tris;               /* Ttot: the triangles of the first numAreaLights lights */
    const uint64_t* cdf;         /* null: the uniform rule; else the scene's power table (include/rtr_power.h), and pa.slotsIn is needed */
};

/* Arguments of the resampled-pick kernel (rtr_pick_slots_ris): MisPickArgs as rtr_mis_pick_weights_power's (ma.cdf is needed; ma.pa.slotsIn
 * and ma.outSamples are not read; ma.lobes with mis alone), and what include/rtr_ris.h needs. */
struct RisArgs {
    MisPickArgs ma;              /* ma.pa.outSlots, ma.outWeights: n * P slots and weights for rtr_light_rays_picked / rtr_shade_hits_picked */
    uint32_t candidates;         /* M: 1 ... RTR_RIS_MAX_CANDIDATES */
    uint32_t mis;                /* RTR_RIS_MIS: the targets and the weights carry wPick */
    uint32_t* outCandidates;     /* n * P * M slots, or null */
    float* outTargets;           /* n * P * M targets as used; null exactly when outCandidates is */
};

/* The per-scene triangle -> leaf table (rtr_hit_leaves, rtr_light_rays_hinted): entry base[customIndex] + primitiveId, base = the prefix
 * sum of triCount, is the child code of the BVH2 leaf that holds that world-space record (RtrBvhNode::child: negative); an entry no leaf
 * wrote stays 0.  A start hint of the queued occlusion query (include/rtr.h). */
struct LeafArgs {
    const float4* hits;          /* RtrHit as 2 x float4 */
    int32_t* leaves;             /* one hint per hit */
    const uint32_t* triCount;    /* as SurfaceArgs */
    const uint32_t* base;        /* per customIndex: its first entry of the table */
    const int32_t* table;
    uint32_t numInstances;
    uint32_t n;
};
/* fills the table (zeroed by the caller) from the BVH2: nodes as 2 x uint4 apiece, tris as 3 x float4 apiece.  go: the gate of
 * rtr_bvh.h — null: always; else a device word, and the kernel does nothing when it is 0 */
hipError_t launch_leaf_table(const uint4* nodes, uint32_t numNodes, const float4* tris, uint32_t numTris, const uint32_t* triCount,
                             const uint32_t* base, uint32_t numInstances, int32_t* table, hipStream_t stream, const uint32_t* go = nullptr);
/* rtr_scene_set_instance_masks: rewrites bits 8..15 of every record's flags word from maskBits[customIndex] (the complement of the
 * instance's mask, already shifted); records whose customIndex is past the table (the dummy record of an empty scene) are left alone */
hipError_t launch_set_instance_masks(float4* tris, uint32_t numTris, const uint32_t* maskBits, uint32_t numInstances, hipStream_t stream);
/* leaves[k] = the table entry of hits[k]; 0 for a miss or ids out of range, which read nothing */
hipError_t launch_hit_leaves(const LeafArgs& a, hipStream_t stream);

/* flags: RTR_QUERY_ANY | RTR_QUERY_OPAQUE (validated by the caller).  stats: the counting form, counters added there (zeroed by the caller).
 * rm.masked: the MASKED forms of the two kernels, which read the rays' cull masks (RayMaskArgs) and skip the records of instances whose mask
 * does not meet the ray's; a ray whose effective mask is 0 walks nothing. */
hipError_t launch_query(const DeviceScene& sc, const QueryArgs& qa, uint32_t flags, Counters* stats, hipStream_t stream, const RayMaskArgs& rm = RayMaskArgs());
/* k_query_tail alone, any-hit form: finishes the rays another walk abandoned — qa.ctrl[kQueryRedoWord] of them, their indices in
 * qa.redoList (or, past qa.redoCap, found by the sentinel in qa.occluded) — over the BVH2 (the queued occlusion query's third stage) */
hipError_t launch_query_tail_any(const DeviceScene& sc, const QueryArgs& qa, bool alpha, Counters* stats, hipStream_t stream, const RayMaskArgs& rm = RayMaskArgs());
/* Arguments of the multi-hit query (rtr_trace_rays_multi; kernels/rtr_multihit.hip).  The redo list, the control words and the spill stacks
 * are the context's query scratch, as in QueryArgs. */
struct MultiHitArgs {
    const float4* rays;          /* RtrRay as 2 x float4 */
    const float4* after;         /* per ray: the RtrHit to resume behind (2 x float4), or null */
    float4* hits;                /* n * maxHits RtrHit as 2 x float4, ray-major */
    uint32_t* counts;            /* per ray: hits found, or null */
    uint32_t n;
    uint32_t maxHits;            /* K: 1 .. RTR_MULTIHIT_MAX */
    uint32_t redoCap;            /* entries of redoList the query may use */
    uint32_t* ctrl;              /* kQueryCtrlWords words, zeroed before the launch */
    uint32_t* redoList;
    int32_t* spill;              /* kSpillInts: the tail kernel's full-depth stacks */
};
/* k_multihit + k_multihit_tail: the first maxHits members of every ray's accepted set by (t, customIndex, primitiveId), miss records behind
 * them.  alpha: run the opacity-map test (RTR_QUERY_OPAQUE not given).  rm: the cull mask and the culling flags, always read (the kernels
 * have the filtered form only; rm.masked bit 0 is not looked at).  stats: the counting form.  hipErrorInvalidValue for a maxHits out of range. */
hipError_t launch_multihit(const DeviceScene& sc, const MultiHitArgs& ma, bool alpha, Counters* stats, hipStream_t stream, const RayMaskArgs& rm);
/* The queued occlusion query (rtr_trace_occlusion; kernels/rtr_occlusion.hip): queue build over the rays -> k_shadow_trace4's walk over the
 * 4-wide tree (launch_occlusion_walk) -> k_query_tail.  spill: kSpillInts. */
hipError_t launch_occlusion(const DeviceScene& sc, const OcclusionArgs& oa, const Tunables& tun, bool alpha, int32_t* spill, Counters* stats,
                            hipStream_t stream, uint32_t numCus, const RayMaskArgs& rm = RayMaskArgs());
/* rays one workgroup of the queue build bins: what bounds the batches a launch can append to one list (occlusion_list_stride) */
constexpr uint32_t kOcclusionGenRays = 4096;
constexpr uint32_t occlusion_batch(uint32_t n) { return (size_t)n >= ((size_t)100 << 20) ? 512u : 256u; }
constexpr uint32_t occlusion_list_stride(uint32_t n) {      /* for the shorter batch whatever n is: monotone in n */
    return (uint32_t)((uint64_t)n / 256u / kQueueRegions + ((uint64_t)n + kOcclusionGenRays - 1) / kOcclusionGenRays + 1u);
}
/* width * height * spp camera rays of raygen.rgen:83-107, ray k = (py * width + px) * spp + i (< 2^32, checked by the caller) */
hipError_t launch_camera_rays(const RtrCameraData& cam, uint32_t width, uint32_t height, uint32_t spp, float4* out, hipStream_t stream);
/* one RtrSurface per hit: the renderer's surface fetch (fetch_surface) for caller hits */
hipError_t launch_hit_surfaces(const DeviceScene& sc, const SurfaceArgs& sa, hipStream_t stream);
/* the shadow rays raygen.rgen:206-231 and :299-303 send for each hit, at fixed slots; a slot whose ray is not sent holds the null ray.
 * With la.outLeaves: the same rays and, per slot, the hit's leaf code where the ray leaves into its surface, else 0 */
hipError_t launch_light_rays(const DeviceScene& sc, const LightArgs& la, hipStream_t stream);
/* one RtrRadiance per hit: shade_sample with the visibility bytes of those slots */
hipError_t launch_shade_hits(const DeviceScene& sc, const LightArgs& la, hipStream_t stream);
/* the picked forms: per hit the shadow rays of pa.picks area slots and of the directional light, and the slots; the sums over them */
hipError_t launch_light_rays_picked(const DeviceScene& sc, const PickArgs& pa, hipStream_t stream);
hipError_t launch_shade_hits_picked(const DeviceScene& sc, const PickArgs& pa, hipStream_t stream);
/* per pick the weight under the balance heuristic with the vertex's bounce sample, and optionally what it was made from; with ma.cdf the
 * power form (rtr_mis_pick_weights_power) */
hipError_t launch_mis_pick_weights(const DeviceScene& sc, const MisPickArgs& ma, hipStream_t stream);
/* per pick the slot kept of a.candidates draws from the power table in proportion to their unshadowed contributions, and its weight */
hipError_t launch_pick_slots_ris(const DeviceScene& sc, const RisArgs& a, hipStream_t stream);
/* tonemap_pack of n float3 read strideWords floats apart */
hipError_t launch_tonemap_pack(const float* radiance, uint32_t strideWords, uint32_t n, uint32_t* out, hipStream_t stream);

}  // namespace rtrdev
