/* rtr_api_internal.h — what the files that implement the C ABI of include/rtr.h share (internal to librtr_hip.so): the handle structs
 * rtr_ctx and rtr_scene with the types of their members (DevBuf, BuildScratch, TreeStage, SceneTree), HIP_TRY, and the declarations of
 * the helpers that more than one file calls, each under the name of the file that defines it (as rtrapi::name, and extern "C++" where
 * the definition stands inside that file's extern "C" block).  The ABI is split by subsystem —
 * rtr_api.cpp (errors, context, scene), rtr_api_render.cpp (frames and dispatch), rtr_api_query.cpp (ray queries), rtr_api_paths.cpp
 * (lighting and path vertices), rtr_api_power.cpp (the light-power table and its picks), rtr_api_ris.cpp (the resampled picks) — and a new subsystem gets a file of its own, not a section in one of these.  What is shared and is not
 * a name of the ABI lives in namespace rtrapi, which is hidden: the library exports nothing of it.  A helper one file uses stays
 * static in that file.  No anonymous namespace, no static or thread_local object and no function definition that is not inline
 * belongs here: every file would get a copy of its own (the text behind rtr_last_error is rtr_api.cpp's alone). */
#pragma once
#include "../../include/rtr.h"
#include "kernels/rtr_kernels.h"
#include "kernels/rtr_bvh.h"
#include "rtr_arg_check.h"

#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

namespace rtrdev { struct PickArgs; }      /* kernels/rtr_query.h: named by fill_pick_args below */

using rtrdev::Counters;
using rtrdev::DeviceScene;
using rtrdev::FrameOut;
using rtrdev::RenderArgs;
using rtrdev::Workspace;
/* the pointer tables and the params' rules of rtr_arg_check.h, which the rtr_*_host.cpp share */
using rtrdev::Arg;
using rtrdev::check_ptrs;

namespace rtrapi __attribute__((visibility("hidden"))) {

/* rtr_api.cpp */
int fail(int code, const char* fmt, ...);
int launched(hipError_t e, const char* who);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? RTR_ERR_OUT_OF_MEMORY : RTR_ERR_HIP, "%s failed: %s", #expr, \
                        hipGetErrorString(e_));                                                    \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }      /* owns its memory: moved, never copied */
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    /* a buffer that is reused from call to call and grows on demand (its old contents are not kept) */
    hipError_t grow(size_t count) { return (p && n >= count) ? hipSuccess : alloc(count + count / 2); }
    /* a buffer whose size is fixed by its owner and that is kept from call to call: allocated on first use */
    hipError_t ensure(size_t count) { return (p && n >= count) ? hipSuccess : alloc(count); }
    hipError_t upload(const T* src, size_t count, hipStream_t s) {
        hipError_t e = alloc(count);
        if (e != hipSuccess) return e;
        if (count == 0 || !src) return hipSuccess;
        e = hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(s);
    }
};

/* The tree of a scene.  A member is here if and only if it must not outlive the tree: its content or its size is a function of the node
 * count, the leaf order or the boxes.  rtr_scene_rebuild builds a fresh SceneTree and swaps it in whole, so whatever is here starts
 * empty with a new tree and is made again by the call that needs it; what is per customIndex, per instance or per vertex, and the
 * status of the enqueued updates, stays on rtr_scene and is kept through a rebuild. */
struct SceneTree {
    DevBuf<uint4> nodes;                 /* RtrBvhNode, 2 x uint4 each */
    DevBuf<float4> nodesF;               /* rtr::BvhNodeF, 4 x float4 each: device build / refit only */
    DevBuf<RtrBvhGrid> grid;
    DevBuf<unsigned long long> wideSums;     /* scratch of bvh_make_wide */
    DevBuf<uint4> nodes4tmp;             /* the 4-wide entries in BVH2-id order, before the permutation into the resident order */
    DevBuf<uint32_t> wideRemap;          /* the permutation (numNodes words), then bvh_hot_top's scratch */
    DevBuf<uint8_t> wideShape;           /* per BVH2 node: which entries its 4-wide record opens (host builder's cost-driven collapse); empty = greedy */
    std::vector<uint8_t> hostWideShape;
    uint32_t wideReached = 0;            /* entries the 4-wide tree reaches (they come first in nodes4) */
    DevBuf<uint4> nodes4;                /* RtrWideNode: 4-wide view of the tree for the any-hit kernel, resident order: best-first top, then breadth-first (kernels/rtr_hot_top.h) */
    DevBuf<float4> tris;
    std::vector<RtrBvhNode> hostNodes;
    std::vector<RtrBvhTri> hostTris;
    /* device build / refit state (kernels/rtr_bvh.hip) */
    DevBuf<rtrdev::PrimRef> prims;
    DevBuf<rtrdev::InstanceRef> instRefs;
    DevBuf<float4> boxMin, boxMax;
    DevBuf<int32_t> parent;
    DevBuf<uint32_t> counters, depth, slotOfPrim, red;
    uint32_t numPrims = 0, numNodeSlots = 0;
    bool refitReady = false;
    /* the triangle -> leaf table (rtr_hit_leaves, rtr_light_rays_hinted): made by the first call that asks for it (ensure_leaf_table), kept
     * through refits, which keep topology and leaf order.  mutable: the query calls take the scene const */
    mutable DevBuf<int32_t> leafTable;
    mutable bool leafReady = false;
    /* rtr_scene_tree_cost: for a tree without refit arrays whose slots are not all reachable, a parent array of its own (costParentState:
     * 0 not looked at yet, 1 every slot is in the tree, 2 costParent holds it).  mutable: the call takes the scene const, like the leaf table */
    mutable DevBuf<int32_t> costParent;
    mutable int costParentState = 0;
    /* the enqueued updates (rtr_scene_prepare_async_updates): k_wide_order's scratch (2 x numNodes words).  asyncReady: prims and instRefs
     * are on the device for this tree, it is refit-ready, and the scratch and the scene's asyncWords and instCustom exist */
    DevBuf<uint32_t> orderScratch;
    bool asyncReady = false;
    /* the enqueued rebuild (rtr_scene_prepare_async_rebuild): this tree has a device build's array sizes, and the scene's stage and
     * build scratch exist.  Here and not on the scene: a new tree starts unprepared (a host rebuild's has other sizes) */
    bool rebuildReady = false;
    /* the rebuild policy (rtr_scene_prepare_async_rebuild_if): rebuildReady, the scene's policy words exist, and their baseline is the
     * cost of THIS tree right after it was built */
    bool rebuildIfReady = false;
    rtr_scene_stats stats{};
};

}  // namespace rtrapi

using rtrapi::DevBuf;
using rtrapi::SceneTree;

struct rtr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    hipDeviceProp_t prop;
    int numXccs = 0;                     /* hipDeviceAttributeNumberOfXccs (reported by rtr_ctx_device_name): the kernels' eight batch cursors stay private to one XCD each for 8, 4, 2 or 1 XCDs — kernels/rtr_kernels.h, kQueueRegions */
    /* scenes and frames keep a pointer to their context: a context destroyed while it still has children lives on,
     * unusable, until the last child is gone (garbage-collected bindings destroy objects in any order) */
    int children = 0;
    bool destroyed = false;
    rtrdev::Tunables tun;                /* run-time tunables of the staged pipeline: environment at creation, rtr_ctx_set_tunable afterwards */
    /* ray queries (rtr_trace_rays): the tail kernel's scratch — control block, redo list (kQueryRedoCap entries), full-depth stacks —
     * and the counters of the counting form.  Allocated by the first query and reused by every later one: its size does not depend on
     * the number of rays.  qEv: around the query's kernels (timing, and what a query enqueued on another stream waits for). */
    DevBuf<uint32_t> qCtrl, qRedo;
    DevBuf<int32_t> qSpill;
    DevBuf<Counters> qCounters;
    hipEvent_t qEv[2] = {nullptr, nullptr};
    hipStream_t qLastStream = nullptr;   /* the stream the last query was enqueued on */
};

/* what the device LBVH build needs while it runs (rtrdev::BvhScratch): rtr_scene_create frees it with the call, a scene that has been
 * rebuilt on the device keeps it for the next rebuild (sizes depend on the triangle count alone, which no call changes) */
struct BuildScratch {
    DevBuf<float4> trisCanon, minCanon, maxCanon;
    DevBuf<unsigned long long> keysIn, keysOut;
    DevBuf<int2> range, rawChild;
    DevBuf<uint8_t> sortTemp;
    size_t sortTempBytes = 0;            /* what hipcub asked for (sortTemp may be larger) */
};

/* rtr_scene_rebuild_async's stage: a second set of the arrays a device build writes, which nothing else reads.  The enqueued build fills
 * it, k_commit_tree copies it over the live arrays — or does not.  Sizes depend on the triangle count alone; counters and depth are not
 * staged: they are scratch of whatever fit runs next on the scene's stream, and the build uses the live tree's. */
struct TreeStage {
    DevBuf<uint4> nodes;
    DevBuf<float4> nodesF, tris, boxMin, boxMax;
    DevBuf<RtrBvhGrid> grid;
    DevBuf<int32_t> parent;
    DevBuf<uint32_t> slotOfPrim, red;
};

struct rtr_scene {
    rtr_ctx* ctx = nullptr;
    SceneTree tree;
    DevBuf<RtrVertex> vertices;
    DevBuf<uint32_t> indices;
    DevBuf<RtrObjectInfo> objects;       /* written once, by rtr_scene_create: no update, refit or rebuild call touches it ... */
    DevBuf<float4> objectTerms;          /* ... so the per-object material terms made from it (rtrdev::launch_object_terms) are made once too */
    DevBuf<RtrAreaLightInfo> lights;
    DevBuf<float4> lightTris;            /* 4 x float4 per light triangle (rtrdev::launch_light_tris) */
    DevBuf<uint32_t> lightTriFirst;      /* first record of light l */
    DevBuf<uint32_t> triCount;           /* per customIndex: triangles of the light or of the instance's mesh (rtr_hit_surfaces' range check) */
    uint32_t numInstances = 0;
    /* instance cull masks (rtr_scene_set_instance_masks): one byte per instance, in instance order; empty = never set, every mask 0xff.
     * The records carry them (bits 8..15 of flags, complemented); this table is what the getter returns and what a refit re-applies */
    std::vector<uint8_t> hostMasks;
    DevBuf<uint32_t> maskBits;           /* per customIndex: (~mask & 0xff) << 8, the setter kernel's table */
    std::vector<uint32_t> hostTriCount;
    mutable DevBuf<uint32_t> leafBase;   /* per customIndex: prefix sum of triCount (made with the tree's leaf table) */
    DevBuf<float> xforms, nmats, ltc1, ltc2;
    std::vector<DevBuf<uint8_t>> texPixels;
    DevBuf<uint8_t> hdriPixels;
    /* the sky table (rtr_scene_prepare_sky, or the first call that needs it: ensure_sky_table): the rows' 32-bit prefix sums and the 64-bit
     * marginal sums.  The HDRI and the sky colour are fixed for the scene's life, so nothing ever remakes it.  mutable: the sky calls
     * take the scene const, like the leaf table */
    mutable DevBuf<uint32_t> skyRows;
    mutable DevBuf<uint64_t> skyMarginal;
    mutable bool skyReady = false;
    /* the light-power table (rtr_scene_prepare_light_power, or the first call that needs it: ensure_light_power): one weight and one
     * 64-bit inclusive sum per light triangle of all lights, and the word the build's maximum is folded into.  Their sizes are fixed
     * for the scene's life; their CONTENT follows the light triangles and the light infos: whoever rewrites those enqueues the build
     * behind the write (enqueue_light_power), once powerReady.  mutable: as the sky table */
    mutable DevBuf<uint32_t> powerWeights, powerMax;
    mutable DevBuf<uint64_t> powerCdf;
    mutable uint32_t powerTris = 0;
    mutable bool powerReady = false;
    DevBuf<rtrdev::DeviceTexture> texTable;
    std::vector<RtrAreaLightInfo> hostLights;
    std::vector<RtrInstance> hostInstances;
    std::vector<RtrMesh> hostMeshes;
    std::vector<RtrObjectInfo> hostObjects;
    /* rtr_scene_update_vertices: the device table of ranges, their prefix counts (+ the "first bad vertex" word), and the staging
     * buffer host data is packed into (vtxHost) and copied to (vtxStage); they grow on demand and are reused by every call */
    DevBuf<rtrdev::VertexRange> vtxRanges;
    DevBuf<uint32_t> vtxPrefix, vtxStage;
    std::vector<uint32_t> vtxHost;
    BuildScratch buildScratch;           /* rtr_scene_rebuild with RTR_BUILD_DEVICE_LBVH: empty until the first one */
    TreeStage stage;                     /* rtr_scene_prepare_async_rebuild: kept through synchronous rebuilds, like the scratch */
    /* an enqueued rebuild has run (or will) since stats.maxDepth was read back: refresh_mirrors takes it from the live red[7] */
    mutable bool depthStale = false;
    /* the rebuild policy's device memory (rtr_scene_prepare_async_rebuild_if), the scene's and not the tree's — the counts go on through
     * a synchronous rebuild: k_tree_cost's eleven words, a pad word, then one rtrdev::RebuildIfRecord (kPolicyRecordAt) */
    DevBuf<unsigned long long> policy;
    /* the enqueued updates (made by rtr_scene_prepare_async_updates): the words of the enqueued chain — [0] the first bad vertex of the
     * update in flight, [1] the entries the 4-wide tree reaches, [4..6] the sticky status (refused count, serial of the first refused
     * update since the last status call, its first bad vertex).
     * mirrorsStale: an enqueued update has run (or will) since the tree's hostNodes, hostTris, stats.grid, stats.boxPad and wideReached
     * were read back; refresh_mirrors joins the stream and reads them again.  mutable: the export calls take the scene const */
    DevBuf<uint32_t> asyncWords;
    mutable bool mirrorsStale = false;
    /* rtr_scene_update_instances_async: per instance, in instance order, its customIndex (fixed for the scene's life; made by
     * rtr_scene_prepare_async_updates).  instancesStale: an enqueued instance update has run (or will) since hostInstances' transforms
     * and hostLights were current; set together with mirrorsStale, refresh_mirrors reads them back from instRefs and lights */
    DevBuf<uint32_t> instCustom;
    mutable bool instancesStale = false;
    uint64_t asyncEnqueued = 0;
    mutable DevBuf<unsigned long long> costWords;      /* rtr_scene_tree_cost: the kernel's words */
    DeviceScene dev{};
    uint32_t numLights = 0, numObjects = 0, numVertices = 0, numIndices = 0;
    bool hasLtc = false;
};

namespace rtrapi __attribute__((visibility("hidden"))) {

/* rtr_api.cpp */
int ctx_create_prio(int ordinal, int priorityRank, rtr_ctx** out);
void ctx_release_child(rtr_ctx* c);
int refresh_mirrors(const rtr_scene* cs);

/* rtr_api_query.cpp */
bool aligned16(const void* p);
bool aligned4(const void* p);
int check_handles(const rtr_ctx* c, const rtr_scene* s, const char* who);
int check_same_device(const rtr_ctx* c, const rtr_scene* s, const char* who);
int join_if_enqueued(rtr_ctx* c, int rc, uint32_t n);
int ensure_leaf_table(rtr_ctx* c, const rtr_scene* s, const char* who);

/* rtr_api_paths.cpp */
int picked_scene_checks(const rtr_ctx* c, const rtr_scene* s, const rtr_light_params* p, const char* who, uint32_t* areaSlots, uint32_t* tris);
void fill_pick_args(rtrdev::PickArgs& pa, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                    const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, uint32_t areaSlots, uint32_t tris);

/* rtr_api_power.cpp */
/* makes the scene's power table if it has none: allocates, builds on `st` (the current device is the scene's) and JOINS, as the sky table */
int ensure_light_power(const rtr_scene* s, hipStream_t st, const char* who);
/* a scene that has a table: the build's launches on `st`, behind whatever rewrote the light triangles or the light infos there; no
 * allocation, no join.  A scene without one: nothing */
int enqueue_light_power(const rtr_scene* s, hipStream_t st, const char* who);

}  // namespace rtrapi
