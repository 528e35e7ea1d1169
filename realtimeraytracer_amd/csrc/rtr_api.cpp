/* rtr_api.cpp — implementation of the C ABI in include/rtr.h (host side of librtr_hip.so).
 * HIP runtime for device memory / streams / events; kernels in kernels/rtr_kernels.hip.
 * There is NO CPU rendering fallback in this library: without a HIP device every entry point
 * that needs one fails with RTR_ERR_NO_DEVICE / RTR_ERR_HIP. */
#include "../../include/rtr.h"
#include "../../include/rtr_math.h"
#include "bvh_build.h"
#include "kernels/rtr_kernels.h"
#include "kernels/rtr_post.h"
#include "kernels/rtr_bvh.h"
#include "kernels/rtr_mirrored.h"
#include "kernels/rtr_tree_sah.h"
#include "kernels/rtr_query.h"
#include "kernels/rtr_bounce_launch.h"
#include "rtr_bounce_host.h"
#include "kernels/rtr_paths_launch.h"
#include "rtr_paths_host.h"
#include "rtr_pick_host.h"
#include "kernels/rtr_mis_launch.h"
#include "rtr_mis_host.h"
#include "kernels/rtr_sky_launch.h"
#include "rtr_sky_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using rtrdev::Counters;
using rtrdev::DeviceScene;
using rtrdev::FrameOut;
using rtrdev::RenderArgs;
using rtrdev::Workspace;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

/* the status of a call whose kernel launcher returned e */
int launched(hipError_t e, const char* who) {
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
    return RTR_OK;
}

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

}  // namespace

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

static void ctx_free(rtr_ctx* c) {
    (void)hipSetDevice(c->device);
    if (c->qLastStream) (void)hipEventSynchronize(c->qEv[1]);      /* the scratch below is freed with the context */
    for (hipEvent_t e : c->qEv) if (e) (void)hipEventDestroy(e);
    if (c->ownStream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}
static void ctx_release_child(rtr_ctx* c) {
    if (--c->children == 0 && c->destroyed) ctx_free(c);
}

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

/* The tree of a scene.  A member is here if and only if it must not outlive the tree: its content or its size is a function of the node
 * count, the leaf order or the boxes.  rtr_scene_rebuild builds a fresh SceneTree and swaps it in whole, so whatever is here starts
 * empty with a new tree and is made again by the call that needs it; what is per customIndex, per instance or per vertex, and the
 * status of the enqueued updates, stays on rtr_scene and is kept through a rebuild. */
namespace {
struct SceneTree {
    DevBuf<uint4> nodes;                 /* RtrBvhNode, 2 x uint4 each */
    DevBuf<float4> nodesF;               /* rtr::BvhNodeF, 4 x float4 each: device build / refit only */
    DevBuf<RtrBvhGrid> grid;
    DevBuf<unsigned long long> wideSums;     /* scratch of bvh_make_wide */
    DevBuf<uint4> nodes4tmp;             /* the 4-wide entries in BVH2-id order, before the breadth-first permutation */
    DevBuf<uint32_t> wideRemap;
    DevBuf<uint8_t> wideShape;           /* per BVH2 node: which entries its 4-wide record opens (host builder's cost-driven collapse); empty = greedy */
    std::vector<uint8_t> hostWideShape;
    uint32_t wideReached = 0;            /* entries the 4-wide tree reaches (they come first in nodes4) */
    DevBuf<uint4> nodes4;                /* RtrWideNode: 4-wide view of the tree for the any-hit kernel, breadth-first order (kernels/rtr_bvh.hip) */
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
}  // namespace

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

constexpr size_t kPolicyRecordAt = 12, kPolicyWords = kPolicyRecordAt + sizeof(rtrdev::RebuildIfRecord) / sizeof(unsigned long long);
static rtrdev::RebuildIfRecord* policy_record(const rtr_scene* s) { return reinterpret_cast<rtrdev::RebuildIfRecord*>(s->policy.p + kPolicyRecordAt); }

/* no geometry: the host builder's tree of such a scene is one node over one placeholder record */
static bool scene_is_empty(const rtr_scene* s) { return s->tree.hostTris.empty() || s->tree.hostTris[0].customIndex == 0xffffffffu; }

struct rtr_frame {
    rtr_ctx* ctx = nullptr;
    uint32_t width = 0, rows = 0, images = 0;
    DevBuf<uint32_t> img[8];
    uint32_t* ext[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf<float4> hdr;
    /* wavefront scratch */
    DevBuf<float4> hitTuvp, rayDT, rayOrigin;      /* hit records; per ray (direction, tmax); per pixel-sample the shadow rays' origin */
    DevBuf<uint32_t> raySlot;                      /* per ray: index of its visibility byte */
    uint32_t slotStride = 0;                       /* distance of the visibility planes: a power of two >= the pixel-sample slots */
    uint32_t visFill = 1;                          /* pre-fill of the visibility array for the next launch: the commoner outcome of the last one (1 = occluded) */
    DevBuf<uint32_t> hitCustom, queueCount;
    DevBuf<uint8_t> vis;
    DevBuf<int32_t> spill;
    DevBuf<uint32_t> overflow;
    uint32_t overflowCap = 0;
    DevBuf<uint2> batchLists;
    DevBuf<unsigned long long> clk;
    uint32_t listStride = 0;
    DevBuf<Counters> counters;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   /* [5]: between the any-hit kernel and k_shadow_tail */
    hipEvent_t evMega[2] = {nullptr, nullptr};
    rtr_frame_stats stats{};
    bool pendingStats = false, pendingWave = false, pendingCounters = false;
    uint32_t pendingImagesK = 0; bool pendingHdr = false, pendingAccum = false;
    hipEvent_t evDone = nullptr;         /* a frame rendered as a later frame of a batch: recorded on the leading frame's stream behind the launch */
    bool viaBatch = false;
    /* ordering between a batch launch (on the leading frame's stream) and the other frames' own streams, paid only when it is needed:
     * batchStream = the stream of the launch that last wrote this frame as a later frame of a batch and has not been joined (evDone
     * marks its end); ownPending = the frame's own stream may still hold work for it (a launch it led); evOwn orders a later batch
     * behind that work */
    hipStream_t batchStream = nullptr;
    bool ownPending = false;
    hipEvent_t evOwn = nullptr;
    /* rtr_render_split_async: the frame as band-shards ("parts") on streams of their own.  A part is an internal frame object — its
     * own scratch, events, counters and context (= stream) — that owns no image: it is bound to THIS frame's images and writes its
     * rows where they belong (RenderArgs::directRows) */
    std::vector<rtr_ctx*> partCtx;
    std::vector<rtr_frame*> parts;
    std::vector<hipEvent_t> evPart;      /* part k's launches are done (recorded on its stream, waited for by this frame's) */
    hipEvent_t evSplit[2] = {nullptr, nullptr};     /* on this frame's stream: the fork, and behind the join — the split render's duration */
    uint32_t pendingSplit = 0;           /* parts of the split render in flight (0: the last render was not split) */
    float4* extHdr = nullptr;            /* a part: the HDR image of the frame it belongs to */
    uint32_t* image_ptr(int which) const { return ext[which] ? ext[which] : img[which].p; }
    float4* hdr_ptr() const { return extHdr ? extHdr : hdr.p; }
};

/* rtr_bounce_host.cpp's way to this thread's error text */
void rtrdev::set_last_error(const char* msg) { g_err = msg; }

extern "C" {

const char* rtr_last_error(void) { return g_err.c_str(); }

const char* rtr_status_string(int s) {
    switch (s) {
        case RTR_OK: return "RTR_OK";
        case RTR_ERR_INVALID_ARGUMENT: return "RTR_ERR_INVALID_ARGUMENT";
        case RTR_ERR_HIP: return "RTR_ERR_HIP";
        case RTR_ERR_NO_DEVICE: return "RTR_ERR_NO_DEVICE";
        case RTR_ERR_UNSUPPORTED: return "RTR_ERR_UNSUPPORTED";
        case RTR_ERR_OUT_OF_MEMORY: return "RTR_ERR_OUT_OF_MEMORY";
        case RTR_ERR_BVH_TOO_DEEP: return "RTR_ERR_BVH_TOO_DEEP";
        case RTR_ERR_IO: return "RTR_ERR_IO";
        default: return "RTR_ERR_UNKNOWN";
    }
}

int rtr_abi_version(void) { return RTR_ABI_VERSION; }

const char* rtr_kernel_revision(void) { return RTR_ANYHIT_KERNEL_REVISION; }

uint32_t rtr_shard_rows(uint32_t height, uint32_t bandRows, uint32_t shardCount) {
    if (bandRows == 0) bandRows = 8;
    if (shardCount <= 1) return height;               /* unsharded: no padding rows */
    uint32_t bands = (height + bandRows - 1) / bandRows;
    uint32_t per = (bands + shardCount - 1) / shardCount;
    return per * bandRows;
}

/* ---- context ------------------------------------------------------------------------------ */
/* priorityRank < 0: a stream of default priority.  >= 0: rank 0 gets the device's highest stream priority, rank 1 the next ... (the
 * parts of a split render: the dispatcher then prefers the workgroups of an earlier part wherever two parts compete for a slot) */
static int ctx_create_prio(int ordinal, int priorityRank, rtr_ctx** out) {
    if (!out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_create: out is null");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(RTR_ERR_NO_DEVICE, "rtr_ctx_create: no HIP device (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (ordinal < 0 || ordinal >= count) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_create: ordinal %d not in [0,%d)", ordinal, count);
    HIP_TRY(hipSetDevice(ordinal));
    rtr_ctx* c = new rtr_ctx();
    c->device = ordinal;
    e = hipGetDeviceProperties(&c->prop, ordinal);
    if (e != hipSuccess) { delete c; return fail(RTR_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e)); }
    if (hipDeviceGetAttribute(&c->numXccs, hipDeviceAttributeNumberOfXccs, ordinal) != hipSuccess) c->numXccs = 0;
    if (priorityRank >= 0) {
        int least = 0, greatest = 0;                     /* numerically: greatest priority = the smaller number */
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; }
        int prio = greatest + priorityRank;
        if (prio > least) prio = least;
        e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio);
    } else e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(RTR_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    c->ownStream = true;
    c->tun = rtrdev::tunables_from_env();
    *out = c;
    return RTR_OK;
}

int rtr_ctx_create(int ordinal, rtr_ctx** out) { return ctx_create_prio(ordinal, -1, out); }

int rtr_ctx_set_tunable(rtr_ctx* c, const char* name, uint32_t value) {
    if (!c || !name) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_set_tunable: null argument");
    if (!rtrdev::tunable_set(c->tun, name, value)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_set_tunable: no tunable '%s', or %u is outside its range", name, value);
    return RTR_OK;
}

int rtr_ctx_get_tunable(const rtr_ctx* c, const char* name, uint32_t* value) {
    if (!c || !name || !value) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_get_tunable: null argument");
    if (!rtrdev::tunable_get(c->tun, name, value)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_get_tunable: no tunable '%s'", name);
    return RTR_OK;
}

void rtr_ctx_destroy(rtr_ctx* c) {
    if (!c || c->destroyed) return;
    if (c->children > 0) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); c->destroyed = true; return; }
    ctx_free(c);
}

int rtr_ctx_set_stream(rtr_ctx* c, void* s) {
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_set_stream: ctx is null");
    HIP_TRY(hipSetDevice(c->device));
    if (c->ownStream && c->stream) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipStreamDestroy(c->stream); }
    if (s) { c->stream = (hipStream_t)s; c->ownStream = false; }
    else { HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->ownStream = true; }
    return RTR_OK;
}

int rtr_ctx_get_stream(rtr_ctx* c, void** out) {
    if (!c || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_get_stream: null argument");
    *out = (void*)c->stream;
    return RTR_OK;
}

int rtr_ctx_device_name(rtr_ctx* c, char* buf, size_t bytes) {
    if (!c || !buf || bytes == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_ctx_device_name: bad argument");
    if (c->numXccs > 0) snprintf(buf, bytes, "%s (%s, %d CUs in %d XCDs)", c->prop.name, c->prop.gcnArchName, c->prop.multiProcessorCount, c->numXccs);
    else snprintf(buf, bytes, "%s (%s)", c->prop.name, c->prop.gcnArchName);
    return RTR_OK;
}

/* ---- scene -------------------------------------------------------------------------------- */
static int validate_desc(const rtr_scene_desc* d) {
    if (!d) return fail(RTR_ERR_INVALID_ARGUMENT, "scene desc is null");
    if ((d->numVertices && !d->vertices) || (d->numIndices && !d->indices) || (d->numMeshes && !d->meshes) ||
        (d->numInstances && !d->instances) || (d->numObjects && !d->objects) || (d->numLights && !d->lights))
        return fail(RTR_ERR_INVALID_ARGUMENT, "scene desc: null array with non-zero count");
    if ((d->ltc1 == nullptr) != (d->ltc2 == nullptr)) return fail(RTR_ERR_INVALID_ARGUMENT, "scene desc: ltc1 and ltc2 must both be given or both null");
    for (uint32_t m = 0; m < d->numMeshes; ++m) {
        const RtrMesh& me = d->meshes[m];
        if (me.indexCount % 3u) return fail(RTR_ERR_INVALID_ARGUMENT, "mesh %u: indexCount %u not a multiple of 3", m, me.indexCount);
        if ((uint64_t)me.indexOffset + me.indexCount > d->numIndices) return fail(RTR_ERR_INVALID_ARGUMENT, "mesh %u: index range exceeds the index array", m);
        if ((uint64_t)me.vertexOffset + me.vertexCount > d->numVertices) return fail(RTR_ERR_INVALID_ARGUMENT, "mesh %u: vertex range exceeds the vertex array", m);
        for (uint32_t i = 0; i < me.indexCount; ++i)
            if (d->indices[me.indexOffset + i] >= me.vertexCount)
                return fail(RTR_ERR_INVALID_ARGUMENT, "mesh %u: index %u (= %u) outside its %u vertices", m, i, d->indices[me.indexOffset + i], me.vertexCount);
    }
    std::vector<uint8_t> seen(d->numInstances, 0);
    for (uint32_t i = 0; i < d->numInstances; ++i) {
        const RtrInstance& in = d->instances[i];
        if (in.meshIndex >= d->numMeshes) return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: meshIndex %u >= %u", i, in.meshIndex, d->numMeshes);
        if (in.customIndex >= d->numInstances || seen[in.customIndex]) return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: customIndex %u out of range or duplicated", i, in.customIndex);
        seen[in.customIndex] = 1;
        if (in.customIndex >= d->numLights && in.customIndex - d->numLights >= d->numObjects)
            return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: customIndex %u has no ObjectInfo (numLights %u, numObjects %u)", i, in.customIndex, d->numLights, d->numObjects);
        if (in.customIndex >= d->numLights) {
            /* the hit shader reads indices / vertices through the ObjectInfo's offsets (closesthit.rchit:59-65), which the
             * reference sets to the mesh's own when it builds the TLAS (tlas.cppm:58-71): anything else would fetch another
             * mesh's data, or none */
            const RtrObjectInfo& oi = d->objects[in.customIndex - d->numLights];
            const RtrMesh& me = d->meshes[in.meshIndex];
            if (oi.vertexOffset != me.vertexOffset || oi.indexOffset != me.indexOffset)
                return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: ObjectInfo offsets (%u, %u) differ from its mesh's (%u, %u)", i, oi.vertexOffset, oi.indexOffset,
                            me.vertexOffset, me.indexOffset);
        }
        for (int k = 0; k < 12; ++k)
            if (!(in.transform[k] == in.transform[k]) || in.transform[k] > 3.0e38f || in.transform[k] < -3.0e38f)
                return fail(RTR_ERR_INVALID_ARGUMENT, "instance %u: non-finite transform", i);
    }
    if (d->numLights > d->numInstances) return fail(RTR_ERR_INVALID_ARGUMENT, "numLights %u > numInstances %u (lights are the first instances)", d->numLights, d->numInstances);
    if (d->numTextures && !d->textures) return fail(RTR_ERR_INVALID_ARGUMENT, "scene desc: null texture array with non-zero count");
    auto tex_ok = [&](const rtr_texture& t) { return t.pixels && t.width > 0 && t.height > 0 && t.width <= 65536 && t.height <= 65536 && (t.channels == 1 || t.channels == 4); };
    for (uint32_t t = 0; t < d->numTextures; ++t)
        if (d->textures[t].pixels && !tex_ok(d->textures[t])) return fail(RTR_ERR_INVALID_ARGUMENT, "texture %u: bad extent %ux%u or channels %u (1 or 4)", t, d->textures[t].width, d->textures[t].height, d->textures[t].channels);
    if (d->hdri && !tex_ok(*d->hdri)) return fail(RTR_ERR_INVALID_ARGUMENT, "hdri: bad extent or channels");
    for (uint32_t o = 0; o < d->numObjects; ++o) {
        const RtrObjectInfo& oi = d->objects[o];
        const struct { uint32_t uses, index; const char* what; } maps[4] = {{oi.usesColorMap, oi.colorIndex, "color"}, {oi.usesSpecularMap, oi.specularIndex, "specular"},
                                                                            {oi.usesMetallicMap, oi.metallicIndex, "metallic"}, {oi.usesOpacityMap, oi.opacityIndex, "opacity"}};
        for (const auto& m : maps)
            if (m.uses && (m.index >= d->numTextures || !d->textures[m.index].pixels))
                return fail(RTR_ERR_INVALID_ARGUMENT, "object %u uses a %s map but texture index %u is not in the texture array (%u entries); "
                            "the library never substitutes a constant for a missing texture", o, m.what, m.index, d->numTextures);
    }
    for (uint32_t l = 0; l < d->numLights; ++l) {
        const RtrAreaLightInfo& li = d->lights[l];
        if ((uint64_t)li.indexOffset + 3ull * li.numTriangles > d->numIndices) return fail(RTR_ERR_INVALID_ARGUMENT, "light %u: triangle range exceeds the index array", l);
        for (uint32_t i = 0; i < 3u * li.numTriangles; ++i)
            if ((uint64_t)li.vertexOffset + d->indices[li.indexOffset + i] >= d->numVertices)
                return fail(RTR_ERR_INVALID_ARGUMENT, "light %u: vertex reference outside the vertex array", l);
    }
    return RTR_OK;
}

/* The mirrored bit of an instance (the ray queries' face culling, RTR_QUERY_CULL_BACK/FRONT_FACING): 1 iff the determinant of its 3x3
 * transform, evaluated in double, is negative — the instance turns the winding of its triangles over, and Vulkan decides facing in object
 * space.  It lives in word kMirroredWord of the instance's 12-float slot of the normal-matrix table, which the matrix does not use: a
 * per-customIndex table that is uploaded with the transforms by create, create_like and update_instances, and that no triangle record
 * and no kernel argument had to change for.  The determinant is rtr_mirrored_bit (kernels/rtr_mirrored.h), which the enqueued instance update's kernel evaluates too. */
static void set_mirrored_word(const float* m, float* nmatSlot) {
    const uint32_t bit = rtr_mirrored_bit(m);
    memcpy(&nmatSlot[rtrdev::kMirroredWord], &bit, sizeof bit);
}

/* the per-customIndex transform tables: the 3x4 transforms, and the normal matrices with the mirrored word */
static void instance_tables(uint32_t numInstances, const RtrInstance* instances, std::vector<float>& xforms, std::vector<float>& nmats) {
    xforms.assign(12 * (size_t)numInstances, 0.f);
    nmats.assign(12 * (size_t)numInstances, 0.f);
    for (uint32_t i = 0; i < numInstances; ++i) {
        memcpy(&xforms[12 * (size_t)instances[i].customIndex], instances[i].transform, 12 * sizeof(float));
        rtr_normal_matrix(instances[i].transform, &nmats[12 * (size_t)instances[i].customIndex]);
        set_mirrored_word(instances[i].transform, &nmats[12 * (size_t)instances[i].customIndex]);
    }
}

/* flatten TLAS instances to one world-space triangle soup (instance order, then primitive order),
 * fill the per-customIndex transform tables, build the BVH */
static int flatten_and_build(const rtr_scene_desc* d, rtr::BvhResult& bvh, std::vector<float>& xforms, std::vector<float>& nmats,
                             uint32_t* stackEntries, size_t* numTris) {
    std::vector<rtr::WorldTriangle> soup;
    size_t total = 0;
    for (uint32_t i = 0; i < d->numInstances; ++i) total += d->meshes[d->instances[i].meshIndex].indexCount / 3u;
    soup.reserve(total);
    instance_tables(d->numInstances, d->instances, xforms, nmats);
    for (uint32_t i = 0; i < d->numInstances; ++i) {
        const RtrInstance& in = d->instances[i];
        const RtrMesh& me = d->meshes[in.meshIndex];
        for (uint32_t t = 0; t < me.indexCount / 3u; ++t) {
            rtr::WorldTriangle w;
            for (int k = 0; k < 3; ++k) {
                const uint32_t idx = d->indices[me.indexOffset + 3u * t + k] + me.vertexOffset;
                const rtr_v3 p = rtr_xform_point34(in.transform, rtr_ld3(d->vertices[idx].position));
                w.v[k][0] = p.x; w.v[k][1] = p.y; w.v[k][2] = p.z;
            }
            w.customIndex = in.customIndex; w.primitiveId = t;
            /* any-hit (opacity.rahit) runs only on non-opaque geometry (blas.cppm:98-100) of objects with an opacity map */
            w.flags = (in.customIndex >= d->numLights && d->objects[in.customIndex - d->numLights].usesOpacityMap != 0 && me.isOpaque == 0) ? 1u : 0u;
            soup.push_back(w);
        }
    }
    std::string err;
    if (!rtr::build_bvh(soup, bvh, &err)) return fail(RTR_ERR_INVALID_ARGUMENT, "BVH build: %s", err.c_str());
    if (bvh.maxDepth > 64)
        return fail(RTR_ERR_BVH_TOO_DEEP, "BVH depth %u exceeds the 64-entry LDS traversal stack", bvh.maxDepth);
    *stackEntries = bvh.maxDepth <= 16 ? 16 : (bvh.maxDepth <= 32 ? 32 : 64);
    *numTris = soup.size();
    return RTR_OK;
}

static void fill_stats(rtr_scene_stats& st, const rtr::BvhResult& bvh, uint32_t stackEntries, size_t numTris) {
    memset(&st, 0, sizeof st);
    st.numTriangles = (uint32_t)numTris;
    st.numNodes = (uint32_t)bvh.nodes.size();
    st.maxDepth = bvh.maxDepth;
    st.maxLeafSize = bvh.maxLeafSize;
    st.bvhLayoutVersion = RTR_BVH_LAYOUT_VERSION;
    st.stackEntries = stackEntries;
    st.buildMs = bvh.buildMs;
    st.sahCost = bvh.sahCost;
    st.grid = bvh.grid;
    for (int k = 0; k < 3; ++k) { st.boundsMin[k] = bvh.boundsMin[k]; st.boundsMax[k] = bvh.boundsMax[k]; }
    st.boxPad = bvh.boxPad;
}

int rtr_host_build_bvh(const rtr_scene_desc* d, rtr_scene_stats* stats, RtrBvhNode* nodes, size_t nodeBytes, RtrBvhTri* tris, size_t triBytes) {
    return rtr_host_build_bvh_wide(d, stats, nodes, nodeBytes, tris, triBytes, nullptr, 0);
}

int rtr_host_build_bvh_wide(const rtr_scene_desc* d, rtr_scene_stats* stats, RtrBvhNode* nodes, size_t nodeBytes, RtrBvhTri* tris, size_t triBytes,
                            RtrWideNode* wide, size_t wideBytes) {
    int rc = validate_desc(d);
    if (rc != RTR_OK) return rc;
    rtr::BvhResult bvh; std::vector<float> xf, nm; uint32_t stackEntries = 0; size_t numTris = 0;
    rc = flatten_and_build(d, bvh, xf, nm, &stackEntries, &numTris);
    if (rc != RTR_OK) return rc;
    if (stats) fill_stats(*stats, bvh, stackEntries, numTris);
    if (wide || (stats && !nodes && !tris)) {
        std::vector<RtrWideNode> w;
        rtr::make_wide_host(bvh.nodes.data(), bvh.nodes.size(), bvh.wideShape.size() == bvh.nodes.size() ? bvh.wideShape.data() : nullptr, bvh.grid, w);
        if (stats) { stats->grid = bvh.grid; stats->numWideNodes = (uint32_t)w.size(); stats->wideLayoutVersion = RTR_WIDE_LAYOUT_VERSION; }
        if (wide) {
            if (wideBytes != w.size() * sizeof(RtrWideNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_build_bvh_wide: wideBytes %zu != %zu", wideBytes, w.size() * sizeof(RtrWideNode));
            memcpy(wide, w.data(), wideBytes);
        }
    }
    if (nodes) {
        if (nodeBytes != bvh.nodes.size() * sizeof(RtrBvhNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_build_bvh: nodeBytes %zu != %zu", nodeBytes, bvh.nodes.size() * sizeof(RtrBvhNode));
        memcpy(nodes, bvh.nodes.data(), nodeBytes);
    }
    if (tris) {
        if (triBytes != bvh.tris.size() * sizeof(RtrBvhTri)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_build_bvh: triBytes %zu != %zu", triBytes, bvh.tris.size() * sizeof(RtrBvhTri));
        memcpy(tris, bvh.tris.data(), triBytes);
    }
    return RTR_OK;
}

/* canonical (instance-major) primitive table + per-customIndex instance table for the device flatten kernel */
static void make_prim_tables(const rtr_scene_desc* d, const RtrInstance* instances, std::vector<rtrdev::PrimRef>& prims,
                             std::vector<rtrdev::InstanceRef>& refs) {
    prims.clear();
    refs.assign(d->numInstances, rtrdev::InstanceRef{});
    for (uint32_t i = 0; i < d->numInstances; ++i) {
        const RtrInstance& in = instances[i];
        const RtrMesh& me = d->meshes[in.meshIndex];
        rtrdev::InstanceRef& r = refs[in.customIndex];
        memcpy(r.transform, in.transform, sizeof r.transform);
        r.vertexOffset = me.vertexOffset; r.indexOffset = me.indexOffset;
        const uint32_t flags = (in.customIndex >= d->numLights && d->objects[in.customIndex - d->numLights].usesOpacityMap != 0 && me.isOpaque == 0) ? 1u : 0u;
        for (uint32_t t = 0; t < me.indexCount / 3u; ++t) prims.push_back(rtrdev::PrimRef{in.customIndex, t, flags, 0u});
    }
}

/* The host mirrors of a tree the device has (re)written, behind a join of the stream that did it: nodes, records, grid, and the
 * reduction words (`red`, handed back: [6] the largest |coordinate|, which gives boxPad, [7] the tree's depth). */
static int read_back_tree(SceneTree& t, uint32_t (&red)[8]) {
    HIP_TRY(hipMemcpy(t.hostNodes.data(), t.nodes.p, t.hostNodes.size() * sizeof(RtrBvhNode), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t.hostTris.data(), t.tris.p, t.hostTris.size() * sizeof(RtrBvhTri), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&t.stats.grid, t.grid.p, sizeof(RtrBvhGrid), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(red, t.red.p, sizeof red, hipMemcpyDeviceToHost));
    float mabs; memcpy(&mabs, &red[6], 4);
    t.stats.boxPad = (mabs > 1e-6f ? mabs : 1e-6f) * 3.814697265625e-06f;
    return RTR_OK;
}

/* The host mirrors after enqueued updates (rtr_scene_update_vertices_async and rtr_scene_update_instances_async leave them stale):
 * joins the scene's stream and reads back what the synchronous refit reads back — nodes, records, grid, boxPad — and the count of
 * reached 4-wide entries k_wide_order left on the device; after an enqueued INSTANCE update also the transforms of hostInstances (from
 * the InstanceRef table, through customIndex) and hostLights.  Every call that looks at a mirror comes through here first; it costs
 * nothing while no update has been enqueued. */
static int refresh_mirrors(const rtr_scene* cs) {
    if (!cs->mirrorsStale) return RTR_OK;
    rtr_scene* s = const_cast<rtr_scene*>(cs);
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    uint32_t red[8], reached = 0;
    { const int rc = read_back_tree(s->tree, red); if (rc != RTR_OK) return rc; }
    HIP_TRY(hipMemcpy(&reached, s->asyncWords.p + 1, sizeof reached, hipMemcpyDeviceToHost));
    s->tree.wideReached = reached; s->tree.stats.numWideNodes = reached;
    /* after an enqueued rebuild the depth is the new tree's (or, refused, still the old one's: a refit keeps it); stackEntries stays — an
     * enqueued rebuild never lowers the class, and the device refused one that would raise it */
    if (s->depthStale) { s->tree.stats.maxDepth = red[7]; s->depthStale = false; }
    if (s->instancesStale) {
        static_assert(sizeof(rtrdev::InstanceRef) == 64 && sizeof(RtrInstance) == 64, "layout");
        std::vector<rtrdev::InstanceRef> refs(s->hostInstances.size());
        if (!refs.empty()) HIP_TRY(hipMemcpy(refs.data(), s->tree.instRefs.p, refs.size() * sizeof(rtrdev::InstanceRef), hipMemcpyDeviceToHost));
        for (RtrInstance& in : s->hostInstances) memcpy(in.transform, refs[in.customIndex].transform, sizeof in.transform);
        if (s->numLights) HIP_TRY(hipMemcpy(s->hostLights.data(), s->lights.p, s->numLights * sizeof(RtrAreaLightInfo), hipMemcpyDeviceToHost));
        s->instancesStale = false;
    }
    s->mirrorsStale = false;
    return RTR_OK;
}

/* (re)computes the per-light-triangle records light_loops reads; the light transforms live in s->lights on the device */
static int make_light_tris(rtr_scene* s) {
    if (s->numLights == 0) return RTR_OK;
    hipError_t e = rtrdev::launch_light_tris(s->lights.p, s->vertices.p, s->indices.p, s->lightTriFirst.p, s->numLights, s->lightTris.p, s->ctx->stream);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "light-triangle records: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));     /* frames of other contexts may render this scene next */
    return RTR_OK;
}

/* computes the per-object material terms fetch_surface reads, on the device, from s->objects */
static int make_object_terms(rtr_scene* s) {
    if (s->numObjects == 0) return RTR_OK;
    HIP_TRY(s->objectTerms.alloc((size_t)s->numObjects * rtrdev::kObjectTermsRecord));
    hipError_t e = rtrdev::launch_object_terms(s->objects.p, s->numObjects, s->objectTerms.p, s->ctx->stream);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "object terms: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));     /* frames of other contexts may render this scene next */
    return RTR_OK;
}

/* (re)builds the 4-wide view of the tree the any-hit kernel walks, on the device, from the quantised BVH2 nodes */
static int make_wide_nodes(SceneTree& t, hipStream_t st) {
    const uint32_t n = (uint32_t)t.hostNodes.size();
    if (!t.nodes4.p) { HIP_TRY(t.nodes4.alloc((size_t)n * 4)); HIP_TRY(t.nodes4tmp.alloc((size_t)n * 4)); HIP_TRY(t.wideRemap.alloc(n)); HIP_TRY(t.wideSums.alloc(rtrdev::bvh_wide_scratch_words())); }
    if (!t.hostWideShape.empty() && !t.wideShape.p) HIP_TRY(t.wideShape.upload(t.hostWideShape.data(), t.hostWideShape.size(), st));
    hipError_t e = rtrdev::bvh_make_wide(t.nodes.p, n, t.refitReady ? t.parent.p : nullptr, t.grid.p, t.hostWideShape.size() == n ? t.wideShape.p : nullptr, t.nodes4tmp.p, t.wideSums.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "4-wide node build: %s", hipGetErrorString(e));
    /* breadth-first order of the 4-wide tree (child codes = the 4th 16 bytes of every entry), so its top levels are the first
     * entries: k_shadow_trace4 keeps those in LDS.  Entries the 4-wide tree does not reach keep the ids after them. */
    std::vector<uint32_t> codes((size_t)n * 4), remap(n, 0xffffffffu), order;
    HIP_TRY(hipMemcpy2DAsync(codes.data(), 16, reinterpret_cast<const char*>(t.nodes4tmp.p) + 48, 64, 16, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    order.reserve(n);
    order.push_back(0); remap[0] = 0;
    for (size_t head = 0; head < order.size(); ++head)
        for (int k = 0; k < 4; ++k) {
            const int32_t c = (int32_t)codes[(size_t)order[head] * 4 + k];
            if (c >= 0 && (uint32_t)c < n && remap[c] == 0xffffffffu) { remap[c] = (uint32_t)order.size(); order.push_back((uint32_t)c); }
        }
    uint32_t next = (uint32_t)order.size();
    for (uint32_t i = 0; i < n; ++i) if (remap[i] == 0xffffffffu) remap[i] = next++;
    HIP_TRY(hipMemcpyAsync(t.wideRemap.p, remap.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    e = rtrdev::bvh_permute_wide(t.nodes4tmp.p, n, t.wideRemap.p, t.nodes4.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "4-wide node order: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    t.wideReached = (uint32_t)order.size();
    HIP_TRY(hipMemcpy(&t.stats.grid, t.grid.p, sizeof(RtrBvhGrid), hipMemcpyDeviceToHost));     /* the wide centre was set on the device */
    t.stats.numWideNodes = t.wideReached; t.stats.wideLayoutVersion = RTR_WIDE_LAYOUT_VERSION;
    return RTR_OK;
}

static rtrdev::BvhDeviceArrays device_arrays(SceneTree& t) {
    rtrdev::BvhDeviceArrays a{};
    a.nodes = t.nodes.p; a.nodesF = t.nodesF.p; a.grid = t.grid.p; a.tris = t.tris.p; a.boxMin = t.boxMin.p; a.boxMax = t.boxMax.p; a.parent = t.parent.p;
    a.counters = t.counters.p; a.depth = t.depth.p; a.slotOfPrim = t.slotOfPrim.p; a.red = t.red.p;
    return a;
}

/* the build scratch for n triangles, allocated on first use and kept */
static int ensure_build_scratch(BuildScratch& bs, uint32_t n) {
    const uint32_t numNodes = n - 1;
    HIP_TRY(bs.trisCanon.ensure((size_t)n * 3)); HIP_TRY(bs.minCanon.ensure(n)); HIP_TRY(bs.maxCanon.ensure(n));
    HIP_TRY(bs.keysIn.ensure(n)); HIP_TRY(bs.keysOut.ensure(n)); HIP_TRY(bs.range.ensure(numNodes)); HIP_TRY(bs.rawChild.ensure(numNodes));
    bs.sortTempBytes = rtrdev::bvh_sort_temp_bytes(n);
    HIP_TRY(bs.sortTemp.ensure(bs.sortTempBytes));
    return RTR_OK;
}
static rtrdev::BvhScratch scratch_view(const BuildScratch& bs) {
    rtrdev::BvhScratch sc{};
    sc.trisCanon = bs.trisCanon.p; sc.minCanon = bs.minCanon.p; sc.maxCanon = bs.maxCanon.p; sc.keysIn = bs.keysIn.p; sc.keysOut = bs.keysOut.p;
    sc.range = bs.range.p; sc.rawChild = bs.rawChild.p; sc.sortTemp = bs.sortTemp.p; sc.sortTempBytes = bs.sortTempBytes;
    return sc;
}

/* Device LBVH build into t.nodes / t.tris (+ refit arrays) from the primitive tables and the DEVICE vertex / index arrays given;
 * fills hostNodes/hostTris and the stats.  The core rtr_scene_create (build_on_device) and rtr_scene_rebuild share: `t` is the fresh
 * tree that is built, `bs` the scratch (the caller's to keep or free). */
static int build_on_device_core(SceneTree& t, hipStream_t st, const std::vector<rtrdev::PrimRef>& prims, const std::vector<rtrdev::InstanceRef>& refs,
                                const RtrVertex* vertices, const uint32_t* indices, BuildScratch& bs, size_t numPrims) {
    const uint32_t n = (uint32_t)numPrims, numNodes = n - 1;
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(t.prims.upload(prims.data(), prims.size(), st));
    HIP_TRY(t.instRefs.upload(refs.data(), refs.size(), st));
    HIP_TRY(t.nodes.alloc((size_t)numNodes * 2)); HIP_TRY(t.nodesF.alloc((size_t)numNodes * 4)); HIP_TRY(t.grid.alloc(1));
    HIP_TRY(t.tris.alloc((size_t)n * 3));
    HIP_TRY(t.boxMin.alloc(n)); HIP_TRY(t.boxMax.alloc(n)); HIP_TRY(t.parent.alloc(numNodes));
    HIP_TRY(t.counters.alloc(numNodes)); HIP_TRY(t.depth.alloc(numNodes)); HIP_TRY(t.slotOfPrim.alloc(n)); HIP_TRY(t.red.alloc(8));
    { const int rcs = ensure_build_scratch(bs, n); if (rcs != RTR_OK) return rcs; }
    const rtrdev::BvhScratch sc = scratch_view(bs);
    HIP_TRY(hipMemsetAsync(t.nodesF.p, 0, (size_t)numNodes * 64, st));
    rtrdev::BvhInputs in{t.prims.p, t.instRefs.p, vertices, indices};
    hipError_t e = rtrdev::bvh_build_lbvh(in, n, device_arrays(t), sc, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "device BVH build: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    t.hostNodes.resize(numNodes); t.hostTris.resize(n);
    memset(&t.stats, 0, sizeof t.stats);
    uint32_t red[8];
    { const int rc = read_back_tree(t, red); if (rc != RTR_OK) return rc; }
    const float buildMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (red[7] > 64) return fail(RTR_ERR_BVH_TOO_DEEP, "device-built BVH depth %u exceeds the 64-entry LDS traversal stack", red[7]);
    t.stats.numTriangles = n; t.stats.numNodes = numNodes; t.stats.maxDepth = red[7]; t.stats.maxLeafSize = 4;
    t.stats.bvhLayoutVersion = RTR_BVH_LAYOUT_VERSION;
    t.stats.stackEntries = red[7] <= 16 ? 16 : (red[7] <= 32 ? 32 : 64);
    t.stats.buildMs = buildMs;
    t.numPrims = n; t.numNodeSlots = numNodes; t.refitReady = true;
    return RTR_OK;
}

/* rtr_scene_create's device build: the tables from the description, the vertices it uploaded; the scratch goes with the call */
static int build_on_device(rtr_scene* s, const rtr_scene_desc* d, size_t numPrims) {
    std::vector<rtrdev::PrimRef> prims; std::vector<rtrdev::InstanceRef> refs;
    make_prim_tables(d, d->instances, prims, refs);
    for (uint32_t v = 0; v < d->numVertices; ++v)
        for (int k = 0; k < 3; ++k)
            if (!(d->vertices[v].position[k] > -3.0e38f && d->vertices[v].position[k] < 3.0e38f))
                return fail(RTR_ERR_INVALID_ARGUMENT, "BVH build: non-finite vertex position in vertex %u", v);
    BuildScratch scratch;
    return build_on_device_core(s->tree, s->ctx->stream, prims, refs, s->vertices.p, s->indices.p, scratch, numPrims);
}

/* DeviceScene's view of the tree: what the kernels walk */
static void point_at_tree(DeviceScene& dv, const SceneTree& t) {
    dv.nodes = t.nodes.p; dv.nodes4 = t.nodes4.p; dv.numNodes4 = (uint32_t)t.hostNodes.size(); dv.grid = t.grid.p; dv.tris = t.tris.p;
}

static int scene_create_impl(rtr_ctx* ctx, const rtr_scene_desc* d, const rtr_scene* like, rtr_scene** out) {
    if (!ctx || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create: null ctx/out");
    if (ctx->destroyed) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create: the context has been destroyed");
    *out = nullptr;
    int rc = validate_desc(d);
    if (rc != RTR_OK) return rc;
    if (d->buildFlags > RTR_BUILD_DEVICE_LBVH) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create: unknown buildFlags %u", d->buildFlags);
    HIP_TRY(hipSetDevice(ctx->device));
    size_t totalPrims = 0;
    for (uint32_t i = 0; i < d->numInstances; ++i) totalPrims += d->meshes[d->instances[i].meshIndex].indexCount / 3u;
    /* every triangle may end up in a leaf of its own: numTriangles - 1 inner nodes, hence as many 4-wide records at most */
    rc = rtr_check_scene_limits(totalPrims, totalPrims ? totalPrims - 1 : 0);
    if (rc != RTR_OK) return rc;
    /* tiny scenes always take the host builder (the radix tree needs a root with more than one leaf's worth of primitives) */
    const bool deviceBuild = !like && d->buildFlags == RTR_BUILD_DEVICE_LBVH && totalPrims >= 16;
    rtr::BvhResult bvh; std::vector<float> xforms, nmats; uint32_t stackEntries = 0; size_t numTris = 0;
    if (like) {
        rc = refresh_mirrors(like);
        if (rc != RTR_OK) return rc;
        /* the tree of `like`, as its host copy holds it (nodes and records are kept in step with the device by every update) */
        const SceneTree& lt = like->tree;
        if (lt.stats.numTriangles != totalPrims || lt.hostNodes.empty() || lt.hostTris.empty())
            return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create_like: the built scene has %u triangles, this description %zu", lt.stats.numTriangles, totalPrims);
        bvh.nodes = lt.hostNodes; bvh.tris = lt.hostTris; bvh.grid = lt.stats.grid; bvh.wideShape = lt.hostWideShape;
        if (!like->hostMasks.empty()) for (RtrBvhTri& t : bvh.tris) t.flags &= ~RTR_TRI_MASK_BITS;      /* a new scene's instance masks are 0xff, whatever `like` has set */
        bvh.maxDepth = lt.stats.maxDepth; bvh.maxLeafSize = lt.stats.maxLeafSize; bvh.sahCost = lt.stats.sahCost; bvh.boxPad = lt.stats.boxPad;
        for (int k = 0; k < 3; ++k) { bvh.boundsMin[k] = lt.stats.boundsMin[k]; bvh.boundsMax[k] = lt.stats.boundsMax[k]; }
        bvh.buildMs = 0.f;                                   /* nothing was built here */
        stackEntries = lt.stats.stackEntries; numTris = lt.stats.numTriangles;
        instance_tables(d->numInstances, d->instances, xforms, nmats);
    } else if (!deviceBuild) {
        rc = flatten_and_build(d, bvh, xforms, nmats, &stackEntries, &numTris);
        if (rc != RTR_OK) return rc;
    } else {
        instance_tables(d->numInstances, d->instances, xforms, nmats);
    }

    rtr_scene* s = new rtr_scene();
    s->ctx = ctx; ++ctx->children;
    SceneTree& tree = s->tree;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    static_assert(sizeof(RtrBvhNode) == 2 * sizeof(uint4) && sizeof(RtrBvhTri) == 3 * sizeof(float4), "layout");
    if (!deviceBuild) {
        chk(tree.nodes.upload(reinterpret_cast<const uint4*>(bvh.nodes.data()), bvh.nodes.size() * 2, st));
        chk(tree.grid.upload(&bvh.grid, 1, st));
        chk(tree.tris.upload(reinterpret_cast<const float4*>(bvh.tris.data()), bvh.tris.size() * 3, st));
    }
    chk(s->vertices.upload(d->vertices, d->numVertices, st));
    chk(s->indices.upload(d->indices, d->numIndices, st));
    chk(s->objects.upload(d->objects, d->numObjects, st));
    chk(s->lights.upload(d->lights, d->numLights, st));
    {
        std::vector<uint32_t> first(d->numLights);
        uint32_t total = 0;
        for (uint32_t l = 0; l < d->numLights; ++l) { first[l] = total; total += d->lights[l].numTriangles; }
        chk(s->lightTriFirst.upload(first.data(), first.size(), st));
        chk(s->lightTris.alloc((size_t)total * rtrdev::kLightTriRecord));
        /* what a hit's primitiveId may be, per customIndex: a light's records or its instance's mesh triangles */
        std::vector<uint32_t> count(d->numInstances);
        for (uint32_t i = 0; i < d->numInstances; ++i) {
            const RtrInstance& in = d->instances[i];
            count[in.customIndex] = in.customIndex < d->numLights ? d->lights[in.customIndex].numTriangles : d->meshes[in.meshIndex].indexCount / 3u;
        }
        chk(s->triCount.upload(count.data(), count.size(), st));
        s->hostTriCount.swap(count);
    }
    chk(s->xforms.upload(xforms.data(), xforms.size(), st));
    chk(s->nmats.upload(nmats.data(), nmats.size(), st));
    if (d->ltc1) {
        chk(s->ltc1.upload(d->ltc1, 64 * 64 * 4, st));
        chk(s->ltc2.upload(d->ltc2, 64 * 64 * 4, st));
        s->hasLtc = true;
    }
    std::vector<rtrdev::DeviceTexture> table(d->numTextures);
    s->texPixels.resize(d->numTextures);
    for (uint32_t t = 0; t < d->numTextures; ++t) {
        const rtr_texture& tx = d->textures[t];
        table[t] = rtrdev::DeviceTexture{nullptr, 0, 0, 0, 0};
        if (!tx.pixels) continue;
        chk(s->texPixels[t].upload(tx.pixels, (size_t)tx.width * tx.height * tx.channels, st));
        table[t] = rtrdev::DeviceTexture{s->texPixels[t].p, tx.width, tx.height, tx.channels, 0};
    }
    chk(s->texTable.upload(table.data(), table.size(), st));
    rtrdev::DeviceTexture hdri{nullptr, 0, 0, 0, 0};
    if (d->hdri) {
        chk(s->hdriPixels.upload(d->hdri->pixels, (size_t)d->hdri->width * d->hdri->height * d->hdri->channels, st));
        hdri = rtrdev::DeviceTexture{s->hdriPixels.p, d->hdri->width, d->hdri->height, d->hdri->channels, 0};
    }
    if (e != hipSuccess) {
        delete s; ctx_release_child(ctx);
        return fail(e == hipErrorOutOfMemory ? RTR_ERR_OUT_OF_MEMORY : RTR_ERR_HIP, "scene upload: %s", hipGetErrorString(e));
    }
    s->numLights = d->numLights; s->numObjects = d->numObjects; s->numInstances = d->numInstances; s->numVertices = d->numVertices; s->numIndices = d->numIndices;
    if (d->numLights) s->hostLights.assign(d->lights, d->lights + d->numLights);
    if (d->numInstances) s->hostInstances.assign(d->instances, d->instances + d->numInstances);
    if (d->numMeshes) s->hostMeshes.assign(d->meshes, d->meshes + d->numMeshes);
    if (d->numObjects) s->hostObjects.assign(d->objects, d->objects + d->numObjects);
    if (deviceBuild) {
        rc = build_on_device(s, d, totalPrims);
        if (rc != RTR_OK) { delete s; ctx_release_child(ctx); return rc; }
    } else {
        fill_stats(tree.stats, bvh, stackEntries, numTris);
        tree.hostNodes.swap(bvh.nodes);
        tree.hostTris.swap(bvh.tris);
        tree.hostWideShape.swap(bvh.wideShape);
        tree.numPrims = (uint32_t)tree.hostTris.size(); tree.numNodeSlots = (uint32_t)tree.hostNodes.size();
    }

    rc = make_wide_nodes(tree, st);
    if (rc == RTR_OK) rc = make_light_tris(s);
    if (rc == RTR_OK) rc = make_object_terms(s);
    if (rc != RTR_OK) { delete s; ctx_release_child(ctx); return rc; }
    DeviceScene& dv = s->dev;
    point_at_tree(dv, tree);
    dv.vertices = s->vertices.p; dv.indices = s->indices.p;
    dv.objects = s->objects.p; dv.objectTerms = s->objectTerms.p; dv.lights = s->lights.p;
    dv.lightTris = s->lightTris.p; dv.lightTriFirst = s->lightTriFirst.p;
    dv.xforms = s->xforms.p; dv.nmats = s->nmats.p;
    dv.ltc1 = s->hasLtc ? s->ltc1.p : nullptr; dv.ltc2 = s->hasLtc ? s->ltc2.p : nullptr;
    for (int k = 0; k < 3; ++k) dv.skyLinear[k] = rtr_to_linear(d->skyColor[k]);
    dv.numLights = d->numLights;
    dv.numLightTris = 0;
    for (uint32_t l = 0; l < d->numLights; ++l) dv.numLightTris += d->lights[l].numTriangles;
    dv.textures = s->texTable.p;
    dv.hdri = hdri;
    *out = s;
    return RTR_OK;
}

int rtr_scene_create(rtr_ctx* ctx, const rtr_scene_desc* d, rtr_scene** out) { return scene_create_impl(ctx, d, nullptr, out); }

int rtr_scene_create_like(rtr_ctx* ctx, const rtr_scene_desc* d, const rtr_scene* built, rtr_scene** out) {
    if (!built) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_create_like: null scene to copy the tree from");
    return scene_create_impl(ctx, d, built, out);
}

/* parent links of a node array, as the refit keeps them: (parentIndex << 1) | slot, -1 for the root, -2 for a slot the root does not
 * reach; returns how many slots it reaches */
static size_t host_parent_array(const std::vector<RtrBvhNode>& nodes, std::vector<int32_t>& parent) {
    parent.assign(nodes.size(), -2);
    if (nodes.empty()) return 0;
    parent[0] = -1;
    size_t reached = 1;
    std::vector<uint32_t> stack{0};
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        for (int sl = 0; sl < 2; ++sl) {
            const int32_t c = nodes[i].child[sl];
            if (c >= 0 && parent[(size_t)c] == -2) { parent[(size_t)c] = (int32_t)((i << 1) | (uint32_t)sl); stack.push_back((uint32_t)c); ++reached; }
        }
    }
    return reached;
}

/* A host-built tree gets its refit arrays on the first update: parent links from the node array, the
 * canonical-primitive -> leaf-slot map from the ids stored in the triangle records. */
static int ensure_refit_ready(rtr_scene* s) {
    SceneTree& t = s->tree;
    if (t.refitReady) return RTR_OK;
    if (s->hostInstances.empty()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_instances: the scene has no instances");
    hipStream_t st = s->ctx->stream;
    const uint32_t numNodes = (uint32_t)t.hostNodes.size(), n = (uint32_t)t.hostTris.size();
    std::vector<int32_t> parent;
    host_parent_array(t.hostNodes, parent);
    /* canonical order = instances in creation order, primitives in mesh order */
    std::vector<uint32_t> base(s->hostInstances.size(), 0);       /* by customIndex */
    uint32_t acc = 0;
    for (const RtrInstance& in : s->hostInstances) { base[in.customIndex] = acc; acc += s->hostMeshes[in.meshIndex].indexCount / 3u; }
    if (acc != n) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_instances: scene has no geometry to refit");
    std::vector<uint32_t> slotOfPrim(n, 0);
    for (uint32_t slot = 0; slot < n; ++slot) slotOfPrim[base[t.hostTris[slot].customIndex] + t.hostTris[slot].primitiveId] = slot;
    /* the fit works on fp32 planes: child codes from the host tree, boxes recomputed by the refit */
    std::vector<rtr::BvhNodeF> nf(numNodes);
    for (uint32_t i = 0; i < numNodes; ++i) {
        memset(&nf[i], 0, sizeof nf[i]);
        nf[i].child[0] = t.hostNodes[i].child[0]; nf[i].child[1] = t.hostNodes[i].child[1];
    }
    HIP_TRY(t.nodesF.upload(reinterpret_cast<const float4*>(nf.data()), (size_t)numNodes * 4, st));
    HIP_TRY(t.parent.upload(parent.data(), parent.size(), st));
    HIP_TRY(t.slotOfPrim.upload(slotOfPrim.data(), slotOfPrim.size(), st));
    HIP_TRY(t.boxMin.alloc(n)); HIP_TRY(t.boxMax.alloc(n));
    HIP_TRY(t.counters.alloc(numNodes)); HIP_TRY(t.depth.alloc(numNodes)); HIP_TRY(t.red.alloc(8));
    t.numPrims = n; t.numNodeSlots = numNodes; t.refitReady = true;
    return RTR_OK;
}

/* per customIndex: the complement of the instance's mask where the records keep it (RtrBvhTri::flags, RTR_TRI_MASK_SHIFT) */
static std::vector<uint32_t> instance_mask_bits(const rtr_scene* s, const uint8_t* masks) {
    std::vector<uint32_t> bits(s->hostInstances.size(), 0u);
    for (size_t i = 0; i < s->hostInstances.size(); ++i) bits[s->hostInstances[i].customIndex] = ((uint32_t)(uint8_t)~masks[i]) << RTR_TRI_MASK_SHIFT;
    return bits;
}

/* the description a scene's host mirrors make (no vertices, no indices: the device holds those) */
static rtr_scene_desc host_view(const rtr_scene* s) {
    rtr_scene_desc view{};
    view.meshes = s->hostMeshes.data(); view.numMeshes = (uint32_t)s->hostMeshes.size();
    view.instances = s->hostInstances.data(); view.numInstances = (uint32_t)s->hostInstances.size();
    view.objects = s->hostObjects.data(); view.numObjects = (uint32_t)s->hostObjects.size();
    view.lights = s->hostLights.data(); view.numLights = s->numLights;
    return view;
}

/* the tables a refit or a device build flattens from (PrimRef / InstanceRef) for the transforms given, with the instance masks in the
 * flags: both write the records from this table */
static void scene_prim_tables(const rtr_scene* s, const RtrInstance* inst, std::vector<rtrdev::PrimRef>& prims, std::vector<rtrdev::InstanceRef>& refs) {
    const rtr_scene_desc view = host_view(s);
    make_prim_tables(&view, inst, prims, refs);
    if (s->hostMasks.empty()) return;
    const std::vector<uint32_t> bits = instance_mask_bits(s, s->hostMasks.data());
    for (rtrdev::PrimRef& pr : prims) pr.flags |= bits[pr.customIndex];
}

/* those tables on the device, for the scene's tree */
static int upload_prim_tables(rtr_scene* s, const RtrInstance* inst) {
    std::vector<rtrdev::PrimRef> prims; std::vector<rtrdev::InstanceRef> refs;
    scene_prim_tables(s, inst, prims, refs);
    HIP_TRY(s->tree.prims.upload(prims.data(), prims.size(), s->ctx->stream));
    HIP_TRY(s->tree.instRefs.upload(refs.data(), refs.size(), s->ctx->stream));
    return RTR_OK;
}

int rtr_scene_set_instance_masks(rtr_scene* s, const uint8_t* masks, uint32_t numInstances) {
    if (!s || (!masks && numInstances)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_set_instance_masks: null argument");
    if (numInstances != s->hostInstances.size()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_set_instance_masks: %u masks given, scene has %zu instances", numInstances, s->hostInstances.size());
    if (numInstances == 0) return RTR_OK;
    const std::vector<uint32_t> bits = instance_mask_bits(s, masks);
    HIP_TRY(hipSetDevice(s->ctx->device));
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    /* queries of OTHER contexts (other streams) may be walking these records: everything enqueued on the device so far is joined before
     * they are rewritten (contract in rtr.h, as rtr_scene_update_instances) */
    HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s->ctx->stream;
    const uint32_t numTris = (uint32_t)(s->tree.tris.n / 3);
    HIP_TRY(s->maskBits.upload(bits.data(), bits.size(), st));
    const hipError_t e = rtrdev::launch_set_instance_masks(s->tree.tris.p, numTris, s->maskBits.p, numInstances, st);
    if (const int rc = launched(e, "rtr_scene_set_instance_masks")) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    /* the host mirror (rtr_scene_export_bvh, rtr_scene_create_like) in step: the same rule as the kernel's */
    for (RtrBvhTri& t : s->tree.hostTris)
        if (t.customIndex < numInstances) t.flags = (t.flags & ~RTR_TRI_MASK_BITS) | bits[t.customIndex];
    s->hostMasks.assign(masks, masks + numInstances);
    /* an enqueued refit writes its records from the device tables: they carry the new masks from here on */
    if (s->tree.asyncReady) return upload_prim_tables(s, s->hostInstances.data());
    return RTR_OK;
}

int rtr_scene_get_instance_masks(const rtr_scene* s, uint8_t* masks, uint32_t numInstances) {
    if (!s || (!masks && numInstances)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_get_instance_masks: null argument");
    if (numInstances != s->hostInstances.size()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_get_instance_masks: room for %u masks, scene has %zu instances", numInstances, s->hostInstances.size());
    for (uint32_t i = 0; i < numInstances; ++i) masks[i] = s->hostMasks.empty() ? 0xffu : s->hostMasks[i];
    return RTR_OK;
}

/* The argument checks the two refitting calls share (rtr_scene_update_instances, rtr_scene_update_vertices); `who` names the caller in
 * the message.  instances == NULL (rtr_scene_update_vertices only): the current transforms are kept and nothing is checked for them. */
static int check_refit_args(const rtr_scene* s, const RtrInstance* instances, uint32_t numInstances, const RtrAreaLightInfo* lights, uint32_t numLights,
                            const char* who) {
    if (instances) {
        if (numInstances != s->hostInstances.size()) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %u instances given, scene has %zu", who, numInstances, s->hostInstances.size());
        for (uint32_t i = 0; i < numInstances; ++i) {
            if (instances[i].meshIndex != s->hostInstances[i].meshIndex || instances[i].customIndex != s->hostInstances[i].customIndex)
                return fail(RTR_ERR_INVALID_ARGUMENT, "%s: instance %u changed mesh or customIndex; only transforms may change (a refit keeps the topology)", who, i);
            for (int k = 0; k < 12; ++k)
                if (!(instances[i].transform[k] > -3.0e38f && instances[i].transform[k] < 3.0e38f))
                    return fail(RTR_ERR_INVALID_ARGUMENT, "%s: instance %u has a non-finite transform", who, i);
        }
    }
    if (lights) {
        if (numLights != s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %u lights given, scene has %u", who, numLights, s->numLights);
        for (uint32_t l = 0; l < numLights; ++l)
            if (lights[l].vertexOffset != s->hostLights[l].vertexOffset || lights[l].indexOffset != s->hostLights[l].indexOffset ||
                lights[l].numTriangles != s->hostLights[l].numTriangles)
                return fail(RTR_ERR_INVALID_ARGUMENT, "%s: light %u changed its mesh", who, l);
    }
    return RTR_OK;
}

/* The refit both calls end in, on a scene that is refit-ready and a device that has been joined: world-space records from the device
 * vertex array, boxes, grid, 4-wide view, host mirrors, boxPad.  instances == NULL keeps the current transforms (and with them the
 * transform, normal-matrix and mirrored tables); lights == NULL keeps the light infos.  lightTris: remake the light-triangle table even
 * when no lights are given (the vertices of a light's mesh may have changed). */
static int refit_scene(rtr_scene* s, const RtrInstance* instances, const RtrAreaLightInfo* lights, bool lightTris) {
    hipStream_t st = s->ctx->stream;
    const uint32_t numInstances = (uint32_t)s->hostInstances.size(), numLights = s->numLights;
    { const int rct = upload_prim_tables(s, instances ? instances : s->hostInstances.data()); if (rct != RTR_OK) return rct; }
    std::vector<float> xforms, nmats;      /* outlive the asynchronous copies: the stream is joined below */
    if (instances) {
        instance_tables(numInstances, instances, xforms, nmats);
        HIP_TRY(hipMemcpyAsync(s->xforms.p, xforms.data(), xforms.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->nmats.p, nmats.data(), nmats.size() * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (lights && numLights) HIP_TRY(hipMemcpyAsync(s->lights.p, lights, numLights * sizeof(RtrAreaLightInfo), hipMemcpyHostToDevice, st));
    SceneTree& t = s->tree;
    rtrdev::BvhInputs in{t.prims.p, t.instRefs.p, s->vertices.p, s->indices.p};
    hipError_t e = rtrdev::bvh_refit(in, t.numPrims, t.numNodeSlots, device_arrays(t), st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "device BVH refit: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    /* keep the host mirror (rtr_scene_export_bvh) and the stats in step */
    uint32_t red[8];
    { const int rcb = read_back_tree(t, red); if (rcb != RTR_OK) return rcb; }
    { const int rc4 = make_wide_nodes(t, st); if (rc4 != RTR_OK) return rc4; }
    if (lightTris || (lights && numLights)) { const int rcl = make_light_tris(s); if (rcl != RTR_OK) return rcl; }
    if (instances) s->hostInstances.assign(instances, instances + numInstances);
    if (lights && numLights) s->hostLights.assign(lights, lights + numLights);
    return RTR_OK;
}

int rtr_scene_update_instances(rtr_scene* s, const RtrInstance* instances, uint32_t numInstances, const RtrAreaLightInfo* lights, uint32_t numLights) {
    if (!s || (!instances && numInstances)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_instances: null argument");
    if (numInstances != s->hostInstances.size()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_instances: %u instances given, scene has %zu", numInstances, s->hostInstances.size());
    int rc = check_refit_args(s, instances, numInstances, lights, numLights, "rtr_scene_update_instances");
    if (rc != RTR_OK) return rc;
    rc = refresh_mirrors(s);
    if (rc != RTR_OK) return rc;
    if (scene_is_empty(s)) return RTR_OK;     /* nothing to refit */
    HIP_TRY(hipSetDevice(s->ctx->device));
    rc = ensure_refit_ready(s);
    if (rc != RTR_OK) return rc;
    /* frames of OTHER contexts (other streams) may be rendering this scene: everything enqueued on the device so far is joined
     * before the nodes, records and light tables are rewritten (contract in rtr.h) */
    HIP_TRY(hipDeviceSynchronize());
    return refit_scene(s, instances, lights, false);
}

/* The checks of the ranges that the synchronous and the enqueued vertex update share, with the same messages (`who` names the caller):
 * strides, ranges inside the vertex array, null positions, device-pointer alignment, overlaps. */
static int check_vertex_ranges(const rtr_scene* s, const rtr_vertex_range* ranges, uint32_t numRanges, uint32_t positionStride, uint32_t normalStride,
                               bool device, const char* who) {
    if ((positionStride & 3u) || positionStride < 12u) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: positionStride %u must be a multiple of 4 and at least 12", who, positionStride);
    bool anyNormals = false;
    for (uint32_t r = 0; r < numRanges; ++r) {
        const rtr_vertex_range& vr = ranges[r];
        if ((uint64_t)vr.firstVertex + vr.numVertices > s->numVertices)
            return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u (vertices %u .. %llu) leaves the scene's %u vertices", who, r, vr.firstVertex,
                        (unsigned long long)vr.firstVertex + vr.numVertices, s->numVertices);
        if (vr.numVertices && !vr.positions) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u has %u vertices and null positions", who, r, vr.numVertices);
        if (device && ((((uintptr_t)vr.positions) | ((uintptr_t)vr.normals)) & 3u))
            return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u: device pointers must be 4-byte aligned", who, r);
        anyNormals = anyNormals || (vr.normals && vr.numVertices);
    }
    if (anyNormals && ((normalStride & 3u) || normalStride < 12u)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: normalStride %u must be a multiple of 4 and at least 12", who, normalStride);
    {   /* no two ranges may name a vertex twice: the result would depend on the order the lanes run in */
        std::vector<uint32_t> order;
        for (uint32_t r = 0; r < numRanges; ++r) if (ranges[r].numVertices) order.push_back(r);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ranges[a].firstVertex < ranges[b].firstVertex; });
        for (size_t k = 1; k < order.size(); ++k) {
            const rtr_vertex_range& a = ranges[order[k - 1]]; const rtr_vertex_range& b = ranges[order[k]];
            if ((uint64_t)a.firstVertex + a.numVertices > b.firstVertex)
                return fail(RTR_ERR_INVALID_ARGUMENT, "%s: ranges %u and %u overlap (vertex %u)", who, order[k - 1], order[k], b.firstVertex);
        }
    }
    return RTR_OK;
}

int rtr_scene_update_vertices(rtr_scene* s, const rtr_vertex_range* ranges, uint32_t numRanges, uint32_t positionStride, uint32_t normalStride, uint32_t flags,
                              const RtrInstance* instances, uint32_t numInstances, const RtrAreaLightInfo* lights, uint32_t numLights) {
    static const char* who = "rtr_scene_update_vertices";
    static_assert(sizeof(rtr_vertex_range) == 24, "layout");
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (!ranges || numRanges == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null ranges (or numRanges == 0): nothing to update", who);
    if (flags > RTR_VERTICES_DEVICE) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", who, flags & ~RTR_VERTICES_DEVICE);
    const bool device = flags == RTR_VERTICES_DEVICE;
    int rc = check_vertex_ranges(s, ranges, numRanges, positionStride, normalStride, device, who);
    if (rc != RTR_OK) return rc;
    rc = check_refit_args(s, instances, numInstances, lights, numLights, who);
    if (rc != RTR_OK) return rc;
    rc = refresh_mirrors(s);
    if (rc != RTR_OK) return rc;
    if (scene_is_empty(s)) return RTR_OK;     /* nothing to refit */

    /* the device tables of the launches: the ranges in chunks of kVertexRangesPerLaunch, each with its own prefix counts */
    const uint32_t kChunk = rtrdev::kVertexRangesPerLaunch;
    const uint32_t numChunks = (numRanges + kChunk - 1) / kChunk;
    std::vector<rtrdev::VertexRange> table(numRanges);
    std::vector<uint32_t> prefix((size_t)numRanges + numChunks), chunkBase(numChunks + 1, 0u);
    for (uint32_t c = 0; c < numChunks; ++c) {
        uint32_t acc = 0;
        const uint32_t r0 = c * kChunk, r1 = std::min(numRanges, r0 + kChunk);
        for (uint32_t r = r0; r < r1; ++r) { prefix[(size_t)r + c] = acc; acc += ranges[r].numVertices; }      /* non-overlapping ranges inside a 32-bit array: no wrap */
        prefix[(size_t)r1 + c] = acc;
        chunkBase[c + 1] = chunkBase[c] + acc;
    }
    auto name_bad = [&](uint64_t concat, uint32_t* range, uint32_t* vertex) {      /* concatenated index -> (range, vertex in it) */
        uint32_t r = 0; uint64_t before = 0;
        while (before + ranges[r].numVertices <= concat) before += ranges[r++].numVertices;
        *range = r; *vertex = (uint32_t)(concat - before);
    };

    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const uint32_t posWords = device ? positionStride / 4u : 3u, nrmWords = device ? normalStride / 4u : 3u;
    if (!device) {
        /* host data: checked here, then packed (three words per vertex: all positions, then the normals of the ranges that bring them)
         * and staged in a device buffer of the scene, from where it takes the path of device data */
        size_t words = 0;
        for (uint32_t r = 0; r < numRanges; ++r) words += (size_t)ranges[r].numVertices * (ranges[r].normals ? 6u : 3u);
        s->vtxHost.resize(words);
        size_t at = 0;
        for (uint32_t r = 0; r < numRanges; ++r) {
            const char* src = static_cast<const char*>(ranges[r].positions);
            for (uint32_t v = 0; v < ranges[r].numVertices; ++v, at += 3) {
                float p[3];
                memcpy(p, src + (size_t)v * positionStride, sizeof p);
                for (int k = 0; k < 3; ++k)
                    if (!(p[k] > -3.0e38f && p[k] < 3.0e38f))
                        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u, vertex %u (scene vertex %u): non-finite position", who, r, v, ranges[r].firstVertex + v);
                memcpy(&s->vtxHost[at], p, sizeof p);
            }
        }
        HIP_TRY(s->vtxStage.grow(words));
        size_t pos = 0;
        for (uint32_t r = 0; r < numRanges; ++r) {
            table[r] = rtrdev::VertexRange{s->vtxStage.p + pos, nullptr, ranges[r].firstVertex, 0u};
            pos += (size_t)ranges[r].numVertices * 3u;
        }
        for (uint32_t r = 0; r < numRanges; ++r) {
            if (!ranges[r].normals || !ranges[r].numVertices) continue;
            const char* src = static_cast<const char*>(ranges[r].normals);
            table[r].normals = s->vtxStage.p + at;
            for (uint32_t v = 0; v < ranges[r].numVertices; ++v, at += 3) memcpy(&s->vtxHost[at], src + (size_t)v * normalStride, 12);
        }
    } else {
        for (uint32_t r = 0; r < numRanges; ++r)
            table[r] = rtrdev::VertexRange{static_cast<const uint32_t*>(ranges[r].positions), ranges[r].numVertices ? static_cast<const uint32_t*>(ranges[r].normals) : nullptr,
                                           ranges[r].firstVertex, 0u};
    }
    /* renders and queries of other streams read the vertices, and with RTR_VERTICES_DEVICE the caller's data may still be in the
     * making on one of them: everything enqueued on the device so far is joined (contract in rtr.h) */
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(s->vtxRanges.grow(table.size()));
    HIP_TRY(s->vtxPrefix.grow(prefix.size() + 1));        /* the last word: first bad vertex */
    uint32_t* firstBad = s->vtxPrefix.p + prefix.size();
    const uint32_t none = 0xffffffffu;
    HIP_TRY(hipMemcpyAsync(s->vtxRanges.p, table.data(), table.size() * sizeof(rtrdev::VertexRange), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->vtxPrefix.p, prefix.data(), prefix.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(firstBad, &none, sizeof none, hipMemcpyHostToDevice, st));
    if (!device && !s->vtxHost.empty()) HIP_TRY(hipMemcpyAsync(s->vtxStage.p, s->vtxHost.data(), s->vtxHost.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    for (uint32_t c = 0; c < numChunks; ++c) {
        const uint32_t r0 = c * kChunk, n = std::min(numRanges, r0 + kChunk) - r0;
        const hipError_t e = rtrdev::launch_check_vertices(s->vtxRanges.p + r0, s->vtxPrefix.p + r0 + c, n, chunkBase[c + 1] - chunkBase[c], posWords, chunkBase[c], firstBad, st);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: checking kernel: %s", who, hipGetErrorString(e));
    }
    uint32_t bad = none;
    HIP_TRY(hipMemcpyAsync(&bad, firstBad, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad != none) {
        uint32_t r = 0, v = 0;
        name_bad(bad, &r, &v);
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: range %u, vertex %u (scene vertex %u): non-finite position", who, r, v, ranges[r].firstVertex + v);
    }
    /* nothing of the scene has been touched up to here */
    rc = ensure_refit_ready(s);
    if (rc != RTR_OK) return rc;
    for (uint32_t c = 0; c < numChunks; ++c) {
        const uint32_t r0 = c * kChunk, n = std::min(numRanges, r0 + kChunk) - r0;
        const hipError_t e = rtrdev::launch_write_vertices(s->vtxRanges.p + r0, s->vtxPrefix.p + r0 + c, n, chunkBase[c + 1] - chunkBase[c], posWords, nrmWords, s->vertices.p, st);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: writing kernel: %s", who, hipGetErrorString(e));
    }
    return refit_scene(s, instances, lights, true);
}

int rtr_scene_export_vertices(const rtr_scene* s, RtrVertex* out, size_t bytes) {
    if (!s || (!out && bytes)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_vertices: null argument");
    if (bytes != (size_t)s->numVertices * sizeof(RtrVertex)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_vertices: bytes %zu != %zu", bytes, (size_t)s->numVertices * sizeof(RtrVertex));
    if (!bytes) return RTR_OK;
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpy(out, s->vertices.p, bytes, hipMemcpyDeviceToHost));
    return RTR_OK;
}

/* ---- the enqueued vertex update (contract in rtr.h) ---- */
int rtr_scene_prepare_async_updates(rtr_scene* s) {
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_prepare_async_updates: null scene");
    HIP_TRY(hipSetDevice(s->ctx->device));
    int rc = refresh_mirrors(s);
    if (rc != RTR_OK) return rc;
    if (s->tree.asyncReady) return RTR_OK;
    if (!scene_is_empty(s)) {
        rc = ensure_refit_ready(s);
        if (rc != RTR_OK) return rc;
        rc = upload_prim_tables(s, s->hostInstances.data());
        if (rc != RTR_OK) return rc;
        HIP_TRY(s->tree.orderScratch.ensure(2 * s->tree.hostNodes.size()));
        if (!s->instCustom.p) {      /* kept through a rebuild: the instances are the scene's, not the tree's */
            std::vector<uint32_t> custom(s->hostInstances.size());
            for (size_t i = 0; i < custom.size(); ++i) custom[i] = s->hostInstances[i].customIndex;
            HIP_TRY(s->instCustom.upload(custom.data(), custom.size(), s->ctx->stream));
        }
    }
    if (!s->asyncWords.p) {      /* kept through a rebuild: the status is the scene's, not the tree's */
        const uint32_t none = 0xffffffffu, init[8] = {none, 0u, 0u, 0u, 0u, none, none, 0u};
        HIP_TRY(s->asyncWords.upload(init, 8, s->ctx->stream));
    }
    s->tree.asyncReady = true;
    return RTR_OK;
}

/* What both enqueued updates end in, on the tables and vertices as they are when the stream gets there: the refit, the 4-wide view, its
 * breadth-first order made on the device, the permutation, the light triangles (always remade), and the fold of the update's word
 * (asyncWords[0]) into the sticky status under this call's serial.  Counts the update as enqueued. */
static int enqueue_refit_tail(rtr_scene* s, uint32_t serial, const char* who) {
    hipStream_t st = s->ctx->stream;
    uint32_t* firstBad = s->asyncWords.p;
    SceneTree& t = s->tree;
    const uint32_t n = (uint32_t)t.hostNodes.size();
    rtrdev::BvhInputs in{t.prims.p, t.instRefs.p, s->vertices.p, s->indices.p};
    hipError_t e = rtrdev::bvh_refit_enqueued(in, t.numPrims, t.numNodeSlots, device_arrays(t), st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: device BVH refit: %s", who, hipGetErrorString(e));
    s->mirrorsStale = true;
    e = rtrdev::bvh_make_wide(t.nodes.p, n, t.parent.p, t.grid.p, t.hostWideShape.size() == n ? t.wideShape.p : nullptr, t.nodes4tmp.p, t.wideSums.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: 4-wide node build: %s", who, hipGetErrorString(e));
    e = rtrdev::bvh_wide_order(t.nodes4tmp.p, n, t.wideRemap.p, t.orderScratch.p, s->asyncWords.p + 1, st);
    if (e == hipSuccess) e = rtrdev::bvh_permute_wide(t.nodes4tmp.p, n, t.wideRemap.p, t.nodes4.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: 4-wide node order: %s", who, hipGetErrorString(e));
    if (s->numLights) {
        e = rtrdev::launch_light_tris(s->lights.p, s->vertices.p, s->indices.p, s->lightTriFirst.p, s->numLights, s->lightTris.p, st);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: light-triangle records: %s", who, hipGetErrorString(e));
    }
    e = rtrdev::launch_fold_update_status(firstBad, s->asyncWords.p + 4, serial, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: status kernel: %s", who, hipGetErrorString(e));
    ++s->asyncEnqueued;
    return RTR_OK;
}

int rtr_scene_update_vertices_async(rtr_scene* s, const rtr_vertex_range* ranges, uint32_t numRanges, uint32_t positionStride, uint32_t normalStride) {
    static const char* who = "rtr_scene_update_vertices_async";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (!ranges || numRanges == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null ranges (or numRanges == 0): nothing to update", who);
    int rc = check_vertex_ranges(s, ranges, numRanges, positionStride, normalStride, true, who);
    if (rc != RTR_OK) return rc;
    if (!s->tree.asyncReady) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene has not been prepared: call rtr_scene_prepare_async_updates once first", who);
    const uint32_t serial = (uint32_t)(s->asyncEnqueued + 1);
    if (scene_is_empty(s)) { ++s->asyncEnqueued; return RTR_OK; }      /* nothing to refit, as the synchronous call */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    uint32_t* firstBad = s->asyncWords.p;
    HIP_TRY(hipMemsetAsync(firstBad, 0xff, sizeof(uint32_t), st));
    const uint32_t posWords = positionStride / 4u, nrmWords = normalStride / 4u;
    const uint32_t kChunk = rtrdev::kVertexRangesPerArgs;
    /* the ranges reach the kernels as kernel arguments, a chunk per launch: first every check, then every (predicated) write */
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t r0 = 0; r0 < numRanges; r0 += kChunk) {
            rtrdev::VertexRangeArgs t;
            t.numRanges = std::min(numRanges - r0, kChunk);
            uint32_t acc = 0;
            for (uint32_t k = 0; k < t.numRanges; ++k) {
                const rtr_vertex_range& vr = ranges[r0 + k];
                t.ranges[k] = rtrdev::VertexRange{static_cast<const uint32_t*>(vr.positions), vr.numVertices ? static_cast<const uint32_t*>(vr.normals) : nullptr, vr.firstVertex, 0u};
                t.prefix[k] = acc; acc += vr.numVertices;
            }
            t.prefix[t.numRanges] = acc;
            const hipError_t e = pass == 0 ? rtrdev::launch_check_vertices_args(t, posWords, firstBad, st)
                                           : rtrdev::launch_write_vertices_args(t, posWords, nrmWords, s->vertices.p, firstBad, st);
            if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: %s kernel: %s", who, pass == 0 ? "checking" : "writing", hipGetErrorString(e));
        }
    return enqueue_refit_tail(s, serial, who);
}

int rtr_scene_update_instances_async(rtr_scene* s, const void* transforms, uint32_t transformStride, uint32_t firstInstance, uint32_t numInstances,
                                     const RtrAreaLightInfo* lights, uint32_t numLights) {
    static const char* who = "rtr_scene_update_instances_async";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (!transforms && !lights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null transforms and null lights: nothing to update", who);
    if (!transforms && numInstances) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null transforms with numInstances %u", who, numInstances);
    if (transforms && !numInstances) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: transforms given with numInstances 0", who);
    if (transforms && ((transformStride & 3u) || transformStride < 48u))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: transformStride %u must be a multiple of 4 and at least 48", who, transformStride);
    if ((((uintptr_t)transforms) | ((uintptr_t)lights)) & 3u) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: device pointers must be 4-byte aligned", who);
    /* nothing of the scene has been read up to here */
    if ((uint64_t)firstInstance + numInstances > s->hostInstances.size())
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: instances %u .. %llu leave the scene's %zu instances", who, firstInstance,
                    (unsigned long long)firstInstance + numInstances, s->hostInstances.size());
    if (lights && numLights != s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %u lights given, scene has %u", who, numLights, s->numLights);
    if (!s->tree.asyncReady) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene has not been prepared: call rtr_scene_prepare_async_updates once first", who);
    const uint32_t serial = (uint32_t)(s->asyncEnqueued + 1);
    if (scene_is_empty(s)) { ++s->asyncEnqueued; return RTR_OK; }      /* nothing to refit, as the synchronous call */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    uint32_t* firstBad = s->asyncWords.p;
    HIP_TRY(hipMemsetAsync(firstBad, 0xff, sizeof(uint32_t), st));
    const uint32_t strideWords = transforms ? transformStride / 4u : 12u, sceneInstances = (uint32_t)s->hostInstances.size();
    hipError_t e = rtrdev::launch_check_instances(transforms, strideWords, firstInstance, numInstances, lights, numLights, sceneInstances, s->lights.p, firstBad, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: checking kernel: %s", who, hipGetErrorString(e));
    e = rtrdev::launch_write_instances(transforms, strideWords, firstInstance, numInstances, lights, numLights, s->instCustom.p, rtrdev::kMirroredWord,
                                       s->xforms.p, s->nmats.p, s->tree.instRefs.p, s->lights.p, firstBad, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: writing kernel: %s", who, hipGetErrorString(e));
    s->instancesStale = true;      /* with mirrorsStale, which the tail sets: refresh_mirrors reads the transforms and lights back */
    s->mirrorsStale = true;
    return enqueue_refit_tail(s, serial, who);
}

int rtr_scene_export_instances(const rtr_scene* s, RtrInstance* out, size_t bytes) {
    if (!s || (!out && bytes)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_instances: null argument");
    if (bytes != s->hostInstances.size() * sizeof(RtrInstance))
        return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_instances: bytes %zu != %zu", bytes, s->hostInstances.size() * sizeof(RtrInstance));
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (bytes) memcpy(out, s->hostInstances.data(), bytes);
    return RTR_OK;
}

int rtr_scene_update_status(rtr_scene* s, rtr_update_status* out) {
    static_assert(sizeof(rtr_update_status) == 32, "layout");
    if (!s || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_status: null argument");
    memset(out, 0, sizeof *out);
    out->enqueued = s->asyncEnqueued;
    out->firstRefusedUpdate = out->firstBadVertex = 0xffffffffu;
    if (!s->asyncWords.p) return RTR_OK;      /* never prepared: nothing was enqueued */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    uint32_t w[3];
    HIP_TRY(hipMemcpyAsync(w, s->asyncWords.p + 4, sizeof w, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->refused = w[0]; out->firstRefusedUpdate = w[1]; out->firstBadVertex = w[2];
    if (w[1] != 0xffffffffu) HIP_TRY(hipMemsetAsync(s->asyncWords.p + 5, 0xff, 2 * sizeof(uint32_t), st));      /* "first since the last status call" starts again */
    return RTR_OK;
}

/* ---- the enqueued rebuild (contract in rtr.h) ---- */
int rtr_scene_prepare_async_rebuild(rtr_scene* s) {
    static const char* who = "rtr_scene_prepare_async_rebuild";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    HIP_TRY(hipSetDevice(s->ctx->device));
    int rc = refresh_mirrors(s);
    if (rc != RTR_OK) return rc;
    SceneTree& t = s->tree;
    if (t.rebuildReady) return RTR_OK;
    if (scene_is_empty(s)) {
        rc = rtr_scene_prepare_async_updates(s);
        if (rc == RTR_OK) t.rebuildReady = true;
        return rc;
    }
    /* the commit copies a device build over the live arrays IN PLACE: they must have a device build's sizes already */
    const size_t n = t.hostTris.size();
    if (n < 16 || t.hostNodes.size() != n - 1 || !t.hostWideShape.empty())
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene's tree (%zu triangles, %zu node slots%s) was not made by the device builder, whose arrays an enqueued "
                    "rebuild commits into: call rtr_scene_rebuild(scene, RTR_BUILD_DEVICE_LBVH) first%s", who, n, t.hostNodes.size(),
                    t.hostWideShape.empty() ? "" : ", a cost-driven 4-wide shape", n < 16 ? " (a scene of fewer than 16 triangles always takes the host builder: it has no enqueued rebuild)" : "");
    rc = rtr_scene_prepare_async_updates(s);
    if (rc != RTR_OK) return rc;
    const size_t numNodes = n - 1;
    if (!t.refitReady || t.numPrims != n || t.numNodeSlots != numNodes || t.nodes.n < numNodes * 2 || t.nodesF.n < numNodes * 4 || t.tris.n < n * 3 || t.boxMin.n < n ||
        t.boxMax.n < n || t.parent.n < numNodes || t.counters.n < numNodes || t.depth.n < numNodes || t.slotOfPrim.n < n || t.red.n < 8)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the live arrays do not have a device build's sizes: call rtr_scene_rebuild(scene, RTR_BUILD_DEVICE_LBVH) first", who);
    TreeStage& g = s->stage;
    HIP_TRY(g.nodes.ensure(numNodes * 2)); HIP_TRY(g.nodesF.ensure(numNodes * 4)); HIP_TRY(g.grid.ensure(1)); HIP_TRY(g.tris.ensure(n * 3));
    HIP_TRY(g.boxMin.ensure(n)); HIP_TRY(g.boxMax.ensure(n)); HIP_TRY(g.parent.ensure(numNodes)); HIP_TRY(g.slotOfPrim.ensure(n)); HIP_TRY(g.red.ensure(8));
    rc = ensure_build_scratch(s->buildScratch, (uint32_t)n);
    if (rc != RTR_OK) return rc;
    t.rebuildReady = true;
    return RTR_OK;
}

/* The chain of an enqueued rebuild, counted as enqueued under `serial`.  go: null — rtr_scene_rebuild_async, every launch as it always
 * was — or the policy's decision word (rtr_scene_rebuild_if_async): the build's kernels, the commit and the tail do nothing when it is 0.
 * On a scene prepared for the policy the chain closes with the baseline: the cost of the live tree again, predicated on this chain's own
 * commit, and the one lane that takes it as builtSah. */
static int enqueue_rebuild_chain(rtr_scene* s, uint32_t serial, const char* who, const uint32_t* go) {
    hipStream_t st = s->ctx->stream;
    SceneTree& t = s->tree;
    TreeStage& g = s->stage;
    uint32_t* word = s->asyncWords.p;
    rtrdev::RebuildIfRecord* rec = t.rebuildIfReady ? policy_record(s) : nullptr;
    uint32_t* committed = rec ? &rec->committed : nullptr;
    HIP_TRY(hipMemsetAsync(word, 0xff, sizeof(uint32_t), st));
    /* the build, into the stage, from the LIVE tables (current after enqueued instance updates and mask changes) and the scene's vertices */
    const uint32_t n = t.numPrims, numNodes = t.numNodeSlots;
    rtrdev::BvhDeviceArrays a{};
    a.nodes = g.nodes.p; a.nodesF = g.nodesF.p; a.grid = g.grid.p; a.tris = g.tris.p; a.boxMin = g.boxMin.p; a.boxMax = g.boxMax.p; a.parent = g.parent.p;
    a.counters = t.counters.p; a.depth = t.depth.p; a.slotOfPrim = g.slotOfPrim.p; a.red = g.red.p;
    rtrdev::BvhInputs in{t.prims.p, t.instRefs.p, s->vertices.p, s->indices.p};
    hipError_t e = rtrdev::bvh_build_lbvh_enqueued(in, n, a, scratch_view(s->buildScratch), st, go);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: device BVH build: %s", who, hipGetErrorString(e));
    /* the commit: all staged arrays over their live twins, unless the stack class would have to rise */
    rtrdev::CommitTable ct{};
    auto add = [&](const void* src, void* dst, size_t bytes) { ct.a[ct.count].src = src; ct.a[ct.count].dst = dst; ct.a[ct.count].bytes = bytes; ++ct.count; };
    add(g.nodesF.p, t.nodesF.p, (size_t)numNodes * 64); add(g.tris.p, t.tris.p, (size_t)n * 48); add(g.nodes.p, t.nodes.p, (size_t)numNodes * 32);
    add(g.boxMin.p, t.boxMin.p, (size_t)n * 16); add(g.boxMax.p, t.boxMax.p, (size_t)n * 16); add(g.parent.p, t.parent.p, (size_t)numNodes * 4);
    add(g.slotOfPrim.p, t.slotOfPrim.p, (size_t)n * 4); add(g.grid.p, t.grid.p, sizeof(RtrBvhGrid)); add(g.red.p, t.red.p, 8 * sizeof(uint32_t));
    e = rtrdev::bvh_commit_tree(ct, g.red.p, t.stats.stackEntries, word, st, go, committed);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: commit kernel: %s", who, hipGetErrorString(e));
    s->mirrorsStale = true; s->depthStale = true;
    /* the 4-wide view of whatever tree is live now (after a refused commit: the unchanged one, whose bytes these launches reproduce) */
    e = rtrdev::bvh_make_wide(t.nodes.p, numNodes, t.parent.p, t.grid.p, nullptr, t.nodes4tmp.p, t.wideSums.p, st, go);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: 4-wide node build: %s", who, hipGetErrorString(e));
    e = rtrdev::bvh_wide_order(t.nodes4tmp.p, numNodes, t.wideRemap.p, t.orderScratch.p, s->asyncWords.p + 1, st, go);
    if (e == hipSuccess) e = rtrdev::bvh_permute_wide(t.nodes4tmp.p, numNodes, t.wideRemap.p, t.nodes4.p, st, go);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: 4-wide node order: %s", who, hipGetErrorString(e));
    if (t.leafReady) {      /* the leaf order changed: the table is made again where it is (4 B per triangle, nothing to allocate) */
        /* gated, the clearing is a kernel: a skip must not clear the table without the launch that fills it again */
        if (go) e = rtrdev::bvh_clear_words(reinterpret_cast<uint32_t*>(t.leafTable.p), t.leafTable.n, st, go);
        else HIP_TRY(hipMemsetAsync(t.leafTable.p, 0, t.leafTable.n * sizeof(int32_t), st));
        if (e == hipSuccess)
            e = rtrdev::launch_leaf_table(t.nodes.p, (uint32_t)(t.nodes.n / 2), t.tris.p, (uint32_t)(t.tris.n / 3), s->triCount.p, s->leafBase.p, s->numInstances, t.leafTable.p, st, go);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: leaf table: %s", who, hipGetErrorString(e));
    }
    if (rec) {      /* the baseline follows the build: sums of the new live tree and builtSah from them, when this chain's commit copied */
        e = rtrdev::bvh_tree_cost(t.nodes.p, numNodes, t.parent.p, s->policy.p, st, committed);
        if (e == hipSuccess) e = rtrdev::bvh_rebuild_if_close(s->policy.p, t.grid.p, rec, go ? 1u : 0u, st);
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: baseline kernels: %s", who, hipGetErrorString(e));
    }
    e = rtrdev::launch_fold_update_status(word, s->asyncWords.p + 4, serial, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: status kernel: %s", who, hipGetErrorString(e));
    ++s->asyncEnqueued;
    return RTR_OK;
}

int rtr_scene_rebuild_async(rtr_scene* s, uint32_t buildFlags) {
    static const char* who = "rtr_scene_rebuild_async";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (buildFlags == RTR_BUILD_HOST_SAH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: buildFlags RTR_BUILD_HOST_SAH: the host builder is host code and cannot be enqueued; only RTR_BUILD_DEVICE_LBVH can", who);
    if (buildFlags != RTR_BUILD_DEVICE_LBVH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown buildFlags %u", who, buildFlags);
    /* nothing of the scene has been read up to here */
    if (!s->tree.rebuildReady)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene is not prepared for an enqueued rebuild: call rtr_scene_prepare_async_rebuild first (once per scene, and again after a host rebuild)", who);
    const uint32_t serial = (uint32_t)(s->asyncEnqueued + 1);
    if (scene_is_empty(s)) { ++s->asyncEnqueued; return RTR_OK; }      /* nothing to build, as the synchronous call */
    HIP_TRY(hipSetDevice(s->ctx->device));
    return enqueue_rebuild_chain(s, serial, who, nullptr);
}

/* ---- the rebuild policy on the device (contract in rtr.h) ---- */
/* sets the baseline to the cost of the tree as it is now; the counts of a scene that was prepared before go on */
static int prepare_rebuild_if(rtr_scene* s, const char* who) {
    int rc = rtr_scene_prepare_async_rebuild(s);
    if (rc != RTR_OK) return rc;
    SceneTree& t = s->tree;
    if (t.rebuildIfReady) return RTR_OK;
    if (scene_is_empty(s)) { t.rebuildIfReady = true; return RTR_OK; }
    if (rtrdev::bvh_tree_cost_words() + 1 != kPolicyRecordAt) return fail(RTR_ERR_HIP, "%s: the cost kernel has %zu words, the policy expects 11", who, rtrdev::bvh_tree_cost_words());
    rtr_tree_cost c{};
    rc = rtr_scene_tree_cost(s, &c);      /* joins the scene's stream */
    if (rc != RTR_OK) return rc;
    hipStream_t st = s->ctx->stream;
    if (!s->policy.p) {
        HIP_TRY(s->policy.alloc(kPolicyWords));
        HIP_TRY(hipMemsetAsync(s->policy.p, 0, kPolicyWords * sizeof(unsigned long long), st));
        rtrdev::RebuildIfRecord r{};
        r.builtSah = c.sah; r.lastDecision = 0xffffffffu;
        HIP_TRY(hipMemcpyAsync(policy_record(s), &r, sizeof r, hipMemcpyHostToDevice, st));
    } else
        HIP_TRY(hipMemcpyAsync(&policy_record(s)->builtSah, &c.sah, sizeof c.sah, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      /* the copies read this frame's variables */
    t.rebuildIfReady = true;
    return RTR_OK;
}

int rtr_scene_prepare_async_rebuild_if(rtr_scene* s) {
    static const char* who = "rtr_scene_prepare_async_rebuild_if";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    return prepare_rebuild_if(s, who);
}

int rtr_scene_rebuild_if_async(rtr_scene* s, uint32_t buildFlags, double rebuildAbove) {
    static const char* who = "rtr_scene_rebuild_if_async";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (buildFlags == RTR_BUILD_HOST_SAH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: buildFlags RTR_BUILD_HOST_SAH: the host builder is host code and cannot be enqueued; only RTR_BUILD_DEVICE_LBVH can", who);
    if (buildFlags != RTR_BUILD_DEVICE_LBVH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown buildFlags %u", who, buildFlags);
    if (!(rebuildAbove >= 0.0)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: rebuildAbove %g must be a number >= 0 (+inf: never rebuild)", who, rebuildAbove);
    /* nothing of the scene has been read up to here */
    if (!s->tree.rebuildIfReady)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene is not prepared for the rebuild policy: call rtr_scene_prepare_async_rebuild_if first (once per scene, and again after a host rebuild)", who);
    const uint32_t serial = (uint32_t)(s->asyncEnqueued + 1);
    if (scene_is_empty(s)) { ++s->asyncEnqueued; return RTR_OK; }      /* nothing to look at */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    SceneTree& t = s->tree;
    rtrdev::RebuildIfRecord* rec = policy_record(s);
    /* the cost of the live tree and the decision, both on the device */
    hipError_t e = rtrdev::bvh_tree_cost(t.nodes.p, t.numNodeSlots, t.parent.p, s->policy.p, st);
    if (e == hipSuccess) e = rtrdev::bvh_rebuild_if_decide(s->policy.p, t.grid.p, rec, rebuildAbove, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: cost and decision kernels: %s", who, hipGetErrorString(e));
    return enqueue_rebuild_chain(s, serial, who, &rec->go);
}

int rtr_scene_rebuild_if_status(rtr_scene* s, rtr_rebuild_if_status* out) {
    static const char* who = "rtr_scene_rebuild_if_status";
    static_assert(sizeof(rtr_rebuild_if_status) == sizeof(rtrdev::RebuildIfRecord), "layout");
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (!out) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null out", who);
    memset(out, 0, sizeof *out);
    out->lastDecision = 0xffffffffu;
    if (!s->policy.p) return RTR_OK;      /* never prepared (or empty): nothing was evaluated */
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    rtrdev::RebuildIfRecord r{};
    HIP_TRY(hipMemcpyAsync(&r, policy_record(s), sizeof r, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->evaluated = r.evaluated; out->rebuilt = r.rebuilt; out->builtSah = r.builtSah; out->lastSah = r.lastSah; out->lastDecision = r.lastDecision;
    return RTR_OK;
}

/* ---- the cost of the tree, and the rebuild (contracts in rtr.h) ---- */
/* the integer sums are complete: sah from them in double, in the order rtr.h states (-ffp-contract=off: no fused step) */
static void finish_tree_cost(rtr_tree_cost* c, const RtrBvhGrid& grid) {
    uint64_t w[11];
    for (int k = 0; k < 3; ++k) { w[k] = c->innerArea[k]; w[3 + k] = c->leafArea[k]; w[6 + k] = c->rootArea[k]; }
    w[9] = c->numInner; w[10] = c->numLeafRefs;
    c->sah = rtr_tree_sah(w, grid.scale[0], grid.scale[1], grid.scale[2]);      /* the device's function too (kernels/rtr_tree_sah.h) */
}

int rtr_host_tree_cost(const RtrBvhNode* nodes, size_t nodeBytes, const RtrBvhGrid* grid, rtr_tree_cost* out) {
    if (!nodes || !grid || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_tree_cost: null argument");
    if (nodeBytes == 0 || nodeBytes % sizeof(RtrBvhNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_tree_cost: nodeBytes %zu is not a positive multiple of %zu", nodeBytes, sizeof(RtrBvhNode));
    const size_t n = nodeBytes / sizeof(RtrBvhNode);
    rtr_tree_cost c{};
    auto triple = [](const uint32_t lo[3], const uint32_t hi[3], uint64_t t[3]) {
        uint64_t d[3];
        for (int k = 0; k < 3; ++k) d[k] = hi[k] > lo[k] ? (uint64_t)(hi[k] - lo[k]) : 0u;
        t[0] = d[0] * d[1]; t[1] = d[1] * d[2]; t[2] = d[2] * d[0];
    };
    /* the walk from the root: every node it reaches is counted once, whichever slots name it */
    std::vector<uint8_t> seen(n, 0);
    std::vector<uint32_t> stack{0};
    seen[0] = 1;
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        const RtrBvhNode& nd = nodes[i];
        uint32_t lo[2][3], hi[2][3];
        uint64_t t[3];
        for (int sd = 0; sd < 2; ++sd) {
            for (int a = 0; a < 3; ++a) { lo[sd][a] = nd.q[RTR_BVH_QSLOT(sd, 0, a)]; hi[sd][a] = nd.q[RTR_BVH_QSLOT(sd, 1, a)]; }
            triple(lo[sd], hi[sd], t);
            const int32_t code = nd.child[sd];
            if (code >= 0) {
                if ((size_t)code >= n) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_host_tree_cost: node %u names child %d, the array has %zu nodes", i, code, n);
                for (int k = 0; k < 3; ++k) c.innerArea[k] += t[k];
                ++c.numInner;
                if (!seen[(size_t)code]) { seen[(size_t)code] = 1; stack.push_back((uint32_t)code); }
            } else {
                const uint64_t cnt = ((uint32_t)~code & 7u) + 1u;
                for (int k = 0; k < 3; ++k) c.leafArea[k] += cnt * t[k];
                ++c.numLeafRefs;
            }
        }
        if (i == 0) {
            uint32_t rlo[3], rhi[3];
            for (int a = 0; a < 3; ++a) { rlo[a] = std::min(lo[0][a], lo[1][a]); rhi[a] = std::max(hi[0][a], hi[1][a]); }
            triple(rlo, rhi, t);
            for (int k = 0; k < 3; ++k) { c.innerArea[k] += t[k]; c.rootArea[k] = t[k]; }
            ++c.numInner;
        }
    }
    finish_tree_cost(&c, *grid);
    *out = c;
    return RTR_OK;
}

int rtr_scene_tree_cost(const rtr_scene* s, rtr_tree_cost* out) {
    if (!s || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_tree_cost: null argument");
    HIP_TRY(hipSetDevice(s->ctx->device));
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }      /* the grid the sums are scaled with */
    hipStream_t st = s->ctx->stream;
    const SceneTree& t = s->tree;
    const uint32_t numNodes = (uint32_t)t.hostNodes.size();
    /* which slots are part of the tree: the refit's parent array where the scene has one (a device build leaves slots unused); a host
     * tree without one is looked at once, and gets a parent array of its own only if the root does not reach every slot */
    const int32_t* parent = t.refitReady ? t.parent.p : nullptr;
    if (!t.refitReady && t.costParentState == 0) {
        std::vector<int32_t> par;
        if (host_parent_array(t.hostNodes, par) == t.hostNodes.size()) t.costParentState = 1;
        else { HIP_TRY(t.costParent.upload(par.data(), par.size(), st)); t.costParentState = 2; }
    }
    if (!t.refitReady && t.costParentState == 2) parent = t.costParent.p;
    const size_t words = rtrdev::bvh_tree_cost_words();
    HIP_TRY(s->costWords.ensure(words));
    const hipError_t e = rtrdev::bvh_tree_cost(t.nodes.p, numNodes, parent, s->costWords.p, st);
    if (const int rc = launched(e, "rtr_scene_tree_cost")) return rc;
    uint64_t w[11];
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "layout");
    if (words != 11) return fail(RTR_ERR_HIP, "rtr_scene_tree_cost: the kernel has %zu words, the host expects 11", words);
    HIP_TRY(hipMemcpyAsync(w, s->costWords.p, sizeof w, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rtr_tree_cost c{};
    for (int k = 0; k < 3; ++k) { c.innerArea[k] = w[k]; c.leafArea[k] = w[3 + k]; c.rootArea[k] = w[6 + k]; }
    c.numInner = w[9]; c.numLeafRefs = w[10];
    finish_tree_cost(&c, t.stats.grid);
    *out = c;
    return RTR_OK;
}

int rtr_scene_rebuild(rtr_scene* s, uint32_t buildFlags) {
    static const char* who = "rtr_scene_rebuild";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    if (buildFlags > RTR_BUILD_DEVICE_LBVH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown buildFlags %u", who, buildFlags);
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (scene_is_empty(s)) return RTR_OK;     /* nothing to build */
    HIP_TRY(hipSetDevice(s->ctx->device));
    /* frames and queries of OTHER contexts (other streams) may be walking this tree: everything enqueued on the device so far is joined
     * before it is replaced (contract in rtr.h, as the update calls) */
    HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s->ctx->stream;
    const size_t totalPrims = s->tree.hostTris.size();
    const bool deviceBuild = buildFlags == RTR_BUILD_DEVICE_LBVH && totalPrims >= 16;     /* tiny scenes: the host builder, as at creation */
    /* the new tree is built apart from the scene, from its vertices and host mirrors: whatever fails, `s` is as it was */
    SceneTree fresh;
    int rc = RTR_OK;
    if (deviceBuild) {
        std::vector<rtrdev::PrimRef> prims; std::vector<rtrdev::InstanceRef> refs;
        scene_prim_tables(s, s->hostInstances.data(), prims, refs);
        rc = build_on_device_core(fresh, st, prims, refs, s->vertices.p, s->indices.p, s->buildScratch, totalPrims);
        if (rc != RTR_OK) return rc;
    } else {
        std::vector<RtrVertex> vertices(s->numVertices); std::vector<uint32_t> indices(s->numIndices);
        if (s->numVertices) HIP_TRY(hipMemcpy(vertices.data(), s->vertices.p, vertices.size() * sizeof(RtrVertex), hipMemcpyDeviceToHost));
        if (s->numIndices) HIP_TRY(hipMemcpy(indices.data(), s->indices.p, indices.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        rtr_scene_desc view = host_view(s);
        view.vertices = vertices.data(); view.numVertices = s->numVertices; view.indices = indices.data(); view.numIndices = s->numIndices;
        rtr::BvhResult bvh; std::vector<float> xforms, nmats; uint32_t stackEntries = 0; size_t numTris = 0;
        rc = flatten_and_build(&view, bvh, xforms, nmats, &stackEntries, &numTris);      /* the transform tables it fills are the scene's own already */
        if (rc != RTR_OK) return rc;
        if (!s->hostMasks.empty()) {      /* the new records carry the instance masks, as a refit's do */
            const std::vector<uint32_t> maskBits = instance_mask_bits(s, s->hostMasks.data());
            for (RtrBvhTri& tr : bvh.tris) if (tr.customIndex < maskBits.size()) tr.flags |= maskBits[tr.customIndex];
        }
        HIP_TRY(fresh.nodes.upload(reinterpret_cast<const uint4*>(bvh.nodes.data()), bvh.nodes.size() * 2, st));
        HIP_TRY(fresh.grid.upload(&bvh.grid, 1, st));
        HIP_TRY(fresh.tris.upload(reinterpret_cast<const float4*>(bvh.tris.data()), bvh.tris.size() * 3, st));
        fill_stats(fresh.stats, bvh, stackEntries, numTris);
        fresh.hostNodes.swap(bvh.nodes); fresh.hostTris.swap(bvh.tris); fresh.hostWideShape.swap(bvh.wideShape);
        fresh.numPrims = (uint32_t)fresh.hostTris.size(); fresh.numNodeSlots = (uint32_t)fresh.hostNodes.size();
    }
    rc = make_wide_nodes(fresh, st);
    if (rc != RTR_OK) return rc;
    /* the stage outlives a host rebuild, which drops the readiness: a scene that was EVER prepared for the enqueued rebuild is prepared
     * again by the next rebuild that gives it a device tree */
    const bool prepared = s->tree.asyncReady, preparedRebuild = s->tree.rebuildReady || s->stage.red.p != nullptr;
    const bool preparedPolicy = s->tree.rebuildIfReady || s->policy.p != nullptr;      /* likewise; its baseline becomes the new tree's cost */
    std::swap(s->tree, fresh);      /* `fresh` takes the old tree away: freed on return — the device was joined, and nothing has been enqueued against it since */
    point_at_tree(s->dev, s->tree);
    /* the enqueued update's tables and scratch belong to a tree: made again for the new one (its node count, its leaf slots) */
    if (prepared) { rc = rtr_scene_prepare_async_updates(s); if (rc != RTR_OK) return rc; }
    /* and the enqueued rebuild's readiness, where the new tree can take a commit: a host tree has other sizes, and stays unprepared */
    if (preparedRebuild && deviceBuild) { rc = rtr_scene_prepare_async_rebuild(s); if (rc != RTR_OK) return rc; }
    return preparedPolicy && deviceBuild ? prepare_rebuild_if(s, who) : RTR_OK;
}

void rtr_scene_destroy(rtr_scene* s) {
    if (!s) return;
    rtr_ctx* c = s->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete s;
    ctx_release_child(c);
}

int rtr_scene_get_stats(const rtr_scene* s, rtr_scene_stats* out) {
    if (!s || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_get_stats: null argument");
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    *out = s->tree.stats;
    return RTR_OK;
}

int rtr_scene_export_bvh(const rtr_scene* s, RtrBvhNode* nodes, size_t nodeBytes, RtrBvhTri* tris, size_t triBytes) {
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_bvh: null scene");
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (nodes) {
        if (nodeBytes != s->tree.hostNodes.size() * sizeof(RtrBvhNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_bvh: nodeBytes %zu != %zu", nodeBytes, s->tree.hostNodes.size() * sizeof(RtrBvhNode));
        memcpy(nodes, s->tree.hostNodes.data(), nodeBytes);
    }
    if (tris) {
        if (triBytes != s->tree.hostTris.size() * sizeof(RtrBvhTri)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_bvh: triBytes %zu != %zu", triBytes, s->tree.hostTris.size() * sizeof(RtrBvhTri));
        memcpy(tris, s->tree.hostTris.data(), triBytes);
    }
    return RTR_OK;
}

int rtr_scene_export_wide(const rtr_scene* s, RtrWideNode* nodes, size_t nodeBytes) {
    if (!s || !nodes) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_wide: null argument");
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }
    if (nodeBytes != (size_t)s->tree.wideReached * sizeof(RtrWideNode)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_export_wide: nodeBytes %zu != %zu", nodeBytes, (size_t)s->tree.wideReached * sizeof(RtrWideNode));
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpy(nodes, s->tree.nodes4.p, nodeBytes, hipMemcpyDeviceToHost));      /* the records the tree reaches come first */
    return RTR_OK;
}

int rtr_scene_update_lights(rtr_scene* s, const RtrAreaLightInfo* lights, uint32_t n) {
    if (!s || (!lights && n)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_lights: null argument");
    if (n != s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_lights: %u lights given, scene has %u (light geometry is part of the BVH)", n, s->numLights);
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }      /* the transforms compared below: an enqueued instance update may have moved the lights */
    for (uint32_t l = 0; l < n; ++l) {
        if (lights[l].vertexOffset != s->hostLights[l].vertexOffset || lights[l].indexOffset != s->hostLights[l].indexOffset ||
            lights[l].numTriangles != s->hostLights[l].numTriangles || memcmp(lights[l].transform, s->hostLights[l].transform, sizeof lights[l].transform))
            return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_scene_update_lights: light %u geometry/transform changed; only colour, intensity and sidedness may be updated without a rebuild", l);
    }
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (n) {
        HIP_TRY(hipDeviceSynchronize());       /* frames in flight on other streams read s->lights: joined before the rewrite (contract in rtr.h) */
        HIP_TRY(hipMemcpyAsync(s->lights.p, lights, n * sizeof(RtrAreaLightInfo), hipMemcpyHostToDevice, s->ctx->stream));
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        s->hostLights.assign(lights, lights + n);
    }
    return RTR_OK;
}

/* The traversal kernels address triangle records, BVH2 nodes and 4-wide records through 32-bit byte offsets from one buffer base
 * each ((first + i) * 48, node << 5, record << 6 in signed 32-bit lane arithmetic: kernels/rtr_device.h trace(), kernels/rtr_kernels.hip
 * inner_nodes4 / tri_any): a scene whose arrays reach 2 GiB would silently intersect the wrong records, so it is refused here. */
int rtr_check_scene_limits(uint64_t numTriangles, uint64_t numNodes) {
    const uint64_t kMaxBytes = 1ull << 31;
    if (numTriangles >= (1ull << 28)) return fail(RTR_ERR_INVALID_ARGUMENT, "%llu triangles: too many for the leaf encoding (2^28)", (unsigned long long)numTriangles);
    if (numTriangles * sizeof(RtrBvhTri) >= kMaxBytes)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%llu triangles: the %zu-byte triangle records would reach 2 GiB, past the kernels' 32-bit record offsets (at most %llu triangles)",
                    (unsigned long long)numTriangles, sizeof(RtrBvhTri), (unsigned long long)((kMaxBytes - 1) / sizeof(RtrBvhTri)));
    if (numNodes * RTR_WIDE_NODE_BYTES >= kMaxBytes)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%llu BVH nodes: the %d-byte 4-wide records would reach 2 GiB, past the kernels' 32-bit record offsets (at most %llu nodes)",
                    (unsigned long long)numNodes, RTR_WIDE_NODE_BYTES, (unsigned long long)((kMaxBytes - 1) / RTR_WIDE_NODE_BYTES));
    return RTR_OK;
}

/* ---- frame -------------------------------------------------------------------------------- */
/* ownImages == false: a part of a split render (no images of its own, see rtr_frame::parts) */
static int frame_new(rtr_ctx* ctx, uint32_t width, uint32_t rows, uint32_t images, bool ownImages, rtr_frame** out) {
    if (!ctx || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_create: null ctx/out");
    if (ctx->destroyed) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_create: the context has been destroyed");
    *out = nullptr;
    if (width == 0 || rows == 0 || width > 65536 || rows > 65536) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_create: bad extent %ux%u", width, rows);
    if (images == 0) images = RTR_IMAGES_FRAMEBUFFER;
    const uint32_t known = 0xffu | RTR_IMG_BIT(RTR_IMAGE_HDR);
    if (images & ~known) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_create: unknown image bits 0x%x", images & ~known);
    HIP_TRY(hipSetDevice(ctx->device));
    rtr_frame* f = new rtr_frame();
    f->ctx = ctx; ++ctx->children; f->width = width; f->rows = rows; f->images = images;
    const size_t px = (size_t)width * rows;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 8 && e == hipSuccess && ownImages; ++i)
        if (images & RTR_IMG_BIT(i)) { e = f->img[i].alloc(px); if (e == hipSuccess) e = hipMemsetAsync(f->img[i].p, 0, px * 4, ctx->stream); }
    if (e == hipSuccess && ownImages && (images & RTR_IMG_BIT(RTR_IMAGE_HDR))) { e = f->hdr.alloc(px); if (e == hipSuccess) e = hipMemsetAsync(f->hdr.p, 0, px * 16, ctx->stream); }
    if (e == hipSuccess) e = f->counters.alloc(1);
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&f->ev[i]);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreate(&f->evMega[i]);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { rtr_frame_destroy(f); return fail(e == hipErrorOutOfMemory ? RTR_ERR_OUT_OF_MEMORY : RTR_ERR_HIP, "rtr_frame_create: %s", hipGetErrorString(e)); }
    *out = f;
    return RTR_OK;
}

int rtr_frame_create(rtr_ctx* ctx, uint32_t width, uint32_t rows, uint32_t images, rtr_frame** out) {
    return frame_new(ctx, width, rows, images, true, out);
}

void rtr_frame_destroy(rtr_frame* f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    for (auto& e : f->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : f->evMega) if (e) (void)hipEventDestroy(e);
    if (f->evDone) { (void)hipEventSynchronize(f->evDone); (void)hipEventDestroy(f->evDone); }
    if (f->evOwn) (void)hipEventDestroy(f->evOwn);
    for (rtr_frame* part : f->parts) rtr_frame_destroy(part);
    for (rtr_ctx* pc : f->partCtx) rtr_ctx_destroy(pc);
    for (auto& e : f->evPart) if (e) (void)hipEventDestroy(e);
    for (auto& e : f->evSplit) if (e) (void)hipEventDestroy(e);
    rtr_ctx* c = f->ctx;
    delete f;
    ctx_release_child(c);
}

int rtr_frame_bind_external(rtr_frame* f, int which, void* dptr, size_t bytes) {
    if (!f || which < 0 || which > 7) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_bind_external: bad argument");
    if (dptr && bytes != (size_t)f->width * f->rows * 4) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_bind_external: %zu bytes given, image is %zu", bytes, (size_t)f->width * f->rows * 4);
    if (dptr && ((uintptr_t)dptr & 3u)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_bind_external: pointer not 4-byte aligned");
    f->ext[which] = (uint32_t*)dptr;
    if (dptr) f->images |= RTR_IMG_BIT(which);
    return RTR_OK;
}

int rtr_frame_device_ptr(const rtr_frame* f, int which, void** dptr, size_t* bytes) {
    if (!f || !dptr) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_device_ptr: null argument");
    if (which == RTR_IMAGE_HDR) {
        if (!f->hdr.p) return fail(RTR_ERR_INVALID_ARGUMENT, "frame has no HDR image");
        *dptr = f->hdr.p; if (bytes) *bytes = (size_t)f->width * f->rows * 16; return RTR_OK;
    }
    if (which < 0 || which > 7 || !f->image_ptr(which)) return fail(RTR_ERR_INVALID_ARGUMENT, "frame has no image %d", which);
    *dptr = f->image_ptr(which); if (bytes) *bytes = (size_t)f->width * f->rows * 4;
    return RTR_OK;
}

int rtr_frame_download(const rtr_frame* f, int which, void* dst, size_t bytes) {
    if (!f || !dst) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_download: null argument");
    void* src = nullptr; size_t need = 0;
    int rc = rtr_frame_device_ptr(f, which, &src, &need);
    if (rc != RTR_OK) return rc;
    if (bytes != need) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_download: %zu bytes given, image %d is %zu", bytes, which, need);
    HIP_TRY(hipSetDevice(f->ctx->device));
    if (f->viaBatch) HIP_TRY(hipEventSynchronize(f->evDone));          /* its pixels came from another frame's stream */
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, f->ctx->stream));
    HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return RTR_OK;
}

/* Work about to be enqueued for `f` on its own stream comes behind a batch launch on another stream that wrote it last (the launch
 * runs on its leading frame's stream), and a later batch must come behind this work (ownPending): the ordering contract of
 * rtr_render_batch_async for everything that is not itself a render */
static int order_on_own_stream(rtr_frame* f) {
    hipStream_t st = f->ctx->stream;
    if (f->batchStream && f->batchStream != st) HIP_TRY(hipStreamWaitEvent(st, f->evDone, 0));
    f->batchStream = nullptr;
    f->ownPending = true;
    return RTR_OK;
}

int rtr_frame_clear(rtr_frame* f) {
    if (!f) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_clear: null frame");
    HIP_TRY(hipSetDevice(f->ctx->device));
    { const int rc = order_on_own_stream(f); if (rc != RTR_OK) return rc; }
    const size_t px = (size_t)f->width * f->rows;
    for (int i = 0; i < 8; ++i) if (f->image_ptr(i)) HIP_TRY(hipMemsetAsync(f->image_ptr(i), 0, px * 4, f->ctx->stream));
    if (f->hdr.p) HIP_TRY(hipMemsetAsync(f->hdr.p, 0, px * 16, f->ctx->stream));
    HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return RTR_OK;
}

/* ---- dispatch ------------------------------------------------------------------------------ */
/* Enqueues one launch of the pipeline over n frames (n = 1: rtr_render / rtr_render_async).  frames[0] leads: its context's stream
 * carries the work, its scratch holds the batch, its statistics describe the launch. */
static_assert(RTR_MAX_BATCH == rtrdev::kMaxBatch, "include/rtr.h and kernels/rtr_device.h disagree on the frames per launch");
static int enqueue_render(rtr_scene* s, const RtrCameraData* cams, const RtrSceneInfo* infos, const rtr_render_params* pin, rtr_frame* const* frames, uint32_t n, bool direct = false) {
    if (!s || !cams || !infos || !pin || !frames || n < 1 || !frames[0]) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: null argument");
    if (n > rtrdev::kMaxBatch) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: %u frames, at most %u per launch", n, rtrdev::kMaxBatch);
    rtr_frame* f = frames[0];
    /* work is enqueued on the (leading) FRAME's context stream; the (read-only) scene may belong to another context of the same
     * device, so two frames on two streams can be in flight against one scene */
    if (s->ctx->device != f->ctx->device) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: scene and frame live on different devices");
    rtr_render_params p = *pin;
    if (p.bandRows == 0) p.bandRows = 8;
    if (p.shardCount == 0) p.shardCount = 1;
    if (p.images == 0) p.images = RTR_IMAGES_FRAMEBUFFER;
    if (p.width == 0 || p.height == 0 || p.spp == 0 || p.spp > 1024 || p.numShadowRays > 1024)
        return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: bad width/height/spp/numShadowRays (%u,%u,%u,%u)", p.width, p.height, p.spp, p.numShadowRays);
    if (p.bandRows % 8u) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: bandRows %u must be a multiple of 8 (one wave = one 8x8 tile)", p.bandRows);
    if (p.shardIndex >= p.shardCount) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: shardIndex %u >= shardCount %u", p.shardIndex, p.shardCount);
    const uint32_t rows = rtr_shard_rows(p.height, p.bandRows, p.shardCount);
    const uint32_t frameRows = direct ? p.height : rows;     /* direct: the images are the whole frame, this shard writes its own rows of them */
    if (p.images & RTR_IMAGES_DENOISE) return fail(RTR_ERR_UNSUPPORTED, "rtr_render: denoise/combine images are produced by rtr_denoise_combine, not by the ray-gen dispatch");
    if ((p.images & RTR_IMG_BIT(RTR_IMAGE_ANALYTIC)) && !s->hasLtc) return fail(RTR_ERR_UNSUPPORTED, "rtr_render: RTR_IMAGE_ANALYTIC needs the LTC tables (rtr_scene_desc.ltc1/ltc2)");
    const bool wantHdr = (p.images & RTR_IMG_BIT(RTR_IMAGE_HDR)) != 0 || p.accumulate;
    if (n > 1 && p.pipeline == 1) return fail(RTR_ERR_UNSUPPORTED, "rtr_render_batch_async: the megakernel renders one frame per launch");

    rtrdev::FrameBatch fb{};
    fb.n = n;
    uint32_t k = 0;
    uint64_t maxRays = 1;
    for (uint32_t b = 0; b < n; ++b) {
        rtr_frame* fr = frames[b];
        if (!fr) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: frame %u is null", b);
        for (uint32_t c = 0; c < b; ++c) if (frames[c] == fr) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: frame %u given twice", b);
        if (fr->ctx->device != f->ctx->device) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: frame %u lives on another device", b);
        if (infos[b].numAreaLights > s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: SceneInfo.numAreaLights %u > scene lights %u", infos[b].numAreaLights, s->numLights);
        if (infos[b].numAreaLights != infos[0].numAreaLights) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_async: the frames of a launch must use the same number of area lights");
        if (fr->width != p.width || fr->rows != frameRows) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: frame is %ux%u, this shard needs %ux%u", fr->width, fr->rows, p.width, frameRows);
        if (wantHdr && !fr->hdr_ptr()) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: HDR accumulation requested but the frame has no RTR_IMAGE_HDR");
        FrameOut& fo = fb.fo[b];
        k = 0;
        for (int i = 0; i < 8; ++i) {
            fo.img[i] = nullptr;
            if (p.images & RTR_IMG_BIT(i)) {
                if (!fr->image_ptr(i)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: image %d requested but not in the frame", i);
                fo.img[i] = fr->image_ptr(i); ++k;
            }
        }
        fo.hdr = wantHdr ? fr->hdr_ptr() : nullptr;
        RenderArgs& ra = fb.ra[b];
        ra.cam = cams[b]; ra.info = infos[b];
        ra.width = p.width; ra.height = p.height; ra.spp = p.spp; ra.numShadowRays = p.numShadowRays;
        ra.bandRows = p.bandRows; ra.shardIndex = p.shardIndex; ra.shardCount = p.shardCount;
        ra.localRows = rows; ra.tilesPerRow = (p.width + 7u) / 8u;
        ra.images = p.images; ra.accumulate = p.accumulate; ra.accumulatedFrames = p.accumulatedFrames; ra.directRows = direct ? 1u : 0u;
        if (b == 0) for (uint32_t l = 0; l < infos[0].numAreaLights; ++l) maxRays += (uint64_t)s->hostLights[l].numTriangles * p.numShadowRays;
        ra.maxRaysPerSample = (uint32_t)maxRays;
    }
    const RenderArgs& ra = fb.ra[0];
    const FrameOut& fo = fb.fo[0];

    HIP_TRY(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    Counters* dstats = nullptr;
    if (p.collectStats) { HIP_TRY(hipMemsetAsync(f->counters.p, 0, sizeof(Counters), st)); dstats = f->counters.p; }

    const uint64_t paddedPixels = (uint64_t)((rows + 7u) / 8u) * ra.tilesPerRow * 64u;
    const uint64_t blocks = (paddedPixels + 255u) / 256u;
    const uint64_t nPS = blocks * 256u * p.spp * n;          /* pixel-sample slots of the launch */
    const uint64_t nRays = nPS * maxRays;                    /* queue capacity: every pixel-sample issuing every query */
    uint64_t slotStride = 256;                                /* the visibility planes are a power of two apart, so a slot names its pixel-sample with a mask */
    while (slotStride < nPS) slotStride <<= 1;
    const uint64_t nSlots = slotStride * maxRays;
    bool wave = p.pipeline != 1;
    if (wave && (nSlots >= (1ull << 31) || maxRays > 4096)) {
        if (p.pipeline == 2 || n > 1) return fail(RTR_ERR_UNSUPPORTED, "rtr_render: wavefront scratch would need %llu visibility slots", (unsigned long long)nSlots);
        wave = false;
    }
    if (blocks * n >= (1ull << 31)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render: frame too large");

    /* the counting form IS the timed kernel template; the 2-wide comparison kernel has none, and counting another kernel's work
     * under its name would be a wrong number */
    if (wave && p.collectStats && f->ctx->tun.trace_bvh4 == 0u)
        return fail(RTR_ERR_UNSUPPORTED, "rtr_render: collectStats with the tunable trace_bvh4 = 0: the 2-wide comparison kernel has no counting form (set it back to 1, or render with pipeline 1)");
    f->pendingWave = wave; f->pendingCounters = p.collectStats != 0;
    f->pendingImagesK = k; f->pendingHdr = wantHdr; f->pendingAccum = p.accumulate != 0;
    memset(&f->stats, 0, sizeof f->stats);
    f->stats.localRows = rows; f->stats.localPixels = rows * p.width * n;
    f->viaBatch = false; f->pendingSplit = 0;
    /* The launch runs on THIS frame's stream.  What another stream still holds for one of its frames comes first: a launch the frame
     * led on its own stream (ownPending), or a batch on a third stream that wrote it (batchStream).  In steady state — the same
     * frames batched behind the same leader, or frames joined between uses — neither is set and nothing is enqueued here (cross-stream
     * waits on every launch cost 3 % of the frame rate at N = 1 and 25 % on a 1/8 shard: profiles/r03/ab_batch_stream_order.log). */
    if (f->batchStream && f->batchStream != st) HIP_TRY(hipStreamWaitEvent(st, f->evDone, 0));
    f->batchStream = nullptr;
    for (uint32_t b = 1; b < n; ++b) {
        rtr_frame* fr = frames[b];
        if (fr->ownPending && fr->ctx->stream != st) {
            if (!fr->evOwn) HIP_TRY(hipEventCreateWithFlags(&fr->evOwn, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(fr->evOwn, fr->ctx->stream));
            HIP_TRY(hipStreamWaitEvent(st, fr->evOwn, 0));
        }
        if (fr->batchStream && fr->batchStream != st) HIP_TRY(hipStreamWaitEvent(st, fr->evDone, 0));
    }
    hipError_t e;
    if (wave) {
        /* the list of rays left to the redo kernels: the camera rays' needs one entry per pixel-sample at most; the any-hit kernel's
         * gets 1/16 of the queue (at least 2^20 entries) and k_shadow_tail redoes the whole queue should that ever overflow */
        uint64_t ovCap = std::max<uint64_t>(std::max<uint64_t>(nPS, nRays / 16), 1ull << 20);
        if (ovCap > nRays) ovCap = std::max<uint64_t>(nRays, nPS);
        if (f->hitTuvp.n < nPS) { HIP_TRY(f->hitTuvp.alloc(nPS)); HIP_TRY(f->hitCustom.alloc(nPS)); HIP_TRY(f->rayOrigin.alloc(nPS)); }
        if (f->vis.n < nSlots) HIP_TRY(f->vis.alloc(nSlots));
        if (f->rayDT.n < nRays) { HIP_TRY(f->rayDT.alloc(nRays)); HIP_TRY(f->raySlot.alloc(nRays)); }
        /* every array is (re)sized by its OWN need: the redo list is also k_primary's (one entry per pixel-sample at most), and a
         * launch with fewer queries per sample but more samples than an earlier one needs a longer list with a shorter queue */
        if (f->overflow.n < ovCap + 1) HIP_TRY(f->overflow.alloc(ovCap + 1));
        f->overflowCap = (uint32_t)std::min<uint64_t>(ovCap, f->overflow.n - 1);      /* what the any-hit kernel may use of it */
#ifdef RTR_TEST_HOOKS
        if (const char* e = getenv("RTR_TRACE_OVERFLOW_CAP")) { const uint64_t v = strtoull(e, nullptr, 10); if (v >= 1 && v < f->overflowCap) f->overflowCap = (uint32_t)v; }   /* a list short enough to overflow */
#endif
        {   /* batch lists of the binned queue (octant x consumer XCD): a run's batches are dealt round-robin to the eight lists of
             * its octant, so a list holds at most 1/8 of one batch per 64 rays (the smallest batch) + one per k_shadow_gen_oct workgroup */
            const uint64_t ls = nRays / 64 / rtrdev::kQueueRegions + nPS / 256 + 16;
            if ((uint64_t)f->listStride < ls) { HIP_TRY(f->batchLists.alloc((size_t)ls * rtrdev::kQueueLists)); f->listStride = (uint32_t)ls; }
        }
        f->slotStride = (uint32_t)slotStride;
        if (!f->queueCount.p) HIP_TRY(f->queueCount.alloc(rtrdev::kQueueCtrlWords));
        if (!f->clk.p) { HIP_TRY(f->clk.alloc(2 * rtrdev::kQueueRegions)); HIP_TRY(hipMemsetAsync(f->clk.p, 0, 2 * rtrdev::kQueueRegions * sizeof(unsigned long long), st)); }
        if (!f->spill.p) HIP_TRY(f->spill.alloc(rtrdev::kSpillInts));      /* 64 entries x the redo kernels' grid */
        Workspace ws;
        ws.hitTuvp = f->hitTuvp.p; ws.hitCustom = f->hitCustom.p; ws.vis = f->vis.p; ws.visFill = f->visFill;
        ws.visPlaneBytes = (size_t)nPS; ws.visPlanes = (uint32_t)maxRays;      /* what a launch fills: the first nPS bytes of each of the maxRays planes, not the power-of-two pitch between them */
#ifdef RTR_TEST_HOOKS
        if (const char* e = getenv("RTR_TRACE_VIS_FILL")) if ((e[0] == '0' || e[0] == '1') && !e[1]) ws.visFill = (uint32_t)(e[0] - '0');      /* force the pre-fill */
#endif
        ws.rayQueue.dt = f->rayDT.p; ws.rayQueue.slot = f->raySlot.p; ws.rayQueue.origin = f->rayOrigin.p; ws.rayQueue.slotStride = f->slotStride; ws.rayQueue.slotMask = f->slotStride - 1u;
        ws.queueCount = f->queueCount.p; ws.capPixelSamples = nPS; ws.capRays = nRays; ws.spill = f->spill.p; ws.overflow = f->overflow.p; ws.overflowCap = f->overflowCap; ws.batchLists = f->batchLists.p; ws.listStride = f->listStride; ws.clk = f->clk.p;
        e = rtrdev::launch_wavefront(s->dev, fb, ws, f->ctx->tun, (int)s->tree.stats.stackEntries, dstats, st, f->ev, (uint32_t)f->ctx->prop.multiProcessorCount);
    } else {
        (void)hipEventRecord(f->evMega[0], st);
        e = rtrdev::launch_megakernel(s->dev, ra, fo, (int)s->tree.stats.stackEntries, dstats, st);
        (void)hipEventRecord(f->evMega[1], st);
    }
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    f->pendingStats = true;
    f->ownPending = true;
    /* ... and each of the other frames gets an event behind the launch: rtr_frame_wait / rtr_frame_download wait on it, and so does
     * the stream of whatever launch writes the frame next (above) */
    for (uint32_t b = 1; b < n; ++b) {
        rtr_frame* fr = frames[b];
        if (!fr->evDone) HIP_TRY(hipEventCreateWithFlags(&fr->evDone, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(fr->evDone, st));
        fr->batchStream = st;
        fr->viaBatch = true; fr->pendingStats = false;
        memset(&fr->stats, 0, sizeof fr->stats);
    }
    return RTR_OK;
}

int rtr_render_batch_limit(const rtr_scene* s, const rtr_render_params* pin, uint32_t numAreaLights, uint32_t* maxFrames) {
    if (!s || !pin || !maxFrames) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_limit: null argument");
    if (numAreaLights > s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_limit: %u area lights, the scene has %u", numAreaLights, s->numLights);
    rtr_render_params p = *pin;
    if (p.bandRows == 0) p.bandRows = 8;
    if (p.shardCount == 0) p.shardCount = 1;
    if (p.width == 0 || p.height == 0 || p.spp == 0 || p.bandRows % 8u) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_batch_limit: bad width/height/spp/bandRows");
    *maxFrames = 1;
    if (p.pipeline == 1) return RTR_OK;
    /* the arithmetic of enqueue_render() */
    uint64_t maxRays = 1;
    for (uint32_t l = 0; l < numAreaLights; ++l) maxRays += (uint64_t)s->hostLights[l].numTriangles * p.numShadowRays;
    const uint32_t rows = rtr_shard_rows(p.height, p.bandRows, p.shardCount);
    const uint64_t blocks = ((uint64_t)((rows + 7u) / 8u) * ((p.width + 7u) / 8u) * 64u + 255u) / 256u;
    for (uint32_t n = rtrdev::kMaxBatch; n > 1; --n) {
        const uint64_t nPS = blocks * 256u * p.spp * n;
        uint64_t slotStride = 256;
        while (slotStride < nPS) slotStride <<= 1;
        if (slotStride * maxRays < (1ull << 31) && maxRays <= 4096 && blocks * n < (1ull << 31)) { *maxFrames = n; break; }
    }
    return RTR_OK;
}

/* One frame as `parts` band-shards, each on a stream of its own, all writing their rows of the SAME images: the kernels of one frame
 * are a dependency chain and each ends in a tail, so part k+1's camera rays and queue build run under part k's traversal and its
 * traversal fills the tail of part k's — frames in flight, inside one frame. */
int rtr_render_split_async(rtr_scene* s, const RtrCameraData* cam, const RtrSceneInfo* info, const rtr_render_params* pin, rtr_frame* f, uint32_t parts) {
    if (!s || !cam || !info || !pin || !f) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: null argument");
    if (parts < 1 || parts > RTR_MAX_SPLIT) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: %u parts, 1 to %d", parts, RTR_MAX_SPLIT);
    if (pin->shardCount > 1) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: the frame must be whole (shardCount %u); a shard of a multi-GPU frame is not split again", pin->shardCount);
    if (f->extHdr) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: not a frame of the caller's");
    rtr_render_params p = *pin;
    if (p.bandRows == 0) p.bandRows = 8;
    if (p.bandRows % 8u) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: bandRows %u must be a multiple of 8", p.bandRows);
    if (p.height == 0 || p.width == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: empty frame");
    const uint32_t bands = (p.height + p.bandRows - 1) / p.bandRows;
    if (parts > bands) parts = bands;                 /* never a part without a band */
    if (parts <= 1) { p.shardIndex = 0; p.shardCount = 1; return enqueue_render(s, cam, info, &p, &f, 1); }
    if (f->width != p.width || f->rows != p.height) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_render_split_async: frame is %ux%u, the whole frame is %ux%u", f->width, f->rows, p.width, p.height);
    HIP_TRY(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    /* the parts: internal frame objects (scratch, events, counters; no images) on contexts (streams) of their own */
    while (f->parts.size() < parts) {
        rtr_ctx* pc = nullptr; rtr_frame* pf = nullptr;
        int rc = ctx_create_prio(f->ctx->device, f->ctx->tun.split_priorities ? (int)f->parts.size() : -1, &pc);
        if (rc != RTR_OK) return rc;
        rc = frame_new(pc, f->width, f->rows, f->images, false, &pf);
        if (rc != RTR_OK) { rtr_ctx_destroy(pc); return rc; }
        hipEvent_t ev = nullptr;
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) { rtr_frame_destroy(pf); rtr_ctx_destroy(pc); return fail(RTR_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e)); }
        f->partCtx.push_back(pc); f->parts.push_back(pf); f->evPart.push_back(ev);
    }
    for (auto& e : f->evSplit) if (!e) HIP_TRY(hipEventCreate(&e));
    /* what another stream still holds for this frame comes first (enqueue_render's rule) */
    if (f->batchStream && f->batchStream != st) HIP_TRY(hipStreamWaitEvent(st, f->evDone, 0));
    f->batchStream = nullptr;
    HIP_TRY(hipEventRecord(f->evSplit[0], st));          /* the fork */
    /* A failure inside the loop must not leave the frame's stream un-joined from parts that were already enqueued (a download, clear
     * or denoise that follows would race them, and rtr_frame_wait would never collect them): the error is kept, every part that WAS
     * enqueued is joined, the frame is marked pending for exactly those, and then the error is returned. */
    int rc = RTR_OK;
    uint32_t started = 0;
    auto hip_keep = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == RTR_OK) rc = fail(RTR_ERR_HIP, "rtr_render_split_async: %s: %s", what, hipGetErrorString(e));
        return e == hipSuccess;
    };
    for (uint32_t k = 0; k < parts && rc == RTR_OK; ++k) {
        rtr_frame* pf = f->parts[k];
        pf->ctx->tun = f->ctx->tun;
        pf->images = f->images;
        for (int i = 0; i < 8; ++i) pf->ext[i] = f->image_ptr(i);
        pf->extHdr = f->hdr.p;
        hipStream_t ps = pf->ctx->stream;
        if (!hip_keep(hipStreamWaitEvent(ps, f->evSplit[0], 0), "hipStreamWaitEvent (fork)")) break;
        p.shardIndex = k; p.shardCount = parts;
        const int prc = enqueue_render(s, cam, info, &p, &pf, 1, true);
        if (prc != RTR_OK) { rc = prc; break; }
        ++started;                                              /* from here on part k has work on its stream: it must be joined */
        if (hip_keep(hipEventRecord(f->evPart[k], ps), "hipEventRecord (part)")) hip_keep(hipStreamWaitEvent(st, f->evPart[k], 0), "hipStreamWaitEvent (join)");
        else hip_keep(hipStreamSynchronize(ps), "hipStreamSynchronize (join of last resort)");      /* no event to order behind: drain the part here */
    }
    hip_keep(hipEventRecord(f->evSplit[1], st), "hipEventRecord (join)");
    f->ownPending = true; f->viaBatch = false;
    f->pendingSplit = started; f->pendingStats = started != 0;
    return rc;
}

int rtr_render_split(rtr_scene* s, const RtrCameraData* cam, const RtrSceneInfo* info, const rtr_render_params* p, rtr_frame* f, uint32_t parts) {
    int rc = rtr_render_split_async(s, cam, info, p, f, parts);
    if (rc != RTR_OK) return rc;
    return rtr_frame_wait(f);
}

/* joins a split render and makes the frame's statistics out of its parts': counters and per-kernel times are SUMS over the parts (the
 * parts' kernels overlap: the sum of their durations exceeds the frame's), totalMs is the frame's own duration, fork to join */
static int wait_split(rtr_frame* f) {
    const uint32_t parts = f->pendingSplit;
    f->pendingSplit = 0; f->pendingStats = false;
    rtr_frame_stats t; memset(&t, 0, sizeof t);
    double clk = 0; uint32_t nclk = 0;
    for (uint32_t k = 0; k < parts; ++k) {
        int rc = rtr_frame_wait(f->parts[k]);
        if (rc != RTR_OK) return rc;
        const rtr_frame_stats& a = f->parts[k]->stats;
        t.numRays += a.numRays; t.numPrimaryRays += a.numPrimaryRays; t.numShadowRays += a.numShadowRays; t.numNodeVisits += a.numNodeVisits;
        t.numTriTests += a.numTriTests; t.numHits += a.numHits; t.numLightFetches += a.numLightFetches; t.numLightTriFetches += a.numLightTriFetches;
        t.numTexFetches += a.numTexFetches; t.numAlphaTests += a.numAlphaTests; t.algorithmicBytes += a.algorithmicBytes;
        t.numShadowNodeVisits += a.numShadowNodeVisits; t.numShadowTriTests += a.numShadowTriTests; t.shadowTraceBytes += a.shadowTraceBytes;
        t.primaryMs += a.primaryMs; t.shadowGenMs += a.shadowGenMs; t.shadowTraceMs += a.shadowTraceMs; t.resolveMs += a.resolveMs; t.shadowTailMs += a.shadowTailMs;
        t.localRows += a.localRows; t.localPixels += a.localPixels; t.pipelineUsed = a.pipelineUsed;
        t.shadowInnerIterations += a.shadowInnerIterations; t.shadowInnerActiveLanes += a.shadowInnerActiveLanes;
        t.shadowTriIterations += a.shadowTriIterations; t.shadowTriActiveLanes += a.shadowTriActiveLanes; t.shadowRefills += a.shadowRefills;
        t.primaryTailRays += a.primaryTailRays; t.shadowTailRays += a.shadowTailRays;
        if (a.shadowTraceClockMHz > 0.f) {
            clk += a.shadowTraceClockMHz; ++nclk;
            t.shadowTraceClockMinMHz = (t.shadowTraceClockMinMHz == 0.f || a.shadowTraceClockMinMHz < t.shadowTraceClockMinMHz) ? a.shadowTraceClockMinMHz : t.shadowTraceClockMinMHz;
            t.shadowTraceClockMaxMHz = a.shadowTraceClockMaxMHz > t.shadowTraceClockMaxMHz ? a.shadowTraceClockMaxMHz : t.shadowTraceClockMaxMHz;
        }
    }
    if (nclk) t.shadowTraceClockMHz = (float)(clk / nclk);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, f->evSplit[0], f->evSplit[1]);
    t.totalMs = ms;
    f->stats = t;
    return RTR_OK;
}

int rtr_frame_wait(rtr_frame* f) {
    if (!f) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_wait: null frame");
    HIP_TRY(hipSetDevice(f->ctx->device));
    HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    f->ownPending = false;
    if (f->pendingSplit) return wait_split(f);
    if (f->viaBatch) { HIP_TRY(hipEventSynchronize(f->evDone)); f->batchStream = nullptr; return RTR_OK; }      /* rendered in another frame's launch: that launch's times and counters are the leading frame's */
    if (!f->pendingStats) return RTR_OK;
    f->pendingStats = false;
    rtr_frame_stats& s = f->stats;
    if (f->pendingWave) {
        float a = 0, b = 0, c = 0, d = 0;
        (void)hipEventElapsedTime(&a, f->ev[0], f->ev[1]);
        (void)hipEventElapsedTime(&b, f->ev[1], f->ev[2]);
        (void)hipEventElapsedTime(&c, f->ev[2], f->ev[5]);
        float tail = 0;
        (void)hipEventElapsedTime(&tail, f->ev[5], f->ev[3]);
        s.shadowTailMs = tail;
        (void)hipEventElapsedTime(&d, f->ev[3], f->ev[4]);
        s.primaryMs = a; s.shadowGenMs = b; s.shadowTraceMs = c; s.resolveMs = d; s.totalMs = a + b + c + tail + d;
        s.pipelineUsed = 2;
        if (f->clk.p) {      /* shader clock held during the any-hit launch: s_memtime ticks over 100-MHz ticks of one wave per XCD; the MEAN over the XCDs — they clock
                              * independently (2.25 ... 2.40 GHz within one launch on a warm part) and the launch's vector-issue capacity is the sum of theirs */
            unsigned long long h[2 * rtrdev::kQueueRegions];
            HIP_TRY(hipMemcpy(h, f->clk.p, sizeof h, hipMemcpyDeviceToHost));
            float mhz[rtrdev::kQueueRegions]; int nv = 0;
            for (uint32_t r = 0; r < rtrdev::kQueueRegions; ++r) if (h[2 * r + 1]) mhz[nv++] = (float)((double)h[2 * r] / (double)h[2 * r + 1] * 100.0);
            for (int i = 1; i < nv; ++i) for (int j = i; j > 0 && mhz[j] < mhz[j - 1]; --j) { const float t = mhz[j]; mhz[j] = mhz[j - 1]; mhz[j - 1] = t; }
            double sum = 0; for (int i = 0; i < nv; ++i) sum += mhz[i];
            s.shadowTraceClockMHz = nv ? (float)(sum / nv) : 0.f;
            s.shadowTraceClockMinMHz = nv ? mhz[0] : 0.f; s.shadowTraceClockMaxMHz = nv ? mhz[nv - 1] : 0.f;
        }
        if (f->queueCount.p) {      /* the next launch pre-fills the visibility array with this one's commoner outcome */
            uint32_t q[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpy(q, f->queueCount.p, sizeof q, hipMemcpyDeviceToHost));
            if (q[0]) f->visFill = (2ull * q[3] >= q[0]) ? 1u : 0u;
        }
    } else {
        float a = 0;
        (void)hipEventElapsedTime(&a, f->evMega[0], f->evMega[1]);
        s.primaryMs = a; s.totalMs = a;
        s.pipelineUsed = 1;
    }
    if (f->pendingCounters) {
        Counters h;
        HIP_TRY(hipMemcpy(&h, f->counters.p, sizeof h, hipMemcpyDeviceToHost));
        s.numRays = h.rays; s.numPrimaryRays = h.primary; s.numShadowRays = h.shadow;
        s.numNodeVisits = h.nodes; s.numTriTests = h.tris; s.numHits = h.hits;
        s.numLightFetches = h.lightFetch; s.numLightTriFetches = h.lightTriFetch;
        s.numShadowNodeVisits = h.shadowNodes; s.numShadowTriTests = h.shadowTris;
        s.numTexFetches = h.texFetch; s.numAlphaTests = h.alphaTests;
        const uint64_t shadowNodeBytes = f->pendingWave ? RTR_WIDE_NODE_BYTES : RTR_BVH_NODE_BYTES;     /* the megakernel walks the BVH2 for its shadow rays too */
        s.shadowTraceBytes = shadowNodeBytes * h.shadowNodes + 48ull * h.shadowTris + 37ull * h.shadow;      /* per ray: 20 B of queue record + the 16-B origin of its pixel-sample + its visibility byte */
        s.shadowInnerIterations = h.innerIters; s.shadowInnerActiveLanes = h.innerLanes;
        s.shadowTriIterations = h.triIters; s.shadowTriActiveLanes = h.triLanes; s.shadowRefills = h.refills;
        if (f->overflow.p) { uint32_t ov = 0; HIP_TRY(hipMemcpy(&ov, f->overflow.p, sizeof ov, hipMemcpyDeviceToHost)); s.shadowTailRays = ov; }
        if (f->pendingWave && f->queueCount.p) { uint32_t rd = 0; HIP_TRY(hipMemcpy(&rd, f->queueCount.p + 2, sizeof rd, hipMemcpyDeviceToHost)); s.primaryTailRays = rd; }
        s.algorithmicBytes = (uint64_t)RTR_BVH_NODE_BYTES * (h.nodes - h.shadowNodes) + shadowNodeBytes * h.shadowNodes + 48ull * h.tris + 236ull * (h.hits + h.alphaTests) + 96ull * h.lightFetch + 156ull * h.lightTriFetch +
                             16ull * h.texFetch +
                             4ull * f->pendingImagesK * s.localPixels + (f->pendingHdr ? (f->pendingAccum ? 32ull : 16ull) * s.localPixels : 0ull);
    }
    return RTR_OK;
}

int rtr_render_async(rtr_scene* s, const RtrCameraData* cam, const RtrSceneInfo* info, const rtr_render_params* p, rtr_frame* f) {
    return enqueue_render(s, cam, info, p, &f, 1);
}

int rtr_render_batch_async(rtr_scene* s, const RtrCameraData* cams, const RtrSceneInfo* infos, const rtr_render_params* p, rtr_frame* const* frames, uint32_t n) {
    return enqueue_render(s, cams, infos, p, frames, n);
}

int rtr_render(rtr_scene* s, const RtrCameraData* cam, const RtrSceneInfo* info, const rtr_render_params* p, rtr_frame* f) {
    int rc = enqueue_render(s, cam, info, p, &f, 1);
    if (rc != RTR_OK) return rc;
    return rtr_frame_wait(f);
}

int rtr_frame_get_stats(const rtr_frame* f, rtr_frame_stats* out) {
    if (!f || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_frame_get_stats: null argument");
    *out = f->stats;
    return RTR_OK;
}

/* the checks, launches and ping-pong of rtr_denoise_combine, enqueued on the frame's context stream (behind a batch launch that wrote
 * the frame on another stream, and ahead of a later one: order_on_own_stream) */
static int enqueue_denoise_combine(rtr_frame* f, int iterations, const char* who) {
    if (!f) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null frame", who);
    if (iterations < 0 || iterations > 64) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: iterations %d", who, iterations);
    for (int i = 0; i < 8; ++i)
        if (!f->image_ptr(i)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the frame lacks image %d (create it with all of images 0-7)", who, i);
    HIP_TRY(hipSetDevice(f->ctx->device));
    { const int rc = order_on_own_stream(f); if (rc != RTR_OK) return rc; }
    hipStream_t st = f->ctx->stream;
    uint32_t* sh = f->image_ptr(RTR_IMAGE_SHADOWED); uint32_t* un = f->image_ptr(RTR_IMAGE_UNSHADOWED);
    uint32_t* dsh = f->image_ptr(RTR_IMAGE_DENOISED_SHADOWED); uint32_t* dun = f->image_ptr(RTR_IMAGE_DENOISED_UNSHADOWED);
    const uint32_t* nrm = f->image_ptr(RTR_IMAGE_NORMAL); const uint32_t* pos = f->image_ptr(RTR_IMAGE_POSITION);
    int denoisingOutput = 1;                                            /* application.cppm:392 */
    for (int i = 0; i < iterations; ++i) {
        const int step = (i + 1) * 1;                                   /* (i + 1) * DENOISING_STRENGTH */
        hipError_t e;
        if (denoisingOutput == 1) {
            e = rtrdev::launch_denoise_pair(un, dun, sh, dsh, nrm, pos, f->width, f->rows, step, 1.0f, 0.001f, 0.001f, st);
        } else {
            e = rtrdev::launch_denoise_pair(dun, un, dsh, sh, nrm, pos, f->width, f->rows, step, 1.0f, 0.001f, 0.001f, st);
        }
        if (e != hipSuccess) return fail(RTR_ERR_HIP, "denoise launch: %s", hipGetErrorString(e));
        denoisingOutput = 1 - denoisingOutput;
    }
    hipError_t e = rtrdev::launch_combine(f->image_ptr(RTR_IMAGE_ANALYTIC), denoisingOutput == 0 ? sh : dsh, denoisingOutput == 0 ? un : dun,
                                          f->image_ptr(RTR_IMAGE_FINAL), f->width, f->rows, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "combine launch: %s", hipGetErrorString(e));
    return RTR_OK;
}

int rtr_denoise_combine(rtr_frame* f, int iterations) {
    const int rc = enqueue_denoise_combine(f, iterations, "rtr_denoise_combine");
    if (rc != RTR_OK) return rc;
    HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return RTR_OK;
}

int rtr_denoise_combine_async(rtr_frame* f, int iterations) {
    return enqueue_denoise_combine(f, iterations, "rtr_denoise_combine_async");     /* rtr_frame_wait joins */
}

int rtr_deinterleave_bands(rtr_ctx* ctx, const void* gathered, void* dst, uint32_t width, uint32_t height, uint32_t bandRows, uint32_t shardCount) {
    if (!ctx || !gathered || !dst || width == 0 || height == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_bands: bad argument");
    if (bandRows == 0) bandRows = 8;
    if (shardCount == 0) shardCount = 1;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t localRows = rtr_shard_rows(height, bandRows, shardCount);
    hipError_t e = rtrdev::launch_deinterleave((const uint32_t*)gathered, (uint32_t*)dst, width, height, bandRows, shardCount, localRows, ctx->stream);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "deinterleave launch: %s", hipGetErrorString(e));
    return RTR_OK;   /* enqueued on the ctx stream; the caller synchronises (stream order is enough for a following copy) */
}

int rtr_deinterleave_images(rtr_ctx* ctx, const void* gathered, uint32_t numImages, void* const* dst, uint32_t width, uint32_t height,
                            uint32_t bandRows, uint32_t shardCount) {
    if (!ctx || !gathered || !dst || width == 0 || height == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_images: bad argument");
    if (numImages == 0 || numImages > rtrdev::kMaxDeinterleaveImages) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_images: %u images, 1 to %u", numImages, rtrdev::kMaxDeinterleaveImages);
    for (uint32_t i = 0; i < numImages; ++i) if (!dst[i]) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_images: destination %u is null", i);
    if (bandRows == 0) bandRows = 8;
    if (bandRows % 8u) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_deinterleave_images: bandRows %u is not a multiple of 8", bandRows);
    if (shardCount == 0) shardCount = 1;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t localRows = rtr_shard_rows(height, bandRows, shardCount);
    uint32_t* d[rtrdev::kMaxDeinterleaveImages];
    for (uint32_t i = 0; i < numImages; ++i) d[i] = static_cast<uint32_t*>(dst[i]);
    hipError_t e = rtrdev::launch_deinterleave_images(static_cast<const uint32_t*>(gathered), d, numImages, width, height, bandRows, shardCount, localRows, ctx->stream);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "deinterleave launch: %s", hipGetErrorString(e));
    return RTR_OK;   /* enqueued on the ctx stream, like rtr_deinterleave_bands */
}

/* ---- ray queries ---------------------------------------------------------------------------- */
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
/* the pointer tables and the params' rules of rtr_arg_check.h, which the rtr_*_host.cpp share */
using rtrdev::Arg;
using rtrdev::check_ptrs;

/* the handles every call of this section takes, and the device they must share */
static int check_handles(const rtr_ctx* c, const rtr_scene* s, const char* who) {
    if (!c || !s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null context or scene", who);
    return RTR_OK;
}
static int check_same_device(const rtr_ctx* c, const rtr_scene* s, const char* who) {
    if (s->ctx->device != c->device) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene lives on device %d, the context on device %d", who, s->ctx->device, c->device);
    return RTR_OK;
}
/* a synchronous call joins the context's stream when its asynchronous form (rc) enqueued something */
static int join_if_enqueued(rtr_ctx* c, int rc, uint32_t n) {
    if (rc != RTR_OK || n == 0) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RTR_OK;
}

/* the context's query scratch, allocated by its first query (the current device is the context's) */
static int query_scratch(rtr_ctx* c) {
    if (c->qCtrl.p) return RTR_OK;
    HIP_TRY(c->qRedo.alloc(rtrdev::kQueryRedoCap));
    HIP_TRY(c->qSpill.alloc(rtrdev::kSpillInts));
    HIP_TRY(c->qCounters.alloc(1));
    for (hipEvent_t& e : c->qEv) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(c->qCtrl.alloc(rtrdev::kQueryCtrlWords));
    return RTR_OK;
}

/* Every query that walks rays (rtr_trace_rays, rtr_trace_rays_multi, rtr_trace_occlusion and their forms) goes through that scratch the
 * same way: scratch_open, its own memsets, qEv[0], its launches, scratch_close; the counting form reads back in query_join. */

/* entries of a redo list of cap entries the query may use: all of them, or in the test build a list short enough to overflow */
static uint32_t redo_cap(uint32_t cap) {
#ifdef RTR_TEST_HOOKS
    if (const char* e = getenv("RTR_QUERY_REDO_CAP")) { const uint64_t v = strtoull(e, nullptr, 10); if (v >= 1 && v < cap) cap = (uint32_t)v; }
#endif
    return cap;
}

/* The scratch is the context's — redo list, deep stacks, counters, events — so a query enqueued on another stream than the last one
 * (rtr_ctx_set_stream) comes behind it.  count: the counting form, whose counters start at zero. */
static int scratch_open(rtr_ctx* c, bool count) {
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = query_scratch(c)) return rc;
    hipStream_t st = c->stream;
    if (c->qLastStream && c->qLastStream != st) HIP_TRY(hipStreamWaitEvent(st, c->qEv[1], 0));
    if (count) HIP_TRY(hipMemsetAsync(c->qCounters.p, 0, sizeof(Counters), st));
    return RTR_OK;
}

/* launch: what the query's launcher returned */
static int scratch_close(rtr_ctx* c, hipError_t launch, const char* who) {
    if (const int rc = launched(launch, who)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(hipEventRecord(c->qEv[1], st));
    c->qLastStream = st;
    return RTR_OK;
}

/* the cull mask of the masked calls: NoMask for the unmasked ones, which launch the kernels' unmasked forms */
struct CullMask { bool masked; const uint8_t* rayMasks; uint32_t cullMask; };
static const CullMask NoMask{false, nullptr, 0xffu};

/* the flags argument of every query entry point: the known bits, and the combinations Vulkan forbids (VUID-RayFlags: one face flag at
 * most; one of Opaque, CullOpaque, CullNoOpaque at most) */
static const uint32_t kQueryCullFlags = RTR_QUERY_CULL_BACK_FACING | RTR_QUERY_CULL_FRONT_FACING | RTR_QUERY_CULL_OPAQUE | RTR_QUERY_CULL_NO_OPAQUE;
static int check_query_flags(uint32_t flags, const char* who) {
    const uint32_t known = RTR_QUERY_ANY | RTR_QUERY_OPAQUE | kQueryCullFlags;
    if (flags & ~known) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", who, flags & ~known);
    if ((flags & RTR_QUERY_CULL_BACK_FACING) && (flags & RTR_QUERY_CULL_FRONT_FACING))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: flags RTR_QUERY_CULL_BACK_FACING and RTR_QUERY_CULL_FRONT_FACING exclude each other", who);
    const uint32_t op = flags & (RTR_QUERY_OPAQUE | RTR_QUERY_CULL_OPAQUE | RTR_QUERY_CULL_NO_OPAQUE);
    if (op & (op - 1u))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: flags%s%s%s exclude each other (at most one of RTR_QUERY_OPAQUE, RTR_QUERY_CULL_OPAQUE, RTR_QUERY_CULL_NO_OPAQUE)", who,
                    (op & RTR_QUERY_OPAQUE) ? " RTR_QUERY_OPAQUE" : "", (op & RTR_QUERY_CULL_OPAQUE) ? " RTR_QUERY_CULL_OPAQUE" : "",
                    (op & RTR_QUERY_CULL_NO_OPAQUE) ? " RTR_QUERY_CULL_NO_OPAQUE" : "");
    return RTR_OK;
}
/* what the kernels get: a call with culling flags launches the MASKED forms — with the mask 0xff and no per-ray bytes when it brought no
 * cull mask — and hands them the flags beside the selecting bit; a call without launches what it always did */
static rtrdev::RayMaskArgs ray_mask_args(const CullMask& cm, uint32_t flags) {
    rtrdev::RayMaskArgs rm;
    const uint32_t cull = flags & kQueryCullFlags;
    rm.rayMasks = cm.masked ? cm.rayMasks : nullptr; rm.cullMask = cm.masked ? cm.cullMask : 0xffu;
    rm.masked = (cm.masked || cull) ? (1u | cull) : 0u;
    return rm;
}

/* what the three kinds of query check first, in this order: the handles, the cull mask's range, the flags */
static int check_query(const rtr_ctx* c, const rtr_scene* s, const CullMask& cm, uint32_t flags, const char* who) {
    if (const int rc = check_handles(c, s, who)) return rc;
    if (cm.masked && (cm.cullMask & ~0xffu)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: cullMask 0x%x has bits above the low 8 (an instance mask is 8 bits)", who, cm.cullMask);
    return check_query_flags(flags, who);
}

/* the checks and launches of rtr_trace_rays[_async], enqueued on the context's stream; count: the counting form */
static int enqueue_query(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, RtrHit* hits, uint8_t* occluded,
                         bool count, const char* who, const CullMask& cm = NoMask) {
    if (const int rc = check_query(c, s, cm, flags, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    const bool any = (flags & RTR_QUERY_ANY) != 0u;
    if (!rays) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: rays is null", who);
    if (!aligned16(rays)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: rays is not 16-B aligned", who);
    if (!any && !hits) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: a closest-hit query needs hits", who);
    if (!any && !aligned16(hits)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: hits is not 16-B aligned", who);
    if (any && !occluded) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: an any-hit query (RTR_QUERY_ANY) needs occluded", who);
    if (any && !aligned16(occluded)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: occluded is not 16-B aligned", who);
    if (const int rc = scratch_open(c, count)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(c->qCtrl.p, 0, rtrdev::kQueryCtrlWords * sizeof(uint32_t), st));
    HIP_TRY(hipEventRecord(c->qEv[0], st));
    rtrdev::QueryArgs qa{};
    qa.rays = reinterpret_cast<const float4*>(rays); qa.hits = reinterpret_cast<float4*>(hits); qa.occluded = occluded; qa.n = n;
    qa.redoCap = redo_cap(rtrdev::kQueryRedoCap); qa.ctrl = c->qCtrl.p; qa.redoList = c->qRedo.p; qa.spill = c->qSpill.p;
    const rtrdev::RayMaskArgs rm = ray_mask_args(cm, flags);
    return scratch_close(c, rtrdev::launch_query(s->dev, qa, flags & (RTR_QUERY_ANY | RTR_QUERY_OPAQUE), count ? c->qCounters.p : nullptr, st, rm), who);
}

/* ---- queued occlusion queries (kernels/rtr_occlusion.hip): the layout of the caller's scratch ---- */
namespace {
/* the caller's scratch: control block (zeroed with the count of abandoned rays behind it) | abandoned rays' list | index queue | batch lists */
struct OcclusionLayout { size_t ctrl, overflow, queue, lists, bytes; uint32_t overflowCap, listStride; };
size_t up16(size_t x) { return (x + 15u) & ~(size_t)15u; }
OcclusionLayout occlusion_layout(uint32_t n) {
    OcclusionLayout l{};
    l.overflowCap = n < rtrdev::kQueryRedoCap ? n : rtrdev::kQueryRedoCap;
    l.listStride = rtrdev::occlusion_list_stride(n);
    l.ctrl = 0;
    l.overflow = up16(rtrdev::kQueueCtrlWords * sizeof(uint32_t));
    l.queue = l.overflow + up16(((size_t)l.overflowCap + 1u) * sizeof(uint32_t));
    l.lists = l.queue + up16((size_t)n * sizeof(uint32_t));
    l.bytes = l.lists + up16((size_t)rtrdev::kQueueLists * l.listStride * sizeof(uint2));
    return l;
}
}  // namespace

/* What a synchronous query does behind its asynchronous form (rc: what that returned): it joins the context's stream, and the counting
 * form reads back the counters, the count of abandoned rays and the time between the two events — copies on the context's stream, so the
 * call joins that stream only.  occlusionScratch: the caller's scratch of a queued occlusion query, which keeps that count behind its
 * control block; null: the count is the context's control word. */
static int query_join(rtr_ctx* c, int rc, uint32_t n, rtr_query_stats* stats, const void* occlusionScratch = nullptr) {
    if (rc != RTR_OK) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return RTR_OK;
    hipStream_t st = c->stream;
    if (stats) {
        Counters h;
        uint32_t tail = 0;
        const void* tailWord = c->qCtrl.p + rtrdev::kQueryRedoWord;
        if (occlusionScratch) tailWord = static_cast<const char*>(occlusionScratch) + occlusion_layout(n).overflow;
        HIP_TRY(hipMemcpyAsync(&h, c->qCounters.p, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&tail, tailWord, sizeof tail, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        stats->numRays = h.rays; stats->numNodeVisits = h.nodes; stats->numTriTests = h.tris; stats->numAlphaTests = h.alphaTests;
        stats->tailRays = tail;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->qEv[0], c->qEv[1]));
        stats->ms = ms;
    } else HIP_TRY(hipStreamSynchronize(st));
    return RTR_OK;
}

int rtr_trace_rays_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, RtrHit* hits, uint8_t* occluded) {
    return enqueue_query(c, s, rays, n, flags, hits, occluded, false, "rtr_trace_rays_async");
}

int rtr_trace_rays(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, RtrHit* hits, uint8_t* occluded, rtr_query_stats* stats) {
    return query_join(c, enqueue_query(c, s, rays, n, flags, hits, occluded, stats != nullptr, "rtr_trace_rays"), n, stats);
}

int rtr_trace_rays_masked_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t flags, uint32_t cullMask,
                                RtrHit* hits, uint8_t* occluded) {
    return enqueue_query(c, s, rays, n, flags, hits, occluded, false, "rtr_trace_rays_masked_async", CullMask{true, rayMasks, cullMask});
}

int rtr_trace_rays_masked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t flags, uint32_t cullMask,
                          RtrHit* hits, uint8_t* occluded, rtr_query_stats* stats) {
    return query_join(c, enqueue_query(c, s, rays, n, flags, hits, occluded, stats != nullptr, "rtr_trace_rays_masked", CullMask{true, rayMasks, cullMask}), n, stats);
}

/* ---- multi-hit queries (kernels/rtr_multihit.hip) ---- */
/* the checks and launches of rtr_trace_rays_multi[_async], enqueued on the context's stream; count: the counting form.  The flag and mask
 * validation is the masked query's; the kernels have the filtered form only, so the call always brings a cull mask. */
static int enqueue_multihit(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t maxHits, uint32_t flags,
                            uint32_t cullMask, const RtrHit* after, RtrHit* hits, uint32_t* counts, bool count, const char* who) {
    const CullMask cm{true, rayMasks, cullMask};
    if (const int rc = check_query(c, s, cm, flags, who)) return rc;
    if (flags & RTR_QUERY_ANY) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: RTR_QUERY_ANY is refused: an any-hit walk has no order to report hits in", who);
    if (maxHits == 0u || maxHits > RTR_MULTIHIT_MAX) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: maxHits %u, 1 to %u", who, maxHits, RTR_MULTIHIT_MAX);
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    const Arg args[4] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, {after, "after", 16, false}, {counts, "counts", 4, false}};
    if (const int rc = check_ptrs(who, args)) return rc;
    if (const int rc = scratch_open(c, count)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(c->qCtrl.p, 0, rtrdev::kQueryCtrlWords * sizeof(uint32_t), st));
    HIP_TRY(hipEventRecord(c->qEv[0], st));
    rtrdev::MultiHitArgs ma{};
    ma.rays = reinterpret_cast<const float4*>(rays); ma.after = reinterpret_cast<const float4*>(after); ma.hits = reinterpret_cast<float4*>(hits);
    ma.counts = counts; ma.n = n; ma.maxHits = maxHits;
    ma.redoCap = redo_cap(rtrdev::kQueryRedoCap); ma.ctrl = c->qCtrl.p; ma.redoList = c->qRedo.p; ma.spill = c->qSpill.p;
    const rtrdev::RayMaskArgs rm = ray_mask_args(cm, flags);
    return scratch_close(c, rtrdev::launch_multihit(s->dev, ma, (flags & RTR_QUERY_OPAQUE) == 0u, count ? c->qCounters.p : nullptr, st, rm), who);
}

int rtr_trace_rays_multi_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t maxHits, uint32_t flags,
                               uint32_t cullMask, const RtrHit* after, RtrHit* hits, uint32_t* counts) {
    return enqueue_multihit(c, s, rays, rayMasks, n, maxHits, flags, cullMask, after, hits, counts, false, "rtr_trace_rays_multi_async");
}

int rtr_trace_rays_multi(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const uint8_t* rayMasks, uint32_t n, uint32_t maxHits, uint32_t flags,
                         uint32_t cullMask, const RtrHit* after, RtrHit* hits, uint32_t* counts, rtr_query_stats* stats) {
    return query_join(c, enqueue_multihit(c, s, rays, rayMasks, n, maxHits, flags, cullMask, after, hits, counts, stats != nullptr, "rtr_trace_rays_multi"), n, stats);
}

/* ---- queued occlusion queries (kernels/rtr_occlusion.hip) ---- */
int rtr_occlusion_scratch_bytes(uint32_t numRays, size_t* bytes) {
    if (!bytes) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_occlusion_scratch_bytes: bytes is null");
    *bytes = occlusion_layout(numRays).bytes;
    return RTR_OK;
}

/* startLeaves: the hints of rtr_trace_occlusion_hinted (null: none; the unhinted calls pass null) */
static int enqueue_occlusion(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, uint32_t n, uint32_t flags, void* scratch,
                             size_t scratchBytes, uint8_t* occluded, bool count, const char* who, const CullMask& cm = NoMask) {
    if (n && !aligned4(startLeaves)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: startLeaves is not 4-B aligned", who);
    if (const int rc = check_query(c, s, cm, flags, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    const Arg args[3] = {{rays, "rays", 16, true}, {occluded, "occluded", 16, true}, {scratch, "scratch", 16, true}};
    if (const int rc = check_ptrs(who, args)) return rc;
    const OcclusionLayout l = occlusion_layout(n);
    if (scratchBytes < l.bytes) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %zu bytes of scratch, %u rays need %zu (rtr_occlusion_scratch_bytes)", who, scratchBytes, n, l.bytes);
    if (const int rc = scratch_open(c, count)) return rc;      /* the deep stacks and the counters are the context's */
    hipStream_t st = c->stream;
    char* const base = static_cast<char*>(scratch);
    HIP_TRY(hipMemsetAsync(base + l.ctrl, 0, l.overflow + 16u, st));       /* the control block and the count of abandoned rays */
    HIP_TRY(hipMemsetAsync(occluded, 0, n, st));                           /* the walk stores the occluded rays' bytes only */
    HIP_TRY(hipEventRecord(c->qEv[0], st));
    rtrdev::OcclusionArgs oa{};
    oa.rays = reinterpret_cast<const float4*>(rays); oa.occluded = occluded; oa.n = n; oa.batch = rtrdev::occlusion_batch(n);
    oa.ctrl = reinterpret_cast<uint32_t*>(base + l.ctrl); oa.overflow = reinterpret_cast<uint32_t*>(base + l.overflow); oa.overflowCap = redo_cap(l.overflowCap);
    oa.queue = reinterpret_cast<uint32_t*>(base + l.queue); oa.lists = reinterpret_cast<uint2*>(base + l.lists); oa.listStride = l.listStride;
    oa.startLeaves = startLeaves; oa.numTris = (uint32_t)(s->tree.tris.n / 3);          /* a hint is checked against the records the scene holds */
    const rtrdev::RayMaskArgs rm = ray_mask_args(cm, flags);
    return scratch_close(c, rtrdev::launch_occlusion(s->dev, oa, c->tun, (flags & RTR_QUERY_OPAQUE) == 0u, c->qSpill.p, count ? c->qCounters.p : nullptr, st,
                                                     (uint32_t)c->prop.multiProcessorCount, rm), who);
}

int rtr_trace_occlusion_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, void* scratch, size_t scratchBytes, uint8_t* occluded) {
    return enqueue_occlusion(c, s, rays, nullptr, n, flags, scratch, scratchBytes, occluded, false, "rtr_trace_occlusion_async");
}

int rtr_trace_occlusion_hinted_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, uint32_t n, uint32_t flags, void* scratch,
                                     size_t scratchBytes, uint8_t* occluded) {
    return enqueue_occlusion(c, s, rays, startLeaves, n, flags, scratch, scratchBytes, occluded, false, "rtr_trace_occlusion_hinted_async");
}

int rtr_trace_occlusion_masked_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, const uint8_t* rayMasks, uint32_t n,
                                     uint32_t flags, uint32_t cullMask, void* scratch, size_t scratchBytes, uint8_t* occluded) {
    return enqueue_occlusion(c, s, rays, startLeaves, n, flags, scratch, scratchBytes, occluded, false, "rtr_trace_occlusion_masked_async", CullMask{true, rayMasks, cullMask});
}

int rtr_trace_occlusion_masked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, const uint8_t* rayMasks, uint32_t n,
                               uint32_t flags, uint32_t cullMask, void* scratch, size_t scratchBytes, uint8_t* occluded, rtr_query_stats* stats) {
    return query_join(c, enqueue_occlusion(c, s, rays, startLeaves, n, flags, scratch, scratchBytes, occluded, stats != nullptr, "rtr_trace_occlusion_masked",
                                           CullMask{true, rayMasks, cullMask}), n, stats, scratch);
}

int rtr_trace_occlusion(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, uint32_t n, uint32_t flags, void* scratch, size_t scratchBytes, uint8_t* occluded,
                        rtr_query_stats* stats) {
    return query_join(c, enqueue_occlusion(c, s, rays, nullptr, n, flags, scratch, scratchBytes, occluded, stats != nullptr, "rtr_trace_occlusion"), n, stats, scratch);
}

int rtr_trace_occlusion_hinted(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const int32_t* startLeaves, uint32_t n, uint32_t flags, void* scratch,
                               size_t scratchBytes, uint8_t* occluded, rtr_query_stats* stats) {
    return query_join(c, enqueue_occlusion(c, s, rays, startLeaves, n, flags, scratch, scratchBytes, occluded, stats != nullptr, "rtr_trace_occlusion_hinted"), n, stats, scratch);
}

/* the checks and the launch of rtr_hit_surfaces[_async], enqueued on the context's stream */
static int enqueue_surfaces(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, RtrSurface* out, const char* who) {
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    const Arg args[3] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, {out, "out", 16, true}};
    if (const int rc = check_ptrs(who, args)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::SurfaceArgs sa{};
    sa.rays = reinterpret_cast<const float4*>(rays); sa.hits = reinterpret_cast<const float4*>(hits); sa.out = reinterpret_cast<float4*>(out);
    sa.triCount = s->triCount.p; sa.numInstances = s->numInstances; sa.n = n;
    return launched(rtrdev::launch_hit_surfaces(s->dev, sa, c->stream), who);
}

int rtr_hit_surfaces_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, RtrSurface* out) {
    return enqueue_surfaces(c, s, rays, hits, n, out, "rtr_hit_surfaces_async");
}

int rtr_hit_surfaces(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, RtrSurface* out) {
    return join_if_enqueued(c, enqueue_surfaces(c, s, rays, hits, n, out, "rtr_hit_surfaces"), n);
}

/* ---- start hints: the triangle -> leaf table (kernels/rtr_query.hip: k_leaf_table) ---- */
/* Made by the first call that needs it, on the calling context's stream (the current device is the scene's), and JOINED before the call
 * goes on: whichever context of the device asks next finds it complete, without an event to wait for.  rtr_scene_update_instances
 * keeps it (a refit moves boxes and records, not the leaves they sit in). */
static int ensure_leaf_table(rtr_ctx* c, const rtr_scene* s, const char* who) {
    const SceneTree& t = s->tree;
    if (t.leafReady) return RTR_OK;
    { const int rcm = refresh_mirrors(s); if (rcm != RTR_OK) return rcm; }      /* joins an enqueued refit: this kernel may run on another stream */
    std::vector<uint32_t> base(s->hostTriCount.size() + 1, 0u);
    uint64_t total = 0;
    for (size_t i = 0; i < s->hostTriCount.size(); ++i) { base[i] = (uint32_t)total; total += s->hostTriCount[i]; }
    if (total > 0xffffffffull) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %llu (customIndex, primitiveId) pairs do not fit the leaf table's 32-bit index", who, (unsigned long long)total);
    hipStream_t st = c->stream;
    HIP_TRY(s->leafBase.upload(base.data(), base.size(), st));
    HIP_TRY(t.leafTable.alloc((size_t)total));
    HIP_TRY(hipMemsetAsync(t.leafTable.p, 0, t.leafTable.n * sizeof(int32_t), st));
    const hipError_t e = rtrdev::launch_leaf_table(t.nodes.p, (uint32_t)(t.nodes.n / 2), t.tris.p, (uint32_t)(t.tris.n / 3), s->triCount.p, s->leafBase.p,
                                                   s->numInstances, t.leafTable.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: leaf table: %s", who, hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    t.leafReady = true;
    return RTR_OK;
}

/* the checks and the launch of rtr_hit_leaves[_async].  The pointers are checked first: that needs nothing of the handles */
static int enqueue_hit_leaves(rtr_ctx* c, const rtr_scene* s, const RtrHit* hits, uint32_t n, int32_t* leaves, const char* who) {
    const Arg args[2] = {{hits, "hits", 16, true}, {leaves, "leaves", 4, true}};
    if (const int rc = n ? check_ptrs(who, args) : RTR_OK) return rc;
    if (const int hrc = check_handles(c, s, who)) return hrc;
    if (const int drc = check_same_device(c, s, who)) return drc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const int rc = ensure_leaf_table(c, s, who);
    if (rc != RTR_OK) return rc;
    rtrdev::LeafArgs a{};
    a.hits = reinterpret_cast<const float4*>(hits); a.leaves = leaves; a.triCount = s->triCount.p; a.base = s->leafBase.p; a.table = s->tree.leafTable.p;
    a.numInstances = s->numInstances; a.n = n;
    return launched(rtrdev::launch_hit_leaves(a, c->stream), who);
}

int rtr_hit_leaves_async(rtr_ctx* c, const rtr_scene* s, const RtrHit* hits, uint32_t n, int32_t* leaves) {
    return enqueue_hit_leaves(c, s, hits, n, leaves, "rtr_hit_leaves_async");
}

int rtr_hit_leaves(rtr_ctx* c, const rtr_scene* s, const RtrHit* hits, uint32_t n, int32_t* leaves) {
    return join_if_enqueued(c, enqueue_hit_leaves(c, s, hits, n, leaves, "rtr_hit_leaves"), n);
}

int rtr_camera_rays_async(rtr_ctx* c, const RtrCameraData* cam, uint32_t width, uint32_t height, uint32_t spp, RtrRay* out) {
    if (!c || !cam || !out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_camera_rays_async: null argument");
    if (!aligned16(out)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_camera_rays_async: out is not 16-B aligned");
    if (width == 0 || height == 0 || spp == 0) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_camera_rays_async: extent %ux%u x %u spp", width, height, spp);
    if ((uint64_t)width * height * spp > 0xffffffffull) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_camera_rays_async: %ux%u x %u spp is more than 2^32 - 1 rays", width, height, spp);
    HIP_TRY(hipSetDevice(c->device));
    return launched(rtrdev::launch_camera_rays(*cam, width, height, spp, reinterpret_cast<float4*>(out), c->stream), "rtr_camera_rays_async");
}

/* ---- direct lighting for ray-query hits -------------------------------------------------------------------------------------- */

/* Q of rtr_light_slots, from the host copy of the light table (as enqueue_render counts maxRaysPerSample) */
static int light_slots(const rtr_scene* s, const rtr_light_params* p, uint32_t* q, const char* who) {
    if (!s || !p) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene or params", who);
    if (p->numAreaLights > s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: numAreaLights %u > scene lights %u", who, p->numAreaLights, s->numLights);
    if (const int rc = rtrdev::check_shadow_rays(who, p->numShadowRays)) return rc;
    if (const int rc = rtrdev::check_light_outputs(who, p->outputs)) return rc;
    uint64_t slots = 1;
    for (uint32_t l = 0; l < p->numAreaLights; ++l) slots += (uint64_t)s->hostLights[l].numTriangles * p->numShadowRays;
    if (slots > 0xffffffffull) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %llu slots per hit do not fit 32 bits", who, (unsigned long long)slots);
    *q = (uint32_t)slots;
    return RTR_OK;
}

int rtr_light_slots(const rtr_scene* s, const rtr_light_params* p, uint32_t* slotsPerHit) {
    if (!slotsPerHit) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_light_slots: slotsPerHit is null");
    return light_slots(s, p, slotsPerHit, "rtr_light_slots");
}

/* what every lighting launch takes of the call alike; slots, the output arrays, the hint fields and the test hook are the caller's */
static void fill_light_args(rtrdev::LightArgs& la, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                            const uint32_t* seeds) {
    la.rays = reinterpret_cast<const float4*>(rays); la.hits = reinterpret_cast<const float4*>(hits); la.seeds = seeds;
    la.triCount = s->triCount.p; la.numInstances = s->numInstances; la.n = n;
    la.numAreaLights = p->numAreaLights; la.numShadowRays = p->numShadowRays; la.frame = p->frame; la.width = p->width; la.spp = p->spp;
    la.outputs = p->outputs;
}

/* the checks and the launch of rtr_light_rays[_async] (shade == false) and rtr_shade_hits[_async], enqueued on the context's stream */
static int enqueue_light(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                         const uint32_t* seeds, RtrRay* outRays, const uint8_t* occluded, RtrRadiance* out, bool shade, const char* who,
                         int32_t* outLeaves = nullptr, bool hinted = false) {
    const Arg own[1] = {{outLeaves, "outLeaves", 4, true}};       /* rtr_light_rays_hinted: its own array is checked first, which needs nothing of the handles */
    if (const int rc = hinted && n ? check_ptrs(who, own) : RTR_OK) return rc;
    if (!c || !s || !p) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null context, scene or params", who);
    if (const int rc = check_same_device(c, s, who)) return rc;
    uint32_t slots = 0;
    if (const int rc = light_slots(s, p, &slots, who)) return rc;
    if (shade && (p->outputs & RTR_LIGHT_ANALYTIC) && !s->hasLtc) return fail(RTR_ERR_UNSUPPORTED, "%s: RTR_LIGHT_ANALYTIC needs the LTC tables (rtr_scene_desc.ltc1/ltc2)", who);
    if (n == 0) return RTR_OK;
    if (const int rc = rtrdev::check_fits_32(who, n, "hits", slots, "slots")) return rc;
    const Arg args[5] = {{rays, "rays", 16, true}, {hits, "hits", 16, true}, shade ? Arg{out, "out", 16, true} : Arg{outRays, "outRays", 16, true},
                         {occluded, "occluded", 1, shade}, {seeds, "seeds", 4, false}};
    if (const int rc = check_ptrs(who, args)) return rc;
    if (const int rc = rtrdev::check_pixel_seeds(who, seeds, p->width, p->spp)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = hinted ? ensure_leaf_table(c, s, who) : RTR_OK) return rc;
    rtrdev::LightArgs la{};
    if (hinted) { la.outLeaves = outLeaves; la.leafTable = s->tree.leafTable.p; la.leafBase = s->leafBase.p; }
    fill_light_args(la, s, rays, hits, n, p, seeds);
    la.slots = slots;
    la.outRays = reinterpret_cast<float4*>(outRays); la.occluded = occluded; la.out = reinterpret_cast<float4*>(out);
#ifdef RTR_TEST_HOOKS
    if (const char* e = getenv("RTR_LIGHT_RAYS_DIRECT")) la.direct = atoi(e) != 0 ? 1u : 0u;   /* the kernel's unstaged form for a light table that would be staged */
#endif
    return launched(shade ? rtrdev::launch_shade_hits(s->dev, la, c->stream) : rtrdev::launch_light_rays(s->dev, la, c->stream), who);
}

int rtr_light_rays_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                         const uint32_t* seeds, RtrRay* outRays) {
    return enqueue_light(c, s, rays, hits, n, p, seeds, outRays, nullptr, nullptr, false, "rtr_light_rays_async");
}

int rtr_light_rays(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                   const uint32_t* seeds, RtrRay* outRays) {
    return join_if_enqueued(c, enqueue_light(c, s, rays, hits, n, p, seeds, outRays, nullptr, nullptr, false, "rtr_light_rays"), n);
}

int rtr_light_rays_hinted_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                const uint32_t* seeds, RtrRay* outRays, int32_t* outLeaves) {
    return enqueue_light(c, s, rays, hits, n, p, seeds, outRays, nullptr, nullptr, false, "rtr_light_rays_hinted_async", outLeaves, true);
}

int rtr_light_rays_hinted(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                          const uint32_t* seeds, RtrRay* outRays, int32_t* outLeaves) {
    return join_if_enqueued(c, enqueue_light(c, s, rays, hits, n, p, seeds, outRays, nullptr, nullptr, false, "rtr_light_rays_hinted", outLeaves, true), n);
}

int rtr_shade_hits_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                         const uint32_t* seeds, const uint8_t* occluded, RtrRadiance* out) {
    return enqueue_light(c, s, rays, hits, n, p, seeds, nullptr, occluded, out, true, "rtr_shade_hits_async");
}

int rtr_shade_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                   const uint32_t* seeds, const uint8_t* occluded, RtrRadiance* out) {
    return join_if_enqueued(c, enqueue_light(c, s, rays, hits, n, p, seeds, nullptr, occluded, out, true, "rtr_shade_hits"), n);
}

int rtr_tonemap_pack_async(rtr_ctx* c, const float* radiance, uint32_t strideBytes, uint32_t n, uint32_t* out) {
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_tonemap_pack: null context");
    if (strideBytes < 12 || (strideBytes & 3u)) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_tonemap_pack: strideBytes %u (a multiple of 4, at least 12)", strideBytes);
    if (n == 0) return RTR_OK;
    const Arg args[2] = {{radiance, "radiance", 4, true}, {out, "outBGRA8", 4, true}};
    if (const int rc = check_ptrs("rtr_tonemap_pack", args)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launched(rtrdev::launch_tonemap_pack(radiance, strideBytes / 4u, n, out, c->stream), "rtr_tonemap_pack");
}

int rtr_tonemap_pack(rtr_ctx* c, const float* radiance, uint32_t strideBytes, uint32_t n, uint32_t* out) {
    return join_if_enqueued(c, rtr_tonemap_pack_async(c, radiance, strideBytes, n, out), n);
}

/* ---- continuation rays for ray-query hits (kernels/rtr_bounce.hip; the host form is rtr_bounce_host.cpp) -------------------------- */
static int enqueue_bounce(rtr_ctx* c, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p, const uint32_t* seeds,
                          RtrRay* outRays, RtrBounce* outBounce, const char* who) {
    /* the arrays and the params are checked first, which needs nothing of the handle */
    if (const int rc = n ? rtrdev::bounce_check_args(who, rays, surfaces, n, p, seeds, outRays, outBounce) : RTR_OK) return rc;
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: ctx is null", who);
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::BounceArgs a{};
    a.rays = reinterpret_cast<const float4*>(rays); a.surfaces = reinterpret_cast<const float4*>(surfaces); a.seeds = seeds;
    a.outRays = reinterpret_cast<float4*>(outRays); a.outBounce = reinterpret_cast<float4*>(outBounce); a.params = *p; a.n = n;
    return launched(rtrdev::launch_bounce_rays(a, c->stream), who);
}

int rtr_bounce_rays_async(rtr_ctx* c, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p, const uint32_t* seeds,
                          RtrRay* outRays, RtrBounce* outBounce) {
    return enqueue_bounce(c, rays, surfaces, n, p, seeds, outRays, outBounce, "rtr_bounce_rays_async");
}

int rtr_bounce_rays(rtr_ctx* c, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_bounce_params* p, const uint32_t* seeds,
                    RtrRay* outRays, RtrBounce* outBounce) {
    return join_if_enqueued(c, enqueue_bounce(c, rays, surfaces, n, p, seeds, outRays, outBounce, "rtr_bounce_rays"), n);
}

/* ---- compaction of live paths (kernels/rtr_paths.hip; the host form and the argument checks are rtr_paths_host.cpp) ----------------- */
static int enqueue_compact(rtr_ctx* c, const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds, uint32_t n,
                           const rtr_compact_params* p, void* scratch, size_t scratchBytes, RtrRay* outRays, float* outThroughput,
                           uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount, const char* who) {
    /* the arrays and the params are checked first, which needs nothing of the handle */
    const rtrdev::CompactCall call{rays, throughput, seeds, pathIds, n, p, scratch, scratchBytes, rtrdev::compact_scratch_bytes(n), true,
                                   outRays, outThroughput, outSeeds, outPathIds, outCount};
    if (const int rc = n ? rtrdev::compact_check_args(who, call) : RTR_OK) return rc;
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: ctx is null", who);
    if (n == 0 && !outCount) return RTR_OK;
    if (n == 0 && !aligned4(outCount)) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: outCount is not 4-B aligned", who);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(outCount, 0, sizeof(uint32_t), c->stream));
        return RTR_OK;
    }
    const size_t groups = ((size_t)n + 255u) / 256u;
    rtrdev::CompactArgs a{};
    a.rays = reinterpret_cast<const float4*>(rays); a.throughput = reinterpret_cast<const char*>(throughput); a.seeds = seeds; a.pathIds = pathIds;
    a.ballots = static_cast<unsigned long long*>(scratch);
    a.groupTotals = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + groups * 32u);
    a.outRays = reinterpret_cast<float4*>(outRays); a.outThroughput = outThroughput; a.outSeeds = outSeeds; a.outPathIds = outPathIds;
    a.outCount = outCount; a.params = *p; a.n = n;
    return launched(rtrdev::launch_compact_paths(a, c->stream), who);
}

int rtr_compact_paths_async(rtr_ctx* c, const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds, uint32_t n,
                            const rtr_compact_params* p, void* scratch, size_t scratchBytes, RtrRay* outRays, float* outThroughput,
                            uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount) {
    return enqueue_compact(c, rays, throughput, seeds, pathIds, n, p, scratch, scratchBytes, outRays, outThroughput, outSeeds, outPathIds, outCount,
                           "rtr_compact_paths_async");
}

int rtr_compact_paths(rtr_ctx* c, const RtrRay* rays, const float* throughput, const uint32_t* seeds, const uint32_t* pathIds, uint32_t n,
                      const rtr_compact_params* p, void* scratch, size_t scratchBytes, RtrRay* outRays, float* outThroughput,
                      uint32_t* outSeeds, uint32_t* outPathIds, uint32_t* outCount, uint32_t* hostCount) {
    const int rc = enqueue_compact(c, rays, throughput, seeds, pathIds, n, p, scratch, scratchBytes, outRays, outThroughput, outSeeds, outPathIds,
                                   outCount, "rtr_compact_paths");
    if (rc != RTR_OK) return rc;
    if (n == 0) {                        /* nothing was launched; the count's memset, when there is one, is joined like a launch */
        if (hostCount) *hostCount = 0u;
        if (outCount) HIP_TRY(hipStreamSynchronize(c->stream));
        return RTR_OK;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (hostCount) {                     /* on the context's stream, so that no other stream is joined */
        HIP_TRY(hipMemcpyAsync(hostCount, outCount, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RTR_OK;
}

/* ---- picked light samples (kernels/rtr_query.hip; the rule is include/rtr_pick.h, the host form and the argument checks rtr_pick_host.cpp) -- */
/* What the picked calls and rtr_mis_pick_weights do between their own argument checks and the launch: the handles, their device, the
 * scene's lights against the params.  areaSlots: A of include/rtr_pick.h; tris: the light triangles behind it. */
static int picked_scene_checks(const rtr_ctx* c, const rtr_scene* s, const rtr_light_params* p, const char* who, uint32_t* areaSlots, uint32_t* tris) {
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    uint32_t q = 0;
    if (const int rc = light_slots(s, p, &q, who)) return rc;
    *areaSlots = q - 1u; *tris = *areaSlots / p->numShadowRays;
    return rtrdev::pick_check_area(who, *areaSlots);
}

/* and what their launches take alike; the output arrays and the weights are the caller's */
static void fill_pick_args(rtrdev::PickArgs& pa, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                           const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, uint32_t areaSlots, uint32_t tris) {
    fill_light_args(pa.la, s, rays, hits, n, p, seeds);
    pa.la.slots = pick->numPicks + 1u;
    pa.picks = pick->numPicks; pa.depth = pick->depth; pa.areaSlots = areaSlots;
    pa.defaultWeight = (float)tris / (float)pick->numPicks;
    pa.slotsIn = slots;
}

static int enqueue_light_picked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, RtrRay* outRays, uint32_t* outSlots,
                                const float* weights, const uint8_t* occluded, RtrRadiance* out, bool shade, const char* who) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::pick_check_params(who, p, pick, shade)) return rc;
    const rtrdev::PickCall call{rays, hits, n, p, pick, seeds, shade, slots, outRays, outSlots, weights, occluded, out};
    if (const int rc = n ? rtrdev::pick_check_arrays(who, call) : RTR_OK) return rc;
    uint32_t areaSlots = 0, tris = 0;
    if (const int rc = picked_scene_checks(c, s, p, who, &areaSlots, &tris)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::PickArgs pa{};
    fill_pick_args(pa, s, rays, hits, n, p, pick, seeds, slots, areaSlots, tris);
    pa.la.outRays = reinterpret_cast<float4*>(outRays); pa.la.occluded = occluded; pa.la.out = reinterpret_cast<float4*>(out);
    pa.outSlots = outSlots; pa.weights = weights;
    return launched(shade ? rtrdev::launch_shade_hits_picked(s->dev, pa, c->stream) : rtrdev::launch_light_rays_picked(s->dev, pa, c->stream), who);
}

int rtr_light_rays_picked_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slotsIn, RtrRay* outRays, uint32_t* outSlots) {
    return enqueue_light_picked(c, s, rays, hits, n, p, pick, seeds, slotsIn, outRays, outSlots, nullptr, nullptr, nullptr, false, "rtr_light_rays_picked_async");
}

int rtr_light_rays_picked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                          const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slotsIn, RtrRay* outRays, uint32_t* outSlots) {
    return join_if_enqueued(c, enqueue_light_picked(c, s, rays, hits, n, p, pick, seeds, slotsIn, outRays, outSlots, nullptr, nullptr, nullptr, false,
                                                    "rtr_light_rays_picked"), n);
}

int rtr_shade_hits_picked_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, const float* weights,
                                const uint8_t* occluded, RtrRadiance* out) {
    return enqueue_light_picked(c, s, rays, hits, n, p, pick, seeds, slots, nullptr, nullptr, weights, occluded, out, true, "rtr_shade_hits_picked_async");
}

int rtr_shade_hits_picked(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                          const rtr_pick_params* pick, const uint32_t* seeds, const uint32_t* slots, const float* weights,
                          const uint8_t* occluded, RtrRadiance* out) {
    return join_if_enqueued(c, enqueue_light_picked(c, s, rays, hits, n, p, pick, seeds, slots, nullptr, nullptr, weights, occluded, out, true,
                                                    "rtr_shade_hits_picked"), n);
}

/* ---- MIS at a path vertex (kernels/rtr_query.hip, kernels/rtr_mis.hip; the rule is include/rtr_mis.h, the host forms and the argument checks rtr_mis_host.cpp) -- */
static int enqueue_mis_pick_weights(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                                    const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds, const uint32_t* slots,
                                    float* outWeights, RtrMisSample* outSamples, const char* who) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::mis_check_params(who, mis)) return rc;
    if (const int rc = rtrdev::pick_check_params(who, p, pick, true)) return rc;
    if (const int rc = rtrdev::mis_check_pick_call(who, p, pick, mis, rays, hits, n, seeds, slots, outWeights, outSamples)) return rc;
    uint32_t areaSlots = 0, tris = 0;
    if (const int rc = picked_scene_checks(c, s, p, who, &areaSlots, &tris)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::MisPickArgs ma{};
    fill_pick_args(ma.pa, s, rays, hits, n, p, pick, seeds, slots, areaSlots, tris);
    ma.outWeights = outWeights; ma.outSamples = reinterpret_cast<float4*>(outSamples); ma.lobes = mis->lobes; ma.tris = tris;
    return launched(rtrdev::launch_mis_pick_weights(s->dev, ma, c->stream), who);
}

int rtr_mis_pick_weights_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                               const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds, const uint32_t* slots, float* outWeights,
                               RtrMisSample* outSamples) {
    return enqueue_mis_pick_weights(c, s, rays, hits, n, p, pick, mis, seeds, slots, outWeights, outSamples, "rtr_mis_pick_weights_async");
}

int rtr_mis_pick_weights(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, uint32_t n, const rtr_light_params* p,
                         const rtr_pick_params* pick, const rtr_mis_params* mis, const uint32_t* seeds, const uint32_t* slots, float* outWeights,
                         RtrMisSample* outSamples) {
    return join_if_enqueued(c, enqueue_mis_pick_weights(c, s, rays, hits, n, p, pick, mis, seeds, slots, outWeights, outSamples, "rtr_mis_pick_weights"), n);
}

static int enqueue_emitter_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces,
                                const RtrBounce* bounces, uint32_t n, const rtr_mis_params* mis, RtrEmitter* out, const char* who) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::mis_check_params(who, mis)) return rc;
    if (const int rc = n ? rtrdev::mis_check_emitter_arrays(who, rays, hits, prevSurfaces, bounces, out) : RTR_OK) return rc;
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (mis->numAreaLights > s->numLights) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: numAreaLights %u > scene lights %u", who, mis->numAreaLights, s->numLights);
    uint64_t tris = 0;
    for (uint32_t l = 0; l < mis->numAreaLights; ++l) tris += s->hostLights[l].numTriangles;
    if (tris > RTR_PICK_MAX_SLOTS) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: %llu light triangles are more than 2^24", who, (unsigned long long)tris);
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::EmitterArgs a{};
    a.rays = reinterpret_cast<const float4*>(rays); a.hits = reinterpret_cast<const float4*>(hits);
    a.prevSurfaces = reinterpret_cast<const float4*>(prevSurfaces); a.bounces = reinterpret_cast<const float4*>(bounces);
    a.out = reinterpret_cast<float4*>(out);
    a.lightTris = s->dev.lightTris; a.lightTriFirst = s->dev.lightTriFirst; a.lights = s->dev.lights; a.numLights = s->numLights;
    a.numAreaLights = mis->numAreaLights; a.tris = (uint32_t)tris; a.picks = mis->numPicks; a.n = n;
    return launched(rtrdev::launch_emitter_hits(a, c->stream), who);
}

int rtr_emitter_hits_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                           uint32_t n, const rtr_mis_params* mis, RtrEmitter* out) {
    return enqueue_emitter_hits(c, s, rays, hits, prevSurfaces, bounces, n, mis, out, "rtr_emitter_hits_async");
}

int rtr_emitter_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                     uint32_t n, const rtr_mis_params* mis, RtrEmitter* out) {
    return join_if_enqueued(c, enqueue_emitter_hits(c, s, rays, hits, prevSurfaces, bounces, n, mis, out, "rtr_emitter_hits"), n);
}

/* ---- sky importance sampling (kernels/rtr_sky.hip; the rule is include/rtr_sky.h, the host forms and the argument checks rtr_sky_host.cpp) -- */
static rtr_sky_source scene_sky_source(const rtr_scene* s) {
    rtr_sky_source src{};
    src.pixels = s->dev.hdri.pixels; src.width = s->dev.hdri.width; src.height = s->dev.hdri.height; src.channels = s->dev.hdri.channels;
    for (int k = 0; k < 3; ++k) src.skyLinear[k] = s->dev.skyLinear[k];
    return src;
}

/* Made by the first call that needs it, on `st` (the current device is the scene's), and JOINED before the call goes on, as the leaf
 * table is: whichever context of the device asks next finds it complete.  It reads the HDRI's texels and the sky colour alone, which
 * no update, refit or rebuild writes. */
static int ensure_sky_table(const rtr_scene* s, hipStream_t st, const char* who) {
    if (s->skyReady) return RTR_OK;
    const rtr_sky_source src = scene_sky_source(s);
    const uint32_t W = rtr_sky_table_width(&src), H = rtr_sky_table_height(&src);
    if (W > RTR_SKY_MAX_WIDTH) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: the scene's hdri is %u texels wide: a row's sum fits 32 bits up to %u", who, W, RTR_SKY_MAX_WIDTH);
    HIP_TRY(s->skyRows.alloc((size_t)W * H));
    HIP_TRY(s->skyMarginal.alloc(H));
    const hipError_t e = rtrdev::launch_sky_table(src, s->skyRows.p, s->skyMarginal.p, st);
    if (e != hipSuccess) return fail(RTR_ERR_HIP, "%s: sky table: %s", who, hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    s->skyReady = true;
    return RTR_OK;
}

static rtrdev::SkyDevice scene_sky_device(const rtr_scene* s) {
    rtrdev::SkyDevice sd{};
    sd.sky = scene_sky_source(s);
    sd.table.rows = s->skyRows.p; sd.table.marginal = s->skyMarginal.p;
    sd.table.width = rtr_sky_table_width(&sd.sky); sd.table.height = rtr_sky_table_height(&sd.sky);
    return sd;
}

int rtr_scene_prepare_sky(rtr_scene* s) {
    static const char* who = "rtr_scene_prepare_sky";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    HIP_TRY(hipSetDevice(s->ctx->device));
    return ensure_sky_table(s, s->ctx->stream, who);
}

int rtr_scene_export_sky_table(const rtr_scene* s, uint32_t* outWidth, uint32_t* outHeight, uint32_t* outRows, size_t capacityCells, uint64_t* outMarginal,
                               uint32_t capacityRows) {
    static const char* who = "rtr_scene_export_sky_table";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    const rtr_sky_source src = scene_sky_source(s);
    const uint32_t W = rtr_sky_table_width(&src), H = rtr_sky_table_height(&src);
    if (outWidth) *outWidth = W;
    if (outHeight) *outHeight = H;
    if (!outRows || !outMarginal || capacityCells < (size_t)W * H || capacityRows < H)
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: capacity %zu cells, %u rows; %zu and %u are needed", who, outRows ? capacityCells : (size_t)0,
                    outMarginal ? capacityRows : 0u, (size_t)W * H, H);
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (const int rc = ensure_sky_table(s, s->ctx->stream, who)) return rc;
    HIP_TRY(hipMemcpy(outRows, s->skyRows.p, (size_t)W * H * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(outMarginal, s->skyMarginal.p, (size_t)H * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RTR_OK;
}

static int enqueue_sky_rays(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_sky_params* p,
                            const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples, const char* who) {
    /* the params and the arrays are checked first, which needs nothing of the handles */
    if (const int rc = rtrdev::sky_check_params(who, p, false)) return rc;
    if (const int rc = rtrdev::sky_check_rays_call(who, p, rays, surfaces, n, seeds, outRays, outSamples)) return rc;
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = ensure_sky_table(s, c->stream, who)) return rc;
    rtrdev::SkyRaysArgs a{};
    a.sd = scene_sky_device(s);
    a.rays = reinterpret_cast<const float4*>(rays); a.surfaces = reinterpret_cast<const float4*>(surfaces); a.seeds = seeds;
    a.outRays = reinterpret_cast<float4*>(outRays); a.outSamples = reinterpret_cast<float4*>(outSamples);
    a.params = *p; a.n = n;
    return launched(rtrdev::launch_sky_rays(a, a.sd.table.height <= rtrdev::kSkyLdsRows, c->stream), who);
}

int rtr_sky_rays_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_sky_params* p,
                       const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples) {
    return enqueue_sky_rays(c, s, rays, surfaces, n, p, seeds, outRays, outSamples, "rtr_sky_rays_async");
}

int rtr_sky_rays(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrSurface* surfaces, uint32_t n, const rtr_sky_params* p,
                 const uint32_t* seeds, RtrRay* outRays, RtrSkySample* outSamples) {
    return join_if_enqueued(c, enqueue_sky_rays(c, s, rays, surfaces, n, p, seeds, outRays, outSamples, "rtr_sky_rays"), n);
}

static int enqueue_shade_sky(rtr_ctx* c, const RtrSkySample* samples, const uint8_t* occluded, uint32_t n, uint32_t numSamples, float* out, const char* who) {
    if (const int rc = rtrdev::sky_check_shade_call(who, samples, occluded, n, numSamples, out)) return rc;
    if (!c) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null context", who);
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    rtrdev::SkyShadeArgs a{};
    a.samples = reinterpret_cast<const float4*>(samples); a.occluded = occluded; a.out = reinterpret_cast<float4*>(out);
    a.numSamples = numSamples; a.n = n;
    return launched(rtrdev::launch_shade_sky(a, c->stream), who);
}

int rtr_shade_sky_async(rtr_ctx* c, const RtrSkySample* samples, const uint8_t* occluded, uint32_t n, uint32_t numSamples, float* out) {
    return enqueue_shade_sky(c, samples, occluded, n, numSamples, out, "rtr_shade_sky_async");
}

int rtr_shade_sky(rtr_ctx* c, const RtrSkySample* samples, const uint8_t* occluded, uint32_t n, uint32_t numSamples, float* out) {
    const int rc = enqueue_shade_sky(c, samples, occluded, n, numSamples, out, "rtr_shade_sky");
    return rc == RTR_OK ? join_if_enqueued(c, rc, n) : rc;
}

static int enqueue_sky_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                            uint32_t n, const rtr_sky_params* p, RtrSkyEscape* out, const char* who) {
    if (const int rc = rtrdev::sky_check_params(who, p, true)) return rc;
    if (const int rc = n ? rtrdev::sky_check_hits_arrays(who, rays, hits, prevSurfaces, bounces, n, out) : RTR_OK) return rc;
    if (const int rc = check_handles(c, s, who)) return rc;
    if (const int rc = check_same_device(c, s, who)) return rc;
    if (n == 0) return RTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = ensure_sky_table(s, c->stream, who)) return rc;
    rtrdev::SkyHitsArgs a{};
    a.sd = scene_sky_device(s);
    a.rays = reinterpret_cast<const float4*>(rays); a.hits = reinterpret_cast<const float4*>(hits);
    a.prevSurfaces = reinterpret_cast<const float4*>(prevSurfaces); a.bounces = reinterpret_cast<const float4*>(bounces);
    a.out = reinterpret_cast<float4*>(out); a.numSamples = p->numSamples; a.flags = p->flags; a.n = n;
    return launched(rtrdev::launch_sky_hits(a, c->stream), who);
}

int rtr_sky_hits_async(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                       uint32_t n, const rtr_sky_params* p, RtrSkyEscape* out) {
    return enqueue_sky_hits(c, s, rays, hits, prevSurfaces, bounces, n, p, out, "rtr_sky_hits_async");
}

int rtr_sky_hits(rtr_ctx* c, const rtr_scene* s, const RtrRay* rays, const RtrHit* hits, const RtrSurface* prevSurfaces, const RtrBounce* bounces,
                 uint32_t n, const rtr_sky_params* p, RtrSkyEscape* out) {
    return join_if_enqueued(c, enqueue_sky_hits(c, s, rays, hits, prevSurfaces, bounces, n, p, out, "rtr_sky_hits"), n);
}

int rtr_scene_export_light_tris(const rtr_scene* s, float* outRecords, uint32_t capacityTris, uint32_t* outFirst, uint32_t* outCount) {
    static const char* who = "rtr_scene_export_light_tris";
    if (!s) return fail(RTR_ERR_INVALID_ARGUMENT, "%s: null scene", who);
    uint32_t total = 0;
    std::vector<uint32_t> first(s->numLights);
    for (uint32_t l = 0; l < s->numLights; ++l) { first[l] = total; total += s->hostLights[l].numTriangles; }
    if (outCount) *outCount = total;
    if (capacityTris < total || (total && !outRecords))
        return fail(RTR_ERR_INVALID_ARGUMENT, "%s: capacity %u light triangles, %u are needed", who, outRecords ? capacityTris : 0u, total);
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (total) HIP_TRY(hipMemcpyAsync(outRecords, s->lightTris.p, (size_t)total * rtrdev::kLightTriRecord * sizeof(float4), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (outFirst) for (uint32_t l = 0; l < s->numLights; ++l) outFirst[l] = first[l];
    return RTR_OK;
}

#ifdef RTR_TEST_HOOKS
/* librtr_hip_test.so only: what the loaded code object says of the binned queue build, k_shadow_gen_oct<single> (spp == 1) or <false> —
 * out[0] VGPRs, out[1] private-segment bytes per lane, out[2] static LDS bytes, out[3] the launch bound.  Register and scratch figures
 * only: the spp == 1 form is meant to have no private segment at its eight waves per SIMD (tests/test_gpu_gen_oct_scratch.py). */
int rtr_test_gen_oct_attributes(int single, uint32_t out[4]) {
    if (!out) return fail(RTR_ERR_INVALID_ARGUMENT, "rtr_test_gen_oct_attributes: null output");
    hipFuncAttributes a{};
    HIP_TRY(rtrdev::gen_oct_attributes(single != 0, &a));
    out[0] = (uint32_t)a.numRegs; out[1] = (uint32_t)a.localSizeBytes; out[2] = (uint32_t)a.sharedSizeBytes; out[3] = (uint32_t)a.maxThreadsPerBlock;
    return RTR_OK;
}
#endif

}  // extern "C"
