/* rtr_bvh.h — device BVH build / refit (internal to librtr_hip.so); see rtr_bvh.hip. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/rtr_types.h"

namespace rtrdev {

struct PrimRef { uint32_t customIndex, primitiveId, flags, _pad; };                     /* canonical (instance, primitive) order */
struct InstanceRef { float transform[12]; uint32_t vertexOffset, indexOffset, _pad[2]; };  /* indexed by customIndex */

struct BvhInputs {
    const PrimRef* prims;
    const InstanceRef* instances;
    const RtrVertex* vertices;
    const uint32_t* indices;
};

struct BvhDeviceArrays {          /* persistent: the tree + what a refit needs */
    float4* nodesF;               /* numNodes x 4: builder-side nodes with fp32 planes (rtr::BvhNodeF); the fit / refit works here */
    uint4*  nodes;                /* numNodes x 2: RtrBvhNode (16-bit planes on *grid), what the traversal reads */
    RtrBvhGrid* grid;             /* 1 record, rewritten by every build / refit */
    float4* tris;                 /* numPrims x 3, leaf order */
    float4* boxMin; float4* boxMax;   /* per leaf-ordered primitive */
    int32_t* parent;              /* per node: (parentIndex << 1) | slot, -1 root, -2 not part of the tree */
    uint32_t* counters; uint32_t* depth;
    uint32_t* slotOfPrim;         /* canonical primitive -> leaf-order slot */
    uint32_t* red;                /* 8 words: centroid bounds, max |coordinate| (float bits) in [6], max depth in [7] */
};

struct BvhScratch {               /* build only */
    float4* trisCanon; float4* minCanon; float4* maxCanon;
    unsigned long long* keysIn; unsigned long long* keysOut;
    int2* range; int2* rawChild;
    void* sortTemp; size_t sortTempBytes;
};

size_t bvh_sort_temp_bytes(uint32_t numPrims);
/* LBVH build: numPrims >= 16.  Node array has numPrims-1 entries (entries inside collapsed subtrees are unused). */
hipError_t bvh_build_lbvh(const BvhInputs& in, uint32_t numPrims, const BvhDeviceArrays& a, const BvhScratch& t, hipStream_t s);
/* Refit after transforms changed: recompute world records in place (leaf order), re-fit every box, re-derive the grid
 * from the new root bounds and re-quantise. */
hipError_t bvh_refit(const BvhInputs& in, uint32_t numPrims, uint32_t numNodes, const BvhDeviceArrays& a, hipStream_t s);

/* ---- vertex updates (rtr_scene_update_vertices): new positions / normals for ranges of the scene's vertex array -------------------
 * One entry of the device table of ranges.  positions / normals point at DEVICE memory (the caller's, or the scene's staging buffer
 * for host data), three 32-bit words per vertex, a launch-wide stride apart; normals may be null: the range keeps its normals. */
struct VertexRange { const uint32_t* positions; const uint32_t* normals; uint32_t firstVertex; uint32_t _pad; };   /* 24 B */
constexpr uint32_t kVertexRangesPerLaunch = 1024;     /* prefix counts of one launch live in LDS (4 KB + 1 word) */
/* One lane per vertex of the concatenation of numRanges (<= kVertexRangesPerLaunch) ranges; prefix: numRanges + 1 words, prefix[r] = the
 * vertices of the ranges before r, prefix[numRanges] = all of them (< 2^32).  Strides in 32-bit words (>= 3).
 * check: atomicMin(firstBad, concatBase + i) for every lane i whose position rtr_scene_create would refuse (not inside +-3.0e38);
 * nothing is written but that word, which the host sets to 0xffffffff first and reads before it launches the write.
 * write: words 0..2 (position) and, where the range has normals, words 4..6 (normal) of vertices[firstVertex + v]; the other six words
 * of the 48-B vertex are not touched.  The caller guarantees firstVertex + count <= the array's length for every range. */
hipError_t launch_check_vertices(const VertexRange* ranges, const uint32_t* prefix, uint32_t numRanges, uint32_t total, uint32_t positionStrideWords,
                                 uint32_t concatBase, uint32_t* firstBad, hipStream_t s);
hipError_t launch_write_vertices(const VertexRange* ranges, const uint32_t* prefix, uint32_t numRanges, uint32_t total, uint32_t positionStrideWords,
                                 uint32_t normalStrideWords, RtrVertex* vertices, hipStream_t s);

/* The enqueued form (rtr_scene_update_vertices_async): up to kVertexRangesPerArgs ranges and their prefix counts as ONE kernel argument
 * (1 800 B of the 4 KB a launch may carry), copied when the launch is enqueued.  check reduces the smallest offending SCENE vertex index
 * (firstVertex + v) into *firstBad (0xffffffff on entry: a memset on the stream); write does nothing at all when the word is set.
 * launch_fold_update_status: one lane adds a set word to status[0..2] = refused count, serial of the first refused update since the
 * host last reset it (0xffffffff: none), its first bad scene vertex. */
constexpr uint32_t kVertexRangesPerArgs = 64;
struct VertexRangeArgs { VertexRange ranges[kVertexRangesPerArgs]; uint32_t prefix[kVertexRangesPerArgs + 1]; uint32_t numRanges; };
hipError_t launch_check_vertices_args(const VertexRangeArgs& t, uint32_t positionStrideWords, uint32_t* firstBad, hipStream_t s);
hipError_t launch_write_vertices_args(const VertexRangeArgs& t, uint32_t positionStrideWords, uint32_t normalStrideWords, RtrVertex* vertices,
                                      const uint32_t* firstBad, hipStream_t s);
hipError_t launch_fold_update_status(const uint32_t* firstBad, uint32_t* status, uint32_t serial, hipStream_t s);
/* The enqueued instance update (rtr_scene_update_instances_async): the instance and light tables of a refit made on the device.  One
 * lane per element of the update — numInstances records of 12 words (a row-major 3x4), strideWords apart, for the instances
 * firstInstance .. in INSTANCE ORDER, then the numLights light infos (24 words each; lights null: no light lanes).
 * check: atomicMin(firstBad, e) for the smallest offending element e — instance index i when one of its 12 floats is not inside
 * +-3.0e38, sceneInstances + l when light l names another vertexOffset / indexOffset / numTriangles than sceneLights[l] holds.
 * write: nothing at all when *firstBad is set; else, at the slot customOf[instance] of every named instance, xforms (12 words), nmats
 * words 0..8 (rtr_normal_matrix) and word mirroredWord (rtr_mirrored.h), refs[].transform; and the light infos into sceneLights. */
hipError_t launch_check_instances(const void* transforms, uint32_t strideWords, uint32_t firstInstance, uint32_t numInstances, const void* lights,
                                  uint32_t numLights, uint32_t sceneInstances, const RtrAreaLightInfo* sceneLights, uint32_t* firstBad, hipStream_t s);
hipError_t launch_write_instances(const void* transforms, uint32_t strideWords, uint32_t firstInstance, uint32_t numInstances, const void* lights,
                                  uint32_t numLights, const uint32_t* customOf, uint32_t mirroredWord, float* xforms, float* nmats, InstanceRef* refs,
                                  RtrAreaLightInfo* sceneLights, const uint32_t* firstBad, hipStream_t s);
/* bvh_refit with the reduction words set by a kernel: no host memory is read after the call returns */
hipError_t bvh_refit_enqueued(const BvhInputs& in, uint32_t numPrims, uint32_t numNodes, const BvhDeviceArrays& a, hipStream_t s);

/* The enqueued rebuild (rtr_scene_rebuild_async).  bvh_build_lbvh_enqueued: bvh_build_lbvh — the same kernels in the same order — with the
 * reduction words set by k_refit_init and the nodesF memset inside: launches only (the hipcub sort runs in the caller's temp storage), no
 * host memory is read after the call returns.  `a` is the STAGE (counters and depth may be the live tree's: scratch of the same stream).
 * bvh_commit_tree: k_commit_tree — when the staged depth stagedRed[7] is above `limit`, the depth goes into *word and nothing is copied;
 * otherwise every (src, dst, bytes) of the table is copied, 16 bytes per lane and trip, word-wise after an array's last whole 16 bytes.
 * bytes: multiples of 4; src, dst: 16-B aligned.  One launch of at most kCommitMaxBlocks workgroups of 256 lanes, grid-strided: 4 MiB
 * per trip — four workgroups (16 waves) per CU of a 256-CU part, which a copy does not need more of. */
constexpr uint32_t kCommitArrays = 12;
constexpr uint32_t kCommitMaxBlocks = 1024;
struct CommitTable { struct { const void* src; void* dst; uint64_t bytes; } a[kCommitArrays]; uint32_t count; };
hipError_t bvh_build_lbvh_enqueued(const BvhInputs& in, uint32_t numPrims, const BvhDeviceArrays& a, const BvhScratch& t, hipStream_t s, const uint32_t* go = nullptr);
hipError_t bvh_commit_tree(const CommitTable& t, const uint32_t* stagedRed, uint32_t limit, uint32_t* word, hipStream_t s, const uint32_t* go = nullptr,
                           uint32_t* committed = nullptr);

/* The rebuild policy on the device (rtr_scene_rebuild_if_async).  THE GATE: the functions above and below that end in `const uint32_t* go`
 * take a device word the launch is predicated on — null: always (every launch that existed before the policy passes null and gives the
 * bytes it gave); else every kernel of the function reads *go first and returns at once when it is 0.  The gated build clears its
 * arrays with gated kernels; the sort and the small memsets of sum words are not gated.  bvh_commit_tree's `committed`, where given, gets 1 when the stage was copied, 0 when not (gate 0, or depth refused).
 * RebuildIfRecord: rtr_rebuild_if_status's fields in its order; the first two pad words are the chain's two gates.
 * bvh_rebuild_if_decide (one lane): sah = rtr_tree_sah(words, grid->scale); lastSah = sah, ++evaluated,
 *   go = lastDecision = sah > rebuildAbove * builtSah, committed = 0.
 * bvh_rebuild_if_close (one lane): when rec->committed, builtSah = rtr_tree_sah(words, grid->scale) and rebuilt += countRebuilt.
 * bvh_clear_words: n 32-bit words to zero, gated — a hipMemsetAsync that a skip can switch off. */
struct RebuildIfRecord { uint64_t evaluated, rebuilt; double builtSah, lastSah; uint32_t lastDecision, go, committed, _pad; };
hipError_t bvh_rebuild_if_decide(const unsigned long long* words, const RtrBvhGrid* grid, RebuildIfRecord* rec, double rebuildAbove, hipStream_t s);
hipError_t bvh_rebuild_if_close(const unsigned long long* words, const RtrBvhGrid* grid, RebuildIfRecord* rec, uint32_t countRebuilt, hipStream_t s);
hipError_t bvh_clear_words(uint32_t* p, uint64_t n, hipStream_t s, const uint32_t* go = nullptr);

/* The 4-wide view of a finished (quantised) tree that the any-hit kernel walks: numNodes x 4 uint4, see k_wide_nodes.
 * parentOrNull: the refit parent array (entries outside the tree are skipped) or null. */
/* sets grid->wideCentreXY / Z (k_wide_centre_*; sums4 = bvh_wide_scratch_words() x u64 of scratch) and writes the 4-wide records about it */
size_t bvh_wide_scratch_words();
/* shapeOrNull: per BVH2 node, which entries its wide record opens (bvh_build.h collapse_wide); null = the greedy rule */
hipError_t bvh_make_wide(const uint4* nodes, uint32_t numNodes, const int32_t* parentOrNull, RtrBvhGrid* grid, const uint8_t* shapeOrNull, uint4* wide, unsigned long long* sums4, hipStream_t s,
                         const uint32_t* go = nullptr);
/* out[remap[i]] = in[i] with inner child codes renumbered through remap (a permutation of 0..numNodes-1, remap[0] == 0) */
hipError_t bvh_permute_wide(const uint4* in, uint32_t numNodes, const uint32_t* remap, uint4* out, hipStream_t stream, const uint32_t* go = nullptr);

/* The permutation bvh_permute_wide takes, made on the device (k_wide_order): the breadth-first order of the 4-wide entries `wide`
 * (un-permuted, child codes in words 12..15), bit for bit what rtr_api.cpp's host loop computes; *reached = the entries the tree reaches.
 * scratch: 2 x numNodes words.  One launch of one workgroup; nothing is read back. */
hipError_t bvh_wide_order(const uint4* wide, uint32_t numNodes, uint32_t* remap, uint32_t* scratch, uint32_t* reached, hipStream_t s, const uint32_t* go = nullptr);

/* The resident order (rtr_hot_top.h): turns remap[] — breadth-first ids, from bvh_wide_order or the host loop — into the positions
 * bvh_permute_wide moves the records to: the best-first top of at most `top` records towards the lights, then every other record in
 * breadth-first order.  wide: the un-permuted records remap[] was made from.  sel: bvh_hot_top_words() words of scratch.  Two launches
 * (one wave, then one lane per record); none without lights or with top <= 1: remap[] stays breadth-first. */
size_t bvh_hot_top_words();
hipError_t bvh_hot_top(const uint4* wide, uint32_t numNodes, uint32_t* remap, uint32_t* sel, const RtrBvhGrid* grid, const RtrAreaLightInfo* lights, uint32_t numLights,
                       uint32_t top, hipStream_t s, const uint32_t* go = nullptr);

/* The SAH cost sums of a finished (quantised) tree, rtr_scene_tree_cost: words = bvh_tree_cost_words() x u64, zeroed here and filled by
 * k_tree_cost as innerArea[3], leafArea[3], rootArea[3], numInner, numLeafRefs (rtr_tree_cost's integers, in that order).
 * parentOrNull: as bvh_make_wide — the refit parent array (slots outside the tree are skipped) or null when every slot is in the tree. */
size_t bvh_tree_cost_words();
hipError_t bvh_tree_cost(const uint4* nodes, uint32_t numNodes, const int32_t* parentOrNull, unsigned long long* words, hipStream_t s, const uint32_t* go = nullptr);

}  // namespace rtrdev
