/*
 * omm_mi355x_ext.h -- MI355X-specific additions to the C ABI (not part of the reference SDK).
 *
 * The reference exposes no timing or device-resident interface: its baker is a host library
 * (libraries/omm-lib/include/omm.h:568-594).  These entry points exist so a harness can (a) read HIP-event
 * timings of the kernels a bake launched on the library's own stream and (b) run a bake whose inputs and
 * outputs stay in HBM.  They use only plain C types.
 */
#ifndef OMM_MI355X_EXT_H
#define OMM_MI355X_EXT_H
#include "omm_mi355x.h"

/* HIP-event timings of the most recent successful bake on this baker (milliseconds). */
typedef struct ommxBakeTimings {
    float    hostSetupMs;      /* work-item setup on the host (0 when the device setup path ran) */
    float    uploadMs;         /* host -> device copies of the work-item tables */
    float    classifyMs;       /* all classify_tiles launches (hierarchical + per-micro-triangle SAT pass, fine level-line pass) */
    float    digestMs;         /* XXH64 digests */
    float    tailMs;           /* promote / dedup / sort / offsets / index buffer */
    float    gatherMs;         /* gather of surviving OMM blocks + descriptors */
    float    downloadMs;       /* device -> host copy of the result arrays */
    float    totalMs;          /* wall clock of the whole call */
    uint64_t microTriangles;   /* sum of 4^level over unique work items */
    uint32_t uniqueItems;
    uint32_t classifyLaunches;
    uint64_t stateBytes;       /* packed state bytes written by classification */
    float    triageMs;         /* level-0 hierarchical query per item + compaction of the active items */
    uint32_t activeItems;      /* items that needed per-micro-triangle classification */
    uint64_t fineMicroTriangles; /* micro-triangles that needed the level-line (fine) pass */
    float    setupMs;          /* device work-item setup: UV fetch, level selection, first-occurrence dedup, level grouping */
    /* ommCpuBake only: the finished OMM blocks are copied to their final place in the host array WHILE the classification runs (ommxBakerKnob_StreamChunks) */
    uint32_t streamChunks;     /* ranges of the classification whose blocks were streamed (0 = the result was copied after the bake) */
    uint64_t streamedBytes;    /* bytes that crossed PCIe that way */
    float    streamTailMs;     /* wall clock from the end of the classification to the last streamed byte on the host (the exposed part of the copy) */
    uint32_t openTiles;        /* tiles (4096 micro-triangles; 1024 for level-5 items) that the tile triage left open, i.e. the units the persistent
                                  classify_tiles launches really process */
    uint64_t openTileMicroTriangles; /* micro-triangles in those tiles */
    uint32_t streamEarlyItems; /* streamed bakes: work items classified with an EARLIER range than their own because another item shares their level-5
                                  preview (possible duplicates: the first member of such a family pulls the others into its range) */
    float    persistentMs;     /* HIP events around the persistent classify_tiles launch of the levels >= 6 alone (classifyMs also holds the tile triage, the
                                  launches of the lower levels and, for streamed bakes, the preview); 0 for streamed bakes */
    float    genericMs;        /* HIP events around the deferred generic pass (classify_generic: micro-triangles of several texels, ommxBakerKnob_GenericPass); 0 when
                                  that work ran inside the persistent launch */
    uint64_t genericMicroTriangles; /* micro-triangles that pass classified */
    uint64_t exchangeBytes;    /* ommxShardedBakeRccl: bytes every rank put on the wire in the block all-gather (the contributions travel as unit codes + raw
                                  units; a contribution that does not shrink below half its size travels as it is) */
    uint64_t contributionBytes; /* ... and the size of a rank's (padded) contribution before that */
    /* (round 4; read them through ommxGetLastBakeTimingsSized) streamed ommCpuBake, wall clock in ms since the bake's device work was first enqueued: */
    float    streamPreviewMs;      /* HIP events around the level-5 preview of the items of level >= 6 (the possible-duplicate search in front of the classification) */
    float    streamFirstCopyMs;    /* the first range's blocks are placed and their copy is issued */
    float    streamLastCopyMs;     /* the last range's copy is issued */
    float    streamRangeReadyMs[32]; /* range k placed (its event seen by the host thread, which then issues its copy) */
    /* (round 5) how arrayData reached the host (ommxResultTransfer_*; ommCpuBake only) and, for the compressed form: */
    uint32_t resultTransfer;
    uint32_t expandThreads;        /* host threads that expanded the codec stream (the caller's included) */
    uint64_t compressedBytes;      /* bytes of the codec stream that crossed PCIe instead of arrayDataSize */
    float    compressMs;           /* wall clock from the end of the bake proper to the stream's size on the host (codec kernels + the small read-backs) */
    float    expandMs;             /* wall clock of the stream's copy and its expansion into arrayData (overlapped slice by slice) */
    uint32_t devices;              /* devices a multi-device ommCpuBake ran on (ommxBakerKnob_Devices); 0 / 1: one */
    /* (round 6) compressed transfer: the helper threads zero an idle result block of the baker WHILE the device bakes; codec blocks that repeat state 0 are then not written again */
    uint64_t prefilledBytes;       /* bytes of the result array that were zeroed ahead (0: no idle block, first bake, another transfer) */
    uint64_t expandSkippedBytes;   /* bytes of arrayData the expansion did not have to write because of that */
} ommxBakeTimings;

/* ommxBakeTimings only ever grows at its END.  ommxGetLastBakeTimingsSized copies min(outBytes, the library's size) bytes and zeros the rest of `out`, so a
 * caller and a library built from different versions of this header stay compatible; *libraryBytes (optional) <- the library's sizeof(ommxBakeTimings).
 * ommxGetLastBakeTimings is the round-3 symbol: it fills the fields up to and including contributionBytes (the struct as it was then) and never writes
 * beyond them, whatever the caller's header says -- the fields from streamPreviewMs on are only available through the sized call. */
OMM_MI355X_API ommResult ommxGetLastBakeTimingsSized(ommBaker baker, void* out, size_t outBytes, size_t* libraryBytes);
/* DEPRECATED (kept for binaries built against the round-3 header): fills only the round-3 prefix of the struct and leaves the rest of `out` untouched --
 * zero the struct first, or better call ommxGetLastBakeTimingsSized(baker, &t, sizeof t, NULL). */
OMM_MI355X_API ommResult ommxGetLastBakeTimings(ommBaker baker, ommxBakeTimings* out)
#if defined(__GNUC__)
    __attribute__((deprecated("use ommxGetLastBakeTimingsSized")))
#endif
    ;

/* ---- per-baker knobs ----
 * Tuning and test switches are state of ONE baker, set explicitly through this call; the library reads no environment variables.
 * A value of 0 restores the default.  Unknown knobs -> INVALID_ARGUMENT. */
typedef enum ommxBakerKnob {
    ommxBakerKnob_Reserved0        = 0, /* (was ommxBakerKnob_SetupKeyBits, a test switch of rounds 1 - 5: the work-item ids are the reference's own 64-bit ids
                                           since round 6, see omm_amd/csrc/vm_id.h; setting it has no effect) */
    ommxBakerKnob_ShardChunkBytes  = 1, /* sharded bake: bytes per rank and chunk of the block all-gather (>= 256; default 64 MiB, at most 8 chunks) */
    ommxBakerKnob_StreamChunks     = 2, /* ommCpuBake: number of ranges (of work items, in the order of the result) whose finished OMM blocks are copied to
                                           their place in the host array while the following ranges are being classified; a value (1..32) forces streaming
                                           whatever the size of the bake (1 = classify everything, then one copy).  Default: bakes with >= 64 MiB of packed
                                           states stream, one range per 32 MiB, at most 32 */
    ommxBakerKnob_GenericPass      = 3, /* where micro-triangles that span several texels (asset-sized triangles) are classified: 1 = inside the persistent
                                           classification launch, one lane each; 2 = queued and classified by a second launch whose lanes pull them as their walks end (not for streamed
                                           bakes); 0 = automatic: 2 when the texels under the triangles outweigh the micro-triangles */
    ommxBakerKnob_RetainMemory     = 4, /* what a baker keeps between bakes.  0 / default: the working set of a bake (device arenas, streams), up to six idle device result
                                           blocks and up to two idle PINNED host blocks for arrayData (a fresh 1.3 GB host block costs more in page faults and munmap than the
                                           PCIe copy of its contents) stay with the baker until it is destroyed; 1: nothing is retained -- every block goes back to the system
                                           when the result that uses it is destroyed.  For pipelines that create many bakers, or bake rarely.  See also ommxTrimBaker. */
    ommxBakerKnob_ResultTransfer   = 5, /* ommCpuBake: how a large arrayData reaches the caller's memory, one of ommxResultTransfer_*.  Auto (0 / default): Compressed when the
                                           bake carries ommCpuBakeFlags_EnableInternalThreads and the process has >= 6 CPUs (affinity / cgroup quota), else Streamed */
    ommxBakerKnob_ExpandThreads    = 6, /* threads (the caller's included, <= 64) that expand a compressed result; 0 / default: three quarters of the CPUs the process may use, at most 12 */
    ommxBakerKnob_Devices          = 7, /* ommCpuBake over N >= 2 devices of this process (at most 16): one host thread per device, rank r on HIP device (baker's + r) mod the
                                           device count; the texture is copied to the other devices by the first bake that needs it; every device classifies its share of
                                           the work items and sends its own blocks to the host as a codec stream over its own PCIe link.  Not for bakes with near-duplicate
                                           merging / maxArrayDataSize or per-triangle formats (those keep to one device).  0 / 1: one device.
                                           HELPER THREADS: a baker starts threads of its own only with the caller's permission.  That permission is
                                           ommCpuBakeFlags_EnableInternalThreads on the bake (the automatic choice of the compressed transfer looks at it), OR setting one of the two
                                           knobs that cannot work without threads: ommxBakerKnob_ResultTransfer = ommxResultTransfer_Compressed (helper threads expand the
                                           result) and ommxBakerKnob_Devices >= 2 (a host thread per device + the expansion).  Setting such a knob IS the permission, whatever
                                           the bake's flags say; without either, ommCpuBake runs on the calling thread only, like the reference without the flag */
    ommxBakerKnob_HelperAffinity   = 8, /* where the baker's helper threads run while they fill a large arrayData.  0 / default: each helper thread is bound to its own slice of
                                           the physical cores of the NUMA node that holds the array (pthread_setaffinity_np on the baker's OWN threads only -- never on the
                                           caller's; measured on the two-socket host of the GPU box: 16.6 - 16.8 ms per bake bound, 17 - 26 ms unbound).  1: the threads are
                                           left where the scheduler puts them (for hosts whose thread placement is managed from outside) */
    ommxBakerKnob_ZeroAhead        = 9, /* compressed transfer: 0 / default: while the device bakes, the helper threads zero the idle result block the previous bake of this
                                           baker left (default allocator only), and the expansion does not write codec blocks of zeros again (ommxBakeTimings::prefilledBytes,
                                           expandSkippedBytes); 1: off -- the helper threads only run during the expansion */
    ommxBakerKnob_PoisonMemory     = 10, /* debugging aid in the spirit of glibc's MALLOC_PERTURB_.  0 / default: off.  (1 << 32) | word: every block the baker's device pool hands
                                           out (scratch of every device entry, the arrays of every device result, texture uploads), fresh or reused, and every device arena of
                                           a bake's working set when the bake reserves it, is filled over its whole capacity with the 32-bit `word` before the caller sees
                                           it (bit 32 only says "on", so a word of 0 can be asked for).  The fill is complete before the call goes on.  Any other non-zero
                                           value is INVALID_ARGUMENT.  An answer that changes with the word reads device memory nobody wrote.  The pinned host result pool
                                           is not filled.  See ommxDebugGetPoisonedBytes. */
    ommxBakerKnob_MAX_NUM          = 11
} ommxBakerKnob;
typedef enum ommxResultTransfer {
    ommxResultTransfer_Auto        = 0,
    ommxResultTransfer_Plain       = 1, /* one device-to-host copy of the finished array after the bake (what small results always get) */
    ommxResultTransfer_Streamed    = 2, /* rounds 3 - 4: finished blocks are placed and copied to their final offsets by the DMA engine WHILE the classification runs
                                           (>= 64 MiB of packed states; ommxBakerKnob_StreamChunks); bound by the PCIe link */
    ommxResultTransfer_Compressed  = 3  /* round 5: the finished array crosses PCIe as a codec stream (one nibble per 16-byte unit: the state it repeats, or raw: 6 % of the
                                           bytes at the metric configuration) and is expanded into the caller's array by helper threads of the baker (ommxBakerKnob_ExpandThreads) */
} ommxResultTransfer;
OMM_MI355X_API ommResult ommxSetBakerKnob(ommBaker baker, ommxBakerKnob knob, uint64_t value);
/* Gives every idle pooled block of the baker back to the system now: pinned host blocks, device result blocks, device working sets of finished bakes.  Results
 * that are still alive keep their memory.  Safe to call at any time from any thread; the next bake allocates again. */
OMM_MI355X_API ommResult ommxTrimBaker(ommBaker baker);
/* Bytes of device memory filled under ommxBakerKnob_PoisonMemory since the baker was created: blocks of the device pool and arenas of bake working sets (the
 * shadow bakers of a multi-device ommCpuBake count into their owner's).  Either pointer may be NULL; a baker that never filled anything gives zeros.  Null or
 * foreign baker -> INVALID_ARGUMENT. */
OMM_MI355X_API ommResult ommxDebugGetPoisonedBytes(ommBaker baker, uint64_t* devicePoolBytes, uint64_t* workingSetBytes);

/* ---- device-resident bake ----
 * Same contract as ommCpuBake (include/omm_mi355x.h; reference omm.h:574) except for where the bulk data lives:
 *   in : desc->texCoords, desc->indexBuffer and desc->subdivisionLevels are DEVICE pointers (HBM of the current HIP device);
 *        desc->formats must be NULL.  All other fields, validation, result codes and log messages are those of ommCpuBake.
 *   out: an ommCpuBakeResultDesc whose arrayData, descArray and indexBuffer are DEVICE pointers; the two histograms are
 *        host arrays.  Buffers stay valid until ommxDestroyDeviceBakeResult.
 * Stream ordering: the library works on its own non-blocking HIP stream, which does NOT order against the caller's streams or the
 * null stream.  Device buffers handed in (inputs here, `words` / `gathered` of the sharded bake below) must be complete -- the
 * producing stream synchronised -- before the call; everything handed back is complete when the call returns.
 * The call returns when the result is complete (the library synchronises its own stream). */
typedef struct _ommxDeviceBakeResult* ommxDeviceBakeResult;
OMM_MI355X_API ommResult ommxBakeDevice(ommBaker baker, const ommCpuBakeInputDesc* deviceDesc, ommxDeviceBakeResult* outResult);
OMM_MI355X_API ommResult ommxGetDeviceBakeResultDesc(ommxDeviceBakeResult result, const ommCpuBakeResultDesc** desc);
OMM_MI355X_API ommResult ommxDestroyDeviceBakeResult(ommxDeviceBakeResult result);


/* ---- multi-GPU sharded bake (one process per GPU) ----
 * Every rank calls the same four functions with the SAME desc (device-resident inputs as for ommxBakeDevice); the caller
 * performs the two collectives in between with whatever transport it has (MPI, torch.distributed, ...).  ommxShardedBakeRccl further
 * down is the same bake as one call with the collectives done by the library.  The handle owns its device working set from Begin to
 * Destroy and holds no lock in between: other bakes on the same baker run concurrently, Destroy may come from any thread.
 *
 *   ommxShardedBegin   work-item setup + triage (replicated, cheap), then classification and digests of THIS rank's share of
 *                      the active work items (contiguous ranges of the per-level lists)
 *   ommxShardedGetMeta -> device array of `numWords` uint32 (4 per active item: state mask, known count, digest lo/hi), zero
 *                      for items of other ranks.           CALLER: all-reduce(SUM) over all ranks, in place.
 *   ommxShardedTail    replicated deterministic tail (promote, first-occurrence dedup, spatial sort, offsets) on the merged
 *                      metadata; packs this rank's surviving OMM blocks -> `contribution` (device), its size, and the common
 *                      padded size `strideBytes`.          CALLER: all-gather of strideBytes per rank into gathered[world][strideBytes].
 *   ommxShardedFinish  places every rank's blocks at their final arrayData offsets -> the same ommxDeviceBakeResult on every
 *                      rank, bit-identical to a single-GPU ommxBakeDevice of the same desc. */
typedef struct _ommxShardedBake* ommxShardedBake;
OMM_MI355X_API ommResult ommxShardedBegin(ommBaker baker, const ommCpuBakeInputDesc* deviceDesc, uint32_t rank, uint32_t worldSize, ommxShardedBake* out);
OMM_MI355X_API ommResult ommxShardedGetMeta(ommxShardedBake bake, void** deviceWords, uint64_t* numWords);
OMM_MI355X_API ommResult ommxShardedTail(ommxShardedBake bake, void** contribution, uint64_t* contributionBytes, uint64_t* strideBytes);
OMM_MI355X_API ommResult ommxShardedFinish(ommxShardedBake bake, const void* gathered, ommxDeviceBakeResult* outResult);
OMM_MI355X_API ommResult ommxShardedDestroy(ommxShardedBake bake);

/* ---- the same sharded bake as ONE call, collectives included (RCCL over xGMI, issued by the library from C++) ----
 * Every rank calls ommxShardedBakeRccl with the SAME desc; the library runs Begin, the SUM all-reduce of the metadata words
 * (ncclAllReduce, in place, on the bake's own stream), Tail, the all-gather of the contributions and Finish.  The contributions cross the links
 * as codec streams -- one nibble per 16-byte unit (which of the four states it repeats, or "raw") plus the raw units: a few per cent of the bytes
 * for ordinary bakes -- and are decoded straight to their final arrayData offsets on arrival; if a rank's contribution does not shrink
 * below half its size, all ranks send the padded contributions themselves (ncclAllGather in chunks of <= 64 MiB per rank on a second stream,
 * each chunk scattered while the next one is on the wire).  A rank-local failure stops all ranks (status agreement before each exchange).  Every rank returns the same merged ommxDeviceBakeResult, bit-identical to a single-GPU ommxBakeDevice of the desc.
 * librccl.so.1 is bound with dlopen at the first call: callers that never shard need no RCCL.
 *
 * Communicator: either wrap an ncclComm_t the application already owns (ommxRcclCommWrap; not destroyed by the library), or let the
 * library create one: rank 0 calls ommxRcclGetUniqueId and distributes the 128 bytes by any means (MPI, a file, torch.distributed),
 * then every rank calls ommxRcclCommInitRank on its own HIP device (collective: it returns once all ranks have joined). */
typedef struct _ommxRcclComm* ommxRcclComm;
#define OMMX_RCCL_UNIQUE_ID_BYTES 128
OMM_MI355X_API ommResult ommxRcclGetUniqueId(void* outId, size_t idBytes);
OMM_MI355X_API ommResult ommxRcclCommInitRank(const void* id, size_t idBytes, uint32_t rank, uint32_t worldSize, ommxRcclComm* outComm);
OMM_MI355X_API ommResult ommxRcclCommWrap(void* ncclComm, ommxRcclComm* outComm);
OMM_MI355X_API ommResult ommxRcclCommDestroy(ommxRcclComm comm);
/* rank and size as the communicator itself reports them (a wrapped or library-made RCCL communicator: ncclCommUserRank / ncclCommCount asked again at the
 * time of the call; a communicator of caller collectives: the values it was made with) */
OMM_MI355X_API ommResult ommxRcclCommInfo(ommxRcclComm comm, uint32_t* outRank, uint32_t* outWorldSize);
OMM_MI355X_API ommResult ommxShardedBakeRccl(ommBaker baker, const ommCpuBakeInputDesc* deviceDesc, ommxRcclComm comm, ommxDeviceBakeResult* outResult);

/* ---- the one-call sharded bake over a transport of the caller (MPI with device pointers, torch.distributed, a test harness) ----
 * ommxCommFromCollectives makes a communicator whose two collectives are the caller's functions instead of RCCL's; ommxShardedBakeRccl takes it like
 * any other and runs the identical sequence (status agreement, metadata all-reduce, codec streams or raw chunks, scatter).  Both functions
 * work on DEVICE pointers and are collective: every rank calls them in the same order with the same counts.  They are stream-ordered like their RCCL
 * counterparts: `send` is complete once the work queued on `hipStream` so far has run, and work queued on `hipStream` after the call must see `recv`
 * (a blocking implementation synchronises the stream, exchanges, and returns).  `send` may equal `recv` in allReduceU32.  Return 0 for success.
 * The structure is copied; `user` must stay valid until ommxRcclCommDestroy. */
typedef enum ommxReduceOp { ommxReduceOp_Sum = 0, ommxReduceOp_Max = 1, ommxReduceOp_Min = 2 } ommxReduceOp;
typedef struct ommxCollectives
{
    int (*allReduceU32)(void* user, const void* send, void* recv, size_t count, ommxReduceOp op, void* hipStream);       /* `count` uint32 elements */
    int (*allGatherBytes)(void* user, const void* send, void* recv, size_t bytesPerRank, void* hipStream);               /* recv[rank r] = recv + r * bytesPerRank */
    void* user;
} ommxCollectives;
OMM_MI355X_API ommResult ommxCommFromCollectives(const ommxCollectives* collectives, uint32_t rank, uint32_t worldSize, ommxRcclComm* outComm);

/* ---- using a baked micromap on the GPU (include/omm_mi355x_lookup.h is the per-hit device function behind these) ----
 * A hit is a triangle of the baked mesh and the DXR / Vulkan barycentrics of the hit point: (1-u-v) * V0 + u * V1 + v * V2, V0..V2 in
 * index-buffer order.  Every call below takes `count` hits and writes one byte per hit; count == 0 is SUCCESS without a launch.
 *
 * ommxLookupOpacity      out[i] = ommx_opacity_state(result, hit i): 0..3 (ommOpacityState) or OMMX_OPACITY_INVALID (0xFF).
 *                        `result` is a HOST struct whose arrays (arrayData, descArray, indexBuffer) are DEVICE memory: the desc of
 *                        ommxGetDeviceBakeResultDesc, or one the caller filled with device copies of an ommCpuBake result.  The struct is
 *                        read during the call; the arrays, `hits` and `outStates` (device memory) are used by the kernel, which is enqueued
 *                        on `hipStream` (a hipStream_t; null = the null stream) and runs asynchronously.  Flags: Force2State only.
 * ommxLookupOpacityHost  the same answer from the same header code on the CPU: host pointers, synchronous.
 * ommxResolveHits        the any-hit answer.  out[i]: bit 0 = opaque, bits 1-2 = OMM state, bit 3 = the texture was sampled; 0xFF = a hit the
 *                        result cannot answer.  A hit whose OMM state is Transparent or Opaque is answered from the OMM alone; any other hit
 *                        samples mip 0 of the texture at the hit's interpolated texture coordinate with the desc's runtimeSamplerDesc and
 *                        maps alpha > alphaCutoff to alphaCutoffGreater, otherwise to alphaCutoffLessEqual (an Unknown* answer counts as its
 *                        opaque / transparent half).  Flag IgnoreMicromap samples the texture for every hit (the plain alpha test); Force2State
 *                        applies to the OMM state, so an unknown state then becomes known and the texture is not sampled.
 *                        `deviceDesc` is the device-resident input desc the result was baked from (as given to ommxBakeDevice: a texture of
 *                        this baker, sampler, cut-off, device texcoords and indices); it is refused where ommxBakeDevice would refuse it, with
 *                        the same result code.  `result`, `hits`, `out` and the stream as for ommxLookupOpacity.
 *                        The result may have more index entries than deviceDesc has triangles (indexCount / 3).  A hit on a primitive at or
 *                        beyond the desc's triangle count is answered from the OMM where its state there is Transparent or Opaque (after
 *                        Force2State, if set); where the texture would have to be sampled -- an unknown state, or any state under
 *                        IgnoreMicromap -- it reads 0xFF, and the desc's index buffer and texture coordinates are not read for it.
 * None of the three allocates memory or synchronises a stream. */
typedef struct ommxHit { uint32_t primitiveIndex; float u, v; } ommxHit;
typedef enum ommxLookupFlags {
    ommxLookupFlags_None           = 0,
    ommxLookupFlags_Force2State    = 1,
    ommxLookupFlags_IgnoreMicromap = 2
} ommxLookupFlags;
OMM_MI355X_API ommResult ommxLookupOpacity(const ommCpuBakeResultDesc* result, const ommxHit* hits, uint32_t count, uint8_t* outStates, uint32_t flags, void* hipStream);
OMM_MI355X_API ommResult ommxLookupOpacityHost(const ommCpuBakeResultDesc* result, const ommxHit* hits, uint32_t count, uint8_t* outStates, uint32_t flags);
OMM_MI355X_API ommResult ommxResolveHits(ommBaker baker, const ommCpuBakeInputDesc* deviceDesc, const ommCpuBakeResultDesc* result,
                                         const ommxHit* hits, uint32_t count, uint8_t* out, uint32_t flags, void* hipStream);

/* ---- ommDebugStats of a device-resident result, computed where the result lives ----
 * ommxDebugGetStatsDevice   ommDebugGetStats / ommDebugGetStats2 for a result whose arrays are DEVICE memory.  `deviceResult` is a HOST struct as for
 *                        ommxLookupOpacity: the desc of ommxGetDeviceBakeResultDesc, or one the caller filled with device copies of an ommCpuBake
 *                        result (on the baker's device).  One streaming pass over arrayData and one over the index buffer; nothing is downloaded.
 *   integer fields       exactly what ommDebugGetStats answers for a host copy of the same arrays, its 32-bit arithmetic included: per referenced
 *                        block, (uint32_t)(references * count[state]) is added to the 64-bit totals.  Blocks no primitive selects add nothing.
 *   bounds               the host call trusts the descriptors; this one applies the rule of include/omm_mi355x_lookup.h before any read: a
 *                        descriptor with a level above 12, a format other than OC1_2_State / OC1_4_State or a block that does not fit inside
 *                        arrayDataSize has zero counts and adds nothing, and a primitive that selects it is ignored like one whose entry is below -4
 *                        or at or beyond descArrayCount (which the host ignores too).  *outSkippedPrimitives (optional) <- the number of primitives
 *                        ignored for any of these reasons.
 *   outputs (optional)   per-block and per-primitive answers in DEVICE memory, every member optional; complete when the call returns:
 *                        stateCounts[d][s]   micro-triangles of block d in ommOpacityState s (all blocks, referenced or not),
 *                        referenceCounts[d]  primitives whose index entry selects block d,
 *                        knownFraction[i]    1 for FullyTransparent / FullyOpaque, 0 for the two FullyUnknown specials and for ignored primitives,
 *                                            otherwise (float)(T + O) / (float)(T + O + UT + UO) of the selected block, one IEEE fp32 division.
 *   knownAreaMetric      with `deviceTriangleAreas` (indexCount floats in device memory):
 *                            (float)( sum_i (double)area[i] * (double)knownFraction[i]  /  sum_i (double)area[i] )
 *                        both sums in fp64 over a fixed partition and a fixed tree, without floating-point atomics: two calls on the same inputs
 *                        return the same bits.  This is the QUANTITY ommDebugGetStats2 reports, not its rounding: the host sums in fp32 in triangle
 *                        order (per block first), which no parallel reduction reproduces; the two agree to about (indexCount + 4) * 2^-22.
 *                        A zero area sum gives the host's NaN.  Without areas (NULL) the metric is 0, as in ommDebugGetStats.
 *   stream, memory       the kernels run on `hipStream` (a hipStream_t; null = the null stream), which the call synchronises before it returns -- the
 *                        answer is a host struct.  Scratch comes from the baker's device pool and is back there when the call returns.
 *   result codes         null baker, deviceResult or out, a baker of unknown type, an unknown indexFormat -> INVALID_ARGUMENT; indexCount == 0 ->
 *                        SUCCESS without a launch (all fields zero, `outputs` untouched).
 * ommxGetDeviceBakeResultTriangleAreas   the UV-space area of every input triangle (the side channel ommDebugGetStats2 reads from an
 *                        ommCpuBakeResult): every result of ommxBakeDevice owns a device copy, indexCount floats, valid until
 *                        ommxDestroyDeviceBakeResult.  Results of ommxShardedFinish / ommxShardedBakeRccl do not carry areas: *deviceAreas <- NULL.
 * ommxDebugGetStatsDevice2  the ommDebugGetStats2 of device results: ommxDebugGetStatsDevice on the result's desc with its own areas, on the null
 *                        stream.  For a sharded result (no areas) knownAreaMetric is 0. */
typedef struct ommxDeviceStatsOutputs {   /* every member optional (NULL = not wanted); DEVICE memory */
    uint32_t* stateCounts;      /* [descArrayCount][4]: Transparent, Opaque, UnknownTransparent, UnknownOpaque micro-triangles of each OMM block */
    uint32_t* referenceCounts;  /* [descArrayCount]: primitives whose index entry selects the block */
    float*    knownFraction;    /* [indexCount]: per primitive, see above */
} ommxDeviceStatsOutputs;
OMM_MI355X_API ommResult ommxDebugGetStatsDevice(ommBaker baker, const ommCpuBakeResultDesc* deviceResult,
                                                 const float* deviceTriangleAreas,            /* indexCount floats in HBM, or NULL */
                                                 const ommxDeviceStatsOutputs* outputs,       /* or NULL */
                                                 ommDebugStats* out, uint32_t* outSkippedPrimitives /* or NULL */, void* hipStream);
OMM_MI355X_API ommResult ommxGetDeviceBakeResultTriangleAreas(ommxDeviceBakeResult result, const float** deviceAreas);
OMM_MI355X_API ommResult ommxDebugGetStatsDevice2(ommBaker baker, ommxDeviceBakeResult result, ommDebugStats* out);

/* ---- geometry from a micromap: opacity-sorted triangles for hardware without an OMM unit ----
 * ommxExtractMicroGeometry  cuts every primitive of a device-resident result into the largest sub-triangles of the bird curve whose micro-triangles
 *                        all go to one output list, so that the known-opaque part of a mesh can go into a geometry without a filter function, the
 *                        known-transparent part can be left out of the BVH, and only the remainder keeps the alpha test.  `deviceResult` is a HOST
 *                        struct as for ommxLookupOpacity / ommxDebugGetStatsDevice: the desc of ommxGetDeviceBakeResultDesc, or one the caller filled
 *                        over device copies of an ommCpuBake result.
 *   records              a record is (primitiveIndex, node), node = level << 24 | index with level <= 12 and index < 4^level: micro-triangle `index`
 *                        of subdivision level `level` of that primitive.  The micro-triangles 4j..4j+3 of level l + 1 tile micro-triangle j of level
 *                        l (the bird curve is hierarchical), so node (l, j) covers the micro-triangles [j * 4^(L-l), (j+1) * 4^(L-l)) of a block of
 *                        level L, and its vertices are ommx_micro_vertices(j, l) (include/omm_mi355x_lookup.h).
 *   the block of primitive i   entry e = indexBuffer[i] selects its block by the rule of ommx_opacity_state.  A special index -1..-4 is ONE node
 *                        (level 0, index 0) of state -(e + 1).  e >= 0 selects descArray[e].  A primitive is SKIPPED, and counted in
 *                        *outSkippedPrimitives, when e < -4, e >= descArrayCount, the level is above 12, the format is not OC1_2_State (1) /
 *                        OC1_4_State (2), or the block does not fit inside arrayDataSize: it emits nothing and nothing is read through its descriptor.
 *                        Blocks may start at any byte offset; unused bits of a one-byte block are ignored.
 *   classes              let the block have level L and E = min(L, maxEmitLevel).  A node (E, j) covers the micro-triangles
 *                        [j * 4^(L-E), (j+1) * 4^(L-E)); its class is listOfState[s] when that value is the same for the state s of every covered
 *                        micro-triangle, and mixedList otherwise.  A node (l < E, j) has class c if and only if its four children (l+1, 4j..4j+3)
 *                        all have class c; otherwise it has no class.  OMMX_GEOMETRY_DROP is a class like any other, for merging.
 *   emission and order   every node that has a class is emitted if its parent has none, or if it is the root, into the list its class names
 *                        (nothing goes anywhere for OMMX_GEOMETRY_DROP).  Within a list, records are ordered by (primitiveIndex, first covered
 *                        micro-triangle) ascending.  The outputs are a pure function of the inputs: two calls return the same bytes.
 *   presets              listOfState = { DROP, 0, 1, 1 }: opaque triangles in list 0, alpha-tested ones in list 1, transparent ones gone.
 *                        maxEmitLevel = 0 with mixedList = 1: the same partition on whole primitives, no new vertices.
 *                        The "force 2-state" ray flag: map state 2 like state 0 and state 3 like state 1.
 *   counts and capacity  outCounts[k] <- the number of records of list k, written on SUCCESS and on the capacity failure: where outputs->nodes[k] is
 *                        not NULL and capacity[k] < outCounts[k] the call returns INSUFFICIENT_SCRATCH_MEMORY with a log line, the counts reported
 *                        and NOT ONE BYTE of any output array written.  Expected use: call with outputs == NULL, allocate, call again.
 *   outputs              DEVICE memory, every member optional: nodes[k] (capacity[k] records) and primitiveOffsets[k] (indexCount + 1 entries: the
 *                        records of primitive i in list k are [off[i], off[i+1])).
 *   stream, memory       the kernels run on `hipStream` (null = the null stream), which the call synchronises before it returns -- the counts are
 *                        host values.  Scratch comes from the baker's device pool and is back there when the call returns.
 *   result codes         judged before the device is touched: a null baker, deviceResult, desc or outCounts, a baker of unknown type, an unknown
 *                        indexFormat, a listOfState[] / mixedList value that is neither 0..3 nor OMMX_GEOMETRY_DROP, non-zero reserved bytes ->
 *                        INVALID_ARGUMENT.  indexCount == 0 -> SUCCESS with zero counts and no launch.  Null arrays with non-zero counts ->
 *                        INVALID_ARGUMENT as in ommxDebugGetStatsDevice.  Without a usable device -> FAILURE.
 * ommxExpandMicroNodes   records -> vertices, one grid-stride kernel enqueued on `hipStream`; allocates nothing and synchronises nothing, like
 *                        ommxLookupOpacity.  count == 0 is SUCCESS without a launch.
 *   outBarycentrics      [count][3][2]: ommx_micro_vertices(node & 0xFFFFFF, node >> 24) of every record -- positive orientation in (u, v), hence
 *                        the winding of the primitive.  Callers interpolate their other attributes with these.
 *   outPositions         [count][3][3]: for each vertex (u, v) and component c, w = (1.f - u) - v and P.c = (V0.c * w + V1.c * u) + V2.c * v in fp32,
 *                        one rounding per operation, V0..V2 in index-buffer order.  A vertex at a corner of the primitive therefore equals that
 *                        corner and vertices shared by nodes of ONE primitive are bit-identical.  A vertex on an edge between two primitives is
 *                        computed from different corners on each side, and merged nodes leave T-junctions inside a primitive: the triangles are
 *                        not watertight.
 *   malformed records    a record whose node has a level above 12 or an index >= 4^level, or (with `mesh`) a primitiveIndex >= triangleCount, gets
 *                        0x7FC00000 in every float it owns; the mesh is not read for it.
 *   result codes         outPositions without mesh, an unknown mesh indexFormat, a stride below 12 or no multiple of 4, null nodes with count > 0,
 *                        null mesh arrays where they would be read -> INVALID_ARGUMENT. */
#define OMMX_GEOMETRY_DROP 0xFFu
typedef struct ommxMicroNode { uint32_t primitiveIndex; uint32_t node; } ommxMicroNode;   /* node = level << 24 | index; level <= 12, index < 4^level */
typedef struct ommxMicroGeometryDesc {
    uint8_t  listOfState[4];   /* ommOpacityState 0..3 -> output list 0..3, or OMMX_GEOMETRY_DROP */
    uint8_t  mixedList;        /* list (or DROP) of a node at maxEmitLevel whose micro-triangles map to different lists */
    uint8_t  reserved[3];      /* must be 0 */
    uint32_t maxEmitLevel;     /* no node deeper than this is emitted; >= 12: no limit */
} ommxMicroGeometryDesc;
typedef struct ommxMicroGeometryOutputs {     /* DEVICE memory; every member optional */
    ommxMicroNode* nodes[4];   uint64_t capacity[4];   /* records of list k */
    uint64_t*      primitiveOffsets[4];                /* [indexCount + 1]: records of primitive i in list k are [off[i], off[i+1]) */
} ommxMicroGeometryOutputs;
OMM_MI355X_API ommResult ommxExtractMicroGeometry(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxMicroGeometryDesc* desc,
                                                  const ommxMicroGeometryOutputs* outputs /* NULL: count only */, uint64_t outCounts[4],
                                                  uint32_t* outSkippedPrimitives /* or NULL */, void* hipStream);
typedef struct ommxMicroMeshDesc {         /* the mesh the result was baked from, in DEVICE memory */
    const void* positions;  uint32_t positionStrideInBytes;   /* 3 floats per vertex; stride >= 12 and a multiple of 4; 0 = 12 */
    const void* indexBuffer; ommIndexFormat indexFormat; uint32_t triangleCount;
} ommxMicroMeshDesc;
OMM_MI355X_API ommResult ommxExpandMicroNodes(const ommxMicroNode* nodes, uint64_t count, const ommxMicroMeshDesc* mesh /* NULL if outPositions is */,
                                              float* outBarycentrics /* [count][3][2] or NULL */, float* outPositions /* [count][3][3] or NULL */, void* hipStream);

/* ---- a coarser micromap from a finer one: cap a device-resident result's subdivision level ----
 * ommxCoarsenMicromap    makes a new device-resident result in which no block is finer than maxSubdivisionLevel, from the bits of the source alone:
 *                        no texture, no UVs, no classification.  For a lower level of detail (distant instances, a cheaper BLAS); for a memory
 *                        budget see ommxFitMicromap, which caps block by block.  `deviceResult` is a HOST struct over DEVICE arrays as for ommxLookupOpacity /
 *                        ommxDebugGetStatsDevice / ommxExtractMicroGeometry; the source is not modified.  The output is an ordinary
 *                        ommxDeviceBakeResult: ommxGetDeviceBakeResultDesc reads it, the lookup, resolve, stats and geometry entries accept it,
 *                        ommxDestroyDeviceBakeResult destroys it; its memory comes from the baker's device pool.  It carries no triangle areas
 *                        (ommxGetDeviceBakeResultTriangleAreas gives NULL, as for sharded results).  The outputs are a pure function of the
 *                        inputs: two calls return the same bytes.
 *   source blocks        entry e = indexBuffer[i] selects the block of primitive i by the rule of ommx_opacity_state.  A special index -1..-4
 *                        passes through unchanged under every flag.  A primitive is SKIPPED when e < -4, e >= descArrayCount, the level is above
 *                        12, the format is not OC1_2_State (1) / OC1_4_State (2), or the block does not fit inside arrayDataSize: nothing is read
 *                        through its descriptor, its output entry is -4 (FullyUnknownOpaque), and it is counted in skippedPrimitives.  Descriptors
 *                        that no primitive selects are dropped.  Blocks may start at any byte offset; unused bits of a one-byte block are ignored
 *                        on input and are zero on output.
 *   the level            a block of level L becomes a block of level T = min(L, maxSubdivisionLevel) of the same format.  The micro-triangles
 *                        4j..4j+3 of level l + 1 tile micro-triangle j of level l (the bird curve is hierarchical), so output micro-triangle j
 *                        covers the source micro-triangles [j * 4^(L-T), (j+1) * 4^(L-T)).
 *   the state, 4-state   with side = s & 1 and unknown = s >> 1 of every covered state s: if the covered states differ in side, the output state is
 *                        mixedState; otherwise it is side | (any unknown ? 2 : 0).  So {T} -> T, {O} -> O, {T, UT} -> UT, {O, UO} -> UO, anything
 *                        that holds both sides -> mixedState.  A region is known only if all of it was known: the result is conservative.  The
 *                        rule is associative: applied level by level it gives the same answer.
 *   the state, 2-state   all covered states 0 -> 0, all 1 -> 1, otherwise mixedState & 1 (the format cannot express "unknown"; the bake maps
 *                        unknown states the same way).
 *   uniform blocks       an output block whose states all equal s is uniform.  Without DisableSpecialIndices it is not emitted and its primitives
 *                        get the entry -(s + 1); this holds for blocks with L <= T too.
 *   duplicates           without DisableDuplicateDetection two output blocks are one when level, format and every byte are equal.  A 64-bit
 *                        digest of the bytes, keyed with level and format, finds ONE candidate per block -- the block with the lowest SOURCE
 *                        descriptor index under the same key -- and level, format and bytes confirm it.  The representative of a class is its
 *                        member with the lowest source descriptor index.  A block that shares its key with a lower block of other bytes (a
 *                        collision: never seen on baked data, but constructible) is kept, and so is every later block equal to it: each is
 *                        compared with the same candidate only.  That is a loss of compression, never a wrong state, and deterministic.  A
 *                        source descriptor selected by several primitives is always reduced once and yields one block, with or without the flag.
 *   order, offsets       output descriptors are ordered by block size in bytes descending, then by representative source index ascending; a
 *                        block's size is max(1, 4^T * bits / 8).  Blocks are packed without gaps from offset 0; sizes are powers of two in
 *                        descending order, so every block is naturally aligned.  An output larger than a 32-bit descriptor offset can express
 *                        (possible only with detection disabled and overlapping source descriptors) is FAILURE with a log line.
 *   index buffer         indexCount entries in the source's indexFormat (8, 16 and 32 bits are accepted, as in the lookup): the special index of
 *                        a source special, a skipped primitive or a promoted block, otherwise the output descriptor of the block's
 *                        representative.  The output never has more descriptors than the source, so the entries fit.
 *   histograms           descArrayHistogram counts output descriptors per (level, format); indexHistogram counts primitives with an entry >= 0
 *                        per (level, format) of the selected block.  Zero counts are omitted.
 *   info                 see ommxCoarsenInfo.  With default flags referencedBlocks == descArrayCount + uniformBlocks + duplicateBlocks.  With
 *                        outResult == NULL the same numbers are computed and no output arrays are allocated or written -- to learn the size of
 *                        a level before building it.
 *   stream, memory       the kernels run on `hipStream` (null = the null stream), which the call synchronises before it returns.  Scratch comes
 *                        from the baker's device pool and is back there when the call returns.  *outResult is written on SUCCESS only.
 *   result codes         judged before the device is touched, each INVALID_ARGUMENT with a log line of its own: a null baker, deviceResult or
 *                        desc, outResult and outInfo both null, a baker of unknown type, an unknown indexFormat, a mixedState other than 2 or 3,
 *                        unknown flag bits, non-zero reserved bytes, null arrays with non-zero counts as in ommxDebugGetStatsDevice.
 *                        indexCount == 0 -> SUCCESS without a launch: the info is all zeros and *outResult is an empty result that can be
 *                        destroyed.  Without a usable device, or when device memory runs out -> FAILURE with a log line. */
typedef enum ommxCoarsenFlags {
    ommxCoarsenFlags_None                      = 0,
    ommxCoarsenFlags_DisableSpecialIndices     = 1,  /* uniform blocks stay blocks */
    ommxCoarsenFlags_DisableDuplicateDetection = 2   /* equal blocks are not merged */
} ommxCoarsenFlags;
typedef struct ommxCoarsenDesc {
    uint32_t maxSubdivisionLevel;  /* no block of the output is finer than this; >= 12: no limit */
    uint8_t  mixedState;           /* 2 (UnknownTransparent) or 3 (UnknownOpaque): see "the state" */
    uint8_t  reserved[3];          /* must be 0 */
    uint32_t flags;                /* ommxCoarsenFlags */
} ommxCoarsenDesc;
typedef struct ommxCoarsenInfo {
    uint64_t arrayDataSize;        /* of the output */
    uint32_t descArrayCount;       /* of the output */
    uint32_t referencedBlocks;     /* valid source descriptors that at least one primitive selects */
    uint32_t coarsenedBlocks;      /* of those: level > maxSubdivisionLevel */
    uint32_t uniformBlocks;        /* of those: every output state equal (promoted to a special index unless disabled) */
    uint32_t duplicateBlocks;      /* of those: merged into another block's output */
    uint32_t skippedPrimitives;
} ommxCoarsenInfo;
OMM_MI355X_API ommResult ommxCoarsenMicromap(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxCoarsenDesc* desc,
                                             ommxDeviceBakeResult* outResult /* NULL: info only */, ommxCoarsenInfo* outInfo /* or NULL */, void* hipStream);

/* ---- a micromap under a byte budget: per-block levels from what every block would keep ----
 * Three entries, each usable on its own; ommxFitMicromap is the first followed by a plan on the host followed by the second.  All take `deviceResult`
 * as ommxCoarsenMicromap does (a HOST struct over DEVICE arrays, not modified), select blocks by its "source blocks" rule, run their kernels on
 * `hipStream` (null = the null stream), which the call synchronises before it returns, and take their scratch from the baker's device pool.  The
 * outputs are pure functions of the inputs: every counter is an integer, no float is ever summed, two calls return the same bytes.  This is NOT the
 * bake's maxArrayDataSize (ommCpuBakeInputDesc), whose serial host algorithm and answers stay as they are; the rule here is its own, stated below.
 *
 * ommxProfileMicromapLevels   for every source descriptor d and every level t, what block d would keep if it were coarsened to level t.
 *   rows of zeros        for a descriptor d that no primitive selects, or that fails the bounds rule, every output row of d is zero.
 *   counts               for a selected block of level L and t in 0..L: knownCounts[d][t] is the number of level-t micro-triangles j whose covered
 *                        source states [j * 4^(L-t), (j+1) * 4^(L-t)) are all known (state < 2) and all of one side; knownOpaqueCounts[d][t] counts
 *                        those whose side is 1.  For t > L both are 0.  The states of a 2-state block are 0 or 1, so a group of such a block is known
 *                        exactly when it is not mixed.  Unused bits of a one-byte block are ignored.  The counts do not depend on a mixedState: a mixed
 *                        group is unknown under either value.  At t = L the two numbers are T + O and O of ommxDebugGetStatsDevice's stateCounts[d].
 *                        knownCounts[d][t-1] * 4 <= knownCounts[d][t]: a known parent has four known children.
 *   referenceCounts      referenceCounts[d] is the number of primitives that select d.
 *   weights              devicePrimitiveWeights: indexCount floats in DEVICE memory (ommxGetDeviceBakeResultTriangleAreas, or the caller's world-space
 *                        areas), read on `hipStream`.  A weight that is not a finite positive number counts as 0.  M is the largest weight left, over
 *                        all indexCount primitives.  M == 0: every q_i = 0 and weightExponent = 0.  Otherwise M = m * 2^e with 1 <= m < 2,
 *                        weightExponent = e and q_i = (uint64_t)floor((double)w_i * 2^(31-e)), exact in fp64 and below 2^32.  blockWeights[d] is the
 *                        sum of q_i over the primitives that select d, in 64-bit integers; it cannot overflow.  With devicePrimitiveWeights == NULL
 *                        every q_i = 1 and weightExponent = 0, so blockWeights[d] == referenceCounts[d].
 *   outputs              DEVICE memory, every member optional; blockWeights 8-byte aligned, the others 4-byte aligned.
 *   result codes         judged before the device is touched, each INVALID_ARGUMENT with a log line of its own: a null baker or deviceResult, outputs
 *                        and outInfo both null, a baker of unknown type, an unknown indexFormat, null arrays with non-zero counts.  indexCount == 0 ->
 *                        SUCCESS without a launch: the info is all zeros and no output array is written.  Without a usable device, or when device
 *                        memory runs out -> FAILURE with a log line.
 *
 * ommxCoarsenMicromapLevels   ommxCoarsenMicromap with a cap per source block: everything is as there, except that block d of level L_d becomes a block
 *                        of level T_d = min(L_d, desc->maxSubdivisionLevel, deviceBlockLevels[d]).  deviceBlockLevels: descArrayCount bytes in DEVICE
 *                        memory, read on `hipStream`; a value of 12 or more means no limit from that source; entries of descriptors that are unselected
 *                        or invalid have no effect.  With deviceBlockLevels == NULL the output is byte for byte ommxCoarsenMicromap's.
 *                        coarsenedBlocks counts the blocks with L_d > T_d.
 *
 * ommxFitMicromap        a new device-resident result of at most desc->maxArrayDataSize bytes of arrayData, every block at the level the plan gives it.
 *   the plan             every selected block d has its level L_d, its format's bits b_d (1 or 2), its weight W_d = blockWeights[d] and its two profile
 *                        rows, all as ommxProfileMicromapLevels gives them for devicePrimitiveWeights.
 *                          size(d,t)  = 0 if special indices are enabled and either t == 0, or knownCounts[d][t] == 4^t with knownOpaqueCounts[d][t]
 *                                       equal to 0 or 4^t (the block is promoted); otherwise max(1, 4^t * b_d / 8).
 *                          value(d,t) = W_d * knownCounts[d][t] * 4^(12-t), an unsigned 128-bit integer: weight times known share.
 *                        Start: t_d = min(L_d, maxSubdivisionLevel), total = sum of size(d, t_d) = unfittedArrayDataSize.  A block is a candidate while
 *                        t_d > 0 and ds = size(d, t_d) - size(d, t_d - 1) > 0; its loss is dv = value(d, t_d) - value(d, t_d - 1) >= 0.  While
 *                        total > maxArrayDataSize: the candidate with the smallest dv / ds -- compared by cross-multiplication in 128 bits (every product
 *                        is below 2^114), ties to the lower descriptor index -- goes down one level (t_d -= 1, total -= ds, steps += 1).  The sequence of
 *                        steps does not depend on the budget, which only says where it stops: the levels are monotone in the budget.  Duplicates and
 *                        blocks uniform in an unknown state are not anticipated, so the output's arrayDataSize can only come out at or below
 *                        plannedArrayDataSize.  The plan runs on the host, on 116 bytes per source descriptor read back from the profile.
 *   infeasible           no candidate left and total still above the budget (possible only with DisableSpecialIndices): FAILURE with a log line;
 *                        nothing is written, *outResult included.
 *   the output           byte for byte ommxCoarsenMicromapLevels(source, the plan's levels, { 12, mixedState, flags }).  outDeviceBlockLevels[d]
 *                        (DEVICE memory, descArrayCount bytes) is the level of block d, or 0xFF for a descriptor that is unselected or invalid.
 *   result codes         as ommxCoarsenMicromap, with ommxFitDesc in the place of ommxCoarsenDesc; refused only when outDeviceBlockLevels, outResult
 *                        and outInfo are all null.  indexCount == 0 -> SUCCESS without a launch: the info is all zeros, *outResult is an empty result,
 *                        outDeviceBlockLevels is not written. */
#define OMMX_PROFILE_LEVELS 13
typedef struct ommxLevelProfileOutputs {   /* DEVICE memory, every member optional */
    uint32_t* knownCounts;        /* [descArrayCount][OMMX_PROFILE_LEVELS] */
    uint32_t* knownOpaqueCounts;  /* [descArrayCount][OMMX_PROFILE_LEVELS] */
    uint32_t* referenceCounts;    /* [descArrayCount] */
    uint64_t* blockWeights;       /* [descArrayCount] */
} ommxLevelProfileOutputs;
typedef struct ommxLevelProfileInfo {
    uint32_t referencedBlocks;     /* valid source descriptors that at least one primitive selects */
    uint32_t skippedPrimitives;
    int32_t  weightExponent;       /* e of "weights" */
    uint32_t reserved;             /* 0 */
} ommxLevelProfileInfo;
OMM_MI355X_API ommResult ommxProfileMicromapLevels(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const float* devicePrimitiveWeights /* indexCount floats or NULL */,
                                                   const ommxLevelProfileOutputs* outputs /* or NULL */, ommxLevelProfileInfo* outInfo /* or NULL */, void* hipStream);
OMM_MI355X_API ommResult ommxCoarsenMicromapLevels(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const uint8_t* deviceBlockLevels /* [descArrayCount] or NULL */,
                                                   const ommxCoarsenDesc* desc, ommxDeviceBakeResult* outResult /* NULL: info only */, ommxCoarsenInfo* outInfo /* or NULL */,
                                                   void* hipStream);
typedef struct ommxFitDesc {
    uint64_t     maxArrayDataSize;         /* the output's arrayDataSize is at most this */
    const float* devicePrimitiveWeights;   /* as in ommxProfileMicromapLevels; NULL: every primitive counts 1 */
    uint32_t     maxSubdivisionLevel;      /* a global cap applied first; >= 12: none */
    uint8_t      mixedState;               /* 2 or 3, as ommxCoarsenDesc::mixedState */
    uint8_t      reserved[3];              /* must be 0 */
    uint32_t     flags;                    /* ommxCoarsenFlags */
} ommxFitDesc;
typedef struct ommxFitInfo {
    ommxCoarsenInfo result;                /* what ommxCoarsenMicromapLevels reports for the chosen levels */
    uint64_t unfittedArrayDataSize;        /* the plan's size before its first step */
    uint64_t plannedArrayDataSize;         /* the plan's size after its last step: <= maxArrayDataSize, >= result.arrayDataSize */
    uint64_t steps;                        /* single-level steps taken */
} ommxFitInfo;
OMM_MI355X_API ommResult ommxFitMicromap(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxFitDesc* desc, uint8_t* outDeviceBlockLevels /* [descArrayCount] or NULL */,
                                         ommxDeviceBakeResult* outResult /* NULL: info only */, ommxFitInfo* outInfo /* or NULL */, void* hipStream);

/* ---- one conservative micromap from several results over the same primitives ----
 * ommxCombineMicromaps   makes a new device-resident result that is safe wherever EVERY source is: a micro-triangle is known only where all sources
 *                        know it and agree.  For a BLAS that is built once and used under several alpha tests: the bakes at the lowest and the highest
 *                        cut-off of an animated alphaCutoff (alpha against a cut-off is monotonic, so what both ends agree on holds in between),
 *                        bakes of several mips, flipbook frames or material variants on the same triangles, or bakes of the same mesh at different
 *                        subdivision levels ("level 9 where the texture needs it, the level-7 answer elsewhere").  Nothing is downloaded: it is a
 *                        streaming pass over bits that are already in device memory.
 *   sources              resultCount is 1..OMMX_COMBINE_MAX_SOURCES.  Each element of deviceResults is a HOST struct over DEVICE arrays as for
 *                        ommxCoarsenMicromap.  All sources have the same indexCount: they describe the same primitives, and primitive i is the same
 *                        triangle in each.  Index formats (8, 16 and 32 bits) may differ between sources.  The same source may be given more than
 *                        once.  No source is modified.
 *   tuple of primitive i (e_0 .. e_{K-1}) with e_k = source k's index entry.  An entry -1..-4 is the uniform state -(e + 1) at level 0.  An entry
 *                        >= 0 selects a block by the bounds rule of omm_mi355x_lookup.h.  If any e_k fails that rule -- an entry below -4, an entry at
 *                        or beyond descArrayCount, a level above 12, a format other than 1 or 2, a block outside arrayDataSize -- the primitive is
 *                        SKIPPED: nothing is read through any of its descriptors, its output entry is -4, and it counts once in skippedPrimitives.
 *   the level            T is the maximum level over the blocks of the tuple.  Output micro-triangle j of level T reads micro-triangle
 *                        j >> 2(T - L_k) of a source block of level L_k (the bird curve is hierarchical), and the one state of a special entry.
 *   the state            source states are 0..3; a 2-state block gives 0 or 1.  With side = s & 1 over the K states: if the sides differ,
 *                        r = mixedState; otherwise r = side | (any s >> 1 ? 2 : 0).  An output of format 2 stores r; an output of format 1 stores
 *                        r & 1, which is ommx_force_2state(r).  The rule is symmetric and associative (the join of ommxCoarsenMicromap's rule).
 *   only special entries no block is made: the output entry is -(r + 1) for format 2 and -((r & 1) + 1) for format 1.
 *   uniform blocks       an output block whose states all equal s is always promoted: it is not emitted and its primitives get the entry -(s + 1).
 *   duplicates           two output blocks are one when their level and every byte are equal.  A 64-bit digest of the bytes, keyed with the level,
 *                        finds ONE candidate per block -- the block under the same key whose tuple has the lowest primitive index -- and level
 *                        and bytes confirm it.  A block that shares its key with a lower block of other bytes is kept, and so is every later
 *                        block equal to it: each is compared with the same candidate only -- a loss of compression, never a wrong state, and
 *                        deterministic.  The representative of a class is the member whose lowest primitive index is lowest.
 *   order, offsets       output descriptors are ordered by block size in bytes descending, then by the representative's lowest primitive index
 *                        ascending.  Blocks are packed from offset 0 without gaps; a block's size is max(1, 4^T * bits / 8), and the unused bits of a
 *                        one-byte block are zero.  An arrayDataSize above what a 32-bit descriptor offset can express is FAILURE with a log line.
 *   index buffer         indexCount entries, always ommIndexFormat_UINT_32: the output can have more descriptors than any one source.
 *   histograms           as in ommxCoarsenMicromap: descArrayHistogram counts output descriptors per (level, format), indexHistogram counts
 *                        primitives with an entry >= 0 per (level, format) of the selected block.  Zero counts are omitted.
 *   purity               the output is a pure function of the inputs: two calls return the same bytes, and any permutation of the sources returns
 *                        the same bytes.
 *   outResult            an ordinary ommxDeviceBakeResult from the baker's device pool.  It carries no triangle areas and is accepted by the
 *                        lookup, resolve, stats, geometry and coarsen entries and by ommxCombineMicromaps itself.
 *   info                 see ommxCombineInfo.  With outResult == NULL the same info is computed and no output arrays are allocated.
 *                        combinedTuples == descArrayCount + uniformBlocks + duplicateBlocks.
 *   stream, memory       the kernels run on `hipStream` (null = the null stream), which the call synchronises before it returns.  Scratch comes
 *                        from the baker's device pool and is back there when the call returns.  *outResult is written on SUCCESS only.
 *   result codes         judged before the device is touched, each INVALID_ARGUMENT with a log line of its own: a null baker, a baker of unknown
 *                        type, null deviceResults, null desc, resultCount 0 or above 16, a null element of deviceResults, outResult and outInfo
 *                        both null, a format other than 1 or 2, a mixedState other than 2 or 3, non-zero flags, non-zero reserved bytes, an unknown
 *                        indexFormat in any source, indexCount values that differ between sources, null arrays with non-zero counts as in
 *                        ommxCoarsenMicromap.  indexCount == 0 -> SUCCESS without a launch: the info is all zeros and *outResult is an empty result
 *                        that can be destroyed.  Without a usable device, or when device memory runs out -> FAILURE with a log line. */
#define OMMX_COMBINE_MAX_SOURCES 16
typedef struct ommxCombineDesc {
    uint32_t format;        /* ommFormat_OC1_2_State (1) or ommFormat_OC1_4_State (2): the format of EVERY output block */
    uint8_t  mixedState;    /* 2 (UnknownTransparent) or 3 (UnknownOpaque), as ommxCoarsenDesc::mixedState */
    uint8_t  reserved[3];   /* must be 0 */
    uint32_t flags;         /* must be 0 (room to grow) */
} ommxCombineDesc;
typedef struct ommxCombineInfo {
    uint64_t arrayDataSize;      /* of the output */
    uint32_t descArrayCount;     /* of the output */
    uint32_t combinedTuples;     /* distinct tuples of source entries with at least one block among them (each is joined once) */
    uint32_t refinedTuples;      /* of those: at least one source block is coarser than the output block */
    uint32_t uniformBlocks;      /* of those: every output state equal -> special index */
    uint32_t duplicateBlocks;    /* of those: merged into another tuple's output */
    uint32_t skippedPrimitives;
} ommxCombineInfo;
OMM_MI355X_API ommResult ommxCombineMicromaps(ommBaker baker, const ommCpuBakeResultDesc* const* deviceResults, uint32_t resultCount,
                                              const ommxCombineDesc* desc, ommxDeviceBakeResult* outResult /* NULL: info only */,
                                              ommxCombineInfo* outInfo /* or NULL */, void* hipStream);

/* ---- one micromap from chosen primitives of several results ----
 * ommxGatherMicromaps    makes a new device-resident result whose primitives are CHOSEN primitives of the sources, with the same bits: the one entry
 *                        that changes which primitives a result describes.  For a BLAS built from several meshes or a scene-wide OMM array (equal
 *                        blocks of different bakes become one block); for a subset or a reordering of one mesh (an LOD, a meshlet split, an index
 *                        buffer reordered after the bake, the survivors of a culling pass: descriptors that are no longer referenced leave
 *                        arrayData); and for more inputs than ommxCombineMicromaps takes.  Nothing is downloaded.
 *   sources              resultCount is 1..OMMX_GATHER_MAX_SOURCES.  Each element of deviceResults is a HOST struct over DEVICE arrays as for
 *                        ommxCombineMicromaps.  indexCount and the index formats (8, 16 and 32 bits) may differ between sources; a source may have
 *                        indexCount == 0; the same source may be given more than once.  No source is modified.  Larger scenes chain calls: the
 *                        output is an ordinary result and is accepted as a source.
 *   output primitive i   names (k, p): selection[i], or -- when selection is NULL -- the i-th primitive of the concatenation of the sources (every
 *                        primitive of source 0, then of source 1, ...).  k >= resultCount or p >= source k's indexCount: the primitive is SKIPPED.
 *                        Otherwise e = source k's index entry p.  An entry -1..-4 passes through unchanged under every flag.  An entry >= 0 selects
 *                        descArray_k[e] by the bounds rule of omm_mi355x_lookup.h.  An entry below -4, an entry at or beyond descArrayCount_k, a level
 *                        above 12, a format other than 1 or 2, a block outside arrayDataSize_k: the primitive is SKIPPED.  For a skipped primitive
 *                        nothing is read through a descriptor, its output entry is -4, and it counts once in skippedPrimitives.  The same (k, p) may
 *                        be selected many times.
 *   blocks               every distinct accepted (k, e) is one item; its block is copied with level and format unchanged.  The unused bits of a
 *                        one-byte block are ignored on input and zero on output.  One output may hold blocks of both formats.  No byte outside
 *                        [offset, offset + size) of a block is read: a block may end at the last byte of the caller's allocation.
 *   uniform blocks       as in ommxCoarsenMicromap: a block whose states all equal s is uniform; without DisableSpecialIndices it is not emitted and
 *                        its primitives get the entry -(s + 1).
 *   duplicates           as in ommxCoarsenMicromap: without DisableDuplicateDetection two blocks are one when level, format and every byte are equal.
 *                        An item's rank is (k, e) in lexicographic order.  A 64-bit digest of the bytes, keyed with level and format, finds ONE
 *                        candidate per block -- the lowest-ranked block under the same key -- and level, format and bytes confirm it; the
 *                        representative of a class is its lowest-ranked member.  A block that shares its key with a lower-ranked block of other
 *                        bytes is kept, and so is every later block equal to it -- a loss of compression, never a wrong state, and deterministic.
 *   order, offsets       output descriptors are ordered by block size in bytes descending, then by the representative's rank ascending; a block's
 *                        size is max(1, 4^level * bits / 8).  Blocks are packed without gaps from offset 0; every size is a power of two, so every
 *                        block is naturally aligned.  An arrayDataSize above what a 32-bit descriptor offset can express is FAILURE with a log line.
 *   index buffer         primitiveCount entries, always ommIndexFormat_UINT_32: the special index of a source special, a skipped primitive or a
 *                        promoted block, otherwise the output descriptor of the block's representative.
 *   histograms           as in ommxCoarsenMicromap.
 *   purity               the output is a pure function of the inputs: two calls return the same bytes.  With selection == NULL and resultCount == 1,
 *                        arrayData, descArray, both histograms and the index VALUES equal those of ommxCoarsenMicromap with maxSubdivisionLevel = 12
 *                        and the same flags on that source.
 *   outResult            an ordinary ommxDeviceBakeResult from the baker's device pool.  It carries no triangle areas and is accepted by the lookup,
 *                        resolve, stats, geometry, coarsen and combine entries and by ommxGatherMicromaps itself.
 *   info                 see ommxGatherInfo.  With default flags referencedBlocks == descArrayCount + uniformBlocks + duplicateBlocks.  With
 *                        outResult == NULL the same numbers are computed and no output arrays are allocated.
 *   stream, memory       the kernels run on `hipStream` (null = the null stream), which the call synchronises before it returns; the selection is
 *                        read there, behind whatever the caller queued on that stream.  Scratch comes from the baker's device pool and is back there
 *                        when the call returns.  *outResult is written on SUCCESS only.
 *   result codes         judged before the device is touched, each INVALID_ARGUMENT with a log line of its own: a null baker, a baker of unknown
 *                        type, null deviceResults, null desc, resultCount 0 or above 4096, a null element of deviceResults, outResult and outInfo
 *                        both null, unknown flag bits, non-zero reserved, a null selection with selectionCount != 0, an unknown indexFormat in any
 *                        source, null arrays with non-zero counts as in ommxCombineMicromaps, a sum of indexCount (NULL selection) or of
 *                        descArrayCount over the sources above 2^32 - 1.  primitiveCount == 0 -> SUCCESS without a launch: the info is all zeros and
 *                        *outResult is an empty result that can be destroyed.  Without a usable device, or when device memory runs out -> FAILURE
 *                        with a log line. */
#define OMMX_GATHER_MAX_SOURCES 4096
typedef struct ommxPrimitiveRef {
    uint32_t source;        /* index into deviceResults */
    uint32_t primitive;     /* index into that source's index buffer */
} ommxPrimitiveRef;
typedef enum ommxGatherFlags {                       /* same values and meaning as ommxCoarsenFlags */
    ommxGatherFlags_None                      = 0,
    ommxGatherFlags_DisableSpecialIndices     = 1,
    ommxGatherFlags_DisableDuplicateDetection = 2
} ommxGatherFlags;
typedef struct ommxGatherDesc {
    const ommxPrimitiveRef* selection;  /* DEVICE memory, selectionCount entries; NULL: every primitive of source 0, then of source 1, ... */
    uint32_t selectionCount;            /* must be 0 when selection is NULL */
    uint32_t flags;                     /* ommxGatherFlags */
    uint32_t reserved;                  /* must be 0 */
} ommxGatherDesc;
typedef struct ommxGatherInfo {
    uint64_t arrayDataSize;      /* of the output */
    uint32_t descArrayCount;     /* of the output */
    uint32_t primitiveCount;     /* of the output: selectionCount, or the sum of the sources' indexCount */
    uint32_t referencedBlocks;   /* distinct (source, descriptor) pairs that a selected primitive selects and the bounds rule accepts */
    uint32_t uniformBlocks;      /* of those: every state equal (promoted to a special index unless disabled) */
    uint32_t duplicateBlocks;    /* of those: merged into another block */
    uint32_t skippedPrimitives;
} ommxGatherInfo;
OMM_MI355X_API ommResult ommxGatherMicromaps(ommBaker baker, const ommCpuBakeResultDesc* const* deviceResults, uint32_t resultCount,
                                             const ommxGatherDesc* desc, ommxDeviceBakeResult* outResult /* NULL: info only */,
                                             ommxGatherInfo* outInfo /* or NULL */, void* hipStream);

/* ---- a micromap for triangles whose vertices were re-ordered ----
 * ommxReorientMicromap   makes a new device-resident result for the SAME primitives with the three vertices of each triangle in another order.  A
 *                        micromap is addressed by the barycentrics of a hit, and those follow the order of a triangle's vertices in the index buffer:
 *                        a vertex-cache optimiser or meshlet builder that rotates (a, b, c) to (b, c, a), a strip-to-list conversion that flips every
 *                        second triangle, a mirrored instance drawn with flipped winding all need the bits in another order -- a pure permutation of
 *                        what is already in HBM, where a second bake would need the texture and the UVs.  ommxGatherMicromaps moves whole
 *                        primitives; this entry re-orders inside them; chained (gather, then re-orient) they follow an index buffer that was
 *                        both reordered and rotated.  Nothing is downloaded.
 *   orientation codes    orientation o means: new vertex k is old vertex perm_o[k].
 *                            0 (0,1,2) identity      1 (1,2,0) rotation      2 (2,0,1) rotation
 *                            3 (0,2,1) reflection    4 (2,1,0) reflection    5 (1,0,2) reflection  (the winding flips)
 *                        1 and 2 are inverses of each other; 3, 4 and 5 are their own.  Primitive p has desc->deviceOrientations[p], or
 *                        desc->orientation when deviceOrientations is NULL.
 *   the state            all in integers.  Output micro-triangle j' of a block of level L has the discrete barycentrics (iu', iv', iw') of the
 *                        forward decode in ommx_micro_vertices (omm_mi355x_lookup.h), before its upright / inverted adjustment.  With
 *                        t' = (iw', iu', iv') and t[perm_o[k]] = t'[k], the source micro-triangle j is the index that the digit loop of
 *                        ommx_micro_index gives for (iu, iv, iw) = (t[1], t[2], t[0]); output state j' = source state j; level and format are
 *                        unchanged.  ommx_reorient_index(j', L, o) in omm_mi355x_lookup.h is j.  For hits, with b' = (1-u'-v', u', v') and
 *                        b[perm_o[k]] = b'[k]:  ommx_opacity_state(out, i, u', v') == ommx_opacity_state(src, i, b[1], b[2]) for every point strictly
 *                        inside a micro-triangle.  At level 1 the source indices of output indices 0..3 are  o=0: 0 1 2 3   1: 2 1 3 0   2: 3 1 0 2
 *                        3: 0 1 3 2   4: 3 1 2 0   5: 2 1 0 3.
 *   selection, skipping  e = index entry p of deviceResult.  A primitive whose orientation byte is above 5 is SKIPPED, whatever its entry.  Otherwise
 *                        the selection rule of ommxGatherMicromaps: an entry -1..-4 passes through unchanged under every orientation and flag; an
 *                        entry >= 0 selects descArray[e] by the bounds rule of omm_mi355x_lookup.h; anything else is SKIPPED.  For a skipped primitive
 *                        nothing is read through a descriptor, its output entry is -4, and it counts once in skippedPrimitives.
 *   items                every distinct accepted pair (e, o) is one item, its rank (e, o) in lexicographic order: a descriptor used under several
 *                        orientations yields several blocks.  A block that is symmetric under o equals its other item and merges with it as any
 *                        duplicate does.
 *   blocks               may start at any byte offset; no byte outside [offset, offset + size) is read; the unused bits of a one-byte block are
 *                        ignored on input and zero on output.
 *   uniform blocks, duplicates, order, offsets, histograms      as in ommxGatherMicromaps, with the rank above.
 *   index buffer         indexCount entries, always ommIndexFormat_UINT_32 (the output can have up to six times the source's descriptors).
 *   purity               two calls return the same bytes.  With deviceOrientations == NULL and orientation == 0, arrayData, descArray, both histograms
 *                        and the index VALUES equal those of ommxCoarsenMicromap with maxSubdivisionLevel = 12 and the same flags.
 *   outResult            an ordinary ommxDeviceBakeResult from the baker's device pool, accepted by every entry that takes a result, this one
 *                        included.  It carries no triangle areas: the primitives are unchanged, so the SOURCE's areas
 *                        (ommxGetDeviceBakeResultTriangleAreas) remain valid weights for it, e.g. for ommxFitMicromap.
 *   info                 see ommxReorientInfo.  With default flags referencedBlocks == descArrayCount + uniformBlocks + duplicateBlocks.  With
 *                        outResult == NULL the same numbers are computed and no output arrays are allocated.
 *   stream, memory       the kernels run on `hipStream` (null = the null stream), which the call synchronises before it returns; the orientations
 *                        are read there.  Scratch comes from the baker's device pool (with deviceOrientations it is sized for six items per source
 *                        descriptor) and is back there when the call returns.  *outResult is written on SUCCESS only.
 *   result codes         judged before the device is touched, in this order, each INVALID_ARGUMENT with a log line of its own: a null baker, a baker
 *                        of unknown type (these two without a line: there is nobody to tell), null deviceResult, null desc, outResult and outInfo
 *                        both null, unknown flag bits, non-zero reserved, orientation above 5 with deviceOrientations NULL, an unknown indexFormat,
 *                        null arrays with non-zero counts, deviceOrientations set and descArrayCount above (2^32 - 1) / 6.  indexCount == 0 ->
 *                        SUCCESS without a launch: the info is all zeros and *outResult is an empty result that can be destroyed.  Without a usable
 *                        device, or when device memory runs out -> FAILURE with a log line. */
typedef struct ommxReorientDesc {
    const uint8_t* deviceOrientations;  /* DEVICE memory, indexCount bytes, read on hipStream; NULL: `orientation` for every primitive */
    uint8_t  orientation;               /* used when deviceOrientations is NULL; must be 0..5 (checked on the host) */
    uint8_t  reserved[3];               /* must be 0 */
    uint32_t flags;                     /* ommxCoarsenFlags values: DisableSpecialIndices, DisableDuplicateDetection */
} ommxReorientDesc;
typedef struct ommxReorientInfo {
    uint64_t arrayDataSize;      /* of the output */
    uint32_t descArrayCount;     /* of the output */
    uint32_t referencedBlocks;   /* distinct accepted (descriptor, orientation) pairs */
    uint32_t reorientedBlocks;   /* of those: orientation != 0 */
    uint32_t uniformBlocks;      /* of those: every state equal (promoted to a special index unless disabled) */
    uint32_t duplicateBlocks;    /* of those: merged into another block */
    uint32_t skippedPrimitives;
} ommxReorientInfo;
OMM_MI355X_API ommResult ommxReorientMicromap(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxReorientDesc* desc,
                                              ommxDeviceBakeResult* outResult /* NULL: info only */, ommxReorientInfo* outInfo /* or NULL */,
                                              void* hipStream);

/* ---- what two results say about the same primitives: a state-by-state difference ----
 * ommxCompareMicromaps   reads two device-resident results over the same primitives side by side and counts, per primitive, how many micro-triangles
 *                        are in state sa in A and in state sb in B: a 4 x 4 confusion matrix, a relation byte and exact totals.  For checking what a
 *                        derived result promises about its source -- ommxCoarsenMicromap and ommxFitMicromap ("known only where all of it was known"),
 *                        ommxCombineMicromaps ("safe wherever every source is"), ommxGatherMicromaps ("the same bits"), ommxReorientMicromap (o, then
 *                        its inverse) -- for "what did I lose, and where" after fitting or rebaking at a lower level, and for the hard question "is
 *                        there a micro-triangle that A calls opaque and B calls transparent".  Nothing is downloaded and nothing is modified: one
 *                        streaming pass over bits that are already in device memory.
 *   sources              deviceResultA and deviceResultB are HOST structs over DEVICE arrays as for ommxCombineMicromaps.  They have the same
 *                        indexCount; index formats (8, 16 and 32 bits) may differ; A == B is allowed.
 *   pair of primitive i  (e_a, e_b), the two index entries.  The skip rule of ommxCombineMicromaps applies: if either entry is below -4 or at or
 *                        beyond descArrayCount, names a level above 12, a format other than 1 or 2, or a block outside arrayDataSize, the primitive is
 *                        SKIPPED: nothing is read through either descriptor, its relation is OMMX_RELATION_SKIPPED (0x80), its level 0xFF, its
 *                        confusion zero, and it adds to nothing but skippedPrimitives.
 *   the level            T is the maximum level over the blocks of the pair.  A special index -1..-4 is the one state -(e + 1) at level 0.
 *                        Micro-triangle j of level T reads micro-triangle j >> 2(T - L) of a block of level L (the bird curve is hierarchical).  Two
 *                        special entries give T = 0 and one field.
 *   the states           states are 0..3; a 2-state block gives 0 or 1.  Under ommxCompareFlags_Force2State every state s of both sides becomes
 *                        s & 1 (ommx_force_2state) before it is counted: only the diagonal and CONFLICT can then occur.
 *   blocks               may start at any byte address; no byte outside [offset, offset + size) of a block is read; the unused bits of a one-byte
 *                        block are ignored.
 *   confusion            confusion[i][sa][sb] is the number of level-T micro-triangles whose state is sa in A and sb in B.  Its 16 entries sum to
 *                        4^T exactly.
 *   relation             the OR of one bit for every non-zero cell off the diagonal: both states below 2 and different: CONFLICT; sa >= 2 > sb:
 *                        A_WEAKER; sa < 2 <= sb: B_WEAKER; both at or above 2 and different: HINT.  0: the two sides say the same everywhere.
 *                        "A is safe wherever B is" is exactly (relation & (OMMX_RELATION_CONFLICT | OMMX_RELATION_B_WEAKER)) == 0 for every
 *                        primitive: wherever A knows a state, B knows the same one, so A claims nothing that B does not.
 *   totals               totals[sa][sb] is the sum over the primitives that were not skipped of confusion[i][sa][sb] * 4^(12 - T_i): in units of
 *                        4^-12 of a primitive, so that levels are commensurable.  They are exact 64-bit integers (at most 2^32 * 2^24); the 16
 *                        totals sum to (indexCount - skippedPrimitives) * 4^12.  No float is summed anywhere.  Every primitive weighs the same:
 *                        weighting by area is left to the caller, who has the per-primitive matrices for it (and, for a bake's own result, the areas
 *                        of ommxGetDeviceBakeResultTriangleAreas).
 *   purity               two calls return the same bytes.  Exchanging A and B transposes every matrix and the totals and swaps the A_WEAKER and
 *                        B_WEAKER bits and counts.  No answer depends on how pairs are found: the pass streams each distinct pair once and
 *                        comparedPairs counts them (two pairs whose 64-bit hashes collide are both streamed, the later one once per primitive and
 *                        counted so; every matrix is still the pair's own).
 *   outputs              DEVICE memory, every member optional, written for every primitive, skipped ones included.
 *   stream, memory       the kernels run on `hipStream` (null = the null stream), which the call synchronises before it returns.  Scratch comes
 *                        from the baker's device pool and is back there when the call returns.  *outInfo is written on SUCCESS only.
 *   result codes         judged before the device is touched, in this order, each INVALID_ARGUMENT with a log line of its own: a null baker, a baker
 *                        of unknown type (these two without a line: there is nobody to tell), null deviceResultA, null deviceResultB, null desc,
 *                        outputs and outInfo both null, unknown flag bits, non-zero reserved, an unknown indexFormat in either source, indexCount
 *                        values that differ, null arrays with non-zero counts as in ommxCombineMicromaps, a confusion pointer that is not 16-byte
 *                        aligned.  indexCount == 0 -> SUCCESS without a launch: the info is all zeros with firstConflictPrimitive = 0xFFFFFFFF, and
 *                        no output is written.  Without a usable device, or when device memory runs out -> FAILURE with a log line. */
#define OMMX_RELATION_CONFLICT  0x01u  /* some micro-triangle is known in both and the sides differ (T vs O) */
#define OMMX_RELATION_A_WEAKER  0x02u  /* some micro-triangle is unknown in A (2, 3) and known in B (0, 1) */
#define OMMX_RELATION_B_WEAKER  0x04u  /* some micro-triangle is known in A and unknown in B */
#define OMMX_RELATION_HINT      0x08u  /* some micro-triangle is unknown in both with different hints (UT vs UO) */
#define OMMX_RELATION_SKIPPED   0x80u  /* the primitive was skipped (alone in its byte) */
typedef enum ommxCompareFlags {
    ommxCompareFlags_None        = 0,
    ommxCompareFlags_Force2State = 1
} ommxCompareFlags;
typedef struct ommxCompareDesc {
    uint32_t flags;         /* ommxCompareFlags */
    uint32_t reserved;      /* must be 0 */
} ommxCompareDesc;
typedef struct ommxCompareOutputs {      /* DEVICE memory, every member optional */
    uint8_t*  relations;    /* [indexCount] */
    uint8_t*  levels;       /* [indexCount]: T of the primitive's pair; 0xFF for a skipped primitive */
    uint32_t* confusion;    /* [indexCount][4][4], 16-byte aligned: [stateA][stateB] at level T; zeros for a skipped primitive */
} ommxCompareOutputs;
typedef struct ommxCompareInfo {
    uint64_t totals[4][4];             /* sum over the primitives that were not skipped of confusion[i] * 4^(12 - T_i) */
    uint32_t identicalPrimitives;      /* relation == 0 */
    uint32_t conflictPrimitives, aWeakerPrimitives, bWeakerPrimitives, hintPrimitives;   /* primitives with that bit */
    uint32_t skippedPrimitives;
    uint32_t comparedPairs;            /* distinct (entryA, entryB) with at least one block, each streamed once */
    uint32_t refinedPairs;             /* of those: the two blocks differ in level, or one side is a special index */
    uint32_t firstConflictPrimitive;   /* lowest primitive with CONFLICT; 0xFFFFFFFF when there is none */
    uint32_t reserved;                 /* 0 */
} ommxCompareInfo;
OMM_MI355X_API ommResult ommxCompareMicromaps(ommBaker baker, const ommCpuBakeResultDesc* deviceResultA, const ommCpuBakeResultDesc* deviceResultB,
                                              const ommxCompareDesc* desc, const ommxCompareOutputs* outputs /* or NULL */,
                                              ommxCompareInfo* outInfo /* or NULL */, void* hipStream);

/* ---- a smaller micromap from near-copies: blocks that differ in a few micro-triangles become one, conservatively ----
 * ommxMergeSimilarMicromaps  makes a new device-resident result in which 4-state blocks that are near-copies of each other share one block: the
 *                        device-resident counterpart of the SDK's near-duplicate detection (which stays what it is inside ommCpuBake), for any
 *                        result that is already in device memory -- a bake, the scene-wide array of ommxGatherMicromaps, a combined or a fitted
 *                        result.  The SDK's rule is a serial greedy walk in a seeded random order; this is a rule of this library's own that is
 *                        parallel, deterministic and conservative, in integers only.  `deviceResult` is a HOST struct over DEVICE arrays as for
 *                        ommxCoarsenMicromap; the source is not modified.  The output is an ordinary ommxDeviceBakeResult without triangle areas,
 *                        accepted by every entry that takes a result.
 *   items                source selection, the bounds rule, skipping (entry -4, counted once in skippedPrimitives), special indices passing
 *                        through and dropped unreferenced descriptors are those of ommxCoarsenMicromap ("source blocks").  Every valid source
 *                        descriptor that a primitive selects is an item; its rank is its source descriptor index.  Items of format OC1_4_State
 *                        with level >= 1 are CANDIDATES.  All other items pass through with their bits, as ommxCoarsenMicromap at
 *                        maxSubdivisionLevel 12 leaves them: the 2-state format cannot express "unknown", so a join would not be conservative.
 *   rounds               there are `rounds` rounds r = 0, 1, ...; all of them always run.  At the start of a round every live candidate i has
 *                        bits B_i of level L_i.
 *   positions            pos(L, r, j) = lowbias32(seed + 0x9E3779B9 * ((L << 16) | (r << 8) | j)) & (4^L - 1) for j < samples, all arithmetic
 *                        modulo 2^32, with lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.  Repeated
 *                        positions are allowed.
 *   key                  key_i = (uint64)L_i << 56 | sum over j of state(B_i, pos(L_i, r, j)) << 2j.  The key is exact: no hash decides who
 *                        meets whom.
 *   leader               the leader of a key is the live candidate of lowest rank with that key.
 *   absorption           a candidate i that is not the leader l of its key is absorbed iff d(B_i, B_l) * 4^(12 - L) <= maxDistance, where d is
 *                        the number of micro-triangles whose 2-bit states differ; both blocks as they were at the start of the round.  i is
 *                        compared with l only.
 *   join                 after all decisions of the round, B_l <- join(B_l, every absorbed B_i) with "the state, 4-state" of ommxCoarsenMicromap
 *                        applied to each micro-triangle across the blocks: sides differ -> mixedState, otherwise side | (any unknown ? 2 : 0).
 *                        The join is symmetric and associative, so the result does not depend on order.
 *   after a round        absorbed items are dead for good.  A leader is never absorbed in its own round.  absorbedPerRound[r] counts the items
 *                        absorbed in round r.
 *   after the rounds     root(d) is d if d was never absorbed, else the root of its leader.  The primitives of d get the block of root(d).
 *                        outDeviceBlockRoots[d] = root(d): d itself for an item that passes through or survives, 0xFFFFFFFF for a descriptor
 *                        that no primitive selects or that fails the bounds rule.  The exact merges of the tail are not reflected there.
 *   the tail             the surviving blocks go through the tail of ommxCoarsenMicromap: uniform blocks become special indices unless
 *                        DisableSpecialIndices, equal blocks merge with the lowest source index as representative, blocks are ordered by size
 *                        descending, then representative ascending, and packed from offset 0.  The index buffer is in the source's indexFormat
 *                        (the output never has more descriptors than the source).  Histograms as in ommxCoarsenMicromap.
 *   info                 see ommxMergeInfo.  With default flags referencedBlocks == descArrayCount + absorbedBlocks + uniformBlocks +
 *                        duplicateBlocks.  With outResult == NULL the same numbers are computed and no output arrays are allocated.
 *   what follows         for every micro-triangle of every primitive the output state is the source state or an unknown state: with A = the
 *                        output and B = the source, ommxCompareMicromaps shows neither CONFLICT nor B_WEAKER on any primitive.  Two calls return
 *                        the same bytes.  With maxDistance == 0 only equal blocks can be absorbed, which the tail would have merged anyway:
 *                        arrayData, descArray, the index buffer and both histograms equal those of ommxCoarsenMicromap at maxSubdivisionLevel 12
 *                        with the same flags.  A leader that absorbs many members drifts away from each of them: the loss is bounded per
 *                        comparison, not per cluster -- the totals of ommxCompareMicromaps and ommxDebugGetStatsDevice show what was lost.
 *   stream, memory       as ommxCoarsenMicromap: the kernels run on `hipStream`, which the call synchronises before it returns; scratch comes
 *                        from the baker's device pool; *outResult is written on SUCCESS only.
 *   result codes         judged before the device is touched, in this order, each INVALID_ARGUMENT with a log line of its own: a null baker, a
 *                        baker of unknown type (these two without a line), null deviceResult, null desc, outDeviceBlockRoots, outResult and
 *                        outInfo all null, an unknown indexFormat, maxDistance > 4^12, rounds > 32, samples > 28, a mixedState other than 2 or 3,
 *                        flag bits other than DisableSpecialIndices, non-zero reserved bytes, null arrays with non-zero counts.
 *                        indexCount == 0 -> SUCCESS without a launch: the info is all zeros, *outResult is an empty result, the roots are not
 *                        written.  Without a usable device, or when device memory runs out -> FAILURE with a log line. */
#define OMMX_MERGE_MAX_ROUNDS  32
#define OMMX_MERGE_MAX_SAMPLES 28
typedef struct ommxMergeDesc {
    uint32_t maxDistance;   /* in units of 4^-12 of a block: a block of level L is absorbed iff d * 4^(12-L) <= maxDistance; at most 4^12 */
    uint32_t rounds;        /* 1..32; 0 = 8 */
    uint32_t samples;       /* 1..28 sampled micro-triangles per signature; 0 = 16 */
    uint32_t seed;
    uint8_t  mixedState;    /* 2 or 3, as ommxCoarsenDesc::mixedState */
    uint8_t  reserved[3];   /* must be 0 */
    uint32_t flags;         /* ommxCoarsenFlags_DisableSpecialIndices only; any other bit -> INVALID_ARGUMENT */
} ommxMergeDesc;
typedef struct ommxMergeInfo {
    uint64_t arrayDataSize;        /* of the output */
    uint32_t descArrayCount;       /* of the output */
    uint32_t referencedBlocks;     /* valid source descriptors that a primitive selects */
    uint32_t candidateBlocks;      /* of those: OC1_4_State and level >= 1 (the only ones that take part) */
    uint32_t absorbedBlocks;       /* of those: merged into a leader in some round */
    uint32_t uniformBlocks, duplicateBlocks;   /* of the blocks left after the rounds, as in ommxCoarsenInfo */
    uint32_t skippedPrimitives;
    uint32_t absorbedPerRound[OMMX_MERGE_MAX_ROUNDS];
} ommxMergeInfo;
OMM_MI355X_API ommResult ommxMergeSimilarMicromaps(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxMergeDesc* desc,
                                                   uint32_t* outDeviceBlockRoots /* [descArrayCount], DEVICE, or NULL */,
                                                   ommxDeviceBakeResult* outResult /* NULL: info only */, ommxMergeInfo* outInfo /* or NULL */,
                                                   void* hipStream);

/* ---- a micromap drawn in texture space: which primitive, which micro-triangle and which state lies over each pixel of a viewport ----
 * ommxRasterizeMicromap  draws the primitives of a device-resident result over the alpha texture they were baked from, one sample per pixel, and counts
 *                        per pixel where a known state contradicts the alpha test at that point.  It is the view the SDK's ommDebugSaveAsImages gives
 *                        (which stays NOT_IMPLEMENTED here: that dump has no exact definition), under a rule of this library's own that is exact, and
 *                        the answer to "does this result still agree with this texture?" without a second bake.  Inputs and outputs are device memory.
 *   inputs               `deviceDesc` is the device-resident input desc as ommxResolveHits takes it (a texture of this baker, sampler, cut-off, the two
 *                        alphaCutoff* states, device texcoords and indices).  `deviceResult` is a HOST struct over DEVICE arrays as for
 *                        ommxLookupOpacity; a derived result (coarsened, fitted, combined, gathered, re-oriented) is as good as a bake's.
 *   pixels               pixel (x, y), 0 <= x < width, 0 <= y < height; row 0 is the lowest v.  Its sample point, in fp64 with one rounding per written
 *                        operation and no contraction:  stepU = ((double)uvMax[0] - (double)uvMin[0]) / (double)width,
 *                        U = (double)uvMin[0] + ((double)x + 0.5) * stepU; V likewise from uvMin[1], uvMax[1], height and y.
 *   primitives           [firstPrimitive, firstPrimitive + primitiveCount), the sum taken in 64 bits and cut to deviceDesc->indexCount / 3;
 *                        primitiveCount 0xFFFFFFFF means "to the end", 0 draws the background only.  The triangle of primitive p is A, B, C in
 *                        index-buffer order: its three texture coordinates exactly as the bake's setup reads them (UNORM16, FP16, FP32, any stride,
 *                        8-, 16- and 32-bit indices), widened to fp64.
 *   coverage             in fp64, in the written order:
 *                            wA = (Bx-U)*(Cy-V) - (By-V)*(Cx-U)      wB = (Cx-U)*(Ay-V) - (Cy-V)*(Ax-U)      wC = (Ax-U)*(By-V) - (Ay-V)*(Bx-U)
 *                            area2 = (Bx-Ax)*(Cy-Ay) - (By-Ay)*(Cx-Ax)
 *                        area2 zero or not finite: the primitive is degenerate, covers nothing and is counted (a NaN or infinite coordinate makes it
 *                        so).  Otherwise the pixel is covered iff each of wA, wB, wC is zero or has area2's sign: the closed triangle, either
 *                        winding.  The two triangles at a shared edge compute exactly negated values there, so adjacent triangles leave no gap.
 *   owner                the LOWEST covering primitive index of the range.  Barycentrics u = (float)(wB / area2), v = (float)(wC / area2): the hit
 *                        convention (1-u-v) V0 + u V1 + v V2.  state = ommx_opacity_state(deviceResult, owner, u, v) (omm_mi355x_lookup.h); the
 *                        micro-triangle is ommx_micro_index(u, v, level of the selected block), 0 for a special index.  A primitive at or beyond the
 *                        result's indexCount, or one that fails that function's bounds rule, has state OMMX_OPACITY_INVALID (0xFF) and micro-triangle
 *                        0xFFFFFFFF; nothing is read outside the arrays.
 *   alpha                mip 0 sampled at ((float)U, (float)V) with runtimeSamplerDesc, by the sampler of ommxResolveHits.  alphaTest = alphaCutoff <
 *                        alpha; c = alphaTest ? alphaCutoffGreater : alphaCutoffLessEqual.  A covered pixel with state s < 2 and (c & 1) != s is a
 *                        contradiction.  Consequences: a 2-state result contradicts by construction where the bake was unknown (it had to name a known
 *                        state for a micro-triangle the alpha edge crosses); a fresh 4-state bake is expected to contradict nowhere, since it calls a
 *                        micro-triangle known only where the alpha test is the same all over it (under the Linear filter up to the sliver finding of
 *                        DESIGN 5.12).
 *   picture              integers only.  g = (uint8)(min(max(alpha, 0), 1) * 255.f + 0.5f), NaN gives 0.  An uncovered pixel is (g, g, g, 255).  A
 *                        covered one is (lut[s] + g + 1) >> 1 per channel with the SDK's colours: Transparent (0, 0, 255), Opaque (0, 255, 0),
 *                        UnknownTransparent (255, 0, 255), UnknownOpaque (255, 255, 0), invalid (255, 128, 0); MonochromeUnknowns draws
 *                        UnknownTransparent like UnknownOpaque.  Then, in this order: c -= c >> 3 for an inverted micro-triangle (d < 0 in
 *                        ommx_micro_vertices; special indices, level 0 and invalid states are upright); c >>= 1 under HighlightReuse for a reused
 *                        block: the state is valid, the owner's entry e is >= 0 and a lower primitive of the range (and of the result's indexCount) has
 *                        the same entry.  Alpha is 255.  Contour: unless NoContour is set, a pixel is (255, 0, 0, 255) instead if its alphaTest
 *                        differs from that of (x + 1, y) or of (x, y + 1), where those exist.
 *   outputs              DEVICE memory, every member optional, tight rows ([height][width], row 0 first); a member that is set is written for every
 *                        pixel.  primitiveIds and microTriangles are 4-byte aligned.
 *   info                 exact counts: coveredPixels; pixelsPerState[s] and invalidPixels (they add up to coveredPixels); alphaAbovePixels (alphaTest
 *                        of EVERY pixel, covered or not); contradictions; drawnPrimitives (primitives of the range that own at least one pixel);
 *                        degeneratePrimitives (of the range).  The info is the same whichever outputs are asked for.
 *   purity               a pure function of its inputs: ownership is an integer minimum, every count an integer sum.  Two calls return the same bytes.
 *   stream, memory       the kernels run on `hipStream` (null = the null stream), which the call synchronises before it returns.  Scratch comes from
 *                        the baker's device pool and is back there when the call returns: an owner word per pixel when primitiveIds is not handed in,
 *                        eighteen bytes per primitive of the range, and a word per descriptor under HighlightReuse.  *outInfo is written on
 *                        SUCCESS only.
 *   result codes         judged before the device is touched, in this order, each with a log line of its own: a null baker or a handle that is no
 *                        baker's (these without a line: there is nobody to tell), null deviceDesc, null deviceResult, null desc, outputs and outInfo
 *                        both null, unknown flag bits, non-zero reserved bytes, width or height 0 or above OMMX_RASTER_MAX_SIZE, a viewport bound that
 *                        is not finite or uvMax <= uvMin on an axis, an unknown indexFormat of the result, null arrays of the result with non-zero
 *                        counts as in ommxCompareMicromaps, primitiveIds or microTriangles not 4-byte aligned -- all INVALID_ARGUMENT; then
 *                        deviceDesc is judged as ommxResolveHits judges it, with the same codes (a baker of another type, no texture, unknown sampler
 *                        enums, the checks of a bake's desc, a texture of another baker).  Without a usable device, or when device memory runs out
 *                        -> FAILURE with a log line.
 * ommxDebugSaveImagePNG  writes an 8-bit RGBA image in HOST memory (an rgba output after hipMemcpy) as a PNG file: colour type 6, filter byte 0 per row,
 *                        one zlib stream of stored blocks of at most 65 535 bytes, CRC-32 and Adler-32 computed here; no device, no third-party code.
 *                        Rows are written in memory order (row 0 of a rasterized picture, the lowest v, is the file's top row).  rowPitchInBytes 0
 *                        means 4 * width.  Null arguments, a zero size or a pitch below 4 * width -> INVALID_ARGUMENT; a file that cannot be written
 *                        -> FAILURE. */
#define OMMX_RASTER_MAX_SIZE 16384u
typedef enum ommxRasterFlags {
    ommxRasterFlags_None               = 0,
    ommxRasterFlags_NoContour          = 1,   /* do not draw the alpha test's contour */
    ommxRasterFlags_MonochromeUnknowns = 2,   /* UnknownTransparent in UnknownOpaque's colour */
    ommxRasterFlags_HighlightReuse     = 4    /* halve the colour of blocks that a lower primitive of the range uses too */
} ommxRasterFlags;
typedef struct ommxRasterDesc {
    float    uvMin[2], uvMax[2];              /* the viewport in texture coordinates: finite, uvMin < uvMax on both axes */
    uint32_t width, height;                   /* 1..OMMX_RASTER_MAX_SIZE each */
    uint32_t firstPrimitive, primitiveCount;  /* 0xFFFFFFFF: to the end */
    uint32_t flags;                           /* ommxRasterFlags */
    uint8_t  reserved[4];                     /* must be 0 */
} ommxRasterDesc;
typedef struct ommxRasterOutputs {            /* DEVICE memory, every member optional, [height][width], row 0 = lowest v */
    uint32_t* primitiveIds;                   /* the owner; 0xFFFFFFFF = no primitive */
    uint32_t* microTriangles;                 /* index within the block; 0 for a special index; 0xFFFFFFFF = no primitive or an invalid state */
    uint8_t*  states;                         /* 0..3; 0xFF = invalid (OMMX_OPACITY_INVALID); 0xFE = no primitive */
    uint8_t*  alphaTest;                      /* 0 / 1, for every pixel */
    uint8_t*  rgba;                           /* [height][width][4] */
} ommxRasterOutputs;
typedef struct ommxRasterInfo {
    uint64_t coveredPixels;
    uint64_t pixelsPerState[4];
    uint64_t invalidPixels;
    uint64_t alphaAbovePixels;
    uint64_t contradictions;
    uint32_t drawnPrimitives;
    uint32_t degeneratePrimitives;
} ommxRasterInfo;
OMM_MI355X_API ommResult ommxRasterizeMicromap(ommBaker baker, const ommCpuBakeInputDesc* deviceDesc, const ommCpuBakeResultDesc* deviceResult,
                                               const ommxRasterDesc* desc, const ommxRasterOutputs* outputs /* or NULL */,
                                               ommxRasterInfo* outInfo /* or NULL */, void* hipStream);
OMM_MI355X_API ommResult ommxDebugSaveImagePNG(const char* path, const void* hostRgba8, uint32_t width, uint32_t height,
                                               uint32_t rowPitchInBytes /* 0 = 4 * width */);

/* ---- an alpha texture from an image that is already in device memory ----
 * ommxCreateTextureDevice  ommCpuCreateTexture for texels that live in HBM: ONE channel of an interleaved (or packed single-channel) image is read where
 *                        it is; nothing is downloaded, restaged or uploaded.  The result is an ordinary ommCpuTexture, byte for byte the texture
 *                        ommCpuCreateTexture makes from the extracted channel -- same texels, same summed-area table, same serialized blob -- and is
 *                        accepted wherever a texture is: ommCpuBake, ommxBakeDevice, the sharded and multi-device bakes, ommxResolveHits,
 *                        ommCpuGetTextureDesc, ommCpuSerialize, ommCpuDestroyTexture.
 *   the source           pixel (x, y) of mip m starts at  (const char*)mips[m].deviceData + y * rowPitchInBytes + x * pixelStrideInBytes ; the channel is
 *                        the channelFormat-typed value channelOffsetInBytes into it.  Examples: A of RGBA8 = { UNORM8, 4, 3 }; A of RGBA16F =
 *                        { FP16, 8, 6 }; A of RGBA32F = { FP32, 16, 12 }; G of RGB8 = { UNORM8, 3, 1 }; a packed R8 / R16F / R32F image = { format, 0, 0 }.
 *                        Only bytes of [row start, row start + width * pixelStrideInBytes) of each row are read, and only the channel's own bytes are
 *                        used: the other channels and the pitch padding may hold anything.
 *   the texture          UNORM8 -> an ommCpuTextureFormat_UNORM8 texture of those bytes; FP32 -> an FP32 texture of those bit patterns; FP16 -> an FP32
 *                        texture holding the exact value of each half (subnormals included; a NaN stays a NaN, its payload is not promised).
 *                        flags and alphaCutoff are recorded as by ommCpuCreateTexture: alphaCutoff >= 0 gives the texture its summed-area table,
 *                        ommCpuTextureFlags_DisableZOrder only changes the layout of a serialized blob.  Mips are independent allocations of any size.
 *   memory               deviceData is device memory of the BAKER'S device (the HIP device current when the baker's first texture is created; this call
 *                        binds it if it is the first), managed memory or pinned host memory.  Each mip's first and last byte are asked of
 *                        hipPointerGetAttributes before anything is launched: pageable host memory, a pointer the runtime does not know, or memory
 *                        of another device is INVALID_ARGUMENT.
 *   stream               the reads are enqueued on `hipStream` (a hipStream_t; null = the null stream) behind whatever the caller queued there, so a
 *                        kernel or copy on that stream that produces the image needs no synchronisation.  The call synchronises the stream before it
 *                        returns: the texture is complete then and the source may be overwritten or freed.
 *   result codes         as ommCpuCreateTexture where the condition is the same (null baker / desc, a baker not of CPU type, mipCount 0 or above 17, a
 *                        width or height of 0 or above 65536, null deviceData, a channelFormat that is not one of the three) plus, each INVALID_ARGUMENT
 *                        with a log line of its own: a stride smaller than the channel; channelOffsetInBytes + the channel's size above the stride; a
 *                        stride, offset, pitch or pointer that is not a multiple of the channel's size (1, 4, 2 bytes); a non-zero pitch below
 *                        width * stride.  All of this is judged before the device is touched.  Without a usable HIP device: FAILURE (there is no CPU
 *                        fallback).  *outTexture is written on SUCCESS only. */
typedef enum ommxTexelFormat {
    ommxTexelFormat_UNORM8  = 0,
    ommxTexelFormat_FP32    = 1,
    ommxTexelFormat_FP16    = 2,   /* IEEE binary16 */
    ommxTexelFormat_MAX_NUM = 3
} ommxTexelFormat;
typedef struct ommxDeviceTextureMipDesc {
    uint32_t    width, height;
    uint32_t    rowPitchInBytes;       /* 0 = width * pixelStrideInBytes; ALWAYS bytes (ommCpuTextureMipDesc::rowPitch counts texels for Morton-Z textures) */
    const void* deviceData;            /* first pixel of the mip */
} ommxDeviceTextureMipDesc;
typedef struct ommxDeviceTextureDesc {
    ommxTexelFormat                 channelFormat;         /* type of the ONE channel that is read */
    uint32_t                        pixelStrideInBytes;    /* 0 = size of one channel (single-channel, packed) */
    uint32_t                        channelOffsetInBytes;  /* of that channel inside a pixel */
    ommCpuTextureFlags              flags;
    const ommxDeviceTextureMipDesc* mips;                  /* mip 0 first */
    uint32_t                        mipCount;
    float                           alphaCutoff;           /* >= 0: the texture carries a summed-area table of alpha > alphaCutoff; < 0: none */
} ommxDeviceTextureDesc;
OMM_MI355X_API ommResult ommxCreateTextureDevice(ommBaker baker, const ommxDeviceTextureDesc* desc, void* hipStream, ommCpuTexture* outTexture);

/* ---- an alpha texture straight from BC1..BC5 blocks ----
 * A bake must see the alpha the runtime shader samples: for a block-compressed texture that is the DECODED value, not the source art.  The MI355X has
 * no texture unit that decodes BC blocks, so these two calls decode the alpha of the blocks with a kernel and return an ordinary ommCpuTexture, accepted
 * wherever a texture is (ommCpuBake, ommxBakeDevice, the sharded and multi-device bakes, ommxResolveHits, ommCpuGetTextureDesc, ommCpuSerialize) and
 * destroyed with ommCpuDestroyTexture.  It is byte for byte the texture ommCpuCreateTexture makes from the decoded texels, summed-area table included.
 * ommxCreateTextureBC       `data` is HOST memory of any kind, as for ommCpuCreateTexture; pointers and pitches need no alignment beyond what a memcpy
 *                        needs.  The blocks are uploaded with tight rows into scratch of the baker's device pool and decoded on the null stream.
 * ommxCreateTextureBCDevice `data` is read IN PLACE from memory the baker's device can read; memory rule and the hipPointerGetAttributes check of the first
 *                        and last byte of every mip are those of ommxCreateTextureDevice.  The decode runs on `hipStream` (null = the null stream)
 *                        behind whatever the caller queued there; the stream is synchronised before the call returns, so the blocks may be
 *                        overwritten or freed then.  `data` and a non-zero pitch must be multiples of 8.
 *   the source           block (bx, by) of mip m starts at  (const char*)mips[m].data + by * rowPitchInBytes + bx * blockSize , bx < ceil(width / 4),
 *                        by < ceil(height / 4); texel i = 4 * y + x of a block, x, y in 0..3, is texel (4 * bx + x, 4 * by + y) of the mip.  Multi-byte
 *                        fields are little-endian.  Only the 8 bytes that hold the alpha are read: the colour half of a BC2 / BC3 block, the
 *                        unselected channel of BC5, the codes of texels beyond width / height in a partial block and the pitch padding may hold
 *                        anything.  A DDS file's payload is this layout with a tight pitch, mip after mip.
 *   the value            BC1  c0 = u16 at bytes 0..1, c1 = u16 at bytes 2..3, code = bits 2i..2i+1 of the u32 at bytes 4..7: byte 0 if c0 <= c1 and
 *                             code == 3, else byte 255.                                                              -> UNORM8 texture
 *                        BC2  a = bits 4i..4i+3 of the u64 at bytes 0..7: byte 17 * a.                               -> UNORM8 texture
 *                        BC3 (bytes 0..7), BC4 (the block), BC5 (bytes 0..7 for channel 0, 8..15 for channel 1)      -> FP32 texture
 *                             a0 = byte 0, a1 = byte 1, k = bits 3i..3i+2 of the 48-bit integer at bytes 2..7.  The texel is n / D:
 *                             a0 > a1:  D = 7;  k = 0: n = 7 a0;  k = 1: n = 7 a1;  k = 2..7: n = (8 - k) a0 + (k - 1) a1
 *                             else:     D = 5;  k = 0: n = 5 a0;  k = 1: n = 5 a1;  k = 2..5: n = (6 - k) a0 + (k - 1) a1;  k = 6: n = 0;  k = 7: n = 5 * 255
 *                             stored as the fp32  ((float)n / (float)D) * (1.f / 255.f) : one IEEE division, then the multiplication the
 *                             classification applies to a UNORM8 byte.  Where the code selects an integer alpha a (k = 0, 1, and 6, 7 of the second
 *                             mode) the texel is bit for bit the value the library gives the UNORM8 byte a, so such a texture bakes exactly like
 *                             the UNORM8 texture of those bytes; everywhere else it is the interpolated value "as a float", as D3D10+ defines these
 *                             formats (not rounded to a byte), within 1.5 ulp of the real quotient n / (255 D).
 *   not covered          BC7 has a call of its own, ommxCreateTextureBC7 below.  The SNORM variants of BC4 / BC5 and BC6H are not covered: decode
 *                        those yourself and use ommxCreateTextureDevice.  The enum leaves room at its end.
 *   result codes         INVALID_ARGUMENT, each with a log line of its own and judged before the device is touched: a null baker, desc or outTexture;
 *                        a baker not of CPU type; mips null with mipCount != 0; mipCount 0 or above 17; a width or height of 0 or above 65536; a
 *                        null data; a format outside the enum; a channel above 1, or non-zero for a format other than BC5; a non-zero pitch below
 *                        ceil(width / 4) * blockSize; ommxCreateTextureBCDevice only: data or a pitch that is not a multiple of 8.  After that,
 *                        ommxCreateTextureBCDevice only: a mip whose first or last byte the baker's device cannot read is INVALID_ARGUMENT, before
 *                        anything is launched.  Without a usable HIP device: FAILURE (no CPU fallback).  *outTexture is written on SUCCESS only. */
typedef enum ommxBlockFormat {
    ommxBlockFormat_BC1 = 0,   /*  8-byte blocks; alpha = the punch-through bit                              -> UNORM8 texture */
    ommxBlockFormat_BC2 = 1,   /* 16-byte blocks; alpha = the explicit 4-bit values of bytes 0..7            -> UNORM8 texture */
    ommxBlockFormat_BC3 = 2,   /* 16-byte blocks; alpha = the interpolated block of bytes 0..7               -> FP32 texture   */
    ommxBlockFormat_BC4 = 3,   /*  8-byte blocks; the one UNORM channel                                      -> FP32 texture   */
    ommxBlockFormat_BC5 = 4,   /* 16-byte blocks; channel 0 (bytes 0..7) or 1 (bytes 8..15), UNORM           -> FP32 texture   */
    ommxBlockFormat_MAX_NUM = 5
} ommxBlockFormat;
typedef struct ommxBlockTextureMipDesc {
    uint32_t    width, height;      /* TEXELS; need not be multiples of 4 (the last block column / row is partial) */
    uint32_t    rowPitchInBytes;    /* bytes from one ROW OF BLOCKS to the next; 0 = ceil(width / 4) * block size */
    const void* data;               /* first block of the mip */
} ommxBlockTextureMipDesc;
typedef struct ommxBlockTextureDesc {
    ommxBlockFormat                format;
    uint32_t                       channel;      /* BC5: 0 or 1; every other format: must be 0 */
    ommCpuTextureFlags             flags;
    const ommxBlockTextureMipDesc* mips;         /* mip 0 first; independent allocations */
    uint32_t                       mipCount;
    float                          alphaCutoff;  /* as ommCpuTextureDesc: >= 0 gives the summed-area table */
} ommxBlockTextureDesc;
OMM_MI355X_API ommResult ommxCreateTextureBC(ommBaker baker, const ommxBlockTextureDesc* desc, ommCpuTexture* outTexture);
OMM_MI355X_API ommResult ommxCreateTextureBCDevice(ommBaker baker, const ommxBlockTextureDesc* desc, void* hipStream, ommCpuTexture* outTexture);

/* ---- an alpha texture straight from BC7 blocks ----
 * BC7 is the block format for RGBA with a real alpha channel (DXGI_FORMAT_BC7_UNORM, _UNORM_SRGB: sRGB does not touch alpha).  Its decode is defined
 * exactly, an 8-bit integer per channel on which every conforming decoder agrees, so the result is always an ommCpuTextureFormat_UNORM8 texture: byte for
 * byte the texture ommCpuCreateTexture makes from the decoded alpha bytes, summed-area table included, and a bake from it is bit-exact with a bake from
 * those bytes.  It is accepted wherever a texture is (ommCpuBake, ommxBakeDevice, the sharded and multi-device bakes, ommxResolveHits,
 * ommCpuGetTextureDesc, ommCpuSerialize) and destroyed with ommCpuDestroyTexture.
 * ommxCreateTextureBC7       the host entry, as ommxCreateTextureBC: `data` is HOST memory of any kind, no alignment needed; the blocks are uploaded
 *                        with tight rows into scratch of the baker's device pool and decoded on the null stream.
 * ommxCreateTextureBC7Device the device entry, as ommxCreateTextureBCDevice: `data` is read IN PLACE from memory the baker's device can read (same memory
 *                        rule, same hipPointerGetAttributes check of the first and last byte of every mip before anything is launched), on `hipStream`
 *                        (null = the null stream) behind whatever the caller queued there; the stream is synchronised before the call returns.
 *                        `data` and a non-zero pitch must be multiples of 16: a lane reads its block with one aligned 16-byte load.
 *   the source           as ommxCreateTextureBC with 16-byte blocks: block (bx, by) of mip m starts at  (const char*)mips[m].data + by * rowPitchInBytes
 *                        + 16 * bx ; texel i = 4 * y + x of a block is texel (4 * bx + x, 4 * by + y) of the mip.  Only the alpha is decoded: the
 *                        colour fields are read only when rot != 0, and then only the one channel.  The index bits of texels beyond width / height
 *                        in a partial block and the pitch padding may hold anything.  A DDS file's payload is this layout with a tight pitch.
 *   the value            q is the 128-bit little-endian integer of the block; fields are read LSB first.
 *                        Mode m = the number of trailing zero bits of byte 0; fields start at bit m + 1.  Byte 0 == 0 (reserved): all 16 texels
 *                        are 0, as D3D defines it.  Modes 0..3: 255 everywhere.
 *                        Mode 4  rot(2), idxMode(1), R0 R1 G0 G1 B0 B1 (5 bits each), A0 A1 (6 each, at bits 38 and 44); sixteen 2-bit indices from
 *                                bit 50 (texel 0 has 1 bit: 31 bits), sixteen 3-bit indices from bit 81 (texel 0 has 2 bits: 47 bits).  idxMode == 0:
 *                                colour uses the 2-bit set and alpha the 3-bit set; idxMode == 1: the other way round.  Endpoints widen to 8 bits by
 *                                bit replication: 5 -> (v<<3)|(v>>2), 6 -> (v<<2)|(v>>4).
 *                        Mode 5  rot(2), R0 R1 G0 G1 B0 B1 (7 bits each, widened (v<<1)|(v>>6)), A0 A1 (8 each, at bits 50 and 58); 2-bit colour
 *                                indices from bit 66, 2-bit alpha indices from bit 97, each set 31 bits (texel 0 has 1 bit).
 *                        Rotation (modes 4, 5): rot swaps A with R (1), G (2) or B (3) after interpolation.  With rot != 0 the output alpha is that
 *                                colour channel, interpolated with the colour index set; with rot == 0 it is A with the alpha index set.
 *                        Mode 6  R0 R1 G0 G1 B0 B1 A0 A1 (7 bits each; A0 at bit 49, A1 at bit 56), P0 (bit 63), P1 (bit 64); alpha endpoint k is
 *                                (Ak << 1) | Pk; 4-bit indices from bit 65 (texel 0 has 3 bits).
 *                        Mode 7  part(6, bits 8..13), then R, G, B, A with four 5-bit values each in the order subset 0 endpoint 0, subset 0 endpoint
 *                                1, subset 1 endpoint 0, subset 1 endpoint 1 (A starts at bit 74), then P[4] in that order at bits 94..97.  An alpha
 *                                endpoint is v = (A << 1) | P, 6 bits, widened (v<<2)|(v>>4).  2-bit indices from bit 98; texel 0 and texel
 *                                anchor[part] have 1 bit each (30 bits).  Texel i belongs to subset (mask[part] >> i) & 1.
 *                        Interpolation  ((64 - w) * e0 + w * e1 + 32) >> 6  with the weights  2-bit: 0 21 43 64;  3-bit: 0 9 18 27 37 46 55 64;
 *                                4-bit: 0 4 9 13 17 21 26 30 34 38 43 47 51 55 60 64  (= (64 i + 1) / 3, (64 i + 3) / 7, (64 i + 7) / 15 in integer
 *                                division).
 *                        mask[64], hexadecimal, bit i is texel i:
 *                                CCCC 8888 EEEE ECC8 C880 FEEC FEC8 EC80 C800 FFEC FE80 E800 FFE8 FF00 FFF0 F000
 *                                F710 008E 7100 08CE 008C 7310 3100 8CCE 088C 3110 6666 366C 17E8 0FF0 718E 399C
 *                                AAAA F0F0 5A5A 33CC 3C3C 55AA 9696 A55A 73CE 13C8 324C 3BDC 6996 C33C 9966 0660
 *                                0272 04E4 4E40 2720 C936 936C 39C6 639C 9336 9CC6 817E E718 CCF0 0FCC 7744 EE22
 *                        anchor[64]:
 *                                15 15 15 15 15 15 15 15  15 15 15 15 15 15 15 15  15  2  8  2  2  8  8 15   2  8  2  2  8  8  2  2
 *                                15 15  6  8  2  8 15 15   2  8  2  2  2 15 15  6   6  2  6  8 15 15  2  2  15 15 15 15 15  2  2 15
 *   not covered          the colour channels of BC7 as the alpha source (modes 0..3 have three subsets), BC6H.
 *   result codes         as ommxCreateTextureBC, without the format and channel checks: INVALID_ARGUMENT, each with a log line of its own and judged
 *                        before the device is touched: a null baker, desc or outTexture; a baker not of CPU type; mips null with mipCount != 0;
 *                        mipCount 0 or above 17; a width or height of 0 or above 65536; a null data; a non-zero pitch below ceil(width / 4) * 16;
 *                        ommxCreateTextureBC7Device only: data or a pitch that is not a multiple of 16.  After that, ommxCreateTextureBC7Device only:
 *                        a mip whose first or last byte the baker's device cannot read is INVALID_ARGUMENT, before anything is launched.  Without
 *                        a usable HIP device: FAILURE (no CPU fallback).  *outTexture is written on SUCCESS only. */
typedef struct ommxBC7TextureDesc {
    ommCpuTextureFlags             flags;
    const ommxBlockTextureMipDesc* mips;        /* mip 0 first; independent allocations; 16-byte blocks */
    uint32_t                       mipCount;
    float                          alphaCutoff; /* as ommCpuTextureDesc: >= 0 gives the summed-area table */
} ommxBC7TextureDesc;
OMM_MI355X_API ommResult ommxCreateTextureBC7(ommBaker baker, const ommxBC7TextureDesc* desc, ommCpuTexture* outTexture);
OMM_MI355X_API ommResult ommxCreateTextureBC7Device(ommBaker baker, const ommxBC7TextureDesc* desc, void* hipStream, ommCpuTexture* outTexture);

#endif
