/*
 * cloudtrace.h -- C ABI of libcloudtrace.so, the MI355X (gfx950) replacement for
 * the Monte-Carlo cloud radiance estimator of marsermd/DeepestScatter.
 *
 * The reference hides its estimator behind the `ARenderer` plug-in interface
 *     class ARenderer { getCamera(); init(); render(optix::Buffer frameResultBuffer); }
 *     (src/Scene/Cameras/ARenderer.h:6-16, implementation PathTracingRenderer.cpp:14-31)
 * whose real "signature" is the set of OptiX context variables the device
 * programs read.  That interface is OptiX-typed and cannot
 * be kept literally; this header keeps its three verbs and makes the implicit
 * inputs explicit.  Every entry point cites the reference code it replaces.
 * "src/" below = DeepestScatter_DataGen/DeepestScatter_DataGen/src/.
 *
 * Conventions
 *   - plain C: pointers, sizes, PODs.  No C++/torch/HIP types in signatures.
 *   - every function returns 0 (CT_OK) or a negative CtStatus; nothing throws,
 *     nothing calls exit().  ct_last_error() gives the message of the last
 *     failure on that handle (or of the last failed ct_create when h == NULL).
 *   - a handle is NOT thread-safe (the reference is single-threaded:
 *     GuiExecutionLoop.cpp:53-60); distinct handles are independent.
 *   - image layout: row-major W x H, 4 floats (or 4 bytes) per pixel, row 0 is the
 *     BOTTOM of the picture (cameraCommon.cuh:22-25).
 *   - pointers named *_dev are device pointers valid on the handle's GPU,
 *     pointers named *_host are host pointers; `ct_download` copies device->host.
 *   - all device work is issued on one HIP stream owned by the handle (or the one
 *     given with ct_set_stream) and the *_async-free entry points return after
 *     that stream is idle.
 */
#ifndef CLOUDTRACE_H
#define CLOUDTRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CT_ABI_VERSION 1

#if defined(__GNUC__)
#define CT_API __attribute__((visibility("default")))
#else
#define CT_API
#endif

typedef enum CtStatus {
    CT_OK = 0,
    CT_E_INVAL = -1,   /* bad argument (std::invalid_argument in CloudMaterial.cpp:62) */
    CT_E_HIP = -2,     /* a HIP call or kernel failed (optix::Exception path, main.cpp:65-69) */
    CT_E_NOMEM = -3,   /* host or device allocation failed */
    CT_E_STATE = -4,   /* call order violated (e.g. render before ct_set_camera) */
    CT_E_NODEVICE = -5, /* no usable gfx950 device / extension missing */
    CT_E_RCCL = -6     /* librccl missing or a collective failed (ct_group_*) */
} CtStatus;

/* Cloud::Rendering::Mode, src/Scene/SceneDescription.h:39-44 -> program chosen in
 * CloudMaterial.cpp:51-64 */
typedef enum CtMode {
    CT_MODE_SUN_AND_SKY_ALL_SCATTER = 0, /* totalRadiance,              cloudRadianceMaterials.cu:9-66  */
    CT_MODE_SUN_MULTIPLE_SCATTER = 1,    /* multipleScatterSunRadiance, cloudRadianceMaterials.cu:72-115 */
    CT_MODE_SUN_SINGLE_SCATTER = 2       /* singleScatterSunRadiance,   cloudRadianceMaterials.cu:120-148 */
} CtMode;

/* Free-flight sampler. MARCH is the reference's estimator (cloud.cuh:77-114);
 * DELTA is Woodcock tracking over a grid of majorant cells (BASELINE.json north_star). */
typedef enum CtEstimator {
    CT_EST_MARCH = 0,
    CT_EST_DELTA = 1
} CtEstimator;

/* Which buffer ct_download / ct_device_ptr refers to. */
typedef enum CtBuffer {
    CT_BUF_MEAN = 0,       /* progressiveBuffer  float4 W*H   (Camera.cpp:46)        */
    CT_BUF_M2 = 1,         /* varianceBuffer     float4 W*H   (Camera.cpp:47)        */
    CT_BUF_FRAME = 2,      /* frameResultBuffer  float4 W*H   (Camera.cpp:45)        */
    CT_BUF_SCREEN = 3,     /* screenBuffer       uchar4 W*H   (Camera.cpp:48)        */
    CT_BUF_INSCATTER = 4,  /* inScatterBuffer    uint8  X*Y*Z (VDBCloud.cpp:70)      */
    CT_BUF_DENSITY = 5     /* density            uint8  X*Y*Z (Resources.cpp:127-141)*/
} CtBuffer;

/*
 * Everything the reference's device programs read from OptiX variable scopes,
 * as one POD (SURVEY.md section 8b "implicit inputs").
 */
typedef struct CtScene {
    uint32_t abi_version;     /* must be CT_ABI_VERSION */

    /* --- density texture: Resources::loadVolumeBuffer, src/Util/Resources.cpp:68-155 --- */
    uint32_t dims[3];         /* X,Y,Z texels, INCLUDING the 1-texel zero border (:97-101) */
    const uint8_t *density_host; /* X*Y*Z bytes, x fastest, z slowest (:127-141); copied at create */

    /* --- Cloud::Model, src/Scene/SceneDescription.h:60-83 --- */
    float cloud_size_m;       /* 7000 in main.cpp:63 */
    float mean_free_path_m;   /* 10, SceneDescription.h:80; densityMultiplier = size/mfp (VDBCloud.cpp:109) */

    /* --- Cloud::Rendering, SceneDescription.h:35-57; installers.cpp:86 --- */
    float sample_step;        /* 1/512 */
    int32_t mode;             /* CtMode */
    int32_t estimator;        /* CtEstimator */
    uint32_t max_depth;       /* MAX_DEPTH = 2000, cloudRadianceMaterials.cu:4 */

    /* --- DirectionalLight, SceneDescription.h:13-26; Sun.cpp:13-18; installers.cpp:74-101 --- */
    float light_direction[3]; /* direction the light TRAVELS; normalised twice like the reference */
    float light_color[3];     /* (1,1,1) */
    float light_intensity;    /* 1e6 */

    /* --- Camera::Settings, src/Scene/Cameras/Camera.h:20-28 --- */
    /* The largest frame ct_create accepts is 12288 x 4096 (width: the tonemap kernel keeps a row of column sums in LDS;
     * height: the seed packs x * 4096 + y); anything larger, or 0, is CT_E_INVAL. */
    uint32_t width, height;

    /* --- Mie tables: Scene::init binds them (Scene.cpp:38-40); data of Mie.cpp:8-8203 --- */
    const float *mie_host;         /* raw `mie` table,        mie_count floats */
    const float *chopped_mie_host; /* raw `choppedMie` table, mie_count floats */
    uint32_t mie_count;            /* 4096 */

    /* --- placement (new: the reference is single-GPU) --- */
    int32_t device;           /* HIP device ordinal this handle lives on */
    uint32_t shard_index;     /* this handle renders the 8x8-pixel tiles (tx,ty) with        */
    uint32_t shard_count;     /*   ct_tile_owner(tx,ty,shard_count) == shard_index; 1 = all  */

    uint32_t flags;           /* CT_FLAG_* */
} CtScene;

#define CT_FLAG_NONE 0u
#define CT_FLAG_SIMPLE_KERNEL 1u /* one thread per pixel, nested loops (A/B + cross-check only) */
#define CT_FLAG_LIGHT_NORMALIZED 2u /* light_direction already went through the reference's two
                                       normalisations (a host that mirrors installSceneSetup +
                                       DirectionalLight); use it as is */

#define CT_FLAG_SPARSE_BRICKS 4u    /* store the MARCH estimator's density bricks sparsely (only the bricks between the first and
                                       the last non-empty one of every brick row; 9.5x smaller at 1024^3, 20 % slower: for
                                       volumes whose dense bricks would not fit; identical results) */
#define CT_FLAG_VMM_BRICKS 8u       /* EXPERIMENTS BUILD ONLY (libcloudtrace_exp.so; the product's library answers CT_E_INVAL): measured and
                                       rejected in round 4 -- memory mapped in 2-MiB pieces is gathered at 0.55 of the hipMalloc rate.
                                       The same bricks with dense ADDRESSING and sparse BACKING: the dense array's virtual range
                                       is reserved (hipMemAddressReserve) and only the 2-MiB chunks that hold a non-zero texel,
                                       or lie within a few texels of one, get memory of their own; every other chunk is mapped
                                       onto one of a few shared chunks (all-zero texels, a clearance rounded down to 4, 8, 16,
                                       32, 64 or 127 texels).  The kernel and its address arithmetic are the dense ones;
                                       identical results (a smaller clearance only makes the exact free-space skip shorter) */
#define CT_FLAG_TEX_FIXED8 16u      /* filter with the reference's texture arithmetic: every linear / trilinear filter weight becomes
                                       rint(frac * 256) / 256, round to nearest even -- the 9-bit fixed point with 8 fractional bits
                                       in which the CUDA texture unit stores it -- exactly as the oracle's ORC_TEX_FIXED8 build does.
                                       A weight can round up to exactly 1.0, and that value is kept.
                                       Covers every filtered fetch: the density and the shadow volume (both estimators, the simple
                                       kernel, the shadow-volume precompute, ct_point_radiance_launch, ct_generate_scatter_samples),
                                       the phase tables of the NEE, and each pyramid level that ct_collect_descriptors reads.  Not
                                       covered: the blend between two mip levels of the descriptor sampler stays exact, as in the
                                       oracle; the CDF bisection of the scatter direction is unchanged (its weights are multiples of
                                       1/16, which the rounding keeps).  Off (the default): the exact fraction.  The experiments
                                       build's path-exchange kernels (CT_EXCHANGE) answer CT_E_INVAL. */

/* Deterministic work counters of everything rendered since create/ct_reset
 * (the algorithmic-bytes figure is built from these). */
typedef struct CtCounters {
    uint64_t paths;            /* primary rays traced (pixels x subframes in this shard) */
    uint64_t box_hits;         /* primary rays that hit the cloud's box */
    uint64_t density_lookups;  /* trilinear fetches of the density texture (8 B each) */
    uint64_t inscatter_lookups;/* trilinear fetches of the shadow volume   (8 B each) */
    uint64_t scatter_events;   /* accepted collisions = NEE evaluations */
    uint64_t depth_capped;     /* paths stopped by max_depth */
} CtCounters;

/* What the kernels actually ISSUED for the lookups above since create/ct_reset (implementation figures, not
 * the algorithm's: the MARCH estimator replays free-space steps without a fetch, walks the part of a primary
 * flight that is the same for every sample of a pixel once per pose, and reuses a lane's last shadow-volume
 * footprint; every such step is still a density/inscatter lookup of the algorithm).  bench.py builds the
 * issued-bytes roofline figure from these: 8 useful bytes per fetch. */
typedef struct CtFetchCounters {
    uint64_t density_fetches;   /* trilinear footprints of the density actually loaded by the estimator kernel */
    uint64_t inscatter_fetches; /* the same for the shadow volume */
} CtFetchCounters;

typedef struct CtHandle_ *CtHandle;

/* ---- lifetime --------------------------------------------------------------------- */

/* Scene::init for the path-tracing configuration (Scene.cpp:36-46): uploads density,
 * prepares the three Mie textures (Mie.cpp:8206-8297), publishes the Sun/VDBCloud
 * variables (Sun.cpp:13-18, VDBCloud.cpp:88-117), runs the inScatter precompute
 * (VDBCloud.cpp:57-86 -> inScatter.cu:40-66), allocates frame/progressive/variance/
 * screen buffers and clears them (Camera.cpp:45-48,77-86).  Sets the default camera
 * pose of Camera.cpp:37-39. */
CT_API int ct_create(const CtScene *scene, CtHandle *out);

/* Context destruction between tasks, GuiExecutionLoop.cpp:93-97. NULL is a no-op. */
CT_API int ct_destroy(CtHandle h);

/* Message of the last failure (UTF-8, owned by the library, valid until the next call
 * on the same handle).  h == NULL: last failure of ct_create in this thread. */
CT_API const char *ct_last_error(CtHandle h);

/* Use `hip_stream` (a hipStream_t passed as void*) for all later work on this handle
 * instead of the handle's own stream.  NULL restores the handle's stream. */
CT_API int ct_set_stream(CtHandle h, void *hip_stream);

/* ---- ARenderer verbs ----------------------------------------------------------------- */

/* ARenderer::getCamera()["eye"|"U"|"V"|"W"]->setFloat(...)   Camera.cpp:126-133 */
CT_API int ct_set_camera(CtHandle h, const float eye[3], const float U[3], const float V[3], const float W[3]);

/* Sun::init again (Sun.cpp:13-18) on a live handle: a new light without a new ct_create.  In the reference the light belongs to
 * the scene setup, not to the cloud -- Tasks::renderCloud renders every cloud under two suns (Tasks.cpp:52-65) -- and only the
 * shadow volume (VDBCloud::InitInScatter), its bricks, the shadow-zero flags of the march bricks, the shadow half of the twin
 * bricks and the uniforms lightDirection / lightColor * lightIntensity depend on it: those are rebuilt, everything else of the
 * handle (density layouts, Mie tables, frame buffers, scratch) stays.  Afterwards the handle's device state is that of a handle
 * created with the new light, and the next render call starts as that handle's first one would: the pose's pixel list and job
 * order are rebuilt and its path costs measured again, as after ct_set_camera.
 * `direction` is the direction the light travels, as CtScene::light_direction, and goes through the same two normalisations
 * unless the handle was created with CT_FLAG_LIGHT_NORMALIZED.  color == NULL keeps the handle's colour; intensity is always
 * set.  A NULL handle, a NULL, zero or non-finite direction: CT_E_INVAL, and the handle is exactly as it was (colour and
 * intensity are not checked: as at ct_create, non-finite ones only turn the shadow-zero NEE skip off).
 * Waits for the batches in flight, drops the samples rendered ahead (ct_set_render_ahead) -- no path of the old light survives
 * -- and returns when the stream is idle.  Its temporaries are allocated before anything changes: CT_E_NOMEM leaves the old
 * light in place and the handle usable.
 * Does NOT touch mean, M2, the subframe count or the counters: follow it with ct_reset, as after a camera move in the reference
 * (Camera.cpp:93-98).  What ct_set_stop_when_converged has set, a frozen image included, is likewise kept until ct_reset
 * clears it. */
CT_API int ct_set_light(CtHandle h, const float direction[3], const float color[3], float intensity);

/* ARenderer::render(frameResultBuffer) after context["subframeId"]=id  (Camera.cpp:191-195,
 * PathTracingRenderer.cpp:21-31): one path per pixel, result float4(r,g,b,1) per pixel into
 * the handle's frame buffer; if frame_rgba_dev != NULL the frame is also copied there
 * (device pointer, W*H*4 floats, caller-owned).  Pixels of other shards are written as 0
 * with alpha 0.  Seeds are tea<4>(x*4096+y, subframe_id)  (documented deviation from
 * random.cuh:38, which mixes in clock()). */
CT_API int ct_render_subframe(CtHandle h, uint32_t subframe_id, float *frame_rgba_dev);

/* updateFrameResult, progressive.cu:17-27, launched by Camera.cpp:197-199: Welford update
 * of mean/M2 with n = subframe_id from the handle's frame buffer (or from frame_rgba_dev
 * when not NULL). */
CT_API int ct_accumulate(CtHandle h, uint32_t subframe_id, const float *frame_rgba_dev);

/* The hot path of Camera::render's loop (Camera.cpp:189-200) fused: for id = first ..
 * first+count-1 { render(id); updateFrameResult(id) } with identical results, in one launch,
 * without materialising the frame buffer.  Requires first == (subframes accumulated so far)+1. */
CT_API int ct_render_accumulate(CtHandle h, uint32_t first_subframe_id, uint32_t count);

/* The same, pipelined: the call enqueues the batch on the handle's stream and returns.  With the MARCH
 * estimator a launch does not run its surviving paths to their end once its job list is empty (that tail of
 * waves carrying a few long paths each is 19 ms of a 107 ms launch at 256 subframes): it suspends them and the
 * next batch's launch resumes them first, so the accumulate kernel of batch k runs behind the launch of batch
 * k+1, and ct_synchronize() (or any entry point that waits) finishes the last batch with a launch that only
 * resumes.  Paths, arithmetic and the subframe order of the accumulation are unchanged: results are identical
 * to ct_render_accumulate's.  Every other entry point waits for the batches in flight first, except
 * ct_copy_to_device_async and ct_subframes; a copy enqueued after batch k sees the running mean up to batch
 * k-1.  (The reference is synchronous: Camera::render maps its buffers right after context->launch,
 * Camera.cpp:189-240; SURVEY section 8b asks for an _async variant.) */
CT_API int ct_render_accumulate_async(CtHandle h, uint32_t first_subframe_id, uint32_t count);
CT_API int ct_synchronize(CtHandle h);

/* Render-ahead for the reference's display cadence (Camera::render: 10 subframes, then tonemap and display,
 * Camera.cpp:189-214).  With subframes > 0, a call of ct_render_accumulate_async for FEWER subframes than that is served by
 * an estimator launch of `subframes` subframes -- a launch of 10 subframes is mostly beginning and end: every lane resumes a
 * path and suspends one, the lanes fill and drain; per subframe a launch of 80 keeps the chip busy for 21 % fewer cycles
 *  -- and every call accumulates ITS OWN share of it, in order: the images the calls produce are the
 * reference's images for those subframe counts, bit for bit, each a fixed number of calls later (the running mean follows
 * the calls by `subframes` subframes per launch a path may span; ct_synchronize and every entry point that waits bring it
 * to exactly the subframes asked for).  Samples rendered ahead and not asked for yet stay in the scratch for the next
 * calls; ct_set_camera, ct_reset, ct_set_subframes and ct_accumulate drop them, and CtCounters count them when they are
 * rendered.  0 (the default) turns it off; also CT_RENDER_AHEAD in the environment at ct_create.
 * ct_rendered_subframes: how far the estimator has been launched (>= ct_subframes). */
CT_API int ct_set_render_ahead(CtHandle h, uint32_t subframes);
CT_API int ct_rendered_subframes(CtHandle h, uint32_t *count_out);

/* Camera::reset, Camera.cpp:77-86 (clearScreen, progressive.cu:29-34): zero frame, mean, M2,
 * subframe count.  Counters are zeroed too. */
CT_API int ct_reset(CtHandle h);

/* Reinhard tonemap of the running mean: firstPass/secondPass/applyReinhard,
 * reinhard.cu:26-84, launched by Camera.cpp:202-210; default exposure 0.4 (Camera.h:90).
 * Result goes to the handle's screen buffer and, if rgba_host != NULL, is copied to the host
 * (W*H*4 bytes). avg_luminance_out (optional) receives reinhard.cu:53 averageLuminance. */
CT_API int ct_tonemap(CtHandle h, float exposure, uint8_t *rgba_host, float *avg_luminance_out);

/* The same enqueued behind the batches of ct_render_accumulate_async, without waiting: the display update of
 * Camera::render (Camera.cpp:202-210, every 10 subframes) at the reference's cadence without a host round trip per
 * update.  It tonemaps the running mean of the batches accumulated so far -- with path continuation a batch is
 * accumulated a few launches after it was enqueued (ct_synchronize brings everything up to date) -- into the handle's
 * CT_BUF_SCREEN; read it with ct_download / ct_copy_to_device after ct_synchronize, or display it from the device. */
CT_API int ct_tonemap_async(CtHandle h, float exposure);

/* Camera::isConverged, Camera.cpp:232-268, evaluated on the device.  *converged_out = 1 when
 * fewer than 500 pixels are outside the 95 % interval; *unconverged_pixels_out optional. */
CT_API int ct_is_converged(CtHandle h, int32_t *converged_out, uint64_t *unconverged_pixels_out);

/* Camera::render's `if (!isConverged())` (Camera.cpp:179) without a host round trip per update.  With cadence > 0 the
 * library enqueues the test of Camera::isConverged behind the accumulate kernel of every cadence-th subframe from
 * min_subframes on (the reference: 10 and 100, Camera.cpp:189,234) -- the accumulate kernels are cut at those counts, whatever
 * the sizes of the calls, render-ahead included -- and takes the reference's decision on the device: at the first such count
 * with fewer than 500 pixels outside the interval the running mean and M2 are FROZEN; every later accumulate kernel leaves
 * them alone.  So a host that enqueues update after update (ct_render_accumulate_async + ct_tonemap_async) and looks at
 * ct_converged_at now and then -- it never waits -- ends with exactly the image, and the subframe count, at which the
 * reference's loop stops; what it enqueued beyond that point is rendered and dropped.  ct_converged_at: *subframes_out = the
 * count the image was frozen at (0 = still running), *tested_at_out / *unconverged_pixels_out = the last test that has
 * finished (any of them may be NULL); up to date after ct_synchronize.  ct_reset and ct_set_stop_when_converged clear the
 * state; ct_is_converged after a freeze tests the frozen image with its own count.  A batch rendered in several chunks of
 * pixel groups (it did not fit the scratch) is tested at its end only.  Whole frames only: CT_E_INVAL on a shard of a
 * multi-GPU job (test the merged frame with ct_is_converged_buffers).  cadence 0 (the default) turns it off. */
CT_API int ct_set_stop_when_converged(CtHandle h, uint32_t cadence, uint32_t min_subframes);
CT_API int ct_converged_at(CtHandle h, uint32_t *subframes_out, uint32_t *tested_at_out, uint64_t *unconverged_pixels_out);

/* The same two on caller-owned device buffers of W*H float4 each: the frame a multi-GPU reduce merged on rank 0
 * (every shard's handle holds its own tiles and zeros elsewhere; the SUM of the shards' CT_BUF_MEAN / CT_BUF_M2 is
 * the whole image).  reinhard.cu:44-55 sums the luminance of the WHOLE frame in a fixed order
 * and Camera.cpp:232-268 counts over the WHOLE frame, so both run on the merged buffers, on one rank, with the
 * single-GPU arithmetic -- not as per-shard partial sums, which would change the order of the float additions.
 * `subframes` = samples per pixel the buffers hold.  The screen bytes go to the handle's CT_BUF_SCREEN as usual. */
CT_API int ct_tonemap_buffer(CtHandle h, const float *mean_rgba_dev, float exposure, uint8_t *rgba_host,
                             float *avg_luminance_out);
CT_API int ct_is_converged_buffers(CtHandle h, const float *mean_rgba_dev, const float *m2_rgba_dev, uint32_t subframes,
                                   int32_t *converged_out, uint64_t *unconverged_pixels_out);

/* ---- radiance samples: the estimator over (point, direction) tasks -------------------------- */

/* Gpu::PointRadianceTask, src/CUDA/PointRadianceTask.h:12-78 (40 bytes, same field order). */
typedef struct CtPointRadianceTask {
    int32_t id;
    uint32_t experimentCount;
    float radiance;          /* running mean of prd.result.x */
    float runningVariance;   /* running M2 */
    float position[3];       /* ray origin, world coordinates (box centred at 0) */
    float direction[3];      /* ray direction (need not be normalised) */
} CtPointRadianceTask;

/* `launches` consecutive launches of estimateEmission (src/CUDA/pointEmissionCamera.cu:20-40) over
 * tasks[0..count): for frame = first_frame_id .. first_frame_id+launches-1, thread i traces one path
 * from (position, direction) with the handle's render mode (the reference uses SunMultipleScatter,
 * Tasks.cpp:135), seed tea<4>(i*4096, frame), and folds prd.result.x into task i with
 * PointRadianceTask::addExperimentResult (:40-51), in frame order.  tasks_host is updated in place.
 * This is the device part of RadianceCollector::update (RadianceCollector.cpp:88-96); replication,
 * merging, convergence and rescheduling stay with the caller.
 * A task whose direction is zero, or whose direction or position has a component that is not finite, has no ray (a NaN sample
 * of ct_generate_scatter_samples is one): CT_E_INVAL before anything is launched, tasks_host untouched. */
CT_API int ct_point_radiance_launch(CtHandle h, CtPointRadianceTask *tasks_host, uint32_t count,
                                    uint32_t first_frame_id, uint32_t launches);

/* ---- the radiance collector on the device: RadianceCollector's loop behind the C ABI ------------------
 *
 * RadianceCollector::update (RadianceCollector.cpp:73-141) around ct_point_radiance_launch is, on the host: replicate the
 * unconverged tasks over max_thread_count threads (scheduleTasks, :176-192), launch, merge the replicas of every task with
 * PointRadianceTask::operator+= (:104-108), test the rule (:112-118), re-pack.  A CtCollector does all of that on the device; the
 * host reads one word per update, the number of tasks that go on.
 *
 * Tasks have ids 0 .. B-1 (B = count); task i has position positions_host[3 i ..] and direction directions_host[3 i ..].
 * State per id: mean, m2, count and converged_update, all 0 at create.  The live list is 0 .. B-1, ascending; frame_id is 0.
 *
 * Update u (u = 1, 2, ..) with n live tasks, in list order, T = max_thread_count, L = launches_per_update:
 *     r = T / n (integer division), threads = n r; thread i = t r + j is replica j of the t-th live task.
 *     Thread i traces frames frame_id + 1 .. frame_id + L: exactly the paths ct_point_radiance_launch traces on this handle for
 *     a task at array index i -- seed tea<4>(i * 4096, frame) -- with the handle's mode, estimator and CT_FLAG_TEX_FIXED8.
 *     Replica 0 folds its L results onto the task's (mean, m2, count), replicas j >= 1 fold theirs from (0, 0, 0), all with
 *     PointRadianceTask::addExperimentResult's arithmetic as ct_point_radiance_launch folds (float32, no contraction):
 *         N = (float)count, w = (float)(1.0 / (double)N), new_mean = mean + (x - mean) * w, m2 += (x - mean) * (x - new_mean)
 *     Merge: replicas j = 1 .. r-1 into replica 0, in that order, with PointRadianceTask::operator+= (PointRadianceTask.h:56-68):
 *         w = ((float)n1 * 1.0f) / (float)(n0 + n1)    (IEEE division, the integer sum converted once)
 *         mean = mean + (o.mean - mean) * w            (no contraction)
 *         m2 = m2 + o.m2                               (the reference omits the between-means term, and so does this)
 *         count = n0 + n1
 *     Test, on the merged triple, in float32 with IEEE division and square root:
 *         absolute = (1.96f * sqrt(m2 / N)) / sqrt(N),  relative = absolute / (mean + FLT_EPSILON),
 *         converged = relative < rel_tol || absolute < abs_tol;  if mean < FLT_EPSILON: converged = count > zero_samples
 *     (a NaN compares false).  A converged task stores converged_update[id] = u and leaves the list; the survivors keep their
 *     order.  frame_id += L.  The collector is completed when the list is empty.
 *
 * All live tasks hold the same count c at all times.  An update that would carry it beyond 2^32 - 1 (c + r L), or whose frame ids
 * would wrap, is CT_E_STATE, answered before anything of that update runs; the updates of the call before it stand.
 *
 * ct_collector_update runs up to `updates` updates and stops when the collector is completed; on a completed collector it is
 * CT_OK and launches nothing.  After k updates the state is, bit for bit, what RadianceCollector's loop with the same constants
 * leaves after k update()s over ct_point_radiance_launch on the same handle: the statistics of every task, the set converged in
 * every update, r and frame_id -- whatever the split of k over calls.
 *
 * ct_collector_download writes the B tasks in id order: id, experimentCount, radiance, runningVariance, and position and
 * direction as given; a live task carries its current merged statistics and converged_update 0.  count must equal B.
 * converged_update_host_out may be NULL.
 *
 * CtCounters, CtFetchCounters, ct_kernel_time and the armed invariants (CT_DEBUG_INVARIANTS) see the paths exactly as
 * ct_point_radiance_launch's of the same threads.  Mean, M2, frame, subframe count, samples rendered ahead and the pose's pixel
 * list are not touched.
 *
 * Everything the collector owns -- positions, directions, the three state arrays, converged_update, two live lists of B words,
 * the wave counts -- is allocated in ct_collector_create: CT_E_NOMEM there leaves the handle as it was.  The estimator's
 * scratch is the handle's, grown as for ct_point_radiance_launch.
 *
 * CT_E_INVAL, before anything changes: a NULL argument (a NULL handle is answered without a device); a wrong abi_version; T, L
 * or a tolerance out of range; count == 0 or count > T; T rounded up to 64, times L, > 2^32 - 1; a zero or non-finite direction
 * or a non-finite position (the message names the task, as ct_point_radiance_launch's); a CT_FLAG_SIMPLE_KERNEL handle; a
 * collector of another handle; updates == 0; a wrong count in ct_collector_download.
 * CT_E_STATE: an update after ct_set_light changed the handle's light (ct_collector_download still works); the two overflows.
 * ct_collector_destroy(NULL) is a no-op; destroy a collector before its handle. */
typedef struct CtCollectorDesc {
    uint32_t abi_version;         /* CT_ABI_VERSION */
    uint32_t max_thread_count;    /* T: 1 .. 2^24 (reference: 20480, RadianceCollector.cpp:17) */
    uint32_t launches_per_update; /* L: 1 .. 65535 (reference: 100, :88) */
    uint32_t zero_samples;        /* a task whose mean is < FLT_EPSILON stops once count > zero_samples (reference: 100000) */
    float    rel_tol;             /* finite, >= 0 (reference: 2e-2f) */
    float    abs_tol;             /* finite, >= 0 (reference: 1e-4f) */
} CtCollectorDesc;                /* 24 bytes */
typedef struct CtCollector_ *CtCollector;
typedef struct CtCollectorInfo {
    uint32_t batch;               /* B */
    uint32_t remaining;           /* live tasks */
    uint32_t converged;           /* B - remaining */
    uint32_t updates;             /* updates run since create */
    uint32_t frame_id;
    uint32_t repeat_count;        /* r of the next update, 0 when completed */
    uint32_t threads;             /* remaining * repeat_count */
    uint32_t completed;           /* 1: the live list is empty */
    uint64_t paths;               /* estimator paths since create */
    double   trace_ms;            /* GPU time of the last ct_collector_update call: the estimator launches, */
    double   fold_ms;             /* the rays and fold-and-merge kernels (the fold evaluates the rule), */
    double   test_ms;             /* the scans and the compacting writes */
} CtCollectorInfo;                /* 64 bytes; frame_id at 16, paths at 32, trace_ms at 40 */

CT_API int ct_collector_create(CtHandle h, const CtCollectorDesc *d, const float *positions_host, const float *directions_host,
                               uint32_t count, CtCollector *out);
CT_API int ct_collector_update(CtHandle h, CtCollector c, uint32_t updates);
CT_API int ct_collector_info(CtCollector c, CtCollectorInfo *out);
CT_API int ct_collector_download(CtCollector c, CtPointRadianceTask *tasks_host_out, uint32_t *converged_update_host_out, uint32_t count);
CT_API int ct_collector_destroy(CtCollector c);

/* ---- the adaptive frame: the progressive image with the stopping rule applied per pixel ---------------
 *
 * ct_set_stop_when_converged mirrors Camera::isConverged (Camera.cpp:232-268): every pixel of the frame gets further subframes
 * until fewer than 500 pixels fail the test, so the whole frame pays for the few pixels over the dense core.  A CtAdaptiveFrame
 * renders the handle's image, for the pose and light the handle has at ct_adaptive_frame_create, in rounds of R = round_samples
 * subframes that go only to the pixels which have not yet passed the test.  It keeps a mean, an M2 and a sample count per pixel
 * of its own; the handle's image state (frame, mean, M2, subframe count, samples rendered ahead, freeze state) and the pose's
 * pixel list are not touched.
 *
 * Pixels are p = y * width + x.  At create every pixel of the frame is live, in ascending p, and mean, M2 and count are 0.
 * All live pixels hold the same count c.  A round gives each of them subframes c + 1 .. c + R:
 *     The sample of pixel p and subframe s is ct_render_subframe's for that pixel: the pose's primary ray as for the image,
 *     seed tea<4>(x * 4096 + y, s), the handle's mode, estimator and CT_FLAG_TEX_FIXED8.
 *     The samples are folded in subframe order as ct_accumulate folds, on all four channels (float32, no contraction):
 *         w = 1.0f / (float)s,  nm = mu + (v - mu) * w,  m2 += (v - mu) * (v - nm),  mu = nm
 *     If c + R >= min_samples, the test of ct_is_converged is applied with the frame's tolerances: channel x only, in float32
 *     with IEEE division and square root, N = (float)(c + R):
 *         sigma = sqrt(m2.x / N),  abs = 1.96f * sigma / sqrt(N),  rel = abs / (mean.x + FLT_EPSILON),
 *         converged = rel < rel_tol || abs < abs_tol          (a NaN compares false)
 *     A pixel leaves the live list when it is converged, or when its count equals max_samples.  At the cap the pixels that
 *     fail the rule are kept as the capped list.  Survivors keep their ascending order.
 * So, for every pixel, (mean, M2) is bit for bit that pixel of ct_render_accumulate(h2, 1, counts[p]) on a handle h2 of the same
 * scene and pose, and counts is what the rule gives on those uniform images -- whatever the split of rounds over calls,
 * chunk_pixels or pass_subframes.
 *
 * ct_adaptive_frame_update runs at most `rounds` rounds (0: until nothing is live).  With nothing live it is CT_OK and launches
 * nothing.  ct_adaptive_frame_raise_cap sets a higher cap, a multiple of R: the capped pixels go live again, and the next
 * updates give the bits of a frame created with that cap.  ct_adaptive_frame_info may be called at any time.
 * ct_adaptive_frame_download copies CT_ADAPTIVE_MEAN or CT_ADAPTIVE_M2 (width * height float4) or CT_ADAPTIVE_COUNTS (width *
 * height uint32) to the host; `bytes` must be the exact size.  ct_adaptive_frame_device_ptr gives the device address of the
 * same arrays: ct_tonemap_buffer(h, mean, ..) and ct_is_converged_buffers work on them unchanged.
 *
 * A round's live list is traced in chunks of whole groups of 64 entries (chunk_pixels; default: at most 2^20 entries) and a
 * chunk's R subframes in passes (pass_subframes; default: at most 2^24 results per estimator launch); the fold of a round's
 * last pass evaluates the rule, a scan and a ranked write compact the survivors, and the host reads one count per round.
 * CtCounters, CtFetchCounters, ct_kernel_time and the armed invariants (CT_DEBUG_INVARIANTS) see the paths exactly as
 * ct_point_radiance_launch's.  The estimator's scratch is the handle's, grown as for ct_point_radiance_launch; everything else
 * -- mean, M2, counts, two live lists of width * height words, the wave counts -- is allocated in ct_adaptive_frame_create:
 * CT_E_NOMEM there leaves the handle as it was.
 *
 * Stopping per pixel biases a pixel's mean towards runs of low variance: a pixel whose first samples happen to agree leaves
 * early, with them.  min_samples is the guard against that -- no pixel is tested on fewer samples -- and the only one; keep the
 * reference's 100 unless the bias has been measured for the scene.
 *
 * CT_E_INVAL, before anything changes: a NULL argument (a NULL handle or frame is answered without a device); a wrong
 * abi_version; a value outside the ranges below; a CT_FLAG_SIMPLE_KERNEL handle; a shard of a multi-GPU job (shard_count > 1;
 * ct_adaptive_frame_create_shard below takes one); a cap that is not higher, or no multiple of R, or above 2^24; an unknown `which` or a wrong size.
 * CT_E_STATE: ct_adaptive_frame_update and ct_adaptive_frame_raise_cap after ct_set_camera changed the pose or after
 * ct_set_light (info, download and device_ptr still work).  Errors go to the owning handle's ct_last_error.
 * ct_adaptive_frame_destroy(NULL) is a no-op; destroy a frame before its handle. */
#define CT_ADAPTIVE_MEAN 0
#define CT_ADAPTIVE_M2 1
#define CT_ADAPTIVE_COUNTS 2
typedef struct CtAdaptiveFrameDesc {
    uint32_t abi_version;    /* CT_ABI_VERSION */
    uint32_t round_samples;  /* R: subframes per live pixel and round, 1 .. 65535 (reference cadence: 10) */
    uint32_t min_samples;    /* a pixel is tested only at counts >= this; a multiple of R, R .. max_samples (reference: 100) */
    uint32_t max_samples;    /* cap per pixel: a multiple of R, R .. 2^24 */
    float    rel_tol;        /* finite, >= 0 (reference: 2e-2f) */
    float    abs_tol;        /* finite, >= 0 (reference: 1e-2f, Camera.cpp:232-268) */
    uint32_t chunk_pixels;   /* 0 = the library's choice; else a multiple of 64: live entries per estimator launch */
    uint32_t pass_subframes; /* 0 = the library's choice; else 1 .. R: subframes per estimator launch */
} CtAdaptiveFrameDesc;       /* 32 bytes */
typedef struct CtAdaptiveFrame_ *CtAdaptiveFrame;
typedef struct CtAdaptiveFrameInfo {
    uint32_t width, height, round_samples, min_samples, max_samples, rounds;
    float    rel_tol, abs_tol;                       /* 32 bytes so far */
    uint64_t pixels, live, converged, capped, paths; /* pixels = live + converged + capped; paths = sum of the counts */
    double   trace_ms, fold_ms, test_ms;             /* GPU time of the last ct_adaptive_frame_update call, as CtCollectorInfo's */
} CtAdaptiveFrameInfo;       /* 96 bytes */

CT_API int ct_adaptive_frame_create(CtHandle h, const CtAdaptiveFrameDesc *d, CtAdaptiveFrame *out);
CT_API int ct_adaptive_frame_update(CtAdaptiveFrame f, uint32_t rounds);
CT_API int ct_adaptive_frame_raise_cap(CtAdaptiveFrame f, uint32_t max_samples);
CT_API int ct_adaptive_frame_info(CtAdaptiveFrame f, CtAdaptiveFrameInfo *out);
CT_API int ct_adaptive_frame_download(CtAdaptiveFrame f, uint32_t which, void *host, size_t bytes);
CT_API int ct_adaptive_frame_device_ptr(CtAdaptiveFrame f, uint32_t which, void **out);
CT_API int ct_adaptive_frame_destroy(CtAdaptiveFrame f);

/* The adaptive frame of one shard of a multi-GPU job.  ct_adaptive_frame_create_shard is ct_adaptive_frame_create for a handle
 * of any shard_count >= 1 -- the same checks in the same order, only the refusal of a shard is absent (ct_adaptive_frame_create
 * itself keeps it).  The live list at create is the handle's own pixels in ascending p: those with
 * ct_tile_owner(x / 8, y / 8, shard_count) == shard_index, listed on the device by a ballot count per 64 pixels, a scan and a
 * ranked write (no atomics: the same list on every run).  A pixel's samples depend on (x, y, subframe) alone and all live pixels
 * hold one count, so the shard's rounds need nothing from the other shards:
 *     on its own pixels mean, M2 and counts are, bit for bit and after the same number of completed rounds, those of the frame
 *     ct_adaptive_frame_create makes on an unsharded handle of the same scene, pose, light and description;
 *     a foreign pixel's 36 bytes are never written and stay all-zero bits for the frame's lifetime;
 *     over the shards of one job `live`, `converged`, `capped`, `paths` and the handles' CtCounters::paths sum to that frame's.
 * mean, M2 and counts stay whole-frame arrays (width * height float4, float4, uint32).  CtAdaptiveFrameInfo::pixels is the number
 * of own pixels (pixels = live + converged + capped as before); width and height are the frame's.  A shard that owns no pixel is
 * legal: create is CT_OK, nothing is live, update launches nothing.  Everything else -- update, raise_cap, info, download,
 * device_ptr, destroy, the CT_E_STATE rules, counters, invariants, chunks and passes -- is the object above.  With
 * shard_count == 1 the frame is ct_adaptive_frame_create's, allocations included.  Allocated at create for shard_count > 1:
 * mean, M2, counts, width * height / 64 (rounded up) + 1 wave counts, and two live lists of exactly the own-pixel count of words
 * each (none for a shard without pixels); CT_E_NOMEM leaves the handle as it was. */
CT_API int ct_adaptive_frame_create_shard(CtHandle h, const CtAdaptiveFrameDesc *d, CtAdaptiveFrame *out);

/* generatePoints (src/CUDA/pointGeneratorCamera.cu:20-42) + firstScatterPosition
 * (cloudFirstScatterMaterial.cu:8-29), launched over `count` threads by ScatterSampleCollector::collect
 * (ScatterSampleCollector.cpp:36-62): thread i draws a direction uniformly on the sphere and a point on
 * the reference's disc of radius sqrt(3)/2, shoots a ray from 2 units away and keeps the first scatter
 * position (world coordinates, box centred at 0) and the view direction; it retries until a ray
 * scatters inside the cloud (at most 4096 times, then the sample stays NaN like after `clear`).
 * Seeds: tea<4>(i, batch_seed) for the generator and tea<4>(i*4096, batch_seed + attempt) for the
 * flight (the reference mixes clock() into both).  Outputs are host arrays of 3*count floats. */
CT_API int ct_generate_scatter_samples(CtHandle h, uint32_t count, uint32_t batch_seed,
                                       float *positions_host_out, float *directions_host_out);

/* setupHierarchicalDescriptor<DisneyDescriptor, uint8_t> (src/CUDA/DisneyDescriptor.cuh:71-112) as launched
 * by DisneyDescriptorCollector::collect (src/Scene/DisneyDescriptorCollector.cpp:57-63; program `collect`,
 * src/CUDA/disneyDescriptorCollector.cu:21-28): for every (position, view direction) sample, 10 layers of
 * 9 x 5 x 5 trilinear + mip-linear samples of the density pyramid (Resources::generateMipmaps,
 * Resources.cpp:169-209) in the frame eZ = -light, eX = normalize(eZ x view), eY = eX x eZ; layer l spans
 * [-1,1]^2 x [-1,3] * 2^l free paths at LOD level0 + l, faded to zero outside the box, stored as uint8
 * (f * 255, truncating).  positions are the ScatterSample records' `point` (world coordinates, box centred
 * at 0); both inputs are host arrays of 3*count floats; descriptors_host_out receives
 * count * CT_DESCRIPTOR_BYTES bytes, layer-major, then z, y, x -- the `grid` field of
 * Persistance::DisneyDescriptor (DeepestScatter_Train/Protocols/DisneyDescriptor.proto:7-10).
 * A view exactly parallel or antiparallel to the light has no frame: eX = normalize(0) is NaN and with it every grid point.
 * The reference converts that NaN to a byte, which C leaves undefined; here a grid point whose position is not finite (this
 * case, or a sample whose position or view is not finite) stores 0 -- what a saturating conversion gives -- so such a sample's
 * descriptor is 2250 zero bytes.  The test is made on the floats, before any conversion to an integer. */
#define CT_DESCRIPTOR_LAYERS 10
#define CT_DESCRIPTOR_LAYER_SIZE 225
#define CT_DESCRIPTOR_BYTES (CT_DESCRIPTOR_LAYERS * CT_DESCRIPTOR_LAYER_SIZE)
CT_API int ct_collect_descriptors(CtHandle h, const float *positions_host, const float *directions_host,
                                  uint32_t count, uint8_t *descriptors_host_out);

/* The device side of the reference's neural renderer (src/CUDA/disneyCamera.cu + sampleDisneyDescriptor over rects of the
 * frame): for every pixel of a rect, the first scatter position of the primary ray and the hierarchical descriptor at that
 * point, as a device-resident batch a model can consume -- the two entry points above without the host in between.
 * rect = {x0, y0, x1, y1}, half-open, inside the frame; NULL = the whole frame.  Pixel (x, y) follows the first lines of
 * pinholeCamera / singleScatterSunRadiance (pathTracingCamera.cu:12-21, cloudRadianceMaterials.cu:11-21,120-134) exactly:
 * d1 = normalize(U*dx + V*dy + W), dx = x / width * 2 - 1; a ray that misses the box gives no record; the flight starts at
 * eye + d1 * t_hit + bbox / 2 in the direction d2 = normalize(d1) with xi = the first number of the seed
 * tea<4>(x*4096+y, subframe_id) and is ONE march flight (getNextScatteringEvent, cloud.cuh:77-114) -- the first event
 * CT_MODE_SUN_SINGLE_SCATTER draws for that pixel and subframe, whatever the handle's mode; the handle's estimator does not
 * matter either (a DELTA handle makes the same march flight, as in ct_generate_scatter_samples).  A pixel whose flight
 * scattered at a position inside the box (isInBox) is VALID and yields one record: position = the scatter position in world
 * coordinates (box centred at 0, as ct_generate_scatter_samples), direction = d2, pixel = y * width + x, descriptor = exactly
 * the bytes ct_collect_descriptors returns for that (position, direction).  CT_FLAG_TEX_FIXED8 applies to the flight and the
 * gather as it does there.
 * Records are compacted in ascending row-major order INSIDE THE RECT (wave counts, a scan, a ranked write: no atomics), so the
 * same call always gives the same bytes.  *count_out = valid pixels of the rect.  The three record arrays hold `capacity`
 * records each (descriptors_dev capacity * CT_DESCRIPTOR_BYTES bytes, positions_dev / directions_dev 3 * capacity floats,
 * pixels_dev capacity words; those three may be NULL); *count_out > capacity: CT_E_INVAL with *count_out set, the arrays'
 * contents unspecified (nothing is written past them), the handle usable.  No valid pixel: CT_OK, count 0.
 * CT_E_INVAL: a NULL handle, descriptors_dev or count_out; a rect that is empty, exceeds the frame or has more than 2^20
 * pixels.  The scene's shard_index / shard_count are IGNORED: the rect is the caller's way to split a frame over GPUs.
 * Waits for the batches in flight, runs on the handle's stream and returns when it is idle.  Does not touch mean, M2, the
 * frame, the subframe count, CtCounters or CtFetchCounters, drops no samples rendered ahead and leaves the pose's pixel
 * list alone.  Temporaries are allocated before any kernel runs: CT_E_NOMEM leaves the handle usable.  The mip pyramid is
 * built on first use, as in ct_collect_descriptors. */
CT_API int ct_descriptor_frame(CtHandle h, uint32_t subframe_id, const uint32_t rect[4],
                               uint32_t capacity,          /* records the three arrays can hold */
                               uint8_t  *descriptors_dev,  /* capacity * CT_DESCRIPTOR_BYTES    */
                               float    *positions_dev,    /* capacity * 3, may be NULL         */
                               float    *directions_dev,   /* capacity * 3, may be NULL         */
                               uint32_t *pixels_dev,       /* capacity, y * width + x, may be NULL */
                               uint32_t *count_out);

/* Diagnostic: milliseconds the GPU spent in the last ct_descriptor_frame of this handle, measured with HIP events on its
 * stream: the first flights with their compaction, and the descriptor gather (0 when the call did not get that far).
 * Either pointer may be NULL. */
CT_API int ct_debug_descriptor_frame_time(CtHandle h, double *first_scatter_ms_out, double *gather_ms_out);

/* ---- the scattering network ------------------------------------------------------------
 *
 * ct_network_eval runs a network on the records that ct_descriptor_frame (or ct_collect_descriptors, uploaded) leaves on the
 * device: one fused bf16 MFMA kernel that reads each record's 2250 bytes once and writes one float per record.
 *
 * THE NETWORK IS THIS PROJECT'S DEFINITION.  The reference's DisneyModel.py was not available when this was written; what
 * follows is the progressive-feed residual MLP of the paper the reference implements (Kallweit et al. 2017, "Deep Scattering"),
 * parameterised by its shapes.  A model trained elsewhere is exported into it by name (deepestscatter_amd/network.py, ScatterNet):
 *     blocks.k.fc1.weight / .bias = W1_k, c1_k     blocks.k.fc2.weight / .bias = W2_k, c2_k      (k = 0 .. 9)
 *     head.i.weight / .bias       = V_i, d_i       (i = 0 .. H - 2)                out.weight / .bias = v, d
 *
 * Parameters: K = CT_DESCRIPTOR_LAYERS (10) blocks; width Wd, a multiple of 8 with 16 <= Wd <= 256 (the reference-sized case is
 * 200); A aux inputs per record, 0 <= A <= 8; H head layers, 1 <= H <= 4.
 * Per record: b_k = the 225 bytes of descriptor layer k in the order ct_collect_descriptors stores them (z, y, x); a = the
 * record's A aux floats.
 * Forward pass (there is no state z_0):
 *     block 0:      h = relu(W1_0 [b_0/255 | a] + c1_0)            z_1     = relu(W2_0 h + c2_0)
 *     block k >= 1: h = relu(W1_k [z_k | b_k/255 | a] + c1_k)      z_{k+1} = relu(z_k + W2_k h + c2_k)
 *     head:         H - 1 layers z <- relu(V_i z + d_i) of width Wd, then out = v z + d, one float, no output transform.
 * Matrices are [out][in] row-major (the torch.nn.Linear layout), biases float32.
 * Rounding (the "rounded model" the device implements; reference_forward of deepestscatter_amd/network.py restates it):
 *   - every matrix entry is rounded to bf16, round-to-nearest-even, once, at create; the byte columns of W1_k are stored as
 *     bf16(float32(w) / 255.0f) and the bytes enter as the integers 0 .. 255, which bf16 holds exactly;
 *   - a, every h and every z_k are bf16 values, each rounded when it is produced; the residual adds the rounded z_k;
 *   - inside a layer the products are summed in float32, and the float32 bias and the ReLU are applied there; out is float32.
 *   The kernel pads to its tile sizes with zeros, which is exact and no part of the definition.  The order of a layer's float32
 *   sum is the matrix unit's, so results agree with a CPU evaluation of the rounded model to float32 summation error, which
 *   can flip a bf16 rounding that later layers carry on (tests/test_network.py states the bound).
 *
 * weights_host is one flat float32 array: block after block W1_k, c1_k, W2_k, c2_k (W1_0 has 225 + A columns, every other W1_k
 * Wd + 225 + A in the order [z | b | a]), then the head V_0, d_0, ..., then v (Wd floats) and d (1) -- each matrix before its
 * bias.  weight_count must be the number the shapes imply:
 *     Wd (225 + A) + 9 Wd (Wd + 225 + A) + 10 (Wd Wd + 2 Wd) + (H - 1)(Wd Wd + Wd) + Wd + 1.
 * The array is packed (padded, permuted to the kernel's fragments, rounded) at create and not retained. */
typedef struct CtNetworkDesc {
    uint32_t abi_version;      /* must be CT_ABI_VERSION */
    uint32_t blocks;           /* must be CT_DESCRIPTOR_LAYERS */
    uint32_t width;            /* Wd */
    uint32_t aux;              /* A */
    uint32_t head_layers;      /* H */
    const float *weights_host;
    size_t weight_count;
} CtNetworkDesc;
typedef struct CtNetwork_ *CtNetwork;

/* A network on h's device, owned by the caller: destroy it before h.  CT_E_INVAL, before anything is allocated: a NULL
 * argument, a wrong abi_version, blocks, width, aux or head_layers, a wrong weight_count, a weight that is not finite.
 * ct_last_error(h) has the message. */
CT_API int ct_network_create(CtHandle h, const CtNetworkDesc *d, CtNetwork *out);
CT_API int ct_network_destroy(CtNetwork n);   /* NULL is a no-op */

/* out_dev[i] = the network's output for record i, i < count.  descriptors_dev holds count * CT_DESCRIPTOR_BYTES bytes, aux_dev
 * count * A floats, record after record (NULL if and only if A == 0); the arrays are 4-byte aligned.  Waits for the batches
 * in flight like every synchronous entry point, runs on the handle's stream and returns when it is idle.  Allocates nothing
 * (the packed weights belong to the CtNetwork) and uses no atomics: the same call gives the same bits.  Reads nothing past
 * the count records, writes nothing but out_dev[0 .. count), and touches nothing of the progressive render -- mean, M2,
 * frame, subframe count, counters, samples rendered ahead -- exactly as ct_descriptor_frame.  count == 0: CT_OK, nothing
 * written.  CT_E_INVAL: a NULL handle, network, descriptors_dev or out_dev, aux_dev not matching A, an unaligned array,
 * count > 2^20, a network that lives on another device than h. */
CT_API int ct_network_eval(CtHandle h, CtNetwork n, const uint8_t *descriptors_dev, const float *aux_dev, uint32_t count,
                           float *out_dev);

/* Diagnostic: milliseconds the GPU spent in the kernel of the last ct_network_eval of this network (HIP events on its stream). */
CT_API int ct_debug_network_time(CtNetwork n, double *ms_out);

/* Diagnostic: x rounded to bf16 (round to nearest, ties to even; a NaN stays a NaN) and widened again -- the one rounding
 * routine ct_network_create packs with. */
CT_API float ct_debug_bf16_round(float x);

/* ---- the scattering network as a renderer ---------------------------------------------------
 *
 * The reference's neural renderers are ARenderers: render(frameResultBuffer) fills the frame and Camera::render runs the same
 * Welford accumulation, tonemap and convergence test as for the path tracer (Camera.cpp:189-214).  These two entry points are
 * that for a CtNetwork with ONE aux input: ct_descriptor_frame, the aux input, ct_network_eval and the frame, for whole frames
 * of any size ct_create accepts, without leaving the device.
 *
 * Definition, per pixel (x, y) of the whole frame and subframe s:
 *   - the record is ct_descriptor_frame's for that pixel and subframe: the same flight, position, direction d2 and descriptor
 *     bytes; CT_FLAG_TEX_FIXED8 applies as it does there, the handle's estimator and mode do not matter;
 *   - aux = d2.x * l.x + d2.y * l.y + d2.z * l.z with l = the handle's twice-normalised light travel direction (ct_set_light),
 *     evaluated left to right in float32 without contraction;
 *   - out = ct_network_eval's value for that record;
 *   - L = out (CT_NET_OUT_LINEAR) or ct_expf(out) - 1.0f (CT_NET_OUT_EXPM1, include/ct_fmath.h); g = L > 0 ? L : 0, so a NaN
 *     becomes 0;
 *   - the pixel is (rgb_scale[0] * g, rgb_scale[1] * g, rgb_scale[2] * g, 1);
 *   - a pixel without a record is (0, 0, 0, 1), the miss value of ct_render_subframe.
 *
 * The sun's single-scatter term (CT_NET_ADD_SINGLE_SCATTER).  A network trained on ct_point_radiance_launch's
 * CT_MODE_SUN_MULTIPLE_SCATTER labels predicts the multiply scattered light only; per pixel and subframe
 *     CT_MODE_TOTAL  =  CT_MODE_SUN_SINGLE_SCATTER  +  (multiple scatter from the first-scatter point),
 * the first summand being the un-chopped-Mie NEE at the first collision, with the same seed and the same first flight.  With
 * the flag in `transform` a pixel that has a record is
 *     (rgb_scale[0] * g + D.x, rgb_scale[1] * g + D.y, rgb_scale[2] * g + D.z, 1),
 * each product rounded to float32 before its sum (no contraction).  D is what singleScatterSunRadiance returns for that pixel
 * and subframe, i.e. what ct_render_subframe of a CT_MODE_SUN_SINGLE_SCATTER handle writes there: getInScattering at the
 * flight's end position and d2 with the un-chopped Mie table, the handle's shadow volume (it follows ct_set_light), light
 * colour x intensity and sun_ratio.  rgb_scale does not apply to D, which is in the estimator's own units.  D is evaluated in
 * the first-flight pass, at the flight's own texture-space end position (the record's world position plus the half box does
 * not round back to it).  Like the flight, D ignores the handle's mode and estimator; CT_FLAG_TEX_FIXED8 applies to it as to
 * every other NEE.  A pixel without a record stays (0, 0, 0, 1).  A call without the flag is bit for bit what it was.
 *
 * Bands.  The frame is cut into bands of whole rows of at most band_pixels pixels (at least one row, at most 2^20 pixels; 0 =
 * 2^20), taken bottom to top; each band is one pass through the first flights and their compaction, the 4-byte read of the
 * record count, the descriptor gather, the aux kernel, the network and one kernel that forms the pixels.  That kernel ranks a
 * pixel among its wave's valid lanes from the flight's per-pixel temporary and the scanned wave counts and reads its record's
 * output there: no scatter, no atomics, the same call gives the same bits.  Records are per pixel and a record's output does
 * not depend on its place in a batch, so the image does not depend on band_pixels.  A band without a record skips the gather,
 * the aux kernel and the network.
 *
 * Scratch.  The temporaries belong to the handle: allocated on first use, grown when a call needs more, never freed between
 * calls, freed by ct_destroy; a warm call allocates nothing.  The per-pixel temporary, positions, directions, aux and out --
 * and, from the first call that carries CT_NET_ADD_SINGLE_SCATTER on, the single-scatter temporary, 16 more bytes per band
 * pixel -- are sized for the band and allocated, with a first piece of the descriptor array, before the call's first kernel:
 * CT_E_NOMEM can only be answered there, and then frame, mean, M2 and the subframe count are exactly as they were and the
 * handle is usable.
 * The descriptor array (2250 bytes per record: 2^20 records would be 2.4 GB, which is why the count is read first and why
 * band_pixels exists) is sized for the largest record count seen so far and grown between bands, with the stream idle; if
 * the device refuses that growth the band's records go through the gather and the network in pieces of the size it has -- the
 * same bits, since records are independent -- and the call succeeds.
 *
 * CT_E_INVAL: a NULL handle (answered without a device), network or params; a wrong abi_version; an unknown transform (a low
 * byte that is no CT_NET_OUT_* value, or any bit set above it other than CT_NET_ADD_SINGLE_SCATTER); an rgb_scale that is not
 * finite; a network with aux != 1; a network on another device than h; a handle created with
 * shard_count > 1 (a shard renders its tiles with ct_network_render_shard_* below, a CtGroup with
 * ct_group_network_render_accumulate); subframe_id == 0; count == 0.  CT_E_STATE: no camera pose (ct_create sets the default
 * one, so a live handle always has one); ct_network_render_accumulate with first_subframe_id != subframes + 1, as
 * ct_render_accumulate.  Arguments are checked before anything of the handle changes.
 * Both wait for the batches in flight, run on the handle's stream and return when it is idle. */
enum { CT_NET_OUT_LINEAR = 0, CT_NET_OUT_EXPM1 = 1 };
#define CT_NET_ADD_SINGLE_SCATTER 0x100   /* bit 8 of CtNetworkRender::transform: add the sun's single-scatter term D */
typedef struct CtNetworkRender {
    uint32_t abi_version;   /* must be CT_ABI_VERSION */
    int32_t  transform;     /* low byte: CT_NET_OUT_LINEAR: L = out; CT_NET_OUT_EXPM1: L = ct_expf(out) - 1.0f.  Bit 8:
                               CT_NET_ADD_SINGLE_SCATTER.  Any other bit set: CT_E_INVAL */
    float    rgb_scale[3];  /* finite */
    uint32_t band_pixels;   /* largest number of pixels handled at once; 0 = 2^20.  Bands are whole rows, at least one row,
                               at most 2^20 pixels */
} CtNetworkRender;

/* ARenderer::render(frameResultBuffer) of the network: the frame defined above into the handle's CT_BUF_FRAME and, when
 * frame_rgba_dev != NULL, into that device buffer too (W*H*4 floats, caller-owned), exactly as ct_render_subframe.  Touches
 * nothing else: not the mean, M2, the subframe count, CtCounters, CtFetchCounters, the samples rendered ahead or the pose's
 * pixel list. */
CT_API int ct_network_render_subframe(CtHandle h, CtNetwork n, const CtNetworkRender *p, uint32_t subframe_id, float *frame_rgba_dev);

/* for id = first .. first + count - 1 { ct_network_render_subframe(id); ct_accumulate(id, NULL) } fused: mean, M2, the subframe
 * count, the frozen state and ct_converged_at are left bit for bit as that loop leaves them (ct_set_stop_when_converged is
 * honoured the way ct_accumulate honours it: the test follows every cadence-th subframe from min_subframes on), but the
 * float4 frame is not materialised -- the kernel that forms a band's pixels applies the Welford update to mean and M2
 * directly -- and CT_BUF_FRAME is left alone.  Like ct_accumulate it drops the samples rendered ahead. */
CT_API int ct_network_render_accumulate(CtHandle h, CtNetwork n, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count);

/* The same renderer on a handle of any shard_count >= 1: the frame of THIS SHARD, as ct_render_subframe leaves a shard's frame.
 *
 * Definition.  A pixel of a tile the shard owns (ct_tile_owner) is exactly the pixel defined above -- same flight, seed, record,
 * aux, output, transform, single-scatter term -- so on a shard_count == 1 handle the two entry points give the bits of
 * ct_network_render_subframe / ct_network_render_accumulate.  A foreign pixel of the frame is (0, 0, 0, 0); foreign pixels of
 * mean and M2 are never touched and stay exactly 0, so a SUM over the shards is the unsharded image bit for bit and
 * ct_group_merge, ct_group_tonemap and ct_group_is_converged apply unchanged.
 *
 * Bands.  The shard's tiles are taken in ascending ty * tiles_x + tx (ct_shard_tiles; the list is built on the device on first
 * use and freed by ct_destroy).  A band is a run of at most max(1, band_pixels / 64) consecutive tiles of that list, at most
 * 2^14 (band_pixels == 0 or > 2^20: 2^14), one wave per tile: lane l of a tile is its pixel (l & 7, l >> 3), and a lane
 * the frame clips has no pixel.  A wave's 64 flights are therefore one tile's, and a shard spends nothing on foreign pixels.
 * The passes of a band, the ranking by ballot (one count per tile), "no scatter, no atomics" and "the image does not depend on
 * band_pixels" are as above; records reach gather and network in tile order.  ct_network_render_shard_subframe first fills the
 * frame with the shard's background -- (0, 0, 0, 1) on own pixels, (0, 0, 0, 0) on foreign ones -- and the bands then write
 * the own pixels.
 *
 * Scratch is the same scratch, shared with the two entry points above and sized in lanes (64 per tile of a band); the
 * tile list is allocated with it, before the call's first kernel.  Errors, their order, "arguments checked before anything
 * changes", the samples rendered ahead, ct_set_stop_when_converged (which refuses shards itself) and the stages of
 * ct_debug_network_render_time (the background fill counts to [3]) are those of the two entry points above, except that
 * shard_count > 1 is accepted.  Both are synchronous: every band waits for its record count, so the shards of a job only work
 * at the same time when each is driven by its own host thread (ct_group_network_render_accumulate does that). */
CT_API int ct_network_render_shard_subframe(CtHandle h, CtNetwork n, const CtNetworkRender *p, uint32_t subframe_id, float *frame_rgba_dev);
CT_API int ct_network_render_shard_accumulate(CtHandle h, CtNetwork n, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count);

/* Diagnostic: the scratch of the network renderer as the handle holds it now: out[0 .. 8] = the device addresses of the
 * per-lane temporary, the wave counts, positions, directions, aux, out, the descriptor array, the single-scatter temporary and
 * the shard's tile list (0 = not allocated), out[9 .. 11] = the capacities in lanes of the band arrays, in records of the
 * descriptor array, in lanes of the single-scatter temporary.  A warm call leaves all twelve as they were. */
CT_API int ct_debug_network_scratch(CtHandle h, uint64_t out[12]);

/* Diagnostic: the aux kernel of the two entry points above on caller-supplied directions: aux_dev_out[i] = d.x * l.x + d.y * l.y +
 * d.z * l.z for d = directions_dev[3 i .. 3 i + 2] and the handle's light.  count == 0: CT_OK, nothing read or written.
 * CT_E_INVAL: a NULL handle, or a NULL array with count > 0. */
CT_API int ct_debug_network_aux(CtHandle h, const float *directions_dev, uint32_t count, float *aux_dev_out);

/* Diagnostic: milliseconds the GPU spent in the last ct_network_render_subframe / ct_network_render_accumulate of this handle
 * (HIP events on its stream), summed over its bands and subframes: ms_out[0] first flights with their compaction (and the NEE of
 * CT_NET_ADD_SINGLE_SCATTER, which runs in the flight's kernel), [1] the
 * descriptor gather, [2] the network, [3] the aux kernel and the kernel that forms the pixels (and accumulates them). */
CT_API int ct_debug_network_render_time(CtHandle h, double ms_out[4]);

/* ---- the network baked into a probe table ---------------------------------------------------
 *
 * The reference's default renderer is its second neural one: BakedRenderer keeps light probes on a grid and interpolates them
 * (bakedCamera.cu, lightProbeMaterial.cu, LightProbe.cuh; not available, like DisneyModel.py, so THE DEFINITION BELOW IS THIS
 * PROJECT'S).  It rests on a symmetry of the renderer above: for a fixed cloud, light and network a record's output is a
 * function of five numbers -- the position, the azimuth of the view around the light axis (all the descriptor sees of the view:
 * eX = normalize(eZ x view)) and aux = d2 . l (which the descriptor does not depend on).  ct_network_bake evaluates the network
 * once on a regular grid over those five; a subframe is then the first flight and a 32-tap interpolation: no gather, no network,
 * no record count, no compaction, no host wait between bands or subframes.  A new light is a re-bake (ct_bake_update), as
 * ct_set_light is a rebuild of the shadow volume.  What the table costs in accuracy is its resolution: the caller's trade.
 *
 * The grid.  b = the box size (dims / max dim, the box centred at 0 like every position of this ABI).  Nx, Ny, Nz = grid, each
 * 2 .. 256; Nphi = azimuths, a multiple of 4 in 4 .. 64; Nc = cosines, 2 .. 64; entries = Nx Ny Nz Nphi Nc <= 2^26.
 *   - position node i of an axis: -b/2 + b * i / (N - 1);
 *   - azimuth: the library picks an orthonormal pair a, b perpendicular to l when it bakes (CtBakeInfo).  For a direction d:
 *     px = d.a, py = d.b (each left to right in float32), s = |px| + |py|; t = 0 when s is 0 or not finite, otherwise p = px / s
 *     and t = py >= 0 ? 1 - p : 3 + p, a number in [0, 4] made without a trigonometric function.  Azimuth node j sits at
 *     t_j = j / (Nphi / 4); its probe direction is u_j = normalize(p a + q b) with p = 1 - t_j, q = 1 - |p| for t_j <= 2 and
 *     p = t_j - 3, q = -(1 - |p|) beyond: a unit vector perpendicular to the light;
 *   - polar node k: cosine[k] = -1 + 2 k / (Nc - 1);
 *   - probe (z, y, x, j) has index ((z Ny + y) Nx + x) Nphi + j and the record (position node, u_j); ct_bake_probes returns
 *     exactly the floats the bake used;
 *   - table[index * Nc + k] = ct_network_eval's value for the descriptor ct_collect_descriptors gives that record, with
 *     aux = cosine[k]: raw outputs, the transform is applied at lookup.  CT_FLAG_TEX_FIXED8 applies to the gather as everywhere.
 *
 * The lookup for (world position w, direction d2), which ct_debug_bake_lookup exposes.  Per spatial axis
 * fx = (w.x + 0.5f * bx) * ((float)(Nx - 1) / bx) clamped to [0, Nx - 1], x0 = min((int)fx, Nx - 2), wx = fx - x0; polar
 * c = d2 . l left to right, fc = (c + 1.0f) * (0.5f * (Nc - 1)) clamped and split into k0, wc the same way; azimuth
 * ft = t(d2) * (Nphi * 0.25f), j0 = (int)floor(ft), wphi = ft - j0, j0 %= Nphi, j1 = (j0 + 1) % Nphi.  Every lerp is
 * u + (v - u) * w with the product rounded before the sum, over k, then j, then x, y, z.
 *
 * The pixel is exactly ct_network_render_*'s pixel with `out` replaced by the lookup at the record's world position and d2:
 * flight, seed, validity, transform, g, rgb_scale, the CT_NET_ADD_SINGLE_SCATTER term, the miss value and a shard's foreign
 * pixels are the same; "fused = the loop subframe + ct_accumulate, bit for bit" holds; the frozen test and
 * ct_set_stop_when_converged behave as there.  band_pixels sizes only the flight's temporaries (the handle's scratch of the
 * renderer above, which the bake's chunks use too) and the image does not depend on it.  A render call enqueues all its bands and
 * subframes and waits once (the convergence test keeps its own wait); a warm call allocates nothing.
 *
 * The bake sends the probes through gather and network in chunks of at most min(CT_NET_DESC_RECORDS, 2^20) records, one gather
 * per chunk serving all Nc evaluations; the result does not depend on the chunk size.  The table is allocated before the first
 * kernel: CT_E_NOMEM leaves the handle -- and in ct_bake_update the old table -- as they were.
 *
 * Errors, checked before anything changes, in the order of the renderer above.  CT_E_INVAL: a NULL argument (a NULL handle is
 * answered without a device); a wrong abi_version; a size outside the ranges above, or too many entries; a network with
 * aux != 1 or on another device; a bake made on another handle; a sharded handle on the unsharded entry points;
 * subframe_id == 0 or count == 0; an unknown transform or a non-finite scale; ct_bake_probes / ct_bake_download out of range.
 * CT_E_STATE: rendering, or ct_debug_bake_lookup, with a bake whose light is no longer the handle's (ct_bake_update bakes it
 * again); first_subframe_id != subframes + 1. */
typedef struct CtBakeDesc {
    uint32_t abi_version;   /* must be CT_ABI_VERSION */
    uint32_t grid[3];       /* Nx, Ny, Nz */
    uint32_t azimuths;      /* Nphi */
    uint32_t cosines;       /* Nc */
} CtBakeDesc;
typedef struct CtBake_ *CtBake;
typedef struct CtBakeInfo {
    uint32_t grid[3], azimuths, cosines;
    uint64_t entries;
    float light[3];                /* l: the twice-normalised travel direction the table was baked for */
    float axis_a[3], axis_b[3];    /* orthonormal, perpendicular to l; chosen by the library */
    float cosine[64];              /* the aux value of polar node k, k < cosines */
    uint32_t current;              /* 1 while the handle's light is the one the table was baked for */
    double gather_ms, network_ms;  /* GPU time of the last bake / update */
} CtBakeInfo;

CT_API int ct_network_bake(CtHandle h, CtNetwork n, const CtBakeDesc *d, CtBake *out);
CT_API int ct_bake_update(CtHandle h, CtNetwork n, CtBake b);   /* bake again, in place: after ct_set_light, or for another network */
CT_API int ct_bake_destroy(CtBake b);                           /* NULL is a no-op; destroy before h */
CT_API int ct_bake_info(CtBake b, CtBakeInfo *out);
/* Probes first .. first + count - 1 (index order) as the bake made them: 3 floats each.  first + count <= entries / cosines. */
CT_API int ct_bake_probes(CtBake b, uint64_t first, uint32_t count, float *positions_host_out, float *directions_host_out);
CT_API int ct_bake_download(CtBake b, float *table_host_out, size_t count);   /* count must equal entries */
/* Diagnostic: the lookup on caller-supplied records (3 floats each, device memory) -> count floats.  count == 0: CT_OK. */
CT_API int ct_debug_bake_lookup(CtHandle h, CtBake b, const float *positions_dev, const float *directions_dev, uint32_t count,
                                float *out_dev);

/* ---- the sparse bake: only the probes a flight can reach ---------------------------------------
 *
 * A lookup only ever happens at a first-scatter position, and a first-scatter position is next to non-zero density: the flight
 * ends at most one march step (S = sample_step * max dim texels) behind a sample whose eight-texel footprint holds a non-zero
 * texel.  ct_network_bake_sparse bakes the probes of the position nodes such a position can touch and leaves every other entry
 * of the table 0.0f.  The table stays dense in memory: the lookup, the render entry points and every function above take the
 * CtBake as they take ct_network_bake's, and every frame is the dense bake's frame bit for bit.
 *
 * The mask, in integers.  dims = (Dx, Dy, Dz), M = ceil((double)sample_step * max dim) + 3.  Per axis with N nodes and D texels,
 * cell c (between nodes c and c + 1) has the texel range, computed in double,
 *     t_lo(c) = max(0, floor(c * D / (N - 1)) - M),   t_hi(c) = min(D - 1, ceil((c + 1) * D / (N - 1)) + M);
 * cell (cx, cy, cz) is occupied when any texel of the level-0 density in the box of its three ranges is non-zero; node (x, y, z)
 * is active when one of the up to eight cells it is a corner of is occupied.  The sparse table is the dense table, bit for bit,
 * on every entry (all Nphi azimuths, all Nc polar nodes) of an active node and 0.0f elsewhere.  The probes baked are the active
 * nodes in ascending node index, each with j = 0 .. Nphi - 1, in chunks as above; the result does not depend on the chunk size.
 * ct_bake_probes keeps answering every probe of the grid, baked or not.
 *
 * THE ONE OBSERVABLE DIFFERENCE from a dense bake: ct_debug_bake_lookup at a position that no flight can produce (far from
 * every non-zero texel) interpolates the zeros of inactive nodes.
 *
 * ct_network_bake_sparse has ct_network_bake's validation, error order and limits (the storage is dense: 2^26 entries).  The
 * table, the mask's temporaries, the node bytes and the list are allocated before the first kernel: CT_E_NOMEM leaves the handle
 * as it was.  A grid without an active node is CT_OK: an all-zero table, no gather and no network call.  ct_bake_update of a
 * sparse bake stays sparse and reuses the list (the density of a live handle never changes); it bakes into a zeroed second table
 * and swaps, as for a dense bake.  CtBakeInfo's gather_ms and network_ms are those of the probes actually baked. */
typedef struct CtBakeSparseInfo {
    uint32_t sparse;          /* 1: made by ct_network_bake_sparse */
    uint32_t margin_texels;   /* M (0 for a dense bake) */
    uint64_t nodes;           /* Nx Ny Nz */
    uint64_t active_nodes;    /* = nodes for a dense bake */
    uint64_t probes_baked;    /* active_nodes * Nphi */
    double   mask_ms;         /* GPU time of the mask, list and record kernels of the last bake / update (an update: the record kernel) */
} CtBakeSparseInfo;

CT_API int ct_network_bake_sparse(CtHandle h, CtNetwork n, const CtBakeDesc *d, CtBake *out);
CT_API int ct_bake_sparse_info(CtBake b, CtBakeSparseInfo *out);
/* One byte per node, index (z Ny + y) Nx + x; a dense bake answers all 1.  count must equal Nx Ny Nz. */
CT_API int ct_bake_mask(CtBake b, uint8_t *nodes_host_out, size_t count);
/* Diagnostic, no network needed: the mask of a grid (2 .. 256 nodes per axis) on this handle.
 * cells_host_out: (Nx-1)(Ny-1)(Nz-1) bytes, x fastest.  nodes_host_out: Nx Ny Nz bytes.
 * active_host_out: up to `capacity` ascending node indices.  Any of the three may be NULL.
 * *count_out = active nodes (set even when capacity is too small, which is CT_E_INVAL). */
CT_API int ct_debug_bake_mask(CtHandle h, const uint32_t grid[3], uint8_t *cells_host_out, uint8_t *nodes_host_out,
                              uint32_t *active_host_out, uint32_t capacity, uint32_t *count_out);

/* ---- the compact bake: only the active nodes are stored -----------------------------------------
 *
 * ct_network_bake_compact is the sparse bake with a table that holds nothing for an inactive node.  Mask, margin M, occupied
 * cells, active nodes and their ascending list are the sparse bake's, byte for byte.
 *   - slots: slot[node] = 0 for an inactive node; the r-th active node in ascending node index (r from 0) has slot[node] = 1 + r.
 *     One uint32 per node, Nx Ny Nz of them, in node index order (z Ny + y) Nx + x (ct_bake_slots).
 *   - the stored table holds (active + 1) Nphi Nc floats (ct_bake_download_stored): slot 0 is Nphi Nc times 0.0f, slot s >= 1 the
 *     [Nphi][Nc] block of node list[s - 1], bit for bit the dense bake's values for that node.
 *   - the lookup is exactly the lookup defined above -- same cell split, same weights, same lerp order k, j, x, y, z -- with the tap
 *     of (node, j, k) read at ((size_t)slot[node] Nphi + j) Nc + k.  An inactive corner reads the zero slot; there is no branch on
 *     activity.  It is therefore the SPARSE bake's lookup bit for bit for every input, positions no flight can produce included,
 *     and "the one observable difference from a dense bake" stays the sparse bake's.
 * Every ct_baked_render_* entry point, the shard ones included, and ct_debug_bake_lookup take a compact CtBake as they take any
 * other; every frame, mean and M2 is the dense bake's bit for bit wherever a dense bake of that grid exists.
 *
 * Limits.  Grid, azimuth and cosine ranges are unchanged.  The 2^26 bound applies to the STORED entries (active + 1) Nphi Nc, not
 * to the virtual Nx Ny Nz Nphi Nc: CtBakeInfo::entries stays the virtual count (at most 2^36).  Dense and sparse bakes keep their
 * limit.
 *
 * The existing entry points on a compact bake: ct_bake_download takes count == entries (the virtual count) and writes the table
 * expanded on the host -- zeros off the mask, the stored blocks on it: the sparse bake's table bit for bit; ct_bake_sparse_info
 * and ct_bake_mask answer as for a sparse bake (sparse = 1); ct_bake_probes answers every probe of the grid; ct_bake_update
 * stays compact, reuses the list and the slots, bakes into a second STORED table and swaps (a failure leaves everything as it was).
 *
 * Errors and allocation: ct_network_bake's validation and order, without the bound on the virtual entries.  The mask's
 * temporaries, the node bytes, the list, the slots and the probe tables are allocated before the first kernel.  THE ONE PLACE
 * WHERE THE ORDER DIFFERS FROM THE SPARSE BAKE: the stored table can only be sized once the 4-byte count of active nodes is back,
 * so it is allocated behind the mask kernels.  More than 2^26 stored entries is CT_E_INVAL (the message names both numbers), a
 * refused allocation CT_E_NOMEM; both come before any gather or network kernel, with *out = NULL and the handle exactly as it
 * was.  No active node is CT_OK: one zero slot, no gather and no network call. */
typedef struct CtBakeStorageInfo {
    uint32_t compact;        /* 1: made by ct_network_bake_compact */
    uint32_t reserved;       /* 0 */
    uint64_t slots;          /* active + 1; dense / sparse bake: Nx Ny Nz */
    uint64_t stored_entries; /* floats the table holds on the device */
    uint64_t table_bytes;    /* 4 * stored_entries (a half bake, "half tables" below: 2 * stored_entries) */
    uint64_t index_bytes;    /* 4 * Nx Ny Nz; 0 for a dense / sparse bake */
} CtBakeStorageInfo;

CT_API int ct_network_bake_compact(CtHandle h, CtNetwork n, const CtBakeDesc *d, CtBake *out);
CT_API int ct_bake_storage_info(CtBake b, CtBakeStorageInfo *out);                    /* every kind of bake */
/* One uint32 per node, index (z Ny + y) Nx + x.  count must equal Nx Ny Nz; a bake that is not compact: CT_E_INVAL. */
CT_API int ct_bake_slots(CtBake b, uint32_t *slots_host_out, size_t count);
/* The table as stored: [slot][Nphi][Nc].  count must equal stored_entries; a bake that is not compact: CT_E_INVAL. */
CT_API int ct_bake_download_stored(CtBake b, float *table_host_out, size_t count);

/* ---- the traced bake: the probe table filled with path-traced radiance -----------------------------
 *
 * A table entry at (position node, azimuth node j, polar node k) stands for the multiply scattered sun radiance that arrives at
 * the node from direction d(j, k): the label a network of this ABI is trained on, and what ct_point_radiance_launch estimates on a
 * CT_MODE_SUN_MULTIPLE_SCATTER handle.  ct_bake_traced makes a CtBake whose entries are Monte-Carlo means of that estimator,
 * traced on the device over the bake's own nodes, with no network: pictures from ct_baked_render_* at the baked subframe's cost
 * (with CT_NET_ADD_SINGLE_SCATTER the path tracer's total, up to the table's resolution), and the table a network bake of the
 * same grid should approach.
 *
 * Grid, limits, frame (l, a, b), cosine[k], position nodes, u_j, mask, active list and slots are those of ct_network_bake (kind
 * CT_BAKE_DENSE), ct_network_bake_sparse (CT_BAKE_SPARSE) or ct_network_bake_compact (CT_BAKE_COMPACT), with their validation,
 * their order of errors and their 2^26 bound (a compact bake: on the stored entries).
 *   - d(j, k) = c l + sqrt(1 - c^2) u_j with c = cosine[k], computed in double from the floats l and u_j (ct_bake_probes') and
 *     rounded once to float; at c = -1 and c = 1 it is -l and l for every j.  ct_bake_directions returns exactly the floats
 *     the tracer used, [j][k][xyz], for any kind of bake.
 *   - e = probe index * Nc + k is the entry's virtual index, whatever the kind.  Experiment f = 1, 2, ... of the entry is the path
 *     ct_point_radiance_launch traces for a task at array index (uint32_t)e with the probe's position, direction d(j, k) and
 *     frame f, on a handle of this cloud, light, flags and estimator in CT_MODE_SUN_MULTIPLE_SCATTER: seed
 *     tea<4>((uint32_t)(e * 4096), f).  ENTRIES 2^20 APART THEREFORE SHARE THEIR RANDOM NUMBERS, as the tasks of that entry
 *     point do.  The handle's own mode does not matter; its estimator and CT_FLAG_TEX_FIXED8 apply as everywhere.
 *   - the stored value after S experiments is the `radiance` of PointRadianceTask::addExperimentResult applied S times from
 *     (0, count 0) in frame order, in float32 with new_weight = (float)(1.0 / (double)N).
 *   - only the entries of active nodes are traced: a sparse table is 0.0f off the mask, a compact one keeps its zero block, a
 *     dense bake traces every node; the three agree bit for bit on every active node's block.
 * ct_bake_trace_more continues the fold with frames samples + 1 ..: traced(a) and then trace_more(b) are the bits of traced(a + b).
 * ct_bake_retrace, after ct_set_light, rebuilds the frame and traces from frame 1 into a zeroed second table, then swaps; a
 * failure leaves table, frame and sample count as they were.  ct_bake_update on a traced bake is CT_E_INVAL (ct_bake_retrace).
 *
 * Every ct_baked_render_* entry point, the shard ones included, ct_debug_bake_lookup and every ct_bake_* function above take a
 * traced bake as they take any other; CtBakeInfo's gather_ms and network_ms are 0.  A handle of any shard_count is accepted:
 * point tasks are not pixels.
 *
 * The calls wait for the batches in flight, run on the handle's stream and return when it is idle.  They touch neither mean, M2,
 * frame, the subframe count, samples rendered ahead nor the pose's pixel list.  CtCounters, CtFetchCounters, ct_kernel_time and
 * the armed invariants (CT_DEBUG_INVARIANTS) COUNT THE TRACED PATHS EXACTLY AS ct_point_radiance_launch COUNTS ITS OWN.  The
 * table, the direction table and everything the mask needs are allocated before the first kernel (a compact table behind the
 * mask's count, as there).  Scratch is the handle's point-task buffers: the entries go through in chunks of at most 2^20, a
 * chunk's samples in passes of at most max(1, CT_BAKE_TRACE_RESULTS / padded chunk) (default 2^24 results, 256 MiB; 64 .. 2^26);
 * the result depends neither on the chunks nor on the passes.
 *
 * CT_E_INVAL: a NULL argument (a NULL handle is answered without a device); a wrong abi_version, an unknown kind, a grid error;
 * more than 65535 samples in one call, or 0 in ct_bake_trace_more / ct_bake_retrace (ct_bake_traced with 0 samples is CT_OK: an
 * all-zero table, nothing launched); more than 2^24 samples in a table's life; a CT_FLAG_SIMPLE_KERNEL handle; a bake of another
 * handle; ct_bake_trace_more / ct_bake_retrace on a network's bake; a wrong count in ct_bake_directions.
 * CT_E_STATE: ct_bake_trace_more on a bake whose light is no longer the handle's. */
enum { CT_BAKE_DENSE = 0, CT_BAKE_SPARSE = 1, CT_BAKE_COMPACT = 2 };
typedef struct CtBakeTraceInfo {
    uint32_t traced;      /* 1: made by ct_bake_traced (a network bake answers all zeros) */
    uint32_t samples;     /* experiments folded into every stored entry of an active node so far */
    uint64_t paths;       /* estimator paths traced for this table since it was (re)started */
    double   trace_ms;    /* GPU time of the estimator launches of the last call */
    double   fold_ms;     /* GPU time of the task and fold kernels of the last call */
} CtBakeTraceInfo;       /* 32 bytes; samples at 4, paths at 8, trace_ms at 16 */

CT_API int ct_bake_traced(CtHandle h, const CtBakeDesc *d, uint32_t kind, uint32_t samples, CtBake *out);
CT_API int ct_bake_trace_more(CtHandle h, CtBake b, uint32_t samples);
CT_API int ct_bake_retrace(CtHandle h, CtBake b, uint32_t samples);   /* after ct_set_light: from sample 1, into a second table, then swap */
CT_API int ct_bake_trace_info(CtBake b, CtBakeTraceInfo *out);
/* 3 * Nphi * Nc floats, [j][k][xyz]; any kind of bake.  count must equal that number. */
CT_API int ct_bake_directions(CtBake b, float *directions_host_out, size_t count);

/* ---- the adaptive traced bake: per-entry variance and the reference's stopping rule ------------------
 *
 * ct_bake_traced gives every entry the same number of experiments and keeps only the mean.  ct_bake_traced_adaptive traces in
 * rounds, keeps m2 and count beside every mean, and after each round stops the entries that pass the reference's test
 * (PointRadianceTask.h:23-36, RadianceCollector.cpp:112-118), on the device: rule and compaction are kernels, the host reads one
 * survivor count per round.
 *
 * Grid, limits, frame, cosine[k], nodes, u_j, d(j, k), mask, list, slots, the virtual index e, validation and order of errors are
 * ct_bake_traced's for the same kind.  Experiment f of entry e is the same path: task index (uint32_t)e, seed
 * tea<4>((uint32_t)(e * 4096), f), on a CT_MODE_SUN_MULTIPLE_SCATTER copy of the scene, with the handle's estimator and
 * CT_FLAG_TEX_FIXED8.
 *
 * State per stored entry of an active node: mean (the table), m2, count, all 0 at the start.  A round: every live entry holds the
 * same count c and receives experiments c + 1 .. c + R (R = round_samples), folded in frame order with
 * PointRadianceTask::addExperimentResult's arithmetic in float32, no contraction:
 *     N = (float)count, w = (float)(1.0 / (double)N), new_mean = mean + (x - mean) * w, m2 += (x - mean) * (x - new_mean)
 * (the old mean in the first factor).  Then, in float32 with IEEE division and square root:
 *     absolute = (1.96f * sqrt(m2 / N)) / sqrt(N),  relative = absolute / (mean + FLT_EPSILON),
 *     converged = relative < rel_tol || absolute < abs_tol;  if mean < FLT_EPSILON: converged = count > zero_samples
 * (a NaN compares false).  An entry leaves the live set when it is converged or count == max_samples; the call ends when the
 * live set is empty.  In the first round every stored entry of an active node is live.  Since all live entries share c, every
 * estimator launch of a round has first_frame_id = c + 1: max_samples is a multiple of R, and a bake continues only by a higher cap.
 *
 * A dense bake traces every node, sparse and compact bakes the active ones; the three agree bit for bit in mean, m2 and count
 * on every active node's block, a sparse bake holds 0 / 0 / 0 off the mask and a compact bake 0 / 0 / 0 in its zero block.  WITH
 * THE REFERENCE'S zero_samples (100000) A DENSE BAKE RUNS EVERY NODE WHOSE RAYS MEET NO LIT CLOUD TO THE CAP: sparse and compact
 * bakes are the intended kinds.
 *
 * ct_bake_download_counts / ct_bake_download_m2 return the arrays as stored: count must equal CtBakeStorageInfo's
 * stored_entries (the virtual count for dense and sparse bakes, [slot][Nphi][Nc] for a compact one).  CT_E_INVAL on a bake that
 * is not adaptive.
 *
 * ct_bake_trace_adaptive_more(h, b, max): max is a multiple of R, greater than the current cap, at most 2^24.  Its live set is
 * the entries that reached the old cap without converging (they all hold that count); converged entries stay as they are:
 * adaptive(cap a) and then more(b) are the bits of adaptive(cap b).  ct_bake_retrace_adaptive, after ct_set_light, works as
 * ct_bake_retrace: the new frame, a zeroed second table / m2 / counts, traced with the bake's parameters and cap, then all three
 * are swapped in; a failure leaves everything as it was.
 *
 * On an adaptive bake ct_bake_trace_more, ct_bake_retrace and ct_bake_update are CT_E_INVAL (the message names the adaptive
 * call), and the two adaptive calls are CT_E_INVAL on any other bake.  ct_bake_trace_info reports traced = 1, samples = the
 * count the last round reached (rounds * R) and paths = the exact sum of the counts.  ct_baked_render_*, ct_debug_bake_lookup,
 * ct_bake_download, ct_bake_download_stored, ct_bake_directions and the other ct_bake_* functions take it as any traced bake.
 *
 * Table, m2, counts, the two live lists (one word per stored entry of an active node each; the bake keeps them for
 * ct_bake_trace_adaptive_more) and the wave counts are allocated before the first trace kernel: for a dense bake before any
 * kernel, for a sparse or compact bake behind the mask's count, which sizes them (as it sizes a compact table there); CT_E_NOMEM
 * leaves the handle as it was.  The estimator launches are ct_bake_traced's: a round's live
 * entries in chunks of at most min(2^20, CT_BAKE_TRACE_RESULTS) (whole groups of 64), a chunk's R samples in passes of at most
 * max(1, CT_BAKE_TRACE_RESULTS / padded chunk); the result depends on neither.  What the calls leave alone and what the counters
 * see is as for ct_bake_traced.
 *
 * CT_E_INVAL, before anything changes, in ct_bake_traced's order and then: a NULL parameter struct, a wrong abi_version there,
 * round_samples 0 or > 65535, a cap that is 0, no multiple of round_samples or > 2^24, a tolerance that is negative or not finite.
 * CT_E_STATE: ct_bake_trace_adaptive_more on a bake whose light is no longer the handle's. */
typedef struct CtBakeAdaptive {
    uint32_t abi_version;    /* CT_ABI_VERSION */
    uint32_t round_samples;  /* R: experiments per live entry and round, 1 .. 65535 (reference: 100) */
    uint32_t max_samples;    /* cap per entry: a multiple of R, R .. 2^24 */
    uint32_t zero_samples;   /* an entry whose mean is < FLT_EPSILON stops once count > zero_samples (reference: 100000) */
    float    rel_tol;        /* finite, >= 0 (reference: 2e-2f) */
    float    abs_tol;        /* finite, >= 0 (reference: 1e-4f) */
} CtBakeAdaptive;            /* 24 bytes */
typedef struct CtBakeAdaptiveInfo {
    uint32_t adaptive;        /* 1: made by ct_bake_traced_adaptive (any other bake answers all zeros) */
    uint32_t round_samples;   /* the bake's parameters, max_samples as ct_bake_trace_adaptive_more has left it */
    uint32_t max_samples;
    uint32_t zero_samples;
    float    rel_tol;
    float    abs_tol;
    uint32_t rounds;          /* rounds traced since the table was (re)started */
    uint32_t reserved;
    uint64_t entries_active;  /* stored entries of active nodes */
    uint64_t converged;       /* ... of them, those that passed the rule */
    uint64_t capped;          /* ... and those at max_samples that fail it */
    uint64_t paths;           /* the sum of the counts */
    double   trace_ms;        /* GPU time of the last call: the estimator launches, */
    double   fold_ms;         /* the task and fold kernels (the fold of a round's last pass evaluates the rule), */
    double   test_ms;         /* the scans and the compacting writes */
} CtBakeAdaptiveInfo;         /* 88 bytes; rounds at 24, entries_active at 32, paths at 56, trace_ms at 64 */

CT_API int ct_bake_traced_adaptive(CtHandle h, const CtBakeDesc *d, uint32_t kind, const CtBakeAdaptive *p, CtBake *out);
CT_API int ct_bake_trace_adaptive_more(CtHandle h, CtBake b, uint32_t max_samples);   /* raise the cap, continue */
CT_API int ct_bake_retrace_adaptive(CtHandle h, CtBake b);                             /* after ct_set_light */
CT_API int ct_bake_adaptive_info(CtBake b, CtBakeAdaptiveInfo *out);
CT_API int ct_bake_download_counts(CtBake b, uint32_t *counts_host_out, size_t count);
CT_API int ct_bake_download_m2(CtBake b, float *m2_host_out, size_t count);

/* ---- bake files ----------------------------------------------------------------------------------
 *
 * A bake is the most expensive object of this ABI and lived as long as its process.  ct_bake_save writes any bake to a file,
 * ct_bake_load makes a CtBake from such a file on a handle of the same cloud, ct_bake_file_info reads and checks a file without
 * a device.  The format is THIS PROJECT'S.
 *
 * Layout, little-endian: the 256-byte header below, then the sections, each starting at the next multiple of 16 bytes with the
 * gap zero-filled, in this order:
 *   1. node bytes, Nx Ny Nz of them, 0 or 1, node index (z Ny + y) Nx + x (ct_bake_mask's).  A dense bake has no such section;
 *   2. the stored table: stored_entries values, float32 (CT_BAKE_F32) or IEEE binary16 (CT_BAKE_F16), in the order of
 *      ct_bake_download_stored for a compact bake and of ct_bake_download for dense and sparse ones;
 *   3. m2, stored_entries float32, adaptive bakes only;
 *   4. counts, stored_entries uint32, adaptive bakes only;
 *   5. at the next multiple of 8 bytes, a uint64: FNV-1a 64 (offset basis 0xCBF29CE484222325, prime 0x100000001B3, byte by
 *      byte) over every byte of the file before it.  The file ends there.
 * Nothing in the file depends on the machine that wrote it beyond its endianness.
 *
 * The volume hash identifies the cloud: with i the linear index of a level-0 texel of the handle's quantised density (x fastest)
 * and t_i its byte, H = sum_i (t_i + 1) * ((i + 1) * 0x9E3779B97F4A7C15 mod 2^64) mod 2^64.  The sum does not depend on its order.
 *
 * ct_bake_save(b, path): every kind and format of bake.  Waits for the handle's stream, writes "<path>.tmp<pid>" in path's
 * directory and renames it: a failure leaves no partial file under `path` (CT_E_INVAL: the file cannot be written).  ms fields are
 * not stored.  Saving a loaded bake writes the bytes it was loaded from.
 *
 * ct_bake_file_info(path, out): no device, no handle.  CT_E_INVAL, with a message (ct_last_error(NULL)) that names the reason, for:
 * a file that cannot be read or is shorter than header and checksum; a wrong magic; an unknown version; an unknown kind or
 * format; any size outside the ranges of ct_network_bake (grid 2 .. 256, azimuths a multiple of 4 in 4 .. 64, cosines 2 .. 64,
 * entries = their product, at most 2^26 stored entries) or of ct_bake_traced / ct_bake_traced_adaptive (samples, the adaptive
 * parameters); counts that contradict each other (stored_entries against kind and active_nodes; a half or a network file that
 * claims to be adaptive); non-zero reserved bytes; a length other than the one the header implies (a truncated section); a wrong
 * checksum; node bytes other than 0 / 1 or whose number of ones is not active_nodes.
 *
 * ct_bake_load(h, path, out): ct_bake_file_info's checks, then, before anything is allocated: dims, the bits of sample_step,
 * mean_free_path_m and cloud_size_m, the estimator, the CT_FLAG_TEX_FIXED8 bit and the volume hash must be the handle's
 * (CT_E_INVAL, "a bake of another cloud / estimator", naming the field); a traced file on a CT_FLAG_SIMPLE_KERNEL handle is
 * CT_E_INVAL as in ct_bake_traced.  For sparse and compact kinds the mask is computed again on this handle by the mask kernels;
 * it must equal the file's node bytes (CT_E_INVAL), and list and slots are the recomputation's.  Everything is allocated before
 * the first copy: CT_E_NOMEM leaves the handle as it was and *out = NULL.  The bake is current when the file's light, light
 * colour and light intensity are the handle's, bit for bit; otherwise it loads with current = 0: rendering it is CT_E_STATE and
 * ct_bake_retrace / ct_bake_retrace_adaptive / ct_bake_update work on it as on any bake whose light is stale.
 *
 * A loaded bake answers every accessor as the saved one did (the ms fields are 0), renders the same frames, and continues:
 * traced(a), save, load, trace_more(b) is traced(a + b); adaptive(cap a), save, load, trace_adaptive_more(b) is adaptive(cap b)
 * in mean, m2 and counts -- the live list is made again at load by the rule and compaction kernels from the stored state: the
 * stored entries of active nodes that fail the rule, ascending (a file whose `capped` disagrees is CT_E_INVAL).  A loaded network
 * bake takes ct_bake_update.
 *
 * The header, packed (every field is naturally aligned): */
#define CT_BAKE_FILE_MAGIC "CTBAKE\r\n"   /* 8 bytes, no terminator */
#define CT_BAKE_FILE_VERSION 1u
enum { CT_BAKE_F32 = 0, CT_BAKE_F16 = 1 };
typedef struct CtBakeFileHeader {
    uint8_t  magic[8];             /*   0  CT_BAKE_FILE_MAGIC */
    uint32_t version;              /*   8  CT_BAKE_FILE_VERSION */
    uint32_t header_bytes;         /*  12  256 */
    uint32_t kind;                 /*  16  CT_BAKE_DENSE / _SPARSE / _COMPACT */
    uint32_t format;               /*  20  CT_BAKE_F32 / CT_BAKE_F16 */
    uint32_t traced;               /*  24  0 / 1 */
    uint32_t adaptive;             /*  28  0 / 1 */
    uint32_t grid[3];              /*  32  Nx, Ny, Nz */
    uint32_t azimuths;             /*  44  Nphi */
    uint32_t cosines;              /*  48  Nc */
    uint32_t margin_texels;        /*  52  M (0 for a dense bake) */
    uint64_t entries;              /*  56  the virtual count Nx Ny Nz Nphi Nc */
    uint64_t stored_entries;       /*  64  values in the table section */
    uint64_t active_nodes;         /*  72  (a dense bake: Nx Ny Nz) */
    float    light[3];             /*  80  CtBakeInfo's light, */
    float    axis_a[3];            /*  92  axis_a */
    float    axis_b[3];            /* 104  and axis_b */
    uint32_t dims[3];              /* 116  the volume the table was made on */
    uint32_t sample_step_bits;     /* 128  the bits of CtScene's sample_step, */
    uint32_t mean_free_path_bits;  /* 132  mean_free_path_m */
    uint32_t cloud_size_bits;      /* 136  and cloud_size_m */
    int32_t  estimator;            /* 140  CtEstimator */
    uint32_t tex_fixed8;           /* 144  1: the handle had CT_FLAG_TEX_FIXED8 */
    uint32_t light_color_bits[3];  /* 148  the bits of the handle's light colour */
    uint32_t light_intensity_bits; /* 160  and intensity at the bake */
    uint32_t samples;              /* 164  CtBakeTraceInfo's samples */
    uint64_t volume_hash;          /* 168  H above */
    uint64_t paths;                /* 176  CtBakeTraceInfo's paths */
    uint32_t round_samples;        /* 184  CtBakeAdaptive's parameters, max_samples as it is in force; 0 unless adaptive */
    uint32_t max_samples;          /* 188 */
    uint32_t zero_samples;         /* 192 */
    uint32_t rel_tol_bits;         /* 196 */
    uint32_t abs_tol_bits;         /* 200 */
    uint32_t rounds;               /* 204  CtBakeAdaptiveInfo's rounds, */
    uint64_t converged;            /* 208  converged */
    uint64_t capped;               /* 216  and capped */
    uint8_t  reserved[32];         /* 224  zero */
} CtBakeFileHeader;                /* 256 bytes */
typedef struct CtBakeFileInfo {
    CtBakeFileHeader header;       /*   0  as read */
    uint64_t file_bytes;           /* 256 */
    uint64_t nodes_offset;         /* 264  byte offsets of the sections; 0 for a section the file does not have */
    uint64_t table_offset;         /* 272 */
    uint64_t m2_offset;            /* 280 */
    uint64_t counts_offset;        /* 288 */
    uint64_t checksum_offset;      /* 296 */
    uint64_t checksum;             /* 304 */
} CtBakeFileInfo;                  /* 312 bytes */

CT_API int ct_bake_save(CtBake b, const char *path);
CT_API int ct_bake_file_info(const char *path, CtBakeFileInfo *out);   /* errors: ct_last_error(NULL) */
CT_API int ct_bake_load(CtHandle h, const char *path, CtBake *out);
/* Diagnostic: the handle's volume hash, by the device reduction ct_bake_save and ct_bake_load use. */
CT_API int ct_debug_volume_hash(CtHandle h, uint64_t *hash_out);

/* ---- half tables: a bake whose stored table is IEEE binary16 ---------------------------------------
 *
 * The table is the one large, randomly read array of the baked subframe.  ct_bake_half(h, src, out) makes a NEW bake with
 * format CT_BAKE_F16 from any float32 bake of h: same kind, grid, frame, mask, list and slots (copies: src stays as it is and can
 * be destroyed), its stored table the binary16 value nearest to each float32 value, ties to even, subnormals included, the
 * sign of zero kept (ct_debug_half_round is the rounding, on the host).  If any stored value is a NaN, infinite, or rounds to
 * an infinity (|v| >= 65520) the call is CT_E_INVAL -- a condition, not a measurement; the message gives the number of such
 * values and the first stored index -- with *out = NULL and nothing changed.  The conversion kernel counts them; the host reads
 * that count (4 bytes) and, only when it refuses, the index.
 *
 * The lookup of a half bake is the lookup of "the network baked into a probe table" / "the compact bake": same cell split,
 * weights, lerp order k, j, x, y, z, slot loads, no branch on activity.  Each tap pair is two adjacent binary16 values at half
 * index (probe + j) Nc + k0, widened exactly to float32 before the first lerp.  Every frame is therefore defined bit for bit by
 * the rounded table: ct_bake_download / ct_bake_download_stored return the stored values widened to float32, and the float32
 * lookup applied to them is the half bake's lookup.  Every ct_baked_render_* entry point and ct_debug_bake_lookup take it.
 *
 * A half bake is final: traced and samples are carried over for information, adaptive is 0 (no m2, no counts);
 * ct_bake_update, ct_bake_trace_more, ct_bake_retrace, ct_bake_trace_adaptive_more, ct_bake_retrace_adaptive and ct_bake_half on
 * it are CT_E_INVAL (bake again from float32); after ct_set_light it is simply not current.  ct_bake_storage_info reports
 * table_bytes = 2 * stored_entries.  The entry limits are unchanged.  ct_bake_save / ct_bake_load carry it with a 2-byte table
 * section and no m2 or counts sections. */
CT_API int ct_bake_half(CtHandle h, CtBake src, CtBake *out);
CT_API int ct_bake_format(CtBake b, uint32_t *format_out);                             /* CT_BAKE_F32 / CT_BAKE_F16 */
/* The stored bits.  count must equal stored_entries; CT_E_INVAL on a float32 bake. */
CT_API int ct_bake_download_half(CtBake b, uint16_t *table_host_out, size_t count);
CT_API uint16_t ct_debug_half_round(float x);   /* float32 -> binary16 bits, as the conversion kernel rounds (no device) */

/* ct_network_render_subframe / _accumulate / _shard_subframe / _shard_accumulate with the table in the network's place. */
CT_API int ct_baked_render_subframe(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t subframe_id, float *frame_rgba_dev);
CT_API int ct_baked_render_accumulate(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count);
CT_API int ct_baked_render_shard_subframe(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t subframe_id, float *frame_rgba_dev);
CT_API int ct_baked_render_shard_accumulate(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count);
/* Diagnostic: GPU milliseconds of the last ct_baked_render_* of this handle, one event pair around the call's kernels. */
CT_API int ct_debug_baked_render_time(CtHandle h, double *gpu_ms_out);

/* ---- hybrid frames: trace `depth` collisions, then read the bake -----------------------------------------
 *
 * The table of a traced bake is read at the FIRST collision, at the cloud's lit surface, where the multiply scattered radiance
 * varies most sharply; a few collisions further in it is smooth.  A hybrid frame of depth k follows the path tracer's own path
 * through its first k collisions, adding their NEE terms as the path tracer does, and reads the bake at collision k for
 * everything beyond: a depth knob that costs no memory.  A table entry at (x, d) stands for multipleScatterSunRadiance of a point
 * task at x with view direction d, which redirects first and then scatters with the chopped phase -- in distribution what a
 * mode-0 path still has to collect after a collision at x that it reached travelling along d.
 *
 * Defined on a handle h and a bake b with CtNetworkRender p, for subframe s and pixel (x, y); 1 <= k <= 64 and k < the scene's
 * max_depth.
 *   The path is the one ct_render_subframe draws for that pixel and subframe in CT_MODE_SUN_AND_SKY_ALL_SCATTER: seed
 *     tea<4>(x * 4096 + y, s); per bounce one draw for the flight, then getNewDirection's draws.  The flight is the march flight,
 *     whatever the handle's estimator and mode, as for ct_baked_render_*; CT_FLAG_TEX_FIXED8 applies as everywhere.
 *   If the primary ray misses the box, or its first flight has no collision inside the box, the pixel is (0, 0, 0, 1), as
 *     ct_baked_render_* gives.
 *   Otherwise S = (0, 0, 0) and for i = 1 .. k: S += the NEE at collision i (un-chopped Mie at i = 1, chopped after); if i < k
 *     the new direction is drawn and the next flight made, and if that has no collision inside the box the path has ENDED: the
 *     pixel is (S, 1).
 *   A path that reaches collision k is ALIVE at x_k, having travelled there along w_{k-1} (for k = 1 the normalised primary
 *     direction); no direction is drawn at x_k.  Its pixel is rgb_scale * g + S, alpha 1, each product rounded before its sum,
 *     where g is the transform of p (as in ct_network_render_*) applied to the lookup of b at (x_k - half box, w_{k-1}).
 *   CT_NET_ADD_SINGLE_SCATTER must be set in p for k >= 2: the frame is the path tracer's total, and without the first NEE it is
 *     no picture this library defines.  For k = 1 both settings are legal and mean what they mean for ct_baked_render_*.
 * Consequences, bit for bit: depth 1 is ct_baked_render_* with the same arguments; with a table that is 0 everywhere and a finite
 * rgb_scale the frame is ct_render_subframe's on a MARCH mode-0 handle of the same scene with max_depth = k + 1, and the number
 * of alive pixels is that handle's depth_capped; _accumulate is the loop of _subframe + ct_accumulate whatever the band size; a
 * shard writes its own tiles only and the shards sum to the frame; ct_group_baked_render_hybrid_accumulate + ct_group_merge give
 * one handle's mean and M2.
 * Every check, CT_E_STATE rule (the bake's light, a frozen image) and side effect is ct_baked_render_*'s, the counters and
 * ct_debug_baked_render_time included, and every kind of bake is taken.  The handle keeps one more temporary, 16 bytes per band
 * pixel, from the first hybrid call on.  CT_E_INVAL, each naming the value: depth 0, depth above 64, depth >= max_depth, depth
 * >= 2 without the flag.  A NULL handle is answered without a device. */
CT_API int ct_baked_render_hybrid_subframe(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t depth, uint32_t subframe_id,
                                           float *frame_rgba_dev);
CT_API int ct_baked_render_hybrid_accumulate(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t depth, uint32_t first_subframe_id,
                                             uint32_t count);
CT_API int ct_baked_render_hybrid_shard_subframe(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t depth, uint32_t subframe_id,
                                                 float *frame_rgba_dev);
CT_API int ct_baked_render_hybrid_shard_accumulate(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t depth,
                                                   uint32_t first_subframe_id, uint32_t count);

/* ---- data access -------------------------------------------------------------------- */

/* BufferBind<T>(buffer) map/copy, src/Util/BufferBind.h:11-74 (e.g. Camera.cpp:161,239-240).
 * Copies the whole buffer to dst_host; dst_bytes must equal ct_buffer_bytes(). */
CT_API int ct_download(CtHandle h, int32_t which /*CtBuffer*/, void *dst_host, size_t dst_bytes);
CT_API int ct_buffer_bytes(CtHandle h, int32_t which /*CtBuffer*/, size_t *bytes_out);

/* The other direction, for CT_BUF_MEAN and CT_BUF_M2 only: with ct_download and ct_set_subframes this is checkpoint / resume of
 * a progressive render -- (mean, M2, subframe count) IS its whole state, because a sample's seed is (pixel, subframe id): a
 * handle that is given the three continues exactly where the saved one was (the reference's own EXR dumps
 * every 40 subframes, Camera.cpp:211-214, cannot be resumed from -- no variance, no count).  src_bytes must equal
 * ct_buffer_bytes(); other buffers are CT_E_INVAL.  With ct_set_stop_when_converged the count that belongs to the buffers
 * is the FROZEN count (ct_converged_at) once the image has frozen, not ct_subframes, which goes on counting what the host
 * submits; and both ct_upload and ct_set_subframes release a frozen handle (the image they describe is a new one). */
CT_API int ct_upload(CtHandle h, int32_t which /*CtBuffer*/, const void *src_host, size_t src_bytes);

/* Raw device pointer of CT_BUF_MEAN / CT_BUF_M2 / CT_BUF_FRAME / CT_BUF_SCREEN, so a caller can
 * hand the accumulated radiance buffer to a collective (RCCL) without a copy. */
CT_API int ct_device_ptr(CtHandle h, int32_t which /*CtBuffer*/, void **ptr_out);

/* Device-to-device copy of a whole buffer into caller-owned device memory (e.g. a tensor that a
 * collective will reduce), on the handle's stream; returns after the copy completed. */
CT_API int ct_copy_to_device(CtHandle h, int32_t which /*CtBuffer*/, void *dst_dev, size_t dst_bytes);
/* Enqueued on the handle's stream, not waited for (see ct_render_accumulate_async). */
CT_API int ct_copy_to_device_async(CtHandle h, int32_t which, void *dst_dev, size_t dst_bytes);

/* Number of subframes submitted so far (Camera::subframeId, Camera.h:76); equals the samples in the buffers unless the image
 * has frozen (ct_set_stop_when_converged: ct_converged_at then names the count the buffers hold). */
CT_API int ct_subframes(CtHandle h, uint32_t *count_out);

/* After an external reduction wrote merged data into CT_BUF_MEAN/CT_BUF_M2 (multi-GPU frame
 * reduce), tell the handle how many subframes those buffers now represent. */
CT_API int ct_set_subframes(CtHandle h, uint32_t count);

CT_API int ct_counters(CtHandle h, CtCounters *out);

CT_API int ct_fetch_counters(CtHandle h, CtFetchCounters *out);

/* Milliseconds the GPU spent in the estimator kernel and in the accumulate kernel since
 * create/reset, measured with HIP events on the handle's stream, and the number of estimator
 * launches.  Any pointer may be NULL. */
CT_API int ct_kernel_time(CtHandle h, double *render_ms_out, double *accumulate_ms_out, uint64_t *launches_out);

/* Scheduler statistics of the estimator kernel since create/reset (implementation diagnostics, not
 * part of the algorithm): out[0..15] = regen phases, regen lanes, march phases, march lanes,
 * scatter phases, scatter lanes, fetched march steps, fetched steps whose 8 texels were all 0,
 * skipped (replayed) march steps, skip-loop trips (wave level), rest reserved. */
CT_API int ct_debug_stats(CtHandle h, uint64_t out[64]);
/* All `count` <= 72 diagnostic words (64..67: path conservation, 68..69: brick-line reuse of the march fetches). */
CT_API int ct_debug_stats_ex(CtHandle h, uint64_t *out, uint32_t count);
/* Diagnostics (a library built with -DCT_DIAG_TIMELINE, CT_TIMELINE=1 in the environment at ct_create, MARCH estimator): [start, end, the time it learnt that no job is left, what it
 * held then: live lanes | lanes too old to hand on << 8 | job unfinished << 16] of every wave of the last ENQUEUED estimator
 * launch, times on the device's 100 MHz wall clock, 4 * waves words (the launch that only resumes does not write it). */
CT_API int ct_debug_timeline(CtHandle h, uint64_t *out, uint32_t waves);

/* Paths that ct_render_accumulate_async launches have handed to their successors so far (diagnostic). */
CT_API int ct_debug_suspended(CtHandle h, uint64_t *paths_out);

/* Path conservation and sample integrity (diagnostic).  out[0] = 1 when the handle was created with
 * CT_DEBUG_INVARIANTS=1 in the environment: then the diagnostics build of the estimator runs, the per-sample scratch
 * is filled with NaNs before every launch, and every entry point that waits for the batches in flight checks
 *     samples dealt + paths resumed == results written + paths suspended,   paths resumed == paths suspended,
 *     samples dealt == what the host handed out,   no sample without alpha == 1 reached an accumulate kernel
 * and fails with CT_E_STATE otherwise.  out[1] = checks made, out[2] = violations, out[3] = samples without
 * alpha 1 seen by the accumulate kernels (always counted), out[4..7] = dealt, resumed, written, suspended
 * (0 unless out[0]). */
CT_API int ct_debug_invariants(CtHandle h, uint64_t out[8]);

/* The pixels of this shard under the current pose, by class (diagnostic): out[0] = the primary ray misses the box,
 * out[1] = listed (the estimator runs a path for every sample), out[2] = through pixels: the ray crosses the box without
 * meeting a non-zero density footprint, so every sample is (0,0,0,1) after the same number of lookups and none is
 * rendered -- the counters and the running mean / M2 are what rendering them would give.  out[3] = those lookups, for one
 * sample of each through pixel, summed.  Through pixels exist for the MARCH estimator's persistent kernel in modes 0 and
 * 2 unless CT_THROUGH_PIXELS=0 or CT_NO_ADVANCE=1 is in the environment at ct_create; otherwise out[2] = out[3] = 0 and
 * every box-hitting pixel is listed.  Needs a camera; not for CT_FLAG_SIMPLE_KERNEL handles. */
CT_API int ct_debug_pixel_classes(CtHandle h, uint64_t out[4]);

/* The same per pixel of the whole frame (foreign shards' pixels included), out[y * width + x] = class << 30 | steps: class
 * as above (0, 1, 2), steps = the lookups of one sample of a through pixel (0 for the other classes).  count = width *
 * height.  Downloads the prefix plane: a diagnostic for tests, not for a render loop. */
CT_API int ct_debug_pixel_class_plane(CtHandle h, uint32_t *out, size_t count);

/* Device memory of the volume representations (bytes): out[0] raw density texture, out[1] density apron bricks,
 * out[2] shadow-volume apron bricks, out[3] march bricks if stored densely, out[4] march bricks as stored,
 * out[5] = 1 when they are stored sparsely (row extents; CT_FLAG_SPARSE_BRICKS or CT_SPARSE=1), out[6] bytes of the
 * row-extent table, out[7] bytes of the coarse clearance grid.  out[5] = 2: dense addressing with sparse backing
 * (CT_FLAG_VMM_BRICKS or CT_SPARSE=2); out[3] is then the size of the address range and out[4] the memory behind it. */
CT_API int ct_debug_memory(CtHandle h, uint64_t out[8]);

/* The DELTA estimator's majorant grid and kernel variant (zeros for a MARCH handle): out[0] cell edge in texels, out[1..3] stored
 * cells per axis, out[4..6] the stored box's first cell in the virtual grid, out[7] = NEE variant (0, 1, 2) | 0x100 when every
 * non-zero texel lies two texels or more inside the volume's faces and the stored cells a texel or more inside the brick grid
 * (then a real collision is inside the box and a tentative one inside the grid by construction, and the kernel instantiated
 * without that test and that clamp runs; CT_DELTA_INTERIOR=0 keeps both). */
CT_API int ct_debug_delta_grid(CtHandle h, uint32_t out[8]);

/* The MARCH estimator's march-brick row meta bytes (bit 7 interior, bit 6 shadow-zero, bits 0-5 clearance in texels).
 * geom_out: [0] radius r of the shadow-zero flags (0: none set), [1] x bias, [2] y/z bias, [3..5] bricks per axis (3x4x4
 * texels each), [6] 1 when the bricks are sparse.  meta_out (NULL: geometry only; dense bricks only) receives one byte per
 * row, [z][y][brick x] with z, y in [0, 4 * bricks): the row of base texels x = 3 bx - x bias .. +2, y - bias, z - bias. */
CT_API int ct_debug_march_meta(CtHandle h, uint32_t geom_out[8], uint8_t *meta_out, size_t capacity);

/* The raw bytes of one of the volume layouts that ct_create builds on the device, as stored (diagnostic; tests/test_layouts.py
 * holds every one of them to a brute-force reference).  Waits for the handle's stream, fills geom_out with what is needed to
 * index the structure (unused words 0), stores its size in *bytes_out and, when dst_host is not NULL, copies it there.
 * A structure the handle does not have (twin bricks without the twin layout, the row table of dense march bricks, the
 * majorant grid of a MARCH handle), an unknown `which` and a capacity below the size answer CT_E_INVAL.
 *   CT_LAYOUT_DENSITY_BRICKS, CT_LAYOUT_SHADOW_BRICKS   128 bytes per apron brick, x fastest;
 *                             geom: [0] bias, [1..3] bricks x, y, z
 *   CT_LAYOUT_MARCH_BRICKS    128 bytes per march brick: dense x fastest, or (sparse) the stored bricks row after row;
 *                             geom: [0] x bias, [1] y/z bias, [2..4] bricks x, y, z of the dense grid, [5] 1 when sparse
 *   CT_LAYOUT_MARCH_ROWS      (sparse) two uint32 per brick row (by, bz), y fastest: index of the row's first stored brick,
 *                             first brick x | count << 16;  geom: [0] rows in y, [1] rows in z
 *   CT_LAYOUT_MARCH_COARSE    (sparse) one byte per coarse cell, x fastest;  geom: [0] log2 of the cell edge, [1..3] cells x, y, z,
 *                             [4] bias
 *   CT_LAYOUT_TWIN_BRICKS     128 bytes per twin brick, x fastest;  geom: [0] bias, [1..3] bricks x, y, z
 *   CT_LAYOUT_MAJORANT_CELLS, CT_LAYOUT_MAJORANT_CODES   one byte per stored cell, x fastest;  geom: [0] cell edge, [1] mc_div,
 *                             [2..4] stored cells x, y, z, [5..7] first stored cell, [8..10] virtual cells, [11] bias
 *   CT_LAYOUT_MIP_PYRAMID     the density pyramid that ct_collect_descriptors and ct_descriptor_frame sample (built here if neither
 *                             has run yet): one byte per texel, x fastest, level after level from level 0, level l having
 *                             max(1, n >> l) texels per axis;  geom: [0] levels, [1..3] texels x, y, z of level 0 */
enum {
    CT_LAYOUT_DENSITY_BRICKS = 0,
    CT_LAYOUT_SHADOW_BRICKS = 1,
    CT_LAYOUT_MARCH_BRICKS = 2,
    CT_LAYOUT_MARCH_ROWS = 3,
    CT_LAYOUT_MARCH_COARSE = 4,
    CT_LAYOUT_TWIN_BRICKS = 5,
    CT_LAYOUT_MAJORANT_CELLS = 6,
    CT_LAYOUT_MAJORANT_CODES = 7,
    CT_LAYOUT_MIP_PYRAMID = 8
};
CT_API int ct_debug_layout(CtHandle h, int32_t which, uint32_t geom_out[16], void *dst_host, size_t capacity, size_t *bytes_out);

/* PMC calibration probe (no handle): allocates 2^log2_lines 128-byte lines on `device`, and has one
 * thread per line issue the estimator's access pattern (two unaligned 8-byte loads at byte 13 and
 * byte 38 of a pseudo-randomly chosen, never repeated line).  Under rocprofv3 --pmc FETCH_SIZE this
 * tells how many bytes the counter reports per touched line.  Odd-numbered repeats move the second
 * load to byte 85 so that both 64-byte halves of the line are touched.  Returns a checksum. */
CT_API int ct_debug_fetch_probe(int32_t device, uint32_t log2_lines, uint32_t repeats, uint64_t *sum_out);

/* The same access shape over a WORKING SET of `ws_lines` 128-byte lines: each of 2^log2_threads lanes reads one
 * pseudo-random line of the set, so a set smaller than a cache level is re-read from that level -- the random-line
 * fill ceiling of L2 (4 MiB per XCD), of the Infinity Cache (256 MiB) and of HBM, by size.  `repeats` launches;
 * time two calls with different repeat counts and divide the difference. */
CT_API int ct_debug_fetch_probe_ws(int32_t device, uint32_t log2_threads, uint64_t ws_lines, uint32_t repeats, uint64_t *sum_out);

/* The estimator's working set (diagnostics kernels: CT_STATS=1 or CT_DEBUG_INVARIANTS=1 at ct_create).
 * ct_debug_track_lines(h, 1) allocates and clears one bit per 128-byte line of the density array the estimator reads
 * (MARCH: march bricks; DELTA: apron or twin bricks) and of the shadow volume's apron bricks; every fetch of a later
 * launch sets its line's bit; (h, 0) frees them.  ct_debug_touched_lines waits for the batches in flight and returns
 * out[0], out[1] = distinct lines touched (density, shadow), out[2], out[3] = lines in the two arrays; clear != 0
 * resets the bits. */
CT_API int ct_debug_track_lines(CtHandle h, int32_t enable);
CT_API int ct_debug_touched_lines(CtHandle h, uint64_t out[4], int32_t clear);

/* Self-test hook: the kernels' short correctly-rounded reciprocal (which = 0) and square root (which = 1) against the IEEE
 * operations for EVERY float of their range, 2^-60 <= |x| < 2^61 (reciprocal: both signs), on the device:
 * out[0] = floats tested, out[1] = mismatches (must be 0), out[2] = smallest mismatching bit pattern or 0xffffffff.
 * The same for the kernels' other device-only variants, each against what it stands for:
 *   which = 2  expf_inrange(x)   against ct_expf(x)                     every float with -87 < x <= -0.0f, and +0.0f
 *   which = 3  logf_above_one(x) against ct_logf(x)                     every positive normal float
 *   which = 4  floor_to_int(x)   against (int32_t)floorf(x)             every float with -2^31 <= x < 2^31 (zeros, subnormals)
 *   which = 5  fract_(x)         against fminf(x - floorf(x), 1 - 2^-24) every finite float */
CT_API int ct_debug_math_selftest(CtHandle h, int32_t which, uint64_t out[3]);

/* Self-test hook: ONE scalar function of the numeric contract, as the kernels compile and call it, on given operands.
 * in_bits and out_bits are host arrays of 2 * n words: the bit patterns of item i's two operands at in_bits[2i], [2i+1],
 * of its two results at out_bits[2i], [2i+1].  An unused operand is ignored, an unused result is written as 0.
 * 1 <= n <= 2^24.  fn (device expression -> results):
 *    0  ct_expf(x)            1  ct_logf(x)            2  ct_log2f(x)          3  ct_powf(x, y)
 *    4  ct_sincosf(x) -> (sin, cos)                    5  expf_inrange(x)      6  logf_above_one(x)
 *    7  div_(x, y) = x / y    8  u24_to_float(u)       9  tea4(v0, v1)        10  lcg24(state) -> (value, new state)
 *   11  floor_to_int(x)      12  fract_(x)            13  tex_weight<false>(x) 14  tex_weight<true>(x)
 * x, y are floats, u, v0, v1, state and the results of 9, 10 and 11 are 32-bit integers.  A function is evaluated on
 * whatever bits it is given, also outside the range its callers keep to. */
#define CT_MATH_FN_COUNT 15
CT_API int ct_debug_math_eval(CtHandle h, int32_t fn, const uint32_t *in_bits, uint32_t n, uint32_t *out_bits);

/* Self-test hook: k(val) of the CDF inversion (cloud.cuh:162-180) for `count` consecutive 24-bit
 * random integers starting at first_u24, evaluated by the device code; cos(theta) = (2k+1)/65536-1. */
CT_API int ct_debug_cdf_inversion(CtHandle h, uint32_t first_u24, uint32_t count, uint32_t *k_host_out);

/* ---- multi-GPU below the C ABI: one process, the GPUs of one node (SURVEY section 8b "multi-GPU is internal",
 * section 8e) ------------------------------------------------------------------------------------------------------
 * The reference is single-GPU; BASELINE.json shards the frame by pixel tile over the GPUs of a
 * node and reduces the accumulated radiance buffer with RCCL.  A CtGroup is that for a C or C++ host: one CtHandle
 * per entry of `devices` (handle i renders the tiles of shard i of `count`, see ct_tile_owner) and an RCCL
 * communicator over them (ncclCommInitAll; librccl is loaded on first use, CT_E_RCCL when it cannot be).
 * ct_group_render_accumulate enqueues the batch on every device and waits for all of them; ct_group_merge SUM-reduces
 * every shard's [mean | M2] (2 x W*H float4; foreign pixels are exactly 0, so the sum is the merged frame, bit for bit
 * the single-GPU image) onto devices[0] with one ncclReduce per device inside ncclGroupStart/End; ct_group_download,
 * ct_group_tonemap and ct_group_is_converged work on the merged frame (and merge first when needed).
 * scene->device, shard_index and shard_count are ignored.  A device may appear more than once in `devices` -- a
 * rehearsal of an N-GPU job on fewer GPUs; RCCL refuses two ranks on one device, so such a group merges with peer
 * copies and an add kernel instead of a collective.  The Python host does the same job with one process per GPU over
 * torch.distributed (deepestscatter_amd/distributed.py); both produce identical frames. */
typedef struct CtGroup_ *CtGroup;
CT_API int ct_group_create(const CtScene *scene, const int32_t *devices, uint32_t count, CtGroup *out);
CT_API int ct_group_destroy(CtGroup g);
CT_API const char *ct_group_last_error(CtGroup g);      /* g == NULL: last failure of ct_group_create in this thread */
CT_API int ct_group_size(CtGroup g, uint32_t *count_out);
CT_API int ct_group_handle(CtGroup g, uint32_t index, CtHandle *out);   /* shard `index` (owned by the group) */
CT_API int ct_group_set_camera(CtGroup g, const float eye[3], const float U[3], const float V[3], const float W[3]);
CT_API int ct_group_set_light(CtGroup g, const float direction[3], const float color[3], float intensity);   /* ct_set_light on every shard; follow with ct_group_reset */
CT_API int ct_group_render_accumulate(CtGroup g, uint32_t first_subframe_id, uint32_t count);
CT_API int ct_group_reset(CtGroup g);
CT_API int ct_group_merge(CtGroup g);
CT_API int ct_group_download(CtGroup g, int32_t which /*CT_BUF_MEAN | CT_BUF_M2*/, void *dst_host, size_t dst_bytes);
CT_API int ct_group_tonemap(CtGroup g, float exposure, uint8_t *rgba_host, float *avg_luminance_out);
CT_API int ct_group_is_converged(CtGroup g, int32_t *converged_out, uint64_t *unconverged_pixels_out);
CT_API int ct_group_counters(CtGroup g, CtCounters *out);              /* sums over the shards */

/* The scattering network on a group: one CtNetwork per shard handle, on that shard's device, from one description
 * (ct_network_create's rules and errors; the first failing shard's code and message are the group's).  Destroy it BEFORE the
 * group.  ct_group_network_render_accumulate is ct_network_render_shard_accumulate(first_subframe_id, count) on every shard --
 * shards 1 .. N-1 each on a host thread of their own, shard 0 on the caller, because the entry point is synchronous -- and
 * returns when all have finished; the first failing shard's code and message are reported then.  Like
 * ct_group_render_accumulate it sets the group's subframe count and invalidates the merge.  CT_E_INVAL: a NULL argument, a gn
 * that belongs to another group. */
typedef struct CtGroupNetwork_ *CtGroupNetwork;
CT_API int ct_group_network_create(CtGroup g, const CtNetworkDesc *d, CtGroupNetwork *out);
CT_API int ct_group_network_destroy(CtGroupNetwork gn);   /* NULL is a no-op */
CT_API int ct_group_network_render_accumulate(CtGroup g, CtGroupNetwork gn, const CtNetworkRender *p, uint32_t first_subframe_id,
                                              uint32_t count);

/* The adaptive frame on a group: one shard frame per handle (ct_adaptive_frame_create_shard's rules; the first failing shard's
 * code and message become the group's, the frames already made are destroyed and the group is left as it was), per shard a
 * staging buffer of 9 * width * height 32-bit words [mean | M2 | counts] on the shard's device, and one landing buffer of that
 * size on devices[0].  The shards must show one view: CT_E_STATE when a handle of the group was given another pose or light on
 * its own.  Destroy it BEFORE the group.
 * ct_group_adaptive_frame_update is ct_adaptive_frame_update(shard i, rounds) on every shard -- shards 1 .. N-1 each on a host
 * thread of their own, shard 0 on the caller, because the entry point is synchronous -- and returns when all have finished;
 * the first failing shard's code and message are reported then.  Shards do not wait for each other between rounds, and a shard
 * whose list empties stops.  ct_group_adaptive_frame_raise_cap checks the cap once, before any shard changes, then raises it on
 * every shard.  Both invalidate the merge.  ct_group_adaptive_frame_info: width, height, R, min, cap and tolerances as given;
 * rounds and the three times are the largest over the shards (they run concurrently); pixels, live, converged, capped and paths
 * are sums.  ct_group_adaptive_frame_shard gives shard `index`'s frame (owned by gf).
 * ct_group_adaptive_frame_merge stages every shard's three arrays and reduces them onto devices[0] with the UNSIGNED MAXIMUM OF
 * EACH 32-BIT WORD: a pixel's 36 bytes are non-zero on at most one shard, so the result is that shard's bytes for every bit
 * pattern (-0.0, NaN payloads, denormals, the integer counts) -- deliberately not ct_group_merge's float sum.  One path for every
 * device list: hipMemcpyPeerAsync into the landing buffer, then a max-into kernel on devices[0]'s stream; no collective.
 * download and device_ptr serve the merged arrays on devices[0] (CT_ADAPTIVE_MEAN, _M2, _COUNTS) and merge first when needed;
 * ct_tonemap_buffer and ct_is_converged_buffers on ct_group_handle(g, 0) take the pointers unchanged.
 * So after any sequence of update and raise_cap calls the merged mean, M2 and counts are the bytes of the frame
 * ct_adaptive_frame_create makes on one unsharded handle after the same calls, and rounds, pixels, live, converged, capped and
 * paths of the info are that frame's -- for every N and every device list, shards that own nothing and partial edge tiles
 * included.  The group's own image state (mean, M2, subframe count, merged flag) is not touched.  Nothing here has been run on
 * more than one device; a device list that repeats a device takes the same path.
 * CT_E_STATE: update and raise_cap after ct_group_set_camera or ct_group_set_light (the shards' own check; download still
 * works).  CT_E_INVAL: a NULL argument (a NULL gf is answered without a device), an index >= the group's size, a wrong `which`
 * or size, a cap that is not higher, no multiple of R or above 2^24.  Errors go to ct_group_last_error(g). */
typedef struct CtGroupAdaptiveFrame_ *CtGroupAdaptiveFrame;
CT_API int ct_group_adaptive_frame_create(CtGroup g, const CtAdaptiveFrameDesc *d, CtGroupAdaptiveFrame *out);
CT_API int ct_group_adaptive_frame_update(CtGroupAdaptiveFrame gf, uint32_t rounds);
CT_API int ct_group_adaptive_frame_raise_cap(CtGroupAdaptiveFrame gf, uint32_t max_samples);
CT_API int ct_group_adaptive_frame_info(CtGroupAdaptiveFrame gf, CtAdaptiveFrameInfo *out);
CT_API int ct_group_adaptive_frame_shard(CtGroupAdaptiveFrame gf, uint32_t index, CtAdaptiveFrame *out);   /* owned by gf */
CT_API int ct_group_adaptive_frame_merge(CtGroupAdaptiveFrame gf);
CT_API int ct_group_adaptive_frame_download(CtGroupAdaptiveFrame gf, uint32_t which, void *host, size_t bytes);
CT_API int ct_group_adaptive_frame_device_ptr(CtGroupAdaptiveFrame gf, uint32_t which, void **out);
CT_API int ct_group_adaptive_frame_destroy(CtGroupAdaptiveFrame gf);   /* NULL is a no-op; destroy before the group */

/* ---- bakes on a group: a bake built and rendered across the group's GPUs -------------------
 * A CtGroupBake holds one CtBake per shard, on that shard's device and handle.  Every call that builds or continues the bake
 *   1. cuts the nodes the build covers into one span per shard: with A = Nx Ny Nz nodes for a dense bake, the active nodes in
 *      the list's order otherwise, shard i of N owns the list positions [floor(i A / N), floor((i + 1) A / N)) in 64-bit
 *      arithmetic (deepestscatter_amd.network.bake_spans_reference restates it).  A span covers whole node blocks -- x Nphi Nc
 *      stored entries, x Nphi probes -- and may be empty (A < N, a bake without active nodes);
 *   2. lets every shard bake or trace its own span with the single-GPU call, shards 1 .. N-1 each on a host thread of their own,
 *      shard 0 on the caller.  Entry e's experiment f depends on (e, f) alone and a network record's output not on its batch, so
 *      the values are the single-GPU bake's;
 *   3. exchanges the results, so that EVERY SHARD THEN HOLDS THE COMPLETE BAKE (a shard's tiles look up anywhere in the table): a
 *      span is one contiguous range of the stored arrays -- dense [lo B, hi B) with B = Nphi Nc, compact [B + lo B, B + hi B),
 *      sparse [list[lo] B, (list[hi - 1] + 1) B), where only the zero blocks of inactive nodes lie between two shards' ranges --
 *      and every shard's range of the table (an adaptive bake: of m2 and counts too) goes to every other shard with device-to-
 *      device copies: peer copies across devices, plain copies where a device list repeats a device.  No collective, no kernel.
 *      The lists of the entries left at the cap are concatenated in shard order into every shard's live list, ascending as the
 *      single-GPU list is.  samples and rounds become the maximum over the shards (a shard whose entries all stop early ends
 *      sooner), paths and the capped count the sums, the millisecond fields the slowest shard's.
 * After a call returns CT_OK every shard's CtBake is indistinguishable -- bit for bit, for every N -- from the bake the same
 * sequence of single-GPU calls leaves on one handle of the scene: stored table, table, slots, mask, directions, m2, counts, the
 * live list, ct_bake_info, _storage_info, _sparse_info, _trace_info and _adaptive_info, the millisecond fields apart.  A file
 * saved from any shard loads on a single handle as that bake and continues as it does; a single-GPU file loads on a group
 * (ct_group_bake_load is ct_bake_load on every shard) and is continued under the same span rule.
 * ct_group_baked_render_accumulate is ct_baked_render_shard_accumulate on every shard, each on a host thread of its own as in
 * ct_group_network_render_accumulate; ct_group_merge then gives ct_baked_render_accumulate's mean and M2 of one handle, bit for
 * bit.  A build leaves the group's and the shards' image state untouched.
 * ct_group_bake_update follows ct_group_set_light; the uniform, adaptive and network calls refuse each other's bakes as the
 * single-GPU calls do: their checks are passed through from shard 0 BEFORE any shard works, and such a refusal, like every
 * argument error, leaves everything as it was.  When a shard fails in its work, the first failing shard's code and message are
 * the group's and the CtGroupBake is good for ct_group_bake_destroy only: every other call returns CT_E_STATE and says so.
 * ct_group_bake_shard gives shard `index`'s bake, owned by gb: every ct_bake_* accessor and ct_bake_save work on it, nothing that
 * changes it may be called on it.  ct_group_bake_spans: lo and hi of every shard, 2 N words of node-list positions.
 * ct_bake_half has no group form.  Nothing here has been run on more than one device; a device list that repeats a device takes
 * the same path with plain copies.  CT_E_INVAL: a NULL argument (a NULL group or gb is answered without a device), a gn or gb of
 * another group, an index >= the group's size, a wrong count.  Errors go to ct_group_last_error(g). */
typedef struct CtGroupBake_ *CtGroupBake;
CT_API int ct_group_network_bake(CtGroup g, CtGroupNetwork gn, const CtBakeDesc *d, uint32_t kind /*CT_BAKE_DENSE | _SPARSE | _COMPACT*/, CtGroupBake *out);
CT_API int ct_group_bake_traced(CtGroup g, const CtBakeDesc *d, uint32_t kind, uint32_t samples, CtGroupBake *out);
CT_API int ct_group_bake_traced_adaptive(CtGroup g, const CtBakeDesc *d, uint32_t kind, const CtBakeAdaptive *p, CtGroupBake *out);
CT_API int ct_group_bake_load(CtGroup g, const char *path, CtGroupBake *out);
CT_API int ct_group_bake_update(CtGroupBake gb, CtGroupNetwork gn);
CT_API int ct_group_bake_trace_more(CtGroupBake gb, uint32_t samples);
CT_API int ct_group_bake_retrace(CtGroupBake gb, uint32_t samples);
CT_API int ct_group_bake_trace_adaptive_more(CtGroupBake gb, uint32_t max_samples);
CT_API int ct_group_bake_retrace_adaptive(CtGroupBake gb);
CT_API int ct_group_bake_shard(CtGroupBake gb, uint32_t index, CtBake *out);   /* owned by gb */
CT_API int ct_group_bake_spans(CtGroupBake gb, uint64_t *lo_hi_out, size_t count);
CT_API int ct_group_baked_render_accumulate(CtGroup g, CtGroupBake gb, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count);
/* ct_baked_render_hybrid_shard_accumulate on every shard ("hybrid frames"), otherwise as ct_group_baked_render_accumulate. */
CT_API int ct_group_baked_render_hybrid_accumulate(CtGroup g, CtGroupBake gb, const CtNetworkRender *p, uint32_t depth,
                                                   uint32_t first_subframe_id, uint32_t count);
CT_API int ct_group_bake_destroy(CtGroupBake gb);   /* NULL is a no-op; destroy before the group */
/* Diagnostic: what shard `shard` of `shards` builds of ct_bake_traced (p == NULL) or ct_bake_traced_adaptive, alone on h: only
 * its span of the table is traced, the rest is zero.  For timing one shard's work without the others (tools/traced_bake_time.py). */
CT_API int ct_debug_bake_shard(CtHandle h, const CtBakeDesc *d, uint32_t kind, uint32_t samples, const CtBakeAdaptive *p, uint32_t shard,
                               uint32_t shards, CtBake *out);
/* Diagnostic: the bytes the last exchange of gb copied between shards and its milliseconds on the host's clock. */
CT_API int ct_debug_group_bake_exchange(CtGroupBake gb, uint64_t *bytes_out, double *ms_out);

/* ---- host-side helpers of the same path (pure CPU, no handle, no GPU) ------------------- */

/* sutil::calculateCameraVariables(..., fov_is_vertical=false), src/Util/sutil.cpp:501-524, as
 * called by Camera::updatePosition (Camera.cpp:100-134): hfov in degrees. */
CT_API int ct_calculate_camera_variables(const float eye[3], const float lookat[3], const float up[3],
                                  float hfov_deg, float aspect_ratio,
                                  float U_out[3], float V_out[3], float W_out[3]);

/* The quantiser of Resources::loadVolumeBuffer, Resources.cpp:92-141: payload float grid
 * (nx*ny*nz, x fastest) -> uint8 texture of (nx+2)(ny+2)(nz+2) with a 1-texel zero border,
 * value = (uint8)(v / max * 255) computed in double, truncating. */
CT_API int ct_quantize_volume(const float *grid_host, const uint32_t payload_dims[3], uint8_t *texture_host_out);

/* Resources::loadVolumeBuffer for a .vdb file, Resources.cpp:82-143, without OpenVDB (deepestscatter_amd/host/
 * VdbReader.h reads the file format): the FIRST grid of the file, which must be a FloatGrid; maxDensity = the largest
 * ACTIVE value; the active bounding box expanded by one voxel on every side; dense fill by getValue (inactive voxels
 * and tiles included), x fastest; uint8 = (uint8)(value / maxDensity * 255).  dims_out = the texture's size in
 * texels (what CtScene::dims wants); texture_host_out may be NULL to query dims_out / *bytes_out.  On failure the
 * message (unsupported compression codec, not a FloatGrid, ...) goes to error_out. */
CT_API int ct_load_vdb(const char *path, uint32_t dims_out[3], uint8_t *texture_host_out, size_t capacity, size_t *bytes_out,
                       char *error_out, size_t error_capacity);

/* Resources::generateMipmaps, Resources.cpp:169-209: level count = floor(log2(maxdim))+1; each
 * level is the 2x2x2 integer mean (uint16 sum / 8, zero outside).  level_offsets_out[l] = byte
 * offset of level l in `pyramid_host_out`; returns CT_E_INVAL if capacity is too small.  Pass
 * pyramid_host_out == NULL to query *levels_out and *bytes_out. */
CT_API int ct_generate_mipmaps(const uint8_t *level0_host, const uint32_t dims[3],
                        uint8_t *pyramid_host_out, size_t capacity,
                        uint32_t *levels_out, size_t *bytes_out, size_t *level_offsets_out /*[32]*/);

/* The pixel-tile -> shard map used for multi-GPU sharding: the frame is cut
 * into 8x8-pixel tiles; tile (tx,ty) belongs to shard (tx + 3*ty) mod shard_count, a skewed
 * interleave that gives every GPU the same mix of cloud and background. */
CT_API uint32_t ct_tile_owner(uint32_t tile_x, uint32_t tile_y, uint32_t shard_count);

/* The tiles of shard `shard_index` of `shard_count` of a width x height frame, as ty * tiles_x + tx (tiles_x = ceil(width / 8)),
 * ascending: the order ct_network_render_shard_* takes them in.  *count_out = their number; tiles_out == NULL queries it.
 * CT_E_INVAL: an empty frame, shard_count == 0, shard_index >= shard_count, count_out == NULL, or capacity < the count (the
 * first `capacity` tiles are written and *count_out is set all the same). */
CT_API int ct_shard_tiles(uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count, uint32_t *tiles_out,
                          uint32_t capacity, uint32_t *count_out);

/* Diagnostic, process-wide (no handle): what the library holds right now.  out[0] = device buffers, out[1] = their bytes,
 * out[2] = pinned host buffers, out[3] = their bytes.  Every allocation of the library has exactly one owner, which counts it
 * when it allocates and when it frees, so the difference around a create ... destroy pair is exactly zero in all four.  The
 * physical chunks behind CT_FLAG_VMM_BRICKS (experiments build) are not counted.  CT_E_INVAL: out == NULL. */
CT_API int ct_debug_allocations(uint64_t out[4]);

/* Synthetic cloud of SURVEY section 8(d): 5-octave gradient-noise fBm x ellipsoidal falloff,
 * thresholded, quantised by ct_quantize_volume's rule into an n^3 texture (payload n-2). */
CT_API int ct_make_procedural_cloud(uint32_t n, uint32_t seed, uint8_t *texture_host_out);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDTRACE_H */
