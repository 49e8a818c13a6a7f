/*
 * acgpt.h — C ABI of the MI355X-native path-trace hot path.
 *
 * This is the drop-in boundary for the render path of the reference's
 * PathTracer_Optix/PathTracerMain.cpp: every entry point below replaces one of
 * the plain functions that file calls over its `PathTracerState&`
 * (PathTracerMain.cpp:71-93).  The reference has no FFI layer of its own; these
 * are the symbols a cgo / JNI / ctypes / C++ binding for that path would bind.
 *
 * Conventions
 *   - every call returns 0 on success, non-zero on failure; the message is
 *     available from pt_last_error() (the reference throws sutil::Exception
 *     from CUDA_CHECK / OPTIX_CHECK, sutil/Exception.h:82-112; the C++ wrapper
 *     in acgpathtracing_amd/host re-throws to keep that convention).
 *   - the context owns every device allocation it makes; host arrays are
 *     borrowed for the duration of the call only.
 *   - a context is single-threaded (the reference is: one host thread, one
 *     stream, launch-then-sync per frame, PathTracerMain.cpp:184-210).
 *   - image row 0 is the BOTTOM row (pathTracerPrograms.cu:782-783 with
 *     sutil/Camera.cpp:34-45: V points up).
 *   - there is NO CPU fallback behind this ABI: without a HIP device
 *     pt_create() fails.
 */
#ifndef ACGPT_H
#define ACGPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_ctx pt_ctx;

typedef struct pt_float3 { float x, y, z; } pt_float3;

/* BSDFType, PathTracer_Optix/TinyObjWrapper.h:27-31 */
enum { PT_BSDF_DIFFUSE = 0, PT_BSDF_METALLIC = 1, PT_BSDF_REFRACTION = 2 };

/* Material, PathTracer_Optix/TinyObjWrapper.h:33-40 (40 bytes, same field order).
 * roughness and metallic are carried but ignored by the shading, exactly as in
 * the reference (pathTracerPrograms.cu:879-880). */
typedef struct pt_material {
    pt_float3 diffuse;
    pt_float3 emission;
    float     roughness;
    float     metallic;
    float     ior;
    int32_t   bsdfType;
} pt_material;

/* AreaLight, PathTracer_Optix/pathTracer.h:77-83 (60 bytes). */
typedef struct pt_area_light {
    pt_float3 corner;
    pt_float3 v1;
    pt_float3 v2;
    pt_float3 normal;
    pt_float3 emission;
} pt_area_light;

/* PathTraceParams, PathTracer_Optix/pathTracer.h:85-108 — field for field,
 * sizeof == 168 on LP64 like the reference's.  accumulationBuffer (float4[w*h],
 * linear radiance, alpha 1) and frameBuffer (uchar4[w*h], sRGB) are DEVICE
 * pointers supplied by the caller, as in the reference (PathTracerMain.cpp:
 * 145-148, 186-188); frameBuffer may also be pinned host memory mapped into
 * the device (the ZERO_COPY mode of sutil/CUDAOutputBuffer.h:45-51).
 * `handle` is the value returned by pt_scene_handle() (the reference stores
 * the OptixTraversableHandle there, PathTracerMain.cpp:159). */
typedef struct pt_params {
    uint32_t      currentFrameIdx;
    float*        accumulationBuffer;
    uint8_t*      frameBuffer;
    uint32_t      width;
    uint32_t      height;
    uint32_t      samplesPerPixel;
    uint32_t      maxDepth;
    pt_float3     cameraEye;
    pt_float3     cameraU;
    pt_float3     cameraV;
    pt_float3     cameraW;
    pt_area_light areaLight;
    uint64_t      handle;
    uint8_t       useDirectLighting;     /* bool */
    uint8_t       useImportanceSampling; /* bool */
} pt_params;

/* Counters of the most recent pt_launch (the reference counts nothing; Mray/s
 * is defined in SURVEY.md §8d as radiance segments + shadow rays per second). */
typedef struct pt_stats {
    uint64_t radiance_rays;   /* closest-hit segments traced                  */
    uint64_t shadow_rays;     /* next-event occlusion rays traced             */
    uint64_t paths;           /* camera paths started (= pixels * spp)        */
    float    kernel_ms;       /* megakernel duration, HIP events on its stream*/
    float    launch_ms;       /* pt_launch entry -> synchronised return       */
    uint32_t pixels;          /* pixels this launch rendered (tile partition) */
    uint32_t grid_blocks;     /* persistent workgroups launched                */
    uint32_t sample_chunks;   /* runs per pixel this launch used (pt_set_sample_chunks) */
    uint32_t variant;         /* render kernel variant that ran (pt_variant_name)      */
    /* scheduler diagnostics (0 for the segment-synchronous variant):          */
    uint64_t trav_wave_steps;   /* BVH loop iterations summed over waves       */
    uint64_t trav_lane_steps;   /* ... times lanes with a ray in flight        */
    uint64_t shade_wave_rounds; /* shade/regenerate rounds summed over waves   */
    uint64_t shade_lane_rounds; /* ... times lanes shaded in them              */
    uint64_t culled_rays;       /* camera rays that end at the scene's bounding box without a traversal: one radiance
                                 * segment that misses (pathTracerPrograms.cu:833-847); counted in radiance_rays and paths too */
    uint32_t math_mode;         /* arithmetic of the shading code this launch ran with (pt_set_math_mode)        */
    uint32_t reserved;
} pt_stats;

/* What the on-device LBVH build produced. */
typedef struct pt_bvh_info {
    uint32_t n_tris;
    uint32_t n_nodes;         /* internal nodes (n_tris - 1, or 1 if n_tris==1) */
    uint32_t max_depth;       /* longest root->leaf path, in internal nodes   */
    uint32_t stack_entries;   /* per-lane traversal stack entries reserved    */
    float    scene_lo[3];
    float    scene_hi[3];
    float    build_ms;        /* morton + sort + hierarchy + refit, device ms */
    uint32_t node_bytes;      /* bytes of the traversal node array            */
    uint32_t tri_bytes;       /* bytes of the leaf triangle array             */
    uint32_t wide_nodes;      /* four-wide tree: nodes                        */
    uint32_t wide_depth;      /* four-wide tree: levels                       */
    uint32_t wide_bytes;      /* four-wide tree: record array (nodes + triangles, 48 B each) */
    float    wide_ms;         /* collapse of the two-child tree, host ms      */
    uint32_t half_node_bytes; /* bytes of the fp16 node array (32 B per node)  */
    float    half_area_ratio; /* summed child-box area with fp16 planes / with fp32 planes (>= 1) */
    float    half_box_inflation; /* mean over the child boxes of their own fp16 / fp32 area (>= 1): large where geometry is finer than the fp16 planes */
    uint64_t device_bytes;    /* bytes of device memory the scene's arrays hold right now (ABI version 4).  A scene keeps ONE node array — the one
                               * its kernel reads: fp16 nodes (32 B per node) or fp32 nodes (64 B) — plus triangle records (48 B) and shading
                               * records (16 B); node_bytes / half_node_bytes above are the SIZES of the two formats, whichever is resident.
                               * The other array, the experiment formats and pt_temporal_blend's bsdfType per triangle (1 B) are built on first use (a ray
                               * query, pt_set_tuning, the first blend) and count from then on. */
} pt_bvh_info;

/* ---- lifetime -------------------------------------------------------------
 * pt_create   <- createDeviceContext(), PathTracerMain.cpp:240-258, plus
 *                createModule/ProgramGroups/Pipeline, :400-539 (nothing to JIT:
 *                the code object is built ahead of time for gfx950).
 * pt_destroy  <- CleanAllTheThings(), PathTracerMain.cpp:629-646.            */
int         pt_create(pt_ctx** out, int device_id);
/* A context over n_devices GPUs of one node (1 <= n <= 16; device_ids[0] is "rank 0": the caller's buffers live there).
 * Every call below then acts on the whole group: pt_set_scene builds the BVH on every device (the scene is replicated),
 * pt_launch / pt_launch_frames render with the pixel tiles of sutil/WorkDistribution.h:50-81 split over the devices — one
 * host thread and stream per device — and finish with ONE ncclReduce(SUM) (librccl, loaded on first use) of the ranks'
 * accumulation buffers into params->accumulationBuffer on rank 0, where make_color fills params->frameBuffer; every pixel
 * has exactly one non-zero term, so the buffers equal a one-device launch with the same sample-run setting bit for bit.
 * pt_get_stats sums the ranks' counters (kernel_ms: the slowest rank); queries and the memory helpers act on rank 0.
 * pt_set_partition is refused.  With ACGPT_REHEARSE_SAME_GPU=1 in the environment the same device id may be listed
 * more than once: every rank then shares that GPU and a sum kernel stands in for RCCL (a rehearsal for one-GPU boxes).   */
int         pt_create_multi(pt_ctx** out, const int* device_ids, int n_devices);
int         pt_device_count(pt_ctx* ctx);   /* devices behind the context: 1 for pt_create */
void        pt_destroy(pt_ctx* ctx);
const char* pt_last_error(pt_ctx* ctx);   /* ctx may be NULL: last global error */

/* ---- scene ------------------------------------------------------------------
 * pt_set_scene <- buildTheAccelarationStructure(), PathTracerMain.cpp:260-398
 *                 + createShaderBindingTable(), :544-627.
 * verts_xyzw: n_verts * 4 floats (w ignored; stride 16 B as :314);
 * idx: n_tris * 3 vertex indices; mat_ids: one per triangle (the reference's
 * sbtIndexOffsetBuffer, :325-328); mats: n_mats records.
 * A material id >= n_mats is an error (the reference would index past its SBT).
 * Builds the LBVH on the device; replaces any previous scene.               */
int      pt_set_scene(pt_ctx* ctx,
                      const float* verts_xyzw, size_t n_verts,
                      const uint32_t* idx, size_t n_tris,
                      const uint32_t* mat_ids,
                      const pt_material* mats, size_t n_mats);
/* Hierarchy builder used by the NEXT pt_set_scene: all start from the same on-device Morton radix
 * sort; 0 = Karras radix tree (classic LBVH), 1 = PLOC (locally-ordered clustering: fewer node visits
 * per ray), 2 = PLOC followed by an insertion-based optimisation of the tree — the default: for scenes
 * up to 16 384 triangles on the host, one node at a time (Bittner et al. 2013; 12 ms for the 1 264
 * triangles of the Cornell scenes, 2.5 % fewer visits), for larger ones on the device, all nodes at
 * once (parallel reinsertion, Meister & Bittner 2018; +73 ms at 1.31 M triangles, +0.6 s at 10.5 M,
 * render 6 % / 13 % faster); scenes above 50 000 triangles get their nodes in depth-first order.
 * Results of every query and every image bit are identical, only speed differs.                  */
int      pt_set_build_mode(pt_ctx* ctx, int mode);
uint64_t pt_scene_handle(pt_ctx* ctx);
int      pt_get_bvh_info(pt_ctx* ctx, pt_bvh_info* out);

/* ---- in-place vertex updates (OPTIX_BUILD_OPERATION_UPDATE; nothing above changes) ------------------------------------------------
 * pt_update_vertices gives the scene new vertex positions and keeps everything else of the last pt_set_scene: the index buffer, the
 * material ids and the materials.  verts_xyzw: a HOST array in pt_set_scene's layout, n_verts * 4 floats; n_verts must equal the
 * scene's vertex count.
 *   PT_UPDATE_REFIT    keeps the tree's topology and node order (the depth-first numbering of large scenes included) and recomputes
 *                      from the new vertices: the triangle records, the shading records' geometric normals, the scene box and the
 *                      triangle boxes' absolute pad, every node's box in the node array the scene keeps, the fp16 space and
 *                      pt_bvh_info.half_area_ratio / half_box_inflation.  A variant chosen per scene is chosen again as pt_set_scene
 *                      chooses it; arrays derived from the old boxes (the other node formats, the four-wide records, ...) are released
 *                      and come back on first use.  Light mode 1's list of emissive triangles is rebuilt.  Upload plus two passes over
 *                      the leaves and one over the nodes: milliseconds where a build takes a hundred.
 *   PT_UPDATE_REBUILD  pt_set_scene with the kept index buffer, ids and materials: every bit, pt_get_bvh_info included, as a fresh one.
 *   PT_UPDATE_AUTO     refits, then rebuilds if the refitted tree's area_ratio exceeds PT_UPDATE_AUTO_AREA_RATIO.
 * THE CONTRACT: after a refit every query result, every pt_render_features output and every accumulation and frame-buffer bit equals
 * what a context gets from pt_set_scene with the same arguments and the new vertices, in both math modes and both light modes (boxes only
 * prune; hits are bit-exact whatever the tree).  Only speed differs: a refitted tree over vertices that moved far from where it was
 * built has larger, more overlapping boxes.  half_area_ratio and half_box_inflation are summed in a fixed order here and with float
 * atomics by the build: they agree to about 1e-6 relative, not bit for bit.
 * area_ratio (the tree's quality): the sum of the inner nodes' surface areas divided by the root's, over the same quantity at the last
 * build — scale-invariant; 1 for unchanged vertices (exactly: summed from per-block partials in a fixed order, no float atomics), 1 after
 * a rebuild.
 * pt_scene_handle changes on every successful update, whatever the mode: a params.handle taken before is refused by pt_launch as any
 * stale handle is.  A caller refreshes it after the call, as an OptiX caller stores the handle optixAccelBuild returns from an update.
 * A pt_create_multi context updates every rank.  Refused before any device work, leaving the scene as it was: no scene, a scene without
 * triangles, a null array, a wrong n_verts, an unknown mode.
 * Memory: the context keeps host copies of the index buffer, the ids and the materials from pt_set_scene on.  The first update (or the
 * first pt_temporal_blend_motion with vertex arrays) puts the index buffer on the device (12 B per triangle); it counts in pt_bvh_info.device_bytes from then on and is freed with the scene.  Later
 * updates allocate nothing that stays.  info may be NULL.                                                                             */
typedef struct pt_update_info {
    float    ms;            /* host wall time of the call, upload included                                     */
    float    area_ratio;    /* tree quality after the update vs at the last build (>= 0; 1 = unchanged)        */
    uint32_t rebuilt;       /* 1 if the call ran a full build                                                  */
    uint32_t reserved;
} pt_update_info;
#define PT_UPDATE_REFIT   0
#define PT_UPDATE_REBUILD 1
#define PT_UPDATE_AUTO    2
#define PT_UPDATE_AUTO_AREA_RATIO 1.25f
int pt_update_vertices(pt_ctx* ctx, const float* verts_xyzw, size_t n_verts, int mode, pt_update_info* info);

/* ---- material edits (an SBT update without an accel rebuild; nothing above changes) -------------------------------------------------
 * pt_update_materials replaces the scene's material table and, optionally, which material each triangle has; the vertices, the index
 * buffer and the tree stay.  mats: a HOST array of n_mats pt_material, the whole new table (n_mats may differ from the old count).
 * mat_ids: a HOST array of n_tris ids in the caller's triangle order (pt_set_scene's), or NULL to keep every triangle's id (n_tris is
 * then ignored).  The call uploads the table, rewrites each leaf slot's material id and its shading record's bsdfType / emission tag
 * (one pass over the leaves), rebuilds light mode 1's list of emissive triangles, and releases pt_temporal_blend's bsdfType array and
 * the arrays that copy triangle records (four-wide and experiment records): they come back on first use.  The light list takes each
 * emissive triangle's v0, e1 and e2 from its triangle record — the same single subtractions pt_set_scene makes from the vertices —, so
 * no host copy of the vertices is kept; the running area sum is the host's fp32 sum in triangle order, as pt_set_scene's.
 * THE CONTRACT: afterwards every query result, every pt_render_features output, every pt_temporal_blend output and every accumulation
 * and frame-buffer bit equals what a context gets from pt_set_scene with the same vertices, index buffer, ids and table, in both math
 * modes and both light modes; so does pt_get_bvh_info except build_ms (device_bytes does not count the material table).  The kernel
 * variant chosen per scene does not depend on materials and stays.  A later pt_update_vertices(PT_UPDATE_REBUILD) builds with the new
 * table and ids.  A pt_create_multi context updates every rank.
 * pt_scene_handle changes on every successful call: a params.handle taken before is refused by pt_launch, as after pt_update_vertices.
 * Refused before any device work, leaving the scene and context as they were: a null context, no scene, a null mats while the scene
 * has triangles (or n_mats > 0), n_tris not the scene's triangle count (mat_ids given), an id not below n_mats (a kept one included
 * when mat_ids is NULL), a bsdfType outside 0..2, more than 2^24 materials — pt_set_scene's checks.
 * Memory: the table is reallocated only when n_mats changes; the call's scratch (the ids, 4 B per triangle and per light) is freed
 * before it returns.  info may be NULL; else ms is the host wall time, area_ratio 1 and rebuilt 0.                                     */
int pt_update_materials(pt_ctx* ctx, const pt_material* mats, size_t n_mats, const uint32_t* mat_ids, size_t n_tris, pt_update_info* info);

/* ---- the hot call -------------------------------------------------------------
 * pt_launch <- LaunchCurrentFrame(), PathTracerMain.cpp:184-210: consumes a
 * PathTraceParams by value, runs the megakernel over width x height pixels and
 * returns synchronised (CUDA_SYNC_CHECK, :209).  Progressive accumulation
 * follows pathTracerPrograms.cu:803-811 (running mean over currentFrameIdx).
 * maxDepth outside [1,28] and samplesPerPixel == 0 are errors
 * (PathTracerMain.cpp:42, 122-128; the do{}while(--i) at
 * pathTracerPrograms.cu:727,780 requires spp >= 1).                           */
int pt_launch(pt_ctx* ctx, const pt_params* params);

/* A batch of sub-frames in ONE kernel launch: renders frames params->currentFrameIdx ..
 * currentFrameIdx + n_frames - 1 (each samplesPerPixel samples per pixel with its own
 * tea<4>(pixel, frame) seeds) and folds them into the accumulation buffer in frame order.
 * The buffers end up bit-identical to n_frames consecutive pt_launch calls (the loop
 * of PathTracerMain.cpp:700-730 without its per-launch synchronisation); what is saved is
 * the ramp-up and drain of n_frames - 1 launches.  n_frames in [1, 64].              */
int pt_launch_frames(pt_ctx* ctx, const pt_params* params, uint32_t n_frames);

/* Upper bound on the per-launch scratch of a frame batch (one float4 per pixel and sub-frame, held until the batch is
 * blended into the accumulation buffer): pt_launch_frames runs a batch whose sums would not fit as several kernel
 * launches — same bits.  Default 1 GiB (32 sub-frames at 1920x1080); at least 1 MiB.                                   */
int pt_set_scratch_limit(pt_ctx* ctx, size_t bytes);

/* Multi-GPU pixel partition: this context renders only the pixels that
 * sutil/WorkDistribution.h:50-81 assigns to `rank` of `world` (interleaved 8x4
 * tiles, rotated per strip row); other pixels of the buffers are left
 * untouched.  world == 1 (the default) renders everything.                   */
int pt_set_partition(pt_ctx* ctx, int rank, int world);

/* After a multi-GPU reduce the root holds the summed accumulation but no colours: this applies
 * make_color (cuda/helpers.h:58-63, as pathTracerPrograms.cu:814 does per pixel) to n_pixels of
 * a float4 DEVICE array and writes uchar4 into frameBuffer (device or mapped host).          */
int pt_resolve_framebuffer(pt_ctx* ctx, const float* accumulation_rgba, uint8_t* framebuffer_rgba, size_t n_pixels);

/* Light mode (strictly opt-in, the default 0 is the reference bit for bit).
 *   0  the reference's estimator: the rectangle of params->areaLight (hard-coded at PathTracerMain.cpp:154-158), light
 *      samples and BSDF-sampled light hits both counted (pathTracerPrograms.cu:992-1026), the emitter quirks of a8/a9;
 *   1  the area light is the scene's own emissive triangles (materials with Ke != 0; params->areaLight is ignored), light
 *      sampling by area, combined with BSDF sampling by the power heuristic; a seen light contributes Ke, uniform
 *      hemisphere sampling carries its 2 cos weight: direct lighting on / off and importance sampling on / off converge to
 *      the same image.  Same random draws per segment as mode 0.  One kernel variant serves it (pt_variant_name "LIGHTS").  */
int pt_set_light_mode(pt_ctx* ctx, int mode);

/* Environment lighting: an HDR latitude-longitude map that a ray leaving the scene sees (the reference's
 * MissData::backgroundColor, 0 there, PathTracerMain.cpp:568, replaced by the map).
 *   rgb: linear radiance, HOST float[height][width][3]; row 0 is the +Y pole.  Each texel is multiplied by `scale`.
 *   rgb == NULL or width == 0 clears the map.  Refused, with the previous map left in place: width or height outside
 *   [1, 16384], more than 2^25 texels, a texel that is NaN, infinite or negative after the scale.
 * Mapping, for the unit direction d:  u = 0.5 + atan2(d.x, -d.z) / (2 pi),  v = acos(clamp(d.y, -1, 1)) / pi;
 *   texel column min(int(u W), W - 1), row min(int(v H), H - 1); nearest texel (no filtering), so that what a ray sees is what the
 *   sampling pdf assumes.  A caller rotates the map by shifting its columns.
 * Light mode 0: a radiance ray that misses returns the map's radiance (the reference's estimator otherwise; the map is not
 *   light-sampled, params->areaLight still is).  Light mode 1: the map is also a light — importance-sampled by luminance
 *   times sin(theta), chosen for a light sample with probability 0.5 beside emissive triangles (1 without; 0 for a black map),
 *   MIS with BSDF sampling by the power heuristic.
 * The map belongs to the context: it survives pt_set_scene, pt_update_vertices and pt_update_materials; under
 * pt_create_multi every rank gets it.  While a map is set pt_launch runs the "ENV" kernel variants (pt_variant_name). */
int pt_set_environment(pt_ctx* ctx, const float* rgb, uint32_t width, uint32_t height, pt_float3 scale);

/* Material model of light mode 1 (opt-in; the default, PT_MATERIALS_REFERENCE, changes nothing).
 *   PT_MATERIALS_REFERENCE (0): the reference's materials — the conductor samples its literal GGX lobe of width 0.2 with weight
 *      F Kd, glass is perfectly smooth; pt_material.roughness is not read.
 *   PT_MATERIALS_MICROFACET (1): metal and glass honour pt_material.roughness as isotropic GGX microfacet BSDFs, light-sampled and
 *      combined with BSDF sampling by the power heuristic, against emissive triangles and the environment map.  The model
 *      (tests/microfacet_ref.py states it in NumPy):
 *      - N is light mode 1's face-forwarded geometric normal, the tangent frame onb_transform's.  alpha = roughness clamped to
 *        [0, 1] (NaN: 0), the meaning of the reference's sampleGGX parameter; alpha < 1e-3 is smooth.  D is GGX, G1 Smith,
 *        G2 the height-correlated 1 / (1 + Lambda(wo) + Lambda(wi)); half vectors from Heitz 2018's visible-normal sampling.
 *      - DIFFUSE: light mode 1's code, the same draws and bits.
 *      - METALLIC, rough: wi reflected about the sampled h; weight F Kd G2 / G1(wo) with the reference's conductor Fresnel
 *        F(wo.h) (eta (1.45, 0.7, 1.55), k (3, 2.2, 3.5)); pdf G1(wo) D(h) / (4 cos_o); a wi below the plane ends the path.
 *        A light sample (triangles or map, chosen as at a diffuse vertex) is weighed against the BRDF's pdf.  Draws 2 + 2.
 *        Smooth: a mirror about N with weight F(cos_o) Kd, the same draws, no light sample (an emitter seen next counts in full).
 *      - REFRACTION, rough: Walter et al. 2007 with the material's ior (eta swapped on exit as fr_dielectric swaps it); reflection
 *        with probability F = fr_dielectric(wo.h) (1 under total internal reflection), else refraction about h; weight Kd G2 / G1(wo)
 *        for both lobes.  There is no 1 / eta^2 radiance factor, as smooth glass carries none: the BTDF is normalised as
 *        f = Kd (1 - F) D G2 eta^2 |wo.h| |wi.h| / (cos_o |cos_i| (wo.h + eta wi.h)^2), so that f |cos_i| / pdf is the sampled
 *        weight and rough glass tends to smooth glass as alpha goes to 0.  Light samples on either side use the matching lobe.
 *        Draws 3 + 2.  Smooth: light mode 1's glass, the same single draw and bits.
 *      - After a rough vertex that took a light sample, an emitter or the map hit by the sampled direction is weighed by the
 *        power heuristic against its pdf (lobe choice included), as after a diffuse vertex.  Emitters, the roulette,
 *        pt_render_features and the temporal blends are unchanged.  pt_material.metallic is not used.
 *   Model 1 is part of light mode 1's estimator: pt_launch / pt_launch_frames with model 1 in light mode 0 are refused before any
 *   device work (the buffers are left as they were).  Unknown models are refused.  The model belongs to the context: it survives
 *   pt_set_scene, pt_update_vertices and pt_update_materials; under pt_create_multi every rank gets it.  Memory: one float of alpha
 *   per material on the device, uploaded with the material table and, like it, not counted in pt_bvh_info.device_bytes.  Under
 *   model 1 pt_launch runs the "LIGHTS GGX" kernel variants (pt_variant_name). */
#define PT_MATERIALS_REFERENCE 0
#define PT_MATERIALS_MICROFACET 1
int pt_set_material_model(pt_ctx* ctx, int model);

/* Arithmetic of the shading code (closest-hit, samplers, light sample, roulette, camera-ray set-up).
 *   PT_MATH_FAST (default): the arithmetic of the reference's own build.  /root/reference/CMakeLists.txt:267 compiles
 *      pathTracerPrograms.cu with nvcc --use_fast_math (-prec-div=false -prec-sqrt=false, sinf -> __sinf, cosf -> __cosf):
 *      a / b is a * rcp(b), sqrtf / 1 / sqrtf are the approximate instructions, sin / cos of 2 pi u the hardware ones.  Here:
 *      v_rcp_f32, v_sqrt_f32, v_rsq_f32, v_sin_f32, v_cos_f32 (1 ulp each) and sqrt(1 - z) for sin(acos(sqrt(z))).
 *   PT_MATH_IEEE: correctly rounded division and square root, the C library's sincosf / acosf — the level the CPU oracle
 *      (oracle/oracle_pt.cpp) is written at; the mode in which most pixels of an image equal the oracle's bit for bit.
 * BVH traversal and the triangle test are the same code in both modes (hit triangle and distance of a given ray are bit-exact
 * either way); the modes differ in the last bits of shading values, i.e. by less than the parity tolerance (image MSE < 1e-6
 * against the oracle in both; tests/test_gpu_parity.py).  Every kernel variant of the product library exists in both modes. */
#define PT_MATH_IEEE 0
#define PT_MATH_FAST 1
int pt_set_math_mode(pt_ctx* ctx, int mode);

/* Sample chunks (1, 2, 4, 8, 16, 32; 0 = automatic, the default: 8 runs per pixel, 16 when this rank
 * holds fewer than 2^20 pixels, reduced until every run keeps at least 4 samples).  With c > 1 a pixel's samplesPerPixel samples are cut into
 * c consecutive runs, each owned by its own lane with the PRNG skipped ahead to where the run
 * starts, and the runs' partial sums are added in run order.  Same samples, same paths; only the
 * association of the fp32 sum changes ((s1+..+sk) + (sk+1+..) instead of one left-to-right chain), so
 * images differ from c = 1 in the last bits.  It shortens the per-pixel serial chain, which is what
 * bounds a launch when a GPU holds few pixels (multi-GPU tiles), and keeps neighbouring lanes on
 * similar rays.  samplesPerPixel must divide by c.
 * WHICH SETTING REPRODUCES THE REFERENCE'S SUMMATION ORDER: c = 1, and only c = 1 — one left-to-right fp32 chain per pixel, as
 * pathTracerPrograms.cu:727-780 adds its samples.  A drop-in caller who wants the reference order's last bits asks for it
 * (pt_set_sample_chunks(ctx, 1); __graft_entry__.smoke() and most parity tests do).  bench.py does NOT: it times the
 * automatic setting (8 or 16 runs per pixel; the oracle is called with the same association wherever bits are compared),
 * which is 20-30 % faster on the headline configuration and differs from c = 1 by <= 1e-4 relative on any channel. */
int pt_set_sample_chunks(pt_ctx* ctx, int chunks);

/* Launch tuning: persistent workgroups per CU (0 = from the occupancy query) and the render
 * kernel variant: -1 = chosen per scene (the default: fp16 nodes unless the scene has geometry finer than their planes —
 * pt_bvh_info.half_box_inflation above 3 —, fp32 nodes then), 0 = segment-synchronous, n >= 1 = persistent traversal
 * with deferred shading, see csrc/render_megakernel.hip.  Every variant produces the same image bits.   */
int pt_set_tuning(pt_ctx* ctx, int blocks_per_cu, int variant);
/* Human-readable description of a kernel variant, NULL past the last one.  Names starting with "DIAG"
 * are timing experiments (some deliberately compute different bits) and are never selected by default; "FAST-MATH" and
 * "LIGHTS" (the kernel of pt_set_light_mode(1)) are opt-in and compute other bits than the reference's estimator. */
const char* pt_variant_name(int variant);
/* The variant's kernel in a math mode as a kernel trace prints it ("k_render_pw<40, 16, 11, 256, 5, false, 0, 6, 2, false, 0, 0, 1>":
 * the last argument is the math mode), and a hash of the kernel sources this library was built from: what bench.py checks a
 * committed profile against before quoting it. */
const char* pt_variant_kernel(int variant, int math_mode);
const char* pt_kernel_source_hash(void);

/* Stream the launches are enqueued on (a hipStream_t, e.g. torch's current
 * stream); NULL restores the context's own stream (PathTracerMain.cpp:161). */
int pt_set_stream(pt_ctx* ctx, void* hip_stream);
int pt_get_stats(pt_ctx* ctx, pt_stats* out);

/* ---- queries used by the parity tests ------------------------------------------
 * rays: n records of 8 floats (origin xyz, direction xyz, tmin, tmax), HOST.
 * closest: t_out[i] = hit distance or -1, prim_out[i] = triangle index (in the
 * caller's index-buffer order) or 0xFFFFFFFF; interval is open (tmin, tmax),
 * two-sided, ties -> lowest triangle index.  any: hit_out[i] = 1 if any
 * triangle is hit inside the interval (traceOcclusion, pathTracerPrograms.cu:
 * 651-684).  Both bring the fp32 node array onto the device first, whatever the
 * scene holds.  pt_query_closest / pt_query_any below give the same answers for
 * rays and results in DEVICE memory, add the rest of the hit record, and walk the
 * node array the scene already holds.                                           */
int pt_trace_closest(pt_ctx* ctx, const float* rays, size_t n, float* t_out, uint32_t* prim_out);
int pt_trace_any(pt_ctx* ctx, const float* rays, size_t n, uint8_t* hit_out);

/* ---- device-resident ray queries (opt-in; nothing above changes) ---------------------------------------------------------------
 * A scene on the GPU to shoot rays at: picking, visibility and ambient-occlusion passes, probe baking, range sensors.  Rays and results
 * stay in DEVICE memory (a hipMalloc'ed or pt_device_malloc'ed buffer, a torch tensor's data_ptr()), 16-byte aligned.  Both calls
 * enqueue on the context's stream and return synchronised, act on rank 0 of a pt_create_multi context, and never write the
 * accumulation buffer, the frame buffer or pt_stats.
 *
 *   rays      n records of 8 floats, pt_trace_closest's: origin xyz, direction xyz, tmin, tmax.  The direction is not normalised and t is
 *             in units of its length; the interval (tmin, tmax) is open and two-sided; ties go to the lowest triangle index;
 *             tmax = +inf is allowed.
 *   same hits t and prim equal pt_trace_closest's, occluded equals pt_trace_any's, on every ray, as bits.
 *   nodes     the rays walk the node array the scene holds — the fp16 centre / half-extent nodes of a default scene, else the fp32
 *             nodes: pt_render_features' choice —, so pt_bvh_info.device_bytes is the same before and after a call (except under a
 *             variant forced onto another format by pt_set_tuning, which brings the fp32 nodes back as pt_trace_closest does: the first
 *             call adds 64 B per node, later calls nothing; pt_update_vertices releases them and the next call brings them again).
 *   empty     a scene without triangles (pt_set_scene with n_tris = 0) is a scene: every ray gets the miss record and occluded 0.
 *   a miss before any traversal: a non-finite origin or direction component, a NaN tmin or tmax, !(tmax > tmin), a scene without
 *             triangles.  (A zero direction needs no rule of its own: the triangle test rejects a zero determinant.)
 *   miss      {t -1, prim 0xFFFFFFFF, u 0, v 0, n (0, 0, 0), material 0xFFFFFFFF}; occluded 0
 *   hit       t the distance, prim the triangle's index in the caller's index-buffer order, material its material id;
 *             n the unit geometric normal normalize(cross(e1, e2)), negated if dot(n, dir) > 0: it faces the ray's origin;
 *             u, v the barycentrics of v1 and v2 (the point is (1 - u - v) v0 + u v1 + v v2), not clamped, recomputed once from the
 *             hit triangle with e1 = v1 - v0, e2 = v2 - v0, o the origin and d the direction, in plain fp32 multiplies and adds,
 *             left to right, and one IEEE division each (tests/query_ref.py is the NumPy statement, equal bit for bit):
 *               p = cross(d, e2);  det = dot(e1, p);  s = o - v0;  u = dot(s, p) / det;  q = cross(s, e1);  v = dot(d, q) / det
 *               cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x);  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z
 *   occluded  one byte per ray, 1 if any triangle is hit inside the interval, else 0
 * n == 0 is a no-op success.  Refused, with the context left usable: n > 0x7FFFFFFF, a null rays or output pointer with n > 0, an array
 * that is not 16-byte aligned (occluded may have any alignment), an output that overlaps the rays, a context without a scene.
 * No atomics: two calls give the same bits.                                                                                        */
typedef struct { float t; uint32_t prim; float u, v; float nx, ny, nz; uint32_t material; } pt_hit;   /* 32 bytes */
int pt_query_closest(pt_ctx* ctx, const float* rays, size_t n, pt_hit* hits);
int pt_query_any(pt_ctx* ctx, const float* rays, size_t n, uint8_t* occluded);

/* ---- the first hits of a ray in order, and how many there are (opt-in; nothing above changes) --------------------------------------
 * What a ray hits after its first hit: entry and exit pairs for thickness and penetration depth, x-ray and layered picking, multi-echo
 * range sensors, inside / outside by the parity of crossings.  One walk per ray instead of one pt_query_closest call per layer, which
 * also loses every second triangle that ties in t.  pt_query_closest's rays, rules and memory: DEVICE arrays, 16-byte aligned (counts
 * 4-byte), the call enqueues on the context's stream and returns synchronised, acts on rank 0 of a pt_create_multi context, never
 * writes the accumulation buffer, the frame buffer or pt_stats, walks the node array the scene holds (pt_bvh_info.device_bytes as for
 * pt_query_closest) and uses no atomics: two calls give the same bits.
 *
 *   a hit     a triangle that the triangle test accepts inside the open interval (tmin, tmax): exactly what pt_query_closest could
 *             return for that interval.  Each triangle counts once.
 *   hits      null with max_hits == 0, or n * max_hits records (1 <= max_hits <= PT_QUERY_MULTI_MAX), ray-major: record j of ray i is
 *             hits[i * max_hits + j].  A ray's records are its hits in ascending (t, prim): t compared as floats, equal t to the lower
 *             triangle index.  Each is pt_query_closest's full record (u, v in plain fp32, the normal towards the origin, the
 *             material); the slots past the ray's last hit hold the miss record.  Record 0 equals pt_query_closest's, bit for bit.
 *   counts    null, or n words: the number of hits of the ray in the interval, not clamped to max_hits.  0 for a miss before any
 *             traversal (pt_query_closest's list) and in a scene without triangles.
 *   the walk  with counts nothing can be pruned at a hit: the walk is cut at the ray's tmax only, and costs what the ray crosses.
 *             Without counts it is also cut behind the last kept hit once max_hits are known (widened so that a triangle that ties
 *             with that hit and has a lower index is still reached).  The hits are the same either way.
 *   NOT WATERTIGHT.  The counts are the triangle test's: Moeller-Trumbore per triangle, with no shared-edge rule.  A ray through an
 *             edge or a vertex that triangles share may count that crossing 0, 1 or several times (of 642 rays from the centre of a
 *             1 280-triangle icosphere through its own vertices, 186 count 0 and some count up to 6); rays in generic directions
 *             count every crossing once.  Parity tests should vote over several directions (pathtracer.pointsInside).
 * n == 0 is a no-op success.  Refused, with the context left usable: n > 0x7FFFFFFF, hits and counts both null, hits null with
 * max_hits != 0 or the reverse, max_hits > PT_QUERY_MULTI_MAX, a null or misaligned rays or output pointer with n > 0, an output that
 * overlaps the rays or the other output, a context without a scene.                                                                   */
#define PT_QUERY_MULTI_MAX 8
int pt_query_multi(pt_ctx* ctx, const float* rays, size_t n, uint32_t max_hits, pt_hit* hits, uint32_t* counts);

/* ---- closest-point queries on the device (opt-in; nothing above changes) ----------------------------------------------------------
 * The other question a scene on the GPU answers beside ray casts: how far is a point from the surface, and where is the nearest surface
 * point — clearance and collision checks, snapping and projection onto the mesh, distance-field baking, proximity shading, sensor
 * models.  Points and results stay in DEVICE memory, 16-byte aligned.  The call enqueues on the context's stream and returns
 * synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame buffer or pt_stats, and
 * walks the node array the scene holds exactly as pt_query_closest does (pt_bvh_info.device_bytes does not change, except under a
 * variant forced by pt_set_tuning onto a format the queries do not walk: there the first call brings the fp32 nodes, 64 B per node,
 * which stay until the next pt_set_scene or pt_update_vertices).  No atomics: two calls give the same bits.  A scene without triangles
 * (pt_set_scene with n_tris = 0) answers every point with the miss record, at max_radius = +inf too.
 *
 *   points    n records of 4 floats {x, y, z, max_radius}
 *   out       n records of 32 bytes (pt_nearest)
 *   d2        the squared distance from the point q to a triangle, all fp32, every multiply, add and division on its own, evaluated
 *             as written, no fused multiply-add (tests/nearest_ref.py is the NumPy statement, equal bit for bit).  With the vectors the
 *             build stores for the triangle, ab = e1 = v1 - v0 and ac = e2 = v2 - v0 (one fp32 subtraction per component), the region
 *             test of Ericson, Real-Time Collision Detection 5.1.5:
 *               ap = q - v0;   d1 = dot(ab, ap);  d2_ = dot(ac, ap);     dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z
 *               bp = ap - ab;  d3 = dot(ab, bp);  d4 = dot(ac, bp);
 *               cp = ap - ac;  d5 = dot(ab, cp);  d6 = dot(ac, cp);
 *               vc = d1 d4 - d3 d2_;  vb = d5 d2_ - d1 d6;  va = d3 d6 - d5 d4;  e43 = d4 - d3;  e56 = d5 - d6
 *             the first region that holds, in this order, gives the weights (v, w) of v1 and v2:
 *               vertex A  d1 <= 0 and d2_ <= 0                   (0, 0)
 *               vertex B  d3 >= 0 and d4 <= d3                   (1, 0)
 *               edge AB   vc <= 0 and d1 >= 0 and d3 <= 0        (t, 0),          t = d1 / (d1 - d3)
 *               vertex C  d6 >= 0 and d5 <= d6                   (0, 1)
 *               edge AC   vb <= 0 and d2_ >= 0 and d6 <= 0       (0, t),          t = d2_ / (d2_ - d6)
 *               edge BC   va <= 0 and e43 >= 0 and e56 >= 0      (1 - t, t),      t = e43 / (e43 + e56)
 *               face      otherwise                              (vb t, vc t),    t = 1 / ((va + vb) + vc)
 *             then the closest point c = (v0 + ab v) + ac w per component, s = q - c, d2 = dot(s, s).  One IEEE division per triangle.
 *   candidate a triangle with d2 <= max_radius * max_radius, the product taken in fp32; max_radius = +inf is allowed and its square
 *             is +inf.  A NaN d2 (a degenerate triangle can give one) is no candidate.
 *   answer    the candidate with the smallest d2; ties go to the lowest triangle index in the caller's index-buffer order
 *   found     distance = sqrtf(d2) of the winner, one IEEE square root; prim its index; u, v the weights (v, w) above: the closest point
 *             is (1 - u - v) v0 + u v1 + v v2; (cx, cy, cz) the point c as computed above; material the triangle's material id
 *   a miss before any traversal: a non-finite coordinate, a NaN or negative max_radius, a scene without triangles
 *   miss      {distance -1, prim 0xFFFFFFFF, u 0, v 0, c (0, 0, 0), material 0xFFFFFFFF}: pt_hit's pattern
 * n == 0 is a no-op success.  Refused, with the context left usable: n > 0x7FFFFFFF, a null points or out pointer with n > 0, an array
 * that is not 16-byte aligned, an output that overlaps the points, a context without a scene.                                         */
typedef struct { float distance; uint32_t prim; float u, v; float cx, cy, cz; uint32_t material; } pt_nearest;   /* 32 bytes */
int pt_query_nearest(pt_ctx* ctx, const float* points, size_t n, pt_nearest* out);

/* ---- box-overlap queries on the device (opt-in; nothing above changes) ------------------------------------------------------------
 * The third question a scene on the GPU answers beside ray casts and closest points: which triangles lie in a region of space — the
 * broad phase of collision checks, box selection, "is this cell empty" for navigation and probe placement, conservative voxelisation.
 * pt_query_multi's memory and call rules: DEVICE arrays, boxes and prims 16-byte aligned, counts 4-byte, hit any alignment; the call
 * enqueues on the context's stream and returns synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation
 * buffer, the frame buffer or pt_stats, walks the node array the scene holds (pt_bvh_info.device_bytes as for pt_query_closest) and
 * uses no atomics: two calls give the same bits.
 *
 *   boxes     n records of 8 floats {cx, cy, cz, hx, hy, hz, 0, 0}: centre and half extent of an axis-aligned box.  The last two
 *             floats are reserved and ignored.  A half extent of 0 (or -0) on any axis is allowed: a rectangle, a segment, a point.
 *   overlap   a triangle overlaps the box iff all 13 conditions below hold: the separating-axis test of Akenine-Moeller (Fast 3D
 *             Triangle-Box Overlap Testing) in keep form.  All fp32, every operation on its own, evaluated as written, no fused
 *             multiply-add (tests/overlap_ref.py is the NumPy statement, equal bit for bit), on the vectors the build stores for the
 *             triangle, v0, e1 = v1 - v0, e2 = v2 - v0, with c the centre, h the half extent, dot and cross as written under
 *             pt_query_closest, fmin3 / fmax3 = fminf / fmaxf applied twice (they ignore a NaN operand):
 *               p0 = v0 - c;  p1 = p0 + e1;  p2 = p0 + e2                                                       (per component)
 *               box faces, k in x, y, z:  fmin3(p0[k], p1[k], p2[k]) <= h[k]  and  fmax3(p0[k], p1[k], p2[k]) >= -h[k]
 *               triangle plane:           n = cross(e1, e2);  d = dot(n, p0);  r = (h.x |n.x| + h.y |n.y|) + h.z |n.z|;
 *                                         d <= r  and  d >= -r
 *               nine edge axes, f in (e1, e2 - e1, e2), i in x, y, z, j = i + 1, k = i + 2 cyclic:
 *                                         s_m = p_m[k] f[j] - p_m[j] f[k]  (m = 0, 1, 2);  r = h[j] |f[k]| + h[k] |f[j]|
 *                                         fmin3(s_0, s_1, s_2) <= r  and  fmax3(s_0, s_1, s_2) >= -r
 *             The conditions are closed: touching is overlap.  A NaN r, or three NaN s, fails its condition.  A zero-area triangle
 *             is tested like any other; its zero axes separate nothing.
 *   counts    null, or n words: the number of triangles that overlap box i, not clamped to max_prims
 *   prims     null with max_prims == 0, or n * max_prims words (1 <= max_prims <= PT_QUERY_OVERLAP_MAX), box-major:
 *             prims[i * max_prims + j] is the j-th lowest index, in the caller's index-buffer order, among the triangles that overlap
 *             box i, ascending; the slots past the last one hold 0xFFFFFFFF.  The walk is the same with and without counts: the lowest
 *             indices are known only when every overlapping triangle has been seen.
 *   hit       pt_query_overlap_any: one byte per box, 1 iff counts[i] would be non-zero.  A box's walk ends at its first accepted
 *             triangle.
 *   a miss before any traversal: a non-finite centre or half extent, a negative or NaN half extent, a scene without triangles.  It
 *             gives count 0, prims all 0xFFFFFFFF, hit 0.
 * n == 0 is a no-op success.  Refused, with the context left usable: n > 0x7FFFFFFF, prims and counts both null, prims null with
 * max_prims != 0 or the reverse, max_prims > PT_QUERY_OVERLAP_MAX, a null or misaligned boxes or output pointer with n > 0, an output
 * that overlaps the boxes or the other output, a context without a scene.                                                             */
#define PT_QUERY_OVERLAP_MAX 8
int pt_query_overlap(pt_ctx* ctx, const float* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts);
int pt_query_overlap_any(pt_ctx* ctx, const float* boxes, size_t n, uint8_t* hit);

/* ---- triangle-against-mesh intersection queries on the device (opt-in; nothing above changes) --------------------------------------
 * Which triangles of the scene does a triangle of the caller's intersect: the narrow phase of mesh-to-mesh collision, for the thing
 * that actually moves through a scene — a robot link, a tool, a character hull — where pt_query_overlap answers only for its boxes.
 * pt_query_overlap's memory and call rules, word for word: DEVICE arrays, tris and prims 16-byte aligned, counts 4-byte, hit any
 * alignment; the call enqueues on the context's stream and returns synchronised, acts on rank 0 of a pt_create_multi context, never
 * writes the accumulation buffer, the frame buffer or pt_stats, walks the node array the scene holds (pt_bvh_info.device_bytes as for
 * pt_query_closest) and uses no atomics: two calls give the same bits.
 *
 *   tris      n records of 12 floats {a0.xyz, 0, a1.xyz, 0, a2.xyz, 0}: the three vertices of a query triangle.  The fourth float of
 *             each vertex is reserved and ignored.
 *   intersect a scene triangle intersects the query triangle iff all 20 conditions below hold: a separating-axis test in keep form.
 *             All fp32, every operation on its own, evaluated as written, no fused multiply-add (tests/tritri_ref.py is the NumPy
 *             statement, equal bit for bit), on the vectors the build stores for the scene triangle, v0, e1 = v1 - v0, e2 = v2 - v0;
 *             dot and cross as written under pt_query_closest, fmin3 / fmax3 = fminf / fmaxf applied twice (they ignore a NaN
 *             operand), vector sums and differences per component:
 *               w1 = v0 + e1;  w2 = v0 + e2
 *               boxes, k in x, y, z:  fmin3(v0[k], w1[k], w2[k]) <= fmax3(a0[k], a1[k], a2[k])  and
 *                                     fmax3(v0[k], w1[k], w2[k]) >= fmin3(a0[k], a1[k], a2[k])
 *               f1 = a1 - a0;  f2 = a2 - a0;  p0 = v0 - a0;  p1 = p0 + e1;  p2 = p0 + e2
 *               axis(L):  s_m = dot(L, p_m)  (m = 0, 1, 2);  t1 = dot(L, f1);  t2 = dot(L, f2);
 *                         fmin3(s_0, s_1, s_2) <= fmax3(0, t1, t2)  and  fmax3(s_0, s_1, s_2) >= fmin3(0, t1, t2)
 *               nA = cross(f1, f2);  nB = cross(e1, e2)
 *               17 axes:  nA;  nB;  cross(a, b) for a in (f1, f2 - f1, f2) and b in (e1, e2 - e1, e2);
 *                         cross(nA, a) for the three a;  cross(nB, b) for the three b
 *             The three box conditions compare coordinates as they are, without a subtraction: a pair that is kept has bounding
 *             boxes that overlap exactly, which is what lets the walk prune by boxes.  The six in-plane axes cross(n, edge) are
 *             what separates two coplanar triangles: the other eleven are all parallel to the common normal there.  The conditions
 *             are closed: touching is intersecting.  Three NaN s fail their condition; a NaN t is ignored.
 *             A zero-area triangle on either side (a segment, a point) is tested like any other.  The test then never misses an
 *             intersection, but it may keep a pair that is apart within a common plane: a segment's own in-plane normal is not
 *             among the axes, since its n = 0 makes cross(n, edge) = 0.  For exact segment queries use pt_query_any.
 *   counts    null, or n words: the number of scene triangles that intersect query triangle i, not clamped to max_prims
 *   prims     null with max_prims == 0, or n * max_prims words (1 <= max_prims <= PT_QUERY_TRIANGLES_MAX), query-major:
 *             prims[i * max_prims + j] is the j-th lowest index, in the caller's index-buffer order, among the triangles that
 *             intersect query i, ascending; the slots past the last one hold 0xFFFFFFFF.
 *   hit       pt_query_triangles_any: one byte per query, 1 iff counts[i] would be non-zero.  A query's walk ends at its first
 *             accepted triangle.
 *   a miss before any traversal: any of the nine coordinates non-finite, a scene without triangles.  It gives count 0, prims all
 *             0xFFFFFFFF, hit 0.
 * The walk's boxes only prune; which pairs intersect is decided by the test above alone.
 * n == 0 is a no-op success.  Refused, with the context left usable: n > 0x7FFFFFFF, prims and counts both null, prims null with
 * max_prims != 0 or the reverse, max_prims > PT_QUERY_TRIANGLES_MAX, a null or misaligned tris or output pointer with n > 0, an output
 * that overlaps the triangles or the other output, a context without a scene.                                                         */
#define PT_QUERY_TRIANGLES_MAX 8
int pt_query_triangles(pt_ctx* ctx, const float* tris, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts);
int pt_query_triangles_any(pt_ctx* ctx, const float* tris, size_t n, uint8_t* hit);

/* ---- complete result lists in compressed-sparse-row form (opt-in; nothing above changes) --------------------------------------------
 * pt_query_overlap and pt_query_triangles give a count and at most 8 indices.  These three calls give every index: a selection box,
 * the narrow phase behind a broad phase, the triangles of each cell of a voxeliser.  The caller's sequence:
 *     pt_query_overlap(ctx, boxes, n, 0, NULL, counts);                      the number per query (unchanged code)
 *     pt_list_offsets(ctx, counts, n, offsets, &total);                      counts -> offsets
 *     allocate total words;
 *     pt_query_overlap_lists(ctx, boxes, n, offsets, prims, total, NULL);    query i's list is prims[offsets[i] .. offsets[i + 1])
 * and the same with pt_query_triangles / pt_query_triangles_lists.  Nothing is allocated behind the caller's back but one small
 * scratch buffer the context owns (the scan's tile sums and one flag word: 8 bytes per 2048 counts, grown on demand, freed by
 * pt_destroy, not part of pt_bvh_info.device_bytes, which describes the scene).
 *
 * pt_list_offsets: offsets[0] = 0, offsets[i + 1] = offsets[i] + counts[i].
 *   counts    n DEVICE words, 4-byte aligned
 *   offsets   n + 1 DEVICE words, 4-byte aligned, not overlapping counts (the scan is not in place)
 *   total     a HOST pointer or null: receives the sum of all counts as 64 bits
 * All arithmetic is integer (the sums are 64-bit inside), so any schedule gives the same bits.  n == 0 with a non-null offsets writes
 * the single 0 and *total = 0.  A sum above 0xFFFFFFFF is refused after it has been computed: *total is set, so that the caller can
 * split the batch; offsets is then unspecified.  Also refused, with the context left usable: n > 0x7FFFFFFF, a null or misaligned
 * pointer with n > 0 (a null offsets with n == 0 is a no-op success), offsets overlapping counts, a null context.  The call needs no
 * scene; it enqueues on the context's stream, returns synchronised, and acts on rank 0 of a pt_create_multi context.
 *
 * pt_query_overlap_lists / pt_query_triangles_lists:
 *   boxes, tris   exactly the records of pt_query_overlap / pt_query_triangles.  Which triangles belong to a query is decided by the
 *             same 13 / 20 conditions and the same misses before any traversal, word for word.
 *   offsets   n + 1 DEVICE words, 4-byte aligned: the slices.  Normally pt_list_offsets' of the counts of these queries on this scene.
 *   prims     capacity DEVICE words, 4-byte aligned (null is allowed with capacity == 0).  prims[offsets[i] .. offsets[i + 1]) receives
 *             every accepted triangle index of query i, in the caller's index-buffer order, ascending.  Ascending is part of the
 *             contract and does not depend on the tree: the lists are equal after pt_update_vertices in refit and in rebuild mode,
 *             under every build mode and under both node formats.
 *   capacity  the number of words prims holds.  A query whose slice does not satisfy offsets[i] <= offsets[i + 1] <= capacity writes
 *             nothing and raises the mismatch flag.  No word outside the slices is ever written, whatever offsets contains: stale
 *             offsets cannot write out of bounds.
 *   found     null, or n DEVICE words, 4-byte aligned: the number of triangles accepted on this walk, which is what counts would be.
 *   A slice longer than the number found holds 0xFFFFFFFF in its surplus slots, after the indices: offsets taken from counts plus a
 *   margin are accepted without a flag if and only if every slice is at least as long as its list.  A slice shorter than the number
 *   found has unspecified contents; the writes still stay inside the slice, and the query raises the mismatch flag.
 *   When any query raised the flag the call returns non-zero after the lists have been written and found is complete; pt_last_error
 *   says that the offsets do not fit this scene and these queries.  The context stays usable.  (The flag is one device word in the
 *   context's scratch: cleared before the launch, set by a plain store of 1 — no atomic, every writer stores the same value — and read
 *   after the sync.)
 * Everything else is pt_query_overlap's: DEVICE arrays, boxes / tris 16-byte aligned; the call enqueues on the context's stream and
 * returns synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame buffer or
 * pt_stats, and two calls give the same bits.  n == 0 is a no-op success.  Refused, with the context left usable: n > 0x7FFFFFFF, a
 * null boxes / tris, offsets or prims with n > 0 (prims may be null with capacity == 0), a misaligned pointer, any two of the four
 * spans (records, offsets, prims, found) overlapping, a context without a scene.                                                     */
int pt_list_offsets(pt_ctx* ctx, const uint32_t* counts, size_t n, uint32_t* offsets, uint64_t* total);
int pt_query_overlap_lists(pt_ctx* ctx, const float* boxes, size_t n, const uint32_t* offsets,
                           uint32_t* prims, size_t capacity, uint32_t* found);
int pt_query_triangles_lists(pt_ctx* ctx, const float* tris, size_t n, const uint32_t* offsets,
                             uint32_t* prims, size_t capacity, uint32_t* found);

/* ---- oriented-box overlap queries on the device (opt-in; nothing above changes) ----------------------------------------------------
 * pt_query_overlap for a box in a frame of its own: a robot link, a vehicle hull, a tool, a selection gizmo, the cells of a grid that
 * is turned against the world.  The world AABB of such a box reports many times the triangles and calls free space occupied; its
 * twelve surface triangles miss everything that lies inside it.  The three calls are pt_query_overlap, pt_query_overlap_any and
 * pt_query_overlap_lists with another record and another statement; everything else is theirs, word for word: the memory rules (DEVICE
 * arrays, boxes and prims 16-byte aligned, counts / offsets / found 4-byte, hit any alignment), the refusals, which leave the context
 * usable, PT_QUERY_OVERLAP_MAX, the max_prims / counts combinations, the CSR contract with pt_list_offsets (ascending, surplus slots
 * 0xFFFFFFFF, the mismatch flag, no write outside a slice whatever offsets holds), rank 0 of a pt_create_multi context, no atomics —
 * two calls give the same bits —, device_bytes unchanged.
 *
 *   boxes     n records of 16 floats, 64 bytes: {m[0..11] | hx, hy, hz, 0}.  m is a row-major 3 x 4 matrix laid out exactly as a pose
 *             of pt_query_poses_* (below); the box is the image of [-h, h] under m.  Its axes in world coordinates are the columns of
 *             the 3 x 3 part, u = (m0, m4, m8), v = (m1, m5, m9), w = (m2, m6, m10), its centre is c = (m3, m7, m11).  The last
 *             float is reserved and ignored.  A half extent of 0 (or -0) is allowed: rectangles, segments, points.
 *   overlap   all fp32, every operation on its own, evaluated as written, no fused multiply-add (tests/oriented_ref.py is the NumPy
 *             statement, equal bit for bit).  A world vector p has the local coordinates
 *               L(p) = ((m0 p.x + m4 p.y) + m8 p.z,  (m1 p.x + m5 p.y) + m9 p.z,  (m2 p.x + m6 p.y) + m10 p.z)
 *             and on the triangle's stored vectors v0, e1, e2:  P0 = L(v0 - c),  E1 = L(e1),  E2 = L(e2).  The triangle overlaps the box
 *             iff the 13 conditions of pt_query_overlap hold for centre (0, 0, 0), half extent h and the vectors (P0, E1, E2) in the
 *             place of (v0, e1, e2).  The edges are rotated, not formed again from rotated points: with the exact identity as the
 *             3 x 3 part the statement reproduces pt_query_overlap's answers.
 *   a miss before any traversal: a non-finite value among the first 15 floats; a negative or NaN half extent; a scene without
 *             triangles; axes that are not orthonormal: with dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z the record is searchable only
 *             if |dot(u,u) - 1|, |dot(v,v) - 1|, |dot(w,w) - 1|, |dot(u,v)|, |dot(v,w)| and |dot(w,u)| are all <= 2^-10.  Mirrors
 *             pass; a rotation built in fp32 from a quaternion is within 2e-7.  The rule lets the walk bound the box in world space
 *             without inverting a matrix; it is part of the statement.  A miss gives count 0, prims all 0xFFFFFFFF, hit 0.
 *
 * pt_pose_boxes turns poses that are on the device already into oriented-box records: record p is pose p with its fourth column
 * replaced by the pose statement (below, "pose") applied to local_box[0..2], followed by {local_box[3..5], 0}.  local_box is a HOST
 * pointer: centre and half extent of the box in the mesh's own frame.  poses and boxes_out are DEVICE, 16-byte aligned, P * 48 and
 * P * 64 bytes, and must not overlap.  The call needs neither a scene nor a query mesh.  P == 0 is a no-op success.  Refused: a null
 * context or argument, P > 0x7FFFFFFF, a negative or non-finite local_box, a misaligned array, boxes_out overlapping the poses.       */
int pt_query_overlap_oriented(pt_ctx* ctx, const float* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts);
int pt_query_overlap_oriented_any(pt_ctx* ctx, const float* boxes, size_t n, uint8_t* hit);
int pt_query_overlap_oriented_lists(pt_ctx* ctx, const float* boxes, size_t n, const uint32_t* offsets,
                                    uint32_t* prims, size_t capacity, uint32_t* found);
int pt_pose_boxes(pt_ctx* ctx, const float* poses, size_t P, const float local_box[6], float* boxes_out);

/* ---- swept-sphere casts on the device (opt-in; nothing above changes) --------------------------------------------------------------
 * How far a ball of radius r travels along a direction before it touches the mesh, and where it touches: the sphere cast of physics
 * and robotics libraries — continuous collision, character and camera controllers, path clearance of a round robot, thick rays and
 * beam-width sensors.  pt_query_nearest's memory and call rules: DEVICE arrays, 16-byte aligned (blocked: any alignment); the call
 * enqueues on the context's stream and returns synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation
 * buffer, the frame buffer or pt_stats, walks the node array the scene holds (pt_bvh_info.device_bytes as for pt_query_closest) and
 * uses no atomics: two calls give the same bits.
 *
 *   sweeps    n records of 8 floats {ox, oy, oz, dx, dy, dz, radius, tmax}.  The sphere's centre moves along o + t d for
 *             0 <= t <= tmax, closed at both ends.  d is not normalised and t is in units of its length.  tmax = +inf and radius = 0
 *             are allowed.
 *   time of impact of one triangle: the entry of the centre line into the triangle's Minkowski sum with the sphere — a start-overlap
 *             test, three vertex spheres, three edge cylinders, two offset faces —, the smallest candidate t below.  All fp32, every
 *             operation on its own, evaluated as written, no fused multiply-add, IEEE division and square root (tests/sweep_ref.py
 *             is the NumPy statement, equal bit for bit), on the vectors the build stores for the triangle, v0, e1 = v1 - v0,
 *             e2 = v2 - v0; dot and cross as written under pt_query_closest; x + y * s for vectors is per component, one multiply
 *             and one add; dd = dot(d, d), rr = r * r:
 *               start overlap   d2 of pt_query_nearest's closest_on_triangle at o; d2 <= rr: candidate t = 0
 *               vertex P in (v0, v0 + e1, v0 + e2):
 *                               m = o - P;  t0 = (-dot(m, d)) / dd;  mp = m + d * t0;  q = (rr - dot(mp, mp)) / dd;  t = t0 - sqrt(q);
 *                               candidate iff q >= 0 and t >= 0
 *               edge (A, E) in ((v0, e1), (v0, e2), (v0 + e1, e2 - e1)):
 *                               m = o - A;  ee = dot(E, E);  md = dot(m, E);  nd = dot(d, E);
 *                               mp = m - E * (md / ee);  dp = d - E * (nd / ee);  a = dot(dp, dp);
 *                               t0 = (-dot(mp, dp)) / a;  mq = mp + dp * t0;  q = (rr - dot(mq, mq)) / a;
 *                               t = t0 - sqrt(q);  s = md + t * nd;
 *                               candidate iff q >= 0, t >= 0 and 0 <= s <= ee
 *               face            n = cross(e1, e2);  nn = dot(n, n);  m = o - v0;  s0 = dot(n, m);
 *                               t = ((s0 >= 0 ? r : -r) * sqrt(nn) - s0) / dot(n, d);  w = m + d * t;
 *                               u = dot(cross(w, e2), n) / nn;  v = dot(cross(e1, w), n) / nn;
 *                               candidate iff t >= 0, u >= 0, v >= 0 and u + v <= 1
 *             The residuals mp, mq are projected before they are squared: the textbook b^2 - a c loses the contact to cancellation
 *             (DESIGN.md section 28).  Every compare is false on a NaN, so a NaN anywhere makes that feature no candidate: a
 *             degenerate triangle keeps the features that are defined, and with d = 0 only the start overlap can answer.
 *   the answer over all triangles, the smallest finite time of impact t <= tmax; ties go to the lowest index in the caller's index-buffer
 *             order.  The walk's boxes only prune; the winner is decided by the test above alone.
 *   hits      per sweep {t, prim, u, v, cx, cy, cz, material}: the time of impact, the winning triangle, then pt_query_nearest's
 *             weights of v1 and v2 and closest point, from closest_on_triangle evaluated once on the winner at the centre
 *             o + d * t (one multiply and one add per component), and the triangle's material id.  The contact normal is the caller's
 *             (centre - c) / r.  A miss is {-1, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0xFFFFFFFF}.
 *   blocked   pt_query_sweep_any: one byte per sweep, 1 iff some triangle has a time of impact t <= tmax (iff hits[i].t >= 0).  A
 *             sweep's walk ends at its first such triangle: "can the ball move along this segment".
 *   a miss before any traversal: a non-finite component of o or d, a radius that is NaN, negative or infinite, a NaN or negative
 *             tmax, a scene without triangles.
 * Not watertight at shared edges: neighbouring triangles compute a shared edge's cylinder (and a shared vertex's sphere) from their own
 * stored vectors, and the two times may differ in their last bits; the smaller wins, whichever triangle it belongs to.
 * n == 0 is a no-op success.  Refused, with the context left usable: n > 0x7FFFFFFF, a null pointer, a misaligned sweeps or hits array,
 * an output that overlaps the sweeps, a context without a scene.                                                                       */
typedef struct { float t; uint32_t prim; float u, v; float cx, cy, cz; uint32_t material; } pt_sweep_hit;   /* 32 bytes */
int pt_query_sweep(pt_ctx* ctx, const float* sweeps, size_t n, pt_sweep_hit* hits);
int pt_query_sweep_any(pt_ctx* ctx, const float* sweeps, size_t n, uint8_t* blocked);

/* ---- swept-capsule casts on the device (opt-in; nothing above changes) -------------------------------------------------------------
 * How far a capsule — a segment with a radius: a character, a camera boom, a robot link — travels along a direction before it touches
 * the mesh, and where: the capsule cast that physics libraries offer beside the sphere cast.  Sampling spheres along the axis and
 * casting each misses every contact between the samples, a vertex or an edge of the mesh that meets the cylinder's side.
 * pt_query_sweep's memory and call rules: DEVICE arrays, 16-byte aligned (blocked: any alignment); the call enqueues on the context's
 * stream and returns synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame buffer
 * or pt_stats, walks the node array the scene holds and uses no atomics: two calls give the same bits.
 *
 *   casts     n records of 12 floats {p0.x, p0.y, p0.z, radius | p1.x, p1.y, p1.z, tmax | d.x, d.y, d.z, ignored}; the first eight have
 *             the layout of a pt_query_segments record.  The twelfth float is never read into a decision.  The capsule's axis is
 *             {p0 + t d, p1 + t d} for 0 <= t <= tmax, closed at both ends.  d is not normalised and t is in units of its length.
 *             radius = 0 (a swept segment), tmax = +inf and p1 == p0 (a sphere) are allowed.
 *   time of impact of one triangle: the entry of the line p0 + t d into the r-offset of the prism K = triangle + (-[0, a]),
 *             a = p1 - p0 (one subtraction per component).  K has 6 vertices, 9 edges and 5 faces, and outside K the distance to K is
 *             the distance to its faces, so the time is the smallest candidate of the twenty-two sub-tests below.  All fp32, every
 *             operation on its own, evaluated as written, no fused multiply-add, IEEE division and square root (tests/capsule_ref.py
 *             is the NumPy statement, equal bit for bit), on the stored v0, e1, e2; dd = dot(d, d), rr = r * r; "vertex", "edge" and
 *             "face" are pt_query_sweep's three feature forms above with the m and E given here:
 *               at p0           pt_query_sweep's seven features other than the start overlap, with o = p0
 *               at p1           the same seven with o = p1, p1 as the record gives it (not p0 + a)
 *               axis edge       P in (v0, v0 + e1, v0 + e2): the edge form with m = p1 - P, E = a
 *               side face       (A, E) in ((v0, e1), (v0, e2), (v0 + e1, e2 - e1)): the face form with m = p1 - A, E in the place of e1
 *                               and a in the place of e2; candidate iff t >= 0, 0 <= u <= 1 and 0 <= v <= 1
 *               start overlap   d2 of pt_query_segments' statement for the segment {p0, p1} (its d = a, its a = dot(a, a)) against the
 *                               triangle; d2 <= rr: t = 0, whatever the candidates say
 *             Every compare is false on a NaN, so a degenerate feature — a = 0, E parallel to a, d parallel to a, d = 0 — simply is
 *             no candidate.  What two sub-tests share depends on E and d alone and may be computed once: the bits do not change.
 *   the answer over all triangles, the smallest finite time of impact t <= tmax; ties go to the lowest index in the caller's
 *             index-buffer order.  The walk's boxes only prune; the winner is decided by the test above alone.
 *   hits      per cast {t, prim, s, feature, cx, cy, cz, material}: the time of impact, the winning triangle, then pt_query_segments'
 *             (s, feature, c) for the segment {p0 + d * t, p1 + d * t} (one multiply and one add per component) against the winner,
 *             evaluated once after the walk: the parameter on the axis and the point of the triangle where the two come closest, and
 *             the triangle's material id.  The point on the axis is p0' + (p1' - p0') * s and the contact normal the caller's
 *             (axis point - c) / r.  A miss is pt_segment_hit's: {-1, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0xFFFFFFFF}.
 *   blocked   pt_query_capsule_cast_any: one byte per cast, 1 iff some triangle has a time of impact t <= tmax (iff hits[i].t >= 0).  A
 *             cast's walk ends at its first such triangle.
 *   a miss before any traversal: a non-finite component of p0, p1, a or d, a radius that is NaN, negative or infinite, a NaN or
 *             negative tmax, a scene without triangles.
 * Not watertight at shared edges, as pt_query_sweep is not.  n == 0 is a no-op success.  Refused, with the context left usable:
 * n > 0x7FFFFFFF, a null pointer, a misaligned casts or hits array, an output that overlaps the casts, a context without a scene.   */
typedef struct { float t; uint32_t prim; float s, feature; float cx, cy, cz; uint32_t material; } pt_capsule_cast_hit;   /* 32 bytes */
int pt_query_capsule_cast(pt_ctx* ctx, const float* casts, size_t n, pt_capsule_cast_hit* hits);
int pt_query_capsule_cast_any(pt_ctx* ctx, const float* casts, size_t n, uint8_t* blocked);

/* ---- swept oriented-box casts on the device (opt-in; nothing above changes) ---------------------------------------------------------
 * How far an oriented box — a vehicle hull, a crate, a robot link with a square section, a door, a camera volume — travels along a
 * direction before it touches the mesh, which triangle it touches, with which normal and where: the box cast that physics libraries
 * offer beside the sphere and the capsule cast.  Casting the 12 triangles of the box's surface with pt_query_triangle_cast misses every
 * triangle that starts wholly inside the solid box.  pt_query_capsule_cast's memory and call rules: DEVICE arrays, 16-byte aligned
 * (blocked: any alignment); the call enqueues on the context's stream and returns synchronised, acts on rank 0 of a pt_create_multi
 * context, never writes the accumulation buffer, the frame buffer or pt_stats, walks the node array the scene holds and uses no
 * atomics: two calls give the same bits.
 *
 *   casts     n records of 20 floats {m0 .. m11 | hx hy hz - | d.x d.y d.z tmax}: the first sixteen are a pt_query_overlap_oriented
 *             record word for word (the sixteenth is never read).  The box occupies centre c + t d for 0 <= t <= tmax, closed at both
 *             ends.  d is not normalised and t is in units of its length.  tmax = +inf is allowed and stands for the largest finite
 *             float.  A half extent may be 0: a swept rectangle, segment or point.
 *   time of impact of one triangle: in the box's frame the box is the cube |q_j| <= h_j and the triangle translates by -L(d) t; the
 *             time is the entry of that line into the Minkowski difference of triangle and cube, a convex polytope whose face normals
 *             are the 13 axes of pt_query_overlap's test.  All fp32, every operation on its own, evaluated as written, no fused
 *             multiply-add, IEEE division and square root (tests/boxcast_ref.py is the NumPy statement, equal bit for bit), on the
 *             stored v0, e1, e2.  With L pt_query_overlap_oriented's local:  P0 = L(v0 - c), E1 = L(e1), E2 = L(e2), D = L(d),
 *             V = (-D.x, -D.y, -D.z), corners p0 = P0, p1 = P0 + E1, p2 = P0 + E2, h the half extent.
 *               per axis, in this order (axis number 0..12):
 *                 0, 1, 2         box face k:  lo = fmin3, hi = fmax3 of (p0[k], p1[k], p2[k]);  r = h[k];  s = V[k]
 *                 3               N = cross(E1, E2):  lo = hi = dot(N, p0);  r = (h.x |N.x| + h.y |N.y|) + h.z |N.z|;  s = dot(N, V)
 *                 4 + 3 g + i     edge f_g in (E1, E2 - E1, E2), box axis i, (j, k) the two axes after i:  proj(p) = p[k] f[j] - p[j] f[k];
 *                                 lo = fmin3, hi = fmax3 of proj(p0), proj(p1), proj(p2);  r = h[j] |f[k]| + h[k] |f[j]|;  s = proj(V)
 *               (fmin3(a, b, c) = fmin(fmin(a, b), c), likewise fmax3: pt_query_overlap's own projections and radii.)
 *               s != 0:  a = (-r - hi) / s;  b = (r - lo) / s;  entry = b < a ? b : a;  exit = b < a ? a : b
 *               s == 0:  entry = +inf, exit = -inf if lo > r or hi < -r (the axis rules the pair out), else entry = -inf, exit = +inf
 *                        (a degenerate axis, lo = hi = r = s = 0, constrains nothing)
 *               te = -inf, axis = 0, tx = +inf; then per axis in order:  if entry > te: te = entry, axis = this one (ties keep the
 *               lowest axis);  if exit < tx: tx = exit.  Every compare is false on a NaN.
 *               candidate iff te <= tx and tx >= 0 and te <= tmax;  t = te > 0 ? te : 0
 *               start overlap   pt_query_overlap_oriented's statement on the same P0, E1, E2 holds: t = 0, feature 13, whatever the
 *                               entry times say.  So t == 0 iff pt_query_overlap_oriented_any's byte for the first sixteen floats,
 *                               for that triangle, bit for bit; with d = 0 the cast is that query.
 *   the answer over all triangles, the smallest time of impact; ties go to the lowest index in the caller's index-buffer order.  The
 *             walk's boxes only prune; the winner is decided by the test above alone.
 *   hits      per cast {t, prim, feature, material | n.xyz, 0 | c.xyz, 0}, evaluated once after the walk on the winner.  feature: the
 *             winning axis as a float, 0..12, or 13 for a start overlap (then n = c = 0).  With sg the s of the winning axis and a the
 *             axis in local coordinates (unit k; N; for 4..12 the vector with a[i] = 0, a[j] = -f[k], a[k] = f[j]):
 *               g = sg > 0 ? a : -a;  W[k] = (g.x m[4 k] + g.y m[4 k + 1]) + g.z m[4 k + 2];  len = sqrt(dot(W, W));
 *               n = len > 0 ? W / len : 0 — the unit normal from the triangle to the box, dot(n, d) <= 0
 *               sc[j] = g[j] > 0 ? -h[j] : h[j] — the box's corner towards the triangle, in local coordinates
 *               0, 1, 2     ext = sg > 0 ? hi : lo of the axis;  c = the first of v0, v0 + e1, v0 + e2 whose projection equals ext
 *               3           cen = c + d * t;  c[k] = cen[k] + ((sc.x m[4 k] + sc.y m[4 k + 1]) + sc.z m[4 k + 2]): the box corner
 *               4 + 3 g + i the triangle's edge (A, E) in ((v0, e1), (v0 + e1, e2 - e1), (v0, e2)), pa = its start p0, p1, p0;
 *                           al = pa + V * t;  dj = sc[j] - al[j];  dk = sc[k] - al[k];  ff = f[j] f[j] + f[k] f[k];
 *                           u = (dj f[j] + dk f[k]) / ff, clamped to [0, 1] (u < 0 ? 0, then u > 1 ? 1), 0 unless ff > 0;  c = A + E * u
 *             (x + y * s for vectors is per component, one multiply and one add.)  A contact that is a segment or a polygon reports
 *             this one representative point.  material: the hit triangle's material id.
 *             A miss is {-1, 0xFFFFFFFF, 0, 0xFFFFFFFF | 0 0 0 0 | 0 0 0 0}.
 *   blocked   pt_query_box_cast_any: one byte per cast, 1 iff hits[i].t >= 0.  A cast's walk ends at its first candidate.
 *   a miss before any traversal: pt_query_overlap_oriented's rules on the first sixteen floats (a non-finite value among the first
 *             fifteen, a negative half extent, axes not orthonormal to 2^-10), a non-finite component of d, a NaN or negative tmax, a
 *             scene without triangles.
 * Not watertight at shared edges, as pt_query_sweep is not.  n == 0 is a no-op success.  Refused, with the context left usable:
 * n > 0x7FFFFFFF, a null pointer, a misaligned casts or hits array, an output that overlaps the casts, a context without a scene.   */
typedef struct { float t; uint32_t prim; float feature; uint32_t material; float nx, ny, nz, pad0; float cx, cy, cz, pad1; } pt_box_cast_hit;   /* 48 bytes */
int pt_query_box_cast(pt_ctx* ctx, const float* casts, size_t n, pt_box_cast_hit* hits);
int pt_query_box_cast_any(pt_ctx* ctx, const float* casts, size_t n, uint8_t* blocked);

/* ---- segment-to-mesh distance on the device (opt-in; nothing above changes) --------------------------------------------------------
 * How far a line segment is from the surface and where the two come closest: the clearance query of motion planning.  A capsule (robot
 * link, cable, tool shaft, limb) clears the mesh by this distance minus its radius, and the closest pair is the direction to push away
 * in; a segment that passes THROUGH a triangle has distance 0, which no sampling of pt_query_nearest along the axis finds.
 * pt_query_nearest's memory and call rules: DEVICE arrays, 16-byte aligned; the call enqueues on the context's stream and returns
 * synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame buffer or pt_stats, walks
 * the node array the scene holds (pt_bvh_info.device_bytes does not change, with pt_query_nearest's one exception) and uses no
 * atomics: two calls give the same bits.  A scene without triangles answers every segment with the miss record.
 *
 *   segments  n records of 8 floats {p0.x, p0.y, p0.z, max_radius | p1.x, p1.y, p1.z, ignored}.  The eighth float is never read into a
 *             decision: a NaN there changes nothing.
 *   out       n records of 32 bytes (pt_segment_hit)
 *   d2        the squared distance from the segment to a triangle, all fp32, every multiply, add and division on its own, evaluated as
 *             written, no fused multiply-add (tests/segment_ref.py is the NumPy statement, equal bit for bit).  With the vectors the
 *             build stores for the triangle, v0, e1 = v1 - v0, e2 = v2 - v0, and d = p1 - p0 (one subtraction per component),
 *             a = dot(d, d), dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, six sub-tests, each giving (d2, s, c): the squared distance,
 *             the parameter on the segment and the point on the triangle.
 *               feature 0   pt_query_nearest's closest_on_triangle at p0, exactly: its d2 and c; s = 0
 *               feature 1   the same at p1 as given in the record (not p0 + d); s = 1
 *               feature 2   segment against the edge {A, E} = {v0, e1}
 *               feature 3   {v0, e2}
 *               feature 4   {fl(v0 + e1), fl(e2 - e1)}, one operation per component
 *               feature 5   the segment crosses the triangle
 *             Features 2 to 4, Ericson, Real-Time Collision Detection 5.1.9, with every case a select:
 *               r = p0 - A;  e = dot(E, E);  b = dot(d, E);  c_ = dot(d, r);  f = dot(E, r);  den = a e - b b
 *               (num1, den1) = (b f - c_ e, den)  if a > 0 and e > 0 and den > 0
 *                              (-c_, a)           if a > 0 and not e > 0
 *                              (0, 1)             otherwise (a segment without length; parallel lines)
 *               s0 = clamp01(num1 / den1);   clamp01(q): q < 0 ? 0 : q, then q > 1 ? 1 : q (a -0 stays, a NaN stays)
 *               tnom = b s0 + f;   lo = e > 0 and tnom < 0;   hi = e > 0 and tnom > e
 *               (num2, den2) = (tnom, e) if e > 0, else (0, 1);  lo: (-c_, a);  hi: (b - c_, a);  (lo or hi) and not a > 0: (0, 1)
 *               q2 = clamp01(num2 / den2);   s = (lo or hi) ? q2 : s0;   t = lo ? 0 : hi ? 1 : q2
 *               p~ = p0 + d s;  c = A + E t (a product, then a sum, per component);  d2 = dot(p~ - c, p~ - c)
 *             Two IEEE divisions per edge; every denominator a select keeps is > 0.
 *             Feature 5, a two-sided Moeller-Trumbore test in plain multiplies and adds, cross(a, b).x = a.y b.z - a.z b.y:
 *               pv = cross(d, e2);  det = dot(e1, pv);  tv = p0 - v0;  U = dot(tv, pv);  qv = cross(tv, e1);  V = dot(d, qv);
 *               T = dot(e2, qv);  det < 0: det, U, V, T change sign
 *               accepted iff det > 0 and U >= 0 and V >= 0 and U + V <= det and 0 <= T <= det;
 *               then d2 = 0 exactly, s = T / det, c = p0 + d s
 *             Among features 0 to 4 the smallest d2 wins, ties to the lower feature; a NaN d2 is no candidate (a feature replaces the
 *             running one iff its d2 is smaller, or the running d2 is a NaN and its own is not).  An accepted crossing overrides them.
 *             Nine divisions per triangle.
 *   candidate a triangle with d2 <= max_radius * max_radius, the product taken in fp32; max_radius = +inf is allowed and its square
 *             is +inf.  A NaN d2 is no candidate.
 *   answer    the candidate with the smallest d2; ties go to the lowest triangle index in the caller's index-buffer order
 *   found     distance = sqrtf(d2) of the winner, one IEEE square root; prim its index; s and feature the winner's, the feature number
 *             stored as a float; (cx, cy, cz) the winner's point c on the triangle (for feature 5 the crossing point p0 + d s);
 *             material the triangle's material id.  The point on the segment is p0 + (p1 - p0) s.
 *   a miss before any traversal: a non-finite coordinate of p0 or p1, a non-finite component of d (finite ends whose difference
 *             overflows), a NaN or negative max_radius, a scene without triangles
 *   miss      {distance -1, prim 0xFFFFFFFF, s 0, feature 0, c (0, 0, 0), material 0xFFFFFFFF}: pt_hit's pattern
 * Not watertight in d2 at shared edges: neighbouring triangles compute a shared edge from their own stored vectors; the smaller d2
 * wins, ties to the lower index.  Products of four lengths (den, the va, vb, vc of features 0 and 1, the crossing test's U, V, T)
 * leave fp32's range when edge length times segment length times the distance between them passes about 1e19 squared; such a
 * sub-test yields a NaN or fails and silently stops being a candidate.
 * n == 0 is a no-op success.  Refused, with the context left usable, in pt_query_nearest's order: a null context, a null segments or
 * out pointer with n > 0, n > 0x7FFFFFFF, an array that is not 16-byte aligned, an output that overlaps the segments, a context
 * without a scene.                                                                                                                     */
typedef struct { float distance; uint32_t prim; float s, feature; float cx, cy, cz; uint32_t material; } pt_segment_hit;   /* 32 bytes */
int pt_query_segments(pt_ctx* ctx, const float* segments, size_t n, pt_segment_hit* out);

/* ---- triangle-to-mesh distance on the device (opt-in; nothing above changes) -------------------------------------------------------
 * How far a triangle is from the surface and where the two come closest: the distance query of PQP and FCL for a mesh that moves
 * through the scene (a robot link, a tool, a character hull), which pt_query_triangles only answers with "intersects: yes / no".
 * pt_query_segments on the moving mesh's edges misses a scene edge that pierces a query face (it reports a positive distance for an
 * intersecting pair) and a scene vertex that is closest to the interior of a query face.
 * pt_query_segments' memory and call rules: DEVICE arrays, 16-byte aligned; the call enqueues on the context's stream and returns
 * synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame buffer or pt_stats, walks
 * the node array the scene holds (pt_bvh_info.device_bytes does not change, with pt_query_nearest's one exception) and uses no
 * atomics: two calls give the same bits.  A scene without triangles answers every query with the miss record.
 *
 *   tris      n records of 12 floats {a0.x, a0.y, a0.z, max_radius | a1.x, a1.y, a1.z, ignored | a2.x, a2.y, a2.z, ignored}:
 *             pt_query_triangles' layout with the radius in the fourth float.  The eighth and twelfth float are never read into a
 *             decision: a NaN there changes nothing.
 *   out       n records of 48 bytes (pt_triangle_distance_hit)
 *   d2        the squared distance from the query triangle to a scene triangle, all fp32, every multiply, add and division on its own,
 *             evaluated as written, no fused multiply-add (tests/tridist_ref.py is the NumPy statement, equal bit for bit).  With the
 *             vectors the build stores for the scene triangle, v0, e1, e2, one operation per component in
 *               f1 = a1 - a0;  f2 = a2 - a0;  g = a2 - a1;  w1 = fl(v0 + e1);  w2 = fl(v0 + e2);  h = fl(e2 - e1)
 *             the query's edges are Q0 = {a0, f1}, Q1 = {a0, f2}, Q2 = {a1, g} and the scene triangle's S0 = {v0, e1}, S1 = {v0, e2},
 *             S2 = {w1, h} (pt_query_segments' own edge order).  Twenty-one sub-tests, each giving (d2, q, c): the squared distance,
 *             the point on the query triangle and the point on the scene triangle.
 *               features 0, 1, 2     pt_query_nearest's closest_on_triangle(a_i; v0, e1, e2), exactly, at a0, a1, a2 as given in the
 *                                    record: its d2 and c; q = a_i
 *               features 3, 4, 5     closest_on_triangle(b_j; a0, f1, f2) for b = (v0, w1, w2): its d2; q its closest point, c = b_j
 *               features 6 + 3 i + j the segment section's edge statement, verbatim, of the segment Q_i = {P, D} with a = dot(D, D)
 *                                    against the edge S_j = {A, E}: its d2; q = P + D s (a product, then a sum, per component), c its
 *                                    point A + E t on the edge
 *               features 15, 16, 17  the segment section's crossing test of Q_i against {v0, e1, e2}; accepted: d2 = 0 exactly,
 *                                    s = T / det, q = c = P + D s
 *               features 18, 19, 20  the same crossing test of S_j against {a0, f1, f2}: q = c = A + E s
 *             Among features 0 to 14 the smallest d2 wins, ties to the lower feature; a NaN d2 is no candidate (a feature replaces the
 *             running one iff its d2 is smaller, or the running d2 is a NaN and its own is not).  An accepted crossing overrides
 *             them; of several accepted crossings the lowest feature number gives the record.  Computing d2 alone costs 24 IEEE
 *             divisions per pair (6 + 18); the crossings' divisions are needed for the winner's record only.
 *   candidate a triangle with d2 <= max_radius * max_radius, the product taken in fp32; max_radius = +inf is allowed and its square
 *             is +inf.  A NaN d2 is no candidate.
 *   answer    the candidate with the smallest d2; ties go to the lowest triangle index in the caller's index-buffer order
 *   found     distance = sqrtf(d2) of the winner, one IEEE square root; prim its index; feature the winner's, the number stored as a
 *             float; material the scene triangle's material id; (qx, qy, qz) the point on the query triangle and (cx, cy, cz) the
 *             point on the scene triangle: c - q is the direction to push the query away from the scene along, and for a crossing
 *             both are the crossing point
 *   a miss before any traversal: a non-finite one of the nine coordinates, a non-finite component of a1 - a0, a2 - a0 or a2 - a1
 *             (finite vertices whose difference overflows), a NaN or negative max_radius, a scene without triangles
 *   miss      {distance -1, prim 0xFFFFFFFF, feature 0, material 0xFFFFFFFF | 0, 0, 0, 0 | 0, 0, 0, 0}
 *   pad0, pad1 are written as 0 in every record.
 * A query without area (a2 == a1: a segment; three equal vertices: a point) is a query like any other: its vertex and edge features
 * answer, and its distance is at most pt_query_segments' and pt_query_nearest's on the same input.
 * Not watertight in d2 at shared edges: neighbouring triangles compute a shared edge from their own stored vectors; the smaller d2
 * wins, ties to the lower index.  Products of four lengths (den of the edge statement, the va, vb, vc of features 0 to 5, the
 * crossing tests' U, V, T) leave fp32's range when edge length times edge length times the distance between them passes about 1e19
 * squared; such a sub-test yields a NaN or fails and silently stops being a candidate.
 * n == 0 is a no-op success.  Refused, with the context left usable, in pt_query_segments' order and with messages that start
 * "pt_query_triangle_distance: ": a null context, a null tris or out pointer with n > 0, n > 0x7FFFFFFF ("too many triangles"), an
 * array that is not 16-byte aligned, an output that overlaps the triangles, a context without a scene.                              */
typedef struct { float distance; uint32_t prim; float feature; uint32_t material;
                 float qx, qy, qz, pad0;  float cx, cy, cz, pad1; } pt_triangle_distance_hit;   /* 48 bytes */
int pt_query_triangle_distance(pt_ctx* ctx, const float* tris, size_t n, pt_triangle_distance_hit* out);

/* ---- posed-mesh queries on the device (opt-in; nothing above changes) --------------------------------------------------------------
 * The per-pose part of "a mesh that moves through the scene, tested in many poses": the mesh is registered once, P poses go in, one
 * byte or one closest pair per pose comes out.  The P x T posed records and the P x T per-triangle answers that
 * pt_query_triangles_any / pt_query_triangle_distance would need are never materialised, a pose that is decided stops costing walks,
 * and a C caller needs no loop of its own.
 *
 * pt_set_query_mesh   tris: a HOST pointer to ntris records of 12 floats in pt_query_triangles' layout {a0.xyz, . | a1.xyz, . |
 *             a2.xyz, .}, in the mesh's own frame; the fourth floats are ignored.  The records are copied into device memory the
 *             context owns.  The mesh is independent of the scene: it survives pt_set_scene, pt_update_vertices and
 *             pt_update_materials.  A second call replaces it; ntris == 0 frees it.  ntris <= PT_QUERY_MESH_MAX (2^20).  Its memory
 *             is not part of pt_bvh_info.device_bytes; pt_get_query_mesh reports the mesh (either output may be null).  Refused: a
 *             null context, a null tris with ntris > 0, ntris above the limit ("too many triangles").
 *
 *   pose      12 floats, a row-major 3 x 4 matrix m.  The posed vertex of (x, y, z) is
 *               x' = ((m[0] * x + m[1] * y) + m[2]  * z) + m[3]
 *               y' = ((m[4] * x + m[5] * y) + m[6]  * z) + m[7]
 *               z' = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
 *             all fp32, every multiply and add on its own in exactly that order, no fused multiply-add (tests/poses_ref.py is the
 *             NumPy statement, equal bit for bit).  Any matrix is allowed: scale, shear, mirror, singular.  This statement is what
 *             makes every answer below bit-defined: the posed triangle (p, t) is these nine numbers, wherever they are formed.
 *   poses     P poses; DEVICE, 16-byte aligned.
 *
 * pt_pose_triangles   writes the P x T posed records, pose-major (record p * T + t), in pt_query_triangles' layout with the three
 *             fourth floats 0: what pt_query_triangles_lists and the other per-triangle queries take.  tris_out: DEVICE, 16-byte
 *             aligned, P * T records of 48 bytes.
 *
 * pt_query_poses_any  hit[p] = 1 iff pt_query_triangles_any answers 1 for at least one posed triangle of pose p, else 0.  first is
 *             optional: first[p] = the lowest mesh triangle index for which pt_query_triangles_any answers 1, 0xFFFFFFFF where there
 *             is none.  hit: DEVICE, P bytes; first: DEVICE, 4-byte aligned, P words, or null.
 *
 * pt_query_poses_distance   out[p]: the closest pair of pose p within max_radius.  A mesh triangle is a candidate of its pose iff
 *             pt_query_triangle_distance finds something for its posed triangle with that max_radius (d2 <= max_radius^2 as that
 *             section decides it).  The winner is the candidate with the smallest SQUARED distance — that section's d2 of the
 *             record's pair, before the square root —, ties to the lowest mesh triangle index.  (This is d2, not the rounded
 *             distance: an argmin over the sqrtf'd distances can differ where two d2 round to one distance.)  The record is, bit for
 *             bit, pt_query_triangle_distance's record for that one posed triangle with that radius, with query_triangle = the mesh
 *             triangle's index in the place of pad0.  A pose without a candidate gets the miss record {distance -1, prim 0xFFFFFFFF,
 *             feature 0, material 0xFFFFFFFF | 0, 0, 0, query_triangle 0xFFFFFFFF | 0, 0, 0, 0}.  A non-finite pose entry, and a
 *             transform that overflows, make posed triangles "a miss before any traversal" by the rules above, for both queries; a
 *             NaN or negative max_radius makes every pose a miss (it is not refused).  out: DEVICE, 16-byte aligned, P records.
 *
 * The calls enqueue on the context's stream and return synchronised, act on rank 0 of a pt_create_multi context, never write the
 * accumulation buffer, the frame buffer or pt_stats, and keep one 8-byte word per pose of scratch in the context (not counted in
 * device_bytes).  Inside, lanes of different workgroups meet in that word through order-independent atomic minima only and never wait
 * for one another: two calls give the same bits.
 * P == 0 is a no-op success.  Refused, with the context left usable, in this order and with messages that start "<entry point>: ": a
 * null context; a null required argument; P > 0x7FFFFFFF ("too many poses"); P * T > 0x7FFFFFFF ("too many posed triangles (2^31 - 1
 * per call): split the poses"); a poses, tris_out or out array that is not 16-byte aligned, a first that is not 4-byte aligned; any
 * two of the arrays overlapping; no query mesh ("pt_set_query_mesh first"); a context without a scene.                             */
#define PT_QUERY_MESH_MAX 1048576u
typedef struct { float distance; uint32_t prim; float feature; uint32_t material;
                 float qx, qy, qz; uint32_t query_triangle;  float cx, cy, cz, pad1; } pt_pose_distance_hit;   /* 48 bytes */
int pt_set_query_mesh(pt_ctx* ctx, const float* tris, size_t ntris);
int pt_get_query_mesh(pt_ctx* ctx, size_t* ntris, size_t* device_bytes);
int pt_pose_triangles(pt_ctx* ctx, const float* poses, size_t P, float* tris_out);
int pt_query_poses_any(pt_ctx* ctx, const float* poses, size_t P, uint8_t* hit, uint32_t* first);
int pt_query_poses_distance(pt_ctx* ctx, const float* poses, size_t P, float max_radius, pt_pose_distance_hit* out);

/* ---- translating-mesh casts: time of impact of a moving triangle or posed mesh (opt-in; nothing above changes) -------------------
 * The queries above that take a mesh of the caller's are discrete: does it intersect in this pose, how far away is it in this pose.
 * Sampled along a motion they tunnel through a thin wall between two free poses.  These are the shape cast for a shape that is a mesh:
 * how far can this triangle, or this whole posed mesh, translate along d before it first touches the scene, and where.
 *
 *   casts     n records of 16 floats {a0.xyz, tmax | a1.xyz, . | a2.xyz, . | d.xyz, .}; DEVICE, 16-byte aligned.  The dotted floats
 *             are never read into a decision.  The triangle occupies a_i + t d for 0 <= t <= tmax, closed at both ends; d is not
 *             normalised (t is in units of |d|); tmax = +inf is allowed and stands for the largest finite t.
 *   hits      n records of 32 bytes; DEVICE, 16-byte aligned.  blocked: n bytes, DEVICE, any alignment.
 *   motions   pt_query_poses_cast: P records {d.xyz, tmax} in the WORLD frame, applied after the pose's transform; DEVICE, 16-byte
 *             aligned.
 *
 * The time of impact of one pair.  All arithmetic is fp32, every operation on its own, no fused multiply-add, IEEE division, on the
 * stored v0, e1, e2 of the scene triangle, with dot and cross as written under pt_query_closest (tests/tricast_ref.py is the NumPy
 * statement, equal bit for bit).  f1 = a1 - a0, f2 = a2 - a0, g = a2 - a1; w1 = v0 + e1, w2 = v0 + e2, h = e2 - e1; the query's edges
 * Q0 = {a0, f1}, Q1 = {a0, f2}, Q2 = {a1, g}, the scene triangle's S0 = {v0, e1}, S1 = {v0, e2}, S2 = {w1, h}; qlo, qhi and slo, shi
 * the fmin3 / fmax3 boxes of the query's and of the scene triangle's three corners (a0, a1, a2 and v0, w1, w2).
 *
 *   ray(o, r; p, k1, k2)   pv = cross(r, k2); det = dot(k1, pv); tv = o - p; U = dot(tv, pv); qv = cross(tv, k1); V = dot(r, qv);
 *                          T = dot(k2, qv); where det < 0: det, U, V, T change sign.
 *                          accepted iff det > 0, U >= 0, V >= 0, U + V <= det, T >= 0;  t = T / det + 0  (the + 0 turns a -0 into +0)
 *   features 0, 1, 2       ray(a_i, d; v0, e1, e2);  c = a_i + d t;  guard: c inside [slo - eps, shi + eps]
 *   features 3, 4, 5       ray(b_j, -d; a0, f1, f2) with b = (v0, w1, w2);  c = b_j;  guard: b_j - d t inside [qlo - eps, qhi + eps]
 *   features 6 + 3 i + j   Q_i = {P, D} against S_j = {A, E}:  n = cross(D, E); det = dot(d, n); w = A - P; T = dot(w, n);
 *                          S = dot(d, cross(w, E)); G = dot(d, cross(w, D)); where det < 0: det, T, S, G change sign.
 *                          accepted iff det > 0, 0 <= S <= det, 0 <= G <= det, T >= 0;  t = T / det + 0;  c = A + E (G / det)
 *                          guard: c - d t inside [qlo - eps, qhi + eps]
 *   feature 15             the 20 conditions of pt_query_triangles hold at t = 0 (start overlap): t = 0, c = (0, 0, 0); it overrides
 *                          the others
 *   eps = 2^-16 * (largest |component| of v0, w1, w2  +  largest |component| of a0, a1, a2);  "inside" is six closed compares, each
 *   bound one fp32 subtraction or addition.
 *
 * A feature is a candidate iff it is accepted, its guard holds and t <= tmax; every compare is false on a NaN, and t = +inf is no
 * candidate.  Within a pair the smallest t wins, ties to the lower feature; over the scene the smallest t wins, ties to the lowest
 * triangle index in the caller's order.  The guards tie every candidate's contact to both triangles' boxes within eps, whatever the
 * angle: a near-singular det makes t noise, and a contact that noise has carried off both boxes is no contact.
 * The record: t; prim; feature (the winning feature's number as a float); query_triangle (0 in the per-triangle calls); the contact
 * c in world space (for features 0..2 the query's corner at t, for 3..5 the scene triangle's corner, for 6..14 the point of the scene
 * edge; zero for a start overlap); material.  A miss is {-1, 0xFFFFFFFF, 0, 0 | 0, 0, 0, 0xFFFFFFFF}.  A miss before any traversal: a
 * non-finite coordinate of the query or of d; a non-finite f1, f2 or g; a NaN or negative tmax; a scene without triangles.
 * blocked[i] = 1 iff hits[i].t >= 0; its walk leaves at the first candidate.  With d = 0 only feature 15 can answer.
 * Not seen: a triangle that slides exactly within a scene triangle's plane has every det = 0, so such a motion is reported only as a
 * start overlap (in-plane sliding contacts are out of scope); likewise an edge sliding along a parallel edge.  Products of four
 * lengths leave fp32's range as under pt_query_triangle_distance; such a feature silently stops being a candidate.
 *
 * pt_query_poses_cast   out[p] is, bit for bit, pt_query_triangle_cast's record for one posed triangle of pt_pose_triangles with
 *             {tmax, d} = motions[p]: the one with the smallest t, ties to the lowest mesh triangle index, which is stored in
 *             query_triangle.  A pose without a candidate gets the miss record with query_triangle 0xFFFFFFFF.  A non-finite motion,
 *             like a non-finite pose entry, makes the pose a miss.
 *
 * Memory and call rules are pt_query_triangle_distance's (per triangle) and pt_query_poses_distance's (posed): the calls enqueue on the
 * context's stream and return synchronised, act on rank 0 of a pt_create_multi context, never write the accumulation buffer, the frame
 * buffer or pt_stats, and leave device_bytes unchanged.  The per-triangle calls use no atomics; the posed call uses the 8-byte word per
 * pose with order-independent minima only.  Two calls give the same bits.  n == 0 and P == 0 are no-op successes.  Refused, with the
 * context left usable, in the siblings' order and with messages that start "<entry point>: ": a null context; a null argument;
 * n > 0x7FFFFFFF ("too many casts") or the posed calls' two limits; an array that is not 16-byte aligned; arrays that overlap; no
 * query mesh (posed); a context without a scene.                                                                                  */
typedef struct { float t; uint32_t prim; float feature; uint32_t query_triangle;
                 float cx, cy, cz; uint32_t material; } pt_triangle_cast_hit;   /* 32 bytes */
int pt_query_triangle_cast(pt_ctx* ctx, const float* casts, size_t n, pt_triangle_cast_hit* hits);
int pt_query_triangle_cast_any(pt_ctx* ctx, const float* casts, size_t n, uint8_t* blocked);
int pt_query_poses_cast(pt_ctx* ctx, const float* poses, const float* motions, size_t P, pt_triangle_cast_hit* out);

/* ---- the K closest triangles of a point, and "is anything within r" (opt-in; nothing above changes) ------------------------------
 * pt_query_nearest answers with one triangle.  A ball resting in a corner touches three walls and needs all three contacts; a point
 * whose closest feature is an edge or a vertex ties between two to six triangles, of which pt_query_nearest names the lowest index
 * only — and the triangles at the winning feature are what a pseudonormal sign, a contact manifold or a blend over the nearest
 * surfaces needs.  pt_query_nearest_k lists the first max_k candidates in order and counts them all (the sphere form of
 * pt_query_overlap's count); pt_query_within_any answers the clearance check "is anything within r of this point" with one byte,
 * leaving at the first candidate instead of searching for the closest.  pt_query_nearest's memory and call rules: DEVICE arrays,
 * points and out 16-byte aligned, counts 4-byte, hit any alignment; the call enqueues on the context's stream and returns
 * synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame buffer or pt_stats,
 * walks the node array the scene holds (pt_bvh_info.device_bytes does not change, with pt_query_nearest's one exception) and uses no
 * atomics: two calls give the same bits.
 *
 *   points    pt_query_nearest's: n records of 4 floats {x, y, z, max_radius}
 *   d2        pt_query_nearest's, word for word: the closest_on_triangle statement above in plain fp32, one IEEE division per
 *             triangle, no fused multiply-add
 *   candidate pt_query_nearest's: a triangle with d2 <= max_radius * max_radius, the product taken in fp32 (+inf squared is +inf); a
 *             NaN d2 is no candidate.  Each triangle is a candidate at most once.
 *   a miss before any traversal: pt_query_nearest's — a non-finite coordinate, a NaN or negative max_radius, a scene without triangles
 *   out       null with max_k == 0, or n * max_k records (1 <= max_k <= PT_QUERY_NEAREST_MAX), point-major: record j of point i is
 *             out[i * max_k + j], its j-th candidate in ascending (d2, prim): d2 compared as floats, equal d2 to the lower triangle
 *             index.  Each is pt_query_nearest's full 32-byte record (distance = sqrtf(d2), prim, the weights, the point c, the
 *             material), computed once from the kept triangle by the same statement; the slots past the point's last candidate hold
 *             the miss record.  Record 0 equals pt_query_nearest's on the same point, bit for bit.
 *   counts    null, or n words: the number of candidates of point i, not clamped to max_k.  0 for a miss before any traversal.
 *             max_radius = +inf with counts is legal: it counts every triangle whose d2 is not a NaN, and walks the whole tree.
 *   the walk  with counts nothing can be pruned at a candidate: the walk is cut at max_radius only and costs what the ball holds.
 *             Without counts it is also cut at the d2 of entry max_k - 1 once that entry is filled (widened as pt_query_nearest's
 *             cut is, and closed, so that a triangle that ties with the last kept entry and has a lower index is still reached).
 *             The records are the same either way.
 *   hit       (pt_query_within_any) one byte per point: 1 iff counts[i] would be non-zero, else 0.  The point's walk ends at its
 *             first candidate.
 * n == 0 is a no-op success.  Refused, with the context left usable, in pt_query_nearest's order with pt_query_multi's additions: a
 * null context, max_k > PT_QUERY_NEAREST_MAX, out null with max_k != 0 or the reverse, out and counts both null, a null points (or
 * hit) pointer with n > 0, n > 0x7FFFFFFF, a misaligned points, out or counts pointer, an output that overlaps the points or the
 * other output, a context without a scene.                                                                                           */
#define PT_QUERY_NEAREST_MAX 8
int pt_query_nearest_k(pt_ctx* ctx, const float* points, size_t n, uint32_t max_k, pt_nearest* out, uint32_t* counts);
int pt_query_within_any(pt_ctx* ctx, const float* points, size_t n, uint8_t* hit);

/* ---- generalised winding numbers (opt-in; nothing above changes) -------------------------------------------------------------------
 * Whether a point is inside the mesh, for meshes that are not watertight: w(q) = (1 / 4 pi) sum_t Omega_t(q), the signed solid angle
 * the mesh subtends at q (Jacobson et al. 2013; Barill et al. 2018).  A closed, outward-wound mesh gives 1 inside and 0 outside; a
 * hole of solid angle omega lowers the inside value by omega / 4 pi, so w > 0.5 stays a usable inside test where crossing parity
 * (pt_query_multi's counts) is wrong for every ray that leaves through the hole.  pt_query_nearest's memory and call rules: DEVICE
 * arrays, points 16-byte aligned, out 4-byte aligned; the call enqueues on the context's stream and returns synchronised, acts on
 * rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame buffer or pt_stats and uses no atomics in the
 * walk: two calls give the same bits.
 *
 *   points    pt_query_nearest's layout: n records of 4 floats {x, y, z, unused}; the fourth float is ignored
 *   out       n floats: out[i] = w(q_i).  A triangle is what the scene's record holds, as for pt_query_nearest: v0, e1 = v1 - v0 and
 *             e2 = v2 - v0 in fp32, its vertices v0, v0 + e1, v0 + e2.  With a, b, c the triangle's vertices minus q,
 *               Omega_t = 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|).
 *             A point with a non-finite coordinate gets a NaN without traversal; a scene without triangles answers 0; on the surface
 *             itself the value is unspecified but finite.
 *   beta      the accuracy knob.  Every inner node carries the first-order moments of its subtree: p, the area-weighted centroid
 *             of its triangles; r2, the squared distance from p to the farthest corner of the exact box of its vertices; N, the sum
 *             of the triangles' area-weighted normals.  A node's whole subtree is replaced by its dipole iff d2 > beta2 * r2, evaluated
 *             in fp32 exactly as written: beta2 = beta * beta computed in float on the host, dx = px - qx (likewise y, z),
 *             d2 = (dx * dx + dy * dy) + dz * dz, no contraction.  The dipole contributes N . (p - q) / (d2 * sqrt(d2)) in units of
 *             Omega.  The test is made for the root first, then for every inner child before it is entered; leaves are always exact
 *             solid angles.  beta = +inf is legal and is the exact sum over every triangle (inf * 0 is a NaN and the comparison is
 *             false).  PT_WINDING_BETA_DEFAULT is the paper's value: on an icosphere of 320 triangles, first order at beta = 2 is off
 *             by at most 0.024.
 *   moments   fp32, per triangle from its record {v0, e1, e2}: n2 = e1 x e2, N_t = 0.5 n2, A_t = 0.5 sqrt(n2 . n2), centroid
 *             c_t = v0 + (e1 + e2) / 3, S_t = A_t c_t.  Per node, child 0 then child 1: N = N0 + N1, A = A0 + A1, S = S0 + S1; lo and
 *             hi the exact min and max of the vertices below it (v0, v0 + e1, v0 + e2, without the builder's pad).  p = S / A (IEEE
 *             division; the box centre 0.5 (lo + hi) where A is 0), r2 = sum over the axes of max(p - lo, hi - p)^2.  The two-child
 *             order makes every sum deterministic whatever the schedule.  csrc/winding.h; tests/winding_ref.py restates it.
 *   lifetime  the moments (96 bytes per node: the 32-byte records and the 64-byte records the walk reads) are built on the first
 *             pt_query_winding after pt_set_scene or pt_update_vertices, kept across calls and across pt_update_materials and freed
 *             with the scene.  They do NOT count in pt_bvh_info.device_bytes; pt_get_winding_info reports them.  A failed build
 *             leaves the context usable and nothing half-built.
 * n == 0 is a no-op success.  Refused, with the context left usable, in pt_query_nearest's order: a null context, beta < 1 or NaN, a
 * null points or out pointer with n > 0, n > 0x7FFFFFFF, a misaligned pointer, an out that overlaps the points, a context without a
 * scene.                                                                                                                            */
#define PT_WINDING_BETA_DEFAULT 2.0f
typedef struct pt_winding_info {
    uint32_t built;      /* 1 while the moments are on the device */
    uint32_t n_nodes;    /* nodes they cover (0 while not built) */
    uint64_t bytes;      /* device memory they hold (0 while not built) */
} pt_winding_info;
int pt_query_winding(pt_ctx* ctx, const float* points, size_t n, float beta, float* out);
int pt_get_winding_info(pt_ctx* ctx, pt_winding_info* out);

/* ---- ambient occlusion traced on the device (opt-in; nothing above changes) -----------------------------------------------------
 * The share of the hemisphere over a surface point that is open within `radius`: K rays per point, generated, traced with
 * pt_query_any's walk and counted inside one kernel, so no ray reaches memory.  pt_ao_points takes the points from a device array
 * (baking: vertices, texels, probes), pt_ao_image from pt_render_features' second output (an AO pass of the current view).  Both
 * enqueue on the context's stream and return synchronised, act on rank 0 of a pt_create_multi context, never write the accumulation
 * buffer, the frame buffer or pt_stats, and walk the node array the scene holds exactly as pt_query_any does
 * (pt_bvh_info.device_bytes does not change, with pt_query_any's exception: a variant forced onto a format the queries do not walk gets
 * the fp32 nodes on the first call).  No atomics: two calls give the same bits.  On a scene without triangles (pt_set_scene with
 * n_tris = 0) no ray is occluded: visible counts every sample, ao is samples / total_samples.
 *
 *   points        DEVICE, 16-byte aligned, n records of two float4: {P.xyz, unused} {N.xyz, unused}.  N is a unit normal as the caller
 *                 has it; it is not renormalised.
 *   normal_depth  DEVICE, float4[w*h]: pt_render_features' second output for the view in params, of which the call reads width, height
 *                 and the camera, nothing else.  n = w * h, the point of pixel p = y * w + x is P = eye + t * dir per component (one
 *                 multiply, one add), dir the direction pt_render_features traced (the same expression: the same bits),
 *                 t = normal_depth.w, N = normal_depth.xyz.
 *   disk          HOST, K pairs (x, y) with x * x + y * y <= 1 in fp32: the sample pattern, the caller's.  The library copies it into a
 *                 small buffer the context keeps (pt_destroy frees it).
 *   visible       DEVICE uint32[n], 4-byte aligned: the rays that found nothing, 0..K per call
 *   ao            DEVICE float[n], 4-byte aligned, or NULL: visible / total_samples
 *
 * Per point i, all fp32, evaluated left to right as written, no fused multiply-add (tests/ao_ref.py is the NumPy statement, equal bit
 * for bit):
 *   no surface  a non-finite component of P or N, N = (0, 0, 0), or (image form) normal_depth.w < 0: count = K, nothing is traced
 *   hash        h = tea4(i, seed)  (four rounds of TEA over (i, seed), the first word; the renderer's own seed function)
 *   rotation    a = float(h & 0xFFFF) * 2^-16;  a2 = a * a;  den = 1 + a2;  c = (1 - a2) / den;  s = (a + a) / den;  then
 *               q = (h >> 16) & 3 quarter turns, exactly: q = 1: (c, s) <- (-s, c);  q = 2: (-c, -s);  q = 3: (s, -c)
 *   frame       sg = copysignf(1, N.z);  A = -1 / (sg + N.z);  B = N.x * N.y * A;                             (Duff et al. 2017)
 *               T = (1 + sg * N.x * N.x * A, sg * B, -sg * N.x);  S = (B, sg + N.y * N.y * A, -N.y)
 *   origin      o = P + bias * N per component
 *   ray k       x' = c * x_k - s * y_k;  y' = s * x_k + c * y_k;  z = sqrtf(fmaxf(0, (1 - x' * x') - y' * y'));
 *               d = (x' * T + y' * S) + z * N per component;  the ray {o, d, tmin 0, tmax radius} under pt_query_any's rules, its miss
 *               before any traversal included;  count += not occluded
 *   outputs     visible[i] = count, or visible[i] += count when accumulate is set;  ao[i] = float(visible[i]) / float(total_samples),
 *               one IEEE division, of the value just stored
 * A progressive caller passes accumulate = 1, its call index as seed and its running sum of samples as total_samples.
 * n == 0 (or an empty image) is a no-op success.  Refused, with the context left usable: a null context, params, input, disk, ao
 * parameters or visible; an input that is not 16-byte or an output that is not 4-byte aligned; n > 0x7FFFFFFF; samples outside
 * 1..256; a radius that is not positive and finite; a bias that is negative or not finite; total_samples < samples; a non-zero reserved
 * field; a disk point outside the unit disk or not finite; an output that overlaps the input or the other output; a context without
 * a scene.                                                                                                                          */
typedef struct { uint32_t samples;        /* K: rays per point in this call, 1..256 */
                 float    radius;         /* reach of a ray, > 0, finite */
                 float    bias;           /* origin offset along the normal, >= 0, finite */
                 uint32_t seed;           /* second word of the per-point hash; a progressive caller passes its call index */
                 uint32_t accumulate;     /* 0: visible[i] = count;  non-zero: visible[i] += count */
                 uint32_t total_samples;  /* divisor of `ao`: the caller's running sum of `samples`, this call included; >= samples */
                 uint32_t reserved[2];    /* must be 0 */ } pt_ao_params;   /* 32 bytes */
int pt_ao_points(pt_ctx* ctx, const float* points, size_t n, const float* disk, const pt_ao_params* ao_params, uint32_t* visible, float* ao);
int pt_ao_image(pt_ctx* ctx, const pt_params* params, const float* normal_depth, const float* disk, const pt_ao_params* ao_params, uint32_t* visible, float* ao);

/* ---- denoised preview (opt-in; nothing above changes) -------------------------------------------------------------------------
 * Both calls enqueue on the context's stream and return synchronised, cover the whole image (pt_set_partition does not apply), act
 * on rank 0 of a pt_create_multi context, and never write the accumulation buffer, the frame buffer or pt_stats.  A caller of the
 * reference's loop calls them after LaunchCurrentFrame and before display.
 *
 * pt_render_features: one camera ray per pixel through the pixel centre, the camera of pathTracerPrograms.cu:730-740 with the jitter at
 * 0.5 and IEEE fp32 whatever pt_set_math_mode says: d = 2 * ((x + 0.5) / w, (y + 0.5) / h) - 1, dir = normalize(d.x U + d.y V + W) as
 * 1 / sqrtf(dot) left to right, origin cameraEye, interval (0.01, 1e16), row 0 at the bottom.  Reads width, height and the camera of
 * params, nothing else.  DEVICE outputs, float4[w*h] each:
 *   albedo_prim   .xyz the first hit's pt_material.diffuse (any bsdfType), .w the hit triangle's index in the caller's index-buffer order
 *                 as uint32 bits; a miss: (0, 0, 0, 0xFFFFFFFF bits)
 *   normal_depth  .xyz the unit geometric normal normalize(cross(e1, e2)), negated if it faces away from the ray; .w the hit distance t;
 *                 a miss: (0, 0, 0, -1)
 * Hit triangle and t equal pt_trace_closest's on the same rays bit for bit.  The rays walk the node array the scene holds
 * (pt_bvh_info.device_bytes does not change), except under a variant forced onto another format by pt_set_tuning, which brings the
 * fp32 nodes back as a ray query does.  Fails without a scene.
 *
 * pt_denoise: edge-avoiding a-trous filter (Dammertz et al. 2010) with the variance-driven luminance edge-stop of SVGF (Schied et al.
 * 2017), no temporal part of its own (pt_temporal_blend below is that).  Reads params->accumulationBuffer (linear radiance, float4[w*h]), width, height and the two feature buffers;
 * writes linear float4 {r, g, b, 1} to out_rgba (device; pt_resolve_framebuffer makes colours of it).  iterations in [1, 8]; 5 reaches
 * 2 * (1 + 2 + 4 + 8 + 16) = 62 pixels.  out_rgba must not overlap an input.  All arithmetic fp32 in the order written here
 * (tests/denoise_ref.py is the NumPy statement of the same thing):
 *   hit_p    normal_depth_p.w >= 0
 *   a_p      max(albedo_p, 0.01) per channel on a hit, 1 on a miss;  c_p = rgb_p / a_p;  l(c) = 0.2126 c.r + 0.7152 c.g + 0.0722 c.b
 *   geometry between p and a tap q at step s: no weight (the tap is skipped) if exactly one of them misses; if both miss w_n = 1 and
 *            z = 0; if both hit z = |t_p - t_q| / (sigma_z * s * t_p) and w_n = max(0, n_p . n_q)^sigma_n (seven squarings)
 *   variance pre-pass (s = 1, 5x5 taps inside the image): w = w_n * exp(-z); M1, M2 = sum w (l_q - l_p), sum w (l_q - l_p)^2 over sum w;
 *            var_p = max(0, M2 - M1^2) — the variance of l about l_p, i.e. the M2 - M1^2 of l without its cancellation
 *   iteration i = 0 .. iterations-1, s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2 (dy outer), taps outside the image skipped:
 *            g_p = 3x3 {1/4, 1/2, 1/4}^2 blur of var at distance 1, renormalised at the borders
 *            k = h[dx] h[dy] * w_n * exp(-(z + |l_p - l_q| / (sigma_l * sqrt(g_p) + 1e-6))),  h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *            (w_z * w_l in one exponential); c' = sum k c_q / sum k;  var' = sum k^2 var_q / (sum k)^2
 *   output   c' * a_p after the last iteration, alpha 1
 *   sigma_z = 0.01, sigma_n = 128, sigma_l = 5: the best of a sweep (sigma_z 0.002 ... 1, sigma_l 1 ... 16) on the CPU oracle's Cornell
 *   box at 128 x 128, 8 samples per pixel against 8192 (tests/test_denoise_host.py): the MSE falls 7.0-fold.
 *   invalid inputs (comparisons and selects only: where no rule fires, the arithmetic above is untouched and so are its bits):
 *            a source pixel is UNUSABLE if a channel of c_p is not finite or |l(c_p)| > 2^60 (a NaN l included; below 2^60 the
 *            squares and their sums stay finite).  An unusable pixel is skipped as a tap q in the variance pre-pass, in every iteration
 *            and in the 3x3 blur of var, and its own output is its accumulation rgb as bits, alpha 1.
 *            If sigma_z * s * t_p is zero or not finite, z = 0 for taps with t_q == t_p and every other tap is skipped.
 *            max(0, n_p . n_q) and max(0, M2 - M1^2) are fmaxf: 0 for a NaN.  max(albedo_p, 0.01) likewise: 0.01 for a NaN albedo.
 *            If after a pass the sum of weights is not > 0, or c' or var' is not finite, the pixel keeps c_p and var_p for that pass
 *            (the pre-pass: var_p = 0): a zero, NaN or short normal, or a sum that left fp32.
 *            normal_depth.w NaN is a miss (not >= 0); +0 and -0 are hits.
 *            So, with a finite albedo: every output pixel is finite unless its own accumulation pixel is not, and a pixel farther than
 *            2 * (2^iterations - 1) + 2 from every invalid pixel has the bits it has without them.
 * The context keeps two float4[w*h] scratch buffers ({c, var}, ping-pong; var = -1 marks an unusable pixel), grown on demand and freed
 * by pt_destroy.  No atomics: two calls give the same bits, and so do the two math modes.                                          */
int pt_render_features(pt_ctx* ctx, const pt_params* params, float* albedo_prim, float* normal_depth);
int pt_denoise(pt_ctx* ctx, const pt_params* params, const float* albedo_prim, const float* normal_depth, float* out_rgba, uint32_t iterations);

/* ---- temporal reprojection (opt-in; nothing above changes) --------------------------------------------------------------------
 * pt_temporal_blend carries an accumulated image across a camera move: the history of the previous view is reprojected into the
 * current one, each reprojected sample is checked for consistency, and what passes is blended with the fresh accumulation by sample
 * count — the temporal half of SVGF (Schied et al. 2017) that pt_denoise lacks.  Enqueues on the context's stream and returns
 * synchronised, covers the whole image, acts on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame
 * buffer or pt_stats.  All buffers DEVICE, float4 per pixel, row 0 at the bottom:
 *   params          the current view: camera, width, height and accumulationBuffer (linear rgb; .w is not read); nothing else is read
 *   accum_samples   N >= 1, the samples the accumulation stands for (currentFrameIdx * samplesPerPixel for the reference's loop)
 *   albedo_prim, normal_depth   pt_render_features of the current view
 *   prev            the previous view: camera, width w' and height h' (any size); nothing else is read
 *   prev_history    float4[w'*h'] {linear rgb, the samples it stands for}: a former out_history, or an accumulation as {rgb, N}
 *   prev_albedo_prim, prev_normal_depth   pt_render_features of the previous view
 *   history_cap     the most samples the history may count for (finite, >= 0; 0: the output is exactly {accum.rgb, N})
 *   out_history     float4[w*h] {rgb, samples}: the input of the next call; must not overlap an input (chained calls ping-pong two)
 * prev, prev_history, prev_albedo_prim and prev_normal_depth may be NULL together: no history.  All arithmetic fp32 in the order
 * written here (tests/temporal_ref.py is the NumPy statement of the same thing):
 *   c = accum_p.rgb;  the pass-through is out = {c, N}, taken on a miss (normal_depth_p.w < 0, or not >= 0), without a history, where
 *            the hit triangle's bsdfType is not PT_BSDF_DIFFUSE (metal and glass are view-dependent; a Lambertian hit is not, in light
 *            mode 0 or 1), and wherever a step below says so
 *   ray      dir_p exactly as pt_render_features traces it (same expression, same order: the same bits), t_p = normal_depth_p.w;
 *            v = (eye + t_p * dir_p) - eye'
 *   project  s = dot(v, W') / dot(W', W'), dot = x*x' + y*y' + z*z' left to right; s > 0 or the pass-through;
 *            du = dot(v, U') / (s * dot(U', U')), dv = dot(v, V') / (s * dot(V', V'))  (the UVW frame taken as orthogonal);
 *            fx = (du + 1) * 0.5 * w' - 0.5, fy = (dv + 1) * 0.5 * h' - 0.5  (the inverse of the pixel-centre mapping);
 *            fx in [-1, w') and fy in [-1, h') or the pass-through
 *   taps     x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0; taps (x0 + tx, y0 + ty), ty outer, tx inner, in {0, 1},
 *            w_q = (tx ? ax : 1 - ax) * (ty ? ay : 1 - ay).  A tap is accepted if it lies inside the previous image, its
 *            prev_albedo_prim.w bits equal the pixel's triangle, and dot(prev_normal_q, normal_p) > 0 (the same side of the same plane:
 *            both normals face their camera, so a camera that crossed the plane is rejected)
 *   sums     over the accepted taps, in tap order: a = sum w_q, (r, g, b) = sum w_q * hist_q.rgb, m = sum w_q * hist_q.w
 *   count    n = (m < cap) ? m : cap — a times the accepted taps' mean count, so a partly accepted footprint counts for less;
 *            a > 0 and n > 0, or the pass-through
 *   blend    h = (r, g, b) / a;  out.rgb = (n * h + N * c) / (n + N) per channel;  out.w = n + N
 *   invalid inputs (comparisons and selects only: where no rule fires, the bits above are untouched):
 *            a pixel whose accumulation rgb is not finite takes the pass-through {c, N} as bits;
 *            a tap whose history rgb or count is not finite is not accepted, exactly like a tap on another triangle;
 *            a blend whose rgb is not finite (a finite history or accumulation near FLT_MAX times its count) is the pass-through.
 *            So every output pixel is finite unless its own accumulation pixel is not, a poisoned history heals on the next call (a
 *            non-finite history pixel reaches no output), and only the pixels whose footprint holds an invalid pixel change at all.
 *            A NaN in normal_depth fails its comparison (a miss, a rejected tap, a footprint outside): the pass-through.
 * PT_TEMPORAL_HISTORY_CAP = 256 is the default cap (pathtracer.TemporalHistory, acgpt_main --history-in), from a sweep on the CPU
 * oracle's Cornell box at 128 x 128 (tests/test_temporal_host.py): a 256-spp history and an 8-spp accumulation 10 degrees of orbit
 * away, against 8192 spp, lose 5.1x of the MSE at any cap >= 256; with a converged history, caps 128 ... 256 are best (the bilinear
 * resampling's blur weighs more as the history does).
 * The first call after pt_set_scene builds an n_tris-byte array of the triangles' bsdfTypes on the device (a scatter over the leaf
 * slots); it counts in pt_bvh_info.device_bytes from then on and is freed with the scene.  No atomics: two calls, and the two math
 * modes, give the same bits.
 * A history stays valid for the caller only while the scene, maxDepth, useDirectLighting, useImportanceSampling, the light mode and the
 * math mode stay as they were: a key toggle or a reset that restarts the accumulation (PathTracerMain.cpp updateState) also discards
 * the history.  A camera move does not; it is what the call is for (the scene is static).                                     */
#define PT_TEMPORAL_HISTORY_CAP 256.0f
int pt_temporal_blend(pt_ctx* ctx, const pt_params* params, uint32_t accum_samples, const float* albedo_prim, const float* normal_depth,
                      const pt_params* prev, const float* prev_history, const float* prev_albedo_prim, const float* prev_normal_depth,
                      float history_cap, float* out_history);

/* pt_temporal_blend_motion is pt_temporal_blend for a scene whose vertices moved between the two views (pt_update_vertices): the
 * motion of each hit point enters the reprojection, and the history mean is clipped to the current neighbourhood's spread, which limits
 * moved shadows and changed indirect light on surfaces that did not move themselves (SVGF's motion vectors and a variance clip).
 * Every argument pt_temporal_blend takes means the same here, every step above stays as it is, and so does everything it promises
 * (rank 0 of a group, never writes the accumulation, the frame buffer or pt_stats, no atomics, same bits twice and in both math modes).
 *   verts_xyzw, prev_verts_xyzw   DEVICE float[n_verts * 4] in pt_set_scene's layout (w ignored): the positions the current view was
 *                 traced with (the scene's current ones) and those the previous view was traced with; both or neither (no motion)
 *   n_verts       the scene's vertex count
 *   clip_gamma    finite, >= 0; 0 turns the clip off
 * Two additions, fp32 in the order written (tests/motion_ref.py is the NumPy statement of the same thing):
 *   motion   after "ray", for a diffuse hit p on triangle prim: i0, i1, i2 = the scene's index buffer at prim, D_k = prev_v[i_k] - v[i_k]
 *            per component.  If all nine components are zero, nothing is added (m = 0) and no barycentrics are computed.  Else
 *            Moller-Trumbore on the current triangle with the feature ray (o = eye, d = dir_p), no fma, dots left to right:
 *            e1 = v1 - v0, e2 = v2 - v0, pv = cross(d, e2), det = dot(e1, pv), b1 = dot(o - v0, pv) / det,
 *            b2 = dot(d, cross(o - v0, e1)) / det, m = (D0 + b1 (D1 - D0)) + b2 (D2 - D0); a non-finite m is the pass-through.
 *            Then v = ((eye + t_p * dir_p) + m) - eye', and project, taps, sums and count go on exactly as above.  A triangle that did
 *            not move therefore gives pt_temporal_blend's bits exactly.
 *   clip     (clip_gamma > 0) before the blend, per channel: over the 3 x 3 neighbourhood of p in the accumulation, taps inside the
 *            image, dy outer, dx inner, k taps: mu = sum c / k, sigma = sqrtf(max(0, sum c^2 / k - mu^2));
 *            h = min(max(h, mu - gamma sigma), mu + gamma sigma)
 *   invalid inputs: pt_temporal_blend's rules, and in the clip a neighbour whose rgb is not all finite is left out of the moments (k
 *            counts the rest; the pixel itself is finite, so k >= 1); if sum c^2 / k - mu^2 is not finite, sigma = 0.  The bounds are
 *            then never NaN.  An invalid accumulation pixel therefore reaches its 3 x 3 neighbours through the clip and no further.
 * PT_TEMPORAL_CLIP_GAMMA is the default clip (pathtracer.TemporalHistory(motion=True) when the positions differ between the views,
 * acgpt_main --move-history), the best gamma at cap 256 of a sweep on the CPU oracle (tests/test_motion_host.py).
 * The index buffer is read on the device: the first call with vertex arrays uploads it, as the first pt_update_vertices does (the same
 * array, 12 B per triangle, counted in pt_bvh_info.device_bytes from then on, freed with the scene).  Refused before any device work,
 * with a message, leaving the context usable: whatever pt_temporal_blend refuses, one vertex array without the other, a wrong n_verts,
 * a negative or non-finite clip_gamma, out_history overlapping any input (the vertex arrays included).
 * A history stays valid across pt_update_vertices when the caller keeps the positions each view was traced with and passes them here;
 * everything else that discards it above still does.                                                                            */
#define PT_TEMPORAL_CLIP_GAMMA 4.0f
int pt_temporal_blend_motion(pt_ctx* ctx, const pt_params* params, uint32_t accum_samples, const float* albedo_prim, const float* normal_depth,
                             const pt_params* prev, const float* prev_history, const float* prev_albedo_prim, const float* prev_normal_depth,
                             const float* verts_xyzw, const float* prev_verts_xyzw, size_t n_verts, float history_cap, float clip_gamma,
                             float* out_history);

/* ---- display transform (opt-in; nothing above changes) ------------------------------------------------------------------------
 * pt_display_transform is the last stage of the preview chain: it meters a linear HDR image (histogram auto-exposure), applies the
 * exposure and a tone curve, and writes display-linear floats and / or the 8-bit sRGB colours of make_color.  Enqueues on the
 * context's stream and returns synchronised, acts on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the
 * context's frame buffer or pt_stats.  A caller of the reference's loop calls it after LaunchCurrentFrame, or after the denoise or
 * the blend, and before display.
 *   src_rgba          DEVICE float4[n_pixels] of linear radiance: the accumulation buffer, a pt_denoise output, a temporal history;
 *                     .w is not read
 *   out_rgba          DEVICE float4[n_pixels], display-linear {r, g, b, 1} in [0, 1]; must not overlap src_rgba
 *   framebuffer_rgba  uchar4[n_pixels], device or mapped host, as for pt_resolve_framebuffer: make_color of the same {r, g, b}
 *   info              HOST, what was metered and applied
 * Each of out_rgba, framebuffer_rgba and info may be NULL, but not both outputs.  n_pixels in [1, 2^31].
 * The arithmetic.  All floating point is fp32, one rounding per written operation, no contraction, IEEE division; no transcendental
 * function anywhere in the metering or the curves (the sRGB powf of make_color is the only one, after them); the metering runs on
 * integers, so the order of the atomic adds cannot change a bit.  tests/display_ref.py is the NumPy statement of the same thing.
 *   lum(c) = 0.2126 c.r + 0.7152 c.g + 0.0722 c.b, left to right (pt_denoise's l)
 *   Metering (exposure == 0):
 *     a pixel is metered if l = lum(src.rgb) is finite and l >= 2^-20, else it counts in unmetered_pixels
 *     its bin is k = min((bits(l) >> 20) - 856, 319): eight bins per octave from 2^-20 upward, read off the float's own exponent and
 *     top three mantissa bits (856 = bits(2^-20) >> 20); counts h_k are uint32; c_k = h_0 + ... + h_(k-1)
 *     1  n = sum h_k;  r_lo = n * lo_permille / 1000, r_hi = n * hi_permille / 1000  (uint64, integer division)
 *     2  if r_hi <= r_lo: r_lo = 0, r_hi = n
 *     3  t_k = max(0, min(c_k + h_k, r_hi) - max(c_k, r_lo)): the pixels of bin k whose rank lies in the window
 *     4  T = sum t_k,  S = sum t_k * (2k + 1)  (uint64)
 *     5  L_avg = as_float((856 << 20) + (S << 19) / T)  (integer division): the windowed mean of the bin centres in the piecewise-
 *        linear log domain, turned back into a float
 *     6  target = key / L_avg, then max(target, min_exposure), then min(that, max_exposure)
 *     7  exposure = prev_exposure > 0 ? prev_exposure + (target - prev_exposure) * adapt : target
 *     n == 0: exposure = prev_exposure > 0 ? prev_exposure : 1, metered_luminance = 0 (no clamp, no adaptation)
 *     A flat image of luminance L gets key / (the centre of L's bin): within half a bin of key / L, about 4.4 % (2^(1/16); the bins
 *     are linear inside an octave, so it is 5.9 % in an octave's first bin and 3.2 % in its last).
 *   Manual (exposure > 0): that factor; nothing is metered, and info holds it, zero counts and a zero histogram.
 *   Apply, per channel:  v = src * exposure;  x = v > 0 ? (v < 65504 ? v : 65504) : 0  (NaN and negatives 0, infinity 65504)
 *     PT_TONE_LINEAR    y = min(x, 1)
 *     PT_TONE_ACES      y = min((x * (2.51 x + 0.03)) / (x * (2.43 x + 0.59) + 0.14), 1)  (Narkowicz 2015)
 *     PT_TONE_REINHARD  l = lum(x);  s = l > 0 ? (1 + l / (white * white)) / (1 + l) : 0;  y = min(x * s, 1)
 *     out_rgba = {y.r, y.g, y.b, 1};  framebuffer_rgba = make_color(y), the function behind pt_resolve_framebuffer
 * Refused before any device work, with a message, leaving the context usable: a NULL src_rgba or params; both outputs NULL; n_pixels
 * outside [1, 2^31]; an unknown tone curve; a negative or non-finite exposure; in automatic mode a key that is not finite or not
 * > 0, lo_permille >= hi_permille, hi_permille > 1000, min_exposure or max_exposure not finite, min_exposure <= 0 or > max_exposure,
 * a negative or non-finite prev_exposure, adapt outside [0, 1]; under PT_TONE_REINHARD a white that is not finite or not > 0;
 * out_rgba overlapping src_rgba.
 * Three kernels (csrc/display.hip): a grid-stride histogram (per-wave LDS histograms, one vector atomicAdd per non-empty bin and
 * workgroup), one wave that turns the counts into the exposure, and the apply pass, which reads the exposure from the device
 * record: no host round trip in between.  The context keeps the histogram and that record (about 2.6 KB), freed by pt_destroy.  Two
 * calls give the same bits, and so do the two math modes (pt_set_math_mode does not reach this code).                            */
#define PT_TONE_LINEAR   0   /* exposure only, clamp */
#define PT_TONE_REINHARD 1   /* extended Reinhard on luminance, white point `white` */
#define PT_TONE_ACES     2   /* Narkowicz' fitted ACES curve, per channel */

typedef struct {
    uint32_t tone_curve;     /* PT_TONE_* */
    float    exposure;       /* > 0: manual, metering is skipped; 0: automatic */
    float    key;            /* automatic: target for the metered luminance; default 0.18 */
    float    white;          /* REINHARD: luminance that maps to 1; finite, > 0; default 4 */
    uint32_t lo_permille;    /* automatic: share of metered pixels ignored at the dark end; default 100 */
    uint32_t hi_permille;    /* ... the metering window ends here; default 900; lo < hi <= 1000 */
    float    min_exposure;   /* clamp of the automatic exposure; 0 < min <= max, finite */
    float    max_exposure;
    float    prev_exposure;  /* > 0: the last frame's exposure (eye adaptation); 0: none */
    float    adapt;          /* in [0, 1]: exposure = prev + (target - prev) * adapt; 1 = jump */
} pt_display_params;

#define PT_DISPLAY_BINS 320
typedef struct {
    float    exposure;            /* the factor that was applied */
    float    metered_luminance;   /* automatic: L_avg above; manual: 0 */
    uint32_t metered_pixels;      /* pixels that entered the histogram */
    uint32_t unmetered_pixels;    /* the rest: luminance below 2^-20, zero, negative or not finite */
    uint32_t histogram[PT_DISPLAY_BINS];   /* automatic: the counts; manual: zeros */
} pt_display_info;

int pt_display_transform(pt_ctx* ctx, const float* src_rgba, size_t n_pixels, const pt_display_params* dp,
                         float* out_rgba, uint8_t* framebuffer_rgba, pt_display_info* info);

/* ---- convergence estimate (opt-in; nothing above changes) ---------------------------------------------------------------------
 * pt_convergence_update says when an image is finished and where its noise is: a per-pixel estimate of the relative standard error
 * of the accumulated mean, a per-tile max of it, and a histogram with a quantile for a stopping rule.  It needs nothing from the
 * render kernel: after k frames the accumulation holds the running mean A_k, the difference between two successive accumulations
 * fixes the mean of the frames rendered in between, and a weighted Welford update (West 1979) over those batch means gives an
 * unbiased variance of the accumulated mean.  Enqueues on the context's stream and returns synchronised, covers the whole image, acts
 * on rank 0 of a pt_create_multi context, never writes the accumulation buffer, the frame buffer or pt_stats.  A caller of the
 * reference's loop calls it after LaunchCurrentFrame, once per launch or per batch of frames.
 *   params        only width, height and accumulationBuffer are read (DEVICE float4[w*h], row 0 at the bottom; .w is not read)
 *   accum_frames  in [1, 2^24]: the equal-spp frames the accumulation stands for (currentFrameIdx plus the frames just launched)
 *   state         DEVICE float4[w*h] {l0, M2, k0, B}: the luminance and frame count at the last call, the weighted sum of squares
 *                 and the number of observations.  The caller owns it, as it owns a temporal history, zero-fills it to start, and
 *                 passes it to every call; it is updated in place
 *   out_error     DEVICE float[w*h] or NULL: err below, -1 where the pixel has none yet
 *   out_tiles     DEVICE float[ceil(w/16) * ceil(h/16)] or NULL, row-major with tile row 0 at the bottom: the max err over the
 *                 measured pixels of each 16 x 16 tile, -1 for a tile without one
 *   info          HOST or NULL
 * The arithmetic.  All floating point is fp32, one rounding per written operation, no contraction, IEEE division and sqrtf; every
 * reduction runs on integers or is a max, so the order of the atomics cannot change a bit.  tests/convergence_ref.py is the NumPy
 * statement of the same thing.
 *   lum as for pt_denoise, left to right;  k1 = (float)accum_frames;  l1 = lum(accum.rgb);  {l0, M2, k0, B} = state
 *   1  l1 not finite: state = {0, 0, 0, 0}, the pixel counts as invalid (and not as unmeasured), out_error = -1
 *   2  else if !(k0 > 0) || !(k1 > k0): state = {l1, 0, k1, 1}: a first observation or a restarted accumulation; unmeasured, -1
 *   3  else n = k1 - k0;  d = l1 - l0;  w = (k0 * k1) / n;  M2' = M2 + w * (d * d);  B' = B + 1;  state = {l1, M2', k1, B'}
 *      (West's update with the batch mean eliminated: no k A_k - (k - 1) A_(k-1) cancellation); the pixel is measured:
 *      v = M2' / ((B' - 1) * k1);  sem = sqrtf(v);  err = sem / max(l1, lum_floor)
 *   over the measured pixels: converged_pixels counts err <= threshold; max_error is the max of bits(err) as uint32 (non-negative
 *   floats: unsigned order is float order); the histogram bin is clamp((bits(err) >> 20) - 824, 0, 255): eight bins per octave from
 *   2^-24, both end bins open (a NaN err lands in bin 255); with n = measured_pixels, r = max(1, (n * quantile_permille + 999) /
 *   1000) in uint64, j the first bin whose inclusive prefix count is >= r, quantile_error = as_float((824 + j + 1) << 20).
 * Refused before any device work, with a message, leaving the context usable: a NULL ctx, params, cp, state or accumulationBuffer; a
 * zero width or height, or w * h > 2^31; accum_frames outside [1, 2^24]; a lum_floor or threshold that is not finite or not > 0; a
 * quantile_permille outside [1, 1000]; a non-zero reserved; state, out_error or out_tiles overlapping the accumulation buffer or
 * each other.
 * Two kernels (csrc/convergence.hip): the update, one workgroup per 16 x 16 tile with per-wave LDS counters and one vector atomic
 * per non-empty slot and workgroup, and one wave that scans the bins for the quantile, writes the record and clears the counts.
 * The context keeps the counts and that record (about 2 KB), freed by pt_destroy.  Two calls with the same inputs give the same
 * bits, and so do the two math modes (pt_set_math_mode does not reach this code).
 * The estimate assumes frames of equal spp and independent seeds (distinct currentFrameIdx); it measures the noise of the luminance,
 * not bias, and a pixel whose every batch mean is equal (a black pixel, a directly seen light) reads err = 0.                   */
typedef struct {
    float    lum_floor;         /* finite, > 0: error = sem / max(l, lum_floor); default 0.01 */
    float    threshold;         /* finite, > 0: a pixel is converged when its error <= threshold; default 0.02 */
    uint32_t quantile_permille; /* in [1, 1000]: which quantile of the error info reports; default 950 */
    uint32_t reserved;          /* 0 */
} pt_convergence_params;

#define PT_CONVERGENCE_BINS 256
#define PT_CONVERGENCE_TILE 16
typedef struct {
    uint32_t frames;              /* accum_frames of this call */
    uint32_t measured_pixels;     /* pixels with an error (at least two observations) */
    uint32_t unmeasured_pixels;   /* one observation so far, or restarted in this call */
    uint32_t invalid_pixels;      /* luminance not finite: the pixel's state was cleared */
    uint32_t converged_pixels;    /* measured pixels with error <= threshold */
    float    max_error;           /* over the measured pixels; 0 if none */
    float    quantile_error;      /* upper edge of the histogram bin holding the quantile; 0 if none */
    uint32_t reserved;
    uint32_t histogram[PT_CONVERGENCE_BINS];
} pt_convergence_info;

int pt_convergence_update(pt_ctx* ctx, const pt_params* params, uint32_t accum_frames,
                          const pt_convergence_params* cp, float* state,
                          float* out_error, float* out_tiles, pt_convergence_info* info);

/* ---- firefly filter (opt-in; nothing above changes) ---------------------------------------------------------------------------
 * pt_firefly_filter clamps isolated outlier pixels ahead of the denoiser and replaces pixels that hold no usable value: a pixel may
 * be `ratio` times brighter than the rank-th brightest of its 3 x 3 or 5 x 5 neighbours and no more.  pt_denoise widens its
 * luminance stop with the local variance, so one spike opens the stop of its whole neighbourhood and is spread into a blob; a NaN
 * or an infinity in the accumulation passes every other stage untouched.  The clamp removes energy, which is a bias: info reports
 * how much.  Enqueues on the context's stream and returns synchronised, acts on rank 0 of a pt_create_multi context, needs no scene,
 * never touches the accumulation buffer (unless it is passed as src, which is only read), the frame buffer or pt_stats.  A caller of
 * the reference's loop calls it between LaunchCurrentFrame and the denoiser.
 *   src_rgba   DEVICE float4[width * height], row-major; only read
 *   out_rgba   DEVICE float4[width * height]; must not overlap src_rgba (refused, not undefined)
 *   info       HOST or NULL (NULL skips only the copy to the host)
 * The arithmetic.  All floating point is fp32, one rounding per written operation, no contraction, IEEE division; the reductions are
 * integer sums and a max of bit patterns, so the order of the atomics cannot change a bit.  tests/firefly_ref.py is the NumPy
 * statement of the same thing.
 *   l(p) = (0.2126f * r + 0.7152f * g) + 0.0722f * b;   valid(p): l(p) is finite and l(p) >= 0
 *   N(p): the taps q = p + (dx, dy), dx and dy in [-radius, radius] without (0, 0), dy outer, dx inner, both ascending, that lie
 *         inside the image and are valid
 *   R(p): the rank-th largest l(q) over N(p), counted with multiplicity; undefined when |N(p)| < rank
 *   1  valid p, R undefined: out = src, all four floats as bits; the pixel passes
 *   2  valid p, R defined: t = ratio * max(R(p), floor); if l(p) > t: s = t / l(p), out.rgb = rgb * s, the pixel is clamped;
 *      otherwise out = src as bits and the pixel passes
 *   3  invalid p: out.rgb = (the sum of src.rgb over N(p), per channel, added in tap order from 0.0f) / (float)|N(p)|, or (0, 0, 0)
 *      when N(p) is empty; the pixel is replaced
 *   out.w is src.w as bits in every case (pt_temporal_blend keeps a sample count there).  Neighbours are read from src, never from
 *   out: the result does not depend on the execution order and two calls give the same bits.
 *   info: clamped_pixels + replaced_pixels + passed_pixels = width * height; max_ratio is the max of bits(l(p) / t) as uint32 over
 *   the clamped pixels (positive floats: unsigned order is float order), 0 if none; removed_luma_q16 is the sum over the clamped
 *   pixels of (uint64) trunc(min(l(p) - t, 2^24) * 65536) and total_luma_q16 the sum over the valid pixels of (uint64) trunc(min(l(p),
 *   2^24) * 65536), both modulo 2^64: removed / total is the share of the image's energy the filter took.
 * Refused before any device work, with a message, leaving the context usable: a NULL ctx, src_rgba, fp or out_rgba; a zero width or
 * height, or width * height > 2^31; a ratio that is not finite or < 1; a floor that is not finite or not > 0; a rank outside [1, 4];
 * a radius other than 1 or 2; out_rgba overlapping src_rgba.
 * Two kernels (csrc/firefly.hip): the filter, one workgroup per 16 x 16 tile with the tile's luminances and their halo in LDS and
 * one vector atomic per workgroup and field, and one lane that writes the record and clears the counts.  The context keeps the
 * counts and that record (72 bytes), freed by pt_destroy.  pt_set_math_mode does not reach this code.
 * An edge between two materials or at an emitter survives: an edge pixel has neighbours on its own side.  A bright feature thinner
 * than `rank` pixels of a window does not; raise rank to keep it.                                                                */
typedef struct pt_firefly_params {
    float    ratio;    /* finite, >= 1: a pixel may be this many times brighter than its reference neighbour; default 16 */
    float    floor;    /* finite, > 0: the reference luminance is never taken below this; default 0.01 */
    uint32_t rank;     /* 1..4: the reference neighbour is the rank-th brightest; default 1 */
    uint32_t radius;   /* 1 or 2: a 3 x 3 or a 5 x 5 window; default 1 */
} pt_firefly_params;

typedef struct pt_firefly_info {
    uint32_t clamped_pixels;    /* valid pixels scaled down to their limit */
    uint32_t replaced_pixels;   /* invalid pixels (NaN, infinite or negative luminance) replaced by their neighbours' mean */
    uint32_t passed_pixels;     /* valid pixels left as they were */
    uint32_t reserved;
    uint64_t total_luma_q16;    /* the luminance of the valid pixels, in 2^-16 */
    uint64_t removed_luma_q16;  /* the luminance the clamp took, in 2^-16 */
    float    max_ratio;         /* the largest l / t among the clamped pixels; 0 if none */
    uint32_t reserved2;
} pt_firefly_info;

int pt_firefly_filter(pt_ctx* ctx, const float* src_rgba, uint32_t width, uint32_t height,
                      const pt_firefly_params* fp, float* out_rgba, pt_firefly_info* info);

/* ---- bloom (opt-in; nothing above changes) -------------------------------------------------------------------------------------
 * pt_bloom adds the glare of the pixels brighter than display white to a linear HDR image, ahead of pt_display_transform: the tone
 * curves clamp at 1, so without it an emitter of radiance 15 and one of 1500 are the same flat disc.  The part of every pixel above
 * a threshold goes down an image pyramid (a 4 x 4 binomial per level) and comes up again (bilinear), every level added to the next
 * finer one; the sum, scaled so that the filters together have the gain `intensity`, is added to the source.  Enqueues on the
 * context's stream and returns synchronised, acts on rank 0 of a pt_create_multi context, needs no scene, never writes the
 * accumulation buffer (unless it is passed as src, which is only read), the frame buffer or pt_stats.  A caller of the reference's
 * loop calls it after the denoiser and before the display transform.
 *   src_rgba   DEVICE float4[width * height], row-major, linear radiance; only read
 *   out_rgba   DEVICE float4[width * height]; must not overlap src_rgba (refused, not undefined)
 *   info       HOST or NULL (NULL skips only the copy to the host)
 * The arithmetic.  All floating point is fp32, one rounding per written operation, evaluated left to right as bracketed, no
 * contraction, IEEE division, no transcendental function; the reductions are integer sums and a max of bit patterns, so the order of
 * the atomics cannot change a bit.  tests/bloom_ref.py is the NumPy statement of the same thing.
 *   Levels.  (w_0, h_0) = (width, height); w_k = (w_(k-1) + 1) / 2 in integers, h_k likewise; n = min(levels, the first k with
 *     w_k = h_k = 1): a 1 x 1 source builds one 1 x 1 level.  cx_k(i) = min(max(i, 0), w_k - 1), cy_k likewise: clamp to the edge.
 *   Prefilter P(p).  l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;  valid(p): l is finite and l >= 0.  An invalid pixel gives
 *     P = (0, 0, 0).  A valid one:  d = l - threshold;
 *       knee > 0:  s = min(max(l - (threshold - knee), 0), knee + knee);  q = (s * s) / ((knee + knee) + (knee + knee));  e = max(q, d)
 *       knee = 0:  e = max(d, 0)
 *       clamp > 0: e = min(e, clamp)
 *     e > 0: c = e / l, P = rgb * c per channel, the pixel is bright; otherwise P = 0.  With threshold = knee = clamp = 0, c is
 *     exactly 1 and P is the pixel's own bits.
 *   Down D, level a to level a + 1 at (X, Y), per channel: the separable binomial {1, 3, 3, 1} / 8 over the 4 x 4 footprint
 *     row(y) = ((0.125f * A(cx_a(2X-1), y) + 0.375f * A(cx_a(2X), y)) + 0.375f * A(cx_a(2X+1), y)) + 0.125f * A(cx_a(2X+2), y)
 *     D = ((0.125f * row(cy_a(2Y-1)) + 0.375f * row(cy_a(2Y))) + 0.375f * row(cy_a(2Y+1))) + 0.125f * row(cy_a(2Y+2))
 *     level 1 = D of the prefiltered source (P in A's place), level k + 1 = D of level k.
 *   Up U, level b to the size of level b - 1 at (x, y), per channel: bilinear at the texel centres.  i = x >> 1;
 *       x even: j0 = cx_b(i - 1), j1 = i, (a0, a1) = (0.25f, 0.75f);   x odd: j0 = i, j1 = cx_b(i + 1), (a0, a1) = (0.75f, 0.25f)
 *     row(yy) = a0 * E(j0, yy) + a1 * E(j1, yy); the same rule in y gives k0, k1, b0, b1;  U = b0 * row(k0) + b1 * row(k1)
 *   Combine.  E_n = level n; for k = n - 1 .. 1: E_k = D_k + spread * U(E_(k+1)), in place (a texel reads only itself on its own
 *     level).  On the host, in fp32: norm = 1, t = 1, then n - 1 times t = t * spread, norm = norm + t;  gain = intensity / norm.
 *   Output.  out.rgb = src.rgb + gain * U(E_1);  out.w = src.w as bits.  The add is a plain IEEE add: a NaN or infinite source pixel
 *     stays what it was (a signalling NaN quieted) and, feeding nothing, reaches no other pixel; -0 becomes +0.
 *   info: total_luma_q16 is the sum over the valid pixels of (uint64) trunc(min(l, 2^24) * 65536) and bright_luma_q16 the same
 *     conversion of e over the bright pixels, both modulo 2^64: bright / total is the share of the image's luminance that glares;
 *     max_luma is the max of bits(l) as uint32 over the valid pixels (unsigned order is float order for l >= +0; a luminance of -0,
 *     which only a pixel of zeros with a sign gives, counts with its own bits), 0 if none.
 * Refused before any device work, with a message, leaving the context usable: a NULL ctx, src_rgba, bp or out_rgba; a zero width or
 * height, or width * height > 2^31; a threshold, clamp or intensity that is not finite or < 0; a knee that is not finite or outside
 * [0, threshold]; a spread that is not finite or outside [0, 4]; levels outside [1, 8]; out_rgba overlapping src_rgba.
 * Kernels (csrc/bloom.hip): prefilter and first down step in one, a workgroup per 16 x 16 tile of level 1 with the prefiltered 34 x
 * 34 source footprint in LDS and one vector atomic per workgroup and field; the same kernel without the prefilter for the further
 * levels; one kernel for every up step, the last of which is the composite; one lane that writes the record and clears the counts:
 * 2 n + 1 launches.  The context keeps the pyramid (float4 per texel, all levels in one allocation, at most a third of the source
 * plus a few texels; it grows on demand), the counts and the record (72 bytes), all freed by pt_destroy.  Two calls give the same
 * bits; pt_set_math_mode does not reach this code.                                                                              */
typedef struct pt_bloom_params {
    float    threshold;  /* finite, >= 0, in src's radiance units: luminance below it does not glare; 0: everything does; default 1 */
    float    knee;       /* finite, 0 <= knee <= threshold: half width of the soft transition around threshold; 0: hard; default 0.5 */
    float    clamp;      /* finite, >= 0: most luminance one pixel may feed into the pyramid; 0: no limit (the default) */
    float    intensity;  /* finite, >= 0: the glare added is intensity x the spread-out bright part; default 0.02 */
    float    spread;     /* finite, in [0, 4]: weight of each coarser level against the next finer one; 1: all equal (the default) */
    uint32_t levels;     /* 1..8 requested; fewer are built when the image runs out (info.levels); default 6 */
} pt_bloom_params;

typedef struct pt_bloom_info {
    uint32_t levels;           /* n, the levels built */
    uint32_t bright_pixels;    /* valid pixels with e > 0 */
    uint32_t invalid_pixels;   /* NaN, infinite or negative luminance: they feed nothing */
    uint32_t reserved;
    uint64_t total_luma_q16;   /* the luminance of the valid pixels, in 2^-16 */
    uint64_t bright_luma_q16;  /* the luminance e the bright pixels fed into the pyramid, in 2^-16 */
    float    max_luma;         /* the largest luminance among the valid pixels; 0 if none */
    uint32_t reserved2;
} pt_bloom_info;

int pt_bloom(pt_ctx* ctx, const float* src_rgba, uint32_t width, uint32_t height,
             const pt_bloom_params* bp, float* out_rgba, pt_bloom_info* info);

/* ---- device memory helpers for bindings that have no HIP runtime of their own
 * (the reference app calls cudaMalloc/cudaMemcpy directly, :145-148).         */
int pt_device_malloc(pt_ctx* ctx, void** out, size_t bytes);
int pt_device_free(pt_ctx* ctx, void* ptr);
int pt_device_memset(pt_ctx* ctx, void* ptr, int value, size_t bytes);
int pt_copy_to_host(pt_ctx* ctx, void* dst_host, const void* src_device, size_t bytes);
int pt_copy_to_device(pt_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);
int pt_host_malloc_mapped(pt_ctx* ctx, void** host_out, void** device_out, size_t bytes);
int pt_host_free_mapped(pt_ctx* ctx, void* host_ptr);

/* Version of this ABI. */
uint32_t pt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ACGPT_H */
