// PathTracerMain.cpp — headless counterpart of the reference's PathTracer_Optix/PathTracerMain.cpp.
//
// Same structure, same function names over a PathTracerState, same defaults (512x512, 128 samples
// per launch, maxDepth 4, both toggles off, the hard-coded area light and camera); what the
// reference hard-codes or reads from the keyboard is a command line here, and frames go to image
// files instead of a GLFW window:
//
//   acgpt_main --obj scene.obj [--width 512 --height 512] [--spp-per-launch 128] [--frames 8] [--fuse-frames 1]
//              [--max-depth 4] [--direct-lighting] [--importance-sampling] [--device 0]
//              [--keys "0,1,UP,UP,R"] [--out frame.png] [--dump-every k] [--zero-copy]
//              [--orbit dx,dy] [--zoom n] [--sample-chunks c] [--build-mode 0|1]
//              [--gpus N] [--multi] [--save-accum file] [--restore-accum file] [--light-mode 0|1] [--math fast|ieee]
//              [--denoise N] [--history-out file] [--history-in file] [--move material:dx,dy,dz [--move-history]]
//              [--set-material name:kd=r,g,b[,ke=r,g,b][,bsdf=diffuse|metal|glass][,ior=x] ...]
//              [--env map.hdr|map.pfm [--env-scale s]] [--no-area-light] [--materials reference|microfacet]
//              [--tonemap linear|reinhard|aces] [--exposure auto|<EV>] [--out-hdr file.pfm]
//              [--until-error E [--until-permille P] [--error-floor F] [--error-out file.pfm]]
//              [--firefly ratio[,rank[,radius]]] [--bloom [threshold,intensity[,levels[,spread]]]] [--pick x,y ...]
//              [--nearest x,y,z[,radius] ...] [--pick-all x,y[,k] ...] [--overlap cx,cy,cz,hx,hy,hz[,k|,all] ...] [--overlap-oriented cx,cy,cz,hx,hy,hz,qw,qx,qy,qz[,k|,all] ...] [--intersect x0,y0,z0,x1,y1,z1,x2,y2,z2[,k|,all] ...]
//              [--cast x0,y0,z0,x1,y1,z1,x2,y2,z2,dx,dy,dz[,tmax] ...] [--cast-mesh mesh.obj,dx,dy,dz[,tmax] ...]
//              [--sweep ox,oy,oz,dx,dy,dz,r[,tmax] ...] [--capsule-cast x0,y0,z0,x1,y1,z1,dx,dy,dz,r[,tmax] ...]
//              [--box-cast cx,cy,cz,hx,hy,hz,qw,qx,qy,qz,dx,dy,dz[,tmax] ...] [--clearance x0,y0,z0,x1,y1,z1[,radius] ...]
//              [--tri-distance x0,y0,z0,x1,y1,z1,x2,y2,z2[,radius] ...]
//              [--collide mesh.obj[,tx,ty,tz[,radius]] ...]
//              [--nearest-k x,y,z,k[,radius] ...] [--within x,y,z,radius ...] [--winding x,y,z[,beta] ...]
//              [--ao K[,radius[,bias]] --ao-out file.pfm [--ao-frames n]]
// --ao K[,radius[,bias]] with --ao-out: once the scene is set and before the first frame, the ambient occlusion of the view
// (pt_render_features + pt_ao_image): K rays per pixel (1..256) and call over --ao-frames calls (default 1; call j has seed j and
// accumulates), on the default pattern — the Vogel spiral of pathtracer.aoSamples, the same formula in double —, written as a .pfm
// (grey in three channels, bottom row first).  radius defaults to a quarter of the scene box's diagonal, bias to a thousandth of it,
// both computed in double and rounded.  The frames are the same with or without it.
// --pick x,y (repeatable): once the scene is set and before the first frame, what lies under pixel (x, y), row 0 at the bottom: the
// closest hit of the camera ray through the pixel's centre (pt_query_closest; the ray of pt_render_features), one JSON line each:
// {"pick": [x, y], "hit": true, "t": .., "prim": .., "material": "<newmtl name>", "position": [eye + t * dir], "normal": [..]}, on a
// miss {"pick": [x, y], "hit": false}.  Floats are printed with nine digits: they read back as the same fp32 values.  A pixel
// outside the image is refused with exit status 2.  The frames are the same with or without it.
// --pick-all x,y[,k] (repeatable): --pick's camera ray, and everything it goes through (pt_query_multi with counts, one call): one JSON
// line each, {"pick_all": [x, y], "count": <triangles the ray crosses inside the interval>, "hits": [<the first k of them in order of
// (t, prim), k = 1..8, default 4, each with --pick's fields t, prim, material, position, normal>]}.  A pixel outside the image or a k
// outside 1..8 is refused with exit status 2.  The frames are the same with or without it.
// --nearest x,y,z[,radius] (repeatable): once the scene is set and before the first frame, the closest surface point to (x, y, z) within
// radius (no limit if not given), by pt_query_nearest in one call, one JSON line each: {"nearest": [x, y, z], "found": true,
// "distance": .., "triangle": .., "material": "<newmtl name>", "point": [..], "u": .., "v": ..} (u, v the weights of the triangle's second
// and third vertex at the point), {"nearest": [x, y, z], "found": false} if nothing lies within the radius.  Floats are printed with
// nine digits.  A coordinate that is not finite or a radius that is negative or no number is refused with exit status 2.  The frames
// are the same with or without it.
// --nearest-k x,y,z,k[,radius] (repeatable): once the scene is set and before the first frame, the k closest triangles (k = 1..8) of the
// point within the radius (default: no limit) in order, by pt_query_nearest_k with counts in one call per k, one JSON line each:
// {"nearest_k": [x, y, z], "k": k, "count": <triangles within the radius>, "list": [{"distance": .., "triangle": .., "material":
// "<newmtl name>", "point": [..], "u": .., "v": ..} per listed triangle, closest first]}.  Floats are printed with nine digits.  A
// coordinate that is not finite, a k outside 1..8 or a radius that is negative or no number is refused with exit status 2.
// --within x,y,z,radius (repeatable): whether anything of the scene lies within the radius of the point, all in one call of
// pt_query_within_any, one JSON line each: {"within": [x, y, z], "radius": r, "hit": true or false}.  The same refusals.  The frames
// are the same with or without either.
// --winding x,y,z[,beta] (repeatable): once the scene is set and before the first frame, the generalised winding number of the mesh at
// the point (pt_query_winding, one call per point; beta >= 1, default PT_WINDING_BETA_DEFAULT, inf for the exact sum), one JSON line
// each: {"winding": [x, y, z], "beta": b, "w": .., "inside": true or false} (inside: w > 0.5; an infinite beta is printed as the
// string "inf").  A coordinate that is not finite or a beta below 1 or no number is refused with exit status 2.  The frames are the
// same with or without it.
// --overlap cx,cy,cz,hx,hy,hz[,k] (repeatable): once the scene is set and before the first frame, the triangles that overlap the
// axis-aligned box of centre (cx, cy, cz) and half extent (hx, hy, hz), by pt_query_overlap in one call per k, one JSON line each:
// {"overlap": [cx, cy, cz, hx, hy, hz], "count": <triangles that overlap the box>, "triangles": [<the k lowest indices among them,
// k = 0..8, default 8>], "materials": ["<newmtl name>" per listed triangle]}.  A value that is not finite, a negative half extent or a
// k outside 0..8 is refused with exit status 2.  The frames are the same with or without it.  With "all" in place of k the line is the
// same and "triangles" holds every overlapping triangle, ascending: pt_query_overlap counts, pt_list_offsets makes the offsets,
// pt_query_overlap_lists fills the list.
// --overlap-oriented cx,cy,cz,hx,hy,hz,qw,qx,qy,qz[,k] (repeatable): the same for the oriented box whose axes are the columns of the
// rotation of the quaternion (qw, qx, qy, qz), normalised in double here, by pt_query_overlap_oriented and
// pt_query_overlap_oriented_lists: {"overlap_oriented": [the ten numbers, the quaternion normalised], "count", "triangles", "materials"}.
// --intersect x0,y0,z0,x1,y1,z1,x2,y2,z2[,k] (repeatable): once the scene is set and before the first frame, the scene triangles that
// intersect the triangle of these three vertices, by pt_query_triangles in one call per k, one JSON line each: {"intersect": [the nine
// coordinates], "count": <scene triangles that intersect it>, "triangles": [<the k lowest indices among them, k = 0..8, default 8>]}.
// A coordinate that is not finite or a k outside 0..8 is refused with exit status 2.  The frames are the same with or without it.
// "all" in place of k lists every intersecting scene triangle, through pt_query_triangles_lists as --overlap does.
// --sweep ox,oy,oz,dx,dy,dz,r[,tmax] (repeatable): once the scene is set and before the first frame, how far the sphere of radius r
// whose centre starts at o travels along d before it touches the scene (t in units of |d|, at most tmax, default unbounded), all in
// one call of pt_query_sweep, one JSON line each: {"sweep": [ox, oy, oz, dx, dy, dz, r], "tmax": <tmax or null>, "hit": true, "t": ...,
// "triangle": <index>, "material": "<newmtl name>", "point": [x, y, z], "u": ..., "v": ...} (the contact point on the triangle and the
// weights of its second and third vertex there), {"sweep": [...], "tmax": ..., "hit": false} if nothing is touched.  Floats are printed
// with nine digits.  A value that is not finite (tmax may be inf), a negative radius or a negative tmax is refused with exit status 2.
// The frames are the same with or without it.
// --capsule-cast x0,y0,z0,x1,y1,z1,dx,dy,dz,r[,tmax] (repeatable): how far the capsule of radius r around the axis {p0, p1} travels along d
// before it touches the scene (t in units of |d|, at most tmax, default unbounded), all in one call of pt_query_capsule_cast, one JSON
// line each: {"capsule_cast": [the ten numbers], "tmax": <tmax or null>, "hit": true, "t": ..., "triangle": <index>, "material":
// "<newmtl name>", "point": [x, y, z], "s": ..., "feature": <0..5>} (the contact point on the triangle, the parameter of the axis' point
// that touches and pt_query_segments' feature there), {"capsule_cast": [...], "tmax": ..., "hit": false} if nothing is touched.  The same
// refusals as --sweep.  The frames are the same with or without it.
// --box-cast cx,cy,cz,hx,hy,hz,qw,qx,qy,qz,dx,dy,dz[,tmax] (repeatable): how far the box of centre c and half extents h, turned by the unit
// quaternion q, travels along d before it touches the scene (t in units of |d|, at most tmax, default unbounded), all in one call of
// pt_query_box_cast, one JSON line each: {"box_cast": [the thirteen numbers], "tmax": <tmax or null>, "hit": true, "t": ..., "triangle":
// <index>, "material": "<newmtl name>", "feature": <0..13>, "normal": [x, y, z], "point": [x, y, z]} (the winning axis of the 13-axis
// test, 13 for a box that starts in contact; the unit normal from the triangle to the box and the contact point),
// {"box_cast": [...], "tmax": ..., "hit": false} if nothing is touched.  Refused: a value that is not finite, a negative half extent or
// tmax, a quaternion whose squared length is off 1 by more than 1e-4.  The frames are the same with or without it.
// --cast x0,y0,z0,x1,y1,z1,x2,y2,z2,dx,dy,dz[,tmax] (repeatable): how far the triangle of these three vertices translates along d before it
// first touches the scene (t in units of |d|, at most tmax, default unbounded), all in one call of pt_query_triangle_cast, one JSON line
// each: {"cast": [the twelve numbers], "tmax": <tmax or null>, "hit": true, "t": ..., "triangle": <index>, "feature": <0..15>,
// "material": "<newmtl name>", "point": [x, y, z]}, or {"cast": [...], "tmax": ..., "hit": false}.  A value that is not finite (tmax may
// be inf) or a negative tmax is refused with exit status 2.
// --cast-mesh mesh.obj,dx,dy,dz[,tmax] (repeatable): the same for a whole second OBJ, as it is, by pt_set_query_mesh and
// pt_query_poses_cast: {"cast_mesh": "<path>", "triangles": T, "motion": [dx, dy, dz], "tmax": ..., "hit": true, "t": ..., "triangle":
// <scene triangle>, "feature": .., "query_triangle": <the mesh triangle that touches first>, "material": .., "point": [..]}.
// --clearance x0,y0,z0,x1,y1,z1[,radius] (repeatable): once the scene is set and before the first frame, how far the segment from
// (x0, y0, z0) to (x1, y1, z1) is from the scene and where the two come closest, all in one call of pt_query_segments with no limit on
// the distance, one JSON line each: {"clearance": [the six coordinates], "radius": r, "found": true, "distance": .., "clear": <distance
// - radius: negative where a capsule of that radius penetrates>, "triangle": .., "material": "<newmtl name>", "s": <parameter of the
// closest point on the segment>, "feature": <0, 1 an end; 2, 3, 4 an edge of the triangle; 5 the segment crosses it>, "on_segment":
// [..], "point": [<on the triangle>]}, {"clearance": [..], "radius": r, "found": false} for a scene without triangles.  radius
// defaults to 0.  Floats are printed with nine digits.  A coordinate that is not finite or a radius that is negative or no number is
// refused with exit status 2.  The frames are the same with or without it.
// --tri-distance x0,y0,z0,x1,y1,z1,x2,y2,z2[,radius] (repeatable): once the scene is set and before the first frame, how far the
// triangle with these vertices is from the scene and where the two come closest, all in one call of pt_query_triangle_distance, one
// JSON line each: {"tri_distance": [the nine coordinates], "radius": <radius or null>, "found": true, "distance": .., "triangle": ..,
// "material": "<newmtl name>", "feature": <0..2 a vertex of the query; 3..5 a vertex of the scene triangle; 6..14 an edge pair; 15..17
// a query edge crosses the scene triangle; 18..20 a scene edge crosses the query>, "on_query": [<on the query triangle>], "point": [<on
// the scene triangle>]}, {"tri_distance": [..], "radius": .., "found": false} if nothing lies within the radius (default: no limit).
// Floats are printed with nine digits.  Fewer than nine or more than ten numbers, a coordinate that is not finite or a radius that is
// negative or no number is refused with exit status 2.  The frames are the same with or without it.
// --bloom (with --tonemap or --exposure): the image the display transform shows goes through pt_bloom first.  threshold is in display
// units, multiples of exposed white, and is divided by the exposure (and so are the default knee, half the threshold, and the
// clamp, none); an automatic exposure is metered on the image without its glare and then applied as a manual one.  --out-hdr gets
// the glare too.  One line names the levels built, the bright and invalid pixels and the bright share of the luminance.  Without a
// value: threshold 1, intensity 0.02, levels 6, spread 1.
// --firefly: after the last frame the accumulation goes through pt_firefly_filter into a buffer of its own, and that image is what
// --out, --out-hdr, --denoise and --tonemap see; --save-accum, --history-out and --until-error keep the raw accumulation (the
// convergence estimate measures the renderer's noise, not a clamped image).  One line names the pixels clamped and replaced, the
// share of the luminance removed and the largest excess.  rank defaults to 1, radius to 1.
// --until-error E: stop when the image is finished instead of after a fixed count.  After every launch (with --fuse-frames, every
// batch) pt_convergence_update estimates each pixel's relative standard error; the run ends as soon as every pixel has an estimate
// and --until-permille (default 950) of them are at or below E.  --frames becomes the cap.  --error-floor (default 0.01) is the
// luminance below which the error is taken against the floor instead of the pixel.  The last line printed names the frames used,
// the quantile error and the converged share.  --error-out writes the error map as a .pfm (grey in three channels, bottom row
// first, -1 where a pixel has no estimate).  The frames rendered are the same with or without these options.
// --tonemap / --exposure: after the last frame, also write <out-stem>_display<ext>: the accumulation (with --denoise N the denoised
// image) through pt_display_transform — the histogram auto-exposure (auto, the default) or the manual factor 2^EV, computed here, then
// the tone curve (default aces).  The frames and --out are the same with or without them.  --out-hdr writes the linear accumulation
// as a .pfm (bottom row first, as the buffer holds it).
// --materials microfacet (with --light-mode 1): metal and glass honour the MTL's Pr as rough GGX BSDFs (pt_set_material_model); the
// default, reference, is the reference's materials.
// --env: an environment map (Radiance .hdr or .pfm, latitude-longitude, top row = +Y) that rays leaving the scene see, scaled by
// --env-scale (default 1); in light mode 1 it is importance-sampled as a light (pt_set_environment).  --no-area-light zeroes
// params.areaLight.emission, so that a model can be lit by the map alone in light mode 0.
//
// --set-material (repeatable): after the last frame (and after --move's, if given), give the named material (its newmtl name) the
// fields listed — any of kd, ke, bsdf, ior, in any order, each at most once —, apply every edit at once with pt_update_materials —
// no rebuild —, render the same --frames again from a zeroed accumulation and write <out-stem>_material<ext>: the image acgpt_main
// renders of the OBJ with a .mtl edited so, bit for bit.  The run summary gives the update's time.  An unknown material or a
// malformed field is refused, before any device work, with a message and exit status 1.
// --move material:dx,dy,dz: after the last frame, translate every vertex that a face of that material (its newmtl name) references by
// (dx, dy, dz), give the scene the new vertices with pt_update_vertices(PT_UPDATE_REFIT) — no rebuild —, render the same --frames again
// from a zeroed accumulation and write <out-stem>_moved<ext>: the image acgpt_main renders of an OBJ whose vertices were moved so, bit
// for bit.  The run summary gives the update's time and tree-quality ratio.  An unknown material is refused with exit status 2.
// --move-history (with --move only): keep the accumulation before the refit as a history {rgb, frames * spp} with its features, and
// after the moved frames also write <out-stem>_moved_temporal<ext>: that history carried into the moved scene at the same camera by
// pt_temporal_blend_motion (default cap and clip); with --denoise N also <out-stem>_moved_temporal_denoised<ext>.
//
// --denoise N (1..8; default 0 = off): after the last frame, also write <out-stem>_denoised<ext>, the accumulation through N
// iterations of the edge-avoiding a-trous filter guided by first-hit features (pt_render_features + pt_denoise), coloured by
// pt_resolve_framebuffer.  The frames and --out are the same with or without it.
//
// --history-out / --history-in carry the accumulated image across a camera move (pt_temporal_blend).  --history-out writes, after the
// last frame, the history of this run's view: the blended one with --history-in, else the accumulation as {rgb, currentFrameIdx * spp}.
// --history-in reads one written by an earlier run of the same scene and settings (size and camera may differ: --orbit, --zoom) and
// refuses any other with a message and exit status 1.  After the last frame it traces the stored view's features, blends its history
// into this view and writes <out-stem>_temporal<ext>; with --denoise N also <out-stem>_temporal_denoised<ext>, the blend through the
// filter.  File: "ACGPTHST" | width | height | maxDepth | direct lighting | importance sampling | light mode | math mode | triangles
// (uint32 each) | eye, U, V, W (12 floats) | float4[width * height] {linear rgb, samples}.
//
// --math: arithmetic of the shading code (pt_set_math_mode).  fast (default) is what the reference's own build computes with —
// nvcc --use_fast_math, /root/reference/CMakeLists.txt:267 —, ieee the correctly rounded level of the CPU oracle.
//
// --gpus N renders on devices 0..N-1 of the node through ONE context (pt_create_multi): pixel tiles of
// sutil/WorkDistribution.h per device, one RCCL reduce of the accumulation per launch — the reference's dormant multi-GPU
// path, behind the same functions.  --save-accum / --restore-accum write and read the progressive state of the reference
// (params.accumulationBuffer + currentFrameIdx, pathTracerPrograms.cu:803-811): a restored run continues the running mean
// where the saved one stopped, bit for bit.
//
// --keys replays the reference's key handler (PathTracerMain.cpp:100-141) between frames, one key
// per frame: 0 = direct lighting, 1 = importance sampling, UP/DOWN = max depth +-1 in [1,28],
// R = reset, Q = quit; every change resets the accumulation and the frame index.
// --orbit / --zoom drive the camera through Trackball (sutil/Trackball.cpp:51-137: 0.5 degree per
// pixel, zoom factor 1.1 per step) before the first frame; the reference includes Trackball but never
// wires it to an input callback (PathTracerMain.cpp:18, 686-688).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/acgpt.h"
#include "Camera.h"
#include "Exception.h"
#include "ImageIO.h"
#include "OutputBuffer.h"
#include "TinyObjWrapper.h"
#include "Trackball.h"

using namespace acgpt;

constexpr unsigned int maxiumumRecursionDepth = 28;     // PathTracerMain.cpp:42
static int32_t samples_per_launch = 128;                // :43
static uint32_t frame_counter = 0, sample_summ = 0;
static double avg_ms = 0.0, total_ms = 0.0;
static bool refreshAccumulationBuffer = false;
static Camera g_camera;

struct PathTracerState {                                // :71-93
    pt_ctx* context = nullptr;
    pt_params params = {};
    int device = 0;
    int gpus = 1;                                       // > 1: one context over devices 0..gpus-1
    bool multi = false;                                 // --multi: the group context even for one device (its RCCL reduce then runs with one rank)
};

static bool keyCallback(PathTracerState& state, const std::string& key)   // :100-141; false = quit
{
    pt_params* params = &state.params;
    if (key == "Q" || key == "ESC") return false;
    if (key == "0") {
        params->useDirectLighting = !params->useDirectLighting;
        std::cout << std::endl << "Using Direct Lighting: " << (params->useDirectLighting ? "yes" : "no") << std::endl;
        refreshAccumulationBuffer = true;
    } else if (key == "1") {
        params->useImportanceSampling = !params->useImportanceSampling;
        std::cout << std::endl << "Using Importance Sampling: " << (params->useImportanceSampling ? "yes" : "no") << std::endl;
        refreshAccumulationBuffer = true;
    } else if (key == "UP") {
        params->maxDepth = std::min((int)maxiumumRecursionDepth, (int)params->maxDepth + 1);
        refreshAccumulationBuffer = true;
        std::cout << std::endl << "Max Depth: " << params->maxDepth << std::endl;
    } else if (key == "DOWN") {
        params->maxDepth = std::max(1, (int)params->maxDepth - 1);
        refreshAccumulationBuffer = true;
        std::cout << std::endl << "Max Depth: " << params->maxDepth << std::endl;
    } else if (key == "R") {
        refreshAccumulationBuffer = true;
    }
    return true;
}

static void allocAccumulation(PathTracerState& state)
{
    void* p = nullptr;
    PT_CHECK(state.context, pt_device_malloc(state.context, &p, (size_t)state.params.width * state.params.height * 4 * sizeof(float)));
    state.params.accumulationBuffer = (float*)p;
    // zero-filled: with pt_set_partition(rank, world) the pixels of other ranks are never written and the
    // cross-rank reduce(SUM) relies on them being 0 (the reference's single-GPU cudaMalloc leaves them undefined)
    PT_CHECK(state.context, pt_device_memset(state.context, p, 0, (size_t)state.params.width * state.params.height * 4 * sizeof(float)));
}

static void initializeTheLaunch(PathTracerState& state)                   // :143-164
{
    allocAccumulation(state);
    state.params.frameBuffer = nullptr;
    state.params.samplesPerPixel = samples_per_launch;
    state.params.currentFrameIdx = 0u;
    pt_area_light& al = state.params.areaLight;
    al.emission = {10.0f, 10.0f, 10.0f};
    al.corner = {343.0f, 547.0f, 227.0f};
    al.v1 = {0.0f, 0.0f, 105.0f};
    al.v2 = {-130.0f, 0.0f, 0.0f};
    const float3 n = normalize(cross(make_float3(al.v1.x, al.v1.y, al.v1.z), make_float3(al.v2.x, al.v2.y, al.v2.z)));
    al.normal = {n.x, n.y, n.z};
    state.params.handle = pt_scene_handle(state.context);
}

static void updateState(OutputBuffer<uchar4>&, PathTracerState& state)    // :166-182
{
    if (refreshAccumulationBuffer) {
        refreshAccumulationBuffer = false;
        state.params.currentFrameIdx = 0;
        sample_summ = 0; frame_counter = 0; avg_ms = 0; total_ms = 0;
        PT_CHECK(state.context, pt_device_free(state.context, state.params.accumulationBuffer));
        allocAccumulation(state);
    }
}

// sub_frames > 1 (--fuse-frames): that many consecutive launches of the reference's loop in one kernel launch
static void LaunchCurrentFrame(OutputBuffer<uchar4>& output_buffer, PathTracerState& state, uint32_t sub_frames = 1)   // :184-210
{
    uchar4* result_buffer_data = output_buffer.map();
    state.params.frameBuffer = reinterpret_cast<uint8_t*>(result_buffer_data);
    PT_CHECK(state.context, pt_launch_frames(state.context, &state.params, sub_frames));
    output_buffer.unmap();
}

static void initCamera()                                                 // :228-233
{
    g_camera.setEye(make_float3(278.0f, 273.0f, -900.0f));
    g_camera.setLookat(make_float3(278.0f, 273.0f, 330.0f));
    g_camera.setUp(make_float3(0.0f, 1.0f, 0.0f));
    g_camera.setFovY(35.0f);
}

static void createDeviceContext(PathTracerState& state)                  // :240-258
{
    if (state.gpus > 1 || state.multi) {
        // devices device, device + 1, ...; as a rehearsal on a one-GPU box (ACGPT_REHEARSE_SAME_GPU=1) every rank shares `device`
        const char* reh = getenv("ACGPT_REHEARSE_SAME_GPU");
        std::vector<int> ids((size_t)state.gpus);
        for (int i = 0; i < state.gpus; i++) ids[(size_t)i] = (reh && reh[0] == '1') ? state.device : state.device + i;
        if (pt_create_multi(&state.context, ids.data(), state.gpus) != 0) throw Exception(std::string("createDeviceContext: ") + pt_last_error(nullptr));
    } else if (pt_create(&state.context, state.device) != 0) throw Exception(std::string("createDeviceContext: ") + pt_last_error(nullptr));
    makeContextCurrent(state.context);      // OutputBuffer(type, w, h) allocates here, as CUDAOutputBuffer does on the current device
}

static void buildTheAccelarationStructure(PathTracerState& state, const TinyObjWrapper& objs)   // :260-398 (+ :544-627)
{
    std::vector<float> h_vertices = objs.getVerticesFloat();
    std::vector<uint32_t> h_mat_indices = objs.getMaterialIndices();
    std::vector<uint32_t> h_indxbuffer = objs.getIndexBuffer();
    std::vector<Material> materials = objs.getMaterials();
    PT_CHECK(state.context, pt_set_scene(state.context, h_vertices.data(), h_vertices.size() / 4, h_indxbuffer.data(), h_indxbuffer.size() / 3,
                                         h_mat_indices.data(), reinterpret_cast<const pt_material*>(materials.data()), materials.size()));
}

// The progressive state of the reference is the accumulation buffer and the frame index (pathTracerPrograms.cu:803-811).
// File: "ACGPTACC" | width | height | frames accumulated | float4[width * height]
static void saveAccumulation(PathTracerState& state, const std::string& path)
{
    const size_t n = (size_t)state.params.width * state.params.height * 4;
    std::vector<float> host(n);
    PT_CHECK(state.context, pt_copy_to_host(state.context, host.data(), state.params.accumulationBuffer, n * sizeof(float)));
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) throw Exception("cannot write " + path);
    const uint32_t hdr[3] = {state.params.width, state.params.height, state.params.currentFrameIdx};
    const bool ok = fwrite("ACGPTACC", 1, 8, f) == 8 && fwrite(hdr, 4, 3, f) == 3 && fwrite(host.data(), sizeof(float), n, f) == n;
    fclose(f);
    if (!ok) throw Exception("short write to " + path);
}
static void restoreAccumulation(PathTracerState& state, const std::string& path)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw Exception("cannot read " + path);
    char magic[8]; uint32_t hdr[3] = {0, 0, 0};
    const size_t n = (size_t)state.params.width * state.params.height * 4;
    std::vector<float> host(n);
    const bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, "ACGPTACC", 8) == 0 && fread(hdr, 4, 3, f) == 3 &&
                    hdr[0] == state.params.width && hdr[1] == state.params.height && fread(host.data(), sizeof(float), n, f) == n;
    fclose(f);
    if (!ok) throw Exception(path + ": not an accumulation dump of a " + std::to_string(state.params.width) + "x" + std::to_string(state.params.height) + " image");
    PT_CHECK(state.context, pt_copy_to_device(state.context, state.params.accumulationBuffer, host.data(), n * sizeof(float)));
    state.params.currentFrameIdx = hdr[2];
}

// :400-627 — nothing to JIT, link or bind here (the gfx950 code object is built ahead of time, materials travel with pt_set_scene);
// the functions stay so that main() reads, and prints, like the reference's
static void createModule(PathTracerState&) {}
static void createProgramGroups(PathTracerState&) {}
static void createPipeline(PathTracerState&) {}
static void createShaderBindingTable(PathTracerState&, const TinyObjWrapper&) {}

// --bloom: src (DEVICE float4[width * height], linear) through pt_bloom into dst.  bloom holds threshold, knee and clamp in display
// units: they are divided by the exposure, which is dp's manual one or is metered on src here (a pt_display_transform call whose
// frame buffer, fb, is discarded).  Returns the exposure; "" in err if all went well.
static float bloomForDisplay(PathTracerState& state, const float* src, const pt_display_params& dp, const pt_bloom_params& bloom, float* dst, void* fb,
                             pt_display_info& info, pt_bloom_info& bi, std::string& err)
{
    const size_t n = (size_t)state.params.width * state.params.height;
    memset(&info, 0, sizeof(info));
    info.exposure = dp.exposure;
    if (!(dp.exposure > 0.0f) && pt_display_transform(state.context, src, n, &dp, nullptr, (uint8_t*)fb, &info) != 0) { err = pt_last_error(state.context); return 0.0f; }
    pt_bloom_params bp = bloom;
    bp.threshold = bloom.threshold / info.exposure; bp.knee = bloom.knee / info.exposure; bp.clamp = bloom.clamp / info.exposure;
    if (pt_bloom(state.context, src, state.params.width, state.params.height, &bp, dst, &bi) != 0) err = pt_last_error(state.context);
    return info.exposure;
}

// src (DEVICE float4[width * height], linear) through pt_display_transform, written as an image (--tonemap, --exposure); with bloom,
// through pt_bloom first
static void saveDisplay(PathTracerState& state, const std::string& path, const float* src, const pt_display_params& dp, const pt_bloom_params* bloom = nullptr)
{
    const size_t n = (size_t)state.params.width * state.params.height;
    void* fb = nullptr;
    void* glared = nullptr;
    std::string err;
    pt_display_info info;
    pt_bloom_info bi;
    std::vector<uint8_t> host(n * 4);
    if (pt_device_malloc(state.context, &fb, n * 4) != 0) err = pt_last_error(state.context);
    if (err.empty() && bloom) {
        if (pt_device_malloc(state.context, &glared, n * 16) != 0) err = pt_last_error(state.context);
        pt_display_params manual = dp;
        if (err.empty()) manual.exposure = bloomForDisplay(state, src, dp, *bloom, (float*)glared, fb, info, bi, err);
        if (err.empty() && pt_display_transform(state.context, (const float*)glared, n, &manual, nullptr, (uint8_t*)fb, nullptr) != 0) err = pt_last_error(state.context);
    } else if (err.empty() && pt_display_transform(state.context, src, n, &dp, nullptr, (uint8_t*)fb, &info) != 0) {
        err = pt_last_error(state.context);
    }
    if (err.empty() && pt_copy_to_host(state.context, host.data(), fb, n * 4) != 0) err = pt_last_error(state.context);
    if (fb) pt_device_free(state.context, fb);
    if (glared) pt_device_free(state.context, glared);
    if (!err.empty()) throw Exception("display transform: " + err);
    if (bloom)
        std::cout << "Bloom: " << bi.levels << " levels, " << bi.bright_pixels << " bright, " << bi.invalid_pixels << " invalid; bright share "
                  << (bi.total_luma_q16 ? (double)bi.bright_luma_q16 / (double)bi.total_luma_q16 : 0.0) << ", max luminance " << bi.max_luma << std::endl;
    std::cout << "Display exposure: " << info.exposure << (dp.exposure > 0.0f ? " (manual)" : " (metered)") << std::endl;
    if (!saveImage(path, host.data(), (int)state.params.width, (int)state.params.height)) std::cerr << "could not write " << path << std::endl;
}

// the denoised preview of the current accumulation, written as an image next to the frame (--denoise); with a display transform
// (dp), that of the denoised image goes to display_path
static void saveDenoised(PathTracerState& state, const std::string& path, uint32_t iterations, const pt_display_params* dp = nullptr,
                         const std::string& display_path = std::string(), const float* image = nullptr, const pt_bloom_params* bloom = nullptr)
{
    auto params = state.params;                 // image (--firefly): denoise that instead of the accumulation
    if (image) params.accumulationBuffer = const_cast<float*>(image);
    const size_t n = (size_t)state.params.width * state.params.height;
    void* bufs[4] = {nullptr, nullptr, nullptr, nullptr};      // albedo_prim, normal_depth, denoised float4, colours uchar4
    std::string err;
    for (int i = 0; i < 4 && err.empty(); i++)
        if (pt_device_malloc(state.context, &bufs[i], n * (i < 3 ? 16 : 4)) != 0) err = pt_last_error(state.context);
    std::vector<uint8_t> host(n * 4);
    if (err.empty() && (pt_render_features(state.context, &state.params, (float*)bufs[0], (float*)bufs[1]) != 0 ||
                        pt_denoise(state.context, &params, (const float*)bufs[0], (const float*)bufs[1], (float*)bufs[2], iterations) != 0 ||
                        pt_resolve_framebuffer(state.context, (const float*)bufs[2], (uint8_t*)bufs[3], n) != 0 ||
                        pt_copy_to_host(state.context, host.data(), bufs[3], n * 4) != 0))
        err = pt_last_error(state.context);
    if (err.empty() && dp) {
        try { saveDisplay(state, display_path, (const float*)bufs[2], *dp, bloom); } catch (const std::exception& e) { err = e.what(); }
    }
    for (void* b : bufs) if (b) pt_device_free(state.context, b);
    if (!err.empty()) throw Exception("denoise: " + err);
    if (!saveImage(path, host.data(), (int)state.params.width, (int)state.params.height)) std::cerr << "could not write " << path << std::endl;
}

static std::string suffixedName(const std::string& out, const std::string& suffix)
{
    const size_t slash = out.find_last_of('/'), dot = out.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return out + suffix;
    return out.substr(0, dot) + suffix + out.substr(dot);
}
static std::string denoisedName(const std::string& out) { return suffixedName(out, "_denoised"); }

// ---- temporal history (--history-out, --history-in) -----------------------------------------------------------------------
struct HistoryFile {
    uint32_t hdr[8] = {};            // width, height, maxDepth, direct lighting, importance sampling, light mode (| material model << 8), math mode, triangles
    float camera[12] = {};           // eye, U, V, W
    std::vector<float> data;         // float4[width * height] {linear rgb, samples}
};
static const char kHistoryMagic[8] = {'A', 'C', 'G', 'P', 'T', 'H', 'S', 'T'};

// what a history of this run's view records about it
// (the material model is folded into bit 8 of the light-mode word: 0 for the reference's materials, so such files are as before)
static HistoryFile historyOfRun(PathTracerState& state, int light_mode, int math_mode, int material_model)
{
    pt_bvh_info bi;
    PT_CHECK(state.context, pt_get_bvh_info(state.context, &bi));
    const pt_params& p = state.params;
    HistoryFile h;
    const uint32_t hdr[8] = {p.width, p.height, p.maxDepth, (uint32_t)p.useDirectLighting, (uint32_t)p.useImportanceSampling, (uint32_t)light_mode | ((uint32_t)material_model << 8),
                             (uint32_t)math_mode, bi.n_tris};
    memcpy(h.hdr, hdr, sizeof(hdr));
    const pt_float3 cam[4] = {p.cameraEye, p.cameraU, p.cameraV, p.cameraW};
    for (int i = 0; i < 4; i++) { h.camera[3 * i] = cam[i].x; h.camera[3 * i + 1] = cam[i].y; h.camera[3 * i + 2] = cam[i].z; }
    return h;
}

static void writeHistory(const std::string& path, const HistoryFile& h)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) throw Exception("cannot write " + path);
    const bool ok = fwrite(kHistoryMagic, 1, 8, f) == 8 && fwrite(h.hdr, 4, 8, f) == 8 && fwrite(h.camera, 4, 12, f) == 12 &&
                    fwrite(h.data.data(), sizeof(float), h.data.size(), f) == h.data.size();
    fclose(f);
    if (!ok) throw Exception("short write to " + path);
}

static HistoryFile readHistory(const std::string& path)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw Exception("cannot read " + path);
    HistoryFile h;
    char magic[8];
    bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, kHistoryMagic, 8) == 0 && fread(h.hdr, 4, 8, f) == 8 && fread(h.camera, 4, 12, f) == 12 &&
              h.hdr[0] >= 1 && h.hdr[0] <= 65535 && h.hdr[1] >= 1 && h.hdr[1] <= 65535;
    if (ok) {
        h.data.resize((size_t)h.hdr[0] * h.hdr[1] * 4);
        ok = fread(h.data.data(), sizeof(float), h.data.size(), f) == h.data.size() && fgetc(f) == EOF;
    }
    fclose(f);
    if (!ok) throw Exception(path + ": not a history file (acgpt_main --history-out)");
    return h;
}

// "" if the history file was made under this run's scene and settings, else what differs
static std::string historyMismatch(const HistoryFile& file, const HistoryFile& run)
{
    static const char* names[8] = {"width", "height", "maxDepth", "direct lighting", "importance sampling", "light mode", "math mode", "triangles"};
    for (int i = 2; i < 8; i++)        // the size may differ: it is the previous view's
        if (file.hdr[i] != run.hdr[i])
            return std::string(names[i]) + " is " + std::to_string(file.hdr[i]) + " in the history, " + std::to_string(run.hdr[i]) + " in this run";
    return "";
}

// blends the history of the view in `file` into this run's view (pt_temporal_blend), writes <out>_temporal (and _temporal_denoised);
// the blended history comes back in `blended`
static void blendHistory(PathTracerState& state, const HistoryFile& file, const std::string& out, uint32_t denoise_iters, std::vector<float>& blended)
{
    const pt_params& p = state.params;
    const size_t n = (size_t)p.width * p.height, n_prev = (size_t)file.hdr[0] * file.hdr[1];
    pt_params prev = p;
    prev.width = file.hdr[0]; prev.height = file.hdr[1];
    pt_float3* cam[4] = {&prev.cameraEye, &prev.cameraU, &prev.cameraV, &prev.cameraW};
    for (int i = 0; i < 4; i++) *cam[i] = {file.camera[3 * i], file.camera[3 * i + 1], file.camera[3 * i + 2]};
    // prev history, prev albedo_prim, prev normal_depth, albedo_prim, normal_depth, blended history, denoised (float4), colours (uchar4)
    const size_t sizes[8] = {n_prev * 16, n_prev * 16, n_prev * 16, n * 16, n * 16, n * 16, n * 16, n * 4};
    void* b[8] = {};
    std::string err;
    for (int i = 0; i < 8 && err.empty(); i++)
        if (pt_device_malloc(state.context, &b[i], sizes[i]) != 0) err = pt_last_error(state.context);
    std::vector<uint8_t> host(n * 4), host_dn(n * 4);
    blended.assign(n * 4, 0.0f);
    pt_params dn = p;
    dn.accumulationBuffer = (float*)b[5];                         // pt_denoise reads the blend's .xyz
    const uint32_t samples = p.currentFrameIdx * p.samplesPerPixel;
    if (err.empty() && (pt_copy_to_device(state.context, b[0], file.data.data(), sizes[0]) != 0 ||
                        pt_render_features(state.context, &prev, (float*)b[1], (float*)b[2]) != 0 ||
                        pt_render_features(state.context, &p, (float*)b[3], (float*)b[4]) != 0 ||
                        pt_temporal_blend(state.context, &p, samples, (const float*)b[3], (const float*)b[4], &prev, (const float*)b[0],
                                          (const float*)b[1], (const float*)b[2], PT_TEMPORAL_HISTORY_CAP, (float*)b[5]) != 0 ||
                        pt_copy_to_host(state.context, blended.data(), b[5], n * 16) != 0 ||
                        pt_resolve_framebuffer(state.context, (const float*)b[5], (uint8_t*)b[7], n) != 0 ||
                        pt_copy_to_host(state.context, host.data(), b[7], n * 4) != 0))
        err = pt_last_error(state.context);
    if (err.empty() && denoise_iters > 0 &&
        (pt_denoise(state.context, &dn, (const float*)b[3], (const float*)b[4], (float*)b[6], denoise_iters) != 0 ||
         pt_resolve_framebuffer(state.context, (const float*)b[6], (uint8_t*)b[7], n) != 0 ||
         pt_copy_to_host(state.context, host_dn.data(), b[7], n * 4) != 0))
        err = pt_last_error(state.context);
    for (void* x : b) if (x) pt_device_free(state.context, x);
    if (!err.empty()) throw Exception("temporal blend: " + err);
    const std::string name = suffixedName(out, "_temporal");
    if (!saveImage(name, host.data(), (int)p.width, (int)p.height)) std::cerr << "could not write " << name << std::endl;
    if (denoise_iters > 0) {
        const std::string dname = suffixedName(out, "_temporal_denoised");
        if (!saveImage(dname, host_dn.data(), (int)p.width, (int)p.height)) std::cerr << "could not write " << dname << std::endl;
    }
}

// --move-history: the view before the refit (accumulation as {rgb, frames * spp}, features), carried into the moved scene after it
struct MovedHistory {
    PathTracerState* state = nullptr;
    pt_params prev = {};
    void* b[3] = {nullptr, nullptr, nullptr};       // history, albedo_prim, normal_depth of the view before the move

    void keep(PathTracerState& s)
    {
        state = &s;
        prev = s.params;
        const size_t n = (size_t)prev.width * prev.height;
        for (int i = 0; i < 3; i++) PT_CHECK(s.context, pt_device_malloc(s.context, &b[i], n * 16));
        std::vector<float> host(n * 4);
        PT_CHECK(s.context, pt_copy_to_host(s.context, host.data(), prev.accumulationBuffer, n * 16));
        const float samples = (float)(prev.currentFrameIdx * prev.samplesPerPixel);
        for (size_t i = 3; i < host.size(); i += 4) host[i] = samples;
        PT_CHECK(s.context, pt_copy_to_device(s.context, b[0], host.data(), n * 16));
        PT_CHECK(s.context, pt_render_features(s.context, &prev, (float*)b[1], (float*)b[2]));
    }

    // writes <out>_moved_temporal (and _moved_temporal_denoised); `before` / `after`: the vertices of the two views
    void blend(PathTracerState& s, const std::vector<float>& before, const std::vector<float>& after, const std::string& out, uint32_t denoise_iters)
    {
        const pt_params& p = s.params;
        const size_t n = (size_t)p.width * p.height, vbytes = before.size() * sizeof(float);
        // albedo_prim, normal_depth, blended history, denoised (float4), colours (uchar4), vertices now, vertices before
        const size_t sizes[7] = {n * 16, n * 16, n * 16, n * 16, n * 4, vbytes, vbytes};
        void* d[7] = {};
        std::string err;
        for (int i = 0; i < 7 && err.empty(); i++)
            if (pt_device_malloc(s.context, &d[i], sizes[i]) != 0) err = pt_last_error(s.context);
        std::vector<uint8_t> host(n * 4), host_dn(n * 4);
        pt_params dn = p;
        dn.accumulationBuffer = (float*)d[2];                         // pt_denoise reads the blend's .xyz
        if (err.empty() && (pt_copy_to_device(s.context, d[5], after.data(), vbytes) != 0 ||
                            pt_copy_to_device(s.context, d[6], before.data(), vbytes) != 0 ||
                            pt_render_features(s.context, &p, (float*)d[0], (float*)d[1]) != 0 ||
                            pt_temporal_blend_motion(s.context, &p, p.currentFrameIdx * p.samplesPerPixel, (const float*)d[0], (const float*)d[1],
                                                     &prev, (const float*)b[0], (const float*)b[1], (const float*)b[2], (const float*)d[5],
                                                     (const float*)d[6], before.size() / 4, PT_TEMPORAL_HISTORY_CAP, PT_TEMPORAL_CLIP_GAMMA,
                                                     (float*)d[2]) != 0 ||
                            pt_resolve_framebuffer(s.context, (const float*)d[2], (uint8_t*)d[4], n) != 0 ||
                            pt_copy_to_host(s.context, host.data(), d[4], n * 4) != 0))
            err = pt_last_error(s.context);
        if (err.empty() && denoise_iters > 0 &&
            (pt_denoise(s.context, &dn, (const float*)d[0], (const float*)d[1], (float*)d[3], denoise_iters) != 0 ||
             pt_resolve_framebuffer(s.context, (const float*)d[3], (uint8_t*)d[4], n) != 0 ||
             pt_copy_to_host(s.context, host_dn.data(), d[4], n * 4) != 0))
            err = pt_last_error(s.context);
        for (void* x : d) if (x) pt_device_free(s.context, x);
        if (!err.empty()) throw Exception("moved temporal blend: " + err);
        const std::string name = suffixedName(out, "_moved_temporal");
        if (!saveImage(name, host.data(), (int)p.width, (int)p.height)) std::cerr << "could not write " << name << std::endl;
        if (denoise_iters > 0) {
            const std::string dname = suffixedName(out, "_moved_temporal_denoised");
            if (!saveImage(dname, host_dn.data(), (int)p.width, (int)p.height)) std::cerr << "could not write " << dname << std::endl;
        }
    }

    ~MovedHistory()
    {
        if (state && state->context)
            for (void* x : b) if (x) pt_device_free(state->context, x);
    }
};

// --set-material name:field,field,...: applies one spec to `mats` (indexed as `names`); false + why on an unknown name or a bad field
static bool applyMaterialEdit(const std::string& spec, const std::vector<std::string>& names, std::vector<Material>& mats, std::string& why)
{
    const size_t colon = spec.rfind(':');
    if (colon == std::string::npos || colon == 0 || colon + 1 == spec.size()) {
        why = "expected name:kd=r,g,b[,ke=r,g,b][,bsdf=diffuse|metal|glass][,ior=x], got '" + spec + "'";
        return false;
    }
    const std::string name = spec.substr(0, colon);
    const size_t id = (size_t)(std::find(names.begin(), names.end(), name) - names.begin());
    if (id == names.size()) { why = "no material named '" + name + "'"; return false; }
    Material m = mats[id];
    const char* p = spec.c_str() + colon + 1;
    std::vector<std::string> seen;
    // n finite floats separated by commas, from p on
    auto floats = [&](float* out, int n) -> bool {
        for (int k = 0; k < n; k++) {
            if (k > 0) { if (*p != ',') return false; ++p; }
            char* end = nullptr;
            out[k] = strtof(p, &end);
            if (end == p || !std::isfinite(out[k])) return false;
            p = end;
        }
        return true;
    };
    while (true) {
        const char* eq = strchr(p, '=');
        if (!eq) { why = "field without '=' in '" + spec + "'"; return false; }
        const std::string key(p, eq);
        if (std::find(seen.begin(), seen.end(), key) != seen.end()) { why = "field '" + key + "' given twice in '" + spec + "'"; return false; }
        seen.push_back(key);
        p = eq + 1;
        float v[3];
        if (key == "kd" || key == "ke") {
            if (!floats(v, 3)) { why = "'" + key + "' takes three finite numbers r,g,b in '" + spec + "'"; return false; }
            (key == "kd" ? m.diffuse : m.emission) = make_float3(v[0], v[1], v[2]);
        } else if (key == "ior") {
            if (!floats(v, 1)) { why = "'ior' takes one finite number in '" + spec + "'"; return false; }
            m.ior = v[0];
        } else if (key == "bsdf") {
            const char* end = strchr(p, ',');
            const std::string b = end ? std::string(p, end) : std::string(p);
            if (b == "diffuse") m.bsdfType = BSDF_DIFFUSE;
            else if (b == "metal") m.bsdfType = BSDF_METALLIC;
            else if (b == "glass") m.bsdfType = BSDF_REFRACTION;
            else { why = "'bsdf' is diffuse, metal or glass, not '" + b + "'"; return false; }
            p += b.size();
        } else {
            why = "unknown field '" + key + "' (kd, ke, bsdf, ior)";
            return false;
        }
        if (*p == '\0') break;
        if (*p != ',') { why = "unexpected '" + std::string(p) + "' in '" + spec + "'"; return false; }
        ++p;
    }
    mats[id] = m;
    return true;
}

// --pick: the camera ray through the centre of each pixel (the direction of pixel_centre_dir, csrc/image_common.h, restated: the same
// fp32 operations), traced by pt_query_closest in one call; one JSON line per pick
static void pickPixels(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<int2>& picks)
{
    const pt_params& p = state.params;
    const size_t n = picks.size();
    std::vector<float> rays(n * 8);
    const float3 eye = make_float3(p.cameraEye.x, p.cameraEye.y, p.cameraEye.z);
    const float3 U = make_float3(p.cameraU.x, p.cameraU.y, p.cameraU.z), V = make_float3(p.cameraV.x, p.cameraV.y, p.cameraV.z),
                 W = make_float3(p.cameraW.x, p.cameraW.y, p.cameraW.z);
    for (size_t i = 0; i < n; i++) {
        const float dx = 2.0f * (((float)picks[i].x + 0.5f) / (float)p.width) - 1.0f;
        const float dy = 2.0f * (((float)picks[i].y + 0.5f) / (float)p.height) - 1.0f;
        const float3 dir = normalize(dx * U + dy * V + W);
        const float r[8] = {eye.x, eye.y, eye.z, dir.x, dir.y, dir.z, 0.01f, 1e16f};      // pt_render_features' interval
        memcpy(&rays[8 * i], r, sizeof(r));
    }
    void* d_rays = nullptr; void* d_hits = nullptr;
    std::vector<pt_hit> hits(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_rays, n * 32) != 0 || pt_device_malloc(state.context, &d_hits, n * sizeof(pt_hit)) != 0 ||
        pt_copy_to_device(state.context, d_rays, rays.data(), n * 32) != 0 ||
        pt_query_closest(state.context, (const float*)d_rays, n, (pt_hit*)d_hits) != 0 ||
        pt_copy_to_host(state.context, hits.data(), d_hits, n * sizeof(pt_hit)) != 0)
        err = pt_last_error(state.context);
    if (d_rays) pt_device_free(state.context, d_rays);
    if (d_hits) pt_device_free(state.context, d_hits);
    if (!err.empty()) throw Exception("pick: " + err);
    const std::vector<std::string>& names = obj.getMaterialNames();
    for (size_t i = 0; i < n; i++) {
        const pt_hit& h = hits[i];
        if (h.prim == 0xFFFFFFFFu) { printf("{\"pick\": [%d, %d], \"hit\": false}\n", picks[i].x, picks[i].y); continue; }
        const float* r = &rays[8 * i];
        std::string name = h.material < names.size() ? names[h.material] : std::string();
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        printf("{\"pick\": [%d, %d], \"hit\": true, \"t\": %.9g, \"prim\": %u, \"material\": \"%s\", \"position\": [%.9g, %.9g, %.9g], \"normal\": [%.9g, %.9g, %.9g]}\n",
               picks[i].x, picks[i].y, h.t, h.prim, name.c_str(), r[0] + h.t * r[3], r[1] + h.t * r[4], r[2] + h.t * r[5], h.nx, h.ny, h.nz);
    }
    fflush(stdout);
}

// --pick-all: --pick's rays through pt_query_multi in one call, at the largest k asked for; one JSON line per pixel with its own k
struct PickAll { int x, y, k; };
static void pickAllPixels(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<PickAll>& picks)
{
    const pt_params& p = state.params;
    const size_t n = picks.size();
    uint32_t kmax = 1;
    std::vector<float> rays(n * 8);
    const float3 eye = make_float3(p.cameraEye.x, p.cameraEye.y, p.cameraEye.z);
    const float3 U = make_float3(p.cameraU.x, p.cameraU.y, p.cameraU.z), V = make_float3(p.cameraV.x, p.cameraV.y, p.cameraV.z),
                 W = make_float3(p.cameraW.x, p.cameraW.y, p.cameraW.z);
    for (size_t i = 0; i < n; i++) {
        const float dx = 2.0f * (((float)picks[i].x + 0.5f) / (float)p.width) - 1.0f;
        const float dy = 2.0f * (((float)picks[i].y + 0.5f) / (float)p.height) - 1.0f;
        const float3 dir = normalize(dx * U + dy * V + W);
        const float r[8] = {eye.x, eye.y, eye.z, dir.x, dir.y, dir.z, 0.01f, 1e16f};      // pickPixels' ray
        memcpy(&rays[8 * i], r, sizeof(r));
        if ((uint32_t)picks[i].k > kmax) kmax = (uint32_t)picks[i].k;
    }
    void* d_rays = nullptr; void* d_hits = nullptr; void* d_counts = nullptr;
    std::vector<pt_hit> hits(n * kmax);
    std::vector<uint32_t> counts(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_rays, n * 32) != 0 || pt_device_malloc(state.context, &d_hits, hits.size() * sizeof(pt_hit)) != 0 ||
        pt_device_malloc(state.context, &d_counts, n * 4) != 0 ||
        pt_copy_to_device(state.context, d_rays, rays.data(), n * 32) != 0 ||
        pt_query_multi(state.context, (const float*)d_rays, n, kmax, (pt_hit*)d_hits, (uint32_t*)d_counts) != 0 ||
        pt_copy_to_host(state.context, hits.data(), d_hits, hits.size() * sizeof(pt_hit)) != 0 ||
        pt_copy_to_host(state.context, counts.data(), d_counts, n * 4) != 0)
        err = pt_last_error(state.context);
    if (d_rays) pt_device_free(state.context, d_rays);
    if (d_hits) pt_device_free(state.context, d_hits);
    if (d_counts) pt_device_free(state.context, d_counts);
    if (!err.empty()) throw Exception("pick-all: " + err);
    const std::vector<std::string>& names = obj.getMaterialNames();
    for (size_t i = 0; i < n; i++) {
        const float* r = &rays[8 * i];
        printf("{\"pick_all\": [%d, %d], \"count\": %u, \"hits\": [", picks[i].x, picks[i].y, counts[i]);
        for (int j = 0; j < picks[i].k; j++) {
            const pt_hit& h = hits[i * kmax + (size_t)j];
            if (h.prim == 0xFFFFFFFFu) break;
            std::string name = h.material < names.size() ? names[h.material] : std::string();
            for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
            printf("%s{\"t\": %.9g, \"prim\": %u, \"material\": \"%s\", \"position\": [%.9g, %.9g, %.9g], \"normal\": [%.9g, %.9g, %.9g]}", j ? ", " : "",
                   h.t, h.prim, name.c_str(), r[0] + h.t * r[3], r[1] + h.t * r[4], r[2] + h.t * r[5], h.nx, h.ny, h.nz);
        }
        printf("]}\n");
    }
    fflush(stdout);
}

// The complete lists of m records of rec_bytes each, for --overlap / --intersect with "all": the counts, pt_list_offsets, the
// allocation, the fill.  Returns the error, or an empty string with offsets (m + 1) and prims (offsets[m]) filled.
static const uint32_t kListAll = 9u;      // the k that stands for "all"
static bool wantsAll(std::string& text)
{
    if (text.size() < 4 || text.compare(text.size() - 4, 4, ",all") != 0) return false;
    text.resize(text.size() - 4);
    return true;
}
static std::string completeLists(PathTracerState& state, const std::vector<float>& recs, size_t m, size_t rec_bytes,
                                 int (*count)(pt_ctx*, const float*, size_t, uint32_t, uint32_t*, uint32_t*),
                                 int (*fill)(pt_ctx*, const float*, size_t, const uint32_t*, uint32_t*, size_t, uint32_t*),
                                 std::vector<uint32_t>& offsets, std::vector<uint32_t>& prims)
{
    void* d_recs = nullptr; void* d_counts = nullptr; void* d_offsets = nullptr; void* d_prims = nullptr;
    uint64_t total = 0;
    offsets.assign(m + 1, 0u);
    std::string err;
    if (pt_device_malloc(state.context, &d_recs, m * rec_bytes) != 0 || pt_device_malloc(state.context, &d_counts, m * 4) != 0 ||
        pt_device_malloc(state.context, &d_offsets, (m + 1) * 4) != 0 || pt_copy_to_device(state.context, d_recs, recs.data(), m * rec_bytes) != 0 ||
        count(state.context, (const float*)d_recs, m, 0u, nullptr, (uint32_t*)d_counts) != 0 ||
        pt_list_offsets(state.context, (const uint32_t*)d_counts, m, (uint32_t*)d_offsets, &total) != 0 ||
        pt_copy_to_host(state.context, offsets.data(), d_offsets, (m + 1) * 4) != 0)
        err = pt_last_error(state.context);
    prims.assign(err.empty() ? (size_t)total : 0u, 0xFFFFFFFFu);
    if (err.empty() &&
        ((total != 0 && pt_device_malloc(state.context, &d_prims, (size_t)total * 4) != 0) ||
         fill(state.context, (const float*)d_recs, m, (const uint32_t*)d_offsets, (uint32_t*)d_prims, (size_t)total, nullptr) != 0 ||
         (total != 0 && pt_copy_to_host(state.context, prims.data(), d_prims, (size_t)total * 4) != 0)))
        err = pt_last_error(state.context);
    if (d_recs) pt_device_free(state.context, d_recs);
    if (d_counts) pt_device_free(state.context, d_counts);
    if (d_offsets) pt_device_free(state.context, d_offsets);
    if (d_prims) pt_device_free(state.context, d_prims);
    return err;
}

// --overlap: the boxes of one k in one call of pt_query_overlap; one JSON line per box, in the order given.  --overlap-oriented: the
// same through pt_query_overlap_oriented and pt_query_overlap_oriented_lists on records of 16 floats; the line names the ten numbers
// of the argument, the quaternion as it was normalised.
struct OverlapBox { float v[16]; uint32_t k; double arg[10]; };
static void overlapBoxes(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<OverlapBox>& boxes, bool oriented = false)
{
    const size_t n = boxes.size();
    const size_t W = oriented ? 16 : 8, B = 4 * W;      // floats and bytes of a record
    const char* what = oriented ? "overlap-oriented: " : "overlap: ";
    std::vector<uint32_t> counts(n, 0u), prims(n * 8, 0xFFFFFFFFu);
    for (uint32_t k = 0; k <= 8u; k++) {
        std::vector<size_t> which;
        std::vector<float> recs;
        for (size_t i = 0; i < n; i++)
            if (boxes[i].k == k) { which.push_back(i); recs.insert(recs.end(), boxes[i].v, boxes[i].v + W); }
        const size_t m = which.size();
        if (m == 0) continue;
        void* d_boxes = nullptr; void* d_prims = nullptr; void* d_counts = nullptr;
        std::vector<uint32_t> c(m), p(m * (k ? k : 1u));
        std::string err;
        if (pt_device_malloc(state.context, &d_boxes, m * B) != 0 || pt_device_malloc(state.context, &d_counts, m * 4) != 0 ||
            (k != 0 && pt_device_malloc(state.context, &d_prims, m * k * 4) != 0) ||
            pt_copy_to_device(state.context, d_boxes, recs.data(), m * B) != 0 ||
            (oriented ? pt_query_overlap_oriented : pt_query_overlap)(state.context, (const float*)d_boxes, m, k, (uint32_t*)d_prims, (uint32_t*)d_counts) != 0 ||
            pt_copy_to_host(state.context, c.data(), d_counts, m * 4) != 0 ||
            (k != 0 && pt_copy_to_host(state.context, p.data(), d_prims, m * k * 4) != 0))
            err = pt_last_error(state.context);
        if (d_boxes) pt_device_free(state.context, d_boxes);
        if (d_prims) pt_device_free(state.context, d_prims);
        if (d_counts) pt_device_free(state.context, d_counts);
        if (!err.empty()) throw Exception(what + err);
        for (size_t j = 0; j < m; j++) {
            counts[which[j]] = c[j];
            for (uint32_t e = 0; e < k; e++) prims[which[j] * 8 + e] = p[j * k + e];
        }
    }
    // the boxes that ask for every triangle: their complete lists, box by box
    std::vector<std::vector<uint32_t> > whole(n);
    {
        std::vector<size_t> which;
        std::vector<float> recs;
        for (size_t i = 0; i < n; i++)
            if (boxes[i].k == kListAll) { which.push_back(i); recs.insert(recs.end(), boxes[i].v, boxes[i].v + W); }
        if (!which.empty()) {
            std::vector<uint32_t> offsets, all;
            const std::string err = completeLists(state, recs, which.size(), B, oriented ? pt_query_overlap_oriented : pt_query_overlap,
                                                  oriented ? pt_query_overlap_oriented_lists : pt_query_overlap_lists, offsets, all);
            if (!err.empty()) throw Exception(what + err);
            for (size_t j = 0; j < which.size(); j++) {
                whole[which[j]].assign(all.begin() + offsets[j], all.begin() + offsets[j + 1]);
                counts[which[j]] = offsets[j + 1] - offsets[j];
            }
        }
    }
    const std::vector<std::string>& names = obj.getMaterialNames();
    const std::vector<uint32_t> mats = obj.getMaterialIndices();
    for (size_t i = 0; i < n; i++) {
        const float* b = boxes[i].v;
        if (oriented) {
            const double* q = boxes[i].arg;
            printf("{\"overlap_oriented\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.17g, %.17g, %.17g, %.17g], \"count\": %u, \"triangles\": [", q[0], q[1], q[2], q[3],
                   q[4], q[5], q[6], q[7], q[8], q[9], counts[i]);
        } else
            printf("{\"overlap\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"count\": %u, \"triangles\": [", b[0], b[1], b[2], b[3], b[4], b[5], counts[i]);
        std::string mat_list;
        bool first = true;
        const bool all = boxes[i].k == kListAll;
        for (uint32_t e = 0; e < (all ? (uint32_t)whole[i].size() : boxes[i].k); e++) {
            const uint32_t t = all ? whole[i][e] : prims[i * 8 + e];
            if (t == 0xFFFFFFFFu) break;
            const uint32_t id = t < mats.size() ? mats[t] : 0xFFFFFFFFu;
            std::string name = id < names.size() ? names[id] : std::string();
            for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
            printf("%s%u", first ? "" : ", ", t);
            mat_list += std::string(first ? "" : ", ") + "\"" + name + "\"";
            first = false;
        }
        printf("], \"materials\": [%s]}\n", mat_list.c_str());
    }
    fflush(stdout);
}

// --intersect: the triangles of one k in one call of pt_query_triangles; one JSON line per triangle, in the order given
struct IntersectTri { float v[12]; uint32_t k; };
static void intersectTriangles(PathTracerState& state, const std::vector<IntersectTri>& tris)
{
    const size_t n = tris.size();
    std::vector<uint32_t> counts(n, 0u), prims(n * 8, 0xFFFFFFFFu);
    for (uint32_t k = 0; k <= 8u; k++) {
        std::vector<size_t> which;
        std::vector<float> recs;
        for (size_t i = 0; i < n; i++)
            if (tris[i].k == k) { which.push_back(i); recs.insert(recs.end(), tris[i].v, tris[i].v + 12); }
        const size_t m = which.size();
        if (m == 0) continue;
        void* d_tris = nullptr; void* d_prims = nullptr; void* d_counts = nullptr;
        std::vector<uint32_t> c(m), p(m * (k ? k : 1u));
        std::string err;
        if (pt_device_malloc(state.context, &d_tris, m * 48) != 0 || pt_device_malloc(state.context, &d_counts, m * 4) != 0 ||
            (k != 0 && pt_device_malloc(state.context, &d_prims, m * k * 4) != 0) ||
            pt_copy_to_device(state.context, d_tris, recs.data(), m * 48) != 0 ||
            pt_query_triangles(state.context, (const float*)d_tris, m, k, (uint32_t*)d_prims, (uint32_t*)d_counts) != 0 ||
            pt_copy_to_host(state.context, c.data(), d_counts, m * 4) != 0 ||
            (k != 0 && pt_copy_to_host(state.context, p.data(), d_prims, m * k * 4) != 0))
            err = pt_last_error(state.context);
        if (d_tris) pt_device_free(state.context, d_tris);
        if (d_prims) pt_device_free(state.context, d_prims);
        if (d_counts) pt_device_free(state.context, d_counts);
        if (!err.empty()) throw Exception("intersect: " + err);
        for (size_t j = 0; j < m; j++) {
            counts[which[j]] = c[j];
            for (uint32_t e = 0; e < k; e++) prims[which[j] * 8 + e] = p[j * k + e];
        }
    }
    // the triangles that ask for every scene triangle: their complete lists
    std::vector<std::vector<uint32_t> > whole(n);
    {
        std::vector<size_t> which;
        std::vector<float> recs;
        for (size_t i = 0; i < n; i++)
            if (tris[i].k == kListAll) { which.push_back(i); recs.insert(recs.end(), tris[i].v, tris[i].v + 12); }
        if (!which.empty()) {
            std::vector<uint32_t> offsets, all;
            const std::string err = completeLists(state, recs, which.size(), 48, pt_query_triangles, pt_query_triangles_lists, offsets, all);
            if (!err.empty()) throw Exception("intersect: " + err);
            for (size_t j = 0; j < which.size(); j++) {
                whole[which[j]].assign(all.begin() + offsets[j], all.begin() + offsets[j + 1]);
                counts[which[j]] = offsets[j + 1] - offsets[j];
            }
        }
    }
    for (size_t i = 0; i < n; i++) {
        const float* a = tris[i].v;
        printf("{\"intersect\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"count\": %u, \"triangles\": [", a[0], a[1], a[2], a[4], a[5], a[6], a[8],
               a[9], a[10], counts[i]);
        if (tris[i].k == kListAll)
            for (size_t e = 0; e < whole[i].size(); e++) printf("%s%u", e ? ", " : "", whole[i][e]);
        else
            for (uint32_t e = 0; e < tris[i].k && prims[i * 8 + e] != 0xFFFFFFFFu; e++) printf("%s%u", e ? ", " : "", prims[i * 8 + e]);
        printf("]}\n");
    }
    fflush(stdout);
}

// --sweep: every sweep in one call of pt_query_sweep; one JSON line per sweep
struct SweepArg { float v[8]; };
static void sweepSpheres(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<SweepArg>& sweeps)
{
    const size_t n = sweeps.size();
    void* d_sweeps = nullptr; void* d_out = nullptr;
    std::vector<pt_sweep_hit> out(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_sweeps, n * 32) != 0 || pt_device_malloc(state.context, &d_out, n * sizeof(pt_sweep_hit)) != 0 ||
        pt_copy_to_device(state.context, d_sweeps, sweeps.data(), n * 32) != 0 ||
        pt_query_sweep(state.context, (const float*)d_sweeps, n, (pt_sweep_hit*)d_out) != 0 ||
        pt_copy_to_host(state.context, out.data(), d_out, n * sizeof(pt_sweep_hit)) != 0)
        err = pt_last_error(state.context);
    if (d_sweeps) pt_device_free(state.context, d_sweeps);
    if (d_out) pt_device_free(state.context, d_out);
    if (!err.empty()) throw Exception("sweep: " + err);
    const std::vector<std::string>& names = obj.getMaterialNames();
    for (size_t i = 0; i < n; i++) {
        const pt_sweep_hit& r = out[i];
        const float* q = sweeps[i].v;
        printf("{\"sweep\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"tmax\": ", q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
        if (std::isfinite(q[7])) printf("%.9g", q[7]); else printf("null");
        if (r.prim == 0xFFFFFFFFu) { printf(", \"hit\": false}\n"); continue; }
        std::string name = r.material < names.size() ? names[r.material] : std::string();
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        printf(", \"hit\": true, \"t\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"point\": [%.9g, %.9g, %.9g], \"u\": %.9g, \"v\": %.9g}\n",
               r.t, r.prim, name.c_str(), r.cx, r.cy, r.cz, r.u, r.v);
    }
    fflush(stdout);
}

// --capsule-cast: every capsule in one call of pt_query_capsule_cast; one JSON line per cast
struct CapsuleCastArg { float v[12]; };
static void castCapsules(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<CapsuleCastArg>& casts)
{
    const size_t n = casts.size();
    void* d_casts = nullptr; void* d_out = nullptr;
    std::vector<pt_capsule_cast_hit> out(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_casts, n * 48) != 0 || pt_device_malloc(state.context, &d_out, n * sizeof(pt_capsule_cast_hit)) != 0 ||
        pt_copy_to_device(state.context, d_casts, casts.data(), n * 48) != 0 ||
        pt_query_capsule_cast(state.context, (const float*)d_casts, n, (pt_capsule_cast_hit*)d_out) != 0 ||
        pt_copy_to_host(state.context, out.data(), d_out, n * sizeof(pt_capsule_cast_hit)) != 0)
        err = pt_last_error(state.context);
    if (d_casts) pt_device_free(state.context, d_casts);
    if (d_out) pt_device_free(state.context, d_out);
    if (!err.empty()) throw Exception("capsule-cast: " + err);
    const std::vector<std::string>& names = obj.getMaterialNames();
    for (size_t i = 0; i < n; i++) {
        const pt_capsule_cast_hit& r = out[i];
        const float* q = casts[i].v;
        printf("{\"capsule_cast\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"tmax\": ", q[0], q[1], q[2], q[4], q[5], q[6], q[8], q[9], q[10], q[3]);
        if (std::isfinite(q[7])) printf("%.9g", q[7]); else printf("null");
        if (r.prim == 0xFFFFFFFFu) { printf(", \"hit\": false}\n"); continue; }
        std::string name = r.material < names.size() ? names[r.material] : std::string();
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        printf(", \"hit\": true, \"t\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"point\": [%.9g, %.9g, %.9g], \"s\": %.9g, \"feature\": %d}\n",
               r.t, r.prim, name.c_str(), r.cx, r.cy, r.cz, r.s, (int)r.feature);
    }
    fflush(stdout);
}

// --box-cast: every oriented box in one call of pt_query_box_cast; one JSON line per cast.  in: the thirteen numbers as given
struct BoxCastArg { float v[20]; float in[13]; };
static void castBoxes(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<BoxCastArg>& casts)
{
    const size_t n = casts.size();
    std::vector<float> recs(n * 20);
    for (size_t i = 0; i < n; i++) for (int j = 0; j < 20; j++) recs[i * 20 + j] = casts[i].v[j];
    void* d_casts = nullptr; void* d_out = nullptr;
    std::vector<pt_box_cast_hit> out(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_casts, n * 80) != 0 || pt_device_malloc(state.context, &d_out, n * sizeof(pt_box_cast_hit)) != 0 ||
        pt_copy_to_device(state.context, d_casts, recs.data(), n * 80) != 0 ||
        pt_query_box_cast(state.context, (const float*)d_casts, n, (pt_box_cast_hit*)d_out) != 0 ||
        pt_copy_to_host(state.context, out.data(), d_out, n * sizeof(pt_box_cast_hit)) != 0)
        err = pt_last_error(state.context);
    if (d_casts) pt_device_free(state.context, d_casts);
    if (d_out) pt_device_free(state.context, d_out);
    if (!err.empty()) throw Exception("box-cast: " + err);
    const std::vector<std::string>& names = obj.getMaterialNames();
    for (size_t i = 0; i < n; i++) {
        const pt_box_cast_hit& r = out[i];
        const float* q = casts[i].in;
        printf("{\"box_cast\": [");
        for (int j = 0; j < 13; j++) printf(j ? ", %.9g" : "%.9g", q[j]);
        printf("], \"tmax\": ");
        if (std::isfinite(casts[i].v[19])) printf("%.9g", casts[i].v[19]); else printf("null");
        if (r.prim == 0xFFFFFFFFu) { printf(", \"hit\": false}\n"); continue; }
        std::string name = r.material < names.size() ? names[r.material] : std::string();
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        printf(", \"hit\": true, \"t\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"feature\": %d, \"normal\": [%.9g, %.9g, %.9g], \"point\": [%.9g, %.9g, %.9g]}\n",
               r.t, r.prim, name.c_str(), (int)r.feature, r.nx, r.ny, r.nz, r.cx, r.cy, r.cz);
    }
    fflush(stdout);
}

// --cast: every translating triangle in one call of pt_query_triangle_cast; one JSON line per cast
struct CastArg { float v[16]; };
static void printCastHit(const pt_triangle_cast_hit& r, const std::vector<std::string>& names, bool posed)
{
    if (r.prim == 0xFFFFFFFFu) { printf(", \"hit\": false}\n"); return; }
    std::string name = r.material < names.size() ? names[r.material] : std::string();
    for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
    printf(", \"hit\": true, \"t\": %.9g, \"triangle\": %u, \"feature\": %d, ", r.t, r.prim, (int)r.feature);
    if (posed) printf("\"query_triangle\": %u, ", r.query_triangle);
    printf("\"material\": \"%s\", \"point\": [%.9g, %.9g, %.9g]}\n", name.c_str(), r.cx, r.cy, r.cz);
}
static void castTriangles(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<CastArg>& casts)
{
    const size_t n = casts.size();
    void* d_casts = nullptr; void* d_out = nullptr;
    std::vector<pt_triangle_cast_hit> out(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_casts, n * 64) != 0 || pt_device_malloc(state.context, &d_out, n * sizeof(pt_triangle_cast_hit)) != 0 ||
        pt_copy_to_device(state.context, d_casts, casts.data(), n * 64) != 0 ||
        pt_query_triangle_cast(state.context, (const float*)d_casts, n, (pt_triangle_cast_hit*)d_out) != 0 ||
        pt_copy_to_host(state.context, out.data(), d_out, n * sizeof(pt_triangle_cast_hit)) != 0)
        err = pt_last_error(state.context);
    if (d_casts) pt_device_free(state.context, d_casts);
    if (d_out) pt_device_free(state.context, d_out);
    if (!err.empty()) throw Exception("cast: " + err);
    for (size_t i = 0; i < n; i++) {
        const float* q = casts[i].v;
        printf("{\"cast\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"tmax\": ", q[0], q[1], q[2], q[4], q[5], q[6], q[8], q[9], q[10],
               q[12], q[13], q[14]);
        if (std::isfinite(q[3])) printf("%.9g", q[3]); else printf("null");
        printCastHit(out[i], obj.getMaterialNames(), false);
    }
    fflush(stdout);
}

// --cast-mesh mesh.obj,dx,dy,dz[,tmax] (repeatable): a second OBJ as the query mesh (pt_set_query_mesh), as it is, moving along d; one
// JSON line: how far it gets (pt_query_poses_cast) and which of its triangles touches what first
struct CastMesh { std::string path; float d[3]; float tmax; };
static void castMeshes(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<CastMesh>& meshes)
{
    for (size_t i = 0; i < meshes.size(); i++) {
        const CastMesh& m = meshes[i];
        TinyObjWrapper mesh(m.path);
        const std::vector<float> v = mesh.getVerticesFloat();
        const std::vector<uint32_t> idx = mesh.getIndexBuffer();
        const size_t T = idx.size() / 3;
        std::vector<float> recs(T * 12, 0.0f);
        for (size_t k = 0; k < T * 3; k++) for (int c = 0; c < 3; c++) recs[k * 4 + c] = v[(size_t)idx[k] * 4 + c];
        const float pose[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
        const float motion[4] = {m.d[0], m.d[1], m.d[2], m.tmax};
        void* d_pose = nullptr; void* d_motion = nullptr; void* d_out = nullptr;
        pt_triangle_cast_hit r;
        std::string err;
        if (T == 0) err = "the mesh has no triangles";
        else if (pt_set_query_mesh(state.context, recs.data(), T) != 0 || pt_device_malloc(state.context, &d_pose, 48) != 0 || pt_device_malloc(state.context, &d_motion, 16) != 0 ||
                 pt_device_malloc(state.context, &d_out, sizeof(r)) != 0 || pt_copy_to_device(state.context, d_pose, pose, 48) != 0 ||
                 pt_copy_to_device(state.context, d_motion, motion, 16) != 0 ||
                 pt_query_poses_cast(state.context, (const float*)d_pose, (const float*)d_motion, 1, (pt_triangle_cast_hit*)d_out) != 0 ||
                 pt_copy_to_host(state.context, &r, d_out, sizeof(r)) != 0)
            err = pt_last_error(state.context);
        if (d_pose) pt_device_free(state.context, d_pose);
        if (d_motion) pt_device_free(state.context, d_motion);
        if (d_out) pt_device_free(state.context, d_out);
        if (!err.empty()) throw Exception("cast-mesh: " + err);
        std::string name = m.path;
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        printf("{\"cast_mesh\": \"%s\", \"triangles\": %zu, \"motion\": [%.9g, %.9g, %.9g], \"tmax\": ", name.c_str(), T, m.d[0], m.d[1], m.d[2]);
        if (std::isfinite(m.tmax)) printf("%.9g", m.tmax); else printf("null");
        printCastHit(r, obj.getMaterialNames(), true);
    }
    fflush(stdout);
}

// --clearance: every segment in one call of pt_query_segments; one JSON line per segment
struct ClearanceSegment { float g[8]; float radius; };
static void clearanceSegments(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<ClearanceSegment>& segs)
{
    const size_t n = segs.size();
    void* d_segs = nullptr; void* d_out = nullptr;
    std::vector<float> in(n * 8);
    for (size_t i = 0; i < n; i++) for (int k = 0; k < 8; k++) in[i * 8 + k] = segs[i].g[k];
    std::vector<pt_segment_hit> out(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_segs, n * 32) != 0 || pt_device_malloc(state.context, &d_out, n * sizeof(pt_segment_hit)) != 0 ||
        pt_copy_to_device(state.context, d_segs, in.data(), n * 32) != 0 ||
        pt_query_segments(state.context, (const float*)d_segs, n, (pt_segment_hit*)d_out) != 0 ||
        pt_copy_to_host(state.context, out.data(), d_out, n * sizeof(pt_segment_hit)) != 0)
        err = pt_last_error(state.context);
    if (d_segs) pt_device_free(state.context, d_segs);
    if (d_out) pt_device_free(state.context, d_out);
    if (!err.empty()) throw Exception("clearance: " + err);
    const std::vector<std::string>& names = obj.getMaterialNames();
    for (size_t i = 0; i < n; i++) {
        const pt_segment_hit& r = out[i];
        const float* g = segs[i].g;
        printf("{\"clearance\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"radius\": %.9g, ", g[0], g[1], g[2], g[4], g[5], g[6], segs[i].radius);
        if (r.prim == 0xFFFFFFFFu) { printf("\"found\": false}\n"); continue; }
        std::string name = r.material < names.size() ? names[r.material] : std::string();
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        const float px = g[0] + (g[4] - g[0]) * r.s, py = g[1] + (g[5] - g[1]) * r.s, pz = g[2] + (g[6] - g[2]) * r.s;
        printf("\"found\": true, \"distance\": %.9g, \"clear\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"s\": %.9g, \"feature\": %d, \"on_segment\": [%.9g, %.9g, %.9g], \"point\": [%.9g, %.9g, %.9g]}\n",
               r.distance, r.distance - segs[i].radius, r.prim, name.c_str(), r.s, (int)r.feature, px, py, pz, r.cx, r.cy, r.cz);
    }
    fflush(stdout);
}

// --collide mesh.obj[,tx,ty,tz[,radius]] (repeatable): a second OBJ as the query mesh of the posed-mesh queries (pt_set_query_mesh), moved by
// the translation; one JSON line: does it touch the scene, the first mesh triangle that does, and with a radius the closest pair
struct CollideMesh { std::string path; float t[3]; float radius; bool limited; };
static void collideMeshes(PathTracerState& state, const std::vector<CollideMesh>& meshes)
{
    for (size_t i = 0; i < meshes.size(); i++) {
        const CollideMesh& m = meshes[i];
        TinyObjWrapper mesh(m.path);
        const std::vector<float> v = mesh.getVerticesFloat();
        const std::vector<uint32_t> idx = mesh.getIndexBuffer();
        const size_t T = idx.size() / 3;
        std::vector<float> recs(T * 12, 0.0f);
        for (size_t k = 0; k < T * 3; k++) for (int c = 0; c < 3; c++) recs[k * 4 + c] = v[(size_t)idx[k] * 4 + c];
        const float pose[12] = {1.0f, 0.0f, 0.0f, m.t[0], 0.0f, 1.0f, 0.0f, m.t[1], 0.0f, 0.0f, 1.0f, m.t[2]};
        void* d_pose = nullptr; void* d_hit = nullptr; void* d_first = nullptr; void* d_out = nullptr;
        uint8_t hit = 0; uint32_t first = 0xFFFFFFFFu;
        pt_pose_distance_hit r;
        std::string err;
        if (T == 0) err = "the mesh has no triangles";
        else if (pt_set_query_mesh(state.context, recs.data(), T) != 0 || pt_device_malloc(state.context, &d_pose, 48) != 0 || pt_device_malloc(state.context, &d_hit, 16) != 0 ||
                 pt_device_malloc(state.context, &d_first, 16) != 0 || pt_device_malloc(state.context, &d_out, sizeof(r)) != 0 ||
                 pt_copy_to_device(state.context, d_pose, pose, 48) != 0 ||
                 pt_query_poses_any(state.context, (const float*)d_pose, 1, (uint8_t*)d_hit, (uint32_t*)d_first) != 0 ||
                 pt_copy_to_host(state.context, &hit, d_hit, 1) != 0 || pt_copy_to_host(state.context, &first, d_first, 4) != 0 ||
                 (m.limited && (pt_query_poses_distance(state.context, (const float*)d_pose, 1, m.radius, (pt_pose_distance_hit*)d_out) != 0 ||
                                pt_copy_to_host(state.context, &r, d_out, sizeof(r)) != 0)))
            err = pt_last_error(state.context);
        if (d_pose) pt_device_free(state.context, d_pose);
        if (d_hit) pt_device_free(state.context, d_hit);
        if (d_first) pt_device_free(state.context, d_first);
        if (d_out) pt_device_free(state.context, d_out);
        if (!err.empty()) throw Exception("collide: " + err);
        std::string name = m.path;
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        printf("{\"collide\": {\"mesh\": \"%s\", \"triangles\": %zu, \"translation\": [%.9g, %.9g, %.9g], \"hit\": %d, \"first\": %lld", name.c_str(), T, m.t[0], m.t[1], m.t[2],
               (int)hit, first == 0xFFFFFFFFu ? -1ll : (long long)first);
        if (m.limited) {
            const bool found = r.prim != 0xFFFFFFFFu;
            printf(", \"radius\": %.9g, \"found\": %s, \"distance\": %.9g, \"query_triangle\": %lld, \"prim\": %lld, \"feature\": %d, \"on_query\": [%.9g, %.9g, %.9g], \"point\": [%.9g, %.9g, %.9g]",
                   m.radius, found ? "true" : "false", r.distance, found ? (long long)r.query_triangle : -1ll, found ? (long long)r.prim : -1ll, (int)r.feature, r.qx, r.qy, r.qz,
                   r.cx, r.cy, r.cz);
        }
        printf("}}\n");
    }
    fflush(stdout);
}

// --tri-distance: every triangle in one call of pt_query_triangle_distance; one JSON line per triangle
struct DistanceTriangle { float g[12]; bool limited; };
static void triangleDistances(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<DistanceTriangle>& tris)
{
    const size_t n = tris.size();
    void* d_tris = nullptr; void* d_out = nullptr;
    std::vector<float> in(n * 12);
    for (size_t i = 0; i < n; i++) for (int k = 0; k < 12; k++) in[i * 12 + k] = tris[i].g[k];
    std::vector<pt_triangle_distance_hit> out(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_tris, n * 48) != 0 || pt_device_malloc(state.context, &d_out, n * sizeof(pt_triangle_distance_hit)) != 0 ||
        pt_copy_to_device(state.context, d_tris, in.data(), n * 48) != 0 ||
        pt_query_triangle_distance(state.context, (const float*)d_tris, n, (pt_triangle_distance_hit*)d_out) != 0 ||
        pt_copy_to_host(state.context, out.data(), d_out, n * sizeof(pt_triangle_distance_hit)) != 0)
        err = pt_last_error(state.context);
    if (d_tris) pt_device_free(state.context, d_tris);
    if (d_out) pt_device_free(state.context, d_out);
    if (!err.empty()) throw Exception("tri-distance: " + err);
    const std::vector<std::string>& names = obj.getMaterialNames();
    for (size_t i = 0; i < n; i++) {
        const pt_triangle_distance_hit& r = out[i];
        const float* g = tris[i].g;
        printf("{\"tri_distance\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"radius\": ", g[0], g[1], g[2], g[4], g[5], g[6], g[8], g[9], g[10]);
        if (tris[i].limited && std::isfinite(g[3])) printf("%.9g, ", g[3]); else printf("null, ");
        if (r.prim == 0xFFFFFFFFu) { printf("\"found\": false}\n"); continue; }
        std::string name = r.material < names.size() ? names[r.material] : std::string();
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        printf("\"found\": true, \"distance\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"feature\": %d, \"on_query\": [%.9g, %.9g, %.9g], \"point\": [%.9g, %.9g, %.9g]}\n",
               r.distance, r.prim, name.c_str(), (int)r.feature, r.qx, r.qy, r.qz, r.cx, r.cy, r.cz);
    }
    fflush(stdout);
}

// --nearest: every point in one call of pt_query_nearest; one JSON line per point
static void nearestPoints(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<float4>& points)
{
    const size_t n = points.size();
    void* d_points = nullptr; void* d_out = nullptr;
    std::vector<pt_nearest> out(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_points, n * 16) != 0 || pt_device_malloc(state.context, &d_out, n * sizeof(pt_nearest)) != 0 ||
        pt_copy_to_device(state.context, d_points, points.data(), n * 16) != 0 ||
        pt_query_nearest(state.context, (const float*)d_points, n, (pt_nearest*)d_out) != 0 ||
        pt_copy_to_host(state.context, out.data(), d_out, n * sizeof(pt_nearest)) != 0)
        err = pt_last_error(state.context);
    if (d_points) pt_device_free(state.context, d_points);
    if (d_out) pt_device_free(state.context, d_out);
    if (!err.empty()) throw Exception("nearest: " + err);
    const std::vector<std::string>& names = obj.getMaterialNames();
    for (size_t i = 0; i < n; i++) {
        const pt_nearest& r = out[i];
        const float4& q = points[i];
        if (r.prim == 0xFFFFFFFFu) { printf("{\"nearest\": [%.9g, %.9g, %.9g], \"found\": false}\n", q.x, q.y, q.z); continue; }
        std::string name = r.material < names.size() ? names[r.material] : std::string();
        for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
        printf("{\"nearest\": [%.9g, %.9g, %.9g], \"found\": true, \"distance\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"point\": [%.9g, %.9g, %.9g], \"u\": %.9g, \"v\": %.9g}\n",
               q.x, q.y, q.z, r.distance, r.prim, name.c_str(), r.cx, r.cy, r.cz, r.u, r.v);
    }
    fflush(stdout);
}

// --nearest-k: the points of one k in one call of pt_query_nearest_k, with counts; one JSON line per point, in the order given
struct NearestKPoint { float4 q; uint32_t k; };
static void nearestKPoints(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<NearestKPoint>& points)
{
    const std::vector<std::string>& names = obj.getMaterialNames();
    std::vector<std::string> lines(points.size());
    for (uint32_t k = 1; k <= PT_QUERY_NEAREST_MAX; k++) {
        std::vector<size_t> which;
        std::vector<float4> in;
        for (size_t i = 0; i < points.size(); i++) if (points[i].k == k) { which.push_back(i); in.push_back(points[i].q); }
        const size_t n = in.size();
        if (n == 0) continue;
        void* d_points = nullptr; void* d_out = nullptr; void* d_counts = nullptr;
        std::vector<pt_nearest> out(n * k);
        std::vector<uint32_t> counts(n);
        std::string err;
        if (pt_device_malloc(state.context, &d_points, n * 16) != 0 || pt_device_malloc(state.context, &d_out, n * k * sizeof(pt_nearest)) != 0 ||
            pt_device_malloc(state.context, &d_counts, n * 4) != 0 || pt_copy_to_device(state.context, d_points, in.data(), n * 16) != 0 ||
            pt_query_nearest_k(state.context, (const float*)d_points, n, k, (pt_nearest*)d_out, (uint32_t*)d_counts) != 0 ||
            pt_copy_to_host(state.context, out.data(), d_out, n * k * sizeof(pt_nearest)) != 0 ||
            pt_copy_to_host(state.context, counts.data(), d_counts, n * 4) != 0)
            err = pt_last_error(state.context);
        if (d_points) pt_device_free(state.context, d_points);
        if (d_out) pt_device_free(state.context, d_out);
        if (d_counts) pt_device_free(state.context, d_counts);
        if (!err.empty()) throw Exception("nearest-k: " + err);
        char buf[512];
        for (size_t i = 0; i < n; i++) {
            const float4& q = in[i];
            snprintf(buf, sizeof buf, "{\"nearest_k\": [%.9g, %.9g, %.9g], \"k\": %u, \"count\": %u, \"list\": [", q.x, q.y, q.z, k, counts[i]);
            std::string line = buf;
            for (uint32_t j = 0; j < k; j++) {
                const pt_nearest& r = out[i * k + j];
                if (r.prim == 0xFFFFFFFFu) break;
                std::string name = r.material < names.size() ? names[r.material] : std::string();
                for (size_t c = 0; c < name.size(); c++) if (name[c] == '"' || name[c] == '\\' || (unsigned char)name[c] < 0x20) name[c] = '_';
                snprintf(buf, sizeof buf, "%s{\"distance\": %.9g, \"triangle\": %u, \"material\": \"", j ? ", " : "", r.distance, r.prim);
                line += buf;
                line += name;
                snprintf(buf, sizeof buf, "\", \"point\": [%.9g, %.9g, %.9g], \"u\": %.9g, \"v\": %.9g}", r.cx, r.cy, r.cz, r.u, r.v);
                line += buf;
            }
            lines[which[i]] = line + "]}";
        }
    }
    for (const std::string& l : lines) printf("%s\n", l.c_str());
    fflush(stdout);
}

// --within: every point in one call of pt_query_within_any; one JSON line per point
static void withinPoints(PathTracerState& state, const std::vector<float4>& points)
{
    const size_t n = points.size();
    void* d_points = nullptr; void* d_hit = nullptr;
    std::vector<uint8_t> hit(n);
    std::string err;
    if (pt_device_malloc(state.context, &d_points, n * 16) != 0 || pt_device_malloc(state.context, &d_hit, n) != 0 ||
        pt_copy_to_device(state.context, d_points, points.data(), n * 16) != 0 ||
        pt_query_within_any(state.context, (const float*)d_points, n, (uint8_t*)d_hit) != 0 ||
        pt_copy_to_host(state.context, hit.data(), d_hit, n) != 0)
        err = pt_last_error(state.context);
    if (d_points) pt_device_free(state.context, d_points);
    if (d_hit) pt_device_free(state.context, d_hit);
    if (!err.empty()) throw Exception("within: " + err);
    for (size_t i = 0; i < n; i++)
        printf("{\"within\": [%.9g, %.9g, %.9g], \"radius\": %.9g, \"hit\": %s}\n", points[i].x, points[i].y, points[i].z, points[i].w, hit[i] ? "true" : "false");
    fflush(stdout);
}

// --winding: one call of pt_query_winding per point (each has its own beta, in .w); one JSON line per point
static void windingPoints(PathTracerState& state, const std::vector<float4>& points)
{
    void* d_point = nullptr; void* d_w = nullptr;
    std::string err;
    std::vector<float> w(points.size(), 0.0f);
    if (pt_device_malloc(state.context, &d_point, 16) != 0 || pt_device_malloc(state.context, &d_w, 4) != 0) err = pt_last_error(state.context);
    for (size_t i = 0; i < points.size() && err.empty(); i++)
        if (pt_copy_to_device(state.context, d_point, &points[i], 16) != 0 ||
            pt_query_winding(state.context, (const float*)d_point, 1, points[i].w, (float*)d_w) != 0 ||
            pt_copy_to_host(state.context, &w[i], d_w, 4) != 0)
            err = pt_last_error(state.context);
    if (d_point) pt_device_free(state.context, d_point);
    if (d_w) pt_device_free(state.context, d_w);
    if (!err.empty()) throw Exception("winding: " + err);
    for (size_t i = 0; i < points.size(); i++) {
        char beta[32];
        if (std::isinf(points[i].w)) snprintf(beta, sizeof(beta), "\"inf\""); else snprintf(beta, sizeof(beta), "%.9g", points[i].w);
        printf("{\"winding\": [%.9g, %.9g, %.9g], \"beta\": %s, \"w\": %.9g, \"inside\": %s}\n", points[i].x, points[i].y, points[i].z, beta, w[i],
               w[i] > 0.5f ? "true" : "false");
    }
    fflush(stdout);
}

// --ao: the default sample pattern (pathtracer.aoSamples restated: the same double operations, the same fp32 pull-in)
static std::vector<float> aoSamples(int K)
{
    const double golden = M_PI * (3.0 - std::sqrt(5.0));
    std::vector<float> disk(2 * (size_t)K);
    for (int k = 0; k < K; k++) {
        const double r = std::sqrt((k + 0.5) / K);
        float x = (float)(r * std::cos(k * golden)), y = (float)(r * std::sin(k * golden));
        while (x * x + y * y > 1.0f) { x = std::nextafterf(x, 0.0f); y = std::nextafterf(y, 0.0f); }
        disk[2 * k] = x; disk[2 * k + 1] = y;
    }
    return disk;
}

// --ao: pt_render_features, then `frames` accumulating pt_ao_image calls; the AO image as a grey .pfm
static void ambientOcclusion(PathTracerState& state, int K, float radius, float bias, int frames, const std::string& path)
{
    const pt_params& p = state.params;
    const size_t n = (size_t)p.width * p.height;
    pt_bvh_info info;
    PT_CHECK(state.context, pt_get_bvh_info(state.context, &info));
    double diag = 0.0;
    for (int k = 0; k < 3; k++) diag += ((double)info.scene_hi[k] - (double)info.scene_lo[k]) * ((double)info.scene_hi[k] - (double)info.scene_lo[k]);
    diag = std::sqrt(diag);
    if (!(radius > 0.0f)) radius = (float)(0.25 * diag);
    if (bias < 0.0f) bias = (float)(1e-3 * diag);
    const std::vector<float> disk = aoSamples(K);
    void* d_alb = nullptr; void* d_nd = nullptr; void* d_vis = nullptr; void* d_ao = nullptr;
    std::vector<float> ao(n);
    std::string err;
    bool ok = pt_device_malloc(state.context, &d_alb, n * 16) == 0 && pt_device_malloc(state.context, &d_nd, n * 16) == 0 &&
              pt_device_malloc(state.context, &d_vis, n * 4) == 0 && pt_device_malloc(state.context, &d_ao, n * 4) == 0 &&
              pt_render_features(state.context, &p, (float*)d_alb, (float*)d_nd) == 0;
    for (int j = 0; ok && j < frames; j++) {
        const pt_ao_params ap = {(uint32_t)K, radius, bias, (uint32_t)j, j > 0 ? 1u : 0u, (uint32_t)K * (uint32_t)(j + 1), {0u, 0u}};
        ok = pt_ao_image(state.context, &p, (const float*)d_nd, disk.data(), &ap, (uint32_t*)d_vis, (float*)d_ao) == 0;
    }
    ok = ok && pt_copy_to_host(state.context, ao.data(), d_ao, n * 4) == 0;
    if (!ok) err = pt_last_error(state.context);
    for (void* b : {d_alb, d_nd, d_vis, d_ao}) if (b) pt_device_free(state.context, b);
    if (!ok) throw Exception("ao: " + err);
    std::vector<float> grey(n * 3);
    double sum = 0.0;
    for (size_t i = 0; i < n; i++) { grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = ao[i]; sum += ao[i]; }
    if (!savePFM(path, grey.data(), (int)p.width, (int)p.height, 3)) throw Exception("could not write " + path);
    std::cout << "Ambient occlusion: " << K << " x " << frames << " rays per pixel, radius " << radius << ", bias " << bias << ", mean " << sum / (double)n
              << " -> " << path << std::endl;
}

static void CleanAllTheThings(PathTracerState& state)                    // :629-646
{
    if (state.params.accumulationBuffer) pt_device_free(state.context, state.params.accumulationBuffer);
    pt_destroy(state.context);
    state.context = nullptr;
}

int main(int argc, char** argv)
{
    std::string objfilepath, out = "frame.png", keys, save_accum, restore_accum, history_out, history_in, move;
    std::vector<std::string> material_edits;
    std::vector<int2> picks;
    std::vector<PickAll> pickAlls;
    std::vector<float4> nearest;
    std::vector<NearestKPoint> nearestKs;
    std::vector<float4> withins;
    std::vector<float4> windings;
    std::vector<ClearanceSegment> clearances;
    std::vector<DistanceTriangle> triDistances;
    std::vector<CollideMesh> collides;
    std::vector<OverlapBox> overlaps, oriented_overlaps;
    std::vector<IntersectTri> intersects;
    std::vector<SweepArg> sweeps;
    std::vector<CapsuleCastArg> capsuleCasts;
    std::vector<BoxCastArg> boxCasts;
    std::vector<CastArg> casts;
    std::vector<CastMesh> castMeshList;
    int32_t width = 512, height = 512, frames = 8, dump_every = 0, denoise_iters = 0;
    bool zero_copy = false, move_history = false, no_area_light = false;
    std::string env_path, tonemap, exposure_arg, out_hdr, error_out, ao_out;
    int ao_samples = 0, ao_frames = 1;
    float ao_radius = 0.0f, ao_bias = -1.0f;      // the defaults: from the scene box (ambientOcclusion)
    pt_firefly_params firefly = {0.0f, 0.01f, 1u, 1u};       // ratio 0: no --firefly; the other defaults of include/acgpt.h
    pt_bloom_params bloom = {1.0f, 0.5f, 0.0f, 0.02f, 1.0f, 6u};   // pt_bloom_params' defaults (include/acgpt.h), in display units
    bool use_bloom = false;
    // pt_convergence_params' defaults (include/acgpt.h); threshold 0: no --until-error
    pt_convergence_params until = {0.01f, 0.0f, 950u, 0u};
    float env_scale = 1.0f;
    int orbit_dx = 0, orbit_dy = 0, zoom_steps = 0, sample_chunks = 0, build_mode = 1, fuse = 1, light_mode = 0, math_mode = PT_MATH_FAST, material_model = PT_MATERIALS_REFERENCE;
    PathTracerState state;
    state.params.useDirectLighting = false;
    state.params.useImportanceSampling = false;
    state.params.maxDepth = 4;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::cerr << "missing value for " << a << std::endl; exit(2); } return argv[++i]; };
        if (a == "--obj") objfilepath = next();
        else if (a == "--width") width = atoi(next());
        else if (a == "--height") height = atoi(next());
        else if (a == "--spp-per-launch") samples_per_launch = atoi(next());
        else if (a == "--frames") frames = atoi(next());
        else if (a == "--max-depth") state.params.maxDepth = (uint32_t)std::min((int)maxiumumRecursionDepth, std::max(1, atoi(next())));
        else if (a == "--direct-lighting") state.params.useDirectLighting = true;
        else if (a == "--importance-sampling") state.params.useImportanceSampling = true;
        else if (a == "--device") state.device = atoi(next());
        else if (a == "--gpus") state.gpus = std::max(1, atoi(next()));
        else if (a == "--multi") state.multi = true;
        else if (a == "--save-accum") save_accum = next();
        else if (a == "--restore-accum") restore_accum = next();
        else if (a == "--keys") keys = next();
        else if (a == "--out") out = next();
        else if (a == "--dump-every") dump_every = atoi(next());
        else if (a == "--zero-copy") zero_copy = true;
        else if (a == "--orbit") { if (sscanf(next(), "%d,%d", &orbit_dx, &orbit_dy) != 2) { std::cerr << "--orbit dx,dy" << std::endl; return 2; } }
        else if (a == "--zoom") zoom_steps = atoi(next());
        else if (a == "--sample-chunks") sample_chunks = atoi(next());
        else if (a == "--build-mode") build_mode = atoi(next());
        else if (a == "--fuse-frames") fuse = std::min(64, std::max(1, atoi(next())));
        else if (a == "--math") { const std::string m = next(); math_mode = (m == "ieee" || m == "0") ? PT_MATH_IEEE : PT_MATH_FAST; }   // fast: the arithmetic of the reference's own build (nvcc --use_fast_math); ieee: the CPU oracle's
        else if (a == "--denoise") denoise_iters = atoi(next());
        else if (a == "--history-out") history_out = next();
        else if (a == "--history-in") history_in = next();
        else if (a == "--move") move = next();
        else if (a == "--move-history") move_history = true;
        else if (a == "--set-material") material_edits.push_back(next());
        else if (a == "--env") env_path = next();
        else if (a == "--env-scale") env_scale = (float)atof(next());
        else if (a == "--no-area-light") no_area_light = true;
        else if (a == "--tonemap") tonemap = next();
        else if (a == "--exposure") exposure_arg = next();
        else if (a == "--out-hdr") out_hdr = next();
        else if (a == "--until-error") { until.threshold = (float)atof(next()); if (!std::isfinite(until.threshold) || !(until.threshold > 0.0f)) { std::cerr << "--until-error takes an error > 0" << std::endl; return 2; } }
        else if (a == "--until-permille") { const int v = atoi(next()); if (v < 1 || v > 1000) { std::cerr << "--until-permille takes 1 to 1000" << std::endl; return 2; } until.quantile_permille = (uint32_t)v; }
        else if (a == "--error-floor") { until.lum_floor = (float)atof(next()); if (!std::isfinite(until.lum_floor) || !(until.lum_floor > 0.0f)) { std::cerr << "--error-floor takes a luminance > 0" << std::endl; return 2; } }
        else if (a == "--error-out") error_out = next();
        else if (a == "--firefly") {
            int rank = 1, radius = 1;
            const int got = sscanf(next(), "%f,%d,%d", &firefly.ratio, &rank, &radius);
            if (got < 1 || !std::isfinite(firefly.ratio) || !(firefly.ratio >= 1.0f) || rank < 1 || rank > 4 || radius < 1 || radius > 2) {
                std::cerr << "--firefly takes ratio[,rank[,radius]]: ratio >= 1, rank 1 to 4, radius 1 or 2" << std::endl; return 2;
            }
            firefly.rank = (uint32_t)rank; firefly.radius = (uint32_t)radius;
        }
        else if (a == "--bloom") {
            use_bloom = true;
            if (i + 1 < argc && argv[i + 1][0] != '-') {              // a value: threshold,intensity[,levels[,spread]]; the knee is half the threshold
                int levels = 6;
                const int got = sscanf(next(), "%f,%f,%d,%f", &bloom.threshold, &bloom.intensity, &levels, &bloom.spread);
                if (got < 2 || !std::isfinite(bloom.threshold) || bloom.threshold < 0.0f || !std::isfinite(bloom.intensity) || bloom.intensity < 0.0f || levels < 1 ||
                    levels > 8 || !std::isfinite(bloom.spread) || bloom.spread < 0.0f || bloom.spread > 4.0f) {
                    std::cerr << "--bloom takes threshold,intensity[,levels[,spread]]: threshold and intensity >= 0, levels 1 to 8, spread 0 to 4" << std::endl; return 2;
                }
                bloom.levels = (uint32_t)levels; bloom.knee = 0.5f * bloom.threshold;
            }
        }
        else if (a == "--ao") {
            const int got = sscanf(next(), "%d,%f,%f", &ao_samples, &ao_radius, &ao_bias);
            if (got < 1 || ao_samples < 1 || ao_samples > 256 || (got >= 2 && (!std::isfinite(ao_radius) || !(ao_radius > 0.0f))) || (got >= 3 && (!std::isfinite(ao_bias) || !(ao_bias >= 0.0f)))) {
                std::cerr << "--ao takes K[,radius[,bias]]: K 1 to 256, radius > 0, bias >= 0" << std::endl; return 2;
            }
        }
        else if (a == "--ao-out") ao_out = next();
        else if (a == "--ao-frames") { ao_frames = atoi(next()); if (ao_frames < 1 || ao_frames > 65536) { std::cerr << "--ao-frames takes 1 to 65536" << std::endl; return 2; } }
        else if (a == "--pick-all") {
            PickAll pa; pa.k = 4;
            const int got = sscanf(next(), "%d,%d,%d", &pa.x, &pa.y, &pa.k);
            if (got < 2 || pa.k < 1 || pa.k > PT_QUERY_MULTI_MAX) { std::cerr << "--pick-all x,y[,k] with k = 1.." << PT_QUERY_MULTI_MAX << std::endl; return 2; }
            pickAlls.push_back(pa);
        }
        else if (a == "--pick") { int2 px; if (sscanf(next(), "%d,%d", &px.x, &px.y) != 2) { std::cerr << "--pick x,y" << std::endl; return 2; } picks.push_back(px); }
        else if (a == "--nearest") {
            float4 q = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
            const int got = sscanf(next(), "%f,%f,%f,%f", &q.x, &q.y, &q.z, &q.w);
            if (got < 3 || !std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z) || !(q.w >= 0.0f)) { std::cerr << "--nearest x,y,z[,radius]: finite coordinates, a radius >= 0" << std::endl; return 2; }
            nearest.push_back(q);
        }
        else if (a == "--nearest-k") {
            NearestKPoint p = {make_float4(0.0f, 0.0f, 0.0f, INFINITY), 0u};
            float kf = 0.0f;
            const int got = sscanf(next(), "%f,%f,%f,%f,%f", &p.q.x, &p.q.y, &p.q.z, &kf, &p.q.w);
            if (got < 4 || !std::isfinite(p.q.x) || !std::isfinite(p.q.y) || !std::isfinite(p.q.z) || !(kf >= 1.0f && kf <= (float)PT_QUERY_NEAREST_MAX) || kf != std::floor(kf) || !(p.q.w >= 0.0f)) {
                std::cerr << "--nearest-k x,y,z,k[,radius]: finite coordinates, k = 1..8, a radius >= 0" << std::endl; return 2;
            }
            p.k = (uint32_t)kf;
            nearestKs.push_back(p);
        }
        else if (a == "--within") {
            float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int got = sscanf(next(), "%f,%f,%f,%f", &q.x, &q.y, &q.z, &q.w);
            if (got < 4 || !std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z) || !(q.w >= 0.0f)) { std::cerr << "--within x,y,z,radius: finite coordinates, a radius >= 0" << std::endl; return 2; }
            withins.push_back(q);
        }
        else if (a == "--winding") {
            float4 q = make_float4(0.0f, 0.0f, 0.0f, PT_WINDING_BETA_DEFAULT);
            const int got = sscanf(next(), "%f,%f,%f,%f", &q.x, &q.y, &q.z, &q.w);
            if (got < 3 || !std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z) || !(q.w >= 1.0f)) { std::cerr << "--winding x,y,z[,beta]: finite coordinates, a beta >= 1 (inf: the exact sum)" << std::endl; return 2; }
            windings.push_back(q);
        }
        else if (a == "--clearance") {
            ClearanceSegment cs = {{0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f}, 0.0f};
            float* g = cs.g;
            const int got = sscanf(next(), "%f,%f,%f,%f,%f,%f,%f", &g[0], &g[1], &g[2], &g[4], &g[5], &g[6], &cs.radius);
            bool fine = got >= 6 && cs.radius >= 0.0f && std::isfinite(cs.radius);
            for (int k = 0; k < 7; k++) if (k != 3 && !std::isfinite(g[k])) fine = false;
            if (!fine) { std::cerr << "--clearance x0,y0,z0,x1,y1,z1[,radius]: finite coordinates, a finite radius >= 0" << std::endl; return 2; }
            clearances.push_back(cs);
        }
        else if (a == "--tri-distance") {
            DistanceTriangle dt = {{0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, false};
            float* g = dt.g;
            const char* text = next();
            int used = 0;
            int got = sscanf(text, "%f,%f,%f,%f,%f,%f,%f,%f,%f%n", &g[0], &g[1], &g[2], &g[4], &g[5], &g[6], &g[8], &g[9], &g[10], &used);
            bool fine = got == 9;
            if (fine && text[used] != '\0') {                  // a tenth number, the radius, and nothing behind it
                int more = 0;
                fine = sscanf(text + used, ",%f%n", &g[3], &more) == 1 && text[used + more] == '\0' && g[3] >= 0.0f;
                dt.limited = true;
            }
            for (int k = 0; k < 11; k++) if (k != 3 && k != 7 && !std::isfinite(g[k])) fine = false;
            if (!fine) { std::cerr << "--tri-distance x0,y0,z0,x1,y1,z1,x2,y2,z2[,radius]: nine finite coordinates, a radius >= 0" << std::endl; return 2; }
            triDistances.push_back(dt);
        }
        else if (a == "--collide") {
            CollideMesh cm = {std::string(), {0.0f, 0.0f, 0.0f}, 0.0f, false};
            const std::string text = next();
            const size_t comma = text.find(',');
            cm.path = text.substr(0, comma);
            bool fine = !cm.path.empty();
            if (fine && comma != std::string::npos) {
                int used = 0;
                const char* rest = text.c_str() + comma;
                fine = sscanf(rest, ",%f,%f,%f%n", &cm.t[0], &cm.t[1], &cm.t[2], &used) == 3;
                if (fine && rest[used] != '\0') {               // a fourth number, the radius, and nothing behind it
                    int more = 0;
                    fine = sscanf(rest + used, ",%f%n", &cm.radius, &more) == 1 && rest[used + more] == '\0' && cm.radius >= 0.0f;
                    cm.limited = true;
                }
                for (int k = 0; k < 3; k++) if (!std::isfinite(cm.t[k])) fine = false;
            }
            if (!fine) { std::cerr << "--collide mesh.obj[,tx,ty,tz[,radius]]: a file, a finite translation, a radius >= 0" << std::endl; return 2; }
            collides.push_back(cm);
        }
        else if (a == "--overlap") {
            OverlapBox b = {{0.0f}, 8u, {0.0}};
            int k = 8;
            std::string text = next();
            const bool all = wantsAll(text);
            const int got = sscanf(text.c_str(), "%f,%f,%f,%f,%f,%f,%d", &b.v[0], &b.v[1], &b.v[2], &b.v[3], &b.v[4], &b.v[5], &k);
            bool ok = (all ? got == 6 : got >= 6) && k >= 0 && k <= 8;
            if (all) k = (int)kListAll;
            for (int j = 0; j < 6; j++) ok = ok && std::isfinite(b.v[j]) && (j < 3 || b.v[j] >= 0.0f);
            if (!ok) { std::cerr << "--overlap cx,cy,cz,hx,hy,hz[,k]: finite values, half extents >= 0, k = 0..8 or all" << std::endl; return 2; }
            b.k = (uint32_t)k;
            overlaps.push_back(b);
        }
        else if (a == "--overlap-oriented") {
            OverlapBox b = {{0.0f}, 8u, {0.0}};
            int k = 8;
            std::string text = next();
            const bool all = wantsAll(text);
            double* q = b.arg;
            const int got = sscanf(text.c_str(), "%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf,%d", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6], &q[7], &q[8], &q[9], &k);
            bool ok = (all ? got == 10 : got >= 10) && k >= 0 && k <= 8;
            if (all) k = (int)kListAll;
            for (int j = 0; j < 10; j++) ok = ok && std::isfinite((float)q[j]) && (j < 3 || j >= 6 || (float)q[j] >= 0.0f);
            const double len = std::sqrt(q[6] * q[6] + q[7] * q[7] + q[8] * q[8] + q[9] * q[9]);
            ok = ok && std::isfinite(len) && len > 0.0;
            if (!ok) {
                std::cerr << "--overlap-oriented cx,cy,cz,hx,hy,hz,qw,qx,qy,qz[,k]: finite values, half extents >= 0, a quaternion that is not zero, k = 0..8 or all" << std::endl;
                return 2;
            }
            // the quaternion is normalised in double; the rotation it stands for, local -> world, rounded to float once per entry
            for (int j = 6; j < 10; j++) q[j] /= len;
            const double w = q[6], x = q[7], y = q[8], z = q[9];
            const double r[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                                 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
            for (int row = 0; row < 3; row++) {
                for (int col = 0; col < 3; col++) b.v[4 * row + col] = (float)r[3 * row + col];
                b.v[4 * row + 3] = (float)q[row];
                b.v[12 + row] = (float)q[3 + row];
            }
            b.k = (uint32_t)k;
            oriented_overlaps.push_back(b);
        }
        else if (a == "--intersect") {
            IntersectTri t = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, 8u};
            int k = 8;
            float* v = t.v;
            std::string text = next();
            const bool all = wantsAll(text);
            const int got = sscanf(text.c_str(), "%f,%f,%f,%f,%f,%f,%f,%f,%f,%d", &v[0], &v[1], &v[2], &v[4], &v[5], &v[6], &v[8], &v[9], &v[10], &k);
            bool ok = (all ? got == 9 : got >= 9) && k >= 0 && k <= 8;
            if (all) k = (int)kListAll;
            for (int j = 0; j < 12; j++) ok = ok && std::isfinite(v[j]);
            if (!ok) { std::cerr << "--intersect x0,y0,z0,x1,y1,z1,x2,y2,z2[,k]: finite coordinates, k = 0..8 or all" << std::endl; return 2; }
            t.k = (uint32_t)k;
            intersects.push_back(t);
        }
        else if (a == "--sweep") {
            SweepArg w = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, INFINITY}};
            const int got = sscanf(next(), "%f,%f,%f,%f,%f,%f,%f,%f", &w.v[0], &w.v[1], &w.v[2], &w.v[3], &w.v[4], &w.v[5], &w.v[6], &w.v[7]);
            bool ok = got >= 7 && w.v[6] >= 0.0f && w.v[7] >= 0.0f;
            for (int j = 0; j < 7; j++) ok = ok && std::isfinite(w.v[j]);
            if (!ok) { std::cerr << "--sweep ox,oy,oz,dx,dy,dz,r[,tmax]: finite values, a radius >= 0, a tmax >= 0" << std::endl; return 2; }
            sweeps.push_back(w);
        }
        else if (a == "--capsule-cast") {
            CapsuleCastArg w = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f}};
            float* v = w.v;
            const int got = sscanf(next(), "%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f", &v[0], &v[1], &v[2], &v[4], &v[5], &v[6], &v[8], &v[9], &v[10], &v[3], &v[7]);
            bool ok = got >= 10 && v[3] >= 0.0f && v[7] >= 0.0f;
            for (int j = 0; j < 11; j++) ok = ok && (j == 7 || std::isfinite(v[j]));
            if (!ok) { std::cerr << "--capsule-cast x0,y0,z0,x1,y1,z1,dx,dy,dz,r[,tmax]: finite values, a radius >= 0, a tmax >= 0" << std::endl; return 2; }
            capsuleCasts.push_back(w);
        }
        else if (a == "--box-cast") {
            BoxCastArg w = {};
            float* q = w.in;
            float tmax = INFINITY;
            const int got = sscanf(next(), "%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6], &q[7], &q[8], &q[9], &q[10], &q[11],
                                   &q[12], &tmax);
            bool ok = got >= 13 && q[3] >= 0.0f && q[4] >= 0.0f && q[5] >= 0.0f && tmax >= 0.0f;
            for (int j = 0; j < 13; j++) ok = ok && std::isfinite(q[j]);
            const float qw = q[6], qx = q[7], qy = q[8], qz = q[9];
            ok = ok && std::fabs((qw * qw + qx * qx) + (qy * qy + qz * qz) - 1.0f) <= 1e-4f;
            if (!ok) { std::cerr << "--box-cast cx,cy,cz,hx,hy,hz,qw,qx,qy,qz,dx,dy,dz[,tmax]: finite values, half extents >= 0, a unit quaternion, a tmax >= 0" << std::endl; return 2; }
            // the rotation of the unit quaternion, row-major beside the centre: a pt_query_overlap_oriented record, then {d, tmax}
            const float m[12] = {1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qz * qw), 2.0f * (qx * qz + qy * qw), q[0],
                                 2.0f * (qx * qy + qz * qw), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qx * qw), q[1],
                                 2.0f * (qx * qz - qy * qw), 2.0f * (qy * qz + qx * qw), 1.0f - 2.0f * (qx * qx + qy * qy), q[2]};
            for (int j = 0; j < 12; j++) w.v[j] = m[j];
            w.v[12] = q[3]; w.v[13] = q[4]; w.v[14] = q[5]; w.v[15] = 0.0f;
            w.v[16] = q[10]; w.v[17] = q[11]; w.v[18] = q[12]; w.v[19] = tmax;
            boxCasts.push_back(w);
        }
        else if (a == "--cast") {
            CastArg w = {{0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
            float* v = w.v;
            const int got = sscanf(next(), "%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f", &v[0], &v[1], &v[2], &v[4], &v[5], &v[6], &v[8], &v[9], &v[10], &v[12], &v[13], &v[14], &v[3]);
            bool ok = got >= 12 && v[3] >= 0.0f;
            for (int j = 0; j < 15; j++) ok = ok && (j == 3 || std::isfinite(v[j]));
            if (!ok) { std::cerr << "--cast x0,y0,z0,x1,y1,z1,x2,y2,z2,dx,dy,dz[,tmax]: finite values, a tmax >= 0" << std::endl; return 2; }
            casts.push_back(w);
        }
        else if (a == "--cast-mesh") {
            CastMesh cm = {std::string(), {0.0f, 0.0f, 0.0f}, INFINITY};
            const std::string text = next();
            const size_t comma = text.find(',');
            cm.path = text.substr(0, comma);
            bool fine = !cm.path.empty() && comma != std::string::npos;
            if (fine) {
                int used = 0;
                const char* rest = text.c_str() + comma;
                fine = sscanf(rest, ",%f,%f,%f%n", &cm.d[0], &cm.d[1], &cm.d[2], &used) == 3;
                if (fine && rest[used] != '\0') {               // a fourth number, tmax, and nothing behind it
                    int more = 0;
                    fine = sscanf(rest + used, ",%f%n", &cm.tmax, &more) == 1 && rest[used + more] == '\0' && cm.tmax >= 0.0f;
                }
                for (int k = 0; k < 3; k++) if (!std::isfinite(cm.d[k])) fine = false;
            }
            if (!fine) { std::cerr << "--cast-mesh mesh.obj,dx,dy,dz[,tmax]: a file, a finite motion, a tmax >= 0" << std::endl; return 2; }
            castMeshList.push_back(cm);
        }
        else if (a == "--materials") {
            const std::string m = next();
            if (m == "reference") material_model = PT_MATERIALS_REFERENCE;
            else if (m == "microfacet") material_model = PT_MATERIALS_MICROFACET;
            else { std::cerr << "--materials reference|microfacet" << std::endl; return 2; }
        }
        else if (a == "--light-mode") light_mode = atoi(next());      // 0 = the reference's hard-coded rectangle (:154-158), 1 = the OBJ's emissive triangles + MIS
        else { std::cerr << "unknown option " << a << std::endl; return 2; }
    }
    if (objfilepath.empty()) { std::cerr << "usage: acgpt_main --obj scene.obj [options]" << std::endl; return 2; }
    if (denoise_iters < 0 || denoise_iters > 8) { std::cerr << "--denoise takes 0 (off) to 8 iterations" << std::endl; return 2; }
    const bool display = !tonemap.empty() || !exposure_arg.empty();
    // pt_display_params' defaults (include/acgpt.h): key 0.18, white 4, the window 100 .. 900 permille, exposure within 2^-16 .. 2^16
    pt_display_params display_params = {PT_TONE_ACES, 0.0f, 0.18f, 4.0f, 100u, 900u, 1.0f / 65536.0f, 65536.0f, 0.0f, 1.0f};
    if (display) {
        if (tonemap == "linear") display_params.tone_curve = PT_TONE_LINEAR;
        else if (tonemap == "reinhard") display_params.tone_curve = PT_TONE_REINHARD;
        else if (!tonemap.empty() && tonemap != "aces") { std::cerr << "--tonemap linear|reinhard|aces" << std::endl; return 2; }
        if (!exposure_arg.empty() && exposure_arg != "auto") {
            char* end = nullptr;
            const double ev = strtod(exposure_arg.c_str(), &end);
            const float factor = (float)std::exp2(ev);
            if (end == exposure_arg.c_str() || *end != '\0' || !std::isfinite(factor) || !(factor > 0.0f)) { std::cerr << "--exposure auto|<EV>" << std::endl; return 2; }
            display_params.exposure = factor;
        }
    }
    if (use_bloom && !display) { std::cerr << "--bloom needs --tonemap or --exposure" << std::endl; return 2; }
    for (const PickAll& px : pickAlls)
        if (px.x < 0 || px.y < 0 || px.x >= width || px.y >= height) { std::cerr << "--pick-all: pixel " << px.x << "," << px.y << " is outside the " << width << " x " << height << " image" << std::endl; return 2; }
    for (const int2& px : picks)
        if (px.x < 0 || px.y < 0 || px.x >= width || px.y >= height) { std::cerr << "--pick: pixel " << px.x << "," << px.y << " is outside the " << width << " x " << height << " image" << std::endl; return 2; }
    if ((ao_samples > 0) != !ao_out.empty()) { std::cerr << "--ao and --ao-out go together" << std::endl; return 2; }
    if (move_history && move.empty()) { std::cerr << "--move-history needs --move" << std::endl; return 2; }
    const bool until_error = until.threshold > 0.0f;
    if (!error_out.empty() && !until_error) { std::cerr << "--error-out needs --until-error" << std::endl; return 2; }
    std::vector<std::string> key_list;
    { std::stringstream ss(keys); std::string k; while (std::getline(ss, k, ',')) if (!k.empty()) key_list.push_back(k); }

    TinyObjWrapper obj(objfilepath);
    if (!obj.loaded()) return 1;
    std::vector<float> moved_vertices;          // --move: the scene's vertices after the move
    if (!move.empty()) {
        const size_t colon = move.rfind(':');
        float d[3];
        if (colon == std::string::npos || sscanf(move.c_str() + colon + 1, "%f,%f,%f", &d[0], &d[1], &d[2]) != 3) {
            std::cerr << "--move material:dx,dy,dz" << std::endl;
            return 2;
        }
        const std::string name = move.substr(0, colon);
        const std::vector<std::string>& names = obj.getMaterialNames();
        const size_t id = (size_t)(std::find(names.begin(), names.end(), name) - names.begin());
        if (id == names.size()) { std::cerr << "--move: no material named '" << name << "' in " << objfilepath << std::endl; return 2; }
        moved_vertices = obj.getVerticesFloat();
        const std::vector<uint32_t> idx = obj.getIndexBuffer(), mat = obj.getMaterialIndices();
        std::vector<uint8_t> moves(moved_vertices.size() / 4, 0);
        for (size_t t = 0; t < mat.size(); t++)
            if (mat[t] == (uint32_t)id) moves[idx[3 * t]] = moves[idx[3 * t + 1]] = moves[idx[3 * t + 2]] = 1;
        for (size_t v = 0; v < moves.size(); v++)
            if (moves[v]) for (int k = 0; k < 3; k++) moved_vertices[4 * v + k] += d[k];
    }
    std::vector<Material> edited_materials;     // --set-material: the table after every edit
    if (!material_edits.empty()) {
        edited_materials = obj.getMaterials();
        for (const std::string& spec : material_edits) {
            std::string why;
            if (!applyMaterialEdit(spec, obj.getMaterialNames(), edited_materials, why)) {
                std::cerr << "--set-material: " << why << " (" << objfilepath << ")" << std::endl;
                return 1;
            }
        }
    }
    state.params.width = width;
    state.params.height = height;
    try {
        initCamera();
        g_camera.setAspectRatio(static_cast<float>(state.params.width) / static_cast<float>(state.params.height));
        if (orbit_dx || orbit_dy || zoom_steps) {
            Trackball trackball;
            trackball.setCamera(&g_camera);
            trackball.setMoveSpeed(10.0f);
            trackball.setReferenceFrame(make_float3(1.0f, 0.0f, 0.0f), make_float3(0.0f, 0.0f, 1.0f), make_float3(0.0f, 1.0f, 0.0f));
            trackball.setGimbalLock(true);
            if (orbit_dx || orbit_dy) { trackball.startTracking(0, 0); trackball.updateTracking(orbit_dx, orbit_dy, width, height); }
            for (int z = 0; z < std::abs(zoom_steps); z++) trackball.wheelEvent(zoom_steps > 0 ? 1 : -1);
        }
        const float3 eye = g_camera.eye();
        state.params.cameraEye = {eye.x, eye.y, eye.z};
        float3 U, V, W;
        g_camera.UVWFrame(U, V, W);
        state.params.cameraU = {U.x, U.y, U.z}; state.params.cameraV = {V.x, V.y, V.z}; state.params.cameraW = {W.x, W.y, W.z};

        std::cout << "Using Direct Lighting: " << (state.params.useDirectLighting ? "yes" : "no") << std::endl;
        std::cout << "Using Importance Sampling: " << (state.params.useImportanceSampling ? "yes" : "no") << std::endl;
        createDeviceContext(state);
        PT_CHECK(state.context, pt_set_build_mode(state.context, build_mode));
        PT_CHECK(state.context, pt_set_sample_chunks(state.context, sample_chunks));
        PT_CHECK(state.context, pt_set_light_mode(state.context, light_mode));
        PT_CHECK(state.context, pt_set_material_model(state.context, material_model));
        PT_CHECK(state.context, pt_set_math_mode(state.context, math_mode));
        if (!env_path.empty()) {
            std::vector<float> env_rgb;
            int ew = 0, eh = 0;
            std::string why;
            if (!acgpt::loadEnvironment(env_path, env_rgb, ew, eh, why)) throw Exception(why);
            PT_CHECK(state.context, pt_set_environment(state.context, env_rgb.data(), (uint32_t)ew, (uint32_t)eh, pt_float3{env_scale, env_scale, env_scale}));
            std::cout << "Environment map: " << env_path << " (" << ew << " x " << eh << ", scale " << env_scale << ")" << std::endl;
        }
        buildTheAccelarationStructure(state, obj);
        std::cout << "Acceleration Structure Built" << std::endl;
        createModule(state);
        std::cout << "Module Created" << std::endl;
        createProgramGroups(state);
        std::cout << "Program Groups Created" << std::endl;
        createPipeline(state);
        std::cout << "Pipeline Created" << std::endl;
        createShaderBindingTable(state, obj);
        std::cout << "Shader Binding Table Created" << std::endl;
        initializeTheLaunch(state);
        if (no_area_light) state.params.areaLight.emission = {0.0f, 0.0f, 0.0f};
        std::cout << "Launch Initialized" << std::endl;
        if (!picks.empty()) { std::cout.flush(); pickPixels(state, obj, picks); }
        if (!pickAlls.empty()) { std::cout.flush(); pickAllPixels(state, obj, pickAlls); }
        if (!nearest.empty()) { std::cout.flush(); nearestPoints(state, obj, nearest); }
        if (!nearestKs.empty()) { std::cout.flush(); nearestKPoints(state, obj, nearestKs); }
        if (!withins.empty()) { std::cout.flush(); withinPoints(state, withins); }
        if (!windings.empty()) { std::cout.flush(); windingPoints(state, windings); }
        if (!clearances.empty()) { std::cout.flush(); clearanceSegments(state, obj, clearances); }
        if (!triDistances.empty()) { std::cout.flush(); triangleDistances(state, obj, triDistances); }
        if (!collides.empty()) { std::cout.flush(); collideMeshes(state, collides); }
        if (!overlaps.empty()) { std::cout.flush(); overlapBoxes(state, obj, overlaps); }
        if (!oriented_overlaps.empty()) { std::cout.flush(); overlapBoxes(state, obj, oriented_overlaps, true); }
        if (!intersects.empty()) { std::cout.flush(); intersectTriangles(state, intersects); }
        if (!sweeps.empty()) { std::cout.flush(); sweepSpheres(state, obj, sweeps); }
        if (!capsuleCasts.empty()) { std::cout.flush(); castCapsules(state, obj, capsuleCasts); }
        if (!boxCasts.empty()) { std::cout.flush(); castBoxes(state, obj, boxCasts); }
        if (!casts.empty()) { std::cout.flush(); castTriangles(state, obj, casts); }
        if (!castMeshList.empty()) { std::cout.flush(); castMeshes(state, obj, castMeshList); }
        if (ao_samples > 0) ambientOcclusion(state, ao_samples, ao_radius, ao_bias, ao_frames, ao_out);
        HistoryFile history;
        if (!history_in.empty()) {              // refused before any frame is rendered
            history = readHistory(history_in);
            const std::string why = historyMismatch(history, historyOfRun(state, light_mode, math_mode, material_model));
            if (!why.empty()) throw Exception(history_in + " was made under other settings: " + why);
        }
        if (!restore_accum.empty()) {
            restoreAccumulation(state, restore_accum);
            std::cout << "Accumulation restored: " << state.params.currentFrameIdx << " frames" << std::endl;
        }
        if (state.gpus > 1 || state.multi) std::cout << "Devices: " << pt_device_count(state.context) << std::endl;
        uint64_t rays = 0;
        std::string stop_line;                  // --until-error: printed last
        pt_update_info moved = {0.0f, 0.0f, 0u, 0u}, material_update = {0.0f, 0.0f, 0u, 0u};
        {
            OutputBuffer<uchar4> output_buffer(zero_copy ? OutputBufferType::ZERO_COPY : OutputBufferType::DEVICE,
                                               state.params.width, state.params.height);
            size_t next_key = 0;
            const size_t n_pixels = (size_t)width * height;
            void* conv_state = nullptr; void* conv_error = nullptr;          // --until-error: the estimate's state and its error map
            pt_convergence_info conv_info;
            bool conv_done = false;
            memset(&conv_info, 0, sizeof(conv_info));
            if (until_error) {
                PT_CHECK(state.context, pt_device_malloc(state.context, &conv_state, n_pixels * 16));
                PT_CHECK(state.context, pt_device_memset(state.context, conv_state, 0, n_pixels * 16));
                if (!error_out.empty()) PT_CHECK(state.context, pt_device_malloc(state.context, &conv_error, n_pixels * 4));
            }
            for (int f = 0; f < frames;) {
                auto start = std::chrono::high_resolution_clock::now();
                if (next_key < key_list.size() && f > 0) { if (!keyCallback(state, key_list[next_key++])) break; }
                updateState(output_buffer, state);
                // a batch never crosses a key press or a dump point
                int batch = key_list.empty() ? std::min(fuse, frames - f) : 1;
                if (dump_every > 0) batch = std::min(batch, dump_every - f % dump_every);
                LaunchCurrentFrame(output_buffer, state, (uint32_t)batch);
                state.params.currentFrameIdx += (uint32_t)batch;
                f += batch - 1;
                auto end = std::chrono::high_resolution_clock::now();
                const double ms = std::chrono::duration<double, std::milli>(end - start).count();
                avg_ms += ms; total_ms += ms;
                sample_summ += samples_per_launch * batch;
                frame_counter += batch;
                pt_stats st; pt_get_stats(state.context, &st);
                rays += st.radiance_rays + st.shadow_rays;
                std::cout << "\rFrame Render Time: " << (long)ms << "ms" << std::flush;
                if (dump_every > 0 && (f + 1) % dump_every == 0 && f + 1 < frames) {
                    std::stringstream nm; nm << out << "." << (f + 1) << ".ppm";
                    saveImage(nm.str(), reinterpret_cast<const uint8_t*>(output_buffer.getHostPointer()), width, height);
                }
                f++;
                if (until_error) {              // one update per launch; a key press that reset the accumulation restarts the estimate by itself
                    PT_CHECK(state.context, pt_convergence_update(state.context, &state.params, state.params.currentFrameIdx, &until, (float*)conv_state,
                                                                  (float*)conv_error, nullptr, &conv_info));
                    if (conv_info.unmeasured_pixels == 0u && conv_info.invalid_pixels == 0u &&
                        (uint64_t)conv_info.converged_pixels * 1000u >= (uint64_t)conv_info.measured_pixels * until.quantile_permille) { conv_done = true; break; }
                }
            }
            std::cout << std::endl;
            if (until_error) {
                if (!error_out.empty()) {
                    std::vector<float> err(n_pixels), grey(n_pixels * 3);
                    PT_CHECK(state.context, pt_copy_to_host(state.context, err.data(), conv_error, n_pixels * sizeof(float)));
                    for (size_t i = 0; i < n_pixels; i++) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = err[i];
                    if (!savePFM(error_out, grey.data(), width, height, 3)) std::cerr << "could not write " << error_out << std::endl;
                }
                pt_device_free(state.context, conv_state);
                if (conv_error) pt_device_free(state.context, conv_error);
                std::stringstream line;
                line << "Stopped after " << state.params.currentFrameIdx << " of " << frames << " frames: " << until.quantile_permille << " permille error "
                     << conv_info.quantile_error << ", " << conv_info.converged_pixels << " of " << conv_info.measured_pixels << " pixels at or below "
                     << until.threshold << (conv_done ? " (converged)" : " (frame cap)");
                stop_line = line.str();
            }
            void* filtered = nullptr;               // --firefly: the image the outputs below see instead of the accumulation
            if (firefly.ratio > 0.0f) {
                pt_firefly_info fi;
                void* fb = nullptr;
                std::vector<uint8_t> host(n_pixels * 4);
                PT_CHECK(state.context, pt_device_malloc(state.context, &filtered, n_pixels * 16));
                PT_CHECK(state.context, pt_device_malloc(state.context, &fb, n_pixels * 4));
                PT_CHECK(state.context, pt_firefly_filter(state.context, state.params.accumulationBuffer, (uint32_t)width, (uint32_t)height, &firefly,
                                                          (float*)filtered, &fi));
                PT_CHECK(state.context, pt_resolve_framebuffer(state.context, (const float*)filtered, (uint8_t*)fb, n_pixels));
                PT_CHECK(state.context, pt_copy_to_host(state.context, host.data(), fb, n_pixels * 4));
                pt_device_free(state.context, fb);
                std::cout << "Firefly filter: " << fi.clamped_pixels << " clamped, " << fi.replaced_pixels << " replaced, " << fi.passed_pixels
                          << " passed; removed share " << (fi.total_luma_q16 ? (double)fi.removed_luma_q16 / (double)fi.total_luma_q16 : 0.0)
                          << ", max ratio " << fi.max_ratio << std::endl;
                if (!saveImage(out, host.data(), width, height)) std::cerr << "could not write " << out << std::endl;
            } else if (!saveImage(out, reinterpret_cast<const uint8_t*>(output_buffer.getHostPointer()), width, height))
                std::cerr << "could not write " << out << std::endl;
            const float* shown = filtered ? (const float*)filtered : state.params.accumulationBuffer;
            if (!save_accum.empty()) saveAccumulation(state, save_accum);
            if (!out_hdr.empty()) {
                std::vector<float> host((size_t)width * height * 4);
                if (use_bloom) {                    // the glare at the exposure the display image of `shown` gets
                    void* glared = nullptr; void* fb = nullptr;
                    pt_display_info di; pt_bloom_info bi; std::string err;
                    PT_CHECK(state.context, pt_device_malloc(state.context, &glared, n_pixels * 16));
                    PT_CHECK(state.context, pt_device_malloc(state.context, &fb, n_pixels * 4));
                    bloomForDisplay(state, shown, display_params, bloom, (float*)glared, fb, di, bi, err);
                    if (err.empty() && pt_copy_to_host(state.context, host.data(), glared, host.size() * sizeof(float)) != 0) err = pt_last_error(state.context);
                    pt_device_free(state.context, fb); pt_device_free(state.context, glared);
                    if (!err.empty()) throw Exception("bloom: " + err);
                } else {
                    PT_CHECK(state.context, pt_copy_to_host(state.context, host.data(), shown, host.size() * sizeof(float)));
                }
                if (!savePFM(out_hdr, host.data(), width, height, 4)) std::cerr << "could not write " << out_hdr << std::endl;
            }
            if (denoise_iters > 0) saveDenoised(state, denoisedName(out), (uint32_t)denoise_iters, display ? &display_params : nullptr, suffixedName(out, "_display"),
                                                (const float*)filtered, use_bloom ? &bloom : nullptr);
            else if (display) saveDisplay(state, suffixedName(out, "_display"), shown, display_params, use_bloom ? &bloom : nullptr);
            if (filtered) pt_device_free(state.context, filtered);
            if (!history_in.empty() || !history_out.empty()) {
                HistoryFile mine = historyOfRun(state, light_mode, math_mode, material_model);      // the settings at the end: --keys may have changed them
                if (!history_in.empty()) {
                    const std::string why = historyMismatch(history, mine);
                    if (!why.empty()) throw Exception(history_in + " was made under other settings: " + why);
                    blendHistory(state, history, out, (uint32_t)denoise_iters, mine.data);
                } else {
                    const size_t n = (size_t)width * height * 4;
                    mine.data.resize(n);
                    PT_CHECK(state.context, pt_copy_to_host(state.context, mine.data.data(), state.params.accumulationBuffer, n * sizeof(float)));
                    const float samples = (float)(state.params.currentFrameIdx * state.params.samplesPerPixel);
                    for (size_t i = 3; i < n; i += 4) mine.data[i] = samples;
                }
                if (!history_out.empty()) writeHistory(history_out, mine);
            }
            if (!moved_vertices.empty()) {          // --move: refit, then the same frames again from zero
                MovedHistory kept;
                if (move_history) kept.keep(state);
                PT_CHECK(state.context, pt_update_vertices(state.context, moved_vertices.data(), moved_vertices.size() / 4, PT_UPDATE_REFIT, &moved));
                state.params.handle = pt_scene_handle(state.context);
                state.params.currentFrameIdx = 0u;
                PT_CHECK(state.context, pt_device_memset(state.context, state.params.accumulationBuffer, 0,
                                                         (size_t)state.params.width * state.params.height * 4 * sizeof(float)));
                for (int f = 0; f < frames;) {
                    const int batch = std::min(fuse, frames - f);
                    LaunchCurrentFrame(output_buffer, state, (uint32_t)batch);
                    state.params.currentFrameIdx += (uint32_t)batch;
                    f += batch;
                }
                const std::string name = suffixedName(out, "_moved");
                if (!saveImage(name, reinterpret_cast<const uint8_t*>(output_buffer.getHostPointer()), width, height))
                    std::cerr << "could not write " << name << std::endl;
                if (move_history) kept.blend(state, obj.getVerticesFloat(), moved_vertices, out, (uint32_t)denoise_iters);
            }
            if (!edited_materials.empty()) {        // --set-material: the new table, then the same frames again from zero
                PT_CHECK(state.context, pt_update_materials(state.context, reinterpret_cast<const pt_material*>(edited_materials.data()),
                                                            edited_materials.size(), nullptr, 0, &material_update));
                state.params.handle = pt_scene_handle(state.context);
                state.params.currentFrameIdx = 0u;
                PT_CHECK(state.context, pt_device_memset(state.context, state.params.accumulationBuffer, 0,
                                                         (size_t)state.params.width * state.params.height * 4 * sizeof(float)));
                for (int f = 0; f < frames;) {
                    const int batch = std::min(fuse, frames - f);
                    LaunchCurrentFrame(output_buffer, state, (uint32_t)batch);
                    state.params.currentFrameIdx += (uint32_t)batch;
                    f += batch;
                }
                const std::string name = suffixedName(out, "_material");
                if (!saveImage(name, reinterpret_cast<const uint8_t*>(output_buffer.getHostPointer()), width, height))
                    std::cerr << "could not write " << name << std::endl;
            }
        }
        CleanAllTheThings(state);
        if (frame_counter > 0) avg_ms /= frame_counter;
        std::cout << "Total Samples " << sample_summ << std::endl;
        std::cout << "Average ms per frame: " << (long)avg_ms << std::endl;
        std::cout << "Total ms: " << (long)total_ms << std::endl;
        std::cout << "Rays: " << rays << "  Mray/s: " << (total_ms > 0 ? rays / total_ms / 1e3 : 0.0) << std::endl;
        if (!moved_vertices.empty()) std::cout << "Refit: " << moved.ms << " ms  area ratio: " << moved.area_ratio << std::endl;
        if (!edited_materials.empty()) std::cout << "Material update: " << material_update.ms << " ms" << std::endl;
        if (!stop_line.empty()) std::cout << stop_line << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "Caught exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
