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
// --pick ... --cast-mesh, the query options: what each takes, calls and prints is told at its entry in QueryCommands.cpp.
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
#include "PathTracerState.h"                            // struct PathTracerState, :71-93
#include "QueryCommands.h"
#include "TinyObjWrapper.h"
#include "Trackball.h"

using namespace acgpt;

constexpr unsigned int maxiumumRecursionDepth = 28;     // PathTracerMain.cpp:42
static int32_t samples_per_launch = 128;                // :43
static uint32_t frame_counter = 0, sample_summ = 0;
static double avg_ms = 0.0, total_ms = 0.0;
static bool refreshAccumulationBuffer = false;
static Camera g_camera;

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
    const size_t bytes = (size_t)state.params.width * state.params.height * 4 * sizeof(float);
    state.accumulation = DeviceBuffer(state.context, bytes, "accumulation buffer");
    state.params.accumulationBuffer = state.accumulation.as<float>();
    // zero-filled: with pt_set_partition(rank, world) the pixels of other ranks are never written and the
    // cross-rank reduce(SUM) relies on them being 0 (the reference's single-GPU cudaMalloc leaves them undefined)
    PT_CHECK(state.context, pt_device_memset(state.context, state.accumulation.get(), 0, bytes));
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
        state.accumulation.reset();
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
// frame buffer, fb, is discarded).  Returns the exposure; a failing call throws under the caller's name, `what`.
static float bloomForDisplay(PathTracerState& state, const float* src, const pt_display_params& dp, const pt_bloom_params& bloom, float* dst, void* fb,
                             pt_display_info& info, pt_bloom_info& bi, const char* what)
{
    const size_t n = (size_t)state.params.width * state.params.height;
    memset(&info, 0, sizeof(info));
    info.exposure = dp.exposure;
    if (!(dp.exposure > 0.0f)) ptRequire(state.context, pt_display_transform(state.context, src, n, &dp, nullptr, (uint8_t*)fb, &info), what);
    pt_bloom_params bp = bloom;
    bp.threshold = bloom.threshold / info.exposure; bp.knee = bloom.knee / info.exposure; bp.clamp = bloom.clamp / info.exposure;
    ptRequire(state.context, pt_bloom(state.context, src, state.params.width, state.params.height, &bp, dst, &bi), what);
    return info.exposure;
}

// src (DEVICE float4[width * height], linear) through pt_display_transform, written as an image (--tonemap, --exposure); with bloom,
// through pt_bloom first
static void saveDisplay(PathTracerState& state, const std::string& path, const float* src, const pt_display_params& dp, const pt_bloom_params* bloom = nullptr)
{
    const size_t n = (size_t)state.params.width * state.params.height;
    const char* what = "display transform";
    pt_display_info info;
    pt_bloom_info bi;
    std::vector<uint8_t> host(n * 4);
    DeviceBuffer fb(state.context, n * 4, what);
    if (bloom) {
        DeviceBuffer glared(state.context, n * 16, what);
        pt_display_params manual = dp;
        manual.exposure = bloomForDisplay(state, src, dp, *bloom, glared.as<float>(), fb.get(), info, bi, what);
        ptRequire(state.context, pt_display_transform(state.context, glared.as<float>(), n, &manual, nullptr, fb.as<uint8_t>(), nullptr), what);
    } else
        ptRequire(state.context, pt_display_transform(state.context, src, n, &dp, nullptr, fb.as<uint8_t>(), &info), what);
    fb.download(host.data(), n * 4);
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
    const char* what = "denoise";
    DeviceBuffer albedo_prim(state.context, n * 16, what), normal_depth(state.context, n * 16, what), denoised(state.context, n * 16, what), colours(state.context, n * 4, what);
    std::vector<uint8_t> host(n * 4);
    ptRequire(state.context, pt_render_features(state.context, &state.params, albedo_prim.as<float>(), normal_depth.as<float>()), what);
    ptRequire(state.context, pt_denoise(state.context, &params, albedo_prim.as<float>(), normal_depth.as<float>(), denoised.as<float>(), iterations), what);
    ptRequire(state.context, pt_resolve_framebuffer(state.context, denoised.as<float>(), colours.as<uint8_t>(), n), what);
    colours.download(host.data(), n * 4);
    if (dp) {
        try { saveDisplay(state, display_path, denoised.as<float>(), *dp, bloom); } catch (const std::exception& e) { throw Exception(std::string("denoise: ") + e.what()); }
    }
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

// a blended history (DEVICE float4[width * height]) coloured by pt_resolve_framebuffer as <out><suffix>, and with denoise_iters > 0
// through pt_denoise, guided by this view's features, as <out><suffix>_denoised; every device call comes before the first file
static void saveBlend(PathTracerState& state, const char* what, const DeviceBuffer& blend, const DeviceBuffer& albedo_prim, const DeviceBuffer& normal_depth,
                      const std::string& out, const std::string& suffix, uint32_t denoise_iters)
{
    const pt_params& p = state.params;
    const size_t n = (size_t)p.width * p.height;
    DeviceBuffer denoised(state.context, n * 16, what), colours(state.context, n * 4, what);
    std::vector<uint8_t> host(n * 4), host_dn(n * 4);
    pt_params dn = p;
    dn.accumulationBuffer = blend.as<float>();                    // pt_denoise reads the blend's .xyz
    ptRequire(state.context, pt_resolve_framebuffer(state.context, blend.as<float>(), colours.as<uint8_t>(), n), what);
    colours.download(host.data(), n * 4);
    if (denoise_iters > 0) {
        ptRequire(state.context, pt_denoise(state.context, &dn, albedo_prim.as<float>(), normal_depth.as<float>(), denoised.as<float>(), denoise_iters), what);
        ptRequire(state.context, pt_resolve_framebuffer(state.context, denoised.as<float>(), colours.as<uint8_t>(), n), what);
        colours.download(host_dn.data(), n * 4);
    }
    const std::string name = suffixedName(out, suffix);
    if (!saveImage(name, host.data(), (int)p.width, (int)p.height)) std::cerr << "could not write " << name << std::endl;
    if (denoise_iters > 0) {
        const std::string dname = suffixedName(out, suffix + "_denoised");
        if (!saveImage(dname, host_dn.data(), (int)p.width, (int)p.height)) std::cerr << "could not write " << dname << std::endl;
    }
}

// blends the history of the view in `file` into this run's view (pt_temporal_blend), writes <out>_temporal (and _temporal_denoised);
// the blended history comes back in `blended`
static void blendHistory(PathTracerState& state, const HistoryFile& file, const std::string& out, uint32_t denoise_iters, std::vector<float>& blended)
{
    const pt_params& p = state.params;
    const size_t n = (size_t)p.width * p.height, n_prev = (size_t)file.hdr[0] * file.hdr[1];
    const char* what = "temporal blend";
    pt_params prev = p;
    prev.width = file.hdr[0]; prev.height = file.hdr[1];
    pt_float3* cam[4] = {&prev.cameraEye, &prev.cameraU, &prev.cameraV, &prev.cameraW};
    for (int i = 0; i < 4; i++) *cam[i] = {file.camera[3 * i], file.camera[3 * i + 1], file.camera[3 * i + 2]};
    DeviceBuffer prev_history(state.context, n_prev * 16, what), prev_albedo(state.context, n_prev * 16, what), prev_normal(state.context, n_prev * 16, what);
    DeviceBuffer albedo_prim(state.context, n * 16, what), normal_depth(state.context, n * 16, what), blend(state.context, n * 16, what);
    blended.assign(n * 4, 0.0f);
    prev_history.upload(file.data.data(), n_prev * 16);
    ptRequire(state.context, pt_render_features(state.context, &prev, prev_albedo.as<float>(), prev_normal.as<float>()), what);
    ptRequire(state.context, pt_render_features(state.context, &p, albedo_prim.as<float>(), normal_depth.as<float>()), what);
    ptRequire(state.context, pt_temporal_blend(state.context, &p, p.currentFrameIdx * p.samplesPerPixel, albedo_prim.as<float>(), normal_depth.as<float>(), &prev,
                                               prev_history.as<float>(), prev_albedo.as<float>(), prev_normal.as<float>(), PT_TEMPORAL_HISTORY_CAP, blend.as<float>()), what);
    blend.download(blended.data(), n * 16);
    saveBlend(state, what, blend, albedo_prim, normal_depth, out, "_temporal", denoise_iters);
}

// --move-history: the view before the refit (accumulation as {rgb, frames * spp}, features), carried into the moved scene after it
struct MovedHistory {
    pt_params prev = {};
    DeviceBuffer history, albedo_prim, normal_depth;      // of the view before the move

    void keep(PathTracerState& s)
    {
        prev = s.params;
        const size_t n = (size_t)prev.width * prev.height;
        const char* what = "move history";
        history = DeviceBuffer(s.context, n * 16, what); albedo_prim = DeviceBuffer(s.context, n * 16, what); normal_depth = DeviceBuffer(s.context, n * 16, what);
        std::vector<float> host(n * 4);
        PT_CHECK(s.context, pt_copy_to_host(s.context, host.data(), prev.accumulationBuffer, n * 16));
        const float samples = (float)(prev.currentFrameIdx * prev.samplesPerPixel);
        for (size_t i = 3; i < host.size(); i += 4) host[i] = samples;
        history.upload(host.data(), n * 16);
        PT_CHECK(s.context, pt_render_features(s.context, &prev, albedo_prim.as<float>(), normal_depth.as<float>()));
    }

    // writes <out>_moved_temporal (and _moved_temporal_denoised); `before` / `after`: the vertices of the two views
    void blend(PathTracerState& s, const std::vector<float>& before, const std::vector<float>& after, const std::string& out, uint32_t denoise_iters)
    {
        const pt_params& p = s.params;
        const size_t n = (size_t)p.width * p.height, vbytes = before.size() * sizeof(float);
        const char* what = "moved temporal blend";
        DeviceBuffer albedo_now(s.context, n * 16, what), normal_now(s.context, n * 16, what), blended(s.context, n * 16, what);
        DeviceBuffer vertices_now(s.context, vbytes, what), vertices_before(s.context, vbytes, what);
        vertices_now.upload(after.data(), vbytes);
        vertices_before.upload(before.data(), vbytes);
        ptRequire(s.context, pt_render_features(s.context, &p, albedo_now.as<float>(), normal_now.as<float>()), what);
        ptRequire(s.context, pt_temporal_blend_motion(s.context, &p, p.currentFrameIdx * p.samplesPerPixel, albedo_now.as<float>(), normal_now.as<float>(), &prev,
                                                      history.as<float>(), albedo_prim.as<float>(), normal_depth.as<float>(), vertices_now.as<float>(),
                                                      vertices_before.as<float>(), before.size() / 4, PT_TEMPORAL_HISTORY_CAP, PT_TEMPORAL_CLIP_GAMMA, blended.as<float>()), what);
        saveBlend(s, what, blended, albedo_now, normal_now, out, "_moved_temporal", denoise_iters);
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
    DeviceBuffer d_alb(state.context, n * 16, "ao"), d_nd(state.context, n * 16, "ao"), d_vis(state.context, n * 4, "ao"), d_ao(state.context, n * 4, "ao");
    std::vector<float> ao(n);
    ptRequire(state.context, pt_render_features(state.context, &p, d_alb.as<float>(), d_nd.as<float>()), "ao");
    for (int j = 0; j < frames; j++) {
        const pt_ao_params ap = {(uint32_t)K, radius, bias, (uint32_t)j, j > 0 ? 1u : 0u, (uint32_t)K * (uint32_t)(j + 1), {0u, 0u}};
        ptRequire(state.context, pt_ao_image(state.context, &p, d_nd.as<float>(), disk.data(), &ap, d_vis.as<uint32_t>(), d_ao.as<float>()), "ao");
    }
    d_ao.download(ao.data(), n * 4);
    std::vector<float> grey(n * 3);
    double sum = 0.0;
    for (size_t i = 0; i < n; i++) { grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = ao[i]; sum += ao[i]; }
    if (!savePFM(path, grey.data(), (int)p.width, (int)p.height, 3)) throw Exception("could not write " + path);
    std::cout << "Ambient occlusion: " << K << " x " << frames << " rays per pixel, radius " << radius << ", bias " << bias << ", mean " << sum / (double)n
              << " -> " << path << std::endl;
}

// after --move's refit or --set-material's new table: the same frames again from a zeroed accumulation, written as `name`
static void rerenderFromZero(PathTracerState& state, OutputBuffer<uchar4>& output_buffer, int frames, int fuse, const std::string& name)
{
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
    if (!saveImage(name, reinterpret_cast<const uint8_t*>(output_buffer.getHostPointer()), (int)state.params.width, (int)state.params.height))
        std::cerr << "could not write " << name << std::endl;
}

static void CleanAllTheThings(PathTracerState& state)                   // :629-646
{
    state.accumulation.reset();
    pt_destroy(state.context);
    state.context = nullptr;
}

int main(int argc, char** argv)
{
    std::string objfilepath, out = "frame.png", keys, save_accum, restore_accum, history_out, history_in, move;
    std::vector<std::string> material_edits;
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
        if (QueryCommand* query = findQueryCommand(a)) {
            if (!query->parse(next())) { std::cerr << query->usage << std::endl; return 2; }
            query->given++;
        }
        else if (a == "--obj") objfilepath = next();
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
    for (size_t c = queryCommands().size(); c-- > 0;) {        // what the image size decides; the later option's arguments first, as ever
        const QueryCommand& query = queryCommands()[c];
        const std::string why = query.check ? query.check(width, height) : std::string();
        if (!why.empty()) { std::cerr << why << std::endl; return 2; }
    }
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
        for (const QueryCommand& query : queryCommands())
            if (query.given) { std::cout.flush(); query.run(state, obj); }
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
            DeviceBuffer conv_state, conv_error;                            // --until-error: the estimate's state and its error map
            pt_convergence_info conv_info;
            bool conv_done = false;
            memset(&conv_info, 0, sizeof(conv_info));
            if (until_error) {
                conv_state = DeviceBuffer(state.context, n_pixels * 16, "until-error");
                PT_CHECK(state.context, pt_device_memset(state.context, conv_state.get(), 0, n_pixels * 16));
                if (!error_out.empty()) conv_error = DeviceBuffer(state.context, n_pixels * 4, "until-error");
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
                    PT_CHECK(state.context, pt_convergence_update(state.context, &state.params, state.params.currentFrameIdx, &until, conv_state.as<float>(),
                                                                  conv_error.as<float>(), nullptr, &conv_info));
                    if (conv_info.unmeasured_pixels == 0u && conv_info.invalid_pixels == 0u &&
                        (uint64_t)conv_info.converged_pixels * 1000u >= (uint64_t)conv_info.measured_pixels * until.quantile_permille) { conv_done = true; break; }
                }
            }
            std::cout << std::endl;
            if (until_error) {
                if (!error_out.empty()) {
                    std::vector<float> err(n_pixels), grey(n_pixels * 3);
                    conv_error.download(err.data(), n_pixels * sizeof(float));
                    for (size_t i = 0; i < n_pixels; i++) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = err[i];
                    if (!savePFM(error_out, grey.data(), width, height, 3)) std::cerr << "could not write " << error_out << std::endl;
                }
                conv_state.reset();
                conv_error.reset();
                std::stringstream line;
                line << "Stopped after " << state.params.currentFrameIdx << " of " << frames << " frames: " << until.quantile_permille << " permille error "
                     << conv_info.quantile_error << ", " << conv_info.converged_pixels << " of " << conv_info.measured_pixels << " pixels at or below "
                     << until.threshold << (conv_done ? " (converged)" : " (frame cap)");
                stop_line = line.str();
            }
            DeviceBuffer filtered;                  // --firefly: the image the outputs below see instead of the accumulation
            if (firefly.ratio > 0.0f) {
                pt_firefly_info fi;
                std::vector<uint8_t> host(n_pixels * 4);
                filtered = DeviceBuffer(state.context, n_pixels * 16, "firefly");
                DeviceBuffer fb(state.context, n_pixels * 4, "firefly");
                PT_CHECK(state.context, pt_firefly_filter(state.context, state.params.accumulationBuffer, (uint32_t)width, (uint32_t)height, &firefly,
                                                          filtered.as<float>(), &fi));
                PT_CHECK(state.context, pt_resolve_framebuffer(state.context, filtered.as<float>(), fb.as<uint8_t>(), n_pixels));
                fb.download(host.data(), n_pixels * 4);
                std::cout << "Firefly filter: " << fi.clamped_pixels << " clamped, " << fi.replaced_pixels << " replaced, " << fi.passed_pixels
                          << " passed; removed share " << (fi.total_luma_q16 ? (double)fi.removed_luma_q16 / (double)fi.total_luma_q16 : 0.0)
                          << ", max ratio " << fi.max_ratio << std::endl;
                if (!saveImage(out, host.data(), width, height)) std::cerr << "could not write " << out << std::endl;
            } else if (!saveImage(out, reinterpret_cast<const uint8_t*>(output_buffer.getHostPointer()), width, height))
                std::cerr << "could not write " << out << std::endl;
            const float* shown = filtered ? filtered.as<float>() : state.params.accumulationBuffer;
            if (!save_accum.empty()) saveAccumulation(state, save_accum);
            if (!out_hdr.empty()) {
                std::vector<float> host((size_t)width * height * 4);
                if (use_bloom) {                    // the glare at the exposure the display image of `shown` gets
                    DeviceBuffer glared(state.context, n_pixels * 16, "bloom"), fb(state.context, n_pixels * 4, "bloom");
                    pt_display_info di; pt_bloom_info bi;
                    bloomForDisplay(state, shown, display_params, bloom, glared.as<float>(), fb.get(), di, bi, "bloom");
                    glared.download(host.data(), host.size() * sizeof(float));
                } else {
                    PT_CHECK(state.context, pt_copy_to_host(state.context, host.data(), shown, host.size() * sizeof(float)));
                }
                if (!savePFM(out_hdr, host.data(), width, height, 4)) std::cerr << "could not write " << out_hdr << std::endl;
            }
            if (denoise_iters > 0) saveDenoised(state, denoisedName(out), (uint32_t)denoise_iters, display ? &display_params : nullptr, suffixedName(out, "_display"),
                                                filtered.as<float>(), use_bloom ? &bloom : nullptr);
            else if (display) saveDisplay(state, suffixedName(out, "_display"), shown, display_params, use_bloom ? &bloom : nullptr);
            filtered.reset();
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
                rerenderFromZero(state, output_buffer, frames, fuse, suffixedName(out, "_moved"));
                if (move_history) kept.blend(state, obj.getVerticesFloat(), moved_vertices, out, (uint32_t)denoise_iters);
            }
            if (!edited_materials.empty()) {        // --set-material: the new table, then the same frames again from zero
                PT_CHECK(state.context, pt_update_materials(state.context, reinterpret_cast<const pt_material*>(edited_materials.data()),
                                                            edited_materials.size(), nullptr, 0, &material_update));
                rerenderFromZero(state, output_buffer, frames, fuse, suffixedName(out, "_material"));
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
