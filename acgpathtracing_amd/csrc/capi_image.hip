// capi_image.hip — the entry points of include/acgpt.h that work on a finished image: first-hit features and the denoiser, the
// metered stages (display transform, convergence estimate, firefly filter, bloom), temporal reprojection.  Host code only; the
// kernels are in the stage's own .hip.  The context and what the units share: context.h.
#include <cmath>
#include <cstring>

#include "context.h"
#include "bloom.h"
#include "convergence.h"
#include "denoise.h"
#include "display.h"
#include "firefly.h"
#include "image_common.h"
#include "temporal.h"

// ---- denoised preview (pt_render_features, pt_denoise; kernels in denoise.hip) -------------------------------------------------
static int check_image(pt_ctx* c, const pt_params* p, const char* what)
{
    if (p->width == 0 || p->height == 0) return fail(c, std::string(what) + ": width and height must be >= 1");
    if (p->width > 65535u || p->height > 65535u || (uint64_t)p->width * p->height > (1ull << 28))
        return fail(c, std::string(what) + ": image too large (65535 per side, 2^28 pixels)");
    return 0;
}

PT_API int pt_render_features(pt_ctx* c, const pt_params* p, float* albedo_prim, float* normal_depth)
{
    if (!c) return fail(nullptr, "pt_render_features: null context");
    if (!p || !albedo_prim || !normal_depth) return fail(c, "pt_render_features: null argument");
    if (int rc = check_image(c, p, "pt_render_features")) return rc;
    const size_t bytes = (size_t)p->width * p->height * sizeof(float4);
    if (spans_overlap(albedo_prim, bytes, normal_depth, bytes)) return fail(c, "pt_render_features: the two output buffers overlap");
    if (c->scene_serial == 0) return fail(c, "pt_render_features: no scene (pt_set_scene first)");
    CK(c, hipSetDevice(c->device));
    // the node array the scene holds: fp16 centre / half-extent nodes for the default variants, fp32 nodes for the fp32 ones; only a
    // variant forced onto another format (pt_set_tuning) leaves neither, and gets the fp32 nodes back as a ray query would
    int fmt = 0;
    if (c->bvh.hcnodes) fmt = 11;
    else if (int rc = ensure_node_format(c, 0)) return rc;
    Range range("pt_render_features");
    CK(c, ptd::launch_features(fmt, device_scene(c), c->stack_entries, p->width, p->height, p->cameraEye, p->cameraU, p->cameraV, p->cameraW,
                               (float4*)albedo_prim, (float4*)normal_depth, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_denoise(pt_ctx* c, const pt_params* p, const float* albedo_prim, const float* normal_depth, float* out_rgba, uint32_t iterations)
{
    if (!c) return fail(nullptr, "pt_denoise: null context");
    if (!p || !p->accumulationBuffer || !albedo_prim || !normal_depth || !out_rgba) return fail(c, "pt_denoise: null argument");
    if (iterations < 1u || iterations > ptd::kDnMaxIterations) return fail(c, "pt_denoise: iterations must be in [1, 8]");
    if (int rc = check_image(c, p, "pt_denoise")) return rc;
    const size_t n = (size_t)p->width * p->height, bytes = n * sizeof(float4);
    if (spans_overlap(out_rgba, bytes, p->accumulationBuffer, bytes) || spans_overlap(out_rgba, bytes, albedo_prim, bytes) ||
        spans_overlap(out_rgba, bytes, normal_depth, bytes))
        return fail(c, "pt_denoise: out_rgba overlaps an input (writing into the accumulation buffer would corrupt the progressive state)");
    CK(c, hipSetDevice(c->device));
    for (DevBuf<float4>& b : c->d_denoise) CK(c, b.reserve(n, c->stream));
    Range range("pt_denoise");
    CK(c, ptd::launch_denoise((const float4*)p->accumulationBuffer, (const float4*)albedo_prim, (const float4*)normal_depth, p->width, p->height, iterations,
                              c->d_denoise[0].p, c->d_denoise[1].p, (float4*)out_rgba, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the metered stages (display, convergence, firefly, bloom) -----------------------------------------------------------------------
// Each keeps a small state on the device: live counts, which the stage's last kernel clears after it has read them, and the record
// that kernel writes.  run_metered allocates the state on first use, zeroes it when it is new or dirty (an earlier call failed half
// way), runs launch(state), copies the record to `info` if there is one, and synchronises.  fn: the entry point's name.
template <typename State, typename Info, typename F>
static int run_metered(pt_ctx* c, const char* fn, StageBuf<State>& st, Info* info, F launch)
{
    hipError_t e = hipSuccess;
    if (!st.p) { e = st.reserve(1, c->stream); st.dirty = true; }
    if (e == hipSuccess && st.dirty) e = hipMemsetAsync(st.p, 0, sizeof(State), c->stream);
    Range range(fn);
    st.dirty = true;                         // until the stage's last kernel has run to its end and cleared the counts
    if (e == hipSuccess) e = launch(st.p);
    if (e == hipSuccess && info) e = hipMemcpyAsync(info, &st.p->record, sizeof(Info), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, std::string(fn) + ": " + hipGetErrorString(e));
    st.dirty = false;
    return 0;
}

// ---- display transform (pt_display_transform; kernels in display.hip) ----------------------------------------------------------
static_assert(sizeof(pt_display_params) == 40 && sizeof(pt_display_info) == 16 + 4 * PT_DISPLAY_BINS, "pt_display_params / pt_display_info: a change of these layouts bumps pt_abi_version");

PT_API int pt_display_transform(pt_ctx* c, const float* src_rgba, size_t n_pixels, const pt_display_params* dp, float* out_rgba, uint8_t* framebuffer_rgba,
                                pt_display_info* info)
{
    const char* f = "pt_display_transform: ";
    if (!c) return fail(nullptr, std::string(f) + "null context");
    if (!src_rgba || !dp) return fail(c, std::string(f) + "null argument");
    if (!out_rgba && !framebuffer_rgba) return fail(c, std::string(f) + "out_rgba and framebuffer_rgba are both null");
    if (n_pixels < 1u || n_pixels > ((size_t)1 << 31)) return fail(c, std::string(f) + "n_pixels must be in [1, 2^31]");
    if (dp->tone_curve != PT_TONE_LINEAR && dp->tone_curve != PT_TONE_REINHARD && dp->tone_curve != PT_TONE_ACES) return fail(c, std::string(f) + "unknown tone curve");
    if (!std::isfinite(dp->exposure) || dp->exposure < 0.0f) return fail(c, std::string(f) + "exposure must be finite and >= 0 (0: automatic)");
    const bool automatic = !(dp->exposure > 0.0f);
    if (automatic) {
        if (!std::isfinite(dp->key) || !(dp->key > 0.0f)) return fail(c, std::string(f) + "key must be finite and > 0");
        if (dp->lo_permille >= dp->hi_permille || dp->hi_permille > 1000u) return fail(c, std::string(f) + "the metering window needs lo_permille < hi_permille <= 1000");
        if (!std::isfinite(dp->min_exposure) || !std::isfinite(dp->max_exposure) || !(dp->min_exposure > 0.0f) || !(dp->min_exposure <= dp->max_exposure))
            return fail(c, std::string(f) + "the exposure limits need 0 < min_exposure <= max_exposure, both finite");
        if (!std::isfinite(dp->prev_exposure) || dp->prev_exposure < 0.0f) return fail(c, std::string(f) + "prev_exposure must be finite and >= 0 (0: none)");
        if (!(dp->adapt >= 0.0f && dp->adapt <= 1.0f)) return fail(c, std::string(f) + "adapt must be in [0, 1]");
    }
    if (dp->tone_curve == PT_TONE_REINHARD && (!std::isfinite(dp->white) || !(dp->white > 0.0f))) return fail(c, std::string(f) + "white must be finite and > 0");
    if (out_rgba && spans_overlap(out_rgba, n_pixels * sizeof(float4), src_rgba, n_pixels * sizeof(float4))) return fail(c, std::string(f) + "out_rgba overlaps src_rgba");
    CK(c, hipSetDevice(c->device));
    const auto launch = [&](ptd::DisplayState* st) {
        return ptd::launch_display((const float4*)src_rgba, (uint64_t)n_pixels, *dp, st, (float4*)out_rgba, (uint32_t*)framebuffer_rgba, c->stream);
    };
    if (automatic) return run_metered(c, "pt_display_transform", c->d_display, info, launch);
    // a manual exposure: the apply kernel alone, the state neither read nor written
    Range range("pt_display_transform");
    CK(c, launch(c->d_display.p));
    if (info) { memset(info, 0, sizeof(*info)); info->exposure = dp->exposure; }
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- convergence estimate (pt_convergence_update; kernels in convergence.hip) --------------------------------------------------
static_assert(sizeof(pt_convergence_params) == 16 && sizeof(pt_convergence_info) == 32 + 4 * PT_CONVERGENCE_BINS,
              "pt_convergence_params / pt_convergence_info: a change of these layouts bumps pt_abi_version");

PT_API int pt_convergence_update(pt_ctx* c, const pt_params* p, uint32_t accum_frames, const pt_convergence_params* cp, float* state, float* out_error,
                                 float* out_tiles, pt_convergence_info* info)
{
    const std::string f("pt_convergence_update: ");
    if (!c) return fail(nullptr, f + "null context");
    if (!p || !cp || !state || !p->accumulationBuffer) return fail(c, f + "null argument");
    if (p->width == 0 || p->height == 0) return fail(c, f + "width and height must be >= 1");
    const uint64_t n = (uint64_t)p->width * p->height;
    if (n > (1ull << 31)) return fail(c, f + "image too large (2^31 pixels)");
    if (accum_frames < 1u || accum_frames > (1u << 24)) return fail(c, f + "accum_frames must be in [1, 2^24]");
    if (!std::isfinite(cp->lum_floor) || !(cp->lum_floor > 0.0f)) return fail(c, f + "lum_floor must be finite and > 0");
    if (!std::isfinite(cp->threshold) || !(cp->threshold > 0.0f)) return fail(c, f + "threshold must be finite and > 0");
    if (cp->quantile_permille < 1u || cp->quantile_permille > 1000u) return fail(c, f + "quantile_permille must be in [1, 1000]");
    if (cp->reserved != 0u) return fail(c, f + "reserved must be 0");
    const uint64_t tiles = ptd::tile_walk(p->width, p->height, ptd::kConvTile, ptd::kConvBlocks).tiles;
    const void* bufs[4] = {p->accumulationBuffer, state, out_error, out_tiles};
    const size_t sizes[4] = {(size_t)n * sizeof(float4), (size_t)n * sizeof(float4), (size_t)n * sizeof(float), (size_t)tiles * sizeof(float)};
    const char* names[4] = {"the accumulation buffer", "state", "out_error", "out_tiles"};
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (bufs[i] && bufs[j] && spans_overlap(bufs[i], sizes[i], bufs[j], sizes[j])) return fail(c, f + names[j] + " overlaps " + names[i]);
    CK(c, hipSetDevice(c->device));
    return run_metered(c, "pt_convergence_update", c->d_convergence, info, [&](ptd::ConvergenceState* st) {
        return ptd::launch_convergence((const float4*)p->accumulationBuffer, p->width, p->height, accum_frames, *cp, (float4*)state, out_error, out_tiles,
                                       st, c->stream);
    });
}

// ---- firefly filter (pt_firefly_filter; kernels in firefly.hip) -----------------------------------------------------------------
static_assert(sizeof(pt_firefly_params) == 16 && sizeof(pt_firefly_info) == 40, "pt_firefly_params / pt_firefly_info: a change of these layouts bumps pt_abi_version");

PT_API int pt_firefly_filter(pt_ctx* c, const float* src_rgba, uint32_t width, uint32_t height, const pt_firefly_params* fp, float* out_rgba, pt_firefly_info* info)
{
    const std::string f("pt_firefly_filter: ");
    if (!c) return fail(nullptr, f + "null context");
    if (!src_rgba || !fp || !out_rgba) return fail(c, f + "null argument");
    if (width == 0 || height == 0) return fail(c, f + "width and height must be >= 1");
    const uint64_t n = (uint64_t)width * height;
    if (n > (1ull << 31)) return fail(c, f + "image too large (2^31 pixels)");
    if (!std::isfinite(fp->ratio) || !(fp->ratio >= 1.0f)) return fail(c, f + "ratio must be finite and >= 1");
    if (!std::isfinite(fp->floor) || !(fp->floor > 0.0f)) return fail(c, f + "floor must be finite and > 0");
    if (fp->rank < 1u || fp->rank > 4u) return fail(c, f + "rank must be in [1, 4]");
    if (fp->radius < 1u || fp->radius > 2u) return fail(c, f + "radius must be 1 or 2");
    if (spans_overlap(src_rgba, (size_t)n * sizeof(float4), out_rgba, (size_t)n * sizeof(float4))) return fail(c, f + "out_rgba overlaps src_rgba");
    CK(c, hipSetDevice(c->device));
    return run_metered(c, "pt_firefly_filter", c->d_firefly, info, [&](ptd::FireflyState* st) {
        return ptd::launch_firefly((const float4*)src_rgba, width, height, *fp, (float4*)out_rgba, st, c->stream);
    });
}

// ---- bloom (pt_bloom; kernels in bloom.hip) -------------------------------------------------------------------------------------
static_assert(sizeof(pt_bloom_params) == 24 && sizeof(pt_bloom_info) == 40, "pt_bloom_params / pt_bloom_info: a change of these layouts bumps pt_abi_version");

PT_API int pt_bloom(pt_ctx* c, const float* src_rgba, uint32_t width, uint32_t height, const pt_bloom_params* bp, float* out_rgba, pt_bloom_info* info)
{
    const std::string f("pt_bloom: ");
    if (!c) return fail(nullptr, f + "null context");
    if (!src_rgba || !bp || !out_rgba) return fail(c, f + "null argument");
    if (width == 0 || height == 0) return fail(c, f + "width and height must be >= 1");
    const uint64_t n = (uint64_t)width * height;
    if (n > (1ull << 31)) return fail(c, f + "image too large (2^31 pixels)");
    if (!std::isfinite(bp->threshold) || bp->threshold < 0.0f) return fail(c, f + "threshold must be finite and >= 0");
    if (!std::isfinite(bp->knee) || bp->knee < 0.0f || bp->knee > bp->threshold) return fail(c, f + "knee must be finite and in [0, threshold]");
    if (!std::isfinite(bp->clamp) || bp->clamp < 0.0f) return fail(c, f + "clamp must be finite and >= 0 (0: no limit)");
    if (!std::isfinite(bp->intensity) || bp->intensity < 0.0f) return fail(c, f + "intensity must be finite and >= 0");
    if (!std::isfinite(bp->spread) || bp->spread < 0.0f || bp->spread > 4.0f) return fail(c, f + "spread must be finite and in [0, 4]");
    if (bp->levels < 1u || bp->levels > ptd::kBloomMaxLevels) return fail(c, f + "levels must be in [1, 8]");
    if (spans_overlap(src_rgba, (size_t)n * sizeof(float4), out_rgba, (size_t)n * sizeof(float4))) return fail(c, f + "out_rgba overlaps src_rgba");
    CK(c, hipSetDevice(c->device));
    const ptd::BloomLevels lv = ptd::bloom_levels(width, height, bp->levels);
    CK(c, c->d_bloom_pyramid.reserve((size_t)lv.off[lv.n + 1u], c->stream));      // all levels in one allocation
    return run_metered(c, "pt_bloom", c->d_bloom, info, [&](ptd::BloomState* st) {
        return ptd::launch_bloom((const float4*)src_rgba, width, height, *bp, (float4*)out_rgba, c->d_bloom_pyramid.p, st, c->stream);
    });
}

// ---- temporal reprojection (pt_temporal_blend; kernels in temporal.hip) --------------------------------------------------------
// the per-triangle bsdfType array: on the first call after pt_set_scene, counted in device_bytes from then on, freed with the scene
static int ensure_tri_bsdf(pt_ctx* c)
{
    if (c->d_tri_bsdf.p || c->bvh.n_tris == 0) return 0;
    CK(c, c->d_tri_bsdf.reserve(c->bvh.n_tris, c->stream));
    hipError_t e = ptd::launch_tri_bsdf(device_scene(c), c->d_tri_bsdf.p, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->d_tri_bsdf.release(); return fail(c, std::string("pt_temporal_blend: per-triangle materials: ") + hipGetErrorString(e)); }
    return 0;
}

// pt_temporal_blend and pt_temporal_blend_motion: every refusal before any device work, in this order, named after the caller
static int temporal_blend(pt_ctx* c, const char* fn, const pt_params* p, uint32_t accum_samples, const float* albedo_prim,
                          const float* normal_depth, const pt_params* prev, const float* prev_history, const float* prev_albedo_prim,
                          const float* prev_normal_depth, float history_cap, bool motion, const float* verts_xyzw, const float* prev_verts_xyzw,
                          size_t n_verts, float clip_gamma, float* out_history)
{
    const std::string f(fn);
    if (!c) return fail(nullptr, f + ": null context");
    if (!p || !p->accumulationBuffer || !albedo_prim || !normal_depth || !out_history) return fail(c, f + ": null argument");
    const int n_prev = (prev != nullptr) + (prev_history != nullptr) + (prev_albedo_prim != nullptr) + (prev_normal_depth != nullptr);
    if (n_prev != 0 && n_prev != 4) return fail(c, f + ": prev, prev_history, prev_albedo_prim and prev_normal_depth are all given or all NULL");
    if (accum_samples == 0u) return fail(c, f + ": accum_samples must be >= 1");
    if (!(history_cap >= 0.0f) || !std::isfinite(history_cap)) return fail(c, f + ": history_cap must be finite and >= 0");
    if (int rc = check_image(c, p, fn)) return rc;
    if (prev) if (int rc = check_image(c, prev, (f + " (previous view)").c_str())) return rc;
    const size_t bytes = (size_t)p->width * p->height * sizeof(float4);
    const size_t prev_bytes = prev ? (size_t)prev->width * prev->height * sizeof(float4) : 0;
    const void* inputs[6] = {p->accumulationBuffer, albedo_prim, normal_depth, prev_history, prev_albedo_prim, prev_normal_depth};
    for (int i = 0; i < 6; i++)
        if (inputs[i] && spans_overlap(out_history, bytes, inputs[i], i < 3 ? bytes : prev_bytes))
            return fail(c, f + ": out_history overlaps an input (chained calls ping-pong two history buffers)");
    if (c->scene_serial == 0) return fail(c, f + ": no scene (pt_set_scene first)");
    if (motion) {
        if ((verts_xyzw != nullptr) != (prev_verts_xyzw != nullptr)) return fail(c, f + ": verts_xyzw and prev_verts_xyzw are both given or both NULL");
        if (!(clip_gamma >= 0.0f) || !std::isfinite(clip_gamma)) return fail(c, f + ": clip_gamma must be finite and >= 0");
        if (n_verts != c->kept_n_verts)
            return fail(c, f + ": " + std::to_string(n_verts) + " vertices, the scene has " + std::to_string(c->kept_n_verts));
        const size_t vbytes = n_verts * sizeof(float4);
        if (verts_xyzw && (spans_overlap(out_history, bytes, verts_xyzw, vbytes) || spans_overlap(out_history, bytes, prev_verts_xyzw, vbytes)))
            return fail(c, f + ": out_history overlaps an input (a vertex array)");
    }
    CK(c, hipSetDevice(c->device));
    if (int rc = ensure_tri_bsdf(c)) return rc;
    ptd::TpMotion mo = {};
    if (motion && verts_xyzw && c->bvh.n_tris > 0) {
        if (int rc = ensure_dev_idx(c)) return rc;
        mo.idx = c->d_idx.p; mo.verts = (const float4*)verts_xyzw; mo.prev_verts = (const float4*)prev_verts_xyzw;
    }
    mo.gamma = motion ? clip_gamma : 0.0f;
    ptd::TpPrev tp = {};
    if (prev) {
        tp.eye = prev->cameraEye; tp.U = prev->cameraU; tp.V = prev->cameraV; tp.W = prev->cameraW;
        tp.w = prev->width; tp.h = prev->height;
        tp.hist = (const float4*)prev_history; tp.albedo_prim = (const float4*)prev_albedo_prim; tp.normal_depth = (const float4*)prev_normal_depth;
    }
    Range range(fn);
    CK(c, ptd::launch_temporal((const float4*)p->accumulationBuffer, (const float4*)albedo_prim, (const float4*)normal_depth, p->width, p->height,
                               p->cameraEye, p->cameraU, p->cameraV, p->cameraW, (float)accum_samples, tp, c->d_tri_bsdf.p, c->bvh.n_tris,
                               history_cap, motion ? &mo : nullptr, (float4*)out_history, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_temporal_blend(pt_ctx* c, const pt_params* p, uint32_t accum_samples, const float* albedo_prim, const float* normal_depth,
                             const pt_params* prev, const float* prev_history, const float* prev_albedo_prim, const float* prev_normal_depth,
                             float history_cap, float* out_history)
{
    return temporal_blend(c, "pt_temporal_blend", p, accum_samples, albedo_prim, normal_depth, prev, prev_history, prev_albedo_prim,
                          prev_normal_depth, history_cap, false, nullptr, nullptr, 0, 0.0f, out_history);
}

PT_API int pt_temporal_blend_motion(pt_ctx* c, const pt_params* p, uint32_t accum_samples, const float* albedo_prim, const float* normal_depth,
                                    const pt_params* prev, const float* prev_history, const float* prev_albedo_prim,
                                    const float* prev_normal_depth, const float* verts_xyzw, const float* prev_verts_xyzw, size_t n_verts,
                                    float history_cap, float clip_gamma, float* out_history)
{
    return temporal_blend(c, "pt_temporal_blend_motion", p, accum_samples, albedo_prim, normal_depth, prev, prev_history, prev_albedo_prim,
                          prev_normal_depth, history_cap, true, verts_xyzw, prev_verts_xyzw, n_verts, clip_gamma, out_history);
}
