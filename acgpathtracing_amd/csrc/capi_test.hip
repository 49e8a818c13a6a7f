// capi_test.hip — the test hooks and diagnostics of include/acgpt_test.h (not part of the drop-in boundary).  Host code only.
#include <cstring>

#include "../../include/acgpt_test.h"
#include "context.h"
#include "selftest.h"
#include "small_ref.h"

PT_API int pt_bench_traversal(pt_ctx* c, const float* rays, size_t n, int repeats, int node_format, float* t_out, uint32_t* prim_out, float* ms_out,
                              uint64_t* counters_out)
{
    if (!c || !rays || !t_out || !prim_out || !ms_out || n == 0 || n > 0x7FFFFFFFull || repeats < 1 || node_format < 0 || node_format > 4)
        return fail(c, "pt_bench_traversal: bad argument");
    CK(c, hipSetDevice(c->device));
    if (int rc = ensure_node_format(c, node_format == 1 ? 3 : node_format == 3 ? 9 : node_format == 4 ? 11 : 0)) return rc;       // stream formats 0 / 2: fp32 nodes, 3: fp16 {lo, hi}, 4: fp16 {centre, half extent}, 1: four-wide
    const uint32_t entries = node_format == 1 ? (c->bvh.wide_depth + 1u) : c->stack_entries;
    DevBuf<float> d_rays, d_t;
    DevBuf<uint32_t> d_p, d_head;
    int bpc = 0;
    hipError_t e = ptd::trace_stream_occupancy(node_format, entries, &bpc);
    if (e == hipSuccess && bpc < 1) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = d_rays.reserve(n * 8, c->stream);
    if (e == hipSuccess) e = d_t.reserve(n, c->stream);
    if (e == hipSuccess) e = d_p.reserve(n, c->stream);
    if (e == hipSuccess) e = d_head.reserve(1, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays.p, rays, n * 32, hipMemcpyHostToDevice, c->stream);
    float best = 1e30f;
    const ptd::DeviceScene sc = device_scene(c);
    for (int r = 0; r < repeats && e == hipSuccess; r++) {
        e = hipMemsetAsync(d_head.p, 0, 4, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->d_counters.p, 0, 8 * sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev0, c->stream);
        if (e == hipSuccess) e = ptd::launch_trace_stream(node_format, sc, entries, d_rays.p, (uint32_t)n, d_head.p, d_t.p, d_p.p, c->d_counters.p, (uint32_t)(c->n_cus * bpc), c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
        if (ms < best) best = ms;
    }
    if (e == hipSuccess) e = hipMemcpy(t_out, d_t.p, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(prim_out, d_p.p, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && counters_out) e = hipMemcpy(counters_out, c->d_counters.p, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, std::string("pt_bench_traversal: ") + hipGetErrorString(e));
    *ms_out = best;
    return 0;
}

// in / out sizes per element, in dwords (op 1: in = {seed, count}, out = 2 * count)
PT_API int pt_selftest(pt_ctx* c, int op, const void* in, size_t n, void* out)
{
    //                            0  1  2   3   4   5   6   7   8  9 10 11 12 13 14 15 16 17 18  19  20 .. 29 unused           30 31 32 33 34 35 36 37 38  39  40  41  42  43
    static const int in_dw[44] = {2, 2, 3, 10, 10, 10, 10, 10, 10, 7, 4, 1, 6, 4, 2, 2, 6, 7, 3, 17, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 6, 4, 2, 2, 6, 7, 3, 20, 17, 19, 19, 19},
                     out_dw[44] = {1, 0, 1, 3, 3, 3, 3, 3, 3, 4, 2, 4, 3, 3, 3, 3, 3, 3, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 3, 3, 3, 3, 3, 3, 1, 3, 3, 3, 3, 3};
    if (!c || !in || !out || op < 0 || op > 43 || in_dw[op] == 0 || n == 0 || n > (1u << 24)) return fail(c, "pt_selftest: bad argument");
    CK(c, hipSetDevice(c->device));
    size_t in_bytes = n * (size_t)in_dw[op] * 4, out_bytes = n * (size_t)out_dw[op] * 4;
    uint32_t launch_n = (uint32_t)n;
    if (op == 1) {
        const uint32_t count = ((const uint32_t*)in)[1];
        if (n != 1 || count == 0 || count > (1u << 22)) return fail(c, "pt_selftest: op 1 takes one {seed, count} record");
        in_bytes = 8; out_bytes = (size_t)count * 8; launch_n = 1;
    }
    return device_round_trip(c, "pt_selftest", in, in_bytes, out, out_bytes, nullptr, 0, [&](void* d_in, void* d_out, void*) {
        return ptd::launch_selftest(op, (const uint32_t*)d_in, launch_n, (uint32_t*)d_out, c->stream);
    });
}

PT_API int pt_debug_environment(pt_ctx* c, int op, const float* in, size_t n, float* out)
{
    static const int in_dw[3] = {3, 3, 2}, out_dw[3] = {4, 1, 4};
    if (!c || op < 0 || op > 2 || (n != 0 && (!in || !out)) || n > (1u << 24)) return fail(c, "pt_debug_environment: bad argument");
    if (n == 0) return 0;
    CK(c, hipSetDevice(c->device));
    const size_t in_bytes = n * (size_t)in_dw[op] * 4, out_bytes = n * (size_t)out_dw[op] * 4;
    return device_round_trip(c, "pt_debug_environment", in, in_bytes, out, out_bytes, nullptr, 0, [&](void* d_in, void* d_out, void*) {
        return ptd::env_debug(ptd::env_view(c->env), op, c->math_mode != 0 ? 1 : 0, (const float*)d_in, (uint32_t)n, (float*)d_out, c->stream);
    });
}

// The map's tables as the device holds them (environment.hip builds them): device-to-host copies only, no kernel, nothing is built.
PT_API int pt_debug_environment_tables(pt_ctx* c, float* texels, float* marginal, float* conditional, float* info2, uint32_t* dims2)
{
    if (!c) { fail(nullptr, "pt_debug_environment_tables: null context"); return -1; }
    const ptd::EnvDevice& e = c->env;
    const bool set = e.w != 0u && e.texels != nullptr;
    if (dims2) { dims2[0] = set ? e.w : 0u; dims2[1] = set ? e.h : 0u; }
    if (!set) return 0;
    const size_t n = (size_t)e.w * e.h;
    hipError_t rc = hipSetDevice(c->device);
    if (rc == hipSuccess) rc = hipStreamSynchronize(c->stream);
    if (rc == hipSuccess && texels) rc = hipMemcpy(texels, e.texels, n * sizeof(float4), hipMemcpyDeviceToHost);
    if (rc == hipSuccess && marginal) rc = hipMemcpy(marginal, e.marginal, (size_t)e.h * sizeof(float), hipMemcpyDeviceToHost);
    if (rc == hipSuccess && conditional) rc = hipMemcpy(conditional, e.conditional, n * sizeof(float), hipMemcpyDeviceToHost);
    if (rc != hipSuccess) { fail(c, std::string("pt_debug_environment_tables: ") + hipGetErrorString(rc)); return -1; }
    if (info2) { info2[0] = e.total; info2[1] = e.pdf_scale; }
    return 1;
}

PT_API int pt_debug_microfacet(pt_ctx* c, int op, const float* in, size_t n, float* out)
{
    static const int out_dw[2] = {8, 4};
    if (!c || op < 0 || op > 1 || (n != 0 && (!in || !out)) || n > (1u << 24)) return fail(c, "pt_debug_microfacet: bad argument");
    if (n == 0) return 0;
    CK(c, hipSetDevice(c->device));
    const size_t in_bytes = n * 9u * 4u, out_bytes = n * (size_t)out_dw[op] * 4u;
    return device_round_trip(c, "pt_debug_microfacet", in, in_bytes, out, out_bytes, nullptr, 0, [&](void* d_in, void* d_out, void*) {
        return ptd::microfacet_debug(op, c->math_mode != 0 ? 1 : 0, (const float*)d_in, (uint32_t)n, (float*)d_out, c->stream);
    });
}

PT_API int pt_debug_wave_times(pt_ctx* c, uint64_t* out, size_t max_waves)
{
    if (!c || !out) return fail(c, "pt_debug_wave_times: null argument");
    if (max_waves > ptd::kMaxTimedWaves) max_waves = ptd::kMaxTimedWaves;
    CK(c, hipSetDevice(c->device));
    CK(c, hipMemcpy(out, c->d_counters.p + 8, 3 * max_waves * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

PT_API int pt_debug_queue_progress(pt_ctx* c, uint64_t* out)
{
    if (!c || !out) return fail(c, "pt_debug_queue_progress: null argument");
    CK(c, hipSetDevice(c->device));
    CK(c, hipMemcpy(out, c->d_counters.p + 8 + 3 * (size_t)ptd::kMaxTimedWaves, 2056 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

PT_API int pt_debug_queue_order(pt_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 3) return fail(c, "pt_debug_queue_order: 0 = contiguous eighths of the tile order per shard; round robin over the shards in units of 1 = a tile-strip row (default), 2 = a tile; 3 = one queue in image order");
    c->queue_order = mode;
    if (c->multi) for (size_t i = 1; i < c->multi->ranks.size(); i++) c->multi->ranks[i]->queue_order = mode;
    return 0;
}

// The host side of the pixel classes alone (no context, no GPU): out = 2 * params->height words, {outer lo | hi << 16, inner lo | hi << 16}
// per image row.  Returns 0 when the spans could be computed, 1 when they could not (box not entirely in front of the eye, ...).
PT_API int pt_debug_row_spans(const pt_params* p, const float* box_lo, const float* box_hi, uint32_t* out)
{
    if (!p || !box_lo || !box_hi || !out || p->width == 0 || p->height == 0 || p->width > 65535u || p->height > 32767u) return 2;
    std::vector<uint32_t> spans;
    const bool ok = row_spans(p, box_lo, box_hi, spans);
    memcpy(out, spans.data(), spans.size() * sizeof(uint32_t));
    return ok ? 0 : 1;
}

PT_API int pt_debug_pixel_classes(pt_ctx* c, int on)
{
    if (!c) return fail(c, "pt_debug_pixel_classes: null context");
    c->pixel_classes = on ? 1 : 0;
    if (c->multi) for (size_t i = 1; i < c->multi->ranks.size(); i++) c->multi->ranks[i]->pixel_classes = c->pixel_classes;
    return 0;
}

PT_API int pt_debug_window_moves(pt_ctx* c, uint64_t* out)
{
    if (!c || !out) return fail(c, "pt_debug_window_moves: null argument");
    CK(c, hipSetDevice(c->device));
    CK(c, hipMemcpy(out, c->d_counters.p + ptd::kWindowMoves, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

// ---- the small-scene path (render_small.hip) ----
PT_API int pt_debug_small_kernel(pt_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 3) return fail(c, "pt_debug_small_kernel: 0 = automatic, 1 = off, 2 = the 1024-thread grid alone, 3 = the 256-thread grid alone");
    c->small_mode = mode;
    return 0;
}

PT_API int pt_debug_small_kernel_path(pt_ctx* c) { return c ? c->small_last : -1; }

// no context, no GPU: the 16-bit references of small_ref.h for n 32-bit ones
PT_API int pt_debug_small_ref(const int32_t* refs, size_t n, uint16_t* encoded, int32_t* decoded, int32_t* local)
{
    if (!refs || !encoded || !decoded || !local) return 1;
    for (size_t i = 0; i < n; i++) {
        encoded[i] = ptd::small_ref_encode(refs[i]);
        decoded[i] = ptd::small_ref_decode(encoded[i]);
        local[i] = ptd::small_ref_local(refs[i]);
    }
    return 0;
}

// no context, no GPU: out = {LDS bytes of the 1024-thread workgroup, of the 256-thread workgroup, eligible (0 / 1), node limit, triangle limit}
PT_API int pt_debug_small_budget(uint32_t n_nodes, uint32_t n_tris, uint32_t stack_entries, uint64_t cu_lds_bytes, uint64_t* out)
{
    if (!out) return 1;
    out[0] = ptd::small_lds_bytes(ptd::kSmallBigThreads, stack_entries, n_nodes);
    out[1] = ptd::small_lds_bytes(ptd::kSmallLittleThreads, stack_entries, n_nodes);
    out[2] = ptd::small_eligible(n_nodes, n_tris, stack_entries, (size_t)cu_lds_bytes) ? 1u : 0u;
    out[3] = ptd::kSmallMaxNodes;
    out[4] = ptd::kSmallMaxTris;
    return 0;
}

// force: 0 the fp32 shape where its budget fits (default), 1 the fp16 two-copy shape always, -1 leave as it is.  Returns the shape of the last launch.
PT_API int pt_debug_small_shape(pt_ctx* c, int force)
{
    if (!c) return -1;
    if (force < -1 || force > 1) { fail(c, "pt_debug_small_shape: force = -1 (ask only), 0 (automatic) or 1 (the fp16 shape)"); return -1; }
    if (force >= 0) c->small_force_half = force;
    return c->small_shape_last;
}

// no context, no GPU: out = {LDS bytes of the 1024-thread workgroup with fp32 nodes, of the 256-thread workgroup without nodes, what the
// 256-thread launch asks for, fits (0 / 1)}
PT_API int pt_debug_small_float_budget(uint32_t n_nodes, uint32_t stack_entries, uint64_t cu_lds_bytes, uint64_t* out)
{
    if (!out) return 1;
    const ptd::SmallFloatBudget b = ptd::small_float_budget(stack_entries, n_nodes, (size_t)cu_lds_bytes);
    out[0] = b.big; out[1] = b.little; out[2] = b.little_request; out[3] = b.fits ? 1u : 0u;
    return 0;
}

// the kernel's own staging function over the scene's fp16 nodes, into a HOST buffer of 64 bytes a node
PT_API int pt_debug_small_staged(pt_ctx* c, void* out, size_t capacity_bytes)
{
    if (!c || !out) return fail(c, "pt_debug_small_staged: null argument");
    const ptd::LbvhResult& b = c->bvh;
    if (!c->scene_kept || b.n_tris == 0 || !b.hcnodes) return fail(c, "pt_debug_small_staged: no fp16 nodes held (pt_set_scene with triangles first)");
    if (b.n_nodes > ptd::kSmallMaxNodes) return fail(c, "pt_debug_small_staged: more nodes than the 16-bit references reach");
    const size_t bytes = (size_t)b.n_nodes * ptd::kSmallFloatNodeBytes;
    if (capacity_bytes < bytes) return fail(c, "pt_debug_small_staged: capacity " + std::to_string(capacity_bytes) + " bytes, the staged nodes take " + std::to_string(bytes));
    CK(c, hipSetDevice(c->device));
    const uint32_t no_input = 0u;      // the nodes are on the device already
    return device_round_trip(c, "pt_debug_small_staged", &no_input, sizeof(no_input), out, bytes, nullptr, 0, [&](void*, void* d_out, void*) {
        return ptd::launch_small_stage_f32(b.hcnodes, b.n_nodes, d_out, c->stream);
    });
}

#ifdef ACGPT_EXPERIMENTS
// experiments build only: renumber the resident fp16 nodes (0: the build's order, 1: sibling pairs share a 64-byte line, 2: depth first)
namespace ptd { bool reorder_records_dfs(LbvhResult& r, hipStream_t stream, std::string& err); }      // lbvh_experiments.inc
PT_API int pt_debug_node_order(pt_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 3) return fail(c, "pt_debug_node_order: mode 0, 1, 2 or 3");
    CK(c, hipSetDevice(c->device));
    CK(c, hipStreamSynchronize(c->stream));
    std::string err;
    if (mode == 3) {        // the triangle records in depth-first leaf order (in place; the nodes stay as they are)
        if (!ptd::reorder_records_dfs(c->bvh, c->stream, err)) return fail(c, "pt_debug_node_order: " + err);
        return 0;
    }
    if (!ptd::reorder_hcnodes(c->bvh, mode, c->stream, err)) return fail(c, "pt_debug_node_order: " + err);
    return 0;
}

// experiments build only: per-role times of the last launch of a wavefront kernel (render_wavefront.hip), 17 values (tools/wf_check.py)
PT_API int pt_debug_wf(pt_ctx* c, uint64_t* out)
{
    if (!c || !out) return fail(c, "pt_debug_wf: null argument");
    CK(c, hipSetDevice(c->device));
    CK(c, hipMemcpy(out, c->d_counters.p + ptd::kWfDiag, 17 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}
#endif

PT_API int pt_read_morton(pt_ctx* c, uint32_t* codes_sorted, uint32_t* prims_sorted)
{
    if (!c || !codes_sorted || !prims_sorted) return fail(c, "pt_read_morton: null argument");
    if (c->bvh.n_tris == 0) return 0;
    CK(c, hipSetDevice(c->device));
    std::string err;
    if (!ptd::read_morton(c->bvh, c->stream, codes_sorted, prims_sorted, err)) return fail(c, "pt_read_morton: " + err);
    return 0;
}

// The scene's tree as the device holds it (tests/tree_ref.py): device-to-host copies only, nothing is built or released.
PT_API int pt_debug_read_tree(pt_ctx* c, int what, void* out, size_t capacity_bytes, pt_tree_info* info)
{
    if (!c) return fail(nullptr, "pt_debug_read_tree: null context");
    if (what < 0 || what > 6) return fail(c, "pt_debug_read_tree: what = 0 (info only) .. 6");
    if (what == 0 ? !info : !out) return fail(c, "pt_debug_read_tree: null argument");
    if (!c->scene_kept || c->bvh.n_tris == 0) return fail(c, "pt_debug_read_tree: no scene (pt_set_scene with triangles first)");
    const ptd::LbvhResult& b = c->bvh;
    const void* src[7] = {nullptr, b.nodes, b.hnodes, b.hcnodes, b.wrecs, b.tris, b.shade};
    const size_t bytes[7] = {0, (size_t)b.n_nodes * sizeof(ptd::BvhNode), (size_t)b.n_nodes * sizeof(ptd::HNode), (size_t)b.n_nodes * sizeof(ptd::HNode),
                             (size_t)b.n_wrecs * 48u, (size_t)b.n_tris * sizeof(ptd::TriRecord), (size_t)b.n_tris * sizeof(float4)};
    if (what != 0) {
        if (!src[what]) return fail(c, "pt_debug_read_tree: array " + std::to_string(what) + " is not held");
        if (capacity_bytes < bytes[what])
            return fail(c, "pt_debug_read_tree: capacity " + std::to_string(capacity_bytes) + " bytes, the array has " + std::to_string(bytes[what]));
        CK(c, hipSetDevice(c->device));
        CK(c, hipStreamSynchronize(c->stream));
        CK(c, hipMemcpy(out, src[what], bytes[what], hipMemcpyDeviceToHost));
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->n_tris = b.n_tris; info->n_nodes = b.n_nodes; info->max_depth = b.max_depth; info->mode = b.mode; info->pad_abs = b.pad_abs;
        memcpy(info->hspace, &b.hspace, sizeof(info->hspace));
        for (int k = 0; k < 3; k++) { info->scene_lo[k] = b.scene_lo[k]; info->scene_hi[k] = b.scene_hi[k]; }
        info->n_wrecs = b.n_wrecs; info->n_wnodes = b.n_wnodes; info->wide_depth = b.wide_depth;
        for (int w = 1; w <= 6; w++) if (src[w]) info->held |= 1u << (w - 1);
    }
    return 0;
}

// pt_query_winding's moments as the device holds them (tests/winding_ref.py): a device-to-host copy only, nothing is built or released.
PT_API int pt_debug_read_winding(pt_ctx* c, void* out, size_t capacity_bytes)
{
    if (!c) return fail(nullptr, "pt_debug_read_winding: null context");
    if (!out) return fail(c, "pt_debug_read_winding: null argument");
    if (!c->winding.built) return fail(c, "pt_debug_read_winding: the moments are not built (pt_query_winding builds them)");
    const size_t bytes = (size_t)c->winding.n_nodes * sizeof(ptd::WindMoment);
    if (capacity_bytes < bytes) return fail(c, "pt_debug_read_winding: capacity " + std::to_string(capacity_bytes) + " bytes, the moments take " + std::to_string(bytes));
    CK(c, hipSetDevice(c->device));
    CK(c, hipStreamSynchronize(c->stream));
    CK(c, hipMemcpy(out, c->winding.moments, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// What the last build recorded about itself (tests/build_ref.py holds it to the references): plain reads of the context, no device call.
PT_API int pt_debug_build_stats(pt_ctx* c, pt_build_stats* out)
{
    if (!c) return fail(nullptr, "pt_debug_build_stats: null context");
    if (!out) return fail(c, "pt_debug_build_stats: null argument");
    if (!c->scene_kept || c->bvh.n_tris == 0) return fail(c, "pt_debug_build_stats: no scene (pt_set_scene with triangles first)");
    const ptd::LbvhResult& b = c->bvh;
    memset(out, 0, sizeof(*out));
    out->opt_area_before = b.opt_area_before; out->opt_area_after = b.opt_area_after; out->opt_ms = b.opt_ms;
    out->opt_passes = b.opt_passes; out->build_iterations = b.build_iterations; out->mode = b.mode;
    return 0;
}
