// capi_query.hip — the entry points of include/acgpt.h that answer queries in device memory: pt_query_closest, pt_query_any, the
// ordered multi-hit query pt_query_multi, the ambient-occlusion stage on top of them: pt_ao_points, pt_ao_image, and the
// closest-point query pt_query_nearest, the box-overlap queries pt_query_overlap, pt_query_overlap_any and the swept-sphere casts
// pt_query_sweep, pt_query_sweep_any, the swept-capsule casts pt_query_capsule_cast, pt_query_capsule_cast_any, the triangle-against-mesh queries pt_query_triangles, pt_query_triangles_any, the
// segment-to-mesh distance query pt_query_segments and the K-closest and within-radius queries pt_query_nearest_k,
// pt_query_within_any and the generalised winding number pt_query_winding (each with its counting twin of include/acgpt_test.h),
// the complete lists in CSR form: pt_list_offsets, pt_query_overlap_lists, pt_query_triangles_lists, and the posed-mesh queries
// pt_set_query_mesh, pt_get_query_mesh, pt_pose_triangles, pt_query_poses_any, pt_query_poses_distance, and the translating-triangle
// casts pt_query_triangle_cast, pt_query_triangle_cast_any, pt_query_poses_cast, and the oriented-box overlap queries
// pt_query_overlap_oriented, pt_query_overlap_oriented_any, pt_query_overlap_oriented_lists with pt_pose_boxes, and the swept
// oriented-box casts pt_query_box_cast, pt_query_box_cast_any.
// Host code only; the kernels are in query.hip, multihit.hip, ao.hip, nearest.hip, nearest_k.hip, overlap.hip, sweep.hip, capsule.hip, tritri.hip, segment.hip, tridist.hip, winding.hip, lists.hip, poses.hip, tricast.hip, oriented.hip and boxcast.hip; their one walk, leaf routine and launch are in bvh_walk.h, closest_point.h and query_launch.h.  The context and what the units share: context.h.
#include <cmath>

#include "../../include/acgpt_test.h"
#include "context.h"
#include "ao.h"
#include "boxcast.h"
#include "capsule.h"
#include "lists.h"
#include "multihit.h"
#include "nearest.h"
#include "nearest_k.h"
#include "oriented.h"
#include "overlap.h"
#include "poses.h"
#include "query.h"
#include "segment.h"
#include "tridist.h"
#include "sweep.h"
#include "tricast.h"
#include "tritri.h"

static_assert(sizeof(pt_hit) == 32, "pt_hit: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_nearest) == 32, "pt_nearest: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_sweep_hit) == 32, "pt_sweep_hit: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_capsule_cast_hit) == 32, "pt_capsule_cast_hit: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_box_cast_hit) == 48, "pt_box_cast_hit: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_segment_hit) == 32, "pt_segment_hit: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_triangle_distance_hit) == 48, "pt_triangle_distance_hit: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_pose_distance_hit) == 48, "pt_pose_distance_hit: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_triangle_cast_hit) == 32, "pt_triangle_cast_hit: a change of this layout bumps pt_abi_version");
static_assert(sizeof(pt_ao_params) == 32, "pt_ao_params: a change of this layout bumps pt_abi_version");

// The node array the scene holds, as pt_render_features picks it: fp16 centre / half-extent nodes for the default variants, fp32
// nodes for the fp32 ones; only a variant forced onto another format (pt_set_tuning) leaves neither and gets the fp32 nodes back.
// The last refusals of a call: no scene, no device.  f: the entry point's name and ": ".
static int query_node_format(pt_ctx* c, const std::string& f, int* fmt)
{
    if (c->scene_serial == 0) return fail(c, f + "no scene (pt_set_scene first)");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, f + "hipSetDevice failed");
    *fmt = 0;
    if (c->bvh.hcnodes) *fmt = 11;
    else if (int rc = ensure_node_format(c, 0)) return rc;
    return 0;
}

// every refusal of the two calls before any device work, in this order; out_bytes: bytes of output per ray.  *fmt: the node format
// the scene holds (pt_render_features' choice).  Returns 0 to go on, 1 refused, -1 nothing to do (n == 0).
static int query_prepare(pt_ctx* c, const char* fn, const float* rays, size_t n, const void* out, size_t out_bytes, bool out_aligned, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!rays || !out) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many rays (2^31 - 1 per call)");
    if (((uintptr_t)rays & 15u) || (out_aligned && ((uintptr_t)out & 15u))) return fail(c, f + "the ray and hit arrays must be 16-byte aligned");
    if (spans_overlap(rays, n * 32u, out, n * out_bytes)) return fail(c, f + "the output overlaps the rays");
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_closest(pt_ctx* c, const float* rays, size_t n, pt_hit* hits)
{
    int fmt = 0;
    if (int rc = query_prepare(c, "pt_query_closest", rays, n, hits, sizeof(pt_hit), true, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_closest");
    CK(c, ptd::launch_query_closest(fmt, device_scene(c), c->stack_entries, (const float4*)rays, (uint32_t)n, (float4*)hits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_any(pt_ctx* c, const float* rays, size_t n, uint8_t* occluded)
{
    int fmt = 0;
    if (int rc = query_prepare(c, "pt_query_any", rays, n, occluded, 1, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_any");
    CK(c, ptd::launch_query_any(fmt, device_scene(c), c->stack_entries, (const float4*)rays, (uint32_t)n, occluded, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the first hits in order, and their number -----------------------------------------------------------------------------------
static_assert(PT_QUERY_MULTI_MAX == ptd::kMultiMaxHits, "PT_QUERY_MULTI_MAX is the size of the kernel's largest list");

PT_API int pt_query_multi(pt_ctx* c, const float* rays, size_t n, uint32_t max_hits, pt_hit* hits, uint32_t* counts)
{
    const std::string f = "pt_query_multi: ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return 0;
    if (max_hits > PT_QUERY_MULTI_MAX) return fail(c, f + "max_hits must be at most " + std::to_string(PT_QUERY_MULTI_MAX));
    if ((max_hits != 0u) != (hits != nullptr)) return fail(c, f + "hits goes with max_hits: both or neither");
    if (!hits && !counts) return fail(c, f + "nothing to write (hits and counts are both null)");
    if (!rays) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many rays (2^31 - 1 per call)");
    if (((uintptr_t)rays & 15u) || ((uintptr_t)hits & 15u) || ((uintptr_t)counts & 3u))
        return fail(c, f + "the ray and hit arrays must be 16-byte aligned, the counts 4-byte aligned");
    const size_t hit_bytes = n * (size_t)max_hits * sizeof(pt_hit);      // n < 2^31, max_hits <= 8: below 2^39
    if (hits && spans_overlap(rays, n * 32u, hits, hit_bytes)) return fail(c, f + "hits overlaps the rays");
    if (counts && spans_overlap(rays, n * 32u, counts, n * 4u)) return fail(c, f + "counts overlaps the rays");
    if (hits && counts && spans_overlap(hits, hit_bytes, counts, n * 4u)) return fail(c, f + "counts overlaps hits");
    int fmt = 0;
    if (int rc = query_node_format(c, f, &fmt)) return rc;
    Range range("pt_query_multi");
    CK(c, ptd::launch_query_multi(fmt, device_scene(c), c->stack_entries, (const float4*)rays, (uint32_t)n, max_hits, (float4*)hits, counts, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- closest point ---------------------------------------------------------------------------------------------------------------
// every refusal of pt_query_nearest before any device work, in pt_query_closest's order.  Returns 0 to go on, 1 refused, -1 nothing to do.
static int nearest_prepare(pt_ctx* c, const char* fn, const float* points, size_t n, const void* out, const void* visits, bool with_visits, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!points || !out || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many points (2^31 - 1 per call)");
    if (((uintptr_t)points & 15u) || ((uintptr_t)out & 15u) || ((uintptr_t)visits & 7u)) return fail(c, f + "the point and record arrays must be 16-byte aligned");
    if (spans_overlap(points, n * 16u, out, n * sizeof(pt_nearest))) return fail(c, f + "the output overlaps the points");
    if (with_visits && (spans_overlap(points, n * 16u, visits, n * 8u) || spans_overlap(out, n * sizeof(pt_nearest), visits, n * 8u)))
        return fail(c, f + "the visit counts overlap another array");
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_nearest(pt_ctx* c, const float* points, size_t n, pt_nearest* out)
{
    int fmt = 0;
    if (int rc = nearest_prepare(c, "pt_query_nearest", points, n, out, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_nearest");
    CK(c, ptd::launch_query_nearest(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)points,
                                    (uint32_t)n, (float4*)out, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_nearest_visits(pt_ctx* c, const float* points, size_t n, pt_nearest* out, uint32_t* visits)
{
    int fmt = 0;
    if (int rc = nearest_prepare(c, "pt_debug_nearest_visits", points, n, out, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_nearest_visits(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)points,
                                     (uint32_t)n, (float4*)out, (uint2*)visits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the K closest triangles, anything within a radius ----------------------------------------------------------------------------
static_assert(PT_QUERY_NEAREST_MAX == ptd::kNearestMaxK, "PT_QUERY_NEAREST_MAX is the size of the kernel's largest list");

// every refusal of the two calls and their twin before any device work, in pt_query_nearest's order with pt_query_multi's additions.
// list: the call has max_k, out and counts; otherwise it has hit.  visits: null unless with_visits.  Returns 0 to go on, 1 refused,
// -1 nothing to do (n == 0).
static int nearest_k_prepare(pt_ctx* c, const char* fn, const float* points, size_t n, bool list, uint32_t max_k, const void* out, const void* counts,
                             const void* hit, const void* visits, bool with_visits, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (list) {
        if (max_k > PT_QUERY_NEAREST_MAX) return fail(c, f + "max_k must be at most " + std::to_string(PT_QUERY_NEAREST_MAX));
        if ((max_k != 0u) != (out != nullptr)) return fail(c, f + "out goes with max_k: both or neither");
        if (!out && !counts) return fail(c, f + "nothing to write (out and counts are both null)");
    }
    if (!points || (!list && !hit) || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many points (2^31 - 1 per call)");
    if (((uintptr_t)points & 15u) || ((uintptr_t)out & 15u) || ((uintptr_t)counts & 3u) || ((uintptr_t)visits & 7u))
        return fail(c, f + "the point and record arrays must be 16-byte aligned, the counts 4-byte aligned");
    // n < 2^31, max_k <= 8: the byte counts stay below 2^39
    const struct { const void* p; size_t bytes; const char* name; } spans[5] = {
        {points, n * 16u, "the points"}, {out, n * (size_t)max_k * sizeof(pt_nearest), "out"}, {counts, n * 4u, "counts"}, {hit, n, "hit"}, {visits, n * 8u, "the visit counts"}};
    for (int k = 1; k < 5; k++) {
        if (!spans[k].p) continue;
        for (int j = 0; j < k; j++)
            if (spans[j].p && spans_overlap(spans[j].p, spans[j].bytes, spans[k].p, spans[k].bytes))
                return fail(c, f + spans[k].name + " overlaps " + spans[j].name);
    }
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_nearest_k(pt_ctx* c, const float* points, size_t n, uint32_t max_k, pt_nearest* out, uint32_t* counts)
{
    int fmt = 0;
    if (int rc = nearest_k_prepare(c, "pt_query_nearest_k", points, n, true, max_k, out, counts, nullptr, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_nearest_k");
    CK(c, ptd::launch_query_nearest_k(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)points,
                                      (uint32_t)n, max_k, (float4*)out, counts, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_within_any(pt_ctx* c, const float* points, size_t n, uint8_t* hit)
{
    int fmt = 0;
    if (int rc = nearest_k_prepare(c, "pt_query_within_any", points, n, false, 0u, nullptr, nullptr, hit, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_within_any");
    CK(c, ptd::launch_query_within_any(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)points,
                                       (uint32_t)n, hit, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_nearest_k_visits(pt_ctx* c, const float* points, size_t n, uint32_t max_k, pt_nearest* out, uint32_t* counts, uint8_t* hit, uint32_t* visits)
{
    if (c && hit && (max_k != 0u || out || counts)) return fail(c, "pt_debug_nearest_k_visits: hit goes with max_k 0 and no out or counts");
    int fmt = 0;
    if (int rc = nearest_k_prepare(c, "pt_debug_nearest_k_visits", points, n, hit == nullptr, max_k, out, counts, hit, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_nearest_k_visits(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)points,
                                       (uint32_t)n, max_k, (float4*)out, counts, hit, (uint2*)visits, hit ? 1u : 0u, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- generalised winding numbers ---------------------------------------------------------------------------------------------------
static_assert(sizeof(pt_winding_info) == 16, "pt_winding_info: a change of this layout bumps pt_abi_version");

// every refusal of pt_query_winding and its twin before any device work, in pt_query_nearest's order with a bad beta after n == 0 and
// the overlaps last; then the moments, built on the first call after the scene or its vertices changed.  Returns 0 to go on, 1
// refused or failed, -1 nothing to do.
static int winding_prepare(pt_ctx* c, const char* fn, const float* points, size_t n, float beta, const void* out, const void* visits, bool with_visits)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!(beta >= 1.0f)) return fail(c, f + "beta must be at least 1 (+inf: the exact sum)");
    if (!points || !out || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many points (2^31 - 1 per call)");
    if (((uintptr_t)points & 15u) || ((uintptr_t)out & 3u) || ((uintptr_t)visits & 7u))
        return fail(c, f + "the points must be 16-byte aligned, the output 4-byte aligned");
    if (spans_overlap(points, n * 16u, out, n * 4u)) return fail(c, f + "the output overlaps the points");
    if (with_visits && (spans_overlap(points, n * 16u, visits, n * 8u) || spans_overlap(out, n * 4u, visits, n * 8u)))
        return fail(c, f + "the visit counts overlap another array");
    int fmt = 0;
    if (int rc = query_node_format(c, f, &fmt)) return rc;
    if (c->bvh.n_tris != 0u && !c->winding.built) {
        Range range("acgpt: winding moments");
        std::string err;
        if (!ptd::build_winding(c->bvh, c->stream, c->winding, err)) return fail(c, f + err);
    }
    return 0;
}

PT_API int pt_query_winding(pt_ctx* c, const float* points, size_t n, float beta, float* out)
{
    if (int rc = winding_prepare(c, "pt_query_winding", points, n, beta, out, nullptr, false)) return rc < 0 ? 0 : rc;
    Range range("pt_query_winding");
    CK(c, ptd::launch_query_winding(c->winding, c->bvh.tris, c->bvh.n_tris, c->stack_entries, beta * beta, (const float4*)points, (uint32_t)n, out, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_winding_visits(pt_ctx* c, const float* points, size_t n, float beta, float* out, uint32_t* visits)
{
    if (int rc = winding_prepare(c, "pt_debug_winding_visits", points, n, beta, out, visits, true)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_winding_visits(c->winding, c->bvh.tris, c->bvh.n_tris, c->stack_entries, beta * beta, (const float4*)points, (uint32_t)n, out,
                                     (uint2*)visits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- box overlap -----------------------------------------------------------------------------------------------------------------
static_assert(PT_QUERY_OVERLAP_MAX == ptd::kOverlapMaxPrims, "PT_QUERY_OVERLAP_MAX is the size of the kernel's largest list");

// One output array of an overlap call: bytes per box, the alignment it needs (a mask), whether the call cannot do without it.
struct OverlapOut { const void* p; size_t bytes_per_box; uintptr_t align_mask; bool required; const char* name; };

// every refusal of the three calls before any device work, in pt_query_multi's order.  list: the call has max_prims and prims
// (outs[0] is prims).  The triangle queries share it: what names the input records ("boxes") and in_bytes, the bytes of one.
// Returns 0 to go on, 1 refused, -1 nothing to do (n == 0).
static int overlap_prepare(pt_ctx* c, const char* fn, const float* boxes, size_t n, bool list, uint32_t max_prims, const OverlapOut* outs, int n_outs, int* fmt,
                           const char* what = "boxes", size_t in_bytes = 32u)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (list) {
        if (max_prims > PT_QUERY_OVERLAP_MAX) return fail(c, f + "max_prims must be at most " + std::to_string(PT_QUERY_OVERLAP_MAX));
        if ((max_prims != 0u) != (outs[0].p != nullptr)) return fail(c, f + "prims goes with max_prims: both or neither");
        if (!outs[0].p && !outs[1].p) return fail(c, f + "nothing to write (prims and counts are both null)");
    }
    if (!boxes) return fail(c, f + "null argument");
    for (int k = 0; k < n_outs; k++)
        if (outs[k].required && !outs[k].p) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many " + what + " (2^31 - 1 per call)");
    if ((uintptr_t)boxes & 15u) return fail(c, f + "the " + what + " must be 16-byte aligned");
    for (int k = 0; k < n_outs; k++)
        if ((uintptr_t)outs[k].p & outs[k].align_mask) return fail(c, f + outs[k].name + " must be " + std::to_string(outs[k].align_mask + 1u) + "-byte aligned");
    for (int k = 0; k < n_outs; k++) {
        if (!outs[k].p) continue;
        if (spans_overlap(boxes, n * in_bytes, outs[k].p, n * outs[k].bytes_per_box)) return fail(c, f + outs[k].name + " overlaps the " + what);
        for (int j = 0; j < k; j++)
            if (outs[j].p && spans_overlap(outs[j].p, n * outs[j].bytes_per_box, outs[k].p, n * outs[k].bytes_per_box))
                return fail(c, f + outs[k].name + " overlaps " + outs[j].name);
    }
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_overlap(pt_ctx* c, const float* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts)
{
    // n < 2^31, max_prims <= 8: the byte counts stay below 2^36
    const OverlapOut outs[2] = {{prims, (size_t)max_prims * 4u, 15u, false, "prims"}, {counts, 4u, 3u, false, "counts"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_overlap", boxes, n, true, max_prims, outs, 2, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_overlap");
    CK(c, ptd::launch_query_overlap(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)boxes,
                                    (uint32_t)n, max_prims, prims, counts, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_overlap_any(pt_ctx* c, const float* boxes, size_t n, uint8_t* hit)
{
    const OverlapOut outs[1] = {{hit, 1u, 0u, true, "hit"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_overlap_any", boxes, n, false, 0u, outs, 1, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_overlap_any");
    CK(c, ptd::launch_query_overlap_any(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)boxes,
                                        (uint32_t)n, hit, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_overlap_visits(pt_ctx* c, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits)
{
    const OverlapOut outs[2] = {{counts, 4u, 3u, true, "counts"}, {visits, 8u, 7u, true, "visits"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_debug_overlap_visits", boxes, n, false, 0u, outs, 2, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_overlap_visits(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)boxes,
                                     (uint32_t)n, counts, (uint2*)visits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- triangle against mesh -------------------------------------------------------------------------------------------------------
static_assert(PT_QUERY_TRIANGLES_MAX == ptd::kTrianglesMaxPrims, "PT_QUERY_TRIANGLES_MAX is the size of the kernel's largest list");
static_assert(PT_QUERY_TRIANGLES_MAX == PT_QUERY_OVERLAP_MAX, "overlap_prepare names one limit for both");

// The three calls refuse what pt_query_overlap's refuse, in the same order (overlap_prepare); a query is 48 bytes.
PT_API int pt_query_triangles(pt_ctx* c, const float* tris, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts)
{
    // n < 2^31, max_prims <= 8: the byte counts stay below 2^37
    const OverlapOut outs[2] = {{prims, (size_t)max_prims * 4u, 15u, false, "prims"}, {counts, 4u, 3u, false, "counts"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_triangles", tris, n, true, max_prims, outs, 2, &fmt, "triangles", 48u)) return rc < 0 ? 0 : rc;
    Range range("pt_query_triangles");
    CK(c, ptd::launch_query_triangles(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)tris,
                                      (uint32_t)n, max_prims, prims, counts, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_triangles_any(pt_ctx* c, const float* tris, size_t n, uint8_t* hit)
{
    const OverlapOut outs[1] = {{hit, 1u, 0u, true, "hit"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_triangles_any", tris, n, false, 0u, outs, 1, &fmt, "triangles", 48u)) return rc < 0 ? 0 : rc;
    Range range("pt_query_triangles_any");
    CK(c, ptd::launch_query_triangles_any(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)tris,
                                          (uint32_t)n, hit, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_triangles_visits(pt_ctx* c, const float* tris, size_t n, uint32_t* counts, uint32_t* visits)
{
    const OverlapOut outs[2] = {{counts, 4u, 3u, true, "counts"}, {visits, 8u, 7u, true, "visits"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_debug_triangles_visits", tris, n, false, 0u, outs, 2, &fmt, "triangles", 48u)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_triangles_visits(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)tris,
                                       (uint32_t)n, counts, (uint2*)visits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- complete lists in CSR form ---------------------------------------------------------------------------------------------------
// counts -> offsets.  Needs no scene.  The refusals in the siblings' order; the total is judged after it has been computed.
PT_API int pt_list_offsets(pt_ctx* c, const uint32_t* counts, size_t n, uint32_t* offsets, uint64_t* total)
{
    const std::string f = "pt_list_offsets: ";
    if (!c) return fail(nullptr, f + "null context");
    if (total) *total = 0u;
    if (n == 0 && !offsets) return 0;
    if (!offsets || (n != 0 && !counts)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many counts (2^31 - 1 per call)");
    if (((uintptr_t)counts & 3u) || ((uintptr_t)offsets & 3u)) return fail(c, f + "counts and offsets must be 4-byte aligned");
    if (n != 0 && spans_overlap(counts, n * 4u, offsets, (n + 1u) * 4u)) return fail(c, f + "offsets overlaps counts (the scan is not in place)");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, f + "hipSetDevice failed");
    Range range("pt_list_offsets");
    if (n == 0) {
        CK(c, hipMemsetAsync(offsets, 0, 4u, c->stream));
        CK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    const size_t words = ptd::list_scratch_words(n);
    CK(c, c->d_list_scratch.reserve(words, c->stream));
    CK(c, ptd::launch_list_offsets(counts, (uint32_t)n, offsets, c->d_list_scratch.p, c->stream));
    unsigned long long sum = 0ull;
    CK(c, hipMemcpyAsync(&sum, c->d_list_scratch.p + (words - 1u), sizeof(sum), hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    if (total) *total = sum;
    if (sum > 0xFFFFFFFFull) return fail(c, f + "the total " + std::to_string(sum) + " does not fit 32-bit offsets: split the batch");
    return 0;
}

// every refusal of the two list calls before any device work, in pt_query_overlap's order.  what names the input records, in_bytes the
// bytes of one.  Returns 0 to go on, 1 refused, -1 nothing to do (n == 0).
static int lists_prepare(pt_ctx* c, const char* fn, const float* recs, size_t n, const uint32_t* offsets, const uint32_t* prims, size_t capacity,
                         const uint32_t* found, int* fmt, const char* what, size_t in_bytes)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!recs || !offsets || (!prims && capacity != 0)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many " + what + " (2^31 - 1 per call)");
    if ((uintptr_t)recs & 15u) return fail(c, f + "the " + what + " must be 16-byte aligned");
    if (((uintptr_t)offsets & 3u) || ((uintptr_t)prims & 3u) || ((uintptr_t)found & 3u)) return fail(c, f + "offsets, prims and found must be 4-byte aligned");
    if (capacity > ((size_t)-1 >> 2)) return fail(c, f + "capacity is more words than memory has");
    const struct { const void* p; size_t bytes; const char* name; } spans[4] = {
        {recs, n * in_bytes, what}, {offsets, (n + 1u) * 4u, "offsets"}, {capacity ? prims : nullptr, capacity * 4u, "prims"}, {found, n * 4u, "found"}};
    for (int k = 1; k < 4; k++) {
        if (!spans[k].p) continue;
        for (int j = 0; j < k; j++)
            if (spans[j].p && spans_overlap(spans[j].p, spans[j].bytes, spans[k].p, spans[k].bytes))
                return fail(c, f + spans[k].name + " overlaps " + (j == 0 ? "the " : "") + spans[j].name);
    }
    return query_node_format(c, f, fmt);
}

// the flag is cleared, the lists are written, the flag is read after the sync; a raised flag is the call's failure, the lists stay
template <typename Launch>
static int lists_run(pt_ctx* c, const char* fn, Launch launch)
{
    CK(c, c->d_list_scratch.reserve(ptd::list_scratch_words(0), c->stream));
    uint32_t* flag = (uint32_t*)c->d_list_scratch.p;
    CK(c, hipMemsetAsync(flag, 0, sizeof(uint32_t), c->stream));
    CK(c, launch(flag));
    uint32_t raised = 0u;
    CK(c, hipMemcpyAsync(&raised, flag, sizeof(raised), hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    if (raised) return fail(c, std::string(fn) + ": the offsets do not fit this scene and these queries (a slice is shorter than its list, or lies outside prims): "
                                                 "count again and rebuild them with pt_list_offsets");
    return 0;
}

PT_API int pt_query_overlap_lists(pt_ctx* c, const float* boxes, size_t n, const uint32_t* offsets, uint32_t* prims, size_t capacity, uint32_t* found)
{
    int fmt = 0;
    if (int rc = lists_prepare(c, "pt_query_overlap_lists", boxes, n, offsets, prims, capacity, found, &fmt, "boxes", 32u)) return rc < 0 ? 0 : rc;
    Range range("pt_query_overlap_lists");
    const uint32_t cap = capacity > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)capacity;      // no 32-bit offset reaches further
    return lists_run(c, "pt_query_overlap_lists", [&](uint32_t* flag) {
        return ptd::launch_overlap_lists(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)boxes,
                                         (uint32_t)n, offsets, prims, cap, found, flag, c->list_phases, c->stream);
    });
}

PT_API int pt_query_triangles_lists(pt_ctx* c, const float* tris, size_t n, const uint32_t* offsets, uint32_t* prims, size_t capacity, uint32_t* found)
{
    int fmt = 0;
    if (int rc = lists_prepare(c, "pt_query_triangles_lists", tris, n, offsets, prims, capacity, found, &fmt, "triangles", 48u)) return rc < 0 ? 0 : rc;
    Range range("pt_query_triangles_lists");
    const uint32_t cap = capacity > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)capacity;
    return lists_run(c, "pt_query_triangles_lists", [&](uint32_t* flag) {
        return ptd::launch_triangles_lists(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)tris,
                                           (uint32_t)n, offsets, prims, cap, found, flag, c->list_phases, c->stream);
    });
}

PT_API int pt_debug_list_phases(pt_ctx* c, uint32_t phases)
{
    if (!c) return fail(nullptr, "pt_debug_list_phases: null context");
    if (phases > 7u || !(phases & ptd::kListPhaseAll)) return fail(c, "pt_debug_list_phases: phases is 1 (fill), 2 (sort) or 3 (both), plus 4 for no register list");
    c->list_phases = phases;
    return 0;
}

// ---- oriented-box overlap ---------------------------------------------------------------------------------------------------------
// The three calls refuse what pt_query_overlap's and pt_query_overlap_lists' refuse, in the same order (overlap_prepare, lists_prepare);
// a record is 64 bytes.
static float oriented_term(pt_ctx* c) { return ptd::oriented_scene_term(c->bvh.scene_lo, c->bvh.scene_hi); }

PT_API int pt_query_overlap_oriented(pt_ctx* c, const float* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts)
{
    // n < 2^31, max_prims <= 8: the byte counts stay below 2^37
    const OverlapOut outs[2] = {{prims, (size_t)max_prims * 4u, 15u, false, "prims"}, {counts, 4u, 3u, false, "counts"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_overlap_oriented", boxes, n, true, max_prims, outs, 2, &fmt, "boxes", 64u)) return rc < 0 ? 0 : rc;
    Range range("pt_query_overlap_oriented");
    CK(c, ptd::launch_query_oriented(fmt, device_scene(c), c->stack_entries, oriented_term(c), (const float4*)boxes, (uint32_t)n, max_prims, prims, counts, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_overlap_oriented_any(pt_ctx* c, const float* boxes, size_t n, uint8_t* hit)
{
    const OverlapOut outs[1] = {{hit, 1u, 0u, true, "hit"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_overlap_oriented_any", boxes, n, false, 0u, outs, 1, &fmt, "boxes", 64u)) return rc < 0 ? 0 : rc;
    Range range("pt_query_overlap_oriented_any");
    CK(c, ptd::launch_query_oriented_any(fmt, device_scene(c), c->stack_entries, oriented_term(c), (const float4*)boxes, (uint32_t)n, hit, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int oriented_visits_run(pt_ctx* c, const char* fn, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits, bool cross)
{
    const OverlapOut outs[2] = {{counts, 4u, 3u, true, "counts"}, {visits, 8u, 7u, true, "visits"}};
    int fmt = 0;
    if (int rc = overlap_prepare(c, fn, boxes, n, false, 0u, outs, 2, &fmt, "boxes", 64u)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_oriented_visits(fmt, device_scene(c), c->stack_entries, oriented_term(c), (const float4*)boxes, (uint32_t)n, counts, (uint2*)visits, cross, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_overlap_oriented_visits(pt_ctx* c, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits)
{
    return oriented_visits_run(c, "pt_debug_overlap_oriented_visits", boxes, n, counts, visits, false);
}

PT_API int pt_debug_overlap_oriented_visits_cross(pt_ctx* c, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits)
{
    return oriented_visits_run(c, "pt_debug_overlap_oriented_visits_cross", boxes, n, counts, visits, true);
}

PT_API int pt_query_overlap_oriented_lists(pt_ctx* c, const float* boxes, size_t n, const uint32_t* offsets, uint32_t* prims, size_t capacity, uint32_t* found)
{
    int fmt = 0;
    if (int rc = lists_prepare(c, "pt_query_overlap_oriented_lists", boxes, n, offsets, prims, capacity, found, &fmt, "boxes", 64u)) return rc < 0 ? 0 : rc;
    Range range("pt_query_overlap_oriented_lists");
    const uint32_t cap = capacity > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)capacity;      // no 32-bit offset reaches further
    return lists_run(c, "pt_query_overlap_oriented_lists", [&](uint32_t* flag) {
        return ptd::launch_oriented_lists(fmt, device_scene(c), c->stack_entries, oriented_term(c), (const float4*)boxes, (uint32_t)n, offsets, prims, cap, found, flag,
                                          c->list_phases, c->stream);
    });
}

// poses -> oriented-box records.  Needs neither a scene nor a query mesh.  The refusals in the posed calls' order.
PT_API int pt_pose_boxes(pt_ctx* c, const float* poses, size_t P, const float local_box[6], float* boxes_out)
{
    const std::string f = "pt_pose_boxes: ";
    if (!c) return fail(nullptr, f + "null context");
    if (P == 0) return 0;
    if (!poses || !local_box || !boxes_out) return fail(c, f + "null argument");
    if (P > 0x7FFFFFFFull) return fail(c, f + "too many poses (2^31 - 1 per call)");
    for (int k = 0; k < 6; k++)
        if (!std::isfinite(local_box[k]) || (k >= 3 && !(local_box[k] >= 0.0f))) return fail(c, f + "local_box must be finite, its half extent non-negative");
    if ((uintptr_t)poses & 15u) return fail(c, f + "the poses must be 16-byte aligned");
    if ((uintptr_t)boxes_out & 15u) return fail(c, f + "boxes_out must be 16-byte aligned");
    if (spans_overlap(poses, P * 48u, boxes_out, P * 64u)) return fail(c, f + "boxes_out overlaps the poses");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, f + "hipSetDevice failed");
    Range range("pt_pose_boxes");
    CK(c, ptd::launch_pose_boxes((const float4*)poses, (uint32_t)P, local_box[0], local_box[1], local_box[2], local_box[3], local_box[4], local_box[5], (float4*)boxes_out,
                                 c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- segment to mesh -------------------------------------------------------------------------------------------------------------
// every refusal of pt_query_segments before any device work, in pt_query_nearest's order; a segment is 32 bytes.  Returns 0 to go on,
// 1 refused, -1 nothing to do.
static int segments_prepare(pt_ctx* c, const char* fn, const float* segments, size_t n, const void* out, const void* visits, bool with_visits, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!segments || !out || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many segments (2^31 - 1 per call)");
    if (((uintptr_t)segments & 15u) || ((uintptr_t)out & 15u) || ((uintptr_t)visits & 7u)) return fail(c, f + "the segment and record arrays must be 16-byte aligned");
    if (spans_overlap(segments, n * 32u, out, n * sizeof(pt_segment_hit))) return fail(c, f + "the output overlaps the segments");
    if (with_visits && (spans_overlap(segments, n * 32u, visits, n * 8u) || spans_overlap(out, n * sizeof(pt_segment_hit), visits, n * 8u)))
        return fail(c, f + "the visit counts overlap another array");
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_segments(pt_ctx* c, const float* segments, size_t n, pt_segment_hit* out)
{
    int fmt = 0;
    if (int rc = segments_prepare(c, "pt_query_segments", segments, n, out, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_segments");
    CK(c, ptd::launch_query_segments(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)segments,
                                     (uint32_t)n, (float4*)out, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_segments_visits(pt_ctx* c, const float* segments, size_t n, pt_segment_hit* out, uint32_t* visits, uint32_t flags)
{
    if (c && flags > ptd::kSegmentNoAxes) return fail(c, "pt_debug_segments_visits: flags must be 0 or 1");
    int fmt = 0;
    if (int rc = segments_prepare(c, "pt_debug_segments_visits", segments, n, out, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_segments_visits(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)segments,
                                      (uint32_t)n, (float4*)out, (uint2*)visits, flags, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- triangle to mesh distance ----------------------------------------------------------------------------------------------------
// every refusal of pt_query_triangle_distance before any device work, in pt_query_segments' order; a query is 48 bytes and so is a
// record.  Returns 0 to go on, 1 refused, -1 nothing to do.
static int triangle_distance_prepare(pt_ctx* c, const char* fn, const float* tris, size_t n, const void* out, const void* visits, bool with_visits, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!tris || !out || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many triangles (2^31 - 1 per call)");
    if (((uintptr_t)tris & 15u) || ((uintptr_t)out & 15u) || ((uintptr_t)visits & 7u)) return fail(c, f + "the triangle and record arrays must be 16-byte aligned");
    if (spans_overlap(tris, n * 48u, out, n * sizeof(pt_triangle_distance_hit))) return fail(c, f + "the output overlaps the triangles");
    if (with_visits && (spans_overlap(tris, n * 48u, visits, n * 8u) || spans_overlap(out, n * sizeof(pt_triangle_distance_hit), visits, n * 8u)))
        return fail(c, f + "the visit counts overlap another array");
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_triangle_distance(pt_ctx* c, const float* tris, size_t n, pt_triangle_distance_hit* out)
{
    int fmt = 0;
    if (int rc = triangle_distance_prepare(c, "pt_query_triangle_distance", tris, n, out, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_triangle_distance");
    CK(c, ptd::launch_query_triangle_distance(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)tris,
                                              (uint32_t)n, (float4*)out, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_triangle_distance_visits(pt_ctx* c, const float* tris, size_t n, pt_triangle_distance_hit* out, uint32_t* visits, uint32_t flags)
{
    if (c && flags > ptd::kTriDistNoPlane) return fail(c, "pt_debug_triangle_distance_visits: flags must be 0 or 1");
    int fmt = 0;
    if (int rc = triangle_distance_prepare(c, "pt_debug_triangle_distance_visits", tris, n, out, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_triangle_distance_visits(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)tris,
                                               (uint32_t)n, (float4*)out, (uint2*)visits, flags, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- posed-mesh queries ----------------------------------------------------------------------------------------------------------
static_assert(ptd::kPoseMeshMaxTris == PT_QUERY_MESH_MAX, "PT_QUERY_MESH_MAX is pt_set_query_mesh's limit");

PT_API int pt_set_query_mesh(pt_ctx* c, const float* tris, size_t ntris)
{
    const std::string f = "pt_set_query_mesh: ";
    if (!c) return fail(nullptr, f + "null context");
    if (ntris != 0 && !tris) return fail(c, f + "null argument");
    if (ntris > PT_QUERY_MESH_MAX) return fail(c, f + "too many triangles (2^20 per mesh)");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, f + "hipSetDevice failed");
    // the allocation is the mesh's size exactly: the old one goes first (every call that used it has returned synchronised)
    CK(c, hipStreamSynchronize(c->stream));
    c->d_pose_mesh.release();
    c->pose_mesh_tris = 0u;
    if (ntris == 0) return 0;
    CK(c, c->d_pose_mesh.reserve(3u * ntris, c->stream));
    CK(c, hipMemcpyAsync(c->d_pose_mesh.p, tris, ntris * 48u, hipMemcpyHostToDevice, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    c->pose_mesh_tris = (uint32_t)ntris;
    return 0;
}

PT_API int pt_get_query_mesh(pt_ctx* c, size_t* ntris, size_t* device_bytes)
{
    if (!c) return fail(nullptr, "pt_get_query_mesh: null context");
    if (ntris) *ntris = c->pose_mesh_tris;
    if (device_bytes) *device_bytes = c->d_pose_mesh.cap * sizeof(float4);
    return 0;
}

// One array of a posed-mesh call: its bytes, the alignment it needs (a mask), whether the call cannot do without it.
struct PoseSpan { const void* p; size_t bytes; uintptr_t align_mask; bool required; const char* name; };

// every refusal of the posed-mesh calls before any device work, in the siblings' order; spans[0] is the poses.  Returns 0 to go on,
// 1 refused, -1 nothing to do (P == 0).  per_pair: bytes of spans[k] are per posed triangle (pt_pose_triangles' output), known only
// here, where P * T has been judged.
static int poses_prepare(pt_ctx* c, const char* fn, size_t P, PoseSpan* spans, int n_spans, int per_pair, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (P == 0) return -1;
    for (int k = 0; k < n_spans; k++)
        if (spans[k].required && !spans[k].p) return fail(c, f + "null argument");
    if (P > 0x7FFFFFFFull) return fail(c, f + "too many poses (2^31 - 1 per call)");
    const size_t T = c->pose_mesh_tris;
    if (P * T > 0x7FFFFFFFull) return fail(c, f + "too many posed triangles (2^31 - 1 per call): split the poses");      // P < 2^31, T <= 2^20
    if (per_pair >= 0) spans[per_pair].bytes *= T;
    for (int k = 0; k < n_spans; k++)
        if ((uintptr_t)spans[k].p & spans[k].align_mask) return fail(c, f + spans[k].name + " must be " + std::to_string(spans[k].align_mask + 1u) + "-byte aligned");
    for (int k = 1; k < n_spans; k++) {
        if (!spans[k].p) continue;
        for (int j = 0; j < k; j++)
            if (spans[j].p && spans_overlap(spans[j].p, spans[j].bytes, spans[k].p, spans[k].bytes))
                return fail(c, f + spans[k].name + " overlaps " + spans[j].name);
    }
    if (T == 0) return fail(c, f + "no query mesh (pt_set_query_mesh first)");
    return query_node_format(c, f, fmt);
}

PT_API int pt_pose_triangles(pt_ctx* c, const float* poses, size_t P, float* tris_out)
{
    PoseSpan spans[2] = {{poses, P * 48u, 15u, true, "the poses"}, {tris_out, P * 48u, 15u, true, "tris_out"}};
    int fmt = 0;
    if (int rc = poses_prepare(c, "pt_pose_triangles", P, spans, 2, 1, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_pose_triangles");
    CK(c, ptd::launch_pose_triangles(c->d_pose_mesh.p, c->pose_mesh_tris, (const float4*)poses, (uint32_t)P, (float4*)tris_out, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int poses_any_run(pt_ctx* c, const char* fn, const float* poses, size_t P, uint8_t* hit, uint32_t* first, uint32_t flags)
{
    PoseSpan spans[3] = {{poses, P * 48u, 15u, true, "the poses"}, {hit, P, 0u, true, "hit"}, {first, P * 4u, 3u, false, "first"}};
    int fmt = 0;
    if (int rc = poses_prepare(c, fn, P, spans, 3, -1, &fmt)) return rc < 0 ? 0 : rc;
    Range range(fn);
    CK(c, c->d_pose_words.reserve(P, c->stream));
    CK(c, ptd::launch_poses_any(fmt, device_scene(c), c->stack_entries, ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi), c->d_pose_mesh.p, c->pose_mesh_tris,
                                (const float4*)poses, (uint32_t)P, (uint32_t*)c->d_pose_words.p, hit, first, flags, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int poses_distance_run(pt_ctx* c, const char* fn, const float* poses, size_t P, float max_radius, pt_pose_distance_hit* out, uint32_t flags)
{
    PoseSpan spans[2] = {{poses, P * 48u, 15u, true, "the poses"}, {out, P * sizeof(pt_pose_distance_hit), 15u, true, "out"}};
    int fmt = 0;
    if (int rc = poses_prepare(c, fn, P, spans, 2, -1, &fmt)) return rc < 0 ? 0 : rc;
    Range range(fn);
    CK(c, c->d_pose_words.reserve(P, c->stream));
    CK(c, ptd::launch_poses_distance(fmt, device_scene(c), c->stack_entries, ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi), c->d_pose_mesh.p, c->pose_mesh_tris,
                                     (const float4*)poses, (uint32_t)P, max_radius, c->d_pose_words.p, (float4*)out, flags, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_poses_any(pt_ctx* c, const float* poses, size_t P, uint8_t* hit, uint32_t* first)
{
    return poses_any_run(c, "pt_query_poses_any", poses, P, hit, first, 0u);
}

PT_API int pt_query_poses_distance(pt_ctx* c, const float* poses, size_t P, float max_radius, pt_pose_distance_hit* out)
{
    return poses_distance_run(c, "pt_query_poses_distance", poses, P, max_radius, out, 0u);
}

PT_API int pt_debug_query_poses(pt_ctx* c, const float* poses, size_t P, float max_radius, uint8_t* hit, uint32_t* first, pt_pose_distance_hit* out, uint32_t flags)
{
    const std::string f = "pt_debug_query_poses: ";
    if (c && flags > (ptd::kPoseNoEarly | ptd::kPosePoseMajor)) return fail(c, f + "flags is 0..3 (1: no early look, 2: pose-major lanes)");
    if (c && out && (hit || first)) return fail(c, f + "out goes alone, hit (and first) go without it");
    if (out) return poses_distance_run(c, "pt_debug_query_poses", poses, P, max_radius, out, flags);
    return poses_any_run(c, "pt_debug_query_poses", poses, P, hit, first, flags);
}

// ---- swept spheres ---------------------------------------------------------------------------------------------------------------
// every refusal of the three calls before any device work, in pt_query_nearest's order.  out_bytes: bytes of output per sweep.
// Returns 0 to go on, 1 refused, -1 nothing to do (n == 0).
static int sweep_prepare(pt_ctx* c, const char* fn, const float* sweeps, size_t n, const void* out, size_t out_bytes, bool out_aligned, const void* visits,
                         bool with_visits, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!sweeps || !out || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many sweeps (2^31 - 1 per call)");
    if (((uintptr_t)sweeps & 15u) || (out_aligned && ((uintptr_t)out & 15u)) || ((uintptr_t)visits & 7u))
        return fail(c, f + "the sweep and hit arrays must be 16-byte aligned");
    if (spans_overlap(sweeps, n * 32u, out, n * out_bytes)) return fail(c, f + "the output overlaps the sweeps");
    if (with_visits && (spans_overlap(sweeps, n * 32u, visits, n * 8u) || spans_overlap(out, n * out_bytes, visits, n * 8u)))
        return fail(c, f + "the visit counts overlap another array");
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_sweep(pt_ctx* c, const float* sweeps, size_t n, pt_sweep_hit* hits)
{
    int fmt = 0;
    if (int rc = sweep_prepare(c, "pt_query_sweep", sweeps, n, hits, sizeof(pt_sweep_hit), true, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_sweep");
    CK(c, ptd::launch_query_sweep(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)sweeps,
                                  (uint32_t)n, (float4*)hits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_sweep_any(pt_ctx* c, const float* sweeps, size_t n, uint8_t* blocked)
{
    int fmt = 0;
    if (int rc = sweep_prepare(c, "pt_query_sweep_any", sweeps, n, blocked, 1, false, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_sweep_any");
    CK(c, ptd::launch_query_sweep_any(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)sweeps,
                                      (uint32_t)n, blocked, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_sweep_visits(pt_ctx* c, const float* sweeps, size_t n, pt_sweep_hit* hits, uint32_t* visits)
{
    int fmt = 0;
    if (int rc = sweep_prepare(c, "pt_debug_sweep_visits", sweeps, n, hits, sizeof(pt_sweep_hit), true, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_sweep_visits(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)sweeps,
                                   (uint32_t)n, (float4*)hits, (uint2*)visits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- swept capsules ---------------------------------------------------------------------------------------------------------------
// every refusal of the three calls before any device work, in pt_query_sweep's order; a cast is 48 bytes.  out_bytes: bytes of output
// per cast.  Returns 0 to go on, 1 refused, -1 nothing to do (n == 0).
static int capsule_cast_prepare(pt_ctx* c, const char* fn, const float* casts, size_t n, const void* out, size_t out_bytes, bool out_aligned, const void* visits,
                                bool with_visits, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!casts || !out || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many casts (2^31 - 1 per call)");
    if (((uintptr_t)casts & 15u) || (out_aligned && ((uintptr_t)out & 15u)) || ((uintptr_t)visits & 7u))
        return fail(c, f + "the cast and hit arrays must be 16-byte aligned");
    if (spans_overlap(casts, n * 48u, out, n * out_bytes)) return fail(c, f + "the output overlaps the casts");
    if (with_visits && (spans_overlap(casts, n * 48u, visits, n * 8u) || spans_overlap(out, n * out_bytes, visits, n * 8u)))
        return fail(c, f + "the visit counts overlap another array");
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_capsule_cast(pt_ctx* c, const float* casts, size_t n, pt_capsule_cast_hit* hits)
{
    int fmt = 0;
    if (int rc = capsule_cast_prepare(c, "pt_query_capsule_cast", casts, n, hits, sizeof(pt_capsule_cast_hit), true, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_capsule_cast");
    CK(c, ptd::launch_query_capsule_cast(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                         (uint32_t)n, (float4*)hits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_capsule_cast_any(pt_ctx* c, const float* casts, size_t n, uint8_t* blocked)
{
    int fmt = 0;
    if (int rc = capsule_cast_prepare(c, "pt_query_capsule_cast_any", casts, n, blocked, 1, false, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_capsule_cast_any");
    CK(c, ptd::launch_query_capsule_cast_any(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                             (uint32_t)n, blocked, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_capsule_cast_visits(pt_ctx* c, const float* casts, size_t n, pt_capsule_cast_hit* hits, uint32_t* visits, uint32_t mode)
{
    if (c && mode > 1u) return fail(c, "pt_debug_capsule_cast_visits: mode is 0 (the product's walk) or 1 (without the plane axis)");
    int fmt = 0;
    if (int rc = capsule_cast_prepare(c, "pt_debug_capsule_cast_visits", casts, n, hits, sizeof(pt_capsule_cast_hit), true, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_capsule_cast_visits(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                          (uint32_t)n, (float4*)hits, (uint2*)visits, mode == 0u && ptd::kCapsulePlane, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- swept oriented boxes ---------------------------------------------------------------------------------------------------------
// every refusal of the three calls before any device work, in pt_query_capsule_cast's order; a cast is 80 bytes.  out_bytes: bytes of
// output per cast.  Returns 0 to go on, 1 refused, -1 nothing to do (n == 0).
static int box_cast_prepare(pt_ctx* c, const char* fn, const float* casts, size_t n, const void* out, size_t out_bytes, bool out_aligned, const void* visits,
                            bool with_visits, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!casts || !out || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many casts (2^31 - 1 per call)");
    if (((uintptr_t)casts & 15u) || (out_aligned && ((uintptr_t)out & 15u)) || ((uintptr_t)visits & 7u))
        return fail(c, f + "the cast and hit arrays must be 16-byte aligned");
    if (spans_overlap(casts, n * 80u, out, n * out_bytes)) return fail(c, f + "the output overlaps the casts");
    if (with_visits && (spans_overlap(casts, n * 80u, visits, n * 8u) || spans_overlap(out, n * out_bytes, visits, n * 8u)))
        return fail(c, f + "the visit counts overlap another array");
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_box_cast(pt_ctx* c, const float* casts, size_t n, pt_box_cast_hit* hits)
{
    int fmt = 0;
    if (int rc = box_cast_prepare(c, "pt_query_box_cast", casts, n, hits, sizeof(pt_box_cast_hit), true, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_box_cast");
    CK(c, ptd::launch_query_box_toi(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                    (uint32_t)n, (float4*)hits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_box_cast_any(pt_ctx* c, const float* casts, size_t n, uint8_t* blocked)
{
    int fmt = 0;
    if (int rc = box_cast_prepare(c, "pt_query_box_cast_any", casts, n, blocked, 1, false, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_box_cast_any");
    CK(c, ptd::launch_query_box_toi_any(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                        (uint32_t)n, blocked, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_box_cast_visits(pt_ctx* c, const float* casts, size_t n, pt_box_cast_hit* hits, uint32_t* visits, uint32_t mode)
{
    if (c && mode > 1u) return fail(c, "pt_debug_box_cast_visits: mode is 0 (the walk with the extra axes) or 1 (the slab alone)");
    int fmt = 0;
    if (int rc = box_cast_prepare(c, "pt_debug_box_cast_visits", casts, n, hits, sizeof(pt_box_cast_hit), true, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_box_toi_visits(fmt, device_scene(c), c->stack_entries, ptd::sweep_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                     (uint32_t)n, (float4*)hits, (uint2*)visits, mode == 0u, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- translating-triangle casts ---------------------------------------------------------------------------------------------------
// every refusal of the three per-triangle calls before any device work, in pt_query_triangle_distance's order; a cast is 64 bytes.
// out_bytes: bytes of output per cast.  Returns 0 to go on, 1 refused, -1 nothing to do (n == 0).
static int triangle_cast_prepare(pt_ctx* c, const char* fn, const float* casts, size_t n, const void* out, size_t out_bytes, bool out_aligned, const void* visits,
                                 bool with_visits, int* fmt)
{
    const std::string f = std::string(fn) + ": ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return -1;
    if (!casts || !out || (with_visits && !visits)) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many casts (2^31 - 1 per call)");
    if (((uintptr_t)casts & 15u) || (out_aligned && ((uintptr_t)out & 15u))) return fail(c, f + "the cast and hit arrays must be 16-byte aligned");
    if ((uintptr_t)visits & 7u) return fail(c, f + "the visit counts must be 8-byte aligned");
    if (spans_overlap(casts, n * 64u, out, n * out_bytes)) return fail(c, f + "the output overlaps the casts");
    if (with_visits && (spans_overlap(casts, n * 64u, visits, n * 8u) || spans_overlap(out, n * out_bytes, visits, n * 8u)))
        return fail(c, f + "the visit counts overlap another array");
    return query_node_format(c, f, fmt);
}

PT_API int pt_query_triangle_cast(pt_ctx* c, const float* casts, size_t n, pt_triangle_cast_hit* hits)
{
    int fmt = 0;
    if (int rc = triangle_cast_prepare(c, "pt_query_triangle_cast", casts, n, hits, sizeof(pt_triangle_cast_hit), true, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_triangle_cast");
    CK(c, ptd::launch_query_triangle_cast(fmt, device_scene(c), c->stack_entries, ptd::cast_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                          (uint32_t)n, (float4*)hits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_triangle_cast_any(pt_ctx* c, const float* casts, size_t n, uint8_t* blocked)
{
    int fmt = 0;
    if (int rc = triangle_cast_prepare(c, "pt_query_triangle_cast_any", casts, n, blocked, 1, false, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    Range range("pt_query_triangle_cast_any");
    CK(c, ptd::launch_query_triangle_cast_any(fmt, device_scene(c), c->stack_entries, ptd::cast_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                              (uint32_t)n, blocked, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_debug_triangle_cast_visits(pt_ctx* c, const float* casts, size_t n, pt_triangle_cast_hit* hits, uint32_t* visits)
{
    int fmt = 0;
    if (int rc = triangle_cast_prepare(c, "pt_debug_triangle_cast_visits", casts, n, hits, sizeof(pt_triangle_cast_hit), true, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    CK(c, ptd::launch_triangle_cast_visits(fmt, device_scene(c), c->stack_entries, ptd::cast_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), (const float4*)casts,
                                           (uint32_t)n, (float4*)hits, (uint2*)visits, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int poses_cast_run(pt_ctx* c, const char* fn, const float* poses, const float* motions, size_t P, pt_triangle_cast_hit* out, uint32_t flags)
{
    PoseSpan spans[3] = {{poses, P * 48u, 15u, true, "the poses"}, {motions, P * 16u, 15u, true, "the motions"}, {out, P * sizeof(pt_triangle_cast_hit), 15u, true, "out"}};
    int fmt = 0;
    if (int rc = poses_prepare(c, fn, P, spans, 3, -1, &fmt)) return rc < 0 ? 0 : rc;
    Range range(fn);
    CK(c, c->d_pose_words.reserve(P, c->stream));
    CK(c, ptd::launch_poses_cast(fmt, device_scene(c), c->stack_entries, ptd::cast_scene_scale(c->bvh.scene_lo, c->bvh.scene_hi), c->d_pose_mesh.p, c->pose_mesh_tris,
                                 (const float4*)poses, (const float4*)motions, (uint32_t)P, c->d_pose_words.p, (float4*)out, flags, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_query_poses_cast(pt_ctx* c, const float* poses, const float* motions, size_t P, pt_triangle_cast_hit* out)
{
    return poses_cast_run(c, "pt_query_poses_cast", poses, motions, P, out, 0u);
}

PT_API int pt_debug_query_poses_cast(pt_ctx* c, const float* poses, const float* motions, size_t P, pt_triangle_cast_hit* out, uint32_t flags)
{
    if (c && flags > (ptd::kPoseNoEarly | ptd::kPosePoseMajor)) return fail(c, "pt_debug_query_poses_cast: flags is 0..3 (1: no early look, 2: pose-major lanes)");
    return poses_cast_run(c, "pt_debug_query_poses_cast", poses, motions, P, out, flags);
}

// ---- ambient occlusion ----------------------------------------------------------------------------------------------------------
// every refusal of the two calls before any device work, in this order.  in: the points or the feature buffer, in_bytes per point.
// On 0 the disk pattern is in c->d_ao_disk (enqueued on the context's stream) and *args is what the kernel gets.
static int ao_prepare(pt_ctx* c, const std::string& f, const void* in, size_t in_bytes, size_t n, const float* disk, const pt_ao_params* ap,
                      const uint32_t* visible, const float* ao, int* fmt, ptd::AoArgs* args)
{
    if (!in || !disk || !ap || !visible) return fail(c, f + "null argument");
    if (n > 0x7FFFFFFFull) return fail(c, f + "too many points (2^31 - 1 per call)");
    if (((uintptr_t)in & 15u) || ((uintptr_t)visible & 3u) || ((uintptr_t)ao & 3u)) return fail(c, f + "the input must be 16-byte aligned, the outputs 4-byte aligned");
    if (ap->samples < 1u || ap->samples > ptd::kAoMaxSamples) return fail(c, f + "samples must be 1..256");
    if (!(ap->radius > 0.0f) || !std::isfinite(ap->radius)) return fail(c, f + "radius must be positive and finite");
    if (!(ap->bias >= 0.0f) || !std::isfinite(ap->bias)) return fail(c, f + "bias must be non-negative and finite");
    if (ap->total_samples < ap->samples) return fail(c, f + "total_samples must be at least samples");
    if (ap->reserved[0] || ap->reserved[1]) return fail(c, f + "reserved fields must be 0");
    for (uint32_t k = 0; k < ap->samples; k++) {
        const float x = disk[2u * k], y = disk[2u * k + 1u];
        if (!std::isfinite(x) || !std::isfinite(y) || !(x * x + y * y <= 1.0f))
            return fail(c, f + "disk point " + std::to_string(k) + " is outside the unit disk");
    }
    if (spans_overlap(in, n * in_bytes, visible, n * 4u)) return fail(c, f + "visible overlaps the input");
    if (ao && spans_overlap(in, n * in_bytes, ao, n * 4u)) return fail(c, f + "ao overlaps the input");
    if (ao && spans_overlap(visible, n * 4u, ao, n * 4u)) return fail(c, f + "ao overlaps visible");
    if (int rc = query_node_format(c, f, fmt)) return rc;
    CK(c, c->d_ao_disk.reserve(ptd::kAoMaxSamples, c->stream));
    CK(c, hipMemcpyAsync(c->d_ao_disk.p, disk, (size_t)ap->samples * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    *args = {ap->samples, ap->radius, ap->bias, ap->seed, ap->accumulate, ap->total_samples};
    return 0;
}

PT_API int pt_ao_points(pt_ctx* c, const float* points, size_t n, const float* disk, const pt_ao_params* ap, uint32_t* visible, float* ao)
{
    const std::string f = "pt_ao_points: ";
    if (!c) return fail(nullptr, f + "null context");
    if (n == 0) return 0;
    int fmt = 0;
    ptd::AoArgs args;
    if (int rc = ao_prepare(c, f, points, 32u, n, disk, ap, visible, ao, &fmt, &args)) return rc;
    Range range("pt_ao_points");
    CK(c, ptd::launch_ao_points(fmt, device_scene(c), c->stack_entries, (const float4*)points, (uint32_t)n, c->d_ao_disk.p, args, visible, ao, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PT_API int pt_ao_image(pt_ctx* c, const pt_params* p, const float* normal_depth, const float* disk, const pt_ao_params* ap, uint32_t* visible, float* ao)
{
    const std::string f = "pt_ao_image: ";
    if (!c) return fail(nullptr, f + "null context");
    if (!p) return fail(c, f + "null argument");
    const size_t n = (size_t)p->width * p->height;
    if (n == 0) return 0;
    int fmt = 0;
    ptd::AoArgs args;
    if (int rc = ao_prepare(c, f, normal_depth, 16u, n, disk, ap, visible, ao, &fmt, &args)) return rc;
    Range range("pt_ao_image");
    const ptd::AoView view = {p->cameraEye, p->cameraU, p->cameraV, p->cameraW, p->width, p->height};
    CK(c, ptd::launch_ao_image(fmt, device_scene(c), c->stack_entries, view, (const float4*)normal_depth, c->d_ao_disk.p, args, visible, ao, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return 0;
}
