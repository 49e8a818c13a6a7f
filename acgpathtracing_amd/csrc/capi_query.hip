// capi_query.hip — the entry points of include/acgpt.h (and their counting twins of include/acgpt_test.h) that answer queries in
// device memory.  Host code only.  Every call refuses through check_arrays ("Query entry points") and ends in run_query.
// The kernels' one walk, leaf routine and launch are in bvh_walk.h, closest_point.h and query_launch.h; the context: context.h.
//
//   entry points                                                            kernels        checker row
//   pt_query_closest, _any                                                  query.hip      records_prepare(kRays)
//   pt_query_multi                                                          multihit.hip   check_arrays, named
//   pt_query_nearest (+ visits)                                             nearest.hip    records_prepare(kPoints)
//   pt_query_nearest_k, pt_query_within_any (+ visits)                      nearest_k.hip  nearest_k_prepare: check_arrays, named
//   pt_query_winding (+ visits)                                             winding.hip    winding_prepare: records_prepare(kWindingPoints)
//   pt_query_overlap, _any (+ visits)                                       overlap.hip    overlap_prepare: check_arrays, named
//   pt_query_triangles, _any (+ visits)                                     tritri.hip     overlap_prepare
//   pt_query_overlap_oriented, _any (+ visits, visits_cross)                oriented.hip   overlap_prepare
//   pt_query_overlap_lists, pt_query_triangles_lists, .._oriented_lists     lists.hip      lists_prepare: check_arrays, named
//   pt_list_offsets, pt_debug_list_phases                                   lists.hip      their own (no scene)
//   pt_pose_boxes                                                           oriented.hip   its own (no scene)
//   pt_query_segments (+ visits)                                            segment.hip    records_prepare(kSegments)
//   pt_query_triangle_distance (+ visits)                                   tridist.hip    records_prepare(kTriangles)
//   pt_set_query_mesh, pt_get_query_mesh                                    —              their own (no scene)
//   pt_pose_triangles, pt_query_poses_any, _distance, pt_debug_query_poses  poses.hip      poses_prepare: check_arrays, named
//   pt_query_sweep, _any (+ visits)                                         sweep.hip      records_prepare(kSweeps)
//   pt_query_capsule_cast, _any (+ visits)                                  capsule.hip    records_prepare(kCapsuleCasts)
//   pt_query_box_cast, _any (+ visits)                                      boxcast.hip    records_prepare(kBoxCasts)
//   pt_query_triangle_cast, _any (+ visits)                                 tricast.hip    records_prepare(kTriangleCasts)
//   pt_query_poses_cast, pt_debug_query_poses_cast                          tricast.hip    poses_prepare
//   pt_ao_points, pt_ao_image                                               ao.hip         ao_prepare: its own order, first_overlap
#include <cmath>
#include <optional>

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
#include "query_launch.h"
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

// ---- what every call shares: the refusals, the run, the scene's terms ---------------------------------------------------------------
// The node array the scene holds, as pt_render_features picks it: fp16 centre / half-extent nodes for the default variants, fp32
// nodes for the fp32 ones; only a variant forced onto another format (pt_set_tuning) leaves neither and gets the fp32 nodes back.
// The last refusals of a call: no scene, no device.
static int refuse(pt_ctx* c, const char* fn, const std::string& why) { return fail(c, std::string(fn) + ": " + why); }

static int query_node_format(pt_ctx* c, const char* fn, int* fmt)
{
    if (c->scene_serial == 0) return refuse(c, fn, "no scene (pt_set_scene first)");
    if (hipSetDevice(c->device) != hipSuccess) return refuse(c, fn, "hipSetDevice failed");
    *fmt = 0;
    if (c->bvh.hcnodes) *fmt = 11;
    else if (int rc = ensure_node_format(c, 0)) return rc;
    return 0;
}

// One array of a call: its bytes, the alignment it needs (a mask), whether the call cannot do without it, its name in "X overlaps Y",
// and what a misaligned pointer is told (null: "<name> must be N-byte aligned").  A null optional array takes part in nothing.
struct Span { const void* p; size_t bytes; uintptr_t align_mask; bool required; const char* name; const char* misaligned; };

// The checks only one call has, each as the message it failed with (null: passed), named by the step of check_arrays it follows.
struct OwnChecks { const char* first = nullptr; const char* counted = nullptr; const char* aligned = nullptr; const char* disjoint = nullptr; };

// the first pair of arrays that share a byte, later array first, each against the ones before it in order
static bool first_overlap(const Span* s, int n_spans, int* later, int* earlier)
{
    for (int k = 1; k < n_spans; k++) {
        if (!s[k].p) continue;
        for (int j = 0; j < k; j++)
            if (s[j].p && spans_overlap(s[j].p, s[j].bytes, s[k].p, s[k].bytes)) {
                *later = k;
                *earlier = j;
                return true;
            }
    }
    return false;
}

// Every refusal of a query before any device work, in the one order all of them keep: null context, n == 0 (nothing to do), the call's
// own limits, a null argument, too many <noun>, alignment, overlaps, (no query mesh), no scene.  s[0] is the input.  named: an overlap
// reads "X overlaps Y"; otherwise s is {input, output, visit counts} and it reads "the output overlaps the <noun>" or "the visit counts
// overlap another array".  *fmt: the node format the scene holds.  Returns 0 to go on, 1 refused, -1 nothing to do.
static int check_arrays(pt_ctx* c, const char* fn, size_t n, const char* noun, const Span* s, int n_spans, const OwnChecks& own, bool named, int* fmt)
{
    if (!c) return refuse(nullptr, fn, "null context");
    if (n == 0) return -1;
    if (own.first) return refuse(c, fn, own.first);
    for (int k = 0; k < n_spans; k++)
        if (s[k].required && !s[k].p) return refuse(c, fn, "null argument");
    if (n > 0x7FFFFFFFull) return refuse(c, fn, std::string("too many ") + noun + " (2^31 - 1 per call)");
    if (own.counted) return refuse(c, fn, own.counted);
    for (int k = 0; k < n_spans; k++)
        if ((uintptr_t)s[k].p & s[k].align_mask)
            return refuse(c, fn, s[k].misaligned ? std::string(s[k].misaligned) : s[k].name + (" must be " + std::to_string(s[k].align_mask + 1u)) + "-byte aligned");
    if (own.aligned) return refuse(c, fn, own.aligned);
    int k = 0, j = 0;
    if (first_overlap(s, n_spans, &k, &j))
        return refuse(c, fn, named ? std::string(s[k].name) + " overlaps " + s[j].name : k == 1 ? std::string("the output overlaps the ") + noun : "the visit counts overlap another array");
    if (own.disjoint) return refuse(c, fn, own.disjoint);
    return query_node_format(c, fn, fmt);
}

// The input records of the calls with one output per record and, in the counting twin, the visit counts: their noun, the bytes of
// one, and the sentence a misaligned array gets (visits: the visit counts' own, where they have one).
struct Records { const char* noun; size_t bytes; const char* misaligned; const char* visits_misaligned; };
static const Records kRays = {"rays", 32u, "the ray and hit arrays must be 16-byte aligned", nullptr};
static const Records kPoints = {"points", 16u, "the point and record arrays must be 16-byte aligned", nullptr};
static const Records kWindingPoints = {"points", 16u, "the points must be 16-byte aligned, the output 4-byte aligned", nullptr};
static const Records kSegments = {"segments", 32u, "the segment and record arrays must be 16-byte aligned", nullptr};
static const Records kTriangles = {"triangles", 48u, "the triangle and record arrays must be 16-byte aligned", nullptr};
static const Records kSweeps = {"sweeps", 32u, "the sweep and hit arrays must be 16-byte aligned", nullptr};
static const Records kCapsuleCasts = {"casts", 48u, "the cast and hit arrays must be 16-byte aligned", nullptr};
static const Records kBoxCasts = {"casts", 80u, "the cast and hit arrays must be 16-byte aligned", nullptr};
static const Records kTriangleCasts = {"casts", 64u, "the cast and hit arrays must be 16-byte aligned", "the visit counts must be 8-byte aligned"};

// check_arrays for those calls.  out_bytes: bytes of output per record, out_mask its alignment (0: a byte each); visits: null in the
// product calls, required in the twins (with_visits).
static int records_prepare(pt_ctx* c, const char* fn, const Records& r, const void* in, size_t n, const void* out, size_t out_bytes, uintptr_t out_mask,
                           const void* visits, bool with_visits, int* fmt, const char* own_first = nullptr)
{
    const Span s[3] = {{in, n * r.bytes, 15u, true, r.noun, r.misaligned},
                       {out, n * out_bytes, out_mask, true, "the output", r.misaligned},
                       {visits, n * 8u, 7u, with_visits, "the visit counts", r.visits_misaligned ? r.visits_misaligned : r.misaligned}};
    OwnChecks own;
    own.first = own_first;
    return check_arrays(c, fn, n, r.noun, s, 3, own, false, fmt);
}

// The end of every call: the launch and the sync under the call's ROCTx range (product calls; the counting twins have none), a HIP
// error reported as "<entry point>: <error string>".
template <typename Launch>
static int run_query(pt_ctx* c, const char* fn, bool product, Launch launch)
{
    std::optional<Range> range;
    if (product) range.emplace(fn);
    hipError_t e = launch();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return refuse(c, fn, hipGetErrorString(e));
    return 0;
}

// the scene's terms the kernels get, each from the scene's box
static float nearest_abs_term(pt_ctx* c) { return ptd::nearest_abs_term(c->bvh.scene_lo, c->bvh.scene_hi); }
static float overlap_scene_term(pt_ctx* c) { return ptd::overlap_scene_term(c->bvh.scene_lo, c->bvh.scene_hi); }
static float oriented_term(pt_ctx* c) { return ptd::oriented_scene_term(c->bvh.scene_lo, c->bvh.scene_hi); }
static float query_scene_scale(pt_ctx* c) { return ptd::scene_max_abs(c->bvh.scene_lo, c->bvh.scene_hi); }      // S of sweep.h, capsule.h, boxcast.h, tricast.h

// ---- rays -------------------------------------------------------------------------------------------------------------------------
PT_API int pt_query_closest(pt_ctx* c, const float* rays, size_t n, pt_hit* hits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_closest", kRays, rays, n, hits, sizeof(pt_hit), 15u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_closest", true, [&] {
        return ptd::launch_query_closest(fmt, device_scene(c), c->stack_entries, (const float4*)rays, (uint32_t)n, (float4*)hits, c->stream);
    });
}

PT_API int pt_query_any(pt_ctx* c, const float* rays, size_t n, uint8_t* occluded)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_any", kRays, rays, n, occluded, 1u, 0u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_any", true, [&] {
        return ptd::launch_query_any(fmt, device_scene(c), c->stack_entries, (const float4*)rays, (uint32_t)n, occluded, c->stream);
    });
}

// ---- the first hits in order, and their number -----------------------------------------------------------------------------------
static_assert(PT_QUERY_MULTI_MAX == ptd::kMultiMaxHits, "PT_QUERY_MULTI_MAX is the size of the kernel's largest list");

// The limits of a call with a list of `list` and `counts`: the message of the first one broken, or null.  at_most: "<max> must be at
// most <limit>", both_or_neither: "<list> goes with <max>: both or neither", nothing: "nothing to write (<list> and counts are both null)".
static const char* list_limits(uint32_t max, uint32_t limit, const void* list, const void* counts, const char* at_most, const char* both_or_neither, const char* nothing)
{
    if (max > limit) return at_most;
    if ((max != 0u) != (list != nullptr)) return both_or_neither;
    if (!list && !counts) return nothing;
    return nullptr;
}

PT_API int pt_query_multi(pt_ctx* c, const float* rays, size_t n, uint32_t max_hits, pt_hit* hits, uint32_t* counts)
{
    static const std::string at_most = "max_hits must be at most " + std::to_string(PT_QUERY_MULTI_MAX);
    const char* one = "the ray and hit arrays must be 16-byte aligned, the counts 4-byte aligned";
    // n < 2^31, max_hits <= 8: the hits' bytes stay below 2^39
    const Span s[3] = {{rays, n * 32u, 15u, true, "the rays", one}, {hits, n * (size_t)max_hits * sizeof(pt_hit), 15u, false, "hits", one}, {counts, n * 4u, 3u, false, "counts", one}};
    OwnChecks own;
    own.first = list_limits(max_hits, PT_QUERY_MULTI_MAX, hits, counts, at_most.c_str(), "hits goes with max_hits: both or neither", "nothing to write (hits and counts are both null)");
    int fmt = 0;
    if (int rc = check_arrays(c, "pt_query_multi", n, "rays", s, 3, own, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_multi", true, [&] {
        return ptd::launch_query_multi(fmt, device_scene(c), c->stack_entries, (const float4*)rays, (uint32_t)n, max_hits, (float4*)hits, counts, c->stream);
    });
}

// ---- closest point ---------------------------------------------------------------------------------------------------------------
PT_API int pt_query_nearest(pt_ctx* c, const float* points, size_t n, pt_nearest* out)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_nearest", kPoints, points, n, out, sizeof(pt_nearest), 15u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_nearest", true, [&] {
        return ptd::launch_query_nearest(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)points, (uint32_t)n, (float4*)out, c->stream);
    });
}

PT_API int pt_debug_nearest_visits(pt_ctx* c, const float* points, size_t n, pt_nearest* out, uint32_t* visits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_debug_nearest_visits", kPoints, points, n, out, sizeof(pt_nearest), 15u, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_nearest_visits", false, [&] {
        return ptd::launch_nearest_visits(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)points, (uint32_t)n, (float4*)out, (uint2*)visits, c->stream);
    });
}

// ---- the K closest triangles, anything within a radius ----------------------------------------------------------------------------
static_assert(PT_QUERY_NEAREST_MAX == ptd::kNearestMaxK, "PT_QUERY_NEAREST_MAX is the size of the kernel's largest list");

// check_arrays for the two calls and their twin.  list: the call has max_k, out and counts; otherwise it has hit.  visits: null unless
// with_visits.
static int nearest_k_prepare(pt_ctx* c, const char* fn, const float* points, size_t n, bool list, uint32_t max_k, const void* out, const void* counts,
                             const void* hit, const void* visits, bool with_visits, int* fmt)
{
    static const std::string at_most = "max_k must be at most " + std::to_string(PT_QUERY_NEAREST_MAX);
    const char* one = "the point and record arrays must be 16-byte aligned, the counts 4-byte aligned";
    // n < 2^31, max_k <= 8: the byte counts stay below 2^39
    const Span s[5] = {{points, n * 16u, 15u, true, "the points", one}, {out, n * (size_t)max_k * sizeof(pt_nearest), 15u, false, "out", one},
                       {counts, n * 4u, 3u, false, "counts", one}, {hit, n, 0u, !list, "hit", one}, {visits, n * 8u, 7u, with_visits, "the visit counts", one}};
    OwnChecks own;
    if (list) own.first = list_limits(max_k, PT_QUERY_NEAREST_MAX, out, counts, at_most.c_str(), "out goes with max_k: both or neither", "nothing to write (out and counts are both null)");
    return check_arrays(c, fn, n, "points", s, 5, own, true, fmt);
}

PT_API int pt_query_nearest_k(pt_ctx* c, const float* points, size_t n, uint32_t max_k, pt_nearest* out, uint32_t* counts)
{
    int fmt = 0;
    if (int rc = nearest_k_prepare(c, "pt_query_nearest_k", points, n, true, max_k, out, counts, nullptr, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_nearest_k", true, [&] {
        return ptd::launch_query_nearest_k(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)points, (uint32_t)n, max_k, (float4*)out, counts, c->stream);
    });
}

PT_API int pt_query_within_any(pt_ctx* c, const float* points, size_t n, uint8_t* hit)
{
    int fmt = 0;
    if (int rc = nearest_k_prepare(c, "pt_query_within_any", points, n, false, 0u, nullptr, nullptr, hit, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_within_any", true, [&] {
        return ptd::launch_query_within_any(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)points, (uint32_t)n, hit, c->stream);
    });
}

PT_API int pt_debug_nearest_k_visits(pt_ctx* c, const float* points, size_t n, uint32_t max_k, pt_nearest* out, uint32_t* counts, uint8_t* hit, uint32_t* visits)
{
    if (c && hit && (max_k != 0u || out || counts)) return fail(c, "pt_debug_nearest_k_visits: hit goes with max_k 0 and no out or counts");
    int fmt = 0;
    if (int rc = nearest_k_prepare(c, "pt_debug_nearest_k_visits", points, n, hit == nullptr, max_k, out, counts, hit, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_nearest_k_visits", false, [&] {
        return ptd::launch_nearest_k_visits(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)points, (uint32_t)n, max_k, (float4*)out, counts, hit,
                                            (uint2*)visits, hit ? 1u : 0u, c->stream);
    });
}

// ---- generalised winding numbers ---------------------------------------------------------------------------------------------------
static_assert(sizeof(pt_winding_info) == 16, "pt_winding_info: a change of this layout bumps pt_abi_version");

// check_arrays with a bad beta as the call's own limit; then the moments, built on the first call after the scene or its vertices
// changed.  Returns 0 to go on, 1 refused or failed, -1 nothing to do.
static int winding_prepare(pt_ctx* c, const char* fn, const float* points, size_t n, float beta, const void* out, const void* visits, bool with_visits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, fn, kWindingPoints, points, n, out, 4u, 3u, visits, with_visits, &fmt, beta >= 1.0f ? nullptr : "beta must be at least 1 (+inf: the exact sum)"))
        return rc;
    if (c->bvh.n_tris != 0u && !c->winding.built) {
        Range range("acgpt: winding moments");
        std::string err;
        if (!ptd::build_winding(c->bvh, c->stream, c->winding, err)) return refuse(c, fn, err);
    }
    return 0;
}

PT_API int pt_query_winding(pt_ctx* c, const float* points, size_t n, float beta, float* out)
{
    if (int rc = winding_prepare(c, "pt_query_winding", points, n, beta, out, nullptr, false)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_winding", true, [&] {
        return ptd::launch_query_winding(c->winding, c->bvh.tris, c->bvh.n_tris, c->stack_entries, beta * beta, (const float4*)points, (uint32_t)n, out, c->stream);
    });
}

PT_API int pt_debug_winding_visits(pt_ctx* c, const float* points, size_t n, float beta, float* out, uint32_t* visits)
{
    if (int rc = winding_prepare(c, "pt_debug_winding_visits", points, n, beta, out, visits, true)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_winding_visits", false, [&] {
        return ptd::launch_winding_visits(c->winding, c->bvh.tris, c->bvh.n_tris, c->stack_entries, beta * beta, (const float4*)points, (uint32_t)n, out, (uint2*)visits, c->stream);
    });
}

// ---- box overlap -----------------------------------------------------------------------------------------------------------------
static_assert(PT_QUERY_OVERLAP_MAX == ptd::kOverlapMaxPrims, "PT_QUERY_OVERLAP_MAX is the size of the kernel's largest list");

// The input records of the overlap, triangle and oriented-box calls: the noun, its name in "X overlaps Y", the bytes of one.
struct Shapes { const char* noun; const char* name; size_t bytes; };
static const Shapes kBoxes = {"boxes", "the boxes", 32u}, kQueryTriangles = {"triangles", "the triangles", 48u}, kOrientedBoxes = {"boxes", "the boxes", 64u};

// check_arrays for the three kinds of call on those records: the list (max_prims, prims, counts), the any-hit call (hit), the
// counting twin (counts, visits).  What a kind does not have is null.
enum OverlapKind { kOverlapList, kOverlapAny, kOverlapTwin };
static int overlap_prepare(pt_ctx* c, const char* fn, const Shapes& in, OverlapKind kind, const float* recs, size_t n, uint32_t max_prims, const void* prims,
                           const void* counts, const void* hit, const void* visits, int* fmt)
{
    static const std::string at_most = "max_prims must be at most " + std::to_string(PT_QUERY_OVERLAP_MAX);
    // n < 2^31, max_prims <= 8: the byte counts stay below 2^37
    const Span s[5] = {{recs, n * in.bytes, 15u, true, in.name, nullptr},
                       {prims, n * (size_t)max_prims * 4u, 15u, false, "prims", nullptr},
                       {counts, n * 4u, 3u, kind == kOverlapTwin, "counts", nullptr},
                       {hit, n, 0u, kind == kOverlapAny, "hit", nullptr},
                       {visits, n * 8u, 7u, kind == kOverlapTwin, "visits", nullptr}};
    OwnChecks own;
    if (kind == kOverlapList)
        own.first = list_limits(max_prims, PT_QUERY_OVERLAP_MAX, prims, counts, at_most.c_str(), "prims goes with max_prims: both or neither", "nothing to write (prims and counts are both null)");
    return check_arrays(c, fn, n, in.noun, s, 5, own, true, fmt);
}

PT_API int pt_query_overlap(pt_ctx* c, const float* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_overlap", kBoxes, kOverlapList, boxes, n, max_prims, prims, counts, nullptr, nullptr, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_overlap", true, [&] {
        return ptd::launch_query_overlap(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), (const float4*)boxes, (uint32_t)n, max_prims, prims, counts, c->stream);
    });
}

PT_API int pt_query_overlap_any(pt_ctx* c, const float* boxes, size_t n, uint8_t* hit)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_overlap_any", kBoxes, kOverlapAny, boxes, n, 0u, nullptr, nullptr, hit, nullptr, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_overlap_any", true, [&] {
        return ptd::launch_query_overlap_any(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), (const float4*)boxes, (uint32_t)n, hit, c->stream);
    });
}

PT_API int pt_debug_overlap_visits(pt_ctx* c, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_debug_overlap_visits", kBoxes, kOverlapTwin, boxes, n, 0u, nullptr, counts, nullptr, visits, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_overlap_visits", false, [&] {
        return ptd::launch_overlap_visits(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), (const float4*)boxes, (uint32_t)n, counts, (uint2*)visits, c->stream);
    });
}

// ---- triangle against mesh -------------------------------------------------------------------------------------------------------
static_assert(PT_QUERY_TRIANGLES_MAX == ptd::kTrianglesMaxPrims, "PT_QUERY_TRIANGLES_MAX is the size of the kernel's largest list");
static_assert(PT_QUERY_TRIANGLES_MAX == PT_QUERY_OVERLAP_MAX, "overlap_prepare names one limit for both");

// The three calls refuse what pt_query_overlap's refuse, in the same order (overlap_prepare); a query is 48 bytes.
PT_API int pt_query_triangles(pt_ctx* c, const float* tris, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_triangles", kQueryTriangles, kOverlapList, tris, n, max_prims, prims, counts, nullptr, nullptr, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_triangles", true, [&] {
        return ptd::launch_query_triangles(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), (const float4*)tris, (uint32_t)n, max_prims, prims, counts, c->stream);
    });
}

PT_API int pt_query_triangles_any(pt_ctx* c, const float* tris, size_t n, uint8_t* hit)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_triangles_any", kQueryTriangles, kOverlapAny, tris, n, 0u, nullptr, nullptr, hit, nullptr, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_triangles_any", true, [&] {
        return ptd::launch_query_triangles_any(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), (const float4*)tris, (uint32_t)n, hit, c->stream);
    });
}

PT_API int pt_debug_triangles_visits(pt_ctx* c, const float* tris, size_t n, uint32_t* counts, uint32_t* visits)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_debug_triangles_visits", kQueryTriangles, kOverlapTwin, tris, n, 0u, nullptr, counts, nullptr, visits, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_triangles_visits", false, [&] {
        return ptd::launch_triangles_visits(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), (const float4*)tris, (uint32_t)n, counts, (uint2*)visits, c->stream);
    });
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

// A list call from its refusals (check_arrays, with the capacity judged once the arrays are known to be aligned) to its end: the flag
// is cleared, the lists are written, the flag is read after the sync; a raised flag is the call's failure, the lists stay.
// launch(fmt, cap, flag): cap is the capacity as the kernels take it.
template <typename Launch>
static int lists_run(pt_ctx* c, const char* fn, const Shapes& in, const float* recs, size_t n, const uint32_t* offsets, const uint32_t* prims, size_t capacity,
                     const uint32_t* found, Launch launch)
{
    const char* one = "offsets, prims and found must be 4-byte aligned";
    const Span s[4] = {{recs, n * in.bytes, 15u, true, in.name, nullptr}, {offsets, (n + 1u) * 4u, 3u, true, "offsets", one},
                       {capacity ? prims : nullptr, capacity * 4u, 3u, capacity != 0, "prims", one}, {found, n * 4u, 3u, false, "found", one}};
    OwnChecks own;      // prims without capacity takes part in no overlap, yet has to be aligned
    if (capacity == 0 && ((uintptr_t)prims & 3u)) own.aligned = one;
    if (capacity > ((size_t)-1 >> 2)) own.aligned = "capacity is more words than memory has";
    int fmt = 0;
    if (int rc = check_arrays(c, fn, n, in.noun, s, 4, own, true, &fmt)) return rc < 0 ? 0 : rc;
    const uint32_t cap = capacity > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)capacity;      // no 32-bit offset reaches further
    uint32_t raised = 0u;
    const int rc = run_query(c, fn, true, [&] {
        hipError_t e = c->d_list_scratch.reserve(ptd::list_scratch_words(0), c->stream);
        uint32_t* flag = (uint32_t*)c->d_list_scratch.p;
        if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(uint32_t), c->stream);
        if (e == hipSuccess) e = launch(fmt, cap, flag);
        if (e == hipSuccess) e = hipMemcpyAsync(&raised, flag, sizeof(raised), hipMemcpyDeviceToHost, c->stream);
        return e;
    });
    if (rc == 0 && raised) return refuse(c, fn, "the offsets do not fit this scene and these queries (a slice is shorter than its list, or lies outside prims): "
                                                "count again and rebuild them with pt_list_offsets");
    return rc;
}

PT_API int pt_query_overlap_lists(pt_ctx* c, const float* boxes, size_t n, const uint32_t* offsets, uint32_t* prims, size_t capacity, uint32_t* found)
{
    return lists_run(c, "pt_query_overlap_lists", kBoxes, boxes, n, offsets, prims, capacity, found, [&](int fmt, uint32_t cap, uint32_t* flag) {
        return ptd::launch_overlap_lists(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), (const float4*)boxes, (uint32_t)n, offsets, prims, cap, found, flag,
                                         c->list_phases, c->stream);
    });
}

PT_API int pt_query_triangles_lists(pt_ctx* c, const float* tris, size_t n, const uint32_t* offsets, uint32_t* prims, size_t capacity, uint32_t* found)
{
    return lists_run(c, "pt_query_triangles_lists", kQueryTriangles, tris, n, offsets, prims, capacity, found, [&](int fmt, uint32_t cap, uint32_t* flag) {
        return ptd::launch_triangles_lists(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), (const float4*)tris, (uint32_t)n, offsets, prims, cap, found, flag,
                                           c->list_phases, c->stream);
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
// The calls refuse what pt_query_overlap's and pt_query_overlap_lists' refuse, in the same order (overlap_prepare, lists_run); a record
// is 64 bytes.
PT_API int pt_query_overlap_oriented(pt_ctx* c, const float* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_overlap_oriented", kOrientedBoxes, kOverlapList, boxes, n, max_prims, prims, counts, nullptr, nullptr, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_overlap_oriented", true, [&] {
        return ptd::launch_query_oriented(fmt, device_scene(c), c->stack_entries, oriented_term(c), (const float4*)boxes, (uint32_t)n, max_prims, prims, counts, c->stream);
    });
}

PT_API int pt_query_overlap_oriented_any(pt_ctx* c, const float* boxes, size_t n, uint8_t* hit)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, "pt_query_overlap_oriented_any", kOrientedBoxes, kOverlapAny, boxes, n, 0u, nullptr, nullptr, hit, nullptr, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_overlap_oriented_any", true, [&] {
        return ptd::launch_query_oriented_any(fmt, device_scene(c), c->stack_entries, oriented_term(c), (const float4*)boxes, (uint32_t)n, hit, c->stream);
    });
}

static int oriented_visits_run(pt_ctx* c, const char* fn, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits, bool cross)
{
    int fmt = 0;
    if (int rc = overlap_prepare(c, fn, kOrientedBoxes, kOverlapTwin, boxes, n, 0u, nullptr, counts, nullptr, visits, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, fn, false, [&] {
        return ptd::launch_oriented_visits(fmt, device_scene(c), c->stack_entries, oriented_term(c), (const float4*)boxes, (uint32_t)n, counts, (uint2*)visits, cross, c->stream);
    });
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
    return lists_run(c, "pt_query_overlap_oriented_lists", kOrientedBoxes, boxes, n, offsets, prims, capacity, found, [&](int fmt, uint32_t cap, uint32_t* flag) {
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
PT_API int pt_query_segments(pt_ctx* c, const float* segments, size_t n, pt_segment_hit* out)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_segments", kSegments, segments, n, out, sizeof(pt_segment_hit), 15u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_segments", true, [&] {
        return ptd::launch_query_segments(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)segments, (uint32_t)n, (float4*)out, c->stream);
    });
}

PT_API int pt_debug_segments_visits(pt_ctx* c, const float* segments, size_t n, pt_segment_hit* out, uint32_t* visits, uint32_t flags)
{
    if (c && flags > ptd::kSegmentNoAxes) return fail(c, "pt_debug_segments_visits: flags must be 0 or 1");
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_debug_segments_visits", kSegments, segments, n, out, sizeof(pt_segment_hit), 15u, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_segments_visits", false, [&] {
        return ptd::launch_segments_visits(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)segments, (uint32_t)n, (float4*)out, (uint2*)visits, flags,
                                           c->stream);
    });
}

// ---- triangle to mesh distance ----------------------------------------------------------------------------------------------------
// a query is 48 bytes and so is a record
PT_API int pt_query_triangle_distance(pt_ctx* c, const float* tris, size_t n, pt_triangle_distance_hit* out)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_triangle_distance", kTriangles, tris, n, out, sizeof(pt_triangle_distance_hit), 15u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_triangle_distance", true, [&] {
        return ptd::launch_query_triangle_distance(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)tris, (uint32_t)n, (float4*)out, c->stream);
    });
}

PT_API int pt_debug_triangle_distance_visits(pt_ctx* c, const float* tris, size_t n, pt_triangle_distance_hit* out, uint32_t* visits, uint32_t flags)
{
    if (c && flags > ptd::kTriDistNoPlane) return fail(c, "pt_debug_triangle_distance_visits: flags must be 0 or 1");
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_debug_triangle_distance_visits", kTriangles, tris, n, out, sizeof(pt_triangle_distance_hit), 15u, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_triangle_distance_visits", false, [&] {
        return ptd::launch_triangle_distance_visits(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), (const float4*)tris, (uint32_t)n, (float4*)out, (uint2*)visits,
                                                    flags, c->stream);
    });
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

// One array of a posed-mesh call beside the poses: bytes per pose, the alignment mask, whether the call cannot do without it.
struct PoseArray { const void* p; size_t bytes_per_pose; uintptr_t align_mask; bool required; const char* name; };

// A posed-mesh call from its refusals (check_arrays, with the posed triangles counted after the poses and the query mesh asked for
// after the overlaps) to its end.  per_triangle: others[0] has its bytes per posed triangle (pt_pose_triangles' output); words: the
// call needs the per-pose scratch words.  launch(fmt).
template <typename Launch>
static int poses_run(pt_ctx* c, const char* fn, const float* poses, size_t P, const PoseArray* others, int n_others, bool per_triangle, bool words, Launch launch)
{
    const size_t T = c ? c->pose_mesh_tris : 0u;      // P < 2^31, T <= 2^20 where the products below are looked at
    Span s[3] = {{poses, P * 48u, 15u, true, "the poses", nullptr}};
    for (int k = 0; k < n_others; k++)
        s[k + 1] = {others[k].p, P * others[k].bytes_per_pose * (per_triangle ? T : 1u), others[k].align_mask, others[k].required, others[k].name, nullptr};
    OwnChecks own;
    if (P * T > 0x7FFFFFFFull) own.counted = "too many posed triangles (2^31 - 1 per call): split the poses";
    if (T == 0) own.disjoint = "no query mesh (pt_set_query_mesh first)";
    int fmt = 0;
    if (int rc = check_arrays(c, fn, P, "poses", s, n_others + 1, own, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, fn, true, [&] {
        hipError_t e = words ? c->d_pose_words.reserve(P, c->stream) : hipSuccess;
        return e == hipSuccess ? launch(fmt) : e;
    });
}

PT_API int pt_pose_triangles(pt_ctx* c, const float* poses, size_t P, float* tris_out)
{
    const PoseArray others[1] = {{tris_out, 48u, 15u, true, "tris_out"}};
    return poses_run(c, "pt_pose_triangles", poses, P, others, 1, true, false, [&](int) {
        return ptd::launch_pose_triangles(c->d_pose_mesh.p, c->pose_mesh_tris, (const float4*)poses, (uint32_t)P, (float4*)tris_out, c->stream);
    });
}

static int poses_any_run(pt_ctx* c, const char* fn, const float* poses, size_t P, uint8_t* hit, uint32_t* first, uint32_t flags)
{
    const PoseArray others[2] = {{hit, 1u, 0u, true, "hit"}, {first, 4u, 3u, false, "first"}};
    return poses_run(c, fn, poses, P, others, 2, false, true, [&](int fmt) {
        return ptd::launch_poses_any(fmt, device_scene(c), c->stack_entries, overlap_scene_term(c), c->d_pose_mesh.p, c->pose_mesh_tris, (const float4*)poses, (uint32_t)P,
                                     (uint32_t*)c->d_pose_words.p, hit, first, flags, c->stream);
    });
}

static int poses_distance_run(pt_ctx* c, const char* fn, const float* poses, size_t P, float max_radius, pt_pose_distance_hit* out, uint32_t flags)
{
    const PoseArray others[1] = {{out, sizeof(pt_pose_distance_hit), 15u, true, "out"}};
    return poses_run(c, fn, poses, P, others, 1, false, true, [&](int fmt) {
        return ptd::launch_poses_distance(fmt, device_scene(c), c->stack_entries, nearest_abs_term(c), c->d_pose_mesh.p, c->pose_mesh_tris, (const float4*)poses, (uint32_t)P,
                                          max_radius, c->d_pose_words.p, (float4*)out, flags, c->stream);
    });
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
PT_API int pt_query_sweep(pt_ctx* c, const float* sweeps, size_t n, pt_sweep_hit* hits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_sweep", kSweeps, sweeps, n, hits, sizeof(pt_sweep_hit), 15u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_sweep", true, [&] {
        return ptd::launch_query_sweep(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)sweeps, (uint32_t)n, (float4*)hits, c->stream);
    });
}

PT_API int pt_query_sweep_any(pt_ctx* c, const float* sweeps, size_t n, uint8_t* blocked)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_sweep_any", kSweeps, sweeps, n, blocked, 1u, 0u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_sweep_any", true, [&] {
        return ptd::launch_query_sweep_any(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)sweeps, (uint32_t)n, blocked, c->stream);
    });
}

PT_API int pt_debug_sweep_visits(pt_ctx* c, const float* sweeps, size_t n, pt_sweep_hit* hits, uint32_t* visits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_debug_sweep_visits", kSweeps, sweeps, n, hits, sizeof(pt_sweep_hit), 15u, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_sweep_visits", false, [&] {
        return ptd::launch_sweep_visits(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)sweeps, (uint32_t)n, (float4*)hits, (uint2*)visits, c->stream);
    });
}

// ---- swept capsules ---------------------------------------------------------------------------------------------------------------
// a cast is 48 bytes
PT_API int pt_query_capsule_cast(pt_ctx* c, const float* casts, size_t n, pt_capsule_cast_hit* hits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_capsule_cast", kCapsuleCasts, casts, n, hits, sizeof(pt_capsule_cast_hit), 15u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_capsule_cast", true, [&] {
        return ptd::launch_query_capsule_cast(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, (float4*)hits, c->stream);
    });
}

PT_API int pt_query_capsule_cast_any(pt_ctx* c, const float* casts, size_t n, uint8_t* blocked)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_capsule_cast_any", kCapsuleCasts, casts, n, blocked, 1u, 0u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_capsule_cast_any", true, [&] {
        return ptd::launch_query_capsule_cast_any(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, blocked, c->stream);
    });
}

PT_API int pt_debug_capsule_cast_visits(pt_ctx* c, const float* casts, size_t n, pt_capsule_cast_hit* hits, uint32_t* visits, uint32_t mode)
{
    if (c && mode > 1u) return fail(c, "pt_debug_capsule_cast_visits: mode is 0 (the product's walk) or 1 (without the plane axis)");
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_debug_capsule_cast_visits", kCapsuleCasts, casts, n, hits, sizeof(pt_capsule_cast_hit), 15u, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_capsule_cast_visits", false, [&] {
        return ptd::launch_capsule_cast_visits(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, (float4*)hits, (uint2*)visits,
                                               mode == 0u && ptd::kCapsulePlane, c->stream);
    });
}

// ---- swept oriented boxes ---------------------------------------------------------------------------------------------------------
// a cast is 80 bytes
PT_API int pt_query_box_cast(pt_ctx* c, const float* casts, size_t n, pt_box_cast_hit* hits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_box_cast", kBoxCasts, casts, n, hits, sizeof(pt_box_cast_hit), 15u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_box_cast", true, [&] {
        return ptd::launch_query_box_toi(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, (float4*)hits, c->stream);
    });
}

PT_API int pt_query_box_cast_any(pt_ctx* c, const float* casts, size_t n, uint8_t* blocked)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_box_cast_any", kBoxCasts, casts, n, blocked, 1u, 0u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_box_cast_any", true, [&] {
        return ptd::launch_query_box_toi_any(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, blocked, c->stream);
    });
}

PT_API int pt_debug_box_cast_visits(pt_ctx* c, const float* casts, size_t n, pt_box_cast_hit* hits, uint32_t* visits, uint32_t mode)
{
    if (c && mode > 1u) return fail(c, "pt_debug_box_cast_visits: mode is 0 (the walk with the extra axes) or 1 (the slab alone)");
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_debug_box_cast_visits", kBoxCasts, casts, n, hits, sizeof(pt_box_cast_hit), 15u, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_box_cast_visits", false, [&] {
        return ptd::launch_box_toi_visits(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, (float4*)hits, (uint2*)visits, mode == 0u,
                                          c->stream);
    });
}

// ---- translating-triangle casts ---------------------------------------------------------------------------------------------------
// a cast is 64 bytes; the visit counts of the twin have an alignment sentence of their own
PT_API int pt_query_triangle_cast(pt_ctx* c, const float* casts, size_t n, pt_triangle_cast_hit* hits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_triangle_cast", kTriangleCasts, casts, n, hits, sizeof(pt_triangle_cast_hit), 15u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_triangle_cast", true, [&] {
        return ptd::launch_query_triangle_cast(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, (float4*)hits, c->stream);
    });
}

PT_API int pt_query_triangle_cast_any(pt_ctx* c, const float* casts, size_t n, uint8_t* blocked)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_query_triangle_cast_any", kTriangleCasts, casts, n, blocked, 1u, 0u, nullptr, false, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_query_triangle_cast_any", true, [&] {
        return ptd::launch_query_triangle_cast_any(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, blocked, c->stream);
    });
}

PT_API int pt_debug_triangle_cast_visits(pt_ctx* c, const float* casts, size_t n, pt_triangle_cast_hit* hits, uint32_t* visits)
{
    int fmt = 0;
    if (int rc = records_prepare(c, "pt_debug_triangle_cast_visits", kTriangleCasts, casts, n, hits, sizeof(pt_triangle_cast_hit), 15u, visits, true, &fmt)) return rc < 0 ? 0 : rc;
    return run_query(c, "pt_debug_triangle_cast_visits", false, [&] {
        return ptd::launch_triangle_cast_visits(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), (const float4*)casts, (uint32_t)n, (float4*)hits, (uint2*)visits, c->stream);
    });
}

static int poses_cast_run(pt_ctx* c, const char* fn, const float* poses, const float* motions, size_t P, pt_triangle_cast_hit* out, uint32_t flags)
{
    const PoseArray others[2] = {{motions, 16u, 15u, true, "the motions"}, {out, sizeof(pt_triangle_cast_hit), 15u, true, "out"}};
    return poses_run(c, fn, poses, P, others, 2, false, true, [&](int fmt) {
        return ptd::launch_poses_cast(fmt, device_scene(c), c->stack_entries, query_scene_scale(c), c->d_pose_mesh.p, c->pose_mesh_tris, (const float4*)poses, (const float4*)motions,
                                      (uint32_t)P, c->d_pose_words.p, (float4*)out, flags, c->stream);
    });
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
// every refusal of the two calls before any device work, in an order of their own: the parameters and the disk pattern are judged
// between the alignment and the overlaps.  in: the points or the feature buffer, in_bytes per point.  On 0 the disk pattern is in
// c->d_ao_disk (enqueued on the context's stream) and *args is what the kernel gets.
static int ao_prepare(pt_ctx* c, const char* fn, const void* in, size_t in_bytes, size_t n, const float* disk, const pt_ao_params* ap, const uint32_t* visible, const float* ao,
                      int* fmt, ptd::AoArgs* args)
{
    if (!in || !disk || !ap || !visible) return refuse(c, fn, "null argument");
    if (n > 0x7FFFFFFFull) return refuse(c, fn, "too many points (2^31 - 1 per call)");
    if (((uintptr_t)in & 15u) || ((uintptr_t)visible & 3u) || ((uintptr_t)ao & 3u)) return refuse(c, fn, "the input must be 16-byte aligned, the outputs 4-byte aligned");
    if (ap->samples < 1u || ap->samples > ptd::kAoMaxSamples) return refuse(c, fn, "samples must be 1..256");
    if (!(ap->radius > 0.0f) || !std::isfinite(ap->radius)) return refuse(c, fn, "radius must be positive and finite");
    if (!(ap->bias >= 0.0f) || !std::isfinite(ap->bias)) return refuse(c, fn, "bias must be non-negative and finite");
    if (ap->total_samples < ap->samples) return refuse(c, fn, "total_samples must be at least samples");
    if (ap->reserved[0] || ap->reserved[1]) return refuse(c, fn, "reserved fields must be 0");
    for (uint32_t k = 0; k < ap->samples; k++) {
        const float x = disk[2u * k], y = disk[2u * k + 1u];
        if (!std::isfinite(x) || !std::isfinite(y) || !(x * x + y * y <= 1.0f))
            return refuse(c, fn, "disk point " + std::to_string(k) + " is outside the unit disk");
    }
    const Span s[3] = {{in, n * in_bytes, 15u, true, "the input", nullptr}, {visible, n * 4u, 3u, true, "visible", nullptr}, {ao, n * 4u, 3u, false, "ao", nullptr}};
    int k = 0, j = 0;
    if (first_overlap(s, 3, &k, &j)) return refuse(c, fn, std::string(s[k].name) + " overlaps " + s[j].name);
    if (int rc = query_node_format(c, fn, fmt)) return rc;
    *args = {ap->samples, ap->radius, ap->bias, ap->seed, ap->accumulate, ap->total_samples};
    return 0;
}

// the end of the two calls: the disk pattern goes up on the context's stream ahead of the launch
template <typename Launch>
static int ao_run(pt_ctx* c, const char* fn, const float* disk, uint32_t samples, Launch launch)
{
    return run_query(c, fn, true, [&] {
        hipError_t e = c->d_ao_disk.reserve(ptd::kAoMaxSamples, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_ao_disk.p, disk, (size_t)samples * sizeof(float2), hipMemcpyHostToDevice, c->stream);
        return e == hipSuccess ? launch() : e;
    });
}

PT_API int pt_ao_points(pt_ctx* c, const float* points, size_t n, const float* disk, const pt_ao_params* ap, uint32_t* visible, float* ao)
{
    if (!c) return fail(nullptr, "pt_ao_points: null context");
    if (n == 0) return 0;
    int fmt = 0;
    ptd::AoArgs args;
    if (int rc = ao_prepare(c, "pt_ao_points", points, 32u, n, disk, ap, visible, ao, &fmt, &args)) return rc;
    return ao_run(c, "pt_ao_points", disk, ap->samples, [&] {
        return ptd::launch_ao_points(fmt, device_scene(c), c->stack_entries, (const float4*)points, (uint32_t)n, c->d_ao_disk.p, args, visible, ao, c->stream);
    });
}

PT_API int pt_ao_image(pt_ctx* c, const pt_params* p, const float* normal_depth, const float* disk, const pt_ao_params* ap, uint32_t* visible, float* ao)
{
    if (!c) return fail(nullptr, "pt_ao_image: null context");
    if (!p) return fail(c, "pt_ao_image: null argument");
    const size_t n = (size_t)p->width * p->height;
    if (n == 0) return 0;
    int fmt = 0;
    ptd::AoArgs args;
    if (int rc = ao_prepare(c, "pt_ao_image", normal_depth, 16u, n, disk, ap, visible, ao, &fmt, &args)) return rc;
    const ptd::AoView view = {p->cameraEye, p->cameraU, p->cameraV, p->cameraW, p->width, p->height};
    return ao_run(c, "pt_ao_image", disk, ap->samples, [&] {
        return ptd::launch_ao_image(fmt, device_scene(c), c->stack_entries, view, (const float4*)normal_depth, c->d_ao_disk.p, args, visible, ao, c->stream);
    });
}
