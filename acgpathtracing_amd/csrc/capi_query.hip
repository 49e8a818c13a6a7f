// capi_query.hip — the entry points of include/acgpt.h that answer ray queries in device memory: pt_query_closest, pt_query_any.
// Host code only; the kernels are in query.hip.  The context and what the units share: context.h.
#include "context.h"
#include "query.h"

static_assert(sizeof(pt_hit) == 32, "pt_hit: a change of this layout bumps pt_abi_version");

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
    if (c->scene_serial == 0) return fail(c, f + "no scene (pt_set_scene first)");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, f + "hipSetDevice failed");
    // the node array the scene holds, as pt_render_features picks it: fp16 centre / half-extent nodes for the default variants, fp32
    // nodes for the fp32 ones; only a variant forced onto another format (pt_set_tuning) leaves neither and gets the fp32 nodes back
    *fmt = 0;
    if (c->bvh.hcnodes) *fmt = 11;
    else if (int rc = ensure_node_format(c, 0)) return rc;
    return 0;
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
