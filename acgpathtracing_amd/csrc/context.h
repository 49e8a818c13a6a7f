// context.h — what the host units of the C ABI share: the context, the group, error reporting, the owner of a device allocation.
// Host only (no kernel, not under pt_kernel_source_hash).  capi.hip: render core; capi_image.hip: the stages on a finished image;
// capi_query.hip: the device-resident ray queries and ambient occlusion; capi_test.hip: include/acgpt_test.h.
#pragma once
#include <hip/hip_runtime.h>
// RCCL: types only — librccl is loaded with dlopen by pt_create_multi, a single-GPU caller never touches it, and a box without
// the RCCL headers still builds the library (the handful of types and enumerators used below, with rccl.h's values)
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm* ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclFloat = 7 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
#endif
#include <string>
#include <thread>
#include <vector>

#include "../../include/acgpt.h"
#include "environment.h"
#include "lbvh_build.h"
#include "render_megakernel.h"
#include "render_small.h"
#include "winding.h"

#define PT_API extern "C" __attribute__((visibility("default")))

namespace ptd { struct DisplayState; struct FireflyState; struct BloomState; struct ConvergenceState; }

// One owner for a device allocation: grows on demand, never shrinks, freed with whatever holds it (a context: destroy_one).
// cap counts elements and reads 0 while there is no allocation, so a failed hipMalloc leaves it consistent.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // room for n elements; the old allocation goes only after `stream` has finished what may still use it
    hipError_t reserve(size_t n, hipStream_t stream)
    {
        if (n <= cap) return hipSuccess;
        if (p) { const hipError_t e = hipStreamSynchronize(stream); if (e != hipSuccess) return e; }
        release();
        const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
};
// a metered stage's state (run_metered, capi_image.hip): live counts and the record.  dirty: a call failed half way
template <typename State> struct StageBuf : DevBuf<State> { bool dirty = false; };

struct pt_multi;

struct pt_ctx {
    int device = 0;
    int n_cus = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // bracket the render kernel alone (k_finalize sits outside)
    ptd::LbvhResult bvh;
    DevBuf<ptd::DevMaterial> d_mats;          // pt_material repacked into two aligned 16-byte halves (pt_device.h)
    uint32_t n_mats = 0;
    DevBuf<float4> d_lights;                  // emissive triangles of the scene (light mode 1), 5 float4 each
    uint32_t n_lights = 0;
    float light_area = 0.0f;
    int light_mode = 0;                       // 0 the reference's estimator, 1 scene lights + MIS (pt_set_light_mode)
    int material_model = PT_MATERIALS_REFERENCE;   // pt_set_material_model: the context's, kept across scene changes
    DevBuf<float> d_alpha;                    // GGX alpha per material (the GGX kernels' table, pt_microfacet.h), beside d_mats
    int math_mode = PT_MATH_FAST;             // arithmetic of the shading code (pt_set_math_mode): the reference's own build uses nvcc --use_fast_math
    uint32_t stack_entries = 8;
    int blocks_per_cu = 0;        // from the occupancy query for the current stack size
    int tune_blocks_per_cu = 0;   // user override
    int build_mode = 2;           // 0 Karras LBVH, 1 PLOC over the Morton order, 2 PLOC + insertion-based optimisation of small trees (the default)
    int variant = ptd::kDefaultVariant;   // render kernel variant (render_megakernel.hip)
    bool variant_auto = true;             // until pt_set_tuning picks one: chosen per scene size in pt_set_scene
    DevBuf<uint32_t> d_queue;                 // 8 shard heads
    DevBuf<unsigned long long> d_counters;    // ptd::kCounterWords counters
    int rank = 0, world = 1;
    bool in_group = false;                    // a rank of a pt_create_multi group (rank 0 included)
    int chunks = 0;                           // sample chunks per pixel: 0 = automatic, else 1/2/4/8/16
    DevBuf<float4> d_frame_sums;              // [pixel][sub-frame] of a frame batch
    DevBuf<float> d_wave_scratch;             // fold slots of every wave of the grid
    DevBuf<uint32_t> d_stack_ovf;             // stack entries beyond a kernel's LDS cap
    // the small-scene path (render_small.hip): the 256-thread grid runs on a stream of its own beside the 1024-thread grid on `stream`;
    // small_fork / small_join order it behind the launch's memsets and ahead of ev1.  Created on the first launch that takes the path.
    hipStream_t small_stream = nullptr;
    hipEvent_t small_fork = nullptr, small_join = nullptr;
    size_t cu_lds_bytes = 0;                  // hipDeviceProp_t::maxSharedMemoryPerMultiProcessor: what the path's LDS budget is held against
    int small_mode = 0;                       // pt_debug_small_kernel: 0 automatic, 1 off, 2 / 3 the 1024- / 256-thread grid alone
    int small_last = 0;                       // what the last launch ran: 0 the variant table's kernel, 1 both grids, 2 / 3 one of them
    int small_force_half = 0;                 // pt_debug_small_shape: 1 keeps the fp16 two-copy shape where the fp32 shape would fit
    int small_shape_last = 0;                 // ptd::kSmallShape* of the last launch
    size_t scratch_limit = (size_t)1 << 30;   // a frame batch is cut into launches whose frame sums fit
    // division constants of the tile order, valid for (div_width, div_world_n): built and verified once per image width
    uint32_t div_width = 0; int div_world_n = 0; ptd::FastDiv div_cols = {0, 0, 0}, div_world = {0, 0, 0};
    DevBuf<uint2> d_row_spans;                // pixel classes per image row (capi.hip row_spans)
    std::vector<float> spans_key;             // what the spans on the device were computed from
    int pixel_classes = 1;                    // 0: off (pt_debug_pixel_classes)
    int queue_order = 1;                      // tile-strip rows dealt round robin over the queue shards (render_common.h queue_slot; pt_debug_queue_order)
    pt_multi* multi = nullptr;                // pt_create_multi: this context is rank 0 of a group (below)
    DevBuf<float4> d_group_accum;             // ... and every rank's private accumulation buffer (its own pixels, zero elsewhere)
    DevBuf<float4> d_denoise[2];              // pt_denoise's ping-pong {colour, variance} buffers
    ptd::EnvDevice env;                       // pt_set_environment's map and CDFs (w == 0: none); the context's, kept across scene changes
    StageBuf<ptd::DisplayState> d_display;            // pt_display_transform's counts and meter record
    StageBuf<ptd::FireflyState> d_firefly;            // pt_firefly_filter's counts and record
    StageBuf<ptd::BloomState> d_bloom;                // pt_bloom's counts and record ...
    DevBuf<float4> d_bloom_pyramid;                   // ... and its pyramid, all levels in one allocation
    StageBuf<ptd::ConvergenceState> d_convergence;    // pt_convergence_update's counts and record
    DevBuf<float2> d_ao_disk;                 // pt_ao_points / pt_ao_image: the caller's disk pattern of the last call (at most 256 pairs)
    DevBuf<unsigned long long> d_list_scratch;   // pt_list_offsets' tile sums and the list queries' mismatch flag (lists.h list_scratch_words); the
                                              // context's, not the scene's: not counted in device_bytes
    uint32_t list_phases = 3u;                // pt_debug_list_phases: fill | sort (ptd::kListPhaseAll), the product's
    DevBuf<float4> d_pose_mesh;               // pt_set_query_mesh: pose_mesh_tris records of three float4; the context's, kept across scene changes,
    uint32_t pose_mesh_tris = 0;              // not counted in device_bytes (pt_get_query_mesh reports it)
    DevBuf<unsigned long long> d_pose_words;  // the posed-mesh queries' word or key per pose (poses.h)
    DevBuf<uint8_t> d_tri_bsdf;              // bsdfType per triangle (caller's order): pt_temporal_blend's, built on its first call per scene
    // what pt_update_vertices keeps of the last pt_set_scene: host copies of everything but the vertices, and after the first update
    // the index buffer on the device (freed with the scene)
    bool scene_kept = false;
    size_t kept_n_verts = 0;
    std::vector<uint32_t> kept_idx, kept_mat_ids;
    std::vector<pt_material> kept_mats;
    DevBuf<uint32_t> d_idx;
    ptd::WindingTree winding;                 // pt_query_winding's far-field moments: built on its first call per scene or vertex update, kept across
                                              // material edits, freed with the scene (capi.hip free_scene, update_one); not counted in device_bytes
    double build_area = -1.0;                 // inner-node area sum over the root's at the last build (refit_tree_area; < 0: not taken yet)
    pt_stats stats;
    uint64_t scene_serial = 0;
    std::string err;
};

int fail(pt_ctx* c, const std::string& m);      // records m as the context's (and the process's) last error; returns 1
#define CK(c, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail((c), std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// ROCTx range (tracing): a no-op without the marker library (capi.hip)
struct Range {
    bool on;
    explicit Range(const char* name);
    ~Range();
};

// ---- multi-GPU group (pt_create_multi): rank 0 is the context the caller holds; it owns the others -----------------
// One context, stream and host thread per device; the tile partition of sutil/WorkDistribution.h:50-81 per rank; each rank
// accumulates its own pixels in a private full-size float4 buffer that is zero elsewhere; ONE ncclReduce(SUM) per launch
// brings them into the caller's accumulation buffer on rank 0 (every pixel has exactly one non-zero term, so the sum is
// that term bit for bit) and rank 0 applies make_color.  Replaces the dormant multi-GPU branch of the reference
// (sutil/WorkDistribution.h, sutil/CUDAOutputBuffer.h CUDA_P2P).
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
struct pt_multi {
    std::vector<pt_ctx*> ranks;          // ranks[0] = the context the caller holds
    uint32_t accum_w = 0, accum_h = 0;   // image shape the ranks' private buffers (d_group_accum) were last laid out for
    bool rehearsal = false;              // all ranks on ONE device (one-GPU box): a sum kernel stands in for RCCL
    RcclApi rccl;
    std::vector<ncclComm_t> comms;
    const void* cont_accum = nullptr;    // the caller's buffer and the frame index a straight continuation would pass next
    uint32_t cont_frame = 0, cont_w = 0, cont_h = 0;
    float reduce_ms = 0.0f;
    pt_stats group_stats;
};

// f(rank context, rank index) on every rank of a group, each on its own host thread (rank 0 on the caller's); the first
// failure's message becomes the group's.  A context that is no group: f(c, 0) on the caller's thread, its result as it is.
template <typename F>
int on_every_rank(pt_ctx* c, F f)
{
    pt_multi* m = c->multi;
    if (!m) return f(c, 0);
    const size_t n = m->ranks.size();
    std::vector<int> rc(n, 0);
    std::vector<std::thread> th;
    for (size_t i = 1; i < n; i++) th.emplace_back([&, i]() { rc[i] = f(m->ranks[i], (int)i); });
    rc[0] = f(m->ranks[0], 0);
    for (auto& t : th) t.join();
    for (size_t i = 0; i < n; i++)
        if (rc[i] != 0) return fail(c, "rank " + std::to_string(i) + " (device " + std::to_string(m->ranks[i]->device) + "): " + m->ranks[i]->err);
    return 0;
}

// do the byte spans [a, a + a_bytes) and [b, b + b_bytes) share a byte?
inline bool spans_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// helpers of capi.hip that the other units need
ptd::DeviceScene device_scene(pt_ctx* c);
int ensure_node_format(pt_ctx* c, int fmt);      // the node array of that format, present on the device (built on first use)
int ensure_dev_idx(pt_ctx* c);                   // the scene's index buffer on the device
bool row_spans(const pt_params* p, const float lo[3], const float hi[3], std::vector<uint32_t>& out);

// The round trip of the ray queries and the debug entry points: upload in_bytes, launch(d_in, d_a, d_b) on the context's stream,
// download the one or two outputs (bytes_b == 0: no second one, d_b is null).  fn: the entry point's name.
template <typename F>
int device_round_trip(pt_ctx* c, const char* fn, const void* in, size_t in_bytes, void* out_a, size_t bytes_a, void* out_b, size_t bytes_b, F launch)
{
    DevBuf<uint8_t> d_in, d_a, d_b;
    hipError_t e = d_in.reserve(in_bytes, c->stream);
    if (e == hipSuccess) e = d_a.reserve(bytes_a, c->stream);
    if (e == hipSuccess) e = d_b.reserve(bytes_b, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in.p, in, in_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch((void*)d_in.p, (void*)d_a.p, (void*)d_b.p);
    if (e == hipSuccess) e = hipMemcpyAsync(out_a, d_a.p, bytes_a, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && bytes_b) e = hipMemcpyAsync(out_b, d_b.p, bytes_b, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, std::string(fn) + ": " + hipGetErrorString(e));
    return 0;
}
