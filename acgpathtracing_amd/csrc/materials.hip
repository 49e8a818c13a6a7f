// materials.hip — the kernels behind pt_update_materials (include/acgpt.h): a new material assignment for a built tree.
//
//   k_mt_slots   per leaf slot: its triangle (the record's prim field) gets its new id in the record and, tagged, in the shade record;
//                and, when asked, slot_of[prim] = slot for k_mt_gather
//   k_mt_gather  per emissive triangle, in the caller's triangle order: v0, e1, e2 of its record, for the host's light list
//
// The tag is lbvh_build.hip k_tag_shade's expression, restated; tests/test_gpu_materials.py pins every bit against a fresh build.
#include "materials.h"
#include "pt_device.h"
#include <vector>

namespace ptd {

__global__ void __launch_bounds__(256)
k_mt_slots(TriRecord* __restrict__ tris, float4* __restrict__ shade, uint32_t n, const uint32_t* __restrict__ ids,
           const DevMaterial* __restrict__ mats, uint32_t* __restrict__ slot_of)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 r2 = tris[i].r2;
    const uint32_t prim = __float_as_uint(r2.y);
    if (prim >= n) return;      // a permutation of 0..n-1 by construction
    const uint32_t id = ids ? ids[prim] : __float_as_uint(r2.z);
    tris[i].r2 = make_float4(r2.x, r2.y, __uint_as_float(id), r2.w);
    // k_tag_shade: bsdfType in the upper byte, and whether the emission has a non-zero component (a NaN component counts)
    const float4 m1 = mats[id].ke_bsdf;
    const bool has_ke = !(m1.x == 0.0f && m1.y == 0.0f && m1.z == 0.0f);
    shade[i].w = __uint_as_float(id | ((__float_as_uint(m1.w) & 3u) << kShadeBsdfShift) | (has_ke ? kShadeHasKe : 0u));
    if (slot_of) slot_of[prim] = i;
}

__global__ void __launch_bounds__(256)
k_mt_gather(const TriRecord* __restrict__ tris, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ prims, uint32_t n_prims,
            uint32_t n, float* __restrict__ edges)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_prims) return;
    const uint32_t prim = prims[j];
    if (prim >= n) return;
    const TriRecord r = tris[slot_of[prim]];
    float* e = edges + 9 * (size_t)j;
    e[0] = r.r0.x; e[1] = r.r0.y; e[2] = r.r0.z;        // v0
    e[3] = r.r0.w; e[4] = r.r1.x; e[5] = r.r1.y;        // e1 = v1 - v0
    e[6] = r.r1.z; e[7] = r.r1.w; e[8] = r.r2.x;        // e2 = v2 - v0
}

#define MTCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string("materials: ") + #x + ": " + hipGetErrorString(e_); return false; } } while (0)

namespace {

// scratch of one call, released on every exit path
struct MtScratch {
    std::vector<void*> ptrs;
    template <typename T> hipError_t alloc(T** p, size_t bytes)
    {
        hipError_t e = hipMalloc((void**)p, bytes ? bytes : 4);
        if (e == hipSuccess) ptrs.push_back((void*)*p);
        return e;
    }
    ~MtScratch() { for (void* p : ptrs) (void)hipFree(p); }
};

template <typename T> void release(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

}  // namespace

bool update_materials(LbvhResult& r, const DevMaterial* d_mats, const uint32_t* h_ids, const std::vector<uint32_t>& light_prims,
                      std::vector<float>& edges, hipStream_t stream, std::string& err)
{
    edges.assign(light_prims.size() * 9, 0.0f);
    // the records' copies: their material words are the old ones
    release(r.wrecs); release(r.srecs);
    r.n_wrecs = 0; r.n_wnodes = 0; r.wide_depth = 0; r.wide_ms = 0.0f; r.n_srecs = 0;
    if (r.n_tris == 0) return true;
    if (!r.tris || !r.shade || !d_mats) { err = "materials: the scene holds no triangle records or materials"; return false; }
    const uint32_t n = r.n_tris, n_lights = (uint32_t)light_prims.size();
    MtScratch sc;
    uint32_t *d_ids = nullptr, *d_slot_of = nullptr, *d_prims = nullptr;
    float* d_edges = nullptr;
    if (h_ids) {
        MTCK(sc.alloc(&d_ids, (size_t)n * 4));
        MTCK(hipMemcpyAsync(d_ids, h_ids, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    }
    if (n_lights) {
        MTCK(sc.alloc(&d_slot_of, (size_t)n * 4));
        MTCK(hipMemsetAsync(d_slot_of, 0, (size_t)n * 4, stream));       // every entry is written; a valid slot regardless
    }
    k_mt_slots<<<(n + 255u) / 256u, 256, 0, stream>>>(r.tris, r.shade, n, d_ids, d_mats, d_slot_of);
    MTCK(hipGetLastError());
    if (n_lights) {
        MTCK(sc.alloc(&d_prims, (size_t)n_lights * 4));
        MTCK(sc.alloc(&d_edges, (size_t)n_lights * 36));
        MTCK(hipMemcpyAsync(d_prims, light_prims.data(), (size_t)n_lights * 4, hipMemcpyHostToDevice, stream));
        k_mt_gather<<<(n_lights + 255u) / 256u, 256, 0, stream>>>(r.tris, d_slot_of, d_prims, n_lights, n, d_edges);
        MTCK(hipGetLastError());
        MTCK(hipMemcpyAsync(edges.data(), d_edges, (size_t)n_lights * 36, hipMemcpyDeviceToHost, stream));
    }
    MTCK(hipStreamSynchronize(stream));
    return true;
}

}  // namespace ptd
