// winding.h — generalised winding numbers on the scene's BVH: pt_query_winding (include/acgpt.h states the contract;
// tests/winding_ref.py is the NumPy statement of the moments and of the accept rule, operation for operation).  Kernels in
// winding.hip; they read the render kernels' headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "lbvh_build.h"
#include "pt_device.h"

namespace ptd {

// What a node's subtree looks like from far away, fp32: the area-weighted centroid p, the squared distance r2 from p to the farthest
// corner of the exact box of the vertices below the node, the area-weighted normal sum N and the area sum A.  32 bytes; the side
// array holds one per inner node in the scene's node numbering (pt_debug_read_winding copies it out as it is).
struct WindMoment { float px, py, pz, r2, nx, ny, nz, area; };
static_assert(sizeof(WindMoment) == 32, "pt_debug_read_winding's record");

// What the bottom-up pass carries per node: N, A, S = sum of A_t * c_t, and the exact box.
struct WindSums { float n[3], area, s[3], lo[3], hi[3]; };

// One triangle from its record (v0, e1, e2).  Built with -ffp-contract=off: every product and sum below rounds once, as written.
__host__ __device__ inline WindSums wind_triangle(const float v0[3], const float e1[3], const float e2[3])
{
    WindSums t;
    const float n2[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    t.area = 0.5f * sqrtf((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2]);
    for (int k = 0; k < 3; k++) {
        t.n[k] = 0.5f * n2[k];
        const float c = v0[k] + (e1[k] + e2[k]) / 3.0f;
        t.s[k] = t.area * c;
        const float b = v0[k] + e1[k], cc = v0[k] + e2[k];
        t.lo[k] = fminf(v0[k], fminf(b, cc));
        t.hi[k] = fmaxf(v0[k], fmaxf(b, cc));
    }
    return t;
}

// A node from its two children, child 0 first.
__host__ __device__ inline WindSums wind_combine(const WindSums& a, const WindSums& b)
{
    WindSums t;
    t.area = a.area + b.area;
    for (int k = 0; k < 3; k++) {
        t.n[k] = a.n[k] + b.n[k];
        t.s[k] = a.s[k] + b.s[k];
        t.lo[k] = fminf(a.lo[k], b.lo[k]);
        t.hi[k] = fmaxf(a.hi[k], b.hi[k]);
    }
    return t;
}

// The moment of a node from its sums: p = S / A (the box centre where A is 0), r2 to the farthest corner.
__host__ __device__ inline WindMoment wind_moment(const WindSums& t)
{
    float p[3], r2 = 0.0f, m[3];
    for (int k = 0; k < 3; k++) {
        p[k] = t.area == 0.0f ? 0.5f * (t.lo[k] + t.hi[k]) : t.s[k] / t.area;
        m[k] = fmaxf(p[k] - t.lo[k], t.hi[k] - p[k]);
    }
    r2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    return WindMoment{p[0], p[1], p[2], r2, t.n[0], t.n[1], t.n[2], t.area};
}

// What the walk reads: one 64-byte record per inner node holding both children — the child's moment without its area (the walk has
// no use for it) and the child reference in the freed word: an inner node's index, ~slot of a leaf, or kWindEmpty for the second
// child of a single-triangle scene's one node, which no walk may enter (every other walk skips it by its NaN box bound; this one
// tests no boxes).  A leaf child's seven floats are zero: leaves are always exact solid angles.
struct WindChild { float px, py, pz, r2, nx, ny, nz; int ref; };
struct WindNode { WindChild c[2]; };
static_assert(sizeof(WindNode) == 64, "one visit is one 64-byte record");
constexpr int kWindEmpty = (int)0x80000000u;      // ~slot of slot 2^31 - 1: a scene holds fewer than 2^26 triangles

// The side arrays of one scene.  root: the moment of node 0, handed to the walk as a kernel argument.
struct WindingTree {
    WindMoment* moments = nullptr;      // device, n_nodes
    WindNode*   walk = nullptr;         // device, n_nodes
    WindMoment  root = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t    n_nodes = 0;
    bool        built = false;
};
inline size_t winding_bytes(const WindingTree& w) { return w.built ? (size_t)w.n_nodes * (sizeof(WindMoment) + sizeof(WindNode)) : 0u; }

// Builds both arrays from the topology of whichever node array r holds and from its triangle records.  Everything is allocated into
// locals and published to `out` only after the stream has synchronised without an error: a failure leaves `out` as it was (not
// built) and frees what it had allocated.  r.n_tris >= 1.
bool build_winding(const LbvhResult& r, hipStream_t stream, WindingTree& out, std::string& err);
void free_winding(WindingTree& w);

// points: n float4 {x, y, z, unused}, 16-byte aligned; out: n floats.  Both DEVICE, n >= 1.  beta2 = beta * beta in float.  A scene
// without triangles passes n_tris = 0 and a tree that is not built.
hipError_t launch_query_winding(const WindingTree& w, const TriRecord* tris, uint32_t n_tris, uint32_t stack_entries, float beta2, const float4* points,
                                uint32_t n, float* out, hipStream_t stream);
// The same walk, and per point the dipoles it took and the triangles it evaluated (acgpt_test.h pt_debug_winding_visits).
hipError_t launch_winding_visits(const WindingTree& w, const TriRecord* tris, uint32_t n_tris, uint32_t stack_entries, float beta2, const float4* points,
                                 uint32_t n, float* out, uint2* visits, hipStream_t stream);

}  // namespace ptd
