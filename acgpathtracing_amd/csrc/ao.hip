// ao.hip — the kernel behind pt_ao_points and pt_ao_image (include/acgpt.h).
//
//   k_ao<FMT, IMAGE>   one point per lane: K rays over the hemisphere of its normal, generated, traced with the any-hit walk and counted
//                      in the lane; 4 or 8 bytes out per point.  No ray ever reaches memory.
//
// FMT 11 walks the fp16 centre / half-extent nodes (traverse_hc_any, traverse_hc.h), FMT 0 the fp32 nodes (traverse<true>, pt_device.h):
// the node array the scene holds.  IMAGE false: the point is a device record {P, N}, lane i of a one-dimensional grid is point i.
// IMAGE true: the point is pixel (x, y)'s first hit, P = eye + t * pixel_centre_dir, {N, t} = normal_depth[y * w + x]; a wave is an
// 8 x 8 pixel tile, so that its 64 origins are neighbours on screen and mostly on one surface.  256-lane workgroups, the LDS lane
// stack of query_launch.h (stack_entries * 64 words per wave).  The K disk points are the same for every lane: `disk[k]` with a
// wave-uniform k is a scalar load.  Lanes without a point and points that are no surface stay in the wave, inactive; a wave without
// any surface traces nothing.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: every expression is evaluated as written, and tests/ao_ref.py mirrors it operation for operation.
#include "ao.h"
#include "image_common.h"
#include "query_launch.h"
#include "traverse_hc.h"

namespace ptd {

__device__ __forceinline__ bool finite3(const f3& v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }

template <int FMT, bool IMAGE>
__global__ void __launch_bounds__(256)
k_ao(const DeviceScene sc, uint32_t stack_entries, const float4* __restrict__ src, uint32_t n, const AoView view, uint32_t tiles_x,
     const float2* __restrict__ disk, const AoArgs a, uint32_t* __restrict__ visible, float* __restrict__ ao)
{
    const LaneStack st = lane_stack(stack_entries);

    // ---- the lane's point -------------------------------------------------------------------------------------------------------
    uint32_t i;
    bool have;
    f3 P = mk(0.0f), N = mk(0.0f, 0.0f, 1.0f);
    bool surface = false;
    if (IMAGE) {
        const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;      // w * h <= 2^31 - 1: no product below wraps
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
        have = x < view.w && y < view.h;
        i = y * view.w + x;
        if (have) {
            const float4 nd = src[i];
            const f3 dir = pixel_centre_dir(x, y, view.w, view.h, view.U, view.V, view.W);      // the ray k_dn_features traced (denoise.hip)
            P = mk(view.eye) + nd.w * dir;
            N = mk(nd.x, nd.y, nd.z);
            surface = !(nd.w < 0.0f);
        }
    } else {
        i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
        have = i < n;
        if (have) {
            const float4 p = src[2ull * i], q = src[2ull * i + 1ull];
            P = mk(p.x, p.y, p.z);
            N = mk(q.x, q.y, q.z);
            surface = true;
        }
    }
    surface = surface && finite3(P) && finite3(N) && !(N.x == 0.0f && N.y == 0.0f && N.z == 0.0f);

    uint32_t count = a.samples;      // no surface: fully open
    if (__ballot(surface) != 0ull) {
        // ---- rotation of the disk pattern: the rational point of the unit circle at parameter a in [0, 1), then quarter turns ------
        const uint32_t hsh = tea4(i, a.seed);
        const float ra = (float)(hsh & 0xFFFFu) * 0x1p-16f;
        const float a2 = ra * ra, den = 1.0f + a2;
        float c = (1.0f - a2) / den, s = (ra + ra) / den;
        const uint32_t q = (hsh >> 16) & 3u;
        const float c0 = c, s0 = s;
        if (q == 1u) { c = -s0; s = c0; }
        else if (q == 2u) { c = -c0; s = -s0; }
        else if (q == 3u) { c = s0; s = -c0; }
        // ---- frame (Duff et al. 2017) and origin ------------------------------------------------------------------------------------
        const float sg = copysignf(1.0f, N.z);
        const float A = -1.0f / (sg + N.z);
        const float B = N.x * N.y * A;
        const f3 T = mk(1.0f + sg * N.x * N.x * A, sg * B, -sg * N.x);
        const f3 S = mk(B, sg + N.y * N.y * A, -N.y);
        const f3 o = P + a.bias * N;
        const bool origin_ok = surface && finite3(o);
        count = 0u;
        for (uint32_t k = 0; k < a.samples; k++) {
            const float2 p = disk[k];
            const float xr = c * p.x - s * p.y, yr = s * p.x + c * p.y;
            const float z = sqrtf(fmaxf(0.0f, (1.0f - xr * xr) - yr * yr));
            const f3 d = (xr * T + yr * S) + z * N;
            const bool ok = origin_ok && finite3(d);      // pt_query_any's miss before any traversal; radius > 0 = tmin
            bool found;
            if (FMT == 11) found = traverse_hc_any(sc, st, ok, o, d, 0.0f, a.radius);
            else { HitRec hit; found = traverse<true>(sc, st, ok, o, d, 0.0f, a.radius, hit); }
            count += found ? 0u : 1u;
        }
    }
    if (!have) return;
    const uint32_t v = a.accumulate ? visible[i] + count : count;
    visible[i] = v;
    if (ao) ao[i] = (float)v / (float)a.total_samples;
}

hipError_t launch_ao_points(int fmt, const DeviceScene& sc, uint32_t stack_entries, const float4* points, uint32_t n, const float2* disk, const AoArgs& args,
                            uint32_t* visible, float* ao, hipStream_t stream)
{
    const AoView none = {};
    const uint32_t blocks = (n + 255u) / 256u;
    if (fmt == 11) return launch_lane_stack_blocks(k_ao<11, false>, stack_entries, blocks, stream, sc, stack_entries, points, n, none, 0u, disk, args, visible, ao);
    return launch_lane_stack_blocks(k_ao<0, false>, stack_entries, blocks, stream, sc, stack_entries, points, n, none, 0u, disk, args, visible, ao);
}

hipError_t launch_ao_image(int fmt, const DeviceScene& sc, uint32_t stack_entries, const AoView& view, const float4* normal_depth, const float2* disk,
                           const AoArgs& args, uint32_t* visible, float* ao, hipStream_t stream)
{
    const uint32_t tiles_x = (view.w + 7u) / 8u, tiles_y = (view.h + 7u) / 8u;      // w * h <= 2^31 - 1: at most 2^28 + ... tiles
    const uint32_t blocks = (uint32_t)(((uint64_t)tiles_x * tiles_y + 3u) / 4u);
    const uint32_t n = view.w * view.h;
    if (fmt == 11) return launch_lane_stack_blocks(k_ao<11, true>, stack_entries, blocks, stream, sc, stack_entries, normal_depth, n, view, tiles_x, disk, args, visible, ao);
    return launch_lane_stack_blocks(k_ao<0, true>, stack_entries, blocks, stream, sc, stack_entries, normal_depth, n, view, tiles_x, disk, args, visible, ao);
}

}  // namespace ptd
