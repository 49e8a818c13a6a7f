// sweep_device.h — the device functions the swept-sphere cast (sweep.hip) and the swept-capsule cast (capsule.hip) share: the three
// feature forms of include/acgpt.h's swept-sphere section, vertex sphere, edge cylinder and offset face.
// Evaluated as written (-ffp-contract=off); tests/sweep_ref.py mirrors them operation for operation.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// The three kinds of feature of the triangle's Minkowski sum with the sphere (include/acgpt.h states each operation).  Each lowers t
// to its own time of entry when it is a candidate; every compare is false on a NaN, so a NaN anywhere leaves t as it was.  Selects on
// one instruction stream: no feature branches.
__device__ __forceinline__ void sweep_vertex(const f3& m, const f3& d, float dd, float rr, float& t)
{
    const float t0 = -dot(m, d) / dd;
    const f3 mp = mk(m.x + d.x * t0, m.y + d.y * t0, m.z + d.z * t0);
    const float q = (rr - dot(mp, mp)) / dd;
    const float tv = t0 - sqrtf(q);
    if (q >= 0.0f && tv >= 0.0f && tv < t) t = tv;
}
__device__ __forceinline__ void sweep_edge(const f3& m, const f3& E, const f3& d, float rr, float& t)
{
    const float ee = dot(E, E), md = dot(m, E), nd = dot(d, E);
    const float km = md / ee, kd = nd / ee;
    const f3 mp = mk(m.x - E.x * km, m.y - E.y * km, m.z - E.z * km);
    const f3 dp = mk(d.x - E.x * kd, d.y - E.y * kd, d.z - E.z * kd);
    const float a = dot(dp, dp);
    const float t0 = -dot(mp, dp) / a;
    const f3 mq = mk(mp.x + dp.x * t0, mp.y + dp.y * t0, mp.z + dp.z * t0);
    const float q = (rr - dot(mq, mq)) / a;
    const float te = t0 - sqrtf(q);
    const float s = md + te * nd;
    if (q >= 0.0f && te >= 0.0f && s >= 0.0f && s <= ee && te < t) t = te;
}
__device__ __forceinline__ void sweep_face(const f3& m, const f3& e1, const f3& e2, const f3& d, float r, float& t)
{
    const f3 n = cross(e1, e2);
    const float nn = dot(n, n), s0 = dot(n, m);
    const float sr = s0 >= 0.0f ? r : -r;
    const float tf = (sr * sqrtf(nn) - s0) / dot(n, d);
    const f3 w = mk(m.x + d.x * tf, m.y + d.y * tf, m.z + d.z * tf);
    const float u = dot(cross(w, e2), n) / nn, v = dot(cross(e1, w), n) / nn;
    if (tf >= 0.0f && u >= 0.0f && v >= 0.0f && u + v <= 1.0f && tf < t) t = tf;
}

}  // namespace ptd
