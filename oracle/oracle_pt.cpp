/*
 * oracle_pt.cpp — CPU restatement of the reference's per-pixel path-trace launch.
 *
 * TEST INFRASTRUCTURE, NOT PRODUCT.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load this library, and only as the checker /
 * the timed CPU baseline.  Nothing under acgpathtracing_amd/ links or calls it.
 *
 * What is restated, and from where (all paths relative to /root/reference):
 *   tea<4>, lcg, rnd                    cuda/random.h:31-46, 49-55, 64-67
 *   float3 algebra                      sutil/vec_math.h:378-570 (operation order kept:
 *                                       a/s = a*(1/s), normalize = v*(1/sqrt(dot)), ...)
 *   make_color / toSRGB / quantize      cuda/helpers.h:35-62
 *   refract                             cuda/helpers.h:107-137
 *   Camera::UVWFrame                    sutil/Camera.cpp:34-45
 *   __raygen__rg                        PathTracer_Optix/pathTracerPrograms.cu:707-816
 *   __closesthit__diffuse__ch           PathTracer_Optix/pathTracerPrograms.cu:866-1031
 *   __miss__ms                          PathTracer_Optix/pathTracerPrograms.cu:833-847
 *   OrthonormalBasis, *_sample_hemisphere, sampleGGX, fresnelSchlickConductor,
 *   FrDielectric, traceOcclusion        same file :54-85, :341-380, :455-476, :494-510,
 *                                       :534-559, :651-684
 *   StaticWorkDistribution              sutil/WorkDistribution.h:50-81
 *
 * PARITY PINNING.  cuda/random.h, cuda/helpers.h, sutil/vec_math.h, sutil/Camera.cpp
 * and PathTracer_Optix/TinyObjWrapper.cpp compile here from where they lie (recipe:
 * oracle/Makefile -> oracle/_ref/libref.so) and this restatement is checked against
 * them function by function (tests/test_oracle_golden.py, fixtures in tests/golden/).
 * pathTracerPrograms.cu itself needs <optix.h>, which this image does not have, so the
 * three OptiX programs are UNBUILDABLE here and the reference ships no test or golden
 * vector for them: for the raygen/closest-hit/miss glue, PARITY IS UNPINNED — it is a
 * line-by-line restatement with the citations above, nothing stronger.
 *
 * What the reference does NOT define and this file therefore defines (the reference
 * delegates it to OptiX's built-in triangle GAS, pathTracerPrograms.cu:600-613):
 *   ray/triangle test  tri_test() below: Moeller-Trumbore, two-sided, fused multiply-adds
 *                      exactly where written, one IEEE division; open interval (tmin,tmax).
 *   closest hit        smallest t over all triangles; equal t -> lowest triangle index.
 *   occlusion          any triangle hit inside (tmin,tmax) occludes.
 * The GPU kernels must reproduce exactly these three definitions bit for bit.
 *
 * Beyond the reference, opt-in and off by default (a scene without them computes what it did before they existed): light mode 1
 * (closesthit_scene_lights), an environment map (orc_scene_set_environment) and the microfacet material model
 * (orc_scene_set_material_model).  Their maths are tests/env_ref.py and tests/microfacet_ref.py, to which
 * tests/test_oracle_env_ggx.py pins these functions.
 *
 * Build: see oracle/Makefile.  -ffp-contract=off is REQUIRED (the only fused operations
 * are the explicit __builtin_fmaf calls).
 */
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <cmath>
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <thread>
#include <vector>
#include <algorithm>
#include <chrono>

#include "../include/acgpt.h"   /* POD layouts of the boundary only (no product code) */

#define ORC_API extern "C" __attribute__((visibility("default")))

namespace {

/* ---------------------------------------------------------------- float3 ---- */
struct f3 { float x, y, z; };
static inline f3 mk(float x, float y, float z) { f3 r = {x, y, z}; return r; }
static inline f3 mk(float s) { return mk(s, s, s); }
static inline f3 mk(const pt_float3& p) { return mk(p.x, p.y, p.z); }
static inline f3 operator-(const f3& a) { return mk(-a.x, -a.y, -a.z); }
static inline f3 operator+(const f3& a, const f3& b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline f3 operator-(const f3& a, const f3& b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline f3 operator*(const f3& a, const f3& b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline f3 operator*(const f3& a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
static inline f3 operator*(float s, const f3& a) { return mk(s * a.x, s * a.y, s * a.z); }
static inline f3 operator/(const f3& a, const f3& b) { return mk(a.x / b.x, a.y / b.y, a.z / b.z); }
/* vec_math.h:483-487: division by a scalar multiplies by the reciprocal */
static inline f3 operator/(const f3& a, float s) { float inv = 1.0f / s; return a * inv; }
static inline void operator+=(f3& a, const f3& b) { a.x += b.x; a.y += b.y; a.z += b.z; }
static inline void operator*=(f3& a, const f3& b) { a.x *= b.x; a.y *= b.y; a.z *= b.z; }
static inline void operator*=(f3& a, float s) { a.x *= s; a.y *= s; a.z *= s; }
/* vec_math.h:527-530 */
static inline float dot(const f3& a, const f3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
/* vec_math.h:533-536 */
static inline f3 cross(const f3& a, const f3& b)
{ return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
/* vec_math.h:539-542 */
static inline float length(const f3& v) { return sqrtf(dot(v, v)); }
/* vec_math.h:545-549 */
static inline f3 normalize(const f3& v) { float invLen = 1.0f / sqrtf(dot(v, v)); return v * invLen; }
/* vec_math.h:558-561 */
static inline f3 reflect(const f3& i, const f3& n) { return i - 2.0f * n * dot(n, i); }
/* vec_math.h:567-570 */
static inline f3 faceforward(const f3& n, const f3& i, const f3& nref) { return n * copysignf(1.0f, dot(i, nref)); }
/* vec_math.h:500-503 */
static inline f3 lerp(const f3& a, const f3& b, float t) { return a + t * (b - a); }
/* vec_math.h:119-122 */
static inline float clampf(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }

static const float kPIf = 3.14159265358979323846f;   /* M_PIf, vec_math.h:43-45 */

/* ------------------------------------------------------------------ PRNG ---- */
/* cuda/random.h:31-46 */
static inline uint32_t tea4(uint32_t val0, uint32_t val1)
{
    uint32_t v0 = val0, v1 = val1, s0 = 0;
    for (uint32_t n = 0; n < 4; n++) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}
/* cuda/random.h:49-55 */
static inline uint32_t lcg(uint32_t& prev)
{
    prev = 1664525u * prev + 1013904223u;
    return prev & 0x00FFFFFFu;
}
/* cuda/random.h:64-67 */
static inline float rnd(uint32_t& prev) { return (float)lcg(prev) / (float)0x01000000; }

/* ------------------------------------------------------------ make_color ---- */
/* cuda/helpers.h:35-44 */
static inline f3 toSRGB(const f3& c)
{
    float invGamma = 1.0f / 2.4f;
    f3 powed = mk(powf(c.x, invGamma), powf(c.y, invGamma), powf(c.z, invGamma));
    return mk(c.x < 0.0031308f ? 12.92f * c.x : 1.055f * powed.x - 0.055f,
              c.y < 0.0031308f ? 12.92f * c.y : 1.055f * powed.y - 0.055f,
              c.z < 0.0031308f ? 12.92f * c.z : 1.055f * powed.z - 0.055f);
}
/* cuda/helpers.h:51-56 */
static inline uint8_t quantizeUnsigned8Bits(float x)
{
    x = clampf(x, 0.0f, 1.0f);
    unsigned v = (unsigned)(x * 256.0f);
    return (uint8_t)(v < 255u ? v : 255u);
}
/* cuda/helpers.h:58-63 */
static inline void make_color(const f3& c, uint8_t out[4])
{
    f3 cl = mk(clampf(c.x, 0.0f, 1.0f), clampf(c.y, 0.0f, 1.0f), clampf(c.z, 0.0f, 1.0f));
    f3 srgb = toSRGB(cl);
    out[0] = quantizeUnsigned8Bits(srgb.x);
    out[1] = quantizeUnsigned8Bits(srgb.y);
    out[2] = quantizeUnsigned8Bits(srgb.z);
    out[3] = 255u;
}

/* --------------------------------------------------------------- refract ---- */
/* cuda/helpers.h:107-137 */
static inline bool refract(f3& r, const f3& i, const f3& n, float ior)
{
    f3 nn = n;
    float negNdotV = dot(i, nn);
    float eta;
    if (negNdotV > 0.0f) { eta = ior; nn = -n; negNdotV = -negNdotV; }
    else                 { eta = 1.f / ior; }
    const float k = 1.f - eta * eta * (1.f - negNdotV * negNdotV);
    if (k < 0.0f) { r = mk(0.f); return false; }
    r = normalize(eta * i - (eta * negNdotV + sqrtf(k)) * nn);
    return true;
}

/* ------------------------------------------------- sampling / BSDF pieces ---- */
/* pathTracerPrograms.cu:54-85 */
struct OrthonormalBasis {
    f3 m_tangent, m_binormal, m_normal;
    explicit OrthonormalBasis(const f3& normal)
    {
        m_normal = normal;
        if (fabsf(m_normal.x) > fabsf(m_normal.z)) {
            m_binormal.x = -m_normal.y; m_binormal.y = m_normal.x; m_binormal.z = 0;
        } else {
            m_binormal.x = 0; m_binormal.y = -m_normal.z; m_binormal.z = m_normal.y;
        }
        m_binormal = normalize(m_binormal);
        m_tangent = cross(m_binormal, m_normal);
    }
    void inverse_transform(f3& p) const { p = p.x * m_tangent + p.y * m_binormal + p.z * m_normal; }
};
/* pathTracerPrograms.cu:341-353 */
static inline void cosine_sample_hemisphere(float eta1, float eta2, f3& p)
{
    const float theta = acosf(sqrtf(eta1));
    const float phi = 2.0f * kPIf * eta2;
    p.x = sinf(theta) * cosf(phi);
    p.y = sinf(theta) * sinf(phi);
    p.z = cosf(theta);
}
/* pathTracerPrograms.cu:368-380 (theta is computed and unused there) */
static inline void uniform_sample_hemisphere(float u1, float u2, f3& wi)
{
    const float phi = 2.0f * kPIf * u2;
    wi.x = cosf(phi) * sqrtf(1 - u1 * u1);
    wi.y = sinf(phi) * sqrtf(1 - u1 * u1);
    wi.z = u1;
}
/* pathTracerPrograms.cu:455-476 (the clamp at :458 discards its result) */
static inline f3 sampleGGX(float u1, float u2, float roughness, const f3& N)
{
    float phi = 2.0f * kPIf * u1;
    float cosTheta = sqrtf((1.0f - u2) / (1.0f + (roughness * roughness - 1.0f) * u2));
    float sinTheta = sqrtf(1.0f - cosTheta * cosTheta);
    f3 H = mk(sinTheta * cosf(phi), sinTheta * sinf(phi), cosTheta);
    /* :470 `abs(N.z) < 0.999`: nvcc device code takes the float overload; the
       comparison is in double */
    f3 up = (double)fabsf(N.z) < 0.999 ? mk(0, 0, 1) : mk(1, 0, 0);
    f3 tangent = normalize(cross(up, N));
    f3 bitangent = cross(N, tangent);
    f3 sampleDir = H.x * tangent + H.y * bitangent + H.z * N;
    return normalize(sampleDir);
}
/* pathTracerPrograms.cu:494-510 */
static inline f3 fresnelSchlickConductor(float cosTheta, f3 eta, f3 k)
{
    f3 eta2 = eta * eta;
    f3 k2 = k * k;
    f3 c2 = mk(cosTheta * cosTheta);
    f3 t1 = eta2 - k2 - c2;
    f3 a2plusb2 = mk(sqrtf(t1.x * t1.x + 4 * eta2.x * k2.x),
                     sqrtf(t1.y * t1.y + 4 * eta2.y * k2.y),
                     sqrtf(t1.z * t1.z + 4 * eta2.z * k2.z));
    f3 t2 = a2plusb2 + c2;
    f3 Rs = (t2 - 2 * eta * cosTheta + c2) / (t2 + 2 * eta * cosTheta + c2);
    f3 Rp = Rs * (t2 - 2 * eta * cosTheta + mk(1)) / (t2 + 2 * eta * cosTheta + mk(1));
    return (Rs + Rp) * 0.5f;
}
/* pathTracerPrograms.cu:534-559 */
static inline float FrDielectric(float cosThetaI, float etaI, float etaT)
{
    cosThetaI = clampf(cosThetaI, -1.0f, 1.0f);
    bool entering = cosThetaI > 0.0f;
    if (!entering) { float t = etaI; etaI = etaT; etaT = t; cosThetaI = fabsf(cosThetaI); }
    float sinThetaI = sqrtf(fmaxf(0.0f, 1.0f - cosThetaI * cosThetaI));
    float sinThetaT = etaI / etaT * sinThetaI;
    if (sinThetaT >= 1.0f) return 1.0f;
    float cosThetaT = sqrtf(fmaxf(0.0f, 1.0f - sinThetaT * sinThetaT));
    float rParl = ((etaT * cosThetaI) - (etaI * cosThetaT)) / ((etaT * cosThetaI) + (etaI * cosThetaT));
    float rPerp = ((etaI * cosThetaI) - (etaT * cosThetaT)) / ((etaI * cosThetaI) + (etaT * cosThetaT));
    return (rParl * rParl + rPerp * rPerp) / 2.0f;
}
/* pathTracerPrograms.cu:256-264 */
static inline float safeDivide(float a, float b) { return b == 0.0f ? 0.0f : a / b; }
static inline f3 safeDivide(f3 a, float b) { return mk(safeDivide(a.x, b), safeDivide(a.y, b), safeDivide(a.z, b)); }

/* ------------------------------------------------- ray / triangle (OURS) ---- */
static inline float dot_fma(const f3& a, const f3& b)
{ return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
static inline f3 cross_fma(const f3& a, const f3& b)
{
    return mk(__builtin_fmaf(a.y, b.z, -(a.z * b.y)),
              __builtin_fmaf(a.z, b.x, -(a.x * b.z)),
              __builtin_fmaf(a.x, b.y, -(a.y * b.x)));
}
/* The triangle test every intersector in this repository must reproduce bit for bit. */
static inline bool tri_test(const f3& o, const f3& d, const f3& v0, const f3& e1, const f3& e2,
                            float tmin, float tmax, float& t_out)
{
    f3 p = cross_fma(d, e2);
    float det = dot_fma(e1, p);
    f3 s = o - v0;
    float U = dot_fma(s, p);
    f3 q = cross_fma(s, e1);
    float V = dot_fma(d, q);
    float T = dot_fma(e2, q);
    if (det < 0.0f) { det = -det; U = -U; V = -V; T = -T; }
    if (!(det > 0.0f)) return false;
    if (U < 0.0f || V < 0.0f || U + V > det) return false;
    float t = T / det;
    if (!(t > tmin && t < tmax)) return false;
    t_out = t;
    return true;
}

/* ------------------------------------------------------------------ scene ---- */
struct Tri { f3 v0, e1, e2; };
struct BNode { float lo[3], hi[3]; uint32_t left, right, first, count; };  /* count>0: leaf */

/* One emissive triangle of the scene (light mode 1, see closesthit_scene_lights): geometry, unit normal, emission, and
 * the running sum of the areas up to and including this one (the selection CDF). */
struct LightTri { f3 v0, e1, e2, n, Ke; float area, cdf; };

/* An environment map (NOT the reference: pt_set_environment, include/acgpt.h).  texels: {r, g, b, weight} with the scale applied, row 0
 * the +Y pole; marg[h] / cond[h][w]: the normalised inclusive scans of the row totals and of each row's weights; w == 0: no map. */
struct EnvMapH {
    std::vector<float> texels, marg, cond;
    uint32_t w = 0, h = 0;
    float total = 0.0f, pdf_scale = 0.0f;
};

struct Scene {
    std::vector<Tri> tris;
    std::vector<uint32_t> mat_ids;
    std::vector<pt_material> mats;
    std::vector<BNode> nodes;
    std::vector<uint32_t> order;   /* leaf triangle order */
    std::vector<LightTri> lights;  /* emissive triangles in triangle order */
    int light_mode;                /* 0 = the reference's estimator (hard-coded rectangle, double counting); 1 = scene lights + MIS */
    EnvMapH env;                   /* orc_scene_set_environment */
    float p_env;                   /* light mode 1: probability that a light sample goes to the map (0: no map or a black one) */
    int material_model;            /* light mode 1: 0 = the reference's materials, 1 = GGX metal and glass (orc_scene_set_material_model) */
    std::vector<float> alpha;      /* GGX alpha per material: roughness clamped to [0, 1], NaN and negative values as 0 */
};

static void tri_bounds(const Tri& t, float lo[3], float hi[3])
{
    f3 v1 = t.v0 + t.e1, v2 = t.v0 + t.e2;   /* slightly off the original v1/v2: padded below */
    const float* a = &t.v0.x; const float* b = &v1.x; const float* c = &v2.x;
    for (int k = 0; k < 3; k++) {
        lo[k] = fminf(a[k], fminf(b[k], c[k]));
        hi[k] = fmaxf(a[k], fmaxf(b[k], c[k]));
        float pad = 1e-5f * fmaxf(1.0f, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
        lo[k] -= pad; hi[k] += pad;
    }
}

/* Median-split BVH (its own builder: results do not depend on the tree as long as the
 * box test is conservative, which the padded boxes + widened slab test guarantee; the
 * tests check it against brute force). */
static uint32_t build_rec(Scene& sc, std::vector<float>& lo, std::vector<float>& hi,
                          std::vector<f3>& cen, uint32_t first, uint32_t count)
{
    uint32_t me = (uint32_t)sc.nodes.size();
    sc.nodes.push_back(BNode());
    float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = first; i < first + count; i++) {
        uint32_t t = sc.order[i];
        const float* c = &cen[t].x;
        for (int k = 0; k < 3; k++) {
            blo[k] = fminf(blo[k], lo[3 * t + k]); bhi[k] = fmaxf(bhi[k], hi[3 * t + k]);
            clo[k] = fminf(clo[k], c[k]); chi[k] = fmaxf(chi[k], c[k]);
        }
    }
    BNode n; memcpy(n.lo, blo, 12); memcpy(n.hi, bhi, 12);
    n.left = n.right = 0; n.first = first; n.count = 0;
    int axis = 0; float ext = chi[0] - clo[0];
    for (int k = 1; k < 3; k++) if (chi[k] - clo[k] > ext) { ext = chi[k] - clo[k]; axis = k; }
    if (count <= 4 || !(ext > 0.0f)) { n.count = count; sc.nodes[me] = n; return me; }
    uint32_t mid = first + count / 2;
    std::nth_element(sc.order.begin() + first, sc.order.begin() + mid, sc.order.begin() + first + count,
                     [&](uint32_t a, uint32_t b) {
                         float ca = (&cen[a].x)[axis], cb = (&cen[b].x)[axis];
                         return ca < cb || (ca == cb && a < b);
                     });
    n.left = build_rec(sc, lo, hi, cen, first, mid - first);
    n.right = build_rec(sc, lo, hi, cen, mid, first + count - mid);
    sc.nodes[me] = n;
    return me;
}

static void build_bvh(Scene& sc)
{
    size_t n = sc.tris.size();
    std::vector<float> lo(3 * n), hi(3 * n);
    std::vector<f3> cen(n);
    sc.order.resize(n);
    for (size_t i = 0; i < n; i++) {
        tri_bounds(sc.tris[i], &lo[3 * i], &hi[3 * i]);
        cen[i] = mk(0.5f * (lo[3 * i] + hi[3 * i]), 0.5f * (lo[3 * i + 1] + hi[3 * i + 1]), 0.5f * (lo[3 * i + 2] + hi[3 * i + 2]));
        sc.order[i] = (uint32_t)i;
    }
    sc.nodes.clear();
    if (n) build_rec(sc, lo, hi, cen, 0, (uint32_t)n);
}

/* Conservative slab test: far distance widened (Ize, "Robust BVH Ray Traversal", 2013);
 * NaNs from 0*inf are dropped by fminf/fmaxf, which only ever widens the interval. */
static inline bool box_test(const BNode& b, const f3& o, const f3& inv, float tmin, float tmax)
{
    float t0 = tmin, t1 = tmax;
    const float* oo = &o.x; const float* ii = &inv.x;
    for (int k = 0; k < 3; k++) {
        float a = (b.lo[k] - oo[k]) * ii[k];
        float c = (b.hi[k] - oo[k]) * ii[k];
        float near = fminf(a, c), far = fmaxf(a, c);
        far *= 1.0000004f;
        t0 = fmaxf(t0, near); t1 = fminf(t1, far);   /* fmaxf/fminf ignore a NaN operand */
    }
    return t0 <= t1;
}

struct Hit { float t; uint32_t prim; };

static inline void closest_brute(const Scene& sc, const f3& o, const f3& d, float tmin, float tmax, Hit& h)
{
    h.t = tmax; h.prim = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < sc.tris.size(); i++) {
        float t;
        /* strict '<' on ascending i keeps the lowest index among equal t */
        if (tri_test(o, d, sc.tris[i].v0, sc.tris[i].e1, sc.tris[i].e2, tmin, tmax, t) && t < h.t) { h.t = t; h.prim = i; }
    }
}

static inline void closest_bvh(const Scene& sc, const f3& o, const f3& d, float tmin, float tmax, Hit& h)
{
    h.t = tmax; h.prim = 0xFFFFFFFFu;
    if (sc.nodes.empty()) return;
    f3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    uint32_t stack[128]; int sp = 0; stack[sp++] = 0;
    while (sp) {
        const BNode& n = sc.nodes[stack[--sp]];
        /* widened: a triangle whose distance ties with the best so far must still be reached (its box entry
         * distance and its Moeller-Trumbore distance round independently) */
        if (!box_test(n, o, inv, tmin, h.t * 1.00002f)) continue;
        if (n.count) {
            for (uint32_t i = n.first; i < n.first + n.count; i++) {
                uint32_t p = sc.order[i]; float t;
                if (tri_test(o, d, sc.tris[p].v0, sc.tris[p].e1, sc.tris[p].e2, tmin, tmax, t)
                    && (t < h.t || (t == h.t && p < h.prim))) { h.t = t; h.prim = p; }
            }
        } else {
            stack[sp++] = n.right; stack[sp++] = n.left;
        }
    }
}

static inline bool any_brute(const Scene& sc, const f3& o, const f3& d, float tmin, float tmax)
{
    for (uint32_t i = 0; i < sc.tris.size(); i++) {
        float t;
        if (tri_test(o, d, sc.tris[i].v0, sc.tris[i].e1, sc.tris[i].e2, tmin, tmax, t)) return true;
    }
    return false;
}

static inline bool any_bvh(const Scene& sc, const f3& o, const f3& d, float tmin, float tmax)
{
    if (sc.nodes.empty()) return false;
    f3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    uint32_t stack[128]; int sp = 0; stack[sp++] = 0;
    while (sp) {
        const BNode& n = sc.nodes[stack[--sp]];
        if (!box_test(n, o, inv, tmin, tmax)) continue;
        if (n.count) {
            for (uint32_t i = n.first; i < n.first + n.count; i++) {
                uint32_t p = sc.order[i]; float t;
                if (tri_test(o, d, sc.tris[p].v0, sc.tris[p].e1, sc.tris[p].e2, tmin, tmax, t)) return true;
            }
        } else {
            stack[sp++] = n.right; stack[sp++] = n.left;
        }
    }
    return false;
}

/* ------------------------------------------------------------- the launch ---- */
struct Counters { uint64_t radiance_rays, shadow_rays, paths; };

/* RadiancePayloadRayData, pathTracer.h:19-32 */
struct PRD {
    f3 attenuation; uint32_t randomSeed; int depth;
    f3 emissionColor, radiance, origin, direction; int done;
};

/* __closesthit__diffuse__ch, pathTracerPrograms.cu:866-1031 */
static inline void closesthit(const Scene& sc, const pt_params& params, int use_bvh,
                              const f3& ray_org, const f3& ray_dir, float t_hit, uint32_t prim_idx,
                              PRD& prd, Counters& cnt)
{
    const pt_material& rt = sc.mats[sc.mat_ids[prim_idx]];
    const Tri& tri = sc.tris[prim_idx];
    const bool useDirectLighting = params.useDirectLighting != 0;
    const float roughness = 0.2;                       /* :880 — the material's value is ignored */
    const float IOR = rt.ior;
    const int bsdfType = rt.bsdfType;
    const bool useImportanceSampling = params.useImportanceSampling != 0;

    /* :886-891; v1 - v0 and v2 - v0 are the stored edges (same single subtraction) */
    const f3 N_0 = normalize(cross(tri.e1, tri.e2));
    const f3 N = faceforward(N_0, -ray_dir, N_0);
    const f3 P = ray_org + t_hit * ray_dir;            /* :894 */

    if (prd.depth == 0) prd.emissionColor = mk(rt.emission);   /* :898-901 */
    else                prd.emissionColor = mk(0.0f);

    uint32_t seed = prd.randomSeed;
    const f3 Kd = mk(rt.diffuse);

    switch (bsdfType) {
    case PT_BSDF_DIFFUSE: {                            /* :907-930 */
        const float z1 = rnd(seed);
        const float z2 = rnd(seed);
        OrthonormalBasis onb(N);
        f3 w_in;
        if (useImportanceSampling) cosine_sample_hemisphere(z1, z2, w_in);
        else                       uniform_sample_hemisphere(z1, z2, w_in);
        onb.inverse_transform(w_in);
        prd.direction = w_in;
        prd.origin = P;
        prd.attenuation *= Kd;
        break;
    }
    case PT_BSDF_METALLIC: {                           /* :931-953 */
        const float z1 = rnd(seed);
        const float z2 = rnd(seed);
        f3 microfacetNormal = sampleGGX(z1, z2, roughness, N);
        f3 R = reflect(ray_dir, microfacetNormal);
        prd.direction = R;
        prd.origin = P + R * 1e-4f;
        f3 eta = mk((float)1.45, (float)0.7, (float)1.55);
        f3 k = mk((float)3.0, (float)2.2, (float)3.5);
        float cosTheta = fmaxf(dot(microfacetNormal, -ray_dir), 0.0f);
        f3 F = fresnelSchlickConductor(cosTheta, eta, k);
        f3 color = F * Kd;
        prd.attenuation *= color;
        break;
    }
    case PT_BSDF_REFRACTION: {                         /* :954-982 */
        f3 incidentRayDir = normalize(ray_dir);
        float cos_theta = dot(normalize(-ray_dir), N_0);
        float F = FrDielectric(cos_theta, 1.0f, IOR);
        if (rnd(seed) < F) {
            prd.direction = reflect(incidentRayDir, N_0);
        } else {
            f3 refractedDir;
            bool didRefract = refract(refractedDir, incidentRayDir, N_0, IOR);
            prd.direction = didRefract ? refractedDir : reflect(incidentRayDir, N_0);
        }
        prd.origin = P + prd.direction * 1e-3f;
        prd.attenuation *= Kd;
        break;
    }
    default: break;
    }

    const float z1 = rnd(seed);                        /* :985-987, drawn always */
    const float z2 = rnd(seed);
    prd.randomSeed = seed;

    if (length(mk(rt.emission)) > 0.0f) { prd.radiance = mk(rt.emission); prd.done = 1; }   /* :992-1000 */
    else                                { prd.radiance = mk(0.0f); prd.done = 0; }

    if (useDirectLighting && bsdfType != PT_BSDF_REFRACTION) {          /* :1003-1026 */
        const pt_area_light& light = params.areaLight;
        const f3 light_pos = mk(light.corner) + mk(light.v1) * z1 + mk(light.v2) * z2;
        const float Ldist = length(light_pos - P);
        const f3 L = normalize(light_pos - P);
        const float nDl = dot(N, L);
        const float LnDl = -dot(mk(light.normal), L);
        if (nDl > 0.0f && LnDl > 0.0f) {
            cnt.shadow_rays++;
            /* traceOcclusion :651-684: any hit occludes */
            const bool occluded = use_bvh ? any_bvh(sc, P, L, 0.01f, Ldist - 0.01f)
                                          : any_brute(sc, P, L, 0.01f, Ldist - 0.01f);
            if (!occluded) {
                const float A = length(cross(mk(light.v1), mk(light.v2)));
                float weight = nDl * LnDl * A / (kPIf * Ldist * Ldist);
                prd.radiance += mk(light.emission) * weight;
            }
        }
    }
}

/* ------------------------------------------------------- environment map (NOT the reference) ----
 * The maths of tests/env_ref.py (which tests/test_oracle_env_ggx.py pins these functions to); float32 operations in the order the
 * device kernels use at the IEEE level, so that a render can match theirs bit for bit. */
static const float kInv2PIf = 0.159154943091895336f, kInvPIf = 0.318309886183790672f;

/* env_ref.block_scan: 256 runs of ceil(n / 256) values summed in order, Hillis-Steele over the run sums, then each run's values added
 * in order to the sum of the runs before it; normalised by the total (a zero total: the uniform CDF (i + 1) / n).  Returns the total. */
static float env_block_scan(const float* vals, uint32_t n, float* out)
{
    const uint32_t T = 256, run = (n + T - 1) / T;
    float sums[256];
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t b = std::min(t * run, n), e = std::min(b + run, n);
        float s = 0.0f;
        for (uint32_t i = b; i < e; i++) s += vals[i];
        sums[t] = s;
    }
    for (uint32_t off = 1; off < T; off <<= 1) {
        float old[256];
        memcpy(old, sums, sizeof(old));
        for (uint32_t t = off; t < T; t++) sums[t] = old[t] + old[t - off];
    }
    const float total = sums[T - 1];
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t b = std::min(t * run, n), e = std::min(b + run, n);
        float acc = t ? sums[t - 1] : 0.0f;
        for (uint32_t i = b; i < e; i++) {
            acc += vals[i];
            out[i] = total > 0.0f ? acc / total : (float)(i + 1) / (float)n;
        }
    }
    return total;
}

/* texels times scale; weight = lum(rgb) * sin(pi (row + 0.5) / h), the sine in double rounded to float; the CDFs; pdf_scale =
 * w h / (2 pi^2 total) in double (0 for a black map) */
static void env_build(EnvMapH& E, const float* rgb, uint32_t w, uint32_t h, const float* scale3)
{
    const float sx = scale3 ? scale3[0] : 1.0f, sy = scale3 ? scale3[1] : 1.0f, sz = scale3 ? scale3[2] : 1.0f;
    E.w = w; E.h = h;
    E.texels.assign((size_t)w * h * 4, 0.0f);
    E.cond.assign((size_t)w * h, 0.0f);
    E.marg.assign(h, 0.0f);
    std::vector<float> weight(w), row_total(h);
    for (uint32_t r = 0; r < h; r++) {
        const float s = (float)sin(M_PI * ((double)r + 0.5) / (double)h);
        for (uint32_t c = 0; c < w; c++) {
            const size_t i = (size_t)r * w + c;
            float* t = &E.texels[4 * i];
            t[0] = rgb[3 * i] * sx; t[1] = rgb[3 * i + 1] * sy; t[2] = rgb[3 * i + 2] * sz;
            t[3] = (0.2126f * t[0] + 0.7152f * t[1] + 0.0722f * t[2]) * s;
            weight[c] = t[3];
        }
        row_total[r] = env_block_scan(weight.data(), w, &E.cond[(size_t)r * w]);
    }
    E.total = env_block_scan(row_total.data(), h, E.marg.data());
    E.pdf_scale = E.total > 0.0f ? (float)((double)w * (double)h / (2.0 * M_PI * M_PI * (double)E.total)) : 0.0f;
    if (!std::isfinite(E.pdf_scale)) E.pdf_scale = 0.0f;
}

/* u = 0.5 + atan2(d.x, -d.z) / (2 pi), v = acos(d.y) / pi; the texel that holds (u, v) */
static inline uint32_t env_texel(const EnvMapH& E, const f3& d)
{
    const float u = 0.5f + atan2f(d.x, -d.z) * kInv2PIf;
    const float v = acosf(clampf(d.y, -1.0f, 1.0f)) * kInvPIf;
    const int col = std::min(std::max((int)(u * (float)E.w), 0), (int)E.w - 1);
    const int row = std::min(std::max((int)(v * (float)E.h), 0), (int)E.h - 1);
    return (uint32_t)row * E.w + (uint32_t)col;
}
static inline f3 env_eval(const EnvMapH& E, const f3& d)
{
    if (E.w == 0) return mk(0.0f);
    const float* t = &E.texels[4 * (size_t)env_texel(E, d)];
    return mk(t[0], t[1], t[2]);
}
static inline float env_pdf_weight(float w, float sin_theta, float pdf_scale) { return sin_theta > 0.0f ? (w * pdf_scale) / sin_theta : 0.0f; }
/* solid-angle pdf of env_sample for d: weight * pdf_scale / sin(theta), sin(theta) = sqrt((1 - y)(1 + y)) */
static inline float env_pdf(const EnvMapH& E, const f3& d)
{
    if (E.w == 0 || !(E.pdf_scale > 0.0f)) return 0.0f;
    const float w = E.texels[4 * (size_t)env_texel(E, d) + 3];
    return env_pdf_weight(w, sqrtf(fmaxf(0.0f, (1.0f - d.y) * (1.0f + d.y))), E.pdf_scale);
}
/* the bin of x: the first k with cdf[k] > x (n - 1 if none), and where x lies inside it */
static inline uint32_t env_search(const float* cdf, uint32_t n, float x)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}
static inline float env_offset(const float* cdf, uint32_t k, float x)
{
    const float c0 = k ? cdf[k - 1] : 0.0f, c1 = cdf[k];
    const float f = c1 > c0 ? (x - c0) / (c1 - c0) : 0.5f;
    return fminf(fmaxf(f, 0.0f), 0.99999994f);
}
/* (u1, u2) -> a direction from the map's distribution: the row by u1, the column by u2, a linear offset inside each bin */
static inline bool env_sample(const EnvMapH& E, float u1, float u2, f3& dir, float& pdf, f3& Le)
{
    pdf = 0.0f; Le = mk(0.0f); dir = mk(0.0f, 1.0f, 0.0f);
    if (E.w == 0 || !(E.pdf_scale > 0.0f)) return false;
    const uint32_t row = env_search(E.marg.data(), E.h, u1);
    const float fv = env_offset(E.marg.data(), row, u1);
    const float* cdf = &E.cond[(size_t)row * E.w];
    const uint32_t col = env_search(cdf, E.w, u2);
    const float fu = env_offset(cdf, col, u2);
    const float u = ((float)col + fu) / (float)E.w, v = ((float)row + fv) / (float)E.h;
    float st = sinf(kPIf * v);
    const float ct = cosf(kPIf * v);
    const float ph = 2.0f * kPIf * (u - 0.5f);
    const float sp = sinf(ph), cp = cosf(ph);
    st = fmaxf(st, 0.0f);
    dir = mk(st * sp, ct, -(st * cp));
    const float* t = &E.texels[4 * ((size_t)row * E.w + col)];
    Le = mk(t[0], t[1], t[2]);
    pdf = env_pdf_weight(t[3], st, E.pdf_scale);
    return pdf > 0.0f;
}

/* ------------------------------------------------------ microfacet model (NOT the reference) ----
 * The maths of tests/microfacet_ref.py: isotropic GGX, Smith Lambda, height-correlated G2, Heitz 2018 visible-normal sampling, the
 * reference's conductor Fresnel and FrDielectric.  float32 in the device's operation order at the IEEE level. */
static const float kSmoothAlpha = 1e-3f;      /* alpha below this: the smooth BSDF (mirror / light mode 1's glass) */

static inline void onb_axes(const f3& n, f3& tg, f3& bn)
{
    const OrthonormalBasis onb(n);
    tg = onb.m_tangent; bn = onb.m_binormal;
}
static inline float ggx_lambda(float c, float a2)
{
    const float c2 = c * c;
    return 0.5f * (sqrtf(1.0f + a2 * ((1.0f - c2) / c2)) - 1.0f);
}
static inline float ggx_d(float ch, float a2)
{
    const float t = ch * ch * (a2 - 1.0f) + 1.0f;
    return a2 / (kPIf * t * t);
}
static inline f3 ggx_sample_vndf(const f3& ve, float alpha, float u1, float u2)
{
    const f3 vh = normalize(mk(alpha * ve.x, alpha * ve.y, ve.z));
    const float lensq = vh.x * vh.x + vh.y * vh.y;
    const f3 t1v = lensq > 0.0f ? mk(-vh.y, vh.x, 0.0f) * (1.0f / sqrtf(lensq)) : mk(1.0f, 0.0f, 0.0f);
    const f3 t2v = cross(vh, t1v);
    const float r = sqrtf(u1);
    const float phi = 2.0f * kPIf * u2;
    const float sp = sinf(phi), cp = cosf(phi);
    const float t1 = r * cp;
    const float s = 0.5f * (1.0f + vh.z);
    const float t2 = (1.0f - s) * sqrtf(fmaxf(0.0f, 1.0f - t1 * t1)) + s * (r * sp);
    const f3 nh = t1 * t1v + t2 * t2v + sqrtf(fmaxf(0.0f, 1.0f - t1 * t1 - t2 * t2)) * vh;
    return normalize(mk(alpha * nh.x, alpha * nh.y, fmaxf(0.0f, nh.z)));
}
static inline f3 mf_conductor_f(float c) { return fresnelSchlickConductor(c, mk(1.45f, 0.7f, 1.55f), mk(3.0f, 2.2f, 3.5f)); }
static inline float mf_dielectric_f(float c, bool entering, float ior) { return FrDielectric(entering ? c : -c, 1.0f, ior); }

/* microfacet_ref.sample for one wo (unit, away from the surface) at the face-forwarded normal N: u1, u2 the visible normal, u3 the
 * dielectric's lobe.  Out: wi, weight = f |cos_i| / pdf without Kd, pdf, lobe (1 reflection, 2 transmission).  false (lobe 0, weight
 * 0, pdf 0): wi lies on the wrong side, the path ends. */
static inline bool mf_sample(int bsdf, const f3& wo, const f3& N, bool entering, float alpha, float ior, float u1, float u2, float u3,
                             f3& wi, f3& weight, float& pdf, int& lobe)
{
    f3 tg, bn;
    onb_axes(N, tg, bn);
    const float co = dot(wo, N);
    f3 h = ggx_sample_vndf(mk(dot(wo, tg), dot(wo, bn), co), alpha, u1, u2);
    h = h.x * tg + h.y * bn + h.z * N;
    const float a2 = alpha * alpha;
    const float oh = dot(wo, h);
    const float lo = ggx_lambda(co, a2);
    const float d = ggx_d(dot(N, h), a2);
    const float pdf_h = d / (4.0f * co * (1.0f + lo));
    weight = mk(0.0f); pdf = 0.0f; lobe = 0;
    float F = 1.0f;
    bool transmit = false;
    if (bsdf == PT_BSDF_REFRACTION) {
        F = mf_dielectric_f(oh, entering, ior);
        transmit = !(u3 < F);
    }
    if (!transmit) {
        wi = (2.0f * oh) * h - wo;
        const float ci = dot(wi, N);
        if (!(ci > 0.0f)) return false;
        const float g = (1.0f + lo) / (1.0f + lo + ggx_lambda(ci, a2));
        weight = bsdf == PT_BSDF_METALLIC ? mf_conductor_f(oh) * g : mk(g);
        pdf = bsdf == PT_BSDF_METALLIC ? pdf_h : F * pdf_h;
        lobe = 1;
        return true;
    }
    const float eta = entering ? ior : 1.0f / ior;
    const float e = 1.0f / eta;
    const float k = 1.0f - e * e * (1.0f - oh * oh);
    if (!(k >= 0.0f)) { wi = mk(0.0f); return false; }
    wi = (e * oh - sqrtf(k)) * h - e * wo;
    const float ci = dot(wi, N);
    if (!(ci < 0.0f)) return false;
    const float ih = dot(wi, h);
    const float den = oh + eta * ih;
    weight = mk((1.0f + lo) / (1.0f + lo + ggx_lambda(ci, a2)));
    pdf = (1.0f - F) * ((d * oh * eta * eta * fabsf(ih)) / (co * (1.0f + lo) * den * den));
    lobe = 2;
    return true;
}

/* microfacet_ref.evaluate: f (without Kd) and the solid-angle pdf of mf_sample for (wo, wi); zero where mf_sample cannot draw wi */
static inline void mf_eval(int bsdf, const f3& wo, const f3& N, bool entering, float alpha, float ior, const f3& wi, f3& f, float& pdf)
{
    f = mk(0.0f); pdf = 0.0f;
    const float a2 = alpha * alpha;
    const float co = dot(wo, N), ci = dot(wi, N);
    const float lo = ggx_lambda(co, a2);
    if (ci > 0.0f) {
        const f3 h = normalize(wo + wi);
        const float oh = dot(wo, h);
        if (!(oh > 0.0f)) return;
        const float d = ggx_d(dot(N, h), a2);
        const float g2 = 1.0f / (1.0f + lo + ggx_lambda(ci, a2));
        const float dg = (d * g2) / (4.0f * co * ci);
        const float pdf_h = d / (4.0f * co * (1.0f + lo));
        if (bsdf == PT_BSDF_METALLIC) { f = mf_conductor_f(oh) * dg; pdf = pdf_h; }
        else { const float F = mf_dielectric_f(oh, entering, ior); f = mk(F * dg); pdf = F * pdf_h; }
    } else if (ci < 0.0f && bsdf == PT_BSDF_REFRACTION) {
        const float eta = entering ? ior : 1.0f / ior;
        f3 h = normalize(wo + eta * wi);
        if (dot(h, N) < 0.0f) h = -h;
        const float oh = dot(wo, h), ih = dot(wi, h);
        if (!(oh > 0.0f && ih < 0.0f)) return;
        const float F = mf_dielectric_f(oh, entering, ior);
        const float d = ggx_d(dot(N, h), a2);
        const float g2 = 1.0f / (1.0f + lo + ggx_lambda(ci, a2));
        const float den = oh + eta * ih;
        const float j = (d * oh * eta * eta * fabsf(ih)) / (co * den * den);
        f = mk((1.0f - F) * ((j * g2) / fabsf(ci)));
        pdf = (1.0f - F) * (j / (1.0f + lo));
    }
}

/* ---------------------------------------------------------- light mode 1 (NOT the reference) ----
 * SURVEY.md section 8 f4, opt-in: the area light is what the OBJ says is emissive (every triangle whose material has
 * Ke != 0) instead of the rectangle hard-coded at PathTracerMain.cpp:154-158, and the estimator is a consistent one:
 *   - next-event estimation samples a point on the emissive triangles uniformly by area (z1 picks the triangle through
 *     the area CDF and, rescaled, is the first barycentric variate; z2 the second) — the same two draws the reference
 *     makes at :985-986, so the random streams stay aligned with mode 0;
 *   - a BSDF-sampled ray that hits an emitter and the light sample are combined with the power heuristic (Veach) instead
 *     of being added twice (:992-1000 + :1003-1026);
 *   - a directly seen emitter contributes Ke (mode 0: Ke + Ke * Kd), an emitter reached by a bounce
 *     throughput * Ke (mode 0: throughput * Kd_emitter * Ke);
 *   - uniform hemisphere sampling carries its 2 cos(theta) weight (mode 0 omits it), so importance sampling
 *     on / off and direct lighting on / off all converge to the same image;
 *   - under the reference's material model (orc_scene_set_material_model 0) conductor and dielectric keep the reference's
 *     directions and throughput; they take no light sample (their emitter hits count in full).
 * With an environment map (orc_scene_set_environment) the map is a light too: a light sample goes to it when z1 < p_env (0.5 beside
 * emissive triangles, 1 without, 0 for a black map), z1 rescaled for the strategy chosen; the triangles' pdfs carry 1 - p_env; the
 * map's shadow ray runs to 1e16; a miss after a light-sampled vertex is weighted against p_env * env_pdf (raygen_pixel).
 * Under the microfacet model (1) metal and glass of alpha >= kSmoothAlpha are GGX BSDFs (mf_sample: metal 2 draws, glass 3; a failed
 * sample ends the path, its light sample still counts) that take light samples weighted against mf_eval's pdf; a smooth conductor
 * draws 2, discards them and is a mirror about N; smooth glass is the code above.
 * `contrib` is everything this segment adds to the pixel, already multiplied by the path throughput. */
static inline float light_pdf_area_to_solid(float dist2, float cos_l, float area_total) { return dist2 / (area_total * cos_l); }

static inline void closesthit_scene_lights(const Scene& sc, const pt_params& params, int use_bvh,
                                           const f3& ray_org, const f3& ray_dir, float t_hit, uint32_t prim_idx,
                                           PRD& prd, float& prev_pdf, f3& contrib, Counters& cnt)
{
    const uint32_t mat_id = sc.mat_ids[prim_idx];
    const pt_material& rt = sc.mats[mat_id];
    const Tri& tri = sc.tris[prim_idx];
    const bool env = sc.env.w != 0;
    const float p_env = sc.p_env;
    const bool useDirectLighting = params.useDirectLighting != 0 && (!sc.lights.empty() || (env && p_env > 0.0f));
    const bool useImportanceSampling = params.useImportanceSampling != 0;
    const int bsdfType = rt.bsdfType;
    const f3 N_0 = normalize(cross(tri.e1, tri.e2));
    const f3 N = faceforward(N_0, -ray_dir, N_0);
    const f3 P = ray_org + t_hit * ray_dir;
    const f3 Kd = mk(rt.diffuse), Ke = mk(rt.emission);
    const float area_total = sc.lights.empty() ? 0.0f : sc.lights.back().cdf;
    contrib = mk(0.0f);
    prd.emissionColor = mk(0.0f);
    prd.radiance = mk(0.0f);

    uint32_t seed = prd.randomSeed;
    if (length(Ke) > 0.0f) {
        /* an emitter ends the path (as :992-1000); seen directly it counts in full, reached by a sampled bounce that also
         * took a light sample it gets the BSDF strategy's share */
        float w = 1.0f;
        if (prd.depth > 0 && prev_pdf > 0.0f) {
            const float cos_l = fabsf(dot(N_0, ray_dir));
            float p_l = light_pdf_area_to_solid(t_hit * t_hit, cos_l, area_total);
            if (env) p_l = p_l * (1.0f - p_env);
            w = cos_l > 0.0f ? (prev_pdf * prev_pdf) / (prev_pdf * prev_pdf + p_l * p_l) : 1.0f;
        }
        contrib = prd.attenuation * Ke * w;
        /* the reference's draws of this segment, so that the stream position does not depend on what was hit */
        if (bsdfType == PT_BSDF_REFRACTION) (void)rnd(seed); else { (void)rnd(seed); (void)rnd(seed); }
        (void)rnd(seed); (void)rnd(seed);
        prd.randomSeed = seed;
        prd.done = 1;
        return;
    }
    prd.done = 0;
    const f3 att_in = prd.attenuation;
    float bsdf_pdf = 0.0f;                 /* solid-angle pdf of the sampled continuation; 0 = no light sample taken here */
    const bool micro = sc.material_model == 1 && bsdfType != PT_BSDF_DIFFUSE;
    const float alpha = micro ? sc.alpha[mat_id] : 0.0f;
    const bool rough = micro && !(alpha < kSmoothAlpha);
    const f3 wo = -ray_dir;
    const bool entering = dot(wo, N_0) > 0.0f;
    if (bsdfType == PT_BSDF_DIFFUSE) {
        const float z1 = rnd(seed);
        const float z2 = rnd(seed);
        OrthonormalBasis onb(N);
        f3 w_in;
        if (useImportanceSampling) cosine_sample_hemisphere(z1, z2, w_in);
        else                       uniform_sample_hemisphere(z1, z2, w_in);
        const float cos_out = w_in.z;
        onb.inverse_transform(w_in);
        prd.direction = w_in;
        prd.origin = P;
        if (useImportanceSampling) { prd.attenuation = att_in * Kd; bsdf_pdf = cos_out / kPIf; }
        else                       { prd.attenuation = att_in * Kd * (2.0f * cos_out); bsdf_pdf = 1.0f / (2.0f * kPIf); }
    } else if (rough) {                    /* metal: 2 draws, glass: 3 */
        const float z1 = rnd(seed);
        const float z2 = rnd(seed);
        const float z3 = bsdfType == PT_BSDF_REFRACTION ? rnd(seed) : 0.0f;
        f3 wi = mk(0.0f), wt; float pdf; int lobe;
        const bool ok = mf_sample(bsdfType, wo, N, entering, alpha, rt.ior, z1, z2, z3, wi, wt, pdf, lobe);
        prd.direction = wi;
        prd.origin = P + wi * (bsdfType == PT_BSDF_METALLIC ? 1e-4f : 1e-3f);
        prd.attenuation = att_in * (wt * Kd);
        bsdf_pdf = pdf;
        prd.done = !ok;                    /* below the plane: the path ends here (its light sample still counts) */
    } else if (bsdfType == PT_BSDF_METALLIC && micro) {     /* smooth conductor: a mirror about N, the same two draws */
        (void)rnd(seed); (void)rnd(seed);
        const f3 R = reflect(ray_dir, N);
        prd.direction = R;
        prd.origin = P + R * 1e-4f;
        prd.attenuation = att_in * (mf_conductor_f(fmaxf(dot(N, wo), 0.0f)) * Kd);
    } else if (bsdfType == PT_BSDF_METALLIC) {
        const float z1 = rnd(seed);
        const float z2 = rnd(seed);
        f3 microfacetNormal = sampleGGX(z1, z2, 0.2f, N);
        f3 R = reflect(ray_dir, microfacetNormal);
        prd.direction = R;
        prd.origin = P + R * 1e-4f;
        f3 eta = mk((float)1.45, (float)0.7, (float)1.55);
        f3 k = mk((float)3.0, (float)2.2, (float)3.5);
        float cosTheta = fmaxf(dot(microfacetNormal, -ray_dir), 0.0f);
        prd.attenuation = att_in * (fresnelSchlickConductor(cosTheta, eta, k) * Kd);
    } else if (bsdfType == PT_BSDF_REFRACTION) {
        f3 incidentRayDir = normalize(ray_dir);
        float cos_theta = dot(normalize(-ray_dir), N_0);
        float F = FrDielectric(cos_theta, 1.0f, rt.ior);
        if (rnd(seed) < F) {
            prd.direction = reflect(incidentRayDir, N_0);
        } else {
            f3 refractedDir;
            bool didRefract = refract(refractedDir, incidentRayDir, N_0, rt.ior);
            prd.direction = didRefract ? refractedDir : reflect(incidentRayDir, N_0);
        }
        prd.origin = P + prd.direction * 1e-3f;
        prd.attenuation = att_in * Kd;
    }
    const float z1 = rnd(seed);
    const float z2 = rnd(seed);
    prd.randomSeed = seed;
    prev_pdf = 0.0f;
    const bool lit = useDirectLighting && (bsdfType == PT_BSDF_DIFFUSE || rough);     /* this vertex takes a light sample */
    if (!lit) return;
    bool to_env = false;
    float zl = z1;
    if (env) {
        to_env = z1 < p_env;
        zl = to_env ? z1 / p_env : (z1 - p_env) / (1.0f - p_env);
    }
    prev_pdf = bsdf_pdf;                   /* a later emitter hit or miss is MIS-weighted */
    f3 L, Le = mk(0.0f);
    float Ldist, p_l, nDl, geom = 0.0f;
    bool want_shadow;
    if (to_env) {                          /* a direction from the map; its shadow ray reaches as far as a radiance ray */
        float pdf_e;
        const bool ok = env_sample(sc.env, zl, z2, L, pdf_e, Le);
        Ldist = 1e16f;
        nDl = dot(N, L);
        p_l = p_env * pdf_e;
        want_shadow = ok && (rough || nDl > 0.0f);
    } else {                               /* pick the triangle whose CDF interval holds zl * A, reuse the position inside the interval */
        const float target = zl * area_total;
        size_t k = 0;
        while (k + 1 < sc.lights.size() && !(target < sc.lights[k].cdf)) k++;
        const LightTri& lt = sc.lights[k];
        const float lo = k ? sc.lights[k - 1].cdf : 0.0f;
        const float u = fminf(fmaxf((target - lo) / lt.area, 0.0f), 0.99999994f);
        const float su = sqrtf(u);
        const f3 light_pos = lt.v0 + lt.e1 * (su * (1.0f - z2)) + lt.e2 * (su * z2);
        const f3 Lv = light_pos - P;
        const float dist2 = dot(Lv, Lv);
        Ldist = sqrtf(dist2);
        L = Lv / Ldist;
        nDl = dot(N, L);
        const float LnDl = fabsf(dot(lt.n, L));
        p_l = light_pdf_area_to_solid(dist2, LnDl, area_total);
        if (env) p_l = p_l * (1.0f - p_env);
        geom = nDl * LnDl * area_total / (kPIf * dist2);      /* (Kd / pi) cos / p_area-as-solid-angle, Kd below */
        if (env) geom = geom / (1.0f - p_env);
        Le = lt.Ke;
        want_shadow = nDl > 0.0f && LnDl > 0.0f;
        if (rough) want_shadow = LnDl > 0.0f;
    }
    f3 f = mk(0.0f);
    float p_b;
    if (bsdfType == PT_BSDF_DIFFUSE) {
        p_b = useImportanceSampling ? nDl / kPIf : 1.0f / (2.0f * kPIf);
    } else {
        mf_eval(bsdfType, wo, N, entering, alpha, rt.ior, L, f, p_b);
        want_shadow = want_shadow && p_b > 0.0f;
    }
    if (!want_shadow) return;
    cnt.shadow_rays++;
    const bool occluded = use_bvh ? any_bvh(sc, P, L, 0.01f, Ldist - 0.01f) : any_brute(sc, P, L, 0.01f, Ldist - 0.01f);
    if (occluded) return;
    const float w = (p_l * p_l) / (p_l * p_l + p_b * p_b);
    if (bsdfType != PT_BSDF_DIFFUSE) contrib = att_in * Kd * f * Le * ((fabsf(nDl) / p_l) * w);
    else if (to_env)                 contrib = att_in * Kd * Le * ((nDl / (kPIf * p_l)) * w);
    else                             contrib = att_in * Kd * Le * (geom * w);
}

/* __raygen__rg, pathTracerPrograms.cu:707-816, for launch index (x, y) */
static void raygen_pixel(const Scene& sc, const pt_params& params, int use_bvh, int chunks, uint32_t x, uint32_t y,
                         float* accumulation, uint8_t* framebuffer, Counters& cnt)
{
    const int w = params.width, h = params.height;
    const f3 eye = mk(params.cameraEye), U = mk(params.cameraU), V = mk(params.cameraV), W = mk(params.cameraW);
    const int subframe_index = params.currentFrameIdx;
    const unsigned maxDepth = params.maxDepth;

    uint32_t seed = tea4(y * w + x, subframe_index);               /* :721 */
    // `chunks` > 1 is NOT the reference: the same samples in the same order, but summed as `chunks`
    // consecutive runs whose partial sums are then added in run order (the association the product's
    // pt_set_sample_chunks() uses).  chunks == 1 is the reference's single left-to-right sum (:760-761).
    f3 total = mk(0.0f);
    f3 result = mk(0.0f);
    int i = params.samplesPerPixel;
    const int run = (int)params.samplesPerPixel / (chunks > 0 ? chunks : 1);
    int in_run = 0, runs_done = 0;
    PRD prd; memset(&prd, 0, sizeof(prd));
    do {
        /* :730 make_float2(rnd(seed), rnd(seed)): left-to-right, x first */
        const float jx = rnd(seed);
        const float jy = rnd(seed);
        const float dx = 2.0f * (((float)x + jx) / (float)w) - 1.0f;       /* :732-735 */
        const float dy = 2.0f * (((float)y + jy) / (float)h) - 1.0f;
        f3 ray_direction = normalize(dx * U + dy * V + W);
        f3 ray_origin = eye;
        prd.attenuation = mk(1.f);
        prd.randomSeed = seed;
        prd.depth = 0;
        float prev_pdf = 0.0f;             /* light mode 1 only */
        cnt.paths++;
        for (;;) {
            Hit hit;
            cnt.radiance_rays++;
            if (use_bvh) closest_bvh(sc, ray_origin, ray_direction, 0.01f, 1e16f, hit);
            else         closest_brute(sc, ray_origin, ray_direction, 0.01f, 1e16f, hit);
            if (hit.prim != 0xFFFFFFFFu && sc.light_mode == 1) {
                f3 contrib;
                closesthit_scene_lights(sc, params, use_bvh, ray_origin, ray_direction, hit.t, hit.prim, prd, prev_pdf, contrib, cnt);
                result += contrib;         /* already carries the throughput; prd.emissionColor / radiance are zero */
            } else if (hit.prim != 0xFFFFFFFFu) {
                closesthit(sc, params, use_bvh, ray_origin, ray_direction, hit.t, hit.prim, prd, cnt);
            } else {                                   /* __miss__ms :833-847, background 0 (PathTracerMain.cpp:568) */
                prd.radiance = mk(0.0f);
                prd.emissionColor = mk(0.f);
                prd.done = 1;
                if (sc.env.w != 0) {                   /* NOT the reference: the environment map replaces the background */
                    const f3 Le = env_eval(sc.env, ray_direction);
                    if (sc.light_mode == 1) {          /* a BSDF-sampled direction after a light sample: power heuristic against the map */
                        float wm = 1.0f;
                        if (prd.depth > 0 && prev_pdf > 0.0f) {
                            const float pe = sc.p_env * env_pdf(sc.env, ray_direction);
                            wm = (prev_pdf * prev_pdf) / (prev_pdf * prev_pdf + pe * pe);
                        }
                        result += prd.attenuation * Le * wm;
                    } else {
                        prd.radiance = Le;
                    }
                }
            }
            result += prd.emissionColor;               /* :760-761 */
            result += prd.radiance * prd.attenuation;
            float p = dot(prd.attenuation, mk(0.30f, 0.59f, 0.11f));
            if (sc.light_mode == 1) p = fminf(p, 1.0f);   /* mode 1: the 2 cos weight can lift the throughput above 1; a survival probability is <= 1 */
            bool russianRoulette = rnd(prd.randomSeed) > p;
            const bool done = prd.done || russianRoulette || (unsigned)prd.depth >= maxDepth;
            if (done) break;
            prd.attenuation = safeDivide(prd.attenuation, p);
            ray_origin = prd.origin;
            ray_direction = prd.direction;
            ++prd.depth;
        }
        if (chunks > 1 && ++in_run == run) {
            total = runs_done == 0 ? result : total + result;
            result = mk(0.0f); in_run = 0; runs_done++;
        }
    } while (--i);
    if (chunks > 1) result = total;

    const uint32_t image_index = y * params.width + x;
    f3 accum_color = result / (float)params.samplesPerPixel;        /* :784 */
    if (subframe_index > 0) {                                       /* :803-810 */
        const float a = 1.0f / (float)(subframe_index + 1);
        const f3 prev = mk(accumulation[4 * image_index], accumulation[4 * image_index + 1], accumulation[4 * image_index + 2]);
        accum_color = lerp(prev, accum_color, a);
    }
    accumulation[4 * image_index + 0] = accum_color.x;
    accumulation[4 * image_index + 1] = accum_color.y;
    accumulation[4 * image_index + 2] = accum_color.z;
    accumulation[4 * image_index + 3] = 1.0f;
    if (framebuffer) make_color(accum_color, framebuffer + 4 * image_index);
}

/* sutil/WorkDistribution.h:60-81 */
static inline void sample_pixel(int num_gpus, int width, int gpu_idx, int sample_idx, int& px, int& py)
{
    const int TILE_WIDTH = 8, TILE_HEIGHT = 4;
    const int tile_strip_width = TILE_WIDTH * num_gpus;
    const int tile_strip_height = TILE_HEIGHT;
    const int num_tile_strip_cols = width / tile_strip_width + (width % tile_strip_width == 0 ? 0 : 1);
    const int tile_strip_idx = sample_idx / (TILE_WIDTH * TILE_HEIGHT);
    const int tile_strip_y = tile_strip_idx / num_tile_strip_cols;
    const int tile_strip_x = tile_strip_idx - tile_strip_y * num_tile_strip_cols;
    const int tile_strip_x_start = tile_strip_x * tile_strip_width;
    const int tile_strip_y_start = tile_strip_y * tile_strip_height;
    const int tile_pixel_idx = sample_idx - (tile_strip_idx * TILE_WIDTH * TILE_HEIGHT);
    const int tile_pixel_y = tile_pixel_idx / TILE_WIDTH;
    const int tile_pixel_x = tile_pixel_idx - tile_pixel_y * TILE_WIDTH;
    const int tile_offset_x = (gpu_idx + tile_strip_y % num_gpus) % num_gpus * TILE_WIDTH;
    py = tile_strip_y_start + tile_pixel_y;
    px = tile_strip_x_start + tile_pixel_x + tile_offset_x;
}
/* sutil/WorkDistribution.h:50-57 */
static inline int num_samples(int num_gpus, int width, int height)
{
    const int tile_strip_width = 8 * num_gpus, tile_strip_height = 4;
    const int cols = width / tile_strip_width + (width % tile_strip_width == 0 ? 0 : 1);
    const int rows = height / tile_strip_height + (height % tile_strip_height == 0 ? 0 : 1);
    return rows * cols * 8 * 4;
}

} /* namespace */

/* ======================================================================= C API == */
ORC_API uint32_t orc_tea4(uint32_t v0, uint32_t v1) { return tea4(v0, v1); }

ORC_API void orc_rnd_stream(uint32_t seed, size_t n, uint32_t* states_out, float* values_out)
{
    for (size_t i = 0; i < n; i++) { float v = rnd(seed); if (states_out) states_out[i] = seed; if (values_out) values_out[i] = v; }
}

ORC_API void orc_make_color(const float* rgb, size_t n, uint8_t* rgba_out)
{
    for (size_t i = 0; i < n; i++) make_color(mk(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]), rgba_out + 4 * i);
}

ORC_API void orc_refract(const float* i3, const float* n3, float ior, float* r3, int* ok)
{
    f3 r; bool b = refract(r, mk(i3[0], i3[1], i3[2]), mk(n3[0], n3[1], n3[2]), ior);
    r3[0] = r.x; r3[1] = r.y; r3[2] = r.z; *ok = b;
}

/* op: 0 normalize(a) 1 reflect(a,b) 2 faceforward(a,b,c) 3 lerp(a,b,s) 4 cross(a,b) 5 a/s */
ORC_API void orc_vec_op(int op, const float* a, const float* b, const float* c, float s, float* out)
{
    f3 A = mk(a[0], a[1], a[2]), B = b ? mk(b[0], b[1], b[2]) : mk(0), C = c ? mk(c[0], c[1], c[2]) : mk(0), r = mk(0);
    switch (op) {
    case 0: r = normalize(A); break;
    case 1: r = reflect(A, B); break;
    case 2: r = faceforward(A, B, C); break;
    case 3: r = lerp(A, B, s); break;
    case 4: r = cross(A, B); break;
    case 5: r = A / s; break;
    }
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}

/* ---- the OptiX-free helpers of pathTracerPrograms.cu, one export each, same signatures as ref_math_shim.cpp's
 * exports over the reference's own text (tests/test_oracle_golden.py compares them bit for bit) ---- */
ORC_API void orc_onb_transform(const float* n3, const float* p3, size_t n, float* out3)
{
    for (size_t i = 0; i < n; i++) {
        OrthonormalBasis onb(mk(n3[3 * i], n3[3 * i + 1], n3[3 * i + 2]));
        f3 p = mk(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]);
        onb.inverse_transform(p);
        out3[3 * i] = p.x; out3[3 * i + 1] = p.y; out3[3 * i + 2] = p.z;
    }
}
ORC_API void orc_safe_divide(const float* a, const float* b, size_t n, float* out)
{
    for (size_t i = 0; i < n; i++) out[i] = safeDivide(a[i], b[i]);
}
ORC_API void orc_safe_divide3(const float* a3, const float* b, size_t n, float* out3)
{
    for (size_t i = 0; i < n; i++) { f3 r = safeDivide(mk(a3[3 * i], a3[3 * i + 1], a3[3 * i + 2]), b[i]); out3[3 * i] = r.x; out3[3 * i + 1] = r.y; out3[3 * i + 2] = r.z; }
}
ORC_API void orc_sample_hemisphere(int which, const float* u1, const float* u2, size_t n, float* out3)
{
    for (size_t i = 0; i < n; i++) {
        f3 p = mk(0.0f);
        if (which == 0) cosine_sample_hemisphere(u1[i], u2[i], p);
        else            uniform_sample_hemisphere(u1[i], u2[i], p);
        out3[3 * i] = p.x; out3[3 * i + 1] = p.y; out3[3 * i + 2] = p.z;
    }
}
ORC_API void orc_sample_ggx(const float* u1, const float* u2, const float* roughness, const float* n3, size_t n, float* out3)
{
    for (size_t i = 0; i < n; i++) {
        f3 r = sampleGGX(u1[i], u2[i], roughness[i], mk(n3[3 * i], n3[3 * i + 1], n3[3 * i + 2]));
        out3[3 * i] = r.x; out3[3 * i + 1] = r.y; out3[3 * i + 2] = r.z;
    }
}
ORC_API void orc_fresnel_conductor(const float* cos_theta, const float* eta3, const float* k3, size_t n, float* out3)
{
    for (size_t i = 0; i < n; i++) {
        f3 r = fresnelSchlickConductor(cos_theta[i], mk(eta3[3 * i], eta3[3 * i + 1], eta3[3 * i + 2]), mk(k3[3 * i], k3[3 * i + 1], k3[3 * i + 2]));
        out3[3 * i] = r.x; out3[3 * i + 1] = r.y; out3[3 * i + 2] = r.z;
    }
}
ORC_API void orc_fr_dielectric(const float* cos_i, const float* eta_i, const float* eta_t, size_t n, float* out)
{
    for (size_t i = 0; i < n; i++) out[i] = FrDielectric(cos_i[i], eta_i[i], eta_t[i]);
}

/* Camera::UVWFrame, sutil/Camera.cpp:34-45 */
ORC_API void orc_camera_uvw(const float* eye, const float* lookat, const float* up, float fovY, float aspect,
                            float* U3, float* V3, float* W3)
{
    f3 W = mk(lookat[0], lookat[1], lookat[2]) - mk(eye[0], eye[1], eye[2]);
    float wlen = length(W);
    f3 U = normalize(cross(W, mk(up[0], up[1], up[2])));
    f3 V = normalize(cross(U, W));
    float vlen = wlen * tanf(0.5f * fovY * kPIf / 180.0f);
    V *= vlen;
    float ulen = vlen * aspect;
    U *= ulen;
    U3[0] = U.x; U3[1] = U.y; U3[2] = U.z; V3[0] = V.x; V3[1] = V.y; V3[2] = V.z; W3[0] = W.x; W3[1] = W.y; W3[2] = W.z;
}

ORC_API int orc_num_samples(int num_gpus, int width, int height) { return num_samples(num_gpus, width, height); }
ORC_API void orc_sample_pixel(int num_gpus, int width, int gpu_idx, int sample_idx, int* px, int* py)
{ sample_pixel(num_gpus, width, gpu_idx, sample_idx, *px, *py); }

ORC_API void* orc_scene_create(const float* verts_xyzw, size_t n_verts, const uint32_t* idx, size_t n_tris,
                               const uint32_t* mat_ids, const pt_material* mats, size_t n_mats)
{
    Scene* sc = new Scene();
    sc->tris.resize(n_tris);
    for (size_t i = 0; i < n_tris; i++) {
        uint32_t a = idx[3 * i], b = idx[3 * i + 1], c = idx[3 * i + 2];
        if (a >= n_verts || b >= n_verts || c >= n_verts) { delete sc; return NULL; }
        f3 v0 = mk(verts_xyzw[4 * a], verts_xyzw[4 * a + 1], verts_xyzw[4 * a + 2]);
        f3 v1 = mk(verts_xyzw[4 * b], verts_xyzw[4 * b + 1], verts_xyzw[4 * b + 2]);
        f3 v2 = mk(verts_xyzw[4 * c], verts_xyzw[4 * c + 1], verts_xyzw[4 * c + 2]);
        sc->tris[i].v0 = v0; sc->tris[i].e1 = v1 - v0; sc->tris[i].e2 = v2 - v0;
        if (mat_ids && mat_ids[i] >= n_mats) { delete sc; return NULL; }
    }
    if (mat_ids) sc->mat_ids.assign(mat_ids, mat_ids + n_tris);
    if (mats) sc->mats.assign(mats, mats + n_mats);
    sc->light_mode = 0;
    sc->p_env = 0.0f;
    sc->material_model = 0;
    sc->alpha.assign(n_mats, 0.0f);
    for (size_t i = 0; mats && i < n_mats; i++)
        sc->alpha[i] = mats[i].roughness > 0.0f ? fminf(mats[i].roughness, 1.0f) : 0.0f;     /* NaN and negative values: 0 */
    if (mat_ids && mats) {
        float run = 0.0f;
        for (size_t i = 0; i < n_tris; i++) {
            const f3 Ke = mk(mats[mat_ids[i]].emission);
            if (!(length(Ke) > 0.0f)) continue;
            const f3 c = cross(sc->tris[i].e1, sc->tris[i].e2);
            const float area = 0.5f * length(c);
            if (!(area > 0.0f)) continue;
            LightTri lt; lt.v0 = sc->tris[i].v0; lt.e1 = sc->tris[i].e1; lt.e2 = sc->tris[i].e2; lt.n = normalize(c); lt.Ke = Ke; lt.area = area;
            run += area; lt.cdf = run;
            sc->lights.push_back(lt);
        }
    }
    build_bvh(*sc);
    return sc;
}
/* 0: the reference's estimator; 1: scene lights + MIS (closesthit_scene_lights).  Returns the number of light triangles. */
ORC_API int orc_scene_set_light_mode(void* s, int mode) { Scene* sc = (Scene*)s; sc->light_mode = mode == 1 ? 1 : 0; return (int)sc->lights.size(); }
ORC_API void orc_scene_destroy(void* s) { delete (Scene*)s; }

/* The environment map (pt_set_environment): rgb float[h][w][3], row 0 the +Y pole, times scale3 (NULL: 1); rgb NULL or w 0 clears
 * it.  p_env follows: 0.5 with emissive triangles, 1 without, 0 for a black map.  Returns 0, or -1 for a bad size. */
ORC_API int orc_scene_set_environment(void* s, const float* rgb, uint32_t w, uint32_t h, const float* scale3)
{
    Scene* sc = (Scene*)s;
    sc->env = EnvMapH();
    sc->p_env = 0.0f;
    if (!rgb || w == 0) return 0;
    if (h == 0) return -1;
    env_build(sc->env, rgb, w, h, scale3);
    sc->p_env = sc->env.pdf_scale > 0.0f ? (sc->lights.empty() ? 1.0f : 0.5f) : 0.0f;
    return 0;
}
/* the map's tables: texels float[h][w][4] ({r, g, b, weight}), marginal float[h], conditional float[h][w], info {total, pdf_scale,
 * p_env} (any may be NULL).  Returns w * h (0: no map). */
ORC_API size_t orc_scene_environment_tables(void* s, float* texels, float* marginal, float* conditional, float* info3)
{
    const Scene* sc = (const Scene*)s;
    const EnvMapH& E = sc->env;
    if (texels && E.w) memcpy(texels, E.texels.data(), E.texels.size() * sizeof(float));
    if (marginal && E.w) memcpy(marginal, E.marg.data(), E.marg.size() * sizeof(float));
    if (conditional && E.w) memcpy(conditional, E.cond.data(), E.cond.size() * sizeof(float));
    if (info3) { info3[0] = E.total; info3[1] = E.pdf_scale; info3[2] = sc->p_env; }
    return (size_t)E.w * E.h;
}
/* light mode 1's material model (pt_set_material_model): 0 the reference's, 1 GGX metal and glass.  Returns the model set, -1 if unknown. */
ORC_API int orc_scene_set_material_model(void* s, int model)
{
    if (model != 0 && model != 1) return -1;
    ((Scene*)s)->material_model = model;
    return model;
}

/* pt_debug_environment's layouts on the scene's map: op 0 lookup, in float[n][3] -> out float[n][4] (rgb, texel index or -1 without
 * a map); op 1 pdf, in float[n][3] -> out float[n]; op 2 sample, in float[n][2] (u1, u2) -> out float[n][4] (direction, pdf). */
ORC_API int orc_debug_environment(void* s, int op, const float* in, size_t n, float* out)
{
    const EnvMapH& E = ((const Scene*)s)->env;
    if (op < 0 || op > 2) return -1;
    for (size_t i = 0; i < n; i++) {
        if (op == 2) {
            f3 d, Le; float pdf;
            env_sample(E, in[2 * i], in[2 * i + 1], d, pdf, Le);
            out[4 * i] = d.x; out[4 * i + 1] = d.y; out[4 * i + 2] = d.z; out[4 * i + 3] = pdf;
            continue;
        }
        const f3 d = mk(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
        if (op == 1) { out[i] = env_pdf(E, d); continue; }
        const f3 c = env_eval(E, d);
        out[4 * i] = c.x; out[4 * i + 1] = c.y; out[4 * i + 2] = c.z;
        out[4 * i + 3] = E.w ? (float)env_texel(E, d) : -1.0f;
    }
    return 0;
}
/* pt_debug_microfacet's layouts: normal (0, 0, 1) face-forwarded to wo.  op 0 mf_sample, in float[n][9] = wo, alpha, ior, bsdf, u1, u2,
 * u3 -> out float[n][8] = wi, weight, pdf, lobe; op 1 mf_eval, in float[n][9] = wo, wi, alpha, ior, bsdf -> out float[n][4] = f, pdf. */
ORC_API int orc_debug_microfacet(int op, const float* in, size_t n, float* out)
{
    if (op < 0 || op > 1) return -1;
    for (size_t i = 0; i < n; i++) {
        const float* a = in + 9 * i;
        const f3 wo = mk(a[0], a[1], a[2]);
        const f3 N0 = mk(0.0f, 0.0f, 1.0f);
        const f3 N = faceforward(N0, wo, N0);
        const bool entering = wo.z > 0.0f;
        if (op == 0) {
            f3 wi = mk(0.0f), wt; float pdf; int lobe;
            (void)mf_sample((int)a[5], wo, N, entering, a[3], a[4], a[6], a[7], a[8], wi, wt, pdf, lobe);
            float* o = out + 8 * i;
            o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = wt.x; o[4] = wt.y; o[5] = wt.z; o[6] = pdf; o[7] = (float)lobe;
        } else {
            f3 f; float pdf;
            mf_eval((int)a[8], wo, N, entering, a[6], a[7], mk(a[3], a[4], a[5]), f, pdf);
            float* o = out + 4 * i;
            o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = pdf;
        }
    }
    return 0;
}

ORC_API void orc_trace_closest(void* s, const float* rays, size_t n, int use_bvh, float* t_out, uint32_t* prim_out)
{
    const Scene& sc = *(Scene*)s;
    for (size_t i = 0; i < n; i++) {
        const float* r = rays + 8 * i; Hit h;
        if (use_bvh) closest_bvh(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], r[7], h);
        else         closest_brute(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], r[7], h);
        t_out[i] = h.prim == 0xFFFFFFFFu ? -1.0f : h.t; prim_out[i] = h.prim;
    }
}
ORC_API void orc_trace_any(void* s, const float* rays, size_t n, int use_bvh, uint8_t* hit_out)
{
    const Scene& sc = *(Scene*)s;
    for (size_t i = 0; i < n; i++) {
        const float* r = rays + 8 * i;
        hit_out[i] = use_bvh ? any_bvh(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], r[7])
                             : any_brute(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], r[7]);
    }
}

/* One launch (LaunchCurrentFrame, PathTracerMain.cpp:184-210) on the host.
 * accumulation / framebuffer are HOST arrays here (params->accumulationBuffer and
 * ->frameBuffer are ignored).  rank/world select the WorkDistribution partition; chunks: see raygen_pixel
 * (1 = the reference's summation order).
 * stats_out: radiance_rays, shadow_rays, paths.  Returns wall seconds. */
static double render_impl(void* s, const pt_params* params, float* accumulation, uint8_t* framebuffer,
                          int use_bvh, int n_threads, int rank, int world, int chunks, const int* window, uint64_t* stats_out);

ORC_API double orc_render(void* s, const pt_params* params, float* accumulation, uint8_t* framebuffer,
                          int use_bvh, int n_threads, int rank, int world, int chunks, uint64_t* stats_out)
{
    return render_impl(s, params, accumulation, framebuffer, use_bvh, n_threads, rank, world, chunks, NULL, stats_out);
}

/* The same launch restricted to the pixels of a window {x0, y0, width, height} of the full image: pixels outside are
 * neither computed nor written (accumulation / framebuffer stay full-size arrays).  A pixel's value does not depend on
 * any other pixel (:721 seeds by pixel index, :782-814 writes only image_index), so a window of a 1920x1080 launch can
 * be checked without rendering the other two million pixels on the CPU. */
ORC_API double orc_render_window(void* s, const pt_params* params, float* accumulation, uint8_t* framebuffer,
                                 int use_bvh, int n_threads, int chunks, const int* window4, uint64_t* stats_out)
{
    return render_impl(s, params, accumulation, framebuffer, use_bvh, n_threads, 0, 1, chunks, window4, stats_out);
}

static double render_impl(void* s, const pt_params* params, float* accumulation, uint8_t* framebuffer,
                          int use_bvh, int n_threads, int rank, int world, int chunks, const int* window, uint64_t* stats_out)
{
    const Scene& sc = *(Scene*)s;
    const int w = params->width, h = params->height;
    if (world < 1) world = 1;
    const int total = num_samples(world, w, h);
    const int chunk = 64;
    std::atomic<int> next(0);
    if (n_threads < 1) n_threads = 1;
    std::vector<Counters> cnts(n_threads);
    auto t0 = std::chrono::steady_clock::now();
    auto worker = [&](int tid) {
        Counters c = {0, 0, 0};
        for (;;) {
            int b = next.fetch_add(chunk);
            if (b >= total) break;
            int e = std::min(total, b + chunk);
            for (int si = b; si < e; si++) {
                int px, py; sample_pixel(world, w, rank, si, px, py);
                if (px >= w || py >= h) continue;
                if (window && (px < window[0] || py < window[1] || px >= window[0] + window[2] || py >= window[1] + window[3])) continue;
                raygen_pixel(sc, *params, use_bvh, chunks, (uint32_t)px, (uint32_t)py, accumulation, framebuffer, c);
            }
        }
        cnts[tid] = c;
    };
    if (n_threads == 1) worker(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_threads; t++) th.emplace_back(worker, t);
        for (auto& t : th) t.join();
    }
    auto t1 = std::chrono::steady_clock::now();
    if (stats_out) {
        stats_out[0] = stats_out[1] = stats_out[2] = 0;
        for (auto& c : cnts) { stats_out[0] += c.radiance_rays; stats_out[1] += c.shadow_rays; stats_out[2] += c.paths; }
    }
    return std::chrono::duration<double>(t1 - t0).count();
}

ORC_API int orc_uses_hw_fma(void)
{
#ifdef __FMA__
    return 1;
#else
    return 0;
#endif
}
