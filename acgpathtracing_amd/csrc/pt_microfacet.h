// pt_microfacet.h — the microfacet material model (pt_set_material_model(ctx, PT_MATERIALS_MICROFACET), include/acgpt.h): rough
// conductor and rough dielectric as isotropic GGX BSDFs with visible-normal sampling (Heitz 2018), and the light-mode-1 closest-hit
// that uses them (shade_hit_micro, the twin of pt_shading.h's shade_hit_lights).  tests/microfacet_ref.py states the same model in
// NumPy; the render kernels k_render_ggx / k_render_ggx_env (render_pw.inc) and pt_debug_microfacet call these very functions.
// FM: arithmetic level of pt_device.h.
#pragma once
#include "pt_shading.h"

namespace ptd {

constexpr float kSmoothAlpha = 1e-3f;       // alpha below this: the smooth BSDF (mirror / light mode 1's glass)

// the tangent frame of onb_transform (pt_shading.h): local (x, y, z) -> x tg + y bn + z n
template <int FM>
__device__ __forceinline__ void onb_axes(const f3& n, f3& tg, f3& bn)
{
    if (fabsf(n.x) > fabsf(n.z)) bn = mk(-n.y, n.x, 0.0f);
    else                         bn = mk(0.0f, -n.z, n.y);
    bn = m_normalize<FM>(bn);
    tg = m_cross<FM>(bn, n);
}

// Smith Lambda of isotropic GGX for a direction at cosine c to the normal (c != 0), a2 = alpha^2
template <int FM>
__device__ __forceinline__ float ggx_lambda(float c, float a2)
{
    const float c2 = c * c;
    return 0.5f * (m_sqrt<FM>(1.0f + a2 * m_div<FM>(1.0f - c2, c2)) - 1.0f);
}
// D(h) for the cosine ch of the half vector
template <int FM>
__device__ __forceinline__ float ggx_d(float ch, float a2)
{
    const float t = ch * ch * (a2 - 1.0f) + 1.0f;
    return m_div<FM>(a2, kPIf * t * t);
}

// Heitz 2018, "Sampling the GGX Distribution of Visible Normals": a half vector in the local frame for the local direction ve (ve.z > 0)
template <int FM>
__device__ __forceinline__ f3 ggx_sample_vndf(const f3& ve, float alpha, float u1, float u2)
{
    const f3 vh = m_normalize<FM>(mk(alpha * ve.x, alpha * ve.y, ve.z));
    const float lensq = vh.x * vh.x + vh.y * vh.y;
    const f3 t1v = lensq > 0.0f ? mk(-vh.y, vh.x, 0.0f) * m_div<FM>(1.0f, m_sqrt<FM>(lensq)) : mk(1.0f, 0.0f, 0.0f);
    const f3 t2v = cross(vh, t1v);
    const float r = m_sqrt<FM>(u1);
    float sp, cp;
    m_sincos_2pi<FM>(u2, sp, cp);
    const float t1 = r * cp;
    const float s = 0.5f * (1.0f + vh.z);
    const float t2 = (1.0f - s) * m_sqrt<FM>(fmaxf(0.0f, 1.0f - t1 * t1)) + s * (r * sp);
    const f3 nh = t1 * t1v + t2 * t2v + m_sqrt<FM>(fmaxf(0.0f, 1.0f - t1 * t1 - t2 * t2)) * vh;
    return m_normalize<FM>(mk(alpha * nh.x, alpha * nh.y, fmaxf(0.0f, nh.z)));
}

// the reference's conductor Fresnel (pt_shading.h fresnel_conductor with the constants of shade_hit)
template <int FM>
__device__ __forceinline__ f3 mf_conductor_f(float c) { return fresnel_conductor<FM>(c, mk(1.45f, 0.7f, 1.55f), mk(3.0f, 2.2f, 3.5f)); }
// fr_dielectric for the microfacet cosine c = wo.h > 0 on the side wo lies on (entering: outside, eta_i = 1, eta_t = ior)
template <int FM>
__device__ __forceinline__ float mf_dielectric_f(float c, bool entering, float ior) { return fr_dielectric<FM>(entering ? c : -c, 1.0f, ior); }

// Samples the rough BSDF (alpha >= kSmoothAlpha) of bsdf (PT_BSDF_METALLIC or PT_BSDF_REFRACTION) for wo (unit, pointing away from
// the surface) at the face-forwarded normal N (wo.N > 0).  u1, u2 draw the visible normal, u3 the dielectric's lobe.  Out: wi, the
// weight f |wi.N| / pdf without Kd (conductor F G2 / G1(wo) per channel, dielectric G2 / G1(wo)), the solid-angle pdf of wi
// including the lobe's probability, lobe 1 reflection / 2 transmission.  Returns false (lobe 0, weight 0, pdf 0) when wi lies on the
// wrong side of the plane: the path ends.
template <int FM>
__device__ __forceinline__ bool mf_sample(int bsdf, const f3& wo, const f3& N, bool entering, float alpha, float ior,
                                          float u1, float u2, float u3, f3& wi, f3& weight, float& pdf, int& lobe)
{
    f3 tg, bn;
    onb_axes<FM>(N, tg, bn);
    const float co = m_dot<FM>(wo, N);
    f3 h = ggx_sample_vndf<FM>(mk(m_dot<FM>(wo, tg), m_dot<FM>(wo, bn), co), alpha, u1, u2);
    onb_transform<FM>(N, h);
    const float a2 = alpha * alpha;
    const float oh = m_dot<FM>(wo, h);
    const float lo = ggx_lambda<FM>(co, a2);
    const float d = ggx_d<FM>(m_dot<FM>(N, h), a2);
    const float pdf_h = m_div<FM>(d, 4.0f * co * (1.0f + lo));          // G1(wo) D / (4 cos_o): the reflected direction's pdf
    weight = mk(0.0f); pdf = 0.0f; lobe = 0;
    float f = 1.0f;
    bool transmit = false;
    if (bsdf == PT_BSDF_REFRACTION) {
        f = mf_dielectric_f<FM>(oh, entering, ior);
        transmit = !(u3 < f);
    }
    if (!transmit) {
        wi = (2.0f * oh) * h - wo;
        const float ci = m_dot<FM>(wi, N);
        if (!(ci > 0.0f)) return false;
        const float g = m_div<FM>(1.0f + lo, 1.0f + lo + ggx_lambda<FM>(ci, a2));    // G2 / G1(wo)
        weight = bsdf == PT_BSDF_METALLIC ? mf_conductor_f<FM>(oh) * g : mk(g);
        pdf = bsdf == PT_BSDF_METALLIC ? pdf_h : f * pdf_h;
        lobe = 1;
        return true;
    }
    const float eta = entering ? ior : m_div<FM>(1.0f, ior);           // eta_t / eta_i
    const float e = m_div<FM>(1.0f, eta);
    const float k = 1.0f - e * e * (1.0f - oh * oh);
    if (!(k >= 0.0f)) { wi = mk(0.0f); return false; }                  // (total internal reflection has f = 1: not reached)
    wi = (e * oh - m_sqrt<FM>(k)) * h - e * wo;
    const float ci = m_dot<FM>(wi, N);
    if (!(ci < 0.0f)) return false;
    const float ih = m_dot<FM>(wi, h);
    const float den = oh + eta * ih;
    weight = mk(m_div<FM>(1.0f + lo, 1.0f + lo + ggx_lambda<FM>(ci, a2)));
    pdf = (1.0f - f) * m_div<FM>(d * oh * eta * eta * fabsf(ih), co * (1.0f + lo) * den * den);
    lobe = 2;
    return true;
}

// f (per channel, without Kd) and the solid-angle pdf of mf_sample for the pair (wo, wi); zero where mf_sample cannot produce wi
template <int FM>
__device__ __forceinline__ void mf_eval(int bsdf, const f3& wo, const f3& N, bool entering, float alpha, float ior, const f3& wi,
                                        f3& f, float& pdf)
{
    f = mk(0.0f); pdf = 0.0f;
    const float a2 = alpha * alpha;
    const float co = m_dot<FM>(wo, N), ci = m_dot<FM>(wi, N);
    const float lo = ggx_lambda<FM>(co, a2);
    if (ci > 0.0f) {
        const f3 h = m_normalize<FM>(wo + wi);
        const float oh = m_dot<FM>(wo, h);
        if (!(oh > 0.0f)) return;
        const float d = ggx_d<FM>(m_dot<FM>(N, h), a2);
        const float g2 = m_div<FM>(1.0f, 1.0f + lo + ggx_lambda<FM>(ci, a2));
        const float dg = m_div<FM>(d * g2, 4.0f * co * ci);
        const float pdf_h = m_div<FM>(d, 4.0f * co * (1.0f + lo));
        if (bsdf == PT_BSDF_METALLIC) { f = mf_conductor_f<FM>(oh) * dg; pdf = pdf_h; }
        else { const float F = mf_dielectric_f<FM>(oh, entering, ior); f = mk(F * dg); pdf = F * pdf_h; }
    } else if (ci < 0.0f && bsdf == PT_BSDF_REFRACTION) {
        const float eta = entering ? ior : m_div<FM>(1.0f, ior);
        f3 h = m_normalize<FM>(wo + eta * wi);
        if (m_dot<FM>(h, N) < 0.0f) h = -h;
        const float oh = m_dot<FM>(wo, h), ih = m_dot<FM>(wi, h);
        if (!(oh > 0.0f && ih < 0.0f)) return;
        const float F = mf_dielectric_f<FM>(oh, entering, ior);
        const float d = ggx_d<FM>(m_dot<FM>(N, h), a2);
        const float g2 = m_div<FM>(1.0f, 1.0f + lo + ggx_lambda<FM>(ci, a2));
        const float den = oh + eta * ih;
        const float j = m_div<FM>(d * oh * eta * eta * fabsf(ih), co * den * den);      // D (wo.h) / cos_o times the refraction Jacobian
        f = mk((1.0f - F) * m_div<FM>(j * g2, fabsf(ci)));
        pdf = (1.0f - F) * m_div<FM>(j, 1.0f + lo);
    }
}

// ---- light mode 1 with the microfacet model --------------------------------------------------------------------------------------
// shade_hit_lights (pt_shading.h) with metal and glass per the model of include/acgpt.h (pt_set_material_model).  Diffuse vertices,
// smooth glass and emitter hits are that function's code, operation for operation: a scene without metal or rough glass gives its
// bits.  A rough vertex takes a light sample as a diffuse one does (the same z1 rescaling and p_env) and weighs it against mf_eval's
// pdf; its sampled direction's pdf becomes prev_pdf when a light sample was taken.  A smooth conductor is a mirror about N with
// prev_pdf = 0.  ggx(): the GgxArgs of the launch (per-material alpha), env(): the EnvArgs (ENV only), both read where used.
template <int FM = 0, bool ENV = false, typename Late, typename GgxLate, typename EnvLate = int>
__device__ __forceinline__ bool shade_hit_micro(const DeviceScene& sc, Late late, const f3& org, const f3& dir,
                                                float t_hit, int slot, int depth, uint32_t& pseed, f3& att, float& prev_pdf,
                                                Pending& pd, f3& P, f3& L, float& Ldist, GgxLate ggx, EnvLate env = 0)
{
    const float4 sr = sc.shade[slot];
    const uint32_t mw = __float_as_uint(sr.w);
    const DevMaterial* mp = sc.mats + (mw & kShadeMatMask);
    const float4 m0 = mp->kd_ior;
    const f3 Kd = mk(m0.x, m0.y, m0.z);
    const float ior = m0.w;
    f3 Ke = mk(0.0f);
    if ((mw & kShadeHasKe) != 0u) { const float4 m1 = mp->ke_bsdf; Ke = mk(m1.x, m1.y, m1.z); }
    const int bsdf = (int)((mw >> kShadeBsdfShift) & 3u);
    const f3 N0 = mk(sr.x, sr.y, sr.z);
    const f3 N = faceforward(N0, -dir, N0);
    P = org + t_hit * dir;
    const auto& La = late();
    float p_env = 0.0f;
    if constexpr (ENV) p_env = env().p;
    const bool useDL = La.useDL != 0u && (sc.n_lights != 0u || (ENV && p_env > 0.0f));
    const bool useIS = La.useIS != 0u;
    const float area_total = sc.light_area;
    uint32_t s = pseed;
    pd.radiance = mk(0.0f); pd.weight = 0.0f;
    pd.nxt_org = org; pd.nxt_dir = dir;
    if (dot(Ke, Ke) > 0.0f) {                         // emitter hit: shade_hit_lights' code
        float w = 1.0f;
        if (depth > 0 && prev_pdf > 0.0f) {
            const float cos_l = fabsf(dot(N0, dir));
            float p_l = m_div<FM>(t_hit * t_hit, area_total * cos_l);
            if (ENV) p_l = p_l * (1.0f - p_env);
            w = cos_l > 0.0f ? m_div<FM>(prev_pdf * prev_pdf, prev_pdf * prev_pdf + p_l * p_l) : 1.0f;
        }
        pd.radiance = att * Ke * w;
        if (bsdf == PT_BSDF_REFRACTION) (void)rnd(s); else { (void)rnd(s); (void)rnd(s); }
        (void)rnd(s); (void)rnd(s);
        pseed = s;
        pd.done = true;
        return false;
    }
    pd.done = false;
    const f3 att_in = att;
    float bsdf_pdf = 0.0f;
    // a rough vertex: alpha from the launch's table (diffuse vertices do not fetch it)
    const float alpha = bsdf == PT_BSDF_DIFFUSE ? 0.0f : ggx().alpha[mw & kShadeMatMask];
    const bool rough = bsdf != PT_BSDF_DIFFUSE && !(alpha < kSmoothAlpha);
    const f3 wo = -dir;
    const bool entering = dot(wo, N0) > 0.0f;
    if (bsdf == PT_BSDF_DIFFUSE) {
        const float z1 = rnd(s);
        const float z2 = rnd(s);
        f3 w_in = useIS ? (FM >= 1 ? cosine_sample_hemisphere_fast<FM>(z1, z2) : cosine_sample_hemisphere(z1, z2)) : uniform_sample_hemisphere<FM>(z1, z2);
        const float cos_out = w_in.z;
        onb_transform<FM>(N, w_in);
        pd.nxt_dir = w_in;
        pd.nxt_org = P;
        if (useIS) { att = att_in * Kd; bsdf_pdf = FM >= 2 ? cos_out * (1.0f / kPIf) : cos_out / kPIf; }
        else       { att = att_in * Kd * (2.0f * cos_out); bsdf_pdf = 1.0f / (2.0f * kPIf); }
    } else if (rough) {                               // metal: 2 draws, glass: 3
        const float z1 = rnd(s);
        const float z2 = rnd(s);
        const float z3 = bsdf == PT_BSDF_REFRACTION ? rnd(s) : 0.0f;
        f3 wi, wt; float pdf; int lobe;
        const bool ok = mf_sample<FM>(bsdf, wo, N, entering, alpha, ior, z1, z2, z3, wi, wt, pdf, lobe);
        pd.nxt_dir = wi;
        pd.nxt_org = P + wi * (bsdf == PT_BSDF_METALLIC ? 1e-4f : 1e-3f);
        att = att_in * (wt * Kd);
        bsdf_pdf = pdf;
        pd.done = !ok;                                // below the plane: the path ends here (its light sample still counts)
    } else if (bsdf == PT_BSDF_METALLIC) {            // smooth conductor: a mirror about N, the same two draws
        (void)rnd(s); (void)rnd(s);
        const f3 R = reflect(dir, N);
        pd.nxt_dir = R;
        pd.nxt_org = P + R * 1e-4f;
        att = att_in * (mf_conductor_f<FM>(fmaxf(dot(N, wo), 0.0f)) * Kd);
    } else if (bsdf == PT_BSDF_REFRACTION) {          // smooth glass: shade_hit_lights' code
        const f3 inc = m_normalize<FM>(dir);
        const float cos_theta = dot(m_normalize<FM>(-dir), N0);
        const float F = fr_dielectric<FM>(cos_theta, 1.0f, ior);
        if (rnd(s) < F) {
            pd.nxt_dir = reflect(inc, N0);
        } else {
            f3 rd;
            pd.nxt_dir = refract_dir<FM>(rd, inc, N0, ior) ? rd : reflect(inc, N0);
        }
        pd.nxt_org = P + pd.nxt_dir * 1e-3f;
        att = att_in * Kd;
    }
    const float z1 = rnd(s);
    const float z2 = rnd(s);
    pseed = s;
    prev_pdf = 0.0f;
    const bool lit = bsdf == PT_BSDF_DIFFUSE || rough;      // the vertices that take a light sample
    bool want_shadow = false;
    bool to_env = false;
    float zl = z1;
    if (ENV && useDL && lit) {
        to_env = z1 < p_env;
        zl = to_env ? m_div<FM>(z1, p_env) : m_div<FM>(z1 - p_env, 1.0f - p_env);
    }
    bool to_tris = useDL && lit;
    if constexpr (ENV) if (to_env) {                  // a direction from the map; its shadow ray reaches as far as a radiance ray
        to_tris = false;
        float pdf_e; f3 Le;
        const bool ok = env_sample<FM>(env().map, zl, z2, L, pdf_e, Le);
        Ldist = 1e16f;
        const float nDl = dot(N, L);
        prev_pdf = bsdf_pdf;
        const float p_l = p_env * pdf_e;
        if (bsdf == PT_BSDF_DIFFUSE) {
            want_shadow = ok && nDl > 0.0f;
            const float p_b = useIS ? (FM >= 2 ? nDl * (1.0f / kPIf) : nDl / kPIf) : 1.0f / (2.0f * kPIf);
            const float w = m_div<FM>(p_l * p_l, p_l * p_l + p_b * p_b);
            if (want_shadow) pd.radiance = att_in * Kd * Le * (m_div<FM>(nDl, kPIf * p_l) * w);
        } else {
            f3 f; float p_b;
            mf_eval<FM>(bsdf, wo, N, entering, alpha, ior, L, f, p_b);
            want_shadow = ok && p_b > 0.0f;
            const float w = m_div<FM>(p_l * p_l, p_l * p_l + p_b * p_b);
            if (want_shadow) pd.radiance = att_in * Kd * f * Le * (m_div<FM>(fabsf(nDl), p_l) * w);
        }
    }
    if (to_tris) {
        const float target = zl * area_total;
        uint32_t k = 0;
        while (k + 1u < sc.n_lights && !(target < sc.lights[5u * k + 1u].w)) k++;
        const float4 l0 = sc.lights[5u * k], l1 = sc.lights[5u * k + 1u], l2 = sc.lights[5u * k + 2u], l3 = sc.lights[5u * k + 3u], l4 = sc.lights[5u * k + 4u];
        const float lo = k ? sc.lights[5u * (k - 1u) + 1u].w : 0.0f;
        const float u = fminf(fmaxf(m_div<FM>(target - lo, l0.w), 0.0f), 0.99999994f);
        const float su = m_sqrt<FM>(u);
        const f3 light_pos = mk(l0.x, l0.y, l0.z) + mk(l1.x, l1.y, l1.z) * (su * (1.0f - z2)) + mk(l2.x, l2.y, l2.z) * (su * z2);
        const f3 Lv = light_pos - P;
        const float dist2 = dot(Lv, Lv);
        Ldist = m_sqrt<FM>(dist2);
        L = FM >= 2 ? Lv * __builtin_amdgcn_rsqf(dist2) : Lv / Ldist;
        const float nDl = dot(N, L);
        const float LnDl = fabsf(dot(mk(l3.x, l3.y, l3.z), L));
        prev_pdf = bsdf_pdf;
        float p_l = m_div<FM>(dist2, area_total * LnDl);
        if (ENV) p_l = p_l * (1.0f - p_env);
        if (bsdf == PT_BSDF_DIFFUSE) {
            want_shadow = nDl > 0.0f && LnDl > 0.0f;
            const float p_b = useIS ? (FM >= 2 ? nDl * (1.0f / kPIf) : nDl / kPIf) : 1.0f / (2.0f * kPIf);
            const float w = m_div<FM>(p_l * p_l, p_l * p_l + p_b * p_b);
            float geom = m_div<FM>(nDl * LnDl * area_total, kPIf * dist2);
            if (ENV) geom = m_div<FM>(geom, 1.0f - p_env);
            if (want_shadow) pd.radiance = att_in * Kd * mk(l4.x, l4.y, l4.z) * (geom * w);      // counted only if the shadow ray finds nothing
        } else {
            f3 f; float p_b;
            mf_eval<FM>(bsdf, wo, N, entering, alpha, ior, L, f, p_b);
            want_shadow = LnDl > 0.0f && p_b > 0.0f;
            const float w = m_div<FM>(p_l * p_l, p_l * p_l + p_b * p_b);
            if (want_shadow) pd.radiance = att_in * Kd * f * mk(l4.x, l4.y, l4.z) * (m_div<FM>(fabsf(nDl), p_l) * w);
        }
    }
    return want_shadow;
}

}  // namespace ptd
