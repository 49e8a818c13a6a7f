// microfacet.hip — pt_debug_microfacet (include/acgpt_test.h): the device functions of pt_microfacet.h run on arrays, so that
// tests/microfacet_ref.py can hold the kernels' BSDF to its NumPy statement.  Normal (0, 0, 1), face-forwarded to wo; a wo below it
// is a ray leaving the surface's inside (the dielectric's eta swapped).
#include "render_megakernel.h"
#include "pt_microfacet.h"

namespace ptd {

template <int FM>
__global__ void __launch_bounds__(256) k_microfacet_debug(int op, const float* in, uint32_t n, float* out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* a = in + (size_t)i * 9u;
    const f3 wo = mk(a[0], a[1], a[2]);
    const f3 N0 = mk(0.0f, 0.0f, 1.0f);
    const f3 N = faceforward(N0, wo, N0);
    const bool entering = wo.z > 0.0f;
    if (op == 0) {
        const float alpha = a[3], ior = a[4];
        const int bsdf = (int)a[5];
        f3 wi = mk(0.0f), wt; float pdf; int lobe;
        (void)mf_sample<FM>(bsdf, wo, N, entering, alpha, ior, a[6], a[7], a[8], wi, wt, pdf, lobe);
        float* o = out + (size_t)i * 8u;
        o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = wt.x; o[4] = wt.y; o[5] = wt.z; o[6] = pdf; o[7] = (float)lobe;
    } else {
        const f3 wi = mk(a[3], a[4], a[5]);
        const float alpha = a[6], ior = a[7];
        const int bsdf = (int)a[8];
        f3 f; float pdf;
        mf_eval<FM>(bsdf, wo, N, entering, alpha, ior, wi, f, pdf);
        float* o = out + (size_t)i * 4u;
        o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = pdf;
    }
}

hipError_t microfacet_debug(int op, int math, const float* d_in, uint32_t n, float* d_out, hipStream_t stream)
{
    if (op < 0 || op > 1) return hipErrorInvalidValue;
    if (n == 0u) return hipSuccess;
    const dim3 grid((n + 255u) / 256u);
    if (math) hipLaunchKernelGGL(k_microfacet_debug<2>, grid, dim3(256), 0, stream, op, d_in, n, d_out);
    else      hipLaunchKernelGGL(k_microfacet_debug<0>, grid, dim3(256), 0, stream, op, d_in, n, d_out);
    return hipGetLastError();
}

}  // namespace ptd
