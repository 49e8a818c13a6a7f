// environment.hip — the kernels behind pt_set_environment (include/acgpt.h) and pt_debug_environment (include/acgpt_test.h).
//
//   k_env_rows      one workgroup per row: the texels' sampling weights lum(rgb) * sin(pi (row + 0.5) / H), written into .w, and
//                   the row's normalised inclusive scan (its conditional CDF) and total
//   k_env_marginal  one workgroup: the normalised inclusive scan of the row totals (the marginal CDF) and the map's total
//   k_env_debug     the render kernels' lookup, pdf and sample (pt_environment.h) for a list of queries
//
// Both scans run in one fixed order, so that two uploads of the same texels give the same bits (tests/env_ref.py restates it):
// thread t of 256 sums the t-th run of ceil(n / 256) consecutive values in order; a Hillis-Steele scan over the 256 run sums
// (x[t] + x[t - off], off = 1, 2, ..., 128); then each thread adds its run's values in order to the sum of the runs before it.
#include "environment.h"
#include <cmath>
#include <vector>

namespace ptd {

constexpr uint32_t kEnvThreads = 256;

// the inclusive scan of vals[0 .. n) into out[], normalised by the total (a zero total: the uniform CDF (i + 1) / n); returns the total
template <typename Val>
__device__ __forceinline__ float env_block_scan(Val val, float* __restrict__ out, uint32_t n, float* lds)
{
    const uint32_t t = threadIdx.x;
    const uint32_t run = (n + kEnvThreads - 1u) / kEnvThreads;
    const uint32_t b = min(t * run, n), e = min(b + run, n);
    float s = 0.0f;
    for (uint32_t i = b; i < e; i++) s += val(i);
    lds[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < kEnvThreads; off <<= 1) {
        const float left = t >= off ? lds[t - off] : 0.0f;
        __syncthreads();
        if (t >= off) lds[t] = lds[t] + left;
        __syncthreads();
    }
    const float total = lds[kEnvThreads - 1u];
    float acc = t ? lds[t - 1u] : 0.0f;
    for (uint32_t i = b; i < e; i++) {
        acc += val(i);
        out[i] = total > 0.0f ? acc / total : (float)(i + 1u) / (float)n;
    }
    return total;
}

__global__ void __launch_bounds__(kEnvThreads)
k_env_rows(float4* __restrict__ texels, const float* __restrict__ row_sin, float* __restrict__ cond, float* __restrict__ row_total, uint32_t w)
{
    __shared__ float lds[kEnvThreads];
    const uint32_t row = blockIdx.x;
    float4* tx = texels + (size_t)row * w;
    const float s = row_sin[row];
    const uint32_t t = threadIdx.x, run = (w + kEnvThreads - 1u) / kEnvThreads;
    for (uint32_t i = min(t * run, w), e = min(i + run, w); i < e; i++) {        // this thread's run: its own texels only
        float4 v = tx[i];
        v.w = (0.2126f * v.x + 0.7152f * v.y + 0.0722f * v.z) * s;
        tx[i] = v;
    }
    const float total = env_block_scan([&](uint32_t i) { return tx[i].w; }, cond + (size_t)row * w, w, lds);
    if (t == 0u) row_total[row] = total;
}

__global__ void __launch_bounds__(kEnvThreads)
k_env_marginal(const float* __restrict__ row_total, float* __restrict__ marg, uint32_t h, float* __restrict__ total_out)
{
    __shared__ float lds[kEnvThreads];
    const float total = env_block_scan([&](uint32_t i) { return row_total[i]; }, marg, h, lds);
    if (threadIdx.x == 0u) *total_out = total;
}

template <int FM>
__global__ void __launch_bounds__(256)
k_env_debug(const EnvMap E, int op, const float* __restrict__ in, uint32_t n, float* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == 2) {
        f3 d, Le; float pdf;
        env_sample<FM>(E, in[2u * i], in[2u * i + 1u], d, pdf, Le);
        out[4u * i] = d.x; out[4u * i + 1u] = d.y; out[4u * i + 2u] = d.z; out[4u * i + 3u] = pdf;
        return;
    }
    const f3 d = mk(in[3u * i], in[3u * i + 1u], in[3u * i + 2u]);
    if (op == 1) { out[i] = env_pdf<FM>(E, d); return; }
    const f3 c = env_eval(E, d);
    out[4u * i] = c.x; out[4u * i + 1u] = c.y; out[4u * i + 2u] = c.z;
    out[4u * i + 3u] = E.w ? (float)env_texel(E, d) : -1.0f;
}

hipError_t env_debug(const EnvMap& m, int op, int math, const float* d_in, uint32_t n, float* d_out, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    const uint32_t blocks = (n + 255u) / 256u;
    if (math) hipLaunchKernelGGL(k_env_debug<2>, dim3(blocks), dim3(256), 0, stream, m, op, d_in, n, d_out);
    else hipLaunchKernelGGL(k_env_debug<0>, dim3(blocks), dim3(256), 0, stream, m, op, d_in, n, d_out);
    return hipGetLastError();
}

void env_free(EnvDevice& e)
{
    if (e.texels) (void)hipFree(e.texels);
    if (e.marginal) (void)hipFree(e.marginal);
    if (e.conditional) (void)hipFree(e.conditional);
    e = EnvDevice();
}

#define ENV_CK(x) do { const hipError_t rc_ = (x); if (rc_ != hipSuccess) { err = std::string("pt_set_environment: ") + #x + ": " + hipGetErrorString(rc_); goto fail; } } while (0)
bool env_upload(EnvDevice& e, const float4* h_rgba, uint32_t w, uint32_t h, hipStream_t stream, std::string& err)
{
    EnvDevice n;
    n.w = w; n.h = h;
    float* d_sin = nullptr;
    float* d_rows = nullptr;
    const size_t texels = (size_t)w * h;
    std::vector<float> row_sin(h);
    for (uint32_t r = 0; r < h; r++) row_sin[r] = (float)std::sin(M_PI * ((double)r + 0.5) / (double)h);     // the same table as tests/env_ref.py
    ENV_CK(hipMalloc((void**)&n.texels, texels * sizeof(float4)));
    ENV_CK(hipMalloc((void**)&n.conditional, texels * sizeof(float)));
    ENV_CK(hipMalloc((void**)&n.marginal, (size_t)h * sizeof(float)));
    ENV_CK(hipMalloc((void**)&d_sin, (size_t)h * sizeof(float)));
    ENV_CK(hipMalloc((void**)&d_rows, ((size_t)h + 1u) * sizeof(float)));
    ENV_CK(hipMemcpyAsync(n.texels, h_rgba, texels * sizeof(float4), hipMemcpyHostToDevice, stream));
    ENV_CK(hipMemcpyAsync(d_sin, row_sin.data(), (size_t)h * sizeof(float), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_env_rows, dim3(h), dim3(kEnvThreads), 0, stream, n.texels, (const float*)d_sin, n.conditional, d_rows, w);
    ENV_CK(hipGetLastError());
    hipLaunchKernelGGL(k_env_marginal, dim3(1), dim3(kEnvThreads), 0, stream, (const float*)d_rows, n.marginal, h, d_rows + h);
    ENV_CK(hipGetLastError());
    ENV_CK(hipMemcpyAsync(&n.total, d_rows + h, sizeof(float), hipMemcpyDeviceToHost, stream));
    ENV_CK(hipStreamSynchronize(stream));
    (void)hipFree(d_sin); (void)hipFree(d_rows);
    n.pdf_scale = n.total > 0.0f ? (float)((double)w * (double)h / (2.0 * M_PI * M_PI * (double)n.total)) : 0.0f;
    if (!std::isfinite(n.pdf_scale)) n.pdf_scale = 0.0f;
    env_free(e);
    e = n;
    return true;
fail:
    if (d_sin) (void)hipFree(d_sin);
    if (d_rows) (void)hipFree(d_rows);
    env_free(n);
    return false;
}

}  // namespace ptd
