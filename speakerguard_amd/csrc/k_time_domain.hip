// Time-domain input defenses (reference defense/time_domain.py), both directions, on (B,T) float32 waveforms, one utterance
// per row: quantisation QT (:10-44; BDR :46-48 is QT with q = 2^(bits - param)), additive noise AT (:50-70), average
// smoothing AS (:72-97), median smoothing MS (:100-127).  All memory-bound, one pass over the row each.
//
// Determinism contract: every output value is computed by ONE fixed sequence of float32 operations that does
// not depend on B, on how a batch is cut into calls, or on the launch geometry.  tests/time_domain_restate.py restates the
// sequences below in numpy, operation for operation.
//
//   QT  fwd  out = rint(x*s / q) * q / s;  s = 32768 or 1 from the WHOLE CALL's max / min (sg_input_scale: the reference
//            takes the decision per call, time_domain.py:31); rint = round half to even (torch.round); both divisions are
//            correctly rounded IEEE divisions (__fdiv_rn).
//       bwd  identity (BPDA, :44).
//   AS  fwd  out[t] = fmaf chain over the taps j = 0 .. k-1 in order, from 0: acc = fmaf(w, xpad[t + j - h], acc),
//            w = float32(1 / k), h = (k-1)/2, zero padding.
//       bwd  the operator is symmetric under zero padding: gx[i] = sum_j w g[i - j + h] = sum_j' w gpad[i + j' - h] with
//            j' = k-1-j, so gx = AS(g), THE SAME KERNEL -- no second one.  (Its chain runs over the exact adjoint's taps in
//            mirrored order; all weights are equal, so the two differ by the order of k additions only.)
//   MS  fwd  window = xpad[t - h .. t + h]; out[t] = the element of rank h under the order (value, window position); the pad
//            zeros take part with their positions.  sel[t] (int8) = its window position - h.  Rank counting: k^2 compares
//            per output, no branches, the row tile with its halo in LDS.
//       bwd  gx[i] = sum over t = i-h .. i+h (ascending, inside the row) of (sel[t] == i - t ? g[t] : 0), from 0: a gather,
//            no atomics.  A cotangent whose selected element is a pad zero is dropped.
//   AT  fwd  c = float32(1 / sqrt(T)) (host, double arithmetic rounded once); v = x*c; P[b] = sum v*v in the tree below;
//            sigma[b] = sqrt(P[b] / snr) (both correctly rounded), snr = float32(10^(param/10)); out = fmaf(n, sigma[b], x).
//       bwd  dot[b] = sum g*n in the same tree; coef[b] = P[b] == 0 ? 0 : dot[b] / ((float(T) * snr) * sigma[b]);
//            gx = fmaf(x, coef[b], g).  Exact autograd of the reference (the noise power depends on x), except for a silent
//            utterance (P == 0): the reference's gradient is 0/0 = NaN there, ours defines the second term as 0.
//       tree thread j of 1024 adds its terms i = j, j + 1024, ... in ascending order (acc = acc + term, from 0), the 64
//            lanes of a wave combine by v += shfl_xor(v, o) for o = 32, 16, .. 1, and the 16 wave sums are added in wave
//            order.  A function of T only.
//       noise  an explicit (B,T) tensor, or unit normals regenerated (never stored) from Philox4x32-10 (philox.h):
//            for row b:  g = row_base + b, repeat = rep_rows > 0 ? g / rep_rows : 0, key = seed + repeat * 0xC2B2AE3D27D4EB4F,
//            utterance = index_base + (g - repeat * rep_rows)                       (exactly sg_dither's derivation)
//            (w0, w1) = first two words of philox(key, counter = (sample t, kAtDomain, utterance lo, utterance hi))
//            u_i = ((w_i >> 8) + 0.5) / 2^24;  n = sqrt(-2 ln u_0) * cos(2 pi u_1)   (Box-Muller, like nes_normal)
//            kAtDomain = 0xA7000000 in counter word 1: the dither's counters carry the FRAME there (< 2^31 / 160) and
//            the NES queries the antithetic pair index, so the three streams never share a counter even under one key.
#include <cmath>
#include <cstdio>

#include "philox.h"
#include "wave_reduce.h"
#include "sg_internal.h"

// every sequence above names its roundings: nothing may be contracted behind its back (the chains use fmaf explicitly)
#pragma clang fp contract(off)

using namespace sg;

namespace {

constexpr int kTdBlock = 256;     // samples (= threads) per block of the elementwise / windowed kernels
constexpr int kTdMaxK = 31;       // largest window
constexpr int kTdHalo = (kTdMaxK - 1) / 2;
constexpr int kTdRowThreads = 1024;  // the per-utterance reductions: a constant of the ARITHMETIC (the tree above)
constexpr uint32_t kAtDomain = 0xA7000000u;

// ---------------------------------------------------------------- QT / BDR
__global__ __launch_bounds__(kTdBlock) void td_qt_kernel(const float* __restrict__ x, const float* __restrict__ scale_p, float q,
                                                         float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (i >= n) return;
    const float s = *scale_p;
    const float v = rintf(__fdiv_rn(x[i] * s, q)) * q;
    out[i] = s != 1.f ? __fdiv_rn(v, s) : v;  // (time_domain.py:39-40: the division happens only when the input was scaled)
}

// ---------------------------------------------------------------- row tile with halo
// tile[i] = xpad[t0 - kTdHalo + i] for i < kTdBlock + 2 kTdHalo (zero outside the row)
__device__ __forceinline__ void td_load_tile(const float* __restrict__ row, int T, int t0, float* tile) {
    for (int i = threadIdx.x; i < kTdBlock + 2 * kTdHalo; i += kTdBlock) {
        const int t = t0 - kTdHalo + i;
        tile[i] = (t >= 0 && t < T) ? row[t] : 0.f;
    }
    __syncthreads();
}

// ---------------------------------------------------------------- AS (forward and, the operator being symmetric, backward)
__global__ __launch_bounds__(kTdBlock) void td_as_kernel(const float* __restrict__ x, int T, int k, float w,
                                                         float* __restrict__ out) {
    __shared__ float tile[kTdBlock + 2 * kTdHalo];
    const size_t base = (size_t)blockIdx.y * T;
    const int t0 = blockIdx.x * kTdBlock;
    td_load_tile(x + base, T, t0, tile);
    const int t = t0 + threadIdx.x;
    if (t >= T) return;
    const int h = (k - 1) / 2;
    const float* win = tile + kTdHalo + threadIdx.x - h;
    float acc = 0.f;
    for (int j = 0; j < k; ++j) acc = fmaf(w, win[j], acc);
    out[base + t] = acc;
}

// ---------------------------------------------------------------- MS
__global__ __launch_bounds__(kTdBlock) void td_ms_fwd_kernel(const float* __restrict__ x, int T, int k, float* __restrict__ out,
                                                             int8_t* __restrict__ sel) {
    __shared__ float tile[kTdBlock + 2 * kTdHalo];
    const size_t base = (size_t)blockIdx.y * T;
    const int t0 = blockIdx.x * kTdBlock;
    td_load_tile(x + base, T, t0, tile);
    const int t = t0 + threadIdx.x;
    if (t >= T) return;
    const int h = (k - 1) / 2;
    const float* win = tile + kTdHalo + threadIdx.x - h;
    // rank of window entry p = entries before it in the order (value, position); exactly one entry has rank h
    float val = win[h];
    int pos = h;
    for (int p = 0; p < k; ++p) {
        const float vp = win[p];
        int rank = 0;
        for (int q = 0; q < k; ++q) {
            const float vq = win[q];
            rank += (int)((vq < vp) | ((vq == vp) & (q < p)));
        }
        const bool hit = rank == h;
        val = hit ? vp : val;
        pos = hit ? p : pos;
    }
    out[base + t] = val;
    sel[base + t] = (int8_t)(pos - h);
}

__global__ __launch_bounds__(kTdBlock) void td_ms_bwd_kernel(const float* __restrict__ g, const int8_t* __restrict__ sel, int T, int k,
                                                             float* __restrict__ gx) {
    const size_t base = (size_t)blockIdx.y * T;
    const int i = blockIdx.x * kTdBlock + threadIdx.x;
    if (i >= T) return;
    const int h = (k - 1) / 2;
    const int lo = i - h < 0 ? 0 : i - h, hi = i + h > T - 1 ? T - 1 : i + h;
    float acc = 0.f;
    for (int t = lo; t <= hi; ++t) acc = acc + ((int)sel[base + t] == i - t ? g[base + t] : 0.f);
    gx[base + i] = acc;
}

// ---------------------------------------------------------------- AT
__device__ __forceinline__ float at_normal(uint64_t key, int64_t utt, int t) {
    uint32_t w1;
    const uint32_t w0 = philox4x32_10_w01(key, (uint32_t)t, kAtDomain, (uint32_t)utt, (uint32_t)((uint64_t)utt >> 32), &w1);
    const float u0 = philox_unit24(w0);
    const float u1 = philox_unit24(w1);
    return sqrtf(-2.f * logf(u0)) * cosf(6.283185307179586f * u1);
}

struct AtNoise {
    const float* given;  // explicit (B,T) noise or null
    uint64_t seed;
    int64_t index_base, row_base;
    int rep_rows;
};
// (key, utterance) of row b: sg_dither's derivation, as noise_row_key of philox.h (kept in this form: these kernels were
// compiled from it, and the shared function's statement order schedules them differently)
__device__ __forceinline__ void at_row_key(const AtNoise& nz, int b, uint64_t* key, int64_t* utt) {
    const int64_t g = nz.row_base + b;
    const int64_t rep = nz.rep_rows > 0 ? g / nz.rep_rows : 0;
    *key = nz.seed + (uint64_t)rep * kRepKey;
    *utt = nz.index_base + (g - rep * nz.rep_rows);
}

// saved[b] = sigma[b], saved[B + b] = P[b]; one block per utterance
__global__ __launch_bounds__(kTdRowThreads) void td_at_power_kernel(const float* __restrict__ x, int B, int T, float c, float snr,
                                                                    float* __restrict__ saved) {
    __shared__ float red[kTdRowThreads / 64];
    const int b = blockIdx.x;
    const float* row = x + (size_t)b * T;
    float acc = 0.f;
    for (int i = threadIdx.x; i < T; i += kTdRowThreads) {
        const float v = row[i] * c;
        acc = acc + v * v;
    }
    const float P = block_reduce_xor<kTdRowThreads / 64, false>(acc, red, OpSum());
    if (threadIdx.x == 0) {
        saved[b] = sqrtf(__fdiv_rn(P, snr));  // (sqrtf is the correctly rounded one here; __fsqrt_rn compiles to the bare 1-ulp instruction)
        saved[B + b] = P;
    }
}

__global__ __launch_bounds__(kTdBlock) void td_at_fwd_kernel(const float* __restrict__ x, int T, AtNoise nz,
                                                             const float* __restrict__ saved, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * kTdBlock + threadIdx.x;
    if (t >= T) return;
    const size_t o = (size_t)b * T + t;
    float n;
    if (nz.given) {
        n = nz.given[o];
    } else {
        uint64_t key;
        int64_t utt;
        at_row_key(nz, b, &key, &utt);
        n = at_normal(key, utt, t);
    }
    out[o] = fmaf(n, saved[b], x[o]);
}

// saved[2 B + b] = coef[b] (workspace of the backward); one block per utterance
__global__ __launch_bounds__(kTdRowThreads) void td_at_dot_kernel(const float* __restrict__ g, int B, int T, AtNoise nz, float snr,
                                                                  float* __restrict__ saved) {
    __shared__ float red[kTdRowThreads / 64];
    const int b = blockIdx.x;
    const size_t base = (size_t)b * T;
    uint64_t key;
    int64_t utt;
    at_row_key(nz, b, &key, &utt);
    float acc = 0.f;
    for (int i = threadIdx.x; i < T; i += kTdRowThreads) {
        const float n = nz.given ? nz.given[base + i] : at_normal(key, utt, i);
        acc = acc + g[base + i] * n;
    }
    const float dot = block_reduce_xor<kTdRowThreads / 64, false>(acc, red, OpSum());
    if (threadIdx.x == 0) {
        const float sigma = saved[b], P = saved[B + b];
        saved[2 * B + b] = P == 0.f ? 0.f : __fdiv_rn(dot, ((float)T * snr) * sigma);
    }
}

__global__ __launch_bounds__(kTdBlock) void td_at_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, int B, int T,
                                                             const float* __restrict__ saved, float* __restrict__ gx) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * kTdBlock + threadIdx.x;
    if (t >= T) return;
    const size_t o = (size_t)b * T + t;
    gx[o] = fmaf(x[o], saved[2 * B + b], g[o]);
}

// ---------------------------------------------------------------- argument checks shared by both directions
// window length of AS / MS from the float parameter, 0 if it is not an odd integer in [1, 31]
int td_window(float param) {
    const int k = (int)param;
    return ((float)k == param && k >= 1 && k <= kTdMaxK && (k & 1)) ? k : 0;
}

// what a spec alone can get wrong (both directions, and the defended loop before its first launch)
int td_check_spec(sg_ctx* ctx, const char* who, const sg_wav_defense* d) {
    switch (d->kind) {
    case SG_TD_QT:
        if (!(d->param > 0.f) || !std::isfinite(d->param)) return fail(ctx, SG_ERR_ARG, "%s: QT needs a finite q > 0 (%g)", who, d->param);
        break;
    case SG_TD_AS:
    case SG_TD_MS:
        if (!td_window(d->param)) return fail(ctx, SG_ERR_ARG, "%s: the window must be odd, 1 <= k <= %d (%g)", who, kTdMaxK, d->param);
        break;
    case SG_TD_AT:
        if (!std::isfinite(d->param)) return fail(ctx, SG_ERR_ARG, "%s: AT needs a finite SNR in dB (%g)", who, d->param);
        if (d->rep_rows < 0 || d->row_base < 0) return fail(ctx, SG_ERR_ARG, "%s: row_base and rep_rows must not be negative", who);
        break;
    default:
        return fail(ctx, SG_ERR_ARG, "%s: unknown kind %d", who, d->kind);
    }
    return SG_OK;
}

int td_check(sg_ctx* ctx, const char* who, const sg_wav_defense* d, const void* a, const void* b, int32_t B, int32_t T) {
    if (!ctx) return SG_ERR_ARG;
    if (!d || !a || !b) return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    if (B < 1 || B > 65535 || T < 1) return fail(ctx, SG_ERR_ARG, "%s: need 1 <= B <= 65535 and T >= 1 (B %d, T %d)", who, B, T);
    if (int rc = td_check_spec(ctx, who, d)) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    return SG_OK;
}

inline float at_snr(float param_db) { return (float)std::pow(10.0, (double)param_db / 10.0); }
inline AtNoise at_noise(const sg_wav_defense* d) { return AtNoise{d->noise_dev, d->seed, d->index_base, d->row_base, d->rep_rows}; }

}  // namespace

int sg::wav_defense_check_spec(sg_ctx* ctx, const char* who, const sg_wav_defense* d) { return td_check_spec(ctx, who, d); }

extern "C" int sg_wav_defense_forward(sg_ctx* ctx, const sg_wav_defense* d, const float* x_dev, int32_t B, int32_t T,
                                      float* out_dev, void* saved_dev, void* stream) {
    int rc = td_check(ctx, "sg_wav_defense_forward", d, x_dev, out_dev, B, T);
    if (rc) return rc;
    if (d->kind != SG_TD_AS && !saved_dev) return fail(ctx, SG_ERR_ARG, "sg_wav_defense_forward: this kind needs saved_dev");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((T + kTdBlock - 1) / kTdBlock, B);
    trace_mark(ctx, SG_STAGE_TD_FWD, s, 0);
    switch (d->kind) {
    case SG_TD_QT: {
        const int64_t n = (int64_t)B * T;
        hipLaunchKernelGGL(td_qt_kernel, dim3((unsigned)((n + kTdBlock - 1) / kTdBlock)), dim3(kTdBlock), 0, s, x_dev,
                           static_cast<const float*>(saved_dev), d->param, out_dev, n);
        break;
    }
    case SG_TD_AS: {
        const int k = td_window(d->param);
        hipLaunchKernelGGL(td_as_kernel, grid, dim3(kTdBlock), 0, s, x_dev, T, k, (float)(1.0 / k), out_dev);
        break;
    }
    case SG_TD_MS:
        hipLaunchKernelGGL(td_ms_fwd_kernel, grid, dim3(kTdBlock), 0, s, x_dev, T, td_window(d->param), out_dev,
                           static_cast<int8_t*>(saved_dev));
        break;
    default: {  // SG_TD_AT
        float* saved = static_cast<float*>(saved_dev);
        hipLaunchKernelGGL(td_at_power_kernel, dim3(B), dim3(kTdRowThreads), 0, s, x_dev, B, T, (float)(1.0 / std::sqrt((double)T)),
                           at_snr(d->param), saved);
        hipLaunchKernelGGL(td_at_fwd_kernel, grid, dim3(kTdBlock), 0, s, x_dev, T, at_noise(d), saved, out_dev);
        break;
    }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_wav_defense_forward: %s", hipGetErrorString(e));
    trace_mark(ctx, SG_STAGE_TD_FWD, s, 1);
    return SG_OK;
}

extern "C" int sg_wav_defense_backward(sg_ctx* ctx, const sg_wav_defense* d, const float* x_dev, const float* g_dev,
                                       void* saved_dev, int32_t B, int32_t T, float* gx_dev, void* stream) {
    int rc = td_check(ctx, "sg_wav_defense_backward", d, g_dev, gx_dev, B, T);
    if (rc) return rc;
    if ((d->kind == SG_TD_MS || d->kind == SG_TD_AT) && !saved_dev)
        return fail(ctx, SG_ERR_ARG, "sg_wav_defense_backward: this kind needs the forward's saved_dev");
    if (d->kind == SG_TD_AT && !x_dev) return fail(ctx, SG_ERR_ARG, "sg_wav_defense_backward: AT needs the forward's input");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((T + kTdBlock - 1) / kTdBlock, B);
    trace_mark(ctx, SG_STAGE_TD_BWD, s, 0);
    hipError_t e = hipSuccess;
    switch (d->kind) {
    case SG_TD_QT:  // BPDA's identity substitute: a caller that can alias the two launches nothing (defense.time_domain.QT)
        if (gx_dev != g_dev) e = hipMemcpyAsync(gx_dev, g_dev, (size_t)B * T * sizeof(float), hipMemcpyDeviceToDevice, s);
        break;
    case SG_TD_AS: {  // symmetric operator: the forward kernel is its own adjoint (header)
        const int k = td_window(d->param);
        hipLaunchKernelGGL(td_as_kernel, grid, dim3(kTdBlock), 0, s, g_dev, T, k, (float)(1.0 / k), gx_dev);
        break;
    }
    case SG_TD_MS:
        hipLaunchKernelGGL(td_ms_bwd_kernel, grid, dim3(kTdBlock), 0, s, g_dev, static_cast<const int8_t*>(saved_dev), T,
                           td_window(d->param), gx_dev);
        break;
    default: {  // SG_TD_AT
        float* saved = static_cast<float*>(saved_dev);
        hipLaunchKernelGGL(td_at_dot_kernel, dim3(B), dim3(kTdRowThreads), 0, s, g_dev, B, T, at_noise(d), at_snr(d->param), saved);
        hipLaunchKernelGGL(td_at_bwd_kernel, grid, dim3(kTdBlock), 0, s, x_dev, g_dev, B, T, saved, gx_dev);
        break;
    }
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_wav_defense_backward: %s", hipGetErrorString(e));
    trace_mark(ctx, SG_STAGE_TD_BWD, s, 1);
    return SG_OK;
}
