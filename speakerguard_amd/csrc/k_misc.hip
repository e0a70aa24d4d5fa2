// Small memory-bound kernels around the TDNN contractions: input range check, CMVN, statistics
// pooling (+backward), the fused PGD update.
#include "sg_internal.h"
#include "wave_reduce.h"

namespace sg {

// ---------------------------------------------------------------- check_input_range (model/utils.py:7-19)
// range_type='origin' (xv_plda.py:48): if 0.9*max <= 1 and 0.9*min >= -1 the batch is in the
// [-1,1] float domain and is multiplied by 2^15, otherwise it is left alone.  Single block; the
// result stays on the device so no host sync is needed.  Two stages: 256 blocks -> partial max/min,
// one block -> the decision (a single-block version cost 0.86 ms at 64 x 3 s, 11 % of a PGD step).
constexpr int kScaleBlocks = 256;

// (round 5: 16-byte loads, four of them in flight per thread, 1024 threads per block -- the one-float-per-iteration loop of
// 256-thread blocks ran at 0.8 TB/s: 121 us for the 98 MB of 512 utterances, three times per attack.  max / min do not
// depend on the order.)
constexpr int kScaleThreads = 1024;
__global__ __launch_bounds__(kScaleThreads) void input_range_partial_kernel(const float* __restrict__ x, int64_t n,
                                                                            float* __restrict__ part) {
    __shared__ float smax[kScaleThreads / 64], smin[kScaleThreads / 64];
    float mx = -INFINITY, mn = INFINITY;
    const int64_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n / 4 : 0;  // whole float4s (an unaligned row: one by one)
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const int64_t stride = (int64_t)kScaleBlocks * kScaleThreads;
    int64_t i = (int64_t)blockIdx.x * kScaleThreads + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const float4 a = x4[i], b = x4[i + stride], c = x4[i + 2 * stride], d = x4[i + 3 * stride];
        mx = fmaxf(fmaxf(fmaxf(mx, fmaxf(a.x, a.y)), fmaxf(fmaxf(a.z, a.w), fmaxf(b.x, b.y))),
                   fmaxf(fmaxf(fmaxf(b.z, b.w), fmaxf(c.x, c.y)), fmaxf(fmaxf(c.z, c.w), fmaxf(fmaxf(d.x, d.y), fmaxf(d.z, d.w)))));
        mn = fminf(fminf(fminf(mn, fminf(a.x, a.y)), fminf(fminf(a.z, a.w), fminf(b.x, b.y))),
                   fminf(fminf(fminf(b.z, b.w), fminf(c.x, c.y)), fminf(fminf(c.z, c.w), fminf(fminf(d.x, d.y), fminf(d.z, d.w)))));
    }
    for (; i < n4; i += stride) {
        const float4 a = x4[i];
        mx = fmaxf(mx, fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)));
        mn = fminf(mn, fminf(fminf(a.x, a.y), fminf(a.z, a.w)));
    }
    for (int64_t j = 4 * n4 + (int64_t)blockIdx.x * kScaleThreads + threadIdx.x; j < n; j += stride) {
        const float v = x[j];
        mx = fmaxf(mx, v);
        mn = fminf(mn, v);
    }
    mx = wave_max_xor(mx);
    mn = wave_min_xor(mn);
    if ((threadIdx.x & 63) == 0) {
        smax[threadIdx.x >> 6] = mx;
        smin[threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kScaleThreads / 64; ++w) {
            mx = fmaxf(mx, smax[w]);
            mn = fminf(mn, smin[w]);
        }
        part[blockIdx.x] = mx;
        part[kScaleBlocks + blockIdx.x] = mn;
    }
}

__global__ __launch_bounds__(256) void input_range_final_kernel(const float* __restrict__ part, float* scale, int mode) {
    __shared__ float smax[4], smin[4];
    float mx = wave_max_xor(part[threadIdx.x]);
    float mn = wave_min_xor(part[kScaleBlocks + threadIdx.x]);
    if ((threadIdx.x & 63) == 0) {
        smax[threadIdx.x >> 6] = mx;
        smin[threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
        mn = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        const bool unit = 0.9f * mx <= 1.f && 0.9f * mn >= -1.f;  // ori_type == 'scale'
        *scale = mode == 0 ? (unit ? 32768.f : 1.f) : (unit ? 1.f : 1.f / 32768.f);
    }
}

hipError_t launch_input_scale(const float* x, int64_t n, float* scratch, float* scale, int mode, hipStream_t s) {
    hipLaunchKernelGGL(input_range_partial_kernel, dim3(kScaleBlocks), dim3(kScaleThreads), 0, s, x, n, scratch);
    hipLaunchKernelGGL(input_range_final_kernel, dim3(1), dim3(256), 0, s, scratch, scale, mode);
    return hipGetLastError();
}

// ---------------------------------------------------------------- PGD update (attack/FGSM.py:65,68)
__global__ __launch_bounds__(256) void pgd_update_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                         const float* __restrict__ lo, const float* __restrict__ hi,
                                                         int64_t n, float step, int grad_sign, int vec) {
    const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (vec && i4 + 3 < n) {
        float4 xv = *reinterpret_cast<float4*>(x + i4);
        const float4 gv = *reinterpret_cast<const float4*>(g + i4);
        const float4 lv = *reinterpret_cast<const float4*>(lo + i4);
        const float4 hv = *reinterpret_cast<const float4*>(hi + i4);
        const float s = step * (float)grad_sign;
#define SG_UPD(c) xv.c = fminf(fmaxf(xv.c + s * (gv.c > 0.f ? 1.f : (gv.c < 0.f ? -1.f : 0.f)), lv.c), hv.c)
        SG_UPD(x); SG_UPD(y); SG_UPD(z); SG_UPD(w);
#undef SG_UPD
        *reinterpret_cast<float4*>(x + i4) = xv;
    } else {
        // the row's tail, or (vec == 0: a base off a 16-byte boundary) this thread's four; step * +-1 is exact: same bits as above
        const int64_t e = i4 + 4 < n ? i4 + 4 : n;
        for (int64_t i = i4; i < e; ++i) {
            const float gv = g[i];
            const float sg = gv > 0.f ? 1.f : (gv < 0.f ? -1.f : 0.f);
            x[i] = fminf(fmaxf(x[i] + step * (float)grad_sign * sg, lo[i]), hi[i]);
        }
    }
}

hipError_t launch_pgd_update(float* x, const float* g, const float* lo, const float* hi, int64_t n, float step,
                             int grad_sign, hipStream_t s) {
    const int64_t blocks = (n + 1023) / 1024;
    // the C-ABI asks for no alignment of a caller's buffer (a row slice of a batch of odd length): 16-byte accesses only when
    // all four bases allow them
    const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(lo) |
                      reinterpret_cast<uintptr_t>(hi)) & 15) == 0;
    hipLaunchKernelGGL(pgd_update_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, g, lo, hi, n, step, grad_sign, vec);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void copy_cols_kernel(const float* __restrict__ in, int ld_in, float* __restrict__ out,
                                                        int ld_out, int64_t rows, int ncol) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * ld_out) return;
    const int64_t r = i / ld_out;
    const int c = (int)(i - r * ld_out);
    out[i] = c < ncol ? in[r * ld_in + c] : 0.f;
}

hipError_t launch_copy_cols(const float* in, int ld_in, float* out, int ld_out, int64_t rows, int ncol, hipStream_t s) {
    const int64_t n = rows * ld_out;
    hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, ld_in, out, ld_out, rows,
                       ncol);
    return hipGetLastError();
}

// out[r][0..ncol) = sum_z in[z][r][0..ncol)  (split-K slabs, fixed order)
__global__ __launch_bounds__(256) void sum_cols_kernel(const float* __restrict__ in, int ld_in, int nsplit,
                                                       long long slab_stride, float* __restrict__ out, int ld_out,
                                                       int64_t rows, int ncol) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * ncol) return;
    const int64_t r = i / ncol;
    const int c = (int)(i - r * ncol);
    float v = 0.f;
    for (int z = 0; z < nsplit; ++z) v += in[(size_t)z * slab_stride + r * ld_in + c];
    out[r * ld_out + c] = v;
}

hipError_t launch_sum_cols(const float* in, int ld_in, int nsplit, long long slab_stride, float* out, int ld_out,
                           int64_t rows, int ncol, hipStream_t s) {
    const int64_t n = rows * ncol;
    hipLaunchKernelGGL(sum_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, ld_in, nsplit, slab_stride,
                       out, ld_out, rows, ncol);
    return hipGetLastError();
}

// ---------------------------------------------------------------- CMVN (model/iv_plda.py:296-377)
// Centred sliding window of 300 frames, mean only.  window(t) = [start, end) as at :321-336.
__device__ __forceinline__ void cmvn_window(int t, int F, int& start, int& end) {
    start = t - kCmnWindow / 2;
    end = start + kCmnWindow;
    if (start < 0) {
        end -= start;
        start = 0;
    }
    if (end > F) {
        start -= end - F;
        end = F;
        if (start < 0) start = 0;
    }
}

// grid (B), block 1024.  out row stride ld_out >= 30; columns 30..ld_out-1 are zeroed (GEMM K pad).
// One block per utterance is all the parallelism there is (64 blocks at B = 64), so the kernels are latency
// bound: 1024 threads and 32 row-strided partial sums per column keep 4x more loads in flight than the first
// version (256 threads, 8 partials: 23 us per launch for 2.3 MB).
constexpr int kCmvnThreads = 1024;
constexpr int kCmvnParts = kCmvnThreads / 32;
__global__ __launch_bounds__(kCmvnThreads) void cmvn_fwd_kernel(const float* __restrict__ in, int ld_in, float* __restrict__ out,
                                                       int ld_out, int F) {
    const int b = blockIdx.x;
    const float* x = in + (size_t)b * F * ld_in;
    float* y = out + (size_t)b * F * ld_out;
#define SG_MISC_BODY 1
#include "k_misc_bodies.h"
}

// A batch of unequal lengths (RowLens, sg_internal.h): rows Fld frames apart, row b normalised over its own F frames -- window,
// mean and the branch on kCmnWindow as for that utterance alone; the rows behind them are written as zeros, all ld_out columns.
__global__ __launch_bounds__(kCmvnThreads) void cmvn_fwd_ragged_kernel(const float* __restrict__ in, int ld_in, float* __restrict__ out,
                                                              int ld_out, int Fld, const int32_t* __restrict__ lens, int nlen, int T) {
    const int b = blockIdx.x;
    const int F = num_frames(row_samples(lens, nlen, b, T));
    const float* x = in + (size_t)b * Fld * ld_in;
    float* y = out + (size_t)b * Fld * ld_out;
#define SG_MISC_BODY 1
#include "k_misc_bodies.h"
    for (int i = F * ld_out + threadIdx.x; i < Fld * ld_out; i += kCmvnThreads) y[i] = 0.f;
}

// d_in[u] = d_out[u] - sum_{t : u in window(t)} d_out[t] / |window(t)|
// d_out arrives as `nsplit` split-K slabs of the tdnn1 data-gradient contraction (summed in order).
// NS > 0: the slab count as a compile-time constant (the attack loop's kL1BwdSplitK): the slab loads of a row are then one
// batch of independent loads instead of two dependent ones.
template <int NS>
__global__ __launch_bounds__(kCmvnThreads) void cmvn_bwd_kernel(const float* __restrict__ dout, int ld_dout, int nsplit_rt,
                                                       long long slab_stride, float* __restrict__ din, int ld_din,
                                                       int F) {
    const int b = blockIdx.x;
    const float* g = dout + (size_t)b * F * ld_dout;
    float* y = din + (size_t)b * F * ld_din;
#define SG_MISC_BODY 2
#include "k_misc_bodies.h"
}

// ... of a batch of unequal lengths (cmvn_fwd_ragged_kernel): row b over its own F frames, +0 behind them
template <int NS>
__global__ __launch_bounds__(kCmvnThreads) void cmvn_bwd_ragged_kernel(const float* __restrict__ dout, int ld_dout, int nsplit_rt,
                                                              long long slab_stride, float* __restrict__ din, int ld_din, int Fld,
                                                              const int32_t* __restrict__ lens, int nlen, int T) {
    const int b = blockIdx.x;
    const int F = num_frames(row_samples(lens, nlen, b, T));
    const float* g = dout + (size_t)b * Fld * ld_dout;
    float* y = din + (size_t)b * Fld * ld_din;
#define SG_MISC_BODY 2
#include "k_misc_bodies.h"
    for (int i = F * ld_din + threadIdx.x; i < Fld * ld_din; i += kCmvnThreads) y[i] = 0.f;
}

// rl.dev: a batch of unequal lengths, T its row stride in samples (F = num_frames(T))
hipError_t launch_cmvn_fwd(const float* in, int ld_in, float* out, int ld_out, int B, int F, hipStream_t s, const RowLens& rl, int T) {
    if (rl.dev) hipLaunchKernelGGL(cmvn_fwd_ragged_kernel, dim3(B), dim3(kCmvnThreads), 0, s, in, ld_in, out, ld_out, F, rl.dev, rl.n, T);
    else hipLaunchKernelGGL(cmvn_fwd_kernel, dim3(B), dim3(kCmvnThreads), 0, s, in, ld_in, out, ld_out, F);
    return hipGetLastError();
}
hipError_t launch_cmvn_bwd(const float* dout, int ld_dout, int nsplit, long long slab_stride, float* din, int ld_din,
                           int B, int F, hipStream_t s, const RowLens& rl, int T) {
    if (rl.dev && nsplit == kL1BwdSplitK)
        hipLaunchKernelGGL(cmvn_bwd_ragged_kernel<kL1BwdSplitK>, dim3(B), dim3(kCmvnThreads), 0, s, dout, ld_dout, nsplit, slab_stride, din,
                           ld_din, F, rl.dev, rl.n, T);
    else if (rl.dev)
        hipLaunchKernelGGL(cmvn_bwd_ragged_kernel<0>, dim3(B), dim3(kCmvnThreads), 0, s, dout, ld_dout, nsplit, slab_stride, din, ld_din, F,
                           rl.dev, rl.n, T);
    else if (nsplit == kL1BwdSplitK)
        hipLaunchKernelGGL(cmvn_bwd_kernel<kL1BwdSplitK>, dim3(B), dim3(kCmvnThreads), 0, s, dout, ld_dout, nsplit, slab_stride, din, ld_din, F);
    else
        hipLaunchKernelGGL(cmvn_bwd_kernel<0>, dim3(B), dim3(kCmvnThreads), 0, s, dout, ld_dout, nsplit, slab_stride, din, ld_din, F);
    return hipGetLastError();
}

// ---------------------------------------------------------------- statistics pooling (xvecTDNN.py:62)
// stats = cat(mean_t, std_t (unbiased)) over the tdnn5 relu output (BatchNorm folded into fc1).
// grid (kPoolC/64, B), block 256: lane = channel, the 4 waves split the frames.
__global__ __launch_bounds__(256) void pool_fwd_kernel(const float* __restrict__ act, int Tc, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
    const float* a = act + (size_t)b * Tc * kPoolC + c;
#define SG_MISC_BODY 3
#include "k_misc_bodies.h"
}

// A batch of unequal lengths (RowLens, sg_internal.h): rows Tld frames apart, row b pooled over its own Tc frames, kTdnnContext
// fewer than its MFCC has -- the sums in the order, and on the branch, of that utterance alone.
__global__ __launch_bounds__(256) void pool_fwd_ragged_kernel(const float* __restrict__ act, int Tld, float* __restrict__ stats,
                                                              const int32_t* __restrict__ lens, int nlen, int T) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
    const int Tc = min(num_frames(row_samples(lens, nlen, b, T)) - kTdnnContext, Tld);
    const float* a = act + (size_t)b * Tld * kPoolC + c;
#define SG_MISC_BODY 3
#include "k_misc_bodies.h"
}

// d act[t][c] = relu'(act) * ( dmean[c]/T + dstd[c] * (act - mean) / ((T-1) * std) ), std == 0 -> no std term
// (torch std_backward masks result == 0).  dstats arrives as `nsplit` split-K partials.
// NS > 0: the slab count at compile time (kFc1BwdSplitK): all 2 NS loads of the slab sums in flight at once.
template <int NS>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ act, const float* __restrict__ stats,
                                                       const float* __restrict__ dpart, int nsplit, int B, int Tc,
                                                       float* __restrict__ dact) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
#define SG_MISC_BODY 4
#include "k_misc_bodies.h"
    const float* a = act + (size_t)b * Tc * kPoolC + c;
    float* d = dact + (size_t)b * Tc * kPoolC + c;
    // elementwise from here on: the frames are dealt over the blocks of grid.z (small batches: 24 x 8 blocks of a 68-step
    // loop left most CUs idle, 15 us at 8 utterances) -- any split gives the same bits
    const int per = (Tc + (int)gridDim.z - 1) / (int)gridDim.z;
    const int t0 = (int)blockIdx.z * per, t1 = min(Tc, t0 + per);
    for (int t = t0 + wid; t < t1; t += 4) {
        const float v = a[(size_t)t * kPoolC];
        d[(size_t)t * kPoolC] = v > 0.f ? alpha + beta * (v - mean) : 0.f;
    }
}

// ... of a batch of unequal lengths (pool_fwd_ragged_kernel): the coefficients from the row's own frame count Tc, +0 into the
// rows behind its own frames -- the zeros the data gradients carry down the stack
template <int NS>
__global__ __launch_bounds__(256) void pool_bwd_ragged_kernel(const float* __restrict__ act, const float* __restrict__ stats,
                                                              const float* __restrict__ dpart, int nsplit, int B, int Tld,
                                                              float* __restrict__ dact, const int32_t* __restrict__ lens, int nlen, int T) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
    const int Tc = min(num_frames(row_samples(lens, nlen, b, T)) - kTdnnContext, Tld);
#define SG_MISC_BODY 4
#include "k_misc_bodies.h"
    const float* a = act + (size_t)b * Tld * kPoolC + c;
    float* d = dact + (size_t)b * Tld * kPoolC + c;
    const int per = (Tld + (int)gridDim.z - 1) / (int)gridDim.z;
    const int t0 = (int)blockIdx.z * per, t1 = min(Tld, t0 + per);
    for (int t = t0 + wid; t < t1; t += 4) {
        const float v = t < Tc ? a[(size_t)t * kPoolC] : 0.f;
        d[(size_t)t * kPoolC] = v > 0.f ? alpha + beta * (v - mean) : 0.f;
    }
}

// rl.dev: a batch of unequal lengths, T its row stride in samples (Tc = num_frames(T) - kTdnnContext)
hipError_t launch_pool_fwd(const float* act5, int B, int Tc, float* stats, hipStream_t s, const RowLens& rl, int T) {
    if (rl.dev) hipLaunchKernelGGL(pool_fwd_ragged_kernel, dim3(kPoolC / 64, B), dim3(256), 0, s, act5, Tc, stats, rl.dev, rl.n, T);
    else hipLaunchKernelGGL(pool_fwd_kernel, dim3(kPoolC / 64, B), dim3(256), 0, s, act5, Tc, stats);
    return hipGetLastError();
}
hipError_t launch_pool_bwd(const float* act5, const float* stats, const float* dstats_part, int nsplit, int B, int Tc,
                           float* dact5, hipStream_t s, const RowLens& rl, int T) {
    const int z = B >= 64 ? 1 : (1536 + (kPoolC / 64) * B - 1) / ((kPoolC / 64) * B);  // >= ~1500 blocks in all
    if (rl.dev && nsplit == kFc1BwdSplitK)
        hipLaunchKernelGGL(pool_bwd_ragged_kernel<kFc1BwdSplitK>, dim3(kPoolC / 64, B, z), dim3(256), 0, s, act5, stats, dstats_part, nsplit,
                           B, Tc, dact5, rl.dev, rl.n, T);
    else if (rl.dev)
        hipLaunchKernelGGL(pool_bwd_ragged_kernel<0>, dim3(kPoolC / 64, B, z), dim3(256), 0, s, act5, stats, dstats_part, nsplit, B, Tc, dact5,
                           rl.dev, rl.n, T);
    else if (nsplit == kFc1BwdSplitK)
        hipLaunchKernelGGL(pool_bwd_kernel<kFc1BwdSplitK>, dim3(kPoolC / 64, B, z), dim3(256), 0, s, act5, stats, dstats_part, nsplit, B,
                           Tc, dact5);
    else
        hipLaunchKernelGGL(pool_bwd_kernel<0>, dim3(kPoolC / 64, B, z), dim3(256), 0, s, act5, stats, dstats_part, nsplit, B, Tc, dact5);
    return hipGetLastError();
}

// ---------------------------------------------------------------- per-step records of a step with R EOT repeats
// rows r * B + b -> loss_out[b] = mean over r (repeat order), dec_out[b] = the most frequent decision, the first seen
// winning a tie (attack/FGSM.py:50-58 divides the summed per-batch means; attack/utils.py:118-125 Counter.most_common)
__global__ void eot_trace_reduce_kernel(const float* __restrict__ loss_rows, const int64_t* __restrict__ dec_rows, int R, int B,
                                        float* __restrict__ loss_out, int64_t* __restrict__ dec_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (loss_out) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += loss_rows[(size_t)r * B + b];
        loss_out[b] = s / (float)R;
    }
    if (dec_out) {
        int64_t best = dec_rows[b];
        int best_n = 0;
        for (int r = 0; r < R; ++r) {
            const int64_t d = dec_rows[(size_t)r * B + b];
            bool seen = false;
            for (int q = 0; q < r; ++q) seen |= dec_rows[(size_t)q * B + b] == d;
            if (seen) continue;
            int n = 0;
            for (int q = r; q < R; ++q) n += dec_rows[(size_t)q * B + b] == d;
            if (n > best_n) { best_n = n; best = d; }
        }
        dec_out[b] = best;
    }
}

hipError_t launch_eot_trace_reduce(const float* loss_rows, const int64_t* dec_rows, int R, int B, float* loss_out,
                                   int64_t* dec_out, hipStream_t s) {
    hipLaunchKernelGGL(eot_trace_reduce_kernel, dim3((B + 127) / 128), dim3(128), 0, s, loss_rows, dec_rows, R, B, loss_out, dec_out);
    return hipGetLastError();
}

}  // namespace sg
