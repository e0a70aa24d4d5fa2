// Elementwise attack-state kernels around the model call (all HBM-bound, one pass each):
//   cw2_step      attack/CW2.py:72-82   tanh box, L2 term, chain through tanh, torch.optim.Adam update
//   nes_queries   adaptive_attack/NES.py:19-25  antithetic Gaussian queries around x
//   nes_grad      adaptive_attack/NES.py:47-54  loss-weighted noise average (noise regenerated, never stored)
//   fakebob_step  attack/FAKEBOB.py:93-104      momentum, per-example LR sign step, epsilon-ball clamp
//   wav_rep_sum_update  the defended PGD loop: cotangents of the EOT repeats summed in repeat order, then carried on or
//                 turned into the sign step (attack/FGSM.py:65,68)
#include "loss_device.h"
#include "sg_internal.h"
#include "philox.h"
#include "wave_reduce.h"

// These updates mirror torch elementwise expressions (separate multiply and add roundings); keep hipcc
// from contracting them into FMAs so the results are bit-identical to the reference formulas.
#pragma clang fp contract(off)

namespace sg {

// ---------------------------------------------------------------- CW2
// One pass: (optional) Adam update of the modifier from d loss1/d input_x of the CURRENT input, then
// the NEXT input_x = tanh(modifier + atanh(0.999999 x)) and per-block partials of
// loss2 = sum (input_x - x)^2.  grid (nblk, B), block 256; part[b][blockIdx.x].
__global__ __launch_bounds__(256) void cw2_step_kernel(float* __restrict__ modifier, float* __restrict__ exp_avg,
                                                       float* __restrict__ exp_avg_sq, const float* __restrict__ x,
                                                       const float* __restrict__ input_cur,
                                                       const float* __restrict__ grad1,
                                                       const float* __restrict__ const_c, int T, float step_size,
                                                       float bc2_sqrt, float one_m_b1, float beta2, float one_m_b2, float eps,
                                                       float* __restrict__ input_next, float* __restrict__ part) {
    const int b = blockIdx.y;
    const size_t base = (size_t)b * T;
    const float c = grad1 ? const_c[b] : 0.f;
    float acc = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < T; i += gridDim.x * 256) {
        const size_t o = base + i;
        const float xv = x[o];
        float m = modifier[o];
        if (grad1) {
            const float in = input_cur[o];
            // d/d modifier of const*loss1 + ||input - x||^2 through input = tanh(.)
            const float g = (c * grad1[o] + 2.f * (in - xv)) * (1.f - in * in);
            // torch.optim.Adam (single-tensor path): exp_avg.lerp_(g, 1-b1); exp_avg_sq.mul_(b2)
            // .addcmul_(g, g, value=1-b2); denom = sqrt(v)/sqrt(bc2) + eps; p.addcdiv_(m, denom, -lr/bc1)
            float ea = exp_avg[o], es = exp_avg_sq[o];
            ea = ea + one_m_b1 * (g - ea);
            es = es * beta2 + (one_m_b2 * g) * g;
            const float denom = sqrtf(es) / bc2_sqrt + eps;
            m = m + (-step_size * ea) / denom;
            exp_avg[o] = ea;
            exp_avg_sq[o] = es;
            modifier[o] = m;
        }
        const float nx = tanhf(m + atanhf(xv * 0.999999f));
        input_next[o] = nx;
        const float d = nx - xv;
        acc += d * d;
    }
    __shared__ float red[4];
    acc = wave_sum_xor(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(64) void row_sum_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    const int b = blockIdx.x;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) acc += part[(size_t)b * n + i];
    acc = wave_sum_xor(acc);
    if (threadIdx.x == 0) out[b] = acc;
}

hipError_t launch_cw2_step(float* modifier, float* exp_avg, float* exp_avg_sq, const float* x, const float* input_cur,
                           const float* grad1, const float* const_c, int B, int T, float lr, int step_t,
                           float* input_next, float* loss2, float* scratch, hipStream_t s) {
    const double b1 = 0.9, b2 = 0.999;  // torch.optim.Adam defaults (CW2.py:57); scalars rounded like Python does
    const float beta2 = (float)b2, eps = 1e-8f;
    const double bc1 = 1.0 - pow(b1, step_t), bc2 = 1.0 - pow(b2, step_t);
    const int nblk = 32;
    hipLaunchKernelGGL(cw2_step_kernel, dim3(nblk, B), dim3(256), 0, s, modifier, exp_avg, exp_avg_sq, x, input_cur, grad1,
                       const_c, T, (float)(lr / bc1), (float)sqrt(bc2), (float)(1.0 - b1), beta2, (float)(1.0 - b2), eps, input_next,
                       scratch);
    hipLaunchKernelGGL(row_sum_kernel, dim3(B), dim3(64), 0, s, scratch, nblk, loss2);
    return hipGetLastError();
}

// ---------------------------------------------------------------- NES / FAKEBOB
// standard normal for (example index, antithetic pair index, sample t): Box-Muller on two Philox words
__device__ __forceinline__ float nes_normal(uint64_t seed, int64_t example, int pair, int t) {
    uint32_t r1;
    const uint32_t r0 = philox4x32_10_w01(seed, (uint32_t)t, (uint32_t)pair, (uint32_t)example, (uint32_t)((uint64_t)example >> 32), &r1);
    const float u0 = philox_unit24(r0);
    const float u1 = philox_unit24(r1);
    return sqrtf(-2.f * logf(u0)) * cosf(6.283185307179586f * u1);
}

// queries (n, Q, T): [clean?] then S/2 "+" then S/2 "-" (NES.py:19-23); noise_out optional (n, S/2, T)
__global__ __launch_bounds__(256) void nes_queries_kernel(const float* __restrict__ x, int T, int half, int with_clean,
                                                          float sigma, uint64_t seed, int64_t index_base, int pair_base,
                                                          const float* __restrict__ noise_in,
                                                          float* __restrict__ queries, float* __restrict__ noise_out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int e = blockIdx.y;
    if (t >= T) return;
    const int Q = 2 * half + with_clean;
    const float xv = x[(size_t)e * T + t];
    float* q = queries + (size_t)e * Q * T + t;
    if (with_clean) q[0] = xv;
    for (int p = 0; p < half; ++p) {
        const float z = noise_in ? noise_in[((size_t)e * half + p) * T + t] : nes_normal(seed, index_base + e, pair_base + p, t);
        if (noise_out) noise_out[((size_t)e * half + p) * T + t] = z;
        q[(size_t)(with_clean + p) * T] = z * sigma + xv;
        q[(size_t)(with_clean + half + p) * T] = -z * sigma + xv;
    }
}

// grad[e][t] (+)= (1/S) sum_p (loss[e][p+] - loss[e][p-]) * noise[e][p][t]; accumulate != 0 adds to grad
__global__ __launch_bounds__(256) void nes_grad_kernel(const float* __restrict__ loss, int T, int half, int with_clean,
                                                       uint64_t seed, int64_t index_base, int pair_base,
                                                       const float* __restrict__ noise_in, int accumulate,
                                                       float final_sigma, float final_batches,
                                                       float* __restrict__ grad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int e = blockIdx.y;
    if (t >= T) return;
    const int Q = 2 * half + with_clean;
    const float* l = loss + (size_t)e * Q + with_clean;
    float acc = 0.f;
    // mean over the 2*half queries of loss * noise, in the reference's order: all "+" terms, then all "-"
    for (int p = 0; p < half; ++p) {
        const float z = noise_in ? noise_in[((size_t)e * half + p) * T + t] : nes_normal(seed, index_base + e, pair_base + p, t);
        acc += l[p] * z;
    }
    for (int p = 0; p < half; ++p) {
        const float z = noise_in ? noise_in[((size_t)e * half + p) * T + t] : nes_normal(seed, index_base + e, pair_base + p, t);
        acc += l[half + p] * -z;
    }
    acc /= (float)(2 * half);
    const size_t o = (size_t)e * T + t;
    float g = accumulate ? grad[o] + acc : acc;
    if (final_sigma > 0.f) g = (g / final_sigma) / final_batches;  // NES.py:54 divides twice
    grad[o] = g;
}

// grad = momentum*prev + (1-momentum)*grad (in place); x = clamp(x + grad_sign*lr[e]*sign(grad), lower, upper)
__global__ __launch_bounds__(256) void fakebob_step_kernel(float* __restrict__ x, float* __restrict__ grad,
                                                           const float* __restrict__ prev_grad,
                                                           const float* __restrict__ lr, const float* __restrict__ lower,
                                                           const float* __restrict__ upper, int T, float momentum,
                                                           float one_m_momentum, int grad_sign) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int e = blockIdx.y;
    if (t >= T) return;
    const size_t o = (size_t)e * T + t;
    // FAKEBOB.py:93: the two weights are Python doubles rounded to fp32 by the caller
    const float g = momentum * prev_grad[o] + one_m_momentum * grad[o];
    grad[o] = g;
    const float sg = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);
    const float v = x[o] + (float)grad_sign * lr[e] * sg;
    x[o] = fminf(fmaxf(v, lower[o]), upper[o]);
}

hipError_t launch_nes_queries(const float* x, int n, int T, int half, int with_clean, float sigma, uint64_t seed,
                              int64_t index_base, int pair_base, const float* noise_in, float* queries, float* noise_out,
                              hipStream_t s) {
    hipLaunchKernelGGL(nes_queries_kernel, dim3((T + 255) / 256, n), dim3(256), 0, s, x, T, half, with_clean, sigma, seed,
                       index_base, pair_base, noise_in, queries, noise_out);
    return hipGetLastError();
}

hipError_t launch_nes_grad(const float* loss, int n, int T, int half, int with_clean, uint64_t seed, int64_t index_base,
                           int pair_base, const float* noise_in, int accumulate, float final_sigma, int final_batches,
                           float* grad, hipStream_t s) {
    hipLaunchKernelGGL(nes_grad_kernel, dim3((T + 255) / 256, n), dim3(256), 0, s, loss, T, half, with_clean, seed,
                       index_base, pair_base, noise_in, accumulate, final_sigma, (float)final_batches, grad);
    return hipGetLastError();
}

hipError_t launch_fakebob_step(float* x, float* grad, const float* prev_grad, const float* lr, const float* lower,
                               const float* upper, int n, int T, float momentum, float one_m_momentum, int grad_sign,
                               hipStream_t s) {
    hipLaunchKernelGGL(fakebob_step_kernel, dim3((T + 255) / 256, n), dim3(256), 0, s, x, grad, prev_grad, lr, lower, upper,
                       T, momentum, one_m_momentum, grad_sign);
    return hipGetLastError();
}

// ---------------------------------------------------------------- repeat sum + PGD update (sg_xv_pgd_run_defended)
// planes (G, n): plane r starts r * n floats after plane 0.  total[i] = ((carry[i] +) p0[i] + p1[i]) + ... + p(G-1)[i], plain
// float32 additions in that order.  sum_out: the total (may alias carry: every element is read before it is written, by the
// thread that writes it).  x: the update of pgd_update_kernel (k_misc.hip) on the total, bit for bit -- step * grad_sign
// times a sign in {-1, 0, 1} is exact, so neither the association nor a contraction can change the sum with x.
// One pass: a thread owns the four elements 4 j .. 4 j + 3.  x, lower, upper, carry, sum_out and plane 0 are read and
// written as 16-byte vectors when their bases are aligned (`vec`, decided by the launcher).  Plane r is misaligned by
// m = (r n) & 3 floats when n is no multiple of 4: its four elements then come from the two ALIGNED vectors that cover
// them (the neighbouring thread's second vector is this thread's first: the second request hits the cache, HBM traffic
// stays one pass), unless one of the two would reach outside [planes, planes + G n) -- the first thread of the head, the
// last of the tail -- or the thread owns the ragged end of the row (n & 3 elements): those go element by element.
typedef float rs_f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void wav_rep_sum_update_kernel(const float* __restrict__ planes, int G, int64_t n,
                                                                 const float* carry, float* sum_out, float* __restrict__ x,
                                                                 const float* __restrict__ lo, const float* __restrict__ hi,
                                                                 float step, int grad_sign, int vec) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const float s = step * (float)grad_sign;
    if (vec && i0 + 3 < n) {
        rs_f4 tot = *reinterpret_cast<const rs_f4*>(planes + i0);
        if (carry) tot = *reinterpret_cast<const rs_f4*>(carry + i0) + tot;
        const int64_t end = (int64_t)G * n;
        for (int r = 1; r < G; ++r) {
            const int64_t a = (int64_t)r * n + i0;
            const int m = (int)(a & 3);  // uniform over the launch
            rs_f4 p;
            if (m == 0) {
                p = *reinterpret_cast<const rs_f4*>(planes + a);
            } else if (a - m + 8 <= end) {  // (a - m >= 0: r >= 1)
                const rs_f4 u = *reinterpret_cast<const rs_f4*>(planes + (a - m));
                const rs_f4 v = *reinterpret_cast<const rs_f4*>(planes + (a - m + 4));
                p = m == 1 ? rs_f4{u.y, u.z, u.w, v.x} : m == 2 ? rs_f4{u.z, u.w, v.x, v.y} : rs_f4{u.w, v.x, v.y, v.z};
            } else {
                p = rs_f4{planes[a], planes[a + 1], planes[a + 2], planes[a + 3]};
            }
            tot = tot + p;
        }
        if (sum_out) *reinterpret_cast<rs_f4*>(sum_out + i0) = tot;
        if (x) {
            rs_f4 xv = *reinterpret_cast<const rs_f4*>(x + i0);
            const rs_f4 lv = *reinterpret_cast<const rs_f4*>(lo + i0), hv = *reinterpret_cast<const rs_f4*>(hi + i0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float sg = tot[c] > 0.f ? 1.f : (tot[c] < 0.f ? -1.f : 0.f);
                xv[c] = fminf(fmaxf(xv[c] + s * sg, lv[c]), hv[c]);
            }
            *reinterpret_cast<rs_f4*>(x + i0) = xv;
        }
        return;
    }
    for (int64_t i = i0; i < n && i < i0 + 4; ++i) {
        float tot = planes[i];
        if (carry) tot = carry[i] + tot;
        for (int r = 1; r < G; ++r) tot = tot + planes[(int64_t)r * n + i];
        if (sum_out) sum_out[i] = tot;
        if (x) {
            const float sg = tot > 0.f ? 1.f : (tot < 0.f ? -1.f : 0.f);
            x[i] = fminf(fmaxf(x[i] + s * sg, lo[i]), hi[i]);
        }
    }
}

hipError_t launch_wav_rep_sum_update(const float* planes, int G, int64_t n, const float* carry, float* sum_out, float* x,
                                     const float* lo, const float* hi, float step, int grad_sign, hipStream_t s) {
    const uintptr_t bases = reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(carry) |
                            reinterpret_cast<uintptr_t>(sum_out) | reinterpret_cast<uintptr_t>(x) |
                            reinterpret_cast<uintptr_t>(x ? lo : nullptr) | reinterpret_cast<uintptr_t>(x ? hi : nullptr);
    const int64_t blocks = (n + 1023) / 1024;
    hipLaunchKernelGGL(wav_rep_sum_update_kernel, dim3((unsigned)blocks), dim3(256), 0, s, planes, G, n, carry, sum_out, x, lo, hi,
                       step, grad_sign, (int)(bases % 16 == 0));
    return hipGetLastError();
}

// ---------------------------------------------------------------- loss stage alone
// attack/utils.py:7-102 on given scores: one thread per utterance (S is 10 .. 251), global memory as its scratch.
__global__ __launch_bounds__(64) void loss_eval_kernel(const float* __restrict__ scores, const int64_t* __restrict__ y, int B,
                                                       int S, float threshold, sg_loss_spec ls, int64_t* __restrict__ dec_out,
                                                       float* __restrict__ loss_out, float* __restrict__ dsc_out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float* dsc = dsc_out + (size_t)b * S;
    for (int s = 0; s < S; ++s) dsc[s] = 0.f;
    int64_t dec = 0;
    const float loss = loss_and_dscores(scores + (size_t)b * S, dsc, S, threshold, y ? y[b] : 0, y != nullptr, ls, &dec,
                                        ls.coef_dev ? ls.coef_dev + (size_t)b * S : nullptr);
    if (dec_out) dec_out[b] = dec;
    if (loss_out) loss_out[b] = loss;
}

hipError_t launch_loss_eval(const float* scores, const int64_t* y, int B, int S, float threshold, const sg_loss_spec& ls,
                            int64_t* dec, float* loss, float* dscores, hipStream_t s) {
    if (S < 1 || S > kLossMaxS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loss_eval_kernel, dim3((B + 63) / 64), dim3(64), 0, s, scores, y, B, S, threshold, ls, dec, loss, dscores);
    return hipGetLastError();
}

}  // namespace sg
