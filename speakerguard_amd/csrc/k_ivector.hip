// GMM / i-vector / PLDA system (reference model/iv_plda.py, _iv_plda/gmm.py, _iv_plda/ivector_extract.py): the forward, and the
// tail's adjoint behind its forward (iv_tail_kernel); the rest of the backward is k_ivector_bwd.hip.
// Every formula and every summation order of the file, stage by stage.  An utterance's numbers are one fixed sequence of
// operations: no sum below depends on the batch size, on the row's place in the call or on the chunk it falls into.
//
// 1. iv_delta_cmvn_kernel (one block per utterance), iv_plda.py:248-377.  With x = the first 24 columns of a raw row and
//    the frame index clamped to [0, F-1]:
//      delta[t][c]      = x[t][c]
//      delta[t][24 + c] = sum_{j=-3..3} x[t+j][c] s1[j],   s1[j] = fl(j fl(1/28))
//      delta[t][48 + c] = sum_{j=-6..6} x[t+j][c] s2[j],   s2 = s1 * s1 (get_scales, built on the host in its float32 order)
//    float32, j ascending.  CMVN: window [ws, we) of <= 300 frames around t (the reference's clipping rules),
//      cmvn[t][c] = delta[t][c] + (sum_{f=ws..we-1} delta[f][c]) * fl(-1 / (we - ws)),
//    the window sum taken DIRECTLY in float32, f ascending (the reference slides a running sum; the direct sum carries no
//    drift and needs no order between frames).
// 2. iv_loglik_kernel, gmm.py:120-131 as ONE contraction on v_mfma_f32_32x32x2_f32:
//      ll[t][c] = gconst_c + sum_{k<2700} z_t[k] W_c[k],   z_t = [x_t ; x_i x_j (i <= j)],  W_c = [mi_c ; -S_c,ii / 2 ; -S_c,ij]
//    (the symmetric form: half the multiplications of x^T (S x)).  z is NOT materialised: a 64-frame tile of x sits in LDS
//    (row stride 73, entry 72 = 1 so that the linear terms are products too) and every lane forms its A operand
//    fl(x_i x_j) from two LDS reads and the (i, j) table while staging -- z would be 37.5 x the size of x and would be
//    written and read once, for a product that costs one multiplication.  The k chain of an MFMA accumulator is a
//    sequential float32 fmaf chain, k ascending, of 180 terms; the 15 chains of an entry are added in float64, in order, and
//    gconst last, rounded once.  No (frames, C, 72) intermediate exists.
// 3. iv_rowstat_kernel (one wave per frame) + iv_stats_kernel, gmm.py:133-171: softmax with the row maximum subtracted
//    before expf, so a frame far from every component still gives finite posteriors:
//      mx_t = max_c ll[t][c],  s_t = sum_c expf(ll[t][c] - mx_t)  (float64 sum: lane-strided, then the xor butterfly)
//      post[t][c] = expf(ll[t][c] - mx_t) / fl(s_t)
//      n[c] = sum_t post[t][c],  f[c][d] = sum_t post[t][c] x[t][d]   float64 accumulators, t ascending, rounded once.
// 4. iv_assemble_L_kernel / iv_assemble_lin_kernel, ivector_extract.py:98-108 from the tables packed at load
//    (V_c = M_c^T Sigma_c^-1, U_c = upper triangle of V_c M_c; float64 on the host, rounded once):
//      L[p] = sum_c n_c U_c[p]  (+ 1 on the diagonal, added by the solve),  c ascending, float64 accumulators
//      lin[r] = sum_{slices of 16 components, ascending} (sum_{c in slice, d} V_c[r][d] f_c[d]),  (c, d) ascending, float64.
//    A block keeps 16 utterances' accumulators per entry, so U (660 MB at C = 2048, R = 400) is streamed once per 16 rows.
// 5. iv_solve_kernel (one block per utterance): L = G G^T by a left-looking Cholesky in float64, panels of 4 columns in
//    LDS (R x R does not fit), then G y = lin (+ offset on entry 0), G^T w = y, w[0] -= offset (ivector_extract.py:108-112;
//    the reference inverts L).  L is I + PSD by construction.  Column j of G occupies row j of the packed upper triangle.
//    Every dot product runs k (or i) ascending per thread; the back substitution's per-column sums are combined by
//    block_reduce_xor (wave_reduce.h).
// 6. iv_tail_kernel (one block per utterance): k_tail.hip's forward on an R-vector -- mean subtraction, LDA affine, length
//    normalisation to sqrt(D), PLDA transform and normalisation factor, log-likelihood-ratio scores, decision, loss
//    (loss_device.h) -- float32, every product k ascending per output, block sums by block_reduce_xor.
#include <cmath>

#include "loss_device.h"
#include "plda_device.h"
#include "sg_internal.h"
#include "wave_reduce.h"

namespace sg {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kDcThreads = 1024;
__global__ __launch_bounds__(kDcThreads) void iv_delta_cmvn_kernel(const float* __restrict__ raw, int ld, int F, IvDeltaScales sc,
                                                                   float* __restrict__ delta_ws, float* __restrict__ delta_out,
                                                                   float* __restrict__ cmvn_out) {
    const int b = blockIdx.x, n = F * kIvDim;
    const float* r = raw ? raw + (size_t)b * F * ld : nullptr;
    float* dw = delta_ws + (size_t)b * n;
    // raw == null: delta_ws already holds the utterance's delta rows (a caller's flag-2 input), only the CMVN runs
    for (int idx = threadIdx.x; raw && idx < n; idx += kDcThreads) {
        const int t = idx / kIvDim, col = idx - t * kIvDim, o = col / kIvCep, c = col - o * kIvCep;
        float v = 0.f;
        if (o == 0) {
            v = r[(size_t)t * ld + c];
        } else if (o == 1) {
            for (int j = -3; j <= 3; ++j) v += r[(size_t)min(max(t + j, 0), F - 1) * ld + c] * sc.s1[j + 3];
        } else {
            for (int j = -6; j <= 6; ++j) v += r[(size_t)min(max(t + j, 0), F - 1) * ld + c] * sc.s2[j + 6];
        }
        dw[idx] = v;
        if (delta_out) delta_out[(size_t)b * n + idx] = v;
    }
    if (!cmvn_out) return;
    __syncthreads();  // the block reads back its own rows
    for (int idx = threadIdx.x; idx < n; idx += kDcThreads) {
        const int t = idx / kIvDim, col = idx - t * kIvDim;
        int ws = t - kCmnWindow / 2, we = ws + kCmnWindow;  // iv_plda.py:321-337
        if (ws < 0) { we -= ws; ws = 0; }
        if (we > F) { ws -= we - F; we = F; if (ws < 0) ws = 0; }
        float s = 0.f;
        for (int f = ws; f < we; ++f) s += dw[f * kIvDim + col];
        cmvn_out[(size_t)b * n + idx] = dw[idx] + s * (-1.f / (float)(we - ws));
    }
}

constexpr int kLlRows = 64, kLlXld = kIvDim + 1, kLlFlush = 90;  // 1350 k-steps = 15 flushes
static_assert((kIvK / 2) % kLlFlush == 0, "whole flushes");
__global__ __launch_bounds__(256) void iv_loglik_kernel(const float* __restrict__ x, int M, const float* __restrict__ W,
                                                        const uint16_t* __restrict__ pairs, const float* __restrict__ gconst, int C,
                                                        int Cp, float* __restrict__ ll) {
    __shared__ float xs[kLlRows * kLlXld];
    __shared__ uint16_t pr[kIvK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * kLlRows;
    for (int i = tid; i < kLlRows * kLlXld; i += 256) {
        const int row = i / kLlXld, col = i - row * kLlXld;
        const int m = min(m0 + row, M - 1);  // rows past the call repeat its last row; they are not stored
        xs[i] = col < kIvDim ? x[(size_t)m * kIvDim + col] : 1.f;
    }
    for (int i = tid; i < kIvK; i += 256) pr[i] = pairs[i];
    __syncthreads();
    const int c0 = (blockIdx.y * 4 + wave) * 64;  // a wave owns 64 frames x 64 components: 2 x 2 MFMA tiles
    if (c0 >= Cp) return;                          // (no barrier follows)
    // Two levels: the MFMA accumulators run kLlFlush k-steps (a float32 fmaf chain of 2 kLlFlush terms), then go into float64
    // totals and start again from zero.  One 2700-term float32 chain measured 5.6 x the reference's own distance from float64
    // on the zeroth statistics (its sums are 72 terms long); the flush costs 64 float64 adds per 360 MFMAs.
    f32x16 acc[2][2];
    double tot[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int e = 0; e < 16; ++e) tot[a][bb][e] = 0.0;
    const int r = lane & 31, h = lane >> 5;
    const float* wp = W + c0 + r;
    const float* x0 = xs + r * kLlXld;
    const float* x1 = xs + (32 + r) * kLlXld;
    for (int kc = 0; kc < kIvK / 2; kc += kLlFlush) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][bb][e] = 0.f;
#pragma unroll 3
        for (int ks = kc; ks < kc + kLlFlush; ++ks) {
            const int k = 2 * ks + h;  // lane l feeds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31]
            const unsigned p = pr[k];
            const int i = p & 0xff, j = p >> 8;
            const float a0 = x0[i] * x0[j], a1 = x1[i] * x1[j];
            const float b0 = wp[(size_t)k * Cp], b1 = wp[(size_t)k * Cp + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                for (int e = 0; e < 16; ++e) tot[a][bb][e] += (double)acc[a][bb][e];
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int c = c0 + ni * 32 + r;
            if (c >= C) continue;
            const double g = (double)gconst[c];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (m < M) ll[(size_t)m * C + c] = (float)(tot[mi][ni][e] + g);
            }
        }
}

__global__ __launch_bounds__(256) void iv_rowstat_kernel(const float* __restrict__ ll, int M, int C, float* __restrict__ rowmax,
                                                         float* __restrict__ rowsum) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;  // (a whole wave; the kernel has no barrier)
    const float* row = ll + (size_t)m * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, row[c]);
    mx = wave_max_xor(mx);
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)expf(row[c] - mx);
    s = wave_sum_xor_steps(s);
    if (lane == 0) {
        rowmax[m] = mx;
        rowsum[m] = (float)s;
    }
}

constexpr int kStFrames = 32, kStD = kIvDim / 4;
__global__ __launch_bounds__(256) void iv_stats_kernel(const float* __restrict__ x, const float* __restrict__ ll,
                                                       const float* __restrict__ rowmax, const float* __restrict__ rowsum, int F, int C,
                                                       float* __restrict__ n, float* __restrict__ f) {
    __shared__ float xs[kStFrames * kIvDim];
    __shared__ float ps[kStFrames * 64];
    const int tid = threadIdx.x, cl = tid & 63, ds = tid >> 6, b = blockIdx.y, c0 = blockIdx.x * 64, c = c0 + cl;
    double acc[kStD], accn = 0.0;
#pragma unroll
    for (int d = 0; d < kStD; ++d) acc[d] = 0.0;
    for (int t0 = 0; t0 < F; t0 += kStFrames) {
        const int nt = min(kStFrames, F - t0);
        const size_t mbase = (size_t)b * F + t0;
        __syncthreads();
        for (int i = tid; i < nt * kIvDim; i += 256) xs[i] = x[mbase * kIvDim + i];
        for (int i = tid; i < nt * 64; i += 256) {
            const int tt = i >> 6, cc = c0 + (i & 63);
            const size_t m = mbase + tt;
            ps[i] = cc < C ? expf(ll[m * C + cc] - rowmax[m]) / rowsum[m] : 0.f;
        }
        __syncthreads();
        for (int tt = 0; tt < nt; ++tt) {
            const double p = (double)ps[tt * 64 + cl];
            if (ds == 0) accn += p;
#pragma unroll
            for (int d = 0; d < kStD; ++d) acc[d] += p * (double)xs[tt * kIvDim + ds * kStD + d];
        }
    }
    if (c >= C) return;
    if (ds == 0) n[(size_t)b * C + c] = (float)accn;
#pragma unroll
    for (int d = 0; d < kStD; ++d) f[((size_t)b * C + c) * kIvDim + ds * kStD + d] = (float)acc[d];
}

constexpr int kAsmG = 16;  // utterances per block: U and V are read once per group of 16
__global__ __launch_bounds__(256) void iv_assemble_L_kernel(const float* __restrict__ U, int Pp, int C, const float* __restrict__ n, int B,
                                                            double* __restrict__ Lmat) {
    __shared__ float ns[kAsmG][256];
    const int tid = threadIdx.x, b0 = blockIdx.y * kAsmG, nb = min(kAsmG, B - b0);
    const size_t p = (size_t)blockIdx.x * 256 + tid;  // < Pp: Pp is a multiple of 256 and the grid covers exactly Pp
    double acc[kAsmG];
#pragma unroll
    for (int bb = 0; bb < kAsmG; ++bb) acc[bb] = 0.0;
    for (int cb = 0; cb < C; cb += 256) {
        const int cn = min(256, C - cb);
        __syncthreads();
        for (int i = tid; i < kAsmG * 256; i += 256) {
            const int bb = i >> 8, cc = i & 255;
            ns[bb][cc] = (bb < nb && cc < cn) ? n[(size_t)(b0 + bb) * C + cb + cc] : 0.f;
        }
        __syncthreads();
        for (int cc = 0; cc < cn; ++cc) {
            const double u = (double)U[(size_t)(cb + cc) * Pp + p];
#pragma unroll
            for (int bb = 0; bb < kAsmG; ++bb) acc[bb] += (double)ns[bb][cc] * u;
        }
    }
    for (int bb = 0; bb < nb; ++bb) Lmat[(size_t)(b0 + bb) * Pp + p] = acc[bb];
}

__global__ __launch_bounds__(256) void iv_assemble_lin_kernel(const float* __restrict__ Vt, int R, int C, const float* __restrict__ f, int B,
                                                              double* __restrict__ linpart) {
    __shared__ float fs[kAsmG][kIvDim];
    const int tid = threadIdx.x, r = blockIdx.x * 256 + tid, sl = blockIdx.y, b0 = blockIdx.z * kAsmG, nb = min(kAsmG, B - b0);
    double acc[kAsmG];
#pragma unroll
    for (int bb = 0; bb < kAsmG; ++bb) acc[bb] = 0.0;
    const int cend = min(C, (sl + 1) * kIvLinSlice);
    for (int c = sl * kIvLinSlice; c < cend; ++c) {
        __syncthreads();
        for (int i = tid; i < kAsmG * kIvDim; i += 256) {
            const int bb = i / kIvDim, d = i - bb * kIvDim;
            fs[bb][d] = bb < nb ? f[((size_t)(b0 + bb) * C + c) * kIvDim + d] : 0.f;
        }
        __syncthreads();
        if (r < R)
            for (int d = 0; d < kIvDim; ++d) {
                const double v = (double)Vt[((size_t)c * kIvDim + d) * R + r];
#pragma unroll
                for (int bb = 0; bb < kAsmG; ++bb) acc[bb] += (double)fs[bb][d] * v;
            }
    }
    if (r < R)
        for (int bb = 0; bb < nb; ++bb) linpart[((size_t)sl * B + b0 + bb) * R + r] = acc[bb];
}

constexpr int kChNb = 4, kChThreads = 256;
__global__ __launch_bounds__(kChThreads) void iv_solve_kernel(double* __restrict__ Lmat, int Pp, const double* __restrict__ linpart, int NS,
                                                              int B, int R, float offset, float* __restrict__ ivec,
                                                              double* __restrict__ solved) {
    __shared__ double pan[kIvMaxR * kChNb];
    __shared__ double vec[kIvMaxR];
    __shared__ double red[kChThreads / 64];
    constexpr int NT = kChThreads, NB = kChNb;
    const int tid = threadIdx.x, b = blockIdx.x;
    double* A = Lmat + (size_t)b * Pp;
    // column j of the factor = row j of the packed upper triangle: entry (i, j), i >= j, at off(j) + i - j
    const auto off = [R](int j) { return (size_t)j * R - (size_t)j * (j - 1) / 2; };
    for (int i = tid; i < R; i += NT) {
        double v = 0.0;
        for (int sl = 0; sl < NS; ++sl) v += linpart[((size_t)sl * B + b) * R + i];
        vec[i] = i == 0 ? v + (double)offset : v;
        A[off(i)] += 1.0;  // L = I + sum_c n_c U_c
    }
    __syncthreads();
    for (int j0 = 0; j0 < R; j0 += NB) {
        const int nbk = min(NB, R - j0), rows = R - j0;
        // the panel's rows minus the columns already factored: a[jj] -= sum_{k < j0} G[i][k] G[j0 + jj][k], k ascending
        for (int il = tid; il < rows; il += NT) {
            const int i = j0 + il;
            double a[NB];
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) a[jj] = (jj < nbk && il >= jj) ? A[off(j0 + jj) + (il - jj)] : 0.0;
            for (int k = 0; k < j0; ++k) {
                const double* col = A + off(k) - k;
                const double lik = col[i];
#pragma unroll
                for (int jj = 0; jj < NB; ++jj) a[jj] -= lik * col[min(j0 + jj, R - 1)];
            }
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) pan[il * NB + jj] = a[jj];
        }
        __syncthreads();
        for (int jj = 0; jj < nbk; ++jj) {
            const double d = sqrt(pan[jj * NB + jj]);
            __syncthreads();  // everyone holds the pivot before its owner overwrites it
            for (int il = jj + tid; il < rows; il += NT) pan[il * NB + jj] = il == jj ? d : pan[il * NB + jj] / d;
            __syncthreads();
            for (int il = jj + 1 + tid; il < rows; il += NT) {
                const double l = pan[il * NB + jj];
                for (int j2 = jj + 1; j2 < nbk; ++j2)
                    if (il >= j2) pan[il * NB + j2] -= l * pan[j2 * NB + jj];
            }
            __syncthreads();
        }
        for (int il = tid; il < rows; il += NT)
            for (int jj = 0; jj < nbk; ++jj)
                if (il >= jj) A[off(j0 + jj) + (il - jj)] = pan[il * NB + jj];
        __syncthreads();  // the next panel reads these columns back
    }
    // G y = lin: column sweeps
    for (int j = 0; j < R; ++j) {
        const double* col = A + off(j);
        const double yj = vec[j] / col[0];
        __syncthreads();
        for (int i = j + 1 + tid; i < R; i += NT) vec[i] -= col[i - j] * yj;
        if (tid == 0) vec[j] = yj;
        __syncthreads();
    }
    // G^T w = y: w[j] = (y[j] - sum_{i > j} G[i][j] w[i]) / G[j][j]
    for (int j = R - 1; j >= 0; --j) {
        const double* col = A + off(j);
        double part = 0.0;
        for (int i = j + 1 + tid; i < R; i += NT) part += col[i - j] * vec[i];
        const double sum = block_reduce_xor<kChThreads / 64, true>(part, red, OpSum());
        if (tid == 0) vec[j] = (vec[j] - sum) / col[0];
        __syncthreads();
    }
    for (int i = tid; i < R; i += NT) {
        ivec[(size_t)b * R + i] = (float)(i == 0 ? vec[i] - (double)offset : vec[i]);
        if (solved) solved[(size_t)b * R + i] = vec[i];  // s = w + offset e0, for the backward's dL = -lambda s^T
    }
}

struct IvTailDev {
    const float *emb_mean, *lda_t, *plda_mean, *plda_pt, *plda_psi, *enroll;
    int R, D, S;
    float threshold, logdet_given, logdet_without;
};
constexpr int kTlThreads = 256;
__global__ __launch_bounds__(kTlThreads) void iv_tail_kernel(IvTailDev m, const float* __restrict__ ivec, const int64_t* __restrict__ y,
                                                             sg_loss_spec ls, const float* __restrict__ coef, float* __restrict__ emb_out,
                                                             float* __restrict__ scores_out, int64_t* __restrict__ dec_out,
                                                             float* __restrict__ loss_out, float* __restrict__ dw_out) {
    __shared__ float e1[kIvMaxR];
    __shared__ float e2[kIvMaxD], e4[kIvMaxD], e5[kIvMaxD], c_psi[kIvMaxD];
    __shared__ float sc[kLossMaxS], dsc[kLossMaxS];
    __shared__ float red[kTlThreads / 64];
    constexpr int NT = kTlThreads;
    const int b = blockIdx.x, tid = threadIdx.x, R = m.R, D = m.D, S = m.S;
    const float sqrtD = sqrtf((float)D);
    for (int i = tid; i < R; i += NT) e1[i] = ivec[(size_t)b * R + i] - m.emb_mean[i];  // iv_plda.py:419
    for (int d = tid; d < D; d += NT) c_psi[d] = m.plda_psi[d];
    __syncthreads();
    // LDA affine (row R of the transposed matrix = the offset column), iv_plda.py:423-435
    float n2 = 0.f;
    for (int d = tid; d < D; d += NT) {
        float acc = 0.f;
        for (int k = 0; k < R; ++k) acc += m.lda_t[(size_t)k * D + d] * e1[k];
        acc += m.lda_t[(size_t)R * D + d];
        e2[d] = acc;
        n2 += acc * acc;
    }
    const float ratio = sqrtD / sqrtf(block_reduce_xor<NT / 64, true>(n2, red, OpSum()));  // a constant in the backward (.item())
    for (int d = tid; d < D; d += NT) e2[d] = e2[d] * ratio - m.plda_mean[d];
    __syncthreads();
    // PLDA transform + normalisation factor, plda.py:73-97
    float qp = 0.f;
    for (int d = tid; d < D; d += NT) {
        float acc = 0.f;
        for (int j = 0; j < D; ++j) acc += m.plda_pt[(size_t)j * D + d] * e2[j];
        e4[d] = acc;
        qp += acc * acc / (c_psi[d] + 1.f);
    }
    const float q = block_reduce_xor<NT / 64, true>(qp, red, OpSum());
    const float fac = sqrtf((float)D / q);
    for (int d = tid; d < D; d += NT) {
        e5[d] = e4[d] * fac;
        if (emb_out) emb_out[(size_t)b * D + d] = e5[d];
    }
    __syncthreads();
    // PLDA scores: one wave per enrolled speaker, plda.py:140-190 (k_tail.hip step 5)
    plda_llr_scores<NT>(e5, c_psi, m.enroll, D, S, m.logdet_given, m.logdet_without, sc, dsc,
                        scores_out ? scores_out + (size_t)b * S : nullptr);
    __syncthreads();
    if (tid == 0) {
        int64_t dec = 0;
        const float loss = loss_and_dscores(sc, dsc, S, m.threshold, y ? y[b] : 0, y != nullptr, ls, &dec,
                                            coef ? coef + (size_t)b * S : nullptr);
        if (dec_out) dec_out[b] = dec;
        if (loss_out) loss_out[b] = loss;
    }
    if (!dw_out) return;
    __syncthreads();
    // The adjoint of the tail (k_tail.hip steps 9-13 on an R-vector), float32, every sum in index order per output:
    //   d e5 = sum_s dsc_s (-(e5 - r enroll_s) / (1 + r) + e5 / (psi + 1)),
    //   d e4 = fac d e5 - (d e5 . e4) (fac / q) e4 / (psi + 1)      (the normalisation factor is differentiated, plda.py:92-97)
    //   d e2 = ratio P^T d e4                                       (the length normalisation's norm is a CONSTANT: .item())
    //   d w  = A^T d e2                                             (A: the LDA matrix without its offset column)
    float* dv = e5;  // every thread reads e5 at its own d below, then writes d e4 there
    float dotp = 0.f;
    float g_own[(kIvMaxD + NT - 1) / NT];
    {
        int slot = 0;
        for (int d = tid; d < D; d += NT, ++slot) {
            const float g = plda_de5_term(e5, c_psi, m.enroll, dsc, D, S, d);
            g_own[slot] = g;
            dotp += g * e4[d];
        }
    }
    const float dot = block_reduce_xor<NT / 64, true>(dotp, red, OpSum());
    {
        int slot = 0;
        for (int d = tid; d < D; d += NT, ++slot) dv[d] = (fac * g_own[slot] - dot * (fac / q) * e4[d] / (c_psi[d] + 1.f)) * ratio;
    }
    __syncthreads();
    for (int j = tid; j < D; j += NT) {  // P^T: plda_pt holds P transposed, [j][d] = P[d][j]
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc += m.plda_pt[(size_t)j * D + d] * dv[d];
        e2[j] = acc;
    }
    __syncthreads();
    for (int k = tid; k < R; k += NT) {
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc += m.lda_t[(size_t)k * D + d] * e2[d];
        dw_out[(size_t)b * R + k] = acc;
    }
}

}  // namespace

IvDeltaScales iv_delta_scales() {
    // get_scales(window=3, order=2): cur[j + k + off] += j * prev[k] in float32, then * float32(1 / normalizer)
    IvDeltaScales sc;
    const float inv = (float)(1.0 / 28.0);
    for (int j = -3; j <= 3; ++j) sc.s1[j + 3] = (float)j * inv;
    float cur[13] = {};
    for (int j = -3; j <= 3; ++j)
        for (int k = -3; k <= 3; ++k) cur[j + k + 6] += (float)j * sc.s1[k + 3];
    for (int i = 0; i < 13; ++i) sc.s2[i] = cur[i] * inv;
    return sc;
}

bool iv_pack_model(const sg_iv_weights* w, int Cp, int Pp, std::vector<float>* W, std::vector<uint16_t>* pairs, std::vector<float>* Vt,
                   std::vector<float>* U, std::string* why) {
    const int C = w->C, R = w->R, Dm = kIvDim;
    const auto finite = [](const float* p, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(p[i])) return false;
        return true;
    };
    const auto symmetric = [](const float* a) {
        constexpr int Dm = kIvDim;
        for (int i = 0; i < Dm; ++i)
            for (int j = i + 1; j < Dm; ++j) {
                const float u = a[i * Dm + j], v = a[j * Dm + i];
                if (std::fabs(u - v) > 1e-6f * std::max(std::fabs(u), std::fabs(v))) return false;
            }
        return true;
    };
    if (!finite(w->gconsts, C) || !finite(w->means_invcovars, (size_t)C * Dm) || !finite(w->extractor, (size_t)C * Dm * R)) {
        *why = "a non-finite entry in gconsts, means_invcovars or the extractor matrix";
        return false;
    }
    if (!finite(w->invcovars, (size_t)C * Dm * Dm) || !finite(w->sigma_inv, (size_t)C * Dm * Dm)) {
        *why = "a non-finite entry in invcovars or sigma_inv";
        return false;
    }
    for (int c = 0; c < C; ++c)
        if (!symmetric(w->invcovars + (size_t)c * Dm * Dm) || !symmetric(w->sigma_inv + (size_t)c * Dm * Dm)) {
            *why = "invcovars or sigma_inv of component " + std::to_string(c) + " is not symmetric";
            return false;
        }
    pairs->assign(kIvK, 0);
    for (int k = 0; k < Dm; ++k) (*pairs)[k] = (uint16_t)(k | (Dm << 8));  // x_k * x_72, x_72 = 1
    for (int i = 0; i < Dm; ++i)
        for (int j = i; j < Dm; ++j) (*pairs)[iv_zpos(i, j)] = (uint16_t)(i | (j << 8));
    W->assign((size_t)kIvK * Cp, 0.f);
    for (int c = 0; c < C; ++c) {
        const float* S = w->invcovars + (size_t)c * Dm * Dm;
        for (int k = 0; k < Dm; ++k) (*W)[(size_t)k * Cp + c] = w->means_invcovars[(size_t)c * Dm + k];
        for (int i = 0; i < Dm; ++i)
            for (int j = i; j < Dm; ++j) {
                const double s = 0.5 * ((double)S[i * Dm + j] + (double)S[j * Dm + i]);
                (*W)[(size_t)iv_zpos(i, j) * Cp + c] = (float)(i == j ? -0.5 * s : -s);
            }
    }
    Vt->assign((size_t)C * Dm * R, 0.f);
    U->assign((size_t)C * Pp, 0.f);
    std::vector<double> V((size_t)Dm * R), Ut((size_t)R * (R + 1) / 2);
    for (int c = 0; c < C; ++c) {
        const float* M = w->extractor + (size_t)c * Dm * R;   // [e][r]
        const float* Sg = w->sigma_inv + (size_t)c * Dm * Dm;  // [e][d]
        std::fill(V.begin(), V.end(), 0.0);
        for (int e = 0; e < Dm; ++e)
            for (int d = 0; d < Dm; ++d) {
                const double sg = Sg[e * Dm + d];
                double* vd = V.data() + (size_t)d * R;
                const float* me = M + (size_t)e * R;
                for (int r = 0; r < R; ++r) vd[r] += sg * (double)me[r];  // V[r][d] = sum_e M[e][r] Sigma^-1[e][d]
            }
        std::fill(Ut.begin(), Ut.end(), 0.0);
        for (int d = 0; d < Dm; ++d) {
            const double* vd = V.data() + (size_t)d * R;
            const float* md = M + (size_t)d * R;
            for (int r1 = 0; r1 < R; ++r1) {
                const double v = vd[r1];
                double* u = Ut.data() + iv_tri(r1, r1, R) - r1;
                for (int r2 = r1; r2 < R; ++r2) u[r2] += v * (double)md[r2];  // U[r1][r2] = sum_d V[r1][d] M[d][r2]
            }
        }
        float* vt = Vt->data() + (size_t)c * Dm * R;
        for (size_t i = 0; i < V.size(); ++i) vt[i] = (float)V[i];
        float* uc = U->data() + (size_t)c * Pp;
        for (size_t i = 0; i < Ut.size(); ++i) uc[i] = (float)Ut[i];
    }
    return true;
}

hipError_t launch_iv_delta_cmvn(const float* raw, int ld, int B, int F, float* delta_ws, float* delta_out, float* cmvn_out,
                                hipStream_t s) {
    hipLaunchKernelGGL(iv_delta_cmvn_kernel, dim3(B), dim3(kDcThreads), 0, s, raw, ld, F, iv_delta_scales(), delta_ws, delta_out,
                       cmvn_out);
    return hipGetLastError();
}

hipError_t launch_iv_stats(const IvModel& m, const float* cmvn, int B, int F, float* ll, float* rowmax, float* rowsum, float* n,
                           float* f, hipStream_t s) {
    const int M = B * F;
    hipLaunchKernelGGL(iv_loglik_kernel, dim3((M + kLlRows - 1) / kLlRows, (m.Cp + 255) / 256), dim3(256), 0, s, cmvn, M, m.W, m.pairs,
                       m.gconst, m.C, m.Cp, ll);
    hipLaunchKernelGGL(iv_rowstat_kernel, dim3((M + 3) / 4), dim3(256), 0, s, ll, M, m.C, rowmax, rowsum);
    hipLaunchKernelGGL(iv_stats_kernel, dim3((m.C + 63) / 64, B), dim3(256), 0, s, cmvn, ll, rowmax, rowsum, F, m.C, n, f);
    return hipGetLastError();
}

hipError_t launch_iv_extract(const IvModel& m, const float* n, const float* f, int B, double* Lmat, double* linpart, float* ivec,
                             hipStream_t s, double* solved) {
    const int NS = (m.C + kIvLinSlice - 1) / kIvLinSlice, G = (B + kAsmG - 1) / kAsmG;
    hipLaunchKernelGGL(iv_assemble_L_kernel, dim3(m.Pp / 256, G), dim3(256), 0, s, m.U, m.Pp, m.C, n, B, Lmat);
    hipLaunchKernelGGL(iv_assemble_lin_kernel, dim3((m.R + 255) / 256, NS, G), dim3(256), 0, s, m.Vt, m.R, m.C, f, B, linpart);
    hipLaunchKernelGGL(iv_solve_kernel, dim3(B), dim3(kChThreads), 0, s, Lmat, m.Pp, linpart, NS, B, m.R, m.offset, ivec, solved);
    return hipGetLastError();
}

hipError_t launch_iv_tail(const IvModel& x, const IvTailArgs& a, hipStream_t s) {
    const PldaBackend& be = x.be;
    IvTailDev m;
    plda_backend_active(be, &m.enroll, &m.S);
    if (x.R > kIvMaxR || be.D > kIvMaxD || m.S > kLossMaxS || m.S < 1) return hipErrorInvalidValue;
    m.emb_mean = x.emb_mean; m.lda_t = x.lda_t; m.plda_mean = be.plda_mean; m.plda_pt = x.plda_pt; m.plda_psi = be.plda_psi;
    m.R = x.R; m.D = be.D; m.threshold = be.threshold; m.logdet_given = be.logdet_given; m.logdet_without = be.logdet_without;
    hipLaunchKernelGGL(iv_tail_kernel, dim3(a.B), dim3(kTlThreads), 0, s, m, a.ivec, a.y, a.loss, a.coef, a.emb, a.scores, a.decisions,
                       a.loss_out, a.dw);
    return hipGetLastError();
}

}  // namespace sg
