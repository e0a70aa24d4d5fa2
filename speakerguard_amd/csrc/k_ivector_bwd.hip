// GMM / i-vector / PLDA system, the hand-coded gradient: d loss / d x from d loss / d i-vector (the tail's own adjoint sits
// behind its forward in k_ivector.hip's iv_tail_kernel) back to the CMVN features, the delta rows and the raw cepstra.  The
// adjoint of every stage of k_ivector.hip's header, in the backward's order; x is an utterance's (F, 72) CMVN features.
//
// CONTRACT (the library's): no float atomics; every sum of an utterance runs in an order fixed by C, R and F alone, so an
// utterance's gradient is bit-identical whatever B, its row in the call, or the chunk it lands in.  A chunk's backward runs
// right after that chunk's forward, on the chunk's workspace (the Cholesky factor, ll, the row maxima and sums are the state).
//
// 2. iv_solve_bwd_kernel (one block per utterance): w = L^-1 lin, so with dw = d loss / d w
//      lambda = L^-1 dw   (L symmetric: G z = dw, G^T lambda = z on the factor the forward left in Lmat, float64)
//      d lin = lambda,   d L = -lambda s^T,   s = w + offset e0 (the solved vector, kept by the forward's solve).
//    U_c is kept as its upper triangle, so what the assembly adjoint needs is dLsym[p(i, j)] = -(lambda_i s_j + lambda_j s_i)
//    for i < j and -lambda_i s_i on the diagonal; the kernel writes it over the factor (zero past P).
// 3. iv_rowdot_kernel, twice: out[b][row] = sum_k T[row][k] v[b][k] with float64 accumulators, k ascending inside slices of a
//    fixed length, the slices added in order:
//      d n[c]    = sum_p U_c[p] dLsym[p]            (T = U,  k = p < P, slices of kIvDnSlice, iv_slice_sum_kernel adds them)
//      d f[c][d] = sum_r Vt[c 72 + d][r] lambda_r   (T = Vt, k = r < R, one slice)
//    A block keeps 16 utterances' accumulators per row, so U and Vt are streamed once per 16 rows of the call, like the forward.
// 4. iv_dgamma_kernel + iv_dll_kernel: n_c = sum_t post[t][c], f_c = sum_t post[t][c] x_t, post = softmax(ll):
//      dgamma[t][c] = d n_c + d f_c . x_t     (K = 73: the forward's "entry 72 = 1" row; a float32 fmaf chain, k ascending)
//      r_t = sum_c post[t][c] dgamma[t][c]    (float64: lane-strided, then the xor butterfly -- the forward's row sum order)
//      dll[t][c] = post[t][c] (dgamma[t][c] - r_t),   post rebuilt as expf(ll - mx_t) / fl(s_t), the forward's expression.
//    dll overwrites dgamma in a (frames, Cp) buffer of its own (zero past C); ll stays, step 5 rebuilds post from it once more.
// 5. iv_dx_post_kernel + iv_dx_quad_kernel:
//      dx_t = sum_c post[t][c] d f_c  +  sum_c dll[t][c] (mi_c - S_c x_t)
//    The first sum: float64 accumulators, c ascending.  The second is the forward's contraction transposed,
//      dz[t][k] = sum_c dll[t][c] W_c[k]      (frames x 2700, K = C) on v_mfma_f32_32x32x2_f32,
//    folded against x: linear k = i: dx_i += dz_i;  k = (i, j), i < j: dx_i += dz_ij x_j, dx_j += dz_ij x_i;  k = (i, i): dx_i += 2
//    dz_ii x_i.  dz is NOT written to global memory (37.5 x the size of x): a block owns 64 frames of one utterance and walks the
//    2700 columns in tiles of 128; a tile's dz goes to LDS and every (frame, column i) owner adds what the tile holds for it -- its
//    row part (k = (i, j), j ascending), then its column part (k = (i', i), i' ascending), then its linear entry -- into a
//    register, tile after tile; four blocks share an utterance's 22 tiles (6, 6, 6, 4) and iv_dx_post_kernel adds their partial
//    sums to the first sum in order.  The k chain of an accumulator is a float32 fmaf chain over c in the order c0, c0 + 4, c0 + 1,
//    c0 + 5, .. of each group of 8 (a lane loads 4 adjacent components: 16-byte loads of both operands), flushed into float64
//    totals every 256 components.  No (frames, C, 72) intermediate exists.
// 6. iv_delta_cmvn_bwd_kernel (one block per utterance): the transposes of k_ivector.hip's step 1,
//      d delta[f] = d cmvn[f] + sum_{t : ws_t <= f < we_t} d cmvn[t] fl(-1 / (we_t - ws_t))      (t ascending, float64, rounded once)
//      d raw[f][c] = d delta[f][c] + sum_t sum_j [clamp(t + j) = f] (s1[j] d delta[t][24 + c] + s2[j] d delta[t][48 + c])
//    so that an edge frame collects every clamped tap (t ascending, the 7 taps then the 13, float64, rounded once).
#include <cmath>

#include "sg_internal.h"
#include "wave_reduce.h"

namespace sg {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSbThreads = 256;
__global__ __launch_bounds__(kSbThreads) void iv_solve_bwd_kernel(double* __restrict__ Lmat, int Pp, int P, int R,
                                                                  const float* __restrict__ dw, const double* __restrict__ solved,
                                                                  double* __restrict__ lam) {
    __shared__ double vec[kIvMaxR];
    __shared__ double sv[kIvMaxR];
    __shared__ double red[kSbThreads / 64];
    constexpr int NT = kSbThreads;
    const int tid = threadIdx.x, b = blockIdx.x;
    double* A = Lmat + (size_t)b * Pp;
    const auto off = [R](int j) { return (size_t)j * R - (size_t)j * (j - 1) / 2; };
    for (int i = tid; i < R; i += NT) {
        vec[i] = (double)dw[(size_t)b * R + i];
        sv[i] = solved[(size_t)b * R + i];
    }
    __syncthreads();
    // G z = dw, then G^T lambda = z: the forward's two sweeps (k_ivector.hip, iv_solve_kernel), word for word
    for (int j = 0; j < R; ++j) {
        const double* col = A + off(j);
        const double yj = vec[j] / col[0];
        __syncthreads();
        for (int i = j + 1 + tid; i < R; i += NT) vec[i] -= col[i - j] * yj;
        if (tid == 0) vec[j] = yj;
        __syncthreads();
    }
    for (int j = R - 1; j >= 0; --j) {
        const double* col = A + off(j);
        double part = 0.0;
        for (int i = j + 1 + tid; i < R; i += NT) part += col[i - j] * vec[i];
        const double sum = block_reduce_xor<kSbThreads / 64, true>(part, red, OpSum());
        if (tid == 0) vec[j] = (vec[j] - sum) / col[0];
        __syncthreads();
    }
    for (int i = tid; i < R; i += NT) lam[(size_t)b * R + i] = vec[i];
    // dLsym over the factor (every read of it is behind the last barrier): row i of the packed upper triangle
    for (int i = 0; i < R; ++i) {
        const double li = vec[i], si = sv[i];
        double* row = A + off(i);
        for (int j = i + tid; j < R; j += NT) row[j - i] = j == i ? -(li * si) : -(li * sv[j] + vec[j] * si);
    }
    for (int p = P + tid; p < Pp; p += NT) A[p] = 0.0;
}

// out[b][row] = sum_k T[row * ldT + k] v[b * ldv + k], k in [sl * slice, min(K, (sl + 1) * slice)), k ascending, float64.
// A 64 row x 64 k tile of T and a 16 utterance x 64 k tile of v go through LDS; a thread owns one row and 4 utterances.
constexpr int kRdG = 16;
__global__ __launch_bounds__(256) void iv_rowdot_kernel(const float* __restrict__ T, int nrows, size_t ldT, int K,
                                                        const double* __restrict__ v, size_t ldv, int B, int slice,
                                                        double* __restrict__ outd, float* __restrict__ outf) {
    __shared__ float Ts[64 * 65];
    __shared__ double vs[kRdG * 64];
    const int tid = threadIdx.x, cl = tid & 63, bg = tid >> 6;
    const int r0 = blockIdx.x * 64, sl = blockIdx.y, b0 = blockIdx.z * kRdG, nb = min(kRdG, B - b0);
    const int kbeg = sl * slice, kend = min(K, kbeg + slice);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = kbeg; k0 < kend; k0 += 64) {
        __syncthreads();
        for (int i = tid; i < 64 * 64; i += 256) {
            const int rr = i >> 6, kk = i & 63, row = r0 + rr, k = k0 + kk;
            Ts[rr * 65 + kk] = (row < nrows && k < kend) ? T[(size_t)row * ldT + k] : 0.f;
        }
        for (int i = tid; i < kRdG * 64; i += 256) {
            const int bb = i >> 6, kk = i & 63, k = k0 + kk;
            vs[i] = (bb < nb && k < kend) ? v[(size_t)(b0 + bb) * ldv + k] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < 64; ++kk) {
            const double t = (double)Ts[cl * 65 + kk];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += t * vs[(bg * 4 + q) * 64 + kk];
        }
    }
    const int row = r0 + cl;
    if (row >= nrows) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int bb = bg * 4 + q;
        if (bb >= nb) continue;
        if (outd) outd[((size_t)sl * B + b0 + bb) * nrows + row] = acc[q];
        else outf[(size_t)(b0 + bb) * nrows + row] = (float)acc[q];
    }
}

__global__ __launch_bounds__(256) void iv_slice_sum_kernel(const double* __restrict__ part, int NS, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int sl = 0; sl < NS; ++sl) s += part[(size_t)sl * n + i];
    out[i] = (float)s;
}

constexpr int kDgFrames = 32, kDgLd = kIvDim + 1;
__global__ __launch_bounds__(256) void iv_dgamma_kernel(const float* __restrict__ x, int F, int C, int Cp, const float* __restrict__ dn,
                                                        const float* __restrict__ df, float* __restrict__ dg) {
    __shared__ float xs[kDgFrames * kDgLd];
    __shared__ float ws[64 * kDgLd];
    const int tid = threadIdx.x, cl = tid & 63, fg = tid >> 6;
    const int t0 = blockIdx.x * kDgFrames, c0 = blockIdx.y * 64, b = blockIdx.z;
    for (int i = tid; i < kDgFrames * kDgLd; i += 256) {
        const int tt = i / kDgLd, k = i - tt * kDgLd, t = min(t0 + tt, F - 1);
        xs[i] = k < kIvDim ? x[((size_t)b * F + t) * kIvDim + k] : 1.f;
    }
    for (int i = tid; i < 64 * kDgLd; i += 256) {
        const int cc = i / kDgLd, k = i - cc * kDgLd, c = c0 + cc;
        ws[i] = c >= C ? 0.f : k < kIvDim ? df[((size_t)b * C + c) * kIvDim + k] : dn[(size_t)b * C + c];
    }
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    for (int k = 0; k < kDgLd; ++k) {
        const float w = ws[cl * kDgLd + k];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = fmaf(xs[(fg * 8 + q) * kDgLd + k], w, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int t = t0 + fg * 8 + q;
        if (t < F) dg[((size_t)b * F + t) * Cp + c0 + cl] = acc[q];  // (c0 + cl < Cp: the grid covers exactly Cp)
    }
}

__global__ __launch_bounds__(256) void iv_dll_kernel(const float* __restrict__ ll, const float* __restrict__ rowmax,
                                                     const float* __restrict__ rowsum, int M, int C, int Cp, float* __restrict__ dg) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;  // (a whole wave; the kernel has no barrier)
    const float* row = ll + (size_t)m * C;
    float* g = dg + (size_t)m * Cp;
    const float mx = rowmax[m], sm = rowsum[m];
    double r = 0.0;
    for (int c = lane; c < C; c += 64) r += (double)(expf(row[c] - mx) / sm) * (double)g[c];
    r = wave_sum_xor_steps(r);
    for (int c = lane; c < C; c += 64) g[c] = (expf(row[c] - mx) / sm) * (float)((double)g[c] - r);
}

constexpr int kDpFrames = 32, kDpThreads = 4 * kIvDim;
__global__ __launch_bounds__(kDpThreads) void iv_dx_post_kernel(const float* __restrict__ ll, const float* __restrict__ rowmax,
                                                                const float* __restrict__ rowsum, int F, int C,
                                                                const float* __restrict__ df, const float* __restrict__ dxpart,
                                                                int nsplit, float* __restrict__ dx) {
    __shared__ float gs[kDpFrames * 65];
    __shared__ float dfs[64 * kIvDim];
    const int tid = threadIdx.x, d = tid % kIvDim, fg = tid / kIvDim;
    const int t0 = blockIdx.x * kDpFrames, b = blockIdx.y;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    for (int c0 = 0; c0 < C; c0 += 64) {
        __syncthreads();
        for (int i = tid; i < kDpFrames * 64; i += kDpThreads) {
            const int tt = i >> 6, cc = i & 63, t = t0 + tt, c = c0 + cc;
            const size_t m = (size_t)b * F + min(t, F - 1);
            gs[tt * 65 + cc] = (t < F && c < C) ? expf(ll[m * C + c] - rowmax[m]) / rowsum[m] : 0.f;
        }
        for (int i = tid; i < 64 * kIvDim; i += kDpThreads) {
            const int cc = i / kIvDim, c = c0 + cc;
            dfs[i] = c < C ? df[((size_t)b * C + c) * kIvDim + (i - cc * kIvDim)] : 0.f;
        }
        __syncthreads();
        for (int cc = 0; cc < 64; ++cc) {
            const double w = (double)dfs[cc * kIvDim + d];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] += (double)gs[(fg * 8 + q) * 65 + cc] * w;
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int t = t0 + fg * 8 + q;
        if (t >= F) continue;
        const size_t o = ((size_t)b * F + t) * kIvDim + d;
        float v = (float)acc[q];  // the posterior term, then the log-likelihood term's partial sums in order
        for (int z = 0; z < nsplit; ++z) v += dxpart[(size_t)z * gridDim.y * F * kIvDim + o];
        dx[o] = v;
    }
}

constexpr int kDqRows = 64, kDqTile = 128, kDqXld = kIvDim + 1, kDqZld = kDqTile + 1, kDqFlush = 32;  // 32 groups of 8 components
constexpr int kDqItems = kDqRows * kIvDim / 256;                                                     // 18 (frame, column) owners a thread
constexpr int kDqSplit = kIvDxSplit, kDqTilesPerSplit = ((kIvK + kDqTile - 1) / kDqTile + kDqSplit - 1) / kDqSplit;  // 22 tiles: 6, 6, 6, 4
static_assert(kDqRows * kIvDim % 256 == 0, "whole owners");
__device__ __forceinline__ int iv_zrow(int i) { return kIvDim + i * kIvDim - i * (i - 1) / 2; }  // k of (i, i); row i ends 72 - i later
__global__ __launch_bounds__(256) void iv_dx_quad_kernel(const float* __restrict__ x, int F, const float* __restrict__ W, int Cp,
                                                         const float* __restrict__ dll, float* __restrict__ dxpart) {
    __shared__ float xs[kDqRows * kDqXld];
    __shared__ float dzs[kDqRows * kDqZld];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int t0 = blockIdx.x * kDqRows, b = blockIdx.y;
    for (int i = tid; i < kDqRows * kDqXld; i += 256) {
        const int row = i / kDqXld, col = i - row * kDqXld, t = min(t0 + row, F - 1);  // rows past the utterance repeat its last
        xs[i] = col < kIvDim ? x[((size_t)b * F + t) * kIvDim + col] : 1.f;            // frame; they are not stored
    }
    const float* a0p = dll + ((size_t)b * F + min(t0 + r, F - 1)) * Cp + 4 * h;
    const float* a1p = dll + ((size_t)b * F + min(t0 + 32 + r, F - 1)) * Cp + 4 * h;
    float fold[kDqItems];
#pragma unroll
    for (int mm = 0; mm < kDqItems; ++mm) fold[mm] = 0.f;
    // blockIdx.z: one of kDqSplit runs of kDqTilesPerSplit column tiles (a constant of the arithmetic: the runs' partial sums are
    // added in order by iv_dx_post_kernel); 5 x B blocks alone left three quarters of the chip's wave slots empty at B = 64
    const int nbeg = blockIdx.z * kDqTilesPerSplit * kDqTile, nend = min(kIvK, nbeg + kDqTilesPerSplit * kDqTile);
    for (int n0 = nbeg; n0 < nend; n0 += kDqTile) {
        const int n1 = min(n0 + kDqTile, kIvK);
        // a wave owns 64 frames x 32 columns of the tile; columns past 2700 repeat the last one and are never folded
        const float* wp = W + (size_t)min(n0 + wave * 32 + r, kIvK - 1) * Cp + 4 * h;
        f32x16 acc0, acc1;
        double tot0[16], tot1[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) tot0[e] = tot1[e] = 0.0;
        for (int cg = 0; cg < Cp / 8; cg += kDqFlush) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc0[e] = acc1[e] = 0.f;
            const int cge = min(cg + kDqFlush, Cp / 8);
            for (int g = cg; g < cge; ++g) {
                const float4 a0 = *reinterpret_cast<const float4*>(a0p + 8 * g);
                const float4 a1 = *reinterpret_cast<const float4*>(a1p + 8 * g);
                const float4 bw = *reinterpret_cast<const float4*>(wp + 8 * g);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, bw.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, bw.x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, bw.y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, bw.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, bw.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, bw.z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, bw.w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, bw.w, acc1, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                tot0[e] += (double)acc0[e];
                tot1[e] += (double)acc1[e];
            }
        }
        __syncthreads();  // the last tile's fold has read dzs (and, the first time, xs is complete)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = (e & 3) + 8 * (e >> 2) + 4 * h;  // lane l holds column l & 31, rows (e & 3) + 8 (e >> 2) + 4 (l >> 5)
            dzs[row * kDqZld + wave * 32 + r] = (float)tot0[e];
            dzs[(32 + row) * kDqZld + wave * 32 + r] = (float)tot1[e];
        }
        __syncthreads();
#pragma unroll
        for (int mm = 0; mm < kDqItems; ++mm) {
            const int t = lane, i = wave + 4 * mm;  // owner (frame t, column i): i is the same on every lane of the wave
            const float* dz = dzs + t * kDqZld - n0;
            const float* xt = xs + t * kDqXld;
            float a = fold[mm];
            const int zi = iv_zrow(i);
            for (int k = max(n0, zi); k < min(n1, zi + kIvDim - i); ++k) {  // row part: k = (i, j), j = i + k - zi
                const float v = dz[k] * xt[i + k - zi];
                a += k == zi ? v + v : v;
            }
            for (int i2 = 0; i2 < i; ++i2) {  // column part: k = (i2, i)
                const int k = iv_zrow(i2) + i - i2;
                if (k >= n0 && k < n1) a += dz[k] * xt[i2];
            }
            if (i >= n0 && i < n1) a += dz[i];  // the linear entry
            fold[mm] = a;
        }
    }
#pragma unroll
    for (int mm = 0; mm < kDqItems; ++mm) {
        const int t = t0 + lane, i = wave + 4 * mm;
        if (t < F) dxpart[(((size_t)blockIdx.z * gridDim.y + b) * F + t) * kIvDim + i] = fold[mm];
    }
}

constexpr int kDcbThreads = 1024;
__global__ __launch_bounds__(kDcbThreads) void iv_delta_cmvn_bwd_kernel(const float* __restrict__ dout, int from_cmvn, int F,
                                                                        IvDeltaScales sc, float* __restrict__ ddelta,
                                                                        float* __restrict__ draw, int ld) {
    const int b = blockIdx.x, n = F * kIvDim;
    const float* dd = from_cmvn ? ddelta + (size_t)b * n : dout + (size_t)b * n;
    if (from_cmvn) {
        const float* dc = dout + (size_t)b * n;
        float* o = ddelta + (size_t)b * n;
        for (int idx = threadIdx.x; idx < n; idx += kDcbThreads) {
            const int f = idx / kIvDim, col = idx - f * kIvDim;
            double acc = 0.0;
            for (int t = max(0, f - kCmnWindow); t <= min(F - 1, f + kCmnWindow); ++t) {
                int ws = t - kCmnWindow / 2, we = ws + kCmnWindow;  // the forward's window of frame t
                if (ws < 0) { we -= ws; ws = 0; }
                if (we > F) { ws -= we - F; we = F; if (ws < 0) ws = 0; }
                if (f >= ws && f < we) acc += (double)dc[t * kIvDim + col] * (double)(-1.f / (float)(we - ws));
            }
            o[idx] = (float)((double)dc[idx] + acc);
        }
        if (!draw) return;
        __syncthreads();  // the block reads back its own rows
    }
    if (!draw) return;
    float* o = draw + (size_t)b * F * ld;
    for (int idx = threadIdx.x; idx < F * ld; idx += kDcbThreads) {
        const int f = idx / ld, c = idx - f * ld;
        if (c >= kIvCep) { o[idx] = 0.f; continue; }
        double acc = (double)dd[f * kIvDim + c];
        for (int t = max(0, f - 6); t <= min(F - 1, f + 6); ++t) {
            for (int j = -3; j <= 3; ++j)
                if (min(max(t + j, 0), F - 1) == f) acc += (double)dd[t * kIvDim + kIvCep + c] * (double)sc.s1[j + 3];
            for (int j = -6; j <= 6; ++j)
                if (min(max(t + j, 0), F - 1) == f) acc += (double)dd[t * kIvDim + 2 * kIvCep + c] * (double)sc.s2[j + 6];
        }
        o[idx] = (float)acc;
    }
}

}  // namespace

hipError_t launch_iv_extract_bwd(const IvModel& m, const float* dw, int B, double* Lmat, const double* solved, double* lam, double* dnpart,
                                 float* dn, float* df, hipStream_t s) {
    const int NS = iv_dn_slices(m.P), G = (B + kRdG - 1) / kRdG;
    hipLaunchKernelGGL(iv_solve_bwd_kernel, dim3(B), dim3(kSbThreads), 0, s, Lmat, m.Pp, m.P, m.R, dw, solved, lam);
    hipLaunchKernelGGL(iv_rowdot_kernel, dim3((m.C + 63) / 64, NS, G), dim3(256), 0, s, m.U, m.C, (size_t)m.Pp, m.P,
                       (const double*)Lmat, (size_t)m.Pp, B, kIvDnSlice, dnpart, (float*)nullptr);
    const size_t n = (size_t)B * m.C;
    hipLaunchKernelGGL(iv_slice_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)dnpart, NS, n, dn);
    hipLaunchKernelGGL(iv_rowdot_kernel, dim3((m.C * kIvDim + 63) / 64, 1, G), dim3(256), 0, s, m.Vt, m.C * kIvDim, (size_t)m.R, m.R,
                       (const double*)lam, (size_t)m.R, B, m.R, (double*)nullptr, df);
    return hipGetLastError();
}

hipError_t launch_iv_stats_bwd(const IvModel& m, const float* cmvn, int B, int F, const float* ll, const float* rowmax, const float* rowsum,
                               const float* dn, const float* df, float* dg, float* dxpart, float* dx, hipStream_t s) {
    const int M = B * F;
    hipLaunchKernelGGL(iv_dgamma_kernel, dim3((F + kDgFrames - 1) / kDgFrames, m.Cp / 64, B), dim3(256), 0, s, cmvn, F, m.C, m.Cp, dn, df,
                       dg);
    hipLaunchKernelGGL(iv_dll_kernel, dim3((M + 3) / 4), dim3(256), 0, s, ll, rowmax, rowsum, M, m.C, m.Cp, dg);
    hipLaunchKernelGGL(iv_dx_quad_kernel, dim3((F + kDqRows - 1) / kDqRows, B, kDqSplit), dim3(256), 0, s, cmvn, F, m.W, m.Cp,
                       (const float*)dg, dxpart);
    hipLaunchKernelGGL(iv_dx_post_kernel, dim3((F + kDpFrames - 1) / kDpFrames, B), dim3(kDpThreads), 0, s, ll, rowmax, rowsum, F, m.C, df,
                       (const float*)dxpart, kDqSplit, dx);
    return hipGetLastError();
}

hipError_t launch_iv_delta_cmvn_bwd(const float* dout, bool from_cmvn, int B, int F, float* ddelta, float* draw, int ld, hipStream_t s) {
    hipLaunchKernelGGL(iv_delta_cmvn_bwd_kernel, dim3(B), dim3(kDcbThreads), 0, s, dout, from_cmvn ? 1 : 0, F, iv_delta_scales(), ddelta,
                       draw, ld);
    return hipGetLastError();
}

}  // namespace sg
