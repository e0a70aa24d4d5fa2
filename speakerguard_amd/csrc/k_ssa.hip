// Singular spectrum analysis of whole utterances (reference attack/_kenan.py ssa_compression :86-112 and attack/ssa_core.py ssa /
// inv_ssa) for Kenan's `ssa` variant, without the trajectory matrix.  T samples, window W = min(int(0.05 T), 3000), t = T - W + 1
// lagged rows; everything after the quantisation is float64 (or exact integers), the grid's outer dimension is the utterance,
// and what an utterance computes depends on (T, its samples, its rank) alone: a batch equals its utterances run alone, bit for bit.
//
// sg_ssa_decompose
//   quantise (attack/Kenan.py:31-34), one workgroup per utterance: mx / mn = the row's largest / smallest sample; when
//     0.9f * mx <= 1 and 0.9f * mn >= -1 (float32) every sample is multiplied by 2^(bits-1) in float32.  The value goes to int32
//     toward zero (NaN: 0; beyond the int32 range: the nearest end) and its low 16 bits are the int16 sample: a value outside the
//     int16 range WRAPS, as the reference's `astype(np.int16)` does on the hosts it was run on.
//   lag covariance C[a][b] = sum_{p<t} x[p+a] x[p+b], exact in int64: the first row as W block reductions (integer sums: any order
//     gives the same bits), then every diagonal as a scan C[a+1][b+1] = C[a][b] - x[a] x[b] + x[a+t] x[b+t], one thread per
//     diagonal.  |C| <= t 2^30 < 2^53: the float64 copy the iteration starts from is exact.
//   eigenvectors by a two-sided cyclic Jacobi iteration, round-robin pairing: n = W rounded up to even (an odd W gets the idle
//     index W), round r of n - 1 pairs index n-1 with r and (r + k) mod (n-1) with (r - k) mod (n-1) for k = 1 .. n/2 - 1.  A round
//     is three launches, and no block ever waits for another:
//       (a) ssa_rot_kernel   per pair (p < q): skip when a_pq == 0 or |a_pq| <= 2^-52 sqrt(|a_pp a_qq|); else theta = (a_qq - a_pp) /
//                            (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c (t == 0,
//                            |theta| beyond 1e154: skipped as well); a'_pp = a_pp - t a_pq, a'_qq = a_qq + t a_pq.  Applied
//                            rotations are counted per utterance (an integer atomic).
//       (b) ssa_cols_kernel  A <- A J, V <- V J: one row per block, held in LDS; column p' = c p - s q, column q' = s p + c q.
//       (c) ssa_rows_kernel  A <- J^T A: one pair per block on its two whole rows, same formulas; the four entries of the pair's
//                            own 2 x 2 block are SET: a'_pp, a'_qq from (a) and exact zeros off the diagonal.
//     After a sweep (n - 1 rounds) the host reads the counters (one stream synchronisation per sweep); an utterance is done after
//     a sweep without a rotation and is skipped from then on (its matrices would not change any more: which other utterances
//     share the call cannot show in its result).  sweeps[b] = the sweeps that rotated.  30 sweeps without convergence: SG_ERR_STATE.
//   the eigenvalues are the diagonal the iteration ends on.  The ~W/2 x sweeps rotations every entry of V went through leave
//     V^T V - I at some hundred ulp (measured 5e-14 at W = 200, 3e-13 at W = 800), and a projector built from such a V carries that
//     error into every sample; one Newton-Schulz step V <- V (1.5 I - 0.5 V^T V) (ssa_atb_kernel, twice) brings it back to the
//     rounding of one W-term inner product.
//   order: rank of eigenvalue i = the number of j with l_j > l_i, or l_j == l_i and j < i (descending, ties by index);
//     evec[rank][.] = column i of V: the ROWS of evec are the eigenvectors.
//
// sg_ssa_reconstruct, rank k[b] per utterance
//   P = V_k V_k^T:   P[i][l] = sum_{j<k} evec[j][i] evec[j][l], one fma chain per element, j ascending from 0 (ssa_atb_kernel).
//   taps:            h[d] = sum_{l-i=d} P[i][l], d = -(W-1) .. W-1: lane u of one wave sums the terms i = i0 + u, i0 + u + 64, ... in
//                    ascending order (fma-free adds), then the 64 partials meet in a xor butterfly (32, 16, .., 1).
//   interior  W-1 <= m <= t-1:   z[m] = sum_d h[d] x[m+d], one fma chain, d ascending from -(W-1).
//   edges     otherwise:         z[m] = sum_{i: 0 <= m-i < t} sum_l x[m-i+l] P[i][l]: thread u of 256 takes l = u, u + 256, ... and
//                    runs one fma chain over (i ascending, l ascending); the partials meet in a xor butterfly per wave and the
//                    four waves' sums are added in wave order.
//   z[m] / min(m+1, W, T-m) (the reference's two sqrt(t) factors cancel), to int32 toward zero, low 16 bits, written as float32;
//   optionally the float64 quotient itself.
#include <cmath>
#include <cstring>

#include "sg_internal.h"
#include "wave_reduce.h"

using namespace sg;

namespace {

constexpr int kSsaMaxW = 3000;
constexpr int kSsaMinT = 20;
constexpr int kSsaMaxT = 1 << 22;
constexpr int kSsaMaxB = 65535;
constexpr int kSsaMaxSweeps = 30;
constexpr int kSsaThreads = 256;
constexpr int kSsaPutK = 64;

struct SsaRot {
    double c, s, app, aqq;  // s == 0: no rotation
};
struct SsaKChunk {
    int32_t v[kSsaPutK];
};

int ssa_window(int T) {
    if (T < kSsaMinT || T > kSsaMaxT) return -1;
    const int w = (int)((double)T * 0.05);
    return w > kSsaMaxW ? kSsaMaxW : w;
}

// round r (0 .. n-2) of the round-robin over n (even) indices, pair k (0 .. n/2-1): p < q
__host__ __device__ inline void ssa_pair(int n, int r, int k, int* p, int* q) {
    int a, b;
    if (k == 0) {
        a = n - 1, b = r;
    } else {
        a = (r + k) % (n - 1), b = (r + (n - 1) - k) % (n - 1);
    }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

__device__ __forceinline__ int ssa_trunc_i32(double v) {
    if (v != v) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (-2147483647 - 1);
    return (int)v;
}
__device__ __forceinline__ int16_t ssa_low16(int v) { return (int16_t)(uint16_t)((unsigned)v & 0xFFFFu); }

// ---------------------------------------------------------------- quantise: one workgroup per utterance
__global__ void __launch_bounds__(1024) ssa_quantise_kernel(const float* x, int T, float mul, int16_t* xq) {
    __shared__ float red_hi[16], red_lo[16];
    const int tid = threadIdx.x, nt = blockDim.x;
    const float* xr = x + (size_t)blockIdx.x * T;
    int16_t* qr = xq + (size_t)blockIdx.x * T;
    float hi = -INFINITY, lo = INFINITY;
    for (int i = tid; i < T; i += nt) hi = fmaxf(hi, xr[i]), lo = fminf(lo, xr[i]);
    for (int d = 32; d >= 1; d >>= 1) hi = fmaxf(hi, __shfl_xor(hi, d)), lo = fminf(lo, __shfl_xor(lo, d));  // both butterflies in one loop, order 32 .. 1
    if ((tid & 63) == 0) red_hi[tid >> 6] = hi, red_lo[tid >> 6] = lo;
    __syncthreads();
    hi = red_hi[0], lo = red_lo[0];
    for (int w = 1; w < (nt + 63) / 64; ++w) hi = fmaxf(hi, red_hi[w]), lo = fminf(lo, red_lo[w]);
    const bool scale = 0.9f * hi <= 1.f && 0.9f * lo >= -1.f;
    for (int i = tid; i < T; i += nt) {
        const float v = scale ? xr[i] * mul : xr[i];
        qr[i] = ssa_low16(ssa_trunc_i32((double)v));
    }
}

// ---------------------------------------------------------------- lag covariance
// grid (W, B): row0[b][lag] = sum_{p<t} x[p] x[p+lag]
__global__ void __launch_bounds__(kSsaThreads) ssa_cov_row_kernel(const int16_t* xq, int T, int W, long long* row0) {
    __shared__ long long red[kSsaThreads / 64];
    const int tid = threadIdx.x, lag = blockIdx.x, t = T - W + 1;
    const int16_t* x = xq + (size_t)blockIdx.y * T;
    long long acc = 0;
    for (int p = tid; p < t; p += kSsaThreads) acc += (long long)((int)x[p] * (int)x[p + lag]);
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);  // order 32 .. 1 (wave_sum_xor selects other instructions for this loop)
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kSsaThreads / 64; ++w) acc += red[w];
        row0[(size_t)blockIdx.y * W + lag] = acc;
    }
}

// grid (ceil(W / 256), B): thread d walks diagonal d of C into A (both triangles), the identity into V, C into cov (optional)
__global__ void __launch_bounds__(kSsaThreads) ssa_cov_diag_kernel(const int16_t* xq, int T, int W, const long long* row0, double* A,
                                                                   double* V, double* cov) {
    const int d = blockIdx.x * kSsaThreads + threadIdx.x, t = T - W + 1;
    if (d >= W) return;
    const size_t b = blockIdx.y, ww = (size_t)W * W;
    const int16_t* x = xq + b * T;
    double* Ab = A + b * ww;
    double* Vb = V + b * ww;
    double* Cb = cov ? cov + b * ww : nullptr;
    long long c = row0[b * W + d];
    const double one = d == 0 ? 1.0 : 0.0;
    for (int a = 0; a + d < W; ++a) {
        const double v = (double)c;
        const size_t up = (size_t)a * W + a + d, dn = (size_t)(a + d) * W + a;
        Ab[up] = v, Ab[dn] = v;
        Vb[up] = one, Vb[dn] = one;
        if (Cb) Cb[up] = v, Cb[dn] = v;
        if (a + d + 1 < W) c += (long long)((int)x[a + t] * (int)x[a + d + t]) - (long long)((int)x[a] * (int)x[a + d]);
    }
}

// ---------------------------------------------------------------- one Jacobi round
// (a) grid (ceil(n/2 / 256), B)
__global__ void __launch_bounds__(kSsaThreads) ssa_rot_kernel(const double* A, int W, int n, int r, SsaRot* rot, int* cnt,
                                                              const int* active) {
    const int k = blockIdx.x * kSsaThreads + threadIdx.x, b = blockIdx.y;
    if (k >= n / 2 || !active[b]) return;
    int p, q;
    ssa_pair(n, r, k, &p, &q);
    SsaRot o{1.0, 0.0, 0.0, 0.0};
    if (q < W) {
        const double* Ab = A + (size_t)b * W * W;
        const double app = Ab[(size_t)p * W + p], aqq = Ab[(size_t)q * W + q], apq = Ab[(size_t)p * W + q];
        if (apq != 0.0 && !(fabs(apq) <= 0x1p-52 * sqrt(fabs(app * aqq)))) {
            const double theta = (aqq - app) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (t != 0.0) {
                o.c = 1.0 / sqrt(t * t + 1.0);
                o.s = t * o.c;
                o.app = app - t * apq;
                o.aqq = aqq + t * apq;
                if (o.s != 0.0) atomicAdd(&cnt[b], 1);
            }
        }
    }
    rot[(size_t)b * (n / 2) + k] = o;
}

// (b) grid (2 W, B): block x < W takes row x of A, else row x - W of V
__global__ void __launch_bounds__(kSsaThreads) ssa_cols_kernel(double* A, double* V, int W, int n, int r, const SsaRot* rot,
                                                               const int* active) {
    __shared__ double row[kSsaMaxW];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (!active[b]) return;
    const int bx = blockIdx.x;
    double* g = (bx < W ? A : V) + (size_t)b * W * W + (size_t)(bx < W ? bx : bx - W) * W;
    for (int j = tid; j < W; j += kSsaThreads) row[j] = g[j];
    __syncthreads();
    const SsaRot* rb = rot + (size_t)b * (n / 2);
    for (int k = tid; k < n / 2; k += kSsaThreads) {
        int p, q;
        ssa_pair(n, r, k, &p, &q);
        if (q >= W) continue;
        const SsaRot R = rb[k];
        if (R.s == 0.0) continue;
        const double x = row[p], y = row[q];
        row[p] = R.c * x - R.s * y;
        row[q] = R.s * x + R.c * y;
    }
    __syncthreads();
    for (int j = tid; j < W; j += kSsaThreads) g[j] = row[j];
}

// (c) grid (n / 2, B): block k takes rows p and q of its pair
__global__ void __launch_bounds__(kSsaThreads) ssa_rows_kernel(double* A, int W, int n, int r, const SsaRot* rot, const int* active) {
    const int b = blockIdx.y, k = blockIdx.x;
    if (!active[b]) return;
    int p, q;
    ssa_pair(n, r, k, &p, &q);
    if (q >= W) return;
    const SsaRot R = rot[(size_t)b * (n / 2) + k];
    if (R.s == 0.0) return;
    double* Ap = A + (size_t)b * W * W + (size_t)p * W;
    double* Aq = A + (size_t)b * W * W + (size_t)q * W;
    for (int j = threadIdx.x; j < W; j += kSsaThreads) {
        const double x = Ap[j], y = Aq[j];
        double np = R.c * x - R.s * y, nq = R.s * x + R.c * y;
        if (j == p) np = R.app, nq = 0.0;
        if (j == q) np = 0.0, nq = R.aqq;
        Ap[j] = np, Aq[j] = nq;
    }
}

// ---------------------------------------------------------------- ordering
// grid (ceil(W / 256), B)
__global__ void __launch_bounds__(kSsaThreads) ssa_rank_kernel(const double* A, int W, int* rank, double* eval) {
    const int i = blockIdx.x * kSsaThreads + threadIdx.x;
    if (i >= W) return;
    const size_t b = blockIdx.y;
    const double* Ab = A + b * W * W;
    const double li = Ab[(size_t)i * W + i];
    int before = 0;
    for (int j = 0; j < W; ++j) {
        const double lj = Ab[(size_t)j * W + j];
        before += (lj > li || (lj == li && j < i)) ? 1 : 0;
    }
    rank[b * W + i] = before;
    eval[b * W + before] = li;
}

// grid (ceil(W / 32), ceil(W / 32), B), block 32 x 8: out[c][i] = V[i][c]
__global__ void __launch_bounds__(256) ssa_transpose_kernel(const double* V, int W, double* evec) {
    __shared__ double tile[32][33];
    const size_t b = blockIdx.z;
    const double* Vb = V + b * W * W;
    double* Eb = evec + b * W * W;
    const int c0 = blockIdx.x * 32, i0 = blockIdx.y * 32, tx = threadIdx.x, ty = threadIdx.y;
    for (int y = ty; y < 32; y += 8)
        if (i0 + y < W && c0 + tx < W) tile[y][tx] = Vb[(size_t)(i0 + y) * W + c0 + tx];
    __syncthreads();
    for (int y = ty; y < 32; y += 8) {
        const int c = c0 + y, i = i0 + tx;
        if (c < W && i < W) Eb[(size_t)c * W + i] = tile[tx][y];
    }
}

// ---------------------------------------------------------------- reconstruction
__global__ void ssa_put_k_kernel(SsaKChunk vals, int n, int32_t* k_dev) {
    if ((int)threadIdx.x < n) k_dev[threadIdx.x] = vals.v[threadIdx.x];
}

// grid (ceil(W / 32), ceil(W / 32), B), block 16 x 16, 2 x 2 elements per thread: out[i][l] = sum_{j<k} X[j][i] Y[j][l], one fma
// chain per element, j ascending from 0; k = k_dev[b], or k_const when k_dev is null.  newton: out = 1.5 [i == l] - 0.5 sum instead.
__global__ void __launch_bounds__(256) ssa_atb_kernel(const double* X, const double* Y, const int32_t* k_dev, int k_const, int W,
                                                      double* out, int newton) {
    __shared__ double Xs[32][33], Ys[32][33];  // [j][i], [j][l]
    const size_t b = blockIdx.z;
    const double* Xb = X + b * W * W;
    const double* Yb = Y + b * W * W;
    const int k = k_dev ? k_dev[b] : k_const;
    const int l0 = blockIdx.x * 32, i0 = blockIdx.y * 32, tx = threadIdx.x, ty = threadIdx.y, tid = ty * 16 + tx;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int j0 = 0; j0 < k; j0 += 32) {
        for (int e = tid; e < 32 * 32; e += 256) {
            const int jj = e >> 5, cc = e & 31, j = j0 + jj;
            Xs[jj][cc] = (j < k && i0 + cc < W) ? Xb[(size_t)j * W + i0 + cc] : 0.0;
            Ys[jj][cc] = (j < k && l0 + cc < W) ? Yb[(size_t)j * W + l0 + cc] : 0.0;
        }
        __syncthreads();
        const int jn = k - j0 < 32 ? k - j0 : 32;
        for (int jj = 0; jj < jn; ++jj) {
            const double a0 = Xs[jj][ty], a1 = Xs[jj][ty + 16], b0 = Ys[jj][tx], b1 = Ys[jj][tx + 16];
            acc[0][0] = fma(a0, b0, acc[0][0]);
            acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]);
            acc[1][1] = fma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    double* Ob = out + b * W * W;
    for (int u = 0; u < 2; ++u)
        for (int v = 0; v < 2; ++v) {
            const int i = i0 + ty + 16 * u, l = l0 + tx + 16 * v;
            if (i < W && l < W) Ob[(size_t)i * W + l] = newton ? (i == l ? 1.5 : 0.0) - 0.5 * acc[u][v] : acc[u][v];
        }
}

// grid (W, B): dst[rank[c]][.] = src[c][.]
__global__ void __launch_bounds__(kSsaThreads) ssa_sort_rows_kernel(const double* src, const int* rank, int W, double* dst) {
    const size_t b = blockIdx.y;
    const int c = blockIdx.x;
    const double* s = src + b * W * W + (size_t)c * W;
    double* d = dst + b * W * W + (size_t)rank[b * W + c] * W;
    for (int i = threadIdx.x; i < W; i += kSsaThreads) d[i] = s[i];
}

// grid (2 W - 1, B), one wave: h[d + W - 1] = sum_{l - i = d} P[i][l]
__global__ void __launch_bounds__(64) ssa_taps_kernel(const double* P, int W, double* h) {
    const size_t b = blockIdx.y;
    const int d = (int)blockIdx.x - (W - 1);
    const int i_lo = d < 0 ? -d : 0, i_hi = d < 0 ? W - 1 : W - 1 - d;  // 0 <= i, i + d <= W - 1
    const double* Pb = P + b * W * W;
    double acc = 0.0;
    for (int i = i_lo + (int)threadIdx.x; i <= i_hi; i += 64) acc += Pb[(size_t)i * W + i + d];
    acc = wave_sum_xor(acc);
    if (threadIdx.x == 0) h[b * (2 * (size_t)W - 1) + blockIdx.x] = acc;
}

__device__ __forceinline__ void ssa_emit(double z, int m, int T, int W, float* out, double* out64, size_t at) {
    const int left = m + 1, right = T - m;
    const int times = left < W ? (left < right ? left : right) : (W < right ? W : right);
    const double q = z / (double)times;
    out[at] = (float)ssa_low16(ssa_trunc_i32(q));
    if (out64) out64[at] = q;
}

// grid (ceil((T - 2 W + 2) / 256), B): the samples W-1 .. t-1
__global__ void __launch_bounds__(kSsaThreads) ssa_interior_kernel(const int16_t* xq, const double* h, int T, int W, float* out,
                                                                   double* out64) {
    __shared__ double hs[2 * kSsaMaxW - 1];
    const size_t b = blockIdx.y;
    const int nh = 2 * W - 1;
    for (int j = threadIdx.x; j < nh; j += kSsaThreads) hs[j] = h[b * nh + j];
    __syncthreads();
    const int m = W - 1 + blockIdx.x * kSsaThreads + threadIdx.x;
    if (m > T - W) return;
    const int16_t* x = xq + b * T + (m - (W - 1));
    double acc = 0.0;
    for (int j = 0; j < nh; ++j) acc = fma(hs[j], (double)x[j], acc);
    ssa_emit(acc, m, T, W, out, out64, b * T + m);
}

// grid (2 (W - 1), B): block e < W-1 takes sample e, else sample t + e - (W-1)
__global__ void __launch_bounds__(kSsaThreads) ssa_edge_kernel(const int16_t* xq, const double* P, int T, int W, float* out,
                                                               double* out64) {
    __shared__ double red[kSsaThreads / 64];
    const size_t b = blockIdx.y;
    const int e = blockIdx.x, t = T - W + 1, tid = threadIdx.x;
    const int m = e < W - 1 ? e : t + (e - (W - 1));
    const int i_lo = m - t + 1 > 0 ? m - t + 1 : 0, i_hi = m < W - 1 ? m : W - 1;
    const int16_t* x = xq + b * T;
    const double* Pb = P + b * W * W;
    double acc = 0.0;
    for (int i = i_lo; i <= i_hi; ++i) {
        const int16_t* xu = x + (m - i);  // 0 <= m - i < t: xu[l] stays below T for l < W
        const double* Pi = Pb + (size_t)i * W;
        for (int l = tid; l < W; l += kSsaThreads) acc = fma((double)xu[l], Pi[l], acc);
    }
    acc = wave_sum_xor(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kSsaThreads / 64; ++w) acc += red[w];
        ssa_emit(acc, m, T, W, out, out64, b * T + m);
    }
}

int ssa_launched(sg_ctx* ctx, const char* who) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return SG_OK;
}

}  // namespace

extern "C" int32_t sg_ssa_window(int32_t T) { return ssa_window(T); }

extern "C" int sg_ssa_decompose(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, int32_t bits, int16_t* xq_dev, double* eval_dev,
                                double* evec_dev, int32_t* sweeps_dev, double* cov_dev, void* stream) {
    const char* who = "sg_ssa_decompose";
    if (!ctx) return SG_ERR_ARG;
    if (!x_dev || !xq_dev || !eval_dev || !evec_dev || !sweeps_dev) return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    const int W = ssa_window(T);
    if (B < 1 || B > kSsaMaxB || W < 1)
        return fail(ctx, SG_ERR_ARG, "%s: need 1 <= B <= %d and %d <= T <= %d (B %d, T %d)", who, kSsaMaxB, kSsaMinT, kSsaMaxT, B, T);
    if (bits < 1 || bits > 16) return fail(ctx, SG_ERR_ARG, "%s: bits must lie in 1 .. 16 (%d)", who, bits);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    hipStream_t s = (hipStream_t)stream;
    const int n = W + (W & 1), half = n / 2;
    const size_t ww = (size_t)W * W;
    // workspace: A, V (B W W each), the rotations (B n/2 x 4), the first row (B W int64); counters and flags (2 B), ranks (B W)
    const size_t need = (size_t)B * (2 * ww + 4 * (size_t)half + W);
    if (int rc = dev_grow(ctx, ctx->model_allocs, &ctx->ssa_ws, need, s)) return rc;
    if (int rc = dev_grow(ctx, ctx->model_allocs, &ctx->ssa_iws, (size_t)B * (2 + (size_t)W), s)) return rc;
    double* A = ctx->ssa_ws.ptr;
    double* V = A + (size_t)B * ww;
    SsaRot* rot = reinterpret_cast<SsaRot*>(V + (size_t)B * ww);
    long long* row0 = reinterpret_cast<long long*>(V + (size_t)B * ww + (size_t)B * 4 * half);
    int* cnt = ctx->ssa_iws.ptr;
    int* active = cnt + B;
    int* rank = active + B;

    hipLaunchKernelGGL(ssa_quantise_kernel, dim3((unsigned)B), dim3(1024), 0, s, x_dev, T, ldexpf(1.f, bits - 1), xq_dev);
    hipLaunchKernelGGL(ssa_cov_row_kernel, dim3((unsigned)W, (unsigned)B), dim3(kSsaThreads), 0, s, (const int16_t*)xq_dev, T, W, row0);
    hipLaunchKernelGGL(ssa_cov_diag_kernel, dim3((unsigned)((W + kSsaThreads - 1) / kSsaThreads), (unsigned)B), dim3(kSsaThreads), 0, s,
                       (const int16_t*)xq_dev, T, W, (const long long*)row0, A, V, cov_dev);
    if (int rc = ssa_launched(ctx, who)) return rc;

    std::vector<int32_t> h_active((size_t)B, 1), h_cnt((size_t)B, 0), h_sweeps((size_t)B, 0);
    int left = B;
    for (int sweep = 0; left > 0; ++sweep) {
        if (sweep == kSsaMaxSweeps)
            return fail(ctx, SG_ERR_STATE, "%s: %d of %d utterances still rotate after %d Jacobi sweeps (W %d)", who, left, B, kSsaMaxSweeps, W);
        SG_HIP(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(int), s));
        SG_HIP(hipMemcpyAsync(active, h_active.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
        for (int r = 0; r < n - 1; ++r) {
            hipLaunchKernelGGL(ssa_rot_kernel, dim3((unsigned)((half + kSsaThreads - 1) / kSsaThreads), (unsigned)B), dim3(kSsaThreads), 0, s,
                               (const double*)A, W, n, r, rot, cnt, (const int*)active);
            hipLaunchKernelGGL(ssa_cols_kernel, dim3((unsigned)(2 * W), (unsigned)B), dim3(kSsaThreads), 0, s, A, V, W, n, r,
                               (const SsaRot*)rot, (const int*)active);
            hipLaunchKernelGGL(ssa_rows_kernel, dim3((unsigned)half, (unsigned)B), dim3(kSsaThreads), 0, s, A, W, n, r, (const SsaRot*)rot,
                               (const int*)active);
        }
        if (int rc = ssa_launched(ctx, who)) return rc;
        SG_HIP(hipMemcpyAsync(h_cnt.data(), cnt, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
        SG_HIP(hipStreamSynchronize(s));  // (also: h_active has been read)
        for (int b = 0; b < B; ++b) {
            if (!h_active[b]) continue;
            if (h_cnt[b] == 0) h_active[b] = 0, --left;
            else ++h_sweeps[b];
        }
    }
    hipLaunchKernelGGL(ssa_rank_kernel, dim3((unsigned)((W + kSsaThreads - 1) / kSsaThreads), (unsigned)B), dim3(kSsaThreads), 0, s,
                       (const double*)A, W, rank, eval_dev);
    const unsigned tiles = (unsigned)((W + 31) / 32);
    // one Newton-Schulz step on the accumulated rotations, V <- V (1.5 I - 0.5 V^T V): A takes M = 1.5 I - 0.5 V^T V, evec_dev
    // V^T for the while, V's place R = M^T V^T = (V M)^T, whose rows go to evec_dev in eigenvalue order
    hipLaunchKernelGGL(ssa_atb_kernel, dim3(tiles, tiles, (unsigned)B), dim3(16, 16), 0, s, (const double*)V, (const double*)V,
                       (const int32_t*)nullptr, W, W, A, 1);
    hipLaunchKernelGGL(ssa_transpose_kernel, dim3(tiles, tiles, (unsigned)B), dim3(32, 8), 0, s, (const double*)V, W, evec_dev);
    hipLaunchKernelGGL(ssa_atb_kernel, dim3(tiles, tiles, (unsigned)B), dim3(16, 16), 0, s, (const double*)A, (const double*)evec_dev,
                       (const int32_t*)nullptr, W, W, V, 0);
    hipLaunchKernelGGL(ssa_sort_rows_kernel, dim3((unsigned)W, (unsigned)B), dim3(kSsaThreads), 0, s, (const double*)V, (const int*)rank, W,
                       evec_dev);
    if (int rc = ssa_launched(ctx, who)) return rc;
    SG_HIP(hipMemcpyAsync(sweeps_dev, h_sweeps.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SG_HIP(hipStreamSynchronize(s));  // h_sweeps leaves scope
    return SG_OK;
}

extern "C" int sg_ssa_reconstruct(sg_ctx* ctx, const int16_t* xq_dev, const double* evec_dev, const int32_t* k_host, int32_t B, int32_t T,
                                  float* out_dev, double* out64_dev, void* stream) {
    const char* who = "sg_ssa_reconstruct";
    if (!ctx) return SG_ERR_ARG;
    if (!xq_dev || !evec_dev || !k_host || !out_dev) return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    const int W = ssa_window(T);
    if (B < 1 || B > kSsaMaxB || W < 1)
        return fail(ctx, SG_ERR_ARG, "%s: need 1 <= B <= %d and %d <= T <= %d (B %d, T %d)", who, kSsaMaxB, kSsaMinT, kSsaMaxT, B, T);
    for (int b = 0; b < B; ++b)
        if (k_host[b] < 1 || k_host[b] > W) return fail(ctx, SG_ERR_ARG, "%s: rank %d of utterance %d outside 1 .. %d", who, k_host[b], b, W);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    hipStream_t s = (hipStream_t)stream;
    const size_t ww = (size_t)W * W, nh = 2 * (size_t)W - 1;
    // workspace: P (B W W), the taps (B (2 W - 1)); the ranks (B)
    if (int rc = dev_grow(ctx, ctx->model_allocs, &ctx->ssa_ws, (size_t)B * (ww + nh), s)) return rc;
    if (int rc = dev_grow(ctx, ctx->model_allocs, &ctx->ssa_iws, (size_t)B, s)) return rc;
    double* P = ctx->ssa_ws.ptr;
    double* h = P + (size_t)B * ww;
    int32_t* k_dev = ctx->ssa_iws.ptr;
    for (int b0 = 0; b0 < B; b0 += kSsaPutK) {  // the ranks travel as launch arguments: nothing of the caller's is read later
        SsaKChunk c{};
        const int nb = B - b0 < kSsaPutK ? B - b0 : kSsaPutK;
        std::memcpy(c.v, k_host + b0, (size_t)nb * sizeof(int32_t));
        hipLaunchKernelGGL(ssa_put_k_kernel, dim3(1), dim3(kSsaPutK), 0, s, c, nb, k_dev + b0);
    }
    const unsigned tiles = (unsigned)((W + 31) / 32);
    hipLaunchKernelGGL(ssa_atb_kernel, dim3(tiles, tiles, (unsigned)B), dim3(16, 16), 0, s, evec_dev, evec_dev, (const int32_t*)k_dev, 0, W,
                       P, 0);
    hipLaunchKernelGGL(ssa_taps_kernel, dim3((unsigned)nh, (unsigned)B), dim3(64), 0, s, (const double*)P, W, h);
    const int interior = T - 2 * W + 2;  // >= 18 W + 2
    hipLaunchKernelGGL(ssa_interior_kernel, dim3((unsigned)((interior + kSsaThreads - 1) / kSsaThreads), (unsigned)B), dim3(kSsaThreads), 0, s,
                       xq_dev, (const double*)h, T, W, out_dev, out64_dev);
    if (W > 1)
        hipLaunchKernelGGL(ssa_edge_kernel, dim3((unsigned)(2 * (W - 1)), (unsigned)B), dim3(kSsaThreads), 0, s, xq_dev, (const double*)P, T,
                           W, out_dev, out64_dev);
    return ssa_launched(ctx, who);
}
