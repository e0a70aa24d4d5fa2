// STOI (Taal, Hendriks, Heusdens, Jensen 2011; the reference's metric/metric.py:50-54 calls pystoi) of B utterance pairs on the
// device, float64 after the float32 samples are read.  DESIGN.md section 4 holds the contract (written from the published
// algorithm, unpinned by pystoi); tests/stoi_restate.py restates it in numpy in the orders below.
//
//   input rule    per row and signal: samples / 2^15 unless -1 <= max <= 1 (metric.py:10-14).
//   resample      fs 16000 only: y[m] = sum_i G[8 m - 5 i] x[i], G = 5 h, h = Octave's 581-tap resample filter for 5/8 (unit sum),
//                 zero-phase, ceil(5 T / 8) samples, zeros outside the signal.  fs 10000: y = x.
//   silent frames frames of the BENIGN y at range(0, n10 - 256, 128) (nF of them), e_f = 20 log10(|w frame_f| + EPS), kept iff
//                 max(e) - 40 - e_f < 0; both signals keep the same K frames; the kept windowed frames are overlap-added at hop 128.
//   spectra       frames of the overlap-added signal at range(0, len - 256, 128): M = K - 1 of them, windowed again, 512-point power.
//   bands         15 one-third-octave bands from 150 Hz: sqrt of the power summed over the band's bins.
//   segments      M < 30: d = 1e-5.  Else J = M - 29 segments of 30 frames per band; per (segment, band): y scaled to x's norm,
//                 clipped at x (1 + 10^(15/20)), both centred and normalised, multiplied and summed; d = total / (15 J).
//
// Launches (all on the caller's stream; nothing returns to the host between them):
//   stoi_scale_kernel     grid (8, 2, B): the maximum of an eighth of one signal's row; the row's scale (1 or 2^-15) follows from the eight.
//   stoi_resample_kernel  grid (tiles, 2, B): a block owns 8 frames = 1152 samples of one signal at 10 kHz (128 of them shared with
//                         the next tile), stages its source samples as scaled float64 in LDS, writes the samples to the workspace
//                         and -- benign signal -- the 8 frame energies, one wave per frame.
//   stoi_mask_kernel      grid B: row maximum of the energies, the mask, its exclusive scan -> the kept frames' indices and K.
//   stoi_bands_kernel     grid (ceil((nF - 1) / 4), B), one wave per output frame m < K - 1: gathers the at most three kept source
//                         frames that overlap it (the overlap-added signal never exists in memory), windows, transforms (fft512.h,
//                         the upper half of the input zero) and writes the 15 band values, for both signals in turn.
//   stoi_segments_kernel  grid B: the segment statistics and the final sum.
//
// Determinism: no atomics, no implicit contraction (the only fused multiply-adds are the written-out ones of the transform's complex
// products, fft512.h), every reduction in ONE order:
//   resampler      output m = 5 u + p: acc = 0; for j = 0 .. 122: acc += G[p][j] * x[8 u - 58 + j] (terms outside the signal or the
//                  filter are exact zeros).
//   sum of 256     (frame energy) lane l: ((a[l] + a[l+64]) + a[l+128]) + a[l+192]; then s += s(lane ^ 32), ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.
//   band           ascending bin.   Segment sums (two norms, two means, two norms, the product sum): ascending frame.
//   final sum      c[q], q = 15 j + band: thread i adds c[i], c[i + 256], ... in ascending q; then t[i] += t[i + 128], + 64, ... + 1.
// A row's result depends on its own samples, T and fs only -- not on B, not on its place in the call.
#include <cmath>
#include <cstring>

#include "fft512.h"
#include "sg_internal.h"
#include "wave_reduce.h"

#pragma clang fp contract(off)

using namespace sg;

namespace {

constexpr int kStFs = 10000, kStFrame = 256, kStHop = 128, kStBands = 15, kStSeg = 30;
constexpr double kStEps = 2.220446049250313e-16;  // 2^-52
constexpr double kStDyn = 40.0, kStShort = 1e-5;
constexpr int kStUp = 5, kStDown = 8, kStHalf = 290;  // 16 kHz -> 10 kHz: filter taps -290 .. 290
constexpr int kStJ0 = -58, kStW = 123;                // branch p reads source samples 8 u + kStJ0 + j, j < kStW
constexpr int kStTileFrames = 8;                      // frames a resampling block owns
constexpr int kStTileOut = kStTileFrames * kStHop + kStHop;                       // 1152 samples at 10 kHz
constexpr int kStTileSrc = ((kStTileOut + 3) / kStUp + 1) * kStDown + kStW + 5;   // >= source samples under them
constexpr int kStThreads = 256;
constexpr int kStSlices = 8;  // blocks that share a row's maximum
constexpr int kStMaxT = 1 << 24, kStMaxB = 65535;
constexpr size_t kStCacheMax = 2;

struct StoiTab {                 // the device tables, float64 built on the host (sg_stoi_debug_tables hands the blob out: tests/test_stoi_host.py
                                 // compares it with the restatement's tables, tests/native/stoi_asan_driver.cpp mirrors this layout)
    double g[kStUp * kStW + 1];  // the 5 polyphase branches of 5 h: g[p][j] = 5 h[290 + 8 p - 5 (kStJ0 + j)], 0 outside the filter
    double win[kStFrame];        // hanning(258)[1:-1]
    double2 tw1[kFftTw1];        // fft512.h: W512^(j lane)
    double2 tw2[kFftTw2];        // W64^(b c)
    double clip;                 // 1 + 10^(15/20)
    double pad;
    int32_t lo[16], hi[16];      // band b: bins lo[b] .. hi[b] - 1
};
static_assert(sizeof(StoiTab) % 16 == 0, "one blob");

struct StoiGeo {
    int T, n10, n10s;   // samples per row at fs / at 10 kHz / the workspace's row stride
    int nF, nW;         // frames of the 10 kHz signal, samples under them
    int Mmax;           // row stride of the band values (>= nF - 1)
    int resample;
};

// pmax[row][sig][slice] = the maximum of one eighth of the row (-inf for an empty slice)
__global__ __launch_bounds__(kStThreads) void stoi_scale_kernel(const float* __restrict__ benign, const float* __restrict__ adver, int T,
                                                                float* __restrict__ pmax) {
    __shared__ float red[kStThreads];
    const int sl = blockIdx.x, sig = blockIdx.y, row = blockIdx.z;
    const float* x = (sig ? adver : benign) + (size_t)row * (size_t)T;
    const int i0 = (int)((int64_t)sl * T / kStSlices), i1 = (int)((int64_t)(sl + 1) * T / kStSlices);
    float m = -INFINITY;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += kStThreads) m = fmaxf(m, x[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int st = kStThreads / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0) pmax[(2 * row + sig) * kStSlices + sl] = red[0];
}
// the input rule: 1 when -1 <= max(row) <= 1, else 2^-15
__device__ __forceinline__ double st_scale(const float* __restrict__ pmax, int row, int sig) {
    const float* p = pmax + (2 * row + sig) * kStSlices;
    float m = p[0];
    for (int i = 1; i < kStSlices; ++i) m = fmaxf(m, p[i]);
    return (-1.f <= m && m <= 1.f) ? 1.0 : 1.0 / 32768.0;
}

// the 10 kHz samples of one signal (y10 [B][2][n10s], samples below nW only) and, benign signal, the frame energies en [B][nF]
__global__ __launch_bounds__(kStThreads) void stoi_resample_kernel(const StoiTab* __restrict__ tab, const StoiGeo g,
                                                                   const float* __restrict__ benign, const float* __restrict__ adver,
                                                                   const float* __restrict__ pmax, double* __restrict__ y10,
                                                                   double* __restrict__ en) {
    __shared__ double xs[kStTileSrc];
    __shared__ double ys[kStTileOut];
    __shared__ double gs[kStUp * kStW + 1];
    __shared__ double ws[kStFrame];
    const int tile = blockIdx.x, sig = blockIdx.y, row = blockIdx.z;
    const float* x = (sig ? adver : benign) + (size_t)row * (size_t)g.T;
    const double sc = st_scale(pmax, row, sig);
    const int m0 = tile * kStTileFrames * kStHop;
    for (int i = threadIdx.x; i < kStFrame; i += kStThreads) ws[i] = tab->win[i];
    if (g.resample) {
        for (int i = threadIdx.x; i < kStUp * kStW; i += kStThreads) gs[i] = tab->g[i];
        const int u0 = m0 / kStUp;
        const int i0 = kStDown * u0 + kStJ0;
        for (int k = threadIdx.x; k < kStTileSrc; k += kStThreads) {
            const int i = i0 + k;
            xs[k] = (i >= 0 && i < g.T) ? (double)x[i] * sc : 0.0;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < kStTileOut; k += kStThreads) {
            const int m = m0 + k;
            double acc = 0.0;
            if (m < g.nW) {
                const int u = m / kStUp, p = m - u * kStUp;
                const double* gp = gs + p * kStW;
                const double* xp = xs + kStDown * (u - u0);  // (<= 8 * 231 + 122 < kStTileSrc)
                for (int j = 0; j < kStW; ++j) acc = acc + gp[j] * xp[j];
            }
            ys[k] = acc;
        }
    } else {
        for (int k = threadIdx.x; k < kStTileOut; k += kStThreads) {
            const int m = m0 + k;
            ys[k] = m < g.nW ? (double)x[m] * sc : 0.0;
        }
    }
    __syncthreads();
    // samples: this tile's first 1024 (the rest belongs to the next tile, which computes the same values), the last tile's all
    double* yrow = y10 + ((size_t)row * 2 + sig) * (size_t)g.n10s;
    const bool last = tile == (int)gridDim.x - 1;
    for (int k = threadIdx.x; k < kStTileOut; k += kStThreads) {
        const int m = m0 + k;
        if ((k < kStTileFrames * kStHop || last) && m < g.nW) yrow[m] = ys[k];
    }
    if (sig != 0) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = wave; q < kStTileFrames; q += kStThreads / 64) {
        const int f = tile * kStTileFrames + q;
        if (f >= g.nF) break;
        const double* fr = ys + q * kStHop;
        double a[4];
        for (int j = 0; j < 4; ++j) {
            const double v = fr[lane + 64 * j] * ws[lane + 64 * j];
            a[j] = v * v;
        }
        const double s = wave_sum_xor_steps(((a[0] + a[1]) + a[2]) + a[3]);
        if (lane == 0) en[(size_t)row * g.nF + f] = 20.0 * log10(sqrt(s) + kStEps);
    }
}

// src [B][nF]: the indices of the kept frames, ascending; kept [B]: their number K (also to frames_out when given)
__global__ __launch_bounds__(kStThreads) void stoi_mask_kernel(const double* __restrict__ en, int nF, int32_t* __restrict__ src,
                                                               int32_t* __restrict__ kept, int32_t* __restrict__ frames_out) {
    __shared__ double red[kStThreads];
    __shared__ int cnt[kStThreads];
    const int row = blockIdx.x, tid = threadIdx.x;
    const double* e = en + (size_t)row * nF;
    double m = -INFINITY;
    for (int f = tid; f < nF; f += kStThreads) m = fmax(m, e[f]);
    red[tid] = m;
    __syncthreads();
    for (int st = kStThreads / 2; st > 0; st >>= 1) {
        if (tid < st) red[tid] = fmax(red[tid], red[tid + st]);
        __syncthreads();
    }
    const double mx = red[0];
    const int per = (nF + kStThreads - 1) / kStThreads;
    const int f0 = min(nF, tid * per), f1 = min(nF, f0 + per);
    int c = 0;
    for (int f = f0; f < f1; ++f) c += (mx - kStDyn - e[f]) < 0.0 ? 1 : 0;
    cnt[tid] = c;
    __syncthreads();
    int at = 0;
    for (int t = 0; t < tid; ++t) at += cnt[t];
    int32_t* out = src + (size_t)row * nF;
    for (int f = f0; f < f1; ++f)
        if ((mx - kStDyn - e[f]) < 0.0) out[at++] = f;  // (at <= nF: at most one entry per frame)
    if (tid == kStThreads - 1) {
        kept[row] = at;
        if (frames_out) frames_out[row] = at;
    }
}

// bands [B][2][15][Mmax]: one wave per output frame
__global__ __launch_bounds__(kStThreads) void stoi_bands_kernel(const StoiTab* __restrict__ tab, const StoiGeo g,
                                                                const double* __restrict__ y10, const int32_t* __restrict__ src,
                                                                const int32_t* __restrict__ kept, double* __restrict__ bands) {
    __shared__ double2 tw1[kFftTw1];
    __shared__ double2 tw2[kFftTw2];
    __shared__ double ws[kStFrame];
    __shared__ double2 work[kStThreads / 64][576];
    for (int i = threadIdx.x; i < kFftTw1; i += kStThreads) tw1[i] = tab->tw1[i];
    for (int i = threadIdx.x; i < kFftTw2; i += kStThreads) tw2[i] = tab->tw2[i];
    for (int i = threadIdx.x; i < kStFrame; i += kStThreads) ws[i] = tab->win[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.y;
    const int m = blockIdx.x * (kStThreads / 64) + wave;
    const int K = kept[row];
    if (m >= K - 1 || m >= g.Mmax) return;  // (wave-uniform; no block barrier follows)
    const int32_t* sr = src + (size_t)row * g.nF;
    // kept frames m - 1, m, m + 1 <= K - 1 start at 128 src[.] <= 128 (nF - 1): every read below stays under nW
    const int s0 = sr[m] * kStHop, sn = sr[m + 1] * kStHop, sp = m > 0 ? sr[m - 1] * kStHop : -1;
    double2* buf = work[wave];
    double* pw = reinterpret_cast<double*>(buf);
    const int lo = lane < kStBands ? tab->lo[lane] : 0, hi = lane < kStBands ? tab->hi[lane] : 0;
    for (int sig = 0; sig < 2; ++sig) {
        const double* y = y10 + ((size_t)row * 2 + sig) * (size_t)g.n10s;
        double v[4];
        for (int j = 0; j < 4; ++j) {
            const int t = lane + 64 * j;
            double z = ws[t] * y[s0 + t];
            if (j < 2) {
                if (sp >= 0) z = z + ws[t + kStHop] * y[sp + t + kStHop];
            } else {
                z = z + ws[t - kStHop] * y[sn + t - kStHop];
            }
            v[j] = ws[t] * z;
        }
        const double2 zero = make_double2(0.0, 0.0);
        const double2 in[8] = {make_double2(v[0], 0.0), make_double2(v[1], 0.0), make_double2(v[2], 0.0), make_double2(v[3], 0.0), zero, zero,
                               zero, zero};
        double2 X[8];
        fft512T_regs<double>(buf, tw1, tw2, lane, -1.0, in, X);
        const int k0 = (lane >> 3) + 8 * (lane & 7);  // X[d] is bin k0 + 64 d
        for (int d = 0; d < 4; ++d) pw[k0 + 64 * d] = X[d].x * X[d].x + X[d].y * X[d].y;
        wave_sync();
        if (lane < kStBands) {
            double acc = 0.0;
            for (int k = lo; k < hi; ++k) acc = acc + pw[k];
            bands[(((size_t)row * 2 + sig) * kStBands + lane) * (size_t)g.Mmax + m] = sqrt(acc);
        }
        wave_sync();
    }
}

// d [B]
__global__ __launch_bounds__(kStThreads) void stoi_segments_kernel(const StoiTab* __restrict__ tab, const StoiGeo g,
                                                                   const double* __restrict__ bands, const int32_t* __restrict__ kept,
                                                                   double* __restrict__ d_out) {
    __shared__ double red[kStThreads];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int M = min(kept[row] - 1, g.Mmax);
    if (M < kStSeg) {  // (block-uniform)
        if (tid == 0) d_out[row] = kStShort;
        return;
    }
    const int J = M - kStSeg + 1, P = J * kStBands;
    const double clip = tab->clip;
    double total = 0.0;
    for (int q = tid; q < P; q += kStThreads) {
        const int j = q / kStBands, b = q - j * kStBands;
        const double* xb = bands + (((size_t)row * 2 + 0) * kStBands + b) * (size_t)g.Mmax + j;
        const double* yb = bands + (((size_t)row * 2 + 1) * kStBands + b) * (size_t)g.Mmax + j;
        double x[kStSeg], y[kStSeg];
        double sx = 0.0, sy = 0.0;
        for (int n = 0; n < kStSeg; ++n) {
            x[n] = xb[n], y[n] = yb[n];
            sx = sx + x[n] * x[n];
            sy = sy + y[n] * y[n];
        }
        const double a = sqrt(sx) / (sqrt(sy) + kStEps);
        double mx = 0.0, my = 0.0;
        for (int n = 0; n < kStSeg; ++n) {
            y[n] = fmin(y[n] * a, x[n] * clip);
            mx = mx + x[n];
            my = my + y[n];
        }
        mx = mx / kStSeg, my = my / kStSeg;
        sx = 0.0, sy = 0.0;
        for (int n = 0; n < kStSeg; ++n) {
            x[n] = x[n] - mx, y[n] = y[n] - my;
            sx = sx + x[n] * x[n];
            sy = sy + y[n] * y[n];
        }
        const double nx = sqrt(sx) + kStEps, ny = sqrt(sy) + kStEps;
        double c = 0.0;
        for (int n = 0; n < kStSeg; ++n) c = c + (y[n] / ny) * (x[n] / nx);
        total = total + c;
    }
    red[tid] = total;
    __syncthreads();
    for (int st = kStThreads / 2; st > 0; st >>= 1) {
        if (tid < st) red[tid] = red[tid] + red[tid + st];
        __syncthreads();
    }
    if (tid == 0) d_out[row] = red[0] / (double)P;
}

// ---------------------------------------------------------------- host: the tables, the cache
double st_i0(double x) {  // modified Bessel function of order 0: the power series, to the last bit that moves
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

void st_build(StoiTab* t) {
    const double pi = 3.14159265358979323846;
    std::memset(t, 0, sizeof(*t));
    // Octave's resample filter for 5/8: fc = 1/16, roll-off fc/10, 60 dB -> L = ceil((60 - 8) / (28.714 * fc / 10)) = 290
    const double fc = 1.0 / (2.0 * kStDown), beta = 0.1102 * (60.0 - 8.7);
    double h[2 * kStHalf + 1], sum = 0.0;
    for (int n = 0; n <= 2 * kStHalf; ++n) {
        const double r = (double)(n - kStHalf) / kStHalf, x = pi * 2.0 * fc * (n - kStHalf);
        const double kaiser = st_i0(beta * std::sqrt(1.0 - r * r)) / st_i0(beta);
        h[n] = kaiser * (2.0 * kStUp * fc * (n == kStHalf ? 1.0 : std::sin(x) / x));
        sum += h[n];
    }
    for (int p = 0; p < kStUp; ++p)
        for (int j = 0; j < kStW; ++j) {
            const int d = kStDown * p - kStUp * (kStJ0 + j);
            if (d >= -kStHalf && d <= kStHalf) t->g[p * kStW + j] = kStUp * (h[kStHalf + d] / sum);
        }
    for (int i = 0; i < kStFrame; ++i) t->win[i] = 0.5 + 0.5 * std::cos(pi * (double)(2 * (i + 1) - (kStFrame + 1)) / (kStFrame + 1));
    auto w512 = [&](int m) { return make_double2(std::cos(2.0 * pi * (m % 512) / 512.0), -std::sin(2.0 * pi * (m % 512) / 512.0)); };
    fft512_twiddle_tables(w512, reinterpret_cast<double*>(t->tw1), reinterpret_cast<double*>(t->tw2));
    t->clip = 1.0 + std::pow(10.0, 15.0 / 20.0);
    // band b: bins [argmin |f - 150 2^((2 b - 1) / 6)|, argmin |f - 150 2^((2 b + 1) / 6)|), f_k = k 10000 / 512, first minimum
    auto nearest = [&](double f) {
        int best = 0;
        for (int k = 1; k <= 256; ++k)
            if (std::fabs(k * (kStFs / 512.0) - f) < std::fabs(best * (kStFs / 512.0) - f)) best = k;
        return best;
    };
    for (int b = 0; b < kStBands; ++b) {
        t->lo[b] = nearest(150.0 * std::pow(2.0, (2 * b - 1) / 6.0));
        t->hi[b] = nearest(150.0 * std::pow(2.0, (2 * b + 1) / 6.0));
    }
}

int st_tables(sg_ctx* ctx, int fs, hipStream_t s, const StoiTab** out) {
    const std::vector<int32_t> key{fs};
    if (DevTable* hit = ctx->stoi_cache.find(key)) return *out = static_cast<const StoiTab*>(hit->dev), SG_OK;
    DevTable* e = new DevTable();
    e->key = key;
    e->blob.resize(sizeof(StoiTab));
    StoiTab* t = new StoiTab();
    st_build(t);
    std::memcpy(e->blob.data(), t, sizeof(StoiTab));
    delete t;
    if (int rc = dev_tables_insert(ctx, "sg_wav_stoi", "", &ctx->stoi_cache, kStCacheMax, e, s)) return rc;
    return *out = static_cast<const StoiTab*>(e->dev), SG_OK;
}

}  // namespace

extern "C" int32_t sg_stoi_debug_tables(void* out, int32_t capacity) {
    if (out && capacity >= (int32_t)sizeof(StoiTab)) {
        StoiTab* t = new StoiTab();
        st_build(t);
        std::memcpy(out, t, sizeof(StoiTab));
        delete t;
    }
    return (int32_t)sizeof(StoiTab);
}

extern "C" int sg_wav_stoi(sg_ctx* ctx, const float* benign_dev, const float* adver_dev, int32_t B, int32_t T, int32_t fs, double* stoi_dev,
                           int32_t* frames_dev, void* stream) {
    const char* who = "sg_wav_stoi";
    hipStream_t s = (hipStream_t)stream;
    if (!ctx) return SG_ERR_ARG;
    if (!benign_dev || !adver_dev || !stoi_dev) return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    if (B < 1 || B > kStMaxB) return fail(ctx, SG_ERR_ARG, "%s: need 1 <= B <= %d (B %d)", who, kStMaxB, B);
    if (fs != kStFs && fs != 16000) return fail(ctx, SG_ERR_ARG, "%s: fs must be 10000 or 16000 (%d)", who, fs);
    if (T < 1 || T > kStMaxT) return fail(ctx, SG_ERR_ARG, "%s: need 1 <= T <= %d (T %d)", who, kStMaxT, T);
    StoiGeo g{};
    g.T = T, g.resample = fs != kStFs;
    g.n10 = g.resample ? (int)(((int64_t)kStUp * T + kStDown - 1) / kStDown) : T;
    if (g.n10 <= kStFrame)
        return fail(ctx, SG_ERR_ARG, "%s: %d samples at %d Hz are %d at 10 kHz, more than %d are needed", who, T, fs, g.n10, kStFrame);
    g.nF = (g.n10 - kStFrame + kStHop - 1) / kStHop;  // len(range(0, n10 - 256, 128)) >= 1
    g.nW = (g.nF - 1) * kStHop + kStFrame;            // <= n10
    g.n10s = (g.nW + 1) & ~1;
    g.Mmax = std::max(g.nF - 1, 1);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);

    // the workspaces, before the first launch: [B][2][n10s] samples, [B][nF] energies, [B][2][15][Mmax] bands, [B][2][8] slice maxima (float32);
    // [B] kept counts, [B][nF] kept indices
    const size_t n_y = (size_t)B * 2 * g.n10s, n_e = ((size_t)B * g.nF + 1) & ~(size_t)1, n_b = (size_t)B * 2 * kStBands * g.Mmax;
    if (int rc = dev_grow(ctx, ctx->model_allocs, &ctx->stoi_ws, n_y + n_e + n_b + kStSlices * (size_t)B, s)) return rc;
    if (int rc = dev_grow(ctx, ctx->model_allocs, &ctx->stoi_iws, (size_t)B * (1 + (size_t)g.nF), s)) return rc;
    const StoiTab* tab = nullptr;
    if (int rc = st_tables(ctx, fs, s, &tab)) return rc;
    double* y10 = ctx->stoi_ws.ptr;
    double* en = y10 + n_y;
    double* bands = en + n_e;
    float* pmax = reinterpret_cast<float*>(bands + n_b);
    int32_t* kept = ctx->stoi_iws.ptr;
    int32_t* src = kept + B;

    const int tiles = (g.nF + kStTileFrames - 1) / kStTileFrames;
    trace_mark(ctx, SG_STAGE_STOI_SCALE, s, 0);
    hipLaunchKernelGGL(stoi_scale_kernel, dim3(kStSlices, 2, B), dim3(kStThreads), 0, s, benign_dev, adver_dev, (int)T, pmax);
    SG_HIP(hipGetLastError());
    trace_mark(ctx, SG_STAGE_STOI_SCALE, s, 1);
    trace_mark(ctx, SG_STAGE_STOI_RESAMPLE, s, 0);
    hipLaunchKernelGGL(stoi_resample_kernel, dim3(tiles, 2, B), dim3(kStThreads), 0, s, tab, g, benign_dev, adver_dev, (const float*)pmax, y10,
                       en);
    SG_HIP(hipGetLastError());
    trace_mark(ctx, SG_STAGE_STOI_RESAMPLE, s, 1);
    trace_mark(ctx, SG_STAGE_STOI_MASK, s, 0);
    hipLaunchKernelGGL(stoi_mask_kernel, dim3(B), dim3(kStThreads), 0, s, (const double*)en, g.nF, src, kept, frames_dev);
    SG_HIP(hipGetLastError());
    trace_mark(ctx, SG_STAGE_STOI_MASK, s, 1);
    if (g.nF - 1 >= kStSeg) {  // (fewer frames: every row has M < 30, the last launch needs no band value)
        trace_mark(ctx, SG_STAGE_STOI_BANDS, s, 0);
        hipLaunchKernelGGL(stoi_bands_kernel, dim3((g.nF - 1 + 3) / 4, B), dim3(kStThreads), 0, s, tab, g, (const double*)y10,
                           (const int32_t*)src, (const int32_t*)kept, bands);
        SG_HIP(hipGetLastError());
        trace_mark(ctx, SG_STAGE_STOI_BANDS, s, 1);
    }
    trace_mark(ctx, SG_STAGE_STOI_SEGMENTS, s, 0);
    hipLaunchKernelGGL(stoi_segments_kernel, dim3(B), dim3(kStThreads), 0, s, tab, g, (const double*)bands, (const int32_t*)kept, stoi_dev);
    SG_HIP(hipGetLastError());
    trace_mark(ctx, SG_STAGE_STOI_SEGMENTS, s, 1);
    return SG_OK;
}
