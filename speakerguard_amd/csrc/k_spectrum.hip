// The whole-utterance spectrum gate (reference attack/_kenan_fft.py fft_compression :57-82 and the peak of :198) on (B,T)
// float32 waveforms, one utterance per row:  X = rfft(x);  X[k] = 0 where |X[k]| < factor[b];  y = irfft(X).
// One launch per call and ONE WORKGROUP PER UTTERANCE: forward transform, magnitude, gate and inverse transform run as a loop
// of passes inside the launch with a workgroup barrier between them.  What a row computes depends on T alone -- not on B, not
// on the row's place in the call: a batch equals its shards, bit for bit.
//
// Transform.  T is even; M = T / 2.  z[n] = x[2n] + i x[2n+1] goes through a complex DFT of length M and the real post-pass
//     X[k] = E + t,  X[M-k] = conj(E - t),   E = (Z[k] + conj Z[M-k]) / 2,  t = -i w^k (Z[k] - conj Z[M-k]) / 2,  w = exp(-2 pi i / T)
// for 0 < k <= M / 2;  X[0] = Re Z[0] + Im Z[0] and X[M] = Re Z[0] - Im Z[0] are real.  The inverse is the transposed route:
//     Z'[k] = S + u,  Z'[M-k] = conj(S - u),   S = X[k] + conj X[M-k],  u = i conj(w^k) (X[k] - conj X[M-k]),
// an inverse DFT of length M as conj(DFT(conj Z')), and one product with the float32 value 1 / T.
//
// The DFT of length N is a Stockham autosort network (decimation in frequency, no bit reversal): a pass of radix R at stride s
// reads a[j] = in[i + j N/R], takes the R-point butterfly and writes out[q + R s p + s k] = b[k] * tw[s p k], where i = q + s p,
// q < s, and tw[j] = exp(-2 pi i j / N).  Radices 4, 2, 3, 5 in that order (plan: sp_make_plan).  All tables are built on the
// host in float64 and rounded ONCE to float32; there is no sine or cosine on the device.
//   smooth lengths, M = 2^a 3^b 5^c (16000, 48000, 480):  N = M.
//   every other even T:  Bluestein.  With c[n] = exp(-i pi n^2 / M) (n^2 mod 2M in integers, on the host),
//       Z[k] = c[k] sum_n (z[n] c[n]) conj c[k-n]:  a circular convolution of length L = the next power of two >= 2M - 1, run as
//       conj(DFT_L(conj(DFT_L(a) * bhat))) with bhat = DFT_L(conj c, wrapped) / L built on the host in float64.  N = L.
//
// Where the data lives: two buffers of N complex values.  In LDS when both fit the 160 KB a workgroup may take (N <= 10224), else
// in a workspace of the context (2 N values per row: 64 x 2 x 192 KB at T = 48000 stays in L2 / Infinity Cache).  A workgroup
// barrier orders a pass's global stores before the next pass's loads: the waves of one workgroup share one L1.  No workgroup
// ever reads what another wrote.
//
// Gate.  |X| = sqrtf(re * re + im * im), three float32 roundings, no fused multiply-add; bin k of row b is zeroed when
// |X[b,k]| < factor[b], STRICTLY.  It follows from the comparison that a factor that is NaN, negative or zero keeps every bin
// (nothing compares below it) and that a bin whose magnitude is NaN is kept.  DC and Nyquist carry a zero imaginary part, so
// they are gated on their real value.  peak[b] = max_k |X[b,k]| is reduced in the same launch, from the same magnitudes.
//
// Host cost of a table: the blob stays on the host beside its device copy for the life of the cache entry (the upload is
// asynchronous from pageable memory), 8 bytes per complex value: 3 T / 4 values for a smooth T, up to 4.75 T for a Bluestein T
// whose M lies just past a power of two.  At T = 48000 that is 0.29 MB, at T = 52960 1.4 MB; a non-smooth T near 2^22 costs up to
// ~90 MB of host memory per entry (and as much on the device) and a float64 FFT of 2^22 points on the host at first use.
// Sixteen entries at most per context.
//
// Arithmetic: float32 throughout, no contraction (every product and sum rounds on its own): tests/kenan_restate.py restates the
// network in numpy, and tests/test_gpu_kenan.py holds the kernel to it value for value.
#include <cmath>
#include <cstring>

#include "sg_internal.h"

#pragma clang fp contract(off)

using namespace sg;

namespace {

constexpr int kSpThreads = 1024;
constexpr int kSpMaxPass = 24;           // 3^13 < 2^21 < 3^14; radix 4 first: a power of two takes at most 11
constexpr int kSpMaxLen = 1 << 22;       // T
constexpr size_t kSpLdsBytes = 160 * 1024;
constexpr size_t kSpLdsStatic = 256;     // the reductions' words (128 bytes, static_assert in the kernel) and as much headroom
constexpr size_t kSpCacheMax = 16;

struct SpPlan {
    int T, M, N;           // N: length of the pass network (M, or Bluestein's L)
    int bluestein;
    int n_pass;
    unsigned char radix[kSpMaxPass];
    int o_tw, o_post, o_chirp, o_bhat;  // complex-value offsets in the table blob: tw[N], post[M/2+1], chirp[M], bhat[N]
    int words;                          // complex values in the blob
    float inv_T;
};

bool sp_make_plan(int T, SpPlan* p) {
    if (T < 2 || T > kSpMaxLen || (T & 1)) return false;
    std::memset(p, 0, sizeof(*p));
    p->T = T, p->M = T / 2;
    int rest = p->M;
    for (int f : {2, 3, 5})
        while (rest % f == 0) rest /= f;
    p->bluestein = rest != 1;
    p->N = p->M;
    if (p->bluestein) {
        p->N = 1;
        while (p->N < 2 * p->M - 1) p->N *= 2;
    }
    int n = p->N;
    for (int f : {4, 2, 3, 5})
        while (n % f == 0) {
            if (p->n_pass == kSpMaxPass) return false;
            p->radix[p->n_pass++] = (unsigned char)f;
            n /= f;
        }
    p->o_tw = 0;
    p->o_post = p->o_tw + p->N;
    p->o_chirp = p->o_post + p->M / 2 + 1;
    p->o_bhat = p->o_chirp + (p->bluestein ? p->M : 0);
    p->words = p->o_bhat + (p->bluestein ? p->N : 0);
    p->inv_T = (float)(1.0 / (double)T);
    return n == 1;
}

bool sp_in_lds(const SpPlan& p) { return (size_t)p.N * 2 * sizeof(float2) + kSpLdsStatic <= kSpLdsBytes; }

// ---------------------------------------------------------------- the tables, float64 rounded once
void sp_fft64(std::vector<double>& re, std::vector<double>& im) {  // in place, power of two, forward
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(re[i], re[j]), std::swap(im[i], im[j]);
    }
    const double pi = 3.14159265358979323846;
    for (size_t len = 2; len <= n; len <<= 1) {
        const size_t h = len / 2;
        std::vector<double> wr(h), wi(h);
        for (size_t k = 0; k < h; ++k) wr[k] = std::cos(2 * pi * (double)k / (double)len), wi[k] = -std::sin(2 * pi * (double)k / (double)len);
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < h; ++k) {
                const double ur = re[i + k], ui = im[i + k];
                const double vr = re[i + k + h] * wr[k] - im[i + k + h] * wi[k], vi = re[i + k + h] * wi[k] + im[i + k + h] * wr[k];
                re[i + k] = ur + vr, im[i + k] = ui + vi;
                re[i + k + h] = ur - vr, im[i + k + h] = ui - vi;
            }
    }
}

void sp_build_tables(const SpPlan& p, float2* t) {  // t: p.words values, zeroed
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < p.N; ++j) {
        const double a = 2 * pi * (double)j / (double)p.N;
        t[p.o_tw + j] = make_float2((float)std::cos(a), (float)-std::sin(a));
    }
    for (int k = 0; k <= p.M / 2; ++k) {
        const double a = 2 * pi * (double)k / (double)p.T;
        t[p.o_post + k] = make_float2((float)std::cos(a), (float)-std::sin(a));
    }
    if (!p.bluestein) return;
    std::vector<double> br((size_t)p.N, 0.0), bi((size_t)p.N, 0.0);
    for (int n = 0; n < p.M; ++n) {
        const long long sq = ((long long)n * n) % (2LL * p.M);
        const double a = pi * (double)sq / (double)p.M;
        const double cr = std::cos(a), ci = -std::sin(a);  // c[n] = exp(-i pi n^2 / M)
        t[p.o_chirp + n] = make_float2((float)cr, (float)ci);
        br[n] = cr, bi[n] = -ci;  // conj c, at n and wrapped at L - n
        if (n) br[p.N - n] = cr, bi[p.N - n] = -ci;
    }
    sp_fft64(br, bi);
    for (int j = 0; j < p.N; ++j) t[p.o_bhat + j] = make_float2((float)(br[j] / (double)p.N), (float)(bi[j] / (double)p.N));
}

// ---------------------------------------------------------------- the passes (one workgroup; `tid` of `nt` threads)
#define SP_DEV __device__ __forceinline__

SP_DEV float2 c_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
SP_DEV float2 c_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
SP_DEV float2 c_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
SP_DEV float2 c_conj(float2 a) { return make_float2(a.x, -a.y); }
SP_DEV float2 c_scale(float s, float2 a) { return make_float2(s * a.x, s * a.y); }
SP_DEV float2 c_mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // -i a
SP_DEV float2 c_mul_pi(float2 a) { return make_float2(-a.y, a.x); }  // +i a
SP_DEV float sp_mag(float2 a) { return sqrtf(a.x * a.x + a.y * a.y); }

template <int R>
SP_DEV void sp_butterfly(float2 (&a)[R]);
template <>
SP_DEV void sp_butterfly<2>(float2 (&a)[2]) {
    const float2 b0 = c_add(a[0], a[1]), b1 = c_sub(a[0], a[1]);
    a[0] = b0, a[1] = b1;
}
template <>
SP_DEV void sp_butterfly<4>(float2 (&a)[4]) {
    const float2 t0 = c_add(a[0], a[2]), t1 = c_sub(a[0], a[2]), t2 = c_add(a[1], a[3]), t3 = c_mul_mi(c_sub(a[1], a[3]));
    a[0] = c_add(t0, t2), a[1] = c_add(t1, t3), a[2] = c_sub(t0, t2), a[3] = c_sub(t1, t3);
}
template <>
SP_DEV void sp_butterfly<3>(float2 (&a)[3]) {
    const float s3 = 0.86602540378443864676f;  // sin(2 pi / 3)
    const float2 t1 = c_add(a[1], a[2]), t2 = c_sub(a[0], c_scale(0.5f, t1)), t3 = c_scale(s3, c_sub(a[1], a[2]));
    a[0] = c_add(a[0], t1);
    a[1] = c_add(t2, c_mul_mi(t3));
    a[2] = c_add(t2, c_mul_pi(t3));
}
template <>
SP_DEV void sp_butterfly<5>(float2 (&a)[5]) {
    const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;  // cos(2 pi / 5), cos(4 pi / 5)
    const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;   // sin(2 pi / 5), sin(4 pi / 5)
    const float2 t1 = c_add(a[1], a[4]), t2 = c_add(a[2], a[3]), t3 = c_sub(a[1], a[4]), t4 = c_sub(a[2], a[3]);
    const float2 m1 = c_add(c_add(a[0], c_scale(c1, t1)), c_scale(c2, t2));
    const float2 m2 = c_add(c_add(a[0], c_scale(c2, t1)), c_scale(c1, t2));
    const float2 n1 = c_add(c_scale(s1, t3), c_scale(s2, t4));
    const float2 n2 = c_sub(c_scale(s2, t3), c_scale(s1, t4));
    a[0] = c_add(c_add(a[0], t1), t2);
    a[1] = c_add(m1, c_mul_mi(n1));
    a[4] = c_add(m1, c_mul_pi(n1));
    a[2] = c_add(m2, c_mul_mi(n2));
    a[3] = c_add(m2, c_mul_pi(n2));
}

template <int R>
SP_DEV void sp_pass(const float2* in, float2* out, const float2* tw, int N, int s, int tid, int nt) {
    const int nb = N / R;
    for (int i = tid; i < nb; i += nt) {
        const int q = (int)((unsigned)i % (unsigned)s), sp = i - q;  // i = q + s p
        float2 a[R];
#pragma unroll
        for (int j = 0; j < R; ++j) a[j] = in[i + j * nb];
        sp_butterfly<R>(a);
        const int o = q + sp * R;
        out[o] = a[0];
#pragma unroll
        for (int k = 1; k < R; ++k) out[o + s * k] = c_mul(a[k], tw[sp * k]);
    }
}

// DFT of length N over buf[cur .. cur + N) (cur is 0 or N); returns where the result lies.  Ends on a barrier.
SP_DEV int sp_network(float2* buf, int cur, const SpPlan& p, const float2* tw, int tid, int nt) {
    int s = 1;
    for (int i = 0; i < p.n_pass; ++i) {
        const int R = p.radix[i];
        const float2* in = buf + cur;
        float2* out = buf + (p.N - cur);
        if (R == 4) sp_pass<4>(in, out, tw, p.N, s, tid, nt);
        else if (R == 2) sp_pass<2>(in, out, tw, p.N, s, tid, nt);
        else if (R == 3) sp_pass<3>(in, out, tw, p.N, s, tid, nt);
        else sp_pass<5>(in, out, tw, p.N, s, tid, nt);
        __syncthreads();
        cur = p.N - cur;
        s *= R;
    }
    return cur;
}

// DFT of length M of the M values at buf[cur ..): the network itself, or Bluestein's three steps around two networks
SP_DEV int sp_dft(float2* buf, int cur, const SpPlan& p, const float2* tab, int tid, int nt) {
    const float2* tw = tab + p.o_tw;
    if (!p.bluestein) return sp_network(buf, cur, p, tw, tid, nt);
    const float2* chirp = tab + p.o_chirp;
    const float2* bhat = tab + p.o_bhat;
    for (int n = tid; n < p.N; n += nt) buf[cur + n] = n < p.M ? c_mul(buf[cur + n], chirp[n]) : make_float2(0.f, 0.f);
    __syncthreads();
    cur = sp_network(buf, cur, p, tw, tid, nt);
    for (int n = tid; n < p.N; n += nt) buf[cur + n] = c_conj(c_mul(buf[cur + n], bhat[n]));
    __syncthreads();
    cur = sp_network(buf, cur, p, tw, tid, nt);
    for (int k = tid; k < p.M; k += nt) buf[cur + k] = c_mul(chirp[k], c_conj(buf[cur + k]));
    __syncthreads();
    return cur;
}

// One workgroup per row.  out == nullptr: the spectrum only (sg_wav_spectrum); else the gate (sg_wav_spectrum_gate).
template <bool LDS>
__global__ void __launch_bounds__(kSpThreads)
sp_kernel(SpPlan p, const float2* tab, const float* x, float2* ws, float* spec, float* peak, const float* factor, float* out,
          uint8_t* keep, int32_t* kept) {
    extern __shared__ float2 sp_lds[];
    __shared__ float red_f[kSpThreads / 64];
    __shared__ int red_i[kSpThreads / 64];
    static_assert(sizeof(red_f) + sizeof(red_i) <= kSpLdsStatic, "the static LDS must fit what sp_in_lds sets aside for it");
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t row = blockIdx.x;
    float2* buf = LDS ? sp_lds : ws + row * 2 * (size_t)p.N;
    const float* xr = x + row * (size_t)p.T;
    const int M = p.M;

    for (int n = tid; n < M; n += nt) buf[n] = make_float2(xr[2 * n], xr[2 * n + 1]);
    __syncthreads();
    int cur = sp_dft(buf, 0, p, tab, tid, nt);

    // the real post-pass, the magnitudes, the gate and the inverse's pre-pass: thread k owns bins k and M - k
    float2* Z = buf + cur;
    const float2* post = tab + p.o_post;
    const bool gate = out != nullptr;
    const float f = gate ? factor[row] : 0.f;
    // (the caller's spectrum is a float buffer, aligned as floats: a pair goes out as two floats, not as one 8-byte word)
    float* srow = spec ? spec + row * 2 * (size_t)(M + 1) : nullptr;
    uint8_t* krow = keep ? keep + row * (size_t)(M + 1) : nullptr;
    float pk = 0.f;
    int cnt = 0;
    for (int k = tid; k <= M / 2; k += nt) {
        const int m = M - k;
        float2 Xk, Xm;
        if (k == 0) {
            const float2 z0 = Z[0];
            Xk = make_float2(z0.x + z0.y, 0.f), Xm = make_float2(z0.x - z0.y, 0.f);
        } else {
            const float2 A = Z[k], Bc = c_conj(Z[m]);
            const float2 E = c_scale(0.5f, c_add(A, Bc)), D = c_scale(0.5f, c_sub(A, Bc));
            const float2 t = c_mul_mi(c_mul(post[k], D));
            Xk = c_add(E, t), Xm = c_conj(c_sub(E, t));
        }
        const bool two = k != m;  // (k == m: the middle bin of an even M, alone)
        if (!two) Xm = Xk;
        const float mk = sp_mag(Xk), mm = sp_mag(Xm);
        pk = fmaxf(pk, fmaxf(mk, mm));
        if (srow) {
            srow[2 * k] = Xk.x, srow[2 * k + 1] = Xk.y;
            if (two) srow[2 * m] = Xm.x, srow[2 * m + 1] = Xm.y;
        }
        if (gate) {
            const bool kk = !(mk < f), km = !(mm < f);
            cnt += (int)kk + (two ? (int)km : 0);
            if (krow) {
                krow[k] = (uint8_t)kk;
                if (two) krow[m] = (uint8_t)km;
            }
            const float2 zero = make_float2(0.f, 0.f);
            const float2 Gk = kk ? Xk : zero, Gm = km ? Xm : zero;
            if (k == 0) {
                Z[0] = make_float2(Gk.x + Gm.x, -(Gk.x - Gm.x));  // conj Z'[0]
            } else {
                const float2 S = c_add(Gk, c_conj(Gm)), Dd = c_sub(Gk, c_conj(Gm));
                const float2 u = c_mul_pi(c_mul(c_conj(post[k]), Dd));
                Z[k] = c_conj(c_add(S, u));  // conj Z'[k]
                if (two) Z[m] = c_sub(S, u);  // conj Z'[M-k]
            }
        }
    }
    // the row's peak and count
    for (int d = 32; d >= 1; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d)), cnt += __shfl_xor(cnt, d);  // both butterflies in one loop, order 32 .. 1
    if ((tid & 63) == 0) red_f[tid >> 6] = pk, red_i[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < (nt + 63) / 64; ++w) pk = fmaxf(pk, red_f[w]), cnt += red_i[w];
        if (peak) peak[row] = pk;
        if (gate && kept) kept[row] = cnt;
    }
    if (!gate) return;

    cur = sp_dft(buf, cur, p, tab, tid, nt);
    const float2* Y = buf + cur;
    float* orow = out + row * (size_t)p.T;
    for (int n = tid; n < M; n += nt) {
        const float2 y = Y[n];
        orow[2 * n] = y.x * p.inv_T, orow[2 * n + 1] = -y.y * p.inv_T;
    }
}

// ---------------------------------------------------------------- per-T tables, kept in the context
struct SpEntry : DevTable {  // key: T
    SpPlan plan{};
};

// T's tables on the device: found, or built and uploaded on `s` (first use of T only)
int sp_tables(sg_ctx* ctx, const char* who, const SpPlan& plan, hipStream_t s, SpEntry** out) {
    const std::vector<int32_t> key{plan.T};
    if (DevTable* hit = ctx->sp_cache.find(key)) return *out = static_cast<SpEntry*>(hit), SG_OK;
    SpEntry* e = new SpEntry();
    e->key = key;
    e->plan = plan;
    e->blob.resize((size_t)plan.words * sizeof(float2));
    sp_build_tables(plan, reinterpret_cast<float2*>(e->blob.data()));
    char of[32];
    snprintf(of, sizeof(of), " of T = %d", plan.T);
    if (int rc = dev_tables_insert(ctx, who, of, &ctx->sp_cache, kSpCacheMax, e, s)) return rc;
    return *out = e, SG_OK;
}

int sp_run(sg_ctx* ctx, const char* who, const float* x_dev, int32_t B, int32_t T, float* spec, float* peak, const float* factor,
           float* out, uint8_t* keep, int32_t* kept, hipStream_t s) {
    SpPlan plan;
    if (B < 1 || !sp_make_plan(T, &plan))
        return fail(ctx, SG_ERR_ARG, "%s: need B >= 1 and an even T in 2 .. %d (B %d, T %d)", who, kSpMaxLen, B, T);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    SpEntry* e = nullptr;
    if (int rc = sp_tables(ctx, who, plan, s, &e)) return rc;
    const bool lds = sp_in_lds(plan);
    size_t dyn = 0;
    if (lds) {
        dyn = (size_t)plan.N * 2 * sizeof(float2);
        if (!ctx->sp_lds_opted) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sp_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kSpLdsBytes - kSpLdsStatic)) != hipSuccess)
                return fail(ctx, SG_ERR_HIP, "%s: a workgroup cannot take %zu bytes of LDS on this device", who, kSpLdsBytes);
            ctx->sp_lds_opted = true;
        }
    } else {
        if (int rc = dev_grow(ctx, ctx->model_allocs, &ctx->sp_ws, (size_t)B * 2 * (size_t)plan.N, s)) return rc;
    }
    auto kernel = lds ? sp_kernel<true> : sp_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(kSpThreads), dyn, s, e->plan, (const float2*)e->dev, x_dev, ctx->sp_ws.ptr,
                       spec, peak, factor, out, keep, kept);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return SG_OK;
}

}  // namespace

extern "C" int sg_wav_spectrum(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, float* spec_dev, float* peak_dev, void* stream) {
    const char* who = "sg_wav_spectrum";
    if (!ctx) return SG_ERR_ARG;
    if (!x_dev || (!spec_dev && !peak_dev)) return fail(ctx, SG_ERR_ARG, "%s: null argument (x, or both outputs)", who);
    return sp_run(ctx, who, x_dev, B, T, spec_dev, peak_dev, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int sg_wav_spectrum_gate(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, const float* factor_dev, float* out_dev,
                                    uint8_t* keep_dev, int32_t* kept_dev, void* stream) {
    const char* who = "sg_wav_spectrum_gate";
    if (!ctx) return SG_ERR_ARG;
    if (!x_dev || !factor_dev || !out_dev) return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    if (out_dev == x_dev) return fail(ctx, SG_ERR_ARG, "%s: out_dev may not alias x_dev", who);
    return sp_run(ctx, who, x_dev, B, T, nullptr, nullptr, factor_dev, out_dev, keep_dev, kept_dev, (hipStream_t)stream);
}
