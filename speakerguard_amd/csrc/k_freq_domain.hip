// Frequency-domain input defenses (reference defense/frequency_domain.py LPF :33-70, BPF :72-112), both directions, on (B,T)
// float32 waveforms, one utterance per row: a Butterworth filter followed by a clamp.  The reference runs the filter as
// ONE direct form of order 2N on the host, one utterance after the other; here the SAME design runs as a cascade of S
// second-order sections (1 <= S <= 16) with zero initial state, as a parallel scan, one launch per direction, one block per
// row, all sections back to back on registers.  (Why sections: DESIGN.md "The frequency-domain defenses" -- the reference's
// float32 direct form of its default BPF has poles outside the unit circle.)
//
//   forward   v = H x;  out = min(max(v, lo), hi);  mask = (v >= lo) & (v <= hi)      (torch's clamp and its gradient)
//   backward  gx = flip(H flip(mask ? g : 0)): the anti-causal filter H^T, THE SAME KERNEL with the sample index reversed at
//             the loads and stores (position q of the kernel's signal is sample T-1-q) and the mask applied at the load.
//
// Determinism contract: every output value is computed by ONE fixed sequence of float32 operations that does
// not depend on B, on how a batch is cut into calls, or on the launch geometry.  (Forward values do not depend on T either;
// backward values do, through the flip.)  tests/freq_domain_restate.py restates the sequence below in numpy, operation
// for operation.  kFdChunk and kFdThreads are constants of the ARITHMETIC, not tuning knobs.
//
// Section k has float32 coefficients b0 b1 b2 a1 a2 (the float64 row divided by its a0, rounded once), state (s1, s2):
//       y  = fmaf(b0, x, s1);  s1' = fmaf(-a1, y, fmaf(b1, x, s2));  s2' = fmaf(-a2, y, b2 * x)      (transposed direct form II)
// With x = 0 the state advances by s' = A s, A = [[-a1, 1], [-a2, 0]], and the output is s1.  Host tables per section, in
// float64 from the ROUNDED a1, a2, each entry rounded to float32 once (fd_tables below):
//       r[i]   = first row of A^i, i = 0 .. C-1        (output at chunk position i for a unit carried-in state)
//       lev[d] = M^(2^d), d = 0 .. 5, M = A^C;   wav[e] = M^(64 * 2^e), e = 0 .. 3     (powers by repeated squaring)
// mv(N, o, v) = (fmaf(N01, o2, fmaf(N00, o1, v1)), fmaf(N11, o2, fmaf(N10, o1, v2))).
//
// The row is cut into passes of P = 1024 * C positions (zeros past T); thread j = 64 w + l (wave w, lane l) owns positions
// p0 + j C .. + C-1.  sp = the section's state at the start of the pass (0 for the first).  Per pass, per section, in order:
//   (a) from state 0, the recurrence over the C samples -> y[0..C-1], end state f.
//   (b) in the wave: v = f; for d = 0 .. 5: lanes l >= 2^d: v = mv(lev[d], v of lane l - 2^d, v).
//       over the block: t_u = v of lane 63 of wave u; t_0 = mv(wav[0], sp, t_0); for e = 0 .. 3: waves u >= 2^e:
//       t_u = mv(wav[e], t_(u - 2^e), t_u).  c = sp for wave 0, t_(w-1) otherwise; the next pass's sp = t_15.
//       u = c; for d = 0 .. 5: if bit d of l is set: u = mv(lev[d], u, 0).     (c advanced to the lane's chunk)
//       s_in = (v of lane l-1, or 0 for l = 0) + u                               (two plain additions)
//   (c) y[i] = fmaf(r[i][1], s_in2, fmaf(r[i][0], s_in1, y[i])), i = 0 .. C-1; y is the next section's x.
//
// Memory: the pass's P positions are loaded coalesced into LDS, each thread takes its chunk as one 16-byte LDS read
// (consecutive lanes, consecutive slots: conflict-free), and the results go back the same way; clamp and mask happen at the
// coalesced store.  One barrier per section (the wave totals, double-buffered), three per pass.
#include <cmath>
#include <cstdio>

#include "sg_internal.h"

#pragma clang fp contract(off)

using namespace sg;

namespace {

constexpr int kFdChunk = 4;                       // C: samples per lane
constexpr int kFdThreads = 1024;                  // 16 waves
constexpr int kFdWaves = kFdThreads / 64;
constexpr int kFdPass = kFdThreads * kFdChunk;    // P
constexpr int kFdMaxSections = 16;
constexpr int kFdMaxT = 0x7FFFFFFF - 2 * kFdPass;  // the pass loop counts positions in int
static_assert(kFdChunk == 4, "the chunk is moved as one float4");

struct FdSection {
    float b0, b1, b2, na1, na2;  // na = -a
    float lev[6][4];             // M^(2^d): m00 m01 m10 m11
    float wav[4][4];             // M^(64 2^e)
    float r[kFdChunk][2];
};
struct FdTables {
    FdSection sec[kFdMaxSections];
};
static_assert(sizeof(FdTables) <= 3600, "the tables travel as kernel arguments (4 KB with the rest)");

struct FdVec {
    float a, b;
};
__device__ __forceinline__ FdVec fd_mv(const float* n, FdVec o, FdVec v) {
    return FdVec{fmaf(n[1], o.b, fmaf(n[0], o.a, v.a)), fmaf(n[3], o.b, fmaf(n[2], o.a, v.b))};
}

// scale_p != null: the reference's rule (frequency_domain.py:46-51) from sg_input_scale's float: [lo_a, hi_a] when the call
// lies in the unit range (scale 32768), [lo_b, hi_b] otherwise; null: [lo_a, hi_a]
template <bool kBackward>
__global__ __launch_bounds__(kFdThreads) void fd_cascade_kernel(const float* __restrict__ in, const int8_t* __restrict__ mask_in,
                                                                float* __restrict__ out, int8_t* __restrict__ mask_out,
                                                                const float* __restrict__ scale_p, float lo_a, float hi_a,
                                                                float lo_b, float hi_b, int T, int S, const FdTables tab) {
    __shared__ __attribute__((aligned(16))) float sh[kFdPass];
    __shared__ float tot[2][kFdWaves][2];         // wave end states, by section parity
    __shared__ float sps[2][kFdMaxSections][2];   // pass-start states, by pass parity
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)blockIdx.x * (size_t)T;
    float lo = lo_a, hi = hi_a;
    if (!kBackward && scale_p && *scale_p == 1.f) lo = lo_b, hi = hi_b;
    if (tid < 2 * kFdMaxSections) sps[0][tid >> 1][tid & 1] = 0.f;

    int par = 0;
    for (int p0 = 0; p0 < T; p0 += kFdPass, par ^= 1) {
#pragma unroll
        for (int i = 0; i < kFdChunk; ++i) {
            const int q = p0 + tid + kFdThreads * i;
            float v = 0.f;
            if (q < T) {
                const size_t o = base + (size_t)(kBackward ? T - 1 - q : q);
                v = in[o];
                if (kBackward) v = mask_in[o] ? v : 0.f;
            }
            sh[tid + kFdThreads * i] = v;
        }
        __syncthreads();
        const float4 xv = reinterpret_cast<const float4*>(sh)[tid];
        float y[kFdChunk] = {xv.x, xv.y, xv.z, xv.w};

        for (int k = 0; k < S; ++k) {
            const FdSection& c = tab.sec[k];
            // (a)
            FdVec f{0.f, 0.f};
#pragma unroll
            for (int i = 0; i < kFdChunk; ++i) {
                const float x = y[i];
                const float yy = fmaf(c.b0, x, f.a);
                const float s1 = fmaf(c.na1, yy, fmaf(c.b1, x, f.b));
                const float s2 = fmaf(c.na2, yy, c.b2 * x);
                y[i] = yy;
                f = FdVec{s1, s2};
            }
            // (b) in the wave
            FdVec v = f;
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                const FdVec o{__shfl_up(v.a, 1u << d, 64), __shfl_up(v.b, 1u << d, 64)};
                const FdVec n = fd_mv(c.lev[d], o, v);
                if (lane >= (1 << d)) v = n;
            }
            if (lane == 63) tot[k & 1][wave][0] = v.a, tot[k & 1][wave][1] = v.b;
            __syncthreads();
            // over the block: every wave scans the 16 totals in its lanes 0 .. 15 (no second barrier)
            const FdVec sp{sps[par][k][0], sps[par][k][1]};
            FdVec t{0.f, 0.f};
            if (lane < kFdWaves) t = FdVec{tot[k & 1][lane][0], tot[k & 1][lane][1]};
            {
                const FdVec n = fd_mv(c.wav[0], sp, t);
                if (lane == 0) t = n;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const FdVec o{__shfl_up(t.a, 1u << e, 64), __shfl_up(t.b, 1u << e, 64)};
                const FdVec n = fd_mv(c.wav[e], o, t);
                if (lane >= (1 << e)) t = n;
            }
            const int src = wave > 0 ? wave - 1 : 0;
            FdVec u{__shfl(t.a, src, 64), __shfl(t.b, src, 64)};
            if (wave == 0) u = sp;
            if (tid == kFdWaves - 1) sps[par ^ 1][k][0] = t.a, sps[par ^ 1][k][1] = t.b;  // wave 0's lane 15 holds t_15
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                const FdVec n = fd_mv(c.lev[d], u, FdVec{0.f, 0.f});
                if ((lane >> d) & 1) u = n;
            }
            FdVec e{__shfl_up(v.a, 1, 64), __shfl_up(v.b, 1, 64)};
            if (lane == 0) e = FdVec{0.f, 0.f};
            const FdVec s_in{e.a + u.a, e.b + u.b};
            // (c)
#pragma unroll
            for (int i = 0; i < kFdChunk; ++i) y[i] = fmaf(c.r[i][1], s_in.b, fmaf(c.r[i][0], s_in.a, y[i]));
        }

        reinterpret_cast<float4*>(sh)[tid] = make_float4(y[0], y[1], y[2], y[3]);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kFdChunk; ++i) {
            const int q = p0 + tid + kFdThreads * i;
            if (q < T) {
                const float v = sh[tid + kFdThreads * i];
                if (kBackward) {
                    out[base + (size_t)(T - 1 - q)] = v;
                } else {
                    out[base + q] = fminf(fmaxf(v, lo), hi);
                    mask_out[base + q] = (int8_t)((v >= lo) & (v <= hi));
                }
            }
        }
        __syncthreads();
    }
}

struct Mat2 {
    double m00, m01, m10, m11;
};
inline Mat2 mat_mul(const Mat2& a, const Mat2& b) {
    return Mat2{a.m00 * b.m00 + a.m01 * b.m10, a.m00 * b.m01 + a.m01 * b.m11, a.m10 * b.m00 + a.m11 * b.m10,
                a.m10 * b.m01 + a.m11 * b.m11};
}
inline void mat_store(const Mat2& a, float* o) { o[0] = (float)a.m00, o[1] = (float)a.m01, o[2] = (float)a.m10, o[3] = (float)a.m11; }

// poles of z^2 + a1 z + a2 strictly inside the unit circle
inline bool fd_stable(double a1, double a2) { return std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2; }

// sos (S,6) float64 -> the kernel's tables; 0, or the 1-based number of the first section that is refused (why in *why)
int fd_tables(const double* sos, int S, FdTables* tab, const char** why) {
    for (int k = 0; k < S; ++k) {
        const double* row = sos + 6 * k;
        for (int i = 0; i < 6; ++i)
            if (!std::isfinite(row[i])) return *why = "a coefficient is not finite", k + 1;
        if (row[3] == 0.0) return *why = "a0 is zero", k + 1;
        FdSection& c = tab->sec[k];
        c.b0 = (float)(row[0] / row[3]), c.b1 = (float)(row[1] / row[3]), c.b2 = (float)(row[2] / row[3]);
        const float a1 = (float)(row[4] / row[3]), a2 = (float)(row[5] / row[3]);
        c.na1 = -a1, c.na2 = -a2;
        if (!std::isfinite(c.b0) || !std::isfinite(c.b1) || !std::isfinite(c.b2) || !std::isfinite(a1) || !std::isfinite(a2))
            return *why = "a coefficient overflows float32", k + 1;
        // (the float64 design AND the rounded coefficients the recurrence runs with)
        if (!fd_stable(row[4] / row[3], row[5] / row[3]) || !fd_stable((double)a1, (double)a2))
            return *why = "its poles are not strictly inside the unit circle", k + 1;
        const Mat2 A{-(double)a1, 1.0, -(double)a2, 0.0};
        Mat2 p{1.0, 0.0, 0.0, 1.0};  // A^i
        for (int i = 0; i < kFdChunk; ++i) {
            c.r[i][0] = (float)p.m00, c.r[i][1] = (float)p.m01;
            p = mat_mul(p, A);
        }
        for (int d = 0; d < 6; ++d) {  // p = M^(2^d)
            mat_store(p, c.lev[d]);
            p = mat_mul(p, p);
        }
        for (int e = 0; e < 4; ++e) {  // p = M^(64 2^e)
            mat_store(p, c.wav[e]);
            p = mat_mul(p, p);
        }
    }
    for (int k = S; k < kFdMaxSections; ++k) tab->sec[k] = FdSection{};
    return 0;
}

// what a spec alone can get wrong about its sections; builds the kernel's tables on the way
int fd_check_sections(sg_ctx* ctx, const char* who, const sg_wav_filter* f, FdTables* tab) {
    if (f->n_sections < 1 || f->n_sections > kFdMaxSections)
        return fail(ctx, SG_ERR_ARG, "%s: 1 .. %d sections are built (%d)", who, kFdMaxSections, f->n_sections);
    const char* why = "";
    const int bad = fd_tables(f->sos, f->n_sections, tab, &why);
    if (bad) return fail(ctx, SG_ERR_ARG, "%s: section %d of %d: %s", who, bad, f->n_sections, why);
    return SG_OK;
}

int fd_check(sg_ctx* ctx, const char* who, const sg_wav_filter* f, const void* a, const void* b, const void* c, int32_t B,
             int32_t T, FdTables* tab) {
    if (!ctx) return SG_ERR_ARG;
    if (!f || !a || !b || !c || !f->sos) return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    if (B < 1 || T < 1 || T > kFdMaxT) return fail(ctx, SG_ERR_ARG, "%s: need B >= 1 and 1 <= T <= %d (B %d, T %d)", who, kFdMaxT, B, T);
    if (int rc = fd_check_sections(ctx, who, f, tab)) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    return SG_OK;
}

// the forward's clip range from the spec: [lo_a, hi_a] in the unit range (or given), [lo_b, hi_b] otherwise
int fd_clip(sg_ctx* ctx, const char* who, const sg_wav_filter* f, bool have_scale, float* lo_a, float* hi_a, float* lo_b, float* hi_b) {
    *lo_a = -1.f, *hi_a = 1.f, *lo_b = 0.f, *hi_b = 0.f;
    if (f->clip_mode == SG_FD_CLIP_RANGE) {
        if (!have_scale) return fail(ctx, SG_ERR_ARG, "%s: SG_FD_CLIP_RANGE needs scale_dev", who);
        if (f->bits < 2 || f->bits > 24) return fail(ctx, SG_ERR_ARG, "%s: bits must be 2 .. 24 (%d)", who, f->bits);
        *lo_b = -(float)(1 << (f->bits - 1)), *hi_b = (float)((1 << (f->bits - 1)) - 1);
    } else if (f->clip_mode == SG_FD_CLIP_GIVEN) {
        if (!(f->clip_lo <= f->clip_hi)) return fail(ctx, SG_ERR_ARG, "%s: need clip_lo <= clip_hi", who);
        *lo_a = f->clip_lo, *hi_a = f->clip_hi;
    } else {
        return fail(ctx, SG_ERR_ARG, "%s: unknown clip_mode %d", who, f->clip_mode);
    }
    return SG_OK;
}

}  // namespace

int sg::wav_filter_check_spec(sg_ctx* ctx, const char* who, const sg_wav_filter* f) {
    if (!f->sos) return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    FdTables tab;
    if (int rc = fd_check_sections(ctx, who, f, &tab)) return rc;
    float lo_a, hi_a, lo_b, hi_b;
    return fd_clip(ctx, who, f, true, &lo_a, &hi_a, &lo_b, &hi_b);
}

extern "C" int sg_wav_filter_forward(sg_ctx* ctx, const sg_wav_filter* f, const float* x_dev, int32_t B, int32_t T,
                                     const float* scale_dev, float* out_dev, int8_t* mask_dev, void* stream) {
    FdTables tab;
    int rc = fd_check(ctx, "sg_wav_filter_forward", f, x_dev, out_dev, mask_dev, B, T, &tab);
    if (rc) return rc;
    float lo_a, hi_a, lo_b, hi_b;
    if ((rc = fd_clip(ctx, "sg_wav_filter_forward", f, scale_dev != nullptr, &lo_a, &hi_a, &lo_b, &hi_b))) return rc;
    if (f->clip_mode == SG_FD_CLIP_GIVEN) scale_dev = nullptr;
    hipStream_t s = (hipStream_t)stream;
    trace_mark(ctx, SG_STAGE_FD_FWD, s, 0);
    hipLaunchKernelGGL(fd_cascade_kernel<false>, dim3(B), dim3(kFdThreads), 0, s, x_dev, (const int8_t*)nullptr, out_dev, mask_dev,
                       scale_dev, lo_a, hi_a, lo_b, hi_b, T, f->n_sections, tab);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_wav_filter_forward: %s", hipGetErrorString(e));
    trace_mark(ctx, SG_STAGE_FD_FWD, s, 1);
    return SG_OK;
}

extern "C" int sg_wav_filter_backward(sg_ctx* ctx, const sg_wav_filter* f, const float* g_dev, const int8_t* mask_dev, int32_t B,
                                      int32_t T, float* gx_dev, void* stream) {
    FdTables tab;
    int rc = fd_check(ctx, "sg_wav_filter_backward", f, g_dev, mask_dev, gx_dev, B, T, &tab);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    trace_mark(ctx, SG_STAGE_FD_BWD, s, 0);
    hipLaunchKernelGGL(fd_cascade_kernel<true>, dim3(B), dim3(kFdThreads), 0, s, g_dev, mask_dev, gx_dev, (int8_t*)nullptr,
                       (const float*)nullptr, 0.f, 0.f, 0.f, 0.f, T, f->n_sections, tab);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_wav_filter_backward: %s", hipGetErrorString(e));
    trace_mark(ctx, SG_STAGE_FD_BWD, s, 1);
    return SG_OK;
}
