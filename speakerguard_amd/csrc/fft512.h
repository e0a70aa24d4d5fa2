// One-wave FFT-512 on a private, padded LDS buffer, the scalar type a template parameter -- shared by the MFCC front-end
// (k_mfcc.hip, 512-point frames), the AudioNet log-mel front-end (k_audionet.hip, 1024-point REAL frames done as one
// 512-point complex transform plus a split step) and STOI (k_stoi.hip).  float: the AudioNet reference's own STFT is float32
// (model/_audionet/Preprocessor.py:100-105 -> torch.stft), torchaudio 0.6's kaldi.mfcc likewise; double: the form of the
// first rounds, kept as the counterpart, and STOI's precision.  Twiddles are always computed in float64 on the host and
// rounded once (sg_internal.h, fft512_twiddle_tables).
#pragma once
#include <hip/hip_runtime.h>

#include "sg_internal.h"

namespace sg {

// Every LDS buffer here is private to one wave, and a wave's DS instructions execute in program order, so cross-lane
// hand-offs through LDS need no s_barrier -- only a fence that stops the compiler from moving LDS accesses across it.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 512-point complex FFT of one wave, natural order in, "transform order" out (or the reverse: the transposed network below).
// 512 = 8 x 8 x 8: three passes of in-register radix-8 butterflies, one butterfly per lane and pass,
// with an LDS exchange between passes (Cooley-Tukey, decimation in frequency):
//   n = 64 n1 + n2,  k = k1 + 8 c + 64 d
//   pass 1  lane n2       : DFT8 over n1, times W512^(n2 k1)          -> y[k1][n2]
//   pass 2  lane (k1, b)  : DFT8 over a of y[k1][8a + b], times W64^(b c) -> z[k1][b][c]
//   pass 3  lane (k1, c)  : DFT8 over b of z[k1][b][c]                 -> X[k1 + 8c + 64d]
// 48 LDS accesses per lane instead of the 144 of a radix-2 network, and 6 wave-level fences instead
// of 9 (measured on the MFCC forward kernel: FFT share 55 us -> see profiles/).
// sgn = -1: forward transform; +1: unnormalised inverse (conjugate twiddles).
// The work buffer keeps element i at SP(i) = i + i/8 (one element of pad per 8 elements). ds_write_b128
// is served in groups of 8 consecutive lanes over 32 banks (128 B): unpadded, the pass-2 and pass-3
// scatters put all 8 lanes of a group on one bank slot (stride 128 B) -- 8x the LDS cycles, which made
// the FFT ~1500 LDS cycles per frame and the whole kernel LDS-issue bound. With the pad every access
// pattern below is conflict-free within its lane group.  With 8-byte elements (float) the pass-2 / pass-3 gathers
// (lane (k1, b): 72 k1 + b + 9 a) stay conflict-free for ds_read_b64 (32 lanes over 64 banks: 8 k1 + b covers 32 distinct
// 8-byte slots) and the scatters for ds_write_b64 (16 lanes: 9 b + 8 k1 mod 16 distinct).
#define SP(i) ((i) + ((i) >> 3))

// The twiddles of passes 1 and 2 sit in dedicated tables (PMC, MFCC forward: of 240 bank-conflict cycles per
// frame 152 came from the transform, and the butterfly exchanges are conflict-free -- it was the GATHER of twiddles from a
// half-circle table: pass 2 reads tw[8 b c], eight distinct addresses per 16-lane group all on one or two 16-byte slots of
// the 256-byte bank row, 4- to 8-way, ~130 extra LDS cycles per transform):
//   tw1[(j - 1) * 64 + lane] = W512^(j lane), j = 1..7   (lane-linear reads: conflict-free)
//   tw2[9 b + c]             = W64^(b c),     b, c < 8   (row pad 1: the eight b of a lane group fall on eight slots)
// both for the forward sign; sgn = +1 conjugates.  kFftTw1 / kFftTw2 elements, laid out by the host (sg_internal.h).

template <typename T> struct Cx;
template <> struct Cx<float> { using type = float2; };
template <> struct Cx<double> { using type = double2; };
template <typename T> using cx = typename Cx<T>::type;

// No implicit contraction in the front-end's arithmetic (round 5): the same per-frame functions are instantiated in five
// kernels (forward, adjoint with / without the caches, with / without the fused overlap-add) that must give the SAME bits,
// and what -ffp-contract fuses depends on the code around an expression.  Every fused multiply-add is written out.
#pragma clang fp contract(off)
__device__ __forceinline__ float fmaT(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fmaT(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T> __device__ __forceinline__ cx<T> cmk(T x, T y) { cx<T> r; r.x = x; r.y = y; return r; }
template <typename T> __device__ __forceinline__ cx<T> cmulT(cx<T> a, cx<T> b) {
    return cmk<T>(fmaT(a.x, b.x, -(a.y * b.y)), fmaT(a.x, b.y, a.y * b.x));
}
template <typename T> __device__ __forceinline__ cx<T> caddT(cx<T> a, cx<T> b) { return cmk<T>(a.x + b.x, a.y + b.y); }
template <typename T> __device__ __forceinline__ cx<T> csubT(cx<T> a, cx<T> b) { return cmk<T>(a.x - b.x, a.y - b.y); }
template <typename T> __device__ __forceinline__ cx<T> cconjT(cx<T> a) { return cmk<T>(a.x, -a.y); }
// multiply by sgn * i
template <typename T> __device__ __forceinline__ cx<T> cmuliT(cx<T> a, T sgn) { return cmk<T>(-sgn * a.y, sgn * a.x); }
template <typename T> __device__ __forceinline__ cx<T> tw_sgnT(cx<T> w, T sgn) { return cmk<T>(w.x, -sgn * w.y); }

template <typename T>
__device__ __forceinline__ void dft8T(cx<T>& a0, cx<T>& a1, cx<T>& a2, cx<T>& a3, cx<T>& a4, cx<T>& a5, cx<T>& a6, cx<T>& a7, T sgn) {
    const T h = (T)0.70710678118654752440;
    cx<T> b0 = caddT<T>(a0, a4), b4 = csubT<T>(a0, a4), b1 = caddT<T>(a1, a5), b5 = csubT<T>(a1, a5);
    cx<T> b2 = caddT<T>(a2, a6), b6 = csubT<T>(a2, a6), b3 = caddT<T>(a3, a7), b7 = csubT<T>(a3, a7);
    b5 = cmulT<T>(b5, cmk<T>(h, sgn * h));
    b6 = cmuliT<T>(b6, sgn);
    b7 = cmulT<T>(b7, cmk<T>(-h, sgn * h));
    const cx<T> c0 = caddT<T>(b0, b2), c2 = csubT<T>(b0, b2), c1 = caddT<T>(b1, b3), c3 = cmuliT<T>(csubT<T>(b1, b3), sgn);
    const cx<T> c4 = caddT<T>(b4, b6), c6 = csubT<T>(b4, b6), c5 = caddT<T>(b5, b7), c7 = cmuliT<T>(csubT<T>(b5, b7), sgn);
    a0 = caddT<T>(c0, c1); a1 = caddT<T>(c4, c5); a2 = caddT<T>(c2, c3); a3 = caddT<T>(c6, c7);
    a4 = csubT<T>(c0, c1); a5 = csubT<T>(c4, c5); a6 = csubT<T>(c2, c3); a7 = csubT<T>(c6, c7);
}

// The three passes, separately, with the transform's input and output in REGISTERS: a caller that knows its input (real,
// zero-padded: the MFCC forward; one-sided: the gradient spectrum) or needs only part of the output (bins 0..255; the real
// part of samples 0..399) skips the LDS traffic of the parts it does not need -- 16-byte LDS accesses are what these
// kernels are short of (PMC: the LDS pipe is busy 54 % of the MFCC forward kernel, 31 % of that in bank conflicts).
// pass 1: lane n2 holds v_j = x[n2 + 64 j]; leaves y[k1][n2] at SP(n2 + 64 k1)
template <typename T>
__device__ __forceinline__ void fft512_pass1T(cx<T>* buf, const cx<T>* __restrict__ tw1, int lane, T sgn, cx<T> v0, cx<T> v1, cx<T> v2,
                                              cx<T> v3, cx<T> v4, cx<T> v5, cx<T> v6, cx<T> v7) {
    cx<T>* p1 = buf + SP(lane);  // SP(lane + 64 j) = SP(lane) + 72 j
    dft8T<T>(v0, v1, v2, v3, v4, v5, v6, v7, sgn);
    p1[0] = v0;
    p1[72] = cmulT<T>(v1, tw_sgnT<T>(tw1[lane], sgn));
    p1[144] = cmulT<T>(v2, tw_sgnT<T>(tw1[64 + lane], sgn));
    p1[216] = cmulT<T>(v3, tw_sgnT<T>(tw1[128 + lane], sgn));
    p1[288] = cmulT<T>(v4, tw_sgnT<T>(tw1[192 + lane], sgn));
    p1[360] = cmulT<T>(v5, tw_sgnT<T>(tw1[256 + lane], sgn));
    p1[432] = cmulT<T>(v6, tw_sgnT<T>(tw1[320 + lane], sgn));
    p1[504] = cmulT<T>(v7, tw_sgnT<T>(tw1[384 + lane], sgn));
    wave_sync();
}
// pass 2: lane = (k1, b), in place
template <typename T>
__device__ __forceinline__ void fft512_pass2T(cx<T>* buf, const cx<T>* __restrict__ tw2, int lane, T sgn) {
    const int k1 = lane >> 3, b = lane & 7;
    const cx<T>* r = buf + k1 * 72 + b;  // SP(64 k1 + 8 a + b) = 72 k1 + 9 a + b
    cx<T> v0 = r[0], v1 = r[9], v2 = r[18], v3 = r[27], v4 = r[36], v5 = r[45], v6 = r[54], v7 = r[63];
    wave_sync();
    dft8T<T>(v0, v1, v2, v3, v4, v5, v6, v7, sgn);
    cx<T>* w = buf + k1 * 72 + 9 * b;  // z[k1][b][c] at SP(64 k1 + 8 b + c)
    const cx<T>* t2 = tw2 + 9 * b;
    w[0] = v0;
    w[1] = cmulT<T>(v1, tw_sgnT<T>(t2[1], sgn));
    w[2] = cmulT<T>(v2, tw_sgnT<T>(t2[2], sgn));
    w[3] = cmulT<T>(v3, tw_sgnT<T>(t2[3], sgn));
    w[4] = cmulT<T>(v4, tw_sgnT<T>(t2[4], sgn));
    w[5] = cmulT<T>(v5, tw_sgnT<T>(t2[5], sgn));
    w[6] = cmulT<T>(v6, tw_sgnT<T>(t2[6], sgn));
    w[7] = cmulT<T>(v7, tw_sgnT<T>(t2[7], sgn));
    wave_sync();
}
// pass 3: lane = (k1, c) = (lane >> 3, lane & 7); out[d] = X[k1 + 8 c + 64 d].  Ends with the fence that lets the caller
// overwrite the buffer.
template <typename T>
__device__ __forceinline__ void fft512_pass3T(const cx<T>* buf, int lane, T sgn, cx<T> (&out)[8]) {
    const int k1 = lane >> 3, c = lane & 7;
    const cx<T>* r = buf + k1 * 72 + c;
    cx<T> v0 = r[0], v1 = r[9], v2 = r[18], v3 = r[27], v4 = r[36], v5 = r[45], v6 = r[54], v7 = r[63];
    wave_sync();
    dft8T<T>(v0, v1, v2, v3, v4, v5, v6, v7, sgn);
    out[0] = v0; out[1] = v1; out[2] = v2; out[3] = v3; out[4] = v4; out[5] = v5; out[6] = v6; out[7] = v7;
}

// registers in (v_j = x[lane + 64 j]), registers out (lane (k1, c) = (lane >> 3, lane & 7): out[d] = X[k1 + 8 c + 64 d] -- "transform
// order": element k of such a spectrum sits at 64 d + lane, lane = 8 k1 + c); the buffer is free again on return
template <typename T>
__device__ __forceinline__ void fft512T_regs(cx<T>* buf, const cx<T>* __restrict__ tw1, const cx<T>* __restrict__ tw2, int lane, T sgn,
                                             const cx<T> (&in)[8], cx<T> (&out)[8]) {
    fft512_pass1T<T>(buf, tw1, lane, sgn, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7]);
    fft512_pass2T<T>(buf, tw2, lane, sgn);
    fft512_pass3T<T>(buf, lane, sgn, out);
}

// The TRANSPOSED network (round 5): the three passes run backwards, each one transposed.  The DFT matrix is symmetric, so
// this is the same transform with the roles of the two layouts swapped: input in transform order (lane (k1, c):
// v[d] = G[k1 + 8 c + 64 d]), output in natural order (v[j] = g[lane + 64 j]), both in registers.  After a spectrum that
// was produced in transform order by fft512T_regs, the inverse needs no exchange in front of it and none behind it: two LDS
// round trips instead of five (the adjoint of the log-mel front-end, k_audionet.hip).
//   T3: DFT-8 over d -> b, times W64^(b c), to 72 k1 + 9 b + c        (the pass-2 gather pattern, as a scatter)
//   T2: lane (k1, b) reads c = 0..7, DFT-8 over c -> a, to 72 k1 + 9 a + b  (the pass-2 scatter / gather patterns swapped)
//   T1: lane n2 reads SP(n2) + 72 k1, times W512^(k1 n2), DFT-8 over k1 -> j
template <typename T>
__device__ __forceinline__ void fft512T_transposed(cx<T>* buf, const cx<T>* __restrict__ tw1, const cx<T>* __restrict__ tw2, int lane, T sgn,
                                                   cx<T> (&v)[8]) {
    const int k1 = lane >> 3, c = lane & 7;
    dft8T<T>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], sgn);
    {
        const cx<T>* t2 = tw2 + 9 * c;
        cx<T>* w = buf + k1 * 72 + c;
        w[0] = v[0];
#pragma unroll
        for (int b = 1; b < 8; ++b) w[9 * b] = cmulT<T>(v[b], tw_sgnT<T>(t2[b], sgn));
    }
    wave_sync();
    {
        const cx<T>* r = buf + k1 * 72 + 9 * c;  // this lane as (k1, b = lane & 7)
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = r[i];
    }
    wave_sync();
    dft8T<T>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], sgn);
    {
        cx<T>* w = buf + k1 * 72 + c;
#pragma unroll
        for (int a = 0; a < 8; ++a) w[9 * a] = v[a];
    }
    wave_sync();
    {
        const cx<T>* p1 = buf + SP(lane);
        v[0] = p1[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) v[j] = cmulT<T>(p1[72 * j], tw_sgnT<T>(tw1[(j - 1) * 64 + lane], sgn));
    }
    wave_sync();
    dft8T<T>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], sgn);
}

#pragma clang fp contract(fast)

}  // namespace sg
