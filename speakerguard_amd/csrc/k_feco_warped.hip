// FeCo with warped k-means (reference defense/feature_level.py:53-165): the frames of an utterance are cut into k
// CONTIGUOUS segments -- initial boundaries from TS (:53-77), from a random draw (:80-85) or given -- and the boundaries
// are then moved one frame at a time while a move lowers the squared error (wk_compute, :114-154).  The result is the k
// segment means.  A sequential, data-dependent sweep: one wave per (utterance, EOT repeat) row, lanes over the D <= 64
// feature dimensions, frames (when they fit) and means in LDS; every decision is made by the whole wave at once.
//
// DETERMINISM CONTRACT (restated in tests/feco_warped_restate.py, checked bit for bit):
//   * float32 throughout (no fused multiply-add: fp contract off); counts are int32 and converted to float where the
//     reference mixes them into float arithmetic;
//   * every sum over the feature dimensions -- sum((x - m)^2) of delta_SQE and the squared TS norm -- is the xor butterfly
//     over 64 lanes, d >= D zero: s[d] += s[d ^ 1], then ^ 2, ^ 4, ^ 8, ^ 16, ^ 32 (every step all d at once), which is the
//     pairwise tree over adjacent blocks of the padded vector; the TS norm is sqrtf of it (correctly rounded);
//   * TS: distance[0] = 0, distance[i] = distance[i - 1] + norm(x_i - x_{i-1}) in ascending i (sequential float32 prefix
//     sum); seg_dist = distance[F - 1] / (float)k; boundary j (1 <= j < k) is the first index after the previous boundary
//     with required_dist = seg_dist * (float)j <= distance[index] (F if none); then the reference's surpass fix-up (:67-76),
//     which stops at index 2;
//   * random init: the k - 1 frames of lowest (Philox4x32-10(counter = (frame, 0, utterance lo, utterance hi), key) word 0,
//     frame) among frames 1 .. F - 1, sorted, after 0 -- keyed like oracle/philox.py feco_random_init, with the global
//     utterance index_base + u and key + r * kRepKey for row r * rep_rows + u (EOT repeat r);
//   * the initial boundaries must rise strictly from 0 (a TS init of a pathological input does not: the reference then
//     takes means of empty slices, NaN); a row whose boundaries do not is refused (SG_ERR_ARG), it never yields NaN;
//   * initial segment means (:88-107): the segment's frames summed in ascending frame order from 0.f, / (float)count;
//   * the sweep (:120-153): for i = 0 .. k-1, first the left boundary of segment i moving forward over
//     j = b_i .. b_i + floor(c_i / 2 * (1 - delta)) - 1, then its right boundary moving backward over
//     j = b_{i+1} - 1 down to b_{i+1} - 1 - floor(c_i / 2 * (1 - delta)) + 1 (both ranges fixed when the loop starts, the
//     floor taken in double, c_i the count at that moment); at frame j with neighbour segment l,
//     delta_SQE = (s_l * (float)c_l) / (float)(c_l + 1) - (s_i * (float)c_i) / (float)(c_i - 1), s = sum((x_j - m)^2);
//     the frame moves when c_i > 1 and delta_SQE < 0, else the loop ends; a move does c_i -= 1, c_l += 1,
//     m_i -= (x_j - m_i) / (float)c_i, then m_l += (x_j - m_l) / (float)c_l (the reference's order, :135-136 / :150-151);
//   * sweeps repeat until one moves nothing; the count includes that last sweep.  The reference's `while` has no cap;
//     here a row still moving after 4 F sweeps stops and is reported (SG_ERR_STATE), it never hangs.
// The reference moves the means through `.data`, so its autograd sees only the INITIAL segment means: the gradient is
// sg_feco_compress_backward of the initial segment ids and counts this kernel returns (no kernel of its own).
#include <cmath>
#include <cstdio>
#include <vector>

#include "sg_internal.h"
#include "philox.h"

#pragma clang fp contract(off)

using namespace sg;

namespace {

constexpr int kWarpMaxF = 1200;   // 12 s of 10 ms frames
constexpr int kWarpMaxD = 64;     // one lane per dimension
constexpr size_t kWarpLdsMax = 150 * 1024;
constexpr int kWarpBadInit = -1;  // sweeps[row]: initial boundaries not strictly increasing from 0
constexpr int kWarpCapped = -2;   // sweeps[row]: still moving after the cap

__host__ __device__ constexpr int wal4(int n) { return (n + 3) & ~3; }

// dynamic LDS in 4-byte words: boundaries, counts, scratch (TS distances / random keys), flag, [means], [frames]
struct WarpLds {
    int bnd, cnt, scr, flag, means, x, total;
};
__host__ __device__ inline WarpLds warp_layout(int F, int k, int D, int means_in, int x_in) {
    WarpLds L;
    int o = 0;
    L.bnd = o; o += wal4(k);
    L.cnt = o; o += wal4(k);
    L.scr = o; o += wal4(F);
    L.flag = o; o += 4;
    L.means = o; o += means_in ? wal4(k * D) : 0;
    L.x = o; o += x_in ? F * D : 0;
    L.total = o;
    return L;
}

// What sg_feco_warped launches for a shape (pure) -- the instantiation <wide, xl, ml> and its dynamic LDS: the means live in LDS
// when they fit, the frames when both fit
struct FecoWarpedPlan {
    int wide, xl, ml;
    size_t lds;
};
inline FecoWarpedPlan feco_warped_plan(int F, int k, int D) {
    const auto bytes = [&](int ml, int xl) { return (size_t)warp_layout(F, k, D, ml, xl).total * sizeof(float); };
    const int ml = bytes(1, 0) <= kWarpLdsMax;
    const int xl = ml && bytes(1, 1) <= kWarpLdsMax;
    return {D > 32, xl, ml, bytes(ml, xl)};
}

__device__ __forceinline__ float rfl(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }

// xor swizzle inside 32-lane groups (ds_swizzle bit mode: and 0x1F, xor m)
template <int M>
__device__ __forceinline__ float swz(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1F | (M << 10)));
}

// the contract's butterfly; with D <= 32 the ^ 32 step only adds the zero upper half and is skipped.  The result is the
// same in every lane that matters (lane 0 is read by readfirstlane).
template <bool WIDE>
__device__ __forceinline__ float bfly(float s) {
    s = s + swz<1>(s);
    s = s + swz<2>(s);
    s = s + swz<4>(s);
    s = s + swz<8>(s);
    s = s + swz<16>(s);
    if (WIDE) s = s + __shfl_xor(s, 32, 64);
    return s;
}

// WIDE: D > 32.  XL: frames in LDS (else read from `feats`).  ML: means in LDS (else worked on in `out` directly).
template <bool WIDE, bool XL, bool ML>
__global__ __launch_bounds__(64) void feco_warped_kernel(const float* __restrict__ feats, int F, int D, int k, int mode,
                                                         double delta, unsigned long long key, long long index_base,
                                                         int rep_rows, int cap, int* __restrict__ bnd_io,
                                                         int* __restrict__ init_ids, int* __restrict__ init_counts,
                                                         float* __restrict__ out, int* __restrict__ sweeps) {
    constexpr int DP = WIDE ? 64 : 32;
    extern __shared__ float lds[];
    const WarpLds L = warp_layout(F, k, D, ML, XL);
    int* bnd = reinterpret_cast<int*>(lds + L.bnd);
    int* cnt = reinterpret_cast<int*>(lds + L.cnt);
    float* scr = lds + L.scr;
    int* flag = reinterpret_cast<int*>(lds + L.flag);
    const int row = blockIdx.x;
    const int lane = threadIdx.x;
    const float* xg = feats + (size_t)row * F * D;
    float* orow = out + (size_t)row * k * D;
    int* brow = bnd_io + (size_t)row * k;
    const bool act = lane < D;

    float* xs;
    if constexpr (XL) {
        xs = lds + L.x;
        for (int e = lane; e < F * D; e += 64) xs[e] = xg[e];
    }
    float* ms;
    if constexpr (ML) ms = lds + L.means; else ms = orow;
    auto xat = [&](int j) -> float {
        if constexpr (XL) return act ? xs[j * D + lane] : 0.f;
        else return act ? xg[(size_t)j * D + lane] : 0.f;
    };
    if (lane == 0) flag[0] = 0;
    __syncthreads();

    // ---- initial boundaries ---------------------------------------------------------------------------------------
    if (mode == 0) {
        // TS (:53-77): squared distances of consecutive frames, one frame per lane, the butterfly's tree in registers
        for (int i = 1 + lane; i < F; i += 64) {
            float s[DP];
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                float v = 0.f;
                if (d < D) {
                    if constexpr (XL) v = xs[i * D + d] - xs[(i - 1) * D + d];
                    else v = xg[(size_t)i * D + d] - xg[(size_t)(i - 1) * D + d];
                }
                s[d] = v * v;
            }
#pragma unroll
            for (int w = DP / 2; w >= 1; w >>= 1)
#pragma unroll
                for (int q = 0; q < w; ++q) s[q] = s[2 * q] + s[2 * q + 1];
            scr[i] = __fsqrt_rn(s[0]);
        }
        __syncthreads();
        if (lane == 0) {
            float acc = 0.f;
            scr[0] = 0.f;
            for (int i = 1; i < F; ++i) {
                acc = acc + scr[i];
                scr[i] = acc;
            }
            const float seg = scr[F - 1] / (float)k;
            bnd[0] = 0;
            int index = 0, last = 0;
            for (int j = 1; j < k; ++j) {
                const float req = seg * (float)j;
                while (index < F && (req > scr[index] || index == last)) ++index;
                bnd[j] = index;
                last = index;
            }
            int p = k;  // first boundary equal to F (they do not decrease: a tail)
            while (p > 0 && bnd[p - 1] == F) --p;
            const int ns = k - p;
            if (ns > 0) {
                for (int i = 0; i < ns; ++i) bnd[p + i] = F - ns + i;
                for (int i = p - 1; i > 1; --i) {
                    if (bnd[i] >= bnd[i + 1]) bnd[i] = bnd[i + 1] - 1;
                    else break;
                }
            }
        }
    } else if (mode == 1) {
        // random init (:80-85): rank of frame f among frames 1 .. F-1 by (key, frame); the k - 1 lowest, in frame order
        const int rep = rep_rows > 0 ? row / rep_rows : 0;
        const long long utt = index_base + (rep_rows > 0 ? row - rep * rep_rows : row);
        const unsigned long long rkey = key + (unsigned long long)rep * kRepKey;
        unsigned* keys = reinterpret_cast<unsigned*>(scr);
        for (int f = lane; f < wal4(F); f += 64)
            keys[f] = f < F ? philox4x32_10_w0(rkey, (uint32_t)f, 0u, (uint32_t)utt, (uint32_t)((unsigned long long)utt >> 32))
                            : 0xFFFFFFFFu;
        if (lane == 0) bnd[0] = 0;
        __syncthreads();
        int base = 1;
        for (int c0 = 1; c0 < F; c0 += 64) {
            const int f = c0 + lane;
            bool sel = false;
            if (f < F) {
                const unsigned kf = keys[f];
                int rank = 0;
                for (int g = 0; g < wal4(F); g += 4) {
                    const uint4 kg = *reinterpret_cast<const uint4*>(keys + g);
                    const unsigned kk[4] = {kg.x, kg.y, kg.z, kg.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int gg = g + t;
                        rank += (gg >= 1 && gg < F && (kk[t] < kf || (kk[t] == kf && gg < f))) ? 1 : 0;
                    }
                }
                sel = rank < k - 1;
            }
            const unsigned long long m = __ballot(sel);
            if (sel) bnd[base + __popcll(m & ((1ULL << lane) - 1ULL))] = f;
            base += __popcll(m);
        }
    } else {
        for (int i = lane; i < k; i += 64) bnd[i] = brow[i];
    }
    __syncthreads();
    if (lane == 0) {
        bool ok = bnd[0] == 0 && bnd[k - 1] < F;
        for (int i = 1; i < k && ok; ++i) ok = bnd[i] > bnd[i - 1];
        flag[0] = ok ? 0 : 1;
    }
    __syncthreads();
    if (rfl(flag[0])) {
        for (int e = lane; e < k * D; e += 64) orow[e] = 0.f;
        for (int i = lane; i < k; i += 64) {
            brow[i] = bnd[i];
            init_counts[(size_t)row * k + i] = 0;
        }
        for (int f = lane; f < F; f += 64) init_ids[(size_t)row * F + f] = -1;
        if (lane == 0) sweeps[row] = kWarpBadInit;
        return;
    }

    // ---- init (:88-107): counts, segment ids, segment means ---------------------------------------------------------
    for (int i = lane; i < k; i += 64) {
        const int c = (i + 1 < k ? bnd[i + 1] : F) - bnd[i];
        cnt[i] = c;
        init_counts[(size_t)row * k + i] = c;
    }
    for (int f = lane; f < F; f += 64) {
        int lo = 0, hi = k - 1;  // last boundary <= f
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (bnd[mid] <= f) lo = mid; else hi = mid - 1;
        }
        init_ids[(size_t)row * F + f] = lo;
    }
    __syncthreads();
    for (int i = 0; i < k; ++i) {
        const int b0 = rfl(bnd[i]), b1 = i + 1 < k ? rfl(bnd[i + 1]) : F;
        float sum = 0.f;
        int j = b0;
        for (; j + 4 <= b1; j += 4) {  // four loads in flight, additions in ascending frame order
            const float v0 = xat(j), v1 = xat(j + 1), v2 = xat(j + 2), v3 = xat(j + 3);
            sum = sum + v0;
            sum = sum + v1;
            sum = sum + v2;
            sum = sum + v3;
        }
        for (; j < b1; ++j) sum = sum + xat(j);
        if (act) ms[i * D + lane] = sum / (float)(b1 - b0);
    }
    __syncthreads();

    // ---- wk_compute (:118-153) ----------------------------------------------------------------------------------------
    auto mload = [&](int i) -> float { return act ? ms[i * D + lane] : 0.f; };
    auto mstore = [&](int i, float v) { if (act) ms[i * D + lane] = v; };
    int sw = 0;
    bool moved = true;
    while (moved && sw < cap) {
        moved = false;
        ++sw;
        float mi = mload(0), mprev = 0.f;  // means of segments i and i - 1, carried in registers along the sweep
        for (int i = 0; i < k; ++i) {
            int ci = rfl(cnt[i]);
            if (i > 0) {  // left boundary of segment i moves forward into segment i - 1
                int cl = rfl(cnt[i - 1]);
                const int begin = rfl(bnd[i]);
                const int end = begin + (int)floor((double)ci / 2.0 * (1.0 - delta));
                int j = begin;
                for (; j < end && j < F; ++j) {
                    if (ci <= 1) break;
                    const float x = xat(j);
                    const float dl = x - mprev, dj = x - mi;
                    const float sl = rfl(bfly<WIDE>(dl * dl)), sj = rfl(bfly<WIDE>(dj * dj));
                    const float dsq = (sl * (float)cl) / (float)(cl + 1) - (sj * (float)ci) / (float)(ci - 1);
                    if (!(dsq < 0.f)) break;
                    moved = true;
                    ci -= 1;
                    cl += 1;
                    mi = mi - (x - mi) / (float)ci;
                    mprev = mprev + (x - mprev) / (float)cl;
                }
                if (j != begin) {
                    bnd[i] = j;
                    cnt[i] = ci;
                    cnt[i - 1] = cl;
                }
                mstore(i - 1, mprev);  // segment i - 1 is final for this sweep
            }
            if (i < k - 1) {  // right boundary of segment i moves backward into segment i + 1
                int cr = rfl(cnt[i + 1]);
                float mr = mload(i + 1);
                const int b1 = rfl(bnd[i + 1]);
                const int end = b1 - 1;
                const int begin = end - (int)floor((double)ci / 2.0 * (1.0 - delta));
                int j = end;
                for (; j > begin && j >= 0; --j) {
                    if (ci <= 1) break;
                    const float x = xat(j);
                    const float dr = x - mr, dj = x - mi;
                    const float sr = rfl(bfly<WIDE>(dr * dr)), sj = rfl(bfly<WIDE>(dj * dj));
                    const float dsq = (sr * (float)cr) / (float)(cr + 1) - (sj * (float)ci) / (float)(ci - 1);
                    if (!(dsq < 0.f)) break;
                    moved = true;
                    ci -= 1;
                    cr += 1;
                    mi = mi - (x - mi) / (float)ci;
                    mr = mr + (x - mr) / (float)cr;
                }
                if (j != end) {
                    bnd[i + 1] = j + 1;
                    cnt[i] = ci;
                    cnt[i + 1] = cr;
                }
                mprev = mi;
                mi = mr;
            } else {
                mstore(i, mi);
            }
        }
    }
    __syncthreads();
    if constexpr (ML)
        for (int e = lane; e < k * D; e += 64) orow[e] = ms[e];
    for (int i = lane; i < k; i += 64) brow[i] = bnd[i];
    if (lane == 0) sweeps[row] = moved ? kWarpCapped : sw;
}

template <bool WIDE, bool XL, bool ML>
hipError_t launch_warped(int B, size_t lds, hipStream_t s, const float* feats, int F, int D, int k, int mode, double delta,
                         uint64_t key, int64_t index_base, int rep_rows, int cap, int32_t* bnd, int32_t* ids, int32_t* counts,
                         float* out, int32_t* sweeps) {
    auto fn = feco_warped_kernel<WIDE, XL, ML>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3(B), dim3(64), lds, s, feats, F, D, k, mode, delta, (unsigned long long)key,
                       (long long)index_base, rep_rows, cap, bnd, ids, counts, out, sweeps);
    return hipGetLastError();
}

}  // namespace

extern "C" int sg_feco_warped(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                              int32_t init_mode, double delta, uint64_t key, int64_t index_base, int32_t rep_rows,
                              int32_t* boundaries_dev, int32_t* init_ids_dev, int32_t* init_counts_dev, float* out_dev,
                              int32_t* sweeps_dev, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (!feats_dev || !boundaries_dev || !init_ids_dev || !init_counts_dev || !out_dev || !sweeps_dev)
        return fail(ctx, SG_ERR_ARG, "sg_feco_warped: null pointer argument");
    if (B <= 0 || B > 65535 || F <= 0 || F > kWarpMaxF || D <= 0 || D > kWarpMaxD || k < 1 || k > F)
        return fail(ctx, SG_ERR_ARG, "sg_feco_warped: need 0 < B <= 65535, 0 < F <= %d, 0 < D <= %d, 1 <= k <= F "
                         "(got B %d, F %d, D %d, k %d)", kWarpMaxF, kWarpMaxD, B, F, D, k);
    if (init_mode < 0 || init_mode > 2 || rep_rows < 0 || !(delta >= 0.0 && delta <= 1.0))
        return fail(ctx, SG_ERR_ARG, "sg_feco_warped: need init_mode 0 (ts) / 1 (random) / 2 (given), rep_rows >= 0, "
                         "0 <= delta <= 1");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_warped: hipSetDevice failed");
    const FecoWarpedPlan plan = feco_warped_plan(F, k, D);
    const int cap = 4 * F;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    switch ((plan.wide ? 4 : 0) | (plan.xl ? 2 : 0) | plan.ml) {
#define SG_WARP_CASE(W, X, M)                                                                                              \
    case (W ? 4 : 0) | (X ? 2 : 0) | M:                                                                                     \
        e = launch_warped<W, X, M>(B, plan.lds, s, feats_dev, F, D, k, init_mode, delta, key, index_base, rep_rows, cap,   \
                                   boundaries_dev, init_ids_dev, init_counts_dev, out_dev, sweeps_dev);                    \
        break;
        SG_WARP_CASE(false, false, false)
        SG_WARP_CASE(false, false, true)
        SG_WARP_CASE(false, true, true)
        SG_WARP_CASE(true, false, false)
        SG_WARP_CASE(true, false, true)
        SG_WARP_CASE(true, true, true)
#undef SG_WARP_CASE
        default:  // (frames in LDS without the means: feco_warped_plan never plans it)
            return fail(ctx, SG_ERR_ARG, "sg_feco_warped: no layout for F %d, D %d, k %d", F, D, k);
    }
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_warped: %s", hipGetErrorString(e));
    // the per-row status decides the return code: wait for it
    std::vector<int32_t> st((size_t)B);
    e = hipMemcpyAsync(st.data(), sweeps_dev, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_warped: %s", hipGetErrorString(e));
    for (int b = 0; b < B; ++b) {
        if (st[b] == kWarpBadInit)
            return fail(ctx, SG_ERR_ARG, "sg_feco_warped: row %d: the initial boundaries do not rise strictly from 0 "
                             "(%s); the reference would average empty segments (NaN)", b,
                             init_mode == 0 ? "degenerate TS init" : "bad boundaries given");
        if (st[b] == kWarpCapped)
            return fail(ctx, SG_ERR_STATE, "sg_feco_warped: row %d: boundaries still moving after %d sweeps (cap); "
                             "its means are those of the last sweep", b, cap);
    }
    return SG_OK;
}
