// FeCo k-means for WIDE frames, 65 <= D <= 128 (iv_plda's delta and CMVN features are 72 wide): the whole forward of the
// defense -- clustering + cluster means -- as sg_feco_kmeans_compress_wide.  The entries of k_feco.hip stop at 64 columns
// and keep doing so; this is a kernel of its own, not a third instantiation of theirs: at 1024 threads and 128 registers
// a lane the 64-wide instantiation already spills, so this block is 512 threads (256 registers a lane) and keeps the B
// operand of ONE frame tile in registers while the centroid rows stream through LDS.
//
// DETERMINISM CONTRACT "version 2, wide": version 2 of k_feco.hip's header with one change, the padded width is 128
// (restated in tests/feco_wide_restate.py on oracle/feco.py centre / half_norms(c, 128) and oracle/conv_chain.c
// sg_feco_scores at Dp = 128, checked bit for bit).  Everything fp32, fp contract off:
//   * centring: mu[d] = (p_0 + p_1 + ... + p_15 in that order) / F with p_q = sum over frames i = q, q + 16, ... ascending (from
//     0.f); x'[i][d] = x[i][d] - mu[d];
//   * k centroids, centroid j initialised to frame floor(j * F / k) -- or, seeded form (random_init != 0), to the frame of rank j
//     when the frames are ordered by (Philox4x32-10(counter = (frame, 0, utterance lo, utterance hi), key = seed) word 0, frame)
//     ascending, utterance = index_base + row (oracle/philox.py feco_random_init);
//   * assignment: frame i goes to the centroid with the LARGEST score(i, j), ties to the lowest index.  score(i, j) is ONE fp32
//     fmaf chain: it starts at h_j = -0.5f * n_j and adds fmaf(c_j[d], x'_i[d], .) over d in the contraction order (groups of 8
//     ascending, inside a group 0, 4, 1, 5, 2, 6, 3, 7; dimensions padded with zeros to 128) -- what v_mfma_f32_32x32x2_f32
//     computes.  n_j = the sum of the rounded squares c_j[d]^2 over the 128 zero-padded lanes by the butterfly s[d] += s[d ^ 1],
//     s[d ^ 2], ... s[d ^ 64] (every step all d at once).  A trailing group of zeros adds fmaf(0, 0, s) = s (or turns -0 into
//     +0, which no comparison sees), so the kernel runs only the ceil(D / 8) groups that hold a column: same ids;
//   * stop when no assignment changed or after max_iter assignment steps; otherwise update: centroid j = (sum of its frames x'
//     in ascending frame order, from 0.f) / count, an empty cluster keeps its centroid (and its h_j);
//   * the ids of the LAST assignment step are the result; out / counts = sg_feco_compress of those ids bit for bit (means of
//     the ORIGINAL frames over the final member lists, ascending sums, the `force` fallback to frame j for an empty cluster).
//
// The block: 8 waves.  A wave takes frame tiles w, w + 8, ... (32 frames each): it loads the tile's centred frames from
// global memory / L2 once per step (NG = ceil(D / 8) float4 per lane, all register-resident -- the kernel is instantiated per
// NG, so every register index is a constant), then walks ALL centroid tiles with the accumulators started at h_j: per tile NG
// ds_read_b128 of the centroid rows and 4 NG MFMAs in the chain's order, the lane's running maximum (ascending centroid,
// strict >), the two lane halves merged with ties to the lower index.  No chunking of the centroid tiles, so no merge arrays:
// at 300 x 150 x 72 the ten frame tiles give the SIMDs 3 / 3 / 2 / 2 units of 5 x 36 MFMAs (14 us of matrix-pipe time per step
// on the busiest against the 12 us of a perfect split).
// LDS (feco_wide_layout): the centroid rows [kp = (k + 31) & ~31][8 NG + 4] -- the stride is 4 (mod 8) floats, so the 16 lanes
// one ds_read_b128 cycle serves hit 16 different 16-byte slots without a permutation -- h, mu, the centring's partial sums,
// ids, counts, list starts, member lists.  The frames stay in global memory.  At D = 72 (stride 84) and ratio 0.5 the longest
// utterance is F = 833 (k = 416 = kp: 146 864 of the 153 600 bytes); F = 834 (k = 417, kp = 448: 156 736 bytes) is refused.
// F = 300, k = 150 takes 61 600 bytes.
// Launch discipline as next door: no float atomics, member lists in ascending frame order, sums in list order.
#include <cstdio>

#include "sg_internal.h"
#include "philox.h"
#include "wave_reduce.h"

#pragma clang fp contract(off)

using namespace sg;

namespace {

constexpr int kWideThreads = 512;
constexpr int kWideWaves = kWideThreads / 64;
constexpr int kWideMinD = 65, kWideMaxD = 128;
constexpr size_t kWideLdsMax = 150 * 1024;  // kFecoLdsMax of k_feco.hip
__host__ __device__ constexpr int wal4(int n) { return (n + 3) & ~3; }
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Dynamic LDS in 4-byte words (every array 16-byte aligned); host and device use the same function.
struct FecoWideLds {
    int cq, hq, mu, part, ids, cnt, start, members, total;
};
__host__ __device__ inline FecoWideLds feco_wide_layout(int F, int k, int ng) {
    const int kp = (k + 31) & ~31;
    FecoWideLds L;
    int o = 0;
    L.cq = o; o += kp * (8 * ng + 4);   // centred centroids, row stride 8 ng + 4
    L.hq = o; o += kp;                  // -|c|^2 / 2
    L.mu = o; o += 128;
    L.part = o; o += 16 * 128;          // partial sums of the centring
    L.ids = o; o += wal4(F);
    L.cnt = o; o += wal4(k);
    L.start = o; o += wal4(k + 1);
    L.members = o; o += wal4(F);        // frames grouped by cluster, ascending inside a group
    L.total = o;
    return L;
}

// What sg_feco_kmeans_compress_wide launches for a shape (pure): the dimension groups -- the instantiation -- and its dynamic LDS
struct FecoWidePlan {
    int ng;
    size_t lds;
};
inline FecoWidePlan feco_wide_plan(int F, int k, int D) {
    const int ng = (D + 7) / 8;
    return {ng, (size_t)feco_wide_layout(F, k, ng).total * sizeof(float)};
}

// lanes 0 .. 63 hold 64 consecutive dimensions: the butterfly steps 1 .. 32 (row16_sum_dpp = steps 1, 2, 4, 8)
__device__ __forceinline__ float tree64(float v) {
    v = row16_sum_dpp(v);
    v = v + __shfl_xor(v, 16);
    v = v + __shfl_xor(v, 32);
    return v;
}

template <int NG>
__global__ __launch_bounds__(kWideThreads) void feco_kmeans_wide_kernel(const float* __restrict__ feats, int F, int D, int k, int max_iter,
                                                                        int seeded, uint64_t seed, int64_t index_base,
                                                                        int* __restrict__ assign, float* __restrict__ out,
                                                                        int* __restrict__ counts) {
    constexpr int DS = 8 * NG + 4;  // row stride of the centroid image; columns [0, 8 NG) are stored
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FecoWideLds L = feco_wide_layout(F, k, NG);
    const int kp = (k + 31) & ~31;
    float* cq = lds + L.cq;
    float* hq = lds + L.hq;
    float* mu = lds + L.mu;
    float* part = lds + L.part;
    int* ids = reinterpret_cast<int*>(lds + L.ids);
    int* cnt = reinterpret_cast<int*>(lds + L.cnt);
    int* start = reinterpret_cast<int*>(lds + L.start);
    int* members = reinterpret_cast<int*>(lds + L.members);
    __shared__ int changed;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lh = lane >> 5, ln = lane & 31;
    const size_t slot = blockIdx.x;
    const float* x = feats + slot * F * D;
    for (int i = tid; i < wal4(F); i += kWideThreads) ids[i] = -1;  // the pad entries stay -1: no cluster
    // centring: 16 interleaved partial sums per dimension, added up in order
    for (int e = tid; e < 16 * 128; e += kWideThreads) {
        const int q = e >> 7, d = e & 127;
        float s = 0.f;
        if (d < D) {
#pragma unroll 8
            for (int i = q; i < F; i += 16) s = s + x[(size_t)i * D + d];
        }
        part[e] = s;
    }
    __syncthreads();
    for (int d = tid; d < 128; d += kWideThreads) {
        float t = part[d];
#pragma unroll
        for (int q = 1; q < 16; ++q) t = t + part[q * 128 + d];
        mu[d] = d < D ? t / (float)F : 0.f;
    }
    __syncthreads();
    // element d of centred frame i (pad dimensions are zero)
    auto xc_at = [&](int i, int d) __attribute__((always_inline)) -> float { return d < D ? x[(size_t)i * D + d] - mu[d] : 0.f; };
    if (seeded) {
        // random initialisation: rank the frames by (key, frame); `members` holds the keys, `cnt` the k chosen frames (both
        // are free until the first update)
        unsigned* keys = reinterpret_cast<unsigned*>(members);
        int* chosen = cnt;
        const int64_t utt = index_base + (int64_t)slot;
        for (int i = tid; i < wal4(F); i += kWideThreads)
            keys[i] = i < F ? philox4x32_10_w0(seed, (uint32_t)i, 0u, (uint32_t)utt, (uint32_t)((uint64_t)utt >> 32)) : 0xFFFFFFFFu;
        __syncthreads();
        // rank of frame i = number of (key, frame) pairs below its own; the scan of the keys is shared by `parts` threads per
        // frame (partial ranks meet in `ids`, which is not in use yet)
        const int parts = F >= kWideThreads ? 1 : kWideThreads / F;
        const int nq = wal4(F) / 4, per = (nq + parts - 1) / parts;
        for (int i = tid; i < F; i += kWideThreads) ids[i] = 0;
        __syncthreads();
        for (int t0 = tid; t0 < F * parts; t0 += kWideThreads) {
            const int i = t0 % F, pt = t0 / F;
            const unsigned ki = keys[i];
            int rank = 0;
            const int q0 = pt * per, q1 = min(nq, q0 + per);
            for (int q = q0; q < q1; ++q) {  // a pad key (all ones, index >= F) never counts as smaller
                const uint4 kg = *reinterpret_cast<const uint4*>(keys + 4 * q);
                const int g = 4 * q;
                rank += (kg.x < ki) || (kg.x == ki && g < i);
                rank += (kg.y < ki) || (kg.y == ki && g + 1 < i);
                rank += (kg.z < ki) || (kg.z == ki && g + 2 < i);
                rank += (kg.w < ki) || (kg.w == ki && g + 3 < i);
            }
            if (parts > 1) atomicAdd(&ids[i], rank);
            else ids[i] = rank;
        }
        __syncthreads();
        for (int i = tid; i < F; i += kWideThreads) {
            const int rank = ids[i];
            if (rank < k) chosen[rank] = i;
            ids[i] = -1;
        }
        __syncthreads();
    }
    // A centroid row belongs to one wave: lane l holds dimensions l and l + 64, so the butterfly over the 128 padded lanes is the
    // 64-lane butterfly of either half (steps 1 .. 32) and one addition (step 64).
    auto store_row = [&](int j, float v0, float v1, bool live) __attribute__((always_inline)) {
        cq[j * DS + lane] = v0;
        if (lane + 64 < 8 * NG) cq[j * DS + lane + 64] = v1;
        const float n = tree64(v0 * v0) + tree64(v1 * v1);
        if (lane == 0) hq[j] = live ? -0.5f * n : -INFINITY;  // a pad row of the last tile never wins
    };
    for (int j = wave; j < kp; j += kWideWaves) {
        float v0 = 0.f, v1 = 0.f;
        if (j < k) {
            const int f0 = seeded ? cnt[j] : (int)((long long)j * F / k);
            v0 = xc_at(f0, lane);
            v1 = xc_at(f0, lane + 64);
        }
        store_row(j, v0, v1, j < k);
    }
    __syncthreads();
    const int ntf = (F + 31) >> 5, ntc = kp >> 5;
    for (int it = 0; it < max_iter; ++it) {
        if (tid == 0) changed = 0;
        __syncthreads();
        // ---- assignment on the matrix pipes: A = 32 centroids, B = 32 frames, accumulators from h_j
        for (int ft = wave; ft < ntf; ft += kWideWaves) {
            const int frame = ft * 32 + ln;
            const bool in = frame < F;
            const float* xr = x + (size_t)(in ? frame : 0) * D;
            // B operand: dimensions 8 g + 4 lh .. + 3 of this lane's frame (a column past the utterance is computed and never used)
            float4 xb[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int d0 = 8 * g + 4 * lh;
                xb[g].x = in && d0 < D ? xr[d0] - mu[d0] : 0.f;
                xb[g].y = in && d0 + 1 < D ? xr[d0 + 1] - mu[d0 + 1] : 0.f;
                xb[g].z = in && d0 + 2 < D ? xr[d0 + 2] - mu[d0 + 2] : 0.f;
                xb[g].w = in && d0 + 3 < D ? xr[d0 + 3] - mu[d0 + 3] : 0.f;
            }
            float best = -INFINITY;
            int bj = 4 * lh;
            for (int ct = 0; ct < ntc; ++ct) {
                f32x16 acc;
#pragma unroll
                for (int q = 0; q < 4; ++q) {  // accumulator row (r & 3) + 8 (r >> 2) + 4 lh = centroid of the tile
                    const float4 hv = *reinterpret_cast<const float4*>(hq + ct * 32 + 8 * q + 4 * lh);
                    acc[4 * q] = hv.x;
                    acc[4 * q + 1] = hv.y;
                    acc[4 * q + 2] = hv.z;
                    acc[4 * q + 3] = hv.w;
                }
                const float* arow = cq + (ct * 32 + ln) * DS + 4 * lh;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const float4 a = *reinterpret_cast<const float4*>(arow + 8 * g);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xb[g].x, acc, 0, 0, 0);  // k = 8 g + 0, 8 g + 4
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xb[g].y, acc, 0, 0, 0);  //     8 g + 1, 8 g + 5
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xb[g].z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xb[g].w, acc, 0, 0, 0);
                }
                // the tile's largest score of this lane, then the lowest row that reaches it; tiles ascending, strict >
                float tb = acc[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) tb = fmaxf(tb, acc[r]);
                int rr = 0;
#pragma unroll
                for (int r = 15; r >= 0; --r) rr = acc[r] == tb ? r : rr;
                if (tb > best) {
                    best = tb;
                    bj = ct * 32 + 4 * lh + (rr & 3) + 8 * (rr >> 2);
                }
            }
            {  // the other half of the tile's rows sits in lane ^ 32
                const float ov = __shfl_xor(best, 32);
                const int oj = __shfl_xor(bj, 32);
                if (ov > best || (ov == best && oj < bj)) {
                    best = ov;
                    bj = oj;
                }
            }
            if (lh == 0 && in && ids[frame] != bj) {
                ids[frame] = bj;
                changed = 1;
            }
        }
        __syncthreads();
        if (!changed) break;
        // ---- member lists: frames grouped by cluster, ascending inside a cluster
        for (int j = tid; j < k; j += kWideThreads) cnt[j] = 0;
        __syncthreads();
        for (int i = tid; i < F; i += kWideThreads) atomicAdd(&cnt[ids[i]], 1);
        __syncthreads();
        for (int j = tid; j <= k; j += kWideThreads) {  // offsets: cluster j adds up the counts below it
            int run = 0;
            const int j4 = j & ~3;
            for (int q = 0; q < j4; q += 4) {
                const int4 c = *reinterpret_cast<const int4*>(cnt + q);
                run += c.x + c.y + c.z + c.w;
            }
            for (int q = j4; q < j; ++q) run += cnt[q];
            start[j] = run;
        }
        __syncthreads();
        for (int i = tid; i < F; i += kWideThreads) {  // slots: frame i goes behind the earlier frames of its cluster
            const int j = ids[i];
            int pos = 0;
            const int i4 = i & ~3;
            for (int q = 0; q < i4; q += 4) {
                const int4 v = *reinterpret_cast<const int4*>(ids + q);
                pos += (v.x == j) + (v.y == j) + (v.z == j) + (v.w == j);
            }
            for (int q = i4; q < i; ++q) pos += ids[q] == j;
            members[start[j] + pos] = i;
        }
        __syncthreads();
        // ---- update: a wave per cluster sums the centred frames in ascending frame order; an empty cluster keeps its row
        for (int j = wave; j < k; j += kWideWaves) {
            const int n = cnt[j];
            if (n == 0) continue;  // (the whole wave)
            float s0 = 0.f, s1 = 0.f;
            const int o = start[j];
            for (int m = 0; m < n; m += 4) {  // four members' loads in flight; entries past the cluster are read and not added
                const int i0 = members[o + m], i1 = members[min(o + m + 1, F - 1)], i2 = members[min(o + m + 2, F - 1)],
                          i3 = members[min(o + m + 3, F - 1)];
                const float a0 = xc_at(i0, lane), a1 = xc_at(i1, lane), a2 = xc_at(i2, lane), a3 = xc_at(i3, lane);
                const float b0 = xc_at(i0, lane + 64), b1 = xc_at(i1, lane + 64), b2 = xc_at(i2, lane + 64), b3 = xc_at(i3, lane + 64);
                s0 = s0 + a0;
                s1 = s1 + b0;
                if (m + 1 < n) { s0 = s0 + a1; s1 = s1 + b1; }
                if (m + 2 < n) { s0 = s0 + a2; s1 = s1 + b2; }
                if (m + 3 < n) { s0 = s0 + a3; s1 = s1 + b3; }
            }
            store_row(j, s0 / (float)n, s1 / (float)n, true);
        }
        __syncthreads();
    }
    // cnt / start / members describe the final ids in both exits: "nothing changed" leaves the previous iteration's lists
    // valid, the max_iter exit has just rebuilt them.  (max_iter >= 1 and ids start at -1: the lists exist.)
    float* o = out + slot * k * D;
    for (int e = tid; e < k * D; e += kWideThreads) {
        const int j = e / D, d = e - j * D;
        const int n = cnt[j];
        float v;
        if (n > 0) {
            float sum = 0.f;
            const int s0 = start[j];
            for (int m = 0; m < n; m += 4) {
                const int i0 = members[s0 + m], i1 = members[min(s0 + m + 1, F - 1)], i2 = members[min(s0 + m + 2, F - 1)],
                          i3 = members[min(s0 + m + 3, F - 1)];
                const float v0 = x[(size_t)i0 * D + d], v1 = x[(size_t)i1 * D + d], v2 = x[(size_t)i2 * D + d], v3 = x[(size_t)i3 * D + d];
                sum = sum + v0;
                if (m + 1 < n) sum = sum + v1;
                if (m + 2 < n) sum = sum + v2;
                if (m + 3 < n) sum = sum + v3;
            }
            v = sum / (float)n;
        } else {
            v = x[(size_t)j * D + d];  // feature_level.py:213-214 `force` fallback
        }
        o[e] = v;
    }
    for (int j = tid; j < k; j += kWideThreads) counts[slot * k + j] = cnt[j];
    for (int i = tid; i < F; i += kWideThreads) assign[slot * F + i] = ids[i];
}

template <int NG>
hipError_t launch_wide(const float* feats, int B, int F, int D, int k, int max_iter, int seeded, uint64_t seed, int64_t index_base,
                       int* assign, float* out, int* counts, size_t lds, hipStream_t s) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(feco_kmeans_wide_kernel<NG>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWideLdsMax);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(feco_kmeans_wide_kernel<NG>, dim3(B), dim3(kWideThreads), lds, s, feats, F, D, k, max_iter, seeded, seed,
                       index_base, assign, out, counts);
    return hipGetLastError();
}

}  // namespace

extern "C" int sg_feco_kmeans_compress_wide(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                            int32_t max_iter, int32_t random_init, uint64_t seed, int64_t index_base,
                                            int32_t* assign_dev, float* out_dev, int32_t* counts_dev, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (!feats_dev || !assign_dev || !out_dev || !counts_dev || B <= 0 || F <= 0 || D < kWideMinD || D > kWideMaxD || k <= 0 || k > F ||
        max_iter <= 0)
        return fail(ctx, SG_ERR_ARG, "sg_feco_kmeans_compress_wide: need feats, assign, out and counts, B > 0, 0 < k <= F, %d <= D <= %d, "
                         "max_iter > 0", kWideMinD, kWideMaxD);
    const FecoWidePlan plan = feco_wide_plan(F, k, D);
    if (plan.lds > kWideLdsMax)
        return fail(ctx, SG_ERR_ARG, "sg_feco_kmeans_compress_wide: %d clusters x %d dims + %d frames need %zu bytes of LDS (limit %zu): "
                         "utterance too long for one block", k, D, F, plan.lds, kWideLdsMax);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_kmeans_compress_wide: hipSetDevice failed");
    hipError_t e = hipErrorInvalidValue;
    const int seeded = random_init != 0;
    hipStream_t s = (hipStream_t)stream;
#define SG_WIDE_CASE(n) \
    case n: e = launch_wide<n>(feats_dev, B, F, D, k, max_iter, seeded, seed, index_base, assign_dev, out_dev, counts_dev, plan.lds, s); break;
    switch (plan.ng) {
        SG_WIDE_CASE(9) SG_WIDE_CASE(10) SG_WIDE_CASE(11) SG_WIDE_CASE(12) SG_WIDE_CASE(13) SG_WIDE_CASE(14) SG_WIDE_CASE(15) SG_WIDE_CASE(16)
    }
#undef SG_WIDE_CASE
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_kmeans_compress_wide: %s", hipGetErrorString(e));
    return SG_OK;
}
