// FeCo feature-level defense: per-utterance k-means over the frames of a feature
// matrix, then every cluster replaced by the mean of its frames (reference defense/feature_level.py:168-217),
// forward and backward.
//
// The reference calls a third-party k-means with a RANDOM initialisation (libKMCUDA / kmeans_pytorch), so its
// cluster ids are not reproducible even between two runs of the reference.  The clustering here follows its own
// DETERMINISM CONTRACT (version 2, round 5: the assignment is a contraction on the matrix pipes; restated in
// oracle/feco.py + oracle/conv_chain.c sg_feco_scores, checked bit for bit):
//   * centring (k-means is translation invariant; it keeps the cancellation of the expanded distance small):
//     mu[d] = (p_0 + p_1 + ... + p_15 in that order) / F with p_q = sum over frames i = q, q + 16, ... ascending (fp32, from
//     0.f); x'[i][d] = x[i][d] - mu[d].  Everything below works on x'.
//   * k = int(F * ratio) centroids, centroid j initialised to frame floor(j * F / k) -- or, for the SEEDED form
//     (sg_feco_kmeans_seeded: what makes expectation-over-transformation against this defense meaningful, like
//     the reference's randomly initialised k-means), to the frame of rank j when the frames are ordered by
//     (Philox4x32-10(counter = (frame, 0, utterance lo, utterance hi), key = seed) word 0, frame) ascending:
//     k distinct frames, a uniformly random subset in random order, a function of (seed, GLOBAL utterance index)
//     only (oracle/philox.py feco_random_init);
//   * assignment: frame i goes to the centroid with the LARGEST score(i, j) = x'_i . c_j - |c_j|^2 / 2 (= the nearest one),
//     ties to the lowest index.  The score is ONE fp32 fmaf chain: it starts at h_j = -0.5f * n_j and adds
//     fmaf(c_j[d], x'_i[d], .) over d in the contraction kernels' order (groups of 8 ascending, inside a group 0, 4, 1, 5,
//     2, 6, 3, 7; dimensions padded with zeros to DPAD = 32 or 64) -- what v_mfma_f32_32x32x2_f32 computes
//     (tools/native/mfma_order.hip); n_j = the sum of the squares c_j[d]^2 (each rounded) over the DPAD padded
//     dimensions by the butterfly s[d] += s[d ^ 1], s[d ^ 2], ... s[d ^ DPAD/2] (every step all d at once);
//   * stop when no assignment changed or after max_iter assignment steps; otherwise update: centroid j = (sum of its
//     frames x' in ascending frame order, fp32, from 0.f) / count, an empty cluster keeps its centroid;
//   * the ids of the LAST assignment step are the result.
// The reference's second distance, other_param 'cos' (:174-182, kmeans_pytorch pairwise_cosine), has a contract of its own --
// "cosine", next to version 2 (sg_feco_kmeans_compress_metric with SG_FECO_COS; restated in tests/feco_cos_restate.py on
// oracle/conv_chain.c sg_feco_scores with h = 0).  Everything fp32, fp contract off:
//   * NO centring: the cosine distance is not translation invariant, the frames are used as they are (pad dimensions zero);
//   * initial centroids m_j: the frames version 2 starts from, even or seeded form, same keys;
//   * a centroid row is stored normalised: n_j = the butterfly sum of the rounded squares m_j[d]^2 over the DPAD lanes (the
//     tree of n_j above), r_j = sqrtf(n_j) correctly rounded, c_j[d] = m_j[d] / r_j (IEEE division) if n_j > 0, else
//     c_j = 0 -- the reference would divide by zero there; here a zero centroid scores 0 and nothing is ever NaN;
//   * assignment: the LARGEST score(i, j) = x_i . c_j wins, ties to the lowest index: ONE fmaf chain from 0.f in the order
//     of version 2.  |x_i| does not change the arg-max and is not computed;
//   * stop as above; update: m_j = (sum of the cluster's frames in ascending frame order, from 0.f) / count, then
//     normalised as above; an empty cluster keeps its c_j bit for bit (it is not normalised again);
//   * the ids of the LAST assignment step are the result.
// Given the ids, the compression is the reference's :204-216 on the ORIGINAL frames: mean of the cluster's frames, an
// empty cluster i falls back to frame i when `force` (batch > 1) and is dropped otherwise (the host compacts).
#include <cstdio>
#include <cstdlib>

#include "sg_internal.h"
#include "philox.h"
#include "wave_reduce.h"

#pragma clang fp contract(off)

using namespace sg;

namespace {

// tuning aid (SG_FECO_TRACE=1): phase timestamps (100 MHz) of block (0, 0): per iteration [start, after the assignment,
// after the member lists, after the update] for the first 16 iterations, then [loop end, kernel end, kernel start]
constexpr int kFecoTraceIters = 16;
// (ONE device object: hipcc places separate device globals of a file in an order that is not stable from one build to the
// next -- the same source gave two different code objects, equal but for the addresses of these two)
struct FecoTraceDev {
    unsigned long long t[4 * kFecoTraceIters + 4 + 24];  // + detail stamps (set-up, iteration 0) + cycle counts
    int on;
};
__device__ FecoTraceDev g_feco_tr;
#ifdef SG_EXP_FECO_JC
__device__ int g_feco_ablate;  // experiment builds only (never the shipped library): 1 no MFMAs, 2 no per-tile maxima, 4 no B operand loads
#endif
#define FECO_STAMP(i) \
    if (g_feco_tr.on && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) g_feco_tr.t[i] = __builtin_amdgcn_s_memrealtime();
#define FECO_DETAIL(i) FECO_STAMP(4 * kFecoTraceIters + 4 + (i))
#define FECO_CYCLES(i) \
    if (g_feco_tr.on && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) g_feco_tr.t[4 * kFecoTraceIters + 4 + (i)] = __builtin_readcyclecounter();

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr unsigned long long kFecoPairWait = 2000;  // 20 us of the 100 MHz clock

// float offset of 16-byte slot `slot` of row `row` in a [rows][DPAD] image: the 16 lanes one ds_read_b128 cycle serves
// (MI355X_MICROARCH.md, LDS: rows {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of a 32-row tile) hit 16 different slots
template <int DPAD>
__device__ __forceinline__ int sw_slot(int row, int slot) {
    const int key = DPAD == 32 ? ((row >> 1) & 7) : (row & 15);
    return row * DPAD + ((slot ^ key) << 2);
}
template <int DPAD>
__device__ __forceinline__ int sw_at(int row, int d) { return sw_slot<DPAD>(row, d >> 2) + (d & 3); }

// The contract's butterfly over the DPAD lanes that hold a centroid row (s[d] += s[d ^ 1], s[d ^ 2], ...): what lane d = 0 ends
// up with is the balanced pairwise tree over the row.  Steps 1 and 2 are quad permutes; after them a quad holds one value,
// so mirroring the 8 lanes of a half row (then the 16 of a row) pairs exactly the quads the steps 4 and 8 pair -- four DPP
// adds instead of four trips through the LDS crossbar; steps 16 (and 32) go through ds_bpermute.
template <int DPAD>
__device__ __forceinline__ float row_tree_sum(float v) {
    v = row16_sum_dpp(v);
    v = v + __shfl_xor(v, 16);
    if (DPAD == 64) v = v + __shfl_xor(v, 32);
    return v;
}

// The k-means kernel, once per metric (k_feco_kmeans.h): feco_kmeans_kernel<DPAD>, the L2 contract, and
// feco_kmeans_cos_kernel<DPAD>, the cosine one
#define FECO_KMEANS_KERNEL feco_kmeans_kernel
#define FECO_KMEANS_COS false
#include "k_feco_kmeans.h"
#undef FECO_KMEANS_KERNEL
#undef FECO_KMEANS_COS
#define FECO_KMEANS_KERNEL feco_kmeans_cos_kernel
#define FECO_KMEANS_COS true
#include "k_feco_kmeans.h"
#undef FECO_KMEANS_KERNEL
#undef FECO_KMEANS_COS

// out[b][j][d] = mean over frames with id j (ascending order) or, for an empty cluster, feats[b][j][d]
__global__ void feco_compress_kernel(const float* __restrict__ feats, const int* __restrict__ assign, int F, int D, int k,
                                     float* __restrict__ out, int* __restrict__ counts) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= k * D) return;
    const int j = e / D, d = e - j * D;
    const float* x = feats + (size_t)b * F * D;
    const int* ids = assign + (size_t)b * F;
    float sum = 0.f;
    int cnt = 0;
    for (int i = 0; i < F; ++i)
        if (ids[i] == j) {
            sum = sum + x[(size_t)i * D + d];
            ++cnt;
        }
    out[((size_t)b * k + j) * D + d] = cnt > 0 ? sum / (float)cnt : x[(size_t)j * D + d];
    if (d == 0) counts[(size_t)b * k + j] = cnt;
}

// dfeats[b][i][d] = dout[b][id_i][d] / count[id_i]  (+ dout[b][i][d] if cluster i is empty and force)
__global__ void feco_compress_bwd_kernel(const float* __restrict__ dout, const int* __restrict__ assign,
                                         const int* __restrict__ counts, int F, int D, int k, int force,
                                         float* __restrict__ dfeats) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= F * D) return;
    const int i = e / D, d = e - i * D;
    const int j = assign[(size_t)b * F + i];
    float g = dout[((size_t)b * k + j) * D + d] / (float)counts[(size_t)b * k + j];
    if (force && i < k && counts[(size_t)b * k + i] == 0) g = g + dout[((size_t)b * k + i) * D + d];
    dfeats[((size_t)b * F + i) * D + d] = g;
}

// The same for R repeats of the clustering of the SAME features (EOT over the defense): the compression is linear, so
// the repeats' gradients wrt the features are summed right here, in repeat order -- one log-mel / MFCC adjoint
// serves all of them.  dout (R, B, k, D), assign (R, B, F), counts (R, B, k) -> dfeats (B, F, D).
__global__ void feco_compress_bwd_reps_kernel(const float* __restrict__ dout, const int* __restrict__ assign,
                                              const int* __restrict__ counts, int B, int F, int D, int k, int force, int R,
                                              const float* carry, float* dfeats) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= F * D) return;
    const int i = e / D, d = e - i * D;
    // carry: the sum over the repeats of earlier passes of the same step (may alias dfeats: one thread per element)
    float acc = carry ? carry[((size_t)b * F + i) * D + d] : 0.f;
    for (int r = 0; r < R; ++r) {
        const size_t u = (size_t)r * B + b;
        const int j = assign[u * F + i];
        float g = dout[(u * k + j) * D + d] / (float)counts[u * k + j];
        if (force && i < k && counts[u * k + i] == 0) g = g + dout[(u * k + i) * D + d];
        acc = r == 0 && !carry ? g : acc + g;
    }
    dfeats[((size_t)b * F + i) * D + d] = acc;
}

}  // namespace

int sg::feco_kmeans_check(sg_ctx* ctx, int B, int F, int D, int k, int max_iter, int reps) {
    if (B <= 0 || F <= 0 || D <= 0 || D > kFecoMaxD || k <= 0 || k > F || max_iter <= 0 || reps < 1 || reps > 65535)
        return fail(ctx, SG_ERR_ARG, "sg_feco_kmeans: need 0 < k <= F, 0 < D <= %d, max_iter > 0", kFecoMaxD);
    const size_t least = (size_t)feco_layout(F, k, D <= 32 ? 32 : 64, 1, 0, 0).total * sizeof(float);  // one chunk, no extras
    if (least > kFecoLdsMax)
        return fail(ctx, SG_ERR_ARG, "sg_feco_kmeans: %d clusters x %d dims + %d frames need %zu bytes of LDS (limit %zu): "
                         "utterance too long for one block", k, D, F, least, kFecoLdsMax);
    return SG_OK;
}

// the most instances a context's device can pair, and the exchange words they need
static size_t feco_pair_instances(const sg_ctx* ctx) { return (size_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) / 2; }
static size_t feco_xchg_words(const sg_ctx* ctx) { return feco_pair_instances(ctx) * 2 * 2 * kFecoMergeCap; }

bool sg::feco_pair_buffers(sg_ctx* ctx) {
    if (ctx->feco_xchg) return true;
    if (ctx->feco_two_cu == 0) return false;
    const size_t inst_max = feco_pair_instances(ctx), words = feco_xchg_words(ctx);
    void *px = nullptr, *pf = nullptr;
    if (hipMalloc(&px, words * sizeof(unsigned long long)) == hipSuccess && hipMalloc(&pf, inst_max * 2 * sizeof(unsigned)) == hipSuccess &&
        hipMemset(pf, 0, inst_max * 2 * sizeof(unsigned)) == hipSuccess &&
        hipDeviceSynchronize() == hipSuccess) {  // (a null-stream fill, read by launches on the caller's stream: awaited, once)
        ctx->feco_xchg = static_cast<unsigned long long*>(px);
        ctx->feco_flags = static_cast<unsigned*>(pf);
        ctx->model_allocs.push_back(px);
        ctx->model_allocs.push_back(pf);
        ctx->feco_epoch = 0;
        return true;
    }
    if (px) (void)hipFree(px);  // no room: one block per instance
    if (pf) (void)hipFree(pf);
    (void)hipGetLastError();
    return false;
}

// The pair state of one launch of a paired plan: the exchange buffers, this launch's id and tag base, the wipe when the tags
// start over, the fault-injection budget
static int feco_pair_begin(sg_ctx* ctx, hipStream_t s, FecoPair& pr) {
    const unsigned launch = ++ctx->feco_epoch;  // (0 is what a fresh flag word holds: never a launch id)
    if (launch == 0) ctx->feco_epoch = 1;
    // tags repeat every 2^15 launches: the words of the last cycle are wiped before they could be taken for new ones
    if ((ctx->feco_epoch & 0x7FFFu) == 1u && hipMemsetAsync(ctx->feco_xchg, 0, feco_xchg_words(ctx) * sizeof(unsigned long long), s) != hipSuccess)
        return fail(ctx, SG_ERR_HIP, "sg_feco_kmeans: hipMemsetAsync failed");
    pr.on = 1;
    pr.xchg = ctx->feco_xchg;
    pr.flags = ctx->feco_flags;
    pr.launch = ctx->feco_epoch;
    pr.tag0 = (ctx->feco_epoch & 0x7FFFu) << 6;
    if (ctx->lose_feco > 0) {  // test hook (sg_debug_lose_handoffs): this launch's second halves publish nothing
        pr.drop = 1;
        --ctx->lose_feco;
    }
    return SG_OK;
}

static FecoKnobs feco_knobs(const sg_ctx* ctx) {
    FecoKnobs knobs;
    knobs.two_cu = ctx->feco_two_cu;
#ifdef SG_EXP_FECO_JC
    if (const char* ev = sg_tune_env("SG_FECO_ABLATE")) { const int a = atoi(ev); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_feco_ablate), &a, sizeof(a)); }
    if (const char* ev = sg_tune_env("SG_FECO_JC")) knobs.jc = atoi(ev) < 1 ? 1 : atoi(ev);
#endif
    return knobs;
}

// tuning aid (SG_FECO_TRACE=1): arms the device switch on the first launch, reads back and prints the phases of every later one
static void feco_trace_report(int max_iter, hipStream_t s) {
    static const bool tr_on = sg_tune_env("SG_FECO_TRACE") != nullptr;
    if (!tr_on) return;
    static bool armed[kMaxDevices] = {};  // the switch is a device symbol: one per device
    const int dslot = sg_device_slot();
    if (!armed[dslot]) {
        const int one = 1;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_feco_tr), &one, sizeof(one), offsetof(FecoTraceDev, on));
        armed[dslot] = true;
        return;
    }
    unsigned long long h[4 * kFecoTraceIters + 4 + 24];
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpyFromSymbol(h, HIP_SYMBOL(g_feco_tr), sizeof(h), offsetof(FecoTraceDev, t)) != hipSuccess)
        return;
    fprintf(stderr, "feco k-means phases (us), block (0, 0): set-up %.2f;", (h[0] - h[4 * kFecoTraceIters + 2]) * 0.01);
    for (int it = 0; it < max_iter && it < kFecoTraceIters && h[4 * it + 1] > h[4 * it]; ++it)
        fprintf(stderr, " it%d assign %.2f lists %.2f update %.2f;", it, (h[4 * it + 1] - h[4 * it]) * 0.01,
                h[4 * it + 2] > h[4 * it + 1] ? (h[4 * it + 2] - h[4 * it + 1]) * 0.01 : 0.0,
                h[4 * it + 3] > h[4 * it + 2] ? (h[4 * it + 3] - h[4 * it + 2]) * 0.01 : 0.0);
    const unsigned long long* dt = h + 4 * kFecoTraceIters + 4;
    fprintf(stderr, " [set-up: centring %.2f staging %.2f seeding %.2f init %.2f; it0: units %.2f merge %.2f | rank+count %.2f sizes+scan %.2f "
            "slots %.2f zero %.2f; shader clock %.0f MHz]", (dt[0] - h[4 * kFecoTraceIters + 2]) * 0.01, (dt[1] - dt[0]) * 0.01,
            (dt[2] - dt[1]) * 0.01, (h[0] - dt[2]) * 0.01, (dt[3] - h[0]) * 0.01, (h[1] - dt[3]) * 0.01, (dt[4] - h[1]) * 0.01,
            (dt[5] - dt[4]) * 0.01, (dt[6] - dt[5]) * 0.01, (h[2] - dt[6]) * 0.01,
            (double)(dt[21] - dt[20]) / ((h[4 * kFecoTraceIters] - dt[0]) * 0.01));
    fprintf(stderr, " out %.2f; loop + out total %.2f\n", (h[4 * kFecoTraceIters + 1] - h[4 * kFecoTraceIters]) * 0.01, (h[4 * kFecoTraceIters + 1] - h[0]) * 0.01);
}

// the four instantiations share one signature: [metric][dpad == 64]
using FecoKernel = void (*)(const float*, int, int, int, int, int, int, uint64_t, int64_t, int, int, int, FecoSched, FecoPair, int*, float*, int*);
static const FecoKernel kFecoKernels[2][2] = {{feco_kmeans_kernel<32>, feco_kmeans_kernel<64>},
                                              {feco_kmeans_cos_kernel<32>, feco_kmeans_cos_kernel<64>}};
static_assert(SG_FECO_L2 == 0 && SG_FECO_COS == 1, "kFecoKernels is indexed by the metric");

// What an entry point asks for beyond the shape.  `entry` is the name its refusals carry; out and counts (the means and sizes
// of the clusters) are required of the compress entries
struct FecoCall {
    const char* entry;
    int metric, seeded, row_wise;
    uint64_t seed;
    int64_t index_base;
    int reps;
    int32_t* assign;
    float* out;
    int32_t* counts;
    bool compress;
};

static int feco_kmeans_impl(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k, int32_t max_iter,
                            const FecoCall& c, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (c.metric != SG_FECO_L2 && c.metric != SG_FECO_COS) return fail(ctx, SG_ERR_ARG, "%s: metric must be SG_FECO_L2 or SG_FECO_COS", c.entry);
    if (c.row_wise != 0 && c.row_wise != 1) return fail(ctx, SG_ERR_ARG, "%s: row_wise must be 0 or 1", c.entry);
    // the L2 metric of sg_feco_kmeans_compress_metric is the entries that exist, refusals and bits included
    const char* who = !c.compress || c.metric == SG_FECO_COS ? c.entry : c.row_wise ? "sg_feco_kmeans_compress_rows" : "sg_feco_kmeans_compress";
    if (c.compress && (!c.out || !c.counts)) return fail(ctx, SG_ERR_ARG, "%s: out and counts are required", who);
    if (c.compress && !c.row_wise && c.reps > 1 && !c.seeded)
        return fail(ctx, SG_ERR_ARG, "%s: repeats of the evenly started clustering coincide (reps must be 1)", who);
    if (!feats_dev || !c.assign) return fail(ctx, SG_ERR_ARG, "sg_feco_kmeans: need 0 < k <= F, 0 < D <= %d, max_iter > 0", kFecoMaxD);
    if (int rc = feco_kmeans_check(ctx, B, F, D, k, max_iter, c.reps)) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_kmeans: hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const FecoKnobs knobs = feco_knobs(ctx);
    FecoPlan plan = feco_plan(F, D, k, max_iter, (long)B * c.reps, ctx->num_cus, true, knobs);
    if (plan.pair && !feco_pair_buffers(ctx)) plan = feco_plan(F, D, k, max_iter, (long)B * c.reps, ctx->num_cus, false, knobs);
    FecoPair pr{};
    pr.owner = plan.owner;
    pr.sched1 = plan.sched1;
    if (plan.pair)
        if (int rc = feco_pair_begin(ctx, s, pr)) return rc;
    const FecoKernel fn = kFecoKernels[c.metric][plan.dpad == 64];
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFecoLdsMax);
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_kmeans: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(fn, dim3(B, c.reps, plan.pair ? 2 : 1), dim3(kFecoThreads), plan.lds, s, feats_dev, F, D, k, max_iter, c.seeded, c.row_wise,
                       c.seed, c.index_base, plan.x_in_lds, plan.fast_lists, plan.JC, plan.sched0, pr, c.assign, c.out, c.counts);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_kmeans: %s", hipGetErrorString(e));
    feco_trace_report(max_iter, s);
    return SG_OK;
}

extern "C" int sg_feco_set_two_cu(sg_ctx* ctx, int32_t mode) {
    if (!ctx || mode < -1 || mode > 0) return SG_ERR_ARG;
    ctx->feco_two_cu = mode;
    return SG_OK;
}

extern "C" int sg_feco_kmeans(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                              int32_t max_iter, int32_t* assign_dev, void* stream) {
    const FecoCall c{"sg_feco_kmeans", SG_FECO_L2, 0, 0, 0, 0, 1, assign_dev, nullptr, nullptr, false};
    return feco_kmeans_impl(ctx, feats_dev, B, F, D, k, max_iter, c, stream);
}

extern "C" int sg_feco_kmeans_seeded(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                     int32_t max_iter, uint64_t seed, int64_t index_base, int32_t* assign_dev, void* stream) {
    const FecoCall c{"sg_feco_kmeans_seeded", SG_FECO_L2, 1, 0, seed, index_base, 1, assign_dev, nullptr, nullptr, false};
    return feco_kmeans_impl(ctx, feats_dev, B, F, D, k, max_iter, c, stream);
}

extern "C" int sg_feco_kmeans_compress(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                       int32_t max_iter, int32_t random_init, uint64_t seed, int64_t index_base, int32_t reps,
                                       int32_t* assign_dev, float* out_dev, int32_t* counts_dev, void* stream) {
    const FecoCall c{"sg_feco_kmeans_compress", SG_FECO_L2, random_init != 0, 0, seed, index_base, reps, assign_dev, out_dev, counts_dev, true};
    return feco_kmeans_impl(ctx, feats_dev, B, F, D, k, max_iter, c, stream);
}

extern "C" int sg_feco_kmeans_compress_rows(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                            int32_t max_iter, int32_t random_init, uint64_t seed, int64_t index_base, int32_t reps,
                                            int32_t* assign_dev, float* out_dev, int32_t* counts_dev, void* stream) {
    const FecoCall c{"sg_feco_kmeans_compress_rows", SG_FECO_L2, random_init != 0, 1, seed, index_base, reps, assign_dev, out_dev, counts_dev, true};
    return feco_kmeans_impl(ctx, feats_dev, B, F, D, k, max_iter, c, stream);
}

extern "C" int sg_feco_kmeans_compress_metric(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                              int32_t max_iter, int32_t metric, int32_t random_init, uint64_t seed, int64_t index_base,
                                              int32_t reps, int32_t row_wise, int32_t* assign_dev, float* out_dev, int32_t* counts_dev,
                                              void* stream) {
    const FecoCall c{"sg_feco_kmeans_compress_metric", metric, random_init != 0, row_wise, seed, index_base, reps, assign_dev, out_dev, counts_dev, true};
    return feco_kmeans_impl(ctx, feats_dev, B, F, D, k, max_iter, c, stream);
}

extern "C" int sg_feco_compress(sg_ctx* ctx, const float* feats_dev, const int32_t* assign_dev, int32_t B, int32_t F,
                                int32_t D, int32_t k, float* out_dev, int32_t* counts_dev, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (!feats_dev || !assign_dev || !out_dev || !counts_dev || B <= 0 || F <= 0 || D <= 0 || k <= 0 || k > F)
        return fail(ctx, SG_ERR_ARG, "sg_feco_compress: bad arguments");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_compress: hipSetDevice failed");
    hipLaunchKernelGGL(feco_compress_kernel, dim3((k * D + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, feats_dev,
                       assign_dev, F, D, k, out_dev, counts_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_compress: %s", hipGetErrorString(e));
    return SG_OK;
}

extern "C" int sg_feco_compress_backward(sg_ctx* ctx, const float* dout_dev, const int32_t* assign_dev,
                                         const int32_t* counts_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                         int32_t force, float* dfeats_dev, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (!dout_dev || !assign_dev || !counts_dev || !dfeats_dev || B <= 0 || F <= 0 || D <= 0 || k <= 0 || k > F)
        return fail(ctx, SG_ERR_ARG, "sg_feco_compress_backward: bad arguments");
    if (hipSetDevice(ctx->device) != hipSuccess)
        return fail(ctx, SG_ERR_HIP, "sg_feco_compress_backward: hipSetDevice failed");
    hipLaunchKernelGGL(feco_compress_bwd_kernel, dim3((F * D + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, dout_dev,
                       assign_dev, counts_dev, F, D, k, force, dfeats_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_compress_backward: %s", hipGetErrorString(e));
    return SG_OK;
}

extern "C" int sg_feco_compress_backward_reps(sg_ctx* ctx, const float* dout_dev, const int32_t* assign_dev,
                                              const int32_t* counts_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                              int32_t force, int32_t reps, float* dfeats_dev, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (!dout_dev || !assign_dev || !counts_dev || !dfeats_dev || B <= 0 || F <= 0 || D <= 0 || k <= 0 || k > F || reps < 1)
        return fail(ctx, SG_ERR_ARG, "sg_feco_compress_backward_reps: bad arguments");
    if (hipSetDevice(ctx->device) != hipSuccess)
        return fail(ctx, SG_ERR_HIP, "sg_feco_compress_backward_reps: hipSetDevice failed");
    const hipError_t e = launch_feco_bwd_reps(dout_dev, assign_dev, counts_dev, B, F, D, k, force, reps, nullptr, dfeats_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, SG_ERR_HIP, "sg_feco_compress_backward_reps: %s", hipGetErrorString(e));
    return SG_OK;
}

hipError_t sg::launch_feco_bwd_reps(const float* dout, const int* assign, const int* counts, int B, int F, int D, int k, int force,
                                    int R, const float* carry, float* dfeats, hipStream_t s) {
    hipLaunchKernelGGL(feco_compress_bwd_reps_kernel, dim3((F * D + 255) / 256, B), dim3(256), 0, s, dout, assign, counts, B, F, D, k,
                       force, R, carry, dfeats);
    return hipGetLastError();
}
