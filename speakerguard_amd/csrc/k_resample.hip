// The down-/up-sampling input defense (reference defense/frequency_domain.py DS :8-31), both directions, on (B,T) float32
// waveforms, one utterance per row:  y = Trunc(Up(Down(x))),  gx = Down^T(Up^T(pad(g))).  Each of the two resamplers is
// Kaldi's LinearResample as torchaudio 0.6.0 ports it: a polyphase FIR whose per-phase windows (`first`) and weights are
// built by the CALLER (defense/frequency_domain.py ds_tables, float32 operations in torchaudio's order) and handed over
// in the spec.  One launch per direction for the whole composite: a block owns a tile of one row's result, stages the
// source tile plus halo and the tables in LDS, writes the low-rate intermediate to LDS only, and produces its results from
// LDS.  The grid is tiles x B.  Global loads and stores are coalesced and 16 bytes wide wherever a chunk of four samples sits on
// a 16-byte boundary of the row's memory (any T, any row: only a row's first and last chunk can fall back to single samples).
//
// A stage (in_unit, out_unit, W, first[out_unit], weight[out_unit][W]) maps n_in samples to n_out = ceil(n_in out_unit /
// in_unit):  output m = u out_unit + p  is  sum_j weight[p][j] in[first[p] + u in_unit + j],  `in` zero outside [0, n_in).
//
// Determinism contract: every value is ONE float32 fmaf chain started from +0 -- it depends neither on B, nor on
// the tile, nor on where the row sits in the call.  tests/ds_restate.py restates the chains in numpy.
//   forward   acc = 0; for j = 0 .. W-1 (ascending tap): acc = fmaf(weight[p][j], in[first[p] + u in_unit + j], acc).
//   backward  the gather form, no atomics: input sample i = v in_unit + r collects, in ASCENDING OUTPUT INDEX m, every pair
//             (m, j) with first[p] + u in_unit + j = i and 0 <= j < W:  acc = fmaf(weight[p][j], g[m], acc).  The pairs of a
//             residue r are a host-built list (toff = m - v out_unit, weight), sorted by toff: no division in the loop.
//   Zero-padded terms: ALL of them enter, everywhere, as exact zeros -- taps that fall outside [0, n_in) forward, outputs
//             outside [0, n_out) and the truncated tail [n_final, n_up) backward, zero weights included.  A chain that starts
//             at +0 is left unchanged, bit for bit, by a term whose factor is an exact zero as long as the other factor is
//             finite (weights are refused otherwise), so a restatement that skips these terms computes the same bits.
//   The low-rate intermediate is zero outside [0, n_low) in both directions (the second stage's own zero padding).
//
// Table bound: out_unit * W <= 2048 and in_unit, out_unit <= 1024 per stage.  With that both stages' tables (backward: the
// sorted lists, two words per pair, plus a start index per residue) take at most 48 KB; a tile of 2048 samples (rounded
// down to whole units), its low-rate intermediate and its source tile take ~13 KB at param = 0.5.  A spec whose tables
// and tile do not fit the 64 KB a block gets without opting in is refused (SG_ERR_ARG), never cut differently.
#include <cmath>
#include <cstring>

#include "sg_internal.h"

#pragma clang fp contract(off)

using namespace sg;

namespace {

constexpr int kRsThreads = 512;
constexpr int kRsTile = 2048;           // samples of the result a block owns (whole units: kRsTile / unit, at least one)
constexpr int kRsMaxTable = 2048;       // out_unit * W of a stage
constexpr int kRsMaxUnit = 1024;
constexpr int kRsMaxFirst = 1 << 20;    // |first[p]|
constexpr int kRsMaxLen = 1 << 30;      // every length of the composite: all sample indices stay in int
constexpr size_t kRsLdsBytes = 64 * 1024;
constexpr size_t kRsCacheMax = 32;

struct RsStageGeo {
    int iu, ou, W, E;          // E = ou * W pairs
    int minfirst, span;        // forward: a unit's outputs read source [u iu + minfirst, + span)
    int dumin, dumax;          // backward: pair (p, j) belongs to source unit u + du, du = floor((first[p] + j) / iu)
    int o_first, o_w;          // word offsets in the blob: forward tables
    int o_tstart, o_toff, o_tw;  // ... backward lists: pairs of residue r at [tstart[r], tstart[r + 1])
};
struct RsGeo {
    RsStageGeo d, u;           // Down: x -> low, Up: low -> y
    int fwd_words, bwd_off, bwd_words;  // the two halves of the blob (multiples of 4 words)
    int UT, VT;                // units per tile: forward in Up's output units, backward in Down's input units
    int f_in_max, f_low_max;   // LDS floats of the forward's source tile (later: the tile's results) / intermediate
    int b_g_max, b_low_max;    // ... of the backward's cotangent tile (likewise) / intermediate
};

__host__ __device__ inline int rs_floordiv(int a, int b) {
    const int q = a / b;
    return (a % b != 0 && (a < 0)) ? q - 1 : q;
}

__device__ __forceinline__ void rs_copy_words(int32_t* dst, const int32_t* src, int words) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (int k = threadIdx.x; k < words / 4; k += kRsThreads) d4[k] = s4[k];
}

// row[i0 .. i0 + cnt) -> dst, zero outside [0, n): chunks of four samples on the 16-byte boundaries of the row's memory, one
// 16-byte load where a chunk lies inside both ranges, sample by sample at the edges
__device__ __forceinline__ void rs_stage_row(float* dst, const float* __restrict__ row, int i0, int cnt, int n) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);  // row[a] is 16-byte aligned where (a + mis) % 4 == 0
    const int a0 = i0 - ((i0 + mis) & 3), i1 = i0 + cnt;
    const int chunks = (i1 - a0 + 3) >> 2;
    for (int c = threadIdx.x; c < chunks; c += kRsThreads) {
        const int a = a0 + 4 * c;
        if (a >= i0 && a + 4 <= i1 && a >= 0 && a + 4 <= n) {
            const float4 v = *reinterpret_cast<const float4*>(row + a);
            float* d = dst + (a - i0);
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
            for (int e = 0; e < 4; ++e) {
                const int i = a + e;
                if (i >= i0 && i < i1) dst[i - i0] = (i >= 0 && i < n) ? row[i] : 0.f;
            }
        }
    }
}

// src = result[m0 .. m0 + cnt) -> row, samples below n only (m0 >= 0): the same chunks, 16-byte stores
__device__ __forceinline__ void rs_store_row(float* __restrict__ row, const float* src, int m0, int cnt, int n) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
    const int a0 = m0 - ((m0 + mis) & 3), m1 = min(m0 + cnt, n);
    const int chunks = (m1 - a0 + 3) >> 2;
    for (int c = threadIdx.x; c < chunks; c += kRsThreads) {
        const int a = a0 + 4 * c;
        if (a >= m0 && a + 4 <= m1) {
            const float* q = src + (a - m0);
            *reinterpret_cast<float4*>(row + a) = make_float4(q[0], q[1], q[2], q[3]);
        } else {
            for (int e = 0; e < 4; ++e) {
                const int i = a + e;
                if (i >= m0 && i < m1) row[i] = src[i - m0];
            }
        }
    }
}

// outputs m0 .. m0 + cnt of a stage -> dst[0 .. cnt) from its source tile src = source[s0 .. s0 + scnt); outputs outside
// [0, n_valid) are zero
__device__ __forceinline__ void rs_fwd_stage(float* dst, int m0, int cnt, int n_valid, const float* src, int s0, int scnt,
                                             const int32_t* first, const float* w, const RsStageGeo& g) {
    int m = m0 + (int)threadIdx.x;
    int u = rs_floordiv(m, g.ou), p = m - u * g.ou;
    const int su = kRsThreads / g.ou, sp = kRsThreads - su * g.ou;
    for (int k = threadIdx.x; k < cnt; k += kRsThreads, m += kRsThreads) {
        float acc = 0.f;
        const bool live = m >= 0 && m < n_valid;
        if (live) {
            const int base = first[p] + u * g.iu - s0;
            const float* wp = w + p * g.W;
            for (int j = 0; j < g.W; ++j) {
                const int idx = base + j;
                const float v = (unsigned)idx < (unsigned)scnt ? src[idx] : 0.f;
                acc = fmaf(wp[j], v, acc);
            }
        }
        dst[k] = acc;
        p += sp, u += su;
        if (p >= g.ou) p -= g.ou, ++u;
    }
}

// the adjoint of a stage: source samples m0 .. m0 + cnt -> dst[0 .. cnt) from the cotangent tile src = g[s0 .. s0 + scnt) of its
// outputs
__device__ __forceinline__ void rs_bwd_stage(float* dst, int m0, int cnt, int n_valid, const float* src, int s0, int scnt,
                                             const int32_t* tstart, const int32_t* toff, const float* tw, const RsStageGeo& g) {
    int m = m0 + (int)threadIdx.x;
    int v = rs_floordiv(m, g.iu), r = m - v * g.iu;
    const int sv = kRsThreads / g.iu, sr = kRsThreads - sv * g.iu;
    for (int k = threadIdx.x; k < cnt; k += kRsThreads, m += kRsThreads) {
        float acc = 0.f;
        const bool live = m >= 0 && m < n_valid;
        if (live) {
            const int base = v * g.ou - s0;
            const int e1 = tstart[r + 1];
            for (int e = tstart[r]; e < e1; ++e) {
                const int idx = base + toff[e];
                const float c = (unsigned)idx < (unsigned)scnt ? src[idx] : 0.f;
                acc = fmaf(tw[e], c, acc);
            }
        }
        dst[k] = acc;
        r += sr, v += sv;
        if (r >= g.iu) r -= g.iu, ++v;
    }
}

extern __shared__ uint4 rs_lds[];

// x (B,T) -> out (B,n_final); block = (tile, row)
__global__ __launch_bounds__(kRsThreads) void rs_forward_kernel(const int32_t* __restrict__ blob, const RsGeo g,
                                                                const float* __restrict__ x, float* __restrict__ out, int tiles,
                                                                int T, int n_low, int n_final) {
    int32_t* tab = reinterpret_cast<int32_t*>(rs_lds);
    float* xs = reinterpret_cast<float*>(tab + g.fwd_words);
    float* low = xs + g.f_in_max;
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    rs_copy_words(tab, blob, g.fwd_words);
    const int U0 = tile * g.UT;
    const int l0 = U0 * g.u.iu + g.u.minfirst, lcnt = (g.UT - 1) * g.u.iu + g.u.span;
    const int v0 = rs_floordiv(l0, g.d.ou), v1 = rs_floordiv(l0 + lcnt - 1, g.d.ou);
    const int i0 = v0 * g.d.iu + g.d.minfirst, icnt = min((v1 - v0) * g.d.iu + g.d.span, g.f_in_max);
    rs_stage_row(xs, x + (size_t)row * (size_t)T, i0, icnt, T);
    __syncthreads();
    rs_fwd_stage(low, l0, lcnt, n_low, xs, i0, icnt, tab + g.d.o_first, reinterpret_cast<const float*>(tab + g.d.o_w), g.d);
    __syncthreads();
    // (the source tile is spent: its room takes the tile's results, which leave as 16-byte stores)
    rs_fwd_stage(xs, U0 * g.u.ou, g.UT * g.u.ou, n_final, low, l0, lcnt, tab + g.u.o_first, reinterpret_cast<const float*>(tab + g.u.o_w), g.u);
    __syncthreads();
    rs_store_row(out + (size_t)row * (size_t)n_final, xs, U0 * g.u.ou, g.UT * g.u.ou, n_final);
}

// gy (B,n_final) -> gx (B,T)
__global__ __launch_bounds__(kRsThreads) void rs_backward_kernel(const int32_t* __restrict__ blob, const RsGeo g,
                                                                 const float* __restrict__ gy, float* __restrict__ gx, int tiles,
                                                                 int T, int n_low, int n_final) {
    int32_t* tab = reinterpret_cast<int32_t*>(rs_lds);
    float* gs = reinterpret_cast<float*>(tab + g.bwd_words);
    float* glow = gs + g.b_g_max;
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    rs_copy_words(tab, blob + g.bwd_off, g.bwd_words);
    const int V0 = tile * g.VT;
    const int l0 = (V0 - g.d.dumax) * g.d.ou, lcnt = (g.VT + g.d.dumax - g.d.dumin) * g.d.ou;
    const int w0 = rs_floordiv(l0, g.u.iu), w1 = rs_floordiv(l0 + lcnt - 1, g.u.iu);
    const int t0 = (w0 - g.u.dumax) * g.u.ou, tcnt = min((w1 - w0 + g.u.dumax - g.u.dumin + 1) * g.u.ou, g.b_g_max);
    rs_stage_row(gs, gy + (size_t)row * (size_t)n_final, t0, tcnt, n_final);
    __syncthreads();
    rs_bwd_stage(glow, l0, lcnt, n_low, gs, t0, tcnt, tab + g.u.o_tstart, tab + g.u.o_toff, reinterpret_cast<const float*>(tab + g.u.o_tw),
                 g.u);
    __syncthreads();
    rs_bwd_stage(gs, V0 * g.d.iu, g.VT * g.d.iu, T, glow, l0, lcnt, tab + g.d.o_tstart, tab + g.d.o_toff,
                 reinterpret_cast<const float*>(tab + g.d.o_tw), g.d);
    __syncthreads();
    rs_store_row(gx + (size_t)row * (size_t)T, gs, V0 * g.d.iu, g.VT * g.d.iu, T);
}

// ---------------------------------------------------------------- host: validation, tables, the cache
inline int rs_pad4(int words) { return (words + 3) & ~3; }
inline int64_t rs_out_len(int64_t n, int iu, int ou) { return (n * ou + iu - 1) / iu; }

int rs_check_stage(sg_ctx* ctx, const char* who, const char* name, const sg_resample_stage& st) {
    if (!st.first || !st.weight) return fail(ctx, SG_ERR_ARG, "%s: null table of the %s stage", who, name);
    if (st.in_unit < 1 || st.out_unit < 1 || st.W < 1 || st.in_unit > kRsMaxUnit || st.out_unit > kRsMaxUnit)
        return fail(ctx, SG_ERR_ARG, "%s: the %s stage needs 1 <= in_unit, out_unit <= %d and W >= 1 (%d, %d, %d)", who, name, kRsMaxUnit,
                    st.in_unit, st.out_unit, st.W);
    if ((int64_t)st.out_unit * st.W > kRsMaxTable)
        return fail(ctx, SG_ERR_ARG, "%s: the %s stage's table has out_unit * W = %lld entries, %d are built", who, name,
                    (long long)st.out_unit * st.W, kRsMaxTable);
    for (int p = 0; p < st.out_unit; ++p)
        if (st.first[p] > kRsMaxFirst || st.first[p] < -kRsMaxFirst)
            return fail(ctx, SG_ERR_ARG, "%s: first[%d] of the %s stage is out of range (%d)", who, p, name, st.first[p]);
    if (st.first[0] > 0) return fail(ctx, SG_ERR_ARG, "%s: the %s stage's window of phase 0 starts past its own output (first %d)", who, name, st.first[0]);
    for (int e = 0; e < st.out_unit * st.W; ++e)
        if (!std::isfinite(st.weight[e])) return fail(ctx, SG_ERR_ARG, "%s: weight %d of the %s stage is not finite", who, e, name);
    return SG_OK;
}

// the stage's halves of the blob, appended to `fwd` and `bwd`; offsets relative to the halves' starts
void rs_build_stage(const sg_resample_stage& st, RsStageGeo* g, std::vector<int32_t>* fwd, std::vector<int32_t>* bwd) {
    g->iu = st.in_unit, g->ou = st.out_unit, g->W = st.W, g->E = st.out_unit * st.W;
    int lo = st.first[0], hi = st.first[0];
    for (int p = 0; p < g->ou; ++p) lo = std::min(lo, st.first[p]), hi = std::max(hi, st.first[p]);
    g->minfirst = lo, g->span = hi + g->W - lo;
    g->dumin = rs_floordiv(lo, g->iu), g->dumax = rs_floordiv(hi + g->W - 1, g->iu);
    // forward: first[ou], weight[ou][W]
    g->o_first = (int)fwd->size();
    fwd->insert(fwd->end(), st.first, st.first + g->ou);
    fwd->resize(rs_pad4((int)fwd->size()));
    g->o_w = (int)fwd->size();
    fwd->resize(fwd->size() + g->E);
    std::memcpy(fwd->data() + g->o_w, st.weight, sizeof(float) * g->E);
    fwd->resize(rs_pad4((int)fwd->size()));
    // backward: the pairs by residue, each list in ascending output offset toff = p - du ou (distinct within a residue)
    struct Pair { int r, toff; float w; };
    std::vector<Pair> pairs;
    pairs.reserve(g->E);
    for (int p = 0; p < g->ou; ++p)
        for (int j = 0; j < g->W; ++j) {
            const int du = rs_floordiv(st.first[p] + j, g->iu);
            pairs.push_back(Pair{st.first[p] + j - du * g->iu, p - du * g->ou, st.weight[p * g->W + j]});
        }
    std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.r != b.r ? a.r < b.r : a.toff < b.toff; });
    g->o_tstart = (int)bwd->size();
    bwd->resize(bwd->size() + g->iu + 1, 0);
    for (const Pair& q : pairs) ++(*bwd)[g->o_tstart + q.r + 1];
    for (int r = 0; r < g->iu; ++r) (*bwd)[g->o_tstart + r + 1] += (*bwd)[g->o_tstart + r];
    bwd->resize(rs_pad4((int)bwd->size()));
    g->o_toff = (int)bwd->size();
    for (const Pair& q : pairs) bwd->push_back(q.toff);
    bwd->resize(rs_pad4((int)bwd->size()));
    g->o_tw = (int)bwd->size();
    for (const Pair& q : pairs) {
        int32_t bits;
        std::memcpy(&bits, &q.w, sizeof(bits));
        bwd->push_back(bits);
    }
    bwd->resize(rs_pad4((int)bwd->size()));
}

struct RsEntry : DevTable {  // key: the spec's content -- units, W, first and weight bits of both stages
    RsGeo geo{};
    size_t lds_fwd = 0, lds_bwd = 0;
};

void rs_key_stage(const sg_resample_stage& st, std::vector<int32_t>* key) {
    key->push_back(st.in_unit), key->push_back(st.out_unit), key->push_back(st.W);
    key->insert(key->end(), st.first, st.first + st.out_unit);
    const size_t at = key->size();
    key->resize(at + (size_t)st.out_unit * st.W);
    std::memcpy(key->data() + at, st.weight, sizeof(float) * (size_t)st.out_unit * st.W);
}

// the (checked) spec's tables on the device: found by content, or built and uploaded on `s` (first use only)
int rs_tables(sg_ctx* ctx, const char* who, const sg_wav_resample* r, hipStream_t s, RsEntry** out) {
    std::vector<int32_t> key;
    rs_key_stage(r->down, &key);
    rs_key_stage(r->up, &key);
    if (DevTable* hit = ctx->rs_cache.find(key)) return *out = static_cast<RsEntry*>(hit), SG_OK;

    RsEntry* e = new RsEntry();
    e->key.swap(key);
    RsGeo& g = e->geo;
    std::vector<int32_t> fwd, bwd;
    rs_build_stage(r->down, &g.d, &fwd, &bwd);
    rs_build_stage(r->up, &g.u, &fwd, &bwd);
    g.fwd_words = (int)fwd.size(), g.bwd_off = g.fwd_words, g.bwd_words = (int)bwd.size();
    fwd.insert(fwd.end(), bwd.begin(), bwd.end());
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(fwd.data());
    e->blob.assign(bytes, bytes + fwd.size() * sizeof(int32_t));
    g.UT = std::max(1, kRsTile / g.u.ou), g.VT = std::max(1, kRsTile / g.d.iu);
    // the largest tiles any block stages (the kernels' own formulas, bounded over the tile's position)
    g.f_low_max = (g.UT - 1) * g.u.iu + g.u.span;
    g.f_in_max = std::max(((g.f_low_max - 1) / g.d.ou + 1) * g.d.iu + g.d.span, g.UT * g.u.ou);
    g.b_low_max = (g.VT + g.d.dumax - g.d.dumin) * g.d.ou;
    g.b_g_max = std::max(((g.b_low_max - 1) / g.u.iu + 2 + g.u.dumax - g.u.dumin) * g.u.ou, g.VT * g.d.iu);
    e->lds_fwd = sizeof(float) * ((size_t)g.fwd_words + g.f_low_max + g.f_in_max);
    e->lds_bwd = sizeof(float) * ((size_t)g.bwd_words + g.b_low_max + g.b_g_max);
    if (e->lds_fwd > kRsLdsBytes || e->lds_bwd > kRsLdsBytes) {
        const size_t f = e->lds_fwd, b = e->lds_bwd;
        delete e;
        return fail(ctx, SG_ERR_ARG, "%s: tables and tile need %zu (forward) / %zu (backward) bytes of LDS, a block has %zu", who, f, b,
                    kRsLdsBytes);
    }
    if (int rc = dev_tables_insert(ctx, who, "", &ctx->rs_cache, kRsCacheMax, e, s)) return rc;
    return *out = e, SG_OK;
}

struct RsLens {
    int n_low, n_up, n_final;
};

int rs_check(sg_ctx* ctx, const char* who, const sg_wav_resample* r, const void* a, const void* b, int32_t B, int32_t T, int32_t N,
             hipStream_t s, RsEntry** e, RsLens* len) {
    if (!ctx) return SG_ERR_ARG;
    if (!r || !a || !b) return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    if (B < 1 || T < 1 || T > kRsMaxLen) return fail(ctx, SG_ERR_ARG, "%s: need B >= 1 and 1 <= T <= %d (B %d, T %d)", who, kRsMaxLen, B, T);
    if (r->same_size != 0 && r->same_size != 1) return fail(ctx, SG_ERR_ARG, "%s: same_size must be 0 or 1 (%d)", who, r->same_size);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    if (int rc = rs_check_stage(ctx, who, "down", r->down)) return rc;
    if (int rc = rs_check_stage(ctx, who, "up", r->up)) return rc;
    const int64_t n_low = rs_out_len(T, r->down.in_unit, r->down.out_unit);
    const int64_t n_up = rs_out_len(n_low, r->up.in_unit, r->up.out_unit);
    if (n_low > kRsMaxLen || n_up > kRsMaxLen) return fail(ctx, SG_ERR_ARG, "%s: the resampled row is longer than %d samples", who, kRsMaxLen);
    if (r->same_size && n_up < T) return fail(ctx, SG_ERR_ARG, "%s: same_size, but the round trip returns %lld of %d samples", who, (long long)n_up, T);
    len->n_low = (int)n_low, len->n_up = (int)n_up, len->n_final = r->same_size ? T : (int)n_up;
    if (N != len->n_final) return fail(ctx, SG_ERR_ARG, "%s: the output row has %d samples, the caller says %d", who, len->n_final, N);
    // (last: a refused call leaves no table behind)
    if (int rc = rs_tables(ctx, who, r, s, e)) return rc;
    return SG_OK;
}

int rs_grid(sg_ctx* ctx, const char* who, int n, int per_tile, int B, int* tiles, unsigned* blocks) {
    *tiles = (n + per_tile - 1) / per_tile;
    const int64_t total = (int64_t)*tiles * B;
    if (total > 0x7FFFFFFF) return fail(ctx, SG_ERR_ARG, "%s: %lld blocks are more than a launch holds", who, (long long)total);
    *blocks = (unsigned)total;
    return SG_OK;
}

}  // namespace

extern "C" int sg_wav_resample_forward(sg_ctx* ctx, const sg_wav_resample* r, const float* x_dev, int32_t B, int32_t T, float* out_dev,
                                       int32_t N, void* stream) {
    const char* who = "sg_wav_resample_forward";
    hipStream_t s = (hipStream_t)stream;
    RsEntry* e = nullptr;
    RsLens len;
    if (int rc = rs_check(ctx, who, r, x_dev, out_dev, B, T, N, s, &e, &len)) return rc;
    int tiles;
    unsigned blocks;
    if (int rc = rs_grid(ctx, who, len.n_final, e->geo.UT * e->geo.u.ou, B, &tiles, &blocks)) return rc;
    trace_mark(ctx, SG_STAGE_DS_FWD, s, 0);
    hipLaunchKernelGGL(rs_forward_kernel, dim3(blocks), dim3(kRsThreads), e->lds_fwd, s, (const int32_t*)e->dev, e->geo, x_dev, out_dev,
                       tiles, (int)T, len.n_low, len.n_final);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    trace_mark(ctx, SG_STAGE_DS_FWD, s, 1);
    return SG_OK;
}

extern "C" int sg_wav_resample_backward(sg_ctx* ctx, const sg_wav_resample* r, const float* g_dev, int32_t B, int32_t T, int32_t N,
                                        float* gx_dev, void* stream) {
    const char* who = "sg_wav_resample_backward";
    hipStream_t s = (hipStream_t)stream;
    RsEntry* e = nullptr;
    RsLens len;
    if (int rc = rs_check(ctx, who, r, g_dev, gx_dev, B, T, N, s, &e, &len)) return rc;
    int tiles;
    unsigned blocks;
    if (int rc = rs_grid(ctx, who, T, e->geo.VT * e->geo.d.iu, B, &tiles, &blocks)) return rc;
    trace_mark(ctx, SG_STAGE_DS_BWD, s, 0);
    hipLaunchKernelGGL(rs_backward_kernel, dim3(blocks), dim3(kRsThreads), e->lds_bwd, s, (const int32_t*)e->dev, e->geo, g_dev, gx_dev,
                       tiles, (int)T, len.n_low, len.n_final);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    trace_mark(ctx, SG_STAGE_DS_BWD, s, 1);
    return SG_OK;
}
