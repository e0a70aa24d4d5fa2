// Eleventh driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks the GMM / i-vector entries under AddressSanitizer + UBSan -- every refusal of sg_iv_load (NULL pointers, sizes out of
// range, a non-finite entry, an asymmetric invcovars / sigma_inv) and of the pass entries (SG_ERR_ARG before the first launch,
// SG_ERR_STATE without a model), the packing sg_iv_load uploads (W, the (i, j) table, V^T and U read back through the first
// launch that takes them: "device" memory is host memory here) against the direct formulas, the launch sequence of a forward
// at every flag, the chunking of a large call (64 utterances per chunk) and the workspace (grown before the first launch of a
// shape, never again at that shape; released by sg_destroy).  No kernel runs.
#include "driver_common.h"

static const int kDim = 72, kK = 2700;

struct IvModel {
    int C, R, D, S;
    std::vector<float> g, mi, ic, ext, si, emean, lda, pmean, ptrans, ppsi, enroll;
    sg_iv_weights desc{};
    static std::vector<float> spd(int C, unsigned seed) {  // symmetric, diagonally dominant
        std::vector<float> a = rnd((size_t)C * kDim * kDim, seed, 0.01f);
        for (int c = 0; c < C; ++c)
            for (int i = 0; i < kDim; ++i)
                for (int j = 0; j <= i; ++j) {
                    float* m = a.data() + (size_t)c * kDim * kDim;
                    m[j * kDim + i] = m[i * kDim + j];
                    if (i == j) m[i * kDim + j] += 1.f;
                }
        return a;
    }
    IvModel(int C_, int R_, int D_, int S_) : C(C_), R(R_), D(D_), S(S_) {
        g = rnd(C, 1, 1.f, -80.f); mi = rnd((size_t)C * kDim, 2); ic = spd(C, 3); ext = rnd((size_t)C * kDim * R, 4, 0.2f);
        si = spd(C, 5); emean = rnd(R, 6); lda = rnd((size_t)D * (R + 1), 7); pmean = rnd(D, 8); ptrans = rnd((size_t)D * D, 9);
        ppsi = rnd(D, 10, 0.5f, 1.f); enroll = rnd((size_t)S * D, 11);
        desc.C = C; desc.R = R; desc.D = D; desc.S = S;
        desc.gconsts = g.data(); desc.means_invcovars = mi.data(); desc.invcovars = ic.data(); desc.extractor = ext.data();
        desc.sigma_inv = si.data(); desc.ivector_offset = 3.f; desc.emb_mean = emean.data(); desc.lda = lda.data();
        desc.plda_mean = pmean.data(); desc.plda_transform = ptrans.data(); desc.plda_psi = ppsi.data(); desc.enroll = enroll.data();
        desc.threshold = -INFINITY;
    }
};

// what the launches carry: the packed tables (first arguments of the kernels that read them)
static const float *g_W = nullptr, *g_U = nullptr, *g_Vt = nullptr;
static const uint16_t* g_pairs = nullptr;
static int g_Cp = 0, g_Pp = 0;
static void on_launch(const Launch& l, void** args) {
    g_seen.push_back(l);
    see_tail(l, args);
    const std::string k = kernel_name(l.name);
    if (k == "iv_loglik_kernel") {
        g_W = *static_cast<const float* const*>(args[2]);
        g_pairs = *static_cast<const uint16_t* const*>(args[3]);
        g_Cp = *static_cast<const int*>(args[6]);
    } else if (k == "iv_assemble_L_kernel") {
        g_U = *static_cast<const float* const*>(args[0]);
        g_Pp = *static_cast<const int*>(args[1]);
    } else if (k == "iv_assemble_lin_kernel") {
        g_Vt = *static_cast<const float* const*>(args[0]);
    }
}
static bool seq_is(std::initializer_list<const char*> want) {
    if (g_seen.size() != want.size()) return false;
    size_t i = 0;
    for (const char* w : want)
        if (kernel_name(g_seen[i++].name) != w) return false;
    return true;
}

int main() {
    hipdouble_set_launch_hook(record_launch);
    g_on_launch = on_launch;
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int C = 5, R = 7, D = 4, S = 3, F = 13, BMAX = 130, T = 1600;
    IvModel m(C, R, D, S);
    std::vector<float> x((size_t)BMAX * T, 0.1f), feats((size_t)BMAX * F * kDim, 0.3f), scores((size_t)BMAX * S), emb((size_t)BMAX * D),
        ivec((size_t)BMAX * R), loss(BMAX), zeroth((size_t)BMAX * C), first((size_t)BMAX * C * kDim), out((size_t)BMAX * F * kDim);
    std::vector<int64_t> dec(BMAX), y(BMAX, 1);
    sg_loss_spec ce{};
    ce.loss = SG_LOSS_ENTROPY; ce.task = SG_TASK_CSI;
    auto fwd = [&](int B, int TF, int flag) {
        return sg_iv_forward(ctx, flag == 0 ? x.data() : feats.data(), B, TF, flag, nullptr, dec.data(), scores.data(), emb.data(),
                             ivec.data(), nullptr);
    };

    // ---- without a model: SG_ERR_STATE, nothing launched
    const long l0 = hipdouble_launches(), a0 = hipdouble_live_allocs();
    EXPECT(fwd(1, F, 3) == SG_ERR_STATE);
    EXPECT(sg_iv_stats(ctx, feats.data(), 1, F, zeroth.data(), first.data(), nullptr) == SG_ERR_STATE);
    EXPECT(sg_iv_set_enroll(ctx, m.enroll.data(), S, 0.f) == SG_ERR_STATE);
    EXPECT(sg_iv_enroll_override(ctx, m.enroll.data(), S) == SG_ERR_STATE);

    // ---- every refusal of the load: nothing allocated
    EXPECT(sg_iv_load(nullptr, &m.desc) == SG_ERR_ARG && sg_iv_load(ctx, nullptr) == SG_ERR_ARG);
    {
        sg_iv_weights w = m.desc;
        const float** ptrs[] = {&w.gconsts, &w.means_invcovars, &w.invcovars, &w.extractor, &w.sigma_inv, &w.emb_mean, &w.lda,
                                &w.plda_mean, &w.plda_transform, &w.plda_psi, &w.enroll};
        for (const float** p : ptrs) {
            const float* keep = *p;
            *p = nullptr;
            EXPECT(sg_iv_load(ctx, &w) == SG_ERR_ARG);
            *p = keep;
        }
        for (int bad : {0, -1, 4097}) { w = m.desc; w.C = bad; EXPECT(sg_iv_load(ctx, &w) == SG_ERR_ARG); }
        for (int bad : {0, -1, 1025}) { w = m.desc; w.R = bad; EXPECT(sg_iv_load(ctx, &w) == SG_ERR_ARG); }
        for (int bad : {0, -1, 513}) { w = m.desc; w.D = bad; EXPECT(sg_iv_load(ctx, &w) == SG_ERR_ARG); }
        for (int bad : {0, -1, 1025}) { w = m.desc; w.S = bad; EXPECT(sg_iv_load(ctx, &w) == SG_ERR_ARG); }
        w = m.desc; w.ivector_offset = NAN; EXPECT(sg_iv_load(ctx, &w) == SG_ERR_ARG);
        // a non-finite entry at the very end of each array, an asymmetric pair in the last component
        for (std::vector<float>* v : {&m.g, &m.mi, &m.ic, &m.ext, &m.si}) {
            const float keep = v->back();
            v->back() = INFINITY;
            EXPECT(sg_iv_load(ctx, &m.desc) == SG_ERR_ARG);
            v->back() = keep;
        }
        for (std::vector<float>* v : {&m.ic, &m.si}) {
            float& e = (*v)[(size_t)(C - 1) * kDim * kDim + 70 * kDim + 71];
            const float keep = e;
            e = keep + 0.5f;
            EXPECT(sg_iv_load(ctx, &m.desc) == SG_ERR_ARG);
            EXPECT(std::string(sg_last_error(ctx)).find("not symmetric") != std::string::npos);
            e = keep;
        }
    }
    EXPECT(hipdouble_launches() == l0 && hipdouble_live_allocs() == a0);

    // ---- the load, twice: the second releases what the first took
    EXPECT(sg_iv_load(ctx, &m.desc) == SG_OK);
    const long a1 = hipdouble_live_allocs();
    EXPECT(sg_iv_load(ctx, &m.desc) == SG_OK);
    EXPECT(hipdouble_live_allocs() == a1 && hipdouble_launches() == l0);

    // ---- every refusal of the pass entries: nothing launched, nothing allocated
    EXPECT(sg_iv_forward(nullptr, feats.data(), 1, F, 3, nullptr, dec.data(), nullptr, nullptr, nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_forward(ctx, nullptr, 1, F, 3, nullptr, dec.data(), nullptr, nullptr, nullptr, nullptr) == SG_ERR_ARG);
    for (int B : {0, -1, (1 << 20) + 1}) EXPECT(fwd(B, F, 3) == SG_ERR_ARG);
    for (int flag : {-1, 4}) EXPECT(fwd(1, F, flag) == SG_ERR_ARG);
    for (int Tbad : {0, 399, (1 << 24) + 1}) EXPECT(fwd(1, Tbad, 0) == SG_ERR_ARG);
    for (int Fbad : {0, -3, 65536}) EXPECT(fwd(1, Fbad, 2) == SG_ERR_ARG);
    EXPECT(sg_iv_loss(ctx, feats.data(), y.data(), 1, F, 3, nullptr, nullptr, dec.data(), nullptr, loss.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_loss(ctx, feats.data(), nullptr, 1, F, 3, &ce, nullptr, dec.data(), nullptr, loss.data(), nullptr) == SG_ERR_ARG);
    {
        sg_loss_spec lin{};
        lin.loss = SG_LOSS_LINEAR;
        EXPECT(sg_iv_loss(ctx, feats.data(), nullptr, 1, F, 3, &lin, nullptr, dec.data(), nullptr, loss.data(), nullptr) == SG_ERR_ARG);
    }
    EXPECT(sg_iv_delta_cmvn(ctx, nullptr, 1, F, 24, out.data(), out.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn(ctx, feats.data(), 1, F, 24, nullptr, nullptr, nullptr) == SG_ERR_ARG);
    for (int ld : {23, 0, 4097}) EXPECT(sg_iv_delta_cmvn(ctx, feats.data(), 1, F, ld, out.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn(ctx, feats.data(), 0, F, 24, out.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn(ctx, feats.data(), 1, 65536, 24, out.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_stats(ctx, nullptr, 1, F, zeroth.data(), first.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_stats(ctx, feats.data(), 1, F, nullptr, first.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_extract(ctx, zeroth.data(), nullptr, 1, ivec.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_extract(ctx, zeroth.data(), first.data(), 0, ivec.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_set_enroll(ctx, m.enroll.data(), 0, 0.f) == SG_ERR_ARG && sg_iv_enroll_override(ctx, m.enroll.data(), 1025) == SG_ERR_ARG);
    EXPECT(hipdouble_launches() == l0 && hipdouble_live_allocs() == a1 && sg_last_error(ctx)[0] != 0);

    // ---- a forward at every flag: the launch sequence, and the tables the kernels were handed
    g_seen.clear();
    EXPECT(fwd(3, F, 3) == SG_OK);
    EXPECT(seq_is({"iv_loglik_kernel", "iv_rowstat_kernel", "iv_stats_kernel", "iv_assemble_L_kernel", "iv_assemble_lin_kernel",
                   "iv_solve_kernel", "iv_tail_kernel"}));
    if (g_seen.size() == 7) {
        EXPECT(g_seen[0].grid.x == 1 && g_seen[0].grid.y == 1 && g_seen[0].block.x == 256);       // 39 frames: one 64-row tile
        EXPECT(g_seen[1].grid.x == 10 && g_seen[2].grid.x == 1 && g_seen[2].grid.y == 3);
        EXPECT(g_seen[3].grid.x == 1 && g_seen[3].grid.y == 1);                                  // P = 28 -> one block of 256
        EXPECT(g_seen[4].grid.x == 1 && g_seen[4].grid.y == 1 && g_seen[4].grid.z == 1);
        EXPECT(g_seen[5].grid.x == 3 && g_seen[6].grid.x == 3);
    }
    const long a2 = hipdouble_live_allocs();
    g_seen.clear();
    EXPECT(fwd(3, F, 3) == SG_OK && hipdouble_live_allocs() == a2);  // the same shape again: nothing allocated
    EXPECT(fwd(2, F, 3) == SG_OK && hipdouble_live_allocs() == a2);  // a smaller one: nothing either
    g_seen.clear();
    EXPECT(fwd(2, F, 2) == SG_OK && g_seen.size() == 8 && kernel_name(g_seen[0].name) == "iv_delta_cmvn_kernel");
    g_seen.clear();
    EXPECT(fwd(2, F, 1) == SG_OK && g_seen.size() == 8 && kernel_name(g_seen[0].name) == "iv_delta_cmvn_kernel" && g_seen[0].grid.x == 2);
    g_seen.clear();
    EXPECT(fwd(2, T, 0) == SG_OK);
    {   // the scale decision and the MFCC first, then the same eight launches
        size_t at = 0;
        while (at < g_seen.size() && kernel_name(g_seen[at].name) != "iv_delta_cmvn_kernel") ++at;
        EXPECT(at >= 2 && g_seen.size() == at + 8);
    }
    EXPECT(sg_iv_loss(ctx, feats.data(), y.data(), 2, F, 3, &ce, nullptr, dec.data(), scores.data(), loss.data(), nullptr) == SG_OK);

    // ---- the packing against the direct formulas (float64 here, rounded once, as the library does)
    EXPECT(g_W && g_pairs && g_U && g_Vt && g_Cp == 64 && g_Pp == 256);
    if (g_W && g_pairs && g_U && g_Vt && g_Cp == 64 && g_Pp == 256) {
        int seen_k = 0;
        for (int k = 0; k < kK; ++k) {
            const int i = g_pairs[k] & 0xff, j = g_pairs[k] >> 8;
            if (k < kDim) { EXPECT(i == k && j == kDim); }
            else { EXPECT(i <= j && j < kDim && k == kDim + i * kDim - i * (i - 1) / 2 + (j - i)); }
            for (int c = 0; c < C; ++c) {
                const float* Sm = m.ic.data() + (size_t)c * kDim * kDim;
                const float want = k < kDim ? m.mi[(size_t)c * kDim + k]
                                            : (float)(i == j ? -0.5 * (double)Sm[i * kDim + i] : -(double)Sm[i * kDim + j]);
                EXPECT(g_W[(size_t)k * g_Cp + c] == want);
            }
            for (int c = C; c < g_Cp; ++c) EXPECT(g_W[(size_t)k * g_Cp + c] == 0.f);  // the padded components weigh nothing
            ++seen_k;
        }
        EXPECT(seen_k == kK);
        for (int c = 0; c < C; ++c) {
            const float* M = m.ext.data() + (size_t)c * kDim * R;
            const float* Sg = m.si.data() + (size_t)c * kDim * kDim;
            std::vector<double> V((size_t)R * kDim, 0.0);
            for (int r = 0; r < R; ++r)
                for (int d = 0; d < kDim; ++d)
                    for (int e = 0; e < kDim; ++e) V[(size_t)r * kDim + d] += (double)M[(size_t)e * R + r] * (double)Sg[e * kDim + d];
            for (int r = 0; r < R; ++r)
                for (int d = 0; d < kDim; ++d) {
                    const double got = g_Vt[((size_t)c * kDim + d) * R + r], want = V[(size_t)r * kDim + d];
                    EXPECT(std::fabs(got - want) <= 1e-6 * (std::fabs(want) + 1e-3));
                }
            size_t p = 0;
            for (int r1 = 0; r1 < R; ++r1)
                for (int r2 = r1; r2 < R; ++r2, ++p) {
                    double u = 0.0;
                    for (int d = 0; d < kDim; ++d) u += V[(size_t)r1 * kDim + d] * (double)M[(size_t)d * R + r2];
                    EXPECT(std::fabs((double)g_U[(size_t)c * g_Pp + p] - u) <= 1e-6 * (std::fabs(u) + 1e-3));
                }
            for (; p < (size_t)g_Pp; ++p) EXPECT(g_U[(size_t)c * g_Pp + p] == 0.f);
        }
    }

    // ---- a call of 130 rows: three chunks (64 + 64 + 2), each with the whole sequence; the workspace is sized for one chunk
    g_seen.clear();
    EXPECT(fwd(BMAX, F, 3) == SG_OK && g_seen.size() == 21);
    if (g_seen.size() == 21) EXPECT(g_seen[5].grid.x == 64 && g_seen[12].grid.x == 64 && g_seen[19].grid.x == 2 && g_seen[20].grid.x == 2);
    const long a3 = hipdouble_live_allocs();
    EXPECT(fwd(BMAX, F, 3) == SG_OK && fwd(64, F, 3) == SG_OK && hipdouble_live_allocs() == a3);
    // the stage entries chunk the same way and own nothing beyond the workspace
    g_seen.clear();
    EXPECT(sg_iv_stats(ctx, feats.data(), BMAX, F, zeroth.data(), first.data(), nullptr) == SG_OK && g_seen.size() == 9);
    g_seen.clear();
    EXPECT(sg_iv_extract(ctx, zeroth.data(), first.data(), BMAX, ivec.data(), nullptr) == SG_OK && g_seen.size() == 9);
    g_seen.clear();
    EXPECT(sg_iv_delta_cmvn(ctx, feats.data(), 5, F, 72, out.data(), nullptr, nullptr) == SG_OK && g_seen.size() == 1);
    EXPECT(sg_iv_delta_cmvn(ctx, feats.data(), 5, F, 24, nullptr, out.data(), nullptr) == SG_OK);
    EXPECT(hipdouble_live_allocs() == a3);

    // ---- enrolment: a larger table replaces the old one, an override owns nothing
    {
        std::vector<float> more((size_t)9 * D, 0.2f);
        EXPECT(sg_iv_set_enroll(ctx, more.data(), 9, 1.5f) == SG_OK && hipdouble_live_allocs() == a3);
        std::vector<float> sc9((size_t)2 * 9);
        EXPECT(sg_iv_forward(ctx, feats.data(), 2, F, 3, nullptr, dec.data(), sc9.data(), nullptr, nullptr, nullptr) == SG_OK);
        EXPECT(sg_iv_enroll_override(ctx, more.data(), 2) == SG_OK && sg_iv_enroll_override(ctx, nullptr, 0) == SG_OK);
        EXPECT(sg_iv_set_enroll(ctx, nullptr, 9, -INFINITY) == SG_OK && hipdouble_live_allocs() == a3);
    }

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);

    // ---- the enrol path shared with the x-vector model, from a model loaded with one speaker
    {
        IvModel one(C, R, D, 1);
        sg_ctx* c1 = nullptr;
        EXPECT(sg_create(0, &c1) == SG_OK && c1 && sg_iv_load(c1, &one.desc) == SG_OK);
        if (c1) {
            walk_enrol_path(c1, sg_iv_set_enroll, sg_iv_enroll_override, [&] {
                return sg_iv_forward(c1, feats.data(), 2, F, 3, nullptr, dec.data(), scores.data(), nullptr, nullptr, nullptr);
            }, D, one.enroll.data(), one.ppsi.data());
            sg_destroy(c1);
        }
        EXPECT(hipdouble_live_allocs() == 0);
    }
    if (g_fail) return 1;
    std::fprintf(stderr, "iv_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
