// Twelfth driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and iv_asan_driver.cpp):
// walks the i-vector GRADIENT entries under AddressSanitizer + UBSan -- every refusal of sg_iv_loss_grad and of the backward
// stage entries (SG_ERR_STATE without a model, SG_ERR_ARG before the first launch), the launch sequence of a chunk's forward
// and backward at every flag, the chunking of a large call (a chunk's backward right after its forward), and the workspace:
// a decision query grows none of the gradient's buffers, the first gradient call of a shape grows them before its first
// launch and never again at that shape; sg_destroy releases them.  No kernel runs.
#include "driver_common.h"

static const int kDim = 72;

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

static void on_launch(const Launch& l, void**) { g_seen.push_back(l); }
static bool tail_is(size_t at, std::initializer_list<const char*> want) {
    if (g_seen.size() < at + want.size()) return false;
    for (const char* w : want)
        if (kernel_name(g_seen[at++].name) != w) return false;
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
    std::vector<float> x((size_t)BMAX * T, 0.1f), feats((size_t)BMAX * F * kDim, 0.3f), scores((size_t)BMAX * S), loss(BMAX),
        grad((size_t)BMAX * T), zeroth((size_t)BMAX * C), first((size_t)BMAX * C * kDim), dz((size_t)BMAX * C),
        df((size_t)BMAX * C * kDim), div((size_t)BMAX * R, 0.2f), out((size_t)BMAX * F * kDim), raw((size_t)BMAX * F * 24);
    std::vector<int64_t> dec(BMAX), y(BMAX, 1);
    sg_loss_spec ce{};
    ce.loss = SG_LOSS_ENTROPY; ce.task = SG_TASK_CSI;
    auto lg = [&](int B, int TF, int flag) {
        return sg_iv_loss_grad(ctx, flag == 0 ? x.data() : feats.data(), y.data(), B, TF, flag, &ce, nullptr, dec.data(), scores.data(),
                               loss.data(), grad.data(), nullptr);
    };

    // ---- without a model: SG_ERR_STATE, nothing launched
    const long l0 = hipdouble_launches();
    EXPECT(lg(1, F, 3) == SG_ERR_STATE);
    EXPECT(sg_iv_extract_backward(ctx, zeroth.data(), first.data(), div.data(), 1, dz.data(), df.data(), nullptr) == SG_ERR_STATE);
    EXPECT(sg_iv_stats_backward(ctx, feats.data(), 1, F, dz.data(), df.data(), out.data(), nullptr) == SG_ERR_STATE);
    EXPECT(sg_iv_load(ctx, &m.desc) == SG_OK);
    const long a1 = hipdouble_live_allocs();

    // ---- every refusal: nothing launched, nothing allocated
    EXPECT(sg_iv_loss_grad(nullptr, feats.data(), y.data(), 1, F, 3, &ce, nullptr, dec.data(), nullptr, loss.data(), grad.data(), nullptr) ==
           SG_ERR_ARG);
    EXPECT(sg_iv_loss_grad(ctx, nullptr, y.data(), 1, F, 3, &ce, nullptr, dec.data(), nullptr, loss.data(), grad.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_loss_grad(ctx, feats.data(), nullptr, 1, F, 3, &ce, nullptr, dec.data(), nullptr, loss.data(), grad.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_loss_grad(ctx, feats.data(), y.data(), 1, F, 3, nullptr, nullptr, dec.data(), nullptr, loss.data(), grad.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_loss_grad(ctx, feats.data(), y.data(), 1, F, 3, &ce, nullptr, dec.data(), nullptr, loss.data(), nullptr, nullptr) == SG_ERR_ARG);
    {
        sg_loss_spec lin{};
        lin.loss = SG_LOSS_LINEAR;
        EXPECT(sg_iv_loss_grad(ctx, feats.data(), nullptr, 1, F, 3, &lin, nullptr, dec.data(), nullptr, loss.data(), grad.data(), nullptr) ==
               SG_ERR_ARG);
    }
    for (int B : {0, -1, (1 << 20) + 1}) EXPECT(lg(B, F, 3) == SG_ERR_ARG);
    for (int flag : {-1, 4}) EXPECT(lg(1, F, flag) == SG_ERR_ARG);
    for (int Tbad : {0, 399, (1 << 24) + 1}) EXPECT(lg(1, Tbad, 0) == SG_ERR_ARG);
    for (int Fbad : {0, -3, 65536}) EXPECT(lg(1, Fbad, 2) == SG_ERR_ARG);
    EXPECT(sg_iv_extract_backward(ctx, nullptr, first.data(), div.data(), 1, dz.data(), df.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_extract_backward(ctx, zeroth.data(), first.data(), nullptr, 1, dz.data(), df.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_extract_backward(ctx, zeroth.data(), first.data(), div.data(), 1, dz.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_extract_backward(ctx, zeroth.data(), first.data(), div.data(), 0, dz.data(), df.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_stats_backward(ctx, nullptr, 1, F, dz.data(), df.data(), out.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_stats_backward(ctx, feats.data(), 1, F, dz.data(), df.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_stats_backward(ctx, feats.data(), 1, 0, dz.data(), df.data(), out.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn_backward(nullptr, feats.data(), 3, 1, F, out.data(), raw.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn_backward(ctx, nullptr, 3, 1, F, out.data(), raw.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), 3, 1, F, nullptr, nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), 2, 1, F, out.data(), raw.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), 2, 1, F, nullptr, nullptr, nullptr) == SG_ERR_ARG);
    for (int ff : {0, 1, 4}) EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), ff, 1, F, nullptr, raw.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), 3, 0, F, out.data(), raw.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), 3, 1, 65536, out.data(), raw.data(), nullptr) == SG_ERR_ARG);
    EXPECT(hipdouble_launches() == l0 && hipdouble_live_allocs() == a1 && sg_last_error(ctx)[0] != 0);

    // ---- a decision query grows none of the gradient's buffers; the first gradient call of the shape does, once
    EXPECT(sg_iv_loss(ctx, feats.data(), y.data(), 3, F, 3, &ce, nullptr, dec.data(), scores.data(), loss.data(), nullptr) == SG_OK);
    const long a2 = hipdouble_live_allocs();
    g_seen.clear();
    EXPECT(lg(3, F, 3) == SG_OK);
    const long a3 = hipdouble_live_allocs();
    EXPECT(a3 > a2);
    // the chunk's forward (7 launches), then its backward: solve, d n (+ slice sum), d f, dgamma, dll, the contraction, posterior term + sum
    EXPECT(g_seen.size() == 15 && tail_is(0, {"iv_loglik_kernel", "iv_rowstat_kernel", "iv_stats_kernel", "iv_assemble_L_kernel",
                                             "iv_assemble_lin_kernel", "iv_solve_kernel", "iv_tail_kernel", "iv_solve_bwd_kernel",
                                             "iv_rowdot_kernel", "iv_slice_sum_kernel", "iv_rowdot_kernel", "iv_dgamma_kernel",
                                             "iv_dll_kernel", "iv_dx_quad_kernel", "iv_dx_post_kernel"}));
    if (g_seen.size() == 15) {
        EXPECT(g_seen[7].grid.x == 3 && g_seen[8].grid.x == 1 && g_seen[8].grid.y == 1 && g_seen[8].grid.z == 1);  // P = 28: one slice
        EXPECT(g_seen[10].grid.x == (unsigned)(C * kDim + 63) / 64 && g_seen[10].grid.y == 1);
        EXPECT(g_seen[11].grid.x == 1 && g_seen[11].grid.y == 1 && g_seen[11].grid.z == 3);                      // Cp = 64
        EXPECT(g_seen[14].block.x == 288 && g_seen[14].grid.y == 3 && g_seen[12].grid.x == 10);                  // 39 frames, 4 a block
        EXPECT(g_seen[13].grid.x == 1 && g_seen[13].grid.y == 3 && g_seen[13].grid.z == 4 && g_seen[13].block.x == 256);
    }
    g_seen.clear();
    EXPECT(lg(3, F, 3) == SG_OK && lg(2, F, 3) == SG_OK && hipdouble_live_allocs() == a3);  // the same shape, a smaller one: nothing
    EXPECT(sg_iv_loss(ctx, feats.data(), y.data(), 3, F, 3, &ce, nullptr, dec.data(), scores.data(), loss.data(), nullptr) == SG_OK);
    EXPECT(hipdouble_live_allocs() == a3);
    // flags 2 and 1 end with the front-end adjoint; flag 0 adds the MFCC adjoint and the overlap-add behind it
    g_seen.clear();
    EXPECT(lg(2, F, 2) == SG_OK && g_seen.size() == 17 && kernel_name(g_seen[0].name) == "iv_delta_cmvn_kernel" &&
           kernel_name(g_seen[16].name) == "iv_delta_cmvn_bwd_kernel");
    g_seen.clear();
    EXPECT(lg(2, F, 1) == SG_OK && g_seen.size() == 17 && kernel_name(g_seen[16].name) == "iv_delta_cmvn_bwd_kernel" && g_seen[16].grid.x == 2);
    g_seen.clear();
    EXPECT(lg(2, T, 0) == SG_OK);
    {
        size_t at = 0;
        while (at < g_seen.size() && kernel_name(g_seen[at].name) != "iv_delta_cmvn_bwd_kernel") ++at;
        EXPECT(at + 3 == g_seen.size());  // d raw (30 columns), then the two launches of the MFCC adjoint
    }
    const long a4 = hipdouble_live_allocs();
    EXPECT(lg(2, T, 0) == SG_OK && hipdouble_live_allocs() == a4);

    // ---- a call of 130 rows: three chunks (64 + 64 + 2), each chunk's backward right after its forward
    g_seen.clear();
    EXPECT(lg(BMAX, F, 3) == SG_OK && g_seen.size() == 45);
    if (g_seen.size() == 45)
        EXPECT(g_seen[7].grid.x == 64 && g_seen[15].grid.x > 0 && kernel_name(g_seen[15].name) == "iv_loglik_kernel" &&
               kernel_name(g_seen[28].name) == "iv_dx_quad_kernel" && g_seen[37].grid.x == 2 && g_seen[44].grid.y == 2);
    const long a5 = hipdouble_live_allocs();
    EXPECT(lg(BMAX, F, 3) == SG_OK && lg(64, F, 3) == SG_OK && hipdouble_live_allocs() == a5);
    // the stage entries chunk the same way and own nothing beyond the workspace
    g_seen.clear();
    EXPECT(sg_iv_extract_backward(ctx, zeroth.data(), first.data(), div.data(), BMAX, dz.data(), df.data(), nullptr) == SG_OK &&
           g_seen.size() == 21);
    g_seen.clear();
    EXPECT(sg_iv_stats_backward(ctx, feats.data(), BMAX, F, dz.data(), df.data(), out.data(), nullptr) == SG_OK && g_seen.size() == 21);
    g_seen.clear();
    EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), 3, 5, F, out.data(), raw.data(), nullptr) == SG_OK && g_seen.size() == 1);
    EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), 3, 5, F, nullptr, raw.data(), nullptr) == SG_OK);
    EXPECT(sg_iv_delta_cmvn_backward(ctx, feats.data(), 2, 5, F, nullptr, raw.data(), nullptr) == SG_OK);
    EXPECT(hipdouble_live_allocs() == a5);

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "iv_grad_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
