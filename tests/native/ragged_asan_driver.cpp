// Driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp) for the
// entry points that take batches of unequal lengths: sg_xv_forward_ragged, sg_xv_loss_grad_ragged, sg_xv_pgd_run_ragged.  Under
// AddressSanitizer + UBSan it walks valid calls, every refusal (each leaves one line with its return code and must come before
// the first launch), a context that goes from a uniform call to a ragged one and back (the workspace grows once and is reused),
// and two contexts side by side.  It prints one line per kernel launch, in order -- kernel name with template arguments, grid,
// block, dynamic LDS -- for tests/test_ragged_launch_sequence.py, which compares the output with
// tests/native/ragged_launch_sequence.expected.  "Device" buffers are host buffers sized exactly as the header says (the
// lengths' device copy is never read by the host half); the double's copies are real.  No kernel runs.
#include "driver_common.h"

static std::string g_label;
static int g_n = 0;
static void print_line(const Launch& l, void**) {
    print_launch(g_label, ++g_n, l);
    std::printf("\n");
}

struct Call {  // one call's buffers, exact extents
    int B, T;
    std::vector<float> x, lower, upper, scores, loss, grad, emb, temb, ltr;
    std::vector<int64_t> y, dec, dtr;
    std::vector<uint8_t> succ;
    std::vector<int32_t> len_dev, len_host;
    Call(int B_, int T_, std::vector<int32_t> lens, int D, int S, int K)
        : B(B_), T(T_), x(rnd((size_t)B_ * T_, 200, 0.3f)), lower(x), upper(x), scores((size_t)B_ * S), loss(B_), grad((size_t)B_ * T_),
          emb((size_t)B_ * D), temb((size_t)B_ * 512), ltr((size_t)(K + 1) * B_), y(B_, 1), dec(B_), dtr((size_t)(K + 1) * B_), succ(B_),
          len_dev(lens), len_host(lens) {}
};

int main() {
    setenv("SG_TUNE", "1", 1);  // SG_EOT_MAX_ROWS counts, where a case sets it
    unsetenv("SG_EOT_MAX_ROWS");
    g_on_launch = print_line;
    hipdouble_set_launch_hook(record_launch);
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int D = 24, S = 4, K = 2;
    XvModel xv(D, S);
    EXPECT(sg_xv_load(ctx, &xv.desc) == SG_OK);
    sg_loss_spec ls{};
    ls.loss = SG_LOSS_ENTROPY;
    sg_dither dz{};
    sg_pgd_params pp{};
    pp.step_size = 4e-4f; pp.max_iter = K; pp.grad_sign = 1; pp.eot_size = 1; pp.eot_batch_size = 1;
    pp.dither.seed = 99; pp.dither.index_base = 5;

    const auto said = [&](const std::string& label, int rc) {
        if (rc != SG_OK) std::printf("%s | rc=%d %s\n", label.c_str(), rc, sg_last_error(ctx));
        return rc;
    };
    const auto forward = [&](sg_ctx* c, const std::string& label, Call& a, const int32_t* ld, const int32_t* lh) {
        g_label = label; g_n = 0;
        return said(label, sg_xv_forward_ragged(c, a.x.data(), ld, lh, a.B, a.T, &dz, a.dec.data(), a.scores.data(), a.emb.data(), a.temb.data(),
                                                nullptr));
    };
    const auto loss_grad = [&](sg_ctx* c, const std::string& label, Call& a, const int32_t* ld, const int32_t* lh) {
        g_label = label; g_n = 0;
        return said(label, sg_xv_loss_grad_ragged(c, a.x.data(), ld, lh, a.y.data(), a.B, a.T, &ls, &dz, a.dec.data(), a.scores.data(),
                                                  a.loss.data(), a.grad.data(), nullptr));
    };
    const auto pgd = [&](sg_ctx* c, const std::string& label, Call& a, const int32_t* ld, const int32_t* lh) {
        g_label = label; g_n = 0;
        return said(label, sg_xv_pgd_run_ragged(c, a.x.data(), a.y.data(), a.lower.data(), a.upper.data(), ld, lh, a.B, a.T, &pp, a.succ.data(),
                                                a.dec.data(), a.scores.data(), a.loss.data(), a.ltr.data(), a.dtr.data(), nullptr));
    };

    // ---- every refusal, at each of the three entries: SG_ERR_ARG before the first launch and before the workspace is touched
    const long l0 = hipdouble_launches(), a0 = hipdouble_live_allocs();
    struct Bad { const char* what; int T; std::vector<int32_t> lens; };
    const Bad bad[] = {
        {"a length above T_max", 16001, {16001, 16002, 9999}},
        {"a length below one window", 16001, {16001, 399, 9999}},
        {"a length below the TDNN context", 16001, {16001, 5039, 9999}},
        {"no row at T_max", 16001, {16000, 9999, 8000}},
        {"B=3 T_max=5043 lengths 5043 4000 3333: 25 and 21 frames are below the TDNN context", 5043, {5043, 4000, 3333}},
    };
    for (const Bad& b : bad) {
        Call a(3, b.T, b.lens, D, S, K);
        EXPECT(forward(ctx, std::string("refused: forward, ") + b.what, a, a.len_dev.data(), a.len_host.data()) == SG_ERR_ARG);
        EXPECT(loss_grad(ctx, std::string("refused: loss_grad, ") + b.what, a, a.len_dev.data(), a.len_host.data()) == SG_ERR_ARG);
        EXPECT(pgd(ctx, std::string("refused: pgd_run, ") + b.what, a, a.len_dev.data(), a.len_host.data()) == SG_ERR_ARG);
    }
    {
        Call a(3, 16001, {16001, 9999, 5043}, D, S, K);
        EXPECT(forward(ctx, "refused: forward, lengths_host NULL", a, a.len_dev.data(), nullptr) == SG_ERR_ARG);
        EXPECT(loss_grad(ctx, "refused: loss_grad, lengths_dev NULL", a, nullptr, a.len_host.data()) == SG_ERR_ARG);
        EXPECT(pgd(ctx, "refused: pgd_run, lengths_host NULL", a, a.len_dev.data(), nullptr) == SG_ERR_ARG);
        std::vector<float> noise(16);
        dz.noise_dev = noise.data();
        EXPECT(loss_grad(ctx, "refused: loss_grad, an explicit dither tensor", a, a.len_dev.data(), a.len_host.data()) == SG_ERR_ARG);
        dz.noise_dev = nullptr;
        pp.max_iter = -1;
        EXPECT(pgd(ctx, "refused: pgd_run, max_iter -1", a, a.len_dev.data(), a.len_host.data()) == SG_ERR_ARG);
        pp.max_iter = K;
        pp.eot_size = 4; pp.eot_batch_size = 3;
        EXPECT(pgd(ctx, "refused: pgd_run, eot 4 in batches of 3", a, a.len_dev.data(), a.len_host.data()) == SG_ERR_ARG);
        pp.eot_size = 1; pp.eot_batch_size = 1;
        a.B = 0;
        EXPECT(forward(ctx, "refused: forward, B 0", a, a.len_dev.data(), a.len_host.data()) == SG_ERR_ARG);
    }
    EXPECT(hipdouble_launches() == l0 && hipdouble_live_allocs() == a0);

    // ---- a context from a uniform call to a ragged one and back: the workspace grows for the ragged call and is then reused
    {
        Call u(2, 8000, {8000, 8000}, D, S, K);
        g_label = "uniform B=2 T=8000 loss_grad"; g_n = 0;
        EXPECT(sg_xv_loss_grad(ctx, u.x.data(), u.y.data(), 2, 8000, SG_FLAG_WAV, &ls, &dz, u.dec.data(), u.scores.data(), u.loss.data(),
                               u.grad.data(), nullptr) == SG_OK);
        Call a(3, 16001, {16001, 9999, 5043}, D, S, K);  // 5043: the shortest utterance the engine takes (32 frames)
        EXPECT(loss_grad(ctx, "B=3 T_max=16001 lengths 16001 9999 5043 loss_grad", a, a.len_dev.data(), a.len_host.data()) == SG_OK);
        const long live = hipdouble_live_allocs();
        int32_t dims[4] = {0, 0, 0, 0};  // the debug read-backs report the padded dims
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DFEATS_RAW, nullptr, 0, dims, nullptr) == SG_OK);
        EXPECT(dims[0] == 1 && dims[1] == 3 && dims[2] == sg_xv_num_frames(16001) && dims[3] == 30);
        std::vector<float> raw((size_t)3 * dims[2] * 30);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DFEATS_RAW, raw.data(), (int64_t)raw.size(), nullptr, nullptr) == SG_OK);
        int32_t rows = 0, ch = 0;
        EXPECT(sg_xv_debug_activation(ctx, 5, nullptr, 0, &rows, &ch, nullptr) == SG_OK && rows == dims[2] - 30 && ch == 1536);
        std::vector<float> act((size_t)3 * rows * ch);
        EXPECT(sg_xv_debug_activation(ctx, 5, act.data(), (int64_t)act.size(), nullptr, nullptr, nullptr) == SG_OK);
        EXPECT(forward(ctx, "B=3 T_max=16001 lengths 16001 9999 5043 forward", a, a.len_dev.data(), a.len_host.data()) == SG_OK);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DEMB, nullptr, 0, dims, nullptr) == SG_ERR_STATE);  // (a forward since)
        g_label = "uniform B=3 T=16001 loss_grad"; g_n = 0;
        EXPECT(sg_xv_loss_grad(ctx, a.x.data(), a.y.data(), 3, 16001, SG_FLAG_WAV, &ls, &dz, a.dec.data(), a.scores.data(), a.loss.data(),
                               a.grad.data(), nullptr) == SG_OK);
        g_label = "uniform B=2 T=8000 loss_grad again"; g_n = 0;
        EXPECT(sg_xv_loss_grad(ctx, u.x.data(), u.y.data(), 2, 8000, SG_FLAG_WAV, &ls, &dz, u.dec.data(), u.scores.data(), u.loss.data(),
                               u.grad.data(), nullptr) == SG_OK);
        Call s(2, 9999, {9999, 8000}, D, S, K);
        EXPECT(loss_grad(ctx, "B=2 T_max=9999 lengths 9999 8000 loss_grad", s, s.len_dev.data(), s.len_host.data()) == SG_OK);
        EXPECT(hipdouble_live_allocs() == live);  // nothing grew after the largest call
    }

    // ---- the device loop: B = 3 utterances, 2 steps, without and with dither (EOT repeats as rows of one pass, and in groups)
    {
        Call a(3, 16001, {16001, 9999, 5043}, D, S, K);
        pp.dither.dither = 0.f; pp.eot_size = 2; pp.eot_batch_size = 2;
        EXPECT(pgd(ctx, "pgd_run B=3 T_max=16001 lengths 16001 9999 5043 2 steps dither 0 (eot 2 asked: one pass)", a, a.len_dev.data(),
                   a.len_host.data()) == SG_OK);
        pp.dither.dither = 1.0f;
        EXPECT(pgd(ctx, "pgd_run B=3 T_max=16001 lengths 16001 9999 5043 2 steps dither 1 eot 2 one group", a, a.len_dev.data(),
                   a.len_host.data()) == SG_OK);
        setenv("SG_EOT_MAX_ROWS", "3", 1);
        EXPECT(pgd(ctx, "pgd_run B=3 T_max=16001 lengths 16001 9999 5043 2 steps dither 1 eot 2 max_rows 3: one repeat per pass", a,
                   a.len_dev.data(), a.len_host.data()) == SG_OK);
        unsetenv("SG_EOT_MAX_ROWS");
        pp.eot_size = 1; pp.eot_batch_size = 1;
        pp.max_iter = 0;  // only the final pass
        EXPECT(pgd(ctx, "pgd_run B=3 T_max=16001 lengths 16001 9999 5043 max_iter 0", a, a.len_dev.data(), a.len_host.data()) == SG_OK);
        pp.max_iter = K;
        // a batch large enough for the four-sample overlap-add (B T_max >= 768000, T_max % 4 == 0)
        pp.dither.dither = 0.f;
        Call q(12, 67200, {67200, 9999, 9998, 66001, 16000, 33333, 67200, 8000, 48000, 66001, 9999, 51200}, D, S, K);
        EXPECT(pgd(ctx, "pgd_run B=12 T_max=67200 2 steps dither 0", q, q.len_dev.data(), q.len_host.data()) == SG_OK);
        g_label = "uniform pgd_run B=3 T=16001 2 steps dither 0"; g_n = 0;
        EXPECT(sg_xv_pgd_run(ctx, a.x.data(), a.y.data(), a.lower.data(), a.upper.data(), 3, 16001, &pp, a.succ.data(), a.dec.data(), a.scores.data(),
                             a.loss.data(), a.ltr.data(), a.dtr.data(), nullptr) == SG_OK);
    }

    // ---- two contexts side by side
    {
        sg_ctx* other = nullptr;
        EXPECT(sg_create(0, &other) == SG_OK && other != nullptr);
        if (other) {
            EXPECT(sg_xv_load(other, &xv.desc) == SG_OK);
            Call a(2, 9999, {8000, 9999}, D, S, K), b(3, 16001, {16001, 9999, 5043}, D, S, K);
            EXPECT(loss_grad(other, "second context B=2 T_max=9999 loss_grad", a, a.len_dev.data(), a.len_host.data()) == SG_OK);
            EXPECT(loss_grad(ctx, "first context B=3 T_max=16001 loss_grad, the second one live", b, b.len_dev.data(), b.len_host.data()) == SG_OK);
            std::vector<int32_t> wrong = {8000, 9998};
            EXPECT(sg_xv_forward_ragged(other, a.x.data(), wrong.data(), wrong.data(), 2, 9999, &dz, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                   SG_ERR_ARG);
            EXPECT(std::string(sg_last_error(other)).find("no utterance has T_max = 9999") != std::string::npos);
            EXPECT(std::string(sg_last_error(ctx)).find("T_max = 9999") == std::string::npos);  // (error texts are per context)
            sg_destroy(other);
        }
    }

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "ragged_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
