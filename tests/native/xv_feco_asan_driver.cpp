// Fourth driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks sg_xv_pgd_run_feco under AddressSanitizer + UBSan and prints one line per kernel launch, in order -- kernel name with
// template arguments, grid, block, dynamic LDS -- for tests/test_xv_feco_launch_sequence.py, which compares the output with
// tests/native/xv_feco_launch_sequence.expected.  Every refusal leaves one line with its return code and must come before the
// first launch.  "Device" buffers are host buffers sized exactly as the header says; the double's copies are real.  No kernel runs.
#include "driver_common.h"

static std::string g_label;
static int g_n = 0;
static void print_line(const Launch& l, void**) {
    print_launch(g_label, ++g_n, l);
    std::printf("\n");
}

int main() {
    setenv("SG_TUNE", "1", 1);  // SG_EOT_MAX_ROWS counts, where a case sets it
    unsetenv("SG_EOT_MAX_ROWS");
    g_on_launch = print_line;
    hipdouble_set_launch_hook(record_launch);
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int B = 3, T = 16001, F = sg_xv_num_frames(T), D = 24, S = 4, K = 2, REPS = 5;
    XvModel xv(D, S);
    EXPECT(sg_xv_load(ctx, &xv.desc) == SG_OK);
    std::vector<float> x = rnd((size_t)B * T, 200, 0.3f), lower = x, upper = x, scores((size_t)B * S), loss(B), ltr((size_t)(K + 1) * B);
    std::vector<int64_t> y(B, 1), dec(B), dtr((size_t)(K + 1) * B);
    std::vector<uint8_t> succ(B);
    sg_pgd_params pp{};
    pp.step_size = 4e-4f; pp.max_iter = K; pp.grad_sign = 1; pp.eot_size = 1; pp.eot_batch_size = 1;
    pp.dither.seed = 99; pp.dither.index_base = 5;
    sg_feco_params fp{};
    fp.k = F / 2; fp.max_iter = 10; fp.seed = 7; fp.index_base = 5;
    auto run = [&](const std::string& label, int level, int b = 3, int t = 16001) {
        g_label = label;
        g_n = 0;
        const int rc = sg_xv_pgd_run_feco(ctx, x.data(), y.data(), lower.data(), upper.data(), b, t, &pp, &fp, level, succ.data(), dec.data(),
                                          scores.data(), loss.data(), ltr.data(), dtr.data(), nullptr);
        if (rc != SG_OK) std::printf("%s | rc=%d %s\n", label.c_str(), rc, sg_last_error(ctx));
        return rc;
    };

    // ---- every refusal: SG_ERR_ARG before the first launch (and before the workspace is touched)
    const long l0 = hipdouble_launches();
    g_label = "refused: feco NULL";
    EXPECT(sg_xv_pgd_run_feco(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, nullptr, 1, succ.data(), dec.data(), scores.data(),
                              loss.data(), nullptr, nullptr, nullptr) == SG_ERR_ARG);
    std::printf("%s | rc=%d %s\n", g_label.c_str(), SG_ERR_ARG, sg_last_error(ctx));
    EXPECT(run("refused: level 0", 0) == SG_ERR_ARG);
    EXPECT(run("refused: level 3", 3) == SG_ERR_ARG);
    EXPECT(run("refused: B 1", 1, 1) == SG_ERR_ARG);
    fp.k = 0;
    EXPECT(run("refused: k 0", 1) == SG_ERR_ARG);
    fp.k = F + 1;
    EXPECT(run("refused: k F+1", 2) == SG_ERR_ARG);
    fp.k = 31;  // tdnn1 .. tdnn3 take 30 frames of context and the pooling needs two
    EXPECT(run("refused: k 31 below the TDNN context", 1) == SG_ERR_ARG);
    fp.k = F / 2;
    fp.max_iter = 0;
    EXPECT(run("refused: FeCo max_iter 0", 1) == SG_ERR_ARG);
    fp.max_iter = 10;
    fp.k = 2500;  // 50 s: the clustering of one utterance no longer fits a block's LDS
    EXPECT(run("refused: F 5000 k 2500 past the k-means kernel's LDS", 1, 2, 800000) == SG_ERR_ARG);
    fp.k = F / 2;
    pp.eot_size = 4; pp.eot_batch_size = 3;
    EXPECT(run("refused: eot 4 in batches of 3", 1) == SG_ERR_ARG);
    pp.eot_size = 1; pp.eot_batch_size = 1;
    fp.k = 150;
    EXPECT(run("refused: 3000 x 48000 past the 2 GiB activation bound", 2, 3000, 48000) == SG_ERR_ARG);
    fp.k = F / 2;
    pp.max_iter = -1;
    EXPECT(run("refused: max_iter -1", 1) == SG_ERR_ARG);
    pp.max_iter = K;
    EXPECT(hipdouble_launches() == l0);

    // ---- the pass forms, at both levels
    for (int level = 1; level <= 2; ++level) {
        const std::string at = "level " + std::to_string(level) + " B=3 T=16001 k=" + std::to_string(fp.k);
        pp.dither.dither = 0.f; fp.random_init = 0; pp.eot_size = REPS; pp.eot_batch_size = REPS;
        EXPECT(run(at + " deterministic (eot 5 asked: one pass)", level) == SG_OK);
        fp.random_init = 1;
        EXPECT(run(at + " dither 0 random eot 5 one group", level) == SG_OK);
        setenv("SG_EOT_MAX_ROWS", "6", 1);
        EXPECT(run(at + " dither 0 random eot 5 max_rows 6: groups 2 2 1", level) == SG_OK);
        unsetenv("SG_EOT_MAX_ROWS");
        pp.dither.dither = 1.0f;
        EXPECT(run(at + " dither 1 random eot 5 one group", level) == SG_OK);
        fp.random_init = 0;
        EXPECT(run(at + " dither 1 even eot 5 one group", level) == SG_OK);
        fp.random_init = 1;
        setenv("SG_EOT_MAX_ROWS", "6", 1);
        EXPECT(run(at + " dither 1 random eot 5 max_rows 6: groups 2 2 1", level) == SG_OK);
        setenv("SG_EOT_MAX_ROWS", "3", 1);
        EXPECT(run(at + " dither 1 random eot 5 max_rows 3: one repeat per pass", level) == SG_OK);
        unsetenv("SG_EOT_MAX_ROWS");
        pp.max_iter = 0;  // only the final pass
        EXPECT(run(at + " dither 1 random max_iter 0", level) == SG_OK);
        pp.max_iter = K;
    }
    // the stage trace names the new launches
    pp.dither.dither = 1.0f; fp.random_init = 1; pp.eot_size = 2; pp.eot_batch_size = 2;
    EXPECT(sg_trace_begin(ctx, 4096) == SG_OK);
    EXPECT(run("level 2 traced", 2) == SG_OK);
    std::vector<int32_t> tags(4096);
    std::vector<float> ms(4096);
    int32_t n_rec = 0;
    EXPECT(sg_trace_end(ctx, tags.data(), ms.data(), 4096, &n_rec) == SG_OK && n_rec > 40);
    int seen[3] = {0, 0, 0};
    for (int i = 0; i < n_rec; ++i)
        if (tags[i] >= SG_STAGE_XV_FECO_FWD && tags[i] <= SG_STAGE_XV_FECO_COLS) ++seen[tags[i] - SG_STAGE_XV_FECO_FWD];
    EXPECT(seen[0] == K + 1 && seen[1] == K && seen[2] == 2 * K + 1);

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "xv_feco_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
