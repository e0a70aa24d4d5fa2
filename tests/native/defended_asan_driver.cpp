// Second driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and
// abi_asan_driver.cpp): walks sg_xv_pgd_run_defended and sg_wav_rep_sum_update -- refusals, workspace growth, the
// stage / key / buffer bookkeeping of every pass -- under AddressSanitizer + UBSan.  "Device" buffers are host buffers
// sized exactly as the header says; the double's copies are real, so a replicated iterate or a label copy past an extent is
// an ASan error here.  No kernel runs.
#include "driver_common.h"

int main() {
    setenv("SG_TUNE", "1", 1);
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int B = 3, T = 5043, D = 24, S = 4, K = 2;
    XvModel xv(D, S);
    EXPECT(sg_xv_load(ctx, &xv.desc) == SG_OK);
    std::vector<float> x = rnd((size_t)B * T, 200, 0.3f), lower = x, upper = x, scores((size_t)B * S), loss(B), ltr((size_t)(K + 1) * B);
    std::vector<int64_t> y(B, 1), dec(B), dtr((size_t)(K + 1) * B);
    std::vector<uint8_t> succ(B);
    sg_pgd_params pp{};
    pp.step_size = 4e-4f; pp.max_iter = K; pp.grad_sign = 1; pp.eot_size = 4; pp.eot_batch_size = 2;
    const double bad_sos[1][6] = {{1.0, 0.0, 0.0, 1.0, -2.5, 1.0}};
    const sg_wav_stage lpf = lpf_stage();
    auto run = [&](const sg_wav_stage* chain, int n, bool trace) {
        return sg_xv_pgd_run_defended(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, chain, n, succ.data(), dec.data(),
                                      scores.data(), loss.data(), trace ? ltr.data() : nullptr, trace ? dtr.data() : nullptr, nullptr);
    };

    // ---- refusals: before any launch
    const long l0 = hipdouble_launches();
    sg_wav_stage one = td(SG_TD_AS, 3.f);
    EXPECT(sg_xv_pgd_run_defended(nullptr, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, &one, 1, succ.data(), dec.data(),
                                  scores.data(), loss.data(), nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(run(nullptr, 1, false) == SG_ERR_ARG);
    EXPECT(run(&one, 0, false) == SG_ERR_ARG);
    std::vector<sg_wav_stage> nine(SG_WAV_CHAIN_MAX + 1, one);
    EXPECT(run(nine.data(), SG_WAV_CHAIN_MAX + 1, false) == SG_ERR_ARG);
    sg_wav_stage bad = one;
    bad.tag = 7;
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    bad = td(SG_TD_AS, 4.f);
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    bad = td(SG_TD_MS, 33.f);
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    bad = td(SG_TD_QT, 0.f);
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    bad = td(9, 1.f);
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    bad = td(SG_TD_AT, 25.f);
    bad.u.defense.noise_dev = x.data();
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    bad = lpf;
    bad.u.filter.sos = &bad_sos[0][0]; bad.u.filter.n_sections = 1;
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    bad = lpf;
    bad.u.filter.sos = nullptr;
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    bad = lpf;
    bad.u.filter.clip_mode = 5;
    EXPECT(run(&bad, 1, false) == SG_ERR_ARG);
    EXPECT(std::strlen(sg_last_error(ctx)) > 0);
    EXPECT(hipdouble_launches() == l0);

    // ---- valid chains: deterministic, identity-backward only, randomised with repeats (one group, two groups, one repeat per pass)
    sg_wav_stage full[SG_WAV_CHAIN_MAX] = {td(SG_TD_MS, 5.f), td(SG_TD_AS, 31.f), td(SG_TD_QT, 256.f), lpf,
                                           td(SG_TD_AT, 25.f), td(SG_TD_QT, 128.f), td(SG_TD_MS, 3.f), lpf};
    EXPECT(run(&one, 1, false) == SG_OK);
    sg_wav_stage qt2[2] = {td(SG_TD_QT, 128.f), td(SG_TD_QT, 256.f)};
    EXPECT(run(qt2, 2, true) == SG_OK);
    pp.dither.dither = 1.0f; pp.dither.seed = 99; pp.dither.index_base = 5;
    EXPECT(run(qt2, 2, true) == SG_OK);   // repeats through the dither: the identity chain keeps the shared-row pass
    EXPECT(run(&lpf, 1, true) == SG_OK);  // ... and a non-identity one runs every repeat as its own row
    pp.dither.dither = 0.f;
    EXPECT(run(full, SG_WAV_CHAIN_MAX, true) == SG_OK);  // grows the workspace: 8 outputs, 4 int8 planes, 12 rows
    for (const char* rows : {"6", "3"}) {
        setenv("SG_EOT_MAX_ROWS", rows, 1);
        EXPECT(run(full, SG_WAV_CHAIN_MAX, true) == SG_OK);
        EXPECT(run(full + 3, 2, false) == SG_OK);
    }
    unsetenv("SG_EOT_MAX_ROWS");
    EXPECT(sg_trace_begin(ctx, 4096) == SG_OK);
    EXPECT(run(full + 1, 4, true) == SG_OK);
    std::vector<int32_t> tags(4096);
    std::vector<float> ms(4096);
    int32_t n_rec = 0;
    EXPECT(sg_trace_end(ctx, tags.data(), ms.data(), 4096, &n_rec) == SG_OK && n_rec > 60);
    bool seen[4] = {false, false, false, false};
    for (int i = 0; i < n_rec; ++i)
        if (tags[i] >= SG_STAGE_TD_FWD && tags[i] <= SG_STAGE_DEF_REP_SUM) seen[tags[i] >= SG_STAGE_DEF_SCALE ? tags[i] - SG_STAGE_DEF_SCALE + 1 : 0] = true;
    EXPECT(seen[0] && seen[1] && seen[2] && seen[3]);
    pp.max_iter = 0;  // only the final pass
    EXPECT(run(full, SG_WAV_CHAIN_MAX, false) == SG_OK);

    // ---- the repeat-summing update on caller buffers
    const int64_t n = (int64_t)B * T;
    std::vector<float> planes = rnd((size_t)3 * n, 7), carry = rnd((size_t)n, 8), sum((size_t)n);
    EXPECT(sg_wav_rep_sum_update(ctx, planes.data(), 3, n, carry.data(), sum.data(), nullptr, nullptr, nullptr, 0.f, 1, nullptr) == SG_OK);
    EXPECT(sg_wav_rep_sum_update(ctx, planes.data(), 3, n, nullptr, nullptr, x.data(), lower.data(), upper.data(), 4e-4f, -1, nullptr) == SG_OK);
    EXPECT(sg_wav_rep_sum_update(ctx, planes.data(), 0, n, nullptr, sum.data(), nullptr, nullptr, nullptr, 0.f, 1, nullptr) == SG_ERR_ARG);
    EXPECT(sg_wav_rep_sum_update(ctx, planes.data(), 3, n, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 1, nullptr) == SG_ERR_ARG);
    EXPECT(sg_wav_rep_sum_update(ctx, planes.data(), 3, n, nullptr, nullptr, x.data(), nullptr, upper.data(), 0.f, 1, nullptr) == SG_ERR_ARG);
    EXPECT(sg_wav_rep_sum_update(ctx, nullptr, 3, n, nullptr, sum.data(), nullptr, nullptr, nullptr, 0.f, 1, nullptr) == SG_ERR_ARG);

    sg_destroy(ctx);
    if (g_fail) return 1;
    std::printf("defended_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
