// Third driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp, abi_asan_driver.cpp and
// defended_asan_driver.cpp): walks sg_an_pgd_run_defended -- refusals before any launch, workspace growth, the stage / key /
// buffer bookkeeping of every pass, repeat groups with a carried sum, the chain in front of FeCo -- under AddressSanitizer +
// UBSan.  "Device" buffers are host buffers sized exactly as the header says.  No kernel runs.
#include "driver_common.h"

int main() {
    setenv("SG_TUNE", "1", 1);
    const int B = 3, K = 2;
    std::vector<int64_t> y(B, 1), dec(B);
    std::vector<uint8_t> succ(B);
    const sg_wav_stage lpf = lpf_stage();
    sg_wav_stage one = td(SG_TD_AS, 3.f), bad = one;
    std::vector<sg_wav_stage> nine(SG_WAV_CHAIN_MAX + 1, one);
    sg_wav_stage qt2[2] = {td(SG_TD_QT, 128.f), td(SG_TD_QT, 256.f)};
    sg_wav_stage full[SG_WAV_CHAIN_MAX] = {td(SG_TD_MS, 5.f), td(SG_TD_AS, 31.f), td(SG_TD_QT, 256.f), lpf,
                                           td(SG_TD_AT, 25.f), td(SG_TD_QT, 128.f), td(SG_TD_MS, 3.f), lpf};
    {
        sg_ctx* an_ctx = nullptr;
        EXPECT(sg_create(0, &an_ctx) == SG_OK && an_ctx != nullptr);
        if (!an_ctx) return 1;
        const int Ta = 10081, Sa = 5;  // 64 log-mel frames: FeCo's k = 32 passes the stack
        AnModel an(Sa);
        EXPECT(sg_an_load(an_ctx, &an.desc) == SG_OK);
        std::vector<float> xa = rnd((size_t)B * Ta, 201, 0.3f), lo = xa, hi = xa, sc((size_t)B * Sa), ls(B), lt((size_t)(K + 1) * B);
        std::vector<int64_t> dt((size_t)(K + 1) * B);
        sg_pgd_params pa{};
        pa.step_size = 4e-4f; pa.max_iter = K; pa.grad_sign = 1; pa.eot_size = 4; pa.eot_batch_size = 2;
        sg_feco_params fp{};
        fp.k = 32; fp.max_iter = 3; fp.random_init = 1; fp.seed = 5;
        auto run_an = [&](const sg_wav_stage* chain, int n, const sg_feco_params* f, bool trace, int rows = B) {
            return sg_an_pgd_run_defended(an_ctx, xa.data(), y.data(), lo.data(), hi.data(), rows, Ta, &pa, chain, n, f, succ.data(), dec.data(),
                                          sc.data(), ls.data(), trace ? lt.data() : nullptr, trace ? dt.data() : nullptr, nullptr);
        };
        const long l1 = hipdouble_launches();
        sg_wav_stage at = td(SG_TD_AT, 25.f), as_at[2] = {one, at};
        EXPECT(run_an(&one, 0, nullptr, false) == SG_ERR_ARG);
        EXPECT(run_an(nine.data(), SG_WAV_CHAIN_MAX + 1, nullptr, false) == SG_ERR_ARG);
        bad = one; bad.tag = 7;
        EXPECT(run_an(&bad, 1, nullptr, false) == SG_ERR_ARG);
        bad = at; bad.u.defense.noise_dev = xa.data();
        EXPECT(run_an(&bad, 1, nullptr, false) == SG_ERR_ARG);
        pa.eot_size = 3;
        EXPECT(run_an(&one, 1, nullptr, false) == SG_ERR_ARG);
        pa.eot_size = 4;
        EXPECT(run_an(as_at, 2, &fp, false) == SG_ERR_ARG);     // AT in front of FeCo
        EXPECT(run_an(&one, 1, &fp, false, 1) == SG_ERR_ARG);   // FeCo with one utterance
        EXPECT(std::strlen(sg_last_error(an_ctx)) > 0);
        EXPECT(hipdouble_launches() == l1);
        fp.k = 16;
        EXPECT(run_an(&one, 1, &fp, false) == SG_ERR_ARG);      // too few cluster frames for the stack
        fp.k = 32;
        EXPECT(run_an(&one, 1, nullptr, true) == SG_OK);
        EXPECT(run_an(qt2, 2, nullptr, true) == SG_OK);         // identity backward: the waveform ping-pong
        EXPECT(run_an(full, SG_WAV_CHAIN_MAX, nullptr, true) == SG_OK);  // AT: 4 repeats as rows of one pass
        for (const char* rows : {"6", "3"}) {                   // ... as two groups, as one repeat per pass
            setenv("SG_EOT_MAX_ROWS", rows, 1);
            EXPECT(run_an(full, SG_WAV_CHAIN_MAX, nullptr, true) == SG_OK);
            EXPECT(run_an(full + 3, 2, nullptr, false) == SG_OK);
        }
        pa.eot_size = 3; pa.eot_batch_size = 3;
        setenv("SG_EOT_MAX_ROWS", "6", 1);                      // a last, smaller group
        EXPECT(run_an(as_at, 2, nullptr, true) == SG_OK);
        unsetenv("SG_EOT_MAX_ROWS");
        pa.eot_size = 4; pa.eot_batch_size = 2;
        EXPECT(run_an(&one, 1, &fp, true) == SG_OK);            // chain + FeCo, 4 clusterings per step
        EXPECT(run_an(qt2, 2, &fp, true) == SG_OK);
        sg_wav_stage det[3] = {td(SG_TD_MS, 5.f), lpf, td(SG_TD_QT, 128.f)};
        fp.random_init = 0;
        EXPECT(run_an(det, 3, &fp, false) == SG_OK);
        pa.max_iter = 0;  // only the final pass
        EXPECT(run_an(full, SG_WAV_CHAIN_MAX, nullptr, false) == SG_OK);
        EXPECT(run_an(det, 3, &fp, true) == SG_OK);
        sg_destroy(an_ctx);
    }

    if (g_fail) return 1;
    std::printf("an_defended_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
