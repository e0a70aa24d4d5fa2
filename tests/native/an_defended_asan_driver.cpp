// Third driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp, abi_asan_driver.cpp and
// defended_asan_driver.cpp): walks sg_an_pgd_run_defended -- refusals before any launch, workspace growth, the stage / key /
// buffer bookkeeping of every pass, repeat groups with a carried sum, the chain in front of FeCo -- under AddressSanitizer +
// UBSan.  "Device" buffers are host buffers sized exactly as the header says.  No kernel runs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "speakerguard_hip.h"

extern "C" long hipdouble_launches();

static int g_fail = 0;
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_fail;                                                                \
        }                                                                            \
    } while (0)

static std::vector<float> rnd(size_t n, unsigned seed, float scale = 0.1f, float shift = 0.f) {
    std::vector<float> v(n);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        v[i] = shift + scale * ((float)(s >> 8) / 8388608.0f - 1.0f);
    }
    return v;
}

struct AnModel {
    std::vector<float> c1w, c1b, bn1[4], cw[7], cb[7], g[7], be[7], mu[7], va[7], fcw, fcb;
    sg_an_weights desc{};
    explicit AnModel(int S) {
        const int cin[7] = {32, 64, 128, 128, 128, 128, 64}, cout[7] = {64, 128, 128, 128, 128, 64, 32};
        c1w = rnd(25, 50); c1b = rnd(1, 51);
        for (int i = 0; i < 4; ++i) { bn1[i] = rnd(1, 52 + i, 0.1f, i == 3 || i == 0 ? 1.f : 0.f); desc.bn1[i] = bn1[i].data(); }
        desc.conv1_weight = c1w.data(); desc.conv1_bias = c1b.data();
        for (int l = 0; l < 7; ++l) {
            cw[l] = rnd((size_t)cout[l] * cin[l] * 3, 60 + l); cb[l] = rnd(cout[l], 70 + l); g[l] = rnd(cout[l], 80 + l, 0.1f, 1.f);
            be[l] = rnd(cout[l], 90 + l); mu[l] = rnd(cout[l], 100 + l); va[l] = rnd(cout[l], 110 + l, 0.3f, 1.f);
            desc.conv_weight[l] = cw[l].data(); desc.conv_bias[l] = cb[l].data(); desc.bn_weight[l] = g[l].data();
            desc.bn_bias[l] = be[l].data(); desc.bn_mean[l] = mu[l].data(); desc.bn_var[l] = va[l].data();
        }
        fcw = rnd((size_t)S * 32, 120); fcb = rnd(S, 121);
        desc.fc_weight = fcw.data(); desc.fc_bias = fcb.data(); desc.num_class = S; desc.bn_eps = 1e-5f;
    }
};

static sg_wav_stage td(int kind, float param) {
    sg_wav_stage st{};
    st.tag = SG_WAV_STAGE_DEFENSE;
    st.u.defense.kind = kind;
    st.u.defense.param = param;
    return st;
}

int main() {
    setenv("SG_TUNE", "1", 1);
    const int B = 3, K = 2;
    std::vector<int64_t> y(B, 1), dec(B);
    std::vector<uint8_t> succ(B);
    const double sos[2][6] = {{0.2, 0.4, 0.2, 1.0, -0.3, 0.1}, {1.0, 2.0, 1.0, 1.0, -0.2, 0.3}};
    sg_wav_stage lpf{};
    lpf.tag = SG_WAV_STAGE_FILTER;
    lpf.u.filter.n_sections = 2; lpf.u.filter.sos = &sos[0][0]; lpf.u.filter.clip_mode = SG_FD_CLIP_RANGE; lpf.u.filter.bits = 16;
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
