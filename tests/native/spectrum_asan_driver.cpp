// Seventh driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks sg_wav_spectrum / sg_wav_spectrum_gate under AddressSanitizer + UBSan -- every refusal (SG_ERR_ARG before the first
// launch, nothing allocated), one accepted call per route (both buffers in LDS, the workspace, Bluestein on either), the plan's
// launch geometry and dynamic LDS, the float64 table builder (Bluestein's transformed chirp included), the per-T table cache (a
// hit allocates nothing, 16 tables stay, the 17th replaces the oldest) and the workspace (grown only when a call needs more).
// "Device" buffers are host buffers sized exactly as the header says.  No kernel runs.
#include "driver_common.h"

int main() {
    hipdouble_set_launch_hook(record_launch);
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int BMAX = 3, TMAX = 52960;
    std::vector<float> x((size_t)BMAX * TMAX, 0.25f), out((size_t)BMAX * TMAX), spec((size_t)BMAX * (TMAX / 2 + 1) * 2), peak(BMAX),
        factor(BMAX, 1.f);
    std::vector<uint8_t> keep((size_t)BMAX * (TMAX / 2 + 1));
    std::vector<int32_t> kept(BMAX);
    auto sp = [&](const float* xi, int B, int T, float* s, float* p) { return sg_wav_spectrum(ctx, xi, B, T, s, p, nullptr); };
    auto gate = [&](const float* xi, int B, int T, const float* f, float* o, uint8_t* k, int32_t* c) {
        return sg_wav_spectrum_gate(ctx, xi, B, T, f, o, k, c, nullptr);
    };

    // ---- every refusal: nothing is launched, nothing is allocated, no table is built
    const long l0 = hipdouble_launches(), a0 = hipdouble_live_allocs();
    EXPECT(sg_wav_spectrum(nullptr, x.data(), 2, 480, spec.data(), peak.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_wav_spectrum_gate(nullptr, x.data(), 2, 480, factor.data(), out.data(), keep.data(), kept.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sp(nullptr, 2, 480, spec.data(), peak.data()) == SG_ERR_ARG);
    EXPECT(sp(x.data(), 2, 480, nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(gate(nullptr, 2, 480, factor.data(), out.data(), keep.data(), kept.data()) == SG_ERR_ARG);
    EXPECT(gate(x.data(), 2, 480, nullptr, out.data(), keep.data(), kept.data()) == SG_ERR_ARG);
    EXPECT(gate(x.data(), 2, 480, factor.data(), nullptr, keep.data(), kept.data()) == SG_ERR_ARG);
    EXPECT(gate(x.data(), 2, 480, factor.data(), x.data(), keep.data(), kept.data()) == SG_ERR_ARG);  // out aliases x
    for (int B : {0, -1}) {
        EXPECT(sp(x.data(), B, 480, spec.data(), peak.data()) == SG_ERR_ARG);
        EXPECT(gate(x.data(), B, 480, factor.data(), out.data(), nullptr, nullptr) == SG_ERR_ARG);
    }
    for (int T : {0, 1, -2, 3, 481, 52961, (1 << 22) + 2, 0x7FFFFFFE}) {
        EXPECT(sp(x.data(), 1, T, spec.data(), peak.data()) == SG_ERR_ARG);
        EXPECT(gate(x.data(), 1, T, factor.data(), out.data(), nullptr, nullptr) == SG_ERR_ARG);
    }
    EXPECT(hipdouble_launches() == l0 && sg_last_error(ctx)[0] != 0);
    EXPECT(hipdouble_live_allocs() == a0);

    // ---- what runs: one launch per call, one workgroup of 1024 threads per utterance; the route by the network's length
    struct Case { int T, N; bool lds; };  // N: the network's length (M, or Bluestein's power of two)
    const Case cases[] = {{2, 1, true},        {4, 2, true},          {6, 3, true},           {10, 5, true},
                          {14, 16, true},      {480, 240, true},      {662, 1024, true},      {16000, 8000, true},
                          {8190, 8192, true},  {8194, 16384, false},  {20000, 10000, true},   {20480, 10240, false},
                          {48000, 24000, false}, {52960, 65536, false}};
    const long n_cases = (long)(sizeof(cases) / sizeof(cases[0]));
    for (const Case& c : cases)
        for (int B : {1, BMAX}) {
            g_seen.clear();
            EXPECT(sp(x.data(), B, c.T, spec.data(), peak.data()) == SG_OK);
            EXPECT(sp(x.data(), B, c.T, nullptr, peak.data()) == SG_OK);
            EXPECT(sp(x.data(), B, c.T, spec.data(), nullptr) == SG_OK);
            EXPECT(gate(x.data(), B, c.T, factor.data(), out.data(), keep.data(), kept.data()) == SG_OK);
            const long live = hipdouble_live_allocs();
            EXPECT(gate(x.data(), B, c.T, factor.data(), out.data(), nullptr, nullptr) == SG_OK);
            EXPECT(hipdouble_live_allocs() == live);  // nothing allocated after the first call at (B, T)
            EXPECT(g_seen.size() == 5);
            for (const Launch& l : g_seen) {
                EXPECT(l.name.find(c.lds ? "sp_kernel<true>" : "sp_kernel<false>") != std::string::npos);
                EXPECT(l.grid.x == (unsigned)B && l.grid.y == 1 && l.block.x == 1024);
                EXPECT(l.lds == (c.lds ? (size_t)c.N * 16 : 0) && l.lds + 256 <= 160 * 1024);
            }
        }

    // ---- the table cache holds 16 lengths: eight more than the cases' push the oldest out, and a hit allocates nothing
    {
        const long live = hipdouble_live_allocs();
        for (int k = 0; k < 8; ++k) EXPECT(sp(x.data(), 1, 100 + 2 * k, nullptr, peak.data()) == SG_OK);
        EXPECT(n_cases <= 16 && hipdouble_live_allocs() == live + 16 - n_cases);
        EXPECT(sp(x.data(), 1, 114, nullptr, peak.data()) == SG_OK && hipdouble_live_allocs() == live + 16 - n_cases);
        EXPECT(sp(x.data(), 1, 2, nullptr, peak.data()) == SG_OK && hipdouble_live_allocs() == live + 16 - n_cases);  // (left, rebuilt)
    }

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "spectrum_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
