// Sixth driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks sg_wav_resample_forward / _backward under AddressSanitizer + UBSan -- every refusal (SG_ERR_ARG before the first launch),
// the table builder (the backward's sorted pair lists included) for ratios 1:2, 3:10 and 33:100, the content-keyed table cache
// (a hit allocates nothing, 32 tables stay, the 33rd replaces the oldest) and the grid and dynamic LDS of both launches.
// "Device" buffers are host buffers sized exactly as the header says.  No kernel runs.
#include <limits>

#include "driver_common.h"

// one stage of a down-/up-sampler between rates in the ratio in_unit : out_unit: windows and weights of the right shape (a
// triangle: the walk is about extents, not about audio), exactly sized
struct Stage {
    std::vector<int32_t> first;
    std::vector<float> weight;
    sg_resample_stage spec{};
    Stage(int in_unit, int out_unit, int W, float salt = 0.f) : first(out_unit), weight((size_t)out_unit * W) {
        for (int p = 0; p < out_unit; ++p) {
            first[p] = (int)std::ceil((double)p * in_unit / out_unit - 0.5 * W);
            for (int j = 0; j < W; ++j) weight[(size_t)p * W + j] = (1.f + salt) / (1.f + std::fabs((float)j - 0.5f * W));
        }
        spec.in_unit = in_unit, spec.out_unit = out_unit, spec.W = W;
        spec.first = first.data(), spec.weight = weight.data();
    }
};
static int64_t out_len(int64_t n, int iu, int ou) { return (n * ou + iu - 1) / iu; }

int main() {
    hipdouble_set_launch_hook(record_launch);
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int BMAX = 3, TMAX = 5001;
    std::vector<float> x((size_t)BMAX * TMAX, 0.25f), y((size_t)BMAX * (TMAX + 200)), gx((size_t)BMAX * TMAX);

    Stage down(2, 1, 25), up(1, 2, 13);
    sg_wav_resample r{};
    r.down = down.spec, r.up = up.spec, r.same_size = 1;
    auto fwd = [&](const sg_wav_resample* s, const float* xi, int B, int T, float* out, int N) {
        return sg_wav_resample_forward(ctx, s, xi, B, T, out, N, nullptr);
    };
    auto bwd = [&](const sg_wav_resample* s, const float* g, int B, int T, int N, float* o) {
        return sg_wav_resample_backward(ctx, s, g, B, T, N, o, nullptr);
    };

    // ---- every refusal: nothing is launched, no table is built
    const long l0 = hipdouble_launches(), a0 = hipdouble_live_allocs();
    EXPECT(sg_wav_resample_forward(nullptr, &r, x.data(), 2, 300, y.data(), 300, nullptr) == SG_ERR_ARG);
    EXPECT(fwd(nullptr, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
    EXPECT(fwd(&r, nullptr, 2, 300, y.data(), 300) == SG_ERR_ARG);
    EXPECT(fwd(&r, x.data(), 2, 300, nullptr, 300) == SG_ERR_ARG);
    EXPECT(bwd(&r, nullptr, 2, 300, 300, gx.data()) == SG_ERR_ARG);
    EXPECT(bwd(&r, y.data(), 2, 300, 300, nullptr) == SG_ERR_ARG);
    for (int B : {0, -1}) EXPECT(fwd(&r, x.data(), B, 300, y.data(), 300) == SG_ERR_ARG);
    for (int T : {0, -5, (1 << 30) + 1}) EXPECT(fwd(&r, x.data(), 2, T, y.data(), T) == SG_ERR_ARG);
    EXPECT(fwd(&r, x.data(), 2, 301, y.data(), 302) == SG_ERR_ARG);  // same_size: the row is T long
    EXPECT(bwd(&r, y.data(), 2, 301, 300, gx.data()) == SG_ERR_ARG);
    {
        sg_wav_resample bad = r;
        bad.same_size = 2;
        EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        bad = r, bad.same_size = 0;
        EXPECT(fwd(&bad, x.data(), 2, 301, y.data(), 301) == SG_ERR_ARG);  // the up-sampler's own length is 302
        bad = r, bad.down.first = nullptr;
        EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        bad = r, bad.up.weight = nullptr;
        EXPECT(bwd(&bad, y.data(), 2, 300, 300, gx.data()) == SG_ERR_ARG);
        for (int v : {0, -1, 1025}) {
            bad = r, bad.down.in_unit = v;
            EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
            bad = r, bad.up.out_unit = v;  // (checked before first / weight are read past their extent)
            EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        }
        bad = r, bad.up.W = 0;
        EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        Stage wide(3, 100, 21);  // 2100 entries: past the table bound
        bad = r, bad.up = wide.spec;
        EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        EXPECT(std::string(sg_last_error(ctx)).find("2048") != std::string::npos);
        for (float v : {std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) {
            Stage nf(1, 2, 13);
            nf.weight[17] = v;
            bad = r, bad.up = nf.spec;
            EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        }
        Stage late(2, 1, 25);
        late.first[0] = 1;  // phase 0 cannot reach its own output
        bad = r, bad.down = late.spec;
        EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        late.first[0] = (1 << 20) + 1;
        EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        late.first[0] = -(1 << 20) - 1;
        EXPECT(fwd(&bad, x.data(), 2, 300, y.data(), 300) == SG_ERR_ARG);
        // tables within the bound whose tile does not fit a block's LDS: 1 : 1024 with a 2-tap window
        Stage blow_down(1, 1024, 2), blow_up(1024, 1, 2048);
        bad = r, bad.down = blow_down.spec, bad.up = blow_up.spec;
        EXPECT(fwd(&bad, x.data(), 1, 8, y.data(), 8) == SG_ERR_ARG);
    }
    EXPECT(hipdouble_launches() == l0 && sg_last_error(ctx)[0] != 0);

    EXPECT(hipdouble_live_allocs() == a0);

    // ---- what runs: three ratios, both directions, same_size 0 / 1, T below, at and past a tile, B 1 and 3
    struct Ratio { int iu, ou, Wd, Wu; };
    const Ratio ratios[] = {{2, 1, 25, 13}, {10, 3, 41, 13}, {100, 33, 37, 13}};
    for (const Ratio& q : ratios) {
        Stage d(q.iu, q.ou, q.Wd), u(q.ou, q.iu, q.Wu);
        sg_wav_resample s{};
        s.down = d.spec, s.up = u.spec;
        const int tile_f = (2048 / q.iu > 0 ? 2048 / q.iu : 1) * q.iu;  // Up's out_unit = Down's in_unit: both tiles
        for (int same : {1, 0})
            for (int T : {1, 13, tile_f, tile_f + 1, TMAX})
                for (int B : {1, BMAX}) {
                    s.same_size = same;
                    const int n_low = (int)out_len(T, q.iu, q.ou), n_up = (int)out_len(n_low, q.ou, q.iu), N = same ? T : n_up;
                    EXPECT(n_up >= T && N <= TMAX + 200);
                    g_seen.clear();
                    const long live = hipdouble_live_allocs();
                    EXPECT(fwd(&s, x.data(), B, T, y.data(), N) == SG_OK);
                    EXPECT(bwd(&s, y.data(), B, T, N, gx.data()) == SG_OK);
                    EXPECT(g_seen.size() == 2);
                    if (g_seen.size() != 2) continue;
                    EXPECT(g_seen[0].name.find("rs_forward_kernel") != std::string::npos);
                    EXPECT(g_seen[1].name.find("rs_backward_kernel") != std::string::npos);
                    EXPECT(g_seen[0].grid.x == (unsigned)(B * ((N + tile_f - 1) / tile_f)) && g_seen[0].block.x == 512);
                    EXPECT(g_seen[1].grid.x == (unsigned)(B * ((T + tile_f - 1) / tile_f)) && g_seen[1].block.x == 512);
                    EXPECT(g_seen[0].lds > 0 && g_seen[0].lds <= 64 * 1024 && g_seen[1].lds > 0 && g_seen[1].lds <= 64 * 1024);
                    // only the ratio's first call allocates (its tables)
                    EXPECT(hipdouble_live_allocs() == live + (same == 1 && T == 1 && B == 1 ? 1 : 0));
                }
    }

    // ---- the cache is keyed by content: another copy of the same tables hits, one changed weight misses; it holds 32
    {
        Stage d2(2, 1, 25), u2(1, 2, 13);
        sg_wav_resample s{};
        s.down = d2.spec, s.up = u2.spec, s.same_size = 1;
        long live = hipdouble_live_allocs();
        EXPECT(fwd(&s, x.data(), 1, 300, y.data(), 300) == SG_OK && hipdouble_live_allocs() == live);
        u2.weight[3] *= 1.5f;
        EXPECT(fwd(&s, x.data(), 1, 300, y.data(), 300) == SG_OK && hipdouble_live_allocs() == live + 1);
        for (int k = 0; k < 40; ++k) {
            Stage dk(2, 1, 25, 0.01f * (float)(k + 1));
            s.down = dk.spec;
            EXPECT(bwd(&s, y.data(), 1, 300, 300, gx.data()) == SG_OK);
        }
        EXPECT(hipdouble_live_allocs() == live - 3 + 32);  // (the three ratios' tables were held before this block's `live`)
    }

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "ds_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
