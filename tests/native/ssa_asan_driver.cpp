// Eighth driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks sg_ssa_window / sg_ssa_decompose / sg_ssa_reconstruct under AddressSanitizer + UBSan -- every refusal (SG_ERR_ARG before
// the first launch, nothing allocated), the window of every length class, one accepted call per window parity (odd W: the idle
// index) with the launch sequence and geometry of a sweep, the sweep loop's bookkeeping (no kernel runs: the counters stay zero,
// so every utterance is done after the first sweep and reports 0 sweeps), the ranks travelling as launch arguments in chunks of
// 64, and the workspace (grown only when a call needs more).  "Device" buffers are host buffers sized exactly as the header says.
#include "driver_common.h"

static int count(const char* kernel) {
    int n = 0;
    for (const Launch& l : g_seen) n += kernel_name(l.name) == kernel ? 1 : 0;
    return n;
}
static const Launch* first(const char* kernel) {
    for (const Launch& l : g_seen)
        if (kernel_name(l.name) == kernel) return &l;
    return nullptr;
}

int main() {
    hipdouble_set_launch_hook(record_launch);
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;

    // ---- the window: pure
    const int tw[][2] = {{20, 1}, {39, 1}, {40, 2}, {60, 3}, {100, 5}, {480, 24}, {4000, 200}, {16000, 800}, {48000, 2400},
                         {59999, 2999}, {60000, 3000}, {60020, 3000}, {1 << 22, 3000}};
    for (const auto& c : tw) EXPECT(sg_ssa_window(c[0]) == c[1]);
    for (int T : {19, 1, 0, -1, -2147483647 - 1, (1 << 22) + 1, 2147483647}) EXPECT(sg_ssa_window(T) == -1);

    const int BMAX = 70, TMAX = 480, WMAX = 24;
    std::vector<float> x((size_t)BMAX * TMAX, 0.25f), out((size_t)BMAX * TMAX);
    std::vector<int16_t> xq((size_t)BMAX * TMAX);
    std::vector<double> lam((size_t)BMAX * WMAX), E((size_t)BMAX * WMAX * WMAX), cov((size_t)BMAX * WMAX * WMAX), out64((size_t)BMAX * TMAX);
    std::vector<int32_t> sweeps(BMAX, 7), k(BMAX, 1);
    auto dec = [&](const float* xi, int B, int T, int bits, int16_t* q, double* l, double* e, int32_t* s, double* c) {
        return sg_ssa_decompose(ctx, xi, B, T, bits, q, l, e, s, c, nullptr);
    };
    auto rec = [&](const int16_t* q, const double* e, const int32_t* kk, int B, int T, float* o, double* o64) {
        return sg_ssa_reconstruct(ctx, q, e, kk, B, T, o, o64, nullptr);
    };

    // ---- every refusal: nothing is launched, nothing is allocated
    const long l0 = hipdouble_launches(), a0 = hipdouble_live_allocs();
    EXPECT(sg_ssa_decompose(nullptr, x.data(), 2, 480, 16, xq.data(), lam.data(), E.data(), sweeps.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_ssa_reconstruct(nullptr, xq.data(), E.data(), k.data(), 2, 480, out.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(dec(nullptr, 2, 480, 16, xq.data(), lam.data(), E.data(), sweeps.data(), nullptr) == SG_ERR_ARG);
    EXPECT(dec(x.data(), 2, 480, 16, nullptr, lam.data(), E.data(), sweeps.data(), nullptr) == SG_ERR_ARG);
    EXPECT(dec(x.data(), 2, 480, 16, xq.data(), nullptr, E.data(), sweeps.data(), nullptr) == SG_ERR_ARG);
    EXPECT(dec(x.data(), 2, 480, 16, xq.data(), lam.data(), nullptr, sweeps.data(), nullptr) == SG_ERR_ARG);
    EXPECT(dec(x.data(), 2, 480, 16, xq.data(), lam.data(), E.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(rec(nullptr, E.data(), k.data(), 2, 480, out.data(), nullptr) == SG_ERR_ARG);
    EXPECT(rec(xq.data(), nullptr, k.data(), 2, 480, out.data(), nullptr) == SG_ERR_ARG);
    EXPECT(rec(xq.data(), E.data(), nullptr, 2, 480, out.data(), nullptr) == SG_ERR_ARG);
    EXPECT(rec(xq.data(), E.data(), k.data(), 2, 480, nullptr, out64.data()) == SG_ERR_ARG);
    for (int B : {0, -1, 65536}) {
        EXPECT(dec(x.data(), B, 480, 16, xq.data(), lam.data(), E.data(), sweeps.data(), nullptr) == SG_ERR_ARG);
        EXPECT(rec(xq.data(), E.data(), k.data(), B, 480, out.data(), nullptr) == SG_ERR_ARG);
    }
    for (int T : {19, 1, 0, -20, (1 << 22) + 1, 0x7FFFFFFF}) {
        EXPECT(dec(x.data(), 1, T, 16, xq.data(), lam.data(), E.data(), sweeps.data(), nullptr) == SG_ERR_ARG);
        EXPECT(rec(xq.data(), E.data(), k.data(), 1, T, out.data(), nullptr) == SG_ERR_ARG);
    }
    for (int bits : {0, -1, 17, 32}) EXPECT(dec(x.data(), 1, 480, bits, xq.data(), lam.data(), E.data(), sweeps.data(), nullptr) == SG_ERR_ARG);
    for (int bad : {0, -1, 25, 0x7FFFFFFF}) {  // W = 24; the offender is the LAST rank: all of them are looked at
        std::vector<int32_t> kk{24, 1, bad};
        EXPECT(rec(xq.data(), E.data(), kk.data(), 3, 480, out.data(), nullptr) == SG_ERR_ARG);
    }
    EXPECT(hipdouble_launches() == l0 && sg_last_error(ctx)[0] != 0);
    EXPECT(hipdouble_live_allocs() == a0);

    // ---- what runs.  T -> W: 20 -> 1 (odd: n = 2, the one pair is idle), 40 -> 2, 60 -> 3, 100 -> 5, 480 -> 24
    struct Case { int T, W; };
    for (const Case& c : {Case{20, 1}, Case{40, 2}, Case{60, 3}, Case{100, 5}, Case{480, 24}})
        for (int B : {1, 3, BMAX}) {
            const int n = c.W + (c.W & 1), half = n / 2, tiles = (c.W + 31) / 32;
            g_seen.clear();
            std::fill(sweeps.begin(), sweeps.end(), 7);
            EXPECT(dec(x.data(), B, c.T, 16, xq.data(), lam.data(), E.data(), sweeps.data(), B == 3 ? cov.data() : nullptr) == SG_OK);
            // one sweep (no kernel ran: no rotation was counted), then the ordering and the Newton-Schulz step
            EXPECT((int)g_seen.size() == 3 + 3 * (n - 1) + 5);
            EXPECT(count("ssa_quantise_kernel") == 1 && count("ssa_cov_row_kernel") == 1 && count("ssa_cov_diag_kernel") == 1);
            EXPECT(count("ssa_rot_kernel") == n - 1 && count("ssa_cols_kernel") == n - 1 && count("ssa_rows_kernel") == n - 1);
            EXPECT(count("ssa_rank_kernel") == 1 && count("ssa_atb_kernel") == 2 && count("ssa_transpose_kernel") == 1 &&
                   count("ssa_sort_rows_kernel") == 1);
            for (int b = 0; b < BMAX; ++b) EXPECT(sweeps[b] == (b < B ? 0 : 7));
            const Launch* l;
            EXPECT((l = first("ssa_quantise_kernel")) && l->grid.x == (unsigned)B && l->block.x == 1024);
            EXPECT((l = first("ssa_cov_row_kernel")) && l->grid.x == (unsigned)c.W && l->grid.y == (unsigned)B && l->block.x == 256);
            EXPECT((l = first("ssa_cov_diag_kernel")) && l->grid.x == 1 && l->grid.y == (unsigned)B);
            EXPECT((l = first("ssa_rot_kernel")) && l->grid.x == 1 && l->grid.y == (unsigned)B);
            EXPECT((l = first("ssa_cols_kernel")) && l->grid.x == 2u * c.W && l->grid.y == (unsigned)B && l->block.x == 256);
            EXPECT((l = first("ssa_rows_kernel")) && l->grid.x == (unsigned)half && l->grid.y == (unsigned)B);
            EXPECT((l = first("ssa_atb_kernel")) && l->grid.x == (unsigned)tiles && l->grid.y == (unsigned)tiles && l->grid.z == (unsigned)B &&
                   l->block.x == 16 && l->block.y == 16);
            EXPECT((l = first("ssa_sort_rows_kernel")) && l->grid.x == (unsigned)c.W && l->grid.y == (unsigned)B);
            for (const Launch& s : g_seen) EXPECT(s.lds == 0);

            g_seen.clear();
            for (int b = 0; b < B; ++b) k[b] = 1 + b % c.W;
            const long live = hipdouble_live_allocs();
            EXPECT(rec(xq.data(), E.data(), k.data(), B, c.T, out.data(), out64.data()) == SG_OK);
            EXPECT(rec(xq.data(), E.data(), k.data(), B, c.T, out.data(), nullptr) == SG_OK);
            EXPECT(hipdouble_live_allocs() == live);  // the decomposition's workspace covers the reconstruction's
            const int puts = (B + 63) / 64, edge = c.W > 1 ? 1 : 0;
            EXPECT((int)g_seen.size() == 2 * (puts + 3 + edge));
            EXPECT(count("ssa_put_k_kernel") == 2 * puts && count("ssa_atb_kernel") == 2 && count("ssa_taps_kernel") == 2 &&
                   count("ssa_interior_kernel") == 2 && count("ssa_edge_kernel") == 2 * edge);
            EXPECT((l = first("ssa_taps_kernel")) && l->grid.x == 2u * c.W - 1 && l->grid.y == (unsigned)B && l->block.x == 64);
            EXPECT((l = first("ssa_interior_kernel")) && l->grid.x == (unsigned)((c.T - 2 * c.W + 2 + 255) / 256) && l->grid.y == (unsigned)B);
            if (edge) EXPECT((l = first("ssa_edge_kernel")) && l->grid.x == 2u * (c.W - 1) && l->grid.y == (unsigned)B && l->block.x == 256);
        }

    // ---- a reconstruction before any decomposition of its size grows the workspace once
    {
        const long before = hipdouble_live_allocs();
        sg_ctx* fresh = nullptr;
        EXPECT(sg_create(0, &fresh) == SG_OK && fresh != nullptr);
        if (fresh) {
            const long live = hipdouble_live_allocs();
            EXPECT(sg_ssa_reconstruct(fresh, xq.data(), E.data(), k.data(), 2, 480, out.data(), nullptr, nullptr) == SG_OK);
            EXPECT(hipdouble_live_allocs() == live + 2);
            EXPECT(sg_ssa_reconstruct(fresh, xq.data(), E.data(), k.data(), 1, 100, out.data(), nullptr, nullptr) == SG_OK);
            EXPECT(hipdouble_live_allocs() == live + 2);
            sg_destroy(fresh);
            EXPECT(hipdouble_live_allocs() == before);
        }
    }

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "ssa_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
