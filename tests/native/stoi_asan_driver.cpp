// Ninth driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks sg_wav_stoi under AddressSanitizer + UBSan -- every refusal (SG_ERR_ARG before the first launch, nothing allocated), the
// tables the host builds (read back through the first launch that takes them: "device" memory is host memory here), the launch
// sequence and geometry at both sample rates and at a length without a segment, the workspace at B = 1, 3 and 64 (grown, never
// multiplied), the table cache (one entry per fs, reused), and two contexts side by side.  No kernel runs.
#include "driver_common.h"

// the table blob as csrc/k_stoi.hip lays it out (StoiTab); main() holds its size against the library's own
struct Tab {
    double g[5 * 123 + 1];
    double win[256];
    double tw1[448][2];
    double tw2[72][2];
    double clip, pad;
    int32_t lo[16], hi[16];
};
static const Tab* g_tab = nullptr;
static void on_launch(const Launch& l, void** args) {
    g_seen.push_back(l);
    if (kernel_name(l.name) == "stoi_resample_kernel") g_tab = *static_cast<const Tab* const*>(args[0]);
}
static bool is(const Launch& l, const char* kernel, unsigned gx, unsigned gy, unsigned gz) {
    return kernel_name(l.name) == kernel && l.grid.x == gx && l.grid.y == gy && l.grid.z == gz && l.block.x == 256 && l.lds == 0;
}

int main() {
    hipdouble_set_launch_hook(record_launch);
    g_on_launch = on_launch;
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int BMAX = 64, TMAX = 16001;
    std::vector<float> x((size_t)BMAX * TMAX, 0.25f), y((size_t)BMAX * TMAX, 0.125f);
    std::vector<double> d(BMAX, -1.0);
    std::vector<int32_t> frames(BMAX, -1);
    auto run = [&](sg_ctx* c, int B, int T, int fs, int32_t* fr) { return sg_wav_stoi(c, x.data(), y.data(), B, T, fs, d.data(), fr, nullptr); };

    // ---- the mirror above has the library's size, and the pure table call copies only into room that holds it
    {
        EXPECT(sg_stoi_debug_tables(nullptr, 0) == (int32_t)sizeof(Tab));
        std::vector<unsigned char> room(sizeof(Tab) + 16, 0xAB);
        EXPECT(sg_stoi_debug_tables(room.data(), (int32_t)sizeof(Tab) - 1) == (int32_t)sizeof(Tab) && room[0] == 0xAB);
        EXPECT(sg_stoi_debug_tables(room.data(), (int32_t)sizeof(Tab)) == (int32_t)sizeof(Tab) && room[sizeof(Tab)] == 0xAB);
        Tab t;
        std::memcpy(&t, room.data(), sizeof(Tab));
        EXPECT(t.lo[0] == 7 && t.hi[14] == 219 && t.win[0] > 0.0);
    }

    // ---- every refusal: nothing is launched, nothing is allocated
    const long l0 = hipdouble_launches(), a0 = hipdouble_live_allocs();
    EXPECT(sg_wav_stoi(nullptr, x.data(), y.data(), 1, 8000, 16000, d.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_wav_stoi(ctx, nullptr, y.data(), 1, 8000, 16000, d.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_wav_stoi(ctx, x.data(), nullptr, 1, 8000, 16000, d.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(sg_wav_stoi(ctx, x.data(), y.data(), 1, 8000, 16000, nullptr, frames.data(), nullptr) == SG_ERR_ARG);
    for (int B : {0, -1, 65536, -2147483647 - 1}) EXPECT(run(ctx, B, 8000, 16000, nullptr) == SG_ERR_ARG);
    for (int fs : {8000, 0, -16000, 44100, 16001}) EXPECT(run(ctx, 1, 8000, fs, nullptr) == SG_ERR_ARG);
    // 16 kHz: ceil(5 T / 8) <= 256 up to T = 409; 10 kHz: T <= 256
    for (int T : {0, -1, 1, 400, 409, (1 << 24) + 1, 0x7FFFFFFF}) EXPECT(run(ctx, 1, T, 16000, nullptr) == SG_ERR_ARG);
    for (int T : {0, 255, 256, (1 << 24) + 1}) EXPECT(run(ctx, 1, T, 10000, nullptr) == SG_ERR_ARG);
    EXPECT(hipdouble_launches() == l0 && sg_last_error(ctx)[0] != 0);
    EXPECT(hipdouble_live_allocs() == a0);

    // ---- what runs.  T -> samples at 10 kHz -> frames nF = ceil((n10 - 256) / 128); tiles of 8 frames; the band launch has one wave
    // per output frame (nF - 1 of them) and is left out where no row can hold a segment (nF - 1 < 30)
    struct Case { int T, fs, nF; };
    bool first_call = true;
    for (const Case& c : {Case{410, 16000, 1}, Case{6400, 16000, 30}, Case{6758, 16000, 31}, Case{8000, 16000, 38}, Case{16001, 16000, 77},
                          Case{257, 10000, 1}, Case{10001, 10000, 77}})
        for (int B : {1, 3, BMAX}) {
            g_seen.clear();
            const long live = hipdouble_live_allocs();
            EXPECT(run(ctx, B, c.T, c.fs, B == 3 ? nullptr : frames.data()) == SG_OK);
            const bool bands = c.nF - 1 >= 30;
            EXPECT((int)g_seen.size() == (bands ? 5 : 4));
            if ((int)g_seen.size() != (bands ? 5 : 4)) continue;
            const unsigned ub = (unsigned)B;
            EXPECT(is(g_seen[0], "stoi_scale_kernel", 8, 2, ub));
            EXPECT(is(g_seen[1], "stoi_resample_kernel", (unsigned)((c.nF + 7) / 8), 2, ub));
            EXPECT(is(g_seen[2], "stoi_mask_kernel", ub, 1, 1));
            if (bands) EXPECT(is(g_seen[3], "stoi_bands_kernel", (unsigned)((c.nF - 1 + 3) / 4), ub, 1));
            EXPECT(is(g_seen.back(), "stoi_segments_kernel", ub, 1, 1));
            // the first call brings the two workspaces and the fs's tables, the first call of the other fs its tables; growing a
            // workspace releases the one it replaces
            const bool new_fs = B == 1 && (c.T == 410 || c.T == 257);
            EXPECT(hipdouble_live_allocs() == live + (first_call ? 3 : new_fs ? 1 : 0));
            first_call = false;
        }

    // ---- the tables, as the host built them
    EXPECT(g_tab != nullptr);
    if (g_tab) {
        std::vector<unsigned char> pure(sizeof(Tab));
        sg_stoi_debug_tables(pure.data(), (int32_t)sizeof(Tab));
        EXPECT(std::memcmp(pure.data(), g_tab, sizeof(Tab)) == 0);  // what the launches read is what the pure call hands out
        const Tab& t = *g_tab;
        double all = 0.0;
        for (int p = 0; p < 5; ++p) {
            double s = 0.0;
            for (int j = 0; j < 123; ++j) s += t.g[p * 123 + j];
            EXPECT(std::fabs(s - 1.0) < 1e-3);  // every branch of a low-pass that passes DC passes it alone, nearly
            all += s;
        }
        EXPECT(std::fabs(all - 5.0) < 1e-12);  // h has unit sum, the branches hold 5 h
        EXPECT(t.g[0 * 123 + 58] > t.g[0 * 123 + 57] && t.g[0 * 123 + 57] == t.g[0 * 123 + 59]);  // phase 0: symmetric about tap 58
        EXPECT(t.g[0] != 0.0 && t.g[4 * 123 + 0] == 0.0 && t.g[4 * 123 + 121] != 0.0);             // the window's two ends
        for (int i = 0; i < 128; ++i) EXPECT(t.win[i] > 0.0 && t.win[i] < 1.0 && std::fabs(t.win[i] - t.win[255 - i]) < 1e-15);
        EXPECT(std::fabs(t.win[0] - (0.5 - 0.5 * std::cos(2.0 * M_PI / 257.0))) < 1e-15);
        EXPECT(t.tw1[0][0] == 1.0 && t.tw1[0][1] == 0.0 && std::fabs(t.tw1[1][0] - std::cos(2.0 * M_PI / 512.0)) < 1e-15 &&
               std::fabs(t.tw1[1][1] + std::sin(2.0 * M_PI / 512.0)) < 1e-15);
        EXPECT(std::fabs(t.tw2[9 * 1 + 1][0] - std::cos(2.0 * M_PI / 64.0)) < 1e-15 && t.tw2[8][0] == 0.0);
        EXPECT(std::fabs(t.clip - (1.0 + std::pow(10.0, 0.75))) < 1e-15);
        const int edges[16] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
        for (int b = 0; b < 15; ++b) EXPECT(t.lo[b] == edges[b] && t.hi[b] == edges[b + 1]);
    }

    // ---- a smaller call after the largest, and the cached tables again: nothing new
    {
        const long live = hipdouble_live_allocs();
        const Tab* before = g_tab;
        EXPECT(run(ctx, 2, 8000, 10000, frames.data()) == SG_OK && g_tab == before);
        EXPECT(run(ctx, 1, 6758, 16000, nullptr) == SG_OK && g_tab != before && g_tab != nullptr);
        EXPECT(hipdouble_live_allocs() == live);
    }

    // ---- two contexts: each its own tables and workspaces, released with it
    {
        const long before = hipdouble_live_allocs();
        sg_ctx* other = nullptr;
        EXPECT(sg_create(0, &other) == SG_OK && other != nullptr);
        if (other) {
            const long live = hipdouble_live_allocs();
            const Tab* mine = g_tab;
            EXPECT(run(other, 3, 8000, 16000, frames.data()) == SG_OK);
            EXPECT(hipdouble_live_allocs() == live + 3 && g_tab != mine);
            EXPECT(run(ctx, 3, 8000, 16000, frames.data()) == SG_OK && g_tab == mine);
            EXPECT(run(other, 1, 410, 16000, nullptr) == SG_OK && hipdouble_live_allocs() == live + 3);
            sg_destroy(other);
            EXPECT(hipdouble_live_allocs() == before);
        }
    }

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "stoi_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
