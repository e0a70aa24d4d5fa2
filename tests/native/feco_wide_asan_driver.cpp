// Driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp): walks
// sg_feco_kmeans_compress_wide under AddressSanitizer + UBSan -- every refusal (SG_ERR_ARG before the first launch), one accepted
// call each at D 65, 72 and 128 with the kernel instantiation, grid, block and dynamic LDS it must issue, the first accepted call
// of a context at a larger shape, the longest utterance and the refusal behind it, and two contexts side by side.  The narrow
// entry next door keeps refusing 65 columns.  "Device" buffers are host buffers sized exactly as the header says.  No kernel runs.
#include "driver_common.h"

static bool is_wide(const Launch& l, int ng) {
    return l.name.find("::feco_kmeans_wide_kernel<" + std::to_string(ng) + ">(") != std::string::npos;
}
// dynamic LDS in bytes of (F, k, D): the layout the header describes (k_feco_wide.hip feco_wide_layout), written out again
static size_t wide_lds(int F, int k, int D) {
    const auto al4 = [](int n) { return (n + 3) & ~3; };
    const int ng = (D + 7) / 8, kp = (k + 31) & ~31;
    return (size_t)(kp * (8 * ng + 4) + kp + 128 + 16 * 128 + al4(F) + al4(k) + al4(k + 1) + al4(F)) * 4;
}

int main() {
    hipdouble_set_launch_hook(record_launch);
    sg_ctx *ctx = nullptr, *ctx2 = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int BMAX = 3, FMAX = 833, DMAX = 128;
    std::vector<float> feats((size_t)BMAX * FMAX * DMAX, 0.5f), out((size_t)BMAX * FMAX * DMAX);
    std::vector<int32_t> ids((size_t)BMAX * FMAX), counts((size_t)BMAX * FMAX);
    auto call = [&](sg_ctx* c, int B, int F, int D, int k, int max_iter, int random_init) {
        return sg_feco_kmeans_compress_wide(c, feats.data(), B, F, D, k, max_iter, random_init, 7, 5, ids.data(), out.data(), counts.data(),
                                            nullptr);
    };
    auto too_long = [&]() { return std::string(sg_last_error(ctx)).find("utterance too long for one block") != std::string::npos; };

    // ---- every refusal: nothing is launched
    const long l0 = hipdouble_launches();
    EXPECT(call(nullptr, 3, 300, 72, 150, 10, 0) == SG_ERR_ARG);                // no context
    EXPECT(call(ctx, 0, 300, 72, 150, 10, 0) == SG_ERR_ARG);                    // B
    EXPECT(call(ctx, -1, 300, 72, 150, 10, 0) == SG_ERR_ARG);
    EXPECT(call(ctx, 3, 0, 72, 0, 10, 0) == SG_ERR_ARG);                        // F
    for (int D : {0, 30, 64, 129, 256}) EXPECT(call(ctx, 3, 300, D, 150, 10, 0) == SG_ERR_ARG && !too_long());  // D outside 65 .. 128
    EXPECT(call(ctx, 3, 300, 72, 0, 10, 0) == SG_ERR_ARG);                      // k
    EXPECT(call(ctx, 3, 300, 72, 301, 10, 0) == SG_ERR_ARG);                    // k > F
    EXPECT(call(ctx, 3, 300, 72, 150, 0, 0) == SG_ERR_ARG);                     // max_iter
    EXPECT(call(ctx, 3, 300, 72, 150, -2, 1) == SG_ERR_ARG);
    const long l1 = l0;
    EXPECT(call(ctx, 1, 834, 72, 417, 10, 0) == SG_ERR_ARG && too_long());      // one frame past the longest utterance
    EXPECT(call(ctx, 1, 864, 72, 432, 10, 0) == SG_ERR_ARG && too_long());      // the next multiple of 32
    EXPECT(call(ctx, 2, 5000, 72, 2500, 10, 0) == SG_ERR_ARG && too_long());
    EXPECT(call(ctx, 1, 400, 128, 400, 10, 0) == SG_ERR_ARG && too_long());     // k = F at full width: 416 rows of 132 floats
    EXPECT(sg_feco_kmeans_compress_wide(ctx, nullptr, 3, 300, 72, 150, 10, 0, 7, 5, ids.data(), out.data(), counts.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_feco_kmeans_compress_wide(ctx, feats.data(), 3, 300, 72, 150, 10, 0, 7, 5, nullptr, out.data(), counts.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_feco_kmeans_compress_wide(ctx, feats.data(), 3, 300, 72, 150, 10, 0, 7, 5, ids.data(), nullptr, counts.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_feco_kmeans_compress_wide(ctx, feats.data(), 3, 300, 72, 150, 10, 0, 7, 5, ids.data(), out.data(), nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(hipdouble_launches() == l1 && sg_last_error(ctx)[0] != 0);
    // the narrow entry keeps its cap and its words
    EXPECT(sg_feco_kmeans_compress(ctx, feats.data(), 3, 50, 65, 25, 10, 0, 7, 5, 1, ids.data(), out.data(), counts.data(), nullptr) == SG_ERR_ARG);
    EXPECT(std::string(sg_last_error(ctx)) == "sg_feco_kmeans: need 0 < k <= F, 0 < D <= 64, max_iter > 0");
    EXPECT(hipdouble_launches() == l1);

    // ---- what runs: one launch each, the instantiation of ceil(D / 8) groups, a block per utterance, the layout's LDS
    struct Shape { int B, F, k, D; };
    const Shape shapes[] = {{3, 300, 150, 72}, {1, 90, 36, 65}, {2, 40, 20, 128}, {3, 300, 12, 96}, {1, 33, 1, 80}, {1, 37, 37, 72},
                            {1, 833, 416, 72}};
    for (const Shape& s : shapes)
        for (int random_init : {0, 1}) {
            g_seen.clear();
            EXPECT(call(ctx, s.B, s.F, s.D, s.k, 10, random_init) == SG_OK);
            EXPECT(g_seen.size() == 1);
            if (g_seen.size() != 1) continue;
            const Launch& l = g_seen[0];
            EXPECT(is_wide(l, (s.D + 7) / 8));
            EXPECT(l.grid.x == (unsigned)s.B && l.grid.y == 1 && l.grid.z == 1 && l.block.x == 512);
            EXPECT(l.lds == wide_lds(s.F, s.k, s.D) && l.lds <= 150 * 1024);
        }
    EXPECT(wide_lds(833, 416, 72) == 146864 && wide_lds(834, 417, 72) > 150 * 1024 && wide_lds(300, 150, 72) == 61600);

    // ---- a second context: its FIRST accepted call is the large shape; the two contexts do not disturb each other
    EXPECT(sg_create(0, &ctx2) == SG_OK && ctx2 != nullptr);
    if (ctx2) {
        g_seen.clear();
        EXPECT(call(ctx2, 3, 833, 72, 416, 10, 1) == SG_OK);
        EXPECT(call(ctx, 3, 300, 72, 150, 10, 0) == SG_OK);
        EXPECT(call(ctx2, 1, 834, 72, 417, 10, 0) == SG_ERR_ARG);
        EXPECT(call(ctx, 2, 77, 72, 23, 10, 0) == SG_OK);
        EXPECT(g_seen.size() == 3 && std::string(sg_last_error(ctx2)).find("too long") != std::string::npos);
        sg_destroy(ctx2);
    }
    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "feco_wide_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
