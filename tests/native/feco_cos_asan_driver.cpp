// Fifth driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks sg_feco_kmeans_compress_metric under AddressSanitizer + UBSan -- every refusal (SG_ERR_ARG before the first launch), both
// metrics, row_wise 0 / 1, reps 1 and 3, DPAD 32 and 64, one and two CUs per instance.  It checks which kernel a call launches
// and on what grid: the L2 metric must issue exactly the launch of the entry it stands for, the cosine metric the same grid,
// block and dynamic LDS on the cosine kernel.  "Device" buffers are host buffers sized exactly as the header says.  No kernel runs.
#include "driver_common.h"

static bool is_kernel(const Launch& l, const char* kernel, int dpad) {
    return l.name.find(std::string("::") + kernel + "<" + std::to_string(dpad) + ">(") != std::string::npos;
}

int main() {
    hipdouble_set_launch_hook(record_launch);
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int BMAX = 3, RMAX = 3, FMAX = 300, DMAX = 64;
    std::vector<float> feats((size_t)RMAX * BMAX * FMAX * DMAX, 0.5f), out((size_t)RMAX * BMAX * FMAX * DMAX);
    std::vector<int32_t> ids((size_t)RMAX * BMAX * FMAX), counts((size_t)RMAX * BMAX * FMAX);
    auto call = [&](int metric, int B, int F, int D, int k, int max_iter, int random_init, int reps, int row_wise) {
        return sg_feco_kmeans_compress_metric(ctx, feats.data(), B, F, D, k, max_iter, metric, random_init, 7, 5, reps, row_wise, ids.data(),
                                              out.data(), counts.data(), nullptr);
    };

    // ---- every refusal, under both metrics where the metric is not what is refused: nothing is launched
    const long l0 = hipdouble_launches();
    EXPECT(sg_feco_kmeans_compress_metric(nullptr, feats.data(), 3, 50, 30, 25, 10, SG_FECO_COS, 0, 0, 0, 1, 0, ids.data(), out.data(),
                                          counts.data(), nullptr) == SG_ERR_ARG);
    for (int metric : {-1, 2, 7}) EXPECT(call(metric, 3, 50, 30, 25, 10, 0, 1, 0) == SG_ERR_ARG);
    for (int metric : {SG_FECO_L2, SG_FECO_COS}) {
        for (int row_wise : {-1, 2}) EXPECT(call(metric, 3, 50, 30, 25, 10, 0, 1, row_wise) == SG_ERR_ARG);
        for (int row_wise : {0, 1}) {
            EXPECT(call(metric, 0, 50, 30, 25, 10, 0, 1, row_wise) == SG_ERR_ARG);    // B
            EXPECT(call(metric, 3, 0, 30, 0, 10, 0, 1, row_wise) == SG_ERR_ARG);      // F
            EXPECT(call(metric, 3, 50, 0, 25, 10, 0, 1, row_wise) == SG_ERR_ARG);     // D
            EXPECT(call(metric, 3, 50, 65, 25, 10, 0, 1, row_wise) == SG_ERR_ARG);    // D past 64
            EXPECT(call(metric, 3, 50, 30, 0, 10, 0, 1, row_wise) == SG_ERR_ARG);     // k
            EXPECT(call(metric, 3, 50, 30, 51, 10, 0, 1, row_wise) == SG_ERR_ARG);    // k > F
            EXPECT(call(metric, 3, 50, 30, 25, 0, 0, 1, row_wise) == SG_ERR_ARG);     // max_iter
            EXPECT(call(metric, 3, 50, 30, 25, 10, 1, 0, row_wise) == SG_ERR_ARG);    // reps
            EXPECT(call(metric, 3, 50, 30, 25, 10, 1, 65536, row_wise) == SG_ERR_ARG);
            EXPECT(call(metric, 2, 5000, 30, 2500, 10, 0, 1, row_wise) == SG_ERR_ARG);  // one utterance past a block's LDS
        }
        // repeats of the evenly started clustering coincide: refused unless the rows have features of their own
        EXPECT(call(metric, 3, 50, 30, 25, 10, 0, 3, 0) == SG_ERR_ARG);
    }
    for (int metric : {SG_FECO_L2, SG_FECO_COS})
        for (int row_wise : {0, 1}) {
            EXPECT(sg_feco_kmeans_compress_metric(ctx, nullptr, 3, 50, 30, 25, 10, metric, 0, 7, 5, 1, row_wise, ids.data(), out.data(),
                                                  counts.data(), nullptr) == SG_ERR_ARG);
            EXPECT(sg_feco_kmeans_compress_metric(ctx, feats.data(), 3, 50, 30, 25, 10, metric, 0, 7, 5, 1, row_wise, nullptr, out.data(),
                                                  counts.data(), nullptr) == SG_ERR_ARG);
            EXPECT(sg_feco_kmeans_compress_metric(ctx, feats.data(), 3, 50, 30, 25, 10, metric, 0, 7, 5, 1, row_wise, ids.data(), nullptr,
                                                  counts.data(), nullptr) == SG_ERR_ARG);
            EXPECT(sg_feco_kmeans_compress_metric(ctx, feats.data(), 3, 50, 30, 25, 10, metric, 0, 7, 5, 1, row_wise, ids.data(), out.data(),
                                                  nullptr, nullptr) == SG_ERR_ARG);
        }
    EXPECT(hipdouble_launches() == l0 && sg_last_error(ctx)[0] != 0);

    // ---- what runs: (F, k, D) at DPAD 32 and 64, reps 1 and 3, row_wise 0 / 1, one and two CUs per instance
    struct Shape { int F, k, D, dpad; };
    const Shape shapes[] = {{50, 25, 30, 32}, {300, 150, 32, 32}, {200, 100, 32, 32}, {70, 14, 40, 64}, {33, 33, 30, 32}, {40, 1, 64, 64}};
    int paired = 0;
    for (int two_cu : {-1, 0}) {
        EXPECT(sg_feco_set_two_cu(ctx, two_cu) == SG_OK);
        for (const Shape& s : shapes)
            for (int reps : {1, 3})
                for (int row_wise : {0, 1})
                    for (int random_init : {0, 1}) {
                        if (reps > 1 && !row_wise && !random_init) continue;  // refused above
                        g_seen.clear();
                        const int rc_old = row_wise ? sg_feco_kmeans_compress_rows(ctx, feats.data(), BMAX, s.F, s.D, s.k, 10, random_init, 7, 5, reps,
                                                                                   ids.data(), out.data(), counts.data(), nullptr)
                                                    : sg_feco_kmeans_compress(ctx, feats.data(), BMAX, s.F, s.D, s.k, 10, random_init, 7, 5, reps,
                                                                              ids.data(), out.data(), counts.data(), nullptr);
                        EXPECT(rc_old == SG_OK);
                        EXPECT(call(SG_FECO_L2, BMAX, s.F, s.D, s.k, 10, random_init, reps, row_wise) == SG_OK);
                        EXPECT(call(SG_FECO_COS, BMAX, s.F, s.D, s.k, 10, random_init, reps, row_wise) == SG_OK);
                        EXPECT(g_seen.size() == 3);
                        if (g_seen.size() != 3) continue;
                        EXPECT(is_kernel(g_seen[0], "feco_kmeans_kernel", s.dpad) && is_kernel(g_seen[1], "feco_kmeans_kernel", s.dpad));
                        EXPECT(is_kernel(g_seen[2], "feco_kmeans_cos_kernel", s.dpad));
                        EXPECT(g_seen[1].same_shape(g_seen[0]) && g_seen[2].same_shape(g_seen[0]));
                        EXPECT(g_seen[0].grid.x == (unsigned)BMAX && g_seen[0].grid.y == (unsigned)reps && g_seen[0].block.x == 1024);
                        EXPECT(g_seen[0].grid.z == 1 || (two_cu == -1 && s.dpad == 32));
                        paired += g_seen[2].grid.z == 2;
                    }
    }
    EXPECT(paired > 0);  // the two-CU form was among them, for the cosine kernel too

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "feco_cos_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
