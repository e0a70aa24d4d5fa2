// Fifth driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks sg_feco_kmeans_compress_metric under AddressSanitizer + UBSan -- every refusal (SG_ERR_ARG before the first launch), both
// metrics, row_wise 0 / 1, reps 1 and 3, DPAD 32 and 64, one and two CUs per instance.  It checks which kernel a call launches
// and on what grid: the L2 metric must issue exactly the launch of the entry it stands for, the cosine metric the same grid,
// block and dynamic LDS on the cosine kernel.  "Device" buffers are host buffers sized exactly as the header says.  No kernel runs.
//
// `feco_cos_asan_driver --plan-table` is the second mode: it walks the FeCo k-means launchers (k_feco.hip, k_feco_wide.hip,
// k_feco_warped.hip) over the shapes the GPU tests pin, the benchmark's and the loops' shapes and every branch edge of the plan,
// and prints one line per launch -- kernel, grid, block, dynamic LDS and, for the base kernels, what the launcher planned: x_in_lds,
// fast_lists, JC, the unit table of each block, the owner mask.  Every one of these choices gives the same bits on the GPU, so
// only this shows a changed one.  Recorded in tests/native/feco_plan_table.expected (tests/test_feco_plan_table.py), one process
// per device / knob setting (HIPDOUBLE_CUS; `--plan-table two_cu0`: after sg_feco_set_two_cu(ctx, 0)).
#include "driver_common.h"
#include "../../speakerguard_amd/csrc/sg_internal.h"  // FecoSched, FecoPair: the plan table reads the kernel's arguments

extern "C" long hipdouble_memset_asyncs();

// ---- the plan table ----------------------------------------------------------------------------------------------
static std::string g_label;
static int g_lines = 0;
static bool g_show_tag = false;  // the epoch case alone prints the tag base
static sg::FecoPair g_last_pair;
static long g_wipes = 0;  // hipMemsetAsync calls the double had counted at the last line

static std::string units(const unsigned (*u)[2]) {
    std::string s;
    for (int w = 0; w < sg::kFecoThreads / 64; ++w)
        for (int slot = 0; slot < 2; ++slot) {
            const unsigned v = u[w][slot];
            char b[40] = "-";  // ft:lo-hi:jc = frame tile, centroid tiles [lo, hi), chunk
            if (v != sg::kFecoNoUnit) std::snprintf(b, sizeof(b), "%u:%u-%u:%u", v & 255, v >> 8 & 255, v >> 16 & 255, v >> 24);
            s += (slot ? "," : w ? ";" : "") + std::string(b);
        }
    return s;
}

static void plan_launch(const Launch& l, void** args) {
    const std::string name = kernel_name(l.name);
    if (name.find("feco_") != 0) return;
    std::printf("%s | %s grid=%u,%u,%u block=%u lds=%zu", g_label.c_str(), name.c_str(), l.grid.x, l.grid.y, l.grid.z, l.block.x, l.lds);
    ++g_lines;
    if (name.find("feco_kmeans_kernel<") == 0 || name.find("feco_kmeans_cos_kernel<") == 0) {
        // (feats, F, D, k, max_iter, seeded, row_wise, seed, index_base, x_in_lds, fast_lists, JC, sched, pr, assign, out, counts)
        const auto i = [&](int at) { return *static_cast<const int*>(args[at]); };
        const sg::FecoSched& sc = *static_cast<const sg::FecoSched*>(args[12]);
        const sg::FecoPair& pr = *static_cast<const sg::FecoPair*>(args[13]);
        g_last_pair = pr;
        std::printf(" seeded=%d row_wise=%d x_in_lds=%d fast_lists=%d JC=%d table=%d u0=%s on=%d owner=%08x table1=%d", i(5), i(6), i(9), i(10),
                    i(11), sc.table, units(sc.u).c_str(), pr.on, pr.owner, pr.sched1.table);
        if (pr.on) std::printf(" u1=%s", units(pr.sched1.u).c_str());
        std::printf(" drop=%d", pr.drop);
        // the wipe of the exchange buffers (hipMemsetAsync, counted by the double) ahead of this launch
        if (hipdouble_memset_asyncs() != g_wipes) std::printf(" wipe=1");
        if (g_show_tag) std::printf(" tag0=%u", pr.tag0);
        g_wipes = hipdouble_memset_asyncs();
    }
    std::printf("\n");
}

// one call = one line: the launch, or the refusal
static void plan_case(sg_ctx* ctx, const std::string& label, int rc) {
    if (rc != SG_OK) std::printf("%s | rc=%d %s\n", label.c_str(), rc, sg_last_error(ctx));
    else EXPECT(g_lines == 1);
    g_lines = 0;
}

static int plan_table(const std::string& mode) {
    g_on_launch = plan_launch;
    hipdouble_set_launch_hook(record_launch);
    sg_ctx* ctx = nullptr;
    if (sg_create(0, &ctx) != SG_OK) return 1;
    g_wipes = hipdouble_memset_asyncs();
    if (mode == "two_cu0" && sg_feco_set_two_cu(ctx, 0) != SG_OK) return 1;
    static float feats[4], out[4];  // never dereferenced: the double runs no kernel
    static int32_t ids[4], counts[4];
    const auto label = [](const char* what, int metric, int B, int reps, int F, int k, int D, int it, int ri, int rw) {
        char b[200];
        std::snprintf(b, sizeof(b), "%s %s B=%dx%d F=%d k=%d D=%d it=%d ri=%d rw=%d", what, metric == SG_FECO_COS ? "cos" : "l2", B, reps, F, k, D, it,
                      ri, rw);
        return std::string(b);
    };
    const auto run = [&](const char* what, int metric, int B, int reps, int F, int k, int D, int it = 10, int ri = 1, int rw = 0) {
        g_label = label(what, metric, B, reps, F, k, D, it, ri, rw);
        plan_case(ctx, g_label, sg_feco_kmeans_compress_metric(ctx, feats, B, F, D, k, it, metric, ri, 7, 5, reps, rw, ids, out, counts, nullptr));
    };
    // ---- metric / kind: both metrics, row_wise 0 / 1, random_init 0 / 1 where accepted, and the two plain entries
    for (int metric : {SG_FECO_L2, SG_FECO_COS})
        for (int rw : {0, 1})
            for (int ri : {0, 1})
                for (int reps : {1, 3}) run("kind", metric, 3, reps, 300, 150, 32, 10, ri, rw);  // (reps 3, even start, not row-wise: refused)
    g_label = "kind sg_feco_kmeans B=3 F=300 k=150 D=32";
    plan_case(ctx, g_label, sg_feco_kmeans(ctx, feats, 3, 300, 32, 150, 10, ids, nullptr));
    g_label = "kind sg_feco_kmeans_seeded B=3 F=300 k=150 D=32";
    plan_case(ctx, g_label, sg_feco_kmeans_seeded(ctx, feats, 3, 300, 32, 150, 10, 7, 5, ids, nullptr));
    // ---- instances: pairing ends where 2 x instances exceed the CUs (256: 64 x 2 and 128 x 1 pair, 129 x 1 and 64 x 3 do not)
    const int inst[][2] = {{1, 1}, {3, 3}, {64, 2}, {128, 1}, {129, 1}, {64, 3}};  // (3 x 1: above)
    for (auto& br : inst) run("instances", SG_FECO_L2, br[0], br[1], 300, 150, 32);
    // ---- (F, k, D): this driver's six, the twelve of tests/test_gpu_feco.py::test_kmeans_ids_bit_exact (300 x 150 x 32 twice there),
    // the x-vector loop's 100 x 50 x 30; the benchmark's 300 x 150 x 32 is the shape of the cases above
    const int shapes[][4] = {{3, 50, 25, 30}, {3, 200, 100, 32}, {3, 70, 14, 40}, {3, 33, 33, 30}, {3, 40, 1, 64},
                             {3, 300, 150, 30}, {2, 77, 23, 13}, {2, 300, 150, 32}, {1, 80, 40, 8}, {2, 1500, 750, 30}, {2, 200, 100, 48},
                             {1, 90, 36, 64}, {1, 1850, 925, 32}, {2, 700, 350, 32}, {1, 1000, 250, 20}, {3, 300, 12, 32}, {2, 100, 50, 30}};
    for (auto& s : shapes)
        for (int metric : {SG_FECO_L2, SG_FECO_COS}) run("shape", metric, s[0], 1, s[1], s[2], s[3], 10, 0);
    // ---- branch edges, with what today's launcher selects
    run("edge 33 units", SG_FECO_L2, 1, 1, 1025, 64, 8);          // ntf 33, JC 1: table 0 (dealt in the kernel), fast_lists 0, frames in LDS
    run("edge fast_lists", SG_FECO_L2, 1, 1, 1024, 512, 32);      // 32 units: the last table; fast_lists 1, frames not in LDS
    run("edge fast_lists", SG_FECO_L2, 1, 1, 1025, 512, 32);      // F > 1024: fast_lists 0, table 0
    run("edge x_in_lds", SG_FECO_L2, 1, 1, 1025, 64, 32);         // the last k at F 1025, D 32 whose frames fit ...
    run("edge x_in_lds", SG_FECO_L2, 1, 1, 1025, 65, 32);         // ... and the first whose do not: x_in_lds 0
    run("edge longest", SG_FECO_L2, 1, 1, 1930, 965, 30);         // 156320 bytes with one chunk and no extras: REFUSED (limit 153600)
    run("edge merge cap", SG_FECO_L2, 1, 1, 2048, 64, 8);         // JC 1 either way (ntf >= 20): the cap rule holds at JC * F = 2048
    run("edge merge cap", SG_FECO_L2, 1, 1, 2049, 64, 8);
    run("edge merge cap", SG_FECO_L2, 1, 1, 600, 256, 8);         // JC 2 (ntf 19), 1200 <= 2048
    run("edge merge cap", SG_FECO_L2, 1, 1, 300, 256, 8);         // ntf 10: JC 2, far below the cap
    run("edge merge cap", SG_FECO_L2, 1, 1, 100, 100, 8);         // ntf 4: JC 5 asked, ntc 4 caps it
    run("edge merge cap", SG_FECO_L2, 1, 1, 64, 64, 8);           // ntf 2: JC 10 asked, ntc 2 caps it
    run("edge merge cap", SG_FECO_L2, 1, 1, 40, 40, 8);           // ntf 2, ntc 2
    run("edge max chunks", SG_FECO_L2, 1, 1, 32, 32, 8);          // ntf 1: JC 20 asked, ntc 1: one unit
    run("edge max chunks", SG_FECO_L2, 1, 1, 300, 300, 8);        // ntf 10, ntc 10: JC 2
    run("edge max_iter", SG_FECO_L2, 3, 1, 300, 150, 32, 62);     // kFecoPairMaxIter: paired
    run("edge max_iter", SG_FECO_L2, 3, 1, 300, 150, 32, 63);     // one more: the tag has no room, one block
    run("edge kp", SG_FECO_L2, 1, 1, 2049, 2049, 8);              // kp_host 2080 > 2048: REFUSED for its LDS long before (the pairing rule's kp bound is never reached)
    run("edge dpad 64", SG_FECO_L2, 3, 1, 40, 1, 64, 10, 1);      // dpad 64: never paired
    run("edge dpad 64", SG_FECO_L2, 3, 1, 70, 14, 40, 10, 1);
    run("edge dpad 64", SG_FECO_L2, 3, 1, 300, 150, 33);          // JC 2, 20 units, and still one block
    // ---- fault injection: exactly the next paired launch drops
    if (sg_debug_lose_handoffs(ctx, 1) != SG_OK) return 1;
    run("lose_handoffs=1 first", SG_FECO_L2, 3, 1, 300, 150, 32);
    EXPECT(mode == "two_cu0" || !g_last_pair.on || g_last_pair.drop == 1);
    run("lose_handoffs=1 second", SG_FECO_L2, 3, 1, 300, 150, 32);
    EXPECT(g_last_pair.drop == 0);
    if (sg_debug_lose_handoffs(ctx, 0) != SG_OK) return 1;
    // ---- epoch: the counter parked one below the 2^15 wrap -- the launch after it wipes the exchange buffers and starts the tags over
    if (sg_debug_feco_epoch(ctx, 0x7FFEu) != SG_OK) return 1;
    g_show_tag = true;
    run("epoch 0x7ffe +1", SG_FECO_L2, 3, 1, 300, 150, 32);
    run("epoch 0x7ffe +2", SG_FECO_L2, 3, 1, 300, 150, 32);
    run("epoch 0x7ffe +3", SG_FECO_L2, 3, 1, 300, 150, 32);
    g_show_tag = false;
    // ---- wide (k_feco_wide.hip): NG = ceil(D / 8) is the choice; 513 x 256 is the largest F x F / 2 one block holds at D 128
    const int wide[][3] = {{50, 25, 65}, {50, 25, 72}, {50, 25, 73}, {50, 25, 128}, {513, 256, 128}, {514, 257, 128}};
    for (auto& w : wide) {
        char b[120];
        std::snprintf(b, sizeof(b), "wide B=3 F=%d k=%d D=%d", w[0], w[1], w[2]);
        g_label = b;
        plan_case(ctx, g_label, sg_feco_kmeans_compress_wide(ctx, feats, 3, w[0], w[2], w[1], 10, 1, 7, 5, ids, out, counts, nullptr));
    }
    // ---- warped (k_feco_warped.hip): the six <WIDE, XL, ML> instantiations.  XL implies ML (sg_feco_warped), so the selector
    // never takes the values 2 and 6 and the `default:` refusal of its switch cannot be reached.
    const int warped[][3] = {{100, 50, 30}, {100, 50, 40}, {1200, 600, 32}, {1200, 300, 64}, {1200, 1200, 32}, {1200, 600, 64}};
    std::vector<int32_t> sweeps(3, 1);  // the status the entry point reads back: 1 sweep, converged
    for (auto& w : warped) {
        char b[120];
        std::snprintf(b, sizeof(b), "warped B=3 F=%d k=%d D=%d", w[0], w[1], w[2]);
        g_label = b;
        plan_case(ctx, g_label, sg_feco_warped(ctx, feats, 3, w[0], w[2], w[1], 0, 0.5, 7, 5, 0, ids, ids, counts, out, sweeps.data(), nullptr));
    }
    sg_destroy(ctx);
    return g_fail ? 1 : 0;
}

// ---- the plan's invariants: sg::feco_plan walked directly, no context.  Their violation would make the kernel skip or double a
// unit of the assignment, or run past its LDS; on the GPU they hold "by the tests passing" only for the shapes the tests use.
static void walk_plan_invariants() {
    constexpr int kWaves = sg::kFecoThreads / 64;
    long plans = 0, paired = 0;
    for (int F : {1, 31, 32, 33, 64, 65, 300, 1024, 1025, 1930, 2048, 2049})
        for (int k : {1, (F + 1) / 2, F})
            for (int D : {1, 30, 32, 33, 64})
                for (long instances : {1L, 2L, 128L, 129L})
                    for (int cus : {8, 120, 256, 304})
                        for (bool allow_pair : {false, true})
                            for (int max_iter : {10, 62, 63}) {
                                // what feco_kmeans_check admits: one chunk, no extras, fits
                                if ((size_t)sg::feco_layout(F, k, D <= 32 ? 32 : 64, 1, 0, 0).total * 4 > sg::kFecoLdsMax) continue;
                                const sg::FecoPlan p = sg::feco_plan(F, D, k, max_iter, instances, cus, allow_pair, sg::FecoKnobs());
                                ++plans;
                                paired += p.pair;
                                const int ntc = (k + 31) / 32, ntf = (F + 31) / 32, nunits = ntf * p.JC;
                                EXPECT(p.dpad == (D <= 32 ? 32 : 64) && p.JC >= 1 && p.JC <= ntc && p.JC <= sg::kFecoMaxChunks);
                                // the chunk-maxima arrays exist only for JC > 1 (feco_layout); a single chunk may be longer (F 2049)
                                EXPECT(p.JC == 1 || p.JC * F <= sg::kFecoMergeCap);
                                EXPECT(p.lds <= sg::kFecoLdsMax);
                                EXPECT(p.lds == (size_t)sg::feco_layout(F, k, p.dpad, p.JC, p.fast_lists, p.x_in_lds).total * 4);
                                EXPECT(!p.pair || (allow_pair && p.dpad == 32 && p.JC > 1 && nunits <= 32 && max_iter <= sg::kFecoPairMaxIter &&
                                                   2 * instances <= cus));
                                EXPECT(p.sched0.table == (nunits <= 2 * kWaves) && p.sched1.table == p.sched0.table);
                                if (!p.sched0.table) {
                                    EXPECT(!p.pair && p.owner == 0);
                                    continue;
                                }
                                // every unit (frame tile, chunk) exactly once over both blocks, at most two per wave (the table has
                                // no more room), with the chunk's range of centroid tiles: the JC ranges of a frame tile partition
                                // [0, ntc) and none is empty
                                std::vector<int> seen(nunits, 0);
                                unsigned owner = 0;
                                int in_block1 = 0;
                                for (int half = 0; half < 2; ++half)
                                    for (int w = 0; w < kWaves; ++w)
                                        for (int slot = 0; slot < 2; ++slot) {
                                            const unsigned v = (half ? p.sched1 : p.sched0).u[w][slot];
                                            if (v == sg::kFecoNoUnit) continue;
                                            const int ft = v & 255, lo = v >> 8 & 255, hi = v >> 16 & 255, jc = v >> 24;
                                            EXPECT(ft < ntf && jc < p.JC);
                                            if (ft >= ntf || jc >= p.JC) continue;
                                            ++seen[ft * p.JC + jc];
                                            EXPECT(lo == ntc * jc / p.JC && hi == ntc * (jc + 1) / p.JC && lo < hi && hi <= ntc);
                                            EXPECT(jc > 0 || lo == 0);
                                            EXPECT(jc < p.JC - 1 || hi == ntc);
                                            if (half) owner |= 1u << (ft * p.JC + jc);
                                            in_block1 += half;
                                        }
                                EXPECT(std::count(seen.begin(), seen.end(), 1) == nunits);
                                EXPECT(owner == p.owner);
                                EXPECT(p.pair || in_block1 == 0);
                            }
    EXPECT(plans > 0 && paired > 0);
}

static bool is_kernel(const Launch& l, const char* kernel, int dpad) {
    return l.name.find(std::string("::") + kernel + "<" + std::to_string(dpad) + ">(") != std::string::npos;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "--plan-table") return plan_table(argc > 2 ? argv[2] : "default");
    walk_plan_invariants();
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
