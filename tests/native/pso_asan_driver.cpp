// Tenth driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp and abi_asan_driver.cpp):
// walks sg_pso_init / sg_pso_select / sg_pso_move under AddressSanitizer + UBSan -- every refusal (SG_ERR_ARG before the first
// launch: NULL arguments, n / P / T out of range, row lists that leave 0 .. n-1 or repeat a slot, best_index / gbest_from out of
// range), then accepted calls at P = 1, T = 1 and T = 1025 and at a vectorisable T, with the launch geometry of each: the grid is
// sized from n_active T, one launch per call, the 16-byte kernels only where T and every base allow them (SG_PSO_VEC=4 for that
// walk) and, by the library's own rule, only from two waves per SIMD of the device on (a device of one compute unit shows both
// sides).  "Device" buffers are host buffers sized exactly as the header says.  No kernel runs.
#include "driver_common.h"

int main() {
    hipdouble_set_launch_hook(record_launch);
    setenv("SG_TUNE", "1", 1);  // SG_PSO_VEC counts, where the walk sets it
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    const int N = 3, PMAX = 5, TMAX = 1028;
    std::vector<float> x((size_t)N * TMAX, 0.1f), lo((size_t)N * TMAX, -0.01f), hi((size_t)N * TMAX, 0.01f);
    std::vector<float> loc((size_t)N * PMAX * TMAX), vel(loc.size()), pbl(loc.size()), gbl((size_t)N * TMAX), pb((size_t)N * PMAX),
        gb(N, INFINITY), q(loc.size()), draws(loc.size(), 0.5f), loss((size_t)N * PMAX, 1.f), report(3 * (size_t)N);
    std::vector<uint8_t> imp((size_t)N * PMAX, 1);
    const int32_t rows[3] = {2, 0, 1}, best[3] = {0, 4, 2}, from[3] = {-1, 4, 0}, cont[3] = {1, 0, 1};

    auto init = [&](const float* xi, int n, int P, int T, const int32_t* r, int na, int epoch, const int32_t* b, float* l) {
        return sg_pso_init(ctx, xi, lo.data(), hi.data(), n, P, T, r, na, epoch, b, 7, 0, nullptr, nullptr, l, vel.data(), pbl.data(),
                           pb.data(), q.data(), nullptr);
    };
    auto select = [&](const float* ls, int n, int P, const int32_t* r, int na, float* rep) {
        return sg_pso_select(ctx, ls, n, P, r, na, pb.data(), gb.data(), imp.data(), rep, nullptr);
    };
    auto move = [&](const float* xi, int n, int P, int T, const int32_t* r, int na, const int32_t* f, const int32_t* c, int do_move,
                    float* qs) {
        return sg_pso_move(ctx, xi, lo.data(), hi.data(), n, P, T, r, na, f, c, do_move, 0.5f, 1.4961f, 1.4961f, 7, 0, nullptr, nullptr,
                           imp.data(), loc.data(), vel.data(), pbl.data(), gbl.data(), qs, nullptr);
    };

    // ---- every refusal: nothing is launched, nothing is allocated
    const long l0 = hipdouble_launches(), a0 = hipdouble_live_allocs();
    EXPECT(sg_pso_init(nullptr, x.data(), lo.data(), hi.data(), N, PMAX, 8, rows, 3, 0, nullptr, 7, 0, nullptr, nullptr, loc.data(),
                       vel.data(), pbl.data(), pb.data(), q.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_pso_select(nullptr, loss.data(), N, PMAX, rows, 3, pb.data(), gb.data(), imp.data(), report.data(), nullptr) == SG_ERR_ARG);
    EXPECT(sg_pso_move(nullptr, x.data(), lo.data(), hi.data(), N, PMAX, 8, rows, 3, from, cont, 1, 0.5f, 1.f, 1.f, 7, 0, nullptr, nullptr,
                       imp.data(), loc.data(), vel.data(), pbl.data(), gbl.data(), q.data(), nullptr) == SG_ERR_ARG);
    EXPECT(init(nullptr, N, PMAX, 8, rows, 3, 0, nullptr, loc.data()) == SG_ERR_ARG);
    EXPECT(init(x.data(), N, PMAX, 8, nullptr, 3, 0, nullptr, loc.data()) == SG_ERR_ARG);
    EXPECT(init(x.data(), N, PMAX, 8, rows, 3, 0, nullptr, nullptr) == SG_ERR_ARG);
    EXPECT(init(x.data(), N, PMAX, 8, rows, 3, 1, nullptr, loc.data()) == SG_ERR_ARG);   // epoch > 0 without best_index
    EXPECT(init(x.data(), N, PMAX, 8, rows, 3, -1, best, loc.data()) == SG_ERR_ARG);
    EXPECT(select(nullptr, N, PMAX, rows, 3, report.data()) == SG_ERR_ARG);
    EXPECT(select(loss.data(), N, PMAX, nullptr, 3, report.data()) == SG_ERR_ARG);
    EXPECT(select(loss.data(), N, PMAX, rows, 3, nullptr) == SG_ERR_ARG);
    EXPECT(move(nullptr, N, PMAX, 8, rows, 3, from, cont, 1, q.data()) == SG_ERR_ARG);
    EXPECT(move(x.data(), N, PMAX, 8, nullptr, 3, from, cont, 1, q.data()) == SG_ERR_ARG);
    EXPECT(move(x.data(), N, PMAX, 8, rows, 3, nullptr, cont, 1, q.data()) == SG_ERR_ARG);
    EXPECT(move(x.data(), N, PMAX, 8, rows, 3, from, nullptr, 1, q.data()) == SG_ERR_ARG);
    EXPECT(move(x.data(), N, PMAX, 8, rows, 3, from, cont, 1, nullptr) == SG_ERR_ARG);   // rows move, no room for their queries
    struct Shape { int n, P, T; };
    for (const Shape& s : {Shape{0, 5, 8}, Shape{-1, 5, 8}, Shape{257, 5, 8}, Shape{3, 0, 8}, Shape{3, -2, 8}, Shape{3, 1025, 8},
                           Shape{3, 5, 0}, Shape{3, 5, -4}}) {
        EXPECT(init(x.data(), s.n, s.P, s.T, rows, 1, 0, nullptr, loc.data()) == SG_ERR_ARG);
        EXPECT(move(x.data(), s.n, s.P, s.T, rows, 1, from, cont, 1, q.data()) == SG_ERR_ARG);
        if (s.T == 8) EXPECT(select(loss.data(), s.n, s.P, rows, 1, report.data()) == SG_ERR_ARG);
    }
    const int32_t twice[3] = {1, 2, 1}, beyond[3] = {0, 3, 1}, below[3] = {0, -1, 1}, four[4] = {0, 1, 2, 0};
    for (const int32_t* bad : {twice, beyond, below}) {
        EXPECT(init(x.data(), N, PMAX, 8, bad, 3, 0, nullptr, loc.data()) == SG_ERR_ARG);
        EXPECT(select(loss.data(), N, PMAX, bad, 3, report.data()) == SG_ERR_ARG);
        EXPECT(move(x.data(), N, PMAX, 8, bad, 3, from, cont, 1, q.data()) == SG_ERR_ARG);
    }
    for (int na : {0, -1, 4}) {  // an empty list, more rows than utterances
        EXPECT(init(x.data(), N, PMAX, 8, four, na, 0, nullptr, loc.data()) == SG_ERR_ARG);
        EXPECT(select(loss.data(), N, PMAX, four, na, report.data()) == SG_ERR_ARG);
        EXPECT(move(x.data(), N, PMAX, 8, four, na, from, cont, 1, q.data()) == SG_ERR_ARG);
    }
    const int32_t best_hi[3] = {0, 5, 2}, best_lo[3] = {0, -1, 2}, from_hi[3] = {-1, 5, 0}, from_lo[3] = {-2, 4, 0};
    EXPECT(init(x.data(), N, PMAX, 8, rows, 3, 1, best_hi, loc.data()) == SG_ERR_ARG);
    EXPECT(init(x.data(), N, PMAX, 8, rows, 3, 2, best_lo, loc.data()) == SG_ERR_ARG);
    EXPECT(move(x.data(), N, PMAX, 8, rows, 3, from_hi, cont, 1, q.data()) == SG_ERR_ARG);
    EXPECT(move(x.data(), N, PMAX, 8, rows, 3, from_lo, cont, 0, q.data()) == SG_ERR_ARG);
    EXPECT(hipdouble_launches() == l0 && sg_last_error(ctx)[0] != 0);
    EXPECT(hipdouble_live_allocs() == a0);

    // ---- what runs: one launch per call, the grid from n_active and T, the kernel by T and the bases' alignment
    setenv("SG_PSO_VEC", "4", 1);
    struct Case { int P, T; bool vec; unsigned gx; };
    const Case cases[] = {{1, 1, false, 1}, {1, 1025, false, 5}, {5, 1, false, 1}, {5, 1025, false, 5}, {5, 1028, true, 2}, {2, 3, false, 1},
                          {5, 1024, true, 1}};
    for (const Case& c : cases)
        for (int na : {1, 3}) {
            g_seen.clear();
            const int32_t zero[3] = {0, 0, 0};
            EXPECT(init(x.data(), N, c.P, c.T, rows, na, 0, nullptr, loc.data()) == SG_OK);
            EXPECT(init(x.data(), N, c.P, c.T, rows, na, 1, zero, loc.data()) == SG_OK);
            EXPECT(select(loss.data(), N, c.P, rows, na, report.data()) == SG_OK);
            const int32_t lead[3] = {-1, c.P - 1, 0};
            EXPECT(move(x.data(), N, c.P, c.T, rows, na, lead, cont, 1, q.data()) == SG_OK);
            EXPECT(move(x.data(), N, c.P, c.T, rows, na, lead, cont, 0, nullptr) == SG_OK);   // the last iteration: nothing moves
            EXPECT(move(x.data(), N, c.P, c.T, rows, na, lead, zero, 1, nullptr) == SG_OK);   // every row found
            EXPECT(g_seen.size() == 6);
            for (size_t i = 0; i < g_seen.size(); ++i) {
                const Launch& l = g_seen[i];
                if (i == 2) {
                    EXPECT(l.name.find("pso_select_kernel") != std::string::npos && l.grid.x == (unsigned)na && l.block.x == 64);
                    continue;
                }
                const std::string want = std::string(i < 2 ? "pso_init_kernel<" : "pso_move_kernel<") + (c.vec ? "4>" : "1>");
                EXPECT(l.name.find(want) != std::string::npos);
                EXPECT(l.grid.x == c.gx && l.grid.y == (unsigned)na && l.grid.z == 1 && l.block.x == 256 && l.lds == 0);
            }
        }
    // a misaligned base keeps a vectorisable T on the scalar kernels
    g_seen.clear();
    EXPECT(init(x.data(), N, 5, 1024, rows, 3, 0, nullptr, loc.data() + 1) == SG_OK);
    EXPECT(move(x.data() + 1, N, 5, 1024, rows, 3, from, cont, 1, q.data()) == SG_OK);
    EXPECT(g_seen.size() == 2 && g_seen[0].name.find("pso_init_kernel<1>") != std::string::npos &&
           g_seen[1].name.find("pso_move_kernel<1>") != std::string::npos && g_seen[0].grid.x == 4 && g_seen[1].grid.x == 4);
    // given draws are taken as they are: the same launches
    g_seen.clear();
    EXPECT(sg_pso_init(ctx, x.data(), lo.data(), hi.data(), N, 5, 1024, rows, 3, 1, best, 7, 0, draws.data(), draws.data(), loc.data(),
                       vel.data(), pbl.data(), pb.data(), q.data(), nullptr) == SG_OK);
    EXPECT(sg_pso_move(ctx, x.data(), lo.data(), hi.data(), N, 5, 1024, rows, 3, from, cont, 1, 0.5f, 1.f, 1.f, 7, 0, draws.data(),
                       draws.data(), imp.data(), loc.data(), vel.data(), pbl.data(), gbl.data(), q.data(), nullptr) == SG_OK);
    EXPECT(g_seen.size() == 2 && g_seen[0].name.find("pso_init_kernel<4>") != std::string::npos &&
           g_seen[1].name.find("pso_move_kernel<4>") != std::string::npos);
    EXPECT(hipdouble_live_allocs() == a0);  // the swarm's calls own no device memory
    // SG_PSO_VEC=1: the scalar kernels at a vectorisable T
    setenv("SG_PSO_VEC", "1", 1);
    g_seen.clear();
    EXPECT(init(x.data(), N, 5, 1024, rows, 3, 0, nullptr, loc.data()) == SG_OK);
    EXPECT(g_seen.size() == 1 && g_seen[0].name.find("pso_init_kernel<1>") != std::string::npos);
    // the library's own rule: 16 bytes per lane from compute units x 512 threads on.  256 units: never at these sizes ...
    unsetenv("SG_PSO_VEC");
    g_seen.clear();
    EXPECT(init(x.data(), N, 5, 1024, rows, 3, 0, nullptr, loc.data()) == SG_OK);
    EXPECT(move(x.data(), N, 5, 1024, rows, 3, from, cont, 1, q.data()) == SG_OK);
    EXPECT(g_seen.size() == 2 && g_seen[0].name.find("pso_init_kernel<1>") != std::string::npos &&
           g_seen[1].name.find("pso_move_kernel<1>") != std::string::npos);
    {   // ... one unit: 3 x 1024 / 4 = 768 threads are enough, 2 x 1024 / 4 = 512 too, 1 x 1024 / 4 = 256 are not
        setenv("HIPDOUBLE_CUS", "1", 1);
        sg_ctx* small = nullptr;
        EXPECT(sg_create(0, &small) == SG_OK && small != nullptr);
        unsetenv("HIPDOUBLE_CUS");
        if (small) {
            const char* want[3] = {"pso_init_kernel<1>", "pso_init_kernel<4>", "pso_init_kernel<4>"};
            for (int na = 1; na <= 3; ++na) {
                g_seen.clear();
                EXPECT(sg_pso_init(small, x.data(), lo.data(), hi.data(), N, 5, 1024, rows, na, 0, nullptr, 7, 0, nullptr, nullptr,
                                   loc.data(), vel.data(), pbl.data(), pb.data(), q.data(), nullptr) == SG_OK);
                EXPECT(g_seen.size() == 1 && g_seen[0].name.find(want[na - 1]) != std::string::npos);
            }
            sg_destroy(small);
        }
    }

    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);
    if (g_fail) return 1;
    std::fprintf(stderr, "pso_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
