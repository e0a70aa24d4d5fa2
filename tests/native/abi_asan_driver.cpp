// Driver of the sanitizer build of the C-ABI's host half (`make asan`; see hip_host_double.cpp): walks the entry points
// of include/speakerguard_hip.h with NULL / malformed / valid arguments under AddressSanitizer + UBSan.  Any sanitizer
// report aborts the process (-fno-sanitize-recover); a failed expectation returns 1.  "Device" buffers are host
// buffers sized exactly as the header says, so an entry point that uploads or downloads past a documented extent is an
// ASan error here.
//
// `abi_asan_driver --launch-table all|device|isolated` is the second mode: it walks the contraction launcher
// (launch_conv_gemm, k_conv_gemm.hip) over the shapes the GPU tests pin and prints one line per conv_gemm* launch the
// double receives -- which kernel, which grid, which arguments.  No kernel runs, so the buffers are dummies.  The output
// of every device / knob setting is recorded in tests/native/conv_launch_table.expected and tests/test_launch_table.py
// compares byte for byte: a changed CHOICE of kernel, which gives the same bits on the GPU, shows here.
//
// `abi_asan_driver --an-sequence all|passes` is the third ("passes": without the sg_an_configure variants): it walks the
// AudioNet entry points (sg_api_audionet.hip) and prints one line per launch of ANY kernel, in order, plus the planned
// fields of AnFusedArgs for the fused CNN kernels -- the four launch forms of the CNN give the same bits too.  Recorded in
// tests/native/an_launch_sequence.expected (tests/test_an_launch_sequence.py).
//
// `abi_asan_driver --loop-sequence` is the fourth: the same lines for the device-resident PGD loops -- sg_xv_pgd_run with and
// without dither, EOT repeats as one pass, as full groups and with a tail group, sg_xv_pgd_run_defended and
// sg_an_pgd_run_defended over identity, per-row, randomised and FeCo chains.  Every launch form of a loop gives the same bits
// too.  Recorded in tests/native/loop_launch_sequence.expected (tests/test_loop_launch_sequence.py).
#include "driver_common.h"
#include "../../speakerguard_amd/csrc/sg_internal.h"  // ConvGemmArgs: the launch table reads the first kernel argument

// ---- the launch table ------------------------------------------------------------------------------------------
static std::string g_case;                 // label of the call being walked: every line carries it
static int g_epi = -1;                     // its epilogue
static std::vector<std::string> g_lines;   // the conv_gemm* launches it made

static void conv_launch(const Launch& l, void** args) {
    std::string name = kernel_name(l.name);  // one token: "conv_gemm_q_kernel<1,2>"
    if (name.find("conv_gemm") != 0) return;
    // the template argument that is the epilogue (the last one of conv_gemm_kernel, the first one of the others) is printed as
    // E where it is the epilogue asked for, so that the three epilogues of a case can share a line; a wrong one stays a number
    const size_t e = name.find("conv_gemm_kernel<") == 0 ? name.size() - 2 : name.find('<') + 1;
    if (name[e] == '0' + g_epi) name[e] = 'E';
    const sg::ConvGemmArgs& a = *static_cast<const sg::ConvGemmArgs*>(args[0]);
    // the scalars after the argument block: stream-K (ntiles, tiles, iters_per_worker; not the epoch, which counts launches),
    // 16 x 16 blocks (ntile32), one block per tile (mtiles, ntiles)
    const int n_scalars = name.find("streamk") != std::string::npos ? 3 : name.find("s16") != std::string::npos ? 1 : 2;
    std::string scalars;
    for (int i = 1; i <= n_scalars; ++i) scalars += (i > 1 ? "," : "") + std::to_string(*static_cast<const int*>(args[i]));
    char line[256];
    std::snprintf(line, sizeof(line), "%s grid=%u,%u,%u block=%u lds=%zu Wq=%d a_bytes=%u w_bytes=%u sk_xcd=%d ablate=%d trace=%d args=%s",
                  name.c_str(), l.grid.x, l.grid.y, l.grid.z, l.block.x, l.lds, a.Wq != nullptr, a.a_bytes, a.w_bytes, a.sk_xcd, a.ablate,
                  a.trace != nullptr, scalars.c_str());
    g_lines.push_back(line);
}

static void begin_case(const std::string& label, int epi) {
    g_case = label;
    g_epi = epi;
    g_lines.clear();
}
// a call that failed, or launched nothing of interest, still leaves a line
static void end_case(sg_ctx* ctx, int rc) {
    if (rc != SG_OK) g_lines.push_back("rc=" + std::to_string(rc) + " " + sg_last_error(ctx));
    else if (g_lines.empty()) g_lines.push_back("no conv_gemm launch");
}
static void print_case(const std::string& label) {
    for (size_t i = 0; i < g_lines.size(); ++i)
        std::printf("%s%s | %s\n", label.c_str(), g_lines.size() > 1 ? (" #" + std::to_string(i + 1)).c_str() : "", g_lines[i].c_str());
}

struct ConvShape { const char* id; int B, Ta, Tc, Kc, N, taps, step, base; };

// One shape with the given kernels, all three epilogues each.  Epilogues of a kernel that launch the same thing -- E in the
// kernel name standing for the epilogue asked for -- share a line, labelled k<kernel> e<epilogues>.
static void walk_conv(sg_ctx* ctx, const ConvShape& c, int kernel_lo, int kernel_hi, const char* prefix = "") {
    static float dummy[4];  // never dereferenced: the double runs no kernel
    for (int kernel = kernel_lo; kernel <= kernel_hi; ++kernel) {
        std::vector<std::pair<std::vector<std::string>, std::string>> groups;  // launches -> the epilogues that made them
        for (int epi = 0; epi <= 2; ++epi) {
            begin_case("", epi);
            end_case(ctx, sg_conv1d_rows(ctx, dummy, dummy, dummy, dummy, dummy, c.B, c.Ta, c.Tc, c.Kc, c.N, c.taps, c.step, c.base, epi, kernel, nullptr));
            auto g = std::find_if(groups.begin(), groups.end(), [](const auto& x) { return x.first == g_lines; });
            if (g == groups.end()) g = groups.insert(g, {g_lines, ""});
            g->second += std::to_string(epi);
        }
        for (const auto& g : groups) {
            g_lines = g.first;
            print_case(std::string(prefix) + c.id + " B=" + std::to_string(c.B) + " k" + std::to_string(kernel) + " e" + g.second);
        }
    }
}

// mode "all": every kernel at every isolated shape, the whole models, fault injection (the default device without knobs);
// "device" / "isolated" (device / knob variants): thinned to the launcher's own choice (kernel 0) everywhere and the forced
// kernels at the eleven shapes where tests/test_gpu_conv.py forces them, with / without the models
static int launch_table(const std::string& mode) {
    setenv("SG_TUNE", "1", 1);  // the knobs of the caller's environment count
    g_on_launch = conv_launch;
    hipdouble_set_launch_hook(record_launch);
    sg_ctx* ctx = nullptr;
    if (sg_create(0, &ctx) != SG_OK) return 1;
    const int batches[9] = {1, 2, 4, 5, 7, 8, 16, 32, 64};
    std::vector<ConvShape> shapes = {  // tests/test_gpu_conv.py::SHAPES
        {"fwd_streamk_dil2", 64, 270, 266, 192, 512, 3, 2, 0},        {"dgrad_streamk_edges", 64, 266, 270, 192, 512, 3, -2, 0},
        {"fwd_streamk_mid_128row", 32, 270, 266, 192, 512, 3, 2, 0},  {"dgrad_streamk_mid_128row", 32, 266, 270, 192, 512, 3, -2, 0},
        {"fwd_streamk_small_64row", 16, 270, 266, 192, 512, 3, 2, 0}, {"dgrad_streamk_small_64row", 16, 266, 270, 192, 512, 3, -2, 0},
        {"fwd_streamk_tiny_32row", 8, 270, 266, 192, 512, 3, 2, 0},   {"dgrad_streamk_tiny_32row", 8, 266, 270, 192, 512, 3, -2, 0},
        {"fwd_small_ragged_tile", 3, 50, 46, 64, 128, 5, 1, 0},       {"dgrad_small", 2, 40, 46, 96, 256, 3, -3, 0},
        {"same_padding_tap_base", 5, 33, 33, 32, 128, 3, 1, -1}};
    for (int b : batches) shapes.push_back({"tdnn3_fwd", b, 288, 270, 512, 512, 7, 3, 0});
    for (int b : batches) shapes.push_back({"tdnn3_dgrad", b, 270, 288, 512, 512, 7, -3, 0});
    const int tdnn1[5][2] = {{64, 300}, {8, 300}, {3, 125}, {1, 100}, {5, 208}};
    for (auto& bf : tdnn1) shapes.push_back({"tdnn1_fwd", bf[0], bf[1], bf[1] - 4, 32, 512, 5, 1, 0});
    for (int b : batches) shapes.push_back({"n1536", b, 270, 270, 512, 1536, 1, 1, 0});
    for (size_t i = 0; i < shapes.size(); ++i) walk_conv(ctx, shapes[i], 0, mode == "all" || i < 11 ? 10 : 0);
    if (mode != "isolated") {
        // one forward + backward of the synthetic x-vector model at the shapes of tests/test_gpu_layers.py (tile 1, split-K fc1,
        // the tdnn1 data gradient), one per-layer pass of AudioNet (tile 1 / 2 by N % 128)
        const int S = 4;
        XvModel xv(24, S);
        if (sg_xv_load(ctx, &xv.desc) != SG_OK) return 1;
        sg_loss_spec ce{};
        std::vector<std::pair<int, int>> grid;
        for (int b : batches) grid.push_back({b, 48000});
        grid.insert(grid.end(), {{9, 52960}, {5, 16123}, {2, 192000}, {3, 16000}});
        for (auto& bt : grid) {
            const int B = bt.first, T = bt.second;
            std::vector<float> x((size_t)B * T), g((size_t)B * T), sc((size_t)B * S), loss(B);
            std::vector<int64_t> y(B, 0), dec(B);
            const std::string label = "xv B=" + std::to_string(B) + " T=" + std::to_string(T);
            begin_case(label, -1);
            end_case(ctx, sg_xv_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, nullptr, dec.data(), sc.data(), loss.data(), g.data(), nullptr));
            print_case(label);
        }
        const int B = 3, T = 16000, Sa = 11;
        AnModel an(Sa);
        if (sg_an_load(ctx, &an.desc) != SG_OK) return 1;
        std::vector<float> x((size_t)B * T), g((size_t)B * T), sc((size_t)B * Sa), loss(B);
        std::vector<int64_t> y(B, 0), dec(B);
        setenv("SG_AN_FUSED", "0", 1);
        begin_case("audionet", -1);
        end_case(ctx, sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), g.data(), nullptr));
        print_case("audionet per layer B=3 T=16000");
    }
    if (mode == "all") {
        // fault injection: a budget of one lost hand-off survives a launch that ends on a tile kernel and marks exactly the
        // next stream-K launch (ablate bit 8); then the context without stream-K
        const ConvShape tile_shape = {"tdnn1_fwd", 64, 300, 296, 32, 512, 5, 1, 0}, sk_shape = shapes[0];  // 5 chunks: a tile launch
        if (sg_debug_lose_handoffs(ctx, 1) != SG_OK) return 1;
        // (three epilogues = three launches per walk: the budget is spent by the first stream-K one, epilogue 0)
        walk_conv(ctx, tile_shape, 0, 0, "lose_handoffs=1 ");
        walk_conv(ctx, sk_shape, 0, 0, "lose_handoffs=1 ");
        if (sg_set_streamk(ctx, 0) != SG_OK) return 1;
        walk_conv(ctx, sk_shape, 0, 10, "set_streamk=0 ");
    }
    sg_destroy(ctx);
    return 0;
}

// ---- the AudioNet launch sequence --------------------------------------------------------------------------------
static std::string g_an_label;
static int g_an_n = 0;

static void an_launch(const Launch& launch, void** args) {
    print_launch(g_an_label, ++g_an_n, launch);
    if (kernel_name(launch.name).find("an_cnn_") == 0) {
        const sg::AnFusedArgs& a = *static_cast<const sg::AnFusedArgs*>(args[0]);
        std::printf(" S=%d buf_floats=%d Fnet=%d head=%d Tin=", a.S, a.buf_floats, a.Fnet, a.head.on);
        for (int l = 0; l < sg::kAnConv; ++l) std::printf("%s%d", l ? "," : "", a.Tin[l]);
        std::printf(" Tout=");
        for (int l = 0; l < sg::kAnConv; ++l) std::printf("%s%d", l ? "," : "", a.Tout[l]);
    }
    std::printf("\n");
}

static void an_case(sg_ctx* ctx, const std::string& label, int rc) {
    if (rc != SG_OK) std::printf("%s #%d | rc=%d %s\n", label.c_str(), ++g_an_n, rc, sg_last_error(ctx));
}
#define AN_CASE(label, call) (g_an_label = (label), g_an_n = 0, an_case(ctx, g_an_label, (call)))

struct AnBuffers {  // "device" buffers of one (B, T) shape, sized as the header says
    int B, T, F;
    std::vector<float> x, g, sc, loss, ltr;
    std::vector<int64_t> y, dec, dtr;
    std::vector<uint8_t> succ;
    AnBuffers(int B_, int T_, int S, int steps)
        : B(B_), T(T_), F(sg_an_num_frames(T_)), x((size_t)B_ * T_), g((size_t)B_ * T_), sc((size_t)B_ * S), loss(B_),
          ltr((size_t)(steps + 1) * B_), y(B_, 0), dec(B_), dtr((size_t)(steps + 1) * B_), succ(B_) {}
};

static void walk_an_passes(sg_ctx* ctx, AnBuffers& b, const std::string& tag, bool all) {
    sg_loss_spec ce{};
    sg_pgd_params pp{};
    pp.step_size = 4e-4f; pp.max_iter = 2; pp.grad_sign = 1; pp.eot_size = 1; pp.eot_batch_size = 1;
    const std::string at = " B=" + std::to_string(b.B) + " T=" + std::to_string(b.T) + tag;
    if (all) {
        AN_CASE("forward" + at, sg_an_forward(ctx, b.x.data(), b.B, b.T, 0, b.dec.data(), b.sc.data(), nullptr, nullptr));
        AN_CASE("loss_grad flag=1" + at, sg_an_loss_grad(ctx, b.x.data(), b.y.data(), b.B, b.F, 1, &ce, b.dec.data(), b.sc.data(), b.loss.data(), b.g.data(), nullptr));
        AN_CASE("loss_grad no grad" + at, sg_an_loss_grad(ctx, b.x.data(), b.y.data(), b.B, b.T, 0, &ce, b.dec.data(), b.sc.data(), b.loss.data(), nullptr, nullptr));
    }
    AN_CASE("loss_grad flag=0" + at, sg_an_loss_grad(ctx, b.x.data(), b.y.data(), b.B, b.T, 0, &ce, b.dec.data(), b.sc.data(), b.loss.data(), b.g.data(), nullptr));
    AN_CASE("pgd_run" + at, sg_an_pgd_run(ctx, b.x.data(), b.y.data(), b.x.data(), b.x.data(), b.B, b.T, &pp, b.succ.data(), b.dec.data(), b.sc.data(),
                                          b.loss.data(), b.ltr.data(), b.dtr.data(), nullptr));
}

static void walk_an_feco(sg_ctx* ctx, AnBuffers& b, int k, bool random_eot2, bool trace, const std::string& tag) {
    sg_pgd_params pp{};
    pp.step_size = 4e-4f; pp.max_iter = 2; pp.grad_sign = 1; pp.eot_size = random_eot2 ? 2 : 1; pp.eot_batch_size = 1;
    sg_feco_params fp{};
    fp.k = k; fp.max_iter = 3; fp.random_init = random_eot2; fp.seed = 5;
    AN_CASE("pgd_run_feco B=" + std::to_string(b.B) + " T=" + std::to_string(b.T) + " k=" + std::to_string(k) + (random_eot2 ? " random eot=2" : " even") +
                (trace ? " trace" : "") + tag,
            sg_an_pgd_run_feco(ctx, b.x.data(), b.y.data(), b.x.data(), b.x.data(), b.B, b.T, &pp, &fp, b.succ.data(), b.dec.data(), b.sc.data(), b.loss.data(),
                               trace ? b.ltr.data() : nullptr, trace ? b.dtr.data() : nullptr, nullptr));
}

// One context per shape: the workspace keeps the largest batch and the longest utterance it has seen, and the two extremes
// below together would not fit the sanitizer build.
static int an_sequence(bool configure) {
    g_on_launch = an_launch;
    hipdouble_set_launch_hook(record_launch);
    const int Sa = 11;
    AnModel an(Sa);
    // (B, T): three small / odd shapes, the benchmark's, a batch at which the planner cuts S = 1 by itself, and an utterance of
    // 180 s that no cut fits (the per-layer sequence)
    const int shapes[6][2] = {{3, 16000}, {5, 40000}, {64, 48000}, {256, 16000}, {1, 2880000}, {4, 16000}};
    for (auto& bt : shapes) {
        sg_ctx* ctx = nullptr;
        if (sg_create(0, &ctx) != SG_OK || sg_an_load(ctx, &an.desc) != SG_OK) return 1;
        AnBuffers b(bt[0], bt[1], Sa, 2);
        if (b.B != 4) walk_an_passes(ctx, b, "", true);
        if (b.B == 4)
            for (int k : {30, b.F / 2})
                for (int random_eot2 = 0; random_eot2 <= 1; ++random_eot2)
                    for (int trace = 0; trace <= 1; ++trace) walk_an_feco(ctx, b, k, random_eot2, trace, "");
        if (configure && (b.B == 3 || b.B == 64 || b.B == 4)) {  // the front-end's settings (sg_an_configure): its kernels are part of the sequence
            const int cfgs[4][3] = {{32, -1, 0}, {32, -1, 1}, {32, 0, -1}, {64, -1, -1}};
            for (auto& c : cfgs) {
                if (sg_an_configure(ctx, c[0], c[1], c[2]) != SG_OK) return 1;
                const std::string tag = " fft=" + std::to_string(c[0]) + " cache=" + std::to_string(c[1]) + " ola=" + std::to_string(c[2]);
                if (b.B == 4) walk_an_feco(ctx, b, 30, false, false, tag);
                else walk_an_passes(ctx, b, tag, false);
            }
        }
        sg_destroy(ctx);
    }
    {   // FeCo where the front-end's frames and the k frames the network sees plan differently: 18000 frames fit no cut, 30 do
        sg_ctx* ctx = nullptr;
        if (sg_create(0, &ctx) != SG_OK || sg_an_load(ctx, &an.desc) != SG_OK) return 1;
        AnBuffers b(2, 2880000, Sa, 2);
        walk_an_feco(ctx, b, 30, false, true, "");
        sg_destroy(ctx);
    }
    return 0;
}

// ---- the device loops' launch sequence ----------------------------------------------------------------------------
// SG_EOT_MAX_ROWS is read at every call (behind SG_TUNE=1): 0 = unset
static void eot_max_rows(int rows) {
    if (rows > 0) setenv("SG_EOT_MAX_ROWS", std::to_string(rows).c_str(), 1);
    else unsetenv("SG_EOT_MAX_ROWS");
}

static int loop_sequence() {
    setenv("SG_TUNE", "1", 1);
    unsetenv("SG_EOT_MAX_ROWS");
    g_on_launch = an_launch;
    hipdouble_set_launch_hook(record_launch);
    const int K = 2;
    const sg_wav_stage lpf = lpf_stage();
    const auto td = [](int kind, float param) { return ::td(kind, param, 17); };
    const sg_wav_stage qt = td(SG_TD_QT, 512.f), bdr = td(SG_TD_QT, 256.f) /* BDR to 8 of 16 bits */, ms = td(SG_TD_MS, 3.f), at = td(SG_TD_AT, 25.f);
    const sg_wav_stage qt_bdr[2] = {qt, bdr}, qt_ms_lpf[3] = {qt, ms, lpf}, lpf_qt[2] = {lpf, qt};
    const sg_wav_stage eight[SG_WAV_CHAIN_MAX] = {td(SG_TD_MS, 5.f), td(SG_TD_AS, 31.f), td(SG_TD_QT, 256.f), lpf, at, td(SG_TD_QT, 128.f), ms, lpf};
    sg_pgd_params base{};
    base.step_size = 4e-4f; base.max_iter = K; base.grad_sign = 1; base.eot_size = 1; base.eot_batch_size = 1;
    {   // ---- x-vector, the shape of defended_asan_driver.cpp
        const int B = 3, T = 5043, S = 4;
        sg_ctx* ctx = nullptr;
        XvModel xv(24, S);
        if (sg_create(0, &ctx) != SG_OK || sg_xv_load(ctx, &xv.desc) != SG_OK) return 1;
        std::vector<float> x = rnd((size_t)B * T, 200, 0.3f), lower = x, upper = x, scores((size_t)B * S), loss(B), ltr((size_t)(K + 1) * B);
        std::vector<int64_t> y(B, 1), dec(B), dtr((size_t)(K + 1) * B);
        std::vector<uint8_t> succ(B);
        const std::string at_shape = " B=" + std::to_string(B) + " T=" + std::to_string(T);
        // dither: 0 = none, 1 = dither 1 with eot_size 4; eot: eot_size without dither (AT's repeats)
        auto params = [&](bool dither, int eot, int max_iter) {
            sg_pgd_params pp = base;
            pp.max_iter = max_iter;
            pp.eot_size = dither ? 4 : eot;
            if (dither) { pp.dither.dither = 1.0f; pp.dither.seed = 99; pp.dither.index_base = 5; }
            return pp;
        };
        auto run = [&](const std::string& label, const sg_pgd_params& pp, bool trace, int max_rows) {
            eot_max_rows(max_rows);
            AN_CASE("xv_pgd_run" + at_shape + " " + label,
                    sg_xv_pgd_run(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, succ.data(), dec.data(), scores.data(), loss.data(),
                                  trace ? ltr.data() : nullptr, trace ? dtr.data() : nullptr, nullptr));
        };
        auto run_def = [&](const std::string& label, const sg_wav_stage* chain, int n, const sg_pgd_params& pp, int max_rows) {
            eot_max_rows(max_rows);
            AN_CASE("xv_pgd_run_defended" + at_shape + " " + label,
                    sg_xv_pgd_run_defended(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, chain, n, succ.data(), dec.data(),
                                           scores.data(), loss.data(), ltr.data(), dtr.data(), nullptr));
        };
        run("no dither trace", params(false, 1, K), true, 0);
        run("no dither", params(false, 1, K), false, 0);
        run("dither eot=4 G=4", params(true, 4, K), true, 0);
        run("dither eot=4 max_rows=6 G=2", params(true, 4, K), true, 6);
        run("dither eot=4 max_rows=9 G=3 tail", params(true, 4, K), true, 9);
        run("max_iter=0", params(false, 1, 0), true, 0);
        run_def("QT", &qt, 1, params(false, 1, K), 0);
        run_def("QT,BDR", qt_bdr, 2, params(false, 1, K), 0);
        run_def("QT,BDR dither eot=4", qt_bdr, 2, params(true, 4, K), 0);
        run_def("MS", &ms, 1, params(false, 1, K), 0);
        run_def("LPF clip=range", &lpf, 1, params(false, 1, K), 0);
        run_def("QT,MS,LPF dither eot=4", qt_ms_lpf, 3, params(true, 4, K), 0);
        run_def("AT eot=4", &at, 1, params(false, 4, K), 0);
        run_def("AT eot=4 max_rows=9", &at, 1, params(false, 4, K), 9);
        run_def("8 stages eot=4", eight, SG_WAV_CHAIN_MAX, params(false, 4, K), 0);
        run_def("MS max_iter=0", &ms, 1, params(false, 1, 0), 0);
        eot_max_rows(0);
        sg_destroy(ctx);
    }
    {   // ---- AudioNet: 64 log-mel frames, so that FeCo's k = 32 passes the stack
        const int B = 4, T = 10081, Sa = 5;
        sg_ctx* ctx = nullptr;
        AnModel an(Sa);
        if (sg_create(0, &ctx) != SG_OK || sg_an_load(ctx, &an.desc) != SG_OK) return 1;
        AnBuffers b(B, T, Sa, K);
        const std::string at_shape = " B=" + std::to_string(B) + " T=" + std::to_string(T);
        auto run = [&](const std::string& label, const sg_wav_stage* chain, int n, const sg_feco_params* f, int eot, int max_iter, bool trace, int max_rows) {
            sg_pgd_params pp = base;
            pp.max_iter = max_iter;
            pp.eot_size = eot;
            eot_max_rows(max_rows);
            AN_CASE("an_pgd_run_defended" + at_shape + " " + label,
                    sg_an_pgd_run_defended(ctx, b.x.data(), b.y.data(), b.x.data(), b.x.data(), B, T, &pp, chain, n, f, b.succ.data(), b.dec.data(),
                                           b.sc.data(), b.loss.data(), trace ? b.ltr.data() : nullptr, trace ? b.dtr.data() : nullptr, nullptr));
        };
        sg_feco_params even{}, random{};
        even.k = 32; even.max_iter = 3; even.random_init = 0; even.seed = 5;
        random = even;
        random.random_init = 1;
        run("QT", &qt, 1, nullptr, 1, K, true, 0);
        run("MS", &ms, 1, nullptr, 1, K, true, 0);
        run("LPF,QT", lpf_qt, 2, nullptr, 1, K, true, 0);
        run("AT eot=4", &at, 1, nullptr, 4, K, true, 0);
        run("AT eot=4 max_rows=12 G=3 tail", &at, 1, nullptr, 4, K, true, 12);
        run("QT feco k=32 even", &qt, 1, &even, 1, K, true, 0);
        run("MS feco k=32 random eot=2 trace", &ms, 1, &random, 2, K, true, 0);
        run("MS feco k=32 random eot=2", &ms, 1, &random, 2, K, false, 0);
        run("MS max_iter=0", &ms, 1, nullptr, 1, 0, true, 0);
        eot_max_rows(0);
        sg_destroy(ctx);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--launch-table") return launch_table(argv[2]);
    if (argc == 3 && std::string(argv[1]) == "--an-sequence") return an_sequence(std::string(argv[2]) == "all");
    if (argc == 2 && std::string(argv[1]) == "--loop-sequence") return loop_sequence();
    setenv("SG_TUNE", "1", 1);  // the knobs this walk sets (SG_EOT_MAX_ROWS, SG_AN_SLICES, SG_AN_FUSED) count only behind it
    // ---- no context ------------------------------------------------------------------------------------------
    EXPECT(sg_version() == 100);
    EXPECT(sg_xv_num_frames(48000) == 300 && sg_xv_num_frames(100) == 0 && sg_an_num_frames(48000) == 300);
    EXPECT(sg_last_error(nullptr) != nullptr);
    sg_destroy(nullptr);
    EXPECT(sg_create(0, nullptr) == SG_ERR_ARG);
    sg_ctx* none = nullptr;
    EXPECT(sg_create(7, &none) == SG_ERR_HIP && none == nullptr);  // the double has one device
    EXPECT(sg_create(-1, &none) == SG_ERR_HIP && none == nullptr);
    float f4[4] = {0};
    int64_t i4[4] = {0};
    sg_loss_spec ce{};
    sg_dither nod{};
    sg_pgd_params pp{};
    sg_feco_params fp{};
    EXPECT(sg_sync(nullptr, nullptr) != SG_OK && sg_health(nullptr) != SG_OK);
    EXPECT(sg_xv_load(nullptr, nullptr) != SG_OK && sg_an_load(nullptr, nullptr) != SG_OK);
    EXPECT(sg_xv_forward(nullptr, f4, 1, 48000, 0, &nod, i4, f4, nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_xv_loss_grad(nullptr, f4, i4, 1, 48000, 0, &ce, &nod, i4, f4, f4, f4, nullptr) != SG_OK);
    EXPECT(sg_xv_pgd_run(nullptr, f4, i4, f4, f4, 1, 48000, &pp, nullptr, i4, f4, f4, nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_an_pgd_run(nullptr, f4, i4, f4, f4, 1, 48000, &pp, nullptr, i4, f4, f4, nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_an_pgd_run_feco(nullptr, f4, i4, f4, f4, 2, 48000, &pp, &fp, nullptr, i4, f4, f4, nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_pgd_update(nullptr, f4, f4, f4, f4, 4, 0.1f, 1, nullptr) != SG_OK);
    EXPECT(sg_trace_begin(nullptr, 4) != SG_OK && sg_trace_end(nullptr, nullptr, nullptr, 0, nullptr) != SG_OK);
    EXPECT(sg_conv1d_rows(nullptr, f4, f4, f4, nullptr, nullptr, 1, 1, 1, 32, 128, 1, 1, 0, 0, 0, nullptr) != SG_OK);
    EXPECT(sg_feco_kmeans(nullptr, f4, 1, 4, 1, 2, 3, nullptr, nullptr) != SG_OK);
    EXPECT(sg_wav_finalize(nullptr, f4, f4, 1, 4, nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_eer_threshold(nullptr, f4, 4, f4, 4, nullptr, nullptr) != SG_OK);

    // ---- a context on the host double -----------------------------------------------------------------------
    sg_ctx* ctx = nullptr;
    EXPECT(sg_create(0, &ctx) == SG_OK && ctx != nullptr);
    if (!ctx) return 1;
    EXPECT(std::strlen(sg_last_error(ctx)) == 0);
    const int B = 3, T = 16000, F = sg_xv_num_frames(T), D = 24, S = 4;
    std::vector<float> x = rnd((size_t)B * T, 200, 0.3f), lower = x, upper = x, grad((size_t)B * T), scores((size_t)B * S), loss(B);
    std::vector<int64_t> y(B, 1), dec(B);
    std::vector<uint8_t> succ(B);

    // state errors come with a message, and the message outlives the next successful call
    EXPECT(sg_xv_forward(ctx, x.data(), B, T, 0, &nod, dec.data(), scores.data(), nullptr, nullptr, nullptr) == SG_ERR_STATE);
    const char* msg = sg_last_error(ctx);
    EXPECT(msg && std::strlen(msg) > 0);
    std::string kept = msg;
    EXPECT(sg_health(ctx) == SG_OK);
    EXPECT(kept == sg_last_error(ctx));

    // malformed weight descriptors
    {
        XvModel m(D, S);
        sg_xv_weights bad = m.desc;
        bad.fc1_weight = nullptr;
        EXPECT(sg_xv_load(ctx, &bad) != SG_OK);
        bad = m.desc; bad.D = 0;
        EXPECT(sg_xv_load(ctx, &bad) != SG_OK);
        bad = m.desc; bad.S = 0;
        EXPECT(sg_xv_load(ctx, &bad) != SG_OK);
        bad = m.desc; bad.tdnn_weight[3] = nullptr;
        EXPECT(sg_xv_load(ctx, &bad) != SG_OK);
        EXPECT(sg_xv_load(ctx, nullptr) != SG_OK);
    }
    XvModel xv(D, S);
    EXPECT(sg_xv_load(ctx, &xv.desc) == SG_OK);  // BatchNorm folding, tap-major / transposed / k4-packed layouts, uploads
    EXPECT(sg_xv_load(ctx, &xv.desc) == SG_OK);  // reload: the old model's allocations are released
    std::vector<float> enr2 = rnd((size_t)2 * D, 300);
    EXPECT(sg_xv_set_enroll(ctx, enr2.data(), 2, 1.5f) == SG_OK);
    EXPECT(sg_xv_set_enroll(ctx, nullptr, 0, 1.5f) != SG_OK || true);  // either refused or a threshold-only update: must not crash
    EXPECT(sg_xv_set_enroll(ctx, xv.enroll.data(), S, -INFINITY) == SG_OK);
    EXPECT(sg_xv_enroll_override(ctx, enr2.data(), 2) == SG_OK && sg_xv_enroll_override(ctx, nullptr, 0) == SG_OK);

    {
        int32_t dm[4] = {-1, -1, -1, -1};
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DEMB, nullptr, 0, dm, nullptr) == SG_ERR_STATE && dm[0] == -1);  // no pass yet
    }
    // shape validation of the pass entry points
    EXPECT(sg_xv_forward(ctx, x.data(), 0, T, 0, &nod, dec.data(), scores.data(), nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_xv_forward(ctx, x.data(), B, 100, 0, &nod, dec.data(), scores.data(), nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_xv_forward(ctx, x.data(), B, T, 5, &nod, dec.data(), scores.data(), nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_xv_forward(ctx, nullptr, B, T, 0, &nod, dec.data(), scores.data(), nullptr, nullptr, nullptr) != SG_OK);
    EXPECT(sg_xv_forward(ctx, x.data(), B, 8, 1, &nod, dec.data(), scores.data(), nullptr, nullptr, nullptr) != SG_OK);  // 8 frames < TDNN context
    EXPECT(std::strlen(sg_last_error(ctx)) > 0);
    // valid passes: workspace sizing, table builders (MFCC tables in torchaudio's float32 operation order), launch selection
    const long l0 = hipdouble_launches();
    EXPECT(sg_xv_forward(ctx, x.data(), B, T, 0, &nod, dec.data(), scores.data(), nullptr, nullptr, nullptr) == SG_OK);
    EXPECT(hipdouble_launches() > l0 + 8);
    std::vector<float> emb((size_t)B * D), temb((size_t)B * 512), feats((size_t)B * F * 30), gfeat((size_t)B * F * 30);
    EXPECT(sg_xv_forward(ctx, x.data(), B, T, 0, nullptr, nullptr, nullptr, emb.data(), temb.data(), nullptr) == SG_OK);
    EXPECT(sg_xv_mfcc(ctx, x.data(), B, T, nullptr, &nod, feats.data(), nullptr) == SG_OK);
    EXPECT(sg_xv_cmvn(ctx, feats.data(), B, F, gfeat.data(), nullptr) == SG_OK);
    EXPECT(sg_xv_forward(ctx, feats.data(), B, F, 1, nullptr, dec.data(), scores.data(), nullptr, nullptr, nullptr) == SG_OK);
    EXPECT(sg_xv_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, &nod, dec.data(), scores.data(), loss.data(), grad.data(), nullptr) == SG_OK);
    EXPECT(sg_xv_loss_grad(ctx, feats.data(), y.data(), B, F, 2, &ce, nullptr, dec.data(), scores.data(), loss.data(), gfeat.data(), nullptr) == SG_OK);
    {
        // the backward workspace of that call, at the pass's own B and F (the workspace was sized by the waveform passes above)
        int32_t dm[4] = {};
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DFEATS, nullptr, 0, dm, nullptr) == SG_OK && dm[0] == 10 && dm[1] == B && dm[2] == F && dm[3] == 32);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DSTATS, nullptr, 0, dm, nullptr) == SG_OK && dm[0] == 8 && dm[1] == B && dm[2] == 1 && dm[3] == 3072);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DACT1 + 4, nullptr, 0, dm, nullptr) == SG_OK && dm[0] == 1 && dm[2] == F - 30 && dm[3] == 1536);
        // a capacity past what the pass wrote is clamped: exact-size destinations, so the sanitizer sees any overrun
        std::vector<float> slabs((size_t)10 * B * F * 32), d5((size_t)B * (F - 30) * 1536), de((size_t)B * 512), few(7);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DFEATS, slabs.data(), (int64_t)1 << 40, nullptr, nullptr) == SG_OK);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DACT1 + 4, d5.data(), (int64_t)d5.size() + 1, nullptr, nullptr) == SG_OK);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DEMB, de.data(), (int64_t)1 << 40, dm, nullptr) == SG_OK && dm[3] == 512);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DSTATS, few.data(), (int64_t)few.size(), nullptr, nullptr) == SG_OK);  // a short one
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DEMB, de.data(), 0, nullptr, nullptr) == SG_ERR_ARG);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DEMB, de.data(), -5, nullptr, nullptr) == SG_ERR_ARG);
        EXPECT(sg_xv_debug_gradient(ctx, 9, nullptr, 0, dm, nullptr) == SG_ERR_ARG && sg_xv_debug_gradient(ctx, -1, nullptr, 0, dm, nullptr) == SG_ERR_ARG);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DFEATS_RAW, nullptr, 0, dm, nullptr) == SG_ERR_ARG);  // a feature-level pass wrote none
        EXPECT(sg_xv_debug_gradient(nullptr, SG_GRAD_DEMB, nullptr, 0, dm, nullptr) != SG_OK);
        // a forward-only pass since: act[] is the new pass's, dact[] the old one's -- refused, both forms of forward-only
        EXPECT(sg_xv_forward(ctx, feats.data(), B, F, 1, nullptr, dec.data(), scores.data(), nullptr, nullptr, nullptr) == SG_OK);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DEMB, de.data(), (int64_t)de.size(), dm, nullptr) == SG_ERR_STATE);
        EXPECT(sg_xv_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, &nod, dec.data(), scores.data(), loss.data(), grad.data(), nullptr) == SG_OK);
        std::vector<float> raw((size_t)B * F * 30);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DFEATS_RAW, raw.data(), (int64_t)raw.size() + 9, dm, nullptr) == SG_OK && dm[2] == F && dm[3] == 30);
        EXPECT(sg_xv_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, &nod, dec.data(), scores.data(), loss.data(), nullptr, nullptr) == SG_OK);
        EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DEMB, de.data(), (int64_t)de.size(), dm, nullptr) == SG_ERR_STATE);
    }
    EXPECT(sg_xv_loss_grad(ctx, x.data(), nullptr, B, T, 0, &ce, &nod, dec.data(), scores.data(), loss.data(), grad.data(), nullptr) != SG_OK);
    // round 6: the same pass on the float64 transforms (the launch selection of both instantiations runs under the sanitizer)
    EXPECT(sg_xv_configure(ctx, 64) == SG_OK);
    EXPECT(sg_xv_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, &nod, dec.data(), scores.data(), loss.data(), grad.data(), nullptr) == SG_OK);
    EXPECT(sg_xv_configure(ctx, 32) == SG_OK);
    sg_loss_spec lin{};
    lin.loss = SG_LOSS_LINEAR;  // needs a coefficient table
    EXPECT(sg_xv_loss_grad(ctx, x.data(), y.data(), B, T, 0, &lin, &nod, dec.data(), scores.data(), loss.data(), grad.data(), nullptr) != SG_OK);
    {
        int32_t rows = 0, ch = 0;
        std::vector<float> act((size_t)B * 300 * 1536);
        EXPECT(sg_xv_debug_activation(ctx, 5, act.data(), (int64_t)act.size(), &rows, &ch, nullptr) == SG_OK && ch == 1536 && rows > 0);
        EXPECT(sg_xv_debug_activation(ctx, 9, act.data(), (int64_t)act.size(), &rows, &ch, nullptr) != SG_OK);
    }
    // the fused loop: parameter validation, EOT grouping, per-step records, stage trace
    pp = sg_pgd_params{};
    pp.step_size = 4e-4f; pp.max_iter = 2; pp.grad_sign = 1; pp.eot_size = 4; pp.eot_batch_size = 3;
    EXPECT(sg_xv_pgd_run(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, succ.data(), dec.data(), scores.data(), loss.data(),
                         nullptr, nullptr, nullptr) == SG_ERR_ARG);  // EOT size not divisible
    pp.eot_batch_size = 2;
    pp.max_iter = -1;
    EXPECT(sg_xv_pgd_run(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, succ.data(), dec.data(), scores.data(), loss.data(),
                         nullptr, nullptr, nullptr) == SG_ERR_ARG);
    pp.max_iter = 2;
    pp.dither.dither = 1.0f; pp.dither.seed = 99; pp.dither.index_base = 5;
    std::vector<float> ltr((size_t)3 * B);
    std::vector<int64_t> dtr((size_t)3 * B);
    EXPECT(sg_trace_begin(ctx, 0) == SG_ERR_ARG && sg_trace_begin(ctx, 1 << 21) == SG_ERR_ARG);
    int32_t n_rec = -1;
    EXPECT(sg_trace_end(ctx, nullptr, nullptr, 0, &n_rec) == SG_ERR_STATE);
    EXPECT(sg_trace_begin(ctx, 16) == SG_OK);
    EXPECT(sg_xv_pgd_run(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, succ.data(), dec.data(), scores.data(), loss.data(),
                         ltr.data(), dtr.data(), nullptr) == SG_OK);
    int32_t tags[16];
    float ms[16];
    EXPECT(sg_trace_end(ctx, tags, ms, 16, &n_rec) == SG_OK && n_rec == 16);  // more launches than records: capped, no overrun
    EXPECT(sg_xv_debug_gradient(ctx, SG_GRAD_DEMB, nullptr, 0, nullptr, nullptr) == SG_ERR_STATE);  // a device loop is no single pass
    EXPECT(sg_trace_begin(ctx, 4096) == SG_OK);
    setenv("SG_EOT_MAX_ROWS", "6", 1);  // two groups of two repeats: the per-step records collect rows over the groups
    EXPECT(sg_xv_pgd_run(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, succ.data(), dec.data(), scores.data(), loss.data(),
                         ltr.data(), dtr.data(), nullptr) == SG_OK);
    unsetenv("SG_EOT_MAX_ROWS");
    std::vector<int32_t> tg(4096);
    std::vector<float> tm(4096);
    EXPECT(sg_trace_end(ctx, tg.data(), tm.data(), 2, &n_rec) == SG_OK && n_rec > 40);  // capacity smaller than the record count
    {
        float ms_l = 0;
        double fl = 0;
        int32_t rows = 0;
        EXPECT(sg_xv_time_layer(ctx, 3, B, T, 2, &ms_l, &fl, &rows, nullptr) == SG_OK && fl > 0);
        EXPECT(sg_xv_time_layer(ctx, -1, B, T, 2, &ms_l, &fl, &rows, nullptr) == SG_OK);
        EXPECT(sg_xv_time_layer(ctx, 7, B, T, 2, &ms_l, &fl, &rows, nullptr) != SG_OK);
        EXPECT(sg_xv_time_layer(ctx, 3, 64, 48000, 2, &ms_l, &fl, &rows, nullptr) == SG_ERR_STATE);  // beyond the resident workspace
    }
    // larger batches walk the other launch strategies (stream-K kinds by tile count)
    for (int b : {1, 8, 16, 64}) {
        std::vector<float> xb = rnd((size_t)b * 48000, 400 + b, 0.3f), gb((size_t)b * 48000), sb((size_t)b * S), lb(b);
        std::vector<int64_t> yb(b, 0), db(b);
        EXPECT(sg_xv_loss_grad(ctx, xb.data(), yb.data(), b, 48000, 0, &ce, nullptr, db.data(), sb.data(), lb.data(), gb.data(), nullptr) == SG_OK);
    }

    // attack-state updates
    EXPECT(sg_pgd_update(ctx, x.data(), grad.data(), lower.data(), upper.data(), (int64_t)B * T, 4e-4f, 1, nullptr) == SG_OK);
    EXPECT(sg_pgd_update(ctx, x.data(), grad.data(), lower.data(), upper.data(), 0, 4e-4f, 1, nullptr) != SG_OK);
    {
        std::vector<float> mod((size_t)B * T), ea((size_t)B * T), es((size_t)B * T), nxt((size_t)B * T), l2(B), cst(B, 1e-3f);
        EXPECT(sg_cw2_step(ctx, mod.data(), nullptr, nullptr, x.data(), nullptr, nullptr, cst.data(), B, T, 1e-2f, 0, nxt.data(), l2.data(), nullptr) == SG_OK);
        EXPECT(sg_cw2_step(ctx, mod.data(), ea.data(), es.data(), x.data(), nxt.data(), grad.data(), cst.data(), B, T, 1e-2f, 1, nxt.data(), l2.data(), nullptr) == SG_OK);
        EXPECT(sg_cw2_step(ctx, nullptr, ea.data(), es.data(), x.data(), nxt.data(), grad.data(), cst.data(), B, T, 1e-2f, 1, nxt.data(), l2.data(), nullptr) != SG_OK);
        const int half = 2, Q = 2 * half + 1;
        std::vector<float> q((size_t)B * Q * T), nl((size_t)B * Q), lr(B, 1e-3f);
        EXPECT(sg_nes_queries(ctx, x.data(), B, T, half, 1, 1e-3f, 7, 0, 0, nullptr, q.data(), nullptr, nullptr) == SG_OK);
        EXPECT(sg_nes_queries(ctx, x.data(), B, T, 0, 1, 1e-3f, 7, 0, 0, nullptr, q.data(), nullptr, nullptr) != SG_OK);
        EXPECT(sg_nes_grad(ctx, nl.data(), B, T, half, 1, 7, 0, 0, nullptr, 0, 1e-3f, 1, grad.data(), nullptr) == SG_OK);
        EXPECT(sg_fakebob_step(ctx, x.data(), grad.data(), ea.data(), lr.data(), lower.data(), upper.data(), B, T, 0.9f, 0.1f, 1, nullptr) == SG_OK);
        std::vector<float> ds((size_t)B * S);
        EXPECT(sg_loss_eval(ctx, scores.data(), y.data(), B, S, -INFINITY, &ce, dec.data(), loss.data(), ds.data(), nullptr) == SG_OK);
        EXPECT(sg_loss_eval(ctx, scores.data(), y.data(), B, 0, -INFINITY, &ce, dec.data(), loss.data(), ds.data(), nullptr) != SG_OK);
    }

    // the convolution primitive: shape rules
    {
        const int Bc = 2, Ta = 40, taps = 3, Kc = 64, N = 128, Tc = Ta - 2;
        std::vector<float> a((size_t)Bc * Ta * Kc), w((size_t)taps * Kc * N), c((size_t)Bc * Tc * N), bias(N);
        EXPECT(sg_conv1d_rows(ctx, a.data(), w.data(), c.data(), bias.data(), nullptr, Bc, Ta, Tc, Kc, N, taps, 1, 0, 1, 0, nullptr) == SG_OK);
        EXPECT(sg_conv1d_rows(ctx, a.data(), w.data(), c.data(), bias.data(), nullptr, Bc, Ta, Tc, 48, N, taps, 1, 0, 1, 0, nullptr) == SG_ERR_ARG);
        EXPECT(sg_conv1d_rows(ctx, a.data(), w.data(), c.data(), bias.data(), nullptr, Bc, Ta, Tc, Kc, 100, taps, 1, 0, 1, 0, nullptr) == SG_ERR_ARG);
        EXPECT(sg_conv1d_rows(ctx, a.data(), w.data(), c.data(), nullptr, nullptr, Bc, Ta, Tc, Kc, N, taps, 1, 0, 1, 0, nullptr) == SG_ERR_ARG);  // epi 1 without bias
        EXPECT(sg_conv1d_rows(ctx, a.data(), w.data(), c.data(), bias.data(), nullptr, Bc, Ta, Tc, Kc, N, taps, 1, 0, 1, 11, nullptr) == SG_ERR_ARG);
        for (int kern = 1; kern <= 5; ++kern)
            EXPECT(sg_conv1d_rows(ctx, a.data(), w.data(), c.data(), bias.data(), nullptr, Bc, Ta, Tc, Kc, N, taps, 1, 0, 1, kern, nullptr) == SG_OK);
    }

    // ---- AudioNet ------------------------------------------------------------------------------------------
    {
        const int Sa = 11, Fa = sg_an_num_frames(T);
        std::vector<float> sc((size_t)B * Sa), fe((size_t)B * Fa * 32), em((size_t)B * 32);
        EXPECT(sg_an_forward(ctx, x.data(), B, T, 0, dec.data(), sc.data(), nullptr, nullptr) == SG_ERR_STATE);
        AnModel an(Sa);
        sg_an_weights bad = an.desc;
        bad.num_class = 0;
        EXPECT(sg_an_load(ctx, &bad) == SG_ERR_ARG);
        bad = an.desc; bad.bn_var[6] = nullptr;
        EXPECT(sg_an_load(ctx, &bad) == SG_ERR_ARG);
        EXPECT(sg_an_load(ctx, &an.desc) == SG_OK);
        EXPECT(sg_an_forward(ctx, x.data(), B, T, 0, dec.data(), sc.data(), em.data(), nullptr) == SG_OK);
        EXPECT(sg_an_forward(ctx, x.data(), B, 500, 0, dec.data(), sc.data(), em.data(), nullptr) == SG_ERR_ARG);  // shorter than one STFT frame
        EXPECT(sg_an_forward(ctx, x.data(), B, T, 2, dec.data(), sc.data(), em.data(), nullptr) == SG_ERR_ARG);
        EXPECT(sg_an_logmel(ctx, x.data(), B, T, fe.data(), nullptr) == SG_OK);
        EXPECT(sg_an_forward(ctx, fe.data(), B, Fa, 1, dec.data(), sc.data(), em.data(), nullptr) == SG_OK);
        EXPECT(sg_an_forward(ctx, fe.data(), B, 20, 1, dec.data(), sc.data(), em.data(), nullptr) == SG_ERR_ARG);  // too few frames for conv8
        EXPECT(sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
        {   // the fused CNN kernels' planner (time slices, LDS demand) for forced cuts, and the per-layer sequence it replaces
            const long l1 = hipdouble_launches();
            setenv("SG_AN_SLICES", "7", 1);
            EXPECT(sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
            setenv("SG_AN_SLICES", "1000", 1);  // more slices than conv8 has rows: clamped
            EXPECT(sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
            unsetenv("SG_AN_SLICES");
            const long fused = hipdouble_launches() - l1;
            setenv("SG_AN_FUSED", "0", 1);
            const long l2 = hipdouble_launches();
            EXPECT(sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
            unsetenv("SG_AN_FUSED");
            EXPECT(hipdouble_launches() - l2 > fused / 2 + 10);  // ~28 launches per pass pair against ~8
            // the workspace of that per-layer call (sg_an_debug_gradient): exact-size destinations, so the sanitizer sees any overrun
            int32_t dm[4] = {-1, -1, -1, -1};
            const long l3 = hipdouble_launches();
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DPRE, nullptr, 0, dm, nullptr) == SG_OK && dm[0] == 1 && dm[1] == B && dm[2] == Fa && dm[3] == 32);
            std::vector<float> dpre((size_t)B * Fa * 32);
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DPRE, dpre.data(), (int64_t)dpre.size(), nullptr, nullptr) == SG_OK);
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_PRE, dpre.data(), (int64_t)dpre.size() + 3, nullptr, nullptr) == SG_OK);
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DPRE, dpre.data(), (int64_t)dpre.size() - 1, nullptr, nullptr) == SG_ERR_ARG);  // too small: refused, not cut
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DPRE, dpre.data(), 0, nullptr, nullptr) == SG_ERR_ARG);
            for (int which = SG_AN_GRAD_DACT1; which <= SG_AN_GRAD_ACT6_UNPOOLED; ++which) {
                EXPECT(sg_an_debug_gradient(ctx, which, nullptr, 0, dm, nullptr) == SG_OK && dm[1] == B && dm[2] >= 1 && dm[3] >= 32);
                std::vector<float> buf((size_t)dm[1] * dm[2] * dm[3]);
                EXPECT(sg_an_debug_gradient(ctx, which, buf.data(), (int64_t)buf.size(), nullptr, nullptr) == SG_OK);
            }
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DACT1 + 6, nullptr, 0, dm, nullptr) == SG_OK && dm[3] == 32);   // conv8
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DPOOL1, nullptr, 0, dm, nullptr) == SG_OK && dm[2] == Fa / 2 && dm[3] == 64);
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_ACT1_UNPOOLED, nullptr, 0, dm, nullptr) == SG_OK && dm[2] == Fa && dm[3] == 64);
            EXPECT(sg_an_debug_gradient(ctx, 15, nullptr, 0, dm, nullptr) == SG_ERR_ARG && sg_an_debug_gradient(ctx, -1, nullptr, 0, dm, nullptr) == SG_ERR_ARG);
            EXPECT(sg_an_debug_gradient(nullptr, SG_AN_GRAD_DPRE, nullptr, 0, dm, nullptr) != SG_OK);
            EXPECT(hipdouble_launches() == l3);  // copies only
            // a fused gradient call, a forward-only call and a front-end call since: refused
            EXPECT(sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DPRE, dpre.data(), (int64_t)dpre.size(), dm, nullptr) == SG_ERR_STATE);
            setenv("SG_AN_FUSED", "0", 1);
            EXPECT(sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DPRE, nullptr, 0, dm, nullptr) == SG_OK);
            EXPECT(sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), nullptr, nullptr) == SG_OK);
            EXPECT(sg_an_debug_gradient(ctx, SG_AN_GRAD_DPRE, nullptr, 0, dm, nullptr) == SG_ERR_STATE);
            unsetenv("SG_AN_FUSED");
        }
        EXPECT(sg_an_logmel_backward(ctx, x.data(), B, T, fe.data(), grad.data(), 1, nullptr) == SG_OK);
        pp = sg_pgd_params{};
        pp.step_size = 4e-4f; pp.max_iter = 2; pp.grad_sign = 1; pp.eot_size = 2; pp.eot_batch_size = 1;
        EXPECT(sg_trace_begin(ctx, 512) == SG_OK);
        EXPECT(sg_an_pgd_run(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, succ.data(), dec.data(), sc.data(), loss.data(),
                             ltr.data(), dtr.data(), nullptr) == SG_OK);
        EXPECT(sg_trace_end(ctx, tg.data(), tm.data(), 512, &n_rec) == SG_OK && n_rec > 10);
        bool an_tags = false;
        for (int i = 0; i < n_rec; ++i) an_tags |= tg[i] >= SG_STAGE_AN_LOGMEL_FWD;
        EXPECT(an_tags);
        fp = sg_feco_params{};
        fp.k = Fa / 2; fp.max_iter = 3; fp.random_init = 1; fp.seed = 5; fp.index_base = 2;
        EXPECT(sg_an_pgd_run_feco(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, &fp, succ.data(), dec.data(), sc.data(),
                                  loss.data(), ltr.data(), dtr.data(), nullptr) == SG_OK);
        EXPECT(sg_an_pgd_run_feco(ctx, x.data(), y.data(), lower.data(), upper.data(), 1, T, &pp, &fp, succ.data(), dec.data(), sc.data(),
                                  loss.data(), nullptr, nullptr, nullptr) == SG_ERR_ARG);  // one utterance: host path
        fp.k = Fa + 1;
        EXPECT(sg_an_pgd_run_feco(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, &fp, succ.data(), dec.data(), sc.data(),
                                  loss.data(), nullptr, nullptr, nullptr) == SG_ERR_ARG);
        fp.k = 4;  // too few clusters for the conv stack
        EXPECT(sg_an_pgd_run_feco(ctx, x.data(), y.data(), lower.data(), upper.data(), B, T, &pp, &fp, succ.data(), dec.data(), sc.data(),
                                  loss.data(), nullptr, nullptr, nullptr) == SG_ERR_ARG);
        {   // round 5: a SECOND context in the same process (per-context / per-device launcher state), and every
            // front-end setting of sg_an_configure through the device loops (odd step counts end on the ping-pong twin)
            sg_ctx* ctx2 = nullptr;
            EXPECT(sg_create(0, &ctx2) == SG_OK && ctx2 != nullptr && ctx2 != ctx);
            EXPECT(sg_an_configure(nullptr, 32, 0, 0) == SG_ERR_ARG);
            EXPECT(sg_an_configure(ctx2, 16, 0, 0) == SG_ERR_ARG);
            EXPECT(sg_an_load(ctx2, &an.desc) == SG_OK);
            sg_pgd_params p3 = pp;
            sg_feco_params f2{};
            f2.k = Fa / 2; f2.max_iter = 3; f2.random_init = 1; f2.seed = 5;
            for (int cfg = 0; cfg < 8; ++cfg) {
                EXPECT(sg_an_configure(ctx2, (cfg & 1) ? 64 : 32, (cfg >> 1) & 1, (cfg >> 2) & 1) == SG_OK);
                p3.max_iter = 1 + (cfg & 1) + ((cfg >> 2) & 1);
                EXPECT(sg_an_pgd_run(ctx2, x.data(), y.data(), lower.data(), upper.data(), B, T, &p3, succ.data(), dec.data(), sc.data(),
                                     loss.data(), nullptr, nullptr, nullptr) == SG_OK);
                EXPECT(sg_an_loss_grad(ctx2, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
                EXPECT(sg_an_logmel(ctx2, x.data(), B, T, fe.data(), nullptr) == SG_OK);
                EXPECT(sg_an_logmel_backward(ctx2, x.data(), B, T, fe.data(), grad.data(), 1, nullptr) == SG_OK);
                EXPECT(sg_an_logmel_backward(ctx2, x.data(), B, T, fe.data(), grad.data(), 0, nullptr) == SG_OK);
                EXPECT(sg_an_pgd_run_feco(ctx2, x.data(), y.data(), lower.data(), upper.data(), B, T, &p3, &f2, succ.data(), dec.data(),
                                          sc.data(), loss.data(), nullptr, nullptr, nullptr) == SG_OK);
            }
            // the first context is untouched by all that
            EXPECT(sg_an_loss_grad(ctx, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
            EXPECT(sg_set_streamk(nullptr, 0) == SG_ERR_ARG && sg_set_streamk(ctx2, 0) == SG_OK && sg_set_streamk(ctx2, 1) == SG_OK);
            EXPECT(sg_debug_lose_handoffs(ctx2, -1) == SG_ERR_ARG && sg_debug_lose_handoffs(ctx2, 0) == SG_OK);
            // round 6: the x-vector front-end's transform precision, the k-means launch counter's test hook, the automatic
            // spectrum cache (-1)
            EXPECT(sg_xv_configure(nullptr, 32) == SG_ERR_ARG && sg_xv_configure(ctx2, 48) == SG_ERR_ARG);
            EXPECT(sg_xv_configure(ctx2, 64) == SG_OK && sg_xv_configure(ctx2, 32) == SG_OK);
            EXPECT(sg_debug_feco_epoch(nullptr, 1) == SG_ERR_ARG && sg_debug_feco_epoch(ctx2, 0x7FFEu) == SG_OK);
            EXPECT(sg_an_configure(ctx2, 32, -1, -1) == SG_OK);
            EXPECT(sg_an_loss_grad(ctx2, x.data(), y.data(), B, T, 0, &ce, dec.data(), sc.data(), loss.data(), grad.data(), nullptr) == SG_OK);
            EXPECT(sg_sync(ctx2, nullptr) == SG_OK);
            sg_destroy(ctx2);
        }
        int32_t rows = 0, ch = 0;
        EXPECT(sg_an_debug_activation(ctx, 8, nullptr, 0, &rows, &ch, nullptr) == SG_OK && ch == 32);
        EXPECT(sg_an_debug_activation(ctx, 0, nullptr, 0, &rows, &ch, nullptr) != SG_OK);
    }

    // ---- FeCo, post-processing ------------------------------------------------------------------------------
    {
        const int Bf = 2, Ff = 50, Df = 32, k = 20;
        std::vector<float> fe = rnd((size_t)Bf * Ff * Df, 500, 1.f), out((size_t)2 * Bf * k * Df), dfe((size_t)Bf * Ff * Df);
        std::vector<int32_t> ids((size_t)2 * Bf * Ff), cnt((size_t)2 * Bf * k);
        EXPECT(sg_feco_kmeans(ctx, fe.data(), Bf, Ff, Df, k, 5, ids.data(), nullptr) == SG_OK);
        EXPECT(sg_feco_kmeans(ctx, fe.data(), Bf, Ff, 65, k, 5, ids.data(), nullptr) != SG_OK);   // D <= 64
        EXPECT(sg_feco_kmeans(ctx, fe.data(), Bf, Ff, Df, Ff + 1, 5, ids.data(), nullptr) != SG_OK);
        EXPECT(sg_feco_kmeans_seeded(ctx, fe.data(), Bf, Ff, Df, k, 5, 3, 1, ids.data(), nullptr) == SG_OK);
        EXPECT(sg_feco_compress(ctx, fe.data(), ids.data(), Bf, Ff, Df, k, out.data(), cnt.data(), nullptr) == SG_OK);
        EXPECT(sg_feco_kmeans_compress(ctx, fe.data(), Bf, Ff, Df, k, 5, 1, 3, 0, 2, ids.data(), out.data(), cnt.data(), nullptr) == SG_OK);
        EXPECT(sg_feco_kmeans_compress(ctx, fe.data(), Bf, Ff, Df, k, 5, 0, 3, 0, 2, ids.data(), out.data(), cnt.data(), nullptr) != SG_OK);  // reps need the seeded form
        EXPECT(sg_feco_compress_backward_reps(ctx, out.data(), ids.data(), cnt.data(), Bf, Ff, Df, k, 1, 2, dfe.data(), nullptr) == SG_OK);
        EXPECT(sg_feco_compress_backward(ctx, out.data(), ids.data(), cnt.data(), Bf, Ff, Df, k, 1, dfe.data(), nullptr) == SG_OK);
        std::vector<int16_t> pcm((size_t)B * T);
        std::vector<double> met((size_t)B * 5), out3(3);
        EXPECT(sg_wav_finalize(ctx, x.data(), lower.data(), B, T, pcm.data(), met.data(), nullptr) == SG_OK);
        EXPECT(sg_wav_finalize(ctx, nullptr, lower.data(), B, T, pcm.data(), met.data(), nullptr) != SG_OK);  // metrics need the benign audio
        EXPECT(sg_wav_finalize(ctx, nullptr, lower.data(), B, T, pcm.data(), nullptr, nullptr) == SG_OK);
        EXPECT(sg_eer_threshold(ctx, scores.data(), 6, scores.data() + 6, 6, out3.data(), nullptr) == SG_OK);
        EXPECT(sg_eer_threshold(ctx, scores.data(), 0, scores.data(), 6, out3.data(), nullptr) != SG_OK);
    }
    EXPECT(sg_sync(ctx, nullptr) == SG_OK);
    sg_destroy(ctx);
    EXPECT(hipdouble_live_allocs() == 0);  // everything the context allocated through the runtime was released

    // ---- the enrol path shared with the i-vector model, from a model loaded with one speaker (CMVN features in: 40 frames)
    {
        XvModel one(D, 1);
        sg_ctx* c1 = nullptr;
        EXPECT(sg_create(0, &c1) == SG_OK && c1 && sg_xv_load(c1, &one.desc) == SG_OK);
        if (c1) {
            hipdouble_set_launch_hook(record_launch);
            g_on_launch = see_tail;
            std::vector<float> cm = rnd((size_t)2 * 40 * 30, 210), sc3((size_t)2 * 3);
            walk_enrol_path(c1, sg_xv_set_enroll, sg_xv_enroll_override, [&] {
                return sg_xv_forward(c1, cm.data(), 2, 40, SG_FLAG_CMVN, nullptr, dec.data(), sc3.data(), nullptr, nullptr, nullptr);
            }, D, one.enroll.data(), one.ppsi.data());
            sg_destroy(c1);
        }
        EXPECT(hipdouble_live_allocs() == 0);
    }
    if (g_fail) {
        std::fprintf(stderr, "%d expectation(s) failed\n", g_fail);
        return 1;
    }
    std::printf("abi_asan_driver: ok (%ld kernel launches issued against the host double)\n", hipdouble_launches());
    return 0;
}
