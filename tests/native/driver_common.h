// What the drivers of the sanitizer build of the C-ABI's host half share (`make asan`; see hip_host_double.cpp): the double's
// own entry points, EXPECT, the launch recorder, and the synthetic models and stages.  Every driver stays a stand-alone
// program with its own main and its own walk; this header is test infrastructure, never part of the product.
#pragma once
#include <cxxabi.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "speakerguard_hip.h"

extern "C" long hipdouble_launches();
extern "C" long hipdouble_live_allocs();
extern "C" void hipdouble_set_launch_hook(void (*)(const char*, dim3, dim3, size_t, void**));

static int g_fail = 0;
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_fail;                                                                \
        }                                                                            \
    } while (0)

// ---- the launch recorder: hipdouble_set_launch_hook(record_launch).  A launch goes to the driver's own hook (g_on_launch,
// which also sees the kernel arguments while they live) or, without one, is kept in g_seen.
struct Launch {
    std::string name;  // demangled, in full
    dim3 grid, block;
    size_t lds = 0;
    bool same_shape(const Launch& o) const {
        return grid.x == o.grid.x && grid.y == o.grid.y && grid.z == o.grid.z && block.x == o.block.x && lds == o.lds;
    }
};
static std::vector<Launch> g_seen;
static void (*g_on_launch)(const Launch&, void** args) = nullptr;
static void record_launch(const char* mangled, dim3 grid, dim3 block, size_t shmem, void** args) {
    int status = 0;
    char* dm = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
    Launch l;
    l.name = dm ? dm : mangled;
    std::free(dm);
    l.grid = grid; l.block = block; l.lds = shmem;
    if (g_on_launch) g_on_launch(l, args);
    else g_seen.push_back(l);
}

// "void sg::(anonymous namespace)::k<1, (sg::E)2>(args)" -> "k<1,(E)2>"
static std::string kernel_name(std::string name) {
    for (const char* drop : {"(anonymous namespace)::", "sg::", "void "})
        for (size_t at; (at = name.find(drop)) != std::string::npos;) name.erase(at, std::strlen(drop));
    int depth = 0;
    for (size_t i = 0; i < name.size(); ++i) {  // the parameter list opens at template depth 0
        depth += name[i] == '<' ? 1 : name[i] == '>' ? -1 : 0;
        if (name[i] == '(' && depth == 0) { name.resize(i); break; }
    }
    name.erase(std::remove(name.begin(), name.end(), ' '), name.end());
    return name;
}
// one line of a launch sequence (the .expected files), without its end: "<label> #<n> | <kernel> grid=.. block=.. lds=.."
static void print_launch(const std::string& label, int n, const Launch& l) {
    std::printf("%s #%d | %s grid=%u,%u,%u block=%u lds=%zu", label.c_str(), n, kernel_name(l.name).c_str(), l.grid.x, l.grid.y, l.grid.z,
                l.block.x * l.block.y * l.block.z, l.lds);
}

// ---- synthetic inputs, models and stages
static std::vector<float> rnd(size_t n, unsigned seed, float scale = 0.1f, float shift = 0.f) {
    std::vector<float> v(n);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        v[i] = shift + scale * ((float)(s >> 8) / 8388608.0f - 1.0f);
    }
    return v;
}

struct XvModel {
    std::vector<float> w[5], b[5], mean[5], var[5], fc1w, fc1b, emean, lda, pmean, ptrans, ppsi, enroll;
    sg_xv_weights desc{};
    XvModel(int D, int S) {
        const int cin[5] = {30, 512, 512, 512, 512}, cout[5] = {512, 512, 512, 512, 1500}, k[5] = {5, 5, 7, 1, 1};
        for (int l = 0; l < 5; ++l) {
            w[l] = rnd((size_t)cout[l] * cin[l] * k[l], 10 + l);
            b[l] = rnd(cout[l], 20 + l);
            mean[l] = rnd(cout[l], 30 + l);
            var[l] = rnd(cout[l], 40 + l, 0.5f, 1.0f);
            desc.tdnn_weight[l] = w[l].data(); desc.tdnn_bias[l] = b[l].data();
            desc.bn_mean[l] = mean[l].data(); desc.bn_var[l] = var[l].data();
        }
        fc1w = rnd((size_t)512 * 3000, 1); fc1b = rnd(512, 2); emean = rnd(512, 3); lda = rnd((size_t)D * 513, 4);
        pmean = rnd(D, 5); ptrans = rnd((size_t)D * D, 6); ppsi = rnd(D, 7, 0.5f, 1.0f); enroll = rnd((size_t)S * D, 8);
        desc.fc1_weight = fc1w.data(); desc.fc1_bias = fc1b.data(); desc.emb_mean = emean.data(); desc.lda = lda.data();
        desc.plda_mean = pmean.data(); desc.plda_transform = ptrans.data(); desc.plda_psi = ppsi.data(); desc.enroll = enroll.data();
        desc.D = D; desc.S = S; desc.bn_eps = 1e-5f; desc.threshold = -INFINITY;
    }
};

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

// ---- the enrol path both speaker models share (csrc/plda_backend.hip), walked through one model's public entries.  What a tail
// kernel was handed is read off its first argument, the model block it takes by value: mirrors of TailModelDev (k_tail.hip)
// and IvTailDev (k_ivector.hip), the enrolled table being the last pointer of each.
struct XvTailBlock { const float* p[10]; int D, S, Dp; float threshold, logdet_given, logdet_without; };
struct IvTailBlock { const float* p[6]; int R, D, S; float threshold, logdet_given, logdet_without; };
struct TailSeen { const float* enroll = nullptr; int S = 0; float threshold = 0.f, logdet_given = 0.f, logdet_without = 0.f; long launches = 0; };
static TailSeen g_tail;
static void see_tail(const Launch& l, void** args) {
    const std::string k = kernel_name(l.name);
    if (k == "tail_kernel") {
        const XvTailBlock& m = *static_cast<const XvTailBlock*>(args[0]);
        g_tail.enroll = m.p[8]; g_tail.S = m.S; g_tail.threshold = m.threshold;
        g_tail.logdet_given = m.logdet_given; g_tail.logdet_without = m.logdet_without; ++g_tail.launches;
    } else if (k == "iv_tail_kernel") {
        const IvTailBlock& m = *static_cast<const IvTailBlock*>(args[0]);
        g_tail.enroll = m.p[5]; g_tail.S = m.S; g_tail.threshold = m.threshold;
        g_tail.logdet_given = m.logdet_given; g_tail.logdet_without = m.logdet_without; ++g_tail.launches;
    }
}
// On a context whose model was just loaded with ONE enrolled speaker (table enroll1, D columns, psi as loaded): `forward` runs one
// small pass that writes n_scores scores per row for as many speakers as are active (room for 3).  The launch hook must reach see_tail.
template <typename SetEnroll, typename Override, typename Forward>
static void walk_enrol_path(sg_ctx* ctx, SetEnroll set_enroll, Override enroll_override, Forward forward, int D, const float* enroll1,
                            const float* psi) {
    const auto same_rows = [&](const float* table, int S) { return g_tail.enroll && !std::memcmp(g_tail.enroll, table, (size_t)S * D * 4); };
    double ldg = 0.0, ldw = 0.0;
    for (int d = 0; d < D; ++d) {
        ldg += std::log(1.0 + (double)psi[d] / ((double)psi[d] + 1.0));
        ldw += std::log((double)psi[d] + 1.0);
    }
    const float want_g = (float)ldg, want_w = (float)ldw;
    const auto pass = [&](const float* table, int S, float thr) {
        const long before = g_tail.launches;
        EXPECT(forward() == SG_OK && g_tail.launches == before + 1);
        EXPECT(g_tail.S == S && same_rows(table, S) && g_tail.threshold == thr);
        EXPECT(!std::memcmp(&g_tail.logdet_given, &want_g, 4) && !std::memcmp(&g_tail.logdet_without, &want_w, 4));
    };
    const std::vector<float> three = rnd((size_t)3 * D, 201), two = rnd((size_t)2 * D, 202), other = rnd((size_t)3 * D, 203);
    // 1. as loaded: one speaker
    pass(enroll1, 1, -INFINITY);
    const long live = hipdouble_live_allocs();
    // 2. three speakers: a new table, the old one released
    EXPECT(set_enroll(ctx, three.data(), 3, 0.5f) == SG_OK && hipdouble_live_allocs() == live);
    pass(three.data(), 3, 0.5f);
    const float* own = g_tail.enroll;
    // 3. two speakers: the same buffer
    EXPECT(set_enroll(ctx, two.data(), 2, 0.25f) == SG_OK && hipdouble_live_allocs() == live);
    pass(two.data(), 2, 0.25f);
    EXPECT(g_tail.enroll == own);
    // 4. the threshold alone
    EXPECT(set_enroll(ctx, nullptr, 2, 1.5f) == SG_OK && hipdouble_live_allocs() == live);
    pass(two.data(), 2, 1.5f);
    EXPECT(g_tail.enroll == own);
    // 5. refused counts: the text, and nothing changed
    for (int bad : {0, 1025}) {
        EXPECT(set_enroll(ctx, three.data(), bad, 9.f) == SG_ERR_ARG && std::string(sg_last_error(ctx)) == "S must be 1..1024");
        EXPECT(enroll_override(ctx, three.data(), bad) == SG_ERR_ARG && std::string(sg_last_error(ctx)) == "S must be 1..1024");
    }
    pass(two.data(), 2, 1.5f);
    // 6. a per-call override: the caller's table as it is, then the model's own again
    EXPECT(enroll_override(ctx, other.data(), 3) == SG_OK && hipdouble_live_allocs() == live);
    pass(other.data(), 3, 1.5f);
    EXPECT(g_tail.enroll == other.data());
    EXPECT(enroll_override(ctx, nullptr, 0) == SG_OK);
    pass(two.data(), 2, 1.5f);
    EXPECT(g_tail.enroll == own && hipdouble_live_allocs() == live);
}

// a time-domain stage of a defended loop's chain
static sg_wav_stage td(int kind, float param, uint64_t seed = 0) {
    sg_wav_stage st{};
    st.tag = SG_WAV_STAGE_DEFENSE;
    st.u.defense.kind = kind;
    st.u.defense.param = param;
    st.u.defense.seed = seed;
    return st;
}
// ... and a filter stage: two second-order sections, clipped to the 16-bit range
static sg_wav_stage lpf_stage() {
    static const double sos[2][6] = {{0.2, 0.4, 0.2, 1.0, -0.3, 0.1}, {1.0, 2.0, 1.0, 1.0, -0.2, 0.3}};
    sg_wav_stage st{};
    st.tag = SG_WAV_STAGE_FILTER;
    st.u.filter.n_sections = 2; st.u.filter.sos = &sos[0][0]; st.u.filter.clip_mode = SG_FD_CLIP_RANGE; st.u.filter.bits = 16;
    return st;
}
