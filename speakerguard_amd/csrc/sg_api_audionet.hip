// C-ABI entry points of the AudioNet CSI-NE path (include/speakerguard_hip.h, "sg_an_*"):
// model load (BatchNorm folding), workspace, forward / backward / PGD kernel sequences.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "sg_internal.h"

using namespace sg;

namespace {

// ---- front-end tables: periodic hann(800), librosa-0.8.0 slaney mel basis (Preprocessor.py:57-60) ----
double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_hz / f_sp + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

int an_build_tables(sg_ctx* ctx) {
    if (ctx->an_tables_ready) return SG_OK;
    const double PI = 3.14159265358979323846;
    std::vector<float> window(kAnWin), melw((size_t)kAnMel * kAnBins, 0.f), w0(kAnBins, 0.f), w1(kAnBins, 0.f);
    std::vector<int> lo(kAnMel), hi(kAnMel), m0(kAnBins, -1);
    std::vector<double2> tw(kAnFft / 2);
    std::vector<uint16_t> br(kAnFft);
    {   // torch.hann_window(800) (periodic): arange * (2 pi / 800) -> cos -> * -0.5 + 0.5, float32
        const float step = (float)(PI * 2.0 / (double)kAnWin);
        for (int n = 0; n < kAnWin; ++n) window[n] = cosf((float)n * step) * -0.5f + 0.5f;
    }
    {   // librosa.filters.mel(16000, 1024, 32, fmin=0, fmax=8000): float64 arithmetic, cast to float32
        std::vector<double> mel_f(kAnMel + 2);
        const double mmin = hz_to_mel(0.0), mmax = hz_to_mel(8000.0);
        for (int i = 0; i < kAnMel + 2; ++i) mel_f[i] = mel_to_hz(mmin + (mmax - mmin) * i / (kAnMel + 1));
        for (int m = 0; m < kAnMel; ++m) {
            const double enorm = 2.0 / (mel_f[m + 2] - mel_f[m]);
            lo[m] = kAnBins;
            hi[m] = 0;
            for (int k = 0; k < kAnBins; ++k) {
                const double fr = 8000.0 * k / (kAnBins - 1);
                const double lower = (fr - mel_f[m]) / (mel_f[m + 1] - mel_f[m]);
                const double upper = (mel_f[m + 2] - fr) / (mel_f[m + 2] - mel_f[m + 1]);
                const double w = std::fmax(0.0, std::fmin(lower, upper)) * enorm;
                melw[(size_t)m * kAnBins + k] = (float)w;
                if (w > 0.0) {
                    if (k < lo[m]) lo[m] = k;
                    hi[m] = k + 1;
                }
            }
            if (lo[m] > hi[m]) lo[m] = hi[m] = 0;
        }
        for (int k = 0; k < kAnBins; ++k) {
            int first = -1, cnt = 0;
            for (int m = 0; m < kAnMel; ++m)
                if (melw[(size_t)m * kAnBins + k] > 0.f) {
                    if (first < 0) first = m;
                    ++cnt;
                }
            if (cnt > 2 || (cnt == 2 && melw[(size_t)(first + 1) * kAnBins + k] <= 0.f))
                return fail(ctx, SG_ERR_STATE, "mel filterbank is not a two-overlap triangular bank");
            m0[k] = first;
            if (first >= 0) {
                w0[k] = melw[(size_t)first * kAnBins + k];
                w1[k] = first + 1 < kAnMel ? melw[(size_t)(first + 1) * kAnBins + k] : 0.f;
            }
        }
    }
    for (int k = 0; k < kAnFft / 2; ++k) tw[k] = make_double2(std::cos(2.0 * PI * k / kAnFft), -std::sin(2.0 * PI * k / kAnFft));
    for (int i = 0; i < kAnFft; ++i) {
        int r = 0;
        for (int bit = 0; bit < 10; ++bit)
            if (i & (1 << bit)) r |= 1 << (9 - bit);
        br[i] = (uint16_t)r;
    }
    AnTables& t = ctx->an_tab;
    std::vector<void*>& pool = ctx->model_allocs;
    int rc = 0;
    rc |= dev_upload(ctx, pool, &t.window, window);
    rc |= dev_upload(ctx, pool, &t.mel_w, melw);
    rc |= dev_upload(ctx, pool, &t.mel_lo, lo);
    rc |= dev_upload(ctx, pool, &t.mel_hi, hi);
    {   // the per-lane views of window and filterbank the front-end kernels keep in LDS (k_audionet.hip, AnLaneTab)
        // mel: every filter is cut into ceil(width / 20) runs of consecutive bins of (nearly) equal length, one lane per run
        // (971 filter taps over 63 lanes, <= 20 each; the two-lanes-per-filter split of rounds 3-4 was bound by its widest
        // half, 44 taps, 64 % of them zero padding).  mel_seg[m] = first lane | runs << 8: lane m adds the runs' sums up in
        // ascending order.
        constexpr int kLaneBins = 20;  // = kAnMelLaneBins
        std::vector<float> lwin(16 * 64), lmelw((size_t)kLaneBins * 64, 0.f);
        std::vector<int> lk0(64, 0), seg(kAnMel, 0);
        for (int tap = 0; tap < 16; ++tap)
            for (int l = 0; l < 64; ++l) {
                const int n = 2 * (l + 64 * (tap >> 1)) + (tap & 1) - (kAnFft - kAnWin) / 2;
                lwin[tap * 64 + l] = (n >= 0 && n < kAnWin) ? window[n] : 0.f;
            }
        int lanes = 0;
        for (int m = 0; m < kAnMel; ++m) {
            const int w = hi[m] - lo[m], runs = w > 0 ? (w + kLaneBins - 1) / kLaneBins : 1;
            if (lanes + runs > 64 || runs > 5) return fail(ctx, SG_ERR_STATE, "mel filterbank needs more than 64 runs of %d bins", kLaneBins);
            seg[m] = lanes | (runs << 8);
            for (int i = 0; i < runs; ++i, ++lanes) {
                const int k0 = lo[m] + (int)((long long)w * i / runs), k1 = lo[m] + (int)((long long)w * (i + 1) / runs);
                lk0[lanes] = k0;
                for (int j = 0; j < k1 - k0; ++j) lmelw[(size_t)j * 64 + lanes] = melw[(size_t)m * kAnBins + k0 + j];
            }
        }
        rc |= dev_upload(ctx, pool, &t.mel_seg, seg);
        rc |= dev_upload(ctx, pool, &t.lane_win, lwin);
        rc |= dev_upload(ctx, pool, &t.lane_melw, lmelw);
        rc |= dev_upload(ctx, pool, &t.lane_k0, lk0);
    }
    {   // twiddle tables of the 512-point complex transform (W512^m = W1024^(2 m)), float64 and the same rounded once to float32
        auto w512 = [&](int m) {
            const double2 w = tw[(2 * (m & 255)) % (kAnFft / 2)];
            return (m & 256) ? make_double2(-w.x, -w.y) : w;
        };
        std::vector<double2> t1(kFftTw1), t2(kFftTw2);
        std::vector<float2> t1f(kFftTw1), t2f(kFftTw2);
        fft512_twiddle_tables(w512, reinterpret_cast<double*>(t1.data()), reinterpret_cast<double*>(t2.data()));
        fft512_twiddle_tables(w512, reinterpret_cast<float*>(t1f.data()), reinterpret_cast<float*>(t2f.data()));
        rc |= dev_upload(ctx, pool, &t.tw1d, t1);
        rc |= dev_upload(ctx, pool, &t.tw2d, t2);
        rc |= dev_upload(ctx, pool, &t.tw1f, t1f);
        rc |= dev_upload(ctx, pool, &t.tw2f, t2f);
    }
    rc |= dev_upload(ctx, pool, &t.bin_m0, m0);
    rc |= dev_upload(ctx, pool, &t.bin_w0, w0);
    rc |= dev_upload(ctx, pool, &t.bin_w1, w1);
    rc |= dev_upload(ctx, pool, &t.twiddle, tw);
    rc |= dev_upload(ctx, pool, &t.bitrev, br);
    if (!ctx->range_scratch) rc |= dev_alloc(ctx, pool, &ctx->range_scratch, 512);
    if (rc) return SG_ERR_HIP;
    ctx->an_tables_ready = true;
    return SG_OK;
}

int an_ensure_workspace(sg_ctx* ctx, int B, int T, int F) {
    AnWorkspace& w = ctx->an_ws;
    if (B <= w.B && F <= w.F && T <= w.T && w.scale) return SG_OK;
    (void)hipDeviceSynchronize();
    for (void* p : w.allocs) (void)hipFree(p);
    const int cb = B > w.B ? B : w.B, cf = F > w.F ? F : w.F, ct = T > w.T ? T : w.T;
    w = AnWorkspace();
    w.B = cb; w.F = cf; w.T = ct;
    int Tin[kAnConv], Tout[kAnConv];
    an_layer_frames(cf, Tin, Tout);
    const size_t b = (size_t)cb;
    int rc = 0;
    rc |= dev_alloc(ctx, w.allocs, &w.scale, 4);
    rc |= dev_alloc(ctx, w.allocs, &w.feats, b * cf * kAnMel);
    rc |= dev_alloc(ctx, w.allocs, &w.pre, b * cf * kAnMel);
    rc |= dev_alloc(ctx, w.allocs, &w.dpre, b * cf * kAnMel);
    rc |= dev_alloc(ctx, w.allocs, &w.dfeats, b * cf * kAnMel);
    rc |= dev_alloc(ctx, w.allocs, &w.dframes, b * cf * kAnWin);
    rc |= dev_alloc(ctx, w.allocs, &w.mel_cache, b * cf * kAnMel);
    rc |= dev_alloc(ctx, w.allocs, &w.feco_ids, b * cf);
    rc |= dev_alloc(ctx, w.allocs, &w.feco_cnt, b * cf);
    rc |= dev_alloc(ctx, w.allocs, &w.feco_out, b * cf * kAnMel);
    rc |= dev_alloc(ctx, w.allocs, &w.dfeco, b * cf * kAnMel);
    rc |= dev_alloc(ctx, w.allocs, &w.y_rep, b);
    rc |= dev_alloc(ctx, w.allocs, &w.trace_l, b);
    rc |= dev_alloc(ctx, w.allocs, &w.trace_d, b);
    for (int l = 0; l < kAnConv; ++l) {
        const size_t n = b * (size_t)(Tout[l] > 0 ? Tout[l] : 1) * kAnCout[l];
        rc |= dev_alloc(ctx, w.allocs, &w.act[l], n);
        rc |= dev_alloc(ctx, w.allocs, &w.dact[l], n);
        if (kAnPool[l]) {
            rc |= dev_alloc(ctx, w.allocs, &w.pool[l], n / 2 + kAnCout[l]);
            rc |= dev_alloc(ctx, w.allocs, &w.dpool[l], n / 2 + kAnCout[l]);
        }
    }
    if (rc) {
        for (void* p : w.allocs) (void)hipFree(p);
        w = AnWorkspace();
        return SG_ERR_HIP;
    }
    return SG_OK;
}

struct AnDims {
    int B, T, F;
    bool keep_scale = false;
};

int an_check(sg_ctx* ctx, int B, int TF, int flag, AnDims* d) {
    if (!ctx) return SG_ERR_ARG;
    ctx->an_ws.grad_B = 0;  // a pass starts: the buffers of the last gradient call are no longer its own
    if (!ctx->an.loaded) return fail(ctx, SG_ERR_STATE, "no AudioNet model loaded (call sg_an_load)");
    SG_HIP(hipSetDevice(ctx->device));
    if (B < 1) return fail(ctx, SG_ERR_ARG, "B must be >= 1");
    if (flag != 0 && flag != 1) return fail(ctx, SG_ERR_ARG, "flag must be 0 (wav) or 1 (log-mel feat)");
    d->B = B;
    if (flag == 0) {
        if (TF < kAnFft) return fail(ctx, SG_ERR_ARG, "waveform shorter than one 1024-sample STFT frame");
        d->T = TF;
        d->F = an_num_frames(TF);
    } else {
        d->T = 0;
        d->F = TF;
    }
    int Tin[kAnConv], Tout[kAnConv];
    if (!an_layer_frames(d->F, Tin, Tout))
        return fail(ctx, SG_ERR_ARG, "%d frames are too few for the AudioNet stack (need >= 3 frames at conv8)", d->F);
    // 32-bit buffer offsets in the contraction kernels (k_conv_gemm.hip): every activation tensor < 2 GiB
    for (int l = 0; l < kAnConv; ++l)
        if ((size_t)B * Tout[l] * kAnCout[l] * sizeof(float) >= 0x80000000ull || (size_t)B * d->F * 32 * sizeof(float) >= 0x80000000ull)
            return fail(ctx, SG_ERR_ARG, "batch of %d x %d frames exceeds the 2 GiB per-tensor limit of one pass: split the batch",
                           B, d->F);
    int rc = an_build_tables(ctx);
    if (rc) return rc;
    rc = an_ensure_workspace(ctx, d->B, d->T, d->F);
    if (rc) return fail(ctx, rc, "workspace allocation failed: %s", ctx->err.c_str());
    return SG_OK;
}

const float* an_layer_input(const AnWorkspace& w, int l) {
    if (l == 0) return w.pre;
    return kAnPool[l - 1] ? w.pool[l - 1] : w.act[l - 1];
}

// Does the forward keep the frames' spectra for the adjoint of the same pass?  sg_an_configure: 1 / 0, or -1 = by size
// (profiles/r06_an_frontend_ab.txt, PGD-20, float32 transforms): the cache wins at every size measured (2-6 % of a step)
// except between 24 000 and 40 000 frames (80 .. 133 utterances of 3 s: -1 .. -6 %), where the chip is just full of
// forward waves and the cache's write traffic costs the forward more than the second transform costs the adjoint.
static bool an_use_spec_cache(const sg_ctx* ctx, int B, int F) {
    if (ctx->an_cfg.spec_cache >= 0) return ctx->an_cfg.spec_cache != 0;
    const long frames = (long)B * F;
    return !(frames >= 24000 && frames < 40000);
}

// waveform -> log-mel features in ws.feats (the backward of the same pass starts from the stored mel energies)
int an_frontend_forward(sg_ctx* ctx, const float* x, const AnDims& d, hipStream_t s) {
    AnWorkspace& w = ctx->an_ws;
    if (!d.keep_scale) SG_HIP(launch_input_scale(x, (int64_t)d.B * d.T, ctx->range_scratch, w.scale, 1, s));
    AnTables tab = ctx->an_tab;
    tab.mel_cache = w.mel_cache;
    if (an_use_spec_cache(ctx, d.B, d.F)) {
        // the cache is an optional speed-up: sized for this call (grown when a larger one comes), and a refused allocation
        // leaves the pass on the backward's own transforms instead of failing it
        const size_t need = (size_t)d.B * d.F * (kAnFft / 2) * sizeof(float2);
        if (need > w.spec_cache_bytes && !w.spec_cache_refused) {
            void* p = nullptr;
            if (hipMalloc(&p, need) == hipSuccess) {
                if (w.spec_cache) {
                    SG_HIP(hipStreamSynchronize(s));  // (an earlier pass may still read the old buffer)
                    (void)hipFree(w.spec_cache);
                    w.allocs.erase(std::remove(w.allocs.begin(), w.allocs.end(), static_cast<void*>(w.spec_cache)), w.allocs.end());
                }
                w.allocs.push_back(p);
                w.spec_cache = static_cast<float2*>(p);
                w.spec_cache_bytes = need;
            } else {
                (void)hipGetLastError();
                w.spec_cache_refused = true;
                fprintf(stderr, "speakerguard: no room for the %zu MB spectrum cache of the log-mel front-end; the adjoint transforms again\n", need >> 20);
            }
        }
        if (need <= w.spec_cache_bytes) tab.spec_cache = w.spec_cache;
    }
    w.cache_x = x; w.cache_B = d.B; w.cache_T = d.T; w.cache_spec = tab.spec_cache != nullptr;
    SG_STAGE(SG_STAGE_AN_LOGMEL_FWD, launch_an_logmel_fwd(tab, x, d.B, d.T, d.F, w.scale, w.feats, ctx->an_cfg.fft32, s));
    return SG_OK;
}

// the launch-form knobs of this call (AnKnobs, sg_internal.h)
AnKnobs an_knobs() {
    AnKnobs k;
    const char* e;
    if ((e = sg_tune_env("SG_AN_FUSED"))) k.fused = atoi(e) != 0;
    if ((e = sg_tune_env("SG_AN_HEAD"))) k.head = atoi(e) != 0;
    if ((e = sg_tune_env("SG_AN_ONE"))) k.one = atoi(e) != 0;
    if ((e = sg_tune_env("SG_AN_SLICES"))) k.slices = atoi(e);
    return k;
}
// rows x Fnet frames through the network; Fnet is the frame count the network sees (the front-end's, or the number of FeCo
// clusters when the defense sits between front-end and network)
AnNetPlan an_plan(sg_ctx* ctx, const AnKnobs& k, int rows, int Fnet, bool want_grad) {
    return an_net_plan(k, rows, Fnet, ctx->num_cus, k.fused && an_fused_device_ok(), want_grad);
}

AnFusedArgs an_fused_args(sg_ctx* ctx, const AnNetPlan& p) {
    AnWorkspace& w = ctx->an_ws;
    const AnModel& m = ctx->an;
    AnFusedArgs a{};
    a.pre = w.pre;
    for (int l = 0; l < kAnConv; ++l) {
        a.act[l] = w.act[l];
        a.pool[l] = w.pool[l];
        a.bias[l] = m.bias[l];
        a.Tin[l] = p.Tin[l];
        a.Tout[l] = p.Tout[l];
    }
    a.w25 = m.w25;
    a.pre_bias = m.pre_bias;
    a.Fnet = p.Fnet;
    return a;
}

// what the head computes and where it writes, whichever launch runs it (an_tail, the fused backward, the one launch)
AnHeadArgs an_head_args(sg_ctx* ctx, const int64_t* y, const sg_loss_spec& ls, int coef_rows, float* emb, float* scores, int64_t* decisions,
                        float* loss, float* loss_trace, int64_t* dec_trace, uint8_t* success) {
    AnHeadArgs h{};
    h.on = 1;
    h.fc_w = ctx->an.fc_w;
    h.fc_b = ctx->an.fc_b;
    h.S = ctx->an.S;
    h.threshold = -INFINITY;
    h.y = y;
    h.ls = ls;
    h.coef_rows = coef_rows;
    h.emb_out = emb;
    h.scores_out = scores;
    h.dec_out = decisions;
    h.loss_out = loss;
    h.loss_trace = loss_trace;
    h.dec_trace = dec_trace;
    h.success = success;
    return h;
}

// features (rows, Fnet, 32) -> conv stack
int an_net_forward(sg_ctx* ctx, const AnNetPlan& p, const float* feats, int B, hipStream_t s) {
    AnWorkspace& w = ctx->an_ws;
    const AnModel& m = ctx->an;
    if (p.form != AN_PER_LAYER) {
        AnFusedArgs a = an_fused_args(ctx, p);
        a.feats = feats;
        for (int l = 0; l < kAnConv; ++l) a.wq[l] = m.wfq[l];
        SG_STAGE(SG_STAGE_AN_FUSED_FWD, launch_an_cnn_fused(a, p, B, false, s));
        return SG_OK;
    }
    SG_STAGE(SG_STAGE_AN_PREFILTER_FWD, launch_an_prefilter(feats, w.pre, B, p.Fnet, m.w25, m.pre_bias, 0, s));
    for (int l = 0; l < kAnConv; ++l) {
        ConvGemmArgs a{};
        a.A = an_layer_input(w, l);
        a.W = m.wf[l];
        a.C = w.act[l];
        a.bias = m.bias[l];
        a.Ta = p.Tin[l];
        a.Tc = p.Tout[l];
        a.M = B * a.Tc;
        a.N = kAnCout[l];
        a.Kc = kAnCin[l];
        a.lda = kAnCin[l];
        a.ldw = kAnCout[l];
        a.ldc = kAnCout[l];
        a.taps = 3;
        a.tap_step = 1;
        a.tap_base = -kAnPad[l];
        a.total_chunks = 3 * (a.Kc / 32);
        a.chunks_per_split = a.total_chunks;
        a.Wq = a.N % 128 == 0 ? m.wfq[l] : nullptr;
        SG_STAGE(SG_STAGE_AN_CONV_FWD + l, launch_conv_gemm(a, a.N % 128 == 0 ? 2 : 1, EPI_BIAS_RELU, 1, s));
        if (kAnPool[l]) SG_STAGE(SG_STAGE_AN_POOL_FWD, launch_an_pool_fwd(w.act[l], w.pool[l], B, p.Tout[l], kAnCout[l], s));
    }
    return SG_OK;
}

// d loss / d conv8 pre-activation (ws.dact[6], or the head inside the launch) -> d loss / d features (rows, Fnet, 32)
int an_net_backward(sg_ctx* ctx, const AnNetPlan& p, int B, const AnHeadArgs* head, float* dfeats_out, hipStream_t s) {
    AnWorkspace& w = ctx->an_ws;
    const AnModel& m = ctx->an;
    if (p.form != AN_PER_LAYER) {
        AnFusedArgs a = an_fused_args(ctx, p);
        a.dtop = w.dact[kAnConv - 1];
        a.dfeats = dfeats_out;
        if (head) a.head = *head;
        for (int l = 0; l < kAnConv; ++l) a.wq[l] = m.wbq[l];
        SG_STAGE(SG_STAGE_AN_FUSED_BWD, launch_an_cnn_fused(a, p, B, true, s));
        return SG_OK;
    }
    // (the plan puts the head into a launch only in a fused form: nobody would have written dact[6])
    if (head) return fail(ctx, SG_ERR_STATE, "AudioNet: the per-layer backward cannot run the head");
    for (int l = kAnConv - 1; l >= 0; --l) {
        // data gradient of conv l: reads dact[l] (B, Tout, Cout), writes the gradient of its input
        const bool in_pooled = l > 0 && kAnPool[l - 1];
        ConvGemmArgs a{};
        a.A = w.dact[l];
        a.W = m.wb[l];
        a.C = l == 0 ? w.dpre : (in_pooled ? w.dpool[l - 1] : w.dact[l - 1]);
        a.mask = (l == 0 || in_pooled) ? nullptr : w.act[l - 1];
        a.Ta = p.Tout[l];
        a.Tc = p.Tin[l];
        a.M = B * a.Tc;
        a.N = kAnCin[l];
        a.Kc = kAnCout[l];
        a.lda = kAnCout[l];
        a.ldw = kAnCin[l];
        a.ldc = kAnCin[l];
        a.taps = 3;
        a.tap_step = -1;
        a.tap_base = kAnPad[l];  // d in[t] = sum_j W_j^T d out[t + pad - j]
        a.total_chunks = 3 * (a.Kc / 32);
        a.chunks_per_split = a.total_chunks;
        a.Wq = a.N % 128 == 0 ? m.wbq[l] : nullptr;
        SG_STAGE(SG_STAGE_AN_CONV_BWD + l, launch_conv_gemm(a, a.N % 128 == 0 ? 2 : 1, a.mask ? EPI_RELU_MASK : EPI_NONE, 1, s));
        if (in_pooled)
            SG_STAGE(SG_STAGE_AN_POOL_BWD, launch_an_pool_bwd(w.act[l - 1], w.dpool[l - 1], w.dact[l - 1], B, p.Tout[l - 1], kAnCout[l - 1], s));
    }
    SG_STAGE(SG_STAGE_AN_PREFILTER_BWD, launch_an_prefilter(w.dpre, dfeats_out, B, p.Fnet, m.w25, 0.f, 1, s));
    return SG_OK;
}

// the per-row records of a step that ran R EOT repeats, reduced to per-utterance ones right after the head (null: none)
struct AnEotRecords {
    int R, B;
    float* loss_out;
    int64_t* dec_out;
};

// One pass through the network by the plan's form: forward, head, and -- where dfeats_out is given -- backward to
// d loss / d features.  Leaves the pass's frame counts in the workspace (sg_an_debug_activation).
int an_net_step(sg_ctx* ctx, const AnNetPlan& p, const float* feats, int rows, const AnHeadArgs& head, const AnEotRecords* eot,
                float* dfeats_out, hipStream_t s) {
    AnWorkspace& w = ctx->an_ws;
    const AnModel& m = ctx->an;
    const int L = kAnConv - 1;
    const bool head_inside = p.form == AN_FUSED_HEAD || p.form == AN_ONE_LAUNCH;
    if (head_inside && !dfeats_out) return fail(ctx, SG_ERR_STATE, "AudioNet: a plan with the head inside the backward needs a gradient target");
    std::copy(p.Tin, p.Tin + kAnConv, w.Tin);
    std::copy(p.Tout, p.Tout + kAnConv, w.Tout);
    int rc;
    if (p.form == AN_ONE_LAUNCH) {
        AnFusedArgs a = an_fused_args(ctx, p);
        a.feats = feats;
        a.dfeats = dfeats_out;
        a.head = head;
        for (int l = 0; l < kAnConv; ++l) {
            a.wq[l] = m.wfq[l];
            a.wq_bwd[l] = m.wbq[l];
        }
        SG_STAGE(SG_STAGE_AN_FUSED_FWDBWD, launch_an_cnn_fwdbwd(a, p, rows, s));
    } else {
        if ((rc = an_net_forward(ctx, p, feats, rows, s))) return rc;
        if (head_inside) {
            if ((rc = an_net_backward(ctx, p, rows, &head, dfeats_out, s))) return rc;
        } else {
            SG_STAGE(SG_STAGE_AN_TAIL, launch_an_tail(w.act[L], rows, p.Tout[L], head.fc_w, head.fc_b, head.S, head.threshold, head.y, head.ls,
                                                      dfeats_out != nullptr, head.emb_out, head.scores_out, head.dec_out, head.loss_out, w.dact[L],
                                                      head.loss_trace, head.dec_trace, head.success, s, head.coef_rows));
        }
    }
    if (eot) SG_HIP(launch_eot_trace_reduce(head.loss_trace, head.dec_trace, eot->R, eot->B, eot->loss_out, eot->dec_out, s));
    if (dfeats_out && !head_inside) return an_net_backward(ctx, p, rows, nullptr, dfeats_out, s);
    return SG_OK;
}

// the overlap-add inside the adjoint, or the separate pair?  (AnFrontCfg::ola: 1 / 0, or -1 = whichever the batch favours:
// the fused form cuts utterances into runs with 5 halo frames each, k_audionet.hip an_ola_pays)
static bool an_use_ola(const sg_ctx* ctx, int B, int F) {
    return ctx->an_cfg.ola > 0 || (ctx->an_cfg.ola < 0 && an_ola_pays(B, F, ctx->an_cfg.fft32, ctx->num_cus));
}

// d loss / d log-mel (B, F, 32) -> d loss / d waveform: written to grad_out and / or applied as the fused PGD update
// x_update: the iterate to step from (== x); x_next: where the stepped iterate goes.  The fused overlap-add needs
// x_next != x_update (neighbour blocks still read x around their cut); the separate pair updates in place and copies if
// the caller asked for another buffer.
int an_frontend_backward(sg_ctx* ctx, const float* x, const AnDims& d, const float* dfeats, float* grad_out, float* x_update, float* x_next,
                         const float* lower, const float* upper, float step, int grad_sign, hipStream_t s) {
    AnWorkspace& w = ctx->an_ws;
    AnTables tab = ctx->an_tab;
    tab.mel_cache = w.mel_cache;
    tab.spec_cache = w.cache_spec ? w.spec_cache : nullptr;
    if (an_use_ola(ctx, d.B, d.F) && (!x_update || x_next != x_update)) {
        AnOlaArgs a{};
        a.x = x; a.dfeats = dfeats; a.dframes = w.dframes; a.grad_out = grad_out;
        a.x_in = x_update; a.x_out = x_update ? x_next : nullptr; a.lower = lower; a.upper = upper; a.scale_p = w.scale;
        a.step = step; a.grad_sign = grad_sign; a.B = d.B; a.T = d.T; a.F = d.F;
        SG_STAGE(SG_STAGE_AN_LOGMEL_BWD, launch_an_logmel_bwd_ola(tab, a, ctx->an_cfg.fft32, ctx->num_cus, s));
        return SG_OK;
    }
    SG_STAGE(SG_STAGE_AN_LOGMEL_BWD, launch_an_logmel_bwd(tab, x, d.B, d.T, d.F, w.scale, dfeats, w.dframes, ctx->an_cfg.fft32, s));
    SG_STAGE(SG_STAGE_AN_OVERLAP_ADD, launch_an_frames_to_wave(w.dframes, d.B, d.T, d.F, w.scale, grad_out, x_update, lower, upper, step, grad_sign, s));
    if (x_update && x_next != x_update)
        SG_HIP(hipMemcpyAsync(x_next, x_update, (size_t)d.B * d.T * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SG_OK;
}

// the buffer the fused overlap-add steps into (null: the separate pair updates in place)
float* an_step_target(sg_ctx* ctx, const AnDims& d, hipStream_t s) {
    AnWorkspace& w = ctx->an_ws;
    if (!an_use_ola(ctx, d.B, d.F)) return nullptr;
    if (dev_grow(ctx, w.allocs, &w.x_alt, (size_t)w.B * w.T, s)) return nullptr;  // falls back to the separate pair
    return w.x_alt;
}

// ---- the device-resident PGD loop (sg_an_pgd_run, sg_an_pgd_run_feco, sg_an_pgd_run_defended)
struct AnLoopCall {  // the caller's buffers, the chain and the feature-level defense, as the entry point received them
    float* x_adv;
    const int64_t* y; int coef_rows;  // the labels the head reads: the caller's B (coef_rows 0), or ws.y_rep, once per repeat (coef_rows B)
    const float* lower; const float* upper;
    int B, T;
    const sg_pgd_params* p;
    const sg_wav_stage* chain; int n_stages;  // n_stages 0: no chain
    const sg_feco_params* feco;               // null: no FeCo between front-end and network
    uint8_t* success; int64_t* decisions; float* scores; float* loss; float* loss_trace; int64_t* decision_trace;
};

// FeCo inside a loop: 1 <= k <= F cluster frames, enough of them for the stack
int an_feco_check(sg_ctx* ctx, const sg_feco_params* f, int B, int F) {
    const bool k_ok = f->k >= 1 && f->k <= F && f->max_iter >= 1;
    if (!an_plan(ctx, an_knobs(), B, k_ok ? f->k : 0, false).frames_ok)
        return fail(ctx, SG_ERR_ARG, "FeCo: need 1 <= k <= %d frames, enough of them for the AudioNet stack, max_iter >= 1", F);
    return SG_OK;
}

// One loop for every entry point.  A step's repeats are either `reps` repeats of the chain (AT: every repeat a row of its own
// through chain, model and both backwards, G per pass, the cotangents summed after the chain's backward in repeat order and
// carried from group to group), or R clusterings of FeCo behind ONE chain and front-end pass (their gradients summed at the
// feature level); never both (reps == 1 or R == 1).  identity: no chain, or one whose backward is the identity (QT / BDR only):
// d loss / d defended IS d loss / d iterate, and the log-mel adjoint steps the iterate directly -- the fused overlap-add from
// one waveform buffer into another, so the iterate alternates between the caller's buffer and a workspace twin and is copied
// home once if the attack ends on the twin.  Otherwise the adjoint writes a plane, the chain's backward follows and the
// repeat-sum kernel is the update, in place.
int an_pgd_loop(sg_ctx* ctx, const AnLoopCall& c, AnDims d, bool identity, int reps, int G, int R, hipStream_t s) {
    AnWorkspace& w = ctx->an_ws;
    DefWorkspace& dw = ctx->def_ws;
    const sg_pgd_params* p = c.p;
    const sg_feco_params* f = c.feco;
    const int B = c.B, T = c.T, F = d.F, Fnet = f ? f->k : F;  // Fnet: the frames the network sees in every pass
    const size_t n = (size_t)B * T;
    const int step_reps = reps * R, cap = G * R;  // repeats of a step at either level, and how many of them a pass holds
    const AnKnobs knobs = an_knobs();
    const int tail = step_reps % cap;  // repeats of a last, smaller group
    const AnNetPlan full_plan = an_plan(ctx, knobs, B * cap, Fnet, true), tail_plan = an_plan(ctx, knobs, B * (tail ? tail : cap), Fnet, true),
                    final_plan = an_plan(ctx, knobs, B, Fnet, false);
    const bool want_rec = c.loss_trace || c.decision_trace;
    d.B = B;
    float* xc = c.x_adv;
    float* xn = identity ? an_step_target(ctx, d, s) : nullptr;
    if (!xn) xn = c.x_adv;
    int rc;
    for (int it = 0; it <= p->max_iter; ++it) {
        float* lrec = c.loss_trace ? c.loss_trace + (size_t)it * B : nullptr;
        int64_t* drec = c.decision_trace ? c.decision_trace + (size_t)it * B : nullptr;
        for (int g0 = 0, more = 1; more; g0 += cap) {
            const LoopPass ps = loop_pass(it, p->max_iter, g0, cap, step_reps, B, want_rec);  // the final pass: one forward repeat
            more = !ps.final_group;
            const int Gc = f ? 1 : ps.Gi, Ri = f ? ps.Gi : 1;  // repeats in front of the log-mel front-end / clusterings behind it
            const int rows = B * Gc;
            const float* cur = xc;
            if (Gc > 1) {
                trace_mark(ctx, SG_STAGE_DEF_REPLICATE, s, 0);
                for (int r = 0; r < Gc; ++r)
                    SG_HIP(hipMemcpyAsync(dw.x_rep + (size_t)r * n, xc, n * sizeof(float), hipMemcpyDeviceToDevice, s));
                trace_mark(ctx, SG_STAGE_DEF_REPLICATE, s, 1);
                cur = dw.x_rep;
            }
            DefChainTape tape;  // (no stages: cur stays the iterate)
            if ((rc = def_chain_forward(ctx, c.chain, c.n_stages, cur, rows, T, ps.pass_key, Gc > 1 ? B : 0, &tape, &cur, s))) return rc;
            d.B = rows;
            // the model's range decision: iterates stay in [-1, 1], one decision serves; behind a chain it is taken from the
            // defended rows of every pass, as a model call takes it
            d.keep_scale = c.n_stages == 0 && it > 0;
            if ((rc = an_frontend_forward(ctx, cur, d, s))) return rc;
            const float* net_in = w.feats;
            float* dnet = w.dfeats;
            if (f) {
                trace_mark(ctx, SG_STAGE_AN_FECO_FWD, s, 0);
                rc = sg_feco_kmeans_compress(ctx, w.feats, B, F, kAnMel, f->k, f->max_iter, f->random_init, f->seed + ps.pass_key /* repeat r: + r * kRepKey */,
                                             f->index_base, Ri, w.feco_ids, w.feco_out, w.feco_cnt, s);
                if (rc) return rc;
                trace_mark(ctx, SG_STAGE_AN_FECO_FWD, s, 1);
                net_in = w.feco_out;
                dnet = w.dfeco;
            }
            // per-step records (LoopPass::Records): a pass of several repeats reduces its rows right after the head, the groups of
            // a step after the last one
            const AnHeadArgs head = an_head_args(ctx, c.y, p->loss, c.coef_rows, nullptr, ps.last ? c.scores : nullptr, ps.last ? c.decisions : nullptr,
                                                 ps.last ? c.loss : nullptr, loop_record_rows(ps, lrec, w.trace_l, w.eot_loss_rows.ptr),
                                                 loop_record_rows(ps, drec, w.trace_d, w.eot_dec_rows.ptr), ps.last ? c.success : nullptr);
            const AnEotRecords reduce = {ps.nrep, B, lrec, drec};
            const AnNetPlan& plan = ps.last ? final_plan : (ps.Gi == cap ? full_plan : tail_plan);
            rc = an_net_step(ctx, plan, net_in, ps.rows, head, ps.rec == LoopPass::PASS ? &reduce : nullptr, ps.last ? nullptr : dnet, s);
            if (rc) return rc;
            if (ps.rec == LoopPass::GROUPED && ps.reduce)
                SG_HIP(launch_eot_trace_reduce(w.eot_loss_rows, w.eot_dec_rows, ps.nrep, B, lrec, drec, s));
            if (ps.last) continue;
            if (f) {
                trace_mark(ctx, SG_STAGE_AN_FECO_BWD, s, 0);
                if ((rc = sg_feco_compress_backward_reps(ctx, w.dfeco, w.feco_ids, w.feco_cnt, B, F, kAnMel, f->k, 1, Ri, w.dfeats, s))) return rc;
                trace_mark(ctx, SG_STAGE_AN_FECO_BWD, s, 1);
            }
            if (identity) {  // straight into the update (one pass per step: Gc == 1)
                rc = an_frontend_backward(ctx, cur, d, w.dfeats, nullptr, xc, xn, c.lower, c.upper, p->step_size, p->grad_sign, s);
                if (rc) return rc;
                if (xn != xc) std::swap(xc, xn);
                continue;
            }
            if ((rc = an_frontend_backward(ctx, cur, d, w.dfeats, dw.g[0], nullptr, nullptr, nullptr, nullptr, 0.f, 0, s))) return rc;
            int gi = 0;
            if ((rc = def_chain_backward(ctx, c.chain, c.n_stages, tape, rows, T, &gi, s))) return rc;
            // the repeats' sum, carried to the next group or turned into the step
            SG_STAGE(SG_STAGE_DEF_REP_SUM,
                     launch_wav_rep_sum_update(dw.g[gi], Gc, (int64_t)n, g0 > 0 ? w.grad_carry : nullptr, ps.final_group ? nullptr : w.grad_carry,
                                               ps.final_group ? xc : nullptr, c.lower, c.upper, p->step_size, p->grad_sign, s));
        }
    }
    if (xc != c.x_adv) SG_HIP(hipMemcpyAsync(c.x_adv, xc, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SG_OK;
}

}  // namespace

extern "C" {

int32_t sg_an_num_frames(int32_t T) { return an_num_frames(T); }

int sg_an_load(sg_ctx* ctx, const sg_an_weights* w) {
    if (!ctx || !w) return SG_ERR_ARG;
    if (w->num_class < 1 || w->num_class > 1024) return fail(ctx, SG_ERR_ARG, "num_class must be 1..1024");
    if (!w->conv1_weight || !w->conv1_bias || !w->fc_weight || !w->fc_bias) return fail(ctx, SG_ERR_ARG, "missing tensor");
    for (int i = 0; i < 4; ++i)
        if (!w->bn1[i]) return fail(ctx, SG_ERR_ARG, "missing conv1 BatchNorm tensor");
    for (int l = 0; l < kAnConv; ++l)
        if (!w->conv_weight[l] || !w->conv_bias[l] || !w->bn_weight[l] || !w->bn_bias[l] || !w->bn_mean[l] || !w->bn_var[l])
            return fail(ctx, SG_ERR_ARG, "missing tensor for conv%d", l + 2);
    SG_HIP(hipSetDevice(ctx->device));
    int rc = an_build_tables(ctx);
    if (rc) return rc;
    const double eps = w->bn_eps > 0.f ? w->bn_eps : 1e-5;
    AnModel& m = ctx->an;
    m = AnModel();
    std::vector<void*>& pool = ctx->model_allocs;
    // BatchNorm (eval, affine) directly follows every convolution and precedes the ReLU
    // (audionet_csine.py:68-115): y = g (conv + b - mean) / sqrt(var + eps) + beta folds into W, b.
    {
        const double g = w->bn1[0][0], beta = w->bn1[1][0], mean = w->bn1[2][0], var = w->bn1[3][0];
        const double sc = g / std::sqrt(var + eps);
        std::vector<float> w25(25);
        for (int i = 0; i < 25; ++i) w25[i] = (float)(w->conv1_weight[i] * sc);  // [mel offset][time offset]
        m.pre_bias = (float)((w->conv1_bias[0] - mean) * sc + beta);
        rc |= dev_upload(ctx, pool, &m.w25, w25);
    }
    for (int l = 0; l < kAnConv; ++l) {
        const int cin = kAnCin[l], cout = kAnCout[l];
        std::vector<float> wf((size_t)3 * cin * cout), wb((size_t)3 * cout * cin), bias(cout);
        for (int co = 0; co < cout; ++co) {
            const double sc = w->bn_weight[l][co] / std::sqrt((double)w->bn_var[l][co] + eps);
            bias[co] = (float)((w->conv_bias[l][co] - w->bn_mean[l][co]) * sc + w->bn_bias[l][co]);
            for (int ci = 0; ci < cin; ++ci)
                for (int j = 0; j < 3; ++j) {
                    const float v = (float)(w->conv_weight[l][((size_t)co * cin + ci) * 3 + j] * sc);
                    wf[((size_t)j * cin + ci) * cout + co] = v;
                    wb[((size_t)j * cout + co) * cin + ci] = v;
                }
        }
        rc |= dev_upload(ctx, pool, &m.wf[l], wf);
        rc |= dev_upload(ctx, pool, &m.wb[l], wb);
        auto packed = [](const std::vector<float>& w, int K, int N) {  // [K][N] -> k4-major [K/4][N][4]
            std::vector<float> q((size_t)K * N);
            for (int k = 0; k < K; ++k)
                for (int n = 0; n < N; ++n) q[((size_t)(k / 4) * N + n) * 4 + (k & 3)] = w[(size_t)k * N + n];
            return q;
        };
        // (every layer: the fused CNN kernels take all their weights k4-packed; the per-layer sequence uses the packed copy
        // where its quad-fed tile kernel applies, N % 128 == 0)
        rc |= dev_upload(ctx, pool, &m.wfq[l], packed(wf, 3 * cin, cout));
        rc |= dev_upload(ctx, pool, &m.wbq[l], packed(wb, 3 * cout, cin));
        rc |= dev_upload(ctx, pool, &m.bias[l], bias);
    }
    rc |= dev_upload(ctx, pool, &m.fc_w, std::vector<float>(w->fc_weight, w->fc_weight + (size_t)w->num_class * 32));
    rc |= dev_upload(ctx, pool, &m.fc_b, std::vector<float>(w->fc_bias, w->fc_bias + w->num_class));
    if (rc) return fail(ctx, SG_ERR_HIP, "model upload failed: %s", ctx->err.c_str());
    m.S = w->num_class;
    m.loaded = true;
    return SG_OK;
}

int sg_an_logmel(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, float* feats_dev, void* stream) {
    if (!ctx || !x_dev || !feats_dev || B < 1 || T < kAnFft) return fail(ctx, SG_ERR_ARG, "bad argument");
    int rc = an_build_tables(ctx);
    if (rc) return rc;
    float* scale = nullptr;
    hipStream_t s = (hipStream_t)stream;
    AnTables tab = ctx->an_tab;
    if (ctx->an.loaded) {
        // with a model loaded the workspace is sized for (B, T) anyway: leave the mel energies there so that
        // sg_an_logmel_backward(reuse_forward) on the same input need not recompute the forward
        AnDims d;
        if ((rc = an_check(ctx, B, T, 0, &d))) return rc;
        AnWorkspace& w = ctx->an_ws;
        tab.mel_cache = w.mel_cache;
        w.cache_x = x_dev; w.cache_B = B; w.cache_T = T; w.cache_spec = false;
    } else if (!ctx->an_ws.scale) {
        rc = an_ensure_workspace(ctx, 1, kAnFft, an_num_frames(kAnFft) + 40);
        if (rc) return rc;
    }
    scale = ctx->an_ws.scale;
    SG_HIP(launch_input_scale(x_dev, (int64_t)B * T, ctx->range_scratch, scale, 1, s));
    SG_HIP(launch_an_logmel_fwd(tab, x_dev, B, T, an_num_frames(T), scale, feats_dev, ctx->an_cfg.fft32, s));
    return SG_OK;
}

int sg_an_logmel_backward(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, const float* dfeats_dev, float* grad_dev,
                          int32_t reuse_forward, void* stream) {
    if (!x_dev || !dfeats_dev || !grad_dev) return fail(ctx, SG_ERR_ARG, "bad argument");
    AnDims d;
    int rc = an_check(ctx, B, T, 0, &d);  // sizes the per-frame gradient scratch
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    AnWorkspace& w = ctx->an_ws;
    AnTables tab = ctx->an_tab;
    if (reuse_forward && w.cache_x == x_dev && w.cache_B == B && w.cache_T == T) {
        tab.mel_cache = w.mel_cache;
        tab.spec_cache = w.cache_spec ? w.spec_cache : nullptr;
    }
    SG_HIP(launch_input_scale(x_dev, (int64_t)B * T, ctx->range_scratch, w.scale, 1, s));
    if (tab.mel_cache && an_use_ola(ctx, d.B, d.F)) {  // the attack loops' form of the adjoint (same sums in the same order as the pair below)
        AnOlaArgs a{};
        a.x = x_dev; a.dfeats = dfeats_dev; a.dframes = w.dframes; a.grad_out = grad_dev; a.scale_p = w.scale;
        a.B = d.B; a.T = d.T; a.F = d.F;
        SG_HIP(launch_an_logmel_bwd_ola(tab, a, ctx->an_cfg.fft32, ctx->num_cus, s));
        return SG_OK;
    }
    SG_HIP(launch_an_logmel_bwd(tab, x_dev, d.B, d.T, d.F, w.scale, dfeats_dev, w.dframes, ctx->an_cfg.fft32, s));
    SG_HIP(launch_an_frames_to_wave(w.dframes, d.B, d.T, d.F, w.scale, grad_dev, nullptr, nullptr, nullptr, 0.f, 1, s));
    return SG_OK;
}

int sg_an_configure(sg_ctx* ctx, int32_t fft_bits, int32_t spectrum_cache, int32_t fused_overlap_add) {
    if (!ctx) return SG_ERR_ARG;
    if (fft_bits != 32 && fft_bits != 64) return fail(ctx, SG_ERR_ARG, "fft_bits must be 32 or 64");
    ctx->an_cfg.fft32 = fft_bits == 32;
    ctx->an_cfg.spec_cache = spectrum_cache < 0 ? -1 : (spectrum_cache != 0);
    ctx->an_cfg.ola = fused_overlap_add < 0 ? -1 : (fused_overlap_add != 0);
    ctx->an_ws.cache_x = nullptr;  // what an earlier forward left behind was computed under the old settings
    ctx->an_ws.cache_spec = false;
    return SG_OK;
}

int sg_an_forward(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T_or_F, int32_t flag, int64_t* decisions_dev,
                  float* scores_dev, float* emb_dev, void* stream) {
    AnDims d;
    int rc = an_check(ctx, B, T_or_F, flag, &d);
    if (rc) return rc;
    if (!x_dev) return fail(ctx, SG_ERR_ARG, "x is NULL");
    hipStream_t s = (hipStream_t)stream;
    const AnNetPlan plan = an_plan(ctx, an_knobs(), B, d.F, false);
    const float* feats = x_dev;
    if (flag == 0) {
        if ((rc = an_frontend_forward(ctx, x_dev, d, s))) return rc;
        feats = ctx->an_ws.feats;
    }
    const AnHeadArgs head = an_head_args(ctx, nullptr, sg_loss_spec{}, 0, emb_dev, scores_dev, decisions_dev, nullptr, nullptr, nullptr, nullptr);
    return an_net_step(ctx, plan, feats, B, head, nullptr, nullptr, s);
}

int sg_an_debug_activation(sg_ctx* ctx, int32_t layer, float* out_dev, int64_t capacity_floats, int32_t* rows_per_utt,
                           int32_t* channels, void* stream) {
    if (!ctx || layer < 1 || layer > kAnConv + 1 || !ctx->an_ws.scale) return fail(ctx, SG_ERR_ARG, "bad layer or no pass run");
    const AnWorkspace& w = ctx->an_ws;
    const float* src;
    int rows, ch;
    if (layer == 1) { src = w.pre; rows = w.F >= 0 ? w.Tin[0] : 0; ch = kAnMel; }
    else {
        const int l = layer - 2;
        src = kAnPool[l] ? w.pool[l] : w.act[l];
        rows = kAnPool[l] ? w.Tout[l] / 2 : w.Tout[l];
        ch = kAnCout[l];
    }
    if (rows_per_utt) *rows_per_utt = rows;
    if (channels) *channels = ch;
    if (out_dev) {
        if (capacity_floats <= 0) return fail(ctx, SG_ERR_ARG, "capacity must be positive");
        const size_t held = (size_t)w.B * (size_t)(rows > 0 ? rows : 1) * ch;  // never read past what the workspace holds
        const size_t n = (size_t)capacity_floats < held ? (size_t)capacity_floats : held;
        SG_HIP(hipMemcpyAsync(out_dev, src, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return SG_OK;
}

int sg_an_loss_grad(sg_ctx* ctx, const float* x_dev, const int64_t* y_dev, int32_t B, int32_t T_or_F, int32_t flag,
                    const sg_loss_spec* loss, int64_t* decisions_dev, float* scores_dev, float* loss_dev, float* grad_dev,
                    void* stream) {
    AnDims d;
    int rc = an_check(ctx, B, T_or_F, flag, &d);
    if (rc) return rc;
    if (!x_dev || !y_dev || !loss) return fail(ctx, SG_ERR_ARG, "x, y and loss are required");
    if (loss->loss == SG_LOSS_LINEAR && !loss->coef_dev) return fail(ctx, SG_ERR_ARG, "SG_LOSS_LINEAR needs coef_dev");
    hipStream_t s = (hipStream_t)stream;
    AnWorkspace& w = ctx->an_ws;
    const AnNetPlan plan = an_plan(ctx, an_knobs(), B, d.F, grad_dev != nullptr);
    const float* feats = x_dev;
    if (flag == 0) {
        if ((rc = an_frontend_forward(ctx, x_dev, d, s))) return rc;
        feats = w.feats;
    }
    const AnHeadArgs head = an_head_args(ctx, y_dev, *loss, 0, nullptr, scores_dev, decisions_dev, loss_dev, nullptr, nullptr, nullptr);
    float* dfeats = !grad_dev ? nullptr : flag == 1 ? grad_dev : w.dfeats;
    if ((rc = an_net_step(ctx, plan, feats, B, head, nullptr, dfeats, s)) || !grad_dev) return rc;
    if (flag == 0 && (rc = an_frontend_backward(ctx, x_dev, d, w.dfeats, grad_dev, nullptr, nullptr, nullptr, nullptr, 0.f, 0, s))) return rc;
    if (plan.form == AN_PER_LAYER) { w.grad_B = B; w.grad_F = d.F; }  // what sg_an_debug_gradient may read back
    return SG_OK;
}

int sg_an_debug_gradient(sg_ctx* ctx, int32_t which, float* out_dev, int64_t capacity_floats, int32_t* dims, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    const AnWorkspace& w = ctx->an_ws;
    if (!w.scale || w.grad_B < 1)
        return fail(ctx, SG_ERR_STATE, "sg_an_debug_gradient: the last AudioNet pass on this context was not an sg_an_loss_grad call with a gradient "
                                       "in the per-layer form (the fused forms keep these tensors in LDS)");
    const int B = w.grad_B, F = w.grad_F;
    int Tin[kAnConv], Tout[kAnConv];
    an_layer_frames(F, Tin, Tout);
    static const int kPooled[3] = {0, 3, 5};  // conv2, conv5, conv7: the layers with a MaxPool (kAnPool)
    const float* src = nullptr;
    int rows = 0, cols = 0;
    if (which >= SG_AN_GRAD_DACT1 && which < SG_AN_GRAD_DACT1 + kAnConv) {
        const int l = which - SG_AN_GRAD_DACT1;
        src = w.dact[l]; rows = Tout[l]; cols = kAnCout[l];
    }
    else if (which >= SG_AN_GRAD_DPOOL1 && which <= SG_AN_GRAD_DPOOL6) {
        const int l = kPooled[which - SG_AN_GRAD_DPOOL1];
        src = w.dpool[l]; rows = Tout[l] / 2; cols = kAnCout[l];
    }
    else if (which == SG_AN_GRAD_DPRE) { src = w.dpre; rows = F; cols = kAnMel; }
    else if (which == SG_AN_GRAD_PRE) { src = w.pre; rows = F; cols = kAnMel; }
    else if (which >= SG_AN_GRAD_ACT1_UNPOOLED && which <= SG_AN_GRAD_ACT6_UNPOOLED) {
        const int l = kPooled[which - SG_AN_GRAD_ACT1_UNPOOLED];
        src = w.act[l]; rows = Tout[l]; cols = kAnCout[l];
    }
    else return fail(ctx, SG_ERR_ARG, "sg_an_debug_gradient: unknown buffer %d", which);
    if (dims) { dims[0] = 1; dims[1] = B; dims[2] = rows; dims[3] = cols; }
    if (out_dev) {
        // the pass fits its workspace (B <= w.B, F <= w.F) and every buffer is one contiguous run at the pass's own strides
        const size_t n = (size_t)B * rows * cols;
        if (capacity_floats < 0 || (size_t)capacity_floats < n)
            return fail(ctx, SG_ERR_ARG, "sg_an_debug_gradient: capacity of %lld floats, the buffer holds %zu", (long long)capacity_floats, n);
        SG_HIP(hipSetDevice(ctx->device));
        SG_HIP(hipMemcpyAsync(out_dev, src, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return SG_OK;
}

int sg_an_pgd_run(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev, const float* upper_dev,
                  int32_t B, int32_t T, const sg_pgd_params* p, uint8_t* success_dev, int64_t* decisions_dev,
                  float* scores_dev, float* loss_dev, float* loss_trace_dev, int64_t* decision_trace_dev, void* stream) {
    AnDims d;
    int rc = an_check(ctx, B, T, 0, &d);
    if (rc) return rc;
    if ((rc = loop_check_args(ctx, !x_adv_dev || !y_dev || !lower_dev || !upper_dev || !p, nullptr, p))) return rc;
    // the model is deterministic: one pass stands for every EOT repeat, and the final pass is a single forward
    const AnLoopCall c{x_adv_dev, y_dev, 0, lower_dev, upper_dev, B, T, p, nullptr, 0, nullptr,
                       success_dev, decisions_dev, scores_dev, loss_dev, loss_trace_dev, decision_trace_dev};
    return an_pgd_loop(ctx, c, d, true, 1, 1, 1, (hipStream_t)stream);
}

int sg_an_pgd_run_feco(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev, const float* upper_dev,
                       int32_t B, int32_t T, const sg_pgd_params* p, const sg_feco_params* f, uint8_t* success_dev,
                       int64_t* decisions_dev, float* scores_dev, float* loss_dev, float* loss_trace_dev,
                       int64_t* decision_trace_dev, void* stream) {
    int rc, eot_size;
    if (!ctx) return SG_ERR_ARG;
    if ((rc = loop_check_args(ctx, !x_adv_dev || !y_dev || !lower_dev || !upper_dev || !p || !f, nullptr, p))) return rc;
    // defense/feature_level.py:33: with a single utterance the reference DROPS empty clusters (variable frame count);
    // that case stays on the host-chained path (model/defended_model.py)
    if (B < 2) return fail(ctx, SG_ERR_ARG, "the fused FeCo loop needs a batch of at least 2 utterances");
    if ((rc = loop_eot_size(ctx, p, &eot_size))) return rc;
    // Expectation over the defense's randomness (adaptive_attack/EOT.py:16-54): eot_size clusterings per gradient step,
    // each started from fresh random frames.  The reference repeats the batch (x_batch.repeat, EOT.py:24) and runs the
    // whole model on the copies; only the DEFENSE is random here, so the log-mel front-end runs once per step, the R
    // clusterings and the CNN run as one batch of R x B, and because the compression is linear in the features the
    // repeats' gradients are summed at the feature level (repeat order) and ONE log-mel adjoint + overlap-add takes the
    // sum to the waveform: sign(sum) == sign(mean).  (EOT_batch_size only says how the reference cuts the repeats into
    // model calls.)  The evenly started clustering is a deterministic function of its input: every repeat is the same
    // computation, one stands for all.  The final pass is a single forward.
    const int R = f->random_init ? eot_size : 1;
    AnDims d;
    if ((rc = an_check(ctx, B * R, T, 0, &d))) return rc;  // workspace for the batch of R x B rows
    if ((rc = an_feco_check(ctx, f, B, d.F))) return rc;
    hipStream_t s = (hipStream_t)stream;
    AnWorkspace& w = ctx->an_ws;
    for (int r = 0; r < R; ++r)
        SG_HIP(hipMemcpyAsync(w.y_rep + (size_t)r * B, y_dev, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    const AnLoopCall c{x_adv_dev, w.y_rep, B, lower_dev, upper_dev, B, T, p, nullptr, 0, f,
                       success_dev, decisions_dev, scores_dev, loss_dev, loss_trace_dev, decision_trace_dev};
    return an_pgd_loop(ctx, c, d, true, 1, 1, R, s);
}

int sg_an_pgd_run_defended(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev, const float* upper_dev,
                           int32_t B, int32_t T, const sg_pgd_params* p, const sg_wav_stage* chain, int32_t n_stages,
                           const sg_feco_params* feco, uint8_t* success_dev, int64_t* decisions_dev, float* scores_dev,
                           float* loss_dev, float* loss_trace_dev, int64_t* decision_trace_dev, void* stream) {
    static const char* who = "sg_an_pgd_run_defended";
    int rc, eot_size;
    if (!ctx) return SG_ERR_ARG;
    const char* shape = B < 1 || T < kAnFft ? "need B >= 1 and a waveform of at least one 1024-sample STFT frame" : nullptr;
    if ((rc = loop_check_args(ctx, !x_adv_dev || !y_dev || !lower_dev || !upper_dev || !p, shape, p))) return rc;
    if ((rc = loop_eot_size(ctx, p, &eot_size))) return rc;
    // ---- the chain: everything a stage call would refuse, before the first launch
    DefChainInfo ci;
    if ((rc = def_chain_check(ctx, who, chain, n_stages, &ci))) return rc;
    if (feco) {
        // (one utterance: the reference drops empty clusters, sg_an_pgd_run_feco)
        if (B < 2) return fail(ctx, SG_ERR_ARG, "%s: the FeCo loop needs a batch of at least 2 utterances", who);
        // the clusterings' gradients are summed at the feature level, behind ONE chain pass: that pass must not be random
        if (ci.randomised) return fail(ctx, SG_ERR_ARG, "%s: a randomised stage (AT) in front of FeCo is not supported in the loop", who);
    }
    // Repeats: AT makes the repeats of a step differ (AudioNet has no dither); otherwise one pass stands for all.  With FeCo
    // only the clustering is repeated (R times, behind one chain and front-end pass).
    const int reps = !feco && ci.randomised ? eot_size : 1;
    const int R = feco && feco->random_init ? eot_size : 1;
    long cap = 65535;  // rows a stage kernel takes
    if (const char* e = sg_tune_env("SG_EOT_MAX_ROWS")) cap = std::min<long>(cap, atol(e));  // tests: force groups
    const int G = (int)std::min<long>(reps, std::max<long>(1, cap / B));
    const bool per_row = !ci.identity;  // the chain has a backward of its own: cotangent planes are needed
    const int chain_rows = B * G;
    if (chain_rows > 65535) return fail(ctx, SG_ERR_ARG, "%s: %d rows per pass, the stage kernels take at most 65535: split the batch", who, chain_rows);
    AnDims d;
    if ((rc = an_check(ctx, feco ? B * R : chain_rows, T, 0, &d))) return rc;  // workspace for the largest pass
    if (feco && (rc = an_feco_check(ctx, feco, B, d.F))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_def_workspace(ctx, chain_rows, T, n_stages, ci.n_saved, per_row, s)))
        return fail(ctx, rc, "%s: %s", who, ctx->err.c_str());
    AnWorkspace& w = ctx->an_ws;
    if (G < reps) {  // the repeats of a step run as several passes: the carried sum, and the rows of LoopPass::GROUPED
        const bool want_rec = loss_trace_dev || decision_trace_dev;
        if ((rc = dev_grow(ctx, w.allocs, &w.grad_carry, (size_t)B * T, s))) return rc;
        if (want_rec && (rc = dev_grow(ctx, w.allocs, &w.eot_loss_rows, (size_t)reps * B, s))) return rc;
        if (want_rec && (rc = dev_grow(ctx, w.allocs, &w.eot_dec_rows, (size_t)reps * B, s))) return rc;
    }
    for (int r = 0; r < (feco ? R : G); ++r)
        SG_HIP(hipMemcpyAsync(w.y_rep + (size_t)r * B, y_dev, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    // the iterate is clamped into [lower, upper] within [-1, 1] at every step: a first stage's decision is taken once
    if ((rc = def_chain_first_scale(ctx, chain, x_adv_dev, (int64_t)B * T, s))) return fail(ctx, rc, "%s: %s", who, ctx->err.c_str());
    const AnLoopCall c{x_adv_dev, w.y_rep, B, lower_dev, upper_dev, B, T, p, chain, n_stages, feco,
                       success_dev, decisions_dev, scores_dev, loss_dev, loss_trace_dev, decision_trace_dev};
    return an_pgd_loop(ctx, c, d, ci.identity, reps, G, R, s);
}

}  // extern "C"
