// C-ABI entry points of the GMM / i-vector / PLDA system (include/speakerguard_hip.h, kernels: k_ivector.hip): model load
// (the packing of k_ivector.hip's tables), the chunk workspace, the stage entries, the forward pass and the gradient
// (k_ivector_bwd.hip): a chunk's backward runs right after its forward, on the chunk's buffers.
#include <cmath>
#include <cstring>

#include "sg_internal.h"

using namespace sg;

namespace {

struct IvDims {
    int B, TF, flag;
    int T;   // samples per row (flag 0), else 0
    int F;   // frames per row
    int chunk;
};

int iv_check_dims(sg_ctx* ctx, const char* who, int B, int TF, int flag, IvDims* d) {
    if (!ctx) return SG_ERR_ARG;
    if (!ctx->iv.loaded) return fail(ctx, SG_ERR_STATE, "%s: no i-vector model loaded (sg_iv_load)", who);
    if (B < 1 || B > (1 << 20)) return fail(ctx, SG_ERR_ARG, "%s: B must be 1 .. 2^20", who);
    if (flag < SG_IV_FLAG_WAV || flag > SG_IV_FLAG_CMVN) return fail(ctx, SG_ERR_ARG, "%s: flag must be 0 .. 3", who);
    d->B = B; d->TF = TF; d->flag = flag; d->T = 0;
    if (flag == SG_IV_FLAG_WAV) {
        if (TF < kWin || TF > (1 << 24)) return fail(ctx, SG_ERR_ARG, "%s: T must be %d .. 2^24 samples", who, kWin);
        d->T = TF;
        d->F = num_frames(TF);
    } else {
        d->F = TF;
    }
    if (d->F < 1 || d->F > 65535) return fail(ctx, SG_ERR_ARG, "%s: F must be 1 .. 65535 frames", who);
    d->chunk = std::min(B, iv_chunk_rows(d->F, ctx->iv.C));
    return SG_OK;
}

// the chunk buffers of a call of `chunk` utterances x F frames (and T samples when the MFCC runs); grown before any launch
int iv_ensure_workspace(sg_ctx* ctx, int chunk, int F, bool wav, hipStream_t s, bool grad = false) {
    IvWorkspace& w = ctx->iv_ws;
    const IvModel& m = ctx->iv;
    const size_t rows = (size_t)chunk * F;
    const int NS = (m.C + kIvLinSlice - 1) / kIvLinSlice;
    int rc = SG_OK;
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.scale, 1, s);
    if (!rc && wav) rc = dev_grow(ctx, w.allocs, &w.raw, rows * kCep, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.delta, rows * kIvDim, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.cmvn, rows * kIvDim, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.ll, rows * m.C, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.rowmax, rows, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.rowsum, rows, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.n, (size_t)chunk * m.C, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.f, (size_t)chunk * m.C * kIvDim, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.ivec, (size_t)chunk * m.R, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.Lmat, (size_t)chunk * m.Pp, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.linpart, (size_t)NS * chunk * m.R, s);
    if (!grad) return rc;
    // what only the gradient keeps: the solved vector, lambda, the adjoint statistics, a second (frames, Cp) buffer for
    // dgamma / dll, and the feature gradients on the way to the caller's flag
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.solved, (size_t)chunk * m.R, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.lam, (size_t)chunk * m.R, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.dw, (size_t)chunk * m.R, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.dnpart, (size_t)iv_dn_slices(m.P) * chunk * m.C, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.dn, (size_t)chunk * m.C, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.df, (size_t)chunk * m.C * kIvDim, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.dg, rows * m.Cp, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.dxpart, kIvDxSplit * rows * kIvDim, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.dcmvn, rows * kIvDim, s);
    if (!rc) rc = dev_grow(ctx, w.allocs, &w.ddelta, rows * kIvDim, s);
    if (!rc && wav) rc = dev_grow(ctx, w.allocs, &w.draw, rows * kCep, s);
    if (!rc && wav) rc = dev_grow(ctx, w.allocs, &w.dframes, rows * kWin, s);
    return rc;
}

// one forward: the whole call's scale decision first (model/utils.py:7-19), then chunk after chunk
int iv_run(sg_ctx* ctx, const char* who, const float* x, const int64_t* y, int B, int TF, int flag, const sg_loss_spec* loss,
           const sg_dither* dither, int64_t* dec, float* scores, float* emb, float* ivec_out, float* loss_out, hipStream_t s,
           float* grad = nullptr) {
    IvDims d;
    int rc = iv_check_dims(ctx, who, B, TF, flag, &d);
    if (rc) return rc;
    if (!x) return fail(ctx, SG_ERR_ARG, "%s: x is NULL", who);
    if (loss && loss->loss == SG_LOSS_LINEAR && !loss->coef_dev) return fail(ctx, SG_ERR_ARG, "%s: SG_LOSS_LINEAR needs coef_dev", who);
    if (loss && loss->loss != SG_LOSS_LINEAR && !y) return fail(ctx, SG_ERR_ARG, "%s: y is NULL", who);
    SG_HIP(hipSetDevice(ctx->device));
    if (grad && !loss) return fail(ctx, SG_ERR_ARG, "%s: loss is NULL", who);
    if ((rc = iv_ensure_workspace(ctx, d.chunk, d.F, flag == SG_IV_FLAG_WAV, s, grad != nullptr))) return rc;
    IvWorkspace& w = ctx->iv_ws;
    const IvModel& m = ctx->iv;
    const float* enroll;
    int S;
    plda_backend_active(m.be, &enroll, &S);
    if (flag == SG_IV_FLAG_WAV && (rc = sg_input_scale(ctx, x, (int64_t)B * d.T, w.scale, s))) return rc;
    for (int b0 = 0; b0 < B; b0 += d.chunk) {
        const int nb = std::min(d.chunk, B - b0);
        const size_t row_floats = flag == SG_IV_FLAG_WAV ? (size_t)d.T : (size_t)d.F * (flag == SG_IV_FLAG_RAW ? kIvCep : kIvDim);
        const float* xc = x + (size_t)b0 * row_floats;
        const float* cm = w.cmvn;
        sg_dither dz{};
        if (flag == SG_IV_FLAG_WAV) {
            if (dither) dz = *dither;
            dz.row_base += b0;  // the chunk is a slice of the call: same noise as in one piece
            if (dz.noise_dev) dz.noise_dev += (size_t)b0 * d.F * kWin;
            if ((rc = sg_xv_mfcc(ctx, xc, nb, d.T, w.scale, &dz, w.raw, s))) return rc;
            SG_HIP(launch_iv_delta_cmvn(w.raw, kCep, nb, d.F, w.delta, nullptr, w.cmvn, s));
        } else if (flag == SG_IV_FLAG_RAW) {
            SG_HIP(launch_iv_delta_cmvn(xc, kIvCep, nb, d.F, w.delta, nullptr, w.cmvn, s));
        } else if (flag == SG_IV_FLAG_DELTA) {
            // no raw rows: the kernel takes the caller's delta rows as they are (it only reads them) and runs the CMVN
            SG_HIP(launch_iv_delta_cmvn(nullptr, 0, nb, d.F, const_cast<float*>(xc), nullptr, w.cmvn, s));
        } else {
            cm = xc;
        }
        SG_HIP(launch_iv_stats(m, cm, nb, d.F, w.ll, w.rowmax, w.rowsum, w.n, w.f, s));
        SG_HIP(launch_iv_extract(m, w.n, w.f, nb, w.Lmat, w.linpart, w.ivec, s, grad ? w.solved.ptr : nullptr));
        if (ivec_out) SG_HIP(hipMemcpyAsync(ivec_out + (size_t)b0 * m.R, w.ivec, (size_t)nb * m.R * sizeof(float), hipMemcpyDeviceToDevice, s));
        IvTailArgs t{};
        t.ivec = w.ivec; t.B = nb;
        t.y = (loss && y) ? y + b0 : nullptr;
        if (loss) {
            t.loss = *loss;
            t.coef = loss->coef_dev ? loss->coef_dev + (size_t)b0 * S : nullptr;
        }
        t.emb = emb ? emb + (size_t)b0 * m.be.D : nullptr;
        t.scores = scores ? scores + (size_t)b0 * S : nullptr;
        t.decisions = dec ? dec + b0 : nullptr;
        t.loss_out = (loss && loss_out) ? loss_out + b0 : nullptr;
        t.dw = grad ? w.dw.ptr : nullptr;
        SG_HIP(launch_iv_tail(m, t, s));
        if (!grad) continue;
        // the chunk's backward, on the state its forward left: the factor in Lmat, ll, the row maxima and sums
        float* gc = grad + (size_t)b0 * row_floats;
        SG_HIP(launch_iv_extract_bwd(m, w.dw, nb, w.Lmat, w.solved, w.lam, w.dnpart, w.dn, w.df, s));
        SG_HIP(launch_iv_stats_bwd(m, cm, nb, d.F, w.ll, w.rowmax, w.rowsum, w.dn, w.df, w.dg, w.dxpart,
                                   flag == SG_IV_FLAG_CMVN ? gc : w.dcmvn.ptr, s));
        if (flag == SG_IV_FLAG_DELTA) {
            SG_HIP(launch_iv_delta_cmvn_bwd(w.dcmvn, true, nb, d.F, gc, nullptr, 0, s));
        } else if (flag == SG_IV_FLAG_RAW) {
            SG_HIP(launch_iv_delta_cmvn_bwd(w.dcmvn, true, nb, d.F, w.ddelta, gc, kIvCep, s));
        } else if (flag == SG_IV_FLAG_WAV) {
            // d raw zero-padded to the MFCC's 30 columns, then the MFCC adjoint with the forward's scale and dither keys, on the
            // chunk's own frame buffer
            SG_HIP(launch_iv_delta_cmvn_bwd(w.dcmvn, true, nb, d.F, w.ddelta, w.draw, kCep, s));
            if ((rc = mfcc_adjoint(ctx, ctx->tab, xc, nb, d.T, d.F, w.scale, &dz, w.draw, w.dframes, 1, nullptr, gc, nullptr, nullptr,
                                   nullptr, 0.f, 1, false, s)))
                return rc;
        }
    }
    return SG_OK;
}

}  // namespace

extern "C" {

int sg_iv_load(sg_ctx* ctx, const sg_iv_weights* w) {
    if (!ctx || !w) return fail(ctx, SG_ERR_ARG, "sg_iv_load: NULL argument");
    if (!w->gconsts || !w->means_invcovars || !w->invcovars || !w->extractor || !w->sigma_inv || !w->emb_mean || !w->lda ||
        !w->plda_mean || !w->plda_transform || !w->plda_psi || !w->enroll)
        return fail(ctx, SG_ERR_ARG, "sg_iv_load: a weight pointer is NULL");
    const int C = w->C, R = w->R, D = w->D, S = w->S;
    if (C < 1 || C > kIvMaxC || R < 1 || R > kIvMaxR || D < 1 || D > kIvMaxD || S < 1 || S > 1024)
        return fail(ctx, SG_ERR_ARG, "sg_iv_load: C must be 1 .. %d, R 1 .. %d, D 1 .. %d, S 1 .. 1024", kIvMaxC, kIvMaxR, kIvMaxD);
    if (!std::isfinite(w->ivector_offset)) return fail(ctx, SG_ERR_ARG, "sg_iv_load: the i-vector offset is not finite");
    const int Cp = (C + 63) / 64 * 64, P = R * (R + 1) / 2, Pp = (P + 255) / 256 * 256;
    std::vector<float> W, Vt, U;
    std::vector<uint16_t> pairs;
    std::string why;
    if (!iv_pack_model(w, Cp, Pp, &W, &pairs, &Vt, &U, &why)) return fail(ctx, SG_ERR_ARG, "sg_iv_load: %s", why.c_str());
    SG_HIP(hipSetDevice(ctx->device));
    SG_HIP(hipDeviceSynchronize());
    IvModel& m = ctx->iv;
    for (void* p : m.allocs) (void)hipFree(p);
    m = IvModel();
    std::vector<void*>& pool = m.allocs;
    std::vector<float> ldat((size_t)(R + 1) * D), pt((size_t)D * D);
    for (int d = 0; d < D; ++d) {
        for (int k = 0; k <= R; ++k) ldat[(size_t)k * D + d] = w->lda[(size_t)d * (R + 1) + k];
        for (int j = 0; j < D; ++j) pt[(size_t)j * D + d] = w->plda_transform[(size_t)d * D + j];
    }
    int rc = SG_OK;
    rc |= dev_upload(ctx, pool, &m.gconst, std::vector<float>(w->gconsts, w->gconsts + C));
    rc |= dev_upload(ctx, pool, &m.W, W);
    rc |= dev_upload(ctx, pool, &m.pairs, pairs);
    rc |= dev_upload(ctx, pool, &m.Vt, Vt);
    rc |= dev_upload(ctx, pool, &m.U, U);
    rc |= dev_upload(ctx, pool, &m.emb_mean, std::vector<float>(w->emb_mean, w->emb_mean + R));
    rc |= dev_upload(ctx, pool, &m.lda_t, ldat);
    rc |= dev_upload(ctx, pool, &m.plda_pt, pt);
    rc |= plda_backend_load(ctx, pool, &m.be, w->plda_mean, w->plda_psi, w->enroll, D, S, w->threshold);
    if (rc) return fail(ctx, SG_ERR_HIP, "sg_iv_load: model upload failed: %s", ctx->err.c_str());
    m.C = C; m.Cp = Cp; m.R = R; m.P = P; m.Pp = Pp;
    m.offset = w->ivector_offset;
    m.loaded = true;
    return SG_OK;
}

int sg_iv_set_enroll(sg_ctx* ctx, const float* enroll_host, int32_t S, float threshold) {
    if (!ctx || !ctx->iv.loaded) return fail(ctx, SG_ERR_STATE, "no i-vector model loaded");
    if (S < 1 || S > 1024) return fail(ctx, SG_ERR_ARG, "S must be 1..1024");
    return plda_backend_set_enroll(ctx, &ctx->iv.be, ctx->iv.allocs, enroll_host, S, threshold);
}

int sg_iv_enroll_override(sg_ctx* ctx, const float* enroll_dev, int32_t S) {
    if (!ctx || !ctx->iv.loaded) return fail(ctx, SG_ERR_STATE, "no i-vector model loaded");
    if (enroll_dev && (S < 1 || S > 1024)) return fail(ctx, SG_ERR_ARG, "S must be 1..1024");
    plda_backend_override(&ctx->iv.be, enroll_dev, S);
    return SG_OK;
}

int sg_iv_delta_cmvn(sg_ctx* ctx, const float* raw_dev, int32_t B, int32_t F, int32_t ld, float* delta_dev, float* cmvn_dev,
                     void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (!raw_dev || (!delta_dev && !cmvn_dev)) return fail(ctx, SG_ERR_ARG, "sg_iv_delta_cmvn: NULL argument");
    if (B < 1 || B > (1 << 20) || F < 1 || F > 65535 || ld < kIvCep || ld > 4096)
        return fail(ctx, SG_ERR_ARG, "sg_iv_delta_cmvn: B must be 1 .. 2^20, F 1 .. 65535, ld %d .. 4096", kIvCep);
    hipStream_t s = (hipStream_t)stream;
    SG_HIP(hipSetDevice(ctx->device));
    // the kernel reads its delta rows back, so they need a home even when the caller does not want them: chunks of the workspace
    IvWorkspace& w = ctx->iv_ws;
    const int chunk = std::min<int64_t>(B, std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)F * kIvDim * 4)));
    int rc = delta_dev ? SG_OK : dev_grow(ctx, w.allocs, &w.delta, (size_t)chunk * F * kIvDim, s);
    if (rc) return rc;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const size_t o = (size_t)b0 * F;
        float* home = delta_dev ? delta_dev + o * kIvDim : w.delta.ptr;
        SG_HIP(launch_iv_delta_cmvn(raw_dev + o * ld, ld, nb, F, home, nullptr, cmvn_dev ? cmvn_dev + o * kIvDim : nullptr, s));
    }
    return SG_OK;
}

int sg_iv_stats(sg_ctx* ctx, const float* cmvn_dev, int32_t B, int32_t F, float* zeroth_dev, float* first_dev, void* stream) {
    IvDims d;
    int rc = iv_check_dims(ctx, "sg_iv_stats", B, F, SG_IV_FLAG_CMVN, &d);
    if (rc) return rc;
    if (!cmvn_dev || !zeroth_dev || !first_dev) return fail(ctx, SG_ERR_ARG, "sg_iv_stats: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    SG_HIP(hipSetDevice(ctx->device));
    if ((rc = iv_ensure_workspace(ctx, d.chunk, d.F, false, s))) return rc;
    IvWorkspace& w = ctx->iv_ws;
    const IvModel& m = ctx->iv;
    for (int b0 = 0; b0 < B; b0 += d.chunk) {
        const int nb = std::min(d.chunk, B - b0);
        SG_HIP(launch_iv_stats(m, cmvn_dev + (size_t)b0 * F * kIvDim, nb, F, w.ll, w.rowmax, w.rowsum, zeroth_dev + (size_t)b0 * m.C,
                               first_dev + (size_t)b0 * m.C * kIvDim, s));
    }
    return SG_OK;
}

int sg_iv_extract(sg_ctx* ctx, const float* zeroth_dev, const float* first_dev, int32_t B, float* ivector_dev, void* stream) {
    IvDims d;
    int rc = iv_check_dims(ctx, "sg_iv_extract", B, 1, SG_IV_FLAG_CMVN, &d);
    if (rc) return rc;
    if (!zeroth_dev || !first_dev || !ivector_dev) return fail(ctx, SG_ERR_ARG, "sg_iv_extract: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    SG_HIP(hipSetDevice(ctx->device));
    const int chunk = std::min(B, kIvChunkMax);
    if ((rc = iv_ensure_workspace(ctx, chunk, 1, false, s))) return rc;
    IvWorkspace& w = ctx->iv_ws;
    const IvModel& m = ctx->iv;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        SG_HIP(launch_iv_extract(m, zeroth_dev + (size_t)b0 * m.C, first_dev + (size_t)b0 * m.C * kIvDim, nb, w.Lmat, w.linpart,
                                 ivector_dev + (size_t)b0 * m.R, s));
    }
    return SG_OK;
}

int sg_iv_forward(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T_or_F, int32_t flag, const sg_dither* dither,
                  int64_t* decisions_dev, float* scores_dev, float* emb_dev, float* ivector_dev, void* stream) {
    return iv_run(ctx, "sg_iv_forward", x_dev, nullptr, B, T_or_F, flag, nullptr, dither, decisions_dev, scores_dev, emb_dev,
                  ivector_dev, nullptr, (hipStream_t)stream);
}

int sg_iv_loss(sg_ctx* ctx, const float* x_dev, const int64_t* y_dev, int32_t B, int32_t T_or_F, int32_t flag,
               const sg_loss_spec* loss, const sg_dither* dither, int64_t* decisions_dev, float* scores_dev, float* loss_dev,
               void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (!loss) return fail(ctx, SG_ERR_ARG, "sg_iv_loss: loss is NULL");
    return iv_run(ctx, "sg_iv_loss", x_dev, y_dev, B, T_or_F, flag, loss, dither, decisions_dev, scores_dev, nullptr, nullptr, loss_dev,
                  (hipStream_t)stream);
}

int sg_iv_loss_grad(sg_ctx* ctx, const float* x_dev, const int64_t* y_dev, int32_t B, int32_t T_or_F, int32_t flag,
                    const sg_loss_spec* loss, const sg_dither* dither, int64_t* decisions_dev, float* scores_dev, float* loss_dev,
                    float* grad_dev, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (!loss) return fail(ctx, SG_ERR_ARG, "sg_iv_loss_grad: loss is NULL");
    if (!grad_dev) return fail(ctx, SG_ERR_ARG, "sg_iv_loss_grad: grad is NULL");
    return iv_run(ctx, "sg_iv_loss_grad", x_dev, y_dev, B, T_or_F, flag, loss, dither, decisions_dev, scores_dev, nullptr, nullptr,
                  loss_dev, (hipStream_t)stream, grad_dev);
}

int sg_iv_extract_backward(sg_ctx* ctx, const float* zeroth_dev, const float* first_dev, const float* d_ivector_dev, int32_t B,
                           float* d_zeroth_dev, float* d_first_dev, void* stream) {
    IvDims d;
    int rc = iv_check_dims(ctx, "sg_iv_extract_backward", B, 1, SG_IV_FLAG_CMVN, &d);
    if (rc) return rc;
    if (!zeroth_dev || !first_dev || !d_ivector_dev || !d_zeroth_dev || !d_first_dev)
        return fail(ctx, SG_ERR_ARG, "sg_iv_extract_backward: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    SG_HIP(hipSetDevice(ctx->device));
    const int chunk = std::min(B, kIvChunkMax);
    if ((rc = iv_ensure_workspace(ctx, chunk, 1, false, s, true))) return rc;
    IvWorkspace& w = ctx->iv_ws;
    const IvModel& m = ctx->iv;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const size_t oc = (size_t)b0 * m.C;
        SG_HIP(launch_iv_extract(m, zeroth_dev + oc, first_dev + oc * kIvDim, nb, w.Lmat, w.linpart, w.ivec, s, w.solved));
        SG_HIP(launch_iv_extract_bwd(m, d_ivector_dev + (size_t)b0 * m.R, nb, w.Lmat, w.solved, w.lam, w.dnpart, d_zeroth_dev + oc,
                                     d_first_dev + oc * kIvDim, s));
    }
    return SG_OK;
}

int sg_iv_stats_backward(sg_ctx* ctx, const float* cmvn_dev, int32_t B, int32_t F, const float* d_zeroth_dev, const float* d_first_dev,
                         float* d_cmvn_dev, void* stream) {
    IvDims d;
    int rc = iv_check_dims(ctx, "sg_iv_stats_backward", B, F, SG_IV_FLAG_CMVN, &d);
    if (rc) return rc;
    if (!cmvn_dev || !d_zeroth_dev || !d_first_dev || !d_cmvn_dev) return fail(ctx, SG_ERR_ARG, "sg_iv_stats_backward: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    SG_HIP(hipSetDevice(ctx->device));
    if ((rc = iv_ensure_workspace(ctx, d.chunk, d.F, false, s, true))) return rc;
    IvWorkspace& w = ctx->iv_ws;
    const IvModel& m = ctx->iv;
    for (int b0 = 0; b0 < B; b0 += d.chunk) {
        const int nb = std::min(d.chunk, B - b0);
        const size_t of = (size_t)b0 * F * kIvDim, oc = (size_t)b0 * m.C;
        SG_HIP(launch_iv_stats(m, cmvn_dev + of, nb, F, w.ll, w.rowmax, w.rowsum, w.n, w.f, s));
        SG_HIP(launch_iv_stats_bwd(m, cmvn_dev + of, nb, F, w.ll, w.rowmax, w.rowsum, d_zeroth_dev + oc, d_first_dev + oc * kIvDim, w.dg,
                                   w.dxpart, d_cmvn_dev + of, s));
    }
    return SG_OK;
}

int sg_iv_delta_cmvn_backward(sg_ctx* ctx, const float* dout_dev, int32_t from_flag, int32_t B, int32_t F, float* d_delta_dev,
                              float* d_raw_dev, void* stream) {
    if (!ctx) return SG_ERR_ARG;
    if (from_flag != SG_IV_FLAG_CMVN && from_flag != SG_IV_FLAG_DELTA)
        return fail(ctx, SG_ERR_ARG, "sg_iv_delta_cmvn_backward: from_flag must be 3 (d cmvn) or 2 (d delta)");
    const bool from_cmvn = from_flag == SG_IV_FLAG_CMVN;
    if (!dout_dev || (!d_delta_dev && !d_raw_dev) || (!from_cmvn && (d_delta_dev || !d_raw_dev)))
        return fail(ctx, SG_ERR_ARG, "sg_iv_delta_cmvn_backward: NULL input, no output, or a d delta output asked of a d delta input");
    if (B < 1 || B > (1 << 20) || F < 1 || F > 65535)
        return fail(ctx, SG_ERR_ARG, "sg_iv_delta_cmvn_backward: B must be 1 .. 2^20, F 1 .. 65535");
    hipStream_t s = (hipStream_t)stream;
    SG_HIP(hipSetDevice(ctx->device));
    // as in sg_iv_delta_cmvn: the kernel reads its d delta rows back, so they need a home even when the caller wants d raw only
    IvWorkspace& w = ctx->iv_ws;
    const int chunk = std::min<int64_t>(B, std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)F * kIvDim * 4)));
    int rc = (d_delta_dev || !from_cmvn) ? SG_OK : dev_grow(ctx, w.allocs, &w.ddelta, (size_t)chunk * F * kIvDim, s);
    if (rc) return rc;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const size_t o = (size_t)b0 * F;
        float* home = !from_cmvn ? nullptr : d_delta_dev ? d_delta_dev + o * kIvDim : w.ddelta.ptr;
        SG_HIP(launch_iv_delta_cmvn_bwd(dout_dev + o * kIvDim, from_cmvn, nb, F, home, d_raw_dev ? d_raw_dev + o * kIvCep : nullptr, kIvCep, s));
    }
    return SG_OK;
}

}  // extern "C"
