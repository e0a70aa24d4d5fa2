/* TEST INFRASTRUCTURE ONLY (checker; never linked into or called by the product).
 *
 * Bit-exact CPU restatement of the contraction kernels' ARITHMETIC (speakerguard_amd/csrc/k_conv_gemm.hip): the dilated
 * Conv1d of the TDNN / AudioNet layers (reference model/_xv_plda/xvecTDNN.py:16-33, model/audionet_csine.py:66-118) and
 * the data gradient autograd derives for it, as ONE float32 fmaf chain per output element.
 *
 * tools/native/mfma_order.hip shows that v_mfma_f32_32x32x2_f32 and v_mfma_f32_16x16x4_f32 are sequential fused
 * multiply-adds over their k values, bit for bit.  Every kernel variant feeds the k values of a tap in the same order --
 * chunks of 32 ascending, k-groups of 8 ascending, inside a group (0, 4, 1, 5, 2, 6, 3, 7) -- taps ascending, and a tap
 * row outside its utterance enters as zeros (the MFMA is still executed: fmaf(0, w, acc)).  So the device result must
 * equal this loop bit for bit, for every launch strategy and batch size (tests/test_gpu_conv.py).
 *
 * This pins the kernels' own arithmetic contract; the agreement with the reference's conv1d (whose summation order is
 * cuDNN's / MKL's business) is checked separately in float64 (oracle/conv_rows.py, tests/test_oracle_conv.py).
 *
 *   gcc -O2 -mfma -fopenmp -ffp-contract=off -shared -fPIC oracle/conv_chain.c -o oracle/libconv_chain.so -lm
 *   (-mfma: fmaf becomes the hardware's fused multiply-add, still one rounding; -ffp-contract=off: nothing ELSE is fused)
 */
#include <math.h>
#include <stddef.h>

static const int kOrder[8] = {0, 4, 1, 5, 2, 6, 3, 7};

/* a (B*Ta, Kc), w (taps*Kc, N), out (B*Tc, N); epi 0: none, 1: max(acc + bias[n], 0), 2: mask[m][n] > 0 ? acc : 0 */
void sg_conv_chain(const float* a, const float* w, const float* bias, const float* mask, float* out, int B, int Ta, int Tc,
                   int Kc, int N, int taps, int tap_step, int tap_base, int epi) {
#pragma omp parallel for schedule(static)
    for (long bt = 0; bt < (long)B * Tc; ++bt) {
        const int b = (int)(bt / Tc), t = (int)(bt - (long)b * Tc);
        const size_t m = (size_t)bt;
        for (int n = 0; n < N; ++n) {
            float acc = 0.f;
            for (int j = 0; j < taps; ++j) {
                const int src = t + tap_base + j * tap_step;
                const float* row = (src >= 0 && src < Ta) ? a + ((size_t)b * Ta + src) * Kc : NULL;
                for (int kc = 0; kc < Kc; kc += 32)
                    for (int kg = 0; kg < 4; ++kg)
                        for (int s = 0; s < 8; ++s) {
                            const int k = kc + 8 * kg + kOrder[s];
                            acc = fmaf(row ? row[k] : 0.f, w[((size_t)j * Kc + k) * N + n], acc);
                        }
            }
            if (epi == 1) acc = fmaxf(acc + bias[n], 0.f);
            if (epi == 2) acc = mask[m * N + n] > 0.f ? acc : 0.f;
            out[m * N + n] = acc;
        }
    }
}

/* FeCo k-means assignment scores (speakerguard_amd/csrc/k_feco.hip, contract version 2): score(i, j) = h[j] + x'_i . c_j as
 * ONE fmaf chain in the k order above (Dp = 32 or 64 padded dimensions, pad entries zero).  The reference delegates the
 * clustering to a randomly initialised third-party k-means (defense/feature_level.py:185-203): this restates the
 * library's own contract, nothing of the reference.  xc (F, Dp), cc (k, Dp), h (k), out (F, k). */
void sg_feco_scores(const float* xc, const float* cc, const float* h, float* out, int F, int k, int Dp) {
#pragma omp parallel for schedule(static)
    for (int i = 0; i < F; ++i)
        for (int j = 0; j < k; ++j) {
            float acc = h[j];
            for (int g = 0; g < Dp; g += 8)
                for (int s = 0; s < 8; ++s) acc = fmaf(cc[(size_t)j * Dp + g + kOrder[s]], xc[(size_t)i * Dp + g + kOrder[s]], acc);
            out[(size_t)i * k + j] = acc;
        }
}

/* AudioNet's 5 x 5 pre-filter (speakerguard_amd/csrc/k_audionet.hip an_prefilter_kernel; reference model/audionet_csine.py
 * conv1 + BatchNorm folded by the loader) as ONE fmaf chain of 25 terms per output, started from the bias, in the kernel's
 * order: mel offset i outer, time offset j inner, weight w25[5 i + j]; a sample outside the 32 mel bands or the utterance's T
 * frames enters as zero (the fmaf is still executed).  transpose != 0: the data gradient -- the sample at (t - j + 2, m - i + 2),
 * started from 0 (the bias argument is ignored, as the kernel ignores it).  in / out (B, T, 32).
 * sg_prefilter_chain_defect is the same loop with a planted defect, for tests/test_an_stages_power.py alone (defect 1: the mel
 * edge clamped to bands 0 / 31 instead of zero-padded), so that the planted value is itself an exact fmaf chain. */
static void prefilter_chain(const float* in, int B, int T, const float* w25, float bias, int transpose, int defect, float* out) {
#pragma omp parallel for schedule(static)
    for (long bt = 0; bt < (long)B * T; ++bt) {
        const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
        const float* x = in + (size_t)b * T * 32;
        for (int m = 0; m < 32; ++m) {
            float acc = transpose ? 0.f : bias;
            for (int i = 0; i < 5; ++i)
                for (int j = 0; j < 5; ++j) {
                    const int mm = transpose ? m - i + 2 : m + i - 2, tt = transpose ? t - j + 2 : t + j - 2;
                    const int mc = mm < 0 ? 0 : (mm > 31 ? 31 : mm);
                    const int ok = (defect == 1 || mm == mc) && tt >= 0 && tt < T;
                    acc = fmaf(w25[i * 5 + j], ok ? x[(size_t)tt * 32 + mc] : 0.f, acc);
                }
            out[(size_t)bt * 32 + m] = acc;
        }
    }
}
void sg_prefilter_chain(const float* in, int B, int T, const float* w25, float bias, int transpose, float* out) {
    prefilter_chain(in, B, T, w25, bias, transpose, 0, out);
}
void sg_prefilter_chain_defect(const float* in, int B, int T, const float* w25, float bias, int transpose, int defect, float* out) {
    prefilter_chain(in, B, T, w25, bias, transpose, defect, out);
}
