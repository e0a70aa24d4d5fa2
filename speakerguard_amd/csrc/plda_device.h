// The PLDA scoring both tail kernels run (tail_kernel of k_tail.hip, iv_tail_kernel of k_ivector.hip) and its adjoint's
// per-column term, written once: plda.py:140-190.  e5: the normalised embedding (D) and c_psi: psi (D), both in LDS; enr: the
// enrolled table (S, D), in LDS or global memory.  No barrier in here: the caller places them.
#pragma once
#include "wave_reduce.h"

namespace sg {

// One wave per enrolled speaker, NT the block's thread count: sc[s] = log-likelihood ratio, dsc[s] = 0, and the same score to
// scores_out[s] (the utterance's row, or null).  Called by every thread of the block.
template <int NT>
__device__ __forceinline__ void plda_llr_scores(const float* e5, const float* c_psi, const float* enr, int D, int S, float logdet_given,
                                                float logdet_without, float* sc, float* dsc, float* scores_out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float l2pi = logf(2.f * 3.1415926f) * (float)D;  // plda.py:179 (cancels in the ratio)
    float s0 = 0.f;  // sum e5^2 / (psi + 1)
    for (int d = lane; d < D; d += 64) s0 += e5[d] * e5[d] * (1.f / (c_psi[d] + 1.f));
    s0 = wave_sum_rows(s0);
    const float without = -0.5f * (logdet_without + l2pi + s0);
    for (int s = wid; s < S; s += NT / 64) {
        float s1 = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float psi = c_psi[d];
            const float r = psi / (psi + 1.f);
            const float df = e5[d] - r * enr[(size_t)s * D + d];
            s1 += df * df * (1.f / (1.f + r));
        }
        s1 = wave_sum_rows(s1);
        if (lane == 0) {
            const float given = -0.5f * (logdet_given + l2pi + s1);
            const float v = given - without;
            sc[s] = v;
            dsc[s] = 0.f;
            if (scores_out) scores_out[s] = v;
        }
    }
}

// column d of d e5 = sum_s dsc_s (-(e5 - r enroll_s) / (1 + r) + e5 / (psi + 1)), r = psi / (psi + 1), in speaker order
__device__ __forceinline__ float plda_de5_term(const float* e5, const float* c_psi, const float* enr, const float* dsc, int D, int S,
                                               int d) {
    const float psi = c_psi[d];
    const float r = psi / (psi + 1.f);
    const float iv1 = 1.f / (1.f + r), iv0 = 1.f / (psi + 1.f);
    float g = 0.f;
    for (int s = 0; s < S; ++s) {
        const float w = dsc[s];
        if (w != 0.f) g += w * (-(e5[d] - r * enr[(size_t)s * D + d]) * iv1 + e5[d] * iv0);
    }
    return g;
}

}  // namespace sg
