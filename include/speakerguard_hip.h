/*
 * speakerguard_hip.h -- C-ABI of the MI355X (gfx950) attack hot path.
 *
 * The reference (SpeakerGuard, pure Python/PyTorch) has no native boundary of its own; this is
 * the boundary a maintainer would bind with ctypes.  Every entry point
 * names the reference interface it stands in for (file:line under /root/reference).
 *
 * Conventions
 *   - plain C, no torch types; every pointer marked "dev" is a DEVICE pointer owned by the
 *     caller (e.g. tensor.data_ptr()); pointers marked "host" are host memory.  A device pointer needs only the
 *     alignment of its element type (a row slice of a batch of odd length is fine; sg_conv1d_rows alone asks for 16
 *     bytes), and a context may be driven from any ONE stream at a time.
 *   - the library owns only the workspace inside sg_ctx (grown on demand, freed by sg_destroy).
 *   - every call returns 0 on success, non-zero on error; sg_last_error(ctx) gives the text.
 *     Nothing throws across the ABI.
 *   - one sg_ctx per device, not thread-safe.  Work is enqueued on `stream` (a hipStream_t passed
 *     as void*; NULL = the default stream) and is asynchronous unless stated otherwise.
 *   - all floating point is IEEE fp32 (f32-input MFMA); labels / decisions are int64.
 *
 * Tensor shapes use the reference's names: B utterances, T samples, F frames (snip_edges=False:
 * F = (T + 80) / 160), 30 cepstra, D = back-end dimension (rows of transform.txt), S = enrolled
 * speakers.
 */
#ifndef SPEAKERGUARD_HIP_H
#define SPEAKERGUARD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sg_ctx sg_ctx;

#define SG_OK 0
#define SG_ERR_ARG 1
#define SG_ERR_HIP 2
#define SG_ERR_STATE 3

/* ---- context ------------------------------------------------------------------------------ */
int sg_version(void);
int sg_create(int device, sg_ctx** out);
void sg_destroy(sg_ctx* ctx);
const char* sg_last_error(const sg_ctx* ctx);
/* blocks until everything enqueued on `stream` by this ctx has finished, then reports sg_health() */
int sg_sync(sg_ctx* ctx, void* stream);
/* SG_ERR_HIP if a kernel of an earlier launch raised the context's health word (a stream-K hand-off wait that timed
 * out: the contraction's output, and everything computed from it, is invalid); clears the word.  Does not
 * synchronise -- call it after the results were awaited (sg_sync does both).  Every pass entry point checks it too. */
int sg_health(sg_ctx* ctx);
/* The large contractions (TDNN layers 2-5, both directions) run as "stream-K" launches: one persistent block per compute
 * unit, a tile that is split between two blocks handed over through device memory.  A waiting block spins on its
 * predecessor, so ALL blocks of a launch must be resident at once: the context needs the GPU TO ITSELF while a pass runs
 * (no other process or context computing on the same device).  On a shared GPU a hand-off wait can time out; that is
 * reported, never silent (sg_health), and the caller's remedy is sg_set_streamk(ctx, 0): every contraction then runs as
 * one block per tile -- the same fused multiply-add chain per output, bit-identical results, a few percent slower at
 * batch 64 -- with no residency requirement.  speakerguard_amd's attack drivers do exactly that once, automatically
 * (attack/FGSM.py _run_batches), before they give up.  Default: enabled. */
int sg_set_streamk(sg_ctx* ctx, int32_t enable);
/* TEST HOOK (fault injection for the health path; no production use): the next `launches` stream-K launches of this
 * context publish no hand-off flags, so their waiting blocks time out (after a shortened bound) and raise the health word.
 * Only launches that really run a stream-K kernel count (a contraction that ends up on a tile kernel does not use the
 * budget up).  The two-unit k-means protocol below has a budget of its own, set to the same number by the same call. */
int sg_debug_lose_handoffs(sg_ctx* ctx, int32_t launches);
/* The FeCo k-means (sg_feco_kmeans*) runs an instance on TWO compute units when the batch leaves room for it (2 x instances
 * <= compute units): both blocks compute the same clustering and share only the assignment step's work through device
 * memory, every wait bounded (20 us) -- a block whose partner does not show up (GPU shared with something else) computes
 * everything itself: same bits, the one-unit speed.  mode -1: where it fits (default); 0: never.
 * (sg_debug_lose_handoffs also arms this protocol, with its own count: a paired launch it counts makes every second block
 * publish nothing.) */
int sg_feco_set_two_cu(sg_ctx* ctx, int32_t mode);
/* TEST HOOK (no production use): parks the launch counter of the two-unit k-means protocol, so that a test reaches the wrap
 * of the exchange words' 15-bit launch tag (and of the 32-bit counter itself) in a handful of launches instead of 2^15.  The
 * counter only moves the way real launches move it from there on -- the wipe of the exchange buffer at a tag wrap included. */
int sg_debug_feco_epoch(sg_ctx* ctx, uint32_t epoch);

/* How the x-vector front-end's 512-point transforms run (forward and adjoint): fft_bits 32 (default) = float32, the
 * reference's own precision (torchaudio 0.6's kaldi.mfcc is float32 end to end, model/xv_plda.py:114-148); 64 = float64
 * transforms around the same float32 stages (the form of rounds 1-5, kept as the counterpart).  Takes effect from the next
 * pass; results of the two differ by float32 round-off of the spectrum. */
int sg_xv_configure(sg_ctx* ctx, int32_t fft_bits);

/* ---- x-vector + PLDA model ----------------------------------------------------------------
 * Replaces the tensors the reference holds after model/xv_plda.py:17-47 ran: the xvecTDNN
 * state_dict (model/_xv_plda/xvecTDNN.py:16-44), emb_mean (model/utils.py:50-60), the LDA
 * matrix (model/utils.py:63-80), PLDA mean/transform/psi (model/_xv_plda/plda.py:27-49) and the
 * enrolled embeddings (model/utils.py:21-47).  All pointers are HOST fp32, PyTorch layouts.
 * The library folds the eval-mode BatchNorms (affine=False, xvecTDNN.py:17) into the following
 * layer's weights and re-lays everything out for the kernels. */
typedef struct sg_xv_weights {
    const float* tdnn_weight[5]; /* (cout, cin, k): (512,30,5) (512,512,5) (512,512,7) (512,512,1) (1500,512,1) */
    const float* tdnn_bias[5];   /* (cout) */
    const float* bn_mean[5];     /* running_mean (cout) */
    const float* bn_var[5];      /* running_var (cout)  */
    const float* fc1_weight;     /* (512, 3000) */
    const float* fc1_bias;       /* (512) */
    const float* emb_mean;       /* (512) */
    const float* lda;            /* (D, 513) last column = offset (iv_plda.py:423-435) */
    const float* plda_mean;      /* (D) */
    const float* plda_transform; /* (D, D) */
    const float* plda_psi;       /* (D) */
    const float* enroll;         /* (S, D) processed enrolment embeddings */
    int32_t D;
    int32_t S;
    float bn_eps;                /* 1e-5 */
    float threshold;             /* -INFINITY for CSI (xv_plda.py:41) */
} sg_xv_weights;

int sg_xv_load(sg_ctx* ctx, const sg_xv_weights* w);
/* replace the enrolled speakers / threshold only (model.enroll_embs, model.threshold) */
int sg_xv_set_enroll(sg_ctx* ctx, const float* enroll_host, int32_t S, float threshold);
/* The per-call `enroll_embs=` argument of forward / score / make_decision (model/iv_plda.py:155-165,172-194): score
 * the following passes against a caller-owned DEVICE table (S, D) instead of the model's enrolled set, which stays
 * untouched.  NULL ends the override.  No allocation, no synchronisation; the table must stay valid until the passes
 * enqueued while it was set have finished. */
int sg_xv_enroll_override(sg_ctx* ctx, const float* enroll_dev, int32_t S);

/* number of frames / TDNN output frames for T samples (0 if too short) */
int32_t sg_xv_num_frames(int32_t T);

/* loss selector: attack/utils.py:104-116 resolve_loss */
#define SG_LOSS_ENTROPY 0 /* SEC4SR_CrossEntropy, attack/utils.py:7-29 */
#define SG_LOSS_MARGIN 1  /* SEC4SR_MarginLoss,  attack/utils.py:31-102 */
#define SG_LOSS_LINEAR 2  /* loss[b] = sum_s coef[b][s] * score[b][s]: the vector-Jacobian product of the scores.  What
                           * autograd hands down at adaptive_attack/EOT.py:35 for ANY loss of the scores: a caller-defined
                           * loss L passes coef = dL/dscores and gets dL/dx; model/defended_model.py:67-75 ('average' order:
                           * the loss of the MEAN score of several defended branches) uses it per branch. */
#define SG_TASK_CSI 0
#define SG_TASK_SV 1
#define SG_TASK_OSI 2

typedef struct sg_loss_spec {
    int32_t loss;       /* SG_LOSS_* */
    int32_t task;       /* SG_TASK_* */
    int32_t targeted;   /* 0/1 */
    int32_t clip_max;   /* Margin: max(0, loss) (attack/utils.py:99-100) */
    float confidence;   /* Margin kappa */
    float threshold;    /* SV/OSI threshold used INSIDE the loss */
    const float* coef_dev; /* SG_LOSS_LINEAR: (B,S) device tensor, else NULL */
} sg_loss_spec;

/* Input levels, reference model/xv_plda.py:45-47 allowed_flags */
#define SG_FLAG_WAV 0  /* x: (B,1,T) waveform            */
#define SG_FLAG_RAW 1  /* x: (B,F,30) raw MFCC           */
#define SG_FLAG_CMVN 2 /* x: (B,F,30) CMVN-normalised    */

/* Dither policy for the MFCC front-end (xv_plda.py:119 hard-codes dither=1.0 from the global
 * RNG).  dither == 0 disables it.  Otherwise the noise is kaldi's sqrt(-2 ln u) cos(2 pi u) with
 * u from a counter-based generator keyed by (key, utterance, frame, sample), where for row b of the call
 *     g = row_base + b,  repeat = rep_rows > 0 ? g / rep_rows : 0,  key = seed + repeat * 0xC2B2AE3D27D4EB4F,
 *     utterance = index_base + (g - repeat * rep_rows)
 * i.e. index_base is the GLOBAL index of the first utterance (times the rows an utterance contributes to the call),
 * row_base the position of row 0 inside the full call this one is a slice of, and rep_rows > 0 says that the full
 * call's rows are EOT repeats of rep_rows rows (adaptive_attack/EOT.py:29 `x_batch.repeat(EOT_batch_size, 1, 1)`):
 * the noise an utterance sees does not depend on how a batch is chunked or sharded over GPUs.  noise_dev, when
 * non-NULL, is an explicit (B,F,400) tensor that is added instead (parity tests). */
typedef struct sg_dither {
    float dither;
    uint64_t seed;
    int64_t index_base;
    const float* noise_dev;
    int64_t row_base;
    int32_t rep_rows;
} sg_dither;

/* ---- per-stage entry points (parity tests; also what model.compute_feat etc. call) --------- */

/* model/utils.py:7-19 check_input_range(range_type='origin'): writes 32768.f or 1.f to
 * *scale_dev (device float) from the batch max/min; no host sync. */
int sg_input_scale(sg_ctx* ctx, const float* x_dev, int64_t n, float* scale_dev, void* stream);

/* model/xv_plda.py:107-156 raw() = torchaudio.compliance.kaldi.mfcc per utterance.
 * x (B,T) dev; scale_dev: device float multiplied into x (NULL = 1); feats (B,F,30) dev. */
int sg_xv_mfcc(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, const float* scale_dev,
               const sg_dither* dither, float* feats_dev, void* stream);

/* model/iv_plda.py:296-377 cmvn(): sliding 300-frame centred mean subtraction. (B,F,30)->(B,F,30) */
int sg_xv_cmvn(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, float* out_dev, void* stream);

/* Backward of the two front-end stages alone (what autograd derives for xv_plda.py:107-156 and
 * iv_plda.py:296-377): needed when something sits BETWEEN the stages, i.e. a feature-level defense
 * (model/defended_model.py:46-65 process_sequential with a flag-1 or flag-2 defense).
 * sg_xv_mfcc_backward: d loss/d raw MFCC (B,F,30) -> d loss/d waveform (B,T); same scale / dither as the forward.
 *   It needs a loaded model for its frame scratch: the x-vector model's workspace or, on a context that holds an i-vector
 *   model only (whose 24 cepstra are the first of the 30; the caller zero-pads), the i-vector workspace's.
 * sg_xv_cmvn_backward: d loss/d CMVN features -> d loss/d raw features, (B,F,30) both. */
int sg_xv_mfcc_backward(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, const float* scale_dev,
                        const sg_dither* dither, const float* dfeats_dev, float* grad_dev, void* stream);
int sg_xv_cmvn_backward(sg_ctx* ctx, const float* dout_dev, int32_t B, int32_t F, float* din_dev, void* stream);

/* Forward pass: model.make_decision / score / embedding (iv_plda.py:155-194, xv_plda.py:87-104).
 * Any output pointer may be NULL.  decisions (B) int64, scores (B,S), emb (B,D) processed
 * embedding (xv_plda.py:159-174), tdnn_emb (B,512) raw fc1 output (xvecTDNN.py:63). */
int sg_xv_forward(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T_or_F, int32_t flag,
                  const sg_dither* dither, int64_t* decisions_dev, float* scores_dev, float* emb_dev,
                  float* tdnn_emb_dev, void* stream);

/* TDNN layer activations of the LAST sg_xv_forward / sg_xv_loss_grad call (debug / parity):
 * layer 1..5 -> relu output (B, F_l, C_l) channel-last, C_5 padded to 1536; copies to out_dev. */
int sg_xv_debug_activation(sg_ctx* ctx, int32_t layer, float* out_dev, int64_t capacity_floats,
                           int32_t* rows_per_utt, int32_t* channels, void* stream);

/* The autograd call site the hand-coded backward replaces: adaptive_attack/EOT.py:32-35
 * (make_decision, loss, loss.backward(ones)).  grad has the shape of x (flag 0: (B,T); 1/2:
 * (B,F,30)); loss (B); outputs may be NULL. */
int sg_xv_loss_grad(sg_ctx* ctx, const float* x_dev, const int64_t* y_dev, int32_t B, int32_t T_or_F,
                    int32_t flag, const sg_loss_spec* loss, const sg_dither* dither,
                    int64_t* decisions_dev, float* scores_dev, float* loss_dev, float* grad_dev,
                    void* stream);

/* Backward workspace of the LAST sg_xv_loss_grad call that asked for a gradient (debug / parity): copies one buffer to
 * out_dev, laid out as that pass wrote it (its B and F, not the workspace's capacity), at most capacity_floats floats.
 *   which                    buffer                                                 dims[0..3]
 *   SG_GRAD_DEMB             d loss / d fc1 output                                  1, B, 1, 512
 *   SG_GRAD_DACT1 + l - 1    d loss / d pre-activation of tdnn l = 1..5             1, B, F_l, C_l (C_5 padded to 1536)
 *   SG_GRAD_DSTATS           the 8 split-K slabs of fc1's data gradient             8, B, 1, 3072
 *   SG_GRAD_DFEATS           the 10 split-K slabs of tdnn1's data gradient          10, B, F, 32
 *   SG_GRAD_DFEATS_RAW       d loss / d raw MFCC (a flag-0 pass only)               1, B, F, 30
 * dims (4 host int32, may be NULL) is filled whether or not out_dev is NULL.  Read only: launches nothing but the copy.
 * SG_ERR_STATE unless the context's last x-vector pass was such a call: a forward-only call, a device loop, a layer
 * timing or a rebuilt workspace since leave these buffers stale.  SG_ERR_ARG for an unknown `which`, capacity <= 0 with
 * out_dev, SG_GRAD_DFEATS_RAW after a feature-level pass. */
#define SG_GRAD_DEMB 0
#define SG_GRAD_DACT1 1
#define SG_GRAD_DSTATS 6
#define SG_GRAD_DFEATS 7
#define SG_GRAD_DFEATS_RAW 8
int sg_xv_debug_gradient(sg_ctx* ctx, int32_t which, float* out_dev, int64_t capacity_floats, int32_t* dims,
                         void* stream);

/* attack/FGSM.py:65,68: x += step*sign(grad)*grad_sign; x = min(max(x, lower), upper). In place. */
int sg_pgd_update(sg_ctx* ctx, float* x_dev, const float* grad_dev, const float* lower_dev,
                  const float* upper_dev, int64_t n, float step_size, int32_t grad_sign, void* stream);

/* attack/utils.py:7-102 on given scores (B,S): per-example loss, d loss/d scores and the decision (argmax, -1 unless
 * max > threshold) -- the tail kernels' loss stage alone.  Used where a loss is taken of scores that no single model
 * pass produced (model/defended_model.py 'average' order: mean score over the defended branches). */
int sg_loss_eval(sg_ctx* ctx, const float* scores_dev, const int64_t* y_dev, int32_t B, int32_t S, float threshold,
                 const sg_loss_spec* loss, int64_t* decisions_dev, float* loss_dev, float* dscores_dev, void* stream);

/* ---- attack-state updates around the model call (config 3: CW2, config 5: FAKEBOB/NES) -------
 * attack/CW2.py:72-82.  One pass over (B,T): if grad1 != NULL, the Adam update (torch.optim.Adam
 * defaults, step_t = 1-based step count) of `modifier` from grad1 = d loss1/d input_cur, where the full
 * objective is const[b]*loss1 + ||input_cur - x||^2 and input = tanh(modifier + atanh(0.999999 x));
 * then input_next = tanh(modifier + atanh(0.999999 x)) and loss2[b] = sum_t (input_next - x)^2.
 * Call with grad1 == NULL to produce the first input from a fresh modifier. */
int sg_cw2_step(sg_ctx* ctx, float* modifier_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                const float* x_dev, const float* input_cur_dev, const float* grad1_dev,
                const float* const_dev, int32_t B, int32_t T, float lr, int32_t step_t,
                float* input_next_dev, float* loss2_dev, void* stream);

/* adaptive_attack/NES.py:19-25: queries (n, 2*half + with_clean, T) = [x] , x + sigma z_p , x - sigma z_p.
 * z_p comes from noise_in (n, half, T) when given, else from a counter-based generator keyed by
 * (seed, example index + index_base, pair_base + p, t) -- the same noise is regenerated by
 * sg_nes_grad, so it is never stored.  noise_out (optional) receives the draws (parity tests). */
int sg_nes_queries(sg_ctx* ctx, const float* x_dev, int32_t n, int32_t T, int32_t half, int32_t with_clean,
                   float sigma, uint64_t seed, int64_t index_base, int32_t pair_base,
                   const float* noise_in_dev, float* queries_dev, float* noise_out_dev, void* stream);

/* adaptive_attack/NES.py:47,52,54: grad (n,T) (+)= mean over the 2*half noisy queries of loss * noise;
 * loss (n, 2*half + with_clean) in query order.  On the last chunk pass final_sigma = sigma (> 0) and
 * final_batches = number of chunks to apply NES.py:54's grad / sigma / num_batches. */
int sg_nes_grad(sg_ctx* ctx, const float* loss_dev, int32_t n, int32_t T, int32_t half, int32_t with_clean,
                uint64_t seed, int64_t index_base, int32_t pair_base, const float* noise_in_dev,
                int32_t accumulate, float final_sigma, int32_t final_batches, float* grad_dev, void* stream);

/* attack/FAKEBOB.py:93-104: grad <- momentum*prev + one_minus_momentum*grad (in place);
 * x <- min(max(x + grad_sign*lr[e]*sign(grad), lower), upper).  lr (n) per example. */
int sg_fakebob_step(sg_ctx* ctx, float* x_dev, float* grad_dev, const float* prev_grad_dev,
                    const float* lr_dev, const float* lower_dev, const float* upper_dev, int32_t n, int32_t T,
                    float momentum, float one_minus_momentum, int32_t grad_sign, void* stream);

/* ---- SirenAttack's particle swarm, resident on the device (attack/SirenAttack.py:40-188; k_pso.hip states the whole
 * contract).  State of a chunk of n <= 256 utterances with P <= 1024 particles, float32, each utterance in its own slot
 * for the whole chunk: loc, vel, pbest_loc (n,P,T); gbest_loc (n,T); pbest (n,P); gbest (n).  x, lower, upper: (n,T).
 * rows_host (n_active): the slots still attacked (consider_index), a HOST array like every `_host` argument: distinct, in
 * 0 .. n-1, checked before any launch.  Per-row arrays (loss, improved, report, given draws) and the queries
 * (n_active*P, T) = loc + x are dense in the order of that list.  Draws: `*_in` given -> used exactly as given; NULL ->
 * Philox4x32-10, counter (t, particle, index_base + slot), key `key` (one key per draw number, from the host); words 0 / 1
 * through ((w >> 8) + 0.5) / 2^24 give position / velocity (init) or r1 - 1e-5f / r2 - 1e-5f (move).
 *
 * sg_pso_init (:66-86), one launch.  epoch 0: pbest_loc = positions, U[lower, upper) per sample (pos_in: (n_active,P,T)),
 * pbest = +inf.  epoch > 0: particle 0 takes location and value of particle best_index_host[k] (the first-index argmin of
 * pbest, sg_pso_select's report), particles 1 .. P-1 are fresh (pos_in: (n_active,P-1,T)).  Then loc = pbest_loc,
 * vel ~ U[-|lower-upper|, |lower-upper|) (vel_in: (n_active,P,T)), and the queries. */
int sg_pso_init(sg_ctx* ctx, const float* x_dev, const float* lower_dev, const float* upper_dev, int32_t n, int32_t P,
                int32_t T, const int32_t* rows_host, int32_t n_active, int32_t epoch, const int32_t* best_index_host,
                uint64_t key, int64_t index_base, const float* pos_in_dev, const float* vel_in_dev, float* loc_dev,
                float* vel_dev, float* pbest_loc_dev, float* pbest_dev, float* queries_dev, void* stream);

/* :115-132, the scalar work, one small launch.  loss (n_active,P): pbest = loss where loss < pbest (strict), improved
 * (n_active*P bytes) = that; gbest = min pbest where it is < gbest (strict).  report (3, n_active) floats: the row's gbest
 * after the update; the first-index argmin of its new pbest; gbest_from = that argmin where gbest was updated, else -1
 * (the integers are exact in a float).  The one read the host needs per iteration (:138-161). */
int sg_pso_select(sg_ctx* ctx, const float* loss_dev, int32_t n, int32_t P, const int32_t* rows_host, int32_t n_active,
                  float* pbest_dev, float* gbest_dev, uint8_t* improved_dev, float* report_dev, void* stream);

/* :121, :131, :163-174, ONE streaming launch that touches each state element at most once.  For every row of the list (the
 * active set sg_pso_select saw): pbest_loc = loc where improved; gbest_loc = the new pbest_loc of particle
 * gbest_from_host[k] where that is >= 0.  Then, if do_move (iter < max_iter), for the rows with continue_host[k] != 0 (not
 * found: gbest >= 0), in float32 without contraction: vel = (w vel + (c1 r1)(pbest_loc - loc)) + (c2 r2)(gbest_loc - loc),
 * loc = min(max(loc + vel, lower), upper), and the next queries, dense over the continuing rows in list order (as are
 * r1_in, r2_in: (n_continue,P,T)).  queries_dev may be NULL when nothing moves. */
int sg_pso_move(sg_ctx* ctx, const float* x_dev, const float* lower_dev, const float* upper_dev, int32_t n, int32_t P,
                int32_t T, const int32_t* rows_host, int32_t n_active, const int32_t* gbest_from_host,
                const int32_t* continue_host, int32_t do_move, float w, float c1, float c2, uint64_t key,
                int64_t index_base, const float* r1_in_dev, const float* r2_in_dev, const uint8_t* improved_dev,
                float* loc_dev, float* vel_dev, float* pbest_loc_dev, float* gbest_loc_dev, float* queries_dev,
                void* stream);

/* ---- fused attack loop ----------------------------------------------------------------------
 * attack/FGSM.py:38-70 attack_batch for the xv_plda model: max_iter gradient steps plus the final
 * forward-only pass, entirely on the device (FGSM = max_iter 1, step_size epsilon). */
typedef struct sg_pgd_params {
    sg_loss_spec loss;
    float step_size;
    int32_t max_iter;
    int32_t grad_sign;       /* attack/utils.py:114 */
    int32_t eot_size;        /* EOT.py:16-54: passes per gradient step, each with fresh dither (key = dither.seed +
                              * step * 0x9E3779B97F4A7C15 + repeat * 0xC2B2AE3D27D4EB4F); their data gradients are summed
                              * in pass order before the sign step.  The repeats of a step are rows of ONE batch
                              * (eot_size x B rows, as many as fit one pass), with the bits of separate passes.
                              * With dither == 0 all repeats coincide: one pass. */
    int32_t eot_batch_size;  /* how the reference groups the repeats into model calls; must divide eot_size */
    sg_dither dither;
} sg_pgd_params;

/* x_adv (B,T) dev: in = start point, out = adversarial audio; lower/upper (B,T) dev.
 * success (B) uint8, decisions (B) int64, scores (B,S), loss (B): state at the final pass (a single forward,
 * FGSM.py:45-47).  loss_trace ((max_iter+1)*B) / decision_trace ((max_iter+1)*B): optional per-step records, as the
 * reference prints them (FGSM.py:50-58): the loss averaged over the step's EOT repeats, the decision voted over them
 * (attack/utils.py:118-125, first seen wins a tie).  A loss of kind SG_LOSS_LINEAR passes ONE (B,S) coef table; the
 * rows of the repeats of an utterance share its row. */
int sg_xv_pgd_run(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev,
                  const float* upper_dev, int32_t B, int32_t T, const sg_pgd_params* params,
                  uint8_t* success_dev, int64_t* decisions_dev, float* scores_dev, float* loss_dev,
                  float* loss_trace_dev, int64_t* decision_trace_dev, void* stream);

/* ---- batches of unequal lengths (waveform level, flag 0) ----------------------------------------
 * x (B,T_max) is a padded batch: utterance b is x[b, :lengths[b]], the rest of the row is padding whose content does not
 * matter.  Row b of every output is, bit for bit, what the uniform entry point gives for utterance b alone at its own
 * length: reflection at lengths[b], CMVN and statistics pooling over the utterance's own frames (each on the branch that
 * length takes alone), dither keyed by utterance, frame and sample.  grad (B,T_max) is 0 in the padding and the loop never
 * moves a padding sample.  Buffers keep the row strides of T_max; a pass costs what a uniform batch of T_max costs in the
 * TDNN and less in the front-end.  The range decision (x32768 or not) is taken once per batch, padding included, as the
 * uniform entry points take it.
 * lengths come twice: lengths_dev (B) int32 is what the kernels read, lengths_host (B) int32 the caller's host copy of the same
 * numbers, which is validated before any launch or allocation -- so no entry point waits for the device.  SG_ERR_ARG when
 * either is NULL, a length exceeds T_max, is shorter than one 25 ms window (400) or has too few frames for the TDNN context
 * (what the uniform entry point refuses), when no length equals T_max, or with an explicit dither tensor (noise_dev).  A
 * device copy that differs from the host copy cannot make a kernel leave its row (counts are clamped to [400, T_max]), but
 * the results are then undefined.
 * sg_xv_debug_activation / sg_xv_debug_gradient after such a pass report the padded dims (F of T_max); rows beyond an
 * utterance's own frames hold zeros in every gradient buffer and unspecified values in the activations.
 * sg_xv_pgd_run_ragged: sg_xv_pgd_run with lengths of the B utterances; the EOT repeats of a pass share them. */
int sg_xv_forward_ragged(sg_ctx* ctx, const float* x_dev, const int32_t* lengths_dev, const int32_t* lengths_host,
                         int32_t B, int32_t T_max, const sg_dither* dither, int64_t* decisions_dev, float* scores_dev,
                         float* emb_dev, float* tdnn_emb_dev, void* stream);
int sg_xv_loss_grad_ragged(sg_ctx* ctx, const float* x_dev, const int32_t* lengths_dev, const int32_t* lengths_host,
                           const int64_t* y_dev, int32_t B, int32_t T_max, const sg_loss_spec* loss,
                           const sg_dither* dither, int64_t* decisions_dev, float* scores_dev, float* loss_dev,
                           float* grad_dev, void* stream);
int sg_xv_pgd_run_ragged(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev,
                         const float* upper_dev, const int32_t* lengths_dev, const int32_t* lengths_host, int32_t B,
                         int32_t T_max, const sg_pgd_params* params, uint8_t* success_dev, int64_t* decisions_dev,
                         float* scores_dev, float* loss_dev, float* loss_trace_dev, int64_t* decision_trace_dev,
                         void* stream);

/* ---- AudioNet CSI-NE model (model/audionet_csine.py) ----------------------------------------
 * log-mel(32) front-end (model/_audionet/Preprocessor.py:85-112) -> 5x5 pre-filter -> seven
 * Conv1d/BatchNorm/ReLU(/MaxPool) blocks -> max over time -> Linear(32, num_class).  Input levels:
 * flag 0 = wav (B,1,T) in [-1,1] (int16-scaled input is divided by 32768, model/utils.py:15-16),
 * flag 1 = log-mel features (B,F,32).  All pointers in sg_an_weights are HOST fp32 tensors in the
 * reference's state_dict layout (keys convN.0.weight/bias, convN.1.weight/bias/running_mean/
 * running_var, fc.weight/bias); the BatchNorms are folded into the convolutions at load time. */
typedef struct sg_an_weights {
    const float* conv1_weight;   /* (1,1,5,5) */
    const float* conv1_bias;     /* (1) */
    const float* bn1[4];         /* conv1.1 weight, bias, running_mean, running_var (1 each) */
    const float* conv_weight[7]; /* conv2..conv8 .0.weight (cout, cin, 3) */
    const float* conv_bias[7];
    const float* bn_weight[7];
    const float* bn_bias[7];
    const float* bn_mean[7];
    const float* bn_var[7];
    const float* fc_weight;      /* (num_class, 32) */
    const float* fc_bias;        /* (num_class) */
    int32_t num_class;
    float bn_eps;                /* 1e-5 */
} sg_an_weights;

int sg_an_load(sg_ctx* ctx, const sg_an_weights* w);
/* frames of the centred STFT: 1 + (T-1)/160 (0 if T < 1024) */
int32_t sg_an_num_frames(int32_t T);
/* Preprocessor.forward: x (B,T) dev -> log-mel (B,F,32) dev (channel-last) */
int sg_an_logmel(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, float* feats_dev, void* stream);
/* backward of Preprocessor.forward alone: d loss/d log-mel (B,F,32) -> d loss/d x (B,T); used when a
 * feature-level defense sits between the front-end and the CNN (defended_model.py:46-65).
 * reuse_forward != 0: the caller states that x_dev still holds exactly the samples of this context's last sg_an_logmel /
 * waveform-level pass (same pointer, B, T -- the library checks those, it cannot check the contents); the backward then
 * starts from that pass's mel energies instead of recomputing them (126 -> 82 us at 64 x 3 s).  With 0, or when pointer
 * or shape differ, the forward is recomputed. */
int sg_an_logmel_backward(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, const float* dfeats_dev, float* grad_dev,
                          int32_t reuse_forward, void* stream);
/* How the log-mel front-end and its adjoint run on this context (defaults 32, -1, -1 = the library's choice by size):
 *   fft_bits 32 | 64: the scalar type of the STFT's transforms.  The reference computes its STFT in float32
 *     (model/_audionet/Preprocessor.py:100-105, torch.stft on a float32 signal); 64 is the form of rounds 1-4.
 *   spectrum_cache: the forward of a pass keeps every frame's packed spectrum (B x F x 4 KB) for the backward of the same
 *     pass instead of the backward transforming the frame again: 1 / 0, or -1 = decided per call from B x F (it pays
 *     everywhere except around 24-40 thousand frames).  An optional speed-up: when the buffer cannot be allocated the
 *     passes run without it.
 *   fused_overlap_add: the adjoint adds the frames' gradients up on chip (and applies the attack's update there) instead
 *     of writing B x F x 800 floats for a second kernel; same sums in the same order, same bits.  1 / 0, or -1: the
 *     library decides per call from the batch (the fused form cuts utterances into runs with 5 halo frames each and pays
 *     from ~200 utterances of 3 s; below that the separate pair is faster).
 * Takes effect from the next pass; results of the two transform precisions differ by float32 round-off. */
int sg_an_configure(sg_ctx* ctx, int32_t fft_bits, int32_t spectrum_cache, int32_t fused_overlap_add);
/* audionet_csine.make_decision / score / embedding (:149-257): decisions (B), scores (B,num_class), emb (B,32) */
int sg_an_forward(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T_or_F, int32_t flag,
                  int64_t* decisions_dev, float* scores_dev, float* emb_dev, void* stream);
/* activations of the last pass (parity): layer 1 = pre-filter output, 2..8 = conv2..conv8 block outputs
 * (after pooling where the block has one), channel-last (B, rows, C) */
int sg_an_debug_activation(sg_ctx* ctx, int32_t layer, float* out_dev, int64_t capacity_floats,
                           int32_t* rows_per_utt, int32_t* channels, void* stream);
/* adaptive_attack/EOT.py:32-35 for AudioNet: make_decision + loss + d loss/d x (hand-coded backward) */
int sg_an_loss_grad(sg_ctx* ctx, const float* x_dev, const int64_t* y_dev, int32_t B, int32_t T_or_F,
                    int32_t flag, const sg_loss_spec* loss, int64_t* decisions_dev, float* scores_dev,
                    float* loss_dev, float* grad_dev, void* stream);
/* Workspace of the LAST sg_an_loss_grad call that asked for a gradient and ran the per-layer launch sequence (debug /
 * parity): copies one buffer to out_dev, laid out as that pass wrote it (its B and frame counts, not the workspace's capacity).
 *   which                          buffer                                                            dims[0..3]
 *   SG_AN_GRAD_DACT1 + l - 1       d loss / d pre-activation of conv(l+1), l = 1..7 (conv2 .. conv8)   1, B, Tout_l, Cout_l
 *   SG_AN_GRAD_DPOOL1 / 4 / 6      d loss / d pooled output of conv2 / conv5 / conv7                   1, B, Tout_l / 2, Cout_l
 *   SG_AN_GRAD_DPRE                d loss / d pre-filter output                                        1, B, F, 32
 *   SG_AN_GRAD_PRE                 the pre-filter's forward output                                     1, B, F, 32
 *   SG_AN_GRAD_ACT1_UNPOOLED / 4 / 6   ReLU output of conv2 / conv5 / conv7 BEFORE its MaxPool (what the pooling backward reads;
 *                                  sg_an_debug_activation returns the pooled tensor)                   1, B, Tout_l, Cout_l
 * dims (4 host int32, may be NULL) is filled whether or not out_dev is NULL.  Read only: launches nothing but the copy.
 * SG_ERR_STATE unless the context's last AudioNet pass was such a call: the fused forms (the default) keep these tensors in
 * LDS, and a forward-only call, a device loop, a front-end call or a rebuilt workspace since leave the buffers stale.
 * SG_ERR_ARG for an unknown `which` and, with out_dev, a capacity below the buffer's size. */
#define SG_AN_GRAD_DACT1 0
#define SG_AN_GRAD_DPOOL1 7
#define SG_AN_GRAD_DPOOL4 8
#define SG_AN_GRAD_DPOOL6 9
#define SG_AN_GRAD_DPRE 10
#define SG_AN_GRAD_PRE 11
#define SG_AN_GRAD_ACT1_UNPOOLED 12
#define SG_AN_GRAD_ACT4_UNPOOLED 13
#define SG_AN_GRAD_ACT6_UNPOOLED 14
int sg_an_debug_gradient(sg_ctx* ctx, int32_t which, float* out_dev, int64_t capacity_floats, int32_t* dims,
                         void* stream);
/* attack/FGSM.py:38-70 attack_batch on AudioNet, whole loop on the device (params->dither ignored).
 * On a non-zero return x_adv_dev is UNSPECIFIED (the loop steps between two buffers when the overlap-add runs inside the
 * adjoint; an error in the middle leaves the caller's buffer on an earlier iterate): discard it with the error. */
int sg_an_pgd_run(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev,
                  const float* upper_dev, int32_t B, int32_t T, const sg_pgd_params* params,
                  uint8_t* success_dev, int64_t* decisions_dev, float* scores_dev, float* loss_dev,
                  float* loss_trace_dev, int64_t* decision_trace_dev, void* stream);

/* ---- measurement ---------------------------------------------------------------------------
 * Time `iters` launches of one TDNN contraction (layer 1..5 = forward, -1..-5 = data gradient) with HIP
 * events on `stream`; returns average milliseconds per launch in *ms_per_launch and the
 * algorithmic FLOPs of one launch in *flops, and the tile height (rows) the launcher picked in
 * *tile_rows.  Used by bench.py for the roofline block. */
int sg_xv_time_layer(sg_ctx* ctx, int32_t layer, int32_t B, int32_t T, int32_t iters,
                     float* ms_per_launch, double* flops, int32_t* tile_rows, void* stream);

/* Stage trace of the pass sequences (what rocprofv3 --kernel-trace shows, from inside the process).  The
 * reference has no counterpart: its only timing is a time.time() per training batch (adver_train.py:185,237); this
 * is the measurement hook SURVEY.md section 5 asks for "around the C-ABI step call".
 * Between sg_trace_begin and sg_trace_end every launch of sg_xv_forward / sg_xv_loss_grad / sg_xv_pgd_run and of
 * sg_an_forward / sg_an_loss_grad / sg_an_pgd_run / sg_an_pgd_run_feco (tags 30..) is bracketed by a pair of HIP events
 * on the launch stream, up to max_records launches (further launches are not recorded).  The per-stage entry points
 * (sg_xv_mfcc, sg_an_logmel, sg_feco_*, the attack-state updates) are not traced; sg_wav_defense_*, sg_wav_filter_* and sg_wav_resample_* are (tags 60 .. 63, 70, 71), sg_wav_stoi is (tags 72 .. 76), and so are sg_xv_pgd_run_defended and sg_an_pgd_run_defended (tags 64 .. 66 besides).  An event record that fails drops
 * its launch record, and sg_trace_end then returns SG_ERR_HIP with the count in sg_last_error.
 * sg_trace_end waits for the last recorded event, writes tag and elapsed milliseconds of each record in launch order
 * (at most `capacity`), the number of records to *n_out, and switches the trace off.  Tags: +l / -l = forward /
 * data-gradient contraction of TDNN layer l (1..5), others below.  Event records cost a few microseconds between
 * launches: trace a run of its own, not the run that is timed. */
#define SG_STAGE_MFCC_FWD 10
#define SG_STAGE_CMVN_FWD 11
#define SG_STAGE_POOL_FWD 12
#define SG_STAGE_FC1_FWD 13
#define SG_STAGE_TAIL 14
#define SG_STAGE_FC1_BWD 15
#define SG_STAGE_POOL_BWD 16
#define SG_STAGE_CMVN_BWD 17
#define SG_STAGE_MFCC_BWD 18
#define SG_STAGE_OVERLAP_ADD 19
/* AudioNet: 30 + l / 40 + l = forward / data-gradient contraction of conv block l (0..6 = conv2..conv8) */
#define SG_STAGE_AN_LOGMEL_FWD 20
#define SG_STAGE_AN_PREFILTER_FWD 21
#define SG_STAGE_AN_POOL_FWD 22
#define SG_STAGE_AN_TAIL 23
#define SG_STAGE_AN_POOL_BWD 24
#define SG_STAGE_AN_PREFILTER_BWD 25
#define SG_STAGE_AN_LOGMEL_BWD 26
#define SG_STAGE_AN_OVERLAP_ADD 27
#define SG_STAGE_AN_FECO_FWD 28
#define SG_STAGE_AN_FECO_BWD 29
#define SG_STAGE_AN_CONV_FWD 30
#define SG_STAGE_AN_CONV_BWD 40
#define SG_STAGE_AN_FUSED_FWD 50 /* the whole conv stack of a pass in one launch (round 4) */
#define SG_STAGE_AN_FUSED_BWD 51 /* (round 6: with the network's head inside, when a gradient follows) */
#define SG_STAGE_AN_FUSED_FWDBWD 52 /* forward + head + backward of whole utterances in one launch (round 6) */
/* time-domain input defenses (sg_wav_defense_forward / _backward below: traced although they are per-stage entry points,
 * because a defended attack step is the model's pass sequence plus exactly these launches) */
#define SG_STAGE_TD_FWD 60
#define SG_STAGE_TD_BWD 61
/* frequency-domain input defenses (sg_wav_filter_forward / _backward), traced for the same reason */
#define SG_STAGE_FD_FWD 62
#define SG_STAGE_FD_BWD 63
/* the defended device loops (sg_xv_pgd_run_defended, sg_an_pgd_run_defended): their stage launches carry the four tags above; their own are */
#define SG_STAGE_DEF_SCALE 64     /* scale / clip decision of a stage that is not first, and of the MFCC, from the pass's rows */
#define SG_STAGE_DEF_REPLICATE 65 /* the iterate copied once per EOT repeat of the pass */
#define SG_STAGE_DEF_REP_SUM 66   /* repeat sum of the cotangents, carried on or turned into the sign step (one launch) */
/* FeCo inside the x-vector device loop (sg_xv_pgd_run_feco): the clustering + compression launch, its backward, and the level-2
 * column copy / slab sum either side of the TDNN (the CMVN launches of that loop carry SG_STAGE_CMVN_FWD / _BWD) */
#define SG_STAGE_XV_FECO_FWD 67
#define SG_STAGE_XV_FECO_BWD 68
#define SG_STAGE_XV_FECO_COLS 69
/* the down-/up-sampling input defense (sg_wav_resample_forward / _backward), traced like the other input defenses */
#define SG_STAGE_DS_FWD 70
#define SG_STAGE_DS_BWD 71
/* the launches of sg_wav_stoi, traced so that its stages can be timed from outside */
#define SG_STAGE_STOI_SCALE 72
#define SG_STAGE_STOI_RESAMPLE 73
#define SG_STAGE_STOI_MASK 74
#define SG_STAGE_STOI_BANDS 75
#define SG_STAGE_STOI_SEGMENTS 76
int sg_trace_begin(sg_ctx* ctx, int32_t max_records);
int sg_trace_end(sg_ctx* ctx, int32_t* tags_out, float* ms_out, int32_t capacity, int32_t* n_out);

/* ---- the convolution primitive on caller buffers ------------------------------------------------
 * Dilated 1-D convolution / its data gradient on channel-last rows, the contraction behind
 * torch.nn.functional.conv1d in model/_xv_plda/xvecTDNN.py:16-33,49-53 and behind autograd's conv
 * input-gradient (adaptive_attack/EOT.py:35), exposed so the MFMA kernels can be checked in isolation:
 *
 *   C[b*Tc + t][n] = epi( sum_{j < taps} sum_{c < Kc} A[b*Ta + t + tap_base + j*tap_step][c] * W[j*Kc + c][n] )
 *
 * rows outside [0, Ta) of an utterance contribute zero.  A: (B*Ta, Kc) floats, W: (taps*Kc, N), C: (B*Tc, N);
 * Kc % 32 == 0, N % 128 == 0, so every row is a multiple of 16 bytes: a, w, c, bias and mask must be 16-byte aligned
 * (SG_ERR_ARG before any launch otherwise).  epi: 0 none, 1 relu(acc + bias[n]), 2 acc where mask[row][n] > 0 else 0
 * (mask shaped like C).  kernel: 0 = what the TDNN layers get (stream-K with 16-wave 256x128 quad-fed blocks when
 * the shape qualifies, one 16x16 block per wave on the 16x16x4 MFMA when there are at most 2800 such blocks, else one
 * quad-fed 64x128 block per tile), 1 = one b32-fed 64x128 block per tile, 2 = stream-K with the b32-fed 8-wave kernel,
 * (6 / 7 / 8 / 9 = stream-K with the roles split between waves, 128- / 64- / 32- / 256-row tiles, 10 = 128-row tiles as four
 * 64x64 computing waves; an error when the shape does not qualify),
 * 3 = stream-K with 8-wave 128x128 quad-fed blocks, 4 = one quad-fed 64x128 block per tile, 5 = one 16x16 block per
 * wave.  All choices give bit-identical results: the float32 fmaf chain restated in oracle/conv_chain.c. */
int sg_conv1d_rows(sg_ctx* ctx, const float* a_dev, const float* w_dev, float* c_dev, const float* bias_dev,
                   const float* mask_dev, int32_t B, int32_t Ta, int32_t Tc, int32_t Kc, int32_t N, int32_t taps,
                   int32_t tap_step, int32_t tap_base, int32_t epi, int32_t kernel, void* stream);

/* ---- data formats either side of the path ----------------------------
 * attackMain.py:154-166 save_audio + metric/metric.py:8-42, one pass over the batch:
 *   pcm (B,T) int16: per utterance, x * 2^15 if 0.9*max <= 1 and 0.9*min >= -1, then numpy astype(int16)
 *     (truncate toward zero, keep the low 16 bits: 1.0 -> -32768);
 *   metrics (B,5) double: L2, L0, L1, Linf of preprocess(adver) - preprocess(benign) and SNR in dB
 *     (+inf for a zero perturbation); preprocess divides by 2^15 unless -1 <= max <= 1 (metric.py:8-12).
 * pcm_dev or metrics_dev may be NULL; benign_dev is only needed for the metrics. */
int sg_wav_finalize(sg_ctx* ctx, const float* benign_dev, const float* adver_dev, int32_t B, int32_t T,
                    int16_t* pcm_dev, double* metrics_dev, void* stream);

/* STOI of B utterance pairs (reference metric/metric.py:50-54, which calls pystoi; Taal, Hendriks, Heusdens, Jensen 2011), float64
 * after the float32 samples are read.  The contract -- written from the published algorithm, unpinned by pystoi -- is DESIGN.md
 * section 4; csrc/k_stoi.hip's header states every summation order, tests/stoi_restate.py restates them in numpy.
 *   benign, adver (B,T) float32 at fs = 16000 (resampled by 5/8 with Octave's resample filter) or fs = 10000 (taken as is); each
 *   row of each signal is divided by 2^15 unless -1 <= max <= 1 (metric.py:10-14).  Frames of 256 samples at hop 128 of the benign
 *   signal more than 40 dB under its loudest frame are dropped from both signals; stoi (B) double is the mean clipped, normalised
 *   correlation of the 15 one-third-octave band envelopes over every 30-frame segment, or exactly 1e-5 for a row that keeps fewer
 *   than 31 frames (pystoi's "not enough frames" value).  frames (B) int32, optional: the frames the row kept (the value is 1e-5
 *   iff frames - 1 < 30).
 * Five launches on `stream`, no synchronisation and no host round trip between them; tables (keyed by fs) and workspace come from the
 * context: the first use of an fs uploads its tables, a call larger than any before grows the workspace (one stream
 * synchronisation), which makes the calls of ONE context on DIFFERENT streams unsafe to overlap.  A row's result depends on its own
 * samples, T and fs only: not on B, not on its place in the call.  Traced (tags 72 .. 76).
 * SG_ERR_ARG before any launch: ctx or a required pointer NULL, B outside 1 .. 65535, fs other than 10000 / 16000, T outside
 * 1 .. 2^24, a T whose length at 10 kHz (ceil(5 T / 8) for fs = 16000) is <= 256. */
/* pure, no context (parity tests): the bytes of sg_wav_stoi's device tables as the host builds them -- float64 [5][123] polyphase
 * branches (+ 1 pad), [256] window, [448] + [72] complex twiddles, the clipping factor (+ 1 pad), then int32 [16] + [16] band edges --
 * copied to `out` when it is not NULL and `capacity` bytes hold them; returns their size in bytes either way. */
int32_t sg_stoi_debug_tables(void* out, int32_t capacity);
int sg_wav_stoi(sg_ctx* ctx, const float* benign_dev, const float* adver_dev, int32_t B, int32_t T, int32_t fs,
                double* stoi_dev, int32_t* frames_dev, void* stream);

/* set_threshold.py:22-47 set_threshold(score_target, score_untarget): scans the target scores in order and
 * keeps the first one minimising |FRR - FAR| (both in percent).  out3_dev: threshold, FRR, FAR (doubles).
 * Synchronises the stream. */
int sg_eer_threshold(sg_ctx* ctx, const float* target_dev, int32_t n_target, const float* untarget_dev,
                     int32_t n_untarget, double* out3_dev, void* stream);

/* ---- FeCo feature-level defense -------------------------------------------
 * defense/feature_level.py:168-217 kmeans(): cluster the F frames of each utterance into k = int(F * ratio)
 * groups and replace every group by the mean of its frames; feats (B,F,D), D <= 64.
 * sg_feco_kmeans: cluster ids (B,F) under this library's determinism contract (k_feco.hip header; the reference
 *   delegates to a randomly initialised third-party k-means, so its ids are not reproducible).
 * sg_feco_kmeans_seeded: the same clustering started from k distinct RANDOM frames (the reference's third-party k-means
 *   starts from a random draw of numpy's global generator, kmeans_pytorch initialize(): np.random.choice(F, k,
 *   replace=False)); here the draw is a function of (seed, index_base + utterance) only -- Philox4x32-10, k_feco.hip
 *   header -- so a pass is reproducible and independent of the shard layout, and fresh seeds per pass give the
 *   randomised defense that expectation-over-transformation attacks (adaptive_attack/EOT.py) average over.
 * sg_feco_compress: :204-216 given the ids: out (B,k,D) = cluster means, an empty cluster i takes frame i (the
 *   reference's `force` fallback; with B == 1 the reference drops such rows -- the host compacts using counts).
 * sg_feco_compress_backward: the gradient autograd derives for that step.
 * sg_feco_kmeans_compress_metric: the whole forward under either distance of the reference's kmeans() (:174-182 other_param
 *   "L2" / "cos"): SG_FECO_L2 is the clustering above, SG_FECO_COS the cosine distance under a contract of its own (k_feco.hip
 *   header, "cosine").  The gradient depends on the ids only: sg_feco_compress_backward(_reps) serves both. */
int sg_feco_kmeans(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k, int32_t max_iter,
                   int32_t* assign_dev, void* stream);
int sg_feco_kmeans_seeded(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k, int32_t max_iter,
                          uint64_t seed, int64_t index_base, int32_t* assign_dev, void* stream);
int sg_feco_compress(sg_ctx* ctx, const float* feats_dev, const int32_t* assign_dev, int32_t B, int32_t F, int32_t D,
                     int32_t k, float* out_dev, int32_t* counts_dev, void* stream);
/* The whole forward of the defense in one launch: the clustering (random_init != 0: seeded form) and the cluster means
 * with the `force` fallback -- the means ARE the centroids of the clustering's last update (same ids, same ascending
 * sums), so out / counts equal sg_feco_compress of the returned ids bit for bit.
 * reps > 1 (seeded form only): the SAME features clustered reps times, repeat r from key seed + r * 0xC2B2AE3D27D4EB4F --
 * the EOT repeats of an adaptive attack (adaptive_attack/EOT.py:24-25 x_batch.repeat) without repeating the front-end;
 * assign (reps,B,F), out (reps,B,k,D), counts (reps,B,k).  sg_feco_compress_backward_reps is the matching gradient:
 * dout (reps,B,k,D) -> dfeats (B,F,D) = sum over the repeats, in repeat order (the compression is linear in the
 * features, so one front-end adjoint serves all repeats). */
int sg_feco_kmeans_compress(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k, int32_t max_iter,
                            int32_t random_init, uint64_t seed, int64_t index_base, int32_t reps, int32_t* assign_dev,
                            float* out_dev, int32_t* counts_dev, void* stream);
int sg_feco_compress_backward_reps(sg_ctx* ctx, const float* dout_dev, const int32_t* assign_dev, const int32_t* counts_dev,
                                   int32_t B, int32_t F, int32_t D, int32_t k, int32_t force, int32_t reps,
                                   float* dfeats_dev, void* stream);
/* sg_feco_kmeans_compress for EOT repeats that each have their OWN features (a dithered front-end in front of the defense):
 * feats (reps,B,F,D), row r * B + u = repeat r of utterance u.  Instance (u, r) clusters row r * B + u from key
 * seed + r * 0xC2B2AE3D27D4EB4F and utterance index_base + u -- ids, means and counts bit for bit those of a single-row
 * sg_feco_kmeans_compress(feats + (r * B + u) F D, B = 1, ..., that key, index_base + u, reps = 1) -- and writes
 * assign (reps,B,F), out (reps,B,k,D), counts (reps,B,k) at the same row.  random_init == 0: every row is clustered from the
 * even start (reps > 1 allowed: the rows differ).  The matching gradient is sg_feco_compress_backward on reps * B rows. */
int sg_feco_kmeans_compress_rows(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                 int32_t max_iter, int32_t random_init, uint64_t seed, int64_t index_base, int32_t reps,
                                 int32_t* assign_dev, float* out_dev, int32_t* counts_dev, void* stream);
int sg_feco_compress_backward(sg_ctx* ctx, const float* dout_dev, const int32_t* assign_dev, const int32_t* counts_dev,
                              int32_t B, int32_t F, int32_t D, int32_t k, int32_t force, float* dfeats_dev, void* stream);
/* The forward with the distance as an argument.  metric == SG_FECO_L2: sg_feco_kmeans_compress (row_wise 0) or
 * sg_feco_kmeans_compress_rows (row_wise 1), bit for bit, with their refusals.  metric == SG_FECO_COS: the cosine contract --
 * raw frames (no centring), unit centroids (a mean divided by sqrtf of its tree-summed squares, a zero mean stays zero: never
 * NaN), score = the fmaf chain of the L2 contract started at 0.f, largest score wins, ties to the lowest index; initial
 * frames, keys, index_base, reps and row_wise as in the L2 entries, the same shapes refused, outputs laid out alike and
 * out / counts equal to sg_feco_compress of the returned ids bit for bit.
 * SG_ERR_ARG before any launch: a metric other than the two, row_wise outside {0, 1}, whatever the L2 entries refuse.
 * The device-resident loops (sg_*_pgd_run_feco, sg_*_pgd_run_defended) cluster with L2 only. */
#define SG_FECO_L2 0
#define SG_FECO_COS 1
int sg_feco_kmeans_compress_metric(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                   int32_t max_iter, int32_t metric, int32_t random_init, uint64_t seed, int64_t index_base,
                                   int32_t reps, int32_t row_wise, int32_t* assign_dev, float* out_dev, int32_t* counts_dev,
                                   void* stream);
/* sg_feco_kmeans_compress for WIDE frames, 65 <= D <= 128 (iv_plda's delta and CMVN features, 72 columns): the entries above
 * keep refusing D > 64.  Arguments as sg_feco_kmeans_compress without `reps` (one launch per EOT repeat is the caller's):
 * assign (B,F), out (B,k,D), counts (B,k); out / counts equal sg_feco_compress of the returned ids bit for bit, and
 * sg_feco_compress / sg_feco_compress_backward(_reps), which have no width cap, serve the wide form unchanged.
 * Determinism contract "version 2, wide" (k_feco_wide.hip header): version 2 with the padded width 128 -- same centring, same
 * initial frames (even, or seeded with the Philox keys of sg_feco_kmeans_seeded), same stop rule, update and tie rule, the
 * ids of the last assignment step; n_j = the butterfly s[d] += s[d ^ 1], s[d ^ 2], ... s[d ^ 64] over 128 zero-padded lanes of
 * the rounded squares, h_j = -0.5f * n_j, score(i, j) = ONE fp32 fmaf chain from h_j over the dimensions in the contraction
 * order (groups of 8 ascending, inside a group 0, 4, 1, 5, 2, 6, 3, 7), padded with zeros to 128.
 * One 512-thread block per utterance; the frames stay in global memory, the centroid rows ((k + 31) & ~31 rows of
 * 8 ceil(D / 8) + 4 floats) and the lists must fit 150 KB of LDS: D = 72 at ratio 0.5 runs up to F = 833.
 * SG_ERR_ARG before any launch: a NULL pointer, B <= 0, D outside 65 .. 128, k outside 1 .. F, max_iter <= 0, a shape past the
 * LDS budget ("utterance too long for one block"). */
int sg_feco_kmeans_compress_wide(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k,
                                 int32_t max_iter, int32_t random_init, uint64_t seed, int64_t index_base,
                                 int32_t* assign_dev, float* out_dev, int32_t* counts_dev, void* stream);

/* FeCo with warped k-means (defense/feature_level.py:53-165 warped_kmeans / wk_compute): the F frames of each row cut into
 * k contiguous segments, the boundaries moved frame by frame while the squared error falls, out (B,k,D) = the final
 * segment means.  Determinism contract: k_feco_warped.hip header.  F <= 1200, D <= 64, 1 <= k <= F, 0 <= delta <= 1.
 * init_mode 0: TS init (:53-77); 1: random init (:80-85) -- the k - 1 frames of lowest Philox4x32-10 rank among frames
 *   1 .. F-1, keyed by (key + r * 0xC2B2AE3D27D4EB4F, index_base + u) for row r * rep_rows + u (rep_rows 0: r = 0, u = row),
 *   like sg_feco_kmeans_seeded; 2: the initial boundaries are read from `boundaries` (B,k).
 * boundaries (B,k): in for mode 2, out always (the final boundaries); init_ids (B,F) / init_counts (B,k): the INITIAL
 *   segmentation -- the reference updates its means through `.data`, so its gradient is that of the initial segment means:
 *   sg_feco_compress_backward(dout, init_ids, init_counts, force = 1); sweeps (B): sweeps made, the last one moving nothing.
 * Synchronises the stream.  SG_ERR_ARG naming the row if its initial boundaries do not rise strictly from 0 (TS of a
 * pathological input; the reference then averages empty segments: NaN) -- that row's out is zero, never NaN;
 * SG_ERR_STATE naming the row if it still moves after 4 F sweeps (the reference's loop has no cap). */
int sg_feco_warped(sg_ctx* ctx, const float* feats_dev, int32_t B, int32_t F, int32_t D, int32_t k, int32_t init_mode,
                   double delta, uint64_t key, int64_t index_base, int32_t rep_rows, int32_t* boundaries_dev,
                   int32_t* init_ids_dev, int32_t* init_counts_dev, float* out_dev, int32_t* sweeps_dev, void* stream);

/* BASELINE.json configs[3]: PGD + EOT against the FeCo-defended AudioNet as ONE device-resident loop --
 * attack/FGSM.py:38-70 attack_batch with the model of model/defended_model.py:46-65 (FeCo at feature level 1:
 * waveform -> log-mel -> FeCo -> AudioNet CNN) and the gradient chained back through the defense by hand.
 * k = int(F * cl_r) is computed by the caller (Python float arithmetic, feature_level.py:184).  random_init != 0: every
 * gradient step clusters the step's log-mel features params->eot_size times from fresh random frames (repeat r of step
 * it: key = seed + it * 0x9E3779B97F4A7C15 + r * 0xC2B2AE3D27D4EB4F, sg_feco_kmeans_compress with reps), runs the CNN on
 * the eot_size x B compressed copies as one batch, sums the repeats' feature-level gradients in repeat order
 * (sg_feco_compress_backward_reps) and takes the sum through ONE log-mel adjoint: only the defense is random, so the
 * front-end is not repeated.  random_init == 0: deterministic defense, one pass per step.  Needs B >= 2 (with one utterance the reference drops
 * empty clusters, feature_level.py:209-212: host path).  Outputs as sg_an_pgd_run. */
typedef struct sg_feco_params {
    int32_t k;
    int32_t max_iter;     /* k-means assignment steps */
    int32_t random_init;
    uint64_t seed;
    int64_t index_base;   /* global index of utterance 0 (shard offset) */
} sg_feco_params;
int sg_an_pgd_run_feco(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev,
                       const float* upper_dev, int32_t B, int32_t T, const sg_pgd_params* params,
                       const sg_feco_params* feco, uint8_t* success_dev, int64_t* decisions_dev, float* scores_dev,
                       float* loss_dev, float* loss_trace_dev, int64_t* decision_trace_dev, void* stream);

/* ---- time-domain input defenses (defense/time_domain.py) -----------------------------------------------------
 * The reference's waveform-level transforms and their gradients, x / out / g / gx all (B,T) float32 on the device, one
 * utterance per row, 1 <= B <= 65535.  Every output value is one fixed sequence of float32 operations that depends neither
 * on B nor on how a batch is cut into calls (the sequences: csrc/k_time_domain.hip header, restated in
 * tests/time_domain_restate.py).  Both calls are stream-ordered, allocate nothing and never synchronise.
 *   SG_TD_QT  :10-44 quantisation, param = q > 0: out = rint(x*s / q) * q / s, rint = round half to even, IEEE divisions.
 *             saved_dev = ONE device float s, an INPUT: sg_input_scale(x, B*T) writes it first (32768 if the whole call lies
 *             in [-1,1], else 1 -- the reference decides per call, :31, so QT alone couples the rows of a call).  BDR
 *             (:46-48) is QT with q = 2^(bits - param), computed by the caller.  Backward: the identity (BPDA, :44) -- gx_dev
 *             may alias g_dev, and then nothing is launched.
 *   SG_TD_AS  :72-97 average smoothing, param = window k (odd, 1 <= k <= 31): out[t] = sum_j w xpad[t + j - (k-1)/2],
 *             w = float32(1/k), zero padding, one fmaf chain in tap order.  saved_dev unused (NULL).  The operator is
 *             symmetric: backward = forward applied to g.
 *   SG_TD_MS  :100-127 median smoothing, param = window k (odd, 1 <= k <= 31), zero padding: out[t] = the window element of
 *             rank (k-1)/2 under the order (value, window position) -- torch.median's value; the tie rule is ours.
 *             saved_dev = (B,T) int8, written by the forward: window offset of the selected element, -(k-1)/2 .. (k-1)/2.
 *             Backward: gx[i] = sum over t ascending, |t - i| <= (k-1)/2, of g[t] [sel[t] == i - t] (what autograd does for
 *             torch.median(dim): scatter to the returned index); cotangents selected onto a pad entry are dropped.
 *   SG_TD_AT  :50-70 additive noise at param dB SNR: P[b] = sum_t (x[b,t] / sqrt(T))^2, sigma[b] = sqrt(P[b] / 10^(param/10)),
 *             out = x + n sigma[b].  n = noise_dev (B,T) when given (parity tests), else unit normals from Philox4x32-10,
 *             regenerated by the backward, never stored: key and utterance of row b derive from seed, index_base, row_base,
 *             rep_rows exactly as sg_dither documents; counter = (sample t, 0xA7000000, utterance lo, utterance hi), Box-Muller
 *             on output words 0 and 1 like sg_nes_queries.  Counter word 1 holds the frame (< 2^31 / 160) in the dither's
 *             stream and the pair index in the NES stream: the three never share a counter.
 *             saved_dev = (3,B) floats: sigma and P written by the forward, row 2 the backward's workspace.
 *             Backward (needs x_dev): gx[b,j] = g[b,j] + x[b,j] / (T 10^(param/10) sigma[b]) * sum_t g[b,t] n[b,t] -- exact
 *             autograd of the reference, whose noise power depends on x.  DEVIATION: for a silent utterance (P[b] == 0) the
 *             reference's gradient is NaN; here the second term is defined as 0, gx = g.
 * SG_ERR_ARG for anything else (even or too long windows, q <= 0, unknown kind, missing saved_dev). */
#define SG_TD_QT 0
#define SG_TD_AS 1
#define SG_TD_MS 2
#define SG_TD_AT 3
typedef struct sg_wav_defense {
    int32_t kind;       /* SG_TD_* */
    float param;        /* q | window | window | SNR in dB */
    uint64_t seed;      /* AT only, like sg_dither: */
    int64_t index_base;
    int64_t row_base;
    int32_t rep_rows;
    const float* noise_dev;
} sg_wav_defense;
int sg_wav_defense_forward(sg_ctx* ctx, const sg_wav_defense* d, const float* x_dev, int32_t B, int32_t T, float* out_dev,
                           void* saved_dev, void* stream);
/* x_dev: the forward's input (read by AT only, may be NULL otherwise) */
int sg_wav_defense_backward(sg_ctx* ctx, const sg_wav_defense* d, const float* x_dev, const float* g_dev, void* saved_dev,
                            int32_t B, int32_t T, float* gx_dev, void* stream);

/* ---- frequency-domain input defenses (defense/frequency_domain.py LPF :33-70, BPF :72-112) ----------------------
 * A Butterworth filter followed by a clamp, x / out / g / gx (B,T) float32 on the device, one utterance per row, zero initial
 * state.  The filter is handed over as the float64 second-order sections of the design (scipy's `sos` layout: S rows of
 * b0 b1 b2 a0 a1 a2, 1 <= S <= 16, a HOST pointer read during the call) and runs as that cascade in float32, as a parallel
 * scan, one launch per direction -- NOT as the reference's single direct form (b, a) in float32, whose default BPF is
 * unstable after its float32 cast (DESIGN.md "The frequency-domain defenses").  Every output value is one fixed sequence of
 * float32 operations that depends neither on B nor on how a batch is cut into calls (csrc/k_freq_domain.hip header,
 * restated in tests/freq_domain_restate.py).  Both calls are stream-ordered, allocate nothing and never synchronise; the
 * derived float32 tables travel as kernel arguments.
 *   forward   v = H x; out = clamp(v, lo, hi); mask (B,T) int8 = 1 where lo <= v <= hi, else 0 (torch's clamp gradient).
 *             SG_FD_CLIP_RANGE: the reference's per-call rule (:46-51) -- [-1, 1] when the whole call lies in the unit range,
 *             else [-2^(bits-1), 2^(bits-1) - 1] -- decided on the device from *scale_dev, the float sg_input_scale(x, B*T)
 *             wrote (32768 = unit range); SG_FD_CLIP_GIVEN: [clip_lo, clip_hi] (infinities allowed), scale_dev unused.
 *   backward  gx = H^T (g . mask), H^T the anti-causal filter flip(H flip(.)): the forward's sequence on the reversed row.
 * SG_ERR_ARG for S outside 1..16, B or T < 1, a missing pointer, a non-finite sos entry, a zero a0, a section whose poles
 * (of the float64 row or of its float32 rounding) are not strictly inside the unit circle, an unknown clip_mode. */
#define SG_FD_CLIP_RANGE 0
#define SG_FD_CLIP_GIVEN 1
typedef struct sg_wav_filter {
    int32_t n_sections;
    const double* sos;   /* host, (n_sections, 6) */
    int32_t clip_mode;   /* SG_FD_CLIP_* */
    int32_t bits;        /* SG_FD_CLIP_RANGE: the integer range's width (the reference's `bits`, 16) */
    float clip_lo;       /* SG_FD_CLIP_GIVEN */
    float clip_hi;
} sg_wav_filter;
int sg_wav_filter_forward(sg_ctx* ctx, const sg_wav_filter* f, const float* x_dev, int32_t B, int32_t T,
                          const float* scale_dev, float* out_dev, int8_t* mask_dev, void* stream);
int sg_wav_filter_backward(sg_ctx* ctx, const sg_wav_filter* f, const float* g_dev, const int8_t* mask_dev, int32_t B,
                           int32_t T, float* gx_dev, void* stream);

/* ---- the down-/up-sampling input defense (defense/frequency_domain.py DS :8-31) -----------------------------------------
 * y = Up(Down(x)), truncated to the first T samples when same_size is set; x (B,T), y / g (B,N), gx (B,T) float32 on the
 * device, one utterance per row.  N is the row length of y: T with same_size, else n_up, where n_low = ceil(T down.out_unit /
 * down.in_unit) and n_up = ceil(n_low up.out_unit / up.in_unit); the caller passes it and the call refuses another value.
 * A stage is Kaldi's LinearResample as torchaudio 0.6.0 ports it, handed over as its polyphase tables (HOST pointers, read
 * during the call): output m = u out_unit + p is the sum over j < W of weight[p * W + j] * in[first[p] + u * in_unit + j], `in`
 * zero outside its length.  The tables are the caller's (defense.frequency_domain.ds_tables builds them with float32
 * operations in torchaudio's order); the library keeps a device copy per distinct content in the context (up to 32; past that
 * the oldest leaves after one stream synchronisation).  A table is uploaded on the stream of its first call -- a call on
 * another stream must be ordered after that one.  Apart from that both calls are stream-ordered, allocate nothing after a
 * table's first use and never synchronise.  One launch per direction; the low-rate intermediate never leaves the chip.
 *   forward   every output one float32 fmaf chain from 0 in ascending tap order.
 *   backward  gx = Down^T(Up^T(g padded with zeros to n_up)) in gather form: every value one float32 fmaf chain from 0 over
 *             the outputs whose window holds it, in ascending output index.  No clamp, no mask: the exact adjoint.
 * (csrc/k_resample.hip header: the contract, zero-padded terms included; restated in tests/ds_restate.py.)
 * SG_ERR_ARG before any launch: B or T < 1 or T > 2^30, a missing pointer, same_size outside {0, 1}, N not the length above,
 * a stage with in_unit or out_unit outside 1 .. 1024, W < 1 or out_unit * W > 2048 (the TABLE BOUND: both stages' tables, the
 * backward's sorted pair lists included, then take at most 48 KB of a block's 64 KB of LDS and leave room for a tile of 2048
 * samples with its halo and intermediate; a spec whose tables and tile still do not fit is refused as well), |first[p]| >
 * 2^20, a weight that is not finite, first[0] > 0 (a window that cannot reach its own output). */
typedef struct sg_resample_stage {
    int32_t in_unit;      /* fi / gcd(fi, fo) */
    int32_t out_unit;     /* fo / gcd(fi, fo): the number of phases */
    int32_t W;            /* taps per phase */
    const int32_t* first; /* host, (out_unit) */
    const float* weight;  /* host, (out_unit, W) */
} sg_resample_stage;
typedef struct sg_wav_resample {
    sg_resample_stage down; /* fs -> int(fs * param) */
    sg_resample_stage up;   /* ... and back */
    int32_t same_size;
} sg_wav_resample;
int sg_wav_resample_forward(sg_ctx* ctx, const sg_wav_resample* r, const float* x_dev, int32_t B, int32_t T, float* out_dev,
                            int32_t N, void* stream);
int sg_wav_resample_backward(sg_ctx* ctx, const sg_wav_resample* r, const float* g_dev, int32_t B, int32_t T, int32_t N,
                             float* gx_dev, void* stream);

/* ---- the whole-utterance spectrum gate (attack/_kenan_fft.py fft_compression :57-82, the peak of :198) ---------------------
 * X = rfft(x) over each row of x (B,T) float32 on the device, T EVEN and 2 <= T <= 2^22 (the reference's own gate breaks on an
 * odd T: its irfft returns T - 1 samples); spec (B, T/2+1, 2) float32 as (re, im) pairs, peak (B) float32, factor (B) float32,
 * out (B,T) float32, keep (B, T/2+1) bytes 0 / 1, kept (B) int32, all on the device, rows contiguous.
 *   sg_wav_spectrum        spec = X and / or peak[b] = max_k |X[b,k]| (either may be NULL, not both).
 *   sg_wav_spectrum_gate   keep[b,k] = !(|X[b,k]| < factor[b]); out = irfft(X where keep, else 0), scaled by the float32 1 / T;
 *                          kept[b] = the row sum of keep.  keep_dev and kept_dev may be NULL.
 * |X| = sqrtf(re * re + im * im) in float32 without fused multiply-add, and the comparison is STRICT: a bin whose magnitude
 * equals the factor stays.  It follows from the comparison that a factor that is NaN, negative or zero keeps every bin, and that
 * a bin whose magnitude is NaN stays.  DC and Nyquist have a zero imaginary part and are gated on their real value.
 * One launch per call, one workgroup per utterance: forward transform, magnitudes, peak, gate and inverse run inside it, and a
 * row's bits depend on T alone, not on B or on the row's place in the call.  The transform is a complex Stockham network of
 * length T / 2 (radices 4, 2, 3, 5) with the real post-pass when T / 2 = 2^a 3^b 5^c, and Bluestein's convolution over a
 * power-of-two network otherwise; twiddles, chirp and transformed chirp are built on the host in float64, rounded once, and kept
 * on the device per distinct T in the context (up to 16; past that the oldest leaves after one stream synchronisation).  A table
 * is uploaded on the stream of its first call -- a call on another stream must be ordered after that one.  Lengths whose two
 * buffers do not fit a workgroup's 160 KB of LDS (a network longer than 10224 points: T = 48000) run through a workspace in the
 * context, B x 2 x network length complex values, grown (one stream synchronisation) when a call needs more than any before.
 * Apart from those two first-use cases both calls are stream-ordered, never synchronise and allocate nothing after the first
 * call at a given (B,T).  The workspace makes the calls of ONE context on DIFFERENT streams unsafe to overlap.
 * out_dev may not alias x_dev (the call refuses the same pointer; overlapping rows are the caller's to avoid): the rows are read
 * by other waves than those that write them.
 * A table costs 6 T bytes on the host and on the device for such a smooth T and up to 38 T bytes otherwise (a non-smooth T near
 * 2^22: ~90 MB each, and a float64 FFT of 2^22 points on the host at its first call); the host copy lives as long as the entry.
 * (csrc/k_spectrum.hip header: the network and its arithmetic; restated in tests/kenan_restate.py, which the GPU suite holds the
 * kernel to value for value.)
 * SG_ERR_ARG before any launch: ctx NULL, x_dev / factor_dev / out_dev NULL, both outputs of sg_wav_spectrum NULL, B < 1, T odd
 * or outside 2 .. 2^22, out_dev == x_dev. */
int sg_wav_spectrum(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, float* spec_dev, float* peak_dev, void* stream);
int sg_wav_spectrum_gate(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, const float* factor_dev, float* out_dev,
                         uint8_t* keep_dev, int32_t* kept_dev, void* stream);

/* ---- singular spectrum analysis of whole utterances (attack/_kenan.py ssa_compression :86-112, attack/ssa_core.py) -----------
 * Kenan's `ssa` variant without the trajectory matrix: W = min(int(0.05 T), 3000), t = T - W + 1; float64 (or exact integers)
 * after the quantisation; no buffer larger than W x W per utterance.  csrc/k_ssa.hip's header states every formula and every
 * summation order; tests/ssa_restate.py restates the route in numpy.
 *   sg_ssa_window      pure: W for T, or -1 when T < 20 (W would be 0) or T > 2^22.
 *   sg_ssa_decompose   x (B,T) float32 -> xq (B,T) int16: per utterance, when 0.9f * max <= 1 and 0.9f * min >= -1 (float32) the
 *                      samples are multiplied by 2^(bits-1) in float32; then int32 toward zero (NaN: 0, beyond int32: its nearest
 *                      end), low 16 bits -- a value outside the int16 range WRAPS.  The W x W lag covariance C[a][b] = sum_{p<t}
 *                      xq[p+a] xq[p+b] is formed exactly in int64 (cov (B,W,W) float64, optional: the exact values), and its
 *                      eigenpairs by a two-sided cyclic Jacobi iteration in a fixed round-robin order, closed by one Newton-Schulz
 *                      step on the accumulated rotations (V <- V (1.5 I - 0.5 V^T V)): eval (B,W) float64 in descending order,
 *                      ties by index; evec (B,W,W) float64, ROW j = eigenvector j; sweeps (B) int32 = the sweeps
 *                      that rotated (0 for a silent utterance).  A pair (p,q) is left alone when a_pq == 0 or |a_pq| <= 2^-52
 *                      sqrt(|a_pp a_qq|); an utterance is done after a sweep without a rotation.  The host reads the rotation
 *                      counters once per sweep: the call SYNCHRONISES the stream, once per sweep and once at its end.
 *                      SG_ERR_STATE when an utterance still rotates after 30 sweeps (the outputs are then undefined).
 *   sg_ssa_reconstruct xq, evec as above and k (B) int32 ON THE HOST (read before the call returns), 1 <= k[b] <= W: the rank-k[b]
 *                      reconstruction P = V_k V_k^T, diagonal averaging as one FIR filter (taps = the diagonal sums of P) away
 *                      from the first and last W - 1 samples and triangular sums there, divided by min(m+1, W, T-m); out (B,T)
 *                      float32 = the int16 value (toward zero; wraps like xq), out64 (B,T) float64 (optional) = the value before
 *                      that cast.  Stream-ordered, no synchronisation.
 * All other pointers are device pointers, rows contiguous.  The workspace comes from the context: at most B (2 W^2 + 3 W + 2) float64 for
 * sg_ssa_decompose, B (W^2 + 2 W) for sg_ssa_reconstruct, grown (one stream synchronisation) when a call needs more than any before,
 * which makes the calls of ONE context on DIFFERENT streams unsafe to overlap.  An utterance's results do not depend on B or on its
 * place in the call, and two calls give the same bits.
 * SG_ERR_ARG before any launch: ctx or a required pointer NULL, B outside 1 .. 65535, T outside 20 .. 2^22, bits outside 1 .. 16,
 * a k[b] outside 1 .. W. */
int32_t sg_ssa_window(int32_t T);
int sg_ssa_decompose(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T, int32_t bits, int16_t* xq_dev, double* eval_dev,
                     double* evec_dev, int32_t* sweeps_dev, double* cov_dev, void* stream);
int sg_ssa_reconstruct(sg_ctx* ctx, const int16_t* xq_dev, const double* evec_dev, const int32_t* k_host, int32_t B, int32_t T,
                       float* out_dev, double* out64_dev, void* stream);

/* ---- input-level defenses inside the device-resident x-vector PGD loop ---------------------------------------
 * sg_xv_pgd_run for a model that carries a chain of 1 .. SG_WAV_CHAIN_MAX waveform-level defenses (flag 0, sequential
 * order), applied in chain order to the waveform before the MFCC.  A stage is one sg_wav_defense or one sg_wav_filter,
 * exactly as the single-stage calls above take them (sg_wav_filter.sos: a HOST pointer read during the call); the stage
 * kernels and their arithmetic contracts are those calls'.  Arguments and outputs as sg_xv_pgd_run.
 *
 * Per step `it` and repeat group starting at repeat g0: chain forward on the iterate (each stage keeps its saved state and
 * its input), front-end / TDNN / tail and the backward to the DEFENDED waveform, chain backward in reverse order, then
 * x <- clamp(project(x + step * sign(sum over the repeats))).  The final pass (it == max_iter) is one forward repeat, chain
 * included.  reps = eot_size when a stage is randomised (SG_TD_AT) or dither != 0, else 1.  Every repeat is its own row
 * (row = repeat * B + utterance, G repeats per pass chosen as in sg_xv_pgd_run); the per-repeat cotangents are summed AFTER
 * the chain's backward, in repeat order ((g0 + g1) + g2) + ..., in float32, earlier groups carried through the workspace.
 * A chain of SG_TD_QT stages only (identity backward) keeps sg_xv_pgd_run's pass: the repeats share the defended rows and
 * the overlap-add sums them and takes the step.
 * Keys: a stage's AT key for a pass is seed + it * 0x9E3779B97F4A7C15 + g0 * 0xC2B2AE3D27D4EB4F (seed as handed in),
 * rep_rows = B when the pass holds more than one repeat, else 0; index_base / row_base are the caller's: the dither's
 * scheme, so noise depends on (utterance, step, repeat) only.
 * Scale decisions: the iterate's (a QT / filter stage that is first) once per call; a QT / filter stage that is not first,
 * and the MFCC, from their own input at every pass, over the rows of that pass, on the device.  DEVIATION: the reference
 * decides per model call of EOT_batch_size * B rows, the loop per pass of G * B rows; the two differ only when a preceding
 * stage pushes samples past the check_input_range bound (|x| > 1 / 0.9).
 * All buffers come from the context's workspace and are grown before the loop; inside it nothing is allocated, nothing
 * synchronises and nothing is copied to the host.
 * SG_ERR_ARG before any launch: chain NULL, n_stages outside 1 .. SG_WAV_CHAIN_MAX, an unknown tag, whatever the
 * single-stage calls refuse about a spec, a stage with noise_dev set (explicit noise is not supported in the loop). */
#define SG_WAV_CHAIN_MAX 8
#define SG_WAV_STAGE_DEFENSE 0
#define SG_WAV_STAGE_FILTER 1
typedef struct sg_wav_stage {
    int32_t tag; /* SG_WAV_STAGE_* */
    union {
        sg_wav_defense defense;
        sg_wav_filter filter;
    } u;
} sg_wav_stage;
int sg_xv_pgd_run_defended(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev,
                           const float* upper_dev, int32_t B, int32_t T, const sg_pgd_params* params,
                           const sg_wav_stage* chain, int32_t n_stages, uint8_t* success_dev, int64_t* decisions_dev,
                           float* scores_dev, float* loss_dev, float* loss_trace_dev, int64_t* decision_trace_dev,
                           void* stream);

/* The loop's repeat-summing update on caller buffers: planes (G, n) float32, total = ((carry +) p0 + p1) + ... in that
 * order (carry may be NULL).  sum_out != NULL: the total is written there (may alias carry).  x != NULL:
 * x <- min(max(x + step * grad_sign * sign(total), lower), upper), bit for bit sg_pgd_update on that total. */
int sg_wav_rep_sum_update(sg_ctx* ctx, const float* planes_dev, int32_t G, int64_t n, const float* carry_dev,
                          float* sum_out_dev, float* x_dev, const float* lower_dev, const float* upper_dev,
                          float step_size, int32_t grad_sign, void* stream);

/* ---- input-level defenses inside the device-resident AudioNet PGD loops ---------------------------------------
 * sg_xv_pgd_run_defended transposed onto sg_an_pgd_run (feco == NULL) and onto sg_an_pgd_run_feco (feco != NULL): the same
 * chain of 1 .. SG_WAV_CHAIN_MAX stages in front of the log-mel front-end, the same stage kernels, the same checks, all made
 * before the first launch.  Arguments and outputs as sg_an_pgd_run; params->dither is not read (AudioNet has no dither).
 *
 * feco == NULL.  reps = eot_size when the chain holds SG_TD_AT, else 1; G = min(reps, 65535 / B) repeats per pass, every
 * repeat its own row (row = repeat * B + utterance).  Per step `it` and group starting at repeat g0: chain forward, log-mel /
 * CNN / head on the defended rows, the adjoint to a workspace plane, chain backward last stage first, then the repeat sum
 * ((g0 + g1) + g2) + ... in float32 (sg_wav_rep_sum_update), carried to the next group or turned into the sign step.  AT's
 * key for a pass is seed + it * 0x9E3779B97F4A7C15 + g0 * 0xC2B2AE3D27D4EB4F, rep_rows = B when the pass holds more than one
 * repeat.  Per-step records: loss averaged, decision voted over the step's repeats.  The final pass is one forward repeat,
 * chain included.  A chain of SG_TD_QT stages only (identity backward) keeps sg_an_pgd_run's pass: B defended rows, and the
 * log-mel adjoint steps the iterate directly (the fused overlap-add and its waveform ping-pong where they apply).
 *
 * feco != NULL (a level-1 FeCoDefense behind the chain; B >= 2 as in sg_an_pgd_run_feco): the chain must be deterministic.
 * Per step: chain forward on B rows, log-mel, sg_feco_kmeans_compress with eot_size repeats when random_init (key
 * feco->seed + it * 0x9E3779B97F4A7C15) else one, the CNN on the repeats as one batch, sg_feco_compress_backward_reps (the
 * repeats summed at the feature level), ONE log-mel adjoint to a plane of B rows, chain backward, the sign step.
 *
 * Scale decisions: the iterate's (a QT / filter stage that is first) once per call; a later stage's and the model's range
 * decision from their own input at every pass, over the rows of that pass.
 * Nothing is allocated, synchronised or copied to the host inside the loop.
 * SG_ERR_ARG before any launch: what sg_xv_pgd_run_defended refuses about the chain, eot_size % eot_batch_size != 0, more
 * than 65535 rows per pass, feco with B < 2, feco with SG_TD_AT in the chain, feco->k outside what the AudioNet stack takes. */
int sg_an_pgd_run_defended(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev,
                           const float* upper_dev, int32_t B, int32_t T, const sg_pgd_params* params,
                           const sg_wav_stage* chain, int32_t n_stages, const sg_feco_params* feco, uint8_t* success_dev,
                           int64_t* decisions_dev, float* scores_dev, float* loss_dev, float* loss_trace_dev,
                           int64_t* decision_trace_dev, void* stream);

/* ---- FeCo inside the device-resident x-vector PGD loop -------------------------------------------------------
 * sg_xv_pgd_run against defended_model(xv_plda, [(level, FeCoDefense)]): arguments and outputs as sg_xv_pgd_run, plus the
 * FeCo block (k = int(F * ratio) computed by the caller) and the level: 1 = FeCo on the raw MFCC, before CMVN; 2 = on the
 * CMVN features.  The TDNN, tail, loss and TDNN backward run on k frames per row.  Per pass (step `it`, group starting at
 * repeat g0, pass key = it * 0x9E3779B97F4A7C15 + g0 * 0xC2B2AE3D27D4EB4F, added to the dither's and to FeCo's seed):
 *   dither != 0: reps = eot_size, every repeat a row (row = repeat * B + utterance, G per pass as in sg_xv_pgd_run).  MFCC on
 *     the G * B rows, sg_feco_kmeans_compress_rows (repeat r of the group at + r * 0xC2B2AE3D27D4EB4F), the network, back
 *     through CMVN and sg_feco_compress_backward to d loss / d raw MFCC (G * B, F, 30), then the MFCC adjoint and the
 *     overlap-add of sg_xv_pgd_run: it sums the repeats in repeat order, carries earlier groups and takes the step on the
 *     step's last group.
 *   dither == 0, random_init: only the defense is random.  MFCC once per step on B rows, sg_feco_kmeans_compress with the
 *     group's repeats, the network on them as one batch, sg_feco_compress_backward_reps (the repeats summed at the feature
 *     level in repeat order, earlier groups carried there), ONE MFCC adjoint on B rows after the step's last group.
 *   dither == 0, random_init == 0: one pass per step.
 *   The final pass (it == max_iter) is one forward repeat, FeCo included.
 * Level 1: MFCC -> FeCo -> CMVN over k frames into the padded features; back: CMVN backward from the split-K slabs ->
 * compression backward.  Level 2: MFCC -> CMVN over F frames -> FeCo -> column copy into the padded features; back: slab sum ->
 * compression backward -> CMVN backward over F frames.  Per-step records as sg_xv_pgd_run.
 * All buffers come from the context's workspace and are grown before the loop -- the two-CU exchange buffers of the k-means
 * (sg_feco_set_two_cu) included; inside it nothing is allocated, nothing synchronises and nothing is copied to the host.
 * The workspace, the group size G and the 2 GiB activation bound are all taken at F frames per row, not at the k <= F frames
 * the TDNN sees: stricter than the passes need (a batch may be refused, or cut into more groups, where k frames would fit),
 * never looser.
 * SG_ERR_ARG before any launch: feco NULL, level outside {1, 2}, B < 2 (with one utterance the reference drops empty clusters:
 * host path), k < 1 or k > F, k frames too few for the TDNN context, whatever sg_feco_kmeans_compress refuses about F, k and
 * max_iter, eot_size % eot_batch_size != 0, more than 65535 rows per pass, the 2 GiB activation bound of sg_xv_pgd_run. */
int sg_xv_pgd_run_feco(sg_ctx* ctx, float* x_adv_dev, const int64_t* y_dev, const float* lower_dev, const float* upper_dev,
                       int32_t B, int32_t T, const sg_pgd_params* params, const sg_feco_params* feco, int32_t level,
                       uint8_t* success_dev, int64_t* decisions_dev, float* scores_dev, float* loss_dev,
                       float* loss_trace_dev, int64_t* decision_trace_dev, void* stream);

/* ---- GMM / i-vector / PLDA system (reference model/iv_plda.py), both directions (csrc/k_ivector.hip, k_ivector_bwd.hip) ----
 * raw MFCC (the first 24 cepstra of sg_xv_mfcc's 30: same mel bank, lifter and energy) -> delta + delta-delta (window 3,
 * replicate edges, 72 columns) -> sliding 300-frame CMVN -> full-covariance GMM posteriors (no Gaussian pruning) ->
 * Baum-Welch statistics n (C), f (C, 72) -> i-vector w = L^-1 lin with L = I + sum_c n_c M_c^T Sigma_c^-1 M_c and
 * lin = sum_c M_c^T Sigma_c^-1 f_c (+ offset on entry 0, taken off w[0] again) -> mean subtraction, LDA, length
 * normalisation, PLDA transform and scores, decision.  sg_iv_loss_grad runs the hand-coded adjoint of that chain.
 * An utterance's result is one fixed sequence of operations: it depends neither on B, nor on the row's place in the call, nor
 * on how the library cuts a large call into chunks (the workspace holds at most 64 utterances and 256 MiB of log-likelihoods).
 * All pointers of sg_iv_weights are HOST fp32 in the reference's layouts. */
#define SG_IV_FLAG_WAV 0   /* x: (B,1,T) waveform                                  */
#define SG_IV_FLAG_RAW 1   /* x: (B,F,24) raw MFCC                                 */
#define SG_IV_FLAG_DELTA 2 /* x: (B,F,72) raw + delta + delta-delta                */
#define SG_IV_FLAG_CMVN 3  /* x: (B,F,72) CMVN-normalised                          */
typedef struct sg_iv_weights {
    int32_t C;                    /* Gaussians, 1 .. 4096                                                     */
    int32_t R;                    /* i-vector dimension, 1 .. 1024                                            */
    int32_t D;                    /* LDA / PLDA dimension, 1 .. 512                                           */
    int32_t S;                    /* enrolled speakers, 1 .. 1024                                             */
    const float* gconsts;         /* (C)          _iv_plda/gmm.py <GCONSTS>                                   */
    const float* means_invcovars; /* (C, 72)      <MEANS_INVCOVARS>                                           */
    const float* invcovars;       /* (C, 72, 72)  <INV_COVARS>, full symmetric matrices                       */
    const float* extractor;       /* (C, 72, R)   _iv_plda/ivector_extract.py <M>                             */
    const float* sigma_inv;       /* (C, 72, 72)  <SigmaInv>, full symmetric matrices                         */
    float ivector_offset;         /* <IvectorOffset>                                                          */
    const float* emb_mean;        /* (R)                                                                      */
    const float* lda;             /* (D, R + 1) last column = offset (iv_plda.py:423-435)                     */
    const float* plda_mean;       /* (D)                                                                      */
    const float* plda_transform;  /* (D, D)                                                                   */
    const float* plda_psi;        /* (D)                                                                      */
    const float* enroll;          /* (S, D) processed enrolment embeddings                                    */
    float threshold;              /* -INFINITY for CSI                                                        */
} sg_iv_weights;
/* Packs the model for the kernels (float64 on the host, rounded once): W_c = [mi_c ; -S_c,ii / 2 ; -S_c,ij (i < j)],
 * V_c = M_c^T Sigma_c^-1 and the upper triangle of U_c = V_c M_c.  SG_ERR_ARG: a NULL pointer, a size outside the bounds above,
 * a non-finite entry, or an invcovars / sigma_inv matrix that is not symmetric (|a_ij - a_ji| > 1e-6 max(|a_ij|, |a_ji|)). */
int sg_iv_load(sg_ctx* ctx, const sg_iv_weights* w);
/* as sg_xv_set_enroll / sg_xv_enroll_override, for the i-vector model's table (S, D) */
int sg_iv_set_enroll(sg_ctx* ctx, const float* enroll_host, int32_t S, float threshold);
int sg_iv_enroll_override(sg_ctx* ctx, const float* enroll_dev, int32_t S);
/* add_delta + cmvn (iv_plda.py:248-377) in one launch: raw (B, F, ld) device rows of which the first 24 columns are read
 * (ld = 30: sg_xv_mfcc's output, ld = 24: a caller's), delta_dev (B, F, 72) or NULL, cmvn_dev (B, F, 72) or NULL.
 * SG_ERR_ARG before any launch: a NULL input, both outputs NULL, B outside 1 .. 2^20, F outside 1 .. 65535, ld outside 24 .. 4096. */
int sg_iv_delta_cmvn(sg_ctx* ctx, const float* raw_dev, int32_t B, int32_t F, int32_t ld, float* delta_dev, float* cmvn_dev,
                     void* stream);
/* FullGMM.Zeroth_First_Stats (gmm.py:166-171) of CMVN features (B, F, 72): zeroth_dev (B, C), first_dev (B, C, 72). */
int sg_iv_stats(sg_ctx* ctx, const float* cmvn_dev, int32_t B, int32_t F, float* zeroth_dev, float* first_dev, void* stream);
/* ivectorExtractor.Extractivector (ivector_extract.py:98-114): (B, C), (B, C, 72) -> ivector_dev (B, R) */
int sg_iv_extract(sg_ctx* ctx, const float* zeroth_dev, const float* first_dev, int32_t B, float* ivector_dev, void* stream);
/* model.make_decision / score / embedding.  flag: SG_IV_FLAG_*; T_or_F: samples (flag 0, >= 400) or frames.  Any output may be
 * NULL: decisions (B) int64, scores (B, S), emb (B, D) processed embedding, ivector (B, R) the raw i-vector.
 * SG_ERR_STATE without a model; SG_ERR_ARG before any launch: x NULL, B outside 1 .. 2^20, a flag outside 0 .. 3, T < 400 or
 * T > 2^24, F outside 1 .. 65535. */
int sg_iv_forward(sg_ctx* ctx, const float* x_dev, int32_t B, int32_t T_or_F, int32_t flag, const sg_dither* dither,
                  int64_t* decisions_dev, float* scores_dev, float* emb_dev, float* ivector_dev, void* stream);
/* sg_iv_forward plus the per-utterance loss of `loss` (y_dev (B) int64 labels); no gradient argument: sg_iv_loss_grad. */
int sg_iv_loss(sg_ctx* ctx, const float* x_dev, const int64_t* y_dev, int32_t B, int32_t T_or_F, int32_t flag,
               const sg_loss_spec* loss, const sg_dither* dither, int64_t* decisions_dev, float* scores_dev, float* loss_dev,
               void* stream);
/* sg_iv_loss plus grad_dev = d loss_b / d x, the shape of x at every flag: (B, T), (B, F, 24), (B, F, 72), (B, F, 72).  The
 * adjoint of the tail (the length normalisation's norm a constant, as the reference's .item()), of the solve (two triangular
 * solves on the forward's Cholesky factor, float64), of the assembly (U and V^T streamed once per 16 rows), of the statistics
 * and the softmax, of the log-likelihoods (the forward's contraction transposed, on the matrix cores, folded against x without
 * writing it out), of CMVN and deltas, and at flag 0 the MFCC adjoint of sg_xv_mfcc_backward with the forward's scale and
 * dither keys.  No float atomics; every sum of an utterance runs in an order fixed by C, R and F alone: a row's gradient is
 * bit-identical whatever B, its place in the call or the chunk it falls into.  A chunk's backward runs right after its
 * forward; the gradient's buffers (a second (frames, C) buffer among them) are grown by this entry and the backward stage
 * entries only.  decisions, scores and loss are bit-equal to sg_iv_loss's.  Refusals as sg_iv_loss, and grad_dev NULL. */
int sg_iv_loss_grad(sg_ctx* ctx, const float* x_dev, const int64_t* y_dev, int32_t B, int32_t T_or_F, int32_t flag,
                    const sg_loss_spec* loss, const sg_dither* dither, int64_t* decisions_dev, float* scores_dev, float* loss_dev,
                    float* grad_dev, void* stream);
/* The backward's stages alone (parity tests), each after re-running its forward stage on the given inputs:
 * sg_iv_extract_backward: statistics (B, C), (B, C, 72) and d loss / d i-vector (B, R) -> d_zeroth (B, C), d_first (B, C, 72);
 * sg_iv_stats_backward: CMVN features (B, F, 72) and d_zeroth, d_first -> d_cmvn (B, F, 72);
 * sg_iv_delta_cmvn_backward: dout (B, F, 72) = d cmvn (from_flag 3) or d delta (from_flag 2) -> d_delta (B, F, 72) (from_flag 3
 * only; may be NULL) and d_raw (B, F, 24) (may be NULL with from_flag 3).
 * SG_ERR_STATE without a model (the first two); SG_ERR_ARG before any launch: a NULL argument, B outside 1 .. 2^20, F outside
 * 1 .. 65535, another from_flag, no output, a d_delta output with from_flag 2. */
int sg_iv_extract_backward(sg_ctx* ctx, const float* zeroth_dev, const float* first_dev, const float* d_ivector_dev, int32_t B,
                           float* d_zeroth_dev, float* d_first_dev, void* stream);
int sg_iv_stats_backward(sg_ctx* ctx, const float* cmvn_dev, int32_t B, int32_t F, const float* d_zeroth_dev, const float* d_first_dev,
                         float* d_cmvn_dev, void* stream);
int sg_iv_delta_cmvn_backward(sg_ctx* ctx, const float* dout_dev, int32_t from_flag, int32_t B, int32_t F, float* d_delta_dev,
                              float* d_raw_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPEAKERGUARD_HIP_H */
