// Internal declarations shared by the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/speakerguard_hip.h"

namespace sg {

// ---------------------------------------------------------------- front-end constants
// Kaldi MFCC as called at reference model/xv_plda.py:116-148.
constexpr int kShift = 160;     // frame_shift 10 ms
constexpr int kWin = 400;       // frame_length 25 ms
constexpr int kFft = 512;       // round_to_power_of_two
constexpr int kMel = 30;        // num_mel_bins
constexpr int kCep = 30;        // num_ceps
constexpr int kLdaLd = 516;     // row length of the device copy of the (D, 513) LDA matrix
constexpr int kFeatPad = 32;    // cepstra padded to the GEMM K granule
constexpr int kCmnWindow = 300; // iv_plda.py:310
constexpr float kEps = 1.1920928955078125e-07f;  // torch.finfo(float32).eps

// TDNN geometry, reference model/_xv_plda/xvecTDNN.py:16-33
constexpr int kLayers = 5;
constexpr int kCin[kLayers] = {30, 512, 512, 512, 512};
constexpr int kCout[kLayers] = {512, 512, 512, 512, 1500};
constexpr int kCinPad[kLayers] = {32, 512, 512, 512, 512};
constexpr int kCoutPad[kLayers] = {512, 512, 512, 512, 1536};
constexpr int kTaps[kLayers] = {5, 5, 7, 1, 1};
constexpr int kDil[kLayers] = {1, 2, 3, 1, 1};
constexpr int kEmb = 512;
constexpr int kPoolC = 1536;           // padded tdnn5 channels
constexpr int kStats = 2 * kPoolC;     // [mean | std], padded
constexpr int kFc1SplitK = 48;         // fc1 forward split-K (3072 / 64: two chunks per block)
constexpr int kFc1BwdSplitK = 8;          // (512 / 64: two chunks per block)
constexpr int kL1BwdSplitK = 10;       // tdnn1 data gradient: two K-slabs per tap (N = 32 gives only 19 tiles per 8 utterances: with one
                                       // slab per tap 95 blocks for 256 CUs, 19 -> 11 us at 8 utterances, 29 -> 24 at 32, same at 64).  A
                                       // constant of the arithmetic: the slabs are summed in order, whatever the batch

constexpr int num_frames(int T) { return (T + kShift / 2) / kShift; }
constexpr int kTdnnContext = 30;  // frames tdnn1 .. tdnn3 take off an utterance: (5 - 1) 1 + (5 - 1) 2 + (7 - 1) 3 (tdnn4 / tdnn5: none)

// A batch of unequal lengths (sg_xv_*_ragged): the device array of per-utterance sample counts.  Every buffer keeps the row
// stride of the longest utterance (T, F, F5 of the call); row r of a pass is utterance r % n, so EOT repeats wrap.  dev == null:
// a uniform batch, the kernels of old.
struct RowLens {
    const int32_t* dev = nullptr;  // (n) int32
    int n = 0;
};
// samples of row `row`, held inside what the buffers and the front-end can take whatever the array says (the entry points
// validate a host copy before the first launch; a kernel still never derives an address from an unchecked count)
__device__ __forceinline__ int row_samples(const int32_t* lens, int n, int row, int T) {
    const int t = lens[row % n];
    return t > T ? T : (t < kWin ? kWin : t);
}

// a device buffer that is grown on demand (dev_grow): the pointer and the elements it has room for; reads as the pointer
template <typename T>
struct DevBuf {
    T* ptr = nullptr;
    size_t cap = 0;
    operator T*() const { return ptr; }
};

// ---------------------------------------------------------------- the FFT-512's twiddle tables (fft512.h)
// The one place that knows their layout: tw1[(j - 1) * 64 + lane] = W512^(j lane), j = 1 .. 7, and tw2[9 b + c] = W64^(b c) =
// W512^(8 b c), b, c < 8, the pad entry (c = 8) zero; (re, im) pairs of T, forward sign.  w512(m) is the CALLER's float64
// W512^m (a double2, m < 512) -- from a half-circle table or from cos / sin, which can differ in the last bit -- rounded once to T.
constexpr int kFftTw1 = 7 * 64, kFftTw2 = 72;
template <typename T, typename W>
inline void fft512_twiddle_tables(W w512, T* tw1, T* tw2) {
    auto put = [&](int m, T* out) {
        const double2 w = w512(m);
        out[0] = (T)w.x;
        out[1] = (T)w.y;
    };
    for (int i = 0; i < kFftTw1; ++i) put((i / 64 + 1) * (i % 64), tw1 + 2 * i);
    for (int i = 0; i < kFftTw2; ++i) {
        const int b = i / 9, c = i - 9 * b;
        if (c < 8) put(8 * b * c, tw2 + 2 * i);
        else tw2[2 * i] = tw2[2 * i + 1] = (T)0;
    }
}

// ---------------------------------------------------------------- AudioNet CSI-NE (model/audionet_csine.py)
constexpr int kAnFft = 1024, kAnHop = 160, kAnWin = 800, kAnMel = 32, kAnBins = 513;  // Preprocessor.py:13-23
constexpr int kAnConv = 7;                                                              // conv2 .. conv8
constexpr int kAnCin[kAnConv] = {32, 64, 128, 128, 128, 128, 64};
constexpr int kAnCout[kAnConv] = {64, 128, 128, 128, 128, 64, 32};
constexpr int kAnPad[kAnConv] = {1, 1, 1, 1, 1, 1, 0};
constexpr bool kAnPool[kAnConv] = {true, false, false, true, false, true, false};
// torch.stft(center=True) on the pre-emphasised signal of T-1 samples: 1 + (T-1)/hop frames
inline int an_num_frames(int T) { return T < kAnWin ? 0 : 1 + (T - 1) / kAnHop; }
// frames entering / leaving every conv; false if the utterance is too short for conv8 (kernel 3, no pad)
inline bool an_layer_frames(int F, int* Tin, int* Tout) {
    int t = F;
    for (int l = 0; l < kAnConv; ++l) {
        Tin[l] = t;
        Tout[l] = t + 2 * kAnPad[l] - 2;
        if (Tout[l] < 1) return false;
        t = kAnPool[l] ? Tout[l] / 2 : Tout[l];
        if (t < 1) return false;
    }
    return Tin[kAnConv - 1] >= 3;
}

struct AnTables {            // device pointers
    float* window;           // [800] periodic hann
    float* mel_w;            // [32][513] slaney mel filterbank
    int* mel_lo;             // [32]
    int* mel_hi;             // [32]
    int* bin_m0;             // [513]
    float* bin_w0;           // [513]
    float* bin_w1;           // [513]
    double2* twiddle;        // [512] exp(-2 pi i k / 1024)
    uint16_t* bitrev;        // [1024]
    float* mel_cache;        // [B*F][32] forward -> backward hand-over within one pass (null: the backward recomputes)
    float2* spec_cache;      // [B*F][512] packed spectrum Z of every frame, same hand-over (null: the backward transforms again)
    // what a block's waves read lane by lane (k_audionet.hip AnLaneTab), laid out by the host: a block copies them to LDS
    float* lane_win;         // [16][64] window tap of FFT input 2 (lane + 64 i) + {0, 1} (0 outside the 800-tap window)
    float* lane_melw;        // [20][64] weights of the lane's run of a mel filter's bins, ascending, zero-padded
    int* lane_k0;            // [64] first bin of the lane's run
    int* mel_seg;            // [32] filter m: first lane | number of runs << 8 (an_build_tables)
    // the 512-point transform's twiddle tables as its lanes read them (fft512.h: tw1[(j - 1) * 64 + lane] = W512^(j lane),
    // tw2[9 b + c] = W64^(b c)), float64 values and the same rounded once to float32
    double2* tw1d;           // [448]
    double2* tw2d;           // [72]
    float2* tw1f;
    float2* tw2f;
};
// how the AudioNet front-end runs (sg_an_configure)
struct AnFrontCfg {
    // defaults: float32 transforms (the reference's precision); cache and overlap-add chosen by size, each where it measured
    // faster (profiles/r06_an_frontend_ab.txt; an_use_spec_cache, an_ola_pays)
    int fft32 = 1;       // transforms in float32 (the reference's precision) or float64
    int spec_cache = -1;  // the forward keeps every frame's packed spectrum for the backward of the same pass: 1 / 0, -1 = by size
    int ola = -1;        // overlap-add (+ update) inside the log-mel adjoint: 1 / 0, -1 = where it pays (an_ola_pays: large batches)
};
struct AnOlaArgs {
    const float* x;        // (B, T) waveform the frames are re-transformed from (spectrum cache: unused)
    const float* dfeats;   // (B, F, 32)
    float* dframes;        // (B, F, 800): only the edge frames are written (f < edge_lo or f >= edge_hi)
    float* grad_out;       // (B, T) or null
    const float* x_in;     // update: x_out = clamp(x_in + step * sign(g) * grad_sign); null: no update
    float* x_out;
    const float* lower;
    const float* upper;
    const float* scale_p;
    float step;
    int grad_sign;
    int B, T, F, S;        // S slices per utterance (chosen by the launcher)
    int edge_lo, edge_hi;  // frames the edge kernel needs (launcher)
    int t_lo, t_hi;        // d x[t] for t in [t_lo, t_hi] comes from the fused kernel, the rest from the edge kernel (launcher)
};

struct AnModel {
    bool loaded = false;
    int S = 0;
    float* w25 = nullptr;       // folded 5x5 pre-filter [mel offset][time offset]
    float pre_bias = 0.f;
    float* wf[kAnConv] = {};    // forward  [3*Cin][Cout]   (BatchNorm folded)
    float* wb[kAnConv] = {};    // backward [3*Cout][Cin]
    float* wfq[kAnConv] = {};   // k4-packed copies for the quad-fed tile kernel (layers whose N is a multiple of 128)
    float* wbq[kAnConv] = {};
    float* bias[kAnConv] = {};
    float* fc_w = nullptr;      // [S][32]
    float* fc_b = nullptr;      // [S]
};

struct AnWorkspace {
    int B = 0, T = 0, F = 0;
    // frames entering / leaving each conv (before pooling) of the LAST pass (an_net_step writes them): what
    // sg_an_debug_activation reports.  No decision reads them.
    int Tin[kAnConv] = {}, Tout[kAnConv] = {};
    // B and F of the sg_an_loss_grad call whose per-layer forward and backward buffers are still in place
    // (sg_an_debug_gradient); grad_B == 0: none -- cleared by every later pass (an_check) and with the workspace itself
    int grad_B = 0, grad_F = 0;
    float* scale = nullptr;
    float* feats = nullptr;    // (B, F, 32) log-mel
    float* pre = nullptr;      // (B, F, 32) pre-filter output
    float* act[kAnConv] = {};  // ReLU outputs (B, Tout, Cout)
    float* pool[kAnConv] = {}; // pooled outputs where the layer has a MaxPool
    float* dact[kAnConv] = {}; // gradients wrt pre-activations
    float* dpool[kAnConv] = {};
    float* dpre = nullptr;     // (B, F, 32)
    float* dfeats = nullptr;   // (B, F, 32)
    float* dframes = nullptr;  // (B, F, 800)
    // FeCo inside the fused loop (sg_an_pgd_run_feco): cluster ids / sizes, compressed features and their gradient
    int* feco_ids = nullptr;     // (B, F)
    int* feco_cnt = nullptr;     // (B, F) (k <= F used)
    float* feco_out = nullptr;   // (B, k, 32)
    float* dfeco = nullptr;      // (B, k, 32)
    int64_t* y_rep = nullptr;    // (B) labels repeated for the EOT repeats batched into one pass
    float* trace_l = nullptr;    // (B * R) per-row loss / decision records of such a pass (reduced over the repeats afterwards)
    int64_t* trace_d = nullptr;
    float* mel_cache = nullptr;  // (B, F, 32) mel energies of the forward pass, kept for the backward of the same pass
    float2* spec_cache = nullptr;  // (B, F, 512) packed spectra of the forward pass (allocated on first use, grown on demand)
    size_t spec_cache_bytes = 0;
    bool spec_cache_refused = false;  // an allocation failed once: the passes run without the cache
    DevBuf<float> x_alt;         // (B, T) the other half of the waveform ping-pong of the fused overlap-add update (on demand)
    // the defended loop (sg_an_pgd_run_defended) when a step's EOT repeats run as several passes: the cotangent sum carried
    // from group to group, and the per-repeat records the last group reduces (both on demand, before the loop)
    DevBuf<float> grad_carry;        // (n) floats, n = utterances x T of the call
    DevBuf<float> eot_loss_rows;     // (reps * utterances)
    DevBuf<int64_t> eot_dec_rows;
    // which input the mel cache belongs to (sg_an_logmel_backward(reuse_forward) checks pointer and shape, not contents)
    const float* cache_x = nullptr;
    int cache_B = 0, cache_T = 0;
    bool cache_spec = false;     // the spectrum cache holds that input's spectra too
    std::vector<void*> allocs;
};

// The MFCC kernels' constant tables exactly as they sit in a block's LDS (k_mfcc.hip), built once on the host per transform
// precision R and copied into LDS with 16-byte loads by every block (round 6; rounds 1-5 derived them per block from the raw
// tables -- dependent global look-ups in front of the first frame).
constexpr int kMfccTw1 = kFftTw1, kMfccTw2 = kFftTw2;
constexpr int kMelLaneBins = 24;  // >= bins per half mel filter (21 for 30 filters, 20-7600 Hz, 512-point FFT; host-checked)
template <typename R>
struct MfccLdsImage {
    R tw1[2 * kMfccTw1];                // (re, im) of W512^(j lane) at (j - 1) * 64 + lane, float64 values rounded once to R
    R tw2[2 * kMfccTw2];                // W64^(b c) at 9 b + c
    float window[kFft];                 // povey window, zero beyond sample 399
    float dct[kMel * kCep + 64];        // [m][c] (forward: lane c reads dct[m][c])
    float dct_t[kCep * 32];             // [c][m] (backward: lane m reads dct[m][c])
    float lifter[32];
    float melw_lane[kMelLaneBins * 64]; // [j][lane]: weight of bin mel_k0[lane] + j in the half filter of lane (0 beyond it)
    int mel_k0[64];                     // first bin of lane's half filter (two lanes per filter)
};
static_assert(sizeof(MfccLdsImage<float>) % 16 == 0 && sizeof(MfccLdsImage<double>) % 16 == 0, "copied as 16-byte words");

struct MfccTables {          // device pointers
    const MfccLdsImage<float>* lds_f32;
    const MfccLdsImage<double>* lds_f64;
    int* bin_m0;             // [256] lower mel index touching this bin (-1: none)   (the adjoint's per-bin mel membership)
    float* bin_w0;           // [256] weight into mel bin_m0
    float* bin_w1;           // [256] weight into mel bin_m0+1 (0 if none)
    int fft64;               // sg_xv_configure: 0 = float32 transforms (default, the reference's precision), 1 = float64
    // spectrum hand-over forward -> backward within one pass (null: the backward recomputes the forward):
    // bins 0..255 of every frame's FFT as float2, in the transform's register order (bin (l >> 3) + 8 (l & 7) + 64 d at
    // element 64 d + l), and the 30 mel energies
    float2* spec_cache;      // [B*F][256]
    float* mel_cache;        // [B*F][32]
    int rep_utts;            // > 0: rows are EOT repeats of rep_utts utterances (row = repeat * rep_utts + utterance):
                             // repeats share the waveform row, repeat r draws its dither from key seed + r * 0xC2B2AE3D27D4EB4F
};

// The PLDA back end both speaker models score with (plda_backend.hip; the kernels' side: plda_device.h).  The transform
// matrices stay with their model: their layouts differ.
struct PldaBackend {
    int D = 0, S = 0;
    float threshold = 0.f;
    float logdet_given = 0.f, logdet_without = 0.f;  // sum log(1 + psi/(psi+1)), sum log(psi+1)
    float* plda_mean = nullptr; // [D]
    float* plda_psi = nullptr;  // [D]
    float* enroll = nullptr;    // [S][D]
    int enroll_cap = 0;         // speakers the enroll buffer holds (plda_backend_set_enroll reuses it)
    // per-call override of the enrolled set (iv_plda.py:155-165 enroll_embs=): a caller-owned device table that the
    // next passes score against; the model's own set is untouched
    const float* enroll_override = nullptr;
    int S_override = 0;
};

struct XvModel {
    bool loaded = false;
    PldaBackend be;
    // folded TDNN weights, GEMM layouts
    float* wf[kLayers] = {};    // forward  [taps*CinPad][CoutPad]
    float* wb[kLayers] = {};    // backward [taps*CoutPad][CinPad]
    float* wfq[kLayers] = {};   // wf packed k4-major [taps*CinPad/4][CoutPad][4] (quad-fed GEMM)
    float* wbq[kLayers] = {};   // wb packed k4-major
    float* bias[kLayers] = {};  // [CoutPad] folded
    float* fc1_w = nullptr;     // [kStats][512] folded (K-major)
    float* fc1_wt = nullptr;    // [512][kStats] folded (for the backward GEMM)
    float* fc1_b = nullptr;     // [512] folded
    float* emb_mean = nullptr;  // [512]
    int Dp = 0;                 // D rounded up to a multiple of 4 (row stride of the transposed / PLDA matrices below)
    float* lda = nullptr;       // [D][kLdaLd]: the (D, 513) LDA matrix, rows padded to 516 floats (16-byte aligned rows)
    float* lda_t = nullptr;     // [513][Dp], zero-padded columns
    float* plda_p = nullptr;    // [D][Dp], zero-padded columns
    float* plda_pt = nullptr;   // [D][Dp] transposed, zero-padded columns
    float* pa = nullptr;        // [D][kLdaLd]: (P A)[d][i], i < 512 -- the backward's P^T and LDA^T as one product (float64 product, rounded once)
    std::vector<void*> allocs;  // device memory owned by this model (freed on reload / destroy)
};

struct Workspace {
    int B = 0, T = 0, F = 0;          // capacity the buffers were sized for
    int Fl[kLayers] = {};              // TDNN output frames per layer
    // B, F and flag of the sg_xv_loss_grad backward whose buffers are still in place (sg_xv_debug_gradient); grad_B == 0:
    // none -- cleared by every later pass (check_dims), by a layer timing and with the workspace itself
    int grad_B = 0, grad_F = 0, grad_flag = -1;
    float* scale = nullptr;            // [1]
    float* feats_raw = nullptr;        // [B][F][30]
    float* feats = nullptr;            // [B][F][32] CMVN output, zero padded
    float* act[kLayers] = {};          // relu outputs [B][Fl][CoutPad]
    float* dact[kLayers] = {};         // d loss / d pre-activation [B][Fl][CoutPad]
    float* dfeats = nullptr;           // [kL1BwdSplitK][B][F][32] split-K slabs of the tdnn1 data gradient
    float* dfeats_raw = nullptr;       // [B][F][30]
    float* dframes = nullptr;          // [B][F][400]
    float2* spec_cache = nullptr;      // [B][F][256] forward spectrum kept for the backward (39 MB at B = 64)
    float* mel_cache = nullptr;        // [B][F][32]
    float* stats = nullptr;            // [B][kStats]
    float* fc1_part = nullptr;         // [kFc1SplitK][B][512]
    float* demb = nullptr;             // [B][512]
    float* dstats_part = nullptr;      // [kFc1BwdSplitK][B][kStats]
    float* tdnn_emb = nullptr;         // [B][512]
    float* emb = nullptr;              // [B][D]
    float* scores = nullptr;           // [B][S]
    float* loss = nullptr;             // [B]
    int64_t* decisions = nullptr;      // [B]
    float* grad = nullptr;             // [B][T]
    int64_t* y_rep = nullptr;          // [B] labels repeated for EOT repeats batched into one pass
    DevBuf<float> eot_loss_rows;       // [reps * B] per-repeat records of a step whose repeats run as several passes
    DevBuf<int64_t> eot_dec_rows;
    // FeCo inside the loop (sg_xv_pgd_run_feco), grown before the loop: cluster ids (rows, F) / sizes (rows, k), the compressed
    // features and their cotangent (rows, k, 30), and -- level 2 -- the dense CMVN features and their cotangent (rows, F, 30)
    DevBuf<int> feco_ids, feco_cnt;
    DevBuf<float> feco_out, dfeco, feco_cm, dfeco_cm;
    std::vector<void*> allocs;
};

// Buffers of the defended device loops (sg_xv_pgd_run_defended, sg_an_pgd_run_defended), grown before the loop, never inside it.  `plane` = one
// (rows, T) float32 waveform of the largest pass, rows = G * B when every EOT repeat runs as its own row.
struct DefWorkspace {
    size_t plane = 0;                  // floats per plane the buffers were sized for
    int rows = 0;                      // rows the AT statistics were sized for
    int n_out = 0, n_saved = 0;        // stage outputs / int8 planes held
    bool rep = false;                  // x_rep and the two cotangent planes are held
    float* out[SG_WAV_CHAIN_MAX] = {};   // stage outputs (the next stage's input; AT's backward reads its input here)
    int8_t* saved[SG_WAV_CHAIN_MAX] = {};  // MS's `sel` / a filter's clamp mask, handed out in chain order
    float* stats = nullptr;            // [SG_WAV_CHAIN_MAX][3][rows] AT's sigma, power, backward workspace
    float* scales = nullptr;           // [SG_WAV_CHAIN_MAX] the scale / clip decision of a QT / BDR / filter stage
    float* x_rep = nullptr;            // the iterate, once per repeat of the pass
    float* g[2] = {};                  // cotangent planes of the chain's backward (ping-pong)
    std::vector<void*> allocs;
};

// Tables on the device, found by key, else built by the caller and uploaded (dev_tables_insert).  An entry keeps the host
// bytes beside their device copy for as long as that lives: the upload is asynchronous, from pageable memory.  What a user
// keeps beside them -- geometry, a plan -- it adds by deriving from DevTable.
struct DevTable {
    std::vector<int32_t> key;
    std::vector<unsigned char> blob;  // what the device copy holds
    void* dev = nullptr;
    virtual ~DevTable() {
        if (dev) (void)hipFree(dev);
    }
};
struct DevTableCache {
    std::vector<DevTable*> entries;  // oldest first; a hit does not move an entry
    DevTable* find(const std::vector<int32_t>& key) const {
        for (DevTable* e : entries)
            if (e->key == key) return e;
        return nullptr;
    }
    void clear() {
        for (DevTable* e : entries) delete e;
        entries.clear();
    }
};

// ---------------------------------------------------------------- GMM / i-vector / PLDA system (k_ivector.hip, sg_api_ivector.hip)
constexpr int kIvCep = 24;                        // cepstra read from a raw row (iv_plda.py:230)
constexpr int kIvDim = 72;                        // raw + delta + delta-delta
constexpr int kIvK = kIvDim + kIvDim * (kIvDim + 1) / 2;  // 2700: z = [x ; x_i x_j (i <= j)]
constexpr int kIvMaxC = 4096, kIvMaxR = 1024, kIvMaxD = 512;
constexpr int kIvLinSlice = 16;                   // components per partial sum of lin (a constant of the arithmetic): 64 left the
                                                  // launch at 256 blocks of one long dependent chain each, 2.7 ms at C 2048, R 400, B 64
constexpr int kIvChunkMax = 64;                   // utterances per chunk of a call, at most
// packed index of (i, j), i <= j, in the upper triangle of an n x n matrix stored row by row
inline size_t iv_tri(int i, int j, int n) { return (size_t)i * n - (size_t)i * (i - 1) / 2 + (j - i); }
// position of the product x_i x_j (i <= j < 72) in z, after the 72 linear terms
inline int iv_zpos(int i, int j) { return kIvDim + (int)iv_tri(i, j, kIvDim); }

struct IvModel {
    bool loaded = false;
    int C = 0, Cp = 0;          // Gaussians, rounded up to a multiple of 64 (the loglik kernel's wave tile)
    int R = 0, P = 0, Pp = 0;   // i-vector dimension, R (R + 1) / 2, P rounded up to a multiple of 256
    PldaBackend be;
    float offset = 0.f;
    float* gconst = nullptr;    // [C]
    float* W = nullptr;         // [kIvK][Cp] k-major, zero columns past C
    uint16_t* pairs = nullptr;  // [kIvK]: i | j << 8 with z_k = x_i x_j, x_72 = 1 (the linear terms)
    float* Vt = nullptr;        // [C * 72][R]: V_c^T, V_c = M_c^T Sigma_c^-1
    float* U = nullptr;         // [C][Pp]: upper triangle of V_c M_c, zero past P
    float* emb_mean = nullptr;  // [R]
    float* lda_t = nullptr;     // [R + 1][D] (row R: the offset column)
    float* plda_pt = nullptr;   // [D][D] transposed
    std::vector<void*> allocs;
};
// chunk buffers, grown on demand before the first launch of a call
struct IvWorkspace {
    DevBuf<float> scale, raw, delta, cmvn, ll, rowmax, rowsum, n, f, ivec;
    DevBuf<double> Lmat, linpart;
    // the gradient's buffers (sg_iv_loss_grad and the backward stage entries only: a decision query never grows them)
    DevBuf<float> dw, dn, df, dg, dxpart, dcmvn, ddelta, draw, dframes;
    DevBuf<double> solved, lam, dnpart;
    std::vector<void*> allocs;
};
// utterances per chunk for F frames and C Gaussians: a pure function (the host double walks it)
inline int iv_chunk_rows(int F, int C) {
    const size_t per_utt = (size_t)F * C * sizeof(float);
    const size_t fit = ((size_t)256 << 20) / (per_utt ? per_utt : 1);
    return (int)std::max<size_t>(1, std::min<size_t>(kIvChunkMax, fit));
}
struct IvDeltaScales { float s1[7], s2[13]; };  // get_scales(window 3, order 2), iv_plda.py:277-293, in its float32 order
IvDeltaScales iv_delta_scales();
// What sg_iv_load derives from the reference's arrays, on the host in float64 rounded once: W [kIvK][Cp], Vt [C * 72][R],
// U [C][Pp], pairs [kIvK].  false + text: a non-finite or asymmetric matrix.
bool iv_pack_model(const sg_iv_weights* w, int Cp, int Pp, std::vector<float>* W, std::vector<uint16_t>* pairs, std::vector<float>* Vt,
                   std::vector<float>* U, std::string* why);
hipError_t launch_iv_delta_cmvn(const float* raw, int ld, int B, int F, float* delta_ws, float* delta_out, float* cmvn_out,
                                hipStream_t s);
hipError_t launch_iv_stats(const IvModel& m, const float* cmvn, int B, int F, float* ll, float* rowmax, float* rowsum, float* n,
                           float* f, hipStream_t s);
// solved (B, R) float64 or null: the solved vector s = w + offset e0, kept for the backward (dL = -lambda s^T); Lmat then holds
// the Cholesky factor G (the solve factors in place), which the backward's two triangular solves read
hipError_t launch_iv_extract(const IvModel& m, const float* n, const float* f, int B, double* Lmat, double* linpart, float* ivec,
                             hipStream_t s, double* solved = nullptr);
struct IvTailArgs {
    const float* ivec; int B;
    const int64_t* y; sg_loss_spec loss; const float* coef;  // coef: this chunk's first row of loss.coef_dev, or null
    float* emb; float* scores; int64_t* decisions; float* loss_out;
    float* dw = nullptr;  // (B, R) d loss / d i-vector, or null: forward only
};
hipError_t launch_iv_tail(const IvModel& m, const IvTailArgs& a, hipStream_t s);
// ---- the backward (k_ivector_bwd.hip); every launcher runs on the buffers of the chunk whose forward just ran
constexpr int kIvDnSlice = 8192;  // packed-triangle entries per partial sum of d n (a constant of the arithmetic, like kIvLinSlice)
inline int iv_dn_slices(int P) { return (P + kIvDnSlice - 1) / kIvDnSlice; }
// dw (B, R) float32 -> lam = L^-1 dw (float64) by two triangular solves on the factor in Lmat; Lmat then holds dLsym
// (-(lam_i s_j + lam_j s_i), -lam_i s_i on the diagonal, zero past P); d n (B, C) and d f (B, C, 72) from U and Vt
hipError_t launch_iv_extract_bwd(const IvModel& m, const float* dw, int B, double* Lmat, const double* solved, double* lam, double* dnpart,
                                 float* dn, float* df, hipStream_t s);
// d n, d f -> d ll (written to dg, row stride Cp, zero past C) and dx (B F, 72) = both terms of step 5; dxpart: kIvDxSplit x
// (B F, 72), the partial sums of the log-likelihood term
constexpr int kIvDxSplit = 4;
hipError_t launch_iv_stats_bwd(const IvModel& m, const float* cmvn, int B, int F, const float* ll, const float* rowmax, const float* rowsum,
                               const float* dn, const float* df, float* dg, float* dxpart, float* dx, hipStream_t s);
// dout: d cmvn (from_cmvn) or d delta -> ddelta (B, F, 72; written when from_cmvn, else read from dout) and draw (B, F, ld) with
// columns 24 .. ld - 1 zero, or null
hipError_t launch_iv_delta_cmvn_bwd(const float* dout, bool from_cmvn, int B, int F, float* ddelta, float* draw, int ld, hipStream_t s);

}  // namespace sg

struct sg_ctx {
    int device = 0;
    int num_cus = 256;               // compute units of the device: the stream-K launches are sized to it
    std::string err;
    sg::MfccTables tab{};
    bool tables_ready = false;
    float* range_scratch = nullptr;  // [512] partial max/min of check_input_range
    float* cw2_scratch = nullptr;    // [1024][32] loss2 partials
    float* sk_slabs = nullptr;       // stream-K scratch (k_conv_gemm.hip)
    unsigned* sk_flags = nullptr;
    sg::XvModel xv;
    sg::Workspace ws;
    sg::DefWorkspace def_ws;
    sg::DevTableCache rs_cache;      // the resampling defense's tables, keyed by content (k_resample.hip)
    sg::DevTableCache sp_cache;      // the spectrum gate's, keyed by T (k_spectrum.hip) ...
    sg::DevBuf<float2> sp_ws;        // ... its workspace (in model_allocs): [rows][2][N] of the largest call that did not fit LDS ...
    bool sp_lds_opted = false;       // ... and its > 64 KB dynamic-LDS opt-in
    sg::DevBuf<double> ssa_ws;       // the SSA calls' workspace (k_ssa.hip; in model_allocs): the largest call's matrices ...
    sg::DevBuf<int32_t> ssa_iws;     // ... and its counters, flags and ranks
    sg::DevTableCache stoi_cache;    // STOI's tables, keyed by fs (k_stoi.hip) ...
    sg::DevBuf<double> stoi_ws;      // ... its workspace (in model_allocs): the largest call's 10 kHz signals, energies and band values ...
    sg::DevBuf<int32_t> stoi_iws;    // ... and its kept-frame counts and indices
    // Health word: host-pinned, device-mapped.  A kernel that gives up on a stream-K hand-off (bounded spin) ORs a
    // bit into it; every pass entry point and sg_sync read the host side and fail loudly (no synchronisation needed).
    unsigned* err_host = nullptr;
    unsigned* err_dev = nullptr;
    bool use_streamk = true;         // sg_set_streamk
    int lose_handoffs = 0;           // sg_debug_lose_handoffs: stream-K launches left that publish no hand-off flags
    int lose_feco = 0;               // ... and paired k-means launches left whose second halves publish nothing (own budget)
    // FeCo k-means over two CUs per instance (k_feco.hip): exchange buffers + flags, the launch counter the flag values
    // are derived from, and the switch (sg_feco_set_two_cu: -1 where it fits, 0 never)
    unsigned long long* feco_xchg = nullptr;
    unsigned* feco_flags = nullptr;
    unsigned feco_epoch = 0;
    int feco_two_cu = -1;
    sg::AnTables an_tab{};
    sg::AnFrontCfg an_cfg{};
    bool an_tables_ready = false;
    sg::AnModel an;
    sg::AnWorkspace an_ws;
    sg::IvModel iv;                  // the GMM / i-vector system (sg_api_ivector.hip) ...
    sg::IvWorkspace iv_ws;           // ... and its chunk buffers
    std::vector<void*> model_allocs;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Stage trace (sg_trace_begin / sg_trace_end): while on, every launch of the x-vector pass sequences is bracketed by a
    // pair of HIP events on the launch stream; a record = (stage tag, event before, event after).
    bool trace_on = false;
    bool trace_open = false;   // the opening event of record trace_used was recorded, the closing one not yet
    int trace_dropped = 0;     // records given up because an event record failed (reported by sg_trace_end)
    int trace_used = 0;
    std::vector<hipEvent_t> trace_ev;  // 2 per record
    std::vector<int> trace_tag;
};

namespace sg {

// stage trace: event pair around one launch (no-op unless sg_trace_begin switched it on and records are left).  A
// record whose opening or closing event could not be recorded is dropped -- its slot is reused by the next launch --
// and counted; sg_trace_end reports the count instead of a later, unrelated-looking HIP error.  A launch error
// between the two marks leaves the record open; the next opening mark simply overwrites it.
inline void trace_mark(sg_ctx* ctx, int tag, hipStream_t s, int after) {
    if (!ctx->trace_on || ctx->trace_used >= (int)ctx->trace_tag.size()) return;
    if (!after) {
        ctx->trace_tag[ctx->trace_used] = tag;
        ctx->trace_open = hipEventRecord(ctx->trace_ev[2 * ctx->trace_used], s) == hipSuccess;
        if (!ctx->trace_open) ++ctx->trace_dropped;
    } else {
        if (!ctx->trace_open || ctx->trace_tag[ctx->trace_used] != tag) return;
        ctx->trace_open = false;
        if (hipEventRecord(ctx->trace_ev[2 * ctx->trace_used + 1], s) == hipSuccess) ++ctx->trace_used;
        else ++ctx->trace_dropped;
    }
}

// ---------------------------------------------------------------- host helpers of the entry points
// a refusal or failure: the text goes to the context (sg_last_error), the code back to the caller
inline int fail(sg_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

// inside a function with `ctx` (and, for SG_STAGE, the stream `s`) in scope
#define SG_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return sg::fail(ctx, SG_ERR_HIP, "%s failed: %s (%s:%d)", #expr,         \
                                              hipGetErrorString(e_), __FILE__, __LINE__);              \
    } while (0)

#define SG_STAGE(tag, expr)               \
    do {                                  \
        sg::trace_mark(ctx, (tag), s, 0); \
        SG_HIP(expr);                     \
        sg::trace_mark(ctx, (tag), s, 1); \
    } while (0)

// device memory owned by `pool` (a model's or a workspace's list: freed with it)
template <typename T>
int dev_alloc(sg_ctx* ctx, std::vector<void*>& pool, T** out, size_t count) {
    void* p = nullptr;
    SG_HIP(hipMalloc(&p, count * sizeof(T) + 256));
    pool.push_back(p);
    *out = reinterpret_cast<T*>(p);
    return SG_OK;
}
template <typename T>
int dev_upload(sg_ctx* ctx, std::vector<void*>& pool, T** out, const std::vector<T>& host) {
    int rc = dev_alloc(ctx, pool, out, host.size());
    if (rc) return rc;
    SG_HIP(hipMemcpy(*out, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return SG_OK;
}
// an on-demand workspace buffer of at least `need` elements, grown before a loop: the old one is released once the stream
// has drained (nothing enqueued still uses it), not left in the pool until sg_destroy
template <typename T>
int dev_grow(sg_ctx* ctx, std::vector<void*>& pool, DevBuf<T>* buf, size_t need, hipStream_t s) {
    if (buf->ptr && buf->cap >= need) return SG_OK;
    if (buf->ptr) {
        SG_HIP(hipStreamSynchronize(s));
        (void)hipFree(buf->ptr);
        pool.erase(std::remove(pool.begin(), pool.end(), static_cast<void*>(buf->ptr)), pool.end());
        *buf = DevBuf<T>();
    }
    int rc = dev_alloc(ctx, pool, &buf->ptr, need);
    if (rc) return rc;
    buf->cap = need;
    return SG_OK;
}
// ---- the PLDA back end of a speaker model (plda_backend.hip); `pool`: the model's allocations
// the two log-determinants (float64 sums, rounded once) and the uploads of plda_mean, plda_psi and the enrolled table
int plda_backend_load(sg_ctx* ctx, std::vector<void*>& pool, PldaBackend* be, const float* plda_mean, const float* plda_psi,
                      const float* enroll, int D, int S, float threshold);
// a new enrolled table (waits for the device, grows the buffer and frees the old one when S exceeds it) and / or threshold
int plda_backend_set_enroll(sg_ctx* ctx, PldaBackend* be, std::vector<void*>& pool, const float* enroll_host, int S, float threshold);
inline void plda_backend_override(PldaBackend* be, const float* enroll_dev, int S) {
    be->enroll_override = enroll_dev;
    be->S_override = enroll_dev ? S : 0;
}
// the table and the count a launch scores against: the per-call override, else the model's own
inline void plda_backend_active(const PldaBackend& be, const float** enroll, int* S) {
    *enroll = be.enroll_override ? be.enroll_override : be.enroll;
    *S = be.enroll_override ? be.S_override : be.S;
}

// A new entry (key and blob filled in; the cache owns it from here on) goes to the device on `s` and into `cache`, which holds
// `cap` entries: when it is full, the oldest leaves once nothing enqueued can still read it -- the upload is enqueued first,
// then the stream is waited for, the one case that waits.  On any failure the entry and its device memory are released.  `of`
// ends the text of a refusal for lack of memory.
inline int dev_tables_insert(sg_ctx* ctx, const char* who, const char* of, DevTableCache* cache, size_t cap, DevTable* e,
                             hipStream_t s) {
    std::vector<DevTable*>& all = cache->entries;
    if (hipMalloc(&e->dev, e->blob.size()) != hipSuccess) {
        e->dev = nullptr;
        delete e;
        return fail(ctx, SG_ERR_HIP, "%s: no device memory for the tables%s", who, of);
    }
    bool ok = hipMemcpyAsync(e->dev, e->blob.data(), e->blob.size(), hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok && all.size() >= cap) ok = hipStreamSynchronize(s) == hipSuccess;
    if (!ok) {
        delete e;
        return fail(ctx, SG_ERR_HIP, "%s: the upload of the tables failed", who);
    }
    if (all.size() >= cap) {
        delete all.front();
        all.erase(all.begin());
    }
    all.push_back(e);
    return SG_OK;
}

// ---------------------------------------------------------------- one pass of a device-resident PGD loop
// Step `it` of a loop runs its `reps` EOT repeats as passes of at most G repeats (rows = repeat * B + utterance), the last
// step (it == max_iter) one forward repeat.  What the pass that starts at repeat g0 is: a pure function of its arguments (no HIP
// call, no context), shared by the x-vector and the AudioNet loop.
constexpr uint64_t kStepKey = 0x9E3779B97F4A7C15ull;  // key stride from one PGD step to the next
constexpr uint64_t kRepKey = 0xC2B2AE3D27D4EB4Full;   // ... from one EOT repeat to the next (the kernels' stride for the rows of a pass)
struct LoopPass {
    bool last;          // the final pass: the caller's outputs, no gradient
    int nrep;           // repeats of this step
    int Gi;             // repeats of this pass
    int rows;           // Gi * B
    bool final_group;   // the step's last pass takes the step; earlier ones carry their sum
    uint64_t pass_key;  // added to every seed of the pass (dither, AT, FeCo)
    // Per-step records (attack/FGSM.py:50-58: loss averaged, decision voted over ALL repeats of the step): where the head
    // writes its rows.  DIRECT: one repeat, row `it` of the caller's trace.  PASS: several repeats in one pass, the pass
    // scratch, reduced right after the head.  GROUPED: more repeats than a pass holds, the grouped rows at rec_offset in repeat
    // order, reduced after the last group.
    enum Records { NONE, DIRECT, PASS, GROUPED } rec;
    size_t rec_offset;
    bool reduce;        // the reduction over the step's nrep repeats follows this pass
};
inline LoopPass loop_pass(int it, int max_iter, int g0, int G, int reps, int B, bool want_rec) {
    LoopPass p;
    p.last = it == max_iter;
    p.nrep = p.last ? 1 : reps;
    p.Gi = std::min(G, p.nrep - g0);
    p.rows = B * p.Gi;
    p.final_group = g0 + p.Gi >= p.nrep;
    p.pass_key = (uint64_t)it * kStepKey + (uint64_t)g0 * kRepKey;
    p.rec = !want_rec ? LoopPass::NONE : p.nrep == 1 ? LoopPass::DIRECT : p.nrep > G ? LoopPass::GROUPED : LoopPass::PASS;
    p.rec_offset = (size_t)g0 * B;
    p.reduce = p.rec == LoopPass::PASS || (p.rec == LoopPass::GROUPED && p.final_group);
    return p;
}
// the head's record pointer of the pass: trace_row = row `it` of the caller's trace (null: that record is not wanted)
template <typename T>
T* loop_record_rows(const LoopPass& p, T* trace_row, T* pass_scratch, T* grouped) {
    switch (p.rec) {
        case LoopPass::DIRECT: return trace_row;
        case LoopPass::PASS: return pass_scratch;
        case LoopPass::GROUPED: return grouped + p.rec_offset;
        default: return nullptr;
    }
}
// What every loop entry point refuses about its arguments, after its own NULL test (any_null) and with its own refusal about
// B / T (shape: the text, or null) in their place between the shared ones.
inline int loop_check_args(sg_ctx* ctx, bool any_null, const char* shape, const sg_pgd_params* p) {
    if (any_null) return fail(ctx, SG_ERR_ARG, "NULL argument");
    if (shape) return fail(ctx, SG_ERR_ARG, "%s", shape);
    if (p->max_iter < 0) return fail(ctx, SG_ERR_ARG, "max_iter must be >= 0");
    if (p->loss.loss == SG_LOSS_LINEAR && !p->loss.coef_dev) return fail(ctx, SG_ERR_ARG, "SG_LOSS_LINEAR needs coef_dev");
    return SG_OK;
}
// ... and, where the entry point takes EOT repeats: eot_size, or SG_ERR_ARG
inline int loop_eot_size(sg_ctx* ctx, const sg_pgd_params* p, int* eot_size) {
    const int eot_bs = p->eot_batch_size > 0 ? p->eot_batch_size : 1;
    *eot_size = p->eot_size > 0 ? p->eot_size : 1;
    if (*eot_size % eot_bs) return fail(ctx, SG_ERR_ARG, "EOT size should be divisible by EOT batch size");
    return SG_OK;
}


// ---------------------------------------------------------------- kernel launchers (k_*.hip)
enum Epilogue { EPI_NONE = 0, EPI_BIAS_RELU = 1, EPI_RELU_MASK = 2 };

struct ConvGemmArgs {
    const float* A;     // activations [B*Ta][lda]
    const float* W;     // weights [taps*Kc][ldw]
    const float* Wq;    // same weights packed k4-major [taps*Kc/4][ldw][4] (null: b32-fed kernels only)
    unsigned a_bytes, w_bytes;  // extents of A and W for the buffer descriptors (filled by launch_conv_gemm)
    float* C;           // output [B*Tc][ldc] (+ z*split_stride for split-K partials)
    const float* bias;  // [N]            (EPI_BIAS_RELU)
    const float* mask;  // [B*Tc][ldc]    (EPI_RELU_MASK: keep where mask > 0)
    int M, N;           // M = B*Tc rows, N multiple of the tile width
    int Ta, Tc;         // rows per utterance in A / C
    int Kc;             // K per tap, multiple of 32
    int lda, ldw, ldc;
    int taps, tap_step; // A row offset of tap j = tap_base + j * tap_step
    int tap_base;
    int total_chunks, chunks_per_split;
    long long split_stride;
    int sk_xcd;         // stream-K: XCD-contiguous workers + n-tile-major tile order (see kernel)
    int num_cus;        // stream-K: persistent blocks = resident slots of THIS device (0: assume 256)
    unsigned long long* trace;  // tuning aid (SG_SK_TRACE): per-worker phase timestamps, 16 slots each, or null
    int force;          // parity tests (sg_conv1d_rows `kernel`): 0 auto, 1 one b32-fed block per tile, 2 the b32-fed kernels
                        // only (Wq dropped: stream-K kind 0 where the shape qualifies), 3 stream-K quad-fed 8-wave (kind 1),
                        // 4 one quad-fed block per tile, 5 16 x 16 blocks, 6 .. 10 stream-K kind force - 1 (roles split between
                        // waves: 128- / 64- / 32- / 256-row tiles, 128 rows as four 64 x 64 waves) or an error, never a tile launch
    int ablate;         // 8 = fault injection (sg_debug_lose_handoffs): stream-K hand-off flags are never published;
                        // builds with -DSG_EXP_ABLATE only (never the shipped library), from SG_ABLATE: 1 no global loads,
                        // 2 no LDS stores, 4 no barrier (results become wrong), 16 = A/B agent-scope fences around the hand-off
    int no_streamk;     // one block per tile whatever the shape (sg_set_streamk(ctx, 0): same bits, no co-residency needed)
    float* sk_slabs;    // stream-K: kSkSlabFloats floats, one parked partial tile [bm][128] per worker (may be null -> tile launch)
    unsigned* sk_flags; // stream-K: [kSkFlags] hand-off flags, one per worker, holding the epoch of the launch that parked
    unsigned* err_word; // stream-K: device-visible health word (bit 0 = a hand-off wait timed out), may be null
    int* lose_counter;  // HOST pointer (never dereferenced on the device): the context's fault-injection budget, may be null
};

// A process may hold one sg_ctx per GPU: whatever a launcher remembers between calls -- the > 64 KB dynamic-LDS opt-in of a
// kernel, a tuning aid's device buffer -- is remembered PER DEVICE (index = the current device, which every entry point
// sets from its context before launching).
// Tuning, tracing and test knobs are environment variables that count ONLY when SG_TUNE=1 is set as well (INTEGRATION.md,
// "Environment"): without it the library runs its own choices and a stray SG_* variable in a user's environment changes
// nothing.  The gate is read once per process; the knobs keep their own read-once / read-per-call behaviour.
inline const char* sg_tune_env(const char* name) {
    static const bool on = [] {
        const char* e = getenv("SG_TUNE");
        return e && atoi(e) != 0;
    }();
    return on ? getenv(name) : nullptr;
}

constexpr int kMaxDevices = 64;
inline int sg_device_slot() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d & (kMaxDevices - 1);
}
// a tuning aid's scratch buffer on the current device (allocated on first use, grown on demand, never freed: tuning aids only)
struct PerDeviceScratch {
    void* ptr[kMaxDevices] = {};
    size_t cap[kMaxDevices] = {};
    void* get(size_t bytes) {
        const int d = sg_device_slot();
        if (cap[d] < bytes) {
            if (ptr[d]) (void)hipFree(ptr[d]);
            ptr[d] = nullptr;
            cap[d] = 0;
            if (hipMalloc(&ptr[d], bytes) == hipSuccess) cap[d] = bytes;
        }
        return ptr[d];
    }
};

// the launch-side bookkeeping every contraction of a context carries
inline void conv_ctx_args(sg_ctx* ctx, ConvGemmArgs& a) {
    a.sk_slabs = ctx->sk_slabs;
    a.sk_flags = ctx->sk_flags;
    a.err_word = ctx->err_dev;
    a.num_cus = ctx->num_cus;
    a.no_streamk = ctx->use_streamk ? 0 : 1;
    a.ablate = 0;
    // test hook (sg_debug_lose_handoffs): launch_streamk takes a launch off this counter when it actually launches a
    // stream-K kernel -- launches that end up on tile kernels (tdnn1, split-K, forced kinds) do not use the budget up
    a.lose_counter = ctx->use_streamk ? &ctx->lose_handoffs : nullptr;
}

// stream-K scratch of a context: room for 512 parked 128 x 128 (or 256 parked 256 x 128) partial tiles, and the flags
constexpr size_t kSkSlabFloats = (size_t)512 * 128 * 128;
constexpr int kSkFlags = 1024;

// stream-K kinds (k_conv_gemm.hip, above conv_gemm_streamk_kernel): waves along M and the tile height
constexpr int sk_wm(int kind) { return (kind == 2 || kind == 8) ? 4 : (kind == 3 || kind == 4 || kind == 6 || kind == 7) ? 1 : 2; }  // (9: 2)
constexpr int sk_bm(int kind) { return (kind == 4 || kind == 7) ? 32 : 64 * sk_wm(kind); }

// the launcher's tuning knobs with their defaults (SG_* names: INTEGRATION.md "Environment"; read by conv_knobs())
struct ConvKnobs {
    int streamk = 1;         // SG_STREAMK: 0 = always one block per tile
    int kind = 0;            // SG_STREAMK_KIND: 5 .. 9 = this wave-specialised kind wherever the shape qualifies
    int w16 = 1;             // SG_STREAMK_W16: 0 = two 8-wave 128x128 blocks per CU instead of the 16-wave 256x128 one
    int mid = 1;             // SG_STREAMK_MID: 0 = no one-block-per-CU launches for fewer 256-row tiles than CUs
    int mid9 = 0;            // SG_STREAMK_MID9: 1 = 128-row tiles as four 64 x 64 computing waves (kind 9) instead of kind 5
    int deep = 1;            // SG_STREAMK_DEEP: 0 = the all-in-one kinds 1 / 3 / 4 instead of the wave-specialised 5 / 6 / 7
    int ws = 1;              // SG_STREAMK_WS: 0 = the all-in-one 16-wave kernel (kind 2) for the full batch
    int ws_minchunks = 64;   // SG_STREAMK_WS_MINCHUNKS: full batch, chunks per tile from which kind 8 beats kind 5
    int minchunks = 16;      // SG_STREAMK_MINCHUNKS: shorter K is faster one block per tile (tdnn1: 5 chunks)
    int xcd = 2;             // SG_STREAMK_XCD: worker / tile order, see the kernel
    int quadfeed = 1;        // SG_QUADFEED: 0 = b32-fed kernels even when packed weights exist
    int tile32 = 1;          // SG_TILE32: 0 = always 64-row quad tiles
    long s16_max_blocks = 2800;  // SG_S16_MAX_BLOCKS: 16 x 16 blocks up to which every one has a SIMD (almost) to itself; 0 = never
};

// What launch_conv_gemm launches for a shape: a pure function of its arguments (no HIP call, no state), so the CPU build
// can walk it (tests/test_launch_table.py).  One thing is left to the launcher, because only the runtime knows it: a
// STREAMK plan whose `workers` blocks of `kind` are not all resident at once takes `fallback` instead.
struct ConvPlan {
    enum Path { INVALID, S16, STREAMK, QUAD32, QUAD64, TILE_64x128, TILE_128x32 };
    Path path = INVALID;      // 16 x 16 blocks, stream-K, quad-fed 32- / 64-row tiles, b32-fed 64 x 128 / 128 x 32 tiles
    Path fallback = INVALID;  // STREAMK only: the one-block-per-tile path, INVALID for a forced kind
    int kind = 0, bm = 0, workers = 0, cus = 0, mtiles = 0, ntiles = 0, tiles = 0, ipw = 0;  // STREAMK only; cus: resident slots / blocks per CU
};
// tile: 0 = auto, 1 = 128x32 (4x1 waves), 2 = 64x128, the last two always one block per tile; wq: packed weights usable
inline ConvPlan conv_plan(int M, int N, int total_chunks, int tile, int splits, int force, bool wq, bool slabs, bool no_streamk,
                          int num_cus, const ConvKnobs& k) {
    ConvPlan p;
    // batch 1-4: so few 16 x 16 output blocks that every one can have a SIMD (almost) to itself
    if ((tile == 0 || tile == 2) && splits == 1 && wq && N % 32 == 0 &&
        (force == 5 || (force == 0 && total_chunks >= 4 && (long)((M + 15) / 16) * (N / 16) <= k.s16_max_blocks))) {
        p.path = ConvPlan::S16;
        return p;
    }
    if (tile == 1 && N % 32 == 0) p.path = ConvPlan::TILE_128x32;
    if ((tile != 0 && tile != 2) || N % 128) return p;
    const int nt = N / 128;
    const auto mt = [&](int rows) { return (M + rows - 1) / rows; };
    // One block per tile.  A nearly empty chip (batch <= 8: fewer 64-row tiles than CUs) waits for the sequential k chain of
    // one tile; 32-row tiles halve the MFMAs per wave and chunk, so the chain -- and the launch -- takes half as long.
    p.path = ConvPlan::TILE_64x128;
    if (wq && splits == 1 && force != 1)
        p.path = k.tile32 && force == 0 && total_chunks >= 8 && mt(64) * nt < (num_cus > 0 ? num_cus : 256) ? ConvPlan::QUAD32 : ConvPlan::QUAD64;
    if (tile != 0 || splits != 1 || !k.streamk || no_streamk || force == 1 || force == 4) return p;

    // Stream-K: one worker per resident slot of this device (slabs / flags are sized for 256 CUs) -- two 8-wave blocks per
    // CU for kinds 0 / 1 as first chosen, one block per CU for every other choice.
    const int cus = num_cus > 0 && num_cus < 256 ? num_cus : 256;
    int kind = !wq ? 0 : (k.w16 && force != 3) ? 2 : 1;
    int workers = kind == 2 ? cus : 2 * cus;
    const auto one_per_cu = [&](int kd) { kind = kd; workers = cus; };
    // Medium batches (B = 32 at 3 s: 136 tiles of 256 rows for 256 CUs): fewer 256-row tiles than CUs would leave the launch
    // to the 4-wave tile kernel at ~100 TFLOP/s.  The tallest tile that still gives every CU one: 128 rows (B = 32), 64 rows
    // (B = 16: balances the 272 tiles a one-block-per-tile launch would spread as 240 x 1 + 16 x 2), 32 rows (B = 8: half
    // the k chain per tile).
    if (k.mid && kind == 2 && force == 0 && mt(256) * nt < cus) {
        if (mt(128) * nt >= cus) one_per_cu(k.deep ? (k.mid9 ? 9 : 5) : 1);
        else if (mt(64) * nt >= cus) one_per_cu(k.deep ? 6 : 3);
        else if (mt(32) * nt >= cus) one_per_cu(k.deep ? 7 : 4);
    }
    // The full batch (>= 256 tiles of 256 rows), measured per layer at 64 utterances (profiles/r03_layers.txt): with the roles
    // split between waves (kind 8) tdnn2 / tdnn3 (80 / 112 chunks per tile) gain 1-3 %, tdnn4 / tdnn5 (16 / 48 chunks)
    // lose 4-8 %; those are 3-4 % faster as 128-row tiles on kind 5 than on the all-in-one kind 2.
    if (k.ws && kind == 2 && force == 0) one_per_cu(total_chunks >= k.ws_minchunks ? 8 : 5);
    // every range must span at least one full tile's worth of chunks, so a tile is shared by at most two workers and never
    // lies strictly inside one range
    const auto ipw = [&](int kd, int w) { return (int)(((long)mt(sk_bm(kd)) * nt * total_chunks + w - 1) / w); };
    const auto qualifies = [&](int kd, int w) { return mt(sk_bm(kd)) * nt >= w && ipw(kd, w) >= total_chunks; };
    if (k.kind >= 5 && k.kind <= 9 && force == 0 && wq && qualifies(k.kind, cus)) one_per_cu(k.kind);  // else: leave the choice alone
    if (force >= 6 && force <= 10 && wq) one_per_cu(force - 1);  // parity tests: this kind or an error
    p.fallback = force >= 6 ? ConvPlan::INVALID : p.path;
    p.path = slabs && qualifies(kind, workers) && total_chunks >= k.minchunks ? ConvPlan::STREAMK : p.fallback;
    p.kind = kind; p.bm = sk_bm(kind); p.workers = workers; p.cus = cus;
    p.mtiles = mt(p.bm); p.ntiles = nt; p.tiles = p.mtiles * nt; p.ipw = ipw(kind, workers);
    return p;
}
hipError_t launch_conv_gemm(const ConvGemmArgs& a, int tile, int epi, int splits, hipStream_t s);
// [K][N] row-major -> k4-major [K/4][N][4] on the device (K % 4 == 0): the packed weights (Wq) of the quad-fed kernels
hipError_t launch_pack_k4(const float* w, int K, int N, float* wq, hipStream_t s);

// mode 0: xv_plda ('origin': [-1,1] -> x32768), mode 1: AudioNet ('scale': int16 range -> /32768)
hipError_t launch_input_scale(const float* x, int64_t n, float* scratch512, float* scale, int mode, hipStream_t s);
// rl (here and below): the per-utterance sample counts of a batch of unequal lengths -- T, F (and Tc) are then the row strides,
// the longest utterance's -- or none: a uniform batch
hipError_t launch_mfcc_fwd(const MfccTables& t, const float* x, int B, int T, int F, const float* scale,
                           const sg_dither* dz, float* feats, hipStream_t s, const RowLens& rl = RowLens());
hipError_t launch_mfcc_bwd(const MfccTables& t, const float* x, int B, int T, int F, const float* scale,
                           const sg_dither* dz, const float* dfeats, float* dframes, hipStream_t s, const RowLens& rl = RowLens());
// overlap-add of dframes into d loss / d x (+ acc_in, the sum over earlier EOT repeats; may alias grad_out);
// optional fused PGD update of x (in place)
// dframes (R, B, F, 400): R batched EOT repeats, summed in repeat order
hipError_t launch_frames_to_wave(const float* dframes, int B, int T, int F, int R, const float* acc_in, float* grad_out,
                                 float* x_io, const float* lower, const float* upper, float step, int grad_sign,
                                 hipStream_t s, const RowLens& rl = RowLens());
// The two launches above as the one MFCC adjoint (sg_api.hip): dfeats (B, F, 30) -> dframes (the caller's buffer) -> d loss / d x,
// the B rows being `reps` repeats of B / reps utterances.  `staged`: the launches carry their SG_STAGE tags (the x-vector pass)
int mfcc_adjoint(sg_ctx* ctx, const MfccTables& tab, const float* x, int B, int T, int F, const float* scale, const sg_dither* dz,
                 const float* dfeats, float* dframes, int reps, const float* acc_in, float* grad_out, float* x_io, const float* lower,
                 const float* upper, float step, int grad_sign, bool staged, hipStream_t s, const RowLens& rl = RowLens());
hipError_t launch_pgd_update(float* x, const float* g, const float* lo, const float* hi, int64_t n,
                             float step, int grad_sign, hipStream_t s);
// planes (G, n): the cotangents of G EOT repeats; total = ((carry +) p0 + p1) + ... in float32, in that order.  sum_out != null:
// the total is written there (may alias carry); x != null: x <- clamp(x + step * grad_sign * sign(total), lo, hi), the bits
// of launch_pgd_update on the same total.  One pass over memory (k_attack.hip).
hipError_t launch_wav_rep_sum_update(const float* planes, int G, int64_t n, const float* carry, float* sum_out, float* x,
                                     const float* lo, const float* hi, float step, int grad_sign, hipStream_t s);
// what sg_wav_defense_* / sg_wav_filter_* refuse about the spec itself, said before any launch (k_time_domain.hip,
// k_freq_domain.hip): SG_OK or SG_ERR_ARG with the context's error text set
int wav_defense_check_spec(sg_ctx* ctx, const char* who, const sg_wav_defense* d);
int wav_filter_check_spec(sg_ctx* ctx, const char* who, const sg_wav_filter* f);

// ---- the chain of the defended device loops (sg_api.hip), shared by sg_xv_pgd_run_defended and sg_an_pgd_run_defended
// buffers for passes of `rows` x T: n_out stage outputs, n_saved int8 planes, and -- `rep` -- the replicated iterate and the two
// cotangent planes.  Called before the loop; a request the buffers already cover costs nothing.
int ensure_def_workspace(sg_ctx* ctx, int rows, int T, int n_out, int n_saved, bool rep, hipStream_t s);
struct DefChainInfo {
    bool randomised;  // holds AT: the EOT repeats of a step differ
    bool identity;    // QT / BDR only: the chain's backward is the identity
    int n_saved;      // int8 planes its stages keep (MS, filters)
};
// everything a stage call would refuse about the chain, said before any launch: SG_OK or SG_ERR_ARG with the error text set
int def_chain_check(sg_ctx* ctx, const char* who, const sg_wav_stage* chain, int n_stages, DefChainInfo* info);
struct DefChainTape {  // what one pass's forward leaves for its backward
    sg_wav_defense spec[SG_WAV_CHAIN_MAX];  // the pass's specs (AT: with the pass's key)
    const float* in[SG_WAV_CHAIN_MAX];
    void* saved[SG_WAV_CHAIN_MAX];
};
// the scale / clip decision of a first stage that reads one, from the iterate (n floats), once per call
int def_chain_first_scale(sg_ctx* ctx, const sg_wav_stage* chain, const float* x, int64_t n, hipStream_t s);
// x (rows, T) through the chain into the workspace's stage outputs; *out = the defended rows.  AT's key is its spec's seed +
// pass_key, rep_rows > 0: the rows are EOT repeats of rep_rows utterances.  A later stage's scale / clip decision: from its input.
int def_chain_forward(sg_ctx* ctx, const sg_wav_stage* chain, int n_stages, const float* x, int rows, int T, uint64_t pass_key,
                      int rep_rows, DefChainTape* tape, const float** out, hipStream_t s);
// the cotangent in the workspace's plane g[0] back through the chain, last stage first, ping-ponging the two planes; *gi: the
// plane that holds the result.  Nothing is launched for QT / BDR.
int def_chain_backward(sg_ctx* ctx, const sg_wav_stage* chain, int n_stages, const DefChainTape& tape, int rows, int T, int* gi,
                       hipStream_t s);
// out[r][0..ncol) = in[r][0..ncol), out[r][ncol..ld_out) = 0
hipError_t launch_copy_cols(const float* in, int ld_in, float* out, int ld_out, int64_t rows, int ncol, hipStream_t s);
hipError_t launch_sum_cols(const float* in, int ld_in, int nsplit, long long slab_stride, float* out, int ld_out,
                           int64_t rows, int ncol, hipStream_t s);
hipError_t launch_cmvn_fwd(const float* in, int ld_in, float* out, int ld_out, int B, int F, hipStream_t s,
                           const RowLens& rl = RowLens(), int T = 0);
hipError_t launch_cmvn_bwd(const float* dout, int ld_dout, int nsplit, long long slab_stride, float* din, int ld_din,
                           int B, int F, hipStream_t s, const RowLens& rl = RowLens(), int T = 0);
hipError_t launch_pool_fwd(const float* act5, int B, int Tc, float* stats, hipStream_t s, const RowLens& rl = RowLens(), int T = 0);
hipError_t launch_pool_bwd(const float* act5, const float* stats, const float* dstats_part, int nsplit,
                           int B, int Tc, float* dact5, hipStream_t s, const RowLens& rl = RowLens(), int T = 0);

hipError_t launch_cw2_step(float* modifier, float* exp_avg, float* exp_avg_sq, const float* x, const float* input_cur,
                           const float* grad1, const float* const_c, int B, int T, float lr, int step_t,
                           float* input_next, float* loss2, float* scratch, hipStream_t s);
hipError_t launch_nes_queries(const float* x, int n, int T, int half, int with_clean, float sigma, uint64_t seed,
                              int64_t index_base, int pair_base, const float* noise_in, float* queries, float* noise_out,
                              hipStream_t s);
hipError_t launch_nes_grad(const float* loss, int n, int T, int half, int with_clean, uint64_t seed, int64_t index_base,
                           int pair_base, const float* noise_in, int accumulate, float final_sigma, int final_batches,
                           float* grad, hipStream_t s);
hipError_t launch_fakebob_step(float* x, float* grad, const float* prev_grad, const float* lr, const float* lower,
                               const float* upper, int n, int T, float momentum, float one_m_momentum, int grad_sign,
                               hipStream_t s);

// ---- FeCo k-means (k_feco.hip): what the kernel and its launcher share, and the launcher's plan
constexpr int kFecoMaxD = 64;
constexpr int kFecoThreads = 1024;
constexpr int kFecoMaxChunks = 8;     // centroid-tile chunks a frame tile is cut into (JC)
constexpr int kFecoMergeCap = 2048;   // JC * F <= this: capacity rule of the chunk-maxima arrays
__host__ __device__ constexpr int al4(int n) { return (n + 3) & ~3; }

// Which units of the assignment a wave computes (host-built): u[wave][slot] = frame tile | first centroid tile << 8 | one
// past the last << 16 | chunk index << 24, kFecoNoUnit = none; table == 0: more than 32 units, dealt round robin in the kernel.
constexpr unsigned kFecoNoUnit = 0xFFFFFFFFu;
struct FecoSched {
    int table;
    unsigned u[kFecoThreads / 64][2];
};

// Two CUs per instance (round 5, VERDICT r4 item 1: "off the single CU").  An instance's k-means is bound by the MFMA +
// VALU issue of the four SIMDs of the one CU its block gets, and a batch of 64 x 2 instances leaves half of the chip idle.
// With `on` the grid's z dimension is the HALF: two blocks run the same instance redundantly -- same set-up, same lists,
// same update, bit for bit -- and split only the assignment's units (sched / sched1; bit u of `owner` says whose unit
// u = frame tile * JC + chunk is).  After its units a block stores its chunk maxima into its exchange buffer (two of them,
// alternating by iteration) as self-describing 8-byte words -- score | index << 32 | tag << 43, tag = launch and iteration --
// with write-through (sc1) stores, and polls the partner's words (sc1 loads) until they carry the tag it expects: one
// store -> load visibility delay per iteration, no flag, no fence (the first version published a flag after draining the
// stores: 3.2 us per iteration, as much as the split saved).  A word is accepted only with the exact tag, so stale or
// overwritten data cannot be taken for the partner's; the buffers are zeroed when the launch counter wraps.
// No block ever waits unboundedly, and no result depends on the partner showing up: if any word is not there after
// kFecoPairWait the block computes the partner's units itself from then on (and says so in `flags`, which saves the
// partner its own time-out).  The partner not showing up is what happens when something else occupies the GPU: same bits,
// the single-CU speed (+ one time-out).
struct FecoPair {
    int on;
    unsigned owner;
    FecoSched sched1;
    unsigned long long* xchg;  // [instance][half][buffer 0 / 1][kFecoMergeCap]
    unsigned* flags;           // [instance][half]: launch id of the launch in which the block went on alone
    unsigned tag0;             // this launch's tag base: (launch counter mod 2^15) << 6; a word's tag = tag0 + iteration + 1
    unsigned launch;           // launch id
    int drop;                  // test hook (sg_debug_lose_handoffs): half 1 publishes nothing
};
constexpr int kFecoPairMaxIter = 62;        // tag = 15 bits of launch counter, 6 of iteration
constexpr size_t kFecoLdsMax = 150 * 1024;  // 150 KB cover ~19 s at D <= 32, ratio 0.5 (F = 1930, k = 965); beyond that the call is refused

// Dynamic LDS of feco_kmeans_kernel in 4-byte words (every array 16-byte aligned); host and device use the same function.
struct FecoLds {
    int cq, hq, mu, part, ids, cnt, start, members, cw, spart, wtot, pd, pj, xq, total;
};
__host__ __device__ inline FecoLds feco_layout(int F, int k, int dpad, int JC, int fast_lists, int x_in_lds) {
    const int kp = (k + 31) & ~31;
    FecoLds L;
    int o = 0;
    L.cq = o; o += kp * dpad;              // centred centroids, [kp][dpad], 16-byte slots XOR-permuted per row
    L.hq = o; o += kp;                     // -|c|^2 / 2
    L.mu = o; o += dpad;
    L.part = o; o += 16 * dpad;            // partial sums of the centring
    L.ids = o; o += al4(F);
    L.cnt = o; o += al4(k);
    L.start = o; o += al4(k + 1);
    L.members = o; o += al4(F);            // frames grouped by cluster, ascending inside a group
    L.cw = o; o += fast_lists ? al4(((F + 63) >> 6) * k) : 0;   // members of cluster j among frames 64 c .. 64 c + 63
    L.spart = o; o += fast_lists ? al4(k) : 0;                  // frames of the lower clusters of j's wave of clusters
    L.wtot = o; o += fast_lists ? 16 : 0;                       // frames per wave of clusters
    L.pd = o; o += JC > 1 ? al4(JC * F) : 0;                    // chunk maxima [chunk][frame]
    L.pj = o; o += JC > 1 ? al4(JC * F) : 0;
    L.xq = o; o += x_in_lds ? F * dpad : 0;                     // centred frames, same permuted rows
    L.total = o;
    return L;
}

// What feco_kmeans_impl launches for a shape: a pure function of its arguments (no HIP call, no context, no statics), so the
// CPU build can walk it (tests/test_feco_plan_table.py, and the invariants in tests/native/feco_cos_asan_driver.cpp).  For
// shapes feco_kmeans_check admits.  One thing is left to the launcher, because only the runtime knows it: a plan with `pair`
// whose exchange buffers feco_pair_buffers cannot provide is planned again with allow_pair = false.
struct FecoKnobs {
    int two_cu = -1;  // sg_feco_set_two_cu: -1 where it fits, 0 never
    int jc = 0;       // SG_FECO_JC (experiment builds only): this many chunks where the shape allows, 0 = the plan's own
};
struct FecoPlan {
    int dpad, JC, x_in_lds, fast_lists;
    size_t lds;
    bool pair;                 // two blocks per instance
    FecoSched sched0, sched1;  // units in sched1 and bits in owner only when pair
    unsigned owner;
};
inline FecoPlan feco_plan(int F, int D, int k, int max_iter, long instances, int num_cus, bool allow_pair, const FecoKnobs& knobs) {
    FecoPlan p{};
    // LDS holds the centred centroids (rows padded to 32 / 64 floats), ids, member lists and -- when they fit -- the chunk
    // counts of the fast member lists and the centred frames (else the frames are re-read from HBM / L2 in every step)
    p.dpad = D <= 32 ? 32 : 64;
    const auto bytes = [&](int jc, int fast, int xin) { return (size_t)feco_layout(F, k, p.dpad, jc, fast, xin).total * sizeof(float); };
    // a frame tile's centroid tiles are cut into JC chunks (300 x 150: 10 frame tiles x 2 chunks of 3 / 2 tiles)
    const int ntc = (k + 31) / 32, ntf = (F + 31) / 32;
    int JC = (20 + ntf - 1) / ntf;  // >= 20 units for the 16 waves (5 per SIMD), each as many tiles as possible
    JC = JC > ntc ? ntc : JC;
    JC = JC > kFecoMaxChunks ? kFecoMaxChunks : JC;
    while (JC > 1 && JC * F > kFecoMergeCap) --JC;
    if (knobs.jc) {
        JC = knobs.jc < 1 ? 1 : (knobs.jc > ntc ? ntc : knobs.jc);
        while (JC > 1 && JC * F > kFecoMergeCap) --JC;
    }
    if (bytes(JC, 0, 0) > kFecoLdsMax) JC = 1;  // (one chunk fits: feco_kmeans_check)
    p.JC = JC;
    // two CUs per instance (FecoPair): when every instance can have two resident blocks, the units fit the tables and a bit
    // mask, and the flag values have room for the iterations.  Same units as one block would get (cutting them finer -- 30
    // units of 1-2 tiles for the 32 waves -- measured 94.3 against 92.5 us per call: the SIMDs are throughput-bound, the
    // merge grows)
    const int cus = num_cus > 0 ? num_cus : 256, nunits = ntf * JC;
    p.pair = allow_pair && knobs.two_cu != 0 && p.dpad == 32 && 2 * instances <= cus && JC > 1 && nunits <= 32 &&
             max_iter <= kFecoPairMaxIter && ((k + 31) & ~31) <= 2048;
    // the assignment's units (frame tile, chunk jc of its centroid tiles [ntc jc / JC, ntc (jc + 1) / JC)) dealt to the waves:
    // largest first, each to the least loaded SIMD (waves w, w + 4, w + 8, w + 12; of both blocks when paired) and there to the
    // least loaded wave with a free slot -- 300 x 150: 20 units of 2 / 3 tiles -> 12 / 13 / 12 / 13 tiles per SIMD
    constexpr int kWaves = kFecoThreads / 64;
    if (nunits <= 2 * kWaves) {
        p.sched0.table = p.sched1.table = 1;
        int simd_load[8] = {}, wave_load[2 * kWaves] = {}, wave_n[2 * kWaves] = {};
        for (int w = 0; w < kWaves; ++w) p.sched0.u[w][0] = p.sched0.u[w][1] = p.sched1.u[w][0] = p.sched1.u[w][1] = kFecoNoUnit;
        const auto bin = [&](int w) { return (w / kWaves) * 4 + (w & 3); };
        for (int size = ntc; size >= 1; --size)
            for (int u = 0; u < nunits; ++u) {
                const int ft = u / JC, jc = u - ft * JC, lo = ntc * jc / JC, hi = ntc * (jc + 1) / JC;
                if (hi - lo != size) continue;
                int best_w = -1;
                for (int w = 0; w < (p.pair ? 2 : 1) * kWaves; ++w) {
                    if (wave_n[w] >= 2) continue;
                    if (best_w < 0 || simd_load[bin(w)] < simd_load[bin(best_w)] ||
                        (simd_load[bin(w)] == simd_load[bin(best_w)] && wave_load[w] < wave_load[best_w]))
                        best_w = w;
                }
                const unsigned word = (unsigned)ft | (unsigned)lo << 8 | (unsigned)hi << 16 | (unsigned)jc << 24;
                if (best_w < kWaves) p.sched0.u[best_w][wave_n[best_w]] = word;
                else {
                    p.sched1.u[best_w - kWaves][wave_n[best_w]] = word;
                    p.owner |= 1u << u;
                }
                ++wave_n[best_w];
                wave_load[best_w] += size;
                simd_load[bin(best_w)] += size;
            }
    }
    p.x_in_lds = bytes(JC, 0, 1) <= kFecoLdsMax;
    p.fast_lists = F <= kFecoThreads && bytes(JC, 1, p.x_in_lds) <= kFecoLdsMax;
    p.lds = bytes(JC, p.fast_lists, p.x_in_lds);
    return p;
}

// FeCo (k_feco.hip).  What sg_feco_kmeans_compress(_rows) refuses about a (B, reps) grid of F x D clusterings into k groups,
// said without a launch: SG_OK or SG_ERR_ARG with the error text set
int feco_kmeans_check(sg_ctx* ctx, int B, int F, int D, int k, int max_iter, int reps);
// the two-CU exchange buffers of the k-means (ctx->feco_xchg / feco_flags), allocated and cleared on first use: a loop calls
// this before its first pass so that no pass allocates; false = no room (the launches then run one block per instance)
bool feco_pair_buffers(sg_ctx* ctx);
// sg_feco_compress_backward_reps with the sum started from `carry` (B, F, D) -- the repeats of earlier passes, ((carry + g0) +
// g1) + ... -- when it is not null; carry may alias dfeats
hipError_t launch_feco_bwd_reps(const float* dout, const int* assign, const int* counts, int B, int F, int D, int k, int force,
                                int R, const float* carry, float* dfeats, hipStream_t s);

hipError_t launch_loss_eval(const float* scores, const int64_t* y, int B, int S, float threshold, const sg_loss_spec& ls,
                            int64_t* dec, float* loss, float* dscores, hipStream_t s);
// per-step records of a step that ran R EOT repeats (rows r * B + b): loss_out[b] = mean over the repeats, dec_out[b] = the
// majority vote with first-seen tie-break (attack/FGSM.py:50-58, attack/utils.py:118-125 Counter.most_common)
hipError_t launch_eot_trace_reduce(const float* loss_rows, const int64_t* dec_rows, int R, int B, float* loss_out,
                                   int64_t* dec_out, hipStream_t s);

// The network's head (max over time, fc, decision, loss, d loss / d conv8: what an_tail_kernel does in a launch of its own)
// inside the fused backward launch: every block computes it for its utterance from act[6] -- a few microseconds of a
// block's ~80-160 -- and slice 0 writes the per-utterance outputs.  Same arithmetic in the same order as an_tail_kernel.
struct AnHeadArgs {
    int on;                    // 0: d loss / d conv8 comes from AnFusedArgs::dtop
    const float* fc_w;         // (S, 32)
    const float* fc_b;
    int S;
    float threshold;
    const int64_t* y;          // (rows)
    sg_loss_spec ls;
    int coef_rows;
    float* emb_out; float* scores_out; int64_t* dec_out; float* loss_out;   // optional, per row
    float* loss_trace; int64_t* dec_trace; uint8_t* success;                 // optional, per row
};

// the AudioNet CNN of one pass in one launch per direction (k_audionet_fused.hip), or -- whole utterances per block, S = 1 --
// forward, head and backward in ONE launch (launch_an_cnn_fwdbwd)
struct AnFusedArgs {
    // forward
    const float* feats;        // (rows, Fnet, 32)
    float* pre;                // (rows, Fnet, 32)
    float* act[kAnConv];       // (rows, Tout, Cout) ReLU outputs
    float* pool[kAnConv];      // (rows, Tout / 2, Cout) where the block has a MaxPool
    const float* wq[kAnConv];  // k4-packed weights of the direction: [3 K / 4][N][4]
    const float* wq_bwd[kAnConv];  // the data gradients' weights when one launch runs both directions
    const float* bias[kAnConv];
    const float* w25;
    float pre_bias;
    // backward
    const float* dtop;         // (rows, Tout[6], 32) d loss / d conv8 pre-activation
    float* dfeats;             // (rows, Fnet, 32)
    int Fnet, S, buf_floats;
    int Tin[kAnConv], Tout[kAnConv];
    unsigned long long* trace;  // tuning aid (SG_AN_TRACE): per block 16 timestamps (100 MHz) at the stage boundaries, or null
    AnHeadArgs head;
};
// Which launches run the CNN of one pass.  Knobs (behind SG_TUNE=1, read once per entry-point call: the tests flip them):
// SG_AN_FUSED=0: the per-layer launch sequence of rounds 1-3, the fused kernels' bit-exact counterpart; SG_AN_HEAD=0: the
// head as a separate an_tail launch; SG_AN_ONE=1: forward + head + backward as one launch where whole utterances fit a
// block; SG_AN_SLICES=n: n time slices per utterance instead of the planner's choice (same bits for any cut).
struct AnKnobs {
    bool fused = true, head = true, one = false;
    int slices = 0;
};
enum AnForm {
    AN_PER_LAYER,   // prefilter, 7 contractions, pools; an_tail; the same backwards
    AN_FUSED_TAIL,  // an_cnn_fwd, an_tail, an_cnn_bwd
    AN_FUSED_HEAD,  // an_cnn_fwd, an_cnn_bwd with the head inside (a gradient follows: no an_tail, no d conv8 round trip)
    AN_ONE_LAUNCH,  // an_cnn_fwdbwd: whole utterances per block (S = 1)
};
struct AnNetPlan {
    bool frames_ok;                   // enough frames for the stack (an_layer_frames)
    int Fnet;                         // frames the network sees
    int Tin[kAnConv], Tout[kAnConv];
    AnForm form;
    int S;                            // time slices per utterance (fused forms)
    int buf_floats;                   // floats per LDS buffer: forward, and backward fed by an_tail
    int buf_floats_head;              // ... of a launch with the head inside (its scratch lives in the second buffer)
    bool small;                       // S >= 3: the kernels built for one 32-row tile per wave
};
// Pure: the whole decision from its arguments.  device_ok: the device grants the fused kernels their dynamic LDS
// (an_fused_device_ok).  want_grad: a backward follows the head.
AnNetPlan an_net_plan(const AnKnobs& knobs, int rows, int Fnet, int num_cus, bool device_ok, bool want_grad);
// the > 64 KB dynamic-LDS opt-in of the fused kernels, made once per device; false: the device refuses it
bool an_fused_device_ok();
// S, buf_floats and the kernel build come from the plan; hipErrorNotSupported if the plan is not a fused form
hipError_t launch_an_cnn_fused(AnFusedArgs a, const AnNetPlan& plan, int rows, bool backward, hipStream_t s);
// forward + head + backward of whole utterances in one launch; hipErrorNotSupported unless the plan says AN_ONE_LAUNCH
hipError_t launch_an_cnn_fwdbwd(AnFusedArgs a, const AnNetPlan& plan, int rows, hipStream_t s);
hipError_t launch_an_logmel_fwd(const AnTables& t, const float* x, int B, int T, int F, const float* scale, float* feats,
                                int fft32, hipStream_t s);
hipError_t launch_an_logmel_bwd(const AnTables& t, const float* x, int B, int T, int F, const float* scale,
                                const float* dfeats, float* dframes, int fft32, hipStream_t s);
// the adjoint with the overlap-add (+ update) inside: needs t.mel_cache of the same pass; x_out != x_in
hipError_t launch_an_logmel_bwd_ola(const AnTables& t, AnOlaArgs a, int fft32, int num_cus, hipStream_t s);
bool an_ola_pays(int B, int F, int fft32, int num_cus);
hipError_t launch_an_frames_to_wave(const float* dframes, int B, int T, int F, const float* scale, float* grad_out,
                                    float* x_io, const float* lower, const float* upper, float step, int grad_sign,
                                    hipStream_t s);
hipError_t launch_an_prefilter(const float* in, float* out, int B, int T, const float* w25, float bias, int transpose,
                               hipStream_t s);
hipError_t launch_an_pool_fwd(const float* in, float* out, int B, int Tin, int C, hipStream_t s);
hipError_t launch_an_pool_bwd(const float* act, const float* dpool, float* dact, int B, int Tin, int C, hipStream_t s);
hipError_t launch_an_tail(const float* act8, int B, int T8, const float* fc_w, const float* fc_b, int S, float threshold,
                          const int64_t* y, const sg_loss_spec& ls, int want_grad, float* emb, float* scores,
                          int64_t* decisions, float* loss, float* dact8, float* loss_trace, int64_t* dec_trace,
                          uint8_t* success, hipStream_t s, int coef_rows = 0);

struct TailArgs {
    const float* fc1_part; int nsplit; int B;
    const XvModel* m;  // host struct with device pointers (copied by value into the launch)
    const int64_t* y; sg_loss_spec loss; int want_grad;
    float* tdnn_emb; float* emb; float* scores; int64_t* decisions; float* loss_out; float* demb;
    // optional per-pass records for the fused loop
    float* loss_trace; int64_t* decision_trace; uint8_t* success;
    int coef_rows;  // SG_LOSS_LINEAR: rows of the caller's coef table (0: B); rows of batched EOT repeats wrap (row % coef_rows)
};
hipError_t launch_tail(const TailArgs& a, hipStream_t s);

}  // namespace sg
