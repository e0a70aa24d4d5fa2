// Text shared by the kernels of k_mfcc.hip for uniform batches and their counterparts for batches of unequal lengths
// (*_ragged_kernel).  Included INSIDE a kernel, once per use, with SG_MFCC_BODY naming the piece: textual on purpose -- the
// uniform kernels stay, token for token, what they were before the second user existed, so they compile to the same code (a
// function shared across the two changed their instruction selection), and the two users cannot drift apart.  Every name a
// piece reads is a parameter or a local of the including kernel.
#if SG_MFCC_BODY == 1
// ---- one frame of the MFCC adjoint, inside the frame loop of mfcc_bwd_kernel / mfcc_bwd_ragged_kernel (frame f of row b, its
//      samples in raw): the forward of the frame (or its cached spectrum), then the stages in reverse, down to dframes
        FrameState st;
        float cep;
        cx<R> Xk[4];
        frame_forward<R, CACHED ? 1 : 0, DZ>(t, tb, tz, L, raw, F, b, f, scale, dz, lane, st, cep, Xk);
        // ---- cepstra -> log-mel
        float dc = 0.f;
        if (lane < kCep) dc = dfeats[((size_t)b * F + f) * ld + lane];
        const float denergy = __shfl(dc, 0, 64);
        if (lane < 32) L.tmp[lane] = (lane == 0 || lane >= kCep) ? 0.f : dc * tb.lifter[lane];
        wave_sync();
        if (lane < 32) {
            float dm = 0.f;
            if (lane < kMel) {
                float dl = 0.f;
#pragma unroll
                for (int c = 0; c < kCep; ++c) dl = __builtin_fmaf(L.tmp[c], tb.dct_t[tz + c * 32 + lane], dl);
                const float mel = L.mel[lane];
                dm = mel > kEps ? dl / mel : 0.f;
            }
            L.lmel[lane] = dm;  // d loss / d mel energy (entries 30,31 = 0)
        }
        wave_sync();
        // ---- mel -> power -> spectrum gradient G[k] = 2 X[k] dP[k] at this lane's bins, in transform order -- the layout the
        //      TRANSPOSED inverse network takes (d >= 4: bins 256..511, zero); it returns samples lane + 64 j in registers.
        cx<R> v[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            v[d] = cmk<R>((R)0, (R)0);
            const int m0 = bin_m0[d];
            if (m0 >= 0) {
                const R dp = (R)(2.f * __builtin_fmaf(L.lmel[m0], bin_w0[d], L.lmel[m0 + 1] * bin_w1[d]));
                v[d] = cmk<R>(Xk[d].x * dp, Xk[d].y * dp);
            }
        }
#pragma unroll
        for (int d = 4; d < 8; ++d) v[d] = cmk<R>((R)0, (R)0);
        fft512T_transposed<R>(L.spec, tb.tw1c() + tz, tb.tw2c() + tz, lane, (R)1, v);
        // ---- window, pre-emphasis (sample n + 1 is the right neighbour lane's, lane 63: lane 0's next register), energy,
        //      DC removal
        float sw[8];
#pragma unroll
        for (int i = 0; i < 7; ++i) sw[i] = (float)v[i].x * tb.window[tz + lane + 64 * i];
        sw[7] = 0.f;
        float ds[7];
        float sum = 0.f;
        const float einv = st.energy > kEps ? 2.f * denergy / st.energy : 0.f;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int n = lane + 64 * i;
            const float edge = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sw[i + 1]), 0));
            const float next = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, sw[i]),
                                                                                      0x130 /* wave_shl:1 */, 0xf, 0xf, false));
            float g = 0.f;
            if (n < kWin) {
                g = sw[i] - 0.97f * next;  // (sample 400 does not exist: its sw is 0)
                if (n == 0) g -= 0.97f * sw[0];
                g = __builtin_fmaf(einv, st.s[i], g);
            }
            ds[i] = g;
            sum += g;
        }
        const float mean = wave_sum_rows(sum) / (float)kWin;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int n = lane + 64 * i;
            if (n < kWin) dframes[((size_t)b * F + f) * kWin + n] = (ds[i] - mean) * scale;
        }
#elif SG_MFCC_BODY == 2
// ---- the overlap-add (+ update) of one thread, the whole body of frames_to_wave_kernel / frames_to_wave_ragged_kernel:
//      utterance blockIdx.y has T samples and F frames, in buffers whose rows are SG_OLA_TLD samples / SG_OLA_FLD frames apart
    // acc_in (may alias grad_out): gradient accumulated over the earlier EOT repeats of this step (EOT.py:41-47)
    // V = 4: a thread owns four consecutive samples n0 .. n0 + 3 (n0 a multiple of 4; host: T % 4 == 0).  Away from the
    // reflected edges the four share their frames (frame shift and window are multiples of 4), so every gather is one aligned
    // 16-byte load and the per-sample sums keep their order; a thread whose samples touch an edge takes them one by one.
    const int n0 = (blockIdx.x * 256 + threadIdx.x) * V;
    const int b = blockIdx.y;
    if (n0 >= T) return;
    constexpr int kPad = kWin / 2 - kShift / 2;
    const int last_q = (F - 1) * kShift - kPad + kWin - 1;  // the largest original position a frame covers
    const size_t o = (size_t)b * SG_OLA_TLD + n0;
    float total[V];
    const bool interior = V == 4 && n0 >= kPad && 2 * T - 1 - (n0 + 3) > last_q && n0 + 3 < T;
    // dframes (R, B, F, 400): R batched EOT repeats of the B utterances; their gradients are summed in repeat order,
    // exactly as R sequential passes handing the sum on through acc_in did (EOT.py:41-47)
    if (interior) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const int q = n0 + kPad;
        int fhi = q / kShift;
        const int flo = q > kWin - 1 ? (q - (kWin - 1) + kShift - 1) / kShift : 0;
        if (fhi > F - 1) fhi = F - 1;
        f4 tot = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < R; ++r) {
            const float* df = dframes + ((size_t)r * B + b) * SG_OLA_FLD * kWin;
            f4 g = {0.f, 0.f, 0.f, 0.f};
            for (int f = flo; f <= fhi; ++f) g += *reinterpret_cast<const f4*>(df + (size_t)f * kWin + (q - f * kShift));
            if (r == 0) tot = acc_in ? *reinterpret_cast<const f4*>(acc_in + o) + g : g;
            else tot = tot + g;
        }
        total[0] = tot.x;
        if (V == 4) { total[1] = tot.y; total[2] = tot.z; total[3] = tot.w; }
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int n = n0 + v;
            total[v] = 0.f;
            if (n >= T) continue;
            const int pr = 2 * T - 1 - n;
            for (int r = 0; r < R; ++r) {
                const float* df = dframes + ((size_t)r * B + b) * SG_OLA_FLD * kWin;
                float g = 0.f;
                auto add_pos = [&](int p) {
                    const int q = p + kPad;  // position in the padded signal, >= 0
                    int fhi = q / kShift;
                    int flo = q > kWin - 1 ? (q - (kWin - 1) + kShift - 1) / kShift : 0;
                    if (fhi > F - 1) fhi = F - 1;
                    for (int f = flo; f <= fhi; ++f) g += df[(size_t)f * kWin + (q - f * kShift)];
                };
                add_pos(n);
                if (n < kPad) add_pos(-n - 1);
                if (pr <= last_q) add_pos(pr);
                if (r == 0) total[v] = acc_in ? acc_in[o + v] + g : g;
                else total[v] = total[v] + g;
            }
        }
    }
    if (V == 4 && n0 + 3 < T) {  // (T % 4 == 0: always, for V = 4) the update as 16-byte accesses
        typedef float f4 __attribute__((ext_vector_type(4)));
        if (grad_out) *reinterpret_cast<f4*>(grad_out + o) = f4{total[0], total[V > 1 ? 1 : 0], total[V > 2 ? 2 : 0], total[V > 3 ? 3 : 0]};
        if (x_io) {
            const f4 xv = *reinterpret_cast<const f4*>(x_io + o), lo = *reinterpret_cast<const f4*>(lower + o),
                     hi = *reinterpret_cast<const f4*>(upper + o);
            f4 res;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float g = total[v < V ? v : 0];
                const float sg = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);
                res[v] = fminf(fmaxf(xv[v] + step * sg * (float)grad_sign, lo[v]), hi[v]);
            }
            *reinterpret_cast<f4*>(x_io + o) = res;
        }
        return;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if (n0 + v >= T) break;
        const float g = total[v];
        if (grad_out) grad_out[o + v] = g;
        if (x_io) {
            const float sg = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);
            float val = x_io[o + v] + step * sg * (float)grad_sign;
            val = fminf(fmaxf(val, lower[o + v]), upper[o + v]);
            x_io[o + v] = val;
        }
    }
#endif
#undef SG_MFCC_BODY
