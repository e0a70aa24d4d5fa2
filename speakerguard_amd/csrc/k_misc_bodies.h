// Text shared by the CMVN and pooling kernels of k_misc.hip for uniform batches and their counterparts for batches of unequal
// lengths (*_ragged_kernel).  Included INSIDE a kernel with SG_MISC_BODY naming the piece: textual on purpose -- the uniform
// kernels stay, token for token, what they were before the second user existed, so they compile to the same code, and the two
// users cannot drift apart.  Every name a piece reads is a parameter or a local of the including kernel; the frame counts (F,
// Tc) are the UTTERANCE's, the including kernel has applied the row stride to its pointers.
#if SG_MISC_BODY == 1
// ---- CMVN forward of one utterance by the whole block: x (F, ld_in) -> y (F, ld_out)
    __shared__ double total[kCep];
    __shared__ double part[kCmvnParts][32];
    if (F <= kCmnWindow) {
        // every window is the whole utterance: one column sum per cepstrum, 32 row-strided partial sums per column
        // combined in a fixed order.  Thread (column d, row class r) keeps its <= 10 values (rows r, r + 32, ...) in
        // registers -- loaded in one batch of independent, clamped loads -- and writes the same elements back: one global
        // round trip and two barriers, where the first version read the utterance twice (9.1 -> see profiles/).
        constexpr int kRows = (kCmnWindow + kCmvnParts - 1) / kCmvnParts;
        const int d = threadIdx.x & 31, r = threadIdx.x >> 5;
        float v[kRows];
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int t = min(r + j * kCmvnParts, F - 1);
            v[j] = d < kCep ? x[(size_t)t * ld_in + d] : 0.f;
        }
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kRows; ++j)
            if (r + j * kCmvnParts < F) acc += (double)v[j];
        part[r][d] = acc;
        __syncthreads();
        if (threadIdx.x < kCep) {
            double a2 = 0.0;
            for (int rr = 0; rr < kCmvnParts; ++rr) a2 += part[rr][threadIdx.x];
            total[threadIdx.x] = a2;
        }
        __syncthreads();
        const float mean = d < kCep ? (float)(total[d] / (double)F) : 0.f;
        if (d < ld_out) {
#pragma unroll
            for (int j = 0; j < kRows; ++j) {
                const int t = r + j * kCmvnParts;
                if (t < F) y[(size_t)t * ld_out + d] = d < kCep ? v[j] - mean : 0.f;
            }
        }
        for (int i = threadIdx.x; i < F * (ld_out - 32); i += kCmvnThreads) {  // (row stride above 32: the rest of the zero padding)
            const int t = i / (ld_out - 32), dd = 32 + i - t * (ld_out - 32);
            y[(size_t)t * ld_out + dd] = 0.f;
        }
    } else {
        for (int i = threadIdx.x; i < F * ld_out; i += kCmvnThreads) {
            const int t = i / ld_out, d = i - t * ld_out;
            float v = 0.f;
            if (d < kCep) {
                int s, e;
                cmvn_window(t, F, s, e);
                double acc = 0.0;
                for (int u = s; u < e; ++u) acc += (double)x[(size_t)u * ld_in + d];
                v = x[(size_t)t * ld_in + d] - (float)(acc / (double)(e - s));
            }
            y[i] = v;
        }
    }
#elif SG_MISC_BODY == 2
// ---- CMVN backward of one utterance: g (slabs of (F, ld_dout), slab_stride apart) -> y (F, ld_din)
    const int nsplit = NS > 0 ? NS : nsplit_rt;
    auto gsum = [&](int t, int d) __attribute__((always_inline)) {
        const float* src = g + (size_t)t * ld_dout + d;
        if (NS > 0) {
            float part[NS > 0 ? NS : 1];
#pragma unroll
            for (int z = 0; z < NS; ++z) part[z] = src[(size_t)z * slab_stride];
            float v = 0.f;
#pragma unroll
            for (int z = 0; z < NS; ++z) v += part[z];
            return v;
        }
        float v = 0.f;
#pragma unroll 5
        for (int z = 0; z < nsplit; ++z) v += src[(size_t)z * slab_stride];
        return v;
    };
    __shared__ double total[kCep];
    __shared__ double part[kCmvnParts][32];
    if (F <= kCmnWindow) {
        // thread (column d, row class r): the slab sums of its <= 10 rows stay in registers (kRows x nsplit independent
        // loads, slabs added in order), the column means come from the same row-strided partial sums as before
        constexpr int kRows = (kCmnWindow + kCmvnParts - 1) / kCmvnParts;
        const int d = threadIdx.x & 31, r = threadIdx.x >> 5;
        float v[kRows];
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int t = min(r + j * kCmvnParts, F - 1);
            v[j] = d < kCep ? gsum(t, d) : 0.f;
        }
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kRows; ++j)
            if (r + j * kCmvnParts < F) acc += (double)v[j];
        part[r][d] = acc;
        __syncthreads();
        if (threadIdx.x < kCep) {
            double a2 = 0.0;
            for (int rr = 0; rr < kCmvnParts; ++rr) a2 += part[rr][threadIdx.x];
            total[threadIdx.x] = a2 / (double)F;
        }
        __syncthreads();
        if (d < kCep) {
            const float mean = (float)total[d];
#pragma unroll
            for (int j = 0; j < kRows; ++j) {
                const int t = r + j * kCmvnParts;
                if (t < F) y[(size_t)t * ld_din + d] = v[j] - mean;
            }
        }
    } else {
        for (int i = threadIdx.x; i < F * kCep; i += kCmvnThreads) {
            const int u = i / kCep, d = i - u * kCep;
            double acc = 0.0;
            for (int t = 0; t < F; ++t) {
                int s, e;
                cmvn_window(t, F, s, e);
                if (u >= s && u < e) acc += (double)gsum(t, d) / (double)(e - s);
            }
            y[(size_t)u * ld_din + d] = gsum(u, d) - (float)acc;
        }
    }
#elif SG_MISC_BODY == 3
// ---- pooling forward: channel c of utterance b over its Tc frames, a = its first frame; the block's 4 waves split the frames
    __shared__ float red[4][64];
    // two-pass variance (like torch.std); the <= 96 frames a wave owns stay in registers between the
    // passes so the activation tensor is read once (longer utterances re-read from L2)
    constexpr int kKeep = 96;
    float keep[kKeep];
    const bool fits = Tc <= 4 * kKeep;
    float s = 0.f;
    if (fits) {
#pragma unroll
        for (int i = 0; i < kKeep; ++i) {
            const int t = wid + 4 * i;
            keep[i] = t < Tc ? a[(size_t)t * kPoolC] : 0.f;
            s += keep[i];
        }
    } else {
        for (int t = wid; t < Tc; t += 4) s += a[(size_t)t * kPoolC];
    }
    red[wid][lane] = s;
    __syncthreads();
    const float mean = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)Tc;
    __syncthreads();
    float q = 0.f;
    if (fits) {
#pragma unroll
        for (int i = 0; i < kKeep; ++i) {
            const float d = keep[i] - mean;
            q += (wid + 4 * i < Tc) ? d * d : 0.f;
        }
    } else {
        for (int t = wid; t < Tc; t += 4) {
            const float d = a[(size_t)t * kPoolC] - mean;
            q += d * d;
        }
    }
    red[wid][lane] = q;
    __syncthreads();
    if (wid == 0) {
        const float var = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)(Tc - 1);
        stats[(size_t)b * kStats + c] = mean;
        stats[(size_t)b * kStats + kPoolC + c] = sqrtf(var);
    }
#elif SG_MISC_BODY == 4
// ---- pooling backward: mean, alpha, beta of d act[t][c] = v > 0 ? alpha + beta (v - mean) : 0 for an utterance pooled over Tc frames
    float dmean = 0.f, dstd = 0.f;
    if (NS > 0) {
        float pm[NS > 0 ? NS : 1], ps[NS > 0 ? NS : 1];
#pragma unroll
        for (int z = 0; z < NS; ++z) {
            pm[z] = dpart[((size_t)z * B + b) * kStats + c];
            ps[z] = dpart[((size_t)z * B + b) * kStats + kPoolC + c];
        }
#pragma unroll
        for (int z = 0; z < NS; ++z) {
            dmean += pm[z];
            dstd += ps[z];
        }
    } else {
        for (int z = 0; z < nsplit; ++z) {
            dmean += dpart[((size_t)z * B + b) * kStats + c];
            dstd += dpart[((size_t)z * B + b) * kStats + kPoolC + c];
        }
    }
    const float mean = stats[(size_t)b * kStats + c];
    const float sd = stats[(size_t)b * kStats + kPoolC + c];
    const float beta = sd > 0.f ? dstd / ((float)(Tc - 1) * sd) : 0.f;
    const float alpha = dmean / (float)Tc;
#endif
#undef SG_MISC_BODY
