// One 1024-thread block per (utterance, repeat).  Round 1 kept frames and centroids in LDS and gave every thread a frame
// whose D floats it re-read from LDS for every centroid (3.1 ms per call at 64 x 300 x 32); rounds 2-4 kept a thread's
// frame in registers and measured it against centroid pairs with packed fp32 sub / mul / add -- the contract then was the
// literal sum of squared differences, 3 lane-operations per (frame, centroid, dimension), VALU-bound on the one CU an
// instance gets: 23.5 us per assignment step at 300 x 150 x 32, 198 us per call (35 % of a PGD step against the
// FeCo-defended AudioNet).  Round 5 (contract version 2 above):
//   * the assignment is the contraction x' c^T on v_mfma_f32_32x32x2_f32 (A = 32 centroids, B = 32 frames, the accumulators
//     start at h_j): one fused multiply-add per (frame, centroid, dimension) on the matrix pipes, 50 tile pairs x 16
//     MFMAs = 5.3 us of the CU's four pipes at 300 x 150 x 32.  A unit of work is (frame tile, chunk of centroid tiles), dealt
//     round-robin to the 16 waves; a lane keeps the running maximum of its 16 accumulator rows (ascending centroid, strict
//     >), the two lane halves and then the chunks are merged in ascending centroid order: the lowest index wins ties;
//   * operands come from LDS images whose 16-byte slots are XOR-permuted per row (conflict-free ds_read_b128; the k order
//     0, 4, 1, 5, ... is what a lane half reading four consecutive dimensions per group gives);
//   * member lists: per-64-frame-chunk counts by LDS atomics, a frame's rank inside its chunk by 64 v_readlane compares
//     (was: every frame scanning all earlier ids, 5.6 us) -> ascending frame order inside a cluster by construction;
//   * the update walks the member lists (LDS) and refreshes h_j with a butterfly over the lanes that hold the row;
//   * the cluster means the reference takes next (feature_level.py:204-216) are the means of the ORIGINAL frames over the
//     final lists -- same ids, same ascending sums, same division as feco_compress_kernel -- handed out by the kernel.
//
// COS (the "cosine" contract of k_feco.hip's header): the same block with raw frames for x', unit centroids for c and
// h_j = 0 -- the centring is skipped, the update normalises a mean before it stores it.
//
// This text is included by k_feco.hip ONCE PER METRIC, with FECO_KMEANS_KERNEL (the kernel template's name) and
// FECO_KMEANS_COS (false / true) defined: feco_kmeans_kernel<DPAD> and feco_kmeans_cos_kernel<DPAD>.  Two kernel templates
// from one text, so that the L2 kernels keep their names (the launch sequences name them) and their code, instruction for
// instruction: every `if constexpr (COS)` leaves the L2 path what it was, whereas one __device__ body behind two thin kernels
// moved the L2 code (the by-value tables reach an inlined body another way).
template <int DPAD>
__global__ __launch_bounds__(kFecoThreads) void FECO_KMEANS_KERNEL(const float* __restrict__ feats, int F, int D, int k,
                                                                   int max_iter, int seeded, int row_wise, uint64_t seed,
                                                                   int64_t index_base, int x_in_lds, int fast_lists, int JC, FecoSched sched,
                                                                   FecoPair pr, int* __restrict__ assign, float* __restrict__ out,
                                                                   int* __restrict__ counts) {
    constexpr bool COS = FECO_KMEANS_COS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FecoLds L = feco_layout(F, k, DPAD, JC, fast_lists, x_in_lds);
    const int kp = (k + 31) & ~31;
    float* cq = lds + L.cq;
    float* hq = lds + L.hq;
    float* mu = lds + L.mu;
    float* part = lds + L.part;
    int* ids = reinterpret_cast<int*>(lds + L.ids);
    int* cnt = reinterpret_cast<int*>(lds + L.cnt);
    int* start = reinterpret_cast<int*>(lds + L.start);
    int* members = reinterpret_cast<int*>(lds + L.members);
    int* cw = reinterpret_cast<int*>(lds + L.cw);
    int* spart = reinterpret_cast<int*>(lds + L.spart);
    int* wtot = reinterpret_cast<int*>(lds + L.wtot);
    float* pd = lds + L.pd;
    int* pj = reinterpret_cast<int*>(lds + L.pj);
    float* xq = lds + L.xq;
    __shared__ int changed;
    int tid = threadIdx.x;
    int lane = tid & 63, lh = lane >> 5, ln = lane & 31;
    // COS: the thread's number made opaque at the head of a phase, so that the addresses the phases derive from it are
    // computed where they are used and not kept in registers across the whole loop (the L2 instantiations keep them, and
    // spill: the block has 128 registers per lane).  In the L2 instantiations it is empty and their code is what it was.
    auto fresh_tid = [&]() __attribute__((always_inline)) {
        if constexpr (COS) {
            asm volatile("" : "+v"(tid));
            tid &= kFecoThreads - 1;
            lane = tid & 63, lh = lane >> 5, ln = lane & 31;
        }
    };
    // blockIdx.y = repeat: the same utterances clustered again from other random frames (EOT over the defense); repeat r
    // uses key seed + r * kRepKey and writes slot r * gridDim.x + utterance of every output.  row_wise: the repeats
    // have features of their own (a dithered front-end in front of the defense) -- repeat r reads that slot too
    // Two CUs per instance: the grid's z dimension is the half.  (Blocks go to the 8 XCDs round robin by linear index: with
    // the instances a multiple of 8 the two halves share an XCD -- a speed assumption only.  Halves as neighbours in x --
    // different XCDs -- measured 97 us per call against 90; x and x ^ 8 -- same XCD, dispatched together -- 92.)
    const int half = pr.on ? (int)blockIdx.z : 0;
    const int bx = (int)blockIdx.x, nbx = (int)gridDim.x;
    const size_t slot = (size_t)blockIdx.y * nbx + bx;
    const float* x = feats + (row_wise ? slot : (size_t)bx) * F * D;
    __shared__ int pair_solo;
    if (tid == 0) pair_solo = 0;
    seed += (uint64_t)blockIdx.y * kRepKey;
    FECO_STAMP(4 * kFecoTraceIters + 2)
    for (int i = tid; i < al4(F); i += kFecoThreads) ids[i] = -1;  // the pad entries stay -1: no cluster
    if (fast_lists)
        for (int e = tid; e < ((F + 63) >> 6) * k; e += kFecoThreads) cw[e] = 0;
    // the raw frames go to LDS first (one batch of coalesced loads), the centring reads them there
    if (x_in_lds) {
        for (int e = tid; e < F * DPAD; e += kFecoThreads) {
            const int i = e / DPAD, d = e - i * DPAD;
            xq[sw_at<DPAD>(i, d)] = d < D ? x[(size_t)i * D + d] : 0.f;
        }
        __syncthreads();
    }
    // centring: 16 interleaved partial sums per dimension, added up in order (COS: none -- the frames stay as they are)
    if constexpr (!COS) {
        for (int e = tid; e < 16 * DPAD; e += kFecoThreads) {
            const int q = e / DPAD, d = e - q * DPAD;
            float s = 0.f;
            if (d < D) {
                if (x_in_lds) {
#pragma unroll 8
                    for (int i = q; i < F; i += 16) s = s + xq[sw_at<DPAD>(i, d)];
                } else {
#pragma unroll 8
                    for (int i = q; i < F; i += 16) s = s + x[(size_t)i * D + d];
                }
            }
            part[e] = s;
        }
        __syncthreads();
        for (int d = tid; d < DPAD; d += kFecoThreads) {
            float t = part[d];
#pragma unroll
            for (int q = 1; q < 16; ++q) t = t + part[q * DPAD + d];
            mu[d] = d < D ? t / (float)F : 0.f;
        }
        __syncthreads();
    }
    FECO_DETAIL(0)
    FECO_CYCLES(20)
    if constexpr (!COS) {
        if (x_in_lds) {
            for (int e = tid; e < F * DPAD; e += kFecoThreads) {
                const int i = e / DPAD, d = e - i * DPAD;
                if (d < D) xq[sw_at<DPAD>(i, d)] = xq[sw_at<DPAD>(i, d)] - mu[d];
            }
            __syncthreads();
        }
    }
    // element d of centred frame i (pad dimensions are zero); COS: of the frame itself
    auto xc_at = [&](int i, int d) __attribute__((always_inline)) -> float {
        if (x_in_lds) return xq[sw_at<DPAD>(i, d)];
        if constexpr (COS) return d < D ? x[(size_t)i * D + d] : 0.f;
        return d < D ? x[(size_t)i * D + d] - mu[d] : 0.f;
    };
    // COS: what a centroid row stores for its mean v -- v / sqrtf(n), n = the butterfly sum of the rounded squares over the
    // row's DPAD lanes, 0 where n is 0.  Every lane of the row holds the same bits of n: fp32 addition is commutative, so the
    // two lanes a butterfly step pairs compute the same sum, and by induction a group of 2, 4, ... DPAD lanes holds one value
    // (the mirrors of row_tree_sum pair the same quads as the steps 4 and 8) -- no broadcast from lane d = 0.
    auto unit_row = [&](float v) __attribute__((always_inline)) -> float {
        const float n = row_tree_sum<DPAD>(v * v);
        return n > 0.f ? v / sqrtf(n) : 0.f;
    };
    FECO_DETAIL(1)
    if (seeded) {
        // random initialisation: rank the frames by (key, frame); `members` holds the keys, `cnt` the k chosen frames
        // (both are free until the first update)
        unsigned* keys = reinterpret_cast<unsigned*>(members);
        int* chosen = cnt;
        const int64_t utt = index_base + bx;
        for (int i = tid; i < al4(F); i += kFecoThreads)
            keys[i] = i < F ? philox4x32_10_w0(seed, (uint32_t)i, 0u, (uint32_t)utt, (uint32_t)((uint64_t)utt >> 32)) : 0xFFFFFFFFu;
        __syncthreads();
        // rank of frame i = number of (key, frame) pairs below its own; the scan of the keys is shared by `parts` threads
        // per frame (partial ranks meet in `ids`, which is not in use yet)
        const int parts = F >= kFecoThreads ? 1 : kFecoThreads / F;
        const int nq = al4(F) / 4, per = (nq + parts - 1) / parts;
        for (int i = tid; i < F; i += kFecoThreads) ids[i] = 0;
        __syncthreads();
        for (int t0 = tid; t0 < F * parts; t0 += kFecoThreads) {
            const int i = t0 % F, pt = t0 / F;
            const unsigned ki = keys[i];
            int rank = 0;
            const int q0 = pt * per, q1 = min(nq, q0 + per);
#pragma unroll 4
            for (int q = q0; q < q1; ++q) {  // a pad key (all ones, index >= F) never counts as smaller
                const uint4 kg = *reinterpret_cast<const uint4*>(keys + 4 * q);
                const int g = 4 * q;
                rank += (kg.x < ki) || (kg.x == ki && g < i);
                rank += (kg.y < ki) || (kg.y == ki && g + 1 < i);
                rank += (kg.z < ki) || (kg.z == ki && g + 2 < i);
                rank += (kg.w < ki) || (kg.w == ki && g + 3 < i);
            }
            if (parts > 1) atomicAdd(&ids[i], rank);
            else ids[i] = rank;
        }
        __syncthreads();
        for (int i = tid; i < F; i += kFecoThreads) {
            const int rank = ids[i];
            if (rank < k) chosen[rank] = i;
            ids[i] = -1;
        }
        __syncthreads();
    }
    FECO_DETAIL(2)
    // initial centroids (centred) and their h; kp * DPAD is a multiple of the block: whole waves all the way
    for (int e = tid; e < kp * DPAD; e += kFecoThreads) {
        const int j = e / DPAD, d = e - j * DPAD;
        float v = 0.f;
        if (j < k && d < D) {
            const int f0 = seeded ? cnt[j] : (int)((long long)j * F / k);
            v = xc_at(f0, d);
        }
        if constexpr (COS) {
            cq[sw_at<DPAD>(j, d)] = unit_row(v);
            if (d == 0) hq[j] = j < k ? 0.f : -INFINITY;  // the chains start at 0.f for the whole call
        } else {
            cq[sw_at<DPAD>(j, d)] = v;
            const float sq = row_tree_sum<DPAD>(v * v);
            if (d == 0) hq[j] = j < k ? -0.5f * sq : -INFINITY;  // a pad row of the last tile never wins
        }
    }
    __syncthreads();
    const int ntf = (F + 31) >> 5, ntc = kp >> 5, nunits = ntf * JC;
    // B operand of frame tile ft: dimensions 8 g + 4 lh .. + 3 of this lane's frame (a column past the utterance is
    // computed and never used)
    auto load_b = [&](int ft, float4 (&xb)[DPAD / 8]) __attribute__((always_inline)) {
        const int frame = ft * 32 + ln;
        if (x_in_lds) {
            const int fr = min(frame, F - 1);
#pragma unroll
            for (int g = 0; g < DPAD / 8; ++g) xb[g] = *reinterpret_cast<const float4*>(xq + sw_slot<DPAD>(fr, 2 * g + lh));
        } else {
#pragma unroll
            for (int g = 0; g < DPAD / 8; ++g) {
                const int d0 = 8 * g + 4 * lh;
                const bool in = frame < F;
                if constexpr (COS) {
                    xb[g].x = in && d0 < D ? x[(size_t)frame * D + d0] : 0.f;
                    xb[g].y = in && d0 + 1 < D ? x[(size_t)frame * D + d0 + 1] : 0.f;
                    xb[g].z = in && d0 + 2 < D ? x[(size_t)frame * D + d0 + 2] : 0.f;
                    xb[g].w = in && d0 + 3 < D ? x[(size_t)frame * D + d0 + 3] : 0.f;
                } else {
                    xb[g].x = in && d0 < D ? x[(size_t)frame * D + d0] - mu[d0] : 0.f;
                    xb[g].y = in && d0 + 1 < D ? x[(size_t)frame * D + d0 + 1] - mu[d0 + 1] : 0.f;
                    xb[g].z = in && d0 + 2 < D ? x[(size_t)frame * D + d0 + 2] - mu[d0 + 2] : 0.f;
                    xb[g].w = in && d0 + 3 < D ? x[(size_t)frame * D + d0 + 3] - mu[d0 + 3] : 0.f;
                }
            }
        }
    };
    // scores of frame tile ft against centroid tiles [ct_lo, ct_hi): the lane's best (value, lowest index) -> chunk maxima /
    // ids (jc: the chunk's position inside the frame tile = its row of the merge arrays)
    auto run_unit = [&](int ft, int ct_lo, int ct_hi, int jc, const float4 (&xb)[DPAD / 8]) __attribute__((always_inline)) {
        const int frame = ft * 32 + ln;
        float best = -INFINITY;
        int bj = ct_lo * 32 + 4 * lh;
        for (int ct = ct_lo; ct < ct_hi; ++ct) {
            f32x16 acc;
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // accumulator row (r & 3) + 8 (r >> 2) + 4 lh = centroid of the tile
                const float4 hv = *reinterpret_cast<const float4*>(hq + ct * 32 + 8 * q + 4 * lh);
                acc[4 * q] = hv.x;
                acc[4 * q + 1] = hv.y;
                acc[4 * q + 2] = hv.z;
                acc[4 * q + 3] = hv.w;
            }
            const int row = ct * 32 + ln;
#ifdef SG_EXP_FECO_JC
            if (!(g_feco_ablate & 1))
#endif
#pragma unroll
            for (int g = 0; g < DPAD / 8; ++g) {
                const float4 a = *reinterpret_cast<const float4*>(cq + sw_slot<DPAD>(row, 2 * g + lh));
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xb[g].x, acc, 0, 0, 0);  // k = 8 g + 0, 8 g + 4
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xb[g].y, acc, 0, 0, 0);  //     8 g + 1, 8 g + 5
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xb[g].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xb[g].w, acc, 0, 0, 0);
            }
            // the tile's largest score of this lane, then the lowest row that reaches it; tiles ascending, strict >
            float tb = acc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) tb = fmaxf(tb, acc[r]);
            // (rows ascend with the register index: the last match of a descending walk is the lowest row)
            int rr = 0;
#pragma unroll
            for (int r = 15; r >= 0; --r) rr = acc[r] == tb ? r : rr;
            if (tb > best) {
                best = tb;
                bj = ct * 32 + 4 * lh + (rr & 3) + 8 * (rr >> 2);
            }
        }
        {  // the other half of the tile's rows sits in lane ^ 32
            const float ov = __shfl_xor(best, 32);
            const int oj = __shfl_xor(bj, 32);
            if (ov > best || (ov == best && oj < bj)) {
                best = ov;
                bj = oj;
            }
        }
        if (lh == 0 && frame < F) {
            if (JC > 1) {  // (the two-CU form needs JC > 1: host)
                pd[jc * F + frame] = best;
                pj[jc * F + frame] = bj;
            } else if (ids[frame] != bj) {
                ids[frame] = bj;
                changed = 1;
            }
        }
    };
    // (D > 32: two resident operands of 32 registers do not fit the 128 of a 1024-thread block -- round robin there)
    const bool table = DPAD == 32 && sched.table;
    float4 xb0[DPAD / 8], xb1[DPAD == 32 ? DPAD / 8 : 1];
    unsigned u0 = kFecoNoUnit, u1 = kFecoNoUnit;
    if constexpr (COS) {
        // the wave's row picked by constant indices: the tables are then read where they are, in the kernel's argument
        // segment (indexed by a variable, as the L2 instantiations do, both structs are copied to private memory first)
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        if (table) {
#pragma unroll
            for (int w = 0; w < kFecoThreads / 64; ++w)
                if (w == wv) {
                    u0 = half ? pr.sched1.u[w][0] : sched.u[w][0];
                    u1 = half ? pr.sched1.u[w][1] : sched.u[w][1];
                }
        }
    } else {
        u0 = table ? (half ? pr.sched1.u[tid >> 6][0] : sched.u[tid >> 6][0]) : kFecoNoUnit;
        u1 = table ? (half ? pr.sched1.u[tid >> 6][1] : sched.u[tid >> 6][1]) : kFecoNoUnit;
    }
    if (u0 != kFecoNoUnit) load_b(u0 & 255, xb0);
    if constexpr (DPAD == 32)
        if (u1 != kFecoNoUnit) load_b(u1 & 255, xb1);
    for (int it = 0; it < max_iter; ++it) {
        fresh_tid();
        if (it < kFecoTraceIters) { FECO_STAMP(4 * it) }
        if (tid == 0) changed = 0;
        __syncthreads();
        // ---- assignment on the matrix pipes.  A unit of work is (frame tile, chunk of its centroid tiles).  f32 MFMAs share
        // the SIMD's issue with the VALU instructions of the waves on it (round 3), so what has to balance is the SIMDs: the
        // host deals the units to the waves (waves w, w + 4, w + 8, w + 12 share a SIMD) and a wave keeps the B operands of
        // its (at most two) units in registers for the whole call; utterances with more than 32 units go round the waves.
        if (table) {
            if (u0 != kFecoNoUnit) run_unit(u0 & 255, (u0 >> 8) & 255, (u0 >> 16) & 255, u0 >> 24, xb0);
            if constexpr (DPAD == 32)
                if (u1 != kFecoNoUnit) run_unit(u1 & 255, (u1 >> 8) & 255, (u1 >> 16) & 255, u1 >> 24, xb1);
        } else {
            for (int u = tid >> 6; u < nunits; u += kFecoThreads / 64) {
                const int ft = u / JC, jc = u - ft * JC;
                load_b(ft, xb0);
                run_unit(ft, ntc * jc / JC, ntc * (jc + 1) / JC, jc, xb0);
            }
        }
        __syncthreads();
        if (it == 0) { FECO_DETAIL(3) }
        if (pr.on) {
            // ---- the partner's half of the chunk maxima (FecoPair above)
            const int nE = JC * F;
            bool have_theirs = false;
            if (!pair_solo) {
                const size_t buf = ((size_t)(slot * 2 + half) * 2 + (it & 1)) * kFecoMergeCap;
                const size_t buf_p = ((size_t)(slot * 2 + (half ^ 1)) * 2 + (it & 1)) * kFecoMergeCap;
                const unsigned long long tag = pr.tag0 + (unsigned)it + 1u;
                if (!(pr.drop && half == 1))
                    for (int r = tid; r < nE; r += kFecoThreads) {
                        const int jc = r / F, fr = r - jc * F;
                        if ((int)((pr.owner >> ((fr >> 5) * JC + jc)) & 1u) == half)
                            __hip_atomic_store(pr.xchg + buf + r,
                                               (unsigned long long)(unsigned)__float_as_int(pd[r]) | (unsigned long long)(unsigned)pj[r] << 32 | tag << 43,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                int bad = 0;
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                for (int r = tid; r < nE && !bad; r += kFecoThreads) {
                    const int jc = r / F, fr = r - jc * F;
                    if ((int)((pr.owner >> ((fr >> 5) * JC + jc)) & 1u) == half) continue;
                    for (;;) {
                        const unsigned long long v = __hip_atomic_load(pr.xchg + buf_p + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((v >> 43) == tag) {
                            pd[r] = __int_as_float((int)(unsigned)v);
                            pj[r] = (int)((v >> 32) & 0x7FFu);
                            break;
                        }
                        if (__builtin_amdgcn_s_memrealtime() - t0 > kFecoPairWait ||
                            __hip_atomic_load(pr.flags + slot * 2 + (half ^ 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pr.launch) {
                            bad = 1;  // not there in time, or the partner has said it went on alone
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                bad = __syncthreads_or(bad);
                if (bad) {
                    if (tid == 0) {
                        pair_solo = 1;
                        if (!(pr.drop && half == 1))
                            __hip_atomic_store(pr.flags + slot * 2 + half, pr.launch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                } else {
                    have_theirs = true;
                }
            }
            if (!have_theirs) {  // on its own: the partner's units, dealt round the waves; then this wave's operand again
                int n = 0;
                for (int u = 0; u < nunits; ++u) {
                    if ((int)((pr.owner >> u) & 1u) == half) continue;
                    if ((n++ & (kFecoThreads / 64 - 1)) != (tid >> 6)) continue;
                    const int ft = u / JC, jc = u - ft * JC;
                    load_b(ft, xb0);
                    run_unit(ft, ntc * jc / JC, ntc * (jc + 1) / JC, jc, xb0);
                }
                if (u0 != kFecoNoUnit) load_b(u0 & 255, xb0);
            }
            __syncthreads();
        }
        if (JC > 1) {
            for (int r = tid; r < F; r += kFecoThreads) {  // merge the chunks in ascending centroid order: the lowest index wins ties
                float b = pd[r];
                int bb = pj[r];
                for (int c = 1; c < JC; ++c) {
                    const float v = pd[c * F + r];
                    if (v > b) {
                        b = v;
                        bb = pj[c * F + r];
                    }
                }
                if (ids[r] != bb) {
                    ids[r] = bb;
                    changed = 1;
                }
            }
            __syncthreads();
        }
        if (it < kFecoTraceIters) { FECO_STAMP(4 * it + 1) }
        if (!changed) break;
        fresh_tid();
        // ---- member lists: frames grouped by cluster, ascending inside a cluster
        if (fast_lists) {
            // F <= 1024: one frame per thread, a wave holds the 64 frames of chunk tid >> 6.  Position of frame i in the
            // lists = frames of lower clusters + frames of its cluster in earlier chunks + earlier frames of its cluster
            // inside the wave (64 v_readlane compares).  Three block barriers.
            const int myid = tid < F ? ids[tid] : -1;
            int rank = 0;
#pragma unroll
            for (int l = 0; l < 64; ++l) rank += (__builtin_amdgcn_readlane(myid, l) == myid) & (l < lane);
            if (tid < F) atomicAdd(&cw[(tid >> 6) * k + myid], 1);  // cw is all zero here (start of the kernel / the last update)
            __syncthreads();
            if (it == 0) { FECO_DETAIL(4) }
            const int nch = (F + 63) >> 6;
            {   // cluster tid: its size, and (inclusive scan inside the wave) the frames of the wave's lower clusters
                int c = 0;
                if (tid < k)
                    for (int ch = 0; ch < nch; ++ch) c += cw[ch * k + tid];
                int incl = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int t = __shfl_up(incl, o);
                    if (lane >= o) incl += t;
                }
                if (tid < k) {
                    cnt[tid] = c;
                    spart[tid] = incl - c;
                }
                if (lane == 63) wtot[tid >> 6] = incl;
            }
            __syncthreads();
            if (it == 0) { FECO_DETAIL(5) }
            if (tid < F) {
                int pos = spart[myid] + rank;
                for (int w = 0; w < (myid >> 6); ++w) pos += wtot[w];
                for (int ch = 0; ch < (tid >> 6); ++ch) pos += cw[ch * k + myid];
                members[pos] = tid;
            }
            if (tid < k) {
                int st = spart[tid];
                for (int w = 0; w < (tid >> 6); ++w) st += wtot[w];
                start[tid] = st;
            }
            __syncthreads();
            if (it == 0) { FECO_DETAIL(6) }
            // zero the chunk counts for the next iteration (their next use is behind the update's barrier)
            for (int e = tid; e < nch * k; e += kFecoThreads) cw[e] = 0;
        } else {
            for (int j = tid; j < k; j += kFecoThreads) cnt[j] = 0;
            __syncthreads();
            for (int i = tid; i < F; i += kFecoThreads) atomicAdd(&cnt[ids[i]], 1);
            __syncthreads();
            // offsets: cluster j adds up the counts below it (16-byte broadcast reads)
            for (int j = tid; j <= k; j += kFecoThreads) {
                int run = 0;
                const int j4 = j & ~3;
                for (int q = 0; q < j4; q += 4) {
                    const int4 c = *reinterpret_cast<const int4*>(cnt + q);
                    run += c.x + c.y + c.z + c.w;
                }
                for (int q = j4; q < j; ++q) run += cnt[q];
                start[j] = run;
            }
            __syncthreads();
            // slots: frame i goes behind the earlier frames of its cluster
            for (int i = tid; i < F; i += kFecoThreads) {
                const int j = ids[i];
                int pos = 0;
                const int i4 = i & ~3;
                for (int q = 0; q < i4; q += 4) {
                    const int4 v = *reinterpret_cast<const int4*>(ids + q);
                    pos += (v.x == j) + (v.y == j) + (v.z == j) + (v.w == j);
                }
                for (int q = i4; q < i; ++q) pos += ids[q] == j;
                members[start[j] + pos] = i;
            }
            __syncthreads();
        }
        if (it < kFecoTraceIters) { FECO_STAMP(4 * it + 2) }
        fresh_tid();
        // ---- update: thread (j, d) sums its cluster's centred frames in ascending frame order; an empty cluster keeps
        // its centroid; the row's lanes then rebuild h_j
        for (int e = tid; e < kp * DPAD; e += kFecoThreads) {
            const int j = e / DPAD, d = e - j * DPAD;
            const int n = j < k ? cnt[j] : 0;
            float v;
            if (n > 0) {
                // four members per round: their list entries, then their frame elements, are loads in flight together; the
                // additions keep the ascending order (entries past the cluster are read -- inside the lists -- and not added)
                float sum = 0.f;
                const int o = start[j];
                for (int m = 0; m < n; m += 4) {
                    const int i0 = members[o + m], i1 = members[min(o + m + 1, F - 1)], i2 = members[min(o + m + 2, F - 1)],
                              i3 = members[min(o + m + 3, F - 1)];
                    const float v0 = xc_at(i0, d), v1 = xc_at(i1, d), v2 = xc_at(i2, d), v3 = xc_at(i3, d);
                    sum = sum + v0;
                    if (m + 1 < n) sum = sum + v1;
                    if (m + 2 < n) sum = sum + v2;
                    if (m + 3 < n) sum = sum + v3;
                }
                v = sum / (float)n;
            } else {
                v = cq[sw_at<DPAD>(j, d)];
            }
            if constexpr (COS) {
                // (every lane of the wave takes part in the butterfly; an empty cluster's row is not stored: same bits)
                const float c = unit_row(v);
                if (n > 0) cq[sw_at<DPAD>(j, d)] = c;
            } else {
                const float sq = row_tree_sum<DPAD>(v * v);
                if (n > 0) {
                    cq[sw_at<DPAD>(j, d)] = v;
                    if (d == 0) hq[j] = -0.5f * sq;
                }
            }
        }
        __syncthreads();
        if (it < kFecoTraceIters) { FECO_STAMP(4 * it + 3) }
    }
    FECO_STAMP(4 * kFecoTraceIters)
    FECO_CYCLES(21)
    // cnt / start / members describe the final ids in both exits: "nothing changed" leaves the previous iteration's lists
    // valid, the max_iter exit has just rebuilt them.  (max_iter >= 1 and ids start at -1: the lists exist.)
    // (two CUs: both blocks hold the same result; each writes half of it)
    const int e_lo = pr.on && half ? (k * D) / 2 : 0, e_hi = pr.on && !half ? (k * D) / 2 : k * D;
    if (out) {
        float* o = out + slot * k * D;
        for (int e = e_lo + tid; e < e_hi; e += kFecoThreads) {
            const int j = e / D, d = e - j * D;
            const int n = cnt[j];
            float v;
            if (n > 0) {
                float sum = 0.f;
                const int s0 = start[j];
                for (int m = 0; m < n; m += 4) {  // four loads in flight, additions in ascending order (as in the update)
                    const int i0 = members[s0 + m], i1 = members[min(s0 + m + 1, F - 1)], i2 = members[min(s0 + m + 2, F - 1)],
                              i3 = members[min(s0 + m + 3, F - 1)];
                    const float v0 = x[(size_t)i0 * D + d], v1 = x[(size_t)i1 * D + d], v2 = x[(size_t)i2 * D + d],
                                v3 = x[(size_t)i3 * D + d];
                    sum = sum + v0;
                    if (m + 1 < n) sum = sum + v1;
                    if (m + 2 < n) sum = sum + v2;
                    if (m + 3 < n) sum = sum + v3;
                }
                v = sum / (float)n;
            } else {
                v = x[(size_t)j * D + d];  // feature_level.py:213-214 `force` fallback
            }
            o[e] = v;
        }
        if (half == 0)
            for (int j = tid; j < k; j += kFecoThreads) counts[slot * k + j] = cnt[j];
    }
    if (!pr.on || half == 1)
        for (int i = tid; i < F; i += kFecoThreads) assign[slot * F + i] = ids[i];
    FECO_STAMP(4 * kFecoTraceIters + 1)
}
