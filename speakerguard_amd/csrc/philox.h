// Philox4x32-10 counter-based generator (Salmon, Moraes, Dror, Shaw, SC'11; Random123 philox4x32, 10 rounds), the map from a
// word to a uniform, and the key of a row of a pass: the one copy of each.  Restated on the CPU in oracle/philox.py, which is
// checked against the Random123 known-answer vectors.  (The Box-Muller forms stay with their kernels: they differ on purpose.)
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "sg_internal.h"

namespace sg {

// the ten rounds, in place: (c0, c1, c2, c3) becomes the four output words
__device__ __forceinline__ void philox4x32_10(uint64_t key, uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// the first output word
__device__ __forceinline__ uint32_t philox4x32_10_w0(uint64_t key, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    philox4x32_10(key, c0, c1, c2, c3);
    return c0;
}
// the first TWO output words (a Box-Muller pair from one counter): returns word 0, *w1 = word 1
__device__ __forceinline__ uint32_t philox4x32_10_w01(uint64_t key, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* w1) {
    philox4x32_10(key, c0, c1, c2, c3);
    *w1 = c1;
    return c0;
}

// a word's top 24 bits as a uniform in (0, 1): never 0, never 1, exact in float32
__device__ __forceinline__ float philox_unit24(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// (key, utterance) of row b of a call (speakerguard_hip.h, sg_dither): g = row_base + b, repeat = rep_rows > 0 ? g / rep_rows : 0,
// key = seed + repeat * kRepKey, utterance = index_base + g - repeat * rep_rows -- the same draws however the work was cut.
// rep_rows: the caller's repeat length (a batched EOT pass overrides the struct's).
__device__ __forceinline__ void noise_row_key(const sg_dither& nz, int b, int64_t rep_rows, uint64_t* key, int64_t* utt) {
    const int64_t g = nz.row_base + b;
    const int64_t rep = rep_rows > 0 ? g / rep_rows : 0, u = g - rep * rep_rows;
    *key = nz.seed + (uint64_t)rep * kRepKey;
    *utt = nz.index_base + u;
}

}  // namespace sg
