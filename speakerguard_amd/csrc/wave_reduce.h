// Wave and block reductions, one copy for every kernel file.  Bit equality between launch strategies, shards and loop forms is
// this library's contract, and a reduction's ORDER decides its bits: each function states its order in one line, and that line
// is the contract.  (The butterflies of k_feco_warped.hip -- bfly / swz -- and the argmax merges of loss_device.h and
// k_feco_kmeans.h are contracts of their own and live with their kernels.)
#pragma once
#include <hip/hip_runtime.h>

namespace sg {

struct OpSum { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct OpMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct OpMin { __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); } };

// order: v = op(v, v of lane ^ o) for o = 32, 16, 8, 4, 2, 1; every lane ends with the same value
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_xor(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum_xor(T v) { return wave_reduce_xor(v, OpSum()); }
__device__ __forceinline__ float wave_max_xor(float v) { return wave_reduce_xor(v, OpMax()); }
__device__ __forceinline__ float wave_min_xor(float v) { return wave_reduce_xor(v, OpMin()); }

// order: wave_sum_xor's, the six steps written out.  Same sum, same bits; the compiler orders the shuffles' address arithmetic
// differently for the two spellings, and STOI's kernels (k_stoi.hip) were built from this one.
__device__ __forceinline__ double wave_sum_xor_steps(double s) {
    s = s + __shfl_xor(s, 32, 64);
    s = s + __shfl_xor(s, 16, 64);
    s = s + __shfl_xor(s, 8, 64);
    s = s + __shfl_xor(s, 4, 64);
    s = s + __shfl_xor(s, 2, 64);
    s = s + __shfl_xor(s, 1, 64);
    return s;
}

// order: inside each row of 16 lanes v += v of lane ^ 1, lane ^ 2, then the half-row mirror and the row mirror (after the quad
// steps a quad holds one value, so the mirrors pair exactly the quads that lane ^ 4 and lane ^ 8 pair); every lane of a row ends
// with its row's sum.  Four DPP adds and no LDS traffic.
__device__ __forceinline__ float row16_sum_dpp(float v) {
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));  // row_mirror
    return v;
}
// order: row16_sum_dpp, then the four row sums r0 .. r3 (lanes 0, 16, 32, 48) through scalar registers as (r0 + r1) + (r2 + r3);
// the same value in every lane.  ~12 instructions; the ds_bpermute butterfly costs six dependent LDS round trips per sum.
__device__ __forceinline__ float wave_sum_rows(float v) {
    v = row16_sum_dpp(v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return (r0 + r1) + (r2 + r3);
}

// order: wave_reduce_xor in every wave, then the waves' values w0 .. w(n-1) (lane 0 of wave i writes scratch[i]) combined as
// op(.. op(op(w0, w1), w2) .., w(n-1)); valid on every thread.  N_WAVES: the count when it is a constant of the arithmetic
// (0: the block's own, blockDim.x / 64).  One barrier between the scratch writes and the reads; ENTRY_BARRIER adds one in
// front, for a scratch that an earlier phase may still be reading.  Butterfly and combine are one body, called from the
// kernel itself: split in two, or wrapped once more, the same text schedules differently.
template <int N_WAVES = 0, bool ENTRY_BARRIER = true, typename T, typename Op>
__device__ __forceinline__ T block_reduce_xor(T v, T* scratch, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = N_WAVES > 0 ? N_WAVES : blockDim.x >> 6;
    if (ENTRY_BARRIER) __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    T r = scratch[0];
    for (int i = 1; i < n_waves; ++i) r = op(r, scratch[i]);
    return r;
}

}  // namespace sg
