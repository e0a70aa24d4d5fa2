// SirenAttack's particle swarm (reference attack/SirenAttack.py:40-188), resident on the device.  Three entry points:
//   sg_pso_init    :66-86    the swarm of an epoch: personal bests (fresh, or particle 0 carried over), locations, velocities,
//                            and the epoch's first queries
//   sg_pso_select  :115-132  the scalar work after a model call: personal and global best VALUES, who improved, who leads
//   sg_pso_move    :121, :131, :163-174  the hot path, ONE streaming launch per iteration: personal / global best LOCATIONS
//                            saved, then velocities and locations updated and the next queries written
//
// State, float32, in the slot of its utterance for the whole chunk of n utterances (nothing is compacted by copying):
//   loc, vel, pbest_loc (n, P, T)   gbest_loc (n, T)   pbest (n, P)   gbest (n)
// The ACTIVE set (consider_index, delete_found :191-232) is a list of slots handed to every call; per-row arrays of a call
// (loss, improved, the report, given draws) and the queries are dense in the order of that list: row k of the list owns
// queries [k P, (k + 1) P) = loc + x, the tensor the model call takes.  The list, and the per-row integers that go with it,
// are HOST arrays: they are checked before anything is launched and travel as launch arguments (nothing of the caller's is
// read after the call returns), which bounds a chunk at kPsoMaxRows = 256 utterances.  P <= kPsoMaxParticles = 1024.
//
// Arithmetic: the reference's float32 sequence, one rounding per operation (no contraction, see the pragma):
//   t1 = w vel;  t2 = (c1 r1) (pbest_loc - loc);  t3 = (c2 r2) (gbest_loc - loc);  vel' = (t1 + t2) + t3;
//   loc' = min(max(loc + vel', lower), upper);  query = loc' + x.            w, c1, c2: the caller's doubles rounded to float.
//
// Draws.  GIVEN (pos_in / vel_in / r1_in / r2_in, dense in the order of the rows that use them): used exactly as given,
// nothing clamped or offset -- the reference's own numpy draws, cast to float32, give the reference's bits.
// NOT GIVEN: the library's generator, one Philox4x32-10 call (philox.h) per element and particle,
//   (w0, w1, ., .) = philox(counter = (t, particle, g lo, g hi), key),   g = index_base + slot  (the utterance's GLOBAL index),
//   u0 = philox_unit24(w0), u1 = philox_unit24(w1)  in (0, 1);
//   sg_pso_init:  position = min(max(lower + (upper - lower) u0, lower), upper)           (particle 0 of epoch > 0: unused)
//                 velocity = min(max(-V + (V - -V) u1, -V), V),  V = |lower - upper|
//   sg_pso_move:  r1 = u0 + 1e-5f,  r2 = u1 + 1e-5f                                                    (:167-168)
// `key` names the draw: the host derives it from (seed, attack call, restart, draw number), draw number = epoch (max_iter + 2)
// for the epoch's init and epoch (max_iter + 2) + 1 + iter for the move after evaluation iter (EngineOps.noise_seed with
// SirenAttack's tag).  The key does not know the chunk and the counter holds the global index, so an utterance's draws do not
// depend on how a batch is chunked or sharded.  Restated in tests/pso_restate.py on oracle/philox.py.
//
// Memory: a thread owns V consecutive samples of one active row and walks the particles (the grid is sized from
// n_active T, not from P).  V = 4 -- 16-byte loads and stores -- when T is a multiple of 4, every base is 16-byte aligned
// (then every row of every array is) and the launch is large enough to be bound by bandwidth (pso_vec4); otherwise V = 1:
// with T % 4 != 0 the rows of particle p start p T floats in, at every alignment.  sg_pso_move touches each state element at
// most once: particle gbest_from goes first (its new personal best location IS the new global best location the others
// need), then the others in order.
#include <initializer_list>

#include "philox.h"
#include "sg_internal.h"
#include "wave_reduce.h"

// torch's elementwise expressions round after every multiply and every add: no FMAs here
#pragma clang fp contract(off)

namespace sg {
namespace {

constexpr int kPsoMaxRows = 256, kPsoMaxParticles = 1024;

// the active rows of a call and up to two integers per row, as launch arguments (read with uniform indices only)
struct PsoRows {
    int16_t slot[kPsoMaxRows];
    int16_t a[kPsoMaxRows];  // init: best_index; move: gbest_from
    int16_t q[kPsoMaxRows];  // move: the row's place in the NEXT active set, -1 = it does not continue
};

typedef float pso_f4 __attribute__((ext_vector_type(4)));
template <int V> struct PsoVec { float v[V]; };

template <int V> __device__ __forceinline__ PsoVec<V> pso_ld(const float* p) {
    PsoVec<V> r;
    if constexpr (V == 4) {
        const pso_f4 x = *reinterpret_cast<const pso_f4*>(p);
        r.v[0] = x.x; r.v[1] = x.y; r.v[2] = x.z; r.v[3] = x.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V> __device__ __forceinline__ void pso_st(float* p, const PsoVec<V>& r) {
    if constexpr (V == 4) *reinterpret_cast<pso_f4*>(p) = pso_f4{r.v[0], r.v[1], r.v[2], r.v[3]};
    else *p = r.v[0];
}

// the two uniforms of (sample t, particle p, global utterance g) under `key`
__device__ __forceinline__ void pso_uniforms(uint64_t key, int t, int p, int64_t g, float* u0, float* u1) {
    uint32_t w1;
    const uint32_t w0 = philox4x32_10_w01(key, (uint32_t)t, (uint32_t)p, (uint32_t)g, (uint32_t)((uint64_t)g >> 32), &w1);
    *u0 = philox_unit24(w0);
    *u1 = philox_unit24(w1);
}

// grid (ceil(T / (256 V)), n_active).  carry = epoch > 0: particle 0 takes location and value of particle rows.a[k].  The
// carried row is read before the thread writes any particle of its samples, and no other thread touches those samples.
template <int V>
__global__ __launch_bounds__(256) void pso_init_kernel(PsoRows rows, int P, int T, int carry, const float* __restrict__ x,
                                                       const float* __restrict__ lower, const float* __restrict__ upper,
                                                       uint64_t key, int64_t index_base, const float* __restrict__ pos_in,
                                                       const float* __restrict__ vel_in, float* __restrict__ loc,
                                                       float* __restrict__ vel, float* pbest_loc, float* pbest,
                                                       float* __restrict__ queries) {
    const int k = blockIdx.y, slot = rows.slot[k], best = rows.a[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the values (:70, :78-79); nobody else reads or writes this row
        float* pb = pbest + (size_t)slot * P;
        if (carry) pb[0] = pb[best];
        for (int p = carry; p < P; ++p) pb[p] = INFINITY;
    }
    const int t0 = (blockIdx.x * 256 + threadIdx.x) * V;
    if (t0 >= T) return;
    const size_t urow = (size_t)slot * T + t0;
    const PsoVec<V> xv = pso_ld<V>(x + urow), lo = pso_ld<V>(lower + urow), hi = pso_ld<V>(upper + urow);
    PsoVec<V> bl = xv;
    if (carry) bl = pso_ld<V>(pbest_loc + ((size_t)slot * P + best) * T + t0);
    const int fresh = P - carry;
    const bool draw_vel = vel_in == nullptr;
    for (int p = 0; p < P; ++p) {
        const bool kept = carry && p == 0, draw_pos = !kept && pos_in == nullptr;
        PsoVec<V> pl = bl, vl{};
        if (!kept && pos_in) pl = pso_ld<V>(pos_in + ((size_t)k * fresh + (p - carry)) * T + t0);
        if (vel_in) vl = pso_ld<V>(vel_in + ((size_t)k * P + p) * T + t0);
        if (draw_pos || draw_vel) {
#pragma unroll
            for (int c = 0; c < V; ++c) {
                float u0, u1;
                pso_uniforms(key, t0 + c, p, index_base + slot, &u0, &u1);
                if (draw_pos) pl.v[c] = fminf(fmaxf(lo.v[c] + (hi.v[c] - lo.v[c]) * u0, lo.v[c]), hi.v[c]);
                if (draw_vel) {
                    const float vhi = fabsf(lo.v[c] - hi.v[c]), vlo = -vhi;
                    vl.v[c] = fminf(fmaxf(vlo + (vhi - vlo) * u1, vlo), vhi);
                }
            }
        }
        const size_t o = ((size_t)slot * P + p) * T + t0;
        pso_st<V>(pbest_loc + o, pl);
        pso_st<V>(loc + o, pl);
        pso_st<V>(vel + o, vl);
        PsoVec<V> qv;
#pragma unroll
        for (int c = 0; c < V; ++c) qv.v[c] = pl.v[c] + xv.v[c];
        pso_st<V>(queries + ((size_t)k * P + p) * T + t0, qv);
    }
}

// one wave per active row: grid (n_active), block 64.  Lane l walks particles l, l + 64, ..: pbest = loss where loss < pbest
// (strict), improved = that; the first-index argmin of the new pbest (the lane's first minimum, then the lanes' by (value,
// index)); gbest = that minimum where it is < gbest (strict).  report (3, n_active): gbest after the update, the argmin, and
// gbest_from = the argmin where gbest was updated, else -1 -- the integers as floats (exact: P <= 1024).
__global__ __launch_bounds__(64) void pso_select_kernel(PsoRows rows, int n_active, int P, const float* __restrict__ loss,
                                                        float* __restrict__ pbest, float* __restrict__ gbest,
                                                        uint8_t* __restrict__ improved, float* __restrict__ report) {
    const int k = blockIdx.x, slot = rows.slot[k], lane = threadIdx.x;
    float best = INFINITY;
    int at = 0x7FFFFFFF;  // (a lane without a particle, or whose values are all +inf, defers to any index)
    for (int p = lane; p < P; p += 64) {
        const float l = loss[(size_t)k * P + p];
        float pb = pbest[(size_t)slot * P + p];
        const bool imp = l < pb;
        if (imp) pbest[(size_t)slot * P + p] = pb = l;
        improved[(size_t)k * P + p] = imp ? 1 : 0;
        if (pb < best || at == 0x7FFFFFFF) best = pb, at = p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (ob < best || (ob == best && oa < at)) best = ob, at = oa;
    }
    if (lane == 0) {
        const float g = gbest[slot];
        const bool upd = best < g;
        if (upd) gbest[slot] = best;
        report[k] = upd ? best : g;
        report[(size_t)n_active + k] = (float)at;
        report[2 * (size_t)n_active + k] = upd ? (float)at : -1.f;
    }
}

// grid (ceil(T / (256 V)), n_active of the PREVIOUS active set).  rows.a[k] = gbest_from, rows.q[k] = place among the rows that
// continue (-1: none); do_move = 0 at the last iteration of an epoch: locations are saved, nothing moves.
template <int V>
__global__ __launch_bounds__(256) void pso_move_kernel(PsoRows rows, int P, int T, int do_move, const float* __restrict__ x,
                                                       const float* __restrict__ lower, const float* __restrict__ upper,
                                                       float w, float c1, float c2, uint64_t key, int64_t index_base,
                                                       const float* __restrict__ r1_in, const float* __restrict__ r2_in,
                                                       const uint8_t* __restrict__ improved, float* __restrict__ loc,
                                                       float* __restrict__ vel, float* __restrict__ pbest_loc,
                                                       float* __restrict__ gbest_loc, float* __restrict__ queries) {
    const int k = blockIdx.y, slot = rows.slot[k], gf = rows.a[k], q = rows.q[k];
    const bool cont = do_move && q >= 0;
    const int t0 = (blockIdx.x * 256 + threadIdx.x) * V;
    if (t0 >= T) return;
    const size_t urow = (size_t)slot * T + t0;
    PsoVec<V> xv{}, lo{}, hi{}, G{};
    if (cont) {
        xv = pso_ld<V>(x + urow);
        lo = pso_ld<V>(lower + urow);
        hi = pso_ld<V>(upper + urow);
        if (gf < 0) G = pso_ld<V>(gbest_loc + urow);
    }
    const uint8_t* imp_row = improved + (size_t)k * P;
    auto particle = [&](int p) {
        const bool imp = imp_row[p] != 0;
        if (!imp && !cont && p != gf) return;
        const size_t o = ((size_t)slot * P + p) * T + t0;
        PsoVec<V> L{}, PB;
        if (imp || cont) L = pso_ld<V>(loc + o);
        if (imp) {
            PB = L;
            pso_st<V>(pbest_loc + o, L);  // :121
        } else {
            PB = pso_ld<V>(pbest_loc + o);
        }
        if (p == gf) {
            G = PB;
            pso_st<V>(gbest_loc + urow, G);  // :131
        }
        if (!cont) return;
        PsoVec<V> vl = pso_ld<V>(vel + o), r1{}, r2{}, qv;
        const size_t d = ((size_t)q * P + p) * T + t0;
        if (r1_in) r1 = pso_ld<V>(r1_in + d);
        if (r2_in) r2 = pso_ld<V>(r2_in + d);
        if (!r1_in || !r2_in) {
#pragma unroll
            for (int c = 0; c < V; ++c) {
                float u0, u1;
                pso_uniforms(key, t0 + c, p, index_base + slot, &u0, &u1);
                if (!r1_in) r1.v[c] = u0 + 1e-5f;
                if (!r2_in) r2.v[c] = u1 + 1e-5f;
            }
        }
#pragma unroll
        for (int c = 0; c < V; ++c) {  // :171-174
            const float t1 = w * vl.v[c];
            const float t2 = (c1 * r1.v[c]) * (PB.v[c] - L.v[c]);
            const float t3 = (c2 * r2.v[c]) * (G.v[c] - L.v[c]);
            const float nv = (t1 + t2) + t3;
            const float nl = fminf(fmaxf(L.v[c] + nv, lo.v[c]), hi.v[c]);
            vl.v[c] = nv;
            L.v[c] = nl;
            qv.v[c] = nl + xv.v[c];
        }
        pso_st<V>(vel + o, vl);
        pso_st<V>(loc + o, L);
        pso_st<V>(queries + d, qv);
    };
    if (gf >= 0) particle(gf);
    for (int p = 0; p < P; ++p)
        if (p != gf) particle(p);
}

// 16-byte kernels?  Only where T and every base allow them, and only when the launch then still has two waves for every SIMD
// of the chip (n_active T / 4 threads >= compute units x 4 x 2 x 64): below that the launch is bound by latency, not by
// bandwidth, and four times as many threads with 4-byte accesses are faster.  Measured at P = 50, T = 48000
// (profiles/siren_bench.txt): 1 and 8 rows 0.051 / 0.123 ms scalar against 0.071 / 0.133 ms; 16 rows 0.214 against 0.180 ms;
// 32 rows the same, 64 rows 0.682 against 0.655 ms.  Tuning knob, read per call: SG_PSO_VEC=1 keeps the scalar kernels
// everywhere, SG_PSO_VEC=4 takes the 16-byte ones wherever they are allowed.  Same bits either way.
bool pso_vec4(const sg_ctx* ctx, int T, int n_active, std::initializer_list<const void*> bases) {
    uintptr_t bits = (uintptr_t)(T & 3);
    for (const void* b : bases) bits |= reinterpret_cast<uintptr_t>(b) & 15;
    if (bits != 0) return false;
    if (const char* e = sg_tune_env("SG_PSO_VEC")) return atoi(e) == 4;
    return (int64_t)n_active * (T / 4) >= (int64_t)ctx->num_cus * 4 * 2 * 64;
}

// what the three entries refuse about the shape and the row list; fills rows->slot
int pso_check_rows(sg_ctx* ctx, const char* who, int n, int P, int T, const int32_t* rows_host, int n_active, PsoRows* rows) {
    if (n < 1 || n > kPsoMaxRows || P < 1 || P > kPsoMaxParticles || T < 1)
        return fail(ctx, SG_ERR_ARG, "%s: need 1 <= n <= %d, 1 <= P <= %d, T >= 1 (n %d, P %d, T %d)", who, kPsoMaxRows, kPsoMaxParticles,
                    n, P, T);
    if (n_active < 1 || n_active > n) return fail(ctx, SG_ERR_ARG, "%s: %d active rows of %d utterances", who, n_active, n);
    bool seen[kPsoMaxRows] = {};
    for (int k = 0; k < n_active; ++k) {
        const int r = rows_host[k];
        if (r < 0 || r >= n) return fail(ctx, SG_ERR_ARG, "%s: row %d of the list is slot %d, outside 0 .. %d", who, k, r, n - 1);
        if (seen[r]) return fail(ctx, SG_ERR_ARG, "%s: slot %d is listed twice", who, r);
        seen[r] = true;
        rows->slot[k] = (int16_t)r;
    }
    return SG_OK;
}

int pso_launched(sg_ctx* ctx, const char* who) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return SG_OK;
}

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" int sg_pso_init(sg_ctx* ctx, const float* x_dev, const float* lower_dev, const float* upper_dev, int32_t n, int32_t P,
                           int32_t T, const int32_t* rows_host, int32_t n_active, int32_t epoch, const int32_t* best_index_host,
                           uint64_t key, int64_t index_base, const float* pos_in_dev, const float* vel_in_dev, float* loc_dev,
                           float* vel_dev, float* pbest_loc_dev, float* pbest_dev, float* queries_dev, void* stream) {
    const char* who = "sg_pso_init";
    if (!ctx) return SG_ERR_ARG;
    if (!x_dev || !lower_dev || !upper_dev || !rows_host || !loc_dev || !vel_dev || !pbest_loc_dev || !pbest_dev || !queries_dev)
        return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    if (epoch < 0 || (epoch > 0 && !best_index_host)) return fail(ctx, SG_ERR_ARG, "%s: epoch %d needs best_index", who, epoch);
    PsoRows rows{};
    if (int rc = pso_check_rows(ctx, who, n, P, T, rows_host, n_active, &rows)) return rc;
    for (int k = 0; epoch > 0 && k < n_active; ++k) {
        if (best_index_host[k] < 0 || best_index_host[k] >= P)
            return fail(ctx, SG_ERR_ARG, "%s: best_index %d of row %d outside 0 .. %d", who, best_index_host[k], k, P - 1);
        rows.a[k] = (int16_t)best_index_host[k];
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    hipStream_t s = (hipStream_t)stream;
    const int carry = epoch > 0;
    if (pso_vec4(ctx, T, n_active, {x_dev, lower_dev, upper_dev, pos_in_dev, vel_in_dev, loc_dev, vel_dev, pbest_loc_dev, queries_dev}))
        hipLaunchKernelGGL(pso_init_kernel<4>, dim3((unsigned)((T / 4 + 255) / 256), (unsigned)n_active), dim3(256), 0, s, rows, P, T, carry,
                           x_dev, lower_dev, upper_dev, key, index_base, pos_in_dev, vel_in_dev, loc_dev, vel_dev, pbest_loc_dev,
                           pbest_dev, queries_dev);
    else
        hipLaunchKernelGGL(pso_init_kernel<1>, dim3((unsigned)((T + 255) / 256), (unsigned)n_active), dim3(256), 0, s, rows, P, T, carry,
                           x_dev, lower_dev, upper_dev, key, index_base, pos_in_dev, vel_in_dev, loc_dev, vel_dev, pbest_loc_dev,
                           pbest_dev, queries_dev);
    return pso_launched(ctx, who);
}

extern "C" int sg_pso_select(sg_ctx* ctx, const float* loss_dev, int32_t n, int32_t P, const int32_t* rows_host, int32_t n_active,
                             float* pbest_dev, float* gbest_dev, uint8_t* improved_dev, float* report_dev, void* stream) {
    const char* who = "sg_pso_select";
    if (!ctx) return SG_ERR_ARG;
    if (!loss_dev || !rows_host || !pbest_dev || !gbest_dev || !improved_dev || !report_dev)
        return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    PsoRows rows{};
    if (int rc = pso_check_rows(ctx, who, n, P, 1, rows_host, n_active, &rows)) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    hipLaunchKernelGGL(pso_select_kernel, dim3((unsigned)n_active), dim3(64), 0, (hipStream_t)stream, rows, n_active, P, loss_dev,
                       pbest_dev, gbest_dev, improved_dev, report_dev);
    return pso_launched(ctx, who);
}

extern "C" int sg_pso_move(sg_ctx* ctx, const float* x_dev, const float* lower_dev, const float* upper_dev, int32_t n, int32_t P,
                           int32_t T, const int32_t* rows_host, int32_t n_active, const int32_t* gbest_from_host,
                           const int32_t* continue_host, int32_t do_move, float w, float c1, float c2, uint64_t key,
                           int64_t index_base, const float* r1_in_dev, const float* r2_in_dev, const uint8_t* improved_dev,
                           float* loc_dev, float* vel_dev, float* pbest_loc_dev, float* gbest_loc_dev, float* queries_dev,
                           void* stream) {
    const char* who = "sg_pso_move";
    if (!ctx) return SG_ERR_ARG;
    if (!x_dev || !lower_dev || !upper_dev || !rows_host || !gbest_from_host || !continue_host || !improved_dev || !loc_dev ||
        !vel_dev || !pbest_loc_dev || !gbest_loc_dev)
        return fail(ctx, SG_ERR_ARG, "%s: null argument", who);
    PsoRows rows{};
    if (int rc = pso_check_rows(ctx, who, n, P, T, rows_host, n_active, &rows)) return rc;
    int n_cont = 0;
    for (int k = 0; k < n_active; ++k) {
        if (gbest_from_host[k] < -1 || gbest_from_host[k] >= P)
            return fail(ctx, SG_ERR_ARG, "%s: gbest_from %d of row %d outside -1 .. %d", who, gbest_from_host[k], k, P - 1);
        rows.a[k] = (int16_t)gbest_from_host[k];
        rows.q[k] = (int16_t)(continue_host[k] ? n_cont++ : -1);
    }
    const bool moves = do_move != 0 && n_cont > 0;
    if (moves && !queries_dev) return fail(ctx, SG_ERR_ARG, "%s: rows that move need the queries", who);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SG_ERR_HIP, "%s: hipSetDevice failed", who);
    hipStream_t s = (hipStream_t)stream;
    if (pso_vec4(ctx, T, n_active, {x_dev, lower_dev, upper_dev, r1_in_dev, r2_in_dev, loc_dev, vel_dev, pbest_loc_dev, gbest_loc_dev, queries_dev}))
        hipLaunchKernelGGL(pso_move_kernel<4>, dim3((unsigned)((T / 4 + 255) / 256), (unsigned)n_active), dim3(256), 0, s, rows, P, T,
                           (int)moves, x_dev, lower_dev, upper_dev, w, c1, c2, key, index_base, r1_in_dev, r2_in_dev, improved_dev,
                           loc_dev, vel_dev, pbest_loc_dev, gbest_loc_dev, queries_dev);
    else
        hipLaunchKernelGGL(pso_move_kernel<1>, dim3((unsigned)((T + 255) / 256), (unsigned)n_active), dim3(256), 0, s, rows, P, T,
                           (int)moves, x_dev, lower_dev, upper_dev, w, c1, c2, key, index_base, r1_in_dev, r2_in_dev, improved_dev,
                           loc_dev, vel_dev, pbest_loc_dev, gbest_loc_dev, queries_dev);
    return pso_launched(ctx, who);
}
