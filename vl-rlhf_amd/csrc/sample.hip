// Next-token selection on the device (gfx950): vlr_sample_tokens of include/vlr.h "sampling".  One launch per new token does, per row, the
// transformers logits-processor chain (repetition penalty, temperature, top-k, top-p), a counter-based Gumbel-max draw, the token's
// log-prob and the finished-row / eos bookkeeping.  The logits are read only.
//
// Geometry: ONE workgroup of 1024 threads (16 waves) per row.  A row is walked in groups of 4 consecutive columns (one 16-byte load, one
// Philox block): thread t owns the groups t, t + 1024, ... and takes them in that order, four loads in flight.  The warped value z of a
// column (penalty, then temperature: two correctly rounded fp32 operations) is recomputed in every pass, never stored.
//
// Thresholds.  key(z) is the order-preserving uint32 image of z (-0 reads as +0), and both warpers are "keep key >= thr":
//   top-k: thr = the k-th largest key = the smallest t with count(key > t) < k;
//   top-p: thr = the smallest t with mass(key > t) < top_p * Z, mass = sum exp(z - max z) over the top-k survivors, Z = their total.
// One routine finds both (smp_bisect): the interval (lo, hi] of candidate t is cut 16 ways per pass over the row, 16 counts (exact) or 16
// masses per thread in registers, so a full-vocabulary top-p (top_k = 0, V = 151936) needs no sort, no LDS copy of the row and no
// histogram: at most 9 passes per threshold.
//
// No floating-point atomics; the only atomics are the bit-ORs that fill the penalty's membership map in LDS, whose result is order-free.
// Every float sum runs in an order fixed by V and this geometry alone: per thread over its groups in ascending order and the 4 columns of
// a group in order, then six xor butterflies inside the wave (every lane ends with the same bits), then the 16 waves in order.  The draw
// is an argmax under a total order (larger score, then lower index), which no reduction order can change.  Two calls give the same bits.
// exp / log are expf / logf / log1pf, never the fast intrinsics.
#include "../../include/vlr.h"
#include "common.h"

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / 64)
#define SMP_MAX_EOS 8
#define SMP_MAX_V_PENALTY (1 << 19)      // the V-bit membership map: 64 KB of LDS at most

struct smp_args {
    const float* logits;
    int B, V, ld, do_sample;
    float temperature;
    int top_k;
    float top_p, penalty;
    const int64_t* prompt_ids;
    int T, prompt_ld, prompt_div;
    const int64_t* gen_ids;
    int gen_ld, n_gen;
    const int* eos_ids;
    int n_eos, pad;
    uint32_t k0, k1, call, step;
    const int* row_ids;
    unsigned char* unfinished;
    int* next_tok;
    int64_t* out_ids;
    int out_ld;
    float* logp;
    int* finish_step;
    unsigned char* kept;
};

struct smp_row {
    const float* x;          // the row's logits
    const uint32_t* bm;      // membership map of the row's history (NULL: no penalty)
    int V, vec, do_sample;
    float pen, temp;
};

__device__ __forceinline__ uint32_t smp_key(float z) {
    const uint32_t u = __builtin_bit_cast(uint32_t, z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float smp_unkey(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// steps 1 and 2 of the contract: one multiplication or division by the penalty, one division by the temperature, each rounded once
__device__ __forceinline__ float smp_warp(const smp_row& R, float x, bool hit) {
#pragma clang fp contract(off)
    if (hit) x = x < 0.f ? x * R.pen : x / R.pen;
    if (R.do_sample && R.temp != 1.f) x = x / R.temp;      // (x / 1 is x: the common temperature skips the division, the same bits)
    return x == 0.f ? 0.f : x;      // -0 -> +0: one key per value
}

// f(i, z[4], nv): the warped values of the columns i .. i + nv - 1 (nv = 4 except in the row's last group)
template <class F>
__device__ __forceinline__ void smp_scan(const smp_row& R, F&& f) {
    const int ng = (R.V + 3) >> 2;
    for (int g0 = threadIdx.x; g0 < ng; g0 += 4 * SMP_THREADS) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * SMP_THREADS, i = g * 4;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (g < ng) {
                if (R.vec && i + 3 < R.V) {
                    v[u] = *reinterpret_cast<const f32x4*>(R.x + i);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (i + e < R.V) v[u][e] = R.x[i + e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * SMP_THREADS, i = g * 4;
            if (g < ng) {
                const uint32_t bits = R.bm ? (R.bm[i >> 5] >> (i & 31)) : 0u;      // i % 4 == 0: the group's 4 bits lie in one word
                float z[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) z[e] = smp_warp(R, v[u][e], (bits >> e) & 1u);
                f(i, z, min(4, R.V - i));
            }
        }
    }
}

__device__ __forceinline__ uint32_t smp_block_umax(uint32_t v, uint32_t* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = red[0];
    for (int i = 1; i < SMP_WAVES; ++i) t = max(t, red[i]);
    return t;
}

// The smallest t in (lo, hi] with W(key > t) < target, given that hi satisfies it.  W counts the columns (MASS false, target = k) or sums
// exp(z - m) (MASS true).  Columns with key <= lo are never looked at.  Each pass cuts (lo, hi] into 16 slices of 2^sh keys, a power of
// two so that a column finds its slice with a shift; a column above hi falls into the last slice.  S_j = slices j .. 15 summed from the
// top = W(key > lo + j 2^sh).  The decisions are taken from LDS values every thread reads alike, so the loop is uniform.
template <bool MASS>
__device__ __forceinline__ uint32_t smp_bisect(const smp_row& R, uint32_t lo, uint32_t hi, float target, float m, float* red, float* tot) {
    while (hi - lo > 1u) {
        const uint32_t w = hi - lo;
        const int sh = w <= 16u ? 0 : (32 - __clz((int)(w - 1u))) - 4;
        float acc[16], above = 0.f;      // the slices of (lo, hi], and everything above hi (one add: after the first pass most columns)
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] = 0.f;
        smp_scan(R, [&](int, const float* z, int nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t k = smp_key(z[e]);
                if (e < nv && k > lo) {
                    const float wgt = MASS ? expf(z[e] - m) : 1.f;      // counts stay exact in fp32: V < 2^24
                    const int s = k > hi ? 16 : (int)((k - lo - 1u) >> sh);      // inside: < 16, as k - lo - 1 < w <= 16 * 2^sh
                    above += s == 16 ? wgt : 0.f;
                    if (s < 16) {
#pragma unroll
                        for (int b = 0; b < 16; ++b) acc[b] += (s == b) ? wgt : 0.f;
                    }
                }
            }
        });
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] = wave_sum(acc[b]);
        above = wave_sum(above);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int b = 0; b < 16; ++b) red[(threadIdx.x >> 6) * 17 + b] = acc[b];
            red[(threadIdx.x >> 6) * 17 + 16] = above;
        }
        __syncthreads();
        if (threadIdx.x < 17) {
            float t = 0.f;
            for (int wv = 0; wv < SMP_WAVES; ++wv) t += red[wv * 17 + threadIdx.x];
            tot[threadIdx.x] = t;
        }
        __syncthreads();
        const int jmax = (int)min(15u, (w - 1u) >> sh);      // the cuts lo + j 2^sh below hi: j = 1 .. jmax (>= 1)
        float S = tot[16];
        for (int b = 15; b > jmax; --b) S += tot[b];
        int found = 0;                                       // the lowest cut that satisfies the predicate (S_j only grows as j falls)
        for (int j = jmax; j >= 1; --j) {
            S += tot[j];
            if (S < target) found = j;
        }
        if (found) {
            hi = lo + ((uint32_t)found << sh);
            lo = lo + ((uint32_t)(found - 1) << sh);
        } else {
            lo = lo + ((uint32_t)jmax << sh);
        }
    }
    return hi;
}

// Gumbel noise of column i from the word w of its Philox block: u = (r + 1/2) 2^-24 with r = w >> 8, E = -log u (a unit exponential),
// g = -log E.  (r + 1/2) 2^-24 is exact in fp32 only below 1/2; above, 1 - u = (r' + 1/2) 2^-24 with r' = 2^24 - 1 - r is, and
// E = -log1p(-(1 - u)).  u lies in [2^-25, 1 - 2^-25]: g in [-2.85, +17.33].
__device__ __forceinline__ float smp_gumbel(uint32_t w) {
    const uint32_t r = w >> 8;
    float E;
    if (r < 0x800000u) {
        E = -logf(((float)r + 0.5f) * 5.9604644775390625e-8f);
    } else {
        E = -log1pf(-(((float)(0xffffffu - r) + 0.5f) * 5.9604644775390625e-8f));
    }
    return -logf(E);
}

__global__ __launch_bounds__(SMP_THREADS) void sample_tokens_kernel(smp_args a) {
    extern __shared__ uint32_t bm[];
    __shared__ float red[SMP_WAVES * 17];
    __shared__ float tot[17];
    __shared__ int red_i[SMP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    if (a.unfinished[r] == 0) {      // (uniform over the workgroup; nobody writes the flag before the last barrier below)
        if (tid == 0) {
            a.next_tok[r] = a.pad;
            a.out_ids[(long)r * a.out_ld + a.step] = a.pad;
            a.logp[r] = 0.f;
        }
        return;
    }
    smp_row R;
    R.x = a.logits + (long)r * a.ld;
    R.V = a.V;
    R.vec = ((a.ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.logits) & 15) == 0);
    R.do_sample = a.do_sample;
    R.pen = a.penalty;
    R.temp = a.temperature;
    R.bm = nullptr;
    if (a.penalty != 1.f) {      // step 1: the ids of the row's history, each once however often it occurs
        const int words = (a.V + 31) >> 5;
        for (int i = tid; i < words; i += SMP_THREADS) bm[i] = 0u;
        __syncthreads();
        const int64_t* pr = a.prompt_ids + (long)(r / a.prompt_div) * a.prompt_ld;
        for (int i = tid; i < a.T; i += SMP_THREADS) {
            const int64_t id = pr[i];
            if (id >= 0 && id < a.V) atomicOr(&bm[id >> 5], 1u << (id & 31));
        }
        const int64_t* gr = a.gen_ids + (long)r * a.gen_ld;
        for (int i = tid; i < a.n_gen; i += SMP_THREADS) {
            const int64_t id = gr[i];
            if (id >= 0 && id < a.V) atomicOr(&bm[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
        R.bm = bm;
    }
    // the largest and the smallest key of the row (the smallest as the largest of the complements)
    uint32_t kmax = 0u, nmin = 0u;
    smp_scan(R, [&](int, const float* z, int nv) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < nv) {
                const uint32_t k = smp_key(z[e]);
                kmax = max(kmax, k);
                nmin = max(nmin, ~k);
            }
    });
    kmax = smp_block_umax(kmax, reinterpret_cast<uint32_t*>(red));
    const uint32_t kmin = ~smp_block_umax(nmin, reinterpret_cast<uint32_t*>(red));
    const float m = smp_unkey(kmax);
    uint32_t thr = 0u;      // a column is kept iff key >= thr
    if (a.do_sample && a.top_k > 0 && a.top_k < a.V)
        thr = smp_bisect<false>(R, kmin ? kmin - 1u : 0u, kmax, (float)a.top_k, m, red, tot);
    if (a.do_sample && a.top_p < 1.f) {
        float zs = 0.f;
        smp_scan(R, [&](int, const float* z, int nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nv && smp_key(z[e]) >= thr) zs += expf(z[e] - m);
        });
        const float Z = block_sum(zs, red);
        const uint32_t lo = max(kmin, thr);
        thr = smp_bisect<true>(R, lo ? lo - 1u : 0u, kmax, a.top_p * Z, m, red, tot);
    }
    // the draw and the log-prob over the kept set
    const uint32_t row_id = a.row_ids ? (uint32_t)a.row_ids[r] : (uint32_t)r;
    unsigned char* kept = a.kept ? a.kept + (long)r * a.V : nullptr;
    float zs = 0.f, best = -INFINITY, best_z = 0.f;
    int best_i = 0x7fffffff;
    smp_scan(R, [&](int i, const float* z, int nv) {
        bool k[4], any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            k[e] = e < nv && smp_key(z[e]) >= thr;
            any |= k[e];
            if (kept && e < nv) kept[i + e] = k[e] ? 1 : 0;
        }
        if (!any) return;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (a.do_sample) philox4x32_10((uint32_t)i >> 2, row_id, a.step, a.call, a.k0, a.k1, w);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k[e]) {
                zs += expf(z[e] - m);
                const float s = a.do_sample ? z[e] + smp_gumbel(w[e]) : z[e];
                if (s > best || (s == best && i + e < best_i)) best = s, best_i = i + e, best_z = z[e];
            }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float s = __shfl_xor(best, o), sz = __shfl_xor(best_z, o);
        const int si = __shfl_xor(best_i, o);
        if (s > best || (s == best && si < best_i)) best = s, best_i = si, best_z = sz;
    }
    const float Zk = block_sum(zs, red);
    __syncthreads();
    if (lane == 0) red[wave] = best, red[SMP_WAVES + wave] = best_z, red_i[wave] = best_i;
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < SMP_WAVES; ++wv) {
            const float s = red[wv];
            if (s > best || (s == best && red_i[wv] < best_i)) best = s, best_i = red_i[wv], best_z = red[SMP_WAVES + wv];
        }
        const int tok = (best_i >= 0 && best_i < a.V) ? best_i : 0;      // (a row of NaNs draws nothing: stay inside the vocabulary)
        a.next_tok[r] = tok;
        a.out_ids[(long)r * a.out_ld + a.step] = tok;
        a.logp[r] = best_z - (m + logf(Zk));
        bool fin = false;
        for (int e = 0; e < a.n_eos; ++e) fin |= a.eos_ids[e] == tok;
        if (fin) {
            a.unfinished[r] = 0;
            a.finish_step[r] = (int)a.step;
        }
    }
}

extern "C" int vlr_sample_tokens(const float* logits, int B, int V, int ld, int do_sample, float temperature, int top_k, float top_p,
                                 float repetition_penalty, const int64_t* prompt_ids, int T, int prompt_ld, int prompt_div,
                                 const int64_t* gen_ids, int gen_ld, int n_gen, const int* eos_ids, int n_eos, int pad, uint64_t seed,
                                 uint32_t call, uint32_t step, const int* row_ids, unsigned char* unfinished, int* next_tok,
                                 int64_t* out_ids, int out_ld, float* logp, int* finish_step, unsigned char* kept, hipStream_t st) {
    VLR_REQUIRE(logits && unfinished && next_tok && out_ids && logp && finish_step, "vlr_sample_tokens: null operand");
    VLR_REQUIRE(B >= 1 && V >= 1 && V < (1 << 24) && ld >= V, "vlr_sample_tokens: bad shape B=%d V=%d ld=%d (1 <= V < 2^24, ld >= V)", B, V, ld);
    VLR_REQUIRE(temperature > 0.f, "vlr_sample_tokens: temperature %g has to be a strictly positive float", (double)temperature);
    VLR_REQUIRE(top_p > 0.f && top_p <= 1.f, "vlr_sample_tokens: top_p %g has to be a float > 0 and <= 1", (double)top_p);
    VLR_REQUIRE(repetition_penalty > 0.f, "vlr_sample_tokens: repetition_penalty %g has to be a strictly positive float",
                (double)repetition_penalty);
    VLR_REQUIRE(n_eos >= 0 && n_eos <= SMP_MAX_EOS && (eos_ids || n_eos == 0), "vlr_sample_tokens: n_eos %d (0..%d ids on the device)", n_eos,
                SMP_MAX_EOS);
    VLR_REQUIRE(out_ld >= 1 && step < (uint32_t)out_ld, "vlr_sample_tokens: step %u outside the output ids' %d columns", step, out_ld);
    VLR_REQUIRE(T >= 0 && n_gen >= 0 && prompt_div >= 1, "vlr_sample_tokens: bad history T=%d n_gen=%d prompt_div=%d", T, n_gen, prompt_div);
    if (repetition_penalty != 1.f) {
        VLR_REQUIRE(V <= SMP_MAX_V_PENALTY, "vlr_sample_tokens: repetition_penalty needs V <= %d (the membership map in LDS), got %d",
                    SMP_MAX_V_PENALTY, V);
        VLR_REQUIRE((prompt_ids && prompt_ld >= T) || T == 0, "vlr_sample_tokens: null prompt_ids or prompt_ld %d < T %d", prompt_ld, T);
        VLR_REQUIRE((gen_ids && gen_ld >= n_gen) || n_gen == 0, "vlr_sample_tokens: null gen_ids or gen_ld %d < n_gen %d", gen_ld, n_gen);
    }
    smp_args a;
    a.logits = logits, a.B = B, a.V = V, a.ld = ld, a.do_sample = do_sample ? 1 : 0;
    a.temperature = temperature, a.top_k = top_k, a.top_p = top_p, a.penalty = repetition_penalty;
    a.prompt_ids = prompt_ids, a.T = T, a.prompt_ld = prompt_ld, a.prompt_div = prompt_div;
    a.gen_ids = gen_ids, a.gen_ld = gen_ld, a.n_gen = n_gen;
    a.eos_ids = eos_ids, a.n_eos = n_eos, a.pad = pad;
    a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.call = call, a.step = step;
    a.row_ids = row_ids, a.unfinished = unfinished, a.next_tok = next_tok, a.out_ids = out_ids, a.out_ld = out_ld;
    a.logp = logp, a.finish_step = finish_step, a.kept = kept;
    const size_t lds = repetition_penalty != 1.f ? (size_t)((V + 31) >> 5) * 4 : 0;
    hipLaunchKernelGGL(sample_tokens_kernel, dim3(B), dim3(SMP_THREADS), lds, st, a);
    return vlr_check_launch("vlr_sample_tokens");
}
