// Helpers of the sampled token selection (elementwise.hip, greedy_select_sampled_kernel; ops.h, SampleCtl): the Philox4x32-10
// generator, the order-preserving key of a score, the fixed-point weight, a 256-thread integer scan and the radix select that finds
// the top-k and top-p thresholds.  Everything after the weights is integer arithmetic: no result depends on a summation order.
#pragma once
#include "ops.h"
#include "ban.h"

typedef unsigned long long sample_u64;

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  Known answers: all-zero counter and key
// -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all-ones -> 408f276d 41c83b0e a20bc7c6 6d5451fd.
__host__ __device__ inline void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
    for (int r = 0; r < 10; ++r) {
        const sample_u64 p0 = (sample_u64)0xD2511F53u * c0, p1 = (sample_u64)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// The 64-bit uniform of a caption's draw: counter (draw, 0, key_lo, key_hi), key (seed_lo, seed_hi), U = (out0 << 32) | out1
__host__ __device__ inline sample_u64 sample_uniform(sample_u64 seed, sample_u64 key, unsigned draw) {
    unsigned o[4];
    philox4x32_10(draw, 0u, (unsigned)key, (unsigned)(key >> 32), (unsigned)seed, (unsigned)(seed >> 32), o);
    return ((sample_u64)o[0] << 32) | o[1];
}

// A score as an unsigned key with the order of the floats (-inf lowest, +inf highest; -0 has been made +0 before)
constexpr unsigned SAMPLE_KEY_NEG_INF = 0x007FFFFFu;
__device__ __forceinline__ unsigned sample_key(float z) {
    const unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// Steps 1 and 2 of the distribution on entry i of a row: HF's processors (penalty, then the bans; a NaN stands as -inf), then the
// temperature, a true fp32 division.  mask = an index held at -inf as well (the MinLength EOS; -1 = none).
// s = the raw logit x[i], loaded by the caller: the passes below keep SAMPLE_LOADS independent loads in flight per thread (a pass
// that waits for every load in turn is bound by the L2 latency, not by its arithmetic).
constexpr int SAMPLE_LOADS = 8;
template <bool PEN>
__device__ __forceinline__ unsigned sample_zkey(float s, int i, const unsigned* bm, const unsigned* seen, float pen,
                                                float temperature, int mask) {
    if (PEN && ban_bit(seen, i)) s = repeat_penalise(s, pen);
    if (ban_bit(bm, i) || i == mask || !(s == s)) s = -INFINITY;
    float z = __fdiv_rn(s, temperature);
    if (z == 0.f) z = 0.f;                               // -0 and +0 are one value: one key
    return sample_key(z);
}

// Step 4: w = (uint64)(expf(z - m) * 2^40), accurate expf; the maximum itself is 2^40, -inf is 0 (also in a row that holds nothing else)
__device__ __forceinline__ sample_u64 sample_weight(unsigned key, unsigned mkey, float m) {
    if (key <= SAMPLE_KEY_NEG_INF) return 0ull;
    if (key == mkey) return 1ull << 40;
    return (sample_u64)(expf(sample_unkey(key) - m) * 1099511627776.f);
}

// Inclusive scan of one value per thread over the 256-thread block, in thread order; *total = the sum.  ws: 4 words of LDS.
// Two barriers; integer, so exact.
__device__ __forceinline__ sample_u64 sample_block_scan(sample_u64 v, int tid, sample_u64* ws, sample_u64* total) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const sample_u64 up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    if (lane == 63) ws[wave] = v;
    __syncthreads();
    const sample_u64 w0 = ws[0], w1 = ws[1], w2 = ws[2], w3 = ws[3];
    v += wave > 0 ? w0 : 0ull;
    v += wave > 1 ? w1 : 0ull;
    v += wave > 2 ? w2 : 0ull;
    *total = w0 + w1 + w2 + w3;
    __syncthreads();
    return v;
}

// LDS of the radix select and the draw
struct SampleShared {
    sample_u64 hist[4][256];       // one histogram per wave: a peaked row puts most entries into a few bins
    sample_u64 ws[4];
    sample_u64 rest;               // what is left of the bound below the selected bin
    unsigned bin;
    unsigned mkey[4];
    int token, kept;
};

// One count into the wave's histogram per distinct bin for the first two bins met (ballots), plain atomics for what is left: the top
// byte of a row of logits takes a handful of values, the lower bytes are spread.  Called by every lane of the wave.
__device__ __forceinline__ void sample_count_add(sample_u64* h, bool valid, unsigned bin, int lane) {
    bool pend = valid;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const sample_u64 pm = __ballot(pend);
        if (pm == 0ull) break;                           // uniform over the wave
        const int leader = __ffsll((long long)pm) - 1;
        const unsigned b0 = __shfl(bin, leader);
        const bool mine = pend && bin == b0;
        const sample_u64 mm = __ballot(mine);
        if (lane == leader) atomicAdd(&h[b0], (sample_u64)__popcll(mm));
        if (mine) pend = false;
    }
    if (pend) atomicAdd(&h[bin], 1ull);
}

// The threshold of a cut, by a 4 x 8-bit radix select over LDS histograms (four reads of the row).  Over the entries of the row in
// ascending order of d - d = ~key and weight 1 when COUNT (top-k: descending scores), d = key and weight w of the entries with
// key >= keep_min otherwise (top-p) - it returns the smallest d with sum_{d' <= d} weight > bound, 0 when the total is not above
// it (a row of weight 0).  !COUNT: bound = min(floor(omp * (double)W), W - 1) with W the total weight, from the first histogram -
// the maximal value always stays.  Every thread returns the same value; the control flow does not depend on the data.
template <bool PEN, bool COUNT>
__device__ __forceinline__ unsigned sample_radix_select(const float* __restrict__ x, int V, const unsigned* bm, const unsigned* seen,
                                                        float pen, float temperature, int mask, int tid, sample_u64 bound, double omp,
                                                        unsigned keep_min, unsigned mkey, float m, SampleShared& sh) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0u;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        const unsigned himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int w = 0; w < 4; ++w) sh.hist[w][tid] = 0ull;
        if (tid == 0) { sh.bin = 0u; sh.rest = 0ull; }
        __syncthreads();
        for (int i0 = 0; i0 < V; i0 += 256 * SAMPLE_LOADS) {   // the same trip count for every thread: the ballots need whole waves
            float xv[SAMPLE_LOADS];
#pragma unroll
            for (int u = 0; u < SAMPLE_LOADS; ++u) {
                const int i = i0 + u * 256 + tid;
                xv[u] = i < V ? x[i] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < SAMPLE_LOADS; ++u) {
                const int i = i0 + u * 256 + tid;
                bool valid = i < V;
                unsigned d = 0u;
                sample_u64 wt = 1ull;
                if (valid) {
                    const unsigned key = sample_zkey<PEN>(xv[u], i, bm, seen, pen, temperature, mask);
                    d = COUNT ? ~key : key;
                    if (!COUNT) wt = key >= keep_min ? sample_weight(key, mkey, m) : 0ull;
                    valid = (d & himask) == prefix && wt != 0ull;
                }
                const unsigned bin = (d >> shift) & 255u;
                if (COUNT) sample_count_add(sh.hist[wave], valid, bin, lane);
                else if (valid) atomicAdd(&sh.hist[wave][bin], wt);
            }
        }
        __syncthreads();
        const sample_u64 c = (sh.hist[0][tid] + sh.hist[1][tid]) + (sh.hist[2][tid] + sh.hist[3][tid]);
        sample_u64 total;
        const sample_u64 incl = sample_block_scan(c, tid, sh.ws, &total);
        if (!COUNT && shift == 24) {
            bound = (sample_u64)floor(omp * (double)total);
            if (total > 0ull && bound > total - 1ull) bound = total - 1ull;
        }
        if (incl > bound && incl - c <= bound) { sh.bin = (unsigned)tid; sh.rest = bound - (incl - c); }
        __syncthreads();
        prefix |= sh.bin << shift;
        bound = sh.rest;
        __syncthreads();                                 // sh.bin / sh.rest are reset at the top of the next round
    }
    return prefix;
}
