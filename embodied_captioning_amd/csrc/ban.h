// The ban bitmap of one logits row (ops.h, BanSet), built by the row's 256-thread block in LDS: the static bitmap (tokens banned at
// every step), then every multi-token sequence whose first n - 1 tokens are the tail of the row's history sets its last token's bit.
// Shared by the processed and sampled forms of the greedy selection (elementwise.hip) and the banned and processed modes of the beam
// candidate kernels (beam.hip).
#pragma once
#include "ops.h"

// bm: ban_words(V) words of LDS; hist: the row's context as HF's processor sees it, hlen tokens (oldest first).  HF's rule: a sequence
// of n tokens is looked at when n <= hlen (its n - 1 prefix tokens are then compared with the last n - 1 of the context).  Ends with a barrier: every thread sees the bitmap.
__device__ __forceinline__ void ban_bitmap_fill(unsigned* bm, int V, const BanSet& ban, const int* __restrict__ hist, int hlen, int tid) {
    const int words = ban_words(V);
    for (int w = tid; w < words; w += 256) bm[w] = ban.bits[w];
    __syncthreads();
    for (int j = tid; j < ban.n_multi; j += 256) {
        const int* __restrict__ rec = ban.multi + (size_t)j * BAN_REC;
        const int n = rec[0];
        if (n < 2 || n > BAN_MAX_LEN || n > hlen) continue;
        const int last = rec[n];
        if (last < 0 || last >= V) continue;
        bool hit = true;
        for (int k = 0; k < n - 1; ++k) hit = hit && hist[hlen - (n - 1) + k] == rec[1 + k];
        if (hit) atomicOr(&bm[last >> 5], 1u << (last & 31));
    }
    __syncthreads();
}

// The context of a row as HF's repetition processors see it (ops.h, RepeatCtl): vn virtual copies of vtok, then the stored history
// `real` (rlen tokens, oldest first) whose first token reads as vbos when vbos >= 0.
struct RowContext {
    const int* __restrict__ real;
    int rlen, vn, vtok, vbos;
    __device__ __forceinline__ int len() const { return vn + rlen; }
    __device__ __forceinline__ int at(int j) const { return j < vn ? vtok : (j == vn && vbos >= 0) ? vbos : real[j - vn]; }
};

// The processed form's two bitmaps (ops.h, RepeatCtl): bm = the ban bitmap as ban_bitmap_fill leaves it (zeros where the set has no
// static bitmap) plus the n-gram bans - one n-gram start per thread: the token behind every earlier occurrence of the context's last
// n - 1 tokens (no n-gram exists while the context is shorter than n); seen (null: no penalty) = one bit per distinct context token
// in [0, V).  The ban's own context stays the stored history.  Ends with a barrier.
__device__ __forceinline__ void processed_bitmaps_fill(unsigned* bm, unsigned* seen, int V, const BanSet& ban, int ngram,
                                                       const RowContext& cx, int tid) {
    const int words = ban_words(V);
    if (seen) for (int w = tid; w < words; w += 256) seen[w] = 0u;
    if (ban.bits) {
        ban_bitmap_fill(bm, V, ban, cx.real, cx.rlen, tid);
    } else {
        for (int w = tid; w < words; w += 256) bm[w] = 0u;
        __syncthreads();
    }
    const int c = cx.len();
    if (ngram > 0) {
        const int tail = c - (ngram - 1);
        for (int i = tid; i + ngram <= c; i += 256) {
            bool hit = true;
            for (int k = 0; k < ngram - 1 && hit; ++k) hit = cx.at(i + k) == cx.at(tail + k);
            const int tok = cx.at(i + ngram - 1);
            if (hit && tok >= 0 && tok < V) atomicOr(&bm[tok >> 5], 1u << (tok & 31));
        }
    }
    if (seen) {
        for (int j = tid; j < c; j += 256) {
            const int tok = cx.at(j);
            if (tok >= 0 && tok < V) atomicOr(&seen[tok >> 5], 1u << (tok & 31));
        }
    }
    __syncthreads();
}

// HF's penalty on one score: x < 0 ? x * p : x / p, a true fp32 division (-inf and NaN stay what they are, 0 stays 0)
__device__ __forceinline__ float repeat_penalise(float x, float p) { return x < 0.f ? __fmul_rn(x, p) : __fdiv_rn(x, p); }

// the four ban bits of the float4 chunk that starts at element i (i % 4 == 0: one word holds them), bit u = element i + u
__device__ __forceinline__ unsigned ban_nibble(const unsigned* bm, int i) { return (bm[i >> 5] >> (i & 31)) & 15u; }
__device__ __forceinline__ bool ban_bit(const unsigned* bm, int i) { return ((bm[i >> 5] >> (i & 31)) & 1u) != 0; }
