// The ban bitmap of one logits row (ops.h, BanSet), built by the row's 256-thread block in LDS: the static bitmap (tokens banned at
// every step), then every multi-token sequence whose first n - 1 tokens are the tail of the row's history sets its last token's bit.
// Shared by the banned forms of the greedy selection (elementwise.hip) and of the beam candidate kernels (beam.hip).
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

// the four ban bits of the float4 chunk that starts at element i (i % 4 == 0: one word holds them), bit u = element i + u
__device__ __forceinline__ unsigned ban_nibble(const unsigned* bm, int i) { return (bm[i >> 5] >> (i & 31)) & 15u; }
__device__ __forceinline__ bool ban_bit(const unsigned* bm, int i) { return ((bm[i >> 5] >> (i & 31)) & 1u) != 0; }
