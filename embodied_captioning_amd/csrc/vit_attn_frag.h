// The steps of the seven MFMA ViT attention kernels (attention.hip).  All of them compute S^T = K.Q^T into 32x32 accumulators, so
// that lane (r32, hh) owns query column r32 and accumulator element e of key block kb is key att_key(kb, e, hh): the softmax
// reductions are in-lane plus one cross-half shuffle, and the S^T registers are fed straight back as the B operand of
// O^T = V^T.P^T.  First the steps that depend on that accumulator layout only, then the operand fragments of the three flavours
// (bf16, exact fp32, split fp16 = G8).  Everything is in an anonymous namespace: include after ops.h.
#pragma once

namespace {

constexpr float LOG2E = 1.4426950408889634f;
typedef short s16x4 __attribute__((ext_vector_type(4)));
#define CAP_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define CAP_LPTR(p) ((__attribute__((address_space(3))) void*)(p))

// ---- the accumulator layout ----
__device__ __forceinline__ int att_key(int kb, int e, int hh) { return kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh; }

__device__ __forceinline__ void att_zero(f32x16& a) {
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = 0.f;
}
template <int NB> __device__ __forceinline__ void att_zero(f32x16 (&o)[NB]) {
#pragma unroll
    for (int db = 0; db < NB; ++db) att_zero(o[db]);
}
__device__ __forceinline__ float att_half_max(float m) { return fmaxf(m, __shfl_xor(m, 32, 64)); }

// which key blocks are compared with N: the last one only (every earlier block is full) or every one (blocks past the end are
// computed as zeros: vit_attention_f32_mfma_wide).  vit_attention_flash_wide, the one kernel with a causal rule on top, and
// vit_attention_split without EXACT keep their own loops on att_key: see there.
enum AttMask { ATT_MASK_LAST, ATT_MASK_ALL };

// mask the padding keys of key block kb (`last` = index of the last block) and fold the block into the running maximum.
// key >= N is tested as att_key(0, e, 0) >= N - att_key(kb, 0, hh): one lane value against 16 inline constants
template <AttMask MASK>
__device__ __forceinline__ void att_mask_max(f32x16& s, int kb, int last, int N, int hh, float& cm) {
    const int nk = N - att_key(kb, 0, hh);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (MASK == ATT_MASK_ALL || kb == last) {
            if (att_key(0, e, 0) >= nk) s[e] = -INFINITY;
        }
        cm = fmaxf(cm, s[e]);
    }
}
// the same over a chunk whose first block is c0; returns the maximum of the query column over the chunk
template <AttMask MASK, int KC>
__device__ __forceinline__ float att_mask_max(f32x16 (&s)[KC], int c0, int last, int N, int hh) {
    float cm = -INFINITY;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) att_mask_max<MASK>(s[kc], c0 + kc, last, N, hh, cm);
    return att_half_max(cm);
}

// online softmax: the new running maximum; the denominator and the context go over to it
template <int NB> __device__ __forceinline__ float att_rescale(float& m, float& l, f32x16 (&o)[NB], float cm, float c1) {
    const float mn = fmaxf(m, cm);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * c1);      // first chunk: exp2(-inf) = 0 and l, o are 0
    l *= alpha;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
    m = mn;
    return mn;
}

// scores -> probabilities of one key block, summed into l (raw v_exp_f32: the inputs are <= 0)
__device__ __forceinline__ void att_exp_sum(f32x16& s, float mn, float c1, float& l) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float p = __builtin_amdgcn_exp2f((s[e] - mn) * c1);
        s[e] = p;
        l += p;
    }
}
template <int KC> __device__ __forceinline__ void att_exp_sum(f32x16 (&s)[KC], float mn, float c1, float& l) {
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) att_exp_sum(s[kc], mn, c1, l);
}

// o / l of query column r32 to columns c0 + d of its context row, d = db*32 + 8*g + 4*hh .. + 3 below `lim` (a multiple of 4)
template <int NB, typename TO>
__device__ __forceinline__ void att_store(TO* row, int c0, const f32x16 (&o)[NB], float l, int hh, int lim = NB * 32) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = db * 32 + 8 * g + 4 * hh;
            if (d < lim)
                store4(row, c0 + d, make_float4(o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv));
        }
}

// two ds_read_b64_tr_b16 results (keys key0 .. +3 and key0 + 8 .. + 11 of one d column) as one MFMA A operand
template <typename V8> __device__ __forceinline__ V8 att_join(s16x4 lo, s16x4 hi) {
    return __builtin_bit_cast(V8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ s16x4 att_read_tr(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}
// transposed-read addressing of the P.V A operand: 16-lane group tg = lane >> 4 handles d columns (tg & 1) * 16 .. + 15 and key
// sub-block 4 * (tg >> 1); inside a group lane 4 tq + tp ADDRESSES row (key) tq, columns 4 tp .. 4 tp + 3 and RECEIVES column
// (lane & 15) of the group's 4 rows.  (The same mapping is spelled tq / tp / tg in vit_attention_flash_wide's written-out P.V
// step and in vit_attention_split_pw's lane bases: change the three together.)
__device__ __forceinline__ int att_tr_dcol(int lane, int db) { return db * 32 + ((lane >> 4) & 1) * 16 + (lane & 3) * 4; }
__device__ __forceinline__ int att_tr_key(int lane) { return 4 * (lane >> 5) + ((lane >> 2) & 3); }

// ---- bf16: K and V of one (image, head) sit in LDS as [key][64] rows of 128 B with the 16-byte-chunk XOR swizzle of the GEMM
// tiles, filled by LDS-DMA (swizzle on the source address); a head wider than 64 is NH = 2 such images, IMG bytes apart, whose
// missing columns are masked off the DMA.  Q.K^T reads K rows with ds_read_b128; P.V needs V "by column" (4 consecutive keys
// for one d per lane): ds_read_b64_tr_b16 delivers exactly that from the row-major image, so V is never transposed in memory.
__device__ __forceinline__ int swz_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// 1 KiB pieces of 8 rows; piece p of K and of V go to wave p % 4.  base = q of (token 0, head), D = k's offset from q
template <int NH>
__device__ __forceinline__ void bf16_stage_kv(char* Ks, char* Vs, int NP, const bf16_t* base, int ld, int D, int N, int hd, int wave, int lane) {
    for (int p = wave; p < NP / 8; p += 4) {
        const int row = p * 8 + (lane >> 3);
        const int gch = (lane & 7) ^ ((row >> 1) & 7);
        const bf16_t* src = base + (size_t)min(row, N - 1) * ld + gch * 8;
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
            if (NH == 1 || hf * 64 + gch * 8 < hd) {       // whole 16-byte chunks: head_dim is a multiple of 8
                __builtin_amdgcn_global_load_lds(CAP_GPTR(src + hf * 64 + D), CAP_LPTR(Ks + hf * NP * 128 + p * 1024), 16, 0, 0);
                __builtin_amdgcn_global_load_lds(CAP_GPTR(src + hf * 64 + 2 * D), CAP_LPTR(Vs + hf * NP * 128 + p * 1024), 16, 0, 0);
            }
        }
    }
}
template <int NH> __device__ __forceinline__ void bf16_load_q(bf16x8 (&qf)[4 * NH], const bf16_t* qrow, int hh, int hd) {
#pragma unroll
    for (int ks = 0; ks < 4 * NH; ++ks) {
        const int col = ks * 16 + hh * 8;
        if (NH == 1 || col < hd) qf[ks] = *(const bf16x8*)(qrow + col);
        else
#pragma unroll
            for (int i = 0; i < 8; ++i) qf[ks][i] = (bf16_t)0.f;
    }
}
// S^T block of key rows row0 .. + 31
template <int NH>
__device__ __forceinline__ void bf16_scores(f32x16& s, const char* Ks, int IMG, int row, int hh, const bf16x8 (&qf)[4 * NH]) {
    att_zero(s);
#pragma unroll
    for (int ks = 0; ks < 4 * NH; ++ks) {
        bf16x8 a = *(const bf16x8*)(Ks + (ks >> 2) * IMG + swz_off(row, (ks & 3) * 2 + hh));
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[ks], s, 0, 0, 0);
    }
}
// O^T += V^T.P^T for the 16 keys kb*32 + 16*s2 .. + 15.  B operand: element j of lane half hh is
// P^T[key = kb*32 + 16*s2 + 8*(j>>2) + 4*hh + (j&3)][q]; A operand: lane (d = db*32 + r32, hh) needs V[key0 .. key0+3][d] and
// V[key0+8 .. +11][d], key0 = kb*32 + 16*s2 + 4*hh
template <int NDB>
__device__ __forceinline__ void bf16_pv(f32x16 (&o)[NDB], const f32x16& p, int s2, const char* Vs, int IMG, int kb, int lane) {
    bf16x8 pb;
#pragma unroll
    for (int j = 0; j < 8; ++j) pb[j] = (bf16_t)p[8 * s2 + j];
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
        const int dcol = att_tr_dcol(lane, db & 1);                    // column inside the 64-wide half db >> 1
        const int key0 = kb * 32 + 16 * s2 + att_tr_key(lane);
        const char* vimg = Vs + (db >> 1) * IMG;
        const s16x4 lo = att_read_tr(vimg + swz_off(key0, dcol >> 3) + (dcol & 7) * 2);
        const s16x4 hi = att_read_tr(vimg + swz_off(key0 + 8, dcol >> 3) + (dcol & 7) * 2);
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_join<bf16x8>(lo, hi), pb, o[db], 0, 0, 0);
    }
}

// ---- exact fp32 (v_mfma_f32_32x32x2_f32): LDS rows of fp32 with a pitch of 4 floats over a multiple of 32.  Lane (r32, hh) reads
// the 16-byte chunk 2 ks + hh of key row r32 (its 4 values feed 4 MFMAs as the k-pair (hh = 0, hh = 1); Q uses the same k
// permutation, so the sum is unchanged) - with such a pitch the 16 lanes of a ds_read_b128 phase hit 16 distinct 4-bank groups.
// k-step ks covers dims 8 ks .. 8 ks + 7; steps at or past nks are zero (Q) or skipped (scores)
template <int NKS> __device__ __forceinline__ void f32_load_q(f32x4 (&qf)[NKS], const float* qrow, int hh, int nks = NKS) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = ks < nks ? *(const f32x4*)(qrow + (2 * ks + hh) * 4) : f32x4(0.f);
}
template <int NKS>
__device__ __forceinline__ void f32_scores(f32x16& s, const float* krow, int hh, const f32x4 (&qf)[NKS], bool on = true, int nks = NKS) {
    att_zero(s);
    if (on) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (ks < nks) {
                const f32x4 a = *(const f32x4*)(krow + (2 * ks + hh) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], qf[ks][j], s, 0, 0, 0);
            }
        }
    }
}
// P.V of one key block whose V rows start at vblk: MFMA #e takes keys {kappa_e, kappa_e + 4} = exactly what accumulator register
// e of the two lane halves holds, so P never leaves its registers; V^T[d][key] is a ds_read_b32 of 32 consecutive floats per half
template <int PITCH, int NDB>
__device__ __forceinline__ void f32_pv(f32x16 (&o)[NDB], const f32x16& p, const float* vblk, int r32, int hh) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int key = att_key(0, e, hh);
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(vblk[key * PITCH + db * 32 + r32], p[e], o[db], 0, 0, 0);
        if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- split fp16: q | k | v arrive as G8, both products run on the fp16 MFMA pipe as hi.lo + lo.hi + hi.hi (common.h).  A head's
// 64 dims of one token are 256 contiguous bytes of the G8 row = 16 chunks [H0 L0 H1 L1 .. H7 L7]; K and V sit in LDS as rows of
// 256 B filled by LDS-DMA with the swizzle applied on the DMA's source address.  Lane (r32, hh) of a 32x32x16 MFMA supplies 8
// consecutive d = group 2 ks + hh: hi chunk 2 (2 ks + hh), lo chunk + 1.
// K: chunk c of row r at slot c ^ (r & 15), so the 16 lanes of a ds_read_b128 phase - 16 consecutive keys, same chunk - hit 16
// different slots.
__device__ __forceinline__ int split_kswz(int row) { return row & 15; }
// V is read by ds_read_b64_tr_b16, served in two groups of 32 lanes: 4 consecutive keys x the 4 same-parity chunks of half a
// row x 8 bytes.  Key r & 15 folds those 16 pieces onto 8 slots (2-way conflict on every V read); keys {0, 1, 8, 9} by r & 3
// send the four rows' chunk sets to {0 2 4 6}, {1 3 5 7}, {8 ..}, {9 ..} (+ 8 for the other half): 16 slots, all 64 banks.
__device__ __forceinline__ int split_vswz(int row) { return (row & 1) | ((row & 2) << 2); }
__device__ __forceinline__ int split_koff(int row, int chunk) { return row * 256 + ((chunk ^ split_kswz(row)) << 4); }
__device__ __forceinline__ int split_voff(int row, int chunk) { return row * 256 + ((chunk ^ split_vswz(row)) << 4); }

// 1 KiB pieces of 4 rows; piece p of K and / or of V go to wave p % 8.  base = byte address of q of (token 0, head); the LDS rows
// are tokens row0 .. row0 + NP - 1
template <bool DO_K, bool DO_V>
__device__ __forceinline__ void split_stage(char* Ks, char* Vs, int NP, const char* base, size_t rowb, int D, int row0, int N, int wave, int lane) {
    for (int p = wave; p < NP / 4; p += 8) {
        const int row = p * 4 + (lane >> 4);
        const char* src = base + (size_t)min(row0 + row, N - 1) * rowb;
        if (DO_K) __builtin_amdgcn_global_load_lds(CAP_GPTR(src + (size_t)D * 4 + ((lane & 15) ^ split_kswz(row)) * 16), CAP_LPTR(Ks + p * 1024), 16, 0, 0);
        if (DO_V) __builtin_amdgcn_global_load_lds(CAP_GPTR(src + (size_t)2 * D * 4 + ((lane & 15) ^ split_vswz(row)) * 16), CAP_LPTR(Vs + p * 1024), 16, 0, 0);
    }
}
__device__ __forceinline__ void split_load_q(f16x8 (&qh)[4], f16x8 (&ql)[4], const char* qrow, int hh) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const char* qp = qrow + (2 * ks + hh) * 32;
        qh[ks] = *(const f16x8*)qp;
        ql[ks] = *(const f16x8*)(qp + 16);
    }
}
// one k-step of S^T from the K fragments at kh / kl
__device__ __forceinline__ void split_qk(f32x16& s, const char* khp, const char* klp, f16x8 qh, f16x8 ql) {
    const f16x8 kh = *(const f16x8*)khp;
    const f16x8 kl = *(const f16x8*)klp;
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh, s, 0, 0, 0);
}
// B operand of P.V: element j of lane half hh is P^T[key = kb*32 + 16*s2 + 8*(j>>2) + 4*hh + (j&3)][q]; P (fp32, in (0, 1]) is
// split in registers
__device__ __forceinline__ void split_p(const f32x16& p, int s2, f16x8& ph, f16x8& pl) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float pv = p[8 * s2 + j];
        const f16_t hv = (f16_t)pv;
        ph[j] = hv;
        pl[j] = (f16_t)(pv - (float)hv);
    }
}
__device__ __forceinline__ void split_pv(f32x16& o, f16x8 vh, f16x8 vl, f16x8 ph, f16x8 pl) {
    o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o, 0, 0, 0);
}

}  // namespace
