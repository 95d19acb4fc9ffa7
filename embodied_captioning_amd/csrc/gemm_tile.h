// Pieces shared by the 256x256 LDS-DMA GEMM kernels of gemm.hip and gemm_pp.hip: MFMA operand traits, the LDS chunk swizzle,
// the epilogue address maps and the register-layout epilogue.  Everything is in an anonymous namespace: include it from a
// translation unit that defines GEMM kernels, nowhere else.
#pragma once
#include <type_traits>

#include "gemm.h"

namespace {

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    using vec = bf16x8;
    static constexpr int EPC = 8;          // elements per 16-byte chunk
    __device__ static __forceinline__ void run(f32x16& acc, const vec& a, const vec& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
    // 16x16x32: lane (r16 = lane & 15, kg = lane >> 4) supplies row r16, k = 8 kg .. 8 kg + 7 of a 32-wide k-step;
    // D[4 kg + e][r16].  Every bf16 GEMM kernel of this file accumulates with THIS instruction, k-steps in ascending
    // order, so a row of C has the same bits whichever tile shape its batch size selects (batch invariance).
    __device__ static __forceinline__ void run16(f32x4& acc, const vec& a, const vec& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    using vec = f32x4;
    static constexpr int EPC = 4;
    __device__ static __forceinline__ void run(f32x16& acc, const vec& a, const vec& b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    }
};

// G8 (split fp16, common.h): a 128-byte slab row holds 32 k values as chunks [H0 L0 H1 L1 H2 L2 H3 L3]; lane (r16, kg)
// of a 16x16x32 MFMA takes the hi chunk 2 kg and the lo chunk 2 kg + 1 of its row, and every product is three MFMAs in
// THIS order (all kernels, so a row of C has the same bits whichever tile shape its batch size selects):
//   acc += a_hi.w_lo;  acc += a_lo.w_hi;  acc += a_hi.w_hi
template <> struct Mma<g8_t> {
    using vec = f16x8;
    static constexpr int EPC = 4;
    __device__ static __forceinline__ void run(f32x16&, const vec&, const vec&) {}     // (32x32 path unused)
    __device__ static __forceinline__ void run16(f32x4& acc, const vec& a, const vec& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
    }
};
template <typename T> constexpr bool is_g8 = std::is_same<T, g8_t>::value;

// XOR key of the 16-byte chunk swizzle of a 128-byte slab row (chunk c of row r is stored at chunk c ^ key(r)); the writers (LDS-DMA
// source address / ds_write of the staging registers) and the fragment reads use the same key.  gfx950 serves a ds_read_b128 in four
// lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59}, {36-43,48-51,60-63} (MI355X_MICROARCH.md, LDS).  For a
// 16x16x32 fragment read (lane = r16 + 16 kg) a group holds rows 0-3 and 12-15 of k-group a and rows 4-11 of k-group a ^ 1, i.e.
// chunks c and c ^ d (G8: d = 2, hi / lo chunks 2 kg, 2 kg + 1; bf16: d = 1, chunks 4 ks + kg): the 16 lanes hit 16 distinct 16-byte
// slots of the 256-byte bank row iff {key(t) : t in {0,1,6,7}} and {d ^ key(t) : t in {2,3,4,5}} (t = (r >> 1) & 7) partition 0..7.
// The plain key t - right for groups of 16 consecutive lanes, the round-1/2 choice - is 2-way conflicted on EVERY such read
// (SQ_LDS_BANK_CONFLICT = half of SQ_LDS_IDX_ACTIVE, tools/pmc_lds.sh).  The bf16 key is a permutation of t, so the 32x32x16 reads
// (32 rows of one chunk per half wave: rows 0-3, 12-15, 20-27 in a group = all eight t) stay conflict-free too.
template <bool G8> __device__ __forceinline__ int swz_key(int row) {
    const int t = (row >> 1) & 7;
    if constexpr (G8) return (t & 1) | ((t >> 2) * 6);   // 0 1 0 1 6 7 6 7
    else return t ^ (((t >> 1) ^ (t >> 2)) & 1);         // 0 1 3 2 5 4 6 7
}
template <bool G8> __device__ __forceinline__ int swz_off(int row, int chunk) { return row * 128 + ((chunk ^ swz_key<G8>(row)) << 4); }

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // NOT HIP's uint4: its union members defeat SROA and
                                                                  // the staging registers end up in scratch

// s_barrier is IntrNoMem for the compiler: pin LDS accesses on their side of it with empty memory-clobber asm
#define CAP_RAW_BARRIER() do { asm volatile("" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)
#define CAP_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define CAP_LPTR(p) ((__attribute__((address_space(3))) void*)(p))

template <int EPI>
__device__ __forceinline__ size_t epi_offset(const GemmParams& p, int row, int col, void*& base) {
    base = p.C;
    if constexpr (EPI == EPI_PARTIAL) {
        return ((size_t)p.p3 * p.M + row) * p.ldc + col;
    } else if constexpr (EPI == EPI_STORE) {
        return (size_t)row * p.ldc + col;
    } else if constexpr (EPI == EPI_PATCH) {
        const int b = row / p.p0, pp = row - b * p.p0;
        return ((size_t)b * (p.p0 + 1) + 1 + pp) * p.ldc + col;
    } else if constexpr (EPI == EPI_CROSSKV) {
        const int NT = p.p0, H = p.p1, B = p.p2, Dh = H * 64;
        const int b = row / NT, t = row - b * NT;
        const int l = col / (2 * Dh), r = col - l * 2 * Dh, kv = r / Dh, hd = r - kv * Dh, h = hd >> 6, d = hd & 63;
        return (((((size_t)l * 2 + kv) * B + b) * H + h) * NT + t) * 64 + d;
    } else {  // EPI_QKVCACHE
        const int H = p.p1, Dh = H * 64;
        if (col < Dh) return (size_t)row * Dh + col;
        const int kv = col / Dh - 1, hd = col % Dh, h = hd >> 6, d = hd & 63;
        base = p.C2;
        return ((((size_t)kv * p.p0 + row) * H + h) * p.p2 + p.p3) * 64 + d;
    }
}
template <typename T, int EPI>
__device__ __forceinline__ void epi_store_raw(const GemmParams& p, int row, int col, u32x4 raw, bool full) {
    void* base;
    const size_t o = epi_offset<EPI>(p, row, col, base);
    if (full) *(u32x4*)((T*)base + o) = raw;
    else *(unsigned long long*)((T*)base + o) = (unsigned long long)raw[0] | ((unsigned long long)raw[1] << 32);   // N % 8 == 4 tail
}
template <int EPI>
__device__ __forceinline__ void epi_store_f32(const GemmParams& p, int row, int col, f32x4 v) {
    if constexpr (EPI == EPI_PATCH) {
        const int pp = row % p.p0;
        v += *(const f32x4*)(p.aux + (size_t)(1 + pp) * p.N + col);
    }
    void* base;
    const size_t o = epi_offset<EPI>(p, row, col, base);
    *(f32x4*)((float*)base + o) = v;
}

// Epilogue shared by the second-generation kernels.  acc[i][j][e] = C[row0 + 16 i + r16][col0 + 16 j + 4 kg + e]: bias /
// GELU / convert in that layout, then a wave-private LDS strip (16 rows x 128 payload bytes, row pitch 144) turns "4
// consecutive columns per lane" into "16 consecutive bytes per lane, 8 lanes per 128-byte row": every global store
// instruction writes 8 whole cache lines.  The strip is outside the stage buffers, so no barrier is involved.
// bias_w: LDS address of the fp32 bias of this wave's first column (nullptr: none).
template <typename T, bool OUT_F32, int EPI, int MI, int NI>
__device__ __forceinline__ void big2_epilogue(const GemmParams& p, const f32x4 (&acc)[MI][NI], char* strip,
                                              const char* bias_w, int row0, int col0, int lane) {
    const int r16 = lane & 15, kg = lane >> 4;
    const int act = EPI != EPI_PARTIAL ? p.gelu : 0;     // uniform: 1 = exact-erf GELU, 2 = ReLU
    f32x4 biasv[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) biasv[j] = bias_w ? *(const f32x4*)(bias_w + (j * 16 + 4 * kg) * 4) : f32x4(0.f);
    const int srow = lane >> 3, spiece = lane & 7;
    constexpr bool F32OUT = OUT_F32 || EPI == EPI_PARTIAL || EPI == EPI_PATCH;
    constexpr bool G8OUT = !F32OUT && is_g8<T>;         // 4 bytes per element like fp32: 32 columns = four [hi | lo] groups
    static_assert(!G8OUT || EPI == EPI_STORE, "G8 output exists for plain row-major stores only");
    constexpr int NPB = (F32OUT || G8OUT) ? 2 : 4;      // 16-column blocks per 128-byte strip row
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int jp = 0; jp < NI / NPB; ++jp) {
#pragma unroll
            for (int jj = 0; jj < NPB; ++jj) {
                const int j = jp * NPB + jj;
                f32x4 v = acc[i][j];
                if constexpr (is_g8<T>) v *= (1.0f / G8_WSCALE);
                if (EPI != EPI_PARTIAL) v += biasv[j];
                if (act == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_for<T>(v[e]);
                } else if (act == 2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                } else if (act == 3) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = quick_gelu(v[e]);
                }
                if constexpr (F32OUT) {
                    *(f32x4*)(strip + r16 * 144 + (jj * 16 + 4 * kg) * 4) = v;
                } else if constexpr (G8OUT) {
                    store4((g8_t*)(strip + r16 * 144), jj * 16 + 4 * kg, make_float4(v[0], v[1], v[2], v[3]));
                } else {
                    bf16x4 w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[e] = (bf16_t)v[e];
                    *(bf16x4*)(strip + r16 * 144 + (jj * 16 + 4 * kg) * 2) = w;
                }
            }
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int row = row0 + i * 16 + rr * 8 + srow;
                if constexpr (F32OUT) {
                    const f32x4 v = *(const f32x4*)(strip + (rr * 8 + srow) * 144 + spiece * 16);
                    const int col = col0 + jp * 32 + spiece * 4;
                    if (row < p.M && col < p.N) epi_store_f32<EPI>(p, row, col, v);
                } else if constexpr (G8OUT) {
                    // the strip row is the 128-byte image of 32 G8 elements: copy it out as it is (N % 8 == 0: a group's
                    // two 16-byte pieces are inside or outside together)
                    const u32x4 raw = *(const u32x4*)(strip + (rr * 8 + srow) * 144 + spiece * 16);
                    const int col = col0 + jp * 32 + spiece * 4;
                    if (row < p.M && col < p.N) epi_store_raw<T, EPI>(p, row, col, raw, true);
                } else {
                    const u32x4 raw = *(const u32x4*)(strip + (rr * 8 + srow) * 144 + spiece * 16);
                    const int col = col0 + jp * 64 + spiece * 8;
                    if (row < p.M && col < p.N) epi_store_raw<T, EPI>(p, row, col, raw, col + 8 <= p.N);
                }
            }
        }
    }
}

}  // namespace
