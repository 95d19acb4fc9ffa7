// HBM-bound helper kernels of the captioner path: dtype casts, patch gather, LayerNorm, decoder embeddings,
// greedy token selection.  One wave (64 lanes) per row for the row-wise ops; 16-byte accesses where the layout allows.
#include <algorithm>
#include <cmath>
#include "ops.h"
#include "ban.h"
#include "sample.h"

namespace {

// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void convert_kernel(const float* __restrict__ src, T* __restrict__ dst, size_t n) {
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) store4(dst + (i & ~(size_t)7), (int)(i & 7), *(const float4*)(src + i));
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (size_t j = n & ~(size_t)3; j < n; ++j) store1(dst + (j & ~(size_t)7), (int)(j & 7), src[j]);
}

// scale: 1 except for G8 weights (G8_WSCALE, see common.h)
template <typename T>
__global__ void convert2d_kernel(const float* __restrict__ src, T* __restrict__ dst, int rows, int cols, int dst_ld, float scale) {
    const size_t n = (size_t)rows * cols;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / cols, c = i - r * cols;
        store1(dst + r * dst_ld, (int)c, src[i] * scale);
    }
}

template <typename T>
__global__ void convert2d_t_kernel(const float* __restrict__ src, T* __restrict__ dst, int rows, int cols, float scale) {
    // dst[c][r] = src[r][c]  (one-off weight transposition, e.g. CoCa's text_projection [width, vocab])
    const size_t n = (size_t)rows * cols;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t c = i / rows, r = i - c * rows;
        store1(dst + c * rows, (int)r, src[r * cols + c] * scale);
    }
}

// ------------------------------------------------------------------------------------------------
// One thread per output element; consecutive threads walk x inside an image row, so the pixel reads are
// coalesced (fp32 NCHW: 4 B/lane contiguous; u8 NHWC: 3 B stride) and each thread writes one element of the
// patch matrix.  k = c*ps*ps + dy*ps + dx  (== Conv2d weight [D,3,ps,ps] flattened).
template <typename T>
__global__ void patchify_kernel(const void* __restrict__ pixels, int fmt, int B, int img, int ps, int Kpad,
                                T* __restrict__ out, float m0, float m1, float m2, float s0, float s1, float s2) {
    const int G = img / ps;
    const size_t total = (size_t)B * 3 * img * img;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int x = (int)(i % img);
        size_t r = i / img;
        int y = (int)(r % img); r /= img;
        int c = (int)(r % 3);
        int b = (int)(r / 3);
        float v;
        if (fmt == 0) {
            v = ((const float*)pixels)[i];
        } else {
            unsigned char u = ((const unsigned char*)pixels)[(((size_t)b * img + y) * img + x) * 3 + c];
            float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
            v = ((float)u * (1.0f / 255.0f) - mean) / sd;
        }
        int py = y / ps, dy = y - py * ps, px = x / ps, dx = x - px * ps;
        size_t row = (size_t)b * G * G + (size_t)py * G + px;
        store1(out + row * Kpad, c * ps * ps + dy * ps + dx, v);
    }
}

__global__ void cls_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ X,
                                int B, int tokens, int D) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    int b = i / D, d = i - b * D;
    X[(size_t)b * tokens * D + d] = cls[d] + pos[d];
}

#include "ln.h"   // LN_MAXV, ln_row

template <typename T, int MAXV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ in, int ld_in,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, T* out_t, float* out_f, int M, int D,
                                                        const int* __restrict__ n_rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M || (n_rows && row >= *n_rows)) return;      // n_rows: RowMap::n, rows from the count on are left alone
    const int nv = (D + 255) / 256;
    float4 v[MAXV];
    const float* x = in + (size_t)row * ld_in;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < nv && lane * 4 + i * 256 < D) v[i] = *(const float4*)(x + lane * 4 + i * 256);
    ln_row<T, MAXV>(v, nv, lane, D, gamma, beta, eps, out_t ? out_t + (size_t)row * D : nullptr,
              out_f ? out_f + (size_t)row * D : nullptr);
}

// Consumer of a split-K GEMM (EPI_PARTIAL): y = sum_z partial[z] + bias + resid, summed in slice order (deterministic),
// then LayerNorm -> out_f (fp32 residual stream) and out_t (next GEMM's A operand).
// part: fp32 partial sums - S split-K slices, or one branch output (the ViT blocks' `delta`).
template <typename T, int MAXV>
__global__ __launch_bounds__(256) void reduce_layernorm_kernel(const float* __restrict__ part, int S,
                                                                const float* __restrict__ bias,
                                                                const float* __restrict__ resid,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps, T* out_t,
                                                                float* out_f, float* y_out, int M, int D,
                                                                const int* __restrict__ n_rows) {
#pragma clang fp contract(off)      // sums and LayerNorm as written: the three consumers of a row count range agree bit for bit
    // one wave per row.  Decode (a few hundred rows) launches one wave per block so every row gets its own CU slot and
    // all of its S*nv + 2*nv 16-byte loads are issued before the first add; the encoder launches 4 rows per block.
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M || (n_rows && row >= *n_rows)) return;
    const int nv = (D + 255) / 256;
    float4 v[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane * 4 + i * 256;
        if (i < nv && c < D) {
            float4 a = *(const float4*)(part + (size_t)row * D + c);
            if (S == 4) {
                const float4 b1 = *(const float4*)(part + ((size_t)1 * M + row) * D + c);
                const float4 b2 = *(const float4*)(part + ((size_t)2 * M + row) * D + c);
                const float4 b3 = *(const float4*)(part + ((size_t)3 * M + row) * D + c);
                a.x = ((a.x + b1.x) + b2.x) + b3.x; a.y = ((a.y + b1.y) + b2.y) + b3.y;
                a.z = ((a.z + b1.z) + b2.z) + b3.z; a.w = ((a.w + b1.w) + b2.w) + b3.w;
            } else {
#pragma unroll 4
                for (int z = 1; z < S; ++z) {
                    const float4 b = *(const float4*)(part + ((size_t)z * M + row) * D + c);
                    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
                }
            }
            if (bias) { const float4 b = *(const float4*)(bias + c); a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
            if (resid) {
                const float4 b = *(const float4*)(resid + (size_t)row * D + c);
                a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            }
            v[i] = a;
            if (y_out) *(float4*)(y_out + (size_t)row * D + c) = a;     // pre-LN residual stream (ViT blocks)
        }
    }
    ln_row<T, MAXV>(v, nv, lane, D, gamma, beta, eps, out_t ? out_t + (size_t)row * D : nullptr,
              out_f ? out_f + (size_t)row * D : nullptr);
}

// Decode-sized variant (a few hundred rows): one 256-thread block per row, one float4 per thread, every partial / bias /
// residual / gamma / beta load issued before the first add -> one memory round trip, then two LDS cross-wave reductions.
// Same summation order over slices as the wave-per-row kernel.
template <typename T>
__global__ __launch_bounds__(256) void reduce_layernorm_row_kernel(const float* __restrict__ part, int S,
                                                                    const float* __restrict__ bias,
                                                                    const float* __restrict__ resid,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps, T* out_t,
                                                                    float* out_f, float* y_out, int M, int D,
                                                                    const int* __restrict__ n_rows) {
#pragma clang fp contract(off)
    __shared__ float sp[2][256];
    const int row = blockIdx.x, tid = threadIdx.x, c = tid * 4;
    if (n_rows && row >= *n_rows) return;                // (uniform over the block: before any barrier)
    const bool act = c < D;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pz[8], bb = z4, rr = z4, g = z4, be = z4;
#pragma unroll
    for (int z = 0; z < 8; ++z) pz[z] = (act && z < S) ? *(const float4*)(part + ((size_t)z * M + row) * D + c) : z4;
    if (act) {
        if (bias) bb = *(const float4*)(bias + c);
        if (resid) rr = *(const float4*)(resid + (size_t)row * D + c);
        g = *(const float4*)(gamma + c);
        be = *(const float4*)(beta + c);
    }
    float4 a = pz[0];
#pragma unroll
    for (int z = 1; z < 8; ++z)
        if (z < S) { a.x += pz[z].x; a.y += pz[z].y; a.z += pz[z].z; a.w += pz[z].w; }
    for (int z = 8; z < S; ++z) {
        const float4 b = act ? *(const float4*)(part + ((size_t)z * M + row) * D + c) : z4;
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if (bias) { a.x += bb.x; a.y += bb.y; a.z += bb.z; a.w += bb.w; }
    if (resid) { a.x += rr.x; a.y += rr.y; a.z += rr.z; a.w += rr.w; }
    if (act && y_out) *(float4*)(y_out + (size_t)row * D + c) = a;
    // statistics in exactly the wave-per-row kernel's order (thread j + 64 i holds that kernel's lane j, vector i), so a
    // row normalises to the same bits whichever kernel the row count selects (batch invariance)
    const int lane = tid & 63;
    sp[0][tid] = act ? a.x + a.y + a.z + a.w : 0.f;
    __syncthreads();
    const float mean = wave_sum(((sp[0][lane] + sp[0][64 + lane]) + sp[0][128 + lane]) + sp[0][192 + lane]) / (float)D;
    const float dx = a.x - mean, dy = a.y - mean, dz = a.z - mean, dw = a.w - mean;
    sp[1][tid] = act ? dx * dx + dy * dy + dz * dz + dw * dw : 0.f;
    __syncthreads();
    const float rstd =
        1.0f / sqrtf(wave_sum(((sp[1][lane] + sp[1][64 + lane]) + sp[1][128 + lane]) + sp[1][192 + lane]) / (float)D + eps);
    if (act) {
        float4 o;
        o.x = dx * rstd * g.x + be.x; o.y = dy * rstd * g.y + be.y; o.z = dz * rstd * g.z + be.z; o.w = dw * rstd * g.w + be.w;
        if (out_f) *(float4*)(out_f + (size_t)row * D + c) = o;
        if (out_t) store4(out_t + (size_t)row * D, c, o);
    }
}

// The same consumer for rows wider than 1024 (OPT-2.7b: 2560) when there are only a few of them (a decode step: 32 rows):
// one 256-thread workgroup per row, up to 3 vectors per thread, every slice load in flight at once.  (The wave-per-row
// kernel walks such a row with 64 lanes: 19 us per launch at 32 x 2560 x 4 slices, measured; this one is bound by the launch.)
template <typename T>
__global__ __launch_bounds__(256) void reduce_layernorm_wide_kernel(const float* __restrict__ part, int S,
                                                                     const float* __restrict__ bias,
                                                                     const float* resid,   // may alias y_out (in-place residual stream)
                                                                     const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float eps, T* out_t,
                                                                     float* out_f, float* y_out, int M, int D) {
#pragma clang fp contract(off)
    __shared__ float sp[2][4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a[3];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = tid * 4 + i * 1024;
        a[i] = z4;
        if (c < D) {
            float4 pz[4];                          // the first four slices are loaded before the first add
#pragma unroll
            for (int z = 0; z < 4; ++z) pz[z] = z < S ? *(const float4*)(part + ((size_t)z * M + row) * D + c) : z4;
            a[i] = pz[0];
#pragma unroll
            for (int z = 1; z < 4; ++z)
                if (z < S) { a[i].x += pz[z].x; a[i].y += pz[z].y; a[i].z += pz[z].z; a[i].w += pz[z].w; }
            for (int z = 4; z < S; ++z) {
                const float4 b = *(const float4*)(part + ((size_t)z * M + row) * D + c);
                a[i].x += b.x; a[i].y += b.y; a[i].z += b.z; a[i].w += b.w;
            }
            if (bias) { const float4 b = *(const float4*)(bias + c); a[i].x += b.x; a[i].y += b.y; a[i].z += b.z; a[i].w += b.w; }
            if (resid) { const float4 b = *(const float4*)(resid + (size_t)row * D + c); a[i].x += b.x; a[i].y += b.y; a[i].z += b.z; a[i].w += b.w; }
            if (y_out) *(float4*)(y_out + (size_t)row * D + c) = a[i];
            s += (a[i].x + a[i].y) + (a[i].z + a[i].w);
        }
    }
    s = wave_sum(s);
    if (lane == 0) sp[0][wv] = s;
    __syncthreads();
    const float mean = (((sp[0][0] + sp[0][1]) + sp[0][2]) + sp[0][3]) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (tid * 4 + i * 1024 < D) {
            const float dx = a[i].x - mean, dy = a[i].y - mean, dz = a[i].z - mean, dw = a[i].w - mean;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    q = wave_sum(q);
    if (lane == 0) sp[1][wv] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf((((sp[1][0] + sp[1][1]) + sp[1][2]) + sp[1][3]) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = tid * 4 + i * 1024;
        if (c < D) {
            const float4 g = *(const float4*)(gamma + c), be = *(const float4*)(beta + c);
            float4 o;
            o.x = (a[i].x - mean) * rstd * g.x + be.x; o.y = (a[i].y - mean) * rstd * g.y + be.y;
            o.z = (a[i].z - mean) * rstd * g.z + be.z; o.w = (a[i].w - mean) * rstd * g.w + be.w;
            if (out_f) *(float4*)(out_f + (size_t)row * D + c) = o;
            if (out_t) store4(out_t + (size_t)row * D, c, o);
        }
    }
}

// One decoder embedding row: LayerNorm(word[tok] + pos[t]) -> out_t / out_f row `row`, the raw sum -> y_out (pre-LN residual stream).
// The single step (embed_kernel) and the prompt prefill (embed_prompt_kernel) both run THIS body: same loads, sums and LayerNorm.
template <typename T>
__device__ __forceinline__ void embed_row(int tok, int t, int row, int lane, const float* __restrict__ word, const float* __restrict__ pos,
                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps, T* out_t,
                                          float* out_f, float* y_out, int D) {
    const int nv = (D + 255) / 256;
    float4 v[LN_MAXV];
    const float* w = word + (size_t)tok * D;
    const float* p = pos + (size_t)t * D;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane * 4 + i * 256;
        if (i < nv && c < D) {
            float4 a = *(const float4*)(w + c), b = *(const float4*)(p + c);
            v[i].x = a.x + b.x; v[i].y = a.y + b.y; v[i].z = a.z + b.z; v[i].w = a.w + b.w;
            if (y_out) *(float4*)(y_out + (size_t)row * D + c) = v[i];      // raw sum = pre-LN residual stream (CoCa)
        }
    }
    ln_row<T>(v, nv, lane, D, gamma, beta, eps, out_t ? out_t + (size_t)row * D : nullptr,
              out_f ? out_f + (size_t)row * D : nullptr);
}

template <typename T>
__global__ __launch_bounds__(256) void embed_kernel(const int* __restrict__ seq, int seq_ld, int t,
                                                    const float* __restrict__ word, const float* __restrict__ pos,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, T* out_t, float* out_f, float* y_out, int R, int D, RowMap map) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;      // (compact) output row
    if (row >= R || (map.n && row >= *map.n)) return;
    const int tok = seq[(size_t)(map.live ? map.live[row] : row) * seq_ld + t];
    embed_row<T>(tok, t, row, lane, word, pos, gamma, beta, eps, out_t, out_f, y_out, D);
}

// Prompt prefill (captioner.hip, run_prefill): the rows of several KNOWN positions at once.  Row r of the launch is position
// r % npos of caption row0 + r / npos (caption-major: the npos rows of an image are adjacent, as the beams of an image are).
template <typename T>
__global__ __launch_bounds__(256) void embed_prompt_kernel(const int* __restrict__ seq, int seq_ld, int npos, int row0,
                                                           const float* __restrict__ word, const float* __restrict__ pos,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, T* out_t, float* out_f, float* y_out, int R, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const int cap = row0 + row / npos, t = row - (row / npos) * npos;
    embed_row<T>(seq[(size_t)cap * seq_ld + t], t, row, lane, word, pos, gamma, beta, eps, out_t, out_f, y_out, D);
}

// The sequence rows of a prompted greedy call: columns 0 .. P - 1 the prompt (one row shared by every caption, or one row per
// caption), pad after it; ids are caller data and are clamped to the table, so nothing outside it is ever gathered.
__global__ void init_prompt_seq_kernel(int* seq, int* fin, int* len, int R, int L, const int* __restrict__ prompt, int prompt_rows,
                                       int P, int V, int pad) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < R * L; i += gridDim.x * blockDim.x) {
        const int r = i / L, j = i - r * L;
        seq[i] = j < P ? min(max(prompt[(size_t)(prompt_rows == 1 ? 0 : r) * P + j], 0), V - 1) : pad;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < R; i += gridDim.x * blockDim.x) { fin[i] = 0; len[i] = L; }
}

// Sentence-encoder input embeddings (HF BertEmbeddings, HF:models/bert/modeling_bert.py `BertEmbeddings.forward`):
// (word[id] + token_type[0]) + position[l], then LayerNorm.  One wave per token row; row = b * L + l.
template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int* __restrict__ ids, int L,
                                                           const float* __restrict__ word, const float* __restrict__ pos,
                                                           const float* __restrict__ type0,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, T* out_t, float* out_f, int R, int D, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const int tok = min(max(ids[row], 0), V - 1), l = row % L;      // ids are caller data: never index outside the table
    const int nv = (D + 255) / 256;
    float4 v[LN_MAXV];
    const float* w = word + (size_t)tok * D;
    const float* p = pos + (size_t)l * D;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane * 4 + i * 256;
        if (i < nv && c < D) {
            const float4 a = *(const float4*)(w + c), t = *(const float4*)(type0 + c), b = *(const float4*)(p + c);
            v[i].x = (a.x + t.x) + b.x; v[i].y = (a.y + t.y) + b.y; v[i].z = (a.z + t.z) + b.z; v[i].w = (a.w + t.w) + b.w;
        }
    }
    ln_row<T>(v, nv, lane, D, gamma, beta, eps, out_t + (size_t)row * D, out_f + (size_t)row * D);
}

// sentence-transformers Pooling(mean over the attention mask) + Normalize (F.normalize, eps 1e-12): one block per
// sentence, one thread per 4 columns.
__global__ __launch_bounds__(256) void mean_pool_normalize_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                                  int L, int D, float* __restrict__ out) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, c = tid * 4;
    const int n = min(max(lens[b], 1), L);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < D)
        for (int l = 0; l < n; ++l) {
            const float4 v = *(const float4*)(x + ((size_t)b * L + l) * D + c);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
    const float inv = 1.0f / (float)n;
    a.x *= inv; a.y *= inv; a.z *= inv; a.w *= inv;
    float q = wave_sum(c < D ? a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w : 0.f);
    if ((tid & 63) == 0) red[tid >> 6] = q;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(((red[0] + red[1]) + red[2]) + red[3]), 1e-12f);
    if (c < D) {
        a.x /= nrm; a.y /= nrm; a.z /= nrm; a.w /= nrm;
        *(float4*)(out + (size_t)b * D + c) = a;
    }
}

// ------------------------------------------------------------------------------------------------
// Greedy step (HF:generation/utils.py:2925-2937): next = argmax (first maximal index, like torch.argmax);
// finished rows emit pad; a row finishes when it emits EOS or reaches max_len.
//
// The selection is shared by every arg-max form: block argmax over one logits row (EOS masked while
// mask_eos): the row's maximum in sv[0] for every thread after the last barrier, its index returned to every thread.
// A row with no entry above -inf (all -inf, or finite only at a masked EOS) selects index 0, as torch.argmax does; a NaN never
// compares greater, so it is never selected (ops.h, SelectStep).
// BAN (the processed form): bm = the row's ban bitmap in LDS (ban.h), a set bit stands as -inf does.
// PEN (the processed form with a repetition penalty): seen = the bitmap of the row's context tokens, whose scores are penalised
// (ban.h, repeat_penalise) before the bans, as HF orders its processors.
template <bool BAN = false, bool PEN = false>
__device__ __forceinline__ int greedy_row_argmax(const float* __restrict__ x, int V, int eos, bool mask_eos, int tid,
                                                  float* sv, int* si, const unsigned* bm = nullptr, const unsigned* seen = nullptr,
                                                  float pen = 1.f, bool vec = true) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    // 16-byte loads, 4 independent chunks in flight per thread; ascending index order inside a thread keeps "first
    // maximal index" with a strict > compare
    const int V4 = vec ? V >> 2 : 0;                     // vec = false (a row that is not 16-byte aligned): every element by the tail loop
    for (int c0 = tid; c0 < V4; c0 += 1024) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * 256;
            v[u] = c < V4 ? *(const float4*)(x + 4 * c) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = 4 * (c0 + u * 256);
            if (mask_eos) {          // component-wise: a dynamic index would push v[] into scratch
                if (eos == i) v[u].x = -INFINITY;
                if (eos == i + 1) v[u].y = -INFINITY;
                if (eos == i + 2) v[u].z = -INFINITY;
                if (eos == i + 3) v[u].w = -INFINITY;
            }
            if (PEN) {
                const unsigned nib = c0 + u * 256 < V4 ? ban_nibble(seen, i) : 0u;
                if (nib & 1u) v[u].x = repeat_penalise(v[u].x, pen);
                if (nib & 2u) v[u].y = repeat_penalise(v[u].y, pen);
                if (nib & 4u) v[u].z = repeat_penalise(v[u].z, pen);
                if (nib & 8u) v[u].w = repeat_penalise(v[u].w, pen);
            }
            if (BAN) {               // the chunk's four bits come from one LDS word
                const unsigned nib = c0 + u * 256 < V4 ? ban_nibble(bm, i) : 0u;
                if (nib & 1u) v[u].x = -INFINITY;
                if (nib & 2u) v[u].y = -INFINITY;
                if (nib & 4u) v[u].z = -INFINITY;
                if (nib & 8u) v[u].w = -INFINITY;
            }
            if (v[u].x > best) { best = v[u].x; bi = i; }
            if (v[u].y > best) { best = v[u].y; bi = i + 1; }
            if (v[u].z > best) { best = v[u].z; bi = i + 2; }
            if (v[u].w > best) { best = v[u].w; bi = i + 3; }
        }
    }
    for (int i = (V4 << 2) + tid; i < V; i += 256) {
        float v = x[i];
        if (PEN && ban_bit(seen, i)) v = repeat_penalise(v, pen);
        if ((mask_eos && i == eos) || (BAN && ban_bit(bm, i))) v = -INFINITY;
        if (v > best) { best = v; bi = i; }
    }
    sv[tid] = best; si[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            float v2 = sv[tid + o]; int i2 = si[tid + o];
            if (v2 > sv[tid] || (v2 == sv[tid] && i2 < si[tid])) { sv[tid] = v2; si[tid] = i2; }
        }
        __syncthreads();
    }
    return si[0] == 0x7fffffff ? 0 : si[0];              // no winner: the sentinel never leaves this function
}

// One thread appends the row's token and keeps finished / out_len; returns whether the row was open at this step.
__device__ __forceinline__ bool greedy_row_emit(const SelectRows& a, int row, int best_i) {
    int fin = a.finished[row];
    int tok = fin ? a.pad : best_i;
    if (!fin && a.force_eos && a.t + 2 >= a.max_len) tok = a.eos;
    a.seq[(size_t)row * a.seq_ld + a.t + 1] = tok;
    if (!fin) {
        if (tok == a.eos || a.t + 2 >= a.max_len) { a.finished[row] = 1; a.out_len[row] = a.t + 2; }
        // the reference's CoCa loop also stops a row whose newest token IS the pad id (coca_model.py:305: `mask =
        // last == eos | last == pad`; pad id 0 is an ordinary vocabulary entry there): it emits pad from then on and
        // gets no EOS.  The row's length then excludes that pad.
        else if (a.force_eos && tok == a.pad) { a.finished[row] = 1; a.out_len[row] = a.t + 1; }
    }
    return !fin;
}

// What every selection kernel starts from (ops.h, SelectRows): block crow's logits row x, the caption `row` it belongs to, whether
// min_len still masks EOS, and whether x takes 16-byte loads.  False: a compact row past the open ones (uniform over the block, so
// the kernel returns before any barrier).
struct SelectRow {
    int row;
    bool mask_eos, vec;
    const float* x;
};
__device__ __forceinline__ bool select_row_begin(const SelectRows& a, SelectRow& r) {
    const int crow = blockIdx.x;
    if (a.map.n && crow >= *a.map.n) return false;
    r.row = a.map.live ? a.map.live[crow] : crow;
    // min_len > 0: EOS cannot win while the row has fewer than min_len tokens (HF MinLengthLogitsProcessor, used by the
    // reference's CoCa loop coca_model.py:235-240); force_eos (= "this is the CoCa loop"): the last position is EOS
    // (coca_model.py:317-318) and a sampled pad id ends the row (:305)
    r.mask_eos = a.min_len > 0 && a.t + 1 < a.min_len;
    r.vec = (a.ld & 3) == 0 && ((uintptr_t)a.logits & 15) == 0;
    r.x = a.logits + (size_t)crow * a.ld;
    return true;
}

__global__ __launch_bounds__(256) void greedy_select_kernel(SelectRows a) {
    const int tid = threadIdx.x;
    SelectRow r;
    if (!select_row_begin(a, r)) return;
    __shared__ float sv[256];
    __shared__ int si[256];
    const int imax = greedy_row_argmax(r.x, a.V, a.eos, r.mask_eos, tid, sv, si, nullptr, nullptr, 1.f, r.vec);
    if (tid == 0) greedy_row_emit(a, r.row, imax);
}

// Processed form (ops.h, BanSet, RepeatCtl): HF's repetition controls and NoBadWordsLogitsProcessor ahead of the arg-max.  The block
// builds the row's ban bitmap in LDS - the static bitmap, the multi-token sequences matched against the caption's history
// seq[row][hist0 .. t], the n-gram bans - and the selection above runs with it; the penalty reads a second bitmap ("seen", behind it in
// the dynamic LDS when PEN).  The row's context is RowContext's.  Finished rows, the tie rule, RowMap and force_eos are
// greedy_select_kernel's, from the same functions.
// CTL = false (a ban set alone, PEN = false): the bitmap is ban_bitmap_fill's - what processed_bitmaps_fill leaves with neutral
// controls, one barrier sooner.  At 256 rows x 30 524 a ban alone through CTL = true took 0.17 us per launch more than the separate
// banned kernel this form replaced (10.42 against 10.25 us, spread 0.02 us), and takes none more this way (docs/experiments.md).
template <bool PEN, bool CTL = true>
__global__ __launch_bounds__(256) void greedy_select_processed_kernel(SelectRows a, BanSet ban, int hist0, RepeatCtl ctl) {
    const int tid = threadIdx.x;
    SelectRow r;
    if (!select_row_begin(a, r)) return;
    extern __shared__ unsigned ban_bm[];                 // ban_words(V) words, twice with PEN
    __shared__ float sv[256];
    __shared__ int si[256];
    unsigned* seen = PEN ? ban_bm + ban_words(a.V) : nullptr;
    const RowContext cx{a.seq + (size_t)r.row * a.seq_ld + hist0, max(a.t + 1 - hist0, 0), ctl.vn, ctl.vtok, ctl.vbos};
    if (CTL) processed_bitmaps_fill(ban_bm, seen, a.V, ban, ctl.ngram, cx, tid);
    else ban_bitmap_fill(ban_bm, a.V, ban, cx.real, cx.rlen, tid);
    const int imax = greedy_row_argmax<true, PEN>(r.x, a.V, a.eos, r.mask_eos, tid, sv, si, ban_bm, seen, ctl.penalty, r.vec);
    if (tid == 0) greedy_row_emit(a, r.row, imax);
}

// Sampled form (ops.h, SampleCtl): the processed form with a draw from the row's distribution in place of the arg-max.  On the
// processed scores s (penalty, bans; banned and NaN = -inf), in this order:
//   z = s / T (fp32, a true division)                       top-k: keep z >= the k-th largest value, ties included (0 or >= V: off)
//   w = (uint64)(expf(z - max z) * 2^40) on what is kept    top-p: W = sum w, R = floor((1 - (double)top_p) * (double)W); a value v stays
//                                                           iff sum_{z_j <= v} w_j > R; the maximum always stays (1: off)
//   draw: U = Philox4x32-10 (sample.h) of (seed, the caption's key, draw); r = mulhi64(U, sum of the remaining w); the token is the
//   smallest id i with sum_{j <= i} w_j > r.  A row with nothing left selects 0, as the arg-max forms do.
// From the weights on all arithmetic is integer (LDS integer atomics, an integer scan), so the token depends on the row, the
// parameters, seed, key and draw alone - not on the grid, the row's position or the RowMap.  A token whose weight is below 2^-40 of
// the maximal one has w = 0 and is never drawn.
// Reads of the row (from L2 after the first; a row is at most 200 KB): 1 for the maximum, 4 per cut that is on (one per radix byte,
// sample.h), 1 for the draw's per-thread sums (thread t owns the ids [t * S, (t + 1) * S), S = ceil(V / 256)) and one thread's walk
// over its S entries: 2 + 1/256 with both cuts off, 10 + 1/256 with both on.  No float atomics; no early return after the bitmaps.
template <bool PEN>
__global__ __launch_bounds__(256) void greedy_select_sampled_kernel(SelectRows a, BanSet ban, int hist0, RepeatCtl ctl, SampleCtl sc,
                                                                    const unsigned long long* __restrict__ keys, int draw,
                                                                    int* __restrict__ out_kept) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
    SelectRow sr;
    if (!select_row_begin(a, sr)) return;
    const int row = sr.row, mask = sr.mask_eos ? a.eos : -1;
    extern __shared__ unsigned ban_bm[];                 // ban_words(V) words, twice with PEN
    __shared__ SampleShared sh;
    unsigned* seen = PEN ? ban_bm + ban_words(V) : nullptr;
    const RowContext cx{a.seq + (size_t)row * a.seq_ld + hist0, max(a.t + 1 - hist0, 0), ctl.vn, ctl.vtok, ctl.vbos};
    processed_bitmaps_fill(ban_bm, seen, V, ban, ctl.ngram, cx, tid);
    const float* __restrict__ x = sr.x;
    const float T = sc.temperature, pen = ctl.penalty;

    // the maximum (it is always kept)
    unsigned mk = 0u;
    for (int i0 = tid; i0 < V; i0 += 256 * SAMPLE_LOADS) {
        float xv[SAMPLE_LOADS];
#pragma unroll
        for (int u = 0; u < SAMPLE_LOADS; ++u) xv[u] = i0 + u * 256 < V ? x[i0 + u * 256] : 0.f;
#pragma unroll
        for (int u = 0; u < SAMPLE_LOADS; ++u)
            if (i0 + u * 256 < V) mk = max(mk, sample_zkey<PEN>(xv[u], i0 + u * 256, ban_bm, seen, pen, T, mask));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mk = max(mk, (unsigned)__shfl_xor((int)mk, o));
    if (lane == 0) sh.mkey[wave] = mk;
    if (tid == 0) { sh.token = 0; sh.kept = 0; }
    __syncthreads();
    const unsigned mkey = max(max(sh.mkey[0], sh.mkey[1]), max(sh.mkey[2], sh.mkey[3]));
    const float m = sample_unkey(mkey);

    unsigned keep_min = 0u;
    if (sc.top_k > 0 && sc.top_k < V)                    // (uniform: kernel arguments)
        keep_min = ~sample_radix_select<PEN, true>(x, V, ban_bm, seen, pen, T, mask, tid, (sample_u64)(sc.top_k - 1), 0.0, 0u, mkey, m, sh);
    if (sc.top_p < 1.f)
        keep_min = max(keep_min, sample_radix_select<PEN, false>(x, V, ban_bm, seen, pen, T, mask, tid, 0ull, 1.0 - (double)sc.top_p,
                                                                 keep_min, mkey, m, sh));

    // the draw: per-thread sums over contiguous ids, an integer scan, and the owner of r walks its segment
    const int S = (V + 255) >> 8, lo = min(tid * S, V), hi = min(lo + S, V);
    sample_u64 sum = 0ull;
    int cnt = 0;
    for (int i0 = lo; i0 < hi; i0 += SAMPLE_LOADS) {
        float xv[SAMPLE_LOADS];
#pragma unroll
        for (int u = 0; u < SAMPLE_LOADS; ++u) xv[u] = i0 + u < hi ? x[i0 + u] : 0.f;
#pragma unroll
        for (int u = 0; u < SAMPLE_LOADS; ++u) {
            if (i0 + u >= hi) continue;
            const unsigned key = sample_zkey<PEN>(xv[u], i0 + u, ban_bm, seen, pen, T, mask);
            const sample_u64 w = key >= keep_min ? sample_weight(key, mkey, m) : 0ull;
            sum += w; cnt += w != 0ull;
        }
    }
    sample_u64 total;
    const sample_u64 incl = sample_block_scan(sum, tid, sh.ws, &total);
    const sample_u64 U = sample_uniform(sc.seed, keys ? keys[row] : (sample_u64)row, (unsigned)draw);
    const sample_u64 r = __umul64hi(U, total);
    if (out_kept && cnt) atomicAdd(&sh.kept, cnt);
    if (incl > r && incl - sum <= r) {                   // one thread at most; none when total = 0
        sample_u64 acc = incl - sum;
        int tok = hi - 1;
        for (int i = lo; i < hi; ++i) {
            const unsigned key = sample_zkey<PEN>(x[i], i, ban_bm, seen, pen, T, mask);
            acc += key >= keep_min ? sample_weight(key, mkey, m) : 0ull;
            if (acc > r) { tok = i; break; }
        }
        sh.token = tok;
    }
    __syncthreads();
    if (tid == 0) {
        greedy_row_emit(a, row, sh.token);
        if (out_kept) out_kept[row] = sh.kept;
    }
}

// Scoring form: the same selection, plus log max softmax of the row as the selection sees it (EOS masked while mask_eos) -
// the per-step term of the reference's compute_perplexity (captioning_predictor.py:34-47) - for every row open at this step:
//   lp = z_max - logsumexp(z) = -log(1 + sum_{i != argmax} exp(z_i - z_max))
// written to logprobs[row][lp_col]; scored[row] counts the steps written.  Rows already finished keep the caller's zeros.
// Two reads of the row: the first is the selection above, the second (from L2: a row is at most 200 KB) sums exp(z_i - z_max)
// over every index but the selected one, so a peaked row keeps its tail (1 + 1e-9 would round to 1) and log1pf takes it.
// The sum is never serial across the row: thread tid owns the float4 chunks tid, tid + 256, ... (four partial sums, one per
// component) and the tail elements tid, tid + 256, ...; the 256 thread sums meet in a fixed LDS tree.  Assignment and tree depend
// on V alone, so a row's value does not depend on its position, the grid or the RowMap.  Accurate expf / log1pf.
//
// VOCAB (greedy_select_vocab_kernel): a third read of the row (L2 again) turns it into the step's softmax with the z_max / total /
// EOS mask just computed and keeps each vocabulary entry's maximum over the caption's steps - what the reference's probability
// fusion takes from per-step logits (test_pseudo_caption_generation.py:28-63) - in vocab_acc[row][0..V):
//   acc_i = max(acc_i, exp(z_i - z_max) / (1 + total))          (the selected token's own value is 1 / (1 + total))
// A masked EOS and a -inf entry give 0.  Elementwise (accurate expf, a true division), float4 loads / stores on the chunks of the
// sums and the same scalar tail: a value depends on the row's logits and V alone.  Columns V.. of vocab_acc are never touched.
template <bool VOCAB>
__device__ __forceinline__ void greedy_select_scored_body(const SelectRows& a, float* __restrict__ logprobs, int lp_ld, int lp_col,
                                                          int* __restrict__ scored, float* __restrict__ vocab_acc, int acc_ld) {
    const int tid = threadIdx.x, V = a.V, eos = a.eos;
    SelectRow r;
    if (!select_row_begin(a, r)) return;
    const int row = r.row;
    const bool mask_eos = r.mask_eos;
    const float* x = r.x;
    __shared__ float sv[256];
    __shared__ int si[256];
    const int imax = greedy_row_argmax(x, V, eos, mask_eos, tid, sv, si, nullptr, nullptr, 1.f, r.vec);
    const float zmax = sv[0];
    const bool open = a.finished[row] == 0;              // uniform over the block; thread 0 writes it only after the barrier below
    __syncthreads();                                     // sv[] is reused for the sums
    float total = 0.f;
    if (open) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        const int V4 = V >> 2;
        for (int c0 = tid; c0 < V4; c0 += 1024) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 256;
                v[u] = c < V4 ? *(const float4*)(x + 4 * c) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = 4 * (c0 + u * 256);
                // the selected index is left out, and so is a masked EOS (exp(-inf) = 0); component-wise as above
                const int skip = mask_eos ? eos : -1;
                acc.x += (i == imax || i == skip) ? 0.f : expf(v[u].x - zmax);
                acc.y += (i + 1 == imax || i + 1 == skip) ? 0.f : expf(v[u].y - zmax);
                acc.z += (i + 2 == imax || i + 2 == skip) ? 0.f : expf(v[u].z - zmax);
                acc.w += (i + 3 == imax || i + 3 == skip) ? 0.f : expf(v[u].w - zmax);
            }
        }
        float tail = 0.f;
        for (int i = (V4 << 2) + tid; i < V; i += 256)
            tail += (i == imax || (mask_eos && i == eos)) ? 0.f : expf(x[i] - zmax);
        sv[tid] = ((acc.x + acc.y) + (acc.z + acc.w)) + tail;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) sv[tid] += sv[tid + o];
            __syncthreads();
        }
        total = sv[0];
        if (VOCAB) {
            float* __restrict__ a = vocab_acc + (size_t)row * acc_ld;
            const float denom = 1.f + total;
            const int skip = mask_eos ? eos : -1;
            for (int c0 = tid; c0 < V4; c0 += 1024) {
                float4 v[4], p[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + u * 256;
                    if (c < V4) { v[u] = *(const float4*)(x + 4 * c); p[u] = *(const float4*)(a + 4 * c); }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + u * 256, i = 4 * c;
                    if (c < V4) {
                        p[u].x = fmaxf(p[u].x, i == skip ? 0.f : expf(v[u].x - zmax) / denom);
                        p[u].y = fmaxf(p[u].y, i + 1 == skip ? 0.f : expf(v[u].y - zmax) / denom);
                        p[u].z = fmaxf(p[u].z, i + 2 == skip ? 0.f : expf(v[u].z - zmax) / denom);
                        p[u].w = fmaxf(p[u].w, i + 3 == skip ? 0.f : expf(v[u].w - zmax) / denom);
                        *(float4*)(a + 4 * c) = p[u];
                    }
                }
            }
            for (int i = (V4 << 2) + tid; i < V; i += 256)
                a[i] = fmaxf(a[i], i == skip ? 0.f : expf(x[i] - zmax) / denom);
        }
    }
    if (tid == 0) {
        if (greedy_row_emit(a, row, imax)) {
            logprobs[(size_t)row * lp_ld + lp_col] = -log1pf(total);
            scored[row] += 1;
        }
    }
}

__global__ __launch_bounds__(256) void greedy_select_logprob_kernel(SelectRows a, float* __restrict__ logprobs, int lp_ld, int lp_col,
                                                                    int* __restrict__ scored) {
    greedy_select_scored_body<false>(a, logprobs, lp_ld, lp_col, scored, nullptr, 0);
}

__global__ __launch_bounds__(256) void greedy_select_vocab_kernel(SelectRows a, float* __restrict__ logprobs, int lp_ld, int lp_col,
                                                                  int* __restrict__ scored, float* __restrict__ vocab_acc, int acc_ld) {
    greedy_select_scored_body<true>(a, logprobs, lp_ld, lp_col, scored, vocab_acc, acc_ld);
}

// ------------------------------------------------------------------------------------------------
// Teacher-forced scoring (cap_score_captions): the head consumer that reduces a logits row to the log-softmax at a GIVEN id, beside
// the two things the scoring form above takes from it.  Logits row r0 + b (block b) is position j = r % npos of caption c = r / npos:
//   live      = j < n_live[c]
//   target    = targets[c * tgt_ld + j]                              (clamped to [0, V))
//   out_tlp   [c * out_ld + j] = z_target - logsumexp(z) = (z_target - z_max) - log1p(sum_{i != argmax} exp(z_i - z_max))
//   out_top   [c * out_ld + j] = -log1p(the same sum)                (log max softmax: the scoring form's bits, no EOS mask)
//   out_top_id[c * out_ld + j] = argmax                              (greedy_row_argmax: lowest index wins ties, NaN never wins)
// A dead row writes zeros and reads nothing.  The row is read the way the scoring form reads it - the selection, then the sums from
// L2, both with 16-byte loads, thread assignment and LDS tree a function of V alone - so a row's values do not depend on where it
// sits; when the target is the argmax, out_tlp == out_top bit for bit (z_target - z_max is an exact 0).
__global__ __launch_bounds__(256) void target_logprob_kernel(const float* __restrict__ logits, int ld, int V, int r0, int npos,
                                                             const int* __restrict__ targets, int tgt_ld,
                                                             const int* __restrict__ n_live, float* __restrict__ out_tlp,
                                                             float* __restrict__ out_top, int* __restrict__ out_top_id, int out_ld,
                                                             int j0, int share) {
    // j0: the pass's first position is the caption's j0-th (live = j0 + j < n_live; targets / outputs are passed moved by j0);
    // share: that many consecutive rows read ONE logits row (BLIP-2: an image's prompt logits score the first token of all its captions)
    const int tid = threadIdx.x, r = r0 + blockIdx.x, c = r / npos, j = r - c * npos;
    const size_t o = (size_t)c * out_ld + j;
    if (j0 + j >= n_live[c]) {                                // uniform over the block: before any barrier
        if (tid == 0) { out_tlp[o] = 0.f; out_top[o] = 0.f; out_top_id[o] = 0; }
        return;
    }
    const float* x = logits + (size_t)(blockIdx.x / share) * ld;
    __shared__ float sv[256];
    __shared__ int si[256];
    const int imax = greedy_row_argmax(x, V, -1, false, tid, sv, si);
    const float zmax = sv[0];
    __syncthreads();                                     // sv[] is reused for the sums
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int V4 = V >> 2;
    for (int c0 = tid; c0 < V4; c0 += 1024) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cc = c0 + u * 256;
            v[u] = cc < V4 ? *(const float4*)(x + 4 * cc) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = 4 * (c0 + u * 256);
            acc.x += i == imax ? 0.f : expf(v[u].x - zmax);
            acc.y += i + 1 == imax ? 0.f : expf(v[u].y - zmax);
            acc.z += i + 2 == imax ? 0.f : expf(v[u].z - zmax);
            acc.w += i + 3 == imax ? 0.f : expf(v[u].w - zmax);
        }
    }
    float tail = 0.f;
    for (int i = (V4 << 2) + tid; i < V; i += 256) tail += i == imax ? 0.f : expf(x[i] - zmax);
    sv[tid] = ((acc.x + acc.y) + (acc.z + acc.w)) + tail;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sv[tid] += sv[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const int tgt = min(max(targets[(size_t)c * tgt_ld + j], 0), V - 1);
        const float top = -log1pf(sv[0]);
        out_tlp[o] = (x[tgt] - zmax) + top;
        out_top[o] = top;
        out_top_id[o] = imax;
    }
}

// ------------------------------------------------------------------------------------------------
// Probability fusion behind the vocab form: per group of caption rows (CSR: group_rows[group_off[g] .. group_off[g + 1])), the mean
// of the rows' vocab_acc vectors, the tokens whose mean exceeds th in ascending id order, their means, and their full count.
//   mean(i) = (((a_0 + a_1) + a_2) + ...) / (float)n   in fp32, members in listed order; kept if mean > th (strict)
// One workgroup per group walks the vocabulary in tiles of 1 024 tokens (four rounds of 256 consecutive ids; all loads of a tile are
// issued before its first ballot).  The order inside a round comes from the wave64 ballot, across the four waves and the four
// rounds from one LDS table, across tiles from the running base every thread keeps: no scratch, no atomics, and nothing depends on
// the grid (a group's output is the same bits wherever it stands in the list).  At most K entries are written; out_count is the
// full count.  An empty group writes count 0.
__global__ __launch_bounds__(256) void vocab_group_threshold_kernel(const float* __restrict__ acc, int acc_ld, int V,
                                                                    const int* __restrict__ group_rows,
                                                                    const int* __restrict__ group_off, float th, int K,
                                                                    int* __restrict__ out_ids, float* __restrict__ out_prob,
                                                                    int* __restrict__ out_count) {
    __shared__ int wsum[16];                             // [round][wave]
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = group_off[g], n = group_off[g + 1] - r0;
    int base = 0;
    if (n > 0) {                                         // uniform over the block
        const float fn = (float)n;
        for (int i0 = 0; i0 < V; i0 += 1024) {
            float mean[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * 256 + tid;
                float s = 0.f;
                if (i < V) {
                    s = acc[(size_t)group_rows[r0] * acc_ld + i];
                    for (int j = 1; j < n; ++j) s += acc[(size_t)group_rows[r0 + j] * acc_ld + i];
                    s = s / fn;
                }
                mean[u] = s;
            }
            unsigned long long b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                b[u] = __ballot(i0 + u * 256 + tid < V && mean[u] > th);
                if (lane == 0) wsum[u * 4 + w] = __popcll(b[u]);
            }
            __syncthreads();
            int off = base;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                for (int k = 0; k < 4; ++k) {
                    const int c = wsum[u * 4 + k];
                    if (k == w && ((b[u] >> lane) & 1ull)) {
                        const int pos = off + __popcll(b[u] & ((1ull << lane) - 1ull));
                        if (pos < K) {
                            out_ids[(size_t)g * K + pos] = i0 + u * 256 + tid;
                            out_prob[(size_t)g * K + pos] = mean[u];
                        }
                    }
                    off += c;
                }
            }
            base = off;                                  // the same number in every thread
            __syncthreads();                             // wsum is rewritten by the next tile
        }
    }
    if (tid == 0) out_count[g] = base;
}

__global__ void fill_i32_kernel(int* p, int v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void fill_f32_kernel(float* p, float v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void copy_f32_kernel(const float* s, float* d, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

#define CAP_DISPATCH_T(dtype, MACRO)                                                                                  \
    do { if ((dtype) == CAP_DT_BF16) MACRO(bf16_t); else if ((dtype) == CAP_DT_G8) MACRO(g8_t); else MACRO(float); } while (0)

inline int grid_for(size_t n, int per_block) {
    size_t g = (n + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

int launch_convert(int dtype, const float* src, void* dst, size_t n, hipStream_t s) {
    if (dtype == CAP_DT_G8 && n % 8 != 0) { cap_set_error("convert: a G8 buffer holds whole groups of 8 elements (n=%zu)", n); return -1; }
#define CAP_CV(TT) hipLaunchKernelGGL(convert_kernel<TT>, dim3(grid_for(n, 1024)), dim3(256), 0, s, src, (TT*)dst, n)
    CAP_DISPATCH_T(dtype, CAP_CV);
#undef CAP_CV
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_convert2d(int dtype, const float* src, void* dst, int rows, int cols, int dst_ld, hipStream_t s, float scale) {
    const size_t n = (size_t)rows * cols;
    if (dtype == CAP_DT_G8 && dst_ld % 8 != 0) { cap_set_error("convert2d: G8 rows need ld %% 8 == 0 (ld=%d)", dst_ld); return -1; }
#define CAP_CV(TT) hipLaunchKernelGGL(convert2d_kernel<TT>, dim3(grid_for(n, 256)), dim3(256), 0, s, src, (TT*)dst, rows, cols, dst_ld, scale)
    CAP_DISPATCH_T(dtype, CAP_CV);
#undef CAP_CV
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_convert2d_t(int dtype, const float* src, void* dst, int rows, int cols, hipStream_t s, float scale) {
    const size_t n = (size_t)rows * cols;
    if (dtype == CAP_DT_G8 && rows % 8 != 0) { cap_set_error("convert2d_t: G8 rows need ld %% 8 == 0 (ld=%d)", rows); return -1; }
#define CAP_CV(TT) hipLaunchKernelGGL(convert2d_t_kernel<TT>, dim3(grid_for(n, 256)), dim3(256), 0, s, src, (TT*)dst, rows, cols, scale)
    CAP_DISPATCH_T(dtype, CAP_CV);
#undef CAP_CV
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

// The same gather with one thread per 8 consecutive pixels of an image row (patch sizes that are multiples of 8: 16 for ViT-B/16):
// 8 consecutive k of one patch row = one 32-byte G8 group (16 bytes of bf16), written as whole pieces instead of one 2-byte store
// per half per element (155 us per 256 frames at 224 x 224 before; the values are those of patchify_kernel: same expression).
template <typename T>
__global__ void patchify8_kernel(const void* __restrict__ pixels, int fmt, int B, int img, int ps, int Kpad,
                                 T* __restrict__ out, float m0, float m1, float m2, float s0, float s1, float s2) {
    const int G = img / ps, W8 = img / 8;
    const size_t total = (size_t)B * 3 * img * W8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W8) * 8;
        size_t r = i / W8;
        const int y = (int)(r % img); r /= img;
        const int c = (int)(r % 3);
        const int b = (int)(r / 3);
        float v[8];
        if (fmt == 0) {
            const float4* src = (const float4*)((const float*)pixels + (((size_t)b * 3 + c) * img + y) * img + x);
            const float4 a = src[0], d = src[1];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = d.x; v[5] = d.y; v[6] = d.z; v[7] = d.w;
        } else {
            const unsigned char* src = (const unsigned char*)pixels + (((size_t)b * img + y) * img + x) * 3 + c;
            const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ((float)src[3 * j] * (1.0f / 255.0f) - mean) / sd;
        }
        const int py = y / ps, dy = y - py * ps, px = x / ps, dx = x - px * ps;
        T* row = out + ((size_t)b * G * G + (size_t)py * G + px) * Kpad;
        const int k = c * ps * ps + dy * ps + dx;                    // a multiple of 8
        store4(row, k, make_float4(v[0], v[1], v[2], v[3]));
        store4(row, k + 4, make_float4(v[4], v[5], v[6], v[7]));
    }
}

int launch_patchify(int dtype, const void* pixels, int fmt, int B, int img, int ps, int Kpad, void* out,
                    const float* mean, const float* stdv, hipStream_t s) {
    if (img % ps != 0 || 3 * ps * ps > Kpad) {
        cap_set_error("patchify: image %d not divisible by patch %d or Kpad %d too small", img, ps, Kpad);
        return -1;
    }
    if (dtype == CAP_DT_G8 && Kpad % 8 != 0) { cap_set_error("patchify: G8 rows need Kpad %% 8 == 0 (Kpad=%d)", Kpad); return -1; }
    const size_t n = (size_t)B * 3 * img * img;
    const float m0 = mean ? mean[0] : 0.f, m1 = mean ? mean[1] : 0.f, m2 = mean ? mean[2] : 0.f;
    const float s0 = stdv ? stdv[0] : 1.f, s1 = stdv ? stdv[1] : 1.f, s2 = stdv ? stdv[2] : 1.f;
    if (ps % 8 == 0 && ((uintptr_t)pixels & 15) == 0) {
#define CAP_PF8(TT) hipLaunchKernelGGL(patchify8_kernel<TT>, dim3(grid_for(n / 8, 256)), dim3(256), 0, s, pixels, fmt, B, img, ps, Kpad, (TT*)out, m0, m1, m2, s0, s1, s2)
        CAP_DISPATCH_T(dtype, CAP_PF8);
#undef CAP_PF8
        CAP_HIP_CHECK(hipGetLastError());
        return 0;
    }
#define CAP_PF(TT) hipLaunchKernelGGL(patchify_kernel<TT>, dim3(grid_for(n, 256)), dim3(256), 0, s, pixels, fmt, B, img, ps, Kpad, (TT*)out, m0, m1, m2, s0, s1, s2)
    CAP_DISPATCH_T(dtype, CAP_PF);
#undef CAP_PF
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_cls_rows(const float* cls, const float* pos, float* X, int B, int tokens, int D, hipStream_t s) {
    hipLaunchKernelGGL(cls_rows_kernel, dim3((B * D + 255) / 256), dim3(256), 0, s, cls, pos, X, B, tokens, D);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_layernorm(int dtype, const float* in, int ld_in, const float* gamma, const float* beta, float eps,
                     void* out_t, float* out_f, int M, int D, hipStream_t s, const int* n_rows) {
    if (D % 4 != 0 || D > 256 * LN_MAXV || (ld_in % 4) != 0 || (dtype == CAP_DT_G8 && D % 8 != 0)) {
        cap_set_error("layernorm: unsupported width %d (ld %d)", D, ld_in);
        return -1;
    }
#define CAP_LN(TT, MV)                                                                                                  \
    hipLaunchKernelGGL((layernorm_kernel<TT, MV>), dim3((M + 3) / 4), dim3(256), 0, s, in, ld_in, gamma, beta, eps,    \
                       (TT*)out_t, out_f, M, D, n_rows)
#define CAP_LN_T(TT) do { if (D <= 1024) CAP_LN(TT, 4); else if (D <= 2048) CAP_LN(TT, 8); else CAP_LN(TT, LN_MAXV); } while (0)
    CAP_DISPATCH_T(dtype, CAP_LN_T);
#undef CAP_LN_T
#undef CAP_LN
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_reduce_layernorm(int dtype, const float* part, int S, const float* bias, const float* resid,
                            const float* gamma, const float* beta, float eps, void* out_t, float* out_f, float* y_out,
                            int M, int D, hipStream_t s, bool per_row_block, const int* n_rows) {
    if (n_rows && per_row_block && D > 1024) { cap_set_error("reduce_layernorm: the wide block kernel takes no row count from the device"); return -1; }
    if (D % 4 != 0 || D > 256 * LN_MAXV || S < 1 || (dtype == CAP_DT_G8 && D % 8 != 0)) { cap_set_error("reduce_layernorm: unsupported width %d / slices %d", D, S); return -1; }
    // per_row_block: the decoder's choice up to a few hundred rows (latency-bound).  For rows up to 1024 wide the block-per-row
    // kernel forms the wave-per-row kernel's sums in its order (slices, bias, residual; statistics: thread j + 64 i = lane j,
    // vector i) and the two agree bit for bit (tests/test_kernels_gpu.py::test_reduce_layernorm_kernels_agree_bit_for_bit), so a
    // caller may pick by row count there; the WIDE block kernel (rows beyond 1024) has its own order: by path only.
    if (per_row_block && D <= 1024) {
#define CAP_RR(TT) hipLaunchKernelGGL(reduce_layernorm_row_kernel<TT>, dim3(M), dim3(256), 0, s, part, S, bias, resid, gamma, beta, eps, (TT*)out_t, out_f, y_out, M, D, n_rows)
        CAP_DISPATCH_T(dtype, CAP_RR);
#undef CAP_RR
        CAP_HIP_CHECK(hipGetLastError());
        return 0;
    }
    if (per_row_block && D <= 3072) {     // wide rows, decode-sized row count (the caller's choice, as above)
#define CAP_RW(TT) hipLaunchKernelGGL(reduce_layernorm_wide_kernel<TT>, dim3(M), dim3(256), 0, s, part, S, bias, resid, gamma, beta, eps, (TT*)out_t, out_f, y_out, M, D)
        CAP_DISPATCH_T(dtype, CAP_RW);
#undef CAP_RW
        CAP_HIP_CHECK(hipGetLastError());
        return 0;
    }
    const int wpb = M >= 2048 ? 4 : 1;
    const dim3 grid((M + wpb - 1) / wpb), block(64 * wpb);
#define CAP_RLN(TT, MV)                                                                                                 \
    hipLaunchKernelGGL((reduce_layernorm_kernel<TT, MV>), grid, block, 0, s, part, S, bias, resid, gamma, beta, eps,     \
                       (TT*)out_t, out_f, y_out, M, D, n_rows)
#define CAP_RLN_T(TT) do { if (D <= 1024) CAP_RLN(TT, 4); else if (D <= 2048) CAP_RLN(TT, 8); else CAP_RLN(TT, LN_MAXV); } while (0)
    CAP_DISPATCH_T(dtype, CAP_RLN_T);
#undef CAP_RLN_T
#undef CAP_RLN
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

// Split-K consumer without LayerNorm: out[r][c] = act(sum_z part[z][r][c] + bias[c]) in the compute type (OPT decode: the
// fused q|k|v projection and fc1 + ReLU).  act: 0 none, 2 ReLU.
template <typename T>
__global__ __launch_bounds__(256) void reduce_bias_act_kernel(const float* __restrict__ part, int S, const float* __restrict__ bias,
                                                              T* __restrict__ out, int M, int N, int act) {
    const size_t n4 = (size_t)M * N / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i * 4;
        const int c = e % N;
        float4 a = *(const float4*)(part + e);
        for (int z = 1; z < S; ++z) {
            const float4 b = *(const float4*)(part + (size_t)z * M * N + e);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        if (bias) { const float4 b = *(const float4*)(bias + c); a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
        if (act == 2) { a.x = fmaxf(a.x, 0.f); a.y = fmaxf(a.y, 0.f); a.z = fmaxf(a.z, 0.f); a.w = fmaxf(a.w, 0.f); }
        store4(out + (e - c), c, a);
    }
}

int launch_reduce_bias_act(int dtype, const float* part, int S, const float* bias, void* out, int M, int N, int act, hipStream_t s) {
    if (N % 4 != 0) { cap_set_error("reduce_bias_act: N must be a multiple of 4"); return -1; }
    if (dtype == CAP_DT_G8 && N % 8 != 0) { cap_set_error("reduce_bias_act: G8 rows need N %% 8 == 0 (N=%d)", N); return -1; }
    const int grid = (int)std::min<size_t>(((size_t)M * N / 4 + 255) / 256, 2048);
#define CAP_RB(TT) hipLaunchKernelGGL(reduce_bias_act_kernel<TT>, dim3(grid), dim3(256), 0, s, part, S, bias, (TT*)out, M, N, act)
    CAP_DISPATCH_T(dtype, CAP_RB);
#undef CAP_RB
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_embed_tokens(int dtype, const int* ids, int L, const float* word, const float* pos, const float* type0,
                        const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int R, int D,
                        hipStream_t s, int V) {
    if (D % 4 != 0 || D > 256 * LN_MAXV || V < 1) { cap_set_error("embed_tokens: unsupported width %d / vocabulary %d", D, V); return -1; }
    if (dtype == CAP_DT_G8 && D % 8 != 0) { cap_set_error("embed_tokens: G8 rows need D %% 8 == 0 (D=%d)", D); return -1; }
#define CAP_ET(TT) hipLaunchKernelGGL(embed_tokens_kernel<TT>, dim3((R + 3) / 4), dim3(256), 0, s, ids, L, word, pos, type0, gamma, beta, eps, (TT*)out_t, out_f, R, D, V)
    CAP_DISPATCH_T(dtype, CAP_ET);
#undef CAP_ET
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_mean_pool_normalize(const float* x, const int* lens, int B, int L, int D, float* out, hipStream_t s) {
    if (D % 4 != 0 || D > 1024) { cap_set_error("mean_pool: unsupported width %d", D); return -1; }
    hipLaunchKernelGGL(mean_pool_normalize_kernel, dim3(B), dim3(256), 0, s, x, lens, L, D, out);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_embed(int dtype, const int* seq, int seq_ld, int t, const float* word, const float* pos,
                 const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int R, int D,
                 hipStream_t s, float* y_out, RowMap map) {
    if (D % 4 != 0 || D > 256 * LN_MAXV) { cap_set_error("embed: unsupported width %d", D); return -1; }
    if (dtype == CAP_DT_G8 && D % 8 != 0) { cap_set_error("embed: G8 rows need D %% 8 == 0 (D=%d)", D); return -1; }
#define CAP_EM(TT) hipLaunchKernelGGL(embed_kernel<TT>, dim3((R + 3) / 4), dim3(256), 0, s, seq, seq_ld, t, word, pos, gamma, beta, eps, (TT*)out_t, out_f, y_out, R, D, map)
    CAP_DISPATCH_T(dtype, CAP_EM);
#undef CAP_EM
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_embed_prompt(int dtype, const int* seq, int seq_ld, int npos, int row0, const float* word, const float* pos,
                        const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int n_caps, int D,
                        hipStream_t s, float* y_out) {
    if (D % 4 != 0 || D > 256 * LN_MAXV) { cap_set_error("embed_prompt: unsupported width %d", D); return -1; }
    if (dtype == CAP_DT_G8 && D % 8 != 0) { cap_set_error("embed_prompt: G8 rows need D %% 8 == 0 (D=%d)", D); return -1; }
    if (npos < 1 || npos > seq_ld || n_caps < 1 || row0 < 0) {
        cap_set_error("embed_prompt: %d positions of %d captions from row %d do not fit rows of %d tokens", npos, n_caps, row0, seq_ld);
        return -1;
    }
    const int R = n_caps * npos;
#define CAP_EMP(TT) hipLaunchKernelGGL(embed_prompt_kernel<TT>, dim3((R + 3) / 4), dim3(256), 0, s, seq, seq_ld, npos, row0, word, pos, gamma, beta, eps, (TT*)out_t, out_f, y_out, R, D)
    CAP_DISPATCH_T(dtype, CAP_EMP);
#undef CAP_EMP
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_init_prompt_seq(int* seq, int* finished, int* out_len, int R, int L, const int* prompt, int prompt_rows, int P, int V,
                           int pad, hipStream_t s) {
    if (!prompt || P < 1 || P > L || (prompt_rows != 1 && prompt_rows != R) || V < 1) {
        cap_set_error("init_prompt_seq: a prompt of %d rows x %d tokens does not fit %d rows of %d tokens (vocabulary %d)", prompt_rows, P, R, L, V);
        return -1;
    }
    hipLaunchKernelGGL(init_prompt_seq_kernel, dim3(64), dim3(256), 0, s, seq, finished, out_len, R, L, prompt, prompt_rows, P, V, pad);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_select_step(const SelectStep& st, hipStream_t s) {
    const BanSet& ban = st.ban;
    const RepeatCtl& ctl = st.ctl;
    const bool processed = ctl.active() || ban.bits;
    if (ban.n_multi < 0 || ban.n_multi > BAN_MAX_MULTI || (ban.n_multi && (!ban.multi || !ban.bits)) || st.hist0 < 0 || st.hist0 > st.t + 1) {
        cap_set_error("select_step: n_multi = %d must be in [0, %d] (with ban_multi and ban_bits), hist0 = %d in [0, t + 1 = %d]", ban.n_multi,
                      BAN_MAX_MULTI, st.hist0, st.t + 1);
        return -1;
    }
    if (!(ctl.penalty > 0.f) || !std::isfinite(ctl.penalty) || ctl.ngram < 0 || ctl.vn < 0) {
        cap_set_error("select_step: penalty %g (finite, > 0), n-gram size %d (>= 0), %d virtual context tokens (>= 0)", (double)ctl.penalty,
                      ctl.ngram, ctl.vn);
        return -1;
    }
    if (st.sample) {
        const SampleCtl& sc = st.sc;
        if (!(sc.temperature > 0.f) || !std::isfinite(sc.temperature)) {
            cap_set_error("select_step: temperature = %g (a finite number above 0)", (double)sc.temperature);
            return -1;
        }
        if (sc.top_k < 0) { cap_set_error("select_step: top_k = %d (0 = off, or >= 1)", sc.top_k); return -1; }
        if (!(sc.top_p > 0.f) || !(sc.top_p <= 1.f)) { cap_set_error("select_step: top_p = %g (in (0, 1]; 1 = off)", (double)sc.top_p); return -1; }
        if (st.draw < 0) { cap_set_error("select_step: draw = %d (>= 0)", st.draw); return -1; }
    }
    if (st.logprobs || st.vocab_acc) {
        if (st.sample || processed) {
            cap_set_error("select_step: the log-prob and vocabulary outputs go with the plain arg-max (no ban, repetition controls or sampling)");
            return -1;
        }
        if (st.ld % 4 != 0) { cap_set_error("select_step: the log-prob and vocabulary forms need ld %% 4 == 0 (got %d)", st.ld); return -1; }
        if (!st.logprobs || !st.scored || st.lp_col < 0 || st.lp_col >= st.lp_ld) {
            cap_set_error("select_step: log-prob column %d outside [0, %d), or no log-prob buffer or step counter", st.lp_col, st.lp_ld);
            return -1;
        }
        if (st.vocab_acc && (st.acc_ld < st.V || st.acc_ld % 4 != 0 || ((uintptr_t)st.vocab_acc & 15) != 0)) {
            cap_set_error("select_step: vocab_acc needs acc_ld >= V (%d), acc_ld %% 4 == 0 (got %d) and a 16-byte aligned pointer", st.V, st.acc_ld);
            return -1;
        }
    }
    const SelectRows& rows = st;
    const dim3 grid(st.R), block(256);
    const bool pen = ctl.penalty != 1.f;
    const size_t bmb = (size_t)ban_words(st.V) * 4 * (pen ? 2 : 1);      // the ban bitmap, and the penalty's behind it
    if (st.sample) {
        const unsigned long long* keys = (const unsigned long long*)st.keys;
        if (pen) hipLaunchKernelGGL(greedy_select_sampled_kernel<true>, grid, block, bmb, s, rows, ban, st.hist0, ctl, st.sc, keys, st.draw, st.out_kept);
        else hipLaunchKernelGGL(greedy_select_sampled_kernel<false>, grid, block, bmb, s, rows, ban, st.hist0, ctl, st.sc, keys, st.draw, st.out_kept);
    } else if (processed) {
        if (pen) hipLaunchKernelGGL(greedy_select_processed_kernel<true>, grid, block, bmb, s, rows, ban, st.hist0, ctl);
        else if (ctl.active()) hipLaunchKernelGGL(greedy_select_processed_kernel<false>, grid, block, bmb, s, rows, ban, st.hist0, ctl);
        else hipLaunchKernelGGL((greedy_select_processed_kernel<false, false>), grid, block, bmb, s, rows, ban, st.hist0, ctl);
    } else if (st.vocab_acc) {
        hipLaunchKernelGGL(greedy_select_vocab_kernel, grid, block, 0, s, rows, st.logprobs, st.lp_ld, st.lp_col, st.scored, st.vocab_acc, st.acc_ld);
    } else if (st.logprobs) {
        hipLaunchKernelGGL(greedy_select_logprob_kernel, grid, block, 0, s, rows, st.logprobs, st.lp_ld, st.lp_col, st.scored);
    } else {
        hipLaunchKernelGGL(greedy_select_kernel, grid, block, 0, s, rows);
    }
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_target_logprob(const float* logits, int ld, int V, int rows, int r0, int npos, const int* targets, int tgt_ld,
                          const int* n_live, float* out_tlp, float* out_top, int* out_top_id, int out_ld, hipStream_t s, int j0, int share) {
    if (!logits || !targets || !n_live || !out_tlp || !out_top || !out_top_id) { cap_set_error("target_logprob: null buffer"); return -1; }
    if (rows < 1 || r0 < 0 || npos < 1 || V < 1 || ld < V || ld % 4 != 0 || ((uintptr_t)logits & 15) != 0 || out_ld < npos || tgt_ld < 1 || j0 < 0 || share < 1) {
        cap_set_error("target_logprob: %d rows from %d at %d positions per caption (outputs [., %d]) of [., %d] logits with ld %d: ld >= V, "
                      "ld %% 4 == 0, a 16-byte aligned pointer and out_ld >= positions are needed", rows, r0, npos, out_ld, V, ld);
        return -1;
    }
    hipLaunchKernelGGL(target_logprob_kernel, dim3(rows), dim3(256), 0, s, logits, ld, V, r0, npos, targets, tgt_ld, n_live, out_tlp,
                       out_top, out_top_id, out_ld, j0, share);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

// The open rows in ascending order (stable: a caption's compact position only ever moves towards the front) and their count.
__global__ __launch_bounds__(1024) void compact_rows_kernel(const int* __restrict__ finished, int R, int* __restrict__ live,
                                                            int* __restrict__ n_live) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int r0 = 0; r0 < R; r0 += 1024) {
        const int r = r0 + tid;
        const bool on = r < R && finished[r] == 0;
        const unsigned long long b = __ballot(on);
        if (lane == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int off = base;
        for (int i = 0; i < w; ++i) off += wsum[i];
        if (on) live[off + __popcll(b & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        if (tid == 0) {
            int sum = 0;
            for (int i = 0; i < 16; ++i) sum += wsum[i];
            base += sum;
        }
        __syncthreads();
    }
    if (tid == 0) *n_live = base;
}
int launch_vocab_group_threshold(const float* acc, int acc_ld, int V, const int* group_rows, const int* group_off, int G, float th,
                                 int K, int* out_ids, float* out_prob, int* out_count, hipStream_t s) {
    if (G < 1) return 0;
    hipLaunchKernelGGL(vocab_group_threshold_kernel, dim3(G), dim3(256), 0, s, acc, acc_ld, V, group_rows, group_off, th, K, out_ids,
                       out_prob, out_count);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_compact_rows(const int* finished, int R, int* live, int* n_live, hipStream_t s) {
    hipLaunchKernelGGL(compact_rows_kernel, dim3(1), dim3(1024), 0, s, finished, R, live, n_live);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void absmax_f32_kernel(const float* __restrict__ src, size_t n, unsigned int* out_bits) {
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float a = fabsf(src[i]);
        m = (a > m || a != a) ? a : m;                   // a NaN sticks (and compares above every bound below)
    }
    const float w = (m != m) ? m : wave_max(m);
    // non-negative floats order like their bit patterns; a NaN's pattern is above +inf's
    if ((threadIdx.x & 63) == 0 || m != m) atomicMax(out_bits, __float_as_uint(w));
}
int launch_absmax_f32(const float* src, size_t n, unsigned int* out_bits, hipStream_t s) {
    hipLaunchKernelGGL(absmax_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, src, n, out_bits);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_fill_i32(int* p, int v, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(fill_i32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, p, v, n);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_fill_f32(float* p, float v, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(fill_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, p, v, n);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_copy_f32(const float* src, float* dst, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(copy_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, src, dst, n);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- image state: records <-> the call-packed buffer (ops.h, ImageStateLayout) ----------------------------------------------
// Two copies.  Payload: one row = cpr 16-byte chunks, a lane per chunk, so a wave moves whole rows that are contiguous on both sides
// except where a record or a KV16 group ends; rows are numbered [image][section][row] (the record's order), a workgroup takes
// IMAGE_STATE_ROWS_PER_LANE sets of 256 / cpr rows and issues all its loads before its stores.  The KV16 scales are a 4-byte stream of
// their own in the workgroups behind the payload's, a lane per scale; the same workgroups write a record's zero padding (pack only).
// unpack writes the rows (and scales) of the B images and nothing else of the buffer.
constexpr int IMAGE_STATE_ROWS_PER_LANE = 4;
struct ImageStateGeom {
    int sections, rows, cpr, kv16, B;
    int scale_dwords;                    // per section: the rows' scales and their padding to 16 bytes (0 without scales)
    int tail_dwords;                     // zeros that close a record
    unsigned payload_blocks;
    size_t rec_bytes, sec_bytes, block_bytes;
};
template <bool PACK>
__device__ __forceinline__ void image_state_move(const ImageStateGeom& g, char* __restrict__ buf, char* __restrict__ state) {
    if (blockIdx.x < g.payload_blocks) {
        const int rpb = 256 / g.cpr, lr = (int)threadIdx.x / g.cpr, ch = (int)threadIdx.x - lr * g.cpr;
        const size_t per_img = (size_t)g.sections * g.rows, total = per_img * g.B, row_bytes = (size_t)g.cpr * 16;
        uint4 v[IMAGE_STATE_ROWS_PER_LANE];
        uint4* dst[IMAGE_STATE_ROWS_PER_LANE];
#pragma unroll
        for (int u = 0; u < IMAGE_STATE_ROWS_PER_LANE; ++u) {
            const size_t row = ((size_t)blockIdx.x * IMAGE_STATE_ROWS_PER_LANE + u) * rpb + lr;
            dst[u] = nullptr;
            if (row >= total) continue;
            const size_t img = row / per_img, rem = row - img * per_img, sec = rem / g.rows, r = rem - sec * g.rows;
            const size_t ri = img * g.rows + r;                  // the row inside the section's block of the buffer
            char* b = buf + sec * g.block_bytes + (g.kv16 ? kv16_row_off(ri) : ri * row_bytes) + ch * 16;
            char* st = state + img * g.rec_bytes + sec * g.sec_bytes + r * row_bytes + ch * 16;
            v[u] = *reinterpret_cast<const uint4*>(PACK ? b : st);
            dst[u] = reinterpret_cast<uint4*>(PACK ? st : b);
        }
#pragma unroll
        for (int u = 0; u < IMAGE_STATE_ROWS_PER_LANE; ++u)
            if (dst[u]) *dst[u] = v[u];
        return;
    }
    const size_t n_scale = (size_t)g.sections * g.scale_dwords, aux = n_scale + (PACK ? g.tail_dwords : 0);
    const size_t t = (size_t)(blockIdx.x - g.payload_blocks) * 256 + threadIdx.x;
    if (t >= aux * g.B) return;
    const size_t img = t / aux, a = t - img * aux;
    char* rec = state + img * g.rec_bytes;
    if (a < n_scale) {
        const size_t sec = a / g.scale_dwords, r = a - sec * g.scale_dwords;
        unsigned int* sp = reinterpret_cast<unsigned int*>(rec + sec * g.sec_bytes + (size_t)g.rows * g.cpr * 16) + r;
        if (r < (size_t)g.rows) {
            unsigned int* bp = reinterpret_cast<unsigned int*>(buf + sec * g.block_bytes + kv16_scale_off(img * g.rows + r));
            if (PACK) *sp = *bp; else *bp = *sp;
        } else if (PACK) {
            *sp = 0u;
        }
    } else if (PACK) {
        reinterpret_cast<unsigned int*>(rec + (size_t)g.sections * g.sec_bytes)[a - n_scale] = 0u;
    }
}
__global__ __launch_bounds__(256) void image_state_pack_kernel(ImageStateGeom g, const char* __restrict__ buf, char* __restrict__ state) {
    image_state_move<true>(g, const_cast<char*>(buf), state);
}
__global__ __launch_bounds__(256) void image_state_unpack_kernel(ImageStateGeom g, char* __restrict__ buf, const char* __restrict__ state) {
    image_state_move<false>(g, buf, const_cast<char*>(state));
}
static int image_state_geom(const ImageStateLayout& L, int B, const void* buf, const void* state, const char* who, ImageStateGeom& g,
                            bool pack, unsigned& blocks) {
    if (!buf || !state) { cap_set_error("%s: null buffer", who); return -1; }
    if ((((uintptr_t)buf | (uintptr_t)state) & 15) != 0) { cap_set_error("%s: the cache and the state must be 16-byte aligned", who); return -1; }
    if (L.sections < 1 || L.rows < 1 || B < 1 || (L.row_bytes != 16 && L.row_bytes != 128 && L.row_bytes != 256) || (L.kv16 && L.row_bytes != 128)) {
        cap_set_error("%s: %d sections of %d rows of %d bytes (KV16 %d) for %d images", who, L.sections, L.rows, L.row_bytes, L.kv16, B);
        return -1;
    }
    g.sections = L.sections; g.rows = L.rows; g.cpr = L.row_bytes / 16; g.kv16 = L.kv16 ? 1 : 0; g.B = B;
    g.scale_dwords = L.kv16 ? (L.rows + 3) / 4 * 4 : 0;
    g.rec_bytes = L.record_bytes(); g.sec_bytes = L.section_bytes(); g.block_bytes = L.block_bytes((size_t)B);
    g.tail_dwords = (int)((g.rec_bytes - (size_t)L.sections * g.sec_bytes) / 4);
    const size_t rows = (size_t)B * L.sections * L.rows, per_block = (size_t)(256 / g.cpr) * IMAGE_STATE_ROWS_PER_LANE;
    const size_t pb = (rows + per_block - 1) / per_block;
    const size_t aux = ((size_t)L.sections * g.scale_dwords + (pack ? g.tail_dwords : 0)) * B, ab = (aux + 255) / 256;
    if (pb + ab > 0x7fffffffu) { cap_set_error("%s: %zu rows of %d images exceed one launch", who, rows, B); return -1; }
    g.payload_blocks = (unsigned)pb;
    blocks = (unsigned)(pb + ab);
    return 0;
}
int launch_image_state_pack(const ImageStateLayout& L, int B, const void* buffer, void* state, hipStream_t s) {
    ImageStateGeom g;
    unsigned blocks;
    if (image_state_geom(L, B, buffer, state, "image_state_pack", g, true, blocks) != 0) return -1;
    hipLaunchKernelGGL(image_state_pack_kernel, dim3(blocks), dim3(256), 0, s, g, (const char*)buffer, (char*)state);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_image_state_unpack(const ImageStateLayout& L, int B, void* buffer, const void* state, hipStream_t s) {
    ImageStateGeom g;
    unsigned blocks;
    if (image_state_geom(L, B, buffer, state, "image_state_unpack", g, false, blocks) != 0) return -1;
    hipLaunchKernelGGL(image_state_unpack_kernel, dim3(blocks), dim3(256), 0, s, g, (char*)buffer, (const char*)state);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

CAP_DEFINE_G8_CLAMP_READER(cap_g8_clamped_elementwise)
