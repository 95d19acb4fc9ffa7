// The kernels of the BLIP-2 image-text scorer (CAP_ARCH_BLIP2_ITM) that the other architectures do not have: the Q-Former's text
// embeddings, its self-attention over [query rows | text rows] with a text length per pair, and the ITC / ITM heads.  Replaces, per
// (crop, caption) pair, HF `Blip2ForImageTextRetrieval.forward` as the reference's `--method blip2_itm | blip2_itc` calls the LAVIS
// model it was ported from (experimenting_env/captioner/pseudocaptioner.py:34-37, :193-308); GEMMs, LayerNorm, the query rows'
// cross-attention and the ViT-g tower run on the shared kernels (captioner.hip, run_qformer).
//
// Every sum here is formed in an order fixed by the row's own width and the pair's own text length - never by the batch or by the
// padded L - so a pair has the same bits alone, in a batch, at the end of a partial micro-batch and padded to a longer L
// (tests/test_blip2_itm_gpu.py).
#include "common.h"
#include "ln.h"
#include "ops.h"

namespace {

constexpr int ITM_MAX_D = 1024;                 // widest Q-Former row the embedding / head kernels take
constexpr int ITM_HD = 64;                      // head width of the two-segment attention
constexpr int ITM_MAX_SEG = 32;                 // rows per segment (32 queries, 32 text tokens)
constexpr int HEAD_THREADS = 256, ITM_MAX_P = 1024;

// x[r, :] = LayerNorm(word[ids[r]] + pos[r % L]) (Blip2TextEmbeddings, positions counted from 0 over the text, then
// qformer.layernorm) -> x_f fp32 and x_t in the GEMM-operand type.  One wave per row; ids outside [0, V) are clamped (the host
// validates them; the kernel never reads outside the table).  Rows beyond a pair's length are embedded like any other: nothing
// of a valid row depends on them.
template <typename TO>
__global__ __launch_bounds__(256) void itm_embed_text_kernel(const int* __restrict__ ids, int L, const float* __restrict__ word,
                                                             const float* __restrict__ pos, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, float* __restrict__ x_f,
                                                             TO* __restrict__ x_t, int M, int D, int V) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const int id = min(max(ids[r], 0), V - 1), t = r % L;
    const float* we = word + (size_t)id * D;
    const float* pe = pos + (size_t)t * D;
    constexpr int NV = ITM_MAX_D / 256;          // float4 per lane: column lane * 4 + i * 256 (ln.h's row layout)
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < D) {
            const float4 a = *(const float4*)(we + c), b = *(const float4*)(pe + c);
            v[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        } else {
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    ln_row<TO, NV>(v, NV, lane, D, gamma, beta, eps, x_t + (size_t)r * D, x_f + (size_t)r * D);      // the project's one LayerNorm (ln.h)
}

// Q-Former self-attention of pair b, head h over keys in two segments: the nq query rows (qkv_q [B * nq, 3 * H * 64], never masked)
// and the first lens[b] of the L text rows (qkv_t [B * L, 3 * H * 64]); HF's key mask [1 x nq | attention_mask].  One wave per
// (pair, head): lane = query row (query segment first, then ALL L text rows - a row beyond the pair's length is computed like HF
// computes it and read by nobody), its q and output rows in registers; the pair's keys and values staged once into LDS as fp32 and
// read as wave-wide broadcasts.  Online softmax over the keys in the order query 0..nq-1, text 0..lens[b]-1: the order depends on
// nq and the pair's own length only.  nq = 0 (no query segment) is the ITC text pass; L = 0 the ITC image pass.
template <typename T, typename TO>
__global__ __launch_bounds__(64) void itm_self_attention_kernel(const T* __restrict__ qkv_q, const T* __restrict__ qkv_t,
                                                               const int* __restrict__ lens, TO* __restrict__ ctx_q,
                                                               TO* __restrict__ ctx_t, int nq, int L, int H, float scale) {
    __shared__ float Ks[2 * ITM_MAX_SEG * ITM_HD], Vs[2 * ITM_MAX_SEG * ITM_HD];
    const int h = blockIdx.x % H, b = blockIdx.x / H, lane = threadIdx.x;
    const int W = H * ITM_HD, ld = 3 * W;
    const int len = L > 0 ? min(max(lens[b], 1), L) : 0;
    const int nk = nq + len;                                     // keys this pair sees
    // key j < nq: query row j; else text row j - nq
    for (int i = lane; i < nk * (ITM_HD / 4); i += 64) {
        const int j = i / (ITM_HD / 4), d = (i - j * (ITM_HD / 4)) * 4;
        const T* row = j < nq ? qkv_q + ((size_t)b * nq + j) * ld : qkv_t + ((size_t)b * L + (j - nq)) * ld;
        const T* kp = row + W + h * ITM_HD + d;
        const T* vp = row + 2 * W + h * ITM_HD + d;
        *(float4*)(Ks + j * ITM_HD + d) = make_float4(to_f32(kp[0]), to_f32(kp[1]), to_f32(kp[2]), to_f32(kp[3]));
        *(float4*)(Vs + j * ITM_HD + d) = make_float4(to_f32(vp[0]), to_f32(vp[1]), to_f32(vp[2]), to_f32(vp[3]));
    }
    __syncthreads();
    const bool live = lane < nq + L;
    if (!live) return;
    const bool is_q = lane < nq;
    const size_t orow = is_q ? (size_t)b * nq + lane : (size_t)b * L + (lane - nq);
    const T* qp = (is_q ? qkv_q : qkv_t) + orow * ld + h * ITM_HD;
    float qv[ITM_HD], o[ITM_HD];
#pragma unroll
    for (int d = 0; d < ITM_HD; ++d) {
        qv[d] = to_f32(qp[d]) * scale;
        o[d] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < nk; ++j) {
        float sc = 0.f;
#pragma unroll
        for (int d = 0; d < ITM_HD; ++d) sc = fmaf(qv[d], Ks[j * ITM_HD + d], sc);
        const float mn = fmaxf(m, sc);
        const float c = expf(m - mn), pj = expf(sc - mn);
        l = l * c + pj;
#pragma unroll
        for (int d = 0; d < ITM_HD; ++d) o[d] = fmaf(pj, Vs[j * ITM_HD + d], o[d] * c);
        m = mn;
    }
    const float inv = 1.0f / l;
    TO* op = (is_q ? ctx_q : ctx_t) + orow * W;                  // row base: a multiple of 8 elements (W % 64 == 0) for a G8 output
#pragma unroll
    for (int d = 0; d < ITM_HD; d += 4)
        store4(op, h * ITM_HD + d, make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv));
}

// fixed-order sum over the workgroup: per-thread partials -> LDS -> a tree whose shape depends on HEAD_THREADS only
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int w = HEAD_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}

// ITC heads.  One workgroup per output row r: x row r * rows_per (image head: every query row, rows_per = 1; text head: row 0 =
// [CLS] of each caption, rows_per = L) -> W [P, D] fp32 + bias (vision_projection / text_projection) -> L2 normalised -> out [n, P].
__global__ __launch_bounds__(HEAD_THREADS) void itc_head_kernel(const float* __restrict__ x, int rows_per, const float* __restrict__ W,
                                                                const float* __restrict__ bias, float* __restrict__ out, int D, int P) {
    __shared__ float xs[ITM_MAX_D], ys[ITM_MAX_P], red[HEAD_THREADS];
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* xr = x + (size_t)r * rows_per * D;
    for (int d = t; d < D; d += HEAD_THREADS) xs[d] = xr[d];
    __syncthreads();
    for (int p = wave; p < P; p += HEAD_THREADS / 64) {
        const float* wr = W + (size_t)p * D;
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) acc = fmaf(xs[d], wr[d], acc);
        acc = wave_sum(acc);
        if (lane == 0) ys[p] = acc + bias[p];
    }
    __syncthreads();
    float ss = 0.f;
    for (int p = t; p < P; p += HEAD_THREADS) ss = fmaf(ys[p], ys[p], ss);
    const float nrm = fmaxf(sqrtf(block_sum(ss, red)), 1e-12f);          // torch.nn.functional.normalize's eps
    for (int p = t; p < P; p += HEAD_THREADS) out[(size_t)r * P + p] = ys[p] / nrm;
}

// ITC score = max over the nq query rows of <img[i, q, :], txt[j, :]> (no temperature): one wave per score.  paired: out[i] for
// (i, i), n = Ni; else out [Ni, Nt] (HF's logits_per_image).
__global__ __launch_bounds__(256) void itc_scores_kernel(const float* __restrict__ img, const float* __restrict__ txt, int Ni, int Nt,
                                                         int nq, int P, int paired, float* __restrict__ out) {
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long n = paired ? (long)Ni : (long)Ni * Nt;
    if (w >= n) return;
    const int i = paired ? (int)w : (int)(w / Nt), j = paired ? (int)w : (int)(w % Nt);
    const float* c = txt + (size_t)j * P;
    float best = -INFINITY;
    for (int q = 0; q < nq; ++q) {
        const float* a = img + ((size_t)i * nq + q) * P;
        float acc = 0.f;
        for (int p = lane; p < P; p += 64) acc = fmaf(a[p], c[p], acc);
        best = fmaxf(best, wave_sum(acc));
    }
    if (lane == 0) out[w] = best;
}

// ITM head of pair b: itm_head (W [2, D] + bias) on each of the nq query rows of x [B * nq, D], mean over them in row order ->
// logits [B, 2]; prob [B] = softmax(logits)[1] (what the reference keeps).  One wave per pair.
__global__ __launch_bounds__(64) void itm_head_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                      float* __restrict__ logits, float* __restrict__ prob, int nq, int D) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float s0 = 0.f, s1 = 0.f;
    for (int q = 0; q < nq; ++q) {
        const float* xr = x + ((size_t)b * nq + q) * D;
        float a0 = 0.f, a1 = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float v = xr[d];
            a0 = fmaf(v, W[d], a0);
            a1 = fmaf(v, W[D + d], a1);
        }
        s0 += wave_sum(a0) + bias[0];
        s1 += wave_sum(a1) + bias[1];
    }
    if (lane != 0) return;
    const float l0 = s0 / (float)nq, l1 = s1 / (float)nq;
    logits[2 * b] = l0;
    logits[2 * b + 1] = l1;
    if (prob) {
        const float mx = fmaxf(l0, l1), e0 = expf(l0 - mx), e1 = expf(l1 - mx);
        prob[b] = e1 / (e0 + e1);
    }
}

}  // namespace

int launch_itm_embed_text(int dtype, const int* ids, int L, const float* word, const float* pos, const float* gamma, const float* beta,
                          float eps, float* x_f, void* x_t, int M, int D, int V, hipStream_t s) {
    if (M < 1 || L < 1 || D < 1 || D > ITM_MAX_D || D % 8 || V < 1) {
        cap_set_error("itm_embed_text: bad shape M=%d L=%d D=%d V=%d (width a multiple of 8 up to %d)", M, L, D, V, ITM_MAX_D);
        return -1;
    }
    const dim3 grid((M + 3) / 4);
    if (dtype == CAP_DT_BF16)
        hipLaunchKernelGGL(itm_embed_text_kernel<bf16_t>, grid, dim3(256), 0, s, ids, L, word, pos, gamma, beta, eps, x_f, (bf16_t*)x_t, M, D, V);
    else if (dtype == CAP_DT_G8)
        hipLaunchKernelGGL(itm_embed_text_kernel<g8_t>, grid, dim3(256), 0, s, ids, L, word, pos, gamma, beta, eps, x_f, (g8_t*)x_t, M, D, V);
    else
        hipLaunchKernelGGL(itm_embed_text_kernel<float>, grid, dim3(256), 0, s, ids, L, word, pos, gamma, beta, eps, x_f, (float*)x_t, M, D, V);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_itm_self_attention(int dtype, const void* qkv_q, const void* qkv_t, const int* lens, void* ctx_q, void* ctx_t, int B, int nq,
                              int L, int H, int hd, hipStream_t s, int out_dtype) {
    if (out_dtype < 0) out_dtype = dtype;
    if (out_dtype != dtype && !(dtype == CAP_DT_F32 && out_dtype == CAP_DT_G8)) {
        cap_set_error("itm_self_attention: output type %d for input type %d is not supported here", out_dtype, dtype);
        return -1;
    }
    if (B < 1 || H < 1 || hd != ITM_HD || nq < 0 || nq > ITM_MAX_SEG || L < 0 || L > ITM_MAX_SEG || nq + L < 1 || (L > 0 && !lens) ||
        (nq > 0 && (!qkv_q || !ctx_q)) || (L > 0 && (!qkv_t || !ctx_t))) {
        cap_set_error("itm_self_attention: needs heads of %d and at most %d query + %d text rows per pair (B=%d H=%d hd=%d nq=%d L=%d)",
                      ITM_HD, ITM_MAX_SEG, ITM_MAX_SEG, B, H, hd, nq, L);
        return -1;
    }
    const float scale = 1.0f / sqrtf((float)hd);
#define CAP_ISA(TT, TO)                                                                                                            \
    hipLaunchKernelGGL((itm_self_attention_kernel<TT, TO>), dim3(B * H), dim3(64), 0, s, (const TT*)qkv_q, (const TT*)qkv_t, lens,    \
                       (TO*)ctx_q, (TO*)ctx_t, nq, L, H, scale)
    if (dtype == CAP_DT_BF16) CAP_ISA(bf16_t, bf16_t); else if (out_dtype == CAP_DT_G8) CAP_ISA(float, g8_t); else CAP_ISA(float, float);
#undef CAP_ISA
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_itc_head(const float* x, int rows_per, const float* W, const float* bias, float* out, int n, int D, int P, hipStream_t s) {
    if (n < 1 || D < 1 || D > ITM_MAX_D || P < 1 || P > ITM_MAX_P || rows_per < 1) {
        cap_set_error("itc_head: width %d / projection %d beyond the kernel's %d / %d (or no rows)", D, P, ITM_MAX_D, ITM_MAX_P);
        return -1;
    }
    hipLaunchKernelGGL(itc_head_kernel, dim3(n), dim3(HEAD_THREADS), 0, s, x, rows_per, W, bias, out, D, P);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_itc_scores(const float* img, const float* txt, int Ni, int Nt, int nq, int P, int paired, float* out, hipStream_t s) {
    if (Ni < 1 || Nt < 1 || nq < 1 || P < 1 || (paired && Ni != Nt)) {
        cap_set_error("cap_blip2_itc_scores: bad shape Ni=%d Nt=%d queries=%d P=%d (paired needs Ni == Nt)", Ni, Nt, nq, P);
        return -1;
    }
    const long n = paired ? (long)Ni : (long)Ni * Nt;
    if ((n + 3) / 4 > 0x7fffffffL) { cap_set_error("cap_blip2_itc_scores: %ld scores is too many for one launch", n); return -1; }
    hipLaunchKernelGGL(itc_scores_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, img, txt, Ni, Nt, nq, P, paired, out);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_itm_head(const float* x, const float* W, const float* bias, float* logits, float* prob, int B, int nq, int D, hipStream_t s) {
    if (B < 1 || nq < 1 || D < 1) { cap_set_error("itm_head: bad shape B=%d queries=%d D=%d", B, nq, D); return -1; }
    hipLaunchKernelGGL(itm_head_kernel, dim3(B), dim3(64), 0, s, x, W, bias, logits, prob, nq, D);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

CAP_DEFINE_G8_CLAMP_READER(cap_g8_clamped_blip2_itm)
