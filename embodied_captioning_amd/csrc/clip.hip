// The kernels of the CLIP scorer (CAP_ARCH_CLIP) that the other architectures do not have: the text tower's embeddings, the
// pooled head of both towers and the image-caption logits.  Replaces, per pair, HF `CLIPModel(**inputs).logits_per_image` as
// the reference's `--method clip` calls it (experimenting_env/captioner/pseudocaptioner.py:39-46, :352-357); the towers' blocks
// run on the shared encoder kernels (captioner.hip, run_clip_tower).
//
// Every sum here is formed in an order fixed by the row's own width - never by the batch - so an image or a caption has the
// same bits alone, in a batch of 256 or at the end of a partial micro-batch (tests/test_clip_gpu.py).
#include "common.h"
#include "ops.h"

namespace {

constexpr int HEAD_THREADS = 256, HEAD_MAX_D = 1024, HEAD_MAX_P = 1024;

// x[r, :] = tok[ids[r]] + pos[r % L] (fp32): CLIPTextEmbeddings, no LayerNorm, no token types.  One wave per row; ids
// outside [0, V) are clamped (the host validates them; the kernel never reads outside the table).
__global__ __launch_bounds__(256) void clip_embed_text_kernel(const int* __restrict__ ids, int L, const float* __restrict__ tok,
                                                              const float* __restrict__ pos, float* __restrict__ x, int M, int D,
                                                              int V) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const int id = min(max(ids[r], 0), V - 1), t = r % L;
    const float* te = tok + (size_t)id * D;
    const float* pe = pos + (size_t)t * D;
    float* xr = x + (size_t)r * D;
    for (int d = lane; d < D; d += 64) xr[d] = te[d] + pe[d];
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

// One workgroup per output row b: gather the pooled row of the tower's last hidden states (image: the CLS row b * rows_per;
// text: the EOT row b * rows_per + lens[b] - 1), LayerNorm it (post_layernorm / final_layer_norm), project with W [P, D] fp32
// (visual_projection / text_projection, no bias) and L2-normalise -> out fp32 [B, P].
__global__ __launch_bounds__(HEAD_THREADS) void clip_head_kernel(const float* __restrict__ x, int rows_per, const int* __restrict__ lens,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                 const float* __restrict__ W, float* __restrict__ out, int D, int P) {
    __shared__ float xs[HEAD_MAX_D], ys[HEAD_MAX_P], red[HEAD_THREADS];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int row = 0;
    if (lens) row = min(max(lens[b], 1), rows_per) - 1;
    const float* xr = x + ((size_t)b * rows_per + row) * D;
    float s = 0.f;
    for (int d = t; d < D; d += HEAD_THREADS) {
        const float v = xr[d];
        xs[d] = v;
        s += v;
    }
    const float mean = block_sum(s, red) / (float)D;
    float q = 0.f;
    for (int d = t; d < D; d += HEAD_THREADS) {
        const float c = xs[d] - mean;
        q = fmaf(c, c, q);
    }
    const float rstd = 1.0f / sqrtf(block_sum(q, red) / (float)D + eps);
    for (int d = t; d < D; d += HEAD_THREADS) xs[d] = (xs[d] - mean) * rstd * gamma[d] + beta[d];
    __syncthreads();
    for (int p = wave; p < P; p += HEAD_THREADS / 64) {
        const float* wr = W + (size_t)p * D;
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) acc = fmaf(xs[d], wr[d], acc);
        acc = wave_sum(acc);
        if (lane == 0) ys[p] = acc;
    }
    __syncthreads();
    float ss = 0.f;
    for (int p = t; p < P; p += HEAD_THREADS) ss = fmaf(ys[p], ys[p], ss);
    const float nrm = sqrtf(block_sum(ss, red));
    for (int p = t; p < P; p += HEAD_THREADS) out[(size_t)b * P + p] = ys[p] / nrm;
}

// out = exp(logit_scale) * <img[i], txt[j]>: one wave per logit.  paired: out[i] for (i, i), n = Ni; else out [Ni, Nt]
// (HF's logits_per_image).
__global__ __launch_bounds__(256) void clip_logits_kernel(const float* __restrict__ img, const float* __restrict__ txt, int Ni, int Nt,
                                                          int P, int paired, float logit_scale, float* __restrict__ out) {
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long n = paired ? (long)Ni : (long)Ni * Nt;
    if (w >= n) return;
    const int i = paired ? (int)w : (int)(w / Nt), j = paired ? (int)w : (int)(w % Nt);
    const float* a = img + (size_t)i * P;
    const float* c = txt + (size_t)j * P;
    float acc = 0.f;
    for (int p = lane; p < P; p += 64) acc = fmaf(a[p], c[p], acc);
    acc = wave_sum(acc);
    if (lane == 0) out[w] = expf(logit_scale) * acc;
}

}  // namespace

int launch_clip_embed_text(const int* ids, int L, const float* tok, const float* pos, float* x, int M, int D, int V, hipStream_t s) {
    if (M < 1 || L < 1 || D < 1 || V < 1) { cap_set_error("clip_embed_text: bad shape M=%d L=%d D=%d V=%d", M, L, D, V); return -1; }
    hipLaunchKernelGGL(clip_embed_text_kernel, dim3((M + 3) / 4), dim3(256), 0, s, ids, L, tok, pos, x, M, D, V);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_clip_head(const float* x, int rows_per, const int* lens, const float* gamma, const float* beta, float eps, const float* W,
                     float* out, int B, int D, int P, hipStream_t s) {
    if (B < 1 || D < 1 || D > HEAD_MAX_D || P < 1 || P > HEAD_MAX_P || rows_per < 1) {
        cap_set_error("clip_head: width %d / projection %d beyond the kernel's %d / %d (or no rows)", D, P, HEAD_MAX_D, HEAD_MAX_P);
        return -1;
    }
    hipLaunchKernelGGL(clip_head_kernel, dim3(B), dim3(HEAD_THREADS), 0, s, x, rows_per, lens, gamma, beta, eps, W, out, D, P);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_clip_logits(const float* img, const float* txt, int Ni, int Nt, int P, int paired, float logit_scale, float* out, hipStream_t s) {
    if (Ni < 1 || Nt < 1 || P < 1 || (paired && Ni != Nt)) {
        cap_set_error("cap_clip_logits: bad shape Ni=%d Nt=%d P=%d (paired needs Ni == Nt)", Ni, Nt, P);
        return -1;
    }
    const long n = paired ? (long)Ni : (long)Ni * Nt;
    if ((n + 3) / 4 > 0x7fffffffL) { cap_set_error("cap_clip_logits: %ld logits is too many for one launch", n); return -1; }
    hipLaunchKernelGGL(clip_logits_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, img, txt, Ni, Nt, P, paired, logit_scale, out);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}
