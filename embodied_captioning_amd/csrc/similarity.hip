// Cosine similarity of sentence embeddings on the device: the per-object caption DISAGREEMENT of the reference's exploration loop
// (`_cosine_distance`, experimenting_env/utils/projection_utils.py: mean of 1 - cos over an object's n x n matrix), the paper's
// offline pair statistics (scripts/compute_cosine_sim.py, captioner/test_cosine_similarity.py: mean / std of the pairwise cosine per
// (episode, object) group) and the plain similarity matrix / its paired diagonal (scripts/compute_performance_measures.py,
// sentence-transformers `similarity` / `similarity_pairwise`).
//
// Arithmetic: fp32 operands, products and sums; nothing narrower.  e^_i = fl(e_i * fl(1 / max(||e_i||, 1e-12))); s_ij is one fp32 fmaf
// chain of v_mfma_f32_32x32x2_f32 over e^_i[k] e^_j[k] in a FIXED k order: groups of 8 columns ascending, inside a group k = 8 ks + j,
// 8 ks + 4 + j for j = 0 .. 3 (the two lane halves of an MFMA hold the float4s at 8 ks and 8 ks + 4; columns past D are zeros).  It
// depends on rows i and j alone, so an entry has the same bits in the matrix form, on the paired diagonal and inside any group.  fp32 chains and their lengths (the bounds of tests/_similarity_ref.py
// are derived from exactly these):
//   ||e||^2       at most 16 fmaf per lane (D / 64 columns per lane), then a 6-level butterfly over the wave
//   s_ij          D fmaf, in the order above
//   tile sums     16 fmaf per lane (one 32 x 32 accumulator) for sum w s and sum w s^2; everything above a lane is fp64
//   sum vector    SIM_TILE (64) fmaf per column and 64-row chunk; chunks are added in fp64 and the total rounded to fp32 once
//   e^_i . m      D / 64 <= 16 fmaf per lane, then the butterfly
// fp64 combines partials in a fixed order that depends on the group's own size alone, and there is no floating-point atomic: a group's
// outputs are the same bits wherever it sits in the call and whatever else the call holds.
#include "common.h"
#include "ops.h"

namespace {

constexpr int SIM_TILE = 64;          // rows (and columns) of a Gram tile; four waves, one 32 x 32 accumulator each
constexpr int SIM_SUB = 32;
constexpr int SIM_KC = 64;            // k values staged per LDS pass
constexpr int SIM_PITCH = SIM_KC + 4; // floats: the 16 lanes of a ds_read_b128 phase (16 rows, one chunk) hit 16 distinct 4-bank slots
constexpr int SIM_THREADS = 256;
constexpr int SIM_MAX_D = 1024;
constexpr float SIM_NORM_FLOOR = 1e-12f;

enum { SIM_GROUPS = 0, SIM_MATRIX = 1, SIM_PAIRED = 2 };

static_assert(SIM_TILE == 2 * SIM_SUB && SIM_THREADS == 64 * 4, "four waves cover the tile as 2 x 2 accumulators");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// largest g in [0, G) with pre[g] <= x (pre non-decreasing, pre[0] = 0 <= x < pre[G])
__device__ __forceinline__ int find_group(const int* __restrict__ pre, int G, int x) {
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__host__ __device__ __forceinline__ int sim_chunks(int n) { return (n + SIM_TILE - 1) / SIM_TILE; }

// inv[r] = 1 / max(||e_r||, 1e-12): one wave per row
__global__ __launch_bounds__(SIM_THREADS) void sim_norm_kernel(const float* __restrict__ e, float* __restrict__ inv, int N, int D) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= N) return;
    const float* er = e + (size_t)r * D;
    float ss = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const f32x4 v = *(const f32x4*)(er + d);
#pragma unroll
        for (int j = 0; j < 4; ++j) ss = fmaf(v[j], v[j], ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) inv[r] = 1.0f / fmaxf(sqrtf(ss), SIM_NORM_FLOOR);
}

// cpre[g] = 64-row chunks before group g, tpre[g] = upper-triangle tiles before group g (g = 0 .. G): one workgroup, 1024 groups a round
__global__ __launch_bounds__(1024) void sim_scan_kernel(const int* __restrict__ off, int G, int* __restrict__ cpre, int* __restrict__ tpre) {
    __shared__ int sc[1024], st[1024];
    __shared__ int carry_c, carry_t;
    const int t = threadIdx.x;
    if (t == 0) { carry_c = 0; carry_t = 0; cpre[0] = 0; tpre[0] = 0; }
    __syncthreads();
    for (int g0 = 0; g0 < G; g0 += 1024) {
        const int g = g0 + t;
        int c = 0;
        if (g < G) c = sim_chunks(off[g + 1] - off[g]);
        sc[t] = c;
        st[t] = (int)((long)c * (c + 1) / 2);    // the host has checked that the call's total fits an int
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int ac = t >= o ? sc[t - o] : 0, at = t >= o ? st[t - o] : 0;
            __syncthreads();
            sc[t] += ac;
            st[t] += at;
            __syncthreads();
        }
        if (g < G) { cpre[g + 1] = carry_c + sc[t]; tpre[g + 1] = carry_t + st[t]; }
        __syncthreads();
        if (t == 1023) { carry_c += sc[t]; carry_t += st[t]; }
        __syncthreads();
    }
}

// cm[chunk][d] = sum over the chunk's rows j (ascending, one fp32 fmaf chain of <= 64) of w_j e^_j[d]
__global__ __launch_bounds__(SIM_THREADS) void sim_chunk_sum_kernel(const float* __restrict__ e, const float* __restrict__ inv,
                                                                    const float* __restrict__ w, const int* __restrict__ off,
                                                                    const int* __restrict__ cpre, int G, int D, float* __restrict__ cm) {
    __shared__ float ws[SIM_TILE], is[SIM_TILE];
    const int chunk = blockIdx.x, t = threadIdx.x;
    const int g = find_group(cpre, G, chunk);
    const int r0 = off[g] + (chunk - cpre[g]) * SIM_TILE, n = min(SIM_TILE, off[g + 1] - r0);
    if (t < SIM_TILE) {
        ws[t] = (t < n && w) ? w[r0 + t] : 1.0f;
        is[t] = t < n ? inv[r0 + t] : 0.f;
    }
    __syncthreads();
    for (int d = t * 4; d < D; d += SIM_THREADS * 4) {
        f32x4 acc = f32x4(0.f);
        for (int j = 0; j < n; ++j) {
            const f32x4 v = *(const f32x4*)(e + (size_t)(r0 + j) * D + d) * is[j];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(ws[j], v[q], acc[q]);
        }
        *(f32x4*)(cm + (size_t)chunk * D + d) = acc;
    }
}

// m[g][d] = fl32(sum over the group's chunks, ascending, in fp64)
__global__ __launch_bounds__(SIM_THREADS) void sim_group_sum_kernel(const float* __restrict__ cm, const int* __restrict__ cpre, int D,
                                                                    float* __restrict__ m) {
    const int g = blockIdx.x, c0 = cpre[g], c1 = cpre[g + 1];
    for (int d = threadIdx.x; d < D; d += SIM_THREADS) {
        double acc = 0.0;
        for (int c = c0; c < c1; ++c) acc += (double)cm[(size_t)c * D + d];
        m[(size_t)g * D + d] = (float)acc;
    }
}

// row_mean[i] = (e^_i . m_g - e^_i . e^_i) / (W_g - 1), 0 when W_g == 1: one wave per row.  wsum[g] = W_g (fp64, exact)
__global__ __launch_bounds__(SIM_THREADS) void sim_row_kernel(const float* __restrict__ e, const float* __restrict__ inv,
                                                              const int* __restrict__ off, int G, const float* __restrict__ m,
                                                              const double* __restrict__ wsum, int N, int D, float* __restrict__ row_mean) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= N) return;
    const int g = find_group(off, G, r);              // empty groups share a start: the last of them that starts at or before r is r's own
    const float* er = e + (size_t)r * D;
    const float* mg = m + (size_t)g * D;
    const float iv = inv[r];
    float t = 0.f, sii = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const f32x4 v = *(const f32x4*)(er + d) * iv, mv = *(const f32x4*)(mg + d);
#pragma unroll
        for (int j = 0; j < 4; ++j) { t = fmaf(v[j], mv[j], t); sii = fmaf(v[j], v[j], sii); }
    }
    t = wave_sum(t);
    sii = wave_sum(sii);
    const double W = wsum[g];
    if (lane == 0) row_mean[r] = W > 1.0 ? (float)(((double)t - (double)sii) / (W - 1.0)) : 0.f;
}

// wsum[g] = sum of the group's weights (integers: exact in fp64), one wave per group, lanes strided, fixed butterfly
__global__ __launch_bounds__(SIM_THREADS) void sim_weight_sum_kernel(const float* __restrict__ w, const int* __restrict__ off, int G,
                                                                     double* __restrict__ wsum) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= G) return;
    const int r0 = off[g], r1 = off[g + 1];
    double acc = 0.0;
    for (int r = r0 + lane; r < r1; r += 64) acc += w ? (double)w[r] : 1.0;
    acc = wave_sum_f64(acc);
    if (lane == 0) wsum[g] = acc;
}

struct SimTile {
    const float* a; const float* b;           // rows of the tile's row side / column side ([., D])
    const float* inva; const float* invb;
    const float* w;                           // SIM_GROUPS: weights (null = ones)
    const int* off; const int* tpre; int G;   // SIM_GROUPS
    int Na, Nb, D;
    double* part;                             // SIM_GROUPS: [tiles][2] = sum w s, sum w s^2 over the tile's unordered pairs
    float* out;                               // SIM_MATRIX [Na, Nb]; SIM_PAIRED [Na]
};

// One 64 x 64 tile of the Gram matrix of normalised rows.  Rows are staged through LDS once per tile, SIM_KC columns a pass, scaled
// by their inverse norm on the way in (rows past the side's end are zeros); wave (si, sj) holds the 32 x 32 block (si, sj) in one
// accumulator.  Epilogues: SIM_GROUPS reduces the tile's pairs (i < j: w_i w_j; i == j: w_i (w_i - 1) / 2, the pairs among a row's own
// copies; tiles below the diagonal are never launched), SIM_MATRIX stores the tile, SIM_PAIRED stores its diagonal.
template <int MODE>
__global__ __launch_bounds__(SIM_THREADS) void sim_tile_kernel(SimTile p) {
    __shared__ __attribute__((aligned(16))) float As[SIM_TILE * SIM_PITCH];
    __shared__ __attribute__((aligned(16))) float Bs[SIM_TILE * SIM_PITCH];
    __shared__ float wa[SIM_TILE], wb[SIM_TILE];
    __shared__ double red[4][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r32 = lane & 31, hh = lane >> 5;
    const int si = wave >> 1, sj = wave & 1;
    int rowA0, rowB0, endA, endB;
    bool diag = false;
    if constexpr (MODE == SIM_GROUPS) {
        const int tile = blockIdx.x, g = find_group(p.tpre, p.G, tile);
        const int local = tile - p.tpre[g];
        int tj = (int)((sqrt(8.0 * (double)local + 1.0) - 1.0) * 0.5);          // local = tj (tj + 1) / 2 + ti, ti <= tj
        while ((long)(tj + 1) * (tj + 2) / 2 <= local) ++tj;
        while ((long)tj * (tj + 1) / 2 > local) --tj;
        const int ti = local - (int)((long)tj * (tj + 1) / 2);
        rowA0 = p.off[g] + ti * SIM_TILE;
        rowB0 = p.off[g] + tj * SIM_TILE;
        endA = endB = p.off[g + 1];
        diag = ti == tj;
        if (t < SIM_TILE) {
            wa[t] = (p.w && rowA0 + t < endA) ? p.w[rowA0 + t] : 1.0f;
            wb[t] = (p.w && rowB0 + t < endB) ? p.w[rowB0 + t] : 1.0f;
        }
    } else if constexpr (MODE == SIM_MATRIX) {
        rowA0 = blockIdx.y * SIM_TILE; rowB0 = blockIdx.x * SIM_TILE; endA = p.Na; endB = p.Nb;
    } else {
        rowA0 = rowB0 = blockIdx.x * SIM_TILE; endA = endB = p.Na; diag = true;
    }
    const int lr = t >> 4, lc = (t & 15) * 4;       // staging: thread t moves columns lc .. lc + 3 of rows lr, lr + 16, lr + 32, lr + 48
    float iva[4], ivb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ra = rowA0 + lr + 16 * q, rb = rowB0 + lr + 16 * q;
        iva[q] = ra < endA ? p.inva[ra] : 0.f;
        ivb[q] = rb < endB ? p.invb[rb] : 0.f;
    }
    bool active = rowA0 + si * SIM_SUB < endA && rowB0 + sj * SIM_SUB < endB;
    if (MODE == SIM_GROUPS && diag && si > sj) active = false;
    if (MODE == SIM_PAIRED && si != sj) active = false;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const float* arow = As + (si * SIM_SUB + r32) * SIM_PITCH + hh * 4;
    const bool one_side = MODE == SIM_GROUPS && diag;      // a group's diagonal tile: both sides are the same rows, staged once
    const float* brow = (one_side ? As : Bs) + (sj * SIM_SUB + r32) * SIM_PITCH + hh * 4;
    for (int k0 = 0; k0 < p.D; k0 += SIM_KC) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = lr + 16 * q, ra = rowA0 + row, rb = rowB0 + row, k = k0 + lc;
            f32x4 va = f32x4(0.f), vb = f32x4(0.f);
            if (k < p.D) {
                if (ra < endA) va = *(const f32x4*)(p.a + (size_t)ra * p.D + k) * iva[q];
                if (!one_side && rb < endB) vb = *(const f32x4*)(p.b + (size_t)rb * p.D + k) * ivb[q];
            }
            *(f32x4*)(As + row * SIM_PITCH + lc) = va;
            if (!one_side) *(f32x4*)(Bs + row * SIM_PITCH + lc) = vb;
        }
        __syncthreads();
        if (active) {
            const int nks = min(SIM_KC, p.D - k0) / 8 + ((min(SIM_KC, p.D - k0) & 7) ? 1 : 0);   // columns past D are staged as zeros
#pragma unroll
            for (int ks = 0; ks < SIM_KC / 8; ++ks) {
                if (ks < nks) {
                    const f32x4 a = *(const f32x4*)(arow + ks * 8), b = *(const f32x4*)(brow + ks * 8);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
                }
            }
        }
    }
    // acc[e] = s[i][j], i = si 32 + (e & 3) + 8 (e >> 2) + 4 hh, j = sj 32 + r32 (tile-local)
    const int jl = sj * SIM_SUB + r32, jg = rowB0 + jl;
    if constexpr (MODE == SIM_GROUPS) {
        float p1 = 0.f, p2 = 0.f;
        if (active) {
            const float wj = wb[jl];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = si * SIM_SUB + (e & 3) + 8 * (e >> 2) + 4 * hh, ig = rowA0 + il;
                float wt = 0.f;
                if (ig < endA && jg < endB) {
                    const float wi = wa[il];
                    if (!diag || il < jl) wt = wi * wj;
                    else if (il == jl) wt = 0.5f * wi * (wi - 1.0f);
                }
                const float s = acc[e];
                p1 = fmaf(wt, s, p1);
                p2 = fmaf(wt * s, s, p2);
            }
        }
        const double d1 = wave_sum_f64((double)p1), d2 = wave_sum_f64((double)p2);
        if (lane == 0) { red[wave][0] = d1; red[wave][1] = d2; }
        __syncthreads();
        if (t == 0) {
            p.part[(size_t)blockIdx.x * 2] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
            p.part[(size_t)blockIdx.x * 2 + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        }
    } else if (active) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = si * SIM_SUB + (e & 3) + 8 * (e >> 2) + 4 * hh, ig = rowA0 + il;
            if (ig < endA && jg < endB) {
                if constexpr (MODE == SIM_MATRIX) p.out[(size_t)ig * p.Nb + jg] = acc[e];
                else if (il == jl) p.out[ig] = acc[e];
            }
        }
    }
}

// One wave per group: the tile partials in tile order (lane l takes tiles l, l + 64, ..., then the butterfly), the statistics, the medoid
__global__ __launch_bounds__(SIM_THREADS) void sim_finalize_kernel(const int* __restrict__ off, const int* __restrict__ tpre, int G, int D,
                                                                   const double* __restrict__ part, const float* __restrict__ m,
                                                                   const double* __restrict__ wsum, const float* __restrict__ row_mean,
                                                                   float* __restrict__ disagreement, float* __restrict__ pair_mean,
                                                                   float* __restrict__ pair_var, long long* __restrict__ pairs,
                                                                   int* __restrict__ medoid) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= G) return;
    const int r0 = off[g], r1 = off[g + 1];
    double s1 = 0.0, s2 = 0.0, mm = 0.0;
    for (int tl = tpre[g] + lane; tl < tpre[g + 1]; tl += 64) { s1 += part[(size_t)tl * 2]; s2 += part[(size_t)tl * 2 + 1]; }
    if (r1 > r0)
        for (int d = lane; d < D; d += 64) { const double v = (double)m[(size_t)g * D + d]; mm += v * v; }
    s1 = wave_sum_f64(s1); s2 = wave_sum_f64(s2); mm = wave_sum_f64(mm);
    float best = 0.f;
    int bi = -1;
    for (int r = r0 + lane; r < r1; r += 64) {
        const float v = row_mean[r];
        if (bi < 0 || v > best) { best = v; bi = r; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi >= 0 && (bi < 0 || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
    }
    if (lane != 0) return;
    const double W = r1 > r0 ? wsum[g] : 0.0;
    const long long np = (long long)(W * (W - 1.0) * 0.5);
    double mean = 0.0, var = 0.0;
    if (np > 0) {
        mean = s1 / (double)np;
        var = fmax(0.0, s2 / (double)np - mean * mean);
    }
    disagreement[g] = W > 0.0 ? (float)(1.0 - mm / (W * W)) : 0.f;
    pair_mean[g] = (float)mean;
    pair_var[g] = (float)var;
    pairs[g] = np;
    medoid[g] = bi < 0 ? -1 : bi;
}

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

struct SimLayout { size_t off, cpre, tpre, inv, wsum, cm, m, part, total; long chunks, tiles; };

// the workspace of (N, G, D, offsets); returns nullptr or the name of what is wrong with the grouping
const char* sim_layout(int N, int G, int D, const int* offsets, SimLayout* L) {
    if (N < 0 || G < 0) return "negative counts";
    if (!offsets) return "null offsets";
    if (D < 4 || D % 4 != 0) return "D % 4 != 0";
    if (D > SIM_MAX_D) return "D > 1024";
    if (offsets[0] != 0) return "offsets do not start at 0";
    long chunks = 0, tiles = 0;
    for (int g = 0; g < G; ++g) {
        if (offsets[g + 1] < offsets[g]) return "offsets decrease";
        const long c = sim_chunks(offsets[g + 1] - offsets[g]);
        chunks += c;
        tiles += c * (c + 1) / 2;
    }
    if (offsets[G] != N) return "offsets do not end at N";
    if (tiles > 0x7fffffffL) return "too many tiles for one launch";
    size_t o = 0;
    L->off = o;  o += up256((size_t)(G + 1) * 4);
    L->cpre = o; o += up256((size_t)(G + 1) * 4);
    L->tpre = o; o += up256((size_t)(G + 1) * 4);
    L->inv = o;  o += up256((size_t)N * 4);
    L->wsum = o; o += up256((size_t)G * 8);
    L->cm = o;   o += up256((size_t)chunks * D * 4);
    L->m = o;    o += up256((size_t)G * D * 4);
    L->part = o; o += up256((size_t)tiles * 16);
    L->total = o;
    L->chunks = chunks;
    L->tiles = tiles;
    return nullptr;
}

}  // namespace

size_t sim_group_workspace(int N, int G, int D, const int* offsets) {
    SimLayout L;
    const char* bad = sim_layout(N, G, D, offsets, &L);
    if (bad) { cap_set_error("cap_group_similarity_workspace: %s (N=%d G=%d D=%d)", bad, N, G, D); return 0; }
    return L.total;
}

int launch_cosine_matrix(const float* a, const float* b, int Na, int Nb, int D, int paired, float* out, void* ws, size_t ws_bytes,
                         hipStream_t s) {
    if (!a || !b || !out || !ws) { cap_set_error("cap_cosine_matrix: null buffer"); return -1; }
    if (Na < 0 || Nb < 0) { cap_set_error("cap_cosine_matrix: negative counts Na=%d Nb=%d", Na, Nb); return -1; }
    if (D < 4 || D % 4 != 0) { cap_set_error("cap_cosine_matrix: D % 4 != 0 (D=%d)", D); return -1; }
    if (D > SIM_MAX_D) { cap_set_error("cap_cosine_matrix: D > 1024 (D=%d)", D); return -1; }
    if (paired && Na != Nb) { cap_set_error("cap_cosine_matrix: paired needs Na == Nb (Na=%d Nb=%d)", Na, Nb); return -1; }
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)ws) & 15) != 0) { cap_set_error("cap_cosine_matrix: buffers are not 16-byte aligned"); return -1; }
    const size_t need = ((size_t)Na + Nb) * sizeof(float);
    if (ws_bytes < need) { cap_set_error("cap_cosine_matrix: workspace too small (%zu bytes, %zu needed)", ws_bytes, need); return -1; }
    if (!paired && sim_chunks(Na) > 65535) { cap_set_error("cap_cosine_matrix: Na=%d is too many rows for one launch", Na); return -1; }
    if (Na == 0 || Nb == 0) return 0;
    float* inva = (float*)ws;
    float* invb = inva + Na;
    hipLaunchKernelGGL(sim_norm_kernel, dim3((Na + 3) / 4), dim3(SIM_THREADS), 0, s, a, inva, Na, D);
    hipLaunchKernelGGL(sim_norm_kernel, dim3((Nb + 3) / 4), dim3(SIM_THREADS), 0, s, b, invb, Nb, D);
    SimTile p{};
    p.a = a; p.b = b; p.inva = inva; p.invb = invb; p.Na = Na; p.Nb = Nb; p.D = D; p.out = out;
    const int ta = sim_chunks(Na), tb = sim_chunks(Nb);
    if (paired) {
        hipLaunchKernelGGL(sim_tile_kernel<SIM_PAIRED>, dim3(ta), dim3(SIM_THREADS), 0, s, p);
    } else {
        hipLaunchKernelGGL(sim_tile_kernel<SIM_MATRIX>, dim3(tb, ta), dim3(SIM_THREADS), 0, s, p);
    }
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_group_similarity(const float* e, const int* offsets, const float* weights, int N, int G, int D, float* disagreement,
                            float* pair_mean, float* pair_var, long long* pairs, int* medoid, float* row_mean, void* ws, size_t ws_bytes,
                            hipStream_t s) {
    SimLayout L;
    const char* bad = sim_layout(N, G, D, offsets, &L);
    if (bad) { cap_set_error("cap_group_similarity: %s (N=%d G=%d D=%d)", bad, N, G, D); return -1; }
    if (!ws || (G > 0 && (!disagreement || !pair_mean || !pair_var || !pairs || !medoid)) || (N > 0 && (!e || !row_mean))) {
        cap_set_error("cap_group_similarity: null buffer");
        return -1;
    }
    if ((((uintptr_t)e | (uintptr_t)ws) & 15) != 0) { cap_set_error("cap_group_similarity: buffers are not 16-byte aligned"); return -1; }
    if (ws_bytes < L.total) { cap_set_error("cap_group_similarity: workspace too small (%zu bytes, %zu needed)", ws_bytes, L.total); return -1; }
    if (G == 0) return 0;
    char* base = (char*)ws;
    int* d_off = (int*)(base + L.off);
    int* cpre = (int*)(base + L.cpre);
    int* tpre = (int*)(base + L.tpre);
    float* inv = (float*)(base + L.inv);
    double* wsum = (double*)(base + L.wsum);
    float* cm = (float*)(base + L.cm);
    float* m = (float*)(base + L.m);
    double* part = (double*)(base + L.part);
    CAP_HIP_CHECK(hipMemcpyAsync(d_off, offsets, (size_t)(G + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(sim_scan_kernel, dim3(1), dim3(1024), 0, s, d_off, G, cpre, tpre);
    hipLaunchKernelGGL(sim_weight_sum_kernel, dim3((G + 3) / 4), dim3(SIM_THREADS), 0, s, weights, d_off, G, wsum);
    if (N > 0) {
        hipLaunchKernelGGL(sim_norm_kernel, dim3((N + 3) / 4), dim3(SIM_THREADS), 0, s, e, inv, N, D);
        hipLaunchKernelGGL(sim_chunk_sum_kernel, dim3((unsigned)L.chunks), dim3(SIM_THREADS), 0, s, e, inv, weights, d_off, cpre, G, D, cm);
    }
    hipLaunchKernelGGL(sim_group_sum_kernel, dim3(G), dim3(SIM_THREADS), 0, s, cm, cpre, D, m);
    if (N > 0) {
        hipLaunchKernelGGL(sim_row_kernel, dim3((N + 3) / 4), dim3(SIM_THREADS), 0, s, e, inv, d_off, G, m, wsum, N, D, row_mean);
        SimTile p{};
        p.a = e; p.b = e; p.inva = inv; p.invb = inv; p.w = weights; p.off = d_off; p.tpre = tpre; p.G = G; p.Na = N; p.Nb = N; p.D = D;
        p.part = part;
        hipLaunchKernelGGL(sim_tile_kernel<SIM_GROUPS>, dim3((unsigned)L.tiles), dim3(SIM_THREADS), 0, s, p);
    }
    hipLaunchKernelGGL(sim_finalize_kernel, dim3((G + 3) / 4), dim3(SIM_THREADS), 0, s, d_off, tpre, G, D, part, m, wsum, row_mean,
                       disagreement, pair_mean, pair_var, pairs, medoid);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}
