// Host side of libcaptioner_hip.so: weight registry, arena, the encoder / decoder launch sequences and the C ABI
// declared in include/captioner_hip.h.  Everything on the data path is a kernel launch on the caller's stream; the
// launch sequences never allocate or synchronise (so they can be captured into a hipGraph).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <map>
#include <string>
#include <set>
#include <mutex>
#include <vector>

#include "../../include/captioner_hip.h"
#include "gemm.h"
#include "ops.h"
#include "decode_small.h"

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[2048] = "";
void cap_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int cap_kernel_setup(const void* kernel, int lds_bytes, int* n_cu) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    static std::map<int, int> cus;
    int dev = 0;
    CAP_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (!done.count({kernel, dev})) {
        if (lds_bytes > 64 * 1024)
            CAP_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        done.insert({kernel, dev});
    }
    if (n_cu) {
        auto it = cus.find(dev);
        if (it == cus.end()) {
            int n = 0;
            CAP_HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
            it = cus.emplace(dev, n).first;
        }
        *n_cu = it->second;
    }
    return 0;
}

namespace {

struct Slot {            // where one checkpoint tensor (or a row range of a fused tensor) lives
    void* dst = nullptr;
    int dtype = CAP_DT_F32;   // storage type at dst: compute dtype or fp32
    int64_t rows = 0, cols = 0;
    int dst_ld = 0;
    void* aux = nullptr;      // CAP_DT_I8W: the rows' fp32 scales
    bool loaded = false;
};

struct ProfTag { std::string tag; double flops, bytes; hipEvent_t e0, e1; };

// What an arena allocation holds between ABI calls (DESIGN.md "Arena state"; cap_debug_fill_arena / cap_debug_arena_kinds):
//   ARENA_SCRATCH  fp32 / compute-type / KV16 data a call writes before it reads: no result may depend on what it held before
//   ARENA_INDEX    int32 tables (token rows, row maps, beam ancestry and the beam state block): a value here becomes an address
//   ARENA_KEPT     initialised at create, or carrying state from one ABI call to a later one by documented contract
enum { ARENA_SCRATCH = 0, ARENA_INDEX = 1, ARENA_KEPT = 2, ARENA_KINDS = 3 };
struct ArenaAlloc { void* p; size_t bytes; int kind; const char* name; };   // bytes: as allocated (rounded up to 256)

// The weights of one model on one GPU: device buffers in allocation order + the name -> buffer registry.  Read-only once
// loaded, so every handle of an EnginePool points at the same store (cap_create_shared): a pool of n engines costs one copy
// of the weights plus n arenas.  Freed when the last handle that references it is destroyed.
struct WeightStore {
    std::vector<void*> ptrs;
    std::vector<size_t> sizes;
    std::multimap<std::string, Slot> slots;
    size_t bytes = 0;
    std::atomic<int> refs{1};
    int device = 0;
};

// One projection y = x W^T + b: the weight [N, K] in the GEMM operand type (torch Linear layout, rows ld apart - K everywhere but
// the patch weight, padded to Kpad), the fp32 bias [N] or null, and with CapConfig.weight_int8 the fp32 row scales [N] of an int8
// weight in fragment order.  A fused projection (q|k|v, the cross K/V of all layers) is ONE Linear over all its rows.
struct Linear {
    void* w = nullptr;
    float *b = nullptr, *scale = nullptr;
    int N = 0, K = 0, ld = 0;
};
// a bias-less Linear over a buffer someone else owns: a tied head on the fp32 table, the dequantised scratch of an int8 weight
inline Linear linear_over(void* w, int N, int K) { Linear L; L.w = w; L.N = N; L.K = L.ld = K; return L; }
struct Norm { float *g = nullptr, *b = nullptr; };   // a LayerNorm's gamma, beta
enum OutType { OUT_T = 0, OUT_F32 = 1 };             // a GEMM's output: the operand type, or fp32 (GemmParams::out_f32)

struct VLayer {
    Linear qkv, proj, fc1, fc2;
    Norm ln1, ln2;
};
// int8 weights: up to this many crops per call the prompt pass (crops x 33 rows) runs on the weight-streaming kernels like a decode
// step; beyond, it is a GEMM proper and goes to the tiled kernels (run_opt).  Within each range a crop's bits do not depend on the
// batch it is in; across the two the prompt's sums are formed in a different order (fp32-rounding-level differences before the bf16
// roundings).
constexpr int kI8SkinnyPromptCrops = 4;

struct OLayer {            // OPT decoder layer (pre-LN): fused q|k|v, out_proj, fc1 (ReLU), fc2; K/V caches [B][Lmax][T]
    Linear qkv, o, f1, f2;     // (CapConfig.weight_int8: int8 weights with row scales)
    Norm ln1, ln2;
    void *kc, *vc;
};

// A sub-layer is two projections around its core, followed by bias + residual + ONE LayerNorm.  The BLIP and CoCa text decoders
// are ONE list of sub-layers (run_step / run_step_small walk it; build_blip / build_coca fill it once; the tail is a split-K
// consumer); a post-LN encoder layer (PostLayer below) is made of the same struct.
//   DEC_SELF   q|k|v projection [3W, W] -> causal attention over the self cache -> output projection [W, W]
//   DEC_CROSS  query projection [W, W]  -> attention over the image's K/V        -> output projection [W, W]
//   DEC_FFN    fc [F, W] (GELU)                                                  -> projection back  [W, F]
// BLIP is post-LN: [SELF, CROSS, FFN] per layer, the LayerNorm is the sub-layer's own, its output is the next operand AND the new
// residual row.  CoCa is pre-LN: [SELF, FFN] per unimodal / multimodal self block, [CROSS, FFN] per cross block, the LayerNorm is
// the NEXT sub-layer's (ln_2 of the block, ln_1 of the next block, ln_final after the last), the residual row is the sum.
enum { DEC_SELF = 0, DEC_CROSS = 1, DEC_FFN = 2 };
struct SubLayer {
    int kind = DEC_FFN;
    Linear in, out;
    Norm ln;                                  // the LayerNorm applied to the sub-layer's result (see above)
    void* cache = nullptr;                    // decoder DEC_SELF: [k|v][R][H][max_len][64] in the activation type (arena)
    int slot = -1;                            // decoder DEC_CROSS: layer index inside the cross K/V cache
};
// Profile tags of the decoder's launches, indexed by sub-layer kind.  Batch kernels: input GEMM, attention, output GEMM; fused
// small-batch kernels: the sub-layer's first and second launch.
struct DecTags {
    const char *in[3], *attn[2], *out[3], *tr, *ln, *vocab;
    const char *s_in[3], *s_out[3], *s_tr, *s_vocab;
};
const DecTags kBlipDecTags = {{"dec_gemm_qkv", "dec_gemm_cq", "dec_gemm_f1"}, {"dec_self_attn", "dec_cross_attn"},
                              {"dec_gemm_so", "dec_gemm_co", "dec_gemm_f2"}, "dec_gemm_tr", "dec_layernorm", "dec_gemm_vocab",
                              {"dec_small_qkv", "dec_small_cross", "dec_small_f1"}, {"dec_small_so", "dec_small_co", "dec_small_f2"},
                              "dec_small_tr", "dec_small_vocab"};
const DecTags kCocaDecTags = {{"coca_gemm_qkv", "coca_gemm_cq", "coca_gemm_fc"}, {"coca_self_attn", "coca_cross_attn"},
                              {"coca_gemm_o", "coca_gemm_o", "coca_gemm_pr"}, nullptr, nullptr, "coca_gemm_vocab",
                              {"coca_small_qkv", "coca_small_cross", "coca_small_fc"}, {"coca_small_o", "coca_small_o", "coca_small_pr"},
                              nullptr, "coca_small_vocab"};
struct DecPlan {
    std::vector<SubLayer> subs;
    bool pre_ln = false;          // CoCa (SmallLN::x_is_sum; the batch consumer's y_out instead of out_f)
    bool skip_finished = false;   // BLIP greedy: ended captions' rows are left alone.  CoCa computes them: their step logits are observable
    int W = 0;                    // width: t_hidden (BLIP), embed_dim (CoCa)
    // cross K/V cache [slot][k|v][image][head][kv_tokens][64]: BLIP keeps the NT image tokens and attends all of them, CoCa keeps
    // the pooler's Q tokens and skips the first (the pooled token)
    int kv_tokens = 0, kv_first = 0, kv_keys = 0;
    // embedding: LayerNorm(word[token] + pos[t]) with the embeddings' own LayerNorm (BLIP) or the first sub-layer's ln_1 (CoCa)
    float *word = nullptr, *pos = nullptr;
    Norm emb;
    // head: BLIP transform (dense + GELU, LayerNorm) then the vocabulary GEMM with a bias; CoCa the vocabulary GEMM alone (tr.w
    // null: ln_final is the last sub-layer's LayerNorm).  vocab is tied: in the fp32 mode BLIP's weight IS the fp32 table
    Linear tr, vocab;
    Norm tr_ln;
    const DecTags* tags = nullptr;
};

// One layer of a post-LN (BERT-style) encoder - the BLIP-2 Q-Former, the sentence encoder - as sub-layers (reg_post_layers fills
// them, run_qformer / run_text_encoder walk them): self (q|k|v in), on the Q-Former's cross layers cross (query in; the image's
// k|v projection [2 W, D] is the layer's ckv), ffn, and with CAP_ARCH_BLIP2_ITM ffn_text: the text rows' own FFN.
struct PostLayer {
    bool has_cross = false;
    SubLayer self, cross, ffn, ffn_text;
    Linear ckv;
};
// The activations of a post-LN encoder over R rows of width W, FFN width F (alloc_post_rows)
struct PostRows {
    float *x = nullptr, *y = nullptr;          // fp32 [R, W]: the stream (LayerNorm output = next residual), the pre-LayerNorm sum
    void *x_t = nullptr, *qkv = nullptr, *ctx = nullptr, *h = nullptr;   // [R, W] operand copy of x, [R, 3 W], [R, W], [R, F] in the compute type
};
struct PostDims { int W, F; float eps; };
// Profile tags of one row set's launches (null: the pass has no such launch; ln null: the LayerNorms are not recorded)
struct PostTags { const char *qkv, *self_attn, *so, *cq, *ckv, *cross_attn, *co, *f1, *f2, *ln; };
const PostTags kQformerTags = {"qf_gemm_qkv", "qf_self_attn", "qf_gemm_so", "qf_gemm_cq", "qf_gemm_ckv", "qf_cross_attn", "qf_gemm_co",
                               "qf_gemm_f1", "qf_gemm_f2", nullptr};
const PostTags kItmQueryTags = {"itm_gemm_qkv_q", "itm_self_attn", "itm_gemm_so_q", "itm_gemm_cq", "itm_gemm_ckv", "itm_cross_attn",
                                "itm_gemm_co", "itm_gemm_f1_q", "itm_gemm_f2_q", nullptr};
const PostTags kItmTextTags = {"itm_gemm_qkv_t", "itm_self_attn", "itm_gemm_so_t", nullptr, nullptr, nullptr, nullptr, "itm_gemm_f1_t",
                               "itm_gemm_f2_t", nullptr};
const PostTags kMiniLMTags = {"te_gemm_qkv", "te_attention", "te_gemm_o", nullptr, nullptr, nullptr, nullptr, "te_gemm_f1", "te_gemm_f2",
                              "te_layernorm"};

// The ViT branch GEMMs (proj, fc2) of the MFMA-staged types add their output to the residual stream X IN PLACE (gemm_pp.hip's
// residual epilogue: C = acc + bias + C) and the next LayerNorm reads X once.  The older scheme - branch output to `delta`, the
// add+LayerNorm kernel reads delta and X and writes X back - moves 5 x M x D x 4 bytes per (GEMM, LayerNorm) pair against 4 here,
// and stays for the exact fp32 mode, whose stream kernels have no residual operand.  Same fp32 add of the same two operands: the
// residual stream has the same bits either way.
inline bool vit_adds_in_place(int gdt) { return gdt != CAP_DT_F32; }

// The activations of a pre-LN transformer tower over M rows (alloc_tower).
struct Tower {
    float* X = nullptr;          // fp32 residual stream [M, D]
    float* delta = nullptr;      // exact fp32 mode: the branch output (proj / fc2) the next add+LayerNorm folds into X; fp32 [M, D]
    void *ln = nullptr, *qkv = nullptr, *ctx = nullptr, *mlp = nullptr;   // [M, D], [M, 3D], [M, D], [M, F] in the compute type
};
// Profile tags of one tower's launches (patchify / patch: image towers only)
struct TowerTags { const char *patchify, *patch, *ln, *qkv, *attn, *proj, *fc1, *fc2; };
const TowerTags kEncoderTags = {"patchify", "gemm_patch", "layernorm", "gemm_qkv", "vit_attention", "gemm_proj", "gemm_fc1", "gemm_fc2"};
const TowerTags kClipImageTags = {"clip_patchify", "clip_v_gemm_patch", "clip_v_layernorm", "clip_v_gemm_qkv", "clip_v_attention",
                                  "clip_v_gemm_proj", "clip_v_gemm_fc1", "clip_v_gemm_fc2"};
const TowerTags kClipTextTags = {nullptr, nullptr, "clip_t_layernorm", "clip_t_gemm_qkv", "clip_t_attention", "clip_t_gemm_proj",
                                 "clip_t_gemm_fc1", "clip_t_gemm_fc2"};

struct Captioner {
    CapConfig c;
    int dt; size_t esz;          // storage type of activations / K-V caches that kernels other than the GEMMs read
    int gdt;                     // type of every GEMM operand (A and W): == dt, except CAP_F32_SPLIT: dt = fp32, gdt = G8
                                 // (split fp16, common.h) - there every kernel whose output feeds a GEMM writes G8
    // output of a GEMM that an attention kernel reads (q, k, v): fp32 in the split mode, where only GEMM operands are G8
    OutType attn_out() const { return gdt == CAP_DT_G8 ? OUT_F32 : OUT_T; }
    int NT, P, Kpatch, Kpad;
    bool kv16 = false;           // split mode: the cross-attention K/V cache is KV16 (int16 + one scale per head row, common.h) instead of fp32
    size_t kvrow = 0;            // bytes of one 64-wide head row of that cache (KV16: 132, amortised)
    // bytes of one (layer, k | v) block of the cross cache holding `rows` head rows
    size_t cross_block(size_t rows) const { return kv16 ? kv16_block_bytes(rows) : rows * kvrow; }
    size_t dev_bytes = 0;        // arena (+ the weights when this handle created the store)
    std::vector<ArenaAlloc> allocs;   // arena: owned by this handle
    WeightStore* ws = nullptr;   // weights: shared
    bool replay = false;         // building a handle on an existing store: walloc hands out the store's buffers in order
    size_t wcur = 0;
    float* stage = nullptr; size_t stage_elems = 0;
    unsigned int* absmax_dev = nullptr;   // cap_load_weight: max |w| of a tensor bound for a G8 slot (range check)
    // early exit of the decode loop (cap_set_early_exit): poll every `poll` steps through a host-mapped word
    int poll = 0; int* host_flag = nullptr; int* host_flag_dev = nullptr;
    // banned tokens / sequences (cap_set_bad_words; ops.h, BanSet): device storage of its own, allocated at the first non-empty set
    // (never part of the arena) and freed with the handle; the host copies are what the uploads read
    unsigned* ban_bits = nullptr; int* ban_multi = nullptr;
    int ban_n_single = 0, ban_n_multi = 0;
    std::vector<unsigned> ban_bits_host; std::vector<int> ban_multi_host;
    bool banned() const { return ban_n_single > 0 || ban_n_multi > 0; }
    BanSet ban_set() const { BanSet b; b.bits = ban_bits; b.multi = ban_multi; b.n_multi = ban_n_multi; return b; }
    // repetition controls (cap_set_repeat_controls; ops.h, RepeatCtl): two numbers, no storage; image_token = the id of BLIP-2's image
    // placeholders as HF's processors see them in front of BOS (cap_set_image_token; -1 = not given)
    float rep_penalty = 1.f; int rep_ngram = 0; int image_token = -1;
    bool repeat_active() const { return rep_penalty != 1.f || rep_ngram > 0; }
    RepeatCtl repeat_ctl() const {
        RepeatCtl r; r.penalty = rep_penalty; r.ngram = rep_ngram;
        if (c.arch == CAP_ARCH_BLIP2) { r.vn = c.num_query_tokens; r.vtok = image_token; r.vbos = c.bos; }
        return r;
    }
    // sampling (cap_set_sampling; ops.h, SampleCtl): the greedy loop draws its tokens instead of taking the arg-max
    bool sampling = false; SampleCtl sample_ctl;
    const uint64_t* call_keys = nullptr;   // the keys of the call in flight (cap_generate_sampled; null: the row index)
    int last_steps = 0;          // decode steps the last cap_generate ran (cap_last_decode_steps)
    int decode_path = 0;         // cap_set_decode_path: 0 = by row count (<= SMALL_MAX_ROWS rows: the fused small-batch kernels),
                                 // 1 = always the batch kernels, 2 = always the small-batch kernels (an error beyond their row limit)
    int last_path = 0;           // what the last cap_generate's decode steps ran on (cap_last_decode_path): 1 batch, 2 small-batch
    int compaction = 1;          // cap_set_row_compaction: 1 = the greedy batch path works on the open captions' rows only (RowMap)
    int last_prefill_passes = 0; // prefill passes of the last prompted generate (cap_last_prefill_passes): 1 when the workspace held the batch
    int last_compacted = 0;      // did the last cap_generate's decode loop run compacted (cap_last_row_compaction)
    int last_score_passes = 0;   // decoder passes of the last cap_score_captions (cap_last_score_passes)
    int *live = nullptr, *n_live = nullptr;       // RowMap storage: int32 [max rows] + the count
    // vision weights (patch: [D, Kpatch] in rows of Kpad; post: the image tower's final LayerNorm - CoCa: the pooler's ln_k)
    float *cls, *vpos;
    Linear patch; Norm ln_pre, post;
    std::vector<VLayer> vl;
    // text weights (ckv: the decoder's cross K/V projections of all layers as one)
    float *word_f32, *tpos;
    Norm emb; Linear ckv;
    std::vector<PostLayer> pl;   // post-LN encoder layers: the Q-Former's (BLIP-2, the image-text scorer) or the sentence encoder's
    DecPlan dec;                 // BLIP / CoCa text decoder
    // arena
    void *patches, *emb_t, *cross;
    Tower vt;                    // the image tower's activations (CLIP's text tower: ct)
    float* emb_f;
    int *seq, *finished, *lens, *anc;
    float *dx, *dy, *logits, *dpart;
    float* dx2 = nullptr;        // fused decode paths: second fp32 LayerNorm row buffer (ping-pong with dx), as many rows as dx
    void *dx_t, *dq, *dctx, *dh;
    void* beam = nullptr;
    size_t cache_layer_bytes = 0;
    size_t ws_rows = 0;          // rows the decoder's pass buffers (dx, dx_t, dctx, dh, dpart) hold: the decode rows, or a whole prompt prefill's
    size_t head_rows = 0;        // rows the head's buffers (dy, logits) hold: the decode rows, or CapConfig.max_score_rows
    // ---- CoCa (CAP_ARCH_COCA)
    int Q = 0, E = 0;
    Norm lnpost; Linear pool_kv, pool_out;
    float *pool_q = nullptr, *ones = nullptr, *zeros = nullptr, *pool_o = nullptr, *img_tokens = nullptr;
    void *pool_kvbuf = nullptr, *pool_ctx = nullptr, *xhat = nullptr;
    int ldl;
    // ---- BLIP-2 (CAP_ARCH_BLIP2)
    std::vector<OLayer> ol;
    bool wq8 = false;            // CapConfig.weight_int8: the OPT decoder's Linear weights are row-quantised int8 (gemm_skinny.hip)
    void* w8_scratch = nullptr;  // one weight matrix as row-major bf16 integers: the prompt pass of more than kI8SkinnyPromptCrops crops
    float *q_x0 = nullptr, *o_tok = nullptr, *o_pos = nullptr;
    Norm o_lnf; Linear lproj, o_head;        // o_head: the tied LM head [vocab, T], no bias - the token table o_tok in the operand type
    PostRows qr;                 // the Q-Former's query rows [max_batch * num_query_tokens, .] (the image-text scorer's too)
    float *lm_proj = nullptr, *ox = nullptr;      // activations
    void *qkvimg = nullptr, *oh_t = nullptr, *oqkv = nullptr, *octx = nullptr, *off = nullptr;
    // ---- sentence encoder (CAP_ARCH_MINILM): layers in pl, token-type row 0, activations [max_batch * max_len, .]
    float* tok_type = nullptr;
    PostRows te;
    // ---- CLIP scorer (CAP_ARCH_CLIP): image tower on the encoder's (vl, vt), text tower on its own [max_batch * max_len, .]
    // rows; projections fp32 [embed_dim, width] for the pooled head kernel
    std::vector<VLayer> ctl;
    Tower ct;
    float *c_vproj = nullptr, *c_tproj = nullptr, *c_tok = nullptr, *c_logit = nullptr; Norm c_lnf;
    // ---- BLIP-2 image-text scorer (CAP_ARCH_BLIP2_ITM): image tower on (vl, vt), Q-Former layers in pl with both FFN sets; the
    // text rows tr [max_batch * max_len, .] beside the query rows qr; heads fp32 for the head kernels.  itm_ckv holds the cross
    // K/V of every cross-attention layer for the itm_B images of the last cap_blip2_itm_encode_images: [layer][B * NT, 2 Q]
    // (itm_ckv_slot).
    float *i_word = nullptr, *i_pos = nullptr, *i_vproj = nullptr, *i_vproj_b = nullptr, *i_tproj = nullptr, *i_tproj_b = nullptr,
          *i_head = nullptr, *i_head_b = nullptr; Norm i_ln;
    PostRows tr;
    void* itm_ckv = nullptr;
    int itm_B = 0;
    // profiling
    bool prof = false;
    std::vector<ProfTag> prof_recs;
};

// name: required for every kind but ARENA_SCRATCH (cap_debug_arena_kinds reports it)
int dev_alloc(Captioner* m, void** p, size_t bytes, int kind = ARENA_SCRATCH, const char* name = nullptr) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    CAP_HIP_CHECK(hipMalloc(p, bytes));
    m->allocs.push_back({*p, bytes, kind, name});
    m->dev_bytes += bytes;
    return 0;
}

#define TRY(x) do { if ((x) != 0) return -1; } while (0)

// weight buffer: a new allocation recorded in the store, or (replay) the store's next buffer - the build_* functions run
// the same sequence of calls for the same architecture, which the size check enforces
int walloc(Captioner* m, void** p, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    WeightStore* ws = m->ws;
    if (m->replay) {
        if (m->wcur >= ws->ptrs.size() || ws->sizes[m->wcur] != bytes) {
            cap_set_error("cap_create_shared: the configuration does not describe the model whose weights are shared "
                          "(buffer %zu: %zu bytes wanted)", m->wcur, bytes);
            return -1;
        }
        *p = ws->ptrs[m->wcur++];
        return 0;
    }
    CAP_HIP_CHECK(hipMalloc(p, bytes));
    ws->ptrs.push_back(*p);
    ws->sizes.push_back(bytes);
    ws->bytes += bytes;
    m->dev_bytes += bytes;
    return 0;
}

int add_slot(Captioner* m, const std::string& name, void* dst, int dtype, int64_t rows, int64_t cols, int dst_ld = 0, void* aux = nullptr) {
    if (m->replay) return 0;
    Slot s; s.dst = dst; s.dtype = dtype; s.rows = rows; s.cols = cols; s.dst_ld = dst_ld ? dst_ld : (int)cols; s.aux = aux;
    m->ws->slots.insert({name, s});
    return 0;
}

// allocate a fp32 vector and register it
int reg_f32(Captioner* m, const std::string& name, float** p, int64_t n) {
    TRY(walloc(m, (void**)p, n * 4));
    return add_slot(m, name, *p, CAP_DT_F32, 1, n);
}
// allocate a compute-dtype weight [N, K] and register it.  ld > K (the patch weight): rows of ld columns, zero from K on - the
// product runs over all of them, so the Linear's K is ld
int reg_mat(Captioner* m, const std::string& name, Linear& L, int N, int K, int ld = 0) {
    L.N = N; L.K = L.ld = ld ? ld : K;
    TRY(walloc(m, &L.w, (size_t)N * L.ld * m->esz));
    if (L.ld != K && !m->replay) CAP_HIP_CHECK(hipMemset(L.w, 0, (size_t)N * L.ld * m->esz));
    return add_slot(m, name, L.w, m->gdt, N, K, L.ld);
}
// allocate an int8 weight [N, K] in fragment order + its row scales and register it (CapConfig.weight_int8)
int reg_mat_i8(Captioner* m, const std::string& name, Linear& L, int N, int K) {
    L.N = N; L.K = L.ld = K;
    TRY(walloc(m, &L.w, (size_t)N * K));
    TRY(walloc(m, (void**)&L.scale, (size_t)N * 4));
    return add_slot(m, name, L.w, CAP_DT_I8W, N, K, 0, L.scale);
}
// the plain projection: p + "weight" [N, K] and p + "bias" [N]
int reg_linear(Captioner* m, const std::string& p, Linear& L, int N, int K, int ld = 0) {
    TRY(reg_mat(m, p + "weight", L, N, K, ld));
    return reg_f32(m, p + "bias", &L.b, N);
}

// register the checkpoint tensors p + names[j] + "weight" / "bias" as the row ranges [row0 + j * rows, row0 + (j + 1) * rows) of
// the fused compute-dtype weight and fp32 bias of L
void reg_rows(Captioner* m, const std::string& p, const char* const* names, int n, const Linear& L, int64_t rows, int64_t row0 = 0) {
    for (int j = 0; j < n; ++j) {
        const size_t r = (size_t)(row0 + j * rows);
        add_slot(m, p + names[j] + "weight", (char*)L.w + r * L.K * m->esz, m->gdt, rows, L.K);
        add_slot(m, p + names[j] + "bias", L.b + r, CAP_DT_F32, 1, rows);
    }
}
// allocate a fused weight [total, K] + bias; its row ranges are registered by reg_rows
int alloc_fused(Captioner* m, Linear& L, int64_t total, int K) {
    L.N = (int)total; L.K = L.ld = K;
    TRY(walloc(m, &L.w, (size_t)total * K * m->esz));
    return walloc(m, (void**)&L.b, (size_t)total * 4);
}
// allocate such a fused weight + bias of n parts of `rows` rows and register them (n = 1: one Linear layer)
int reg_fused(Captioner* m, const std::string& p, const char* const* names, int n, Linear& L, int64_t rows, int K) {
    TRY(alloc_fused(m, L, n * rows, K));
    reg_rows(m, p, names, n, L, rows);
    return 0;
}
int reg_ln(Captioner* m, const std::string& p, Norm& n, int64_t D) {
    TRY(reg_f32(m, p + "weight", &n.g, D));
    return reg_f32(m, p + "bias", &n.b, D);
}

// Checkpoint names of a pre-LN transformer tower; every name below ends in the separator before "weight" / "bias".  qkv: one
// fused projection {name}, or {q, k, v} written into the rows of one fused buffer.  Stem names: image towers only (null: absent).
struct TowerNames {
    const char *root, *layers;                            // layer i: root + layers + i + "."
    const char *qkv[3], *proj, *ln1, *fc1, *fc2, *ln2;
    const char *cls, *pos, *patch;                        // (cls / pos: full names)
    bool patch_bias;
    const char *ln_pre, *ln_final;
};
// HF BLIP / BLIP-2 vision model
const TowerNames kBlipVision = {"vision_model.", "encoder.layers.", {"self_attn.qkv."}, "self_attn.projection.", "layer_norm1.",
                                "mlp.fc1.", "mlp.fc2.", "layer_norm2.", "embeddings.class_embedding",
                                "embeddings.position_embedding", "embeddings.patch_embedding.", true, nullptr, "post_layernorm."};
// open_clip CoCa ViT (the final LayerNorm is the attentional pooler's ln_k)
const TowerNames kCocaVision = {"visual.", "transformer.resblocks.", {"attn.in_proj_"}, "attn.out_proj.", "ln_1.", "mlp.c_fc.",
                                "mlp.c_proj.", "ln_2.", "class_embedding", "positional_embedding", "conv1.", false, "ln_pre.",
                                "attn_pool.ln_k."};
// HF CLIPModel towers
const TowerNames kClipVision = {"vision_model.", "encoder.layers.", {"self_attn.q_proj.", "self_attn.k_proj.", "self_attn.v_proj."},
                                "self_attn.out_proj.", "layer_norm1.", "mlp.fc1.", "mlp.fc2.", "layer_norm2.",
                                "embeddings.class_embedding", "embeddings.position_embedding.weight", "embeddings.patch_embedding.",
                                false, "pre_layrnorm.", "post_layernorm."};     // (sic: HF's name)
const TowerNames kClipText = {"text_model.", "encoder.layers.", {"self_attn.q_proj.", "self_attn.k_proj.", "self_attn.v_proj."},
                              "self_attn.out_proj.", "layer_norm1.", "mlp.fc1.", "mlp.fc2.", "layer_norm2.", nullptr, nullptr,
                              nullptr, false, nullptr, "final_layer_norm."};

// an image tower's stem: class row, position table, patch weight [D, Kpad] (+ bias), ln_pre
int reg_stem(Captioner* m, const TowerNames& n) {
    const int D = m->c.v_hidden;
    const std::string r = n.root;
    TRY(reg_f32(m, r + n.cls, &m->cls, D));
    TRY(reg_f32(m, r + n.pos, &m->vpos, (int64_t)m->NT * D));
    if (n.patch_bias) TRY(reg_linear(m, r + n.patch, m->patch, D, m->Kpatch, m->Kpad));
    else TRY(reg_mat(m, r + n.patch + "weight", m->patch, D, m->Kpatch, m->Kpad));
    if (n.ln_pre) TRY(reg_ln(m, r + n.ln_pre, m->ln_pre, D));
    return 0;
}

// the blocks of a pre-LN tower (width D, MLP F) and its final LayerNorm
int reg_tower(Captioner* m, const TowerNames& n, std::vector<VLayer>& layers, int count, int D, int F, Norm& lnf) {
    const int nqkv = n.qkv[1] ? 3 : 1;
    layers.resize(count);
    for (int i = 0; i < count; ++i) {
        VLayer& L = layers[i];
        const std::string p = std::string(n.root) + n.layers + std::to_string(i) + ".";
        TRY(reg_fused(m, p, n.qkv, nqkv, L.qkv, 3 * D / nqkv, D));
        TRY(reg_linear(m, p + n.proj, L.proj, D, D));
        TRY(reg_ln(m, p + n.ln1, L.ln1, D));
        TRY(reg_linear(m, p + n.fc1, L.fc1, F, D));
        TRY(reg_linear(m, p + n.fc2, L.fc2, D, F));
        TRY(reg_ln(m, p + n.ln2, L.ln2, D));
    }
    return reg_ln(m, std::string(n.root) + n.ln_final, lnf, D);
}

// a BERT-style output block into a sub-layer: p + "dense." -> the output projection [N, K], p + "LayerNorm." -> its LayerNorm
int reg_out_ln(Captioner* m, const std::string& p, SubLayer& u, int N, int K) {
    TRY(reg_linear(m, p + "dense.", u.out, N, K));
    return reg_ln(m, p + "LayerNorm.", u.ln, N);
}

// Checkpoint names of a post-LN encoder's layers.  Layer i: layers + i + "."; below it attn holds query. / key. / value. (and
// "cross" + attn the cross-attention's), fc the FFN's first Linear and out its output block.
struct PostNames { const char *layers, *attn, *fc, *out; };
const PostNames kQformerNames = {"qformer.encoder.layer.", "attention.attention.", "intermediate_query.dense.", "output_query."};
const PostNames kBertNames = {"encoder.layer.", "attention.self.", "intermediate.dense.", "output."};

int reg_post_ffn(Captioner* m, const std::string& p, const char* fc, const char* out, SubLayer& u, int W, int F) {
    u.kind = DEC_FFN;
    TRY(reg_linear(m, p + fc, u.in, F, W));
    return reg_out_ln(m, p + out, u, W, F);
}
// `count` post-LN layers of width W, FFN width F.  cross_freq > 0: every cross_freq-th layer cross-attends rows of width D.
// text_ffn: with the text rows' FFN (BERT's own names: `intermediate` / `output`) beside the one n names.
int reg_post_layers(Captioner* m, const PostNames& n, int count, int W, int F, int cross_freq, int D, bool text_ffn) {
    const char* nm[3] = {"query.", "key.", "value."};
    m->pl.resize(count);
    for (int i = 0; i < count; ++i) {
        PostLayer& L = m->pl[i];
        const std::string p = n.layers + std::to_string(i) + ".";
        L.self.kind = DEC_SELF; L.cross.kind = DEC_CROSS;
        TRY(reg_fused(m, p + n.attn, nm, 3, L.self.in, W, W));
        TRY(reg_out_ln(m, p + "attention.output.", L.self, W, W));
        L.has_cross = cross_freq > 0 && i % cross_freq == 0;
        if (L.has_cross) {
            const std::string cp = p + "cross" + n.attn;
            TRY(reg_linear(m, cp + nm[0], L.cross.in, W, W));
            TRY(reg_fused(m, cp, nm + 1, 2, L.ckv, W, D));
            TRY(reg_out_ln(m, p + "crossattention.output.", L.cross, W, W));
        }
        TRY(reg_post_ffn(m, p, n.fc, n.out, L.ffn, W, F));
        if (text_ffn) TRY(reg_post_ffn(m, p, kBertNames.fc, kBertNames.out, L.ffn_text, W, F));
    }
    return 0;
}
int alloc_post_rows(Captioner* m, PostRows& r, size_t R, size_t W, size_t F) {
    const size_t e = m->esz;
    TRY(dev_alloc(m, (void**)&r.x, R * W * 4));
    TRY(dev_alloc(m, (void**)&r.y, R * W * 4));
    TRY(dev_alloc(m, &r.x_t, R * W * e));
    TRY(dev_alloc(m, &r.qkv, R * 3 * W * e));
    TRY(dev_alloc(m, &r.ctx, R * W * e));
    return dev_alloc(m, &r.h, R * F * e);
}

int build_blip(Captioner* m) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, T = c.t_hidden, F = c.t_ffn, V = c.vocab;
    TRY(reg_stem(m, kBlipVision));
    TRY(reg_tower(m, kBlipVision, m->vl, c.v_layers, D, c.v_mlp, m->post));

    DecPlan& P = m->dec;
    P.W = T; P.skip_finished = true; P.kv_tokens = P.kv_keys = m->NT; P.tags = &kBlipDecTags;
    const std::string tb = "text_decoder.bert.";
    // the embedding table is read twice: fp32 rows for the lookup, compute-dtype [V,T] as the (tied) LM-head weight
    TRY(walloc(m, (void**)&m->word_f32, (size_t)V * T * 4));
    add_slot(m, tb + "embeddings.word_embeddings.weight", m->word_f32, CAP_DT_F32, V, T);
    if (m->gdt == CAP_DT_F32) {
        P.vocab = linear_over(m->word_f32, V, T);
    } else {
        TRY(reg_mat(m, tb + "embeddings.word_embeddings.weight", P.vocab, V, T));
    }
    TRY(reg_f32(m, tb + "embeddings.position_embeddings.weight", &m->tpos, (int64_t)c.max_pos * T));
    TRY(reg_ln(m, tb + "embeddings.LayerNorm.", P.emb, T));
    P.word = m->word_f32; P.pos = m->tpos;
    // cross-attention K/V projections of all layers fused into one [L*2*T, D] weight (one GEMM per image batch)
    TRY(alloc_fused(m, m->ckv, (int64_t)c.t_layers * 2 * T, D));
    P.subs.resize(3 * c.t_layers);
    const char* nm[3] = {"query.", "key.", "value."};
    for (int i = 0; i < c.t_layers; ++i) {
        SubLayer &sa = P.subs[3 * i], &ca = P.subs[3 * i + 1], &ff = P.subs[3 * i + 2];
        sa.kind = DEC_SELF; ca.kind = DEC_CROSS; ca.slot = i; ff.kind = DEC_FFN;
        const std::string p = tb + "encoder.layer." + std::to_string(i) + ".";
        TRY(reg_fused(m, p + "attention.self.", nm, 3, sa.in, T, T));
        TRY(reg_out_ln(m, p + "attention.output.", sa, T, T));
        TRY(reg_linear(m, p + "crossattention.self.query.", ca.in, T, T));
        reg_rows(m, p + "crossattention.self.", nm + 1, 2, m->ckv, T, (int64_t)i * 2 * T);
        TRY(reg_out_ln(m, p + "crossattention.output.", ca, T, T));
        TRY(reg_linear(m, p + "intermediate.dense.", ff.in, F, T));
        TRY(reg_out_ln(m, p + "output.", ff, T, F));
    }
    const std::string cp = "text_decoder.cls.predictions.";
    TRY(reg_linear(m, cp + "transform.dense.", P.tr, T, T));
    TRY(reg_ln(m, cp + "transform.LayerNorm.", P.tr_ln, T));
    return reg_f32(m, cp + "bias", &P.vocab.b, V);
}

// One CoCa text block = an attention sub-layer (causal self-attention, or cross-attention over cache slot `slot` >= 0) and an FFN
// sub-layer.  Pre-LN: the block's ln_1 is the LayerNorm of whatever comes BEFORE it (ln1: the previous FFN sub-layer's, the
// embedding's for the first block), its ln_2 the attention sub-layer's; the FFN sub-layer's is left to the next block.
int reg_block(Captioner* m, const std::string& p, SubLayer& at, SubLayer& ff, Norm& ln1, int E, int F, int slot) {
    at.kind = slot < 0 ? DEC_SELF : DEC_CROSS; at.slot = slot; ff.kind = DEC_FFN;
    TRY(reg_ln(m, p + ".ln_1.", ln1, E));
    if (slot < 0) TRY(reg_linear(m, p + ".attn.in_proj_", at.in, 3 * E, E));
    else TRY(reg_linear(m, "derived.cross_q." + std::to_string(slot) + ".", at.in, E, E));
    TRY(reg_linear(m, p + ".attn.out_proj.", at.out, E, E));
    TRY(reg_ln(m, p + ".ln_2.", at.ln, E));
    TRY(reg_linear(m, p + ".mlp.c_fc.", ff.in, F, E));
    return reg_linear(m, p + ".mlp.c_proj.", ff.out, E, F);
}

// open_clip CoCa state-dict names (SURVEY.md section 5 "Checkpoint / resume"); `derived.*` tensors are computed once by
// the host loader (embodied_captioning_amd/coca_weights.py) from the checkpoint.
int build_coca(Captioner* m) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, E = c.embed_dim, F = c.t_ffn, V = c.vocab, Q = c.pool_queries;
    m->Q = Q; m->E = E;
    TRY(reg_stem(m, kCocaVision));
    TRY(reg_tower(m, kCocaVision, m->vl, c.v_layers, D, c.v_mlp, m->post));
    TRY(reg_f32(m, "derived.pool_q", &m->pool_q, (int64_t)Q * E));
    TRY(reg_linear(m, "derived.pool_kv.", m->pool_kv, 2 * E, D));
    TRY(reg_linear(m, "visual.attn_pool.attn.out_proj.", m->pool_out, E, E));
    TRY(reg_ln(m, "visual.ln_post.", m->lnpost, E));
    DecPlan& P = m->dec;
    P.W = E; P.pre_ln = true; P.kv_tokens = Q; P.kv_first = 1; P.kv_keys = Q - 1; P.tags = &kCocaDecTags;
    TRY(reg_f32(m, "text.token_embedding.weight", &P.word, (int64_t)V * E));
    TRY(reg_f32(m, "text.positional_embedding", &m->tpos, (int64_t)c.max_pos * E));
    P.pos = m->tpos;
    // unimodal blocks, then per multimodal layer i a self block and the cross block over slot i
    P.subs.resize(2 * (c.t_layers + 2 * c.mm_layers));
    int n = 0;
    Norm* ln1 = &P.emb;                            // where the next block's ln_1 goes
    auto block = [&](const std::string& p, int slot) {
        SubLayer &at = P.subs[n], &ff = P.subs[n + 1];
        n += 2;
        const int rc = reg_block(m, p, at, ff, *ln1, E, F, slot);
        ln1 = &ff.ln;
        return rc;
    };
    for (int i = 0; i < c.t_layers; ++i) TRY(block("text.transformer.resblocks." + std::to_string(i), -1));
    for (int i = 0; i < c.mm_layers; ++i) {
        TRY(block("text_decoder.resblocks." + std::to_string(i), -1));
        TRY(block("text_decoder.cross_attn." + std::to_string(i), i));
    }
    TRY(reg_linear(m, "derived.cross_kv.", m->ckv, c.mm_layers * 2 * E, E));
    TRY(reg_ln(m, "text_decoder.ln_final.", *ln1, E));
    TRY(reg_mat(m, "derived.vocab.weight", P.vocab, V, E));
    // constant vectors for the affine-free LayerNorm that feeds the folded cross-K/V projection
    TRY(walloc(m, (void**)&m->ones, (size_t)E * 4));
    TRY(walloc(m, (void**)&m->zeros, (size_t)E * 4));
    if (!m->replay) {
        TRY(launch_fill_f32(m->ones, 1.0f, E, nullptr));
        TRY(launch_fill_f32(m->zeros, 0.0f, E, nullptr));
        CAP_HIP_CHECK(hipDeviceSynchronize());
    }
    return 0;
}

// the activations of a tower of width D and MLP F over M rows
int alloc_tower(Captioner* m, Tower& t, size_t M, size_t D, size_t F) {
    TRY(dev_alloc(m, (void**)&t.X, M * D * 4));
    if (!vit_adds_in_place(m->gdt)) TRY(dev_alloc(m, (void**)&t.delta, M * D * 4));
    TRY(dev_alloc(m, &t.ln, M * D * m->esz));
    TRY(dev_alloc(m, &t.qkv, M * 3 * D * m->esz));   // (split mode: fp32 q|k|v where the attention cannot take G8 - esz is 4 there)
    TRY(dev_alloc(m, &t.ctx, M * D * m->esz));
    return dev_alloc(m, &t.mlp, M * F * m->esz);
}
// the image tower's: patch rows (zero padding columns up to Kpad) and its activations over max_batch images
int alloc_image_tower(Captioner* m) {
    const size_t Bm = m->c.max_batch, bytes = Bm * m->P * m->Kpad * m->esz;
    TRY(dev_alloc(m, &m->patches, bytes, ARENA_KEPT, "patches"));
    CAP_HIP_CHECK(hipMemset(m->patches, 0, bytes));
    return alloc_tower(m, m->vt, Bm * m->NT, m->c.v_hidden, m->c.v_mlp);
}

// bytes of one slot of the decoder's cross K/V cache for B images: [k|v][image][head][kv_tokens][64]
size_t cross_slot_bytes(const Captioner* m, size_t B) { return 2 * m->cross_block(B * m->c.t_heads * m->dec.kv_tokens); }

int build_arena_coca(Captioner* m) {
    const CapConfig& c = m->c;
    const size_t Bm = c.max_batch, NT = m->NT, D = c.v_hidden, E = c.embed_dim, e = m->esz, Q = c.pool_queries;
    const size_t M = Bm * NT, R = Bm * c.max_beams, Lm = c.max_len, H = c.t_heads;     // R: decode rows (image x beam)
    TRY(alloc_image_tower(m));
    TRY(dev_alloc(m, (void**)&m->emb_f, 256));
    TRY(dev_alloc(m, &m->emb_t, M * D * e));
    TRY(dev_alloc(m, &m->pool_kvbuf, M * 2 * E * e));
    TRY(dev_alloc(m, &m->pool_ctx, Bm * Q * E * e));
    TRY(dev_alloc(m, (void**)&m->pool_o, Bm * Q * E * 4));
    TRY(dev_alloc(m, (void**)&m->img_tokens, Bm * Q * E * 4));
    TRY(dev_alloc(m, &m->xhat, Bm * Q * E * e));
    TRY(dev_alloc(m, &m->cross, (size_t)c.mm_layers * cross_slot_bytes(m, Bm)));
    TRY(dev_alloc(m, (void**)&m->seq, R * Lm * 4, ARENA_INDEX, "seq"));
    TRY(dev_alloc(m, (void**)&m->finished, R * 4, ARENA_INDEX, "finished"));
    TRY(dev_alloc(m, (void**)&m->lens, R * 4, ARENA_INDEX, "lens"));
    TRY(dev_alloc(m, (void**)&m->anc, 2 * R * Lm * 4 + 256, ARENA_INDEX, "anc"));    // beam ancestry of the self-attention caches (beam.hip)
    TRY(dev_alloc(m, (void**)&m->dx, R * E * 4));
    TRY(dev_alloc(m, (void**)&m->dy, R * E * 4));
    TRY(dev_alloc(m, (void**)&m->dx2, (size_t)(R > SMALL_MAX_ROWS ? R : SMALL_MAX_ROWS) * E * 4));
    TRY(dev_alloc(m, (void**)&m->dpart, 12 * R * E * 4));
    TRY(dev_alloc(m, &m->dx_t, R * E * e));
    TRY(dev_alloc(m, &m->dq, R * E * e));
    TRY(dev_alloc(m, &m->dctx, R * E * e));
    TRY(dev_alloc(m, &m->dh, R * c.t_ffn * e));
    m->ldl = (c.vocab + 3) & ~3;
    TRY(dev_alloc(m, (void**)&m->logits, R * (size_t)m->ldl * 4));
    for (SubLayer& u : m->dec.subs)
        if (u.kind == DEC_SELF) TRY(dev_alloc(m, &u.cache, 2 * R * H * Lm * 64 * e));
    TRY(dev_alloc(m, &m->beam, beam_state_bytes((int)Bm, c.max_beams, (int)Lm), ARENA_INDEX, "beam"));      // (a 1-beam search exists: beam groups)
    return 0;
}

int build_arena(Captioner* m) {
    const CapConfig& c = m->c;
    const size_t Bm = c.max_batch, NT = m->NT, D = c.v_hidden, T = c.t_hidden, e = m->esz;
    const size_t M = Bm * NT, R = Bm * c.max_beams, Lm = c.max_len, H = c.t_heads;
    TRY(alloc_image_tower(m));
    TRY(dev_alloc(m, (void**)&m->emb_f, M * D * 4));
    TRY(dev_alloc(m, &m->emb_t, M * D * e));
    TRY(dev_alloc(m, &m->cross, (size_t)c.t_layers * cross_slot_bytes(m, Bm)));
    TRY(dev_alloc(m, (void**)&m->seq, R * Lm * 4, ARENA_INDEX, "seq"));
    TRY(dev_alloc(m, (void**)&m->finished, R * 4, ARENA_INDEX, "finished"));
    TRY(dev_alloc(m, (void**)&m->lens, R * 4, ARENA_INDEX, "lens"));
    TRY(dev_alloc(m, (void**)&m->live, R * 4, ARENA_INDEX, "live"));
    TRY(dev_alloc(m, (void**)&m->n_live, 256, ARENA_INDEX, "n_live"));
    TRY(dev_alloc(m, (void**)&m->anc, 2 * R * Lm * 4, ARENA_INDEX, "anc"));
    // prompt prefill (run_prefill): max_prompt - 1 known positions of every caption go through the decoder as ONE pass of rows, so
    // the buffers a pass over rows touches hold that many (CapConfig.max_prompt = 0: exactly the decode rows, as ever)
    // teacher-forced scoring (run_score): max_score_rows rows of a pass AND of its head (0: nothing beyond the above)
    const size_t Rs = (size_t)std::max(c.max_score_rows, 0), Rh = std::max(R, Rs);
    const size_t Rw = std::max(std::max(R, Bm * (size_t)std::max(c.max_prompt - 1, 0)), Rs);
    m->ws_rows = Rw;
    m->head_rows = Rh;
    TRY(dev_alloc(m, (void**)&m->dx, Rw * T * 4));
    TRY(dev_alloc(m, (void**)&m->dy, Rh * T * 4));
    TRY(dev_alloc(m, (void**)&m->dx2, (size_t)(R > SMALL_MAX_ROWS ? R : SMALL_MAX_ROWS) * T * 4));
    TRY(dev_alloc(m, (void**)&m->dpart, 12 * Rw * T * 4));      // split-K slabs: 8 x [R,T] (ffn) or 4 x [R,3T] (qkv)
    TRY(dev_alloc(m, &m->dx_t, Rw * T * e));
    TRY(dev_alloc(m, &m->dq, R * T * e));
    TRY(dev_alloc(m, &m->dctx, Rw * T * e));
    TRY(dev_alloc(m, &m->dh, Rw * c.t_ffn * e));
    m->ldl = (c.vocab + 3) & ~3;
    TRY(dev_alloc(m, (void**)&m->logits, Rh * (size_t)m->ldl * 4));
    for (SubLayer& u : m->dec.subs)
        if (u.kind == DEC_SELF) TRY(dev_alloc(m, &u.cache, 2 * R * H * Lm * 64 * e));
    TRY(dev_alloc(m, &m->beam, beam_state_bytes((int)Bm, c.max_beams, (int)Lm), ARENA_INDEX, "beam"));
    return 0;
}

// ---------------------------------------------------------------------------------------------- profiling
struct ProfScope {
    Captioner* m; hipStream_t s; int idx = -1;
    ProfScope(Captioner* m_, hipStream_t s_, const char* tag, double flops, double bytes) : m(m_), s(s_) {
        if (!m->prof || !tag) return;     // (a null tag: the caller's pass does not record this launch)
        ProfTag t; t.tag = tag; t.flops = flops; t.bytes = bytes;
        if (hipEventCreate(&t.e0) != hipSuccess || hipEventCreate(&t.e1) != hipSuccess) return;
        (void)hipEventRecord(t.e0, s);
        m->prof_recs.push_back(t);
        idx = (int)m->prof_recs.size() - 1;
    }
    ~ProfScope() { if (idx >= 0) (void)hipEventRecord(m->prof_recs[idx].e1, s); }
};

// ---------------------------------------------------------------------------------------------- GEMM calls
// A GEMM's profile record: 2 M N K flops (+ a fused attention's), one read of the operand and the weight, and out_bytes per output
// element - a store its element (+ 4 with a residual read), a split-K GEMM 4 for each of its S slabs
struct GemmScope : ProfScope {
    GemmScope(Captioner* m, hipStream_t s, const char* tag, double M, double N, double K, double out_bytes, double more_flops = 0)
        : ProfScope(m, s, tag, 2.0 * M * N * K + more_flops, (M * K + N * K) * m->esz + M * N * out_bytes) {}
};
// The one place a GemmParams is filled: operand, weight, bias, output, shape, activation and epilogue; everything else zero
// (the callers set the extras they have by name)
GemmParams gemm_params(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N, int K,
                       int act, int out_f32, int epi = EPI_STORE, int splitk = 1) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.bias = bias; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
    p.gelu = act; p.out_f32 = out_f32; p.epi = epi; p.splitk = splitk;
    return p;
}
int run_gemm(Captioner* m, hipStream_t s, const char* tag, const GemmParams& p, int tile) {
    GemmScope ps(m, s, tag, p.M, p.N, p.K, p.epi == EPI_PARTIAL ? 4.0 * p.splitk : (p.out_f32 ? 4.0 : (double)m->esz) + (p.resid ? 4.0 : 0.0));
    return launch_gemm(m->gdt, p, tile, s);
}

// The rare extras of a gemm() call, by name
struct GemmOpt {
    const float* resid = nullptr;                          // fp32 [M, N] in C's layout, may alias C
    int epi = EPI_STORE, p0 = 0, p1 = 0, p2 = 0, p3 = 0;   // another epilogue with what it reads (gemm.h), aux and C2 too
    const float* aux = nullptr; void* C2 = nullptr;
    const int* m_live = nullptr;                           // the compacted greedy loop's count of live rows (GemmParams::m_live)
    int tile = 0;                                          // 0 = auto (the stream kernel for encoder-sized problems without residual)
    static GemmOpt residual(const float* r) { GemmOpt o; o.resid = r; return o; }
    static GemmOpt live(const int* n) { GemmOpt o; o.m_live = n; return o; }
};
// C [M, L.N] (rows ldc apart, fp32 or the operand type) = act(A [M, L.K] (rows lda apart) . L.w^T + L.b)
int gemm(Captioner* m, hipStream_t s, const char* tag, const void* A, int lda, const Linear& L, void* C, int ldc, OutType out, int M,
         GemmAct act = ACT_NONE, const GemmOpt& o = GemmOpt()) {
    GemmParams p = gemm_params(A, lda, L.w, L.ld, L.b, C, ldc, M, L.N, L.K, act, out, o.epi);
    p.resid = o.resid; p.ldr = ldc;
    p.p0 = o.p0; p.p1 = o.p1; p.p2 = o.p2; p.p3 = o.p3; p.aux = o.aux; p.C2 = o.C2;
    p.kv16 = o.epi == EPI_CROSSKV && m->kv16 ? 1 : 0;
    p.m_live = o.m_live;
    return run_gemm(m, s, tag, p, o.tile);
}

// Decode loops stop when every caption is finished, as HF generate does (`unfinished_sequences.max() == 0` /
// `is_done.all()`); the remaining steps would only write pad.  The device keeps the state, the host looks at it every
// `poll` steps: one tiny kernel writes the number of open rows (greedy) or the beam loop's active flag to a host-mapped
// word, then the stream is synchronised.  Off by default (poll = 0): the loop is then free of host synchronisation and
// can be captured in a graph.
__global__ void poll_open_kernel(const int* __restrict__ finished, int R, const int* __restrict__ beam_active, int* host_out) {
    if (beam_active) { if (threadIdx.x == 0) *host_out = *beam_active; return; }
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int c = 0;
    for (int r = threadIdx.x; r < R; r += blockDim.x) c += finished[r] == 0;
    if (c) atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) *host_out = cnt;
}
// true = every row is finished (the caller leaves its loop).  step = index of the step just completed, steps = loop length.
int poll_all_finished(Captioner* m, int step, int steps, const int* finished, int R, const int* beam_active, hipStream_t s, bool* done) {
    *done = false;
    if (m->poll <= 0 || !m->host_flag || (step + 1) % m->poll != 0 || step + 2 >= steps) return 0;
    hipLaunchKernelGGL(poll_open_kernel, dim3(1), dim3(256), 0, s, finished, R, beam_active, m->host_flag_dev);
    CAP_HIP_CHECK(hipGetLastError());
    CAP_HIP_CHECK(hipStreamSynchronize(s));
    *done = *(volatile int*)m->host_flag == 0;
    return 0;
}

// ---------------------------------------------------------------------------------------------- a request's per-step outputs
// Both decode loops (run_generate, run_generate_blip2) write a request's optional outputs through these.  R = rows of the loop,
// cols = steps a caption can take (max_len - 1 for BLIP / CoCa, max_len for BLIP-2), step = index among them.
__global__ void copy_logits_kernel(const float* src, int ld, float* dst, int R, int V) {
    const size_t n = (size_t)R * V;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / V, c = i - r * V;
        dst[i] = src[r * ld + c];
    }
}
// out_logprobs [R, cols] / out_scored [R] / out_vocab [R, acc_ld] start from zero, on the caller's stream: the selection kernel
// writes the open captions' entries only, indexed by the caption's row whatever the loop's compaction
int zero_greedy_outputs(const CapGenerateArgs& a, int R, int cols, hipStream_t s) {
    if (a.out_logprobs) {
        TRY(launch_fill_f32(a.out_logprobs, 0.f, (size_t)R * cols, s));
        TRY(launch_fill_i32(a.out_scored, 0, (size_t)R, s));
    }
    if (a.out_vocab) TRY(launch_fill_f32(a.out_vocab, 0.f, (size_t)R * a.acc_ld, s));
    return 0;
}
int copy_step_logits(Captioner* m, const CapGenerateArgs& a, int R, int step, hipStream_t s) {
    if (!a.out_step_logits) return 0;
    hipLaunchKernelGGL(copy_logits_kernel, dim3(1024), dim3(256), 0, s, m->logits, m->ldl,
                       a.out_step_logits + (size_t)step * R * m->c.vocab, R, m->c.vocab);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}
// The token of position t + 1 of every open caption (a row ends on EOS or at `end` tokens; CoCa: MinLength mask and forced EOS), with
// the request's log-prob / vocabulary outputs taken by the same kernel.
int select_greedy_step(Captioner* m, const CapGenerateArgs& a, int R, int step, int cols, int seq_ld, int t, int end, RowMap map,
                       hipStream_t s) {
    const CapConfig& c = m->c;
    const bool coca = c.arch == CAP_ARCH_COCA;
    SelectStep st{};
    st.logits = m->logits; st.ld = m->ldl; st.V = c.vocab;
    st.seq = m->seq; st.seq_ld = seq_ld; st.t = t; st.max_len = end; st.eos = c.eos; st.pad = c.pad;
    st.finished = m->finished; st.out_len = m->lens; st.R = R; st.map = map;
    st.min_len = coca ? c.min_len : 0; st.force_eos = coca ? 1 : 0;
    // a ban in force (cap_set_bad_words) works over the context HF's processor sees - BLIP's row from its BOS column on; BLIP-2's BOS
    // and generated tokens: the generated columns and the one before them, which stands for BOS (it holds pad, and neither id is in
    // any sequence).  The repetition controls (cap_set_repeat_controls) put BLIP-2's image placeholders and BOS in front of the same
    // columns (ops.h, RepeatCtl).
    st.hist0 = c.arch == CAP_ARCH_BLIP2 ? c.num_query_tokens : 0;
    if (m->banned()) st.ban = m->ban_set();
    st.ctl = m->repeat_ctl();
    // sampling (cap_set_sampling): `step` is the draw's counter word and the call's sample keys (cap_generate_sampled; null: the row
    // index) name the captions
    if (m->sampling) { st.sample = 1; st.sc = m->sample_ctl; st.keys = m->call_keys; st.draw = step; }
    // validate_generate refused these outputs, and CoCa, beside any of the three; with nothing set this is the plain launch
    st.logprobs = a.out_logprobs; st.lp_ld = cols; st.lp_col = step; st.scored = a.out_scored;
    st.vocab_acc = a.out_vocab; st.acc_ld = a.acc_ld;
    return launch_select_step(st, s);
}

// One beam step over logits [B * K, ldl] with L token columns (the ancestry table's row length too) and whatever ban set and
// repetition controls are in force (never CoCa: validate_generate); CoCa: raw-logit scores and the MinLength mask.
int engine_beam_step(Captioner* m, const CapGenerateArgs& a, void* state, const float* logits, int* anc, int B, int K, int L, int cur_len,
                     hipStream_t s) {
    const CapConfig& c = m->c;
    const bool coca = c.arch == CAP_ARCH_COCA;
    BeamStep st{};
    st.state = state; st.logits = logits; st.ld = m->ldl; st.V = c.vocab; st.B = B; st.K = K; st.max_len = L; st.cur_len = cur_len;
    st.eos = c.eos; st.length_penalty = a.length_penalty; st.anc = anc; st.anc_ld = L;
    st.mode = coca ? BEAM_LEGACY_RAW : BEAM_HF_V5; st.min_len = coca ? c.min_len : 0;
    if (m->banned()) st.ban = m->ban_set();
    st.ctl = m->repeat_ctl();
    return launch_beam_step(st, s);
}

// ---------------------------------------------------------------------------------------------- BLIP-2 OPT
// (the builder; the OPT decoder and the runs sit behind the decoder sections they call, ahead of the C ABI)
__global__ void copy_new_tokens_kernel(const int* seq, int seq_ld, int P, const int* lens, int* out_ids, int* out_len, int B, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * n; i += gridDim.x * blockDim.x) out_ids[i] = seq[(size_t)(i / n) * seq_ld + P + i % n];
    if (out_len)
        for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) out_len[b] = min(lens[b] - P, n);
}
// The Q-Former: `derived.qformer_x0` = qformer.layernorm(query_tokens), computed once by the host loader (a constant of the
// checkpoint), and the layers - text_ffn: with the text rows' FFN (`intermediate` / `output`) beside the query rows' (the
// image-text scorer; `use_qformer_text_input` checkpoints).
int reg_qformer(Captioner* m, bool text_ffn) {
    const CapConfig& c = m->c;
    TRY(reg_f32(m, "derived.qformer_x0", &m->q_x0, (int64_t)c.num_query_tokens * c.q_hidden));
    return reg_post_layers(m, kQformerNames, c.q_layers, c.q_hidden, c.q_ffn, c.q_cross_freq, c.v_hidden, text_ffn);
}

// HF `Blip2ForConditionalGeneration` state-dict names (transformers 5.x).
int build_blip2(Captioner* m) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, Q = c.q_hidden, F = c.q_ffn, T = c.t_hidden, G = c.t_ffn, V = c.vocab, nq = c.num_query_tokens;
    TRY(reg_stem(m, kBlipVision));
    TRY(reg_tower(m, kBlipVision, m->vl, c.v_layers, D, c.v_mlp, m->post));

    TRY(reg_qformer(m, false));
    TRY(reg_linear(m, "language_projection.", m->lproj, T, Q));

    const std::string lm = "language_model.model.decoder.";
    // token table twice: fp32 rows for the lookup, compute dtype as the tied LM head
    TRY(walloc(m, (void**)&m->o_tok, (size_t)V * T * 4));
    add_slot(m, lm + "embed_tokens.weight", m->o_tok, CAP_DT_F32, V, T);
    if (m->gdt == CAP_DT_F32) m->o_head = linear_over(m->o_tok, V, T);
    else TRY(reg_mat(m, lm + "embed_tokens.weight", m->o_head, V, T));
    TRY(reg_f32(m, lm + "embed_positions.weight", &m->o_pos, (int64_t)(c.max_pos + 2) * T));
    // Rm: the decode step's rows (image x beam); the prompt pass runs over the Bm images whatever the beam count
    const size_t Bm = c.max_batch, Rm = Bm * c.max_beams, Lmax = nq + 1 + c.max_len;
    m->ol.resize(c.t_layers);
    const char* pn[3] = {"q_proj", "k_proj", "v_proj"};
    // a decoder projection: in the operand type, or with CapConfig.weight_int8 int8 + row scales
    auto linear = [&](const std::string& q, Linear& L, int N, int K) {
        if (!m->wq8) return reg_linear(m, q, L, N, K);
        TRY(reg_mat_i8(m, q + "weight", L, N, K));
        return reg_f32(m, q + "bias", &L.b, N);
    };
    for (int i = 0; i < c.t_layers; ++i) {
        OLayer& L = m->ol[i];
        const std::string p = lm + "layers." + std::to_string(i) + ".";
        Linear& q = L.qkv;
        q.N = 3 * T; q.K = q.ld = T;
        TRY(walloc(m, &q.w, (size_t)3 * T * T * (m->wq8 ? 1 : m->esz)));
        if (m->wq8) TRY(walloc(m, (void**)&q.scale, (size_t)3 * T * 4));
        TRY(walloc(m, (void**)&q.b, (size_t)3 * T * 4));
        for (int j = 0; j < 3; ++j) {
            // (int8: a 16-row tile's blocks are contiguous, so rows j T .. of the fused matrix start at byte j T T)
            if (m->wq8) add_slot(m, p + "self_attn." + pn[j] + ".weight", (char*)q.w + (size_t)j * T * T, CAP_DT_I8W, T, T, 0, q.scale + (size_t)j * T);
            else add_slot(m, p + "self_attn." + pn[j] + ".weight", (char*)q.w + (size_t)j * T * T * m->esz, m->gdt, T, T);
            add_slot(m, p + "self_attn." + pn[j] + ".bias", q.b + (size_t)j * T, CAP_DT_F32, 1, T);
        }
        TRY(linear(p + "self_attn.out_proj.", L.o, T, T));
        TRY(reg_ln(m, p + "self_attn_layer_norm.", L.ln1, T));
        TRY(linear(p + "fc1.", L.f1, G, T));
        TRY(linear(p + "fc2.", L.f2, T, G));
        TRY(reg_ln(m, p + "final_layer_norm.", L.ln2, T));
        TRY(dev_alloc(m, &L.kc, Rm * Lmax * T * m->esz));
        TRY(dev_alloc(m, &L.vc, Rm * Lmax * T * m->esz));
    }
    TRY(reg_ln(m, lm + "final_layer_norm.", m->o_lnf, T));

    // arena
    const size_t NT = m->NT, M = Bm * NT, e = m->esz, P = nq + 1;
    const size_t Ro = std::max(Bm * P, Rm);             // rows of the buffers the prompt pass and the step share
    TRY(alloc_image_tower(m));
    TRY(dev_alloc(m, (void**)&m->emb_f, M * D * 4));
    TRY(dev_alloc(m, &m->emb_t, M * D * e));
    TRY(alloc_post_rows(m, m->qr, Bm * nq, Q, F));
    TRY(dev_alloc(m, &m->qkvimg, M * 2 * Q * e));
    TRY(dev_alloc(m, (void**)&m->lm_proj, Bm * nq * T * 4));
    TRY(dev_alloc(m, (void**)&m->ox, Ro * T * 4));
    TRY(dev_alloc(m, &m->oh_t, Ro * T * e));
    TRY(dev_alloc(m, &m->oqkv, Ro * 3 * T * e));
    TRY(dev_alloc(m, &m->octx, Ro * T * e));
    TRY(dev_alloc(m, &m->off, Ro * G * e));
    {
        size_t dpart_bytes = (size_t)8 * Rm * std::max(3 * T, G) * 4;                     // split-K slabs of the decode-step GEMMs
        if (m->wq8) {                                   // int8 weights: the prompt pass runs the same chain over Bm * P rows
            const size_t Sm = (size_t)std::max(skinny_i8_plan(T, T, false), skinny_i8_plan(T, G, false));
            dpart_bytes = std::max(dpart_bytes, Sm * std::min<size_t>(Bm, kI8SkinnyPromptCrops) * P * T * 4);
            if (Bm > (size_t)kI8SkinnyPromptCrops) {    // larger batches: the tiled GEMM's fp32 output [Bm * P, N] + the bf16 scratch
                dpart_bytes = std::max(dpart_bytes, Bm * P * (size_t)std::max(3 * T, G) * 4);
                TRY(dev_alloc(m, &m->w8_scratch, (size_t)std::max(3 * T, G) * T * 2));
            }
        }
        TRY(dev_alloc(m, (void**)&m->dpart, dpart_bytes));
    }
    TRY(dev_alloc(m, (void**)&m->seq, Bm * Lmax * 4, ARENA_INDEX, "seq"));
    TRY(dev_alloc(m, (void**)&m->finished, Bm * 4, ARENA_INDEX, "finished"));
    TRY(dev_alloc(m, (void**)&m->lens, Bm * 4, ARENA_INDEX, "lens"));
    m->ldl = (V + 3) & ~3;
    TRY(dev_alloc(m, (void**)&m->logits, Rm * (size_t)m->ldl * 4));
    if (c.max_beams > 1) {      // beam search (beam.hip): BOS + max_len token columns per row
        TRY(dev_alloc(m, (void**)&m->anc, 2 * Rm * (c.max_len + 1) * 4, ARENA_INDEX, "anc"));
        TRY(dev_alloc(m, &m->beam, beam_state_bytes((int)Bm, c.max_beams, c.max_len + 1), ARENA_INDEX, "beam"));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- post-LN encoders
// The pieces of a post-LN layer over the R rows of one row set r.  Every launch takes m->gdt as its type selector; the sentence
// encoder's kernels are m->dt kernels, the same thing there: cap_create refuses CAP_F32_SPLIT for CAP_ARCH_MINILM.
int post_qkv(Captioner* m, hipStream_t s, const PostTags& tg, const SubLayer& u, const PostRows& r, int R, const PostDims& d) {
    return gemm(m, s, tg.qkv, r.x_t, d.W, u.in, r.qkv, 3 * d.W, m->attn_out(), R);
}
// the tail of a sub-layer: y = A W_out^T + b_out + x; x, x_t = LayerNorm(y)
int post_out_ln(Captioner* m, hipStream_t s, const char* tag, const char* ln_tag, const void* A, const SubLayer& u, const PostRows& r,
                int R, const PostDims& d) {
    TRY(gemm(m, s, tag, A, u.out.K, u.out, r.y, d.W, OUT_F32, R, ACT_NONE, GemmOpt::residual(r.x)));
    ProfScope ps(m, s, ln_tag, 0, (double)R * d.W * (8 + m->esz));
    return launch_layernorm(m->gdt, r.y, d.W, u.ln.g, u.ln.b, d.eps, r.x_t, r.x, R, d.W, s);
}
int post_ffn(Captioner* m, hipStream_t s, const PostTags& tg, const SubLayer& u, const PostRows& r, int R, const PostDims& d) {
    TRY(gemm(m, s, tg.f1, r.x_t, d.W, u.in, r.h, d.F, OUT_T, R, ACT_GELU));
    return post_out_ln(m, s, tg.f2, tg.ln, r.h, u, r, R, d);
}

// the image-text scorer's resident cross K/V of the slot-th cross layer: [max_batch * NT, 2 Q]
char* itm_ckv_slot(const Captioner* m, size_t slot) {
    return (char*)m->itm_ckv + slot * (size_t)m->c.max_batch * m->NT * 2 * m->c.q_hidden * m->esz;
}

// What differs between the Q-Former's two uses: the tags of the query rows' and the text rows' launches, the self-attention
// (queries alone on the generic kernel, or [queries | the pair's text] with the text's key count), and where the image's cross
// K/V come from (projected in the loop into qkvimg, or resident in itm_ckv since cap_blip2_itm_encode_images).
struct QformerPass { const PostTags *qt, *tt; bool pair_attn, resident_kv; };
const QformerPass kCaptionPass = {&kQformerTags, nullptr, false, false};
const QformerPass kScorerPass = {&kItmQueryTags, &kItmTextTags, true, true};

// The Q-Former over B images / pairs with nq query rows (0: none - the ITC text pass) and L text rows (0: none - captioning, the
// ITC image pass) each: self-attention, cross-attention of the query rows to the image's K/V (emb_t [B * NT, D] projected, or
// cached) on the cross layers, the query rows through intermediate_query / output_query and the text rows through intermediate /
// output.  The two kinds of rows live in their own row sets (qr, tr), so every GEMM runs over contiguous rows.  Leaves the last
// hidden states in qr.x / qr.x_t [B * nq, Q] and tr.x [B * L, Q].
int run_qformer(Captioner* m, const QformerPass& ps, int B, int nq, int L, const int* ids, const int* lens, hipStream_t s) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, Q = c.q_hidden, H = c.q_heads, NT = m->NT, Rq = B * nq, Rt = B * L, hd = Q / H;
    const size_t e = m->esz;
    const PostDims d = {Q, c.q_ffn, c.q_eps};
    const PostRows &q = m->qr, &t = m->tr;
    if (nq) TRY(launch_rows_broadcast(m->gdt, m->q_x0, q.x, q.x_t, B, nq, Q, s));
    if (L) {
        ProfScope p(m, s, "itm_embed_text", 0, (double)Rt * Q * (8 + 4 + e));
        TRY(launch_itm_embed_text(m->gdt, ids, L, m->i_word, m->i_pos, m->i_ln.g, m->i_ln.b, c.q_eps, t.x, t.x_t, Rt, Q, c.vocab, s));
    }
    size_t slot = 0;
    for (const PostLayer& Ly : m->pl) {
        if (nq) TRY(post_qkv(m, s, *ps.qt, Ly.self, q, Rq, d));
        if (L) TRY(post_qkv(m, s, *ps.tt, Ly.self, t, Rt, d));
        {
            ProfScope p(m, s, ps.qt->self_attn, 4.0 * B * H * (double)(nq + L) * (nq + L) * hd, (double)(Rq + Rt) * 4 * Q * e);
            const char* base = (const char*)q.qkv;
            if (ps.pair_attn)
                TRY(launch_itm_self_attention(m->dt, q.qkv, t.qkv, lens, q.ctx, t.ctx, B, nq, L, H, hd, s, m->gdt));
            else
                TRY(launch_generic_attention(m->dt, base, 3 * Q, (long)nq * 3 * Q, base + Q * e, 3 * Q, (long)nq * 3 * Q, base + 2 * Q * e,
                                             3 * Q, (long)nq * 3 * Q, q.ctx, Q, (long)nq * Q, B, nq, nq, H, hd, -1, s, m->gdt));
        }
        if (nq) TRY(post_out_ln(m, s, ps.qt->so, nullptr, q.ctx, Ly.self, q, Rq, d));
        if (L) TRY(post_out_ln(m, s, ps.tt->so, nullptr, t.ctx, Ly.self, t, Rt, d));
        if (Ly.has_cross) {
            const char* kv = ps.resident_kv ? itm_ckv_slot(m, slot++) : (const char*)m->qkvimg;
            if (nq) {
                TRY(gemm(m, s, ps.qt->cq, q.x_t, Q, Ly.cross.in, q.qkv, Q, m->attn_out(), Rq));
                if (!ps.resident_kv) TRY(gemm(m, s, ps.qt->ckv, m->emb_t, D, Ly.ckv, m->qkvimg, 2 * Q, m->attn_out(), B * NT));
                {
                    ProfScope p(m, s, ps.qt->cross_attn, 4.0 * B * H * (double)nq * NT * hd, (double)B * NT * 2 * Q * e);
                    TRY(launch_generic_attention(m->dt, q.qkv, Q, (long)nq * Q, kv, 2 * Q, (long)NT * 2 * Q, kv + Q * e, 2 * Q, (long)NT * 2 * Q,
                                                 q.ctx, Q, (long)nq * Q, B, nq, NT, H, hd, -1, s, m->gdt));
                }
                TRY(post_out_ln(m, s, ps.qt->co, nullptr, q.ctx, Ly.cross, q, Rq, d));
            }
        }
        if (nq) TRY(post_ffn(m, s, *ps.qt, Ly.ffn, q, Rq, d));
        if (L) TRY(post_ffn(m, s, *ps.tt, Ly.ffn_text, t, Rt, d));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- BLIP-2 image-text scorer
// HF `Blip2ForImageTextRetrieval` state-dict names (transformers 5.x; `image_token_index` None: the ITM checkpoints): the ViT-g
// tower, the Q-Former with both FFN sets, the text embeddings and the three heads (fp32 for the head kernels).
int build_blip2_itm(Captioner* m) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, Q = c.q_hidden, F = c.q_ffn, P = c.embed_dim, nq = c.num_query_tokens;
    TRY(reg_stem(m, kBlipVision));
    TRY(reg_tower(m, kBlipVision, m->vl, c.v_layers, D, c.v_mlp, m->post));
    TRY(reg_qformer(m, true));
    TRY(reg_f32(m, "embeddings.word_embeddings.weight", &m->i_word, (int64_t)c.vocab * Q));
    TRY(reg_f32(m, "embeddings.position_embeddings.weight", &m->i_pos, (int64_t)c.max_pos * Q));
    TRY(reg_ln(m, "qformer.layernorm.", m->i_ln, Q));
    TRY(reg_f32(m, "vision_projection.weight", &m->i_vproj, (int64_t)P * Q));
    TRY(reg_f32(m, "vision_projection.bias", &m->i_vproj_b, P));
    TRY(reg_f32(m, "text_projection.weight", &m->i_tproj, (int64_t)P * Q));
    TRY(reg_f32(m, "text_projection.bias", &m->i_tproj_b, P));
    TRY(reg_f32(m, "itm_head.weight", &m->i_head, (int64_t)2 * Q));
    TRY(reg_f32(m, "itm_head.bias", &m->i_head_b, 2));
    // arena: image rows [max_batch * tokens, .], query rows [max_batch * nq, .], text rows [max_batch * max_len, .]
    const size_t Bm = c.max_batch, M = Bm * m->NT, e = m->esz;
    int ncross = 0;
    for (const PostLayer& L : m->pl) ncross += L.has_cross;
    TRY(alloc_image_tower(m));
    TRY(dev_alloc(m, (void**)&m->emb_f, M * D * 4));
    TRY(dev_alloc(m, &m->emb_t, M * D * e));
    TRY(dev_alloc(m, &m->itm_ckv, (size_t)ncross * M * 2 * Q * e, ARENA_KEPT, "itm_ckv"));
    TRY(alloc_post_rows(m, m->qr, Bm * nq, Q, F));
    return alloc_post_rows(m, m->tr, Bm * c.max_len, Q, F);
}

// ---------------------------------------------------------------------------------------------- sentence encoder
// HF BertModel state-dict names, as sentence-transformers stores all-MiniLM-L6-v2 (6 layers, 384 wide, 12 heads of 32,
// FFN 1536, post-LN, eps 1e-12).  Replaces `SentenceTransformer("all-MiniLM-L6-v2").encode(caption)` - reference
// agents/goal_exploration/goal_exploration.py:57,102 and detector/pseudolabeler.py:568,677.
int build_minilm(Captioner* m) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden, F = c.t_ffn, V = c.vocab;
    TRY(reg_f32(m, "embeddings.word_embeddings.weight", &m->word_f32, (int64_t)V * T));
    TRY(reg_f32(m, "embeddings.position_embeddings.weight", &m->tpos, (int64_t)c.max_pos * T));
    TRY(walloc(m, (void**)&m->tok_type, (size_t)2 * T * 4));
    add_slot(m, "embeddings.token_type_embeddings.weight", m->tok_type, CAP_DT_F32, 2, T);
    TRY(reg_ln(m, "embeddings.LayerNorm.", m->emb, T));
    TRY(reg_post_layers(m, kBertNames, c.t_layers, T, F, 0, 0, false));
    return alloc_post_rows(m, m->te, (size_t)c.max_batch * c.max_len, T, F);
}

// ids int32 [B, L] (padded rows: any valid id), lens int32 [B] (tokens incl. [CLS]/[SEP]) -> out fp32 [B, T]: mean of the
// last hidden states over the valid tokens, L2-normalised.
int run_text_encoder(Captioner* m, const int* ids, const int* lens, int B, int L, float* out, hipStream_t s) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden, H = c.t_heads, M = B * L;
    const PostDims d = {T, c.t_ffn, c.t_eps};
    const PostTags& tg = kMiniLMTags;
    const PostRows& r = m->te;
    {
        ProfScope ps(m, s, "te_embed", 0, (double)M * T * (12 + m->esz));
        TRY(launch_embed_tokens(m->dt, ids, L, m->word_f32, m->tpos, m->tok_type, m->emb.g, m->emb.b, c.t_eps, r.x_t, r.x, M, T, s,
                                c.vocab));
    }
    for (const PostLayer& Ly : m->pl) {
        TRY(post_qkv(m, s, tg, Ly.self, r, M, d));
        {
            ProfScope ps(m, s, tg.self_attn, 4.0 * B * H * (double)L * L * (T / H), (double)M * 4 * T * m->esz);
            TRY(launch_text_attention(m->dt, r.qkv, lens, r.ctx, B, L, H, T / H, s));
        }
        TRY(post_out_ln(m, s, tg.so, tg.ln, r.ctx, Ly.self, r, M, d));
        TRY(post_ffn(m, s, tg, Ly.ffn, r, M, d));
    }
    ProfScope ps(m, s, "te_pool", 0, (double)M * T * 4);
    return launch_mean_pool_normalize(r.x, lens, B, L, T, out, s);
}

// ---------------------------------------------------------------------------------------------- pre-LN towers
// Image tower stem: patchify, patch GEMM (+ position rows, + bias where the checkpoint has one), class rows, ln_pre where the
// checkpoint has one -> vt.X [B * NT, D].
int run_stem(Captioner* m, const void* pixels, int fmt, int B, const TowerTags& tg, hipStream_t s) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, NT = m->NT;
    float* X = m->vt.X;
    {
        ProfScope ps(m, s, tg.patchify, 0, (double)B * 3 * c.image_size * c.image_size * (fmt ? 1 : 4) + (double)B * m->P * m->Kpad * m->esz);
        TRY(launch_patchify(m->gdt, pixels, fmt, B, c.image_size, c.patch_size, m->Kpad, m->patches, c.pix_mean, c.pix_std, s));
    }
    GemmOpt patch;
    patch.epi = EPI_PATCH; patch.p0 = m->P; patch.aux = m->vpos;
    TRY(gemm(m, s, tg.patch, m->patches, m->Kpad, m->patch, X, D, OUT_F32, B * m->P, ACT_NONE, patch));
    TRY(launch_cls_rows(m->cls, m->vpos, X, B, NT, D, s));
    if (!m->ln_pre.g) return 0;
    ProfScope ps(m, s, tg.ln, 0, (double)B * NT * D * 8);
    return launch_layernorm(m->dt, X, D, m->ln_pre.g, m->ln_pre.b, c.v_eps, nullptr, X, B * NT, D, s);
}

// The pre-LN blocks of a tower over the fp32 residual stream t.X [B * N, D], then its final step: the LayerNorm `fin`
// of the last hidden states to fin_t (compute type) / fin_f (fp32, optional), or with fin == null no LayerNorm - X is left
// holding the last hidden states (CLIP: the head kernel normalises the pooled rows).  act: fc1's activation (gemm.h).  causal:
// the text tower's mask - the generic attention kernel, which in the split mode reads fp32 q|k|v (the G8 kernel takes no mask).
// Exact fp32 mode: the two branch GEMMs (proj, fc2) write their output to t.delta; the next LayerNorm kernel folds it into X in
// the same pass that normalises it, so the GEMM epilogues are store-only.  Other modes: they add into X themselves.
int run_tower(Captioner* m, hipStream_t s, const std::vector<VLayer>& layers, const Tower& t, int B, int N, int D, int H, int F,
              float eps, GemmAct act, bool causal, const TowerTags& tg, const Norm* fin, void* fin_t, float* fin_f) {
    const int M = B * N;
    const bool in_place = vit_adds_in_place(m->gdt);
    float* branch_out = in_place ? t.X : t.delta;
    const GemmOpt branch = GemmOpt::residual(in_place ? t.X : nullptr);
    // split mode: q|k|v stay G8 when the split-fp16 MFMA attention kernel covers this token count, else the GEMM writes fp32
    // for the fp32 attention kernels; either way the context comes out as G8 (the proj GEMM's operand)
    const bool g8_attn = !causal && m->gdt == CAP_DT_G8 && D / H == 64 && vit_attention_takes_g8(N);
    bool pending = false;                                  // delta holds a branch output not yet added to X
    auto add_ln = [&](const Norm& n, void* out_t, float* out_f) -> int {
        ProfScope ps(m, s, tg.ln, 0, (double)M * D * ((pending ? 12 : 4) + (out_t ? m->esz : 0) + (out_f ? 4 : 0)));
        if (pending) return launch_reduce_layernorm(m->gdt, t.delta, 1, nullptr, t.X, n.g, n.b, eps, out_t, out_f, t.X, M, D, s);
        return launch_layernorm(m->gdt, t.X, D, n.g, n.b, eps, out_t, out_f, M, D, s);
    };
    for (const VLayer& L : layers) {
        TRY(add_ln(L.ln1, t.ln, nullptr));
        TRY(gemm(m, s, tg.qkv, t.ln, D, L.qkv, t.qkv, 3 * D, (m->gdt == CAP_DT_G8 && !g8_attn) ? OUT_F32 : OUT_T, M));
        {
            ProfScope ps(m, s, tg.attn, (causal ? 2.0 : 4.0) * B * H * (double)N * N * 64, (double)M * 4 * D * m->esz);
            TRY(launch_vit_attention(g8_attn ? CAP_DT_G8 : m->dt, t.qkv, t.ctx, B, N, H, 0, s, D / H, causal ? 1 : 0, m->gdt));
        }
        TRY(gemm(m, s, tg.proj, t.ctx, D, L.proj, branch_out, D, OUT_F32, M, ACT_NONE, branch));
        pending = !in_place;
        TRY(add_ln(L.ln2, t.ln, nullptr));
        TRY(gemm(m, s, tg.fc1, t.ln, D, L.fc1, t.mlp, F, OUT_T, M, act));
        TRY(gemm(m, s, tg.fc2, t.mlp, F, L.fc2, branch_out, D, OUT_F32, M, ACT_NONE, branch));
    }
    if (fin) return add_ln(*fin, fin_t, fin_f);
    // no LayerNorm outputs: the pass only folds the last fc2 output into X (gamma / beta: any valid vectors)
    return pending ? add_ln(layers.back().ln2, nullptr, nullptr) : 0;
}

// BLIP / BLIP-2: final LayerNorm = post_layernorm -> image_embeds (fp32 to the caller + T for the cross-K/V GEMM).
// CoCa: ln_pre after the embeddings; final LayerNorm = the pooler's ln_k -> T only (run_coca_pool continues).
int run_encoder(Captioner* m, const void* pixels, int fmt, int B, float* out_embeds, hipStream_t s) {
    const CapConfig& c = m->c;
    float* emb_f = c.arch == CAP_ARCH_COCA ? nullptr : out_embeds ? out_embeds : m->emb_f;
    TRY(run_stem(m, pixels, fmt, B, kEncoderTags, s));
    return run_tower(m, s, m->vl, m->vt, B, m->NT, c.v_hidden, c.v_heads, c.v_mlp, c.v_eps, ACT_GELU, false, kEncoderTags, &m->post,
                     m->emb_t, emb_f);
}

// ViT-g over B images -> emb_t [B * NT, D] (post_layernorm on every token), then the cross-attention K/V of every cross layer of
// the Q-Former (they depend on the image alone) -> itm_ckv: what an ITC and an ITM call on this image batch both read.
int run_itm_images(Captioner* m, const void* pixels, int fmt, int B, hipStream_t s) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, Q = c.q_hidden, NT = m->NT;
    m->itm_B = 0;
    TRY(run_encoder(m, pixels, fmt, B, nullptr, s));
    size_t slot = 0;
    for (const PostLayer& L : m->pl) {
        if (!L.has_cross) continue;
        TRY(gemm(m, s, kItmQueryTags.ckv, m->emb_t, D, L.ckv, itm_ckv_slot(m, slot++), 2 * Q, m->attn_out(), B * NT));
    }
    m->itm_B = B;
    return 0;
}

// ---------------------------------------------------------------------------------------------- CLIP scorer
// HF CLIPModel state-dict names (transformers models/clip/modeling_clip.py): kClipVision / kClipText, the projections fp32 for
// the head kernel.
int build_clip(Captioner* m) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, T = c.t_hidden, P = c.embed_dim;
    TRY(reg_stem(m, kClipVision));
    TRY(reg_tower(m, kClipVision, m->vl, c.v_layers, D, c.v_mlp, m->post));
    TRY(walloc(m, (void**)&m->c_vproj, (size_t)P * D * 4));
    add_slot(m, "visual_projection.weight", m->c_vproj, CAP_DT_F32, P, D);
    TRY(reg_f32(m, "text_model.embeddings.token_embedding.weight", &m->c_tok, (int64_t)c.vocab * T));
    TRY(reg_f32(m, "text_model.embeddings.position_embedding.weight", &m->tpos, (int64_t)c.max_pos * T));
    TRY(reg_tower(m, kClipText, m->ctl, c.t_layers, T, c.t_ffn, m->c_lnf));
    TRY(walloc(m, (void**)&m->c_tproj, (size_t)P * T * 4));
    add_slot(m, "text_projection.weight", m->c_tproj, CAP_DT_F32, P, T);
    TRY(reg_f32(m, "logit_scale", &m->c_logit, 1));
    // arena: image rows [max_batch * tokens, .], text rows [max_batch * max_len, .]
    TRY(alloc_image_tower(m));
    return alloc_tower(m, m->ct, (size_t)c.max_batch * c.max_len, T, c.t_ffn);
}

GemmAct clip_act(const Captioner* m) { return m->c.hidden_act == CAP_ACT_GELU ? ACT_GELU : ACT_QUICK_GELU; }

int run_clip_images(Captioner* m, const void* pixels, int fmt, int B, float* out, hipStream_t s) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, NT = m->NT;
    TRY(run_stem(m, pixels, fmt, B, kClipImageTags, s));
    TRY(run_tower(m, s, m->vl, m->vt, B, NT, D, c.v_heads, c.v_mlp, c.v_eps, clip_act(m), false, kClipImageTags, nullptr, nullptr,
                  nullptr));
    ProfScope ps(m, s, "clip_v_head", 2.0 * B * D * c.embed_dim, (double)B * D * 4 + (double)c.embed_dim * D * 4);
    return launch_clip_head(m->vt.X, NT, nullptr, m->post.g, m->post.b, c.v_eps, m->c_vproj, out, B, D, c.embed_dim, s);
}

int run_clip_text(Captioner* m, const int* ids, const int* lens, int B, int L, float* out, hipStream_t s) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden;
    {
        ProfScope ps(m, s, "clip_t_embed", 0, (double)B * L * T * 12);
        TRY(launch_clip_embed_text(ids, L, m->c_tok, m->tpos, m->ct.X, B * L, T, c.vocab, s));
    }
    TRY(run_tower(m, s, m->ctl, m->ct, B, L, T, c.t_heads, c.t_ffn, c.t_eps, clip_act(m), true, kClipTextTags, nullptr, nullptr,
                  nullptr));
    ProfScope ps(m, s, "clip_t_head", 2.0 * B * T * c.embed_dim, (double)B * T * 4 + (double)c.embed_dim * T * 4);
    return launch_clip_head(m->ct.X, L, lens, m->c_lnf.g, m->c_lnf.b, c.t_eps, m->c_tproj, out, B, T, c.embed_dim, s);
}

// CoCa attentional pooler + ln_post, then the affine-free normalisation that feeds the folded cross-K/V projection.
// tokens_out (optional): fp32 [B, Q, E] = ln_post(pooler output); row 0 of each image is the pooled token, rows 1..Q-1
// are the image_embs the decoder cross-attends (reference coca_model.py:152-155).
int run_coca_pool(Captioner* m, int B, float* tokens_out, hipStream_t s) {
    const CapConfig& c = m->c;
    const int D = c.v_hidden, E = m->E, Q = m->Q, NT = m->NT;
    // split mode: k | v of the pooler are read by the attention kernel as fp32; its context is the out_proj GEMM's G8 operand
    TRY(gemm(m, s, "gemm_pool_kv", m->emb_t, D, m->pool_kv, m->pool_kvbuf, 2 * E, m->attn_out(), B * NT));
    {
        ProfScope ps(m, s, "pool_attention", 4.0 * B * Q * (double)NT * E, (double)B * NT * 2 * E * m->esz);
        TRY(launch_pool_attention(m->dt, m->pool_q, m->pool_kvbuf, m->pool_ctx, B, NT, Q, E, c.pool_heads, s, m->gdt));
    }
    TRY(gemm(m, s, "gemm_pool_o", m->pool_ctx, E, m->pool_out, m->pool_o, E, OUT_F32, B * Q));
    float* tok = tokens_out ? tokens_out : m->img_tokens;
    TRY(launch_layernorm(m->dt, m->pool_o, E, m->lnpost.g, m->lnpost.b, c.v_eps, nullptr, tok, B * Q, E, s));
    TRY(launch_layernorm(m->gdt, tok, E, m->ones, m->zeros, c.v_eps, m->xhat, nullptr, B * Q, E, s));
    return 0;
}

// ---------------------------------------------------------------------------------------------- decoder
// The decode state of one call: B images, R = B*K rows, the arena's buffers.  (cap_generate decodes the whole batch as one range:
// row slices of ONE batch on their own streams measured level at 2 and slower at 3-4 - DESIGN.md section 4 - and were removed;
// whole batches overlap through engine.EnginePool instead.)
struct Dec {
    int B, R;
    float *dx, *dy, *logits, *dpart;
    float* dx2;           // the fused paths' second LayerNorm row buffer
    void *dx_t, *dq, *dctx, *dh;
    int *seq, *finished, *lens, *anc;
    void* beam;
    RowMap map;           // compacted greedy loop: the open rows (live / count on the device); null pointers = every row
};

Dec make_dec(Captioner* m, int B, int K) {
    Dec d;
    d.B = B; d.R = B * K;
    d.dx = m->dx; d.dy = m->dy; d.logits = m->logits; d.dpart = m->dpart; d.dx2 = m->dx2;
    d.dx_t = m->dx_t; d.dq = m->dq; d.dctx = m->dctx; d.dh = m->dh;
    d.seq = m->seq; d.finished = m->finished; d.lens = m->lens; d.anc = m->anc; d.beam = m->beam;
    return d;
}

// K slices of a decode GEMM: a function of (N, K, operand type) ONLY - never of the row count, so a caption's sums are ordered
// the same way alone and in a batch of 256.  bf16 / split mode run the "rows" kernel (gemm_rows_kernel: the block's K range
// over its four waves): as many slices as still give every wave a slab, keep the grid within one round of the CUs at the
// nominal 256 rows, and at most 4 (more slices write and re-read more partial sums than they save).  fp32 mode: the
// register-staged 64x64 tile with >= 3 slabs per slice.
int decode_splitk(const Captioner* m, int N, int K, int max_S) {
    if (m->gdt == CAP_DT_F32) {
        const int nk = K / 32;
        for (int cand : {4, 2})
            if (cand <= max_S && nk % cand == 0 && nk / cand >= 3) return cand;
        return 1;
    }
    // nominal row count the grid is sized for: a property of the ARCHITECTURE's deployment (BLIP / CoCa decode a few hundred
    // rows = images x beams at once; the OPT decoder of BLIP-2 a few dozen), never of the call
    const int plan_rows = m->c.arch == CAP_ARCH_BLIP2 ? 64 : 256;
    const int nk = K / (m->gdt == CAP_DT_BF16 ? 64 : 32), tiles = ((plan_rows + 63) / 64) * ((N + 63) / 64);
    for (int cand : {8, 6, 5, 4, 3, 2})      // (> 4 only where the caller allows it: the OPT decoder's weight streams at a few dozen rows)
        if (cand <= max_S && nk % cand == 0 && nk / cand >= 4 && tiles * cand <= 256) return cand;
    return 1;
}
inline int decode_tile(const Captioner* m) { return m->gdt == CAP_DT_F32 ? 2 : 6; }

int gemm_partial(Captioner* m, hipStream_t s, const char* tag, const void* A, const Linear& L, float* part, int R, int max_S, int* S_out,
                 const int* m_live = nullptr) {
    *S_out = decode_splitk(m, L.N, L.K, max_S);
    GemmParams p = gemm_params(A, L.K, L.w, L.ld, nullptr, part, L.N, R, L.N, L.K, ACT_NONE, OUT_F32, EPI_PARTIAL, *S_out);
    p.m_live = m_live;
    return run_gemm(m, s, tag, p, decode_tile(m));
}

// A finished decode projection over dense rows (bias + activation -> operand type): fc1 of the text layers.  Same kernel family
// as the split-K ones at every row count.
int gemm_rows(Captioner* m, hipStream_t s, const char* tag, const void* A, const Linear& L, void* C, int R, GemmAct act,
              const int* m_live = nullptr) {
    GemmOpt o = GemmOpt::live(m_live);
    o.tile = m->gdt == CAP_DT_F32 ? 0 : 6;
    return gemm(m, s, tag, A, L.K, L, C, L.N, OUT_T, R, act, o);
}

// Decode-sized GEMM whose consumer is a LayerNorm: split K over S blocks per tile (every block's slabs are all in flight
// at once -> one memory round trip), partial sums to dpart, then the block-per-row kernel: y = sum + bias + d.dx (-> y_out)
// and LayerNorm(y) -> out_t / out_f.  (Running the consumer inside the GEMM kernel behind arrival counters cost more than the
// launch it saves - cross-XCD hand-over, DESIGN.md section 4 - and was removed.)
int gemm_splitk_reduce_ln(Captioner* m, hipStream_t s, const Dec& d, const char* tag, const void* A, const Linear& L, const Norm& ln,
                          float eps, void* out_t, float* out_f, float* y_out) {
    const int N = L.N;
    int S = 1;
    TRY(gemm_partial(m, s, tag, A, L, d.dpart, d.R, 4, &S, d.map.n));
    const bool per_row_block = d.R < (d.map.n ? 512 : 832) || N > 1024;
    ProfScope ps(m, s, per_row_block ? "dec_reduce_ln" : "dec_reduce_ln_wave", 0, (double)(S + 2) * d.R * N * 4 + (double)d.R * N * m->esz);
    // one 256-thread block per row up to several hundred rows (one memory round trip, latency-bound); at the pool's 1 024-row
    // passes the wave-per-row kernel.  Launches replayed from a captured graph (tools/bench_reduce_ln.py, us per launch, block / wave,
    // split mode | bf16 in place, the CoCa form): 512 rows 5.6 / 6.3 | 5.3 / 6.2, 640 (config 5: 128 images x 5 beams) 6.5 / 6.5 | 6.3 /
    // 6.6, 768 6.6 / 6.7 | 6.4 / 6.8, 896 7.6 / 7.0 | 7.3 / 7.0, 1 024 7.8 / 7.4 | 7.4 / 7.2: the crossing is between 768 and 896 (round 5
    // had put it at 512 from the 1 024-row figure alone, which cost config 5 ~4 % - dec_reduce_ln 17.6 -> 22.3 ms per step).  Same sums in
    // the same order - the two kernels give the same bits (tests/test_kernels_gpu.py::test_reduce_layernorm_kernels_agree_bit_for_bit),
    // so the row count may choose.  In the COMPACTED greedy loop (d.map: rows beyond the live count return at once) the wave kernel
    // keeps its round-5 threshold of 512 rows: a dead row costs it one wave's dispatch instead of four, and most steps of a 768-row
    // pass have far fewer live rows than that - same box, `bench.py --lite`, three interleaved pairs, 512 / 832: 6 476 / 6 460, 6 511 /
    // 6 476, 6 525 / 6 491 captions/s (+0.4 %).
    return launch_reduce_layernorm(m->gdt, d.dpart, S, L.b, d.dx, ln.g, ln.b, eps, out_t, out_f, y_out, d.R, N, s, per_row_block, d.map.n);
}

// Cross K/V of cache slot `slot` in a call over B images (the slots are packed for the CALL's B).  by_row: the bases of the slot's k /
// v blocks and the index of the first head row to attend in them - how a KV16 cache is addressed (head rows inside a block), and
// how the fused small-batch kernel addresses every cache; otherwise the bases already moved to that row (row0 = 0).
struct CrossKV { const char *k, *v; size_t row0; };
CrossKV cross_kv(const Captioner* m, int slot, int B, bool by_row) {
    const size_t blk = cross_slot_bytes(m, B) / 2, first = m->dec.kv_first;
    const char* k = (const char*)m->cross + (size_t)slot * 2 * blk + (by_row ? 0 : first * m->kvrow);
    return {k, k + blk, by_row ? first : 0};
}

// The head over R rows whose operand is x_t: BLIP's transform (dense + GELU -> d.dy, its LayerNorm back to x_t / x_f), then the
// vocabulary GEMM -> d.logits
int run_head(Captioner* m, hipStream_t s, const Dec& d, void* x_t, float* x_f, int R, const int* m_live) {
    const DecPlan& P = m->dec;
    const int W = P.W;
    if (P.tr.w) {
        TRY(gemm(m, s, P.tags->tr, x_t, W, P.tr, d.dy, W, OUT_F32, R, ACT_GELU, GemmOpt::live(m_live)));
        ProfScope ps(m, s, P.tags->ln, 0, (double)R * W * (8 + m->esz));
        TRY(launch_layernorm(m->gdt, d.dy, W, P.tr_ln.g, P.tr_ln.b, m->c.t_eps, x_t, x_f, R, W, s, m_live));
    }
    return gemm(m, s, P.tags->vocab, x_t, W, P.vocab, d.logits, m->ldl, OUT_F32, R, ACT_NONE, GemmOpt::live(m_live));
}

// One KV-cached decoder step on the batch kernels: embedding, the plan's sub-layers, head -> d.logits.  Per sub-layer: the input
// projection (q|k|v and the cross query as split-K partial sums the attention kernel finishes - one memory round trip per kernel
// instead of two in the GEMM; fc finished, GELU), the attention, then gemm_splitk_reduce_ln: the output projection and its
// consumer, which adds the branch to the residual row d.dx and writes the LayerNorm to d.dx_t, the next GEMM's operand - post-LN
// also to d.dx, pre-LN the sum itself goes to d.dx.  (The reference recomputes CoCa's whole prefix through both text towers
// every step, coca_model.py:294-303.)
// tokens [R, tok_ld]: newest token of every row at column t; K rows per image share the image's cross K/V; anc (beams): the
// ancestry table of the self-attention caches (row r's history position j was written by physical row anc[r][j]).
int run_step(Captioner* m, const Dec& d, const int* tokens, int tok_ld, int t, int K, const int* anc, int Lm, hipStream_t s) {
    const CapConfig& c = m->c;
    const DecPlan& P = m->dec;
    const DecTags& tg = *P.tags;
    const int W = P.W, H = c.t_heads, R = d.R;
    const size_t e = m->esz;
    // greedy: a caption that has ended (d.finished, set by greedy_select one step before) is not computed any more.  Compacted
    // (d.map, the merged passes of ~1 000 rows: at that size the projections are no longer a weight stream - 47 % of the decode
    // kernels' time): every kernel of the step works on the open captions' rows, packed to the front - activations, split-K
    // slabs and logits are indexed by the compact row, tokens / self-attention cache rows / the image's cross K/V through
    // map.live[c]; row tiles, rows and (row, head) units from *map.n on return at once.  Without a map (beams, per-step logits
    // wanted, forced off): the attention kernels skip ended rows in place and the GEMMs cover every row.
    const bool cm = d.map.n != nullptr;
    const int* skip = (P.skip_finished && K == 1 && !cm) ? d.finished : nullptr;
    TRY(launch_embed(m->gdt, tokens, tok_ld, t, P.word, P.pos, P.emb.g, P.emb.b, c.t_eps, d.dx_t, P.pre_ln ? nullptr : d.dx, R, W, s,
                     P.pre_ln ? d.dx : nullptr, d.map));
    for (const SubLayer& u : P.subs) {
        const void* A = d.dctx;      // the output projection's operand [R, u.out.K]
        int S = 1;
        if (u.kind == DEC_FFN) {
            TRY(gemm_rows(m, s, tg.in[DEC_FFN], d.dx_t, u.in, d.dh, R, ACT_GELU, d.map.n));
            A = d.dh;
        } else {
            DecodeAttn a;
            memset(&a, 0, sizeof(a));
            a.out = d.dctx; a.R = R; a.H = H; a.out_dtype = m->gdt; a.skip_rows = skip; a.map = d.map;
            if (u.kind == DEC_SELF) {
                a.kbase = u.cache; a.vbase = (char*)u.cache + (size_t)R * H * Lm * 64 * e;
                a.anc = anc; a.anc_ld = Lm; a.rows_per_kv = 1; a.kv_ld = Lm; a.n_keys = t + 1;
            } else {
                // beam-shared cross K/V; a KV16 cache is addressed by row index: the kernel gets the block bases and the first row
                const CrossKV kv = cross_kv(m, u.slot, d.B, m->kv16);
                a.kbase = kv.k; a.vbase = kv.v; a.kv16 = m->kv16 ? 1 : 0; a.kv_row0 = kv.row0;
                a.rows_per_kv = K; a.kv_ld = P.kv_tokens; a.n_keys = P.kv_keys;
            }
            const int self = u.kind == DEC_SELF, Nin = u.in.N;
            double bytes = self ? 2.0 * R * H * a.n_keys * 64 * e : 2.0 * d.B * H * a.n_keys * m->kvrow;
            // (positions beyond 32: BLIP's un-fused branch.  CoCa has none: its step fails the attention launcher's 32-position check)
            if (!self || t + 1 <= 32 || P.pre_ln) {
                TRY(gemm_partial(m, s, tg.in[u.kind], d.dx_t, u.in, d.dpart, R, 4, &S, d.map.n));
                a.q_part = d.dpart; a.q_S = S; a.q_bias = u.in.b; a.q_ld = Nin; a.append_kv = self;   // self: k / v finished and appended too
                if (self && !P.pre_ln) bytes += (double)S * R * Nin * 4;     // (the figure CoCa reports has never counted the partial sums)
            } else {
                if (cm) { cap_set_error("run_step: the compacted loop takes up to 32 positions"); return -1; }   // (run_generate never asks)
                GemmOpt qkv;         // q -> d.dq, k / v of position t -> the cache rows [R][H][Lm][64]
                qkv.epi = EPI_QKVCACHE; qkv.p0 = R; qkv.p1 = H; qkv.p2 = Lm; qkv.p3 = t; qkv.C2 = u.cache;
                TRY(gemm(m, s, tg.in[DEC_SELF], d.dx_t, W, u.in, d.dq, W, OUT_T, R, ACT_NONE, qkv));
                a.q = d.dq;
            }
            ProfScope ps(m, s, tg.attn[u.kind], 4.0 * R * H * a.n_keys * 64, bytes);
            TRY(launch_decode_attention(m->dt, a, s));
        }
        TRY(gemm_splitk_reduce_ln(m, s, d, tg.out[u.kind], A, u.out, u.ln, c.t_eps, d.dx_t, P.pre_ln ? nullptr : d.dx,
                                  P.pre_ln ? d.dx : nullptr));
    }
    // the head: compacted, its row tiles and rows from the open count on return too (the split / bf16 kernels of these shapes take
    // GemmParams::m_live; an fp32-mode vocabulary GEMM covers every row of the pass - the dead rows' logits are never read)
    return run_head(m, s, d, d.dx_t, d.dx, R, d.map.n);
}

// ---------------------------------------------------------------------------------------------- small-batch decoder step
// Up to SMALL_MAX_ROWS rows (the reference calls the captioners with ONE crop - coca.py:27-33 -, BASELINE config 1 with 8): the
// same step as run_step in 2 launches per sub-layer (BLIP 6 per layer instead of 11, CoCa 4 per block instead of 7) - every
// split-K consumer / LayerNorm and the self-attention run in the prologue of the kernel that needs their result, the first half
// of a cross sub-layer (LayerNorm, query projection, attention) is one kernel per (row, head) - decode_small.hip.  The sums are
// those of the batch kernels (same K-slice plan, same chains, same LayerNorm / attention arithmetic): logits and tokens have the
// same bits on either path (tests/test_small_decode_gpu.py).  The fp32 residual rows (the batch path's dx) alternate between d.dx
// and d.dx2: the one workgroup that writes a row never writes the buffer the others are still reading.  Post-LN the row kept is
// the consumer's LayerNorm, pre-LN its SUM (SmallLN::x_is_sum), the LayerNorm then only feeds the GEMM.
bool small_path_takes(const Captioner* m, const Dec& d, int t) {
    const CapConfig& c = m->c;
    if (m->gdt == CAP_DT_F32 || (c.arch != CAP_ARCH_BLIP && c.arch != CAP_ARCH_COCA) || !d.dx2) return false;
    if (d.R > SMALL_MAX_ROWS || t + 1 > 32) return false;
    const int T = m->dec.W, F = c.t_ffn, slab = m->gdt == CAP_DT_BF16 ? 64 : 32;
    if (T > 1024 || T != c.t_heads * 64 || T % 16 != 0 || F % 16 != 0 || T % slab != 0 || F % slab != 0) return false;
    // q|k|v partial sums sit beside the [<= 4][R][T] slabs of the other GEMMs in dpart (12 R T floats): at most 2 K slices
    return decode_splitk(m, 3 * T, T, 4) <= 2;
}

int run_step_small(Captioner* m, const Dec& d, const int* tokens, int tok_ld, int t, int K, const int* anc, int Lm, hipStream_t s) {
    const CapConfig& c = m->c;
    const DecPlan& P = m->dec;
    const DecTags& tg = *P.tags;
    const int W = P.W, H = c.t_heads, R = d.R, nk = P.kv_keys;
    const size_t e = m->esz;
    const int* skip = (P.skip_finished && K == 1) ? d.finished : nullptr;
    float* xb[2] = {d.dx, d.dx2};
    int cur = 0;                                   // xb[cur]: the row the next consumer adds as its residual
    float* qkvp = d.dpart + (size_t)4 * R * W;     // q|k|v partial sums, beside the [<= 4][R][W] slabs of the other GEMMs
    const int kv_kind = m->kv16 ? SMALL_KV_KV16 : (m->dt == CAP_DT_BF16 ? SMALL_KV_BF16 : SMALL_KV_F32);
    TRY(launch_embed(m->gdt, tokens, tok_ld, t, P.word, P.pos, P.emb.g, P.emb.b, c.t_eps, d.dx_t, P.pre_ln ? nullptr : xb[0], R, W, s,
                     P.pre_ln ? xb[0] : nullptr));
    SmallLN pend;                                  // the consumer of the last sub-layer: the next kernel's prologue runs it
    memset(&pend, 0, sizeof(pend));
    // one projection of the step: the batch path's K slices as partial sums (the consumer adds the bias), or finished in one
    auto base = [&](const Linear& L, int pro, int epi) {
        SmallGemm g;
        memset(&g, 0, sizeof(g));
        g.W = L.w; g.R = R; g.N = L.N; g.K = L.K; g.pro = pro; g.epi = epi; g.nchain = 4;
        g.S = epi == SMALL_EPI_PARTIAL ? decode_splitk(m, L.N, L.K, 4) : 1;
        if (epi != SMALL_EPI_PARTIAL) g.bias = L.b;
        return g;
    };
    auto consume = [&](bool keep) {                // bind the pending consumer to the current residual row / the other buffer
        SmallLN ln = pend;
        ln.resid = xb[cur];
        ln.x_out = keep ? xb[cur ^ 1] : nullptr;
        if (keep) cur ^= 1;
        return ln;
    };
    auto launch = [&](const char* tag, const SmallGemm& g, double attn_flops = 0) {
        GemmScope ps(m, s, tag, R, g.N, g.K, g.epi == SMALL_EPI_PARTIAL ? 4.0 * g.S : g.epi == SMALL_EPI_ACT_T ? (double)e : 4.0, attn_flops);
        return launch_small_gemm(m->gdt, g, s);
    };
    bool first = true;                             // the first kernel reads the embedding's LayerNorm from d.dx_t
    for (const SubLayer& u : P.subs) {
        const char *t_in = tg.s_in[u.kind], *t_out = tg.s_out[u.kind];
        SmallGemm g;
        if (u.kind == DEC_SELF) {
            g = base(u.in, first ? SMALL_PRO_GLOBAL : SMALL_PRO_LN, SMALL_EPI_PARTIAL);
            if (first) g.A = d.dx_t; else g.ln = consume(true);
            g.out_part = qkvp;
            TRY(launch(t_in, g));
            g = base(u.out, SMALL_PRO_SELFATTN, SMALL_EPI_PARTIAL);
            g.sa.qkv_part = qkvp; g.sa.qkv_bias = u.in.b; g.sa.qkv_S = decode_splitk(m, u.in.N, u.in.K, 4); g.sa.kc = u.cache;
            g.sa.vc = (char*)u.cache + (size_t)R * H * Lm * 64 * e; g.sa.anc = anc; g.sa.anc_ld = Lm;
            g.sa.kv_ld = Lm; g.sa.n_keys = t + 1; g.sa.H = H; g.sa.skip = skip;
            g.out_part = d.dpart;
            TRY(launch(t_out, g, 4.0 * R * H * (t + 1) * 64));
        } else if (u.kind == DEC_CROSS) {
            SmallCross x;
            memset(&x, 0, sizeof(x));
            x.W = u.in.w; x.bias = u.in.b; x.R = R; x.D = W; x.H = H; x.S = decode_splitk(m, W, W, 4);
            x.ln = consume(true);
            const CrossKV kv = cross_kv(m, u.slot, d.B, true);
            x.kbase = kv.k; x.vbase = kv.v; x.kv_row0 = kv.row0;
            x.rows_per_kv = K; x.kv_ld = P.kv_tokens; x.n_keys = nk; x.kv_kind = kv_kind; x.skip = skip; x.out = d.dctx;
            {
                ProfScope ps(m, s, t_in, 2.0 * R * W * W + 4.0 * R * H * nk * 64, (double)W * W * e + 2.0 * R * H * nk * m->kvrow);
                TRY(launch_small_cross(m->gdt, x, s));
            }
            g = base(u.out, SMALL_PRO_GLOBAL, SMALL_EPI_PARTIAL);
            g.A = d.dctx; g.out_part = d.dpart;
            TRY(launch(t_out, g));
        } else {
            g = base(u.in, SMALL_PRO_LN, SMALL_EPI_ACT_T);
            g.ln = consume(true);
            g.act = ACT_GELU; g.out = d.dh; g.ldc = u.in.N;
            TRY(launch(t_in, g));
            g = base(u.out, SMALL_PRO_GLOBAL, SMALL_EPI_PARTIAL);
            g.A = d.dh; g.out_part = d.dpart;
            TRY(launch(t_out, g));
        }
        memset(&pend, 0, sizeof(pend));          // (g: the sub-layer's output projection)
        pend.part = d.dpart; pend.S = g.S; pend.bias = u.out.b; pend.gamma = u.ln.g; pend.beta = u.ln.b; pend.eps = c.t_eps;
        pend.x_is_sum = P.pre_ln ? 1 : 0;
        first = false;
    }
    if (P.tr.w) {   // prediction head transform: LayerNorm of the last FFN in the prologue, bias + GELU -> fp32
        SmallGemm g = base(P.tr, SMALL_PRO_LN, SMALL_EPI_ACT_F32);
        g.nchain = 1;
        g.ln = consume(false);
        g.act = ACT_GELU; g.out = d.dy; g.ldc = W;
        TRY(launch(tg.s_tr, g));
    }
    // vocabulary GEMM with the last LayerNorm in the prologue: the transform's over d.dy, else the pending consumer's (ln_final)
    SmallGemm g = base(P.vocab, SMALL_PRO_LN, SMALL_EPI_ACT_F32);
    g.nchain = 1;
    if (P.tr.w) { g.ln.part = d.dy; g.ln.S = 1; g.ln.gamma = P.tr_ln.g; g.ln.beta = P.tr_ln.b; g.ln.eps = c.t_eps; }
    else g.ln = consume(false);
    g.act = ACT_NONE; g.out = d.logits; g.ldc = m->ldl;
    return launch(tg.s_vocab, g);
}

// ---------------------------------------------------------------------------------------------- prompt prefill
// Positions 0 .. npos - 1 of the captions c0 .. c0 + nc - 1 of a greedy BLIP call (tokens already in d.seq) through every sub-layer of
// the decoder as ONE pass of nc * npos rows, caption-major: what npos calls of run_step would do to the self-attention caches, with
// one launch sequence and one read of every weight, and without the head (nobody selects a token at a prompt position).  Row-wise
// kernels - the split-K GEMMs (their slice plan depends on (N, K) only), the reduce + LayerNorm consumers, the FFN - are run_step's
// own at another row count; the cross-attention is run_step's with the npos rows of an image sharing its K/V the way beams do
// (rows_per_kv); the embedding and the self-attention are the prefill's kernels (launch_embed_prompt,
// launch_prefill_self_attention), built on the same row / unit functions.  So the caches hold the bits of the single steps.
// d: the CALL's decode state (d.B, d.R = its captions: the caches and the cross K/V are laid out for them).
// kv_rows / img0 (teacher-forced scoring, run_score: several captions of one image in a pass): the rows from row 0 on share cross K/V
// in runs of kv_rows, the first run image img0's; by default every caption is its own image (kv_rows = npos, img0 = c0).
int run_prefill(Captioner* m, const Dec& d, int c0, int nc, int npos, int Lm, hipStream_t s, int kv_rows = 0, int img0 = -1) {
    const CapConfig& c = m->c;
    const DecPlan& P = m->dec;
    const int W = P.W, H = c.t_heads, Rp = nc * npos;
    const size_t e = m->esz;
    if (P.pre_ln || c.arch != CAP_ARCH_BLIP) { cap_set_error("run_prefill: the prompt prefill is built for the BLIP text decoder"); return -1; }
    if ((size_t)Rp > m->ws_rows || c0 < 0 || c0 + nc > d.R) {
        cap_set_error("run_prefill: %d captions x %d positions from caption %d do not fit the workspace (%zu rows, %d captions)", nc, npos, c0,
                      m->ws_rows, d.R);
        return -1;
    }
    Dec pd = d;              // the pass: Rp rows of the shared buffers, no row map
    pd.R = Rp;
    pd.map = RowMap();
    {
        ProfScope ps(m, s, "prefill_embed", 0, (double)Rp * W * (8 + e));
        TRY(launch_embed_prompt(m->gdt, d.seq, Lm, npos, c0, P.word, P.pos, P.emb.g, P.emb.b, c.t_eps, pd.dx_t, pd.dx, nc, W, s));
    }
    for (const SubLayer& u : P.subs) {
        const void* A = pd.dctx;
        int S = 1;
        if (u.kind == DEC_FFN) {
            TRY(gemm_rows(m, s, "prefill_gemm_f1", pd.dx_t, u.in, pd.dh, Rp, ACT_GELU));
            A = pd.dh;
        } else if (u.kind == DEC_SELF) {
            TRY(gemm_partial(m, s, "prefill_gemm_qkv", pd.dx_t, u.in, pd.dpart, Rp, 4, &S));
            ProfScope ps(m, s, "prefill_self_attn", 2.0 * Rp * H * (npos + 1) * 64, (double)(S + 2) * Rp * 3 * W * 4);
            TRY(launch_prefill_self_attention(m->dt, pd.dpart, S, u.in.b, 3 * W, u.cache, (char*)u.cache + (size_t)d.R * H * Lm * 64 * e, Lm,
                                              pd.dctx, m->gdt, nc, npos, c0, H, s));
        } else {
            DecodeAttn a;
            memset(&a, 0, sizeof(a));
            a.out = pd.dctx; a.R = Rp; a.H = H; a.out_dtype = m->gdt;
            // the image of row r is c0 + r / npos (img0 + r / kv_rows where given): the slot's blocks from that image on
            const CrossKV kv = cross_kv(m, u.slot, d.B, m->kv16);
            const size_t hr0 = (size_t)(img0 < 0 ? c0 : img0) * H * P.kv_tokens;       // head rows before the first image
            a.kbase = m->kv16 ? kv.k : kv.k + hr0 * m->kvrow; a.vbase = m->kv16 ? kv.v : kv.v + hr0 * m->kvrow;
            a.kv16 = m->kv16 ? 1 : 0; a.kv_row0 = m->kv16 ? kv.row0 + hr0 : 0;
            a.rows_per_kv = kv_rows > 0 ? kv_rows : npos; a.kv_ld = P.kv_tokens; a.n_keys = P.kv_keys;
            TRY(gemm_partial(m, s, "prefill_gemm_cq", pd.dx_t, u.in, pd.dpart, Rp, 4, &S));
            a.q_part = pd.dpart; a.q_S = S; a.q_bias = u.in.b; a.q_ld = W;
            ProfScope ps(m, s, "prefill_cross_attn", 4.0 * Rp * H * a.n_keys * 64, 2.0 * nc * H * a.n_keys * m->kvrow);
            TRY(launch_decode_attention(m->dt, a, s));
        }
        const char* tag = u.kind == DEC_FFN ? "prefill_gemm_f2" : u.kind == DEC_SELF ? "prefill_gemm_so" : "prefill_gemm_co";
        TRY(gemm_splitk_reduce_ln(m, s, pd, tag, A, u.out, u.ln, c.t_eps, pd.dx_t, pd.dx, nullptr));
    }
    return 0;
}

__global__ void iota_rows_kernel(int* anc, int R, int L) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * R * L; i += gridDim.x * blockDim.x) anc[i] = (i / L) % R;
}
__global__ void init_seq_kernel(int* seq, int* fin, int* len, int R, int L, int bos, int pad) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < R * L; i += gridDim.x * blockDim.x) seq[i] = (i % L == 0) ? bos : pad;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < R; i += gridDim.x * blockDim.x) { fin[i] = 0; len[i] = L; }
}
__global__ void copy_i32_kernel(const int* s, int* d, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

// Image state (captioner_hip.h): what the decode side reads from the image side and where it lives in the arena - BLIP / CoCa the
// cross K/V cache, BLIP-2 the language projection's fp32 rows as 16-byte pieces.
bool takes_image_state(const Captioner* m) {
    return m->c.arch == CAP_ARCH_BLIP || m->c.arch == CAP_ARCH_COCA || m->c.arch == CAP_ARCH_BLIP2;
}
ImageStateLayout image_state_layout(const Captioner* m) {
    const CapConfig& c = m->c;
    if (c.arch == CAP_ARCH_BLIP2) return {1, c.num_query_tokens * c.t_hidden / 4, 16, 0};
    return {2 * (c.arch == CAP_ARCH_COCA ? c.mm_layers : c.t_layers), c.t_heads * m->dec.kv_tokens, m->kv16 ? 128 : (int)(64 * m->esz),
            m->kv16 ? 1 : 0};
}
void* image_state_buffer(const Captioner* m) { return m->c.arch == CAP_ARCH_BLIP2 ? (void*)m->lm_proj : m->cross; }
int export_image_state(Captioner* m, int B, void* state, hipStream_t s) {
    const ImageStateLayout L = image_state_layout(m);
    ProfScope ps(m, s, "state_export", 0, 2.0 * B * L.record_bytes());
    return launch_image_state_pack(L, B, image_state_buffer(m), state, s);
}
int import_image_state(Captioner* m, const void* state, int B, hipStream_t s) {
    const ImageStateLayout L = image_state_layout(m);
    ProfScope ps(m, s, "state_import", 0, 2.0 * B * L.record_bytes());
    return launch_image_state_unpack(L, B, image_state_buffer(m), state, s);
}

static int run_image_side(Captioner* m, const void* pixels, int fmt, int B, hipStream_t s) {
    const CapConfig& c = m->c;
    if (fmt == CAP_PIX_IMAGE_STATE) return import_image_state(m, pixels, B, s);
    TRY(run_encoder(m, pixels, fmt, B, nullptr, s));
    GemmOpt kv;              // every layer's k | v of the image's tokens -> the cross cache: p0 tokens an image, heads, images
    kv.epi = EPI_CROSSKV; kv.p1 = c.t_heads; kv.p2 = B;
    if (c.arch == CAP_ARCH_COCA) {
        TRY(run_coca_pool(m, B, nullptr, s));
        kv.p0 = m->Q;
        return gemm(m, s, "gemm_crosskv", m->xhat, m->E, m->ckv, m->cross, 0, OUT_T, B * m->Q, ACT_NONE, kv);
    }
    kv.p0 = m->NT;
    return gemm(m, s, "gemm_crosskv", m->emb_t, c.v_hidden, m->ckv, m->cross, 0, OUT_T, B * m->NT, ACT_NONE, kv);
}

// Rows of one beam search of the request.  A group search (num_beam_groups given): the reference's loop runs its groups one after
// the other on the SAME logits with only MinLength / RepetitionPenalty(1.0) as processors (coca_model.py:236-241: no
// HammingDiversity processor), every group starts from the same scores (:380-384), and finalize picks the best hypothesis over all
// groups of an image: the groups are identical searches of num_beams / num_beam_groups beams, and the result is that of ONE of
// them.  That one is what runs.
int beams_per_search(const CapGenerateArgs& a) { return a.num_beam_groups ? a.num_beams / a.num_beam_groups : a.num_beams; }

// BLIP / CoCa.  num_beams == 1 is the greedy loop (HF `_sample` with do_sample=False; CoCa: the reference's top-k(1) loop, coca.py:29),
// num_beams > 1 beam search (CoCa: its `_generate_beamsearch`, coca_model.py:335-482; length_penalty is the scorer's).  A group
// search runs as a BEAM search (the scorer's bookkeeping, no forced EOS) even with one beam per group.
// prompt_ids [prompt_rows, prompt_len] (greedy BLIP): every caption starts with these tokens; positions 0 .. prompt_len - 2 run as a
// prefill and the loop starts at t = prompt_len - 1, so the step outputs (out_step_logits, out_logprobs) are indexed from there.
int run_generate(Captioner* m, const CapGenerateArgs& a, hipStream_t s) {
    const CapConfig& c = m->c;
    const int B = a.B, K = beams_per_search(a), Lm = a.max_len;
    const int t0 = a.prompt_ids ? a.prompt_len - 1 : 0;
    const int R = B * K;
    const bool coca = c.arch == CAP_ARCH_COCA;
    const bool greedy = K == 1 && !a.num_beam_groups;
    TRY(zero_greedy_outputs(a, R, Lm - 1, s));
    TRY(run_image_side(m, a.pixels, a.pixel_fmt, B, s));
    Dec d = make_dec(m, B, K);
    // Row compaction (ops.h, RowMap): the greedy BLIP loop on the batch kernels, when nobody asked for per-step logits (their rows
    // are the batch's rows) and every position takes the fused self-attention (<= 32: the k / v append goes through map.live)
    const bool compact = greedy && c.arch == CAP_ARCH_BLIP && m->compaction && m->live && !a.out_step_logits && Lm - 1 <= 32 &&
                         R > SMALL_MAX_ROWS && m->decode_path != 2;
    m->last_compacted = compact ? 1 : 0;
    if (greedy) {
        if (a.prompt_ids) TRY(launch_init_prompt_seq(d.seq, d.finished, d.lens, R, Lm, a.prompt_ids, a.prompt_rows, a.prompt_len, c.vocab, c.pad, s));
        else hipLaunchKernelGGL(init_seq_kernel, dim3(64), dim3(256), 0, s, d.seq, d.finished, d.lens, R, Lm, c.bos, c.pad);
        if (compact) {
            d.map.live = m->live; d.map.n = m->n_live;
            TRY(launch_compact_rows(d.finished, R, m->live, m->n_live, s));
        }
    } else {
        TRY(launch_beam_init(d.beam, B, K, Lm, c.bos, c.pad, c.eos, s, coca ? BEAM_LEGACY_RAW : BEAM_HF_V5));
        hipLaunchKernelGGL(iota_rows_kernel, dim3(64), dim3(256), 0, s, d.anc, R, Lm);
    }
    CAP_HIP_CHECK(hipGetLastError());
    m->last_prefill_passes = 0;
    if (t0 > 0) {
        // the whole batch in one pass where the workspace holds it (CapConfig.max_prompt), else as many captions at a time as it does
        const int per = (int)std::min<size_t>((size_t)R, m->ws_rows / (size_t)t0);
        for (int c0 = 0; c0 < R; c0 += per) {
            TRY(run_prefill(m, d, c0, std::min(per, R - c0), t0, Lm, s));
            ++m->last_prefill_passes;
        }
    }
    for (int t = t0; t + 1 < Lm; ++t) {
        const int cur_len = t + 1;
        m->last_steps = t + 1;
        const int* tokens = greedy ? d.seq : beam_running_tokens_p(d.beam, B, K, Lm, cur_len & 1);
        const int* anc = greedy ? nullptr : d.anc + (size_t)(cur_len & 1) * R * Lm;
        // a forced small path (decode_path 2) takes every step of the call: validate_generate refused the request otherwise
        const bool small = m->decode_path != 1 && small_path_takes(m, d, t);
        m->last_path = small ? 2 : 1;
        TRY((small ? run_step_small : run_step)(m, d, tokens, Lm, t, K, anc, Lm, s));
        TRY(copy_step_logits(m, a, R, t - t0, s));
        ProfScope ps(m, s, greedy ? "greedy_select" : "beam_step", 0, (double)R * c.vocab * 4);
        if (greedy) {
            TRY(select_greedy_step(m, a, R, t - t0, Lm - 1, Lm, t, Lm, d.map, s));
            if (compact) TRY(launch_compact_rows(d.finished, R, m->live, m->n_live, s));
        } else {
            TRY(engine_beam_step(m, a, d.beam, d.logits, d.anc, B, K, Lm, cur_len, s));
        }
        bool done;
        TRY(poll_all_finished(m, t, Lm - 1, d.finished, R, greedy ? nullptr : beam_active_flag_p(d.beam, B, K, Lm), s, &done));
        if (done) break;
    }
    if (greedy) {
        hipLaunchKernelGGL(copy_i32_kernel, dim3(64), dim3(256), 0, s, d.seq, a.out_ids, (size_t)R * Lm);
        if (a.out_len) hipLaunchKernelGGL(copy_i32_kernel, dim3(4), dim3(256), 0, s, d.lens, a.out_len, (size_t)R);
        CAP_HIP_CHECK(hipGetLastError());
    } else {
        TRY(launch_beam_finalize(d.beam, B, K, Lm, a.out_ids, a.out_len, a.out_scores, s));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- teacher-forced scoring (BLIP)
// scored[n] = positions of caption n that have a target: lens[n] - 1 inside [0, L - 1] (an absent slot, lens 0, has none)
__global__ void score_counts_kernel(const int* __restrict__ lens, int* __restrict__ scored, int N, int L) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) scored[i] = min(max(lens[i] - 1, 0), L - 1);
}

struct ScoreArgs {
    const void* pixels; int pixel_fmt, B;
    const int *ids, *lens;      // int32 [B * C, L] / [B * C] (device)
    int C, L;
    float *out_tlp, *out_top; int *out_top_ids, *out_scored;   // [B * C, L - 1] x 3, [B * C]
};

// Captions a scoring pass of this handle takes at npos positions each: what its pass buffers and self-attention caches hold
// (BLIP-2: the caption pass has L - 2 rows per caption - the first token comes from the prompt pass - in buffers of max_batch x P rows)
size_t score_pass_captions(const Captioner* m, int L) {
    if (m->c.arch == CAP_ARCH_BLIP2)
        return L <= 2 ? (size_t)0x7fffffff : (size_t)m->c.max_batch * (m->c.num_query_tokens + 1) / (size_t)(L - 2);
    return std::min<size_t>((size_t)m->c.max_batch * m->c.max_beams, m->ws_rows / (size_t)(L - 1));
}
// Captions of the pass that starts at caption n0 of N, where a pass holds `fit`: whole images while one fits, else part of one image's
// captions (the result is a multiple of C, or below C).
int score_pass_size(size_t fit, int C, int N, int n0) {
    const int per = (int)std::min<size_t>(fit, (size_t)N);
    return per >= C ? std::min(per / C * C, N - n0) : std::min(per, (n0 / C + 1) * C - n0);
}
// A scoring call's outputs before its passes: zeros, and every caption's count of scored positions
int init_score_outputs(const ScoreArgs& a, hipStream_t s) {
    const int N = a.B * a.C;
    const size_t n = (size_t)N * (a.L - 1);
    TRY(launch_fill_f32(a.out_tlp, 0.f, n, s));
    TRY(launch_fill_f32(a.out_top, 0.f, n, s));
    TRY(launch_fill_i32(a.out_top_ids, 0, n, s));
    hipLaunchKernelGGL(score_counts_kernel, dim3((N + 255) / 256), dim3(256), 0, s, a.lens, a.out_scored, N, a.L);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

// log p(ids[n][j + 1] | image n / C, ids[n][0..j]) for every caption and position, with the row's log max softmax and arg-max: the image
// side once per image, then positions 0 .. L - 2 of the captions through the decoder as prefill passes (run_prefill: one read of every
// weight per pass, the C captions of an image sharing its cross K/V as beams do), the head of run_step over the pass's rows - as many
// at a time as the logits buffer holds - and launch_target_logprob on each slice.  Passes take whole images while one fits, else part
// of one image's captions: a caption's rows are computed by row-wise kernels and attend their own caption's positions only, so the
// chunking changes no bits.  Rows behind a caption's end are computed on whatever ids the caller left there (clamped) and come out
// as zeros: attention is causal, so they reach no row that is reported.
int run_score(Captioner* m, const ScoreArgs& a, hipStream_t s) {
    const CapConfig& c = m->c;
    const int N = a.B * a.C, L = a.L, npos = L - 1, W = m->dec.W;
    const size_t e = m->esz;
    TRY(init_score_outputs(a, s));
    TRY(run_image_side(m, a.pixels, a.pixel_fmt, a.B, s));
    m->last_score_passes = 0;
    for (int n0 = 0; n0 < N;) {
        const int nc = score_pass_size(score_pass_captions(m, L), a.C, N, n0);
        Dec d = make_dec(m, a.B, 1);       // the cross K/V are packed for the call's images; the caches hold this pass's captions
        d.R = nc;
        TRY(launch_init_prompt_seq(d.seq, d.finished, d.lens, nc, L, a.ids + (size_t)n0 * L, nc, L, c.vocab, c.pad, s));
        TRY(run_prefill(m, d, 0, nc, npos, L, s, std::min(nc, a.C) * npos, n0 / a.C));
        const int Rp = nc * npos;
        for (int r0 = 0; r0 < Rp; r0 += (int)m->head_rows) {
            const int hr = std::min((int)m->head_rows, Rp - r0);
            const char* x_t = (const char*)d.dx_t + (size_t)r0 * W * e;
            TRY(run_head(m, s, d, (void*)x_t, nullptr, hr, nullptr));
            ProfScope ps(m, s, "target_logprob", 0, 2.0 * hr * c.vocab * 4);
            TRY(launch_target_logprob(d.logits, m->ldl, c.vocab, hr, r0, npos, a.ids + (size_t)n0 * L + 1, L, a.out_scored + n0,
                                      a.out_tlp + (size_t)n0 * npos, a.out_top + (size_t)n0 * npos, a.out_top_ids + (size_t)n0 * npos, npos, s));
        }
        ++m->last_score_passes;
        n0 += nc;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- BLIP-2: the OPT decoder and the runs
// ---- The OPT decoder (pre-LN blocks: what follows a residual add is always a LayerNorm).
// One projection over `rows` rows, left for a consumer to finish: in place (ln == false: bias + act -> out_t, of type out_dt -
// split mode: fp32 for q|k|v, G8 for a GEMM operand) or as *S_out slice sums in m->dpart for the reduce + LayerNorm consumer.
//   int8 weights (L.w = fragment-ordered bytes, L.scale = row scales), tiled: a batch's prompt pass, B x 33 rows, is a GEMM proper.
//     The matrix is unpacked into a row-major bf16 scratch of its INTEGERS (exact), multiplied by the tiled kernel into fp32 and
//     the row scales applied to that output (S = 1): (A . q^T) * scale + bias as in the weight-streaming kernel, the sums in the
//     tiled kernel's order.  Measured at 32 crops (us per fc1 GEMM): 365 on the rows-walking weight-stream kernel, ~135 here.
//   int8 weights otherwise: the weight-streaming kernel, which takes any row count (further row groups re-read a unit's bytes
//     from the XCD's L2).
//   bf16 at a shape the weight-streaming kernel takes: that kernel - at a few dozen rows every GEMM is a weight stream, so K is
//     split over blocks (all slabs of a block in flight at once).  Otherwise the tiled split-K GEMM with a reduce kernel.
// Apart from `tiled` the choice depends on dtype and (N, K) only - never on the row count.
int opt_gemm(Captioner* m, hipStream_t s, const char* tag, const void* A, const Linear& L, GemmAct act, void* out_t, int rows, bool ln,
             int* S_out, int out_dt, bool tiled) {
    const int N = L.N, K = L.K;
    const float* bias = ln ? nullptr : L.b;       // (the reduce + LayerNorm consumer adds it)
    if (m->wq8 && !tiled) {
        const int S8 = skinny_i8_plan(N, K, !ln);
        ProfScope ps(m, s, tag, 2.0 * rows * N * K,
                     (double)rows * K * 2 + (double)N * K + (ln ? (double)S8 * rows * N * 4 : (double)rows * N * 2));
        *S_out = S8;
        return launch_gemm_skinny_i8(A, K, L.w, L.scale, bias, act, out_t, N, ln ? m->dpart : nullptr, rows, N, K, s) == S8 ? 0 : -1;
    }
    const int S = !m->wq8 && m->dt == CAP_DT_BF16 ? skinny_plan(N, K, !ln) : 0;
    if (S >= 1) {
        ProfScope ps(m, s, tag, 2.0 * rows * N * K,
                     ((double)rows * K + (double)N * K) * 2 + (ln ? (double)S * rows * N * 4 : (double)rows * N * 2));
        *S_out = S;
        return launch_gemm_skinny(A, K, L.w, K, bias, act, out_t, N, ln ? m->dpart : nullptr, rows, N, K, s) == S ? 0 : -1;
    }
    if (m->wq8) {
        TRY(launch_dequant_i8_rowmajor(L.w, m->w8_scratch, N, K, s));
        TRY(gemm(m, s, tag, A, K, linear_over(m->w8_scratch, N, K), m->dpart, N, OUT_F32, rows));
        TRY(launch_scale_cols(m->dpart, L.scale, rows, N, s));
        *S_out = 1;
    } else {
        TRY(gemm_partial(m, s, tag, A, L, m->dpart, rows, 8, S_out));
    }
    if (!ln) TRY(launch_reduce_bias_act(out_dt, m->dpart, *S_out, bias, out_t, rows, N, act, s));
    return 0;
}

// Self-attention of one layer over the fused q|k|v rows in oqkv -> octx, the new K/V rows into the layer's caches.  The prompt
// (L positions, nothing cached): causal attention over the rows themselves (MFMA kernel for bf16 heads wider than 64).  A step
// (L == 1): the new position against the `past` cached ones.
// What the B rows-of-L are says OptRows, the three key sources of attention.hip's OPT wave walk:
//   OWN: every row has its own cache row (the greedy call).
//   BEAMS: the caches are those of B x K rows, row = image * K + beam.  The prompt pass runs over the B images and leaves image b's
//     positions in the cache of row b * K, for the K rows of the image (no table yet); the steps run over the B * K rows, each reading
//     the generated positions from the rows its ancestry table names (opt_beam_decode_attention).
//   CAPTIONS (teacher-forced scoring, run_score_blip2): the rows are captions cap0 .. cap0 + B - 1 of a request with C captions per
//     image, their L new positions behind the P positions the prompt pass left in the cache of row image = caption / C; the caches
//     are read only (opt_prefix_attention).
struct OptRows {
    enum Kind { OWN, BEAMS, CAPTIONS } kind = OWN;
    int K = 1; const int* anc = nullptr; int anc_ld = 0;    // BEAMS: anc [B * K, anc_ld], the step's table from the first generated position on
    int C = 0, cap0 = 0;                                    // CAPTIONS
    static OptRows beams(int K, const int* anc = nullptr, int anc_ld = 0) { return {BEAMS, K, anc, anc_ld}; }
    static OptRows captions(int C, int cap0) { return {CAPTIONS, 1, nullptr, 0, C, cap0}; }
};
int opt_attention(Captioner* m, const OLayer& Ly, int B, int L, int past, hipStream_t s, const OptRows& rw) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden, H = c.t_heads, hd = T / H, P = c.num_query_tokens + 1, Lmax = P + c.max_len;
    if (rw.kind == OptRows::CAPTIONS) {
        ProfScope ps(m, s, "opt_prefix_attn", 4.0 * B * H * (double)L * (P + L) * hd, 2.0 * B * (P + L) * T * m->esz);
        return launch_opt_prefix_attention(m->dt, m->oqkv, Ly.kc, Ly.vc, m->octx, B, L, rw.cap0, rw.C, nullptr, T, H, Lmax, P, s, m->gdt);
    }
    if (L > 1 && past != 0) { cap_set_error("opt_attention: %d new positions behind a cached prefix (%d) are not built", L, past); return -1; }
    if (L > 1) TRY(launch_kv_append(m->dt, m->oqkv, Ly.kc, Ly.vc, B, L, T, Lmax, 0, s, rw.K));
    ProfScope ps(m, s, "opt_attn", 4.0 * B * H * (double)L * (past + L) * hd, 2.0 * B * (past + L) * T * m->esz);
    if (L > 1) return launch_vit_attention(m->dt, m->oqkv, m->octx, B, L, H, 0, s, hd, 1, m->gdt);
    if (rw.kind == OptRows::BEAMS)     // (cap_create holds BLIP-2's head widths to what the kernel takes)
        return launch_opt_beam_decode_attention(m->dt, m->oqkv, Ly.kc, Ly.vc, m->octx, B / rw.K, rw.K, T, H, Lmax, P, past, rw.anc,
                                                rw.anc_ld, s, m->gdt);
    if (hd % 8 == 0 && hd <= 128) return launch_opt_decode_attention(m->dt, m->oqkv, Ly.kc, Ly.vc, m->octx, B, T, H, Lmax, past, s, m->gdt);
    TRY(launch_kv_append(m->dt, m->oqkv, Ly.kc, Ly.vc, B, 1, T, Lmax, past, s));
    return launch_generic_attention(m->dt, m->oqkv, 3 * T, 3 * T, Ly.kc, T, (long)Lmax * T, Ly.vc, T, (long)Lmax * T, m->octx, T, T, B, 1, past + 1,
                                    H, hd, past, s, m->gdt);
}

// The decoder layers over L new positions per row behind `past` cached ones (x = ox [B * L, T] fp32 with the positions added,
// oh_t = LayerNorm_1 of layer 0 already applied), then the tied LM head (bf16, no bias) on each row's last new position ->
// m->logits.  Every decode step (L = 1), and the prompt pass with int8 weights: up to kI8SkinnyPromptCrops crops its rows go
// through the step's weight streams (a one-crop prompt is 33 rows: a weight stream too), beyond through the tiled GEMM.  The
// consumers finish the projections' sums - bias (+ ReLU) -> T for q|k|v and fc1; bias + residual + the NEXT LayerNorm (the
// final one on the last layer, over every row) for out_proj and fc2.
// rw (opt_attention) - BEAMS: the prompt pass leaves image b's logits in row b * K of m->logits.
// CAPTIONS: the rows are captions' new positions behind their images' cached prompts; no head here - the final LayerNorm of EVERY
// row is left in oh_t for the caller's vocabulary GEMM over all of them.  Its rows take the weight streams up to the row count of
// kI8SkinnyPromptCrops prompts, the tiled GEMM beyond, as the prompt pass does.
int run_opt(Captioner* m, int B, int L, int past, hipStream_t s, const OptRows& rw) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden, R = B * L;
    const bool sc = rw.kind == OptRows::CAPTIONS;
    const bool tiled = sc ? R > kI8SkinnyPromptCrops * (c.num_query_tokens + 1) : L > 1 && B > kI8SkinnyPromptCrops;
    int S = 1;
    for (int i = 0; i < c.t_layers; ++i) {
        const OLayer& Ly = m->ol[i];
        const bool last = i + 1 == c.t_layers;
        TRY(opt_gemm(m, s, "opt_gemm_qkv", m->oh_t, Ly.qkv, ACT_NONE, m->oqkv, R, false, &S, m->dt, tiled));
        TRY(opt_attention(m, Ly, B, L, past, s, rw));
        TRY(opt_gemm(m, s, "opt_gemm_o", m->octx, Ly.o, ACT_NONE, nullptr, R, true, &S, m->gdt, tiled));
        TRY(launch_reduce_layernorm(m->gdt, m->dpart, S, Ly.o.b, m->ox, Ly.ln2.g, Ly.ln2.b, c.t_eps, m->oh_t, nullptr, m->ox, R, T, s, true));
        TRY(opt_gemm(m, s, "opt_gemm_f1", m->oh_t, Ly.f1, ACT_RELU, m->off, R, false, &S, m->gdt, tiled));
        TRY(opt_gemm(m, s, "opt_gemm_f2", m->off, Ly.f2, ACT_NONE, nullptr, R, true, &S, m->gdt, tiled));
        const Norm& next = last ? m->o_lnf : m->ol[i + 1].ln1;
        TRY(launch_reduce_layernorm(m->gdt, m->dpart, S, Ly.f2.b, m->ox, next.g, next.b, c.t_eps, m->oh_t, nullptr, m->ox, R, T, s, true));
    }
    if (sc) return 0;
    return gemm(m, s, "opt_gemm_vocab", (const char*)m->oh_t + (size_t)(L - 1) * T * m->esz, L * T, m->o_head, m->logits,
                (L > 1 ? rw.K : 1) * m->ldl, OUT_F32, B);
}

// A pass (L > 1) with plain weights (f32 / f32s / bf16): B * L rows are GEMMs proper, so bias and residual ride the tiled GEMM's
// epilogue, every sub-block opens with its own LayerNorm, and the final one covers each row's last position only.
// CAPTIONS: the same chain over captions' new positions behind the cached prompts; the final LayerNorm then covers EVERY row and
// the head is the caller's (run_opt).
int run_opt_prompt_plain(Captioner* m, int B, int L, int past, hipStream_t s, const OptRows& rw) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden, G = c.t_ffn, R = B * L;
    for (const OLayer& Ly : m->ol) {
        TRY(launch_layernorm(m->gdt, m->ox, T, Ly.ln1.g, Ly.ln1.b, c.t_eps, m->oh_t, nullptr, R, T, s));
        // (split mode: q | k | v for the attention kernels and the caches are fp32)
        TRY(gemm(m, s, "opt_gemm_qkv", m->oh_t, T, Ly.qkv, m->oqkv, 3 * T, m->attn_out(), R));
        TRY(opt_attention(m, Ly, B, L, past, s, rw));
        TRY(gemm(m, s, "opt_gemm_o", m->octx, T, Ly.o, m->ox, T, OUT_F32, R, ACT_NONE, GemmOpt::residual(m->ox)));
        TRY(launch_layernorm(m->gdt, m->ox, T, Ly.ln2.g, Ly.ln2.b, c.t_eps, m->oh_t, nullptr, R, T, s));
        TRY(gemm(m, s, "opt_gemm_f1", m->oh_t, T, Ly.f1, m->off, G, OUT_T, R, ACT_RELU));
        TRY(gemm(m, s, "opt_gemm_f2", m->off, G, Ly.f2, m->ox, T, OUT_F32, R, ACT_NONE, GemmOpt::residual(m->ox)));
    }
    if (rw.kind == OptRows::CAPTIONS) return launch_layernorm(m->gdt, m->ox, T, m->o_lnf.g, m->o_lnf.b, c.t_eps, m->oh_t, nullptr, R, T, s);
    TRY(launch_layernorm(m->gdt, m->ox + (size_t)(L - 1) * T, L * T, m->o_lnf.g, m->o_lnf.b, c.t_eps, m->oh_t, nullptr, B, T, s));
    return gemm(m, s, "opt_gemm_vocab", m->oh_t, T, m->o_head, m->logits, rw.K * m->ldl, OUT_F32, B);
}

// The layers over a pass of B x L rows whose inputs are in ox: the prompt (nothing cached), or captions' new positions behind it.
// int8 weights walk as the steps do (run_opt, behind layer 0's first LayerNorm), plain ones as GEMMs proper.
int run_opt_pass(Captioner* m, int B, int L, hipStream_t s, const OptRows& rw) {
    const CapConfig& c = m->c;
    const int past = rw.kind == OptRows::CAPTIONS ? c.num_query_tokens + 1 : 0;
    if (!m->wq8) return run_opt_prompt_plain(m, B, L, past, s, rw);
    TRY(launch_layernorm(m->gdt, m->ox, c.t_hidden, m->ol[0].ln1.g, m->ol[0].ln1.b, c.t_eps, m->oh_t, nullptr, B * L, c.t_hidden, s));
    return run_opt(m, B, L, past, s, rw);
}

// One decode step over B rows: column `col` of tokens [B, ld] is the token at sequence position `at`, the `at` positions before it cached
int run_opt_step(Captioner* m, const int* tokens, int ld, int col, int at, int B, hipStream_t s, const OptRows& rw) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden;
    TRY(launch_opt_token_inputs(tokens, ld, col, m->o_tok, m->o_pos, m->ox, B, T, c.vocab, s, at));
    TRY(launch_layernorm(m->gdt, m->ox, T, m->ol[0].ln1.g, m->ol[0].ln1.b, c.t_eps, m->oh_t, nullptr, B, T, s));
    return run_opt(m, B, 1, at, s, rw);
}

// row b * K of logits [B * K, ld] -> the other K - 1 rows of image b
__global__ void beam_rows_from_first_kernel(float* logits, int ld, int B, int K, int V) {
    const size_t n = (size_t)B * (K - 1) * V;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / V, c = i - r * V, b = r / (K - 1), k = 1 + r % (K - 1);
        logits[(b * K + k) * ld + c] = logits[b * K * ld + c];
    }
}

// The beam search behind the prompt pass (HF `_beam_search` under Blip2ForConditionalGeneration.generate(num_beams = K)): the prompt
// pass ran once per IMAGE and left its positions in the caches of rows b * K and its logits in rows b * K of m->logits; HF runs it on
// K identical rows per image, so step 0 takes K copies of those logits (beam.hip starts beams 1 .. K - 1 at -1e9).
// The bookkeeping is beam.hip's in HF-v5 mode over max_len + 1 token columns, column 0 = BOS.  HF subtracts decoder_prompt_len (the
// query tokens + BOS) from every length it uses: its length penalty's cur_len + 1 - prompt and its early-stop heuristic's
// max_length - prompt count new tokens, and so does beam.hip's cur_len + 1 - 1 with BOS as the only column ahead of them (pinned by
// tests/golden/blip2_tiny_beam.npz).  Column c's token is sequence position P - 1 + c; the ancestry table's entry c names the row
// that wrote that position, so the attention takes the table from column 1 (the first generated position, P) on.
int run_beams_blip2(Captioner* m, const CapGenerateArgs& a, hipStream_t s) {
    const CapConfig& c = m->c;
    const int B = a.B, K = a.num_beams, R = B * K, max_len = a.max_len, Lb = max_len + 1, P = c.num_query_tokens + 1;
    TRY(launch_beam_init(m->beam, B, K, Lb, c.bos, c.pad, c.eos, s, BEAM_HF_V5));
    hipLaunchKernelGGL(iota_rows_kernel, dim3(64), dim3(256), 0, s, m->anc, R, Lb);
    hipLaunchKernelGGL(beam_rows_from_first_kernel, dim3(256), dim3(256), 0, s, m->logits, m->ldl, B, K, c.vocab);
    CAP_HIP_CHECK(hipGetLastError());
    for (int t = 0; t < max_len; ++t) {
        const int cur_len = t + 1, nxt = (cur_len & 1) ^ 1;      // the step fills column cur_len and leaves its state in parity nxt
        m->last_steps = t + 1;
        TRY(copy_step_logits(m, a, R, t, s));
        {
            ProfScope ps(m, s, "beam_step", 0, (double)R * c.vocab * 4);
            TRY(engine_beam_step(m, a, m->beam, m->logits, m->anc, B, K, Lb, cur_len, s));
        }
        if (t + 1 == max_len) break;
        {
            bool done;
            TRY(poll_all_finished(m, t, max_len, nullptr, R, beam_active_flag_p(m->beam, B, K, Lb), s, &done));
            if (done) break;
        }
        const OptRows rows = OptRows::beams(K, m->anc + (size_t)nxt * R * Lb + 1, Lb);
        TRY(run_opt_step(m, beam_running_tokens_p(m->beam, B, K, Lb, nxt), Lb, cur_len, P - 1 + cur_len, R, s, rows));
    }
    // the best hypothesis of every image with its BOS column, then the new tokens alone as the greedy loop returns them
    TRY(launch_beam_finalize(m->beam, B, K, Lb, m->seq, m->lens, a.out_scores, s));
    hipLaunchKernelGGL(copy_new_tokens_kernel, dim3(64), dim3(256), 0, s, m->seq, Lb, 1, m->lens, a.out_ids, a.out_len, B, max_len);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

// BLIP-2's image side: encoder, the Q-Former's caption pass, the language projection -> m->lm_proj fp32 [B * num_query_tokens, T]
int run_blip2_image_side(Captioner* m, const void* pixels, int fmt, int B, hipStream_t s) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden, nq = c.num_query_tokens;
    TRY(run_encoder(m, pixels, fmt, B, nullptr, s));
    TRY(run_qformer(m, kCaptionPass, B, nq, 0, nullptr, nullptr, s));
    return gemm(m, s, "b2_gemm_lproj", m->qr.x_t, c.q_hidden, m->lproj, m->lm_proj, T, OUT_F32, B * nq);
}

// BLIP-2's front half over the B images of a call: the image side (or the import of its state), and the prompt pass
// over the P = query tokens + BOS positions, which leaves image b's prompt in cache row b * K and its BOS logits in row b * K of
// m->logits (K > 1: for the K rows of a beam search).
int run_blip2_prompt(Captioner* m, const void* pixels, int fmt, int B, int K, hipStream_t s) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden, nq = c.num_query_tokens;
    if (fmt == CAP_PIX_IMAGE_STATE) TRY(import_image_state(m, pixels, B, s));
    else TRY(run_blip2_image_side(m, pixels, fmt, B, s));
    TRY(launch_opt_prefill_inputs(m->lm_proj, m->o_tok, m->o_pos, m->ox, B, nq, T, c.bos, s));
    return run_opt_pass(m, B, nq + 1, s, K > 1 ? OptRows::beams(K) : OptRows());
}

// HF Blip2ForConditionalGeneration.generate, greedy: out_ids [B, max_len] = the new tokens (pad after EOS), out_len [B] =
// their count incl. EOS, out_step_logits [max_len, B, vocab]; the optional greedy outputs have max_len columns.
// num_beams > 1: the same front half over the B images, then run_beams_blip2 (out_scores = sequences_scores, out_step_logits
// [max_len, B * num_beams, vocab]).
int run_generate_blip2(Captioner* m, const CapGenerateArgs& a, hipStream_t s) {
    const CapConfig& c = m->c;
    const int B = a.B, max_len = a.max_len, P = c.num_query_tokens + 1, Lmax = P + c.max_len;
    TRY(zero_greedy_outputs(a, B, max_len, s));
    TRY(run_blip2_prompt(m, a.pixels, a.pixel_fmt, B, a.num_beams, s));
    if (a.num_beams > 1) return run_beams_blip2(m, a, s);
    hipLaunchKernelGGL(init_seq_kernel, dim3(64), dim3(256), 0, s, m->seq, m->finished, m->lens, B, Lmax, c.bos, c.pad);
    CAP_HIP_CHECK(hipGetLastError());
    for (int t = 0; t < max_len; ++t) {
        m->last_steps = t + 1;
        // token of position P + t; a row finishes on EOS or at P + max_len tokens (greedy_select's `t` is the last filled index)
        TRY(copy_step_logits(m, a, B, t, s));
        TRY(select_greedy_step(m, a, B, t, max_len, Lmax, P - 1 + t, P + max_len, RowMap(), s));
        if (t + 1 == max_len) break;
        {
            bool done;
            TRY(poll_all_finished(m, t, max_len, m->finished, B, nullptr, s, &done));
            if (done) break;
        }
        TRY(run_opt_step(m, m->seq, Lmax, P + t, P + t, B, s, OptRows()));
    }
    hipLaunchKernelGGL(copy_new_tokens_kernel, dim3(64), dim3(256), 0, s, m->seq, Lmax, P, m->lens, a.out_ids, a.out_len, B, max_len);
    CAP_HIP_CHECK(hipGetLastError());
    return 0;
}

// Teacher-forced scoring under BLIP-2 (cap_score_captions): the front half once per IMAGE (run_blip2_prompt), then
//   entry 0 of every caption from its image's BOS logits (launch_target_logprob, one logits row shared by the image's C captions),
//   the caption pass: the n = L - 2 tokens behind BOS of as many captions as the pass rows hold (max_batch x P: what the prompt
//     pass is sized for), caption-major, behind the cached prompts (opt_prefix_attention; nothing is appended to the caches), the
//     final LayerNorm over every row, and the tied head over those rows in slices of the logits buffer, each reduced at once.
// Passes take whole images while one fits, else part of one image's captions.
int run_score_blip2(Captioner* m, const ScoreArgs& a, hipStream_t s) {
    const CapConfig& c = m->c;
    const int T = c.t_hidden, P = c.num_query_tokens + 1, C = a.C, L = a.L, N = a.B * C, npos = L - 1, n = L - 2;
    const size_t e = m->esz;
    TRY(init_score_outputs(a, s));
    TRY(run_blip2_prompt(m, a.pixels, a.pixel_fmt, a.B, 1, s));
    {
        ProfScope ps(m, s, "target_logprob", 0, 2.0 * N * c.vocab * 4);
        TRY(launch_target_logprob(m->logits, m->ldl, c.vocab, N, 0, 1, a.ids + 1, L, a.out_scored, a.out_tlp, a.out_top, a.out_top_ids, npos, s, 0, C));
    }
    m->last_score_passes = 0;
    if (n < 1) return 0;
    const int head_rows = c.max_batch * c.max_beams;
    for (int n0 = 0; n0 < N;) {
        const int nc = score_pass_size(score_pass_captions(m, L), C, N, n0);
        const int Rp = nc * n;
        TRY(launch_opt_caption_inputs(a.ids + (size_t)n0 * L + 1, L, nc, n, P, m->o_tok, m->o_pos, m->ox, T, c.vocab, s));
        TRY(run_opt_pass(m, nc, n, s, OptRows::captions(C, n0)));
        for (int r0 = 0; r0 < Rp; r0 += head_rows) {
            const int hr = std::min(head_rows, Rp - r0);
            TRY(gemm(m, s, "opt_gemm_vocab", (const char*)m->oh_t + (size_t)r0 * T * e, T, m->o_head, m->logits, m->ldl, OUT_F32, hr));
            ProfScope ps(m, s, "target_logprob", 0, 2.0 * hr * c.vocab * 4);
            TRY(launch_target_logprob(m->logits, m->ldl, c.vocab, hr, r0, n, a.ids + (size_t)n0 * L + 2, L, a.out_scored + n0,
                                      a.out_tlp + (size_t)n0 * npos + 1, a.out_top + (size_t)n0 * npos + 1, a.out_top_ids + (size_t)n0 * npos + 1, npos,
                                      s, 1, 1));
        }
        ++m->last_score_passes;
        n0 += nc;
    }
    return 0;
}

}  // namespace

// Everything a handle owns - also the exit of every failed cap_create (streams and events included).
static void release_captioner(Captioner* m) {
    for (auto& r : m->prof_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (const ArenaAlloc& a : m->allocs) (void)hipFree(a.p);
    if (m->ws && m->ws->refs.fetch_sub(1) == 1) {        // last handle on these weights
        for (void* p : m->ws->ptrs) (void)hipFree(p);
        delete m->ws;
    }
    if (m->stage) (void)hipFree(m->stage);
    if (m->absmax_dev) (void)hipFree(m->absmax_dev);
    if (m->host_flag) (void)hipHostFree(m->host_flag);
    if (m->ban_bits) (void)hipFree(m->ban_bits);
    if (m->ban_multi) (void)hipFree(m->ban_multi);
    delete m;
}

// ================================================================================================ C ABI
extern "C" {

const char* cap_last_error(void) { return g_err; }
int cap_version(void) { return 1; }

static int create_impl(const CapConfig* cfg, Captioner* share, CapHandle* out) {
    if (!cfg || !out) { cap_set_error("cap_create: null argument"); return -1; }
    if (cfg->struct_size != (int)sizeof(CapConfig)) {
        cap_set_error("cap_create: CapConfig size mismatch (caller %d, library %d)", cfg->struct_size, (int)sizeof(CapConfig));
        return -1;
    }
    if (cfg->arch != CAP_ARCH_BLIP && cfg->arch != CAP_ARCH_COCA && cfg->arch != CAP_ARCH_MINILM && cfg->arch != CAP_ARCH_BLIP2 &&
        cfg->arch != CAP_ARCH_CLIP && cfg->arch != CAP_ARCH_BLIP2_ITM) {
        cap_set_error("cap_create: unknown arch %d", cfg->arch);
        return -1;
    }
    if (cfg->compute_dtype != CAP_F32 && cfg->compute_dtype != CAP_BF16 && cfg->compute_dtype != CAP_F32_SPLIT) {
        cap_set_error("cap_create: unknown dtype");
        return -1;
    }
    // (the post-LN helpers the sentence encoder shares with the Q-Former rely on this: with dt == gdt their m->gdt is its m->dt)
    if (cfg->compute_dtype == CAP_F32_SPLIT && cfg->arch == CAP_ARCH_MINILM) {
        cap_set_error("cap_create: CAP_F32_SPLIT is built for the captioner architectures (the sentence encoder takes CAP_F32 or CAP_BF16)");
        return -1;
    }
    const bool text_only = cfg->arch == CAP_ARCH_MINILM;
    if (text_only) {
        const int hd = cfg->t_heads > 0 ? cfg->t_hidden / cfg->t_heads : 0;
        if ((hd != 32 && hd != 64) || hd * cfg->t_heads != cfg->t_hidden || cfg->t_hidden % 64 || cfg->t_ffn % 64 ||
            cfg->t_hidden > 1024 || cfg->t_layers < 1 || cfg->max_batch < 1 || cfg->max_len < 1 || cfg->max_len > cfg->max_pos ||
            cfg->vocab < 1) {
            cap_set_error("cap_create: sentence encoder needs head_dim 32 or 64, widths multiple of 64 (hidden <= 1024), "
                          "1 <= max_len <= max_pos");
            return -1;
        }
        if (2 * cfg->max_len * hd * 4 > TEXT_ATTENTION_MAX_LDS) {      // what launch_text_attention takes: refused here, not at the first long sentence
            cap_set_error("cap_create: sentence encoder max_len %d is beyond the %d tokens its attention kernel holds in LDS at head_dim %d",
                          cfg->max_len, TEXT_ATTENTION_MAX_LDS / (8 * hd), hd);
            return -1;
        }
    } else if (cfg->arch == CAP_ARCH_CLIP) {
        if (cfg->v_heads < 1 || cfg->t_heads < 1 || cfg->v_hidden != cfg->v_heads * 64 || cfg->t_hidden != cfg->t_heads * 64 ||
            cfg->v_hidden > 1024 || cfg->t_hidden > 1024 || cfg->v_mlp % 64 || cfg->t_ffn % 64 || cfg->v_mlp < 64 || cfg->t_ffn < 64 ||
            cfg->v_layers < 1 || cfg->t_layers < 1 || cfg->patch_size < 1 || cfg->image_size % cfg->patch_size ||
            cfg->embed_dim < 1 || cfg->embed_dim > 1024 || cfg->vocab < 1 || cfg->max_batch < 1 || cfg->max_len < 1 ||
            cfg->max_len > cfg->max_pos) {
            cap_set_error("cap_create: CLIP needs head_dim 64 in both towers (widths <= 1024), MLP widths multiple of 64, "
                          "1 <= embed_dim <= 1024 and 1 <= max_len <= max_pos");
            return -1;
        }
        if (cfg->hidden_act != CAP_ACT_QUICK_GELU && cfg->hidden_act != CAP_ACT_GELU) {
            cap_set_error("cap_create: CLIP hidden_act %d is neither CAP_ACT_QUICK_GELU (0) nor CAP_ACT_GELU (1)", cfg->hidden_act);
            return -1;
        }
    } else if (cfg->arch == CAP_ARCH_BLIP2_ITM) {
        const int vhd = cfg->v_heads > 0 ? cfg->v_hidden / cfg->v_heads : 0;
        if (vhd < 8 || vhd > 128 || vhd % 8 || vhd * cfg->v_heads != cfg->v_hidden || cfg->v_hidden % 64 || cfg->v_mlp % 64 || cfg->v_mlp < 64 ||
            cfg->v_layers < 1 || cfg->patch_size < 1 || cfg->image_size % cfg->patch_size || cfg->q_heads < 1 ||
            cfg->q_hidden != cfg->q_heads * 64 || cfg->q_hidden > 1024 || cfg->q_ffn % 64 || cfg->q_ffn < 64 || cfg->q_layers < 1 ||
            cfg->q_cross_freq < 1 || cfg->num_query_tokens < 1 || cfg->num_query_tokens > 32 || cfg->embed_dim < 1 ||
            cfg->embed_dim > 1024 || cfg->vocab < 1 || cfg->max_batch < 1 || cfg->max_len < 1 || cfg->max_len > 32 ||
            cfg->max_len > cfg->max_pos) {
            cap_set_error("cap_create: the BLIP-2 image-text scorer needs a ViT head dim that is a multiple of 8 (<= 128), Q-Former heads of "
                          "64 (width <= 1024), widths multiple of 64, 1..32 query tokens, 1 <= embed_dim <= 1024 and "
                          "1 <= max_len <= min(max_pos, 32)");
            return -1;
        }
        if (cfg->weight_int8) { cap_set_error("cap_create: the BLIP-2 image-text scorer has no int8 weights (CAP_F32, CAP_F32_SPLIT or CAP_BF16)"); return -1; }
    } else if (cfg->arch == CAP_ARCH_BLIP2) {
        auto hd_ok = [](int w, int h) { return h > 0 && w % h == 0 && (w / h) % 8 == 0 && w / h >= 8 && w / h <= 128; };
        if (!hd_ok(cfg->v_hidden, cfg->v_heads) || !hd_ok(cfg->q_hidden, cfg->q_heads) || !hd_ok(cfg->t_hidden, cfg->t_heads) ||
            cfg->v_hidden % 64 || cfg->v_mlp % 64 || cfg->q_hidden % 64 || cfg->q_ffn % 64 || cfg->t_hidden % 64 || cfg->t_ffn % 64 ||
            cfg->t_hidden > 256 * 12 || cfg->image_size % cfg->patch_size || cfg->q_layers < 1 || cfg->q_cross_freq < 1 ||
            cfg->num_query_tokens < 1 || cfg->max_batch < 1 || cfg->max_beams < 1 || cfg->max_beams > 8 || cfg->max_len < 1 ||
            cfg->num_query_tokens + 1 + cfg->max_len > cfg->max_pos) {
            cap_set_error("cap_create: BLIP-2 needs head dims that are multiples of 8 (<= 128), widths multiple of 64 (OPT hidden <= 3072), "
                          "1 <= max_beams <= 8 and num_query_tokens + 1 + max_len <= max_pos");
            return -1;
        }
        if (cfg->num_query_tokens + 1 + cfg->max_len > OPT_DECODE_MAX_KEYS) {      // launch_opt_decode_attention's limit: refused here, not mid-generation
            cap_set_error("cap_create: BLIP-2 num_query_tokens + 1 + max_len = %d is beyond the %d cached positions the decode-step attention "
                          "kernel takes", cfg->num_query_tokens + 1 + cfg->max_len, OPT_DECODE_MAX_KEYS);
            return -1;
        }
    } else {
        if (cfg->arch == CAP_ARCH_COCA) {
            const int hd = cfg->pool_heads > 0 ? cfg->embed_dim / cfg->pool_heads : 0;
            if (cfg->embed_dim != cfg->t_hidden || cfg->pool_queries < 2 || cfg->mm_layers < 1 || (hd != 64 && hd != 96) ||
                hd * cfg->pool_heads != cfg->embed_dim) {
                cap_set_error("cap_create: CoCa needs embed_dim == t_hidden, pooler head_dim 64 or 96, mm_layers >= 1");
                return -1;
            }
        }
        if (cfg->v_hidden != cfg->v_heads * 64 || cfg->t_hidden != cfg->t_heads * 64) {
            cap_set_error("cap_create: head_dim must be 64 (v %d/%d, t %d/%d)", cfg->v_hidden, cfg->v_heads, cfg->t_hidden, cfg->t_heads);
            return -1;
        }
        if (cfg->image_size % cfg->patch_size || cfg->max_batch < 1 || cfg->max_beams < 1 || cfg->max_beams > 8 ||
            cfg->max_len < 2 || cfg->max_len > cfg->max_pos) {
            cap_set_error("cap_create: bad geometry/capacity");
            return -1;
        }
        if (cfg->v_hidden % 64 || cfg->v_mlp % 64 || cfg->t_ffn % 64) { cap_set_error("cap_create: widths must be multiples of 64"); return -1; }
    }
    if (cfg->max_prompt != 0 && (cfg->arch != CAP_ARCH_BLIP || cfg->max_prompt < 2 || cfg->max_prompt > CAP_MAX_PROMPT)) {
        cap_set_error("cap_create: max_prompt %d - prompt capacity is CAP_ARCH_BLIP's, 0 (none) or 2 .. %d tokens (BOS included)",
                      cfg->max_prompt, CAP_MAX_PROMPT);
        return -1;
    }
    if (cfg->max_score_rows != 0 && (cfg->arch != CAP_ARCH_BLIP || cfg->max_score_rows < 0)) {
        cap_set_error("cap_create: max_score_rows %d - scoring capacity is CAP_ARCH_BLIP's, 0 (none) or a row count", cfg->max_score_rows);
        return -1;
    }
    if (cfg->weight_int8) {
        const int T = cfg->t_hidden, G = cfg->t_ffn;
        if (cfg->weight_int8 != 1 || cfg->arch != CAP_ARCH_BLIP2 || cfg->compute_dtype != CAP_BF16) {
            cap_set_error("cap_create: weight_int8 (load_in_8bit) is built for CAP_ARCH_BLIP2 with CAP_BF16 activations");
            return -1;
        }
        if (skinny_i8_plan(3 * T, T, true) < 1 || skinny_i8_plan(G, T, true) < 1 || skinny_i8_plan(T, T, false) < 1 || skinny_i8_plan(T, G, false) < 1) {
            cap_set_error("cap_create: weight_int8 needs OPT widths the int8 weight stream takes (hidden %d, ffn %d: multiples of 256 that "
                          "split into waves of at most 320 k)", T, G);
            return -1;
        }
    }
    int dev = 0;
    CAP_HIP_CHECK(hipGetDevice(&dev));
    if (share) {
        // same model, same arithmetic, same GPU; only the capacity of the arena may differ
        CapConfig a = *cfg, b = share->c;
        a.max_batch = b.max_batch = 0; a.max_beams = b.max_beams = 0; a.max_len = b.max_len = 0; a.max_prompt = b.max_prompt = 0;
        a.max_score_rows = b.max_score_rows = 0;
        if (memcmp(&a, &b, sizeof(a)) != 0 || share->ws->device != dev) {
            cap_set_error("cap_create_shared: the new handle must describe the same model, compute dtype and GPU as the handle "
                          "whose weights it shares");
            return -1;
        }
    }
    Captioner* m = new Captioner();
    m->c = *cfg;
    m->wq8 = cfg->weight_int8 != 0;
    if (share) { m->ws = share->ws; m->ws->refs.fetch_add(1); m->replay = true; }
    else { m->ws = new WeightStore(); m->ws->device = dev; }
    m->dt = cfg->compute_dtype == CAP_BF16 ? CAP_DT_BF16 : CAP_DT_F32;
    m->gdt = cfg->compute_dtype == CAP_F32_SPLIT ? CAP_DT_G8 : m->dt;
    m->esz = m->dt == CAP_DT_BF16 ? 2 : 4;            // a G8 element is 4 bytes like fp32
    const int g = text_only ? 0 : cfg->image_size / cfg->patch_size;
    // (the KV16 layout is read by the chunked cross-attention kernels: more than 32 keys per image - every real geometry; the
    // fixture-sized ones keep fp32 rows)
    m->kv16 = m->gdt == CAP_DT_G8 && !cfg->cross_kv_fp32 &&
              ((cfg->arch == CAP_ARCH_BLIP && g * g + 1 > 32) || (cfg->arch == CAP_ARCH_COCA && cfg->pool_queries - 1 > 32));
    m->kvrow = m->kv16 ? 132 : 64 * m->esz;
    m->P = g * g; m->NT = m->P + 1;
    m->Kpatch = text_only ? 0 : 3 * cfg->patch_size * cfg->patch_size;
    m->Kpad = (m->Kpatch + 63) / 64 * 64;
    const int built = text_only ? (build_minilm(m) != 0)
                      : cfg->arch == CAP_ARCH_BLIP2 ? (build_blip2(m) != 0)
                      : cfg->arch == CAP_ARCH_CLIP ? (build_clip(m) != 0)
                      : cfg->arch == CAP_ARCH_BLIP2_ITM ? (build_blip2_itm(m) != 0)
                      : cfg->arch == CAP_ARCH_COCA ? (build_coca(m) != 0 || build_arena_coca(m) != 0)
                                                   : (build_blip(m) != 0 || build_arena(m) != 0);
    if (built) {
        release_captioner(m);       // the message of the failing step is kept
        return -1;
    }
    if (m->replay && m->wcur != m->ws->ptrs.size()) {
        cap_set_error("cap_create_shared: the shared store holds %zu buffers, this configuration uses %zu", m->ws->ptrs.size(), m->wcur);
        release_captioner(m);
        return -1;
    }
    *out = (CapHandle)m;
    return 0;
}

int cap_create(const CapConfig* cfg, CapHandle* out) { return create_impl(cfg, nullptr, out); }

int cap_create_shared(const CapConfig* cfg, CapHandle weights_of, CapHandle* out) {
    if (!weights_of) { cap_set_error("cap_create_shared: null handle"); return -1; }
    return create_impl(cfg, (Captioner*)weights_of, out);
}

int cap_destroy(CapHandle h) {
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    release_captioner((Captioner*)h);
    return 0;
}

int cap_set_early_exit(CapHandle h, int poll_steps) {
    Captioner* m = (Captioner*)h;
    if (!m || poll_steps < 0) { cap_set_error("cap_set_early_exit: null handle or negative interval"); return -1; }
    if (poll_steps > 0 && !m->host_flag) {
        CAP_HIP_CHECK(hipHostMalloc((void**)&m->host_flag, sizeof(int), hipHostMallocMapped));
        CAP_HIP_CHECK(hipHostGetDevicePointer((void**)&m->host_flag_dev, m->host_flag, 0));
        *m->host_flag = 1;
    }
    m->poll = poll_steps;
    return 0;
}

int cap_set_bad_words(CapHandle h, const int32_t* ids, const int32_t* offsets, int n_sequences, void* stream) {
    Captioner* m = (Captioner*)h;
    const char* who = "cap_set_bad_words";
    if (!m) { cap_set_error("%s: null handle", who); return -1; }
    if (n_sequences < 0 || (n_sequences > 0 && (!ids || !offsets))) {
        cap_set_error("%s: %d sequences with ids %s and offsets %s (CSR: offsets [n_sequences + 1], ids [offsets[n_sequences]])", who, n_sequences,
                      ids ? "given" : "null", offsets ? "given" : "null");
        return -1;
    }
    const CapConfig& c = m->c;
    const int V = c.vocab;
    std::vector<unsigned> bits((size_t)ban_words(V), 0u);
    std::vector<int> multi;
    int n_multi = 0, n_single = 0;
    if (n_sequences > 0 && offsets[0] != 0) { cap_set_error("%s: offsets[0] = %d (CSR offsets start at 0)", who, offsets[0]); return -1; }
    for (int q = 0; q < n_sequences; ++q) {
        const int b = offsets[q], n = offsets[q + 1] - b;
        if (n < 1) { cap_set_error("%s: sequence %d is empty (offsets %d .. %d)", who, q, b, offsets[q + 1]); return -1; }
        for (int k = 0; k < n; ++k) {
            const int id = ids[b + k];
            if (id < 0 || id >= V) { cap_set_error("%s: sequence %d holds id %d, outside the vocabulary [0, %d)", who, q, id, V); return -1; }
            if (id == c.bos || id == c.pad) {
                cap_set_error("%s: sequence %d holds the %s id %d, which is never generated and only ever context", who, q, id == c.bos ? "BOS" : "pad", id);
                return -1;
            }
        }
        if (n == 1) {
            if (ids[b] == c.eos) continue;                     // HF drops [eos] silently
            unsigned& w = bits[(size_t)ids[b] >> 5];
            const unsigned bit = 1u << (ids[b] & 31);
            if (!(w & bit)) ++n_single;
            w |= bit;
            continue;
        }
        if (n > BAN_MAX_LEN) { cap_set_error("%s: sequence %d has %d tokens; a banned sequence has at most %d", who, q, n, BAN_MAX_LEN); return -1; }
        if (n_multi == BAN_MAX_MULTI) {
            cap_set_error("%s: more than %d multi-token sequences (single tokens are unbounded)", who, BAN_MAX_MULTI);
            return -1;
        }
        multi.resize((size_t)(n_multi + 1) * BAN_REC, 0);
        int* rec = multi.data() + (size_t)n_multi * BAN_REC;
        rec[0] = n;
        for (int k = 0; k < n; ++k) rec[1 + k] = ids[b + k];
        ++n_multi;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n_single == 0 && n_multi == 0) {                       // cleared: the launches are the unbanned ones again
        m->ban_n_single = 0; m->ban_n_multi = 0;
        return 0;
    }
    if (!m->ban_bits || !m->ban_multi) {                       // each pointer on its own: a failed allocation leaves nothing half-published
        if (!m->ban_bits) CAP_HIP_CHECK(hipMalloc((void**)&m->ban_bits, (size_t)ban_words(V) * 4));
        if (!m->ban_multi) CAP_HIP_CHECK(hipMalloc((void**)&m->ban_multi, (size_t)BAN_MAX_MULTI * BAN_REC * 4));
    } else {
        CAP_HIP_CHECK(hipStreamSynchronize(s));                // the host copies a previous upload may still be reading are replaced below
    }
    m->ban_bits_host.swap(bits);
    m->ban_multi_host.swap(multi);
    CAP_HIP_CHECK(hipMemcpyAsync(m->ban_bits, m->ban_bits_host.data(), m->ban_bits_host.size() * 4, hipMemcpyHostToDevice, s));
    if (n_multi)
        CAP_HIP_CHECK(hipMemcpyAsync(m->ban_multi, m->ban_multi_host.data(), m->ban_multi_host.size() * 4, hipMemcpyHostToDevice, s));
    m->ban_n_single = n_single; m->ban_n_multi = n_multi;
    return 0;
}

int cap_bad_words(CapHandle h, int* n_single, int* n_multi) {
    const Captioner* m = (const Captioner*)h;
    if (!m) { cap_set_error("cap_bad_words: null handle"); return -1; }
    if (n_single) *n_single = m->ban_n_single;
    if (n_multi) *n_multi = m->ban_n_multi;
    return 0;
}

int cap_set_repeat_controls(CapHandle h, float repetition_penalty, int no_repeat_ngram_size) {
    Captioner* m = (Captioner*)h;
    const char* who = "cap_set_repeat_controls";
    if (!m) { cap_set_error("%s: null handle", who); return -1; }
    const CapConfig& c = m->c;
    if (!std::isfinite(repetition_penalty) || !(repetition_penalty > 0.f)) {
        cap_set_error("%s: repetition_penalty = %g (a finite number above 0; 1 = off)", who, (double)repetition_penalty);
        return -1;
    }
    if (no_repeat_ngram_size < 0) { cap_set_error("%s: no_repeat_ngram_size = %d (0 = off, or an n-gram size >= 1)", who, no_repeat_ngram_size); return -1; }
    // the longest context a processor ever sees: BLIP max_len tokens with BOS; BLIP-2 the placeholders, BOS and max_len new tokens
    const int prefix = c.arch == CAP_ARCH_BLIP2 ? c.num_query_tokens + 1 : 0;
    if (no_repeat_ngram_size > c.max_len + prefix) {
        cap_set_error("%s: no_repeat_ngram_size = %d is beyond the %d tokens a caption of this handle can hold (max_len %d + a prefix of %d)", who,
                      no_repeat_ngram_size, c.max_len + prefix, c.max_len, prefix);
        return -1;
    }
    const bool on = repetition_penalty != 1.f || no_repeat_ngram_size > 0;
    if (on && c.arch != CAP_ARCH_BLIP && c.arch != CAP_ARCH_BLIP2 && c.arch != CAP_ARCH_COCA) {
        cap_set_error("%s: this handle's arch (%d) has no decode loop", who, c.arch);
        return -1;
    }
    if (on && c.arch == CAP_ARCH_BLIP2 && m->image_token < 0) {
        cap_set_error("%s: a BLIP-2 handle needs the id of its image placeholders first (cap_set_image_token): HF's processors see them "
                      "in front of BOS", who);
        return -1;
    }
    m->rep_penalty = repetition_penalty; m->rep_ngram = no_repeat_ngram_size;
    return 0;
}

int cap_repeat_controls(CapHandle h, float* repetition_penalty, int* no_repeat_ngram_size) {
    const Captioner* m = (const Captioner*)h;
    if (!m) { cap_set_error("cap_repeat_controls: null handle"); return -1; }
    if (repetition_penalty) *repetition_penalty = m->rep_penalty;
    if (no_repeat_ngram_size) *no_repeat_ngram_size = m->rep_ngram;
    return 0;
}

int cap_set_image_token(CapHandle h, int image_token) {
    Captioner* m = (Captioner*)h;
    if (!m) { cap_set_error("cap_set_image_token: null handle"); return -1; }
    if (m->c.arch != CAP_ARCH_BLIP2) { cap_set_error("cap_set_image_token: image placeholders are CAP_ARCH_BLIP2's (this handle's arch is %d)", m->c.arch); return -1; }
    if (image_token < 0) { cap_set_error("cap_set_image_token: id %d (>= 0; an id beyond the vocabulary is context no processor acts on)", image_token); return -1; }
    m->image_token = image_token;
    return 0;
}

int cap_set_sampling(CapHandle h, int on, float temperature, int top_k, float top_p, uint64_t seed) {
    Captioner* m = (Captioner*)h;
    const char* who = "cap_set_sampling";
    if (!m) { cap_set_error("%s: null handle", who); return -1; }
    const CapConfig& c = m->c;
    if (!std::isfinite(temperature) || !(temperature > 0.f)) {
        cap_set_error("%s: temperature = %g (a finite number above 0; 1 = neutral)", who, (double)temperature);
        return -1;
    }
    if (top_k < 0) { cap_set_error("%s: top_k = %d (0 = off, or a count >= 1)", who, top_k); return -1; }
    if (!(top_p > 0.f) || !(top_p <= 1.f)) { cap_set_error("%s: top_p = %g (in (0, 1]; 1 = off)", who, (double)top_p); return -1; }
    if (on && c.arch != CAP_ARCH_BLIP && c.arch != CAP_ARCH_BLIP2 && c.arch != CAP_ARCH_COCA) {
        cap_set_error("%s: this handle's arch (%d) has no decode loop", who, c.arch);
        return -1;
    }
    if (on && c.arch == CAP_ARCH_BLIP2 && m->image_token < 0 && m->repeat_active()) {
        cap_set_error("%s: a BLIP-2 handle with repetition controls needs cap_set_image_token first", who);
        return -1;
    }
    m->sampling = on != 0;
    m->sample_ctl.temperature = temperature; m->sample_ctl.top_k = top_k; m->sample_ctl.top_p = top_p; m->sample_ctl.seed = seed;
    return 0;
}

int cap_sampling(CapHandle h, int* on, float* temperature, int* top_k, float* top_p, uint64_t* seed) {
    const Captioner* m = (const Captioner*)h;
    if (!m) { cap_set_error("cap_sampling: null handle"); return -1; }
    if (on) *on = m->sampling ? 1 : 0;
    if (temperature) *temperature = m->sample_ctl.temperature;
    if (top_k) *top_k = m->sample_ctl.top_k;
    if (top_p) *top_p = m->sample_ctl.top_p;
    if (seed) *seed = m->sample_ctl.seed;
    return 0;
}

int cap_last_decode_steps(CapHandle h) { return h ? ((Captioner*)h)->last_steps : -1; }

int cap_set_decode_path(CapHandle h, int path) {
    Captioner* m = (Captioner*)h;
    if (!m) { cap_set_error("cap_set_decode_path: null handle"); return -1; }
    if (path < 0 || path > 2) { cap_set_error("cap_set_decode_path: path must be 0 (by row count), 1 (batch kernels, one launch per operation) or 2 (small-batch kernels), got %d", path); return -1; }
    m->decode_path = path;
    return 0;
}
int cap_last_decode_path(CapHandle h) { return h ? ((Captioner*)h)->last_path : -1; }

int cap_set_row_compaction(CapHandle h, int on) {
    Captioner* m = (Captioner*)h;
    if (!m || (on != 0 && on != 1)) { cap_set_error("cap_set_row_compaction: null handle, or a value other than 0 / 1"); return -1; }
    m->compaction = on;
    return 0;
}
int cap_last_row_compaction(CapHandle h) { return h ? ((Captioner*)h)->last_compacted : -1; }
int cap_cross_cache_kind(CapHandle h) {
    const Captioner* m = (const Captioner*)h;
    if (!m) return -1;
    return m->kv16 ? 2 : (m->dt == CAP_DT_BF16 ? 1 : 0);
}

size_t cap_device_bytes(CapHandle h) { return h ? ((Captioner*)h)->dev_bytes : 0; }

long long cap_debug_fill_arena(CapHandle h, uint32_t pattern, void* stream) {
    Captioner* m = (Captioner*)h;
    if (!m) { cap_set_error("cap_debug_fill_arena: null handle"); return -1; }
    long long filled = 0;
    for (const ArenaAlloc& a : m->allocs) {
        if (a.kind != ARENA_SCRATCH) continue;
        if (launch_fill_i32((int*)a.p, (int)pattern, a.bytes / 4, (hipStream_t)stream) != 0) return -1;    // bytes: a multiple of 256
        filled += (long long)a.bytes;
    }
    return filled;
}

int cap_debug_arena_kinds(CapHandle h, char* buf, size_t buf_bytes) {
    Captioner* m = (Captioner*)h;
    if (!m || !buf) { cap_set_error("cap_debug_arena_kinds: null argument"); return -1; }
    size_t total[ARENA_KINDS] = {0, 0, 0};
    std::string names[ARENA_KINDS];
    for (const ArenaAlloc& a : m->allocs) {
        if (a.kind < 0 || a.kind >= ARENA_KINDS || (a.kind != ARENA_SCRATCH && !a.name)) {
            cap_set_error("cap_debug_arena_kinds: an allocation of kind %d has no name", a.kind);
            return -1;
        }
        total[a.kind] += a.bytes;
        if (a.kind != ARENA_SCRATCH) names[a.kind] += std::string(names[a.kind].empty() ? "\"" : ", \"") + a.name + "\"";
    }
    // the handle's arena as cap_device_bytes counts it: everything it allocated less the weights it created
    const size_t arena = m->dev_bytes - (m->replay || !m->ws ? 0 : m->ws->bytes);
    char head[256];
    snprintf(head, sizeof(head), "{\"arena_bytes\": %zu, \"scratch_bytes\": %zu, \"index_bytes\": %zu, \"kept_bytes\": %zu, ", arena,
             total[ARENA_SCRATCH], total[ARENA_INDEX], total[ARENA_KEPT]);
    const std::string out = std::string(head) + "\"index\": [" + names[ARENA_INDEX] + "], \"kept\": [" + names[ARENA_KEPT] + "]}";
    if (out.size() + 1 > buf_bytes) { cap_set_error("cap_debug_arena_kinds: buffer too small (%zu needed)", out.size() + 1); return -1; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return 0;
}

int cap_load_weight(CapHandle h, const char* name, const float* data, int on_device, int ndim, const int64_t* shape,
                    void* stream) {
    Captioner* m = (Captioner*)h;
    if (!m || !name || !data) { cap_set_error("cap_load_weight: null argument"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    auto range = m->ws->slots.equal_range(name);
    if (range.first == range.second) return 1;   // not a tensor this architecture stores (e.g. tied decoder.weight)
    const float* src = data;
    if (!on_device) {
        if ((size_t)n > m->stage_elems) {
            if (m->stage) { CAP_HIP_CHECK(hipStreamSynchronize(s)); (void)hipFree(m->stage); }
            CAP_HIP_CHECK(hipMalloc((void**)&m->stage, (size_t)n * 4));
            m->stage_elems = n;
        }
        CAP_HIP_CHECK(hipMemcpyAsync(m->stage, data, (size_t)n * 4, hipMemcpyHostToDevice, s));
        src = m->stage;
    }
    bool any_g8 = false;
    for (auto it = range.first; it != range.second; ++it) any_g8 |= it->second.dtype == CAP_DT_G8;
    if (any_g8) {
        // split mode stores 4096 * w as two fp16 halves: a tensor that does not fit fp16's range would be clipped silently -
        // refuse it instead (real checkpoints sit far below the bound; this is the guard for the ones that do not)
        if (!m->absmax_dev) CAP_HIP_CHECK(hipMalloc((void**)&m->absmax_dev, 256));
        CAP_HIP_CHECK(hipMemsetAsync(m->absmax_dev, 0, 4, s));
        TRY(launch_absmax_f32(src, (size_t)n, m->absmax_dev, s));
        unsigned int bits = 0;
        CAP_HIP_CHECK(hipMemcpyAsync(&bits, m->absmax_dev, 4, hipMemcpyDeviceToHost, s));
        CAP_HIP_CHECK(hipStreamSynchronize(s));
        float amax;
        memcpy(&amax, &bits, 4);
        if (!(amax * G8_WSCALE <= G8_AMAX)) {
            cap_set_error("cap_load_weight: %s has max |w| = %g; the split-fp16 mode (CAP_F32_SPLIT / dtype \"f32s\") stores "
                          "%g * w in fp16 and takes |w| <= %g (no NaN) - load this checkpoint with CAP_F32 or CAP_BF16",
                          name, (double)amax, (double)G8_WSCALE, (double)(G8_AMAX / G8_WSCALE));
            return -1;
        }
    }
    for (auto it = range.first; it != range.second; ++it) {
        Slot& sl = it->second;
        if (sl.rows * sl.cols != n) {
            cap_set_error("cap_load_weight: %s has %lld elements, expected %lld x %lld", name, (long long)n,
                          (long long)sl.rows, (long long)sl.cols);
            return -1;
        }
        if (sl.dtype == CAP_DT_I8W) TRY(launch_quant_i8_pack(src, sl.dst, (float*)sl.aux, (int)sl.rows, (int)sl.cols, s));
        else TRY(launch_convert2d(sl.dtype, src, sl.dst, (int)sl.rows, (int)sl.cols, sl.dst_ld, s, sl.dtype == CAP_DT_G8 ? G8_WSCALE : 1.0f));
        sl.loaded = true;
    }
    CAP_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int cap_finalize_weights(CapHandle h) {
    Captioner* m = (Captioner*)h;
    if (!m) { cap_set_error("null handle"); return -1; }
    int missing = 0;
    std::string names;
    for (auto& kv : m->ws->slots)
        if (!kv.second.loaded) {
            if (missing < 8) names += (missing ? ", " : "") + kv.first;
            ++missing;
        }
    if (missing) cap_set_error("%d tensors not loaded: %s%s", missing, names.c_str(), missing > 8 ? ", ..." : "");
    return missing;
}

// what an entry point that needs pixels says to CAP_PIX_IMAGE_STATE
#define REFUSE_IMAGE_STATE(who) cap_set_error("%s: CAP_PIX_IMAGE_STATE is taken by cap_generate_request, the cap_generate* calls and " \
                                              "cap_score_captions; this call needs pixels (CAP_PIX_F32_NCHW or CAP_PIX_U8_NHWC)", who)

// state_ok: the call decodes, so `pixels` may be image-state records (validate_generate / validate_score look at the pointer)
static int check_call(Captioner* m, int B, int K, int Lm, int fmt, const char* who, bool state_ok = false) {
    if (!m) { cap_set_error("%s: null handle", who); return -1; }
    if (cap_finalize_weights((CapHandle)m) != 0) return -1;
    if (B < 1 || B > m->c.max_batch || K < 1 || K > m->c.max_beams || Lm < (m->c.arch == CAP_ARCH_BLIP2 ? 1 : 2) || Lm > m->c.max_len) {
        cap_set_error("%s: request B=%d beams=%d max_len=%d exceeds the handle's capacity (%d, %d, %d)", who, B, K, Lm,
                      m->c.max_batch, m->c.max_beams, m->c.max_len);
        return -1;
    }
    if (fmt == CAP_PIX_IMAGE_STATE && !state_ok) { REFUSE_IMAGE_STATE(who); return -1; }
    if (fmt != CAP_PIX_F32_NCHW && fmt != CAP_PIX_U8_NHWC && fmt != CAP_PIX_IMAGE_STATE) { cap_set_error("%s: unknown pixel format %d", who, fmt); return -1; }
    if (m->c.arch == CAP_ARCH_MINILM) { cap_set_error("%s: this handle is a sentence encoder: use cap_embed_text", who); return -1; }
    if (m->c.arch == CAP_ARCH_CLIP) { cap_set_error("%s: this handle is a CLIP scorer: use cap_clip_embed_images / cap_clip_embed_text", who); return -1; }
    if (m->c.arch == CAP_ARCH_BLIP2_ITM) { cap_set_error("%s: this handle is a BLIP-2 image-text scorer: use cap_blip2_itm_encode_images / cap_blip2_itc_* / cap_blip2_itm_logits", who); return -1; }
    return 0;
}

static int check_clip(Captioner* m, const char* fn) {
    if (!m) { cap_set_error("%s: null handle", fn); return -1; }
    if (m->c.arch != CAP_ARCH_CLIP) { cap_set_error("%s: the handle is not a CLIP scorer (CAP_ARCH_CLIP)", fn); return -1; }
    return cap_finalize_weights((CapHandle)m) != 0 ? -1 : 0;
}

int cap_clip_embed_images(CapHandle h, const void* pixels, int pixel_fmt, int B, float* out, void* stream) {
    Captioner* m = (Captioner*)h;
    TRY(check_clip(m, "cap_clip_embed_images"));
    if (!pixels || !out) { cap_set_error("cap_clip_embed_images: null buffer"); return -1; }
    if (B < 1 || B > m->c.max_batch) { cap_set_error("cap_clip_embed_images: B=%d exceeds the handle's capacity (%d)", B, m->c.max_batch); return -1; }
    if (pixel_fmt == CAP_PIX_IMAGE_STATE) { REFUSE_IMAGE_STATE("cap_clip_embed_images"); return -1; }
    if (pixel_fmt != CAP_PIX_F32_NCHW && pixel_fmt != CAP_PIX_U8_NHWC) { cap_set_error("unknown pixel format %d", pixel_fmt); return -1; }
    return run_clip_images(m, pixels, pixel_fmt, B, out, (hipStream_t)stream);
}

int cap_clip_embed_text(CapHandle h, const int32_t* ids, const int32_t* lens, int B, int L, float* out, void* stream) {
    Captioner* m = (Captioner*)h;
    TRY(check_clip(m, "cap_clip_embed_text"));
    if (!ids || !lens || !out) { cap_set_error("cap_clip_embed_text: null buffer"); return -1; }
    if (B < 1 || B > m->c.max_batch || L < 1 || L > m->c.max_len) {
        cap_set_error("cap_clip_embed_text: B=%d L=%d exceeds the handle's capacity (%d, %d)", B, L, m->c.max_batch, m->c.max_len);
        return -1;
    }
    return run_clip_text(m, ids, lens, B, L, out, (hipStream_t)stream);
}

int cap_clip_logits(const float* img, const float* txt, int Ni, int Nt, int paired, float logit_scale, float* out, int embed_dim,
                    void* stream) {
    if (!img || !txt || !out) { cap_set_error("cap_clip_logits: null buffer"); return -1; }
    return launch_clip_logits(img, txt, Ni, Nt, embed_dim, paired, logit_scale, out, (hipStream_t)stream);
}

int cap_cosine_matrix(const float* a, const float* b, int Na, int Nb, int D, int paired, float* out, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return launch_cosine_matrix(a, b, Na, Nb, D, paired, out, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t cap_group_similarity_workspace(int N, int G, int D, const int32_t* offsets) { return sim_group_workspace(N, G, D, offsets); }

int cap_group_similarity(const float* e, const int32_t* offsets, const float* weights, int N, int G, int D, float* disagreement,
                         float* pair_mean, float* pair_var, int64_t* pairs, int32_t* medoid, float* row_mean, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return launch_group_similarity(e, offsets, weights, N, G, D, disagreement, pair_mean, pair_var, (long long*)pairs, medoid, row_mean,
                                   workspace, workspace_bytes, (hipStream_t)stream);
}

int cap_clip_logit_scale(CapHandle h, float* out) {
    Captioner* m = (Captioner*)h;
    if (!out) { cap_set_error("cap_clip_logit_scale: null output"); return -1; }
    TRY(check_clip(m, "cap_clip_logit_scale"));
    CAP_HIP_CHECK(hipMemcpy(out, m->c_logit, sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

static int check_itm(Captioner* m, const char* fn) {
    if (!m) { cap_set_error("%s: null handle", fn); return -1; }
    if (m->c.arch != CAP_ARCH_BLIP2_ITM) { cap_set_error("%s: the handle is not a BLIP-2 image-text scorer (CAP_ARCH_BLIP2_ITM)", fn); return -1; }
    return cap_finalize_weights((CapHandle)m) != 0 ? -1 : 0;
}
// the pairs of a call are the images of the last cap_blip2_itm_encode_images, in order
static int check_itm_resident(Captioner* m, const char* fn, int B) {
    if (m->itm_B < 1) { cap_set_error("%s: no image batch is resident (call cap_blip2_itm_encode_images first)", fn); return -1; }
    if (B != m->itm_B) { cap_set_error("%s: B=%d, but the resident image batch has %d images", fn, B, m->itm_B); return -1; }
    return 0;
}
static int check_itm_text(Captioner* m, const char* fn, const void* ids, const void* lens, int B, int L) {
    if (!ids || !lens) { cap_set_error("%s: null buffer", fn); return -1; }
    if (L > m->c.max_len) { cap_set_error("%s: text of %d tokens is longer than the handle's max_len (%d): truncate on the host", fn, L, m->c.max_len); return -1; }
    if (B > m->c.max_batch) { cap_set_error("%s: B=%d exceeds the handle's capacity (max_batch %d)", fn, B, m->c.max_batch); return -1; }
    if (B < 1 || L < 1) { cap_set_error("%s: bad shape B=%d L=%d", fn, B, L); return -1; }
    return 0;
}

int cap_blip2_itm_encode_images(CapHandle h, const void* pixels, int pixel_fmt, int B, void* stream) {
    Captioner* m = (Captioner*)h;
    TRY(check_itm(m, "cap_blip2_itm_encode_images"));
    if (!pixels) { cap_set_error("cap_blip2_itm_encode_images: null buffer"); return -1; }
    if (B < 1 || B > m->c.max_batch) { cap_set_error("cap_blip2_itm_encode_images: B=%d exceeds the handle's capacity (max_batch %d)", B, m->c.max_batch); return -1; }
    if (pixel_fmt == CAP_PIX_IMAGE_STATE) { REFUSE_IMAGE_STATE("cap_blip2_itm_encode_images"); return -1; }
    if (pixel_fmt != CAP_PIX_F32_NCHW && pixel_fmt != CAP_PIX_U8_NHWC) { cap_set_error("unknown pixel format %d", pixel_fmt); return -1; }
    return run_itm_images(m, pixels, pixel_fmt, B, (hipStream_t)stream);
}

int cap_blip2_itc_image_features(CapHandle h, int B, float* out, void* stream) {
    Captioner* m = (Captioner*)h;
    TRY(check_itm(m, "cap_blip2_itc_image_features"));
    if (!out) { cap_set_error("cap_blip2_itc_image_features: null buffer"); return -1; }
    TRY(check_itm_resident(m, "cap_blip2_itc_image_features", B));
    const CapConfig& c = m->c;
    hipStream_t s = (hipStream_t)stream;
    TRY(run_qformer(m, kScorerPass, B, c.num_query_tokens, 0, nullptr, nullptr, s));
    ProfScope ps(m, s, "itc_image_head", 2.0 * B * c.num_query_tokens * c.q_hidden * c.embed_dim, (double)B * c.num_query_tokens * (c.q_hidden + c.embed_dim) * 4);
    return launch_itc_head(m->qr.x, 1, m->i_vproj, m->i_vproj_b, out, B * c.num_query_tokens, c.q_hidden, c.embed_dim, s);
}

int cap_blip2_itc_text_features(CapHandle h, const int32_t* ids, const int32_t* lens, int B, int L, float* out, void* stream) {
    Captioner* m = (Captioner*)h;
    TRY(check_itm(m, "cap_blip2_itc_text_features"));
    TRY(check_itm_text(m, "cap_blip2_itc_text_features", ids, lens, B, L));
    if (!out) { cap_set_error("cap_blip2_itc_text_features: null buffer"); return -1; }
    const CapConfig& c = m->c;
    hipStream_t s = (hipStream_t)stream;
    TRY(run_qformer(m, kScorerPass, B, 0, L, ids, lens, s));
    ProfScope ps(m, s, "itc_text_head", 2.0 * B * c.q_hidden * c.embed_dim, (double)B * (c.q_hidden + c.embed_dim) * 4);
    return launch_itc_head(m->tr.x, L, m->i_tproj, m->i_tproj_b, out, B, c.q_hidden, c.embed_dim, s);
}

int cap_blip2_itc_scores(const float* img, const float* txt, int Ni, int Nt, int paired, float* out, int num_queries, int embed_dim,
                         void* stream) {
    if (!img || !txt || !out) { cap_set_error("cap_blip2_itc_scores: null buffer"); return -1; }
    return launch_itc_scores(img, txt, Ni, Nt, num_queries, embed_dim, paired, out, (hipStream_t)stream);
}

int cap_blip2_itm_logits(CapHandle h, const int32_t* ids, const int32_t* lens, int B, int L, float* out_logits, float* out_prob,
                         void* stream) {
    Captioner* m = (Captioner*)h;
    TRY(check_itm(m, "cap_blip2_itm_logits"));
    TRY(check_itm_text(m, "cap_blip2_itm_logits", ids, lens, B, L));
    if (!out_logits) { cap_set_error("cap_blip2_itm_logits: null buffer"); return -1; }
    TRY(check_itm_resident(m, "cap_blip2_itm_logits", B));
    const CapConfig& c = m->c;
    hipStream_t s = (hipStream_t)stream;
    TRY(run_qformer(m, kScorerPass, B, c.num_query_tokens, L, ids, lens, s));
    ProfScope ps(m, s, "itm_head", 4.0 * B * c.num_query_tokens * c.q_hidden, (double)B * c.num_query_tokens * c.q_hidden * 4);
    return launch_itm_head(m->qr.x, m->i_head, m->i_head_b, out_logits, out_prob, B, c.num_query_tokens, c.q_hidden, s);
}

int cap_embed_text(CapHandle h, const int32_t* ids, const int32_t* lens, int B, int L, float* out, void* stream) {
    Captioner* m = (Captioner*)h;
    if (!m) { cap_set_error("null handle"); return -1; }
    if (m->c.arch != CAP_ARCH_MINILM) { cap_set_error("cap_embed_text: the handle is not a sentence encoder"); return -1; }
    if (cap_finalize_weights(h) != 0) return -1;
    if (!ids || !lens || !out) { cap_set_error("cap_embed_text: null buffer"); return -1; }
    if (B < 1 || B > m->c.max_batch || L < 1 || L > m->c.max_len) {
        cap_set_error("cap_embed_text: B=%d L=%d exceeds the handle's capacity (%d, %d)", B, L, m->c.max_batch, m->c.max_len);
        return -1;
    }
    return run_text_encoder(m, ids, lens, B, L, out, (hipStream_t)stream);
}

int cap_encode(CapHandle h, const void* pixels, int pixel_fmt, int B, float* out_embeds, void* stream) {
    Captioner* m = (Captioner*)h;
    TRY(check_call(m, B, 1, 2, pixel_fmt, "cap_encode"));
    if (!pixels || !out_embeds) { cap_set_error("cap_encode: null buffer"); return -1; }
    if (m->c.arch == CAP_ARCH_COCA) {    // out_embeds: fp32 [B, pool_queries, embed_dim] (row 0 pooled token, rows 1.. image_embs)
        TRY(run_encoder(m, pixels, pixel_fmt, B, nullptr, (hipStream_t)stream));
        return run_coca_pool(m, B, out_embeds, (hipStream_t)stream);
    }
    return run_encoder(m, pixels, pixel_fmt, B, out_embeds, (hipStream_t)stream);
}

size_t cap_image_state_bytes(CapHandle h) {
    const Captioner* m = (const Captioner*)h;
    if (!m) { cap_set_error("cap_image_state_bytes: null handle"); return 0; }
    if (!takes_image_state(m)) {
        cap_set_error("cap_image_state_bytes: an image state is what a BLIP, CoCa or BLIP-2 captioner decodes from; this handle's arch is %d", m->c.arch);
        return 0;
    }
    return image_state_layout(m).record_bytes();
}

int cap_encode_image_state(CapHandle h, const void* pixels, int pixel_fmt, int B, void* out_state, void* stream) {
    Captioner* m = (Captioner*)h;
    const char* who = "cap_encode_image_state";
    if (!m) { cap_set_error("%s: null handle", who); return -1; }
    TRY(check_call(m, B, 1, m->c.arch == CAP_ARCH_BLIP2 ? 1 : 2, pixel_fmt, who));
    if (!pixels || !out_state) { cap_set_error("%s: null buffer", who); return -1; }
    if (((uintptr_t)out_state & 15) != 0) { cap_set_error("%s: out_state must be 16-byte aligned", who); return -1; }
    if (m->c.arch == CAP_ARCH_BLIP2) TRY(run_blip2_image_side(m, pixels, pixel_fmt, B, (hipStream_t)stream));
    else TRY(run_image_side(m, pixels, pixel_fmt, B, (hipStream_t)stream));
    return export_image_state(m, B, out_state, (hipStream_t)stream);
}

// Every rule of a generate request, each once, in the order of refusal: the handle and its capacity (check_call), buffers, what the
// architecture takes, shapes - all before anything is launched.  who: the entry point the caller used; missing: what that entry
// point requires beyond the request's own rules and did not get (null: nothing).
static int validate_generate(Captioner* m, const CapGenerateArgs& a, const char* who, const char* missing) {
#define REFUSE_IF(cond, ...) do { if (cond) { cap_set_error(__VA_ARGS__); return -1; } } while (0)
    TRY(check_call(m, a.B, a.num_beams, a.max_len, a.pixel_fmt, who, true));
    const CapConfig& c = m->c;
    const int K = a.num_beams, G = a.num_beam_groups, P = a.prompt_len;
    const bool greedy = K == 1 && !G;
    REFUSE_IF(!a.pixels || !a.out_ids, "%s: null buffer", who);
    REFUSE_IF(a.pixel_fmt == CAP_PIX_IMAGE_STATE && ((uintptr_t)a.pixels & 15) != 0, "%s: the image state must be 16-byte aligned", who);
    REFUSE_IF(missing, "%s: %s", who, missing);
    REFUSE_IF(a.prompt_ids && c.arch != CAP_ARCH_BLIP,
              "%s: a text prompt is taken by CAP_ARCH_BLIP handles (this handle's arch is %d: CoCa's `text=` and BLIP-2's prompt are not built)",
              who, c.arch);
    REFUSE_IF(m->banned() && G && c.arch != CAP_ARCH_COCA,
              "%s: bad words are set on this handle (cap_set_bad_words) and beam groups do not take them", who);
    REFUSE_IF(m->repeat_active() && G && c.arch != CAP_ARCH_COCA,
              "%s: repetition controls are set on this handle (cap_set_repeat_controls) and beam groups do not take them", who);
    REFUSE_IF(m->sampling && G && c.arch != CAP_ARCH_COCA,
              "%s: sampling is set on this handle (cap_set_sampling) and beam groups do not take it: beam sampling is not built", who);
    REFUSE_IF(G && c.arch != CAP_ARCH_COCA,
              "%s: beam groups are the CoCa loop's (coca_model.py:335-482); HF's group beam search for the other architectures needs a "
              "diversity penalty, which this library does not implement", who);
    if (m->banned()) {          // cap_set_bad_words: BLIP and BLIP-2, greedy and beams, tokens only
        REFUSE_IF(c.arch == CAP_ARCH_COCA,
                  "%s: bad words are set on this handle (cap_set_bad_words) and it is a CoCa captioner: the reference's CoCa.generate has no "
                  "such option (BLIP and BLIP-2 only); clear the set with n_sequences = 0", who);
        REFUSE_IF(a.out_logprobs || a.out_scored || a.out_vocab,
                  "%s: bad words are set on this handle (cap_set_bad_words) and out_logprobs / out_vocab describe the raw logits, which no "
                  "longer describe the selection: clear the set, or leave these outputs out", who);
    }
    if (m->repeat_active()) {   // cap_set_repeat_controls: BLIP and BLIP-2, greedy and beams, tokens only
        REFUSE_IF(c.arch == CAP_ARCH_COCA,
                  "%s: repetition controls are set on this handle (cap_set_repeat_controls: penalty %g, n-gram size %d) and it is a CoCa "
                  "captioner: its decode loop does not apply them (BLIP and BLIP-2 only); reset them with (1, 0)", who,
                  (double)m->rep_penalty, m->rep_ngram);
        REFUSE_IF(a.out_logprobs || a.out_scored || a.out_vocab,
                  "%s: repetition controls are set on this handle (cap_set_repeat_controls) and out_logprobs / out_vocab describe the raw "
                  "logits, which no longer describe the selection: reset the controls with (1, 0), or leave these outputs out", who);
    }
    if (m->sampling) {          // cap_set_sampling: BLIP and BLIP-2, the greedy loop, tokens only
        REFUSE_IF(c.arch == CAP_ARCH_COCA,
                  "%s: sampling is set on this handle (cap_set_sampling) and it is a CoCa captioner: CoCa's sampling loop is not built (BLIP "
                  "and BLIP-2 only); switch it off with on = 0", who);
        REFUSE_IF(G, "%s: sampling is set on this handle (cap_set_sampling) and beam groups do not take it: beam sampling is not built", who);
        REFUSE_IF(K > 1, "%s: sampling is set on this handle (cap_set_sampling) and num_beams = %d: beam sampling is not built (num_beams = "
                  "1 only)", who, K);
        REFUSE_IF(a.out_logprobs || a.out_scored || a.out_vocab,
                  "%s: sampling is set on this handle (cap_set_sampling) and out_logprobs / out_vocab describe the arg-max of the raw logits, "
                  "which is not the selection: switch sampling off, or leave these outputs out", who);
    }
    REFUSE_IF(G < 0 || G > K || (G && K % G != 0), "%s: num_beams (%d) must be a multiple of num_beam_groups (%d) (BeamSearchScorer's own check)",
              who, K, G);
    REFUSE_IF(G && a.out_step_logits, "%s: per-step logits are not recorded by the group beam search", who);
    if (a.prompt_ids) {
        REFUSE_IF(!greedy, "%s: a prompt is taken by the greedy loop (num_beams = 1, no beam groups), got num_beams = %d", who, K);
        REFUSE_IF(a.prompt_rows != 1 && a.prompt_rows != a.B, "%s: prompt_rows %d is neither 1 (shared) nor the batch size %d", who, a.prompt_rows, a.B);
        REFUSE_IF(P > CAP_MAX_PROMPT, "%s: prompt_len %d exceeds the limit of %d prompt tokens (BOS included)", who, P, CAP_MAX_PROMPT);
        REFUSE_IF(P < 2 || P >= a.max_len,
                  "%s: prompt_len %d must be in [2, max_len = %d): BOS plus at least one token, and room for one generated token", who, P, a.max_len);
        REFUSE_IF((size_t)(P - 1) > m->ws_rows,
                  "%s: prompt_len %d exceeds the limit of %zu tokens this handle's workspace (%zu rows) takes: create it with "
                  "CapConfig.max_prompt >= %d", who, P, m->ws_rows + 1, m->ws_rows, P);
    }
    REFUSE_IF((a.out_logprobs != nullptr) != (a.out_scored != nullptr), "%s: out_logprobs and out_scored come together (both or neither)", who);
    REFUSE_IF(a.out_logprobs && !greedy,
              "%s: per-step log-probs are the greedy loop's (num_beams = 1), got num_beams = %d: beam search returns sequences_scores", who, K);
    if (a.out_vocab) {
        REFUSE_IF(!a.out_logprobs, "%s: out_vocab needs out_logprobs and out_scored", who);
        REFUSE_IF(a.acc_ld < c.vocab, "%s: acc_ld (%d) is below the vocabulary size (%d)", who, a.acc_ld, c.vocab);
        REFUSE_IF(a.acc_ld % 4 != 0, "%s: acc_ld (%d) must be a multiple of 4 (16-byte rows)", who, a.acc_ld);
        REFUSE_IF(((uintptr_t)a.out_vocab & 15) != 0, "%s: out_vocab must be 16-byte aligned", who);
    }
    if (m->decode_path == 2 && c.arch != CAP_ARCH_BLIP2) {      // within a call small_path_takes varies only through the position
        const int R = a.B * beams_per_search(a), t0 = a.prompt_ids ? P - 1 : 0;
        REFUSE_IF(a.max_len - 1 > 32,
                  "%s: the small-batch decode path was forced (cap_set_decode_path 2) but max_len %d needs %d positions: it takes at most 32 "
                  "(automatic selection continues on the batch kernels from position 33)", who, a.max_len, a.max_len - 1);
        REFUSE_IF(!small_path_takes(m, make_dec(m, a.B, beams_per_search(a)), t0),
                  "%s: the small-batch decode path was forced (cap_set_decode_path 2) but does not take this call (%d rows, step %d, compute "
                  "type %d): at most %d rows, 32 positions, split or bf16 mode, BLIP / CoCa", who, R, t0, m->gdt, SMALL_MAX_ROWS);
    }
#undef REFUSE_IF
    return 0;
}

// The one way into the decode loops: validate, then the architecture's loop.
static int generate(CapHandle h, const CapGenerateArgs& a, void* stream, const char* who, const char* missing) {
    Captioner* m = (Captioner*)h;
    TRY(validate_generate(m, a, who, missing));
    return (m->c.arch == CAP_ARCH_BLIP2 ? run_generate_blip2 : run_generate)(m, a, (hipStream_t)stream);
}

int cap_generate_request(CapHandle h, const CapGenerateArgs* args, void* stream) {
    if (!args) { cap_set_error("cap_generate_request: null request"); return -1; }
    return generate(h, *args, stream, "cap_generate_request", nullptr);
}

// The request with one key per caption for a handle that samples (cap_set_sampling): the keys hold for this call alone.
int cap_generate_sampled(CapHandle h, const CapGenerateArgs* args, const uint64_t* sample_keys, void* stream) {
    if (!args) { cap_set_error("cap_generate_sampled: null request"); return -1; }
    Captioner* m = (Captioner*)h;
    if (m) m->call_keys = sample_keys;
    const int rc = generate(h, *args, stream, "cap_generate_sampled", nullptr);
    if (m) m->call_keys = nullptr;
    return rc;
}

// The five calls below fix parts of a request and leave the rest absent.
static CapGenerateArgs request_of(const void* pixels, int pixel_fmt, int B, int num_beams, int max_len, float length_penalty,
                                  int32_t* out_ids, int32_t* out_len) {
    CapGenerateArgs a = {};
    a.pixels = pixels; a.pixel_fmt = pixel_fmt; a.B = B; a.num_beams = num_beams; a.max_len = max_len; a.length_penalty = length_penalty;
    a.out_ids = out_ids; a.out_len = out_len;
    return a;
}

int cap_generate_scored(CapHandle h, const void* pixels, int pixel_fmt, int B, int num_beams, int max_len, float length_penalty,
                        int32_t* out_ids, int32_t* out_len, float* out_scores, float* out_step_logits, float* out_logprobs,
                        int32_t* out_scored, void* stream) {
    CapGenerateArgs a = request_of(pixels, pixel_fmt, B, num_beams, max_len, length_penalty, out_ids, out_len);
    a.out_scores = out_scores; a.out_step_logits = out_step_logits; a.out_logprobs = out_logprobs; a.out_scored = out_scored;
    return generate(h, a, stream, out_logprobs || out_scored ? "cap_generate_scored" : "cap_generate", nullptr);
}

int cap_generate(CapHandle h, const void* pixels, int pixel_fmt, int B, int num_beams, int max_len, float length_penalty,
                 int32_t* out_ids, int32_t* out_len, float* out_scores, float* out_step_logits, void* stream) {
    return cap_generate_scored(h, pixels, pixel_fmt, B, num_beams, max_len, length_penalty, out_ids, out_len, out_scores,
                               out_step_logits, nullptr, nullptr, stream);
}

int cap_generate_vocab(CapHandle h, const void* pixels, int pixel_fmt, int B, int max_len, int32_t* out_ids, int32_t* out_len,
                       float* out_step_logits, float* out_logprobs, int32_t* out_scored, float* out_vocab, int acc_ld, void* stream) {
    CapGenerateArgs a = request_of(pixels, pixel_fmt, B, 1, max_len, 1.0f, out_ids, out_len);
    a.out_step_logits = out_step_logits; a.out_logprobs = out_logprobs; a.out_scored = out_scored; a.out_vocab = out_vocab; a.acc_ld = acc_ld;
    return generate(h, a, stream, "cap_generate_vocab",
                    out_logprobs && out_scored && out_vocab ? nullptr : "out_logprobs, out_scored and out_vocab are all required");
}

int cap_generate_prompted(CapHandle h, const void* pixels, int pixel_fmt, int B, int max_len, const int32_t* prompt_ids, int prompt_rows,
                          int prompt_len, int32_t* out_ids, int32_t* out_len, float* out_step_logits, float* out_logprobs,
                          int32_t* out_scored, float* out_vocab, int acc_ld, void* stream) {
    CapGenerateArgs a = request_of(pixels, pixel_fmt, B, 1, max_len, 1.0f, out_ids, out_len);
    a.out_step_logits = out_step_logits; a.out_logprobs = out_logprobs; a.out_scored = out_scored; a.out_vocab = out_vocab; a.acc_ld = acc_ld;
    a.prompt_ids = prompt_ids; a.prompt_rows = prompt_rows; a.prompt_len = prompt_len;
    return generate(h, a, stream, "cap_generate_prompted", prompt_ids ? nullptr : "prompt_ids is required");
}

int cap_last_prefill_passes(CapHandle h) { return h ? ((Captioner*)h)->last_prefill_passes : -1; }

// Every rule of a scoring request, before anything is launched (validate_generate's style and order: handle, capacity, buffers, what
// the architecture takes, shapes).  ids and lens are device data: the caller validates them (engine.validate_score_ids); the
// library clamps ids to [0, vocab) and lens - 1 to [0, L - 1].
static int validate_score(Captioner* m, const ScoreArgs& a, const char* who) {
#define REFUSE_IF(cond, ...) do { if (cond) { cap_set_error(__VA_ARGS__); return -1; } } while (0)
    REFUSE_IF(!m, "%s: null handle", who);
    REFUSE_IF(m->c.arch == CAP_ARCH_COCA, "%s: scoring given captions is not built for CoCa handles (CAP_ARCH_COCA): BLIP and BLIP-2 only", who);
    const bool b2 = m->c.arch == CAP_ARCH_BLIP2;
    // capacity: BLIP's max_len counts the caption's tokens with BOS, BLIP-2's the tokens behind BOS
    TRY(check_call(m, a.B, 1, b2 ? std::max(a.L - 1, 1) : std::max(a.L, 2), a.pixel_fmt, who, true));
    REFUSE_IF(m->c.arch != CAP_ARCH_BLIP && !b2, "%s: the handle is not a BLIP / BLIP-2 captioner (arch %d)", who, m->c.arch);
    REFUSE_IF(!a.pixels || !a.ids || !a.lens || !a.out_tlp || !a.out_top || !a.out_top_ids || !a.out_scored, "%s: null buffer", who);
    REFUSE_IF(a.pixel_fmt == CAP_PIX_IMAGE_STATE && ((uintptr_t)a.pixels & 15) != 0, "%s: the image state must be 16-byte aligned", who);
    REFUSE_IF(a.C < 1, "%s: captions_per_image %d must be at least 1", who, a.C);
    REFUSE_IF(a.L < 2, "%s: L = %d - a caption has BOS and at least one scored token", who, a.L);
    REFUSE_IF(!b2 && a.L - 1 > PREFILL_MAX_POS, "%s: L = %d exceeds the %d tokens a scoring pass takes (%d positions)", who, a.L, PREFILL_MAX_POS + 1,
              PREFILL_MAX_POS);
    REFUSE_IF(b2 && m->c.num_query_tokens + 1 + a.L - 1 > m->c.max_pos,
              "%s: %d prompt positions + %d caption positions exceed the OPT decoder's %d positions (max_pos)", who, m->c.num_query_tokens + 1,
              a.L - 1, m->c.max_pos);
    REFUSE_IF((long long)a.B * a.C > 0x7fffffffLL / a.L, "%s: %d x %d captions of %d tokens overflow the row index", who, a.B, a.C, a.L);
    REFUSE_IF(b2 && score_pass_captions(m, a.L) < 1,
              "%s: one caption of L = %d tokens is %d decoder rows and this handle's pass buffers hold %d (max_batch x prompt positions): "
              "create it with a larger max_batch", who, a.L, a.L - 2, m->c.max_batch * (m->c.num_query_tokens + 1));
    REFUSE_IF(!b2 && score_pass_captions(m, a.L) < 1,
              "%s: one caption of L = %d tokens is %d decoder rows and this handle's workspace holds %zu: create it with "
              "CapConfig.max_score_rows >= %d", who, a.L, a.L - 1, m->ws_rows, a.L - 1);
#undef REFUSE_IF
    return 0;
}

int cap_score_captions(CapHandle h, const void* pixels, int pixel_fmt, int B, const int32_t* ids, const int32_t* lens, int captions_per_image,
                       int L, float* out_token_logprobs, float* out_top_logprobs, int32_t* out_top_ids, int32_t* out_scored, void* stream) {
    Captioner* m = (Captioner*)h;
    const ScoreArgs a = {pixels, pixel_fmt, B, ids, lens, captions_per_image, L, out_token_logprobs, out_top_logprobs, out_top_ids, out_scored};
    TRY(validate_score(m, a, "cap_score_captions"));
    return (m->c.arch == CAP_ARCH_BLIP2 ? run_score_blip2 : run_score)(m, a, (hipStream_t)stream);
}
int cap_last_score_passes(CapHandle h) { return h ? ((Captioner*)h)->last_score_passes : -1; }
int cap_score_pass_captions(CapHandle h, int L) {
    Captioner* m = (Captioner*)h;
    if (!m || L < 2) return -1;
    if (m->c.arch == CAP_ARCH_BLIP2) { if (L - 1 > m->c.max_len) return -1; }
    else if (m->c.arch != CAP_ARCH_BLIP || L - 1 > PREFILL_MAX_POS || L > m->c.max_len) return -1;
    return (int)std::min<size_t>(score_pass_captions(m, L), 0x7fffffff);
}

int cap_generate_groups(CapHandle h, const void* pixels, int pixel_fmt, int B, int num_beams, int num_beam_groups, int max_len,
                        float length_penalty, int32_t* out_ids, int32_t* out_len, float* out_scores, void* stream) {
    CapGenerateArgs a = request_of(pixels, pixel_fmt, B, num_beams, max_len, length_penalty, out_ids, out_len);
    a.num_beam_groups = num_beam_groups; a.out_scores = out_scores;
    return generate(h, a, stream, "cap_generate_groups", num_beam_groups >= 1 ? nullptr : "num_beam_groups must be at least 1");
}

long long cap_g8_saturations(int reset) {
    if (hipDeviceSynchronize() != hipSuccess) { cap_set_error("cap_g8_saturations: device synchronisation failed"); return -1; }
    unsigned long long total = 0;
    if (cap_g8_clamped_gemm(&total, reset) != 0 || cap_g8_clamped_gemm_pp(&total, reset) != 0 || cap_g8_clamped_elementwise(&total, reset) != 0 ||
        cap_g8_clamped_attention(&total, reset) != 0 || cap_g8_clamped_decode_small(&total, reset) != 0 ||
        cap_g8_clamped_blip2_itm(&total, reset) != 0)
        return -1;
    return (long long)total;
}

int cap_profile_enable(CapHandle h, int on) {
    Captioner* m = (Captioner*)h;
    if (!m) return -1;
    for (auto& r : m->prof_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    m->prof_recs.clear();
    m->prof = on != 0;
    return 0;
}

int cap_profile_report(CapHandle h, char* buf, size_t buf_bytes) {
    Captioner* m = (Captioner*)h;
    if (!m || !buf) return -1;
    CAP_HIP_CHECK(hipDeviceSynchronize());
    struct Agg { long n = 0; double ms = 0, flops = 0, bytes = 0; };
    std::map<std::string, Agg> agg;
    for (auto& r : m->prof_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
        Agg& a = agg[r.tag];
        a.n++; a.ms += ms; a.flops += r.flops; a.bytes += r.bytes;
    }
    std::string out = "{";
    bool first = true;
    for (auto& kv : agg) {
        char line[512];
        snprintf(line, sizeof(line), "%s\"%s\": {\"launches\": %ld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}",
                 first ? "" : ", ", kv.first.c_str(), kv.second.n, kv.second.ms, kv.second.flops, kv.second.bytes);
        out += line;
        first = false;
    }
    out += "}";
    if (out.size() + 1 > buf_bytes) { cap_set_error("cap_profile_report: buffer too small (%zu needed)", out.size() + 1); return -1; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return 0;
}

// ---- single-kernel entry points.  dtype 2 (CAP_F32_SPLIT) = the split mode's convention: GEMM operands / kernel outputs
// that feed a GEMM are G8 (weights scaled by G8_WSCALE = 4096: cap_op_convert_weight), everything else is fp32.
static int dt_of(int dtype) { return dtype == CAP_BF16 ? CAP_DT_BF16 : dtype == CAP_F32_SPLIT ? CAP_DT_G8 : CAP_DT_F32; }
static int in_dt_of(int dtype) { return dtype == CAP_BF16 ? CAP_DT_BF16 : CAP_DT_F32; }
int cap_op_gemm(int dtype, const void* A, const void* W, const float* bias, const float* resid, void* C, int M, int N,
                int K, int gelu, int out_f32, int tile, void* stream) {
    GemmParams p = gemm_params(A, K, W, K, bias, C, N, M, N, K, gelu, out_f32);
    p.resid = resid; p.ldr = N;
#ifdef CAP_EXPERIMENTS
    if (tile == 9 || tile == 13 || tile == 14 || tile == 21) { p.aux = resid; p.resid = nullptr; }   // instrumented kernels: `resid` is the cycle-count buffer
#endif
    return launch_gemm(dt_of(dtype), p, tile, (hipStream_t)stream);
}
int cap_op_gemm_partial(int dtype, const void* A, const void* W, float* part, int M, int N, int K, int splitk, int tile,
                        void* stream) {
    const GemmParams p = gemm_params(A, K, W, K, nullptr, part, N, M, N, K, ACT_NONE, OUT_F32, EPI_PARTIAL, splitk);
    return launch_gemm(dt_of(dtype), p, tile, (hipStream_t)stream);
}
int cap_op_layernorm(int dtype, const float* in, const float* gamma, const float* beta, float eps, void* out_t,
                     float* out_f, int M, int D, void* stream) {
    return launch_layernorm(dt_of(dtype), in, D, gamma, beta, eps, out_t, out_f, M, D, (hipStream_t)stream);
}
int cap_op_vit_attention(int dtype, const void* qkv, void* ctx, int B, int N, int H, int impl, void* stream) {
    // dtype CAP_F32_SPLIT: impl 3 = G8 q|k|v in (what the split mode's qkv GEMM writes; the split-fp16 MFMA kernel), any other
    // impl = fp32 q|k|v in; the context is G8 either way
    if (dtype == CAP_F32_SPLIT && (impl == 3 || impl == 5))      // 5: the one-workgroup-per-unit kernel where 3 would pick the persistent one
        return launch_vit_attention(CAP_DT_G8, qkv, ctx, B, N, H, impl == 5 ? 5 : 0, (hipStream_t)stream, 64, 0, CAP_DT_G8);
    return launch_vit_attention(in_dt_of(dtype), qkv, ctx, B, N, H, impl, (hipStream_t)stream, 64, 0, dt_of(dtype));
}
int cap_op_vit_attention_hd(int dtype, const void* qkv, void* ctx, int B, int N, int H, int head_dim, int impl, void* stream) {
    // impl bit 8: causal mask (decoder prefill)
    return launch_vit_attention(in_dt_of(dtype), qkv, ctx, B, N, H, impl & 7, (hipStream_t)stream, head_dim, (impl >> 3) & 1,
                                dt_of(dtype));
}
int cap_op_generic_attention(int dtype, const void* qkv, void* ctx, int B, int N, int H, int head_dim, void* stream) {
    const long D = (long)H * head_dim;
    const int dt = in_dt_of(dtype);
    const char* base = (const char*)qkv;
    const size_t e = dt == CAP_DT_BF16 ? 2 : 4;
    return launch_generic_attention(dt, base, 3 * D, (long)N * 3 * D, base + D * e, 3 * D, (long)N * 3 * D, base + 2 * D * e, 3 * D,
                                    (long)N * 3 * D, ctx, D, (long)N * D, B, N, N, H, head_dim, -1, (hipStream_t)stream, dt_of(dtype));
}
int cap_op_itm_self_attention(int dtype, const void* qkv_q, const void* qkv_t, const int32_t* lens, void* ctx_q, void* ctx_t, int B,
                              int num_queries, int L, int H, void* stream) {
    return launch_itm_self_attention(in_dt_of(dtype), qkv_q, qkv_t, lens, ctx_q, ctx_t, B, num_queries, L, H, 64, (hipStream_t)stream, dt_of(dtype));
}
/* the attention launchers of the BLIP-2 / CoCa / sentence-encoder paths alone (tests/test_attention_kernels_gpu.py) */
int cap_op_attention(int dtype, const void* q, int64_t ldq, int64_t qbs, const void* k, int64_t ldk, int64_t kbs, const void* v, int64_t ldv,
                     int64_t vbs, void* out, int64_t ldo, int64_t obs, int B, int Lq, int Lk, int H, int head_dim, int causal_off, void* stream) {
    if (!q || !k || !v || !out) { cap_set_error("cap_op_attention: null pointer"); return -1; }
    return launch_generic_attention(in_dt_of(dtype), q, (long)ldq, (long)qbs, k, (long)ldk, (long)kbs, v, (long)ldv, (long)vbs, out, (long)ldo,
                                    (long)obs, B, Lq, Lk, H, head_dim, causal_off, (hipStream_t)stream, dt_of(dtype));
}
int cap_op_opt_decode_attention(int dtype, const void* qkv, void* kc, void* vc, void* out, int B, int T, int H, int Lmax, int past,
                                void* stream) {
    return launch_opt_decode_attention(in_dt_of(dtype), qkv, kc, vc, out, B, T, H, Lmax, past, (hipStream_t)stream, dt_of(dtype));
}
int cap_op_opt_prefix_attention(int dtype, const void* qkv, const void* kc, const void* vc, void* out, int n_caps, int n, int cap0, int C,
                                const int32_t* n_pos, int T, int H, int Lmax, int P, void* stream) {
    return launch_opt_prefix_attention(in_dt_of(dtype), qkv, kc, vc, out, n_caps, n, cap0, C, n_pos, T, H, Lmax, P, (hipStream_t)stream, dt_of(dtype));
}
int cap_op_opt_beam_decode_attention(int dtype, const void* qkv, void* kc, void* vc, void* out, int B, int K, int T, int H, int Lmax, int P,
                                     int past, const int32_t* anc, int anc_ld, void* stream) {
    return launch_opt_beam_decode_attention(in_dt_of(dtype), qkv, kc, vc, out, B, K, T, H, Lmax, P, past, anc, anc_ld, (hipStream_t)stream,
                                            dt_of(dtype));
}
int cap_op_kv_append(int dtype, const void* qkv, void* kc, void* vc, int B, int L, int T, int Lmax, int pos0, void* stream) {
    return launch_kv_append(in_dt_of(dtype), qkv, kc, vc, B, L, T, Lmax, pos0, (hipStream_t)stream);
}
/* the kernels of a prompt pass alone (tests/test_prefill_kernels_gpu.py) */
int cap_op_prefill_self_attention(int dtype, const float* part, int S, const float* bias, int part_ld, void* kbase, void* vbase, int kv_ld,
                                  void* out, int n_caps, int npos, int row0, int H, void* stream) {
    if (!part || !bias || !kbase || !vbase || !out) { cap_set_error("cap_op_prefill_self_attention: null pointer"); return -1; }
    return launch_prefill_self_attention(in_dt_of(dtype), part, S, bias, part_ld, kbase, vbase, kv_ld, out, dt_of(dtype), n_caps, npos, row0,
                                         H, (hipStream_t)stream);
}
int cap_op_opt_prefill_inputs(const float* proj, const float* tok, const float* pos, float* x, int B, int nq, int T, int bos, void* stream) {
    if (!proj || !tok || !pos || !x) { cap_set_error("cap_op_opt_prefill_inputs: null pointer"); return -1; }
    if (B < 1 || nq < 1 || T < 1 || bos < 0) { cap_set_error("cap_op_opt_prefill_inputs: B = %d, nq = %d, T = %d, bos = %d", B, nq, T, bos); return -1; }
    return launch_opt_prefill_inputs(proj, tok, pos, x, B, nq, T, bos, (hipStream_t)stream);
}
int cap_op_opt_token_inputs(const int32_t* seq, int seq_ld, int cur, const float* tok, const float* pos, float* x, int B, int T, int V,
                            void* stream) {
    if (!seq || !tok || !pos || !x) { cap_set_error("cap_op_opt_token_inputs: null pointer"); return -1; }
    if (B < 1 || T < 1 || V < 1 || cur < 0 || cur >= seq_ld) {
        cap_set_error("cap_op_opt_token_inputs: B = %d, T = %d, V = %d, column %d of %d", B, T, V, cur, seq_ld);
        return -1;
    }
    return launch_opt_token_inputs(seq, seq_ld, cur, tok, pos, x, B, T, V, (hipStream_t)stream);
}
int cap_op_rows_broadcast(int dtype, const float* src, float* dst_f, void* dst_t, int B, int n, int D, void* stream) {
    if (!src || !dst_f || !dst_t) { cap_set_error("cap_op_rows_broadcast: null pointer"); return -1; }
    if (B < 1 || n < 1 || D < 1 || (dtype == CAP_F32_SPLIT && D % 8 != 0)) {
        cap_set_error("cap_op_rows_broadcast: B = %d, n = %d, D = %d (G8 rows need D %% 8 == 0)", B, n, D);
        return -1;
    }
    return launch_rows_broadcast(dt_of(dtype), src, dst_f, dst_t, B, n, D, (hipStream_t)stream);
}
int cap_op_dequant_i8_rowmajor(const void* packed, void* dst_bf16, int rows, int cols, void* stream) {
    if (!packed || !dst_bf16) { cap_set_error("cap_op_dequant_i8_rowmajor: null pointer"); return -1; }
    if (rows < 1 || cols < 1) { cap_set_error("cap_op_dequant_i8_rowmajor: rows = %d, cols = %d", rows, cols); return -1; }
    return launch_dequant_i8_rowmajor(packed, dst_bf16, rows, cols, (hipStream_t)stream);
}
int cap_op_scale_cols(float* part, const float* scale, int M, int N, void* stream) {
    if (!part || !scale) { cap_set_error("cap_op_scale_cols: null pointer"); return -1; }
    if (M < 1 || N < 1) { cap_set_error("cap_op_scale_cols: M = %d, N = %d", M, N); return -1; }
    return launch_scale_cols(part, scale, M, N, (hipStream_t)stream);
}
int cap_op_pool_attention(int dtype, const float* qp, const void* kv, void* out, int B, int N, int Q, int E, int heads, void* stream) {
    return launch_pool_attention(in_dt_of(dtype), qp, kv, out, B, N, Q, E, heads, (hipStream_t)stream, dt_of(dtype));
}
int cap_op_text_attention(int dtype, const void* qkv, const int32_t* lens, void* ctx, int B, int L, int H, int head_dim, void* stream) {
    if (dtype != CAP_F32 && dtype != CAP_BF16) { cap_set_error("cap_op_text_attention: the sentence encoder takes CAP_F32 or CAP_BF16"); return -1; }
    return launch_text_attention(in_dt_of(dtype), qkv, lens, ctx, B, L, H, head_dim, (hipStream_t)stream);
}
int cap_crop_resize_tables(const int32_t* rects, const int32_t* geom, int n, int S, int KH, int KV, int32_t* hb, int32_t* hk,
                           int32_t* vb, int32_t* vk, void* stream) {
    return launch_crop_resize_tables(rects, geom, n, S, KH, KV, hb, hk, vb, vk, (hipStream_t)stream);
}
int cap_crop_resize_u8(const uint8_t* frame, int H, int W, int bgr, const int32_t* rects, const int32_t* hb, const int32_t* hk,
                       int KH, const int32_t* vb, const int32_t* vk, int KV, int n, int S, uint8_t* out, void* stream) {
    return launch_crop_resize_u8(frame, H, W, bgr, rects, hb, hk, KH, vb, vk, KV, n, S, out, (hipStream_t)stream);
}
int cap_crop_resize_u8_frames(const uint8_t* packed, const int64_t* frames, int bgr, const int32_t* rects, const int32_t* hb, const int32_t* hk,
                              int KH, const int32_t* vb, const int32_t* vk, int KV, int n, int S, uint8_t* out, void* stream) {
    if (!frames) { cap_set_error("crop_resize_frames: null frame table"); return -1; }
    return launch_crop_resize_u8(packed, 0, 0, bgr, rects, hb, hk, KH, vb, vk, KV, n, S, out, (hipStream_t)stream, (const long long*)frames);
}
int cap_op_reduce_layernorm(int dtype, const float* part, int S, const float* bias, const float* resid, const float* gamma,
                            const float* beta, float eps, void* out_t, float* out_f, float* y_out, int M, int D,
                            int per_row_block, void* stream) {
    return launch_reduce_layernorm(dt_of(dtype), part, S, bias, resid, gamma, beta, eps, out_t, out_f, y_out, M, D,
                                   (hipStream_t)stream, per_row_block != 0);
}
int cap_op_gemm_skinny(const void* A, const void* W, const float* bias, int act, void* out, float* part, int M, int N, int K,
                       void* stream) {
    return launch_gemm_skinny(A, K, W, K, bias, act, out, N, part, M, N, K, (hipStream_t)stream);
}
int cap_op_gemm_skinny_slices(int N, int K, int finished) { return skinny_plan(N, K, finished != 0); }
int cap_op_quant_i8_pack(const float* W, void* packed, float* scale, int rows, int cols, void* stream) {
    return launch_quant_i8_pack(W, packed, scale, rows, cols, (hipStream_t)stream);
}
int cap_op_gemm_skinny_i8(const void* A, const void* packed, const float* scale, const float* bias, int act, void* out, float* part, int M,
                          int N, int K, void* stream) {
    return launch_gemm_skinny_i8(A, K, packed, scale, bias, act, out, N, part, M, N, K, (hipStream_t)stream);
}
int cap_op_gemm_skinny_i8_slices(int N, int K, int finished) { return skinny_i8_plan(N, K, finished != 0); }
int cap_op_decode_attention(int dtype, const void* q, const void* kbase, const void* vbase, const int32_t* anc,
                            int anc_ld, int rows_per_kv, int kv_ld, int n_keys, void* out, int R, int H, int impl,
                            void* stream) {
    // impl bit 16: kbase / vbase are KV16 blocks (cap_op_pack_kv16) whose row 0 is the launch's first K/V row
    DecodeAttn a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.kbase = kbase; a.vbase = vbase; a.anc = anc; a.anc_ld = anc_ld; a.rows_per_kv = rows_per_kv; a.kv_ld = kv_ld;
    a.n_keys = n_keys; a.out = out; a.R = R; a.H = H; a.impl = impl & 15; a.out_dtype = dt_of(dtype); a.kv16 = (impl >> 4) & 1;
    return launch_decode_attention(in_dt_of(dtype), a, (hipStream_t)stream);
}
int cap_op_decode_attention_fused(int dtype, const float* q_part, int q_S, const float* q_bias, int q_ld, int q_col0, int append_kv,
                                  void* kbase, void* vbase, const int32_t* anc, int anc_ld, int rows_per_kv, int kv_ld, int n_keys,
                                  void* out, int R, int H, int impl, void* stream) {
    if (!q_part || !kbase || !vbase || !out) { cap_set_error("cap_op_decode_attention_fused: null pointer"); return -1; }
    DecodeAttn a;
    memset(&a, 0, sizeof(a));
    a.kbase = kbase; a.vbase = vbase; a.anc = anc; a.anc_ld = anc_ld; a.rows_per_kv = rows_per_kv; a.kv_ld = kv_ld;
    a.n_keys = n_keys; a.out = out; a.R = R; a.H = H; a.impl = impl & 15; a.out_dtype = dt_of(dtype); a.kv16 = (impl >> 4) & 1;
    a.q_part = q_part; a.q_S = q_S; a.q_bias = q_bias; a.q_ld = q_ld; a.q_col0 = q_col0; a.append_kv = append_kv;
    return launch_decode_attention(in_dt_of(dtype), a, (hipStream_t)stream);
}
/* the row-wise decode kernels with the compacted loop's live-row count (tests/test_pass_size_decode_kernels_gpu.py) */
int cap_op_gemm_live(int dtype, const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int gelu, int out_f32,
                     int tile, const int32_t* n_live, void* stream) {
    GemmParams p = gemm_params(A, K, W, K, bias, C, N, M, N, K, gelu, out_f32);
    p.ldr = N; p.m_live = n_live;
    return launch_gemm(dt_of(dtype), p, tile, (hipStream_t)stream);
}
int cap_op_layernorm_live(int dtype, const float* in, const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int M,
                          int D, const int32_t* n_live, void* stream) {
    return launch_layernorm(dt_of(dtype), in, D, gamma, beta, eps, out_t, out_f, M, D, (hipStream_t)stream, n_live);
}
int cap_op_decode_attention_live(int dtype, const float* q_part, int q_S, const float* q_bias, int q_ld, int q_col0, int append_kv,
                                 void* kbase, void* vbase, int kv_ld, int n_keys, void* out, int R, int H, const int32_t* live,
                                 const int32_t* n_live, int form, void* stream) {
    if (!q_part || !kbase || !vbase || !out) { cap_set_error("cap_op_decode_attention_live: null pointer"); return -1; }
    DecodeAttn a;
    memset(&a, 0, sizeof(a));
    a.kbase = kbase; a.vbase = vbase; a.rows_per_kv = 1; a.kv_ld = kv_ld; a.n_keys = n_keys; a.out = out; a.R = R; a.H = H;
    a.out_dtype = dt_of(dtype);
    a.q_part = q_part; a.q_S = q_S; a.q_bias = q_bias; a.q_ld = q_ld; a.q_col0 = q_col0; a.append_kv = append_kv;
    a.map.live = live; a.map.n = n_live; a.form = form;
    return launch_decode_attention(in_dt_of(dtype), a, (hipStream_t)stream);
}
/* the small-batch decode kernels alone (tests/test_small_kernels_gpu.py): the launchers' own structs, filled field for field */
static SmallLN small_ln_of(const CapSmallLN& l) {
    SmallLN o;
    memset(&o, 0, sizeof(o));
    o.part = l.part; o.S = l.S; o.bias = l.bias; o.resid = l.resid; o.gamma = l.gamma; o.beta = l.beta; o.eps = l.eps;
    o.x_out = l.x_out; o.x_is_sum = l.x_is_sum;
    return o;
}
int cap_op_small_gemm(int dtype, const CapSmallGemm* a, void* stream) {
    if (!a || !a->W) { cap_set_error("cap_op_small_gemm: null pointer"); return -1; }
    SmallGemm g;
    memset(&g, 0, sizeof(g));
    g.W = a->W; g.A = a->A; g.R = a->R; g.N = a->N; g.K = a->K; g.S = a->S; g.pro = a->pro; g.epi = a->epi; g.nchain = a->nchain;
    g.ln = small_ln_of(a->ln);
    g.sa.qkv_part = a->sa.qkv_part; g.sa.qkv_bias = a->sa.qkv_bias; g.sa.qkv_S = a->sa.qkv_S; g.sa.kc = a->sa.kc; g.sa.vc = a->sa.vc;
    g.sa.anc = a->sa.anc; g.sa.anc_ld = a->sa.anc_ld; g.sa.kv_ld = a->sa.kv_ld; g.sa.n_keys = a->sa.n_keys; g.sa.H = a->sa.H;
    g.sa.skip = a->sa.skip;
    g.out_part = a->out_part; g.bias = a->bias; g.act = a->act; g.out = a->out; g.ldc = a->ldc;
    const bool ok = (g.pro != SMALL_PRO_GLOBAL || g.A) && (g.pro != SMALL_PRO_LN || (g.ln.part && g.ln.gamma && g.ln.beta)) &&
                    (g.pro != SMALL_PRO_SELFATTN || (g.sa.qkv_part && g.sa.qkv_bias && g.sa.kc && g.sa.vc)) &&
                    (g.epi == SMALL_EPI_PARTIAL ? g.out_part != nullptr : g.out != nullptr);
    if (!ok) { cap_set_error("cap_op_small_gemm: null pointer"); return -1; }
    return launch_small_gemm(dt_of(dtype), g, (hipStream_t)stream);
}
int cap_op_small_cross(int dtype, const CapSmallCross* a, void* stream) {
    if (!a || !a->W || !a->bias || !a->ln.part || !a->ln.gamma || !a->ln.beta || !a->kbase || !a->vbase || !a->out) {
        cap_set_error("cap_op_small_cross: null pointer");
        return -1;
    }
    SmallCross x;
    memset(&x, 0, sizeof(x));
    x.W = a->W; x.bias = a->bias; x.R = a->R; x.D = a->D; x.H = a->H; x.S = a->S;
    x.ln = small_ln_of(a->ln);
    x.kbase = a->kbase; x.vbase = a->vbase; x.kv_row0 = a->kv_row0;
    x.rows_per_kv = a->rows_per_kv; x.kv_ld = a->kv_ld; x.n_keys = a->n_keys; x.kv_kind = a->kv_kind; x.skip = a->skip; x.out = a->out;
    return launch_small_cross(dt_of(dtype), x, (hipStream_t)stream);
}
int cap_op_gemm_crosskv(int dtype, const void* A, const void* W, const float* bias, void* cache, int n_img, int tokens, int heads,
                        int layers, int K, int kv16, void* stream) {
    GemmParams p = gemm_params(A, K, W, K, bias, cache, 0, n_img * tokens, layers * 2 * heads * 64, K, ACT_NONE, OUT_F32, EPI_CROSSKV);
    p.p0 = tokens; p.p1 = heads; p.p2 = n_img; p.kv16 = kv16;
    return launch_gemm(dt_of(dtype), p, 0, (hipStream_t)stream);
}
/* launch_gemm with the whole of GemmParams (tests/test_gemm_epilogues_gpu.py).  launch_gemm checks shapes and alignment, not what an
   epilogue computes its addresses from: that is refused here, before anything is launched */
int cap_op_gemm_epi(int dtype, const CapGemmEpi* a, void* stream) {
    if (!a || !a->A || !a->W || !a->C) { cap_set_error("cap_op_gemm_epi: null pointer (A / W / C)"); return -1; }
    const long long M = a->M, N = a->N;
    switch (a->epi) {
        case EPI_STORE:
            if (a->ldc < a->N) { cap_set_error("cap_op_gemm_epi: store: ldc=%d < N=%d", a->ldc, a->N); return -1; }
            break;
        case EPI_PATCH:
            if (!a->aux) { cap_set_error("cap_op_gemm_epi: patch: null aux (the position table)"); return -1; }
            if (a->p0 < 1 || M % a->p0 != 0) { cap_set_error("cap_op_gemm_epi: patch: M=%d is not whole images of p0=%d patches", a->M, a->p0); return -1; }
            if (a->ldc < a->N) { cap_set_error("cap_op_gemm_epi: patch: ldc=%d < N=%d", a->ldc, a->N); return -1; }
            break;
        case EPI_CROSSKV:
            if (a->p0 < 1 || a->p1 < 1 || a->p2 < 1) {
                cap_set_error("cap_op_gemm_epi: cross K/V: p0=%d tokens, p1=%d heads, p2=%d images must be positive", a->p0, a->p1, a->p2);
                return -1;
            }
            if (M != (long long)a->p0 * a->p2) { cap_set_error("cap_op_gemm_epi: cross K/V: M=%d is not p0 * p2 = %d * %d", a->M, a->p0, a->p2); return -1; }
            if (N % (2LL * a->p1 * 64) != 0) { cap_set_error("cap_op_gemm_epi: cross K/V: N=%d is not whole layers of 2 * p1=%d * 64 columns", a->N, a->p1); return -1; }
            break;
        case EPI_QKVCACHE:
            if (!a->C2) { cap_set_error("cap_op_gemm_epi: q|k|v: null C2 (the cache)"); return -1; }
            if (a->p1 < 1 || N != 3LL * a->p1 * 64) { cap_set_error("cap_op_gemm_epi: q|k|v: N=%d is not 3 * p1=%d * 64", a->N, a->p1); return -1; }
            if (a->p0 < a->M) { cap_set_error("cap_op_gemm_epi: q|k|v: the cache holds p0=%d rows, M=%d", a->p0, a->M); return -1; }
            if (a->p3 < 0 || a->p3 >= a->p2) { cap_set_error("cap_op_gemm_epi: q|k|v: position p3=%d outside [0, p2=%d)", a->p3, a->p2); return -1; }
            break;
        case EPI_PARTIAL:
            if (a->splitk < 1) { cap_set_error("cap_op_gemm_epi: split-K: splitk=%d < 1", a->splitk); return -1; }
            // (the slice index travels in p3 and the kernels with a slice loop set it themselves: the one without reads the host's)
            if (a->p3 != 0) { cap_set_error("cap_op_gemm_epi: split-K: p3=%d must be 0 (the kernels number the slices)", a->p3); return -1; }
            if (a->ldc < a->N) { cap_set_error("cap_op_gemm_epi: split-K: ldc=%d < N=%d", a->ldc, a->N); return -1; }
            break;
        default:
            cap_set_error("cap_op_gemm_epi: unknown epi %d (0 store, 1 patch, 2 cross K/V, 3 q|k|v, 4 split-K)", a->epi);
            return -1;
    }
    GemmParams p = gemm_params(a->A, a->lda, a->W, a->ldw, a->bias, a->C, a->ldc, a->M, a->N, a->K, a->gelu, a->out_f32, a->epi, a->splitk);
    p.C2 = a->C2; p.aux = a->aux; p.p0 = a->p0; p.p1 = a->p1; p.p2 = a->p2; p.p3 = a->p3; p.kv16 = a->kv16; p.m_live = a->m_live;
    return launch_gemm(dt_of(dtype), p, a->tile, (hipStream_t)stream);
}
int cap_op_pack_kv16(const float* src, void* dst, size_t n_rows, void* stream) {
    return launch_pack_kv16(src, dst, n_rows, (hipStream_t)stream);
}
static int op_image_state_layout(const char* who, int kind, int slots, int heads, int tokens, ImageStateLayout& L) {
    if (kind < 0 || kind > 2 || slots < 1 || heads < 1 || tokens < 1 || (long long)heads * tokens > 0x3fffffff || slots > 0x3fffffff) {
        cap_set_error("%s: kind %d (0 fp32, 1 bf16, 2 KV16), %d slots, %d heads, %d tokens", who, kind, slots, heads, tokens);
        return -1;
    }
    L = {2 * slots, heads * tokens, kind == 0 ? 256 : 128, kind == 2 ? 1 : 0};
    return 0;
}
int cap_op_image_state_pack(int kind, int slots, int heads, int tokens, int B, const void* cache, void* state, void* stream) {
    ImageStateLayout L;
    TRY(op_image_state_layout("cap_op_image_state_pack", kind, slots, heads, tokens, L));
    return launch_image_state_pack(L, B, cache, state, (hipStream_t)stream);
}
int cap_op_image_state_unpack(int kind, int slots, int heads, int tokens, int B, void* cache, const void* state, void* stream) {
    ImageStateLayout L;
    TRY(op_image_state_layout("cap_op_image_state_unpack", kind, slots, heads, tokens, L));
    return launch_image_state_unpack(L, B, cache, state, (hipStream_t)stream);
}
int cap_op_beam_candidates(const float* logits, int ld, int V, int B, int K, int legacy_raw, int masked_id, float* out_val,
                           int32_t* out_idx, void* stream) {
    if (!logits || !out_val || !out_idx || B < 1 || K < 1 || V < 1 || ld < V) { cap_set_error("cap_op_beam_candidates: bad arguments"); return -1; }
    void* st = nullptr;
    CAP_HIP_CHECK(hipMalloc(&st, beam_state_bytes(B, K, 4)));
    int rc = beam_candidates_only(st, logits, ld, V, B, K, legacy_raw ? BEAM_LEGACY_RAW : BEAM_HF_V5, masked_id, out_val, out_idx,
                                  (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -1;
    (void)hipFree(st);
    return rc;
}
// The beam search alone over a caller-owned state block (tests/test_beam_search_gpu.py): thin wrappers of the launchers the
// generate paths use.  One argument check for all of them; `what` names the entry in the message.
static int beam_op_args(const char* what, const void* state, int B, int K, int max_len) {
    if (!state) { cap_set_error("%s: state is null", what); return -1; }
    if (K < 1 || K > 8) { cap_set_error("%s: K = %d beams (1 <= K <= 8)", what, K); return -1; }
    if (B < 1 || max_len < 2) { cap_set_error("%s: B = %d, max_len = %d (B >= 1, max_len >= 2)", what, B, max_len); return -1; }
    return 0;
}
size_t cap_op_beam_state_bytes(int B, int K, int max_len) {
    if (K < 1 || K > 8) { cap_set_error("cap_op_beam_state_bytes: K = %d beams (1 <= K <= 8)", K); return 0; }
    if (B < 1 || max_len < 2) { cap_set_error("cap_op_beam_state_bytes: B = %d, max_len = %d (B >= 1, max_len >= 2)", B, max_len); return 0; }
    return beam_state_bytes(B, K, max_len);
}
int cap_op_beam_init(void* state, int B, int K, int max_len, int bos, int pad, int eos, int mode, void* stream) {
    TRY(beam_op_args("cap_op_beam_init", state, B, K, max_len));
    if (mode != BEAM_HF_V5 && mode != BEAM_LEGACY_RAW) { cap_set_error("cap_op_beam_init: mode = %d (0: HF v5, 1: legacy raw)", mode); return -1; }
    return launch_beam_init(state, B, K, max_len, bos, pad, eos, (hipStream_t)stream, mode);
}
// What the three cap_op_beam_step* forms check alike, and the BeamStep they fill
static int beam_op_step(const char* f, BeamStep* st, void* state, const float* logits, int ld, int V, int B, int K, int max_len, int cur_len,
                        int eos, float length_penalty, int32_t* anc, int anc_ld, int mode, int min_len) {
    TRY(beam_op_args(f, state, B, K, max_len));
    if (!logits) { cap_set_error("%s: logits is null", f); return -1; }
    if (V < 1 || ld < V) { cap_set_error("%s: ld = %d, V = %d (ld >= V >= 1)", f, ld, V); return -1; }
    // cur_len is the position the step writes (the running sequences hold cur_len tokens, BOS included): step t = cur_len - 1
    if (cur_len - 1 < 0 || cur_len - 1 >= max_len - 1) {
        cap_set_error("%s: cur_len = %d (step cur_len - 1 must satisfy 0 <= step < max_len - 1 = %d)", f, cur_len, max_len - 1);
        return -1;
    }
    if (anc && anc_ld < 1) { cap_set_error("%s: anc_ld = %d with an ancestry table (anc_ld >= 1)", f, anc_ld); return -1; }
    if (mode != BEAM_HF_V5 && mode != BEAM_LEGACY_RAW) { cap_set_error("%s: mode = %d (0: HF v5, 1: legacy raw)", f, mode); return -1; }
    st->state = state; st->logits = logits; st->ld = ld; st->V = V; st->B = B; st->K = K; st->max_len = max_len; st->cur_len = cur_len;
    st->eos = eos; st->length_penalty = length_penalty; st->anc = anc; st->anc_ld = anc_ld; st->mode = mode; st->min_len = min_len;
    return 0;
}
int cap_op_beam_step(void* state, const float* logits, int ld, int V, int B, int K, int max_len, int cur_len, int eos,
                     float length_penalty, int32_t* anc, int anc_ld, int mode, int min_len, void* stream) {
    BeamStep st{};
    TRY(beam_op_step("cap_op_beam_step", &st, state, logits, ld, V, B, K, max_len, cur_len, eos, length_penalty, anc, anc_ld, mode, min_len));
    return launch_beam_step(st, (hipStream_t)stream);
}
int cap_op_beam_finalize(void* state, int B, int K, int max_len, int32_t* out_ids, int32_t* out_len, float* out_scores, void* stream) {
    TRY(beam_op_args("cap_op_beam_finalize", state, B, K, max_len));
    if (!out_ids) { cap_set_error("cap_op_beam_finalize: out_ids is null"); return -1; }
    return launch_beam_finalize(state, B, K, max_len, out_ids, out_len, out_scores, (hipStream_t)stream);
}
int cap_op_beam_peek(void* state, int B, int K, int max_len, int parity, int32_t* run_tokens, float* run_scores, int32_t* active,
                     void* stream) {
    TRY(beam_op_args("cap_op_beam_peek", state, B, K, max_len));
    if (!run_tokens || !run_scores || !active) { cap_set_error("cap_op_beam_peek: an output pointer is null"); return -1; }
    if (parity != 0 && parity != 1) { cap_set_error("cap_op_beam_peek: parity = %d (0 or 1)", parity); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CAP_HIP_CHECK(hipMemcpyAsync(run_tokens, beam_running_tokens_p(state, B, K, max_len, parity), (size_t)B * K * max_len * 4,
                                 hipMemcpyDeviceToDevice, s));
    CAP_HIP_CHECK(hipMemcpyAsync(run_scores, beam_running_scores_p(state, B, K, max_len, parity), (size_t)B * K * 4,
                                 hipMemcpyDeviceToDevice, s));
    CAP_HIP_CHECK(hipMemcpyAsync(active, beam_active_flag_p(state, B, K, max_len), 4, hipMemcpyDeviceToDevice, s));
    return 0;
}
int cap_op_target_logprob(const float* logits, int ld, int V, int rows, const int32_t* targets, const int32_t* live, float* out_target,
                          float* out_top, int32_t* out_top_id, void* stream) {
    // one position per "caption": row r's target is targets[r], it is live when live[r] > 0
    return launch_target_logprob(logits, ld, V, rows, 0, 1, targets, 1, live, out_target, out_top, out_top_id, 1, (hipStream_t)stream);
}

// What the five cap_op_select_* forms check alike, and the rows of the SelectStep they fill (seq rows of max_len tokens)
static int select_op_rows(const char* f, SelectStep* st, const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad,
                          int32_t* finished, const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths) {
    if (!logits || !finished || !seq || !lengths) { cap_set_error("%s: null buffer (logits, finished, seq and lengths are required)", f); return -1; }
    if (R < 1 || V < 1 || ld < V || t < 0 || t + 1 >= max_len || (live != nullptr) != (n_live != nullptr)) {
        cap_set_error("%s: bad arguments (R = %d >= 1; ld = %d >= V = %d >= 1; 0 <= t = %d < max_len - 1 = %d; live and n_live together)", f, R, ld,
                      V, t, max_len - 1);
        return -1;
    }
    st->logits = logits; st->ld = ld; st->V = V; st->seq = seq; st->seq_ld = max_len; st->t = t; st->max_len = max_len; st->eos = eos;
    st->pad = pad; st->finished = finished; st->out_len = lengths; st->R = R; st->map.live = live; st->map.n = n_live;
    return 0;
}
int cap_op_select_logprob(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int min_len, int force_eos,
                          int32_t* finished, const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths,
                          float* logprobs, int lp_ld, int32_t* scored, void* stream) {
    const char* f = "cap_op_select_logprob";
    SelectStep st{};
    TRY(select_op_rows(f, &st, logits, ld, V, R, t, max_len, eos, pad, finished, live, n_live, seq, lengths));
    if ((logprobs != nullptr) != (scored != nullptr)) { cap_set_error("%s: logprobs and scored come together (both or neither)", f); return -1; }
    st.min_len = min_len; st.force_eos = force_eos;
    st.logprobs = logprobs; st.lp_ld = lp_ld; st.lp_col = t; st.scored = scored;
    return launch_select_step(st, (hipStream_t)stream);
}
int cap_op_select_vocab(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int min_len, int force_eos,
                        int32_t* finished, const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths,
                        float* logprobs, int lp_ld, int32_t* scored, float* vocab_acc, int acc_ld, void* stream) {
    const char* f = "cap_op_select_vocab";
    SelectStep st{};
    TRY(select_op_rows(f, &st, logits, ld, V, R, t, max_len, eos, pad, finished, live, n_live, seq, lengths));
    if (!logprobs || !scored || !vocab_acc) { cap_set_error("%s: null buffer (logprobs, scored and vocab_acc are required)", f); return -1; }
    st.min_len = min_len; st.force_eos = force_eos;
    st.logprobs = logprobs; st.lp_ld = lp_ld; st.lp_col = t; st.scored = scored;
    st.vocab_acc = vocab_acc; st.acc_ld = acc_ld;
    return launch_select_step(st, (hipStream_t)stream);
}
// The banned forms alone (tests/test_bad_words_kernels_gpu.py): the set comes as the device arrays the kernels read (ops.h, BanSet),
// and ban_bits is required.
int cap_op_ban_words(int V) { return V < 1 ? -1 : ban_words(V); }
int cap_op_select_banned(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int32_t* finished,
                         const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths, const uint32_t* ban_bits,
                         const int32_t* ban_multi, int n_multi, int hist0, void* stream) {
    const char* f = "cap_op_select_banned";
    SelectStep st{};
    TRY(select_op_rows(f, &st, logits, ld, V, R, t, max_len, eos, pad, finished, live, n_live, seq, lengths));
    if (!ban_bits) { cap_set_error("%s: ban_bits is required", f); return -1; }
    st.ban.bits = ban_bits; st.ban.multi = ban_multi; st.ban.n_multi = n_multi; st.hist0 = hist0;
    return launch_select_step(st, (hipStream_t)stream);
}
int cap_op_beam_step_banned(void* state, const float* logits, int ld, int V, int B, int K, int max_len, int cur_len, int eos,
                            float length_penalty, int32_t* anc, int anc_ld, int mode, int min_len, const uint32_t* ban_bits,
                            const int32_t* ban_multi, int n_multi, void* stream) {
    const char* f = "cap_op_beam_step_banned";
    BeamStep st{};
    TRY(beam_op_step(f, &st, state, logits, ld, V, B, K, max_len, cur_len, eos, length_penalty, anc, anc_ld, mode, min_len));
    if (!ban_bits) { cap_set_error("%s: ban_bits is required", f); return -1; }
    st.ban.bits = ban_bits; st.ban.multi = ban_multi; st.ban.n_multi = n_multi;
    return launch_beam_step(st, (hipStream_t)stream);
}
// The processed forms alone (tests/test_repeat_controls_kernels_gpu.py): cap_op_select_banned / cap_op_beam_step_banned with the
// repetition controls; ban_bits may be NULL (no static bitmap; n_multi must then be 0).  The launchers check the values; the limit on
// the virtual context is these entry points' own.
static int repeat_op_ctl(const char* f, float penalty, int ngram, int vn, int vtok, int vbos, const uint32_t* ban_bits, const int32_t* ban_multi,
                         int n_multi, RepeatCtl* ctl, BanSet* ban) {
    if (vn > 4096) { cap_set_error("%s: %d virtual context tokens (0 .. 4096)", f, vn); return -1; }
    ctl->penalty = penalty; ctl->ngram = ngram; ctl->vn = vn; ctl->vtok = vtok; ctl->vbos = vbos;
    ban->bits = ban_bits; ban->multi = ban_multi; ban->n_multi = n_multi;
    return 0;
}
int cap_op_select_processed(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int32_t* finished,
                            const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths, const uint32_t* ban_bits,
                            const int32_t* ban_multi, int n_multi, int hist0, float penalty, int ngram, int vn, int vtok, int vbos,
                            void* stream) {
    const char* f = "cap_op_select_processed";
    SelectStep st{};
    TRY(select_op_rows(f, &st, logits, ld, V, R, t, max_len, eos, pad, finished, live, n_live, seq, lengths));
    TRY(repeat_op_ctl(f, penalty, ngram, vn, vtok, vbos, ban_bits, ban_multi, n_multi, &st.ctl, &st.ban));
    st.hist0 = hist0;
    return launch_select_step(st, (hipStream_t)stream);
}
// The sampled form alone (tests/test_sampling_kernels_gpu.py): cap_op_select_processed with the draw in place of the arg-max.
int cap_op_select_sampled(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int32_t* finished,
                          const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths, const uint32_t* ban_bits,
                          const int32_t* ban_multi, int n_multi, int hist0, float penalty, int ngram, int vn, int vtok, int vbos,
                          float temperature, int top_k, float top_p, uint64_t seed, const uint64_t* keys, int draw, int32_t* out_kept,
                          void* stream) {
    const char* f = "cap_op_select_sampled";
    SelectStep st{};
    TRY(select_op_rows(f, &st, logits, ld, V, R, t, max_len, eos, pad, finished, live, n_live, seq, lengths));
    TRY(repeat_op_ctl(f, penalty, ngram, vn, vtok, vbos, ban_bits, ban_multi, n_multi, &st.ctl, &st.ban));
    st.hist0 = hist0;
    st.sample = 1; st.sc.temperature = temperature; st.sc.top_k = top_k; st.sc.top_p = top_p; st.sc.seed = seed;
    st.keys = keys; st.draw = draw; st.out_kept = out_kept;
    return launch_select_step(st, (hipStream_t)stream);
}
int cap_op_beam_step_processed(void* state, const float* logits, int ld, int V, int B, int K, int max_len, int cur_len, int eos,
                               float length_penalty, int32_t* anc, int anc_ld, const uint32_t* ban_bits, const int32_t* ban_multi,
                               int n_multi, float penalty, int ngram, int vn, int vtok, int vbos, void* stream) {
    const char* f = "cap_op_beam_step_processed";
    BeamStep st{};
    TRY(beam_op_step(f, &st, state, logits, ld, V, B, K, max_len, cur_len, eos, length_penalty, anc, anc_ld, BEAM_HF_V5, 0));
    TRY(repeat_op_ctl(f, penalty, ngram, vn, vtok, vbos, ban_bits, ban_multi, n_multi, &st.ctl, &st.ban));
    return launch_beam_step(st, (hipStream_t)stream);
}
int cap_op_vocab_group_threshold(const float* acc, int acc_ld, int V, int N, const int32_t* group_rows, int M, const int32_t* group_off,
                                 int G, float th, int K, int32_t* out_ids, float* out_prob, int32_t* out_count, void* stream) {
    const char* f = "cap_op_vocab_group_threshold";
    if (!acc || !group_off || !out_ids || !out_prob || !out_count || (M > 0 && !group_rows)) { cap_set_error("%s: null buffer", f); return -1; }
    if (V < 1 || acc_ld < V || N < 1 || M < 0 || G < 1) {
        cap_set_error("%s: need V >= 1, acc_ld >= V, N >= 1, M >= 0, G >= 1 (got V %d, acc_ld %d, N %d, M %d, G %d)", f, V, acc_ld, N, M, G);
        return -1;
    }
    if (!(th == th) || th - th != 0.f) { cap_set_error("%s: th must be finite", f); return -1; }
    if (K < 1) { cap_set_error("%s: K (%d) must be at least 1", f, K); return -1; }
    // the CSR arrays are checked on the host before any kernel indexes with them
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> off((size_t)G + 1), rows((size_t)M);
    CAP_HIP_CHECK(hipMemcpyAsync(off.data(), group_off, off.size() * 4, hipMemcpyDeviceToHost, s));
    if (M > 0) CAP_HIP_CHECK(hipMemcpyAsync(rows.data(), group_rows, rows.size() * 4, hipMemcpyDeviceToHost, s));
    CAP_HIP_CHECK(hipStreamSynchronize(s));
    if (off[0] != 0 || off[G] != M) { cap_set_error("%s: group_off must start at 0 and end at M = %d (got %d .. %d)", f, M, off[0], off[G]); return -1; }
    for (int g = 0; g < G; ++g)
        if (off[g + 1] < off[g]) { cap_set_error("%s: group_off is not monotone at group %d (%d > %d)", f, g, off[g], off[g + 1]); return -1; }
    for (int j = 0; j < M; ++j)
        if (rows[j] < 0 || rows[j] >= N) { cap_set_error("%s: group_rows[%d] = %d is outside the N = %d rows", f, j, rows[j], N); return -1; }
    return launch_vocab_group_threshold(acc, acc_ld, V, group_rows, group_off, G, th, K, out_ids, out_prob, out_count, s);
}
/* the helper kernels of elementwise.hip alone (tests/test_elementwise_kernels_gpu.py): pointer and count checks here, every
 * width / layout rule is the launcher's to take or refuse */
int cap_op_embed(int dtype, const int32_t* seq, int seq_ld, int t, const float* word, const float* pos, const float* gamma,
                 const float* beta, float eps, void* out_t, float* out_f, float* y_out, int R, int D, const int32_t* live,
                 const int32_t* n_live, void* stream) {
    if (!seq || !word || !pos || !gamma || !beta || (live != nullptr) != (n_live != nullptr)) { cap_set_error("cap_op_embed: null pointer"); return -1; }
    if (R < 1 || D < 1 || t < 0 || t >= seq_ld) { cap_set_error("cap_op_embed: R = %d, D = %d, t = %d of %d columns", R, D, t, seq_ld); return -1; }
    RowMap map;
    map.live = live; map.n = n_live;
    return launch_embed(dt_of(dtype), seq, seq_ld, t, word, pos, gamma, beta, eps, out_t, out_f, R, D, (hipStream_t)stream, y_out, map);
}
int cap_op_embed_prompt(int dtype, const int32_t* seq, int seq_ld, int npos, int row0, const float* word, const float* pos,
                        const float* gamma, const float* beta, float eps, void* out_t, float* out_f, float* y_out, int n_caps, int D,
                        void* stream) {
    if (!seq || !word || !pos || !gamma || !beta) { cap_set_error("cap_op_embed_prompt: null pointer"); return -1; }
    if (D < 1) { cap_set_error("cap_op_embed_prompt: D = %d", D); return -1; }
    return launch_embed_prompt(dt_of(dtype), seq, seq_ld, npos, row0, word, pos, gamma, beta, eps, out_t, out_f, n_caps, D,
                               (hipStream_t)stream, y_out);
}
int cap_op_embed_tokens(int dtype, const int32_t* ids, int L, const float* word, const float* pos, const float* type0,
                        const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int R, int D, int V, void* stream) {
    // the kernel writes both outputs unconditionally
    if (!ids || !word || !pos || !type0 || !gamma || !beta || !out_t || !out_f) { cap_set_error("cap_op_embed_tokens: null pointer"); return -1; }
    if (R < 1 || L < 1 || D < 1) { cap_set_error("cap_op_embed_tokens: R = %d, L = %d, D = %d", R, L, D); return -1; }
    return launch_embed_tokens(dt_of(dtype), ids, L, word, pos, type0, gamma, beta, eps, out_t, out_f, R, D, (hipStream_t)stream, V);
}
int cap_op_init_prompt_seq(int32_t* seq, int32_t* finished, int32_t* lengths, int R, int L, const int32_t* prompt, int prompt_rows,
                           int P, int V, int pad, void* stream) {
    if (!seq || !finished || !lengths) { cap_set_error("cap_op_init_prompt_seq: null pointer"); return -1; }
    if (R < 1 || L < 1) { cap_set_error("cap_op_init_prompt_seq: R = %d, L = %d", R, L); return -1; }
    return launch_init_prompt_seq(seq, finished, lengths, R, L, prompt, prompt_rows, P, V, pad, (hipStream_t)stream);
}
int cap_op_compact_rows(const int32_t* finished, int R, int32_t* live, int32_t* n_live, void* stream) {
    if (!finished || !live || !n_live) { cap_set_error("cap_op_compact_rows: null pointer"); return -1; }
    if (R < 1) { cap_set_error("cap_op_compact_rows: R = %d", R); return -1; }
    return launch_compact_rows(finished, R, live, n_live, (hipStream_t)stream);
}
int cap_op_reduce_bias_act(int dtype, const float* part, int S, const float* bias, void* out, int M, int N, int act, void* stream) {
    if (!part || !out) { cap_set_error("cap_op_reduce_bias_act: null pointer"); return -1; }
    if (S < 1 || M < 1 || N < 1 || (act != 0 && act != 2)) { cap_set_error("cap_op_reduce_bias_act: S = %d, M = %d, N = %d, act = %d (0 or 2)", S, M, N, act); return -1; }
    return launch_reduce_bias_act(dt_of(dtype), part, S, bias, out, M, N, act, (hipStream_t)stream);
}
int cap_op_mean_pool_normalize(const float* x, const int32_t* lens, int B, int L, int D, float* out, void* stream) {
    if (!x || !lens || !out) { cap_set_error("cap_op_mean_pool_normalize: null pointer"); return -1; }
    if (B < 1 || L < 1 || D < 1) { cap_set_error("cap_op_mean_pool_normalize: B = %d, L = %d, D = %d", B, L, D); return -1; }
    return launch_mean_pool_normalize(x, lens, B, L, D, out, (hipStream_t)stream);
}
int cap_op_patchify(int dtype, const void* pixels, int fmt, int B, int img, int ps, int Kpad, void* out, const float* mean,
                    const float* stdv, void* stream) {
    if (!pixels || !out) { cap_set_error("cap_op_patchify: null pointer"); return -1; }
    if ((fmt != CAP_PIX_F32_NCHW && fmt != CAP_PIX_U8_NHWC) || B < 1 || img < 1 || ps < 1) {
        cap_set_error("cap_op_patchify: fmt = %d, B = %d, img = %d, ps = %d", fmt, B, img, ps);
        return -1;
    }
    return launch_patchify(dt_of(dtype), pixels, fmt, B, img, ps, Kpad, out, mean, stdv, (hipStream_t)stream);
}
int cap_op_cls_rows(const float* cls, const float* pos, float* X, int B, int tokens, int D, void* stream) {
    if (!cls || !pos || !X) { cap_set_error("cap_op_cls_rows: null pointer"); return -1; }
    if (B < 1 || tokens < 1 || D < 1) { cap_set_error("cap_op_cls_rows: B = %d, tokens = %d, D = %d", B, tokens, D); return -1; }
    return launch_cls_rows(cls, pos, X, B, tokens, D, (hipStream_t)stream);
}
int cap_op_convert2d(int dtype, const float* src, void* dst, int rows, int cols, int dst_ld, float scale, int transposed, void* stream) {
    if (!src || !dst) { cap_set_error("cap_op_convert2d: null pointer"); return -1; }
    if (rows < 1 || cols < 1 || dst_ld < (transposed ? rows : cols)) {
        cap_set_error("cap_op_convert2d: rows = %d, cols = %d, dst_ld = %d", rows, cols, dst_ld);
        return -1;
    }
    if (transposed) {
        if (dst_ld != rows) { cap_set_error("cap_op_convert2d: the transposed form writes dense rows (dst_ld = %d, rows = %d)", dst_ld, rows); return -1; }
        return launch_convert2d_t(dt_of(dtype), src, dst, rows, cols, (hipStream_t)stream, scale);
    }
    return launch_convert2d(dt_of(dtype), src, dst, rows, cols, dst_ld, (hipStream_t)stream, scale);
}
int cap_op_absmax(const float* src, size_t n, uint32_t* out_bits, void* stream) {
    if (!src || !out_bits) { cap_set_error("cap_op_absmax: null pointer"); return -1; }
    if (n < 1) { cap_set_error("cap_op_absmax: n = 0"); return -1; }
    return launch_absmax_f32(src, n, out_bits, (hipStream_t)stream);
}
int cap_op_convert(int dtype, const float* src, void* dst, size_t n, void* stream) {
    return launch_convert(dt_of(dtype), src, dst, n, (hipStream_t)stream);
}
int cap_op_convert_weight(int dtype, const float* src, void* dst, int rows, int cols, void* stream) {
    return launch_convert2d(dt_of(dtype), src, dst, rows, cols, cols, (hipStream_t)stream, dtype == CAP_F32_SPLIT ? G8_WSCALE : 1.0f);
}
/* the embedding and head kernels of the CLIP and BLIP-2 scorers alone (tests/test_scorer_kernels_gpu.py); the two score kernels are
 * cap_clip_logits and cap_blip2_itc_scores */
int cap_op_clip_embed_text(const int32_t* ids, int L, const float* tok, const float* pos, float* x, int M, int D, int V, void* stream) {
    if (!ids || !tok || !pos || !x) { cap_set_error("cap_op_clip_embed_text: null pointer"); return -1; }
    return launch_clip_embed_text(ids, L, tok, pos, x, M, D, V, (hipStream_t)stream);
}
int cap_op_clip_head(const float* x, int rows_per, const int32_t* lens, const float* gamma, const float* beta, float eps, const float* W,
                     float* out, int B, int D, int P, void* stream) {
    if (!x || !gamma || !beta || !W || !out) { cap_set_error("cap_op_clip_head: null pointer"); return -1; }
    return launch_clip_head(x, rows_per, lens, gamma, beta, eps, W, out, B, D, P, (hipStream_t)stream);
}
int cap_op_itm_embed_text(int dtype, const int32_t* ids, int L, const float* word, const float* pos, const float* gamma,
                          const float* beta, float eps, float* x_f, void* x_t, int M, int D, int V, void* stream) {
    // the kernel writes both outputs unconditionally
    if (!ids || !word || !pos || !gamma || !beta || !x_f || !x_t) { cap_set_error("cap_op_itm_embed_text: null pointer"); return -1; }
    return launch_itm_embed_text(dt_of(dtype), ids, L, word, pos, gamma, beta, eps, x_f, x_t, M, D, V, (hipStream_t)stream);
}
int cap_op_itc_head(const float* x, int rows_per, const float* W, const float* bias, float* out, int n, int D, int P, void* stream) {
    if (!x || !W || !bias || !out) { cap_set_error("cap_op_itc_head: null pointer"); return -1; }
    return launch_itc_head(x, rows_per, W, bias, out, n, D, P, (hipStream_t)stream);
}
int cap_op_itm_head(const float* x, const float* W, const float* bias, float* logits, float* prob, int B, int nq, int D, void* stream) {
    if (!x || !W || !bias || !logits) { cap_set_error("cap_op_itm_head: null pointer"); return -1; }
    return launch_itm_head(x, W, bias, logits, prob, B, nq, D, (hipStream_t)stream);
}

}  // extern "C"
