// Launchers of the non-GEMM kernels (elementwise.hip, attention.hip, beam.hip).  All launch on `stream`,
// never allocate or synchronise (graph-capturable), and return 0 / -1 (+ cap_set_error).
#pragma once
#include "common.h"

// Row compaction of the greedy decode loop (captioner.hip, run_step): the rows of captions that are still open, in
// row order, and their count - both on the device, rebuilt after every token selection.  A kernel given a RowMap works on
// COMPACT rows c < *n (activations, split-K slabs, logits) and reaches what a caption owns across steps - its tokens, its
// self-attention cache rows, its image's cross K/V - through live[c]; compact rows from *n on return at once.  Null pointers =
// no map (every row, c = row).  A caption's arithmetic does not depend on the row it sits in (batch invariance), so the
// compacted loop produces the bits of the uncompacted one.
struct RowMap {
    const int* live = nullptr;     // int32 [R]: live[c] = row of the batch
    const int* n = nullptr;        // int32: open rows
};

// ---- elementwise.hip -------------------------------------------------------------------------
// fp32 -> T copy (weight upload / activation cast); dst rows may be padded: dst[r*dst_ld + c] = src[r*cols + c]
int launch_convert(int dtype, const float* src, void* dst, size_t n, hipStream_t s);
int launch_convert2d(int dtype, const float* src, void* dst, int rows, int cols, int dst_ld, hipStream_t s, float scale = 1.0f);
// dst[cols][rows] = src[rows][cols]^T
int launch_convert2d_t(int dtype, const float* src, void* dst, int rows, int cols, hipStream_t s, float scale = 1.0f);
// im2col-free patch gather: pixels -> A[B*P, Kpad] (T).  fmt 0: fp32 NCHW normalised; fmt 1: u8 NHWC raw RGB,
// normalised on the fly with (x/255 - mean[c]) / std[c].
int launch_patchify(int dtype, const void* pixels, int fmt, int B, int img, int ps, int Kpad, void* out,
                    const float* mean, const float* stdv, hipStream_t s);
// X[b,0,:] = cls + pos[0]
int launch_cls_rows(const float* cls, const float* pos, float* X, int B, int tokens, int D, hipStream_t s);
// row LayerNorm: in fp32 [M,D]; writes out_t (T, optional) and out_f (fp32, optional; may alias in)
int launch_layernorm(int dtype, const float* in, int ld_in, const float* gamma, const float* beta, float eps,
                     void* out_t, float* out_f, int M, int D, hipStream_t s,
                     const int* n_rows = nullptr);   // device int32: rows from *n_rows on are left alone (RowMap::n)
// split-K / residual consumer: y = sum_z part[z][M][D] + bias + resid (fixed order); y_out (optional, may alias resid)
// receives y, then LayerNorm(y) goes to out_t / out_f as above (out_f may alias resid when y_out is null)
int launch_reduce_layernorm(int dtype, const float* part, int S, const float* bias, const float* resid,
                            const float* gamma, const float* beta, float eps, void* out_t, float* out_f, float* y_out,
                            int M, int D, hipStream_t s, bool per_row_block = false,
                            const int* n_rows = nullptr);   // device int32: rows from *n_rows on are left alone (RowMap::n)
// decoder embeddings: x = LN(word[tok] + pos[t]); tok = seq[row*seq_ld + t]
int launch_reduce_bias_act(int dtype, const float* part, int S, const float* bias, void* out, int M, int N, int act, hipStream_t s);
int launch_embed_tokens(int dtype, const int* ids, int L, const float* word, const float* pos, const float* type0,
                        const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int R, int D,
                        hipStream_t s, int V);   // ids outside [0, V) are clamped
int launch_mean_pool_normalize(const float* x, const int* lens, int B, int L, int D, float* out, hipStream_t s);
constexpr int TEXT_ATTENTION_MAX_LDS = 128 * 1024;      // bytes of LDS text_attention may ask for: 2 * L * head_dim * 4 <= this
int launch_text_attention(int dtype, const void* qkv, const int* lens, void* ctx, int B, int L, int H, int head_dim,
                          hipStream_t s);
int launch_embed(int dtype, const int* seq, int seq_ld, int t, const float* word, const float* pos,
                 const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int R, int D,
                 hipStream_t s, float* y_out = nullptr,    // y_out: the un-normalised sum (pre-LN residual stream)
                 RowMap map = RowMap());                    // compact output row c reads the token of row map.live[c]
// prompt prefill: launch_embed for n_caps * npos rows at once - row r = position r % npos of caption row0 + r / npos (token
// seq[caption * seq_ld + position], absolute position embedding pos[position]); the arithmetic of launch_embed, bit for bit
int launch_embed_prompt(int dtype, const int* seq, int seq_ld, int npos, int row0, const float* word, const float* pos,
                        const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int n_caps, int D,
                        hipStream_t s, float* y_out = nullptr);
// seq [R, L] = the prompt (prompt int32 [prompt_rows, P], prompt_rows 1 or R, ids clamped to [0, V)) then pad; finished = 0, len = L
int launch_init_prompt_seq(int* seq, int* finished, int* out_len, int R, int L, const int* prompt, int prompt_rows, int P, int V,
                           int pad, hipStream_t s);
// ---- token selection of the greedy loop: one step (SelectStep, launch_select_step) --------------------------------------------
// Banned tokens and sequences (HF NoBadWordsLogitsProcessor; captioner_hip.h, cap_set_bad_words), as the selection kernels read them:
//   bits   uint32 [ban_words(V)]: bit i set = token i is banned at every step (the length-1 sequences); bits from V on are 0
//   multi  int32 [n_multi][BAN_REC]: {n, tok[0 .. n - 1]}, 2 <= n <= BAN_MAX_LEN: tok[n - 1] is banned at a step exactly when the row's
//          last n - 1 context tokens equal tok[0 .. n - 2]; a sequence longer than the context (n > its length) never matches
// A block builds the row's bitmap in LDS from both (ban.h) and masks with it; banned = -inf.  bits may be null (no static bitmap;
// n_multi must then be 0).
constexpr int BAN_MAX_MULTI = 1024, BAN_MAX_LEN = 8, BAN_REC = BAN_MAX_LEN + 1;
struct BanSet {
    const unsigned* bits = nullptr;
    const int* multi = nullptr;
    int n_multi = 0;
};
__host__ __device__ inline int ban_words(int V) { return ((V + 31) / 32 + 3) / 4 * 4; }       // whole 16-byte pieces
// Repetition controls (HF RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor; captioner_hip.h, cap_set_repeat_controls), as
// the processed forms of the selection kernels read them.  The context of a row is what HF's processor sees: `vn` copies of `vtok`
// (BLIP-2's image placeholders; 0 = none), then the row's stored history, whose FIRST token reads as `vbos` when vbos >= 0 (BLIP-2
// keeps pad in the column that stands for BOS).
//   penalty  every distinct context token in [0, V): x < 0 ? x * penalty : x / penalty (fp32, a true division); 1 = off
//   ngram    n >= 1: a token that followed an earlier occurrence of the context's last n - 1 tokens is banned; 0 = off
// Order: penalty, n-grams, bad words (the last two are -inf).
struct RepeatCtl {
    float penalty = 1.f;
    int ngram = 0;
    int vn = 0, vtok = 0, vbos = -1;
    bool active() const { return penalty != 1.f || ngram > 0; }
};
// Sampling (HF `generate(do_sample=True, temperature=, top_k=, top_p=)`; captioner_hip.h, cap_set_sampling), as the sampled form of
// the greedy selection reads it: temperature (finite, > 0; 1 leaves the bits), top_k (0 or >= V: off), top_p in (0, 1] (1: off),
// seed = the Philox key.  The distribution is stated step by step at greedy_select_sampled_kernel (elementwise.hip).
struct SampleCtl {
    float temperature = 1.f;
    int top_k = 0;
    float top_p = 1.f;
    uint64_t seed = 0;
};
// The rows of a step, as every selection kernel takes them: logits row c (fp32 [., ld], V entries) belongs to caption row = map.live[c]
// (c without a map), whose token goes to seq[row][t + 1]; pad after EOS, finished / out_len kept per caption.  A row ends on EOS or at
// max_len tokens.  min_len > 0: EOS cannot win while the row has fewer than min_len tokens (HF MinLengthLogitsProcessor); force_eos
// (the reference's CoCa loop): the last position is EOS and a selected pad id ends the row.
struct SelectRows {
    const float* logits; int ld, V;
    int* seq; int seq_ld, t, max_len, eos, pad;
    int* finished; int* out_len;
    int min_len, force_eos;
    RowMap map;
};
// One step of token selection: `SelectStep st{};`, then fill.  The token is the arg-max (lowest index wins ties) of the row after its
// processors - penalty, n-grams, bad words, in HF's order, over the context seq[row][hist0 .. t] behind RepeatCtl's virtual prefix - or,
// with `sample` set, a draw from that row's distribution.  The token is always inside [0, V).  A NaN logit is never selected: no
// comparison with it is true, so it stands as -inf does; a row with nothing above -inf (all -inf, all NaN, everything banned, or finite
// only at an EOS that min_len still masks) selects index 0, which is what torch.argmax gives for an all -inf row.  (Only the token is
// defined for such a row or a row holding a NaN: the scoring forms' log-prob of it is NaN in general.)
// launch_select_step picks the kernel: sample -> the sampled form; else ctl.active() or ban.bits -> the processed form (a ban set alone:
// its instantiation without the controls); else the plain,
// log-prob (logprobs given) or vocabulary (vocab_acc given) form.  The scoring outputs go with the plain arg-max only and need
// ld % 4 == 0; the arg-max forms read a row with 16-byte loads when ld % 4 == 0 and logits is 16-byte aligned, element-wise otherwise.
struct SelectStep : SelectRows {
    int R;                             // logits rows (one block each)
    BanSet ban; int hist0;
    RepeatCtl ctl;
    int sample;                        // 1: draw with sc in place of the arg-max
    SampleCtl sc;
    const uint64_t* keys;              // uint64 [captions] (device), the per-CAPTION Philox counter words (null: the caption's row index)
    int draw;                          // the index of the generated token (the other counter word)
    int* out_kept;                     // null, or int32 [captions]: entries left with a weight above 0 after both cuts
    // log-prob form: logprobs[row * lp_ld + lp_col] = log max softmax of the row as selected from (EOS mask applied), scored[row] += 1,
    // for the rows open at this step
    float* logprobs; int lp_ld, lp_col; int* scored;
    // vocabulary form (needs the log-prob buffers): vocab_acc[row * acc_ld + i] = max(itself, softmax_i of the row as selected from),
    // i < V, for the rows open at this step; acc_ld >= V, acc_ld % 4 == 0, 16-byte aligned
    float* vocab_acc; int acc_ld;
};
int launch_select_step(const SelectStep& st, hipStream_t s);
// teacher-forced scoring: logits row b of `rows` (fp32 [rows, ld]) is pass row r = r0 + b = position r % npos of caption r / npos; for
// positions below n_live[caption] the log-softmax at targets[caption * tgt_ld + position] (clamped to [0, V)), log max softmax and the
// arg-max (launch_select_step's selection and tie rule, no EOS mask) go to out_*[caption * out_ld + position], zeros for the others
int launch_target_logprob(const float* logits, int ld, int V, int rows, int r0, int npos, const int* targets, int tgt_ld,
                          const int* n_live, float* out_tlp, float* out_top, int* out_top_id, int out_ld, hipStream_t s,
                          int j0 = 0,        // the pass starts at the caption's j0-th position: live = j0 + position < n_live[caption]
                          int share = 1);    // consecutive rows reading one logits row (row b reads logits row b / share)
// per group g of rows group_rows[group_off[g] .. group_off[g+1]) of acc [., acc_ld]: the tokens i < V whose fp32 mean over the
// members (summed in listed order) exceeds th, ascending: out_ids / out_prob [G, K] (at most K written), out_count [G] (all)
int launch_vocab_group_threshold(const float* acc, int acc_ld, int V, const int* group_rows, const int* group_off, int G, float th,
                                 int K, int* out_ids, float* out_prob, int* out_count, hipStream_t s);
// live[] = the rows with finished[r] == 0 in ascending order, *n_live = their count (one workgroup; stable)
int launch_compact_rows(const int* finished, int R, int* live, int* n_live, hipStream_t s);
int launch_fill_i32(int* p, int v, size_t n, hipStream_t s);
int launch_fill_f32(float* p, float v, size_t n, hipStream_t s);
int launch_copy_f32(const float* src, float* dst, size_t n, hipStream_t s);
// Image state (include/captioner_hip.h, "image state"): per-image records <-> the arena's buffer packed for a call's B images.
// The buffer is `sections` blocks, each holding the rows of the B images one after the other (row index = image * rows + row): the
// cross K/V cache ([slot][k|v] = 2 * slots sections of heads * kv_tokens head rows; KV16: blocks of kv16_block_bytes) or BLIP-2's
// language projection (one section of 16-byte rows).  A record is the image's sections one after the other, each its row
// payloads then (KV16) the rows' fp32 scales padded to 16 bytes, closed with zeros to a multiple of 256 bytes.
struct ImageStateLayout {
    int sections, rows, row_bytes, kv16;      // row_bytes: 256 / 128 (fp32 / bf16 and KV16 head rows), 16 (projection rows)
    size_t section_bytes() const { return (size_t)rows * row_bytes + (kv16 ? ((size_t)rows * 4 + 15) / 16 * 16 : 0); }
    size_t record_bytes() const { return ((size_t)sections * section_bytes() + 255) / 256 * 256; }
    size_t block_bytes(size_t B) const { return kv16 ? kv16_block_bytes(B * rows) : B * rows * (size_t)row_bytes; }
};
// pack: buffer -> B records at `state` (padding written as zeros); unpack: B records -> the rows of the B images in the buffer,
// nothing else of it.  Both pointers 16-byte aligned.
int launch_image_state_pack(const ImageStateLayout& L, int B, const void* buffer, void* state, hipStream_t s);
int launch_image_state_unpack(const ImageStateLayout& L, int B, void* buffer, const void* state, hipStream_t s);

// max |src[i]| as the bit pattern of a non-negative float, atomically max-ed into *out_bits (caller zeroes it)
int launch_absmax_f32(const float* src, size_t n, unsigned int* out_bits, hipStream_t s);
// per-file readers of the G8 clamp counter (common.h)
int cap_g8_clamped_gemm(unsigned long long* total, int reset);
int cap_g8_clamped_gemm_pp(unsigned long long* total, int reset);
int cap_g8_clamped_elementwise(unsigned long long* total, int reset);
int cap_g8_clamped_attention(unsigned long long* total, int reset);

// ---- attention.hip ---------------------------------------------------------------------------
// ViT self-attention over a fused qkv buffer [B*N, 3*H*64] (T) -> ctx [B*N, H*64] (T); scale = 1/8.
// impl 0 = auto (MFMA for bf16 when N <= 256, scalar otherwise), 1 = scalar, 2 = MFMA.
int launch_vit_attention(int dtype, const void* qkv, void* ctx, int B, int N, int H, int impl, hipStream_t s, int head_dim = 64,
                         int causal = 0,    // causal: query i sees keys 0..i (decoder prefill over fused q|k|v rows)
                         int out_dtype = -1);   // type of ctx when it differs from qkv's (split mode: fp32 in, G8 out)
// split mode: can the q|k|v buffer be G8 (launch_vit_attention(CAP_DT_G8, ...): the split-fp16 MFMA kernel) for N tokens?
// (Yes for every N since the kernel walks the keys in chunks; kept as the switch to the fp32 kernels: fp32 in, G8 out.)
bool vit_attention_takes_g8(int N);
int launch_generic_attention(int dtype, const void* q, long ldq, long qbs, const void* k, long ldk, long kbs, const void* v,
                             long ldv, long vbs, void* out, long ldo, long obs, int B, int Lq, int Lk, int H, int hd,
                             int causal_off, hipStream_t s, int out_dtype = -1);   // out_dtype: see launch_vit_attention
int launch_opt_prefill_inputs(const float* proj, const float* tok, const float* pos, float* x, int B, int nq, int T, int bos,
                              hipStream_t s);
int launch_opt_token_inputs(const int* seq, int seq_ld, int cur, const float* tok, const float* pos, float* x, int B, int T, int V,
                            hipStream_t s, int at = -1);     // ids outside [0, V) are clamped; at: the sequence position (default: cur)
// decode step of a pre-LN decoder: q|k|v row [B, 3T] -> appends k, v to caches [B][Lmax][T] at `past`, out [B, T]
constexpr int OPT_DECODE_MAX_KEYS = 1024;      // keys of a row (past + 1; scoring: P + n) the three launchers below take: the scores sit in LDS
int launch_opt_decode_attention(int dtype, const void* qkv, void* kc, void* vc, void* out, int B, int T, int H, int Lmax,
                                int past, hipStream_t s, int out_dtype = -1);
// the same for the rows r = image * K + beam of a beam search (beam.hip): keys below P from the cache of row image * K, key P + g
// from the cache of row anc[r * anc_ld + g], the new one appended to row r's own
int launch_opt_beam_decode_attention(int dtype, const void* qkv, void* kc, void* vc, void* out, int B, int K, int T, int H, int Lmax,
                                     int P, int past, const int* anc, int anc_ld, hipStream_t s, int out_dtype = -1);
// teacher-forced scoring behind a cached prompt (BLIP-2): n new positions of n_caps captions, caption-major fused q|k|v rows; caption
// cap0 + c belongs to image (cap0 + c) / C, whose P prompt keys are read from cache row `image` of kc / vc [.][Lmax][T], the caption's
// own keys from the rows themselves; n_pos (device, optional): rows with position >= n_pos[cap0 + c] are left untouched
int launch_opt_prefix_attention(int dtype, const void* qkv, const void* kc, const void* vc, void* out, int n_caps, int n, int cap0, int C,
                                const int* n_pos, int T, int H, int Lmax, int P, hipStream_t s, int out_dtype = -1);
// x [n_caps * n, T] = token table[ids[c * ids_ld + t]] + position table[P + t + 2] (ids clamped to [0, V))
int launch_opt_caption_inputs(const int* ids, int ids_ld, int n_caps, int n, int P, const float* tok, const float* pos, float* x, int T, int V,
                              hipStream_t s);
// row_stride: row b's positions go to cache row b * row_stride (a beam search's prompt: the first of each image's K rows)
int launch_kv_append(int dtype, const void* qkv, void* kc, void* vc, int B, int L, int T, int Lmax, int pos0, hipStream_t s,
                     int row_stride = 1);
int launch_rows_broadcast(int dtype, const float* src, float* dst_f, void* dst_t, int B, int n, int D, hipStream_t s);
// single-query decode attention. q [R, H*64] (T).  K/V of row r, head h, position j at
//   kbase + (((size_t)src(r,j) * H + h) * kv_ld + j) * 64   where src(r,j) = anc ? anc[r*anc_ld + j] : r / rows_per_kv
// n_keys positions; out [R, H*64] (T).  impl 0 = fast kernels (wave-per-head, chunked online softmax),
// impl 1 = simple two-pass block kernel (independent implementation kept for cross-checks).
// Fused producer (optional, impl 0 only): q_part != nullptr -> q = sum_z q_part[z][R][q_ld][q_col0 + ...] + q_bias;
// append_kv -> the new position's k/v are finished the same way (columns q_col0 + H*64, + 2*H*64), written to the
// cache of the row itself and attended (self-attention with n_keys <= 32).
struct DecodeAttn {                    // zero-initialise (memset), then fill
    const void* q;                     // [R, H*64] (T), or null with q_part
    const void* kbase; const void* vbase;
    const int* anc; int anc_ld;        // ancestry table (beams) or null
    int rows_per_kv, kv_ld, n_keys;
    void* out;                         // [R, H*64] (out_dtype)
    int R, H, impl;
    const float* q_part; int q_S; const float* q_bias; int q_ld, q_col0, append_kv;   // the fused producer
    int out_dtype;                     // type of out, always set (0 is fp32; < 0: dtype) - see launch_vit_attention: split mode is fp32 in, G8 out
    const int* skip_rows;              // int32 [R] or null: rows with a non-zero flag are left untouched
    int kv16;                          // 1: kbase / vbase are the bases of KV16 blocks (common.h; fp32 q, no
    size_t kv_row0;                    // ancestry, > 32 keys); kv_row0 = index of the launch's first row in them
    RowMap map;                        // q_part / out rows are compact, caches and ancestry belong to map.live[c]
                                       // (wave / online kernels, impl 0)
    int form;                          // the fused k/v-append step (q_part, append_kv): 0 = by row count, 1 = every key sub-lane finishes
                                       // its own partial sums, 2 = each column finished once per unit (the pass-size form); same bits
};
constexpr int DECODE_ATTN_SHARE_ROWS = 256;    // form 0 takes form 2 from this many rows on (attention.hip, launch_decode_attention)
int launch_decode_attention(int dtype, const DecodeAttn& a, hipStream_t s);
// Self-attention of a prompt prefill: n_caps * npos rows, row r = position r % npos of caption row0 + r / npos, its fused q|k|v
// projection as split-K partial sums part fp32 [S][n_caps * npos][part_ld] (+ bias [3 H 64]).  Two launches: every row's k / v are
// finished and written to positions 0 .. npos - 1 of the caption's own cache row (kbase / vbase [.][H][kv_ld][64], dtype), then row
// (c, p) attends keys 0 .. p through decode_attn.h's wave unit with the key count the single step at position p has - the context
// and the caches have the bits npos calls of launch_decode_attention (append_kv) would have left.  npos <= PREFILL_MAX_POS.
constexpr int PREFILL_MAX_POS = 31;
int launch_prefill_self_attention(int dtype, const float* part, int S, const float* bias, int part_ld, void* kbase, void* vbase,
                                  int kv_ld, void* out, int out_dtype, int n_caps, int npos, int row0, int H, hipStream_t s);
// fp32 rows [n_rows, 64] -> one KV16 block of kv16_block_bytes(n_rows) bytes: what the cross-K/V GEMM's epilogue writes, as a
// kernel of its own (tests)
int launch_pack_kv16(const float* src, void* dst, size_t n_rows, hipStream_t s);

// attentional pooler (CoCa): fixed projected queries qp fp32 [Q, E] shared by every image; kv (T) [B*N, 2E] with K in
// columns [0,E) and V in [E,2E); heads of E/heads dims (64 or 96); out (T) [B*Q, E].  scale = 1/sqrt(head_dim).
int launch_pool_attention(int dtype, const float* qp, const void* kv, void* out, int B, int N, int Q, int E, int heads,
                          hipStream_t s, int out_dtype = -1);

// ---- gemm_skinny.hip ---------------------------------------------------------------------------
// Weight-streaming bf16 GEMM for a handful of rows (decode step of a large LM).  skinny_plan: K slices for (N, K) in the
// finished (bias + act -> bf16, one slice) or partial form, 0 if the shape does not fit.  launch: part == nullptr ->
// out (bf16) = act(A W^T + bias), act 0 none / 1 GELU / 2 ReLU; part != nullptr -> part[z][M][N] fp32 slice sums for
// launch_reduce_layernorm / launch_reduce_bias_act.  Returns the slice count, or -1.
int skinny_plan(int N, int K, bool finished, int* nw_out = nullptr, int* tr_out = nullptr, int M = 32);
int launch_gemm_skinny(const void* A, int lda, const void* W, int ldw, const float* bias, int act, void* out, int ldc,
                       float* part, int M, int N, int K, hipStream_t s);

// int8 weights (BLIP-2 load_in_8bit): W as row-quantised signed bytes in MFMA fragment order + fp32 row scales (layout and
// arithmetic: gemm_skinny.hip).  launch_quant_i8_pack: fp32 [rows, cols] (rows % 16 == 0, cols % 64 == 0) -> dst (rows * cols
// bytes) and scale [rows].  skinny_i8_plan / launch_gemm_skinny_i8: as the bf16 pair, N % 32 == 0.
int skinny_i8_plan(int N, int K, bool finished, int* nw_out = nullptr);
int launch_quant_i8_pack(const float* src, void* dst, float* scale, int rows, int cols, hipStream_t s);
int launch_gemm_skinny_i8(const void* A, int lda, const void* Wp, const float* wscale, const float* bias, int act, void* out, int ldc,
                          float* part, int M, int N, int K, hipStream_t s);
// the bytes as a row-major bf16 matrix of the integers (for the tiled GEMM) and part[m][n] *= scale[n] on its fp32 output
int launch_dequant_i8_rowmajor(const void* packed, void* dst_bf16, int rows, int cols, hipStream_t s);
int launch_scale_cols(float* part, const float* scale, int M, int N, hipStream_t s);

// ---- preprocess.hip ----------------------------------------------------------------------------
// n boxes of one uint8 HWC frame -> out uint8 [n, S, S, 3] RGB, bit-exact with Pillow's crop + BICUBIC resize.
// rects int32 [n, 4] (x1, y1, x2, y2, inside the frame); hb/vb int32 [n, S, 2] (first tap, tap count) and hk/vk int32
// [n, S, KH|KV] integer coefficients built by the host (embodied_captioning_amd/preprocess.py).  All device pointers.
// the tables themselves, on the device (fp64, no contraction: equal to the host's bit for bit); geom int32 [n, 4] =
// (resized width, resized height, left, top) of the kept S x S window
int launch_crop_resize_tables(const int* rects, const int* geom, int n, int S, int KH, int KV, int* hb, int* hk, int* vb, int* vk,
                              hipStream_t s);
int launch_crop_resize_u8(const uint8_t* frame, int H, int W, int bgr, const int* rects, const int* hb, const int* hk, int KH,
                          const int* vb, const int* vk, int KV, int n, int S, uint8_t* out, hipStream_t s,
                          const long long* frames = nullptr);     // frames int64 [n, 3] = (byte offset in `frame`, H, W) of box b's own frame

// ---- clip.hip ----------------------------------------------------------------------------------
// CLIP text embeddings: x fp32 [M, D] = tok[ids[r]] + pos[r % L] (ids clamped to [0, V))
int launch_clip_embed_text(const int* ids, int L, const float* tok, const float* pos, float* x, int M, int D, int V, hipStream_t s);
// pooled head: row b * rows_per (+ lens[b] - 1 when lens is given) of x fp32 -> LayerNorm -> . W^T (fp32 [P, D]) -> L2 normalised
// out fp32 [B, P]; one workgroup per row, sums in an order that does not depend on B
int launch_clip_head(const float* x, int rows_per, const int* lens, const float* gamma, const float* beta, float eps, const float* W,
                     float* out, int B, int D, int P, hipStream_t s);
// exp(logit_scale) * img . txt^T: paired -> out [Ni] (row i against row i), else out [Ni, Nt]
int launch_clip_logits(const float* img, const float* txt, int Ni, int Nt, int P, int paired, float logit_scale, float* out, hipStream_t s);

// ---- similarity.hip ----------------------------------------------------------------------------
// cos(a_i, b_j) of fp32 rows [., D] (not assumed normalised; a zero row has cosine 0 with everything): out [Na, Nb], or with paired
// out [Na] = cos(a_i, b_i), bit for bit the matrix's diagonal.  ws: (Na + Nb) floats, caller-owned.
int launch_cosine_matrix(const float* a, const float* b, int Na, int Nb, int D, int paired, float* out, void* ws, size_t ws_bytes,
                         hipStream_t s);
// bytes of workspace launch_group_similarity needs for this grouping (0 + cap_set_error when the grouping is refused)
size_t sim_group_workspace(int N, int G, int D, const int* offsets);
// per-group caption disagreement / pair statistics / medoid and per-row mean similarity (include/captioner_hip.h,
// cap_group_similarity); offsets is a HOST array of G + 1 row bounds, everything else device memory
int launch_group_similarity(const float* e, const int* offsets, const float* weights, int N, int G, int D, float* disagreement,
                            float* pair_mean, float* pair_var, long long* pairs, int* medoid, float* row_mean, void* ws, size_t ws_bytes,
                            hipStream_t s);

// ---- blip2_itm.hip -----------------------------------------------------------------------------
// Q-Former text embeddings: x = qformer.layernorm(word[ids[r]] + pos[r % L]) -> x_f fp32 and x_t (dtype) [M, D] (ids clamped to [0, V))
int launch_itm_embed_text(int dtype, const int* ids, int L, const float* word, const float* pos, const float* gamma, const float* beta,
                          float eps, float* x_f, void* x_t, int M, int D, int V, hipStream_t s);
// Q-Former self-attention over [nq query rows | the first lens[b] of L text rows] per pair b, heads of 64: fused q|k|v rows
// qkv_q [B * nq, 3 H 64] / qkv_t [B * L, 3 H 64] (dtype) -> ctx_q [B * nq, H 64] / ctx_t [B * L, H 64].  nq = 0: text alone (the ITC
// text pass); L = 0: queries alone.  Sums ordered by nq and lens[b] only.
int launch_itm_self_attention(int dtype, const void* qkv_q, const void* qkv_t, const int* lens, void* ctx_q, void* ctx_t, int B, int nq,
                              int L, int H, int hd, hipStream_t s, int out_dtype = -1);   // out_dtype: see launch_vit_attention
// ITC head: rows r * rows_per of x fp32 [., D] -> . W^T + bias (fp32 [P, D], [P]) -> L2 normalised out fp32 [n, P]
int launch_itc_head(const float* x, int rows_per, const float* W, const float* bias, float* out, int n, int D, int P, hipStream_t s);
// ITC score: max over the nq query rows of img [Ni, nq, P] . txt [Nt, P]: paired -> out [Ni], else out [Ni, Nt]
int launch_itc_scores(const float* img, const float* txt, int Ni, int Nt, int nq, int P, int paired, float* out, hipStream_t s);
// ITM head: mean over the nq query rows of x [B * nq, D] . W^T + bias (fp32 [2, D], [2]) -> logits [B, 2], prob [B] = softmax[.., 1] (may be null)
int launch_itm_head(const float* x, const float* W, const float* bias, float* logits, float* prob, int B, int nq, int D, hipStream_t s);
int cap_g8_clamped_blip2_itm(unsigned long long* total, int reset);

// ---- beam.hip --------------------------------------------------------------------------------
size_t beam_state_bytes(int B, int K, int max_len);
int beam_candidates_only(void* state, const float* logits, int ld, int V, int B, int K, int mode, int eos_mask, float* out_val,
                         int* out_idx, hipStream_t s);     // test hook: candidate selection of the first step alone
// mode: BEAM_HF_V5 (log-softmax scores, HF 5.x `_beam_search`) or BEAM_LEGACY_RAW (the reference's CoCa loop: raw-logit
// scores, HF's pre-5.x BeamSearchScorer with one group, MinLength(min_len) on EOS) - see beam.hip
enum { BEAM_HF_V5 = 0, BEAM_LEGACY_RAW = 1 };
int launch_beam_init(void* state, int B, int K, int max_len, int bos, int pad, int eos, hipStream_t s, int mode = BEAM_HF_V5);
// One beam step: `BeamStep st{};`, then fill.  The log-softmax statistics see the raw row; with repetition controls (RepeatCtl above;
// HF v5 scores only) the penalty goes on the log-probs (all <= 0: lp * penalty), then the bans - a banned candidate's value is -inf -
// then the running score.  The history of a row is its LOGICAL one, run_seq[cur_len & 1][row][0 .. cur_len).  min_len masks EOS in
// BEAM_LEGACY_RAW mode alone.
struct BeamStep {
    void* state; const float* logits; int ld, V, B, K, max_len, cur_len, eos;
    float length_penalty;
    int* anc; int anc_ld;
    int mode, min_len;
    BanSet ban;
    RepeatCtl ctl;
};
int launch_beam_step(const BeamStep& st, hipStream_t s);
int launch_beam_finalize(void* state, int B, int K, int max_len, int* out_ids, int* out_len, float* out_scores,
                         hipStream_t s);
// device pointer: int32, 1 while the beam loop of this state is still running (HF `is_done.all()` not yet true)
const int* beam_active_flag_p(void* state, int B, int K, int max_len);
// device pointer: int32 [B*K, max_len] running sequences of the given parity (= cur_len & 1)
const int* beam_running_tokens_p(void* state, int B, int K, int max_len, int parity);
// device pointer: fp32 [B*K] running scores of the given parity
const float* beam_running_scores_p(void* state, int B, int K, int max_len, int parity);
