/* C ABI of the MI355X-native captioner forward path (libcaptioner_hip.so).
 *
 * Nothing like this exists in the reference (it is 100 % Python): every entry point below replaces a
 * piece of Python/torch that the reference's captioner wrappers run on CPU, and is what a binding for this path
 * (ctypes here; pybind11/cffi equally) has to call.  Plain pointers and sizes only - no torch types.
 *
 *   reference interface replaced                                              entry point
 *   -------------------------------------------------------------------------------------------------------------
 *   model construction  captioner/models/blip2/blip2.py:17-22 (from_pretrained),    cap_create, cap_load_weight,
 *                       captioner/models/coca/factory.py:183-338 (create_model),     cap_finalize_weights
 *                       utils/predictor_utils.py:182-185 (load_state_dict)
 *   image tower         coca_model.py:152-155 `_encode_image`;                       cap_encode
 *                       HF modeling_blip.py:901-906 `vision_model(pixel_values)`
 *   generate            blip2.py:26 `model.generate(..., output_logits=True)`;       cap_generate_request (CapGenerateArgs);
 *                       coca.py:29 `model.generate(x, generation_type=...)`;         cap_generate and its siblings fill one
 *                       coca_model.py:205-333 (greedy/top-k loop), :335-482 (beam);
 *                       blip2.py:26 BLIP-2 OPT (CAP_ARCH_BLIP2): out_ids = the max_len NEW tokens (HF's sequences
 *                       minus the 32 image placeholders and BOS), logits as HF's `output_logits`
 *   caption embedding   agents/goal_exploration/goal_exploration.py:57,102 and                cap_embed_text
 *                       detector/pseudolabeler.py:568,677 `SentenceTransformer("all-MiniLM-L6-v2").encode(caption)`  (CAP_ARCH_MINILM handle)
 *   text prompt         HF modeling_blip.py:858-932 `generate(pixel_values, input_ids=...)`    cap_generate_prompted (CAP_ARCH_BLIP, greedy:
 *                       ("a picture of ..."; the decoder gets input_ids[:, :-1], column 0 = BOS);   the prompt positions run as one prefill pass),
 *                       coca_model.py:207, 280-292 `generate(text=...)` is NOT built (refused)       CapConfig.max_prompt, cap_last_prefill_passes
 *   teacher forcing     HF modeling_blip.py / modeling_blip_2.py `forward(pixel_values, input_ids=...)`   cap_score_captions (BLIP, BLIP-2: log-prob of
 *                       (the reference scores only text it generated itself:                       a GIVEN caption's tokens, log max softmax and
 *                       captioning_predictor.py:34-47 `compute_perplexity`)                        arg-max per position), CapConfig.max_score_rows
 *   one crop per call   coca.py:27-33, blip2.py:24-29, goal_exploration.py:95-105,     cap_generate (rows <= 16: fused
 *                       pseudolabeler.py:673-676 (the callers hand over ONE image)      launches), cap_set_decode_path
 *   greedy stopping     HF generation/utils.py:2894-2937 (a finished row keeps its slot and   cap_set_row_compaction (the open
 *                       is fed pad tokens; `unfinished_sequences.max() == 0` ends the loop)  rows only), cap_set_early_exit
 *   banned words        HF `generate(bad_words_ids=...)` (NoBadWordsLogitsProcessor) - what would   cap_set_bad_words, cap_bad_words
 *                       keep the captions experimenting_env/captioner/pseudocaptioner.py:96-123    (BLIP, BLIP-2; inside the token
 *                       throws away for a banned word                                             selection kernels)
 *   repetition          HF `generate(repetition_penalty=, no_repeat_ngram_size=)`; coca_model.py:222,238       cap_set_repeat_controls (BLIP,
 *                       has the penalty in CoCa.generate's signature                                            BLIP-2; same kernels)
 *   batches of crops    detector/pseudolabeler.py:664-711, scripts/run_pseudolabeler.py:77-107  cap_create_shared (n engines on one
 *                       (one generate per crop; here: micro-batches merged into passes)          weight store: engine.EnginePool)
 *   load options        blip2.py:19-22 `load_in_8bit=True, torch_dtype=float16`;       CapConfig.weight_int8 (int8 Linear weights as
 *                       evaluate_finetuned_model.py:147-148 `PeftModel.from_pretrained`  bitsandbytes stores them, quantised by
 *                                                                                      cap_load_weight), CapConfig.compute_dtype,
 *                                                                                      CapConfig.cross_kv_fp32 (host side:
 *                                                                                      weights.merge_peft_lora)
 *   CLIP pseudo-caption experimenting_env/captioner/pseudocaptioner.py:39-46 (CLIPModel.from_pretrained),   cap_clip_embed_images,
 *   scores              :352-357 `model(**processor(text=[caption], images=crop)).logits_per_image`  cap_clip_embed_text,
 *                       (one HF call per (crop, caption) pair; here: batches of pairs, CAP_ARCH_CLIP)    cap_clip_logits
 *   BLIP-2 ITM / ITC    experimenting_env/captioner/pseudocaptioner.py:34-37 (LAVIS blip2_image_text_matching),  cap_blip2_itm_encode_images,
 *   pseudo-caption      :193-308 `model({"image", "text_input"}, match_head="itm" | "itc")` (one call and one    cap_blip2_itc_image_features,
 *   scores              ViT-g pass per (crop, caption) pair; here: batches of pairs, CAP_ARCH_BLIP2_ITM,        cap_blip2_itc_text_features,
 *                       arithmetic of HF `Blip2ForImageTextRetrieval.forward`)                                 cap_blip2_itc_scores, cap_blip2_itm_logits
 *   caption             experimenting_env/utils/projection_utils.py `_cosine_distance` (per object, every map update:   cap_group_similarity,
 *   disagreement,       mean of 1 - cos over the n x n matrix of its caption embeddings); scripts/compute_cosine_sim.py  cap_group_similarity_workspace,
 *   cosine statistics   (mean pairwise cosine over i < j per (episode, object)); captioner/test_cosine_similarity.py     cap_cosine_matrix
 *                       (its mean and std); scripts/compute_performance_measures.py `diag(cos_sim(proposed, reference))`
 *   device move/free    predictor_utils.py:187 `.to(...)`; object lifetime            cap_destroy
 *   errors              Python exceptions (utils_captioner.py:6, factory.py:231,309)  int return codes + cap_last_error
 *
 * Conventions: every function returns 0 on success, non-zero on failure (message via cap_last_error(), thread-local).
 * All device buffers are caller-owned; the library owns weights, KV caches and workspace, sized at cap_create from
 * max_batch / max_beams / max_len.  One handle per stream; a handle is not thread-safe.  Calls enqueue work on the
 * given hipStream_t (passed as void*) and return without synchronising, except where noted.
 */
#ifndef CAPTIONER_HIP_H
#define CAPTIONER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct CapHandle_s* CapHandle;

enum { CAP_ARCH_BLIP = 0, CAP_ARCH_COCA = 1, CAP_ARCH_MINILM = 2, CAP_ARCH_BLIP2 = 3, CAP_ARCH_CLIP = 4, CAP_ARCH_BLIP2_ITM = 5 };
/* activation of the MLPs (CapConfig.hidden_act, CAP_ARCH_CLIP): HF ACT2FN["quick_gelu"] x * sigmoid(1.702 x) (OpenAI CLIP) or exact GELU */
enum { CAP_ACT_QUICK_GELU = 0, CAP_ACT_GELU = 1 };
/* Arithmetic of the GEMM / attention operands (accumulation is fp32 in every mode):
 *   CAP_F32        fp32 operands, exact fp32 products on the fp32 MFMA pipe (v_mfma_f32_32x32x2_f32)
 *   CAP_BF16       bf16 operands on the bf16 MFMA pipe - fastest, but not token-identical to an fp32 reference
 *   CAP_F32_SPLIT  fp32 values carried into every GEMM as two fp16 halves (hi + lo = x to 2^-23), each product formed as
 *                  hi.hi + hi.lo + lo.hi on the fp16 MFMA pipe: products good to ~2^-21 (fp32: 2^-24, bf16: 2^-9) at 3/16
 *                  of the fp32 pipe's cost; LayerNorm, softmax, attention, residual stream and the self-attention K/V cache are
 *                  fp32 as in CAP_F32.  The CROSS-attention K/V cache (the decode side's HBM stream) is KV16 - per token and
 *                  head 64 int16 and one fp32 scale, 15 value bits relative to the row's largest element - whenever an image has
 *                  more than 32 tokens (every real BLIP / CoCa geometry); CapConfig.cross_kv_fp32 = 1 keeps fp32 rows instead
 *                  (1.9x the bytes), cap_cross_cache_kind() reports what a handle uses.  Token-identical to the fp32 reference
 *                  on every golden fixture; the default of the plugin and of bench.py.  Every captioner architecture (BLIP, BLIP-2, CoCa); not the sentence encoder.  The mode has a
 *                  finite range - see cap_g8_saturations. */
enum { CAP_F32 = 0, CAP_BF16 = 1, CAP_F32_SPLIT = 2 };
/* normalised fp32 [B,3,H,W] | raw RGB uint8 [B,H,W,3] | B image-state records (cap_encode_image_state; the decoding calls only) */
enum { CAP_PIX_F32_NCHW = 0, CAP_PIX_U8_NHWC = 1, CAP_PIX_IMAGE_STATE = 2 };

typedef struct CapConfig {
    int32_t struct_size;          /* sizeof(CapConfig), for ABI checking */
    int32_t arch;                 /* CAP_ARCH_BLIP | CAP_ARCH_COCA | CAP_ARCH_MINILM (sentence encoder: only the t_* / vocab /
                                     max_pos / max_batch / max_len fields are read; max_len = tokens per sentence) */
    int32_t compute_dtype;        /* CAP_F32 | CAP_BF16 | CAP_F32_SPLIT (see the enum) */
    /* vision tower */
    int32_t image_size, patch_size, v_hidden, v_layers, v_heads, v_mlp;
    float v_eps;
    /* text decoder */
    int32_t t_hidden, t_layers, t_heads, t_ffn, vocab, max_pos;
    float t_eps;
    int32_t bos, eos, pad;
    /* capacity of the library-owned arena */
    int32_t max_batch, max_beams, max_len;
    /* raw-pixel normalisation for CAP_PIX_U8_NHWC: (x/255 - mean[c]) / std[c] */
    float pix_mean[3], pix_std[3];
    /* CAP_ARCH_COCA only (open_clip coca_ViT-L-14.json): attentional pooler output width / queries / heads, number of
     * multimodal decoder layers (t_layers = unimodal text layers), MinLength of the decode loop.  For CoCa
     * bos = start-of-text id, max_pos = context_length + 1, max_len = generate()'s seq_len. */
    int32_t embed_dim, pool_queries, pool_heads, mm_layers, min_len;
    /* CAP_ARCH_BLIP2 only (HF Blip2Config): Q-Former geometry, cross-attention on layers i % q_cross_freq == 0, number of
     * query tokens.  v_* = ViT-g (head_dim = v_hidden / v_heads, any multiple of 8 up to 128), t_* = OPT decoder (pre-LN,
     * ReLU, learned positions with offset 2; max_pos = rows of embed_positions - 2), max_len = new tokens per caption,
     * bos/eos/pad = OPT ids as generate() uses them. */
    int32_t q_hidden, q_layers, q_heads, q_ffn, q_cross_freq, num_query_tokens;
    float q_eps;
    /* CAP_F32_SPLIT only: 1 = the cross-attention K/V cache keeps fp32 rows (as CAP_F32 does) instead of KV16.  0 (default): KV16
     * for images of more than 32 tokens.  Ignored by the other modes (bf16 rows / fp32 rows). */
    int32_t cross_kv_fp32;
    /* CAP_ARCH_BLIP2 + CAP_BF16 only: 1 = the reference's own load mode for BLIP-2 (captioner/models/blip2/blip2.py:19-22,
     * `load_in_8bit=True`): the OPT decoder layers' Linear weights (q / k / v / out_proj / fc1 / fc2 - where the bytes of a decode
     * step are) are kept as bitsandbytes keeps a Linear8bitLt weight - one signed byte per element, q = rint(w * 127 /
     * absmax(row)), and the row's absmax / 127 in fp32 - quantised on the device by cap_load_weight from the fp32 tensor it is
     * given; the GEMMs stream the bytes and multiply the row sums by the scales.  Activations stay bf16 (bitsandbytes' int8
     * activation path with fp16 outlier columns is not restated: weights-only, "W8A16").  lm_head stays bf16 (HF does not
     * convert it either).  Needs OPT widths the int8 weight stream takes (opt-2.7b's 2560 / 10240 are). */
    int32_t weight_int8;
    /* CAP_ARCH_CLIP only: CAP_ACT_QUICK_GELU (0, the OpenAI checkpoints) or CAP_ACT_GELU (1) in both towers' MLPs. */
    int32_t hidden_act;
    /* CAP_ARCH_BLIP only: prompt capacity of the arena.  0 (default): none reserved - the handle allocates exactly what it did before
     * the field existed; cap_generate_prompted then runs the prefill over as many captions at a time as the decode workspace
     * (max_batch x max_beams rows) holds.  2 .. CAP_MAX_PROMPT: the buffers a decoder pass works in hold max_batch x (max_prompt - 1)
     * rows, so the prompt positions of a full batch are ONE pass (every decoder weight read once per prefill). */
    int32_t max_prompt;
    /* CAP_ARCH_BLIP only: scoring capacity of the arena, in decoder rows (one row per caption position).  0 (default): none reserved -
     * the handle allocates exactly what it did before the field existed; cap_score_captions then works in passes of as many captions
     * as the decode workspace holds (max(max_batch x max_beams, max_batch x (max_prompt - 1)) rows) and runs the head over max_batch x
     * max_beams rows at a time.  > 0: the pass buffers AND the head's (one fp32 logits row of `vocab` columns each) hold this many
     * rows, so N captions of L tokens are one pass with one vocabulary GEMM when N x (L - 1) <= max_score_rows (and N <= max_batch x
     * max_beams: the self-attention caches).  The chunking changes no bits. */
    int32_t max_score_rows;
} CapConfig;
enum { CAP_MAX_PROMPT = 32 };   /* prompt tokens per caption, BOS included, cap_generate_prompted takes */

const char* cap_last_error(void);
int cap_version(void);

int cap_create(const CapConfig* cfg, CapHandle* out);
/* A further handle on the SAME weights (read-only once loaded): own arena / KV caches / workspace, sized by cfg's max_batch,
 * max_beams, max_len; everything else in cfg must equal the configuration of `weights_of` (same model, compute dtype, GPU).
 * What a pool of engines on several streams uses: n handles cost one copy of the weights + n arenas.  Tensors loaded through
 * any of the handles are seen by all.  The weights are freed when the last handle referencing them is destroyed (any order).
 * Replaces: one `model.to(device)` copy per worker (reference utils/predictor_utils.py:187). */
int cap_create_shared(const CapConfig* cfg, CapHandle weights_of, CapHandle* out);
int cap_destroy(CapHandle h);

/* Stream one fp32 tensor of the checkpoint into the library.  Names: HuggingFace BLIP state-dict keys for CAP_ARCH_BLIP;
 * open_clip CoCa keys (`visual.*`, `text.*`, `text_decoder.*`) for CAP_ARCH_COCA plus a few tensors the host derives
 * once at load (embodied_captioning_amd/coca_weights.py): `derived.pool_q` (ln_q(query) projected), `derived.pool_kv.*`
 * (k|v projection of the pooler fused), `derived.cross_q.{i}.*`, `derived.cross_kv.*` (all layers' cross k|v projections
 * with ln_1_kv folded in), `derived.vocab.weight` (text_projection transposed).  `data` is a
 * host pointer (on_device = 0) or a device pointer (on_device = 1); the library converts to its compute layout
 * (bf16 cast, q/k/v and cross-K/V concatenation) on `stream` and synchronises before returning.
 * Unknown names return 1 (not an error for tied/duplicate heads, see cap_finalize_weights). */
int cap_load_weight(CapHandle h, const char* name, const float* data, int on_device, int ndim, const int64_t* shape,
                    void* stream);
/* Returns 0 when every tensor the architecture needs has been loaded; otherwise the count of missing tensors
 * (names in cap_last_error()). */
int cap_finalize_weights(CapHandle h);

/* Early exit of cap_generate's decode loop, as HF generate stops once every caption is finished (the remaining steps
 * would only write pad, so the outputs are the same either way).  poll_steps > 0: after every poll_steps-th step one
 * tiny kernel reports the number of open captions through a host-mapped word and the stream is synchronised.
 * 0 (default): never look - no host synchronisation inside cap_generate, which can then be captured in a graph.  With early
 * exit, rows of out_step_logits beyond the last executed step are left untouched.  Reference: HF
 * GenerationMixin._sample / _beam_search stopping criteria behind captioner/models/blip/blip.py:30 `model.generate`. */
int cap_set_early_exit(CapHandle h, int poll_steps);
/* Decode steps the last cap_generate on this handle ran (max_len - 1 without early exit; diagnostics and tests). */
int cap_last_decode_steps(CapHandle h);

/* Banned tokens and token sequences of the decode loops: HF `generate(bad_words_ids=...)` (NoBadWordsLogitsProcessor), applied
 * on the device inside the token selection.  Handle state, like cap_set_early_exit: it holds for every generating call that follows
 * until it is replaced or cleared.  ids / offsets are HOST arrays in CSR form (sequence q = ids[offsets[q] .. offsets[q + 1]),
 * offsets[0] = 0); n_sequences = 0 clears the set.
 *   a sequence of one token      banned at every step ([eos] alone is dropped silently, as HF drops it); any number of them
 *   a sequence of n > 1 tokens   its last token is banned at a step exactly when the caption's last n - 1 context tokens are its first
 *                                n - 1; a sequence longer than the context (n > its length) never matches.  At most 1024 of them, at most 8 tokens each.
 * Banned = -inf.  Greedy: the arg-max is taken over the banned row (first maximal index; a row with nothing left selects 0).  Beam
 * search: log-softmax of the RAW row, then the ban, then the running score (HF `_beam_search`).  The context is what HF's processor
 * sees: BLIP's BOS, prompt tokens and generated tokens (a sequence may match across the prompt boundary); BLIP-2's BOS and
 * generated tokens.  out_step_logits stays the raw logits.
 * Honoured by cap_generate_request and its siblings on CAP_ARCH_BLIP and CAP_ARCH_BLIP2 handles, num_beams 1 .. 8, on every path
 * (batch, small-batch, compacted, prompted, from an image state).  With a non-empty set they refuse, by name: a CAP_ARCH_COCA handle,
 * beam groups, out_logprobs / out_vocab.  cap_score_captions ignores the set by definition (teacher forcing reads plain logits).
 * Refused by name: an empty sequence, an id outside [0, vocab), the BOS or pad id (context only, never generated), the limits above.
 * The set's storage is allocated at the first non-empty set and freed by cap_destroy; it is not part of the arena.  The upload is
 * in stream order; replacing a set synchronises the GIVEN stream first.  The caller's obligation: no generating call of this handle
 * may be in flight on ANOTHER stream while the set is replaced or cleared (it reads the set's device arrays), and a call on another
 * stream must be ordered behind the upload (CaptionerEngine.set_bad_words synchronises after it).  With nothing set every launch is
 * the unbanned one. */
int cap_set_bad_words(CapHandle h, const int32_t* ids, const int32_t* offsets, int n_sequences, void* stream);
/* The set in force: distinct single tokens and multi-token sequences (either pointer may be NULL). */
int cap_bad_words(CapHandle h, int* n_single, int* n_multi);

/* Repetition controls of the decode loops: HF `generate(repetition_penalty=p, no_repeat_ngram_size=n)` (RepetitionPenaltyLogitsProcessor,
 * NoRepeatNGramLogitsProcessor), applied on the device inside the token selection.  Handle state, like cap_set_bad_words: two numbers
 * that hold for every generating call that follows; (1, 0) switches both off, and every launch is then what it was without them.
 *   penalty p (finite, > 0)   every distinct token id of the caption's context that lies in [0, vocab) has its score x replaced by x * p
 *                             if x < 0, else x / p - once, however often it occurs; fp32, a true division
 *   n-gram size n (>= 1)      every token that followed an earlier occurrence of the context's last n - 1 tokens is banned (-inf); n = 1
 *                             bans every context token; nothing is banned while the context is shorter than n - 1
 * Order: penalty, n-grams, bad words.  Greedy: on the raw fp32 row, then the arg-max (first maximal index; a row with nothing left
 * selects 0).  Beam search: log-softmax of the RAW row, the penalty on the log-probs (lp * p), the bans, then the running score.
 * The context is what HF's processors see: BLIP's BOS, prompt and generated tokens; BLIP-2's num_query_tokens image placeholders
 * (cap_set_image_token gives their id; required before a control is switched on), BOS and generated tokens - so BLIP-2's BOS and
 * placeholder scores are penalised from the first step on, and where BOS and EOS are one id (OPT's 2) so is EOS.  The ban set's own
 * context is unchanged.  out_step_logits stays the raw logits; cap_score_captions ignores the controls.
 * Refused by name here: a non-finite or non-positive penalty, a negative size, a size above max_len plus the prefix (BLIP-2:
 * num_query_tokens + 1).  With a control on, the generating calls refuse by name: a CAP_ARCH_COCA handle (its loop does not apply
 * them), beam groups, out_logprobs / out_vocab. */
int cap_set_repeat_controls(CapHandle h, float repetition_penalty, int no_repeat_ngram_size);
int cap_repeat_controls(CapHandle h, float* repetition_penalty, int* no_repeat_ngram_size);   /* either pointer may be NULL */
/* CAP_ARCH_BLIP2: the id HF puts num_query_tokens times in front of BOS (Blip2Config.image_token_index); context for the repetition
 * controls only.  An id at or beyond the vocabulary is legal (no processor acts on it). */
int cap_set_image_token(CapHandle h, int image_token);

/* Sampling in the greedy loop: HF `generate(do_sample=True, temperature=T, top_k=k, top_p=p)` (the reference's CoCa has a loop of its
 * own, coca_model.py:266-275, 304-320; HF's sits behind its BLIP / BLIP-2 wrappers), on the device inside the token selection.  Handle
 * state, like cap_set_repeat_controls: it holds for every generating call that follows; on = 0 switches it off (the numbers are kept
 * and read back, nothing else), and every launch is then what it was without it.
 * For an open caption at the step that produces its j-th generated token (j = HF's index into its `logits` tuple; prompt positions
 * are not counted), on the raw fp32 logits row x:
 *   1. s = processors(x): repetition penalty, n-gram bans, bad words as in force, HF's order; banned = -inf, a NaN stands as -inf
 *   2. z_i = s_i / T, fp32, a true division (T = 1 leaves the bits)
 *   3. top-k (0 or >= vocab: off): i stays iff z_i >= the k-th largest value - every entry tied with it stays
 *   4. m = max z; w_i = (uint64)(expf(z_i - m) * 2^40) for what stays, 0 otherwise (accurate expf); integer arithmetic from here on
 *   5. top-p (1: off), after top-k as HF orders its warpers: W = sum w, R = (uint64)floor((1.0 - (double)top_p) * (double)W); a value v
 *      stays iff sum_{kept j, z_j <= v} w_j > R; the maximal value always stays (HF min_tokens_to_keep = 1).  On a tie-free row this
 *      is HF TopPLogitsWarper's set; tied values stay or go together
 *   6. W' = the remaining sum; U = a 64-bit uniform; r = the high 64 bits of U * W'; the token is the smallest id i with
 *      sum_{j <= i} w_j > r (an inverse CDF in ascending id order).  A row with nothing left selects 0, as the arg-max forms do
 * A token whose weight relative to the row's maximum is below 2^-40 has w = 0 and is never drawn.
 * RNG: Philox4x32-10, counter (j, 0, key_lo, key_hi), key (seed_lo, seed_hi), U = (out0 << 32) | out1.  `key` is a per-CAPTION 64-bit
 * value (cap_generate_sampled's sample_keys; NULL = the row index), never a row position: a caption's tokens depend on its logits, the
 * parameters, seed, key and j alone - not on the batch, the grid, the row it sits in, the compacted loop or a pool's merged passes.
 * Finished rows, pad after EOS, lengths, early exit: the greedy loop's, unchanged.  out_step_logits stays the raw logits;
 * cap_score_captions ignores the state.
 * Refused by name here: a non-finite or non-positive temperature, top_k < 0, top_p outside (0, 1].  With sampling on the generating
 * calls refuse by name: num_beams > 1 or beam groups (beam sampling is not built), a CAP_ARCH_COCA handle, out_logprobs / out_vocab. */
int cap_set_sampling(CapHandle h, int on, float temperature, int top_k, float top_p, uint64_t seed);
int cap_sampling(CapHandle h, int* on, float* temperature, int* top_k, float* top_p, uint64_t* seed);   /* any pointer may be NULL */

/* Which kernels the decode steps of cap_generate run on (CAP_ARCH_BLIP, split and bf16 modes).  The reference calls its captioner
 * with ONE crop per call (captioner/models/coca/coca.py:27-33, blip2/blip2.py:24-29, agents/goal_exploration/goal_exploration.py:
 * 95-105; BASELINE config 1: 8 crops): for images x beams <= 16 rows a decoder layer-step runs as 6 fused launches
 * (csrc/decode_small.hip) instead of the batch path's 11.  Both paths form the same sums in the same order: tokens, logits and
 * scores have the same bits (tests/test_small_decode_gpu.py).
 *   path 0 (default): by row count;  1: always the batch kernels;  2: always the small-batch kernels - cap_generate then fails for
 *   calls they do not take (more than 16 rows, more than 32 positions, CAP_F32, other architectures), before anything is launched. */
int cap_set_decode_path(CapHandle h, int path);
/* 1 = batch kernels, 2 = small-batch kernels: what the last decode step of the last cap_generate ran on (0 before any). */
int cap_last_decode_path(CapHandle h);
/* Row compaction of the greedy decode loop (CAP_ARCH_BLIP, batch kernels, more than 16 rows, max_len <= 33, no per-step logits):
 * after every token selection the rows of the captions still open are packed to the front and every kernel of the next step
 * works on those rows only (HF's greedy loop, generation/utils.py:2894-2937, keeps feeding pad tokens to a finished row; its
 * outputs are never read).  A caption's arithmetic does not depend on the row it sits in, so tokens and lengths are the bits of the
 * uncompacted loop (tests/test_merged_passes_gpu.py).  on = 1 (default) / 0. */
int cap_set_row_compaction(CapHandle h, int on);
/* 1 if the decode loop of the last cap_generate ran compacted, 0 if not (-1: null handle). */
int cap_last_row_compaction(CapHandle h);
/* Layout of the handle's cross-attention K/V cache: 0 = fp32 rows, 1 = bf16 rows, 2 = KV16 (int16 + one fp32 scale per 64-wide
 * head row; CAP_F32_SPLIT unless CapConfig.cross_kv_fp32).  -1 for a null handle. */
int cap_cross_cache_kind(CapHandle h);

/* Object crops of one frame, resized for the captioner ON THE DEVICE, bit-exact with Pillow's
 * `Image.crop(box).resize((S, S), Image.BICUBIC)` - what the reference does to every detected box on the host before the
 * captioner sees it (detector/pseudolabeler.py:670-675 expand + crop, BGR->RGB at :670; HF BlipImageProcessor.resize).
 *   frame  uint8 [H, W, 3] (device), bgr != 0: channels are swapped to RGB on the way
 *   rects  int32 [n, 4] = x1, y1, x2, y2 of each (already expanded) box; parts outside the frame read as zeros, as
 *          Image.crop pads them
 *   hb, vb int32 [n, S, 2] = first input index (relative to the crop) and tap count of every output column / row
 *   hk, vk int32 [n, S, KH] / [n, S, KV] = Pillow's 22-bit integer coefficients (normalize_coeffs_8bpc), zero padded
 *   out    uint8 [n, S, S, 3] RGB -> feed to cap_generate / cap_encode as CAP_PIX_U8_NHWC
 * The tables are O(S) doubles per box: cap_crop_resize_tables fills them on the device (fp64 without contraction - equal
 * to Pillow's bit for bit), or the host builds them (embodied_captioning_amd/preprocess.py::pil_bicubic_coeffs).  All
 * pointers are device pointers. */
/* geom int32 [n, 4] = (resized width, resized height, left, top): out = the window [left, left+S) x [top, top+S) of the crop
 * resized to (width, height); (S, S, 0, 0) for the plain square resize.  KH / KV >= 2 ceil(2 max(scale, 1)) + 1 of the
 * widest / tallest box (scale = crop size / resized size). */
int cap_crop_resize_tables(const int32_t* rects, const int32_t* geom, int n, int S, int KH, int KV, int32_t* hb, int32_t* hk,
                           int32_t* vb, int32_t* vk, void* stream);
int cap_crop_resize_u8(const uint8_t* frame, int H, int W, int bgr, const int32_t* rects, const int32_t* hb,
                       const int32_t* hk, int KH, const int32_t* vb, const int32_t* vk, int KV, int n, int S, uint8_t* out,
                       void* stream);
/* The same for a LIST of images (what generate_batch / caption_batch receive: PIL crops of different sizes): `packed` holds the n
 * images' bytes back to back, frames int64 [n, 3] = (byte offset, height, width) of image b, rects[b] its rectangle inside it
 * ((0, 0, W, H) for the whole image) - one upload and one launch for the whole list. */
int cap_crop_resize_u8_frames(const uint8_t* packed, const int64_t* frames, int bgr, const int32_t* rects, const int32_t* hb,
                              const int32_t* hk, int KH, const int32_t* vb, const int32_t* vk, int KV, int n, int S, uint8_t* out,
                              void* stream);

/* Image tower.  pixels: B frames in `pixel_fmt`; out_embeds: fp32 [B, tokens, v_hidden] (device). */
int cap_encode(CapHandle h, const void* pixels, int pixel_fmt, int B, float* out_embeds, void* stream);

/* ---- image state: encode once, then generate, prompt and score from it ----
 * Everything the decode side of a handle reads from the image side, as one opaque record per image in CALLER-owned device memory:
 * nothing stays resident in the handle, and no result depends on what the arena held before a call.  cap_encode_image_state runs
 * the image side and packs the records; cap_generate_request, every cap_generate* convenience and cap_score_captions take them as
 * pixel_fmt = CAP_PIX_IMAGE_STATE (`pixels` = B contiguous records) and unpack them into the arena for the call's B INSTEAD of
 * running the image side.  Both are re-layouts of bytes the decoder reads anyway: a call from a state gives the bits of the call
 * from the pixels (tests/test_image_state_gpu.py), whatever the batch, order or repetition the records are given in.
 * A record belongs to handles of the same architecture and geometry, compute type and cross-cache kind (cap_image_state_bytes
 * differs for most other pairs, and the decoding calls cannot tell more than the caller's pointer); a record made with other
 * weights decodes to that other model's image.
 *
 * Record layout.  CAP_ARCH_BLIP / CAP_ARCH_COCA: the image's rows of the cross-attention K/V cache [slot][k|v][image][head][kv_tokens]
 * [64] (slots = t_layers, CoCa: mm_layers; kv_tokens = image tokens, CoCa: pool_queries - the pooled-token row travels with the rest
 * and is not attended, as ever), in the handle's cache kind (cap_cross_cache_kind):
 *     for slot in 0 .. slots - 1:  for part in (k, v):                                        -- one SECTION each
 *         rows = t_heads * kv_tokens row payloads in [head][token] order, row_bytes each:
 *             kind 0: 64 fp32 = 256 bytes,  kind 1: 64 bf16 = 128 bytes,  kind 2 (KV16): 64 int16 = 128 bytes
 *         kind 2 only: the same rows' fp32 scales, rows * 4 bytes, zero-padded to a multiple of 16 bytes
 *     zero padding to a multiple of 256 bytes
 *   section_bytes = rows * row_bytes + (kind 2 ? round_up(rows * 4, 16) : 0);  record_bytes = round_up(2 * slots * section_bytes, 256).
 *   (A KV16 block of the cache groups 32 head rows ACROSS images and the cache is packed for the call's B, so the same record lands
 *   in different places for different B: that is the unpacking's work.)
 * CAP_ARCH_BLIP2: the image's num_query_tokens rows of the language projection's output, fp32 [num_query_tokens][t_hidden], zero-padded
 * to a multiple of 256 bytes.  The prompt pass stays on the decoding side (it depends on the beam count).
 *
 * cap_image_state_bytes: bytes of one record on this handle; 0 (and an error) for a null handle or one that is not BLIP, CoCa or BLIP-2.
 * cap_encode_image_state: pixels = B frames in pixel_fmt (CAP_PIX_F32_NCHW | CAP_PIX_U8_NHWC), B <= max_batch; out_state = B records
 * ([B, cap_image_state_bytes] bytes, device, 16-byte aligned), padding included in what is written.  Refused before anything is
 * launched: another kind of handle, B beyond max_batch, a null or misaligned out_state, CAP_PIX_IMAGE_STATE as the input.  The decoding
 * calls refuse a null or misaligned state the same way; cap_encode and the scorer handles' image calls refuse CAP_PIX_IMAGE_STATE by name. */
size_t cap_image_state_bytes(CapHandle h);
int cap_encode_image_state(CapHandle h, const void* pixels, int pixel_fmt, int B, void* out_state, void* stream);

/* Encoder + autoregressive decode: ONE request, everything a generate call can ask for.  Zero / NULL = absent.  Every rule below is
 * checked by cap_generate_request before anything is launched, in this order: handle and capacity (B <= max_batch, num_beams <=
 * max_beams, max_len <= cfg.max_len), buffers, what the handle's architecture takes, shapes.  A refused request leaves the stream,
 * the output buffers and the handle's cap_last_* values untouched.  Nothing is allocated or synchronised (cap_set_early_exit aside). */
typedef struct CapGenerateArgs {
    const void* pixels;        /* B frames in pixel_fmt (device), or B image-state records (16-byte aligned); required */
    int32_t pixel_fmt;         /* CAP_PIX_F32_NCHW | CAP_PIX_U8_NHWC | CAP_PIX_IMAGE_STATE (the image side does not run: "image state" above) */
    int32_t B;
    int32_t num_beams;         /* 1: greedy (HF `_sample` with do_sample=False; CoCa: the reference's top-k(1) loop, coca.py:29); > 1: HF v5 beam
                                  search (CoCa: its `_generate_beamsearch`, coca_model.py:335-482).  CAP_ARCH_BLIP2: the same search behind the
                                  prompt pass, which runs once per IMAGE - the K rows of an image share its cached prompt positions;
                                  max_len counts new tokens, out_ids / out_len are the new tokens of the best hypothesis, out_step_logits
                                  [max_len, B * num_beams, vocab] (step 0: K copies of the image's prompt logits) */
    int32_t num_beam_groups;   /* 0: not a group search.  >= 1 (CAP_ARCH_COCA only): CoCa's `_generate_beamsearch` with beam GROUPS (`generate()`
                                  defaults num_beams = 6, num_beam_groups = 3, coca_model.py:218-219): num_beams % num_beam_groups == 0, each group
                                  a beam search of num_beams / num_beam_groups beams, the best hypothesis over an image's groups returned.  The
                                  reference attaches no diversity processor (:236-241), so its groups are identical searches and the result equals
                                  ONE search of num_beams / num_beam_groups beams - which is what runs (a group of one beam runs as a 1-beam BEAM
                                  search, not as the greedy loop).  No per-step outputs in that mode */
    int32_t max_len;           /* tokens per caption incl. BOS (and the prompt, as HF's max_length); CAP_ARCH_BLIP2: NEW tokens per caption */
    float length_penalty;      /* beam search's scorer (pass 1.0 for the references' default); unused by greedy */
    int32_t* out_ids;          /* int32 [B, max_len]  token ids incl. BOS, rows padded after their end (BLIP-2: the new tokens only); required */
    int32_t* out_len;          /* int32 [B]  tokens in each row incl. BOS and EOS */
    float* out_scores;         /* fp32 [B]  beam `sequences_scores`; untouched for greedy */
    float* out_step_logits;    /* fp32 [steps, B * beams, vocab]  raw per-step logits, steps = max_len - 1 (BLIP-2: max_len; prompted: max_len -
                                  prompt_len).  Greedy: a caption's rows are meaningful up to and including the step that produced its EOS; later
                                  steps of that row are unspecified (the attention kernels skip ended captions; HF feeds them pad and ignores
                                  the result).  With early exit, steps after the last executed one are left untouched */
    float* out_logprobs;       /* fp32 [B, steps], steps = max_len - 1 (BLIP-2: max_len).  Greedy only, together with out_scored: the per-step term
                                  of the reference's `compute_perplexity` (captioning_predictor.py:34-47), taken by the token selection kernel
                                  from the logits row it reads anyway: log max softmax of the step's row as the selection saw it (CoCa: EOS at
                                  -inf while the caption is shorter than min_len) for every step at which the caption was open; 0 after its end,
                                  for steps an early exit never ran, and in the tail of a prompted row.  It is the log of the MAXIMAL probability,
                                  not of the emitted token (they differ on CoCa's forced-EOS last step), as the reference defines it */
    int32_t* out_scored;       /* int32 [B]  steps at which the caption was open = valid entries of its out_logprobs row;
                                  perplexity = exp(-sum_{j < scored} logprobs[j] / scored) */
    float* out_vocab;          /* fp32 [B, acc_ld]  needs the log-prob pair: out_vocab[b][i] = max over the steps at which caption b was open of
                                  softmax(row as selected from)[i], i < vocab (CoCa: 0 for EOS while it is masked) - the vector the reference's
                                  probability fusion builds from per-step logits (captioner/test_pseudo_caption_generation.py:28-63); columns
                                  vocab .. acc_ld - 1 hold the zero fill.  The three greedy outputs are zero-filled by the call on `stream` */
    int32_t acc_ld;            /* row stride of out_vocab: >= vocab, a multiple of 4, and out_vocab 16-byte aligned (the kernel moves 16 bytes) */
    const int32_t* prompt_ids; /* int32 [prompt_rows, prompt_len] (device).  CAP_ARCH_BLIP, greedy: the tokens every caption starts with, column 0 =
                                  BOS (HF `BlipForConditionalGeneration.generate(pixel_values, input_ids=...)`, modeling_blip.py:858-932: the
                                  text decoder receives input_ids[:, :-1]).  Ids are the caller's to validate (engine.py does, on the host); the
                                  library clamps them to [0, vocab) before any gather.  out_ids rows START WITH the prompt and out_len includes
                                  it; the step outputs cover the GENERATED steps only (entry j is the j-th generated token, HF's `logits`
                                  tuple).  Positions 0 .. prompt_len - 2 of all captions run through the decoder as one prefill pass
                                  (caption-major rows, no vocabulary GEMM, no token selection; in chunks of captions when the workspace is
                                  smaller than B x (prompt_len - 1) rows), which leaves the self-attention caches with the BITS the single
                                  steps would have written; the loop then starts at position prompt_len - 1 with everything an unprompted
                                  call has (small-batch path, row compaction, early exit).  A caption prompted with its own unprompted prefix
                                  decodes to the bits of the unprompted call (tests/test_prompt_gpu.py) */
    int32_t prompt_rows;       /* 1 (one prompt shared by the batch) or B (row b for caption b) */
    int32_t prompt_len;        /* 2 <= prompt_len < max_len, <= CAP_MAX_PROMPT (32), and prompt_len - 1 <= the handle's workspace rows
                                  (max(max_batch x max_beams, max_batch x (max_prompt - 1))) - refused with the limit named */
} CapGenerateArgs;
int cap_generate_request(CapHandle h, const CapGenerateArgs* args, void* stream);
/* cap_generate_request with one key per caption for a handle that samples (cap_set_sampling): sample_keys = uint64 [B] (device), caption
 * b's key - two counter words of its Philox draws; NULL = the row index b, which is what every other generating call uses.  The
 * keys hold for this call alone and are ignored with sampling off.  (CapGenerateArgs itself is unchanged.) */
int cap_generate_sampled(CapHandle h, const CapGenerateArgs* args, const uint64_t* sample_keys, void* stream);

/* Conveniences over cap_generate_request: each fills a CapGenerateArgs from its arguments, leaves the rest absent, and goes the same
 * way (messages name the call that was made).
 *   cap_generate           no greedy outputs, no prompt, no groups
 *   cap_generate_scored    + out_logprobs / out_scored (both NULL = cap_generate)
 *   cap_generate_vocab     num_beams = 1, + out_vocab / acc_ld; out_logprobs, out_scored and out_vocab are all required
 *   cap_generate_prompted  num_beams = 1, + prompt_ids (required) / prompt_rows / prompt_len and the greedy outputs
 *   cap_generate_groups    + num_beam_groups (>= 1), no per-step outputs */
int cap_generate(CapHandle h, const void* pixels, int pixel_fmt, int B, int num_beams, int max_len,
                 float length_penalty, int32_t* out_ids, int32_t* out_len, float* out_scores,
                 float* out_step_logits, void* stream);
int cap_generate_scored(CapHandle h, const void* pixels, int pixel_fmt, int B, int num_beams, int max_len,
                        float length_penalty, int32_t* out_ids, int32_t* out_len, float* out_scores,
                        float* out_step_logits, float* out_logprobs, int32_t* out_scored, void* stream);
int cap_generate_vocab(CapHandle h, const void* pixels, int pixel_fmt, int B, int max_len, int32_t* out_ids, int32_t* out_len,
                       float* out_step_logits, float* out_logprobs, int32_t* out_scored, float* out_vocab, int acc_ld,
                       void* stream);
int cap_generate_prompted(CapHandle h, const void* pixels, int pixel_fmt, int B, int max_len, const int32_t* prompt_ids, int prompt_rows,
                          int prompt_len, int32_t* out_ids, int32_t* out_len, float* out_step_logits, float* out_logprobs,
                          int32_t* out_scored, float* out_vocab, int acc_ld, void* stream);
int cap_generate_groups(CapHandle h, const void* pixels, int pixel_fmt, int B, int num_beams, int num_beam_groups, int max_len,
                        float length_penalty, int32_t* out_ids, int32_t* out_len, float* out_scores, void* stream);
/* Prefill passes the last prompted generate on this handle ran (1 = the whole batch at once; 0 after an unprompted call). */
int cap_last_prefill_passes(CapHandle h);

/* Teacher-forced scoring of GIVEN captions (CAP_ARCH_BLIP, CAP_ARCH_BLIP2): what HF `BlipForConditionalGeneration(pixel_values, input_ids=...)` returns
 * as `logits`, reduced on the device to the numbers a caller wants from them.  Nothing vocabulary-wide leaves the library and no
 * [N, L, vocab] buffer exists: the head runs over as many rows as the handle's logits buffer holds and each slice is reduced at once.
 *   pixels   B frames in pixel_fmt (device), B <= max_batch; the image side runs once per image - or B image-state records
 *            (CAP_PIX_IMAGE_STATE): it does not run at all
 *   ids      int32 [N, L] (device), N = B * captions_per_image; caption n belongs to image n / captions_per_image; column 0 = BOS
 *   lens     int32 [N] (device): tokens of caption n incl. BOS (and EOS / [SEP] if the end is to be scored), 2 <= lens[n] <= L, or 0 for
 *            an absent slot (captions_per_image > 1).  Columns from lens[n] on are padding: any id; they influence nothing returned
 *   out_token_logprobs fp32 [N, L - 1]: entry j = log_softmax(logits at position j)[ids[n][j + 1]] for j < lens[n] - 1, 0 behind
 *   out_top_logprobs   fp32 [N, L - 1], out_top_ids int32 [N, L - 1]: log max softmax and arg-max of the same rows (the selection and
 *            tie rule of the greedy loop) - the reference's compute_perplexity on teacher-forced logits, and where the model would have
 *            said something else.  Where the target IS the arg-max the two log-probs are equal bit for bit
 *   out_scored int32 [N] = lens - 1 (0 for an absent slot)
 * The rows are the model's plain logits: no EOS mask, no MinLength.  ids and lens are the caller's to validate (engine.py does, on the
 * host); the library clamps ids to [0, vocab) and lens - 1 to [0, L - 1].  Refused before anything is launched: a CoCa handle
 * (by name: not built), null buffers, captions_per_image < 1, L < 2, L beyond max_len or 32 (BLIP-2: L - 1 beyond max_len, which counts
 * the tokens behind BOS there, or num_query_tokens + L beyond max_pos), B beyond max_batch, and a request no chunking fits (one caption's
 * rows beyond the workspace: the message names the capacity that takes it - CapConfig.max_score_rows, BLIP-2: max_batch).
 * CAP_ARCH_BLIP2 (`Blip2ForConditionalGeneration(pixel_values, input_ids=[image tokens, BOS, caption])`): ids / lens as above (BOS first,
 * the generation EOS last when the end is to be scored).  The encoder, the Q-Former, the projection and the prompt pass (query tokens +
 * BOS) run once per image as in cap_generate; entry 0 of every caption comes from its image's BOS logits; the L - 2 positions behind
 * BOS run as caption-major passes behind the image's cached prompt (opt_prefix_attention: prompt keys from the image's cache row, the
 * caption's own from the pass; nothing is appended to the caches), in the prompt pass's buffers (max_batch x (num_query_tokens + 1)
 * rows per pass), the final LayerNorm and the tied head over every row in slices of max_batch x max_beams rows.  int8 weights: up to
 * the row count of 4 prompts a pass runs on the weight streams, beyond on the tiled GEMM - as the prompt pass does, so bits are the
 * same across chunkings only within one of the two.
 * Passes take whole images while one fits, else part of one image's captions; the result does not depend on the chunking, on the
 * batch a caption is scored in or on the slot it sits in (tests/test_score_captions_gpu.py).  No label smoothing, no loss, no
 * gradients. */
int cap_score_captions(CapHandle h, const void* pixels, int pixel_fmt, int B, const int32_t* ids, const int32_t* lens, int captions_per_image,
                       int L, float* out_token_logprobs, float* out_top_logprobs, int32_t* out_top_ids, int32_t* out_scored, void* stream);
/* Decoder passes the last cap_score_captions on this handle ran (1 = every caption at once). */
int cap_last_score_passes(CapHandle h);
/* Captions of L tokens one decoder pass of cap_score_captions takes on this handle: BLIP min(max_batch x max_beams, workspace rows /
 * (L - 1)), BLIP-2 max_batch x (num_query_tokens + 1) / (L - 2); 0 = a caption of that length cannot be scored (no chunking fits);
 * -1: not a BLIP / BLIP-2 handle, or L outside what cap_score_captions takes. */
int cap_score_pass_captions(CapHandle h, int L);

/* Sentence encoder (CAP_ARCH_MINILM handle; weights by HF BertModel names as sentence-transformers stores them):
 * WordPiece ids int32 [B, L] incl. [CLS]/[SEP] (rows padded with any valid id), lens int32 [B] = valid tokens per row
 * -> out fp32 [B, t_hidden]: mean of the last hidden states over the valid tokens, L2-normalised
 * (sentence-transformers Pooling(mean) + Normalize).  All pointers are device pointers. */
int cap_embed_text(CapHandle h, const int32_t* ids, const int32_t* lens, int B, int L, float* out, void* stream);

/* CLIP scorer (CAP_ARCH_CLIP handle; weights by HF CLIPModel names: vision_model.*, text_model.*, visual_projection.weight,
 * text_projection.weight, logit_scale).  The handle reads v_* (image tower), t_* (text tower), vocab, max_pos, embed_dim
 * (projection width), eos, max_batch and max_len (tokens per caption, <= max_pos).  All pointers are device pointers.
 *   cap_clip_embed_images: B frames in pixel_fmt (normalised with pix_mean / pix_std for CAP_PIX_U8_NHWC) -> out fp32
 *     [B, embed_dim] = normalize(visual_projection(post_layernorm(CLS row)))  (HF get_image_features, then L2-normalised)
 *   cap_clip_embed_text: ids int32 [B, L] (right padded, any ids after the caption), lens int32 [B] = tokens up to and
 *     including the pooled EOT (1 <= lens[b] <= L <= max_len) -> out fp32 [B, embed_dim] = normalize(text_projection(
 *     final_layer_norm(row lens[b] - 1))).  The mask is causal: no row at or before the EOT sees a pad, so no padding mask
 *     exists and the result does not depend on the ids after lens[b] (nor on L).
 *   cap_clip_logits: img [Ni, embed_dim], txt [Nt, embed_dim] (normalised embeddings) -> out = exp(logit_scale) * img . txt^T:
 *     paired = 1 -> out [Ni] (image i against caption i, Ni == Nt: what the reference scores), paired = 0 -> out [Ni, Nt]
 *     (HF's logits_per_image).  Needs no handle.
 *   cap_clip_logit_scale: the checkpoint's `logit_scale` tensor (before exp) -> *out (synchronises).
 * Other architectures' handles refuse the first two; a CLIP handle refuses cap_encode / cap_generate / cap_embed_text. */
int cap_clip_embed_images(CapHandle h, const void* pixels, int pixel_fmt, int B, float* out, void* stream);
int cap_clip_embed_text(CapHandle h, const int32_t* ids, const int32_t* lens, int B, int L, float* out, void* stream);
int cap_clip_logits(const float* img, const float* txt, int Ni, int Nt, int paired, float logit_scale, float* out, int embed_dim,
                    void* stream);
int cap_clip_logit_scale(CapHandle h, float* out);

/* Cosine similarity of sentence embeddings (no handle; fp32 throughout, exact fp32 products on v_mfma_f32_32x32x2_f32).  Rows are NOT
 * assumed normalised: e^_i = e_i / max(||e_i||, 1e-12) (F.normalize), s_ij = e^_i . e^_j - so a zero row has cosine 0 with everything
 * (itself included).  D % 4 == 0, D <= 1024; e / a / b / workspace 16-byte aligned device pointers.  Refusals name what is wrong: null
 * buffers, D % 4 != 0, D > 1024, negative counts, offsets that do not start at 0 / decrease / do not end at N, a workspace too small.
 *   cap_cosine_matrix: a [Na, D], b [Nb, D] -> out [Na, Nb] = s(a_i, b_j); paired = 1 (Na == Nb) -> out [Na] = s(a_i, b_i), bit for bit
 *     the matrix's diagonal.  workspace: (Na + Nb) * 4 bytes, caller-owned.
 *   cap_group_similarity: e [N, D]; G groups of contiguous rows offsets[g] .. offsets[g + 1] - `offsets` is a HOST array of G + 1 ints (it
 *     is checked, sizes the grid and is copied during the call: it may be freed on return when it is pageable memory); weights fp32 [N]
 *     of positive integer counts (captions_frequency's freq) or null = ones.  A weighted statistic is by definition the unweighted
 *     statistic of the group with row i repeated w_i times; W = sum w_i.  Per group g:
 *       disagreement[g] fp32   sum_ij w_i w_j (1 - s_ij) / W^2, diagonal included (the reference's per-object value); empty group: 0
 *       pairs[g]        int64  W (W - 1) / 2
 *       pair_mean[g], pair_var[g] fp32   mean and population variance of s over the unordered pairs of the expanded group (pairs of two
 *                       copies of one row included); 0 when pairs == 0
 *       medoid[g]       int32  the row (index within the call) with the largest row_mean, first index on equal values; empty group: -1
 *     and per row i: row_mean[i] fp32 = (sum_j w_j s_ij - s_ii) / (W - 1), 0 when W == 1.
 *     No floating-point atomics; partial sums are combined in fp64 in a fixed order, so a group's outputs are the same bits wherever the
 *     group sits in the call and whatever other groups the call holds.  Nothing is allocated inside the call:
 *   cap_group_similarity_workspace: the bytes of caller-owned device workspace cap_group_similarity needs for (N, G, D, offsets);
 *     0 (and cap_last_error) when the grouping is refused. */
int cap_cosine_matrix(const float* a, const float* b, int Na, int Nb, int D, int paired, float* out, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t cap_group_similarity_workspace(int N, int G, int D, const int32_t* offsets);
int cap_group_similarity(const float* e, const int32_t* offsets, const float* weights, int N, int G, int D, float* disagreement,
                         float* pair_mean, float* pair_var, int64_t* pairs, int32_t* medoid, float* row_mean, void* workspace,
                         size_t workspace_bytes, void* stream);

/* BLIP-2 image-text scorer (CAP_ARCH_BLIP2_ITM handle; weights by HF `Blip2ForImageTextRetrieval` names: vision_model.*,
 * derived.qformer_x0 [= qformer.layernorm(query_tokens), host-derived], embeddings.word_embeddings.weight,
 * embeddings.position_embeddings.weight, qformer.layernorm.*, qformer.encoder.layer.N.{attention, crossattention, intermediate,
 * output, intermediate_query, output_query}.*, vision_projection.*, text_projection.*, itm_head.*).  The handle reads v_* (ViT-g,
 * head_dim any multiple of 8 up to 128), q_* (Q-Former, heads of 64), num_query_tokens (<= 32), vocab, max_pos (text positions),
 * embed_dim (projection width), max_batch and max_len (tokens per caption, <= 32).  CAP_F32, CAP_F32_SPLIT or CAP_BF16; no int8.
 * All pointers are device pointers.  Text: ids int32 [B, L] (right padded, any ids after the caption), lens int32 [B] = the
 * caption's tokens (HF's attention_mask summed; clamped to 1..L); rows and keys beyond lens[b] do not influence pair b, and
 * neither does L or the batch: the same bits alone, in a batch and padded to a longer L.
 *   cap_blip2_itm_encode_images: B frames in pixel_fmt -> the image tokens (post_layernorm on every token) and the cross-attention
 *     K/V of every cross layer stay RESIDENT in the handle: the ITC and ITM calls below read them, the tower runs once.
 *   cap_blip2_itc_image_features: the B resident images -> out fp32 [B, num_query_tokens, embed_dim] =
 *     normalize(vision_projection(Q-Former(queries, cross-attending the image)))
 *   cap_blip2_itc_text_features: text alone through the Q-Former (no queries, no cross-attention, the text FFN) -> out fp32
 *     [B, embed_dim] = normalize(text_projection(row 0)).  Needs no resident images; B <= max_batch.
 *   cap_blip2_itc_scores: img [Ni, num_queries, embed_dim], txt [Nt, embed_dim] -> max over the queries of img . txt (no
 *     temperature): paired = 1 -> out [Ni] (image i against caption i), paired = 0 -> out [Ni, Nt] (HF's logits_per_image).
 *     Needs no handle.
 *   cap_blip2_itm_logits: pair b = resident image b with caption b (B = the resident batch): rows [queries | text], key mask
 *     [1 x queries | text mask], query rows cross-attend the image -> out_logits fp32 [B, 2] = mean over the query rows of
 *     itm_head; out_prob fp32 [B] = softmax(logits)[:, 1] (the reference's score; may be NULL).
 * Refused by message: text longer than max_len, B beyond max_batch or unequal to the resident batch, another architecture's
 * handle; an image-text scorer handle refuses cap_encode / cap_generate / cap_embed_text / cap_clip_*. */
int cap_blip2_itm_encode_images(CapHandle h, const void* pixels, int pixel_fmt, int B, void* stream);
int cap_blip2_itc_image_features(CapHandle h, int B, float* out, void* stream);
int cap_blip2_itc_text_features(CapHandle h, const int32_t* ids, const int32_t* lens, int B, int L, float* out, void* stream);
int cap_blip2_itc_scores(const float* img, const float* txt, int Ni, int Nt, int paired, float* out, int num_queries, int embed_dim,
                         void* stream);
int cap_blip2_itm_logits(CapHandle h, const int32_t* ids, const int32_t* lens, int B, int L, float* out_logits, float* out_prob,
                         void* stream);

/* Range guard of CAP_F32_SPLIT.  Weights: cap_load_weight refuses (returns -1, message names the tensor) a tensor bound for
 * a GEMM-operand slot whose max |w| exceeds 65000 / 4096 = 15.87 or that holds a NaN - nothing is clipped silently.
 * Activations: every kernel that writes a GEMM operand clamps to +-65000 (fp16's range) and COUNTS what it clamped; this
 * returns the count on the current device since the last reset (groups of four adjacent elements count once), -1 on error.
 * It synchronises the device.  0 means every value of every generate / encode since the reset was inside the envelope in
 * which the mode is fp32-grade; anything else means "run this checkpoint / input in CAP_F32".
 * Reference behaviour replaced: none (fp32 torch on the CPU has no such range) - this is the honesty clause of the fast mode. */
long long cap_g8_saturations(int reset);

/* Bytes of device memory this handle allocated: its arena, plus the weights if it is the handle that created them
 * (cap_create); a cap_create_shared handle reports its arena only. */
size_t cap_device_bytes(CapHandle h);

/* ---- arena state (tests only: no product code calls these) ----
 * Every buffer of a handle's arena has a kind (DESIGN.md "Arena state"):
 *   scratch  fp32 / compute-type / KV16 data that a call writes before it reads - no result may depend on what it held before;
 *   index    int32 tables (token rows, finished / length flags, row maps, beam ancestry, the beam state block);
 *   kept     initialised at create, or carrying state from one ABI call to a later one by documented contract.
 * cap_debug_fill_arena writes the 32-bit pattern over every scratch allocation of THIS handle's arena, rounded tail included,
 * stream-ordered on `stream`, and returns the bytes filled (-1 on error).  Kept and index buffers are not touched, and neither
 * is the weight store (of a cap_create_shared handle or any other).  0xFFFFFFFF is a NaN as fp32, as bf16 and as both fp16
 * halves of a split-fp16 word (and -1 with a NaN scale in a KV16 block); 0x42F742F7 is finite in all of them.
 * Index buffers are not poisoned on purpose: the only way a stale index shows is as an address, and an arbitrary one may lie
 * outside every allocation.  What reaches them is running a different call first (tests/test_arena_state_gpu.py, case d),
 * which leaves in-range but wrong indices behind.
 * cap_debug_arena_kinds writes a JSON object {"arena_bytes": n, "scratch_bytes": n, "index_bytes": n, "kept_bytes": n,
 * "index": ["name", ...], "kept": ["name", ...]} into buf: arena_bytes is cap_device_bytes less the weights this handle
 * created, so the three totals add up to it exactly when every arena allocation is classified; the names are those of the
 * index and kept allocations in allocation order. */
long long cap_debug_fill_arena(CapHandle h, uint32_t pattern, void* stream);
int cap_debug_arena_kinds(CapHandle h, char* buf, size_t buf_bytes);

/* Per-kernel timing with HIP events on the launch stream (bench.py's roofline leg).  While enabled every launch of the
 * tagged kernels is bracketed by an event pair; cap_profile_report synchronises the stream and writes a JSON object
 * {"tag": {"launches": n, "ms": total, "flops": f, "bytes": b}, ...} into buf. */
int cap_profile_enable(CapHandle h, int on);
int cap_profile_report(CapHandle h, char* buf, size_t buf_bytes);

/* ---- single-kernel entry points (used by tests/ to check each kernel against a plain reference) ----
 * dtype CAP_F32_SPLIT follows the mode's convention: GEMM operands (A, W, and a non-fp32 C) and the outputs of kernels that
 * feed a GEMM (layernorm out_t, attention ctx / out) are G8 = 4 bytes per element, every 8 consecutive elements of a row
 * stored as [8 fp16 hi | 8 fp16 lo]; q|k|v, caches and partial sums are fp32. */
int cap_op_gemm(int dtype, const void* A, const void* W, const float* bias, const float* resid, void* C, int M, int N,
                int K, int gelu, int out_f32, int tile, void* stream);
/* split-K form of the decode GEMMs: part[z][M][N] fp32 = A[:, z-th K slice] . W[:, z-th K slice]^T, no bias (the consumer -
 * cap_op_reduce_layernorm, or the decode attention kernels - sums the slices in order).  K % (slab * splitk) == 0 with slab =
 * 32 (fp32, split) / 64 (bf16); tile as cap_op_gemm (2 = the 64x64 decode tile). */
int cap_op_gemm_partial(int dtype, const void* A, const void* W, float* part, int M, int N, int K, int splitk, int tile,
                        void* stream);
int cap_op_layernorm(int dtype, const float* in, const float* gamma, const float* beta, float eps, void* out_t,
                     float* out_f, int M, int D, void* stream);
int cap_op_vit_attention(int dtype, const void* qkv, void* ctx, int B, int N, int H, int impl, void* stream);
/* heads of any width (BLIP-2's ViT-g/14: 88); impl 1 forces the scalar kernel, 0 picks the MFMA kernel where one exists;
 * impl | 8: causal mask (query i sees keys 0..i: the OPT prefill) */
int cap_op_vit_attention_hd(int dtype, const void* qkv, void* ctx, int B, int N, int H, int head_dim, int impl,
                            void* stream);
/* The generic attention launcher alone, unmasked self-attention over fused q|k|v rows [B * N, 3 H head_dim] -> ctx [B * N, H head_dim]:
 * the kernel choice of launch_generic_attention (N <= 64 keys >= 16, heads <= 64 wide: the key-parallel kernel run_qformer's
 * self-attention runs on).  Kernel tests and timing partners; nothing in the product path calls it. */
int cap_op_generic_attention(int dtype, const void* qkv, void* ctx, int B, int N, int H, int head_dim, void* stream);
/* The Q-Former self-attention of the BLIP-2 image-text scorer alone (csrc/blip2_itm.hip): per pair b the keys are the num_queries
 * query rows and the first lens[b] of the L text rows; fused q|k|v rows qkv_q [B * num_queries, 3 H 64] / qkv_t [B * L, 3 H 64] ->
 * ctx_q [B * num_queries, H 64] / ctx_t [B * L, H 64]; at most 32 rows per segment; num_queries = 0 or L = 0 drops a segment. */
int cap_op_itm_self_attention(int dtype, const void* qkv_q, const void* qkv_t, const int32_t* lens, void* ctx_q, void* ctx_t, int B,
                              int num_queries, int L, int H, void* stream);
/* launch_generic_attention with its whole argument list: q / k / v / out in buffers of their own, row strides ld* and batch strides
 * *bs in elements (out: G8 containers count as elements), head h of a row at column h * head_dim.  causal_off >= 0: query i sees keys
 * j <= i + causal_off (the cached decode step and a prompt continuation); < 0: no mask.  Kernel choice: Lq == 1 with Lk <= 1024 the
 * one-query decode kernel, unmasked Lq <= 64 against Lk >= 16 keys at heads <= 64 wide the four-wave key-parallel kernel, everything
 * else the lane = query kernel. */
int cap_op_attention(int dtype, const void* q, int64_t ldq, int64_t qbs, const void* k, int64_t ldk, int64_t kbs, const void* v, int64_t ldv,
                     int64_t vbs, void* out, int64_t ldo, int64_t obs, int B, int Lq, int Lk, int H, int head_dim, int causal_off, void* stream);
/* The cached OPT decode step: one query per (row, head) from the fused q|k|v rows qkv [B, 3 T]; the row's k | v are written to the
 * caches kc / vc [B][Lmax][T] at position past and the query attends to positions 0..past -> out [B, T].  head_dim = T / H a multiple
 * of 8 up to 128, past < min(Lmax, 1024). */
int cap_op_opt_decode_attention(int dtype, const void* qkv, void* kc, void* vc, void* out, int B, int T, int H, int Lmax, int past,
                                void* stream);
/* The same step for the B * K rows of a beam search, row r = image * K + beam, over caches kc / vc [B * K][Lmax][T]: positions below P
 * (the prompt) are read from the cache of row image * K, position P + g (g < past - P) from the cache of row anc[r * anc_ld + g]
 * (clamped into the image's rows), and the row's own k | v are written to ITS cache at position past.  anc may be null for K = 1
 * (every position the row's own).  1 <= K <= 8, 0 <= P <= past, anc_ld >= past - P.  Same sums in the same order as
 * cap_op_opt_decode_attention: a row with the same history gives the same bits. */
/* Self-attention of cap_score_captions' caption pass on a BLIP-2 handle, alone: n new positions of n_caps captions behind a cached
 * prefix.  qkv [n_caps * n, 3 T] fused rows, caption-major (row = caption * n + position); caption cap0 + c belongs to image
 * (cap0 + c) / C, whose P prefix keys are read from row `image` of kc / vc [.][Lmax][T]; the caption's own keys 0 .. position come
 * from the rows themselves (nothing is written to the caches).  n_pos int32 (device, may be NULL): rows with position >=
 * n_pos[cap0 + c] are left untouched.  head_dim = T / H a multiple of 8 up to 128, P + n <= 1024.  out [n_caps * n, T]. */
int cap_op_opt_prefix_attention(int dtype, const void* qkv, const void* kc, const void* vc, void* out, int n_caps, int n, int cap0, int C,
                                const int32_t* n_pos, int T, int H, int Lmax, int P, void* stream);
int cap_op_opt_beam_decode_attention(int dtype, const void* qkv, void* kc, void* vc, void* out, int B, int K, int T, int H, int Lmax, int P,
                                     int past, const int32_t* anc, int anc_ld, void* stream);
/* k | v columns of fused rows qkv [B * L, 3 T] -> caches kc / vc [B][Lmax][T] at positions pos0 .. pos0 + L - 1 (CAP_F32_SPLIT: fp32). */
int cap_op_kv_append(int dtype, const void* qkv, void* kc, void* vc, int B, int L, int T, int Lmax, int pos0, void* stream);
/* The kernels that run once per prompt pass, alone (tests/test_prefill_kernels_gpu.py).  One kernel (or kernel pair) each.
 *   cap_op_prefill_self_attention: the self-attention of a prompt prefill over n_caps * npos rows, row r = position r % npos of caption
 *     row0 + r / npos.  part fp32 [S][n_caps * npos][part_ld] (S 1..4, part_ld % 4 == 0, >= 3 H 64) + bias [3 H 64] are the fused q|k|v
 *     projection; every row's k / v go to positions 0 .. npos - 1 of its caption's cache row (kbase / vbase [.][H][kv_ld][64]:
 *     CAP_BF16 bf16, otherwise fp32), then row (c, p) attends keys 0 .. p -> out [n_caps * npos, H 64] (CAP_F32_SPLIT: G8).
 *     1 <= npos <= min(31, kv_ld).  The bits of npos calls of cap_op_decode_attention_fused with append_kv.
 *   cap_op_opt_prefill_inputs: x fp32 [B, nq + 1, T]: row (b, j) = (j < nq ? proj [B * nq, T] row (b, j) : tok row bos) + pos row j + 2.
 *   cap_op_opt_token_inputs: x fp32 [B, T]: row b = tok row seq[b * seq_ld + cur] (the id clamped to [0, V)) + pos row cur + 2.
 *   cap_op_rows_broadcast: src fp32 [n, D] repeated for B batch items -> dst_f fp32 and dst_t (dtype; CAP_F32_SPLIT: G8, D % 8 == 0),
 *     both [B * n, D].
 *   cap_op_dequant_i8_rowmajor: the bytes of cap_op_quant_i8_pack -> dst_bf16 [rows, cols], the integers as bf16 (exact).
 *   cap_op_scale_cols: part fp32 [M, N] (N % 4 == 0), part[m][n] *= scale[n]. */
int cap_op_prefill_self_attention(int dtype, const float* part, int S, const float* bias, int part_ld, void* kbase, void* vbase, int kv_ld,
                                  void* out, int n_caps, int npos, int row0, int H, void* stream);
int cap_op_opt_prefill_inputs(const float* proj, const float* tok, const float* pos, float* x, int B, int nq, int T, int bos, void* stream);
int cap_op_opt_token_inputs(const int32_t* seq, int seq_ld, int cur, const float* tok, const float* pos, float* x, int B, int T, int V,
                            void* stream);
int cap_op_rows_broadcast(int dtype, const float* src, float* dst_f, void* dst_t, int B, int n, int D, void* stream);
int cap_op_dequant_i8_rowmajor(const void* packed, void* dst_bf16, int rows, int cols, void* stream);
int cap_op_scale_cols(float* part, const float* scale, int M, int N, void* stream);
/* The CoCa attentional pooler's attention: Q projected queries qp [Q, E] (fp32, shared by the batch) over kv [B * N, 2 E] (K then V)
 * -> out [B * Q, E]; head_dim = E / heads is 64 or 96. */
int cap_op_pool_attention(int dtype, const float* qp, const void* kv, void* out, int B, int N, int Q, int E, int heads, void* stream);
/* The sentence encoder's self-attention over fused rows qkv [B * L, 3 H head_dim] with the key mask j < lens[b] (clamped to 1..L) ->
 * ctx [B * L, H head_dim]; CAP_F32 or CAP_BF16, head_dim 32 (L <= 512) or 64 (L <= 256). */
int cap_op_text_attention(int dtype, const void* qkv, const int32_t* lens, void* ctx, int B, int L, int H, int head_dim, void* stream);
/* split-K consumer: y = sum_z part[z][M][D] + bias + resid (-> y_out, may alias resid), LayerNorm(y) -> out_t (dtype) /
 * out_f (fp32); any output may be NULL.  per_row_block: the decoder's workgroup-per-row kernels (few rows). */
int cap_op_reduce_layernorm(int dtype, const float* part, int S, const float* bias, const float* resid,
                            const float* gamma, const float* beta, float eps, void* out_t, float* out_f, float* y_out,
                            int M, int D, int per_row_block, void* stream);
/* bf16 weight-streaming GEMM for a handful of rows (decode step of a large LM): out (bf16) = act(A W^T + bias) when part
 * is NULL, else part[z][M][N] fp32 slice sums.  Returns the slice count used (>= 1) or -1; cap_op_gemm_skinny_slices
 * tells it beforehand (0 = the shape does not fit the kernel). */
int cap_op_gemm_skinny(const void* A, const void* W, const float* bias, int act, void* out, float* part, int M, int N,
                       int K, void* stream);
int cap_op_gemm_skinny_slices(int N, int K, int finished);
/* The int8 form (CapConfig.weight_int8).  cap_op_quant_i8_pack: fp32 W [rows, cols] (rows % 16 == 0, cols % 64 == 0) ->
 * packed (rows * cols bytes, MFMA fragment order: block (t, s) = rows 16 t.., k = 64 s.. is the KiB at (t * cols / 64 + s) * 1024,
 * lane r + 16 g owns bytes 16 l..: k = 64 s + 8 g.. + 7, then k = 64 s + 32 + 8 g.. + 7) and scale [rows] = absmax(row) / 127.
 * cap_op_gemm_skinny_i8: as cap_op_gemm_skinny with (packed, scale) for W; N % 32 == 0; cap_op_gemm_skinny_i8_slices = its plan. */
int cap_op_quant_i8_pack(const float* W, void* packed, float* scale, int rows, int cols, void* stream);
int cap_op_gemm_skinny_i8(const void* A, const void* packed, const float* scale, const float* bias, int act, void* out, float* part,
                          int M, int N, int K, void* stream);
int cap_op_gemm_skinny_i8_slices(int N, int K, int finished);
int cap_op_decode_attention(int dtype, const void* q, const void* kbase, const void* vbase, const int32_t* anc,
                            int anc_ld, int rows_per_kv, int kv_ld, int n_keys, void* out, int R, int H, int impl,
                            void* stream);        /* impl | 16: kbase / vbase are KV16 blocks (no ancestry, > 32 keys) */
/* cap_op_decode_attention as the decoder step launches it (impl & 15 == 0): q is not a tensor but the split-K partial sums of its
 * projection, q_part fp32 [q_S][R][q_ld], the head's columns from q_col0 on, + q_bias - the attention unit finishes the sum and rounds
 * it through the attention's value type.  append_kv (self-attention, n_keys <= 32): columns q_col0 + H 64 / + 2 H 64 are the new
 * position's k / v, finished the same way, written to position n_keys - 1 of the row's own cache and attended. */
int cap_op_decode_attention_fused(int dtype, const float* q_part, int q_S, const float* q_bias, int q_ld, int q_col0, int append_kv,
                                  void* kbase, void* vbase, const int32_t* anc, int anc_ld, int rows_per_kv, int kv_ld, int n_keys,
                                  void* out, int R, int H, int impl, void* stream);
/* The row-wise decode kernels as a merged pass of the compacted greedy loop launches them (tests/test_pass_size_decode_kernels_gpu.py).
 * n_live (device int32, or NULL = every row): rows, row tiles and (row, head) units from *n_live on return at once and leave
 * their outputs alone.
 *   cap_op_gemm_live: cap_op_gemm without a residual, C rows from the count on untouched.  The 64 x 64 / 128 x 128 / 256 x 256
 *     register-staged tiles (tile 2 / 1 / 4), the fp32-output 256 x 256 kernel of the split and bf16 modes (tile 3 / 20) and the
 *     fp32 mode's 256 x 256 kernel (tile 3) take the count; the other kernels ignore it and cover every row.
 *   cap_op_layernorm_live: cap_op_layernorm.
 *   cap_op_decode_attention_live: cap_op_decode_attention_fused (no ancestry, one row per cache block) with the row map - q_part /
 *     out rows are compact rows c, the caches belong to row live[c] (live NULL: c) - and the form of the fused k/v-append kernel:
 *     0 by row count, 1 every key sub-lane finishes its own partial sums, 2 each column finished once per unit; same bits. */
int cap_op_gemm_live(int dtype, const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int gelu, int out_f32,
                     int tile, const int32_t* n_live, void* stream);
int cap_op_layernorm_live(int dtype, const float* in, const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int M,
                          int D, const int32_t* n_live, void* stream);
int cap_op_decode_attention_live(int dtype, const float* q_part, int q_S, const float* q_bias, int q_ld, int q_col0, int append_kv,
                                 void* kbase, void* vbase, int kv_ld, int n_keys, void* out, int R, int H, const int32_t* live,
                                 const int32_t* n_live, int form, void* stream);
/* The small-batch decode kernels alone (csrc/decode_small.hip; at most 16 rows): the launchers' argument structs field for field
 * (csrc/decode_small.h says what each one means).  dtype CAP_BF16: bf16 operands and caches; CAP_F32_SPLIT: G8 operands (weights
 * through cap_op_convert_weight), fp32 self-attention caches, fp32 or KV16 cross K/V.  The hooks check pointers only: every shape
 * is the launcher's to take or refuse. */
typedef struct CapSmallLN {         /* the LayerNorm prologue: LayerNorm(sum of S slabs + bias + resid) */
    const float* part; int32_t S;   /* fp32 [S][R][D] */
    const float* bias;              /* [D] or NULL */
    const float* resid;             /* fp32 [R][D] or NULL */
    const float* gamma; const float* beta; float eps;
    float* x_out;                   /* fp32 [R][D] or NULL: the LayerNorm output (x_is_sum: the sum), written by one workgroup */
    int32_t x_is_sum;
} CapSmallLN;
typedef struct CapSmallSA {         /* the self-attention prologue */
    const float* qkv_part; const float* qkv_bias; int32_t qkv_S;   /* fp32 [qkv_S][R][3 H 64], bias [3 H 64] */
    void* kc; void* vc;             /* [R][H][kv_ld][64] in the cache type */
    const int32_t* anc; int32_t anc_ld;
    int32_t kv_ld, n_keys, H;
    const int32_t* skip;
} CapSmallSA;
typedef struct CapSmallGemm {
    const void* W; const void* A;   /* W [N, K]; A [R, K] (prologue 0) */
    int32_t R, N, K, S;
    int32_t pro, epi, nchain;       /* pro 0 global / 1 LayerNorm / 2 self-attention; epi 0 slabs / 1 act -> operand type / 2 act -> fp32 */
    CapSmallLN ln;
    CapSmallSA sa;
    float* out_part;                /* epi 0: fp32 [S][R][N] */
    const float* bias; int32_t act; /* act 0 none, 1 GELU, 2 ReLU */
    void* out; int32_t ldc;         /* epi 1 / 2: [R, ldc] */
} CapSmallGemm;
typedef struct CapSmallCross {
    const void* W; const float* bias;      /* query projection [D, D], bias [D] */
    int32_t R, D, H, S;
    CapSmallLN ln;
    const void* kbase; const void* vbase; size_t kv_row0;
    int32_t rows_per_kv, kv_ld, n_keys, kv_kind;   /* kv_kind 0 fp32 rows, 1 bf16 rows, 2 KV16 */
    const int32_t* skip;            /* int32 [R] or NULL: rows left untouched */
    void* out;                      /* context [R][D] in the operand type */
} CapSmallCross;
int cap_op_small_gemm(int dtype, const CapSmallGemm* args, void* stream);
int cap_op_small_cross(int dtype, const CapSmallCross* args, void* stream);
/* The split mode's cross-attention K/V cache layout: fp32 rows [n_rows, 64] -> one KV16 block: per row 64 int16 and one fp32 scale
   (x ~ q * scale, scale = max|x| / 32767 over the row), rows in groups of 32 = [32 x 128 bytes][32 scales] = 4224 bytes; dst holds
   (n_rows + 31) / 32 groups.  The cross-K/V GEMM's epilogue writes this layout; the op exists for the kernel tests. */
int cap_op_pack_kv16(const float* src, void* dst, size_t n_rows, void* stream);
/* The two copies behind the image state alone ("image state" above), between a cross K/V cache packed for B images - kind 0 fp32 /
   1 bf16 / 2 KV16, [slot][k | v][image][head][token][64], every (slot, k | v) block as cap_op_gemm_crosskv lays it out - and B records
   at `state` (both device, 16-byte aligned).  pack writes the records whole, zero padding included; unpack writes the head rows (and
   KV16 scales) of the B images and nothing else of the cache: the ragged tail of the last KV16 group and whatever lies behind the
   call's B stay as they were. */
int cap_op_image_state_pack(int kind, int slots, int heads, int tokens, int B, const void* cache, void* state, void* stream);
int cap_op_image_state_unpack(int kind, int slots, int heads, int tokens, int B, void* cache, const void* state, void* stream);
/* The cross-K/V GEMM as the image side runs it (replaces the per-layer key / value Linear calls of HF:modeling_blip_text.py:161-175):
   A [n_img * tokens, K] x W [layers * 2 * heads * 64, K]^T + bias -> cache [layer][k | v][image][head][token][64]; kv16 = 1 (CAP_F32_SPLIT
   only): every (layer, k | v) block is a KV16 block of (n_img * heads * tokens + 31) / 32 groups, else fp32 / bf16 rows. */
int cap_op_gemm_crosskv(int dtype, const void* A, const void* W, const float* bias, void* cache, int n_img, int tokens, int heads,
                        int layers, int K, int kv16, void* stream);
/* launch_gemm with the whole of its parameter struct (csrc/gemm.h, GemmParams; no residual operand), field for field: every epilogue
   on every tile, alone (tests/test_gemm_epilogues_gpu.py).  A [M, lda] x W [N, ldw]^T + bias [N] (may be NULL); tile as cap_op_gemm.
     epi 0 store:     C [M, ldc] (out_f32: fp32, else the operand type), gelu = the activation.
     epi 1 patch:     row (b, p) -> row b * (p0 + 1) + 1 + p of C fp32 [M / p0 * (p0 + 1), ldc], + aux[(1 + p) * N + col]; aux fp32
                      [p0 + 1, N] is the position table, p0 the patches per image; row 0 of every image (the class token) is not written.
     epi 2 cross K/V: C [N / (2 p1 64)][k | v][p2][p1][p0][64], p0 tokens, p1 heads, p2 images (M = p0 p2); element type: the operand
                      type, fp32 for CAP_F32_SPLIT (kv16 = 1: KV16 blocks, as cap_op_gemm_crosskv).
     epi 3 q|k|v:     columns [0, p1 64) -> C [M, p1 64] whatever ldc says; k | v columns -> C2 [k | v][p0][p1][p2][64] at position p3:
                      p0 the row capacity of the cache (>= M), p1 heads, p2 positions; element type as epi 2.
     epi 4 split-K:   C fp32 [splitk][M][ldc], slice z = the product over the z-th K range, no bias; m_live (device int32, or NULL):
                      row tiles that start at or beyond *m_live are not written (epi 0 and 4; which kernels take it: cap_op_gemm_live).
   launch_gemm checks shapes and alignment; the hook refuses, before anything is launched and under its own name, what would make an
   epilogue compute an address outside its buffer: NULL A / W / C, ldc < N (epi 0, 1, 4), epi 1 NULL aux / p0 < 1 / M % p0, epi 2
   p0, p1, p2 < 1 / M != p0 p2 / N % (2 p1 64), epi 3 NULL C2 / N != 3 p1 64 / p0 < M / p3 outside [0, p2), epi 4 splitk < 1, and
   an epi outside 0..4. */
typedef struct CapGemmEpi {
    const void* A; int32_t lda;
    const void* W; int32_t ldw;
    const float* bias;
    void* C; int32_t ldc;
    void* C2;
    const float* aux;
    int32_t M, N, K, gelu, out_f32, epi, splitk;
    int32_t p0, p1, p2, p3;
    int32_t kv16;
    const int32_t* m_live;
    int32_t tile;
} CapGemmEpi;
int cap_op_gemm_epi(int dtype, const CapGemmEpi* args, void* stream);
/* The candidate selection of a beam step alone (first step: running score 0 for beam 0 of an item, -1e9 for the others):
 * logits fp32 [B*K][ld] -> the 2K best (score, token) per row, best first, ties to the lower token id; legacy_raw: scores are
 * raw logits + running score (CoCa), else log-softmax + running score (HF v5); masked_id >= 0: that token scores -inf (legacy
 * MinLength).  Synchronises the stream. */
int cap_op_beam_candidates(const float* logits, int ld, int V, int B, int K, int legacy_raw, int masked_id, float* out_val,
                           int32_t* out_idx, void* stream);
/* The beam search alone, step by step, over a caller-owned device block of cap_op_beam_state_bytes(B, K, max_len) bytes (0 and
 * an error for sizes outside 1 <= K <= 8, B >= 1, max_len >= 2): the launchers cap_generate runs, for the kernel tests.
 * mode 0: HF v5 scoring and stopping, 1: the legacy CoCa scorer (raw logits, min_len masks EOS while cur_len < min_len).
 * init: every item starts as [bos].  step: logits fp32 [B*K][ld] (ld >= V) are the rows of the running beams; cur_len is the
 * number of tokens they hold (BOS included) = the position this step writes, 1 <= cur_len <= max_len - 1, i.e. step
 * cur_len - 1 in [0, max_len - 1); anc int32 [2][B*K][anc_ld] (may be NULL) is the ancestry table, plane cur_len & 1 read,
 * the other written (columns <= cur_len, < anc_ld).  A step issued after the loop's flag has dropped changes nothing.
 * finalize: best hypothesis per item -> out_ids int32 [B][max_len], out_len int32 [B], out_scores fp32 [B] (the last two may
 * be NULL).  peek: running sequences int32 [B*K][max_len] and scores fp32 [B*K] of the given parity (after a step at cur_len:
 * (cur_len + 1) & 1) and the loop-still-running flag (int32 [1]), all device buffers.  Nothing synchronises. */
size_t cap_op_beam_state_bytes(int B, int K, int max_len);
int cap_op_beam_init(void* state, int B, int K, int max_len, int bos, int pad, int eos, int mode, void* stream);
int cap_op_beam_step(void* state, const float* logits, int ld, int V, int B, int K, int max_len, int cur_len, int eos,
                     float length_penalty, int32_t* anc, int anc_ld, int mode, int min_len, void* stream);
int cap_op_beam_finalize(void* state, int B, int K, int max_len, int32_t* out_ids, int32_t* out_len, float* out_scores, void* stream);
int cap_op_beam_peek(void* state, int B, int K, int max_len, int parity, int32_t* run_tokens, float* run_scores, int32_t* active,
                     void* stream);
/* One step of the greedy token selection alone.  logits fp32 [R][ld] (ld % 4 == 0) are the rows of the launch; row c belongs to
 * caption live[c] when a map is given (live int32 [R], n_live int32: rows from *n_live on are skipped), else to caption c.  Per
 * caption (all device, caller-initialised, updated in place): seq int32 [., max_len] receives the token at column t + 1,
 * finished int32 [.], lengths int32 [.].  min_len > 0 masks EOS while t + 1 < min_len; force_eos: CoCa's loop (EOS at the last
 * position, a pad token ends the row).  logprobs fp32 [., lp_ld] (column t) and scored int32 [.] given: the scoring kernel of
 * cap_generate_scored runs (open captions only: the others keep what the caller put there); both NULL: cap_generate's kernel. */
int cap_op_select_logprob(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int min_len, int force_eos,
                          int32_t* finished, const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths,
                          float* logprobs, int lp_ld, int32_t* scored, void* stream);
/* The head consumer of cap_score_captions alone: logits fp32 [rows][ld] (ld >= V, ld % 4 == 0, 16-byte aligned; columns V .. ld - 1 are
 * never read); per row r with live[r] > 0: out_target[r] = log_softmax(row)[targets[r]] (target clamped to [0, V)), out_top[r] = log max
 * softmax, out_top_id[r] = arg-max (lowest index among equal maxima); a dead row (live[r] <= 0) gets zeros and is not read. */
int cap_op_target_logprob(const float* logits, int ld, int V, int rows, const int32_t* targets, const int32_t* live, float* out_target,
                          float* out_top, int32_t* out_top_id, void* stream);
/* cap_op_select_logprob with the vocabulary accumulator of cap_generate_vocab: vocab_acc fp32 [., acc_ld] (caption rows, updated
 * in place for the open captions: entry i < V becomes the larger of itself and the row's softmax at i; acc_ld >= V, acc_ld % 4 == 0,
 * 16-byte aligned).  logprobs / scored are required. */
int cap_op_select_vocab(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int min_len, int force_eos,
                        int32_t* finished, const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths,
                        float* logprobs, int lp_ld, int32_t* scored, float* vocab_acc, int acc_ld, void* stream);
/* The banned forms of the two selections alone (cap_set_bad_words), the set given as the device arrays the kernels read:
 * ban_bits uint32 [cap_op_ban_words(V)] (bit i = token i banned at every step; bits from V on 0), ban_multi int32 [n_multi][9]
 * ({n, tok[0 .. n - 1], zeros}, 2 <= n <= 8; n_multi <= 1024, ban_multi may be NULL when it is 0).
 * cap_op_select_banned: cap_op_select_logprob's plain form (no min_len, no force_eos, no log-probs) over the row with its banned
 * entries at -inf; a caption's context is seq[caption][hist0 .. t] (a sequence of n tokens is looked at when n <= its length).  cap_op_beam_step_banned: cap_op_beam_step with the ban applied
 * to the candidates after the log-softmax of the raw row; a row's history is its running sequence, columns 0 .. cur_len - 1. */
int cap_op_ban_words(int V);
int cap_op_select_banned(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int32_t* finished,
                         const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths, const uint32_t* ban_bits,
                         const int32_t* ban_multi, int n_multi, int hist0, void* stream);
int cap_op_beam_step_banned(void* state, const float* logits, int ld, int V, int B, int K, int max_len, int cur_len, int eos,
                            float length_penalty, int32_t* anc, int anc_ld, int mode, int min_len, const uint32_t* ban_bits,
                            const int32_t* ban_multi, int n_multi, void* stream);
/* The processed forms alone (cap_set_repeat_controls): the banned forms with a penalty (1 = off) and an n-gram size (0 = off); ban_bits
 * may be NULL (no static bitmap; n_multi is then 0).  A row's context is `vn` copies of `vtok`, then its stored history
 * (cap_op_select_processed: seq[caption][hist0 .. t]; cap_op_beam_step_processed: its running sequence, columns 0 .. cur_len - 1),
 * whose first token reads as vbos when vbos >= 0.  The ban sequences match the stored history alone.  HF v5 beam scores only.
 * cap_op_select_processed takes any ld >= V (rows that are not 16-byte aligned are read element by element). */
int cap_op_select_processed(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int32_t* finished,
                            const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths, const uint32_t* ban_bits,
                            const int32_t* ban_multi, int n_multi, int hist0, float penalty, int ngram, int vn, int vtok, int vbos,
                            void* stream);
int cap_op_beam_step_processed(void* state, const float* logits, int ld, int V, int B, int K, int max_len, int cur_len, int eos,
                               float length_penalty, int32_t* anc, int anc_ld, const uint32_t* ban_bits, const int32_t* ban_multi,
                               int n_multi, float penalty, int ngram, int vn, int vtok, int vbos, void* stream);
/* The sampled form alone (cap_set_sampling): cap_op_select_processed's arguments, then the sampling parameters, seed, keys (uint64
 * [captions], device; NULL = the caption's index) and draw (the counter word j), and out_kept (NULL, or int32 [captions]: the entries
 * left with w > 0 after both cuts, written for every caption a logits row maps to). */
int cap_op_select_sampled(const float* logits, int ld, int V, int R, int t, int max_len, int eos, int pad, int32_t* finished,
                          const int32_t* live, const int32_t* n_live, int32_t* seq, int32_t* lengths, const uint32_t* ban_bits,
                          const int32_t* ban_multi, int n_multi, int hist0, float penalty, int ngram, int vn, int vtok, int vbos,
                          float temperature, int top_k, float top_p, uint64_t seed, const uint64_t* keys, int draw, int32_t* out_kept,
                          void* stream);
/* The group step of the probability fusion.  acc fp32 [N, acc_ld] (device); G groups in CSR form, both arrays on the device:
 * group_rows int32 [M] (row indices into acc, in the caller's order, need not be contiguous, each row in one group at most) and
 * group_off int32 [G + 1] (0 = off[0] <= ... <= off[G] = M; an empty group is legal).  Per group, in fp32,
 *   mean(i) = (((a_0 + a_1) + a_2) + ...) / n   over its members in listed order, i < V
 * and the tokens with mean > th (strict) in ascending id order: out_ids int32 [G, K], out_prob fp32 [G, K] (their means; at most K
 * entries written, nothing beyond min(count, K) touched), out_count int32 [G] (always the full count).  The output of a group does
 * not depend on G or on its place in the list.  Refused by name: offsets not monotone or not within M, rows outside [0, N), th not
 * finite, K < 1.  Copies the CSR arrays back for that check: synchronises the stream. */
int cap_op_vocab_group_threshold(const float* acc, int acc_ld, int V, int N, const int32_t* group_rows, int M,
                                 const int32_t* group_off, int G, float th, int K, int32_t* out_ids, float* out_prob,
                                 int32_t* out_count, void* stream);
/* The helper kernels of csrc/elementwise.hip alone (tests/test_elementwise_kernels_gpu.py).  Every pointer is a device pointer
 * unless said otherwise; dtype picks the type of the GEMM-operand output (CAP_F32 fp32, CAP_BF16 bf16, CAP_F32_SPLIT G8: rows of a
 * multiple of 8 elements, refused by name otherwise).  The hooks check pointers and counts; widths and layouts are the launchers'.
 *
 * Decoder embeddings, one step: compact row c < R (c < *n_live when live / n_live are given, both or neither) takes the token
 * seq[(live ? live[c] : c) * seq_ld + t] and gives y_out fp32 [R, D] = word[tok] + pos[t], out_f fp32 / out_t (dtype) [R, D] =
 * LayerNorm(y).  out_t, out_f, y_out may each be NULL.  Tokens are NOT clamped: every token must be inside the word table. */
int cap_op_embed(int dtype, const int32_t* seq, int seq_ld, int t, const float* word, const float* pos, const float* gamma,
                 const float* beta, float eps, void* out_t, float* out_f, float* y_out, int R, int D, const int32_t* live,
                 const int32_t* n_live, void* stream);
/* The same for positions 0 .. npos - 1 of captions row0 .. row0 + n_caps - 1 at once: output row c * npos + p is position p of
 * caption row0 + c, with the bits of cap_op_embed at t = p. */
int cap_op_embed_prompt(int dtype, const int32_t* seq, int seq_ld, int npos, int row0, const float* word, const float* pos,
                        const float* gamma, const float* beta, float eps, void* out_t, float* out_f, float* y_out, int n_caps, int D,
                        void* stream);
/* Sentence-encoder embeddings: row r of R takes ids[r] (clamped to [0, V)) at position r % L:
 * LayerNorm((word[id] + type0) + pos[r % L]) -> out_t (dtype) and out_f fp32 [R, D], both required. */
int cap_op_embed_tokens(int dtype, const int32_t* ids, int L, const float* word, const float* pos, const float* type0,
                        const float* gamma, const float* beta, float eps, void* out_t, float* out_f, int R, int D, int V, void* stream);
/* The sequence rows of a prompted greedy call: seq int32 [R, L] = prompt int32 [prompt_rows, P] (prompt_rows 1 or R; ids clamped to
 * [0, V)) in columns 0 .. P - 1 and pad after it; finished[r] = 0, lengths[r] = L. */
int cap_op_init_prompt_seq(int32_t* seq, int32_t* finished, int32_t* lengths, int R, int L, const int32_t* prompt, int prompt_rows,
                           int P, int V, int pad, void* stream);
/* live int32 [R] = the rows with finished[r] == 0 in ascending order (entries from the count on are left alone), *n_live = count */
int cap_op_compact_rows(const int32_t* finished, int R, int32_t* live, int32_t* n_live, void* stream);
/* Split-K consumer without LayerNorm: out (dtype) [M, N] = act(((part[0] + part[1]) + ...) + bias), part fp32 [S][M][N], bias [N]
 * or NULL, act 0 none / 2 ReLU.  N % 4 == 0. */
int cap_op_reduce_bias_act(int dtype, const float* part, int S, const float* bias, void* out, int M, int N, int act, void* stream);
/* Sentence pooling: out fp32 [B, D] = normalize(mean over the first clamp(lens[b], 1, L) rows of x fp32 [B, L, D]), F.normalize's
 * eps 1e-12.  D % 4 == 0, D <= 1024. */
int cap_op_mean_pool_normalize(const float* x, const int32_t* lens, int B, int L, int D, float* out, void* stream);
/* Patch gather: pixels (fmt CAP_PIX_F32_NCHW fp32 [B, 3, img, img], or CAP_PIX_U8_NHWC uint8 [B, img, img, 3] normalised with
 * (x / 255 - mean[c]) / std[c]) -> out (dtype) [B * (img / ps)^2, Kpad], column c * ps^2 + dy * ps + dx; columns from 3 ps^2 on are
 * left alone.  mean / std: HOST pointers to 3 floats (NULL: 0 / 1). */
int cap_op_patchify(int dtype, const void* pixels, int fmt, int B, int img, int ps, int Kpad, void* out, const float* mean,
                    const float* std, void* stream);
/* X fp32 [B, tokens, D]: X[b, 0, :] = cls + pos[0, :]; nothing else is written */
int cap_op_cls_rows(const float* cls, const float* pos, float* X, int B, int tokens, int D, void* stream);
/* fp32 src [rows, cols] -> dst (dtype), values times scale: dst[r * dst_ld + c] = src[r][c] (columns from cols on left alone), or
 * with transposed != 0 the dense transpose dst[c * rows + r] (dst_ld == rows). */
int cap_op_convert2d(int dtype, const float* src, void* dst, int rows, int cols, int dst_ld, float scale, int transposed, void* stream);
/* *out_bits = max(*out_bits, bit pattern of max |src[i]|): the caller zeroes it.  A NaN gives a pattern above +inf's. */
int cap_op_absmax(const float* src, size_t n, uint32_t* out_bits, void* stream);
int cap_op_convert(int dtype, const float* src, void* dst, size_t n, void* stream);
/* Weight upload as cap_load_weight does it: dst [rows, cols] in the GEMM-operand type of `dtype` (CAP_F32_SPLIT: G8 halves of
 * 4096 * w - the split GEMM's epilogue divides by 4096; a G8 buffer is 4 bytes per element, cols % 8 == 0). */
int cap_op_convert_weight(int dtype, const float* src, void* dst, int rows, int cols, void* stream);
/* The embedding and head kernels of the CLIP and BLIP-2 scorers alone (tests/test_scorer_kernels_gpu.py); their score kernels are
 * cap_clip_logits and cap_blip2_itc_scores above.  Device pointers, fp32 unless said otherwise; the hooks check pointers, every
 * shape limit is the launcher's and is refused by the launcher's name.
 *
 * CLIP text embeddings: x [M, D] = tok[clamp(ids[r], 0, V - 1)] + pos[r % L], tok [V, D], pos [>= L, D]. */
int cap_op_clip_embed_text(const int32_t* ids, int L, const float* tok, const float* pos, float* x, int M, int D, int V, void* stream);
/* CLIP pooled head: row b * rows_per + (lens ? clamp(lens[b], 1, rows_per) - 1 : 0) of x [B * rows_per, D] -> LayerNorm (gamma,
 * beta, eps) -> . W^T (W [P, D], no bias) -> divided by its L2 norm (no eps: a zero projection gives NaN, as HF does) -> out [B, P].
 * lens may be NULL.  D, P <= 1024. */
int cap_op_clip_head(const float* x, int rows_per, const int32_t* lens, const float* gamma, const float* beta, float eps, const float* W,
                     float* out, int B, int D, int P, void* stream);
/* BLIP-2 Q-Former text embeddings: LayerNorm(word[clamp(ids[r], 0, V - 1)] + pos[r % L]) -> x_f fp32 and x_t (dtype: CAP_F32 fp32,
 * CAP_BF16 bf16, CAP_F32_SPLIT G8) [M, D], both required.  D % 8 == 0, D <= 1024. */
int cap_op_itm_embed_text(int dtype, const int32_t* ids, int L, const float* word, const float* pos, const float* gamma,
                          const float* beta, float eps, float* x_f, void* x_t, int M, int D, int V, void* stream);
/* BLIP-2 ITC head: row r * rows_per of x -> . W^T + bias (W [P, D], bias [P]) -> F.normalize (eps 1e-12) -> out [n, P].
 * D, P <= 1024. */
int cap_op_itc_head(const float* x, int rows_per, const float* W, const float* bias, float* out, int n, int D, int P, void* stream);
/* BLIP-2 ITM head: logits [B, 2] = mean over the nq rows of pair b of x [B * nq, D] . W^T + bias (W [2, D], bias [2]);
 * prob [B] = softmax(logits)[1], may be NULL. */
int cap_op_itm_head(const float* x, const float* W, const float* bias, float* logits, float* prob, int B, int nq, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif
