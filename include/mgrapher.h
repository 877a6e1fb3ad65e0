/* mgrapher.h — C ABI of libmgrapher_hip.so
 *
 * MI355X-native (gfx950, hand-written HIP) implementation of ONE path of DS4SD/MarkushGrapher: the
 * MarkushGrapher-2 VTL (UDOP) encoder + autoregressive CXSMILES decoder forward pass, i.e. what the reference
 * reaches through its transformers fork (`transformers.models.markushgrapher`, imported at
 * /root/reference/markushgrapher/core/common/begin.py:7-13):
 *
 *   mg_generate         replaces  model.generate(**encoding, num_beams, max_length)
 *                                 /root/reference/markushgrapher/utils/ocsr/utils_evaluation.py:269-285
 *   mg_encode + mg_decoder_forward
 *                       replace   model(**sample).logits (teacher-forced forward)
 *                                 /root/reference/markushgrapher/core/trainers/curriculumTrainer.py:654-656
 *   mg_encode + mg_decoder_score
 *                       replace   torch.argmax(model(**sample).logits, dim=2) against the labels, and the loss / the
 *                                 log-probability of given sequences, without the logits
 *                                 markushgrapher/core/trainers/curriculumTrainer.py:654-672
 *   mg_encode + mg_decoder_attribute
 *                       replace   the cross_attentions of model(**sample, output_attentions=True), averaged over heads and layers,
 *                                 without the per-layer [B][H][T][S] tensors (config.output_attentions = True,
 *                                 markushgrapher/core/common/begin.py:121)
 *   mg_create / mg_load_tensor / mg_finalize
 *                       replace   MarkushgrapherForConditionalGeneration.from_pretrained(...).to(device)
 *                                 /root/reference/markushgrapher/core/common/begin.py:128-133
 *   mg_beam_reorder     the KV-cache reorder of beam search (stock transformers cache_utils.py:100-104),
 *                       exposed for the beam-reorder micro-benchmark (BASELINE.json configs[2])
 *
 * Conventions: plain pointers and sizes, no framework types.  Every `void* stream` is a hipStream_t.  Every data
 * pointer is a DEVICE pointer unless the name ends in `_host`.  The caller owns all buffers (weights arena,
 * workspace, inputs, outputs); the library allocates no device memory.  Calls only enqueue work on `stream`
 * unless documented as synchronising.  Return value: 0 (MG_OK) or a negative MG_E_* code, message via
 * mg_last_error() (thread-local).  One mg_model may be used from one thread at a time.
 */
#ifndef MGRAPHER_H
#define MGRAPHER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MG_OK = 0, MG_E_SHAPE = -1, MG_E_ARG = -2, MG_E_STATE = -3, MG_E_HIP = -4, MG_E_UNSUPPORTED = -5,
       MG_E_WORKSPACE = -6, MG_E_KEY = -7, MG_E_INPUT = -8 };
enum { MG_KEY_IGNORED = 1 };   /* mg_load_tensor: key recognised as not on this path (e.g. encoder.molscribe_*) */
enum { MG_F32 = 0, MG_BF16 = 1 };

/* UdopConfig fields the path reads (stock transformers models/udop/configuration_udop.py:43-71). */
typedef struct mg_config {
    int vocab_size, d_model, d_kv, d_ff, num_layers, num_decoder_layers, num_heads;
    int relative_attention_num_buckets, relative_attention_max_distance;
    int max_2d_position_embeddings, image_size, patch_size, num_channels;
    int pad_token_id, eos_token_id, decoder_start_token_id;
    float layer_norm_epsilon;
    int max_decode_len;          /* capacity of the decoder self-attention cache / bias table (>= max_length) */
    int tie_word_embeddings;     /* 1 (UDOP / MarkushGrapher default): lm_head = shared.weight, logits scaled by d_model^-0.5
                                    (stock modeling_udop.py:1405-1413,1554-1557) and a checkpoint's lm_head.weight is ignored,
                                    as HF's tie_weights() does; 0: lm_head.weight is a required tensor, no scale */
} mg_config;

typedef struct mg_model mg_model;

int mg_create(const mg_config* cfg, mg_model** out);
void mg_destroy(mg_model* m);
const char* mg_last_error(void);

/* Weights: caller allocates mg_weights_bytes() of device memory and binds it; mg_load_tensor converts one HF
 * state-dict tensor (key = HF name, e.g. "encoder.block.0.layer.0.SelfAttention.q.weight"; device pointer;
 * MG_F32 or MG_BF16) into the library's bf16 fragment-tile layout inside the arena. mg_finalize builds the derived
 * bias tables, ties lm_head to shared.weight when lm_head.weight was not loaded, and checks completeness. */
size_t mg_weights_bytes(const mg_model* m);
int mg_bind_weights(mg_model* m, void* arena);
int mg_load_tensor(mg_model* m, void* stream, const char* hf_key, const void* src, int dtype, const int64_t* shape,
                   int ndim);
int mg_finalize(mg_model* m, void* stream);

/* A further execution context on the weights of a finalized model: the clone reads the same arena (no copy; the arena must
 * outlive it) and owns everything a call mutates - captured decode graph, events, run-ahead stream, profiling state, last-error
 * text is per host thread - so calls on different contexts may run at the same time from different host threads, each on its
 * own stream with its own workspace.  That is how several batches are kept in flight on one GPU: five of the six launches of
 * a decoder layer are latency-sized, a second and third batch's launches fill the machine they leave idle, and every batch's
 * ids are exactly what it gets alone (rows never meet).  Calls on ONE context stay serial.  Tensors loaded later through any
 * of the contexts land in the shared arena; run mg_finalize on the context that loaded them before the next call of any. */
int mg_clone(const mg_model* src, mg_model** out);

/* Workspace for a batch of B images with L text tokens, num_beams beams, decoder length max_length, (for
 * mg_decoder_forward) T teacher-forced positions (0 if unused) and M_e1 OCSR-branch tokens per image (0 if unused). */
int mg_workspace_bytes(const mg_model* m, int B, int L, int num_beams, int max_length, int T, int M_e1, size_t* out_bytes);

/* Encoder (stock modeling_udop.py:1102-1246 for the encoder stack).  attention_mask may be NULL (= everything
 * attended, incl. the zero-padded visual slots: stock:1183-1186).  Leaves the encoder state (final hidden states,
 * mask, compaction map) in the workspace for mg_decoder_forward.
 * enc_out [B][L+P][d_model] fp32 and enc_mask [B][L+P] u8 are optional outputs (the VTL states e2 only).  Rows of enc_out at
 * positions with enc_mask == 0 (padded text slots, the slots of dropped patches) are UNSPECIFIED: nothing downstream reads them
 * (the decoder's cross-attention masks them), and the encoder GEMMs skip whole 32-row tiles of such positions.  Attended rows are
 * bit-identical with the skip off (environment MG_ENC_ROW_TILES=0, which also makes the unattended rows follow the reference).
 * e1 (nullable, with M_e1 = 0): [B][M_e1][d_model] fp32, the projected embeddings of MarkushGrapher-2's OCSR vision branch
 * (`encoder.molscribe_encoder` Swin-B + `encoder.molscribe_projector`, /root/reference/markushgrapher/utils/model/
 * utils_model_loading.py:23,36), computed by the caller: that branch lives only in the reference's un-vendored fork and is
 * NOT part of this library.  They are fused as the reference describes (README.md:212-215: "e1 is
 * concatenated with the VTL embedding e2 and fed to the text decoder"): the decoder cross-attends over [e1 | e2], every e1
 * token attended.  Parity of this fusion is UNPINNED (no fork source): order and normalisation are inferred. */
int mg_encode(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
              const uint8_t* attention_mask, const float* pixel_values, const float* e1, int M_e1, int B, int L,
              float* enc_out, uint8_t* enc_mask);

/* Teacher-forced decoder + lm_head over T positions (stock:1448-1574): logits [B][T][vocab] fp32.
 * decoder_attention_mask may be NULL.  Requires a preceding mg_encode on the same workspace. */
int mg_decoder_forward(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* decoder_input_ids,
                       const uint8_t* decoder_attention_mask, int B, int T, float* logits);

/* Scoring given target tokens: mg_decoder_forward up to the final norm, then the lm_head with the log-softmax, argmax and gather done in
 * the kernel's epilogue (csrc/k_score.hip) - the [B][T][vocab] logits are never stored.  Replaces
 *     logits = model(**sample).logits; torch.argmax(logits, dim=2) compared with the labels
 *                                 markushgrapher/core/trainers/curriculumTrainer.py:654-672
 * and cross_entropy(logits, labels) / the log-probability of a candidate sequence under the model.  Outputs, each [B][T] and nullable:
 *   token_logprobs[b][t]  = log_softmax(logits[b][t])[targets[b][t]]; a negative target (stock's ignore_index) gives 0.0
 *   argmax_ids[b][t]      = lowest index of the largest logit;  argmax_logprobs[b][t] = its log-probability
 * targets may be NULL when token_logprobs is.  A target >= vocab is reported as MG_E_INPUT, like a bad token id.  Requires a preceding
 * mg_encode on the same workspace and may be called several times after it (once per set of candidates).  SYNCHRONISES.  Deterministic;
 * a position's results do not depend on B or T.
 * WORKSPACE: mg_score_workspace_bytes = mg_workspace_bytes(B, L, 1, 0, T, M_e1) plus the kernel's partials (16 bytes per position and
 * 1024 vocabulary columns); a workspace of that size also serves mg_encode / mg_decoder_forward of the same B, L, T. */
int mg_score_workspace_bytes(const mg_model* m, int B, int L, int T, int M_e1, size_t* out_bytes);
int mg_decoder_score(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* decoder_input_ids,
                     const uint8_t* decoder_attention_mask, const int64_t* targets, int B, int T, float* token_logprobs,
                     int64_t* argmax_ids, float* argmax_logprobs);

/* Attribution of given sequences: WHERE in the page each decoder position looked.  mg_decoder_forward's stack with one more launch per
 * selected layer (csrc/k_attrib.hip) that forms the cross-attention softmax from the bf16 Q / K operands of that layer's cross-attention
 * launch and reduces it on the chip - the [B][H][T][S] probabilities per layer that `output_attentions=True` materialises
 * (markushgrapher/core/common/begin.py:121 sets it on every model) are never stored.
 *   p[l][h][b][t][k] = softmax over the ATTENDED keys of (q . k): no scale, no bias (stock UDOP cross-attention), in fp32 - exp(s - max) / sum,
 *                      not the bf16-rounded weights of the P.V product
 *   map[b][t][k]     = 1 / (n_layers * H) * sum_{l = layer_first .. layer_last} sum_h p[l][h][b][t][k]      (ascending l, then ascending h)
 * map [B][T][M_e1 + L + P] fp32, key axis = [e1 tokens | text slots | visual slots]: mg_encode's enc_out / enc_mask order preceded by the
 * OCSR-branch tokens when the preceding mg_encode had them.  Keys with enc_mask == 0 are exactly 0.0; rows with decoder_attention_mask == 0
 * are exactly 0.0; every other row sums to 1 within fp32 rounding.  opts NULL: all decoder layers.
 * Requires a preceding mg_encode on the same workspace and may be called several times after it.  SYNCHRONISES.  Deterministic: an
 * image's map does not depend on B, on the other images, or on T beyond its own row.
 * Errors: MG_E_ARG layers outside [0, num_decoder_layers) or layer_first > layer_last; MG_E_SHAPE T outside [1, max_decode_len rounded up
 * to 64]; MG_E_STATE no preceding mg_encode; MG_E_WORKSPACE; MG_E_INPUT token ids outside the vocabulary, or an image without a single
 * attended key; MG_E_UNSUPPORTED more than 1536 keys per image (L + P + M_e1 rounded up to 64: the kernel keeps a query tile's head sums
 * over all keys in registers).
 * WORKSPACE: mg_attribute_workspace_bytes = mg_workspace_bytes(B, L, 1, 0, T, M_e1) plus the running sums behind it (4 bytes per query
 * and key, both rounded up to 32, plus a 256-byte header); such a workspace also serves mg_encode / mg_decoder_forward of the same B, L, T.
 * NOT built: maps from inside mg_generate* or the queue forms; self-attention and encoder attention maps; per-head or per-layer outputs;
 * rollout or gradient-based attribution; the ChemicalOCR stage. */
typedef struct mg_attr_opts {
    int layer_first, layer_last;     /* inclusive range of decoder layers */
} mg_attr_opts;
int mg_attribute_workspace_bytes(const mg_model* m, int B, int L, int T, int M_e1, size_t* out_bytes);
int mg_decoder_attribute(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* decoder_input_ids,
                         const uint8_t* decoder_attention_mask, int B, int T, const mg_attr_opts* opts, float* map /* [B][T][M_e1 + L + P] */);

/* generate(): encoder once, then KV-cached decode.  num_beams == 1: greedy (stock generation/utils.py:2783-2975);
 * num_beams > 1: beam search (utils.py:3208-3525, beams_to_keep = 2*num_beams, length_penalty, early_stopping 0/1).
 * min_length suppresses EOS while the sequence is shorter (MinLengthLogitsProcessor).
 * out_ids [B][max_length] i64 (row = [start, tok..., eos, pad...]); *out_cols_host = number of valid columns
 * (the length HF's generate would return).  out_scores [B] (beam: sequences_scores; nullable).
 * step_top2 [max_length][B*num_beams][2] fp32 top-1/top-2 logits per step (greedy only, nullable; parity tests).
 * SYNCHRONISES the stream before returning. */
int mg_generate(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                const uint8_t* attention_mask, const float* pixel_values, const float* e1 /* nullable, see mg_encode */,
                int M_e1, int B, int L, int num_beams, int max_length,
                int min_length, float length_penalty, int early_stopping, int64_t* out_ids, int* out_cols_host,
                float* out_scores, float* step_top2);

/* Scored generation: confidence scores and the n-best list of beam search, computed on the device beside the ids.  Every pointer is
 * nullable (device memory); a NULL opts is the unscored call.  rows_out = B * num_return (queue forms: N * num_return), hypotheses of an
 * image consecutive, best first.
 *   num_return    hypotheses per image, in [1, num_beams] (greedy: 1; stock num_return_sequences)
 *   token_scores  [rows_out][max_length-1] f32: column j scores the token in column j+1 of the ids.
 *                 greedy: log_softmax of the step's processed logits at the emitted token - stock compute_transition_scores(sequences,
 *                 scores, normalize_logits=True) for every token up to and including the row's EOS.  MinLength-suppressed stop tokens
 *                 are not part of the normaliser, as in stock's processed scores.  Columns after a row's EOS hold 0.0 (stock scores the
 *                 pad token there).
 *                 beam: the processed log-probability of each token of the hypothesis (without the running score) - stock
 *                 compute_transition_scores(sequences, scores, beam_indices, normalize_logits=False); 0.0 past the hypothesis' length.
 *   seq_scores    [rows_out] f32, beam only: sequences_scores (the length-penalised score).  Replaces out_scores of the unscored call.
 *   beam_indices  [rows_out][max_length-1] i32, beam only: stock beam_indices (flat row image * num_beams + beam each token was chosen
 *                 from; -1 past the hypothesis' length).
 * Beam: out_ids holds rows_out rows; *out_cols_host (queue: out_len[image]) = the longest returned hypothesis' columns.
 * The scores cost little (the greedy lm_head epilogue adds one exp per logit; the beam state keeps one more float history). */
typedef struct mg_gen_opts {
    int num_return;
    float* token_scores;
    float* seq_scores;
    int32_t* beam_indices;
} mg_gen_opts;
int mg_generate_scored(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                       const uint8_t* attention_mask, const float* pixel_values, const float* e1, int M_e1, int B, int L, int num_beams,
                       int max_length, int min_length, float length_penalty, int early_stopping, int64_t* out_ids, int* out_cols_host,
                       float* out_scores, float* step_top2, const mg_gen_opts* opts);

/* Limits: B * num_beams <= 256 live sequences per call (MG_E_UNSUPPORTED beyond; split the batch), num_beams <= 8. */

/* Sampled generation (stock generation/utils.py::_sample with do_sample = True): mg_generate's arguments without the beam ones, plus the
 * options below.  Per live row and step, in stock's warper order: MinLength (EOS removed while the column written is below min_length),
 * temperature (x / T, T > 0), top-k (every token >= the k-th largest value survives, ties included; 0 = off; k clamped to the vocabulary),
 * top-p (a token of value v survives iff the probability mass of the surviving tokens with value <= v exceeds 1 - top_p - stock's rule with
 * the tokens tied at the boundary kept; >= 1 = off; at least one token survives), then one draw from the survivors.
 *   Randomness is counter-based, Philox4x32-10: key = seed, counter = (stream id lo, stream id hi, column written, 0); the two low output
 * words form a 64-bit r and the token is the inverse CDF at r / 2^64 over the survivors in TOKEN-INDEX order.  All of it is integer
 * arithmetic on fixed-point masses (csrc/k_sample.hip), so a call is reproducible run to run, and a row's draws depend on (seed, stream id,
 * column, its own logits) only: with the cross-attention form pinned (mg_set_cross_absorb 0 or 1) a row's ids do not depend on the size of
 * its call or on its place in it.
 *   num_return    samples per image: R = B * num_return <= 256 decode rows, row b * num_return + j = sample j of image b (stock's order for
 *                 num_return_sequences), each with its own self-attention cache; the encoder and the cross K/V (or the compacted encoder
 *                 states) are computed once per image and read by its rows through a row -> image map.  The rows are greedy-form rows:
 *                 the cross-attention form follows mg_set_cross_absorb by R, as for a greedy call of R rows.
 *   stream_ids    [B * num_return] u64 device, nullable: the rows' stream ids (NULL: the row index)
 *   token_scores  [B * num_return][max_length - 1] f32 device, nullable: the log-probability of each drawn token under the warped
 *                 (filtered, renormalised) distribution - stock compute_transition_scores(sequences, scores, normalize_logits=True) on its
 *                 processed scores; 0.0 after a row's EOS
 * out_ids [B * num_return][max_length]; *out_cols_host as mg_generate; step_top2 [max_length][B * num_return][2] nullable (top-2 of the
 * logits before temperature).
 * WORKSPACE: size it with mg_sampled_workspace_bytes (below), NOT with mg_workspace_bytes.  For num_return = 1 the two agree.  For
 * num_return > 1 they do not: mg_workspace_bytes(num_beams = num_return) sizes a beam-search call, whose cross-attention buffers follow
 * mg_set_beam_cross_absorb, while a sampled call's rows are greedy rows and follow mg_set_cross_absorb by B * num_return; a workspace
 * sized for the one may be too small for the other (MG_E_WORKSPACE).  mg_workspace_bytes keeps reporting exactly what beam search needs.
 * Runs under the decode
 * graph like the other batch forms (every option is part of the captured step's key); mg_debug_decode_capture's logits capture works, its
 * forced ids do not (MG_E_UNSUPPORTED).  Vocabulary <= 36 864 (the selection keeps the row in registers).
 * The greedy queue has a sampled form, mg_generate_stream_sampled (below, after mg_generate_stream).
 * NOT built: the beam and OCR queues and the OCR stage under sampling, one cross-attention pass shared by the samples of an image (the
 * beam form's group = num_return), a Gumbel-max variant on the fused lm_head tail, beam-sample. */
typedef struct mg_sample_opts {
    float temperature;
    int top_k;
    float top_p;
    uint64_t seed;
    const uint64_t* stream_ids;
    int num_return;
    float* token_scores;
} mg_sample_opts;
int mg_sampled_workspace_bytes(const mg_model* m, int B, int L, int num_return, int max_length, int M_e1, size_t* out_bytes);
int mg_generate_sampled(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                        const uint8_t* attention_mask, const float* pixel_values, const float* e1, int M_e1, int B, int L, int max_length,
                        int min_length, int64_t* out_ids, int* out_cols_host, float* step_top2, const mg_sample_opts* opts);

/* Decoder prompt (stock generate(decoder_input_ids=...)): fix the beginning of every answer and let the model write the rest.  One entry
 * for the three batch decode modes: mg_generate_scored's arguments (greedy, beam search; opts nullable), or a sampled call (samp non-NULL:
 * mg_generate_sampled's semantics, num_beams must be 1, opts / length_penalty / early_stopping / out_scores are not used), plus the prompt.
 * prompt == NULL is exactly the unprompted call.
 *   Image b has the prompt ids[b][0 .. len_host[b]); ids[b][0] is the token fed at step 0 (stock puts decoder_start_token_id there).  It
 * serves all rows of the image: its num_beams beams or its samp->num_return samples.  Every row starts at column 0 and the call keeps ONE
 * step counter.  While the column a row writes is below its prompt length the selection kernel writes the prompt's token there, not its
 * own choice; afterwards the row decodes freely.  The forced steps are ordinary decode steps: they fill the self-attention cache through
 * the same projection and attention launches, so positions, relative bias and cache layout are those of the unprompted call, and the
 * forcing happens inside the selection kernels, under the captured decode step (mg_set_decode_graph 0 / 1 / 2 all take it).  A forced column
 *   - never finishes a row, even when the forced token is EOS (stock tests generated tokens only);
 *   - consumes no random draw (the draws are counter-based on (seed, stream id, column): free columns draw what they would draw anyway);
 *   - leaves token_scores at 0.0 - the log-probability of a given prefix is what mg_decoder_score returns;
 *   - keeps the row live for the attention launches.
 * min_length keeps its meaning: EOS is suppressed while the column is below min_length, prompt columns included (stock's
 * MinLengthLogitsProcessor counts the whole sequence).  Outputs include the prompt columns; *out_cols_host counts them.
 *   Beam search follows stock _beam_search with decoder_prompt_len = len_host[b], per image: the K rows start holding the prompt with scores
 * [0, -1e9, ...]; a forced column appends the token to every beam (beam index = identity, running scores and the finished set untouched,
 * log-probability history 0); from the image's first free column on the finished-score divisor is (cur_len + 1 - len)^length_penalty and the
 * early-stop heuristic's best hypothetical length cur_len - len.  beam_indices hold the image's beam-0 flat row in forced columns
 * (non-negative, so compute_transition_scores keeps working), token_scores 0.0.
 *   Two properties follow.  (1) Self-prefix identity: if the prompt is a prefix of what the same call emits unprompted (greedy; sampled with
 * the same seed and stream ids), ids, length and the free columns of token_scores are bit-identical to the unprompted call; a prompt of
 * [start] alone IS the unprompted call, in all three modes.  (2) Row b of a ragged batch equals the call on image b alone with its prompt,
 * under the conditions of the project's call-size independence (cross-attention form pinned).
 *   Checks: ids / len_host non-NULL, ld >= 1, 1 <= len_host[b] <= ld and len_host[b] < max_length (MG_E_ARG); a prompt while
 * mg_debug_decode_capture's forced ids are set: MG_E_UNSUPPORTED (its logits capture alone keeps working); a prompt id outside [0, vocab) is
 * replaced by id 0, never indexes the embedding table, and the call returns MG_E_INPUT, as for encoder ids.
 *   WORKSPACE: mg_prompted_workspace_bytes = the unprompted call's size (mg_workspace_bytes with rows_per_image = num_beams, or
 * mg_sampled_workspace_bytes with rows_per_image = num_return when sampled != 0) plus the [B] lengths, which are validated on the host
 * and uploaded behind the unprompted layout.  ids stay where the caller put them: keep them (and the workspace) in place between calls
 * and a later call of the same shape replays the captured step (pointers and ld are part of its key, the lengths are device data).
 *   The queue forms take a prompt per image: mg_generate_stream_constrained / mg_generate_stream_beam_constrained (below, after the queue forms).
 *   NOT built: the OCR stage under a prompt; a PREFILL of the prompt - one teacher-forced pass
 * that writes the self-attention cache of all prompt positions would replace len - 1 decode steps, and would give up property (1): its
 * large-M projections sum in another order than the decode step's. */
typedef struct mg_decoder_prompt {
    const int64_t* ids;       /* [B][ld] device */
    const int32_t* len_host;  /* [B] host */
    int ld;
} mg_decoder_prompt;
int mg_prompted_workspace_bytes(const mg_model* m, int B, int L, int rows_per_image, int max_length, int M_e1, int sampled, size_t* out_bytes);
int mg_generate_prompted(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                         const uint8_t* attention_mask, const float* pixel_values, const float* e1, int M_e1, int B, int L, int num_beams,
                         int max_length, int min_length, float length_penalty, int early_stopping, int64_t* out_ids, int* out_cols_host,
                         float* out_scores, float* step_top2, const mg_gen_opts* opts, const mg_sample_opts* samp,
                         const mg_decoder_prompt* prompt);

/* Constrained decoding: a set of allowed tokens that depends on what a row has emitted so far, as a finite automaton over token classes
 * that the selection kernels consult and advance inside the captured decode step.  Token t has class cls[t]; a row in state s may emit t
 * iff table[s][cls[t]] >= 0, and that entry is its next state.  The LAST state is the sink: it allows EOS only, and EOS is a class of its
 * own.  Banned tokens and multi-token words, tokens banned at the first free position and "answer with one of these sequences" all
 * compile to this (markushgrapher_amd/constraint.py builds them and checks the conventions).
 *   mg_generate_constrained = mg_generate_prompted plus the constraint; constraint == NULL is exactly mg_generate_prompted.  Greedy
 * (num_beams = 1, samp NULL), beam-search and sampled calls take it; all rows of an image (its beams or samples) start from start_host[b], the image's state at
 * its first free column - with a decoder prompt the caller passes the state after the prompt: forced columns leave the state untouched.
 *   - A disallowed token is treated exactly as MinLength's suppressed EOS: it cannot be chosen, is left out of step_top2 and out of the
 *     normaliser of token_scores (greedy), and becomes -inf before temperature, top-k and top-p (sampled); draws keep their counter and stream.
 *   - A constrained greedy call runs the unfused selection tail, as sampled calls do.
 *   - A finished row emits pad and keeps its state.
 *   - Empty allowed set (MinLength and the state together leave nothing, e.g. an EOS-only state below min_length): the row emits EOS and
 *     ends, moves to the sink, scores 0.0, draws nothing; the call completes and returns MG_E_INPUT, as it does for bad ids.
 *   cls, table and their sizes are part of the captured step's key: keep them in place (and refill them in place for another automaton of
 * the same sizes) and a later call of the same shape replays the graph.  States and start states are device data, reset by every call.
 *   Checks (MG_E_ARG): non-null pointers, 1 <= n_classes <= 4096, n_states >= 2, n_states * n_classes <= 2^24, every start_host[b] in
 * [0, n_states).  The ENTRIES of cls (< n_classes) and table (-1 or < n_states) are NOT checked here: they live on the device; the Python
 * layer checks them on the host before it uploads them (TokenAutomaton's constructor).  A constraint while mg_debug_decode_capture's forced
 * ids are set: MG_E_UNSUPPORTED.
 *   WORKSPACE: mg_constrained_workspace_bytes = mg_prompted_workspace_bytes plus the [rows] states, the class row padded to the logits'
 * row stride and the counter, which follow the prompted layout.
 *   Beam search: the log-softmax stays over the raw logits and the mask sets a candidate's log-probability to -inf where MinLength's EOS is
 * set (stock's order: log_softmax, then the processors); the states of an image's K rows are reordered with the beams.  There is no
 * empty-set rule: -inf candidates are ranked, as in stock, and a beam that takes one moves to the sink.
 *   The queue forms take a constraint with a start state per image: mg_generate_stream_constrained / mg_generate_stream_beam_constrained (below).
 *   NOT built: the OCR stage
 * under a constraint; the mask inside the fused lm_head epilogue; sparse tables for automata beyond 2^24 entries; forced_eos_token_id;
 * repetition_penalty and no_repeat_ngram_size (they change logit values or need unbounded history: not masks). */
typedef struct mg_constraint {
    const uint16_t* cls;         /* [vocab] device */
    const int32_t* table;        /* [n_states][n_classes] device */
    int n_states, n_classes;
    const int32_t* start_host;   /* [B] host: each image's state at its first free column */
} mg_constraint;
int mg_constrained_workspace_bytes(const mg_model* m, int B, int L, int rows_per_image, int max_length, int M_e1, int sampled, size_t* out_bytes);
int mg_generate_constrained(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                            const uint8_t* attention_mask, const float* pixel_values, const float* e1, int M_e1, int B, int L, int num_beams,
                            int max_length, int min_length, float length_penalty, int early_stopping, int64_t* out_ids, int* out_cols_host,
                            float* out_scores, float* step_top2, const mg_gen_opts* opts, const mg_sample_opts* samp,
                            const mg_decoder_prompt* prompt, const mg_constraint* constraint);

/* Continuous greedy decoding of N images - what the reference's evaluation loop does one image at a time with
 * model.generate(**encoding, num_beams=1, max_length=512) until EOS (/root/reference/markushgrapher/utils/ocsr/utils_evaluation.py:140,
 * 269-285), for a whole queue of images: `slots` decode rows work through the queue, a row that ends (EOS / max_length) frees its
 * slot for the next image (no step is spent on finished rows, the batch does not wait for its longest member), and the encoder +
 * cross-K/V projection of the next `chunk` images run ahead on a second stream underneath the launch-bound decode steps.
 *   inputs   input_ids [N][L] i64, bbox [N][L][4] f32, attention_mask [N][L] u8 (nullable), pixel_values [N][3][I][I] f32, all resident
 *   outputs  out_ids [N][max_length] i64 (row = [start, tok..., eos, pad...]), out_len [N] i32 = valid columns per image (device)
 *   chunk    images per encoder pass (32); slots = live decode rows (<= 256); pool_chunks >= 2: the cross-K/V pool holds
 *            pool_chunks * chunk images (the encoder runs at most that far ahead of the oldest unfinished image)
 * Every image's ids equal mg_generate's for that image.  *steps_host (nullable) = decode steps run.  SYNCHRONISES before returning. */
int mg_stream_workspace_bytes(const mg_model* m, int chunk, int L, int slots, int pool_chunks, size_t* out_bytes);
int mg_generate_stream(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                       const uint8_t* attention_mask, const float* pixel_values, int N, int L, int chunk, int slots, int pool_chunks,
                       int max_length, int min_length, int64_t* out_ids, int32_t* out_len, long* steps_host);
/* The same queue under SAMPLING (mg_sample_opts, see mg_generate_sampled): a queue of N images with num_return samples each is a queue of
 * N * num_return SEQUENCES, sequence n * num_return + j = sample j of image n.  `slots` (<= 256, <= pool_chunks * chunk * num_return)
 * greedy-form decode rows work through the sequences in order; the samples of an image may sit in different slots at different times and
 * end independently.  One encoder pass and one pool entry per image whatever num_return is: an entry is reused only when every sample of
 * its image has finished.  The draw of sequence q at a column uses the Philox counter (stream_ids ? stream_ids[q] : q, column) - the
 * sequence's place in the queue, never its slot - so with the cross-attention form pinned its ids, length and token scores are exactly
 * those of mg_generate_sampled on its image alone with that stream id, and do not depend on chunk / slots / pool_chunks.
 *   outputs  out_ids [N * num_return][max_length], out_len [N * num_return], opts->token_scores [N * num_return][max_length - 1] (nullable),
 *            opts->stream_ids [N * num_return] (nullable: the sequence index)
 * WORKSPACE: mg_stream_workspace_bytes(chunk, L, slots, pool_chunks) - the rows are greedy-form rows; the cross-attention form follows
 * mg_set_cross_absorb by `slots`, as for the greedy queue.  Checks: temperature > 0, top_k >= 0, 0 < top_p <= 1, num_return >= 1 (MG_E_ARG),
 * vocabulary <= 36 864 (MG_E_UNSUPPORTED).  Every option is part of the captured step's key.  SYNCHRONISES before returning. */
int mg_generate_stream_sampled(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                               const uint8_t* attention_mask, const float* pixel_values, int N, int L, int chunk, int slots,
                               int pool_chunks, int max_length, int min_length, int64_t* out_ids, int32_t* out_len, long* steps_host,
                               const mg_sample_opts* opts);
/* The same queue with BEAM SEARCH - the reference's shipped decode mode (/root/reference/config/predict.yaml:12-13 beam_search: True;
 * utils_evaluation.py:269-285 generate(num_beams=5, max_length=512)): `slots` IMAGE slots of num_beams rows each (slots * num_beams <= 256)
 * work through the queue; an image whose own stopping condition holds (stock 5.15 generation/utils.py:3055-3075 for that image alone - in a
 * batch call such an image is frozen until the whole batch stops) is written out and its slot handed to the next image.
 *   outputs  out_ids [N][max_length] i64 = best hypothesis (unfinished tails filled as stock does), out_len [N] = its columns,
 *            out_scores [N] f32 (nullable) = its length-penalised score
 * Every image's hypothesis and score equal mg_generate(num_beams)'s for that image.  SYNCHRONISES before returning. */
int mg_stream_beam_workspace_bytes(const mg_model* m, int chunk, int L, int slots, int pool_chunks, int num_beams, int max_length, size_t* out_bytes);
int mg_generate_stream_beam(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                            const uint8_t* attention_mask, const float* pixel_values, int N, int L, int chunk, int slots, int pool_chunks,
                            int num_beams, int max_length, int min_length, float length_penalty, int early_stopping, int64_t* out_ids,
                            int32_t* out_len, float* out_scores, long* steps_host);
/* The queue forms with the outputs of mg_gen_opts (see mg_generate_scored): token_scores / seq_scores / beam_indices per image
 * (rows_out = N * num_return; beam: out_ids [N * num_return][max_length], out_len [N] = the longest returned hypothesis' columns). */
int mg_generate_stream_scored(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                              const uint8_t* attention_mask, const float* pixel_values, int N, int L, int chunk, int slots, int pool_chunks,
                              int max_length, int min_length, int64_t* out_ids, int32_t* out_len, long* steps_host, const mg_gen_opts* opts);
int mg_generate_stream_beam_scored(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                                   const uint8_t* attention_mask, const float* pixel_values, int N, int L, int chunk, int slots, int pool_chunks,
                                   int num_beams, int max_length, int min_length, float length_penalty, int early_stopping, int64_t* out_ids,
                                   int32_t* out_len, long* steps_host, const mg_gen_opts* opts);
/* The queue forms under a decoder prompt and / or a constraint (mg_decoder_prompt, mg_constraint: see mg_generate_prompted and
 * mg_generate_constrained).  Greedy and sampled queue: mg_generate_stream_scored's arguments plus samp (nullable; non-NULL selects the sampled queue, whose outputs
 * are samp's and opts is then ignored), prompt and constraint (both nullable; both NULL is exactly the existing call: same bits, same captured
 * step).  Prompt and start state are PER IMAGE of the queue - prompt->ids [N][ld] (device), prompt->len_host [N], constraint->start_host [N]
 * (host) - and shared by the num_return samples of an image.
 * Beam queue: mg_generate_stream_beam_constrained = mg_generate_stream_beam_scored's arguments plus prompt and constraint (opts nullable).
 *   Sequence q equals the batch call (mg_generate_constrained, greedy, beam search, or sampled with stream id q) on its image alone with that
 * image's prompt and start state: ids, length and token_scores bit for bit - for beam search the n-best list, sequence scores and beam_indices
 * as the queue numbers them - with the cross-attention form pinned, whatever chunk / slots / pool_chunks are.  A prompt of [start] alone and / or an automaton that allows everything give the plain queue's ids, lengths and token scores; a prompt
 * that is a prefix of what the plain queue writes for its image reproduces it (token scores 0.0 in the forced columns).
 *   Everything the batch contract says holds per slot row, the owner of a row being the image of the sequence in its slot:
 *   - a sequence enters its slot with its image's first prompt token where stock puts decoder_start_token_id (column 0 of out_ids holds it)
 *     and in its image's start state; the slot's previous state is gone with the sequence that left;
 *   - a forced column takes the prompt's token, never finishes the row (a forced EOS included), draws nothing, scores 0.0 and leaves the
 *     state alone; min_length counts forced columns; a disallowed token is treated exactly as MinLength's EOS;
 *   - empty allowed set: the row emits EOS, ends, FREES ITS SLOT, scores 0.0 and is counted; the call completes with every other sequence
 *     right and returns MG_E_INPUT;
 *   - a prompt id outside [0, vocab) becomes id 0 and the call returns MG_E_INPUT;
 *   - "a finished row emits pad and keeps its state" has no counterpart: a finished row leaves.
 *   Beam search: a newly assigned slot starts as mg_generate_constrained starts its image (the prompt in both sequence arrays, scores
 * [0, -1e9, ...], the K states at the image's start state, the prompt's first token fed first); the mask follows the log-softmax, the K states
 * of a slot are reordered with its beams, there is no empty-set rule; the finished-score divisor is (cur_len + 1 - len)^length_penalty and the
 * early-stop heuristic's length cur_len - len with len the prompt length of the image in the slot; beam_indices hold the image's beam-0
 * flat row in forced columns, token_scores 0.0.
 *   A constrained greedy queue runs the selection it always runs (the queue's tail is unfused); the cost is the class loads.
 *   Checks as the batch functions', MG_E_ARG naming image [n]; the decode-capture instrumentation stays refused (MG_E_STATE) as for all queue
 * calls.  ids, ld, cls, table, n_states, n_classes and the presence of each are part of the captured step's key; lengths, start states and
 * states are device data: refilling tables or ids in place and calling again replays the graph, and a plain queue call in between never
 * replays a constrained step or vice versa.
 *   WORKSPACE: mg_stream_constrained_workspace_bytes = the queue's size (mg_stream_workspace_bytes; num_beams > 1:
 * mg_stream_beam_workspace_bytes) plus, behind that layout, the [N] lengths and [N] start states (validated on the host, uploaded by the
 * call), the [slots * num_beams] states, the class row padded to the logits' row stride and the counters.
 *   SYNCHRONISES before returning. */
int mg_stream_constrained_workspace_bytes(const mg_model* m, int chunk, int L, int slots, int pool_chunks, int num_beams, int max_length, int N,
                                          size_t* out_bytes);
int mg_generate_stream_constrained(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                                   const uint8_t* attention_mask, const float* pixel_values, int N, int L, int chunk, int slots, int pool_chunks,
                                   int max_length, int min_length, int64_t* out_ids, int32_t* out_len, long* steps_host, const mg_gen_opts* opts,
                                   const mg_sample_opts* samp, const mg_decoder_prompt* prompt, const mg_constraint* constraint);
int mg_generate_stream_beam_constrained(mg_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* bbox,
                                        const uint8_t* attention_mask, const float* pixel_values, int N, int L, int chunk, int slots,
                                        int pool_chunks, int num_beams, int max_length, int min_length, float length_penalty, int early_stopping,
                                        int64_t* out_ids, int32_t* out_len, long* steps_host, const mg_gen_opts* opts,
                                        const mg_decoder_prompt* prompt, const mg_constraint* constraint);
/* Where the encoder of mg_generate_stream runs: 0 = on the caller's stream (serial), 1 = own stream at the lowest priority
 * (default), 2 = own stream restricted to the compute units of cu_mask (nwords x 32 bits, hipExtStreamCreateWithCUMask). */
int mg_stream_encoder_mode(mg_model* m, int mode, const uint32_t* cu_mask, int nwords);

/* Parity-test instrumentation of mg_generate (tests only; while set, the decode steps are launched eagerly with by-value
 * arguments instead of replaying the captured graph - the same kernels).  logits_capture [capture_steps][B*num_beams][vocab]
 * fp32 (device) receives the pre-argmax logits of decode steps 0 .. capture_steps-1.  forced_ids [B][max_length] i64
 * (device, greedy only): the token fed into step t+1 is forced_ids[b][t+1] instead of step t's argmax, i.e. teacher
 * forcing THROUGH the KV-cached decode path; out_ids / step_top2 still record every step's own selection.  NULL clears. */
int mg_debug_decode_capture(mg_model* m, float* logits_capture, int capture_steps, const int64_t* forced_ids);

/* Beam-search KV-cache reorder, physical form: for every decoder layer, dst K/V rows [r] = src rows [beam_idx[r]]
 * (cache_utils.py:100-104 index_select).  kv_src/kv_dst: [layers][2][rows][H][t_cap][64] bf16; only the first
 * `t_used` positions of every row are copied. */
int mg_beam_reorder(void* stream, const void* kv_src, void* kv_dst, const int32_t* beam_idx, int layers, int rows,
                    int H, int t_cap, int t_used);

/* Live timing of the dominant decode kernel (single-query cross-attention over the per-image K/V stream): when
 * every > 0, each `every`-th decode step of mg_generate brackets every decoder layer's launch with HIP events on the
 * caller's stream (at most max_samples launches per call). mg_profile_read returns the number of launches timed, their
 * summed duration and the summed number of (image, key) rows each of them streamed (bytes = rows * H * 64 * 2 * 2). */
int mg_profile_cross_attention(mg_model* m, int every, int max_samples);
int mg_profile_read(mg_model* m, long* launches_host, double* total_ms_host, double* total_keys_host);
/* Calibration of the bracket: after every timed launch a third event is recorded right behind the second; this returns
 * the summed duration of those EMPTY brackets (what two hipEventRecord cost on the stream with nothing in between). */
int mg_profile_read_overhead(mg_model* m, double* empty_ms_host);
/* Phase timing of mg_generate: three HIP events per call bracket [encoder + cross-K/V precompute] and [decode loop];
 * mg_profile_phases_read returns the number of calls and the summed durations since it was enabled. */
int mg_profile_phases(mg_model* m, int enable);
int mg_profile_phases_read(mg_model* m, long* calls_host, double* enc_ms_host, double* dec_ms_host);
int mg_debug_bucket_table(const mg_model* m, int which, int* out_host, int n);

/* Decode-step replay. The ~200 launches of one decode step (the body of the reference's generation loop,
 * transformers generation/utils.py `_sample` / `_beam_search` while-loop) are captured once as a HIP graph whose
 * kernels read the step index from device memory; later steps - and later calls with the same buffers and
 * generation arguments - replay it with one hipGraphLaunch. enable = 0 launches every kernel eagerly (same kernels,
 * same results); enable = 2 launches the graph's device-counter form of the kernels eagerly (test hook). Default: 1.
 * Returns the previous setting. */
int mg_set_decode_graph(mg_model* m, int enable);
/* Trailing text padding of a batch (attention_mask with zeros at the end of a row).  0 (default): the padded slots are part of the
 * sequence, exactly as stock HF computes a padded batch - UDOP's 1-D relative position bias then counts them between the text and
 * the patches, so an image's result depends (slightly) on how far its batch was padded.  1: per-image semantics - every image's
 * patches follow its own last attended text token and its result is what the reference's batch-size-1 loop computes for it
 * (/root/reference/markushgrapher/utils/ocsr/utils_evaluation.py:140), whatever its batch mates are.  Returns the previous setting. */
int mg_set_padding_semantics(mg_model* m, int per_image);
/* Several execution contexts share the GPU (mg_clone; markushgrapher_amd/inflight.py sets it on the contexts it runs).  shared = 1: the one
 * long-lived, chip-filling launch of a decode step - the cross-attention K/V stream - keeps ONE workgroup per CU resident instead of four, so
 * that the latency-sized launches of the other contexts find wave slots (4 contexts x 128 rows: 143 -> 148 images/s; a call alone: 107 -> 103,
 * hence off by default).  Same kernels, same results.  Takes effect from the context's next call (its captured decode step is dropped).
 * Returns the previous setting.  No counterpart in the reference (one batch at a time, utils_evaluation.py:269-285). */
int mg_set_shared_gpu(mg_model* m, int shared);
/* Cross-attention of the greedy decode step (num_beams = 1, batch and queue forms).  Weight-absorbed form: with K_l = enc·Wk_l^T,
 * V_l = enc·Wv_l^T (stock transformers models/udop/modeling_udop.py:524-550, reached from
 * /root/reference/markushgrapher/utils/ocsr/utils_evaluation.py:278-281) softmax(q_h K_h^T) V_h = [softmax((q_h·Wk_h) enc^T) enc]·Wv_h^T, so
 * every layer streams the attended encoder states (2·d_model bytes per position) instead of its own K and V (4·d_model): half the
 * dominant HBM stream of decoding, no cross-K/V projections after the encoder, no per-layer K/V buffers (the workspace shrinks; sizes are
 * computed for the current setting and call shape).  The stream runs one workgroup per decode row: it pays from ~100 rows per call on
 * (160 rows, 4 contexts in flight: 148 -> 197 images/s) and loses below (32 rows alone: 82 -> 50 images/s, latency-bound).
 *   absorb = 2 (default wherever the geometry has the form: d_model a supported multiple of 64, at most 16 heads): by the call's decode
 *              rows - absorbed from 96 rows on, K / V form below;
 *   absorb = 1: absorbed for every greedy call;   absorb = 0: the K / V form for every greedy call;
 *   absorb < 0: query only.
 * key_splits in 1..4: workgroups per decode row of the stream (0 keeps the setting).  The two forms round at different points (q' = q·Wk_h
 * and the normalised context are rounded to bf16 instead of K and V): logits agree within the stated tolerance, NOT bitwise - with
 * absorb = 2 a row decoded in a 160-row call and the same row in a 32-row call go through different forms; pin 0 or 1 where ids must be
 * reproducible across call sizes (markushgrapher_amd/inflight.py does, for the calls it packs).  Takes effect from the context's next
 * call.  Returns the previous `absorb`. */
int mg_set_cross_absorb(mg_model* m, int absorb, int key_splits);
/* Cross-attention of beam search (num_beams > 1: mg_generate and mg_generate_stream_beam, with or without the attached OCSR branch),
 * independent of the greedy setting above.  absorb = 0 (default): the K / V form;  absorb = 1: the weight-absorbed form, in which one
 * workgroup serves two (or three) beams of an image and every stage of the image's states is read once for all of them;  absorb < 0: query
 * only.  key_splits in 1..4: workgroups per (image, beam subset) along the keys (0 keeps the setting; default 2).  Same rounding points and
 * tolerance as the greedy absorbed form; a row's values do not depend on its sibling beams or batch mates.  The workspace sizes follow the
 * setting (mg_workspace_bytes / mg_stream_beam_workspace_bytes).  Takes effect from the context's next call (its captured decode step and
 * queue step are dropped); mg_clone copies it.  Returns the previous `absorb`; MG_E_UNSUPPORTED where the geometry has no absorbed form,
 * MG_E_ARG for bad values. */
int mg_set_beam_cross_absorb(mg_model* m, int absorb, int key_splits);
/* 1 if the last mg_generate replayed a captured graph, 0 if it launched eagerly (mode 0/2, capture unavailable). */
int mg_decode_graph_active(const mg_model* m);

/* The multi-GPU path's one collective behind the C ABI (image shards are independent, the ranks exchange decoded ids):
 * an RCCL all-gather of equal-sized byte blocks on a stream the caller names.  The library resolves librccl at run time (the copy the
 * process already holds, else the system's) and adds no link dependency.  Rendezvous stays with the host: rank 0 calls
 * mg_dist_unique_id and ships the 128 bytes to every rank by whatever it has (markushgrapher_amd/dist.py: torch.distributed's
 * store / broadcast), then EVERY rank calls mg_dist_create (collective).  mg_dist_allgather enqueues ncclAllGather(send, recv) of
 * bytes_per_rank bytes per rank (recv holds world x bytes_per_rank, rank order) and returns; the buffers must stay valid until the
 * stream has passed it.  No counterpart in the reference (one device, /root/reference/markushgrapher/utils/ocsr/utils_evaluation.py:140). */
typedef struct mg_dist mg_dist;
int mg_dist_unique_id(void* out, int bytes);
int mg_dist_create(const void* unique_id, int bytes, int rank, int world, mg_dist** out);
int mg_dist_allgather(mg_dist* d, void* stream, const void* send, void* recv, size_t bytes_per_rank);
void mg_dist_destroy(mg_dist* d);

/* Page preprocessing on the device ("next" row f-3): replaces page_image.resize((512,512), Image.LANCZOS)
 * (/root/reference/markushgrapher/core/datasets/mdu_dataset.py:118) + MarkushgrapherImageProcessor's rescale 1/255 and
 * mean = std = 0.5 normalisation (/root/reference/markushgrapher/core/common/begin.py:105-109), bit-exactly (Pillow's
 * 8-bit fixed-point resampler).  pages_u8 [B][Hs][Ws][3] (RGB, HWC) -> pixel_values [B][3][out][out] f32.
 * scratch: mg_preprocess_scratch_bytes() of device memory. */
size_t mg_preprocess_scratch_bytes(int B, int Hs, int Ws, int out_size);
int mg_preprocess_pages(void* stream, const uint8_t* pages_u8, int B, int Hs, int Ws, int out_size, float* pixel_values,
                        void* scratch, size_t scratch_bytes);

/* Device self-test of the hardware assumptions the kernels rely on (MFMA fragment layout, global_load_lds
 * destination rule, cross-half shuffle). Synchronises. msg_host receives a short report. */
int mg_selftest(void* stream, void* scratch_256k, char* msg_host, int msg_len);

/* ---- kernel-level operator entry points (used by the parity tests) ---- */
int mgk_pack_weight(void* stream, const void* src, int src_is_bf16, int N, int K, void* dst_pk, int Npad);
int mgk_rmsnorm_pack(void* stream, const float* h, const float* gain, void* x_pk, float* out_f32, int M, int d,
                     float eps, float scale);
int mgk_im2col_pack(void* stream, const float* pix, void* x_pk, int B, int C, int I, int ps);
/* TEST / A-B SWITCHES (mgk_set_rows_split, mgk_set_resid_f16, mgk_gemm_set_variant, mgk_set_rows_mt, mgk_set_attention_qt, mgk_set_pp_parts, mgk_set_pp_groups): PROCESS-WIDE, for the parity tests and tools/.
 * Each selects among kernels whose results are bit-identical (that is what the tests that flip them check), so a call that races
 * with a flip still returns the right bits; they are nevertheless meant to be set while no call is running, and the product
 * (markushgrapher_amd/) never touches them.
 * row-tile split policy of the decode-step projections with more than 32 live rows: -1 default (by weight size), 0 never,
 * 1 always one row tile per workgroup */
int mgk_set_rows_split(int mode);
/* residual projections of the decode step with several row tiles: 1 (default) 16 features per workgroup, 0: 8 */
int mgk_set_resid_f16(int on);
/* Half-tile decode projections with three or more 32-row tiles of live rows: 1 = a workgroup takes both 16-feature halves of a weight tile
 * (half the activation re-reads through L2), 0 = one half per workgroup, -1 (default) = as the caller asks (the engine asks for it on
 * contexts that share the GPU, mg_set_shared_gpu).  Same bits either way. */
int mgk_set_rows_ft2(int mode);
/* projections of the decode step with several row tiles: 1 the K-slab form (K chunks as workgroups, partial sums merged by the last
 * arrival in the one-workgroup forms' order) where the caller provides its scratch, 2 the same in two launches (partial sums, then a
 * chip-wide merge launch), 0 (default: measured faster) the one-workgroup forms */
int mgk_set_rows_mt(int on);
/* encoder attention: 1 (default) one 32-query tile per wave / 8 waves per workgroup, 2 two tiles per wave / 4 waves (same bits, slower) */
int mgk_set_attention_qt(int qt);
/* persistent ping-pong GEMM: the row tiles of one problem over several launches - 0 (default) never (problems with more tiles per workgroup
 * than the kernel's table holds go to the two-stage kernel: measured equally fast), 1 when needed, 2 .. 8 always that many (same bits) */
int mgk_set_pp_parts(int mode);
/* persistent ping-pong GEMM: at most that many workgroups per launch - 0 (default) no cap (one per CU), n > 0: min(tiles, CUs, n), rounded down
 * to a multiple of 8 from 8 on as ever; < 0: back to MG_PP_GROUPS or the default.  The kernel takes its tile schedule from its grid, so a small
 * cap makes every workgroup walk several tiles of a small problem (same bits) */
int mgk_set_pp_groups(int cap);
/* mgk_gemm_resid with the scratch of the K-slab form: kpart [16][M padded to 32][N] fp32, ticket [N / 32] i32 zero-initialised;
 * wide_tiles as ResidArgs (8 in the decode steps) */
int mgk_gemm_resid_mt(void* stream, const void* X_pk, const void* W_pk, float* h, const float* gain, float gscale, void* x_pk,
                      float* part, int M, int N, int K, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps, int wide_tiles,
                      float* kpart, int* ticket);
/* epi: 0 fp32 store (+ bias), 1 fp32 accumulate, 2 / 3 packed relu / packed, 7 packed gelu(tanh) (large-M tile kernels only), and
 * (mode 0 only, N % 16 == 0) 8 packed bf16(acc + bias[n]), 9 packed bf16(gelu_erf(acc + bias[n])); bias nullable */
int mgk_gemm(void* stream, int mode, int epi, const void* X_pk, const void* W_pk, int M, int N, int K, float* out_f32,
             int ldo, const float* bias, void* out_pk);
/* Deferred-RMSNorm pair of the encoder (tiled large-M kernels): epi 5 (EPI_RESID_NORM): h_tiled (fp32, tiles of
 * [32 rows][4 features]: index ((m/32)*(N/4) + n/4)*128 + (m%32)*4 + n%4) += X W^T, out_pk = pack(bf16(h * gain)) un-normalised,
 * part[M][part_ld] = per-64-column partial sums of h^2; epi 3 / 2 (packed / packed relu): rows scaled by
 * rsqrt(sum(rs_part[m][0..rs_nparts)) * rs_inv_d + rs_eps) (rs_part NULL: no scale).  M is a multiple of 32, except for epi 5 with gain,
 * out_pk, part and rs_part all NULL (the plain tiled residual update of the Swin branch: rows >= M are not written). */
int mgk_gemm_norm(void* stream, int epi, const void* X_pk, const void* W_pk, int M, int N, int K, float* h_tiled, const float* gain,
                  void* out_pk, float* part, int part_ld, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps);
/* mgk_gemm / mgk_gemm_norm restricted to the 32-row tiles that hold a non-zero entry of row_mask [M] (the encoder's row-tile list:
 * whole tiles of padded text slots / dropped patch slots are neither read nor written).  list_scratch: M/32 + 1 ints. */
int mgk_gemm_row_tiles(void* stream, int epi, const void* X_pk, const void* W_pk, int M, int N, int K, float* out_f32, const float* gain,
                       void* out_pk, float* part, int part_ld, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps,
                       const uint8_t* row_mask, int* list_scratch);
int mgk_gemm_heads(void* stream, int mode, const void* X_pk, const void* W_pk, int M, int N, int K, void* p0, void* p1,
                   void* p2, int f0, int f1, int f2, int H, int S_in, int S_cap, const int* row_map, int pos);
/* The tiled large-M GEMM (mode 0 of the entries above) with everything its call sites in the engines set, on operands the caller makes (test
 * entry).  mgk_gemm_desc = GemmArgs: X packed [M padded to 32][K], W packed [N padded to 32][K]; by epilogue
 *   0 / 1 (fp32 store + bias / accumulate): out_f32 [M][ldo], ldo >= N;
 *   2 / 3 (packed relu / packed): out_pk packed [M][N], N % 16 == 0, rows scaled by the deferred RMSNorm scale rs_*;
 *   5 (EPI_RESID_NORM): out_f32 = the tiled h (mgk_gemm_norm), N % 32 == 0; gain -> out_pk = pack(bf16(h * gain)); part [M][ldo] partial sums of
 *     h^2 (ldo >= N / 64 rounded up); M % 32 == 0 when any of gain / out_pk / part is given;
 *   4 (per head): N = 1 .. 3 regions of H * 64 columns, region i to head_ptr[i] in head_fmt[i] = 0 none (pointer may be null), 1 packed rows,
 *     2 packed transposed ([B][H][S_cap] tokens, token s of image m / S_in at s + s_off: s_off + S_in <= S_cap, S_in, S_cap, s_off multiples
 *     of 32), 3 natural [B][H][S_cap][64] at row row_map[m] (null: m % S_in; < 0: dropped; s_off must be 0); rows scaled by rs_*.
 * rs_part [M][rs_nparts] (null: no scale; epilogues 2, 3, 4 only), rs_nparts a multiple of 4.
 * row_mask [M] + list_scratch [M / 32 + 1] (M % 32 == 0, row_mask 16-byte aligned): the row-tile list is built from the mask as in
 * mgk_gemm_row_tiles (a mask without an attended position gives the list {0}).  list_scratch alone: the caller's own list - [0] the count,
 * then that many ascending tile ids < M / 32 - the only way to an empty one.  The 128 x 128 and 256 x 128 kernels (variants 0 / 1, M < 320,
 * N < 256) have no list support and compute every row.
 * Errors before any device work: MG_E_ARG a missing pointer, MG_E_SHAPE a size rule above, MG_E_UNSUPPORTED any other epilogue or format
 * (the bias / GELU epilogues: mgk_gemm; the decode-step formats: mgk_gemm_heads_step) and a row scale on an epilogue that applies none. */
typedef struct mgk_gemm_desc {
    const void* X;
    const void* W;
    int M, N, K;
    float* out_f32; int ldo;
    const float* bias;
    void* out_pk;
    const float* gain;
    float* part;
    const float* rs_part; int rs_nparts; float rs_inv_d, rs_eps;
    void* head_ptr[3]; int head_fmt[3];
    int H, S_in, S_cap, s_off;
    const int* row_map;
    const uint8_t* row_mask; int* list_scratch;
} mgk_gemm_desc;
int mgk_gemm_ex(void* stream, const mgk_gemm_desc* d, int epi);
/* mode 0 (encoder): tab1/tabh/tabv are the RAW bucket tables [32][H]; bk1[257] / bkhv[201] the bucket ids of integer
 * distances -128..128 / -100..100; bidx_scratch [B][Sk_cap/32][Sk_cap][32] u16 receives the per-pair bucket indices.
 * mode 1 (decoder self): tab1 = [tab1_len][H] by distance; mode 2 (cross): no bias. */
int mgk_attention(void* stream, int mode, const void* Q, const void* K, const void* Vt, void* ctx_pk, int B, int H,
                  int Sq, int Sk, int Sq_cap, int Sk_cap, const uint8_t* kmask, const float* tab1, int tab1_len,
                  const float* tabh, const float* tabv, const double* cx, const double* cy, const int* bk1, const int* bkhv,
                  void* bidx_scratch);
/* One layer's launch of the attribution kernel (csrc/k_attrib.hip), then - map non-null - the gather into map [B][Sq][M_e1 + L + P].
 * Q [B][H][Sq_cap][64], K [B][H][Sk_cap][64] as mgk_attention's (HF_PK_ROWS); keys per image Sk = M_pad + L + P <= min(Sk_cap, 1536):
 * [e1 slots (M_pad, a multiple of 64, the first M_e1 real) | workspace rows of the encoder]; kmask [B][Sk_cap] (nullable).  The head-summed
 * fp32 softmax is stored to scratch (accumulate = 0) or added to it (1), times `scale`.  Column M_e1 + s of the map is encoder output
 * position s in [text L | patches P] order (text_len [B] nullable: image b's workspace rows are [text text_len[b] | patches | text padding]);
 * rows with qmask[b][q] == 0 (qmask [B][Sq], nullable) are 0.0.  scratch: mgk_xattn_map_scratch_bytes(B, Sq, Sk), MG_E_WORKSPACE if smaller. */
size_t mgk_xattn_map_scratch_bytes(int B, int Sq, int Sk);
int mgk_xattn_map(void* stream, const void* Q, const void* K, int B, int H, int Sq, int Sq_cap, int Sk_cap, const uint8_t* kmask, int accumulate,
                  float scale, void* scratch, size_t scratch_bytes, int M_e1, int M_pad, int L, int P, const int* text_len, const uint8_t* qmask,
                  float* map);
/* mgk_attention(mode 0) with the skip lists mg_encode uses: 64-key stages / 128-query blocks without an attended position
 * are not visited (kst_scratch: B*(1+S_cap/64) ints, qbv_scratch: B*ceil(S_cap/128) bytes). */
int mgk_attention_enc_skip(void* stream, const void* Q, const void* K, const void* Vt, void* ctx_pk, int B, int H, int S, int S_cap,
                           const uint8_t* kmask, const float* tab1, const float* tabh, const float* tabv, const double* cx,
                           const double* cy, const int* bk1, const int* bkhv, void* bidx_scratch, int* kst_scratch,
                           uint8_t* qbv_scratch);
int mgk_attention_step(void* stream, const void* q, const void* Kc, const void* Vc, void* ctx_pk, int rows, int H,
                       int group, int cap, const int* len, int n_keys, const float* bias, const int* anc, int t);
/* mgk_attention_step plus what the engine sets on a decode step: position from device memory (t_dev + t_off) or per row (pos_rows + t_off),
 * kv_owner (per row for group 1, per group of rows otherwise; indexes len too), live (rows / groups with 0 are not computed or written),
 * the deferred RMSNorm scale of the query rows as partial sums qrs_part [rows][qrs_nparts] (r = rsqrt(sum * qrs_inv_d + qrs_eps), null: 1),
 * ctx_pk as columns [ctx_col0, ctx_col0 + H*64) of a packed buffer ctx_ld wide (0: H*64), one_wg_per_cu (cross form, group 1). */
int mgk_attention_step_ex(void* stream, const void* q, const void* Kc, const void* Vc, void* ctx_pk, int rows, int H, int group, int cap,
                          const int* len, int n_keys, const float* bias, const int* anc, int t, const int* t_dev, int t_off,
                          const int* pos_rows, const int* kv_owner, const int* live, const float* qrs_part, int qrs_nparts, float qrs_inv_d,
                          float qrs_eps, int ctx_ld, int ctx_col0, int one_wg_per_cu);
/* The rotary grouped-query form of the step (ChemicalOCR text model): qkv fp32 [rows][ld] = [H_kv*group q | H_kv k | H_kv v] x 64, rotated
 * by cs [positions][cos 32 | sin 32] at the row's position, scaled by the deferred RMSNorm scale rs_* (q also by qscale), rounded to bf16;
 * k, v appended to Kc / Vc [pages][H_kv][cap][64] at the position, attention over [0, position].  group in {1, 2, 3, 4, 6, 8}
 * (MG_E_SHAPE otherwise).  Position: pos_rows / t_dev / t as above, plus t_off_rows[page]; page = kv_owner ? kv_owner[row] : row. */
int mgk_attention_step_rope(void* stream, const float* qkv, int ld, const float* cs, const float* rs_part, int rs_nparts, float rs_inv_d,
                            float rs_eps, float qscale, void* Kc, void* Vc, void* ctx_pk, int rows, int H_kv, int group, int cap, int t,
                            const int* t_dev, int t_off, const int* pos_rows, const int* t_off_rows, const int* kv_owner, const int* live,
                            int ctx_ld, int ctx_col0);
/* Weight-absorbed cross-attention of one decoder layer and step (mg_set_cross_absorb; kernels of markushgrapher_amd/csrc/k_xattn.hip):
 * ctx[row][h] = softmax(q_h (enc Wk_h^T)^T) (enc Wv_h^T) (stock modeling_udop.py:524-575 without a position bias) evaluated as
 * [softmax((q_h Wk_h) enc^T) enc] Wv_h^T on the states themselves.  q [rows][H][64] bf16; wkv fp32 [2*H*64][d], K rows first;
 * enc [owners][cap][d] bf16; len [owners] keys per owner; kv_owner [rows] (null: row r reads owner r); scratch wk, wv (H*d*64 bf16
 * each), qx (rows*H*d bf16), part (rows*nsplit*H*d bf16), ml (rows*nsplit*H*2 fp32); ctx_pk packed [rows padded to 32][H*64]. */
int mgk_xattn(void* stream, const void* q, const float* wkv, const void* enc, const int* len, const int* kv_owner, int rows, int H, int d,
              int cap, int nsplit, int nstg, void* wk, void* wv, void* qx, void* part, float* ml, void* ctx_pk);
/* The same for beam search (mg_set_beam_cross_absorb): rows = owners' images x group beams, row r attends owner
 * kv_owner ? kv_owner[r / group] : r / group (kv_owner indexed by image); live [rows] nullable (rows with live == 0 are not written);
 * beams_per_wg: beams of an image per workgroup (2, or 3 with nstg = 3 up to d = 768; 0 = the engine's choice); nt: 1 = the stream's
 * copies carry the non-temporal hint (the engine's default), 0 = default cache policy. */
int mgk_xattn_beams(void* stream, const void* q, const float* wkv, const void* enc, const int* len, const int* kv_owner, const int* live,
                    int rows, int H, int d, int cap, int group, int nsplit, int nstg, int beams_per_wg, int nt, void* wk, void* wv, void* qx,
                    void* part, float* ml, void* ctx_pk);
int mgk_enc_rows(void* stream, const void* src_pk, const int* row_map, void* dst, int B, int rows_per_image, int cap, int d);
int mgk_embed_assemble(void* stream, void* meta_ws, const int64_t* input_ids, const float* bbox,
                       const uint8_t* attention_mask, const float* patch_emb, const void* tok_emb, const void* x_emb,
                       const void* y_emb, int B, int L, int P, int d, int n_side, int M2, int V, int S_cap,
                       float* hidden, double* cx, double* cy, uint8_t* mask, int* xrow, int* xlen, int* err);
size_t mgk_embed_meta_bytes(int B, int S_cap);
/* The stage in front of the first encoder GEMM and behind the last one, in every form mg_encode runs it (test entries; kernels of
 * csrc/k_embed.hip, k_attn.hip, k_pack.hip, k_xattn.hip and the output copies of engine.hip).  Every entry checks its arguments before any
 * device work: MG_E_ARG a missing pointer, MG_E_SHAPE a size rule.
 * mgk_embed_desc = EmbedArgs (csrc/mg_kernels.h) + meta_ws (mgk_embed_meta_bytes(B, S_cap) bytes): hidden [B][S_cap][d] fp32 row-major, or
 * the tiled layout of mgk_gemm_norm's h_tiled when hidden_tiled (S_cap % 32 == 0); cx / cy [B][S_cap] f64; mask [B][S_cap]; xrow [B][S_cap] =
 * x_row0 + rank among the attended positions, or -1; xlen [B] = x_row0 + attended positions; trim_padding = 1 with an attention mask: the
 * layout [text Lb | patches | moved text padding], Lb = last attended text token + 1; text_len [B] nullable receives Lb (L otherwise).
 * Rules: S_cap >= L + P, P == n_side * n_side, d % 4 == 0, x_row0 >= 0. */
typedef struct mgk_embed_desc {
    const int64_t* input_ids; const float* bbox; const uint8_t* attention_mask; const float* patch_emb;
    const void* tok_emb; const void* x_emb; const void* y_emb;
    int B, L, P, d, n_side, M2, V, S_cap;
    float* hidden; int hidden_tiled;
    double* cx; double* cy; uint8_t* mask; int* xrow; int* xlen; int x_row0;
    int trim_padding; int* text_len; int* err;
    void* meta_ws;
} mgk_embed_desc;
int mgk_embed_assemble_ex(void* stream, const mgk_embed_desc* e);
/* bias_index: out [B][S_cap/32][S_cap][32] u16 = byte address 4 * (32 * vertical bucket + horizontal bucket) of every (query, key) pair, keys
 * of a tile in accumulator order (entry half*16 + r <-> key (r%4) + 8*(r/4) + 4*half), 4 * 1024 for keys >= Sk or with kmask 0 (kmask
 * [B][S_cap] nullable); bkhv [201] buckets of the distances -100 .. 100; bk1 is not read.  S_cap % 64 == 0, Sk <= S_cap. */
int mgk_bias_index(void* stream, void* out, const double* cx, const double* cy, const uint8_t* kmask, const int* bk1, const int* bkhv, int B,
                   int Sk, int S_cap);
/* attn_lists: kst [B][1 + S_cap/64] = count, ascending ids of the 64-key stages with an attended key < Sk ({1, 0} when there is none);
 * qbv [B][ceil(S_cap/128)] = 1 for a 128-query block with one.  S_cap % 64 == 0, Sk <= S_cap. */
int mgk_attn_lists(void* stream, const uint8_t* kmask, int B, int Sk, int S_cap, int* kst, uint8_t* qbv);
/* row_tile_list: list = ascending ids of the 32-row tiles of kmask [rows] with a non-zero byte, *count their number ({0}, 1 when there is
 * none); entries behind the count are not written.  rows % 32 == 0, kmask 16-byte aligned. */
int mgk_row_tile_list(void* stream, const uint8_t* kmask, int rows, int* list, int* count);
/* pack_e1: e1 [B][M][d] fp32 -> e1_pk packed bf16 [B * M_pad][d] (rows >= M zero), row_map [B * M_pad] = j < M ? j : -1 and, when xmask is
 * given, xmask [B][M_pad + S_cap] = [1 x M | 0 | enc_mask [B][S_cap]].  M_pad % 32 == 0, M_pad >= M, d % 16 == 0, S_cap % 64 == 0. */
int mgk_pack_e1(void* stream, const float* e1, int B, int M, int M_pad, int d, void* e1_pk, int* row_map, const uint8_t* enc_mask, int S_cap,
                uint8_t* xmask);
/* The two output copies of mg_encode: enc_out [B][S][d] / enc_mask [B][S] in the order [text L | patches S - L] from the workspace rows
 * enc_f32 [B][S_cap][d] / mask [B][S_cap]; text_len [B] (nullable) = text lengths Lb of the layout [text Lb | patches | text padding L - Lb].
 * Either output may be null.  L <= S <= S_cap, d % 4 == 0. */
int mgk_enc_copy_out(void* stream, const float* enc_f32, const uint8_t* mask, float* enc_out, uint8_t* enc_mask, int B, int S, int S_cap, int d,
                     int L, const int* text_len);
/* embed_rows: h [rows][d] fp32 = tok_emb [V][d] bf16 rows of ids (an id outside [0, V) is counted in *err and reads row 0); x_pk (nullable):
 * the same rows into columns [x_col0, x_col0 + d) of a packed bf16 buffer x_ld wide.  d % 4 == 0, x_ld % 16 == 0, x_col0 % 4 == 0. */
int mgk_embed_rows(void* stream, const int64_t* ids, const void* tok_emb, float* h, int rows, int d, int V, int* err, void* x_pk, int x_ld,
                   int x_col0);
/* rmsnorm_pack_rows: packed row dst_row[m] of x_pk = bf16(RMSNorm(h[m]) * gain * scale); dst_row[m] < 0: row m is skipped; dst_row null: m.
 * d % 16 == 0. */
int mgk_rmsnorm_pack_rows(void* stream, const float* h, const float* gain, void* x_pk, const int* dst_row, int M, int d, float eps, float scale);
int mgk_greedy_select(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len,
                      int64_t* next_ids, int64_t* out_ids, int max_len, int pos, int* unfinished, int* n_unfinished,
                      float* top2);

/* Sampled selection of one decode step (csrc/k_sample.hip), the kernel mg_generate_sampled launches: for every row with unfinished != 0
 * MinLength (EOS removed while pos < min_len), temperature, top-k (0 = off), top-p (>= 1 = off) and one Philox4x32-10 draw at counter
 * (stream id, pos); finished rows emit pad.  logits [rows][ldl] fp32, ldl a multiple of 4 >= V, V <= 36 864 (MG_E_UNSUPPORTED beyond);
 * stream_ids [rows] u64 device, nullable (the row index); token_scores [rows][ts_ld] nullable, column pos - 1 written. */
int mgk_sample_select(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                      int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids, int max_len,
                      int pos, int* unfinished, int* n_unfinished, float* token_scores, int ts_ld);
/* The generator itself, on the host: out_host[4] = Philox4x32-10 with key = seed and counter = (stream_id lo, stream_id hi, pos, 0).
 * The draw uses r = out[1] << 32 | out[0]. */
int mgk_philox(uint64_t seed, uint64_t stream_id, uint32_t pos, uint32_t* out_host);
/* The selection step of a decode loop in every form the loops launch it in (test entries).  mgk_slot_table = SlotTable (csrc/mg_kernels.h):
 * pos / img / pool [slots] i32, ctr [16] i32 ([0] live slots, [1] sequences done, [2] steps, [4] queue head, [5] images ready, [7] oldest
 * live sequence), out_len [sequences of the queue]; first_tok [sequences] i64, nullable; stop[0 .. n_stop) the stop tokens slot_refill tests
 * first_tok against; nsamp sequences per image.  pos null = no slot table (batch form).
 * mgk_select_desc = ArgmaxArgs: fused = 0 greedy_select on logits [rows][ldl] (ldl a multiple of 4 >= V; batch form, or the queue form with
 * slots.pos given, which needs img / ctr / out_len too); fused = 1 greedy_select_fused on the lm_head partials ptop [rows][ntiles] float4 /
 * stopv [rows][4] (mgk_lm_head_step), which also writes h [rows][d] fp32, x_pk packed [rows padded to 32][d] and, if given, the window
 * [x2_col0, x2_col0 + d) of x2_pk (x2_ld columns); d <= 2048, a multiple of 16; batch form only.  eos_more[0 .. n_eos_more) are further stop
 * tokens; top2 [rows][2], or [max_len][rows][2] with pos_dev; step_ctr [8] i32 ([0] unfinished rows, [1] first all-finished step, [2] steps,
 * [6] arrivals); token_scores [rows][ts_ld].  n_unfinished is NOT cleared by the call: the caller sets it (the step_ctr path clears it).
 * 1 <= rows <= 256. */
typedef struct mgk_slot_table {
    int* pos; int* img; int* pool; int* ctr; int* out_len;
    int pool_cap, start_id;
    const int64_t* first_tok;
    int n_stop, stop[4], max_len, nsamp;
} mgk_slot_table;
typedef struct mgk_select_desc {
    int fused;
    const float* logits; int rows, V, ldl;
    int eos, pad, suppress_eos, n_eos_more, eos_more[3];
    int64_t* next_ids; int64_t* out_ids; int max_len, pos;
    const int* pos_dev;
    int min_len;
    int* unfinished; int* n_unfinished;
    float* top2;
    int* step_ctr;
    mgk_slot_table slots;
    const void* ptop; const float* stopv; int ntiles;
    const void* tok_emb; float* h; const float* gain; void* x_pk; void* x2_pk; int x2_ld, x2_col0, d; float eps;
    float* token_scores; int ts_ld;
} mgk_select_desc;
int mgk_select_ex(void* stream, const mgk_select_desc* s);
/* mgk_sample_select in the queue form (SampleArgs::slots): row = slot, column slots.pos[row] + 1 of sequence slots.img[row]; stream_ids and
 * token_scores are indexed by the sequence.  Arguments and checks of mgk_sample_select (`pos` and n_unfinished are not used by this form;
 * n_unfinished is not cleared) plus the slot table, whose pos / img / ctr / out_len are required. */
int mgk_sample_select_queue(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                            int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids, int max_len,
                            int pos, int* unfinished, int* n_unfinished, float* token_scores, int ts_ld, const mgk_slot_table* slots);
/* The selection step under a decoder prompt (mg_generate_prompted; DecPrompt in csrc/mg_kernels.h), batch forms only (a slot table with a
 * prompt: MG_E_ARG).  prompt_ids [owners][prompt_ld] i64 and prompt_len [owners] i32, both device; row r takes the prompt of owner
 * r / group (group 0 / 1: its own); *bad (nullable) counts prompt ids outside [0, V), which are replaced by id 0.  While the column written
 * is below the row's prompt length the row emits the prompt's token, scores 0.0, draws nothing and stays unfinished; the unfinished count
 * and the step counters see it as a live row.  mgk_select_prompted = mgk_select_ex (fused or not); mgk_sample_select_prompted =
 * mgk_sample_select with pos_dev / step_ctr as the engine's launch has them (nullable) - neither clears n_unfinished. */
int mgk_select_prompted(void* stream, const mgk_select_desc* s, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld, int group,
                        int* bad);
int mgk_sample_select_prompted(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                               int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids, int max_len,
                               int pos, const int* pos_dev, int* unfinished, int* n_unfinished, int* step_ctr, float* token_scores, int ts_ld,
                               const int64_t* prompt_ids, const int* prompt_len, int prompt_ld, int group, int* bad);
/* slot_refill (csrc/k_decode.hip) after a selection: idle slots take the next ready sequences of the queue.  1 <= rows <= 256, nsamp >= 1,
 * pool_cap >= 1. */
int mgk_slot_refill(void* stream, const mgk_slot_table* slots, int64_t* next_ids, int* unfinished, int rows);

/* ---- kernels of the OCSR vision branch "e1" (csrc/k_swin.hip; test entries, not on the product path) ---- */
/* (Shifted-)window attention of one Swin block, head dim 32.  qkv_pk packed bf16 [B*R*R padded to 32][3C] = [q | k | v] in the natural token
 * order m = (b, y, x) of the R x R map; ctx_pk packed bf16 [B*R*R padded to 32][C] (padding rows are not written); table_HT fp32
 * [H][(2w-1)^2], entry (dy + w - 1) * (2w - 1) + dx + w - 1 for query - key offsets.  w in {4, 8, 12}, R % w == 0, C == 32 H, H < 4 or
 * H % 4 == 0 (MG_E_UNSUPPORTED otherwise); 0 <= shift < w. */
int mgk_swin_attention(void* stream, const void* qkv_pk, void* ctx_pk, const float* table_HT, int B, int R, int C, int H, int w, int shift);
/* LayerNorm of M rows of C features (biased variance, eps inside the root).  h_in fp32: TILED (in_tiled = 1: tiles of [32 rows][4 features],
 * the layout of mgk_gemm_norm's h_tiled) or row-major [M][C]; merge_R > 0 (even): h_in is the TILED [B*merge_R^2][C/4] map and row (b, i, j)
 * of the (merge_R/2)^2 map is [h(2i,2j) | h(2i+1,2j) | h(2i,2j+1) | h(2i+1,2j+1)].  Outputs, each nullable: x_pk packed bf16 [M padded to
 * 32][kaug ? kaug : C] (kaug > C: column C = 1, the following ones 0); out_f32 row-major [M][C]; h_out TILED [M][C] = the row itself
 * (h_out_norm = 0) or its normalised form (1), + add_bias [C] (nullable); h_out may be h_in when that is tiled.  C in {64, 128, 256, 512,
 * 768, 1024, 2048, 4096} (MG_E_UNSUPPORTED otherwise); kaug 0 or a multiple of 16 >= C. */
int mgk_swin_layernorm(void* stream, const float* h_in, int in_tiled, float* h_out, int h_out_norm, const float* w, const float* b,
                       const float* add_bias, void* x_pk, float* out_f32, int M, int C, int merge_R, float eps, int kaug);
/* dst fp32 [B][C][I][I] = bilinear resize (align_corners = false, no antialias) of src fp32 [B][C][S][S], then * scale[c] + shift[c];
 * scale_host / shift_host: C floats in HOST memory (they travel as kernel arguments).  C <= 4. */
int mgk_swin_resize(void* stream, const float* src, float* dst, int B, int C, int S, int I, const float* scale_host, const float* shift_host);
/* pix fp32 [B][C][I][I] -> x_pk packed bf16 [B*(I/ps)^2 padded to 32][Kp], column k = (c*ps + dy)*ps + dx, zero from C*ps*ps on and in the
 * padding rows.  Kp a multiple of 16 >= C*ps*ps. */
int mgk_swin_im2col_pack(void* stream, const float* pix, void* x_pk, int B, int C, int I, int ps, int Kp);
/* src fp32 [n][H] -> dst fp32 [H][n] */
int mgk_swin_transpose(void* stream, const float* src, float* dst, int n, int H);

/* ---- kernels of the ChemicalOCR stage (csrc/k_ocr.hip and the decode-step kernels it starts from; test entries, not on the product path) ----
 * "packed" = the bf16 fragment-tile format of mgk_gemm's operands, rows padded to 32 (rows >= M are not written unless stated); "tiled" = the
 * fp32 layout of mgk_gemm_norm's h_tiled.  Each entry returns MG_E_SHAPE / MG_E_UNSUPPORTED for what its launcher assumes without checking.
 * x_pk packed [M][Kaug] = bf16(LayerNorm(h[m]) * w + b) | 1 at column d | 0 (Kaug a multiple of 16 >= d); out_f32 [M][d] row-major the same
 * unrounded; h [M][d] row-major += add_bias afterwards.  x_pk, out_f32, add_bias each nullable. */
int mgk_ocr_layernorm_pack(void* stream, float* h, const float* w, const float* b, const float* add_bias, void* x_pk, float* out_f32, int M,
                           int d, int Kaug, float eps);
/* y_pk packed [M][Kaug] = bf16(gelu_tanh(in [M][N])) | 1 at column N | 0 */
int mgk_ocr_gelu_pack(void* stream, const float* in, void* y_pk, int M, int N, int Kaug);
/* y_pk packed [M][I] = bf16(silu(in[m][2c]) * in[m][2c + 1]), in [M][2I] gate / up interleaved; _rows: gate and up first multiplied by the row's
 * deferred RMSNorm scale r = rsqrt(sum(rs_part[m][0..rs_nparts)) * rs_inv_d + rs_eps) (rs_part NULL: 1).  I % 16 == 0. */
int mgk_ocr_silu_mul_pack(void* stream, const float* in, void* y_pk, int M, int I);
int mgk_ocr_silu_mul_rows(void* stream, const float* in, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps, void* y_pk, int M,
                          int I);
/* hidden [N][P_cap][d] = patch [N][P][d] + pos [.][d] (bf16) at row pos_ids [N][P] (NULL: p); rows p >= P zero.  vmask [N][P_cap] (nullable) =
 * patch_mask [N][P] != 0 (NULL: 1), 0 from P on. */
int mgk_ocr_add_pos(void* stream, const float* patch, const void* pos, const int* pos_ids, const uint8_t* patch_mask, uint8_t* vmask,
                    float* hidden, int N, int P, int P_cap, int d);
/* Idefics3Connector.pixel_shuffle: x_pk packed [N*(g/sf)^2][e*sf*sf], token (n, y2, x2), feature (dy*sf + dx)*e + c <- vis [N][P_cap][e] at
 * patch (y2*sf + dy)*g + x2*sf + dx.  g % sf == 0, P_cap >= g*g, e*sf*sf % 16 == 0. */
int mgk_ocr_pixel_shuffle_pack(void* stream, const float* vis, void* x_pk, int N, int g, int P_cap, int e, int sf);
/* inputs_merger: h [B][T_cap][d] = ids [B][L] == image_token ? feats [B][per_seq][d] (the sequence's k-th <image> takes its row k) : tok_emb
 * [V][d] (bf16); rows t >= L zero; feats NULL: token embeddings only.  *err += ids outside [0, V) (they read row 0) + sequences whose <image>
 * count is not per_seq.  L <= 2048 (MG_E_UNSUPPORTED beyond). */
int mgk_ocr_merge_embed(void* stream, const int64_t* ids, const void* tok_emb, const float* feats, float* h, int B, int L, int T_cap, int d,
                        int V, int image_token, int per_seq, int* err);
/* Prefill rotary embedding + head layouts: qkv fp32 [B*T_cap][(H + 2 KV)*64] = [q | k | v]; Q (x 1/8), K rotated at position t = row % T_cap,
 * bf16, as mgk_attention's operands Q, K [B][H][T_cap][64] (HF_PK_ROWS) and Vt (HF_PK_T) with key/value head hh / (H / KV) repeated for every
 * query head hh, rows t >= T zero; and once per key/value head into Kc, Vc [B][KV][cap][64], rows t < T only.  H % KV == 0 (MG_E_UNSUPPORTED
 * otherwise), T <= T_cap, T_cap % 32 == 0, T <= cap. */
int mgk_ocr_rope_heads(void* stream, const float* qkv, int B, int T, int T_cap, int H, int KV, float theta, void* Q, void* K, void* Vt, void* Kc,
                       void* Vc, int cap);
/* cs [positions][cos 32 | sin 32] of angle p * theta^(-i/32): the table mgk_attention_step_rope reads */
int mgk_ocr_rope_table(void* stream, float* cs, int positions, float theta);
/* packed weight rows row0 + r*rstride (r < Nfill) of a [.][Kaug] operand <- W [N][K] * scale | bias[r] * scale at column K | 0; rows r >= N zero */
int mgk_ocr_pack_aug(void* stream, const float* W, const float* bias, float scale, void* dst_pk, int row0, int N, int K, int Kaug, int Nfill,
                     int rstride);
/* row-major fp32 [M][d] -> tiled (to_tiled != 0) or back; M % 32 == 0, d % 4 == 0 */
int mgk_ocr_tile_f32(void* stream, const float* src, float* dst, int M, int d, int to_tiled);
/* [B][T_cap] each: last_rows = b at t == (lens ? lens[b] : T) - 1 else -1; all_rows = b*T + t for t < T else -1; key_mask = t < (lens ? lens[b] : T) */
int mgk_ocr_row_maps(void* stream, int* last_rows, int* all_rows, uint8_t* key_mask, int B, int T, int T_cap, const int* lens);
/* delta[n] = clamp(lens[n], 1, L) - L; *err += lengths outside [1, L] */
int mgk_ocr_len_delta(void* stream, const int* lens, int* delta, int N, int L, int* err);
/* The gate / up projection of the decode step (row-streaming kernels, epilogue 6): W_pk packed [N][K], rows gate_0, up_0, gate_1, ...;
 * out[m][j] = bf16(silu(r acc[m][2j]) * (r acc[m][2j + 1])), r as in mgk_ocr_silu_mul_rows, written as columns [out_col0, out_col0 + N/2) of a
 * packed buffer out_ld wide (out_ld = 0: N/2 wide, N % 32 == 0).  X_pk: k-tiles [x_k0, x_k0 + K/16) of a packed buffer of x_kts k-tiles per
 * row tile (x_kts = 0: K/16).  M <= 256 (MG_E_UNSUPPORTED beyond), N % 16 == 0, K % 64 == 0, out_col0 % 4 == 0,
 * rs_nparts % 8 == 0. */
int mgk_gemm_swiglu(void* stream, const void* X_pk, int x_kts, int x_k0, const void* W_pk, int M, int N, int K, const float* rs_part,
                    int rs_nparts, float rs_inv_d, float rs_eps, void* out_pk, int out_ld, int out_col0);
/* mgk_rmsnorm_pack (scale 1) from the tiled fp32 layout; M % 32 == 0, d % 16 == 0 */
int mgk_rmsnorm_pack_tiled(void* stream, const float* h_tiled, const float* gain, void* x_pk, float* out_f32, int M, int d, float eps);
/* h [rows][d] = tok_emb [V][d] (bf16) at ids[row], x_pk packed [rows][d] = bf16(RMSNorm(h) * gain), x2_pk (nullable) columns [x2_col0,
 * x2_col0 + d) of a packed buffer x2_ld wide = the embedding row itself; an id outside [0, V) adds one to *err and reads row 0 */
int mgk_embed_norm_rows(void* stream, const int64_t* ids, const void* tok_emb, float* h, const float* gain, void* x_pk, void* x2_pk, int x2_ld,
                        int x2_col0, int rows, int d, int V, int* err, float eps);

/* decode-step split-K projection: P[ks][m*ldp + n] partial sums (ks < KS); consumers sum the slabs */
int mgk_gemm_splitk(void* stream, const void* X_pk, const void* W_pk, float* P, int M, int N, int K, int ldp,
                    size_t slab_stride, int KS);
int mgk_splitk_factor(int N, int K);
/* lm_head of the teacher-forced path with the log-softmax / argmax / gather in the epilogue (csrc/k_score.hip; the [M][N] logits are never
 * stored).  X_pk packed [M padded to 32][K], W_pk packed [N padded to 32][K] with zero pad rows, K % 64 == 0.  Per row m over the N real
 * columns: lse = log-sum-exp; tok_lp = logit[targets[m]] - lse (target < 0: 0.0; >= N: 0.0, and the first int of scratch counts it);
 * arg_id = lowest index of the largest logit; arg_lp = its logit - lse.  targets and every output are nullable; rows >= M are not written.
 * scratch: mgk_score_scratch_bytes(M, N) bytes (16 per row and 1024-column slab of the vocabulary), MG_E_WORKSPACE if smaller. */
size_t mgk_score_scratch_bytes(int M, int N);
int mgk_score(void* stream, const void* X_pk, const void* W_pk, int M, int N, int K, const int64_t* targets, float* tok_lp, int64_t* arg_id,
              float* arg_lp, float* lse, void* scratch, size_t scratch_bytes);
/* A/B switch of the large-M GEMM kernel (0: 128x128 two-stage, 1: 256x128 three-stage, default) */
int mgk_gemm_set_variant(int v);
/* decode-step residual projection with the next RMSNorm folded in: h += X W^T (optionally scaled per row by the deferred
 * statistic rs_*), x_pk = bf16(h*gain*gscale) un-normalised, part[m][N/8] = per-block sums of h^2 */
int mgk_gemm_resid(void* stream, const void* X_pk, const void* W_pk, float* h, const float* gain, float gscale, void* x_pk,
                   float* part, int M, int N, int K, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps);
/* Pair projection of the decode step with its product weight (test entry for gemm_rows_pair / the mg_finalize helpers):
 *   W2_pk  <- pack([Wn*diag(gain) | Wn*diag(gain)*Wr])   built on the device from Wn_pk [N2][d], Wr_pk [d][inner]
 *             (scratch_f32: at least N2*(2*d+inner) + d*inner floats);
 *   one launch: h[M][d] += ctx*Wr^T, hb_out_pk = pack(bf16(h_new)), part = per-row partial sums of h_new^2   |
 *               out2_pk = pack(relu?(W2 * [hb ; ctx]))     with xwin_pk = packed [rows][d+inner] = [bf16(h_old) | ctx]. */
int mgk_gemm_pair(void* stream, const void* Wn_pk, const void* Wr_pk, const float* gain, int N2, int d, int inner, void* W2_pk,
                  float* scratch_f32, const void* xwin_pk, float* h, void* hb_out_pk, float* part, void* out2_pk, int M, int relu);
/* The projections of the decode step as decode_step (engine.hip) sets them up, on operands the caller makes (test entries; every launcher of
 * this family takes at most 256 rows = 8 row tiles: MG_E_SHAPE beyond, as for K % 64, N % 32 of a residual projection, a window outside
 * its buffer, a row scale whose partial count is not a multiple of 8).  Packed operands hold their rows padded to 32.
 * mgk_resid_desc = ResidArgs: X a window of k-tiles [x_k0, x_k0 + K / 16) of a packed buffer x_kts k-tiles wide (x_kts = 0: K / 16, 0);
 * h [M][N] fp32 += r(m) X W^T; x_pk = bf16(h gain gscale) at columns [x_col0, x_col0 + N) of a packed buffer x_ld wide (x_ld = 0: N), needs
 * gain; x2_pk = bf16(h) likewise; part [M][N / 8] (required); rs_* the deferred RMSNorm scale of the rows of X (rs_part null: none);
 * wide_tiles / alone / kpart / ticket as mgk_gemm_resid_mt. */
typedef struct mgk_resid_desc {
    const void* X; int x_kts, x_k0;
    const void* W;
    float* h;
    const float* gain; float gscale;
    void* x_pk; int x_ld, x_col0;
    void* x2_pk; int x2_ld, x2_col0;
    float* part;
    int M, N, K;
    const float* rs_part; int rs_nparts; float rs_inv_d, rs_eps;
    int wide_tiles, alone;
    float* kpart; int* ticket;
} mgk_resid_desc;
/* mgk_proj_desc = the second projection of a pair (GemmArgs): its own window of X, W [N padded to 32][K], the row scale, both_halves; the
 * output by epilogue: 4 (per head) q [M][N / 64][64] bf16 (N = H * 64: target 0 HF_STEP_Q, the others none, as the engine), 2 (packed relu)
 * out_pk packed [M][N], 0 (fp32 store) out_f32 [M][ldo]. */
typedef struct mgk_proj_desc {
    const void* X; int x_kts, x_k0;
    const void* W;
    int N, K;
    const float* rs_part; int rs_nparts; float rs_inv_d, rs_eps;
    int both_halves;
    void* q;
    void* out_pk;
    float* out_f32; int ldo;
} mgk_proj_desc;
int mgk_gemm_resid_ex(void* stream, const mgk_resid_desc* r);
int mgk_gemm_pair_ex(void* stream, const mgk_resid_desc* r, const mgk_proj_desc* g, int epi);
/* The QKV launch of the decode step (gemm_rows, per-head epilogue): targets / formats as mgk_gemm_heads (0 none, 4 step q [M][H][64], 5 step
 * k / v into the cache [M][H][S_cap][64] at the row's position = pos_rows ? pos_rows[m] : (pos_dev ? *pos_dev : pos)), X as a window, the
 * deferred row scale, GemmArgs::both_halves. */
int mgk_gemm_heads_step(void* stream, const void* X_pk, int x_kts, int x_k0, const void* W_pk, int M, int N, int K, void* p0, void* p1, void* p2,
                        int f0, int f1, int f2, int H, int S_cap, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps, int pos,
                        const int* pos_dev, const int* pos_rows, int both_halves);
/* The lm_head launch of the decode step (gemm_rows_splitk, KS = 1) with the row scale; ptop null: plain projection into P [M][ldp]; otherwise
 * the greedy tail's partials ptop [M][ceil(N / 32)] float4 = {best, second, index of the best (int bits), lse ? sum exp(x - best) : 0} over each
 * 32-feature tile's non-stop features, stopv [M][4] = the logits of stop[0 .. 3] (-1: unused), P written only with write_logits. */
int mgk_lm_head_step(void* stream, const void* X_pk, const void* W_pk, float* P, int M, int N, int K, int ldp, const float* rs_part, int rs_nparts,
                     float rs_inv_d, float rs_eps, void* ptop, float* stopv, const int* stop4_host, int write_logits, int lse);
int mgk_add_norm_pack(void* stream, float* h, const float* P, int KS, int ldp, size_t slab_stride, const float* gain,
                      void* x_pk, int M, int d, float eps, float scale);
int mgk_relu_pack(void* stream, const float* P, int KS, int ldp, size_t slab_stride, void* y_pk, int M, int N);
/* Beam-search step kernels, on buffers the caller owns (device pointers), in the launch order of the decode step.  Geometry: 2 <= K <= 8,
 * B * K <= 1024, max_len >= 2 (MG_E_SHAPE otherwise; mgk_beam_state_bytes then returns 0).
 *   init        state (mgk_beam_state_bytes), next_ids [B*K] i64, anc [T_cap][B*K] (T_cap >= max_len - 1), counters [8] i32 ([0] continue)
 *   step        logits [B*K][ldl] (columns >= V never read); cur_len by value, or tdev (cur_len = *tdev + 1) with div_table [max_len + 1]
 *               of mgk_beam_length_divisor values; slot_pos / slot_live [B*K] (both or neither): the queue form.  Writes next_ids, beam_idx
 *               [B*K] i32 and, in the batch form, counters[0]
 *   reorder_anc anc[j][r] <- anc[j][beam_idx[r]] for j < t_written (tdev: j <= *tdev; queue form: rows of live slots with j <= pos)
 *   finalize    out_ids [B*num_return][max_len], out_cols [1], out_scores [B*num_return], beam_indices / token_scores
 *               [B*num_return][max_len - 1] (nullable)
 *   slots_step  the queue form's end / assign / init after a step: pos, img, pool, live [slots*K], bpool, assign [slots], ctr [16] i32
 *               ([0] live slots, [1] images done, [2] steps, [4] queue head, [5] images ready, [7] oldest live image), out_ids
 *               [N*num_return][max_len], out_len [N], out_scores [N*num_return], beam_indices / token_scores as finalize */
size_t mgk_beam_state_bytes(int B, int K, int max_len);
float mgk_beam_length_divisor(int cur_len, float length_penalty);
int mgk_beam_init(void* stream, void* state, int B, int K, int max_len, int pad, int eos, int start, int64_t* next_ids, int* anc, int T_cap,
                  int* counters);
int mgk_beam_step(void* stream, void* state, const float* logits, int ldl, int V, int B, int K, int max_len, int cur_len, const int* tdev,
                  const float* div_table, int eos, int min_len, float length_penalty, int early_stopping, int64_t* next_ids, int* beam_idx,
                  int* counters, const int* slot_pos, const int* slot_live);
int mgk_beam_reorder_anc(void* stream, int* anc, const int* beam_idx, int rows, int t_written, const int* tdev, const int* counters,
                         const int* slot_pos, const int* slot_live);
int mgk_beam_finalize(void* stream, void* state, int B, int K, int max_len, int64_t* out_ids, int* out_cols, float* out_scores, int num_return,
                      int* beam_indices, float* token_scores);
int mgk_beam_slots_step(void* stream, void* state, int slots, int K, int max_len, int pad, int eos, int start, int early_stopping, int* pos,
                        int* img, int* pool, int* bpool, int* live, int* assign, int64_t* next_ids, int* anc, int T_cap, int pool_cap,
                        int64_t* out_ids, int* out_len, float* out_scores, int* ctr, int end_first, int num_return, int* beam_indices,
                        float* token_scores);
/* init / step of the batch form under a decoder prompt (mg_generate_prompted): prompt_ids [B][prompt_ld] i64, prompt_len [B] i32 (device; one
 * prompt per image, 1 <= len <= prompt_ld, len < max_len).  init: the K rows of image b hold its prompt (ids outside [0, V) -> 0, counted
 * in *bad, nullable).  step: an image whose cur_len is below its prompt length appends the forced token to every beam (beam_idx = identity);
 * otherwise stock's step with decoder_prompt_len = its length.  div_table [max_len + 1] is required in both the by-value and the tdev form. */
int mgk_beam_init_prompted(void* stream, void* state, int B, int K, int max_len, int pad, int eos, int start, int64_t* next_ids, int* anc,
                           int T_cap, int* counters, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld, int V, int* bad);
int mgk_beam_step_prompted(void* stream, void* state, const float* logits, int ldl, int V, int B, int K, int max_len, int cur_len, const int* tdev,
                           const float* div_table, int eos, int min_len, float length_penalty, int early_stopping, int64_t* next_ids,
                           int* beam_idx, int* counters, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld);
/* The selection step under a constraint (mg_generate_constrained; DecConstraint in csrc/mg_kernels.h), batch forms of the greedy scan and
 * of the sampled selection (a slot table, the fused form or ptop with a constraint: MG_E_ARG).  All pointers device.  cls is padded to the
 * logits' row stride ([ldl], the padding is never taken for a token); state [rows] is read and advanced in place; *empty counts the rows
 * that met an empty allowed set.  Sizes are checked as mg_generate_constrained checks them, before any device work (MG_E_ARG).  The
 * decoder prompt is optional (prompt_ids NULL: none): a forced column leaves the row's state untouched, as a finished row does.
 * mgk_select_constrained = mgk_select_ex / mgk_select_prompted; mgk_sample_select_constrained = mgk_sample_select_prompted plus top2
 * [rows][2] (nullable; with pos_dev the base of [max_len][rows][2]) - neither clears n_unfinished. */
typedef struct mgk_constraint {
    const uint16_t* cls;     /* [ldl] */
    const int32_t* table;    /* [n_states][n_classes]: next state, -1 = not allowed */
    int n_states, n_classes;
    int32_t* state;          /* [rows] */
    int32_t* empty;          /* [1] */
} mgk_constraint;
int mgk_select_constrained(void* stream, const mgk_select_desc* s, const mgk_constraint* con, const int64_t* prompt_ids, const int* prompt_len,
                           int prompt_ld, int group, int* bad);
/* Beam search under a constraint: mgk_beam_init_prompted / mgk_beam_step_prompted plus the constraint (prompt_ids NULL: no prompt; cls here
 * is [V]).  init: con->state[b * K + k] = con_start[b] (con_start [B] device).  step: the log-softmax stays over the raw logits and a token
 * the row's state does not allow gets the log-probability -inf where MinLength's EOS does; afterwards running beam k holds
 * table[state of its parent][cls[token]], the sink where that entry is -1; a forced prompt column leaves the states untouched.  div_table
 * [max_len + 1] is required.  *empty is not used: -inf candidates are what stock has there too. */
int mgk_beam_init_constrained(void* stream, void* state, int B, int K, int max_len, int pad, int eos, int start, int64_t* next_ids, int* anc,
                              int T_cap, int* counters, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld, int V, int* bad,
                              const mgk_constraint* con, const int* con_start);
int mgk_beam_step_constrained(void* stream, void* state, const float* logits, int ldl, int V, int B, int K, int max_len, int cur_len,
                              const int* tdev, const float* div_table, int eos, int min_len, float length_penalty, int early_stopping,
                              int64_t* next_ids, int* beam_idx, int* counters, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld,
                              const mgk_constraint* con);
int mgk_sample_select_constrained(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                                  int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids,
                                  int max_len, int pos, const int* pos_dev, int* unfinished, int* n_unfinished, int* step_ctr, float* token_scores,
                                  int ts_ld, float* top2, const mgk_constraint* con, const int64_t* prompt_ids, const int* prompt_len,
                                  int prompt_ld, int group, int* bad);
/* The greedy / sampled queue forms of the selection step and slot_refill under a decoder prompt and / or a constraint
 * (mg_generate_stream_constrained).  q NULL, or prompt_ids and con both NULL: the plain operators (mgk_select_ex with a slot table,
 * mgk_sample_select_queue, mgk_slot_refill), byte for byte.  prompt_ids [images][prompt_ld] / prompt_len [images] / con_start [images] are
 * per image of the queue, con->state [rows] per slot; the owner of a live row is slots.img[row] / slots.nsamp.  mgk_select_queue_ex needs a
 * slot table (MG_E_ARG without).  mgk_slot_refill_ex: a slot handed sequence i is fed prompt_ids[i / nsamp][0] (checked against V, counted
 * in *bad, written to out_ids[i][0] when out_ids [sequences][out_ld] is given) and gets state con_start[i / nsamp]. */
typedef struct mgk_queue_con {
    const int64_t* prompt_ids; const int* prompt_len; int prompt_ld, V; int* bad;
    const mgk_constraint* con;   /* nullable */
    const int* con_start;
} mgk_queue_con;
int mgk_select_queue_ex(void* stream, const mgk_select_desc* s, const mgk_queue_con* q);
int mgk_sample_select_queue_ex(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                               int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids, int max_len,
                               int* unfinished, float* token_scores, int ts_ld, const mgk_slot_table* slots, const mgk_queue_con* q);
int mgk_slot_refill_ex(void* stream, const mgk_slot_table* slots, int64_t* next_ids, int* unfinished, int rows, const mgk_queue_con* q,
                       int64_t* out_ids, int out_ld);
/* The beam queue under the same: mgk_beam_step in the queue form (slot_pos / slot_live required; slot_img [slots * K] = the image in a
 * row's slot, required with a prompt) and mgk_beam_slots_step, whose newly assigned slots start as mgk_beam_init_constrained starts the
 * image they are handed (prompt in both sequence arrays, the K states at con_start[image], the prompt's first token fed first).  cls is
 * [V] here, con->state [slots * K]; *empty is not used.  q NULL: mgk_beam_step / mgk_beam_slots_step. */
int mgk_beam_step_queue_ex(void* stream, void* state, const float* logits, int ldl, int V, int B, int K, int max_len, const float* div_table,
                           int eos, int min_len, float length_penalty, int early_stopping, int64_t* next_ids, int* beam_idx, int* counters,
                           const int* slot_pos, const int* slot_live, const int* slot_img, const mgk_queue_con* q);
int mgk_beam_slots_step_ex(void* stream, void* state, int slots, int K, int max_len, int pad, int eos, int start, int early_stopping, int* pos,
                           int* img, int* pool, int* bpool, int* live, int* assign, int64_t* next_ids, int* anc, int T_cap, int pool_cap,
                           int64_t* out_ids, int* out_len, float* out_scores, int* ctr, int end_first, int num_return, int* beam_indices,
                           float* token_scores, const mgk_queue_con* q);

/* ------------------------------------------------------------------------------------------------------------------------------
 * ChemicalOCR stage ("next" row f-1).  Replaces, for the OCR pass that produces the cells the main model
 * reads, what /root/reference/markushgrapher/ocr/chemical_ocr.py does on one 512-px page at a time:
 *     processor, model = AutoProcessor / AutoModelForVision2Seq.from_pretrained(model_path)            chemical_ocr.py:76-84
 *     inputs = processor(text=prompt, images=[image], return_tensors="pt", size={"longest_edge": 512})  chemical_ocr.py:368-373
 *     generated_ids = model.generate(**inputs, max_new_tokens=4096, do_sample=False)                    chemical_ocr.py:375-380
 * i.e. stock Idefics3ForConditionalGeneration (SigLIP-style vision tower, pixel-shuffle connector, Llama-style text model),
 * greedy.  Tokenisation / image resizing stay on the host (the stock processor); this library takes the processor's tensors.
 * Padded frames (non-square pages: pixel_attention_mask not all ones) are given as the patch grid the stock model derives from the
 * mask: patch_mask [N][P] u8 (a patch is valid if any of its pixels is) and patch_pos [N][P] i32 (the bucketed fractional coordinates
 * of Idefics3VisionEmbeddings, modeling_idefics3.py:128-172, computed by the host wrapper with the same torch ops); both NULL = full
 * frames.  v1 limits: head dim 64 everywhere; every sequence of a call has the same prompt length (no padding), the same number of
 * frames and exactly n_img * image_seq_len <image> tokens.  Same conventions as above (device pointers, caller-owned buffers).
 * ------------------------------------------------------------------------------------------------------------------------------ */
typedef struct mg_ocr_model mg_ocr_model;
typedef struct mg_ocr_config {
    /* Idefics3VisionConfig */
    int v_hidden, v_inter, v_layers, v_heads, image_size, patch_size;
    /* LlamaConfig of the text model */
    int t_hidden, t_inter, t_layers, t_heads, t_kv_heads, vocab;
    /* Idefics3Config */
    int scale_factor, image_token_id, eos_token_id, pad_token_id, tie_word_embeddings;
    float v_eps, rms_eps, rope_theta;
    /* further stop tokens: generation_config.json's eos_token_id may be a list (e.g. <|im_end|> and <end_of_utterance>); a row
     * finishes on eos_token_id or any of eos_extra[0 .. n_eos_extra) (generation/utils.py:2927-2937 with a list of EOS ids) */
    int n_eos_extra, eos_extra[3];
} mg_ocr_config;

int mg_ocr_create(const mg_ocr_config* cfg, mg_ocr_model** out);
void mg_ocr_destroy(mg_ocr_model* m);
/* a further execution context on a finalized model's weights (see mg_clone): own captured graphs, calls may overlap in time with the
 * source's when made from another host thread on another stream with another workspace */
int mg_ocr_clone(const mg_ocr_model* src, mg_ocr_model** out);
size_t mg_ocr_weights_bytes(const mg_ocr_model* m);
int mg_ocr_bind_weights(mg_ocr_model* m, void* arena);
/* hf_key: a state-dict key of stock Idefics3ForConditionalGeneration ("model.vision_model....", "model.connector....",
 * "model.text_model....", "lm_head.weight"); src: device tensor, fp32 (src_is_bf16 = 0) or bf16 bits. */
int mg_ocr_load_tensor(mg_ocr_model* m, void* stream, const char* hf_key, const void* src, int src_is_bf16, const int64_t* shape, int ndim);
int mg_ocr_finalize(mg_ocr_model* m, void* stream);
int mg_ocr_workspace_bytes(const mg_ocr_model* m, int B, int n_img, int L, int max_new_tokens, int full_logits, size_t* out_bytes);
/* get_image_features (modeling_idefics3.py:563-622): pixel_values [N][3][I][I] fp32 -> out [N][image_seq_len][t_hidden] fp32
 * (workspace: mg_ocr_workspace_bytes(m, N, 1, 1, 0, 0)). */
int mg_ocr_image_features(mg_ocr_model* m, void* stream, void* ws, size_t ws_bytes, const float* pixel_values, const int32_t* patch_pos,
                          const uint8_t* patch_mask, int N, float* out);
/* Teacher-forced forward (modeling_idefics3.py:750-840): input_ids [B][L] i64, pixel_values [B][n_img][3][I][I] fp32 (NULL with
 * n_img = 0: text only) -> logits [B][L][vocab] fp32.  Workspace with full_logits = 1.  SYNCHRONISES (reports bad inputs). */
int mg_ocr_forward(mg_ocr_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* pixel_values,
                   const int32_t* patch_pos, const uint8_t* patch_mask, int B, int n_img, int L, float* logits);
/* generate(max_new_tokens, do_sample=False) (generation/utils.py:2783-2975): out_ids [B][max_new_tokens] i64 = the NEW tokens
 * (finished rows padded with pad_token_id), *out_cols_host = columns HF would have produced (steps until every row had emitted
 * EOS).  step_logits (nullable, tests): [capture_steps][B][vocab] fp32 pre-argmax logits of the first steps.  SYNCHRONISES. */
int mg_ocr_generate(mg_ocr_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* pixel_values,
                    const int32_t* patch_pos, const uint8_t* patch_mask, int B, int n_img, int L, int max_new_tokens, int64_t* out_ids,
                    int* out_cols_host, float* step_logits, int capture_steps);

/* Queue form of mg_ocr_generate (continuous decoding): N pages, `slots` decode rows (<= 256).  Vision tower + prompt prefill of all
 * pages first (chunk <= 256 pages per pass) into per-page KV caches, each prefill selecting its page's first token; then a row whose
 * page emits a stop token / reaches max_new_tokens takes the next page (a pointer change: the cache is already there), so the
 * call runs sum(lengths) / slots steps instead of walking every row to the longest page.  Per-page ids equal mg_ocr_generate's.
 * out_ids [N][max_new_tokens] i64 (pad after the stop token), out_len [N] i32 (device), *steps_host decode steps (nullable).
 * Same input contract as mg_ocr_generate (equal prompt length L and n_img frames for every page; prompts of different lengths:
 * mg_ocr_generate_stream_ragged below).  SYNCHRONISES. */
int mg_ocr_stream_workspace_bytes(const mg_ocr_model* m, int N, int n_img, int L, int max_new_tokens, int slots, int chunk, size_t* out_bytes);
int mg_ocr_generate_stream(mg_ocr_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const float* pixel_values,
                           const int32_t* patch_pos, const uint8_t* patch_mask, int N, int n_img, int L, int max_new_tokens, int slots, int chunk,
                           int64_t* out_ids, int32_t* out_len, long* steps_host);
/* The same with prompts of DIFFERENT lengths: input_ids [N][L] holds every page's prompt_len[n] <= L tokens LEFT-ALIGNED (anything behind them is
 * never attended), prompt_len [N] i32 on the device (null: mg_ocr_generate_stream).  What stock transformers computes for the left-padded batch the
 * Idefics3 processor makes of such prompts (position = cumsum(attention_mask) - 1, pad keys masked: every row as if alone; modeling_llama.py
 * position_ids, generation/utils.py prepare_inputs_for_generation) - the reference itself never makes one: its transformers backend calls
 * generate() one page at a time with one prompt (markushgrapher/ocr/chemical_ocr.py:366-392).  Every page still carries n_img frames. */
int mg_ocr_generate_stream_ragged(mg_ocr_model* m, void* stream, void* ws, size_t ws_bytes, const int64_t* input_ids, const int32_t* prompt_len,
                                  const float* pixel_values, const int32_t* patch_pos, const uint8_t* patch_mask, int N, int n_img, int L,
                                  int max_new_tokens, int slots, int chunk, int64_t* out_ids, int32_t* out_len, long* steps_host);

/* ------------------------------------------------------------------------------------------------------------------------------
 * OCSR vision branch "e1" (SURVEY.md section 8 rows a7 / f-2).  The reference's model evaluates, inside forward() / generate() of its
 * transformers fork,
 *     model.encoder.molscribe_encoder    MolScribe's Swin-B (timm swin_base_patch4_window12_384; weights swin_base_char_aux_1m680k.pth)
 *     model.encoder.molscribe_projector  an MLP projector into d_model
 * and concatenates the result in front of the decoder with the VTL encoder's states ("late fusion", architecture_variant
 * me-lf-stack-1): /root/reference/markushgrapher/core/common/begin.py:119-120,137-151, utils/model/utils_model_loading.py:20-36,
 * config/predict.yaml:12,17-18, README.md:212-215.  mg_e1_* computes that branch; mg_attach_e1 makes mg_encode / mg_generate /
 * mg_generate_stream* evaluate it themselves whenever no precomputed e1 is passed.
 * The Swin arithmetic is stock transformers models/swin/modeling_swin.py (patch embedding + LayerNorm, (shifted-)window attention with
 * the relative-position bias table and the -100 region mask, exact-erf GELU MLP, patch merging, final LayerNorm) and is pinned on
 * stock SwinModel; what the fork does around it is INFERRED and therefore configuration: the branch's input = bilinear resize
 * (torch.nn.functional.interpolate, align_corners = false) of the model's pixel_values from src_image_size to image_size followed by
 * x * pix_scale[c] + pix_shift[c]; the projector = n_proj Linear layers (with bias) with proj_act between them.
 * Keys of mg_e1_load_tensor: "swin." + the state-dict names of stock SwinModel(add_pooling_layer=False), and "proj.{j}.weight|bias"
 * (markushgrapher_amd/e1_shapes.py maps timm / transformers-4.x checkpoints onto them).  v1 limits (errors, never silent): head dim
 * 32, stage widths 64 .. 1024 (powers of two), window 4 / 8 / 12, every stage's map a multiple of the window (the reference geometry:
 * 96 / 48 / 24 / 12 with window 12).
 * ------------------------------------------------------------------------------------------------------------------------------ */
typedef struct mg_e1_model mg_e1_model;
typedef struct mg_e1_config {
    /* SwinConfig */
    int image_size, patch_size, num_channels, embed_dim, n_stages;
    int depths[4], num_heads[4];
    int window_size, mlp_ratio;
    float layer_norm_eps;
    /* projector: Linear(C_last -> proj_dims[0]) [act] ... Linear(-> proj_dims[n_proj - 1] = d_model); proj_act 0 none, 1 GELU (erf) */
    int n_proj, proj_dims[4], proj_act;
    /* input derivation */
    int src_image_size;
    float pix_scale[3], pix_shift[3];
} mg_e1_config;

int mg_e1_create(const mg_e1_config* cfg, mg_e1_model** out);
void mg_e1_destroy(mg_e1_model* m);
size_t mg_e1_weights_bytes(const mg_e1_model* m);
int mg_e1_bind_weights(mg_e1_model* m, void* arena);
int mg_e1_load_tensor(mg_e1_model* m, void* stream, const char* key, const void* src, int src_is_bf16, const int64_t* shape, int ndim);
int mg_e1_finalize(mg_e1_model* m, void* stream);
int mg_e1_out_tokens(const mg_e1_model* m);          /* M: tokens per image (144 for Swin-B at 384 px) */
int mg_e1_workspace_bytes(const mg_e1_model* m, int B, size_t* out_bytes);
/* pixel_values [B][num_channels][src_image_size][src_image_size] fp32 (the VTL model's input) ->
 *   e1_out       [B][M][d_model] fp32 (nullable)        what mg_encode / mg_generate take as `e1`
 *   features_out [B][M][C_last] fp32 (nullable)         SwinModel.last_hidden_state (the pinned part)
 * Reads the model, writes only caller buffers: one mg_e1_model may be used by several threads / execution contexts at once (each
 * with its own workspace and stream).  Enqueues only. */
int mg_e1_encode(const mg_e1_model* m, void* stream, void* ws, size_t ws_bytes, const float* pixel_values, int B, float* e1_out,
                 float* features_out);
/* Attach the branch to a model (and to the clones made from it afterwards; NULL detaches): mg_encode / mg_generate calls that pass
 * e1 = NULL, and every mg_generate_stream / mg_generate_stream_beam call, then evaluate mg_e1_encode on their pixel_values inside the
 * call (in the call's own workspace: mg_workspace_bytes / mg_stream_*_workspace_bytes account for it once attached) and decode over
 * [e1 | e2] - what the reference's model does with architecture_variant me-lf-stack-1.  A precomputed e1 passed by the caller still
 * takes precedence.  The branch must outlive the model; d_model, src_image_size and num_channels must match the model's config. */
int mg_attach_e1(mg_model* m, const mg_e1_model* e1);

#ifdef __cplusplus
}
#endif
#endif
