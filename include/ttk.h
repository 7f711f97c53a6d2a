/* libttk -- C ABI of the MI355X-native TorToiSe inference hot path.
 *
 * The reference (e-c-k-e-r/tortoise-tts) is pure Python and has no FFI of its own; its plugin idiom is replacing the
 * module objects that `TTS.inference` calls (tortoise_tts/inference.py:185-202).  The entry points
 * below are what a binding for those call sites needs; each cites the reference interface it stands in for.  The
 * Python classes in tortoise_tts_amd/ wrap them under the reference's own method names.
 *
 * Conventions
 *  - return 0 on success, a negative TTK_E_* code on failure; ttk_last_error() gives the text; nothing throws or aborts.
 *  - every tensor argument is a raw DEVICE pointer to a contiguous row-major buffer in the reference's layout
 *    (b x C x T channels-first for the diffusion net, B x S x D for the AR net); the caller owns them.
 *  - `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); calls only enqueue work and never
 *    synchronise, allocate or free (except the create and destroy calls and the first call that grows a workspace), so a decode
 *    step or a diffusion step can be captured into a HIP graph by the caller.
 *  - a handle owns packed weights, KV cache and workspaces; one handle per (process, device); not re-entrant.  Different handles may be
 *    driven from different host threads on different streams (ttk_last_error is per thread).
 *  - weights are passed as f32 tensors (host or device memory) under the reference's state_dict key names and are copied.
 */
#ifndef TTK_H
#define TTK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTK_VERSION 1

enum { TTK_OK = 0, TTK_E_ARG = -1, TTK_E_HIP = -2, TTK_E_WEIGHT = -3, TTK_E_STATE = -4 };
/* arithmetic mode: storage/MFMA operand type (accumulation is always f32).  TTK_FP8W (BASELINE config 5) = TTK_BF16 arithmetic with
 * the GEMM weights of the GPT-2 blocks / ResBlocks / AttentionBlocks rounded to fp8-e4m3 (OCP, round to nearest even) times a
 * power-of-two per-tensor scale; the KV-cached decode streams them as fp8 bytes, the dense GEMMs hold the same values in bf16.
 * TTK_FP8 (diffusion handle only) = TTK_FP8W with the ACTIVATION operand of the ResBlock / AttentionBlock GEMMs rounded to fp8-e4m3 as well
 * (scale 1: they are GroupNorm outputs and attention outputs), those GEMMs running on the fp8 MFMA with f32 accumulation: the result is
 * the TTK_BF16 arithmetic applied to operands rounded that way, up to f32 summation order.  Diffusion handle, both fp8 modes (round 6): the
 * AttentionBlocks' q / k / v projection keeps its weights and its activation operand in bf16 -- e4m3 on q and k moves peaked attention scores
 * by whole units -- so "block GEMMs" there means in_layers.2, out_layers.3 and proj_out.
 * TTK_F16 (autoregressive and diffusion handles) = the TTK_BF16 design with IEEE half operands on v_mfma_f32_16x16x32_f16 -- the other dtype the
 * reference's `torch.autocast("cuda", dtype)` at inference.py:331 can be given (config.py:625-637); f32 accumulation, residual streams,
 * norms and softmax as in every mode, so unlike autocast nothing but an operand above 65504 can overflow. */
enum { TTK_F32 = 0, TTK_BF16 = 1, TTK_FP8W = 2, TTK_FP8 = 3, TTK_F16 = 4 };

typedef struct {
	const char* name;     /* reference state_dict key, e.g. "gpt.h.0.attn.c_attn.weight" */
	const float* data;    /* f32, contiguous, host or device */
	int ndim;
	int64_t shape[4];
} ttk_weight_view;

int ttk_version(void);
const char* ttk_last_error(void);   /* thread-local text of the last failure */

/* Per-kernel timing for the roofline report (no reference counterpart: the reference has no profiling of its own,
 * SURVEY.md section 5).  Between begin and end every libttk kernel launch is bracketed by HIP events on its own stream and
 * tallied per kernel kind together with its algorithmic work.  Do not capture graphs while enabled.
 * kinds: 0 gemm (flop), 1 skinny gemm (bytes), 2 attention fwd (flop), 3 decode attention (bytes), 4 groupnorm stats (bytes),
 *        5 groupnorm apply (bytes), 6 layernorm (bytes)                                                                 */
typedef struct { double ms; int64_t launches; double work; } ttk_prof_result;
int ttk_prof_begin(void);
int ttk_prof_end(ttk_prof_result* out, int n_kinds);   /* n_kinds >= 7; synchronises the device */

/* ------------------------------------------------------------------------------------------------------------------
 * Autoregressive model: UnifiedVoice + GPT2InferenceModel (tortoise_tts/models/unified_voice.py:98-254, 334-668).   */
typedef struct ttk_ar ttk_ar;

typedef struct {
	int layers, model_dim, heads;             /* unified_voice.py:337-339 ; head_dim must be 64 */
	int max_mel_seq_len, max_text_seq_len;    /* rows of the two learned position tables (:405-406) */
	int number_text_tokens_p1, number_mel_codes;
	int start_text_token, stop_text_token, start_mel_token, stop_mel_token;
	int dtype;                                /* TTK_F32 | TTK_BF16 | TTK_F16 | TTK_FP8W */
	int max_batch;                            /* candidates decoded together (<= 64; <= 32 in TTK_F32) */
	int max_ctx;                              /* KV-cache rows per sequence: prefix + generated tokens */
} ttk_ar_config;

/* Copies and packs the hot-path subset of UnifiedVoice.state_dict() (tortoise_tts_amd/weights.py: ar_shapes). */
int ttk_ar_create(ttk_ar** out, const ttk_ar_config* cfg, const ttk_weight_view* w, int n_w);
int ttk_ar_destroy(ttk_ar* h);

/* Prefill = first forward of `generate` (unified_voice.py:639-649 prefix build, :203-211 prefill branch, lm_head :239).
 *   cond_latent [Bc, D] f32 (Bc == 1 or B), text [Tt] int64 raw token ids (start/stop are added here, :639-640)
 *   logits_out  [B, number_mel_codes] f32 = logits of the last prefill row.  Resets the KV cache to P + 1 rows.   */
int ttk_ar_prefill(ttk_ar* h, const float* cond_latent, int Bc, const int64_t* text, int Tt, int B,
				   float* logits_out, void* stream);

/* Prefill of a PROMPTED continuation (`inference_speech(..., input_tokens=)`, unified_voice.py:651-656: the mel tokens of `input_tokens` follow start_mel in the
 * first forward, :203-211): prompt = device int64 [prompt_rows][n_prompt] mel codes, prompt_rows == 1 (one prompt for all candidates: it joins the shared
 * prefix) or B.  Mel positions 1 .. n_prompt; the cache then holds P + 1 + n_prompt rows, the logits are those of the last prompt row, and the first
 * decode step feeds its token at mel position n_prompt + 2 (the reference's attention_mask.shape[1] - mel_len).                                          */
int ttk_ar_prefill_prompted(ttk_ar* h, const float* cond_latent, int Bc, const int64_t* text, int Tt, const int64_t* prompt, int prompt_rows, int n_prompt, int B,
							float* logits_out, void* stream);

/* One KV-cached decode step (unified_voice.py:212-214 + HF GPT2Model + lm_head): feeds back tok [B] int64, the k-th
 * generated token (k = 1, 2, ... counted by the handle), with mel position k + 1 (the reference's indexing).
 *   logits_out [B, number_mel_codes] f32;  hidden_out (optional, may be NULL) [B, D] f32 = final_norm(ln_f(h)) of the
 *   new row, what `sample_stream` yields (stream_generator.py:1172).                                               */
int ttk_ar_decode(ttk_ar* h, const int64_t* tok, float* logits_out, float* hidden_out, void* stream);

/* final_norm(ln_f(h)) [B, D] f32 of the newest row: after ttk_ar_prefill the prefix's last row, after a decode step that step's row
 * (valid until the next ttk_ar_sample_next / decode call reuses the row buffer).  `sample_stream` yields this next to the token sampled
 * from the same forward's logits (stream_generator.py:1172) -- for the first token that is the prefill's row.                     */
int ttk_ar_last_hidden(ttk_ar* h, float* hidden_out, void* stream);

/* Host-only (no GPU call; usable before any handle exists): the geometry the decode launches of a handle created with (dtype, max_batch) run with when
 * `rows` candidates are decoded -- out[0] = rows ttk_ar_create allocates and zeroes for each fragment-order operand (attention output, MLP
 * activations, the T-typed residual copy), out[1] = sixteen-row tiles of the kernel instantiation the launch selects, out[2] = rows that
 * instantiation requests (every tile of it, whatever `rows` is), out[3] = candidate slices of the KV cache.  out[2] <= out[0] for every
 * rows <= max_batch is what ttk_ar_create asserts and every decode entry re-checks; tests/test_host_logic.py enumerates it.  No reference
 * counterpart (the reference's tensors are sized by the call that makes them).                                                              */
int ttk_ar_decode_geometry(int dtype, int max_batch, int rows, int32_t out[4]);

/* What the decode step's folded LayerNorm (ln_1 + c_attn, ln_2 + c_fc as one matrix over the UN-normalised rows, T-typed) could not represent
 * well since the last call: bit 0 = a row of the residual stream had |mean| > 8 std (more than 3 of the operand's significand bits went to the
 * common offset the norm removes: results drift from the reference's LayerNorm-then-matmul; TTK_AR_LNFOLD=0 selects the form that normalises
 * in f32 first), bit 1 = non-finite row statistics (an f16 operand above 65504).  Synchronises `stream`, clears the word.  No reference
 * counterpart: the fold is this library's, so is the duty to say when it does not apply.                                                   */
int ttk_ar_health(ttk_ar* h, int* flags_out, void* stream);

/* The same rows for EVERY decode step of a captured token loop, without a per-step pointer: while set, each ttk_ar_decode / ttk_ar_decode_next
 * also writes final_norm(ln_f(h)) [B, D] f32 of its new rows to base + index[0] * stride (elements), `index` a device int64 the sampling launch
 * advances (the `col` of ttk_sample_args: tokens sampled so far), so step n's rows land in slot n of a [slots, B, D] buffer although the
 * captured launch arguments never change -- what the streaming generator (unified_voice.py:670-679, stream_generator.py:1172) yields next to
 * token n.  The base is uploaded to a device word on `stream` and read from there by the launches, so a token step captured during one
 * generation writes into the buffer of whichever generation replays it.  Pass base = NULL to switch it off.                            */
int ttk_ar_set_hidden_ring(ttk_ar* h, float* base, const int64_t* index, int64_t stride, void* stream);

/* One sampled token per candidate, the body of HF `_sample` that stream_generator.py drives (warpers :56-101; HF:generation/
 * utils.py:2894-2937): probs = softmax(scores / temperature); next = multinomial(probs, 1) = argmax(probs / q) with q the caller's
 * Exp(1) noise [B, V] (torch `exponential_`, so the generator stream is the reference's); finished rows get `stop_token`;
 * tok[b] = next; ids[b, col[b]] = next (skipped when col[b] >= ids_cols); history[b, hist_off + col[b]] = next (optional);
 * col[b] += 1; unfinished[b] &= next != stop_token.  suppress (optional) is a [V] byte mask of ids forced to -inf before the
 * temperature (SuppressTokensLogitsProcessor); any other warper is applied by the caller, who then passes temperature 1.
 * live_rows / all_done (optional): *live_rows (device int, caller sets it to the number of unfinished rows) is decremented when a
 * row finishes, and the row that brings it to 0 stores the number of tokens sampled so far (col + 1 >= 1: the generation ended WITH that
 * token) to *all_done (device or pinned host int, zeroed by the caller) -- HF's
 * `unfinished_sequences.max() == 0` stopping test without a host round trip per token.  Pointers are device memory unless said
 * otherwise; only enqueues one kernel, so it may be captured in a HIP graph.                                               */
int ttk_sample_step(const float* scores, int64_t ld, int B, int V, const float* q, int64_t ldq,
					const unsigned char* suppress, float temperature, int64_t stop_token, int64_t* unfinished, int64_t* tok, int64_t* ids, int64_t ids_ld, int64_t ids_cols,
					int64_t* col, int64_t* history, int64_t hist_ld, int64_t hist_off, int* live_rows, int* all_done,
					void* stream);

/* ttk_sample_step with the reference's other processors and warpers inside the same kernel, in HF's order (stream_generator.py:56-101 builds
 * Temperature -> TopK -> TopP; HF `_get_logits_processor` puts RepetitionPenaltyLogitsProcessor and SuppressTokensLogitsProcessor in front):
 *   repetition_penalty (HF:generation/logits_process.py RepetitionPenaltyLogitsProcessor): every id that occurs in history[b, 0 : hist_off + col[b]]
 *     (= input_ids: the caller writes the prefix ids into the first hist_off columns, the kernel appends the sampled ones) has its score
 *     multiplied (< 0) or divided (>= 0) by the penalty; 1 or 0 = off;
 *   suppress, temperature: as ttk_sample_step;
 *   top_k (TopKLogitsWarper): scores below the k-th largest become -inf; 0 = off;
 *   top_p (TopPLogitsWarper): ascending cumulative softmax <= 1 - top_p becomes -inf, the largest score always stays; >= 1 or 0 = off.
 * The CLI's defaults (__main__.py:17-21: top-k 16) therefore stay on this one launch: no torch.topk / torch.sort per token, no host
 * round trip, capturable.  top-k / top-p / typical sampling / the penalty need V <= 9216 (the row is held in registers).
 *   typical_mass (TypicalLogitsWarper, unified_voice.py:47-75; what `inference_speech(typical_sampling=True)` adds as a custom processor): tokens in
 *     ascending |-log p - H| are kept until their probability mass reaches typical_mass, the others become -inf; runs after the penalty and the
 *     suppression, before the temperature; 0 or >= 1 = off.                                                                              */
typedef struct {
	const float* scores; int64_t ld; int B, V;
	const float* q; int64_t ldq;              /* Exp(1) noise of torch.multinomial, drawn by the caller */
	const unsigned char* suppress;            /* [V] byte mask or NULL */
	float temperature;                        /* > 0 */
	int top_k; float top_p; float repetition_penalty;
	int64_t stop_token;
	int64_t *unfinished, *tok, *ids; int64_t ids_ld, ids_cols; int64_t* col;
	int64_t* history; int64_t hist_ld, hist_off;   /* optional unless repetition_penalty is on */
	int *live_rows, *all_done;                /* optional, see ttk_sample_step */
	float typical_mass;                       /* TypicalLogitsWarper (unified_voice.py:47-75), applied after the processors and before the temperature,
	                                           * where the reference's custom logits_processor runs; 0 or >= 1 = off */
} ttk_sample_args;
int ttk_sample_step_warped(const ttk_sample_args* a, void* stream);

/* The same launch, additionally writing the input row of the decode step that follows (the first lines of GPT2InferenceModel.forward's
 * cached branch, unified_voice.py:212-214): x[b] = mel_embedding[tok[b]] + mel_pos_embedding[col[b] + 1] with col[b] already counting
 * the new token (the reference's k + 1 indexing).  ttk_ar_decode_next then runs the step from that row: the pair replaces
 * ttk_ar_decode's embedding-gather launch.  Both may be mixed freely with ttk_ar_decode on one handle.                        */
int ttk_ar_sample_next(ttk_ar* h, const ttk_sample_args* a, void* stream);
int ttk_ar_decode_next(ttk_ar* h, float* logits_out, float* hidden_out, void* stream);

/* Greedy search: the same token step with do_sample=False (HF `_sample`, HF:generation/utils.py:2925: `next_tokens = torch.argmax(next_token_scores,
 * dim=-1)`; the reference's fork has the same line in its greedy branch).  Per row, in HF's order: repetition penalty over history[b, 0 : hist_off + col[b]],
 * suppress mask, typical_mass (the custom processor of `inference_speech(typical_sampling=True)`; 0 or >= 1 = off), then the argmax of the processed
 * scores, then the bookkeeping of ttk_sample_step unchanged (finished rows get stop_token; tok, ids, history, col, unfinished, live_rows / all_done).
 * Exact ties go to the LOWEST index: torch.argmax leaves the order among equal values unspecified, so this is the library's choice, as for ttk_beam_step.
 * NOT READ: q, ldq, temperature, top_k, top_p -- HF builds no warpers without do_sample (it only warns), and greedy search draws nothing; q may be NULL.
 * No softmax and no exponentiation except inside the typical warper.  1 <= V <= 9216 (the row is held in registers), else TTK_E_ARG.
 * ttk_ar_greedy_next is to ttk_greedy_step what ttk_ar_sample_next is to ttk_sample_step_warped: the same launch also writes the next decode step's input
 * row mel_embedding[tok] + mel_pos_embedding[col + 1], from which ttk_ar_decode_next runs.  Each enqueues one kernel; capturable.                     */
int ttk_greedy_step(const ttk_sample_args* a, void* stream);
int ttk_ar_greedy_next(ttk_ar* h, const ttk_sample_args* a, void* stream);

/* The reference's own samplers (tortoise_tts/samplers.py; the controls of webui.py:251-265, the commented-out arguments of inference.py:154-163) on a second
 * token-step kernel, k_sample_step_ext (csrc/sample_ext.hip): ttk_sample_step_warped's launch, operands and bookkeeping, with a second struct beside
 * ttk_sample_args, which keeps its layout.  Per row, in this order (everything not named is ttk_sample_step_warped's):
 *   repetition_penalty_decay != 0: reptition_penalize(factor = repetition_penalty, decay, one_time=True) (:11-29) REPLACES HF's processor: over
 *     previous = history[b, hist_off : hist_off + col[b]] (prompt and sampled tokens; NOT the hist_off prefix ids), every distinct token, d = 1 + the number of
 *     tokens behind its most recent occurrence, gets score *= 1.0f / (float)(repetition_penalty * pow((double)d, (double)decay)) -- a division whatever the
 *     sign of the score.  repetition_penalty 1 is off, as in the reference.  one_time=False is not built.
 *   stop_length_penalty != 0: length_penalize (:35-40): score[stop_token] *= 1.0f / (float)pow((double)(col[b] + 1), (double)stop_length_penalty); > 0
 *     lengthens, < 0 shortens.  (`length_penalty` is HF's beam ranking in this ABI and in the reference's call, hence the name.)
 *   suppress, typical_mass;
 *   min_temperature >= 0: dynamic_temperature (:78-91, k = 10, centre 0.5) in the place of the temperature warper, in front of top-k (the reference never wired
 *     it, there is no other order to match): p_max = 1 / sum exp(s - max), T_dyn = T - (T - T_min) / (1 + exp(-10 (p_max - 0.5))), scores *= 1.0f / (float)T_dyn;
 *     negative = off;
 *   top_k, top_p;
 *   mirostat_tau > 0: mirostat v1 (mirostat_sample :117-158) in the place of the plain draw, on mirostat_mu[b] (the reference's max_surprise; the caller
 *     sets it to 2 tau before the first token): k from the 101 largest probabilities of softmax(scores) and mu, computed in f64 (a non-finite value = V,
 *     clamped to [1, V]); the k largest scores stay (equal scores at the threshold stay together, as with top_k); token = argmax over them of
 *     softmax_kept / q; mu -= eta (log2(1 / P[token]) - tau).  Rows with fewer than 101 finite scores (where the reference raises ZeroDivisionError)
 *     keep all of them (k = their number) and still update mu.  A finished row's mu may hold anything.  q is ttk_sample_args' noise row, indexed by
 *     token id: NOT the Philox consumption of the reference's torch.multinomial over the k sorted entries (it depends on k), but the same distribution,
 *     and the noise block per token of the plain draw, so the caller's generator accounting is that of ttk_sample_step_warped.  0 = off.
 * Optional outputs, written when non-null: scores_out [B][scores_out_ld] f32 = the scores behind top_p (-inf where removed; HF's output_scores), temp_out [B]
 * f32 = the temperature applied, mirostat_k [B] int32.
 * Every field off (0, 0, negative, 0): the result equals ttk_sample_step_warped's bit for bit.  TTK_E_ARG: V > 9216, mirostat_tau > 0 without mirostat_mu,
 * mirostat_eta < 0, min_temperature > temperature, decay or stop_length_penalty without `history`.  ttk_ar_sample_next_ext is to ttk_sample_step_ext what
 * ttk_ar_sample_next is to ttk_sample_step_warped.  Each enqueues one kernel and keeps all state in device memory: capturable.                             */
typedef struct {
	float repetition_penalty_decay;           /* 0 = HF's processor */
	float stop_length_penalty;                /* 0 = off */
	float min_temperature;                    /* < 0 = off; <= temperature */
	float mirostat_tau;                       /* 0 = off */
	float mirostat_eta;                       /* >= 0 */
	double* mirostat_mu;                      /* [B], read and written; required with mirostat_tau > 0 */
	int* mirostat_k;                          /* [B] or NULL */
	float* temp_out;                          /* [B] or NULL */
	float* scores_out; int64_t scores_out_ld; /* [B][scores_out_ld >= V] or NULL */
} ttk_sample_ext;
int ttk_sample_step_ext(const ttk_sample_args* a, const ttk_sample_ext* x, void* stream);
int ttk_ar_sample_next_ext(ttk_ar* h, const ttk_sample_args* a, const ttk_sample_ext* x, void* stream);

/* The Exp(1) noise of torch.multinomial without torch in the token step.  `q.exponential_(1)` on the GPU is a pure function of (generator seed,
 * generator offset, element index, launch geometry) -- ATen's distribution_nullary_kernel over a Philox4_32_10 state (csrc/ttk_rng.h restates
 * the indexing; the state and the uniform conversion are rocRAND's own header code, as in torch's build).  ttk_ar_set_noise makes the mel-head
 * launch of ttk_ar_prefill / ttk_ar_decode[_next] write q[m][n] for its logits: rng_args = device int64[6] {seed, offset before the first draw,
 * threads of torch's launch for the full [C, V] tensor, offset step per draw, first row of this handle's candidates in that tensor, candidates per text line or 0 (ttk_ar_prefill_lines)}, draws =
 * device int64[B] draws made so far per row (the `col` of ttk_sample_args), q = f32 rows [B][V].  The caller advances the torch generator by
 * step x draws afterwards, so everything drawn later is the reference's stream too.  Pass NULLs to switch it off.
 * ttk_exponential_like_torch fills out[li] for li < numel with the same function (draw-th draw): the bitwise comparison against
 * torch.Tensor.exponential_ that a caller runs before relying on it (tortoise_tts_amd/autoregressive.py does).                          */
int ttk_ar_set_noise(ttk_ar* h, const int64_t* rng_args, const int64_t* draws, float* q);
int ttk_exponential_like_torch(float* out, int64_t numel, int64_t seed, int64_t offset0, int64_t threads, int64_t step, int64_t draw, void* stream);

/* Several text lines prefilled as ONE decode batch (no reference counterpart: TTS.inference walks the lines of a text one by one,
 * inference.py:244-246, streaming the weights again for each line's 16 candidates).  Line g: conditioning latent cond_latents[g] (f32 [n_lines][model_dim]),
 * text ids text[sum(text_len[:g]) ...] (device int64, concatenated), text_len[g] of them (HOST int array); it occupies candidates
 * [g * rows_per_line, (g + 1) * rows_per_line).  logits_out f32 [n_lines * rows_per_line][number_mel_codes].  The prefixes are right-aligned in the cache (one cache length for the batch); the decode entries
 * then step all candidates together, the attention reading every candidate's keys from where its line begins, and every row's logits are bit for bit those of ttk_ar_prefill / ttk_ar_decode
 * on its line alone.  With ttk_ar_set_noise, rng_args[5] = rows_per_line makes every line draw the same [rows_per_line, V] noise, as the reference's
 * reseeding to 0 per line does.                                                                                                   */
int ttk_ar_prefill_lines(ttk_ar* h, const float* cond_latents, const int64_t* text, const int* text_len, int n_lines, int rows_per_line,
						 float* logits_out, void* stream);

/* Beam search (`TTS.inference(beam_width=N)`, inference.py:161,342: generate(num_beams=N); HF:generation/utils.py `_beam_search` :3208-3509 with
 * do_sample=True is the behaviour restated).
 *
 * ttk_ar_reorder_cache = `_reorder_cache` (unified_voice.py:257-265; HF :3477-3489): beam_idx = device int64 [B], B the prefilled rows (<= 16);
 * new candidate slice b takes the K/V history of old slice beam_idx[b].  In place, one launch: a thread owns one 16-byte piece of one cache row,
 * loads it from every source slice and only then stores the destinations.  Only rows [shared prefix, valid rows) move -- both bounds are
 * the handle's device position words, so the launch may be captured; the shared prefix (ttk_ar_prefill) is one copy for all beams and stays.
 * An identity beam_idx returns before the first load; an entry outside [0, B) moves nothing.  TTK_E_STATE before a prefill and after
 * ttk_ar_prefill_lines.                                                                                                                  */
int ttk_ar_reorder_cache(ttk_ar* h, const int64_t* beam_idx, void* stream);

/* The same gather for a batch of lines, each searched by rows_per_line beams (ttk_beam_step_lines): valid only after ttk_ar_prefill_lines with that
 * rows_per_line (TTK_E_STATE otherwise).  beam_idx = device int64 [B], global over the batch: entry g * rows_per_line + b holds g * rows_per_line + source
 * beam.  Rows [d_pos[1], d_pos[0]) of all B slices move; in lines mode d_pos[1] is the length of the longest prefix: every line's right-aligned prefix lies
 * below it, in the slice of the line's first candidate, and never moves.  An entry outside its own line's range
 * [g * rows_per_line, (g + 1) * rows_per_line) moves nothing, as an out-of-range entry of ttk_ar_reorder_cache does; an identity beam_idx returns before the
 * first load.  B <= 16.                                                                                                                     */
int ttk_ar_reorder_cache_lines(ttk_ar* h, const int64_t* beam_idx, int rows_per_line, void* stream);

/* One step of `_beam_search` for one text line, steps b to g (HF:generation/utils.py:3386-3508), batch_size 1, early_stopping False,
 * pad = eos = stop_token.  With c = col[0] tokens generated so far:
 *   b. per beam row: log_softmax(logits) (:3388), then the processors and warpers ON THE LOG-PROBS in HF's order (:3389; the semantics of
 *      ttk_sample_step_warped): repetition penalty over {prefix_ids, that beam's own c tokens}, suppress, temperature, top-k, top-p -- the
 *      last two with min_tokens_to_keep = 2, as `_get_logits_processor` builds them for num_beams > 1 (:1297-1322) -- plus running score (:3419);
 *   c. `_get_top_k_continuations` (:3077-3129): multinomial WITHOUT replacement of 2 * num_beams from softmax over the flat [num_beams * V]
 *      = the 2 * num_beams largest of softmax / q in descending order, q the caller's Exp(1) noise of that flat tensor (ATen's no-replacement
 *      path; ttk_ar_set_noise with a candidate count of num_beams draws exactly it); beam = idx / V, token = idx % V;
 *   d. a continuation hits the stopping criteria with token == stop_token or c + 1 == max_new (MaxLengthCriteria);
 *   e. `_get_running_beams_for_next_iteration` (:3131-3151);  f. `_update_finished_beams` (:3153-3204) with length_penalty;
 *   g. tok [num_beams] / beam_idx [num_beams] for the next forward and ttk_ar_reorder_cache (:3481), `_check_early_stop_heuristic`
 *      (:3008-3052), `_beam_search_has_unfinished_sequences` (:3055-3075): when the search is over, c + 1 goes to state[2 * num_beams + 1] and to
 *      *all_done (optional; device or pinned host int, zeroed by the caller), and every later call is a no-op.
 * Exact ties (softmax / q, and the scores of e. and f.) go to the lowest index: torch leaves that order unspecified (entries of probability
 * exactly 0 -- the -1e9 beams of the first step, everything top-k / top-p cut -- tie at 0), so this is the library's choice, not the reference's;
 * callers keep top_k == 0 or >= 2 * num_beams.  Scalar divisions are ATen's GPU form, x * (1 / f32(s)).
 * State, all device memory the caller initialises once per generation (L = max_new):
 *   col    int64 [num_beams], zeros: tokens generated so far (every entry is advanced; also the draw counter of ttk_ar_set_noise);
 *   seqs   int64 [2][2][num_beams][L], stop_token: generated tokens of {running, finished} beams, read from half c & 1 and written to the other
 *          (after n steps the finished beams are seqs[n & 1][1], best first; row b holds state[num_beams + b] tokens, then stop_token);
 *   scores f32 [2][num_beams]: running_beam_scores = {0, -1e9, ...} and beam_scores = {-1e9, ...} (:3332-3334);
 *   state  int [2 * num_beams + 2]: is_sent_finished [num_beams] = 0, finished lengths [num_beams] = 0, heuristic bit = 1, done word = 0;
 *   acc    f32 [num_beams * V] and work int [4 * num_beams^2 + 2 * num_beams + 1] (zeroed once): scratch between the two launches.
 * Enqueues two kernels; capturable.  num_beams 2..16, 2 * num_beams <= V <= 9216.                                                         */
typedef struct {
	const float* logits; int64_t ld; int num_beams, V;
	const float* q;                           /* Exp(1) noise, flat [num_beams * V] */
	const unsigned char* suppress;            /* [V] byte mask or NULL */
	float temperature;                        /* > 0 */
	int top_k; float top_p; float repetition_penalty, length_penalty;
	int64_t stop_token, prefix_ids[2];        /* what the penalty sees in front of the generated tokens: {1, start_mel} (unified_voice.py:647-649) */
	int max_new;
	int64_t *col, *seqs; float* scores; int* state;
	float* acc; int* work;
	int64_t *tok, *beam_idx;                  /* out [num_beams] */
	int* all_done;                            /* optional */
} ttk_beam_args;
int ttk_beam_step(const ttk_beam_args* a, void* stream);

/* The same step for n_lines text lines searched together as one decode batch, n_lines >= 1 and n_lines * num_beams <= 16 rows (no reference counterpart:
 * the reference searches line by line).  The same struct; every state array has a leading [n_lines] dimension: logits has n_lines * num_beams rows
 * (line g's beams are rows g * num_beams ...), q is [n_lines][num_beams * V] (ttk_ar_set_noise with rng_args[5] = num_beams gives every line the flat tensor
 * of its own call), col [n_lines][num_beams], seqs [n_lines][2][2][num_beams][L], scores [n_lines][2][num_beams], state [n_lines][2 * num_beams + 2],
 * acc [n_lines][num_beams * V], work [n_lines][4 * num_beams^2 + 2 * num_beams + 1], tok and beam_idx [n_lines * num_beams].  Workgroup x serves line
 * x / num_beams with that line's slices; the last workgroup of a line to arrive does that line's bookkeeping; lines read none of each other's words, so
 * every line's state is bit for bit what ttk_beam_step leaves on that line alone -- with two differences.  beam_idx is global: entry g * num_beams + b holds
 * g * num_beams + source beam, what ttk_ar_reorder_cache_lines takes.  And the step that ends line g's search (its count goes to that line's
 * state[2 * num_beams + 1]) writes stop_token to the line's tok rows and the identity to its beam_idx rows: the decode and the reorder go on for the other
 * lines, every later step returns at entry for this one.  *all_done (optional) is written, non-zero, by the step that ends the last unfinished line.
 * Two launches; capturable.                                                                                                                  */
int ttk_beam_step_lines(const ttk_beam_args* a, int n_lines, void* stream);

/* hipGraphLaunch of an instantiated graph the caller captured around libttk launches (torch.cuda.CUDAGraph.raw_cuda_graph_exec()): the
 * token step replayed without torch.cuda.CUDAGraph.replay()'s prologue, which fills the generator's seed / offset tensors -- two launches per
 * token -- whether or not the captured work draws random numbers.  With ttk_ar_set_noise it does not.                                      */
int ttk_graph_launch(void* graph_exec, void* stream);

/* The weight rounding of TTK_FP8W applied in place to a device f32 array: x <- fp8_e4m3(x / s) * s with s = the smallest power of
 * two >= max|x| / 448, returned in *scale_out (host).  This is exactly what ttk_*_create does to a TTK_FP8W matrix, exposed so that a
 * caller (and the parity tests) can build the equivalent TTK_BF16 model.                                                     */
int ttk_fp8_round_weights(float* x, int64_t n, float* scale_out, void* stream);

/* UnifiedVoice.forward(..., return_latent=True, clip_inputs=False) (unified_voice.py:544-599, get_logits :508-522):
 *   cond [B, D] f32, text [B, Tt] int64, codes [B, M] int64  ->  latents_out [B, M, D] f32 (= mel_logits[:, :-2]).  */
int ttk_ar_latents(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B,
				   float* latents_out, void* stream);

/* UnifiedVoice.forward(..., return_latent=False, text_first=True) on inputs that are clipped and padded already (unified_voice.py:576-612,
 * get_logits :508-531): the teacher-forced dense pass, ln_f + final_norm on the text rows 1 .. Tt+2 and the mel rows Tt+3 .. Tt+M+4 of every
 * sequence, text_head / mel_head, and F.cross_entropy against the targets of build_aligned_inputs_and_targets (:489-492), built on the device:
 *   text [t_0 .. t_{Tt-1}, stop_text, stop_text], mel [c_0 .. c_{M-1}, stop_mel, stop_mel].
 *   cond [B, D] f32, text [B, Tt] int64, codes [B, M] int64.  Every output is optional (null = not wanted), all f32:
 *   loss_out[2] = {text mean, mel mean} (means in the order of ttk_xent_rows); nll_text_out [B, Tt+2], nll_mel_out [B, M+2] = the
 *   reduction="none" rows; text_logits_out [B, number_text_tokens + 1, Tt+2], mel_logits_out [B, number_mel_codes, M+2] = the reference's
 *   permute(0, 2, 1), contiguous.
 * Needs a handle created with `text_head.weight` / `text_head.bias` among its weights (else TTK_E_STATE).  B is not bound by max_batch; the
 * KV cache and the state of a running generation are not touched.                                                                     */
int ttk_ar_score(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, float* loss_out,
				 float* nll_text_out, float* nll_mel_out, float* text_logits_out, float* mel_logits_out, void* stream);

/* The GPT-2 attention maps of that same teacher-forced pass: what get_logits(..., get_attns=True) returns (unified_voice.py:508-516, which
 * forward(return_attentions=True) reaches at :593-602; HF eager attention, HF:models/gpt2/modeling_gpt2.py:144-226).  The sequence has S = Tt + M + 5 rows:
 * 0 conditioning latent, 1 start_text, 2 .. Tt+1 the text, Tt+2 stop_text, Tt+3 start_mel, Tt+4 .. Tt+3+M the codes, Tt+4+M stop_mel.
 *   P[q][k] = softmax over k <= q of 0.125 q_q . k_k on the q and k columns the layer's c_attn GEMM wrote (in the 16-bit modes the rounded values the pass
 *   itself used), accumulated in f32, stored as f32 in every dtype, exactly 0 for k > q.
 * ttk_ar_attentions: layers[n_layers] (host, distinct, each in [0, layers))  ->  out f32 [n_layers][B][H][S][S] (device), layers[j]'s maps at index j.
 * ttk_ar_text_attention: layer_head[n][2] (host, {layer, head} pairs)  ->  out f32 [B][n][M][Tt] (device), the text-alignment block of pair i at index i:
 *   A[m][t] = P[Tt+3+m][2+t], row Tt+3+m being the row that predicts code m.  Its rows do not sum to 1.
 * Both run the dense pass of ttk_ar_latents and read each selected layer's q and k from the pass's own qkv buffer right behind the c_attn GEMM; the pass
 * stops behind the last selected layer.  cond [B, D] f32, text [B, Tt] int64, codes [B, M] int64.  B is not bound by max_batch; the KV cache and the
 * state of a running generation are not touched; adapted (ttk_ar_lora_set) and fp8-weight handles give the maps of what they compute.
 * TTK_E_ARG with a message: an empty or out-of-range selection, a repeated layer, an output of 2 GiB or more (select fewer layers / heads).   */
int ttk_ar_attentions(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, const int* layers, int n_layers,
					  float* out, void* stream);
int ttk_ar_text_attention(ttk_ar* h, const float* cond, const int64_t* text, int Tt, const int64_t* codes, int M, int B, const int* layer_head, int n,
						  float* out, void* stream);

/* Run-time LoRA adapters on a live handle (the reference: TTS.enable_lora / disable_lora, inference.py:99-104, and the weight parametrization
 * W + (lora_B lora_A) * alpha / rank of models/lora.py:120-123, 136-145).  The adapted matrices are the 4 x layers HF Conv1D weights
 * gpt.h.<l>.{attn.c_attn, attn.c_proj, mlp.c_fc, mlp.c_proj}.weight, [K_in][N_out]; lora_B is [K_in][rank], lora_A [rank][N_out].
 *
 * The init call (once, after create; `weights` as given to create, host or device) keeps f32 masters of those matrices plus scratch for one of them
 *   in the handle: 12 d^2 layers 4 bytes (1.51 GB at d = 1024, 30 layers).  TTK_FP8W handles are refused (TTK_E_ARG): their per-matrix scale follows
 *   the adapted matrix.  A handle that never makes this call is what it was before the call existed.
 * The set call makes the handle compute with W0 + (lora_B lora_A) * scaling for every module whose pair is among `adapters`, and with W0 for every
 *   other one; n == 0 detaches everything.  adapters[i].name is "<module>.lora_A" / "<module>.lora_B" (module as above, without ".weight"),
 *   .data an f32 DEVICE pointer that stays valid until the work enqueued here has run, .shape the two sizes; rank 1..256.
 *   Arithmetic, per element: acc = 0; for r rising: acc = acc + lora_B[k][r] * lora_A[r][n], product and sum each rounded to f32 (no fused multiply-add);
 *   W' = W0 + acc * scaling, again two roundings.  A plain f32 loop on the host reproduces the bits, and the packed operands are written by the launches
 *   create uses: a switched handle computes bit for bit what a handle created from the host-folded weights computes.
 *   Only enqueues on `stream`: no allocation, no synchronisation, operands rewritten in place (a captured token step stays valid) and only for matrices
 *   that are or become adapted.  The caller must not switch while a generation is between its prefill and its last step.
 *   Every view is checked before the first launch; TTK_E_ARG / TTK_E_WEIGHT name the tensor: no init call before, half a pair, a module outside the
 *   4 x layers, a shape that does not fit, rank > 256.  After a refusal the handle is unchanged.                                              */
int ttk_ar_lora_init(ttk_ar* h, const ttk_weight_view* weights, int n_w);
int ttk_ar_lora_set(ttk_ar* h, const ttk_weight_view* adapters, int n, float scaling, void* stream);

/* Row cross-entropy on its own (csrc/xent.hip), F.cross_entropy(reduction="none") of f32 logits [rows][ld] whose first C columns are valid
 * (columns [C, ld) are never read) against int64 target [rows]:  nll_out[r] = logsumexp(x_r) - x_r[target[r]], the maximum subtracted before
 * the exponential, one pass over the row.  A target outside [0, C) gives NaN for that row and reads nothing.
 *   mean_out (optional, 1 float): part[i] = nll[i] + nll[i + 256] + ... added in that order from 0.f for i in 0..255, then part[i] += part[i + o]
 *     for o = 128, 64, .. 1 (i < o), mean = part[0] / rows.  One workgroup, no atomics: the same bits on every run.
 *   logits_t_out (optional): the same logits, f32 [rows / T][C][T] contiguous (row r = b * T + t  ->  [b][c][t]); rows % T == 0.          */
int ttk_xent_rows(const float* logits, int64_t ld, int rows, int C, const int64_t* target, float* nll_out, float* mean_out,
				  float* logits_t_out, int T, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Diffusion decoder: DiffusionTTS + the DDIM / ancestral step (tortoise_tts/models/diffusion.py:1389-1574, 325-431,
 * 646-694, 510-554) and AttentionBlock / GroupNorm32 / RelativePositionBias (arch_utils.py:24-190, xtransformers.py:148). */
typedef struct ttk_diff ttk_diff;

typedef struct {
	int model_channels, num_layers, in_channels, in_latent_channels, out_channels, num_heads;   /* diffusion.py:1392-1400 */
	int dtype;                                /* TTK_F32 | TTK_BF16 | TTK_F16 | TTK_FP8W | TTK_FP8 */
} ttk_diff_config;

/* Besides the hot-path subset of DiffusionTTS.state_dict() (weights.py: diffusion_shapes) the caller passes two derived
 * host tables: "__time_freqs" [C/2] (diffusion.py:1288-1290) and, per attention block, "<block>.__relbias" [H, 129] =
 * scale * emb[bucket(d)] for d = -64..64 (xtransformers.py:157-188) -- built by tortoise_tts_amd/diffusion.py.       */
int ttk_diff_create(ttk_diff** out, const ttk_diff_config* cfg, const ttk_weight_view* w, int n_w);
int ttk_diff_destroy(ttk_diff* h);

/* DiffusionTTS.timestep_independent(latents, cond, T, False) (diffusion.py:1487-1510):
 *   latents [b, M, Cl] f32, cond [b, 2C] f32, interp_idx [T] int32 device (nearest-neighbour source row of each output
 *   frame, F.interpolate) -> E_out [b, C, T] f32.                                                                    */
int ttk_diff_precompute(ttk_diff* h, const float* latents, const float* cond, const int32_t* interp_idx, int b, int M,
						int T, float* E_out, void* stream);

/* DiffusionTTS.timestep_independent(codes, cond, T, return_code_pred) for integer mel codes (diffusion.py:1487-1515, the `else` of :1493):
 *   codes [b, M] int64 device -> code_embedding rows -> code_converter (three AttentionBlocks) -> the same code_norm / modulation / expansion as
 *   ttk_diff_precompute -> E_out [b, C, T] f32; mel_pred_out (NULL, or [b, in_channels, T] f32) = mel_head(E), the k = 3 convolution of :1512.
 * Needs a handle whose create call was given "code_embedding.weight" [in_tokens, C] (in_tokens is read off that view), "code_converter.{0,1,2}.*"
 * (+ "__relbias", as every attention block) and "mel_head.weight" / "mel_head.bias" (weights.py: diffusion_code_shapes); else TTK_E_STATE.  The
 * caller validates the ids (0 <= id < in_tokens; tortoise_tts_amd/diffusion.py raises IndexError); the gather clamps, so no id reads outside
 * the table.  Nothing is synchronised.                                                                                                     */
int ttk_diff_precompute_codes(ttk_diff* h, const int64_t* codes, const float* cond, const int32_t* interp_idx, int b, int M, int T,
							  float* E_out, float* mel_pred_out, void* stream);
/* mel_head over embeddings that already exist: E [b, C, T] f32 (from either precompute entry) -> mel_pred_out [b, in_channels, T] f32, bit for
 * bit what ttk_diff_precompute_codes writes beside the same E.  The reference's `return_code_pred=True` on LATENT conditioning (:1509-1515). */
int ttk_diff_mel_head(ttk_diff* h, const float* E, int b, int T, float* mel_pred_out, void* stream);

/* DiffusionTTS.forward(x, t, precomputed_aligned_embeddings=E[, conditioning_free=True]) (diffusion.py:1517-1574):
 *   x [b, in, T] f32, t [b] int64 device, E [b, C, T] f32 or NULL (=> conditioning_free) -> out [b, out_channels, T].  */
int ttk_diff_forward(ttk_diff* h, const float* x, const int64_t* t, const float* E, int b, int T, float* out, void* stream);

typedef struct {
	int64_t t;                 /* original-schedule timestep fed to the network (_WrappedModel map, diffusion.py:1232-1237) */
	float sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac_prev, sqrt_1m_ac_prev;   /* float64 tables -> f32 (:1264) */
	float coef1, coef2, min_log, max_log;                                   /* ancestral sampler only */
	float cfk;                 /* conditioning-free weight of this step (:391-393); < 0 disables the second evaluation */
	int sampler;               /* 0 = ddim (eta 0), 1 = p */
	int nonzero;               /* p sampler: add noise (i != 0) */
} ttk_step;

/* Stage E (as returned by ttk_diff_precompute, [b, C, T] f32) for a run of ttk_diff_step calls. */
int ttk_diff_begin(ttk_diff* h, const float* E, int b, int T, void* stream);
/* One sampler step: both network evaluations batched (cond + cond-free share every weight read), then the fused
 * epilogue; x [b, in, T] f32 updated in place; noise [b, in, T] f32 for the p sampler (NULL for ddim).
 * (GaussianDiffusion.p_mean_variance / ddim_sample / p_sample, diffusion.py:325-431, 646-694, 510-554)               */
int ttk_diff_step(ttk_diff* h, float* x, const ttk_step* st, const float* noise, void* stream);
/* Whole DDIM loop: steps[n-1], ..., steps[0] applied in that order (ddim_sample_loop_progressive :794-810).  The conditioning integrator of a
 * step does not depend on x, so the one of the next step runs on an internal side stream beside the current step's body; the side stream is
 * forked from and joined back to `stream` inside the call (results are ordered on `stream`; identical to the one-stream loop bit for bit). */
int ttk_diff_sample_ddim(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, int n_steps, void* stream);

/* The DDIM loop for several utterances of DIFFERENT length as one batch (no reference counterpart: the reference diffuses a text's lines one at
 * a time, inference.py:237-422; its network is batch-capable, diffusion.py:1517-1574, and its ramped conditioning-free guidance asserts b = 1
 * only because it reads t[0], :391-393 -- every element of this batch is at the same step).  Element e occupies a slot of Tp frames (Tp % 64 == 0)
 * of which tlen[e] (HOST array, 1..Tp) are real: x [b, in, Tp] f32 in place, E [b, C, Tp] f32; padding frames are ignored on input and
 * undefined on output.  Element e comes out bit for bit as ttk_diff_sample_ddim(b = 1, T = tlen[e]) gives it.  b <= 32.                      */
int ttk_diff_sample_ddim_lines(ttk_diff* h, float* x, const float* E, int b, int Tp, const int* tlen, const ttk_step* steps, int n_steps, void* stream);

/* Whole ancestral-sampler loop (p_sample_loop_progressive, diffusion.py:556-644 -- what the second caller of the path, train.py:178, runs with
 * 30 steps): the same two-stream loop with p_sample's update (:510-554).  noise [n_steps, b, in, T] f32: the `th.randn_like(x)` draws of the
 * steps in the order the loop makes them (block j belongs to the j-th executed step, steps[n-1-j]); the caller draws them so the generator
 * stream stays the reference's.  Equal to n_steps ttk_diff_step calls bit for bit.                                                       */
int ttk_diff_sample_p(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, int n_steps, const float* noise, void* stream);

/* The rest of the reference sampler's argument space (GaussianDiffusion.ddim_sample with eta :646-694, clip_denoised=False :401-403,
 * ddim_reverse_sample :696-732), as a second per-step struct beside ttk_step, whose `sampler` field these entries do not read, and a kernel of its
 * own, k_diffusion_step_ext: the entries above keep their code.                                                                             */
typedef struct {
	float sigma;               /* mode 0: eta sqrt((1 - ac_prev) / (1 - ac)) sqrt(1 - ac / ac_prev), f32 as torch computes it (:679-683); 0 reads no noise */
	float dir;                 /* mode 0: sqrt(1 - ac_prev - sigma^2) (:688); == sqrt_1m_ac_prev at sigma 0 */
	float sqrt_ac_next, sqrt_1m_ac_next;   /* mode 2: f32 square roots of alphas_cumprod_next and of 1 - it (:724-729) */
	int mode;                  /* 0 = ddim with eta, 1 = p, 2 = reverse ddim */
	int clip;                  /* clip_denoised: clamp the predicted x0 to [-1, 1] */
} ttk_step_ext;

/* Whole loop of one mode (every ext[i].mode equal), on the machinery of ttk_diff_sample_ddim: the time path of all steps at once, the two-stream
 * integrator pipeline, each update launch writing the next step's operand copy.  Modes 0 and 1 run steps[n-1], ..., steps[0]; mode 2 runs
 * steps[0], ..., steps[n-1] (x_t -> x_{t+1}: the DDIM encoder).  noise [n_steps, b, in, T] f32, block j for the j-th executed step, as for
 * ttk_diff_sample_p; NULL is accepted when no step reads it (mode 2; mode 0 with every sigma 0), else TTK_E_ARG.  Mode 0 with sigma 0, dir =
 * sqrt_1m_ac_prev and clip equals ttk_diff_sample_ddim bit for bit, mode 1 with clip ttk_diff_sample_p.                                      */
int ttk_diff_sample_ext(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, const ttk_step_ext* ext, int n_steps,
						const float* noise, void* stream);
/* One step behind ttk_diff_begin, as ttk_diff_step; pred_xstart (NULL, or [b, in, T] f32): the x0 prediction the step used (after the clamp when
 * ext->clip), the reference's out["pred_xstart"].  A loop of these equals ttk_diff_sample_ext bit for bit.                                  */
int ttk_diff_step_ext(ttk_diff* h, float* x, const ttk_step* st, const ttk_step_ext* ext, const float* noise, float* pred_xstart, void* stream);
/* Kernel form: the update launch alone on caller buffers.  out_c / out_u [nb, 2 C, T] f32 network outputs (out_u read when st->cfk >= 0), x [nb, C, T]
 * f32 in place, noise / pred_xstart [nb, C, T] f32 or NULL, xcl NULL or the channels-last copy [rep nb T][ldo] of the new x in `xcl_dtype`
 * (TTK_F32 | TTK_BF16 | TTK_F16; columns C .. ldo are not written).                                                                          */
int ttk_diffusion_step_ext_rows(const float* out_c, const float* out_u, float* x, const float* noise, float* pred_xstart, int nb, int C, int T,
								const ttk_step* st, const ttk_step_ext* ext, void* xcl, int ldo, int rep, int xcl_dtype, void* stream);

/* DPM-Solver++(2M) (Lu et al. 2022: data prediction, second-order multistep), the sampler `sample_loop(sampler="dpm++2m")` runs.  No reference counterpart: the
 * reference raises on any name but ddim / p (:500-508).  One network evaluation pair per step as DDIM, and one step of x0 history:
 *   x = c_x x + c_d0 x0 + c_d1 x0_prev,   x0 as ttk_step_ext's (guidance mix, fma, the clamp when `clip`)
 * on a kernel of its own, k_diffusion_step_ms.  The three coefficients come from the host's f64 tables (tortoise_tts_amd/diffusion.py: step_coefs_ms; DESIGN.md has
 * the formulas); c_d1 == 0 makes the step first order -- DDIM's -- and such a step does not read the history.  `ttk_step.sampler` is not read by these entries.   */
typedef struct {
	float c_x;                 /* weight of x: sigma(i-1) / sigma(i); 0 at index 0 */
	float c_d0;                /* weight of this step's x0; 1 at index 0 */
	float c_d1;                /* weight of the previous step's x0; 0 at index n-1 (no history yet) and at index 0 (lower-order final step) */
	int clip;                  /* clip_denoised: clamp the predicted x0 to [-1, 1] */
} ttk_step_ms;

/* Whole loop, steps[n-1], ..., steps[0] with ms[i] beside steps[i], on the machinery of ttk_diff_sample_ddim (time path of all steps at once, two-stream integrator
 * pipeline, each update launch writing the next step's operand copy).  The history lives in a grow-only buffer of the handle; every loop writes it before reading
 * it, so nothing carries over between calls.  ms[n_steps-1].c_d1 != 0 is TTK_E_ARG: there is no history yet.  Equal to n_steps ttk_diff_step_ms calls bit for bit. */
int ttk_diff_sample_ms(ttk_diff* h, float* x, const float* E, int b, int T, const ttk_step* steps, const ttk_step_ms* ms, int n_steps, void* stream);
/* The ragged batch of ttk_diff_sample_ddim_lines under this update, same contract: Tp % 64 == 0, b <= 32, every step with guidance (cfk >= 0), padding frames
 * ignored on input and undefined on output; element e bit for bit what ttk_diff_sample_ms(b = 1, T = tlen[e]) gives.                                              */
int ttk_diff_sample_ms_lines(ttk_diff* h, float* x, const float* E, int b, int Tp, const int* tlen, const ttk_step* steps, const ttk_step_ms* ms, int n_steps,
							 void* stream);
/* One step behind ttk_diff_begin, as ttk_diff_step_ext.  x0_hist [b, in, T] f32 belongs to the caller: read as x0_prev when ms->c_d1 != 0, then overwritten with
 * this step's x0; NULL is accepted when ms->c_d1 == 0 (nothing is kept then), else TTK_E_ARG.  pred_xstart: NULL or [b, in, T] f32.                                  */
int ttk_diff_step_ms(ttk_diff* h, float* x, float* x0_hist, const ttk_step* st, const ttk_step_ms* ms, float* pred_xstart, void* stream);
/* Kernel form: the update launch alone on caller buffers, operands as ttk_diffusion_step_ext_rows with x0_hist [nb, C, T] f32 in the place of noise.               */
int ttk_diffusion_step_ms_rows(const float* out_c, const float* out_u, float* x, float* x0_hist, float* pred_xstart, int nb, int C, int T, const ttk_step* st,
							   const ttk_step_ms* ms, void* xcl, int ldo, int rep, int xcl_dtype, void* stream);

/* ------------------------------------------------------------------ BigVGAN vocoder
 * The generator of models/bigvgan.py (BigVGAN.__init__ :419-486) on the hot path's kernels.  Weights: the generator's state_dict
 * with weight norm folded into plain `weight` tensors (tortoise_tts_amd/vocoder.py does that), plus "__aa_filter" [12], the Kaiser
 * low-pass every Activation1d builds (kaiser_sinc_filter1d(0.25, 0.3, 12), :40-69).                                        */
typedef struct ttk_voc ttk_voc;
typedef struct {
	int num_mels;                             /* 100 */
	int n_ups;                                /* <= 8 */
	int up_rate[8], up_kernel[8];             /* kernel % rate == 0, (kernel - rate) even */
	int ch0;                                  /* upsample_initial_channel; halves per stage, every stage a multiple of 8 */
	int n_kernels;                            /* AMP blocks per stage, 2..4 */
	int rb_kernel[4];                         /* odd, <= 11 */
	int rb_dil[4][3];
	int snake_logscale;
	int dtype;                                /* TTK_F32 | TTK_BF16 */
} ttk_voc_config;
int ttk_voc_create(ttk_voc** out, const ttk_voc_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_voc_destroy(ttk_voc* h);
/* BigVGAN.inference(c) :522-534: mel [B, num_mels, T] f32 (denormalised log-mel) -> audio [B, 1, T * hop] f32 in [-1, 1]; the 10
 * padding frames of -11.5129 and the trimming of their 10 hops happen inside.                                             */
int ttk_voc_inference(ttk_voc* h, const float* mel, int B, int T, float* audio, void* stream);

/* ------------------------------------------------------------------ UnivNet vocoder (vocoder_type="vocoder")
 * UnivNetGenerator of models/vocoder.py (:227-314): conv_pre, one LVCBlock per stride (convt_pre, KernelPredictor, the dilated convs
 * and the location-variable convolutions with their gated updates), conv_post.  Weights: the generator's state_dict with weight norm
 * folded into plain `weight` tensors (tortoise_tts_amd/univnet.py does that).                                                        */
typedef struct ttk_univnet ttk_univnet;
typedef struct {
	int num_mels;                             /* 100 */
	int noise_dim;                            /* 64 */
	int channels;                             /* channel_size c_g: 16 or 32 */
	int n_blocks;                             /* LVC blocks = number of strides, 1..4 */
	int strides[4];                           /* 1..16 each; their product must equal hop_length */
	int n_layers;                             /* dilations per block, 1..4 */
	int dilations[4];
	int kpnet_hidden;                         /* 64 */
	int kpnet_conv_size;                      /* odd, <= 11 (3) */
	int conv_kernel_size;                     /* LVC kernel size: 3 only */
	int hop_length;                           /* 256 */
	int dtype;                                /* TTK_F32 | TTK_BF16 */
} ttk_univnet_config;
int ttk_univnet_create(ttk_univnet** out, const ttk_univnet_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_univnet_destroy(ttk_univnet* h);
/* UnivNetGenerator.inference(c, z) :302-314: mel [B, num_mels, T] f32 (denormalised log-mel), z [B, noise_dim, T + 10] f32 (the caller
 * draws it) -> audio [B, 1, T * hop] f32 in [-1, 1]; the 10 padding frames of -11.5129 and the trimming of their hops happen inside. */
int ttk_univnet_inference(ttk_univnet* h, const float* mel, const float* z, int B, int T, float* audio, void* stream);

/* ------------------------------------------------------------------ HiFiGAN vocoder (vocoder_type="hifigan")
 * HifiganGenerator of models/hifigan.py (:161-305), resblock_type "1", with a cond_layer: the AR model's final_norm latents, one per
 * mel token, to audio -- no diffusion.  Weights: the generator's state_dict with weight norm folded into plain `weight` tensors
 * (tortoise_tts_amd/hifigan.py does that).  One utterance per call.                                                                 */
typedef struct ttk_hifigan ttk_hifigan;
typedef struct {
	int in_channels;                          /* 1024: the latent width */
	int cond_channels;                        /* 1024: the conditioning latent's width; 0 (no cond_layer) is refused */
	int upsample_initial_channel;             /* 512; halves per stage, every stage a multiple of 8 */
	int n_ups;                                /* <= 8 */
	int up_rate[8], up_kernel[8];             /* kernel % rate == 0, (kernel - rate) even */
	int n_kernels;                            /* ResBlocks per stage, 1..4 */
	int rb_kernel[4];                         /* odd, <= 11 */
	int rb_dil[4][3];
	int resblock_type;                        /* 1 only */
	int dtype;                                /* TTK_F32 | TTK_BF16 */
} ttk_hifigan_config;
int ttk_hifigan_create(ttk_hifigan** out, const ttk_hifigan_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_hifigan_destroy(ttk_hifigan* h);
/* once per utterance: g f32 [cond_channels] on the device, the AR conditioning latent; cond_layer(g) is folded into conv_pre's bias */
int ttk_hifigan_set_cond(ttk_hifigan* h, const float* g, void* stream);
/* HifiganGenerator.inference(c, g) :270-296: latents f32 [n, in_channels] -> audio f32 [hop * F], F = floor(4 n * 24000 / 22050) frames
 * (the two linear interpolations happen inside), hop = the product of the upsample rates.                                         */
int ttk_hifigan_inference(ttk_hifigan* h, const float* latents, int n, float* audio, void* stream);

/* ------------------------------------------------------------------ DiscreteVAE: mel -> mel codes -> mel
 * The default DiscreteVAE of models/dvae.py (:116-219; 1-D, two stride-2 k = 3 layers, ReLU, no encoder norm, nearest x2 + conv upsampling, the
 * `Quantize` codebook :12-72), inference side.  Weights: the module's state_dict ("encoder.N...", "decoder.N...", "codebook.embed" [dim, tokens]).
 * The convolutions run in `dtype`; the quantizer runs in f32 in every dtype (codes are ids: a 16-bit distance over thousands of candidates moves them). */
typedef struct ttk_dvae ttk_dvae;
typedef struct {
	int channels;                             /* 80 mel bands */
	int hidden_dim;                           /* 512; the two encoder layers give hidden_dim and 2 * hidden_dim channels; multiple of 8 */
	int codebook_dim;                         /* 512; one of 32, 64, 128, 256, 512 */
	int num_tokens;                           /* 8192 */
	int num_resnet_blocks;                    /* 3; 1..8 */
	int dtype;                                /* TTK_F32 | TTK_BF16 | TTK_F16 */
} ttk_dvae_config;
int ttk_dvae_create(ttk_dvae** out, const ttk_dvae_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_dvae_destroy(ttk_dvae* h);
/* get_codebook_indices :239-246: mel f32 [B, channels, T] -> codes int64 [B, T4], T4 = T passed twice through L -> (L - 1) / 2 + 1; z_out
 * (optional) f32 [B, T4, codebook_dim]: the encoder output the codes were taken from. */
int ttk_dvae_encode(ttk_dvae* h, const float* mel, int B, int T, int64_t* codes_out, float* z_out, void* stream);
/* Quantize.forward :29-39, the index alone: z f32 [M, codebook_dim] -> codes int64 [M], the argmin over j of |e_j|^2 - 2 z . e_j in f32 (the
 * reference's distance less the row constant |z|^2); ties go to the lowest index; the same bits on every run. */
int ttk_dvae_quantize(ttk_dvae* h, const float* z, int M, int64_t* codes_out, void* stream);
/* decode :248-270: codes int64 [B, n] (device) -> mel f32 [B, channels, 4 n] and (optional) the last hidden activation f32 [B, hidden_dim, 4 n].
 * The codes are copied to the host and checked first (this call synchronises `stream`): one outside [0, num_tokens) returns TTK_E_ARG and
 * nothing is launched. */
int ttk_dvae_decode(ttk_dvae* h, const int64_t* codes, int B, int n, float* mel_out, float* hidden_out, void* stream);

/* ------------------------------------------------------------------ random voices: RandomLatentConverter
 * models/random_latent_generator.py:10-52: a Gaussian row through five EqualLinear layers and one nn.Linear is a conditioning latent
 * (`rlg_auto.pth`: 1024 channels, `rlg_diffuser.pth`: 2048).  f32 throughout (csrc/rlg.hip).
 *
 * The layer on its own:  out[r, n] = gain * act(sum_k x[r, k] * W[n, k] + bias[n]),  x f32 [rows][ldx], W f32 row-major [N][K], bias f32 [N] or
 * null, out f32 [rows][ldo]; act 0 = identity, 1 = leaky-ReLU with `slope` (y > 0 ? y : y * slope).
 *   1 <= rows <= 16;  K a multiple of 4, 4 <= K <= 8192;  N >= 1;  ldx >= K and a multiple of 4;  ldo >= N;  x and W 16-byte aligned, x != out.
 *   Anything else returns TTK_E_ARG and launches nothing.
 *   Order of one sum: lane l of a 64-lane wave adds the products of elements 4 (l + 64 i) .. 4 (l + 64 i) + 3, i = 0, 1, .., in rising k with
 *   fmaf from 0.f; the 64 partial sums are folded by a + b over lane distances 32, 16, .. 1.  It does not depend on `rows`: row r of a 16-row call
 *   has the bits of the 1-row call on that row.  No atomics: the same bits on every run.                                                   */
int ttk_linear_rows(const float* x, int64_t ldx, const float* W, const float* bias, int rows, int K, int N, int act, float slope, float gain,
					float* out, int64_t ldo, void* stream);

typedef struct ttk_rlg ttk_rlg;
typedef struct {
	int channels;                             /* 1024 / 2048; a multiple of 4, <= 8192 */
	int n_layers;                             /* 6: layers 0 .. n_layers-2 are act 1 with slope and gain, the last is act 0 with gain 1 */
	int max_rows;                             /* latents drawn by one call, 1..16 */
	float slope;                              /* 0.2 (fused_leaky_relu) */
	float gain;                               /* 2 ** 0.5 */
} ttk_rlg_config;
/* weights: "layers.{i}.weight" [channels, channels] and "layers.{i}.bias" [channels], the EFFECTIVE operands: the caller has folded EqualLinear's
 * `weight * scale` and `bias * lr_mul` (tortoise_tts_amd/random_latent.py does, with the reference's own expressions); they are uploaded as given. */
int ttk_rlg_create(ttk_rlg** out, const ttk_rlg_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_rlg_destroy(ttk_rlg* h);
/* RandomLatentConverter.forward :49-52 behind its torch.randn: noise f32 [rows, channels] -> out f32 [rows, channels]; one launch per layer. */
int ttk_rlg_forward(ttk_rlg* h, const float* noise, int rows, float* out, void* stream);

/* ------------------------------------------------------------------ the TorToiSe detector: AudioMiniEncoderWithClassifierHead
 * models/classifier.py:79-149 (what upstream's `classify_audio_clip` runs from classifier.pth): Conv1d(1, 32, k = 3) on raw 24 kHz audio, `depth`
 * stages of `resnet_blocks` ResBlocks (GroupNorm, SiLU, k = 5 conv, twice, + x) and a k = 5 stride-4 Downsample that doubles the channels,
 * GroupNorm + SiLU + 1x1 conv to embedding_dim, `attn_blocks` AttentionBlocks, position 0, Linear(embedding_dim, classes).  Weights: the module's
 * state_dict ("enc.init.0.*", "enc.res.N.*", "enc.final.{0,2}.*", "enc.attn.N.{norm,qkv,proj_out}.*", "head.*").  The residual stream and every
 * GroupNorm are f32; `dtype` rounds only GEMM / MFMA operands (csrc/classifier.hip). */
typedef struct ttk_cls ttk_cls;
typedef struct {
	int classes;                              /* 2; 1..16 */
	int spec_dim;                             /* 1 */
	int embedding_dim;                        /* 512; a multiple of 128 */
	int depth;                                /* 5; 1..6 */
	int downsample_factor;                    /* 4 */
	int resnet_blocks;                        /* 2 */
	int attn_blocks;                          /* 4 */
	int num_attn_heads;                       /* 4; embedding_dim / num_attn_heads is 64 or 128 */
	int base_channels;                        /* 32 */
	int kernel_size;                          /* 5 */
	int dtype;                                /* TTK_F32 | TTK_BF16 */
} ttk_cls_config;
int ttk_cls_create(ttk_cls** out, const ttk_cls_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_cls_destroy(ttk_cls* h);
/* audio f32 [B, T] (one channel, 24 kHz) -> emb_out f32 [B, embedding_dim] and logits_out f32 [B, classes] (either may be null).  A clip whose last
 * stage has more than 3584 positions at head width 128 is refused (the row-wave attention's limit). */
int ttk_cls_forward(ttk_cls* h, const float* audio, int B, int T, float* emb_out, float* logits_out, void* stream);
/* The same, and copies of the f32 channels-last rows along the way: taps[0] the stem [B, T, 32], taps[1 + l] stage l after its Downsample
 * [B, ceil(L_l / 4), 64 * 2^l], taps[depth + 1] enc.final [B, L_depth, embedding_dim]; n_taps = depth + 2, a null entry is skipped. */
int ttk_cls_forward_taps(ttk_cls* h, const float* audio, int B, int T, float* emb_out, float* logits_out, float* const* taps, int n_taps, void* stream);
/* The fused ResBlock convolution of the 32- and 64-channel stages on its own:
 *   out[b, t, n] = bias[n] + sum_{j < 5} sum_k w[n, k, j] * a[b, t + j - 2, k] (+ residual[b, t, n]),   a = silu(groupnorm(x)) or, with stats null, x;
 * rows outside [0, L) of the SAME batch element are zero.  x, residual, out f32 [B, L, C] (out may be residual, not x), C = 32 | 64; stats f32
 * [B, groups, 2] = (mean, rstd) per group as ttk_cls_gn_stats writes them; gamma, beta f32 [C]; w f32 [C, C, 5] (Conv1d's layout); bias f32 [C].
 * dtype TTK_F32 | TTK_BF16: a and w are rounded to it once, products accumulate in f32, taps ascending, then k ascending in steps of 32. */
int ttk_cls_conv5_rows(int dtype, const float* x, int B, int L, int C, const float* stats, int groups, const float* gamma, const float* beta, const float* w,
					   const float* bias, const float* residual, float* out, void* stream);
/* GroupNorm statistics split over row chunks: x f32 [B, L, C] -> stats_out f32 [B, groups, 2] = (mean, 1 / sqrt(biased variance + 1e-5)).  One
 * workgroup per (batch element, chunk of ttk_cls_stats_rows(C) rows) writes a two-pass (count, mean, M2) per group to `part` (scratch of at least
 * B * ceil(L / ttk_cls_stats_rows(C)) * groups * 3 floats); a second launch merges the chunks in ascending order (Chan et al.).  No atomics: the
 * same bits on every run.  C and groups are powers of two. */
int ttk_cls_stats_rows(int C);
int ttk_cls_gn_stats(const float* x, int B, int L, int C, int groups, float* part, int64_t part_floats, float* stats_out, void* stream);

/* ------------------------------------------------------------------ CLVP candidate scoring
 * models/clvp.py:21-136 (x-transformers branch): weights = CLVP.state_dict() with each attention's to_q / to_k / to_v stacked into
 * "<attn>.__qkv.weight" [3 * dim, dim] and "__rotary_inv_freq" [16] (RotaryEmbedding(32).inv_freq), as tortoise_tts_amd/clvp.py packs. */
typedef struct ttk_clvp ttk_clvp;
typedef struct {
	int dim;                                  /* 768; heads * 64 == dim */
	int heads;                                /* 12 */
	int depth;                                /* 20 attention + 20 feed-forward layers per encoder */
	int inner;                                /* dim * ff_mult = 1536 */
	int num_text_tokens, num_speech_tokens;   /* 256, 8192 */
	int dtype;                                /* TTK_F32 | TTK_BF16 */
} ttk_clvp_config;
int ttk_clvp_create(ttk_clvp** out, const ttk_clvp_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_clvp_destroy(ttk_clvp* h);
/* CLVP.forward(text, speech_tokens, return_loss=False) :100-131: text [Bt, Tt] int64 with Bt == 1 (one line scored against every
 * candidate, what `text_tokens.repeat(B, 1)` at inference.py:394 amounts to) or Bt == B; codes [B, M] int64 -> scores [B] f32.  */
int ttk_clvp_score(ttk_clvp* h, const int64_t* text, int Bt, int Tt, const int64_t* codes, int B, int M, float* scores, void* stream);

/* ------------------------------------------------------------------ conditioning-latent encoders
 * One handle type for both: UnifiedVoice.conditioning_encoder (models/unified_voice.py:269-293: 1x1 conv 80 -> 1024, six AttentionBlocks of
 * 16 heads, output = position 0) and DiffusionTTS.contextual_embedder (models/diffusion.py:1441-1447: two k=3 stride-2 convs 100 -> 1024 ->
 * 2048, five AttentionBlocks of 16 heads x 128 with relative position bias; `get_conditioning` :1477-1485 takes the mean over positions).
 * Weights under module-relative names, as tortoise_tts_amd/conditioning.py packs them from the parents' state_dict():
 * "stem.{0,1}.weight" reshaped to [out, in * taps] and ".bias"; "blocks.{i}.norm|qkv|proj_out.weight|bias"; with relpos
 * "blocks.{i}.__relbias" [heads, 129] (the bias of clamp(k - q, -64, 64), already scaled by sqrt(head width), models/xtransformers.py:179-188). */
typedef struct ttk_cond ttk_cond;
enum { TTK_COND_STEM_CONV1 = 0, TTK_COND_STEM_DOWN4 = 1 };
typedef struct {
	int in_channels;      /* mel bands: 80 (AR) / 100 (diffusion) */
	int channels;         /* block width: 1024 / 2048; channels / num_heads must be 64 or 128 */
	int num_heads;
	int num_blocks;       /* 6 / 5 */
	int stem;             /* TTK_COND_STEM_CONV1: one 1x1 conv; TTK_COND_STEM_DOWN4: k=3 stride-2 padding-1 convs in -> channels/2 -> channels */
	int relpos;           /* blocks carry a relative position bias */
	int pool;             /* 0: position 0 (ConditioningEncoder mean=False); 1: mean over positions */
	int dtype;            /* TTK_F32 | TTK_BF16 */
} ttk_cond_config;
int ttk_cond_create(ttk_cond** out, const ttk_cond_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_cond_destroy(ttk_cond* h);
/* one clip per batch row: mel f32 [b, in_channels, T] (the reference's channels-first layout) -> out f32 [b, channels] */
int ttk_cond_encode(ttk_cond* h, const float* mel, int b, int T, float* out, void* stream);

/* ------------------------------------------------------------------ the dense GEMM kernel on caller-provided operands
 * C f32 [M, N] = out_scale * A [M, K] . W [N, K]^T + bias, operands in `dtype`: f32, bf16, or TTK_FP8 = fp8-e4m3 bytes on the fp8 MFMA (out_scale
 * then carries the tensor scale; 0 = none).  N % 128 == 0, K % 32 / 64 / 128 == 0.  No reference counterpart: exposed so the kernel behind every
 * conv / linear of both networks can be tested against a plain matmul of the same operands. */
int ttk_gemm_nt(int dtype, const void* A, const void* W, int M, int N, int K, float out_scale, const float* bias, float* C, void* stream);
/* Every form of the same kernel: the general descriptor, field for field what the networks' launches fill in (up to 12 segments -- row-shifted
 * taps of a convolution, a channel concatenation -- an activation, a residual that may alias C, 16-bit output, the transposed [b][N][rows_per_batch]
 * output and the fused GroupNorm32 statistics).  The tile and role choice is the one every product launch gets.
 *   C = epi( sum_s shift_s(A_s) [M, K] . W_s [N, K]^T ),  W_s = W + w_off_s elements, rows [0, round_up(N, 128)) of ldw elements readable;
 *   shift_s: row m reads A_s row m + shift_s if that stays inside m's batch element of rows_per_batch rows, else zeros;
 *   epi: x out_scale (0 = none), + bias [N], act (0 none, 1 gelu_new, 2 SiLU), + residual f32 [M][ldr] (out_f32 only), in that order;
 *   C: out_f32 ? f32 : the operand type (bf16 for TTK_FP8), [M][ldc]; transpose_out: f32 [M / rows_per_batch][N][rows_per_batch];
 *   gn_part (f32 C only): one (count, mean, M2) triple per (batch element of gn_T rows, group of 32 channels, 64-row chunk) of C,
 *   [ceil(M / gn_T)][32][gn_T / 64][3], only for the shapes whose tiles produce them (N == 1024, M and gn_T multiples of 64, not the 64-row tile).
 * Returns TTK_E_ARG with a message when a precondition the kernels rely on fails. */
typedef struct { const void* A; int64_t lda; int shift; int64_t w_off; } ttk_gemm_seg;
typedef struct {
	int nseg;
	ttk_gemm_seg seg[12];
	const void* W; int64_t ldw;
	int M, N, K;                              /* K per segment: % 32 (f32), % 64 (bf16 / f16), % 128 (fp8) */
	int rows_per_batch;                       /* > 0 when any shift != 0 or transpose_out */
	int act;
	const float* bias; const float* residual; int64_t ldr;
	void* C; int64_t ldc;
	float out_scale; int out_f32; int transpose_out;
	int gn_T; float* gn_part;
} ttk_gemm_desc;
int ttk_gemm(int dtype, const ttk_gemm_desc* d, void* stream);

/* ------------------------------------------------------------------ the attention kernels (head dim 64) on caller-provided operands
 * No reference counterpart: exposed so every launch form of csrc/attn.hip can be tested against a float64 softmax(q k^T) v of the same operands.
 * ttk_attn_fwd: out[b][q][h*64 + d] = sum_k softmax_k(scale * q.k + bias[h][clamp(k - q, -64, 64) + 64]) v_k over keys k < tlen[b] (k <= q when causal),
 *   for queries q < tlen[b] of sequence b, which occupies rows [b*T, b*T + T) of qkv [nb*T][ld] and of out [nb*T][ldo]; element (h, d) of q / k / v is
 *   column q_off / k_off / v_off + h * head_stride + d.  dtype: TTK_F32, TTK_BF16 or TTK_F16 (qkv and out; out_f8, bf16 only: out is fp8-e4m3 bytes).
 *   tlen: null (every sequence has T rows) or device int [nb], each 1..T.  bias: null or device f32 [H][129]; not together with causal.
 *   form: 0 = the launcher's own choice from nb x H x T (what every product launch gets), 1 = 64-query blocks, 2 = 128-query blocks,
 *   3 = 8 waves x 16 queries (non-causal), 4 = balanced (non-causal, no tlen, 256 % (nb*H) == 0, at most 9 16-query tiles per workgroup).
 * ttk_attn_decode: one query per (candidate, head) over the cache rows [start, min(d_pos[0] + 1, max_ctx)): qbuf f32 [B][H*64] (already scaled),
 *   kcache / vcache dtype [B][H][max_ctx][64], d_pos device int[2] = {last valid row, rows of the shared prefix}, out dtype [B][H*64] or (out_frag) the
 *   skinny GEMV's fragment order [ceil(B / 16)][H*2][64][8].  row_info: null or device int [B][2] = {start, first candidate of b's line}.
 *   shared_rows != 0: rows [start, d_pos[1]) are read from the first candidate's slice (candidate 0 without row_info).
 *   variant: 0 = default, 1 = 4 waves x 4 groups, 2 = 8 x 6 (1 and 2: bf16 only).  pos_line != 0: the two words travel through a slot of the position
 *   line (copied there on `stream`; refused when all 8 slots are taken).
 * Both return TTK_E_ARG with a message when a precondition the kernels rely on fails. */
typedef struct {
	const void* qkv; int64_t ld;
	int q_off, k_off, v_off, head_stride;
	void* out; int64_t ldo;
	int out_f8;
	int nb, T, H, causal;
	const int* tlen;
	const float* bias;
	float scale;
	int form;
} ttk_attn_desc;
int ttk_attn_fwd(int dtype, const ttk_attn_desc* d, void* stream);
typedef struct {
	const float* qbuf; const void* kcache; const void* vcache; const int* d_pos;
	int B, H, max_ctx, out_frag;
	void* out;
	const int* row_info;
	int shared_rows, variant, pos_line;
} ttk_attn_decode_desc;
int ttk_attn_decode(int dtype, const ttk_attn_decode_desc* d, void* stream);

/* ------------------------------------------------------------------ attention maps, alignment cost and DTW on caller-provided operands (csrc/align.hip)
 * ttk_attn_probs: the causal softmax probabilities HF's eager GPT-2 attention returns with output_attentions (HF:models/gpt2/modeling_gpt2.py:144-226; reached by
 *   get_logits(get_attns=True), unified_voice.py:508-516), which ttk_attn_fwd never materialises.  qkv [nb*T][ld] is addressed as ttk_attn_desc addresses it; head dim 64.
 *   out f32 [nb][n_sel][R][C]: rows [r0, r0 + R) and columns [c0, c0 + C) of the T x T map of head heads[i] (device int [n_sel], each in [0, H); an entry
 *   outside is skipped), P[q][k] = softmax over k' <= q of scale q.k', 0 for k > q.  The full map is the window (0, T, 0, T); a window's elements are bit for
 *   bit the full map's.  n_sel == 0 launches nothing.
 * ttk_align_prepare: the alignment cost of per-head blocks A f32 [nb][n_sel][M][Tt] (no reference counterpart; the word-timestamp recipe of OpenAI Whisper,
 *   whisper/timing.py, with mel codes as the time axis): every row standardised over the text axis (population std; a row of std 0 becomes zeros), a median
 *   filter of odd `width` <= 15 along M with reflect padding (M <= width / 2: no filter), the mean over the heads as sequential f32 adds in list order and one
 *   division; cost f32 [nb][M][Tt] = -mean, matrix (optional, same shape) = mean.
 * ttk_dtw: D[0][0] = 0, borders +inf, D[i][j] = cost[i-1][j-1] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) in f32, on ties the first of (diagonal, i-1, j-1);
 *   D f32 [nb][(M+1)(Tt+1)] is the caller's workspace, trace u8 [nb][M][Tt] holds 0 / 1 / 2 for the three, total f32 [nb] = D[M][Tt].  The path is read
 *   from the trace on the host.  M <= 606, Tt <= 404 (max_mel_tokens + 2, max_text_tokens + 2 of the largest configuration) in both.
 * All three return TTK_E_ARG with a message when a precondition the kernels rely on fails. */
typedef struct {
	const void* qkv; int64_t ld;
	int q_off, k_off, head_stride, nb, T, H;
	float scale;
	int n_sel;
	const int* heads;
	float* out;
	int r0, R, c0, C;
} ttk_attn_probs_desc;
int ttk_attn_probs(int dtype, const ttk_attn_probs_desc* d, void* stream);
int ttk_align_prepare(const float* A, int nb, int n_sel, int M, int Tt, int width, float* cost, float* matrix, void* stream);
int ttk_dtw(const float* cost, int nb, int M, int Tt, float* D, unsigned char* trace, float* total, void* stream);

/* ------------------------------------------------------------------ the GroupNorm32-apply kernels on caller-provided operands
 * No reference counterpart: exposed so every launch form of csrc/norm.hip's GroupNorm-apply can be run on the same input and statistics (the forms owe the same
 * bits: tests/test_gpu_gn_forms.py) and so the generic form and the chunk statistics can be held, element by element, to a float64 GroupNorm of the same operands
 * (tests/test_gpu_norm_forms.py with tests/norm_ref.py).
 * out [nb][Tout][C] = act( gn(x) * gamma + beta [ * (1 + scale[b]) + shift[b] ] ) over x f32 [nb][T][C], 32 groups; C = 128, 256, 512 or 1024.
 *   ms: f32 [nb][32][ceil(T / (65536 / C))][3] chunk statistics (count, mean, M2); stats != 0: computed from x by this call first, else read as the caller left them.
 *   scale / shift: null or f32 rows ss_stride apart per batch element (0: shared).  row_idx: null (Tout == T) or device int [Tout] into [0, T).
 *   tlen: null or device int [nb], each 1..T (needs Tout == T, no row_idx): rows past tlen[b] are written as zeros, the statistics cover the rows before.
 *   out: out_f8 ? fp8-e4m3 bytes (TTK_BF16 only) : out_f32 ? f32 : dtype.  act: 0 none, 2 SiLU.  pf: null or pf_taps blocks of pf_bytes each, touched into L2.
 *   x, gamma, beta, scale, shift and out 16-byte aligned, ss_stride % 4 == 0, at most 64 chunks.
 *   form: 0 = the launcher's own choice (what every product launch gets), 1 = generic, 2 = 4-row strips (C == 1024, no row_idx), 3 / 4 / 5 = rows dealt evenly over
 *   256 / nb strips of 4 .. 9 / 12 / 18 rows (as 2, and no tlen, nb <= 64; 3 and 4: at most 24 chunks).
 * Returns TTK_E_ARG with a message when a precondition the kernels rely on fails. */
typedef struct {
	const float* x; float* ms; const float* gamma; const float* beta;
	const float* scale; const float* shift; int64_t ss_stride;
	const int* row_idx; const int* tlen;
	int nb, T, Tout, C, act;
	void* out; int out_f32, out_f8;
	const void* pf; int64_t pf_bytes; int pf_taps;
	int stats, form;
} ttk_gn_desc;
int ttk_gn_apply(int dtype, const ttk_gn_desc* d, void* stream);

/* ------------------------------------------------------------------ the LayerNorm kernel on caller-provided operands
 * No reference counterpart: exposed so both instantiations of csrc/norm.hip's k_layernorm (d <= 1024 and d <= 4096) can be tested against a float64 LayerNorm of
 * the same operands, element by element (tests/test_gpu_norm_forms.py with tests/norm_ref.py).
 * out[r] = LN(x[r]; g1, b1), then optionally LN(.; g2, b2) on top, over rows r < rows of x f32 [rows][ldx], d columns each, eps 1e-5.
 *   out: out_f32 ? f32 : dtype (TTK_F32, TTK_BF16 or TTK_F16); row-major [rows][ldo], or (frag != 0) the skinny GEMV's A-fragment order
 *   [ceil(rows / 16)][d / 32][64][8] (ldo unused; rows >= `rows` of the last tile are not written).
 *   out2: null or f32 [rows][d], a second, row-major copy of the result.  out2_idx: null or device int64[1]: the copy goes to out2 + out2_idx[0] * out2_stride
 *   (a ring slot, out2_stride in floats).  out2_base: null or device int64[1] holding the address that replaces out2 (read at launch time on the device).
 *   d % 4 == 0 and 4 <= d <= 4096 (frag: d % 32 == 0); ldx >= d, ldx % 4 == 0; ldo >= d; x, g1, b1, g2, b2 and out2 16-byte aligned; out2_stride % 4 == 0.
 * Returns TTK_E_ARG with a message, and launches nothing, when a precondition the kernel relies on fails. */
typedef struct {
	const float* x; int64_t ldx;
	int rows, d;
	const float* g1; const float* b1; const float* g2; const float* b2;
	void* out; int64_t ldo;
	int out_f32, frag;
	float* out2; const int64_t* out2_idx; int64_t out2_stride; const int64_t* out2_base;
} ttk_ln_desc;
int ttk_layernorm_rows(int dtype, const ttk_ln_desc* d, void* stream);

/* ------------------------------------------------------------------ the vocoders' own kernels on caller-provided operands
 * No reference counterpart: exposed so the location-variable convolution (csrc/univnet.hip: k_lvc, k_lvc_mfma), the narrow-channel MFMA convolution with its
 * weight packing (csrc/hifigan.hip: k_hifi_conv_mfma, k_hifi_pack_frag) and the anti-aliased snake activation (csrc/voc.hip: k_snake_aa) can be held, element by
 * element, to a float64 reference of the same operands (tests/test_gpu_voc_forms.py with tests/voc_ref.py).  Each goes through the launcher its handle uses.
 * All three return TTK_E_ARG with a message, and launch nothing, when a precondition the kernel relies on fails.
 *
 * ttk_lvc_rows: one LVC layer with its gated update over B sequences of L rows, CG = 16 or 32 channels, dtype TTK_F32 | TTK_BF16 (T):
 *     o[t][n] = kbias[f][layer][n] + sum_i sum_k lrelu_0.2(y)[t + k - 1][i] kern[f][layer][i][n][k],   f = t / hop, rows outside [0, L) of a sequence zero
 *     x[t][c] += sigmoid(o[t][c]) tanh(o[t][c + CG]);   at[t][c] = T(lrelu_0.2(x[t][c]))
 *   y f32 [B * L][CG]; kern T [B * Tc][kstride], kstride = n_layers * CG * 2 CG * 3; kbias f32 [B * Tc][bstride], bstride = n_layers * 2 CG; x f32 [B * L][CG],
 *   updated in place; at T [B * L][lda] (columns CG .. lda are not written).  1 <= hop, ceil(L / hop) <= Tc, 0 <= layer < n_layers <= 4, lda >= CG, B <= 65535;
 *   x and at overlap neither each other nor an input.  TTK_BF16 with CG = 32 runs k_lvc_mfma (which rounds lrelu(y) to bf16), everything else k_lvc.          */
typedef struct {
	const float* y; const void* kern; const float* kbias;
	float* x; void* at;
	int B, L, CG, hop, Tc, layer, n_layers, lda;
} ttk_lvc_desc;
int ttk_lvc_rows(int dtype, const ttk_lvc_desc* d, void* stream);
/* ttk_hifi_conv_rows: one 'same' dilated Conv1d C -> C (C = 32 or 64, bf16 operands, f32 accumulation) over one sequence of L rows with its fused epilogue:
 *     v[t][n] = bias[n] + sum_k sum_i a[t + (k - (K - 1) / 2) dil][i] bf16(w[n][i][k])      rows outside [0, L) zero
 *     mode 0: at_out = bf16(lrelu_0.1(v));   1: xout = v + xres, at_out = bf16(lrelu_0.1(xout));   2: mrf = v + xres;   3: mrf += v + xres
 *   a bf16 [L][lda], lda >= C, lda % 8 == 0, 16-byte aligned; w f32 [C][C][k] (Conv1d's layout, on the device; packed by this call the way ttk_hifigan_create
 *   packs it: to bf16 [k][Npad][Kpad], then to B-fragment order), bias f32 [C]; k odd in 1..11, dil >= 1, and the weights plus the 256-row window with its halo
 *   within 160 KiB of LDS.  xres, xout, mrf f32 [L][C], at_out bf16 [L][ldo] (ldo >= C; columns C .. ldo are not written): each is required in the modes that read
 *   or write it and ignored in the others.  xres == xout is allowed; at_out, xout and mrf must not overlap a, xout and mrf must not overlap xres otherwise.
 *   The call synchronises `stream` and frees the packed weights before it returns.                                                                         */
typedef struct {
	const void* a; int lda;
	const float* w; const float* bias;
	int L, C, k, dil, mode;
	const float* xres; float* xout; void* at_out; int ldo; float* mrf;
} ttk_hifi_conv_desc;
int ttk_hifi_conv_rows(const ttk_hifi_conv_desc* d, void* stream);
/* ttk_snake_rows: Activation1d with SnakeBeta over x f32 [B * L][C] -> y T [B * L][C] (dtype TTK_F32 | TTK_BF16): 2x up-sampling with the 12-tap low-pass filt12
 * (replicate padding, gain 2), z = up + invb sin(up a)^2, low-pass and decimation by 2 (replicate padding).  a, invb f32 [C] as the kernel reads them (already
 * exponentiated; invb = 1 / (b + 1e-9)), filt12 f32 [12].  C % 4 == 0, x, a, invb 16-byte aligned, x and y do not overlap.                               */
int ttk_snake_rows(int dtype, const float* x, int B, int L, int C, const float* a, const float* invb, const float* filt12, void* y, void* stream);

/* ------------------------------------------------------------------ the side networks' own kernels on caller-provided operands
 * No reference counterpart: exposed so the kernels of the conditioning encoders, the classifier's AttentionBlocks and CLVP that the hot path does not share
 * (csrc/ttk_attn_block.h: k_cond_gn, k_attn_rowwave; csrc/cond.hip: k_cond_im2col, k_cond_pool; csrc/clvp.hip: k_embed_rows, k_rmsnorm, k_rotary, k_geglu,
 * k_mean_rows, k_clvp_score) can be held, element by element, to a float64 reference of the same operands (tests/test_gpu_side_forms.py with tests/side_ref.py).
 * Each goes through the launch function its handle uses.  dtype (T) is TTK_F32 | TTK_BF16.  Every one returns TTK_E_ARG with a message, and launches nothing, when
 * a precondition its kernel relies on fails.
 *
 * ttk_block_gn_rows: out T [nb][T][C] = gn(x) gamma + beta over x f32 [nb][T][C], `groups` groups of C / groups channels (any width), two-pass biased variance,
 *   eps 1e-5.  C % groups == 0, nb <= 65535.
 * ttk_attn_rowwave: ttk_attn_fwd's operation for head width 128 (out column h * 128 + d), one wave per query row, f32 arithmetic with the scores of a row in LDS:
 *   1 <= T <= 3584.  The descriptor is ttk_attn_desc; causal, tlen, out_f8 and form must be 0 / null.  head_stride >= 128, every head inside ld, ldo >= H * 128;
 *   qkv aligned to 8 elements, ld, k_off and head_stride multiples of 8 (k is read 8 elements at a time); qkv and out do not overlap.
 * ttk_cond_im2col_rows: out T [nb * Tout][Kpad], out[(b, t)][c * taps + j] = src[b * sb + c * sc + (t * stride + j - pad) * st] where that position lies in
 *   [0, Tin), else 0; columns Cin * taps .. Kpad are zeros.  src f32 with element strides (sb, sc, st): channels-first or channels-last.  Kpad >= Cin * taps.
 * ttk_cond_pool_rows: out f32 [nb][C] = row 0 (mode 0) or the mean over the T rows, added in rising t and divided once (mode 1), of x f32 [nb][T][C].             */
int ttk_block_gn_rows(int dtype, const float* x, int nb, int T, int C, int groups, const float* gamma, const float* beta, void* out, void* stream);
int ttk_attn_rowwave(int dtype, const ttk_attn_desc* d, void* stream);
int ttk_cond_im2col_rows(int dtype, const float* src, int64_t sb, int64_t sc, int64_t st, int nb, int Cin, int Tin, int Tout, int taps, int stride, int pad, int Kpad,
						 void* out, void* stream);
int ttk_cond_pool_rows(const float* x, int nb, int T, int C, int mode, float* out, void* stream);
/* ttk_clvp_embed_rows: out f32 [B * S][d] = emb[clamp(ids[b * batch_stride_ids + t], 0, vocab - 1)], emb f32 [vocab][d]; d % 64 == 0, batch_stride_ids >= S, emb and
 *   out 16-byte aligned.
 * ttk_clvp_rmsnorm_rows: y T [rows][d] = x / max(|x| d^-1/2, 1e-8) g over x f32 [rows][d] (a zero row gives zeros); d % 64 == 0, x and g 16-byte aligned.
 * ttk_clvp_rotary_rows: the rotary embedding IN PLACE on features 0..31 of every head of q, k and v of qkv T [B * S][3 * H * 64]: for i < 16,
 *   (x_i, x_{i+16}) -> (x_i cos a - x_{i+16} sin a, x_{i+16} cos a + x_i sin a), a = (row % S) inv_freq[i], inv_freq f32 [16]; features 32..63 are not touched.
 * ttk_clvp_geglu_rows: out T [rows][inner] = h[r][c] gelu(h[r][inner + c]) over h T [rows][2 * inner], gelu exact (erf); h and out do not overlap.
 * ttk_clvp_mean_rows: out T [B][d] = the mean over the S rows of x f32 [B][S][d], added in rising t and divided once; d % 64 == 0.
 * ttk_clvp_latent_score: scores f32 [B] = <t, s_b> / (max(|t|, 1e-12) max(|s_b|, 1e-12)) exp(temperature[0]), t = text_latents row 0 (Bt == 1) or b (Bt == B),
 *   latents f32 [.][d], temperature device f32 [1]; d % 64 == 0.                                                                                              */
int ttk_clvp_embed_rows(const float* emb, int vocab, int d, const int64_t* ids, int B, int S, int batch_stride_ids, float* out, void* stream);
int ttk_clvp_rmsnorm_rows(int dtype, const float* x, int64_t rows, int d, const float* g, void* y, void* stream);
int ttk_clvp_rotary_rows(int dtype, void* qkv, int B, int S, int H, const float* inv_freq, void* stream);
int ttk_clvp_geglu_rows(int dtype, const void* h, int64_t rows, int inner, void* out, void* stream);
int ttk_clvp_mean_rows(int dtype, const float* x, int B, int S, int d, void* out, void* stream);
int ttk_clvp_latent_score(const float* text_latents, int Bt, const float* speech_latents, int B, int d, const float* temperature, float* scores, void* stream);

/* ------------------------------------------------------------------ the weight-streaming decode launches on caller-provided operands
 * No reference counterpart: exposed so every launch form of csrc/skinny.hip (k_skinny) and csrc/gemv.hip (k_gemv) can be tested against a float64
 * LN(x) W^T + b of the same operands, element by element (tests/test_gpu_skinny_forms.py).
 * ttk_gemv_mat: ONE decode matrix, uploaded and packed by the very functions ttk_ar_create uses (fragment order, fp8 rounding, and -- when "gamma" and "beta"
 *   are among the weights -- the folded-LayerNorm operands gamma o W, its column sums and b + beta W).  Weights by name: "weight" f32 [N][K] (layout 0,
 *   nn.Linear as mel_head has it) or [K][N] (layout 1, HF Conv1D), "bias" [N], optional "gamma" / "beta" [K].  K % 64 == 0.  dtype as ttk_ar_config
 *   (TTK_FP8W: fp8 weights under bf16 arithmetic, the fold kept in bf16).
 * ttk_gemv_launch: one launch over M rows.
 *   role: 0 qkv (q pre-scaled to qbuf f32 [M][K], k / v appended to the caches [M][H][max_ctx][64] at row d_pos[0] when that is < max_ctx; N == 3K, K == 64 H),
 *         1 proj (out_f32 [M][N] += the product, in place; out_T optional: the updated rows in fragment order), 2 fc (out_T = gelu_new, fragment order),
 *         3 head (out_f32 [M][N]; noise / rng / draws as ttk_ar_set_noise; bump != 0: d_pos[0] += 1).
 *   form: 0 plain (a = rows of `dtype` in A-fragment order [ceil16(M) / 16][K / 32][64][8], proj and head only), 1 folded LayerNorm over the UN-normalised rows
 *         `a` (qkv and fc, a matrix created with gamma / beta; health optional: the word ttk_ar_health reads), 2 LayerNorm prologue over f32 rows x [M][K] with
 *         (g1, b1) and then optionally (g2, b2) (qkv, fc, head; at most 32 rows outside the head).
 *   `a` and `out_T` hold every row of the 1, 2, 3 or 4 sixteen-row tiles the launch is instantiated for (ttk_ar_decode_geometry); rows >= M of `a` are never
 *   allowed to reach a live output, rows >= M of out_T are never written.
 *   family: 0 = what the decode step chooses (the same code decides), 1 = k_skinny, 2 = k_gemv (refused where it has no instantiation).
 *   waves: 0 = the decode step's choice, else 4..16 waves per k_skinny workgroup (at most 8 in form 2).
 *   model_dim: the width of the model the matrix belongs to, which the decode step's waves choice depends on; 0 = N for proj, K otherwise -- right for every
 *   matrix but mlp.c_proj (N x 4N: pass N) and test matrices whose N is not the model's width.  With it, family 0 / waves 0 is what the decode step runs.
 *   launched (optional, HOST int): receives the family that ran, 1 or 2.
 * Returns TTK_E_ARG with a message, and launches nothing, when a precondition the kernels rely on fails -- including a launch whose LDS exceeds a compute unit's. */
typedef struct ttk_gemv_mat ttk_gemv_mat;
typedef struct { int dtype, layout, N, K; } ttk_gemv_mat_config;
int ttk_gemv_mat_create(ttk_gemv_mat** out, const ttk_gemv_mat_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_gemv_mat_destroy(ttk_gemv_mat* h);
typedef struct {
	int dtype, role, form, M;                 /* dtype: the arithmetic type of a / out_T / the caches: what the matrix was created for (TTK_BF16 for TTK_FP8W) */
	const void* a; const float* x;
	const float *g1, *b1, *g2, *b2;
	float* out_f32; void* out_T;
	float* qbuf; void* kcache; void* vcache;
	int max_ctx, H; float q_scale; int bump;  /* q_scale: must be 0.125 (head dim 64), the one value the decode step uses */
	int* d_pos;
	float* noise; const int64_t* rng; const int64_t* draws;
	int* health;
	int* launched;
	int family, waves, model_dim;
} ttk_gemv_desc;
int ttk_gemv_launch(const ttk_gemv_mat* W, const ttk_gemv_desc* d, void* stream);

/* ------------------------------------------------------------------ mel front-ends of the conditioning path
 * TorchMelSpectrogram (models/arch_utils.py:361-395) and TacotronSTFT (:662-700 over STFT :560-623) as one handle type: reflect-padded
 * frames x "basis" [2 * (n_fft/2 + 1), n_fft] (windowed DFT, Re rows then Im rows) -> |.|^power -> x "mel_basis" [n_mels, n_fft/2 + 1] ->
 * log(max(., 1e-5)) [/ "mel_norms" [n_mels]].  tortoise_tts_amd/mel.py builds the matrices; arithmetic is f32 throughout. */
typedef struct ttk_mel ttk_mel;
typedef struct {
	int n_fft;            /* 1024; multiple of 64; window length == n_fft */
	int hop;              /* 256 */
	int n_mels;           /* 80 (AR side, 22.05 kHz) / 100 (diffusion side, 24 kHz) */
	int power;            /* 2: power spectrogram (TorchMelSpectrogram); 1: magnitude (TacotronSTFT) */
	int clip;             /* clamp samples to [-1, 1] first (TacotronSTFT.mel_spectrogram :694) */
	int has_norms;        /* divide band m of the log-mel by mel_norms[m] (:392-394) */
} ttk_mel_config;
int ttk_mel_create(ttk_mel** out, const ttk_mel_config* cfg, const ttk_weight_view* weights, int n_weights);
int ttk_mel_destroy(ttk_mel* h);
/* wav f32 [b, n] (n > n_fft / 2) -> mel f32 [b, n_mels, n / hop + 1] */
int ttk_mel_forward(ttk_mel* h, const float* wav, int b, int n, float* mel, void* stream);
/* torchaudio.functional.resample's polyphase FIR (emb/mel.py:67,86 resample clips to 22.05 kHz and 22.05 -> 24 kHz): rates reduced by their
 * gcd to gorig -> gnew; kernels f32 [gnew, 2 * width + gorig] on the device (tortoise_tts_amd/mel.py builds the windowed-sinc table);
 * wav f32 [b, n] -> out f32 [b, n_out], n_out = ceil(gnew * n / gorig).  Stateless. */
int ttk_resample_fir(const float* wav, int b, int n, const float* kernels, int gorig, int gnew, int width, float* out, int n_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
