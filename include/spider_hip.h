/* spider_hip.h -- C ABI of libspider_hip.so: the MI355X (gfx950) kernels behind Spider's any-to-many
 * generation hot path (LLM greedy decode + SD/StoryDiffusion UNet step).
 *
 * The reference (Layjins/Spider) has no FFI: every operator below replaces a PyTorch-level op sequence,
 * cited as <file>:<lines> relative to the reference tree. A maintainer binds these with ctypes (see
 * INTEGRATION.md); spider_amd/lib.py is that binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named host_*; bf16 tensors are raw uint16 bit patterns
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work, they never synchronise,
 *     allocate or free, so they can be captured into a hipGraph
 *   - return 0 on success, <0 on error; spider_last_error() (thread-local) holds the message
 *   - all reductions accumulate in fp32; outputs are rounded to bf16 where the reference's bf16 module
 *     would round (documented per function)
 */
#ifndef SPIDER_HIP_H
#define SPIDER_HIP_H
#define SPIDER_ABI_VERSION 4   /* 2: w_tiled argument of the GEMM / conv entry points; *_f16 instantiations
                                * 3: producer-side GroupNorm statistics (spider_conv_nhwc_gn, spider_groupnorm_stats / _apply, spider_gemm_gn_in)
                                * 4: w_tiled = 2 (fragment-major conv weights, in-launch split-K combine); the "precise" fp32-operand forms
                                *    (spider_gemm_a32, spider_gemm_gn_in_a32, spider_conv_nhwc_a32, spider_groupnorm_f32in_nhwc,
                                *    spider_conv2d_small_c{in,out}_f32in, spider_latent_to_nhwc_f32); act 9 = GEGLU rounded once */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library identity / errors ---- */
int spider_abi_version(void);
const char* spider_target_arch(void);
const char* spider_last_error(void);

/* ======================= LLM decode path (HBM-bound) ======================= */

/* nn.Embedding lookup: out[r,:] = table[ids[r],:]   (base_model.py:253-258 embed_tokens) */
int spider_embed_bf16(const void* table, const int* ids, void* out, int rows, int H, int V, void* stream);

/* LlamaRMSNorm (modeling_llama3.py:68-82; modeling_llama.py:57-74) with optional fused residual add
 * (decoder-layer wiring modeling_llama3.py:339-361): h = x (+ res); res_out = h; y = w * bf16(h*rsqrt(mean(h^2)+eps)) */
int spider_rmsnorm_bf16(const void* x, const void* res, const void* w, void* y, void* res_out, int rows, int H,
                        float eps, void* stream);

/* nn.Linear at decode (1..8 tokens): out[b,n] = sum_k xin[b,k] W[n,k] (+bias[n]) (+res[b,n]);
 * xin = RMSNorm(x)*norm_w when norm_w != NULL (fused prologue).  q/k/v/o_proj, down_proj:
 * modeling_llama3.py:186-199,240-313 */
int spider_gemv_bf16(const void* W, const void* x, void* out, const void* bias, const void* res, const void* norm_w,
                     float eps, int B, int N, int K, void* stream);

/* LlamaMLP gate/up + SiLU*mul (modeling_llama3.py:197-199): W_gate_up = [gate rows (I) | up rows (I)] x K */
int spider_gemv_swiglu_bf16(const void* W_gate_up, const void* x, void* out, const void* norm_w, float eps, int B,
                            int I, int K, void* stream);

/* Weight-only FP8 forms of the two calls above for 1 <= B <= 4 (csrc/gemv_wq.hip): Wq [N, K] bytes in OCP e4m3fn (448 = 0x7e,
 * 1.0 = 0x38; not MI300's fnuz), scale [N] fp32 per weight row, K % 16 == 0:
 *   out[b,n] = epilogue(scale[n] * sum_k xin[b,k] * f32(Wq[n,k]))
 * with the prologue (fused RMSNorm, normalised activation rounded to bf16) and the epilogue (+bias -> bf16 -> +res -> bf16) of
 * spider_gemv_bf16. The fp32 sum is scaled once, after the reduction. The fused RMSNorm needs the staged
 * activations, B * ceil(K / 1024) * 2 KiB, within the LDS of a CU (160 KiB less 256 bytes).
 * K % 16, B in 1..4 and null Wq / scale / x / out are refused (-1) before any launch. */
int spider_gemv_w8(const void* Wq, const float* scale, const void* x, void* out, const void* bias, const void* res,
                   const void* norm_w, float eps, int B, int N, int K, void* stream);
/* Wq_gate_up [2 I, K] = [gate rows | up rows], scale [2 I]; out[b,i] = bf16(bf16(silu(bf16(g))) * bf16(u)) */
int spider_gemv_swiglu_w8(const void* Wq_gate_up, const float* scale, const void* x, void* out, const void* norm_w, float eps,
                          int B, int I, int K, void* stream);

/* Weight-only MXFP4 (OCP Microscaling FP4) forms of the same two calls for 1 <= B <= 4 (csrc/gemv_wq.hip), K % 32 == 0:
 *   blocks [N, K / 2] bytes, row-major: byte j of row n holds weight 2 j in its low nibble and weight 2 j + 1 in its high nibble; a
 *          nibble code c has sign bit 3 and magnitude {0, .5, 1, 1.5, 2, 3, 4, 6}[c & 7] (e2m1)
 *   scales [N, K / 32] bytes, row-major, E8M0: weights 32 g .. 32 g + 31 of row n are multiplied by 2^(scales[n, g] - 127); bytes 1..254
 *   out[b,n] = epilogue(sum_k xin[b,k] * W_eff[n,k])
 * with the prologue and the epilogue of spider_gemv_bf16. The block scale is applied inside the conversion to bf16, which is exact.
 * The fused RMSNorm needs the staged activations, B * ceil(K / 2048) * 4 KiB, within the LDS of a CU (160 KiB less 256 bytes).
 * K % 32, B in 1..4 and null blocks / scales / x / out are refused (-1) before any launch. */
int spider_gemv_w4(const void* blocks, const void* scales, const void* x, void* out, const void* bias, const void* res,
                   const void* norm_w, float eps, int B, int N, int K, void* stream);
/* blocks_gate_up [2 I, K / 2] = [gate rows | up rows], scales [2 I, K / 32]; out[b,i] = bf16(bf16(silu(bf16(g))) * bf16(u)) */
int spider_gemv_swiglu_w4(const void* blocks_gate_up, const void* scales, const void* x, void* out, const void* norm_w, float eps,
                          int B, int I, int K, void* stream);

/* Fragment-major weight-only forms for 1 <= B <= 16 rows (csrc/gemv_qfm.hip): the weight decode sits in front of the MFMA of
 * spider_gemv_fm_bf16, the activation rows are its B operand. No fused RMSNorm: x is used as it is.
 *   _w4: qfm [ceil(N/16), K/128, 64, 16] bytes, efm [ceil(N/16), K/128, 16, 4] bytes, K % 128 == 0. In piece (rg, kb) byte 4 sx + j of
 *        lane 16 g + r is blocks[16 rg + r][(128 kb + 32 sx + 8 g) / 2 + j] and efm byte (r, sx) is scales[16 rg + r][4 kb + sx], in
 *        the terms of spider_gemv_w4; padding rows hold nibble code 0 and scale byte 127.
 *   _w8: qfm [ceil(N/16), K/64, 64, 16] bytes, K % 64 == 0: byte 8 sx + e of lane 16 g + r is Wq[16 rg + r][64 kb + 32 sx + 8 g + e];
 *        scale [N] fp32 as in spider_gemv_w8, applied once to the fp32 sum.
 * Epilogues as spider_gemv_w4 / _w8: (+bias) -> bf16 -> (+res -> bf16); the swiglu forms take the copy of [gate rows | up rows]
 * (I % 16 == 0; scale [2 I]) and give bf16(bf16(silu(bf16(g))) * bf16(u)). K, B outside 1..16, I % 16 and null pointers are refused
 * (-1) before any launch. */
int spider_gemv_fm_w4(const void* qfm, const void* efm, const void* x, void* out, const void* bias, const void* res, int B, int N,
                      int K, void* stream);
int spider_gemv_swiglu_fm_w4(const void* qfm_gate_up, const void* efm, const void* x, void* out, int B, int I, int K, void* stream);
int spider_gemv_fm_w8(const void* qfm, const float* scale, const void* x, void* out, const void* bias, const void* res, int B, int N,
                      int K, void* stream);
int spider_gemv_swiglu_fm_w8(const void* qfm_gate_up, const float* scale, const void* x, void* out, int B, int I, int K, void* stream);

/* final norm + lm_head + greedy argmax (modeling_llama3.py:619,870-871; HF greedy loop driven from
 * spider.py:1492-1508). logits (bf16 [B,V]) optional. ws_val/ws_idx: B*spider_lm_head_nparts(V) floats/ints. */
int spider_lm_head_nparts(int V);

/* End of one greedy decode step (the bookkeeping of GenerationMixin's loop, spider.py:1492-1508, kept on the device so that the
 * step is one hipGraph): cur_ids <- next_ids; pos, slot, kv_end += 1; hist[b][n_hist[b]++] = next_ids[b]. int32 [B] each; hist
 * [B, cap] / n_hist [B] optional (both NULL: cursors only); entries past cap are dropped, the counter still advances. */
int spider_decode_advance_i32(const int* next_ids, int* cur_ids, int* pos, int* slot, int* kv_end, int* hist, int* n_hist,
                              int cap, int B, void* stream);
int spider_lm_head_argmax_bf16(const void* W, const void* x, const void* norm_w, float eps, int* out_ids, void* logits,
                               void* ws_val, void* ws_idx, int B, int V, int K, void* stream);

/* Greedy decode with HF's deterministic logits processors (transformers generation/logits_process.py: RepetitionPenalty,
 * SuppressTokens / single-token NoBadWords, MinLength / MinNewTokensLength; the reference passes repetition_penalty and
 * min_length, spider.py:1471-1508, conversation.py:151-172). The *_proc forms of the two lm_head entry points apply, to the
 * bf16-rounded logit widened to fp32 and before the arg-max:
 *   bit n of seen[b] set: lv = lv < 0 ? lv * p : lv / p (IEEE fp32);  bit n of ban[b] set: -inf;
 *   n one of the n_eos[0] (<= 8) ids of eos_ids while n_hist[b] < min_new[0]: -inf.
 * Ties and an all -inf row go to the lowest id. logits (optional) stay the RAW bf16 logits. seen / ban: uint32 [B, ceil(V/32)];
 * penalty float [1]; min_new, n_eos int32 [1]; eos_ids int32 [8]; n_hist int32 [B] -- all in device memory, read when the
 * kernel runs (a captured graph serves requests with different values). */
int spider_lm_head_argmax_proc_bf16(const void* W, const void* x, const void* norm_w, float eps, int* out_ids, void* logits,
                                    void* ws_val, void* ws_idx, const void* seen, const void* ban, const float* penalty,
                                    const int* min_new, const int* eos_ids, const int* n_eos, const int* n_hist, int B, int V,
                                    int K, void* stream);
/* Weight-only FP8 / MXFP4 forms of the two row-major lm_head entry points above for 1 <= B <= 4 (csrc/lm_head_wq.hip): the same
 * final norm, bf16-rounded logits, processors, tie rule, logits output and workspaces, with the vocabulary matrix streamed as
 *   _w8: q [V, K] OCP e4m3fn bytes and scale [V] fp32 (layout of spider_gemv_w8), K % 16 == 0;
 *   _w4: blocks [V, K / 2] e2m1 nibbles and scales [V, K / 32] E8M0 bytes (layout of spider_gemv_w4), K % 32 == 0.
 * The fused RMSNorm (norm_w != NULL) needs the staged activations within the LDS budget of spider_gemv_w8 / _w4. K, B in 1..4,
 * null q / scale / x / out_ids / workspaces and a fused norm beyond the budget are refused (-1) before any launch. */
int spider_lm_head_argmax_w8(const void* q, const void* scale, const void* x, const void* norm_w, float eps, int* out_ids,
                             void* logits, void* ws_val, void* ws_idx, int B, int V, int K, void* stream);
int spider_lm_head_argmax_proc_w8(const void* q, const void* scale, const void* x, const void* norm_w, float eps, int* out_ids,
                                  void* logits, void* ws_val, void* ws_idx, const void* seen, const void* ban,
                                  const float* penalty, const int* min_new, const int* eos_ids, const int* n_eos,
                                  const int* n_hist, int B, int V, int K, void* stream);
int spider_lm_head_argmax_w4(const void* blocks, const void* scales, const void* x, const void* norm_w, float eps, int* out_ids,
                             void* logits, void* ws_val, void* ws_idx, int B, int V, int K, void* stream);
int spider_lm_head_argmax_proc_w4(const void* blocks, const void* scales, const void* x, const void* norm_w, float eps,
                                  int* out_ids, void* logits, void* ws_val, void* ws_idx, const void* seen, const void* ban,
                                  const float* penalty, const int* min_new, const int* eos_ids, const int* n_eos,
                                  const int* n_hist, int B, int V, int K, void* stream);
/* spider_decode_advance_i32 + bit next_ids[b] of seen [B, ceil(V/32)] set (ids outside [0, V) set nothing) */
int spider_decode_advance_seen_i32(const int* next_ids, int* cur_ids, int* pos, int* slot, int* kv_end, int* hist, int* n_hist,
                                   void* seen, int V, int cap, int B, void* stream);
/* bitmap [B, ceil(V/32)] |= the bits of ids [B, n] (int32); ids outside [0, V) are ignored, duplicates are harmless */
int spider_token_bitmap_set_i32(const int* ids, void* bitmap, int B, int n, int V, void* stream);

/* no_repeat_ngram_size (transformers NoRepeatNGramLogitsProcessor) as a per-step ban bitmap for the *_proc lm_head forms and the
 * sampling step. Row b's sequence is s = prompt_ids[b, :n_prompt[0]] ++ hist[b, :n_hist[b]] (length L; prompt_ids [B, pcap],
 * hist [B, cap], n_prompt int32 [1]: the prompt length of an input_ids call, 0 for inputs_embeds), n = ngram[0]:
 *   ban_step[b] = ban[b] | { s[i + n - 1] : 0 <= i < L - n + 1, s[i .. i+n-1) == s[L-n+1 .. L) }     (n = 1: every token of s)
 * n <= 0 or n > L + 1 adds nothing; ids outside [0, V) set no bit. ban / ban_step: uint32 [B, ceil(V/32)], two buffers, at most
 * 64 KB per row. ngram int32 [1] is read when the kernel runs (one captured graph serves every size). One block per row.
 * spider_decode_advance_seen_ngram_i32 = spider_decode_advance_seen_i32 followed by spider_ngram_ban_i32 on the advanced state
 * (the bitmap of the NEXT step), in one launch; hist and n_hist are required. */
int spider_ngram_ban_i32(const int* prompt_ids, const int* n_prompt, int pcap, const int* hist, const int* n_hist, int cap,
                         const int* ngram, const void* ban, void* ban_step, int V, int B, void* stream);
int spider_decode_advance_seen_ngram_i32(const int* next_ids, int* cur_ids, int* pos, int* slot, int* kv_end, int* hist,
                                         int* n_hist, void* seen, const int* prompt_ids, const int* n_prompt, int pcap,
                                         const int* ngram, const void* ban, void* ban_step, int V, int cap, int B, void* stream);

/* Prompt-lookup decoding (transformers generate(prompt_lookup_num_tokens = K), PromptLookupCandidateGenerator; csrc/spec_decode.hip):
 * a decode step of ONE greedy sequence carries R = K + 1 rows, the last accepted token and up to K drafted successors.
 * spider_attn_verify_bf16: spider_attn_decode_bf16 for R consecutive query rows per sequence that share the sequence's cache under
 *   a causal rule. q [B*R, n_q, d] (rotated by spider_rope_kv_append_bf16 with S = R, which also wrote the R new K / V rows at slot
 *   ... slot + R - 1), caches [B, n_kv, T_max, d], kv_beg / kv_end [B] (kv_end includes row 0's own token): row r of sequence b sees
 *   exactly the slots kv_beg[b] <= j < kv_end[b] + r (clamped to T_max). out [B*R, n_q*d]. ws_o: B*R*n_q*nsplit*d floats, ws_ml:
 *   B*R*n_q*nsplit*2. d = 128, GQA group 1 ... 8, R 1 ... 8; anything else returns -1 with a message.
 * Row layout of the step's cursors: ids / pos / slot / lm_out int32 [B*R]; n_prompt, n_hist, kv_end, n_draft int32 [B]; prompt_ids
 *   [B, pcap], hist [B, cap]; ngram (= max_matching_ngram_size, clamped to 0 ... 8) and k_draft (= K, clamped to 0 ... R - 1) int32
 *   [1], read when the kernel runs (one captured graph serves every value); counters int64 [B, 3] = steps, drafted, accepted.
 * spider_prompt_lookup_draft_i32: over s = prompt_ids[b, :n_prompt[b]] ++ hist[b, :n_hist[b]] (length L; history slots at or past
 *   cap read as -1), for n = min(ngram, L - 1) ... 1 the EARLIEST i with s[i : i + n] == s[L - n :] and i + n < L gives the draft
 *   s[i + n : min(i + n + K, L)]; the first n that has one wins, else n_draft[b] = 0. Writes n_draft[b], ids[r] = draft[r - 1] for
 *   1 <= r <= n_draft, ids[r] = ids[0] for the other rows r >= 1, pos[r] = pos[0] + r, slot[r] = slot[0] + r. Row 0 is the caller's.
 * spider_spec_advance_draft_i32: closes a verify step whose arg-max ids are lm_out (lm_out[r] = the token behind row r). a = the
 *   largest j <= n_draft[b] with lm_out[i - 1] == ids[i] for all 1 <= i <= j; hist gets lm_out[0 .. a] (slots at or past cap are
 *   dropped), n_hist, kv_end, pos[0], slot[0] += a + 1, counters += (1, n_draft, a), ids[0] = lm_out[a]; then the draft above on
 *   the advanced sequence. One block per sequence; nothing is written outside the sequence's own rows. */
int spider_attn_verify_bf16(const void* q, const void* k_cache, const void* v_cache, const int* kv_beg, const int* kv_end,
                            void* out, void* ws_o, void* ws_ml, int B, int R, int n_q, int n_kv, int d, int T_max, float scale,
                            int nsplit, void* stream);
int spider_prompt_lookup_draft_i32(const int* prompt_ids, const int* n_prompt, int pcap, const int* hist, const int* n_hist,
                                   int cap, const int* ngram, const int* k_draft, int* ids, int* pos, int* slot, int* n_draft,
                                   int R, int B, void* stream);
int spider_spec_advance_draft_i32(const int* lm_out, int* ids, int* pos, int* slot, int* kv_end, int* n_draft, int* hist,
                                  int* n_hist, int cap, const int* prompt_ids, const int* n_prompt, int pcap, const int* ngram,
                                  const int* k_draft, void* counters, int R, int B, void* stream);

/* Assisted decoding (transformers generate(assistant_model = draft, num_assistant_tokens = K); csrc/spec_assist.hip): a draft engine
 * proposes K tokens one by one, the target verifies them as the K + 1 rows of one step (spider_attn_verify_bf16 and the R-row weight
 * route). Two launches hand tokens and cursors over between the engines; one block per sequence, nothing outside its rows is written.
 * spider_spec_assist_push_i32: behind a draft step of Rs rows per sequence whose row rs produced draft number j (src_out its arg-max,
 *   src_pos / src_slot its cursors, int32 [B*Rs]): row j (1 ... R - 1) of the target's t_ids / t_pos / t_slot [B*R] = (token,
 *   src_pos + 1, src_slot + 1), and the draft engine's next single row d_ids / d_pos / d_slot / d_kv_end [B] = (token if below
 *   draft_vocab else 0, src_pos + 1, src_slot + 1, src_slot + 2). The d_* buffers may be the source's own.
 * spider_spec_assist_advance_i32: closes the verify step (row layout, a, hist, n_hist, kv_end, pos[0], slot[0], ids[0] and counters
 *   as spider_spec_advance_draft_i32; rows 1 ... R - 1 are left to the next pushes) and writes the draft engine's two catch-up rows
 *   d_ids [B*2] = (ids[a], lm_out[a]), ids at or above draft_vocab replaced by 0, d_pos / d_slot [B*2] = (pos[0] + a, + 1) /
 *   (slot[0] + a, + 1) from the values before the advance, d_kv_end [B] = slot[0] + a + 1. */
int spider_spec_assist_push_i32(const int* src_out, const int* src_pos, const int* src_slot, int Rs, int rs, int* t_ids, int* t_pos,
                                int* t_slot, int R, int j, int* d_ids, int* d_pos, int* d_slot, int* d_kv_end, int draft_vocab,
                                int B, void* stream);
int spider_spec_assist_advance_i32(const int* lm_out, int* ids, int* pos, int* slot, int* kv_end, const int* n_draft, int* hist,
                                   int* n_hist, int cap, void* counters, int R, int* d_ids, int* d_pos, int* d_slot, int* d_kv_end,
                                   int draft_vocab, int B, void* stream);

/* Beam search step (transformers GenerationMixin._beam_search: _get_top_k_continuations, _get_running_beams_for_next_iteration and
 * the cache reorder; num_beams / length_penalty reach it from spider.py:1471-1508 and conversation.py:151-173). rows = B * K.
 * spider_beam_partial_bf16: per row of raw bf16 logits [rows, V] and slice of 4096 tokens (nslice = ceil(V / 4096)): ws_ms
 *   [rows, nslice, 2] = (max, sum exp(x - max)) in fp32, ws_val / ws_tok [rows, nslice, C] = the slice's C best logits and tokens
 *   (value descending, token ascending; token -1 where the slice has fewer than C tokens). 1 <= C <= 32.
 * spider_beam_select_f32: per batch row, score = run_scores[b, k] + (logit - lse[k]) in fp32; the C best continuations ordered by
 *   score descending, then k * V + token ascending, go to trace_score / trace_beam / trace_tok [cap, B, C] at step n_hist[b * K]
 *   (dropped when >= cap); the first K of them whose token is none of the n_eos[0] (<= 8) ids of eos_ids become the running beams:
 *   run_scores [B, K] (in place), src_beam [B, K] (beam index within the batch row), next_ids [B * K]. K <= 8, K <= C <= V.
 * spider_kv_row_gather_bf16: caches [layers, rows_alloc, n_kv, T, d]: row r <- old row (r / K) * K + src_beam[r] over the slots
 *   [kv_beg[r], kv_end[r]), for r < R, any map (two launches through k_tmp / v_tmp of the same layout; rows mapped to themselves
 *   are not touched). K = R makes src_beam an absolute row map. d % 8 == 0. */
int spider_beam_partial_bf16(const void* logits, float* ws_ms, float* ws_val, int* ws_tok, int rows, int V, int C, int nslice,
                             void* stream);
int spider_beam_select_f32(const float* ws_ms, const float* ws_val, const int* ws_tok, float* run_scores, const int* eos_ids,
                           const int* n_eos, const int* n_hist, float* trace_score, int* trace_beam, int* trace_tok, int cap,
                           int* src_beam, int* next_ids, int B, int K, int V, int C, int nslice, void* stream);
int spider_kv_row_gather_bf16(void* k_cache, void* v_cache, void* k_tmp, void* v_tmp, const int* src_beam, const int* kv_beg,
                              const int* kv_end, int K, int R, int layers, int rows_alloc, int n_kv, int T, int d, void* stream);

/* Seeded sampling step (transformers' do_sample=True as conversation.py:151-173 drives it: logits processors, temperature, top-k,
 * top-p, one draw), two launches behind the lm_head. nslice = ceil(V / 4096); every parameter is read from device memory when the
 * kernel runs: temperature, top_p float [1], top_k int [1] (1 ... 64), seed uint32 [2] (low, high word), row0 int [1] (absolute
 * index of row 0 in the call), n_hist int [rows] (tokens generated so far = the step).
 * spider_sample_partial_bf16: per row of raw bf16 logits [rows, V] and slice of 4096 tokens, the logits processors of
 *   spider_lm_head_argmax_proc_bf16 (same buffers, same fp32 arithmetic; seen = ban = NULL: none) and the slice's top_k best
 *   (value, token) into ws_val / ws_tok [rows, nslice, 64] (value descending, token ascending; token -1 past the slice's tokens).
 * spider_sample_select_f32: per row the top_k candidates in that order (rank 0 ...; exactly top_k, ties at the cut go to the lower
 *   ids), p_j = expf(x_j / T - x_0 / T) (0 for x_j = -inf), P = sum in rank order; rank j kept iff the mass before it < top_p * P
 *   (at least rank 0), S = kept mass; u = ((x >> 9) + 0.5) * 2^-23 with x the first word of Philox4x32-10 at counter
 *   (n_hist[row], row0 + row, 0, 0), key seed; next_ids[row] = first kept rank with u * S < p_0 + ... + p_j, else the last kept.
 *   Also written: cand_tok / cand_p [rows, 64] (-1 / 0 past top_k), n_keep [rows], u [rows]. */
int spider_sample_partial_bf16(const void* logits, const void* seen, const void* ban, const float* penalty, const int* min_new,
                               const int* eos_ids, const int* n_eos, const int* n_hist, const int* top_k, float* ws_val,
                               int* ws_tok, int rows, int V, int nslice, void* stream);
int spider_sample_select_f32(const float* ws_val, const int* ws_tok, const float* temperature, const float* top_p, const int* top_k,
                             const void* seed, const int* row0, const int* n_hist, int* next_ids, int* cand_tok, float* cand_p,
                             int* n_keep, float* u, int rows, int V, int nslice, void* stream);

/* Teacher-forced scoring of rows of bf16 logits (csrc/logprob.hip). Replaces, per row, `logits.float()` -> `log_softmax(-1)` ->
 * `gather(labels)` of LlamaForCausalLM.forward(labels=...) / ForCausalLMLoss, and softmax / kl_div between two models' logits.
 * logits [rows, ld] bf16 with V valid columns (ld >= V, ld % 8 == 0, the gap is never interpreted); targets int32 [rows].
 * x = float(logits[r, :V]): lse[r] = m + log sum exp(x - m); logprob[r] = x[target] - lse (0 for a target outside [0, V), HF's
 * ignore_index -100); argmax[r] = lowest id among the maxima; entropy[r] = -sum p log p. With logits_ref [rows, ld_ref] (same
 * rules), y = float(logits_ref[r, :V]), p_ref = softmax(y): kl[r] = KL(p_ref || p) = sum p_ref (y - x) - lse_ref + lse and
 * argmax_ref[r]; logits_ref, kl and argmax_ref are all given or all NULL. One pass, fp32, one block per row: a row's result
 * does not depend on the other rows of the call; logits_ref == logits gives kl == 0.0 exactly. Logits must be finite. */
int spider_logprob_rows_bf16(const void* logits, int ld, const int* targets, const void* logits_ref, int ld_ref, float* logprob,
                             float* lse, int* argmax, float* entropy, float* kl, int* argmax_ref, int rows, int V, void* stream);

/* Calibrated MXFP4 (GPTQ on MX blocks; csrc/gptq.hip, `llm.quantize_mxfp4_gptq` is the definition): the quantise-and-compensate
 * sweep over ONE group of nblocks (1..4) consecutive MX blocks, columns [j0, j0 + 32 nblocks), for all N rows, in fp32.
 * Wt [K, N] fp32: the K-major working copy of the weights (column j of every row contiguous), read only; U [K, K] fp32 row-major:
 * the upper Cholesky factor of H^-1, of which the group's diagonal block is read. Per row and block: the E8M0 byte from the amax
 * of the current weights by quantize_mxfp4's rule, then per column in order the e2m1 code (ties to the even significand,
 * saturating at code 7), e = (w - q) / U[j, j], and w' -= e U[j, j'] for the later columns j' of the group. Written: blocks
 * [N, K / 2] uint8 (16 bytes per row and block, quantize_mxfp4's layout), scales [N, K / 32] uint8, Et [32 nblocks, N] fp32 (E
 * transposed; rows of an Et with at least 32 nblocks rows). The caller owes the columns behind the group
 * Wt[j0 + 32 nblocks:, :] -= U[j0 : j0 + 32 nblocks, j0 + 32 nblocks:]^T Et before the next launch. */
int spider_gptq_mxfp4_sweep_f32(const float* Wt, const float* U, void* blocks, void* scales, float* Et, int N, int K, int j0,
                                int nblocks, void* stream);

/* apply_rotary_pos_emb (modeling_llama3.py:150-183; modeling_llama.py:116-123) on q,k of a fused QKV
 * projection + KV-cache append (modeling_llama.py:190-193). qkv [B*S,(n_q+2n_kv)*d]; cos_sin fp32
 * [max_pos, d] = [cos(d/2) | sin(d/2)]; q_out [B*S,n_q,d]; caches [B,n_kv,T_max,d]. */
int spider_rope_kv_append_bf16(const void* qkv, const int* pos, const int* slot, const float* cos_sin, void* q_out,
                               void* k_cache, void* v_cache, int B, int S, int n_q, int n_kv, int d, int T_max,
                               void* stream);
/* Multimodal RoPE of the Qwen2.5-Omni thinker (transformers apply_multimodal_rotary_pos_emb, reached from
 * Qwen2_5OmniModel.generate, qwen2.5omni_infer.py:3 / qwen2.5omni_spider_web.py:468): pos3 is [3, B*S]
 * (temporal, height, width); the first sec_t rotary pairs follow component 0, the next sec_h component 1, the rest
 * component 2 (mrope_section 16/24/24 at head_dim 128). sec_t = sec_h = 0 degenerates to spider_rope_kv_append_bf16. */
int spider_rope_kv_append_mrope_bf16(const void* qkv, const int* pos3, const int* slot, const float* cos_sin, void* q_out,
                                     void* k_cache, void* v_cache, int B, int S, int n_q, int n_kv, int d, int T_max,
                                     int sec_t, int sec_h, void* stream);

/* decode attention, one query token per sequence, GQA, fp32 online softmax, split over the KV length
 * (eager_attention_forward + repeat_kv, modeling_llama3.py:202-237). Valid cache slots per sequence:
 * [kv_beg[b], kv_end[b]) (kv_beg may be NULL = 0). ws_o: B*n_q*nsplit*d floats, ws_ml: B*n_q*nsplit*2.
 * head_dim d = 128; GQA group n_q / n_kv = 1 ... 8 (Llama-3-8B: 4, Qwen2.5-Omni-7B: 7); other shapes return -1 with a message. */
int spider_attn_decode_bf16(const void* q, const void* k_cache, const void* v_cache, const int* kv_beg,
                            const int* kv_end, void* out, void* ws_o, void* ws_ml, int B, int n_q, int n_kv, int d,
                            int T_max, float scale, int nsplit, void* stream);

/* The three calls above (RoPE, KV append, attention + combine) fused into ONE launch for decode: qkv [B,(n_q+2n_kv)d]
 * is the current token's fused projection; kv_end[b] INCLUDES the current token (slot kv_end[b]-1 is written here).
 * counters: int[B*n_kv], zeroed once at allocation (the kernel resets them). */
int spider_attn_decode_fused_bf16(const void* qkv, const int* pos, const float* cos_sin, void* k_cache, void* v_cache,
                                  const int* kv_beg, const int* kv_end, void* out, void* ws_o, void* ws_ml,
                                  int* counters, int B, int n_q, int n_kv, int d, int T_max, float scale, int nsplit,
                                  void* stream);
/* Tuning / test aid: 1 / 2 = the split-KV combine of spider_attn_decode_fused_bf16 runs inside the attention launch (last-arriving
 * block; 1: acq_rel ticket, 2: write-through partials + relaxed ticket + sc1 loads, no fence), 0 = in the separate combine launch
 * (SPIDER_ATTN_INLINE is read once, at the first call). Returns the previous setting. */
int spider_set_attn_inline(int on);
/* Tuning / test aid: form of the kernel behind spider_attn_decode_fused_bf16: 1 = q RoPE once per block (through LDS), cross-lane
 * exchanges on the VALU (DPP, v_permlane16/32_swap) and 16-byte tail stores (default), 0 = the earlier form (q RoPE in every wave,
 * ds_bpermute exchanges, 4-byte tail stores). Same arithmetic in the same order: bit-identical output, cache rows and partials.
 * SPIDER_ATTN_XLANE is read once, at the first use. The SCHED 1 / 2 decode GEMVs use the same VALU exchanges; their old form is
 * spider_set_gemv_sched(0). Returns the previous setting. */
int spider_set_attn_xlane(int on);
/* Tuning / test aid: memory schedule of the decode GEMVs (spider_gemv_bf16 / spider_gemv_swiglu_bf16, 1..8 sequences): 0 = one request
 * at a time (activation staging vector by vector, the next weight chunks requested after the previous ones are consumed), 1 = one round
 * trip per block (default: activations and the hoisted weight chunks -- the whole row where K <= 4096 -- requested together, two register
 * sets in the long-K loop). Same arithmetic in the same order: bit-identical outputs. SPIDER_GEMV_SCHED is read once, at the first use;
 * SPIDER_GEMV_HOIST=0 selects schedule 0 without its weight hoist. Returns the previous setting. */
int spider_set_gemv_sched(int sched);
/* Tuning / test aid: split-K combine of the weight-stationary streaming conv (w_tiled = 2): 1 = inside the launch by the last-arriving
 * block of a strip (default), 0 = partial slabs + the reduce kernel (SPIDER_WS_INLAUNCH is read at the first such launch). Both forms sum
 * the slabs in split order: bit-identical outputs. The arrival counters live in the 4096 bytes behind the declared workspace: ONE stream
 * at a time may use a workspace (and its counter tail) -- concurrent streams need workspaces of their own. Returns the previous setting. */
int spider_set_ws_inlaunch(int on);

/* Batched-decode forms on a FRAGMENT-MAJOR weight copy (5..16 sequences share one weight stream; also valid for 1..4).
 * Wfm = the weight W [N, K] repacked once at load time so that every wave instruction of the kernel reads 1 KiB of contiguous
 * memory: [ceil(N/16) row groups][K/64 k blocks][2 sub-steps][64 lanes][8 bf16], lane 16 g + r of a piece holding
 * W[16 rg + r][64 kb + 32 sx + 8 g + 0..7] (the A fragment of mfma_f32_16x16x32_bf16); rows beyond N are zero. K % 64 == 0.
 * fold_rmsnorm = 0: x [B, K] is used as is. fold_rmsnorm = 1: RMSNorm folded into the projection -- x is the un-normalised
 * residual stream, Wfm was repacked from W * diag(norm_w) (bf16), and the kernel takes sum x^2 per sequence from the x fragments
 * it streams anyway and scales its accumulators by rsqrt(mean + eps): LlamaRMSNorm + nn.Linear in one launch
 * (modeling_llama3.py:77-82 + :186-199). Replaces the same nn.Linear calls as spider_gemv_bf16 /
 * spider_gemv_swiglu_bf16 / spider_lm_head_argmax_bf16 (modeling_llama3.py:186-199,240-313,870-871) at batch sizes where the
 * row-major gather (16 rows x 64 B per instruction) cannot reach the HBM stream rate. */
int spider_gemv_fm_bf16(const void* Wfm, const void* x, void* out, const void* bias, const void* res, int B, int N, int K,
                        int fold_rmsnorm, float eps, void* stream);
/* Wfm_gate_up: the repacked [gate rows (I) | up rows (I)] matrix, I % 16 == 0; out[b, i] = silu(g) * u */
int spider_gemv_swiglu_fm_bf16(const void* Wfm_gate_up, const void* x, void* out, int B, int I, int K, int fold_rmsnorm, float eps,
                               void* stream);
/* logits (optional) [B, V] bf16; ws_val / ws_idx >= B * spider_lm_head_nparts(V) entries; ties -> lowest token id */
int spider_lm_head_argmax_fm_bf16(const void* Wfm, const void* x, int* out_ids, void* logits, void* ws_val, void* ws_idx, int B,
                                  int V, int K, int fold_rmsnorm, float eps, void* stream);
/* the fragment-major lm_head with the logits processors of spider_lm_head_argmax_proc_bf16 */
int spider_lm_head_argmax_fm_proc_bf16(const void* Wfm, const void* x, int* out_ids, void* logits, void* ws_val, void* ws_idx,
                                       const void* seen, const void* ban, const float* penalty, const int* min_new,
                                       const int* eos_ids, const int* n_eos, const int* n_hist, int B, int V, int K,
                                       int fold_rmsnorm, float eps, void* stream);

/* ======================= MFMA GEMM / conv / attention ======================= */

/* C = act(A[M,K] . W[N,K]^T + bias[N] + rowbias[row/rows_per_group, N]) (+res) * out_scale.
 * Exactly one of C (bf16) / C32 (fp32). act: 0 none, 1 silu, 2 gelu(erf), 3 quick-gelu, 4 GEGLU (W = [value rows |
 * gate rows], N counts W rows, the output has N/2 columns: out = (A.Wv^T + bv) * gelu(A.Wg^T + bg), diffusers FeedForward).
 * ws/ws_bytes: optional fp32 split-K workspace (NULL = never split K); small-M / large-K problems use it
 * to fill the 256 CUs.
 * Prefill projections (modeling_llama3.py:186-313), diffusers Attention/FeedForward/proj linears. */
int spider_gemm_bf16(const void* A, const void* W, void* C, void* C32, const void* bias, const void* res,
                     const void* rowbias, int rows_per_group, int M, int N, int K, int lda, int ldc, int act,
                     float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes, void* stream);

/* C = LayerNorm(A; gamma, beta, eps) . W^T + bias (+res) in ONE launch (act 0), or its GEGLU form (act 4, as above).
 * Replaces BasicTransformerBlock.norm1 / norm2 / norm3 + the projection that consumes it (attn1 to_q/k/v, attn2 to_q,
 * ff.net.0.proj; diffusers-0.25 attention.py, reached from custom_sd.py:634-639). The normalisation is folded:
 *   Wf = W * diag(gamma) (bf16 [N,K]), colsum[n] = sum_k Wf[n,k] (fp32), colbias[n] = sum_k beta[k] W[n,k] + bias[n] (fp32)
 * are prepared once per layer by the caller; the kernel takes the row statistics of A while it stages the rows and applies
 * C = rstd * (A.Wf^T - mean * colsum) + colbias in the epilogue. Rows of A are K wide (lda = K).
 * ws (optional, >= ceil(M/256)*256*8 bytes): lets large problems run on the 256x256 LDS-DMA kernel, whose row statistics
 * come from a preceding one-wave-per-row pass instead of the staging loop. */
int spider_gemm_ln_bf16(const void* A, const void* Wf, void* C, const float* colsum, const float* colbias, const void* res,
                        int M, int N, int K, int ldc, int act, float eps, int w_tiled, void* ws, long ws_bytes, void* stream);

/* Fused cross-attention sub-block of BasicTransformerBlock (diffusers-0.25 attention.py, reached from custom_sd.py:634-639):
 *   out = x + to_out( softmax( to_q(LayerNorm(x)) K^T / sqrt(d) ) V )      for 8 heads and <= 80 text keys, ONE launch.
 * The prompt's K / V are constant over the denoising loop and are folded into the projections once per prompt:
 *   Mq[b] [8*80, C] = scale * K_h[b] . Wq_h . diag(gamma)   (key l of head h at row 80 h + l; rows of keys >= n_keys are zero)
 *   Mo[b] [C, 8*80] = Wo_h . V_h[b]^T
 *   colsum[b, r] = sum_c Mq[b][r, c],  colbias[b, r] = scale * K_h[b][l] . (Wq_h . beta)      (LayerNorm fold, fp32)
 * mq_fm / mo_fm are the fragment-major copies of Mq [B2 * 640, C] and Mo [B2 * C, 640] (layout of spider_gemv_fm_bf16's Wfm).
 * x, out [B2 * n_tok, C] bf16 (sample-major rows); C % 64 == 0, C <= 1280; n_tok % 16 == 0. */
int spider_xattn_fused_bf16(const void* x, const void* mq_fm, const void* mo_fm, const float* colsum, const float* colbias,
                            const void* bias_o, void* out, int B2, int n_tok, int C, int heads, int n_keys, float eps,
                            const float* x32, float* out32, void* stream);

/* conv2d NHWC as implicit GEMM (ResnetBlock2D / Downsample2D / Upsample2D convs reached from
 * custom_sd.py:634-639). w is OHWI [Cout,ks,ks,Cin]; ups=1 fuses the nearest-2x upsample. */
int spider_conv2d_nhwc_bf16(const void* x, const void* w, void* y, const void* bias, const void* res,
                            const void* rowbias, int B, int Hin, int Win, int Cin, int Cout, int ks, int stride,
                            int pad, int ups, float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes, void* stream);

/* General NHWC conv as implicit GEMM: rectangular / dilated kernels (w OHWI [Cout,kh,kw,Cin], Cin % 8 == 0), a fused
 * nearest upsample to an explicit size up_h x up_w in (in, 2*in] (diffusers Upsample2D with `upsample_size`, reached when
 * the AudioLDM latent height 125 is not a multiple of 8: custom_ad.py:490-504), fused activation (1 silu, 2 gelu,
 * 3 quick-gelu, 5 leaky-relu(act_param), 6 relu, 7 tanh). 1-D convs (HiFi-GAN vocoder behind
 * custom_ad.py:293-300) are Hin = kh = 1; the (3,1,1) temporal convs of UNet3D (custom_vd.py:671-676) are
 * Hin = frames, Win = H*W, kh = 3, kw = 1.
 * w_tiled: 0 = w as stored (OHWI); 1 = its tile-major copy (see spider_gemm_bf16); 2 = its FRAGMENT-MAJOR copy
 * [ceil(Cout/32)*2][(Cin/32)*9][64 lanes][8]: piece (rg, cb*9 + tap) holds at lane 16 g + r the 8 values
 * w[16 rg + r, tap, 32 cb + 8 g .. + 8] (Cout zero-padded to a multiple of 32) -- operand of the weight-stationary streaming
 * kernel that serves the weight-bound levels of the UNet (ResnetBlock2D convs / the 2x upsampler at <= 512 output pixels,
 * custom_sd.py:634-639): 3x3, stride 1, pad 1, dil 1, Cin % 32 == 0, no activation, B*Hout*Wout <= 512 (and <= 128 input
 * pixels when B*Hout*Wout <= 128); anything else with w_tiled = 2 is refused. With w_tiled = 2 the workspace must extend 4096
 * bytes beyond ws_bytes, zero-initialised once: the arrival counters of the in-launch split-K combine (the block that arrives
 * last at a strip's counter sums the partial slabs in split order and applies the epilogue; the counters are zero again when
 * the call has completed, so graph replays and later calls need no reset). */
int spider_conv_nhwc_ex_bf16(const void* x, const void* w, void* y, const void* bias, const void* res,
                             const void* rowbias, int B, int Hin, int Win, int Cin, int Cout, int kh, int kw, int stride,
                             int pad_h, int pad_w, int dil, int up_h, int up_w, int act, float act_param,
                             float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes, void* stream);

/* fused attention (prefill causal GQA: modeling_llama3.py:202-237; UNet self/cross attention:
 * StoryDiffusion/utils/gradio_utils.py:400-472; consistent self-attention with the column keep vector of
 * cal_attn_mask_xl: Comic_Generation.py:129-196, gradio_utils.py:241-287). Strides in elements. */
int spider_attn_bf16(const void* q, const void* k, const void* v, void* o,
                     long q_bs, long q_hs, long q_rs, long k_bs, long k_hs, long k_rs,
                     long v_bs, long v_hs, long v_rs, long o_bs, long o_hs, long o_rs,
                     int B, int Hq, int Hkv, int Lq, int Lk, int d, float scale, int causal, int kv_off,
                     const int* kv_beg, const void* keep_bits, int blk, int q_off, void* stream);

/* Consistent self-attention (StoryDiffusion SpatialAttnProcessor2_0 + cal_attn_mask_xl, Comic_Generation.py:129-196,
 * gradio_utils.py:241-287) through visible-key lists: query image i sees key j iff its keep bit is set or j lies in image i's
 * own block, so instead of scoring all keys and zeroing the masked ones (spider_attn_bf16 keep_bits / blk / q_off) the kernel
 * walks a per-image list of visible keys -- same softmax, ~40 % fewer keys at keep rate 0.5. head_dim <= 64 (SDXL: 64).
 * spider_story_key_lists_i32 builds, once per UNet step and resolution, key_idx [n_lists * stride] and the query-tile records
 * tiles [n_lists * ceil(N/128)][4]; spider_attn_keylist_bf16 consumes them (strides as in spider_attn_bf16). */
int spider_story_key_lists_i32(const void* keep_bits, int n_keys, int N, int img0, int n_lists, int q_img0, int stride,
                               int* key_idx, int* tiles, void* stream);
int spider_attn_keylist_bf16(const void* q, const void* k, const void* v, void* o,
                             long q_bs, long q_hs, long q_rs, long k_bs, long k_hs, long k_rs,
                             long v_bs, long v_hs, long v_rs, long o_bs, long o_hs, long o_rs,
                             int B, int Hq, int Hkv, int Lq, int Lk, int d, float scale,
                             const int* key_idx, int idx_len, const int* tiles, int n_tiles, void* stream);

/* packed variable-length attention: the per-segment SDPA loop over cu_seqlens of transformers'
 * Qwen2_5OmniVisionAttention / Qwen2_5OmniAudioAttention (window / full-frame / audio-chunk segments), reached from the
 * reference through Qwen2_5OmniModel.generate(**inputs) with images / audios (qwen2.5omni_spider_web.py:461-468).
 * q/k/v/o: [total_rows, heads, d] views (row strides in elements, head stride d). tiles: device int[n_tiles][4] =
 * {q_start, q_len (1..128), k_start, k_len}; the caller guarantees every range lies inside [0, total_rows). */
int spider_attn_varlen_bf16(const void* q, const void* k, const void* v, void* o, long q_rs, long k_rs, long v_rs, long o_rs,
                            int total_rows, int Hq, int Hkv, int d, float scale, const int* tiles, int n_tiles, void* stream);

/* in-place half-rotation RoPE with a per-row angle table: transformers apply_rotary_pos_emb_vision of the Qwen2.5-Omni
 * vision tower (same call path as above). x: bf16 rows of heads*d contiguous elements, row_stride apart;
 * cos_sin: fp32 [rows, d] = [cos(d/2) | sin(d/2)]. */
int spider_rope_rows_bf16(void* x, const float* cos_sin, long row_stride, int rows, int heads, int d, void* stream);

/* ======================= UNet elementwise / normalisation (HBM-bound) ======================= */

/* GroupNorm(+SiLU) on NHWC (ResnetBlock2D.norm1/2, Transformer2DModel.norm, conv_norm_out).
 * ws: B*spider_groupnorm_nchunk(HW)*G*2 floats of scratch; what the call leaves there is private (a centred (mean, M2) per chunk
 * and group, not the public partial format below) and must not be handed to spider_groupnorm_apply_* / spider_gemm_gn_in_*. */
int spider_groupnorm_nchunk(int HW);
int spider_groupnorm_nhwc_bf16(const void* x, const void* gamma, const void* beta, void* y, void* ws, int B, int HW,
                               int C, int G, float eps, int silu, void* stream);
/* The same GroupNorm on the channel concatenation [x1 | x2] without materialising it first: UpBlock2D / UpBlock3D's
 * torch.cat([hidden_states, res_hidden_states], dim=1) followed by ResnetBlock2D.norm1 (diffusers unet_2d_blocks, called from
 * custom_sd.py:634-639). x1 [B,HW,C1], x2 [B,HW,C2] are read in place; y [B,HW,C1+C2] is the normalised (+SiLU) result and
 * cat [B,HW,C1+C2] receives the concatenated input (the resnet's 1x1 conv_shortcut reads it). C1, C2 multiples of 8. */
int spider_groupnorm_cat_nhwc_bf16(const void* x1, const void* x2, const void* gamma, const void* beta, void* y, void* cat,
                                   void* ws, int B, int HW, int C1, int C2, int G, float eps, int silu, void* stream);
/* GroupNorm with the statistics taken from the PRODUCER of its input (round 4; diffusers ResnetBlock2D: conv1 -> norm2, conv2 ->
 * the next block's norm; Transformer2DModel: norm -> proj_in). The reference runs torch.nn.GroupNorm as its own pass over the
 * tensor (custom_sd.py:634-639 -> UNet2DConditionModel.forward); here the conv that writes the tensor also writes, per chunk of
 * `chunk_rows` consecutive output pixels and per group, (sum, sum of squares) of the 16-bit values it stores -- the [B, nchunk, G, 2]
 * fp32 partial array every consumer reduces in a fixed order (no atomics: hipGraph replay stays bit-identical to eager launches).
 *   spider_conv_nhwc_gn_*: spider_conv_nhwc_ex_* + gn_part (room for B * HW / 16 * gn_groups * 2 floats) / gn_groups; *produced =
 *       rows per chunk of the statistics written, nchunk = HW / *produced: 64 (LDS-DMA conv epilogue), 16 (split-K reduce), or 0
 *       when this shape's kernel cannot write them (run spider_groupnorm_stats_* instead). HW must be a multiple of 16.
 *   spider_groupnorm_stats_nhwc_*: the statistics pass alone (any nchunk).
 *   spider_groupnorm_apply_nhwc_*: normalise (+ SiLU) with given partials.
 *   spider_gemm_gn_in_*: C = GroupNorm(A) W^T + bias with the normalisation applied to A on its way into LDS (norm + proj_in in
 *       one launch); c32d optional fp32 copy of C (fp32 residual stream).
 * Limit of this format: every consumer takes var = Q / n - mean^2 from the fp32 sums, which loses about 2 log2(|mean| / sigma) bits
 * of a group whose mean is large against its spread (relative error of the normalised value ~1e-6 at |mean| / sigma = 4, ~3e-4 at 64).
 * The entry points that make their own statistics (spider_groupnorm_nhwc_*, spider_groupnorm_f32in_nhwc_* with partial == NULL)
 * do not go through it and have no such dependence. */
int spider_conv_nhwc_gn_bf16(const void* x, const void* w, void* y, const void* bias, const void* res, const void* rowbias,
                             int B, int Hin, int Win, int Cin, int Cout, int kh, int kw, int stride, int pad_h, int pad_w,
                             int dil, int up_h, int up_w, int act, float act_param, float out_scale, int w_tiled,
                             const float* res32, float* c32d, void* ws, long ws_bytes, void* stream,
                             float* gn_part, int gn_groups, int* produced);
int spider_groupnorm_stats_nhwc_bf16(const void* x, void* partial, int B, int HW, int C, int G, int nchunk, void* stream);
int spider_groupnorm_apply_nhwc_bf16(const void* x, const void* partial, int nchunk, const void* gamma, const void* beta, void* y,
                                     int B, int HW, int C, int G, float eps, int silu, void* stream);
int spider_gemm_gn_in_bf16(const void* A, const void* W, void* C, const void* bias, int M, int N, int K, int ldc, int w_tiled,
                           const float* gn_part, int nchunk, const void* gamma, const void* beta, int G, float eps, int HW,
                           float* c32d, void* stream);
int spider_layernorm_bf16(const void* x, const void* gamma, const void* beta, void* y, int rows, int C, float eps,
                          void* stream);
/* GEGLU (diffusers FeedForward): y[m,n] = x[m,n] * gelu(x[m,inner+n]) */
int spider_geglu_bf16(const void* x, void* y, int M, int inner, void* stream);
/* SwiGLU on a fused [gate|up] prefill projection (modeling_llama3.py:197-199) */
int spider_swiglu_bf16(const void* x, void* y, int M, int inner, void* stream);
int spider_concat_channels_bf16(const void* a, const void* b, void* y, long rows, int C1, int C2, void* stream);
int spider_act_bf16(const void* x, void* y, long n, int act, void* stream);
int spider_add_bf16(const void* a, const void* b, void* y, long n, void* stream);
/* act_ex: 1 silu, 2 gelu(erf), 3 quick-gelu, 5 leaky-relu(param), 6 relu, 7 tanh (HiFi-GAN / CLAP pooler+projection) */
int spider_act_ex_bf16(const void* x, void* y, long n, int act, float param, void* stream);
/* y = (a + b) * scale  (HiFi-GAN: mean of the residual-block branches) */
int spider_add_scaled_bf16(const void* a, const void* b, void* y, long n, float scale, void* stream);
/* y = alpha*a + beta*b: the 0.1 / 0.9 blend of projected LLM states with text-encoder embeddings (spider.py:420,432,444) */
int spider_axpby_bf16(const void* a, const void* b, void* y, long n, float alpha, float beta, void* stream);
/* TextFcLayerMoE router input: mean over tokens, x [B,T,C] -> [B,C] (spider/models/layers.py:254) */
int spider_mean_tokens_bf16(const void* x, void* y, int B, int T, int C, void* stream);
/* TextFcLayerMoE mixing: r = sigmoid(logits[b,:E]) / sum, y[b,...] = sum_e r[e] * x_e[b,...]; host_xs is a HOST array of E
 * device pointers [B, per_batch]; logits rows are ld wide (layers.py:255-267) */
int spider_moe_combine_bf16(const void* const* host_xs, int E, const void* logits, int ld, void* y, int B, long per_batch,
                            void* stream);
/* ConvTranspose1d = per-tap GEMM (spider_gemm_bf16 with fp32 output, cols [B,L_in,k,Cout]) + this overlap-add:
 * y[b,t,:] = bias + sum_{i*stride - pad + j == t} cols[b,i,j,:]; L_out = (L_in-1)*stride - 2*pad + k
 * (HiFi-GAN upsampler, SpeechT5HifiGan called from custom_ad.py:293-300). */
int spider_col2im1d_f32_bf16(const float* cols, const void* bias, void* y, int B, int L_in, int k, int stride, int pad,
                             int Cout, void* stream);
/* y[r,:] = x[r,:] / max(||x[r,:]||_2, eps)  (F.normalize of the CLAP text embedding, custom_ad.py:217-219,272-273) */
int spider_l2_normalize_rows_bf16(const void* x, void* y, int rows, int n, float eps, void* stream);
int spider_conv2d_small_cin_bf16(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int Cin,
                                 int Cout, int ks, void* stream);
int spider_conv2d_small_cout_bf16(const void* x, const void* w, const void* bias, void* y32, void* y16, int B, int H,
                                  int W, int Cin, int Cout, int ks, void* stream);

/* ---- latent plumbing of the denoising loop (custom_sd.py:631-647) ---- */
/* torch.cat([latents]*reps) + scale_model_input: fp32 NCHW -> bf16 NHWC */
int spider_latent_to_nhwc_bf16(const float* lat, void* out, int B, int C, int HW, int reps, float scale, void* stream);
/* noise_pred_uncond + g*(noise_pred_text - noise_pred_uncond): fp32 NHWC [2,B,HW,C] -> fp32 NCHW */
int spider_cfg_combine_f32(const float* eps2, float* out, int B, int C, int HW, float guidance, void* stream);
/* scheduler.step as a linear update: out = sum_j host_coefs[j] * ins[j]; host_ins is a HOST array of n device ptrs */
int spider_lincomb_f32(const float* const* host_ins, const float* host_coefs, int n, float* out, long total, void* stream);
/* row softmax of fp32 scores -> bf16 probabilities (VAE mid-block single-head attention, d = 512). Rows are n wide;
 * the first n_valid columns are normalised, the rest (padding up to a multiple of 8 for the P.V GEMM) written as 0. */
int spider_softmax_rows_f32_bf16(const float* x, void* y, int rows, int n, int n_valid, float scale, void* stream);
int spider_nhwc_to_nchw_f32(const float* x, float* y, int B, int C, int HW, float mul, float add, int clamp01, void* stream);

/* StoryDiffusion keep vector -> bit words for spider_attn_bf16's keep_bits (cal_attn_mask_xl, utils/gradio_utils.py:241-287, reduced to
 * the random per-key keep decision): bit j % 64 of word j / 64 = (u[j] < thr) for j < n_valid, 0 beyond. u [n] fp32 on the device. */
int spider_pack_keep_bits_f32(const float* u, void* words, int n, int n_valid, float thr, void* stream);

/* ---- Stable Diffusion safety checker around the CLIP ViT (csrc/safety.hip; run_safety_checker, custom_sd.py:376-384, called at :658) ----
 * Additive to ABI v4. The 16-bit format of these three is an argument (f16: 0 = bf16, 1 = IEEE half), not a second entry point.
 * spider_clip_preprocess: numpy_to_pil + CLIPImageProcessor on the device. images [B,3,H,W] fp32 in [0,1] -> 8-bit as
 *   (x * 255).round() (half-even) -> Pillow's antialiased BICUBIC resize, horizontal pass then vertical, each pass rounded to 8 bits and
 *   clipped (22-bit fixed-point taps, Pillow's Resample.c) -> centre crop -> (v / 255 - mean_c) / std_c -> patch rows
 *   rows [B * (crop / patch)^2, Kp] (16-bit), column (c * patch + dy) * patch + dx, columns 3 patch^2 .. Kp - 1 written as zeros (Kp = 3 patch^2
 *   rounded up to a multiple of 8: the K of the patch-embedding GEMM). The tap tables depend only on (H, W, size, crop) and live on the
 *   device: xbounds / ybounds [crop, 2] int32 = (first input index, tap count) of each output column / row INSIDE the crop window,
 *   xtaps [crop, ks_x] / ytaps [crop, ks_y] int32 = round(w * 2^22), zero beyond the count. norm [6] fp32 = mean[3], std[3].
 *   tmp: B * 3 * H * crop bytes (the 8-bit image between the passes). Two launches, no atomics. */
int spider_clip_preprocess(const float* images, void* tmp, void* rows, const int* xbounds, const int* xtaps, int ks_x,
                           const int* ybounds, const int* ytaps, int ks_y, const float* norm, int B, int H, int W, int crop, int patch,
                           int Kp, int f16, void* stream);
/* StableDiffusionSafetyChecker.forward (diffusers 0.25) after the ViT, one block per image: fp32 cosine similarity of image_embeds [B,D]
 * against special_care_embeds [n_special,D] and concept_embeds [n_concept,D] (all 16-bit, D % 8 == 0); special-care concepts first, in
 * index order, score = round(cos - thr + adjustment, 3) (half-even on x * 1000) with adjustment 0 until one scores > 0 and 0.01 from the
 * next entry on; then every concept the same way; flags[b] = any concept score > 0. scores [B, n_special + n_concept] fp32
 * (special-care first), flags [B] int32; n_special + n_concept <= 64. */
int spider_safety_decide(const void* image_embeds, const void* concept_embeds, const void* special_care_embeds, const float* thr_concept,
                         const float* thr_special, float* scores, int* flags, int B, int D, int n_concept, int n_special, int f16,
                         void* stream);
/* images [B, per_image] fp32 (per_image = C * H * W, a multiple of 4): every image with flags[b] != 0 becomes zeros, in place */
int spider_image_blackout_f32(float* images, const int* flags, int B, long per_image, void* stream);

/* ---- Whisper log-mel features, the audio input of Qwen2.5-Omni (csrc/audio_features.hip; WhisperFeatureExtractor with
 * padding="max_length", as Qwen2_5OmniProcessor calls it) ---- Additive to ABI v4.
 * waves: fp32 clips packed one behind the other; clip b = waves[offsets[b] .. offsets[b] + lengths[b]) (int32 device arrays; a
 *   length beyond n_samples is truncated). Per clip, as if zero-padded to n_samples: reflect pad n_fft / 2, frames of n_fft at hop,
 *   periodic Hann, |X_k|^2, last frame dropped (cap = n_samples / hop frames), mel projection, log10(max(., 1e-10)),
 *   max(., clip_max - 8), (. + 4) / 4. feat [B, mel, cap] fp32 and mask [B, cap] int32 (1 for frame f < ceil(length / hop)) are written
 *   completely: frames whose window holds only padding get the floor value (max(clip_max - 8, -10) + 4) / 4 without being computed.
 * table [n_fft, ldt] fp32, ldt = 64 G, G = ceil((n_fft / 2 + 1) / 32): columns [64 g, 64 g + 32) = w[n] cos(2 pi n k / n_fft),
 *   [64 g + 32, 64 g + 64) = w[n] sin(2 pi n k / n_fft) for the bins k = 32 g .. 32 g + 31, zero columns beyond n_fft / 2;
 *   fb [n_fft / 2 + 1, mel] fp32. n_fft even and <= 512, mel <= 128, hop <= n_fft, cap * hop <= n_samples.
 * tile_max: B * max_tiles floats of scratch; max_tiles = ceil(F / spider_logmel_tile_frames()), F = the frames of the LONGEST clip
 *   whose window reaches it, min(cap, ceil((length + n_fft / 2) / hop)): the host-known lengths size the grid. Two launches (frames x
 *   DFT table and the mel projection on the fp32-input MFMA; then clip maximum, clamp, scale, floor fill, mask), no atomics, no
 *   synchronisation: the result is a pure function of the inputs. */
int spider_logmel_tile_frames(void);
int spider_logmel_f32(const float* waves, const int* offsets, const int* lengths, const float* table, const float* fb, float* feat,
                      int* mask, float* tile_max, int B, int n_samples, int n_fft, int hop, int mel, int cap, int ldt, int max_tiles,
                      void* stream);

/* ---- Qwen2-VL image patch rows, the image input of Qwen2.5-Omni (csrc/image_features.hip; Qwen2VLImageProcessorPil: smart_resize
 * with Pillow's antialiased BICUBIC, (v / 255 - mean) / std, merge-block patch order, the frame written `temporal` times) ----
 * Additive to ABI v4.
 * images: uint8 RGB, interleaved HWC, packed one behind the other. desc: int64 [n_images, 16] on the device, per image
 *   {byte offset into images, H, W, Ho, Wo, x bounds offset, x taps offset, ks_x, y bounds offset, y taps offset, ks_y, first output
 *   row, byte offset into tmp, first input row the vertical pass reads, number of such rows, 0}; Ho and Wo are multiples of
 *   patch * merge. tabs: int32, the four tables of every image at the offsets the descriptor names: bounds [n_out, 2] = (first input
 *   index, tap count), taps [n_out, ks] (Pillow's 22-bit fixed point; the tap count is a run-time value without a cap).
 * lut: uint32 [3, 256], the output element of channel c and 8-bit value v (bf16 in the low half, or the fp32 word): built on the host,
 *   so that the result carries the host processor's bits. tmp: sum_i 3 * rows_i * Wo_i bytes of scratch, each image's piece 4-byte aligned.
 * rows [sum_i Ho_i Wo_i / patch^2, 3 * temporal * patch^2] bf16 (f32 = 0) or fp32 (f32 = 1), 16-byte aligned, every element written:
 *   row ((gh / merge * (Gw / merge) + gw / merge) * merge + mh) * merge + mw behind the image's first row, column
 *   ((c * temporal + t) * patch + dy) * patch + dx. max_h_items = max_i rows_i * Wo_i / 4 and max_tiles = max_i (Ho_i Wo_i) / (patch merge)^2
 *   size the two grids. Two launches (horizontal pass to 8 bits; vertical pass + clip + lookup + patch rows), no synchronisation. */
int spider_qwen_image_patches(const void* images, const long long* desc, const int* tabs, const void* lut, void* tmp, void* rows,
                              int n_images, int patch, int merge, int temporal, long max_h_items, int max_tiles, int f32, void* stream);


/* ---- "precise" operand forms (ABI v4; UNetEngine(precise=True)) ----
 * north_star asks for UNet latents within 1e-3 relative of the reference; with every MFMA operand rounded to 11 significand bits one
 * evaluation sits at 1.2e-3. The per-site attribution (scripts/exp/precision_sites.py) puts ~70 % of that error variance on the few
 * places where the fp32 MASTER of the residual stream exists but its 16-bit shadow is what a kernel reads: ResnetBlock2D.conv_shortcut,
 * the Down / Upsample2D convs, conv_in / conv_out, Transformer2DModel.norm -> proj_in, proj_out, and every GroupNorm of the stream
 * (diffusers 0.25 UNet2DConditionModel.forward; call site custom_sd.py:634-639). These entry points read the fp32 tensor instead:
 *   spider_gemm_a32_*, spider_conv_nhwc_a32_*, spider_gemm_gn_in_a32_*: A (or the NHWC image) is fp32 and is split, on its way into
 *       LDS, into hi = round16(x) and lo = round16(x - hi); every K step runs two MFMAs (W.hi + W.lo). Otherwise the contracts of
 *       spider_gemm_* (no activation / GEGLU), spider_conv_nhwc_ex_* (no activation; w_tiled 0 / 1) and spider_gemm_gn_in_*.
 *   spider_gemm_ln_a32_*: LayerNorm(A32) . W^T (+ GEGLU) on the fp32 rows with gamma applied to A and W kept exact (spider_gemm_ln's
 *       fold re-rounds W * gamma); colsum[n] = sum_k gamma[k] W[n,k], colbias[n] = sum_k beta[k] W[n,k] + bias[n], both fp32.
 *   spider_groupnorm_f32in_nhwc_*: GroupNorm (+ SiLU) of the fp32 tensor x32 [B, HW, C]; statistics from `partial` [B, nchunk, G, 2]
 *       or (partial NULL) from a pass over x32 into ws (>= B * spider_groupnorm_nchunk(HW) * G * 2 floats); the result is rounded ONCE
 *       into y (16-bit, optional) and / or stored unrounded into y32 (optional).
 *   spider_split_hilo_f32_*: the operand split as a pass of its own (hi = round16(x), lo = round16(x - hi)) for convs large enough to run
 *       on the LDS-DMA / 256^2 kernels twice: conv(hi) (c32d out), then conv(lo) with res32 = that result -- the same fp32 sum.
 *   spider_row_split_f32_* / spider_groupnorm_f32in_split_nhwc_*: "split once, doubled K" -- the operand v (x32 itself, LayerNorm(x32)
 *       * gamma + beta with fp32 two-pass row statistics, or GroupNorm(x32) (+ SiLU)) is written ONCE as y2 [M, 2K] = [round16(v) |
 *       round16(v - round16(v))]; spider_gemm_* / spider_conv_nhwc_ex_* over y2 against the weight repeated along K ([W | W]: channels
 *       [0, Cin) and [Cin, 2 Cin) of every tap for a conv) accumulate hi . W + lo . W in their fp32 accumulator -- the product of the
 *       a32 entry points above on the LDS-DMA / 256^2 tile kernels, with every epilogue of those (GEGLU, rowbias, res32, c32d, GroupNorm
 *       statistics). The host side takes this route above a flop threshold (spider_amd/ops.py: A32_DUP_MIN_FLOP).
 *   spider_conv2d_small_cin_f32in_* / spider_conv2d_small_cout_f32in_*: conv_in on the fp32 NHWC latents (y32: optional fp32 master of
 *       its output) and conv_out on the fp32 GroupNorm + SiLU output.  spider_latent_to_nhwc_f32: fp32 NCHW latents -> fp32 NHWC. */
int spider_gemm_a32_bf16(const float* A32, const void* W, void* C, const void* bias, const void* res, int M, int N, int K, int lda,
                         int ldc, float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes, void* stream);
int spider_gemm_ln_a32_bf16(const float* A32, const void* W, void* C, const void* gamma, const float* colsum, const float* colbias,
                            int M, int N, int K, int ldc, int act, float eps, int w_tiled, void* stream);
int spider_gemm_gn_in_a32_bf16(const float* A32, const void* W, void* C, const void* bias, int M, int N, int K, int ldc, int w_tiled,
                               const float* gn_part, int nchunk, const void* gamma, const void* beta, int G, float eps, int HW,
                               float* c32d, void* stream);
int spider_conv_nhwc_a32_bf16(const float* x32, const void* w, void* y, const void* bias, const void* res, const void* rowbias,
                              int B, int Hin, int Win, int Cin, int Cout, int kh, int kw, int stride, int pad_h, int pad_w, int dil,
                              int up_h, int up_w, float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes,
                              void* stream);
int spider_groupnorm_f32in_nhwc_bf16(const float* x32, const float* partial, int nchunk, const void* gamma, const void* beta, void* y,
                                     float* y32, float* ws, int B, int HW, int C, int G, float eps, int silu, void* stream);
int spider_split_hilo_f32_bf16(const float* x, void* hi, void* lo, long n, void* stream);
int spider_row_split_f32_bf16(const float* x32, const void* gamma, const void* beta, void* y2, long M, int K, float eps, void* stream);
int spider_groupnorm_f32in_split_nhwc_bf16(const float* x32, const float* partial, int nchunk, const void* gamma, const void* beta,
                                            void* y2, float* ws, int B, int HW, int C, int G, float eps, int silu, void* stream);
int spider_conv2d_small_cin_f32in_bf16(const float* x32, const void* w, const void* bias, void* y, float* y32, int B, int H, int W,
                                       int Cin, int Cout, int ks, void* stream);
int spider_conv2d_small_cout_f32in_bf16(const float* x32, const void* w, const void* bias, float* y32, int B, int H, int W, int Cin,
                                        int Cout, int ks, void* stream);
int spider_latent_to_nhwc_f32(const float* lat, float* out, int B, int C, int HW, int reps, float scale, void* stream);

/* ======================= IEEE-half (f16) instantiations of the diffusion-side operators =======================
 * The reference runs its diffusion decoders in torch.float16 (spider_decoder.py:109,114,130,136,153,159; base_model.py:211;
 * StoryDiffusion/Comic_Generation.py:313). Every operator above that the UNet / VAE / text-encoder engines use also exists with
 * f16 tensors (raw uint16 IEEE-half bit patterns) in place of bf16: same arguments, same semantics, fp32 accumulation,
 * mfma_f32_*_f16 at the bf16 rate; outputs beyond +-65504 round to +-inf as torch.float16 does. The LLM decode operators
 * exist in bf16 only (the reference's LLM dtype). */
int spider_gemm_f16(const void* A, const void* W, void* C, void* C32, const void* bias, const void* res,
                     const void* rowbias, int rows_per_group, int M, int N, int K, int lda, int ldc, int act,
                     float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes, void* stream);
int spider_gemm_ln_f16(const void* A, const void* Wf, void* C, const float* colsum, const float* colbias, const void* res,
                        int M, int N, int K, int ldc, int act, float eps, int w_tiled, void* ws, long ws_bytes, void* stream);
int spider_xattn_fused_f16(const void* x, const void* mq_fm, const void* mo_fm, const float* colsum, const float* colbias,
                            const void* bias_o, void* out, int B2, int n_tok, int C, int heads, int n_keys, float eps,
                            const float* x32, float* out32, void* stream);
int spider_conv2d_nhwc_f16(const void* x, const void* w, void* y, const void* bias, const void* res,
                            const void* rowbias, int B, int Hin, int Win, int Cin, int Cout, int ks, int stride,
                            int pad, int ups, float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes, void* stream);
int spider_conv_nhwc_ex_f16(const void* x, const void* w, void* y, const void* bias, const void* res,
                             const void* rowbias, int B, int Hin, int Win, int Cin, int Cout, int kh, int kw, int stride,
                             int pad_h, int pad_w, int dil, int up_h, int up_w, int act, float act_param,
                             float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes, void* stream);
int spider_attn_f16(const void* q, const void* k, const void* v, void* o,
                     long q_bs, long q_hs, long q_rs, long k_bs, long k_hs, long k_rs,
                     long v_bs, long v_hs, long v_rs, long o_bs, long o_hs, long o_rs,
                     int B, int Hq, int Hkv, int Lq, int Lk, int d, float scale, int causal, int kv_off,
                     const int* kv_beg, const void* keep_bits, int blk, int q_off, void* stream);
int spider_attn_keylist_f16(const void* q, const void* k, const void* v, void* o,
                             long q_bs, long q_hs, long q_rs, long k_bs, long k_hs, long k_rs,
                             long v_bs, long v_hs, long v_rs, long o_bs, long o_hs, long o_rs,
                             int B, int Hq, int Hkv, int Lq, int Lk, int d, float scale,
                             const int* key_idx, int idx_len, const int* tiles, int n_tiles, void* stream);
int spider_attn_varlen_f16(const void* q, const void* k, const void* v, void* o, long q_rs, long k_rs, long v_rs, long o_rs,
                            int total_rows, int Hq, int Hkv, int d, float scale, const int* tiles, int n_tiles, void* stream);
int spider_groupnorm_nhwc_f16(const void* x, const void* gamma, const void* beta, void* y, void* ws, int B, int HW,
                               int C, int G, float eps, int silu, void* stream);
int spider_conv_nhwc_gn_f16(const void* x, const void* w, void* y, const void* bias, const void* res, const void* rowbias,
                            int B, int Hin, int Win, int Cin, int Cout, int kh, int kw, int stride, int pad_h, int pad_w,
                            int dil, int up_h, int up_w, int act, float act_param, float out_scale, int w_tiled,
                            const float* res32, float* c32d, void* ws, long ws_bytes, void* stream,
                            float* gn_part, int gn_groups, int* produced);
int spider_groupnorm_stats_nhwc_f16(const void* x, void* partial, int B, int HW, int C, int G, int nchunk, void* stream);
int spider_groupnorm_apply_nhwc_f16(const void* x, const void* partial, int nchunk, const void* gamma, const void* beta, void* y,
                                    int B, int HW, int C, int G, float eps, int silu, void* stream);
int spider_gemm_gn_in_f16(const void* A, const void* W, void* C, const void* bias, int M, int N, int K, int ldc, int w_tiled,
                          const float* gn_part, int nchunk, const void* gamma, const void* beta, int G, float eps, int HW,
                          float* c32d, void* stream);
int spider_groupnorm_cat_nhwc_f16(const void* x1, const void* x2, const void* gamma, const void* beta, void* y, void* cat,
                                   void* ws, int B, int HW, int C1, int C2, int G, float eps, int silu, void* stream);
int spider_layernorm_f16(const void* x, const void* gamma, const void* beta, void* y, int rows, int C, float eps,
                          void* stream);
int spider_geglu_f16(const void* x, void* y, int M, int inner, void* stream);
int spider_swiglu_f16(const void* x, void* y, int M, int inner, void* stream);
int spider_concat_channels_f16(const void* a, const void* b, void* y, long rows, int C1, int C2, void* stream);
int spider_act_f16(const void* x, void* y, long n, int act, void* stream);
int spider_add_f16(const void* a, const void* b, void* y, long n, void* stream);
int spider_act_ex_f16(const void* x, void* y, long n, int act, float param, void* stream);
int spider_add_scaled_f16(const void* a, const void* b, void* y, long n, float scale, void* stream);
int spider_axpby_f16(const void* a, const void* b, void* y, long n, float alpha, float beta, void* stream);
int spider_mean_tokens_f16(const void* x, void* y, int B, int T, int C, void* stream);
int spider_moe_combine_f16(const void* const* host_xs, int E, const void* logits, int ld, void* y, int B, long per_batch,
                            void* stream);
int spider_col2im1d_f32_f16(const float* cols, const void* bias, void* y, int B, int L_in, int k, int stride, int pad,
                             int Cout, void* stream);
int spider_l2_normalize_rows_f16(const void* x, void* y, int rows, int n, float eps, void* stream);
int spider_conv2d_small_cin_f16(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int Cin,
                                 int Cout, int ks, void* stream);
int spider_conv2d_small_cout_f16(const void* x, const void* w, const void* bias, void* y32, void* y16, int B, int H,
                                  int W, int Cin, int Cout, int ks, void* stream);
int spider_latent_to_nhwc_f16(const float* lat, void* out, int B, int C, int HW, int reps, float scale, void* stream);
int spider_softmax_rows_f32_f16(const float* x, void* y, int rows, int n, int n_valid, float scale, void* stream);

int spider_gemm_a32_f16(const float* A32, const void* W, void* C, const void* bias, const void* res, int M, int N, int K, int lda,
                         int ldc, float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes, void* stream);
int spider_gemm_ln_a32_f16(const float* A32, const void* W, void* C, const void* gamma, const float* colsum, const float* colbias,
                            int M, int N, int K, int ldc, int act, float eps, int w_tiled, void* stream);
int spider_gemm_gn_in_a32_f16(const float* A32, const void* W, void* C, const void* bias, int M, int N, int K, int ldc, int w_tiled,
                               const float* gn_part, int nchunk, const void* gamma, const void* beta, int G, float eps, int HW,
                               float* c32d, void* stream);
int spider_conv_nhwc_a32_f16(const float* x32, const void* w, void* y, const void* bias, const void* res, const void* rowbias,
                              int B, int Hin, int Win, int Cin, int Cout, int kh, int kw, int stride, int pad_h, int pad_w, int dil,
                              int up_h, int up_w, float out_scale, int w_tiled, const float* res32, float* c32d, void* ws, long ws_bytes,
                              void* stream);
int spider_groupnorm_f32in_nhwc_f16(const float* x32, const float* partial, int nchunk, const void* gamma, const void* beta, void* y,
                                     float* y32, float* ws, int B, int HW, int C, int G, float eps, int silu, void* stream);
int spider_split_hilo_f32_f16(const float* x, void* hi, void* lo, long n, void* stream);
int spider_row_split_f32_f16(const float* x32, const void* gamma, const void* beta, void* y2, long M, int K, float eps, void* stream);
int spider_groupnorm_f32in_split_nhwc_f16(const float* x32, const float* partial, int nchunk, const void* gamma, const void* beta,
                                            void* y2, float* ws, int B, int HW, int C, int G, float eps, int silu, void* stream);
int spider_conv2d_small_cin_f32in_f16(const float* x32, const void* w, const void* bias, void* y, float* y32, int B, int H, int W,
                                       int Cin, int Cout, int ks, void* stream);
int spider_conv2d_small_cout_f32in_f16(const float* x32, const void* w, const void* bias, float* y32, int B, int H, int W, int Cin,
                                        int Cout, int ks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPIDER_HIP_H */
