// Assisted decoding (transformers `generate(assistant_model=draft, num_assistant_tokens=K)`) for one greedy sequence: a small DRAFT
// engine of the same tokenizer family proposes K tokens one by one, the target engine verifies them as the K + 1 rows of one
// multi-row step (spec_decode.hip: attn_verify, and the engine's R-row weight route), and the agreed prefix plus the target's own
// token join the sequence. Two launches are specific to it; they carry tokens and cursors between the two engines on the device:
//   spider_spec_assist_push_i32      behind a draft step: the drafted token becomes row j of the target's verify step and the input of
//                                    the draft engine's next single-row step
//   spider_spec_assist_advance_i32   behind the verify step: accept (spec_accept.hpp), append, advance, count, and write the two
//                                    catch-up rows of the draft engine's next round
// int32 buffers, int64 counters, one block per sequence, plain vector stores, nothing written outside the sequence's own rows.
#include "common.hpp"
#include "spec_accept.hpp"

using namespace spider;

constexpr int ASSIST_THREADS = 64;      // one wave: the work is a handful of ints per sequence
constexpr int ASSIST_MAX_R = 8;         // rows per sequence of the verify step (spec_decode.hip SPEC_MAX_R)

// an id the draft engine may embed: ids outside its (smaller) vocabulary read row 0 of its table -- for the draft engine only
__device__ __forceinline__ int assist_draft_id(int t, int vd) { return (t >= 0 && t < vd) ? t : 0; }

// ----------------------------------------------------------------------------------------------
// Push. src_out / src_pos / src_slot [B * Rs]: the draft step that just ran (Rs rows per sequence; row rs is the one whose arg-max
// src_out is draft number j). The drafted token sits one position and one slot behind its source row, so the offset between
// position and slot of a left-padded prompt is carried along:
//   t_ids / t_pos / t_slot [B * R], row j    <- (token, src_pos + 1, src_slot + 1)                        the target's verify row
//   d_ids / d_pos / d_slot / d_kv_end [B]    <- (token below vd else 0, src_pos + 1, src_slot + 1, src_slot + 2)   the draft's next row
// The destination of the draft side may be the source's own buffers (a single-row step feeding itself): one thread reads, then writes.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ASSIST_THREADS) void spec_assist_push_kernel(const int* src_out, const int* src_pos, const int* src_slot,
                                                                         int Rs, int rs, int* t_ids, int* t_pos, int* t_slot, int R,
                                                                         int j, int* d_ids, int* d_pos, int* d_slot, int* d_kv_end,
                                                                         int vd) {
    if (threadIdx.x != 0) return;
    const size_t b = blockIdx.x;
    const size_t s = b * Rs + rs, t = b * R + j;
    const int tok = src_out[s], p = src_pos[s] + 1, sl = src_slot[s] + 1;
    t_ids[t] = tok;
    t_pos[t] = p;
    t_slot[t] = sl;
    d_ids[b] = assist_draft_id(tok, vd);
    d_pos[b] = p;
    d_slot[b] = sl;
    d_kv_end[b] = sl + 1;       // the row's own K / V row is the last one it sees
}

// ----------------------------------------------------------------------------------------------
// Advance. Row layout as in spec_decode.hip: ids / pos / slot / lm_out [B * R], row b * R the last accepted token, rows 1 ... n_draft[b]
// the drafts, lm_out[r] the target's greedy token behind row r.
//   a = spec_accept_len;  hist[b] gets lm_out[0 .. a] (slots at or past cap are dropped), n_hist, kv_end, pos[0], slot[0] += a + 1,
//   ids[0] = lm_out[a], counters[b] += (1, n_draft[b], a).  Rows 1 ... R - 1 of ids / pos / slot are left to the next round's pushes.
// The sequence now ends ... ids[a], lm_out[a] (row a is the last row whose token was kept), and the draft engine has consumed at
// most the token in front of ids[a] with certainty, so its next round starts with a two-row step on exactly these two:
//   d_ids [B * 2] = (ids[a], lm_out[a]) below vd else 0;  d_pos = (pos[0] + a, pos[0] + a + 1);  d_slot likewise;
//   d_kv_end [B] = slot[0] + a + 1   (row 0 of the two sees the cache up to its own slot, row 1 one more: attn_verify's rule)
// Every thread reads what it needs before anything it reads is written: the accept loop reads lm_out and ids[1 ...], which this
// kernel never writes; ids[0], pos[0], slot[0] are read and written by thread 0 alone.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ASSIST_THREADS) void spec_assist_advance_kernel(const int* __restrict__ lm_out, int* ids, int* pos,
                                                                            int* slot, int* __restrict__ kv_end,
                                                                            const int* __restrict__ n_draft, int* __restrict__ hist,
                                                                            int* __restrict__ n_hist, int cap,
                                                                            long long* __restrict__ counters, int R,
                                                                            int* __restrict__ d_ids, int* __restrict__ d_pos,
                                                                            int* __restrict__ d_slot, int* __restrict__ d_kv_end,
                                                                            int vd) {
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int* lm_b = lm_out + b * R;
    int* const ids_b = ids + b * R;
    int nd = n_draft[b];
    nd = nd < 0 ? 0 : (nd > R - 1 ? R - 1 : nd);
    const int a = spec_accept_len(lm_b, ids_b, nd, R);
    const int nh = max(n_hist[b], 0);
    if (tid <= a) {                 // a + 1 <= R <= 8 threads append
        const int j = nh + tid;
        if (j < cap) hist[b * cap + j] = lm_b[tid];
    }
    if (tid != 0) return;
    const int pos0 = pos[b * R], slot0 = slot[b * R];
    const int prev = ids_b[a], last = lm_b[a];
    ids_b[0] = last;
    pos[b * R] = pos0 + a + 1;
    slot[b * R] = slot0 + a + 1;
    kv_end[b] += a + 1;
    n_hist[b] = nh + a + 1;
    counters[b * 3] += 1;
    counters[b * 3 + 1] += nd;
    counters[b * 3 + 2] += a;
    d_ids[b * 2] = assist_draft_id(prev, vd);
    d_ids[b * 2 + 1] = assist_draft_id(last, vd);
    d_pos[b * 2] = pos0 + a;
    d_pos[b * 2 + 1] = pos0 + a + 1;
    d_slot[b * 2] = slot0 + a;
    d_slot[b * 2 + 1] = slot0 + a + 1;
    d_kv_end[b] = slot0 + a + 1;
}

extern "C" {

int spider_spec_assist_push_i32(const int* src_out, const int* src_pos, const int* src_slot, int Rs, int rs, int* t_ids, int* t_pos,
                                int* t_slot, int R, int j, int* d_ids, int* d_pos, int* d_slot, int* d_kv_end, int draft_vocab,
                                int B, void* stream) {
    SPIDER_CHECK(src_out && src_pos && src_slot && t_ids && t_pos && t_slot && d_ids && d_pos && d_slot && d_kv_end,
                 "spec_assist_push: source rows [B * Rs], target rows [B * R] and the draft's next row [B] are required");
    SPIDER_CHECK(B > 0 && Rs >= 1 && Rs <= ASSIST_MAX_R && rs >= 0 && rs < Rs, "spec_assist_push: source row must lie in 0 ... Rs - 1, Rs in 1 ... 8");
    SPIDER_CHECK(R >= 2 && R <= ASSIST_MAX_R && j >= 1 && j < R, "spec_assist_push: draft row must lie in 1 ... R - 1, rows per sequence in 2 ... 8");
    SPIDER_CHECK(draft_vocab > 0, "spec_assist_push: draft_vocab must be positive");
    spec_assist_push_kernel<<<B, ASSIST_THREADS, 0, (hipStream_t)stream>>>(src_out, src_pos, src_slot, Rs, rs, t_ids, t_pos, t_slot, R,
                                                                          j, d_ids, d_pos, d_slot, d_kv_end, draft_vocab);
    SPIDER_LAUNCH_OK();
    return 0;
}

int spider_spec_assist_advance_i32(const int* lm_out, int* ids, int* pos, int* slot, int* kv_end, const int* n_draft, int* hist,
                                   int* n_hist, int cap, void* counters, int R, int* d_ids, int* d_pos, int* d_slot, int* d_kv_end,
                                   int draft_vocab, int B, void* stream) {
    SPIDER_CHECK(lm_out && ids && pos && slot && kv_end && n_draft && hist && n_hist && counters,
                 "spec_assist_advance: lm_out, ids, pos, slot [B * R], kv_end, n_draft, n_hist [B], hist [B, cap] and counters int64 [B, 3] are required");
    SPIDER_CHECK(d_ids && d_pos && d_slot && d_kv_end, "spec_assist_advance: the draft's catch-up rows [B * 2] and kv_end [B] are required");
    SPIDER_CHECK(B > 0 && cap > 0 && R >= 2 && R <= ASSIST_MAX_R, "spec_assist_advance: rows per sequence must be 2 ... 8, B and cap > 0");
    SPIDER_CHECK(draft_vocab > 0, "spec_assist_advance: draft_vocab must be positive");
    spec_assist_advance_kernel<<<B, ASSIST_THREADS, 0, (hipStream_t)stream>>>(lm_out, ids, pos, slot, kv_end, n_draft, hist, n_hist, cap,
                                                                             (long long*)counters, R, d_ids, d_pos, d_slot, d_kv_end,
                                                                             draft_vocab);
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"
