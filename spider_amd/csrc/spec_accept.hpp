// The acceptance rule of a verify step (llm.spec_accept_host), shared by spec_decode.hip (prompt-lookup drafts) and
// spec_assist.hip (drafts of an assistant model).
#pragma once

namespace spider {

// ids_b / lm_out_b: the R rows of one sequence (ids_b[0] the last accepted token, ids_b[1 .. nd] its drafted successors, lm_out_b[r]
// the model's greedy token behind row r). Returns the largest j <= nd with lm_out_b[i - 1] == ids_b[i] for all 1 <= i <= j.
// Every thread of the block works it out for itself from the step's 2 R ints (uniform loads); nd <= R - 1.
__device__ __forceinline__ int spec_accept_len(const int* lm_out_b, const int* ids_b, int nd, int R) {
    int a = 0;
    bool ok = true;
    for (int i = 1; i < R; ++i) {
        ok = ok && i <= nd && lm_out_b[i - 1] == ids_b[i];
        if (ok) a = i;
    }
    return a;
}

}  // namespace spider
