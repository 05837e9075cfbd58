// Cosine top-k of query rows against a small table of candidate representations:
// /root/reference/evaluate.py:65-117 (get_filter_text_results) ranks the 214 phrase representations of
// filter_answers.json against every Filter output with nn.CosineSimilarity + argsort and keeps the first 10.
//
// One wave per query.  The query (H <= 1024 floats) sits in registers, H/64 per lane; the candidate table (C x H, 438 KB
// at 214 x 512) is read coalesced from L2 by every wave; one butterfly reduction per candidate leaves the similarity
// in all lanes, and lane c % 64 keeps it.  Selection is k rounds of a wave-wide arg-max (ties: lower index), so
// the kernel is bound by C wave reductions per query, not by memory: n*C*H*4 bytes of L2 reads, n*k*8 bytes written.
#include "common.h"
#include "cosine_rank.h"
#include "ops.h"

namespace stair {

__global__ __launch_bounds__(256) void key_invnorm_kernel(const float *keys, float *inv, int C, int H) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;
    const float v = key_invnorm(keys, c, H, lane);
    if (lane == 0) inv[c] = v;
}

__global__ __launch_bounds__(256) void cosine_topk_kernel(const float *queries, int64_t ldq, const int32_t *q_idx,
                                                          const float *keys, const float *kinv, int n, int C, int H,
                                                          int k, int32_t *out_idx, float *out_sim) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= n) return;
    const float *qp = queries + (int64_t)(q_idx ? q_idx[q] : q) * ldq;
    float sims[TK_SLOTS];
    cosine_sims(qp, keys, kinv, C, H, lane, sims);       // csrc/cosine_rank.h
    cosine_select(sims, C, k, lane, out_idx + (int64_t)q * k, out_sim + (int64_t)q * k);
}

}  // namespace stair

extern "C" int stair_cosine_topk(const float *queries, int64_t ldq, const int32_t *q_idx, const float *keys,
                                 float *key_invnorm_ws, int32_t n, int32_t C, int32_t H, int32_t k, int32_t *out_idx,
                                 float *out_sim, stair_stream stream) {
    using namespace stair;
    STAIR_CHECK(queries && keys && key_invnorm_ws && out_idx && out_sim, "null argument");
    STAIR_CHECK(n >= 0 && C > 0 && H > 0, "bad sizes");
    STAIR_CHECK(C <= 64 * TK_SLOTS, "at most 1024 candidates");
    STAIR_CHECK(k > 0 && k <= C, "k must be in 1..C");
    STAIR_CHECK(ldq >= H && (ldq % 4 == 0) && (reinterpret_cast<uintptr_t>(queries) % 16 == 0) &&
                    (reinterpret_cast<uintptr_t>(keys) % 16 == 0),
                "queries/keys must be 16-byte aligned with ldq a multiple of 4");
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(key_invnorm_kernel, dim3((C + 3) / 4), dim3(256), 0, s, keys, key_invnorm_ws, C, H);
    STAIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(cosine_topk_kernel, dim3((n + 3) / 4), dim3(256), 0, s, queries, ldq, q_idx, keys, key_invnorm_ws, n,
                       C, H, k, out_idx, out_sim);
    STAIR_LAUNCH_CHECK();
    return 0;
}
