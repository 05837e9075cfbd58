// Audit decoders: the supervised intermediate results of a finished pass as something a person reads -- the frame interval of an
// attention row, the yes/no of a pretrain head, the rank of the gold class in a class table -- scored against gold where there is
// gold (include/stair_hip.h, "Audit decoders").  They read the plan's arenas and write arrays of their own.
//
// One wave per item in all three; items are a few per question and rows short, so the attention and head kernels move a few MB and
// are latency bound; the rank kernel is stair_cosine_topk's (csrc/cosine_rank.h) with the class norms formed per workgroup in LDS and
// two more wave reductions per item for the gold rank: n * n_cls * H * 4 bytes of L2 reads.  No atomics, no memset: every output
// slot is stored by the wave that owns it, on every launch.
#include "common.h"
#include "cosine_rank.h"
#include "span_gold.h"

#include <cmath>

namespace stair {

namespace {
constexpr int kAuditBlock = 256;
constexpr int kAuditWaves = kAuditBlock / 64;
__device__ __forceinline__ float audit_nan() { return __int_as_float(0x7fc00000); }
}  // namespace

// One wave per item, its K rows one after the other; a row goes through the wave in chunks of 64 frames, twice: the first pass finds
// the peak and counts the on-frames (one ballot per chunk), the second finds the ends of the run around the peak from the chunks'
// off-frame ballots by bit scans -- the last off-frame below the peak and the first above it, whichever chunk they lie in, so a run
// across a chunk boundary is nothing special.  The row is re-read from L1.
__global__ __launch_bounds__(kAuditBlock) void audit_attention_kernel(const float *att, int att_rows, const int32_t *slot, const int32_t *K,
                                                                      const int32_t *len, const int32_t *iv_off, const double *intervals,
                                                                      const int32_t *has_gold, int n, int T, float threshold,
                                                                      int32_t *o_start, int32_t *o_end, int32_t *o_peak, int32_t *o_on,
                                                                      float *o_peak_value, float *o_iou) {
    const int i = blockIdx.x * kAuditWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int rows = K[i], row0 = iv_off[i];
    const int L = min(max(len ? len[i] : T, 0), T);
    const bool gold = intervals && (!has_gold || has_gold[i] != 0);
    const int chunks = (L + 63) >> 6;
    for (int r = 0; r < rows; ++r) {
        const int64_t arow = (int64_t)slot[i] + r;
        const bool readable = arow >= 0 && arow < att_rows;
        const float *a = att + (readable ? arow : 0) * T;
        // ---- pass 1: peak (first index of the largest comparable value) and the on-frame count
        float best = 0.f;
        int bi = -1, n_on = 0;
        for (int c = 0; c < chunks; ++c) {
            const int t = c * 64 + lane;
            const bool valid = readable && t < L;
            const float v = valid ? a[t] : audit_nan();
            if (v == v && (bi < 0 || v > best)) { best = v; bi = t; }          // t grows: the first of equal values stays
            n_on += __popcll(__ballot(v >= threshold));                        // NaN >= x is false
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi >= 0 && (bi < 0 || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
        }
        const int peak = bi;
        // ---- pass 2: the run of on-frames around the peak
        int last_off = -1, first_off = -1;                                     // off-frames below / above the peak (wave-uniform)
        bool peak_on = false;
        if (peak >= 0) {
            peak_on = best >= threshold;
            for (int c = 0; c < chunks; ++c) {
                const int t = c * 64 + lane;
                const bool valid = t < L;
                const float v = valid ? a[t] : audit_nan();
                const unsigned long long off = __ballot(valid && !(v >= threshold));
                const int lo = peak - c * 64;                                  // bits below lo are frames before the peak
                const unsigned long long below = lo <= 0 ? 0ull : (lo >= 64 ? off : off & ((1ull << lo) - 1ull));
                if (below) last_off = c * 64 + 63 - __clzll((long long)below);
                const int hi = peak + 1 - c * 64;                              // bits from hi on are frames after the peak
                const unsigned long long above = hi <= 0 ? off : (hi >= 64 ? 0ull : off & ~((1ull << hi) - 1ull));
                if (above && first_off < 0) first_off = c * 64 + __ffsll((long long)above) - 1;
            }
        }
        const int start = peak < 0 ? 0 : (peak_on ? last_off + 1 : peak);
        const int end = peak < 0 ? 0 : (peak_on ? (first_off < 0 ? L : first_off) : peak);
        // ---- IoU of the 0/1 mask of [start, end) with the criterion's soft gold mask
        float iou = -1.0f;
        if (gold) {
            const double *iv = intervals + 2 * ((int64_t)row0 + r);
            const double g0 = iv[0], g1 = iv[1];
            float num = 0.f, den = 0.f;
            for (int t = lane; t < L; t += 64) {
                const float g = span_gold(g0, g1, L, t);
                const float m = (t >= start && t < end) ? 1.0f : 0.0f;
                num += m * g;
                den += fmaxf(m, g);
            }
            num = wave_sum(num); den = wave_sum(den);
            iou = den > 0.f ? num / den : 0.0f;
        }
        if (lane == 0) {
            const int64_t o = (int64_t)row0 + r;
            o_start[o] = start; o_end[o] = end; o_peak[o] = peak; o_on[o] = n_on;
            o_peak_value[o] = peak < 0 ? audit_nan() : best;
            o_iou[o] = iou;
        }
    }
}

template <int NOUT>
__global__ __launch_bounds__(kAuditBlock) void audit_head_kernel(const float *vec, int vec_rows, const int32_t *slot, const int32_t *label,
                                                                 const float *W, const float *b, int n, int H, int32_t *o_pred,
                                                                 float *o_score, int32_t *o_correct) {
    const int i = blockIdx.x * kAuditWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int sl = slot[i];
    const bool readable = sl >= 0 && sl < vec_rows;
    const float *x = vec + (int64_t)(readable ? sl : 0) * H;
    float z[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        float d = 0.f;
        for (int c = lane; c < H; c += 64) d += x[c] * W[(int64_t)j * H + c];
        z[j] = wave_sum(d) + b[j];
    }
    const float score = readable ? (NOUT == 2 ? z[NOUT - 1] - z[0] : z[0]) : audit_nan();
    const int pred = NOUT == 2 ? (score > 0.0f) : (score >= 0.5f);             // the decision of the stored score
    if (lane == 0) {
        const int lab = label ? label[i] : -1;
        o_pred[i] = pred; o_score[i] = score;
        o_correct[i] = lab < 0 ? -1 : (pred == (lab != 0));
    }
}

// The class norms first, once per workgroup: wave w takes classes w, w + 4, .. into LDS (the sums of key_invnorm_kernel, so the
// similarities are stair_cosine_topk's bits).  Every wave of the workgroup reaches the barrier, items past n included.
__global__ __launch_bounds__(kAuditBlock) void audit_rank_kernel(const float *vec, int vec_rows, const int32_t *slot, const float *reps, int C,
                                                                 int H, const int32_t *gold_off, const int32_t *gold_cls, int n, int k,
                                                                 int32_t *o_top, float *o_top_sim, int32_t *o_rank, float *o_best_gold) {
    __shared__ float kinv[64 * TK_SLOTS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = wave; c < C; c += kAuditWaves) {
        const float v = key_invnorm(reps, c, H, lane);
        if (lane == 0) kinv[c] = v;
    }
    __syncthreads();
    const int i = blockIdx.x * kAuditWaves + wave;
    if (i >= n) return;
    const int sl = slot[i];
    if (sl < 0 || sl >= vec_rows) {                                            // unreadable item
        for (int r = lane; r < k; r += 64) { o_top[(int64_t)i * k + r] = -1; o_top_sim[(int64_t)i * k + r] = audit_nan(); }
        if (lane == 0) { o_rank[i] = 0; o_best_gold[i] = -INFINITY; }
        return;
    }
    float sims[TK_SLOTS];
    cosine_sims(vec + (int64_t)sl * H, reps, kinv, C, H, lane, sims);
    // the best similarity among the item's gold classes: the lane that holds a gold class offers it
    const int g0 = gold_off ? gold_off[i] : 0, g1 = gold_off ? gold_off[i + 1] : 0;
    float g = -INFINITY;
    bool any = false;
    for (int e = g0; e < g1; ++e) {
        const int c = gold_cls[e];
        if (c < 0 || c >= C) continue;                                         // (the launcher refuses it where it sees the host copy)
        any = true;
#pragma unroll
        for (int t = 0; t < TK_SLOTS; ++t)
            if (t == (c >> 6) && (c & 63) == lane) g = fmaxf(g, sims[t]);
    }
    g = wave_max(g);
    int better = 0;
#pragma unroll
    for (int t = 0; t < TK_SLOTS; ++t) better += __popcll(__ballot(t * 64 + lane < C && sims[t] > g));
    if (lane == 0) { o_rank[i] = any ? 1 + better : 0; o_best_gold[i] = any ? g : -INFINITY; }
    cosine_select(sims, C, k, lane, o_top + (int64_t)i * k, o_top_sim + (int64_t)i * k);
}

}  // namespace stair

extern "C" int stair_audit_attention(const float *att, int32_t att_rows, const int32_t *slot, const int32_t *K, const int32_t *len,
                                     const int32_t *iv_off, const double *intervals, const int32_t *has_gold, int32_t n, int32_t T,
                                     float threshold, int32_t *start, int32_t *end, int32_t *peak, int32_t *on, float *peak_value,
                                     float *iou, stair_stream stream) {
    using namespace stair;
    STAIR_CHECK(n >= 0, "n must not be negative");
    STAIR_CHECK(T >= 1, "T must be at least 1");
    STAIR_CHECK(!std::isnan(threshold), "the threshold is NaN");
    if (n == 0) return 0;
    STAIR_CHECK(att && att_rows > 0, "null att arena");
    STAIR_CHECK(slot && K && iv_off, "null slot / K / iv_off");
    STAIR_CHECK(start && end && peak && on && peak_value && iou, "null output");
    hipLaunchKernelGGL(audit_attention_kernel, dim3((n + kAuditWaves - 1) / kAuditWaves), dim3(kAuditBlock), 0, static_cast<hipStream_t>(stream),
                       att, att_rows, slot, K, len, iv_off, intervals, has_gold, n, T, threshold, start, end, peak, on, peak_value, iou);
    STAIR_LAUNCH_CHECK();
    return 0;
}

extern "C" int stair_audit_head(int32_t nout, const float *vec, int32_t vec_rows, const int32_t *slot, const int32_t *label,
                                const float *W, const float *b, int32_t n, int32_t H, int32_t *pred, float *score, int32_t *correct,
                                stair_stream stream) {
    using namespace stair;
    STAIR_CHECK(nout == 1 || nout == 2, "head width must be 1 (Equals) or 2 (Exists/Xor)");
    STAIR_CHECK(n >= 0, "n must not be negative");
    STAIR_CHECK(H >= 1, "H must be at least 1");
    if (n == 0) return 0;
    STAIR_CHECK(vec && vec_rows > 0, "null vec arena");
    STAIR_CHECK(slot && W && b, "null slot / W / b");
    STAIR_CHECK(pred && score && correct, "null output");
    const dim3 grid((n + kAuditWaves - 1) / kAuditWaves), block(kAuditBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nout == 2) hipLaunchKernelGGL(audit_head_kernel<2>, grid, block, 0, s, vec, vec_rows, slot, label, W, b, n, H, pred, score, correct);
    else hipLaunchKernelGGL(audit_head_kernel<1>, grid, block, 0, s, vec, vec_rows, slot, label, W, b, n, H, pred, score, correct);
    STAIR_LAUNCH_CHECK();
    return 0;
}

extern "C" int stair_audit_rank(const float *vec, int32_t vec_rows, const int32_t *slot, const float *reps, int32_t n_cls, int32_t H,
                                const int32_t *gold_off, const int32_t *gold_cls, const int32_t *gold_cls_host, int32_t n_gold,
                                int32_t n, int32_t k, int32_t *top, float *top_sim, int32_t *rank, float *best_gold_sim,
                                stair_stream stream) {
    using namespace stair;
    STAIR_CHECK(n >= 0, "n must not be negative");
    STAIR_CHECK(H >= 1, "H must be at least 1");
    STAIR_CHECK(n_cls >= 1, "the class table is empty");
    STAIR_CHECK(n_cls <= 64 * TK_SLOTS, "at most 1024 classes");
    STAIR_CHECK(k >= 1 && k <= n_cls, "k must be in 1..n_cls");
    STAIR_CHECK(n_gold >= 0, "n_gold must not be negative");
    if (gold_cls_host)
        for (int32_t e = 0; e < n_gold; ++e)
            if (gold_cls_host[e] < 0 || gold_cls_host[e] >= n_cls)
                STAIR_FAIL("gold class " + std::to_string(gold_cls_host[e]) + " (entry " + std::to_string(e) + ") is outside the table of " +
                           std::to_string(n_cls) + " classes");
    if (n == 0) return 0;
    STAIR_CHECK(vec && vec_rows > 0, "null vec arena");
    STAIR_CHECK(slot && reps, "null slot / reps");
    STAIR_CHECK(!gold_off || n_gold == 0 || gold_cls, "gold_off without gold_cls");
    STAIR_CHECK(top && top_sim && rank && best_gold_sim, "null output");
    STAIR_CHECK((reinterpret_cast<uintptr_t>(vec) % 16 == 0) && (reinterpret_cast<uintptr_t>(reps) % 16 == 0), "vec and reps must be 16-byte aligned");
    hipLaunchKernelGGL(audit_rank_kernel, dim3((n + kAuditWaves - 1) / kAuditWaves), dim3(kAuditBlock), 0, static_cast<hipStream_t>(stream),
                       vec, vec_rows, slot, reps, n_cls, H, gold_off, gold_cls, n, k, top, top_sim, rank, best_gold_sim);
    STAIR_LAUNCH_CHECK();
    return 0;
}
