// Cosine similarities of one query row against a small class table, one wave per query, and the selection of the k best: the
// device code shared by stair_cosine_topk (csrc/topk.hip) and stair_audit_rank (csrc/audit.hip), so that both rank by the same
// fp32 numbers.  The query (H <= 1024 floats when H % 256 == 0) sits in registers, H/64 per lane; the table is read coalesced from
// L2; one butterfly reduction per class leaves the similarity in all lanes, and lane c % 64 keeps it in slot c / 64.
#pragma once
#include "common.h"

namespace stair {

constexpr int TK_MAXJ = 4;       // H <= 1024: float4 groups per lane
constexpr int TK_SLOTS = 16;     // C <= 1024: candidates per lane

// 1 / max(|keys[c]|, 1e-8): nn.CosineSimilarity's eps, per operand; the same value in every lane
__device__ __forceinline__ float key_invnorm(const float *keys, int c, int H, int lane) {
    float s = 0.0f;
    for (int h = lane; h < H; h += 64) { const float v = keys[(int64_t)c * H + h]; s += v * v; }
    s = wave_sum(s);
    return 1.0f / fmaxf(sqrtf(s), 1e-8f);
}

// sims[c / 64] of lane c % 64 = cos(qp, keys[c]) for c < C, -inf elsewhere; kinv [C] (global or LDS) = key_invnorm of every class
__device__ __forceinline__ void cosine_sims(const float *qp, const float *keys, const float *kinv, int C, int H, int lane,
                                            float (&sims)[TK_SLOTS]) {
    const int nj = H >> 8;                     // full float4 groups per lane (H % 256 == 0 fast path)
    const bool vec = (H & 255) == 0 && nj <= TK_MAXJ;
    float4 qv[TK_MAXJ];
    float qn = 0.0f;
    if (vec) {
#pragma unroll
        for (int j = 0; j < TK_MAXJ; ++j)
            if (j < nj) {
                qv[j] = *reinterpret_cast<const float4 *>(qp + j * 256 + lane * 4);
                qn += qv[j].x * qv[j].x + qv[j].y * qv[j].y + qv[j].z * qv[j].z + qv[j].w * qv[j].w;
            }
    } else {
        for (int h = lane; h < H; h += 64) qn += qp[h] * qp[h];
    }
    const float qinv = 1.0f / fmaxf(sqrtf(wave_sum(qn)), 1e-8f);

#pragma unroll
    for (int t = 0; t < TK_SLOTS; ++t) sims[t] = -INFINITY;
    for (int c = 0; c < C; ++c) {
        const float *kp = keys + (int64_t)c * H;
        float d = 0.0f;
        if (vec) {
#pragma unroll
            for (int j = 0; j < TK_MAXJ; ++j)
                if (j < nj) {
                    const float4 kv = *reinterpret_cast<const float4 *>(kp + j * 256 + lane * 4);
                    d += qv[j].x * kv.x + qv[j].y * kv.y + qv[j].z * kv.z + qv[j].w * kv.w;
                }
        } else {
            for (int h = lane; h < H; h += 64) d += qp[h] * kp[h];
        }
        d = wave_sum(d) * qinv * kinv[c];
        const int slot = c >> 6;
#pragma unroll
        for (int t = 0; t < TK_SLOTS; ++t)
            if (t == slot && (c & 63) == lane) sims[t] = d;
    }
}

// k rounds of a wave-wide arg-max over sims (ties: lower index), best first into out_idx / out_sim [k]; consumes sims
__device__ __forceinline__ void cosine_select(float (&sims)[TK_SLOTS], int C, int k, int lane, int32_t *out_idx, float *out_sim) {
    for (int r = 0; r < k; ++r) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < TK_SLOTS; ++t) {
            const int c = t * 64 + lane;
            if (c < C && (sims[t] > best || (sims[t] == best && c < bi))) { best = sims[t]; bi = c; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { out_idx[r] = bi; out_sim[r] = best; }
#pragma unroll
        for (int t = 0; t < TK_SLOTS; ++t)
            if (t * 64 + lane == bi) sims[t] = -INFINITY;
    }
}

}  // namespace stair
