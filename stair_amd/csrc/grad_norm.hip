// stair_grad_norm: per-tensor and global L2 norms of the flat gradient bucket, the clip coefficient of
// torch.nn.utils.clip_grad_norm_ and the "this step's gradients are not finite" bit of the optimizer's guard word -- all on
// the device, between the gradient exchange and stair_adam_step_scaled, with no host read-back (stair_amd/train.py
// Trainer(max_grad_norm=...)).  The reference loop (train_module.py:408-412) has no clipping; this goes beyond it.
//
// The result is a pure function of the inputs (store-and-sum: no float atomics, nothing depends on the order in which
// workgroups arrive or on where the grid places them), so a bit-reproducible step stays bit-reproducible and the ranks of a
// data-parallel job -- which hold the same reduced bucket -- reach the same coefficient and the same refuse / apply decision
// without a second collective.
//
//   pass A  grad_norm_partial_kernel   one wave per 256-float block: four squares per lane added in lane order, a fixed
//           butterfly over the 64 lanes, one fp32 partial per block into block_scratch.  Elements at or beyond the element
//           count of the block's segment are masked, so the padding behind a tensor never matters (it may hold NaN).
//   pass B  grad_norm_final_kernel     ONE workgroup, launched after pass A (the launch boundary makes the partials visible):
//           per segment the block partials are summed in fp64 in a fixed order, the segment sums are added in fp64 in
//           segment-index order, norm and coefficient are evaluated in fp32 as torch does.
#include "ops.h"

namespace stair {

namespace {

constexpr int kSegBlock = 256;            // floats per block: the granule parameter tensors start on (stair_adam_step)
constexpr int kFinalThreads = 1024, kFinalWaves = kFinalThreads / kWave;
constexpr int kSegChunk = 256;            // segments whose sums pass B holds in LDS at a time
constexpr int kSegGroup = 8;              // segments whose first loads a wave of pass B issues before it reduces any of them

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// valid elements of block b: 256 inside a segment, the remainder in a segment's last block, 0 for a block no segment owns.
// Segment index order need not be memory order, so the owner is searched: 64 segments per step, one per lane.
__device__ __forceinline__ int block_valid(int64_t b, const int32_t *seg_first_block, const int64_t *seg_numel, int n_seg, int lane) {
    for (int s0 = 0; s0 < n_seg; s0 += kWave) {
        const int s = s0 + lane;
        int rest = 0;
        if (s < n_seg) {
            const int64_t first = seg_first_block[s], numel = seg_numel[s];
            if (b >= first && (b - first) * kSegBlock < numel)
                rest = numel - (b - first) * kSegBlock < kSegBlock ? (int)(numel - (b - first) * kSegBlock) : kSegBlock;
        }
        const unsigned long long owners = __ballot(rest > 0);
        if (owners) return __shfl(rest, __ffsll(owners) - 1, 64);
    }
    return 0;
}

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float *g, int64_t nblocks, const int32_t *seg_first_block,
                                                                const int64_t *seg_numel, int n_seg, float *block_scratch) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6);
    if (b >= nblocks) return;
    const v4f x = *reinterpret_cast<const v4f *>(g + b * kSegBlock + lane * 4);      // in flight while the owner is searched
    const int valid = block_valid(b, seg_first_block, seg_numel, n_seg, lane);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = lane * 4 + j < valid ? x[j] : 0.f;
        acc = j == 0 ? v * v : acc + v * v;
    }
    acc = wave_sum(acc);
    if (lane == 0) block_scratch[b] = acc;
}

__global__ __launch_bounds__(kFinalThreads) void grad_norm_final_kernel(const float *block_scratch, int64_t nblocks,
                                                                        const int32_t *seg_first_block, const int64_t *seg_numel,
                                                                        int n_seg, float max_norm, float *seg_norm, float *out,
                                                                        uint32_t *guard) {
    __shared__ double s_part[kFinalWaves][kSegChunk];     // [wave][segment of the chunk]: that wave's share of the segment's blocks
    __shared__ double s_sum[kSegChunk];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
    double total = 0.0;                                    // thread 0 only
    for (int c0 = 0; c0 < n_seg; c0 += kSegChunk) {
        const int cn = n_seg - c0 < kSegChunk ? n_seg - c0 : kSegChunk;
        // thread t takes blocks t, t + 1024, ... of every segment, in that order; then the fixed butterfly over its wave
        for (int s0 = 0; s0 < cn; s0 += kSegGroup) {
            double acc[kSegGroup];
            int64_t first[kSegGroup], nb[kSegGroup];
#pragma unroll
            for (int k = 0; k < kSegGroup; ++k) {
                first[k] = nb[k] = 0;
                if (s0 + k < cn) {
                    first[k] = seg_first_block[c0 + s0 + k];
                    nb[k] = (seg_numel[c0 + s0 + k] + kSegBlock - 1) / kSegBlock;
                    if (first[k] < 0 || first[k] >= nblocks) nb[k] = 0;                 // a segment outside the buffer owns nothing
                    else if (nb[k] > nblocks - first[k]) nb[k] = nblocks - first[k];
                }
                acc[k] = tid < nb[k] ? (double)block_scratch[first[k] + tid] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < kSegGroup; ++k) {
                for (int64_t j = tid + kFinalThreads; j < nb[k]; j += kFinalThreads) acc[k] += (double)block_scratch[first[k] + j];
                const double w = wave_sum_f64(acc[k]);
                if (lane == 0 && s0 + k < cn) s_part[wave][s0 + k] = w;
            }
        }
        __syncthreads();
        if (tid < cn) {
            double sum = s_part[0][tid];
#pragma unroll
            for (int w = 1; w < kFinalWaves; ++w) sum += s_part[w][tid];
            s_sum[tid] = sum;
            seg_norm[c0 + tid] = (float)sqrt(sum);
        }
        __syncthreads();
        if (tid == 0)
            for (int s = 0; s < cn; ++s) total += s_sum[s];                              // segment-index order
        __syncthreads();
    }
    if (tid == 0) {
        // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1, on an fp32 tensor -- where
        // torch evaluates scalar / tensor as tensor.reciprocal() * scalar: two roundings, reproduced here bit for bit
        const float norm = (float)sqrt(total);
        out[0] = norm;
        out[1] = fminf(1.0f, __fmul_rn(__frcp_rn(__fadd_rn(norm, 1e-6f)), max_norm));
        if (guard && !isfinite(total)) *guard |= 2u;             // inf or NaN: bit 1, the other bits stay
    }
}

}  // namespace

int launch_grad_norm(const float *g, int64_t n, const int32_t *seg_first_block, const int64_t *seg_numel, int n_seg, float max_norm,
                     float *block_scratch, float *seg_norm, float *out, uint32_t *guard, hipStream_t s) {
    STAIR_CHECK(n % kSegBlock == 0, "the flat gradient buffer is made of whole 256-float blocks");
    const int64_t nblocks = n / kSegBlock;
    STAIR_ACCT("grad_norm_partial_kernel", n * 4 + nblocks * 4);
    STAIR_ACCT("grad_norm_final_kernel", nblocks * 4 + (int64_t)n_seg * (4 + 8 + 4) + 8);
    if (nblocks > 0) {
        const int waves = 256 / kWave;
        hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)((nblocks + waves - 1) / waves)), dim3(256), 0, s, g, nblocks,
                           seg_first_block, seg_numel, n_seg, block_scratch);
        STAIR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(kFinalThreads), 0, s, block_scratch, nblocks, seg_first_block, seg_numel,
                       n_seg, max_norm, seg_norm, out, guard);
    STAIR_LAUNCH_CHECK();
    return 0;
}

}  // namespace stair

extern "C" int stair_grad_norm(const float *grads, int64_t n, const int32_t *seg_first_block, const int64_t *seg_numel, int32_t n_seg,
                               float max_norm, float *block_scratch, float *seg_norm, float *out, uint32_t *guard,
                               stair_stream stream) {
    STAIR_CHECK(out && n >= 0 && n_seg >= 0, "bad argument");
    STAIR_CHECK(n == 0 || (grads && block_scratch), "null argument");
    STAIR_CHECK(n_seg == 0 || (seg_first_block && seg_numel && seg_norm), "null argument");
    STAIR_CHECK(n % 256 == 0, "the flat gradient buffer is made of whole 256-float blocks");
    STAIR_CHECK(n / 256 <= 0x7fffffffll * 4, "the buffer has more blocks than one launch covers");
    STAIR_CHECK(reinterpret_cast<uintptr_t>(grads) % 16 == 0, "grads must be 16-byte aligned");
    STAIR_CHECK(max_norm > 0.f, "max_norm must be positive (+inf: measure, never scale)");
    return stair::launch_grad_norm(grads, n, seg_first_block, seg_numel, n_seg, max_norm, block_scratch, seg_norm, out, guard,
                                   static_cast<hipStream_t>(stream));
}
