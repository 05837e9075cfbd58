// Encoder input gradients and the caller-seeded reverse pass (stair_plan_backward_dlogits, include/stair_hip.h).
//
// After BPTT the gates buffer of each encoder holds the gate pre-activation gradients dG [rows, 8 Hh] in place (forward direction in
// columns 0 .. 4 Hh - 1, reverse direction behind it, gate order i, f, g, o: the layout launch_lstm_bwd_weights reads for dW_ih).  The
// layer's input is x W_ih^T per direction, so its input gradient is ONE NN product over both directions:
//     dX [rows, I] = [dG_fwd | dG_bwd] . [W_ih_fwd ; W_ih_bwd],   K = 8 Hh.
// The stacked W_ih is transposed once into an [I, 8 Hh] image and the product runs as the library's NT GEMM (launch_gemm: C = A W^T with
// A = dG read in place), which follows the context's matmul mode -- exact fp32 MFMA (f32), hi / lo split on the fly (bf16x3), one bf16
// product (bf16).  The plane GEMM of the forward projection (csrc/gemm_planes.hip) would need dG split into hi / lo planes first: 4 bytes
// per element of extra storage and a full extra pass over dG (1 GB at the bench shape), which the register-staged split kernel avoids.
// Gate-gradient rows past a sequence's length are zero after BPTT, so the same rows of dX come out as exact zeros.
#include <algorithm>

#include "common.h"

namespace stair {

// dst[i] = src[i] (the caller's d_logits into the plan's region; a kernel, so the pass stays capturable)
__global__ void seed_copy_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n4, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
        reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src)[i];
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

int launch_seed_dlogits(const float *src, float *dst, int64_t n, hipStream_t s) {
    STAIR_CHECK(src && dst && n >= 0, "bad argument");
    STAIR_CHECK(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0, "pointers must be 16-byte aligned");
    if (n == 0) return 0;
    const int64_t n4 = n / 4;
    const int blocks = (int)std::min<int64_t>((std::max<int64_t>(n4, 1) + 255) / 256, 1024);
    hipLaunchKernelGGL(seed_copy_kernel, dim3(blocks), dim3(256), 0, s, src, dst, n4, n);
    STAIR_LAUNCH_CHECK();
    return 0;
}

// out [I][8 Hh] = transpose of the stacked [W_ih_fwd ; W_ih_bwd] [8 Hh][I], through a 32 x 33 LDS tile: reads along i and writes along k
// are both coalesced.  Grid (ceil(I / 32), 8 Hh / 32), 256 threads.
__global__ __launch_bounds__(256) void wih_stack_transpose_kernel(const float *__restrict__ w_fwd, const float *__restrict__ w_bwd,
                                                                  float *__restrict__ out, int I, int Hh) {
    __shared__ float tile[32][33];
    const int K = 8 * Hh, half = 4 * Hh;
    const int i0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, i = i0 + tx;
        float v = 0.0f;
        if (k < K && i < I) v = k < half ? w_fwd[(int64_t)k * I + i] : w_bwd[(int64_t)(k - half) * I + i];
        tile[r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, k = k0 + tx;
        if (i < I && k < K) out[(int64_t)i * K + k] = tile[tx][r];
    }
}

int launch_enc_input_grad(const float *gates, int64_t rows, int Hh, const float *w_ih_fwd, const float *w_ih_bwd, int I, float *wt_ws,
                          float *dx, hipStream_t s) {
    STAIR_CHECK(gates && w_ih_fwd && w_ih_bwd && wt_ws && dx, "null argument");
    STAIR_CHECK(rows >= 0 && rows < (1ll << 31) && Hh > 0 && Hh % 4 == 0 && I > 0 && I % 4 == 0, "bad shape");
    if (rows == 0) return 0;
    const int K = 8 * Hh;
    hipLaunchKernelGGL(wih_stack_transpose_kernel, dim3((I + 31) / 32, (K + 31) / 32), dim3(256), 0, s, w_ih_fwd, w_ih_bwd, wt_ws, I, Hh);
    STAIR_LAUNCH_CHECK();
    STAIR_ACCT_MFMA("enc_input_grad", (rows * K + (int64_t)I * K + rows * I) * 4, 2 * rows * I * (int64_t)K);
    stair_gemm_args g = {};
    g.A = gates; g.lda = K; g.a_gstride = K;
    g.W = wt_ws; g.ldw = K;
    g.C = dx; g.ldc = I; g.c_gstride = I;
    g.groups = (int32_t)rows; g.rows_per_group = 1; g.N = I; g.K = K; g.act = 0;
    return launch_gemm(g, s);
}

}  // namespace stair
