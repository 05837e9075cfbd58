// Device-resident inputs: the dense tensors a pass reads, gathered on the stream from a clip library and a word table that were
// uploaded once (stair_amd/clip_library.py, data.WordTable).  A step then sends row numbers, not rows.
//
// Both kernels follow gather_encoded_video_kernel (csrc/plan.hip): one 16-byte load and one 16-byte store per element, plain
// stores, every output element written exactly once (the caller clears nothing), no atomics, no LDS, no scratch.  The project's
// shape rules make every row a whole number of 16-byte units: V % 4 == 0 (fp32), V % 32 == 0 (bf16), E % 4 == 0.
#include <algorithm>

#include "common.h"

namespace stair {

// Clip v of dst [n, T, V] = the first min(lens[v], src_frames, T) frames (lens NULL: min(src_frames, T)) of the library clip at
// src + rows[v] * src_stride16, exact zeros behind them up to T.  All counts in 16-byte units: u_frame per frame, tu = T * u_frame
// per output clip.  Nothing behind a clip's frames is read from the library.  Grid (clips, chunks of the clip).
__global__ void __launch_bounds__(256) gather_clips_kernel(const uint4 *__restrict__ src, int64_t src_stride16, const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ lens, uint4 *__restrict__ dst, int tu, int u_frame,
                                                            int src_frames, int T) {
    const int v = blockIdx.x;
    const int frames = max(min(min(lens ? lens[v] : src_frames, src_frames), T), 0);
    const int live = frames * u_frame;
    const uint4 *s = src + (int64_t)rows[v] * src_stride16;
    uint4 *d = dst + (int64_t)v * tu;
    for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < tu; e += gridDim.y * blockDim.x)
        d[e] = e < live ? s[e] : uint4{0u, 0u, 0u, 0u};
}

// dst[i, :] = table[ids[i], :], rows of e4 16-byte units; a workgroup covers 1024 consecutive units of dst -- 13 rows of 300
// floats -- so a batch of short rows is a few thousand workgroups, not one per word.  An id outside the table (the Python layer
// refuses it before the upload) reads nothing and stores NaN: never a read outside the table, never a value that looks like data.
__global__ void __launch_bounds__(256) gather_words_kernel(const uint4 *__restrict__ table, int e4, int n_table_rows, const int32_t *__restrict__ ids,
                                                            uint4 *__restrict__ dst, int64_t total) {
    const int64_t first = (int64_t)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t e = first + k * 256;
        if (e >= total) return;
        const int i = (int)(e / e4), c = (int)(e - (int64_t)i * e4);
        const int id = ids[i];
        const bool ok = (unsigned)id < (unsigned)n_table_rows;
        dst[e] = ok ? table[(int64_t)id * e4 + c] : uint4{0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0x7fc00000u};
    }
}

}  // namespace stair

using namespace stair;

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int stair_gather_clips(const void *src, int32_t elem_bytes, int64_t clip_stride_elems, int32_t rows_cap, int32_t V,
                                  const int32_t *rows, const int32_t *lens, int32_t n, int32_t T, void *dst, stair_stream stream) {
    STAIR_CHECK(src && rows && dst, "null argument (src, rows and dst are required; lens may be NULL)");
    STAIR_CHECK(elem_bytes == 2 || elem_bytes == 4, "elem_bytes must be 2 (bf16) or 4 (fp32)");
    STAIR_CHECK(n >= 0 && T >= 1 && rows_cap >= 1 && V >= 1, "n must be >= 0 and T, rows_cap, V positive");
    STAIR_CHECK(((int64_t)V * elem_bytes) % 16 == 0, "a frame must be a multiple of 16 bytes (V % 4 == 0 for fp32, V % 8 == 0 for bf16)");
    STAIR_CHECK(clip_stride_elems >= (int64_t)rows_cap * V && (clip_stride_elems * elem_bytes) % 16 == 0,
                "clip_stride_elems must be at least rows_cap * V and a multiple of 16 bytes");
    STAIR_CHECK(aligned16(src) && aligned16(dst), "src and dst must be 16-byte aligned");
    STAIR_CHECK((int64_t)T * V * elem_bytes / 16 < (1ll << 31), "an output clip must stay below 2^31 16-byte units");
    if (n == 0) return 0;
    const int u_frame = (int)((int64_t)V * elem_bytes / 16), tu = T * u_frame;
    const int chunks = (int)std::min<int64_t>(((int64_t)tu + 2047) / 2048, 65535);
    STAIR_ACCT("gather_clips", 2ll * n * T * V * elem_bytes);
    hipLaunchKernelGGL(gather_clips_kernel, dim3(n, chunks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint4 *>(src),
                       clip_stride_elems * elem_bytes / 16, rows, lens, static_cast<uint4 *>(dst), tu, u_frame, rows_cap, T);
    STAIR_LAUNCH_CHECK();
    return 0;
}

extern "C" int stair_gather_words(const float *table, int32_t E, int32_t n_table_rows, const int32_t *ids, int32_t n, float *dst,
                                  stair_stream stream) {
    STAIR_CHECK(table && ids && dst, "null argument");
    STAIR_CHECK(E >= 4 && E % 4 == 0, "E must be a positive multiple of 4 (a row is a whole number of 16-byte units)");
    STAIR_CHECK(n >= 0 && n_table_rows >= 1, "n must be >= 0 and the table must hold a row");
    STAIR_CHECK(aligned16(table) && aligned16(dst), "table and dst must be 16-byte aligned");
    if (n == 0) return 0;
    const int e4 = E / 4;
    const int64_t total = (int64_t)n * e4, blocks = (total + 1023) / 1024;
    STAIR_CHECK(blocks < (1ll << 31), "too many rows for one call");
    STAIR_ACCT("gather_words", 2ll * n * E * 4);
    hipLaunchKernelGGL(gather_words_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint4 *>(table), e4, n_table_rows, ids, reinterpret_cast<uint4 *>(dst), total);
    STAIR_LAUNCH_CHECK();
    return 0;
}
