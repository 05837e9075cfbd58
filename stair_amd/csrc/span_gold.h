// The soft interval mask of span_to_attention (train_module.py:67-81), one frame at a time: the ONE device form of it, shared by the
// attention criterion (csrc/losses.hip) and the audit decoder (csrc/audit.hip), so that an IoU is scored against the mask the loss
// was trained on.
#pragma once
#include <hip/hip_runtime.h>

namespace stair {

// value of frame t of the mask drawn for L frames from the gold interval (g0, g1); double arithmetic like the reference
__device__ __forceinline__ float span_gold(double g0, double g1, int L, int t) {
    const double start = fmin((double)L - 0.002, fmax(0.001, g0));
    const double end = fmin((double)L - 0.001, g1);
    const int si = (int)ceil(start), ei = (int)floor(end);
    double v = 0.0;
    if (si < ei && t >= si && t < ei) v += 1.0;
    if (si <= ei) {
        if (t == si - 1) v += (double)si - start;
        if (t == ei) v += end - (double)ei;
    } else if (t == (ei < 0 ? ei + L : ei)) {      // gold_tensor[end_int]: a negative end counts from the clip's end as in Python
        v += end - start;                             // (only here can ei be < 0: si >= 1; the host refuses ei < -L)
    }
    return (float)v;
}

}  // namespace stair
