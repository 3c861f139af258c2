// Token pooling of the Point-M2AE classifiers' tail, shared by cls_tail.hip (the fine-tune forward) and vote.hip (the votes), so
// both feed their heads the same bits: per channel the sum over t = 0..T-1 in token order, then / T, and the first maximum over
// the tokens (a NaN wins, like torch.max).  The feature: mode 0 = mean + max (F = C), mode 1 = [mean ; max] (F = 2C).
#pragma once
#include <hip/hip_runtime.h>

namespace gm3d {

struct PoolAcc {
    float s, m;
    int am;
    // x0: the channel's value at token 0 (the loop then starts at t = 0)
    __device__ __forceinline__ void init(float x0) {
        s = 0.0f;
        m = x0;
        am = 0;
    }
    __device__ __forceinline__ void add(float v, int t) {
        s += v;
        if (v > m || (v != v && m == m)) {
            m = v;
            am = t;
        }
    }
    __device__ __forceinline__ float mean(int T) const { return s / (float)T; }
};

// f: one cloud's feature row (width F); channel c of C
__device__ __forceinline__ void pool_feature(float* f, int C, int c, int mode, float mean, float mx) {
    if (mode) {
        f[c] = mean;
        f[C + c] = mx;
    } else {
        f[c] = mean + mx;
    }
}

}  // namespace gm3d
