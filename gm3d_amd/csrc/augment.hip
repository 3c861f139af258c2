// Point-cloud augmentations as one launch: an ordered program of up to GM3D_AUG_MAX_OPS transforms of the reference's
// Point-MAE_SA3D/datasets/data_transforms.py (PointcloudRotate :6-18, PointcloudScaleAndTranslate :20-35, PointcloudJitter :37-49,
// PointcloudScale :51-63, PointcloudTranslate :65-76, PointcloudRandomInputDropout :79-94, RandomHorizontalFlip :96-118), applied in
// place to pc (B,N,3).  The kernel draws nothing: every random number arrives in cloud_u / point_u / point_z (include/gm3d.h).
//
// One workgroup per cloud; thread t owns points t, t + T, ... for the whole program, so pointwise ops need no synchronisation: a
// thread reads back only what it wrote itself.  Two ops need another thread's data -- the flip (the per-axis maximum over the cloud)
// and the dropout (point 0 as it stands when the op starts) -- and the program is cut into segments in front of each of them: a
// segment is one pass over the thread's points (load, the segment's ops in registers, store) that also gathers what the op behind it
// needs (each wave's maximum, or point 0) into LDS, followed by the launch's only kind of barrier.  The LDS slots alternate with the
// segment's parity: a slot is rewritten two barriers after it was read.  No atomics, no data-dependent order: the result is a pure
// function of pc and the draws.
//
// Per-cloud quantities (the rotation's cos / sin, scales, shifts, the dropout threshold, the flip's axis bits) are worked out once
// per wave: lane j computes op j's six words, and every lane fetches them with v_readlane when it applies op j.
//
// Arithmetic: every product and sum is rounded separately (the file is built with -ffp-contract=off, like the elementwise-op chain
// and gm3d_scale_translate); the rotation angle, cos and sin are double, rounded once to fp32; the thresholds (dropout, the flip's
// 0.95 and 0.5) are compared in double, as the reference compares its float64 draws.
#include <math.h>

#include "common.hpp"

namespace gm3d {

constexpr int AUG_THREADS_MAX = 1024, AUG_KIND_MASK = 0xff;

struct AugProgram {                          // handed to the kernel by value: a captured graph bakes it in
    int nops;
    int code[GM3D_AUG_MAX_OPS];              // GM3D_AUG_* [| GM3D_AUG_FINAL]
    int col[GM3D_AUG_MAX_OPS];               // first column of the op's draws in cloud_u
    float p[GM3D_AUG_MAX_OPS][3];
};

__host__ __device__ inline bool aug_exchanges(int code) {
    const int k = code & AUG_KIND_MASK;
    return k == GM3D_AUG_DROPOUT || k == GM3D_AUG_FLIP;
}

// draw m of group `col` (cnt draws per cloud) for cloud b: cloud_u is one (B,cnt) block per group, blocks in column order
__device__ __forceinline__ float aug_u(const float* __restrict__ cu, int B, int b, int col, int cnt, int m) {
    return cu[(size_t)B * col + (size_t)b * cnt + m];
}

__global__ __launch_bounds__(AUG_THREADS_MAX) void augment_kernel(float* __restrict__ pc, const float* __restrict__ cloud_u,
                                                                   const float* __restrict__ point_u,
                                                                   const float* __restrict__ point_z, int B, int N,
                                                                   AugProgram prog) {
    __shared__ float wave_max[2][AUG_THREADS_MAX / GM3D_WAVE][3];
    __shared__ float first_pt[2][3];
    const int b = blockIdx.x, t = threadIdx.x, T = blockDim.x, lane = t & (GM3D_WAVE - 1), wave = t / GM3D_WAVE;
    float* p = pc + (size_t)b * N * 3;
    const float* pu = point_u ? point_u + (size_t)b * N : nullptr;
    const float* pz = point_z ? point_z + (size_t)b * N * 3 : nullptr;

    // ---- per-cloud words of every op: lane j holds op j's
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
    for (int j = 0; j < prog.nops; ++j) {
        if (lane != j) continue;
        const int kind = prog.code[j] & AUG_KIND_MASK, col = prog.col[j];
        const bool fin = (prog.code[j] & GM3D_AUG_FINAL) != 0;
        const float q0 = prog.p[j][0], q1 = prog.p[j][1], q2 = prog.p[j][2];
        if (kind == GM3D_AUG_ROTATE) {
            const double ang = (double)aug_u(cloud_u, B, b, col, 1, 0) * 2.0 * 3.141592653589793;
            c0 = __float_as_int((float)cos(ang));
            c1 = __float_as_int((float)sin(ang));
        } else if (kind == GM3D_AUG_SCALE || kind == GM3D_AUG_SCALE_TRANSLATE) {
            const float u0 = aug_u(cloud_u, B, b, col, 3, 0), u1 = aug_u(cloud_u, B, b, col, 3, 1), u2 = aug_u(cloud_u, B, b, col, 3, 2);
            c0 = __float_as_int(fin ? u0 : u0 * q1 + q0);                  // u * span + lo, as gm3d_scale_translate
            c1 = __float_as_int(fin ? u1 : u1 * q1 + q0);
            c2 = __float_as_int(fin ? u2 : u2 * q1 + q0);
        }
        if (kind == GM3D_AUG_TRANSLATE || kind == GM3D_AUG_SCALE_TRANSLATE) {
            const int cs = kind == GM3D_AUG_TRANSLATE ? col : col + 3;     // ScaleAndTranslate: the shifts are the second group
            const float tr = kind == GM3D_AUG_TRANSLATE ? q0 : q2;
            const float u0 = aug_u(cloud_u, B, b, cs, 3, 0), u1 = aug_u(cloud_u, B, b, cs, 3, 1), u2 = aug_u(cloud_u, B, b, cs, 3, 2);
            c3 = __float_as_int(fin ? u0 : (u0 * 2.0f - 1.0f) * tr);
            c4 = __float_as_int(fin ? u1 : (u1 * 2.0f - 1.0f) * tr);
            c5 = __float_as_int(fin ? u2 : (u2 * 2.0f - 1.0f) * tr);
        } else if (kind == GM3D_AUG_DROPOUT) {
            const double u = (double)aug_u(cloud_u, B, b, col, 1, 0);
            const double thr = fin ? u : u * (double)q0;
            c0 = __double2loint(thr);
            c1 = __double2hiint(thr);
        } else if (kind == GM3D_AUG_FLIP) {
            const int up = (int)q0, lo = up == 0 ? 1 : 0, hi = up == 2 ? 1 : 2;
            int bits = 0;
            if ((double)aug_u(cloud_u, B, b, col, 3, 0) < 0.95) {
                if ((double)aug_u(cloud_u, B, b, col, 3, 1) < 0.5) bits |= 1 << lo;
                if ((double)aug_u(cloud_u, B, b, col, 3, 2) < 0.5) bits |= 1 << hi;
            }
            c0 = bits;
        }
    }

    // ---- segments: ops [k, e) run in one pass; op k may be an exchanging op (its data is in ex0..2), op e is the next one
    int k = 0, e = 0;
    while (e < prog.nops && !aug_exchanges(prog.code[e])) ++e;
    float ex0 = 0.f, ex1 = 0.f, ex2 = 0.f;                   // op k's exchanged data: the three maxima, or point 0
    for (int seg = 0;; ++seg) {
        const int next = e < prog.nops ? (prog.code[e] & AUG_KIND_MASK) : GM3D_AUG_NONE;
        float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY;
        for (int i = t; i < N; i += T) {
            float x = p[(size_t)i * 3], y = p[(size_t)i * 3 + 1], z = p[(size_t)i * 3 + 2];
            for (int j = k; j < e; ++j) {
                const int kind = prog.code[j] & AUG_KIND_MASK;
                const bool fin = (prog.code[j] & GM3D_AUG_FINAL) != 0;
                const int a0 = __builtin_amdgcn_readlane(c0, j), a1 = __builtin_amdgcn_readlane(c1, j);
                if (kind == GM3D_AUG_ROTATE) {
                    const float c = __int_as_float(a0), s = __int_as_float(a1);
                    const float nx = x * c - z * s, nz = x * s + z * c;
                    x = nx;
                    z = nz;
                } else if (kind == GM3D_AUG_JITTER) {
                    const float sd = prog.p[j][0], clip = prog.p[j][1];
                    float n0 = pz[(size_t)i * 3], n1 = pz[(size_t)i * 3 + 1], n2 = pz[(size_t)i * 3 + 2];
                    if (!fin) {
                        n0 *= sd;
                        n1 *= sd;
                        n2 *= sd;
                    }
                    x += fminf(fmaxf(n0, -clip), clip);
                    y += fminf(fmaxf(n1, -clip), clip);
                    z += fminf(fmaxf(n2, -clip), clip);
                } else if (kind == GM3D_AUG_DROPOUT) {
                    if ((double)pu[i] <= __hiloint2double(a1, a0)) {
                        x = ex0;
                        y = ex1;
                        z = ex2;
                    }
                } else if (kind == GM3D_AUG_FLIP) {
                    if (a0 & 1) x = ex0 - x;
                    if (a0 & 2) y = ex1 - y;
                    if (a0 & 4) z = ex2 - z;
                } else {
                    const int a2 = __builtin_amdgcn_readlane(c2, j);
                    if (kind != GM3D_AUG_TRANSLATE) {
                        x *= __int_as_float(a0);
                        y *= __int_as_float(a1);
                        z *= __int_as_float(a2);
                    }
                    if (kind != GM3D_AUG_SCALE) {
                        x += __int_as_float(__builtin_amdgcn_readlane(c3, j));
                        y += __int_as_float(__builtin_amdgcn_readlane(c4, j));
                        z += __int_as_float(__builtin_amdgcn_readlane(c5, j));
                    }
                }
            }
            if (k < e) {
                p[(size_t)i * 3] = x;
                p[(size_t)i * 3 + 1] = y;
                p[(size_t)i * 3 + 2] = z;
            }
            if (next == GM3D_AUG_FLIP) {
                m0 = fmaxf(m0, x);
                m1 = fmaxf(m1, y);
                m2 = fmaxf(m2, z);
            } else if (next == GM3D_AUG_DROPOUT && i == 0) {
                first_pt[seg & 1][0] = x;
                first_pt[seg & 1][1] = y;
                first_pt[seg & 1][2] = z;
            }
        }
        if (next == GM3D_AUG_NONE) break;                    // uniform: the program is the same for every thread
        if (next == GM3D_AUG_FLIP) {
#pragma unroll
            for (int o = 1; o < GM3D_WAVE; o <<= 1) {
                m0 = fmaxf(m0, __shfl_xor(m0, o));
                m1 = fmaxf(m1, __shfl_xor(m1, o));
                m2 = fmaxf(m2, __shfl_xor(m2, o));
            }
            if (lane == 0) {
                wave_max[seg & 1][wave][0] = m0;
                wave_max[seg & 1][wave][1] = m1;
                wave_max[seg & 1][wave][2] = m2;
            }
        }
        __syncthreads();
        if (next == GM3D_AUG_FLIP) {
            ex0 = wave_max[seg & 1][0][0];
            ex1 = wave_max[seg & 1][0][1];
            ex2 = wave_max[seg & 1][0][2];
            for (int w = 1; w < T / GM3D_WAVE; ++w) {
                ex0 = fmaxf(ex0, wave_max[seg & 1][w][0]);
                ex1 = fmaxf(ex1, wave_max[seg & 1][w][1]);
                ex2 = fmaxf(ex2, wave_max[seg & 1][w][2]);
            }
        } else {
            ex0 = first_pt[seg & 1][0];
            ex1 = first_pt[seg & 1][1];
            ex2 = first_pt[seg & 1][2];
        }
        k = e++;
        while (e < prog.nops && !aug_exchanges(prog.code[e])) ++e;
    }
}

// draws per cloud of one op in cloud_u; -1 for an unknown op code
inline int aug_draws(int code) {
    switch (code & AUG_KIND_MASK) {
        case GM3D_AUG_ROTATE: case GM3D_AUG_DROPOUT: return 1;
        case GM3D_AUG_SCALE: case GM3D_AUG_TRANSLATE: case GM3D_AUG_FLIP: return 3;
        case GM3D_AUG_SCALE_TRANSLATE: return 6;
        case GM3D_AUG_JITTER: return 0;
    }
    return -1;
}

}  // namespace gm3d

extern "C" int gm3d_augment(float* pc, int B, int N, int nops, const int* ops, const float* params, const float* cloud_u,
                            const float* point_u, const float* point_z, gm3d_stream_t stream) {
    using namespace gm3d;
    if (!pc || N < 1 || B < 0 || nops < 1 || nops > GM3D_AUG_MAX_OPS || !ops || !params) return GM3D_EINVAL;
    AugProgram prog = {};
    prog.nops = nops;
    int D = 0, dropouts = 0, jitters = 0;
    for (int j = 0; j < nops; ++j) {
        const int kind = ops[j] & AUG_KIND_MASK, cnt = aug_draws(ops[j]);
        if (cnt < 0 || (ops[j] & ~(AUG_KIND_MASK | GM3D_AUG_FINAL))) return GM3D_EINVAL;
        if (kind == GM3D_AUG_FLIP && !(params[j * 3] == 0.f || params[j * 3] == 1.f || params[j * 3] == 2.f)) return GM3D_EINVAL;
        dropouts += kind == GM3D_AUG_DROPOUT;
        jitters += kind == GM3D_AUG_JITTER;
        prog.code[j] = ops[j];
        prog.col[j] = D;
        for (int q = 0; q < 3; ++q) prog.p[j][q] = params[j * 3 + q];
        D += cnt;
    }
    if (dropouts > 1 || jitters > 1) return GM3D_EINVAL;     // one point_u and one point_z per launch
    if ((D > 0 && !cloud_u) || (dropouts && !point_u) || (jitters && !point_z)) return GM3D_EINVAL;
    if (B == 0) return GM3D_OK;
    const int threads = N >= AUG_THREADS_MAX ? AUG_THREADS_MAX : (N + GM3D_WAVE - 1) / GM3D_WAVE * GM3D_WAVE;
    return launch_lds<augment_kernel>(dim3((unsigned)B), dim3(threads), 0, stream, pc, cloud_u, point_u, point_z, B, N, prog);
}
