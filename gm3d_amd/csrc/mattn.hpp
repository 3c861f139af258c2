// What the two masked-attention files share (attention_masked.hip: T <= 512, a head's images whole in LDS; attention_long.hip:
// 513 <= T <= 2048, the images streamed in row chunks): the padded LDS image of a (rows, HD) bf16 matrix, the workgroup order that
// keeps a cloud on one XCD, and the mask word with the keys beyond T forced on.
#pragma once
#include "mfma.hpp"

namespace gm3d {

// LDS image of a (rows, HD) bf16 matrix: row pitch HD*2 + 16 bytes (48 / 80 / 144: 16-byte row reads of 16 consecutive rows hit
// 16 different bank quads; transposed reads are at worst 2-way)
template <int HD> struct MImg {
    static constexpr int PITCH = HD * 2 + 16;
    static __device__ __forceinline__ bf16x8 row(const unsigned char* img, int r, int ch) {     // 8 consecutive d starting at 8*ch
        return *reinterpret_cast<const bf16x8*>(img + r * PITCH + ch * 16);
    }
    // fragment A[i = column][k] in accumulator-as-operand k order: rows k0 + 16 s + 4 hh + {0..3, 8..11}, column colblk + (lane&15)
    static __device__ __forceinline__ bf16x8 tr8(const unsigned char* img, int k0, int s, int hh, int colblk, int lane) {
        const int l16 = lane & 15, q = l16 >> 2, p = l16 & 3;
        int col = colblk + 4 * p;
        if (col >= HD) col -= HD * (col / HD);            // lanes past the head dim read valid (ignored) data: pad, don't mask
        const int r0 = k0 + 16 * s + 4 * hh + q;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + r0 * PITCH + col * 2));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + (r0 + 8) * PITCH + col * 2));
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = lo[j]; v[4 + j] = hi[j]; }
        return v;
    }
    // cooperative copy of one head's (T, HD) slice into a zero-padded `rows`-row image
    static __device__ __forceinline__ void stage(unsigned char* img, const bf16_t* src, size_t row_stride, int T, int rows, int tid,
                                                 int nthreads) {
        constexpr int CH = HD / 8;
        for (int c = tid; c < rows * CH; c += nthreads) {
            const int r = c / CH, ch = c - r * CH;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r < T) v = *reinterpret_cast<const uint4*>(src + (size_t)r * row_stride + ch * 8);
            *reinterpret_cast<uint4*>(img + r * PITCH + ch * 16) = v;
        }
    }
};

// Workgroup -> (cloud * head, tile block) with the workgroups of ONE cloud on ONE XCD.  The hardware deals consecutive workgroup ids to
// the 8 XCDs round-robin, and the qkv layout (B,T,3,H,hd) interleaves the heads of a cloud within every 2 H hd-byte row (32-byte
// pieces at hd = 16): with id = cloud * H + head the six heads of a cloud pull the same lines into six different L2s (PMC, T = 512,
// hd = 16: 527 MB fetched for 63 MB of operands in the backward).  Remapped, id' = (id % 8) * (total / 8) + id / 8 runs through the
// (tile block, head, cloud) triples in order on each XCD.
__device__ __forceinline__ void mattn_block(int& bh, int& yb) {
    const int nx = gridDim.x, ny = gridDim.y, total = nx * ny;
    int lin = blockIdx.x + nx * blockIdx.y;
    if ((total & 7) == 0) lin = (lin & 7) * (total >> 3) + (lin >> 3);
    yb = lin % ny;
    bh = lin / ny;
}

// word `kt` of mask row `i` with the keys >= T of that word forced on; rows >= T: everything masked
__device__ __forceinline__ unsigned mask_word(const unsigned* mrow /* row i, or nullptr */, bool row_ok, int kt, int T) {
    unsigned w = mrow ? mrow[kt] : 0u;
    const int rem = T - 32 * kt;                    // valid keys in this word
    if (rem < 32) w |= rem <= 0 ? 0xffffffffu : (0xffffffffu << rem);
    return row_ok ? w : 0xffffffffu;
}

}  // namespace gm3d
