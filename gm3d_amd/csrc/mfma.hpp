// Device helpers shared by the MFMA kernels (gemm*.hip, attention*.hip): bf16 operand vectors, the 32x32x16 bf16 MFMA and its
// accumulator layout, the swizzled 128-byte LDS row, the LDS-DMA load that fills it, and the XCD-aware workgroup order.
#pragma once
#include "common.hpp"

namespace gm3d {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// exact-fp32 32x32x2 MFMA: lane (c = lane & 31, h = lane >> 5) supplies A[c][h] and B[h][c]; same C/D layout
__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// C/D layout of a 32x32 MFMA: column = lane & 31, row = crow(reg, lane >> 5).
__device__ __forceinline__ int crow(int g, int hh) { return (g & 3) + 8 * (g >> 2) + 4 * hh; }

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (bf16_t)0.0f;
    return z;
}
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int g = 0; g < 16; ++g) z[g] = 0.f;
    return z;
}
// accumulator registers 8s..8s+7, times `mul`, as a bf16 operand
__device__ __forceinline__ bf16x8 cvt8(const f32x16& x, int s, float mul) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16_t)(x[8 * s + j] * mul);
    return v;
}

// Swizzled LDS row of 128 bytes (64 bf16) with NO padding: the 16-byte chunk ch (0..7) of row `row` sits at byte
// 128*row + 16*(ch ^ swz(row)), swz = the bit-reversed (row >> 1) & 7.  One image serves both kinds of MFMA operand read
// conflict-free (bank rule of ds_read_b128 / ds_read_b64_tr_b16: 64 banks, MI355X_MICROARCH.md LDS):
//   row read   (ds_read_b128):        a 16-lane group reads one chunk of 16 different rows -> swz spreads them over all 16 slots;
//   transposed (ds_read_b64_tr_b16):  a 32-lane half reads 4 consecutive rows x 32 columns -> (row & 1, swz bit 2) picks a
//                                     different 64-byte quarter of the bank row for each of the four rows.
// The LDS-DMA writer (global chunk pslot ^ swz(row) -> slot pslot) and every fragment reader use these two functions.
__device__ __forceinline__ int swz(int row) { return (((row >> 1) & 1) << 2) | (((row >> 2) & 1) << 1) | ((row >> 3) & 1); }
__device__ __forceinline__ int swz_off(int row, int ch) { return row * 128 + ((ch ^ swz(row)) << 4); }

// LDS byte address of a __shared__ pointer (the m0 operand of glds16)
__device__ __forceinline__ unsigned lds_addr(const unsigned char* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char*)p;
}

// One LDS-DMA piece: 64 lanes x 16 bytes from `gsrc` -> 1 KiB at the wave-uniform LDS byte address `dst` (through m0, saved and
// restored).  The compiler does not see this load (no automatic s_waitcnt vmcnt(0) before the next LDS read): callers count its
// completion by hand.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(dst)
                 : "memory");
}

// XCD-aware tile order: the hardware deals workgroups round-robin over the 8 XCDs (each with its own L2), so workgroup `block` of
// `grid` (a multiple of 8) takes logical tile (block % 8) * (grid / 8) + block / 8 -- every XCD walks a contiguous run of tiles,
// and neighbouring tiles that share operand rows hit the same L2.  `I`: unsigned for blockIdx / gridDim, int for a computed index.
template <class I> __device__ __forceinline__ int xcd_tile(I block, I grid) {
    const int per_xcd = grid >> 3;
    return (block & 7) * per_xcd + (block >> 3);
}

}  // namespace gm3d
