// avd_mfma_device.h -- device helpers shared by the matrix-core kernels (avd_vit.hip, avd_cnn.hip): bf16 conversion, the
// blocked + swizzled operand layout, the LDS fragment read that goes with it, the LDS-DMA staging of an operand half tile,
// the counted vmcnt wait and the weight-row permutation of the transposed product.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace avd_mfma {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BKH = 32;                                     // a staging unit ("half stage") is 32 deep in K
constexpr int kStages = 4;                                  // ring: kStages - 1 half stages in flight beside the one being read
                                                            // (5 = all 160 KiB of LDS measured no faster than 4)

__device__ __forceinline__ uint16_t f32_to_bf16(float v)
{
    const unsigned u = __float_as_uint(v);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);       // round to nearest even (inputs are finite)
}
__device__ __forceinline__ float bf16_to_f32(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
// two floats -> two bf16 in one dword (lo in bits 0-15): gfx950's v_cvt_pk_bf16_f32, round to nearest even -- the same bits as
// f32_to_bf16 for finite inputs, one instruction instead of eight
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi)
{
    const bf16x2_t r = __builtin_convertvector(f32x2_t{lo, hi}, bf16x2_t);
    return __builtin_bit_cast(unsigned, r);
}

// Bank swizzle of a half tile (64-byte rows, four 16-byte chunks per row, four rows per 256-byte bank row): chunk c of
// row r sits in slot c ^ swz((r >> 2) & 3).  A ds_read_b128 is served in groups of 16 lanes that are NOT contiguous
// ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...): with lane = (chunk << 4) | row a group reads rows {0-3, 12-15} of
// one chunk and rows {4-11} of the next, and swz = {0, 2, 3, 1} is what makes those sixteen accesses hit sixteen
// different 16-byte bank groups (the plain XOR with (r >> 2) & 3 is two-way conflicted for these groups).
__host__ __device__ __forceinline__ int swz(int k) { return (0x78 >> (2 * k)) & 3; }      // {0, 2, 3, 1}

// OPERAND LAYOUT IN HBM ("blocked"): a K-contiguous matrix [rows][K] is stored as 1-KiB blocks of 16 rows x 32 k, block
// (row / 16, k / 32) at ((row / 16) * (K / 32) + k / 32) * 1 KiB, and INSIDE a block exactly the bytes of the LDS image
// the MFMA fragments are read from: row r at r * 64, its four 16-byte chunks swizzled as above.  One
// global_load_lds_dwordx4 wave-instruction then copies ONE contiguous KiB (eight whole cache lines) straight into LDS.
// Element index of (row, k):
__host__ __device__ __forceinline__ int64_t blocked_index(int row, int k, int K)
{
    const int r = row & 15, kk = k & 31;
    return ((int64_t)(row >> 4) * (K >> 5) + (k >> 5)) * 512 + r * 32 + (((kk >> 3) ^ swz((r >> 2) & 3)) << 3) + (kk & 7);
}

// MFMA fragment (16 rows x 8 k of one 16-byte chunk) of an LDS half tile in that layout
__device__ __forceinline__ bf16x8 frag(const char* lds_tile, int row, int chunk)
{
    return *reinterpret_cast<const bf16x8*>(lds_tile + row * 64 + ((chunk ^ swz((row >> 2) & 3)) << 4));
}

// STAGING an operand half tile (rows x 32 k) by LDS-DMA, R rows per wave: instruction q covers rows
// wave * R + q * 16 + lane / 4; when R is an odd multiple of 8 the last instruction is issued for the lower 32 lanes only
// (8 rows).  `tile` points at the tile's first block of the half stage.
template <int R>
__device__ __forceinline__ void stage_rows(const char* tile, const unsigned (&voff)[(R + 15) / 16], char* lds_half, int wave, int lane)
{
    constexpr int Q = (R + 15) / 16;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        char* dst = lds_half + (wave * R + q * 16) * 64;
        if (q * 16 + 16 <= R) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(tile + voff[q]),
                                             (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        } else if (lane < 32) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(tile + voff[q]),
                                             (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        }
    }
}

// per-lane byte offset, relative to the tile's first block of a half stage, of the 16 bytes a lane copies with
// instruction q: tile row r = wave * R + q * 16 + lane / 4 lives in block r / 16 (blocks of one half stage are `kblocks`
// = K / 32 KiB apart; a run-time value in the convolutions), at r % 16 * 64 + (lane % 4) * 16 inside it -- the swizzle is
// already in the data
template <int R>
__device__ __forceinline__ void stage_offsets(unsigned (&voff)[(R + 15) / 16], int kblocks, int wave, int lane)
{
#pragma unroll
    for (int q = 0; q < (R + 15) / 16; q++) {
        const int r = wave * R + q * 16 + (lane >> 2);
        voff[q] = (unsigned)((r >> 4) * kblocks * 1024 + (r & 15) * 64 + (lane & 3) * 16);
    }
}

// counted wait on the wave's in-order vector-memory queue (LDS-DMAs, loads and stores alike)
#define AVD_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")

// The product is formed transposed (mfma(b, a): rows of a 16x16 result = n, lane column = m), and which weight row feeds
// which MFMA row is free to choose: MFMA row rho of column tile j takes column (j / 2) * 32 +
// (rho / 4) * 8 + (j % 2) * 4 + rho % 4 of wave column wn's `wcols` columns, so that a lane (accumulator rows (lane / 16) * 4 + r of tiles 2 jp and 2 jp + 1)
// owns EIGHT consecutive columns: one 16-byte store of bf16 per lane, 64 contiguous bytes per output row and instruction
// (the natural order gives 8-byte stores, 32 contiguous bytes).  The fragment reads stay conflict-free: the four row
// groups of a read have swizzle keys (0, 2, 0, 2) + j % 2, and the lane groups a ds_read_b128 is served in ({0-3, 12-15}
// of one chunk, {4-11} of the next) still land in four distinct slots.
__device__ __forceinline__ int b_row_of(int wn, int wcols, int j, int rho) { return wn * wcols + (j >> 1) * 32 + (rho >> 2) * 8 + (j & 1) * 4 + (rho & 3); }

}  // namespace avd_mfma
