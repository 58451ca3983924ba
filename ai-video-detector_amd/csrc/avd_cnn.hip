// avd_cnn.hip -- ResNet-50-style CNN forward on the matrix cores (gfx950): SURVEY.md section 8 row A9.
//
// BUILD-DEFINED EXTENSION: the reference has no learned model (its per-frame "model" is the
// closed form of app/analyzers/video.py:54-56).  BASELINE.json's north_star names a "CNN (ResNet-50-style) forward" on
// MFMA; this file is that stage with caller-supplied (seeded random) weights, gated off from ai_score: nothing in the
// parity path calls it.  Its oracle is a float32 restatement with the same bf16 roundings (tests/test_cnn.py).
//
// Topology: 7x7/2 stem (64) + ReLU, 3x3/2 max pool, bottleneck stages [3, 4, 6, 3] of widths 64/128/256/512 (x4 out,
// stride on the 3x3), global average pool, 2048 -> 1000 linear: 53 convolutions, 4.1 GMAC per 224 x 224 frame.  Batch
// norm is taken as folded into the weights and a per-channel bias.
//
// DATA LAYOUT IN HBM: an activation is the matrix [pixels = n * H * W][channels], bf16, in the blocked + swizzled operand
// layout of avd_mfma_device.h (1-KiB blocks of 16 pixels x 32 channels), preceded by one KiB of zeros.  Every
// convolution is ONE implicit GEMM  out[pixel][cout] = sum_{tap, c} in[pixel shifted by tap][c] * W[cout][tap][c] :
//  * the weight operand [cout][K = taps * cin] is re-tiled once on upload: an LDS-DMA instruction copies one KiB block;
//  * the activation operand is GATHERED by the LDS-DMA itself: lane -> (tile row, 16-byte chunk), so a lane's source
//    address is "the 8 channels I need of the input pixel this output pixel sees through tap (dy, dx)"; taps that fall
//    outside the image read the zero page.  No im2col matrix is ever written -- the 7x7 stem gathers pixel pairs from a
//    zero-bordered copy of the input image instead (MODE 1 below);
//  * the epilogue adds bias (+ the residual, read in the same layout), applies ReLU, rounds to bf16 and stores 16 bytes
//    per lane straight into the blocked layout of the NEXT layer's operand.
// Tile: 256 pixels x (64 | 128 | 256) output channels per 512-thread workgroup, K in half stages of 32, ring of four half
// stages with counted vmcnt + raw s_barrier (the scheme of avd_vit.hip; K is a run-time value here).
#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>
#include "avd_internal.h"
#include "avd_mfma_device.h"

namespace {

using namespace avd_mfma;

constexpr int kSide = 224;
constexpr int kZeroPage = 512;                  // elements (1 KiB) of zeros in front of every activation
constexpr int kImgSide = 232;                   // the stem reads a 224 x 224 image with a zero border: pixel (y, x) at (y + 3, x + 3)

struct ConvGeom {
    int hin, win, cin, hout, wout, cout, ksize, stride, pad;
    int m_out;                                  // n * hout * wout
    int nh;                                     // half stages: ksize * ksize * cin / 32
    int cpb;                                    // cin / 32
};

// stem == true: (hin, win, cin, ksize, stride) describe the 7x7/2 convolution over the bordered input image
ConvGeom conv_geom(int n, int hin, int win, int cin, int cout, int ksize, int stride, bool stem = false)
{
    ConvGeom g;
    g.hin = hin; g.win = win; g.cin = cin; g.cout = cout; g.ksize = ksize; g.stride = stride; g.pad = ksize / 2;
    g.hout = (hin + 2 * g.pad - ksize) / stride + 1;
    g.wout = (win + 2 * g.pad - ksize) / stride + 1;
    g.m_out = n * g.hout * g.wout;
    g.cpb = stem ? 1 : cin / 32;
    g.nh = stem ? 7 : ksize * ksize * g.cpb;
    return g;
}

__host__ __device__ constexpr int tiles_of(int m, int bm) { return (m + bm - 1) / bm; }

// ---- one LDS plan per kernel shape: the kernel and its launcher both read it ---------------------------------------
// A workgroup of eight waves, WAVES_M x WAVES_N, each wave TI x 4 MFMA tiles: BM pixels x BN output channels.  The ring
// holds four half stages [A | B]; a layer with fewer than four half stages takes that many slots (more workgroups per CU).
template <int BM_, int WAVES_M_, int TI_>
struct ConvShape {
    static constexpr int BM = BM_, WAVES_M = WAVES_M_, WAVES_N = 8 / WAVES_M, TI = TI_, TJ = 4, BN = WAVES_N * 64;
    static_assert(WAVES_M * TI * 16 == BM && (BM == 256 || BM == 128), "a workgroup covers 256 or 128 output pixels");
    static constexpr int RA = BM / 8, QA = RA / 16;         // activation rows / LDS-DMA instructions per wave and half stage
    static constexpr int RB = BN / 8, QB = (RB + 15) / 16;  // weight rows a wave stages per half stage: 32, 16 or 8
    static constexpr int P = QA + QB;                       // LDS-DMA instructions per wave and half stage
    static constexpr int HALF_A = BM * 64, HALF_B = BN * 64, STAGE = HALF_A + HALF_B, RING = 4 * STAGE;
    static constexpr size_t lds(int nh) { return (size_t)(nh < 4 ? nh : 4) * STAGE; }
};

// the expanding 1x1 behind a 3x3 whose BM x BN output tile stays on the CU (K = mid = BN), NCH chunks of BN output channels
template <int BM, int BN, int TI, int TJ>
struct ExpandSizes {
    static constexpr int NCH = 4;
    static constexpr int KS2 = BN / 32;                     // k steps of the expanding layer
    static constexpr int A2 = BM * BN * 2, B2 = BN * BN * 2;   // bytes: the mid tile; one chunk of W3
    static constexpr int NBLK = (BN / 16) * KS2;            // KiB blocks of one W3 chunk
    static constexpr int NRES = TI * TJ / 2;                // residual loads (= output stores) per wave and chunk
    static constexpr int BIAS3_BYTES = NCH * BN * 4;
    static_assert(NBLK % 8 == 0 && NCH % 2 == 0 && NCH * BN <= 512, "a W3 block per wave, chunk pairs, one bias3 element per thread");
};

// k_conv3_expand: the expand's buffers live in the 3x3's ring.  W3 is RESIDENT when all of it fits beside the mid tile
// (mid = 64: 32 KiB in one go, no barrier in the chunk loop); otherwise its chunks alternate between two buffers, the
// second of which takes over the mid tile's LDS once the fragments are in registers.  W3 (its first chunk) is requested
// during the 3x3's LAST step, into ring slots that step no longer reads: it reads slot (nh - 1) & 3 only, hence PHASE.
//   resident (nh & 3 == 2, slot 1 live):  mid tile [0, A2) | W3 [2 STAGE, + NCH B2) | bias3 behind it
//   otherwise (nh & 3 == 0, slot 3 live): W3 chunk c at (c & 1) B2 | mid tile [B2, B2 + A2) | bias3 behind the ring
template <int BM_, int WAVES_M_, int TI_>
struct FusedShape : ConvShape<BM_, WAVES_M_, TI_>, ExpandSizes<BM_, ConvShape<BM_, WAVES_M_, TI_>::BN, TI_, 4> {
    using C = ConvShape<BM_, WAVES_M_, TI_>;
    using E = ExpandSizes<BM_, C::BN, TI_, 4>;
    static constexpr bool RESIDENT = E::NCH * E::B2 + E::BIAS3_BYTES <= 2 * C::STAGE && E::A2 <= 2 * C::STAGE;
    static constexpr int W3BASE = RESIDENT ? 2 * C::STAGE : 0, A2BASE = RESIDENT ? 0 : E::B2;
    static constexpr int BIAS3 = RESIDENT ? W3BASE + E::NCH * E::B2 : C::RING;
    static constexpr int LDS = RESIDENT ? C::RING : C::RING + E::BIAS3_BYTES;
    static constexpr int PHASE = RESIDENT ? 2 : 0;          // required nh & 3
    static_assert(RESIDENT ? BIAS3 + E::BIAS3_BYTES <= C::RING : (E::B2 + E::A2 <= C::RING && 2 * E::B2 <= C::RING && E::B2 <= 2 * C::STAGE), "LDS plan");
};

// k_slab3_expand: [slab | ring of four W2 steps]; the expand takes all of it over once the slab is dead:
//   W3 | mid tile | bias3 (mid 64, resident), else W3 chunk c at (c & 1) B2 | bias3 | ... mid tile at B2 until its fragments are read
template <int MID>
struct SlabShape : ConvShape<MID == 64 ? 256 : 128, MID == 64 ? 8 : 4, 2>, ExpandSizes<MID == 64 ? 256 : 128, MID, 2, 4> {
    static_assert(MID == 64 || MID == 128, "the two early stages");
    using C = ConvShape<MID == 64 ? 256 : 128, MID == 64 ? 8 : 4, 2>;
    using E = ExpandSizes<C::BM, MID, 2, 4>;
    static_assert(C::BN == MID, "one column tile");
    static constexpr int CPB = MID / 32;                    // channel blocks of the input
    static constexpr int HALO = MID == 64 ? 64 : 32;        // pixels in front of m0 (>= W + 1, whole pixel blocks)
    static constexpr int NSLAB = C::BM + 2 * HALO, SLAB = NSLAB * CPB * 64;       // 384 x 128 B = 192 x 256 B = 48 KiB
    static constexpr int KPS = MID == 64 ? 2 : 1;           // k blocks of W2 per step (a whole tap at 64 channels, a quarter tap at 128)
    static constexpr int STEPB = MID * 64 * KPS, NSTEP = 9 * CPB / KPS;          // 8 KiB per step
    static constexpr int LDS = SLAB + 4 * STEPB;            // ring of four: 80 KiB
    static constexpr bool RESIDENT = E::NCH * E::B2 + E::A2 + E::BIAS3_BYTES <= LDS;
    static constexpr int W3BASE = 0, A2BASE = RESIDENT ? E::NCH * E::B2 : E::B2, BIAS3 = RESIDENT ? A2BASE + E::A2 : 2 * E::B2;
    static_assert(SLAB == 49152 && STEPB == 8192 && BIAS3 + E::BIAS3_BYTES <= LDS && A2BASE + E::A2 <= LDS, "LDS plan");
};

// ---- device parts shared by the three MFMA kernels -----------------------------------------------------------------
// the column tiles of one pixel block run together on one XCD (the gathered activation rows are fetched once)
__device__ __forceinline__ int xcd_tile()
{
    const int per = (gridDim.x + 7) >> 3;
    return (blockIdx.x & 7) * per + (blockIdx.x >> 3);
}

template <int TI, int TJ>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[TI][TJ])
{
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < TJ; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// this lane's 16 bytes inside a KiB block of an output piece (16 pixels x 32 channels): pixel lane % 16, channels (lane / 16) * 8 ..
__device__ __forceinline__ unsigned lane_in_block(int lane) { return (unsigned)((lane & 15) * 64 + (((lane >> 4) ^ swz((lane >> 2) & 3)) << 4)); }

// ---- epilogue arithmetic: a lane's eight consecutive output channels of one pixel (accumulator tiles 2 jp, 2 jp + 1)
struct Bias8 { f32x4 lo, hi; };
__device__ __forceinline__ Bias8 bias8(const float* pb) { return {*reinterpret_cast<const f32x4*>(pb), *reinterpret_cast<const f32x4*>(pb + 4)}; }

// bias (+ the residual: eight bf16, where there is one), ReLU, round to bf16
__device__ __forceinline__ uint4 finish8(f32x4 lo, f32x4 hi, const Bias8& b, const uint4* residual, bool relu)
{
    lo += b.lo; hi += b.hi;
    if (residual) {
        const uint4 rv = *residual;
        lo[0] += bf16_to_f32(rv.x & 0xFFFF); lo[1] += bf16_to_f32(rv.x >> 16);
        lo[2] += bf16_to_f32(rv.y & 0xFFFF); lo[3] += bf16_to_f32(rv.y >> 16);
        hi[0] += bf16_to_f32(rv.z & 0xFFFF); hi[1] += bf16_to_f32(rv.z >> 16);
        hi[2] += bf16_to_f32(rv.w & 0xFFFF); hi[3] += bf16_to_f32(rv.w >> 16);
    }
    if (relu) {
#pragma unroll
        for (int e = 0; e < 4; e++) { lo[e] = fmaxf(lo[e], 0.f); hi[e] = fmaxf(hi[e], 0.f); }
    }
    uint4 pk;
    pk.x = pack_bf16x2(lo[0], lo[1]);
    pk.y = pack_bf16x2(lo[2], lo[3]);
    pk.z = pack_bf16x2(hi[0], hi[1]);
    pk.w = pack_bf16x2(hi[2], hi[3]);
    return pk;
}

// ---- the activation operand of a gathering kernel: the BM / 8 tile rows this wave copies per half stage (instruction q:
// tile row wave * RA + q * 16 + lane / 4).
// MODE 0: a blocked activation, gathered per tap.  Kept per row: the pixel index of tap (0, 0) (rin0), a 9-bit mask of the
// taps that fall inside the image, and the chunk that belongs in this lane's LDS slot; a tap then costs one scalar offset and
// a dozen vector operations.  Half stages come in K order: tap (dy, dx), then channel block.
// MODE 1 (the stem): the operand is the zero-bordered 224 x 224 input image [frame][232][232][4 channels, the fourth zero];
// half stage ky holds the 8 x 4 = 32 (kx, c) values of kernel row ky (kx = 7 and c = 3 carry zero weights), i.e. chunk j of a
// row = the two pixels (2 ox + 2 j, 2 ox + 2 j + 1) of image row 2 oy + ky in border coordinates: 16 contiguous, 16-byte
// aligned bytes.
template <int BM, int MODE, int KS>
struct TapGather {
    static constexpr int RA = BM / 8, QA = RA / 16;
    int rin0[QA], cw[QA];                                   // filled by the kernel (k_conv_bf16 says why)
    unsigned tapmask[QA];
    int cb = 0, dy = 0, dx = 0;                             // channel block and tap of the next half stage to be issued

    // half stage hs (they are issued in order) into the A half of ring slot `st`
    __device__ __forceinline__ void issue(const ConvGeom& g, const char* xb, char* st, int hs, int wave, int lane)
    {
#pragma unroll
        for (int q = 0; q < QA; q++) {
            unsigned off;
            if (MODE == 1) {
                off = (unsigned)(rin0[q] + hs * (kImgSide * 8));  // kernel row ky = hs: one image row down
            } else {
                const int rin = rin0[q] + dy * g.win + dx;        // (the tap offset is uniform: scalar arithmetic)
                const bool ok = (tapmask[q] >> (dy * KS + dx)) & 1u;
                off = (unsigned)(kZeroPage * 2) + (unsigned)((rin >> 4) * g.cpb + cb) * 1024u + (unsigned)((rin & 15) * 64) +
                      (unsigned)((cw[q] ^ swz((rin >> 2) & 3)) << 4);
                off = ok ? off : (unsigned)(lane * 16);           // outside the image (or past the last pixel): the zero page
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xb + off),
                                             (__attribute__((address_space(3))) void*)(st + (wave * RA + q * 16) * 64), 16, 0, 0);
        }
    }
    // ... and on to the next half stage (after the weight loads of this one: the order the kernels were tuned with)
    __device__ __forceinline__ void advance(const ConvGeom& g)
    {
        if (++cb == g.cpb) {
            cb = 0;
            if (++dx == KS) { dx = 0; ++dy; }
        }
    }
};

// ---- one step of the ring of four half stages (the scheme of avd_vit.hip; K is a run-time value here).
// The half stage about to be read must have landed; `younger` half stages (P LDS-DMAs each) were issued after it by this
// wave.  The barrier says so for every wave, and that everyone is done with the half stage before: its slot may be refilled.
template <int P>
__device__ __forceinline__ void ring_wait(int younger)
{
    __builtin_amdgcn_sched_barrier(0);
    if (younger >= 2) AVD_WAIT_VM(2 * P);
    else if (younger == 1) AVD_WAIT_VM(P);
    else AVD_WAIT_VM(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ int ring_younger(int hs, int nh) { return (hs + 2 < nh - 1 ? hs + 2 : nh - 1) - hs; }

// fragment reads of ring slot [A | B] and the wave's TI x TJ MFMAs (transposed product: b first)
template <int TI, int TJ>
__device__ __forceinline__ void ring_mfma(f32x4 (&acc)[TI][TJ], const char* a_half, const char* b_half, int wm, int wn, int lane)
{
    const int chunk = lane >> 4, r16 = lane & 15;
    bf16x8 a[TI], b[TJ];
#pragma unroll
    for (int j = 0; j < TJ; j++) b[j] = frag(b_half, b_row_of(wn, 64, j, r16), chunk);
#pragma unroll
    for (int i = 0; i < TI; i++) a[i] = frag(a_half, (wm * TI + i) * 16 + r16, chunk);
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < TJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
}

// One implicit-GEMM convolution.  MODE / KS: see TapGather.
template <int BM, int WAVES_M, int TI, int MODE, int KS>
__global__ __launch_bounds__(512) void k_conv_bf16(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Wt,
                                                  const float* __restrict__ bias, const uint16_t* __restrict__ R,
                                                  uint16_t* __restrict__ Y, ConvGeom g, int relu)
{
    using S = ConvShape<BM, WAVES_M, TI>;
    constexpr int TJ = S::TJ, BN = S::BN;
    extern __shared__ __align__(16) char lds[];            // ring of four half stages [A | B]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / S::WAVES_N, wn = wave % S::WAVES_N;
    const int tiles_n = g.cout / BN, total = tiles_of(g.m_out, BM) * tiles_n;
    const int lid = xcd_tile();
    if (lid >= total) return;
    const int m0 = (lid / tiles_n) * BM, n0 = (lid % tiles_n) * BN;

    // The per-row state is filled HERE, not in a member function: as a function of its own the tap-mask loop is compiled
    // without branches (60-125 instructions fewer) and every 3x3 shape's scalar register count moves by 1-4.
    TapGather<BM, MODE, KS> ga;
    const int hw = g.hout * g.wout;
#pragma unroll
    for (int q = 0; q < ga.QA; q++) {
        const int r = wave * ga.RA + q * 16 + (lane >> 2), m = m0 + r;
        const bool valid = m < g.m_out;
        const int img = m / hw, rem = m - img * hw, oy = rem / g.wout, ox = rem - oy * g.wout;
        ga.cw[q] = (lane & 3) ^ swz((r >> 2) & 3);         // the chunk that belongs in this lane's LDS slot
        if (MODE == 1) {                                 // byte offset of pixel (2 oy, 2 ox + 2 chunk) of the bordered image
            ga.rin0[q] = valid ? ((img * kImgSide + 2 * oy) * kImgSide + 2 * ox + 2 * ga.cw[q]) * 8 : 0;
            ga.tapmask[q] = 0;
        } else {
            const int y0 = oy * g.stride - g.pad, x0 = ox * g.stride - g.pad;
            ga.rin0[q] = (img * g.hin + y0) * g.win + x0;
            unsigned mk = 0;
#pragma unroll
            for (int t = 0; t < KS * KS; t++) {
                const int yi = y0 + t / KS, xi = x0 + t % KS;
                if (valid && (unsigned)yi < (unsigned)g.hin && (unsigned)xi < (unsigned)g.win) mk |= 1u << t;
            }
            ga.tapmask[q] = mk;
        }
    }
    unsigned vob[S::QB];
    stage_offsets<S::RB>(vob, g.nh, wave, lane);
    auto issue = [&](int hs) __attribute__((always_inline)) {
        char* st = lds + (hs & 3) * S::STAGE;
        ga.issue(g, reinterpret_cast<const char*>(X), st, hs, wave, lane);
        stage_rows<S::RB>(reinterpret_cast<const char*>(Wt + ((int64_t)(n0 >> 4) * g.nh + hs) * 512), vob, st + S::HALF_A, wave, lane);
        ga.advance(g);
    };

    f32x4 acc[TI][TJ];
    zero_acc(acc);
    const int nh = g.nh;
    for (int hs = 0; hs < 3 && hs < nh; hs++) issue(hs);
    for (int hs = 0; hs < nh; hs++) {
        ring_wait<S::P>(ring_younger(hs, nh));
        if (hs + 3 < nh) issue(hs + 3);
        const char* cur = lds + (hs & 3) * S::STAGE;
        ring_mfma(acc, cur, cur + S::HALF_A, wm, wn, lane);
    }

    // ---- epilogue: bias (+ residual), ReLU, bf16, 16 bytes per lane into the blocked layout of the next operand
    const unsigned loff = lane_in_block(lane);
    const int cblocks = g.cout >> 5;
#pragma unroll
    for (int i = 0; i < TI; i++) {
        const int rblk = (m0 >> 4) + wm * TI + i;
#pragma unroll
        for (int jp = 0; jp < TJ / 2; jp++) {
            const int col0 = n0 + wn * 64 + jp * 32;
            const int64_t boff = (int64_t)kZeroPage * 2 + ((int64_t)rblk * cblocks + (col0 >> 5)) * 1024;
            const uint4* res = R ? reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(R) + boff + loff) : nullptr;
            *reinterpret_cast<uint4*>(reinterpret_cast<char*>(Y) + boff + loff) =
                finish8(acc[i][2 * jp], acc[i][2 * jp + 1], bias8(bias + col0 + (lane >> 4) * 8), res, relu);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// A bottleneck block's 3x3 convolution AND its expanding 1x1 in one kernel ("conv2 + conv3"): the 3x3's output tile
// (BM pixels x all `mid` channels) never leaves the CU.  The expanding layers are the slowest of the unfused network
// (K = mid is short: they move a residual and an output four times the size of their input and multiply little:
// 140-260 TFLOP/s); fused, their operand comes from LDS, their residual reads and output stores overlap the NEXT
// workgroup's 3x3 on the same CU, and the mid activation's write + read (2 x 48 MB per block at 56 x 56) disappears.
//   1. the 3x3, BN = mid, one column tile: from the gather ring exactly as k_conv_bf16 (k_conv3_expand) or from a slab of
//      the input in LDS (k_slab3_expand); same K order either way: same bits;
//   2. its epilogue (bias, ReLU, bf16) goes to LDS in the operand layout (KS2 half tiles of BM rows x 64 B) and every
//      wave takes the fragments of ITS pixel rows into registers (KS2 x TI fragments) -- the 3x3's LDS is free again;
//   3. the expanding 1x1 in NCH = 4 chunks of BN output channels: W3's chunk (BN x mid, one contiguous piece of the
//      blocked weight) is copied into LDS by LDS-DMA (all four at once where they fit -- RESIDENT --, else into one of two
//      buffers while the previous chunk multiplies); epilogue = k_conv_bf16's (bias + residual + ReLU -> 16-byte stores
//      into the blocked layout).  Same k order as the unfused layer: the result is bit-identical to conv2 -> conv3.
// Expand is steps 2 and 3, placed in LDS by the kernel's shape S (W3BASE, A2BASE, BIAS3, RESIDENT).  The kernels differ in
// where the 3x3's A operand comes from and in when they request W3 and the first residuals.
template <class S>
struct Expand {
    static constexpr int BM = S::BM, BN = S::BN, TI = S::TI, TJ = S::TJ, NCH = S::NCH, KS2 = S::KS2;
    static constexpr bool RESIDENT = S::RESIDENT;
    // PF: a chunk's residuals are requested one chunk ahead (two register sets); without it (the 128-channel shapes, whose
    // fragments of the mid tile take 32 registers) at the top of their own chunk, in front of its MFMAs
    static constexpr bool PF = RESIDENT;
    static constexpr int cblocks = (NCH * BN) >> 5;
    char* lds;
    const uint16_t *W3, *R;
    uint16_t* Y;
    int wave, lane, wm, wn;
    unsigned loff, obase;
    uint4 rv0[TI][TJ / 2];                                  // with PF: the residuals of chunk 0, requested by the kernel (load_res(0, rv0))

    __device__ __forceinline__ Expand(char* lds_, const uint16_t* W3_, const uint16_t* R_, uint16_t* Y_, int m0, int wave_, int lane_)
        : lds(lds_), W3(W3_), R(R_), Y(Y_), wave(wave_), lane(lane_), wm(wave_ / S::WAVES_N), wn(wave_ % S::WAVES_N), loff(lane_in_block(lane_))
    {
        // byte offset of this lane's 16 bytes of output piece (chunk 0, row tile 0, column pair 0): 32-bit (an activation is < 4 GiB)
        obase = (unsigned)(kZeroPage * 2) + (unsigned)(((m0 >> 4) + wm * TI) * cblocks + wn * 2) * 1024u + loff;
    }
    __device__ __forceinline__ unsigned out_off(int c, int i, int jp) const { return obase + (unsigned)((i * cblocks + c * (BN >> 5) + jp) * 1024); }
    __device__ __forceinline__ char* w3_buf(int c) const { return lds + S::W3BASE + (RESIDENT ? c : (c & 1)) * S::B2; }

    __device__ __forceinline__ void issue_w3(int c)
    {
        char* buf = w3_buf(c);
        const char* src = reinterpret_cast<const char*>(W3) + (size_t)c * S::NBLK * 1024 + lane * 16;
#pragma unroll
        for (int t0 = 0; t0 < S::NBLK; t0 += 8) {
            const int t = t0 + wave, rbl = t / KS2, kb = t % KS2;     // block t of the chunk: 16 weight rows x 32 k
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + t * 1024),
                                             (__attribute__((address_space(3))) void*)(buf + kb * (BN * 64) + rbl * 1024), 16, 0, 0);
        }
    }
    // all of W3 where it is resident, else its first chunk
    __device__ __forceinline__ void issue_first_w3()
    {
        if (RESIDENT) {
#pragma unroll
            for (int c = 0; c < NCH; c++) issue_w3(c);
        } else {
            issue_w3(0);
        }
    }
    __device__ __forceinline__ void load_res(int c, uint4 (&rv)[TI][TJ / 2])
    {
#pragma unroll
        for (int i = 0; i < TI; i++)
#pragma unroll
            for (int jp = 0; jp < TJ / 2; jp++) rv[i][jp] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(R) + out_off(c, i, jp));
    }

    // acc: the 3x3's sums, its last MFMAs issued.  b3v: this thread's element of bias3, fetched before the first LDS-DMA entered
    // the in-order vector-memory queue (a load issued inside the chunk loop would make the compiler wait for everything in flight
    // around it); it is parked in LDS here.  W3_NOW: W3 (its first chunk) is requested here, as soon as the 3x3's LDS is dead;
    // otherwise the kernel has requested it already.  With PF the kernel has also requested the residuals of chunk 0.
    template <bool W3_NOW>
    __device__ __forceinline__ void run(const f32x4 (&acc2)[TI][TJ], const float* __restrict__ bias2, float b3v)
    {
        const int chunk = lane >> 4, r16 = lane & 15;
        char* const a2 = lds + S::A2BASE;
        float* const lbias3 = reinterpret_cast<float*>(lds + S::BIAS3);
        // ---- 2. the mid tile -> LDS (operand layout) -> this wave's fragments
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                        // every wave has read its last fragments: the 3x3's LDS is free
        __builtin_amdgcn_sched_barrier(0);
        // the 3x3's bias: this lane's 16 values.  (The compiler puts a vmcnt(0) in front of the LDS stores below anyway, because
        // LDS-DMAs are in flight, so this load costs no extra wait.)
        Bias8 b2[TJ / 2];
#pragma unroll
        for (int jp = 0; jp < TJ / 2; jp++) b2[jp] = bias8(bias2 + wn * 64 + jp * 32 + (lane >> 4) * 8);
        if (W3_NOW) issue_first_w3();
        if (threadIdx.x < NCH * BN) lbias3[threadIdx.x] = b3v;
#pragma unroll
        for (int i = 0; i < TI; i++)
#pragma unroll
            for (int jp = 0; jp < TJ / 2; jp++)
                *reinterpret_cast<uint4*>(a2 + (wn * 2 + jp) * (BM * 64) + (wm * TI + i) * 1024 + loff) =
                    finish8(acc2[i][2 * jp], acc2[i][2 * jp + 1], b2[jp], nullptr, true);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // this wave's part of W3 has landed, its part of the mid tile is written
        __builtin_amdgcn_s_barrier();                        // ... and everybody else's
        __builtin_amdgcn_sched_barrier(0);
        bf16x8 am[KS2][TI];
#pragma unroll
        for (int ks = 0; ks < KS2; ks++)
#pragma unroll
            for (int i = 0; i < TI; i++) am[ks][i] = frag(a2 + ks * (BM * 64), (wm * TI + i) * 16 + r16, chunk);
        if (!RESIDENT) {                                     // the second W3 buffer takes over the mid tile's LDS
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }

        f32x4 acc[TI][TJ];
        uint4 rv[PF ? 2 : 1][TI][TJ / 2];                   // residuals: the chunk being finished [and the next one, in flight]
        if (PF) {
#pragma unroll
            for (int i = 0; i < TI; i++)
#pragma unroll
                for (int jp = 0; jp < TJ / 2; jp++) rv[0][i][jp] = rv0[i][jp];
        }
        // ---- 3. the expanding 1x1, BN output channels at a time.  Vector-memory queue of a wave (in order), resident W3: res(1) st(0) |
        // res(2) st(1) | res(3) st(2) | st(3); otherwise res(c) DMA(c + 1) st(c) per chunk: the wait for DMA(c + 1) at the end of
        // iteration c leaves the stores of chunk c in flight.  The loop is unrolled by two: the residual buffers alternate.
#pragma unroll 1
        for (int c2 = 0; c2 < NCH; c2 += 2)
#pragma unroll
        for (int cc = 0; cc < 2; cc++) {
            const int c = c2 + cc;
            if (!PF) load_res(c, rv[0]);
            if (!RESIDENT && c + 1 < NCH) issue_w3(c + 1);
            if (PF && c + 1 < NCH) load_res(c + 1, rv[PF ? (c + 1) & 1 : 0]);
            __builtin_amdgcn_sched_barrier(0);
            zero_acc(acc);
            const char* buf = w3_buf(c);
#pragma unroll
            for (int ks = 0; ks < KS2; ks++) {
                bf16x8 b[TJ];
#pragma unroll
                for (int j = 0; j < TJ; j++) b[j] = frag(buf + ks * (BN * 64), b_row_of(wn, 64, j, r16), chunk);
#pragma unroll
                for (int i = 0; i < TI; i++)
#pragma unroll
                    for (int j = 0; j < TJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], am[ks][i], acc[i][j], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < TI; i++)
#pragma unroll
                for (int jp = 0; jp < TJ / 2; jp++)
                    *reinterpret_cast<uint4*>(reinterpret_cast<char*>(Y) + out_off(c, i, jp)) =
                        finish8(acc[i][2 * jp], acc[i][2 * jp + 1], bias8(lbias3 + c * BN + wn * 64 + jp * 32 + (lane >> 4) * 8),
                                &rv[PF ? (c & 1) : 0][i][jp], true);
            __builtin_amdgcn_sched_barrier(0);
            if (!RESIDENT && c + 1 < NCH) {
                AVD_WAIT_VM((PF ? 2 : 1) * S::NRES);         // younger than DMA(c + 1): [res(c + 1),] st(c)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                // the next chunk has landed for every wave; everyone is done reading this one
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
};

// The fused block with the 3x3 gathered as in k_conv_bf16 (same ring, same K order); stride 1 or 2.  W3 (its first chunk) and
// the first residuals are requested during the 3x3's LAST step, into ring slots that step no longer reads (FusedShape).
template <int BM, int WAVES_M, int TI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_conv3_expand(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W2,
                                                     const float* __restrict__ bias2, const uint16_t* __restrict__ W3,
                                                     const float* __restrict__ bias3, const uint16_t* __restrict__ R,
                                                     uint16_t* __restrict__ Y, ConvGeom g)
{
    using S = FusedShape<BM, WAVES_M, TI>;
    constexpr int TJ = S::TJ, KS = 3;
    extern __shared__ __align__(16) char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / S::WAVES_N, wn = wave % S::WAVES_N;
    const int lid = xcd_tile();
    if (lid >= tiles_of(g.m_out, BM)) return;
    const int m0 = lid * BM;
    float b3v = threadIdx.x < S::NCH * S::BN ? bias3[threadIdx.x] : 0.f;

    TapGather<BM, 0, KS> ga;                                // filled as in k_conv_bf16 (MODE 0)
    const int hw = g.hout * g.wout;
#pragma unroll
    for (int q = 0; q < ga.QA; q++) {
        const int r = wave * ga.RA + q * 16 + (lane >> 2), m = m0 + r;
        const bool valid = m < g.m_out;
        const int img = m / hw, rem = m - img * hw, oy = rem / g.wout, ox = rem - oy * g.wout;
        ga.cw[q] = (lane & 3) ^ swz((r >> 2) & 3);
        const int y0 = oy * g.stride - g.pad, x0 = ox * g.stride - g.pad;
        ga.rin0[q] = (img * g.hin + y0) * g.win + x0;
        unsigned mk = 0;
#pragma unroll
        for (int t = 0; t < KS * KS; t++) {
            const int yi = y0 + t / KS, xi = x0 + t % KS;
            if (valid && (unsigned)yi < (unsigned)g.hin && (unsigned)xi < (unsigned)g.win) mk |= 1u << t;
        }
        ga.tapmask[q] = mk;
    }
    unsigned vob[S::QB];
    stage_offsets<S::RB>(vob, g.nh, wave, lane);
    auto issue = [&](int hs) __attribute__((always_inline)) {
        char* st = lds + (hs & 3) * S::STAGE;
        ga.issue(g, reinterpret_cast<const char*>(X), st, hs, wave, lane);
        stage_rows<S::RB>(reinterpret_cast<const char*>(W2 + (int64_t)hs * 512), vob, st + S::HALF_A, wave, lane);
        ga.advance(g);
    };
    f32x4 acc[TI][TJ];
    zero_acc(acc);
    asm volatile("" : "+v"(b3v));                            // it has arrived (as far as the compiler is concerned too) before the queue fills
    Expand<S> ex(lds, W3, R, Y, m0, wave, lane);

    // ---- 1. the 3x3 (the loop of k_conv_bf16; nh >= 18)
    const int nh = g.nh;
    for (int hs = 0; hs < 3; hs++) issue(hs);
    for (int hs = 0; hs < nh - 1; hs++) {
        ring_wait<S::P>(ring_younger(hs, nh));
        if (hs + 3 < nh) issue(hs + 3);
        const char* cur = lds + (hs & 3) * S::STAGE;
        ring_mfma(acc, cur, cur + S::HALF_A, wm, wn, lane);
    }
    ring_wait<S::P>(0);                                      // everyone is past step nh - 2: three ring slots are free
    ex.issue_first_w3();
    __builtin_amdgcn_sched_barrier(0);
    if (ex.PF) ex.load_res(0, ex.rv0);
    __builtin_amdgcn_sched_barrier(0);
    const char* cur = lds + ((nh - 1) & 3) * S::STAGE;
    ring_mfma(acc, cur, cur + S::HALF_A, wm, wn, lane);

    ex.template run<false>(acc, bias2, b3v);
}

// ---------------------------------------------------------------------------------------------------------------
// The same fused block for stride 1 with the 3x3's input as ONE slab in LDS.  k_conv3_expand
// gathers the 256 output pixels' inputs from L2 once per tap: 9 x 32 KB of its 520 KB of ingest per workgroup, on a path that
// delivers ~37-40 GB/s per CU whatever the instruction (profiles/r04_experiments.md section 5).  Output pixels m0 .. m0 + 255 of
// the linear pixel index see, through the nine taps, input pixels m0 - 57 .. m0 + 312: the 384 pixels m0 - 64 .. m0 + 319 are
// 24 pixel blocks x 2 channel blocks = 48 CONTIGUOUS KiB of the blocked activation, copied once (48 LDS-DMA instructions).  A tap
// is then a fragment read at a shifted slab row -- lane (pixel r, chunk) reads row 64 + tile row + r + dy W + dx, which carries its
// own swizzle key -- with the fragment zeroed where the tap leaves the image (a per-lane 9-bit mask).  Only the weights stream:
// one tap (64 x 64 bf16 = 8 KB, one LDS-DMA instruction per wave) per step, ring of four, 16 MFMAs per wave between barriers.
// Same K order (tap, then channel block) as the gathering kernels: bit-identical.  The expanding layer follows (Expand; W3 is
// requested after the last tap, when the slab is dead).
// MID = 64 (56 x 56: 256-pixel tiles, a whole tap of W2 per step, W3 resident) or 128 (28 x 28: 128-pixel tiles, slab = 192 pixels x 4 channel
// blocks -- again 48 contiguous KiB --, W2 streams in half stages of 32 input channels = 8 KiB like the gathering kernel, W3 in two alternating
// chunk buffers).
template <int MID>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_slab3_expand(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W2,
                                                     const float* __restrict__ bias2, const uint16_t* __restrict__ W3,
                                                     const float* __restrict__ bias3, const uint16_t* __restrict__ R,
                                                     uint16_t* __restrict__ Y, ConvGeom g, int in_blocks)
{
    using S = SlabShape<MID>;
    constexpr int BN = S::BN, BM = S::BM, TI = S::TI, TJ = S::TJ, CPB = S::CPB, HALO = S::HALO, SLAB = S::SLAB, KPS = S::KPS, STEPB = S::STEPB, NSTEP = S::NSTEP;
    extern __shared__ __align__(16) char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / S::WAVES_N, wn = wave % S::WAVES_N;
    const int lid = xcd_tile();
    if (lid >= tiles_of(g.m_out, BM)) return;
    const int m0 = lid * BM;
    float b3v = threadIdx.x < S::NCH * S::BN ? bias3[threadIdx.x] : 0.f;
    asm volatile("" : "+v"(b3v));                            // arrived before the queue fills (k_conv3_expand)
    const int chunk = lane >> 4, r16 = lane & 15;
    const char* xb = reinterpret_cast<const char*>(X);

    // ---- the slab: NSLAB / 16 pixel blocks from (m0 - HALO) >> 4 on, CPB channel blocks each = 48 KiB blocks, six per wave; blocks outside
    // the activation come from the zero page (their pixels are masked in every tap: they only must not fault)
    const int blk0 = (m0 - HALO) >> 4;
#pragma unroll
    for (int j0 = 0; j0 < SLAB / 1024; j0 += 8) {
        const int j = j0 + wave, pb = blk0 + j / CPB;
        const bool ok = pb >= 0 && pb < in_blocks;          // wave-uniform
        const char* src = ok ? xb + kZeroPage * 2 + ((size_t)pb * CPB + j % CPB) * 1024 + lane * 16 : xb + lane * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(lds + j * 1024), 16, 0, 0);
    }
    // one step of W2 = KPS k blocks of all BN weight rows: eight KiB blocks, one per wave (k block of step s: s * KPS ..; K = 9 MID)
    auto issue_w2 = [&](int st) __attribute__((always_inline)) {
        const int rb = MID == 64 ? wave >> 1 : wave, kbl = MID == 64 ? wave & 1 : 0;
        const char* src = reinterpret_cast<const char*>(W2) + ((size_t)(rb * (9 * CPB) + st * KPS + kbl)) * 1024 + lane * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(lds + SLAB + (st & 3) * STEPB + kbl * (BN * 64) + rb * 1024), 16, 0, 0);
    };
    issue_w2(0); issue_w2(1); issue_w2(2);

    // per-lane tap masks of this wave's two row tiles, and the slab row of shift 0 of each
    unsigned tapmask[TI];
    int qbase[TI];
    const int hw = g.hout * g.wout;
#pragma unroll
    for (int i = 0; i < TI; i++) {
        const int pl = (wm * TI + i) * 16 + r16, m = m0 + pl;
        const bool valid = m < g.m_out;
        const int img = m / hw, rem = m - img * hw, oy = rem / g.wout, ox = rem - oy * g.wout;
        unsigned mk = 0;
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int yi = oy - 1 + t / 3, xi = ox - 1 + t % 3;
            if (valid && (unsigned)yi < (unsigned)g.hin && (unsigned)xi < (unsigned)g.win) mk |= 1u << t;
        }
        tapmask[i] = mk;
        qbase[i] = HALO + pl;
    }
    f32x4 acc[TI][TJ];
    zero_acc(acc);
    Expand<S> ex(lds, W3, R, Y, m0, wave, lane);

    // ---- 1. the nine taps (K order: tap, then channel block -- the gathering kernels' order)
#pragma unroll
    for (int st = 0; st < NSTEP; st++) {
        // steps st + 1, st + 2 may still be in flight, one LDS-DMA each (the slab is older than step 0)
        ring_wait<1>(NSTEP - 1 - st);
        if (st + 3 < NSTEP) issue_w2(st + 3);
        else if (ex.PF && st == NSTEP - 1) ex.load_res(0, ex.rv0);   // the first residuals, a whole step + the mid tile's epilogue ahead
        __builtin_amdgcn_sched_barrier(0);
        const int t = st * KPS / CPB, cb0 = st * KPS % CPB;  // tap and first channel block of the step
        const int shift = (t / 3 - 1) * g.win + (t % 3 - 1);
        const char* sb = lds + SLAB + (st & 3) * STEPB;
        bf16x8 a[TI][KPS], b[TJ][KPS];
#pragma unroll
        for (int kb = 0; kb < KPS; kb++) {
#pragma unroll
            for (int j = 0; j < TJ; j++) b[j][kb] = frag(sb + kb * (BN * 64), b_row_of(wn, 64, j, r16), chunk);
#pragma unroll
            for (int i = 0; i < TI; i++) {
                const int q = qbase[i] + shift;
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(lds + (q >> 4) * (CPB * 1024) + (cb0 + kb) * 1024 + (q & 15) * 64 +
                                                                  ((chunk ^ swz(((q & 15) >> 2) & 3)) << 4));
                a[i][kb] = ((tapmask[i] >> t) & 1u) ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int kb = 0; kb < KPS; kb++)
#pragma unroll
            for (int i = 0; i < TI; i++)
#pragma unroll
                for (int j = 0; j < TJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][kb], a[i][kb], acc[i][j], 0, 0, 0);
    }

    // ---- 2., 3. W3 (its first chunk) into the dead slab, the mid tile, the expanding 1x1
    ex.template run<true>(acc, bias2, b3v);
}

// BGR uint8 frame -> 224 x 224 (float bilinear taps, cv2's INTER_LINEAR centre mapping), RGB, (x / 255 - mean) / std,
// bf16: img[frame][y + 3][x + 3][4] of the zero-bordered 232 x 232 image (fourth channel zero; the border is cleared once,
// when the buffer is allocated).  Same arithmetic as k_vit_patchify.
__global__ __launch_bounds__(256) void k_cnn_input(const uint8_t* __restrict__ bgr, int n, int h, int w, int64_t row_stride,
                                                  int64_t frame_stride, uint16_t* __restrict__ img)
{
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= n * kSide * kSide) return;
    const int x = gid % kSide, y = (gid / kSide) % kSide, f = gid / (kSide * kSide);
    const float sx = (float)w / kSide, sy = (float)h / kSide;
    float fx = (x + 0.5f) * sx - 0.5f, fy = (y + 0.5f) * sy - 0.5f;
    int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
    fx -= x0; fy -= y0;
    if (x0 < 0) { x0 = 0; fx = 0.f; }
    if (x0 >= w - 1) { x0 = w - 1; fx = 0.f; }
    if (y0 < 0) { y0 = 0; fy = 0.f; }
    if (y0 >= h - 1) { y0 = h - 1; fy = 0.f; }
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const uint8_t* fr = bgr + (int64_t)f * frame_stride;
    const uint8_t *p00 = fr + (int64_t)y0 * row_stride + x0 * 3, *p01 = fr + (int64_t)y0 * row_stride + x1 * 3;
    const uint8_t *p10 = fr + (int64_t)y1 * row_stride + x0 * 3, *p11 = fr + (int64_t)y1 * row_stride + x1 * 3;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, istd[3] = {1.f / 0.229f, 1.f / 0.224f, 1.f / 0.225f};   // RGB (ImageNet)
    uint16_t v4[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int s = 2 - c;
        const float top = p00[s] + (p01[s] - (float)p00[s]) * fx, bot = p10[s] + (p11[s] - (float)p10[s]) * fx;
        const float v = top + (bot - top) * fy;
        v4[c] = f32_to_bf16((v * (1.f / 255.f) - mean[c]) * istd[c]);
    }
    uint2 pk;
    pk.x = v4[0] | ((unsigned)v4[1] << 16);
    pk.y = v4[2];
    reinterpret_cast<uint2*>(img)[((int64_t)f * kImgSide + y + 3) * kImgSide + x + 3] = pk;
}

__device__ __forceinline__ unsigned max_bf16x2(unsigned a, unsigned b)     // inputs are >= 0 (after a ReLU): integer order = value order
{
    const unsigned lo = max(a & 0xFFFFu, b & 0xFFFFu), hi = max(a >> 16, b >> 16);
    return lo | (hi << 16);
}

// 3x3 / 2 max pool (pad 1) over a blocked [n * hin * win][c] activation of non-negative values
__global__ __launch_bounds__(256) void k_maxpool3(const uint16_t* __restrict__ X, int n, int hin, int win, int c, uint16_t* __restrict__ Y)
{
    const int hout = hin / 2, wout = win / 2, c8n = c / 8;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)n * hout * wout * c8n) return;
    const int c8 = (int)(gid % c8n);
    const int m = (int)(gid / c8n);
    const int f = m / (hout * wout), rem = m - f * hout * wout, oy = rem / wout, ox = rem - oy * wout;
    uint4 best = {0, 0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < 3; dy++)
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            const int yi = oy * 2 - 1 + dy, xi = ox * 2 - 1 + dx;
            if ((unsigned)yi < (unsigned)hin && (unsigned)xi < (unsigned)win) {
                const uint4 v = *reinterpret_cast<const uint4*>(X + kZeroPage + blocked_index((f * hin + yi) * win + xi, c8 * 8, c));
                best.x = max_bf16x2(best.x, v.x); best.y = max_bf16x2(best.y, v.y);
                best.z = max_bf16x2(best.z, v.z); best.w = max_bf16x2(best.w, v.w);
            }
        }
    *reinterpret_cast<uint4*>(Y + kZeroPage + blocked_index(m, c8 * 8, c)) = best;
}

// global average pool: blocked [n * hw][c] -> f32 [n][c] (sum in f32 in pixel order, then / hw)
__global__ __launch_bounds__(256) void k_avgpool(const uint16_t* __restrict__ X, int n, int hw, int c, float* __restrict__ out)
{
    const int c8n = c / 8;
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= n * c8n) return;
    const int c8 = gid % c8n, f = gid / c8n;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < hw; p++) {
        const uint4 v = *reinterpret_cast<const uint4*>(X + kZeroPage + blocked_index(f * hw + p, c8 * 8, c));
        s[0] += bf16_to_f32(v.x & 0xFFFF); s[1] += bf16_to_f32(v.x >> 16); s[2] += bf16_to_f32(v.y & 0xFFFF); s[3] += bf16_to_f32(v.y >> 16);
        s[4] += bf16_to_f32(v.z & 0xFFFF); s[5] += bf16_to_f32(v.z >> 16); s[6] += bf16_to_f32(v.w & 0xFFFF); s[7] += bf16_to_f32(v.w >> 16);
    }
    const float inv = 1.f / hw;
#pragma unroll
    for (int e = 0; e < 8; e++) out[(int64_t)f * c + c8 * 8 + e] = s[e] * inv;
}

// logits[f][o] = pooled[f][:] . W[o][:] + b[o]; one wave per (output, group of 8 frames): the weight row (k = 2048: 32
// values per lane) stays in registers, the pooled features come from L2
__global__ __launch_bounds__(256) void k_linear(const float* __restrict__ x, const uint16_t* __restrict__ W, const float* __restrict__ b,
                                               int n, int nout, float* __restrict__ y)
{
    constexpr int K = 2048, FG = 8;
    const int groups = (n + FG - 1) / FG;
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= groups * nout) return;
    const int o = wid % nout, f0 = (wid / nout) * FG;
    float wr[K / 64];
#pragma unroll
    for (int i = 0; i < K / 64; i++) wr[i] = bf16_to_f32(W[(int64_t)o * K + i * 64 + lane]);
    const float bo = b[o];
    for (int f = f0; f < f0 + FG && f < n; f++) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < K / 64; i++) s = __builtin_fmaf(x[(int64_t)f * K + i * 64 + lane], wr[i], s);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0) y[(int64_t)f * nout + o] = s + bo;
    }
}

// ---- network description -----------------------------------------------------------------------------------------
struct Layer { int cin, cout, ksize, stride; size_t w_off, b_off; };        // offsets into the flat parameter arrays (elements)

struct Net {
    std::vector<Layer> convs;          // stem, then per block: conv1, conv2, conv3 [, downsample]
    size_t n_w = 0, n_b = 0;           // including the final linear layer
    size_t fc_w = 0, fc_b = 0;
    Net()
    {
        auto add = [&](int cin, int cout, int k, int s) {
            convs.push_back({cin, cout, k, s, n_w, n_b});
            n_w += (size_t)cout * k * k * cin;
            n_b += cout;
        };
        add(3, 64, 7, 2);
        const int depth[4] = {3, 4, 6, 3};
        int cin = 64;
        for (int st = 0; st < 4; st++) {
            const int mid = 64 << st, out = mid * 4;
            for (int b = 0; b < depth[st]; b++) {
                const int s = (b == 0 && st > 0) ? 2 : 1;
                add(cin, mid, 1, 1);
                add(mid, mid, 3, s);
                add(mid, out, 1, 1);
                if (b == 0) add(cin, out, 1, s);
                cin = out;
            }
        }
        fc_w = n_w; fc_b = n_b;
        n_w += (size_t)1000 * 2048;
        n_b += 1000;
    }
};
const Net& net() { static const Net n; return n; }

int k_padded(const Layer& l) { return l.ksize == 7 ? 7 * 8 * 4 : l.ksize * l.ksize * l.cin; }   // the stem: [7 ky][8 kx][4 c], kx = 7 and c = 3 zero

// a grid of `workgroups` tiles (rounded up to whole XCD rounds: xcd_tile) of 512 threads with `lds` bytes of dynamic LDS
template <class K, class... Args>
int launch_tiles(avd_ctx* ctx, K kern, int workgroups, size_t lds, Args... args)
{
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((workgroups + 7) / 8 * 8), dim3(512), lds, ctx->stream, args...);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <int BM, int WAVES_M, int TI, int MODE, int KS>
int launch_conv_shape(avd_ctx* ctx, const ConvGeom& g, const uint16_t* x, const uint16_t* w, const float* bias, const uint16_t* res, uint16_t* y, int relu)
{
    using S = ConvShape<BM, WAVES_M, TI>;
    return launch_tiles(ctx, k_conv_bf16<BM, WAVES_M, TI, MODE, KS>, tiles_of(g.m_out, S::BM) * (g.cout / S::BN), S::lds(g.nh), x, w, bias, res, y, g, relu);
}

// stem == true: x is the bordered input image, (hin, win, cin, ksize, stride) describe the 7x7/2 convolution.  *ran = the kernel shape it launched
int launch_conv(avd_ctx* ctx, CnnShape* ran, const uint16_t* x, const uint16_t* w, const float* bias, const uint16_t* res, uint16_t* y, int n, int hin,
                int win, int cin, int cout, int ksize, int stride, int relu, bool stem = false)
{
    const ConvGeom g = conv_geom(n, hin, win, cin, cout, ksize, stride, stem);
    if (!stem && (cin % 32 || cout % 64 || (ksize != 1 && ksize != 3))) { ctx->err = "conv: cin % 32, cout % 64, ksize 1 or 3"; return AVD_ERR_ARG; }
    if (stem) { *ran = kCnnStem; return launch_conv_shape<256, 8, 2, 1, 1>(ctx, g, x, w, bias, res, y, relu); }
    // 256-pixel tiles for the long-K layers that fill the chip.  128 x 128 tiles (74 registers, 16 KiB per ring slot: several
    // workgroups per CU) where 256-pixel tiles would leave most of the chip idle (the 14 x 14 and 7 x 7 stages), and for the
    // short-K 1x1 layers, which move bytes rather than multiply: there the time goes to load / store latency, and
    // co-resident workgroups are what hides it.
    const int force = ctx->cnn_tiles;   // avd_set_option "cnn_tiles": 1 = always 256-pixel tiles, 2 = 128 x 128 wherever possible
    const int bn_big = cout % 256 == 0 ? 256 : cout % 128 == 0 ? 128 : 64;
    const int wgs_big = tiles_of(g.m_out, 256) * (cout / bn_big);
    const bool small_ok = cout % 128 == 0;
    // fill_pct = workgroups of the 256-pixel tiling, in percent of the CU count, below which the 128 x 128 tiling is taken;
    // short_k = largest number of half stages that counts as "short K"
    constexpr int fill_pct = 150, short_k = 8;
    const bool want_small = wgs_big * 100 < ctx->num_cus * fill_pct || g.nh <= short_k;
    auto tiled = [&](auto ks) -> int {
        constexpr int KS = decltype(ks)::value;
        if (small_ok && force != 1 && (want_small || force == 2)) { *ran = kCnn128x128; return launch_conv_shape<128, 4, 2, 0, KS>(ctx, g, x, w, bias, res, y, relu); }
        if (bn_big == 256) { *ran = kCnn256x256; return launch_conv_shape<256, 2, 8, 0, KS>(ctx, g, x, w, bias, res, y, relu); }
        if (bn_big == 128) { *ran = kCnn256x128; return launch_conv_shape<256, 4, 4, 0, KS>(ctx, g, x, w, bias, res, y, relu); }
        *ran = kCnn256x64;
        return launch_conv_shape<256, 8, 2, 0, KS>(ctx, g, x, w, bias, res, y, relu);
    };
    return ksize == 3 ? tiled(std::integral_constant<int, 3>{}) : tiled(std::integral_constant<int, 1>{});
}

// conv2 (3x3, mid -> mid, stride s, ReLU) + conv3 (1x1, mid -> 4 mid, + residual, ReLU) of a bottleneck block in one launch
// (k_conv3_expand, or k_slab3_expand in the stride-1 blocks with cnn_fuse = 2); mid = 64 (256-pixel tiles) or 128 (128-pixel
// tiles).  y must not be the 3x3's input.  *ran = which of the two it launched
bool can_fuse_expand(int mid) { return mid == 64 || mid == 128; }
int launch_conv3_expand(avd_ctx* ctx, CnnShape* ran, const uint16_t* x, const uint16_t* w2, const float* b2, const uint16_t* w3, const float* b3,
                        const uint16_t* res, uint16_t* y, int n, int hin, int win, int mid, int stride)
{
    const ConvGeom g = conv_geom(n, hin, win, mid, mid, 3, stride);
    if (!can_fuse_expand(mid) || !res || y == x) { ctx->err = "conv3_expand: mid 64 or 128, a residual, output apart from the input"; return AVD_ERR_ARG; }
    if (stride == 1 && ctx->cnn_fuse == 2) {
        // the 3x3's input as one slab in LDS; the blocks of the input activation that exist: its rows are padded to 256
        const int in_blocks = (int)(((size_t)n * hin * win + 255) / 256 * 256 / 16);
        auto slab = [&](auto shape, auto kern) -> int {
            using S = decltype(shape);
            if (win + 1 > S::HALO) { ctx->err = "conv3_expand: the slab's halo is sized for 56 x 56 (mid 64) and 28 x 28 (mid 128)"; return AVD_ERR_ARG; }
            *ran = kCnnSlab3Expand;
            return launch_tiles(ctx, kern, tiles_of(g.m_out, S::BM), S::LDS, x, w2, b2, w3, b3, res, y, g, in_blocks);
        };
        return mid == 64 ? slab(SlabShape<64>{}, k_slab3_expand<64>) : slab(SlabShape<128>{}, k_slab3_expand<128>);
    }
    auto gather = [&](auto shape, auto kern) -> int {
        using S = decltype(shape);
        // the kernel's LDS plan assumes which ring slot the 3x3's last step reads
        if ((g.nh & 3) != S::PHASE) { ctx->err = "conv3_expand: ring phase"; return AVD_ERR_ARG; }
        *ran = kCnnConv3Expand;
        return launch_tiles(ctx, kern, tiles_of(g.m_out, S::BM), S::LDS, x, w2, b2, w3, b3, res, y, g);
    };
    return mid == 64 ? gather(FusedShape<256, 8, 2>{}, k_conv3_expand<256, 8, 2>) : gather(FusedShape<128, 4, 2>{}, k_conv3_expand<128, 4, 2>);
}

size_t act_elems(size_t rows, int c) { return kZeroPage + (rows + 255) / 256 * 256 * (size_t)c; }

}  // namespace

void cnn_param_counts(size_t* n_w, size_t* n_b) { *n_w = net().n_w; *n_b = net().n_b; }

// flat parameters (conv weights [cout][kh][kw][cin] bf16 in network order, then the linear layer [1000][2048]; biases
// f32 in the same order) -> device: every convolution's weight re-tiled into the blocked operand layout
int cnn_set_weights(avd_ctx* ctx, const uint16_t* w, const float* b)
{
    const Net& nt = net();
    Weights& wt = ctx->weights;
    size_t blocked_total = 0;
    for (const Layer& l : nt.convs) blocked_total += (size_t)l.cout * k_padded(l);
    std::vector<uint16_t> host(blocked_total + (size_t)1000 * 2048), tmp;
    size_t off = 0;
    wt.cnn_w_off.clear();
    for (const Layer& l : nt.convs) {
        const int K = k_padded(l), kin = l.ksize * l.ksize * l.cin;
        const uint16_t* src = w + l.w_off;
        if (K != kin) {                                      // the stem: [cout][7][7][3] -> [cout][7 ky][8 kx][4 c], the extra taps zero
            tmp.assign((size_t)l.cout * K, 0);
            for (int o = 0; o < l.cout; o++)
                for (int ky = 0; ky < 7; ky++)
                    for (int kx = 0; kx < 7; kx++)
                        for (int c = 0; c < 3; c++) tmp[(size_t)o * K + (ky * 8 + kx) * 4 + c] = src[(size_t)o * kin + (ky * 7 + kx) * 3 + c];
            src = tmp.data();
        }
        gemm_block_operand(src, host.data() + off, l.cout, K);
        wt.cnn_w_off.push_back(off);
        off += (size_t)l.cout * K;
    }
    wt.cnn_fc_off = off;
    for (size_t i = 0; i < (size_t)1000 * 2048; i++) host[off + i] = w[nt.fc_w + i];
    if (int e = wt.d_cnn_w.reserve(ctx, host.size())) return e;
    if (int e = wt.d_cnn_b.reserve(ctx, nt.n_b)) return e;
    HIP_TRY(ctx, hipMemcpyAsync(wt.d_cnn_w, host.data(), host.size() * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(wt.d_cnn_b, b, nt.n_b * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AVD_OK;
}

// activation scratch for n frames: four rotating activations, the zero-bordered 224 x 224 input, pooled features, logits
int cnn_reserve(avd_ctx* ctx, int n)
{
    Workspace& ws = ctx->ws;
    if (n <= ws.cnn_frames) return AVD_OK;
    ws.cnn_frames = 0;                                                   // not valid again until every buffer below exists
    // the largest activation: the stem's, or a 56 x 56 x 256 one, whose rows pad further (n * 3136 is a multiple of 256 only when n % 4 == 0) --
    // every tile stores all its rows, so the padding rows must exist
    const size_t act = std::max(act_elems((size_t)n * 112 * 112, 64), act_elems((size_t)n * 56 * 56, 256));
    for (int i = 0; i < 4; i++) {
        if (int e = ws.d_cnn_act[i].reserve(ctx, act)) return e;
        HIP_TRY(ctx, hipMemsetAsync(ws.d_cnn_act[i], 0, kZeroPage * sizeof(uint16_t), ctx->stream));
    }
    if (int e = ws.d_cnn_img.reserve(ctx, (size_t)n * kImgSide * kImgSide * 4)) return e;
    HIP_TRY(ctx, hipMemsetAsync(ws.d_cnn_img, 0, (size_t)n * kImgSide * kImgSide * 4 * sizeof(uint16_t), ctx->stream));   // the zero border
    if (int e = ws.d_cnn_pool.reserve(ctx, (size_t)n * 2048)) return e;
    if (int e = ws.d_cnn_logits.reserve(ctx, (size_t)n * 1000)) return e;
    ws.cnn_frames = n;
    return AVD_OK;
}

// frames (device BGR) -> logits (device f32 [n][1000]); everything on ctx->stream.  Option "cnn_tap" (tests): the one intermediate it names is
// copied into ws.d_cnn_tap right after the launch that produces it; with the option at 0 nothing is enqueued for it.
int launch_cnn_forward(avd_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, int64_t row_stride, int64_t frame_stride)
{
    const Net& nt = net();
    Workspace& ws = ctx->ws;
    const Weights& wt = ctx->weights;
    if (nt.convs.size() != (size_t)kCnnConvs) { ctx->err = "cnn: kCnnConvs"; return AVD_ERR_ARG; }
    int plan[kCnnConvs] = {};                                // kCnnFolded unless a launch of its own is recorded below
    ws.cnn_tap_asked = ctx->cnn_tap;
    ws.cnn_tap_point = 0;                                    // whatever an earlier forward left is no longer "the last forward's"
    // a tile stores ALL its rows, a tail tile's padding rows too: [rows][c] padded to whole tiles must lie inside a scratch buffer
    auto fits = [&](size_t rows, int c) -> int {
        if (act_elems(rows, c) <= ws.d_cnn_act[0].cap) return 0;
        ctx->err = "cnn: an activation of " + std::to_string(rows) + " x " + std::to_string(c) + ", padded to whole tiles, is larger than the scratch buffers";
        return AVD_ERR_NOMEM;
    };
    // c != 0: the blocked activation [rows][c] at src (its zero page and padding rows included); c == 0: `bytes` plain bytes
    auto tap = [&](int point, const void* src, size_t rows, int c, size_t bytes = 0) -> int {
        if (ctx->cnn_tap != point) return 0;
        if (c) bytes = act_elems(rows, c) * sizeof(uint16_t);
        if (int e = ws.d_cnn_tap.reserve(ctx, (bytes + 1) / 2)) return e;
        HIP_TRY(ctx, hipMemcpyAsync(ws.d_cnn_tap, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        ws.cnn_tap_point = point; ws.cnn_tap_rows = rows; ws.cnn_tap_c = c; ws.cnn_tap_bytes = bytes;
        return 0;
    };
    auto wptr = [&](size_t i) { return wt.d_cnn_w + wt.cnn_w_off[i]; };
    auto bptr = [&](size_t i) { return wt.d_cnn_b + nt.convs[i].b_off; };
    // convolution i of the network (hin x hin input, even): launched, recorded in the plan, tapped
    auto conv = [&](size_t i, const uint16_t* x, const uint16_t* res, uint16_t* y, int hin, int ci, int co, int ksize, int s, int relu, bool stem = false) -> int {
        const size_t rows = (size_t)n * (hin / s) * (hin / s);
        if (int e = fits(rows, co)) return e;
        CnnShape ran;
        if (int e = launch_conv(ctx, &ran, x, wptr(i), bptr(i), res, y, n, hin, hin, ci, co, ksize, s, relu, stem)) return e;
        plan[i] = ran;
        return tap(kCnnTapConv0 + (int)i, y, rows, co);
    };
    const int64_t px = (int64_t)n * kSide * kSide;
    hipLaunchKernelGGL(k_cnn_input, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, ctx->stream, d_bgr, n, h, w, row_stride, frame_stride, ws.d_cnn_img);
    if (int e = tap(kCnnTapImage, ws.d_cnn_img, 0, 0, (size_t)n * kImgSide * kImgSide * 4 * sizeof(uint16_t))) return e;
    // the stem gathers straight from the bordered image (one half stage per kernel row)
    if (int e = conv(0, ws.d_cnn_img, nullptr, ws.d_cnn_act[0], kSide, 3, 64, 7, 2, 1, true)) return e;
    size_t li = 1;
    const int64_t pooled = (int64_t)n * 56 * 56 * 8;
    hipLaunchKernelGGL(k_maxpool3, dim3((unsigned)((pooled + 255) / 256)), dim3(256), 0, ctx->stream, ws.d_cnn_act[0], n, 112, 112, 64, ws.d_cnn_act[1]);
    if (int e = tap(kCnnTapMaxPool, ws.d_cnn_act[1], (size_t)n * 56 * 56, 64)) return e;
    int cur = 1, hgt = 56;                                   // index of the block input among the four rotating buffers
    const int depth[4] = {3, 4, 6, 3};
    int cin = 64;
    for (int st = 0; st < 4; st++) {
        const int mid = 64 << st, out = mid * 4;
        for (int b = 0; b < depth[st]; b++) {
            const int s = (b == 0 && st > 0) ? 2 : 1;
            const int t1 = (cur + 1) & 3, t2 = (cur + 2) & 3, sc = (cur + 3) & 3;
            uint16_t *x = ws.d_cnn_act[cur], *a1 = ws.d_cnn_act[t1], *a2 = ws.d_cnn_act[t2], *a3 = ws.d_cnn_act[sc];
            if (int e = conv(li, x, nullptr, a1, hgt, cin, mid, 1, 1, 1)) return e;
            const int ho = hgt / s;
            const uint16_t* res = x;
            if (b == 0) {                                    // projection shortcut into a3
                if (int e = conv(li + 3, x, nullptr, a3, hgt, cin, out, 1, s, 0)) return e;
                res = a3;
            }
            if (ctx->cnn_fuse && can_fuse_expand(mid)) {     // conv2 + conv3 in one launch: a1 -> a2 (other workgroups still read a1's halo)
                const size_t rows = (size_t)n * ho * ho;
                if (int e = fits(rows, out)) return e;
                CnnShape ran;
                if (int e = launch_conv3_expand(ctx, &ran, a1, wptr(li + 1), bptr(li + 1), wptr(li + 2), bptr(li + 2), res, a2, n, hgt, hgt, mid, s)) return e;
                plan[li + 1] = ran;                          // recorded at the 3x3, whose output never leaves the CU: nothing to tap there
                if (int e = tap(kCnnTapConv0 + (int)li + 2, a2, rows, out)) return e;
                cur = t2;
            } else {                                         // conv3 writes over a1
                if (int e = conv(li + 1, a1, nullptr, a2, hgt, mid, mid, 3, s, 1)) return e;
                if (int e = conv(li + 2, a2, res, a1, ho, mid, out, 1, 1, 1)) return e;
                cur = t1;
            }
            li += b == 0 ? 4 : 3;
            hgt = ho; cin = out;
        }
    }
    hipLaunchKernelGGL(k_avgpool, dim3((unsigned)((n * 256 + 255) / 256)), dim3(256), 0, ctx->stream, ws.d_cnn_act[cur], n, 49, 2048, ws.d_cnn_pool);
    if (int e = tap(kCnnTapPooled, ws.d_cnn_pool, 0, 0, (size_t)n * 2048 * sizeof(float))) return e;
    hipLaunchKernelGGL(k_linear, dim3((unsigned)(((n + 7) / 8 * 1000 + 3) / 4)), dim3(256), 0, ctx->stream, ws.d_cnn_pool, wt.d_cnn_w + wt.cnn_fc_off,
                       wt.d_cnn_b + nt.fc_b, n, 1000, ws.d_cnn_logits);
    HIP_TRY(ctx, hipGetLastError());
    for (int i = 0; i < kCnnConvs; i++) ctx->cnn_plan[i] = plan[i];
    ctx->cnn_plan_valid = 1;
    return AVD_OK;
}

// avd_debug_fetch "cnn_tap": what the last forward copied aside, an activation de-blocked to plain NHWC (out_bytes must be the tap's size)
int64_t cnn_tap_fetch(avd_ctx* ctx, void* out, size_t out_bytes)
{
    Workspace& ws = ctx->ws;
    if (!ws.cnn_tap_point || !ws.d_cnn_tap) {
        ctx->err = ws.cnn_tap_asked ? "cnn_tap: no launch of the last forward had that output (a fused block's 3x3 has none of its own while cnn_fuse != 0)"
                                    : "cnn_tap: the last forward copied nothing (option cnn_tap was 0, or no forward has run since the workspace was released)";
        return AVD_ERR_ARG;
    }
    const int c = ws.cnn_tap_c;
    const size_t want = c ? ws.cnn_tap_rows * c * sizeof(uint16_t) : ws.cnn_tap_bytes;
    if (out_bytes != want) { ctx->err = "cnn_tap: tap " + std::to_string(ws.cnn_tap_point) + " holds " + std::to_string(want) + " bytes"; return AVD_ERR_ARG; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!c) {
        HIP_TRY(ctx, hipMemcpy(out, ws.d_cnn_tap, want, hipMemcpyDeviceToHost));
        return (int64_t)want;
    }
    std::vector<uint16_t> blocked(ws.cnn_tap_bytes / sizeof(uint16_t));
    HIP_TRY(ctx, hipMemcpy(blocked.data(), ws.d_cnn_tap, ws.cnn_tap_bytes, hipMemcpyDeviceToHost));
    uint16_t* y = static_cast<uint16_t*>(out);
    for (size_t m = 0; m < ws.cnn_tap_rows; m++)
        for (int k = 0; k < c; k++) y[m * c + k] = blocked[kZeroPage + blocked_index((int)m, k, c)];
    return (int64_t)want;
}

// ONE convolution on host tensors in NHWC order (test entry: the blocked layout stays an internal matter)
int cnn_conv_host(avd_ctx* ctx, const uint16_t* x, int n, int hin, int win, int cin, const uint16_t* w, const float* bias, int cout, int ksize,
                  int stride, int relu, const uint16_t* residual, uint16_t* y)
{
    if (cin % 32 || cout % 64 || (ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || n <= 0) {
        ctx->err = "cnn_conv: cin % 32 == 0, cout % 64 == 0, ksize 1 or 3, stride 1 or 2";
        return AVD_ERR_ARG;
    }
    const int pad = ksize / 2, hout = (hin + 2 * pad - ksize) / stride + 1, wout = (win + 2 * pad - ksize) / stride + 1;
    const size_t min_ = (size_t)n * hin * win, mout = (size_t)n * hout * wout;
    const int K = ksize * ksize * cin;
    std::vector<uint16_t> hx(act_elems(min_, cin), 0), hw((size_t)cout * K), hr, hy(act_elems(mout, cout), 0);
    for (size_t m = 0; m < min_; m++)
        for (int c = 0; c < cin; c++) hx[kZeroPage + blocked_index((int)m, c, cin)] = x[m * cin + c];
    gemm_block_operand(w, hw.data(), cout, K);
    if (residual) {
        hr.assign(act_elems(mout, cout), 0);
        for (size_t m = 0; m < mout; m++)
            for (int c = 0; c < cout; c++) hr[kZeroPage + blocked_index((int)m, c, cout)] = residual[m * cout + c];
    }
    uint16_t *dx = nullptr, *dw = nullptr, *dr = nullptr, *dy = nullptr;
    float* db = nullptr;
    int rc = AVD_OK;
    auto cleanup = [&]() { (void)hipFree(dx); (void)hipFree(dw); (void)hipFree(dr); (void)hipFree(dy); (void)hipFree(db); };
#define CNN_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { ctx->err = hipGetErrorString(e_); cleanup(); return AVD_ERR_DEVICE; } } while (0)
    CNN_TRY(hipMalloc(&dx, hx.size() * 2)); CNN_TRY(hipMalloc(&dw, hw.size() * 2)); CNN_TRY(hipMalloc(&dy, hy.size() * 2));
    CNN_TRY(hipMalloc(&db, cout * sizeof(float)));
    if (residual) CNN_TRY(hipMalloc(&dr, hr.size() * 2));
    CNN_TRY(hipMemcpyAsync(dx, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, ctx->stream));
    CNN_TRY(hipMemcpyAsync(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice, ctx->stream));
    CNN_TRY(hipMemcpyAsync(db, bias, cout * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    CNN_TRY(hipMemsetAsync(dy, 0, hy.size() * 2, ctx->stream));
    if (residual) CNN_TRY(hipMemcpyAsync(dr, hr.data(), hr.size() * 2, hipMemcpyHostToDevice, ctx->stream));
    CnnShape ran;                                            // nobody asks for it here
    rc = launch_conv(ctx, &ran, dx, dw, db, dr, dy, n, hin, win, cin, cout, ksize, stride, relu);
    if (rc == AVD_OK) {
        CNN_TRY(hipMemcpyAsync(hy.data(), dy, hy.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
        CNN_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t m = 0; m < mout; m++)
            for (int c = 0; c < cout; c++) y[m * cout + c] = hy[kZeroPage + blocked_index((int)m, c, cout)];
    }
#undef CNN_TRY
    cleanup();
    return rc;
}
