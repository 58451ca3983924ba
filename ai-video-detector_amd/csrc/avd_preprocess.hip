// avd_preprocess.hip -- fused full-resolution pass over decoded frames (gfx950): BGR, RGB in four layouts, NV12, I420, 4:2:2 in four layouts, 10-bit 4:2:0 in two.
//
// One read of each frame from HBM produces everything the reference derives
// from full-resolution pixels (reference app/analyzers/video.py):
//   :5,:43,:51  cv2.cvtColor(BGR2GRAY) x3   -> gray lives only in LDS
//   :6          cv2.resize(32x32, INTER_AREA) -> per-row partial sums (float, cv2's order)
//   :43         cv2.resize(320x320) INTER_LINEAR (11-bit fixed point)
//   :52         cv2.Laplacian(CV_64F).var()  -> exact int64 sum / sum of squares
// HBM-bound: algorithmic traffic = one frame read + 102 400 B small image + 16 B moments
// + the 32 floats/row area partials (DESIGN.md "preprocess kernel").
//
// Work decomposition: a workgroup owns a band of `rows_per_band` full-width rows of one
// frame.  Phase 1 streams the band (+1 halo row above/below) through the 15-bit
// fixed-point gray conversion into an LDS tile of uint8; phases 2-4 read only LDS.
// Consecutive bands of a frame are placed on the same XCD (blockIdx remap) so the
// halo rows hit that XCD's L2.
//
// Measured design notes (profiles/r01_preprocess_ablation.md): byte ops (v_dot4_u32_u8,
// v_alignbyte, v_perm) issue at half rate on gfx950, the kernel is balanced between the load
// path (0.13 ms alone) and the arithmetic (0.14 ms alone); persistent software-pipelined
// variants (next band's loads in flight in registers during the arithmetic, 256 or 512 threads)
// were built and were 30-40 % SLOWER than many small independent workgroups (4 per CU): the
// dependent float chains of INTER_AREA want thread-level parallelism more than prefetch.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include "avd_internal.h"

namespace {

constexpr int kThreads = 256;       // workgroup size of the ingest kernels
constexpr int kPad = 16;            // bytes of padding left of pixel 0 in every LDS tile row
constexpr int kMaxNI = 9;           // k_preprocess_vec: row chunks (3 x 16 B each) a lane holds in registers at most
constexpr int kBandCap = 14;        // rows per band at most: 16 tile rows + LDS tables = 37 KiB at 1080p, 4 workgroups per CU
constexpr int kLdsBudget = 48 * 1024;   // the tile stays under this so that >= 3 workgroups fit a CU
static_assert(kThreads / 64 <= kLapSlots, "one moment slot per wave");

// What a layout's kernels take besides plane 0 (the kernel's first argument) and PreParams: its other planes, frame 0's (or, for a listed clip,
// the tables of their per-frame pointers), and what only this layout needs.  Packed layouts take nothing.
struct Nv12Params {
    const uint8_t* uv;                 // interleaved U,V plane (NV12: h/2 rows; NV16: h rows)
    int64_t uv_row_stride, uv_frame_stride;
    YuvConsts k;
};
struct I420Params {
    const uint8_t *u, *v;              // planar U and V, uint8[h/2][w/2] each (I422: [h][w/2]; YV12 / YV16: the caller passes them exchanged)
    int64_t c_row_stride, c_frame_stride;   // shared by the two planes
    YuvConsts k;
};
struct YuyvParams {                    // packed 4:2:2: one plane, only the constants
    YuvConsts k;
};
struct RgbpParams {
    const uint8_t *g, *b;              // the G and B planes (plane 0 is R); all three share PreParams' strides
};

// LDS plan, read by the kernels and by the launcher.  The tile is (rows_per_band + 2) rows of `pitch` bytes; behind it sit either the
// resampling tables of k_preprocess_vec (LdsTabs, behind the FULL tile) or the three conversion tables of the 4:2:0 and 4:2:2 table fills (behind the
// rows the band has, rounded to 16: a short last band has them lower than the launcher reserved for).  Their length and index bias travel
// with the conversion constants (YuvConsts::ntab, ::bias): the window of Y + offset follows the constants -- [-221, 475] limited range,
// [-226, 480] full range -- and launch_preprocess refuses constants whose window leaves the table.
__host__ __device__ constexpr size_t lds_tile_bytes(int trows, int pitch) { return (size_t)trows * pitch; }
__host__ __device__ constexpr size_t lds_nvtab_off(int trows, int pitch) { return (lds_tile_bytes(trows, pitch) + 15) / 16 * 16; }
__host__ __device__ constexpr size_t lds_nvtab_bytes(int ntab) { return 3 * sizeof(unsigned) * (size_t)ntab; }

__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// 15-bit fixed-point luma, split into byte coefficients for v_dot4_u32_u8:
//   3735 = 14*256+151 (B)   19235 = 75*256+35 (G)   9798 = 38*256+70 (R)
// gray = (256 h + l) >> 15 with h = px . hi, l = px . lo + 2^14.  Since 256 h + l = 256 (h + (l >> 8)) + (l & 255),
// gray = (h + (l >> 8)) >> 7 = byte 1 of 2 h + 2 (l >> 8); 2 (l >> 8) and l >> 7 differ in bit 0 only and 2 h is even,
// so byte 1 of  v = px . (2 hi) + (l >> 7)  is the gray value: dot4, shift, dot4 -- and the four results of a
// quad are packed by two v_perm picking byte 1 of each.
constexpr unsigned kHi2 = 28u | (150u << 8) | (76u << 16);
constexpr unsigned kLo = 151u | (35u << 8) | (70u << 16);
// The same for pixels stored R, G, B (AVD_FMT_RGB24, AVD_FMT_RGBA32, the pixel words gathered from AVD_FMT_RGBP): bytes 0 and 2 exchanged.  The
// channel order is a constant of the fill -- the template parameter RGB of everything below -- and nothing else knows it.  Byte 3 of either
// constant is zero: a 32-bit pixel's fourth byte (AVD_FMT_BGRA32 / _RGBA32) drops out of both dot products.
constexpr unsigned kHi2Rgb = 76u | (150u << 8) | (28u << 16);
constexpr unsigned kLoRgb = 70u | (35u << 8) | (151u << 16);
template <bool RGB> constexpr unsigned hi2_of() { return RGB ? kHi2Rgb : kHi2; }
template <bool RGB> constexpr unsigned lo_of() { return RGB ? kLoRgb : kLo; }

__device__ __forceinline__ unsigned gray_v(unsigned px, unsigned hi2, unsigned lo)
{
    const unsigned l = __builtin_amdgcn_udot4(px, lo, 1u << 14, false);
    return __builtin_amdgcn_udot4(px, hi2, l >> 7, false);       // gray in bits 8..15
}

// 12 bytes (4 BGR or RGB pixels) -> 4 gray bytes packed little-endian
template <bool RGB>
__device__ __forceinline__ unsigned gray4(unsigned w0, unsigned w1, unsigned w2)
{
    constexpr unsigned hi2 = hi2_of<RGB>(), lo = lo_of<RGB>();
    const unsigned p1 = __builtin_amdgcn_alignbyte(w1, w0, 3);
    const unsigned p2 = __builtin_amdgcn_alignbyte(w2, w1, 2);
    const unsigned v0 = gray_v(w0, hi2, lo);
    const unsigned v1 = gray_v(p1, hi2, lo);
    const unsigned v2 = gray_v(p2, hi2, lo);
    const unsigned v3 = gray_v(w2, hi2 << 8, lo << 8);
    // v_perm_b32(hi, lo, sel): byte k of the result = byte sel[k] of {hi:lo} (0..3 = lo, 4..7 = hi)
    const unsigned g01 = __builtin_amdgcn_perm(v1, v0, 0x0c0c0501u);     // [v0.b1, v1.b1, 0, 0]
    const unsigned g23 = __builtin_amdgcn_perm(v3, v2, 0x05010c0cu);     // [0, 0, v2.b1, v3.b1]
    return g01 | g23;
}

template <bool RGB>
__device__ __forceinline__ unsigned gray1(const uint8_t* p)
{
    return (p[RGB ? 2 : 0] * 3735u + p[1] * 19235u + p[RGB ? 0 : 2] * 9798u + (1u << 14)) >> 15;
}

// four pixels of one dword each (channel c in byte c; byte 3 anything: its coefficient is zero) -> 4 gray bytes.  No alignbyte: the pixels
// arrive aligned.  8 dot4, 4 shifts, 2 perm, 1 or = 15 vector instructions per 4 pixels (gray4: 17).
template <bool RGB>
__device__ __forceinline__ unsigned gray4_px(unsigned p0, unsigned p1, unsigned p2, unsigned p3)
{
    constexpr unsigned hi2 = hi2_of<RGB>(), lo = lo_of<RGB>();
    const unsigned v0 = gray_v(p0, hi2, lo);
    const unsigned v1 = gray_v(p1, hi2, lo);
    const unsigned v2 = gray_v(p2, hi2, lo);
    const unsigned v3 = gray_v(p3, hi2, lo);
    const unsigned g01 = __builtin_amdgcn_perm(v1, v0, 0x0c0c0501u);     // [v0.b1, v1.b1, 0, 0]
    const unsigned g23 = __builtin_amdgcn_perm(v3, v2, 0x05010c0cu);     // [0, 0, v2.b1, v3.b1]
    return g01 | g23;
}

// 4 R, 4 G and 4 B bytes of the same four pixels (AVD_FMT_RGBP) -> 4 gray bytes.  The byte lanes are gathered into pixel words [R, G, B, 0]
// by v_perm: two interleave R with G ([r0 g0 r1 g1], [r2 g2 r3 g3]), four put a B byte behind each pair -- 6 perm + gray4_px's 15 = 21
// vector instructions per 4 pixels.  (Per-plane byte extraction with v_mad_u32_u24 is 12 extractions + 12 multiply-adds + 4 shifts + 3 to
// pack = 31: DESIGN.md section 4.1.)
__device__ __forceinline__ unsigned gray4_planar(unsigned r, unsigned g, unsigned b)
{
    const unsigned rg01 = __builtin_amdgcn_perm(g, r, 0x05010400u);      // [r0, g0, r1, g1]
    const unsigned rg23 = __builtin_amdgcn_perm(g, r, 0x07030602u);      // [r2, g2, r3, g3]
    const unsigned p0 = __builtin_amdgcn_perm(b, rg01, 0x0c040100u);     // [r0, g0, b0, 0]
    const unsigned p1 = __builtin_amdgcn_perm(b, rg01, 0x0c050302u);     // [r1, g1, b1, 0]
    const unsigned p2 = __builtin_amdgcn_perm(b, rg23, 0x0c060100u);
    const unsigned p3 = __builtin_amdgcn_perm(b, rg23, 0x0c070302u);
    return gray4_px<true>(p0, p1, p2, p3);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// The band a workgroup owns.  blockIdx -> lid = (frame, band): logical ids that are consecutive share blockIdx % 8, i.e. an XCD.
// of: the frame of the per-frame outputs (the 320-px image) the band writes -- f itself, except in a grouped launch (OutFrames below), whose
// frames come from several clips; the row and Laplacian partials stay at f (lid), which only the launch's own k_hash reads
struct Band { int lid, f, band, r0, rows, trows, of; };      // rows [r0, r0 + rows) of frame f; tile row 0 = image row r0 - 1, trows = rows + 2

// (no branch in here: the caller's early return then leaves the compiler free to sink the division under the first loads)
__device__ __forceinline__ bool decode_band(const PreParams& P, int n, Band& b)      // false: idle tail block, b unusable
{
    const int total = n * P.nbands;
    const int per = (total + 7) >> 3;
    b.lid = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    b.f = b.lid / P.nbands;
    b.band = b.lid - b.f * P.nbands;
    b.r0 = b.band * P.rows_per_band;
    b.rows = min(P.rows_per_band, P.h - b.r0);
    b.trows = b.rows + 2;
    return b.lid < total;
}

// Where the planes of frame f start.  strided: at a fixed distance from frame 0's.  listed: where a device table of plane pointers says
// (avd_frame_list) -- the kernel's plane argument then IS that table, entry f of it the plane of frame f, and the frame stride is unused.  f is
// uniform over the workgroup and nothing the kernel stores aliases the table, so the base arrives by one scalar load per plane and workgroup,
// ahead of the fill.  The entry is read as a pointer into GLOBAL memory (address space 1; what a kernel argument is known to be and a pointer
// that comes out of memory is not): the fills below then issue the same global_load instructions as in the strided kernels -- a generic pointer
// would make them flat loads, which also count against lgkmcnt beside the LDS traffic of the tile.
// A template parameter of the kernels: the strided instantiations contain no trace of the table.
enum class Frames { strided, listed };
using GlobalPlane = const __attribute__((address_space(1))) uint8_t*;
template <Frames FR>
__device__ __forceinline__ const uint8_t* frame_base(const uint8_t* plane, int f, int64_t frame_stride)
{
    if constexpr (FR == Frames::listed) return (const uint8_t*)reinterpret_cast<const GlobalPlane*>(plane)[f];
    else return plane + (int64_t)f * frame_stride;
}

// The output frame of frame f of a launch.  strided: f, at compile time -- the argument is an empty struct and the strided instantiations contain
// no trace of it.  listed: entry f of a device table (a grouped launch, option "ingest_group": the frames of several clips, whose places in the
// per-frame buffers are not one run), or f where the table is null (a plain list).  f is uniform over the workgroup: like the plane pointers,
// the entry arrives by one scalar load per workgroup.
using GlobalInts = const __attribute__((address_space(1))) int*;
template <Frames FR> struct OutFrames;
template <> struct OutFrames<Frames::strided> {
    __device__ __forceinline__ int at(int f) const { return f; }
};
template <> struct OutFrames<Frames::listed> {
    const int* tab;
    __device__ __forceinline__ int at(int f) const { return tab ? ((GlobalInts)tab)[f] : f; }
};

__device__ __forceinline__ int reflect_once(int p, int len)      // valid for -len < p < 2*len-1
{
    p = p < 0 ? -p : p;
    return p >= len ? 2 * len - 2 - p : p;
}

// 16 BGR or RGB pixels (three 16-byte words) -> 16 gray bytes
template <bool RGB>
__device__ __forceinline__ uint4 gray16(const uint4& a, const uint4& b, const uint4& d)
{
    uint4 g;
    g.x = gray4<RGB>(a.x, a.y, a.z);
    g.y = gray4<RGB>(a.w, b.x, b.y);
    g.z = gray4<RGB>(b.z, b.w, d.x);
    g.w = gray4<RGB>(d.y, d.z, d.w);
    return g;
}

struct Moments { long long s, q; };

// The resampling tables in LDS (k_preprocess_vec; the generic kernels read them from global memory).
struct LdsTabs {
    LinTap lxt[AVD_SMALL], lyt[AVD_SMALL];
    int ax_begin[AVD_HASH], ax_count[AVD_HASH];
    float ax_first[AVD_HASH], ax_mid[AVD_HASH], ax_last[AVD_HASH];
};

__device__ __forceinline__ void fill_lds_tabs(LdsTabs* lt, const PreParams& P, int tid)
{
    const uint2* sx = reinterpret_cast<const uint2*>(P.lxt);
    const uint2* sy = reinterpret_cast<const uint2*>(P.lyt);
    for (int i = tid; i < AVD_SMALL; i += kThreads) {
        reinterpret_cast<uint2*>(lt->lxt)[i] = sx[i];
        reinterpret_cast<uint2*>(lt->lyt)[i] = sy[i];
    }
    if (tid < AVD_HASH) {
        lt->ax_begin[tid] = P.ax_begin[tid]; lt->ax_count[tid] = P.ax_count[tid];
        lt->ax_first[tid] = P.ax_first[tid]; lt->ax_mid[tid] = P.ax_mid[tid]; lt->ax_last[tid] = P.ax_last[tid];
    }
}

// Phases 2-4 of a band whose gray rows [r0-1, r0+rows] (incl. column halo) sit in `tile`:
// exact Laplacian moments, INTER_AREA horizontal partials, INTER_LINEAR 320x320 rows.
// LTAB: the resampling tables come from LDS (lt) instead of global memory: the staged kernel has its whole band's loads in
// flight and vmcnt retires in order, so it fetches the tables ahead of them (fill_lds_tabs) and issues no global load here.
template <bool LTAB>
__device__ __forceinline__ Moments band_phases(const uint8_t* tile, const LdsTabs* lt, const PreParams& P, const Band& b, int tid,
                                               uint8_t* __restrict__ small, float* __restrict__ rowbuf)
{
    const int f = b.f, band = b.band, r0 = b.r0, rows = b.rows;
    const int w = P.w, h = P.h, pitch = P.pitch;
    // ---- Laplacian moments, exact, from row-pair products -----------------------------------
    // lap(t,x) = T(t-1,x) + T(t+1,x) + T(t,x-1) + T(t,x+1) - 4 T(t,x) on the haloed tile T
    // (tile row t = 1..rows are the band's rows).  Expanding sum lap^2 gives 15 sums of byte
    // products per band row; products that involve the same two tile rows are shared between
    // neighbouring band rows, so it is enough to form, when tile row n "enters" a lane's column
    // walk, seven v_dot4_u32_u8 with the rows above it:
    //   A(n)=C.C  HR(n)=C.R  H2(n)=L.R  V1(n-1)=C'.C  V2(n-2)=C''.C  Dp(n-1)=C'.R  Dm(n-1)=C'.L
    // (C = 4 gray bytes of row n, L/R = the same shifted by -1/+1 pixel, ' = previous row).
    // Row n contributes with weights that depend only on whether n-1, n, n+1 are band rows:
    //   A: [n+1 in B] + [n-1 in B] + 18 [n in B]      V1, Dp, Dm: (-8|+2|+2) ([n in B] + [n-1 in B])
    //   HR: -16 [n in B]   H2: +2 [n in B]   V2: +2 [n-1 in B]    row sum: [n+1 in B]+[n-1 in B]-2[n in B]
    // Interior rows (2 <= n <= rows-1) have constant weights (20,-16,2,-16,2,4,4; row sum 0) and
    // accumulate in place; the <= 4 boundary rows use a multiply-add per product.  What the
    // column shifts miss at x = 0 / w-1 is added per band row as exact scalar edge terms.
    long long s_acc = 0, q_acc = 0;
    {
        const int quads = (w + 3) >> 2;
        const int trows = rows + 2;             // formed from rows here: the one-row branch below is then known to walk <= 3 rows
        const unsigned ones = 0x01010101u;
        unsigned iA = 0, iHR = 0, iH2 = 0, iV1 = 0, iV2 = 0, iDp = 0, iDm = 0;   // products with the interior weights
        int xA = 0;                                                                // A with weight 1 (signed: also corrects 20 -> 19)
        unsigned xV1 = 0, xD = 0;                                                  // V1 with weight -8, Dp + Dm with weight 2
        int bq = 0, bs = 0;                                                        // generic path (rows < 2) and row sums
        // two compiled versions: only widths that are not a multiple of 4 need the mask of the last quad
        auto walk = [&](auto ragged_tag) {
        constexpr bool ragged = decltype(ragged_tag)::value;
        for (int qx = tid; qx < quads; qx += kThreads) {
            const uint8_t* col = tile + kPad + qx * 4;
            unsigned mk = 0xFFFFFFFFu;
            if (ragged) {                                  // ragged last quad: drop pixels >= w
                const int valid = w - qx * 4;
                if (valid < 4) mk = (1u << (8 * valid)) - 1u;
            }
            auto ld = [&](int nrow, unsigned& C, unsigned& L, unsigned& R) {
                const uint8_t* cp = col + nrow * pitch;
                const unsigned Cw = *reinterpret_cast<const unsigned*>(cp);
                const unsigned Lw = *reinterpret_cast<const unsigned*>(cp - 4);
                const unsigned Rw = *reinterpret_cast<const unsigned*>(cp + 4);
                C = Cw; L = __builtin_amdgcn_alignbyte(Cw, Lw, 3); R = __builtin_amdgcn_alignbyte(Rw, Cw, 1);
                if (ragged) { C &= mk; L &= mk; R &= mk; }
            };
            unsigned C, L, R, C1, C2;
            if (rows >= 2) {
                // The four boundary rows are peeled (their weights differ from the interior ones only in a few
                // places, which go to the x* accumulators), so the interior loop is seven dot4 and no branch:
                //   row 0      : A x1, row sum +1
                //   row 1      : as interior but A x19, V1 x-8, no V2, Dp/Dm x2, row sum -1
                //   row rows   : as interior but A x19, row sum -1
                //   row rows+1 : A x1, V1 x-8, V2 x2, Dp/Dm x2, row sum +1
                ld(0, C, L, R);
                xA += (int)__builtin_amdgcn_udot4(C, C, 0u, false);
                bs += (int)__builtin_amdgcn_udot4(C, ones, 0u, false);
                C1 = C;
                ld(1, C, L, R);
                {
                    const unsigned t = __builtin_amdgcn_udot4(C, C, 0u, false);
                    iA += t; xA -= (int)t;
                    iHR = __builtin_amdgcn_udot4(C, R, iHR, false);
                    iH2 = __builtin_amdgcn_udot4(L, R, iH2, false);
                    xV1 = __builtin_amdgcn_udot4(C1, C, xV1, false);
                    xD = __builtin_amdgcn_udot4(C1, R, xD, false);
                    xD = __builtin_amdgcn_udot4(C1, L, xD, false);
                    bs -= (int)__builtin_amdgcn_udot4(C, ones, 0u, false);
                }
                C2 = C1; C1 = C;
                for (int nrow = 2; nrow <= rows - 1; nrow++) {
                    ld(nrow, C, L, R);
                    iA = __builtin_amdgcn_udot4(C, C, iA, false);
                    iHR = __builtin_amdgcn_udot4(C, R, iHR, false);
                    iH2 = __builtin_amdgcn_udot4(L, R, iH2, false);
                    iV1 = __builtin_amdgcn_udot4(C1, C, iV1, false);
                    iV2 = __builtin_amdgcn_udot4(C2, C, iV2, false);
                    iDp = __builtin_amdgcn_udot4(C1, R, iDp, false);
                    iDm = __builtin_amdgcn_udot4(C1, L, iDm, false);
                    C2 = C1; C1 = C;
                }
                ld(rows, C, L, R);
                {
                    const unsigned t = __builtin_amdgcn_udot4(C, C, 0u, false);
                    iA += t; xA -= (int)t;
                    iHR = __builtin_amdgcn_udot4(C, R, iHR, false);
                    iH2 = __builtin_amdgcn_udot4(L, R, iH2, false);
                    iV1 = __builtin_amdgcn_udot4(C1, C, iV1, false);
                    iV2 = __builtin_amdgcn_udot4(C2, C, iV2, false);
                    iDp = __builtin_amdgcn_udot4(C1, R, iDp, false);
                    iDm = __builtin_amdgcn_udot4(C1, L, iDm, false);
                    bs -= (int)__builtin_amdgcn_udot4(C, ones, 0u, false);
                }
                C2 = C1; C1 = C;
                ld(rows + 1, C, L, R);
                xA += (int)__builtin_amdgcn_udot4(C, C, 0u, false);
                xV1 = __builtin_amdgcn_udot4(C1, C, xV1, false);
                iV2 = __builtin_amdgcn_udot4(C2, C, iV2, false);
                xD = __builtin_amdgcn_udot4(C1, R, xD, false);
                xD = __builtin_amdgcn_udot4(C1, L, xD, false);
                bs += (int)__builtin_amdgcn_udot4(C, ones, 0u, false);
            } else {
                // a one-row band (last band of some geometries): every tile row is a boundary row
                C1 = 0; C2 = 0;
                for (int nrow = 0; nrow < trows; nrow++) {
                    ld(nrow, C, L, R);
                    const int in0 = nrow >= 1 && nrow <= rows;          // n   in B
                    const int inm = nrow >= 2 && nrow <= rows + 1;      // n-1 in B
                    const int inp = nrow + 1 <= rows;                   // n+1 in B  (n >= 0 always)
                    const int wA = inp + inm + 18 * in0, wP = in0 + inm;
                    bq += wA * (int)__builtin_amdgcn_udot4(C, C, 0u, false);
                    bq -= 16 * in0 * (int)__builtin_amdgcn_udot4(C, R, 0u, false);
                    bq += 2 * in0 * (int)__builtin_amdgcn_udot4(L, R, 0u, false);
                    bq -= 8 * wP * (int)__builtin_amdgcn_udot4(C1, C, 0u, false);
                    bq += 2 * inm * (int)__builtin_amdgcn_udot4(C2, C, 0u, false);
                    bq += 2 * wP * (int)__builtin_amdgcn_udot4(C1, R, 0u, false);
                    bq += 2 * wP * (int)__builtin_amdgcn_udot4(C1, L, 0u, false);
                    bs += (inp + inm - 2 * in0) * (int)__builtin_amdgcn_udot4(C, ones, 0u, false);
                    C2 = C1; C1 = C;
                }
            }
        }
        };
        if (w & 3) walk(std::true_type{}); else walk(std::false_type{});
        q_acc = 20ll * iA - 16ll * iHR + 2ll * iH2 - 16ll * iV1 + 2ll * iV2 + 4ll * iDp + 4ll * iDm
                + (long long)xA - 8ll * xV1 + 2ll * xD + bq;
        s_acc = bs;
        // edge terms of band row t (tile row t = tid + 1): the l/r shifted sums run over x-1 / x+1
        if (tid < rows) {
            const uint8_t* r = tile + (tid + 1) * pitch + kPad;
            const uint8_t* dn = r + pitch;
            const int a = r[-1], b0 = r[0], e = r[w - 1], z = r[w];      // T(t,-1), T(t,0), T(t,w-1), T(t,w)
            const int da = dn[-1], db = dn[0], de = dn[w - 1], dz = dn[w];
            s_acc += a - e - b0 + z;
            q_acc += (a * a - e * e) + (z * z - b0 * b0)                // l^2 + r^2
                     - 8 * (a * b0 - e * z)                            // m*l
                     + 2 * (a * db - e * dz)                           // d*l
                     + 2 * (z * de - b0 * da);                         // d*r
        }
    }

    // ---- INTER_AREA horizontal partials, one float chain per (row, cell), cv2's order ----
    // The chain of a cell is sequential by definition (float adds in cv2's order); a lane runs the
    // chains of two different rows interleaved so that dependent adds of one hide behind the other.
    {
        float* out = rowbuf + ((int64_t)f * h + r0) * AVD_HASH;
        const int dx = tid & 31;
        const int xb = LTAB ? lt->ax_begin[dx] : P.ax_begin[dx];
        const int cnt = LTAB ? lt->ax_count[dx] : P.ax_count[dx];
        const float wf = LTAB ? lt->ax_first[dx] : P.ax_first[dx], wm = LTAB ? lt->ax_mid[dx] : P.ax_mid[dx],
                    wl = LTAB ? lt->ax_last[dx] : P.ax_last[dx];
        constexpr int RSTEP = kThreads / AVD_HASH;             // rows covered per pass
        for (int ra = tid >> 5; ra < rows; ra += 2 * RSTEP) {
            const int rb = ra + RSTEP;
            const bool two = rb < rows;
            const uint8_t* sa = tile + (ra + 1) * pitch + kPad + xb;
            const uint8_t* sb = tile + ((two ? rb : ra) + 1) * pitch + kPad + xb;
            if (P.area_fast) {
                int a0 = 0, a1 = 0;
                for (int k = 0; k < cnt; k++) { a0 += sa[k]; a1 += sb[k]; }
                out[ra * AVD_HASH + dx] = __int_as_float(a0);
                if (two) out[rb * AVD_HASH + dx] = __int_as_float(a1);
            } else if (P.area_x_uniform4) {
                // every cell starts on a 4-byte boundary, spans a multiple of 4 pixels, one weight
                const unsigned* a4 = reinterpret_cast<const unsigned*>(sa);
                const unsigned* b4 = reinterpret_cast<const unsigned*>(sb);
                float a0 = 0.f, a1 = 0.f;
                for (int k = 0; k < (cnt >> 2); k++) {
                    const unsigned va = a4[k], vb = b4[k];
                    a0 = __fadd_rn(a0, __fmul_rn((float)(va & 0xFF), wm));
                    a1 = __fadd_rn(a1, __fmul_rn((float)(vb & 0xFF), wm));
                    a0 = __fadd_rn(a0, __fmul_rn((float)((va >> 8) & 0xFF), wm));
                    a1 = __fadd_rn(a1, __fmul_rn((float)((vb >> 8) & 0xFF), wm));
                    a0 = __fadd_rn(a0, __fmul_rn((float)((va >> 16) & 0xFF), wm));
                    a1 = __fadd_rn(a1, __fmul_rn((float)((vb >> 16) & 0xFF), wm));
                    a0 = __fadd_rn(a0, __fmul_rn((float)(va >> 24), wm));
                    a1 = __fadd_rn(a1, __fmul_rn((float)(vb >> 24), wm));
                }
                out[ra * AVD_HASH + dx] = a0;
                if (two) out[rb * AVD_HASH + dx] = a1;
            } else {
                float a0 = 0.f, a1 = 0.f;
                for (int k = 0; k < cnt; k++) {
                    const float wgt = k == 0 ? wf : (k == cnt - 1 ? wl : wm);
                    a0 = __fadd_rn(a0, __fmul_rn((float)sa[k], wgt));
                    a1 = __fadd_rn(a1, __fmul_rn((float)sb[k], wgt));
                }
                out[ra * AVD_HASH + dx] = a0;
                if (two) out[rb * AVD_HASH + dx] = a1;
            }
        }
    }

    // ---- INTER_LINEAR 320x320 rows whose upper source row lies in this band ----------------
    {
        const int d0 = P.band_dy[band], d1 = P.band_dy[band + 1];        // wave-uniform scalar loads
        uint8_t* dst = small + (int64_t)b.of * AVD_NPIX;
        // a lane owns output COLUMNS (its x taps are unpacked once); the rows of the band are walked with
        // wave-uniform y taps held in scalar registers
        for (int dx = tid; dx < AVD_SMALL; dx += kThreads) {
            const LinTap tx = LTAB ? lt->lxt[dx] : P.lxt[dx];
            const int x0 = tx.i0, x1 = tx.i1, wx0 = tx.w0, wx1 = tx.w1;
            for (int dy = d0; dy < d1; dy++) {
                const uint2 tyw = *reinterpret_cast<const uint2*>(LTAB ? &lt->lyt[dy] : &P.lyt[dy]);
                const unsigned ta = __builtin_amdgcn_readfirstlane(tyw.x), tb = __builtin_amdgcn_readfirstlane(tyw.y);
                const int yi0 = (short)(ta & 0xffffu), yi1 = (short)(ta >> 16);
                const int wy0 = (short)(tb & 0xffffu), wy1 = (short)(tb >> 16);
                const uint8_t* ra = tile + (yi0 - r0 + 1) * pitch + kPad;
                const uint8_t* rb = tile + (yi1 - r0 + 1) * pitch + kPad;
                const int ha = ra[x0] * wx0 + ra[x1] * wx1;
                const int hb = rb[x0] * wx0 + rb[x1] * wx1;
                dst[dy * AVD_SMALL + dx] = (uint8_t)((((wy0 * (ha >> 4)) >> 16) + ((wy1 * (hb >> 4)) >> 16) + 2) >> 2);
            }
        }
    }
    return Moments{s_acc, q_acc};
}

// per-wave partial moments, summed per frame in k_hash (atomics on the 16 B/frame accumulators
// serialise in L2: 65 k same-line atomics cost ~50 us per launch)
__device__ __forceinline__ void store_moments(long long* __restrict__ lap_part, int lid, int tid, const Moments& m)
{
    const long long s64 = wave_sum(m.s), q64 = wave_sum(m.q);
    if ((tid & 63) == 0) {
        long long* slot = lap_part + ((int64_t)lid * kLapSlots + (tid >> 6)) * 2;
        slot[0] = s64; slot[1] = q64;
    }
}

// column halo (BORDER_REFLECT_101) of a filled tile: pixel -1 := pixel 1, pixel w := pixel w-2
__device__ __forceinline__ void fill_column_halo(uint8_t* tile, int trows, int pitch, int w, int tid)
{
    __syncthreads();
    for (int tr = tid; tr < trows; tr += kThreads) {
        uint8_t* row = tile + tr * pitch + kPad;
        row[-1] = row[reflect101(-1, w)];
        row[w] = row[reflect101(w, w)];
    }
    __syncthreads();
}

// ---- the fills: gray rows [r0-1, r0+rows] of the band into the tile.  They are all the kernels differ in. ----
// The packed and the planar RGB layouts share three loops; a layout (the policies further down) hands a loop the callable that fetches and
// converts, the way the 4:2:0 fills take their chroma callable.  `row` is the byte offset of the (reflected) image row in a plane.

// any geometry / alignment: one byte-wise pixel per work item.  gray(row, x): the gray value of pixel x of that row
template <typename Gray>
__device__ __forceinline__ void fill_scalar(uint8_t* tile, const PreParams& P, const Band& b, int tid, Gray gray)
{
    const int w = P.w, pitch = P.pitch;
    for (int it = tid; it < b.trows * w; it += kThreads) {
        const int tr = it / w, x = it - tr * w;
        const int y = reflect_once(b.r0 - 1 + tr, P.h);
        tile[tr * pitch + kPad + x] = (uint8_t)gray((int64_t)y * P.row_stride, x);
    }
}

// 16-byte aligned rows of w % 16 == 0 pixels: one 16-pixel chunk per work item.  gray16_of(row, c): the 16 gray bytes of chunk c of that row
template <typename Gray16>
__device__ __forceinline__ void fill_vec16(uint8_t* tile, const PreParams& P, const Band& b, int tid, Gray16 gray16_of)
{
    const int chunks = P.w >> 4, pitch = P.pitch;
    for (int it = tid; it < b.trows * chunks; it += kThreads) {
        const int tr = it / chunks, c = it - tr * chunks;
        const int y = reflect_once(b.r0 - 1 + tr, P.h);
        *reinterpret_cast<uint4*>(tile + tr * pitch + kPad + c * 16) = gray16_of((int64_t)y * P.row_stride, c);
    }
}

// register-staged (w % 16 == 0, <= 16 * kThreads px): every lane owns one 16-pixel column chunk c and issues ALL its NI row loads (loader(c)
// gives the lane's load(row, q): three 16-byte words each) before the first conversion (convert(q): their 16 gray bytes), so a workgroup has
// its whole band in flight at once; conversions start as the words arrive (vmcnt counts down in issue order).  The lanes that convert the first / last chunk also write
// the reflected column halo bytes, which saves a barrier.
template <int NI, typename Loader, typename Convert>
__device__ __forceinline__ void fill_staged(uint8_t* tile, const PreParams& P, const Band& b, int tid, Loader loader, Convert convert)
{
    const int pitch = P.pitch;
    const int chunks = P.w >> 4;
    const int rpp = kThreads / chunks;               // tile rows covered per pass of the workgroup
    const int rsub = tid / chunks, c = tid - rsub * chunks;
    if (rsub < rpp) {
        const auto load = loader(c);
        uint4 q[NI][3];
#pragma unroll
        for (int k = 0; k < NI; k++) {
            const int t = min(rsub + k * rpp, b.trows - 1);  // surplus items re-read the last row (same bytes)
            const int y = reflect_once(b.r0 - 1 + t, P.h);
            load((int64_t)y * P.row_stride, q[k]);
        }
        uint8_t* dst = tile + kPad + c * 16;
#pragma unroll
        for (int k = 0; k < NI; k++) {
            const int t = min(rsub + k * rpp, b.trows - 1);
            const uint4 g = convert(q[k]);
            uint8_t* d = dst + t * pitch;
            *reinterpret_cast<uint4*>(d) = g;
            if (c == 0) d[-1] = (uint8_t)(g.x >> 8);                 // pixel -1 := pixel 1
            if (c == chunks - 1) d[16] = (uint8_t)(g.w >> 16);       // pixel w  := pixel w-2
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// NV12 ingest: the decoder's surface goes straight into the fused pass.  Per pixel the BGR triple
// that cv2.VideoCapture.retrieve() would have produced (libswscale's table-driven yuv2rgb.c, BT.601 limited range,
// nearest chroma; reference app/analyzers/video.py:28-32) is formed in registers, reduced to cv2's 15-bit gray at
// once and written to the LDS tile: neither BGR nor gray ever reaches HBM, and the frame costs 1.5 bytes per pixel
// of HBM reads instead of 3.  Phases 2-4 are the BGR kernel's.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// chroma part of the three table lookups of one U,V pair: c0 + off * cy per channel
struct ChromaTerms { int r, g, b; };
// every product below has operands inside 24 bits (8-bit samples, 17-bit coefficients of either range -- the largest is cbu = 132201 limited,
// 116129 full, both below 2^17 --, table indices of a few hundred):
// __mul24 / __umul24 are full-rate instructions where a 32-bit multiply is quarter rate
__device__ __forceinline__ ChromaTerms chroma_terms(int U, int V, const YuvConsts& k)
{
    ChromaTerms t;
    t.r = k.c0 + __mul24((__mul24(V, k.crv) >> 16) + k.kr, k.cy);
    t.b = k.c0 + __mul24((__mul24(U, k.cbu) >> 16) + k.kb, k.cy);
    t.g = k.c0 + __mul24((__mul24(U, k.cgu) >> 16) + (__mul24(V, k.cgv) >> 16) + k.kg, k.cy);
    return t;
}

// the table form: the three indices' chroma parts (libswscale's per-U / per-V table offsets), biased so that Y + offset >= 0
__device__ __forceinline__ ChromaTerms chroma_offsets(int U, int V, const YuvConsts& k)
{
    ChromaTerms t;
    t.r = (__mul24(V, k.crv) >> 16) + (k.kr + k.bias);       // the sums in parentheses are uniform: one scalar add per launch, as with a literal bias
    t.b = (__mul24(U, k.cbu) >> 16) + (k.kb + k.bias);
    t.g = (__mul24(U, k.cgu) >> 16) + (__mul24(V, k.cgv) >> 16) + (k.kg + k.bias);
    return t;
}

// the eight chroma-offset triples of a 16-pixel chunk.  Interleaved (NV12, NV16): one 16-byte word, pair j = bytes 2j (U) and 2j + 1 (V)
__device__ __forceinline__ void chroma8_interleaved(const uint4& cc, const YuvConsts& k, ChromaTerms (&t)[8])
{
    const unsigned cw[4] = {cc.x, cc.y, cc.z, cc.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        t[2 * j] = chroma_offsets(cw[j] & 0xFF, (cw[j] >> 8) & 0xFF, k);
        t[2 * j + 1] = chroma_offsets((cw[j] >> 16) & 0xFF, cw[j] >> 24, k);
    }
}
// planar (I420, I422): 8 U and 8 V bytes, pair j = U byte j and V byte j
__device__ __forceinline__ void chroma8_planar(const uint2& uu, const uint2& vv, const YuvConsts& k, ChromaTerms (&t)[8])
{
    const unsigned uw[2] = {uu.x, uu.y}, vw[2] = {vv.x, vv.y};
#pragma unroll
    for (int j = 0; j < 8; j++)
        t[j] = chroma_offsets((uw[j >> 2] >> (8 * (j & 3))) & 0xFF, (vw[j >> 2] >> (8 * (j & 3))) & 0xFF, k);
}

__device__ __forceinline__ unsigned gray_from_tables(int Y, const ChromaTerms& t, const unsigned* tabB, const unsigned* tabG, const unsigned* tabR)
{
    return (tabB[Y + t.b] + tabG[Y + t.g] + tabR[Y + t.r]) >> 15;
}

__device__ __forceinline__ unsigned gray_from_yuv(int Y, const ChromaTerms& t, int cy)
{
    // Y * cy + term: one v_mad_i32_i24 per channel
    const unsigned B = (unsigned)clip8((__mul24(Y, cy) + t.b) >> 16), G = (unsigned)clip8((__mul24(Y, cy) + t.g) >> 16),
                   R = (unsigned)clip8((__mul24(Y, cy) + t.r) >> 16);
    return (__umul24(B, 3735u) + __umul24(G, 19235u) + __umul24(R, 9798u) + (1u << 14)) >> 15;
}

// 4 luma bytes + 2 chroma pairs (U0 V0 U1 V1) -> 4 gray bytes
__device__ __forceinline__ unsigned gray4_nv12(unsigned yw, unsigned cw, const YuvConsts& k)
{
    const ChromaTerms t0 = chroma_terms(cw & 0xFF, (cw >> 8) & 0xFF, k);
    const ChromaTerms t1 = chroma_terms((cw >> 16) & 0xFF, cw >> 24, k);
    return gray_from_yuv(yw & 0xFF, t0, k.cy) | (gray_from_yuv((yw >> 8) & 0xFF, t0, k.cy) << 8) |
           (gray_from_yuv((yw >> 16) & 0xFF, t1, k.cy) << 16) | (gray_from_yuv(yw >> 24, t1, k.cy) << 24);
}

// 4:2:0, any geometry / alignment: one pixel per work item.  Luma::at(row, x) fetches the pixel's luma sample from its stored row, chroma(y >> 1, x >> 1, U, V) its
// chroma sample (8-bit values: a 16-bit layout narrows them): the surface kinds differ in nothing else.  FLIP: the stored picture is the displayed one turned by 180 degrees -- displayed (y, x) is stored
// (h - 1 - y, w - 1 - x), and with even h and w its chroma sample is the mirrored one.
template <bool FLIP, typename Luma, typename ChromaAt>
__device__ __forceinline__ void fill_yuv420_scalar(uint8_t* tile, const uint8_t* yfr, const YuvConsts& k, const PreParams& P, const Band& b, int tid,
                                                   ChromaAt chroma)
{
    const int w = P.w, pitch = P.pitch;
    for (int it = tid; it < b.trows * w; it += kThreads) {
        const int tr = it / w, x = it - tr * w;
        const int y = reflect_once(b.r0 - 1 + tr, P.h);
        const int sy = FLIP ? P.h - 1 - y : y, sx = FLIP ? w - 1 - x : x;
        int U, V;
        chroma(sy >> 1, sx >> 1, U, V);
        const ChromaTerms t = chroma_terms(U, V, k);
        tile[tr * pitch + kPad + x] = (uint8_t)gray_from_yuv(Luma::at(yfr + (int64_t)sy * P.row_stride, sx), t, k.cy);
    }
}

// BORDER_REFLECT_101 rows of a tile whose image rows are filled (and a barrier passed): image row -1 (tile row 0, if `top`) is row 1, image row h (the last tile row,
// if `bottom`) is row h - 2 -- both already in the tile.  Copied as `words` 16-byte words per row.
__device__ __forceinline__ void reflect_tile_rows(uint8_t* tile, int trows, int pitch, int words, bool top, bool bottom, int tid)
{
    if (top)
        for (int c = tid; c < words; c += kThreads)
            *reinterpret_cast<uint4*>(tile + kPad + c * 16) = *reinterpret_cast<const uint4*>(tile + 2 * pitch + kPad + c * 16);
    if (bottom)
        for (int c = tid; c < words; c += kThreads)
            *reinterpret_cast<uint4*>(tile + (trows - 1) * pitch + kPad + c * 16) =
                *reinterpret_cast<const uint4*>(tile + (trows - 3) * pitch + kPad + c * 16);
}

// the three gray tables behind a tile of trows rows (B, G, R: k.ntab entries each); returns the first
__device__ __forceinline__ unsigned* build_gray_tables(uint8_t* tile, int trows, int pitch, const YuvConsts& k, int tid)
{
    unsigned* const tabB = reinterpret_cast<unsigned*>(tile + lds_nvtab_off(trows, pitch));
    unsigned* const tabG = tabB + k.ntab;
    unsigned* const tabR = tabG + k.ntab;
    for (int i = tid; i < k.ntab; i += kThreads) {
        const unsigned v = (unsigned)clip8((k.c0 + (i - k.bias) * k.cy) >> 16);
        tabB[i] = v * 3735u; tabG[i] = v * 19235u + (1u << 14); tabR[i] = v * 9798u;
    }
    __syncthreads();
    return tabB;
}

// NV12, 16-byte aligned planes of w % 16 == 0 pixels.
// libswscale's converter IS a table lookup: B = T[Y + ob(U)], G = T[Y + og(U, V)], R = T[Y + or(V)] with one clip table T(i) = clip8((c0 + i cy) >> 16).
// Three LDS tables of cv2's gray weight times T (3735 T, 19235 T + the rounding 2^14, 9798 T; 32-bit entries, index bias k.bias), so a pixel is
// three index additions, three ds_read_b32, one three-operand add and a shift -- instead of three multiply-adds, three shifts, three clamps and
// three multiply-adds (12.3 -> 8.8 vector instructions per pixel; the LDS pipe does the lookups beside them).  Same integers by construction.
// Luma::chunk(row, c): the 16 luma bytes of 16-pixel chunk c of a stored row; chroma8(p, c, t) forms the eight chroma-term triples of chroma row p, chunk c:
// the surface kinds differ in nothing else.
// FLIP (half turn): the work item of displayed chroma row p, chunk c reads the MIRRORED stored chunk -- chroma row h/2 - 1 - p, chunk
// chunks - 1 - c, luma rows h - 1 - y -- with the same 16-byte loads, and reverses the bytes in registers: displayed byte i of the chunk is
// stored byte 15 - i, whose chroma pair is 7 - (i >> 1).
template <bool FLIP, typename Luma, typename Chroma8>
__device__ __forceinline__ void fill_yuv420_tables(uint8_t* tile, const uint8_t* yfr, const YuvConsts& k, const PreParams& P, const Band& b, int tid,
                                                   Chroma8 chroma8)
{
    const int h = P.h, pitch = P.pitch, r0 = b.r0, rows = b.rows, trows = b.trows;
    unsigned* const tabB = build_gray_tables(tile, trows, pitch, k, tid);
    unsigned* const tabG = tabB + k.ntab;
    unsigned* const tabR = tabG + k.ntab;
    // one work item = one chroma row x one 16-pixel chunk: the eight chroma-term triples are formed once and serve the
    // two luma rows that share them (they are 8.5 of the ~27 integer operations a pixel costs otherwise)
    const int ylo = r0 - 1, yhi = r0 + rows;              // image rows of tile rows 0 and trows - 1, before reflection
    const int ya = max(ylo, 0), yb = min(yhi, h - 1);      // the ones that exist
    const int p0 = ya >> 1, np = (yb >> 1) - p0 + 1;
    const int chunks = P.w >> 4;
    for (int it = tid; it < np * chunks; it += kThreads) {
        const int pr = it / chunks, c = it - pr * chunks, p = p0 + pr;
        const int cs = FLIP ? chunks - 1 - c : c;            // the stored chunk
        ChromaTerms ts[8];
        chroma8(FLIP ? (h >> 1) - 1 - p : p, cs, ts);
        const auto t = [&](int j) -> const ChromaTerms& { return ts[FLIP ? 7 - j : j]; };      // pair j of the displayed chunk
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++) {
            const int y = 2 * p + s2;
            if (y < ya || y > yb) continue;
            const uint4 yy = Luma::chunk(yfr + (int64_t)(FLIP ? h - 1 - y : y) * P.row_stride, cs);
            unsigned yw[4] = {yy.x, yy.y, yy.z, yy.w};
            if (FLIP) {
                yw[0] = __builtin_bswap32(yy.w); yw[1] = __builtin_bswap32(yy.z); yw[2] = __builtin_bswap32(yy.y); yw[3] = __builtin_bswap32(yy.x);
            }
            unsigned g[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                g[j] = gray_from_tables(yw[j] & 0xFF, t(2 * j), tabB, tabG, tabR) | (gray_from_tables((yw[j] >> 8) & 0xFF, t(2 * j), tabB, tabG, tabR) << 8) |
                       (gray_from_tables((yw[j] >> 16) & 0xFF, t(2 * j + 1), tabB, tabG, tabR) << 16) | (gray_from_tables(yw[j] >> 24, t(2 * j + 1), tabB, tabG, tabR) << 24);
            *reinterpret_cast<uint4*>(tile + (y - ylo) * pitch + kPad + c * 16) = make_uint4(g[0], g[1], g[2], g[3]);
        }
    }
    __syncthreads();
    reflect_tile_rows(tile, trows, pitch, chunks, ylo < 0, yhi > h - 1, tid);
}

// ---- 4:2:2: chroma subsampled horizontally only.  Pixel (y, x) takes the chroma sample (y, x >> 1) of its own row, so the work item of the
// 4:2:0 fills -- one chroma row serving two luma rows -- does not exist here: a work item is one luma row, the height may be odd, a band may
// begin and end on any row, and no chroma row is ever shared between workgroups.  The arithmetic per pixel is the 4:2:0 fills'.

// any geometry / alignment: one pixel per work item.  fetch(y, x, Y, U, V): the samples of stored pixel (y, x)
template <typename Fetch>
__device__ __forceinline__ void fill_yuv422_scalar(uint8_t* tile, const YuvConsts& k, const PreParams& P, const Band& b, int tid, Fetch fetch)
{
    const int w = P.w, pitch = P.pitch;
    for (int it = tid; it < b.trows * w; it += kThreads) {
        const int tr = it / w, x = it - tr * w;
        const int y = reflect_once(b.r0 - 1 + tr, P.h);
        int Y, U, V;
        fetch(y, x, Y, U, V);
        tile[tr * pitch + kPad + x] = (uint8_t)gray_from_yuv(Y, chroma_terms(U, V, k), k.cy);
    }
}

// aligned planes of w % 16 == 0 pixels: one work item = one luma row x one 16-pixel chunk, through the three gray tables of the 4:2:0 table
// fill.  chunk16(y, c, yy, t): the 16 luma bytes of chunk c of row y and its eight chroma-offset triples (pair j serves pixels 2j, 2j + 1).
// The offsets are formed per row, not per two rows: about 50 vector instructions more per 16-pixel row than fill_yuv420_tables.
template <typename Chunk16>
__device__ __forceinline__ void fill_yuv422_tables(uint8_t* tile, const YuvConsts& k, const PreParams& P, const Band& b, int tid, Chunk16 chunk16)
{
    const int h = P.h, pitch = P.pitch, trows = b.trows;
    unsigned* const tabB = build_gray_tables(tile, trows, pitch, k, tid);
    unsigned* const tabG = tabB + k.ntab;
    unsigned* const tabR = tabG + k.ntab;
    const int ylo = b.r0 - 1, yhi = b.r0 + b.rows;        // image rows of tile rows 0 and trows - 1, before reflection
    const int ya = max(ylo, 0), yb = min(yhi, h - 1);      // the ones that exist
    const int chunks = P.w >> 4;
    for (int it = tid; it < (yb - ya + 1) * chunks; it += kThreads) {
        const int yr = it / chunks, c = it - yr * chunks, y = ya + yr;
        uint4 yy;
        ChromaTerms t[8];
        chunk16(y, c, yy, t);
        const unsigned yw[4] = {yy.x, yy.y, yy.z, yy.w};
        unsigned g[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            g[j] = gray_from_tables(yw[j] & 0xFF, t[2 * j], tabB, tabG, tabR) | (gray_from_tables((yw[j] >> 8) & 0xFF, t[2 * j], tabB, tabG, tabR) << 8) |
                   (gray_from_tables((yw[j] >> 16) & 0xFF, t[2 * j + 1], tabB, tabG, tabR) << 16) | (gray_from_tables(yw[j] >> 24, t[2 * j + 1], tabB, tabG, tabR) << 24);
        *reinterpret_cast<uint4*>(tile + (y - ylo) * pitch + kPad + c * 16) = make_uint4(g[0], g[1], g[2], g[3]);
    }
    __syncthreads();
    reflect_tile_rows(tile, trows, pitch, chunks, ylo < 0, yhi > h - 1, tid);
}

// ---- quarter turns: the strip fills ----------------------------------------------------------------------------------------------------
// The stored picture S (Hs = P.w rows of Ws = P.h columns) is the displayed one D turned by a quarter: ROT = 1  D[r][c] = S[Hs-1-c][r],
// ROT = 3  D[r][c] = S[c][Ws-1-r].  A band's tile rows are therefore stored COLUMNS: of every stored row the band needs one span of at most
// kBandCap + 2 = 16 contiguous luma bytes (the displayed rows [r0-1, r0+rows] that exist) and the chroma samples under them.  One work item =
// one stored row = one displayed column: it loads the span, forms the chroma terms once per chroma sample (a sample serves the two adjacent
// luma columns of the span), converts through the gray tables and writes one byte into every tile row; the lanes of a wave hold consecutive
// displayed columns, so these are consecutive LDS bytes.  The span starts at stored column r0 - 1 (or ends there), so it has no alignment to
// speak of: the loads are 4-byte copies the compiler may issue at any address (the target guarantees unaligned access to global memory) and
// single bytes for what is left, never a byte outside the span -- one fill serves every geometry, base address and stride.

// the first `len` (<= 4 * NW) bytes at p, little-endian into NW words; the rest of the words is zero
template <int NW>
__device__ __forceinline__ void load_span(const uint8_t* p, int len, unsigned (&wd)[NW])
{
#pragma unroll
    for (int k = 0; k < NW; k++) {
        unsigned v = 0;
        if (4 * k + 4 <= len) __builtin_memcpy(&v, p + 4 * k, 4);
        else {
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (4 * k + j < len) v |= (unsigned)p[4 * k + j] << (8 * j);
        }
        wd[k] = v;
    }
}

// the same for the 16-bit layouts, whose spans are twice as long: a span of at least 16 * FULL bytes -- the common case, every band but a clip's
// first and last has all 16 rows -- takes them as FULL 16-byte copies (the address is only 2-byte aligned: unaligned global access again) and
// load_span's pieces for what is left; `full` is uniform over the workgroup
template <int FULL, int NW>
__device__ __forceinline__ void load_span_wide(const uint8_t* p, int len, unsigned (&wd)[NW])
{
    static_assert(4 * FULL <= NW, "the 16-byte copies fit the words");
    if (len >= 16 * FULL) {
        __builtin_memcpy(&wd[0], p, 16 * FULL);
        if constexpr (NW > 4 * FULL) {
            unsigned rest[NW - 4 * FULL];
            load_span(p + 16 * FULL, len - 16 * FULL, rest);
#pragma unroll
            for (int k = 0; k < NW - 4 * FULL; k++) wd[4 * FULL + k] = rest[k];
        }
    } else load_span(p, len, wd);
}

__device__ __forceinline__ unsigned span_byte(const unsigned* wd, int i) { return (wd[i >> 2] >> (8 * (i & 3))) & 0xFF; }

constexpr int kStripSpan = kBandCap + 2;               // luma bytes of a span at most
constexpr int kStripChroma = kStripSpan / 2 + 1;       // chroma samples under them at most (a span that starts on an odd column)
static_assert(kStripSpan == 16, "load_span<4> holds the luma span");

// Luma::span(row, s0, len, yw): the `len` luma bytes from column s0 of a stored row, little-endian into four words; chroma9(cy, q0, nq, t): the
// chroma-term triples of samples [q0, q0 + nq) of stored chroma row cy.  The surface kinds differ in nothing else.
template <int ROT, typename Luma, typename Chroma9>
__device__ __forceinline__ void fill_yuv420_strip(uint8_t* tile, const uint8_t* yfr, const YuvConsts& k, const PreParams& P, const Band& b, int tid,
                                                  Chroma9 chroma9)
{
    static_assert(ROT == 1 || ROT == 3, "quarter turns");
    const int h = P.h, w = P.w, pitch = P.pitch, trows = b.trows;
    const unsigned* const tabB = build_gray_tables(tile, trows, pitch, k, tid);
    const unsigned* const tabG = tabB + k.ntab;
    const unsigned* const tabR = tabG + k.ntab;
    const int ylo = b.r0 - 1, yhi = b.r0 + b.rows;           // displayed rows of tile rows 0 and trows - 1, before reflection
    const int ya = max(ylo, 0), yb = min(yhi, h - 1);         // the ones that exist
    const int len = yb - ya + 1;                              // <= kStripSpan
    const int s0 = ROT == 1 ? ya : h - 1 - yb;                // first stored column of the span
    const int odd = s0 & 1;                                   // the span's first byte is the SECOND luma column of its chroma sample
    const int q0 = s0 >> 1, nq = ((s0 + len - 1) >> 1) - q0 + 1;
    // span byte i is displayed row ya + i (ROT 1) or yb - i (ROT 3)
    uint8_t* const dst0 = tile + kPad + (ROT == 1 ? ya - ylo : yb - ylo) * pitch;
    const int dstep = ROT == 1 ? pitch : -pitch;
    auto walk = [&](auto odd_tag) {
        constexpr int ODD = decltype(odd_tag)::value;
        for (int c = tid; c < w; c += kThreads) {
            const int sr = ROT == 1 ? w - 1 - c : c;          // the stored row of displayed column c
            unsigned yw[4];
            Luma::span(yfr + (int64_t)sr * P.row_stride, s0, len, yw);
            ChromaTerms t[kStripChroma];
            chroma9(sr >> 1, q0, nq, t);
            uint8_t* d = dst0 + c;
#pragma unroll
            for (int i = 0; i < kStripSpan; i++) {
                if (i < len) *d = (uint8_t)gray_from_tables(span_byte(yw, i), t[(i + ODD) >> 1], tabB, tabG, tabR);
                d += dstep;
            }
        }
    };
    if (odd) walk(std::integral_constant<int, 1>{}); else walk(std::integral_constant<int, 0>{});
    __syncthreads();
    reflect_tile_rows(tile, trows, pitch, (w + 15) >> 4, ylo < 0, yhi > h - 1, tid);      // the last word may end in the tile row's padding
}

// ---- luma of the 4:2:0 fills: 8-bit planes (NV12, I420) load it as it lies ----
struct Luma8 {
    static __device__ __forceinline__ int at(const uint8_t* row, int x) { return row[x]; }
    static __device__ __forceinline__ uint4 chunk(const uint8_t* row, int c) { return *reinterpret_cast<const uint4*>(row + c * 16); }
    static __device__ __forceinline__ void span(const uint8_t* row, int s0, int len, unsigned (&yw)[4]) { load_span<4>(row + s0, len, yw); }
};

// ---- 16-bit samples (little-endian words).  HIGH: the 10 bits sit in the high bits (AVD_FMT_P010; P016 reads the same way), else in the low
// bits (AVD_FMT_I010).  Every word s narrows to s8 = min(255, (s + 128) >> 8) resp. min(255, (s + 2) >> 2) -- total over all 65536 words --
// and from there on the picture is the 8-bit one: the words below are exactly what the 8-bit fills hold after their loads.
template <bool HIGH>
__device__ __forceinline__ int narrow1(unsigned s)          // s: one word, 0 .. 65535
{
    return (int)(HIGH ? min(255u, (s + 128u) >> 8) : min(255u, (s + 2u) >> 2));
}
__device__ __forceinline__ unsigned load_u16(const uint8_t* p) { return *reinterpret_cast<const uint16_t*>(p); }      // planes and strides are 2-byte aligned (check_clip)

// two words in the 16-bit lanes of a dword, narrowed in place.  HIGH: one saturating packed add (v_pk_add_u16 clamp: a word from 0xFF80 up stays
// 0xFFFF, so the min is free), s8 is the lane's HIGH byte; else a saturating packed add, a packed shift and a packed min, s8 is the lane's LOW byte
using u16x2 = unsigned short __attribute__((ext_vector_type(2)));
template <bool HIGH>
__device__ __forceinline__ unsigned narrow_pk(unsigned w)
{
    u16x2 v = __builtin_bit_cast(u16x2, w);
    if (HIGH) v = __builtin_elementwise_add_sat(v, (u16x2)(128));
    else v = __builtin_elementwise_min(__builtin_elementwise_add_sat(v, (u16x2)(2)) >> (u16x2)(2), (u16x2)(255));
    return __builtin_bit_cast(unsigned, v);
}
template <bool HIGH> __device__ __forceinline__ unsigned pk_lo(unsigned pk) { return HIGH ? (pk >> 8) & 0xFF : pk & 0xFF; }      // s8 of the first word
template <bool HIGH> __device__ __forceinline__ unsigned pk_hi(unsigned pk) { return HIGH ? pk >> 24 : (pk >> 16) & 0xFF; }       // of the second
// four words (two dwords) -> their four s8 bytes, in order: one v_perm picks them
template <bool HIGH>
__device__ __forceinline__ unsigned narrow4(unsigned a, unsigned b)
{
    return __builtin_amdgcn_perm(narrow_pk<HIGH>(b), narrow_pk<HIGH>(a), HIGH ? 0x07050301u : 0x06040200u);
}
template <bool HIGH> __device__ __forceinline__ uint2 narrow8(const uint4& a) { return make_uint2(narrow4<HIGH>(a.x, a.y), narrow4<HIGH>(a.z, a.w)); }
// sixteen words at p (two 16-byte loads) -> their 16 s8 bytes
template <bool HIGH>
__device__ __forceinline__ uint4 load_narrow16(const uint8_t* p)
{
    const uint4* src = reinterpret_cast<const uint4*>(p);
    const uint2 lo = narrow8<HIGH>(src[0]), hi = narrow8<HIGH>(src[1]);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

template <bool HIGH>
struct Luma16 {
    static __device__ __forceinline__ int at(const uint8_t* row, int x) { return narrow1<HIGH>(load_u16(row + 2 * x)); }
    static __device__ __forceinline__ uint4 chunk(const uint8_t* row, int c) { return load_narrow16<HIGH>(row + c * 32); }
    // the span is 2 * len <= 32 bytes at a 2-byte aligned address; words beyond it are zero and narrow to bytes nobody reads
    static __device__ __forceinline__ void span(const uint8_t* row, int s0, int len, unsigned (&yw)[4])
    {
        unsigned wd[8];
        load_span_wide<2>(row + 2 * s0, 2 * len, wd);
#pragma unroll
        for (int j = 0; j < 4; j++) yw[j] = narrow4<HIGH>(wd[2 * j], wd[2 * j + 1]);
    }
};

// ---- the layouts ----------------------------------------------------------------------------------------------------------------------
// A fill policy is what a layout contributes to a kernel: planes<FR>() forms the frame bases of its N planes (frame_base<FR>) from plane 0 and
// the layout's extra block, fill() chooses the fill and hands it the layout's callable, id is what the launch is recorded under.
template <int N> struct PlaneSet { const uint8_t* p[N]; };
struct PackedPlanes {                  // one plane of packed pixels
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<1> planes(const uint8_t* plane, const PreParams& P, int f) { return {{frame_base<FR>(plane, f, P.frame_stride)}}; }
};
struct RgbpPlanes {                    // R, G, B planes at the same strides
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<3> planes(const uint8_t* rplane, const RgbpParams& rp, const PreParams& P, int f)
    {
        return {{frame_base<FR>(rplane, f, P.frame_stride), frame_base<FR>(rp.g, f, P.frame_stride), frame_base<FR>(rp.b, f, P.frame_stride)}};
    }
};

// Packed pixels of BPP bytes -- 3: AVD_FMT_BGR24 / _RGB24, 4: AVD_FMT_BGRA32 / _RGBA32, whose fourth byte is not read (scalar) or drops out of
// the dot products (vec16) -- in either channel order (RGB: the coefficient constants with bytes 0 and 2 exchanged, the same instruction stream).
// vec16: a chunk is BPP 16-byte loads; 32-bit pixels arrive one per dword and need no alignbyte.
template <bool VEC, bool RGB, int BPP>
struct Packed : PackedPlanes {
    static constexpr IngestKernel id = BPP == 4 ? (VEC ? kIngestPx32Vec16 : kIngestPx32Scalar) : (VEC ? kIngestBgrVec16 : kIngestBgrScalar);
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<1>& fr, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t* frame = fr.p[0];
        if (VEC)
            fill_vec16(tile, P, b, tid, [&](int64_t row, int c) {
                const uint4* src = reinterpret_cast<const uint4*>(frame + row + c * (16 * BPP));
                if constexpr (BPP == 4) {
                    const uint4 s0 = src[0], s1 = src[1], s2 = src[2], s3 = src[3];
                    return make_uint4(gray4_px<RGB>(s0.x, s0.y, s0.z, s0.w), gray4_px<RGB>(s1.x, s1.y, s1.z, s1.w),
                                      gray4_px<RGB>(s2.x, s2.y, s2.z, s2.w), gray4_px<RGB>(s3.x, s3.y, s3.z, s3.w));
                } else return gray16<RGB>(src[0], src[1], src[2]);
            });
        else fill_scalar(tile, P, b, tid, [&](int64_t row, int x) { return gray1<RGB>(frame + row + x * BPP); });
    }
};

// BGR24 / RGB24, the aligned fast path: a chunk's three 16-byte words are 48 consecutive bytes
template <int NI, bool RGB>
struct PackedStaged : PackedPlanes {
    static constexpr IngestKernel id = kIngestBgrStaged;
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<1>& fr, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t* frame = fr.p[0];
        fill_staged<NI>(tile, P, b, tid,
                        [&](int c) {
                            return [col = frame + c * 48](int64_t row, uint4 (&q)[3]) {
                                const uint4* src = reinterpret_cast<const uint4*>(col + row);
                                q[0] = src[0]; q[1] = src[1]; q[2] = src[2];
                            };
                        },
                        [](const uint4 (&q)[3]) { return gray16<RGB>(q[0], q[1], q[2]); });
    }
};

// the 16 gray bytes of 16 R, 16 G and 16 B bytes
__device__ __forceinline__ uint4 gray16_planar(const uint4& r, const uint4& g, const uint4& b)
{
    return make_uint4(gray4_planar(r.x, g.x, b.x), gray4_planar(r.y, g.y, b.y), gray4_planar(r.z, g.z, b.z), gray4_planar(r.w, g.w, b.w));
}

// Planar RGB (AVD_FMT_RGBP: three h x w planes that share P.row_stride): a pixel or a chunk (one 16-byte load per plane) gathered from the planes
template <bool VEC>
struct Rgbp : RgbpPlanes {
    static constexpr IngestKernel id = VEC ? kIngestRgbpVec16 : kIngestRgbpScalar;
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<3>& fr, const RgbpParams&, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t *rfr = fr.p[0], *gfr = fr.p[1], *bfr = fr.p[2];
        if (VEC)
            fill_vec16(tile, P, b, tid, [&](int64_t row, int c) {
                const int64_t o = row + c * 16;
                return gray16_planar(*reinterpret_cast<const uint4*>(rfr + o), *reinterpret_cast<const uint4*>(gfr + o),
                                     *reinterpret_cast<const uint4*>(bfr + o));
            });
        else
            fill_scalar(tile, P, b, tid, [&](int64_t row, int x) {
                const int64_t o = row + x;
                return (bfr[o] * 3735u + gfr[o] * 19235u + rfr[o] * 9798u + (1u << 14)) >> 15;
            });
    }
};

// Planar RGB, the aligned fast path: the three 16-byte words of a chunk come from the three planes -- PackedStaged's register footprint, so
// BGR's band plan and NI classes carry over (up to NI = 8: launch_preprocess)
template <int NI>
struct RgbpStaged : RgbpPlanes {
    static constexpr IngestKernel id = kIngestRgbpStaged;
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<3>& fr, const RgbpParams&, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t *rfr = fr.p[0], *gfr = fr.p[1], *bfr = fr.p[2];
        fill_staged<NI>(tile, P, b, tid,
                        [&](int c) {
                            return [=](int64_t row, uint4 (&q)[3]) {
                                const int64_t o = row + c * 16;
                                q[0] = *reinterpret_cast<const uint4*>(rfr + o);
                                q[1] = *reinterpret_cast<const uint4*>(gfr + o);
                                q[2] = *reinterpret_cast<const uint4*>(bfr + o);
                            };
                        },
                        [](const uint4 (&q)[3]) { return gray16_planar(q[0], q[1], q[2]); });
    }
};

// 4:2:0.  ROT: quarter turns clockwise from the stored to the displayed picture.  0: the stored picture is the displayed one; 2: the flipped
// instantiations of the same fills; 1, 3: the strip fill (VEC unused).  P describes the DISPLAYED picture throughout.
// NV12: U, V interleaved in one plane
template <bool VEC, int ROT>
struct Nv12 {
    static constexpr IngestKernel id = (ROT & 1) ? kIngestNv12Strip : VEC ? kIngestNv12Tables : kIngestNv12Scalar;
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<2> planes(const uint8_t* yplane, const Nv12Params& nv, const PreParams& P, int f)
    {
        return {{frame_base<FR>(yplane, f, P.frame_stride), frame_base<FR>(nv.uv, f, nv.uv_frame_stride)}};
    }
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<2>& fr, const Nv12Params& nv, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t *yfr = fr.p[0], *cfr = fr.p[1];
        if constexpr (ROT & 1)             // sample q of a chroma row is the byte pair at 2q
            fill_yuv420_strip<ROT, Luma8>(tile, yfr, nv.k, P, b, tid, [&](int cy, int q0, int nq, ChromaTerms (&t)[kStripChroma]) {
                unsigned cw[(kStripChroma + 1) / 2];
                load_span(cfr + (int64_t)cy * nv.uv_row_stride + q0 * 2, nq * 2, cw);
#pragma unroll
                for (int j = 0; j < kStripChroma; j++)
                    if (j < nq) t[j] = chroma_offsets(span_byte(cw, 2 * j), span_byte(cw, 2 * j + 1), nv.k);
            });
        else if (VEC)                      // the 16 chroma bytes of a chunk are one 16-byte load, pair j = bytes 2j (U) and 2j + 1 (V)
            fill_yuv420_tables<ROT == 2, Luma8>(tile, yfr, nv.k, P, b, tid, [&](int p, int c, ChromaTerms (&t)[8]) {
                chroma8_interleaved(*reinterpret_cast<const uint4*>(cfr + (int64_t)p * nv.uv_row_stride + c * 16), nv.k, t);
            });
        else
            fill_yuv420_scalar<ROT == 2, Luma8>(tile, yfr, nv.k, P, b, tid, [&](int cy, int cx, int& U, int& V) {
                const uint8_t* cp = cfr + (int64_t)cy * nv.uv_row_stride + cx * 2;
                U = cp[0]; V = cp[1];
            });
    }
};

// Planar 4:2:0 (I420; YV12 with the chroma pointers exchanged): the chroma fetched from two planes
template <bool VEC, int ROT>
struct I420 {
    static constexpr IngestKernel id = (ROT & 1) ? kIngestI420Strip : VEC ? kIngestI420Tables : kIngestI420Scalar;
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<3> planes(const uint8_t* yplane, const I420Params& ip, const PreParams& P, int f)
    {
        return {{frame_base<FR>(yplane, f, P.frame_stride), frame_base<FR>(ip.u, f, ip.c_frame_stride), frame_base<FR>(ip.v, f, ip.c_frame_stride)}};
    }
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<3>& fr, const I420Params& ip, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t *yfr = fr.p[0], *ufr = fr.p[1], *vfr = fr.p[2];
        if constexpr (ROT & 1)             // sample q is byte q of the U row and of the V row
            fill_yuv420_strip<ROT, Luma8>(tile, yfr, ip.k, P, b, tid, [&](int cy, int q0, int nq, ChromaTerms (&t)[kStripChroma]) {
                const int64_t o = (int64_t)cy * ip.c_row_stride + q0;
                unsigned uw[(kStripChroma + 3) / 4], vw[(kStripChroma + 3) / 4];
                load_span(ufr + o, nq, uw);
                load_span(vfr + o, nq, vw);
#pragma unroll
                for (int j = 0; j < kStripChroma; j++)
                    if (j < nq) t[j] = chroma_offsets(span_byte(uw, j), span_byte(vw, j), ip.k);
            });
        // Y plane 16-byte aligned, U and V planes 8-byte aligned: the 16 chroma bytes of a chunk are two 8-byte loads, 8 U and 8 V; pair j = U byte
        // j and V byte j.  (A contiguous frame has its V plane at 5wh/4, which w % 16 == 0 makes a multiple of 8 but not of 16.)
        else if (VEC)
            fill_yuv420_tables<ROT == 2, Luma8>(tile, yfr, ip.k, P, b, tid, [&](int p, int c, ChromaTerms (&t)[8]) {
                const int64_t o = (int64_t)p * ip.c_row_stride + c * 8;
                chroma8_planar(*reinterpret_cast<const uint2*>(ufr + o), *reinterpret_cast<const uint2*>(vfr + o), ip.k, t);
            });
        else
            fill_yuv420_scalar<ROT == 2, Luma8>(tile, yfr, ip.k, P, b, tid, [&](int cy, int cx, int& U, int& V) {
                const int64_t o = (int64_t)cy * ip.c_row_stride + cx;
                U = ufr[o]; V = vfr[o];
            });
    }
};

// ---- 10-bit 4:2:0 in 16-bit words (AVD_FMT_P010, AVD_FMT_I010): every sample is narrowed to 8 bits where it is loaded (narrow1 / narrow_pk) and
// the fills above run on what NV12 / I420 would have loaded.  Strides stay in BYTES; a luma row has 2w bytes.
// P010: NV12's planes, the 10 bits in the high bits of each word.  A chroma row has w words, sample q is the word pair at 4q
template <bool VEC, int ROT>
struct P010 {
    static constexpr IngestKernel id = (ROT & 1) ? kIngestP010Strip : VEC ? kIngestP010Tables : kIngestP010Scalar;
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<2> planes(const uint8_t* yplane, const Nv12Params& nv, const PreParams& P, int f)
    {
        return Nv12<VEC, ROT>::template planes<FR>(yplane, nv, P, f);
    }
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<2>& fr, const Nv12Params& nv, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t *yfr = fr.p[0], *cfr = fr.p[1];
        using Luma = Luma16<true>;
        if constexpr (ROT & 1)             // nq <= kStripChroma samples = that many dwords, U in the low and V in the high lane
            fill_yuv420_strip<ROT, Luma>(tile, yfr, nv.k, P, b, tid, [&](int cy, int q0, int nq, ChromaTerms (&t)[kStripChroma]) {
                unsigned cw[kStripChroma];
                load_span_wide<2>(cfr + (int64_t)cy * nv.uv_row_stride + q0 * 4, nq * 4, cw);
#pragma unroll
                for (int j = 0; j < kStripChroma; j++)
                    if (j < nq) {
                        const unsigned pk = narrow_pk<true>(cw[j]);
                        t[j] = chroma_offsets(pk_lo<true>(pk), pk_hi<true>(pk), nv.k);
                    }
            });
        else if (VEC)                      // the 16 chroma words of a chunk are two 16-byte loads; narrowed they are NV12's 16 chroma bytes
            fill_yuv420_tables<ROT == 2, Luma>(tile, yfr, nv.k, P, b, tid, [&](int p, int c, ChromaTerms (&t)[8]) {
                chroma8_interleaved(load_narrow16<true>(cfr + (int64_t)p * nv.uv_row_stride + c * 32), nv.k, t);
            });
        else
            fill_yuv420_scalar<ROT == 2, Luma>(tile, yfr, nv.k, P, b, tid, [&](int cy, int cx, int& U, int& V) {
                const uint8_t* cp = cfr + (int64_t)cy * nv.uv_row_stride + cx * 4;
                U = narrow1<true>(load_u16(cp)); V = narrow1<true>(load_u16(cp + 2));
            });
    }
};

// I010 (yuv420p10le; V-first with the chroma pointers exchanged): I420's planes, the 10 bits in the low bits of each word.  A chroma row has
// w / 2 words per plane, sample q is word q of the U row and of the V row
template <bool VEC, int ROT>
struct I010 {
    static constexpr IngestKernel id = (ROT & 1) ? kIngestI010Strip : VEC ? kIngestI010Tables : kIngestI010Scalar;
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<3> planes(const uint8_t* yplane, const I420Params& ip, const PreParams& P, int f)
    {
        return I420<VEC, ROT>::template planes<FR>(yplane, ip, P, f);
    }
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<3>& fr, const I420Params& ip, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t *yfr = fr.p[0], *ufr = fr.p[1], *vfr = fr.p[2];
        using Luma = Luma16<false>;
        if constexpr (ROT & 1)             // nq <= kStripChroma words per plane, two to a dword
            fill_yuv420_strip<ROT, Luma>(tile, yfr, ip.k, P, b, tid, [&](int cy, int q0, int nq, ChromaTerms (&t)[kStripChroma]) {
                const int64_t o = (int64_t)cy * ip.c_row_stride + q0 * 2;
                unsigned uw[(kStripChroma + 1) / 2], vw[(kStripChroma + 1) / 2];
                load_span_wide<1>(ufr + o, nq * 2, uw);
                load_span_wide<1>(vfr + o, nq * 2, vw);
#pragma unroll
                for (int i = 0; i < (kStripChroma + 1) / 2; i++) { uw[i] = narrow_pk<false>(uw[i]); vw[i] = narrow_pk<false>(vw[i]); }
#pragma unroll
                for (int j = 0; j < kStripChroma; j++)
                    if (j < nq) t[j] = chroma_offsets(span_byte(uw, 2 * j), span_byte(vw, 2 * j), ip.k);      // the low byte of lane j
            });
        // every plane 16-byte aligned: the 8 U and the 8 V words of a chunk are one 16-byte load each; narrowed they are I420's 8 + 8 chroma bytes.
        // (A contiguous frame has its V plane at 5wh/2 bytes, which w % 16 == 0 and an even h make a multiple of 16.)
        else if (VEC)
            fill_yuv420_tables<ROT == 2, Luma>(tile, yfr, ip.k, P, b, tid, [&](int p, int c, ChromaTerms (&t)[8]) {
                const int64_t o = (int64_t)p * ip.c_row_stride + c * 16;
                chroma8_planar(narrow8<false>(*reinterpret_cast<const uint4*>(ufr + o)), narrow8<false>(*reinterpret_cast<const uint4*>(vfr + o)), ip.k, t);
            });
        else
            fill_yuv420_scalar<ROT == 2, Luma>(tile, yfr, ip.k, P, b, tid, [&](int cy, int cx, int& U, int& V) {
                const int64_t o = (int64_t)cy * ip.c_row_stride + cx * 2;
                U = narrow1<false>(load_u16(ufr + o)); V = narrow1<false>(load_u16(vfr + o));
            });
    }
};

// 4:2:2.  The stored picture is the displayed one (a turned 4:2:2 picture is refused: avd_ingest_clip.h).
// Packed (AVD_FMT_YUYV422: Y0 U Y1 V; UYVY: U Y0 V Y1): every dword is a pixel pair with its own U and V.  Tables: a chunk is two 16-byte loads;
// a v_perm per luma word picks the four luma bytes of two dwords, the chroma bytes are taken where they lie -- no byte gather.
template <bool VEC, bool UYVY>
struct Yuyv {
    static constexpr IngestKernel id = VEC ? kIngestYuyvTables : kIngestYuyvScalar;
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<1> planes(const uint8_t* plane, const YuyvParams&, const PreParams& P, int f)
    {
        return {{frame_base<FR>(plane, f, P.frame_stride)}};
    }
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<1>& fr, const YuyvParams& yp, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t* frame = fr.p[0];
        if (VEC)
            fill_yuv422_tables(tile, yp.k, P, b, tid, [&](int y, int c, uint4& yy, ChromaTerms (&t)[8]) {
                const uint4* src = reinterpret_cast<const uint4*>(frame + (int64_t)y * P.row_stride + c * 32);
                const uint4 s0 = src[0], s1 = src[1];
                const unsigned d[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                constexpr unsigned luma = UYVY ? 0x07050301u : 0x06040200u;      // bytes 1, 3 (UYVY) or 0, 2 of the low, then of the high dword
                yy = make_uint4(__builtin_amdgcn_perm(d[1], d[0], luma), __builtin_amdgcn_perm(d[3], d[2], luma),
                                __builtin_amdgcn_perm(d[5], d[4], luma), __builtin_amdgcn_perm(d[7], d[6], luma));
#pragma unroll
                for (int j = 0; j < 8; j++)
                    t[j] = UYVY ? chroma_offsets(d[j] & 0xFF, (d[j] >> 16) & 0xFF, yp.k) : chroma_offsets((d[j] >> 8) & 0xFF, d[j] >> 24, yp.k);
            });
        else
            fill_yuv422_scalar(tile, yp.k, P, b, tid, [&](int y, int x, int& Y, int& U, int& V) {
                const uint8_t* p = frame + (int64_t)y * P.row_stride + (x >> 1) * 4;
                Y = p[2 * (x & 1) + (UYVY ? 1 : 0)]; U = p[UYVY ? 0 : 1]; V = p[UYVY ? 2 : 3];
            });
    }
};

// Planar 4:2:2 (I422; YV16 with the chroma pointers exchanged): I420's fetches with one chroma row per luma row -- a 16-byte Y load and two
// 8-byte chroma loads per chunk, hence I420's alignment rule (Y on 16, U and V on 8: a contiguous frame has its V plane at 3wh/2, a multiple
// of 8 but, for odd h, not of 16)
template <bool VEC>
struct I422 {
    static constexpr IngestKernel id = VEC ? kIngestI422Tables : kIngestI422Scalar;
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<3> planes(const uint8_t* yplane, const I420Params& ip, const PreParams& P, int f)
    {
        return I420<VEC, 0>::template planes<FR>(yplane, ip, P, f);
    }
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<3>& fr, const I420Params& ip, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t *yfr = fr.p[0], *ufr = fr.p[1], *vfr = fr.p[2];
        if (VEC)
            fill_yuv422_tables(tile, ip.k, P, b, tid, [&](int y, int c, uint4& yy, ChromaTerms (&t)[8]) {
                yy = *reinterpret_cast<const uint4*>(yfr + (int64_t)y * P.row_stride + c * 16);
                const int64_t o = (int64_t)y * ip.c_row_stride + c * 8;
                chroma8_planar(*reinterpret_cast<const uint2*>(ufr + o), *reinterpret_cast<const uint2*>(vfr + o), ip.k, t);
            });
        else
            fill_yuv422_scalar(tile, ip.k, P, b, tid, [&](int y, int x, int& Y, int& U, int& V) {
                const int64_t o = (int64_t)y * ip.c_row_stride + (x >> 1);
                Y = yfr[(int64_t)y * P.row_stride + x]; U = ufr[o]; V = vfr[o];
            });
    }
};

// NV16: NV12's planes with one chroma row per luma row -- two 16-byte loads per chunk
template <bool VEC>
struct Nv16 {
    static constexpr IngestKernel id = VEC ? kIngestNv16Tables : kIngestNv16Scalar;
    template <Frames FR>
    static __device__ __forceinline__ PlaneSet<2> planes(const uint8_t* yplane, const Nv12Params& nv, const PreParams& P, int f)
    {
        return Nv12<VEC, 0>::template planes<FR>(yplane, nv, P, f);
    }
    static __device__ __forceinline__ void fill(uint8_t* tile, const PlaneSet<2>& fr, const Nv12Params& nv, const PreParams& P, const Band& b, int tid)
    {
        const uint8_t *yfr = fr.p[0], *cfr = fr.p[1];
        if (VEC)
            fill_yuv422_tables(tile, nv.k, P, b, tid, [&](int y, int c, uint4& yy, ChromaTerms (&t)[8]) {
                yy = *reinterpret_cast<const uint4*>(yfr + (int64_t)y * P.row_stride + c * 16);
                chroma8_interleaved(*reinterpret_cast<const uint4*>(cfr + (int64_t)y * nv.uv_row_stride + c * 16), nv.k, t);
            });
        else
            fill_yuv422_scalar(tile, nv.k, P, b, tid, [&](int y, int x, int& Y, int& U, int& V) {
                const uint8_t* cp = cfr + (int64_t)y * nv.uv_row_stride + (x >> 1) * 2;
                Y = yfr[(int64_t)y * P.row_stride + x]; U = cp[0]; V = cp[1];
            });
    }
};

// ---- the two kernels: one workgroup per band; POL fills the tile from plane 0 and the layout's extra block, the rest is written once ----

// Generic kernel: any geometry / alignment that POL's fill takes; the resampling tables are read from global memory.
template <typename POL, Frames FR, typename... Extra>
__global__ __launch_bounds__(kThreads) void k_preprocess(const uint8_t* __restrict__ plane0, Extra... extra, int n, OutFrames<FR> out,
                                                        PreParams P, uint8_t* __restrict__ small,
                                                        float* __restrict__ rowbuf,
                                                        long long* __restrict__ lap_part)
{
    extern __shared__ __align__(16) uint8_t tile[];
    Band b;
    if (!decode_band(P, n, b)) return;
    b.of = out.at(b.f);
    const int tid = threadIdx.x;
    POL::fill(tile, POL::template planes<FR>(plane0, extra..., P, b.f), extra..., P, b, tid);
    fill_column_halo(tile, b.trows, P.pitch, P.w, tid);
    store_moments(lap_part, b.lid, tid, band_phases<false>(tile, nullptr, P, b, tid, small, rowbuf));
}

// Aligned fast path: the band staged in registers (fill_staged, which also writes the column halo) and the resampling tables in LDS, fetched
// ahead of the band's loads.
template <typename POL, Frames FR, typename... Extra>
__global__ __launch_bounds__(kThreads, 4) void k_preprocess_vec(const uint8_t* __restrict__ plane0, Extra... extra, int n, OutFrames<FR> out,
                                                               PreParams P, uint8_t* __restrict__ small,
                                                               float* __restrict__ rowbuf,
                                                               long long* __restrict__ lap_part)
{
    extern __shared__ __align__(16) uint8_t tile[];
    Band b;
    if (!decode_band(P, n, b)) return;
    b.of = out.at(b.f);
    const int tid = threadIdx.x;
    LdsTabs* lt = reinterpret_cast<LdsTabs*>(tile + lds_tile_bytes(P.rows_per_band + 2, P.pitch));
    fill_lds_tabs(lt, P, tid);
    POL::fill(tile, POL::template planes<FR>(plane0, extra..., P, b.f), extra..., P, b, tid);
    __syncthreads();
    store_moments(lap_part, b.lid, tid, band_phases<true>(tile, lt, P, b, tid, small, rowbuf));
}

// 32x32 INTER_AREA cells from the per-row partials (vertical accumulation in cv2's row
// order), then aHash bits: g >= mean(g)  <=>  1024*g >= sum(g)   (video.py:7-8)
// One block per frame f of the launch: it reads the row and Laplacian partials at f and writes the cells, bits and moments at the output frame --
// f, or (GROUPED: a grouped launch, option "ingest_group") entry f of the same table the ingest launch took.
template <bool GROUPED>
__global__ __launch_bounds__(1024) void k_hash(const float* __restrict__ rowbuf, HashParams P,
                                              uint8_t* __restrict__ area, uint8_t* __restrict__ bits,
                                              const long long* __restrict__ lap_part, int nbands, int waves,
                                              unsigned long long* __restrict__ lap, const int* __restrict__ out_frame)
{
    __shared__ int wsum[16];
    __shared__ long long lsum[2][16];
    const int f = blockIdx.x, tid = threadIdx.x;
    {   // exact Laplacian moments of the frame = sum of the per-wave partials of its bands
        long long s = 0, q = 0;
        for (int i = tid; i < nbands * waves; i += 1024) {
            const long long* slot = lap_part + (((int64_t)f * nbands + i / waves) * kLapSlots + i % waves) * 2;
            s += slot[0]; q += slot[1];
        }
        s = wave_sum(s); q = wave_sum(q);
        if ((tid & 63) == 0) { lsum[0][tid >> 6] = s; lsum[1][tid >> 6] = q; }
    }
    const int dy = tid >> 5, dx = tid & 31;
    const float* rb = rowbuf + (int64_t)f * P.h * AVD_HASH + dx;
    const int y0 = P.ay_begin[dy], cnt = P.ay_count[dy];
    int cell;
    if (P.area_fast) {
        int acc = 0;
        for (int k0 = 0; k0 < cnt; k0 += 8) {
            int v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = __float_as_int(rb[(int64_t)(y0 + min(k0 + j, cnt - 1)) * AVD_HASH]);
#pragma unroll
            for (int j = 0; j < 8; j++) acc += k0 + j < cnt ? v[j] : 0;
        }
        if (dx < P.fast_simd_w) cell = (acc + 2) >> 2;
        else {
            const float scale = 1.f / (float)P.fast_area;
            cell = (int)rintf(__fmul_rn((float)acc, scale));
        }
    } else {
        const float wf = P.ay_first[dy], wm = P.ay_mid[dy], wl = P.ay_last[dy];
        float acc = 0.f;
        // the sum is a dependent chain in cv2's row order; the LOADS are not: eight rows are fetched at a time (one frame =
        // one workgroup, so the kernel's time is this chain's memory latency: 35 round trips before, 5 now)
        for (int k0 = 0; k0 < cnt; k0 += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = rb[(int64_t)(y0 + min(k0 + j, cnt - 1)) * AVD_HASH];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int k = k0 + j;
                if (k < cnt) {
                    const float beta = k == 0 ? wf : (k == cnt - 1 ? wl : wm);
                    const float t = __fmul_rn(beta, v[j]);
                    acc = k == 0 ? t : __fadd_rn(acc, t);
                }
            }
        }
        cell = (int)rintf(acc);             // saturate_cast<uchar>: round-half-even, clamp
    }
    cell = min(255, max(0, cell));
    int s = wave_sum(cell);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) total += wsum[i];
    const int of = GROUPED ? out_frame[f] : f;
    area[(int64_t)of * 1024 + tid] = (uint8_t)cell;
    bits[(int64_t)of * 1024 + tid] = (uint8_t)(cell * 1024 >= total);
    if (tid == 0) {
        long long s = 0, q = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) { s += lsum[0][i]; q += lsum[1][i]; }
        lap[2 * of] = (unsigned long long)s;
        lap[2 * of + 1] = (unsigned long long)q;
    }
}

}  // namespace

// The band plan of width w: how the host cuts frames into bands, and which kernel shape that allows.
BandPlan band_plan(int w)
{
    BandPlan p{};
    p.pitch = ((w + 2 * kPad + 15) / 16) * 16;
    int r = kLdsBudget / p.pitch - 2;                  // LDS tile = (rows + 2) * pitch bytes
    int cap = kBandCap;
    const int chunks = w / 16;
    const bool staged = w % 16 == 0 && chunks <= kThreads;
    const int rpp = staged ? kThreads / chunks : 0;    // tile rows one pass of the staged kernel's workgroup covers
    // a lane of the staged kernel holds at most kMaxNI row chunks, so the tile may have at most kMaxNI * rpp rows -- 7-row bands at 4K
    if (staged) cap = std::min(cap, kMaxNI * rpp - 2);
    p.rows_per_band = std::max(std::min(r, cap), 1);
    // every width up to 16 * kThreads lands on one of 3, 4, 6, 8, 9 (narrow frames need fewer than 3 passes: surplus passes re-read the last row)
    if (staged) p.ni = std::max(3, (p.rows_per_band + 2 + rpp - 1) / rpp);
    return p;
}

// ---- runtime values as template arguments (in the style of fb_dispatch_width): f receives std::integral_constant objects ----
template <typename F>
static auto dispatch_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// the NI classes band_plan yields, up to CAP: false = no staged kernel of that NI is built
template <int CAP, int NI = 3, typename F>
static bool dispatch_ni(int ni, F&& f)
{
    if (ni == NI) return f(std::integral_constant<int, NI>{}), true;
    constexpr int next = NI == 3 ? 4 : NI == 4 ? 6 : NI == 6 ? 8 : 9;
    if constexpr (next > NI && next <= CAP) return dispatch_ni<CAP, next>(ni, f);
    return false;
}

// 4:2:0: f(VEC, ROT) for the six fills that are built -- a quarter turn has one fill whatever the alignment
template <typename F>
static void dispatch_turn(bool vec, int rot, F&& f)
{
    if (rot == 1) f(std::false_type{}, std::integral_constant<int, 1>{});
    else if (rot == 3) f(std::false_type{}, std::integral_constant<int, 3>{});
    else dispatch_bool(vec, [&](auto v) { rot == 2 ? f(v, std::integral_constant<int, 2>{}) : f(v, std::integral_constant<int, 0>{}); });
}

static constexpr bool is_staged(IngestKernel id) { return id == kIngestBgrStaged || id == kIngestRgbpStaged; }
static constexpr bool has_gray_tables(IngestKernel id)
{
    return id == kIngestNv12Tables || id == kIngestNv12Strip || id == kIngestI420Tables || id == kIngestI420Strip || id == kIngestYuyvTables ||
           id == kIngestI422Tables || id == kIngestNv16Tables || id == kIngestP010Tables || id == kIngestI010Tables || id == kIngestP010Strip ||
           id == kIngestI010Strip;
}

// POL's kernel: the staged body for the staged fills, the generic one for every other
template <typename POL, Frames FR, typename... Extra>
static constexpr auto ingest_kernel()
{
    if constexpr (is_staged(POL::id)) return k_preprocess_vec<POL, FR, Extra...>;
    else return k_preprocess<POL, FR, Extra...>;
}

// list (null: a strided clip): the clip's frames come from a device table of plane pointers -- d_in / d_uv / d_v are then the addresses of the
// table's per-plane arrays (n entries each), and list->aligned says whether every frame allows the 16-byte fills (list_vec_eligible).
// list->out_frame: a grouped launch -- the list's n frames are those of several clips that share `clip`'s key, and each writes where the table says.
int launch_preprocess(avd_ctx* ctx, const ClipSlot& slot, const IngestClip& clip, const uint8_t* d_in, const uint8_t* d_uv, const uint8_t* d_v,
                      const FrameTable* list)
{
    Workspace& ws = ctx->ws;
    PreParams P = slot.pre;
    P.row_stride = clip.row_stride;
    P.frame_stride = clip.frame_stride;
    const bool grouped = list && list->out_frame;
    const int n = grouped ? list->n : clip.n;
    if ((int64_t)n * P.nbands > avd_group::kMaxLaunchBands) { ctx->err = "too many bands in one ingest launch"; return AVD_ERR_ARG; }
    const int grid = (n * P.nbands + 7) / 8 * 8;
    uint8_t* const small = grouped ? ws.d_small.p : ws.d_small + (size_t)slot.f0 * AVD_NPIX;      // a grouped launch's frames name their places in the whole buffer
    const size_t tile = lds_tile_bytes(P.rows_per_band + 2, P.pitch);
    // bgr: no conversion constants -- BGR24 and the four layouts of RGB producers; planar: I420
    const bool bgr = !clip.is_yuv(), planar = clip.planar_yuv(), yuv422 = clip.is_422();
    const bool rgbp = clip.format == AVD_FMT_RGBP, px32 = clip.format == AVD_FMT_BGRA32 || clip.format == AVD_FMT_RGBA32;
    const bool rgb = clip.format == AVD_FMT_RGB24 || clip.format == AVD_FMT_RGBA32;     // packed pixels stored R, G, B
    const bool wide = clip.is_16bit();                 // P010 (with NV12's planes) and I010 (with I420's)
    const bool vec = list ? list->aligned : strided_vec_eligible(clip, d_in, d_uv, d_v);      // the one rule of avd_ingest_clip.h
    int ni = vec && bgr && !px32 ? band_plan(P.w).ni : 0;       // the layouts with a staged fill: BGR24, RGB24, RGBP
    // planar RGB: the byte gather needs a few registers more than BGR's alignbyte, and NI = 9 (2048 < w <= 4096) no longer fits the 128 VGPRs of
    // __launch_bounds__(256, 4) without spilling: those widths run the 16-byte fill
    if (rgbp && ni > 8) ni = 0;
    const int rot = clip.rotate;
    if (rot && bgr) { ctx->err = "internal error: a turned BGR clip reached the ingest launch"; return AVD_ERR_DEVICE; }
    if (clip.full_range && bgr) { ctx->err = "internal error: a full-range BGR clip reached the ingest launch"; return AVD_ERR_DEVICE; }
    YuvConsts yc{};
    size_t tabs = 0;                                   // tile + the three gray tables
    if (!bgr) {
        build_yuv_consts(yc, clip.full_range != 0);
        // every index the table fills can form, Y + offset + bias, must lie inside the tables these constants dimension
        int lo, hi;
        yuv_index_window(yc, lo, hi);
        if (lo + yc.bias < 0 || hi + yc.bias >= yc.ntab) {
            ctx->err = "internal error: the conversion constants index outside the gray tables";
            return AVD_ERR_DEVICE;
        }
        tabs = lds_nvtab_off(P.rows_per_band + 2, P.pitch) + lds_nvtab_bytes(yc.ntab);
    }
    // the launch of policy POL: its kernel body and LDS follow its id, the source of the frame bases follows `list`
    auto launch = [&](auto pol, auto... extra) {
        using POL = decltype(pol);
        const size_t lds = is_staged(POL::id) ? tile + sizeof(LdsTabs) : has_gray_tables(POL::id) ? tabs : tile;
        IngestRecord& rec = ctx->ingest;
        rec.plan = IngestPlan{P.h, P.w, P.rows_per_band, P.nbands, P.pitch, ni, (int)lds, POL::id};
        rec.launched = 1;
        rec.rotate = clip.rotate;
        rec.format = clip.format;
        rec.range = !bgr && clip.full_range;
        rec.list[0] = grouped ? 2 : list != nullptr;
        rec.list[1] = list ? n : 0;
        dispatch_bool(list != nullptr, [&](auto listed) {
            constexpr Frames FR = decltype(listed)::value ? Frames::listed : Frames::strided;
            auto kernel = ingest_kernel<POL, FR, decltype(extra)...>();
            OutFrames<FR> out{};
            if constexpr (FR == Frames::listed) out.tab = list->out_frame;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), lds, ctx->stream, d_in, extra..., n, out, P, small,
                               ws.d_rowbuf + slot.rowbuf_off, ws.d_lap_part + slot.lappart_off);
        });
    };
    bool built = true;                                 // false: the band plan's NI has no staged kernel
    if (yuv422) {                                      // one table and one scalar fill per layout, no turn
        if (rot) { ctx->err = "internal error: a turned 4:2:2 clip reached the ingest launch"; return AVD_ERR_DEVICE; }
        dispatch_bool(vec, [&](auto v) {
            constexpr bool V = decltype(v)::value;
            if (clip.format == AVD_FMT_I422) launch(I422<V>{}, I420Params{d_uv, d_v, clip.uv_row_stride, clip.uv_frame_stride, yc});
            else if (clip.format == AVD_FMT_NV16) launch(Nv16<V>{}, Nv12Params{d_uv, clip.uv_row_stride, clip.uv_frame_stride, yc});
            else if (clip.format == AVD_FMT_UYVY422) launch(Yuyv<V, true>{}, YuyvParams{yc});
            else launch(Yuyv<V, false>{}, YuyvParams{yc});
        });
    } else if (planar) {
        const I420Params ip{d_uv, d_v, clip.uv_row_stride, clip.uv_frame_stride, yc};
        dispatch_turn(vec, rot, [&](auto v, auto r) {
            if (wide) launch(I010<decltype(v)::value, decltype(r)::value>{}, ip);
            else launch(I420<decltype(v)::value, decltype(r)::value>{}, ip);
        });
    } else if (!bgr) {
        // (a register-staged variant in the style of k_preprocess_vec measured no faster: the kernel is bound by the
        // conversion's integer arithmetic, not by how its loads are issued -- profiles/r02_experiments.md)
        const Nv12Params nv{d_uv, clip.uv_row_stride, clip.uv_frame_stride, yc};
        dispatch_turn(vec, rot, [&](auto v, auto r) {
            if (wide) launch(P010<decltype(v)::value, decltype(r)::value>{}, nv);
            else launch(Nv12<decltype(v)::value, decltype(r)::value>{}, nv);
        });
    } else if (rgbp) {
        const RgbpParams rp{d_uv, d_v};
        // BGR's band plan and NI classes: the chunk has the same register footprint
        if (ni) built = dispatch_ni<8>(ni, [&](auto k) { launch(RgbpStaged<decltype(k)::value>{}, rp); });
        else dispatch_bool(vec, [&](auto v) { launch(Rgbp<decltype(v)::value>{}, rp); });
        if (!built) ctx->err = "internal error: the band plan asks for a k_preprocess_rgbp_vec that is not built";
    } else if (ni) {                                   // BGR24 and RGB24: the same band plan, the same NI, the same ids
        built = dispatch_bool(rgb, [&](auto o) { return dispatch_ni<kMaxNI>(ni, [&](auto k) { launch(PackedStaged<decltype(k)::value, decltype(o)::value>{}); }); });
        if (!built) ctx->err = "internal error: the band plan asks for a k_preprocess_vec that is not built";
    } else
        dispatch_bool(vec, [&](auto v) {
            dispatch_bool(rgb, [&](auto o) {
                if (px32) launch(Packed<decltype(v)::value, decltype(o)::value, 4>{});
                else launch(Packed<decltype(v)::value, decltype(o)::value, 3>{});
            });
        });
    if (!built) return AVD_ERR_DEVICE;
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// (the Hamming distances between consecutive frames are formed from these bits by k_records of the analyze entries)
int launch_hash(avd_ctx* ctx, const ClipSlot& slot, int n, const int* out_frame)
{
    Workspace& ws = ctx->ws;
    // the clip's slice of the call's buffers: frame slot.f0 onwards; a grouped launch's frames name their places in the whole buffers
    const size_t f0 = out_frame ? 0 : (size_t)slot.f0;
    dispatch_bool(out_frame != nullptr, [&](auto g) {
        hipLaunchKernelGGL(k_hash<decltype(g)::value>, dim3(n), dim3(1024), 0, ctx->stream, ws.d_rowbuf + slot.rowbuf_off, slot.hsh, ws.d_area + f0 * 1024,
                           ws.d_hash + f0 * 1024, (const long long*)(ws.d_lap_part + slot.lappart_off), slot.pre.nbands, kThreads / 64,
                           ws.d_lap + 2 * f0, out_frame);
    });
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
