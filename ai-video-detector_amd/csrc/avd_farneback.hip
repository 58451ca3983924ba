// avd_farneback.hip -- dense Farneback optical flow for batches of 320x320 frame pairs (gfx950): the per-frame kernels and the launch schedule.
//
// Replaces cv2.calcOpticalFlowFarneback(prev, cur, None, 0.5, 3, 15, 3, 5, 1.2, 0) and the flow-magnitude statistics of reference
// app/analyzers/video.py:45-48 for all consecutive pairs of a clip at once.  The arithmetic follows OpenCV 4.10's CPU path operation by operation
// (float where it is float, double accumulators where it keeps doubles, fused multiply-add only in the Gaussian row/column filters); what is
// re-designed is the schedule:
//   * per-FRAME work (Gaussian pyramid, polynomial expansion) is done once per frame and shared by the two pairs a frame belongs to (cv2
//     recomputes it per pair);
//   * all pairs of a clip advance through level/iteration in lock step, one launch per stage, so every launch has >= 10^5 independent work items.
// This file holds the kernels that are not a level's blur iterations -- k_pyramid_all, k_polyexp_all (per frame), k_flow_up (initial flow of
// a level), k_mag, k_stats_pair, k_flow_interleave (what follows the levels) -- and the schedule: launch_farneback = pyramid + polynomial
// expansion, then fast_levels (fb_mode = 1, the default) or exact_levels (fb_mode = 0); launch_farneback_rerun = exact_levels for the pairs
// the fast kernels flagged; launch_flow_stats.  The blur iterations (FarnebackUpdateMatrices + FarnebackUpdateFlow_Blur) have three
// implementations, each in its own file behind one launcher (avd_internal.h): avd_fbfast.hip (launch_fb_fast; flow within 1e-5 px of the
// oracle), avd_fbfused.hip (launch_fb_level; bit-identical to oracle/avd_oracle.c) and avd_fbtwo.hip (launch_fb_two; bit-identical, fallback).
// Not GEMM-shaped (11/19-tap separable stencils, 15x15 box sums, per-pixel 2x2 solves); MFMA is not applicable.
#include "avd_internal.h"
#include "avd_fb_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int S = AVD_SMALL;

// ---------------------------------------------------------------------------------------
// Gaussian pyramid level K (scale 2^-K): GaussianBlur(full-res, ksize, sigma) then the
// INTER_LINEAR decimation, which at these exact power-of-two scales is the 2x2 mean
// ((p00+p01)+(p10+p11))*0.25 of the two centre pixels.  Only the columns/rows the
// decimation reads are filtered.  One workgroup = one BAND of one frame, BAND = STEPS x TR output rows, walked in steps of TR rows:
//   source rows (uint8, reflect-101) -> LDS;  row pass (FMA chain, cv2's RowVec_32f order)
//   -> LDS float [rows][NC];  column pass (SymmColumnVec_32f order) + 2x2 mean -> I[f][dy][dx].
// A step's TR output rows read SROWS row-filtered source rows, of which the last KEEP = SROWS - NEW are also the first KEEP of the next step
// (NEW = TR 2^K: how far the window moves).  A later step of a band therefore moves those KEEP float rows to the top of the LDS array and loads,
// converts and row-filters only its NEW rows: the LDS plan stays that of ONE step (29 KB -- the 76 rows that eight 40-px output rows need at
// once are 50 KB and held a CU to three workgroups), while a source row is filtered (SROWS + (STEPS - 1) NEW) / (STEPS NEW) times per frame
// instead of SROWS / NEW times.  The bands are kept short -- a workgroup's steps are a serial chain -- and the 160-px scale, whose 3-tap
// filter overlaps by two rows in sixteen, is not walked at all.  (The kernel's 104 registers, not its LDS, hold a CU to four workgroups;
// a build capped at 96 registers keeps five, spills twelve of them and is 0.4 us of 25 faster: not kept, profiles/pyramid_bands_ab.txt.)
// ---------------------------------------------------------------------------------------
template <int K>
struct PyrGeo {
    static constexpr int WL = S >> K;
    static constexpr int NC = K == 0 ? S : 2 * WL;              // filtered columns per row
    static constexpr int OFF = K == 0 ? 0 : (1 << K) / 2 - 1;
    // output rows per step: four at the two coarse scales -- their long filters need (TR - 1) 2^K + 2 + 2 HALF source rows
    static constexpr int TR = K >= 2 ? 4 : 8;                   // (2 / 4 / 4 / 8 rows -- 22 KB, seven workgroups per CU -- is slower: 57 vs 52 us)
    static constexpr int STEPS = K >= 2 ? 2 : 1, BAND = STEPS * TR;   // a band: eight output rows at every scale
    static constexpr int TILES = WL / BAND;                     // workgroups per frame
    static constexpr int KS = K == 3 ? 19 : (K == 2 ? 9 : 3), HALF = KS / 2;
    static constexpr int SROWS = K == 0 ? TR + 2 * HALF : ((TR - 1) << K) + 2 + 2 * HALF;   // source rows a step reads
    static constexpr int NEW = K == 0 ? TR : TR << K, KEEP = SROWS - NEW;                   // rows a later step adds / takes over
    static constexpr int PADX = 12, PS = S + 2 * PADX;          // source rows carry their reflected borders (HALF <= 9 < PADX, PADX % 4 == 0)
    static constexpr int SRC_BYTES = SROWS * PS, LDS_BYTES = SRC_BYTES + SROWS * NC * 4;
    // source rows loaded, converted and row-filtered per frame, against the frame's S rows, in percent: 112 / 118 / 118 at 160 / 80 / 40 px
    // (unwalked: 112 / 137 / 137; the 320-px scale, which runs with fb_fold_blur off only, is at 125)
    static constexpr int FILTERED_PCT = TILES * (SROWS + (STEPS - 1) * NEW) * 100 / S;
    static_assert(WL % BAND == 0 && (K == 0 || FILTERED_PCT <= 120), "whole bands; a source row is filtered at most 1.2 times per frame");
    static_assert(STEPS == 1 || (KEEP * NC <= 4 * 256 && SRC_BYTES % 16 == 0 && (NEW * NC) % 4 == 0 && (KEEP * NC) % 4 == 0),
                  "the rows a step takes over move as one 16-byte piece per lane");
};
constexpr int cmax(int a, int b) { return a > b ? a : b; }
constexpr int cgcd(int a, int b) { return b == 0 ? a : cgcd(b, a % b); }

// The items it = tid, tid + 256, ... of a 256-thread workgroup as (row, column) = (it / PR, it % PR), without a division: the first by comparisons,
// the following ones by a constant step with one wrap.  The columns a lane meets repeat after PER items, which are SG rows further down.
template <int PR>
struct PyrWalk {
    static constexpr int PER = PR / cgcd(256, PR), SG = 256 / cgcd(256, PR);
    __device__ static __forceinline__ void first(int tid, int& r, int& c)
    {
        r = 0; c = tid;
#pragma unroll
        for (int q = 1; q * PR < 256; q++)
            if (tid >= q * PR) { r = q; c = tid - q * PR; }
    }
    __device__ static __forceinline__ void next(int& r, int& c)
    {
        r += 256 / PR; c += 256 % PR;
        if (c >= PR) { c -= PR; r++; }
    }
};
constexpr int kPyrLds = cmax(cmax(PyrGeo<3>::LDS_BYTES, PyrGeo<2>::LDS_BYTES), cmax(PyrGeo<1>::LDS_BYTES, PyrGeo<0>::LDS_BYTES));   // 29 KB

typedef float pyr_f4 __attribute__((ext_vector_type(4)));
typedef float pyr_f2 __attribute__((ext_vector_type(2)));

// One step of a band: the TR output rows out[0 .. TR)[WL] of frame img, whose first row-filtered source row, LDS row 0, is image row y_first
// (may be < 0: reflected).  LDS rows [0, rb) are taken over from the step before (rb = 0 in a band's first step, KEEP in the others: this lane's
// piece of them arrives in `kept`), rows [rb, SROWS) are loaded and filtered here; `more`: another step follows, its piece is left in `kept`.
// diffword (K == 1 only, may be null): the tile also compares its source rows with the same rows of the NEXT frame and leaves "they differ" in
// *diffword = pairdiff[f * TILES + t] -- the 20 tiles of the 160-px scale read every row of the frame (with overlap), so their OR says whether pair
// (f, f + 1) is a pair of bit-identical frames (which the fast level kernels exempt from the border-sign criterion, avd_fbfast.hip)
// a * b + c of a Gaussian tap: the fused multiply-add of the default model, or (MA: bit 1 of option "cv2_model", GAUSS_MULADD) a rounded product
// followed by a rounded sum -- the intrinsics, which the compiler never contracts
template <bool MA>
__device__ __forceinline__ float pyr_mac(float a, float b, float c)
{
    if constexpr (MA) return __fadd_rn(__fmul_rn(a, b), c);
    else return __builtin_fmaf(a, b, c);
}

// MA: see pyr_mac.  LERP (bit 16 of "cv2_model", RESIZE_LERP): the decimation to 80 / 40 px -- the general INTER_LINEAR path with both weights 0.5 --
// is a + (b - a) * 0.5 along x, then along y, instead of a * 0.5 + b * 0.5 (the 2 x 2 mean); the 160-px scale takes cv2's exact-2x area path and has no lerp
template <int K, bool MA = false, bool LERP = false>
__device__ __forceinline__ void pyramid_step(char* lds, const uint8_t* __restrict__ img, const float (&kw)[PyrGeo<K>::KS], float* __restrict__ out,
                                             int y_first, int rb, pyr_f4& kept, bool more, int* __restrict__ diffword)
{
    using G = PyrGeo<K>;
    constexpr int WL = G::WL, NC = G::NC, OFF = G::OFF, TR = G::TR, KS = G::KS, HALF = G::HALF, SROWS = G::SROWS;
    constexpr int PADX = G::PADX, PS = G::PS;
    uint8_t (*src)[PS] = reinterpret_cast<uint8_t (*)[PS]>(lds);
    float (*rowf)[NC] = reinterpret_cast<float (*)[NC]>(lds + G::SRC_BYTES);
    const int tid = threadIdx.x;
    const bool cmp = K == 1 && diffword != nullptr;      // workgroup-uniform
    static_assert(K != 1 || G::STEPS == 1, "the pair-identity word is formed by a tile that loads all its source rows in one step");
    // Source rows -> LDS.  A lane's loads are issued in batches, a whole batch before the first of them is waited for and written (the item loops
    // are unrolled over registers, the row's reflection is a select): as "load, wait, write" per item the up to fourteen loads of a lane each
    // paid the memory latency, one after the other, and that chain was most of a workgroup's time.
    static_assert(HALF + 1 < S, "a source row is reflected at most once");
    // byte offset of LDS row r's image row (BORDER_REFLECT_101) in the frame: unsigned, so that a load is "uniform base + 32-bit lane offset"
    auto row_at = [&](int r) -> unsigned { const int y = y_first + r; return (unsigned)(y < 0 ? -y : (y >= S ? 2 * S - 2 - y : y)) * S; };
    constexpr int NLD = (SROWS * (S / 4) + 255) / 256, NBD = (SROWS * 2 * HALF + 255) / 256;
    const int nld = (SROWS - rb) * (S / 4), nbd = (SROWS - rb) * 2 * HALF;
    constexpr int NBATCH = 8;                            // loads of a lane in flight at a time: two batches where a lane has up to fourteen
    int differs = 0;
#pragma unroll
    for (int e0 = 0; e0 < NLD; e0 += NBATCH) {
        const bool last = e0 + NBATCH >= NLD;            // the reflected columns' bytes travel with the last batch
        unsigned v[NBATCH], vn[K == 1 ? NBATCH : 1];
        uint8_t bv[NBD];
#pragma unroll
        for (int e = e0; e < NLD && e < e0 + NBATCH; e++) {
            const int it = tid + 256 * e, q = it / (S / 4), c4 = it - q * (S / 4);
            if (it >= nld) continue;
            const unsigned at = row_at(rb + q) + 4u * c4;
            v[e - e0] = *reinterpret_cast<const unsigned*>(img + at);
            if (K == 1 && cmp) vn[e - e0] = *reinterpret_cast<const unsigned*>(img + (at + AVD_NPIX));
        }
        // the reflected columns, so that the taps below need no index arithmetic: x = -1 - i is x = 1 + i, x = S + i is S - 2 - i
#pragma unroll
        for (int e = 0; e < NBD; e++) {
            const int it = tid + 256 * e, q = it / (2 * HALF), i = it - q * (2 * HALF);
            if (!last || it >= nbd) continue;
            bv[e] = img[row_at(rb + q) + (unsigned)(i < HALF ? 1 + i : S - 2 - (i - HALF))];
        }
#pragma unroll
        for (int e = e0; e < NLD && e < e0 + NBATCH; e++) {
            const int it = tid + 256 * e, q = it / (S / 4), c4 = it - q * (S / 4);
            if (it >= nld) continue;
            reinterpret_cast<unsigned*>(src[rb + q] + PADX)[c4] = v[e - e0];
            if (K == 1 && cmp) differs |= v[e - e0] != vn[e - e0];
        }
#pragma unroll
        for (int e = 0; e < NBD; e++) {
            const int it = tid + 256 * e, q = it / (2 * HALF), i = it - q * (2 * HALF);
            if (!last || it >= nbd) continue;
            src[rb + q][i < HALF ? PADX - 1 - i : PADX + S + (i - HALF)] = bv[e];
        }
        __builtin_amdgcn_sched_barrier(0);               // (the next batch's loads stay behind this batch's writes)
    }
    if (K == 1 && cmp) {
        const int any = __syncthreads_or(differs);
        if (tid == 0) *diffword = any;
    } else
        __syncthreads();                                 // (a later step: the column pass of the step before has read the rows written below)
    if (G::STEPS > 1 && rb && tid < G::KEEP * NC / 4) reinterpret_cast<pyr_f4*>(&rowf[0][0])[tid] = kept;
    // The two passes below are item loops "for (it = tid; it < rows * PR; it += 256)" over (row, column) = (it / PR, it % PR), PR items per row,
    // the row pass over LDS rows [rb, SROWS).
    // The columns a lane meets repeat after W::PER items = W::SG rows (PyrWalk), so a lane OWNS up to PER columns and walks down the rows in steps of SG:
    // the column, the window's word base, the LDS addresses and the tap weights are formed once in front of the loop, and no division
    // is left in it (round-5 counters: 2.4 x the VALU instructions of the filters themselves, the difference was this index work per item).
    if (KS == 3) {
        // every column is filtered at these scales (x = j): a lane does four of them from three aligned words
        static_assert(KS != 3 || NC == S, "the 3-tap scales filter whole rows");
        using W = PyrWalk<S / 4>;
        const unsigned* wp0[W::PER]; pyr_f4* dst0[W::PER]; int r0[W::PER];
        {
            int r, c4;
            W::first(tid, r, c4);
#pragma unroll
            for (int i = 0; i < W::PER; i++) {
                r0[i] = r;
                wp0[i] = reinterpret_cast<const unsigned*>(src[r] + PADX + 4 * c4);
                dst0[i] = reinterpret_cast<pyr_f4*>(&rowf[r][4 * c4]);
                W::next(r, c4);
            }
        }
        for (int sb = rb; sb < SROWS; sb += W::SG) {
#pragma unroll
            for (int i = 0; i < W::PER; i++) {
                if (256 * i >= SROWS * (S / 4) || r0[i] + sb >= SROWS) continue;
                const unsigned* wp = wp0[i] + sb * (PS / 4);
                const unsigned pw = wp[-1], cwd = wp[0], nw = wp[1];
                const float b[6] = {(float)(pw >> 24), (float)(cwd & 0xFFu), (float)((cwd >> 8) & 0xFFu), (float)((cwd >> 16) & 0xFFu),
                                    (float)(cwd >> 24), (float)(nw & 0xFFu)};
                pyr_f4 o;
#pragma unroll
                for (int e = 0; e < 4; e++) o[e] = pyr_mac<MA>(b[e + 1], kw[1], (b[e] + b[e + 2]) * kw[0]);
                dst0[i][sb * (NC / 4)] = o;
            }
        }
    } else {
        // The filtered columns come in adjacent pairs x0 = (jp << K) + OFF and x0 + 1, whose windows share KS - 1 of their KS + 1 source bytes: an
        // item is a PAIR.  Its window x0 - HALF .. x0 + HALF + 1 begins B0 + (jp << K) bytes into the LDS row, at the same byte of a word for every
        // pair (2^K is a multiple of four): aligned 32-bit LDS reads, ONE v_cvt_f32_ubyteN per distinct byte with a constant byte number (no
        // alignment of the window), the two FMA chains of the pair on the same converted bytes, and one 8-byte write of the two results.
        static_assert(KS == 3 || (K >= 2 && NC == 2 * WL), "the long filters run at the decimated scales, where the columns are pairs");
        using W = PyrWalk<WL>;
        constexpr int B0 = PADX + OFF - HALF, SH = B0 & 3, NW = (SH + KS + 1 + 3) / 4;   // window of pair 0: first byte, its place in a word, aligned words
        const unsigned* wp0[W::PER]; pyr_f2* dst0[W::PER]; int r0[W::PER];
        {
            int r, jp;
            W::first(tid, r, jp);
#pragma unroll
            for (int i = 0; i < W::PER; i++) {
                r0[i] = r;
                wp0[i] = reinterpret_cast<const unsigned*>(src[r] + (B0 & ~3) + (jp << K));
                dst0[i] = reinterpret_cast<pyr_f2*>(&rowf[r][2 * jp]);
                W::next(r, jp);
            }
        }
        for (int sb = rb; sb < SROWS; sb += W::SG) {
#pragma unroll
            for (int i = 0; i < W::PER; i++) {
                if (256 * i >= SROWS * WL || r0[i] + sb >= SROWS) continue;
                const unsigned* wp = wp0[i] + sb * (PS / 4);
                unsigned d[NW];
#pragma unroll
                for (int q = 0; q < NW; q++) d[q] = wp[q];
                float b[KS + 1];
#pragma unroll
                for (int q = 0; q <= KS; q++) b[q] = (float)((d[(SH + q) >> 2] >> (8 * ((SH + q) & 3))) & 0xFFu);
                float v0 = 0.f, v1 = 0.f;
#pragma unroll
                for (int q = 0; q < KS; q++) {
                    v0 = pyr_mac<MA>(b[q], kw[q], v0);
                    v1 = pyr_mac<MA>(b[q + 1], kw[q], v1);
                }
                dst0[i][sb * (NC / 2)] = pyr_f2{v0, v1};
            }
        }
    }
    __syncthreads();
    auto colf = [&](const float* c) {                    // c = the centre tap's row, this column
        float sacc = pyr_mac<MA>(c[0], kw[HALF], 0.f);
#pragma unroll
        for (int k = 1; k <= HALF; k++) sacc = pyr_mac<MA>(c[k * NC] + c[-k * NC], kw[HALF + k], sacc);
        return sacc;
    };
    {
        using W = PyrWalk<WL>;
        int dyl, dx;
        W::first(tid, dyl, dx);
#pragma unroll
        for (int i = 0; i < W::PER; i++) {
            if (256 * i < TR * WL) {
                for (int y = dyl; y < TR; y += W::SG) {              // (one turn wherever SG >= TR: every scale but the 320-px one)
                    float o;
                    if (K == 0) {
                        o = colf(&rowf[y + HALF][dx]);
                    } else {
                        // the output's 2 x 2 block: centre taps in LDS rows (y << K) + HALF (source row (dy << K) + OFF) and the one below, columns
                        // 2 dx and 2 dx + 1.  The four windows cover 2 HALF + 2 rows of that column pair: each is read ONCE, as 8 bytes
                        const pyr_f2* c = reinterpret_cast<const pyr_f2*>(&rowf[y << K][2 * dx]);
                        float w[2][2 * HALF + 2];
#pragma unroll
                        for (int q = 0; q < 2 * HALF + 2; q++) {
                            const pyr_f2 v = c[q * (NC / 2)];
                            w[0][q] = v.x; w[1][q] = v.y;
                        }
                        float p[2][2];                                     // [row of the block][column]
#pragma unroll
                        for (int a = 0; a < 2; a++)
#pragma unroll
                            for (int e = 0; e < 2; e++) {
                                float sacc = pyr_mac<MA>(w[e][HALF + a], kw[HALF], 0.f);
#pragma unroll
                                for (int k = 1; k <= HALF; k++) sacc = pyr_mac<MA>(w[e][HALF + a + k] + w[e][HALF + a - k], kw[HALF + k], sacc);
                                p[a][e] = sacc;
                            }
                        if constexpr (LERP && K >= 2) {
                            const float h0 = p[0][0] + (p[0][1] - p[0][0]) * 0.5f, h1 = p[1][0] + (p[1][1] - p[1][0]) * 0.5f;
                            o = h0 + (h1 - h0) * 0.5f;
                        } else
                            o = ((p[0][0] + p[0][1]) + (p[1][0] + p[1][1])) * 0.25f;
                    }
                    out[y * WL + dx] = o;
                }
            }
            W::next(dyl, dx);
        }
    }
    // the rows the next step takes over, LDS rows [NEW, SROWS): read before that step's barrier, written to rows [0, KEEP) behind it
    if (G::STEPS > 1 && more && tid < G::KEEP * NC / 4) kept = reinterpret_cast<const pyr_f4*>(&rowf[G::NEW][0])[tid];
}

// blk = frame * TILES + band of this scale: the band's steps, top to bottom.  pairdiff: see pyramid_step
template <int K, bool MA = false, bool LERP = false>
__device__ __forceinline__ void pyramid_body(char* lds, int blk, const uint8_t* __restrict__ small, const FbConsts* __restrict__ C,
                                             float* __restrict__ I, int n = 0, int* __restrict__ pairdiff = nullptr)
{
    using G = PyrGeo<K>;
    constexpr int WL = G::WL;
    const int f = blk / G::TILES, t = blk - f * G::TILES;
    const int dy0 = t * G::BAND;                         // the band's first output row
    const uint8_t* img = small + (int64_t)f * AVD_NPIX;
    float* out = I + ((int64_t)f * WL + dy0) * WL;
    int* diffword = K == 1 && pairdiff != nullptr && f + 1 < n ? pairdiff + blk : nullptr;
    float kw[G::KS];                                     // the tap weights (uniform: scalar registers)
#pragma unroll
    for (int q = 0; q < G::KS; q++) kw[q] = C->gk[K][q];
    const int y_first = (K == 0 ? dy0 : (dy0 << K) + G::OFF) - G::HALF;
    pyr_f4 kept = {0.f, 0.f, 0.f, 0.f};
    for (int step = 0; step < G::STEPS; step++)
        pyramid_step<K, MA, LERP>(lds, img, kw, out + step * G::TR * WL, y_first + step * G::NEW, step ? G::KEEP : 0, kept, step + 1 < G::STEPS, diffword);
}


// the four scales of every frame in ONE launch (coarsest first: its workgroups do the most work): the small scales
// alone cannot fill the chip (600 workgroups at 40 px for a 120-frame clip) and used to run one after the other
// It also clears the per-pair ill-posedness flags of the chunk (the fast level kernels, which come later on the stream, set them).
template <bool MA, bool LERP>
__device__ __forceinline__ void pyramid_all(char* lds, const uint8_t* __restrict__ small, int n, const FbConsts* __restrict__ C,
                                            float* __restrict__ I0, float* __restrict__ I1, float* __restrict__ I2,
                                            float* __restrict__ I3, int* __restrict__ flags, int* __restrict__ pairdiff)
{
    static_assert(PyrGeo<1>::TILES == kPairDiffTiles, "avd_fbfast.hip reads one word per 160-px tile");
    if (flags && (int)(blockIdx.x * 256 + threadIdx.x) < n - 1) flags[blockIdx.x * 256 + threadIdx.x] = 0;
    const int n3 = n * PyrGeo<3>::TILES, n2 = n * PyrGeo<2>::TILES, n1 = n * PyrGeo<1>::TILES;
    int b = blockIdx.x;
    if (b < n3) { pyramid_body<3, MA, LERP>(lds, b, small, C, I3); return; }
    b -= n3;
    if (b < n2) { pyramid_body<2, MA, LERP>(lds, b, small, C, I2); return; }
    b -= n2;
    if (b < n1) { pyramid_body<1, MA, LERP>(lds, b, small, C, I1, n, pairdiff); return; }
    if (I0) pyramid_body<0, MA, LERP>(lds, b - n1, small, C, I0);     // null: the polynomial expansion forms the 320-px scale's 3 x 3 blur itself (the grid ends before)
}

__global__ __launch_bounds__(256) void k_pyramid_all(const uint8_t* __restrict__ small, int n, const FbConsts* __restrict__ C,
                                                    float* __restrict__ I0, float* __restrict__ I1, float* __restrict__ I2,
                                                    float* __restrict__ I3, int* __restrict__ flags, int* __restrict__ pairdiff)
{
    __shared__ __align__(16) char lds[kPyrLds];
    pyramid_all<false, false>(lds, small, n, C, I0, I1, I2, I3, flags, pairdiff);
}

// the same launch under a non-zero "cv2_model" (bits 1 and 16: MA, LERP); with bit 8 (three scales) the 40-px tiles still run -- their
// workgroups are the first of the grid, and nobody reads what they write
template <bool MA, bool LERP>
__global__ __launch_bounds__(256) void k_pyramid_model(const uint8_t* __restrict__ small, int n, const FbConsts* __restrict__ C,
                                                      float* __restrict__ I0, float* __restrict__ I1, float* __restrict__ I2,
                                                      float* __restrict__ I3, int* __restrict__ flags, int* __restrict__ pairdiff)
{
    __shared__ __align__(16) char lds[kPyrLds];
    pyramid_all<MA, LERP>(lds, small, n, C, I0, I1, I2, I3, flags, pairdiff);
}

// ---------------------------------------------------------------------------------------
// FarnebackPolyExp (poly_n = 5), all four scales in ONE launch.  A 320-thread workgroup works on 320 / w consecutive image
// rows of one frame at a time (one row at 320 px, eight at 40 px: every lane has a pixel at every scale).  Vertical 11-tap pass in
// float into LDS (the 3 moments of a column as one quad, replicate border), horizontal pass with double accumulators, 5 interleaved
// coefficients R[y][x][c] (cv2's own layout: the level kernel gathers a pixel's five coefficients and its right-hand
// neighbour's as ten consecutive floats).  The workgroup's output is ONE contiguous span of 1600 floats: it is staged in
// LDS and stored as 16-byte pieces (a lane's own five floats are 20 bytes apart from its neighbour's).
// ---------------------------------------------------------------------------------------
struct PolyPtrs { const float* I[AVD_FB_LEVELS]; float* R[AVD_FB_LEVELS]; const uint8_t* small; };   // small != null: the 320-px scale is blurred here

constexpr int kPolyRows = 16;                            // image rows per workgroup (a band) of the 320-, 160- and 80-px scales
constexpr int kPolyQuads = 4 * (S / 4 + 10);             // quads of one LDS row buffer: the 80-px scale's four sub-rows of w + 10 (330 / 340 / 360)
static_assert(AVD_FB_LEVELS == 4, "three walking scales and the one-row form of the coarsest");
// workgroups per frame at scale k: bands of kPolyRows rows, at the coarsest scale single steps of 2^k rows (20 / 10 / 5 / 5)
__host__ __device__ constexpr int poly_wgs(int k) { return k < AVD_FB_LEVELS - 1 ? (S >> k) / kPolyRows : S >> (2 * k); }

// The vertical pass leaves a column's three moments in LDS as ONE 16-byte quad {t0, t1, t1, t2}: a single 128-bit read then hands the
// horizontal pass (t0, t1) and (t1, t2) as two aligned register pairs, which is what its packed sums, differences and products take as
// operands -- from three separate moment rows every pair had to be put together with register moves first.
typedef float pf4 __attribute__((ext_vector_type(4)));
typedef float pf2 __attribute__((ext_vector_type(2)));

// quad of column x of a w-wide row (rowq: the row's w + 10 quads); the two edge lanes also write the five replicated quads of their side
__device__ __forceinline__ void polyexp_put(pf4* __restrict__ rowq, int x, int w, float t0, float t1, float t2)
{
    const pf4 t = {t0, t1, t1, t2};
    rowq[x + 5] = t;
    if (x == 0)
        for (int q = 0; q < 5; q++) rowq[q] = t;
    if (x == w - 1)
        for (int q = 0; q < 5; q++) rowq[w + 5 + q] = t;
}

// Horizontal pass of one pixel (rq: its own quad; rq[-5 .. 5] are read) -> its five coefficients o[0 .. 4].  Per tap: (s0, s1) and (d0, d1)
// from the low pairs, (s1, s2) from the high pairs, (d0, d1) * xg and (s1, s2) * g -- five two-component operations (v_pk_add_f32 /
// v_pk_mul_f32: each half is the IEEE single operation of the scalar form on the same operands), then cv2's double accumulations in cv2's order.
__device__ __forceinline__ void polyexp_hpass(const pf4* __restrict__ rq, const float (&g)[6], const float (&xg)[6], const double (&gd)[6],
                                              const double (&xxgd)[6], double ig11, double ig03, double ig33, double ig55, float* __restrict__ o)
{
    const pf4 c = rq[0];
    double b1 = (double)(c.x * g[0]), b2 = 0, b3 = (double)(c.y * g[0]), b4 = 0, b5 = (double)(c.w * g[0]), b6 = 0;
#pragma unroll
    for (int q = 1; q <= 5; q++) {
        const pf4 p = rq[q], m = rq[-q];
        const pf2 s01 = p.xy + m.xy, d01 = p.xy - m.xy, s12 = p.zw + m.zw;
        const pf2 dx = d01 * pf2{xg[q], xg[q]};          // (r0p - r0m) * xg, (r1p - r1m) * xg
        const pf2 sg = s12 * pf2{g[q], g[q]};            // (r1p + r1m) * g, (r2p + r2m) * g
        // tg and the taps are float VALUES held in doubles: their product has at most 48 significant bits, i.e. it is exact in
        // double, so cv2's "b += tg * g" (a rounded product, then a rounded sum) IS the fused multiply-add, bit for bit -- one
        // double instruction instead of two on the pass that bounds this kernel
        const double tg = (double)s01.x;
        b1 = __builtin_fma(tg, gd[q], b1);
        b4 = __builtin_fma(tg, xxgd[q], b4);
        b2 += (double)dx.x;
        b3 += (double)sg.x;
        b6 += (double)dx.y;
        b5 += (double)sg.y;
    }
    o[0] = (float)(b3 * ig11);
    o[1] = (float)(b2 * ig11);
    o[2] = (float)(b1 * ig03 + b5 * ig33);
    o[3] = (float)(b1 * ig03 + b4 * ig33);
    o[4] = (float)(b6 * ig55);
}

// The 320-, 160- and 80-px scales (K = 0, 1, 2): a workgroup walks a band of kPolyRows consecutive image rows in steps of R = 2^K rows
// (lane = (sub-row, column): every lane has a pixel in every step).  A lane keeps the eleven rows of its column that the vertical pass
// reads in registers and slides them by R rows per step (R new loads per step instead of eleven, (10 + kPolyRows) / kPolyRows loads per
// pixel with the band's halo), the two LDS buffers alternate, so a step costs ONE workgroup barrier, and the coalesced 16-byte stores
// of step i - 1 are issued while step i is in its horizontal pass.  Same arithmetic per pixel as the one-row form below (which still
// serves the 40-px scale: eight rows per step, nothing to slide): bit-identical.
// FOLD: the scale's input is not the pyramid kernel's blurred float image but the 320 x 320 gray bytes themselves; the 3 x 3 Gaussian of
// pyramid_body<0> (BORDER_REFLECT_101, the same two float passes in the same operation order: bit-identical) is formed on the way into the
// register window -- one 4-byte load per new row instead of one float load, a rolling window of three horizontally filtered rows.  Saves the
// 320-px tiles of the pyramid kernel and 49 MB written + read per 120 frames.
template <int K, bool FOLD>
__device__ __forceinline__ void polyexp_rows(const float* __restrict__ img, const uint8_t* __restrict__ small, float* __restrict__ out, int y0,
                                             const FbConsts* __restrict__ C, pf4 (*rowb)[kPolyQuads], float (*outb)[S * 5])
{
    static_assert(!FOLD || K == 0, "only the 320-px scale forms its own blur");
    constexpr int w = S >> K, h = w, R = 1 << K, STEPS = kPolyRows / R;
    static_assert(R * (w + 10) <= kPolyQuads && h % kPolyRows == 0 && kPolyRows % R == 0, "a step's R rows fit one LDS buffer; whole bands");
    const int tid = threadIdx.x;
    const int sr = K == 0 ? 0 : tid / w, x = tid - sr * w;   // sub-row of this lane within a step, column
    const int yb = y0 + sr;                                  // this lane's row in step 0
    // FOLD: bytes x - 1, x, x + 1 of a row (reflected at the image edge) out of ONE 4-byte load at xs = clamp(x - 1, 0, w - 4)
    const int xs = x - 1 < 0 ? 0 : (x - 1 > w - 4 ? w - 4 : x - 1);
    const int shl = ((x == 0 ? 1 : x - 1) - xs) * 8, shc = (x - xs) * 8, shr = ((x == w - 1 ? w - 2 : x + 1) - xs) * 8;
    const float kx0 = C->gk[0][0], kx1 = C->gk[0][1], kx2 = C->gk[0][2];
    struct __attribute__((packed, aligned(1))) U4 { unsigned v; };
    auto hb = [&](int srow) __attribute__((always_inline)) {               // horizontally filtered value of source row reflect101(srow) at this column
        const int sr = srow < 0 ? -srow : (srow > h - 1 ? 2 * (h - 1) - srow : srow);
        const unsigned wd = reinterpret_cast<const U4*>(small + sr * w + xs)->v;
        const float l = (float)((wd >> shl) & 0xFFu), c = (float)((wd >> shc) & 0xFFu), r = (float)((wd >> shr) & 0xFFu);
        return __builtin_fmaf(c, kx1, (l + r) * kx0);
    };
    float hm = 0.f, h0 = 0.f, hp = 0.f;                      // filtered rows rcur - 1, rcur, rcur + 1
    int rcur = -1000;
    auto blurred = [&](int r) __attribute__((always_inline)) {             // value of the blurred image at (r, x), r clamped by the caller; rows only move down
        if (r != rcur) {                                     // workgroup-uniform
            if (r == rcur + 1) { hm = h0; h0 = hp; hp = hb(r + 1); }
            else { hm = hb(r - 1); h0 = hb(r); hp = hb(r + 1); }
            rcur = r;
        }
        return __builtin_fmaf(hp + hm, kx2, __builtin_fmaf(h0, kx1, 0.f));
    };
    auto pixel = [&](int r) __attribute__((always_inline)) { return FOLD ? blurred(r) : img[r * w + x]; };
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    // the kernel is VALU-bound (profiles/r03_experiments.md): the taps live in registers for all rows of the workgroup, as
    // floats and -- where cv2 multiplies a double by them -- as doubles; pairs of float products that share a factor are
    // formed as two-component vectors (v_pk_mul_f32 / v_pk_add_f32: one instruction for two IEEE operations, same results)
    float g[6], xg[6], xxg[6];
    double gd[6], xxgd[6];
#pragma unroll
    for (int q = 0; q <= 5; q++) { g[q] = C->g[5 + q]; xg[q] = C->xg[5 + q]; xxg[q] = C->xxg[5 + q]; gd[q] = C->gd[q]; xxgd[q] = C->xxgd[q]; }
    const double ig11 = C->ig11, ig03 = C->ig03, ig33 = C->ig33, ig55 = C->ig55;
    float win[11 + kPolyRows - R];                       // win[j] = row yb - 5 + j of this column (clamped: replicate border); step i reads win[R i .. R i + 10]
#pragma unroll
    for (int q = 0; q < 10; q++) win[q] = pixel(min(max(yb - 5 + q, 0), h - 1));
    pf4* rowq[2] = {rowb[0] + sr * (w + 10), rowb[1] + sr * (w + 10)};
#pragma unroll
    for (int i = 0; i < STEPS; i++) {                    // fully unrolled: the window is a static slice
        const int par = i & 1, o = R * i;
#pragma unroll
        for (int j = o + 11 - R; j <= o + 10; j++)       // the rows this step is the first to read (one in step 0: the others were loaded above)
            if (j >= 10) win[j] = pixel(min(yb - 5 + j, h - 1));
        {
            f2 t02 = f2{win[o + 5] * g[0], 0.f};
            float t1 = 0.f;
#pragma unroll
            for (int q = 1; q <= 5; q++) {
                const float a = win[o + 5 - q], bb = win[o + 5 + q];
                const float p = a + bb;
                t02 = t02 + f2{g[q], xxg[q]} * f2{p, p};  // t0 = t0 + g[q] * p;  t2 = t2 + xxg[q] * p
                t1 = t1 + xg[q] * (bb - a);
            }
            polyexp_put(rowq[par], x, w, t02.x, t1, t02.y);
        }
        __syncthreads();
        if (i > 0) {                                     // step i - 1 is complete in outb[par ^ 1]: R rows = 1600 floats = 400 16-byte pieces
            f4* dst = reinterpret_cast<f4*>(out + (int64_t)(y0 + o - R) * w * 5);
            const f4* srcv = reinterpret_cast<const f4*>(outb[par ^ 1]);
            __builtin_nontemporal_store(srcv[tid], dst + tid);
            if (tid < S * 5 / 4 - 320) __builtin_nontemporal_store(srcv[tid + 320], dst + tid + 320);
        }
        polyexp_hpass(rowq[par] + x + 5, g, xg, gd, xxgd, ig11, ig03, ig33, ig55, outb[par] + tid * 5);   // (sub-row, x) order = memory order
    }
    __syncthreads();
    {
        f4* dst = reinterpret_cast<f4*>(out + (int64_t)(y0 + kPolyRows - R) * w * 5);
        const f4* srcv = reinterpret_cast<const f4*>(outb[(STEPS - 1) & 1]);
        __builtin_nontemporal_store(srcv[tid], dst + tid);
        if (tid < S * 5 / 4 - 320) __builtin_nontemporal_store(srcv[tid + 320], dst + tid + 320);
    }
}

__global__ __launch_bounds__(320) void k_polyexp_all(PolyPtrs P, int n, const FbConsts* __restrict__ C)
{
    __shared__ pf4 rowb[2][kPolyQuads];                  // per sub-row: w + 10 quads (5 replicated on either side); two buffers
    __shared__ __align__(16) float outbb[2][S * 5];
    pf4* row = rowb[0];                                  // the one-row form: eight sub-rows of w + 10 quads, 400 of the 720
    static_assert(8 * (S / 8 + 10) <= 2 * kPolyQuads, "the eight sub-rows of the coarsest scale fit");
    float* outb = outbb[0];
    // scale k: n * poly_wgs(k) workgroups, padded to a multiple of 8: within a scale consecutive workgroups -- row bands of a frame, whose
    // 11-row windows overlap -- share an XCD
    int b = (int)blockIdx.x, k = 0, wgs = 0;
    for (; k < AVD_FB_LEVELS; k++) {
        wgs = n * poly_wgs(k);
        const int cnt = ((wgs + 7) >> 3) << 3;
        if (b < cnt) break;
        b -= cnt;
    }
    if (k >= AVD_FB_LEVELS) return;
    const int per = (wgs + 7) >> 3, lid = (b & 7) * per + (b >> 3);
    if (lid >= wgs) return;
    const int w = S >> k, h = w;
    int f = 0;
#pragma unroll
    for (int kk = 0; kk < AVD_FB_LEVELS; kk++)
        if (k == kk) f = lid / poly_wgs(kk);             // (divisions by constants)
    const int t = lid - f * poly_wgs(k);
    float* R = P.R[k] + (int64_t)f * w * h * 5;
    if (k == 0) {
        if (P.small) polyexp_rows<0, true>(nullptr, P.small + (int64_t)f * S * S, R, t * kPolyRows, C, rowb, outbb);
        else polyexp_rows<0, false>(P.I[0] + (int64_t)f * S * S, nullptr, R, t * kPolyRows, C, rowb, outbb);
        return;
    }
    if (k == 1) { polyexp_rows<1, false>(P.I[1] + (int64_t)f * w * h, nullptr, R, t * kPolyRows, C, rowb, outbb); return; }
    if (k == 2) { polyexp_rows<2, false>(P.I[2] + (int64_t)f * w * h, nullptr, R, t * kPolyRows, C, rowb, outbb); return; }
    const int y0 = t << k;
    const int tid = threadIdx.x;
    const int sr = tid / w, x = tid - sr * w;            // sub-row of this lane, column
    const int y = y0 + sr;
    const float* img = P.I[k] + (int64_t)f * w * h;
    float g[6], xg[6], xxg[6];                            // uniform: scalar registers, as are the taps as doubles
    double gd[6], xxgd[6];
#pragma unroll
    for (int q = 0; q <= 5; q++) { g[q] = C->g[5 + q]; xg[q] = C->xg[5 + q]; xxg[q] = C->xxg[5 + q]; gd[q] = C->gd[q]; xxgd[q] = C->xxgd[q]; }
    pf4* rowq = row + sr * (w + 10);
    {
        float t0 = img[y * w + x] * g[0], t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int q = 1; q <= 5; q++) {
            const float a = img[max(y - q, 0) * w + x], bb = img[min(y + q, h - 1) * w + x];
            const float p = a + bb;
            t0 = t0 + g[q] * p;
            t1 = t1 + xg[q] * (bb - a);
            t2 = t2 + xxg[q] * p;
        }
        polyexp_put(rowq, x, w, t0, t1, t2);
    }
    __syncthreads();
    polyexp_hpass(rowq + x + 5, g, xg, gd, xxgd, C->ig11, C->ig03, C->ig33, C->ig55, outb + tid * 5);   // (sub-row, x) order = memory order of the workgroup's rows
    __syncthreads();
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4* dst = reinterpret_cast<f4*>(R + (int64_t)y0 * w * 5);
    const f4* srcv = reinterpret_cast<const f4*>(outb);
    __builtin_nontemporal_store(srcv[tid], dst + tid);
    if (tid < S * 5 / 4 - 320) __builtin_nontemporal_store(srcv[tid + 320], dst + tid + 320);
}

// ---------------------------------------------------------------------------------------
// Initial flow of a level: zeros at the coarsest level, otherwise the previous level's
// flow resized x2 (INTER_LINEAR, float weights, cv2 edge rules) and multiplied by 2.
// flow planes: [pair][2][h][w].  The destination is exactly 2x the source, so cv2's source
// coordinate (d+0.5)*0.5-0.5 = d/2 - 0.25 is exact in float: s = floor, f in {0.75, 0.25};
// horizontally the weights snap to the edge pixel (f = 0) when s falls outside [0, pw-1),
// vertically the rows are clipped and the weights kept.  A lane produces 4 consecutive outputs.
// ---------------------------------------------------------------------------------------
// LERP (bit 16 of option "cv2_model"): a + (b - a) * f in both directions instead of a * (1 - f) + b * f; a copied edge value stays a copy
template <int W, bool LERP = false>
__global__ __launch_bounds__(256) void k_flow_up(const float* __restrict__ prev, float* __restrict__ flow, int npairs, const int* __restrict__ plist)
{
    constexpr int H = W, PW = W / 2, PH = H / 2, Q = W / 4;
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= npairs * 2 * H * Q) return;
    const int q = gid % Q;
    const int dy = (gid / Q) % H;
    int pc = gid / (Q * H);                                // pair*2 + channel
    if (plist) pc = plist[pc >> 1] * 2 + (pc & 1);         // plist (may be null): the launch works on pairs plist[0 .. npairs) (exact re-run of flagged pairs)
    const float* src = prev + (int64_t)pc * PW * PH;
    float fy = dy * 0.5f - 0.25f;
    const int sy = floor_f(fy);
    fy -= sy;
    const float* r0 = src + clampi(sy, 0, PH - 1) * PW;
    const float* r1 = src + clampi(sy + 1, 0, PH - 1) * PW;
    const float b0 = 1.f - fy, b1 = fy;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int dx = q * 4 + i;
        float fx = dx * 0.5f - 0.25f;
        int sx = floor_f(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        bool edge = false;                                  // dx >= xmax: value copied, no weights
        if (sx + 1 >= PW) { edge = true; if (sx >= PW - 1) { fx = 0; sx = PW - 1; } }
        const int x1 = min(sx + 1, PW - 1);
        const float a0 = 1.f - fx, a1 = fx;
        float d0, d1;
        if (edge) { d0 = r0[sx] * 1.f; d1 = r1[sx] * 1.f; }
        else if constexpr (LERP) { d0 = r0[sx] + (r0[x1] - r0[sx]) * a1; d1 = r1[sx] + (r1[x1] - r1[sx]) * a1; }
        else { d0 = r0[sx] * a0 + r0[x1] * a1; d1 = r1[sx] * a0 + r1[x1] * a1; }
        if constexpr (LERP) o[i] = (d0 + (d1 - d0) * b1) * 2.f;
        else o[i] = (d0 * b0 + d1 * b1) * 2.f;
    }
    *reinterpret_cast<float4*>(flow + ((int64_t)pc * H + dy) * W + q * 4) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------------------
// Flow statistics in numpy's float32 order (video.py:46-48): mag = sqrt(fx*fx + fy*fy);
// add.reduce = pairwise sums (128-element leaves, 8 strided accumulators) inside 8192-element
// iterator buffers whose results are added sequentially.  One workgroup per pair.
// ---------------------------------------------------------------------------------------
constexpr int kChunk = 8192;
constexpr int kNChunk = (AVD_NPIX + kChunk - 1) / kChunk;      // 13: twelve full buffers + one of 4096

// sequential combination of the per-buffer sums, as the ufunc reduction loop does
__device__ __forceinline__ float chunk_total(const float* part)
{
    float t = part[0];
#pragma unroll
    for (int i = 1; i < kNChunk; i++) t += part[i];
    return t;
}

// Both statistics of a pair in ONE workgroup of 512 threads, the pair's 102 400 magnitudes in REGISTERS (200 per thread):
// thread (leaf l = tid / 8, accumulator a = tid % 8) holds, for each of the 13 iterator buffers, the 16 elements
// l * 128 + a + 8 k that numpy's unrolled leaf loop adds into accumulator a.  A buffer's sum is then: the sequential
// 16-element sum per thread, the 8-accumulator tree ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the balanced tree over the
// buffer's 64 (last buffer: 32) leaves -- shuffles inside a wave (8 leaves), eight per-wave values through LDS.  The
// second pass, (mag - mean)^2 with mean = sum / N in float32, runs on the registers: the magnitudes are read once.
// (18.6 us for 119 pairs; a variant with 16-byte loads and the 16-element sum relayed over four lanes took 22.9 us.)
// mag[pair][N] = |flow|: written by the last launch of the fast level kernel, or by k_mag below from the two flow planes
__global__ __launch_bounds__(512) void k_stats_pair(const float* __restrict__ mag, float* __restrict__ stats, const int* __restrict__ plist)
{
    __shared__ float wpart[kNChunk][8];
    __shared__ float ctot[kNChunk];
    const int p = plist ? plist[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const int l = tid >> 3, wave = tid >> 6;
    const bool in_last = l < ((AVD_NPIX - (kNChunk - 1) * kChunk) >> 7);          // the last buffer has 32 leaves
    const float* src = mag + (int64_t)p * AVD_NPIX + l * 128 + (tid & 7);
    float v[kNChunk][16];
#pragma unroll
    for (int c = 0; c < kNChunk; c++)
#pragma unroll
        for (int k = 0; k < 16; k++) v[c][k] = (c < kNChunk - 1 || in_last) ? src[c * kChunk + 8 * k] : 0.f;
    float total[2];
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
#pragma unroll
        for (int c = 0; c < kNChunk; c++) {
            float r = v[c][0];
#pragma unroll
            for (int k = 1; k < 16; k++) r += v[c][k];
            // lanes whose partner holds no valid subtree compute values nobody reads
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) r = r + __shfl_down(r, d);
            if ((tid & 63) == 0) wpart[c][wave] = r;
        }
        __syncthreads();
        if (tid < kNChunk) {
            const float* w = wpart[tid];
            ctot[tid] = tid < kNChunk - 1 ? ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7])) : (w[0] + w[1]) + (w[2] + w[3]);
        }
        __syncthreads();
        total[pass] = chunk_total(ctot);
        if (pass == 0) {
            const float mean32 = total[0] / (float)AVD_NPIX;                       // _var: f32 true_divide
#pragma unroll
            for (int c = 0; c < kNChunk; c++)
#pragma unroll
                for (int k = 0; k < 16; k++) { const float d = v[c][k] - mean32; v[c][k] = d * d; }
            __syncthreads();                                                       // ctot / wpart are rewritten by the second pass
        }
    }
    // stats[pair] = { f32(f64(sum)/N), f32(f64(sumsq)/N) }   (_mean / _var final scalar divides)
    if (tid == 0) {
        stats[2 * p] = (float)((double)total[0] / (double)AVD_NPIX);
        stats[2 * p + 1] = (float)((double)total[1] / (double)AVD_NPIX);
    }
}

// mag = np.sqrt(fx * fx + fy * fy) in float32 (video.py:46) from the planar flow [pair][2][N]: the exact-mode level kernels
// leave the flow only, the fast one writes the magnitudes itself
__global__ void k_mag(const float* __restrict__ flow, float* __restrict__ mag, int64_t total4, const int* __restrict__ plist)
{
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total4) return;
    const int64_t ps = gid / (AVD_NPIX / 4), i = gid - ps * (AVD_NPIX / 4);
    const int64_t p = plist ? plist[ps] : ps;
    const float4 fx = reinterpret_cast<const float4*>(flow + p * 2 * AVD_NPIX)[i], fy = reinterpret_cast<const float4*>(flow + (p * 2 + 1) * AVD_NPIX)[i];
    float4 m;
    m.x = sqrtf(fx.x * fx.x + fy.x * fy.x);
    m.y = sqrtf(fx.y * fx.y + fy.y * fy.y);
    m.z = sqrtf(fx.z * fx.z + fy.z * fy.z);
    m.w = sqrtf(fx.w * fx.w + fy.w * fy.w);
    reinterpret_cast<float4*>(mag + p * AVD_NPIX)[i] = m;
}

// planar flow [pair][2][N] -> cv2's interleaved [pair][N][2] (only when the caller asks for the flow)
__global__ void k_flow_interleave(const float* __restrict__ flow, float* __restrict__ out, int64_t total)
{
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int64_t p = gid / AVD_NPIX, i = gid - p * AVD_NPIX;
    out[gid * 2] = flow[p * 2 * AVD_NPIX + i];
    out[gid * 2 + 1] = flow[(p * 2 + 1) * AVD_NPIX + i];
}

template <typename... A>
inline void launch1d(void (*k)(A...), int64_t items, int block, hipStream_t s, A... args)
{
    const int grid = (int)((items + block - 1) / block);
    if (grid > 0) hipLaunchKernelGGL(k, dim3(grid), dim3(block), 0, s, args...);
}

constexpr int kLevelId[AVD_FB_LEVELS] = {AVD_K_LEVEL320, AVD_K_LEVEL160, AVD_K_LEVEL80, AVD_K_LEVEL40};     // avd_kernel_ms regions of the first pass, by level
constexpr int kFlowUpId[AVD_FB_LEVELS - 1] = {AVD_K_FLOWUP320, AVD_K_FLOWUP160, AVD_K_FLOWUP80};

// Gaussian pyramid + polynomial expansion of n frames at all four scales: two launches
void pyramid_and_polyexp(avd_ctx* ctx, const FlowCall& call, const uint8_t* d_small, int n)
{
    Workspace& ws = ctx->ws;
    const FbConsts* C = ctx->d_fbc;
    // ctx->fb_fold_blur (default 1): the 320-px scale's 3 x 3 blur is formed inside the polynomial expansion; the pyramid kernel then has no
    // 320-px tiles and d_pyr[0] is not written (avd_debug_copy "pyr0" is meaningful with the option off only).  Under bit 1 of "cv2_model" the
    // blur is never folded (fb_fold_blur_eff): the mul + add taps exist in the pyramid kernel only
    const bool fold = fb_fold_blur_eff(ctx->fb_fold_blur, call.model) != 0;
    const int wgs = n * ((fold ? 0 : PyrGeo<0>::TILES) + PyrGeo<1>::TILES + PyrGeo<2>::TILES + PyrGeo<3>::TILES);
    kmark(ctx, AVD_K_PYRAMID);
    auto pyramid = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(wgs), dim3(256), 0, ctx->stream, d_small, n, C, fold ? nullptr : ws.d_pyr[0].p, ws.d_pyr[1].p, ws.d_pyr[2].p,
                           ws.d_pyr[3].p, ws.d_fbflags.p, ws.d_pairdiff.p);
    };
    switch (call.model & (kCv2GaussMuladd | kCv2ResizeLerp)) {
    case 0: pyramid(k_pyramid_all); break;                 // the default model: the launch of always
    case kCv2GaussMuladd: pyramid(k_pyramid_model<true, false>); break;
    case kCv2ResizeLerp: pyramid(k_pyramid_model<false, true>); break;
    default: pyramid(k_pyramid_model<true, true>); break;
    }
    PolyPtrs P;
    P.small = fold ? d_small : nullptr;
    int grid = 0;
    for (int k = 0; k < AVD_FB_LEVELS; k++) {
        P.I[k] = ws.d_pyr[k]; P.R[k] = ws.d_poly[k];
        grid += ((n * poly_wgs(k) + 7) >> 3) << 3;
    }
    kmark(ctx, AVD_K_POLYEXP);
    hipLaunchKernelGGL(k_polyexp_all, dim3(grid), dim3(320), 0, ctx->stream, P, n, C);
}

// initial flow of level k = 0 .. 2 from the coarser level's final flow (no launch for any other k); plist (may be null): for the pairs plist[0 .. np) only
// lerp: bit 16 of the call's "cv2_model"
void flow_up_level(hipStream_t stream, int k, const float* prev, float* flow, int np, const int* plist, bool lerp)
{
    fb_dispatch_width(S >> k, [&](auto wc) {
        constexpr int W = decltype(wc)::value;
        if constexpr (W > S / 8) {
            if (lerp) launch1d(k_flow_up<W, true>, (int64_t)np * 2 * W * (W / 4), 256, stream, prev, flow, np, plist);
            else launch1d(k_flow_up<W>, (int64_t)np * 2 * W * (W / 4), 256, stream, prev, flow, np, plist);
        }
    });
}

// Levels 3 -> 0 with the EXACT kernels (bit-identical to the oracle), a level's three iterations in place in its flow buffer: the fused kernel
// (avd_fbfused.hip) where bit k of fused_mask is set, else the two-kernel path (avd_fbtwo.hip) through `scratch`.  plist == null: exact mode, all np
// pairs of the chunk; plist != null: the re-run of the flagged pairs plist[0 .. np).  The two differ in four things, (1) .. (4), and in nothing else.
// chunk: exact mode fills in where it leaves each level's flow; the re-run reads where the fast kernels left the 320-px one.
// call.model ("cv2_model"): under bit 8 the levels are 2 -> 0 -- the 80-px level is the coarsest and starts from zero flow; bit 16 selects k_flow_up's lerp form.
int exact_levels(avd_ctx* ctx, const FlowCall& call, int np, int fused_mask, FbTwoScratch scratch, const int* plist, FbChunk& chunk)
{
    const int top = fb_coarsest(call.model);
    const bool lerp = (call.model & kCv2ResizeLerp) != 0;
    Workspace& ws = ctx->ws;
    const hipStream_t stream = ctx->stream;
    const bool rerun = plist != nullptr;
    // (1) level 0 works in its first flow buffer; the re-run in the one the fast kernels left their final flow in (the caller may read it back)
    float* const flow0 = rerun ? const_cast<float*>(chunk.flow[0]) : ws.d_flow[0].p;
    if (rerun) kmark(ctx, AVD_K_RERUN);                  // (3) avd_kernel_ms: exact mode records the per-level regions, the re-run is one region
    for (int k = top; k >= 0; k--) {
        const int w = S >> k;
        const bool coarsest = k == top, fused = (fused_mask >> k) & 1;
        float* flow = k == 0 ? flow0 : ws.d_flow[k].p;
        if (coarsest) {
            // (2) zero initial flow: the fused kernel is told so; the two-kernel path reads a buffer that only exact mode may clear
            if (!fused && rerun) { ctx->err = "exact re-run: the coarsest level runs the fused kernel (it needs no cleared flow)"; return AVD_ERR_ARG; }
            if (!fused) HIP_TRY(ctx, hipMemsetAsync(flow, 0, sizeof(float) * 2 * w * w * np, stream));
        } else {
            if (!rerun) kmark(ctx, kFlowUpId[k]);
            flow_up_level(stream, k, ws.d_flow[k + 1], flow, np, plist, lerp);
        }
        if (!rerun) { chunk.flow[k] = flow; kmark(ctx, kLevelId[k]); }
        const bool marks = !rerun && k == 0;             // (4) the events of avd_stage_ms 4 / 5 belong to the 320-px level of exact mode
        if (fused) {
            level320_mark(ctx, marks);
            if (int e = launch_fb_level(ctx, stream, w, ws.d_poly[k], flow, np, 3, coarsest, plist)) return e;
            level320_mark(ctx, marks);
        } else {
            for (int it = 0; it < 3; it++)
                if (int e = launch_fb_two(ctx, stream, w, ws.d_poly[k], flow, scratch, np, plist, marks)) return e;
        }
    }
    return 0;
}

// Levels 3 -> 0 with the fast level kernel (avd_fbfast.hip), fb_mode = 1: three iterations per level, the flow ping-pongs between the level's two
// buffers (a = initial flow, results b, a, b), the last launch writes |flow| to d_mag; ctx->fb_fold_up and ctx->fb_fold_up160 (avd_internal.h) say what the
// launches fold in.
// Pairs the kernels flag as ill-posed are re-run by the exact kernels once the HOST has seen the flags (launch_farneback_rerun).
int fast_levels(avd_ctx* ctx, const FlowCall& call, int np, FbChunk& chunk)
{
    Workspace& ws = ctx->ws;
    const hipStream_t stream = ctx->stream;
    // under bit 16 of the call's "cv2_model" no launch resizes a flow itself (fb_fold_up_eff): the lerp form exists in k_flow_up only
    const int fold = fb_fold_up_eff(ctx->fb_fold_up, call.model), top = fb_coarsest(call.model);
    const bool fold160 = fb_fold_up160_eff(ctx->fb_fold_up160, call.model) != 0, lerp = (call.model & kCv2ResizeLerp) != 0;
    int* flags = ctx->fb_rerun ? ws.d_fbflags.p : nullptr;
    const int* pairdiff = ctx->fb_rerun ? ws.d_pairdiff.p : nullptr;
    for (int k = top; k >= 0; k--) {
        const int w = S >> k;
        const bool coarsest = k == top, three = (k == 2 || k == 3) && (fold & 4);
        float *a = ws.d_flow[k], *b = ws.d_flow2[k];
        // the initial flow: zero at the coarsest level, else the coarser level's final flow, resized by the first launch itself or by k_flow_up into a
        const float* prev = coarsest ? nullptr : chunk.flow[k + 1];
        // (160 px: the chain wave resizes in the one-strip shape only, which the call has chosen or not before it got here)
        const bool chain = (k == 0 && (fold & 1)) || (k == 1 && fold160 && call.wide160);
        // the kernel's zero form is compiled for the 40-px level only: an 80-px coarsest level (bit 8) reads a cleared buffer, the same arithmetic.
        // That form also exempts its iteration from the border-sign criterion (a zero initial flow is structural in cv2 too, and "inside" in both);
        // without the exemption nearly every pair is flagged there.  The cleared level gets it through the kernel's other exemption, the one for
        // bit-identical frames: its first iteration runs as a launch of its own (fb_fold_up_eff drops bit 4) and is handed pair-identity words that
        // are all zero -- the cleared flow buffer itself, which that launch only reads (2 w w >= kPairDiffTiles words per pair).  The solver's
        // criterion does not read those words and stays.
        const bool cleared = coarsest && k != AVD_FB_LEVELS - 1;
        static_assert(2 * (S >> (AVD_FB_LEVELS - 2)) * (S >> (AVD_FB_LEVELS - 2)) >= kPairDiffTiles, "the cleared flow serves as the identity words");
        if (cleared) HIP_TRY(ctx, hipMemsetAsync(a, 0, sizeof(float) * 2 * w * w * np, stream));
        const FbFlowFrom from = cleared ? FbFlowFrom::level : coarsest ? FbFlowFrom::zero : chain ? FbFlowFrom::chain
                                : ((k == 1 || k == 2) && (fold & 2)) ? FbFlowFrom::prologue : FbFlowFrom::level;
        if (from == FbFlowFrom::level && !coarsest) {
            kmark(ctx, kFlowUpId[k]);
            flow_up_level(stream, k, prev, a, np, nullptr, lerp);
        }
        const bool from_prev = from == FbFlowFrom::chain || from == FbFlowFrom::prologue;
        kmark(ctx, kLevelId[k]);
        level320_mark(ctx, k == 0);
        if (three) {                                     // (prologue: prev -> a,) a -> b -> a -> b
            const FbFastLaunch L{call.wide160, false, 3, from, from_prev ? prev : a, b, a, nullptr, flags, pairdiff};
            if (int e = launch_fb_fast(ctx, stream, w, ws.d_poly[k], L, np)) return e;
            a = b;
        } else {
            for (int it = 0; it < 3; it++) {
                float* mag = (k == 0 && it == 2) ? ws.d_mag.p : nullptr;
                const int* identity = cleared && it == 0 && pairdiff ? reinterpret_cast<const int*>(a) : pairdiff;
                // the level's last launch: nothing on the device reads the 320-px flow itself -- the statistics read |flow| (d_mag), the exact
                // re-run writes its pairs' flow without reading it -- unless the call interleaves it for its caller (flow_tail).  The one reader
                // after the call, avd_debug_fetch "flow0", has the launch repeated with the stores (launch_flow0_late)
                const bool unread = mag && !call.dense_flow;
                // 320 px: a launch may run a pair as one five-block workgroup (FlowCall::wide320): those that read a flow of their own size, and -- where
                // fb_wide320_up allows it -- the resizing first launch, whose normal-equation waves then resize the 160-px flow themselves (avd_fbfast.hip, UpN)
                const FbFlowFrom from_it = it == 0 ? from : FbFlowFrom::level;
                const bool wide320_up = k == 0 && call.wide320 && from_it == FbFlowFrom::chain && ctx->fb_wide320_up != 0;
                const bool wide320 = (k == 0 && call.wide320 && from_it == FbFlowFrom::level) || wide320_up;
                if (wide320_up) ctx->fb_wide320_up_launches++;
                else if (wide320) ctx->fb_wide320_launches++;
                const FbFastLaunch L{call.wide160, wide320, 1, from_it, it == 0 && from_prev ? prev : a, b, a, mag, flags, identity, !unread};
                if (int e = launch_fb_fast(ctx, stream, w, ws.d_poly[k], L, np)) return e;
                if (unread) { chunk.flow0_late.pairs = np; chunk.flow0_late.flow_in = a; chunk.flow0_late.flags = flags; chunk.flow0_late.pairdiff = pairdiff; }
                float* t = a; a = b; b = t;
            }
        }
        level320_mark(ctx, k == 0);
        chunk.flow[k] = a;                             // the buffer written last
    }
    return 0;
}

// What follows the levels: |flow| (with_mag; the fast kernels write it themselves) and the two statistics of m pairs -- plist[0 .. m), or the first m
// with plist null -- and, when the call wants the dense flow (tests / debugging), cv2's interleaved layout of the whole chunk (np_chunk pairs).
void flow_tail(avd_ctx* ctx, const FlowCall& call, const float* flow, bool with_mag, int m, const int* plist, int np_chunk)
{
    Workspace& ws = ctx->ws;
    const hipStream_t stream = ctx->stream;
    if (with_mag) launch1d(k_mag, (int64_t)m * (AVD_NPIX / 4), 256, stream, flow, ws.d_mag.p, (int64_t)m * (AVD_NPIX / 4), plist);
    hipLaunchKernelGGL(k_stats_pair, dim3(m), dim3(512), 0, stream, (const float*)ws.d_mag, ws.d_stats.p, plist);
    if (call.dense_flow && ws.d_flow_il)
        launch1d(k_flow_interleave, (int64_t)np_chunk * AVD_NPIX, 256, stream, flow, ws.d_flow_il.p, (int64_t)np_chunk * AVD_NPIX);
}

}  // namespace

// All pairs (f, f+1), f in [0, n-1), of n resident 320x320 frames (one chunk), on the context's stream, into the Farneback scratch
int launch_farneback(avd_ctx* ctx, const FlowCall& call, const uint8_t* d_small, int n, FbChunk* left)
{
    if (n < 2) return 0;
    Workspace& ws = ctx->ws;
    if (ctx->profiling) ctx->kern_ev_used = 0;
    const bool fast = ctx->fb_mode == 1;
    FbChunk& chunk = ws.fb_holds;                      // level by level: a launch sequence that fails half way has overwritten those levels
    chunk.mag_valid = fast;
    chunk.flow0_late = {};
    pyramid_and_polyexp(ctx, call, d_small, n);
    if (int e = fast ? fast_levels(ctx, call, n - 1, chunk) : exact_levels(ctx, call, n - 1, ctx->fb_fused, {ws.d_vs, ws.d_vs0}, nullptr, chunk)) return e;
    HIP_TRY(ctx, hipGetLastError());
    *left = chunk;
    return 0;
}

// Exact re-run (fast mode) of the m pairs h_list[0 .. m) of the chunk the workspace still holds (polynomial expansions of all its frames): the four
// levels with the exact kernels from a compacted pair list, then |flow| and the two statistics of those pairs, where the record kernel reads
// them.  The HOST calls this after it has seen the chunk's flag words (avd_capi.hip): nothing is launched for a chunk without flagged pairs, and the
// work is sized by their number -- up to kRerunTwoKernelMax pairs the 160- / 320-px levels run the two-kernel path (a pair spread over seven strips /
// 64-row bands: ~0.15 ms per level for one pair, where the fused kernel's single workgroup per pair takes 0.23 / 0.83 ms however few pairs there are),
// beyond that the fused kernels (one workgroup per pair = the exact mode's own launches, its time for a clip of nothing but flagged pairs).
// ctx->fb_rerun_fused (tuning / tests): level mask of the fused kernel for the few-pairs case, default 0xC (40 and 80 px).
int launch_farneback_rerun(avd_ctx* ctx, const FlowCall& call, const int* h_list, int m, int np_chunk)
{
    if (m <= 0) return 0;
    Workspace& ws = ctx->ws;
    if (m > ws.fb_cap) { ctx->err = "re-run list longer than the chunk"; return AVD_ERR_ARG; }
    if (int e = ws.d_rlist.reserve(ctx, (size_t)ws.fb_cap)) return e;
    // the coarsest level runs the fused kernel, which needs no cleared flow: bit 3 of the option is always set, and under bit 8 of "cv2_model" bit 2 is taken as set
    const int fused_mask = m <= kRerunTwoKernelMax ? ((ctx->fb_rerun_fused & 0xF) | (1 << fb_coarsest(call.model))) : 0xF;
    if (fused_mask != 0xF) {
        const FbTwoScratchSize sz = fb_two_scratch_size(kRerunTwoKernelMax);
        if (int e = ws.d_vs0_rerun.reserve(ctx, sz.vs0)) return e;
        if (int e = ws.d_vs_rerun.reserve(ctx, sz.vs)) return e;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ws.d_rlist, h_list, sizeof(int) * m, hipMemcpyHostToDevice, ctx->stream));
    if (int e = exact_levels(ctx, call, m, fused_mask, {ws.d_vs_rerun, ws.d_vs0_rerun}, ws.d_rlist, ws.fb_holds)) return e;   // the scratch is indexed by position in the list
    flow_tail(ctx, call, ws.fb_holds.flow[0], true, m, ws.d_rlist, np_chunk);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// The 320-px level's last launch once more, this time storing the flow (not |flow|: d_mag has it, and the re-run's pairs have theirs there).  Its
// inputs are all still in the scratch: the polynomial expansions, the flow of the second iteration, the identity words, and the flag words as
// the call left them -- a flagged pair is skipped by every workgroup, so the flow the exact re-run wrote for it stays; the others are computed
// exactly as the first time (the launch is deterministic), so no new flag can rise.
int launch_flow0_late(avd_ctx* ctx)
{
    Workspace& ws = ctx->ws;
    FbChunk& chunk = ws.fb_holds;
    if (chunk.flow0_late.pairs <= 0) return 0;
    const auto late = chunk.flow0_late;
    float* out = const_cast<float*>(chunk.flow[0]);
    const FbFastLaunch L{false, false, 1, FbFlowFrom::level, late.flow_in, out, const_cast<float*>(late.flow_in), nullptr, late.flags, late.pairdiff};
    if (int e = launch_fb_fast(ctx, ctx->stream, S, ws.d_poly[0], L, late.pairs)) return e;
    HIP_TRY(ctx, hipGetLastError());
    chunk.flow0_late = {};
    return 0;
}

int launch_flow_stats(avd_ctx* ctx, const FlowCall& call, const FbChunk& chunk, int n)
{
    if (n < 2) return 0;
    kmark(ctx, AVD_K_STATS);
    flow_tail(ctx, call, chunk.flow[0], !chunk.mag_valid, n - 1, nullptr, n - 1);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
