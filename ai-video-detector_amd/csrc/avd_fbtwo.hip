// avd_fbtwo.hip -- FarnebackUpdateFlow_Blur (winsize 15) as TWO kernels per iteration that exchange the exact double intermediate
// D = vsum(x+7) - vsum(x-8) through HBM (gfx950).  The first exact implementation of a level, bit-identical to oracle/avd_oracle.c like the
// fused kernel (avd_fbfused.hip) that replaced it.  Today a fallback: levels whose bit is clear in "fb_fused" (exact mode), and the 160- /
// 320-px levels of the exact re-run of <= kRerunTwoKernelMax flagged pairs, where a pair spread over seven strips and 64-row bands finishes
// sooner than the fused kernel's one workgroup per pair.  Called by exact_levels (avd_farneback.hip).  Layouts follow the access pattern of
// their consumer: R interleaved [y][x][5] (bilinear gathers read 10 consecutive floats), flow planar, D tiled + XOR-swizzled.
#include "avd_internal.h"
#include "avd_fb_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int S = AVD_SMALL;

// ---------------------------------------------------------------------------------------
// FarnebackUpdateFlow_Blur, winsize 15 (m = 7).  cv2 keeps RUNNING box sums in double and
// rounds at every slide, so the value at (y,x) depends on the whole column / row prefix; the
// chains are reproduced literally, one lane per chain, in two kernels:
//
// k_uv / k_uvp (lanes along x, sequential in y; defined further down): FarnebackUpdateMatrices fused with
//   the vertical running sums vsum in double.  The horizontal pass only ever needs
//   D(x) = vsum(x+7) - vsum(x-8), which is formed there (a strip owns 48 output columns + 8/8 halo
//   lanes, clamped at the edge = cv2's replicate border) and is the only thing written (+ columns
//   0..6 of vsum for the row init).  D is stored in 64-row x 8-column tiles (4 KiB, one tile per
//   channel), the unit k_hscan stages through LDS; inside a tile the 8 doubles of a row are
//   XOR-swizzled by (row & 7) so that lanes reading "their" row spread over the LDS banks.  8
//   consecutive lanes write one 64-byte half line.  In both kernels the waves that LOAD never STORE
//   (one in-order vmcnt for both on this hardware) and their steps have no branches around memory
//   operations (a conditional load or store makes every later s_waitcnt conservative).
//
// k_hscan (lanes along y, sequential in x): five horizontal running sums per row in one lane,
//   2x2 solve per pixel.  Workgroup = 64 rows: wave 0 scans, wave 1 streams the next chunks'
//   five tiles (20 KiB each, perfectly coalesced, two chunks in flight in registers) into the other
//   LDS buffer; the flow leaves through a 10 KiB LDS transpose so that a store instruction writes 64
//   contiguous bytes per row instead of 16.  50 KiB of LDS per workgroup = 3 workgroups per CU, so a
//   whole clip's row blocks (595 at 320 px) are resident in one round.
// ---------------------------------------------------------------------------------------
constexpr int kStripW = 48;          // output columns per wave in k_uv: 64 lanes - 8 - 8 halo
constexpr int kBoxM = 7;             // (winsize - 1) / 2

__host__ __device__ constexpr int strips_of(int w) { return (w + kStripW - 1) / kStripW; }
__host__ __device__ constexpr int d16_xch(int w) { return (w + 7) / 8; }
__host__ __device__ constexpr int d16_nyb(int h) { return (h + 63) / 64; }
// tiles per pair, padded to an ODD count: an unpadded 320x320 pair is exactly 4 MiB, and a power-of-two
// stride between the pairs that all workgroups touch in lock step lands on the same HBM channels
__host__ __device__ constexpr int d16_pair_tiles(int w) { return (d16_nyb(w) * 5 * d16_xch(w)) | 1; }
// The D16 layout: where D(y, x) of channel c of scratch slot ps lives, in doubles.  Tiles of 64 rows x 8 columns (512 doubles) in the
// order [pair][row block][channel][column chunk]; the 8 doubles of a tile row are XOR-swizzled by (row & 7).  (ps, 0, 0, 0) is where
// the tiles of slot ps begin, so d16_index(w, np, 0, 0, 0) is the size for np pairs.
__host__ __device__ constexpr unsigned d16_slot(int row, int col) { return (unsigned)(row * 8 + (col ^ (row & 7))); }
template <typename I>
__host__ __device__ constexpr I d16_index(int w, I ps, int y, int c, int x)
{
    return (ps * (I)d16_pair_tiles(w) + (I)(((y >> 6) * 5 + c) * d16_xch(w) + (x >> 3))) * 512 + d16_slot(y & 63, x & 7);
}
// columns 0..6 of vsum (the row initialisation of the horizontal pass), [pair][channel][y][8]
template <typename I>
__host__ __device__ constexpr I vs0_index(int h, I ps, int c, int y) { return ((ps * 5 + (I)c) * (I)h + (I)y) * 8; }

// The strip of a workgroup of k_uvp / k_uv.  Workgroups are dealt round-robin to the 8 XCDs.  The strips of a pair share their halo
// columns and the gathered R1 rows, and pair p+1 reads as R0 the frame that pair p gathers as R1, at about the same rows at about the
// same time: so an XCD (one L2) gets all strips of a CONTIGUOUS run of pairs.  The grid is 8 * ceil(np / 8) * strips, so some blocks
// are idle: ps < 0, the whole workgroup leaves.
struct Strip {
    int ps, p;       // ps indexes the scratch (D, vsum columns), p the pair's R and flow
    int strip, xl;   // xl: logical column of this lane
    int x;           // clamped: edge replicate = duplicate chain
};
// No early return in here (the only condition guards the pair-list load of an idle block, which would be out of bounds): with
// "if (idle) return" inside, every kernel takes two or three registers more (k_uvp<160, 12>: 108, above the 106 it had with the decode
// written out in the kernel).
template <int W>
__device__ __forceinline__ Strip strip_decode(int npairs, const int* plist, int lane)
{
    constexpr int NSTRIP = strips_of(W);
    const int sj = blockIdx.x >> 3, ppx = (npairs + 7) >> 3;
    const int ps = (blockIdx.x & 7) * ppx + sj / NSTRIP, strip = sj % NSTRIP;
    const bool idle = sj / NSTRIP >= ppx || ps >= npairs;
    const int xl = strip * kStripW - 8 + lane;
    return {idle ? -1 : ps, plist && !idle ? plist[ps] : ps, strip, xl, clampi(xl, 0, W - 1)};
}

// The store part of a strip (k_uvp's storer wave, k_uv's store wave): from a vsum row published in LDS ([channel][lane]) it forms
// D = vsum(x+7) - vsum(x-8) and writes it into the tiles, and the strip that holds them writes columns 0..6 of vsum.
template <int W>
struct StripStore {
    bool writer, head;
    int x, lhi, llo;
    unsigned ps, vcol;
    __device__ __forceinline__ StripStore(const Strip& s, int lane)
        : writer(lane >= 8 && lane < 8 + kStripW && s.xl < W), head(s.strip == 0 && lane >= 8 && lane < 8 + kBoxM), x(s.x),
          lhi(min(lane + kBoxM, 63)), llo(max(lane - kBoxM - 1, 0)), ps((unsigned)s.ps), vcol((unsigned)(lane - 8)) {}
    __device__ __forceinline__ void diff(const double (&vrow)[5][64], double (&d)[5]) const
    {
#pragma unroll
        for (int c = 0; c < 5; c++) d[c] = vrow[c][lhi] - vrow[c][llo];
    }
    __device__ __forceinline__ void put(double* D16, double* VS0, int y, const double (&d)[5], const double (&vrow)[5][64], int lane) const
    {
        if (writer) {
            const unsigned i0 = d16_index(W, ps, y, 0, x), cs = d16_index(W, 0u, 0, 1, 0);   // channel 0, and the step to the next channel's tile
#pragma unroll
            for (int c = 0; c < 5; c++) st_off_nt<double>(D16, (i0 + (unsigned)c * cs) * 8u, d[c]);
        }
        if (head) {
#pragma unroll
            for (int c = 0; c < 5; c++) st_off<double>(VS0, (vs0_index(W, ps, c, y) + vcol) * 8u, vrow[c][lane]);
        }
    }
};

// Constants of a producer count of k_uvp.  4: the throughput shape (three workgroups per CU).  12: the LATENCY shape of the exact re-run of
// a few flagged pairs -- a phase lasts about one memory round trip (the gather issued in phase k is consumed in phase k + 1) however many
// rows it brings in, so twelve producers walk a level's rows in a third of the phases (28 instead of 82 at 320 px); one 14-wave workgroup
// per CU.
//   RSL  M-row ring in LDS: 15 rows of history + two phases in flight (producers write phase k+1 while the summer still reads the
//        leaving rows of phase k); 20 would collide with four producers
//   GL   gather lead in phases.  With four producers a phase is about one memory round trip and the gather of the next phase hides
//        behind it.  With twelve, a phase is the CU's own work for twelve rows (~1.5 us of VALU + texture addresser) and a gather
//        issued at its END would be waited for at the START of the next: it is issued TWO phases ahead, so the round trip overlaps a
//        whole phase of work
//   U    phases per unrolled body (static producer register slots: four input sets, GL + 1 gather sets)
//   WGS  the second launch bound
template <int NPROD> struct Producers;
template <> struct Producers<4> { static constexpr int RSL = 24, GL = 1, U = 4, WGS = 4; };
template <> struct Producers<12> { static constexpr int RSL = 48, GL = 2, U = 12, WGS = 1; };

// ---------------------------------------------------------------------------------------
// k_uvp: FarnebackUpdateMatrices fused into the vertical pass as a producer / consumer workgroup.  Per row of a strip, ~80 % of the
// instructions (loads, bilinear gather, normal equations) do not depend on the previous row; only five
// double adds per row chain.  A strip gets NPROD + 2 waves:
//   waves 2..NPROD+1 (producers): wave w evaluates the normal equations of entry NPROD*k+(w-2) in phase k
//       (entry e = image row min(e, H-1); entries 0..6 initialise the box, entry y+7 enters at step y) and
//       writes the row into a ring in LDS.  They only LOAD: loads and stores share one in-order
//       vmcnt on this hardware, so a wave that also stores waits for its own store acknowledgements
//       whenever it waits for a prefetched load;
//   wave 0 (summer): the only sequential part -- per entry, vsum += entering row - leaving row (both read
//       from the ring, all LDS reads of a phase first), publishes the vsum rows of the phase in LDS;
//   wave 1 (storer): one phase later forms D = vsum(x+7) - vsum(x-8) from those rows and is the only wave
//       that STORES (D tiles, vsum columns 0..6) -- it never waits on memory.
// (s_memtime stamps: with a single consumer wave doing sums, D and stores, that wave was the critical path.)
// ONE barrier per NPROD rows.  Producers software-pipeline their own entries (stride NPROD rows): flow/R0
// loads three phases ahead, gathers one phase ahead, static register slots; their steps have no branches
// around memory operations.  With four producers: 50 KiB of LDS = 3 workgroups per CU, and the registers allow as many (6 waves of at
// most 96 VGPRs: five waves fit on a SIMD).
// ---------------------------------------------------------------------------------------
template <int W, int NPROD>
__global__ __launch_bounds__(64 * (NPROD + 2), Producers<NPROD>::WGS) void k_uvp(const float* __restrict__ R, const float* __restrict__ flow,
                                                           double* __restrict__ D16, double* __restrict__ VS0, int npairs, const int* __restrict__ plist)
{
    using Pr = Producers<NPROD>;
    constexpr int H = W, m = kBoxM;
    constexpr int plane = W * H;
    constexpr int RSL = Pr::RSL, GL = Pr::GL, GR = GL + 1, U = Pr::U;
    static_assert(RSL % NPROD == 0 && RSL >= 15 + 2 * NPROD, "ring: whole phases, history + two phases in flight");
    constexpr int CH = 4;                                // entries the summer / storer hold in registers at a time
    static_assert(NPROD % CH == 0, "whole chunks of entries per phase");
    constexpr int NE = H + m;                            // entries
    constexpr int NP = (NE + NPROD - 1) / NPROD;         // producing phases
    constexpr int NPH = ((NP + 2 + U - 1) / U) * U;      // loop trip count (two drain phases + round up to the unroll)
    __shared__ float ringM[RSL][5][64];                  // normal-equation rows, slot = entry % RSL (30 KiB; 60 KiB with twelve producers)
    __shared__ double Vb[2][NPROD][5][64];               // vsum rows of a phase, summer -> storer
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Strip st = strip_decode<W>(npairs, plist, lane);
    if (st.ps < 0) return;
    const int x = st.x;

    if (wave == 0) {
        // ------------------------------- summer ----------------------------------------------
        // The only sequential part: five running double sums per column.  Phase k takes the rows the producers
        // evaluated in phase k-1 (entries NPROD*(k-1) ..) and publishes the vsum rows.
        double vs[5] = {0, 0, 0, 0, 0};
        for (int k = 0; k < NPH; k++) {
            if (k >= 1 && k - 1 < NP) {
                const int e0 = NPROD * (k - 1), pb = (k - 1) & 1;
                if (e0 < m && e0 + NPROD >= m) {
                    // the phase that completes the initial box: vs = (m+2) * row 0 + rows 1..m-1, in that order
#pragma unroll
                    for (int c = 0; c < 5; c++) {
                        vs[c] = (double)(ringM[0][c][lane] * (float)(m + 2));
#pragma unroll
                        for (int r = 1; r < m; r++) vs[c] += (double)ringM[r][c][lane];
                    }
                }
                // entering rows (this phase's entries) and the rows leaving the box with them (row y-8 = entry e-15;
                // row 0 while the window still touches the top edge), all reads of a chunk of entries first
#pragma unroll
                for (int c0 = 0; c0 < NPROD; c0 += CH) {
                    float a[CH][5], b[CH][5];
#pragma unroll
                    for (int i = 0; i < CH; i++) {
                        const int e = e0 + c0 + i, y = e - m;
                        const int sa = e % RSL, sb = y >= m + 1 ? (e - 15) % RSL : 0;
#pragma unroll
                        for (int c = 0; c < 5; c++) { a[i][c] = ringM[sa][c][lane]; b[i][c] = ringM[sb][c][lane]; }
                    }
#pragma unroll
                    for (int i = 0; i < CH; i++) {
                        const int e = e0 + c0 + i;
                        if (e >= m && e < NE) {
#pragma unroll
                            for (int c = 0; c < 5; c++) {
                                vs[c] += (double)(a[i][c] - b[i][c]);
                                Vb[pb][c0 + i][c][lane] = vs[c];
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
        return;
    }
    if (wave == 1) {
        // ------------------------------- storer ----------------------------------------------
        // Takes the rows the summer published a phase earlier and is the only wave that stores: it never waits on memory.
        const StripStore<W> out(st, lane);
        for (int k = 0; k < NPH; k++) {
            if (k >= 2 && k - 2 < NP) {
                const int e0 = NPROD * (k - 2), pb = (k - 2) & 1;
#pragma unroll
                for (int c0 = 0; c0 < NPROD; c0 += CH) {
                    double dv[CH][5];
#pragma unroll
                    for (int i = 0; i < CH; i++) out.diff(Vb[pb][c0 + i], dv[i]);
#pragma unroll
                    for (int i = 0; i < CH; i++) {
                        const int e = e0 + c0 + i;
                        if (e >= m && e < NE) out.put(D16, VS0, e - m, dv[i], Vb[pb][c0 + i], lane);
                    }
                }
            }
            __syncthreads();
        }
        return;
    }

    // ----------------------------------- producers ------------------------------------------
    const unsigned r0base = (unsigned)st.p * 5u * plane, r1base = r0base + 5u * plane, flbase = (unsigned)st.p * 2u * plane;
    const int pi = wave - 2;                             // entry index inside a phase
    const float sx = border_factor(x, W);                // x part of the border attenuation: a per-lane constant
    NeIn in[4]; NeG g[GR];
    auto row_of = [&](int k) { return min(NPROD * k + pi, H - 1); };
#pragma unroll
    for (int k = 0; k < 3; k++) ne_load(R, flow, r0base, flbase, x, row_of(k), W, plane, in[k]);
#pragma unroll
    for (int q = 0; q < GL; q++) ne_gather(R, r1base, in[q], x, row_of(q), W, H, g[q]);
    for (int kb = 0; kb < NPH; kb += U) {
#pragma unroll
        for (int kk = 0; kk < U; kk++) {
            const int k = kb + kk;
            if (k < NP) {
                // rows past the last entry (e >= NE, only in the final phase) are evaluated on clamped
                // addresses and never consumed: no branch around the loads
                float a[5];
                ne_finish(in[kk & 3], g[kk % GR], sx, border_factor(row_of(k), H), a);
                const int slot = (NPROD * k + pi) % RSL;
#pragma unroll
                for (int c = 0; c < 5; c++) ringM[slot][c][lane] = a[c];
                // refill: gathers of this wave's entry GL phases on, inputs three phases ahead
                ne_gather(R, r1base, in[(kk + GL) & 3], x, row_of(k + GL), W, H, g[(kk + GL) % GR]);
                ne_load(R, flow, r0base, flbase, x, row_of(k + 3), W, plane, in[(kk + 3) & 3]);
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------
// k_uv: the same computation in the STREAMING shape (320 px, more strips than are resident in one round).  Every lane evaluates the
// normal equations of its column row by row and feeds them straight into the vertical running sums, so the five M
// planes never exist in memory.  A row's evaluation needs two dependent memory round trips
// (flow/R0, then the bilinear gather of R1 at the warped position); they are software
// pipelined by hand: at the step that consumes row r, the gathers of row r+2 and the flow/R0
// loads of row r+4 are issued (explicit register stages).  The vsum rows go to LDS, where the strip's
// second wave forms vsum(x+7) - vsum(x-8) and stores it (ds_bpermute would cost ~20 cycles per wave64 on
// gfx950, an LDS write + two reads ~1/3 of that).
// ---------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(128) void k_uv(const float* __restrict__ R, const float* __restrict__ flow,
                                           double* __restrict__ D16, double* __restrict__ VS0, int npairs, const int* __restrict__ plist)
{
    constexpr int H = W, m = kBoxM;
    constexpr int plane = W * H;
    // Workgroup = one strip = compute wave + store wave (more strips per workgroup only couple them through the barrier).  The compute wave only LOADS: on gfx9-family
    // hardware loads and stores share one in-order vmcnt, so a wave that also stores D waits, at every
    // step, for the acknowledgement of stores it issued a step earlier (measured: 126 of 326 us at 320 px).
    // It publishes the two vsum rows of a step in LDS (double-buffered); after the step's barrier its
    // store wave forms D = vsum(x+7) - vsum(x-8) from them and writes the tiles, never waiting on memory.
    __shared__ double xw[2][2][5][64];                  // [buffer][row][channel][lane], 10 KiB
    __shared__ float ringl[16][5][64];                  // the compute wave's last 16 evaluated rows, slot = row & 15
    const int wv = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const Strip st = strip_decode<W>(npairs, plist, lane);
    if (st.ps < 0) return;                               // both waves of a strip leave together
    const int x = st.x;

    if (wv == 1) {
        const StripStore<W> out(st, lane);
        for (int y0 = 0; y0 < H; y0 += 2) {
            const int buf = (y0 >> 1) & 1;
            __syncthreads();
            double d0[5], d1[5];
            out.diff(xw[buf][0], d0);
            out.diff(xw[buf][1], d1);
            out.put(D16, VS0, y0, d0, xw[buf][0], lane);
            out.put(D16, VS0, y0 + 1, d1, xw[buf][1], lane);
        }
        return;
    }

    const unsigned r0base = (unsigned)st.p * 5u * plane, r1base = r0base + 5u * plane, flbase = (unsigned)st.p * 2u * plane;   // R[frame p], R[frame p+1]
    const float sx = border_factor(x, W);               // x part of the border attenuation: a per-lane constant
    auto sy = [](int row) { return border_factor(row, H); };
    // Software pipeline, static register slots, FOUR steps deep: a row's evaluation needs two dependent
    // memory round trips (flow/R0, then the gather of R1 at the warped position), and under load one round
    // trip takes about as long as two steps.  At the step that consumes rows (r, r+1) the gathers of rows
    // r+4, r+5 and the flow/R0 loads of rows r+8, r+9 are issued.  The 16-row history of the box filter
    // lives in LDS (20 KiB), which is what leaves registers for in[8] and g[4].
    NeIn in[8]; NeG g[4];
    double vs[5];
#pragma unroll
    for (int r = 0; r < m; r++) {
        float a[5];
        ne_load(R, flow, r0base, flbase, x, r, W, plane, in[0]);
        ne_gather(R, r1base, in[0], x, r, W, H, g[0]);
        ne_finish(in[0], g[0], sx, sy(r), a);
#pragma unroll
        for (int c = 0; c < 5; c++) {
            ringl[r][c][lane] = a[c];
            if (r == 0) vs[c] = (double)(a[c] * (float)(m + 2));
            else vs[c] += (double)a[c];
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) ne_load(R, flow, r0base, flbase, x, min(m + k, H - 1), W, plane, in[k]);
#pragma unroll
    for (int k = 0; k < 4; k++) ne_gather(R, r1base, in[k], x, min(m + k, H - 1), W, H, g[k]);

    // Two rows per step: their normal equations are independent, only the five double adds per row chain.
    // The step has no branches and no stores, so every s_waitcnt vmcnt is exact.
    static_assert(H % 8 == 0, "four steps per unrolled body");
    for (int yb = 0; yb < H; yb += 8) {
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            const int j0 = 2 * jj, j1 = j0 + 1;
            const int y0 = yb + j0, y1 = y0 + 1;
            const int ra = min(y0 + m, H - 1), rb = min(y1 + m, H - 1);   // entering rows (clamped)
            float a0[5], a1[5];
            ne_finish(in[j0], g[j0 & 3], sx, sy(ra), a0);
            ne_finish(in[j1], g[j1 & 3], sx, sy(rb), a1);
            // The refills must not be scheduled above the arithmetic that consumes the old contents of their slots:
            // otherwise old and new values of a slot are live together, the new ones get other registers, and the
            // loop back-edge becomes ~60 v_mov of just-loaded registers behind an s_waitcnt vmcnt(7) -- a drain of
            // the whole software pipeline every four steps (seen in the ISA).
            __builtin_amdgcn_sched_barrier(0);
            // refill the slots just consumed: gathers two steps ahead, inputs four steps ahead
            ne_gather(R, r1base, in[(j0 + 4) & 7], x, min(ra + 4, H - 1), W, H, g[j0 & 3]);
            ne_gather(R, r1base, in[(j1 + 4) & 7], x, min(rb + 4, H - 1), W, H, g[j1 & 3]);
            ne_load(R, flow, r0base, flbase, x, min(ra + 8, H - 1), W, plane, in[j0]);
            ne_load(R, flow, r0base, flbase, x, min(rb + 8, H - 1), W, plane, in[j1]);
            // leaving rows y-8 (row 0 while the window still touches the top edge); read both before the
            // entering rows overwrite their slots (row y1+7 takes the slot of row y0-8)
            const int so0 = y0 >= m + 1 ? (y0 + 8) & 15 : 0, so1 = y1 >= m + 1 ? (y1 + 8) & 15 : 0;
            float b0[5], b1[5];
#pragma unroll
            for (int c = 0; c < 5; c++) { b0[c] = ringl[so0][c][lane]; b1[c] = ringl[so1][c][lane]; }
#pragma unroll
            for (int c = 0; c < 5; c++) {
                ringl[(y0 + m) & 15][c][lane] = a0[c];
                ringl[(y1 + m) & 15][c][lane] = a1[c];
                vs[c] += (double)(a0[c] - b0[c]);
                xw[jj & 1][0][c][lane] = vs[c];
                vs[c] += (double)(a1[c] - b1[c]);
                xw[jj & 1][1][c][lane] = vs[c];
            }
            __syncthreads();
        }
    }
}

// staging registers of the loader wave: one chunk = 5 channels x 4 x 16 B per lane
typedef double dbl2 __attribute__((ext_vector_type(2)));
struct ChunkRegs { dbl2 v[5][4]; };

// the row block of a workgroup of k_hscan / k_hscan_lat
template <int W>
struct RowBlock {
    static constexpr int XCH = d16_xch(W), NYB = d16_nyb(W);
    int ps, ybk;
    const double* tiles;             // the block's first tile
    __device__ __forceinline__ RowBlock(const double* D16) : ps(blockIdx.x / NYB), ybk(blockIdx.x - ps * NYB), tiles(D16 + d16_index<int64_t>(W, ps, ybk * 64, 0, 0)) {}
    // tile (channel c, column chunk xc): its place among the block's [c][xc]
    __device__ __forceinline__ const double* tile(int c, int xc) const { return tiles + d16_index(W, 0, 0, c, xc * 8); }
};

template <int W>
__device__ __forceinline__ void chunk_issue(ChunkRegs& r, const RowBlock<W>& rb, int xc, int lane)
{
#pragma unroll
    for (int c = 0; c < 5; c++)
#pragma unroll
        for (int i = 0; i < 4; i++)
            r.v[c][i] = __builtin_nontemporal_load(reinterpret_cast<const dbl2*>(rb.tile(c, xc) + i * 128 + lane * 2));
}

__device__ __forceinline__ void chunk_commit(const ChunkRegs& r, double (*buf)[512], int lane)
{
#pragma unroll
    for (int c = 0; c < 5; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<dbl2*>(&buf[c][i * 128 + lane * 2]) = r.v[c][i];
}

// The loader wave of k_hscan: the tile image is copied verbatim (16 B per lane, 4 KiB per channel).  Chunk xc+2 is in flight into one
// register set while chunk xc+1 (the other set) is written to the LDS buffer the scanner released last: two chunks (40 KiB) in flight
// per workgroup with two LDS buffers.  One barrier per chunk, XCH + 1 in all.  (A function of its own: written out inside the kernel the
// same loop compiles to seven more s_waitcnt.)
template <int W>
__device__ __forceinline__ void role_load(const RowBlock<W>& blk, double (*lds)[5][512], int lane)
{
    constexpr int XCH = d16_xch(W);
    ChunkRegs ra, rb;
    chunk_issue(ra, blk, 0, lane);
    if (XCH > 1) chunk_issue(rb, blk, 1, lane);
    chunk_commit(ra, lds[0], lane);
    __syncthreads();
    int xc = 0;
    // steady state without conditionals: behind an `if` the compiler has to assume the loads were skipped
    // and waits vmcnt(19..0) for the commit, i.e. for the chunk it has just issued as well
    for (; xc + 3 < XCH; xc += 2) {
        chunk_issue(ra, blk, xc + 2, lane);
        __builtin_amdgcn_sched_barrier(0);          // keep the loads ahead of the LDS writes of the other set
        chunk_commit(rb, lds[1], lane);
        __syncthreads();
        chunk_issue(rb, blk, xc + 3, lane);
        __builtin_amdgcn_sched_barrier(0);
        chunk_commit(ra, lds[0], lane);
        __syncthreads();
    }
    // the last one (odd XCH: 40 px has 5 chunks) or two chunks
    for (; xc < XCH; xc += 2) {
        if (xc + 2 < XCH) chunk_issue(ra, blk, xc + 2, lane);
        if (xc + 1 < XCH) chunk_commit(rb, lds[1], lane);
        __syncthreads();
        if (xc + 1 < XCH) {
            if (xc + 3 < XCH) chunk_issue(rb, blk, xc + 3, lane);
            if (xc + 2 < XCH) chunk_commit(ra, lds[0], lane);
            __syncthreads();
        }
    }
}

// cv2's initial horizontal sums of image row yc (clamped): g = (m + 2) * vsum[0] + vsum[1] + .. + vsum[m - 1], in that order
template <int H>
__device__ __forceinline__ void row_init(const double* VS0, int ps, int yc, double (&g)[5])
{
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const double* vc = VS0 + vs0_index<int64_t>(H, ps, c, yc);
        double s = vc[0] * (double)(kBoxM + 2);
#pragma unroll
        for (int k = 1; k < kBoxM; k++) s += vc[k];
        g[c] = s;
    }
}

template <int W>
__global__ __launch_bounds__(128) void k_hscan(const double* __restrict__ D16, const double* __restrict__ VS0,
                                              float* __restrict__ flow, int npairs, const int* __restrict__ plist)
{
    constexpr int H = W;
    constexpr int XCH = d16_xch(W);
    constexpr int64_t plane = (int64_t)W * H;
    __shared__ __align__(16) double lds[2][5][512];
    __shared__ __align__(16) float outb[2][64][20];      // row stride 80 B: ds_write_b128 of 8 lanes covers all banks
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const RowBlock<W> blk(D16);
    const int ps = blk.ps, ybk = blk.ybk;
    const int p = plist ? plist[ps] : ps;                // ps indexes the scratch, p the pair's flow

    if (wave == 1) {
        role_load<W>(blk, lds, lane);
        return;
    }

    // scanner (wave 0)
    double g[5];
    row_init<H>(VS0, ps, min(ybk * 64 + lane, H - 1), g);
    __syncthreads();
    auto scan8 = [&](int buf, float (&ox)[8], float (&oy)[8]) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int c = 0; c < 5; c++) g[c] += lds[buf][c][d16_slot(lane, j)];
            fb_solve_exact(g, ox[j], oy[j]);
        }
    };
    // Results leave through a small LDS transpose: a lane owns a ROW, so direct stores would touch 64
    // different lines with 16 B each per instruction (measured: 43 of the kernel's 153 us at 320 px).
    // Re-read as [16 rows][4 lanes x 16 B], one store instruction covers 16 rows x 64 contiguous bytes.
    const int tr = lane >> 2, tq = lane & 3;
    float* fout = flow + (int64_t)p * 2 * plane + (int64_t)(ybk * 64 + tr) * W + tq * 4;
    for (int xc = 0; xc < XCH; xc += 2) {
        float ax[8], ay[8], bx[8], by[8];
        scan8(0, ax, ay);
        __syncthreads();
        const bool second = xc + 1 < XCH;
        if (second) scan8(1, bx, by);
        {
            float4* ox = reinterpret_cast<float4*>(outb[0][lane]);
            float4* oy = reinterpret_cast<float4*>(outb[1][lane]);
            ox[0] = make_float4(ax[0], ax[1], ax[2], ax[3]); ox[1] = make_float4(ax[4], ax[5], ax[6], ax[7]);
            oy[0] = make_float4(ay[0], ay[1], ay[2], ay[3]); oy[1] = make_float4(ay[4], ay[5], ay[6], ay[7]);
            if (second) {
                ox[2] = make_float4(bx[0], bx[1], bx[2], bx[3]); ox[3] = make_float4(bx[4], bx[5], bx[6], bx[7]);
                oy[2] = make_float4(by[0], by[1], by[2], by[3]); oy[3] = make_float4(by[4], by[5], by[6], by[7]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (second || tq < 2) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int r = tr + 16 * k;
                if (ybk * 64 + r < H) {
                    float* o = fout + (int64_t)k * 16 * W + xc * 8;
                    *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(&outb[0][r][tq * 4]);
                    *reinterpret_cast<float4*>(o + plane) = *reinterpret_cast<const float4*>(&outb[1][r][tq * 4]);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (second) __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------
// k_hscan_lat: the same horizontal pass in a LATENCY shape, for the exact re-run of a few flagged pairs (round 5).  In k_hscan a lane owns a
// row and walks its 320 columns alone: five dependent double adds AND the 2 x 2 solve with its IEEE division per column, ~115 ns per column,
// 37 us per launch however few pairs there are.  Only the adds are a chain.  Here the scanner wave does nothing but the chain (g of a chunk of
// eight columns goes to LDS), and four SOLVER waves one chunk behind turn g into flow -- 512 (row, column) solves per chunk, two per lane, the
// same fb_solve_exact as k_hscan (bit-identical) -- and store it through a 16-row transpose.  One barrier per chunk.
// ---------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(384) void k_hscan_lat(const double* __restrict__ D16, const double* __restrict__ VS0,
                                                  float* __restrict__ flow, int npairs, const int* __restrict__ plist)
{
    constexpr int H = W;
    constexpr int XCH = d16_xch(W);
    constexpr int64_t plane = (int64_t)W * H;
    constexpr int GS = 5 * 64 + 2;                        // doubles per column of a g buffer (+ 2: the four columns a solver instruction reads fall on different banks)
    __shared__ __align__(16) double lds[2][5][512];
    __shared__ __align__(16) double gbuf[2][8][GS];
    __shared__ __align__(16) float outb[4][2][16][8];     // per solver wave: [component][row][column of the chunk]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const RowBlock<W> blk(D16);
    const int ps = blk.ps, ybk = blk.ybk;
    const int p = plist ? plist[ps] : ps;                // ps indexes the scratch, p the pair's flow
    if (wave == 1) {
        // loader: chunk xc + 1 is committed to LDS while the scanner walks chunk xc; two chunks further are in flight.  Not k_hscan's
        // role_load: its peeled last step is a second copy of a commit and two barriers, and this kernel then takes 172 registers
        // instead of 169
        static_assert(XCH % 2 == 0, "the loader alternates two register sets");
        ChunkRegs ra, rb;
        chunk_issue(ra, blk, 0, lane);
        chunk_issue(rb, blk, 1, lane);
        chunk_commit(ra, lds[0], lane);
        __syncthreads();
        for (int xc = 0; xc < XCH; xc += 2) {
            if (xc + 2 < XCH) chunk_issue(ra, blk, xc + 2, lane);
            chunk_commit(rb, lds[1], lane);
            __syncthreads();
            if (xc + 3 < XCH) chunk_issue(rb, blk, xc + 3, lane);
            if (xc + 2 < XCH) chunk_commit(ra, lds[0], lane);
            __syncthreads();
        }
        return;
    }
    if (wave == 0) {
        // scanner: cv2's running sums g += D(x), literally; nothing else
        double g[5];
        row_init<H>(VS0, ps, min(ybk * 64 + lane, H - 1), g);
        __syncthreads();
        for (int xc = 0; xc < XCH; xc++) {
            const int buf = xc & 1;
#pragma unroll
            for (int j = 0; j < 8; j++) {
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    g[c] += lds[buf][c][d16_slot(lane, j)];
                    gbuf[buf][j][c * 64 + lane] = g[c];
                }
            }
            __syncthreads();
        }
        return;
    }
    // solvers: wave s owns rows 16 s .. 16 s + 15 of the block; lane = (row, column j) and (row, column j + 4) of the chunk
    const int s4 = wave - 2, r16 = lane & 15, j0 = lane >> 4;
    const int row = 16 * s4 + r16;
    float (*ob)[16][8] = outb[s4];
    const int sr = (lane & 31) >> 1, sh = lane & 1, sc = lane >> 5;       // store phase: row, 16-byte half of the chunk's 32 bytes, component
    const bool store_ok = ybk * 64 + 16 * s4 + sr < H;
    float* fout = flow + (int64_t)p * 2 * plane + (int64_t)sc * plane + (int64_t)(ybk * 64 + 16 * s4 + sr) * W + sh * 4;
    auto solve = [&](int xc) {
        const int buf = xc & 1;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int j = j0 + 4 * i;
            const double* gp = &gbuf[buf][j][row];
            const double g[5] = {gp[0], gp[64], gp[128], gp[192], gp[256]};
            fb_solve_exact(g, ob[0][r16][j], ob[1][r16][j]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (store_ok) *reinterpret_cast<float4*>(fout + xc * 8) = *reinterpret_cast<const float4*>(&ob[sc][sr][sh * 4]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    __syncthreads();
    for (int xc = 0; xc < XCH; xc++) {
        if (xc >= 1) solve(xc - 1);
        __syncthreads();
    }
    solve(XCH - 1);
}

// The three shapes of an iteration.  Below 320 px (latency / issue bound levels) the producer / consumer form k_uvp<W, 4>; at 320 px it wins
// as long as all its workgroups are resident at once (3 per CU, 50 KiB of LDS each): ~170 us per launch instead of ~290 us; beyond that it
// needs a second residency round and k_uv streams (every design measured there with 119 pairs lands at ~290-300 us: HBM read/write mix;
// k_uvp with 2 / 3 / 4 producers 293 / 377 / 340 us).  The exact re-run of a few flagged pairs (a pair list, 160 / 320 px, one workgroup
// per CU) takes the latency pair: twelve producers walk the rows in a third of the phases, and k_hscan_lat.
enum class Shape {
    kProducer,     // k_uvp<W, 4> + k_hscan<W>
    kLatency,      // k_uvp<W, 12> + k_hscan_lat<W>
    kStreaming,    // k_uv<S> + k_hscan<S>
};

// which shapes have kernels at width w: choose_shape returns no other, and blur_iteration instantiates no other
constexpr bool shape_built(Shape s, int w) { return s == Shape::kProducer || (s == Shape::kLatency ? w >= S / 2 : w == S); }

Shape choose_shape(int w, int np, bool listed)
{
    const int blocks = np * strips_of(w);
    if (listed && shape_built(Shape::kLatency, w) && blocks <= 256) return Shape::kLatency;
    if (!shape_built(Shape::kStreaming, w) || blocks <= 3 * 256) return Shape::kProducer;
    return Shape::kStreaming;
}

// one FarnebackUpdateFlow_Blur iteration at width W: matrices from the current flow, box sums, solve
// plist (may be null): the launches work on the pairs plist[0 .. np) of the chunk; the double intermediate is indexed by position in the list
template <int W>
void blur_iteration(avd_ctx* ctx, hipStream_t stream, const float* R, float* flow, FbTwoScratch s, int np, const int* plist, bool marks)
{
    // profiling: HIP events around the two full-resolution kernels (avd_stage_ms 4 and 5)
    auto mark = [&](void) { level320_mark(ctx, marks && W == S); };
    const Shape shape = choose_shape(W, np, plist != nullptr);
    const dim3 grid(8 * ((np + 7) / 8) * strips_of(W));  // (XCD, pair-in-XCD, strip); pairs >= np exit at once
    const float* fin = flow;
    mark();
    switch (shape) {
    case Shape::kProducer:
        hipLaunchKernelGGL((k_uvp<W, 4>), grid, dim3(64 * 6), 0, stream, R, fin, s.vs, s.vs0, np, plist);
        break;
    case Shape::kLatency:
        if constexpr (shape_built(Shape::kLatency, W)) hipLaunchKernelGGL((k_uvp<W, 12>), grid, dim3(64 * 14), 0, stream, R, fin, s.vs, s.vs0, np, plist);
        break;
    case Shape::kStreaming:
        if constexpr (shape_built(Shape::kStreaming, W)) hipLaunchKernelGGL(k_uv<W>, grid, dim3(128), 0, stream, R, fin, s.vs, s.vs0, np, plist);
        break;
    }
    mark(); mark();
    const dim3 hgrid(np * d16_nyb(W));
    const double *D = s.vs, *V = s.vs0;
    if (shape != Shape::kLatency) hipLaunchKernelGGL(k_hscan<W>, hgrid, dim3(128), 0, stream, D, V, flow, np, plist);
    else if constexpr (shape_built(Shape::kLatency, W)) hipLaunchKernelGGL(k_hscan_lat<W>, hgrid, dim3(384), 0, stream, D, V, flow, np, plist);
    mark();
}

}  // namespace

// doubles for np pairs: D as d16_pair_tiles(320) tiles of 64 x 8 per pair, columns 0..6 of vsum as [5][320][8] (smaller levels use the front)
FbTwoScratchSize fb_two_scratch_size(size_t np)
{
    static_assert(d16_index<size_t>(S, 1, 0, 0, 0) == 5 * AVD_NPIX + 512, "five channels + one pad tile per pair");
    return {d16_index<size_t>(S, np, 0, 0, 0), vs0_index<size_t>(S, np, 0, 0)};
}

int launch_fb_two(avd_ctx* ctx, hipStream_t stream, int w, const float* R, float* flow, FbTwoScratch s, int np, const int* plist, bool marks)
{
    if (!s.vs || !s.vs0) { ctx->err = "two-kernel Farneback path: scratch not reserved"; return AVD_ERR_ARG; }
    if (fb_dispatch_width(w, [&](auto wc) { blur_iteration<decltype(wc)::value>(ctx, stream, R, flow, s, np, plist, marks); })) return 0;
    ctx->err = "launch_fb_two: unsupported level size";
    return AVD_ERR_ARG;
}
