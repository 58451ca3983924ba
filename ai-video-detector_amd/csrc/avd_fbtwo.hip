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

__host__ __device__ constexpr int d16_xch(int w) { return (w + 7) / 8; }
__host__ __device__ constexpr int d16_nyb(int h) { return (h + 63) / 64; }
// tiles per pair, padded to an ODD count: an unpadded 320x320 pair is exactly 4 MiB, and a power-of-two
// stride between the pairs that all workgroups touch in lock step lands on the same HBM channels
__host__ __device__ constexpr int d16_pair_tiles(int w) { return (d16_nyb(w) * 5 * d16_xch(w)) | 1; }

// ---------------------------------------------------------------------------------------
// k_uv = FarnebackUpdateMatrices fused into the vertical pass: every lane evaluates the normal equations of its
// column row by row and feeds them straight into the vertical running sums, so the five M
// planes never exist in memory.  A row's evaluation needs two dependent memory round trips
// (flow/R0, then the bilinear gather of R1 at the warped position); they are software
// pipelined by hand: at the step that consumes row r, the gathers of row r+2 and the flow/R0
// loads of row r+4 are issued (explicit register stages).  The vsum rows go to LDS, where the strip's
// second wave forms vsum(x+7) - vsum(x-8) and stores it (ds_bpermute would cost ~20 cycles per wave64 on
// gfx950, an LDS write + two reads ~1/3 of that).
// ---------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------
// k_uvp: the same computation as a producer / consumer workgroup.  Per row of a strip, ~80 % of the
// instructions (loads, bilinear gather, normal equations) do not depend on the previous row; only five
// double adds per row chain.  A strip gets NPROD + 2 waves:
//   waves 2..NPROD+1 (producers): wave w evaluates the normal equations of entry NPROD*k+(w-2) in phase k
//       (entry e = image row min(e, H-1); entries 0..6 initialise the box, entry y+7 enters at step y) and
//       writes the row into a 24-slot ring in LDS.  They only LOAD: loads and stores share one in-order
//       vmcnt on this hardware, so a wave that also stores waits for its own store acknowledgements
//       whenever it waits for a prefetched load;
//   wave 0 (summer): the only sequential part -- per entry, vsum += entering row - leaving row (both read
//       from the ring, all LDS reads of a phase first), publishes the vsum rows of the phase in LDS;
//   wave 1 (storer): one phase later forms D = vsum(x+7) - vsum(x-8) from those rows and is the only wave
//       that STORES (D tiles, vsum columns 0..6) -- it never waits on memory.
// (s_memtime stamps: with a single consumer wave doing sums, D and stores, that wave was the critical path.)
// ONE barrier per NPROD rows.  Producers software-pipeline their own entries (stride NPROD rows): flow/R0
// loads three phases ahead, gathers one phase ahead, static register slots; their steps have no branches
// around memory operations.  50 KiB of LDS = 3 workgroups per CU by LDS, 2 by registers (6 waves x 104 VGPRs).
// ---------------------------------------------------------------------------------------
template <int W, int NPROD>
__global__ __launch_bounds__(64 * (NPROD + 2), (NPROD <= 4 ? 4 : 1)) void k_uvp(const float* __restrict__ R, const float* __restrict__ flow,
                                                           double* __restrict__ D16, double* __restrict__ VS0, int npairs, const int* __restrict__ plist)
{
    // NPROD = 2 .. 4: the throughput shapes (three workgroups per CU).  NPROD = 12 (round 5): the LATENCY shape of the exact re-run of a few
    // flagged pairs -- a phase lasts about one memory round trip (the gather issued in phase k is consumed in phase k + 1) however many rows
    // it brings in, so twelve producers walk a level's rows in a third of the phases (28 instead of 82 at 320 px); one 14-wave workgroup per CU.
    static_assert((NPROD >= 2 && NPROD <= 4 && 24 % NPROD == 0) || NPROD == 8 || NPROD == 12, "ring size below covers these producer counts");
    constexpr int H = W, m = 7;
    constexpr int NSTRIP = (W + kStripW - 1) / kStripW, XCH = d16_xch(W);
    constexpr int plane = W * H;
    constexpr int RSL = NPROD <= 4 ? 24 : 4 * NPROD;     // M-row ring in LDS: 15 rows of history + two phases in flight (producers write phase k+1
                                                         // while the summer still reads the leaving rows of phase k); 20 would collide
    static_assert(RSL % NPROD == 0 && RSL >= 15 + 2 * NPROD, "ring: whole phases, history + two phases in flight");
    constexpr int CH = NPROD <= 4 ? NPROD : 4;           // entries the summer / storer hold in registers at a time
    // gather lead in phases.  With four producers a phase is about one memory round trip and the gather of the next phase hides behind it.  With twelve, a
    // phase is the CU's own work for twelve rows (~1.5 us of VALU + texture addresser) and a gather issued at its END would be waited for at the START of the next:
    // it is issued TWO phases ahead, so the round trip overlaps a whole phase of work
    constexpr int GL = NPROD >= 8 ? 2 : 1, GR = GL + 1;
    constexpr int U = NPROD >= 8 ? 12 : 4;               // phases per unrolled body (static producer register slots: four input sets, GR gather sets)
    constexpr int NE = H + m;                            // entries
    constexpr int NP = (NE + NPROD - 1) / NPROD;         // producing phases
    constexpr int NPH = ((NP + 2 + U - 1) / U) * U;      // loop trip count (two drain phases + round up to the unroll)
    __shared__ float ringM[RSL][5][64];                  // normal-equation rows, slot = entry % RSL (30 KiB; 60 KiB with twelve producers)
    __shared__ double Vb[2][NPROD][5][64];               // vsum rows of a phase, summer -> storer
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // workgroups are dealt round-robin to the 8 XCDs.  The strips of a pair share their halo columns and the
    // gathered R1 rows, and pair p+1 reads as R0 the frame that pair p gathers as R1, at about the same rows at
    // about the same time: so an XCD (one L2) gets all strips of a CONTIGUOUS run of pairs.
    const int sj = blockIdx.x >> 3, ppx = (npairs + 7) >> 3;
    const int ps = (blockIdx.x & 7) * ppx + sj / NSTRIP, strip = sj % NSTRIP;
    if (sj / NSTRIP >= ppx || ps >= npairs) return;
    const int p = plist ? plist[ps] : ps;              // ps indexes the scratch (D, vsum columns), p the pair's R and flow
    const int xl = strip * kStripW - 8 + lane;         // logical column of this lane
    const int x = clampi(xl, 0, W - 1);                // edge replicate = duplicate chain

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
        // Forms D = vsum(x+7) - vsum(x-8) of the rows the summer published a phase earlier and is the only
        // wave that stores (D tiles, vsum columns 0..6): it never waits on memory.
        const bool writer = lane >= 8 && lane < 8 + kStripW && xl < W;
        const bool head = strip == 0 && lane >= 8 && lane < 8 + m;
        const unsigned dbase = ((unsigned)ps * d16_pair_tiles(W) + (x >> 3)) * 512u + (x & 7);   // tile column of this lane
        const unsigned vbase = (unsigned)ps * 5u * H * 8u + (unsigned)(lane - 8);
        const int lhi = min(lane + m, 63), llo = max(lane - m - 1, 0);
        for (int k = 0; k < NPH; k++) {
            if (k >= 2 && k - 2 < NP) {
                const int e0 = NPROD * (k - 2), pb = (k - 2) & 1;
#pragma unroll
                for (int c0 = 0; c0 < NPROD; c0 += CH) {
                    double dv[CH][5];
#pragma unroll
                    for (int i = 0; i < CH; i++)
#pragma unroll
                        for (int c = 0; c < 5; c++) dv[i][c] = Vb[pb][c0 + i][c][lhi] - Vb[pb][c0 + i][c][llo];
#pragma unroll
                    for (int i = 0; i < CH; i++) {
                        const int e = e0 + c0 + i, y = e - m;
                        if (e >= m && e < NE) {
                            if (writer) {
                                const unsigned sw = (unsigned)((x & 7) ^ (y & 7)) - (unsigned)(x & 7);     // swizzled slot - plain slot
                                const unsigned t0 = dbase + ((unsigned)(y >> 6) * 5 * XCH) * 512u + (y & 63) * 8 + sw;
#pragma unroll
                                for (int c = 0; c < 5; c++) st_off_nt<double>(D16, (t0 + (unsigned)c * XCH * 512u) * 8u, dv[i][c]);
                            }
                            if (head) {
#pragma unroll
                                for (int c = 0; c < 5; c++) st_off<double>(VS0, (vbase + (unsigned)((c * H + y) * 8)) * 8u, Vb[pb][c0 + i][c][lane]);
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
        return;
    }

    // ----------------------------------- producers ------------------------------------------
    const unsigned r0base = (unsigned)p * 5u * plane, r1base = r0base + 5u * plane, flbase = (unsigned)p * 2u * plane;
    const int pi = wave - 2;                             // entry index inside a phase
    NeIn in[4]; NeG g[GR];
    auto row_of = [&](int k) { return min(NPROD * k + pi, H - 1); };
#pragma unroll
    for (int k = 0; k < 3; k++) ne_load(R, flow, r0base, flbase, x, row_of(k), W, plane, in[k]);
#pragma unroll
    for (int q = 0; q < GL; q++) ne_gather(R, r1base, in[q], x, row_of(q), W, H, plane, g[q]);
    for (int kb = 0; kb < NPH; kb += U) {
#pragma unroll
        for (int kk = 0; kk < U; kk++) {
            const int k = kb + kk;
            if (k < NP) {
                // rows past the last entry (e >= NE, only in the final phase) are evaluated on clamped
                // addresses and never consumed: no branch around the loads
                float a[5];
                ne_finish(in[kk & 3], g[kk % GR], x, row_of(k), W, H, a);
                const int slot = (NPROD * k + pi) % RSL;
#pragma unroll
                for (int c = 0; c < 5; c++) ringM[slot][c][lane] = a[c];
                // refill: gathers of this wave's entry GL phases on, inputs three phases ahead
                ne_gather(R, r1base, in[(kk + GL) & 3], x, row_of(k + GL), W, H, plane, g[(kk + GL) % GR]);
                ne_load(R, flow, r0base, flbase, x, row_of(k + 3), W, plane, in[(kk + 3) & 3]);
            }
            __syncthreads();
        }
    }
}

template <int W>
__global__ __launch_bounds__(128) void k_uv(const float* __restrict__ R, const float* __restrict__ flow,
                                           double* __restrict__ D16, double* __restrict__ VS0, int npairs, const int* __restrict__ plist)
{
    constexpr int H = W, m = 7;
    constexpr int NSTRIP = (W + kStripW - 1) / kStripW, XCH = d16_xch(W);
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
    // all strips of a contiguous run of pairs on one XCD (see k_uvp)
    const int sj = blockIdx.x >> 3, ppx = (npairs + 7) >> 3;
    const int ps = (blockIdx.x & 7) * ppx + sj / NSTRIP, strip = sj % NSTRIP;
    if (sj / NSTRIP >= ppx || ps >= npairs) return;      // both waves of a strip leave together
    const int p = plist ? plist[ps] : ps;                // ps indexes the scratch, p the pair's R and flow
    const int xl = strip * kStripW - 8 + lane;         // logical column of this lane
    const int x = clampi(xl, 0, W - 1);                // edge replicate = duplicate chain

    if (wv == 1) {
        const bool writer = lane >= 8 && lane < 8 + kStripW && xl < W;
        const bool head = strip == 0 && lane >= 8 && lane < 8 + m;
        const unsigned dbase = ((unsigned)ps * d16_pair_tiles(W) + (x >> 3)) * 512u + (x & 7);   // tile column of this lane
        const unsigned vbase = (unsigned)ps * 5u * H * 8u + (unsigned)(lane - 8);
        const int lhi = min(lane + m, 63), llo = max(lane - m - 1, 0);
        for (int y0 = 0; y0 < H; y0 += 2) {
            const int y1 = y0 + 1, buf = (y0 >> 1) & 1;
            __syncthreads();
            double d0[5], d1[5], h0[5], h1[5];
#pragma unroll
            for (int c = 0; c < 5; c++) {
                d0[c] = xw[buf][0][c][lhi] - xw[buf][0][c][llo];
                d1[c] = xw[buf][1][c][lhi] - xw[buf][1][c][llo];
                h0[c] = xw[buf][0][c][lane];
                h1[c] = xw[buf][1][c][lane];
            }
            if (writer) {
                const unsigned sw0 = (unsigned)((x & 7) ^ (y0 & 7)) - (unsigned)(x & 7);   // swizzled slot - plain slot
                const unsigned sw1 = (unsigned)((x & 7) ^ (y1 & 7)) - (unsigned)(x & 7);
                const unsigned t0 = dbase + ((unsigned)(y0 >> 6) * 5 * XCH) * 512u + (y0 & 63) * 8 + sw0;
                const unsigned t1 = dbase + ((unsigned)(y1 >> 6) * 5 * XCH) * 512u + (y1 & 63) * 8 + sw1;
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    st_off_nt<double>(D16, (t0 + (unsigned)c * XCH * 512u) * 8u, d0[c]);
                    st_off_nt<double>(D16, (t1 + (unsigned)c * XCH * 512u) * 8u, d1[c]);
                }
            }
            if (head) {
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    st_off<double>(VS0, (vbase + (unsigned)((c * H + y0) * 8)) * 8u, h0[c]);
                    st_off<double>(VS0, (vbase + (unsigned)((c * H + y1) * 8)) * 8u, h1[c]);
                }
            }
        }
        return;
    }

    const unsigned r0base = (unsigned)p * 5u * plane, r1base = r0base + 5u * plane, flbase = (unsigned)p * 2u * plane;   // R[frame p], R[frame p+1]
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
        ne_gather(R, r1base, in[0], x, r, W, H, plane, g[0]);
        ne_finish(in[0], g[0], x, r, W, H, a);
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
    for (int k = 0; k < 4; k++) ne_gather(R, r1base, in[k], x, min(m + k, H - 1), W, H, plane, g[k]);

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
            ne_finish(in[j0], g[j0 & 3], x, ra, W, H, a0);
            ne_finish(in[j1], g[j1 & 3], x, rb, W, H, a1);
            // The refills must not be scheduled above the arithmetic that consumes the old contents of their slots:
            // otherwise old and new values of a slot are live together, the new ones get other registers, and the
            // loop back-edge becomes ~60 v_mov of just-loaded registers behind an s_waitcnt vmcnt(7) -- a drain of
            // the whole software pipeline every four steps (seen in the ISA).
            __builtin_amdgcn_sched_barrier(0);
            // refill the slots just consumed: gathers two steps ahead, inputs four steps ahead
            ne_gather(R, r1base, in[(j0 + 4) & 7], x, min(ra + 4, H - 1), W, H, plane, g[j0 & 3]);
            ne_gather(R, r1base, in[(j1 + 4) & 7], x, min(rb + 4, H - 1), W, H, plane, g[j1 & 3]);
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

__device__ __forceinline__ void chunk_issue(ChunkRegs& r, const double* tiles, int xch, int xc, int lane)
{
#pragma unroll
    for (int c = 0; c < 5; c++)
#pragma unroll
        for (int i = 0; i < 4; i++)
            r.v[c][i] = __builtin_nontemporal_load(reinterpret_cast<const dbl2*>(tiles + ((int64_t)c * xch + xc) * 512 + i * 128 + lane * 2));
}

__device__ __forceinline__ void chunk_commit(const ChunkRegs& r, double (*buf)[512], int lane)
{
#pragma unroll
    for (int c = 0; c < 5; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<dbl2*>(&buf[c][i * 128 + lane * 2]) = r.v[c][i];
}

template <int W>
__global__ __launch_bounds__(128) void k_hscan(const double* __restrict__ D16, const double* __restrict__ VS0,
                                              float* __restrict__ flow, int npairs, const int* __restrict__ plist)
{
    constexpr int H = W, m = 7;
    constexpr int XCH = d16_xch(W), NYB = d16_nyb(H);
    constexpr int64_t plane = (int64_t)W * H;
    __shared__ __align__(16) double lds[2][5][512];
    __shared__ __align__(16) float outb[2][64][20];      // row stride 80 B: ds_write_b128 of 8 lanes covers all banks
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ps = blockIdx.x / NYB, ybk = blockIdx.x - ps * NYB;
    const int p = plist ? plist[ps] : ps;                // ps indexes the scratch, p the pair's flow
    const double* tiles = D16 + ((int64_t)ps * d16_pair_tiles(W) + (int64_t)ybk * 5 * XCH) * 512;   // [c][xc][512]

    if (wave == 1) {
        // loader: the tile image is copied verbatim (16 B per lane, 4 KiB per channel).  Chunk xc+2 is in
        // flight into one register set while chunk xc+1 (the other set) is written to the LDS buffer the
        // scanner released last: two chunks (40 KiB) in flight per workgroup with two LDS buffers.
        ChunkRegs ra, rb;
        chunk_issue(ra, tiles, XCH, 0, lane);
        if (XCH > 1) chunk_issue(rb, tiles, XCH, 1, lane);
        chunk_commit(ra, lds[0], lane);
        __syncthreads();
        int xc = 0;
        // steady state without conditionals: behind an `if` the compiler has to assume the loads were skipped
        // and waits vmcnt(19..0) for the commit, i.e. for the chunk it has just issued as well
        for (; xc + 3 < XCH; xc += 2) {
            chunk_issue(ra, tiles, XCH, xc + 2, lane);
            __builtin_amdgcn_sched_barrier(0);          // keep the loads ahead of the LDS writes of the other set
            chunk_commit(rb, lds[1], lane);
            __syncthreads();
            chunk_issue(rb, tiles, XCH, xc + 3, lane);
            __builtin_amdgcn_sched_barrier(0);
            chunk_commit(ra, lds[0], lane);
            __syncthreads();
        }
        for (; xc < XCH; xc += 2) {
            if (xc + 2 < XCH) chunk_issue(ra, tiles, XCH, xc + 2, lane);
            if (xc + 1 < XCH) chunk_commit(rb, lds[1], lane);
            __syncthreads();
            if (xc + 1 < XCH) {
                if (xc + 3 < XCH) chunk_issue(rb, tiles, XCH, xc + 3, lane);
                if (xc + 2 < XCH) chunk_commit(ra, lds[0], lane);
                __syncthreads();
            }
        }
        return;
    }

    // scanner (wave 0)
    const int y = ybk * 64 + lane;
    const int yc = min(y, H - 1);
    double g[5];
    {
        const double* v0 = VS0 + ((int64_t)ps * 5 * H + yc) * 8;
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const double* vc = v0 + (int64_t)c * H * 8;
            double s = vc[0] * (double)(m + 2);
#pragma unroll
            for (int k = 1; k < m; k++) s += vc[k];
            g[c] = s;
        }
    }
    __syncthreads();
    const double scale = 1. / (15 * 15);
    const int sw = lane & 7;
    auto scan8 = [&](int buf, float (&ox)[8], float (&oy)[8]) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int c = 0; c < 5; c++) g[c] += lds[buf][c][lane * 8 + (j ^ sw)];
            const double g11 = g[0] * scale, g12 = g[1] * scale, g22 = g[2] * scale;
            const double h1 = g[3] * scale, h2 = g[4] * scale;
            const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
            ox[j] = (float)((g11 * h2 - g12 * h1) * idet);
            oy[j] = (float)((g22 * h1 - g12 * h2) * idet);
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
// same expressions in the same order as k_hscan (bit-identical) -- and store it through a 16-row transpose.  One barrier per chunk.
// ---------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(384) void k_hscan_lat(const double* __restrict__ D16, const double* __restrict__ VS0,
                                                  float* __restrict__ flow, int npairs, const int* __restrict__ plist)
{
    constexpr int H = W, m = 7;
    constexpr int XCH = d16_xch(W), NYB = d16_nyb(H);
    static_assert(XCH % 2 == 0, "the loader alternates two register sets");
    constexpr int64_t plane = (int64_t)W * H;
    constexpr int GS = 5 * 64 + 2;                        // doubles per column of a g buffer (+ 2: the four columns a solver instruction reads fall on different banks)
    __shared__ __align__(16) double lds[2][5][512];
    __shared__ __align__(16) double gbuf[2][8][GS];
    __shared__ __align__(16) float outb[4][2][16][8];     // per solver wave: [component][row][column of the chunk]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ps = blockIdx.x / NYB, ybk = blockIdx.x - ps * NYB;
    const int p = plist ? plist[ps] : ps;                // ps indexes the scratch, p the pair's flow
    const double* tiles = D16 + ((int64_t)ps * d16_pair_tiles(W) + (int64_t)ybk * 5 * XCH) * 512;   // [c][xc][512]
    if (wave == 1) {
        // loader: chunk xc + 1 is committed to LDS while the scanner walks chunk xc; two chunks further are in flight
        ChunkRegs ra, rb;
        chunk_issue(ra, tiles, XCH, 0, lane);
        chunk_issue(rb, tiles, XCH, 1, lane);
        chunk_commit(ra, lds[0], lane);
        __syncthreads();
        for (int xc = 0; xc < XCH; xc += 2) {
            if (xc + 2 < XCH) chunk_issue(ra, tiles, XCH, xc + 2, lane);
            chunk_commit(rb, lds[1], lane);
            __syncthreads();
            if (xc + 3 < XCH) chunk_issue(rb, tiles, XCH, xc + 3, lane);
            if (xc + 2 < XCH) chunk_commit(ra, lds[0], lane);
            __syncthreads();
        }
        return;
    }
    if (wave == 0) {
        // scanner: cv2's running sums g += D(x), literally; nothing else
        const int yc = min(ybk * 64 + lane, H - 1);
        double g[5];
        const double* v0 = VS0 + ((int64_t)ps * 5 * H + yc) * 8;
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const double* vc = v0 + (int64_t)c * H * 8;
            double s = vc[0] * (double)(m + 2);
#pragma unroll
            for (int k = 1; k < m; k++) s += vc[k];
            g[c] = s;
        }
        __syncthreads();
        const int sw = lane & 7;
        for (int xc = 0; xc < XCH; xc++) {
            const int buf = xc & 1;
#pragma unroll
            for (int j = 0; j < 8; j++) {
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    g[c] += lds[buf][c][lane * 8 + (j ^ sw)];
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
    const double scale = 1. / (15 * 15);
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
            const double g11 = gp[0] * scale, g12 = gp[64] * scale, g22 = gp[128] * scale;
            const double h1 = gp[192] * scale, h2 = gp[256] * scale;
            const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
            ob[0][r16][j] = (float)((g11 * h2 - g12 * h1) * idet);
            ob[1][r16][j] = (float)((g22 * h1 - g12 * h2) * idet);
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

// one FarnebackUpdateFlow_Blur iteration at width W: matrices from the current flow, box sums, solve
// plist (may be null): the launches work on the pairs plist[0 .. np) of the chunk; the double intermediate is indexed by position in the list
template <int W>
void blur_iteration(avd_ctx* ctx, hipStream_t stream, const float* R, float* flow, FbTwoScratch s, int np, const int* plist, bool marks)
{
    constexpr int NSTRIP = (W + kStripW - 1) / kStripW;
    // k_uvp<W, 4> below 320x320 (latency / issue bound levels); at 320x320 k_uv for long clips (every design measured
    // there with 119 pairs lands at ~290-300 us: HBM read/write mix; k_uvp with 2 / 3 / 4 producers 293 / 377 / 340 us)
    // and k_uvp<W, 4> for clips short enough to be resident in one round
    // profiling: HIP events around the two full-resolution kernels (avd_stage_ms 4 and 5)
    auto mark = [&](void) { stage_mark(ctx, marks && W == S); };
    mark();
    const int grid = 8 * ((np + 7) / 8) * NSTRIP;        // (XCD, pair-in-XCD, strip); pairs >= np exit at once
    // at 320x320 the producer / consumer form wins as long as all its workgroups are resident at once (3 per CU,
    // 50 KiB of LDS each): ~170 us per launch instead of ~290 us; beyond that it needs a second residency round
    const bool uvp_fits = np * NSTRIP <= 3 * 256;
    bool latency_shape = false;
    if constexpr (W >= S / 2) {
        // the exact re-run of a few flagged pairs (160 / 320 px): the latency shape (twelve producers: a third of the phases), one workgroup per CU
        if (plist && np * NSTRIP <= 256) {
            latency_shape = true;
            hipLaunchKernelGGL((k_uvp<W, 12>), dim3(grid), dim3(64 * 14), 0, stream, R, (const float*)flow, s.vs, s.vs0, np, plist);
        }
    }
    if (latency_shape) {
    } else if (W < S || uvp_fits) {
        hipLaunchKernelGGL((k_uvp<W, 4>), dim3(grid), dim3(384), 0, stream, R, (const float*)flow, s.vs, s.vs0, np, plist);
    } else {
        hipLaunchKernelGGL(k_uv<W>, dim3(grid), dim3(128), 0, stream, R, (const float*)flow, s.vs, s.vs0, np, plist);
    }
    mark(); mark();
    if constexpr (W >= S / 2) {
        if (latency_shape) {
            hipLaunchKernelGGL(k_hscan_lat<W>, dim3(np * d16_nyb(W)), dim3(384), 0, stream, (const double*)s.vs, (const double*)s.vs0, flow, np, plist);
            mark();
            return;
        }
    }
    hipLaunchKernelGGL(k_hscan<W>, dim3(np * d16_nyb(W)), dim3(128), 0, stream, (const double*)s.vs, (const double*)s.vs0, flow, np, plist);
    mark();
}

}  // namespace

// doubles for np pairs: D as d16_pair_tiles(320) tiles of 64 x 8 per pair, columns 0..6 of vsum as [5][320][8] (smaller levels use the front)
FbTwoScratchSize fb_two_scratch_size(size_t np)
{
    static_assert((size_t)d16_pair_tiles(S) * 512 == 5 * AVD_NPIX + 512, "five channels + one pad tile per pair");
    return {np * (5 * AVD_NPIX + 512), np * 5 * AVD_SMALL * 8};
}

int launch_fb_two(avd_ctx* ctx, hipStream_t stream, int w, const float* R, float* flow, FbTwoScratch s, int np, const int* plist, bool marks)
{
    if (!s.vs || !s.vs0) { ctx->err = "two-kernel Farneback path: scratch not reserved"; return AVD_ERR_ARG; }
    if (fb_dispatch_width(w, [&](auto wc) { blur_iteration<decltype(wc)::value>(ctx, stream, R, flow, s, np, plist, marks); })) return 0;
    ctx->err = "launch_fb_two: unsupported level size";
    return AVD_ERR_ARG;
}
