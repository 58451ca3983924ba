// avd_fbfast.hip -- FarnebackUpdateFlow_Blur (winsize 15), ONE iteration per launch, a pair spread over several
// workgroups, no serial horizontal chain (gfx950).  The default level kernel since round 3 ("fb_mode" = fast).
//
// Reference site: cv2.calcOpticalFlowFarneback(prev, cur, None, 0.5, 3, 15, 3, 5, 1.2, 0), app/analyzers/video.py:45.
//
// What is literal and what is not.  cv2 forms the 15 x 15 box sums of the five normal-equation channels as RUNNING sums:
//   vertical    vsum[x] += (float)(M[y+7][x] - M[y-8][x])      a float difference added to a double, per column
//   horizontal  g       += (vsum[x+7] - vsum[x-8])             doubles
// The vertical chain rounds a FLOAT at every slide, so its value at row y depends on every row above: re-ordering it moves
// the flow by up to 8e-5 px on hard inputs (tools/experiments/fb_tolerance_exp.c, mode 2).  It is kept literal here: one
// "chain" wave per 64 columns walks down the rows exactly as cv2 does (lanes along x: the chain is sequential in y only).
// The horizontal chain only ever adds doubles; forming each window directly, sum of vsum[x-7 .. x+7] in double, differs from
// cv2's running value by a few double ulps (1e-16 relative), which the float cast of the flow swallows: on every input of
// that experiment (smooth clips, scene cuts, white noise, flat boxes) the flow comes out BIT-IDENTICAL to the oracle
// (mode 1: max |delta| = 0; 3e-14 px on a degenerate flat image).  tests/test_gpu_fbfast.py bounds it at 1e-5 px and
// ai_susp at 1e-6 on every geometry the parity suite covers; avd_fbfused.hip stays as fb_mode = exact.
//
// Structure.  The serial scanner wave of avd_fbfused.hip (one wave of 40 lanes walking a dependent double chain over 320
// columns, the pole of that kernel) is gone, and with it the 160 KB transpose buffer that held a workgroup to one per CU
// and a pair to one workgroup.  A workgroup owns a STRIP of a pair: OW output columns plus 7 halo columns on each side
// (recomputed, not exchanged: there is no cross-workgroup dependency inside a launch), all rows.  Columns outside the image
// clamp to the edge column, which is exactly cv2's replicated border of vsum.  Per 64-column block of the strip four waves:
//   N0, N1  normal equations (FarnebackUpdateMatrices up to r2 .. r6) of two image rows each per step -> ring in LDS (float)
//   C       border attenuation and the five products of M (the N waves are the pole of a step, this wave has issue slots to
//           spare), then the literal vertical chain: M rows in, vsum rows (double) out to LDS
//   X       horizontal window sums + 2 x 2 solve + flow stores.  A lane owns FOUR consecutive columns of one row: 18
//           doubles (nine 16-byte LDS reads) per channel give four windows with 21 additions, and a wave covers 4 rows x 64
//           columns per step
// (No touch / prefetch loads: the N waves' own three-entry lead covers the latency, and touching the next rows one dword
// per line from a fourth wave cost 0.16 ms per level: it is the texture-addresser / L1 path that limits this kernel.)
// The LAST launch of the 320-px level writes |flow| for the statistics kernels, and the flow itself only for a call that hands it to its caller (k_fb_fast's
// ST = false: two of the solver wave's three stores per step and 0.8 MB per pair less; -5.7 us of 127.6, profiles/fbfast320_balance_ab.txt).
// The first launch of the 320-px level, and of the 160-px level where a pair is one strip of this same wave mix, has no input flow of its own size: its chain wave forms it from
// the coarser level's flow a few rows ahead of the N waves (UP, role_chain), which saves k_flow_up's full-chip pass (320 px: 37 us for +3.5; 160 px: 12 us alone, 50 us among three
// clips in flight, for +9 us on 119 CUs -- profiles/fold160_pyramid_ab.txt).  Where the 320-px level runs a pair as one workgroup of five blocks there is no LDS left for that
// hand-over and no need of it: each lane sits on an image column, and the N waves form the flow of their own columns in registers (UpN, role_ne; 119 x 210 us instead of
// 238 x 129 us, profiles/fbfast320_wide_up_ab.txt).
// One workgroup barrier per step of 4 rows; N works on group t, C on group t-1, X on group t-2.  A launch is one blur
// iteration: the flow is read from one buffer and written to another (strips of a pair read each other's columns), and the
// next iteration is the next launch.
//
// Bound: VALU issue and the texture addresser together (round-5 counters: VALU issue ~0.54, TA busy ~0.53 of the launch), at
// ~0.4 of the HBM peak (profiles/r05_pmc.json).  Per iteration every frame's R is read once (20 B/px;
// pair p's R1 is pair p+1's R0 and neighbouring pairs share an XCD's L2), the flow is read and written (16 B/px per pair):
// 441 MB at 320 px x 119 pairs.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "avd_internal.h"
#include "avd_fb_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kM = 7;                 // (winsize - 1) / 2

typedef double dbl2 __attribute__((ext_vector_type(2)));

// W level size; NB 64-column blocks per strip; GD lead of the bilinear gather; NPB normal-equation waves per block (1: four
// entries per step, 2: two entries each, 4: one each); XPB solver waves per block (1: four columns per lane, 2: two columns per lane).
// 2 + 1 + 1 waves per block is the throughput shape (320 px: the chip is full and total issue counts); 4 + 1 + 2 is the
// latency shape for the small levels, where a launch is steps x the slowest wave of a step and most CUs are idle anyway.
// 1 + 1 + 1 exists at 320 px as FIVE blocks ("fb_wide320"): the whole pair in one workgroup of 15 waves, every lane on an image column.
template <int W_, int NB_, int GD_ = 1, int NPB_ = 2, int XPB_ = 1>
struct FGeo {
    static constexpr int W = W_, NB = NB_, GD = GD_, NPB = NPB_, XPB = XPB_;
    static constexpr int H = W;
    static constexpr int SW = 64 * NB;               // lane columns of a strip
    static constexpr int WPB = NPB + 1 + XPB;        // waves per block
    static constexpr int NWAVES = WPB * NB;
    static constexpr int EPS = 4 / NPB;              // entries per normal-equation wave and step
    static constexpr int CPL = 4 / XPB;              // columns per solver lane
    // who applies the border attenuation and forms the five products of M: the chain wave where the N waves are the pole of a step
    // (throughput shape, 320 px), the N waves where the chain wave is (latency shape: four N waves per block, one entry each per step)
    static constexpr bool PN = NPB == 4;
    // the strip IS the image row: lane column = image column, nothing clamped and nothing computed twice; the seven replicated border columns on
    // either side exist in the vsum ring only, where the chain waves of the first and the last block leave them (role_chain)
    static constexpr bool WHOLE = SW == W;
    // four waves per SIMD (128 registers): the row part of the input loads' offsets is a scalar (ne_load<true>, avd_fb_device.h)
    static constexpr bool SROW = PN || NWAVES > 12;
    static constexpr int NE = H + kM;                // entries of the vertical chain: image row min(e, H-1)
    static constexpr int NG = (NE + 3) / 4;          // groups of four entries
    static constexpr int T = ((NG + 2 + 3) / 4) * 4; // steps (= barriers): N on group t, C on t-1, X on t-2; the loops unroll by 4
    // doubles per (row slot, channel) line.  Four columns per lane: lanes stride 32 bytes, ROWLEN % 4 == 2 puts the four
    // rows of a solver instruction on different halves of a 32-byte bank pair.  Two columns per lane: lanes stride 16
    // bytes (a row's 16 lanes = one 256-byte bank row), ROWLEN % 32 == 0 keeps the rows of an instruction on it
    // (WHOLE: 8 + 7 replicas + W + 7 replicas; the solver's last chunk reads up to index 8 + W - 4 + 17)
    static constexpr int ROWLEN = WHOLE ? W + 8 + 2 * kM : XPB == 1 ? SW + 18 : ((SW + 18 + 31) / 32) * 32;
    static constexpr int VS_SLOT = 5 * ROWLEN;
    static constexpr int VS_DOUBLES = 8 * VS_SLOT;   // ring of 8 image rows of vsum
    static constexpr int M_SLOT = 5 * 64;            // floats of one row of one block
    static constexpr int M_FLOATS = NB * 8 * M_SLOT; // ring of 8 rows per block
    static constexpr int LDS_DOUBLES = VS_DOUBLES + M_FLOATS / 2;
    // first iteration of a level below the coarsest (UP): the chain wave forms the level's initial flow -- the previous level's
    // flow resized x 2 -- a few rows ahead of the N waves, in a ring of 16 rows x 2 components per block
    static constexpr int F_SLOT = 2 * 64;            // floats of one row of one block
    static constexpr int F_FLOATS = NB * 16 * F_SLOT;
    template <bool UP> static constexpr int lds_doubles() { return LDS_DOUBLES + (UP ? F_FLOATS / 2 : 0); }   // (the flow ring only where an UP form is instantiated)
    static constexpr bool UPN = false;               // (see UpN below)
    static_assert(LDS_DOUBLES * 8 + 8 <= 163840 && NWAVES <= 16, "LDS layout, workgroup size");
    static_assert(H % 4 == 0 && (NPB == 1 || NPB == 2 || NPB == 4) && (XPB == 1 || XPB == 2), "whole groups of image rows");
    static_assert((2 * (GD + 1)) % EPS == 0 && (XPB != 1 || ROWLEN % 4 == 2), "whole steps per loop body; bank layout of the solver's reads");
};

// A geometry whose first launch of a level resizes the coarser level's flow in the NORMAL-EQUATION waves' own registers (role_ne, UPN) instead of the
// chain wave's LDS ring (k_fb_fast's UP): the other two roles, the LDS layout and the barriers are those of a launch that reads a flow of its own size.
// A trait of the geometry, not a template argument of the kernel: the kernels that exist keep their names.
template <typename G>
struct UpN : G {
    static constexpr bool UPN = true;
    static_assert(G::EPS == 4 && G::GD == 1, "one normal-equation wave per block: its entries are consecutive image rows; entry i forms the flow of entry i + 2");
};

// a double of lane `src` (wave-uniform, known when compiled) in every lane
template <int SRC>
__device__ __forceinline__ double lane_value(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)u, SRC), hi = __builtin_amdgcn_readlane((int)(unsigned)(u >> 32), SRC);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
};

// workgroup barrier; debug builds (-DAVD_FBF_DEBUG) account the cycles a wave spends waiting at it
#ifdef AVD_FBF_DEBUG
__device__ long long g_fbf_stamps[16][3];               // [wave][total cycles, cycles at barriers, role] of workgroup 0
#define fb_barrier()                                                      \
    do {                                                                  \
        const long long t0__ = __builtin_amdgcn_s_memtime();              \
        __syncthreads();                                                  \
        fbf_wait += __builtin_amdgcn_s_memtime() - t0__;                  \
    } while (0)
#define FBF_WAIT_DECL long long fbf_wait = 0;
#define FBF_WAIT_OUT(w, role, t0)                                                           \
    if (blockIdx.x == 8 && (threadIdx.x & 63) == 0) {                                       \
        g_fbf_stamps[w][0] = __builtin_amdgcn_s_memtime() - (t0);                           \
        g_fbf_stamps[w][1] = fbf_wait;                                                      \
        g_fbf_stamps[w][2] = role;                                                          \
    }
#else
__device__ __forceinline__ void fb_barrier() { __syncthreads(); }
#define FBF_WAIT_DECL
#define FBF_WAIT_OUT(w, role, t0)
#endif

// ------------------------------------------------------------------------------------------------------------------
// cv2's resize(prev_flow, INTER_LINEAR) * 2 for one lane column, as k_flow_up (avd_farneback.hip) computes it: source coordinate d / 2 - 0.25, weights
// 0.25 / 0.75, the first column with weights (1, 0), the last one copied; vertically the coarse rows are clipped and the weights kept.  Shared by the two
// resizing forms of a launch (the chain wave's, role_chain UP; the normal-equation waves' own, role_ne UPN): the same operations on the same operands.
// ------------------------------------------------------------------------------------------------------------------
// the two coarse values under lane column x: component c of coarse row r (clipped by the caller, up_row)
template <typename Ge>
__device__ __forceinline__ F2 up_load(const float* __restrict__ prev, unsigned pbase, int x, int c, int r)
{
    constexpr int PW = Ge::W / 2, PH = Ge::H / 2;
    const int sx = x == 0 ? 0 : (x - 1) >> 1;            // floor(x / 2 - 0.25), the first column snapped to 0
    const int xs = sx < PW - 2 ? sx : PW - 2;            // an 8-byte load never leaves the row
    return ld_off<F2>(prev, (pbase + (unsigned)(c * PW * PH + r * PW + xs)) * 4u);
}
template <typename Ge>
__device__ __forceinline__ int up_row(int r) { return r < 0 ? 0 : (r > Ge::H / 2 - 1 ? Ge::H / 2 - 1 : r); }

// horizontal blend of N coarse rows (both components) as loaded by up_load
template <typename Ge, int N>
__device__ __forceinline__ void up_hrows(int x, const F2 (&v)[N][2], float (&d)[N][2])
{
    constexpr int W = Ge::W, PW = W / 2;
    const int sx = x == 0 ? 0 : (x - 1) >> 1;
    const bool edge = sx + 1 >= PW;                      // the last column: the value is copied, no weights
    const float a1 = x == 0 ? 0.f : ((x & 1) ? 0.25f : 0.75f), a0 = 1.f - a1;
#pragma unroll
    for (int q = 0; q < N; q++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float lo = sx > PW - 2 ? v[q][c].b : v[q][c].a, hi = v[q][c].b;
            d[q][c] = edge ? lo * 1.f : lo * a0 + hi * a1;
        }
}

// image row y from the blended coarse rows floor(y / 2 - 0.25) = (y - 1) >> 1 (d0) and the one below it (d1)
__device__ __forceinline__ float up_vblend(float d0, float d1, bool odd)
{
    const float b1 = odd ? 0.25f : 0.75f, b0 = 1.f - b1;
    return (d0 * b0 + d1 * b1) * 2.f;
}

// ------------------------------------------------------------------------------------------------------------------
// N: normal equations of entries 4t + 2k, 4t + 2k + 1 at step t (k = 0, 1), columns of one block.
// ------------------------------------------------------------------------------------------------------------------
// GD = entries of lead of the bilinear gather of R1 (its address needs the flow, so it cannot be issued arbitrarily early):
// the gather of entry i + GD is issued while entry i is evaluated, the inputs (flow, R0) of entry i + 2 GD + 1 likewise.
// Slots are statically indexed: the loop body is GD + 1 steps = 2 (GD + 1) entries.
// UP: the flow of this launch is the previous level's, resized: the chain wave leaves row y of it in fring[y & 15] at least
// one step before it is wanted here (see role_chain); it is fetched from there one entry before the gather that needs it.
// ZF (compile time: only the coarsest level's first iteration has it): the flow is known to be zero whatever the buffer holds
// Border-sign criterion (round 5; the second ill-posedness criterion, the first is in role_solve).  cv2's warp is discontinuous at the top / left
// border: at x = 0 a flow dx = -tiny gives x1 = -1, "outside" (the normal equations are formed from R0 alone), dx = +tiny gives x1 = 0, "inside"
// (average with R1); likewise dy at y = 0.  A component below kTinyFlow is of the size of the rounding residue of cv2's own running sums -- its
// sign is an artefact of their summation order, which this kernel does not share -- so where the two branches differ at such a pixel (ne_branch_jump)
// the pair can only be reproduced by the exact kernels: bit 4 + level of flags[p].  Derived on the CPU (tools/experiments/fb_illposed_exp.c,
// border_ind; profiles/r05_experiments.md section 1): it closes the checkerboard residual of round 4 (exactly periodic or static content, where
// the true flow is zero and everything is residue) and fires on no natural / noisy / letterboxed pair of the 3 120-pair experiment.
// chk (wave-uniform): flags are kept and the pair's two frames are not bit-identical (an exact duplicate's zero flow is structural in cv2 too).
// skip (may be null): an LDS word that says, after the workgroup's FIRST barrier, that the pair is flagged already (k_fb_fast) -- every role then returns true
template <typename Ge, bool UP, bool ZF = false>
__device__ __forceinline__ bool role_ne(const float* __restrict__ R, const float* __restrict__ flow, float* __restrict__ mring,
                                        const float* __restrict__ fring, int p, int x, int k, int lane, int* __restrict__ flags, bool chk,
                                        const volatile int* skip)
{
    constexpr bool zf = ZF, UPN = Ge::UPN;
    constexpr int W = Ge::W, GD = Ge::GD, EPS = Ge::EPS;
    static_assert(!(UPN && (UP || ZF)), "one resizing form per launch");
    FBF_WAIT_DECL
#ifdef AVD_FBF_DEBUG
    const long long fbf_t0 = __builtin_amdgcn_s_memtime();
#endif
    constexpr int H = W, plane = W * H;
    constexpr int NGS = GD + 1, NIS = 2 * NGS, U = NIS / EPS;   // gather slots, input slots, steps per loop body
    const unsigned r0base = (unsigned)p * 5u * plane, r1base = r0base + 5u * plane, flbase = (unsigned)p * 2u * plane;
    const float sxn = border_factor(x, W);                 // PN: x part of the border attenuation, a per-lane constant
    auto ent = [&](int i) { return 4 * (i / EPS) + EPS * k + (i % EPS); };  // this wave's i-th entry
    auto row_of = [](int e) { return e < H - 1 ? e : H - 1; };
    NeIn in[NIS];
    NeG g[NGS];
    const bool xz = x == 0;                                // this lane's column decides inside / outside by the sign of dx
    const bool chkx = chk && __builtin_amdgcn_ballot_w64(xz) != 0;   // wave-uniform: only the first block of the first strip holds column 0
    bool ill = false;
    auto gather = [&](const NeIn& s, int row, NeG& gs) __attribute__((always_inline)) { ne_gather(R, r1base, s, x, row, W, H, gs, zf); };
    auto flow_of = [&](int row, NeIn& s) { const float* f = fring + (row & 15) * Ge::F_SLOT + lane; s.dx = f[0]; s.dy = f[64]; };
    auto load_in = [&](int row, NeIn& s) {
        if (UP) ne_load_r0(R, r0base, x, row, W, s);
        else if (UPN) ne_load_r0<Ge::SROW>(R, r0base, x, row, W, s);
        else ne_load<Ge::SROW>(R, flow, r0base, flbase, x, row, W, plane, s);
    };
    // UPN.  This wave's entries are consecutive image rows, and image row y is blended from the coarse rows (y - 1) >> 1 and the next: rows slide over the
    // coarse rows by half a row each.  Entry i forms the flow of entry i + GD + 1 = i + 2, so step t forms rows 4t + 2 .. 4t + 5 from coarse rows 2t .. 2t + 3:
    //   uab[0], uab[1]  rows 2t, 2t + 1, blended horizontally during step t - 1 (one float per component)
    //   uc              row 2t + 2: in flight (rc) since entry 1 of step t - 1, blended at entry 1 of step t
    //   (ud)            row 2t + 3: in flight (rd) since entry 3 of step t - 1, blended at entry 3 of step t; the two then become uab
    // Every coarse load is issued a whole step before its value is wanted and a step and an entry before the first gather that needs its flow; `flow` is the
    // launch's input, so nothing but registers limits the lead.  Coarse rows are clipped at PH - 1: rows H and H + 1, which the last step forms for gathers
    // nobody evaluates, come out as row H - 1 bit for bit (both of their coarse rows are PH - 1, and a b0 + a b1 commutes).
    const unsigned pbase = (unsigned)p * 2u * (W / 2) * (H / 2);
    float uab[2][2], uc[1][2];
    F2 rc[1][2], rd[1][2];
    auto up_form = [&](int t, int j, NeIn& s) __attribute__((always_inline)) {   // j static: the flow of image row 4t + 2 + j
        float f[2];
        if (j == 1) {
            up_hrows<Ge, 1>(x, rc, uc);
#pragma unroll
            for (int c = 0; c < 2; c++) rc[0][c] = up_load<Ge>(flow, pbase, x, c, up_row<Ge>(2 * t + 4));
        }
        float ud[1][2];
        if (j == 3) {
            up_hrows<Ge, 1>(x, rd, ud);
#pragma unroll
            for (int c = 0; c < 2; c++) rd[0][c] = up_load<Ge>(flow, pbase, x, c, up_row<Ge>(2 * t + 5));
        }
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if (j == 0) f[c] = up_vblend(uab[0][c], uab[1][c], false);
            else if (j == 1) f[c] = up_vblend(uab[1][c], uc[0][c], true);
            else if (j == 2) f[c] = up_vblend(uab[1][c], uc[0][c], false);
            else {
                f[c] = up_vblend(uc[0][c], ud[0][c], true);
                uab[0][c] = uc[0][c]; uab[1][c] = ud[0][c];
            }
        }
        s.dx = f[0]; s.dy = f[1];
    };
    bool first = skip != nullptr;                          // the first barrier of this role has not been passed yet
    if (UP) {
        fb_barrier();                                      // the chain wave has filled rows 0 .. 11 of the flow ring
        if (first && *skip) return true;
        first = false;
    }
    [[maybe_unused]] F2 r01[2][2];
    if constexpr (UPN) {                                   // coarse rows 0 .. 3, ahead of the R0 loads: rows 0 and 1 are waited for first
#pragma unroll
        for (int c = 0; c < 2; c++) { r01[0][c] = up_load<Ge>(flow, pbase, x, c, 0); r01[1][c] = up_load<Ge>(flow, pbase, x, c, 1); }
#pragma unroll
        for (int c = 0; c < 2; c++) { rc[0][c] = up_load<Ge>(flow, pbase, x, c, 2); rd[0][c] = up_load<Ge>(flow, pbase, x, c, 3); }
    }
#pragma unroll
    for (int i = 0; i < NIS - 1; i++) load_in(row_of(ent(i)), in[i]);
    if (UP) {
#pragma unroll
        for (int i = 0; i <= GD; i++) flow_of(row_of(ent(i)), in[i]);
    }
    if constexpr (UPN) {                                   // image rows 0 (coarse rows -1 -> 0 and 0) and 1 (0 and 1)
        up_hrows<Ge, 2>(x, r01, uab);
        in[0].dx = up_vblend(uab[0][0], uab[0][0], false); in[0].dy = up_vblend(uab[0][1], uab[0][1], false);
        in[1].dx = up_vblend(uab[0][0], uab[1][0], true);  in[1].dy = up_vblend(uab[0][1], uab[1][1], true);
    }
#pragma unroll
    for (int i = 0; i < GD; i++) gather(in[i], row_of(ent(i)), g[i]);
    auto work = [&](int t, int q) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < EPS; j++) {
            const int i = EPS * t + j, ii = EPS * q + j;                     // ii = i mod NIS, static
            const int e = ent(i);
            // refills first: the gather GD entries ahead goes into the slot the previous entry released, the inputs
            // NIS - 1 entries ahead into the slot of the entry before this one (rows beyond the image clamp to the last)
            gather(in[(ii + GD) % NIS], row_of(ent(i + GD)), g[(ii + GD) % NGS]);
            load_in(row_of(ent(i + NIS - 1)), in[(ii + NIS - 1) % NIS]);
            if (UP) flow_of(row_of(ent(i + GD + 1)), in[(ii + GD + 1) % NIS]);   // for the gather issued with the next entry
            if constexpr (UPN) up_form(t, j, in[(ii + GD + 1) % NIS]);
            __builtin_amdgcn_sched_barrier(0);
            float a[5];                                                      // r2 .. r6: the chain wave attenuates and multiplies (PN: done here)
            ne_finish_r(in[ii % NIS], g[ii % NGS], a, zf);
            if constexpr (!ZF) {                                             // (ZF: the coarsest level's first flow is zero in cv2 as well)
                if (chkx || (chk && e == 0)) {
                    const NeIn& s = in[ii % NIS];
                    const bool tx = chkx && xz && fabsf(s.dx) < kTinyFlow, ty = e == 0 && fabsf(s.dy) < kTinyFlow;
                    if (__builtin_amdgcn_ballot_w64(tx | ty) != 0) {         // cold: rows / columns of residue-sized flow
                        const float jump = ne_branch_jump(s, g[ii % NGS]);
                        ill |= (tx && jump > (s.dx == 0.f ? kJumpMinZero : kJumpMin)) | (ty && jump > (s.dy == 0.f ? kJumpMinZero : kJumpMin));
                    }
                }
            }
            float* dst = mring + (e & 7) * Ge::M_SLOT + lane;
            if constexpr (Ge::PN) {
                float mm[5];
                const int er = row_of(e);
                ne_products(a, sxn * border_factor(er, H), mm);
#pragma unroll
                for (int c = 0; c < 5; c++) dst[c * 64] = mm[c];
            } else {
#pragma unroll
                for (int c = 0; c < 5; c++) dst[c * 64] = a[c];
            }
        }
    };
    constexpr int TN = H / 4;                              // steps that bring image rows in; the rest only keep the barrier count
    int t0 = 0;
    for (; t0 + U <= TN; t0 += U) {
#pragma unroll
        for (int q = 0; q < U; q++) {
            fb_barrier();
            if (first) { first = false; if (*skip) return true; }
            work(t0 + q, q);
        }
    }
#pragma unroll
    for (int q = 0; q < TN % U; q++) {
        fb_barrier();
        work(t0 + q, q);
    }
    for (int t = TN; t < Ge::T; t++) fb_barrier();
    if (chk && __builtin_amdgcn_ballot_w64(ill) != 0 && lane == 0) atomicOr(flags + p, 16 << (Ge::W == 320 ? 0 : Ge::W == 160 ? 1 : Ge::W == 80 ? 2 : 3));
    FBF_WAIT_OUT(threadIdx.x >> 6, k, fbf_t0)
    return false;
}

// ------------------------------------------------------------------------------------------------------------------
// C: cv2's vertical running sums, literally.  Entry e brings image row min(e, H-1) in; from e = 7 on, row e - 15 (row 0
// while the window still touches the top edge) leaves and the vsum row of image row e - 7 is published.
// ------------------------------------------------------------------------------------------------------------------
// UP: the same wave (it has issue slots and registers to spare) also forms the launch's input flow, cv2's
// resize(prev_flow, INTER_LINEAR) * 2 (up_load, up_hrows, up_vblend above).  Group g = rows 4g .. 4g+3 needs the four coarse
// rows 2g-1 .. 2g+2 (clamped); it is written during step g - 3 (groups 0 .. 2 before the first step), read by the N waves
// from step g - 2 on, and its ring slot is reused four steps later.
template <typename Ge>
struct UpRows { F2 v[4][2]; };

template <typename Ge>
__device__ __forceinline__ void up_issue(const float* __restrict__ prev, unsigned pbase, int g, int x, UpRows<Ge>& u)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int r = up_row<Ge>(2 * g - 1 + q);
#pragma unroll
        for (int c = 0; c < 2; c++) u.v[q][c] = up_load<Ge>(prev, pbase, x, c, r);
    }
}

template <typename Ge>
__device__ __forceinline__ void up_finish(float* __restrict__ fring, int g, int x, int lane, const UpRows<Ge>& u)
{
    float d[4][2];
    up_hrows<Ge, 4>(x, u.v, d);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = 4 * g + j;                          // < H: only whole groups of image rows are formed
        const int q0 = j == 0 ? 0 : (j == 3 ? 2 : 1);     // floor(y / 2 - 0.25) - (2g - 1)
        float* dst = fring + (y & 15) * Ge::F_SLOT + lane;
#pragma unroll
        for (int c = 0; c < 2; c++) dst[c * 64] = up_vblend(d[q0][c], d[q0 + 1][c], j & 1);
    }
}

template <typename Ge, bool UP>
__device__ __forceinline__ bool role_chain(const float* __restrict__ mring, double* __restrict__ vsring, float* __restrict__ fring,
                                           const float* __restrict__ prev, int p, int b, int x, int lane, const volatile int* skip)
{
    constexpr int W = Ge::W;
    FBF_WAIT_DECL
#ifdef AVD_FBF_DEBUG
    const long long fbf_t0 = __builtin_amdgcn_s_memtime();
#endif
    constexpr int H = W;
    const float sx = border_factor(x, W);                 // x part of the border attenuation: a per-lane constant
    float ring[16][5];                                   // ring[e & 15] = M row of entry e (statically indexed)
    double vs[5] = {0., 0., 0., 0., 0.};
    double* vdst = vsring + 8 + (Ge::WHOLE ? kM : 0) + 64 * b + lane;
    const unsigned pbase = (unsigned)p * 2u * (W / 2) * (H / 2);
    UpRows<Ge> up;
    bool first = skip != nullptr;
    if (UP) {
#pragma unroll
        for (int g = 0; g < 3; g++) { up_issue<Ge>(prev, pbase, g, x, up); up_finish<Ge>(fring, g, x, lane, up); }
        fb_barrier();
        if (first && *skip) return true;
        first = false;
    }
    for (int t4 = 0; t4 < Ge::T; t4 += 4) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int t = t4 + q;
            fb_barrier();
            if (first) { first = false; if (*skip) return true; }
            const bool up_now = UP && 4 * (t + 3) < H;                       // wave-uniform
            if (up_now) up_issue<Ge>(prev, pbase, t + 3, x, up);             // consumed after the chain work of this step
            if (t >= 1) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int e = 4 * (t - 1) + j;
                    const int kk = 4 * ((q + 3) & 3) + j;                    // e & 15, static
                    if (e < Ge::NE) {                                        // wave-uniform
                        const int er = e < H - 1 ? e : H - 1;
                        const float* src = mring + (er & 7) * Ge::M_SLOT + lane;
                        float rr[5], a[5];
#pragma unroll
                        for (int c = 0; c < 5; c++) rr[c] = src[c * 64];
                        if constexpr (Ge::PN) {
#pragma unroll
                            for (int c = 0; c < 5; c++) a[c] = rr[c];          // the N waves left the products themselves
                        } else {
                            ne_products(rr, sx * border_factor(er, H), a);   // FarnebackUpdateMatrices' last lines, moved here from the N waves
                        }
                        if (e == 0) {
#pragma unroll
                            for (int c = 0; c < 5; c++) vs[c] = (double)(a[c] * (float)(kM + 2));
                        } else if (e < kM) {
#pragma unroll
                            for (int c = 0; c < 5; c++) vs[c] += (double)a[c];
                        } else {
                            const bool top = e < 16;                         // the leaving row is still row 0
#pragma unroll
                            for (int c = 0; c < 5; c++) {
                                const float lv = top ? ring[0][c] : ring[(kk + 1) & 15][c];
                                vs[c] += (double)(a[c] - lv);
                            }
                            double* d = vdst + ((e - kM) & 7) * Ge::VS_SLOT;
#pragma unroll
                            for (int c = 0; c < 5; c++) d[c * Ge::ROWLEN] = vs[c];
                            if constexpr (Ge::WHOLE) {
                                // cv2's replicated border of vsum: column 0 (lane 0 of block 0) to the seven slots on its left, column W - 1 (lane 63
                                // of the last block) to the seven on its right -- what the halo lanes of a strip compute for themselves
                                if (b == 0) {                                // wave-uniform
#pragma unroll
                                    for (int c = 0; c < 5; c++) { const double v = lane_value<0>(vs[c]); if (lane < kM) d[c * Ge::ROWLEN - kM] = v; }
                                } else if (b == Ge::NB - 1) {
#pragma unroll
                                    for (int c = 0; c < 5; c++) { const double v = lane_value<63>(vs[c]); if (lane < kM) d[c * Ge::ROWLEN + 64] = v; }
                                }
                            }
                        }
#pragma unroll
                        for (int c = 0; c < 5; c++) ring[kk][c] = a[c];
                    }
                }
            }
            if (up_now) up_finish<Ge>(fring, t + 3, x, lane, up);
        }
    }
    FBF_WAIT_OUT(threadIdx.x >> 6, 2, fbf_t0)
    return false;
}

// ------------------------------------------------------------------------------------------------------------------
// X: window sums of 15 columns, 2 x 2 solve (double, cv2's operation order), flow stores.  Lane = (row r of the group,
// chunk of four output columns).  The strip's lane column u holds image column clamp(xlo + u) with xlo = o0 - 7, and vsum
// of lane column u sits at index u + 8 of its line: the window of output column o0 + i is lane columns i .. i + 14.
// ------------------------------------------------------------------------------------------------------------------
// Ill-posedness flag (round 4).  Where the 2 x 2 normal equations are singular over whole regions the flow is chaotic: the
// ORACLE's own result moves by tens to hundreds of pixels under one ulp of noise on its inputs, and a kernel that re-orders a
// single double addition (this one: the horizontal window sums) cannot follow it.  Such pairs are recognised here and re-run
// by the exact kernels (avd_fbfused.hip, k_fb_rerun) before anything reads their flow.  Criterion, derived on the CPU over
// 1 440 pairs of 24 content families (tools/experiments/fb_illposed_run.py; profiles/r04_experiments.md section 1):
//   (g11 g22 + g12^2) > kCondMax (g11 g22 - g12^2 + 1e-3)   cancellation in the determinant: 1-D structure (ramps, stripes:
//                                                            3e5 .. 1e7; every natural / noise / scene-cut / letterboxed /
//                                                            saturated pair of the experiment: <= 975)
//   max(|fx|, |fy|) > kFlowMax * W                           a displacement beyond what a 15-px window can estimate at this
//                                                            level (the same experiment: <= 0.25 W on well-posed pairs)
// written so that a NaN or a negative determinant also fires.
// ST: the flow is stored (false: the level's last launch when nobody reads its flow -- |flow| in mag_out is all that is kept)
template <typename Ge, bool UP, bool ST = true>
__device__ __forceinline__ bool role_solve(const double* __restrict__ vsring, float* __restrict__ flow_out, float* __restrict__ mag_out,
                                           int* __restrict__ flags, int p, int b, int xi, int lane, int o0, int ow, const volatile int* skip)
{
    FBF_WAIT_DECL
#ifdef AVD_FBF_DEBUG
    const long long fbf_t0 = __builtin_amdgcn_s_memtime();
#endif
    constexpr int W = Ge::W, H = W, plane = W * H, CPL = Ge::CPL, NV = 14 + CPL;
    const int r = lane >> 4, j = 16 * (Ge::XPB * b + xi) + (lane & 15);      // chunk of CPL columns: output columns CPL j ..
    const bool colok = CPL * j < ow;
    float* fl = flow_out + (size_t)p * 2 * plane + o0 + CPL * j;
    const double* vsrc = vsring + 8 + CPL * j;
    bool first = skip != nullptr;
    if (UP) {
        fb_barrier();                                      // the chain wave's fill of the flow ring
        if (first && *skip) return true;
        first = false;
    }
    bool ill = false;
    for (int t4 = 0; t4 < Ge::T; t4 += 4) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int t = t4 + q;
            fb_barrier();
            if (first) { first = false; if (*skip) return true; }
            const int y = 4 * t - 15 + r;
            if (t >= 2 && colok && y >= 0 && y < H) {
                const dbl2* s = reinterpret_cast<const dbl2*>(vsrc + (y & 7) * Ge::VS_SLOT);
                double o[5][CPL];
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    double v[NV];
#pragma unroll
                    for (int i = 0; i < NV / 2; i++) {
                        const dbl2 w2 = s[c * (Ge::ROWLEN / 2) + i];
                        v[2 * i] = w2.x; v[2 * i + 1] = w2.y;
                    }
                    if (CPL == 4) {
                        double A = v[3];
#pragma unroll
                        for (int i = 4; i < 15; i++) A += v[i];
                        // four windows of fifteen from eighteen values in 19 additions: the twelve they share, then the two pairs next to them
                        const double Bl = A + (v[1] + v[2]), Br = A + (v[15] + v[16]);
                        o[c][0] = Bl + v[0];
                        o[c][1] = Bl + v[15];
                        o[c][2] = Br + v[2];
                        o[c][CPL - 1] = Br + v[NV - 1];
                    } else {
                        double A = v[1];
#pragma unroll
                        for (int i = 2; i < 15; i++) A += v[i];
                        o[c][0] = A + v[0];
                        o[c][CPL - 1] = A + v[15];
                    }
                }
                float fx[CPL], fy[CPL];
#pragma unroll
                for (int i = 0; i < CPL; i++) {
                    // cv2 scales the five sums by 1 / 225 and adds 1e-3 to the determinant; the scale cancels in the quotient, so the sums stay as
                    // they are and the 1e-3 becomes 1e-3 * 225^2 (round 5: 14 double operations per column instead of 28; this mode's flow is held
                    // to a tolerance, not to cv2's rounding -- the exact kernels keep cv2's order).  The criterion t1 + t2 <= kCondMax den with
                    // t1 = den - c + t2 reads t2 <= (kCondMax - 1) / 2 den + c / 2.
                    constexpr double kC = 1e-3 * 225. * 225.;
                    const double a = o[0][i], b = o[1][i], d = o[2][i], h1 = o[3][i], h2 = o[4][i];
                    const double t2 = b * b, den = __builtin_fma(a, d, kC - t2);
                    const double idet = recip_newton2(den);
                    fx[i] = (float)(__builtin_fma(a, h2, -(b * h1)) * idet);
                    fy[i] = (float)(__builtin_fma(d, h1, -(b * h2)) * idet);
                    ill |= !(t2 <= __builtin_fma(0.5 * (kCondMax - 1.), den, 0.5 * kC)) | !(fmaxf(fabsf(fx[i]), fabsf(fy[i])) <= kFlowMax * (float)W);
                }
                // last iteration of the 320-px level: |flow| as np.sqrt(fx * fx + fy * fy) forms it in float32 (video.py:46), for the
                // statistics kernels -- they then read 4 bytes per pixel twice instead of 8, and the flow only once, here
                if (mag_out) {
                    float mg[CPL];
#pragma unroll
                    for (int i = 0; i < CPL; i++) { const float a2 = fx[i] * fx[i], b2 = fy[i] * fy[i]; mg[i] = sqrtf(a2 + b2); }
                    float* md = mag_out + (size_t)p * plane + y * W + o0 + CPL * j;
                    if (CPL == 4) *reinterpret_cast<float4*>(md) = make_float4(mg[0], mg[1], mg[2 % CPL], mg[3 % CPL]);
                    else *reinterpret_cast<float2*>(md) = make_float2(mg[0], mg[1]);
                }
                float* dst = fl + y * W;
                if constexpr (!ST) {
                } else if (CPL == 4) {
                    *reinterpret_cast<float4*>(dst) = make_float4(fx[0], fx[1], fx[2 % CPL], fx[3 % CPL]);
                    *reinterpret_cast<float4*>(dst + plane) = make_float4(fy[0], fy[1], fy[2 % CPL], fy[3 % CPL]);
                } else {
                    *reinterpret_cast<float2*>(dst) = make_float2(fx[0], fx[1]);
                    *reinterpret_cast<float2*>(dst + plane) = make_float2(fy[0], fy[1]);
                }
            }
        }
    }
    if (flags && __builtin_amdgcn_ballot_w64(ill) != 0 && lane == 0) atomicOr(flags + p, 1 << (Ge::W == 320 ? 0 : Ge::W == 160 ? 1 : Ge::W == 80 ? 2 : 3));
    FBF_WAIT_OUT(threadIdx.x >> 6, 3, fbf_t0)
    return false;
}

// between two phases of a launch that hand the flow over through global memory (prologue -> first iteration, iteration -> next
// iteration) INSIDE one workgroup: its waves share the CU's write-through L1, so workgroup scope is all it takes (the stores have
// left the wave, every wave has arrived).  Agent scope here costs a write-back of the L2 per phase on this chip (the XCDs' L2s are
// not coherent with each other): the 80-px level took 158 instead of 79 us with it.
__device__ __forceinline__ void phase_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// UP  (320 px, and 160 px as one strip per pair): flow_in is the PREVIOUS level's flow ([pair][2][H/2][W/2]); the chain wave forms the launch's input flow from it on the
//     fly, a few rows ahead of the normal-equation waves (LDS ring).
// PRO (160 / 80 px): flow_in is the previous level's flow as well, but the whole workgroup resizes it in a PROLOGUE into flow_tmp (the
//     columns its own lanes read; strips of one pair write identical values where they overlap) -- at these sizes the chain wave is the
//     pole of a step and cannot take the resize on, while a prologue costs ~1 us and saves k_flow_up's launch.
// IT  iterations inside the launch (levels whose pairs are ONE strip: no other workgroup reads this one's flow): the flow ping-pongs
//     between flow_out and flow_tmp through L2, one workgroup barrier between iterations; the result is in flow_out (IT odd).
// ST  false: the flow itself is not stored, only |flow| (IT = 1 with mag_out: the 320-px level's last launch of a call that wants no dense flow)
// Ge = UpN<...> (320 px, five blocks): flow_in is the PREVIOUS level's flow as under UP, resized by each normal-equation wave for its own columns in
//     registers (role_ne); UP is false, and the chain and solver waves run as in a launch that reads a flow of its own size.
template <typename Ge, bool UP, int IT = 1, bool PRO = false, bool ST = true>
__global__ __launch_bounds__((64 * Ge::NWAVES)) void k_fb_fast(const float* __restrict__ R, const float* flow_in, float* flow_out, float* flow_tmp,
                                                              float* __restrict__ mag_out, int* __restrict__ flags, const int* __restrict__ pairdiff,
                                                              int npairs, int nstrips, int ow, int zero_first)
{
    constexpr int W = Ge::W, NB = Ge::NB;
    static_assert(IT == 1 || IT == 3, "one iteration per launch, or all three");
    static_assert(!(UP && (PRO || IT > 1 || Ge::PN)), "the chain wave's resize belongs to one-iteration launches of the throughput shape");
    static_assert(ST || (IT == 1 && !UP && !PRO), "only a level's last launch may leave its flow unwritten");
    static_assert(Ge::template lds_doubles<UP>() * 8 + 8 <= 163840, "LDS layout");
    static_assert(!(Ge::WHOLE && (UP || PRO || IT > 1)), "a pair as one workgroup at 320 px: no room for the chain wave's flow ring, no prologue, one iteration");
    static_assert(!(Ge::UPN && (UP || PRO || IT > 1 || !ST)), "the normal-equation waves' own resize (UpN): flow_in is the coarser level's flow, one iteration, stored");
    __shared__ __align__(16) double lds[Ge::template lds_doubles<UP>()];
    double* vsring = lds;
    float* mrings = reinterpret_cast<float*>(lds + Ge::VS_DOUBLES);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // (XCD group, pair inside the group, strip): an XCD's L2 serves a contiguous run of pairs -- pair p gathers as R1 the
    // frame pair p + 1 reads as R0 -- and all strips of a pair; workgroups are dealt round-robin to the 8 XCDs
    const int ppx = (npairs + 7) >> 3;
    const int local = blockIdx.x >> 3;
    const int p = (blockIdx.x & 7) * ppx + local / nstrips;
    const int s = local % nstrips;
    if (p >= npairs) return;                              // whole workgroup
    const int o0 = s * ow;
    const int width = o0 + ow <= W ? ow : W - o0;         // output columns of this strip (multiples of 4)
    // Waves w, w + 4, w + 8 of a workgroup share a SIMD.  VALU issue cycles per step of four rows (ISA of the loops, tools/isa_loop_table.py): X 849
    // (159 double instructions), N 329-335, C 307: with NB = 3 the SIMDs get {X, N1, C} of block 0, 1, 2 and {N0, N0, N0} -- 1485 / 1485 / 1485 / 987 of
    // the ~3200 cycles a step takes.  The slack of the fourth SIMD cannot be used by moving work into its waves: the N waves are the pole of a step (they
    // wait for their gathers, not for issue slots), and whatever they do after the gather arrives lengthens the step.  Letting the k == 0 wave finish its
    // own two rows (border attenuation and products; 1405 / 1227 on paper) made the launches 1.3-1.9 us SLOWER (profiles/fbfast320_balance_ab.txt;
    // round 4 had found the same change neutral, profiles/r04_experiments.md section 2c)
    // role: 0 .. NPB-1 normal equations, NPB the chain, NPB+1 .. solvers
    int b, role;
    if (NB == 3 && Ge::WPB == 4) {
        const int pos = wave & 3, grp = wave >> 2;
        b = pos == 3 ? grp : pos;
        role = pos == 3 ? 0 : (grp == 0 ? 3 : (grp == 1 ? 1 : 2));
    } else if (NB == 5 && Ge::WPB == 3) {
        // 15 waves, waves w, w + 4, w + 8, w + 12 share a SIMD: {X0, X1, C0, C1}, {X2, X3, C2, C3}, {X4, N0, N1, C4}, {N2, N3, N4} (role and block).
        // VALU issue cycles per step from this shape's ISA (tools/isa_loop_table.py): X 849 (the two-strip shape's loop, instruction for instruction), N 650 (four
        // entries: 325 VALU instructions and 40 loads; two waves of the two-strip shape are 2 x 329), C 307 as before plus, in blocks 0 and 4, ten v_readlane and
        // five masked LDS stores per row for the replicas: 2312 / 2312 / 2456 / 1950 per SIMD of a step that measures ~5 900 cycles (203 us / 84 steps; the two-strip
        // shape: 1485 of ~3 500).  No spills, no scratch: 128 VGPRs, 160 648 B of LDS (profiles/fbfast320_wide_ab.txt)
        //   wave   0  1  2  3  4  5  6  7  8  9 10 11 12 13 14
        //   role   X  X  X  N  X  X  N  N  C  C  N  N  C  C  C     (N = 0, C = 1, X = 2: two bits per wave)
        //   block  0  2  4  2  1  3  0  3  0  2  1  4  1  3  4     (three bits per wave)
        constexpr unsigned kRole = 2u | 2u << 2 | 2u << 4 | 0u << 6 | 2u << 8 | 2u << 10 | 0u << 12 | 0u << 14 | 1u << 16 | 1u << 18 | 0u << 20 | 0u << 22
                                   | 1u << 24 | 1u << 26 | 1u << 28;
        constexpr unsigned long long kBlock = 0ull | 2ull << 3 | 4ull << 6 | 2ull << 9 | 1ull << 12 | 3ull << 15 | 0ull << 18 | 3ull << 21 | 0ull << 24
                                              | 2ull << 27 | 1ull << 30 | 4ull << 33 | 1ull << 36 | 3ull << 39 | 4ull << 42;
        role = (int)(kRole >> (2 * wave)) & 3;
        b = (int)(kBlock >> (3 * wave)) & 7;
    } else {
        b = wave / Ge::WPB;
        role = (wave % Ge::WPB + b) % Ge::WPB;            // rotate the roles over a block's waves: every SIMD gets a mix
    }
    const int xu = (Ge::WHOLE ? 0 : o0 - kM) + 64 * b + lane;   // image column of this lane (clamped: replicated border; WHOLE: the lane's own column)
    const int x = Ge::WHOLE ? xu : (xu < 0 ? 0 : (xu > W - 1 ? W - 1 : xu));
    float* mring = mrings + b * 8 * Ge::M_SLOT;
    float* fring = reinterpret_cast<float*>(lds + Ge::LDS_DOUBLES) + b * 16 * Ge::F_SLOT;   // UP only
    // ONE lane reads the pair's flag word (every thread reading it for itself could see different values while another strip of the pair raises it:
    // waves of one workgroup would part ways at a barrier)
    __shared__ int s_skip;
    if (flags && role == Ge::NPB + 1 && b == 0 && lane == 0) s_skip = __builtin_nontemporal_load(flags + p);
    if (PRO) {
        // columns any lane of this strip reads: [o0 - 7, o0 - 7 + 64 NB) clamped to the image, widened to whole chunks of four
        constexpr int H = W, plane = W * H, pplane = (W / 2) * (H / 2);
        const int c_lo = (o0 - kM < 0 ? 0 : o0 - kM) >> 2, c_hi = (o0 - kM + 64 * NB - 1 > W - 1 ? W - 1 : o0 - kM + 64 * NB - 1) >> 2;
        const int nq = c_hi - c_lo + 1;
        for (int item = threadIdx.x; item < 2 * H * nq; item += 64 * Ge::NWAVES) {
            const int q = c_lo + item % nq, dy = (item / nq) % H, c = item / (nq * H);
            float o[4];
            flow_up_chunk<W>(flow_in + ((size_t)p * 2 + c) * pplane, dy, q, o);
            *reinterpret_cast<float4*>(flow_tmp + ((size_t)p * 2 + c) * plane + dy * W + q * 4) = make_float4(o[0], o[1], o[2], o[3]);
        }
        phase_sync();
        if (flags && s_skip) return;                       // (behind the prologue's own barrier: workgroup-uniform)
    }
    // A pair that an earlier launch (or another strip, a moment ago) has flagged is re-run by the exact kernels whatever happens here: the workgroup
    // leaves (a clip of nothing but such pairs then costs the exact mode's time, not the sum of both).  The flag word is read by ONE lane of a solver wave
    // -- which has nothing to do during the first two steps -- into LDS, and every role looks at it after the workgroup's first barrier: the read's
    // latency hides behind the normal-equation waves' first loads instead of standing in front of them (at the head of the kernel it cost 1.5-2.5 % of the launch)
    const volatile int* skip = (flags && !PRO) ? &s_skip : nullptr;
    const float* fin0 = PRO ? flow_tmp : flow_in;
    if (role < Ge::NPB) {
        // border-sign criterion: not for a pair of bit-identical frames (the pyramid kernel left "frame p differs from frame p + 1" per tile)
        bool chk = flags != nullptr;
        if (chk && pairdiff) chk = __builtin_amdgcn_ballot_w64(lane < kPairDiffTiles && pairdiff[p * kPairDiffTiles + (lane < kPairDiffTiles ? lane : 0)] != 0) != 0;
#pragma unroll 1
        for (int it = 0; it < IT; it++) {
            if (it > 0) phase_sync();
            const float* fin = it == 0 ? fin0 : ((it & 1) ? flow_out : flow_tmp);
            const volatile int* sk = it == 0 ? skip : nullptr;
            if (Ge::W == 40 && zero_first != 0 && it == 0) { if (role_ne<Ge, UP, Ge::W == 40>(R, fin, mring, fring, p, x, role, lane, flags, chk, sk)) return; }
            else if (role_ne<Ge, UP, false>(R, fin, mring, fring, p, x, role, lane, flags, chk, sk)) return;
        }
    } else if (role == Ge::NPB) {
        __builtin_amdgcn_s_setprio(3);    // the only sequential part: take the issue slot whenever ready
#pragma unroll 1
        for (int it = 0; it < IT; it++) {
            if (it > 0) phase_sync();
            if (role_chain<Ge, UP>(mring, vsring, fring, flow_in, p, b, x, lane, it == 0 ? skip : nullptr)) return;
        }
    } else {
#pragma unroll 1
        for (int it = 0; it < IT; it++) {
            if (it > 0) phase_sync();
            if (role_solve<Ge, UP, ST>(vsring, (it & 1) ? flow_tmp : flow_out, it == IT - 1 ? mag_out : nullptr, flags, p, b, role - Ge::NPB - 1, lane, o0, width,
                                   it == 0 ? skip : nullptr)) return;
        }
    }
}

// the instantiation that L describes (launch_fb_fast has checked that it exists at this width)
template <typename Ge>
void launch_fast(hipStream_t stream, const float* R, const FbFastLaunch& L, float* mag, int np, int nstrips, int ow)
{
    const int grid = 8 * ((np + 7) / 8) * nstrips;
    const dim3 g(grid), t(64 * Ge::NWAVES);
    const int zero_first = L.from == FbFlowFrom::zero;
    auto go = [&](auto kernel, int zf) { hipLaunchKernelGGL(kernel, g, t, 0, stream, R, L.flow_in, L.flow_out, L.flow_tmp, mag, L.flags, L.pairdiff, np, nstrips, ow, zf); };
    // the chain wave's resize only exists where it pays: in the throughput shape (2 + 1 + 1 waves per block: the chain wave has issue slots to
    // spare).  At 320 px it costs the launch 3.5 us and saves k_flow_up's 37; the 160-px level's one-strip shape is the same wave mix.  The
    // latency shapes are bound by exactly the chain wave that would do it (160 px, two strips: 45 -> 84 us per launch against 12 saved).
    // The five-block shape of the 320-px level has no LDS left for the flow ring (160 648 B of 163 840 without it) and needs none: every lane sits on an
    // image column, so its normal-equation wave resizes the flow of its own columns in registers (UpN) -- FbFlowFrom::chain names both forms
    const bool pro = L.from == FbFlowFrom::prologue, three = L.iterations == 3;
    if constexpr ((Ge::W == 320 && !Ge::WHOLE) || (Ge::W == 160 && !Ge::PN)) { if (L.from == FbFlowFrom::chain) return go(k_fb_fast<Ge, true>, 0); }
    if constexpr (Ge::W == 320 && Ge::WHOLE) { if (L.from == FbFlowFrom::chain) return go(k_fb_fast<UpN<Ge>, false>, 0); }
    if constexpr (Ge::W == 160 || Ge::W == 80) { if (pro && !three) return go(k_fb_fast<Ge, false, 1, true>, 0); }
    if constexpr (Ge::W == 80) { if (pro && three) return go(k_fb_fast<Ge, false, 3, true>, 0); }
    if constexpr (Ge::W == 80 || Ge::W == 40) { if (three) return go(k_fb_fast<Ge, false, 3, false>, zero_first); }
    if constexpr (Ge::W == 320) { if (!L.store_flow) return go(k_fb_fast<Ge, false, 1, false, false>, zero_first); }
    go(k_fb_fast<Ge, false>, zero_first);
}

}  // namespace

// Blur iterations of one pyramid level for `np` pairs (L: avd_internal.h): R = polynomial expansions of np + 1 frames ([frame][y][x][5]), flows planar [pair][2][y][x]
// L.flags (may be null): int[np]; bit k of flags[p] is set when level k (0 = 320 px) of pair p met the solver's ill-posedness criterion, bit 4 + k when it met
// the border-sign criterion; a pair whose word is already non-zero is skipped.  L.pairdiff (may be null): int[np][kPairDiffTiles], non-zero where frame p
// differs from frame p + 1 (k_pyramid_all): bit-identical pairs are exempt from the border-sign criterion
int launch_fb_fast(avd_ctx* ctx, hipStream_t stream, int w, const float* R, const FbFastLaunch& L, int np)
{
    if (np <= 0) return 0;
    // the combinations that exist (k_fb_fast's template arguments, launch_fast)
    const bool one = L.iterations == 1, three = L.iterations == 3;
    const bool ok = L.from == FbFlowFrom::level || L.from == FbFlowFrom::zero ? (one || (three && (w == 80 || w == 40)))
                  : L.from == FbFlowFrom::chain ? (one && (w == 320 || (w == 160 && L.wide160)))      // 160 px: the one-strip shape only
                  : (one ? (w == 160 || w == 80) : (three && w == 80));      // prologue
    if (!ok) { ctx->err = "launch_fb_fast: this mode does not exist at this level size"; return AVD_ERR_ARG; }
    const bool uses_tmp = three || L.from == FbFlowFrom::prologue;
    if (!L.store_flow && !(w == 320 && one && L.from == FbFlowFrom::level && L.mag_out)) { ctx->err = "launch_fb_fast: only the 320-px level's last launch can leave its flow unwritten"; return AVD_ERR_ARG; }
    if (L.wide320 && !(w == 320 && one && (L.from == FbFlowFrom::level || L.from == FbFlowFrom::chain))) { ctx->err = "launch_fb_fast: the five-block shape exists for the 320-px level's one-iteration launches from a flow of its own size or the 160-px level's"; return AVD_ERR_ARG; }
    if (L.flow_in == L.flow_out || (uses_tmp && (!L.flow_tmp || L.flow_tmp == L.flow_out))) { ctx->err = "launch_fb_fast: the flow is not updated in place"; return AVD_ERR_ARG; }
    switch (w) {
    case 320:
        // (neighbour-shared gathers -- each lane loads its left pixel, the right one comes from lane + 1 by a DPP wave shift -- were built,
        // bit-identical and slower, 164 us per launch against 142: profiles/r04_experiments.md section 2; the code is in the history, commit 3e8b43a)
        // two shapes for the launches that read a 320-px flow (FbFastLaunch::wide320, decided per call like wide160: "fb_wide320"): two strips of three blocks,
        // 12 waves each -- 384 lane columns per pair, 14 halo columns computed twice, half a solver wave masked -- or the pair as ONE workgroup of five blocks,
        // 15 waves: 320 lanes on 320 columns, 5/6 of the wave rows of every role, one normal-equation wave per block with four entries per step.  Every column
        // is computed by the same instructions on the same operands, and the solver's chunks of four start at multiples of 4 in both: bit-identical on any content.
        // Measured (profiles/fbfast320_wide_ab.txt): 120 workgroups x (207 + 199) us against 238 x (127 + 122) us for the level's second and third launch, -18 % CU-microseconds;
        // three clips in flight +2.5 % frames/s; one clip alone is 0.16 ms slower, which is why the shape is chosen per call.  The resizing first launch
        // (FbFlowFrom::chain) has both shapes as well; which one it takes is the schedule's decision ("fb_wide320_up", fast_levels).
        if (L.wide320) launch_fast<FGeo<320, 5, 1, 1, 1>>(stream, R, L, L.mag_out, np, 1, 320);
        else launch_fast<FGeo<320, 3, 2, 2, 1>>(stream, R, L, L.mag_out, np, 2, 160);
        break;
    case 160:
        // two shapes (ctx->fb_wide160; default 2 = chosen per call, see below): a pair as ONE strip of three blocks with the 320-px level's wave mix (119 workgroups of 12 waves,
        // 58 us per launch) or as two 80-column strips of 14 waves (238 workgroups, 48 us per launch).  The narrow shape finishes a launch sooner
        // (one clip alone: -25 us); the wide one costs fewer CU-microseconds (119 x 58 against 238 x 48: lanes 91 % instead of 73 % on image
        // columns, 14 halo columns per pair instead of 28) and that is what counts with clips in flight: +2.4 % frames/s.  The two differ in the
        // grouping of the solver's window sums (four columns per lane against two): bit-identical on well-posed content, like the 320-px level.
        // Which of the two a call takes is decided once, when the call is enqueued (FlowCall::wide160, avd_capi.hip): all launches of the call,
        // and the schedule that chooses where the first one's flow comes from (fast_levels), read the same answer.
        if (L.wide160) launch_fast<FGeo<160, 3, 2, 2, 1>>(stream, R, L, nullptr, np, 1, 160);
        else launch_fast<FGeo<160, 2, 1, 4, 2>>(stream, R, L, nullptr, np, 2, 80);
        break;
    case 80: launch_fast<FGeo<80, 2, 1, 4, 2>>(stream, R, L, nullptr, np, 1, 80); break;
    case 40: launch_fast<FGeo<40, 1, 1, 4, 2>>(stream, R, L, nullptr, np, 1, 40); break;
    default: ctx->err = "launch_fb_fast: unsupported level size"; return AVD_ERR_ARG;
    }
    HIP_TRY(ctx, hipGetLastError());
#ifdef AVD_FBF_DEBUG
    static const int stamps_w = [] { const char* e = std::getenv("AVD_FBF_STAMPS"); return e ? std::atoi(e) : 0; }();
    static int printed = 0;
    if (stamps_w == w && printed++ == 10) {
        long long h[16][3];
        (void)hipStreamSynchronize(stream);
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fbf_stamps), sizeof(h)) == hipSuccess)
            for (int i = 0; i < 16; i++)
                if (h[i][0])
                    fprintf(stderr, "fbfast stamps w=%d wave %2d role %lld: total %lld cycles, at barriers %lld (%.1f %%)\n", w, i, h[i][2], h[i][0],
                            h[i][1], 100. * h[i][1] / h[i][0]);
    }
#endif
    return 0;
}
