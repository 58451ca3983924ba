// avd_internal.h -- shared declarations of libavd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/avd.h"
#include "avd_ingest_clip.h"      // IngestClip: one clip of an ingest call, its argument check and its staging plan (host only)
#include "avd_stream_plan.h"      // where the clips of a call lie when some continue a stream slot (host only)
#include "avd_audio_plan.h"       // the tracks, window table and table arena of one avd_audio_features call (host only)
#include "avd_audio_resample.h"   // the converter in front of it (option "audio_rate"): ratios, filter bank, output ranges, tile table (host only)
#include "avd_audio_stream.h"     // a track continued across calls (option "audio_slot"): what one call of it forms, hands out and holds back (host only)
#include "avd_audio_map.h"        // several continued tracks in one call (option "audio_track_slot"): regions, window / tile / source tables, gather and save lists (host only)
#include "avd_ingest_group.h"     // which clips of a call share an ingest launch (option "ingest_group"), and kLapSlots (host only)

#define AVD_FB_LEVELS 4            // pyramid scales 1/8,1/4,1/2,1 of 320 (see avd_farneback.hip)
#define AVD_NPIX (AVD_SMALL * AVD_SMALL)
constexpr int kPairDiffTiles = 20;   // tiles per frame of the pyramid kernel's 160-px scale: each leaves "frame f differs from frame f + 1 here"

#define HIP_TRY(ctx, expr)                                                         \
    do {                                                                           \
        hipError_t e__ = (expr);                                                   \
        if (e__ != hipSuccess) {                                                   \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);       \
            return AVD_ERR_DEVICE;                                                 \
        }                                                                          \
    } while (0)

// ---- host-built resampling tables (avd_tables.cpp) ------------------------------
// INTER_LINEAR uint8 -> 320x320 (cv2.resize default, reference video.py:43)
struct LinearTab {
    std::vector<int> x0, x1, y0, y1;          // clipped source indices
    std::vector<short> a0, a1, b0, b1;        // 11-bit fixed-point weights
};
void build_linear_tab(int src_h, int src_w, int dst_h, int dst_w, LinearTab& t);
// the output rows each band of rows_per_band source rows forms: [band_dy[b], band_dy[b + 1]), nbands + 1 entries, the last one dst_h
void build_band_dy(const LinearTab& t, int src_h, int rows_per_band, std::vector<int>& band_dy);

// INTER_AREA uint8 -> 32x32 (reference video.py:6): per destination index a run of
// consecutive source indices with (first, middle, last) float weights.
struct AreaAxis {
    std::vector<int> begin, count;
    std::vector<float> w_first, w_mid, w_last;
};
struct AreaTab {
    AreaAxis x, y;
    int fast;          // both scales integral: integer box sums (ResizeAreaFast)
    int iscale_x, iscale_y;
};
int build_area_tab(int src_h, int src_w, int dst_h, int dst_w, AreaTab& t);   // <0: unsupported

// Farneback constant tables (polynomial expansion kernels, pyramid Gaussian kernels)
struct FbConsts {
    float g[11], xg[11], xxg[11];      // centre at index 5 (poly_n = 5)
    double ig11, ig03, ig33, ig55;
    float gk[AVD_FB_LEVELS][19];       // per-level Gaussian taps, level index = pyramid k
    int gksize[AVD_FB_LEVELS];
    double gd[6], xxgd[6];             // g[5 + q], xxg[5 + q] as doubles (the same values): scalar operands of the expansion's double multiply-adds
};
void build_fb_consts(FbConsts& c);

// libswscale's C yuv420 -> BGR24 conversion in integer form (avd_tables.cpp, yuv2rgb.c semantics, BT.601, limited or full range):
//   value = clip8((c0 + (Y + off) * cy) >> 16),  off_r = ((V*crv)>>16) - (crv>>9),  off_b likewise with U and cbu,
//   off_g = ((U*cgu)>>16) - (cgu>>9) + ((V*cgv)>>16) - (cgv>>9)   (arithmetic shifts: cgu, cgv are negative)
// bias, ntab: the gray tables of the table fills (avd_preprocess.hip) hold entry Y + off at index Y + off + bias of ntab entries
struct YuvConsts { int cy, crv, cbu, cgu, cgv, c0, kr, kb, kg, bias, ntab; };   // kr = -(crv>>9), kb = -(cbu>>9), kg = -(cgu>>9) - (cgv>>9)
void build_yuv_consts(YuvConsts& c, bool full_range);
void yuv_index_window(const YuvConsts& c, int& lo, int& hi);      // min and max of Y + off over Y, U, V in 0 .. 255

// ---- device-side parameter blocks ------------------------------------------------
struct LinTap { short i0, i1, w0, w1; };   // two source indices + 11-bit weights of one output row/column

struct PreParams {
    // linear 320: packed per-column and per-row taps
    const LinTap *lxt, *lyt;           // [320] each
    const int* band_dy;                // [nbands+1] first dy owned by each band
    // area x axis (32 entries)
    const int *ax_begin, *ax_count;
    const float *ax_first, *ax_mid, *ax_last;
    int area_fast;
    int area_x_uniform4;               // every x cell: begin%4==0, count%4==0, single weight
    int h, w, rows_per_band, nbands, pitch;
    int64_t row_stride, frame_stride;
};

struct HashParams {
    const int *ay_begin, *ay_count;
    const float *ay_first, *ay_mid, *ay_last;
    int area_fast, fast_area, fast_simd_w;   // fast: integer sums; area = iscale_x*iscale_y
    int h;
};

// Band plan of the ingest kernels (avd_preprocess.hip): a workgroup owns rows_per_band full-width rows, its LDS tile rows are `pitch` bytes.
// ni: the NI of the staged kernel (k_preprocess_vec) a 16-byte aligned BGR clip of this width runs (0: odd or too wide a width, the generic kernel).
struct BandPlan { int rows_per_band, pitch, ni; };
BandPlan band_plan(int w);
// What launch_preprocess ran last on a context: read by tests through avd_debug_fetch "ingest_plan" (eight int32 in this order).
enum IngestKernel { kIngestBgrScalar = 0, kIngestBgrVec16, kIngestBgrStaged, kIngestNv12Scalar, kIngestNv12Tables, kIngestI420Scalar, kIngestI420Tables,
                    kIngestNv12Strip, kIngestI420Strip, kIngestPx32Scalar, kIngestPx32Vec16, kIngestRgbpScalar, kIngestRgbpVec16, kIngestRgbpStaged,
                    kIngestYuyvScalar, kIngestYuyvTables, kIngestI422Scalar, kIngestI422Tables, kIngestNv16Scalar, kIngestNv16Tables,
                    kIngestP010Scalar, kIngestP010Tables, kIngestI010Scalar, kIngestI010Tables, kIngestP010Strip, kIngestI010Strip };
static_assert(kIngestP010Scalar == 20 && kIngestI010Strip == 25, "the ids include/avd.h lists");
struct IngestPlan { int h, w, rows_per_band, nbands, pitch, ni, lds_bytes, kernel; };
static_assert(sizeof(IngestPlan) == 8 * sizeof(int), "avd_debug_fetch hands the struct out as int32[8]");
// What the last ingest of a context did; avd_debug_fetch hands each member out under the name beside it.  launch_preprocess records the launch,
// the ingest entries (avd_capi.hip) count the staging of the call.
struct IngestRecord {
    IngestPlan plan{};               // "ingest_plan": the last launch_preprocess
    int launched = 0;                // 0 until the first ingest launch
    int32_t rotate = 0;              // "ingest_rotate": the rotation that launch ran with
    int32_t range = 0;               // "ingest_range": 1 if it ran with full-range conversion constants
    int32_t format = 0;              // "ingest_format": its layout (AVD_FMT_*)
    int32_t list[2] = {0, 0};        // "ingest_list": it took its frame bases from a table of plane pointers (2: a grouped launch, with a table of output frames) / the frames the table held
    int64_t stage_copies = -1;       // "stage_copies": host-to-device staging copies of the last ingest call; -1 until the first one
    int64_t stage_bytes = -1;        // "stage_bytes": bytes that call copied from host memory (0: device input); -1 until the first one
};
// Kernel shape of a CNN convolution launch (avd_cnn.hip), as avd_debug_fetch "cnn_plan" hands it out per convolution: kCnnFolded = no launch
// of its own (the expanding 1x1 of a fused block; the fused launch is recorded at the block's 3x3)
enum CnnShape { kCnnFolded = 0, kCnn128x128, kCnn256x64, kCnn256x128, kCnn256x256, kCnnStem, kCnnConv3Expand, kCnnSlab3Expand };
constexpr int kCnnConvs = 53;      // convolutions of the network, in avd_cnn_set_weights order
// option "cnn_tap": which intermediate avd_cnn_forward copies aside (0 = none); kCnnTapConv0 + i = the output of convolution i
constexpr int kCnnTapImage = 1, kCnnTapConv0 = 2, kCnnTapMaxPool = kCnnTapConv0 + kCnnConvs, kCnnTapPooled = kCnnTapMaxPool + 1;

// ---- owners of device and pinned host memory ------------------------------------------------
// Move-only: pointer + capacity in elements, freed on destruction and on move-assignment.  Converts to its pointer, so
// call sites read as they would with a raw one (ws.d_small + off, kernel arguments, null tests).
struct avd_ctx;
template <typename T, bool kPinned>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;                    // elements
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { reset(); }
    void reset()
    {
        if (p) { if (kPinned) (void)hipHostFree(p); else (void)hipFree(p); }
        p = nullptr; cap = 0;
    }
    // Grow-only: nothing happens while `count` elements fit.  Otherwise the old memory is freed and the buffer is EMPTY until the new
    // allocation exists; a failure sets ctx->err, returns AVD_ERR_NOMEM and leaves it empty.
    int reserve(avd_ctx* ctx, size_t count);
    operator T*() const { return p; }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinBuf = Buf<T, true>;

// Tables and band layout of one frame geometry.  A context keeps the last kGeomCache geometries (a mixed-resolution
// stream alternates between a few sizes): switching between cached geometries allocates and frees nothing.
constexpr int kGeomCache = 4;
struct Geom {
    int h = 0, w = 0;
    DevBuf<uint8_t> d_tables;
    PreParams pre{};
    HashParams hsh{};
    unsigned long long stamp = 0;      // last use (LRU eviction)
};

// One clip of an ingest call, as its launches see it: the geometry it runs with and its slice of the per-frame buffers (a batch concatenates its
// clips).  pre / hsh are COPIES of the geometry's cache entry, not pointers into it: a call with more than kGeomCache geometries evicts entries as it goes.
struct ClipSlot {
    PreParams pre{};
    HashParams hsh{};
    int f0 = 0;                        // first frame of the clip in the [n] buffers
    size_t rowbuf_off = 0, lappart_off = 0;   // its first element of d_rowbuf / d_lap_part
};

// What one Farneback call (all its chunks, and the deferred exact re-run of its last one) runs as: decided once, where the call is enqueued (run_flow_chunks)
struct FlowCall {
    int model;                         // option "cv2_model" as it stood when the call was enqueued: every chunk and the deferred exact re-run follow it
    bool wide160;                      // fast mode: the 160-px level as one three-block strip per pair (see avd_ctx::fb_wide160)
    bool wide320;                      // fast mode: the 320-px level's launches that read a 320-px flow as one five-block workgroup per pair (see avd_ctx::fb_wide320)
    bool dense_flow;                   // the caller fetches the interleaved flow (ws.d_flow_il, reserved): the chunks' flow_tail interleaves it
};
// Option "cv2_model": the oracle's model switches (its header; the same bit values) that the library follows.  What each bit changes in the
// launches is decided by the helpers below and nowhere else.
constexpr int kCv2GaussMuladd = 1, kCv2ThreeScales = 8, kCv2ResizeLerp = 16, kCv2ModelMask = kCv2GaussMuladd | kCv2ThreeScales | kCv2ResizeLerp;
inline int fb_coarsest(int model) { return model & kCv2ThreeScales ? AVD_FB_LEVELS - 2 : AVD_FB_LEVELS - 1; }        // pyramid index of the first level run
// the fold options IN EFFECT (they have no effect on results, so a model whose arithmetic exists in the unfolded kernels only runs those):
// bit 1 -> the 320-px blur comes from the pyramid kernel; bit 16 -> every initial flow comes from k_flow_up (fb_fold_up loses bits 1 and 2);
// bit 8 -> the 80-px level, now the coarsest, runs its iterations one per launch (fb_fold_up loses bit 4: fast_levels says why)
inline int fb_fold_blur_eff(int fold_blur, int model) { return model & kCv2GaussMuladd ? 0 : fold_blur; }
inline int fb_fold_up_eff(int fold_up, int model) { return fold_up & (model & kCv2ResizeLerp ? 4 : 7) & (model & kCv2ThreeScales ? 3 : 7); }
inline int fb_fold_up160_eff(int fold_up160, int model) { return model & kCv2ResizeLerp ? 0 : fold_up160; }
// What launch_farneback left in the Farneback scratch
struct FbChunk {
    const float* flow[AVD_FB_LEVELS] = {};   // the final flow of each level (d_flow or d_flow2)
    bool mag_valid = false;                  // d_mag holds |flow| of the chunk already (the fast level kernel wrote it)
    // fast mode, a call that wants no dense flow: the 320-px level's last launch wrote |flow| only, flow[0] does not hold its flow yet.  Only
    // avd_debug_fetch "flow0" can ask for it afterwards; launch_flow0_late then repeats that launch with the stores (pairs > 0: pending)
    struct { int pairs = 0; const float* flow_in = nullptr; int* flags = nullptr; const int* pairdiff = nullptr; } flow0_late;
};

// Scratch of a context.  Everything here can be given back (avd_release_workspace resets the struct) and is re-reserved on demand.
struct Workspace {
    // capacities of the per-frame buffers, which only ever grow: cap_n frames validates every [n] buffer below at once (0 until all exist)
    int cap_n = 0;
    Geom geoms[kGeomCache];
    unsigned long long geom_clock = 0;
    int fb_cap = 0;                    // pairs the Farneback scratch holds (0 until every buffer of it exists)
    DevBuf<int> d_clipstart; PinBuf<int> h_clipstart;   // [n] 1 = first frame of a clip
    // preprocess
    DevBuf<uint8_t> d_stage;          // staged host input
    // frame lists (avd_frame_list): the plane pointers of every list of the call, per list [plane][frame] -- device addresses (the caller's
    // planes, or their places in d_stage); filled in the pinned mirror and uploaded ONCE per call, so an asynchronous call owns its copy
    DevBuf<const uint8_t*> d_ftab; PinBuf<const uint8_t*> h_ftab;
    DevBuf<uint8_t> d_small;          // [n][320*320]
    DevBuf<float> d_rowbuf;           // [n][h][32]
    DevBuf<uint8_t> d_area;           // [n][1024]
    DevBuf<uint8_t> d_hash;           // [n][1024]
    DevBuf<unsigned long long> d_lap; // [n][2]
    DevBuf<long long> d_lap_part;     // [n][nbands][kLapSlots][2] per-wave partial moments
    // farneback
    DevBuf<float> d_pyr[AVD_FB_LEVELS];     // [n][hL*wL]
    DevBuf<float> d_poly[AVD_FB_LEVELS];    // [n][hL*wL][5] interleaved polynomial coefficients
    DevBuf<float> d_flow[AVD_FB_LEVELS];    // [n-1][2][hL*wL]  planar
    DevBuf<float> d_flow2[AVD_FB_LEVELS];   // second flow buffer of a level: the fast level kernel (avd_fbfast.hip) ping-pongs
    FbChunk fb_holds{};                   // what the scratch holds: launch_farneback's report of the last chunk; the deferred re-run and avd_debug_fetch "flowK" read it
    DevBuf<float> d_mag;                  // [n-1][320*320] |flow| of the full-resolution level (written by the fast level kernel, or by k_mag in exact mode)
    DevBuf<int> d_fbflags;                // [n-1] ill-posedness flags of the fast level kernels (bit k: level k met the solver's criterion, bit 4 + k: the border-sign criterion); such pairs are re-run exactly
    DevBuf<int> d_pairdiff;               // [n-1][20] "frame p differs from frame p + 1" per tile of the pyramid kernel's 160-px scale (all zero: bit-identical frames)
    DevBuf<int> d_rlist;                  // exact re-run: the flagged pairs of a chunk, compacted by the host
    PinBuf<int> h_rlist;                  // pinned staging of that list
    DevBuf<double> d_vs_rerun, d_vs0_rerun;   // the two-kernel path's double intermediate for kRerunTwoKernelMax pairs (allocated by the first re-run)
    DevBuf<double> d_vs;                  // [n-1] x 64x16 tiles of D = vsum(x+7)-vsum(x-8), double
    DevBuf<double> d_vs0;                 // [n-1][5][320][8]  vsum columns 0..6 (row init)
    DevBuf<float> d_flow_il;              // [n-1][320*320][2] interleaved (cv2 layout); allocated when a caller first asks for the dense flow
    DevBuf<float> d_stats;                // [n-1][2] mean, var
    DevBuf<avd_frame_record> d_rec;       // [n]
    PinBuf<avd_frame_record> h_rec;       // [n] pinned landing buffer of the asynchronous copy-out
    // ViT patch-embed extension (avd_vit.hip): im2col patches, token staging (also the row operations' staging)
    DevBuf<uint16_t> d_vit_patches;
    DevBuf<float> d_vit_tokens;
    // audio analyzer (avd_audio.hip): tables (hanning, twiddles) for the current window lengths, scratch, records
    // d_audio_tab: hann | cos | sin of the full length audio_win, kept across calls.  d_audio_call / h_audio_call: what changes with every call
    // (avd_audio_plan.h: the short lengths' table arena, the window table, the two window lists), filled in the pinned mirror and uploaded in one copy
    DevBuf<double> d_audio_tab; int audio_win = 0;
    DevBuf<double> d_audio_call; PinBuf<double> h_audio_call;
    int audio_upload_pending = 0;         // that copy was enqueued by a call that has not drained the stream since
    DevBuf<double> d_audio_buf;
    DevBuf<avd_audio_window> d_audio_out;
    // the converter in front of the analyzer (option "audio_rate", k_audio_resample): the converted tracks, 16 kHz mono int16, side by side (8 spare
    // entries: its 16-byte rows); the filter bank [U][T] of rate audio_rs_rate, kept across calls; the call's tile table with its pinned mirror (which
    // also carries the bank when the rate changed), uploaded like d_audio_call
    DevBuf<int16_t> d_audio_pcm;
    DevBuf<int> d_audio_rs_taps; int audio_rs_rate = 0;
    DevBuf<avd_resample::Tile> d_audio_rs_tiles; PinBuf<avd_resample::Tile> h_audio_rs;
    int audio_rs_upload_pending = 0;      // that copy was enqueued by a call that has not drained the stream since
    // CNN extension (avd_cnn.hip): activation scratch for cnn_frames frames
    DevBuf<uint16_t> d_cnn_act[4], d_cnn_img;
    DevBuf<float> d_cnn_pool, d_cnn_logits; int cnn_frames = 0;
    // test hook (option "cnn_tap"): the one intermediate the last forward copied aside; reserved only by a tapped forward
    DevBuf<uint16_t> d_cnn_tap;
    int cnn_tap_asked = 0, cnn_tap_point = 0;     // what the last forward was asked for / what it copied (0: nothing, d_cnn_tap is not to be read)
    size_t cnn_tap_rows = 0, cnn_tap_bytes = 0;   // a blocked activation of cnn_tap_rows pixels x cnn_tap_c channels, or (cnn_tap_c == 0) cnn_tap_bytes plain bytes
    int cnn_tap_c = 0;
};

// What a caller uploaded (avd_cnn_set_weights, avd_vit_set_weights) is state, not scratch: it survives avd_release_workspace.
struct Weights {
    // CNN extension: blocked conv weights + linear layer, biases
    DevBuf<uint16_t> d_cnn_w; DevBuf<float> d_cnn_b;
    std::vector<size_t> cnn_w_off; size_t cnn_fc_off = 0;
    // ViT patch embedding: weights [768][768] bf16 + bias
    DevBuf<uint16_t> d_vit_w; DevBuf<float> d_vit_bias; int vit_has_bias = 0;
};

// A stream slot (option "stream_slot") is state too: what the pair (previous, current) reads of the last frame the slot absorbed -- its 320 x 320
// gray image, its 1024 hash bits (one per byte) and its two Laplacian moments, in this order.  An avd_analyze_* call with a slot selected puts
// them in front of its own frames (ClipSlot::f0 = 1) and leaves its last frame here; frames = 0: the slot is empty, whatever d_prev holds.
constexpr int kStreamSlots = 8;
constexpr int kStreamMapPositions = 64;          // option "stream_map": the clip positions of a call that can be mapped to a slot
constexpr size_t kStreamHashAt = AVD_NPIX, kStreamLapAt = AVD_NPIX + 1024, kStreamPrevBytes = kStreamLapAt + 2 * sizeof(unsigned long long);
static_assert(kStreamLapAt % sizeof(unsigned long long) == 0, "the moments are copied as two 64-bit words");
struct StreamSlot {
    DevBuf<uint8_t> d_prev;          // [kStreamPrevBytes]
    int frames = 0;                  // frames absorbed since the slot was last emptied ("stream_frames")
};

// An audio slot (option "audio_slot") is state as well: a track continued across avd_audio_features calls.  On the device, in one allocation:
// two history buffers of kMaxHistory mono int16 frames (the save launch reads one and writes the other; hist_side says which one is current) and
// the held-back analysis samples, fewer than win, in the track's analysis type (int16, or float32 for an unconverted float track).  frames = 0:
// the slot is empty, whatever the memory holds.  The values of its first call bind the track (win, rate, channels, format).
constexpr int kAudioSlots = 8;
constexpr int kAudioSlotHeldWords = 2 * avd_audio::kMaxWin;          // 16-bit words: kMaxWin - 1 float32 samples at most
constexpr size_t kAudioSlotHistAt = 0, kAudioSlotHeldAt = 2 * 1024, kAudioSlotWords = kAudioSlotHeldAt + kAudioSlotHeldWords;   // 36 KB
static_assert(avd_resample::kMaxHistory <= 1024, "a history buffer is 1024 entries");
struct AudioSlot {
    DevBuf<int16_t> d_mem;           // [kAudioSlotWords]
    long long frames = 0;            // input frames absorbed since the slot was last emptied
    int held = 0;                    // analysis samples held back
    int windows = 0;                 // records the last call on the slot wrote
    int hist_side = 0;
    int win = 0, rate = 0, channels = 0, format = 0;
    int layout = 0;                  // option "audio_layout" of the first call (0: none); the plane stride may differ from call to call
    int16_t* hist(int side) { return d_mem.p + kAudioSlotHistAt + 1024 * (size_t)side; }
    int16_t* held_at() { return d_mem.p + kAudioSlotHeldAt; }
    void clear() { frames = 0; held = 0; windows = 0; }
};
// the two-part source of a continued track's converter launch: `wav` holds the track's frames from chunk0 on, hist its hist_n frames below
struct AudioSource { long long chunk0 = 0; const int16_t* hist = nullptr; int hist_n = 0; };
// a call of several tracks (option "audio_track_slot"): one move of its gather launch and one row of its save launch, device addresses throughout
// (avd_audio_map.h plans both in entries; the call path turns them into these).  They travel to their kernels by value.
struct AudioGatherMove { const void* src; void* dst; long long bytes; };
struct AudioSaveRow { const void* wav; long long n; const int16_t* hist_old; int16_t* hist_new; const int16_t* held_src; int16_t* held_dst; int hist_old_n, hist_new_n, held_words, pad; };
static_assert(sizeof(AudioGatherMove) == 24 && sizeof(AudioSaveRow) == 64, "the tables are kernel arguments: 72 moves and 8 rows stay far below 4 KB");

struct avd_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_in = nullptr;                // avd_wait_stream: recorded on the caller's stream, waited for by ours
    avd_frame_record* pending_out = nullptr;   // caller buffer the pinned records are handed to in avd_synchronize
    std::vector<avd_stream::Run> pending_runs; // where they lie in ws.h_rec (avd_stream_plan.h): the call's own frames, without the frames restored from stream slots
    hipEvent_t stage_ev[5] = {};
    hipEvent_t kern_ev[12] = {};           // profiling: level320_mark events around the 320-px level's blur launches of a chunk
    int kern_ev_used = 0;
    int profiling = 0;
    int stage_marks = 0;                       // stage events recorded by the call in flight (5 = all of them)
    // per-kernel profiling (avd_kernel_ms): an event in front of every kernel (group) of the path, labelled with the avd_kernel_id of the
    // region that starts there; elapsed times between consecutive events are summed per id when the call is drained
    hipEvent_t kmark_ev[96] = {};
    hipEvent_t kmark_at[96] = {};              // the event that opens region i: kmark_ev[i], or the stage event recorded at the same place (kmark's `shared`)
    int kmark_id[96] = {};
    int kmark_used = 0;
    int kmark_incomplete = 0;                  // the same for the call whose times kernel_ms holds
    int kmark_overflow = 0;                    // a call recorded more regions than kmark_ev holds (reset when the marks are)
    float kernel_ms[AVD_K_COUNT] = {};
    float stage_ms[6] = {};
    std::string err;
    Workspace ws;
    Weights weights;
    FbConsts fbc;
    DevBuf<FbConsts> d_fbc;         // FbConsts on device
    int last_n = 0;
    IngestRecord ingest;             // what the last ingest of this context did
    int rec_n = 0;                   // records the last avd_analyze_* call left in ws.d_rec (0 after any other entry point: avd_allgather_last_records checks it)
    int rec_off = 0;                 // ... from this entry on (1: the call continued a stream slot)
    int rec_mapped = 0;              // that call ran under a non-empty "stream_map": its own records are not one run of ws.d_rec (avd_allgather_last_records refuses)
    StreamSlot streams[kStreamSlots];   // option "stream_slot" = k selects streams[k - 1]
    int stream_slot = 0;             // 0 = every avd_analyze_* call starts a new clip; k = the call continues the clip slot k holds (one clip per call)
    // option "stream_map": clip position p of every avd_analyze_* call continues slot stream_map[p] (0: it starts a new clip).  A slot is mapped at one
    // position at most, and the map is empty while stream_slot != 0 (avd_set_option refuses either way): the two ways of choosing slots never hold at once
    int stream_map[kStreamMapPositions] = {};
    int stream_mapped = 0;           // positions mapped
    // option "ingest_group": 0 = every clip of an avd_analyze_* call has an ingest launch and a k_hash launch of its own; 1 = the clips of a call that
    // share a key (avd_ingest_group.h: geometry, layout, rotation, range, row strides, 16-byte eligibility) share ONE of each.  Durable; no effect on results
    int ingest_group = 0;
    int ingest_call[4] = {};         // debug buffer "ingest_call", of the last avd_analyze_* call: ingest launches, hash launches, groups of more than one clip, frames ingested by grouped launches
    std::vector<int> ingest_groups;  // debug buffer "ingest_groups", of that call: per launch {first clip position, clips, frames, IngestKernel id}
    int stream_call[4] = {};         // debug buffer "stream_call", of the last avd_analyze_* call: clips that continued a filled slot, restore launches, save launches, frames in the buffers
    void* comm = nullptr;            // RCCL communicator (avd_comm.cpp), bound at run time
    int comm_rank = 0, comm_world = 1;
    DevBuf<char> d_comm;             // device staging of the record exchange
    int cnn_tiles = 0;              // convolution tiling of the CNN extension: 0 = heuristic, 1 = 256-pixel tiles, 2 = 128 x 128 wherever possible
    int cv2_model = 0;              // option "cv2_model" (AVD_CV2_MODEL): mask of kCv2GaussMuladd / kCv2ThreeScales / kCv2ResizeLerp, 0 = the default model; a call follows the value it was enqueued under (FlowCall::model)
    int fb_model[4] = {};           // debug buffer "fb_model", of the last call that ran the Farneback stage: model, scales run (4 or 3), fb_fold_up in effect, fb_fold_blur in effect
    int fb_model_valid = 0;         // 0 until the first such call
    int fb_fold_blur = 1;           // the 320-px scale's 3 x 3 pyramid blur formed inside the polynomial expansion (no effect on results); AVD_FB_FOLD_BLUR / avd_set_option
    int fb_wide160 = 2;             // fast mode: the 160-px level as one three-block strip per pair (1: fewer CU-microseconds, throughput) or as two strips (0: shorter launches, latency);
                                    // 2 (default) = by what is in flight when the call is enqueued: one strip if another context of the process holds an undrained call, two if this clip is alone; AVD_FB_WIDE160 / avd_set_option
    int fb_wide320 = 2;             // fast mode: the launches of the 320-px level that read a 320-px flow (and, under fb_wide320_up, the first one, which reads the 160-px flow) run a pair as ONE workgroup of five 64-column blocks, 15 waves (1: no halo columns,
                                    // no idle solver lanes: 120 x 203 us instead of 238 x 124 us per launch, throughput) or as two strips of three blocks (0: a launch is 80 us shorter, latency);
                                    // 2 (default) = per call by what is in flight, as fb_wide160 = 2.  Bit-identical results on any content (the same instructions on the same operands per
                                    // column); AVD_FB_WIDE320 / avd_set_option
    int fb_wide320_used = 0;        // read-only option "fb_wide320_used": FlowCall::wide320 of the last fast-mode call, written when it is enqueued; no launcher reads it
    int fb_wide320_launches = 0;    // debug buffer "fb_wide320_launches": launches of the last call that ran the Farneback stage (all its chunks) in the five-block shape
                                    // from a 320-px flow
    int fb_wide320_up = 1;          // fast mode: the level's FIRST launch, the one that resizes the 160-px flow itself (fb_fold_up bit 1), follows FlowCall::wide320 too (1) -- its
                                    // normal-equation waves resize the flow of their own columns in registers, the five-block shape has no LDS left for the chain wave's ring -- or
                                    // stays in two strips whatever the call chose (0).  Bit-identical results; AVD_FB_WIDE320_UP / avd_set_option
    int fb_wide320_up_launches = 0; // debug buffer "fb_wide320_up_launches": the same count for the resizing launch in the five-block shape
    int counted_in_flight = 0;      // this context's enqueued call is counted in avd_calls_in_flight()
    int fb_wide160_used = 0;        // read-only option "fb_wide160_used": FlowCall::wide160 of the last fast-mode call, written when it is enqueued; no launcher reads it
    int gemm_waves = 8;             // patch-embed GEMM: waves per workgroup (8: 8 x 4 MFMA tiles per wave, 16: 4 x 4; measured no faster), the same 256 x 256 tile; AVD_GEMM_WAVES / avd_set_option
    int cnn_tap = 0;                // CNN extension, tests: the forward copies one intermediate aside for avd_debug_fetch "cnn_tap" (0 = off, 1 = bordered input image,
                                    // 2 + i = output of convolution i, 55 = max pool, 56 = pooled features); one pass, no timing repetitions
    int cnn_plan[kCnnConvs] = {};   // the kernel shape (CnnShape) each convolution of the last forward ran as (debug buffer "cnn_plan")
    int cnn_plan_valid = 0;         // 0 until the first forward
    int audio_plan[4] = {};         // nwin, win, last, nfull (windows on the 80 x 100 path) of the last avd_audio_features (debug buffer "audio_plan")
    int audio_plan_valid = 0;       // 0 until the first one, and while a later one has not enqueued all its launches
    int audio_tracks[avd_audio::kMaxTracks][3] = {};   // per track of that call: first window, windows, length of the last window (debug buffer "audio_tracks")
    int audio_ntracks = 0;
    int audio_host[2] = {};         // of that call: microseconds the host spent forming the short lengths' tables, and how many distinct lengths (debug buffer "audio_host")
    int audio_format = 0;           // option "audio_format": what `wav` of avd_audio_features points at -- 0 float32 samples, 1 little-endian int16 PCM ((float)s * 2^-15)
    // option "audio_cut": the track boundaries of the NEXT avd_audio_features call, strictly ascending sample positions.  One-shot: that call takes
    // the list whatever becomes of it, so a forgotten list never splits a later call and results do not depend on the context's history
    int audio_cuts[avd_audio::kMaxCuts] = {};
    int audio_ncuts = 0;
    // options "audio_rate" / "audio_channels": wav of avd_audio_features holds n FRAMES of audio_channels interleaved samples at audio_rate, converted
    // on the device to the 16 kHz mono int16 track the analyzer runs over (avd_audio_resample.h); audio_rate 0 = the samples are that track already
    int audio_rate = 0;
    int audio_channels = 1;
    // options "audio_layout" / "audio_plane_stride" (read only while audio_rate != 0): 0 = "audio_channels" decides; otherwise id | flags of
    // avd_audio_resample.h -- 1, 2, 6 or 8 channels in FFmpeg's native order, | 0x100 one plane per channel, plane c beginning c * stride samples
    // behind plane 0 (stride 0: the call's frame count, a dense [channels, n] buffer) -- downmixed by the layout's Q15 weights
    int audio_layout = 0;
    int audio_plane_stride = 0;
    int audio_layout_rec[12] = {};  // debug buffer "audio_layout" of the last call that converted: id, planar, channels, the stride in effect, the eight weights
    int audio_layout_valid = 0;     // 0 until a call converted
    std::vector<int> audio_rs_bank[avd_resample::kNumRates];   // the filter bank of each rate a call has used, built once (avd_resample::build_taps)
    int audio_rs_plan[8] = {};      // debug buffer "audio_rs_plan" of the last avd_audio_features call, if it converted: rate, channels, U, D, T, outputs per tile, input frames, output samples
    int audio_rs_valid = 0;         // 0 while the last call that ran did not convert (or none ran)
    int audio_rs_tracks[avd_audio::kMaxTracks][2] = {};   // per track of that call: first output sample, output samples (debug buffer "audio_rs_tracks")
    int audio_rs_ntracks = 0;
    int audio_rs_pcm_at = 0;        // debug buffer "audio_pcm" begins at this entry of ws.d_audio_pcm (a slot call: behind the held samples)
    // options "audio_slot" (durable: 0 = every avd_audio_features call is a whole track, k = it continues the track of audio_slots[k - 1]) and
    // "audio_end" (one-shot like the cut list: the next call carries the track's last samples)
    AudioSlot audio_slots[kAudioSlots];
    int audio_slot = 0;
    int audio_end = 0;
    // option "audio_track_slot": what each track of the NEXT avd_audio_features call is -- slot | 0x10 (the track ends); one-shot like the cut list.
    // It and a non-zero "audio_slot" never hold at once.
    int audio_map_entries[avd_audio_map::kMaxEntries] = {};
    int audio_map_n = 0;
    int audio_map_call[6] = {};     // debug buffer "audio_map_call" of the last list call: tracks, continued tracks, gather / converter launches, analyzer passes, save launches
    int audio_map_valid = 0;        // 0 until a list call ran
    int audio_rs_mapped = 0;        // the converter's debug state is a list call's: "audio_pcm" is gathered region by region ("audio_rs_tracks")
    int cnn_chunk = 128;            // CNN extension: frames per forward pass (activation scratch = 4 x 1.6 MB per frame)
    int cnn_fuse = 2;               // CNN extension: a block's 3x3 and expanding 1x1 in one launch (stages 1, 2): 2 = with the 3x3's input slab in LDS in the stride-1 blocks (k_slab3_expand), 1 = gathering kernels only, 0 = layer by layer
    int fb_fused = 0xF;             // bit k: pyramid level k runs the fused kernel (avd_fbfused.hip) instead of the two-kernel path (avd_fbtwo.hip)
    int fb_fold_up = 5;             // fast mode, bit mask (no effect on results; AVD_FB_FOLD_UP / avd_set_option): 1 the 320-px level's first launch resizes the
                                    // 160-px flow itself (no k_flow_up<320>), 2 the 160- / 80-px levels do so in a prologue, 4 the 80- / 40-px levels run their three
                                    // iterations in one launch
    int fb_fold_up160 = 1;          // fast mode (no effect on results; AVD_FB_FOLD_UP160 / avd_set_option): the 160-px level's first launch resizes the 80-px flow
                                    // itself in its chain wave, as bit 1 of fb_fold_up does at 320 px (no k_flow_up<160>) -- in the one-strip shape only (FlowCall::wide160),
                                    // whose wave mix is the 320-px strip's; with two strips per pair the chain wave is the pole and fb_fold_up decides.  An option of
                                    // its own, not a fourth bit of fb_fold_up: that option is a 3-bit mask with default 5 by its published contract (avd.h, ABI 3)
    int fb_mode = 1;                // 1 = fast level kernel (avd_fbfast.hip: literal vertical chain, direct horizontal window sums; flow within
                                    // 1e-5 px of the oracle, in practice identical), 0 = exact (avd_fbfused.hip / two-kernel path: bit-identical)
    int fb_rerun = 1;               // fast mode: pairs the level kernels flag as ill-posed are re-run by the exact kernels (launch_farneback_rerun); 0 = A/B, tests
    int fb_rerun_fused = 0xC;       // exact re-run of FEW pairs (<= kRerunTwoKernelMax): level mask of the fused kernel (bit 3 = 40 px must be set), the other levels run the two-kernel path
    int last_rerun = 0;             // pairs re-run by the last drained call
    // the last Farneback chunk of an asynchronous call, whose flags the host has not seen yet (impl_synchronize re-runs its flagged pairs, as `call` says)
    struct { int active = 0, p0 = 0, np = 0, fa = 0; const int* clipstart = nullptr; FlowCall call{}; } tail;
    // A thread that waits in avd_synchronize settles the tails of OTHER contexts whose fast pass has finished meanwhile (avd_capi.hip, tail_help_others):
    // one host thread driving several contexts (avd_hip.ClipsInFlight, bench.py) would otherwise start each clip's re-run only when it reaches that clip.
    std::recursive_mutex api_mu;    // held by every entry point that takes this context; helpers only try_lock it
    hipEvent_t tail_ev = nullptr;   // the call's records (with the flag words) have reached the pinned buffer
    int tail_registered = 0;        // in the process-wide list of contexts with an unsettled tail
    int tail_rc = 0;                // status of a settlement another thread did for this context (reported by its avd_synchronize)
    int tail_help = 1;              // option "tail_help": 0 = never settle other contexts' tails, wait with hipStreamSynchronize (A/B, tests)
};

// profiling only (avd_set_profiling): the region that starts here on the context's stream is kernel `id` (AVD_K_COUNT: nobody's -- the end of
// the call).  shared: an event that was recorded at this very place (a stage event of avd_stage_ms); the region is bounded by it instead of by
// an event of its own, so that the stage and the region begin at ONE timestamp and neither decomposition of the call contains a gap between
// two event packets that the other lacks.
inline void kmark(avd_ctx* ctx, int id, hipEvent_t shared = nullptr)
{
    // the last slot is kept for the closing mark (AVD_K_COUNT): a call with more regions than slots loses its LATER regions' split (they are
    // accounted to the region of mark 94), never the end of the timeline; kmark_overflow says so (avd_kernel_ms fails then)
    if (!ctx->profiling) return;
    if (ctx->kmark_used >= 96 || (ctx->kmark_used == 95 && id != AVD_K_COUNT)) { ctx->kmark_overflow = 1; return; }
    if (shared) { ctx->kmark_at[ctx->kmark_used] = shared; ctx->kmark_id[ctx->kmark_used++] = id; return; }
    hipEvent_t& e = ctx->kmark_ev[ctx->kmark_used];
    if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; return; }
    if (hipEventRecord(e, ctx->stream) == hipSuccess) { ctx->kmark_at[ctx->kmark_used] = e; ctx->kmark_id[ctx->kmark_used++] = id; }
}

// the marks of a call begin: whatever an earlier call left behind -- marks it never closed, an overflow nobody drained -- is not this call's
inline void kmark_reset(avd_ctx* ctx) { ctx->kmark_used = 0; ctx->kmark_overflow = 0; }

// profiling only: one of the twelve events around the 320-px level's blur launches (avd_stage_ms 4 and 5 are sums over alternate intervals,
// impl_synchronize); `on` = the caller's launch is one of those (level 0 of a chunk's first pass, never the exact re-run)
inline void level320_mark(avd_ctx* ctx, bool on) { if (on && ctx->profiling && ctx->kern_ev_used < 12) (void)hipEventRecord(ctx->kern_ev[ctx->kern_ev_used++], ctx->stream); }

template <typename T, bool kPinned>
int Buf<T, kPinned>::reserve(avd_ctx* ctx, size_t count)
{
    if (count <= cap) return 0;
    reset();
    const hipError_t e = kPinned ? hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) {
        ctx->err = std::string(kPinned ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e);
        p = nullptr;
        return AVD_ERR_NOMEM;
    }
    cap = count;
    return 0;
}

// ---- stage launchers (each enqueues on ctx->stream) --------------------------------
// the clip's frames, resident at d_in (BGR) or d_in / d_uv (NV12: Y rows at d_in + f*frame_stride + y*row_stride, chroma rows at
// d_uv + f*uv_frame_stride + (y/2)*uv_row_stride) or d_in / d_uv / d_v (I420: d_uv is the U plane, both chroma planes with the uv strides),
// or d_in alone (the packed RGB layouts, as BGR with 3 or 4 bytes per pixel) or d_in / d_uv / d_v (RGBP: R, G, B, all with the clip's row_stride / frame_stride),
// into the clip's slice of the per-frame buffers, with the clip's geometry (slot); which it is says clip.format
// list (null: strided): the frames come from a device table of plane pointers (avd_frame_list) -- d_in / d_uv / d_v are then the addresses of the
// table's per-plane arrays, n entries each, and the clip's frame strides are unused
// A grouped launch (option "ingest_group") is a listed launch over the n frames of several clips that share clip's key -- `clip` is the first of
// them -- with a device table out_frame[n]: frame g of the launch writes its 320-px image at frame out_frame[g] of ws.d_small (slot.f0 is unused),
// its row and Laplacian partials at g of the slot's run.
struct FrameTable { bool aligned; const int* out_frame = nullptr; int n = 0; };      // aligned: every frame of the list allows the 16-byte fills (list_vec_eligible); out_frame / n: a grouped launch
int launch_preprocess(avd_ctx* ctx, const ClipSlot& slot, const IngestClip& clip, const uint8_t* d_in, const uint8_t* d_uv, const uint8_t* d_v,
                      const FrameTable* list = nullptr);
// the clip's n frames; out_frame (device, may be null): a grouped launch's n frames, whose cells, bits and moments go to frame out_frame[g] of the buffers
int launch_hash(avd_ctx* ctx, const ClipSlot& slot, int n, const int* out_frame = nullptr);
int avd_calls_in_flight();      // avd_capi.hip: contexts of this process holding an enqueued, undrained avd_analyze_* call
// all pairs of n resident frames, into the Farneback scratch; *left (and ws.fb_holds) = what it holds then
int launch_farneback(avd_ctx* ctx, const FlowCall& call, const uint8_t* d_small, int n, FbChunk* left);
int launch_flow_stats(avd_ctx* ctx, const FlowCall& call, const FbChunk& chunk, int n);
// the 320-px flow of the chunk the scratch holds, where its last launch left it unwritten (FbChunk::flow0_late); nothing else to do otherwise
int launch_flow0_late(avd_ctx* ctx);
// avd_vit.hip (extension): patchify + bf16 MFMA GEMM; all pointers device
int launch_vit_patch_embed(avd_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, int64_t row_stride, int64_t frame_stride,
                           const uint16_t* d_wt, const float* d_bias, void* d_tokens, int tokens_bf16, uint16_t* d_patches);
void gemm_block_operand(const uint16_t* src_row_major, uint16_t* dst_blocked, int rows, int K);
constexpr int kGemmRowPad = 256;     // the GEMM's tile height: A is allocated in multiples of it
int launch_gemm_bf16_nt(avd_ctx* ctx, const uint16_t* d_a, const uint16_t* d_bt, const float* d_bias, void* d_c, int out_bf16,
                        int M, int N, int K);
// avd_cnn.hip (extension): ResNet-50-style forward as implicit GEMMs on the matrix cores
void cnn_param_counts(size_t* n_weights, size_t* n_biases);
int cnn_set_weights(avd_ctx* ctx, const uint16_t* weights, const float* biases);
int cnn_reserve(avd_ctx* ctx, int n);
int launch_cnn_forward(avd_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, int64_t row_stride, int64_t frame_stride);
int64_t cnn_tap_fetch(avd_ctx* ctx, void* out, size_t out_bytes);   // avd_debug_fetch "cnn_tap": activations de-blocked to NHWC
int cnn_conv_host(avd_ctx* ctx, const uint16_t* x, int n, int hin, int win, int cin, const uint16_t* w, const float* bias, int cout, int ksize,
                  int stride, int relu, const uint16_t* residual, uint16_t* y);
// avd_comm.cpp: RCCL all-gather of the per-frame records (dlopen, no link-time dependency)
int comm_unique_id(std::string& err, void* id128);
int comm_init(avd_ctx* ctx, int rank, int world, const void* id128);
void comm_destroy(avd_ctx* ctx);
int comm_allgather_records(avd_ctx* ctx, const avd_frame_record* local, int count, avd_frame_record* all);
int comm_allgather_last_records(avd_ctx* ctx, int count, avd_frame_record* all);
// avd_audio.hip: per-window features of the mono tracks of `plan` (device pointers; format: option "audio_format")
int launch_audio_features(avd_ctx* ctx, const void* d_wav, int format, const avd_audio::Plan& plan, avd_audio_window* d_out);
// A non-zero mix.id (option "audio_layout") makes the launchers below take the layout kernels: `channels` is then mix.channels, and d_in is
// addressed by the mix (planes mix.stride samples apart, or interleaved frames).
// avd_audio.hip: the frames at d_in (format: option "audio_format"; channels interleaved) to the 16 kHz mono int16 tracks of `plan` at d_pcm
// (device, plan.n_out + 8 entries, 16-byte aligned)
int launch_audio_resample(avd_ctx* ctx, const void* d_in, int format, int channels, const avd_resample::Plan& plan, int16_t* d_pcm, const AudioSource& src = AudioSource{},
                          const avd_resample::Mix& mix = avd_resample::Mix{});
// avd_audio.hip: the converter of a call of several tracks (option "audio_track_slot"): the tiles, tile tracks and source rows of `plan` (avd_audio_map.h)
int launch_audio_resample_map(avd_ctx* ctx, const void* d_in, int format, int channels, const avd_audio_map::Plan& plan, const avd_resample::Ratio& r, long long n_in,
                              int16_t* d_pcm, bool* launched, const avd_resample::Mix& mix = avd_resample::Mix{});
// avd_audio.hip: the gather and the save launch of a call of several tracks (option "audio_track_slot"); elem: bytes of an analysis sample
int launch_audio_gather(avd_ctx* ctx, const AudioGatherMove* moves, int count, int elem);
int launch_audio_slot_save_map(avd_ctx* ctx, int format, int channels, const AudioSaveRow* rows, int count, bool* enqueued,
                               const avd_resample::Mix& mix = avd_resample::Mix{});
// avd_audio.hip: what a call leaves in its audio slot -- the last hist_new_n frames of the track (from the call's n frames at d_in and the old
// history) as mono int16, and held_words 16-bit words of the analyzer's buffer.  *enqueued is set once the launch has been made (not by a refusal before it)
int launch_audio_slot_save(avd_ctx* ctx, const void* d_in, int format, long long n, int channels, const int16_t* hist_old, int hist_old_n, int16_t* hist_new,
                           int hist_new_n, const void* held_src, int16_t* held_dst, int held_words, bool* enqueued,
                           const avd_resample::Mix& mix = avd_resample::Mix{});
// avd_fbfused.hip: all blur iterations of one pyramid level (w = 40 / 80 / 160 / 320) in one launch, one workgroup per pair
// zero_first: the initial flow is zero whatever the buffer holds (the coarsest level: no clearing launch)
// plist (may be null): the launch works on pairs plist[0 .. np)
int launch_fb_level(avd_ctx* ctx, hipStream_t stream, int w, const float* R, float* flow, int np, int iterations, int zero_first, const int* plist = nullptr);
// the width of a pyramid level (320 / 160 / 80 / 40 px) as a compile-time constant: f(std::integral_constant<int, W>{}); false = no such level
template <int W = AVD_SMALL, typename F>
inline bool fb_dispatch_width(int w, F&& f)
{
    if (w == W) return f(std::integral_constant<int, W>{}), true;
    if constexpr (W > (AVD_SMALL >> (AVD_FB_LEVELS - 1))) return fb_dispatch_width<W / 2>(w, f);
    return false;
}
// avd_fbtwo.hip: ONE blur iteration of one pyramid level as two kernels that exchange the double intermediate through `s`; which shape runs
// (k_uvp<W, 12> + k_hscan_lat, k_uvp<W, 4>, k_uv) follows w, np and plist.  plist (may be null): the launch works on pairs plist[0 .. np), the
// intermediate is indexed by position in the list.  marks: a 320-px iteration records four level320_mark events (on ctx->stream, which `stream` is)
struct FbTwoScratch { double *vs, *vs0; };            // exact mode: {ws.d_vs, ws.d_vs0}; the re-run: {ws.d_vs_rerun, ws.d_vs0_rerun}
struct FbTwoScratchSize { size_t vs, vs0; };          // doubles
FbTwoScratchSize fb_two_scratch_size(size_t np);      // what np pairs need at any level
int launch_fb_two(avd_ctx* ctx, hipStream_t stream, int w, const float* R, float* flow, FbTwoScratch s, int np, const int* plist, bool marks);
// avd_fbfast.hip: blur iterations of one pyramid level, a pair spread over several workgroups (column strips), the horizontal window sums
// formed directly in double (the vertical chain stays literal).  One launch runs `iterations` (1, or all 3 where a pair is one workgroup:
// 80 / 40 px) from an initial flow that comes `from`:
//   level     flow_in, a buffer of this level (every width)
//   zero      like level, but at 40 px (the coarsest level) the flow is taken as zero whatever flow_in holds: no clearing launch
//   chain     flow_in = the COARSER level's final flow [pair][2][w/2][w/2], resized by the chain wave on the fly (320 px, and 160 px in the one-strip
//             shape: wide160; 1 iteration); in the 320-px level's five-block shape (wide320) by the normal-equation waves, in registers
//   prologue  the same, resized by the whole workgroup into flow_tmp first (160 / 80 px with 1 iteration, 80 px with 3)
enum class FbFlowFrom { level, zero, chain, prologue };   // the result is in flow_out (3 iterations: flow_tmp is the second buffer); nothing is updated in place
struct FbFastLaunch {
    bool wide160;                                // the 160-px shape of the call (FlowCall::wide160); no other level reads it
    bool wide320;                                // 320 px: this launch runs a pair as one five-block workgroup (from = level or chain, 1 iteration only); no other level reads it
    int iterations; FbFlowFrom from; const float* flow_in; float *flow_out, *flow_tmp;
    float* mag_out;                              // 320-px level, last iteration (else null): float[pair][320][320] receives |flow|
    int* flags; const int* pairdiff;             // may be null, see avd_fbfast.hip
    bool store_flow = true;                      // false (with mag_out only): flow_out is not written, |flow| alone is kept
};
int launch_fb_fast(avd_ctx* ctx, hipStream_t stream, int w, const float* R, const FbFastLaunch& L, int np);
// avd_farneback.hip: exact re-run of the m flagged pairs h_list[0 .. m) (pair indices inside the chunk the workspace holds; h_list pinned); np_chunk = its pairs
constexpr int kRerunTwoKernelMax = 32;
int launch_farneback_rerun(avd_ctx* ctx, const FlowCall& call, const int* h_list, int m, int np_chunk);
// avd_norm.hip (extensions): LayerNorm over rows of 256..2048 values, softmax over rows of logits; device pointers
int launch_layernorm(avd_ctx* ctx, const void* d_x, void* d_y, int bf16, long long rows, int cols, const float* d_gamma, const float* d_beta, float eps);
int launch_softmax(avd_ctx* ctx, const float* d_x, float* d_y, long long rows, int cols);
