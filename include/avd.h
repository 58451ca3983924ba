/*
 * avd.h -- C-ABI of libavd_hip.so, the MI355X (gfx950) implementation of the
 * per-frame video-analysis hot path of backtato/ai-video-detector.
 *
 * The reference has no native boundary: its hot path is 82 lines of Python
 * (reference app/analyzers/video.py:10-83) that call OpenCV per sampled frame.
 * Each entry point below replaces the OpenCV/numpy calls named beside it; the
 * Python shim that binds them (ctypes) is ai-video-detector_amd/avd_hip/_lib.py
 * and the drop-in module is ai-video-detector_amd/app/analyzers/video.py
 * (same module path / signature as the reference).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / HIP types in signatures.
 *   - every function returns 0 on success, a negative avd_status otherwise and
 *     never throws; avd_last_error(ctx) gives a message owned by ctx.
 *   - the caller owns every buffer; the library never frees or retains them.
 *   - `mem` says where an INPUT buffer lives: AVD_MEM_HOST (staged over PCIe) or
 *     AVD_MEM_DEVICE (already resident in HBM of ctx's device, e.g. a
 *     torch-ROCm tensor's data_ptr or a hardware decoder surface).
 *     OUTPUT buffers are always host memory (they are tiny).
 *   - one avd_ctx = one device, one HIP stream, one workspace.  A ctx is not
 *     re-entrant: use one ctx per thread (calls on different ctxs run concurrently;
 *     two calls on the SAME ctx are serialised by a lock, they do not overlap).
 *     A thread that waits in avd_synchronize may enqueue the exact re-run of another
 *     ctx's flagged pairs meanwhile (option "tail_help"); that ctx's results and
 *     errors still come out of its own avd_synchronize.
 *   - every ingest entry point (avd_preprocess_*, avd_analyze_*) checks its clips the same way, before anything is
 *     launched.  A clip with several faults is refused for the FIRST of, in this order: mem that is neither
 *     AVD_MEM_HOST nor AVD_MEM_DEVICE (AVD_ERR_ARG); a size out of range -- n < 0, h or w outside 1 .. 16384
 *     (AVD_ERR_ARG); an odd width or height of 4:2:0 input (AVD_ERR_UNSUPPORTED); a picture below 32 x 32
 *     (AVD_ERR_UNSUPPORTED); a null plane of a clip with n > 0 (AVD_ERR_ARG); strides smaller than the planes
 *     (AVD_ERR_ARG); of a picture in 16-bit words (AVD_FMT_P010 / _I010), a plane base, row stride or frame stride that is odd (AVD_ERR_ARG).
 *     What an avd_picture alone can get wrong is refused before any of these, in this order:
 *     struct_size; format (an unknown layout in the low byte, or a bit above it other than AVD_FMT_FULL_RANGE);
 *     AVD_FMT_FULL_RANGE on a BGR or RGB picture; rotate; reserved; BGR or RGB with a rotation; U and V (RGBP: R, G and B)
 *     strides that differ.
 *     An avd_frame_list is refused for the same things in the same order (it has no frame strides; a null array of plane pointers, then a
 *     null entry of one, stand where the null plane stands).  A records pointer that is null while
 *     there are frames to write, after all of them.  The clips of a batch are checked in order.
 *   - if no HIP device is usable avd_create fails (AVD_ERR_DEVICE): there is no
 *     CPU fallback in this library.
 */
#ifndef AVD_H
#define AVD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avd_ctx avd_ctx;

enum avd_status {
    AVD_OK = 0,
    AVD_ERR_ARG = -1,       /* bad argument (null pointer, size out of range) */
    AVD_ERR_DEVICE = -2,    /* no usable HIP device / HIP runtime error */
    AVD_ERR_NOMEM = -3,     /* workspace allocation failed */
    AVD_ERR_UNSUPPORTED = -4 /* frame smaller than 32x32 (INTER_AREA upscaling) etc. */
};

enum avd_mem { AVD_MEM_HOST = 0, AVD_MEM_DEVICE = 1 };

#define AVD_SMALL 320          /* video.py:43 resize target */
#define AVD_HASH 32            /* video.py:36 aHash size */
#define AVD_ABI_VERSION 3      /* 3 (round 5): avd_frame_record.reserved is a criterion / level mask, option "fb_rerun_fused", "fb_fold_up" is a 3-bit mask */

/* One record per sampled frame: everything video.py:36-57 derives from pixels.
 * The scalar tail (tex variance, ai_susp, summary, timeline; video.py:54-83) is
 * O(N) float64 host work done by the caller from these records. */
typedef struct avd_frame_record {
    int64_t lap_sum;     /* sum  of cv2.Laplacian(gray, CV_64F)        (video.py:52) */
    int64_t lap_sumsq;   /* sum of squares of the same (exact integers)            */
    float   flow_mean;   /* np.mean(|flow|) vs the previous sampled frame (video.py:47); 0 for frame 0 */
    float   flow_var;    /* np.var(|flow|)                                 (video.py:48); 0 for frame 0 */
    int32_t ham;         /* popcount(hash ^ prev_hash)     (video.py:38); -1 for frame 0 */
    int32_t reserved;    /* non-zero: the pair (previous frame, this frame) was flagged ill-posed by the fast Farneback kernels and re-run exactly.
                          * bit k (0 = 320 px .. 3 = 40 px): level k met the solver's criterion; bit 4 + k: the border-sign criterion.  Levels a pair
                          * skipped because it was flagged already leave no bit. */
} avd_frame_record;      /* 32 bytes */

int avd_abi_version(void);

/* Lifetime.  avd_create binds HIP device `device_id`, creates a stream.  */
int avd_create(int device_id, avd_ctx** out);
void avd_destroy(avd_ctx* ctx);
const char* avd_last_error(const avd_ctx* ctx);

/* Replaces, for n decoded BGR frames (uint8, interleaved, frame f row y at
 * bgr + f*frame_stride + y*row_stride):
 *   cv2.cvtColor(BGR2GRAY) x3, cv2.resize(32x32, INTER_AREA) + mean threshold,
 *   cv2.resize(320x320) INTER_LINEAR, cv2.Laplacian(CV_64F) moments
 *   (video.py:4-8, 36, 43, 51-52).
 * Outputs (host, any may be NULL): small320 uint8[n][320*320], hash1024 uint8[n][1024]
 * (0/1), lap_sum / lap_sumsq int64[n]. */
int avd_preprocess_bgr(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w,
                       int64_t row_stride, int64_t frame_stride,
                       uint8_t* small320, uint8_t* hash1024,
                       int64_t* lap_sum, int64_t* lap_sumsq);

/* Replaces cv2.calcOpticalFlowFarneback(prev, cur, None, 0.5, 3, 15, 3, 5, 1.2, 0)
 * + np.sqrt/np.mean/np.var (video.py:45-48) for the n-1 consecutive pairs of
 * n 320x320 uint8 images.  Outputs host float[n-1].  flow_out (host, may be
 * NULL) receives the dense flow float[n-1][320][320][2]. */
int avd_farneback_pairs(avd_ctx* ctx, const uint8_t* small320, int mem, int n,
                        float* flow_mean, float* flow_var, float* flow_out);

/* The whole per-frame pixel path in one call: preprocess + Hamming + Farneback
 * + flow statistics, everything resident in HBM in between (video.py:36-52).
 * records: host avd_frame_record[n]. */
int avd_analyze_frames(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w,
                       int64_t row_stride, int64_t frame_stride,
                       avd_frame_record* records);

/* Same, but only enqueues the work on ctx's stream and returns; records (any HOST
 * memory) are filled by avd_synchronize: the device-to-host copy lands in a pinned
 * buffer of the library, so the call never blocks on it and several contexts can
 * keep clips in flight on one GPU.  One call may be outstanding per context: any
 * other call on the context first completes it -- its records buffer is filled and
 * the re-run of its flagged pairs (fb_mode 1) is settled -- and returns its error
 * instead of running if it failed.  The same holds for avd_analyze_frames_nv12_async,
 * avd_analyze_frames_i420_async, avd_analyze_batch_async, avd_analyze_pictures_async and avd_analyze_frame_lists_async: whichever of them is
 * outstanding is drained by any other call, these included.  Exempt: avd_synchronize, avd_destroy,
 * avd_last_error, avd_get_option, avd_stage_ms, avd_kernel_ms, avd_timer_start /
 * avd_timer_stop and avd_wait_stream.  An option set while a call is pending applies
 * to the calls submitted after it; "rerun_pairs" reports the last call that ran the
 * Farneback stage.  With AVD_MEM_HOST input the frames are staged by
 * hipMemcpyAsync from the caller's buffer, which is only asynchronous if that buffer
 * is pinned. */
int avd_analyze_frames_async(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w,
                             int64_t row_stride, int64_t frame_stride,
                             avd_frame_record* records);
int avd_synchronize(avd_ctx* ctx);

/* A BATCH of clips in one call (BASELINE.json configs[2] / configs[4]: many concurrent clips, mixed resolutions).  The
 * reference analyses one file per request in a sequential loop (app/analyzers/video.py:27-58); a service that has several
 * short clips waiting hands them over together: preprocess / hash / Hamming run per clip with that clip's geometry (the
 * tables of the last few geometries are cached per context: no allocation in steady state), then ONE Farneback launch
 * sequence covers the pairs of all clips (that stage is 320 x 320 whatever the source resolution), so thirteen 20-frame
 * clips fill the chip like one long clip instead of running thirteen sequences of 19 pairs each.
 * A clip is BGR (uv == NULL: data = frames, row_stride / frame_stride in bytes) or NV12 (data = Y plane, uv = interleaved
 * chroma plane, the four strides as for avd_analyze_frames_nv12).  records: host, sum of clips[i].n entries, clip after
 * clip; the first record of every clip has ham = -1 and flow 0 (video.py:37-41, 55).  Results are identical to calling
 * avd_analyze_frames per clip.  avd_clip is frozen at ABI 3 and has no room for a third plane: a batch holds BGR and NV12
 * clips only; planar I420 clips (avd_analyze_frames_i420) wait for the next ABI revision.  They do not have to wait for a batch, though: the
 * descriptor family below (avd_picture, avd_analyze_pictures) is additive at ABI 3, carries three planes and a display rotation, and batches
 * any mix of formats. */
typedef struct avd_clip {
    const uint8_t* data;
    const uint8_t* uv;
    int mem, n, h, w;
    int64_t row_stride, frame_stride, uv_row_stride, uv_frame_stride;
} avd_clip;
int avd_analyze_batch(avd_ctx* ctx, const avd_clip* clips, int nclips, avd_frame_record* records);
int avd_analyze_batch_async(avd_ctx* ctx, const avd_clip* clips, int nclips, avd_frame_record* records);

/* NV12 input (decode -> ingest).  Hardware decoders (VCN / rocDecode) and most software decoders
 * produce YUV 4:2:0, not BGR; the reference gets BGR because cv2.VideoCapture.retrieve() runs libswscale on the
 * decoded picture (reference app/analyzers/video.py:28-32).  These entry points take the decoder's surface
 * directly -- a Y plane uint8[h][w] and an interleaved U,V plane uint8[h/2][w], per frame at
 * y + f*y_frame_stride + row*y_row_stride and uv + f*uv_frame_stride + (row/2)*uv_row_stride -- and form, per pixel
 * and in registers, the BGR triple libswscale's C converter would have written (yuv2rgb.c tables: BT.601 limited
 * range, nearest chroma) before cv2's BGR2GRAY: 1.5 bytes per pixel cross PCIe / HBM instead of 3, and no BGR frame
 * exists anywhere.  Results equal avd_analyze_frames on the BGR frames of oracle/avd_oracle.c's avdo_nv12_to_bgr24
 * bit for bit; parity with a real libswscale is UNPINNED (restated from memory, x86 builds also dispatch to SIMD
 * code that differs by +-1).  Width and height must be even.  Outputs as for the BGR entry points.
 * These entry points, the I420 ones below and the NV12 clips of avd_clip are LIMITED range (Y 16 .. 235, chroma 16 .. 240); full-range
 * pictures (ffmpeg's yuvj420p) go through avd_picture with AVD_FMT_FULL_RANGE. */
int avd_preprocess_nv12(avd_ctx* ctx, const uint8_t* y, const uint8_t* uv, int mem, int n, int h, int w,
                        int64_t y_row_stride, int64_t uv_row_stride, int64_t y_frame_stride, int64_t uv_frame_stride,
                        uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq);
int avd_analyze_frames_nv12(avd_ctx* ctx, const uint8_t* y, const uint8_t* uv, int mem, int n, int h, int w,
                            int64_t y_row_stride, int64_t uv_row_stride, int64_t y_frame_stride, int64_t uv_frame_stride,
                            avd_frame_record* records);
int avd_analyze_frames_nv12_async(avd_ctx* ctx, const uint8_t* y, const uint8_t* uv, int mem, int n, int h, int w,
                                  int64_t y_row_stride, int64_t uv_row_stride, int64_t y_frame_stride,
                                  int64_t uv_frame_stride, avd_frame_record* records);

/* Planar 4:2:0 input (I420, ffmpeg's yuv420p): what SOFTWARE decoders hand over -- libavcodec behind cv2.VideoCapture (the reference's
 * own source), a .y4m file, an `ffmpeg -f rawvideo -pix_fmt yuv420p` pipe, PyAV frames.  A Y plane uint8[h][w] and separate U and V planes
 * uint8[h/2][w/2], per frame at y + f*y_frame_stride + row*y_row_stride, u + f*c_frame_stride + (row/2)*c_row_stride and v likewise (the
 * two chroma planes share their strides).  YV12 (V stored before U) is the same call with the u and v pointers exchanged.  The arithmetic
 * is the NV12 entry points': results equal avd_*_nv12 on the interleaved form of the same planes bit for bit, hence avd_analyze_frames on
 * avdo_nv12_to_bgr24's BGR frames.  Width and height must be even (AVD_ERR_UNSUPPORTED otherwise, as for frames below 32 x 32); null
 * planes, strides smaller than the planes and sizes above 16384 are AVD_ERR_ARG.  With AVD_MEM_HOST input the three per-plane spans are
 * merged where they overlap or touch before they are staged: planes that come out of one buffer per clip (Y, U, V of a frame adjacent)
 * cross the link once, as ONE copy; separately allocated planes are three copies (avd_debug_fetch "stage_bytes").
 * avd_analyze_frames_i420_async follows avd_analyze_frames_async: one call outstanding per context, drained by any other call. */
int avd_preprocess_i420(avd_ctx* ctx, const uint8_t* y, const uint8_t* u, const uint8_t* v, int mem, int n, int h, int w,
                        int64_t y_row_stride, int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride,
                        uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq);
int avd_analyze_frames_i420(avd_ctx* ctx, const uint8_t* y, const uint8_t* u, const uint8_t* v, int mem, int n, int h, int w,
                            int64_t y_row_stride, int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride,
                            avd_frame_record* records);
int avd_analyze_frames_i420_async(avd_ctx* ctx, const uint8_t* y, const uint8_t* u, const uint8_t* v, int mem, int n, int h, int w,
                                  int64_t y_row_stride, int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride,
                                  avd_frame_record* records);

/* Pictures by descriptor, with a display rotation (additive at ABI 3; avd_clip and every entry point above are unchanged).  A decoder hands over
 * the STORED picture; a container may carry a display rotation (every portrait clip a phone records is stored 1920 x 1080 with a 90 degree
 * display matrix), and cv2.VideoCapture applies it before the reference sees a frame (orientation-auto), so the reference's records are those of
 * the DISPLAYED picture.  avd_picture describes the stored planes and says how they turn:
 *   D = np.rot90(S, -rotate) over the picture axes of every plane (chroma planes turn as (h/2, w/2) images of U,V samples)
 * and every output of a call with rotate = k equals, bit for bit, the output of the format's own entry point above on D's planes, in both
 * fb_modes.  (libswscale's nearest-chroma conversion commutes with quarter turns of even-sized pictures, so this is also the rotated BGR frame's
 * result.)  For odd `rotate` the displayed size is w x h; the 32 x 32 minimum, the resampling tables and avd_debug_fetch "ingest_plan" follow the
 * displayed size, the host staging ("stage_bytes") the stored planes.  The turn happens inside the fused pass, where the gray tile is filled: a
 * half turn reads the mirrored rows and chunks of the same kernels, a quarter turn reads of every stored row the 16-byte span a band needs (the
 * strip fill); no turned picture exists in memory.
 *   struct_size  sizeof(avd_picture) of the caller's header; anything else is AVD_ERR_ARG
 *   plane        BGR: [0]; NV12: Y, interleaved UV; I420: Y, U, V (YV12: exchange [1] and [2]); the RGB, 4:2:2 and 10-bit layouts: below the struct's format enum
 *   row_stride, frame_stride   bytes, per plane; I420, I422 and I010: [1] == [2] (AVD_ERR_ARG otherwise); RGBP: [0] == [1] == [2]
 *   h, w         the stored picture;  rotate  quarter turns clockwise from the stored to the displayed picture, 0 .. 3;  reserved  0
 *   format       the layout (AVD_FMT_BGR24 / _NV12 / _I420 / _RGB24 / _BGRA32 / _RGBA32 / _RGBP / _YUYV422 / _UYVY422 / _I422 / _NV16 / _P010 / _I010), for the 4:2:0 and 4:2:2
 *                layouts optionally OR-ed with AVD_FMT_FULL_RANGE
 * Refused without a launch: rotate outside 0 .. 3, a non-zero reserved, a bad format or struct_size (AVD_ERR_ARG); what the format's own entry
 * point refuses, with its status; AVD_FMT_BGR24 with rotate != 0 (AVD_ERR_UNSUPPORTED: cv2 hands BGR over already rotated, stored-orientation
 * BGR does not arise).  Mirrored display matrices are not covered.
 * AVD_FMT_FULL_RANGE: the samples use 0 .. 255 -- ffmpeg's yuvj420p (AVD_FMT_I420 | AVD_FMT_FULL_RANGE) and its semi-planar form
 * (AVD_FMT_NV12 | AVD_FMT_FULL_RANGE): every MJPEG clip, the H.264 of many phones and screen recorders.  cv2.VideoCapture.retrieve() converts
 * those with the same table-driven yuv2rgb.c, its tables built for fullRange = 1 (luma gain 1, chroma coefficients times 224/255), and so does
 * the fused pass: results equal the BGR entry points on that conversion's frames bit for bit (tests/yuv_tables_reference.py restates it; parity
 * with a real libswscale is UNPINNED exactly as in the limited case).  Without the flag a 4:2:0 picture is limited range, as everywhere above.
 * The flag is per clip: a batch may mix ranges.  AVD_FMT_BGR24 | AVD_FMT_FULL_RANGE (BGR has no range), any other bit above the low byte and an
 * unknown layout in the low byte are AVD_ERR_ARG.
 * avd_preprocess_picture: outputs as avd_preprocess_bgr.  avd_analyze_pictures: the batch of avd_analyze_batch with descriptors -- any mix of
 * formats, geometries and rotations, I420 included; records clip after clip, identical to one call per clip; ONE Farneback launch sequence over
 * all clips; nclips = 1 is the single-clip call.  avd_analyze_pictures_async follows avd_analyze_batch_async exactly: one call outstanding per
 * context, drained by any other call, with the same exemptions. */
enum avd_format { AVD_FMT_BGR24 = 0, AVD_FMT_NV12 = 1, AVD_FMT_I420 = 2 };
#define AVD_FMT_FULL_RANGE 0x100      /* a flag OR-ed into the layout in avd_picture.format; the layout is the low byte */
/* RGB producers (additive at ABI 3; avd_picture / avd_frame_list only -- avd_clip and the entry points that name their format are unchanged).
 * Everything that hands over RGB rather than BGR: torchcodec / torchvision.io (uint8[N,3,H,W], channels first), decord, PyAV rgb24, imageio,
 * PIL (uint8[H,W,3]), screen capture, compositors and rocDecode's colour-conversion helpers (BGRA / RGBA), ffmpeg's gbrp.  The gray conversion
 * is the first thing the fused pass does, so the channel order is a constant of the fill: no rearranged copy exists anywhere.
 *   AVD_FMT_RGB24   1 plane   R,G,B interleaved, 3 bytes per pixel
 *   AVD_FMT_BGRA32  1 plane   B,G,R,x, 4 bytes per pixel; the fourth byte is ignored
 *   AVD_FMT_RGBA32  1 plane   R,G,B,x, 4 bytes per pixel; the fourth byte is ignored
 *   AVD_FMT_RGBP    3 planes  plane[0] = R, [1] = G, [2] = B, each uint8[h][w]; the three planes share their row and frame strides
 * A torch uint8[N,3,H,W] tensor is AVD_FMT_RGBP with plane[c] = base + c*H*W and frame stride 3*H*W.  ffmpeg's gbrp (planes stored G, B, R) is
 * the same layout with its three plane pointers handed over in R, G, B order: plane[0] = data[2], plane[1] = data[0], plane[2] = data[1].
 * ARGB and ABGR (alpha first) are not covered, nor 16-bit or float RGB, nor GRAY8.
 * Results: if B is the BGR24 arrangement of the same pixels (alpha dropped), every output equals the BGR entry point's on B bit for bit -- cv2's
 * own RGB2GRAY / BGRA2GRAY use the same three coefficients in other positions.
 * Refused in avd_picture's / avd_frame_list's order, where the BGR and I420 equivalents stand: AVD_FMT_FULL_RANGE on any of the four
 * (AVD_ERR_ARG: RGB has no range); rotate != 0 (AVD_ERR_UNSUPPORTED: producers of RGB hand it over already turned); AVD_FMT_RGBP planes whose
 * row or frame strides differ (AVD_ERR_ARG).  No evenness rule applies; the 32 x 32 minimum, the 16384 limits, null planes and short strides
 * are checked as for every clip, with rows of 3w, 4w and w bytes.  Layouts 3 .. 0x0F, 0x14 .. 0x1F, 0x24 .. 0x2F and 0x32 .. 0xFF stay AVD_ERR_ARG (0x20 .. 0x23: the 4:2:2 layouts below; 0x30, 0x31: the 10-bit layouts below them).
 * AVD_MEM_HOST: the three planes of AVD_FMT_RGBP are staged as the planes of I420 are -- spans merged where they overlap or touch, so a dense
 * [N,3,H,W] stack crosses the link as ONE copy and separately allocated planes as three; the packed layouts are one span.
 * The 16-byte fills need w % 16 == 0 and every plane base, row stride and frame stride 16-byte aligned (a list: every frame); anything else
 * runs the scalar fill with identical results. */
#define AVD_FMT_RGB24  0x10
#define AVD_FMT_BGRA32 0x11
#define AVD_FMT_RGBA32 0x12
#define AVD_FMT_RGBP   0x13
/* 4:2:2 pictures -- chroma subsampled horizontally only (additive at ABI 3; avd_picture / avd_frame_list only -- avd_clip and the entry points that
 * name their format are unchanged).  MJPEG from cameras, webcams and capture boxes (ffmpeg's yuvj422p: AVD_FMT_I422 | AVD_FMT_FULL_RANGE), raw
 * webcam and capture-card frames and V4L2 / DeckLink / AVFoundation pipes (yuyv422, uyvy422), hardware JPEG and capture paths (NV16), a .y4m file
 * with C422.
 *   value  name               planes                                                                row bytes
 *   0x20   AVD_FMT_YUYV422    1: Y0 U Y1 V, a pixel pair per 4 bytes                                 2w
 *   0x21   AVD_FMT_UYVY422    1: U Y0 V Y1                                                           2w
 *   0x22   AVD_FMT_I422       3: Y [h][w], U and V [h][w/2] (YV16: exchange [1] and [2])             w, w/2, w/2
 *   0x23   AVD_FMT_NV16       2: Y [h][w], interleaved U,V [h][w]                                    w, w
 * The conversion: pixel (y, x) has luma Y[y][x] and the chroma sample U[y][x >> 1], V[y][x >> 1] of its OWN row, and its BGR triple is the one
 * libswscale's table converter (yuv2rgb.c) gives -- B = T[Y + ob(U)], G = T[Y + og(U, V)], R = T[Y + or(V)] with the very tables and constants
 * of the 4:2:0 path, limited range by default and full range with AVD_FMT_FULL_RANGE (allowed on all four, per clip of a batch).  Every output
 * of a call equals, bit for bit and in both fb_modes, the BGR entry point's on those BGR frames.  Two equivalent statements: an NV12 picture of
 * height 2h whose luma rows 2y and 2y + 1 are both Y[y] and whose chroma row y is this picture's chroma row y converts (avdo_nv12_to_bgr24,
 * tests/yuv_tables_reference.py) to this picture's BGR frame in its even rows; and a 4:2:2 picture of even height whose chroma rows 2k and
 * 2k + 1 are equal gives exactly the I420 / NV12 result on chroma rows k (tests/yuv422_reference.py restates the definition).
 * Parity with a real libswscale is UNPINNED, and nothing here can check it.  For the packed layouts and NV16 libswscale takes its general path
 * at equal size; as far as it can be restated that path has one-tap filters and (x + 64) >> 7 of a value shifted left by 7, then the same
 * tables: the definition above with every chroma row used.  For planar yuv422p / yuvj422p FFmpeg up to 7.0 takes the unscaled special
 * converter, which doubles the chroma stride and therefore uses only the EVEN chroma rows; later versions use every row.  Both are available:
 * every row is AVD_FMT_I422; even rows only is the AVD_FMT_I420 call on the same planes with the chroma row stride doubled (and an even h).
 * Which FFmpeg the reference's OpenCV wheel bundles could not be determined.
 * Refused in avd_picture's / avd_frame_list's order, where the RGB and I420 equivalents stand: rotate != 0 (AVD_ERR_UNSUPPORTED: the conversion
 * does not commute with quarter turns when only one axis is subsampled, and a turned 4:2:2 fill is not built); AVD_FMT_I422 chroma planes whose
 * row or frame strides differ (AVD_ERR_ARG); an odd width (AVD_ERR_UNSUPPORTED).  The height may be ODD: nothing is subsampled vertically.
 * The 32 x 32 minimum, the 16384 limits, null planes and short strides are checked as for every clip, with the row bytes above.  Layouts
 * 0x14 .. 0x1F, 0x24 .. 0x2F and 0x32 .. 0xFF stay AVD_ERR_ARG.
 * AVD_MEM_HOST: the packed layouts are one span of 2w-byte rows; the three planes of I422 are staged as I420's (merged where they overlap or
 * touch: a .y4m map is ONE copy, separately allocated planes three); NV16 as NV12, two spans.
 * The table fills need w % 16 == 0 and every plane base, row stride and frame stride 16-byte aligned (8 for the chroma planes of I422; a list:
 * every frame); anything else runs the scalar fill with identical results.
 * Not covered: turned 4:2:2 pictures; 4:4:4 and 10-bit 4:2:2 surfaces (libswscale's filtered general path, which is not restatable here; 10-bit
 * 4:2:0 is settled by definition, below); NV21, GRAY8
 * and mirrored display matrices.  avd_clip is unchanged. */
#define AVD_FMT_YUYV422 0x20
#define AVD_FMT_UYVY422 0x21
#define AVD_FMT_I422    0x22
#define AVD_FMT_NV16    0x23
/* 10-bit 4:2:0 pictures in 16-bit words (additive at ABI 3; avd_picture / avd_frame_list only -- avd_clip and the entry points that name their
 * format are unchanged).  HEVC Main10 as phones record it (libavcodec's yuv420p10le: AVD_FMT_I010), the same streams and 10-bit AV1 / VP9 from
 * VCN / rocDecode (P010 surfaces: AVD_FMT_P010).  The plane pointers stay const uint8_t* and every stride stays in BYTES; the words are
 * little-endian.
 *   value  name            planes                                                                                          row bytes
 *   0x30   AVD_FMT_P010    2: Y [h][w], interleaved U,V [h/2][w]; the 10 bits in the HIGH bits of each word (p010le; a       2w, 2w
 *                          P016 surface reads the same way)
 *   0x31   AVD_FMT_I010    3: Y [h][w], U and V [h/2][w/2]; the 10 bits in the LOW bits (yuv420p10le); U and V share their    2w, w, w
 *                          strides; exchange [1] and [2] for V-first
 * The definition, total over all 65536 words so that no input is undefined: a P010 word s becomes s8 = min(255, (s + 128) >> 8), formed without
 * 16-bit overflow -- with the low six bits zero that is min(255, (v10 + 2) >> 2), and non-zero low bits never change it --, an I010 word s
 * becomes s8 = min(255, (s + 2) >> 2).  The 8-bit NV12 / I420 picture of those samples, pushed through the format's own 8-bit path, gives every
 * output of the call: bit for bit, in both fb_modes, for rotate 0 .. 3, limited range by default and full range with AVD_FMT_FULL_RANGE (allowed,
 * per clip of a batch).  tests/yuv10_reference.py restates it.  No narrowed picture exists in memory: the samples are narrowed in registers
 * where the fused pass loads them, and everything behind the load is NV12's / I420's at the same displayed geometry.
 * Where the rounding comes from (restated from memory; parity with a real libswscale is UNPINNED, and nothing here can check it):
 * cv2.VideoCapture.retrieve() has libswscale convert the 10-bit picture to bgr24; its hScale16To15 takes a 10-bit sample v to v << 5 and the
 * one-tap vertical output takes that to (v * 32 + 64) >> 7 = (v + 2) >> 2 before the yuv2rgb tables.  Two known deviations: super-white samples
 * (v10 >= 1022) are clipped to 255 BEFORE the table, where libswscale would index the table at 256; and the vertical chroma interpolation of
 * libswscale's general path is not restated -- the NV12 deviation (nearest chroma), unchanged.
 * Refused in avd_picture's / avd_frame_list's order, where the NV12 / I420 equivalents stand: AVD_FMT_I010 chroma planes whose row or frame
 * strides differ (AVD_ERR_ARG); an odd width or height (AVD_ERR_UNSUPPORTED); the 32 x 32 minimum, the 16384 limits, null planes and short
 * strides as for every clip, with the row bytes above; and LAST a plane base (of a list: any entry), a row stride or a frame stride that is odd
 * (AVD_ERR_ARG: 16-bit samples need 2-byte aligned planes and strides).  Layouts 0x24 .. 0x2F and 0x32 .. 0xFF stay AVD_ERR_ARG.
 * AVD_MEM_HOST: P010 is staged as NV12, two spans; I010 as I420 -- spans merged where they overlap or touch, so a dense yuv420p10le frame stack
 * is ONE copy and separately allocated planes three.
 * The table fills need w % 16 == 0 and every plane base, row stride and frame stride 16-byte aligned, the chroma planes of I010 included (a
 * contiguous I010 frame has its V plane at 5wh/2 bytes, a multiple of 16; a list: every frame); anything else runs the scalar fill with
 * identical results.  A quarter turn runs the strip fill whatever the alignment.
 * Not covered: 10-bit 4:2:2 and 4:4:4, 12-bit and big-endian layouts. */
#define AVD_FMT_P010    0x30
#define AVD_FMT_I010    0x31
typedef struct avd_picture {
    uint32_t struct_size;
    int32_t  format;
    const uint8_t* plane[3];
    int64_t  row_stride[3], frame_stride[3];
    int32_t  mem, n, h, w;
    int32_t  rotate;
    int32_t  reserved;
} avd_picture;
int avd_preprocess_picture(avd_ctx* ctx, const avd_picture* picture, uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq);
int avd_analyze_pictures(avd_ctx* ctx, const avd_picture* clips, int nclips, avd_frame_record* records);
int avd_analyze_pictures_async(avd_ctx* ctx, const avd_picture* clips, int nclips, avd_frame_record* records);

/* Clips as LISTS of separately allocated frames -- avd_frame_list, avd_preprocess_frame_list, avd_analyze_frame_lists(_async): additive at
 * ABI 3 like avd_picture.  The family is declared in a header of its own, which this one includes: nothing else is needed to use it. */
#include "avd_frame_list.h"

/* ViT-B/16 patch embedding on the matrix cores -- a BUILD-DEFINED EXTENSION.  The reference
 * contains no learned model (its per-frame "model" is the closed form of app/analyzers/video.py:54-56); BASELINE.json's
 * north_star / configs[3] ask for this stage, so it exists, with caller-supplied weights, and is never part of
 * ai_score / timeline.  avd_vit_set_weights: weight_bf16 = bf16 bits [768 out][768 in], in = c*256 + py*16 + px (the
 * layout of a [768][3][16][16] conv weight, channels RGB), bias float[768] or NULL; both host pointers, copied.
 * avd_vit_patch_embed: each BGR frame is resized to 224x224 (bilinear), normalised ((x/255 - mean)/std, ImageNet
 * constants), cut into 196 patches of 16x16x3, rounded to bf16 and multiplied with the weights (f32 accumulation):
 * tokens [n][196][768], float (tokens_bf16 = 0) or bf16 bit patterns (tokens_bf16 = 1, round to nearest even), host or
 * device (tokens_mem).  If timing_reps > 0 and gemm_ms != NULL the GEMM kernel alone is launched timing_reps more times
 * between two HIP events and its mean duration is returned (bench hook). */
int avd_vit_set_weights(avd_ctx* ctx, const uint16_t* weight_bf16, const float* bias);
int avd_vit_patch_embed(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride,
                        int64_t frame_stride, void* tokens, int tokens_mem, int tokens_bf16, int timing_reps, float* gemm_ms);

/* CNN extension (build-defined: the reference has no learned model; BASELINE.json's north_star
 * names a "CNN (ResNet-50-style) forward" on the matrix cores).  Never part of ai_score / timeline.  Topology: 7x7/2
 * stem of 64 channels + ReLU, 3x3/2 max pool, bottleneck stages [3, 4, 6, 3] of widths 64/128/256/512 (x4 out, the stride
 * on the 3x3 convolution, projection shortcut in the first block of a stage), global average pool, linear 2048 -> 1000;
 * batch norm folded into weights + bias; bf16 weights and activations, f32 accumulation.
 * avd_cnn_param_counts: elements of the flat parameter arrays.  avd_cnn_set_weights (host pointers, copied): weights =
 * bf16 bits, convolutions in forward order (stem; per block conv1 1x1, conv2 3x3, conv3 1x1, then the projection shortcut
 * where there is one), each [cout][kh][kw][cin], then the linear layer [1000][2048]; biases f32 in the same order.
 * avd_cnn_forward: each BGR frame is resized to 224x224 and normalised as in avd_vit_patch_embed; logits: host float
 * [n][1000]; any n (more than 128 frames are processed in passes of 128).  If timing_reps > 0 and forward_ms != NULL the whole forward pass (input conversion to logits, 57 launches)
 * is run timing_reps more times between two HIP events and its mean duration is returned (bench hook).
 * avd_cnn_conv: ONE convolution layer on host tensors (test entry): x NHWC bf16 [n][hin][win][cin], w [cout][k][k][cin],
 * bias f32[cout], optional residual NHWC [n][hout][wout][cout] added before the optional ReLU, y NHWC bf16; pad = k / 2;
 * cin % 32 == 0, cout % 64 == 0, ksize 1 or 3, stride 1 or 2. */
int avd_cnn_param_counts(size_t* n_weights, size_t* n_biases);
int avd_cnn_set_weights(avd_ctx* ctx, const uint16_t* weights_bf16, size_t n_weights, const float* biases, size_t n_biases);
int avd_cnn_forward(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride, int64_t frame_stride,
                    float* logits, int timing_reps, float* forward_ms);
int avd_cnn_conv(avd_ctx* ctx, const uint16_t* x, int n, int hin, int win, int cin, const uint16_t* w, const float* bias,
                 int cout, int ksize, int stride, int relu, const uint16_t* residual, uint16_t* y);

/* LayerNorm and softmax -- the remaining elements of north_star's "conv / GEMM / LayerNorm / softmax stack"; BUILD-DEFINED
 * EXTENSIONS like the two above (the reference has no learned model), never part of ai_score.  One wave per row, the row
 * held in registers, wave-level shuffle reductions, one pass over HBM.
 * avd_layernorm: y = (x - mean) / sqrt(var + eps) * gamma + beta over the last dimension (biased variance, float32
 * statistics: torch.nn.functional.layer_norm); x / y [rows][cols] float32 (bf16 = 0) or bf16 bit patterns (bf16 = 1), both
 * host or both device (mem); any cols >= 1 -- 256, 512, 768, 1024 and 2048 (768 = the ViT-B/16 token width) run the
 * register-resident kernel, every other width a general one; gamma / beta host float[cols].  avd_softmax: y = exp(x - max) / sum
 * over rows of cols float32 logits, any cols >= 1 (whole float4s up to 4096 stay in registers; 1000 = the CNN's classes).  If timing_reps > 0 and ms != NULL the kernel alone is launched timing_reps more times between two HIP
 * events and its mean duration is returned (bench hook). */
int avd_layernorm(avd_ctx* ctx, const void* x, int mem, int bf16, int64_t rows, int cols, const float* gamma, const float* beta,
                  float eps, void* y, int timing_reps, float* ms);
int avd_softmax(avd_ctx* ctx, const float* x, int mem, int64_t rows, int cols, float* y, int timing_reps, float* ms);

/* Audio analyzer: the per-window loop of reference app/analyzers/audio.py:40-61 for every window of a
 * mono float32 waveform at once.  wav: n samples (host or device); win: samples per window (the reference uses
 * int(sr * 0.5) = 8000 at 16 kHz; at most 8192); windows: host array of ceil(n / win) records, filled in order (the
 * last window may be shorter).  n = 0 is AVD_OK and writes nothing; win outside 1 ... 8192 (whatever n is), n < 0, a null wav or windows with n > 0
 * and max_windows < ceil(n / win) are AVD_ERR_ARG, and the context takes the next call as if the refused one had not been made.  From a record the reference's per-window values follow as
 *   rms = sqrt(sumsq / length); zcr = float32(zero_cross) / float32(length - 1) / 2;
 *   flatness = exp(sum_log / nbins) / (sum_mag / nbins); rolloff = rolloff_index / max(1, nbins);
 *   centroid = sum_fmag / sum_mag          (mag = |rfft(seg * hanning)| + 1e-9, all sums in double)
 * and the scalar tail (audio.py:63-110) is host numpy (avd_hip/audio.py).  sumsq is accumulated in double where
 * audio.py:44 squares and averages in float32 (a deliberate deviation, inside 1e-6 of the reference's rms).
 *
 * Two options of avd_set_option shape a call; with both at their defaults every call is what it was before they existed.  No function and no
 * AVD_FMT_* value is added, and AVD_ABI_VERSION stays 3.
 *   "audio_format" (durable, reads back): 0 (default) float32 samples; 1 little-endian int16 PCM -- wav then points at int16 samples, n still
 *     counts samples, and sample s is the float32 value (float)s * 2^-15: exact for all 65536 values, and what a 16-bit file read as float32
 *     gives (the reference's input).  The samples are widened in registers; host input is staged as 2 * n bytes.  Any other value is
 *     AVD_ERR_ARG with a message that begins "audio_format:", and the old value stays.  With format 1 an odd wav address is AVD_ERR_ARG before
 *     anything is staged.
 *   "audio_cut" (one-shot, for the NEXT avd_audio_features call): a value s > 0 says that a track ends and the next one begins at sample s of that
 *     call's buffer.  Cuts are set one at a time in strictly ascending order, at most 63 (64 tracks); -1 clears the list; the option reads back as
 *     the number of cuts held.  A value of 0 or below other than -1, a value not above the last cut and a 64th cut are AVD_ERR_ARG with a message
 *     that begins "audio_cut:", and the list stays as it was.  The next avd_audio_features call takes the list whether it succeeds, is refused
 *     or fails: a forgotten list never splits a later call.
 *     With cuts c1 < ... < ck the n samples are k + 1 tracks [0, c1), [c1, c2), ..., [ck, n), each windowed from its own start with its own short
 *     last window; windows receives the records track after track, ceil(n_t / win) per track, and the records of a track are byte for byte those
 *     of avd_audio_features on that track's samples alone.  Checked after the argument checks above and before anything is staged, in this order:
 *     a cut >= n is AVD_ERR_ARG ("audio_cut: beyond the buffer"); max_windows below the sum of the tracks' window counts is AVD_ERR_ARG.  n = 0
 *     with cuts pending is AVD_OK, writes nothing and clears the list.
 *
 * Tracks at the decoder's rate.  Two more durable options put a converter in front of the analyzer, on the device: what the reference's
 * "ffmpeg -ac 1 -ar 16000 -f wav" does (audio.py:10) -- downmix to mono, resample to 16 kHz, narrow to 16 bit.  With both at their defaults
 * every call and every record is byte for byte what it was before they existed.
 *   "audio_rate" (durable, reads back): 0 (default) the samples are at the analysis rate already.  One of 8000, 11025, 12000, 16000, 22050,
 *     24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000: wav holds n sample FRAMES at that rate.  Any other value is AVD_ERR_ARG with a
 *     message that begins "audio_rate:", and the old value stays.
 *   "audio_channels" (durable, reads back; read only while "audio_rate" is not 0): 1 (default) or 2 interleaved samples per frame.  Any other
 *     value is AVD_ERR_ARG with a message that begins "audio_channels:".  Not read while "audio_layout" is not 0, which covers every other
 *     shape a decoder hands over: planar samples, 5.1 and 7.1 (below).
 * While "audio_rate" is not 0: "audio_format" gives the sample type of the input (n * channels samples); win, max_windows and the records refer
 * to the 16 kHz OUTPUT; "audio_cut" positions are input frames; each track is converted from its own start with zeros beyond both of its ends
 * and has ceil(n_t * U / D) output samples, and its records are byte for byte those of the track alone.  The analyzer sees an output sample y
 * exactly as it sees an int16 sample under "audio_format" 1: (float)y * 2^-15.  Checks, all before anything is staged, in this order: the
 * argument checks above; alignment -- 2 bytes for int16 ("audio_format 1: ..."), 4 bytes for float32 ("audio_rate: float32 samples need a
 * 4-byte aligned wav"); a cut >= n ("audio_cut: beyond the buffer"); more than 2^31 - 1 output samples ("audio_rate: ..."); max_windows below the
 * OUTPUT's window count.  A refused call leaves the context as if it had not been made; the cut list remains one-shot.
 *
 * The conversion is a stated rule.  It is modelled on libswresample's defaults (a Kaiser-windowed sinc with beta = 9, a 32-tap base length,
 * cutoff 0.97, a 16-bit fixed-point filter bank, a 16-bit result) and is unpinned against a real ffmpeg: no libswresample was at hand to compare
 * with, so nothing here promises ffmpeg's bits.  After step 1 it is integer arithmetic throughout, so a restatement matches it bit for bit
 * (tests/audio_resample_reference.py).  R the rate, g = gcd(R, 16000), U = 16000 / g, D = R / g.
 *   1. Narrow.  An int16 sample is itself.  A float32 sample x is clamp(rint(x * 32768), -32768, 32767), ties to even; NaN is 0, +-inf clamp.
 *   2. Downmix.  M = (sum_c w_c s_c + 16384) >> 15 with the layout's Q15 weights w_c (below), the shift arithmetic.  |sum| is at most 2^30, so
 *      a 32-bit accumulator is exact and nothing is clamped.  One channel, w = {32768}: M = s.  Two, w = {16384, 16384}: M = floor((L + R + 1) / 2).
 *   3. Filter bank (none at R = 16000, which is steps 1 and 2 only; T is then reported as 0).  f = min(1, 0.97 U / D), T = 2 ceil(16 / f) taps
 *      per phase (48000: U 1, D 3, T 100; 44100: U 160, D 441, T 92).  For phase p in [0, U) and tap k in [0, T): x = (k - T/2 + 1) - p / U,
 *      h = f sinc(f x) I0(9 sqrt(1 - (2 x / T)^2)) / I0(9) with sinc(t) = sin(pi t) / (pi t), h = 0 where the root's argument is negative, all in
 *      double; q[p][k] = rint(h / sum_k h * 32768); then 32768 - sum_k q is added to the tap with the largest h (the lowest k on a tie), so every
 *      phase sums to exactly 32768.  Built on the host once per rate and context.
 *   4. Output m in [0, ceil(n U / D)): i0 = floor(m D / U), p = (m D) mod U, acc = sum_k q[p][k] M[i0 - T/2 + 1 + k] with M = 0 outside the
 *      track, y = clamp((acc + 16384) >> 15, -32768, 32767), the shift arithmetic.
 * sum_k |q| is at most 63760 at the downsampling rates (a 32-bit accumulator is exact) and 77084, with entries up to 32768, at 8000, 11025 and
 * 12000 (64-bit accumulator, 32-bit entries).  A 1 kHz sine of 20000 peak comes back within 5 LSB from 48000 and 44100; a 10 kHz tone at 48000
 * leaves at most 3 LSB.
 * avd_debug_fetch, of the last call that ran, if it converted (an error otherwise): "audio_rs_plan" int32[8] -- rate, channels, U, D, T, outputs
 * per tile (a tile: one workgroup's run of outputs of one track), input frames, output samples; "audio_rs_taps" int32[U][T]; "audio_rs_tracks"
 * int32[tracks][2] -- per track its first output sample and its output samples; "audio_pcm" int16[output samples] -- the converted tracks side
 * by side (an error after avd_release_workspace).  "audio_plan", "audio_tracks", "audio_xw" and "audio_mag" then describe the analysis of that output.
 *
 * Tracks as the decoder hands them over: planar samples, 5.1 and 7.1.  libavcodec's AAC, Opus, MP3, Vorbis and AC-3 decoders emit PLANAR samples,
 * one plane per channel (PyAV's AudioFrame.to_ndarray() is [channels, samples]); film and broadcast tracks have six or eight channels.  Two more
 * durable options let such a buffer go to the device as it is -- no host transpose, no host downmix.  No function is added and AVD_ABI_VERSION
 * stays 3; with both at their defaults every call enqueues and returns exactly what it did before they existed.
 *   "audio_layout" (durable, reads back; read only while "audio_rate" is not 0): 0 (default) -- "audio_channels" decides.  Otherwise id | flags.
 *     The id is the channel count, the order FFmpeg's and WAVE's native one: AVD_AUDIO_LAYOUT_MONO 1; AVD_AUDIO_LAYOUT_STEREO 2, FL FR;
 *     AVD_AUDIO_LAYOUT_5POINT1 6, FL FR FC LFE BL BR (side surrounds take the back slots); AVD_AUDIO_LAYOUT_7POINT1 8, FL FR FC LFE BL BR SL SR.
 *     Flag AVD_AUDIO_PLANAR 0x100: one plane per channel.  Any other value is AVD_ERR_ARG with a message that begins "audio_layout:", and the old
 *     value stays.  While the option is not 0, "audio_channels" is not read.
 *   "audio_plane_stride" (durable, reads back; read only with the planar flag): the distance in SAMPLES from plane c to plane c + 1.  0 (default)
 *     means n, the call's frame count: a dense [channels, n] buffer.  A negative value is AVD_ERR_ARG ("audio_plane_stride: ...") at the set; a
 *     non-zero value below n is refused at the call ("audio_plane_stride: ..."), after the alignment check and before every later check.
 * Addressing.  Planar: wav points at plane 0, plane c begins c * stride samples further.  n, "audio_cut" positions and the per-track extents of
 * a list call count frames WITHIN EACH PLANE: several tracks in one call are joined along the frame axis (np.concatenate(tracks, axis=1)).
 * Interleaved 5.1 / 7.1: frames of 6 / 8 samples, as stereo has 2.  Alignment is the sample type's, for wav; the stride is in samples, so every
 * plane inherits it.  Host input: a dense buffer is staged in one copy; a strided one plane by plane into a dense device buffer -- no byte
 * twice, none outside the planes; debug buffer "stage_bytes" then says channels * n * sizeof(sample) ("stage_copies": 1, or the channel count).
 * Device input is read in place with its stride ("stage_bytes" 0).
 * The weights of step 2 come from gains g: FC 1, FL / FR sqrt(1/2), back and side 1/2, LFE 0.  They are modelled on libswresample's default
 * matrix for "-ac 1" and, like the rest of the rule, unpinned against a real ffmpeg.  w_c = rint(g_c / sum g * 32768); then 32768 - sum w is
 * added to the channel with the largest g (the lowest index on a tie), so every row sums to exactly 32768:
 *     mono {32768}    stereo {16384, 16384}    5.1 {6786, 6786, 9598, 0, 4799, 4799}    7.1 {5249, 5249, 7422, 0, 3712, 3712, 3712, 3712}
 * Narrowing (step 1) stays per sample and comes before the mix.  So layouts 1 and 2, interleaved, are byte for byte "audio_channels" 1 and 2,
 * and planar stereo is interleaved stereo on the same samples.  A channel of weight 0 contributes nothing whatever it holds; a planar LFE plane
 * is not even read.
 * The layout goes through every call form: whole tracks, "audio_cut" batches, audio slots and "audio_track_slot" lists.  A slot remembers the
 * layout of its first call with win, rate and format -- another layout on a filled slot is refused where those mismatches are, with their
 * message -- while the plane stride may differ from call to call.  The history a slot keeps is the downmixed frames.
 * avd_debug_fetch "audio_layout" int32[12], host state of the last call that converted (an error before any did): the layout id (0: the call
 * went by "audio_channels"), planar 0 / 1, channels, the plane stride of the caller's buffer in effect (0: interleaved), the eight weights,
 * zero-filled.  "audio_rs_plan"[1] reports the channel count.
 *
 * A track continued across calls (audio slots).  A decoder hands audio out in packets; four more options let a track arrive in as many
 * avd_audio_features calls as the caller likes, in bounded memory, with the records of the whole track.  No function is added and AVD_ABI_VERSION
 * stays 3; with these options at their defaults every call enqueues and returns exactly what it did before they existed.
 *   "audio_slot" (durable, reads back; default 0): 0 -- every call is a whole track.  k = 1 ... 8 -- an avd_audio_features call continues the
 *     track of audio slot k.  Any other value is AVD_ERR_ARG with a message that begins "audio_slot:", and the old value stays.  The audio slots
 *     are apart from the video stream slots: "stream_slot", "stream_map" and "stream_reset" do not touch them, and these options do not touch those.
 *   "audio_end" (one-shot, for the NEXT avd_audio_features call; the value is 1, any other value is AVD_ERR_ARG with a message that begins
 *     "audio_end:"; reads back as 0 or 1): that call carries the last samples of its slot's track.  The next avd_audio_features call takes it
 *     whether it succeeds, is refused or fails, exactly like the "audio_cut" list.  With slot 0 selected it has no effect.
 *   "audio_slot_reset": k = 1 ... 8 empties audio slot k, 0 empties all eight; reads back as 0.
 *   Read-only, of the selected slot; all are 0 with slot 0 selected and for an empty slot (so also after an "audio_end" call):
 *     "audio_slot_frames" -- input frames absorbed, saturated at 2^31 - 1; "audio_slot_held" -- analysis-rate samples held back, fewer than win;
 *     "audio_slot_windows" -- records the last call on this slot wrote.
 * The rule.  N is the frames a slot has absorbed, the present call included.  U, D and T belong to the rate as above (T the taps per phase);
 * with "audio_rate" 0 take U = D = 1 and T = 0.  The outputs that exist after a call that is not the last are
 *     M(N) = ceil(max(0, N - T/2) U / D)
 * -- exactly the outputs m whose last tap floor(m D / U) + T/2 lies at or below frame N - 1.  After the last call M = ceil(N U / D), with zeros
 * beyond the end as in a whole-track call.  The windows handed out so far are W = floor(M / win), and ceil(M / win) after the last call.
 *   - A call writes records W_before ... W_after - 1 of the track into windows, in order, and needs max_windows >= W_after - W_before.
 *   - Output samples [W_after win, M) stay on the device, in the slot, as do the last min(N, T - 1) frames, already narrowed and downmixed
 *     (steps 1 and 2 are per frame, so carrying mono int16 is exact).  A track with "audio_rate" 0 holds its samples in their own type.
 *   - After an "audio_end" call the slot is empty.
 *   - n = 0 is allowed: nothing happens without "audio_end" (the call wrote no record: "audio_slot_windows" then reads 0), and the track is
 *     flushed with it; a null wav is then accepted, as for n = 0 today.  A call that writes no record accepts a null windows.
 * Guarantee: for any split of a track into calls, the concatenated records are byte for byte the records of ONE slot-0 call on the joined
 * samples, and the concatenated new outputs (debug buffer "audio_pcm", which after a slot call holds that call's new outputs only) equal that
 * call's "audio_pcm" -- for float32 and int16 input, every rate, mono and stereo, host and device memory.
 * Refusals: after the argument and alignment checks above (with a slot selected float32 samples need a 4-byte aligned wav at every rate), all
 * before anything is staged, the slot untouched, each AVD_ERR_ARG with a message that begins "audio_slot:", in this order: a pending
 * "audio_cut" list (one track per call); win, "audio_rate", "audio_channels" or "audio_format" other than at the slot's first call; more than
 * 2^31 - 1 outputs for the track; max_windows too small.
 * A slot is state, not scratch (36 KB of device memory each, allocated by the slot's first call): it survives avd_release_workspace and every
 * other call on the context -- slot-0 audio calls, video, the extensions; avd_destroy frees it.  A call that fails before its save launch (the
 * one launch that writes the slot) is enqueued leaves the slot as it was; a call that fails later empties the slot and says so in the error
 * text.  A pending asynchronous analysis is drained first, as by every avd_audio_features call; no host round trip is added.
 * "audio_rs_plan" after a slot call that converted: input frames and output samples are the call's own (its new outputs; 0 is possible), and
 * "audio_rs_tracks" gives where the new outputs begin in the analyzer's buffer -- behind the held samples -- and their count.  A slot call
 * that completes no window runs no analysis: "audio_plan", "audio_tracks", "audio_xw" and "audio_mag" then still describe the last call that did.
 *
 * Several continued tracks per call.  A service that follows K live streams hands over a ROUND of them at once: one more option joins "several
 * tracks per call" ("audio_cut") and "a track across calls" (the audio slots).  No function is added and AVD_ABI_VERSION stays 3; with an empty
 * list every call enqueues and returns exactly what it did before the option existed.
 *   "audio_track_slot" (one-shot list for the NEXT avd_audio_features call, in the manner of "audio_cut"): entries are set one at a time, in track
 *     order; entry i says what track i of that call is, the tracks being counted by the call's cut list.  Low four bits 0: a whole track, as
 *     today.  Low four bits k = 1 ... 8: the track continues audio slot k.  Bit 0x10: the call carries that slot's last samples -- the per-track
 *     form of "audio_end".  -1 clears the list; the option reads back as the number of entries held; at most 64 entries.  Each of these is
 *     AVD_ERR_ARG with a message that begins "audio_track_slot:" and leaves the list as it was: 0x10 with slot 0; a slot already in the list; a
 *     65th entry; any other bit or a slot above 8; a set while "audio_slot" is not 0.  Setting "audio_slot" to a non-zero value while the list is
 *     not empty is refused the same way ("audio_slot: ..."), and the old value stays: the two ways of choosing slots never hold at once, as with
 *     "stream_slot" / "stream_map".  The next avd_audio_features call takes the list whether it succeeds, is refused or fails.
 * A call with a list of t entries: the buffer holds t tracks under "audio_cut" (so every track has at least one sample; a stream that ends with
 * nothing left to give is flushed by a single-slot call with n = 0; n = 0 with a list of ONE entry is that entry's empty call).  All tracks share
 * win and the context's "audio_rate", "audio_channels" and "audio_format": one rate means one filter bank per call.  Each continued track
 * follows the slot rule above unchanged -- it forms outputs [M_before, M_after) behind its slot's held samples, writes records W_before ...
 * W_after - 1, leaves the new history and held remainder in its slot, and with 0x10 empties the slot; whole tracks are what they are in a cut
 * call.  windows receives the records track after track in call order; a track may write none; max_windows must cover the sum, and a null
 * windows is accepted only when that sum is 0.
 * Guarantee: take any number of tracks, any split of each into chunks, and any assignment of chunks to calls and to positions within a call.
 * Then each track's concatenated records are byte for byte those of ONE slot-0 call on its joined samples, and its concatenated new outputs equal
 * that call's "audio_pcm"; a call through a list and a call through "audio_slot" may alternate on one slot; and a list of zeros gives the
 * records and the debug buffers of the same call without a list.
 * Refusals of a list call, all before anything is staged, every slot untouched, each AVD_ERR_ARG, checked in this order: (1) the argument checks
 * above; (2) alignment -- 2 bytes for int16, 4 bytes for float32 at every rate, as for a slot call; (3) a cut beyond the buffer ("audio_cut:
 * beyond the buffer"); (4) a pending "audio_end" ("audio_track_slot: ends are given in the list"), which consumes both the end and the list;
 * (5) a number of entries other than cuts + 1; (6) for a filled slot, win, rate, channels or format other than at its first call; (7) a track
 * beyond 2^31 - 1 outputs, or more than 2^31 - 1 samples in the analyzer's buffer of all tracks together; (8) max_windows below the sum of the
 * tracks' records, or a null windows with records to write, then more than 2^24 records.  (4) ... (8) begin "audio_track_slot:".
 * Atomicity: every slot's memory is reserved before the first launch; the save is the last launch; the host state of all slots moves only after
 * the call has drained.  A failure before the save launch leaves every slot as it was; a failure after it empties every slot the call continued,
 * and says so in the error text.  However many tracks a call has, it runs at most ONE launch of each kind: a gather (every continued track's held
 * samples to the front of its region of the analyzer's buffer; with "audio_rate" 0 the call's own samples behind them), the converter (each
 * tile reads its own track's source: chunk, frames absorbed before, history), the analyzer's passes over one window table, the save.
 * avd_debug_fetch after a list call: "audio_tracks" has one row per track (a track may have count 0); "audio_rs_tracks" gives per track where its
 * new outputs lie in the analyzer's buffer and how many; "audio_pcm" is the tracks' new outputs side by side in track order; "audio_map_call"
 * int32[6] -- tracks, continued tracks, gather launches, converter launches, analyzer passes, save launches (each of the last four 0 or 1) -- is
 * an error before the first list call.  "audio_slot_frames" / "audio_slot_held" / "audio_slot_windows" keep their meaning: select a slot after
 * the call to read them; "audio_slot_windows" is what the last call that continued this slot wrote for it.
 *
 * avd_debug_fetch, host state of the last call that ran: "audio_tracks" int32[tracks][3] -- per track its first window, its windows and the length
 * of its last window; "audio_plan" int32[4] -- windows of all tracks, win, the LAST track's last length, windows of all tracks that took the
 * 80 x 100 transform; "audio_host" int32[2] -- the microseconds the host spent forming the tables of the call's short window lengths, and how
 * many distinct short lengths it had.  "audio_xw" double[windows][win] and "audio_mag" double[windows][win / 2 + 1] are indexed by the call's window number. */
typedef struct avd_audio_window {
    double sumsq;            /* sum of seg^2                                             (audio.py:44) */
    double sum_log;          /* sum of log(mag)                                          (audio.py:50) */
    double sum_mag;          /* sum of mag                                               (audio.py:50,51,61) */
    double sum_fmag;         /* sum of linspace(0,1,nbins) * mag                         (audio.py:60-61) */
    int32_t zero_cross;      /* sum of |diff(sign(seg))|                                 (audio.py:45) */
    int32_t length;          /* samples in this window */
    int32_t rolloff_index;   /* first k with running sum >= 0.85 * sum_mag, else 0       (audio.py:51-58) */
    int32_t nbins;           /* length / 2 + 1 */
} avd_audio_window;          /* 48 bytes */
/* option "audio_layout": id | flags (0: "audio_channels" decides) */
#define AVD_AUDIO_LAYOUT_MONO    1
#define AVD_AUDIO_LAYOUT_STEREO  2      /* FL FR */
#define AVD_AUDIO_LAYOUT_5POINT1 6      /* FL FR FC LFE BL BR */
#define AVD_AUDIO_LAYOUT_7POINT1 8      /* FL FR FC LFE BL BR SL SR */
#define AVD_AUDIO_PLANAR         0x100  /* one plane per channel, "audio_plane_stride" samples apart */
int avd_audio_features(avd_ctx* ctx, const float* wav, int mem, int64_t n, int win, avd_audio_window* windows, int max_windows);

/* The one exchange step of the path: frames and clips shard across GPUs with no data-path collective;
 * only the 32-byte records are reassembled, with ONE RCCL all-gather over xGMI per batch (a few KB: latency-bound).
 * RCCL is bound at run time (dlopen), so single-GPU use never loads it.  avd_comm_unique_id: one rank creates the
 * 128-byte id and the caller distributes it (file, environment, torch's store ...); avd_comm_init: every rank, with
 * its own context (one process per GPU); avd_allgather_records: every rank passes `count` records (the same count on
 * every rank: whole clips per rank, or shards padded by the caller) and receives world * count in rank order.
 * Host pointers; the call blocks until the gathered records are in `all`. */
int avd_comm_unique_id(void* id128);
int avd_comm_init(avd_ctx* ctx, int rank, int world, const void* id128);
int avd_allgather_records(avd_ctx* ctx, const avd_frame_record* local, int count, avd_frame_record* all);
/* The same exchange straight from the device: the first `count` records of this context's LAST avd_analyze_* call
 * (blocking or asynchronous) are gathered from where k_records left them in HBM -- the collective is enqueued on the
 * context's stream behind the analysis, one copy brings the world * count gathered records to `all` (host).  Blocks until
 * they are there; an outstanding asynchronous call is drained too (its own records buffer is filled).
 * Refused (AVD_ERR_UNSUPPORTED, before the communicator is looked at) when that call ran under a non-empty option "stream_map": its own
 * records are then several runs in HBM with the restored frames' between them, and they are not compacted on the device. */
int avd_allgather_last_records(avd_ctx* ctx, int count, avd_frame_record* all);

/* Stream ordering for AVD_MEM_DEVICE inputs.  A context launches on its own non-blocking stream, so device memory
 * that another stream is still writing (e.g. torch's current stream: a freshly computed tensor, a .contiguous()
 * copy, a decoder's colour-conversion kernel) must be ordered explicitly: everything enqueued on `producer_stream`
 * (a hipStream_t passed as a plain pointer; NULL = the default stream) before this call completes before anything
 * submitted to ctx afterwards starts.  No host synchronisation.  The caller keeps the input buffer alive until
 * avd_synchronize / the blocking call returns. */
int avd_wait_stream(avd_ctx* ctx, void* producer_stream);

/* Free the context's scratch memory (about 1.5 GB after a 120-frame 1080p clip) but keep the context; the next
 * call reserves it again.  Weights uploaded with avd_cnn_set_weights / avd_vit_set_weights are state, not scratch: they
 * stay.  For services that keep a pool of idle contexts. */
int avd_release_workspace(avd_ctx* ctx);

/* HIP-event timing of the work enqueued on ctx's stream between the two calls
 * (milliseconds).  avd_timer_stop synchronizes the stream. */
int avd_timer_start(avd_ctx* ctx);
int avd_timer_stop(avd_ctx* ctx, float* elapsed_ms);
/* Per-stage device time (ms, HIP events on ctx's stream) of the LAST avd_analyze_frames*
 * call when profiling was enabled with avd_set_profiling(ctx, 1): stage 0 = staging copies, fused
 * preprocess kernel (+ the 2 KB moment memset) and aHash kernel of every clip of the call, 1 = upload of the clip-start
 * table (calls with several clips; otherwise empty), 2 = Farneback (pyramid .. flow) + flow statistics + the record kernel
 * (Hamming distances, record assembly), 3 = records copy-out; 4 = the 320-px pyramid level of the call's LAST Farneback chunk
 * (a call of more than 513 frames has several), between events of its own inside stage 2 -- by mode:
 *   fb_mode 1 (fast)                      the level's THREE launches, one per blur iteration, between one pair of events;
 *   fb_mode 0, bit 0 of "fb_fused" set    the fused level kernel: all three iterations in ONE launch, events around it;
 *   fb_mode 0, bit 0 of "fb_fused" clear  the two-kernel path: the MEAN duration of one k_uv launch (three of them, one per iteration);
 * 5 = the mean duration of one k_hscan<320> launch in the last of these three cases, and 0 in the other two.
 * The LAST call is the last DRAINED one: an asynchronous call changes nothing before avd_synchronize.
 * Stages 0 .. 3 tile the call: each ends at the event the next begins at.  The kernel regions of avd_kernel_ms that were recorded when the call
 * was enqueued tile the same interval, and the region that opens a stage is bounded by the stage's OWN event: the regions inside a stage sum
 * to that stage (0: AVD_K_PREPROCESS + AVD_K_HASH; 1 + 3: AVD_K_OTHER; 2: the Farneback, statistics and record ids), up to float rounding.
 * All six are 0 until a profiled call has been drained, and keep the values of the last such call: a call made with profiling off, or any
 * other entry point, leaves them alone. */
int avd_set_profiling(avd_ctx* ctx, int enable);
/* Tuning / test switches.  "fb_mode": 1 (default; environment AVD_FB_MODE=fast) = the fast Farneback level kernel
 * (csrc/avd_fbfast.hip: a pair is spread over several workgroups; cv2's vertical running sums are kept literally, the
 * horizontal 15-column window sums are formed directly in double instead of as cv2's running double sum: the flow equals
 * the exact kernels' bit for bit on well-posed inputs, within 1e-5 px otherwise) WITH the exact re-run of the pairs it cannot follow.
 * Two criteria, evaluated by the level kernels at every pixel, iteration and level (derivation: profiles/r04_experiments.md section 1,
 * profiles/r05_experiments.md section 1; tools/experiments/fb_illposed_run.py):
 *   solver      the 2 x 2 normal equations are singular over whole regions -- determinant cancellation above 2000, or a displacement
 *               above 0.3 of the level width: the reference's own flow is chaotic there (ramps, stripes, isolated straight edges);
 *   border sign a flow component at the top / left image border is smaller than 1e-10 px (the size of the rounding residue of cv2's own
 *               running sums) while cv2's warp decides "inside the image" / "outside" by its SIGN and the two branches differ there:
 *               exactly periodic or static content whose true flow is zero (checkerboards; bit-identical frames but for a small patch).
 *               A pair of bit-identical frames is exempt (its zero flow is structural in cv2 too).
 * The host reads the flag words (with the records) and sends flagged pairs through the exact kernels before anything is handed to the caller,
 * so their results are the exact kernels', bit for bit: nothing is launched when nothing is flagged; up to 32 flagged pairs of a chunk run the
 * 160- / 320-px levels through the two-kernel path (a pair spread over many workgroups), more run the fused kernels (one workgroup per pair: a
 * clip of nothing but flagged pairs costs the exact mode's time -- a flagged pair leaves the fast launches at once).
 * avd_frame_record.reserved is non-zero for the frame that closes such a pair; avd_get_option "rerun_pairs" counts
 * them for the last drained call.  Stated guarantee of the mode, with no exception for any content: flow_mean / flow_var within rel 1e-6 and
 * ai_susp within 1e-6 of the oracle (north_star: 1e-4), tests/test_gpu_fbfast.py + the content soak over 28 families in tests/test_gpu_soak.py.
 * "fb_rerun" (default 1, environment AVD_FB_RERUN): 0 switches the re-run off (A/B, tests).  "fb_rerun_fused" (default 0xC): level mask of the
 * fused kernel in the few-pairs re-run (bit 3 is always set); no effect on results.
 * "tail_help" (default 1; no effect on results): the flag words of an asynchronous call's last chunk reach the host with its records, and the host
 * enqueues the re-run.  With the option on, a thread that waits in avd_synchronize -- for its own fast pass or its own re-run -- does that for the
 * OTHER contexts of the device whose records have arrived, instead of each clip's re-run starting only when its own avd_synchronize is reached
 * (one host thread, three fully flagged 120-frame clips in flight: 76 k -> 111 k frames/s; nothing flagged: no difference).  0 = wait in the runtime.
 * 0 (AVD_FB_MODE=exact) = the exact kernels, bit-identical to the oracle everywhere, one workgroup per pair.
 * "fb_fold_up" (fast mode, bit mask, default 5, environment AVD_FB_FOLD_UP; no effect on results): 1 = the first launch of the 320-px level
 * resizes the 160-px level's flow itself instead of reading the output of a separate resize launch; 2 = the 160- and 80-px levels do so in a
 * prologue of their first launch; 4 = the 80- and 40-px levels (a pair is one workgroup there) run their three iterations in one launch.
 * "fb_fold_up160" (fast mode, default 1, environment AVD_FB_FOLD_UP160; no effect on results): the first launch of the 160-px level resizes the
 * 80-px level's flow itself, as bit 1 of "fb_fold_up" does at 320 px, whenever the call runs that level as one strip per pair ("fb_wide160");
 * with two strips per pair it changes nothing and "fb_fold_up" decides.
 * "fb_fold_blur" (default 1, environment AVD_FB_FOLD_BLUR; no effect on results): the 3 x 3 Gaussian of the 320-px pyramid scale is formed inside
 * the polynomial expansion (same two float passes, same operation order) instead of being written by the pyramid kernel and read back;
 * avd_debug_fetch "pyr0" exists with the option off only (an error otherwise: the buffer is not even allocated).
 * "fb_wide160" (fast mode, environment AVD_FB_WIDE160): 1 = the 160-px level runs a pair as ONE strip of three 64-column blocks
 * (119 workgroups, fewer CU-microseconds: +2.4 % frames/s with clips in flight), 0 = as two 80-column strips (238 workgroups, each
 * launch 10 us shorter: one clip alone finishes ~25 us sooner), 2 (default) = chosen ONCE when the call is enqueued, for all its launches: one strip if another context of the
 * process holds an undrained avd_analyze_* call, two strips if this clip has the chip to itself.  Same guarantee; the two shapes group the solver's
 * window sums differently (bit-identical on well-posed content, tests/test_gpu_fbfast.py).
 * "fb_wide320" (fast mode, environment AVD_FB_WIDE320; no effect on results): the shape of the 320-px level's launches that read a 320-px flow
 * (its second and third; with bit 1 of "fb_fold_up" clear the first as well).  1 = a pair is ONE workgroup of five 64-column blocks, 15 waves:
 * every lane on an image column, no halo columns computed twice, no masked solver lanes (a launch takes 203 us on 120 CUs instead of 124 us on 238:
 * -18 % CU-microseconds, +2.5 % frames/s with three clips in flight); 0 = two strips of three blocks, 12 waves each (one clip alone finishes 0.16 ms sooner);
 * 2 (default) = chosen once per call by what is in flight, exactly as "fb_wide160" = 2.  Every column is computed by the same instructions on the same
 * operands in both shapes: flow, |flow| and flag words are bit-identical on any content (tests/test_gpu_fbfast_wide320.py).  Read-only
 * "fb_wide320_used": the shape the last fast-mode call took; avd_debug_fetch "fb_wide320_launches" (int32[1]): its launches in the new shape.
 * "fb_wide320_up" (default 1, environment AVD_FB_WIDE320_UP; no effect on results): 1 = the level's first launch, which resizes the 160-px flow
 * itself (bit 1 of "fb_fold_up"), takes the five-block shape as well whenever the call does -- each normal-equation wave resizes the flow of its
 * own columns in registers; 0 = that launch stays in two strips.  avd_debug_fetch "fb_wide320_up_launches" (int32[1]) counts it apart from
 * "fb_wide320_launches", which keeps counting the launches that read a 320-px flow.
 * "fb_fused" (exact mode only, no effect on results): bit k set = pyramid level k (0 = 320x320 .. 3 = 40x40)
 * of the Farneback stage runs the fused level kernel (default 0xF, or the environment variable AVD_FB_FUSED at
 * avd_create); clear = the two-kernel path that exchanges its double intermediate through HBM.  "cnn_tiles": tiling of the
 * CNN extension's convolutions, 0 = by layer shape (default), 1 = 256-pixel tiles everywhere, 2 = 128 x 128 tiles wherever the
 * channel count allows (the accumulation order of an output does not depend on the tiling: results are bit-identical).
 * "cnn_fuse" (default 2): a bottleneck block's 3x3 and its expanding 1x1 run as ONE launch in the 56x56 and 28x28 stages
 * (the mid activation stays in LDS; bit-identical to the two layers); 2 = in their stride-1 blocks the 3x3 also reads its nine taps from one
 * copy of its input in LDS instead of gathering them tap by tap; 1 = gathering form everywhere; 0 = layer by layer.  "cnn_chunk" (default 128, 1 ... 1024):
 * frames per forward pass of avd_cnn_forward (activation scratch: 4 x 1.6 MB per frame).
 * "cnn_tap" (tests; default 0 = off, 0 ... 56, anything else is refused): avd_cnn_forward copies ONE intermediate aside, device to device on the
 * context's stream right after the launch that produces it, for avd_debug_fetch "cnn_tap": 1 = the zero-bordered input image, 2 + i = the output of
 * convolution i (avd_cnn_set_weights order, 0 = stem ... 52), 55 = the max pool's output, 56 = the pooled features.  While it is set, a call with more
 * frames than one pass ("cnn_chunk") or with timing_reps > 0 is refused (AVD_ERR_ARG); at 0 the forward enqueues nothing for it.
 * Stream slots: calls that continue ONE clip (a decoder that hands out 4 to 16 surfaces per call, a live stream of one or two frames per call).
 * "stream_slot" (default 0; 0 ... 8, anything else is refused with AVD_ERR_ARG and the old value stays): 0 = every avd_analyze_* call starts a new clip
 * (first record: ham = -1, flow 0).  With slot k = 1 ... 8 selected, a call of any avd_analyze_* entry (avd_analyze_frames / _nv12 / _i420, avd_analyze_batch,
 * avd_analyze_pictures, avd_analyze_frame_lists and their _async forms) that carries exactly one non-empty clip CONTINUES the clip of slot k: on an empty slot
 * its records are what they are without the option; on a filled one its n records are, bit for bit and in both "fb_mode"s, records [1:] of the same call
 * made on the slot's frame followed by the n frames -- record 0 carries the Hamming distance and the flow statistics of the pair (slot frame, frame 0),
 * with the fast mode's flag word, exact re-run and bit-identical-pair exemption as for any other pair.  After the call the slot holds the call's last frame
 * (its 320 x 320 gray image, 1024 hash bits and Laplacian moments: 103 KB on the device, kept and restored by copies ordered on the context's stream -- no
 * host round trip, no synchronisation; the caller's frame is free once its call is drained).  One clip per call: more than one non-empty clip while a slot is
 * selected is refused (AVD_ERR_ARG, "stream_slot: one clip per call") before anything is staged.  A refused call, a call that fails before it is
 * enqueued and a call without frames leave the slot as it was.  The layout, geometry, rotation and range may change from call to call.  A slot is state,
 * not scratch: it survives avd_release_workspace and every call in between (other slots, slot-0 analyses, avd_preprocess_*, avd_farneback_pairs -- which
 * ignore the option -- audio, the extensions); avd_destroy frees it.  One context has eight slots and so serves up to eight streams in turn,
 * or with "stream_map" (below) several of them in ONE call.
 * avd_debug_fetch "small" of a call that continued a filled slot begins with the slot's frame ("area": with an entry that is not defined).
 * "stream_reset": setting k = 1 ... 8 empties slot k, 0 empties all eight (other values are refused); it reads back as 0.
 * "stream_frames" (read-only): frames the selected slot has absorbed since it was last emptied; 0 for an empty slot and with slot 0 selected.
 * "stream_map": several clips of one call continue a slot each -- a service that watches several live streams, or drains several decoder pools, pays the
 * Farneback launch sequence once per call instead of once per stream (calls of 1 to 8 frames are bound by their launches, not by pixels).  Durable, like
 * "stream_slot".  The value is (position << 4) | slot with position 0 ... 63 and slot 0 ... 8: slot 1 ... 8 makes the clip at position `position` of every
 * following avd_analyze_* call (blocking or asynchronous, whatever entry it is made through) continue that slot, slot 0 unmaps the position; -1 clears
 * the whole map; it reads back as the number of mapped positions.  Refused with AVD_ERR_ARG, the map unchanged and a message that begins "stream_map:":
 * any other value; a slot that is already mapped at another position; any value but -1 while "stream_slot" is not 0.  Setting "stream_slot" to k != 0
 * while the map is not empty is refused too (AVD_ERR_ARG, the old value stays): the two ways of choosing slots never hold at once.  Positions >= 64 cannot
 * be mapped: clips there start new clips.  With a non-empty map a clip at a mapped position continues its slot exactly as the one-clip call with
 * "stream_slot" = k does (an empty slot: today's call; a filled one: its first record is that of the pair (slot frame, frame 0)), a clip at an unmapped
 * position starts a new clip, and the records go out clip after clip, the callers' own frames only.  An empty clip, and a mapped position the call does not
 * list, leave their slot untouched.  Afterwards every continued slot holds its clip's last frame and has absorbed the clip's n frames; "rerun_pairs" counts
 * the flagged records among those handed out.  The slots' frames are restored by ONE launch ahead of the ingest (none if no continued slot is filled) and
 * saved by ONE launch behind the Farneback stage, whatever the number of streams; the Farneback stage runs once over all frames of the call, each
 * continued clip behind its restored frame.  A refused call, a call that fails while it is enqueued and a call without frames leave every slot as it was.
 * avd_preprocess_* and avd_farneback_pairs ignore the map, as they ignore "stream_slot".  After a call made under a non-empty map
 * avd_allgather_last_records is refused (AVD_ERR_UNSUPPORTED, naming stream_map): the restored frames' records lie between the clips' in HBM and
 * compacting them on the device is left out; gather the handed-out records with avd_allgather_records.  Each clip still has its own
 * preprocess and hash launch unless "ingest_group" (below) is set.
 * "ingest_group" (default 0; 0 or 1, anything else is refused with AVD_ERR_ARG, a message that begins "ingest_group:", and the old value stays; durable; no
 * effect on results): with 1 the clips of ONE avd_analyze_* call (any entry, blocking or asynchronous, with or without "stream_map" / "stream_slot") that
 * share a group key are ingested by ONE ingest launch and ONE k_hash launch per group instead of one of each per clip -- a round of eight one-frame
 * streams, or a batch of short clips, is bound by its launches.  The group key: the displayed height and width, the layout, rotate, full range, the row
 * strides of plane 0 and of the planes behind it, and whether the clip may run the 16-byte fills (decided per clip, by the rule it runs under alone):
 * an aligned and a misaligned clip of one layout are two groups, and each group runs the kernel its clips run alone.  Strided clips, frame lists, host
 * and device memory mix freely inside a group; a host clip's staging copies are enqueued ahead of its group's launch, and "stage_bytes" / "stage_copies"
 * are the sums they are without the option.  Groups run in the order of their first clip.  A group of ONE clip runs today's per-clip path, so a call in
 * which no two clips share a key enqueues the same launches under both values; with 0 every call enqueues exactly what it did before the option
 * existed.  The records, and the debug buffers "small", "area", are bit for bit those of option 0.  avd_preprocess_* takes one clip and ignores the option.
 * What a call did is in avd_debug_fetch "ingest_call" and "ingest_groups"; with profiling on there is one AVD_K_PREPROCESS and one AVD_K_HASH region per
 * launch, so a grouped call has fewer.  Experimental while the default is 0.
 * "cv2_model" (default 0, environment AVD_CV2_MODEL read with strtol base 0; durable, survives avd_release_workspace): the library follows the CPU
 * oracle's model switches (oracle/avd_oracle.h, avdo_set_model) -- the implementation choices of the OpenCV wheel that only golden vectors of a real
 * cv2 settle.  The value is a mask with the oracle's own bit values, so one number means the same on both sides:
 *    1  GAUSS_MULADD   the taps of every 32f Gaussian filter of the Farneback stage (pyramid blurs of 3 / 9 / 19 taps) are a rounded product followed
 *                      by a rounded sum, in the order of the default model's fused multiply-add chains (a host without FMA dispatch);
 *    8  THREE_SCALES   scales 80 / 160 / 320 only: the 80-px level is the coarsest and starts from zero flow;
 *   16  RESIZE_LERP    every 32f INTER_LINEAR resize inside Farneback is a + (b - a) * f instead of a * (1 - f) + b * f: the decimations to 80 and
 *                      40 px and the x2 up-sampling of the flow.  The exact-2x area path to 160 px has no lerp and stays.
 * Any combination of 1, 8 and 16 is accepted.  Every other value -- bits 2 and 4 (the oracle's +-1 ulp jitter switches, which model nothing a library
 * can follow), bits from 32 up, negative values -- is refused with AVD_ERR_ARG and a message that begins "cv2_model:", and the old value stays; an
 * environment value that would be refused leaves 0.  With 0 every call enqueues exactly what it did before the option existed.  The option applies to
 * the Farneback stage of every entry that has one: all avd_analyze_* forms (blocking and asynchronous, batches, pictures, lists, under "stream_slot" /
 * "stream_map" / "ingest_group"), avd_farneback_pairs, both "fb_mode"s, and the exact re-run of flagged pairs -- the deferred one of avd_synchronize and
 * the one "tail_help" runs from another thread included: a call follows the model it was ENQUEUED under.  A stream slot holds model-independent data
 * only, so the model may change between the calls of one stream.  The stated guarantee is unchanged with "the oracle" read as "the oracle under the
 * same flags" (oracle.model(mask)): "fb_mode" 0 bit-identical everywhere; "fb_mode" 1 flagged pairs bit for bit, the others within rel 1e-6 on
 * flow_mean / flow_var and 1e-5 px on the dense flow.  The fold options have no effect on results, so under a non-zero model the launcher runs the
 * unfolded forms where only those carry the model's arithmetic: under bit 1 "fb_fold_blur" is taken as 0 (avd_debug_fetch "pyr0" exists), under bit 16
 * bits 1 and 2 of "fb_fold_up" and "fb_fold_up160" are taken as 0 (every initial flow comes from k_flow_up), under bit 8 bit 4 of "fb_fold_up" is taken
 * as 0 (the 80-px level's first iteration is a launch of its own, exempt from the border-sign criterion as the 40-px level's is); avd_get_option keeps returning what the
 * caller set, avd_debug_fetch "fb_model" what was in effect.  Under bit 8: AVD_K_LEVEL40 and AVD_K_FLOWUP80 are exactly 0 (neither is launched; the
 * pyramid and polynomial-expansion launches still form the unused 40-px scale), the remaining regions still tile stage 2, bits 3 and 7 of
 * avd_frame_record.reserved are never set, and in the few-pairs re-run bit 2 of "fb_rerun_fused" is taken as set (the coarsest level runs the fused
 * kernel).  The fast mode's flag thresholds were fuzzed at full size under the default model only; see DESIGN.md section 2 for what was repeated.
 * "audio_format" (0 float32, 1 int16 PCM; durable) and "audio_cut" (the track boundaries of the next avd_audio_features call; one-shot) belong to the
 * audio analyzer and are described at avd_audio_features, as are "audio_rate" (0, or the decoder's rate of the frames handed over: they are converted
 * to 16 kHz mono int16 on the device first; durable) and "audio_channels" (1 or 2 interleaved samples per frame of such a call; durable), and
 * the audio slots: "audio_slot" (0, or the slot 1 ... 8 whose track the calls continue; durable), "audio_end" (the next call ends the track;
 * one-shot), "audio_slot_reset" and the read-only "audio_slot_frames", "audio_slot_held" and "audio_slot_windows".
 * avd_get_option returns the value an option has now (environment defaults included) and the read-only "rerun_pairs" and "stream_frames". */
int avd_set_option(avd_ctx* ctx, const char* name, int value);
int avd_get_option(avd_ctx* ctx, const char* name, int* value);
int avd_stage_ms(avd_ctx* ctx, int stage, float* ms);
/* Per-kernel device time (ms) of the LAST drained avd_analyze_* call with profiling on: HIP events on the context's stream in
 * front of every kernel (group) of the path; a level's figure is the sum of its launches (fast mode: three, one per blur
 * iteration).  bench.py's roofline.kernels is built from these, with clips run alone.  A call with more kernel regions than the library
 * records (96: ~40 clips in one batch) makes avd_kernel_ms fail rather than report partial sums -- for THAT call: the next profiled call
 * reports normally.  Only avd_analyze_* calls count: avd_farneback_pairs, avd_preprocess_* and the extensions run the same launchers but
 * change no figure, nor does an avd_synchronize with nothing pending.  An id whose kernel the call did not launch is exactly 0 (the
 * k_flow_up ids a fold option absorbs, AVD_K_RERUN with nothing flagged, every Farneback id of a one-frame call). */
enum avd_kernel_id {
    AVD_K_PREPROCESS = 0,  /* k_preprocess_vec / k_preprocess, whatever the layout (+ staging copies of host input) */
    AVD_K_HASH,            /* k_hash: 32 x 32 INTER_AREA cells, mean threshold, moment reduction */
    AVD_K_PYRAMID,         /* k_pyramid_all: Gaussian blur + decimation, four scales */
    AVD_K_POLYEXP,         /* k_polyexp_all: polynomial expansion, four scales */
    AVD_K_LEVEL40, AVD_K_FLOWUP80, AVD_K_LEVEL80, AVD_K_FLOWUP160, AVD_K_LEVEL160, AVD_K_FLOWUP320, AVD_K_LEVEL320,
    AVD_K_RERUN,           /* exact re-run of the pairs the fast level kernels flagged; 0 when none was.  The flagged pairs of a call's LAST chunk are re-run when
                            * the call is drained, behind stage 3: that region holds the exact kernels, the second assembly of the chunk's records and their
                            * second copy-out, and lies outside every stage.  Earlier chunks (calls of more than 513 frames) are re-run inside stage 2. */
    AVD_K_STATS,           /* k_stats_pair (exact mode: + k_mag) */
    AVD_K_RECORDS,         /* k_records: Hamming distances, record assembly */
    AVD_K_OTHER,           /* clip-table upload, records copy-out */
    AVD_K_COUNT
};
int avd_kernel_ms(avd_ctx* ctx, int kernel_id, float* ms);

/* Test hook: copy an internal device buffer of the last call to host.
 * name: "area" uint8[n][1024]; "pyr<L>" float[n][hL][wL]; "poly<L>" float[n][hL][wL][5];
 * "flow<L>" float[n-1][2][hL][wL] (planar, after the last iteration at level L).
 * "pairdiff" int32[n-1][20]: per pair (f, f + 1) and tile of the pyramid kernel's 160-px scale (16 source rows and one on either side), non-zero where
 * the two frames differ in the tile's rows; a pair of bit-identical frames is all zero.
 * "ingest_plan" int32[8], host state rather than a device buffer: what the last ingest launch of the context ran --
 * h, w, rows_per_band, nbands, LDS tile pitch, NI of k_preprocess_vec, the staged kernel of BGR24 / RGB24 / RGBP (0: the generic kernel), dynamic LDS bytes requested,
 * kernel (0 bgr_scalar, 1 bgr_vec16, 2 bgr_staged, 3 nv12_scalar, 4 nv12_tables, 5 i420_scalar, 6 i420_tables, 7 nv12_strip, 8 i420_strip, 9 px32_scalar, 10 px32_vec16, 11 rgbp_scalar, 12 rgbp_vec16, 13 rgbp_staged,
 * 14 yuyv_scalar, 15 yuyv_tables, 16 i422_scalar, 17 i422_tables, 18 nv16_scalar, 19 nv16_tables, 20 p010_scalar, 21 p010_tables, 22 i010_scalar,
 * 23 i010_tables, 24 p010_strip, 25 i010_strip;
 * a half turn runs the flipped instantiations of 3 .. 6 and 20 .. 23 under the same ids; AVD_FMT_RGB24 runs 0 .. 2 with its own coefficient constants, BGRA32 and
 * RGBA32 share 9 and 10, YUYV422 and UYVY422 share 14 and 15: "ingest_format" tells them apart); h, w are the displayed picture's; an error before any ingest launch.
 * "ingest_rotate" int32[1], host state: the rotation (quarter turns) that launch ran with; an error before any ingest launch.
 * "ingest_range" int32[1], host state: 1 if that launch ran with full-range conversion constants (AVD_FMT_FULL_RANGE), else 0; an error before
 * any ingest launch.
 * "ingest_format" int32[1], host state: the layout (AVD_FMT_*, without AVD_FMT_FULL_RANGE) of that launch; an error before any ingest launch.
 * "stage_bytes" int64[1], host state: the bytes the last ingest call of the context (avd_preprocess_*, avd_analyze_*) copied from host
 * memory into its staging buffer -- 0 for device input, the sum over the clips of a batch; an error before any ingest call.
 * "stage_copies" int64[1], host state: the host-to-device staging copies that call issued, summed over its clips (a strided clip: its merged
 * spans, 1 to 3; a frame list: one per merged span, n x planes for separately allocated frames); an error before any ingest call.
 * "ingest_list" int32[2], host state: 1 if the last ingest launch took its frame bases from a table of plane pointers (avd_frame_list) and
 * the frames that table held, else 0, 0; 2 and the group's frames for a grouped launch (option "ingest_group"); an error before any ingest launch.
 * "ingest_call" int32[4], host state, of the last avd_analyze_* call that brought frames: its ingest launches, its hash launches, its groups of more than
 * one clip, and the frames those grouped launches ingested -- {live clips, live clips, 0, 0} with option "ingest_group" off; all 0 after a call without
 * frames and before the first call.  (A call refused or failed keeps the figures of the call before it.)
 * "ingest_groups" int32[launches][4], host state, of that call, in launch order: the position of the launch's first clip, its clips, its frames and the
 * kernel id it ran ("ingest_plan"'s last entry).  out_bytes must hold all rows.  "ingest_plan", "ingest_format", "ingest_rotate", "ingest_range" and
 * "ingest_list" keep describing the LAST launch.
 * "cnn_tap": what option "cnn_tap" made the last avd_cnn_forward copy aside -- 1: uint16[n][232][232][4] bf16 bits; 2 + i and 55: the activation as
 * plain NHWC bf16 bits, uint16[n][H][W][C]; 56: float[n][2048].  out_bytes must be exactly the tap's size.  An error, never stale bytes, when the last
 * forward was not tapped, when none of its launches has that output (the 3x3 of a fused block while "cnn_fuse" != 0), or when the size differs.
 * "cnn_plan" int32[53], host state: the kernel shape each convolution of the last avd_cnn_forward ran as -- 0 no launch of its own (the expanding 1x1
 * of a fused block), 1 128 x 128 tiles, 2 256 x 64, 3 256 x 128, 4 256 x 256, 5 the stem, 6 k_conv3_expand, 7 k_slab3_expand (the fused launches are
 * recorded at the block's 3x3); an error before any forward.
 * "audio_plan" int32[4], host state: nwin, win, last (the length of the last window) and nfull (the windows that took the 80 x 100 transform;
 * the others took the direct sum) of the last avd_audio_features call of the context; an error before any such call.
 * "audio_xw" double[nwin][win]: the windowed samples seg * hanning of that call (a short last window fills only its first `last` entries).
 * "audio_mag" double[nwin][win / 2 + 1]: the magnitudes |rfft| + 1e-9 its sums were taken over (a short last window: its first last / 2 + 1
 * entries).  Both are an error before any such call and after avd_release_workspace.  A call of several tracks (option "audio_cut"): nwin and
 * nfull count the windows of all tracks, last is the last track's, the rows are the call's windows track after track; "audio_tracks" int32[tracks][3]
 * and "audio_host" int32[2] are described at avd_audio_features, as are the converter's "audio_rs_plan" int32[8], "audio_rs_taps" int32[U][T],
 * "audio_rs_tracks" int32[tracks][2] and "audio_pcm" int16[output samples] (option "audio_rate").
 * "stream_state" int32[8][2], host state: for each stream slot 1 ... 8 the frames it has absorbed since it was last emptied and the clip position
 * option "stream_map" maps to it (-1: none).
 * "stream_call" int32[4], host state, of the last avd_analyze_* call that brought frames: the clips that continued a FILLED slot, the launches that restored
 * slot frames (0 or 1), the launches that saved them (0 or 1), and the frames in the per-frame buffers, restored frames included; all 0 after a call
 * without frames.  (A call refused or failed keeps the figures of the call before it.)
 * "fb_model" int32[4], host state, of the last call that ran the Farneback stage (at least one pair): the "cv2_model" it ran under, the scales it ran
 * (4, or 3 under bit 8), the "fb_fold_up" mask in effect and "fb_fold_blur" in effect; an error before any such call.
 * Returns the number of bytes copied (>=0) or a negative status. */
int64_t avd_debug_fetch(avd_ctx* ctx, const char* name, void* out, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* AVD_H */
