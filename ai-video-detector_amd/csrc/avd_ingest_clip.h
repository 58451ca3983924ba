// avd_ingest_clip.h -- one clip as the ingest host path sees it: what it is, whether it is acceptable, where it lands in the staging buffer.
// Pure host C++ (include/avd.h and the standard library; no HIP type, no avd_ctx), so a stand-alone program can include it
// (tests/ingest_clip_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/avd.h"

// format says what the planes are -- nothing downstream looks at which pointers are null to find out:
//   AVD_FMT_BGR24  data = the interleaved frames (row_stride / frame_stride)
//   AVD_FMT_NV12   data = the Y plane, uv = the interleaved chroma plane (uv_row_stride / uv_frame_stride)
//   AVD_FMT_I420   data = Y, uv = the U plane, v = the V plane; the uv strides hold for both chroma planes
//   AVD_FMT_RGB24 / _BGRA32 / _RGBA32   data = the interleaved frames, 3 / 4 / 4 bytes per pixel, as BGR24
//   AVD_FMT_RGBP   data = R, uv = the G plane, v = the B plane, each h x w; row_stride == uv_row_stride and frame_stride == uv_frame_stride
//   AVD_FMT_YUYV422 / _UYVY422   data = the packed frames, 2 bytes per pixel (a pixel pair per dword), as BGR24
//   AVD_FMT_I422   as I420, the chroma planes h rows of w / 2 bytes;  AVD_FMT_NV16   as NV12, the chroma plane h rows of w bytes
//   AVD_FMT_P010   as NV12, AVD_FMT_I010 as I420, every sample a little-endian 16-bit word: rows of 2w (Y), 2w (P010 UV) and w (I010 U, V) bytes;
//                  the pointers stay byte pointers and the strides bytes
// rotate: quarter turns clockwise from the stored picture (h, w, the planes and strides: always the STORED one) to the displayed picture, whose
// size the geometry tables, the band plan and every result follow (4:2:0 clips only).
// full_range: AVD_FMT_FULL_RANGE of the descriptor, taken out of `format`, which stays the plain layout.
// list: the frames do not lie at a fixed distance from each other but where a table says -- list[p][f] = plane p of frame f (avd_frame_list;
// p as data, uv, v).  The arrays are the CALLER's host memory, read while the call runs and never kept.  data / uv / v and the frame strides
// of such a clip are unused (null, 0); everything else means what it means for a strided clip.
// A clip is made by bgr_clip / nv12_clip / i420_clip (the entry points that name their format), rgb_clip / yuv422_clip / yuv10_clip (descriptors only), from_public (avd_clip), from_picture
// (avd_picture) or from_frame_list (avd_frame_list), and by nothing else.
struct IngestClip {
    int format;
    const uint8_t *data, *uv, *v;
    const uint8_t* const* list[3];
    bool is_list;         // from_frame_list made it (the arrays may still be null: check_clip refuses that)
    int planes() const
    {
        if (format == AVD_FMT_P010) return 2;
        if (format == AVD_FMT_I010) return 3;
        return format == AVD_FMT_NV12 || format == AVD_FMT_NV16 ? 2 : (format == AVD_FMT_I420 || format == AVD_FMT_RGBP || format == AVD_FMT_I422 ? 3 : 1);
    }
    bool is_16bit() const { return format == AVD_FMT_P010 || format == AVD_FMT_I010; }      // 10-bit 4:2:0: the samples are 16-bit words, narrowed to 8 bits as they are loaded
    bool is_420() const { return format == AVD_FMT_NV12 || format == AVD_FMT_I420 || is_16bit(); }
    bool is_422() const { return format >= AVD_FMT_YUYV422 && format <= AVD_FMT_NV16; }     // chroma subsampled horizontally only: one chroma row per luma row
    bool is_yuv() const { return is_420() || is_422(); }                                     // converted through the yuv2rgb tables; has a range
    bool planar_yuv() const { return format == AVD_FMT_I420 || format == AVD_FMT_I422 || format == AVD_FMT_I010; }     // separate U and V planes of w / 2 samples a row, at shared strides
    bool is_rgb() const { return format >= AVD_FMT_RGB24 && format <= AVD_FMT_RGBP; }      // the four layouts of RGB producers
    int px_bytes() const      // of plane 0
    {
        if (format == AVD_FMT_BGR24 || format == AVD_FMT_RGB24) return 3;
        if (format == AVD_FMT_BGRA32 || format == AVD_FMT_RGBA32) return 4;
        return format == AVD_FMT_YUYV422 || format == AVD_FMT_UYVY422 || is_16bit() ? 2 : 1;
    }
    // planes 1 and 2: the chroma planes of 4:2:0 (h/2 rows) and of 4:2:2 (h rows) -- w bytes interleaved, w/2 planar; twice that in 16-bit
    // words: 2w for P010, w for I010 --, the G and B planes of RGBP (the size of plane 0)
    int sub_rows() const { return is_420() ? h / 2 : h; }
    int sub_row_bytes() const { return (planar_yuv() ? w / 2 : w) * (is_16bit() ? 2 : 1); }
    int mem, n, h, w;
    int64_t row_stride, frame_stride, uv_row_stride, uv_frame_stride;
    int rotate;
    int full_range;       // 4:2:0 and 4:2:2 clips: the samples use 0 .. 255 (ffmpeg's J formats), not 16 .. 235 / 240; 0 from every entry point but from_picture
    int disp_h() const { return rotate & 1 ? w : h; }
    int disp_w() const { return rotate & 1 ? h : w; }
};

// status 0: accepted; otherwise an avd_status and the text avd_last_error reports
struct Refusal { int status; const char* why; };

inline IngestClip bgr_clip(const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride, int64_t frame_stride)
{
    IngestClip k{};
    k.format = AVD_FMT_BGR24;
    k.data = bgr; k.mem = mem; k.n = n; k.h = h; k.w = w;
    k.row_stride = row_stride; k.frame_stride = frame_stride;
    return k;
}

inline IngestClip nv12_clip(const uint8_t* y, const uint8_t* uv, int mem, int n, int h, int w, int64_t y_row, int64_t uv_row, int64_t y_frame,
                            int64_t uv_frame)
{
    IngestClip k = bgr_clip(y, mem, n, h, w, y_row, y_frame);
    k.format = AVD_FMT_NV12;
    k.uv = uv; k.uv_row_stride = uv_row; k.uv_frame_stride = uv_frame;
    return k;
}

inline IngestClip i420_clip(const uint8_t* y, const uint8_t* u, const uint8_t* v, int mem, int n, int h, int w, int64_t y_row, int64_t c_row,
                            int64_t y_frame, int64_t c_frame)
{
    IngestClip k = nv12_clip(y, u, mem, n, h, w, y_row, c_row, y_frame, c_frame);
    k.format = AVD_FMT_I420;
    k.v = v;
    return k;
}

// the four 4:2:2 layouts: packed (c1, c2 null), NV16 (c1 = the interleaved chroma plane) or I422 (c1 = U, c2 = V at shared strides)
inline IngestClip yuv422_clip(int format, const uint8_t* y, const uint8_t* c1, const uint8_t* c2, int mem, int n, int h, int w, int64_t y_row, int64_t c_row,
                              int64_t y_frame, int64_t c_frame)
{
    IngestClip k = bgr_clip(y, mem, n, h, w, y_row, y_frame);
    k.format = format;
    if (format == AVD_FMT_I422 || format == AVD_FMT_NV16) { k.uv = c1; k.uv_row_stride = c_row; k.uv_frame_stride = c_frame; }
    if (format == AVD_FMT_I422) k.v = c2;
    return k;
}

// the two 10-bit 4:2:0 layouts in 16-bit words: P010 (c1 = the interleaved chroma plane) or I010 (c1 = U, c2 = V at shared strides); strides in bytes
inline IngestClip yuv10_clip(int format, const uint8_t* y, const uint8_t* c1, const uint8_t* c2, int mem, int n, int h, int w, int64_t y_row, int64_t c_row,
                             int64_t y_frame, int64_t c_frame)
{
    IngestClip k = nv12_clip(y, c1, mem, n, h, w, y_row, c_row, y_frame, c_frame);
    k.format = format;
    if (format == AVD_FMT_I010) k.v = c2;
    return k;
}

// the four layouts of RGB producers: packed (g, b null) or planar (AVD_FMT_RGBP: r, g, b share row / frame)
inline IngestClip rgb_clip(int format, const uint8_t* r, const uint8_t* g, const uint8_t* b, int mem, int n, int h, int w, int64_t row, int64_t frame)
{
    IngestClip k = bgr_clip(r, mem, n, h, w, row, frame);
    k.format = format;
    if (format == AVD_FMT_RGBP) { k.uv = g; k.v = b; k.uv_row_stride = row; k.uv_frame_stride = frame; }
    return k;
}

inline bool known_layout(int layout)
{
    return layout == AVD_FMT_BGR24 || layout == AVD_FMT_NV12 || layout == AVD_FMT_I420 || (layout >= AVD_FMT_RGB24 && layout <= AVD_FMT_RGBP) ||
           (layout >= AVD_FMT_YUYV422 && layout <= AVD_FMT_NV16) || layout == AVD_FMT_P010 || layout == AVD_FMT_I010;
}

// avd_clip is frozen at ABI 3 and has no format field: a clip with uv set is NV12, any other is BGR.  The ONE place where a format is inferred
// from a pointer.
inline IngestClip from_public(const avd_clip& c)
{
    if (c.uv) return nv12_clip(c.data, c.uv, c.mem, c.n, c.h, c.w, c.row_stride, c.uv_row_stride, c.frame_stride, c.uv_frame_stride);
    return bgr_clip(c.data, c.mem, c.n, c.h, c.w, c.row_stride, c.frame_stride);
}

// avd_picture spells its format out: the layout in the low byte, AVD_FMT_FULL_RANGE above it.  Refused here: what the descriptor alone can get
// wrong, in the order of the lines below; the planes, strides and sizes are check_clip's.
inline Refusal from_picture(const avd_picture& p, IngestClip& k)
{
    if (p.struct_size != sizeof(avd_picture)) return {AVD_ERR_ARG, "avd_picture.struct_size is not sizeof(avd_picture)"};
    const int layout = p.format & 0xFF, full_range = (p.format & AVD_FMT_FULL_RANGE) != 0;
    if ((p.format & ~(0xFF | AVD_FMT_FULL_RANGE)) || !known_layout(layout))
        return {AVD_ERR_ARG, "bad avd_picture.format"};
    const bool rgb = layout >= AVD_FMT_RGB24 && layout <= AVD_FMT_RGBP, yuv422 = layout >= AVD_FMT_YUYV422 && layout <= AVD_FMT_NV16;
    if (full_range && layout == AVD_FMT_BGR24) return {AVD_ERR_ARG, "AVD_FMT_FULL_RANGE describes 4:2:0 samples: a BGR picture has no range"};
    if (full_range && rgb) return {AVD_ERR_ARG, "AVD_FMT_FULL_RANGE describes 4:2:0 samples: an RGB picture has no range"};
    if (p.rotate < 0 || p.rotate > 3) return {AVD_ERR_ARG, "avd_picture.rotate must be 0 .. 3 quarter turns"};
    if (p.reserved != 0) return {AVD_ERR_ARG, "avd_picture.reserved must be 0"};
    if (layout == AVD_FMT_BGR24) {
        if (p.rotate) return {AVD_ERR_UNSUPPORTED, "a turned BGR picture is not on the path: cv2 hands BGR over already rotated"};
        k = bgr_clip(p.plane[0], p.mem, p.n, p.h, p.w, p.row_stride[0], p.frame_stride[0]);
    } else if (rgb) {
        if (p.rotate) return {AVD_ERR_UNSUPPORTED, "a turned RGB picture is not on the path: producers of RGB hand it over already rotated"};
        if (layout == AVD_FMT_RGBP && (p.row_stride[0] != p.row_stride[1] || p.row_stride[1] != p.row_stride[2] || p.frame_stride[0] != p.frame_stride[1] ||
                                       p.frame_stride[1] != p.frame_stride[2]))
            return {AVD_ERR_ARG, "the R, G and B planes of an RGBP picture share their strides"};
        k = rgb_clip(layout, p.plane[0], p.plane[1], p.plane[2], p.mem, p.n, p.h, p.w, p.row_stride[0], p.frame_stride[0]);
    } else if (yuv422) {
        if (p.rotate) return {AVD_ERR_UNSUPPORTED, "a turned 4:2:2 picture is not on the path: the conversion does not commute with quarter turns"};
        if (layout == AVD_FMT_I422 && (p.row_stride[1] != p.row_stride[2] || p.frame_stride[1] != p.frame_stride[2]))
            return {AVD_ERR_ARG, "the U and V planes of an I422 picture share their strides"};
        k = yuv422_clip(layout, p.plane[0], p.plane[1], p.plane[2], p.mem, p.n, p.h, p.w, p.row_stride[0], p.row_stride[1], p.frame_stride[0], p.frame_stride[1]);
    } else if (layout == AVD_FMT_NV12) {
        k = nv12_clip(p.plane[0], p.plane[1], p.mem, p.n, p.h, p.w, p.row_stride[0], p.row_stride[1], p.frame_stride[0], p.frame_stride[1]);
    } else if (layout == AVD_FMT_P010 || layout == AVD_FMT_I010) {
        if (layout == AVD_FMT_I010 && (p.row_stride[1] != p.row_stride[2] || p.frame_stride[1] != p.frame_stride[2]))
            return {AVD_ERR_ARG, "the U and V planes of an I010 picture share their strides"};
        k = yuv10_clip(layout, p.plane[0], p.plane[1], p.plane[2], p.mem, p.n, p.h, p.w, p.row_stride[0], p.row_stride[1], p.frame_stride[0], p.frame_stride[1]);
    } else {
        if (p.row_stride[1] != p.row_stride[2] || p.frame_stride[1] != p.frame_stride[2])
            return {AVD_ERR_ARG, "the U and V planes of an I420 picture share their strides"};
        k = i420_clip(p.plane[0], p.plane[1], p.plane[2], p.mem, p.n, p.h, p.w, p.row_stride[0], p.row_stride[1], p.frame_stride[0], p.frame_stride[1]);
    }
    k.rotate = p.rotate;
    k.full_range = full_range;
    return {0, nullptr};
}

// avd_frame_list: avd_picture with a table of plane pointers per frame in place of base + f * frame_stride.  The same refusals in the same order.
inline Refusal from_frame_list(const avd_frame_list& p, IngestClip& k)
{
    if (p.struct_size != sizeof(avd_frame_list)) return {AVD_ERR_ARG, "avd_frame_list.struct_size is not sizeof(avd_frame_list)"};
    const int layout = p.format & 0xFF, full_range = (p.format & AVD_FMT_FULL_RANGE) != 0;
    if ((p.format & ~(0xFF | AVD_FMT_FULL_RANGE)) || !known_layout(layout))
        return {AVD_ERR_ARG, "bad avd_frame_list.format"};
    const bool rgb = layout >= AVD_FMT_RGB24 && layout <= AVD_FMT_RGBP, yuv422 = layout >= AVD_FMT_YUYV422 && layout <= AVD_FMT_NV16;
    if (full_range && layout == AVD_FMT_BGR24) return {AVD_ERR_ARG, "AVD_FMT_FULL_RANGE describes 4:2:0 samples: a BGR picture has no range"};
    if (full_range && rgb) return {AVD_ERR_ARG, "AVD_FMT_FULL_RANGE describes 4:2:0 samples: an RGB picture has no range"};
    if (p.rotate < 0 || p.rotate > 3) return {AVD_ERR_ARG, "avd_frame_list.rotate must be 0 .. 3 quarter turns"};
    if (p.reserved != 0) return {AVD_ERR_ARG, "avd_frame_list.reserved must be 0"};
    if (layout == AVD_FMT_BGR24) {
        if (p.rotate) return {AVD_ERR_UNSUPPORTED, "a turned BGR picture is not on the path: cv2 hands BGR over already rotated"};
        k = bgr_clip(nullptr, p.mem, p.n, p.h, p.w, p.row_stride[0], 0);
    } else if (rgb) {
        if (p.rotate) return {AVD_ERR_UNSUPPORTED, "a turned RGB picture is not on the path: producers of RGB hand it over already rotated"};
        if (layout == AVD_FMT_RGBP && (p.row_stride[0] != p.row_stride[1] || p.row_stride[1] != p.row_stride[2]))
            return {AVD_ERR_ARG, "the R, G and B planes of an RGBP picture share their strides"};
        k = rgb_clip(layout, nullptr, nullptr, nullptr, p.mem, p.n, p.h, p.w, p.row_stride[0], 0);
    } else if (yuv422) {
        if (p.rotate) return {AVD_ERR_UNSUPPORTED, "a turned 4:2:2 picture is not on the path: the conversion does not commute with quarter turns"};
        if (layout == AVD_FMT_I422 && p.row_stride[1] != p.row_stride[2]) return {AVD_ERR_ARG, "the U and V planes of an I422 picture share their strides"};
        k = yuv422_clip(layout, nullptr, nullptr, nullptr, p.mem, p.n, p.h, p.w, p.row_stride[0], p.row_stride[1], 0, 0);
    } else if (layout == AVD_FMT_NV12) {
        k = nv12_clip(nullptr, nullptr, p.mem, p.n, p.h, p.w, p.row_stride[0], p.row_stride[1], 0, 0);
    } else if (layout == AVD_FMT_P010 || layout == AVD_FMT_I010) {
        if (layout == AVD_FMT_I010 && p.row_stride[1] != p.row_stride[2]) return {AVD_ERR_ARG, "the U and V planes of an I010 picture share their strides"};
        k = yuv10_clip(layout, nullptr, nullptr, nullptr, p.mem, p.n, p.h, p.w, p.row_stride[0], p.row_stride[1], 0, 0);
    } else {
        if (p.row_stride[1] != p.row_stride[2]) return {AVD_ERR_ARG, "the U and V planes of an I420 picture share their strides"};
        k = i420_clip(nullptr, nullptr, nullptr, p.mem, p.n, p.h, p.w, p.row_stride[0], p.row_stride[1], 0, 0);
    }
    k.is_list = true;
    for (int i = 0; i < k.planes(); i++) k.list[i] = p.plane[i];
    k.rotate = p.rotate;
    k.full_range = full_range;
    return {0, nullptr};
}

// The one argument check of every ingest entry point.  A clip with several faults is refused for the FIRST of, in this order (include/avd.h):
// mem; the size range; even width and height (4:2:0), even width (4:2:2); the 32 x 32 minimum (of the displayed picture: a quarter turn exchanges h and w, which
// this test does not notice); null planes of a clip that has frames -- of a list: a null array, then a null entry of one; strides (a list
// has no frame strides to check: its frames may lie anywhere, in any order, and may repeat); 16-bit layouts last: a plane base (of a list: any
// entry), a row stride or -- where frame strides are looked at: a strided clip of several frames -- a frame stride that is odd.
inline Refusal check_clip(const IngestClip& k)
{
    // bgr: ONE packed plane (BGR24 and the packed RGB layouts: their refusals read alike); planar: I420; rgbp: three full-size planes
    // (the packed 4:2:2 layouts are one plane too; I422 and NV16 have texts of their own)
    const bool bgr = k.planes() == 1, planar = k.format == AVD_FMT_I420, rgbp = k.format == AVD_FMT_RGBP;
    const bool i422 = k.format == AVD_FMT_I422, nv16 = k.format == AVD_FMT_NV16, p010 = k.format == AVD_FMT_P010, i010 = k.format == AVD_FMT_I010;
    const int n = k.n, h = k.h, w = k.w;
    if (k.mem != AVD_MEM_HOST && k.mem != AVD_MEM_DEVICE) return {AVD_ERR_ARG, "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"};
    if (n < 0 || h <= 0 || w <= 0 || h > 16384 || w > 16384) return {AVD_ERR_ARG, "bad frame geometry"};
    if (k.is_420() && ((h | w) & 1))
        return {AVD_ERR_UNSUPPORTED, planar ? "I420 needs even width and height"
                                            : (p010 ? "P010 needs even width and height" : (i010 ? "I010 needs even width and height" : "NV12 needs even width and height"))};
    if (k.is_422() && (w & 1))      // the height may be odd: nothing is subsampled vertically
        return {AVD_ERR_UNSUPPORTED, i422 ? "I422 needs even width" : (nv16 ? "NV16 needs even width" : (k.format == AVD_FMT_YUYV422 ? "YUYV422 needs even width" : "UYVY422 needs even width"))};
    if (h < AVD_HASH || w < AVD_HASH) return {AVD_ERR_UNSUPPORTED, "frame smaller than 32x32: INTER_AREA upscaling is not on the path"};
    if (k.is_list) {
        if (n > 0) {
            for (int p = 0; p < k.planes(); p++)
                if (!k.list[p]) return {AVD_ERR_ARG, "null plane array of a frame list"};
            for (int p = 0; p < k.planes(); p++)
                for (int f = 0; f < n; f++)
                    if (!k.list[p][f]) return {AVD_ERR_ARG, "null plane pointer in a frame list"};
        }
    } else if (n > 0 && (!k.data || (!bgr && !k.uv) || (k.planes() == 3 && !k.v)))
        return {AVD_ERR_ARG, bgr ? "null frame pointer"
                                 : (planar ? "null I420 plane pointer"
                                           : (rgbp ? "null RGBP plane pointer" : (i422 ? "null I422 plane pointer" : (nv16 ? "null NV16 plane pointer" : (p010 ? "null P010 plane pointer" : (i010 ? "null I010 plane pointer" : "null plane pointer"))))))};
    const int64_t row = (int64_t)w * k.px_bytes(), crow = k.sub_row_bytes();      // bytes of a row of plane 0 and of the planes behind it
    const bool strided = !k.is_list && n > 1;
    bool small = k.row_stride < row || (strided && k.frame_stride < k.row_stride * (h - 1) + row);
    if (!bgr) small = small || k.uv_row_stride < crow || (strided && k.uv_frame_stride < k.uv_row_stride * (k.sub_rows() - 1) + crow);
    if (small)
        return {AVD_ERR_ARG, bgr ? "strides smaller than the frame"
                                 : (planar ? "strides smaller than the I420 planes"
                                           : (rgbp ? "strides smaller than the RGBP planes"
                                                   : (i422 ? "strides smaller than the I422 planes"
                                                           : (nv16 ? "strides smaller than the NV16 planes"
                                                                   : (p010 ? "strides smaller than the P010 planes"
                                                                           : (i010 ? "strides smaller than the I010 planes" : "strides smaller than the planes"))))))};
    if (k.is_16bit()) {
        bool odd = ((k.row_stride | k.uv_row_stride) & 1) || (strided && ((k.frame_stride | k.uv_frame_stride) & 1));
        const uint8_t* const base[3] = {k.data, k.uv, k.v};
        for (int p = 0; p < k.planes() && n > 0; p++) {
            if (!k.is_list) odd = odd || ((uintptr_t)base[p] & 1);
            else
                for (int f = 0; f < n; f++) odd = odd || ((uintptr_t)k.list[p][f] & 1);
        }
        if (odd) return {AVD_ERR_ARG, "16-bit samples need 2-byte aligned planes and strides"};
    }
    return {0, nullptr};
}

// ---- staging plan of a HOST clip --------------------------------------------------------------------------------------------------------
// bytes spanned by n frames of `rows` rows of `row_bytes` bytes each, with the given strides
inline size_t plane_span(int64_t frame_stride, int n, int64_t row_stride, int rows, size_t row_bytes)
{
    return (size_t)frame_stride * (n - 1) + (size_t)row_stride * (rows - 1) + row_bytes;
}

inline size_t round256(size_t v) { return (v + 255) / 256 * 256; }

// Where a HOST clip lands in the staging buffer: BGR, the packed RGB layouts and packed 4:2:2 as one span; RGBP, I422 and I010 as I420 (a dense [N,3,H,W] stack,
// a y4m map, a dense yuv420p10le frame stack are one span); NV12, NV16 and P010 as the Y span with the chroma span on the next 256-byte boundary
// behind it.  The three planes of I420 usually come out of ONE buffer per clip (a y4m map, a rawvideo pipe: Y, U, V of a frame adjacent), where
// the per-plane spans overlap almost entirely: spans that overlap or touch are merged and copied once, so no host byte crosses the link twice, and
// a plane sits at its own offset inside the merged span; separately allocated planes stay three spans.  `total` (a multiple of 256) is what
// the clip occupies, `copied` the bytes that cross the link; a device clip is used in place and occupies nothing.
struct StageSpan { const uint8_t* src; size_t bytes, off; };       // off: from the clip's place in the staging buffer, a multiple of 256
struct ClipStage { StageSpan span[3]; int nspans; size_t plane_off[3], total, copied; };      // plane_off: data, uv, v

inline ClipStage clip_stage(const IngestClip& c)
{
    ClipStage s{};
    if (c.mem != AVD_MEM_HOST || c.n <= 0 || c.is_list) return s;      // a list has its own plan: list_stage
    const int planes = c.planes();
    const bool bgr = planes == 1, planar = planes == 3;      // planar: I420, I422 and RGBP, whose three planes usually come out of one buffer
    const uint8_t* src[3] = {c.data, c.uv, c.v};
    size_t len[3] = {plane_span(c.frame_stride, c.n, c.row_stride, c.h, (size_t)c.w * c.px_bytes()), 0, 0};
    if (!bgr) len[1] = len[2] = plane_span(c.uv_frame_stride, c.n, c.uv_row_stride, c.sub_rows(), (size_t)c.sub_row_bytes());
    int order[3] = {0, 1, 2};
    if (planar) std::sort(order, order + 3, [&](int a, int b) { return (uintptr_t)src[a] < (uintptr_t)src[b]; });
    for (int i = 0; i < planes; i++) {
        const int p = order[i];
        StageSpan* last = s.nspans ? &s.span[s.nspans - 1] : nullptr;
        if (planar && last && (uintptr_t)src[p] <= (uintptr_t)last->src + last->bytes)
            last->bytes = std::max(last->bytes, (size_t)(src[p] - last->src) + len[p]);
        else {
            s.span[s.nspans] = StageSpan{src[p], len[p], last ? round256(last->off + last->bytes) : 0};
            last = &s.span[s.nspans++];
        }
        s.plane_off[p] = last->off + (size_t)(src[p] - last->src);
    }
    for (int i = 0; i < s.nspans; i++) s.copied += s.span[i].bytes;
    s.total = round256(s.span[s.nspans - 1].off + s.span[s.nspans - 1].bytes);
    return s;
}

// ---- a list of frames (IngestClip::is_list) ----------------------------------------------------------------------------------------------
// The rule of clip_stage for any number of planes: the spans of all (frame, plane) pairs, in address order, merged where they overlap or touch;
// every merged span on a 256-byte boundary, every plane at its own offset inside its span.  Frames that are views of one stacked array stage as
// the strided clip does (the same bytes, ONE copy where the stack is dense); separately allocated frames are n x planes copies; a frame that
// is listed twice crosses the link once; no host byte is copied twice.  Spans that a gap separates are not merged, however small the gap.
// plane_off[p * n + f]: where plane p of frame f lands.  Only the pointer VALUES are used: nothing is read through them.
struct ListStage { std::vector<StageSpan> span; std::vector<size_t> plane_off; size_t total = 0, copied = 0; };

// bytes of plane p of one frame, first to last
inline size_t list_plane_bytes(const IngestClip& c, int p)
{
    if (p == 0) return plane_span(0, 1, c.row_stride, c.h, (size_t)c.w * c.px_bytes());
    return plane_span(0, 1, c.uv_row_stride, c.sub_rows(), (size_t)c.sub_row_bytes());
}

inline ListStage list_stage(const IngestClip& c)
{
    ListStage s;
    if (!c.is_list || c.mem != AVD_MEM_HOST || c.n <= 0) return s;
    const int planes = c.planes(), n = c.n;
    struct Item { const uint8_t* src; size_t bytes; int slot; };
    std::vector<Item> items;
    items.reserve((size_t)planes * n);
    for (int p = 0; p < planes; p++)
        for (int f = 0; f < n; f++) items.push_back(Item{c.list[p][f], list_plane_bytes(c, p), p * n + f});
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return (uintptr_t)a.src < (uintptr_t)b.src; });
    s.plane_off.resize(items.size());
    for (const Item& it : items) {
        StageSpan* last = s.span.empty() ? nullptr : &s.span.back();
        if (last && (uintptr_t)it.src <= (uintptr_t)last->src + last->bytes)
            last->bytes = std::max(last->bytes, (size_t)((uintptr_t)it.src - (uintptr_t)last->src) + it.bytes);
        else {
            s.span.push_back(StageSpan{it.src, it.bytes, last ? round256(last->off + last->bytes) : 0});
            last = &s.span.back();
        }
        s.plane_off[it.slot] = last->off + (size_t)((uintptr_t)it.src - (uintptr_t)last->src);
    }
    for (const StageSpan& sp : s.span) s.copied += sp.bytes;
    s.total = round256(s.span.back().off + s.span.back().bytes);
    return s;
}

// May a list run the vector fills?  Their rule (launch_preprocess: w % 16 == 0, 16-byte aligned planes and row strides, 8 bytes for the
// chroma planes of I420 and I422; 16 for every plane of RGBP, of P010 and I010 and for the packed RGB layouts) must hold for EVERY frame; one frame that fails sends the whole list through the scalar fill, with the same results.
// tab[p * n + f]: where the kernel will find plane p of frame f (device addresses: the caller's planes, or their places in the staging buffer).
inline bool list_vec_eligible(const IngestClip& c, const uint8_t* const* tab)
{
    const bool bgr = c.planes() == 1;
    const int ca = c.planar_yuv() && !c.is_16bit() ? 8 : 16;
    if (c.w % 16 != 0 || c.row_stride % 16 != 0 || (!bgr && c.uv_row_stride % ca != 0)) return false;
    for (int p = 0; p < c.planes(); p++)
        for (int f = 0; f < c.n; f++)
            if ((uintptr_t)tab[(size_t)p * c.n + f] % (p == 0 ? 16 : ca) != 0) return false;
    return true;
}
