// avd_ingest_clip.h -- one clip as the ingest host path sees it: what it is, whether it is acceptable, where it lands in the staging buffer.
// Pure host C++ (include/avd.h and the standard library; no HIP type, no avd_ctx), so a stand-alone program can include it
// (tests/ingest_check.cpp).
//
// Everything that depends on the layout is ONE row of kIngestLayouts: a new layout is a new row (and a fill policy, a dispatch branch, a record
// in the binding: DESIGN.md, "adding a layout").  No function below asks "which format is this": it reads the clip's row.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/avd.h"

// ---- the layouts ---------------------------------------------------------------------------------------------------------------------------
enum class LayoutFamily { packed_rgb, planar_rgb, yuv420, yuv422 };      // packed_rgb: BGR24 and the packed layouts of RGB producers

// planes behind plane 0 (the chroma planes of 4:2:0 and 4:2:2, the G and B planes of RGBP): h / sub_ydiv rows of w / sub_xdiv samples.
// The texts are whole literals: what include/avd.h documents can be found here by searching.  They are irregular on purpose (NV12 and the
// one-plane layouts were first and say "the planes" / "the frame"; the range and turn texts say "picture" of a frame list too).
struct IngestLayout {
    int value;
    const char* name;         // AVD_FMT_<name>
    int planes, px_bytes;     // px_bytes: of plane 0
    int sample_bytes;         // 2: 16-bit little-endian words, narrowed to 8 bits as they are loaded; pointers stay byte pointers, strides bytes
    int sub_ydiv, sub_xdiv;
    LayoutFamily family;
    bool even_h, even_w;      // what the subsampling needs even
    int shared_from;          // planes shared_from .. 2 share their strides (3: none do)
    int chroma_align;         // bytes the vector fills read of planes 1 and 2 at a time; plane 0 is always read 16 at a time
    const char *no_range, *no_turn;      // why AVD_FMT_FULL_RANGE / a quarter turn is refused; null: allowed
    const char *shared, *even, *null_plane, *small_strides;
};

// the long texts that several rows share
inline constexpr char kNoRangeRgb[] = "AVD_FMT_FULL_RANGE describes 4:2:0 samples: an RGB picture has no range";
inline constexpr char kNoTurnRgb[] = "a turned RGB picture is not on the path: producers of RGB hand it over already rotated";
inline constexpr char kNoTurn422[] = "a turned 4:2:2 picture is not on the path: the conversion does not commute with quarter turns";
constexpr IngestLayout kIngestLayouts[] = {
    // value, name, planes, px, sample, ydiv, xdiv, family, even h, w, shared, align, no_range, no_turn, shared, even, null, small
    {AVD_FMT_BGR24, "BGR24", 1, 3, 1, 1, 1, LayoutFamily::packed_rgb, false, false, 3, 16,
     "AVD_FMT_FULL_RANGE describes 4:2:0 samples: a BGR picture has no range", "a turned BGR picture is not on the path: cv2 hands BGR over already rotated",
     nullptr, nullptr, "null frame pointer", "strides smaller than the frame"},
    {AVD_FMT_NV12, "NV12", 2, 1, 1, 2, 1, LayoutFamily::yuv420, true, true, 3, 16, nullptr, nullptr,
     nullptr, "NV12 needs even width and height", "null plane pointer", "strides smaller than the planes"},
    {AVD_FMT_I420, "I420", 3, 1, 1, 2, 2, LayoutFamily::yuv420, true, true, 1, 8, nullptr, nullptr,
     "the U and V planes of an I420 picture share their strides", "I420 needs even width and height", "null I420 plane pointer", "strides smaller than the I420 planes"},
    {AVD_FMT_RGB24, "RGB24", 1, 3, 1, 1, 1, LayoutFamily::packed_rgb, false, false, 3, 16, kNoRangeRgb, kNoTurnRgb,
     nullptr, nullptr, "null frame pointer", "strides smaller than the frame"},
    {AVD_FMT_BGRA32, "BGRA32", 1, 4, 1, 1, 1, LayoutFamily::packed_rgb, false, false, 3, 16, kNoRangeRgb, kNoTurnRgb,
     nullptr, nullptr, "null frame pointer", "strides smaller than the frame"},
    {AVD_FMT_RGBA32, "RGBA32", 1, 4, 1, 1, 1, LayoutFamily::packed_rgb, false, false, 3, 16, kNoRangeRgb, kNoTurnRgb,
     nullptr, nullptr, "null frame pointer", "strides smaller than the frame"},
    {AVD_FMT_RGBP, "RGBP", 3, 1, 1, 1, 1, LayoutFamily::planar_rgb, false, false, 0, 16, kNoRangeRgb, kNoTurnRgb,
     "the R, G and B planes of an RGBP picture share their strides", nullptr, "null RGBP plane pointer", "strides smaller than the RGBP planes"},
    {AVD_FMT_YUYV422, "YUYV422", 1, 2, 1, 1, 1, LayoutFamily::yuv422, false, true, 3, 16, nullptr, kNoTurn422,
     nullptr, "YUYV422 needs even width", "null frame pointer", "strides smaller than the frame"},
    {AVD_FMT_UYVY422, "UYVY422", 1, 2, 1, 1, 1, LayoutFamily::yuv422, false, true, 3, 16, nullptr, kNoTurn422,
     nullptr, "UYVY422 needs even width", "null frame pointer", "strides smaller than the frame"},
    {AVD_FMT_I422, "I422", 3, 1, 1, 1, 2, LayoutFamily::yuv422, false, true, 1, 8, nullptr, kNoTurn422,
     "the U and V planes of an I422 picture share their strides", "I422 needs even width", "null I422 plane pointer", "strides smaller than the I422 planes"},
    {AVD_FMT_NV16, "NV16", 2, 1, 1, 1, 1, LayoutFamily::yuv422, false, true, 3, 16, nullptr, kNoTurn422,
     nullptr, "NV16 needs even width", "null NV16 plane pointer", "strides smaller than the NV16 planes"},
    {AVD_FMT_P010, "P010", 2, 2, 2, 2, 1, LayoutFamily::yuv420, true, true, 3, 16, nullptr, nullptr,
     nullptr, "P010 needs even width and height", "null P010 plane pointer", "strides smaller than the P010 planes"},
    {AVD_FMT_I010, "I010", 3, 2, 2, 2, 2, LayoutFamily::yuv420, true, true, 1, 16, nullptr, nullptr,
     "the U and V planes of an I010 picture share their strides", "I010 needs even width and height", "null I010 plane pointer", "strides smaller than the I010 planes"},
};

// the row of a layout value; null: the value is not a layout (what include/avd.h says stays refused)
constexpr const IngestLayout* ingest_layout(int value)
{
    for (const IngestLayout& r : kIngestLayouts)
        if (r.value == value) return &r;
    return nullptr;
}
inline bool known_layout(int layout) { return ingest_layout(layout) != nullptr; }

// ---- the clip ------------------------------------------------------------------------------------------------------------------------------
// format says what the planes are -- nothing downstream looks at which pointers are null to find out:
//   one plane     data = the interleaved frames (row_stride / frame_stride)
//   two planes    data = the Y plane, uv = the interleaved chroma plane (uv_row_stride / uv_frame_stride)
//   three planes  data = Y, uv = the U plane, v = the V plane; the uv strides hold for both (RGBP: R, G, B, and all four strides hold for all)
// rotate: quarter turns clockwise from the stored picture (h, w, the planes and strides: always the STORED one) to the displayed picture, whose
// size the geometry tables, the band plan and every result follow (4:2:0 clips only).
// full_range: AVD_FMT_FULL_RANGE of the descriptor, taken out of `format`, which stays the plain layout.
// list: the frames do not lie at a fixed distance from each other but where a table says -- list[p][f] = plane p of frame f (avd_frame_list;
// p as data, uv, v).  The arrays are the CALLER's host memory, read while the call runs and never kept.  data / uv / v and the frame strides
// of such a clip are unused (null, 0); everything else means what it means for a strided clip.
// A clip is made by make_clip: through bgr_clip / nv12_clip / i420_clip (the entry points that name their format), from_public (avd_clip),
// from_picture (avd_picture) or from_frame_list (avd_frame_list), and by nothing else.
struct IngestClip {
    int format;
    const uint8_t *data, *uv, *v;
    const uint8_t* const* list[3];
    bool is_list;         // from_frame_list made it (the arrays may still be null: check_clip refuses that)
    const IngestLayout& row() const { return *ingest_layout(format); }
    int planes() const { return row().planes; }
    bool is_16bit() const { return row().sample_bytes == 2; }
    bool is_420() const { return row().family == LayoutFamily::yuv420; }
    bool is_422() const { return row().family == LayoutFamily::yuv422; }      // chroma subsampled horizontally only: one chroma row per luma row
    bool is_yuv() const { return is_420() || is_422(); }                      // converted through the yuv2rgb tables; has a range
    bool planar_yuv() const { return is_yuv() && planes() == 3; }             // separate U and V planes of w / 2 samples a row, at shared strides
    bool is_rgb() const { return !is_yuv() && format != AVD_FMT_BGR24; }      // the four layouts of RGB producers
    int px_bytes() const { return row().px_bytes; }
    int sub_rows() const { return h / row().sub_ydiv; }
    int sub_row_bytes() const { return w / row().sub_xdiv * row().sample_bytes; }
    int mem, n, h, w;
    int64_t row_stride, frame_stride, uv_row_stride, uv_frame_stride;
    int rotate;
    int full_range;       // 4:2:0 and 4:2:2 clips: the samples use 0 .. 255 (ffmpeg's J formats), not 16 .. 235 / 240; 0 from every entry point but the descriptors
    int disp_h() const { return rotate & 1 ? w : h; }
    int disp_w() const { return rotate & 1 ? h : w; }
};

// status 0: accepted; otherwise an avd_status and the text avd_last_error reports
struct Refusal { int status; const char* why; };

// The one constructor: the planes the row has, the strides of planes 0 and 1 (whatever lies behind is not looked at)
inline IngestClip make_clip(const IngestLayout& L, const uint8_t* const plane[3], const int64_t row[3], const int64_t frame[3], int mem, int n, int h, int w)
{
    IngestClip k{};
    k.format = L.value;
    k.mem = mem; k.n = n; k.h = h; k.w = w;
    k.data = plane[0]; k.row_stride = row[0]; k.frame_stride = frame[0];
    if (L.planes >= 2) { k.uv = plane[1]; k.uv_row_stride = row[1]; k.uv_frame_stride = frame[1]; }
    if (L.planes == 3) k.v = plane[2];
    return k;
}

// the entry points that name their format: one pair of strides for plane 0, one for whatever lies behind it
inline IngestClip named_clip(int format, const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, int mem, int n, int h, int w, int64_t row0, int64_t row1,
                             int64_t frame0, int64_t frame1)
{
    const uint8_t* const plane[3] = {p0, p1, p2};
    const int64_t row[3] = {row0, row1, row1}, frame[3] = {frame0, frame1, frame1};
    return make_clip(*ingest_layout(format), plane, row, frame, mem, n, h, w);
}
inline IngestClip bgr_clip(const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride, int64_t frame_stride)
{
    return named_clip(AVD_FMT_BGR24, bgr, nullptr, nullptr, mem, n, h, w, row_stride, 0, frame_stride, 0);
}
inline IngestClip nv12_clip(const uint8_t* y, const uint8_t* uv, int mem, int n, int h, int w, int64_t y_row, int64_t uv_row, int64_t y_frame,
                            int64_t uv_frame)
{
    return named_clip(AVD_FMT_NV12, y, uv, nullptr, mem, n, h, w, y_row, uv_row, y_frame, uv_frame);
}
inline IngestClip i420_clip(const uint8_t* y, const uint8_t* u, const uint8_t* v, int mem, int n, int h, int w, int64_t y_row, int64_t c_row,
                            int64_t y_frame, int64_t c_frame)
{
    return named_clip(AVD_FMT_I420, y, u, v, mem, n, h, w, y_row, c_row, y_frame, c_frame);
}

// avd_clip is frozen at ABI 3 and has no format field: a clip with uv set is NV12, any other is BGR.  The ONE place where a format is inferred
// from a pointer.
inline IngestClip from_public(const avd_clip& c)
{
    if (c.uv) return nv12_clip(c.data, c.uv, c.mem, c.n, c.h, c.w, c.row_stride, c.uv_row_stride, c.frame_stride, c.uv_frame_stride);
    return bgr_clip(c.data, c.mem, c.n, c.h, c.w, c.row_stride, c.frame_stride);
}

// ---- the two descriptors -------------------------------------------------------------------------------------------------------------------
// The descriptors spell their format out: the layout in the low byte, AVD_FMT_FULL_RANGE above it.  Refused here: what the descriptor alone can
// get wrong, in the order of the lines below (include/avd.h); the planes, strides and sizes are check_clip's.  `k` is written only on success.
struct DescriptorTexts { const char *size, *format, *rotate, *reserved; };      // the four texts that name the struct

inline Refusal from_descriptor(const DescriptorTexts& t, bool size_ok, int format, int rotate, int reserved, const uint8_t* const plane[3],
                               const int64_t row[3], const int64_t frame[3], int mem, int n, int h, int w, IngestClip& k)
{
    if (!size_ok) return {AVD_ERR_ARG, t.size};
    const IngestLayout* L = ingest_layout(format & 0xFF);
    const int full_range = (format & AVD_FMT_FULL_RANGE) != 0;
    if ((format & ~(0xFF | AVD_FMT_FULL_RANGE)) || !L) return {AVD_ERR_ARG, t.format};
    if (full_range && L->no_range) return {AVD_ERR_ARG, L->no_range};
    if (rotate < 0 || rotate > 3) return {AVD_ERR_ARG, t.rotate};
    if (reserved != 0) return {AVD_ERR_ARG, t.reserved};
    if (rotate && L->no_turn) return {AVD_ERR_UNSUPPORTED, L->no_turn};
    for (int p = L->shared_from; p < 2; p++)
        if (row[p] != row[p + 1] || frame[p] != frame[p + 1]) return {AVD_ERR_ARG, L->shared};
    k = make_clip(*L, plane, row, frame, mem, n, h, w);
    k.rotate = rotate;
    k.full_range = full_range;
    return {0, nullptr};
}

inline Refusal from_picture(const avd_picture& p, IngestClip& k)
{
    static constexpr DescriptorTexts t{"avd_picture.struct_size is not sizeof(avd_picture)", "bad avd_picture.format",
                                       "avd_picture.rotate must be 0 .. 3 quarter turns", "avd_picture.reserved must be 0"};
    return from_descriptor(t, p.struct_size == sizeof(avd_picture), p.format, p.rotate, p.reserved, p.plane, p.row_stride, p.frame_stride, p.mem, p.n, p.h, p.w, k);
}

// avd_frame_list: avd_picture with a table of plane pointers per frame in place of base + f * frame_stride.  A list has no frame strides: zeros
// share whatever must be shared.
inline Refusal from_frame_list(const avd_frame_list& p, IngestClip& k)
{
    static constexpr DescriptorTexts t{"avd_frame_list.struct_size is not sizeof(avd_frame_list)", "bad avd_frame_list.format",
                                       "avd_frame_list.rotate must be 0 .. 3 quarter turns", "avd_frame_list.reserved must be 0"};
    const uint8_t* const none[3] = {nullptr, nullptr, nullptr};
    const int64_t zero[3] = {0, 0, 0};
    const Refusal r = from_descriptor(t, p.struct_size == sizeof(avd_frame_list), p.format, p.rotate, p.reserved, none, p.row_stride, zero, p.mem, p.n, p.h, p.w, k);
    if (r.status) return r;
    k.is_list = true;
    for (int i = 0; i < k.planes(); i++) k.list[i] = p.plane[i];
    return {0, nullptr};
}

// The one argument check of every ingest entry point.  A clip with several faults is refused for the FIRST of, in this order (include/avd.h):
// mem; the size range; even width and height (4:2:0), even width (4:2:2); the 32 x 32 minimum (of the displayed picture: a quarter turn exchanges h and w, which
// this test does not notice); null planes of a clip that has frames -- of a list: a null array, then a null entry of one; strides (a list
// has no frame strides to check: its frames may lie anywhere, in any order, and may repeat); 16-bit layouts last: a plane base (of a list: any
// entry), a row stride or -- where frame strides are looked at: a strided clip of several frames -- a frame stride that is odd.
inline Refusal check_clip(const IngestClip& k)
{
    const IngestLayout& L = k.row();
    const int n = k.n, h = k.h, w = k.w;
    if (k.mem != AVD_MEM_HOST && k.mem != AVD_MEM_DEVICE) return {AVD_ERR_ARG, "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"};
    if (n < 0 || h <= 0 || w <= 0 || h > 16384 || w > 16384) return {AVD_ERR_ARG, "bad frame geometry"};
    if ((L.even_h && (h & 1)) || (L.even_w && (w & 1))) return {AVD_ERR_UNSUPPORTED, L.even};      // 4:2:2: the height may be odd, nothing is subsampled vertically
    if (h < AVD_HASH || w < AVD_HASH) return {AVD_ERR_UNSUPPORTED, "frame smaller than 32x32: INTER_AREA upscaling is not on the path"};
    const uint8_t* const base[3] = {k.data, k.uv, k.v};
    if (k.is_list) {
        if (n > 0) {
            for (int p = 0; p < L.planes; p++)
                if (!k.list[p]) return {AVD_ERR_ARG, "null plane array of a frame list"};
            for (int p = 0; p < L.planes; p++)
                for (int f = 0; f < n; f++)
                    if (!k.list[p][f]) return {AVD_ERR_ARG, "null plane pointer in a frame list"};
        }
    } else
        for (int p = 0; p < L.planes && n > 0; p++)
            if (!base[p]) return {AVD_ERR_ARG, L.null_plane};
    const int64_t row = (int64_t)w * L.px_bytes, crow = k.sub_row_bytes();      // bytes of a row of plane 0 and of the planes behind it
    const bool strided = !k.is_list && n > 1;
    bool small = k.row_stride < row || (strided && k.frame_stride < k.row_stride * (h - 1) + row);
    if (L.planes > 1) small = small || k.uv_row_stride < crow || (strided && k.uv_frame_stride < k.uv_row_stride * (k.sub_rows() - 1) + crow);
    if (small) return {AVD_ERR_ARG, L.small_strides};
    if (L.sample_bytes == 2) {
        bool odd = ((k.row_stride | k.uv_row_stride) & 1) || (strided && ((k.frame_stride | k.uv_frame_stride) & 1));
        for (int p = 0; p < L.planes && n > 0; p++) {
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

// ---- may a clip run the 16-byte fills? ------------------------------------------------------------------------------------------------------
// The ONE rule, for lists and strided clips: w % 16 == 0; plane 0 and its row stride 16-byte aligned; the planes behind it and their row stride
// aligned to the row's chroma_align (8 for the chroma planes of I420 and I422, which the table fills read 8 bytes at a time; 16 for every
// other, RGBP's G and B included).  It must hold at EVERY address a frame's plane can have: addr(p, i), i < count, names them.  A clip that
// fails runs the scalar fill, with the same results.  (w is the stored width: where a quarter turn makes it differ from the displayed one,
// the turned fill is chosen whatever this says.)
template <typename Addr>
inline bool vec_eligible(const IngestClip& c, int count, Addr addr)
{
    const IngestLayout& L = c.row();
    if (c.w % 16 != 0 || c.row_stride % 16 != 0 || (L.planes > 1 && c.uv_row_stride % L.chroma_align != 0)) return false;
    for (int p = 0; p < L.planes; p++)
        for (int i = 0; i < count; i++)
            if (addr(p, i) % (p == 0 ? 16 : L.chroma_align) != 0) return false;
    return true;
}

// a list: every frame of every plane.  tab[p * n + f]: where the kernel will find plane p of frame f (device addresses: the caller's planes, or
// their places in the staging buffer); one frame that fails sends the whole list through the scalar fill.
inline bool list_vec_eligible(const IngestClip& c, const uint8_t* const* tab)
{
    return vec_eligible(c, c.n, [&](int p, int f) { return (uintptr_t)tab[(size_t)p * c.n + f]; });
}

// a strided clip: each plane's base and the base plus its frame stride (the stride is looked at whatever n is)
inline bool strided_vec_eligible(const IngestClip& c, const uint8_t* d_in, const uint8_t* d_uv, const uint8_t* d_v)
{
    const uintptr_t base[3] = {(uintptr_t)d_in, (uintptr_t)d_uv, (uintptr_t)d_v};
    return vec_eligible(c, 2, [&](int p, int i) { return base[p] + (uintptr_t)i * (uintptr_t)(p == 0 ? c.frame_stride : c.uv_frame_stride); });
}
