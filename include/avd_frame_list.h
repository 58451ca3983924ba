/*
 * avd_frame_list.h -- clips as lists of separately allocated frames: part of the C-ABI of libavd_hip.so, included by avd.h (include that one;
 * the types used here are declared there).  Additive at ABI 3: avd_picture, avd_clip and every entry point of avd.h are unchanged.
 */
#ifndef AVD_FRAME_LIST_H
#define AVD_FRAME_LIST_H
#ifndef AVD_H
#error "include avd.h: it includes this header"
#endif

/* Clips as LISTS of separately allocated frames (additive at ABI 3; avd_picture and every entry point above are unchanged).  Every descriptor
 * above takes n pictures at one fixed distance in one allocation; no decoder produces that: libavcodec / PyAV hand over one AVFrame per picture,
 * each with its own buffers, rocDecode / VCN surfaces come out of a pool and sit at arbitrary device addresses, torch-based decoders give one
 * tensor per frame.  avd_frame_list is avd_picture with, per plane, an ARRAY of n plane pointers in place of base + f * frame_stride; the ingest
 * kernels take a frame's planes from a table (one scalar load per plane and workgroup) instead of from a stride, the fills are the same.
 *   struct_size  sizeof(avd_frame_list) of the caller's header; anything else is AVD_ERR_ARG
 *   format       exactly as avd_picture.format: the layout in the low byte, AVD_FMT_FULL_RANGE above it
 *   plane        plane[p][f] = plane p of frame f, n entries each.  BGR: [0]; NV12: Y, interleaved UV; I420: Y, U, V; AVD_FMT_RGB24 / _BGRA32 /
 *                _RGBA32: [0]; AVD_FMT_RGBP: R, G, B (a torch uint8[3,H,W] frame: its three channel views; gbrp: data[2], data[0], data[1]);
 *                AVD_FMT_YUYV422 / _UYVY422: [0]; AVD_FMT_I422: Y, U, V; AVD_FMT_NV16: Y, interleaved UV;
 *                AVD_FMT_P010: Y, interleaved UV; AVD_FMT_I010: Y, U, V (16-bit words behind byte pointers, include/avd.h)
 *   row_stride   bytes, per plane, shared by all frames of the list; I420, I422 and I010: [1] == [2], RGBP: [0] == [1] == [2] (AVD_ERR_ARG otherwise)
 *   mem          where the PLANES live;  h, w  the stored picture;  rotate, reserved  as avd_picture
 * Pointer arrays: the arrays plane[p] are always HOST memory, whatever `mem` says.  They are read during the call and never retained: after
 * avd_analyze_frame_lists_async returns the caller may free or overwrite them.  The planes themselves stay alive until avd_synchronize (or the
 * blocking call's return), as for every other entry point.
 * Results: every output of a list equals, bit for bit and in both fb_modes, the output of the format's own strided entry point (or avd_picture
 * call) on the same frames stacked in list order, for every rotation and range.  A frame may appear in the list more than once; frames may lie
 * in any address order.
 * AVD_MEM_HOST: the spans of all (frame, plane) pairs are sorted by address and merged where they overlap or touch; each merged span is ONE copy
 * onto a 256-byte boundary of the staging buffer.  Frames that are views of one stacked array stage as the strided clip does; separately
 * allocated frames are n x planes copies; a frame listed twice crosses the link once; no host byte is copied twice (avd_debug_fetch
 * "stage_bytes", "stage_copies").  Spans separated by a gap, however small, are not merged.  The staged planes then run through the same table
 * as device planes do.  The 16-byte fills need every frame of the list aligned (and w % 16 == 0, aligned row strides); one frame that is not
 * sends the whole list through the scalar fill, with identical results.
 * avd_preprocess_frame_list: outputs as avd_preprocess_bgr.  avd_analyze_frame_lists: the batch of avd_analyze_pictures with lists -- any mix of
 * formats, geometries, rotations and ranges; ONE Farneback launch sequence over all lists; records list after list, identical to one call per
 * list; nlists = 1 is the single-clip call; empty lists (n = 0) are allowed anywhere.  Lists and strided pictures cannot be mixed in one call (a
 * strided clip is trivially a list).  avd_analyze_frame_lists_async follows avd_analyze_pictures_async exactly: one call outstanding per context,
 * drained by any other call, with the same exemptions.
 * Refused before anything is staged or launched, the first of: struct_size; format; AVD_FMT_FULL_RANGE on BGR or an RGB layout; rotate; reserved; BGR or an
 * RGB or 4:2:2 layout with a rotation; I420 / I422 / I010 chroma (RGBP: plane) row strides that differ; then mem; the size range; even size (4:2:0), even width (4:2:2); 32 x 32; a null plane[p] array or a null entry in
 * one while n > 0 (AVD_ERR_ARG); row strides smaller than a row; P010 / I010: an odd plane address or row stride; last, a null records pointer while there are frames.  Statuses as above. */
typedef struct avd_frame_list {
    uint32_t struct_size;            /* sizeof(avd_frame_list); anything else AVD_ERR_ARG */
    int32_t  format;                 /* exactly as avd_picture.format: layout in the low byte, AVD_FMT_FULL_RANGE above it */
    const uint8_t* const* plane[3];  /* plane[p][f] = plane p of frame f, n entries each. BGR: [0]; NV12: Y, UV; I420: Y, U, V */
    int64_t  row_stride[3];          /* bytes, shared by all frames of the list; I420: [1] == [2] */
    int32_t  mem, n, h, w;           /* mem: where the PLANES live; h, w: the stored picture */
    int32_t  rotate, reserved;       /* as avd_picture */
} avd_frame_list;
int avd_preprocess_frame_list(avd_ctx* ctx, const avd_frame_list* list, uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq);
int avd_analyze_frame_lists(avd_ctx* ctx, const avd_frame_list* lists, int nlists, avd_frame_record* records);
int avd_analyze_frame_lists_async(avd_ctx* ctx, const avd_frame_list* lists, int nlists, avd_frame_record* records);

#endif /* AVD_FRAME_LIST_H */
