// fullrange_clip_check.cpp -- what from_picture (csrc/avd_ingest_clip.h) makes of avd_picture.format's range flag, without a GPU and without the
// library.  One line per picture on standard input:
//   format rotate reserved mem
// of an otherwise valid descriptor (2 frames of 64 x 64, tight strides, stand-in plane addresses that are never read through).  One line out:
//   status|why|format|full_range|rotate
// status and why of the first refusal (from_picture, then check_clip), or 0 and an empty text; format, full_range and rotate as the IngestClip
// carries them (zeros for a picture from_picture refused).  Built with the address and undefined-behaviour sanitizers by
// tests/test_fullrange_host.py.
#include <cstdio>
#include "../ai-video-detector_amd/csrc/avd_ingest_clip.h"

int main()
{
    int format, rotate, reserved, mem;
    while (std::scanf("%d %d %d %d", &format, &rotate, &reserved, &mem) == 4) {
        const int h = 64, w = 64, layout = format & 0xFF;
        avd_picture p{};
        p.struct_size = sizeof(avd_picture);
        p.format = format;
        p.mem = mem; p.n = 2; p.h = h; p.w = w;
        p.rotate = rotate; p.reserved = reserved;
        for (int i = 0; i < 3; i++) p.plane[i] = reinterpret_cast<const uint8_t*>((uintptr_t)0x10000000 * (i + 1));
        if (layout == AVD_FMT_BGR24) { p.row_stride[0] = 3 * w; p.frame_stride[0] = 3 * w * h; }
        else {
            const int cw = layout == AVD_FMT_NV12 ? w : w / 2;
            p.row_stride[0] = w; p.frame_stride[0] = w * h;
            p.row_stride[1] = p.row_stride[2] = cw; p.frame_stride[1] = p.frame_stride[2] = cw * (h / 2);
        }
        IngestClip k{};
        Refusal r = from_picture(p, k);
        if (!r.status) r = check_clip(k);
        std::printf("%d|%s|%d|%d|%d\n", r.status, r.why ? r.why : "", k.format, k.full_range, k.rotate);
    }
    return 0;
}
