// Stand-alone driver of csrc/avd_ingest_clip.h for tests/test_ingest_clip_host.py (host C++ only; built with the address and undefined-behaviour
// sanitizers).  Each input line describes one clip and the constructor it goes through:
//   via format mem n h w rotate  plane0 plane1 plane2  row0 row1 row2  frame0 frame1 frame2  struct_size_delta reserved
// via: "direct" (bgr_clip / nv12_clip / i420_clip by format), "public" (an avd_clip through from_public; format is ignored), "picture" (an
// avd_picture through from_picture).  Plane pointers are plain numbers: nothing here ever reads through them.
// Each output line: status|why|format|nspans|span offsets|span bytes|plane offsets|total|copied -- the refusal of from_picture if there is one,
// else check_clip's; the staging plan (clip_stage) only of an accepted clip.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "../ai-video-detector_amd/csrc/avd_ingest_clip.h"

int main()
{
    char via[16];
    int format, mem, n, h, w, rotate, size_delta, reserved;
    unsigned long long plane[3];
    long long row[3], frame[3];
    while (std::scanf("%15s %d %d %d %d %d %d %llu %llu %llu %lld %lld %lld %lld %lld %lld %d %d", via, &format, &mem, &n, &h, &w, &rotate, &plane[0],
                      &plane[1], &plane[2], &row[0], &row[1], &row[2], &frame[0], &frame[1], &frame[2], &size_delta, &reserved) == 18) {
        const uint8_t* p[3];
        for (int i = 0; i < 3; i++) p[i] = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(plane[i]));
        IngestClip k{};
        Refusal r{0, nullptr};
        if (!std::strcmp(via, "direct")) {
            if (format == AVD_FMT_BGR24) k = bgr_clip(p[0], mem, n, h, w, row[0], frame[0]);
            else if (format == AVD_FMT_NV12) k = nv12_clip(p[0], p[1], mem, n, h, w, row[0], row[1], frame[0], frame[1]);
            else k = i420_clip(p[0], p[1], p[2], mem, n, h, w, row[0], row[1], frame[0], frame[1]);
        } else if (!std::strcmp(via, "public")) {
            avd_clip c{};
            c.data = p[0]; c.uv = p[1]; c.mem = mem; c.n = n; c.h = h; c.w = w;
            c.row_stride = row[0]; c.frame_stride = frame[0]; c.uv_row_stride = row[1]; c.uv_frame_stride = frame[1];
            k = from_public(c);
        } else {
            avd_picture pic{};
            pic.struct_size = (uint32_t)((int)sizeof(avd_picture) + size_delta);
            pic.format = format; pic.mem = mem; pic.n = n; pic.h = h; pic.w = w; pic.rotate = rotate; pic.reserved = reserved;
            for (int i = 0; i < 3; i++) { pic.plane[i] = p[i]; pic.row_stride[i] = row[i]; pic.frame_stride[i] = frame[i]; }
            r = from_picture(pic, k);
        }
        if (!r.status) r = check_clip(k);
        ClipStage s{};
        if (!r.status) s = clip_stage(k);
        std::printf("%d|%s|%d|%d|%zu,%zu,%zu|%zu,%zu,%zu|%zu,%zu,%zu|%zu|%zu\n", r.status, r.why ? r.why : "", k.format, s.nspans, s.span[0].off,
                    s.span[1].off, s.span[2].off, s.span[0].bytes, s.span[1].bytes, s.span[2].bytes, s.plane_off[0], s.plane_off[1], s.plane_off[2],
                    s.total, s.copied);
    }
    return 0;
}
