// framelist_check.cpp -- the frame-list part of csrc/avd_ingest_clip.h as a stand-alone host program (tests/test_framelist_host.py builds it with
// the address and undefined-behaviour sanitizers and runs it as its own process).  One line of standard input per case, integers separated by blanks:
//   A                                                     -> sizeof(avd_frame_list)|sizeof(avd_picture)|offsets of format, plane, row_stride, mem, n, h, w, rotate, reserved
//   L format mem n h w rotate reserved size_delta rs0 rs1 rs2 null_arrays  a[0][0..m) a[1][0..m) a[2][0..m)      m = max(n, 0)
//        a frame list through from_frame_list and check_clip; null_arrays: bit p set = plane[p] is a null ARRAY; a[p][f] the plane pointers
//        (made-up addresses: the header never reads through them)
//     -> status|why|nspans|span offsets|span bytes|plane offsets (p * n + f)|total|copied|eligible as given|eligible as staged
//        (the last two: list_vec_eligible with the addresses themselves, a device list, and with 256-aligned base + plane offset, a staged one)
//   S format n h w p0 p1 p2 rs0 rs1 rs2 fs0 fs1 fs2       -> nspans|total|copied of the STRIDED host clip (from_picture, clip_stage)
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include "../ai-video-detector_amd/csrc/avd_ingest_clip.h"

template <typename T>
static std::string join(const std::vector<T>& v)
{
    std::string s;
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

int main()
{
    char buf[1 << 16];
    while (std::fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "A") {
            std::printf("%zu|%zu|%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu\n", sizeof(avd_frame_list), sizeof(avd_picture), offsetof(avd_frame_list, format),
                        offsetof(avd_frame_list, plane), offsetof(avd_frame_list, row_stride), offsetof(avd_frame_list, mem), offsetof(avd_frame_list, n),
                        offsetof(avd_frame_list, h), offsetof(avd_frame_list, w), offsetof(avd_frame_list, rotate), offsetof(avd_frame_list, reserved));
        } else if (kind == "S") {
            avd_picture p{};
            long long a[3], rs[3], fs[3];
            in >> p.format >> p.n >> p.h >> p.w >> a[0] >> a[1] >> a[2] >> rs[0] >> rs[1] >> rs[2] >> fs[0] >> fs[1] >> fs[2];
            p.struct_size = sizeof p;
            p.mem = AVD_MEM_HOST;
            for (int i = 0; i < 3; i++) { p.plane[i] = reinterpret_cast<const uint8_t*>((uintptr_t)a[i]); p.row_stride[i] = rs[i]; p.frame_stride[i] = fs[i]; }
            IngestClip k{};
            Refusal r = from_picture(p, k);
            if (!r.status) r = check_clip(k);
            if (r.status) { std::printf("refused: %s\n", r.why); continue; }
            const ClipStage s = clip_stage(k);
            std::printf("%d|%zu|%zu\n", s.nspans, s.total, s.copied);
        } else if (kind == "L") {
            avd_frame_list l{};
            long long size_delta, rs[3];
            int null_arrays;
            in >> l.format >> l.mem >> l.n >> l.h >> l.w >> l.rotate >> l.reserved >> size_delta >> rs[0] >> rs[1] >> rs[2] >> null_arrays;
            l.struct_size = (uint32_t)(sizeof l + size_delta);
            const int m = l.n > 0 ? l.n : 0;
            std::vector<const uint8_t*> arr[3];
            for (int p = 0; p < 3; p++) {
                l.row_stride[p] = rs[p];
                arr[p].resize((size_t)m);
                for (int f = 0; f < m; f++) {
                    long long a = 0;
                    in >> a;
                    arr[p][f] = reinterpret_cast<const uint8_t*>((uintptr_t)a);
                }
                l.plane[p] = (null_arrays >> p) & 1 ? nullptr : arr[p].data();
            }
            IngestClip k{};
            Refusal r = from_frame_list(l, k);
            if (!r.status) r = check_clip(k);
            ListStage s;
            int as_given = 0, as_staged = 0;
            if (!r.status && k.n > 0) {
                s = list_stage(k);
                std::vector<const uint8_t*> tab;
                for (int p = 0; p < k.planes(); p++) tab.insert(tab.end(), arr[p].begin(), arr[p].end());
                as_given = list_vec_eligible(k, tab.data());
                if (k.mem == AVD_MEM_HOST) {
                    for (size_t i = 0; i < tab.size(); i++) tab[i] = reinterpret_cast<const uint8_t*>((uintptr_t)0x7f0000000000ull + s.plane_off[i]);
                    as_staged = list_vec_eligible(k, tab.data());
                }
            }
            std::vector<size_t> off, bytes;
            for (const StageSpan& sp : s.span) { off.push_back(sp.off); bytes.push_back(sp.bytes); }
            std::printf("%d|%s|%zu|%s|%s|%s|%zu|%zu|%d|%d\n", r.status, r.why ? r.why : "", s.span.size(), join(off).c_str(), join(bytes).c_str(),
                        join(s.plane_off).c_str(), s.total, s.copied, as_given, as_staged);
        } else {
            std::fprintf(stderr, "unknown case kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
