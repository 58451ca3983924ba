// yuv10_clip_check.cpp -- the 10-bit 4:2:0 layouts in 16-bit words (AVD_FMT_P010 / _I010) in csrc/avd_ingest_clip.h as a stand-alone host program
// (tests/test_yuv10_host.py builds it with the address and undefined-behaviour sanitizers and runs it as its own process).  One line of standard
// input per case, integers separated by blanks; addresses are made up: the header never reads through them.  The protocol of
// tests/yuv422_clip_check.cpp: the chroma geometry (sub_rows x sub_row_bytes, in BYTES) and the range in every answer.
//   A    -> sizeof(avd_picture)|sizeof(avd_frame_list)|AVD_FMT_P010,AVD_FMT_I010
//   P format mem n h w rotate reserved p0 p1 p2 rs0 rs1 rs2 fs0 fs1 fs2
//        a picture through from_picture and check_clip, then clip_stage
//     -> status|why|format|planes|px_bytes|nspans|span offsets|span bytes|plane offsets|total|copied|sub_rows|sub_row_bytes|full_range
//   L format mem n h w rotate reserved rs0 rs1 rs2 null_arrays  a[0][0..m) a[1][0..m) a[2][0..m)      m = max(n, 0)
//        a frame list through from_frame_list and check_clip, then list_stage and list_vec_eligible
//     -> status|why|format|planes|px_bytes|nspans|span offsets|span bytes|plane offsets (p * n + f)|total|copied|eligible as given|eligible as staged|
//        sub_rows|sub_row_bytes|full_range
#include <cstdio>
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

static const uint8_t* addr(long long a) { return reinterpret_cast<const uint8_t*>((uintptr_t)a); }

int main()
{
    char buf[1 << 16];
    while (std::fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "A") {
            std::printf("%zu|%zu|%d,%d\n", sizeof(avd_picture), sizeof(avd_frame_list), AVD_FMT_P010, AVD_FMT_I010);
        } else if (kind == "P") {
            avd_picture p{};
            long long a[3], rs[3], fs[3];
            in >> p.format >> p.mem >> p.n >> p.h >> p.w >> p.rotate >> p.reserved >> a[0] >> a[1] >> a[2] >> rs[0] >> rs[1] >> rs[2] >> fs[0] >> fs[1] >> fs[2];
            p.struct_size = sizeof p;
            for (int i = 0; i < 3; i++) { p.plane[i] = addr(a[i]); p.row_stride[i] = rs[i]; p.frame_stride[i] = fs[i]; }
            IngestClip k{};
            Refusal r = from_picture(p, k);
            if (!r.status) r = check_clip(k);
            ClipStage s{};
            if (!r.status) s = clip_stage(k);
            std::vector<size_t> off, bytes, poff;
            for (int i = 0; i < s.nspans; i++) { off.push_back(s.span[i].off); bytes.push_back(s.span[i].bytes); }
            if (s.nspans) poff.assign(s.plane_off, s.plane_off + k.planes());
            std::printf("%d|%s|%d|%d|%d|%d|%s|%s|%s|%zu|%zu|%d|%d|%d\n", r.status, r.why ? r.why : "", k.format, r.status ? 0 : k.planes(), r.status ? 0 : k.px_bytes(),
                        s.nspans, join(off).c_str(), join(bytes).c_str(), join(poff).c_str(), s.total, s.copied, r.status ? 0 : k.sub_rows(),
                        r.status ? 0 : k.sub_row_bytes(), r.status ? 0 : k.full_range);
        } else if (kind == "L") {
            avd_frame_list l{};
            long long rs[3];
            int null_arrays;
            in >> l.format >> l.mem >> l.n >> l.h >> l.w >> l.rotate >> l.reserved >> rs[0] >> rs[1] >> rs[2] >> null_arrays;
            l.struct_size = sizeof l;
            const int m = l.n > 0 ? l.n : 0;
            std::vector<const uint8_t*> arr[3];
            for (int p = 0; p < 3; p++) {
                l.row_stride[p] = rs[p];
                arr[p].resize((size_t)m);
                for (int f = 0; f < m; f++) {
                    long long a = 0;
                    in >> a;
                    arr[p][f] = addr(a);
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
                    for (size_t i = 0; i < tab.size(); i++) tab[i] = addr((long long)(0x7f0000000000ull + s.plane_off[i]));
                    as_staged = list_vec_eligible(k, tab.data());
                }
            }
            std::vector<size_t> off, bytes;
            for (const StageSpan& sp : s.span) { off.push_back(sp.off); bytes.push_back(sp.bytes); }
            std::printf("%d|%s|%d|%d|%d|%zu|%s|%s|%s|%zu|%zu|%d|%d|%d|%d|%d\n", r.status, r.why ? r.why : "", k.format, r.status ? 0 : k.planes(),
                        r.status ? 0 : k.px_bytes(), s.span.size(), join(off).c_str(), join(bytes).c_str(), join(s.plane_off).c_str(), s.total, s.copied,
                        as_given, as_staged, r.status ? 0 : k.sub_rows(), r.status ? 0 : k.sub_row_bytes(), r.status ? 0 : k.full_range);
        } else {
            std::fprintf(stderr, "unknown case kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
