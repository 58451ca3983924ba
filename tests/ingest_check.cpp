// ingest_check.cpp -- csrc/avd_ingest_clip.h as a stand-alone host program: the one program behind every ingest host test (tests/ingest_host_kit.py
// builds it with the address and undefined-behaviour sanitizers and runs it as its own process).  One case per line of standard input, integers
// separated by blanks; one answer line per case, `key=value` fields separated by `|`, so a field added later breaks no reader.  Addresses are
// made up: the header never reads through them.
//   A        -> picture_size, list_size, list_offsets (of format, plane, row_stride, mem, n, h, w, rotate, reserved), AVD_FMT_FULL_RANGE and every
//               AVD_FMT_<layout> by name (from include/avd.h, not from the table), rows (the values that have a row)
//   T value h w
//            -> has_row, and of a row: value, name, planes, px, sample, sub_rows, sub_row (the accessors of a clip of that layout and size)
//   P format mem n h w rotate reserved size_delta p0 p1 p2 rs0 rs1 rs2 fs0 fs1 fs2
//            an avd_picture (struct_size = sizeof + size_delta) through from_picture and check_clip, then clip_stage -> the clip fields
//   L format mem n h w rotate reserved size_delta rs0 rs1 rs2 null_arrays  a[0][0..m) a[1][0..m) a[2][0..m)      m = max(n, 0)
//            an avd_frame_list (null_arrays: bit p set = plane[p] is a null ARRAY) through from_frame_list and check_clip, then list_stage and
//            list_vec_eligible -> the clip fields (plane_off: p * n + f), given (eligible with the addresses themselves, a device list) and
//            staged (with 256-aligned base + plane offset, a staged one)
//   C mem n h w p0 p1 rs0 rs1 fs0 fs1
//            an avd_clip through from_public and check_clip, then clip_stage -> the clip fields
//   D format mem n h w p0 p1 p2 rs0 rs1 fs0 fs1
//            bgr_clip / nv12_clip / i420_clip by format, check_clip, clip_stage -> the clip fields
// the clip fields: status, why (the first refusal: the descriptor's, then check_clip's), format, full, rotate (as the IngestClip carries them:
// zeros where the descriptor was refused), planes, px, sub_rows, sub_row (zeros for a refused clip), nspans, off, bytes (per span), plane_off,
// total, copied; of a strided clip also vec (strided_vec_eligible at the addresses themselves)
#include <cstddef>
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

static void print_clip(const Refusal& r, const IngestClip& k, const std::vector<size_t>& off, const std::vector<size_t>& bytes,
                       const std::vector<size_t>& plane_off, size_t total, size_t copied, const char* tail)
{
    const bool ok = !r.status;
    std::printf("status=%d|why=%s|format=%d|full=%d|rotate=%d|planes=%d|px=%d|sub_rows=%d|sub_row=%d|nspans=%zu|off=%s|bytes=%s|plane_off=%s|total=%zu|copied=%zu%s\n",
                r.status, r.why ? r.why : "", k.format, k.full_range, k.rotate, ok ? k.planes() : 0, ok ? k.px_bytes() : 0, ok ? k.sub_rows() : 0,
                ok ? k.sub_row_bytes() : 0, off.size(), join(off).c_str(), join(bytes).c_str(), join(plane_off).c_str(), total, copied, tail);
}

// a strided clip: check_clip unless already refused, then its staging plan
static void answer_strided(Refusal r, const IngestClip& k)
{
    if (!r.status) r = check_clip(k);
    ClipStage s{};
    if (!r.status) s = clip_stage(k);
    std::vector<size_t> off, bytes, plane_off;
    for (int i = 0; i < s.nspans; i++) { off.push_back(s.span[i].off); bytes.push_back(s.span[i].bytes); }
    if (s.nspans) plane_off.assign(s.plane_off, s.plane_off + k.planes());
    const std::string tail = "|vec=" + std::to_string(!r.status && strided_vec_eligible(k, k.data, k.uv, k.v));      // as a device clip, used in place
    print_clip(r, k, off, bytes, plane_off, s.total, s.copied, tail.c_str());
}

int main()
{
    static const struct { const char* name; int value; } named[] = {
        {"AVD_FMT_BGR24", AVD_FMT_BGR24}, {"AVD_FMT_NV12", AVD_FMT_NV12}, {"AVD_FMT_I420", AVD_FMT_I420}, {"AVD_FMT_RGB24", AVD_FMT_RGB24},
        {"AVD_FMT_BGRA32", AVD_FMT_BGRA32}, {"AVD_FMT_RGBA32", AVD_FMT_RGBA32}, {"AVD_FMT_RGBP", AVD_FMT_RGBP}, {"AVD_FMT_YUYV422", AVD_FMT_YUYV422},
        {"AVD_FMT_UYVY422", AVD_FMT_UYVY422}, {"AVD_FMT_I422", AVD_FMT_I422}, {"AVD_FMT_NV16", AVD_FMT_NV16}, {"AVD_FMT_P010", AVD_FMT_P010},
        {"AVD_FMT_I010", AVD_FMT_I010}, {"AVD_FMT_FULL_RANGE", AVD_FMT_FULL_RANGE}};
    char buf[1 << 16];
    while (std::fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string kind;
        if (!(in >> kind)) continue;
        long long a[3] = {0, 0, 0}, rs[3] = {0, 0, 0}, fs[3] = {0, 0, 0}, size_delta = 0;
        if (kind == "A") {
            const std::vector<size_t> offsets = {offsetof(avd_frame_list, format), offsetof(avd_frame_list, plane), offsetof(avd_frame_list, row_stride),
                                                 offsetof(avd_frame_list, mem), offsetof(avd_frame_list, n), offsetof(avd_frame_list, h),
                                                 offsetof(avd_frame_list, w), offsetof(avd_frame_list, rotate), offsetof(avd_frame_list, reserved)};
            std::vector<int> rows;
            for (const IngestLayout& r : kIngestLayouts) rows.push_back(r.value);
            std::printf("picture_size=%zu|list_size=%zu|list_offsets=%s|rows=%s", sizeof(avd_picture), sizeof(avd_frame_list), join(offsets).c_str(), join(rows).c_str());
            for (const auto& nv : named) std::printf("|%s=%d", nv.name, nv.value);
            std::printf("\n");
        } else if (kind == "T") {
            IngestClip k{};
            in >> k.format >> k.h >> k.w;
            if (!known_layout(k.format)) { std::printf("has_row=0\n"); continue; }
            std::printf("has_row=1|value=%d|name=%s|planes=%d|px=%d|sample=%d|sub_rows=%d|sub_row=%d\n", k.row().value, k.row().name, k.planes(), k.px_bytes(),
                        k.is_16bit() ? 2 : 1, k.sub_rows(), k.sub_row_bytes());
        } else if (kind == "P") {
            avd_picture p{};
            in >> p.format >> p.mem >> p.n >> p.h >> p.w >> p.rotate >> p.reserved >> size_delta >> a[0] >> a[1] >> a[2] >> rs[0] >> rs[1] >> rs[2] >> fs[0] >> fs[1] >> fs[2];
            p.struct_size = (uint32_t)(sizeof p + size_delta);
            for (int i = 0; i < 3; i++) { p.plane[i] = addr(a[i]); p.row_stride[i] = rs[i]; p.frame_stride[i] = fs[i]; }
            IngestClip k{};
            const Refusal r = from_picture(p, k);
            answer_strided(r, k);
        } else if (kind == "C") {
            avd_clip c{};
            in >> c.mem >> c.n >> c.h >> c.w >> a[0] >> a[1] >> rs[0] >> rs[1] >> fs[0] >> fs[1];
            c.data = addr(a[0]); c.uv = addr(a[1]);
            c.row_stride = rs[0]; c.uv_row_stride = rs[1]; c.frame_stride = fs[0]; c.uv_frame_stride = fs[1];
            answer_strided({0, nullptr}, from_public(c));
        } else if (kind == "D") {
            int format, mem, n, h, w;
            in >> format >> mem >> n >> h >> w >> a[0] >> a[1] >> a[2] >> rs[0] >> rs[1] >> fs[0] >> fs[1];
            if (format == AVD_FMT_BGR24) answer_strided({0, nullptr}, bgr_clip(addr(a[0]), mem, n, h, w, rs[0], fs[0]));
            else if (format == AVD_FMT_NV12) answer_strided({0, nullptr}, nv12_clip(addr(a[0]), addr(a[1]), mem, n, h, w, rs[0], rs[1], fs[0], fs[1]));
            else if (format == AVD_FMT_I420) answer_strided({0, nullptr}, i420_clip(addr(a[0]), addr(a[1]), addr(a[2]), mem, n, h, w, rs[0], rs[1], fs[0], fs[1]));
            else { std::fprintf(stderr, "no named constructor for format %d\n", format); return 2; }
        } else if (kind == "L") {
            avd_frame_list l{};
            int null_arrays;
            in >> l.format >> l.mem >> l.n >> l.h >> l.w >> l.rotate >> l.reserved >> size_delta >> rs[0] >> rs[1] >> rs[2] >> null_arrays;
            l.struct_size = (uint32_t)(sizeof l + size_delta);
            const int m = l.n > 0 ? l.n : 0;
            std::vector<const uint8_t*> arr[3];
            for (int p = 0; p < 3; p++) {
                l.row_stride[p] = rs[p];
                arr[p].resize((size_t)m);
                for (int f = 0; f < m; f++) {
                    long long v = 0;
                    in >> v;
                    arr[p][f] = addr(v);
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
            const std::string tail = "|given=" + std::to_string(as_given) + "|staged=" + std::to_string(as_staged);
            print_clip(r, k, off, bytes, s.plane_off, s.total, s.copied, tail.c_str());
        } else {
            std::fprintf(stderr, "unknown case kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
