// tables_check.cpp -- the host-built resampling tables (csrc/avd_tables.cpp) at every frame size, no GPU, no library.
// Built by tests/tables_kit.py with the address and undefined-behaviour sanitizers and run as its own process (tests/test_tables_host.py).
//
// Linked: csrc/avd_tables.cpp as it is (builder 0) and three copies of it that the kit mutates textually and renames with -D (builders
// 1 .. 3, the controls), and oracle/avd_oracle.c.
//
//   tables_check full [every [part parts]]
//                                   invariants of the tables for every size 32 .. 16384 on each axis, then the tables APPLIED -- a plain
//                                   restatement of what the kernels are documented to do with them -- against the oracle's resizes, byte for
//                                   byte, on seeded random gray images 32 x s and s x 32 (the set of s: compare_sizes; every = the step of the
//                                   thinned sizes above 4400, default 64), the class crossings in two dimensions, and a few other destinations;
//                                   part / parts: only the sizes s with s % parts == part
//   tables_check image M H W DH DW FILE
//                                   builder M on the H x W gray image in FILE (raw bytes): how many bytes of the 320 x 320 INTER_LINEAR image
//                                   and of the DH x DW INTER_AREA image differ from the oracle's
// Answers are `key=value` lines on stdout; a failed check is a line that starts with FAIL.  Exit status 0 unless `full` found something.
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "avd_internal.h"
#include "avd_oracle.h"

#define MUTANT(n)                                                                                   \
    void build_linear_tab_m##n(int src_h, int src_w, int dst_h, int dst_w, LinearTab& t);           \
    int build_area_tab_m##n(int src_h, int src_w, int dst_h, int dst_w, AreaTab& t);
MUTANT(1) MUTANT(2) MUTANT(3)

namespace {

struct Builder {
    void (*linear)(int, int, int, int, LinearTab&);
    int (*area)(int, int, int, int, AreaTab&);
};
const Builder kBuilders[4] = {{build_linear_tab, build_area_tab}, {build_linear_tab_m1, build_area_tab_m1},
                              {build_linear_tab_m2, build_area_tab_m2}, {build_linear_tab_m3, build_area_tab_m3}};

constexpr int kMin = 32, kMax = 16384, kBandCap = 14;      // the sizes the API accepts; rows per band: 1 .. 14 (band_plan, avd_preprocess.hip)
long g_fail = 0;

#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            if (++g_fail <= 40) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                         \
    } while (0)

// ---- cv2's own decisions, restated from its expressions (resize.cpp) -------------------------------------------------------------------
inline double cv_scale(int src, int dst) { return 1. / ((double)dst / src); }
inline bool cv_integral(int src, int dst) { const double s = cv_scale(src, dst); return std::fabs(s - (int)std::nearbyint(s)) < DBL_EPSILON; }
// a size the destination divides at which the reciprocal of the reciprocal is not the quotient
inline bool flips(int src, int dst) { return src % dst == 0 && cv_scale(src, dst) != (double)(src / dst); }

// ---- the tables applied: what avd_preprocess.hip does with them ----------------------------------------------------------------------
// INTER_LINEAR: cv2's Q11 horizontal pass, then the >> 4, >> 16, + 2 >> 2 vertical pass; indices and weights as the shorts build_geom packs
void apply_linear(const uint8_t* img, int w, const LinearTab& t, std::vector<uint8_t>& out)
{
    const int dh = (int)t.y0.size(), dw = (int)t.x0.size();
    out.resize((size_t)dh * dw);
    for (int dy = 0; dy < dh; dy++) {
        const uint8_t* ra = img + (size_t)(short)t.y0[dy] * w;
        const uint8_t* rb = img + (size_t)(short)t.y1[dy] * w;
        const int wy0 = t.b0[dy], wy1 = t.b1[dy];
        for (int dx = 0; dx < dw; dx++) {
            const int x0 = (short)t.x0[dx], x1 = (short)t.x1[dx], wx0 = t.a0[dx], wx1 = t.a1[dx];
            const int ha = ra[x0] * wx0 + ra[x1] * wx1;
            const int hb = rb[x0] * wx0 + rb[x1] * wx1;
            out[(size_t)dy * dw + dx] = (uint8_t)((((wy0 * (ha >> 4)) >> 16) + ((wy1 * (hb >> 4)) >> 16) + 2) >> 2);
        }
    }
}

inline float tap_weight(const AreaAxis& a, int d, int k) { return k == 0 ? a.w_first[d] : (k == a.count[d] - 1 ? a.w_last[d] : a.w_mid[d]); }

// INTER_AREA.  fast: integer sums times 1.f / area, (sum + 2) >> 2 in the 8-wide groups of the 2 x 2 case.  general: a float chain per
// (row, cell) in cv2's tap order, then a float chain down the rows of a cell that STARTS with its first product, then rint.
void apply_area(const uint8_t* img, int h, int w, const AreaTab& t, std::vector<uint8_t>& out)
{
    const int dh = (int)t.y.begin.size(), dw = (int)t.x.begin.size();
    out.resize((size_t)dh * dw);
    std::vector<float> rowf((size_t)h * dw);
    std::vector<int> rowi((size_t)h * dw);
    for (int y = 0; y < h; y++)
        for (int dx = 0; dx < dw; dx++) {
            const uint8_t* s = img + (size_t)y * w + t.x.begin[dx];
            if (t.fast) {
                int a = 0;
                for (int k = 0; k < t.x.count[dx]; k++) a += s[k];
                rowi[(size_t)y * dw + dx] = a;
            } else {
                float a = 0.f;
                for (int k = 0; k < t.x.count[dx]; k++) a = a + (float)s[k] * tap_weight(t.x, dx, k);
                rowf[(size_t)y * dw + dx] = a;
            }
        }
    const int simd_w = (t.fast && t.iscale_x == 2 && t.iscale_y == 2) ? (dw & ~7) : 0;
    for (int dy = 0; dy < dh; dy++)
        for (int dx = 0; dx < dw; dx++) {
            const int y0 = t.y.begin[dy], cnt = t.y.count[dy];
            int cell;
            if (t.fast) {
                int acc = 0;
                for (int k = 0; k < cnt; k++) acc += rowi[(size_t)(y0 + k) * dw + dx];
                cell = dx < simd_w ? (acc + 2) >> 2 : (int)std::nearbyintf((float)acc * (1.f / (float)(t.iscale_x * t.iscale_y)));
            } else {
                float acc = 0.f;
                for (int k = 0; k < cnt; k++) {
                    const float p = tap_weight(t.y, dy, k) * rowf[(size_t)(y0 + k) * dw + dx];
                    acc = k == 0 ? p : acc + p;
                }
                cell = (int)std::nearbyintf(acc);
            }
            out[(size_t)dy * dw + dx] = (uint8_t)std::min(255, std::max(0, cell));
        }
}

long count_differences(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b)
{
    long n = 0;
    for (size_t i = 0; i < a.size(); i++) n += a[i] != b[i];
    return n + (a.size() != b.size());
}

struct Differences { long linear, area; };

// builder m on one image against the oracle: the 320 x 320 image always, the adh x adw area image where INTER_AREA is defined (no upscaling)
Differences compare(const Builder& m, const uint8_t* img, int h, int w, int adh, int adw)
{
    Differences d{0, 0};
    std::vector<uint8_t> got, want((size_t)AVD_SMALL * AVD_SMALL);
    LinearTab lt;
    m.linear(h, w, AVD_SMALL, AVD_SMALL, lt);
    apply_linear(img, w, lt, got);
    if (avdo_resize_linear_u8(img, h, w, want.data(), AVD_SMALL, AVD_SMALL)) d.linear = -1;
    else d.linear = count_differences(got, want);
    AreaTab at;
    want.assign((size_t)adh * adw, 0);
    const int rc = m.area(h, w, adh, adw, at), orc = avdo_resize_area_u8(img, h, w, want.data(), adh, adw);
    if (rc || orc) { d.area = (rc != 0) == (orc != 0) ? 0 : -1; return d; }      // both refuse an upscale, or neither does
    apply_area(img, h, w, at, got);
    d.area = count_differences(got, want);
    return d;
}

// seeded noise (splitmix64): full-range bytes keep the area cells away from saturation and close to every rounding boundary
void fill_random(std::vector<uint8_t>& img, size_t n, uint64_t seed)
{
    img.resize(n);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
    for (size_t i = 0; i < n; i += 8) {
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        for (size_t j = 0; j < 8 && i + j < n; j++) img[i + j] = (uint8_t)(z >> (8 * j));
    }
}

// ---- a. invariants ---------------------------------------------------------------------------------------------------------------------
void check_linear_axis(int s, const char* axis, const std::vector<int>& i0, const std::vector<int>& i1, const std::vector<short>& w0,
                       const std::vector<short>& w1)
{
    CHECK((int)i0.size() == AVD_SMALL && i1.size() == i0.size() && w0.size() == i0.size() && w1.size() == i0.size(), "%s s=%d", axis, s);
    for (int d = 0; d < AVD_SMALL; d++) {
        CHECK(i0[d] >= 0 && i0[d] < s && i1[d] >= 0 && i1[d] < s, "%s s=%d d=%d taps %d %d", axis, s, d, i0[d], i1[d]);
        CHECK(i1[d] - i0[d] == 0 || i1[d] - i0[d] == 1, "%s s=%d d=%d taps %d %d", axis, s, d, i0[d], i1[d]);
        CHECK(i0[d] <= SHRT_MAX && i1[d] <= SHRT_MAX, "%s s=%d d=%d taps %d %d", axis, s, d, i0[d], i1[d]);
        CHECK((int)w0[d] + (int)w1[d] == 2048 && w0[d] >= 0 && w1[d] >= 0, "%s s=%d d=%d weights %d %d", axis, s, d, w0[d], w1[d]);
        if (d) CHECK(i0[d] >= i0[d - 1], "%s s=%d d=%d index %d after %d", axis, s, d, i0[d], i0[d - 1]);
    }
}

void check_area_axis(int s, const char* axis, const AreaAxis& a)
{
    CHECK((int)a.begin.size() == AVD_HASH, "%s s=%d", axis, s);
    for (int d = 0; d < AVD_HASH; d++) {
        const int b = a.begin[d], c = a.count[d];
        CHECK(b >= 0 && c >= 1 && b + c <= s, "%s s=%d cell %d [%d, +%d)", axis, s, d, b, c);
        if (d) {
            const int prev_end = a.begin[d - 1] + a.count[d - 1];
            CHECK(b == prev_end || b == prev_end - 1, "%s s=%d cell %d begins at %d, cell %d ends at %d", axis, s, d, b, d - 1, prev_end);
        } else CHECK(b == 0, "%s s=%d first cell begins at %d", axis, s, b);
        double sum = 0;
        for (int k = 0; k < c; k++) sum += tap_weight(a, d, k);
        CHECK(std::fabs(sum - 1.) <= 1e-5, "%s s=%d cell %d weights sum to %.9g", axis, s, d, sum);
        CHECK(a.w_first[d] > 0 && a.w_mid[d] > 0 && a.w_last[d] > 0, "%s s=%d cell %d weights %g %g %g", axis, s, d, a.w_first[d], a.w_mid[d], a.w_last[d]);
    }
    CHECK(a.begin[AVD_HASH - 1] + a.count[AVD_HASH - 1] == s, "%s s=%d the last cell ends at %d", axis, s, a.begin[AVD_HASH - 1] + a.count[AVD_HASH - 1]);
}

// the fourth x-side class as build_geom decides it (csrc/avd_capi.hip), from the table content
bool uniform4(const AreaAxis& a)
{
    for (int d = 0; d < AVD_HASH; d++)
        if ((a.begin[d] & 3) || (a.count[d] & 3) || a.count[d] < 4 || a.w_first[d] != a.w_mid[d] || a.w_last[d] != a.w_mid[d]) return false;
    return true;
}

// part / parts: this process takes the sizes s with s % parts == part (the test runs the parts side by side and adds the answers up)
void invariants(int part, int parts)
{
    std::vector<int> flip32, flip320, reroute, band_dy;
    int fast_sizes = 0, uniform4_sizes = 0, general_path_integral = 0;
    for (int s = kMin; s <= kMax; s++) {
        if (s % parts != part) continue;
        LinearTab lt;
        build_linear_tab(s, s, AVD_SMALL, AVD_SMALL, lt);
        check_linear_axis(s, "linear x", lt.x0, lt.x1, lt.a0, lt.a1);
        check_linear_axis(s, "linear y", lt.y0, lt.y1, lt.b0, lt.b1);
        // the horizontal axis snaps onto the edge pixel, the vertical one keeps its weights: the indices are the same
        CHECK(lt.x0 == lt.y0, "s=%d x0 and y0 differ", s);

        // one axis at a time: the other axis has scale 1, which is integral, so `fast` is this axis's decision alone
        AreaTab ax, ay;
        CHECK(build_area_tab(kMin, s, AVD_HASH, AVD_HASH, ax) == 0 && build_area_tab(s, kMin, AVD_HASH, AVD_HASH, ay) == 0, "s=%d refused", s);
        check_area_axis(s, "area x", ax.x);
        check_area_axis(s, "area y", ay.y);
        check_area_axis(kMin, "area y of 32 rows", ax.y);
        const bool flip = flips(s, AVD_HASH), want_fast = s % AVD_HASH == 0 && !flip;
        if (flip) flip32.push_back(s);
        CHECK(want_fast == cv_integral(s, AVD_HASH), "s=%d cv2's predicate and the list of flip sizes disagree", s);
        CHECK(ax.fast == want_fast && ay.fast == want_fast, "s=%d fast %d %d, want %d", s, ax.fast, ay.fast, want_fast);
        if (s % AVD_HASH == 0) CHECK(ax.iscale_x == s / AVD_HASH && ay.iscale_y == ax.iscale_x && ax.iscale_y == 1 && ay.iscale_x == 1, "s=%d iscale", s);
        fast_sizes += want_fast;
        if (want_fast)
            for (int d = 0; d < AVD_HASH; d++)
                CHECK(ax.x.begin[d] == d * ax.iscale_x && ax.x.count[d] == ax.iscale_x && ay.y.begin[d] == d * ax.iscale_x && ay.y.count[d] == ax.iscale_x,
                      "s=%d fast cell %d is not the box", s, d);
        if (flip) {             // the general path with an integral scale: full boxes, one weight missing
            general_path_integral++;
            for (int d = 0; d < AVD_HASH; d++)
                CHECK(ax.x.count[d] == ax.iscale_x && ax.x.begin[d] == d * ax.iscale_x, "s=%d flip cell %d [%d, +%d)", s, d, ax.x.begin[d], ax.x.count[d]);
        }
        uniform4_sizes += !want_fast && uniform4(ax.x);
        if (uniform4(ax.x)) CHECK(s % 128 == 0, "s=%d uniform4 at a width that is no multiple of 128", s);

        // the 320-px resize: the same flip, and INTER_LINEAR's reroute to INTER_AREA at an exact 2 x 2 (the oracle's predicate)
        if (flips(s, AVD_SMALL)) flip320.push_back(s);
        if (cv_integral(s, AVD_SMALL) && (int)std::nearbyint(cv_scale(s, AVD_SMALL)) == 2) reroute.push_back(s);

        // band_dy for every number of rows per band: by its definition, entry by entry
        for (int R = 1; R <= kBandCap; R++) {
            build_band_dy(lt, s, R, band_dy);
            const int nbands = (s + R - 1) / R;
            CHECK((int)band_dy.size() == nbands + 1 && band_dy[0] == 0 && band_dy[nbands] == AVD_SMALL, "h=%d R=%d band_dy ends", s, R);
            if ((int)band_dy.size() != nbands + 1) continue;
            for (int b = 0; b < nbands; b++) CHECK(band_dy[b] <= band_dy[b + 1], "h=%d R=%d band %d: %d then %d", s, R, b, band_dy[b], band_dy[b + 1]);
            // every output row belongs to the band that holds its upper source row, and to no other; both its source rows then lie in
            // that band's tile, rows [b R - 1, b R + R]
            for (int d = 0; d < AVD_SMALL; d++) {
                const int b = lt.y0[d] / R;
                CHECK(b < nbands && band_dy[b] <= d && d < band_dy[b + 1] && lt.y1[d] <= b * R + R, "h=%d R=%d output row %d reads rows %d %d", s, R, d, lt.y0[d], lt.y1[d]);
            }
        }
    }
    std::printf("fast_sizes=%d\nuniform4_sizes=%d\nflip_sizes=%d\n", fast_sizes, uniform4_sizes, general_path_integral);
    std::printf("flip32=");
    for (size_t i = 0; i < flip32.size(); i++) std::printf("%s%d", i ? "," : "", flip32[i]);
    std::printf("\nflip320=");
    for (size_t i = 0; i < flip320.size(); i++) std::printf("%s%d", i ? "," : "", flip320[i]);
    std::printf("\nreroute320=");
    for (size_t i = 0; i < reroute.size(); i++) std::printf("%s%d", i ? "," : "", reroute[i]);
    std::printf("\n");
}

// ---- b. the tables mean what the oracle computes ----------------------------------------------------------------------------------------
std::set<int> compare_sizes(int every)
{
    std::set<int> s;
    for (int v = kMin; v <= 4400; v++) s.insert(v);
    for (int v = kMin; v <= kMax; v += AVD_HASH) s.insert(v);              // all fast and all flip sizes
    for (int v = AVD_SMALL; v <= kMax; v += AVD_SMALL) s.insert(v);
    for (int v : {16383, 16384, 15679, 15680, 15681}) s.insert(v);
    for (int v = 4400 + every; v <= kMax; v += every) s.insert(v);
    return s;
}

void report(const char* what, int h, int w, int adh, int adw, const Differences& d)
{
    CHECK(d.linear == 0, "%s %d x %d INTER_LINEAR 320 x 320: %ld bytes differ from the oracle", what, h, w, d.linear);
    CHECK(d.area == 0, "%s %d x %d INTER_AREA %d x %d: %ld bytes differ from the oracle", what, h, w, adh, adw, d.area);
}

void comparisons(int every, int part, int parts)
{
    std::vector<uint8_t> img;
    const std::set<int> sizes = compare_sizes(every);
    long geometries = 0, compared = 0;
    for (int s : sizes) {
        if (s % parts != part) continue;
        compared++;
        fill_random(img, (size_t)kMin * s, (uint64_t)s * 2 + 0);
        report("wide", kMin, s, AVD_HASH, AVD_HASH, compare(kBuilders[0], img.data(), kMin, s, AVD_HASH, AVD_HASH));
        fill_random(img, (size_t)kMin * s, (uint64_t)s * 2 + 1);
        report("tall", s, kMin, AVD_HASH, AVD_HASH, compare(kBuilders[0], img.data(), s, kMin, AVD_HASH, AVD_HASH));
        geometries += 2 - (s == kMin);
    }
    // the classes crossed in two dimensions: fast, general, flip, uniform4, the 2 x 2 reroute (640 x 640 alone), up on one axis and down on the other
    const int cross[] = {32, 64, 96, 128, 256, 320, 333, 640, 641, 1568, 3136};
    int item = 0;
    for (int h : cross)
        for (int w : cross) {
            if (item++ % parts != part) continue;
            fill_random(img, (size_t)h * w, (uint64_t)h * 65536 + w);
            report("cross", h, w, AVD_HASH, AVD_HASH, compare(kBuilders[0], img.data(), h, w, AVD_HASH, AVD_HASH));
            geometries += !(h == kMin || w == kMin);
        }
    // other destinations than 32 cells: fractions of a source sample between 1e-3 and 1e-2, which 32 cells never have (their
    // fractions are multiples of 1 / 32)
    const int other[][4] = {{32, 201, 32, 200}, {201, 32, 200, 32}, {203, 407, 200, 400}, {1001, 64, 500, 32}, {64, 2003, 32, 1000}};
    for (const auto& o : other) {
        if (item++ % parts != part) continue;
        fill_random(img, (size_t)o[0] * o[1], (uint64_t)o[0] * 65536 + o[1]);
        report("other", o[0], o[1], o[2], o[3], compare(kBuilders[0], img.data(), o[0], o[1], o[2], o[3]));
    }
    std::printf("compared_sizes=%ld\ncompared_geometries=%ld\n", compared, geometries);
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "full") {
        const int every = argc > 2 ? std::atoi(argv[2]) : 64;
        const int part = argc > 4 ? std::atoi(argv[3]) : 0, parts = argc > 4 ? std::atoi(argv[4]) : 1;
        if (every < 1 || parts < 1 || part < 0 || part >= parts) { std::printf("FAIL bad step or part\n"); return 2; }
        const auto t0 = std::chrono::steady_clock::now();
        invariants(part, parts);
        const auto t1 = std::chrono::steady_clock::now();
        comparisons(every, part, parts);
        const auto t2 = std::chrono::steady_clock::now();
        std::printf("invariants_seconds=%.1f\ncomparisons_seconds=%.1f\nfailures=%ld\n", std::chrono::duration<double>(t1 - t0).count(),
                    std::chrono::duration<double>(t2 - t1).count(), g_fail);
        return g_fail ? 1 : 0;
    }
    if (mode == "image" && argc == 8) {
        const int m = std::atoi(argv[2]), h = std::atoi(argv[3]), w = std::atoi(argv[4]), dh = std::atoi(argv[5]), dw = std::atoi(argv[6]);
        if (m < 0 || m > 3 || h < 1 || w < 1 || h > kMax || w > kMax || dh < 1 || dw < 1) { std::printf("FAIL bad arguments\n"); return 2; }
        std::vector<uint8_t> img((size_t)h * w);
        FILE* f = std::fopen(argv[7], "rb");
        const size_t got = f ? std::fread(img.data(), 1, img.size(), f) : 0;
        if (f) std::fclose(f);
        if (got != img.size()) { std::printf("FAIL short image file\n"); return 2; }
        const Differences d = compare(kBuilders[m], img.data(), h, w, dh, dw);
        std::printf("linear_differs=%ld\narea_differs=%ld\n", d.linear, d.area);
        return 0;
    }
    std::printf("FAIL usage: tables_check full [every [part parts]] | image M H W DH DW FILE\n");
    return 2;
}
