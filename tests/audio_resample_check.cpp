// Stand-alone check of csrc/avd_audio_resample.h (ratios, filter banks, output ranges and the tile table of a converted avd_audio_features call),
// built with the address and undefined-behaviour sanitizers by tests/audio_resample_kit.py and run as a program.  AUDIO_RESAMPLE_HEADER names the
// header under test: the library's own, or a mutated copy that this program must reject.
//
//   audio_resample_check                     every check; prints "audio resample: N plans checked, F failures", status 1 if F > 0
//   audio_resample_check taps RATE           prints "U D T tile_out" and the bank, one phase per line
//   audio_resample_check plan RATE n cut*    prints that call's tracks and tiles
//
// What a plan is compared with is written out again here from the rule in include/avd.h, output sample by output sample: nothing below calls the
// header to learn what the header should say.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include AUDIO_RESAMPLE_HEADER

using namespace avd_resample;

static long g_plans = 0, g_failures = 0;

#define EXPECT(cond, ...)                                                                                     \
    do {                                                                                                      \
        if (!(cond)) {                                                                                        \
            if (g_failures++ < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                     \
    } while (0)

static long long gcd_of(long long a, long long b) { while (b) { const long long c = a % b; a = b; b = c; } return a; }

// the rule, per output sample m of a track [begin, end): it reads frames begin + floor(m D / U) - T/2 + 1 ... through row (m D) mod U
static void check_plan(int rate, long long n, const std::vector<int>& cuts)
{
    g_plans++;
    Ratio r;
    EXPECT(ratio_of(rate, r), "rate %d", rate);
    const long long g = gcd_of(rate, 16000), U = 16000 / g, D = rate / g;
    EXPECT(r.U == U && r.D == D && r.T % 2 == 0, "rate %d: U %d D %d T %d", rate, r.U, r.D, r.T);
    const long long T = r.T, back = T ? T / 2 - 1 : 0;
    const Plan p = plan_convert(n, r, cuts.data(), (int)cuts.size());
    EXPECT(p.refused == kOk, "rate %d n %lld", rate, n);
    if (p.refused) return;
    const int ntracks = (int)cuts.size() + 1;
    EXPECT((int)p.tracks.size() == ntracks && p.out_cuts.size() == cuts.size() && p.n_in == n, "rate %d n %lld: %zu tracks", rate, n, p.tracks.size());
    if ((int)p.tracks.size() != ntracks || p.out_cuts.size() != cuts.size()) return;
    EXPECT(p.tile_out >= 256 && p.tile_out <= 1024 && p.tile_out % 256 == 0 && p.tile_out == tile_outputs(r), "rate %d: %d outputs per tile", rate, p.tile_out);
    long long out_at = 0;
    size_t tile = 0;
    for (int t = 0; t < ntracks; t++) {
        const long long begin = t ? cuts[t - 1] : 0, end = t + 1 < ntracks ? cuts[t] : n;
        long long count = (end - begin) * U / D;
        if (count * D < (end - begin) * U) count++;                         // ceil
        EXPECT(p.tracks[t].first == out_at && p.tracks[t].count == count, "rate %d n %lld track %d: %d %d, want %lld %lld", rate, n, t, p.tracks[t].first,
               p.tracks[t].count, out_at, count);
        if (t) EXPECT(p.out_cuts[t - 1] == out_at, "rate %d n %lld: output cut %d is %d, want %lld", rate, n, t - 1, p.out_cuts[t - 1], out_at);
        // the track's tiles cover its outputs in order; every output is checked up to 300000 of them, else both ends and where m D passes 2^31 and 2^32
        long long m0 = 0;
        while (m0 < count) {
            EXPECT(tile < p.tiles.size(), "rate %d n %lld track %d: the tiles end at output %lld of %lld", rate, n, t, m0, count);
            if (tile >= p.tiles.size()) return;
            const Tile& x = p.tiles[tile++];
            const long long want_count = count - m0 < p.tile_out ? count - m0 : p.tile_out;
            EXPECT(x.count == want_count && x.out0 == out_at + m0 && x.begin == begin && x.end == end, "rate %d n %lld track %d tile at %lld: count %d out0 %lld [%lld, %lld)",
                   rate, n, t, m0, x.count, x.out0, x.begin, x.end);
            EXPECT(x.phase >= 0 && x.phase < U, "rate %d n %lld: phase %d", rate, n, x.phase);
            if (x.count < 1 || x.count > p.tile_out || x.phase < 0 || x.phase >= U) return;
            const int span = tile_span(r, x.count, x.phase);
            EXPECT(span >= 1 && span <= max_span(r), "rate %d n %lld: a span of %d frames, at most %d", rate, n, span, max_span(r));
            const bool all = count <= 300000 || m0 < 4096 || m0 + 2 * p.tile_out >= count;
            const long long m_wrap31 = (1LL << 31) / D, m_wrap32 = (1LL << 32) / D;
            const bool near_wrap = (m0 <= m_wrap31 + p.tile_out && m0 + 2 * p.tile_out >= m_wrap31) || (m0 <= m_wrap32 + p.tile_out && m0 + 2 * p.tile_out >= m_wrap32);
            if (all || near_wrap)
                for (int j = 0; j < x.count; j++) {
                    const long long m = m0 + j, pos = (long long)x.phase + (long long)j * D;
                    const long long want_frame = begin + m * D / U - back, want_phi = m * D % U;
                    EXPECT(pos <= 0x7fffffff, "rate %d: position %lld inside a tile leaves 32 bits", rate, pos);
                    EXPECT(x.in0 + pos / U == want_frame && pos % U == want_phi, "rate %d n %lld track %d output %lld: frame %lld phase %lld, want %lld %lld", rate, n, t, m,
                           x.in0 + pos / U, pos % U, want_frame, want_phi);
                    EXPECT(pos / U + (T ? T : 1) <= span, "rate %d n %lld output %lld reads beyond its tile's span", rate, n, m);
                }
            m0 += x.count;
        }
        // the last output's centre frame lies inside the track, one more output's would not
        EXPECT((count - 1) * D / U < end - begin && count * D / U >= end - begin, "rate %d n %lld track %d: %lld outputs of %lld frames", rate, n, t, count, end - begin);
        out_at += count;
    }
    EXPECT(tile == p.tiles.size() && p.n_out == out_at, "rate %d n %lld: %zu tiles, %zu used; %lld outputs, want %lld", rate, n, p.tiles.size(), tile, p.n_out, out_at);
}

static void check_bank(int rate)
{
    g_plans++;
    Ratio r;
    if (!ratio_of(rate, r)) { EXPECT(false, "rate %d", rate); return; }
    const std::vector<int> q = build_taps(r);
    EXPECT(q.size() == (size_t)r.U * (size_t)r.T && q.size() <= (size_t)kMaxBank, "rate %d: %zu entries", rate, q.size());
    for (int ch = 1; ch <= 2; ch++) EXPECT(lds_bytes(r, ch) <= 160u * 1024u, "rate %d, %d channels: %zu bytes of LDS", rate, ch, lds_bytes(r, ch));
    for (int phi = 0; phi < r.U && r.T; phi++) {
        long long sum = 0, mag = 0;
        int lo = 0, hi = 0;
        for (int k = 0; k < r.T; k++) {
            const int v = q[(size_t)phi * (size_t)r.T + (size_t)k];
            sum += v; mag += v < 0 ? -v : v;
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
        EXPECT(sum == 32768, "rate %d phase %d sums to %lld", rate, phi, sum);
        if (!wide(r)) EXPECT(mag <= 65535 && mag * 32768 + 16384 < (1LL << 31) && lo >= -32768 && hi <= 32767, "rate %d phase %d: sum|q| %lld, entries %d ... %d", rate, phi, mag, lo, hi);
        else EXPECT(rate < 16000, "rate %d takes the wide path", rate);
    }
}

static std::vector<int> cuts_of(const std::vector<long long>& lens)
{
    std::vector<int> cuts;
    long long at = 0;
    for (size_t i = 0; i + 1 < lens.size(); i++) { at += lens[i]; cuts.push_back((int)at); }
    return cuts;
}
static long long sum_of(const std::vector<long long>& lens) { long long s = 0; for (long long l : lens) s += l; return s; }

static void check_everything()
{
    Ratio r;
    EXPECT(!ratio_of(0, r) && !ratio_of(44000, r) && !ratio_of(-48000, r) && !ratio_of(15999, r), "rates outside the list");
    for (int rate : kRates) {
        check_bank(rate);
        // every call of up to 9 frames and every set of cuts; tracks around the tile size
        for (int n = 1; n <= 9; n++)
            for (unsigned m = 0; m < (1u << (n - 1)); m++) {
                std::vector<int> cuts;
                for (int c = 1; c < n; c++) if (m & (1u << (c - 1))) cuts.push_back(c);
                check_plan(rate, n, cuts);
            }
        ratio_of(rate, r);
        const long long per_tile = (long long)tile_outputs(r) * r.D / r.U;
        for (long long n : {per_tile - 1, per_tile, per_tile + 1, 3 * per_tile + 1, 100003LL}) check_plan(rate, n, {});
        // cuts at every frame mod D
        std::vector<long long> lens;
        for (int t = 0; t < 64; t++) lens.push_back(2 * per_tile / 3 + t % (r.D + 1) + (t % 5 == 0 ? per_tile : 0));
        check_plan(rate, sum_of(lens), cuts_of(lens));
    }
    // m D passes 2^31 (five minutes at D = 441) and 2^32
    check_plan(44100, 13500000, {});
    check_plan(44100, 30000000, {1000000, 29000001});
    check_plan(176400, 60000000, {});
    check_plan(192000, 0x7fffffff, {});
    check_plan(8000, 1000000000, {123456789});
    // refusals
    {
        const int c1[] = {5, 10}, c2[] = {5, 9};
        ratio_of(48000, r);
        g_plans += 3;
        EXPECT(plan_convert(10, r, c1, 2).refused == kCutBeyond, "a cut at n");
        EXPECT(plan_convert(10, r, c2, 2).refused == kOk, "cuts 5, 9 of 10 frames");
        const Plan a = plan_convert(10, r, c2, 2);
        EXPECT(a.tracks.size() == 3 && a.tracks[0].count == 2 && a.tracks[1].count == 2 && a.tracks[2].count == 1 && a.n_out == 5, "5 + 4 + 1 frames at 48000 are 2 + 2 + 1 outputs");
        ratio_of(8000, r);
        const Plan b = plan_convert(1LL << 31, r, nullptr, 0);
        EXPECT(b.refused == kTooLong && b.tiles.empty() && b.tracks.empty(), "2^32 output samples");
    }
}

int main(int argc, char** argv)
{
    if (argc == 1) {
        check_everything();
        std::printf("audio resample: %ld plans checked, %ld failures\n", g_plans, g_failures);
        return g_failures ? 1 : 0;
    }
    Ratio r;
    if (argc == 3 && std::strcmp(argv[1], "taps") == 0) {
        if (!ratio_of(std::atoi(argv[2]), r)) return 2;
        const std::vector<int> q = build_taps(r);
        std::printf("%d %d %d %d\n", r.U, r.D, r.T, tile_outputs(r));
        for (int phi = 0; phi < r.U; phi++) {
            for (int k = 0; k < r.T; k++) std::printf("%d ", q[(size_t)phi * (size_t)r.T + (size_t)k]);
            std::printf("\n");
        }
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "plan") == 0) {
        if (!ratio_of(std::atoi(argv[2]), r)) return 2;
        const long long n = std::atoll(argv[3]);
        std::vector<int> cuts;
        for (int i = 4; i < argc; i++) cuts.push_back(std::atoi(argv[i]));
        if (n < 1 || cuts.size() > 63) return 2;
        const Plan p = plan_convert(n, r, cuts.data(), (int)cuts.size());
        std::printf("refused %d tile_out %d n_out %lld ntiles %zu\n", p.refused, p.tile_out, p.n_out, p.tiles.size());
        std::printf("tracks");
        for (const Track& t : p.tracks) std::printf(" %d:%d", t.first, t.count);
        std::printf("\ntiles");
        if (p.tiles.size() <= 64)
            for (const Tile& t : p.tiles) std::printf(" %lld:%lld:%d:%d", t.in0, t.out0, t.count, t.phase);
        else
            for (size_t i : {(size_t)0, p.tiles.size() - 1}) std::printf(" %lld:%lld:%d:%d", p.tiles[i].in0, p.tiles[i].out0, p.tiles[i].count, p.tiles[i].phase);
        std::printf("\n");
        return 0;
    }
    return 2;
}
