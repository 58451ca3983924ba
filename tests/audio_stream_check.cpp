// Stand-alone check of csrc/avd_audio_stream.h (what one call of a track continued across avd_audio_features calls forms, hands out and holds back:
// option "audio_slot"), built with the address and undefined-behaviour sanitizers by tests/audio_stream_kit.py and run as a program.
// AUDIO_STREAM_HEADER names the header under test: the library's own, or a mutated copy that this program must reject.
//
//   audio_stream_check                             every check; prints "audio stream: N calls checked, F failures", status 1 if F > 0
//   audio_stream_check m RATE N LAST               prints M of the rule (RATE 0: an unconverted track)
//   audio_stream_check plan RATE WIN BEFORE N LAST prints that call's plan and its tiles
//
// What a plan is compared with is written out again here from the rule in include/avd.h, output sample by output sample and frame by frame:
// nothing below calls the header to learn what the header should say.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include AUDIO_STREAM_HEADER

using namespace avd_resample;

static long g_calls = 0, g_failures = 0;

#define EXPECT(cond, ...)                                                                                     \
    do {                                                                                                      \
        if (!(cond)) {                                                                                        \
            if (g_failures++ < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                     \
    } while (0)

static bool ratio_for(int rate, Ratio& r)
{
    if (rate == 0) { r = identity_ratio(); return true; }
    return ratio_of(rate, r);
}

// One track of `total` frames handed over in calls of `chunk` frames (the last one shorter; flush: the last samples come in a call of their own
// that is NOT marked, and an empty marked call ends the track).  Every call's plan is checked against the rule, and the calls together against
// plan_convert's coverage of the whole track.
static void check_track(int rate, int win, long long total, long long chunk, bool flush)
{
    Ratio r;
    if (!ratio_for(rate, r)) { EXPECT(false, "rate %d", rate); return; }
    const long long U = r.U, D = r.D, T = r.T, half = T / 2;
    long long n_abs = 0, m_exist = 0, windows = 0;
    int held = 0, hist = 0;
    long long covered = 0;                                    // outputs the tiles have covered so far
    bool done = false;
    while (!done) {
        const long long n = std::min(chunk, total - n_abs);
        const bool last = flush ? n == 0 : n_abs + n == total;
        g_calls++;
        const Continue c = plan_continue(n_abs, n, last, r, win);
        EXPECT(c.refused == kOk, "rate %d at %lld + %lld", rate, n_abs, n);
        if (c.refused) return;
        const long long n_after = n_abs + n;
        // the outputs that exist: last tap floor(m D / U) + T/2 at or below frame N - 1; after the last call every output whose centre is inside
        long long want_m = m_exist;
        if (last) { want_m = n_after * U / D; if (want_m * D < n_after * U) want_m++; }
        else while (want_m * D / U + half <= n_after - 1) want_m++;
        EXPECT(c.n_before == n_abs && c.n_after == n_after && c.m_before == m_exist && c.m_after == want_m, "rate %d at %lld + %lld last %d: outputs [%lld, %lld), want [%lld, %lld)", rate,
               n_abs, n, (int)last, c.m_before, c.m_after, m_exist, want_m);
        EXPECT(c.held_before == held && c.hist_before == hist, "rate %d at %lld: held %d history %d, the call before left %d and %d", rate, n_abs, c.held_before, c.hist_before, held, hist);
        const long long have = held + (want_m - m_exist);
        const long long want_w = last ? (have + win - 1) / win : have / win;
        EXPECT(c.windows == want_w && c.analysed == (last ? have : want_w * win) && c.held_after == (last ? 0 : have - want_w * win) && c.held_after < win,
               "rate %d at %lld + %lld: %lld windows over %lld samples, %d held; want %lld windows of %lld samples", rate, n_abs, n, c.windows, c.analysed, c.held_after, want_w, have);
        const long long want_hist = last ? 0 : std::min<long long>(n_after, T > 0 ? T - 1 : 0);
        EXPECT(c.hist_after == want_hist && c.hist_after <= kMaxHistory, "rate %d at %lld + %lld: history %d, want %lld", rate, n_abs, n, c.hist_after, want_hist);
        // the tiles: the new outputs in order, every tap of every output readable
        long long m0 = m_exist;
        if (rate == 0) EXPECT(c.tiles.empty(), "an unconverted track has %zu tiles", c.tiles.size());
        else
            for (const Tile& x : c.tiles) {
                const long long want_count = std::min<long long>(c.tile_out, want_m - m0);
                EXPECT(x.count == want_count && x.count >= 1 && x.out0 == held + (m0 - m_exist) && x.begin == 0 && x.end == n_after, "rate %d at %lld tile at output %lld: count %d out0 %lld [%lld, %lld)",
                       rate, n_abs, m0, x.count, x.out0, x.begin, x.end);
                if (x.count < 1 || x.count > c.tile_out || x.phase < 0 || x.phase >= U) { EXPECT(false, "rate %d: tile count %d phase %d", rate, x.count, x.phase); return; }
                EXPECT(tile_span(r, x.count, x.phase) <= max_span(r), "rate %d: a span of %d frames", rate, tile_span(r, x.count, x.phase));
                for (int j = 0; j < x.count; j++) {
                    const long long m = m0 + j, pos = (long long)x.phase + (long long)j * D, i0 = m * D / U;
                    const long long first = T ? i0 - half + 1 : i0, lastf = T ? i0 + half : i0;
                    EXPECT(x.in0 + pos / U == first && pos % U == m * D % U, "rate %d output %lld: frame %lld phase %lld, want %lld %lld", rate, m, x.in0 + pos / U, pos % U, first, m * D % U);
                    // below the call's first frame only the history can serve (frames below 0 are zeros) ...
                    EXPECT(first < 0 || first >= n_abs - c.hist_before, "rate %d at %lld: output %lld reads frame %lld, the history begins at %lld", rate, n_abs, m, first, n_abs - c.hist_before);
                    // ... and no tap lies beyond what has arrived, unless the track is over (zeros)
                    EXPECT(last || lastf <= n_after - 1, "rate %d at %lld + %lld: output %lld reads frame %lld, which has not arrived", rate, n_abs, n, m, lastf);
                }
                m0 += x.count;
            }
        if (rate != 0) EXPECT(m0 == want_m, "rate %d at %lld + %lld: the tiles end at output %lld of %lld", rate, n_abs, n, m0, want_m);
        covered += want_m - m_exist;
        windows += c.windows;
        m_exist = want_m; held = c.held_after; hist = c.hist_after; n_abs = n_after;
        done = last;
    }
    // together: plan_convert's coverage of the whole track, and its windows
    long long want_out = total * U / D;
    if (want_out * D < total * U) want_out++;
    EXPECT(covered == want_out && m_exist == want_out && windows == (want_out + win - 1) / win && held == 0, "rate %d, %lld frames by %lld: %lld outputs in %lld windows, want %lld in %lld",
           rate, total, chunk, covered, windows, want_out, (want_out + win - 1) / win);
    if (rate != 0 && total > 0) {
        const Plan whole = plan_convert(total, r, nullptr, 0);
        EXPECT(whole.n_out == covered, "rate %d, %lld frames: plan_convert covers %lld outputs, the calls %lld", rate, total, whole.n_out, covered);
    }
}

static void check_everything()
{
    const int rates[] = {0, 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000};
    for (int rate : rates) {
        Ratio r;
        ratio_for(rate, r);
        const long long T = r.T, per_tile = (long long)tile_outputs(r) * r.D / r.U;
        const long long chunks[] = {1, T / 2 - 1, T / 2, T / 2 + 1, T - 1, T, per_tile - 1, per_tile, per_tile + 1};
        for (long long chunk : chunks) {
            if (chunk < 1) continue;
            const long long total = chunk == 1 ? 3 * T + 7 : std::max(3 * T + 7, 3 * chunk + 5);
            for (int win : {1, 64, 1001, 8000}) {
                check_track(rate, win, total, chunk, false);
                check_track(rate, win, total, chunk, true);
            }
        }
        check_track(rate, 64, 0, 5, true);                   // an empty track
        check_track(rate, 64, 1, 5, false);
        // far along: chunks past m D = 2^31 and 2^32 (44100: five and ten minutes), a minute at a time
        if (rate == 44100 || rate == 192000 || rate == 8000) check_track(rate, 8000, 700LL * rate, 60LL * rate + 17, false);
    }
    // the refusal
    {
        Ratio r;
        ratio_of(8000, r);
        g_calls += 2;
        const Continue a = plan_continue((1LL << 30) - 2, 1, false, r, 8000), b = plan_continue((1LL << 30) - 2, 2, true, r, 8000);
        EXPECT(a.refused == kOk, "2^31 - 2 output samples");
        EXPECT(b.refused == kTooLong && b.tiles.empty(), "2^31 output samples");
    }
}

int main(int argc, char** argv)
{
    if (argc == 1) {
        check_everything();
        std::printf("audio stream: %ld calls checked, %ld failures\n", g_calls, g_failures);
        return g_failures ? 1 : 0;
    }
    Ratio r;
    if (argc == 5 && std::strcmp(argv[1], "m") == 0) {
        if (!ratio_for(std::atoi(argv[2]), r)) return 2;
        std::printf("%lld\n", outputs_after(std::atoll(argv[3]), r, std::atoi(argv[4]) != 0));
        return 0;
    }
    if (argc == 7 && std::strcmp(argv[1], "plan") == 0) {
        if (!ratio_for(std::atoi(argv[2]), r)) return 2;
        const int win = std::atoi(argv[3]);
        const long long before = std::atoll(argv[4]), n = std::atoll(argv[5]);
        if (win < 1 || before < 0 || n < 0) return 2;
        const Continue c = plan_continue(before, n, std::atoi(argv[6]) != 0, r, win);
        std::printf("refused %d m_before %lld m_after %lld held_before %d held_after %d hist_before %d hist_after %d windows %lld analysed %lld tile_out %d ntiles %zu\n", c.refused,
                    c.m_before, c.m_after, c.held_before, c.held_after, c.hist_before, c.hist_after, c.windows, c.analysed, c.tile_out, c.tiles.size());
        std::printf("tiles");
        if (c.tiles.size() <= 64)
            for (const Tile& t : c.tiles) std::printf(" %lld:%lld:%d:%d", t.in0, t.out0, t.count, t.phase);
        else
            for (size_t i : {(size_t)0, c.tiles.size() - 1}) std::printf(" %lld:%lld:%d:%d", c.tiles[i].in0, c.tiles[i].out0, c.tiles[i].count, c.tiles[i].phase);
        std::printf("\n");
        return 0;
    }
    return 2;
}
