// Stand-alone check of csrc/avd_audio_plan.h (the tracks, window table, table arena and buffer sizes of one avd_audio_features call), built with
// the address and undefined-behaviour sanitizers by tests/audio_plan_kit.py and run as a program.  AUDIO_PLAN_HEADER names the header under
// test: the library's own, or a mutated copy that this program must reject.
//
//   audio_plan_check                          every check; prints "audio plan: N plans checked, F failures", status 1 if F > 0
//   audio_plan_check n win max_windows cut*   prints that call's plan
//
// What a plan is compared with is written out again here from the rule in include/avd.h (option "audio_cut"), sample by sample: nothing below
// calls the header to learn what the header should say.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>
#include AUDIO_PLAN_HEADER

using namespace avd_audio;

static long g_plans = 0, g_failures = 0;

#define EXPECT(cond, ...)                                                                                     \
    do {                                                                                                      \
        if (!(cond)) {                                                                                        \
            if (g_failures++ < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                     \
    } while (0)

// the rule, per sample: track_of[i] = cuts at or below i; inside a track, sample j of it lies in the track's window j / win
static void check_plan(long long n, int win, const std::vector<int>& cuts)
{
    g_plans++;
    const Plan p = plan_call(n, win, cuts.data(), (int)cuts.size(), kMaxWindows);
    EXPECT(p.refused == kOk, "n=%lld win=%d", n, win);
    if (p.refused) return;
    const int ntracks = (int)cuts.size() + 1;
    EXPECT((int)p.tracks.size() == ntracks, "n=%lld win=%d: %zu tracks", n, win, p.tracks.size());
    if ((int)p.tracks.size() != ntracks) return;
    // tracks and windows from the rule
    std::vector<long long> begin(ntracks), end(ntracks);
    int first = 0;
    std::map<int, int> want_sets;                 // short length -> 1
    std::vector<Window> want;
    for (int t = 0; t < ntracks; t++) {
        begin[t] = t ? cuts[t - 1] : 0;
        end[t] = t + 1 < ntracks ? cuts[t] : n;
        const long long len = end[t] - begin[t];
        const int count = (int)((len + win - 1) / win);
        const int last = (int)(len - (long long)(count - 1) * win);
        EXPECT(p.tracks[t].first == first && p.tracks[t].count == count && p.tracks[t].last == last, "n=%lld win=%d track %d: %d %d %d, want %d %d %d", n, win, t,
               p.tracks[t].first, p.tracks[t].count, p.tracks[t].last, first, count, last);
        for (int j = 0; j < count; j++) {
            const long long off = begin[t] + (long long)j * win;
            const int l = (int)((end[t] - off) < win ? (end[t] - off) : win);
            want.push_back(Window{off, l, 0});
            if (l != win) want_sets[l] = 1;
        }
        first += count;
    }
    EXPECT(p.nwin() == (int)want.size(), "n=%lld win=%d: %d windows, want %zu", n, win, p.nwin(), want.size());
    if (p.nwin() != (int)want.size()) return;
    for (int w = 0; w < p.nwin(); w++)
        EXPECT(p.windows[w].off == want[w].off && p.windows[w].len == want[w].len, "n=%lld win=%d window %d: off %lld len %d, want %lld %d", n, win, w,
               p.windows[w].off, p.windows[w].len, want[w].off, want[w].len);
    // every sample lies in exactly one window, and that window belongs to the sample's own track
    if (n <= 100000) {
        std::vector<int> hits((size_t)n, 0), owner((size_t)n, -1);
        for (int w = 0; w < p.nwin(); w++)
            for (long long i = p.windows[w].off; i < p.windows[w].off + p.windows[w].len && i >= 0 && i < n; i++) { hits[(size_t)i]++; owner[(size_t)i] = w; }
        int t = 0;
        for (long long i = 0; i < n; i++) {
            while (i >= end[t]) t++;
            const int w = owner[(size_t)i];
            EXPECT(hits[(size_t)i] == 1, "n=%lld win=%d: sample %lld lies in %d windows", n, win, i, hits[(size_t)i]);
            EXPECT(w >= p.tracks[t].first && w < p.tracks[t].first + p.tracks[t].count, "n=%lld win=%d: sample %lld of track %d lies in window %d", n, win, i, t, w);
            if (w >= 0) EXPECT((i - begin[t]) / win == w - p.tracks[t].first, "n=%lld win=%d: sample %lld is not in its track's window %lld", n, win, i, (i - begin[t]) / win);
        }
    }
    // the arena: one set per DISTINCT short length, none for the full length, sets side by side
    EXPECT(p.lengths.size() == want_sets.size() && p.set_at.size() == p.lengths.size(), "n=%lld win=%d: %zu sets, want %zu", n, win, p.lengths.size(), want_sets.size());
    std::set<int> seen;
    size_t at = 0;
    for (size_t k = 0; k < p.lengths.size() && k < p.set_at.size(); k++) {
        EXPECT(want_sets.count(p.lengths[k]) && seen.insert(p.lengths[k]).second, "n=%lld win=%d: set %zu has length %d", n, win, k, p.lengths[k]);
        EXPECT((size_t)p.set_at[k] == at, "n=%lld win=%d: set %zu at %d, want %zu", n, win, k, p.set_at[k], at);
        at += 3 * (size_t)p.lengths[k];
    }
    EXPECT(p.arena == at, "n=%lld win=%d: arena %zu, want %zu", n, win, p.arena, at);
    for (int w = 0; w < p.nwin(); w++) {
        const Window& x = p.windows[w];
        if (x.len == win) { EXPECT(x.tab == kTabFull, "n=%lld win=%d window %d: a full window with set %d", n, win, w, x.tab); continue; }
        size_t k = 0;
        while (k < p.lengths.size() && p.lengths[k] != x.len) k++;
        EXPECT(k < p.lengths.size() && x.tab == p.set_at[k] && x.tab >= 0 && (size_t)x.tab + 3 * (size_t)x.len <= p.arena, "n=%lld win=%d window %d: set %d", n, win, w, x.tab);
    }
    // the two lists: every window in exactly one, ascending; the 80 x 100 path takes full windows of kFftLen samples only
    std::vector<int> in_list((size_t)p.nwin(), 0);
    int longest = 0;
    for (size_t k = 0; k < p.fft.size(); k++) {
        const int w = p.fft[k];
        EXPECT(w >= 0 && w < p.nwin() && (k == 0 || p.fft[k - 1] < w), "fft list entry %zu = %d", k, w);
        if (w >= 0 && w < p.nwin()) { in_list[(size_t)w]++; EXPECT(p.windows[w].len == kFftLen && win == kFftLen, "window %d of length %d on the 80 x 100 path", w, p.windows[w].len); }
    }
    for (size_t k = 0; k < p.dft.size(); k++) {
        const int w = p.dft[k];
        EXPECT(w >= 0 && w < p.nwin() && (k == 0 || p.dft[k - 1] < w), "dft list entry %zu = %d", k, w);
        if (w >= 0 && w < p.nwin()) { in_list[(size_t)w]++; EXPECT(!(p.windows[w].len == kFftLen && win == kFftLen), "a full window %d on the direct path", w); if (p.windows[w].len > longest) longest = p.windows[w].len; }
    }
    for (int w = 0; w < p.nwin(); w++) EXPECT(in_list[(size_t)w] == 1, "n=%lld win=%d: window %d is in %d lists", n, win, w, in_list[(size_t)w]);
    EXPECT(p.max_dft_len == longest, "n=%lld win=%d: max_dft_len %d, want %d", n, win, p.max_dft_len, longest);
    // sizes: scratch in doubles, the upload in bytes, its parts side by side and aligned for what they hold
    const size_t nw = (size_t)p.nwin();
    EXPECT(p.xw_size() == nw * (size_t)win && p.mag_size() == nw * (size_t)(win / 2 + 1) && p.b_size() == p.fft.size() * 16000u, "n=%lld win=%d: scratch sizes", n, win);
    EXPECT(p.windows_at() == 8 * p.arena && p.fft_at() == p.windows_at() + 16 * nw && p.dft_at() == p.fft_at() + 4 * p.fft.size(), "n=%lld win=%d: upload offsets", n, win);
    EXPECT(p.upload_bytes() >= p.dft_at() + 4 * p.dft.size() && p.upload_bytes() < p.dft_at() + 4 * p.dft.size() + 8 && p.upload_bytes() % 8 == 0, "n=%lld win=%d: upload bytes %zu", n, win, p.upload_bytes());
    EXPECT(p.windows_at() % 8 == 0 && p.fft_at() % 4 == 0 && p.dft_at() % 4 == 0, "n=%lld win=%d: alignment", n, win);
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
    // every call of up to 10 samples, every set of cuts, window lengths around and above the track lengths
    for (int win : {1, 2, 3, 4, 5, 8})
        for (int n = 1; n <= 10; n++)
            for (unsigned m = 0; m < (1u << (n - 1)); m++) {
                std::vector<int> cuts;
                for (int c = 1; c < n; c++) if (m & (1u << (c - 1))) cuts.push_back(c);
                check_plan(n, win, cuts);
            }
    // the 80 x 100 path's window length: full windows only, shorter than a window, one sample, a repeated short length, L % 4 = 0 ... 3
    {
        const std::vector<long long> lens = {16037, 8000, 5, 1, 12000, 7999, 8001, 12000, 16002};
        const std::vector<int> cuts = cuts_of(lens);
        check_plan(sum_of(lens), 8000, cuts);
        const Plan p = plan_call(sum_of(lens), 8000, cuts.data(), (int)cuts.size(), kMaxWindows);
        const std::vector<int> want = {37, 5, 1, 4000, 7999, 2};              // in order of first appearance; 8000 has none, 1 and 4000 serve two tracks each
        EXPECT(p.lengths == want, "the distinct short lengths: %zu of them", p.lengths.size());
        EXPECT(p.nwin() == 16 && p.nfull() == 8, "%d windows, %d full", p.nwin(), p.nfull());
        EXPECT(p.windows[7].tab == p.windows[12].tab && p.windows[7].len == 4000, "the two tracks of 12000 samples share one set");      // windows 7 and 12: their last
        EXPECT(p.windows[5].tab == p.windows[10].tab && p.windows[5].len == 1, "the one-sample track and the last window of 8001 share one set");
        EXPECT(p.windows[3].tab == kTabFull && p.tracks[1].count == 1 && p.tracks[1].last == 8000, "a track of one full window has no set");
        check_plan(2 * 8000, 8000, {});                                       // a multiple of win: no arena at all
        const Plan q = plan_call(2 * 8000, 8000, nullptr, 0, kMaxWindows);
        EXPECT(q.arena == 0 && q.lengths.empty() && q.dft.empty() && q.nfull() == 2, "two full windows need no set");
    }
    check_plan(2500 + 1001 + 3 + 2002, 1001, cuts_of({2500, 1001, 3, 2002}));
    // sizes at 1 and at 64 tracks, at win = 1 and win = 8192
    for (int win : {1, 8192})
        for (int ntracks : {1, 64}) {
            std::vector<long long> lens;
            for (int t = 0; t < ntracks; t++) lens.push_back(win == 1 ? 1 + t % 3 : 8192 + 100 + t);       // win = 8192: 64 distinct short lengths
            const std::vector<int> cuts = cuts_of(lens);
            check_plan(sum_of(lens), win, cuts);
            const Plan p = plan_call(sum_of(lens), win, cuts.data(), (int)cuts.size(), kMaxWindows);
            if (win == 1) EXPECT(p.arena == 0 && p.xw_size() == (size_t)sum_of(lens) && p.mag_size() == p.xw_size(), "win = 1: every window is full");
            else {
                size_t arena = 0;
                for (int t = 0; t < ntracks; t++) arena += 3 * (size_t)(100 + t);
                EXPECT(p.arena == arena && p.nwin() == 2 * ntracks && p.xw_size() == (size_t)2 * ntracks * 8192 && p.mag_size() == (size_t)2 * ntracks * 4097 && p.b_size() == 0,
                       "win = 8192, %d tracks: arena %zu", ntracks, p.arena);
                EXPECT(p.upload_bytes() == 8 * arena + 16 * (size_t)p.nwin() + 4 * (size_t)p.nwin(), "win = 8192, %d tracks: upload %zu bytes", ntracks, p.upload_bytes());
            }
        }
    {   // the widest arena: 64 tracks, each ending in a short length of its own just under 8192
        std::vector<long long> lens;
        for (int t = 0; t < 64; t++) lens.push_back(8191 - t);
        check_plan(sum_of(lens), 8192, cuts_of(lens));
    }
    // refusals, in order: a cut at or beyond the buffer first, then the windows array
    {
        const int c1[] = {5, 10}, c2[] = {5, 11}, c3[] = {5, 9};
        g_plans += 6;
        EXPECT(plan_call(10, 4, c1, 2, 100).refused == kCutBeyond, "a cut at n");
        EXPECT(plan_call(10, 4, c2, 2, 0).refused == kCutBeyond, "a cut beyond n wins over a small windows array");
        EXPECT(plan_call(10, 4, c3, 2, 5).refused == kOk, "cuts 5, 9 of 10 samples are 2 + 1 + 1 windows ... and 5 is room enough");
        EXPECT(plan_call(10, 4, c3, 2, 4).refused == kOk && plan_call(10, 4, c3, 2, 3).refused == kWindowsTooSmall, "... 4 is exactly enough, 3 is not although ceil(10 / 4) = 3");
        const Plan r = plan_call(10, 4, c3, 2, 3);
        EXPECT(r.windows.empty() && r.tracks.empty() && r.arena == 0 && r.fft.empty() && r.dft.empty(), "a refused plan holds nothing");
        EXPECT(plan_call((long long)kMaxWindows + 1, 1, nullptr, 0, (long long)kMaxWindows + 1).refused == kWindowsTooSmall, "more than 2^24 windows");
    }
}

int main(int argc, char** argv)
{
    if (argc == 1) {
        check_everything();
        std::printf("audio plan: %ld plans checked, %ld failures\n", g_plans, g_failures);
        return g_failures ? 1 : 0;
    }
    if (argc < 4) return 2;
    const long long n = std::atoll(argv[1]), max_windows = std::atoll(argv[3]);
    const int win = std::atoi(argv[2]);
    std::vector<int> cuts;
    for (int i = 4; i < argc; i++) cuts.push_back(std::atoi(argv[i]));
    if (n < 1 || win < 1 || win > kMaxWin || (int)cuts.size() > kMaxCuts) return 2;
    const Plan p = plan_call(n, win, cuts.data(), (int)cuts.size(), max_windows);
    std::printf("refused %d nwin %d nfull %d arena %zu max_dft_len %d upload_bytes %zu\n", p.refused, p.nwin(), p.nfull(), p.arena, p.max_dft_len, p.upload_bytes());
    std::printf("tracks");
    for (const Track& t : p.tracks) std::printf(" %d:%d:%d", t.first, t.count, t.last);
    std::printf("\nwindows");
    for (const Window& w : p.windows) std::printf(" %lld:%d:%d", w.off, w.len, w.tab);
    std::printf("\nlengths");
    for (int l : p.lengths) std::printf(" %d", l);
    std::printf("\n");
    return 0;
}
