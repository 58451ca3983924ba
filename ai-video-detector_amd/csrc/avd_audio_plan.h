// What one avd_audio_features call runs over: its tracks (option "audio_cut", include/avd.h), the window table its kernels go by, the distinct
// short window lengths with their place in the table arena, and the buffer sizes.  Plain host code over the standard library only: the library
// (avd_capi.hip, avd_audio.hip) and a stand-alone check program (tests/audio_plan_check.cpp) include it.  No table VALUE is formed here: the
// Hann / cosine / sine entries are built in avd_audio.hip, by one function for every length.
//
// With cuts c1 < ... < ck the buffer of n samples is k + 1 tracks [0, c1), [c1, c2), ..., [ck, n).  Each track is windowed from ITS OWN start:
// ceil(n_t / win) windows, the last one shorter when win does not divide n_t.  The windows of the call are numbered track after track:
//
//     track 0: |---win---|---win---|-last0-|   track 1: |---win---|-last1-|   ...
//     window        0         1        2                     3        4
//
// A window of `win` samples reads the full-length tables (cached per win on the device); every other length L reads a set of its own,
// hann[L] | cos[L] | sin[L], at Window::tab in the arena.  Tracks that end in the same short length share one set.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace avd_audio {

constexpr int kMaxCuts = 63, kMaxTracks = kMaxCuts + 1;
constexpr int kMaxWin = 8192;
constexpr int kFftLen = 8000;                    // full windows of this length take the 80 x 100 transform, everything else the direct sum
constexpr int kTabFull = -1;                     // Window::tab of a full window
constexpr long long kMaxWindows = 1 << 24;

enum Refusal { kOk = 0, kCutBeyond = 1, kWindowsTooSmall = 2 };   // in the order they are checked

struct Window { long long off; int len; int tab; };   // first sample in the staged buffer, samples, first double of the length's set in the arena (kTabFull: none)
struct Track { int first, count, last; };             // first window, windows, length of the last window: a row of debug buffer "audio_tracks"
static_assert(sizeof(Window) == 16 && sizeof(Track) == 12, "the window table is uploaded, the track rows are fetched, as they are");

struct Plan {
    int refused = kOk;
    int win = 0;
    std::vector<Track> tracks;
    std::vector<Window> windows;                 // [nwin]
    std::vector<int> fft, dft;                   // window numbers: the full kFftLen windows, and all the others
    std::vector<int> lengths, set_at;            // the distinct short lengths in order of first appearance, and each one's first double in the arena
    size_t arena = 0;                            // doubles: 3 * the sum of `lengths`
    int max_dft_len = 0;                         // the longest window of `dft`
    int nwin() const { return (int)windows.size(); }
    int nfull() const { return (int)fft.size(); }
    // scratch (doubles): xw [nwin][win] | mag [nwin][win / 2 + 1] | the 80 x 100 path's intermediate [nfull][kFftLen] complex
    size_t xw_size() const { return windows.size() * (size_t)win; }
    size_t mag_size() const { return windows.size() * (size_t)(win / 2 + 1); }
    size_t b_size() const { return fft.size() * (size_t)kFftLen * 2; }
    // the per-call upload, ONE copy (bytes; every part 8-byte aligned but the two lists, which are ints): arena | windows | fft | dft
    size_t windows_at() const { return arena * sizeof(double); }
    size_t fft_at() const { return windows_at() + windows.size() * sizeof(Window); }
    size_t dft_at() const { return fft_at() + fft.size() * sizeof(int); }
    size_t upload_bytes() const { return (dft_at() + dft.size() * sizeof(int) + 7) / 8 * 8; }
};

// n > 0 samples, 1 <= win <= kMaxWin, ncuts <= kMaxCuts strictly ascending positive cuts (what "audio_cut" accepted).  A refused plan holds nothing.
inline Plan plan_call(long long n, int win, const int* cuts, int ncuts, long long max_windows)
{
    Plan p;
    p.win = win;
    for (int c = 0; c < ncuts; c++)
        if (cuts[c] >= n) { p.refused = kCutBeyond; return p; }
    long long total = 0;
    for (int t = 0; t <= ncuts; t++) {
        const long long begin = t == 0 ? 0 : cuts[t - 1], end = t == ncuts ? n : cuts[t];
        total += (end - begin + win - 1) / win;
    }
    if (total > max_windows || total > kMaxWindows) { p.refused = kWindowsTooSmall; return p; }
    p.windows.reserve((size_t)total);
    for (int t = 0; t <= ncuts; t++) {
        const long long begin = t == 0 ? 0 : cuts[t - 1], end = t == ncuts ? n : cuts[t];
        Track tr{p.nwin(), 0, 0};
        for (long long s = begin; s < end;) {
            const long long stop = std::min(end, s + (long long)win);
            const int len = (int)(stop - s);
            int tab = kTabFull;
            if (len != win) {
                size_t k = 0;
                while (k < p.lengths.size() && p.lengths[k] != len) k++;
                if (k == p.lengths.size()) {
                    p.lengths.push_back(len);
                    p.set_at.push_back((int)p.arena);
                    p.arena += 3 * (size_t)len;
                }
                tab = p.set_at[k];
            }
            const int w = p.nwin();
            if (len == win && win == kFftLen) p.fft.push_back(w);
            else { p.dft.push_back(w); p.max_dft_len = std::max(p.max_dft_len, len); }
            p.windows.push_back(Window{s, len, tab});
            tr.count++;
            tr.last = len;
            s = stop;
        }
        p.tracks.push_back(tr);
    }
    return p;
}

}  // namespace avd_audio
