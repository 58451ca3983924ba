// Several continued tracks in one avd_audio_features call (option "audio_track_slot", include/avd.h): what ONE such call runs over.  Plain host
// code over the standard library and the three audio headers, in their manner: the library and a stand-alone check program
// (tests/audio_map_check.cpp) include it.
//
// The call's buffer holds t tracks (option "audio_cut"); entry i of the list says what track i is: a whole track, or the continuation of audio
// slot k, possibly its end.  Every track is planned by plan_continue (avd_audio_stream.h) -- a whole track is plan_continue(0, n_t, last = true),
// which is plan_convert's coverage of it -- and gets a region of the analyzer's buffer of its own:
//
//     analyzer's buffer   |held 0|---- new 0 ----|..|held 1|-- new 1 --|..|------ new 2 ------|      (.. : a region begins at a multiple of 8 entries)
//     windows             |--win--|--win--|-held-|  |--win--|-held back-|  |--win--|--win--|last|     numbered track after track
//
// so one window table (avd_audio::Plan) serves the analyzer's kernels as they are, one tile table the converter -- each tile with the index of its
// track, each track with a source row: where its chunk begins in the call's buffer, the frames its slot absorbed before, and its history -- one
// gather list the launch that brings held samples (and, unconverted, the call's own) into the regions, and one save list the launch that leaves
// every continued track's new history and remainder in its slot.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>
#include "avd_audio_plan.h"
#include "avd_audio_resample.h"
#include "avd_audio_stream.h"

namespace avd_audio_map {

constexpr int kMaxEntries = avd_audio::kMaxTracks;   // 64 tracks per call, as under "audio_cut"
constexpr int kSlots = 8;                            // the audio slots; a slot appears at most once in a list, so at most 8 tracks continue
constexpr int kSlotMask = 0xF, kEndBit = 0x10;       // an entry: slot | kEndBit
constexpr int kRegionAlign = 8;                      // entries: the converter's 16-byte rows of two tracks never share a row
constexpr int kMaxGather = 2 * kSlots + (kMaxEntries - kSlots);   // held + own samples of 8 continued tracks, own samples of 56 whole ones

// what the option accepts as ONE entry (the list's own state -- a slot twice, a 65th entry -- is the library's to check)
inline bool entry_ok(int v) { return v >= 0 && (v & ~(kSlotMask | kEndBit)) == 0 && (v & kSlotMask) <= kSlots && !((v & kEndBit) && (v & kSlotMask) == 0); }

// numbered as include/avd.h lists the refusals of a list call (1: the argument checks, 2: alignment -- both the library's, ahead of the plan)
// kTooLong names a track (Plan::refused_track), or with track -1 the analyzer's buffer of all tracks together; kTooManyWindows is decided where
// kWindowsTooSmall is; kSlotState is no caller's fault: the state handed in contradicts the rule
enum Refusal { kOk = 0, kCutBeyond = 3, kEndPending = 4, kEntryCount = 5, kSlotBinding = 6, kTooLong = 7, kWindowsTooSmall = 8, kTooManyWindows = 9, kSlotState = 10 };

// a slot as the call finds it.  same: win, rate, channels and format of the call are those of the slot's first call (read only while frames > 0).
// held and hist are what the slot's memory holds; plan_map holds them to the rule (kSlotState), since the gather and the converter read that many
struct SlotState { long long frames = 0; int held = 0; int hist = 0; bool same = true; };

struct Track {
    int slot = 0;                                // 0: a whole track
    bool last = true;                            // a whole track, or a continued one that ends here
    long long begin = 0, n = 0;                  // its frames in the call's buffer
    avd_resample::Continue c;                    // plan_continue's, tiles included (positions relative to the track and to its region)
    long long region = 0;                        // first entry of [held | new] in the analyzer's buffer; c.held_before + c.fresh() entries
    int first = 0, count = 0;                    // its records in the call's array
    long long extent() const { return c.held_before + c.fresh(); }
};
// a row of the converter's source table, uploaded as it is.  hist: device address of the history of slot `slot`, which the library fills in
// from this row
struct Source { long long at; long long chunk0; unsigned long long hist; int hist_n; int slot; };
static_assert(sizeof(Source) == 32, "the source rows are uploaded as they are");
// one move of the gather launch, in entries of the analysis type: held = the slot's held samples -> the front of the region; else the call's
// own samples from `src` of its buffer -> behind them
struct Copy { int track; bool held; long long src, dst, count; };
// what the save launch leaves in a slot: hist_new frames of history out of the track's n frames and hist_old old ones (n = 0 for an unconverted
// track, which keeps none), and `held` entries of the analyzer's buffer from held_src on
struct Save { int track, slot; long long n; int hist_old, hist_new; long long held_src; int held; };

struct Plan {
    int refused = kOk;
    int refused_track = -1;                      // the track a refusal 6 or 7 names
    std::vector<Track> tracks;
    avd_audio::Plan windows;                     // over the regions; windows.tracks has a row per track, count 0 included
    std::vector<avd_resample::Tile> tiles;       // out0 counts from the start of the analyzer's buffer
    std::vector<int> tile_track;                 // [tiles]
    std::vector<Source> sources;                 // [tracks]
    std::vector<Copy> gather;
    std::vector<Save> saves;
    long long total = 0;                         // entries of the analyzer's buffer
    long long records = 0, fresh = 0;            // of all tracks
    int continued = 0;
};

// the windows of one track, appended to `p` exactly as avd_audio::plan_call forms them: `analysed` samples from `at` on
inline void append_windows(avd_audio::Plan& p, long long at, long long analysed)
{
    avd_audio::Track tr{p.nwin(), 0, 0};
    for (long long s = at; s < at + analysed;) {
        const long long stop = std::min(at + analysed, s + (long long)p.win);
        const int len = (int)(stop - s);
        int tab = avd_audio::kTabFull;
        if (len != p.win) {
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
        if (len == p.win && p.win == avd_audio::kFftLen) p.fft.push_back(w);
        else { p.dft.push_back(w); p.max_dft_len = std::max(p.max_dft_len, len); }
        p.windows.push_back(avd_audio::Window{s, len, tab});
        tr.count++;
        tr.last = len;
        s = stop;
    }
    p.tracks.push_back(tr);
}

// n >= 0 frames, 1 <= win <= kMaxWin, ncuts strictly ascending positive cuts in frames (what "audio_cut" accepted), nentries entries that
// entry_ok accepted with no slot twice (what "audio_track_slot" accepted), slots[k - 1] the state of audio slot k, r the call's ratio
// (identity_ratio() for "audio_rate" 0), channels the samples per frame of the call's buffer.  end_pending: option "audio_end" was set;
// have_windows: the caller passed a records array.  A refused plan holds nothing but the refusal.
inline Plan plan_map(long long n, int win, const int* cuts, int ncuts, const int* entries, int nentries, const SlotState* slots, const avd_resample::Ratio& r,
                     int channels, long long max_windows, bool have_windows, bool end_pending)
{
    Plan p;
    auto refuse = [&p](int why, int track) { p = Plan{}; p.refused = why; p.refused_track = track; return p; };
    for (int c = 0; c < ncuts; c++)
        if (cuts[c] >= n) return refuse(kCutBeyond, -1);
    if (end_pending) return refuse(kEndPending, -1);
    if (nentries != ncuts + 1) return refuse(kEntryCount, -1);
    for (int t = 0; t < nentries; t++) {
        const int slot = entries[t] & kSlotMask;
        if (slot && slots[slot - 1].frames > 0 && !slots[slot - 1].same) return refuse(kSlotBinding, t);
    }
    p.windows.win = win;
    for (int t = 0; t < nentries; t++) {
        Track tr;
        tr.slot = entries[t] & kSlotMask;
        tr.last = tr.slot == 0 || (entries[t] & kEndBit) != 0;
        tr.begin = t == 0 ? 0 : cuts[t - 1];
        tr.n = (t == ncuts ? n : cuts[t]) - tr.begin;
        tr.c = avd_resample::plan_continue(tr.slot ? slots[tr.slot - 1].frames : 0, tr.n, tr.last, r, win);
        if (tr.c.refused) return refuse(kTooLong, t);
        if (tr.slot && (tr.c.held_before != slots[tr.slot - 1].held || tr.c.hist_before != slots[tr.slot - 1].hist)) return refuse(kSlotState, t);
        tr.region = p.total;
        p.total = (tr.region + tr.extent() + kRegionAlign - 1) / kRegionAlign * kRegionAlign;
        if (p.total > avd_resample::kMaxOutputs) return refuse(kTooLong, -1);
        tr.first = (int)p.records;
        tr.count = (int)tr.c.windows;
        p.records += tr.c.windows;
        p.fresh += tr.c.fresh();
        p.continued += tr.slot != 0;
        p.tracks.push_back(std::move(tr));
    }
    if (p.records > max_windows || (p.records > 0 && !have_windows)) return refuse(kWindowsTooSmall, -1);
    if (p.records > avd_audio::kMaxWindows) return refuse(kTooManyWindows, -1);
    p.windows.windows.reserve((size_t)p.records);
    for (int t = 0; t < nentries; t++) {
        const Track& tr = p.tracks[(size_t)t];
        const avd_resample::Continue& c = tr.c;
        append_windows(p.windows, tr.region, c.analysed);
        for (avd_resample::Tile tile : c.tiles) {
            tile.out0 += tr.region;
            p.tiles.push_back(tile);
            p.tile_track.push_back(t);
        }
        p.sources.push_back(Source{tr.begin * channels, c.n_before, 0ULL, c.hist_before, tr.slot});
        if (c.held_before) p.gather.push_back(Copy{t, true, 0, tr.region, c.held_before});
        if (r.rate == 0 && tr.n > 0) p.gather.push_back(Copy{t, false, tr.begin, tr.region + c.held_before, tr.n});
        if (tr.slot && !tr.last) p.saves.push_back(Save{t, tr.slot, r.rate ? tr.n : 0, c.hist_before, c.hist_after, tr.region + c.analysed, c.held_after});
    }
    return p;
}

}  // namespace avd_audio_map
