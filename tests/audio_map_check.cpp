// Stand-alone check of csrc/avd_audio_map.h (what ONE avd_audio_features call with an "audio_track_slot" list runs over: several tracks, each a
// whole one or the continuation of an audio slot), built with the address and undefined-behaviour sanitizers by tests/audio_map_kit.py and run as a
// program.  AUDIO_MAP_HEADER names the header under test: the library's own, or a mutated copy that this program must reject.
//
//   audio_map_check                                          every check; prints "audio map: N calls checked, F failures", status 1 if F > 0
//   audio_map_check plan RATE WIN N CUTS ENTRIES FRAMES MAXW  prints that call's plan; CUTS / ENTRIES / FRAMES (of slots 1 ... 8) are comma lists, "-" is empty
//
// What a plan is compared with comes from plan_continue (avd_audio_stream.h, which tests/audio_stream_check.cpp holds to the rule output by output)
// and from the layout include/avd.h states: a region [held | new] per track, windows inside the analysed part of one region, a source row per track.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include AUDIO_MAP_HEADER

using namespace avd_audio_map;
using avd_resample::Continue;
using avd_resample::Ratio;
using avd_resample::Tile;

static long g_calls = 0, g_failures = 0;

#define EXPECT(cond, ...)                                                                                     \
    do {                                                                                                      \
        if (!(cond)) {                                                                                        \
            if (g_failures++ < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                     \
    } while (0)

static bool ratio_for(int rate, Ratio& r)
{
    if (rate == 0) { r = avd_resample::identity_ratio(); return true; }
    return avd_resample::ratio_of(rate, r);
}

struct Want { int entry; long long n; };                      // a track of the call: its list entry and its frames

// one call: `tracks` side by side in the buffer, the slots as `state` says
static void check_call(int rate, int win, int channels, const std::vector<Want>& tracks, const SlotState* state)
{
    Ratio r;
    if (!ratio_for(rate, r)) { EXPECT(false, "rate %d", rate); return; }
    g_calls++;
    std::vector<int> cuts, entries;
    long long n = 0;
    for (size_t t = 0; t < tracks.size(); t++) {
        if (t) cuts.push_back((int)n);
        n += tracks[t].n;
        entries.push_back(tracks[t].entry);
    }
    const Plan p = plan_map(n, win, cuts.data(), (int)cuts.size(), entries.data(), (int)entries.size(), state, r, channels, 1 << 24, true, false);
    EXPECT(p.refused == kOk, "rate %d win %d: refused %d", rate, win, p.refused);
    if (p.refused) return;
    const size_t nt = tracks.size();
    EXPECT(p.tracks.size() == nt && p.sources.size() == nt && p.windows.tracks.size() == nt && p.tiles.size() == p.tile_track.size(), "rate %d: %zu tracks, %zu rows, %zu window rows",
           rate, p.tracks.size(), p.sources.size(), p.windows.tracks.size());
    if (p.tracks.size() != nt || p.sources.size() != nt || p.windows.tracks.size() != nt || p.tiles.size() != p.tile_track.size()) return;
    long long begin = 0, records = 0, fresh = 0, region_end = 0;
    size_t tile_at = 0, gather_at = 0, save_at = 0;
    int continued = 0;
    for (size_t t = 0; t < nt; t++) {
        const Track& tr = p.tracks[t];
        const int slot = tracks[t].entry & 15;
        const bool last = slot == 0 || (tracks[t].entry & 16);
        const long long before = slot ? state[slot - 1].frames : 0;
        const Continue c = avd_resample::plan_continue(before, tracks[t].n, last, r, win);
        continued += slot != 0;
        // the track's Continue is plan_continue's
        EXPECT(tr.slot == slot && tr.last == last && tr.begin == begin && tr.n == tracks[t].n, "track %zu: slot %d last %d frames [%lld, + %lld)", t, tr.slot, (int)tr.last, tr.begin, tr.n);
        EXPECT(tr.c.n_before == c.n_before && tr.c.n_after == c.n_after && tr.c.m_before == c.m_before && tr.c.m_after == c.m_after && tr.c.held_before == c.held_before &&
               tr.c.held_after == c.held_after && tr.c.hist_before == c.hist_before && tr.c.hist_after == c.hist_after && tr.c.windows == c.windows && tr.c.analysed == c.analysed &&
               tr.c.tiles.size() == c.tiles.size(), "track %zu: its Continue is not plan_continue(%lld, %lld, %d)", t, before, tracks[t].n, (int)last);
        if (slot) EXPECT(c.held_before == state[slot - 1].held && c.hist_before == state[slot - 1].hist, "track %zu: the state table of the check holds %d / %d, the rule %d / %d", t,
                         state[slot - 1].held, state[slot - 1].hist, c.held_before, c.hist_before);
        // regions: in order, apart, [held | new]
        const long long extent = c.held_before + c.fresh();
        EXPECT(tr.region >= region_end && tr.region % kRegionAlign == 0 && tr.extent() == extent, "track %zu: region at %lld of %lld entries, the one before ends at %lld", t, tr.region,
               tr.extent(), region_end);
        region_end = tr.region + extent;
        EXPECT(region_end <= p.total, "track %zu: its region ends at %lld, the buffer at %lld", t, region_end, p.total);
        // the gather list: held samples to the front, an unconverted track's own behind them
        if (c.held_before) {
            const bool ok = gather_at < p.gather.size() && p.gather[gather_at].track == (int)t && p.gather[gather_at].held && p.gather[gather_at].dst == tr.region &&
                            p.gather[gather_at].count == c.held_before && p.gather[gather_at].src == 0;
            EXPECT(ok, "track %zu: %d held samples are not gathered to the front of its region", t, c.held_before);
            gather_at++;
        }
        if (rate == 0 && tracks[t].n > 0) {
            const bool ok = gather_at < p.gather.size() && p.gather[gather_at].track == (int)t && !p.gather[gather_at].held && p.gather[gather_at].dst == tr.region + c.held_before &&
                            p.gather[gather_at].count == tracks[t].n && p.gather[gather_at].src == begin;
            EXPECT(ok, "track %zu: its own %lld samples are not gathered behind the held ones", t, tracks[t].n);
            gather_at++;
        }
        // the windows: numbered track after track, every one inside the analysed part of this region
        const avd_audio::Track& wr = p.windows.tracks[t];
        EXPECT(tr.first == records && tr.count == c.windows && wr.first == records && wr.count == c.windows, "track %zu: records [%d, + %d), window row [%d, + %d), want [%lld, + %lld)", t,
               tr.first, tr.count, wr.first, wr.count, records, c.windows);
        long long at = tr.region;
        for (int w = wr.first; w < wr.first + wr.count && w < p.windows.nwin(); w++) {
            const avd_audio::Window& x = p.windows.windows[(size_t)w];
            EXPECT(x.off == at && x.len >= 1 && x.len <= win, "track %zu window %d: at %lld of %d samples, want it at %lld", t, w, x.off, x.len, at);
            EXPECT(x.off + x.len <= tr.region + c.analysed, "track %zu window %d: [%lld, %lld) runs over the analysed %lld samples of its region at %lld into what is held back or the next region",
                   t, w, x.off, x.off + x.len, c.analysed, tr.region);
            EXPECT((x.len == win) == (x.tab == avd_audio::kTabFull), "track %zu window %d: length %d tables %d", t, w, x.len, x.tab);
            at += x.len;
        }
        EXPECT(at == tr.region + c.analysed, "track %zu: its windows end at %lld, the analysed samples at %lld", t, at, tr.region + c.analysed);
        // the tiles: plan_continue's, moved to the region; each one's source row is this track's
        for (size_t k = 0; k < c.tiles.size(); k++, tile_at++) {
            if (tile_at >= p.tiles.size()) { EXPECT(false, "track %zu: tile %zu is missing", t, k); break; }
            const Tile &x = p.tiles[tile_at], &y = c.tiles[k];
            EXPECT(p.tile_track[tile_at] == (int)t, "tile %zu: track %d, want %zu", tile_at, p.tile_track[tile_at], t);
            EXPECT(x.in0 == y.in0 && x.begin == 0 && x.end == c.n_after && x.count == y.count && x.phase == y.phase && x.out0 == y.out0 + tr.region, "tile %zu of track %zu differs from plan_continue's",
                   tile_at, t);
            EXPECT(x.out0 >= tr.region + c.held_before && x.out0 + x.count <= region_end, "tile %zu: outputs [%lld, + %d) outside the new part of region %lld", tile_at, x.out0, x.count, tr.region);
        }
        const Source& s = p.sources[t];
        EXPECT(s.at == begin * channels && s.chunk0 == before && s.hist_n == c.hist_before && s.hist == 0, "track %zu: source row at %lld chunk0 %lld history %d", t, s.at, s.chunk0, s.hist_n);
        EXPECT(s.slot == slot, "track %zu continues slot %d and is handed the history of slot %d", t, slot, s.slot);
        // the save list: every continued track that does not end
        if (slot && !last) {
            const bool ok = save_at < p.saves.size() && p.saves[save_at].track == (int)t && p.saves[save_at].slot == slot && p.saves[save_at].n == (rate ? tracks[t].n : 0) &&
                            p.saves[save_at].hist_old == c.hist_before && p.saves[save_at].hist_new == c.hist_after && p.saves[save_at].held_src == tr.region + c.analysed &&
                            p.saves[save_at].held == c.held_after && p.saves[save_at].held_src + c.held_after == region_end;
            EXPECT(ok, "track %zu: slot %d is not saved as the rule says", t, slot);
            save_at++;
        }
        records += c.windows;
        fresh += c.fresh();
        begin += tracks[t].n;
    }
    EXPECT(tile_at == p.tiles.size() && gather_at == p.gather.size() && save_at == p.saves.size(), "%zu tiles, %zu moves, %zu saves beyond the tracks' own", p.tiles.size() - tile_at,
           p.gather.size() - gather_at, p.saves.size() - save_at);
    EXPECT(p.records == records && p.windows.nwin() == records && p.fresh == fresh && p.continued == continued && (int)p.gather.size() <= kMaxGather && (int)p.saves.size() <= kSlots,
           "rate %d: %lld records for %d windows, want %lld", rate, p.records, p.windows.nwin(), records);
    EXPECT(p.windows.fft.size() + p.windows.dft.size() == (size_t)records, "%zu + %zu windows in the two lists", p.windows.fft.size(), p.windows.dft.size());
    // a list of zeros over an unconverted buffer: the window table is plan_call's but for where the regions lie
    if (continued == 0 && rate == 0 && n > 0) {
        const avd_audio::Plan q = avd_audio::plan_call(n, win, cuts.data(), (int)cuts.size(), 1 << 24);
        bool same = q.nwin() == p.windows.nwin() && q.fft == p.windows.fft && q.dft == p.windows.dft && q.lengths == p.windows.lengths && q.set_at == p.windows.set_at &&
                    q.arena == p.windows.arena && q.max_dft_len == p.windows.max_dft_len;
        for (int w = 0; same && w < q.nwin(); w++) same = q.windows[(size_t)w].len == p.windows.windows[(size_t)w].len && q.windows[(size_t)w].tab == p.windows.windows[(size_t)w].tab;
        EXPECT(same, "win %d: a list of zeros does not window as the cut call does", win);
    }
}

// a slot that has absorbed `frames`: what the rule says it holds
static SlotState slot_after(long long frames, const Ratio& r, int win)
{
    SlotState s;
    s.frames = frames;
    s.held = (int)(avd_resample::outputs_after(frames, r, false) % win);
    s.hist = avd_resample::history_frames(frames, r);
    return s;
}

static void check_everything()
{
    const int rates[] = {0, 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000};
    for (int rate : rates) {
        Ratio r;
        ratio_for(rate, r);
        const long long T = r.T, per_tile = (long long)avd_resample::tile_outputs(r) * r.D / r.U;
        const int channels = rate == 0 ? 1 : 1 + (rate / 50) % 2;
        for (int win : {64, 1001, 8000}) {
            // slot states: empty, short history, full history, nothing held, win - 1 held (where the ratio lets M reach that residue)
            std::vector<long long> states = {0, std::max<long long>(1, T / 2), 3 * T + 5};
            for (int residue : {0, win - 1})
                for (long long f = 3 * T + 6; f < 3 * T + 6 + 3LL * win * r.D / r.U + 64; f++)
                    if (avd_resample::outputs_after(f, r, false) > 0 && avd_resample::outputs_after(f, r, false) % win == residue) { states.push_back(f); break; }
            const long long chunks[] = {1, T / 2 - 1, T / 2 + 1, T - 1, T, per_tile - 1, per_tile, per_tile + 1};
            const size_t ns = states.size(), nc = sizeof chunks / sizeof chunks[0];
            for (int nt = 1; nt <= 4; nt++) {
                // one track: every state x chunk x kind; more: rotations through them, a different one per position
                const size_t combos = nt == 1 ? ns * nc * 3 : ns * nc;
                for (size_t i = 0; i < combos; i++) {
                    SlotState state[kSlots];
                    std::vector<Want> tracks;
                    for (int j = 0; j < nt; j++) {
                        const size_t si = (i + 2 * (size_t)j) % ns, ci = (i / ns + 3 * (size_t)j) % nc, kind = (i / (ns * nc) + i + (size_t)j) % 3;
                        const long long n = std::max<long long>(1, chunks[ci]);
                        const int slot = 1 + (int)((i + 5 * (size_t)j) % 2) * 4 + j;      // distinct per position: j + 1 or j + 5
                        state[slot - 1] = slot_after(states[si], r, win);
                        tracks.push_back(Want{kind == 0 ? 0 : slot | (kind == 2 ? kEndBit : 0), n});
                    }
                    check_call(rate, win, channels, tracks, state);
                }
            }
        }
        // 8 continued and 56 whole tracks in one call
        {
            SlotState state[kSlots];
            std::vector<Want> tracks;
            for (int t = 0; t < kMaxEntries; t++) {
                const int slot = t % 8 == 3 ? t / 8 + 1 : 0;
                if (slot) state[slot - 1] = slot_after(2 * T + 3 + slot, r, 64);
                tracks.push_back(Want{slot | (slot == 4 ? kEndBit : 0), 1 + 37 * (t % 5) + (t == 9 ? per_tile : 0)});
            }
            check_call(rate, 64, channels, tracks, state);
        }
    }
    // the refusals, in the order include/avd.h lists them: every fault at once, then one fewer each time
    {
        Ratio r;
        avd_resample::ratio_of(48000, r);
        SlotState state[kSlots];
        state[1] = slot_after(5000, r, 64);
        state[1].same = false;                                // slot 2: bound to other values
        state[2] = slot_after((1LL << 31) * r.D / r.U + 10, r, 64);   // slot 3: the track is as long as it may get
        int cuts[2] = {100, 900}, entries[4] = {2, 3, 0, 0};
        struct { long long n; int nentries; bool end, same; int third; long long maxw; bool have; int want; } steps[] = {
            {900, 4, true, false, 3, 0, false, kCutBeyond},   {1000, 4, true, false, 3, 0, false, kEndPending}, {1000, 4, false, false, 3, 0, false, kEntryCount},
            {1000, 3, false, false, 3, 0, false, kSlotBinding}, {1000, 3, false, true, 3, 0, false, kTooLong},  {1000, 3, false, true, 0, 0, true, kWindowsTooSmall},
            {1000, 3, false, true, 0, 100, false, kWindowsTooSmall}, {1000, 3, false, true, 0, 100, true, kOk},
        };
        for (const auto& s : steps) {
            g_calls++;
            state[1].same = s.same;
            entries[1] = s.third;
            const Plan p = plan_map(s.n, 64, cuts, 2, entries, s.nentries, state, r, 2, s.maxw, s.have, s.end);
            EXPECT(p.refused == s.want, "refusal %d, want %d", p.refused, s.want);
            EXPECT(p.refused == kOk || (p.tracks.empty() && p.tiles.empty() && p.gather.empty() && p.saves.empty() && p.windows.nwin() == 0), "a refused plan holds something");
        }
        // a call that completes no window needs no records array
        g_calls++;
        int one[1] = {5};
        const Plan none = plan_map(40, 64, nullptr, 0, one, 1, state, r, 2, 0, false, false);
        EXPECT(none.refused == kOk && none.records == 0 && none.windows.nwin() == 0 && none.tiles.empty() && none.saves.size() == 1, "a call of 40 frames: refused %d, %lld records", none.refused, none.records);
    }
    // a slot whose memory is said to hold other than the rule gives is no call to plan; the buffer of all tracks together has its own limit,
    // and so has the number of records
    {
        Ratio r;
        avd_resample::ratio_of(48000, r);
        SlotState state[kSlots];
        int one[1] = {4};
        for (int wrong = 0; wrong < 3; wrong++) {
            g_calls++;
            state[3] = slot_after(5000, r, 64);
            if (wrong == 1) state[3].held++;
            if (wrong == 2) state[3].hist--;
            const Plan p = plan_map(300, 64, nullptr, 0, one, 1, state, r, 2, 100, true, false);
            EXPECT(p.refused == (wrong ? kSlotState : kOk) && p.refused_track == (wrong ? 0 : -1), "a slot state that is off by one (%d): refusal %d", wrong, p.refused);
        }
        const Ratio id = avd_resample::identity_ratio();
        int cuts[1] = {0x7ffffff0}, whole[2] = {0, 0};
        g_calls += 2;
        const Plan both = plan_map(0x7ffffff0LL + 100, 8000, cuts, 1, whole, 2, state, id, 1, 1 << 24, true, false);
        EXPECT(both.refused == kTooLong && both.refused_track == -1, "two tracks of 2^31 samples together: refusal %d track %d", both.refused, both.refused_track);
        const Plan many = plan_map(0x7ffffff0LL, 1, nullptr, 0, whole, 1, state, id, 1, 0x7fffffff, true, false);
        EXPECT(many.refused == kTooManyWindows, "2^31 records: refusal %d", many.refused);
    }
    // what the option accepts as an entry
    for (int v = -3; v < 70; v++) {
        const bool want = v >= 0 && v <= 0x18 && (v & 15) <= 8 && v != 0x10;
        EXPECT(entry_ok(v) == want, "entry %d", v);
    }
}

static std::vector<long long> list_of(const char* text)
{
    std::vector<long long> out;
    if (std::strcmp(text, "-") == 0) return out;
    for (const char* p = text; *p;) {
        char* end = nullptr;
        const long long v = std::strtoll(p, &end, 0);
        if (end == p) break;
        out.push_back(v);
        if (*end != ',') break;
        p = end + 1;
    }
    return out;
}

int main(int argc, char** argv)
{
    if (argc == 1) {
        check_everything();
        std::printf("audio map: %ld calls checked, %ld failures\n", g_calls, g_failures);
        return g_failures ? 1 : 0;
    }
    if (argc == 9 && std::strcmp(argv[1], "plan") == 0) {
        Ratio r;
        if (!ratio_for(std::atoi(argv[2]), r)) return 2;
        const int win = std::atoi(argv[3]);
        const long long n = std::atoll(argv[4]);
        const std::vector<long long> cuts = list_of(argv[5]), entries = list_of(argv[6]), frames = list_of(argv[7]);
        if (win < 1 || n < 0 || cuts.size() > 63 || entries.size() > 64 || frames.size() > (size_t)kSlots) return 2;
        std::vector<int> c(cuts.begin(), cuts.end()), e(entries.begin(), entries.end());
        SlotState state[kSlots];
        for (size_t k = 0; k < frames.size(); k++) state[k] = slot_after(frames[k], r, win);
        const Plan p = plan_map(n, win, c.data(), (int)c.size(), e.data(), (int)e.size(), state, r, 1, std::atoll(argv[8]), true, false);
        std::printf("refused %d total %lld records %lld fresh %lld continued %d tiles %zu gather %zu saves %zu\n", p.refused, p.total, p.records, p.fresh, p.continued, p.tiles.size(),
                    p.gather.size(), p.saves.size());
        for (const Track& t : p.tracks)
            std::printf("track slot %d last %d begin %lld n %lld region %lld held %d fresh %lld first %d count %d held_after %d\n", t.slot, (int)t.last, t.begin, t.n, t.region, t.c.held_before,
                        t.c.fresh(), t.first, t.count, t.c.held_after);
        return 0;
    }
    return 2;
}
