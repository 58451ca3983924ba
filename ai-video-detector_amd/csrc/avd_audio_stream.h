// A track continued across avd_audio_features calls (option "audio_slot", include/avd.h): what ONE call of such a track runs over.  Plain host
// code over the standard library and avd_audio_resample.h, in that header's manner: the library and a stand-alone check program
// (tests/audio_stream_check.cpp) include it.
//
// The rule (include/avd.h states it in full).  N the frames the slot has absorbed, this call included; U, D, T the rate's (U = D = 1, T = 0 for a
// track that is not converted).  Output m reads frames floor(m D / U) - T/2 + 1 ... floor(m D / U) + T/2, so after a call that is not the last
// exactly the outputs whose last tap lies at or below frame N - 1 exist:
//
//     M(N) = ceil(max(0, N - T/2) U / D)                       and, after the last call,  M = ceil(N U / D)  (zeros beyond the end)
//
// and W = floor(M / win) windows have been handed out (ceil after the last call).  A call forms outputs [M_before, M_after) behind the
// M_before - W_before win samples the slot held back, hands out windows [W_before, W_after) and holds the rest back.  Its first output's first
// tap lies at or above frame N_before - (T - 1): the slot keeps the last min(N, T - 1) frames, narrowed and downmixed (both are per frame).
//
//     frames     ... | history (T - 1) |------------- this call's n frames -------------|
//     outputs    held |------------------ new: [M_before, M_after) -----------|   (the last T/2 frames' outputs wait for the next call)
//     windows    |---win---|---win---|---win---|--- held back --|
//
// A tile carries positions relative to the TRACK (Tile::begin = 0, Tile::end = N: frames at or beyond N are zeros, which only the last call's
// tiles reach); Tile::out0 counts from the first held sample, so the analyzer's buffer is [held | new].
#pragma once
#include "avd_audio_resample.h"

namespace avd_resample {

constexpr int kMaxHistory = 400;                 // frames a slot's history buffer holds: T - 1 is at most 395 (192000: T = 396)

// the ratio of a track that is not converted ("audio_rate" 0): every frame is its own output, no support, no history
inline Ratio identity_ratio() { Ratio r; r.rate = 0; r.U = 1; r.D = 1; r.T = 0; return r; }

// M of the rule; n_frames >= 0
inline long long outputs_after(long long n_frames, const Ratio& r, bool last)
{
    const long long usable = last ? n_frames : std::max<long long>(0, n_frames - r.T / 2);
    return (usable * r.U + r.D - 1) / r.D;
}
// frames of history a slot that has absorbed n_frames keeps
inline int history_frames(long long n_frames, const Ratio& r) { return (int)std::min<long long>(n_frames, r.T > 0 ? r.T - 1 : 0); }

struct Continue {
    int refused = kOk;                           // kTooLong: the track would pass kMaxOutputs outputs
    long long n_before = 0, n_after = 0;         // frames absorbed
    long long m_before = 0, m_after = 0;         // outputs that exist
    int held_before = 0, held_after = 0;         // output samples held back, fewer than win
    int hist_before = 0, hist_after = 0;         // frames of history: the track's frames [n - hist, n)
    long long windows = 0;                       // records this call writes
    long long analysed = 0;                      // samples of [held | new] the analyzer windows: windows * win, or all of them in the last call
    int tile_out = 0;
    std::vector<Tile> tiles;                     // the new outputs; empty when the call forms none
    long long fresh() const { return m_after - m_before; }
};

// n_before frames absorbed so far, n >= 0 more in this call, 1 <= win.  A refused plan holds nothing.
inline Continue plan_continue(long long n_before, long long n, bool last, const Ratio& r, int win)
{
    Continue c;
    c.n_before = n_before;
    c.n_after = n_before + n;
    if (outputs_after(c.n_after, r, true) > kMaxOutputs) { c.refused = kTooLong; return c; }
    c.m_before = outputs_after(n_before, r, false);
    c.m_after = outputs_after(c.n_after, r, last);
    c.held_before = (int)(c.m_before % win);
    const long long have = c.held_before + c.fresh();
    c.windows = last ? (have + win - 1) / win : have / win;
    c.analysed = last ? have : c.windows * win;
    c.held_after = (int)(have - c.analysed);
    c.hist_before = history_frames(n_before, r);
    c.hist_after = last ? 0 : history_frames(c.n_after, r);
    c.tile_out = tile_outputs(r);
    for (long long m0 = c.m_before; r.rate != 0 && m0 < c.m_after; m0 += c.tile_out) {      // an unconverted track has no converter launch
        const long long base = m0 * (long long)r.D;
        Tile tile;
        tile.in0 = base / r.U - (r.T ? r.T / 2 - 1 : 0);
        tile.begin = 0;
        tile.end = c.n_after;
        tile.out0 = c.held_before + (m0 - c.m_before);
        tile.count = (int)std::min<long long>(c.tile_out, c.m_after - m0);
        tile.phase = (int)(base % r.U);
        c.tiles.push_back(tile);
    }
    return c;
}

}  // namespace avd_resample
