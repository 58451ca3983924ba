// Where the clips of one avd_analyze_* call lie in the per-frame buffers when some of them continue a stream slot (options "stream_slot" and
// "stream_map", include/avd.h).  Plain host code over the standard library only: the library (avd_capi.hip) and a stand-alone check program
// (tests/stream_plan_check.cpp) include it.
//
// A clip that continues a FILLED slot gets one extra frame in front of its own -- the slot's frame, restored there ahead of the ingest (its
// "carry").  Every other clip lies where a batch puts it:
//
//     [carry_a][a ...][carry_b][b ...][c ...] ...
//
// The Farneback stage runs once over all consecutive pairs.  The pair that ENDS at a carry frame, or at the first frame of a clip without one,
// is computed in vain (clipstart = 1 there: that frame has no predecessor); the pair (carry, first own frame) is a real one (clipstart = 0).
// The records that go out are the own frames, clip after clip: the buffers minus the carries, as a list of runs.
#pragma once
#include <cstddef>
#include <vector>

namespace avd_stream {

enum SlotState { kUnmapped = 0, kMappedEmpty = 1, kMappedFilled = 2 };

struct ClipIn { int n; int state; };             // the clip's frames (>= 0) and the state of the slot it continues (SlotState)
struct Run { int first, count; };                // records [first, first + count) of the per-frame buffers

struct Plan {
    std::vector<int> f0;                         // per clip: its first own frame (an empty clip: where it would lie)
    std::vector<int> carry;                      // per clip: the frame its slot is restored to (f0 - 1), or -1
    std::vector<int> clipstart;                  // per frame: 1 = no predecessor
    std::vector<Run> runs;                       // the own frames in order; neighbours are merged
    int total = 0;                               // frames in the buffers, carries included
    int own = 0;                                 // the callers' frames = the records that go out
    int carries = 0;
    int segments = 0;                            // frames with clipstart = 1: with one segment nobody needs the table (frame 0 starts it)
};

inline Plan plan_call(const ClipIn* clips, int nclips)
{
    Plan p;
    p.f0.assign((size_t)(nclips > 0 ? nclips : 0), 0);
    p.carry.assign(p.f0.size(), -1);
    int at = 0;
    for (int c = 0; c < nclips; c++) {
        const int n = clips[c].n;
        if (n <= 0) { p.f0[(size_t)c] = at; continue; }          // an empty clip brings nothing and restores nothing
        const bool carried = clips[c].state == kMappedFilled;
        if (carried) {
            p.carry[(size_t)c] = at++;
            p.clipstart.push_back(1);
            p.carries++;
        }
        p.f0[(size_t)c] = at;
        p.clipstart.push_back(carried ? 0 : 1);
        p.clipstart.insert(p.clipstart.end(), (size_t)n - 1, 0);
        if (!p.runs.empty() && p.runs.back().first + p.runs.back().count == at) p.runs.back().count += n;
        else p.runs.push_back(Run{at, n});
        at += n;
        p.own += n;
        p.segments++;
    }
    p.total = at;
    return p;
}

}  // namespace avd_stream
