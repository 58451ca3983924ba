// Which clips of one avd_analyze_* call are ingested by ONE launch (option "ingest_group", include/avd.h), and where each frame of such a launch
// comes from and goes to.  Plain host code over the standard library and avd_ingest_clip.h only: the library (avd_capi.hip) and a stand-alone
// check program (tests/ingest_group_check.cpp) include it.
//
// Clips that share a KEY -- everything an ingest launch is specialised by -- form a group.  A group of several clips runs as one listed launch
// over its frames, clip after clip in call order: group frame g reads the planes of (clip, frame in clip) and writes the per-frame results at
// output frame f0[clip] + frame in clip.  The output frames of a group are not one run (other clips, and the carry frames of "stream_map",
// lie between its members), which is why the launch takes them from a table.  What only the group's own two launches exchange -- the row
// partials and the Laplacian partials -- is indexed by g and forms one run per group.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "avd_ingest_clip.h"

constexpr int kLapSlots = 8;       // per-band slots of the Laplacian partials, one per wave of the ingest workgroup (4 written)

namespace avd_group {

// An ingest launch forms frames * nbands as an int (decode_band, avd_preprocess.hip) and rounds its grid up to a multiple of 8: the frames of
// one launch, a group's as well as a single clip's, stay below this many bands.
constexpr int64_t kMaxLaunchBands = INT_MAX - 7;

// What two clips must share to share a launch.  h, w: the displayed picture's (the geometry tables and the band plan follow them); nbands is a
// function of them, kept here because the split bound needs it.  vec: the clip's OWN answer to "may it run the 16-byte fills"
// (strided_vec_eligible / list_vec_eligible): an aligned and a misaligned clip of one layout run different kernels, alone and here.
struct Key {
    int h, w, nbands;
    int format, rotate, full_range;
    int64_t row_stride, uv_row_stride;
    int vec;
};
inline bool same_key(const Key& a, const Key& b)
{
    return a.h == b.h && a.w == b.w && a.nbands == b.nbands && a.format == b.format && a.rotate == b.rotate && a.full_range == b.full_range &&
           a.row_stride == b.row_stride && a.uv_row_stride == b.uv_row_stride && a.vec == b.vec;
}
inline Key key_of(const IngestClip& k, int nbands, bool vec)
{
    return Key{k.disp_h(), k.disp_w(), nbands, k.format, k.rotate, k.full_range != 0, k.row_stride, k.planes() > 1 ? k.uv_row_stride : 0, vec ? 1 : 0};
}

struct Member { int clip, n, g0, out0; };        // the clip's n frames are group frames [g0, g0 + n) and output frames [out0, out0 + n)
struct Frame { int clip, frame, out; };          // group frame g: frame `frame` of clip `clip`, results at output frame `out`

struct Group {
    Key key{};
    std::vector<Member> members;                 // in call order
    int frames = 0;
    bool grouped = false;                        // several clips: one listed launch with an output table; false: the clip runs today's per-clip path
    size_t rowbuf_off = 0, lappart_off = 0;      // the group's run of the row partials [frames][h][32] / Laplacian partials [frames][nbands][kLapSlots][2]
    size_t rowbuf_elems() const { return (size_t)frames * key.h * AVD_HASH; }
    size_t lappart_elems() const { return (size_t)frames * key.nbands * kLapSlots * 2; }
    Frame at(int g) const
    {
        for (const Member& m : members)
            if (g < m.g0 + m.n) return Frame{m.clip, g - m.g0, m.out0 + (g - m.g0)};
        return Frame{-1, -1, -1};
    }
};

struct Plan {
    std::vector<Group> groups;                   // in the order of their first member
    std::vector<int> group_of;                   // per clip: its group, -1 for a clip without frames
    size_t rowbuf_elems = 0, lappart_elems = 0;  // what the call needs of either buffer
};

// keys[c], n[c], f0[c]: the key, the frames and the first output frame of clip c.  max_bands: kMaxLaunchBands (a check program passes less).
// A clip joins the latest group of its key while the group's frames * nbands stay within the bound; otherwise it opens a new one -- so a
// group is split between clips, and a clip that alone passes the bound is alone, as it is today.
inline Plan plan_groups(const Key* keys, const int* n, const int* f0, int nclips, int64_t max_bands = kMaxLaunchBands)
{
    Plan p;
    p.group_of.assign((size_t)(nclips > 0 ? nclips : 0), -1);
    for (int c = 0; c < nclips; c++) {
        if (n[c] <= 0) continue;
        int at = -1;
        for (int g = (int)p.groups.size() - 1; g >= 0 && at < 0; g--)
            if (same_key(p.groups[(size_t)g].key, keys[c])) at = g;      // the latest group of the key: an earlier one of the same key is full
        if (at >= 0 && ((int64_t)p.groups[(size_t)at].frames + n[c]) * keys[c].nbands > max_bands) at = -1;
        if (at < 0) {
            at = (int)p.groups.size();
            p.groups.emplace_back();
            p.groups.back().key = keys[c];
        }
        Group& G = p.groups[(size_t)at];
        G.members.push_back(Member{c, n[c], G.frames, f0[c]});
        G.frames += n[c];
        G.grouped = G.members.size() > 1;
        p.group_of[(size_t)c] = at;
    }
    for (Group& G : p.groups) {
        G.rowbuf_off = p.rowbuf_elems;
        G.lappart_off = p.lappart_elems;
        p.rowbuf_elems += G.rowbuf_elems();
        p.lappart_elems += G.lappart_elems();
    }
    return p;
}

// A grouped launch's place in the call's table of plane pointers: [plane][frames] device addresses, then the output frames as int32[frames] in
// the entries behind them (two to an entry).
inline size_t table_entries(int planes, int frames) { return (size_t)planes * frames + ((size_t)frames + 1) / 2; }

}  // namespace avd_group
