// Stand-alone check of csrc/avd_ingest_group.h (tests/ingest_group_kit.py compiles it with -fsanitize=address,undefined and runs it).
// Every call of up to four clips with a key out of three, n in {0, 1, 2, 5} and output frames with and without gaps, under the library's bound
// and under one small enough to split groups.  The properties are stated from the rule (include/avd.h, option "ingest_group"; DESIGN.md
// section 3.2.1), not from what plan_groups does -- and two planners that break the rule on purpose must be caught by the same checker.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>
#include "../ai-video-detector_amd/csrc/avd_ingest_group.h"

using namespace avd_group;

struct Call {
    std::vector<Key> keys;
    std::vector<int> n, f0;
    int64_t bound;
};
using Planner = std::function<Plan(const Call&)>;

// the three keys: 96 x 64 BGR with dense rows, the same with padded rows (only row_stride differs), 100 x 66 NV12
static Key key_value(int i)
{
    const Key k[3] = {{64, 96, 5, AVD_FMT_BGR24, 0, 0, 288, 0, 1}, {64, 96, 5, AVD_FMT_BGR24, 0, 0, 320, 0, 1}, {66, 100, 5, AVD_FMT_NV12, 0, 0, 100, 100, 0}};
    return k[i];
}

// field by field, on purpose not same_key
static bool equal_keys(const Key& a, const Key& b)
{
    return a.h == b.h && a.w == b.w && a.nbands == b.nbands && a.format == b.format && a.rotate == b.rotate && a.full_range == b.full_range &&
           a.row_stride == b.row_stride && a.uv_row_stride == b.uv_row_stride && a.vec == b.vec;
}

// the first broken property, or null
static const char* broken(const Call& in, const Plan& p)
{
    const int k = (int)in.n.size();
    if ((int)p.group_of.size() != k) return "group_of size";
    // every frame of every live clip in exactly one group, exactly once, at output frame f0 + i
    std::vector<std::vector<int>> seen((size_t)k);
    for (int c = 0; c < k; c++) seen[(size_t)c].assign((size_t)(in.n[(size_t)c] > 0 ? in.n[(size_t)c] : 0), 0);
    int prev_first = -1;
    for (size_t gi = 0; gi < p.groups.size(); gi++) {
        const Group& G = p.groups[gi];
        if (G.members.empty()) return "a group without members";
        if (G.members.front().clip <= prev_first) return "groups are not in the order of their first member";
        prev_first = G.members.front().clip;
        if (G.grouped != (G.members.size() > 1)) return "a group of one clip is not marked ungrouped (or a larger one is)";
        int frames = 0, prev_clip = -1;
        for (const Member& m : G.members) {
            if (m.clip < 0 || m.clip >= k) return "member out of range";
            if (m.clip <= prev_clip) return "members are not in call order";
            prev_clip = m.clip;
            if (m.n != in.n[(size_t)m.clip] || m.n <= 0) return "a member's frame count";
            if (m.g0 != frames) return "a member's group frames do not follow its predecessor's";
            if (p.group_of[(size_t)m.clip] != (int)gi) return "group_of";
            if (!equal_keys(in.keys[(size_t)m.clip], in.keys[(size_t)G.members.front().clip])) return "members do not share the key";
            if (!equal_keys(G.key, in.keys[(size_t)m.clip])) return "the group's key is not its members'";
            frames += m.n;
        }
        if (G.frames != frames) return "a group's frame count";
        if (G.grouped && (int64_t)G.frames * G.key.nbands > in.bound) return "the split bound";
        for (int g = 0; g < G.frames; g++) {
            const Frame f = G.at(g);
            if (f.clip < 0 || f.clip >= k || f.frame < 0 || f.frame >= in.n[(size_t)f.clip]) return "a group frame names no frame of the call";
            if (p.group_of[(size_t)f.clip] != (int)gi) return "a group frame of a clip that is not a member";
            if (f.out != in.f0[(size_t)f.clip] + f.frame) return "output frame is not f0 + frame in clip";
            seen[(size_t)f.clip][(size_t)f.frame]++;
        }
        if (G.at(G.frames).clip != -1) return "a frame behind the group's last";
    }
    for (int c = 0; c < k; c++) {
        if (in.n[(size_t)c] <= 0 && p.group_of[(size_t)c] != -1) return "a clip without frames is in a group";
        for (int v : seen[(size_t)c])
            if (v != 1) return "a frame is in no group, or in more than one";
    }
    // under the library's bound nothing is split: the clips of a key are ONE group
    if (in.bound == kMaxLaunchBands)
        for (int a = 0; a < k; a++)
            for (int b = a + 1; b < k; b++)
                if (in.n[(size_t)a] > 0 && in.n[(size_t)b] > 0 && equal_keys(in.keys[(size_t)a], in.keys[(size_t)b]) && p.group_of[(size_t)a] != p.group_of[(size_t)b])
                    return "two clips of one key in two groups";
    // the runs of row partials / Laplacian partials: as large as the group's frames need, inside the call's total, disjoint
    for (size_t a = 0; a < p.groups.size(); a++) {
        const Group& A = p.groups[a];
        if (A.rowbuf_elems() != (size_t)A.frames * A.key.h * 32 || A.lappart_elems() != (size_t)A.frames * A.key.nbands * kLapSlots * 2) return "run sizes";
        if (A.rowbuf_off + A.rowbuf_elems() > p.rowbuf_elems || A.lappart_off + A.lappart_elems() > p.lappart_elems) return "a run leaves the buffer";
        for (size_t b = a + 1; b < p.groups.size(); b++) {
            const Group& B = p.groups[b];
            if (A.rowbuf_off < B.rowbuf_off + B.rowbuf_elems() && B.rowbuf_off < A.rowbuf_off + A.rowbuf_elems()) return "row partial runs overlap";
            if (A.lappart_off < B.lappart_off + B.lappart_elems() && B.lappart_off < A.lappart_off + A.lappart_elems()) return "Laplacian partial runs overlap";
        }
    }
    return nullptr;
}

static Plan the_planner(const Call& in) { return plan_groups(in.keys.data(), in.n.data(), in.f0.data(), (int)in.n.size(), in.bound); }

// control 1: a planner that leaves row_stride out of the key
static Plan planner_without_row_stride(const Call& in)
{
    std::vector<Key> keys = in.keys;
    for (Key& k : keys) k.row_stride = 0;
    return plan_groups(keys.data(), in.n.data(), in.f0.data(), (int)in.n.size(), in.bound);
}

// control 2: a planner that numbers the output frames without the gaps
static Plan planner_without_gaps(const Call& in)
{
    std::vector<int> f0(in.n.size());
    int at = 0;
    for (size_t c = 0; c < in.n.size(); c++) { f0[c] = at; at += in.n[c]; }
    return plan_groups(in.keys.data(), in.n.data(), f0.data(), (int)in.n.size(), in.bound);
}

struct Tally { long cases = 0, failed = 0; };

static void run_all(const Planner& planner, Tally& t, bool report)
{
    const int sizes[4] = {0, 1, 2, 5};
    const int64_t bounds[2] = {kMaxLaunchBands, 5 * 6};            // the second one: six frames of five bands
    for (int k = 0; k <= 4; k++) {
        int combos = 1;
        for (int i = 0; i < k; i++) combos *= 12;                  // 3 keys x 4 sizes per clip
        for (int code = 0; code < combos; code++)
            for (int gaps = 0; gaps < 2; gaps++)
                for (int64_t bound : bounds) {
                    Call in;
                    in.bound = bound;
                    int v = code, at = 0;
                    for (int c = 0; c < k; c++) {
                        const int n = sizes[v % 4];
                        in.keys.push_back(key_value((v / 4) % 3));
                        in.n.push_back(n);
                        if (gaps && n > 0) at++;                   // a carry frame in front of every clip that brings frames ("stream_map")
                        in.f0.push_back(at);
                        at += n;
                        v /= 12;
                    }
                    t.cases++;
                    const char* why = broken(in, planner(in));
                    if (!why) continue;
                    if (report && t.failed < 20) {
                        std::fprintf(stderr, "FAIL %s: bound %lld,", why, (long long)bound);
                        for (int c = 0; c < k; c++) std::fprintf(stderr, " (key %d n=%d f0=%d)", (int)(in.keys[(size_t)c].row_stride), in.n[(size_t)c], in.f0[(size_t)c]);
                        std::fprintf(stderr, "\n");
                    }
                    t.failed++;
                }
    }
}

// with arguments "key:n:f0" ... [bound=B]: print that call's plan, for the test to compare with groups written out by hand
static int dump(int argc, char** argv)
{
    Call in;
    in.bound = kMaxLaunchBands;
    for (int i = 1; i < argc; i++) {
        int key, n, f0;
        long long b;
        if (std::sscanf(argv[i], "bound=%lld", &b) == 1) { in.bound = b; continue; }
        if (std::sscanf(argv[i], "%d:%d:%d", &key, &n, &f0) != 3 || key < 0 || key > 2) return 2;
        in.keys.push_back(key_value(key)); in.n.push_back(n); in.f0.push_back(f0);
    }
    const Plan p = the_planner(in);
    for (const Group& G : p.groups) {
        std::printf("group grouped %d frames %d rowbuf %zu lappart %zu members", (int)G.grouped, G.frames, G.rowbuf_off, G.lappart_off);
        for (const Member& m : G.members) std::printf(" %d", m.clip);
        std::printf(" out");
        for (int g = 0; g < G.frames; g++) std::printf(" %d", G.at(g).out);
        std::printf("\n");
    }
    std::printf("total rowbuf %zu lappart %zu\n", p.rowbuf_elems, p.lappart_elems);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1) return dump(argc, argv);
    Tally real, no_stride, no_gaps;
    run_all(the_planner, real, true);
    run_all(planner_without_row_stride, no_stride, false);
    run_all(planner_without_gaps, no_gaps, false);
    std::printf("ingest groups: %ld calls checked, %ld failures; control without row_stride rejected in %ld calls, control without gaps in %ld\n",
                real.cases, real.failed, no_stride.failed, no_gaps.failed);
    return real.failed || !no_stride.failed || !no_gaps.failed ? 1 : 0;
}
