// Stand-alone check of csrc/avd_stream_plan.h (tests/test_stream_plan_host.py compiles it with -fsanitize=address,undefined and runs it).
// Every call of up to four clips with n in {0, 1, 2, 3} and the three slot states: the properties below are stated from the layout rule
// (include/avd.h, option "stream_map"), not from what plan_call does.
#include <cstdio>
#include <vector>
#include "../ai-video-detector_amd/csrc/avd_stream_plan.h"

using namespace avd_stream;

static int g_failed = 0;
static long g_cases = 0;

static void fail(const std::vector<ClipIn>& in, const char* what)
{
    if (g_failed++ > 20) return;
    std::fprintf(stderr, "FAIL %s:", what);
    for (const ClipIn& c : in) std::fprintf(stderr, " (n=%d state=%d)", c.n, c.state);
    std::fprintf(stderr, "\n");
}

static void check(const std::vector<ClipIn>& in)
{
    g_cases++;
    const int k = (int)in.size();
    const Plan p = plan_call(in.data(), k);
    if ((int)p.f0.size() != k || (int)p.carry.size() != k) { fail(in, "sizes"); return; }

    // the segments tile [0, total) in clip order; a carry exists exactly for mapped, filled, non-empty clips, directly in front of f0
    int at = 0, own = 0, carries = 0, segments = 0;
    bool any_filled = false;
    for (int c = 0; c < k; c++) {
        const bool want_carry = in[c].state == kMappedFilled && in[c].n > 0;
        any_filled |= want_carry;
        if (want_carry) {
            if (p.carry[c] != at) fail(in, "carry place");
            at++;
            carries++;
            if (p.carry[c] != p.f0[c] - 1) fail(in, "carry not in front of f0");
        } else if (p.carry[c] != -1) fail(in, "carry where none belongs");
        if (p.f0[c] != at) fail(in, "f0");
        at += in[c].n;
        own += in[c].n;
        segments += in[c].n > 0;
    }
    if (p.total != at) fail(in, "total");
    if (p.own != own) fail(in, "own");
    if (p.carries != carries) fail(in, "carries");
    if (p.segments != segments) fail(in, "segments");

    // clipstart: 1 at every carry frame, 1 at the first frame of every clip without a carry, 0 at the first own frame of a continued clip, 0 elsewhere
    if ((int)p.clipstart.size() != p.total) { fail(in, "clipstart size"); return; }
    std::vector<int> want((size_t)p.total, 0), is_carry((size_t)p.total, 0);
    for (int c = 0; c < k; c++) {
        if (in[c].n <= 0) continue;
        if (p.carry[c] >= 0) { want[(size_t)p.carry[c]] = 1; is_carry[(size_t)p.carry[c]] = 1; }
        else want[(size_t)p.f0[c]] = 1;
    }
    for (int f = 0; f < p.total; f++)
        if (p.clipstart[(size_t)f] != want[(size_t)f]) { fail(in, "clipstart"); break; }
    if (p.total > 0 && p.clipstart[0] != 1) fail(in, "frame 0 has no predecessor");

    // the runs are exactly the own frames in order, no carry among them
    std::vector<int> handed, expect;
    for (const Run& r : p.runs) {
        if (r.count <= 0 || r.first < 0 || r.first + r.count > p.total) { fail(in, "run bounds"); return; }
        for (int i = 0; i < r.count; i++) handed.push_back(r.first + i);
    }
    for (int f = 0; f < p.total; f++)
        if (!is_carry[(size_t)f]) expect.push_back(f);
    if (handed != expect) fail(in, "runs");
    for (size_t i = 1; i < p.runs.size(); i++)
        if (p.runs[i - 1].first + p.runs[i - 1].count >= p.runs[i].first) fail(in, "runs not merged or not ascending");

    // no filled slot: the batch layout -- f0 is the running sum, one run from 0
    if (!any_filled) {
        int sum = 0;
        for (int c = 0; c < k; c++) { if (p.f0[c] != sum) fail(in, "batch f0"); sum += in[c].n; }
        if (sum > 0 && !(p.runs.size() == 1 && p.runs[0].first == 0 && p.runs[0].count == sum)) fail(in, "batch run");
        if (sum == 0 && !p.runs.empty()) fail(in, "runs of an empty call");
    }
    // a single continued clip (whatever empty clips the call lists): the single-slot layout -- f0 = 1, one run from 1, one segment
    int live = 0, who = -1;
    for (int c = 0; c < k; c++)
        if (in[c].n > 0) { live++; who = c; }
    if (live == 1 && in[who].state == kMappedFilled) {
        if (p.f0[who] != 1 || p.total != in[who].n + 1) fail(in, "single-slot f0");
        if (!(p.runs.size() == 1 && p.runs[0].first == 1 && p.runs[0].count == in[who].n)) fail(in, "single-slot run");
        if (p.segments != 1) fail(in, "single-slot segments");
    }
}

// with arguments "n:state" ...: print that call's plan, for the test to compare with a layout written out by hand
static int dump(int argc, char** argv)
{
    std::vector<ClipIn> in;
    for (int i = 1; i < argc; i++) {
        ClipIn c{};
        if (std::sscanf(argv[i], "%d:%d", &c.n, &c.state) != 2) return 2;
        in.push_back(c);
    }
    const Plan p = plan_call(in.data(), (int)in.size());
    std::printf("total %d own %d carries %d segments %d\nf0", p.total, p.own, p.carries, p.segments);
    for (int v : p.f0) std::printf(" %d", v);
    std::printf("\ncarry");
    for (int v : p.carry) std::printf(" %d", v);
    std::printf("\nclipstart");
    for (int v : p.clipstart) std::printf(" %d", v);
    std::printf("\nruns");
    for (const Run& r : p.runs) std::printf(" %d+%d", r.first, r.count);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1) return dump(argc, argv);
    check({});
    for (int k = 1; k <= 4; k++) {
        int combos = 1;
        for (int i = 0; i < k; i++) combos *= 12;                  // 4 sizes x 3 states per clip
        for (int code = 0; code < combos; code++) {
            std::vector<ClipIn> in((size_t)k);
            int v = code;
            for (int c = 0; c < k; c++) { in[(size_t)c] = ClipIn{v % 4, (v / 4) % 3}; v /= 12; }
            check(in);
        }
    }
    // the layout of the header comment, spelled out: [carry_a][a a][carry_b][b][c c]
    {
        const std::vector<ClipIn> in = {{2, kMappedFilled}, {1, kMappedFilled}, {2, kUnmapped}};
        const Plan p = plan_call(in.data(), 3);
        const std::vector<int> cs = {1, 0, 0, 1, 0, 1, 0};
        if (p.clipstart != cs || p.total != 7 || p.runs.size() != 2 || p.runs[0].first != 1 || p.runs[0].count != 2 || p.runs[1].first != 4 ||
            p.runs[1].count != 3) fail(in, "worked example");
    }
    std::printf("stream plan: %ld calls checked, %d failures\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
