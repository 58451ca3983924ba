// Stand-alone check of the channel-layout part of csrc/avd_audio_resample.h (option "audio_layout": ids, downmix weights, the mix a launch goes
// by, the LDS sizing of a layout launch), built with the address and undefined-behaviour sanitizers by tests/audio_layout_kit.py and run as a
// program, in the manner of tests/audio_resample_check.cpp.
//
//   audio_layout_check               every check; prints "audio layout: N checks, F failures", status 1 if F > 0
//   audio_layout_check weights ID    prints the channel count and the eight weights of layout ID
//   audio_layout_check lds RATE      prints "layout stereo max_span" -- lds_layout_bytes, lds_bytes(r, 2) and max_span of the rate
//
// The table the weights are compared with is the one include/avd.h writes out; the bound on the LDS is the one the header states.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../ai-video-detector_amd/csrc/avd_audio_resample.h"

using namespace avd_resample;

static long g_checks = 0, g_failures = 0;

#define EXPECT(cond, ...)                                                                                     \
    do {                                                                                                      \
        g_checks++;                                                                                           \
        if (!(cond)) {                                                                                        \
            if (g_failures++ < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                     \
    } while (0)

static const int kIds[4] = {1, 2, 6, 8};
static const int kTable[4][8] = {{32768, 0, 0, 0, 0, 0, 0, 0},
                                 {16384, 16384, 0, 0, 0, 0, 0, 0},
                                 {6786, 6786, 9598, 0, 4799, 4799, 0, 0},
                                 {5249, 5249, 7422, 0, 3712, 3712, 3712, 3712}};

static void check_everything()
{
    // what the option accepts: 0, and the four ids with or without the planar flag -- nothing else of -2 ... 0x400
    for (int v = -2; v <= 0x400; v++) {
        const int id = v & ~kLayoutPlanar;
        const bool want = v == 0 || (v > 0 && (id == 1 || id == 2 || id == 6 || id == 8));
        EXPECT(layout_ok(v) == want, "layout_ok(%d)", v);
    }
    EXPECT(!layout_ok(0x100) && !layout_ok(0x200 | 2) && !layout_ok(-0x100), "flags alone, other flags, negative values");
    for (int i = 0; i < 4; i++) {
        int w[kMaxChannels];
        const int channels = layout_weights(kIds[i], w);
        EXPECT(channels == kIds[i], "layout %d has %d channels", kIds[i], channels);
        long long sum = 0, mag = 0;
        for (int c = 0; c < kMaxChannels; c++) {
            EXPECT(w[c] == kTable[i][c], "layout %d weight %d is %d, the table says %d", kIds[i], c, w[c], kTable[i][c]);
            EXPECT(w[c] >= 0 && (c < channels || w[c] == 0), "layout %d weight %d", kIds[i], c);
            sum += w[c];
            mag += (long long)w[c] * 32768;
        }
        EXPECT(sum == 32768, "layout %d sums to %lld", kIds[i], sum);
        // every channel at -32768 is the extreme: |sum w s| = 2^30, and the rounding term keeps it inside 32 bits
        EXPECT(mag == (1LL << 30) && mag + 16384 < (1LL << 31), "layout %d reaches %lld", kIds[i], mag);
        for (int planar = 0; planar < 2; planar++) {
            const Mix m = mix_of(kIds[i] | (planar ? kLayoutPlanar : 0), 12345);
            EXPECT(m.id == kIds[i] && m.planar == planar && m.channels == channels && m.stride == (planar ? 12345 : 0), "mix of layout %d planar %d", kIds[i], planar);
            EXPECT(std::memcmp(m.w, w, sizeof w) == 0, "mix of layout %d: weights", kIds[i]);
        }
    }
    int w[kMaxChannels];
    EXPECT(layout_weights(3, w) == 0 && layout_weights(0, w) == 0 && layout_weights(7, w) == 0, "unknown ids have no weights");
    // LFE is channel 3 of both surround layouts, and the centre takes the remainder
    EXPECT(kTable[2][3] == 0 && kTable[3][3] == 0, "LFE");
    // the LDS of a layout launch: at most today's stereo footprint plus one 32-bit accumulator per span frame, at every rate -- and its parts
    // hold what the kernel puts there
    for (int i = 0; i < kNumRates; i++) {
        Ratio r;
        EXPECT(ratio_of(kRates[i], r), "rate %d", kRates[i]);
        const size_t span = (size_t)max_span(r);
        EXPECT(lds_layout_bytes(r) <= lds_bytes(r, 2) + 4 * span + 16, "rate %d: %zu bytes, stereo %zu, span %zu", kRates[i], lds_layout_bytes(r), lds_bytes(r, 2), span);
        EXPECT(lds_acc_bytes(r) >= 4 * span && lds_acc_bytes(r) % 16 == 0 && lds_weights_bytes() == 4 * (size_t)kMaxChannels && lds_weights_bytes() % 16 == 0,
               "rate %d: accumulators %zu", kRates[i], lds_acc_bytes(r));
        EXPECT(lds_layout_bytes(r) == lds_taps_bytes(r) + lds_acc_bytes(r) + lds_weights_bytes() + lds_mono_bytes(r) + up16(((size_t)tile_outputs(r) + 8) * 2),
               "rate %d: the parts", kRates[i]);
        EXPECT(lds_layout_bytes(r) <= 160 * 1024, "rate %d: %zu bytes", kRates[i], lds_layout_bytes(r));
        // a tile never spans more than max_span, whatever its phase
        for (int phase = 0; phase < r.U; phase++) EXPECT(tile_span(r, tile_outputs(r), phase) <= (int)span, "rate %d phase %d", kRates[i], phase);
    }
}

int main(int argc, char** argv)
{
    if (argc == 1) {
        check_everything();
        std::printf("audio layout: %ld checks, %ld failures\n", g_checks, g_failures);
        return g_failures ? 1 : 0;
    }
    if (argc == 3 && std::strcmp(argv[1], "weights") == 0) {
        int w[kMaxChannels];
        std::printf("%d", layout_weights(std::atoi(argv[2]), w));
        for (int c = 0; c < kMaxChannels; c++) std::printf(" %d", w[c]);
        std::printf("\n");
        return 0;
    }
    if (argc == 3 && std::strcmp(argv[1], "lds") == 0) {
        Ratio r;
        if (!ratio_of(std::atoi(argv[2]), r)) return 2;
        std::printf("%zu %zu %d\n", lds_layout_bytes(r), lds_bytes(r, 2), max_span(r));
        return 0;
    }
    return 2;
}
