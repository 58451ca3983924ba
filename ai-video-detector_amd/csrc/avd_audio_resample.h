// What the converter in front of avd_audio_features runs over (options "audio_rate" / "audio_channels", include/avd.h): the supported rates and
// their ratios, the fixed-point filter bank of a rate, each track's run of 16 kHz output samples with the output-side cut list they imply, and
// the tile table the kernel (k_audio_resample, avd_audio.hip) goes by.  Plain host code over the standard library only, in the manner of
// avd_audio_plan.h: the library and a stand-alone check program (tests/audio_resample_check.cpp) include it.
//
// The rule (include/avd.h states it in full).  R the input rate, g = gcd(R, 16000), U = 16000 / g, D = R / g.  A track of n_t frames has
// ceil(n_t U / D) output samples; output m of a track reads the track's frames i0 - T/2 + 1 ... i0 + T/2 with i0 = floor(m D / U) through row
// phi = (m D) mod U of the bank, frames outside the track counting as 0.  Rate 16000 has no bank (T = 0): its output is the downmixed frame.
//
// A tile is one workgroup's run of at most tile_outputs() consecutive output samples of ONE track:
//
//     track t:  |---- tile ----|---- tile ----|-- tile --|      track t + 1:  |---- tile ----|- tile -| ...
//
// It carries the absolute frame its span begins at (64 bits: m D passes 2^31 after five minutes at D = 441; it lies BEFORE the track, even below
// 0, at a track's head) and the phase of its first output; everything inside a tile is small enough for 32 bits.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace avd_resample {

constexpr int kOutRate = 16000;
constexpr int kRates[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000};
constexpr int kNumRates = (int)(sizeof(kRates) / sizeof(kRates[0]));
constexpr double kCutoff = 0.97, kBeta = 9.0;
constexpr int kBaseTaps = 32;
constexpr int kMaxBank = 20480;                  // entries of the largest bank (11025: 640 phases of 32 taps)
constexpr int kTileThreads = 256;
constexpr long long kMaxOutputs = 0x7fffffff;    // the output-side cuts and the analyzer's sample count are ints

struct Ratio { int rate = 0, U = 0, D = 0, T = 0; };

inline int rate_index(int rate)
{
    for (int i = 0; i < kNumRates; i++)
        if (kRates[i] == rate) return i;
    return -1;
}

// -> false for a rate outside the list
inline bool ratio_of(int rate, Ratio& r)
{
    if (rate_index(rate) < 0) return false;
    int a = rate, b = kOutRate;
    while (b) { const int c = a % b; a = b; b = c; }
    r.rate = rate;
    r.U = kOutRate / a;
    r.D = rate / a;
    if (rate == kOutRate) { r.T = 0; return true; }
    const double f = std::min(1.0, kCutoff * (double)r.U / (double)r.D);
    r.T = 2 * (int)std::ceil((double)(kBaseTaps / 2) / f);
    return true;
}

// the upsampling rates: an entry reaches 32768 and 32768 * sum|q| passes 2^31, so entries want 32 bits and the accumulator 64
inline bool wide(const Ratio& r) { return r.U > r.D; }

// I0 by its power series, in double: sum ((x / 2)^k / k!)^2
inline double bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// q[phi][k] of the rule, [U][T] ints; every row sums to exactly 32768.  unrounded (optional): h / sum h * 32768 per entry
inline std::vector<int> build_taps(const Ratio& r, std::vector<double>* unrounded = nullptr)
{
    std::vector<int> q((size_t)r.U * (size_t)r.T);
    if (unrounded) unrounded->assign(q.size(), 0.0);
    if (r.T == 0) return q;
    const double f = std::min(1.0, kCutoff * (double)r.U / (double)r.D), i0b = bessel_i0(kBeta);
    std::vector<double> h((size_t)r.T);
    for (int phi = 0; phi < r.U; phi++) {
        double sum = 0.0;
        for (int k = 0; k < r.T; k++) {
            const double x = (double)(k - r.T / 2 + 1) - (double)phi / (double)r.U;
            const double t = f * x, w = 1.0 - (2.0 * x / (double)r.T) * (2.0 * x / (double)r.T);
            const double sinc = t == 0.0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t);
            h[(size_t)k] = w < 0.0 ? 0.0 : f * sinc * bessel_i0(kBeta * std::sqrt(w)) / i0b;
            sum += h[(size_t)k];
        }
        int total = 0, best = 0;
        int* row = q.data() + (size_t)phi * (size_t)r.T;
        for (int k = 0; k < r.T; k++) {
            const double v = h[(size_t)k] / sum * 32768.0;
            if (unrounded) (*unrounded)[(size_t)phi * (size_t)r.T + (size_t)k] = v;
            row[k] = (int)std::nearbyint(v);
            total += row[k];
            if (h[(size_t)k] > h[(size_t)best]) best = k;        // the lowest k on a tie
        }
        row[best] += 32768 - total;
    }
    return q;
}

// outputs per tile: a multiple of the workgroup's 256 lanes, at most 1024, and few enough that a tile's span stays near 4096 frames at the
// steep ratios (192000: 256 outputs over 3072 + 396 frames)
inline int tile_outputs(const Ratio& r)
{
    const long long fit = 4096LL * r.U / r.D / kTileThreads * kTileThreads;
    return (int)std::min<long long>(1024, std::max<long long>(kTileThreads, fit));
}
// frames a tile of `count` outputs that begins at phase `phase` reads
inline int tile_span(const Ratio& r, int count, int phase) { return r.T == 0 ? count : (phase + (count - 1) * r.D) / r.U + r.T; }
// ... and the most any tile of the rate reads
inline int max_span(const Ratio& r) { return tile_span(r, tile_outputs(r), r.U - 1); }

enum Refusal { kOk = 0, kCutBeyond = 1, kTooLong = 3 };      // 2 is avd_audio::kWindowsTooSmall, which the window plan of the OUTPUT decides next

struct Track { int first, count; };              // first output sample in the converted buffer, output samples: a row of debug buffer "audio_rs_tracks"
struct Tile {
    long long in0;                               // absolute frame (in the call's buffer) of M[0], the first frame of the tile's span
    long long begin, end;                        // the track's frames [begin, end): M is 0 outside
    long long out0;                              // first output sample in the converted buffer
    int count, phase;                            // outputs, and (m0 D) mod U of the first one
};
static_assert(sizeof(Track) == 8 && sizeof(Tile) == 40, "the tile table is uploaded, the track rows are fetched, as they are");

struct Plan {
    int refused = kOk;
    Ratio r;
    int tile_out = 0;
    long long n_in = 0, n_out = 0;
    std::vector<Track> tracks;
    std::vector<int> out_cuts;                   // the cut list of the converted buffer: tracks[t].first for t >= 1
    std::vector<Tile> tiles;
};

// n > 0 frames, ncuts strictly ascending positive cuts in FRAMES (what "audio_cut" accepted).  A refused plan holds nothing.
inline Plan plan_convert(long long n, const Ratio& r, const int* cuts, int ncuts)
{
    Plan p;
    p.r = r;
    for (int c = 0; c < ncuts; c++)
        if (cuts[c] >= n) { p.refused = kCutBeyond; return p; }
    long long total = 0;
    for (int t = 0; t <= ncuts; t++) {
        const long long begin = t == 0 ? 0 : cuts[t - 1], end = t == ncuts ? n : cuts[t];
        total += ((end - begin) * r.U + r.D - 1) / r.D;
    }
    if (total > kMaxOutputs) { p.refused = kTooLong; return p; }
    p.tile_out = tile_outputs(r);
    p.n_in = n;
    for (int t = 0; t <= ncuts; t++) {
        const long long begin = t == 0 ? 0 : cuts[t - 1], end = t == ncuts ? n : cuts[t];
        const long long count = ((end - begin) * r.U + r.D - 1) / r.D;
        if (t) p.out_cuts.push_back((int)p.n_out);
        p.tracks.push_back(Track{(int)p.n_out, (int)count});
        for (long long m0 = 0; m0 < count; m0 += p.tile_out) {
            const long long base = m0 * (long long)r.D;
            const long long i0 = base / r.U;
            Tile tile;
            tile.in0 = begin + i0 - (r.T ? r.T / 2 - 1 : 0);
            tile.begin = begin;
            tile.end = end;
            tile.out0 = p.n_out + m0;
            tile.count = (int)std::min<long long>(p.tile_out, count - m0);
            tile.phase = (int)(base % r.U);
            p.tiles.push_back(tile);
        }
        p.n_out += count;
    }
    return p;
}

// LDS of the kernel (bytes): taps [U][T] (2 or 4 bytes) | samples as narrowed [(max_span * channels + 16)] int16 | mono [max_span] int16 |
// results [tile_out + 8] int16, every part 16-byte aligned
inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
inline size_t lds_taps_bytes(const Ratio& r) { return up16((size_t)r.U * (size_t)r.T * (wide(r) ? 4 : 2)); }
inline size_t lds_samples_bytes(const Ratio& r, int channels) { return up16(((size_t)max_span(r) * (size_t)channels + 16) * 2); }
inline size_t lds_mono_bytes(const Ratio& r) { return up16((size_t)max_span(r) * 2); }
inline size_t lds_bytes(const Ratio& r, int channels) { return lds_taps_bytes(r) + lds_samples_bytes(r, channels) + lds_mono_bytes(r) + up16(((size_t)tile_outputs(r) + 8) * 2); }

// ---- channel layouts (option "audio_layout", include/avd.h): the downmix as ONE rule, M = (sum_c w_c s_c + 16384) >> 15 with Q15 weights ----
// A layout's id is its channel count, in FFmpeg's / WAVE's native order: 1 mono | 2 FL FR | 6 FL FR FC LFE BL BR | 8 FL FR FC LFE BL BR SL SR.
// The gains (FC 1, FL / FR sqrt(1/2), back and side 1/2, LFE 0) are modelled on libswresample's default matrix for one output channel, unpinned
// against a real ffmpeg like the rest of the rule.  w_c = rint(g_c / sum g * 32768), and 32768 - sum w goes to the channel with the largest gain
// (the lowest index on a tie), as a bank row's remainder goes to its largest tap: every row sums to exactly 32768, |sum w s| <= 2^30.
constexpr int kLayoutPlanar = 0x100;             // flag of the option's value: one plane per channel
constexpr int kMaxChannels = 8;

inline bool layout_id_ok(int id) { return id == 1 || id == 2 || id == 6 || id == 8; }
// what option "audio_layout" accepts: 0 ("audio_channels" decides), or id | flags
inline bool layout_ok(int v) { return v == 0 || (v > 0 && layout_id_ok(v & ~kLayoutPlanar)); }

// the gains of layout `id`, in its channel order -> the channel count; 0 for an unknown id
inline int layout_gains(int id, double g[kMaxChannels])
{
    const double c = 1.0, f = std::sqrt(0.5), s = 0.5, lfe = 0.0;
    const double six[6] = {f, f, c, lfe, s, s}, eight[8] = {f, f, c, lfe, s, s, s, s};
    for (int i = 0; i < kMaxChannels; i++) g[i] = 0.0;
    switch (id) {
    case 1: g[0] = 1.0; return 1;
    case 2: g[0] = g[1] = f; return 2;
    case 6: std::copy(six, six + 6, g); return 6;
    case 8: std::copy(eight, eight + 8, g); return 8;
    default: return 0;
    }
}
// w[0 .. channels) of layout `id`, zero-filled to kMaxChannels -> the channel count; 0 for an unknown id
inline int layout_weights(int id, int w[kMaxChannels])
{
    double g[kMaxChannels];
    const int channels = layout_gains(id, g);
    for (int i = 0; i < kMaxChannels; i++) w[i] = 0;
    if (!channels) return 0;
    double sum = 0.0;
    for (int c = 0; c < channels; c++) sum += g[c];
    int total = 0, best = 0;
    for (int c = 0; c < channels; c++) {
        w[c] = (int)std::nearbyint(g[c] / sum * 32768.0);
        total += w[c];
        if (g[c] > g[best]) best = c;                            // the lowest index on a tie
    }
    w[best] += 32768 - total;
    return channels;
}

// What the converter's source phase goes by, as it travels to the kernels (by value).  id 0: no layout -- the launch takes today's path and its
// `channels` argument decides.  planar: plane c begins c * stride samples behind plane 0; interleaved: frames of `channels` samples, stride unused.
struct Mix { long long stride = 0; int id = 0, planar = 0, channels = 0, pad = 0; int w[kMaxChannels] = {}; };
static_assert(sizeof(Mix) == 56, "a kernel argument");

// option value (layout_ok, not 0) and the plane stride in effect -> the mix
inline Mix mix_of(int layout, long long stride)
{
    Mix m;
    m.id = layout & ~kLayoutPlanar;
    m.planar = (layout & kLayoutPlanar) != 0;
    m.channels = layout_weights(m.id, m.w);
    m.stride = m.planar ? stride : 0;
    return m;
}

// LDS of a layout launch: taps | acc [max_span] int32, w_c s_c summed per span frame | weights [8] int32 | mono | results.  The span's samples
// go from global memory straight into acc (no staging area), so any layout stays below today's stereo footprint plus the accumulators:
// lds_layout_bytes(r) <= lds_bytes(r, 2) + 4 * max_span(r) + 16 at every rate.
inline size_t lds_acc_bytes(const Ratio& r) { return up16((size_t)max_span(r) * 4); }
inline size_t lds_weights_bytes() { return (size_t)kMaxChannels * 4; }
inline size_t lds_layout_bytes(const Ratio& r) { return lds_taps_bytes(r) + lds_acc_bytes(r) + lds_weights_bytes() + lds_mono_bytes(r) + up16(((size_t)tile_outputs(r) + 8) * 2); }

}  // namespace avd_resample
