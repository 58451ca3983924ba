// avd_audio.hip -- per-window spectral features of the audio analyzer (gfx950): SURVEY.md section 8f row N3.
//
// Replaces the loop body of reference app/analyzers/audio.py:40-61 for ALL half-second windows of a 16 kHz mono
// float32 waveform at once (the reference walks them one by one in Python):
//   rms, zero-crossing sum              audio.py:44-46   (sum of squares / |diff(sign)| per window)
//   seg * np.hanning, np.fft.rfft, |.|  audio.py:47-49   -> magnitudes, double
//   flatness / rolloff / centroid sums  audio.py:50-61   -> sum log(mag), sum mag, sum freq*mag, first index reaching 85 %
// The scalar tail (percentiles, variances, tts_like, timeline; audio.py:63-110) is O(windows) numpy on the host
// (avd_hip/audio.py), exactly the reference's calls.
//
// The transform: a window is 8000 samples (0.5 s at 16 kHz) = 80 x 100, a real DFT of 4001 bins, in double with EXACT
// twiddles (cos(2 pi j / 8000) tabulated once on the host; the sine is the entry a quarter period away):
//  * full windows: a hundred 80-point DFTs, a twiddle and eighty 100-point DFTs (k_audio_fft_a / _b), each small DFT a
//    direct sum whose factors are entries of that one table -- 2.9 M multiply-adds per window, 0.58 ms per 60 s track;
//  * any other length (the short last window of a stream, or a caller's own window size): the direct 4001 x L sum
//    (k_audio_dft: one lane per bin, window and table in LDS; 64 M multiply-adds per 8000-sample window, 3.4 ms per track
//    when every window goes this way).  Windows whose length is not a multiple of 4 read the sine from a second table.
// Either way the difference to numpy's pocketfft is the order of additions: per bin at most 6.8e-16 * sum|xw| on the 80 x 100
// path and 4.8e-15 * sum|xw| on the direct one, measured bin by bin by tests/test_gpu_audio_spectrum.py (whose docstring is
// the record of these figures; its bound is 1e-12), far inside the 1e-4 tolerance of the path.
//
// One call may hold several tracks (option "audio_cut"), each windowed from its own start, as float32 or as 16-bit PCM (option "audio_format").
// csrc/avd_audio_plan.h lays the call out; the kernels go by its window table, and every window is computed exactly as it would be if its
// track were the only one of the call.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include "avd_internal.h"

#pragma clang fp contract(off)

namespace {

// Every pass takes its windows from the call's window table (avd_audio_plan.h): where a window begins in the staged buffer, how long it is, and
// which tables it reads -- the full-length set (hann | cos | sin, `win` entries each, cached per win) or its own length's set in the call's arena.
using avd_audio::Window;
using avd_audio::kTabFull;

// a sample as the float32 the reference analyses: float32 as it is; int16 PCM s is (float)s * 2^-15, exact for all 65536 values (what
// soundfile's dtype="float32" read gives), widened in registers -- no float32 copy of an int16 track exists in memory
__device__ __forceinline__ float audio_sample(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float audio_sample(const int16_t* p, int64_t i) { return (float)p[i] * 0x1p-15f; }

// ---- pass 1: time-domain sums and the windowed segment ----------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_audio_prepare(const T* __restrict__ wav, const Window* __restrict__ wt, int win,
                                                      const double* __restrict__ tab_full, const double* __restrict__ arena,
                                                      double* __restrict__ xw, avd_audio_window* __restrict__ out)
{
    __shared__ double ssum[4];
    __shared__ int szc[4];
    const int wdx = blockIdx.x, tid = threadIdx.x;
    const Window w = wt[wdx];
    const int len = w.len;
    const double* hann = w.tab == kTabFull ? tab_full : arena + w.tab;
    double sq = 0.;
    int zc = 0;
    for (int i = tid; i < len; i += 256) {
        const float v = audio_sample(wav, w.off + i);
        sq += (double)(v * v);                              // seg**2 is float32 in the reference; summed in double here
        xw[(int64_t)wdx * win + i] = (double)v * hann[i];
        if (i + 1 < len) {
            const float u = audio_sample(wav, w.off + i + 1);
            const int sv = (v > 0.f) - (v < 0.f), su = (u > 0.f) - (u < 0.f);
            zc += abs(su - sv);                             // |diff(sign(seg))|, values 0, 1, 2
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sq += __shfl_down(sq, o, 64); zc += __shfl_down(zc, o, 64); }
    if ((tid & 63) == 0) { ssum[tid >> 6] = sq; szc[tid >> 6] = zc; }
    __syncthreads();
    if (tid == 0) {
        out[wdx].sumsq = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
        out[wdx].zero_cross = szc[0] + szc[1] + szc[2] + szc[3];
        out[wdx].length = len;
        out[wdx].nbins = len / 2 + 1;
    }
}

// ---- pass 2: |rfft| + 1e-9 by direct evaluation -----------------------------------------------------------------
// grid (windows of `list`, ceil(max_bins / 256)); LDS: window [L] + cosine table [L] (dynamic, 16 * lds_len bytes, lds_len = the longest of them)
__global__ __launch_bounds__(256) void k_audio_dft(const double* __restrict__ xw, const Window* __restrict__ wt, const int* __restrict__ list, int win,
                                                  int lds_len, const double* __restrict__ tab_full, const double* __restrict__ arena,
                                                  double* __restrict__ mag)
{
    extern __shared__ __align__(16) double lds[];
    const int wdx = list[blockIdx.x], tid = threadIdx.x;   // the call's windows that do not go through the FFT path
    const Window w = wt[wdx];
    const int L = w.len;
    const int nb = L / 2 + 1;
    if ((int)blockIdx.y * 256 >= nb) return;                // whole workgroup
    const bool full = w.tab == kTabFull;
    const double* ct = full ? tab_full + win : arena + w.tab + L;
    double* x = lds;
    double* c = lds + lds_len;
    for (int i = tid; i < L; i += 256) { x[i] = xw[(int64_t)wdx * win + i]; c[i] = ct[i]; }
    __syncthreads();
    const int k = blockIdx.y * 256 + tid;
    if (k >= nb) return;
    double re = 0., im = 0.;
    if ((L & 3) == 0) {
        // sin(2 pi j / L) = cos(2 pi (j - L/4) / L): one table serves both
        const int q = L >> 2;
        int j = 0, js = L - q;                              // js = (j - q) mod L
        for (int i = 0; i < L; i++) {
            const double v = x[i];
            re += v * c[j];
            im -= v * c[js];
            j += k; if (j >= L) j -= L;
            js += k; if (js >= L) js -= L;
        }
    } else {
        // a length that is not a multiple of 4 has no quarter period in its cosine table: sines of THIS length from
        // global memory (full windows of a caller-chosen size as well as the short last window of a track)
        const double* st = full ? tab_full + 2 * win : arena + w.tab + 2 * L;
        int j = 0;
        for (int i = 0; i < L; i++) {
            const double v = x[i];
            re += v * c[j];
            im -= v * st[j];
            j += k; if (j >= L) j -= L;
        }
    }
    mag[(int64_t)wdx * (win / 2 + 1) + k] = hypot(re, im) + 1e-9;
}

// ---- pass 2, fast path: full windows of 8000 samples ---------------------------------------------------------------
// 8000 = 80 x 100.  With n = 100 n1 + n2 and k = k1 + 80 k2:
//   X[k1 + 80 k2] = sum_{n2} W_100^(n2 k2) * ( W_8000^(n2 k1) * sum_{n1} x[100 n1 + n2] W_80^(n1 k1) )
// i.e. a hundred 80-point DFTs, a twiddle, and eighty 100-point DFTs of which only k2 <= 50 is needed (bins 0..4000):
// 2.9 M real multiply-adds per window instead of 64 M, each of the small DFTs evaluated directly in double with entries of
// the SAME 8000-entry cosine table the direct form uses (W_80^m = W_8000^(100 m), W_100^m = W_8000^(80 m), sines a quarter
// period away): no approximation anywhere, the result differs from the direct sum only by the order of additions
// (figures above).  The intermediate B[n2][k1] (16 bytes per entry, 128 KB per window) goes through global memory / L2.
constexpr int kFftN = avd_audio::kFftLen, kN1 = 80, kN2 = 100;
static_assert(kFftN == kN1 * kN2, "the two-step transform is written for 80 x 100");

// Both kernels run over the compacted list of the call's full windows: workgroup b transforms window list[b], its intermediate is B[b]
__global__ __launch_bounds__(256) void k_audio_fft_a(const double* __restrict__ xw, const int* __restrict__ list, const double* __restrict__ cos_full,
                                                    double2* __restrict__ B)
{
    extern __shared__ __align__(16) double lds[];          // window [8000] | cosine table [8000]
    double* x = lds;
    double* c = lds + kFftN;
    const int wdx = list[blockIdx.x], tid = threadIdx.x;
    for (int i = tid; i < kFftN; i += 256) { x[i] = xw[(int64_t)wdx * kFftN + i]; c[i] = cos_full[i]; }
    __syncthreads();
    double2* out = B + (int64_t)blockIdx.x * kFftN;
    for (int o = tid; o < kFftN; o += 256) {
        const int k1 = o / kN2, n2 = o - k1 * kN2;          // consecutive lanes: consecutive n2, (almost) the same k1
        double re = 0., im = 0.;
        int j = 0;                                           // (n1 k1 mod 80) * 100: the index of W_80^(n1 k1) in the table
        const int stepj = k1 * 100;
        for (int n1 = 0; n1 < kN1; n1++) {
            const double v = x[n1 * kN2 + n2];
            const int js = j >= 2000 ? j - 2000 : j + 6000;  // sin(t) = cos(t - pi / 2)
            re += v * c[j];
            im -= v * c[js];
            j += stepj; if (j >= kFftN) j -= kFftN;
        }
        // twiddle W_8000^(n2 k1) = cos - i sin
        const int t = n2 * k1, ts = t >= 2000 ? t - 2000 : t + 6000;
        const double tc = c[t], tsn = c[ts];
        double2 r;
        r.x = re * tc + im * tsn;
        r.y = im * tc - re * tsn;
        out[n2 * kN1 + k1] = r;
    }
}

__global__ __launch_bounds__(256) void k_audio_fft_b(const double2* __restrict__ B, const int* __restrict__ list, const double* __restrict__ cos_full,
                                                    double* __restrict__ mag)
{
    extern __shared__ __align__(16) double lds[];          // cosine table [8000]
    double* c = lds;
    const int wdx = list[blockIdx.x], tid = threadIdx.x;
    for (int i = tid; i < kFftN; i += 256) c[i] = cos_full[i];
    __syncthreads();
    const double2* in = B + (int64_t)blockIdx.x * kFftN;
    for (int k = tid; k <= kFftN / 2; k += 256) {
        const int k2 = k / kN1, k1 = k - k2 * kN1;          // consecutive lanes: consecutive k1 -> consecutive B entries
        double re = 0., im = 0.;
        int j = 0;                                           // (n2 k2 mod 100) * 80
        const int stepj = k2 * 80;
        for (int n2 = 0; n2 < kN2; n2++) {
            const double2 b = in[n2 * kN1 + k1];
            const int js = j >= 2000 ? j - 2000 : j + 6000;
            const double wc = c[j], ws = c[js];              // W_100^(n2 k2) = wc - i ws
            re += b.x * wc + b.y * ws;
            im += b.y * wc - b.x * ws;
            j += stepj; if (j >= kFftN) j -= kFftN;
        }
        mag[(int64_t)wdx * (kFftN / 2 + 1) + k] = hypot(re, im) + 1e-9;
    }
}

// ---- pass 3: spectral sums and the roll-off index ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_audio_reduce(const double* __restrict__ mag, const Window* __restrict__ wt, int win, avd_audio_window* __restrict__ out)
{
    __shared__ double sl[4], sm[4], sf[4];
    __shared__ double total;
    const int wdx = blockIdx.x, tid = threadIdx.x;
    const int nb = wt[wdx].len / 2 + 1;
    const double* m = mag + (int64_t)wdx * (win / 2 + 1);
    // np.linspace(0, 1, nb): k * step with step = 1 / (nb - 1), the last element exactly 1
    const double step = nb > 1 ? 1.0 / (double)(nb - 1) : 0.0;
    double a = 0., b = 0., f = 0.;
    for (int k = tid; k < nb; k += 256) {
        const double v = m[k];
        a += log(v);
        b += v;
        f += (k == nb - 1 && nb > 1 ? 1.0 : (double)k * step) * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); f += __shfl_down(f, o, 64); }
    if ((tid & 63) == 0) { sl[tid >> 6] = a; sm[tid >> 6] = b; sf[tid >> 6] = f; }
    __syncthreads();
    if (tid == 0) {
        out[wdx].sum_log = (sl[0] + sl[1]) + (sl[2] + sl[3]);
        total = (sm[0] + sm[1]) + (sm[2] + sm[3]);
        out[wdx].sum_mag = total;
        out[wdx].sum_fmag = (sf[0] + sf[1]) + (sf[2] + sf[3]);
        // audio.py:52-58: sequential running sum (python floats = double), first k with s >= 0.85 * sum; 0 if never
        const double cutoff = 0.85 * total;
        double s = 0.;
        int idx = 0;
        for (int k = 0; k < nb; k++) {
            s += m[k];
            if (s >= cutoff) { idx = k; break; }
        }
        out[wdx].rolloff_index = idx;
    }
}

// ---- the converter in front of pass 1 (options "audio_rate" / "audio_channels"): decoder frames -> 16 kHz mono int16 ------------------------
// One workgroup per tile of avd_audio_resample.h: a run of at most tile_outputs() output samples of one track.  LDS (laid out by the header's
// lds_* functions): the rate's filter bank | the span's samples as narrowed | the span downmixed | the tile's results.
//  * the span is read ONCE, with 16-byte loads where a whole 16-byte line of the buffer lies inside the track's part of the span, sample by
//    sample in the partial line at either end (the buffer is aligned for its sample type only, and tracks begin wherever they were cut);
//  * narrowing and downmix happen once per frame; the sums are exact integer multiply-adds -- 32 bits where 32768 * sum|q| stays below 2^31
//    (every downsampling rate), 64 bits with 32-bit bank entries at the three upsampling rates;
//  * lane l forms outputs l, l + 256, ...: consecutive lanes read LDS D / U frames apart (three halfwords at 48 kHz, where the bank row is the
//    same for all lanes and broadcasts; at 44.1 kHz the gathered rows are 92 halfwords long, an odd number of banks apart);
//  * the results leave as 16-byte rows of the converted buffer; the row a tile shares with its neighbour is written entry by entry.
// A continued track (option "audio_slot", avd_audio_stream.h) has a two-part source: tiles carry positions relative to the TRACK, `wav` holds its
// frames from `chunk0` on, and the hist_n frames below chunk0 come from the slot's history -- mono int16 already, so they go straight into
// mono[].  Both extents are the same for every lane of the workgroup.  A whole track is chunk0 = 0 with no history.
using avd_resample::Tile;

// step 1 of the rule: int16 is itself; float32 x is clamp(rint(x * 32768), -32768, 32767), ties to even, NaN -> 0
__device__ __forceinline__ int narrow_sample(int16_t s) { return s; }
__device__ __forceinline__ int narrow_sample(float x)
{
    const float v = rintf(x * 32768.f);
    return v != v ? 0 : (int)fminf(fmaxf(v, -32768.f), 32767.f);
}

// The source phase of a layout launch (option "audio_layout"): the downmix of the span's frames [f_lo, f_hi), which `wav` holds from chunk0 on,
// as acc[f - f_lo] = sum_c w_c s_c -- the samples go from global memory straight into the sums, no staging area.  A run is what is contiguous:
// the track's part of ONE plane (planar; plane c begins c * stride samples behind plane 0, so every plane has its own misalignment), or the
// whole interleaved stretch.  Every sample of a run is read once: in 16-byte loads where a whole 16-byte line lies inside the run, sample by
// sample in the partial line at either end.  A plane whose weight is 0 (LFE) is not read at all; interleaved, its samples come with their
// lines and are dropped.  The sums are LDS integer adds: lines of an interleaved run straddle frames and planes meet in every frame, and integer
// addition does not care about the order.  wl: the weights in LDS (a lane's channel is data).  The caller's barrier follows.
template <typename S>
__device__ __forceinline__ void mix_span(const S* __restrict__ wav, const avd_resample::Mix& mix, long long chunk0, long long f_lo, long long f_hi, int* __restrict__ acc,
                                         const int* __restrict__ wl)
{
    const int tid = threadIdx.x;
    constexpr int per = 16 / (int)sizeof(S);                // samples in a 16-byte line
    const int frames = f_hi > f_lo ? (int)(f_hi - f_lo) : 0;
    const int C = mix.channels;
    const int runs = mix.planar ? C : 1, run_len = mix.planar ? frames : frames * C;
    for (int r = 0; r < runs; r++) {
        if (mix.planar && wl[r] == 0) continue;             // the same for every lane
        const S* run = mix.planar ? wav + (long long)r * mix.stride + (f_lo - chunk0) : wav + (f_lo - chunk0) * C;
        const int lead = (int)((reinterpret_cast<uintptr_t>(run) & 15) / sizeof(S));   // the run begins `lead` samples above a line boundary
        const int lines = run_len > 0 ? (lead + run_len + per - 1) / per : 0;
        for (int l = tid; l < lines; l += 256) {
            const int lo = l * per - lead;                  // the line's first sample, counted in the run
            const int first = lo > 0 ? lo : 0;
            int f = mix.planar ? first : first / C, c = mix.planar ? r : first - f * C;   // frame (counted from f_lo) and channel of sample `first`
            if (lo >= 0 && lo + per <= run_len) {
                int v[per];
                const uint4 q = *reinterpret_cast<const uint4*>(run + lo);
                if constexpr (sizeof(S) == 2) {
                    v[0] = (int16_t)(q.x & 0xffff); v[1] = (int)q.x >> 16; v[2] = (int16_t)(q.y & 0xffff); v[3] = (int)q.y >> 16;
                    v[4] = (int16_t)(q.z & 0xffff); v[5] = (int)q.z >> 16; v[6] = (int16_t)(q.w & 0xffff); v[7] = (int)q.w >> 16;
                } else {
                    v[0] = narrow_sample(__uint_as_float(q.x)); v[1] = narrow_sample(__uint_as_float(q.y));
                    v[2] = narrow_sample(__uint_as_float(q.z)); v[3] = narrow_sample(__uint_as_float(q.w));
                }
#pragma unroll
                for (int e = 0; e < per; e++) {
                    const int w = wl[c];
                    if (w) atomicAdd(&acc[f], w * v[e]);
                    if (mix.planar) f++;
                    else if (++c == C) { c = 0; f++; }
                }
            } else {
                const int stop = lo + per < run_len ? lo + per : run_len;
                for (int s = first; s < stop; s++) {
                    const int w = wl[c];
                    if (w) atomicAdd(&acc[f], w * narrow_sample(run[s]));
                    if (mix.planar) f++;
                    else if (++c == C) { c = 0; f++; }
                }
            }
        }
    }
}

// one tile, by the whole workgroup: the body of the converter kernels below.  kLayout: the source phase is mix_span's (samples_at is where acc
// lies, the weights behind it); without it `mix` is not read and the code is what it was before layouts existed.
template <typename S, typename Q, typename Acc, bool kLayout = false>
__device__ __forceinline__ void resample_tile(const S* __restrict__ wav, const Tile t, const int* __restrict__ taps, int U, int D, int T, int channels, int samples_at,
                                              int mono_at, int res_at, int16_t* __restrict__ pcm, long long chunk0, const int16_t* __restrict__ hist, int hist_n,
                                              const avd_resample::Mix& mix = avd_resample::Mix{})
{
    extern __shared__ __align__(16) unsigned char rs_lds[];
    Q* q = reinterpret_cast<Q*>(rs_lds);
    int16_t* smp = reinterpret_cast<int16_t*>(rs_lds + samples_at);
    int16_t* mono = reinterpret_cast<int16_t*>(rs_lds + mono_at);
    int16_t* res = reinterpret_cast<int16_t*>(rs_lds + res_at);
    const int tid = threadIdx.x;
    for (int i = tid; i < U * T; i += 256) q[i] = (Q)taps[i];
    const int span = T == 0 ? t.count : (t.phase + (t.count - 1) * D) / U + T;
    // the span's frames that `wav` holds: [f_lo, f_hi) of the track; samples [s0, s1) of the buffer
    const long long f_min = t.begin > chunk0 ? t.begin : chunk0;
    const long long f_lo = t.in0 > f_min ? t.in0 : f_min, f_hi = t.in0 + span < t.end ? t.in0 + span : t.end;
    const long long h_lo = chunk0 - hist_n;                 // the history holds frames [h_lo, chunk0)
    if constexpr (kLayout) {
        int* acc = reinterpret_cast<int*>(rs_lds + samples_at);
        int* wl = acc + (mono_at - samples_at) / 4 - avd_resample::kMaxChannels;
        const int frames = f_hi > f_lo ? (int)(f_hi - f_lo) : 0;
        for (int i = tid; i < frames; i += 256) acc[i] = 0;
        if (tid < avd_resample::kMaxChannels) {
            int w = 0;
#pragma unroll
            for (int c = 0; c < avd_resample::kMaxChannels; c++) w = tid == c ? mix.w[c] : w;
            wl[tid] = w;
        }
        __syncthreads();
        mix_span<S>(wav, mix, chunk0, f_lo, f_hi, acc, wl);
        __syncthreads();
        // step 2: M = (sum_c w_c s_c + 16384) >> 15; 0 outside the track
        for (int i = tid; i < span; i += 256) {
            const long long f = t.in0 + i;
            int m = 0;
            if (f >= f_lo && f < f_hi) m = (acc[(int)(f - f_lo)] + 16384) >> 15;
            else if (f >= h_lo && f < chunk0) m = hist[f - h_lo];
            mono[i] = (int16_t)m;
        }
        __syncthreads();
    } else {
        const long long s0 = (f_lo - chunk0) * channels, s1 = (f_hi - chunk0) * channels;
        constexpr int per = 16 / (int)sizeof(S);                // samples in a 16-byte line
        const int lead = (int)((reinterpret_cast<uintptr_t>(wav + s0) & 15) / sizeof(S));   // smp[0] is the sample at the line boundary at or below s0
        const int lines = s1 > s0 ? (lead + (int)(s1 - s0) + per - 1) / per : 0;
        for (int c = tid; c < lines; c += 256) {
            const long long lo = s0 - lead + (long long)c * per;
            int16_t* dst = smp + c * per;
            if (lo >= s0 && lo + per <= s1) {
                const uint4 v = *reinterpret_cast<const uint4*>(wav + lo);
                if constexpr (sizeof(S) == 2) {
                    *reinterpret_cast<uint4*>(dst) = v;
                } else {
                    const int a = narrow_sample(__uint_as_float(v.x)), b = narrow_sample(__uint_as_float(v.y));
                    const int c2 = narrow_sample(__uint_as_float(v.z)), d = narrow_sample(__uint_as_float(v.w));
                    uint2 o;
                    o.x = (unsigned)(a & 0xffff) | ((unsigned)b << 16);
                    o.y = (unsigned)(c2 & 0xffff) | ((unsigned)d << 16);
                    *reinterpret_cast<uint2*>(dst) = o;
                }
            } else {
                for (int e = 0; e < per; e++) {
                    const long long s = lo + e;
                    dst[e] = s >= s0 && s < s1 ? (int16_t)narrow_sample(wav[s]) : (int16_t)0;
                }
            }
        }
        __syncthreads();
        // step 2: M = s, or floor((L + R + 1) / 2); 0 outside the track
        for (int i = tid; i < span; i += 256) {
            const long long f = t.in0 + i;
            int m = 0;
            if (f >= f_lo && f < f_hi) {
                const int at = lead + (int)(f - f_lo) * channels;
                m = channels == 2 ? ((int)smp[at] + (int)smp[at + 1] + 1) >> 1 : (int)smp[at];
            } else if (f >= h_lo && f < chunk0) {
                m = hist[f - h_lo];
            }
            mono[i] = (int16_t)m;
        }
        __syncthreads();
    }
    // step 4; res[e] is entry e of the converted buffer counted from the 16-byte row boundary at or below the tile's first output
    const int shift = (int)(t.out0 & 7);
    for (int j = tid; j < t.count; j += 256) {
        int y;
        if (T == 0) y = mono[j];
        else {
            const int pos = t.phase + j * D, idx = pos / U, phi = pos - idx * U;
            const Q* row = q + phi * T;
            const int16_t* x = mono + idx;
            Acc acc = 0;
            for (int k = 0; k < T; k++) acc += (Acc)row[k] * (Acc)x[k];
            const Acc v = (acc + 16384) >> 15;
            y = v < -32768 ? -32768 : v > 32767 ? 32767 : (int)v;
        }
        res[shift + j] = (int16_t)y;
    }
    __syncthreads();
    int16_t* out = pcm + (t.out0 - shift);
    const int last = shift + t.count;
    for (int r = tid; r < (last + 7) / 8; r += 256) {
        const int e0 = r * 8;
        if (e0 >= shift && e0 + 8 <= last) *reinterpret_cast<uint4*>(out + e0) = *reinterpret_cast<const uint4*>(res + e0);
        else
            for (int e = e0 > shift ? e0 : shift; e < e0 + 8 && e < last; e++) out[e] = res[e];
    }
}

template <typename S, typename Q, typename Acc>
__global__ __launch_bounds__(256) void k_audio_resample(const S* __restrict__ wav, const Tile* __restrict__ tiles, const int* __restrict__ taps, int U, int D,
                                                       int T, int channels, int samples_at, int mono_at, int res_at, int16_t* __restrict__ pcm,
                                                       long long chunk0, const int16_t* __restrict__ hist, int hist_n)
{
    resample_tile<S, Q, Acc>(wav, tiles[blockIdx.x], taps, U, D, T, channels, samples_at, mono_at, res_at, pcm, chunk0, hist, hist_n);
}

// A call of several tracks (option "audio_track_slot", avd_audio_map.h) has a source PER TRACK: tile_track[tile] is the tile's track, rows[track]
// says where the track's chunk begins in the call's buffer, how many frames its slot absorbed before, and where its history is -- in place of the
// three per-launch arguments above.  Both reads are the same for every lane of the workgroup; the bank and the LDS layout are the launch's.
using avd_audio_map::Source;

template <typename S, typename Q, typename Acc>
__global__ __launch_bounds__(256) void k_audio_resample_map(const S* __restrict__ wav, const Tile* __restrict__ tiles, const int* __restrict__ tile_track,
                                                           const Source* __restrict__ rows, const int* __restrict__ taps, int U, int D, int T, int channels,
                                                           int samples_at, int mono_at, int res_at, int16_t* __restrict__ pcm)
{
    const Source row = rows[tile_track[blockIdx.x]];
    resample_tile<S, Q, Acc>(wav + row.at, tiles[blockIdx.x], taps, U, D, T, channels, samples_at, mono_at, res_at, pcm, row.chunk0,
                             reinterpret_cast<const int16_t*>(row.hist), row.hist_n);
}

// The same two kernels for a call with a layout (option "audio_layout"): the mix travels by value, `samples_at` is where the sums lie
template <typename S, typename Q, typename Acc>
__global__ __launch_bounds__(256) void k_audio_resample_layout(const S* __restrict__ wav, const Tile* __restrict__ tiles, const int* __restrict__ taps, int U, int D,
                                                              int T, const avd_resample::Mix mix, int acc_at, int mono_at, int res_at, int16_t* __restrict__ pcm,
                                                              long long chunk0, const int16_t* __restrict__ hist, int hist_n)
{
    resample_tile<S, Q, Acc, true>(wav, tiles[blockIdx.x], taps, U, D, T, mix.channels, acc_at, mono_at, res_at, pcm, chunk0, hist, hist_n, mix);
}

// row.at counts FRAMES of a planar buffer (applied to every plane alike), samples of an interleaved one
template <typename S, typename Q, typename Acc>
__global__ __launch_bounds__(256) void k_audio_resample_map_layout(const S* __restrict__ wav, const Tile* __restrict__ tiles, const int* __restrict__ tile_track,
                                                                  const Source* __restrict__ rows, const int* __restrict__ taps, int U, int D, int T,
                                                                  const avd_resample::Mix mix, int acc_at, int mono_at, int res_at, int16_t* __restrict__ pcm)
{
    const Source row = rows[tile_track[blockIdx.x]];
    resample_tile<S, Q, Acc, true>(wav + row.at, tiles[blockIdx.x], taps, U, D, T, mix.channels, acc_at, mono_at, res_at, pcm, row.chunk0,
                                   reinterpret_cast<const int16_t*>(row.hist), row.hist_n, mix);
}

// where a layout launch's parts lie in LDS (avd_audio_resample.h): taps | acc | weights | mono | results
struct LayoutLds { int acc_at, mono_at, res_at; size_t bytes; };
static LayoutLds layout_lds(const avd_resample::Ratio& r)
{
    const size_t at_a = avd_resample::lds_taps_bytes(r), at_m = at_a + avd_resample::lds_acc_bytes(r) + avd_resample::lds_weights_bytes();
    return LayoutLds{(int)at_a, (int)at_m, (int)(at_m + avd_resample::lds_mono_bytes(r)), avd_resample::lds_layout_bytes(r)};
}

template <typename S, typename Q, typename Acc>
int launch_resample_map_as(avd_ctx* ctx, const void* d_in, const Tile* tiles, const int* tile_track, const Source* rows, const int* taps, int ntiles,
                           const avd_resample::Ratio& r, int channels, int16_t* d_pcm, const avd_resample::Mix& mix)
{
    if (mix.id) {
        const LayoutLds l = layout_lds(r);
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_audio_resample_map_layout<S, Q, Acc>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes));
        hipLaunchKernelGGL((k_audio_resample_map_layout<S, Q, Acc>), dim3(ntiles), dim3(256), l.bytes, ctx->stream, static_cast<const S*>(d_in), tiles, tile_track, rows,
                           taps, r.U, r.D, r.T, mix, l.acc_at, l.mono_at, l.res_at, d_pcm);
        return 0;
    }
    const size_t at_s = avd_resample::lds_taps_bytes(r), at_m = at_s + avd_resample::lds_samples_bytes(r, channels), at_r = at_m + avd_resample::lds_mono_bytes(r);
    const size_t lds = avd_resample::lds_bytes(r, channels);
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_audio_resample_map<S, Q, Acc>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_audio_resample_map<S, Q, Acc>), dim3(ntiles), dim3(256), lds, ctx->stream, static_cast<const S*>(d_in), tiles, tile_track, rows, taps, r.U,
                       r.D, r.T, channels, (int)at_s, (int)at_m, (int)at_r, d_pcm);
    return 0;
}

template <typename S, typename Q, typename Acc>
int launch_resample_as(avd_ctx* ctx, const void* d_in, const Tile* tiles, const int* taps, int ntiles, const avd_resample::Ratio& r, int channels, int16_t* d_pcm,
                       const AudioSource& src, const avd_resample::Mix& mix)
{
    if (mix.id) {
        const LayoutLds l = layout_lds(r);
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_audio_resample_layout<S, Q, Acc>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes));
        hipLaunchKernelGGL((k_audio_resample_layout<S, Q, Acc>), dim3(ntiles), dim3(256), l.bytes, ctx->stream, static_cast<const S*>(d_in), tiles, taps, r.U, r.D, r.T,
                           mix, l.acc_at, l.mono_at, l.res_at, d_pcm, src.chunk0, src.hist, src.hist_n);
        return 0;
    }
    const size_t at_s = avd_resample::lds_taps_bytes(r), at_m = at_s + avd_resample::lds_samples_bytes(r, channels), at_r = at_m + avd_resample::lds_mono_bytes(r);
    const size_t lds = avd_resample::lds_bytes(r, channels);
    // per call (a function attribute belongs to the current device; a process may hold contexts on several)
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_audio_resample<S, Q, Acc>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_audio_resample<S, Q, Acc>), dim3(ntiles), dim3(256), lds, ctx->stream, static_cast<const S*>(d_in), tiles, taps, r.U, r.D, r.T, channels,
                       (int)at_s, (int)at_m, (int)at_r, d_pcm, src.chunk0, src.hist, src.hist_n);
    return 0;
}

// ---- what a call leaves in its audio slot (option "audio_slot"): ONE launch, one workgroup --------------------------------------------------
//  * the new history: the track's last hist_new_n frames, narrowed and downmixed exactly as k_audio_resample does it -- frame r of the call's n
//    (r >= 0) from `wav`, frame r < 0 from the old history, which a chunk shorter than T - 1 shifts.  Old and new history are two buffers
//    (the slot alternates), so no lane reads what another writes; hist_new_n <= n + hist_old_n by the rule.
//  * the new held remainder: held_words 16-bit words of the analyzer's buffer behind its last window (a float32 sample is two of them).
template <typename S>
__device__ __forceinline__ void slot_save(const S* __restrict__ wav, long long n, int channels, const int16_t* __restrict__ hist_old, int hist_old_n,
                                          int16_t* __restrict__ hist_new, int hist_new_n, const int16_t* __restrict__ held_src, int16_t* __restrict__ held_dst,
                                          int held_words)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < hist_new_n; i += 256) {
        const long long r = n - hist_new_n + i;
        int m;
        if (r >= 0) m = channels == 2 ? (narrow_sample(wav[2 * r]) + narrow_sample(wav[2 * r + 1]) + 1) >> 1 : narrow_sample(wav[r]);
        else m = hist_old[hist_old_n + r];
        hist_new[i] = (int16_t)m;
    }
    for (int i = tid; i < held_words; i += 256) held_dst[i] = held_src[i];
}

// ... and of a call with a layout: the same frames by the layout's rule, M = (sum_c w_c s_c + 16384) >> 15, a channel of weight 0 not read
template <typename S>
__device__ __forceinline__ void slot_save_layout(const S* __restrict__ wav, long long n, const avd_resample::Mix& mix, const int16_t* __restrict__ hist_old, int hist_old_n,
                                                 int16_t* __restrict__ hist_new, int hist_new_n, const int16_t* __restrict__ held_src,
                                                 int16_t* __restrict__ held_dst, int held_words)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < hist_new_n; i += 256) {
        const long long r = n - hist_new_n + i;
        int m;
        if (r >= 0) {
            int sum = 16384;
#pragma unroll
            for (int c = 0; c < avd_resample::kMaxChannels; c++)
                if (c < mix.channels && mix.w[c] != 0) sum += mix.w[c] * narrow_sample(mix.planar ? wav[(long long)c * mix.stride + r] : wav[r * mix.channels + c]);
            m = sum >> 15;
        } else m = hist_old[hist_old_n + r];
        hist_new[i] = (int16_t)m;
    }
    for (int i = tid; i < held_words; i += 256) held_dst[i] = held_src[i];
}

template <typename S>
__global__ __launch_bounds__(256) void k_audio_slot_save_layout(const S* __restrict__ wav, long long n, const avd_resample::Mix mix, const int16_t* __restrict__ hist_old,
                                                               int hist_old_n, int16_t* __restrict__ hist_new, int hist_new_n, const int16_t* __restrict__ held_src,
                                                               int16_t* __restrict__ held_dst, int held_words)
{
    slot_save_layout<S>(wav, n, mix, hist_old, hist_old_n, hist_new, hist_new_n, held_src, held_dst, held_words);
}

template <typename S>
__global__ __launch_bounds__(256) void k_audio_slot_save(const S* __restrict__ wav, long long n, int channels, const int16_t* __restrict__ hist_old, int hist_old_n,
                                                        int16_t* __restrict__ hist_new, int hist_new_n, const int16_t* __restrict__ held_src,
                                                        int16_t* __restrict__ held_dst, int held_words)
{
    slot_save<S>(wav, n, channels, hist_old, hist_old_n, hist_new, hist_new_n, held_src, held_dst, held_words);
}

// ---- a call of several tracks (option "audio_track_slot"): ONE gather launch ahead of the converter, ONE save launch behind everything else -----
// The tables travel BY VALUE, as kernel arguments, like k_stream_copy's: 72 moves of 24 bytes (1728 bytes) and 8 save rows of 64 bytes (512 bytes)
// fit the 4 KB of arguments with room to spare, and no upload has to be ordered ahead of either launch.
//
// The save: workgroup b leaves track rows[b]'s new history and held remainder in its slot -- slot_save's arithmetic, once per continued track
// that does not end in this call.
struct SaveTable { AudioSaveRow row[avd_audio_map::kSlots]; };

template <typename S>
__global__ __launch_bounds__(256) void k_audio_slot_save_map(const SaveTable table, int channels)
{
    const AudioSaveRow r = table.row[blockIdx.x];
    slot_save<S>(static_cast<const S*>(r.wav), r.n, channels, r.hist_old, r.hist_old_n, r.hist_new, r.hist_new_n, r.held_src, r.held_dst, r.held_words);
}

template <typename S>
__global__ __launch_bounds__(256) void k_audio_slot_save_map_layout(const SaveTable table, const avd_resample::Mix mix)
{
    const AudioSaveRow r = table.row[blockIdx.x];
    slot_save_layout<S>(static_cast<const S*>(r.wav), r.n, mix, r.hist_old, r.hist_old_n, r.hist_new, r.hist_new_n, r.held_src, r.held_dst, r.held_words);
}

// The gather: move blockIdx.y of the table, by gridDim.x workgroups in strides.  Held samples go from their slot to the front of the track's region;
// an unconverted track's own samples from the call's buffer (staged, or the caller's device memory) behind them.  Where source and destination
// agree mod 16 the body moves in 16-byte lines, with elements (elem bytes each: 2, or 4 for float32) in the partial line at either end; where
// they do not -- a track cut at an odd sample -- it moves element by element.  Every address is a multiple of elem.
struct GatherTable { AudioGatherMove move[avd_audio_map::kMaxGather]; };

template <typename E>
__global__ __launch_bounds__(256) void k_audio_gather(const GatherTable table)
{
    const AudioGatherMove m = table.move[blockIdx.y];
    const char* src = static_cast<const char*>(m.src);
    char* dst = static_cast<char*>(m.dst);
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    constexpr long long elem = sizeof(E);
    if (((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const long long to_line = (long long)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
        const long long head = to_line < m.bytes ? to_line : m.bytes, lines = (m.bytes - head) / 16, tail_at = head + 16 * lines;
        for (long long i = id; i < lines; i += stride)
            *reinterpret_cast<uint4*>(dst + head + 16 * i) = *reinterpret_cast<const uint4*>(src + head + 16 * i);
        const long long edge = (head + (m.bytes - tail_at)) / elem;          // elements of the two partial lines
        for (long long e = id; e < edge; e += stride) {
            const long long at = e * elem < head ? e * elem : tail_at + (e * elem - head);
            *reinterpret_cast<E*>(dst + at) = *reinterpret_cast<const E*>(src + at);
        }
    } else {
        for (long long e = id; e < m.bytes / elem; e += stride) *reinterpret_cast<E*>(dst + e * elem) = *reinterpret_cast<const E*>(src + e * elem);
    }
}

}  // namespace

int launch_audio_gather(avd_ctx* ctx, const AudioGatherMove* moves, int count, int elem)
{
    if (count <= 0) return 0;
    if (count > avd_audio_map::kMaxGather || (elem != 2 && elem != 4)) { ctx->err = "audio_track_slot: internal error (gather table)"; return AVD_ERR_DEVICE; }
    GatherTable table = {};
    long long longest = 0;
    for (int i = 0; i < count; i++) {
        const AudioGatherMove& m = moves[i];
        if (m.bytes <= 0 || m.bytes % elem || reinterpret_cast<uintptr_t>(m.src) % elem || reinterpret_cast<uintptr_t>(m.dst) % elem) {
            ctx->err = "audio_track_slot: internal error (gather extents)";
            return AVD_ERR_DEVICE;
        }
        table.move[i] = m;
        longest = std::max(longest, m.bytes);
    }
    // a workgroup per 16 KB of the longest move, 64 at the most: held samples are one workgroup, a minute of float32 samples 64 in strides
    const unsigned wgs = (unsigned)std::min<long long>(64, (longest + 16383) / 16384);
    if (elem == 2) hipLaunchKernelGGL(k_audio_gather<uint16_t>, dim3(wgs, (unsigned)count), dim3(256), 0, ctx->stream, table);
    else hipLaunchKernelGGL(k_audio_gather<uint32_t>, dim3(wgs, (unsigned)count), dim3(256), 0, ctx->stream, table);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

int launch_audio_slot_save_map(avd_ctx* ctx, int format, int channels, const AudioSaveRow* rows, int count, bool* enqueued, const avd_resample::Mix& mix)
{
    if (count <= 0) return 0;
    if (count > avd_audio_map::kSlots) { ctx->err = "audio_track_slot: internal error (save table)"; return AVD_ERR_DEVICE; }
    SaveTable table = {};
    for (int i = 0; i < count; i++) {
        const AudioSaveRow& r = rows[i];
        if (r.hist_new_n < 0 || r.hist_new_n > avd_resample::kMaxHistory || r.hist_new_n > r.n + r.hist_old_n || r.held_words < 0 || r.held_words > kAudioSlotHeldWords) {
            ctx->err = "audio_track_slot: internal error (save extents)";
            return AVD_ERR_DEVICE;
        }
        table.row[i] = r;
    }
    if (mix.id && format == 1) hipLaunchKernelGGL(k_audio_slot_save_map_layout<int16_t>, dim3((unsigned)count), dim3(256), 0, ctx->stream, table, mix);
    else if (mix.id) hipLaunchKernelGGL(k_audio_slot_save_map_layout<float>, dim3((unsigned)count), dim3(256), 0, ctx->stream, table, mix);
    else if (format == 1) hipLaunchKernelGGL(k_audio_slot_save_map<int16_t>, dim3((unsigned)count), dim3(256), 0, ctx->stream, table, channels);
    else hipLaunchKernelGGL(k_audio_slot_save_map<float>, dim3((unsigned)count), dim3(256), 0, ctx->stream, table, channels);
    *enqueued = true;                                        // from here on the slots' memory may have been written
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

int launch_audio_slot_save(avd_ctx* ctx, const void* d_in, int format, long long n, int channels, const int16_t* hist_old, int hist_old_n, int16_t* hist_new,
                           int hist_new_n, const void* held_src, int16_t* held_dst, int held_words, bool* enqueued, const avd_resample::Mix& mix)
{
    if (hist_new_n < 0 || hist_new_n > avd_resample::kMaxHistory || hist_new_n > n + hist_old_n || held_words < 0 || held_words > kAudioSlotHeldWords) {
        ctx->err = "audio_slot: internal error (save extents)";
        return AVD_ERR_DEVICE;
    }
    if (mix.id && format == 1)
        hipLaunchKernelGGL(k_audio_slot_save_layout<int16_t>, dim3(1), dim3(256), 0, ctx->stream, static_cast<const int16_t*>(d_in), n, mix, hist_old, hist_old_n,
                           hist_new, hist_new_n, static_cast<const int16_t*>(held_src), held_dst, held_words);
    else if (mix.id)
        hipLaunchKernelGGL(k_audio_slot_save_layout<float>, dim3(1), dim3(256), 0, ctx->stream, static_cast<const float*>(d_in), n, mix, hist_old, hist_old_n,
                           hist_new, hist_new_n, static_cast<const int16_t*>(held_src), held_dst, held_words);
    else if (format == 1)
        hipLaunchKernelGGL(k_audio_slot_save<int16_t>, dim3(1), dim3(256), 0, ctx->stream, static_cast<const int16_t*>(d_in), n, channels, hist_old, hist_old_n,
                           hist_new, hist_new_n, static_cast<const int16_t*>(held_src), held_dst, held_words);
    else
        hipLaunchKernelGGL(k_audio_slot_save<float>, dim3(1), dim3(256), 0, ctx->stream, static_cast<const float*>(d_in), n, channels, hist_old, hist_old_n,
                           hist_new, hist_new_n, static_cast<const int16_t*>(held_src), held_dst, held_words);
    *enqueued = true;                                        // from here on the slot's memory may have been written
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// debug buffers "audio_rs_*" / "audio_pcm": what the converter of this call ran over
static void record_resample_plan(avd_ctx* ctx, const avd_resample::Plan& plan, int channels)
{
    const avd_resample::Ratio& r = plan.r;
    const int rs_plan[8] = {r.rate, channels, r.U, r.D, r.T, plan.tile_out, (int)std::min<long long>(plan.n_in, 0x7fffffff), (int)plan.n_out};
    std::memcpy(ctx->audio_rs_plan, rs_plan, sizeof rs_plan);
    ctx->audio_rs_ntracks = (int)plan.tracks.size();
    std::memcpy(ctx->audio_rs_tracks, plan.tracks.data(), sizeof(avd_resample::Track) * plan.tracks.size());
    ctx->audio_rs_pcm_at = plan.tracks.empty() ? 0 : plan.tracks[0].first;   // above 0 only behind a slot's held samples
    ctx->audio_rs_mapped = 0;
    ctx->audio_rs_valid = 1;
}

int launch_audio_resample(avd_ctx* ctx, const void* d_in, int format, int channels, const avd_resample::Plan& plan, int16_t* d_pcm, const AudioSource& src,
                          const avd_resample::Mix& mix)
{
    const avd_resample::Ratio& r = plan.r;
    const int ntiles = (int)plan.tiles.size(), bank = r.U * r.T, idx = avd_resample::rate_index(r.rate);
    if (idx < 0 || (ntiles <= 0 && plan.tracks.empty())) return 0;
    Workspace& ws = ctx->ws;
    ctx->audio_rs_valid = 0;
    if (ntiles <= 0) {                                       // a continued track's call that forms no output: recorded as such, nothing launched
        record_resample_plan(ctx, plan, channels);
        return 0;
    }
    if (ws.audio_rs_upload_pending) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); ws.audio_rs_upload_pending = 0; }
    std::vector<int>& taps = ctx->audio_rs_bank[idx];
    if (taps.empty() && bank) taps = avd_resample::build_taps(r);       // once per rate and context
    const bool new_rate = bank && ws.audio_rs_rate != r.rate;
    // pinned staging, in units of a tile (40 bytes): the tile table, then the bank when the rate changed
    const size_t bank_tiles = new_rate ? (sizeof(int) * (size_t)bank + sizeof(Tile) - 1) / sizeof(Tile) : 0;
    if (int e = ws.h_audio_rs.reserve(ctx, (size_t)ntiles + bank_tiles)) return e;
    if (int e = ws.d_audio_rs_tiles.reserve(ctx, (size_t)ntiles)) return e;
    std::memcpy(ws.h_audio_rs.p, plan.tiles.data(), sizeof(Tile) * (size_t)ntiles);
    if (new_rate) {
        std::memcpy(ws.h_audio_rs.p + ntiles, taps.data(), sizeof(int) * (size_t)bank);
        ws.audio_rs_rate = 0;                                // the bank is not valid again until its copy is enqueued
        if (int e = ws.d_audio_rs_taps.reserve(ctx, (size_t)bank)) return e;
    }
    ws.audio_rs_upload_pending = 1;
    HIP_TRY(ctx, hipMemcpyAsync(ws.d_audio_rs_tiles, ws.h_audio_rs.p, sizeof(Tile) * (size_t)ntiles, hipMemcpyHostToDevice, ctx->stream));
    if (new_rate) {
        HIP_TRY(ctx, hipMemcpyAsync(ws.d_audio_rs_taps, ws.h_audio_rs.p + ntiles, sizeof(int) * (size_t)bank, hipMemcpyHostToDevice, ctx->stream));
        ws.audio_rs_rate = r.rate;
    }
    const Tile* tiles = ws.d_audio_rs_tiles;
    const int* d_taps = ws.d_audio_rs_taps;                  // null at rate 16000 before any other rate ran: T = 0 reads none
    int e;
    if (avd_resample::wide(r))
        e = format == 1 ? launch_resample_as<int16_t, int, long long>(ctx, d_in, tiles, d_taps, ntiles, r, channels, d_pcm, src, mix)
                        : launch_resample_as<float, int, long long>(ctx, d_in, tiles, d_taps, ntiles, r, channels, d_pcm, src, mix);
    else
        e = format == 1 ? launch_resample_as<int16_t, int16_t, int>(ctx, d_in, tiles, d_taps, ntiles, r, channels, d_pcm, src, mix)
                        : launch_resample_as<float, int16_t, int>(ctx, d_in, tiles, d_taps, ntiles, r, channels, d_pcm, src, mix);
    if (e) return e;
    HIP_TRY(ctx, hipGetLastError());
    record_resample_plan(ctx, plan, channels);
    return 0;
}

// The converter of a call of several tracks (option "audio_track_slot"): ONE launch over the tiles of all of them.  The pinned staging holds, in one
// upload, the tile table | the source rows (8-byte aligned: a tile is 40 bytes) | each tile's track; the bank follows when the rate changed, as above.
// plan.sources carry the device address of each continued track's history already.  n_in: the frames of the call's buffer.
int launch_audio_resample_map(avd_ctx* ctx, const void* d_in, int format, int channels, const avd_audio_map::Plan& plan, const avd_resample::Ratio& r, long long n_in,
                              int16_t* d_pcm, bool* launched, const avd_resample::Mix& mix)
{
    const int ntiles = (int)plan.tiles.size(), ntracks = (int)plan.tracks.size(), bank = r.U * r.T, idx = avd_resample::rate_index(r.rate);
    *launched = false;
    if (idx < 0) return 0;
    Workspace& ws = ctx->ws;
    ctx->audio_rs_valid = 0;
    if (ntiles > 0) {
        if (ws.audio_rs_upload_pending) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); ws.audio_rs_upload_pending = 0; }
        std::vector<int>& taps = ctx->audio_rs_bank[idx];
        if (taps.empty() && bank) taps = avd_resample::build_taps(r);       // once per rate and context
        const bool new_rate = bank && ws.audio_rs_rate != r.rate;
        const size_t rows_at = sizeof(Tile) * (size_t)ntiles, track_at = rows_at + sizeof(Source) * (size_t)ntracks, up = track_at + sizeof(int) * (size_t)ntiles;
        const size_t up_tiles = (up + sizeof(Tile) - 1) / sizeof(Tile), bank_tiles = new_rate ? (sizeof(int) * (size_t)bank + sizeof(Tile) - 1) / sizeof(Tile) : 0;
        if (int e = ws.h_audio_rs.reserve(ctx, up_tiles + bank_tiles)) return e;
        if (int e = ws.d_audio_rs_tiles.reserve(ctx, up_tiles)) return e;
        char* hb = reinterpret_cast<char*>(ws.h_audio_rs.p);
        std::memcpy(hb, plan.tiles.data(), sizeof(Tile) * (size_t)ntiles);
        std::memcpy(hb + rows_at, plan.sources.data(), sizeof(Source) * (size_t)ntracks);
        std::memcpy(hb + track_at, plan.tile_track.data(), sizeof(int) * (size_t)ntiles);
        if (new_rate) {
            std::memcpy(ws.h_audio_rs.p + up_tiles, taps.data(), sizeof(int) * (size_t)bank);
            ws.audio_rs_rate = 0;                            // the bank is not valid again until its copy is enqueued
            if (int e = ws.d_audio_rs_taps.reserve(ctx, (size_t)bank)) return e;
        }
        ws.audio_rs_upload_pending = 1;
        HIP_TRY(ctx, hipMemcpyAsync(ws.d_audio_rs_tiles, hb, up, hipMemcpyHostToDevice, ctx->stream));
        if (new_rate) {
            HIP_TRY(ctx, hipMemcpyAsync(ws.d_audio_rs_taps, ws.h_audio_rs.p + up_tiles, sizeof(int) * (size_t)bank, hipMemcpyHostToDevice, ctx->stream));
            ws.audio_rs_rate = r.rate;
        }
        const char* db = reinterpret_cast<const char*>(ws.d_audio_rs_tiles.p);
        const Tile* tiles = ws.d_audio_rs_tiles;
        const Source* rows = reinterpret_cast<const Source*>(db + rows_at);
        const int* tile_track = reinterpret_cast<const int*>(db + track_at);
        const int* d_taps = ws.d_audio_rs_taps;
        int e;
        if (avd_resample::wide(r))
            e = format == 1 ? launch_resample_map_as<int16_t, int, long long>(ctx, d_in, tiles, tile_track, rows, d_taps, ntiles, r, channels, d_pcm, mix)
                            : launch_resample_map_as<float, int, long long>(ctx, d_in, tiles, tile_track, rows, d_taps, ntiles, r, channels, d_pcm, mix);
        else
            e = format == 1 ? launch_resample_map_as<int16_t, int16_t, int>(ctx, d_in, tiles, tile_track, rows, d_taps, ntiles, r, channels, d_pcm, mix)
                            : launch_resample_map_as<float, int16_t, int>(ctx, d_in, tiles, tile_track, rows, d_taps, ntiles, r, channels, d_pcm, mix);
        if (e) return e;
        HIP_TRY(ctx, hipGetLastError());
        *launched = true;
    }
    // debug buffers "audio_rs_*" / "audio_pcm": per track where its new outputs lie in the analyzer's buffer, and how many
    const int rs_plan[8] = {r.rate, channels, r.U, r.D, r.T, avd_resample::tile_outputs(r), (int)std::min<long long>(n_in, 0x7fffffff), (int)plan.fresh};
    std::memcpy(ctx->audio_rs_plan, rs_plan, sizeof rs_plan);
    ctx->audio_rs_ntracks = ntracks;
    for (int t = 0; t < ntracks; t++) {
        const avd_audio_map::Track& tr = plan.tracks[(size_t)t];
        ctx->audio_rs_tracks[t][0] = (int)(tr.region + tr.c.held_before);
        ctx->audio_rs_tracks[t][1] = (int)tr.c.fresh();
    }
    ctx->audio_rs_pcm_at = 0;
    ctx->audio_rs_mapped = 1;
    ctx->audio_rs_valid = 1;
    return 0;
}

// np.hanning(L), cos(2 pi j / L) and sin(2 pi j / L) at t, t + L and t + 2 L.  The one place where a table value is formed, for the full length
// and for every short one, on the host: a track's windows read the same bits whether it is analysed alone or in a batch, which is what makes the
// batch byte-identical to the per-track calls (device cos need not match libm's).
static void fill_length_tables(double* t, int L)
{
    // np.hanning(M) = 0.5 + 0.5 cos(pi n / (M-1)) for n = 1-M, 3-M, ..., M-1 (ones for M = 1)
    for (int i = 0; i < L; i++) t[i] = L == 1 ? 1.0 : 0.5 + 0.5 * std::cos(M_PI * (double)(2 * i + 1 - L) / (double)(L - 1));
    for (int j = 0; j < L; j++) { t[L + j] = std::cos(2.0 * M_PI * (double)j / (double)L); t[2 * L + j] = std::sin(2.0 * M_PI * (double)j / (double)L); }
}

// per-window features of the tracks of `plan` (avd_audio_plan.h), samples at d_wav (device; format 0: float32, 1: int16 PCM); d_out: device array of
// plan.nwin() records
int launch_audio_features(avd_ctx* ctx, const void* d_wav, int format, const avd_audio::Plan& plan, avd_audio_window* d_out)
{
    const int nwin = plan.nwin(), win = plan.win, nfull = plan.nfull(), ndft = (int)plan.dft.size();
    if (nwin <= 0) return 0;
    if (win < 1 || win > avd_audio::kMaxWin) { ctx->err = "audio window must be 1..8192 samples"; return AVD_ERR_ARG; }
    Workspace& ws = ctx->ws;
    ctx->audio_plan_valid = 0;                               // debug buffers "audio_*" describe this call once it is enqueued, never the one before
    // A call that failed between its upload and its drain may have left the copy out of the pinned staging buffer in flight
    if (ws.audio_upload_pending) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); ws.audio_upload_pending = 0; }
    // pinned staging: the per-call upload (arena | window table | the two lists), then the full-length tables when `win` changed.  Both leave in
    // asynchronous copies; the buffer is the workspace's, so nothing waits here for host memory that goes out of scope
    const bool new_win = ws.audio_win != win;
    const size_t up = plan.upload_bytes() / sizeof(double), full_at = up, stage = up + (new_win ? 3 * (size_t)win : 0);
    if (int e = ws.h_audio_call.reserve(ctx, stage)) return e;
    if (int e = ws.d_audio_call.reserve(ctx, up)) return e;
    double* h = ws.h_audio_call;
    char* hb = reinterpret_cast<char*>(h);
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < plan.lengths.size(); k++) fill_length_tables(h + plan.set_at[k], plan.lengths[k]);
    ctx->audio_host[0] = (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    ctx->audio_host[1] = (int)plan.lengths.size();
    std::memcpy(hb + plan.windows_at(), plan.windows.data(), sizeof(Window) * (size_t)nwin);
    if (nfull) std::memcpy(hb + plan.fft_at(), plan.fft.data(), sizeof(int) * (size_t)nfull);
    if (ndft) std::memcpy(hb + plan.dft_at(), plan.dft.data(), sizeof(int) * (size_t)ndft);
    if (new_win) {
        fill_length_tables(h + full_at, win);
        ws.audio_win = 0;                                    // the tables are not valid again until their copy is enqueued
        if (int e = ws.d_audio_tab.reserve(ctx, 3 * (size_t)win)) return e;
    }
    const size_t xw_need = plan.xw_size(), mag_need = plan.mag_size(), b_need = plan.b_size();
    if (int e = ws.d_audio_buf.reserve(ctx, xw_need + mag_need + b_need)) return e;
    ws.audio_upload_pending = 1;
    HIP_TRY(ctx, hipMemcpyAsync(ws.d_audio_call, h, plan.upload_bytes(), hipMemcpyHostToDevice, ctx->stream));
    if (new_win) {
        HIP_TRY(ctx, hipMemcpyAsync(ws.d_audio_tab, h + full_at, sizeof(double) * 3 * (size_t)win, hipMemcpyHostToDevice, ctx->stream));
        ws.audio_win = win;
    }
    const char* db = reinterpret_cast<const char*>(ws.d_audio_call.p);
    const double* arena = ws.d_audio_call;
    const Window* wt = reinterpret_cast<const Window*>(db + plan.windows_at());
    const int* fft_list = reinterpret_cast<const int*>(db + plan.fft_at());
    const int* dft_list = reinterpret_cast<const int*>(db + plan.dft_at());
    const double* t = ws.d_audio_tab;                        // hann | cos | sin of the full length
    double *xw = ws.d_audio_buf, *mag = ws.d_audio_buf + xw_need;
    double2* bbuf = reinterpret_cast<double2*>(ws.d_audio_buf + xw_need + mag_need);
    if (format == 1)
        hipLaunchKernelGGL(k_audio_prepare<int16_t>, dim3(nwin), dim3(256), 0, ctx->stream, static_cast<const int16_t*>(d_wav), wt, win, t, arena, xw, d_out);
    else
        hipLaunchKernelGGL(k_audio_prepare<float>, dim3(nwin), dim3(256), 0, ctx->stream, static_cast<const float*>(d_wav), wt, win, t, arena, xw, d_out);
    // per call (a function attribute belongs to the current device; a process may hold contexts on several)
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_audio_dft, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * 8192));
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_audio_fft_a, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * kFftN));
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_audio_fft_b, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * kFftN));
    // full windows of 8000 samples (the reference's half second at 16 kHz) take the two-step FFT path, everything else
    // (another window length, the short last window of a track) the direct form
    if (nfull > 0) {
        hipLaunchKernelGGL(k_audio_fft_a, dim3(nfull), dim3(256), (size_t)16 * kFftN, ctx->stream, (const double*)xw, fft_list, t + win, bbuf);
        hipLaunchKernelGGL(k_audio_fft_b, dim3(nfull), dim3(256), (size_t)8 * kFftN, ctx->stream, (const double2*)bbuf, fft_list, t + win, mag);
    }
    if (ndft > 0) {
        const int L = plan.max_dft_len;
        hipLaunchKernelGGL(k_audio_dft, dim3(ndft, (L / 2 + 1 + 255) / 256), dim3(256), (size_t)16 * L, ctx->stream, (const double*)xw, wt, dft_list, win, L,
                           t, arena, mag);
    }
    hipLaunchKernelGGL(k_audio_reduce, dim3(nwin), dim3(256), 0, ctx->stream, (const double*)mag, wt, win, d_out);
    HIP_TRY(ctx, hipGetLastError());
    ctx->audio_plan[0] = nwin; ctx->audio_plan[1] = win; ctx->audio_plan[2] = plan.tracks.back().last; ctx->audio_plan[3] = nfull;
    ctx->audio_ntracks = (int)plan.tracks.size();
    std::memcpy(ctx->audio_tracks, plan.tracks.data(), sizeof(avd_audio::Track) * plan.tracks.size());
    ctx->audio_plan_valid = 1;
    return 0;
}
