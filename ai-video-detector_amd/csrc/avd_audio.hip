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

}  // namespace

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
