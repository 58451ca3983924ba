// avd_capi.hip -- C-ABI of libavd_hip.so (include/avd.h): context, workspace, entry points.
// Host C++; the kernels live in the other .hip files (the Farneback schedule: avd_farneback.hip).
#include <algorithm>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <new>
#include <thread>
#include "avd_internal.h"

namespace {

constexpr int kFbChunk = 128;      // Farneback pairs the scratch holds at first (one 120-frame clip)
constexpr int kFbChunkMax = 512;   // ... and at most (2.6 GB): a batch of short clips runs as ONE launch sequence up to here;
                                   // longer calls are processed in chunks of the reserved size with a one-frame overlap

struct TableBlob {
    std::vector<uint8_t> bytes;
    template <typename T>
    size_t push(const std::vector<T>& v)
    {
        size_t off = (bytes.size() + 15) / 16 * 16;
        bytes.resize(off + v.size() * sizeof(T));
        std::memcpy(bytes.data() + off, v.data(), v.size() * sizeof(T));
        return off;
    }
};

}  // namespace

// ---- workspace -----------------------------------------------------------------------
// Build the tables of geometry (h, w) into cache entry g (its old table buffer is re-used when large enough).
static int build_geom(avd_ctx* ctx, Geom& g, int h, int w)
{
    LinearTab lt;
    AreaTab at;
    build_linear_tab(h, w, AVD_SMALL, AVD_SMALL, lt);
    int rc = build_area_tab(h, w, AVD_HASH, AVD_HASH, at);
    if (rc) { ctx->err = "unsupported geometry for INTER_AREA"; return rc; }
    const BandPlan plan = band_plan(w);
    const int R = plan.rows_per_band;
    const int nbands = (h + R - 1) / R;
    std::vector<int> band_dy;
    build_band_dy(lt, h, R, band_dy);
    TableBlob tb;
    std::vector<LinTap> lxt(AVD_SMALL), lyt(AVD_SMALL);
    for (int d = 0; d < AVD_SMALL; d++) {
        lxt[d] = LinTap{(short)lt.x0[d], (short)lt.x1[d], lt.a0[d], lt.a1[d]};
        lyt[d] = LinTap{(short)lt.y0[d], (short)lt.y1[d], lt.b0[d], lt.b1[d]};
    }
    const size_t o_lxt = tb.push(lxt), o_lyt = tb.push(lyt);
    const size_t o_band = tb.push(band_dy);
    const size_t o_axb = tb.push(at.x.begin), o_axc = tb.push(at.x.count);
    const size_t o_axf = tb.push(at.x.w_first), o_axm = tb.push(at.x.w_mid), o_axl = tb.push(at.x.w_last);
    const size_t o_ayb = tb.push(at.y.begin), o_ayc = tb.push(at.y.count);
    const size_t o_ayf = tb.push(at.y.w_first), o_aym = tb.push(at.y.w_mid), o_ayl = tb.push(at.y.w_last);
    g.h = g.w = 0;                                     // not valid until everything below succeeded
    // an evicted entry's tables may still be read by a kernel in flight on this context's stream: drain it before the buffer is
    // freed (larger tables) or re-used (only on the first use of a FIFTH distinct geometry)
    if (g.d_tables) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int e = g.d_tables.reserve(ctx, tb.bytes.size())) return e;
    uint8_t* dt = g.d_tables;
    HIP_TRY(ctx, hipMemcpyAsync(dt, tb.bytes.data(), tb.bytes.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // tb goes out of scope
    PreParams& P = g.pre;
    P = PreParams{};
    P.lxt = (const LinTap*)(dt + o_lxt); P.lyt = (const LinTap*)(dt + o_lyt);
    P.band_dy = (const int*)(dt + o_band);
    P.ax_begin = (const int*)(dt + o_axb); P.ax_count = (const int*)(dt + o_axc);
    P.ax_first = (const float*)(dt + o_axf); P.ax_mid = (const float*)(dt + o_axm); P.ax_last = (const float*)(dt + o_axl);
    P.area_fast = at.fast;
    P.area_x_uniform4 = 1;
    for (int d = 0; d < AVD_HASH; d++)
        if ((at.x.begin[d] & 3) || (at.x.count[d] & 3) || at.x.count[d] < 4 || at.x.w_first[d] != at.x.w_mid[d] ||
            at.x.w_last[d] != at.x.w_mid[d])
            P.area_x_uniform4 = 0;
    P.h = h; P.w = w; P.rows_per_band = R; P.nbands = nbands;
    P.pitch = plan.pitch;
    HashParams& H = g.hsh;
    H = HashParams{};
    H.ay_begin = (const int*)(dt + o_ayb); H.ay_count = (const int*)(dt + o_ayc);
    H.ay_first = (const float*)(dt + o_ayf); H.ay_mid = (const float*)(dt + o_aym); H.ay_last = (const float*)(dt + o_ayl);
    H.area_fast = at.fast;
    H.fast_area = at.iscale_x * at.iscale_y;
    H.fast_simd_w = (at.fast && at.iscale_x == 2 && at.iscale_y == 2) ? (AVD_HASH & ~7) : 0;
    H.h = h;
    g.h = h; g.w = w;
    return 0;
}

// The geometry (h, w) for one clip: slot.pre / slot.hsh become copies of its cache entry.  A hit costs nothing; a miss builds the
// tables in a free entry, or in the least recently used one.
static int avd_ws_geometry(avd_ctx* ctx, int h, int w, ClipSlot& slot)
{
    Workspace& ws = ctx->ws;
    Geom* hit = nullptr;
    Geom* victim = nullptr;                            // a free entry, else the least recently used one
    for (Geom& g : ws.geoms) {
        if (g.h == h && g.w == w) { hit = &g; break; }
        if (!victim || (g.h == 0 && victim->h != 0) || (g.h != 0 && victim->h != 0 && g.stamp < victim->stamp)) victim = &g;
    }
    if (!hit) {
        if (int e = build_geom(ctx, *victim, h, w)) return e;
        hit = victim;
    }
    hit->stamp = ++ws.geom_clock;
    slot.pre = hit->pre; slot.hsh = hit->hsh;
    return 0;
}

// Per-frame buffers for n frames (all clips of a call), `rowbuf_elems` floats of INTER_AREA row partials and `lappart_elems`
// long longs of Laplacian partial moments.  Grow-only: in steady state nothing is allocated or freed.
static int avd_ws_reserve_frames(avd_ctx* ctx, int n, size_t rowbuf_elems, size_t lappart_elems)
{
    Workspace& ws = ctx->ws;
    if (n > ws.cap_n) {
        const size_t cap = (size_t)std::max(n, 1);
        ws.cap_n = 0;                                  // not valid again until every buffer below exists
        if (int e = ws.d_small.reserve(ctx, cap * AVD_NPIX)) return e;
        if (int e = ws.d_area.reserve(ctx, cap * 1024)) return e;
        if (int e = ws.d_hash.reserve(ctx, cap * 1024)) return e;
        if (int e = ws.d_lap.reserve(ctx, cap * 2)) return e;
        if (int e = ws.d_rec.reserve(ctx, cap)) return e;
        if (int e = ws.d_clipstart.reserve(ctx, cap)) return e;
        if (int e = ws.h_rec.reserve(ctx, cap)) return e;
        if (int e = ws.h_clipstart.reserve(ctx, cap)) return e;
        ws.cap_n = (int)cap;
    }
    if (int e = ws.d_rowbuf.reserve(ctx, rowbuf_elems)) return e;
    return ws.d_lap_part.reserve(ctx, lappart_elems);
}

// what n frames of a geometry take of d_rowbuf / d_lap_part
static size_t rowbuf_elems_for(const PreParams& pre, int n) { return (size_t)n * pre.h * AVD_HASH; }
static size_t lappart_elems_for(const PreParams& pre, int n) { return (size_t)n * pre.nbands * kLapSlots * 2; }

// Farneback scratch for min(n - 1, kFbChunkMax) pairs, at least kFbChunk; grows when a call brings more pairs
static int avd_ws_reserve_fb(avd_ctx* ctx, int n)
{
    Workspace& ws = ctx->ws;
    const int want = std::max(kFbChunk, std::min(std::max(n - 1, 0), kFbChunkMax));
    if (want > ws.fb_cap) {
        const size_t nf = (size_t)want + 2, np = (size_t)want;       // frames = pairs + 1, and one spare
        ws.fb_cap = 0;                                 // not valid again until every buffer below exists
        ws.fb_holds = FbChunk{};
        for (int k = 0; k < AVD_FB_LEVELS; k++) {
            const size_t plane = (size_t)(AVD_SMALL >> k) * (AVD_SMALL >> k);
            // the 320-px scale of the pyramid exists only with fb_fold_blur off (the polynomial expansion forms that blur itself): 49 MB per 120 frames
            if (k > 0 || !fb_fold_blur_eff(ctx->fb_fold_blur, ctx->cv2_model)) { if (int e = ws.d_pyr[k].reserve(ctx, nf * plane)) return e; }
            else ws.d_pyr[0].reset();
            if (int e = ws.d_poly[k].reserve(ctx, nf * 5 * plane)) return e;
            if (int e = ws.d_flow[k].reserve(ctx, np * 2 * plane)) return e;
            if (int e = ws.d_flow2[k].reserve(ctx, np * 2 * plane)) return e;
        }
        if (int e = ws.d_stats.reserve(ctx, np * 2)) return e;
        if (int e = ws.d_mag.reserve(ctx, np * (size_t)AVD_NPIX)) return e;
        if (int e = ws.d_fbflags.reserve(ctx, np)) return e;
        if (int e = ws.d_pairdiff.reserve(ctx, np * kPairDiffTiles)) return e;
        if (int e = ws.h_rlist.reserve(ctx, np)) return e;
        // sized by the chunk, allocated by whoever first needs them
        ws.d_rlist.reset(); ws.d_vs.reset(); ws.d_vs0.reset(); ws.d_flow_il.reset();
        ws.fb_cap = want;
    }
    if (!fb_fold_blur_eff(ctx->fb_fold_blur, ctx->cv2_model))       // (a call is enqueued under the option's value of now: FlowCall::model)
        if (int e = ws.d_pyr[0].reserve(ctx, ((size_t)ws.fb_cap + 2) * AVD_NPIX)) return e;
    // the double intermediate of the two-kernel fallback (4 MB per pair): only when that path is selected
    if (ctx->fb_mode == 0 && ctx->fb_fused != 0xF) {
        const FbTwoScratchSize sz = fb_two_scratch_size((size_t)ws.fb_cap);
        if (int e = ws.d_vs0.reserve(ctx, sz.vs0)) return e;
        if (int e = ws.d_vs.reserve(ctx, sz.vs)) return e;
    }
    return 0;
}

// ---- record assembly -------------------------------------------------------------------
// One workgroup per frame, ONE launch per Farneback chunk (it follows the flow statistics): the frame's Laplacian moments,
// its Hamming distance to the previous frame (video.py:8: the 1024 aHash bits, one per byte, of both frames) and the
// statistics of pair (f - 1, f).  The first frame of a clip has no predecessor (ham = -1, flow 0; the pair the Farneback stage
// computed across a clip boundary is ignored): f == 0, or clipstart[f] != 0 when the call holds several clips
// (clipstart == nullptr: one clip).  with_flow == 0: a call without any pair (one frame).
__global__ __launch_bounds__(256) void k_records(const unsigned long long* __restrict__ lap, const uint8_t* __restrict__ bits,
                                                const float* __restrict__ stats, const int* __restrict__ flags, int stats_off,
                                                avd_frame_record* __restrict__ rec, int f0, const int* __restrict__ clipstart, int with_flow)
{
    __shared__ int wsum[4];
    const int f = f0 + blockIdx.x, tid = threadIdx.x;
    const bool first = f == 0 || (clipstart && clipstart[f] != 0);
    int c = 0;
    if (!first) {
        const unsigned a = reinterpret_cast<const unsigned*>(bits + (int64_t)f * 1024)[tid];
        const unsigned b = reinterpret_cast<const unsigned*>(bits + (int64_t)(f - 1) * 1024)[tid];
        c = __popc(a ^ b);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid != 0) return;
    avd_frame_record r;
    r.lap_sum = (int64_t)lap[2 * f];
    r.lap_sumsq = (int64_t)lap[2 * f + 1];
    r.ham = first ? -1 : wsum[0] + wsum[1] + wsum[2] + wsum[3];
    // fast Farneback mode: non-zero when pair (f - 1, f) met the ill-posedness criterion and was re-run by the exact kernels
    r.reserved = (first || !with_flow || !flags) ? 0 : flags[f - 1 - stats_off];
    r.flow_mean = (first || !with_flow) ? 0.f : stats[2 * (f - 1 - stats_off)];
    r.flow_var = (first || !with_flow) ? 0.f : stats[2 * (f - 1 - stats_off) + 1];
    rec[f] = r;
}

// Fast mode: the pairs of the chunk in the workspace whose flag word is set (h_flags[0 .. np), as the host has just read them) go through the
// exact kernels again (launch_farneback_rerun: enqueued, not drained).  Returns the number of such pairs, or a negative status.
static int rerun_flagged(avd_ctx* ctx, const FlowCall& call, const int* h_flags, int stride, int np)
{
    Workspace& ws = ctx->ws;
    int m = 0;
    for (int i = 0; i < np; i++)
        if (h_flags[(size_t)i * stride] != 0) ws.h_rlist[m++] = i;
    if (m == 0) return 0;
    if (int e = launch_farneback_rerun(ctx, call, ws.h_rlist, m, np)) return e < 0 ? e : -1;
    return m;
}

__global__ void k_wake() {}

// the records of frames fa .. p0 + np: the chunk of pairs p0 .. p0 + np - 1 is in the Farneback scratch.  np == 0: a call of one frame, which has no pair.
// again: the deferred re-run assembles its chunk's records a second time; that launch stays in the re-run's region (AVD_K_RERUN), it is not the
// call's record kernel
static void launch_records(avd_ctx* ctx, int p0, int np, int fa, const int* clipstart, bool again = false)
{
    Workspace& ws = ctx->ws;
    const int with_flow = np > 0;
    if (!again) kmark(ctx, AVD_K_RECORDS);
    hipLaunchKernelGGL(k_records, dim3(p0 + np + 1 - fa), dim3(256), 0, ctx->stream, (const unsigned long long*)ws.d_lap,
                       (const uint8_t*)ws.d_hash, (const float*)(with_flow ? ws.d_stats.p : nullptr),
                       (const int*)(with_flow && ctx->fb_mode == 1 && ctx->fb_rerun ? ws.d_fbflags.p : nullptr), p0, ws.d_rec, fa, clipstart, with_flow);
}

// Farneback + stats over all n-1 pairs in chunks; pair p = (frame p, frame p+1).
// Fast mode: the level kernels flag the pairs they cannot follow; the HOST reads the flag words and sends those pairs through the exact kernels
// (nothing is launched when nothing is flagged -- the usual case).  For the last chunk of an asynchronous call that happens when the call is
// drained (ctx->tail, impl_synchronize): the flags travel with the records.  A chunk that is followed by another one (> 512 pairs in a call), and
// every chunk of a call that hands statistics straight to the host, is settled here, before its scratch is reused.
static int run_flow_chunks(avd_ctx* ctx, const uint8_t* d_small, int n, float* h_mean, float* h_var,
                           float* h_flow_out, bool into_records, const int* records_clipstart = nullptr)
{
    Workspace& ws = ctx->ws;
    // every entry point completes a pending asynchronous call before it runs (guarded, drain_pending): a tail found here would be dropped
    if (ctx->tail.active) { ctx->err = "internal error: the re-run of a pending call was not settled"; return AVD_ERR_DEVICE; }
    if (n < 2) return 0;
    if (int e = avd_ws_reserve_fb(ctx, n)) return e;
    const int chunk = ws.fb_cap;
    if (h_flow_out)
        if (int e = ws.d_flow_il.reserve(ctx, (size_t)chunk * AVD_NPIX * 2)) return e;
    const bool flagged_mode = ctx->fb_mode == 1 && ctx->fb_rerun;
    const bool host_wants = h_mean || h_var || h_flow_out;
    // The plan of this call, handed to every launch of it.  Fast mode: the shape of the 160-px level, once for all chunks.  fb_wide160 = 2 chooses by what is
    // in flight: this call is being enqueued and not yet counted, so > 0 means SOMEBODY ELSE's kernels will share the chip with it.
    // The interleaved flow is formed only for a caller who fetches it.
    // fb_wide320 likewise chooses the shape of the 320-px level's launches that read a 320-px flow, and of its resizing first launch where fb_wide320_up allows it.
    const bool shared = avd_calls_in_flight() - ctx->counted_in_flight > 0;
    const FlowCall call{ctx->cv2_model, ctx->fb_wide160 == 1 || (ctx->fb_wide160 == 2 && shared), ctx->fb_wide320 == 1 || (ctx->fb_wide320 == 2 && shared), h_flow_out != nullptr};
    if (ctx->fb_mode == 1) { ctx->fb_wide160_used = call.wide160; ctx->fb_wide320_used = call.wide320; }      // the records behind the read-only options
    ctx->fb_wide320_launches = ctx->fb_wide320_up_launches = 0;
    ctx->fb_model[0] = call.model; ctx->fb_model[1] = fb_coarsest(call.model) + 1;
    ctx->fb_model[2] = fb_fold_up_eff(ctx->fb_fold_up, call.model); ctx->fb_model[3] = fb_fold_blur_eff(ctx->fb_fold_blur, call.model);
    ctx->fb_model_valid = 1;
    int rc = 0;
    for (int p0 = 0; p0 < n - 1 && rc == 0; p0 += chunk) {
        const int np = std::min(chunk, n - 1 - p0);
        const bool last = p0 + np >= n - 1;
        const uint8_t* base = d_small + (size_t)p0 * AVD_NPIX;
        FbChunk left;
        rc = launch_farneback(ctx, call, base, np + 1, &left);
        if (rc) break;
        rc = launch_flow_stats(ctx, call, left, np + 1);
        if (rc) break;
        if (flagged_mode && (!last || host_wants || !into_records)) {
            std::vector<int> fl((size_t)np, 0);
            hipError_t e = hipMemcpyAsync(fl.data(), ws.d_fbflags, sizeof(int) * np, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { ctx->err = hipGetErrorString(e); rc = AVD_ERR_DEVICE; break; }
            const int m = rerun_flagged(ctx, call, fl.data(), 1, np);
            if (m < 0) { rc = m; break; }
            if (!into_records) ctx->last_rerun += m;
        }
        // frames p0 + 1 .. p0 + np, and frame 0 with the first chunk
        const int fa = p0 == 0 ? 0 : p0 + 1;
        if (into_records) {
            launch_records(ctx, p0, np, fa, records_clipstart);
            if (flagged_mode && last && !host_wants) {
                // (the records path asked for no dense flow, so the deferred re-run forms none)
                ctx->tail.active = 1; ctx->tail.p0 = p0; ctx->tail.np = np; ctx->tail.fa = fa; ctx->tail.clipstart = records_clipstart; ctx->tail.call = call;
            }
        }
        if (host_wants) {
            std::vector<float> st((size_t)np * 2);
            hipError_t e = hipMemcpyAsync(st.data(), ws.d_stats, sizeof(float) * 2 * np, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && h_flow_out)
                e = hipMemcpyAsync(h_flow_out + (size_t)p0 * AVD_NPIX * 2, ws.d_flow_il,
                                   sizeof(float) * 2 * AVD_NPIX * np, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { ctx->err = hipGetErrorString(e); rc = AVD_ERR_DEVICE; break; }
            for (int i = 0; i < np; i++) {
                if (h_mean) h_mean[p0 + i] = st[2 * i];
                if (h_var) h_var[p0 + i] = st[2 * i + 1];
            }
        }
    }
    return rc;
}

// Make `src` (host or device) available on the device; host input is staged over PCIe.
static int stage_input(avd_ctx* ctx, const uint8_t* src, int mem, size_t bytes, const uint8_t** d_out)
{
    if (mem == AVD_MEM_DEVICE) { *d_out = src; return 0; }
    if (mem != AVD_MEM_HOST) { ctx->err = "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"; return AVD_ERR_ARG; }
    Workspace& ws = ctx->ws;
    if (int e = ws.d_stage.reserve(ctx, bytes)) return e;
    HIP_TRY(ctx, hipMemcpyAsync(ws.d_stage, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    *d_out = ws.d_stage;
    return 0;
}

// -> the event, for the kernel region that begins at the same place (kmark's `shared`); null with profiling off or when it was not recorded
static hipEvent_t stage_mark(avd_ctx* ctx, int i)
{
    if (!ctx->profiling) return nullptr;
    if (i == 0) ctx->stage_marks = 0;
    if (hipEventRecord(ctx->stage_ev[i], ctx->stream) != hipSuccess) return nullptr;
    ctx->stage_marks++;
    return ctx->stage_ev[i];
}

// contexts of this process (any device) that hold an enqueued, not yet drained avd_analyze_* call: what "fb_wide160" = 2 decides by
std::atomic<int> g_calls_in_flight{0};
int avd_calls_in_flight() { return g_calls_in_flight.load(std::memory_order_relaxed); }

// ---- contexts whose last Farneback chunk awaits its flags (fast mode; ctx->tail) ---------------------------------------------------------
// The exact re-run of a call's flagged pairs needs the HOST (it reads the flag words and sizes the launches).  With one host thread driving
// several contexts in turn, each clip's re-run would start only when the thread reaches that clip's avd_synchronize: the chip sits on one
// re-run chain at a time (a fully flagged 120-frame clip: 76 k frames/s against 108 k with one thread per context).  So a thread that has to wait
// anyway -- for its own fast pass or its own re-run -- looks at the other registered contexts of its device and settles those whose records have
// arrived.  Lock order: ctx->api_mu (blocking, taken by every entry point) -> g_tail_mu -> another context's api_mu (try_lock only).
static std::mutex g_tail_mu;
static std::vector<avd_ctx*> g_tail_list;
static std::atomic<int> g_tail_count{0};

static void tail_register(avd_ctx* ctx)
{
    if (ctx->tail_registered || hipEventRecord(ctx->tail_ev, ctx->stream) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(g_tail_mu);
    g_tail_list.push_back(ctx);
    ctx->tail_registered = 1;
    g_tail_count.fetch_add(1, std::memory_order_relaxed);
}

static void tail_unregister(avd_ctx* ctx)
{
    std::lock_guard<std::mutex> lk(g_tail_mu);             // a helper writes tail_registered under this lock
    if (!ctx->tail_registered) return;
    for (size_t i = 0; i < g_tail_list.size(); i++)
        if (g_tail_list[i] == ctx) { g_tail_list[i] = g_tail_list.back(); g_tail_list.pop_back(); break; }
    ctx->tail_registered = 0;
    g_tail_count.fetch_sub(1, std::memory_order_relaxed);
}

// The records of ctx's last chunk (with the level kernels' flag words) are in the pinned buffer: the pairs they mark go through the exact kernels
// (the workspace still holds the chunk), the chunk's records are assembled again and fetched.  Enqueues only; the caller holds ctx->api_mu.
static int tail_settle(avd_ctx* ctx)
{
    ctx->tail.active = 0;
    Workspace& ws = ctx->ws;
    const int p0 = ctx->tail.p0, np = ctx->tail.np, fa = ctx->tail.fa;
    const int m = rerun_flagged(ctx, ctx->tail.call, &ws.h_rec[p0 + 1].reserved, (int)(sizeof(avd_frame_record) / sizeof(int)), np);
    if (m < 0) return m;
    if (m > 0) {
        launch_records(ctx, p0, np, fa, ctx->tail.clipstart, true);
        HIP_TRY(ctx, hipMemcpyAsync(ws.h_rec + fa, ws.d_rec + fa, sizeof(avd_frame_record) * (size_t)(p0 + np + 1 - fa), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->profiling && ctx->kmark_used > 0) kmark(ctx, AVD_K_COUNT);     // close the re-run's region
    }
    return AVD_OK;
}

static void tail_help_others(avd_ctx* self)
{
    if (g_tail_count.load(std::memory_order_relaxed) == 0) return;
    std::unique_lock<std::mutex> lk(g_tail_mu, std::try_to_lock);
    if (!lk.owns_lock()) return;
    for (size_t i = 0; i < g_tail_list.size();) {
        avd_ctx* c = g_tail_list[i];
        if (c == self || c->device != self->device || !c->api_mu.try_lock()) { i++; continue; }
        bool settled = !c->tail.active;
        if (!settled && hipEventQuery(c->tail_ev) == hipSuccess) {
            int rc;
            try { rc = tail_settle(c); } catch (...) { c->err = "out of host memory"; rc = AVD_ERR_NOMEM; }
            c->tail.active = 0;
            c->tail_rc = rc;
            settled = true;
        }
        if (settled) {
            g_tail_list[i] = g_tail_list.back(); g_tail_list.pop_back();
            c->tail_registered = 0;
            g_tail_count.fetch_sub(1, std::memory_order_relaxed);
        } else {
            i++;
        }
        c->api_mu.unlock();
    }
}

// Wait for `ev` (or, with ev == nullptr, for everything on the context's stream).  While other contexts hold unsettled tails the wait is a poll
// that settles them as their fast passes finish; otherwise it blocks in the runtime.
static hipError_t wait_helping(avd_ctx* ctx, hipEvent_t ev)
{
    int spins = 0;
    while (ctx->tail_help && g_tail_count.load(std::memory_order_relaxed) - ctx->tail_registered > 0) {
        const hipError_t e = ev ? hipEventQuery(ev) : hipStreamQuery(ctx->stream);
        if (e != hipErrorNotReady) return e;
        tail_help_others(ctx);
        if (++spins > 64) std::this_thread::yield();
    }
    return ev ? hipEventSynchronize(ev) : hipStreamSynchronize(ctx->stream);
}

// ---- options (avd_set_option / avd_get_option, environment defaults read by avd_create) ----------------
// One row per option; what an option MEANS is documented at its field in avd_ctx (avd_internal.h).  A read-only row is a counter: avd_set_option does
// not know its name.  norm brings a value into range (false: refused with `refused`, the old value stays); env: read by avd_create through from_env and norm.
// act / read (the stream options): the option is not a plain field -- avd_set_option calls act with the accepted value, avd_get_option returns read's.
// check (the stream options): what the context's state refuses of a value that norm accepted -- the message, or null.
struct Option { const char* name; int avd_ctx::*field; bool writable; bool (*norm)(int& v); const char* env; int (*from_env)(const char* text); const char* refused;
                void (*act)(avd_ctx* ctx, int v); int (*read)(const avd_ctx* ctx); const char* (*check)(const avd_ctx* ctx, int v); };
static bool opt_any(int&) { return true; }
static bool opt_flag(int& v) { v = v != 0; return true; }
template <int AND, int OR = 0> static bool opt_mask(int& v) { v = (v & AND) | OR; return true; }
static bool opt_wide160(int& v) { v = v == 0 ? 0 : (v == 1 ? 1 : 2); return true; }
static bool opt_gemm_waves(int& v) { v = v == 16 ? 16 : 8; return true; }
static bool opt_cnn_fuse(int& v) { v = v < 0 ? 0 : (v > 2 ? 2 : v); return true; }
static bool opt_cnn_chunk(int& v) { return v >= 1 && v <= 1024; }
static bool opt_cnn_tap(int& v) { return v >= 0 && v <= kCnnTapPooled; }
static bool opt_stream(int& v) { return v >= 0 && v <= kStreamSlots; }
// "stream_reset": k empties slot k, 0 all of them (the memory stays: 103 KB a slot); it reads back as 0.  avd_set_option has drained the context.
static void stream_reset(avd_ctx* ctx, int v)
{
    for (int k = 1; k <= kStreamSlots; k++)
        if (v == 0 || v == k) ctx->streams[k - 1].frames = 0;
}
static int stream_reset_read(const avd_ctx*) { return 0; }
// "stream_frames": what the SELECTED slot has absorbed since it was last emptied
static int stream_frames(const avd_ctx* ctx) { return ctx->stream_slot ? ctx->streams[ctx->stream_slot - 1].frames : 0; }
// "stream_slot" and "stream_map" never hold at once: selecting a slot is refused while a position is mapped, mapping one while a slot is selected
static const char* stream_slot_check(const avd_ctx* ctx, int v)
{
    return v != 0 && ctx->stream_mapped > 0 ? "stream_slot: refused while \"stream_map\" maps a position (clear the map first: \"stream_map\" = -1)" : nullptr;
}
// "stream_map": (position << 4) | slot -- position 0 ... 63, slot 1 ... 8 maps it, slot 0 unmaps it; -1 clears the map.  Reads back as the number of
// mapped positions.  avd_set_option has drained the context.
static const char* stream_map_check(const avd_ctx* ctx, int v)
{
    if (v == -1) return nullptr;
    const int pos = v >> 4, slot = v & 15;
    if (v < 0 || pos >= kStreamMapPositions || slot > kStreamSlots) return "stream_map: (position << 4) | slot with position 0 ... 63 and slot 0 ... 8, or -1 (clear the map)";
    if (ctx->stream_slot != 0) return "stream_map: refused while \"stream_slot\" selects a slot (set it to 0 first)";
    for (int p = 0; slot != 0 && p < kStreamMapPositions; p++)
        if (p != pos && ctx->stream_map[p] == slot) return "stream_map: the slot is already mapped at another position";
    return nullptr;
}
static void stream_map_set(avd_ctx* ctx, int v)
{
    if (v == -1) for (int& s : ctx->stream_map) s = 0;
    else ctx->stream_map[v >> 4] = v & 15;
    ctx->stream_mapped = 0;
    for (int s : ctx->stream_map) ctx->stream_mapped += s != 0;
}
static int stream_map_read(const avd_ctx* ctx) { return ctx->stream_mapped; }
// "audio_format": 0 float32 samples, 1 little-endian int16 PCM; durable
static bool opt_audio_format(int& v) { return v == 0 || v == 1; }
// "audio_cut": a track of the NEXT avd_audio_features call ends, and the next one begins, at sample v of its buffer; one at a time, strictly ascending,
// at most 63; -1 clears the list.  Reads back as the number of cuts held.  The call takes the list (impl_audio_features).
static const char* audio_cut_check(const avd_ctx* ctx, int v)
{
    if (v == -1) return nullptr;
    if (v <= 0) return "audio_cut: a sample position above 0, or -1 (clear the list)";
    if (ctx->audio_ncuts > 0 && v <= ctx->audio_cuts[ctx->audio_ncuts - 1]) return "audio_cut: cuts are set in strictly ascending order";
    if (ctx->audio_ncuts >= avd_audio::kMaxCuts) return "audio_cut: at most 63 cuts (64 tracks) per call";
    return nullptr;
}
static void audio_cut_set(avd_ctx* ctx, int v)
{
    if (v == -1) ctx->audio_ncuts = 0;
    else ctx->audio_cuts[ctx->audio_ncuts++] = v;
}
static int audio_cut_read(const avd_ctx* ctx) { return ctx->audio_ncuts; }
// "audio_rate": 0 the samples are the 16 kHz track already; a rate of avd_audio_resample.h: frames at that rate, converted on the device; durable
static bool opt_audio_rate(int& v) { return v == 0 || avd_resample::rate_index(v) >= 0; }
// "audio_channels": interleaved samples per frame of a converted call, 1 or 2; durable
static bool opt_audio_channels(int& v) { return v == 1 || v == 2; }
// "audio_layout": 0 "audio_channels" decides, or id | flags -- id 1 (mono), 2 (stereo), 6 (5.1), 8 (7.1), flag 0x100 planar; durable
static bool opt_audio_layout(int& v) { return avd_resample::layout_ok(v); }
// "audio_plane_stride": samples from plane c to plane c + 1 of a planar call, 0 = the call's frame count; durable
static bool opt_audio_plane_stride(int& v) { return v >= 0; }
// "audio_slot": 0 every avd_audio_features call is a whole track, k = 1 ... 8 it continues the track of audio slot k; durable.  The audio slots are
// apart from the video stream slots: neither family of options touches the other's.
static bool opt_audio_slot(int& v) { return v >= 0 && v <= kAudioSlots; }
// "audio_slot" and "audio_track_slot" never hold at once, as "stream_slot" and "stream_map": selecting a slot is refused while the list holds an
// entry, setting an entry while a slot is selected
static const char* audio_slot_check(const avd_ctx* ctx, int v)
{
    return v != 0 && ctx->audio_map_n > 0 ? "audio_slot: refused while an \"audio_track_slot\" list is held (clear it first: \"audio_track_slot\" = -1)" : nullptr;
}
// "audio_track_slot": what the tracks of the NEXT avd_audio_features call are, one entry at a time in track order -- slot 0 (a whole track) or
// 1 ... 8 (the track continues that audio slot), | 0x10 the call carries the slot's last samples; -1 clears the list.  Reads back as the number of
// entries held.  The call takes the list (avd_audio_features).
static const char* audio_track_slot_check(const avd_ctx* ctx, int v)
{
    if (v == -1) return nullptr;
    if (ctx->audio_slot != 0) return "audio_track_slot: refused while \"audio_slot\" selects a slot (set it to 0 first)";
    if (v >= 0 && (v & ~(avd_audio_map::kSlotMask | avd_audio_map::kEndBit)) == 0 && (v & avd_audio_map::kEndBit) && (v & avd_audio_map::kSlotMask) == 0)
        return "audio_track_slot: 0x10 (the track ends) needs a slot 1 ... 8";
    if (!avd_audio_map::entry_ok(v)) return "audio_track_slot: slot 0 ... 8, | 0x10 (the call carries the slot's last samples), or -1 (clear the list)";
    for (int i = 0; i < ctx->audio_map_n; i++)
        if ((v & avd_audio_map::kSlotMask) && ((ctx->audio_map_entries[i] ^ v) & avd_audio_map::kSlotMask) == 0) return "audio_track_slot: the slot is already in the list";
    if (ctx->audio_map_n >= avd_audio_map::kMaxEntries) return "audio_track_slot: at most 64 entries (64 tracks) per call";
    return nullptr;
}
static void audio_track_slot_set(avd_ctx* ctx, int v)
{
    if (v == -1) ctx->audio_map_n = 0;
    else ctx->audio_map_entries[ctx->audio_map_n++] = v;
}
static int audio_track_slot_read(const avd_ctx* ctx) { return ctx->audio_map_n; }
// "audio_end": one-shot, the next avd_audio_features call carries the last samples of its slot's track; the call takes it (avd_audio_features)
static bool opt_audio_end(int& v) { return v == 1; }
static void audio_end_set(avd_ctx* ctx, int) { ctx->audio_end = 1; }
static int audio_end_read(const avd_ctx* ctx) { return ctx->audio_end; }
// "audio_slot_reset": k empties audio slot k, 0 all of them (the memory stays); it reads back as 0.  avd_set_option has drained the context.
static void audio_slot_reset(avd_ctx* ctx, int v)
{
    for (int k = 1; k <= kAudioSlots; k++)
        if (v == 0 || v == k) ctx->audio_slots[k - 1].clear();
}
static int audio_slot_reset_read(const avd_ctx*) { return 0; }
// read-only, of the SELECTED slot; an empty slot (frames = 0) reads 0 everywhere
static const AudioSlot* audio_slot_selected(const avd_ctx* ctx)
{
    return ctx->audio_slot && ctx->audio_slots[ctx->audio_slot - 1].frames > 0 ? &ctx->audio_slots[ctx->audio_slot - 1] : nullptr;
}
static int audio_slot_frames(const avd_ctx* ctx) { const AudioSlot* s = audio_slot_selected(ctx); return s ? (int)std::min<long long>(s->frames, 0x7fffffff) : 0; }
static int audio_slot_held(const avd_ctx* ctx) { const AudioSlot* s = audio_slot_selected(ctx); return s ? s->held : 0; }
static int audio_slot_windows(const avd_ctx* ctx) { const AudioSlot* s = audio_slot_selected(ctx); return s ? s->windows : 0; }
// "ingest_group": 0 a launch pair per clip, 1 one per group of clips that share a key (avd_ingest_group.h); durable
static bool opt_ingest_group(int& v) { return v == 0 || v == 1; }
// "cv2_model": any combination of the bits 1, 8 and 16 (the oracle's jitter switches 2 and 4 model nothing a library can follow); durable
static bool opt_cv2_model(int& v) { return v >= 0 && (v & ~kCv2ModelMask) == 0; }
static int env_any_base(const char* e) { return (int)std::strtol(e, nullptr, 0); }
static int env_fb_mode(const char* e) { return (std::strcmp(e, "exact") == 0 || std::strcmp(e, "0") == 0) ? 0 : 1; }
static const Option kOptions[] = {
    {"fb_fused", &avd_ctx::fb_fused, true, opt_mask<0xF>, "AVD_FB_FUSED", env_any_base},
    {"fb_mode", &avd_ctx::fb_mode, true, opt_flag, "AVD_FB_MODE", env_fb_mode},
    {"fb_fold_up", &avd_ctx::fb_fold_up, true, opt_mask<7>, "AVD_FB_FOLD_UP", std::atoi},
    {"fb_fold_up160", &avd_ctx::fb_fold_up160, true, opt_flag, "AVD_FB_FOLD_UP160", std::atoi},
    {"fb_rerun", &avd_ctx::fb_rerun, true, opt_flag, "AVD_FB_RERUN", std::atoi},
    {"fb_rerun_fused", &avd_ctx::fb_rerun_fused, true, opt_mask<0xF, 8>},          // bit 3 (40 px) is always set
    {"tail_help", &avd_ctx::tail_help, true, opt_flag},
    {"fb_wide160", &avd_ctx::fb_wide160, true, opt_wide160, "AVD_FB_WIDE160", std::atoi},
    {"fb_wide160_used", &avd_ctx::fb_wide160_used, false, opt_any},
    {"fb_wide320", &avd_ctx::fb_wide320, true, opt_wide160, "AVD_FB_WIDE320", std::atoi},         // the same three values
    {"fb_wide320_used", &avd_ctx::fb_wide320_used, false, opt_any},
    {"fb_wide320_up", &avd_ctx::fb_wide320_up, true, opt_flag, "AVD_FB_WIDE320_UP", std::atoi},
    {"fb_fold_blur", &avd_ctx::fb_fold_blur, true, opt_flag, "AVD_FB_FOLD_BLUR", std::atoi},
    {"gemm_waves", &avd_ctx::gemm_waves, true, opt_gemm_waves, "AVD_GEMM_WAVES", std::atoi},
    {"cnn_tiles", &avd_ctx::cnn_tiles, true, opt_any},
    {"cnn_fuse", &avd_ctx::cnn_fuse, true, opt_cnn_fuse},
    {"cnn_chunk", &avd_ctx::cnn_chunk, true, opt_cnn_chunk, nullptr, nullptr, "cnn_chunk: 1 ... 1024 frames per forward pass"},
    {"cnn_tap", &avd_ctx::cnn_tap, true, opt_cnn_tap, nullptr, nullptr, "cnn_tap: 0 (off), 1 input image, 2 ... 54 convolution 0 ... 52, 55 max pool, 56 pooled features"},
    {"rerun_pairs", &avd_ctx::last_rerun, false, opt_any},   // pairs of the last drained call that the fast level kernel flagged and the exact kernels re-ran
    {"stream_slot", &avd_ctx::stream_slot, true, opt_stream, nullptr, nullptr, "stream_slot: 0 (every call starts a new clip) or slot 1 ... 8", nullptr, nullptr, stream_slot_check},
    {"stream_map", nullptr, true, opt_any, nullptr, nullptr, nullptr, stream_map_set, stream_map_read, stream_map_check},
    {"stream_reset", nullptr, true, opt_stream, nullptr, nullptr, "stream_reset: 0 (every slot) or slot 1 ... 8", stream_reset, stream_reset_read},
    {"stream_frames", nullptr, false, opt_any, nullptr, nullptr, nullptr, nullptr, stream_frames},
    {"audio_format", &avd_ctx::audio_format, true, opt_audio_format, nullptr, nullptr, "audio_format: 0 (float32 samples) or 1 (little-endian int16 PCM)"},
    {"audio_cut", nullptr, true, opt_any, nullptr, nullptr, nullptr, audio_cut_set, audio_cut_read, audio_cut_check},
    {"audio_rate", &avd_ctx::audio_rate, true, opt_audio_rate, nullptr, nullptr, "audio_rate: 0 (samples at 16 kHz already) or 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000"},
    {"audio_channels", &avd_ctx::audio_channels, true, opt_audio_channels, nullptr, nullptr, "audio_channels: 1 or 2 interleaved samples per frame (planar samples and other layouts: option \"audio_layout\")"},
    {"audio_layout", &avd_ctx::audio_layout, true, opt_audio_layout, nullptr, nullptr, "audio_layout: 0 (\"audio_channels\" decides) or 1 (mono), 2 (stereo), 6 (5.1), 8 (7.1), | 0x100 (planar: one plane per channel)"},
    {"audio_plane_stride", &avd_ctx::audio_plane_stride, true, opt_audio_plane_stride, nullptr, nullptr, "audio_plane_stride: samples from one plane to the next, 0 (the call's frame count) or above"},
    {"audio_slot", &avd_ctx::audio_slot, true, opt_audio_slot, nullptr, nullptr, "audio_slot: 0 (every call is a whole track) or audio slot 1 ... 8", nullptr, nullptr, audio_slot_check},
    {"audio_track_slot", nullptr, true, opt_any, nullptr, nullptr, nullptr, audio_track_slot_set, audio_track_slot_read, audio_track_slot_check},
    {"audio_end", nullptr, true, opt_audio_end, nullptr, nullptr, "audio_end: 1 (the next avd_audio_features call carries the last samples of its slot's track)", audio_end_set, audio_end_read},
    {"audio_slot_reset", nullptr, true, opt_audio_slot, nullptr, nullptr, "audio_slot_reset: 0 (every audio slot) or audio slot 1 ... 8", audio_slot_reset, audio_slot_reset_read},
    {"audio_slot_frames", nullptr, false, opt_any, nullptr, nullptr, nullptr, nullptr, audio_slot_frames},
    {"audio_slot_held", nullptr, false, opt_any, nullptr, nullptr, nullptr, nullptr, audio_slot_held},
    {"audio_slot_windows", nullptr, false, opt_any, nullptr, nullptr, nullptr, nullptr, audio_slot_windows},
    {"ingest_group", &avd_ctx::ingest_group, true, opt_ingest_group, nullptr, nullptr, "ingest_group: 0 (an ingest and a hash launch per clip) or 1 (one of each per group of clips that share a key)"},
    {"cv2_model", &avd_ctx::cv2_model, true, opt_cv2_model, "AVD_CV2_MODEL", env_any_base, "cv2_model: a combination of 1 (GAUSS_MULADD), 8 (THREE_SCALES) and 16 (RESIZE_LERP), or 0 (the default model)"},
};
static const Option* find_option(avd_ctx* ctx, const char* name, bool to_write)
{
    for (const Option& o : kOptions)
        if (std::strcmp(name, o.name) == 0 && (o.writable || !to_write)) return &o;
    ctx->err = std::string("unknown option: ") + name;
    return nullptr;
}

// ---- entry-point bodies (wrapped by the extern "C" functions at the end of the file) -----------------
static void impl_destroy(avd_ctx* ctx);
static int impl_synchronize(avd_ctx* ctx);

static int impl_create(int device_id, avd_ctx** out)
{
    if (!out) return AVD_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_id < 0 || device_id >= count)
        return AVD_ERR_DEVICE;
    avd_ctx* ctx = new (std::nothrow) avd_ctx();
    if (!ctx) return AVD_ERR_NOMEM;
    ctx->device = device_id;
    bool ok = hipSetDevice(device_id) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&ctx->ev0) == hipSuccess && hipEventCreate(&ctx->ev1) == hipSuccess &&
              hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&ctx->tail_ev, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < 5; i++) ok = hipEventCreate(&ctx->stage_ev[i]) == hipSuccess;
    for (int i = 0; ok && i < 12; i++) ok = hipEventCreate(&ctx->kern_ev[i]) == hipSuccess;
    if (ok) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0)
            ctx->num_cus = prop.multiProcessorCount;
        for (const Option& o : kOptions)
            if (const char* e = o.env && o.writable ? std::getenv(o.env) : nullptr) { int v = o.from_env(e); if (o.norm(v)) ctx->*o.field = v; }
        build_fb_consts(ctx->fbc);
        ok = ctx->d_fbc.reserve(ctx, 1) == 0 &&
             hipMemcpy(ctx->d_fbc, &ctx->fbc, sizeof(FbConsts), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) { impl_destroy(ctx); return AVD_ERR_DEVICE; }
    *out = ctx;
    return AVD_OK;
}

static void impl_destroy(avd_ctx* ctx)
{
    if (!ctx) return;
    tail_unregister(ctx);                                   // no helper finds the context from here on ...
    { std::lock_guard<std::recursive_mutex> lk(ctx->api_mu); }   // ... and one that had found it has let go
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->counted_in_flight) { ctx->counted_in_flight = 0; g_calls_in_flight.fetch_sub(1, std::memory_order_relaxed); }
    comm_destroy(ctx);
    // everything the context owns on the device goes here: after the drain, before its stream does
    ctx->ws = Workspace{};
    ctx->weights = Weights{};
    for (StreamSlot& s : ctx->streams) s.d_prev.reset();
    for (AudioSlot& s : ctx->audio_slots) s.d_mem.reset();
    ctx->d_fbc.reset();
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev_in) (void)hipEventDestroy(ctx->ev_in);
    if (ctx->tail_ev) (void)hipEventDestroy(ctx->tail_ev);
    for (auto& e : ctx->stage_ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->kern_ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->kmark_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// ---- ingest: one clip = an IngestClip (avd_ingest_clip.h: its format, its argument check, its staging plan) ------------------
static int refuse(avd_ctx* ctx, const Refusal& r)
{
    if (r.status) ctx->err = r.why;
    return r.status;
}

// The frame lists of one call (IngestClip::is_list): the staging plan of each and its place in the table of plane pointers.  The table -- per
// list [plane][frame] device addresses: the caller's planes, or where list_stage puts them in the staging buffer, so that host and device
// lists run the same path -- is filled in the pinned mirror and uploaded once, ahead of the first clip.
struct CallLists {
    std::vector<ListStage> stage;      // per clip; empty for a strided clip
    std::vector<size_t> at;            // per clip: its first entry in the table
    std::vector<size_t> group_at;      // per group of the call's plan (option "ingest_group"): a grouped launch's first entry -- [plane][frames], then its output frames
    size_t entries = 0;
    size_t total(const IngestClip& k, int c) const { return k.is_list ? stage[c].total : clip_stage(k).total; }      // bytes of ws.d_stage clip c occupies
};

static void plan_lists(const IngestClip* clips, int nclips, CallLists& L)
{
    L.stage.resize((size_t)nclips);
    L.at.assign((size_t)nclips, 0);
    for (int c = 0; c < nclips; c++) {
        const IngestClip& k = clips[c];
        if (!k.is_list || k.n <= 0) continue;
        L.stage[c] = list_stage(k);
        L.at[c] = L.entries;
        L.entries += (size_t)k.planes() * k.n;
    }
}

// the table and its pinned mirror, grow-only; with every other reservation of the call, before its first launch
static int reserve_lists(avd_ctx* ctx, const CallLists& L)
{
    if (int e = ctx->ws.d_ftab.reserve(ctx, L.entries)) return e;
    return ctx->ws.h_ftab.reserve(ctx, L.entries);
}

// Where the planes of clip c of a call are on the DEVICE, whatever kind of clip it is: the caller's planes, or their places in the staging buffer
// (the clip occupies ws.d_stage from byte stage_at on, which must be reserved).  What the per-clip path hands its launch, asked per frame: a
// grouped launch's table and a clip's group key (its 16-byte eligibility) are formed from it.
struct DevicePlanes {
    const IngestClip& k;
    const uint8_t* staged;             // the clip's place in ws.d_stage
    const ListStage* list;             // a list's staging plan
    const uint8_t* base[3];            // a strided clip: frame 0's planes
    DevicePlanes(const Workspace& ws, const IngestClip& clip, size_t stage_at, const ListStage* ls)
        : k(clip), staged(ws.d_stage + stage_at), list(ls), base{clip.data, clip.uv, clip.v}
    {
        if (k.is_list || k.mem != AVD_MEM_HOST || k.n <= 0) return;
        const ClipStage s = clip_stage(k);
        for (int p = 0; p < k.planes(); p++) base[p] = staged + s.plane_off[p];
    }
    const uint8_t* at(int p, int f) const
    {
        if (k.is_list) return k.mem == AVD_MEM_HOST ? staged + list->plane_off[(size_t)p * k.n + f] : k.list[p][f];
        return base[p] + (int64_t)f * (p == 0 ? k.frame_stride : k.uv_frame_stride);
    }
    // the clip's own answer, by the rule it runs under alone (avd_ingest_clip.h)
    bool vec_eligible() const
    {
        if (k.is_list) return ::vec_eligible(k, k.n, [&](int p, int f) { return (uintptr_t)at(p, f); });
        return strided_vec_eligible(k, base[0], base[1], base[2]);
    }
};

// ws.d_stage and the table are reserved: the table can be filled.  One upload for all lists of the call, the tables of its grouped launches
// (groups, may be null; stage_at: per clip, its first byte of ws.d_stage) included.
static int upload_lists(avd_ctx* ctx, const IngestClip* clips, int nclips, const CallLists& L, const avd_group::Plan* groups = nullptr,
                        const size_t* stage_at = nullptr)
{
    if (!L.entries) return 0;
    Workspace& ws = ctx->ws;
    for (size_t gi = 0; groups && gi < groups->groups.size(); gi++) {
        const avd_group::Group& G = groups->groups[gi];
        if (!G.grouped) continue;
        const uint8_t** tab = ws.h_ftab + L.group_at[gi];
        const int planes = clips[G.members.front().clip].planes();
        int* out = reinterpret_cast<int*>(tab + (size_t)planes * G.frames);
        for (const avd_group::Member& m : G.members) {
            const DevicePlanes dp(ws, clips[m.clip], stage_at[m.clip], &L.stage[(size_t)m.clip]);
            for (int f = 0; f < m.n; f++) {
                for (int p = 0; p < planes; p++) tab[(size_t)p * G.frames + m.g0 + f] = dp.at(p, f);
                out[m.g0 + f] = m.out0 + f;
            }
        }
        if (G.frames & 1) out[G.frames] = 0;           // the other half of the last entry
    }
    size_t st = 0;
    for (int c = 0; c < nclips; c++) {
        const IngestClip& k = clips[c];
        if (k.is_list && k.n > 0) {
            const uint8_t** tab = ws.h_ftab + L.at[c];
            for (int p = 0; p < k.planes(); p++)
                for (int f = 0; f < k.n; f++) {
                    const size_t i = (size_t)p * k.n + f;
                    tab[i] = k.mem == AVD_MEM_HOST ? ws.d_stage + st + L.stage[c].plane_off[i] : k.list[p][f];
                }
        }
        if (k.n > 0) st += L.total(k, c);
    }
    HIP_TRY(ctx, hipMemcpyAsync(ws.d_ftab, ws.h_ftab, sizeof(const uint8_t*) * L.entries, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

// Stage clip c of the call at offset `at` of ws.d_stage (host input; reserved by the caller) and launch its fused full-resolution kernel, which
// writes the clip's slice of the per-frame buffers with the clip's geometry (slot).
// the copies alone (nothing for device input): a grouped launch has those of all its clips enqueued ahead of it
static int stage_clip(avd_ctx* ctx, const IngestClip& k, size_t at, const CallLists& L, int c)
{
    uint8_t* dst = ctx->ws.d_stage + at;
    if (k.mem != AVD_MEM_HOST) return 0;
    if (k.is_list) {
        const ListStage& s = L.stage[c];
        for (const StageSpan& sp : s.span)
            HIP_TRY(ctx, hipMemcpyAsync(dst + sp.off, sp.src, sp.bytes, hipMemcpyHostToDevice, ctx->stream));
        ctx->ingest.stage_bytes += (int64_t)s.copied;
        ctx->ingest.stage_copies += (int64_t)s.span.size();
        return 0;
    }
    const ClipStage s = clip_stage(k);
    for (int i = 0; i < s.nspans; i++)
        HIP_TRY(ctx, hipMemcpyAsync(dst + s.span[i].off, s.span[i].src, s.span[i].bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->ingest.stage_bytes += (int64_t)s.copied;
    ctx->ingest.stage_copies += s.nspans;
    return 0;
}

static int preprocess_clip(avd_ctx* ctx, const ClipSlot& slot, const IngestClip& k, size_t at, const CallLists& L, int c)
{
    uint8_t* dst = ctx->ws.d_stage + at;
    if (int e = stage_clip(ctx, k, at, L, c)) return e;
    if (k.is_list) {
        const uint8_t* const* h_tab = ctx->ws.h_ftab + L.at[c];
        const uint8_t* const* d_tab = ctx->ws.d_ftab + L.at[c];
        const FrameTable ft{list_vec_eligible(k, h_tab)};
        auto plane = [&](int p) { return p < k.planes() ? reinterpret_cast<const uint8_t*>(d_tab + (size_t)p * k.n) : nullptr; };
        return launch_preprocess(ctx, slot, k, plane(0), plane(1), plane(2), &ft);
    }
    const uint8_t *d_in = k.data, *d_uv = k.uv, *d_v = k.v;
    if (k.mem == AVD_MEM_HOST) {
        const ClipStage s = clip_stage(k);
        d_in = dst + s.plane_off[0];
        if (k.planes() >= 2) d_uv = dst + s.plane_off[1];
        if (k.planes() == 3) d_v = dst + s.plane_off[2];
    }
    return launch_preprocess(ctx, slot, k, d_in, d_uv, d_v);
}

// Every avd_preprocess_* entry: one clip at offset 0 of the buffers, results to the host
static int impl_preprocess(avd_ctx* ctx, const IngestClip& k, uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq)
{
    if (!ctx) return AVD_ERR_ARG;
    if (int e = refuse(ctx, check_clip(k))) return e;
    const int n = k.n;
    if (n == 0) return AVD_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ClipSlot slot;                                         // the one clip starts every buffer
    if (int e = avd_ws_geometry(ctx, k.disp_h(), k.disp_w(), slot)) return e;
    if (int e = avd_ws_reserve_frames(ctx, n, rowbuf_elems_for(slot.pre, n), lappart_elems_for(slot.pre, n))) return e;
    Workspace& ws = ctx->ws;
    CallLists lists;
    plan_lists(&k, 1, lists);
    if (int e = ws.d_stage.reserve(ctx, lists.total(k, 0))) return e;
    if (int e = reserve_lists(ctx, lists)) return e;
    ctx->ingest.stage_bytes = 0;
    ctx->ingest.stage_copies = 0;
    if (int e = upload_lists(ctx, &k, 1, lists)) return e;
    if (int e = preprocess_clip(ctx, slot, k, 0, lists, 0)) return e;
    if (int e = launch_hash(ctx, slot, n)) return e;
    std::vector<unsigned long long> lap((size_t)n * 2);
    if (small320) HIP_TRY(ctx, hipMemcpyAsync(small320, ws.d_small, (size_t)n * AVD_NPIX, hipMemcpyDeviceToHost, ctx->stream));
    if (hash1024) HIP_TRY(ctx, hipMemcpyAsync(hash1024, ws.d_hash, (size_t)n * 1024, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(lap.data(), ws.d_lap, sizeof(unsigned long long) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < n; f++) {
        if (lap_sum) lap_sum[f] = (int64_t)lap[2 * f];
        if (lap_sumsq) lap_sumsq[f] = (int64_t)lap[2 * f + 1];
    }
    ctx->last_n = n;
    ctx->rec_n = 0; ctx->rec_mapped = 0;
    return AVD_OK;
}

// avd_preprocess_picture: the descriptor becomes a clip (from_picture), then the one body
static int impl_preprocess_one_picture(avd_ctx* ctx, const avd_picture* pic, uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq)
{
    if (!ctx) return AVD_ERR_ARG;
    if (!pic) { ctx->err = "null picture"; return AVD_ERR_ARG; }
    IngestClip k{};
    if (int e = refuse(ctx, from_picture(*pic, k))) return e;
    return impl_preprocess(ctx, k, small320, hash1024, lap_sum, lap_sumsq);
}

// avd_preprocess_frame_list: the same with from_frame_list
static int impl_preprocess_one_list(avd_ctx* ctx, const avd_frame_list* list, uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq)
{
    if (!ctx) return AVD_ERR_ARG;
    if (!list) { ctx->err = "null frame list"; return AVD_ERR_ARG; }
    IngestClip k{};
    if (int e = refuse(ctx, from_frame_list(*list, k))) return e;
    return impl_preprocess(ctx, k, small320, hash1024, lap_sum, lap_sumsq);
}

static int impl_farneback_pairs(avd_ctx* ctx, const uint8_t* small320, int mem, int n,
                        float* flow_mean, float* flow_var, float* flow_out)
{
    if (!ctx) return AVD_ERR_ARG;
    if (n < 0 || (!small320 && n > 0)) { ctx->err = "bad arguments"; return AVD_ERR_ARG; }
    if (n < 2) return AVD_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint8_t* d_small = nullptr;
    if (int e = stage_input(ctx, small320, mem, (size_t)n * AVD_NPIX, &d_small)) return e;
    ctx->last_rerun = 0;
    kmark_reset(ctx);
    std::vector<float> fm_tmp;
    if (!flow_mean && !flow_var && !flow_out) { fm_tmp.resize((size_t)n - 1); flow_mean = fm_tmp.data(); }   // the chunks are drained either way
    if (int e = run_flow_chunks(ctx, d_small, n, flow_mean, flow_var, flow_out, false)) return e;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // with profiling on the launchers have recorded marks, but avd_kernel_ms reports avd_analyze_* calls only: these feed no figure (an error
    // return above leaves them behind unclosed, which impl_synchronize does not read either)
    kmark_reset(ctx);
    ctx->last_n = std::min(n, ctx->ws.fb_cap + 1);
    ctx->rec_n = 0; ctx->rec_mapped = 0;
    return AVD_OK;
}

// A stream slot's frame <-> one frame of the per-frame buffers: what the Farneback stage and k_records read of a frame (its rows of small,
// hash and lap), 103 KB in kStreamWords 16-byte words, which the slot keeps back to back.  ONE launch per direction: three copies through the
// runtime cost a 1080p call more than ingesting the frame again did.
constexpr int kStreamSmallWords = AVD_NPIX / 16, kStreamHashWords = 1024 / 16, kStreamWords = kStreamSmallWords + kStreamHashWords + 1;
static_assert(kStreamHashAt == (size_t)kStreamSmallWords * 16 && kStreamLapAt == (size_t)(kStreamSmallWords + kStreamHashWords) * 16 &&
              kStreamPrevBytes == (size_t)kStreamWords * 16, "the slot's layout in 16-byte words");
// One launch serves every slot of a call (option "stream_map": up to eight clips continue a slot each): the grid is (words of a slot frame,
// entries of the table), and the table -- which slot buffer goes with which frame of the buffers -- is a kernel argument by value.
struct StreamCopyEntry { uint4* kept; int frame; };
struct StreamCopyTable { StreamCopyEntry e[kStreamSlots]; };
__global__ __launch_bounds__(256) void k_stream_copy(uint4* __restrict__ small, uint4* __restrict__ hash, uint4* __restrict__ lap,
                                                    const StreamCopyTable table, int save)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kStreamWords) return;
    const StreamCopyEntry e = table.e[blockIdx.y];
    const size_t f = (size_t)e.frame;
    uint4* const frame = i < kStreamSmallWords ? small + f * kStreamSmallWords + i
                       : (i < kStreamSmallWords + kStreamHashWords ? hash + f * kStreamHashWords + (i - kStreamSmallWords) : lap + f);
    if (save) e.kept[i] = *frame;
    else *frame = e.kept[i];
}

// save: each entry's frame of the buffers -> its slot; else slot -> frame.  (A frame's rows are 16-byte aligned: 102 400, 1 024 and 16 bytes a frame.)
// The frames lie inside the buffers the call reserved (avd_ws_reserve_frames), the slots' buffers are reserved in pass 1.
static hipError_t stream_copy(avd_ctx* ctx, const StreamCopyTable& table, int entries, bool save)
{
    Workspace& ws = ctx->ws;
    hipLaunchKernelGGL(k_stream_copy, dim3((kStreamWords + 255) / 256, entries), dim3(256), 0, ctx->stream, reinterpret_cast<uint4*>(ws.d_small.p),
                       reinterpret_cast<uint4*>(ws.d_hash.p), reinterpret_cast<uint4*>(ws.d_lap.p), table, save ? 1 : 0);
    return hipGetLastError();
}

// ---- the whole per-frame path for a BATCH of clips (every avd_analyze_* entry; a single clip is a batch of one) --------
// Frames of all clips are concatenated in the per-frame buffers (small320, hashes, moments, records): clip c occupies frames
// [f0_c, f0_c + n_c).  Preprocess / hash / Hamming run per clip with that clip's geometry (cached tables); the Farneback
// stage does not care where a 320 x 320 frame came from: it runs ONCE over all N - 1 consecutive pairs of the concatenation
// (the one pair per clip boundary it computes in vain is ignored by k_records), so K short clips cost one launch sequence
// over all their pairs instead of K sequences that each leave most of the chip idle.
static int impl_analyze_async(avd_ctx* ctx, const IngestClip* clips, int nclips, avd_frame_record* records)
{
    if (!ctx) return AVD_ERR_ARG;
    if (nclips < 0 || (nclips > 0 && !clips)) { ctx->err = "bad clip list"; return AVD_ERR_ARG; }
    int64_t total = 0;
    int live = 0;                                          // clips that bring frames
    for (int c = 0; c < nclips; c++) {
        if (int e = refuse(ctx, check_clip(clips[c]))) return e;
        total += clips[c].n;
        live += clips[c].n > 0;
    }
    // Option "stream_slot": the call continues the clip whose last frame the slot holds.  That frame (its carry) goes in front of the call's own
    // frames in the per-frame buffers, the one clip starts at frame 1, and everything behind the ingest -- Farneback chunks, flags, the exact
    // re-run, the record kernel -- runs over n + 1 frames as it would for a call that had been handed the frame again; records 1 .. n go out.
    // Option "stream_map": the same for several clips of one call -- the clip at position p continues slot stream_map[p], each behind its own
    // restored frame.  Where every clip lies, which frames have no predecessor and which records go out is the plan (avd_stream_plan.h);
    // with "stream_slot" it is the one clip at frame 1 behind the slot's frame, without a slot the batch layout.
    if (ctx->stream_slot && live > 1) { ctx->err = "stream_slot: one clip per call"; return AVD_ERR_ARG; }
    const bool mapped = ctx->stream_mapped > 0;
    std::vector<StreamSlot*> stream((size_t)nclips, nullptr);     // per clip: the slot it continues (a clip that brings frames only: an empty one leaves its slot alone)
    std::vector<avd_stream::ClipIn> plan_in((size_t)nclips);
    for (int c = 0; c < nclips; c++) {
        const int k = mapped ? (c < kStreamMapPositions ? ctx->stream_map[c] : 0) : ctx->stream_slot;
        if (k && clips[c].n > 0) stream[c] = &ctx->streams[k - 1];
        plan_in[c] = {clips[c].n, !stream[c] ? avd_stream::kUnmapped : (stream[c]->frames > 0 ? avd_stream::kMappedFilled : avd_stream::kMappedEmpty)};
    }
    if (total > (1 << 24)) { ctx->err = "too many frames in one call"; return AVD_ERR_ARG; }
    if (total == 0) {
        for (int& v : ctx->stream_call) v = 0;
        for (int& v : ctx->ingest_call) v = 0;
        ctx->ingest_groups.clear();
        return AVD_OK;
    }
    const avd_stream::Plan plan = avd_stream::plan_call(plan_in.data(), nclips);
    if (plan.total > (1 << 24)) { ctx->err = "too many frames in one call"; return AVD_ERR_ARG; }
    if (!records) { ctx->err = "null pointer"; return AVD_ERR_ARG; }
    const int own = plan.own;                              // the caller's frames = the records that go out
    const int n = plan.total;                              // frames in the buffers
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Workspace& ws = ctx->ws;
    // pass 1: geometry tables (cached), each clip's place in the buffers and their sizes -- everything is reserved before the first launch of the call
    size_t rowbuf_elems = 0, lappart_elems = 0, stage_bytes = 0;
    CallLists lists;
    plan_lists(clips, nclips, lists);
    std::vector<ClipSlot> slots((size_t)nclips);
    std::vector<size_t> stage_at((size_t)nclips, 0);       // the clip's first byte of ws.d_stage
    for (int c = 0; c < nclips; c++) {
        const IngestClip& k = clips[c];
        if (k.n == 0) continue;
        ClipSlot& slot = slots[c];
        if (int e = avd_ws_geometry(ctx, k.disp_h(), k.disp_w(), slot)) return e;
        slot.f0 = plan.f0[c];
        stage_at[c] = stage_bytes;
        stage_bytes += lists.total(k, c);
    }
    if (int e = ws.d_stage.reserve(ctx, stage_bytes)) return e;
    // Which clips share their two launches (avd_ingest_group.h).  With option "ingest_group" off nobody does -- a bound of 0 bands puts every clip in
    // a group of its own, in call order, and the row and Laplacian partials are handed out clip by clip as they always were.  A clip's key needs
    // its planes' device addresses (its 16-byte eligibility), hence the staging buffer first.
    const bool grouping = ctx->ingest_group != 0;
    std::vector<avd_group::Key> keys((size_t)nclips);
    std::vector<int> clip_n((size_t)nclips);
    for (int c = 0; c < nclips; c++) {
        const IngestClip& k = clips[c];
        clip_n[c] = k.n;
        if (k.n == 0) continue;
        keys[c] = avd_group::key_of(k, slots[c].pre.nbands, grouping && DevicePlanes(ws, k, stage_at[c], &lists.stage[c]).vec_eligible());
    }
    const avd_group::Plan groups = avd_group::plan_groups(keys.data(), clip_n.data(), plan.f0.data(), nclips, grouping ? avd_group::kMaxLaunchBands : 0);
    lists.group_at.assign(groups.groups.size(), 0);
    for (size_t gi = 0; gi < groups.groups.size(); gi++) {
        const avd_group::Group& G = groups.groups[gi];
        if (G.grouped) {
            lists.group_at[gi] = lists.entries;
            lists.entries += avd_group::table_entries(clips[G.members.front().clip].planes(), G.frames);
        } else {
            ClipSlot& slot = slots[(size_t)G.members.front().clip];
            slot.rowbuf_off = G.rowbuf_off; slot.lappart_off = G.lappart_off;
        }
    }
    rowbuf_elems = groups.rowbuf_elems; lappart_elems = groups.lappart_elems;
    if (int e = avd_ws_reserve_frames(ctx, n, rowbuf_elems, lappart_elems)) return e;
    if (int e = avd_ws_reserve_fb(ctx, n)) return e;
    if (int e = reserve_lists(ctx, lists)) return e;
    // every continued slot's buffer (an empty slot's first call; frames = 0: still empty if the call fails), and the two tables of the copy kernel
    StreamCopyTable restore{}, save{};
    int nrestore = 0, nsave = 0;
    for (int c = 0; c < nclips; c++) {
        if (!stream[c]) continue;
        if (int e = stream[c]->d_prev.reserve(ctx, kStreamPrevBytes)) return e;
        if (nsave >= kStreamSlots) { ctx->err = "internal error: more continued clips than stream slots"; return AVD_ERR_DEVICE; }
        uint4* const kept = reinterpret_cast<uint4*>(stream[c]->d_prev.p);
        if (plan.carry[c] >= 0) restore.e[nrestore++] = {kept, plan.carry[c]};
        save.e[nsave++] = {kept, plan.f0[c] + clips[c].n - 1};
    }
    // pass 2: per clip, stage (host input) -> fused full-resolution kernel -> hash, in the clip's slot
    kmark_reset(ctx);
    ctx->ingest.stage_bytes = 0;
    ctx->ingest.stage_copies = 0;
    // profiling only: an empty launch in front of the first mark, so that the first region is the first kernel and not the queue's wake-up from idle as well
    if (ctx->profiling) hipLaunchKernelGGL(k_wake, dim3(1), dim3(64), 0, ctx->stream);
    // A stage boundary and the kernel region that begins there are ONE event (kmark's `shared`), here and below: stages 0 .. 3 and the regions
    // recorded at enqueue are two partitions of the same interval.  The first region is the first clip's ingest, the upload of the list table
    // (host input staged for it) included.
    kmark(ctx, AVD_K_PREPROCESS, stage_mark(ctx, 0));
    bool first_clip = true;
    // each filled slot's frame becomes its clip's carry frame (device to device, ordered on the stream like everything else; inside the first
    // region): ONE launch for all of them
    if (nrestore) HIP_TRY(ctx, stream_copy(ctx, restore, nrestore, false));
    if (int e = upload_lists(ctx, clips, nclips, lists, &groups, stage_at.data())) return e;
    std::copy(plan.clipstart.begin(), plan.clipstart.end(), ws.h_clipstart.p);
    // one ingest and one hash launch per group, in the order of the groups' first clips: a clip alone in its group runs the per-clip path (with the
    // option off every clip does), several clips run ONE listed launch over all their frames with the group's table of output frames
    std::vector<int> launched;                             // "ingest_groups" of this call
    int grouped_launches = 0, grouped_frames = 0;
    for (size_t gi = 0; gi < groups.groups.size(); gi++) {
        const avd_group::Group& G = groups.groups[gi];
        const int c = G.members.front().clip;
        const IngestClip& k = clips[c];
        ClipSlot& slot = slots[c];                         // a group's launches run with its first clip's slot: the geometry is the group's
        // the tables again: a cache hit (pass 1 built them) unless the call has > kGeomCache geometries -- then pass 1 has evicted this one since,
        // the slot's copies point into freed tables, and they are rebuilt here (same geometry, same sizes: the offsets hold)
        if (int e = avd_ws_geometry(ctx, k.disp_h(), k.disp_w(), slot)) return e;
        if (!first_clip) kmark(ctx, AVD_K_PREPROCESS);
        first_clip = false;
        if (!G.grouped) {
            if (int e = preprocess_clip(ctx, slot, k, stage_at[c], lists, c)) return e;
            kmark(ctx, AVD_K_HASH);
            if (int e = launch_hash(ctx, slot, k.n)) return e;
        } else {
            for (const avd_group::Member& m : G.members)
                if (int e = stage_clip(ctx, clips[m.clip], stage_at[m.clip], lists, m.clip)) return e;
            slot.rowbuf_off = G.rowbuf_off; slot.lappart_off = G.lappart_off;
            const uint8_t* const* d_tab = ws.d_ftab + lists.group_at[gi];
            const int* d_out = reinterpret_cast<const int*>(d_tab + (size_t)k.planes() * G.frames);
            const FrameTable ft{G.key.vec != 0, d_out, G.frames};
            auto plane = [&](int p) { return p < k.planes() ? reinterpret_cast<const uint8_t*>(d_tab + (size_t)p * G.frames) : nullptr; };
            if (int e = launch_preprocess(ctx, slot, k, plane(0), plane(1), plane(2), &ft)) return e;
            kmark(ctx, AVD_K_HASH);
            if (int e = launch_hash(ctx, slot, G.frames, d_out)) return e;
            grouped_launches++;
            grouped_frames += G.frames;
        }
        const int row[4] = {c, (int)G.members.size(), G.frames, ctx->ingest.plan.kernel};
        launched.insert(launched.end(), row, row + 4);
    }
    kmark(ctx, AVD_K_OTHER, stage_mark(ctx, 1));
    const int* clipstart = nullptr;                        // one segment: frame 0 is the only one without a predecessor
    // more than one segment needs the table (plan.clipstart: 1 at every carry frame and at the first frame of a clip without one, 0 at the first
    // own frame of a continued clip); a batch without a continued clip uploads it as it always did, whatever empty clips the call lists
    if (plan.segments > 1 || (nclips > 1 && plan.carries == 0)) {
        HIP_TRY(ctx, hipMemcpyAsync(ws.d_clipstart, ws.h_clipstart, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
        clipstart = ws.d_clipstart;
    }
    kmark(ctx, n < 2 ? AVD_K_RECORDS : AVD_K_PYRAMID, stage_mark(ctx, 2));     // stage 2 opens with that kernel; its launcher marks the same id again
    // from here on an error return must not leave a tail behind: a later avd_synchronize would settle it from a stale h_rec
    struct TailOnError {
        avd_ctx* c;
        bool ok = false;
        ~TailOnError() { if (!ok) c->tail.active = 0; }
    } tail_on_error{ctx};
    if (n < 2) launch_records(ctx, 0, 0, 0, clipstart);     // one frame: no pair, no flow
    else if (int e = run_flow_chunks(ctx, ws.d_small, n, nullptr, nullptr, nullptr, true, clipstart)) return e;
    kmark(ctx, AVD_K_OTHER, stage_mark(ctx, 3));
    // every continued clip's last frame becomes its slot's, in ONE launch: only here, behind everything that can refuse or fail for want of memory
    // (nothing has written d_small, d_hash or d_lap since the ingest), so that such a call leaves every slot as it was
    if (nsave) HIP_TRY(ctx, stream_copy(ctx, save, nsave, true));
    // into PINNED memory: a device-to-host copy into the caller's pageable buffer would block this thread until
    // the whole call is done and it would not be asynchronous at all; avd_synchronize hands the records over
    // (all n of them, the slot's frame included: the deferred re-run finds its chunk's flag words where it always does)
    ctx->pending_runs = plan.runs;                         // (can throw: while an error still drops the tail, and before the counters move)
    ctx->ingest_groups.reserve(launched.size());           // (the same: the swap below cannot)
    HIP_TRY(ctx, hipMemcpyAsync(ws.h_rec, ws.d_rec, sizeof(avd_frame_record) * n, hipMemcpyDeviceToHost, ctx->stream));
    tail_on_error.ok = true;
    for (int c = 0; c < nclips; c++)
        if (stream[c]) stream[c]->frames = (int)std::min<int64_t>((int64_t)stream[c]->frames + clips[c].n, INT32_MAX);
    ctx->pending_out = records;
    const int launches = (int)groups.groups.size();
    ctx->ingest_call[0] = launches; ctx->ingest_call[1] = launches; ctx->ingest_call[2] = grouped_launches; ctx->ingest_call[3] = grouped_frames;
    ctx->ingest_groups.swap(launched);
    ctx->stream_call[0] = plan.carries; ctx->stream_call[1] = nrestore > 0; ctx->stream_call[2] = nsave > 0; ctx->stream_call[3] = n;
    if (ctx->tail.active) tail_register(ctx);              // from here on a waiting thread may settle this call's tail
    if (!ctx->counted_in_flight) { ctx->counted_in_flight = 1; g_calls_in_flight.fetch_add(1, std::memory_order_relaxed); }
    kmark(ctx, AVD_K_COUNT, stage_mark(ctx, 4));           // end of the last region
    ctx->last_n = n;
    ctx->rec_n = own; ctx->rec_off = plan.runs.front().first; ctx->rec_mapped = mapped;
    return AVD_OK;
}

// The two list entries: every avd_clip (from_public) or avd_picture (from_picture) becomes an IngestClip, the first refusal ends the call.
template <typename Public, typename Convert>
static int impl_analyze_list_async(avd_ctx* ctx, const Public* list, int nclips, avd_frame_record* records, Convert&& convert)
{
    if (!ctx) return AVD_ERR_ARG;
    if (nclips < 0 || (nclips > 0 && !list)) { ctx->err = "bad clip list"; return AVD_ERR_ARG; }
    std::vector<IngestClip> ks((size_t)nclips);
    for (int c = 0; c < nclips; c++)
        if (int e = refuse(ctx, convert(list[c], ks[c]))) return e;
    return impl_analyze_async(ctx, ks.data(), nclips, records);
}
static Refusal clip_from_public(const avd_clip& c, IngestClip& k) { k = from_public(c); return {0, nullptr}; }

static int impl_synchronize(avd_ctx* ctx)
{
    if (!ctx) return AVD_ERR_ARG;
    struct Uncount {                                        // whatever happens below, the call is no longer in flight afterwards
        avd_ctx* c;
        ~Uncount() { if (c->counted_in_flight) { c->counted_in_flight = 0; g_calls_in_flight.fetch_sub(1, std::memory_order_relaxed); } }
    } uncount{ctx};
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->tail.active) {
        // fast Farneback mode: the records of the call's last chunk carry the level kernels' flag words (tail_settle) -- unless a thread that
        // was waiting for its own context has settled this one already
        const hipError_t e = ctx->tail_registered ? wait_helping(ctx, ctx->tail_ev) : hipStreamSynchronize(ctx->stream);
        tail_unregister(ctx);
        if (e != hipSuccess) { ctx->tail.active = 0; ctx->pending_out = nullptr; ctx->err = hipGetErrorString(e); return AVD_ERR_DEVICE; }
        if (ctx->tail.active) ctx->tail_rc = tail_settle(ctx);
    }
    if (ctx->tail_rc) {                                     // the re-run could not be enqueued (by this thread or by a helper): the call has failed
        const int rc = ctx->tail_rc;
        ctx->tail_rc = 0; ctx->pending_out = nullptr;
        return rc;
    }
    HIP_TRY(ctx, wait_helping(ctx, nullptr));
    if (ctx->pending_out) {
        // the call's own frames, run after run (avd_stream_plan.h): the frames restored from stream slots lie between the runs and stay behind
        avd_frame_record* out = ctx->pending_out;
        ctx->last_rerun = 0;
        for (const avd_stream::Run& r : ctx->pending_runs) {
            const avd_frame_record* const got = ctx->ws.h_rec + r.first;
            std::memcpy(out, got, sizeof(avd_frame_record) * (size_t)r.count);
            for (int i = 0; i < r.count; i++) ctx->last_rerun += got[i].reserved != 0;
            out += r.count;
        }
        ctx->pending_out = nullptr;
    }
    // only a mark list that an avd_analyze_* call closed (its last mark is AVD_K_COUNT: impl_analyze_async, tail_settle) is a call's timeline;
    // anything else -- marks of a call that failed half way -- would drop its last region and replace the figures of the last drained call
    if (ctx->profiling && ctx->kmark_used > 1 && ctx->kmark_id[ctx->kmark_used - 1] == AVD_K_COUNT) {
        for (float& v : ctx->kernel_ms) v = 0.f;
        for (int i = 0; i + 1 < ctx->kmark_used; i++) {
            float ms = 0.f;
            if (ctx->kmark_id[i] < AVD_K_COUNT && hipEventElapsedTime(&ms, ctx->kmark_at[i], ctx->kmark_at[i + 1]) == hipSuccess)
                ctx->kernel_ms[ctx->kmark_id[i]] += ms;
        }
        ctx->kmark_incomplete = ctx->kmark_overflow;
    }
    kmark_reset(ctx);
    if (ctx->profiling && ctx->stage_marks == 5) {
        // stages as in include/avd.h (avd_set_profiling): 0 staging copies + preprocess + aHash of every clip, 1 upload of the clip-start table,
        // 2 Farneback + flow statistics + the record kernel, 3 records copy-out
        for (int i = 0; i < 4; i++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ctx->stage_ev[i], ctx->stage_ev[i + 1]) == hipSuccess) ctx->stage_ms[i] = ms;
        }
        // 4 / 5, of the call's last chunk.  One event pair (fast mode, and the fused 320-px kernel of exact mode): 4 = the 320-px level, 5 = 0.
        // Twelve events (the two-kernel path of exact mode): 4 / 5 = mean duration of one k_uv<320> / k_hscan<320> launch
        float sum[2] = {0.f, 0.f}; int cnt[2] = {0, 0};
        for (int i = 0; i + 1 < ctx->kern_ev_used; i += 2) {     // level320_mark events of the drained call
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ctx->kern_ev[i], ctx->kern_ev[i + 1]) == hipSuccess) { sum[(i >> 1) & 1] += ms; cnt[(i >> 1) & 1]++; }
        }
        for (int k = 0; k < 2; k++) ctx->stage_ms[4 + k] = cnt[k] ? sum[k] / cnt[k] : 0.f;
        ctx->stage_marks = 0;                       // the events belong to the call that was just drained
    }
    return AVD_OK;
}

static int impl_timer_start(avd_ctx* ctx)
{
    if (!ctx) return AVD_ERR_ARG;
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return AVD_OK;
}

static int impl_timer_stop(avd_ctx* ctx, float* elapsed_ms)
{
    if (!ctx || !elapsed_ms) return AVD_ERR_ARG;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    HIP_TRY(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return AVD_OK;
}

static int impl_set_profiling(avd_ctx* ctx, int enable)
{
    if (!ctx) return AVD_ERR_ARG;
    ctx->profiling = enable != 0;
    return AVD_OK;
}

static int impl_stage_ms(avd_ctx* ctx, int stage, float* ms)
{
    if (!ctx || !ms || stage < 0 || stage > 5) return AVD_ERR_ARG;
    *ms = ctx->stage_ms[stage];
    return AVD_OK;
}

static int impl_kernel_ms(avd_ctx* ctx, int id, float* ms)
{
    if (!ctx || !ms || id < 0 || id >= AVD_K_COUNT) return AVD_ERR_ARG;
    if (ctx->kmark_incomplete) { ctx->err = "avd_kernel_ms: the profiled call had more kernel regions than the library records (96): split it"; return AVD_ERR_ARG; }
    *ms = ctx->kernel_ms[id];
    return AVD_OK;
}

static int64_t impl_debug_fetch(avd_ctx* ctx, const char* name, void* out, size_t out_bytes)
{
    if (!ctx || !name || !out) return AVD_ERR_ARG;
    Workspace& ws = ctx->ws;
    const int n = ctx->last_n;
    const void* src = nullptr;
    size_t bytes = 0;
    auto level = [&](const char* prefix) -> int {
        const size_t L = std::strlen(prefix);
        if (std::strncmp(name, prefix, L) == 0 && name[L] >= '0' && name[L] < '0' + AVD_FB_LEVELS && name[L + 1] == 0)
            return name[L] - '0';
        return -1;
    };
    int k;
    {   // host state, not device buffers: what the last ingest launch / the last ingest call of the context did (IngestRecord)
        const IngestRecord& in = ctx->ingest;
        const char* const no_launch = "no ingest kernel was launched on this context";
        const char* const no_call = "no ingest call has run on this context";
        // the stream slots as they are now: frames absorbed and the position "stream_map" maps to the slot (-1: none)
        int stream_state[kStreamSlots][2];
        for (int k = 0; k < kStreamSlots; k++) {
            stream_state[k][0] = ctx->streams[k].frames;
            stream_state[k][1] = -1;
            for (int p = 0; p < kStreamMapPositions; p++)
                if (ctx->stream_map[p] == k + 1) stream_state[k][1] = p;
        }
        // type null: a short `out` gets the first out_bytes; otherwise it is refused with the type's name
        const struct { const char* name; const void* p; size_t bytes; bool recorded; const char* missing; const char* type; } host_state[] = {
            {"ingest_plan", &in.plan, sizeof in.plan, in.launched != 0, no_launch, nullptr},
            {"ingest_rotate", &in.rotate, sizeof in.rotate, in.launched != 0, no_launch, "int32[1]"},
            {"ingest_range", &in.range, sizeof in.range, in.launched != 0, no_launch, "int32[1]"},
            {"ingest_format", &in.format, sizeof in.format, in.launched != 0, no_launch, "int32[1]"},
            {"ingest_list", in.list, sizeof in.list, in.launched != 0, no_launch, "int32[2]"},
            {"stage_copies", &in.stage_copies, sizeof in.stage_copies, in.stage_copies >= 0, no_call, "int64[1]"},
            {"stage_bytes", &in.stage_bytes, sizeof in.stage_bytes, in.stage_bytes >= 0, no_call, "int64[1]"},
            {"stream_state", stream_state, sizeof stream_state, true, nullptr, "int32[8][2]"},
            {"stream_call", ctx->stream_call, sizeof ctx->stream_call, true, nullptr, "int32[4]"},
            {"ingest_call", ctx->ingest_call, sizeof ctx->ingest_call, true, nullptr, "int32[4]"},
            {"ingest_groups", ctx->ingest_groups.data(), sizeof(int) * ctx->ingest_groups.size(), true, nullptr, "int32[launches][4]"},
            {"fb_model", ctx->fb_model, sizeof ctx->fb_model, ctx->fb_model_valid != 0, "no call has run the Farneback stage on this context", "int32[4]"},
            {"fb_wide320_launches", &ctx->fb_wide320_launches, sizeof ctx->fb_wide320_launches, ctx->fb_model_valid != 0, "no call has run the Farneback stage on this context", "int32[1]"},
            {"fb_wide320_up_launches", &ctx->fb_wide320_up_launches, sizeof ctx->fb_wide320_up_launches, ctx->fb_model_valid != 0, "no call has run the Farneback stage on this context", "int32[1]"},
            {"audio_layout", ctx->audio_layout_rec, sizeof ctx->audio_layout_rec, ctx->audio_layout_valid != 0, "no avd_audio_features call has converted on this context (option \"audio_rate\")", "int32[12]"},
            {"audio_map_call", ctx->audio_map_call, sizeof ctx->audio_map_call, ctx->audio_map_valid != 0, "no avd_audio_features call with an \"audio_track_slot\" list has run on this context", "int32[6]"},
        };
        for (const auto& e : host_state) {
            if (std::strcmp(name, e.name) != 0) continue;
            if (!e.recorded) { ctx->err = std::string(e.name) + " not recorded yet: " + e.missing; return AVD_ERR_ARG; }
            if (e.type && out_bytes < e.bytes) { ctx->err = std::string(e.name) + " is " + e.type; return AVD_ERR_ARG; }
            bytes = std::min(e.bytes, out_bytes);
            if (bytes) std::memcpy(out, e.p, bytes);      // (no launch yet: "ingest_groups" is empty)
            return (int64_t)bytes;
        }
    }
    if (std::strcmp(name, "cnn_plan") == 0) {          // host state: the kernel shape (CnnShape) of each convolution of the last CNN forward
        if (!ctx->cnn_plan_valid) { ctx->err = "cnn_plan not recorded yet: no CNN forward has run on this context"; return AVD_ERR_ARG; }
        bytes = std::min(sizeof(ctx->cnn_plan), out_bytes);
        std::memcpy(out, ctx->cnn_plan, bytes);
        return (int64_t)bytes;
    }
    if (std::strcmp(name, "cnn_tap") == 0) {           // what option "cnn_tap" made the last CNN forward copy aside
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        return cnn_tap_fetch(ctx, out, out_bytes);
    }
    if (std::strncmp(name, "audio_rs_", 9) == 0 || std::strcmp(name, "audio_pcm") == 0) {   // the converter's part of the last avd_audio_features call (option "audio_rate")
        const bool rs_plan = std::strcmp(name, "audio_rs_plan") == 0, rs_taps = std::strcmp(name, "audio_rs_taps") == 0, rs_tracks = std::strcmp(name, "audio_rs_tracks") == 0;
        if (!rs_plan && !rs_taps && !rs_tracks && std::strcmp(name, "audio_pcm") != 0) { ctx->err = "unknown debug buffer"; return AVD_ERR_ARG; }
        if (!ctx->audio_rs_valid) { ctx->err = "audio_rs_plan / audio_rs_taps / audio_rs_tracks / audio_pcm not recorded: the last avd_audio_features call on this context did not convert (option \"audio_rate\")"; return AVD_ERR_ARG; }
        const int* rp = ctx->audio_rs_plan;
        const void* from = nullptr;
        size_t have = 0;
        const char* type = nullptr;
        if (rs_plan) { from = rp; have = sizeof(ctx->audio_rs_plan); type = "audio_rs_plan is int32[8]"; }
        else if (rs_taps) { const std::vector<int>& b = ctx->audio_rs_bank[avd_resample::rate_index(rp[0])]; from = b.data(); have = sizeof(int) * b.size(); type = "audio_rs_taps is int32[U][T]"; }
        else if (rs_tracks) { from = ctx->audio_rs_tracks; have = sizeof(int) * 2 * (size_t)ctx->audio_rs_ntracks; type = "audio_rs_tracks is int32[tracks][2]"; }
        if (type) {
            if (out_bytes < have) { ctx->err = type; return AVD_ERR_ARG; }
            if (have) std::memcpy(out, from, have);
            return (int64_t)have;
        }
        src = ws.d_audio_pcm.p ? ws.d_audio_pcm.p + ctx->audio_rs_pcm_at : nullptr;   // null after avd_release_workspace: "buffer not allocated yet" below
        bytes = sizeof(int16_t) * (size_t)rp[7];
        if (src && ctx->audio_rs_mapped) {             // a list call ("audio_track_slot"): the tracks' new outputs lie region by region; they are handed over side by side
            if (out_bytes < bytes) { ctx->err = "audio_pcm is int16[output samples]"; return AVD_ERR_ARG; }
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            char* to = static_cast<char*>(out);
            for (int t = 0; t < ctx->audio_rs_ntracks; t++) {
                const size_t part = sizeof(int16_t) * (size_t)ctx->audio_rs_tracks[t][1];
                if (part) HIP_TRY(ctx, hipMemcpy(to, ws.d_audio_pcm.p + ctx->audio_rs_tracks[t][0], part, hipMemcpyDeviceToHost));
                to += part;
            }
            return (int64_t)bytes;
        }
    }
    else if (std::strncmp(name, "audio_", 6) == 0) {   // the last avd_audio_features of this context: its window plan (host state) and its two scratch arrays
        const bool plan = std::strcmp(name + 6, "plan") == 0, xw = std::strcmp(name + 6, "xw") == 0, mag = std::strcmp(name + 6, "mag") == 0;
        const bool tracks = std::strcmp(name + 6, "tracks") == 0;
        if (!plan && !xw && !mag && !tracks && std::strcmp(name + 6, "host") != 0) { ctx->err = "unknown debug buffer"; return AVD_ERR_ARG; }
        if (!ctx->audio_plan_valid) { ctx->err = "audio_plan / audio_xw / audio_mag not recorded yet: no avd_audio_features call has run on this context"; return AVD_ERR_ARG; }
        if (std::strcmp(name + 6, "host") == 0) {      // int32[2]: microseconds spent forming the short lengths' tables, distinct short lengths
            if (out_bytes < sizeof(ctx->audio_host)) { ctx->err = "audio_host is int32[2]"; return AVD_ERR_ARG; }
            std::memcpy(out, ctx->audio_host, sizeof(ctx->audio_host));
            return (int64_t)sizeof(ctx->audio_host);
        }
        if (tracks) {                                  // int32[tracks][3]: first window, windows, length of the last window
            const size_t have = sizeof(int) * 3 * (size_t)ctx->audio_ntracks;
            if (out_bytes < have) { ctx->err = "audio_tracks is int32[tracks][3]"; return AVD_ERR_ARG; }
            std::memcpy(out, ctx->audio_tracks, have);
            return (int64_t)have;
        }
        if (plan) {
            if (out_bytes < sizeof(ctx->audio_plan)) { ctx->err = "audio_plan is int32[4]"; return AVD_ERR_ARG; }
            std::memcpy(out, ctx->audio_plan, sizeof(ctx->audio_plan));
            return (int64_t)sizeof(ctx->audio_plan);
        }
        // launch_audio_features lays ws.d_audio_buf out as xw [nwin][win] | mag [nwin][win / 2 + 1] | the FFT path's intermediate
        const size_t nwin = (size_t)ctx->audio_plan[0], win = (size_t)ctx->audio_plan[1];
        if (!ws.d_audio_buf) { ctx->err = "buffer not allocated yet"; return AVD_ERR_ARG; }   // avd_release_workspace since that call
        src = xw ? ws.d_audio_buf.p : ws.d_audio_buf.p + nwin * win;
        bytes = (xw ? nwin * win : nwin * (win / 2 + 1)) * sizeof(double);
    }
    else if (std::strcmp(name, "area") == 0) { src = ws.d_area; bytes = (size_t)n * 1024; }
    else if (std::strcmp(name, "small") == 0) { src = ws.d_small; bytes = (size_t)n * AVD_NPIX; }
    // the Farneback scratch holds ONE chunk (kFbChunk pairs): for longer clips these are the last chunk's buffers
    else if ((k = level("pyr")) >= 0 && k == 0 && fb_fold_blur_eff(ctx->fb_fold_blur, ctx->cv2_model)) { ctx->err = "pyr0 does not exist while fb_fold_blur is on (the polynomial expansion forms the 320-px blur itself)"; return AVD_ERR_ARG; }
    else if ((k = level("pyr")) >= 0) { src = ws.d_pyr[k]; bytes = (size_t)std::min(n, ws.fb_cap + 1) * (AVD_NPIX >> (2 * k)) * 4; }
    else if ((k = level("poly")) >= 0) { src = ws.d_poly[k]; bytes = (size_t)std::min(n, ws.fb_cap + 1) * 5 * (AVD_NPIX >> (2 * k)) * 4; }
    else if ((k = level("flow")) >= 0 && k == 0 && ws.fb_holds.flow0_late.pairs > 0) {   // a call without dense flow left this one unwritten: form it now
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (int e = launch_flow0_late(ctx)) return e;
        src = ws.fb_holds.flow[0]; bytes = (size_t)std::min(std::max(n - 1, 0), ws.fb_cap) * 2 * AVD_NPIX * 4;
    }
    else if ((k = level("flow")) >= 0) { src = ws.fb_holds.flow[k] ? ws.fb_holds.flow[k] : ws.d_flow[k]; bytes = (size_t)std::min(std::max(n - 1, 0), ws.fb_cap) * 2 * (AVD_NPIX >> (2 * k)) * 4; }
    else if (std::strcmp(name, "pairdiff") == 0) { src = ws.d_pairdiff; bytes = (size_t)std::min(std::max(n - 1, 0), ws.fb_cap) * kPairDiffTiles * sizeof(int); }
    else if (std::strcmp(name, "vs0") == 0) { src = ws.d_vs0; bytes = fb_two_scratch_size((size_t)ws.fb_cap).vs0 * sizeof(double); }
    else { ctx->err = "unknown debug buffer"; return AVD_ERR_ARG; }
    if (!src) { ctx->err = "buffer not allocated yet"; return AVD_ERR_ARG; }
    bytes = std::min(bytes, out_bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return (int64_t)bytes;
}

// Wait for work the caller enqueued on ANOTHER stream (e.g. torch's current stream, which produced or is still
// producing a device input) before anything submitted to this context afterwards: an event on the producer stream,
// waited for by the context's stream.  A null handle names the legacy default stream.
static int impl_wait_stream(avd_ctx* ctx, void* producer)
{
    if (!ctx) return AVD_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_in, (hipStream_t)producer));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
    return AVD_OK;
}

// Give the scratch memory back (a service keeps idle contexts cheap); the next call re-reserves it.
static int impl_release_workspace(avd_ctx* ctx)
{
    if (!ctx) return AVD_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int e = impl_synchronize(ctx)) return e;
    ctx->ws = Workspace{};                                  // the uploaded weights (ctx->weights) are state and stay
    ctx->rec_n = 0; ctx->rec_mapped = 0;
    return AVD_OK;
}

// Tuning / test switches (kOptions above).
static int impl_set_option(avd_ctx* ctx, const char* name, int value)
{
    if (!ctx || !name) return AVD_ERR_ARG;
    const Option* o = find_option(ctx, name, true);
    if (!o) return AVD_ERR_ARG;
    if (!o->norm(value)) { ctx->err = o->refused; return AVD_ERR_ARG; }
    if (o->check)
        if (const char* why = o->check(ctx, value)) { ctx->err = why; return AVD_ERR_ARG; }
    if (o->act) o->act(ctx, value);
    else ctx->*o->field = value;
    return AVD_OK;
}

// The value an option has NOW (environment defaults included), and the read-only counters.
static int impl_get_option(avd_ctx* ctx, const char* name, int* value)
{
    if (!ctx || !name || !value) return AVD_ERR_ARG;
    const Option* o = find_option(ctx, name, false);
    if (!o) return AVD_ERR_ARG;
    *value = o->read ? o->read(ctx) : ctx->*o->field;
    return AVD_OK;
}

// Timing of the extensions: `reps` repetitions of `launch` between ev0 and ev1 on the context's stream; *out_ms = mean time of one
template <typename F>
static int time_reps(avd_ctx* ctx, int reps, F&& launch, float* out_ms)
{
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int r = 0; r < reps; r++)
        if (int e = launch()) return e;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *out_ms = ms / reps;
    return 0;
}

// ---- CNN extension (avd_cnn.hip; never part of ai_score) ---------------------------------------------------------
static int impl_cnn_set_weights(avd_ctx* ctx, const uint16_t* w, size_t n_w, const float* b, size_t n_b)
{
    if (!ctx || !w || !b) return AVD_ERR_ARG;
    size_t want_w = 0, want_b = 0;
    cnn_param_counts(&want_w, &want_b);
    if (n_w != want_w || n_b != want_b) { ctx->err = "avd_cnn_set_weights: parameter counts differ from avd_cnn_param_counts"; return AVD_ERR_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return cnn_set_weights(ctx, w, b);
}

static int impl_cnn_forward(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride, int64_t frame_stride,
                            float* logits, int reps, float* forward_ms)
{
    if (!ctx) return AVD_ERR_ARG;
    if ((!bgr || !logits) && n > 0) { ctx->err = "null pointer"; return AVD_ERR_ARG; }
    if (n < 0 || h < 2 || w < 2 || row_stride < (int64_t)w * 3) { ctx->err = "bad frame geometry"; return AVD_ERR_ARG; }
    if (n == 0) return AVD_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Workspace& ws = ctx->ws;
    if (!ctx->weights.d_cnn_w) { ctx->err = "avd_cnn_set_weights has not been called"; return AVD_ERR_ARG; }
    // frames per forward pass: bounds the activation scratch (4 x 1.6 MB per frame); avd_set_option "cnn_chunk", 1 ... 1024
    // (32-bit byte offsets inside an activation); the late stages fill the chip better with more frames per pass
    const int kChunk = ctx->cnn_chunk;
    if (ctx->cnn_tap && (n > kChunk || reps > 0)) { ctx->err = "avd_cnn_forward: with option cnn_tap set, one pass (n <= cnn_chunk) and no timing repetitions"; return AVD_ERR_ARG; }
    if (int e = cnn_reserve(ctx, std::min(n, kChunk))) return e;
    const uint8_t* d_bgr = nullptr;
    if (int e = stage_input(ctx, bgr, mem, plane_span(frame_stride, n, row_stride, h, (size_t)w * 3), &d_bgr)) return e;
    float total_ms = 0.f;
    for (int f0 = 0; f0 < n; f0 += kChunk) {
        const int m = std::min(kChunk, n - f0);
        const uint8_t* src = d_bgr + (size_t)frame_stride * f0;
        auto forward = [&] { return launch_cnn_forward(ctx, src, m, h, w, row_stride, frame_stride); };
        if (int e = forward()) return e;
        if (reps > 0 && forward_ms) {
            float ms = 0.f;
            if (int e = time_reps(ctx, reps, forward, &ms)) return e;
            total_ms += ms;
        }
        // the logits buffer is reused by the next chunk: the copy is ordered before it on the same stream
        HIP_TRY(ctx, hipMemcpyAsync(logits + (size_t)f0 * 1000, ws.d_cnn_logits, sizeof(float) * (size_t)m * 1000, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (reps > 0 && forward_ms) *forward_ms = total_ms;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AVD_OK;
}

// ---- ViT-B/16 patch embedding (extension; never part of ai_score) ---------------------------------------------
static int impl_vit_set_weights(avd_ctx* ctx, const uint16_t* w_bf16, const float* bias)
{
    if (!ctx || !w_bf16) return AVD_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Weights& wt = ctx->weights;
    if (int e = wt.d_vit_w.reserve(ctx, (size_t)768 * 768)) return e;
    if (int e = wt.d_vit_bias.reserve(ctx, (size_t)768)) return e;
    // the GEMM reads its operands in 1-KiB blocks (avd_vit.hip): re-tile the row-major weight once, here
    std::vector<uint16_t> blocked((size_t)768 * 768);
    gemm_block_operand(w_bf16, blocked.data(), 768, 768);
    HIP_TRY(ctx, hipMemcpyAsync(wt.d_vit_w, blocked.data(), sizeof(uint16_t) * 768 * 768, hipMemcpyHostToDevice, ctx->stream));
    if (bias) HIP_TRY(ctx, hipMemcpyAsync(wt.d_vit_bias, bias, sizeof(float) * 768, hipMemcpyHostToDevice, ctx->stream));
    wt.vit_has_bias = bias != nullptr;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AVD_OK;
}

static int impl_vit_patch_embed(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride,
                                int64_t frame_stride, void* tokens, int tokens_mem, int tokens_bf16, int reps, float* gemm_ms)
{
    if (!ctx) return AVD_ERR_ARG;
    if ((!bgr || !tokens) && n > 0) { ctx->err = "null pointer"; return AVD_ERR_ARG; }
    if (n < 0 || h < 2 || w < 2 || row_stride < (int64_t)w * 3) { ctx->err = "bad frame geometry"; return AVD_ERR_ARG; }
    if (tokens_mem != AVD_MEM_HOST && tokens_mem != AVD_MEM_DEVICE) { ctx->err = "tokens_mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"; return AVD_ERR_ARG; }
    if (n == 0) return AVD_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Workspace& ws = ctx->ws;
    const Weights& wt = ctx->weights;
    if (!wt.d_vit_w) { ctx->err = "avd_vit_set_weights has not been called"; return AVD_ERR_ARG; }
    const size_t m = (size_t)n * 196;
    const size_t m_pad = (m + kGemmRowPad - 1) / kGemmRowPad * kGemmRowPad;   // the persistent GEMM reads whole 256-row tiles of A
    if (ws.d_vit_patches.cap < m_pad * 768) {
        // a regrown buffer is zero-filled (the rows that pad the last tile are read, never written) -- or does not exist
        if (int e = ws.d_vit_patches.reserve(ctx, m_pad * 768)) return e;
        auto zero_fill = [&]() -> int { HIP_TRY(ctx, hipMemsetAsync(ws.d_vit_patches, 0, m_pad * 768 * sizeof(uint16_t), ctx->stream)); return 0; };
        if (int e = zero_fill()) { ws.d_vit_patches.reset(); return e; }
    }
    void* d_tok = tokens;
    const size_t esz = tokens_bf16 ? sizeof(uint16_t) : sizeof(float);
    if (tokens_mem == AVD_MEM_HOST) {
        if (int e = ws.d_vit_tokens.reserve(ctx, m * 768)) return e;
        d_tok = ws.d_vit_tokens;
    }
    const uint8_t* d_bgr = nullptr;
    if (int e = stage_input(ctx, bgr, mem, plane_span(frame_stride, n, row_stride, h, (size_t)w * 3), &d_bgr)) return e;
    const float* d_bias = wt.vit_has_bias ? wt.d_vit_bias : nullptr;
    if (int e = launch_vit_patch_embed(ctx, d_bgr, n, h, w, row_stride, frame_stride, wt.d_vit_w, d_bias, d_tok, tokens_bf16, ws.d_vit_patches)) return e;
    if (reps > 0 && gemm_ms) {
        // the GEMM alone (the patches stay resident)
        auto gemm = [&] { return launch_gemm_bf16_nt(ctx, ws.d_vit_patches, wt.d_vit_w, d_bias, d_tok, tokens_bf16, (int)m, 768, 768); };
        if (int e = time_reps(ctx, reps, gemm, gemm_ms)) return e;
    }
    if (tokens_mem == AVD_MEM_HOST)
        HIP_TRY(ctx, hipMemcpyAsync(tokens, d_tok, esz * m * 768, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AVD_OK;
}

// ---- LayerNorm / softmax (extensions; never part of ai_score) ------------------------------------------------------------
// x / y: host or device (both the same side), gamma / beta: host float[cols].  Host operands are staged through the
// extension scratch (d_vit_tokens, grown on demand).
static int impl_rowop(avd_ctx* ctx, int op, const void* x, int mem, int bf16, int64_t rows, int cols, const float* gamma, const float* beta,
                      float eps, void* y, int reps, float* ms)
{
    if (!ctx) return AVD_ERR_ARG;
    if (rows < 0 || cols <= 0 || (rows > 0 && (!x || !y)) || (op == 0 && (!gamma || !beta))) { ctx->err = "bad arguments"; return AVD_ERR_ARG; }
    if (mem != AVD_MEM_HOST && mem != AVD_MEM_DEVICE) { ctx->err = "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"; return AVD_ERR_ARG; }
    if (rows == 0) return AVD_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Workspace& ws = ctx->ws;
    const size_t esz = (op == 0 && bf16) ? 2 : 4, bytes = (size_t)rows * cols * esz;
    // layout in float units: gamma | beta | pad to a multiple of 64 floats | x (rounded up to 256 bytes) | y -- the size is computed from
    // the SAME expressions the pointers below use (round 3 reserved 2 * bytes + 8 * cols + 256 B, less than pad + round-up can need)
    const size_t gb_f = 2 * (size_t)cols + ((64 - (2 * cols) % 64) % 64);
    const size_t x_bytes = (bytes + 255) / 256 * 256;
    const bool host = mem == AVD_MEM_HOST;
    const size_t want = host ? gb_f + (x_bytes + bytes + 3) / 4 : gb_f;
    if (int e = ws.d_vit_tokens.reserve(ctx, want)) return e;
    float* d_gb = ws.d_vit_tokens;                        // gamma | beta first (16-byte aligned), then x, then y
    char* d_x = (char*)x;
    char* d_y = (char*)y;
    if (op == 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_gb, gamma, sizeof(float) * cols, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_gb + cols, beta, sizeof(float) * cols, hipMemcpyHostToDevice, ctx->stream));
    }
    if (host) {
        d_x = (char*)(d_gb + gb_f);
        d_y = d_x + x_bytes;
        HIP_TRY(ctx, hipMemcpyAsync(d_x, x, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    auto run = [&]() -> int {
        return op == 0 ? launch_layernorm(ctx, d_x, d_y, bf16, rows, cols, d_gb, d_gb + cols, eps)
                       : launch_softmax(ctx, (const float*)d_x, (float*)d_y, rows, cols);
    };
    if (int e = run()) return e;
    if (reps > 0 && ms)
        if (int e = time_reps(ctx, reps, run, ms)) return e;
    if (host) HIP_TRY(ctx, hipMemcpyAsync(y, d_y, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AVD_OK;
}

// ---- audio analyzer (row N3) -------------------------------------------------------------------------------------
// Option "audio_rate" != 0: n FRAMES of audio_channels interleaved samples at that rate.  Two steps: the converter (k_audio_resample) writes the
// 16 kHz mono int16 tracks into ws.d_audio_pcm, then the analyzer runs over that buffer and the output-side cuts exactly as it runs over a caller's
// int16 track (format 1).  Every check comes before anything is staged, in the order include/avd.h lists: the argument checks and the int16
// alignment (impl_audio_features), the float32 alignment, a cut beyond the buffer, the windows array against the OUTPUT's window count.
// What a converted call's buffer is: the channel count, the mix its launches go by (id 0: no layout, "audio_channels" decides and every launch
// takes the path it took before layouts existed), and the plane stride of the CALLER's buffer.  step: what a frame offset is multiplied by to
// reach the track's first sample -- the channel count of an interleaved buffer, 1 within each plane of a planar one.
struct AudioInput { int channels = 1, step = 1, layout = 0; long long stride = 0; avd_resample::Mix mix; };
static AudioInput audio_input(const avd_ctx* ctx, int64_t n)
{
    AudioInput in;
    if (ctx->audio_rate == 0) return in;
    in.channels = in.step = ctx->audio_channels;
    if (ctx->audio_layout == 0) return in;
    in.layout = ctx->audio_layout;
    in.stride = (in.layout & avd_resample::kLayoutPlanar) ? (ctx->audio_plane_stride ? ctx->audio_plane_stride : n) : 0;
    in.mix = avd_resample::mix_of(in.layout, in.stride);
    in.channels = in.mix.channels;
    in.step = in.mix.planar ? 1 : in.channels;
    return in;
}
// refusal 3 of a call, behind the alignment checks: planes that would overlap
static bool audio_stride_refused(avd_ctx* ctx, const AudioInput& in, int64_t n)
{
    if (!in.mix.planar || in.stride >= n) return false;
    ctx->err = "audio_plane_stride: " + std::to_string(in.stride) + " samples from plane to plane, below the call's " + std::to_string((long long)n) + " frames";
    return true;
}
// The staging of a converted call.  Without a layout: stage_input, as ever.  With one, device input is read in place with its stride; a dense
// host buffer (interleaved, or planes n samples apart) is staged in one copy, a strided one plane by plane into a dense device buffer -- no byte
// twice, none outside the planes -- whose stride, n, replaces the caller's in in.mix.  "stage_bytes" / "stage_copies" say what was copied.
static int stage_audio(avd_ctx* ctx, const void* wav, int mem, int64_t n, size_t in_size, AudioInput& in, const uint8_t** d_in)
{
    const size_t plane = (size_t)n * in_size, all = plane * (size_t)in.channels;
    if (!in.mix.id) return stage_input(ctx, static_cast<const uint8_t*>(wav), mem, all, d_in);
    if (mem == AVD_MEM_DEVICE) { *d_in = static_cast<const uint8_t*>(wav); ctx->ingest.stage_bytes = 0; ctx->ingest.stage_copies = 0; return 0; }
    if (!in.mix.planar || in.stride == n) {
        if (int e = stage_input(ctx, static_cast<const uint8_t*>(wav), mem, all, d_in)) return e;
        ctx->ingest.stage_copies = 1;
    } else {
        Workspace& ws = ctx->ws;
        if (int e = ws.d_stage.reserve(ctx, all)) return e;
        for (int c = 0; c < in.channels; c++)
            HIP_TRY(ctx, hipMemcpyAsync(ws.d_stage.p + (size_t)c * plane, static_cast<const uint8_t*>(wav) + (size_t)c * (size_t)in.stride * in_size, plane,
                                        hipMemcpyHostToDevice, ctx->stream));
        *d_in = ws.d_stage;
        in.mix.stride = n;
        ctx->ingest.stage_copies = in.channels;
    }
    ctx->ingest.stage_bytes = (int64_t)all;
    return 0;
}
// debug buffer "audio_layout": a converted call has enqueued its launches
static void record_audio_layout(avd_ctx* ctx, const AudioInput& in)
{
    int* rec = ctx->audio_layout_rec;
    rec[0] = in.mix.id; rec[1] = in.mix.planar; rec[2] = in.channels; rec[3] = (int)std::min<long long>(in.stride, 0x7fffffff);
    if (in.mix.id) std::copy(in.mix.w, in.mix.w + avd_resample::kMaxChannels, rec + 4);
    else avd_resample::layout_weights(in.channels, rec + 4);
    ctx->audio_layout_valid = 1;
}

static int convert_audio_features(avd_ctx* ctx, const void* wav, int mem, int64_t n, int win, avd_audio_window* windows, int max_windows, const int* cuts, int ncuts)
{
    const int format = ctx->audio_format;
    AudioInput in = audio_input(ctx, n);
    const int channels = in.channels;
    if (format == 0 && (reinterpret_cast<uintptr_t>(wav) & 3)) { ctx->err = "audio_rate: float32 samples need a 4-byte aligned wav"; return AVD_ERR_ARG; }
    if (audio_stride_refused(ctx, in, n)) return AVD_ERR_ARG;
    if (mem != AVD_MEM_HOST && mem != AVD_MEM_DEVICE) { ctx->err = "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"; return AVD_ERR_ARG; }
    avd_resample::Ratio ratio;
    if (!avd_resample::ratio_of(ctx->audio_rate, ratio)) { ctx->err = "audio_rate: not a supported rate"; return AVD_ERR_ARG; }   // (the option refuses such a value)
    const avd_resample::Plan conv = avd_resample::plan_convert(n, ratio, cuts, ncuts);
    if (conv.refused == avd_resample::kCutBeyond) { ctx->err = "audio_cut: beyond the buffer"; return AVD_ERR_ARG; }
    if (conv.refused) { ctx->err = "audio_rate: more than 2^31 - 1 output samples"; return AVD_ERR_ARG; }
    const avd_audio::Plan plan = avd_audio::plan_call(conv.n_out, win, conv.out_cuts.data(), ncuts, max_windows);
    if (plan.refused) { ctx->err = "windows array too small"; return AVD_ERR_ARG; }
    const int nwin = plan.nwin();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Workspace& ws = ctx->ws;
    const uint8_t* d_in = nullptr;
    if (int e = stage_audio(ctx, wav, mem, n, format == 1 ? sizeof(int16_t) : sizeof(float), in, &d_in)) return e;
    if (int e = ws.d_audio_pcm.reserve(ctx, (size_t)conv.n_out + 8)) return e;
    if (int e = ws.d_audio_out.reserve(ctx, (size_t)nwin)) return e;
    if (int e = launch_audio_resample(ctx, d_in, format, channels, conv, ws.d_audio_pcm, AudioSource{}, in.mix)) return e;
    record_audio_layout(ctx, in);
    if (int e = launch_audio_features(ctx, ws.d_audio_pcm, 1, plan, ws.d_audio_out)) return e;
    HIP_TRY(ctx, hipMemcpyAsync(windows, ws.d_audio_out, sizeof(avd_audio_window) * nwin, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ws.audio_upload_pending = 0;
    ws.audio_rs_upload_pending = 0;
    return AVD_OK;
}

// Option "audio_slot" != 0: the call continues the track of an audio slot (avd_audio_stream.h plans it; include/avd.h states the rule).  The
// analyzer's buffer is ws.d_audio_pcm, laid out [held | new]: the slot's held samples are copied in front, the converter writes the new outputs
// behind them (an unconverted track: the call's samples are copied there, in their own type), the analyzer runs over whole windows of it with its
// kernels as they are, and ONE save launch leaves the new history and the new held remainder in the slot.  Everything is ordered on the context's
// stream; the host state of the slot changes only once the call has drained.  *saved: the save launch was enqueued -- a failure from there on
// has left the slot's memory in an unknown state.
static int run_audio_slot(avd_ctx* ctx, AudioSlot& slot, const avd_resample::Continue& c, const avd_resample::Ratio& ratio, const void* wav, int mem, int64_t n,
                          int win, avd_audio_window* windows, int max_windows, bool last, bool* saved, AudioInput& in)
{
    const int format = ctx->audio_format, channels = in.channels;
    const bool converted = ratio.rate != 0;
    const size_t in_size = format == 1 ? sizeof(int16_t) : sizeof(float), an_size = converted ? sizeof(int16_t) : in_size;   // bytes per input / analysed sample
    const int an_format = converted ? 1 : format;
    const size_t have = (size_t)c.held_before + (size_t)c.fresh();
    avd_audio::Plan plan;
    if (c.analysed > 0) {
        plan = avd_audio::plan_call(c.analysed, win, nullptr, 0, max_windows);
        if (plan.refused) { ctx->err = "audio_slot: windows array too small"; return AVD_ERR_ARG; }
    }
    const int nwin = plan.nwin();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Workspace& ws = ctx->ws;
    if (int e = slot.d_mem.reserve(ctx, kAudioSlotWords)) return e;
    if (int e = ws.d_audio_pcm.reserve(ctx, have * an_size / sizeof(int16_t) + 8)) return e;
    if (int e = ws.d_audio_out.reserve(ctx, (size_t)std::max(nwin, 1))) return e;
    char* buf = reinterpret_cast<char*>(ws.d_audio_pcm.p);
    const uint8_t* d_in = reinterpret_cast<const uint8_t*>(slot.d_mem.p);          // n = 0: a valid address nobody reads
    if (c.held_before) HIP_TRY(ctx, hipMemcpyAsync(buf, slot.held_at(), (size_t)c.held_before * an_size, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->audio_rs_valid = 0;
    if (converted) {
        if (n > 0)
            if (int e = stage_audio(ctx, wav, mem, n, in_size, in, &d_in)) return e;
        avd_resample::Plan conv;
        conv.r = ratio;
        conv.tile_out = c.tile_out;
        conv.n_in = n;
        conv.n_out = c.fresh();
        conv.tracks.push_back(avd_resample::Track{c.held_before, (int)c.fresh()});
        conv.tiles = c.tiles;
        AudioSource src;
        src.chunk0 = c.n_before;
        src.hist = slot.hist(slot.hist_side);
        src.hist_n = c.hist_before;
        if (int e = launch_audio_resample(ctx, d_in, format, channels, conv, ws.d_audio_pcm, src, in.mix)) return e;
        record_audio_layout(ctx, in);
    } else if (n > 0) {
        d_in = reinterpret_cast<const uint8_t*>(buf + (size_t)c.held_before * an_size);
        HIP_TRY(ctx, hipMemcpyAsync(buf + (size_t)c.held_before * an_size, wav, (size_t)n * in_size, mem == AVD_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (nwin > 0) {
        if (int e = launch_audio_features(ctx, buf, an_format, plan, ws.d_audio_out)) return e;
        HIP_TRY(ctx, hipMemcpyAsync(windows, ws.d_audio_out, sizeof(avd_audio_window) * nwin, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!last) {
        if (int e = launch_audio_slot_save(ctx, d_in, converted ? format : 1, converted ? n : 0, channels, slot.hist(slot.hist_side), c.hist_before,
                                           slot.hist(slot.hist_side ^ 1), c.hist_after, buf + (size_t)c.analysed * an_size, slot.held_at(),
                                           (int)((size_t)c.held_after * an_size / sizeof(int16_t)), saved, in.mix)) return e;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ws.audio_upload_pending = 0;
    ws.audio_rs_upload_pending = 0;
    return AVD_OK;
}

// The checks of a slot call, in the order include/avd.h lists them, all before anything is staged and with the slot untouched; then the call.
static int slot_audio_features(avd_ctx* ctx, const void* wav, int mem, int64_t n, int win, avd_audio_window* windows, int max_windows, int ncuts, bool last)
{
    AudioSlot& slot = ctx->audio_slots[ctx->audio_slot - 1];
    const int format = ctx->audio_format, rate = ctx->audio_rate;
    AudioInput in = audio_input(ctx, n);
    const int channels = in.channels;
    if (audio_stride_refused(ctx, in, n)) return AVD_ERR_ARG;
    if (ncuts > 0) { ctx->err = "audio_slot: one track per call (an \"audio_cut\" list was pending; it is gone)"; return AVD_ERR_ARG; }
    if (slot.frames > 0 && (slot.win != win || slot.rate != rate || slot.channels != channels || slot.format != format || slot.layout != in.layout)) {
        ctx->err = "audio_slot: win, \"audio_rate\", \"audio_channels\" and \"audio_format\" must be those of the slot's first call";
        return AVD_ERR_ARG;
    }
    avd_resample::Ratio ratio = avd_resample::identity_ratio();
    if (rate != 0 && !avd_resample::ratio_of(rate, ratio)) { ctx->err = "audio_rate: not a supported rate"; return AVD_ERR_ARG; }   // (the option refuses such a value)
    const avd_resample::Continue c = avd_resample::plan_continue(slot.frames, n, last, ratio, win);
    if (c.refused) { ctx->err = "audio_slot: more than 2^31 - 1 output samples in the track"; return AVD_ERR_ARG; }
    if (c.windows > max_windows || (c.windows > 0 && !windows)) { ctx->err = "audio_slot: windows array too small"; return AVD_ERR_ARG; }
    if (n == 0 && !last) {                                   // nothing to absorb, nothing to flush: the call wrote no record
        if (slot.frames > 0) slot.windows = 0;
        return AVD_OK;
    }
    bool saved = false;
    const int e = run_audio_slot(ctx, slot, c, ratio, wav, mem, n, win, windows, max_windows, last, &saved, in);
    if (e) {
        if (saved) { slot.clear(); ctx->err += " (audio_slot: the failure came after the slot's save launch; the slot was emptied)"; }
        return e;
    }
    if (last) { slot.clear(); return AVD_OK; }
    if (slot.frames == 0) { slot.win = win; slot.rate = rate; slot.channels = channels; slot.format = format; slot.layout = in.layout; }
    slot.frames = c.n_after;
    slot.held = c.held_after;
    slot.windows = (int)c.windows;
    slot.hist_side ^= 1;
    return AVD_OK;
}

// A call with an "audio_track_slot" list: several tracks, each a whole one or the continuation of an audio slot (avd_audio_map.h plans it;
// include/avd.h states it).  The analyzer's buffer is ws.d_audio_pcm, a region [held | new] per track.  At most ONE launch of each kind, however
// many tracks: the gather (held samples, and an unconverted call's own, into the regions), the converter (per-track sources), the analyzer's
// passes over one window table, the save (every continued track that does not end).  Every slot's memory is reserved before the first launch, the
// save is the last launch, and the host state of the slots moves only once the call has drained.  *saved as in run_audio_slot.
static int run_audio_map(avd_ctx* ctx, avd_audio_map::Plan& plan, const avd_resample::Ratio& ratio, const void* wav, int mem, int64_t n, avd_audio_window* windows,
                         bool* saved, AudioInput& in)
{
    const int format = ctx->audio_format, channels = in.channels;
    const bool converted = ratio.rate != 0;
    const size_t in_size = format == 1 ? sizeof(int16_t) : sizeof(float), an_size = converted ? sizeof(int16_t) : in_size;
    const int an_format = converted ? 1 : format, nwin = plan.windows.nwin();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Workspace& ws = ctx->ws;
    for (const avd_audio_map::Track& tr : plan.tracks)
        if (tr.slot)
            if (int e = ctx->audio_slots[tr.slot - 1].d_mem.reserve(ctx, kAudioSlotWords)) return e;
    if (int e = ws.d_audio_pcm.reserve(ctx, (size_t)plan.total * an_size / sizeof(int16_t) + 8)) return e;
    if (int e = ws.d_audio_out.reserve(ctx, (size_t)std::max(nwin, 1))) return e;
    char* buf = reinterpret_cast<char*>(ws.d_audio_pcm.p);
    const uint8_t* d_in = reinterpret_cast<const uint8_t*>(buf);                   // n = 0: a valid address nobody reads
    ctx->audio_rs_valid = 0;
    int* call = ctx->audio_map_call;
    ctx->audio_map_valid = 0;
    call[0] = (int)plan.tracks.size(); call[1] = plan.continued; call[2] = call[3] = call[4] = call[5] = 0;
    if (n > 0)
        if (int e = stage_audio(ctx, wav, mem, n, in_size, in, &d_in)) return e;
    if (!plan.gather.empty()) {
        AudioGatherMove moves[avd_audio_map::kMaxGather];
        int count = 0;
        for (const avd_audio_map::Copy& c : plan.gather) {
            const void* from = c.held ? static_cast<const void*>(ctx->audio_slots[plan.tracks[(size_t)c.track].slot - 1].held_at())
                                      : static_cast<const void*>(d_in + (size_t)c.src * in_size);
            moves[count++] = AudioGatherMove{from, buf + (size_t)c.dst * an_size, (long long)((size_t)c.count * an_size)};
        }
        if (int e = launch_audio_gather(ctx, moves, count, (int)an_size)) return e;
        call[2] = 1;
    }
    if (converted) {
        for (size_t t = 0; t < plan.tracks.size(); t++)
            if (const int k = plan.sources[t].slot) plan.sources[t].hist = reinterpret_cast<unsigned long long>(ctx->audio_slots[k - 1].hist(ctx->audio_slots[k - 1].hist_side));
        bool launched = false;
        if (int e = launch_audio_resample_map(ctx, d_in, format, channels, plan, ratio, n, ws.d_audio_pcm, &launched, in.mix)) return e;
        record_audio_layout(ctx, in);
        call[3] = launched;
    }
    if (nwin > 0) {
        if (int e = launch_audio_features(ctx, buf, an_format, plan.windows, ws.d_audio_out)) return e;
        HIP_TRY(ctx, hipMemcpyAsync(windows, ws.d_audio_out, sizeof(avd_audio_window) * nwin, hipMemcpyDeviceToHost, ctx->stream));
        call[4] = 1;
    }
    if (!plan.saves.empty()) {
        AudioSaveRow rows[avd_audio_map::kSlots];
        int count = 0;
        for (const avd_audio_map::Save& s : plan.saves) {
            AudioSlot& slot = ctx->audio_slots[s.slot - 1];
            const avd_audio_map::Track& tr = plan.tracks[(size_t)s.track];
            AudioSaveRow r = {};
            r.wav = converted ? d_in + (size_t)tr.begin * (size_t)in.step * in_size : d_in;
            r.n = s.n;
            r.hist_old = slot.hist(slot.hist_side); r.hist_old_n = s.hist_old;
            r.hist_new = slot.hist(slot.hist_side ^ 1); r.hist_new_n = s.hist_new;
            r.held_src = reinterpret_cast<const int16_t*>(buf + (size_t)s.held_src * an_size);
            r.held_dst = slot.held_at();
            r.held_words = (int)((size_t)s.held * an_size / sizeof(int16_t));
            rows[count++] = r;
        }
        if (int e = launch_audio_slot_save_map(ctx, converted ? format : 1, channels, rows, count, saved, in.mix)) return e;
        call[5] = 1;
    }
    ctx->audio_map_valid = 1;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ws.audio_upload_pending = 0;
    ws.audio_rs_upload_pending = 0;
    return AVD_OK;
}

// The checks of a list call, in the order include/avd.h lists them, all before anything is staged and with every slot untouched; then the call.
// entries / nentries: the "audio_track_slot" list the call took from the context.
static int map_audio_features(avd_ctx* ctx, const void* wav, int mem, int64_t n, int win, avd_audio_window* windows, int max_windows, const int* cuts, int ncuts,
                              const int* entries, int nentries, bool end_pending)
{
    const int format = ctx->audio_format, rate = ctx->audio_rate;
    AudioInput in = audio_input(ctx, n);
    const int channels = in.channels;
    if (n > 0 && format == 1 && (reinterpret_cast<uintptr_t>(wav) & 1)) { ctx->err = "audio_format 1: int16 samples need a 2-byte aligned wav"; return AVD_ERR_ARG; }
    if (n > 0 && format == 0 && (reinterpret_cast<uintptr_t>(wav) & 3)) { ctx->err = "audio_track_slot: float32 samples need a 4-byte aligned wav"; return AVD_ERR_ARG; }
    if (audio_stride_refused(ctx, in, n)) return AVD_ERR_ARG;
    avd_resample::Ratio ratio = avd_resample::identity_ratio();
    if (rate != 0 && !avd_resample::ratio_of(rate, ratio)) { ctx->err = "audio_rate: not a supported rate"; return AVD_ERR_ARG; }   // (the option refuses such a value)
    avd_audio_map::SlotState state[kAudioSlots];
    for (int k = 0; k < kAudioSlots; k++) {
        const AudioSlot& s = ctx->audio_slots[k];
        state[k].frames = s.frames;
        state[k].held = s.held;
        state[k].hist = avd_resample::history_frames(s.frames, ratio);
        state[k].same = s.win == win && s.rate == rate && s.channels == channels && s.format == format && s.layout == in.layout;
    }
    avd_audio_map::Plan plan = avd_audio_map::plan_map(n, win, cuts, ncuts, entries, nentries, state, ratio, in.step, max_windows, windows != nullptr, end_pending);
    switch (plan.refused) {
    case avd_audio_map::kOk: break;
    case avd_audio_map::kCutBeyond: ctx->err = "audio_cut: beyond the buffer"; return AVD_ERR_ARG;
    case avd_audio_map::kEndPending: ctx->err = "audio_track_slot: ends are given in the list (an \"audio_end\" was pending; it and the list are gone)"; return AVD_ERR_ARG;
    case avd_audio_map::kEntryCount: ctx->err = "audio_track_slot: the list needs one entry per track of the call (the \"audio_cut\" list's cuts + 1)"; return AVD_ERR_ARG;
    case avd_audio_map::kSlotBinding:
        ctx->err = "audio_track_slot: win, \"audio_rate\", \"audio_channels\" and \"audio_format\" must be those of the slot's first call (track " + std::to_string(plan.refused_track) + ")";
        return AVD_ERR_ARG;
    case avd_audio_map::kTooLong:
        ctx->err = plan.refused_track < 0 ? std::string("audio_track_slot: more than 2^31 - 1 samples in the analyzer's buffer of all tracks together")
                                          : "audio_track_slot: more than 2^31 - 1 output samples in a track (track " + std::to_string(plan.refused_track) + ")";
        return AVD_ERR_ARG;
    case avd_audio_map::kWindowsTooSmall: ctx->err = "audio_track_slot: windows array too small"; return AVD_ERR_ARG;
    case avd_audio_map::kTooManyWindows: ctx->err = "audio_track_slot: more than 2^24 records in one call"; return AVD_ERR_ARG;
    default: ctx->err = "audio_track_slot: internal error (a slot's state contradicts the rule)"; return AVD_ERR_DEVICE;
    }
    bool saved = false;
    const int e = run_audio_map(ctx, plan, ratio, wav, mem, n, windows, &saved, in);
    if (e) {
        if (saved) {
            for (const avd_audio_map::Track& tr : plan.tracks)
                if (tr.slot) ctx->audio_slots[tr.slot - 1].clear();
            ctx->err += " (audio_track_slot: the failure came after the save launch; every slot the call continued was emptied)";
        }
        return e;
    }
    for (const avd_audio_map::Track& tr : plan.tracks) {
        if (!tr.slot) continue;
        AudioSlot& slot = ctx->audio_slots[tr.slot - 1];
        if (tr.last) { slot.clear(); continue; }
        if (slot.frames == 0) { slot.win = win; slot.rate = rate; slot.channels = channels; slot.format = format; slot.layout = in.layout; }
        slot.frames = tr.c.n_after;
        slot.held = tr.c.held_after;
        slot.windows = tr.count;
        slot.hist_side ^= 1;
    }
    return AVD_OK;
}

// cuts / ncuts: the "audio_cut" list the call took from the context (avd_audio_features: one-shot, whatever becomes of the call); last: "audio_end" likewise;
// entries / nentries: the "audio_track_slot" list likewise
static int impl_audio_features(avd_ctx* ctx, const void* wav, int mem, int64_t n, int win, avd_audio_window* windows, int max_windows, const int* cuts, int ncuts,
                               bool last, const int* entries, int nentries)
{
    if (win < 1 || win > 8192) { ctx->err = "audio window must be 1..8192 samples"; return AVD_ERR_ARG; }   // also for n = 0: a bad window is never "nothing to do"
    // a slot call that completes no window needs no windows array (slot_audio_features asks for one only where records are written); a list call likewise
    if (n < 0 || (n > 0 && (!wav || (!windows && ctx->audio_slot == 0 && nentries == 0)))) { ctx->err = "bad arguments"; return AVD_ERR_ARG; }
    if (nentries > 0) {                                      // (the option keeps "audio_slot" at 0 while a list is held)
        if (mem != AVD_MEM_HOST && mem != AVD_MEM_DEVICE) { ctx->err = "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"; return AVD_ERR_ARG; }
        return map_audio_features(ctx, wav, mem, n, win, windows, max_windows, cuts, ncuts, entries, nentries, last);
    }
    if (ctx->audio_slot != 0) {
        if (n > 0 && ctx->audio_format == 1 && (reinterpret_cast<uintptr_t>(wav) & 1)) { ctx->err = "audio_format 1: int16 samples need a 2-byte aligned wav"; return AVD_ERR_ARG; }
        if (n > 0 && ctx->audio_format == 0 && (reinterpret_cast<uintptr_t>(wav) & 3)) { ctx->err = "audio_slot: float32 samples need a 4-byte aligned wav"; return AVD_ERR_ARG; }
        if (mem != AVD_MEM_HOST && mem != AVD_MEM_DEVICE) { ctx->err = "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"; return AVD_ERR_ARG; }
        return slot_audio_features(ctx, wav, mem, n, win, windows, max_windows, ncuts, last);
    }
    if (n == 0) return AVD_OK;
    const int format = ctx->audio_format;
    if (format == 1 && (reinterpret_cast<uintptr_t>(wav) & 1)) { ctx->err = "audio_format 1: int16 samples need a 2-byte aligned wav"; return AVD_ERR_ARG; }
    if (ctx->audio_rate != 0) return convert_audio_features(ctx, wav, mem, n, win, windows, max_windows, cuts, ncuts);
    const avd_audio::Plan plan = avd_audio::plan_call(n, win, cuts, ncuts, max_windows);
    if (plan.refused == avd_audio::kCutBeyond) { ctx->err = "audio_cut: beyond the buffer"; return AVD_ERR_ARG; }
    if (plan.refused) { ctx->err = "windows array too small"; return AVD_ERR_ARG; }
    ctx->audio_rs_valid = 0;                                 // debug buffers "audio_rs_*" / "audio_pcm" describe the last call that ran, and only if it converted
    const int nwin = plan.nwin();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Workspace& ws = ctx->ws;
    const uint8_t* d_wav = nullptr;
    if (int e = stage_input(ctx, static_cast<const uint8_t*>(wav), mem, (size_t)n * (format == 1 ? sizeof(int16_t) : sizeof(float)), &d_wav)) return e;
    if (int e = ws.d_audio_out.reserve(ctx, (size_t)nwin)) return e;
    if (int e = launch_audio_features(ctx, d_wav, format, plan, ws.d_audio_out)) return e;
    HIP_TRY(ctx, hipMemcpyAsync(windows, ws.d_audio_out, sizeof(avd_audio_window) * nwin, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ws.audio_upload_pending = 0;
    return AVD_OK;
}

// An asynchronous call still pending on the context (records not handed over, or its last chunk's re-run not settled) is completed
// first: the workspace, the pinned records buffer and the options it was submitted with belong to it until then.  A failure of the
// pending call is returned instead of running the new one.
static int drain_pending(avd_ctx* ctx)
{
    if (!ctx->pending_out && !ctx->tail.active) return AVD_OK;
    return impl_synchronize(ctx);
}

// Pending::keep: the entry points that neither enqueue work, nor touch the workspace, nor change an option (avd_synchronize itself,
// avd_get_option, the timers and timings, avd_wait_stream); every other one drains.
enum class Pending { drain, keep };

// Nothing may propagate across the C boundary: std::vector / std::string members of the context and the table
// builders can throw std::bad_alloc (or length_error), so every entry point runs inside this guard.
template <typename F>
static int guarded(avd_ctx* ctx, F&& f, Pending pending = Pending::drain) noexcept
{
    try {
        if (!ctx) return f();
        std::lock_guard<std::recursive_mutex> lk(ctx->api_mu);     // one call at a time per context; helpers of other contexts only try_lock (tail_help_others)
        if (pending == Pending::drain)
            if (int e = drain_pending(ctx)) return e;
        return f();
    } catch (const std::bad_alloc&) {
        if (ctx) { try { ctx->err = "out of host memory"; } catch (...) {} }
        return AVD_ERR_NOMEM;
    } catch (...) {
        if (ctx) { try { ctx->err = "unexpected C++ exception"; } catch (...) {} }
        return AVD_ERR_DEVICE;
    }
}

// Every avd_analyze_* entry point is ONE guarded call: the asynchronous body and, in the blocking variants, the drain behind it.
enum class Wait { no, yes };
template <typename F>
static int analyze_entry(avd_ctx* ctx, Wait wait, F&& enqueue) noexcept
{
    return guarded(ctx, [&] {
        const int rc = enqueue();
        return rc || wait == Wait::no ? rc : impl_synchronize(ctx);
    });
}
static int analyze_clip(avd_ctx* ctx, const IngestClip& k, avd_frame_record* records, Wait wait) noexcept
{
    return analyze_entry(ctx, wait, [&] { return impl_analyze_async(ctx, &k, 1, records); });
}
static int analyze_clips(avd_ctx* ctx, const avd_clip* clips, int nclips, avd_frame_record* records, Wait wait) noexcept
{
    return analyze_entry(ctx, wait, [&] { return impl_analyze_list_async(ctx, clips, nclips, records, clip_from_public); });
}
static int analyze_pictures(avd_ctx* ctx, const avd_picture* clips, int nclips, avd_frame_record* records, Wait wait) noexcept
{
    return analyze_entry(ctx, wait, [&] { return impl_analyze_list_async(ctx, clips, nclips, records, from_picture); });
}
static int analyze_frame_lists(avd_ctx* ctx, const avd_frame_list* lists, int nlists, avd_frame_record* records, Wait wait) noexcept
{
    return analyze_entry(ctx, wait, [&] { return impl_analyze_list_async(ctx, lists, nlists, records, from_frame_list); });
}

// ---- C-ABI ------------------------------------------------------------------------------
extern "C" {

int avd_abi_version(void) { return AVD_ABI_VERSION; }

const char* avd_last_error(const avd_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int avd_create(int device_id, avd_ctx** out)
{
    return guarded(nullptr, [&] { return impl_create(device_id, out); });
}

void avd_destroy(avd_ctx* ctx)
{
    (void)guarded(nullptr, [&] { impl_destroy(ctx); return 0; });
}

int avd_preprocess_bgr(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride,
                       int64_t frame_stride, uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq)
{
    const IngestClip k = bgr_clip(bgr, mem, n, h, w, row_stride, frame_stride);
    return guarded(ctx, [&] { return impl_preprocess(ctx, k, small320, hash1024, lap_sum, lap_sumsq); });
}

int avd_farneback_pairs(avd_ctx* ctx, const uint8_t* small320, int mem, int n, float* flow_mean, float* flow_var, float* flow_out)
{
    return guarded(ctx, [&] { return impl_farneback_pairs(ctx, small320, mem, n, flow_mean, flow_var, flow_out); });
}

int avd_analyze_frames_async(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride,
                             int64_t frame_stride, avd_frame_record* records)
{
    return analyze_clip(ctx, bgr_clip(bgr, mem, n, h, w, row_stride, frame_stride), records, Wait::no);
}

int avd_synchronize(avd_ctx* ctx) { return guarded(ctx, [&] { return impl_synchronize(ctx); }, Pending::keep); }

int avd_analyze_batch_async(avd_ctx* ctx, const avd_clip* clips, int nclips, avd_frame_record* records)
{
    return analyze_clips(ctx, clips, nclips, records, Wait::no);
}

int avd_analyze_batch(avd_ctx* ctx, const avd_clip* clips, int nclips, avd_frame_record* records)
{
    return analyze_clips(ctx, clips, nclips, records, Wait::yes);
}

int avd_preprocess_picture(avd_ctx* ctx, const avd_picture* picture, uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq)
{
    return guarded(ctx, [&] { return impl_preprocess_one_picture(ctx, picture, small320, hash1024, lap_sum, lap_sumsq); });
}

int avd_analyze_pictures_async(avd_ctx* ctx, const avd_picture* clips, int nclips, avd_frame_record* records)
{
    return analyze_pictures(ctx, clips, nclips, records, Wait::no);
}

int avd_analyze_pictures(avd_ctx* ctx, const avd_picture* clips, int nclips, avd_frame_record* records)
{
    return analyze_pictures(ctx, clips, nclips, records, Wait::yes);
}

int avd_preprocess_frame_list(avd_ctx* ctx, const avd_frame_list* list, uint8_t* small320, uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq)
{
    return guarded(ctx, [&] { return impl_preprocess_one_list(ctx, list, small320, hash1024, lap_sum, lap_sumsq); });
}

int avd_analyze_frame_lists_async(avd_ctx* ctx, const avd_frame_list* lists, int nlists, avd_frame_record* records)
{
    return analyze_frame_lists(ctx, lists, nlists, records, Wait::no);
}

int avd_analyze_frame_lists(avd_ctx* ctx, const avd_frame_list* lists, int nlists, avd_frame_record* records)
{
    return analyze_frame_lists(ctx, lists, nlists, records, Wait::yes);
}

int avd_preprocess_nv12(avd_ctx* ctx, const uint8_t* y, const uint8_t* uv, int mem, int n, int h, int w, int64_t y_row_stride,
                        int64_t uv_row_stride, int64_t y_frame_stride, int64_t uv_frame_stride, uint8_t* small320,
                        uint8_t* hash1024, int64_t* lap_sum, int64_t* lap_sumsq)
{
    const IngestClip k = nv12_clip(y, uv, mem, n, h, w, y_row_stride, uv_row_stride, y_frame_stride, uv_frame_stride);
    return guarded(ctx, [&] { return impl_preprocess(ctx, k, small320, hash1024, lap_sum, lap_sumsq); });
}

int avd_analyze_frames_nv12_async(avd_ctx* ctx, const uint8_t* y, const uint8_t* uv, int mem, int n, int h, int w,
                                  int64_t y_row_stride, int64_t uv_row_stride, int64_t y_frame_stride,
                                  int64_t uv_frame_stride, avd_frame_record* records)
{
    const IngestClip k = nv12_clip(y, uv, mem, n, h, w, y_row_stride, uv_row_stride, y_frame_stride, uv_frame_stride);
    return analyze_clip(ctx, k, records, Wait::no);
}

int avd_analyze_frames_nv12(avd_ctx* ctx, const uint8_t* y, const uint8_t* uv, int mem, int n, int h, int w,
                            int64_t y_row_stride, int64_t uv_row_stride, int64_t y_frame_stride, int64_t uv_frame_stride,
                            avd_frame_record* records)
{
    const IngestClip k = nv12_clip(y, uv, mem, n, h, w, y_row_stride, uv_row_stride, y_frame_stride, uv_frame_stride);
    return analyze_clip(ctx, k, records, Wait::yes);
}

int avd_preprocess_i420(avd_ctx* ctx, const uint8_t* y, const uint8_t* u, const uint8_t* v, int mem, int n, int h, int w, int64_t y_row_stride,
                        int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride, uint8_t* small320, uint8_t* hash1024,
                        int64_t* lap_sum, int64_t* lap_sumsq)
{
    const IngestClip k = i420_clip(y, u, v, mem, n, h, w, y_row_stride, c_row_stride, y_frame_stride, c_frame_stride);
    return guarded(ctx, [&] { return impl_preprocess(ctx, k, small320, hash1024, lap_sum, lap_sumsq); });
}

int avd_analyze_frames_i420_async(avd_ctx* ctx, const uint8_t* y, const uint8_t* u, const uint8_t* v, int mem, int n, int h, int w,
                                  int64_t y_row_stride, int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride,
                                  avd_frame_record* records)
{
    const IngestClip k = i420_clip(y, u, v, mem, n, h, w, y_row_stride, c_row_stride, y_frame_stride, c_frame_stride);
    return analyze_clip(ctx, k, records, Wait::no);
}

int avd_analyze_frames_i420(avd_ctx* ctx, const uint8_t* y, const uint8_t* u, const uint8_t* v, int mem, int n, int h, int w,
                            int64_t y_row_stride, int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride,
                            avd_frame_record* records)
{
    const IngestClip k = i420_clip(y, u, v, mem, n, h, w, y_row_stride, c_row_stride, y_frame_stride, c_frame_stride);
    return analyze_clip(ctx, k, records, Wait::yes);
}

int avd_analyze_frames(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride,
                       int64_t frame_stride, avd_frame_record* records)
{
    return analyze_clip(ctx, bgr_clip(bgr, mem, n, h, w, row_stride, frame_stride), records, Wait::yes);
}

int avd_cnn_param_counts(size_t* n_weights, size_t* n_biases)
{
    if (!n_weights || !n_biases) return AVD_ERR_ARG;
    cnn_param_counts(n_weights, n_biases);
    return AVD_OK;
}

int avd_cnn_set_weights(avd_ctx* ctx, const uint16_t* weights_bf16, size_t n_weights, const float* biases, size_t n_biases)
{
    return guarded(ctx, [&] { return impl_cnn_set_weights(ctx, weights_bf16, n_weights, biases, n_biases); });
}

int avd_cnn_forward(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride, int64_t frame_stride,
                    float* logits, int timing_reps, float* forward_ms)
{
    return guarded(ctx, [&] { return impl_cnn_forward(ctx, bgr, mem, n, h, w, row_stride, frame_stride, logits, timing_reps, forward_ms); });
}

int avd_cnn_conv(avd_ctx* ctx, const uint16_t* x, int n, int hin, int win, int cin, const uint16_t* w, const float* bias,
                 int cout, int ksize, int stride, int relu, const uint16_t* residual, uint16_t* y)
{
    return guarded(ctx, [&] {
        if (!ctx || !x || !w || !bias || !y) return (int)AVD_ERR_ARG;
        if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return (int)AVD_ERR_DEVICE; }
        return cnn_conv_host(ctx, x, n, hin, win, cin, w, bias, cout, ksize, stride, relu, residual, y);
    });
}

int avd_vit_set_weights(avd_ctx* ctx, const uint16_t* weight_bf16, const float* bias)
{
    return guarded(ctx, [&] { return impl_vit_set_weights(ctx, weight_bf16, bias); });
}

int avd_vit_patch_embed(avd_ctx* ctx, const uint8_t* bgr, int mem, int n, int h, int w, int64_t row_stride, int64_t frame_stride,
                        void* tokens, int tokens_mem, int tokens_bf16, int timing_reps, float* gemm_ms)
{
    return guarded(ctx, [&] { return impl_vit_patch_embed(ctx, bgr, mem, n, h, w, row_stride, frame_stride, tokens, tokens_mem, tokens_bf16, timing_reps, gemm_ms); });
}

int avd_layernorm(avd_ctx* ctx, const void* x, int mem, int bf16, int64_t rows, int cols, const float* gamma, const float* beta, float eps,
                  void* y, int timing_reps, float* ms)
{
    return guarded(ctx, [&] { return impl_rowop(ctx, 0, x, mem, bf16, rows, cols, gamma, beta, eps, y, timing_reps, ms); });
}

int avd_softmax(avd_ctx* ctx, const float* x, int mem, int64_t rows, int cols, float* y, int timing_reps, float* ms)
{
    return guarded(ctx, [&] { return impl_rowop(ctx, 1, x, mem, 0, rows, cols, nullptr, nullptr, 0.f, y, timing_reps, ms); });
}

int avd_audio_features(avd_ctx* ctx, const float* wav, int mem, int64_t n, int win, avd_audio_window* windows, int max_windows)
{
    if (!ctx) return AVD_ERR_ARG;
    // The "audio_cut" list is taken FIRST, ahead of the drain of a pending call: it is gone whether this call succeeds, is refused or fails
    return guarded(ctx, [&] {
        int cuts[avd_audio::kMaxCuts];
        const int ncuts = ctx->audio_ncuts;
        std::copy(ctx->audio_cuts, ctx->audio_cuts + ncuts, cuts);
        ctx->audio_ncuts = 0;
        const bool last = ctx->audio_end != 0;               // "audio_end" goes the same way
        ctx->audio_end = 0;
        int entries[avd_audio_map::kMaxEntries];             // ... and the "audio_track_slot" list
        const int nentries = ctx->audio_map_n;
        std::copy(ctx->audio_map_entries, ctx->audio_map_entries + nentries, entries);
        ctx->audio_map_n = 0;
        if (int e = drain_pending(ctx)) return e;
        return impl_audio_features(ctx, wav, mem, n, win, windows, max_windows, cuts, ncuts, last, entries, nentries);
    }, Pending::keep);
}

int avd_comm_unique_id(void* id128)
{
    if (!id128) return AVD_ERR_ARG;
    return guarded(nullptr, [&] { std::string err; return comm_unique_id(err, id128); });
}
int avd_comm_init(avd_ctx* ctx, int rank, int world, const void* id128)
{
    if (!ctx) return AVD_ERR_ARG;
    return guarded(ctx, [&] { return comm_init(ctx, rank, world, id128); });
}
int avd_allgather_records(avd_ctx* ctx, const avd_frame_record* local, int count, avd_frame_record* all)
{
    if (!ctx) return AVD_ERR_ARG;
    return guarded(ctx, [&] { return comm_allgather_records(ctx, local, count, all); });
}

int avd_allgather_last_records(avd_ctx* ctx, int count, avd_frame_record* all)
{
    if (!ctx) return AVD_ERR_ARG;
    // guarded drains a pending asynchronous call FIRST: the exact re-run of the pairs its fast level kernels flagged happens there, and the
    // records on the device are final only after it
    return guarded(ctx, [&] { return comm_allgather_last_records(ctx, count, all); });
}

int avd_wait_stream(avd_ctx* ctx, void* producer_stream) { return guarded(ctx, [&] { return impl_wait_stream(ctx, producer_stream); }, Pending::keep); }
int avd_release_workspace(avd_ctx* ctx) { return guarded(ctx, [&] { return impl_release_workspace(ctx); }); }
int avd_timer_start(avd_ctx* ctx) { return guarded(ctx, [&] { return impl_timer_start(ctx); }, Pending::keep); }
int avd_timer_stop(avd_ctx* ctx, float* elapsed_ms) { return guarded(ctx, [&] { return impl_timer_stop(ctx, elapsed_ms); }, Pending::keep); }
int avd_set_option(avd_ctx* ctx, const char* name, int value) { return guarded(ctx, [&] { return impl_set_option(ctx, name, value); }); }
int avd_get_option(avd_ctx* ctx, const char* name, int* value) { return guarded(ctx, [&] { return impl_get_option(ctx, name, value); }, Pending::keep); }
int avd_set_profiling(avd_ctx* ctx, int enable) { return guarded(ctx, [&] { return impl_set_profiling(ctx, enable); }); }
int avd_stage_ms(avd_ctx* ctx, int stage, float* ms) { return guarded(ctx, [&] { return impl_stage_ms(ctx, stage, ms); }, Pending::keep); }
int avd_kernel_ms(avd_ctx* ctx, int kernel_id, float* ms) { return guarded(ctx, [&] { return impl_kernel_ms(ctx, kernel_id, ms); }, Pending::keep); }

int64_t avd_debug_fetch(avd_ctx* ctx, const char* name, void* out, size_t out_bytes)
{
    int64_t got = AVD_ERR_DEVICE;
    const int rc = guarded(ctx, [&] { got = impl_debug_fetch(ctx, name, out, out_bytes); return 0; });
    return rc ? rc : got;
}

}  // extern "C"
