// Short-time spectral ridge (gfx950): per short frame the spectral peak, its bin, the power outside a guard band around
// it and the frame's total power -- gj_ridge_dev / gj_ridge_frames of include/gpsjam.h, which states the definition.
// The time series tells the four interferers of the reference's simulator apart (simulate/frontend/jammers/:
// cwJammer.py, chirpJammer.py, pulsedJammer.py, broadbandJammer.py; gpsjam/classify.py reads it).
//
// The transform front end -- the workgroup of transform groups, the loads, the window, the passes and their exchange
// barrier, the group reductions -- is stft_group.h, shared with k_excise.hip and k_skurt.hip; the frame walk and the host
// side of a call over n_frames frames are stft_frames.h, shared with k_chirp.hip.  What is the ridge's own:
//   * a frame starts at first_sample + f * hop, any hop: a frame is only 2-byte aligned and has no fixed relation to
//     its neighbours, so nothing is carried from step to step and every address is a 64-bit frame base + constants;
//   * no mean removal (pulsedJammer.py's carrier sits at 0 Hz) and no PSD scaling: P[k] = |X[k]|^2 in sample units;
//   * instead of accumulating spectra, the N/16 threads of a transform group reduce their bins to one 16-byte record:
//     sum, max with the smallest index that attains it, then the max outside the guard band once the peak bin is known.
//     N <= 1024: the group lies inside one wave (DPP row operations, two cross-row shuffles); 2048 and 4096: wave
//     results meet in LDS and are combined in wave order.
// Determinism: a frame's record is computed by ONE transform group from that frame's bytes alone, every sum runs in an
// order fixed by N (16 bins per thread in slot order, then the lane tree, then the waves in order), and float add / max
// are commutative, so every lane of a group holds the same bits whichever group, workgroup or launch computes the frame.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it
// (tests/hip_stub builds those by name), and K2's module is compiled exactly as before.
#include "stft_frames.h"

namespace gj {

template <int N>
struct RidgeCfg {
    // as K2 (WelchCfg): three workgroups per CU from 32 points on, one LDS buffer with two syncs per exchange
    static constexpr int min_waves = N >= 32 ? 3 : 2;
    static constexpr bool xpose = N == 4096;       // the conflict-free exchange schedule of fft_core.h (X4096)
    static constexpr bool wide_load = N <= 32;     // 16-byte loads of the whole frame (stft_load_frame)
};

struct RidgeGeom {
    unsigned long long first_sample, hop, n_frames, nsteps;
    float neg_off;   // -offset of the unpack convention
    float scale2;    // scale^2: the transform runs on u8 - offset, the three powers are scaled at the end
    int guard;
};

template <int N>
__global__ __launch_bounds__(kBlockThreads, RidgeCfg<N>::min_waves) void ridge_kernel(const uint8_t* __restrict__ iq, RidgeGeom g,
                                                                                      const cf* __restrict__ twtab,
                                                                                      const float* __restrict__ wintab,
                                                                                      gj_ridge_frame* __restrict__ out) {
    using Cfg = RidgeCfg<N>;
    using S = StftShape<N>;
    constexpr int TF = S::TF, B = S::B, NP = S::NP, WPF = S::WPF;
    constexpr bool XP = Cfg::xpose;
    constexpr int SPAN = XP ? X4096::kSpan : lds_span(kBlockPoints);
    __shared__ cf lds0[NP > 1 ? SPAN : 1];
    // wave results of a transform group that spans waves (2048, 4096 points); one array per reduction, so that a wave
    // that is ahead never overwrites what a slower one still reads (the next step's writes lie behind the exchange
    // barriers of its transform)
    constexpr int RB = WPF > 1 ? B : 1;
    __shared__ float red_sum[RB][WPF], red_max[RB][WPF], red_sec[RB][WPF];
    __shared__ int red_bin[RB][WPF];
    const int tid = threadIdx.x;
    const StftRoles role = stft_roles<N, XP>(tid);
    const int b = role.b, jl0 = role.jl0, jl = role.jl;

    const InnerTw ktw = inner_twiddles();
    c2 tw[3][15], wp[8];
    stft_load_twiddles<N>(tw, twtab, jl);
#pragma unroll
    for (int s = 0; s < 8; ++s) wp[s] = stft_window_pair<N>(wintab, jl0, s);
    const c2 koff = make_c2(g.neg_off, g.neg_off);

    auto load_frame = [&](unsigned (&dst)[16], unsigned long long step) {
        stft_load_frame<N, Cfg::wide_load>(dst, frame_base(iq, g, step * B + (unsigned)b), jl0);
    };

    unsigned raw[16];   // the NEXT step's samples are fetched while the current ones are transformed
    unsigned long long step = blockIdx.x;   // the grid never exceeds nsteps
    load_frame(raw, step);
    for (; step < g.nsteps; step += gridDim.x) {
        const unsigned long long f = step * B + (unsigned)b;
        const bool active = f <= g.n_frames - 1;
        c2 v[16];
        stft_unpack_window(v, raw, wp, koff);
        if (step + gridDim.x < g.nsteps) load_frame(raw, step + gridDim.x);   // workgroup-uniform

        if constexpr (XP) stft_passes_x4096(v, lds0, tid, tw, ktw);
        else stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

        // this thread's bins jl + TF s, ascending in s
        float p[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) p[s] = fmaf(v[s].x, v[s].x, v[s].y * v[s].y);
        float tot = p[0], mx = p[0];
        int ms = 0;
#pragma unroll
        for (int s = 1; s < 16; ++s) {
            tot += p[s];
            if (p[s] > mx) { mx = p[s]; ms = s; }   // strictly greater: the smallest slot among equals
        }
        constexpr int G = S::G;
        const auto add = [](float a, float c) { return a + c; };
        const auto fmx = [](float a, float c) { return fmaxf(a, c); };
        tot = group_reduce_f<G>(tot, add);
        float gmx = group_reduce_f<G>(mx, fmx);
        if constexpr (WPF > 1) {
            waves_post(red_sum[b], tid, tot);
            waves_post(red_max[b], tid, gmx);
            __syncthreads();
            tot = waves_fold(red_sum[b], add);
            gmx = waves_fold(red_max[b], fmx);
        }
        // smallest bin that attains the maximum: within a thread it is the thread's first such slot
        int bin = group_min_i<G>(mx == gmx ? jl + TF * ms : INT_MAX);
        if constexpr (WPF > 1) {
            waves_post(red_bin[b], tid, bin);
            __syncthreads();
            bin = waves_fold(red_bin[b], [](int a, int c) { return min(a, c); });
        }
        // largest value outside the guard band (circular distance to the peak bin > guard); powers are >= 0
        float sec = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int d = (jl + TF * s - bin) & (N - 1);
            if (min(d, N - d) > g.guard) sec = fmaxf(sec, p[s]);
        }
        sec = group_reduce_f<G>(sec, fmx);
        if constexpr (WPF > 1) {
            waves_post(red_sec[b], tid, sec);
            __syncthreads();
            sec = waves_fold(red_sec[b], fmx);
        }
        if (active && jl0 == 0) {   // one lane per transform group
            gj_ridge_frame r;
            r.total = tot * g.scale2;
            r.peak = gmx * g.scale2;
            r.second = sec * g.scale2;
            r.peak_bin = bin;
            out[f] = r;
        }
    }
}

template <int N>
static void ridge_launch(gj_ctx* ctx, const uint8_t* d_iq, RidgeGeom g, gj_ridge_frame* d_out) {
    const unsigned grid = frames_one_round<N>(ctx, RidgeCfg<N>::min_waves, g);
    hipLaunchKernelGGL(ridge_kernel<N>, dim3(grid), dim3(kBlockThreads), 0, ctx->stream, d_iq, g, ctx->d_twiddle, window_table(ctx, N),
                       d_out);
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_ridge_frames(size_t nbytes, size_t first_sample, int nfft, size_t hop) {
    const size_t total = nbytes / 2;
    if (nfft < 1 || hop < 1 || first_sample > total || total - first_sample < (size_t)nfft) return 0;
    return (total - first_sample - (size_t)nfft) / hop + 1;
}

int gj_ridge_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, int nfft, size_t hop, size_t n_frames, int guard,
                 gj_ridge_frame* d_out) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (int rc = frames_check_buffers(ctx, d_iq, d_out)) return rc;
    if (int rc = frames_check_geometry(ctx, nbytes, first_sample, nfft, hop, n_frames, guard)) return rc;
    const RidgeGeom g = frames_geom<RidgeGeom>(ctx, first_sample, hop, n_frames, guard);
    stft_dispatch(nfft, [&](auto n) { ridge_launch<decltype(n)::value>(ctx, d_iq, g, d_out); });
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
