// Frequency-domain interference excision (gfx950): windowed 50 %-overlap FFT, per-bin threshold mask, inverse FFT and
// overlap-add back to uint8 I/Q -- gj_excise_dev / gj_excise_frames of include/gpsjam.h, which states the definition.
// The classical excisor of GPS receivers; simulate/frontend/jammers/ of the reference defines the interferers it has
// to remove.  The project's first kernel whose output is a capture.
//
// The transform front end -- the workgroup of transform groups, the loads, the window, the passes and their exchange
// barrier, the group reductions -- is stft_group.h, shared with k_ridge.hip and k_skurt.hip.  What is the excisor's own:
//   * frames hop by N / 2, and a transform group owns a RUN of consecutive frames that it walks in order.  After the
//     last pass a thread holds points jl + TF s (TF = N / 16); its slots s and s + 8 are N / 2 apart, so the
//     overlap-add is prev[s + 8] + cur[s] in registers and eight c2 are carried from frame to frame: no LDS, no atomics;
//   * a run is primed by transforming the frame in front of it once more (ExciseRun, excise_stages.h).  Run boundaries
//     come from the geometry alone (excise_launch);
//   * the inverse transform is the forward passes on the conjugate, IFFT(X) = conj(FFT(conj(X))) / N.  The output
//     pattern of the forward transform (jl + TF s) is the input pattern pass 0 wants, so the mask and the second
//     transform run on the registers as they are, with the same twiddle registers;
//   * 4096 points run the generic exchange schedule of fft_core.h, not X4096: X4096 changes the thread's role between
//     pass 0 and the end, which the register-to-register hand-over above does not survive without one more exchange;
//   * thr[jl + TF s] is constant per thread: 16 registers, loaded once;
//   * per frame the group reduces total, removed and the excised count to one 16-byte record with the DPP / LDS
//     pattern of ridge_kernel.
// Determinism: a frame's spectrum, mask and inverse are computed from that frame's bytes alone by the same
// instructions whichever group, run or launch computes it (the priming pass IS the loop body), every sum runs in an
// order fixed by N, and an output sample is prev + cur of its two frames: a call started k N / 2 samples later
// reproduces the interior bytes and the shared records bit for bit.
//
// The first half frame and the tail behind the last whole hop are copied from the input by a second small launch.
// That copy and the run arithmetic are excise_host.h, the stages behind the transform excise_stages.h; k_excise_chirp.hip
// and k_cancel.hip stand on both too.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it.
#include "excise_host.h"

namespace gj {

template <int N>
struct ExciseCfg {
    // ~160 live registers (32 data, 60 twiddles, 16 each for window, thresholds, carry and prefetch): two workgroups
    // per CU leave the compiler 256 VGPRs, three (168) would spill; the one- and two-pass sizes hold no second
    // twiddle set but keep the same bound (profiles/NOTES_excise.md has the compiler's figures)
    static constexpr int min_waves = 2;
    static constexpr int min_run = 4;   // frames per run at least (but for short calls): bounds the priming overhead at 25 %
};

template <int N>
__global__ __launch_bounds__(kBlockThreads, ExciseCfg<N>::min_waves) void excise_kernel(const uint8_t* __restrict__ iq, ExciseGeom g,
                                                                                        const cf* __restrict__ twtab,
                                                                                        const float* __restrict__ wintab,
                                                                                        const float* __restrict__ thr_tab,
                                                                                        uint8_t* __restrict__ out,
                                                                                        gj_excise_frame* __restrict__ frames) {
    using S = StftShape<N>;
    constexpr int TF = S::TF, B = S::B, NP = S::NP, WPF = S::WPF, H = N / 2;
    __shared__ cf lds0[NP > 1 ? lds_span(kBlockPoints) : 1];
    // wave results of a transform group that spans waves (2048, 4096 points), one array per reduction as in ridge_kernel
    constexpr int RB = WPF > 1 ? B : 1;
    __shared__ float red_tot[RB][WPF], red_rem[RB][WPF], red_cnt[RB][WPF];
    const int tid = threadIdx.x;
    const StftRoles role = stft_roles<N, false>(tid);
    const int b = role.b, jl = role.jl;   // input points, bins and output points of this thread: jl + TF s

    const InnerTw ktw = inner_twiddles();
    c2 tw[3][15], wp[8];
    stft_load_twiddles<N>(tw, twtab, jl);
#pragma unroll
    for (int s = 0; s < 8; ++s) wp[s] = stft_window_pair<N>(wintab, jl, s);
    float thr[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) thr[s] = thr_tab[jl + TF * s];
    const c2 koff = make_c2(-g.offset, -g.offset);

    const ExciseRun run(g, blockIdx.x, b, B);   // iteration 0 primes the carry with the frame in front of the run
    auto frame_base = [&](long long f) { return iq + 2ull * (g.first_sample + run.clamped(f) * H); };
    auto load_frame = [&](unsigned (&dst)[16], const uint8_t* base) { stft_load_frame<N, false>(dst, base, jl); };

    unsigned raw[16];   // the NEXT frame's samples are fetched while the current ones are transformed
    load_frame(raw, frame_base(run.first - 1));
    c2 carry[8];        // second half of the previous frame's inverse transform: y_{f-1}[jl + TF (s + 8)]
#pragma unroll
    for (int s = 0; s < 8; ++s) carry[s] = make_c2(0.f, 0.f);

    for (long long f = run.first - 1; f < run.end; ++f) {
        const bool owned = f >= run.first && f <= run.last;
        c2 v[16];
        stft_unpack_window(v, raw, wp, koff);
        if (f + 1 < run.end) load_frame(raw, frame_base(f + 1));   // workgroup-uniform

        stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

        // this thread's bins jl + TF s: power, mask, conjugate for the way back
        float tot = 0.f, rem = 0.f, cnt = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) excise_mask_bin(v[s], thr[s], g.scale2, tot, rem, cnt);
        const GroupSum<N> s_tot{tot, red_tot}, s_rem{rem, red_rem}, s_cnt{cnt, red_cnt};
        group_sums_post<N>(b, tid, s_tot, s_rem, s_cnt);
        if constexpr (WPF > 1) __syncthreads();
        group_sums_fold<N>(b, s_tot, s_rem, s_cnt);
        if (frames && owned && jl == 0) {   // one lane per transform group
            gj_excise_frame r;
            r.total = tot;
            r.removed = rem;
            r.n_excised = (int)cnt;
            r.reserved = 0;
            frames[f] = r;
        }

        stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

        const bool store = owned && f >= 1;
        uint8_t* dst = out + 2ull * ((unsigned long long)(f < 0 ? 0 : f) * H) + 2 * jl;
#pragma unroll
        for (int s = 0; s < 8; ++s) excise_overlap_add<N>(v[s], v[s + 8], carry[s], g.offset, dst + 2 * TF * s, store);
    }
}

template <int N>
static void excise_launch(gj_ctx* ctx, const uint8_t* d_iq, ExciseGeom g, const float* d_thr, uint8_t* d_out, gj_excise_frame* d_frames) {
    const ExciseRuns runs = excise_runs(g.n_frames, kBlockPoints / N, ExciseCfg<N>::min_waves, ExciseCfg<N>::min_run, ctx->num_cus);
    g.per_run = runs.per_run;
    hipLaunchKernelGGL(excise_kernel<N>, dim3(runs.grid), dim3(kBlockThreads), 0, ctx->stream, d_iq, g, ctx->d_twiddle,
                       window_table(ctx, N), d_thr, d_out, d_frames);
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_excise_frames(size_t n_samples, int nfft) {
    if (nfft < 2 || n_samples < (size_t)nfft) return 0;
    return (n_samples - (size_t)nfft) / ((size_t)nfft / 2) + 1;
}

int gj_excise_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int nfft,
                  const float* d_threshold, uint8_t* d_out, gj_excise_frame* d_frames) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (!d_iq || !d_out || !d_threshold) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = stft_check_capture(ctx, d_iq)) return rc;
    if (int rc = excise_check_shape(ctx, d_threshold, d_frames, n_samples, nfft)) return rc;
    if (int rc = check_range_and_output(ctx, d_iq, nbytes, first_sample, n_samples, d_out)) return rc;
    const ExciseGeom g = excise_geom(ctx, first_sample, n_samples, nfft);
    stft_dispatch(nfft, [&](auto n) { excise_launch<decltype(n)::value>(ctx, d_iq, g, d_threshold, d_out, d_frames); });
    GJ_LAUNCH_CHECK(ctx);
    return excise_copy_edges(ctx, d_iq, g, n_samples, nfft, d_out);
}

}   // extern "C"
