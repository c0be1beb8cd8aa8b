// Two-antenna per-bin canceller (gfx950): the frequency-domain sidelobe canceller, also called per-bin power inversion --
// gj_cancel_dev of include/gpsjam.h, which states the definition.  Capture a's short spectrum is predicted from capture
// b's with one complex weight per bin, the prediction is subtracted, and the difference goes through the excisor's mask,
// inverse transform and overlap-add back to uint8 I/Q.  What is coherent between the antennas -- a broadband Gaussian
// jammer that none of the other cleaners can touch -- is removed; the weights come from gj_csd_dev's sums
// (gpsjam/coherence.py, cancel_weights).
//
// This is excise_kernel (k_excise.hip) with csd_kernel's two-capture pattern (k_csd.hip) in front, on the front end of
// stft_group.h, the device stages of excise_stages.h and the host side of excise_host.h:
//   * runs with their priming iteration, the group sums, the overlap-add and its 16-bit stores are excise_kernel's text
//     (excise_stages.h), the carry of eight c2, the generic exchange schedule at 4096 points and the second pass its
//     structure; the mask loop, with the prediction and a fourth sum, keeps the excisor's arithmetic behind the subtraction:
//     with every weight 0 the call writes gj_excise_dev's bytes on capture a;
//   * per frame the group transforms a's frame and keeps its 16 bins in registers, transforms b's frame through the same
//     LDS buffer (the front end's exchange ends with a barrier behind the gather, so the buffer is free again) and forms
//     Y = A - W B in registers.  A bin belongs to the same thread in both transforms: nothing crosses lanes;
//   * both captures' next frames are fetched under the current transforms;
//   * the weights are per transform group and per frame: set(f) = min(f / frames_per_set, n_sets - 1), read behind b's
//     transform, 16 float2 per thread out of the cache (holding them would add 32 registers to a kernel that has none to
//     spare, and a set lasts only frames_per_set frames anyway).  The priming iteration uses the set of the frame it
//     primes with.  No barrier depends on the set;
//   * the record has one more sum, total_in, over A's bins.
// Determinism: a frame's Y, mask and inverse are computed from the bytes of its frame pair and its weight set alone by the
// same instructions whichever group, run or launch computes it, every sum runs in an order fixed by N, and an output
// sample is prev + cur of its two frames.
//
// A translation unit of its own with its own extern "C" entry point; no other source refers to it.
#include "excise_host.h"

namespace gj {

template <int N>
struct CancelCfg {
    // excise_kernel's ~160 live registers, 32 held bins of a, 16 more prefetched samples and the weights on their way:
    // two workgroups per CU (256 VGPRs) hold that without a spill at every size, 254 registers at 2048 points being the
    // most; three (168) would spill (profiles/NOTES_cancel.md has the compiler's figures)
    static constexpr int min_waves = 2;
    static constexpr int min_run = 4;   // as ExciseCfg: bounds the priming overhead at 25 %
};

struct CancelGeom {
    ExciseGeom e;   // first_sample is capture a's
    unsigned long long first_b, frames_per_set, n_sets;
};

template <int N>
__global__ __launch_bounds__(kBlockThreads, CancelCfg<N>::min_waves) void cancel_kernel(
    const uint8_t* __restrict__ iq_a, const uint8_t* __restrict__ iq_b, CancelGeom cg, const cf* __restrict__ twtab,
    const float* __restrict__ wintab, const float2* __restrict__ weights, const float* __restrict__ thr_tab,
    uint8_t* __restrict__ out, gj_cancel_frame* __restrict__ frames) {
    using S = StftShape<N>;
    constexpr int TF = S::TF, B = S::B, NP = S::NP, WPF = S::WPF, H = N / 2;
    __shared__ cf lds0[NP > 1 ? lds_span(kBlockPoints) : 1];
    // wave results of a transform group that spans waves (2048, 4096 points), one array per reduction as in excise_kernel
    constexpr int RB = WPF > 1 ? B : 1;
    __shared__ float red_in[RB][WPF], red_tot[RB][WPF], red_rem[RB][WPF], red_cnt[RB][WPF];
    const int tid = threadIdx.x;
    const StftRoles role = stft_roles<N, false>(tid);
    const int b = role.b, jl = role.jl;   // input points, bins and output points of this thread: jl + TF s
    const ExciseGeom& g = cg.e;

    const InnerTw ktw = inner_twiddles();
    c2 tw[3][15], wp[8];
    stft_load_twiddles<N>(tw, twtab, jl);
#pragma unroll
    for (int s = 0; s < 8; ++s) wp[s] = stft_window_pair<N>(wintab, jl, s);
    float thr[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) thr[s] = thr_tab[jl + TF * s];
    const c2 koff = make_c2(-g.offset, -g.offset);

    const ExciseRun run(g, blockIdx.x, b, B);   // iteration 0 primes the carry; samples and weight set are clamped alike
    auto load_frame = [&](unsigned (&dst)[16], const uint8_t* base) { stft_load_frame<N, false>(dst, base, jl); };
    const uint8_t* const base_a = iq_a + 2ull * g.first_sample;
    const uint8_t* const base_b = iq_b + 2ull * cg.first_b;

    unsigned raw_a[16], raw_b[16];   // the NEXT pair's samples are fetched while the current ones are transformed
    load_frame(raw_a, base_a + 2ull * (run.clamped(run.first - 1) * H));
    load_frame(raw_b, base_b + 2ull * (run.clamped(run.first - 1) * H));
    c2 carry[8];                     // second half of the previous frame's inverse transform: y_{f-1}[jl + TF (s + 8)]
#pragma unroll
    for (int s = 0; s < 8; ++s) carry[s] = make_c2(0.f, 0.f);

    for (long long f = run.first - 1; f < run.end; ++f) {
        const bool owned = f >= run.first && f <= run.last;
        const bool more = f + 1 < run.end;   // workgroup-uniform
        const unsigned long long next_at = run.clamped(f + 1) * H;
        unsigned long long set = run.clamped(f) / cg.frames_per_set;
        set = set < cg.n_sets ? set : cg.n_sets - 1;
        const float2* wsrc = weights + set * (unsigned long long)N + jl;

        c2 a[16];
        stft_unpack_window(a, raw_a, wp, koff);
        if (more) load_frame(raw_a, base_a + 2ull * next_at);
        stft_passes<N, 0>(a, lds0, b * lds_span(N), jl, tw, ktw);

        c2 v[16];
        stft_unpack_window(v, raw_b, wp, koff);
        if (more) load_frame(raw_b, base_b + 2ull * next_at);
        stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

        // this thread's bins jl + TF s of both: Y = A - W B, power, mask, conjugate for the way back
        float tin = 0.f, tot = 0.f, rem = 0.f, cnt = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            // no contraction here, as in excise_kernel: removed must equal total, bit for bit, when every bin is excised
#pragma clang fp contract(off)
            const float2 w = wsrc[TF * s];
            const c2 wb = cancel_predict(make_c2(w.x, w.y), v[s]);
            const float pin = __builtin_fmaf(a[s].x, a[s].x, a[s].y * a[s].y) * g.scale2;
            const float yx = a[s].x - wb.x, yy = a[s].y - wb.y;
            const float p = __builtin_fmaf(yx, yx, yy * yy) * g.scale2;
            const bool cut = p > thr[s];   // strict; false for a NaN threshold
            tin += pin;
            tot += p;
            rem += cut ? p : 0.f;
            cnt += cut ? 1.f : 0.f;        // at most 4096: exact in float
            v[s] = cut ? make_c2(0.f, 0.f) : make_c2(yx, -yy);
        }
        const GroupSum<N> s_in{tin, red_in}, s_tot{tot, red_tot}, s_rem{rem, red_rem}, s_cnt{cnt, red_cnt};
        group_sums_post<N>(b, tid, s_in, s_tot, s_rem, s_cnt);
        if constexpr (WPF > 1) __syncthreads();
        group_sums_fold<N>(b, s_in, s_tot, s_rem, s_cnt);
        if (frames && owned && jl == 0) {   // one lane per transform group
            gj_cancel_frame r;
            r.total_in = tin;
            r.total = tot;
            r.removed = rem;
            r.n_excised = (int)cnt;
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
static void cancel_launch(gj_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, CancelGeom cg, const float* d_weights, const float* d_thr,
                          uint8_t* d_out, gj_cancel_frame* d_frames) {
    const ExciseRuns runs = excise_runs(cg.e.n_frames, kBlockPoints / N, CancelCfg<N>::min_waves, CancelCfg<N>::min_run, ctx->num_cus);
    cg.e.per_run = runs.per_run;
    hipLaunchKernelGGL(cancel_kernel<N>, dim3(runs.grid), dim3(kBlockThreads), 0, ctx->stream, d_a, d_b, cg, ctx->d_twiddle,
                       window_table(ctx, N), reinterpret_cast<const float2*>(d_weights), d_thr, d_out, d_frames);
}

}   // namespace gj

using namespace gj;

extern "C" {

int gj_cancel_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b, size_t nbytes_b, size_t first_b,
                  size_t n_samples, int nfft, const float* d_weights, size_t frames_per_set, size_t n_sets, const float* d_threshold,
                  uint8_t* d_out, gj_cancel_frame* d_frames) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (!d_a || !d_b || !d_out || !d_threshold || !d_weights) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = stft_check_capture(ctx, d_a)) return rc;
    if (int rc = stft_check_capture(ctx, d_b)) return rc;
    if (frames_per_set == 0 || n_sets == 0) return fail(ctx, GJ_ERR_INVALID, "frames_per_set and n_sets must be >= 1");
    if (reinterpret_cast<uintptr_t>(d_weights) & 7) return fail(ctx, GJ_ERR_INVALID, "weights must be 8-byte aligned");
    if (int rc = excise_check_shape(ctx, d_threshold, d_frames, n_samples, nfft)) return rc;
    if (int rc = check_range_and_output(ctx, d_a, nbytes_a, first_a, n_samples, d_out)) return rc;
    if (int rc = check_range_and_output(ctx, d_b, nbytes_b, first_b, n_samples, d_out)) return rc;
    const CancelGeom cg{excise_geom(ctx, first_a, n_samples, nfft), first_b, frames_per_set, n_sets};
    stft_dispatch(nfft, [&](auto n) { cancel_launch<decltype(n)::value>(ctx, d_a, d_b, cg, d_weights, d_threshold, d_out, d_frames); });
    GJ_LAUNCH_CHECK(ctx);
    return excise_copy_edges(ctx, d_a, cg.e, n_samples, nfft, d_out);
}

}   // extern "C"
