// Three-antenna per-bin canceller (gfx950): the multiple sidelobe canceller with two auxiliaries -- gj_cancel2_dev of
// include/gpsjam.h, which states the definition.  Capture a's short spectrum is predicted from captures b's and c's with
// one complex weight per bin and auxiliary, both predictions are subtracted, and the difference goes through the excisor's
// mask, inverse transform and overlap-add back to uint8 I/Q.  Two auxiliaries give two nulls per bin: two Gaussian jammers
// from different directions in one band, which a single auxiliary cannot null together; the weights are the 2 x 2 MMSE
// solution on gj_csd_dev's sums of the three pairs (gpsjam/coherence.py, cancel_weights2).
//
// This is cancel_kernel (k_cancel.hip) with a third capture, on the same front end (stft_group.h), device stages
// (excise_stages.h) and host side (excise_host.h):
//   * per frame the group transforms a's frame and keeps its 16 bins in registers, transforms b's frame through the same
//     LDS buffer and folds A - W1 B into the held bins, transforms c's frame through the buffer again and subtracts W2 C:
//     Y = (A - W1 B) - W2 C, every product rounded on its own (cancel_predict), the subtractions in that order.  A bin
//     belongs to the same thread in all three transforms: nothing crosses lanes.  A's power is summed in the first fold, in
//     cancel_kernel's order; the mask loop behind the second fold is cancel_kernel's.  So W2 = 0 writes gj_cancel_dev(a, b,
//     W1)'s bytes and records, W1 = 0 those of gj_cancel_dev(a, c, W2), and both 0 gj_excise_dev's on a;
//   * ONE prefetch buffer of 16 registers serves the three captures in rotation: while a is transformed it fetches b's
//     frame, while b is transformed c's, while c is transformed a's next frame.  Every load has one whole transform to
//     land (a's next frame also the inverse), and the kernel holds 16 registers fewer than cancel_kernel there;
//   * the thresholds are held as in cancel_kernel, but at 1024 points, where the 16 registers they take spill: there they are
//     read per frame in the mask loop, out of the cache like the weights (Cancel2Cfg, profiles/NOTES_cancel2.md);
//   * behind the first fold the held bins and A's sum are pinned (an empty asm with "+v", no instruction): without the pin
//     the kernel spills at every size from 32 points on, with one prefetch buffer or two;
//   * the weights are per transform group and per frame as in cancel_kernel: set(f) = min(f / frames_per_set, n_sets - 1),
//     W1 read behind b's transform and W2 behind c's, 16 float2 per thread each out of the cache;
//   * runs, priming iteration, group sums, record, overlap-add and its 16-bit stores are cancel_kernel's.
// Determinism as cancel_kernel's: a frame's Y, mask and inverse are computed from the bytes of its frame triple and its
// weight set alone by the same instructions whichever group, run or launch computes it.
//
// A translation unit of its own with its own extern "C" entry point; no other source refers to it.
#include "excise_host.h"

namespace gj {

template <int N>
struct Cancel2Cfg {
    // cancel_kernel's 32 held and 32 working bins and one prefetch buffer: two workgroups per CU (256 VGPRs) hold that
    // without a spill at every size, 251 registers at 1024 points being the most
    // (profiles/NOTES_cancel2.md has the compiler's figures, and those of the shapes that did spill)
    static constexpr int min_waves = 2;
    static constexpr int min_run = 4;   // as ExciseCfg: bounds the priming overhead at 25 %
    // the 16 thresholds of a thread stay in registers, as in cancel_kernel, wherever that fits: at 1024 points it spills 13
    // registers, and there they are read per frame in the mask loop, out of the cache like the weights.  Held, 4096 points
    // take 0.240 ms for the 10-s triple against 0.273 ms read per frame; at 256 points it makes no difference
    static constexpr bool hold_thresholds = N != 1024;
};

struct Cancel2Geom {
    ExciseGeom e;   // first_sample is capture a's
    unsigned long long first_b, first_c, frames_per_set, n_sets;
};

template <int N>
__global__ __launch_bounds__(kBlockThreads, Cancel2Cfg<N>::min_waves) void cancel2_kernel(
    const uint8_t* __restrict__ iq_a, const uint8_t* __restrict__ iq_b, const uint8_t* __restrict__ iq_c, Cancel2Geom cg,
    const cf* __restrict__ twtab, const float* __restrict__ wintab, const float2* __restrict__ weights,
    const float* __restrict__ thr_tab, uint8_t* __restrict__ out, gj_cancel_frame* __restrict__ frames) {
    using S = StftShape<N>;
    constexpr int TF = S::TF, B = S::B, NP = S::NP, WPF = S::WPF, H = N / 2;
    __shared__ cf lds0[NP > 1 ? lds_span(kBlockPoints) : 1];
    // wave results of a transform group that spans waves (2048, 4096 points), one array per reduction as in cancel_kernel
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
    constexpr bool kHoldThr = Cancel2Cfg<N>::hold_thresholds;
    float thr[kHoldThr ? 16 : 1];
    if constexpr (kHoldThr) {
#pragma unroll
        for (int s = 0; s < 16; ++s) thr[s] = thr_tab[jl + TF * s];
    }
    const c2 koff = make_c2(-g.offset, -g.offset);

    const ExciseRun run(g, blockIdx.x, b, B);   // iteration 0 primes the carry; samples and weight set are clamped alike
    auto load_frame = [&](unsigned (&dst)[16], const uint8_t* base) { stft_load_frame<N, false>(dst, base, jl); };
    const uint8_t* const base_a = iq_a + 2ull * g.first_sample;
    const uint8_t* const base_b = iq_b + 2ull * cg.first_b;
    const uint8_t* const base_c = iq_c + 2ull * cg.first_c;

    unsigned raw[16];                 // a_f, then b_f, c_f, a_{f+1}: the next frame to transform, fetched under the current one
    load_frame(raw, base_a + 2ull * (run.clamped(run.first - 1) * H));
    c2 carry[8];                      // second half of the previous frame's inverse transform: y_{f-1}[jl + TF (s + 8)]
#pragma unroll
    for (int s = 0; s < 8; ++s) carry[s] = make_c2(0.f, 0.f);

    for (long long f = run.first - 1; f < run.end; ++f) {
        const bool owned = f >= run.first && f <= run.last;
        const bool more = f + 1 < run.end;   // workgroup-uniform
        const unsigned long long cur = run.clamped(f);
        const unsigned long long next_at = run.clamped(f + 1) * H;
        unsigned long long set = cur / cg.frames_per_set;
        set = set < cg.n_sets ? set : cg.n_sets - 1;
        const float2* wsrc = weights + set * (2ull * N) + jl;   // W1 of the set; W2 lies N further

        c2 a[16];
        stft_unpack_window(a, raw, wp, koff);
        load_frame(raw, base_b + 2ull * (cur * H));
        stft_passes<N, 0>(a, lds0, b * lds_span(N), jl, tw, ktw);

        c2 v[16];
        stft_unpack_window(v, raw, wp, koff);
        load_frame(raw, base_c + 2ull * (cur * H));
        stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

        // this thread's bins jl + TF s: A's power, then A - W1 B into the held bins
        float tin = 0.f, tot = 0.f, rem = 0.f, cnt = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
#pragma clang fp contract(off)
            const float2 w = wsrc[TF * s];
            const c2 wb = cancel_predict(make_c2(w.x, w.y), v[s]);
            tin += __builtin_fmaf(a[s].x, a[s].x, a[s].y * a[s].y) * g.scale2;
            a[s] = make_c2(a[s].x - wb.x, a[s].y - wb.y);
        }
        // pinned: the subtraction is done here, and only a and tin cross c's transform (NOTES_cancel2.md)
#pragma unroll
        for (int s = 0; s < 16; ++s) asm volatile("" : "+v"(a[s].x), "+v"(a[s].y));
        asm volatile("" : "+v"(tin));

        stft_unpack_window(v, raw, wp, koff);
        if (more) load_frame(raw, base_a + 2ull * next_at);
        stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

        // Y = (A - W1 B) - W2 C, power, mask, conjugate for the way back
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            // no contraction here, as in excise_kernel: removed must equal total, bit for bit, when every bin is excised
#pragma clang fp contract(off)
            const float2 w = wsrc[N + TF * s];
            const c2 wc = cancel_predict(make_c2(w.x, w.y), v[s]);
            const float yx = a[s].x - wc.x, yy = a[s].y - wc.y;
            const float p = __builtin_fmaf(yx, yx, yy * yy) * g.scale2;
            float t;
            if constexpr (kHoldThr) t = thr[s]; else t = thr_tab[jl + TF * s];
            const bool cut = p > t;   // strict; false for a NaN threshold
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
static void cancel2_launch(gj_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, const uint8_t* d_c, Cancel2Geom cg,
                           const float* d_weights, const float* d_thr, uint8_t* d_out, gj_cancel_frame* d_frames) {
    const ExciseRuns runs = excise_runs(cg.e.n_frames, kBlockPoints / N, Cancel2Cfg<N>::min_waves, Cancel2Cfg<N>::min_run, ctx->num_cus);
    cg.e.per_run = runs.per_run;
    hipLaunchKernelGGL(cancel2_kernel<N>, dim3(runs.grid), dim3(kBlockThreads), 0, ctx->stream, d_a, d_b, d_c, cg, ctx->d_twiddle,
                       window_table(ctx, N), reinterpret_cast<const float2*>(d_weights), d_thr, d_out, d_frames);
}

}   // namespace gj

using namespace gj;

extern "C" {

int gj_cancel2_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b, size_t nbytes_b, size_t first_b,
                   const uint8_t* d_c, size_t nbytes_c, size_t first_c, size_t n_samples, int nfft, const float* d_weights,
                   size_t frames_per_set, size_t n_sets, const float* d_threshold, uint8_t* d_out, gj_cancel_frame* d_frames) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (!d_a || !d_b || !d_c || !d_out || !d_threshold || !d_weights) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = stft_check_capture(ctx, d_a)) return rc;
    if (int rc = stft_check_capture(ctx, d_b)) return rc;
    if (int rc = stft_check_capture(ctx, d_c)) return rc;
    if (frames_per_set == 0 || n_sets == 0) return fail(ctx, GJ_ERR_INVALID, "frames_per_set and n_sets must be >= 1");
    if (reinterpret_cast<uintptr_t>(d_weights) & 7) return fail(ctx, GJ_ERR_INVALID, "weights must be 8-byte aligned");
    if (int rc = excise_check_shape(ctx, d_threshold, d_frames, n_samples, nfft)) return rc;
    if (int rc = check_range_and_output(ctx, d_a, nbytes_a, first_a, n_samples, d_out)) return rc;
    if (int rc = check_range_and_output(ctx, d_b, nbytes_b, first_b, n_samples, d_out)) return rc;
    if (int rc = check_range_and_output(ctx, d_c, nbytes_c, first_c, n_samples, d_out)) return rc;
    const Cancel2Geom cg{excise_geom(ctx, first_a, n_samples, nfft), first_b, first_c, frames_per_set, n_sets};
    stft_dispatch(nfft, [&](auto n) { cancel2_launch<decltype(n)::value>(ctx, d_a, d_b, d_c, cg, d_weights, d_threshold, d_out, d_frames); });
    GJ_LAUNCH_CHECK(ctx);
    return excise_copy_edges(ctx, d_a, cg.e, n_samples, nfft, d_out);
}

}   // extern "C"
