// Chirp-domain interference excision (gfx950): the excisor of k_excise.hip with a de-chirp in front of the forward
// transform and the re-chirp behind the inverse one -- gj_excise_chirp_dev of include/gpsjam.h, which states the
// definition -- and gj_chirp_rates_dev, which turns the records of the chirp-rate search (k_chirp.hip) into the per-frame
// rates it reads.  A sweep that crosses hundreds of bins inside one frame is, behind the de-chirp of its rate, a line of
// a few bins: the mask takes that line out and the re-chirp puts everything else back where it was.
//
// The structure is excise_kernel's: the run of consecutive frames per transform group with its priming iteration, the
// mask, the group sums and the overlap-add are the same text (excise_stages.h), and so are the carry of eight c2, the
// generic exchange schedule at 4096 points, the records and the edges copy.  What is this kernel's own:
//   * the rate q_f of the frame is read by the transform group with the frame's samples (prefetched with them, clamped
//     like them), so it is uniform in the group; the priming iteration reads the rate of the frame it primes with;
//   * c_f[jl + TF s], the thread's sixteen factors, come from chirp_phase.h: exact integer phases, 2 + 16 / min(TF, 16)
//     sincospif per thread and frame, nothing carried from frame to frame;
//   * a thread's input points and output points are both jl + TF s, so the SAME sixteen factors serve both ends:
//     v = (w x) c_f goes into the forward transform, and with z = FFT(conj(M X)) the re-chirped frame is
//     conj(c_f) IFFT(M X) = conj(c_f) conj(z) / N = conj(z c_f) / N -- one more multiplication by c_f itself, then the
//     parent's conjugate, 1 / N and overlap-add.  The factors are held across the two transforms: 32 registers on top of
//     excise_kernel's, inside the 256 that two workgroups per CU leave (profiles/NOTES_excise_chirp.md has the counts);
//   * at q_f = 0, or any multiple of 2 N^2, every factor is exactly (1, +0), both products return their other operand
//     (up to the sign of a zero, which no later operation can tell apart) and the frame's record and bytes are
//     gj_excise_dev's.
// Barriers: every __syncthreads() of the loop body is executed by every thread in every iteration, clamped frames outside
// the call included; the factor exchange is a lane permutation inside aligned sets of at most 16 lanes, with every lane
// active.
// Determinism: as excise_kernel, with "its own bytes" read as "its own bytes and its own q".
//
// A translation unit of its own with its own extern "C" entry points; the frame count is gj_excise_frames (k_excise.hip, by
// its declaration in include/gpsjam.h); the shared refusals, the run arithmetic and the edges copy are excise_host.h, which
// gives this translation unit a copy of the edges kernel of its own: a kernel of another translation unit cannot be
// launched from this one without relocatable device code.
#include "chirp_phase.h"
#include "excise_host.h"

namespace gj {

template <int N>
struct ExciseChirpCfg {
    // excise_kernel's ~160 live registers and the 32 of the held factors: two workgroups per CU (256 VGPRs)
    static constexpr int min_waves = 2;
    static constexpr int min_run = 4;   // as ExciseCfg: bounds the priming overhead at 25 %
};

template <int N>
__global__ __launch_bounds__(kBlockThreads, ExciseChirpCfg<N>::min_waves) void excise_chirp_kernel(
    const uint8_t* __restrict__ iq, ExciseGeom g, const cf* __restrict__ twtab, const float* __restrict__ wintab,
    const int32_t* __restrict__ rate, const float* __restrict__ thr_tab, uint8_t* __restrict__ out,
    gj_excise_frame* __restrict__ frames) {
    using S = StftShape<N>;
    constexpr int TF = S::TF, B = S::B, NP = S::NP, WPF = S::WPF, H = N / 2;
    __shared__ cf lds0[NP > 1 ? lds_span(kBlockPoints) : 1];
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

    const ExciseRun run(g, blockIdx.x, b, B);   // iteration 0 primes the carry; samples and rate are clamped alike
    auto frame_base = [&](long long f) { return iq + 2ull * (g.first_sample + run.clamped(f) * H); };
    auto load_frame = [&](unsigned (&dst)[16], const uint8_t* base) { stft_load_frame<N, false>(dst, base, jl); };

    unsigned raw[16];   // the NEXT frame's samples and rate are fetched while the current ones are transformed
    load_frame(raw, frame_base(run.first - 1));
    unsigned q_next = (unsigned)rate[run.clamped(run.first - 1)];
    c2 carry[8];        // second half of the previous frame's re-chirped inverse transform
#pragma unroll
    for (int s = 0; s < 8; ++s) carry[s] = make_c2(0.f, 0.f);

    for (long long f = run.first - 1; f < run.end; ++f) {
        const bool owned = f >= run.first && f <= run.last;
        c2 v[16], c[16];
        stft_unpack_window(v, raw, wp, koff);
        chirp_factors<N>(c, q_next, jl);
        if (f + 1 < run.end) {   // workgroup-uniform
            load_frame(raw, frame_base(f + 1));
            q_next = (unsigned)rate[run.clamped(f + 1)];
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) v[s] = cmul(v[s], c[s]);

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

        // the re-chirp: y_f = conj(v c_f) / N
#pragma unroll
        for (int s = 0; s < 16; ++s) v[s] = cmul(v[s], c[s]);
        const bool store = owned && f >= 1;
        uint8_t* dst = out + 2ull * ((unsigned long long)(f < 0 ? 0 : f) * H) + 2 * jl;
#pragma unroll
        for (int s = 0; s < 8; ++s) excise_overlap_add<N>(v[s], v[s + 8], carry[s], g.offset, dst + 2 * TF * s, store);
    }
}

// d_rate[f] = rate_first + rate_index_f * rate_step where the search concentrated the frame, 0 elsewhere
__global__ __launch_bounds__(256) void chirp_rates_kernel(const gj_chirp_frame* __restrict__ scan, unsigned long long n_frames,
                                                          int rate_first, int rate_step, float min_concentration,
                                                          int32_t* __restrict__ rate) {
    for (unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; f < n_frames;
         f += (unsigned long long)gridDim.x * blockDim.x) {
        const float total = scan[f].total, peak = scan[f].peak;
        float need;
        {
#pragma clang fp contract(off)
            need = min_concentration * total;   // one float multiply, rounded once
        }
        const bool on = total > 0.f && peak >= need;   // false for a NaN on either side
        const unsigned q = (unsigned)rate_first + (unsigned)scan[f].rate_index * (unsigned)rate_step;   // modulo 2^32
        rate[f] = on ? (int32_t)q : 0;
    }
}

template <int N>
static void excise_chirp_launch(gj_ctx* ctx, const uint8_t* d_iq, ExciseGeom g, const int32_t* d_rate, const float* d_thr,
                                uint8_t* d_out, gj_excise_frame* d_frames) {
    const ExciseRuns runs = excise_runs(g.n_frames, kBlockPoints / N, ExciseChirpCfg<N>::min_waves, ExciseChirpCfg<N>::min_run,
                                        ctx->num_cus);
    g.per_run = runs.per_run;
    hipLaunchKernelGGL(excise_chirp_kernel<N>, dim3(runs.grid), dim3(kBlockThreads), 0, ctx->stream, d_iq, g, ctx->d_twiddle,
                       window_table(ctx, N), d_rate, d_thr, d_out, d_frames);
}

}   // namespace gj

using namespace gj;

extern "C" {

int gj_excise_chirp_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int nfft,
                        const int32_t* d_rate, const float* d_threshold, uint8_t* d_out, gj_excise_frame* d_frames) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (!d_iq || !d_out || !d_threshold || !d_rate) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = stft_check_capture(ctx, d_iq)) return rc;
    if (reinterpret_cast<uintptr_t>(d_rate) & 3) return fail(ctx, GJ_ERR_INVALID, "rates must be 4-byte aligned");
    if (int rc = excise_check_shape(ctx, d_threshold, d_frames, n_samples, nfft)) return rc;
    if (int rc = check_range_and_output(ctx, d_iq, nbytes, first_sample, n_samples, d_out)) return rc;
    const ExciseGeom g = excise_geom(ctx, first_sample, n_samples, nfft);
    stft_dispatch(nfft, [&](auto n) { excise_chirp_launch<decltype(n)::value>(ctx, d_iq, g, d_rate, d_threshold, d_out, d_frames); });
    GJ_LAUNCH_CHECK(ctx);
    return excise_copy_edges(ctx, d_iq, g, n_samples, nfft, d_out);
}

int gj_chirp_rates_dev(gj_ctx* ctx, const gj_chirp_frame* d_scan, size_t n_frames, int rate_first, int rate_step,
                       float min_concentration, int32_t* d_rate) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (!d_scan || !d_rate) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (reinterpret_cast<uintptr_t>(d_scan) & 3) return fail(ctx, GJ_ERR_INVALID, "records must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_rate) & 3) return fail(ctx, GJ_ERR_INVALID, "rates must be 4-byte aligned");
    if (n_frames == 0) return fail(ctx, GJ_ERR_INVALID, "n_frames must be >= 1");
    if (rate_step < 1) return fail(ctx, GJ_ERR_INVALID, "rate_step must be >= 1");
    const unsigned long long blocks = ((unsigned long long)n_frames + 255) / 256;
    const unsigned long long cap = (unsigned long long)ctx->num_cus * 8;
    hipLaunchKernelGGL(chirp_rates_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, ctx->stream, d_scan,
                       (unsigned long long)n_frames, rate_first, rate_step, min_concentration, d_rate);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
