// Chirp-rate search (gfx950): the short-time ridge of k_ridge.hip behind a de-chirp, for every rate of a grid --
// gj_chirp_dev of include/gpsjam.h, which states the definition.  A sweep that crosses many bins inside one frame does
// not concentrate in any bin of that frame's spectrum; multiplied by the conjugate of a unit chirp of the right rate it
// is a tone again.  Per frame the kernel transforms the windowed samples once per rate, reduces each spectrum to the
// ridge's four numbers and keeps the rate with the largest peak (gpsjam/classify.py classify_swept reads the result).
//
// The front end is stft_group.h, used as ridge_kernel uses it: same workgroup of transform groups, same loads with the
// next step's prefetch, same passes, same three reductions; the frame walk and the host side of the call are ridge_kernel's
// text (stft_frames.h), the reductions a copy of its text (stft_frames.h says why).  What is the search's own:
//   * the unpacked, windowed frame stays in registers (held[16]) across the rate loop; every rate multiplies a copy by
//     c_r and transforms the copy;
//   * c_r[n] = exp(-i pi m / N^2) with the INTEGER phase m = (q_r n^2) mod 2 N^2.  2 N^2 is a power of two that divides
//     2^32, so the low 2 log2(N) + 1 bits of a 32-bit product q_r * (...) are its phase exactly, whatever the sign of q_r;
//     taken as a signed field they are m' in [-N^2, N^2), congruent to m.  |m'| <= 2^24 converts to float exactly,
//     m' / N^2 is an exact scaling by a power of two, and sincospif of that exact argument is good to the last bits of a
//     float.  A thread's sixteen samples are n = jl0 + TF s, and q n^2 = q jl0^2 + s (2 q jl0 TF) + s^2 (q TF^2) splits
//     c_r[n] into e8 d^(s - 8), the thread's own, and a third factor that depends on (q, s) alone.  So a rate costs three
//     sincospif per thread instead of sixteen: e8 and d from their exact phases, d's powers by at most eight complex
//     products up and down from the middle slot, and the third factor evaluated by lane s for slot s and handed round
//     the wave by v_readlane.  Each of the three comes from an exact integer phase; a slot's factor is a product of at
//     most ten unit-modulus floats (profiles/NOTES_chirp.md has the error this leaves).  Every rate is computed from q_r
//     alone: nothing is carried from rate to rate, neither a complex factor (its rounding error would grow with the number
//     of rates) nor an integer phase;
//   * at q_r = 0 every factor is exactly (1, +-0) and every product returns its other operand's bits, so the single
//     rate 0 gives gj_ridge_dev's record;
//   * the best rate is selected by VALUE in registers (strictly greater: the smallest r among equals).  Every lane of a
//     transform group holds the same reduced bits, so the selection is uniform in the group and needs no exchange.
// Barriers: every __syncthreads() of the loop body is executed by every thread for every rate -- n_rates is a kernel
// argument, `active` only guards the two stores.  At 2048 points two transform groups share the workgroup's barriers.
// Determinism: as ridge_kernel's, and per rate: d_peaks[f][r] depends on the frame's bytes and q_r alone.
//
// A translation unit of its own with its own extern "C" entry point, like k_ridge.hip.
#include "chirp_phase.h"
#include "stft_frames.h"

namespace gj {

template <int N>
struct ChirpCfg {
    // ridge_kernel's three workgroups per CU hold up to 256 points: 149 to 166 of the 168 registers, no scratch.  From 512
    // points on the held frame's 32 registers on top of the window, the twiddles, the prefetched samples, the transform's
    // 32 and the 16 powers no longer fit (ridge_kernel itself needs 143 to 166 there), so those take two
    // (profiles/NOTES_chirp.md has the counts and what was tried).
    static constexpr int min_waves = N <= 256 ? (N >= 32 ? 3 : 2) : 2;
    static constexpr bool xpose = N == 4096;
    static constexpr bool wide_load = N <= 32;
};

struct ChirpGeom {
    unsigned long long first_sample, hop, n_frames, nsteps;
    float neg_off;   // -offset of the unpack convention
    float scale2;    // scale^2, applied to the three powers at the end
    int guard;
    int rate_first, rate_step, n_rates;
};

template <int N>
__global__ __launch_bounds__(kBlockThreads, ChirpCfg<N>::min_waves) void chirp_kernel(const uint8_t* __restrict__ iq, ChirpGeom g,
                                                                                      const cf* __restrict__ twtab,
                                                                                      const float* __restrict__ wintab,
                                                                                      gj_chirp_frame* __restrict__ out,
                                                                                      float* __restrict__ peaks) {
    using Cfg = ChirpCfg<N>;
    using S = StftShape<N>;
    constexpr int TF = S::TF, B = S::B, NP = S::NP, WPF = S::WPF;
    constexpr bool XP = Cfg::xpose;
    constexpr int SPAN = XP ? X4096::kSpan : lds_span(kBlockPoints);
    __shared__ cf lds0[NP > 1 ? SPAN : 1];
    // Wave results of a transform group that spans waves (2048, 4096 points), one array per reduction as in ridge_kernel.
    // The arrays are reused once per RATE here.  Write after read still holds: red_sum / red_max of rate r are read between
    // the first and the second reduction barrier of rate r, and a wave can post rate r + 1's values only after it has
    // passed the second barrier of rate r, at which every wave has finished those reads; red_bin is read between the second
    // and the third barrier and written again behind the third; red_sec is read behind the third barrier and written
    // again only behind the exchange barriers of the next transform (two at least at these sizes), whether that
    // transform belongs to the next rate or to the next step.
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
        c2 held[16];   // the windowed frame, input index jl0 + TF s
        stft_unpack_window(held, raw, wp, koff);
        if (step + gridDim.x < g.nsteps) load_frame(raw, step + gridDim.x);   // workgroup-uniform

        float best_tot = 0.f, best_peak = 0.f, best_sec = 0.f;
        int best_bin = 0, best_rate = 0;
        for (int r = 0; r < g.n_rates; ++r) {
            const unsigned q = (unsigned)(g.rate_first + r * g.rate_step);
            // exp(-i pi m / N^2) of a phase given modulo 2^32, from its exactly reduced integer (chirp_phase.h, and the head
            // of this file): (cos, sin) of pi m / N^2
            const auto turn = [](unsigned ph, float& cs, float& sn) { chirp_turn<N>(ph, cs, sn); };
            // n = jl0 + TF s:  q n^2 = q jl0^2 + s (2 q jl0 TF) + s^2 (q TF^2), all modulo 2^32.  The last term is the same
            // in every thread: lane s of each wave evaluates it for slot s and v_readlane hands it round.
            const unsigned uj = (unsigned)jl0;
            const unsigned pj = q * (uj * uj), pd = q * (2u * uj * (unsigned)TF), pc = q * (unsigned)(TF * TF);
            float lcs, lsn;
            {
                const unsigned sl = (unsigned)tid & 15u;
                turn(pc * (sl * sl), lcs, lsn);
                lsn = 0.f - lsn;   // the imaginary part; 0 - (+0) keeps rate 0 at (1, +0)
            }
            c2 v[16];
            const auto slot = [&](int s, c2 x) {   // x * exp(-i pi q TF^2 s^2 / N^2), the factor wave-uniform
                const float kc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lcs), s));
                const float ks = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lsn), s));
                v[s] = make_c2(fmaf(-x.y, ks, x.x * kc), fmaf(x.y, kc, x.x * ks));
            };
            if constexpr (TF == 1) {   // one thread per frame: jl0 = 0, n = s
#pragma unroll
                for (int s = 0; s < 16; ++s) slot(s, held[s]);
            } else {
                // the thread's own factor exp(-i pi (q jl0^2 + s 2 q jl0 TF) / N^2) = e8 d^(s - 8): e8 and d from their
                // exact phases, the powers by at most eight products up and eight down from the middle slot
                float ecs, esn, dcs, dsn;
                turn(pj + 8u * pd, ecs, esn);
                turn(pd, dcs, dsn);
                const c2 e8 = make_c2(ecs, 0.f - esn), up = make_c2(dcs, 0.f - dsn), down = make_c2(dcs, dsn);
                c2 e = e8;
#pragma unroll
                for (int s = 8; s < 16; ++s) {
                    slot(s, cmul(held[s], e));
                    e = cmul(e, up);
                }
                e = e8;
#pragma unroll
                for (int s = 7; s >= 0; --s) {
                    e = cmul(e, down);
                    slot(s, cmul(held[s], e));
                }
            }

            if constexpr (XP) stft_passes_x4096(v, lds0, tid, tw, ktw);
            else stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

            // this thread's bins jl + TF s, ascending in s; from here to `sec` the arithmetic is ridge_kernel's
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
            int bin = group_min_i<G>(mx == gmx ? jl + TF * ms : INT_MAX);
            if constexpr (WPF > 1) {
                waves_post(red_bin[b], tid, bin);
                __syncthreads();
                bin = waves_fold(red_bin[b], [](int a, int c) { return min(a, c); });
            }
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
            if (peaks && active && jl0 == 0) peaks[f * (unsigned)g.n_rates + (unsigned)r] = gmx * g.scale2;
            // by value, the same in every lane of the group; no barrier and no LDS access depends on it
            if (r == 0 || gmx > best_peak) {
                best_tot = tot; best_peak = gmx; best_sec = sec; best_bin = bin; best_rate = r;
            }
        }
        if (active && jl0 == 0) {   // one lane per transform group
            gj_chirp_frame rec;
            rec.total = best_tot * g.scale2;
            rec.peak = best_peak * g.scale2;
            rec.second = best_sec * g.scale2;
            rec.peak_bin = best_bin;
            rec.rate_index = best_rate;
            rec.reserved = 0;
            out[f] = rec;
        }
    }
}

template <int N>
static void chirp_launch(gj_ctx* ctx, const uint8_t* d_iq, ChirpGeom g, gj_chirp_frame* d_out, float* d_peaks) {
    const unsigned grid = frames_one_round<N>(ctx, ChirpCfg<N>::min_waves, g);
    hipLaunchKernelGGL(chirp_kernel<N>, dim3(grid), dim3(kBlockThreads), 0, ctx->stream, d_iq, g, ctx->d_twiddle, window_table(ctx, N),
                       d_out, d_peaks);
}

}   // namespace gj

using namespace gj;

extern "C" {

int gj_chirp_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, int nfft, size_t hop, size_t n_frames, int guard,
                 int rate_first, int rate_step, int n_rates, gj_chirp_frame* d_out, float* d_peaks) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (n_rates > GJ_CHIRP_MAX_RATES) return fail(ctx, GJ_ERR_UNSUPPORTED, "n_rates %d: at most %d rates per call", n_rates, GJ_CHIRP_MAX_RATES);
    if (n_rates < 1) return fail(ctx, GJ_ERR_INVALID, "n_rates must be >= 1");
    if (rate_step < 1) return fail(ctx, GJ_ERR_INVALID, "rate_step must be >= 1");
    const long long half = (long long)nfft * nfft / 2;
    const long long q_last = (long long)rate_first + (long long)(n_rates - 1) * rate_step;
    if (rate_first < -half || q_last > half)
        return fail(ctx, GJ_ERR_INVALID, "rates %d .. %lld: |q| must not exceed nfft^2 / 2 = %lld", rate_first, q_last, half);
    if (int rc = frames_check_buffers(ctx, d_iq, d_out)) return rc;
    if (reinterpret_cast<uintptr_t>(d_peaks) & 3) return fail(ctx, GJ_ERR_INVALID, "d_peaks must be 4-byte aligned");
    if (int rc = frames_check_geometry(ctx, nbytes, first_sample, nfft, hop, n_frames, guard)) return rc;
    ChirpGeom g = frames_geom<ChirpGeom>(ctx, first_sample, hop, n_frames, guard);
    g.rate_first = rate_first;
    g.rate_step = rate_step;
    g.n_rates = n_rates;
    stft_dispatch(nfft, [&](auto n) { chirp_launch<decltype(n)::value>(ctx, d_iq, g, d_out, d_peaks); });
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
