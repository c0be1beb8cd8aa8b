// Spectral kurtosis (gfx950): per bin the sums of P and P^2 over the M short spectra of a row, and the estimator
//   SK = (M + 1) / (M - 1) * (M * S2 / S1^2 - 1)
// of Nita & Gary -- gj_sk_dev / gj_sk_rows / gj_sk_workspace of include/gpsjam.h, which states the definition.
// Gaussian noise gives 1 whatever its level or the passband's shape, a steady carrier pulls its bin toward 0 and
// anything intermittent pushes it above 1 (gpsjam/kurtosis.py reads it).
//
// The transform front end -- the workgroup of transform groups, the loads, the window, the passes and their exchange
// barrier -- is stft_group.h, shared with k_ridge.hip and k_excise.hip.  What is the kurtosis's own:
//   * a transform group, not a workgroup, is the unit of work: it takes one BLOCK of a row, a run of up to kRowMaxRun
//     consecutive frames, and keeps 16 + 16 accumulators in registers for sum P and sum P^2 of its 16 bins.  Nothing
//     is reduced across lanes: a bin belongs to one thread;
//   * powers are accumulated in LSB units (scale^2 and scale^4 are applied at the end; the worst case, a full-scale
//     tone at 4096 points over 65536 frames, sums P^2 to about 1e27);
//   * a block ends with one partial pair, float32[2][N], in the workspace; a second small launch adds a row's partials
//     in block order, scales, and evaluates SK in double from the rounded float32 sums.
// Rows, blocks, the partition rule and the determinism that rests on it are stft_rows.h, shared with k_csd.hip: a capture
// with few rows still spreads over M / kRowMaxRun times as many groups.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it
// (tests/hip_stub builds those by name), and K2's module is compiled exactly as before.
#include "stft_rows.h"

#include <cmath>

namespace gj {

template <int N>
struct SkCfg {
    // RidgeCfg's shape where the 32 accumulators still fit beside data, twiddles, window and prefetch in the 168
    // registers of three workgroups per CU; from 512 points on (a second twiddle set) they do not, and two workgroups
    // per CU replace a spill (profiles/NOTES_skurt.md has the compiler's figures)
    static constexpr int min_waves = N >= 512 ? 2 : (N >= 32 ? 3 : 2);
    static constexpr bool xpose = N == 4096;       // the conflict-free exchange schedule of fft_core.h (X4096)
    static constexpr bool wide_load = N <= 32;     // as RidgeCfg
};

struct SkGeom {
    unsigned long long first_sample;
    RowGeom rows;
};

template <int N>
__global__ __launch_bounds__(kBlockThreads, SkCfg<N>::min_waves) void sk_kernel(const uint8_t* __restrict__ iq, SkGeom g,
                                                                                const cf* __restrict__ twtab,
                                                                                const float* __restrict__ wintab,
                                                                                float* __restrict__ partial) {
    using Cfg = SkCfg<N>;
    using S = StftShape<N>;
    constexpr int TF = S::TF, B = S::B, NP = S::NP;
    constexpr bool XP = Cfg::xpose;
    constexpr int SPAN = XP ? X4096::kSpan : lds_span(kBlockPoints);
    __shared__ cf lds0[NP > 1 ? SPAN : 1];
    const int tid = threadIdx.x;
    const StftRoles role = stft_roles<N, XP>(tid);
    const int b = role.b, jl0 = role.jl0, jl = role.jl;

    const InnerTw ktw = inner_twiddles();
    c2 tw[3][15];
    stft_load_twiddles<N>(tw, twtab, jl);

    c2 wp[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) wp[s] = stft_window_pair<N>(wintab, jl0, s);
    const c2 koff = make_c2(g.rows.neg_off, g.rows.neg_off);

    auto block_of = [&](unsigned long long step, unsigned& count) { return row_block_of<B>(g.rows, step, b, count); };
    auto frame_base = [&](unsigned long long f) { return iq + 2ull * (g.first_sample + row_clamp_frame(g.rows, f) * g.rows.hop); };
    auto load_frame = [&](unsigned (&dst)[16], const uint8_t* base) { stft_load_frame<N, Cfg::wide_load>(dst, base, jl0); };

    unsigned raw[16];   // the NEXT frame's samples are fetched while the current ones are transformed
    unsigned long long step = blockIdx.x;   // the grid never exceeds nsteps
    unsigned count = 0;
    unsigned long long f0 = block_of(step, count);
    load_frame(raw, frame_base(f0));
    for (; step < g.rows.nsteps; step += gridDim.x) {
        const bool more = step + gridDim.x < g.rows.nsteps;   // workgroup-uniform
        unsigned next_count = 0;
        const unsigned long long next_f0 = more ? block_of(step + gridDim.x, next_count) : 0ull;
        float s1[16], s2[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) s1[s] = s2[s] = 0.f;

        for (unsigned i = 0; i < g.rows.run; ++i) {
            c2 v[16];
            stft_unpack_window(v, raw, wp, koff);
            if (i + 1 < g.rows.run) load_frame(raw, frame_base(f0 + i + 1));
            else if (more) load_frame(raw, frame_base(next_f0));

            if constexpr (XP) stft_passes_x4096(v, lds0, tid, tw, ktw);
            else stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

            // this thread's bins jl + TF s.  A spare iteration adds zeros: the sums keep their bits.
            const bool counted = i < count;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float p = counted ? fmaf(v[s].x, v[s].x, v[s].y * v[s].y) : 0.f;
                s1[s] += p;
                s2[s] = fmaf(p, p, s2[s]);
            }
        }

        if (count) {   // this group holds a block: its partial pair, [2][N] in FFT order
            float* dst = partial + (step * B + (unsigned)b) * (2ull * N) + jl;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                dst[TF * s] = s1[s];
                dst[N + TF * s] = s2[s];
            }
        }
        f0 = next_f0;
        count = next_count;
    }
}

// A row's partials added in block order, scaled to the units of gj_ridge_dev, and SK in double from the ROUNDED sums
// (what the caller can recompute from d_s1 and d_s2), rounded once.
__global__ __launch_bounds__(256) void sk_finalize_kernel(const float* __restrict__ partial, unsigned long long n_out, int n, unsigned nb,
                                                          double scale2, double scale4, double frames_per_row, float* __restrict__ s1,
                                                          float* __restrict__ s2, float* __restrict__ sk) {
    const double m = frames_per_row, lead = (m + 1.0) / (m - 1.0);
    for (unsigned long long at = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; at < n_out;
         at += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long r = at / (unsigned)n;
        const unsigned k = (unsigned)(at - r * (unsigned)n);
        const float* p = partial + r * nb * (2ull * n) + k;
        float a = p[0], c = p[n];
        for (unsigned j = 1; j < nb; ++j) {
            p += 2 * n;
            a += p[0];
            c += p[n];
        }
        const float f1 = (float)((double)a * scale2), f2 = (float)((double)c * scale4);
        s1[at] = f1;
        s2[at] = f2;
        if (sk) {
            const double d = (double)f1;
            sk[at] = f1 == 0.f ? __builtin_nanf("") : (float)(lead * (m * (double)f2 / (d * d) - 1.0));
        }
    }
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_sk_rows(size_t nbytes, size_t first_sample, int nfft, size_t hop, int frames_per_row) {
    return row_fit(nbytes, first_sample, nfft, hop, frames_per_row);
}

size_t gj_sk_workspace(gj_ctx* ctx, int nfft, int frames_per_row, size_t n_rows) {
    (void)ctx;
    return row_workspace_bytes(2, nfft, frames_per_row, n_rows);
}

int gj_sk_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, int nfft, size_t hop, int frames_per_row,
              size_t n_rows, float* d_s1, float* d_s2, float* d_sk) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = row_check_shape(ctx, nfft, frames_per_row)) return rc;
    if (!d_iq || !d_s1 || !d_s2) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = stft_check_capture(ctx, d_iq)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_s1) | reinterpret_cast<uintptr_t>(d_s2) | reinterpret_cast<uintptr_t>(d_sk)) & 3)
        return fail(ctx, GJ_ERR_INVALID, "outputs must be 4-byte aligned");
    if (hop < 1) return fail(ctx, GJ_ERR_INVALID, "hop must be >= 1");
    const size_t fit = gj_sk_rows(nbytes, first_sample, nfft, hop, frames_per_row);
    if (n_rows == 0 || n_rows > fit)
        return fail(ctx, GJ_ERR_INVALID, "n_rows %zu: 1..%zu rows of %d frames of %d points fit from sample %zu at hop %zu", n_rows, fit,
                    frames_per_row, nfft, first_sample, hop);
    float* partial = nullptr;
    if (int rc = row_workspace(ctx, 2, nfft, frames_per_row, n_rows, &partial)) return rc;
    const SkGeom g{first_sample, row_geom(ctx, hop, frames_per_row, n_rows)};
    stft_dispatch(nfft, [&](auto n) {
        constexpr int N = decltype(n)::value;
        row_launch<N>(ctx, sk_kernel<N>, SkCfg<N>::min_waves, g, partial, d_iq);
    });
    GJ_LAUNCH_CHECK(ctx);
    const unsigned long long n_out = (unsigned long long)n_rows * (unsigned)nfft;
    const double sc2 = ctx->scale * ctx->scale;
    hipLaunchKernelGGL(sk_finalize_kernel, dim3(row_finalize_grid(ctx, n_out)), dim3(256), 0, ctx->stream, partial, n_out, nfft, g.rows.nb, sc2,
                       sc2 * sc2, (double)frames_per_row, d_s1, d_s2, d_sk);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
