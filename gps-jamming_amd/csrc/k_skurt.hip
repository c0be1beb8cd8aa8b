// Spectral kurtosis (gfx950): per bin the sums of P and P^2 over the M short spectra of a row, and the estimator
//   SK = (M + 1) / (M - 1) * (M * S2 / S1^2 - 1)
// of Nita & Gary -- gj_sk_dev / gj_sk_rows / gj_sk_workspace of include/gpsjam.h, which states the definition.
// Gaussian noise gives 1 whatever its level or the passband's shape, a steady carrier pulls its bin toward 0 and
// anything intermittent pushes it above 1 (gpsjam/kurtosis.py reads it).
//
// The transform front end -- the workgroup of transform groups, the loads, the window, the passes and their exchange
// barrier -- is stft_group.h, shared with k_ridge.hip and k_excise.hip.  What is the kurtosis's own:
//   * a transform group, not a workgroup, is the unit of work: it takes one BLOCK of a row, a run of up to kSkMaxRun
//     consecutive frames, and keeps 16 + 16 accumulators in registers for sum P and sum P^2 of its 16 bins.  Nothing
//     is reduced across lanes: a bin belongs to one thread;
//   * powers are accumulated in LSB units (scale^2 and scale^4 are applied at the end; the worst case, a full-scale
//     tone at 4096 points over 65536 frames, sums P^2 to about 1e27);
//   * a block ends with one partial pair, float32[2][N], in the workspace; a second small launch adds a row's partials
//     in block order, scales, and evaluates SK in double from the rounded float32 sums.
// The partition is a function of (N, M) alone -- sk_blocks below -- never of the number of rows, the grid or the device:
// a capture with few rows still spreads over M / kSkMaxRun times as many groups.
// Determinism: a block's partial is computed by ONE group from that block's bytes alone, frame by frame in order, by the
// same instructions whichever group, workgroup or launch takes it; the second launch adds the partials of a row in
// block order.  A row is therefore bit-identical wherever it lies in a call and whatever else the call computes.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it
// (tests/hip_stub builds those by name), and K2's module is compiled exactly as before.
#include "stft_group.h"

#include <cmath>

namespace gj {

constexpr int kSkMaxRun = 16;       // frames per block at most: a partial pair (8 N bytes) per 32 N bytes read at hop = N
constexpr int kSkMaxFrames = 65536; // frames per row at most

// blocks of a row and frames per block (the last block may be shorter, never empty: (nb - 1) * run < M)
struct SkBlocks {
    unsigned nb, run;
};
inline SkBlocks sk_blocks(int frames_per_row) {
    const unsigned M = (unsigned)frames_per_row;
    const unsigned nb = (M + kSkMaxRun - 1) / kSkMaxRun;
    return SkBlocks{nb, (M + nb - 1) / nb};
}

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
    unsigned long long first_sample, hop, n_units, nsteps, last_frame;
    unsigned frames_per_row, nb, run;
    float neg_off;   // -offset of the unpack convention
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
    const c2 koff = make_c2(g.neg_off, g.neg_off);

    // This group's block in workgroup step `step`: its first frame and how many frames it holds.  A group behind the
    // last block holds none; it walks the call's last block again so that every load stays inside the capture, and every
    // group of the grid makes g.run iterations per step (the barriers of the large sizes are workgroup-wide).
    auto block_of = [&](unsigned long long step, unsigned& count) {
        unsigned long long u = step * B + (unsigned)b;
        const bool valid = u < g.n_units;
        if (!valid) u = g.n_units - 1;
        const unsigned long long r = u / g.nb;
        const unsigned j = (unsigned)(u - r * g.nb);
        const unsigned rest = g.frames_per_row - j * g.run;
        count = valid ? (rest < g.run ? rest : g.run) : 0u;
        return r * g.frames_per_row + (unsigned long long)j * g.run;
    };
    auto frame_base = [&](unsigned long long f) {
        if (f > g.last_frame) f = g.last_frame;   // a short block's spare iterations
        return iq + 2ull * (g.first_sample + f * g.hop);
    };
    auto load_frame = [&](unsigned (&dst)[16], const uint8_t* base) { stft_load_frame<N, Cfg::wide_load>(dst, base, jl0); };

    unsigned raw[16];   // the NEXT frame's samples are fetched while the current ones are transformed
    unsigned long long step = blockIdx.x;   // the grid never exceeds nsteps
    unsigned count = 0;
    unsigned long long f0 = block_of(step, count);
    load_frame(raw, frame_base(f0));
    for (; step < g.nsteps; step += gridDim.x) {
        const bool more = step + gridDim.x < g.nsteps;   // workgroup-uniform
        unsigned next_count = 0;
        const unsigned long long next_f0 = more ? block_of(step + gridDim.x, next_count) : 0ull;
        float s1[16], s2[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) s1[s] = s2[s] = 0.f;

        for (unsigned i = 0; i < g.run; ++i) {
            c2 v[16];
            stft_unpack_window(v, raw, wp, koff);
            if (i + 1 < g.run) load_frame(raw, frame_base(f0 + i + 1));
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

// bytes of partial sums for n_rows rows; 0 when the product does not fit a size_t
static size_t sk_workspace_bytes(int nfft, int frames_per_row, size_t n_rows) {
    size_t units = 0, bytes = 0;
    if (__builtin_mul_overflow(n_rows, (size_t)sk_blocks(frames_per_row).nb, &units)) return 0;
    if (__builtin_mul_overflow(units, (size_t)nfft * 2 * sizeof(float), &bytes)) return 0;
    return bytes;
}

template <int N>
static void sk_launch(gj_ctx* ctx, const uint8_t* d_iq, SkGeom g, float* partial) {
    constexpr unsigned long long B = kBlockPoints / N;
    g.nsteps = (g.n_units + B - 1) / B;
    const unsigned grid = stft_one_round_grid(ctx, SkCfg<N>::min_waves, g.nsteps);
    hipLaunchKernelGGL(sk_kernel<N>, dim3(grid), dim3(kBlockThreads), 0, ctx->stream, d_iq, g, ctx->d_twiddle, window_table(ctx, N),
                       partial);
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_sk_rows(size_t nbytes, size_t first_sample, int nfft, size_t hop, int frames_per_row) {
    const size_t total = nbytes / 2;
    if (nfft < 1 || hop < 1 || frames_per_row < 1 || first_sample > total || total - first_sample < (size_t)nfft) return 0;
    return ((total - first_sample - (size_t)nfft) / hop + 1) / (size_t)frames_per_row;
}

size_t gj_sk_workspace(gj_ctx* ctx, int nfft, int frames_per_row, size_t n_rows) {
    (void)ctx;
    if (!stft_nfft_ok(nfft) || frames_per_row < 2 || frames_per_row > kSkMaxFrames) return 0;
    return sk_workspace_bytes(nfft, frames_per_row, n_rows);
}

int gj_sk_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, int nfft, size_t hop, int frames_per_row,
              size_t n_rows, float* d_s1, float* d_s2, float* d_sk) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (frames_per_row < 2) return fail(ctx, GJ_ERR_INVALID, "frames_per_row must be >= 2");
    if (frames_per_row > kSkMaxFrames) return fail(ctx, GJ_ERR_UNSUPPORTED, "frames_per_row must be <= %d", kSkMaxFrames);
    if (!d_iq || !d_s1 || !d_s2) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = stft_check_capture(ctx, d_iq)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_s1) | reinterpret_cast<uintptr_t>(d_s2) | reinterpret_cast<uintptr_t>(d_sk)) & 3)
        return fail(ctx, GJ_ERR_INVALID, "outputs must be 4-byte aligned");
    if (hop < 1) return fail(ctx, GJ_ERR_INVALID, "hop must be >= 1");
    const size_t fit = gj_sk_rows(nbytes, first_sample, nfft, hop, frames_per_row);
    if (n_rows == 0 || n_rows > fit)
        return fail(ctx, GJ_ERR_INVALID, "n_rows %zu: 1..%zu rows of %d frames of %d points fit from sample %zu at hop %zu", n_rows, fit,
                    frames_per_row, nfft, first_sample, hop);
    const size_t need = sk_workspace_bytes(nfft, frames_per_row, n_rows);
    if (!need) return fail(ctx, GJ_ERR_NOMEM, "the partial sums of %zu rows do not fit the address space", n_rows);
    int rc = ensure_workspace(ctx, need);
    if (rc) return rc;
    float* partial = reinterpret_cast<float*>(ctx->ws);
    const SkBlocks blk = sk_blocks(frames_per_row);
    SkGeom g;
    g.first_sample = first_sample;
    g.hop = hop;
    g.n_units = (unsigned long long)n_rows * blk.nb;
    g.nsteps = 0;
    g.last_frame = (unsigned long long)n_rows * (unsigned)frames_per_row - 1;
    g.frames_per_row = (unsigned)frames_per_row;
    g.nb = blk.nb;
    g.run = blk.run;
    g.neg_off = -0.5f * (float)ctx->off2;
    stft_dispatch(nfft, [&](auto n) { sk_launch<decltype(n)::value>(ctx, d_iq, g, partial); });
    GJ_LAUNCH_CHECK(ctx);
    const unsigned long long n_out = (unsigned long long)n_rows * (unsigned)nfft;
    const unsigned long long want = (n_out + 255) / 256, cap = (unsigned long long)ctx->num_cus * 32;
    const double sc2 = ctx->scale * ctx->scale;
    hipLaunchKernelGGL(sk_finalize_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, ctx->stream, partial, n_out, nfft, blk.nb,
                       sc2, sc2 * sc2, (double)frames_per_row, d_s1, d_s2, d_sk);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
