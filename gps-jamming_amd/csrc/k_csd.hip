// Cross-spectral density of a capture pair (gfx950): per bin the sums over the M short spectra of a row of |A|^2, |B|^2
// and B conj(A), and the magnitude-squared coherence
//   MSC = |Sab|^2 / (Saa Sbb)
// -- gj_csd_dev / gj_csd_rows / gj_csd_workspace of include/gpsjam.h, which states the definition and the sign.  Two
// antennas see the same jammer under independent receiver noise: MSC is about 1 / M under noise alone and
// (rho / (1 + rho))^2 in a bin of jammer-to-noise ratio rho, and the phase of Sab carries the delay of that band
// (gpsjam/coherence.py reads both).
//
// This is sk_kernel (k_skurt.hip) with two captures and four accumulators per bin, on the front end of stft_group.h:
//   * a transform group takes one BLOCK of a row, a run of up to kRowMaxRun consecutive frame PAIRS.  Per pair it
//     transforms a's frame and keeps its 16 bins in registers, transforms b's frame through the same LDS buffer (the
//     front end's exchange ends with a barrier behind the gather, so the buffer is free again), and accumulates.  A bin
//     belongs to the same thread in both transforms: nothing is reduced across lanes;
//   * the sums run in LSB units (scale^2 is applied at the end);
//   * a block ends with one partial, float32[4][N] (Saa, Sbb, re, im), in the workspace; a second small launch adds a
//     row's partials in block order, scales, and evaluates MSC in double from the rounded float32 values.
// Rows, blocks, the partition rule and the determinism that rests on it are stft_rows.h, shared with k_skurt.hip.  Here
// Saa's accumulator sees a's bins only and Sbb's b's only, so each depends on its own capture's bytes alone.
//
// A translation unit of its own with its own extern "C" entry points; no other source refers to it.
#include "stft_rows.h"

#include <cmath>

namespace gj {

// Im(B conj(A)) as the difference of two ROUNDED products, never contracted into a fused multiply-add: the form is
// antisymmetric in (a, b), so swapping the captures conjugates Sab bit for bit and a capture against itself has no
// imaginary part at all.  (The real part and the powers are symmetric as fused forms already.)
__device__ __forceinline__ float csd_cross_im(c2 b, c2 a) {
#pragma clang fp contract(off)
    const float p = b.y * a.x, q = b.x * a.y;
    return p - q;
}

template <int N>
struct CsdCfg {
    // 64 accumulators, 32 held bins, 32 working bins, 32 prefetched samples, the window and one or two twiddle sets: past
    // the 168 registers of three workgroups per CU at every size.  Two workgroups per CU (256 registers) hold all of it
    // without a spill up to 512 points (255 registers there); from 1024 points on, where the second twiddle set is fully
    // used, two per CU would spill and one workgroup per CU replaces the spill (profiles/NOTES_csd.md has the compiler's
    // figures)
    static constexpr int min_waves = N >= 1024 ? 1 : 2;
    static constexpr bool xpose = N == 4096;       // the conflict-free exchange schedule of fft_core.h (X4096)
    static constexpr bool wide_load = N <= 32;     // as SkCfg
};

struct CsdGeom {
    unsigned long long first_a, first_b;
    RowGeom rows;
};

template <int N>
__global__ __launch_bounds__(kBlockThreads, CsdCfg<N>::min_waves) void csd_kernel(const uint8_t* __restrict__ iq_a,
                                                                                  const uint8_t* __restrict__ iq_b, CsdGeom g,
                                                                                  const cf* __restrict__ twtab,
                                                                                  const float* __restrict__ wintab,
                                                                                  float* __restrict__ partial) {
    using Cfg = CsdCfg<N>;
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
    auto frame_at = [&](unsigned long long f) { return row_clamp_frame(g.rows, f) * g.rows.hop; };
    auto load_frame = [&](unsigned (&dst)[16], const uint8_t* base) { stft_load_frame<N, Cfg::wide_load>(dst, base, jl0); };
    auto transform = [&](c2 (&v)[16]) {
        if constexpr (XP) stft_passes_x4096(v, lds0, tid, tw, ktw);
        else stft_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);
    };
    const uint8_t* const base_a = iq_a + 2ull * g.first_a;
    const uint8_t* const base_b = iq_b + 2ull * g.first_b;

    unsigned raw_a[16], raw_b[16];   // the NEXT pair's samples are fetched while the current ones are transformed
    unsigned long long step = blockIdx.x;   // the grid never exceeds nsteps
    unsigned count = 0;
    unsigned long long f0 = block_of(step, count);
    load_frame(raw_a, base_a + 2ull * frame_at(f0));
    load_frame(raw_b, base_b + 2ull * frame_at(f0));
    for (; step < g.rows.nsteps; step += gridDim.x) {
        const bool more = step + gridDim.x < g.rows.nsteps;   // workgroup-uniform
        unsigned next_count = 0;
        const unsigned long long next_f0 = more ? block_of(step + gridDim.x, next_count) : 0ull;
        float saa[16], sbb[16], sre[16], sim[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) saa[s] = sbb[s] = sre[s] = sim[s] = 0.f;

        for (unsigned i = 0; i < g.rows.run; ++i) {
            const bool within = i + 1 < g.rows.run;
            const unsigned long long next_at = frame_at(within ? f0 + i + 1 : next_f0);

            c2 a[16];
            stft_unpack_window(a, raw_a, wp, koff);
            if (within || more) load_frame(raw_a, base_a + 2ull * next_at);
            transform(a);

            c2 v[16];
            stft_unpack_window(v, raw_b, wp, koff);
            if (within || more) load_frame(raw_b, base_b + 2ull * next_at);
            transform(v);

            // this thread's bins jl + TF s of both.  A spare iteration adds zeros: the sums keep their bits.
            const bool counted = i < count;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float pa = counted ? fmaf(a[s].x, a[s].x, a[s].y * a[s].y) : 0.f;
                const float pb = counted ? fmaf(v[s].x, v[s].x, v[s].y * v[s].y) : 0.f;
                const float re = counted ? fmaf(v[s].x, a[s].x, v[s].y * a[s].y) : 0.f;    // B conj(A)
                const float im = counted ? csd_cross_im(v[s], a[s]) : 0.f;
                saa[s] += pa;
                sbb[s] += pb;
                sre[s] += re;
                sim[s] += im;
            }
        }

        if (count) {   // this group holds a block: its partial, [4][N] in FFT order
            float* dst = partial + (step * B + (unsigned)b) * (4ull * N) + jl;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                dst[TF * s] = saa[s];
                dst[N + TF * s] = sbb[s];
                dst[2 * N + TF * s] = sre[s];
                dst[3 * N + TF * s] = sim[s];
            }
        }
        f0 = next_f0;
        count = next_count;
    }
}

// A row's partials added in block order, scaled to the units of gj_sk_dev's S1, and MSC in double from the ROUNDED
// values (what the caller can recompute from the three outputs), rounded once.
__global__ __launch_bounds__(256) void csd_finalize_kernel(const float* __restrict__ partial, unsigned long long n_out, int n, unsigned nb,
                                                           double scale2, float* __restrict__ saa, float* __restrict__ sbb,
                                                           float2* __restrict__ sab, float* __restrict__ msc) {
    for (unsigned long long at = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; at < n_out;
         at += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long r = at / (unsigned)n;
        const unsigned k = (unsigned)(at - r * (unsigned)n);
        const float* p = partial + r * nb * (4ull * n) + k;
        float a = p[0], c = p[n], re = p[2 * n], im = p[3 * n];
        for (unsigned j = 1; j < nb; ++j) {
            p += 4 * n;
            a += p[0];
            c += p[n];
            re += p[2 * n];
            im += p[3 * n];
        }
        const float fa = (float)((double)a * scale2), fb = (float)((double)c * scale2);
        const float fr = (float)((double)re * scale2), fi = (float)((double)im * scale2);
        saa[at] = fa;
        sbb[at] = fb;
        sab[at] = make_float2(fr, fi);
        if (msc) {
            const double den = (double)fa * (double)fb;
            msc[at] = den == 0.0 ? __builtin_nanf("") : (float)(((double)fr * (double)fr + (double)fi * (double)fi) / den);
        }
    }
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_csd_rows(size_t nbytes_a, size_t first_a, size_t nbytes_b, size_t first_b, int nfft, size_t hop, int frames_per_row) {
    const size_t ra = row_fit(nbytes_a, first_a, nfft, hop, frames_per_row);
    const size_t rb = row_fit(nbytes_b, first_b, nfft, hop, frames_per_row);
    return ra < rb ? ra : rb;
}

size_t gj_csd_workspace(gj_ctx* ctx, int nfft, int frames_per_row, size_t n_rows) {
    (void)ctx;
    return row_workspace_bytes(4, nfft, frames_per_row, n_rows);
}

int gj_csd_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b, size_t nbytes_b, size_t first_b,
               int nfft, size_t hop, int frames_per_row, size_t n_rows, float* d_saa, float* d_sbb, float* d_sab, float* d_msc) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = row_check_shape(ctx, nfft, frames_per_row)) return rc;
    if (!d_a || !d_b || !d_saa || !d_sbb || !d_sab) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = stft_check_capture(ctx, d_a)) return rc;
    if (int rc = stft_check_capture(ctx, d_b)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_saa) | reinterpret_cast<uintptr_t>(d_sbb) | reinterpret_cast<uintptr_t>(d_msc)) & 3)
        return fail(ctx, GJ_ERR_INVALID, "d_saa, d_sbb and d_msc must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_sab) & 7) return fail(ctx, GJ_ERR_INVALID, "d_sab must be 8-byte aligned");
    if (hop < 1) return fail(ctx, GJ_ERR_INVALID, "hop must be >= 1");
    const size_t fit = gj_csd_rows(nbytes_a, first_a, nbytes_b, first_b, nfft, hop, frames_per_row);
    if (n_rows == 0 || n_rows > fit)
        return fail(ctx, GJ_ERR_INVALID, "n_rows %zu: 1..%zu rows of %d frames of %d points fit both captures from samples %zu and %zu at hop %zu",
                    n_rows, fit, frames_per_row, nfft, first_a, first_b, hop);
    float* partial = nullptr;
    if (int rc = row_workspace(ctx, 4, nfft, frames_per_row, n_rows, &partial)) return rc;
    const CsdGeom g{first_a, first_b, row_geom(ctx, hop, frames_per_row, n_rows)};
    stft_dispatch(nfft, [&](auto n) {
        constexpr int N = decltype(n)::value;
        row_launch<N>(ctx, csd_kernel<N>, CsdCfg<N>::min_waves, g, partial, d_a, d_b);
    });
    GJ_LAUNCH_CHECK(ctx);
    const unsigned long long n_out = (unsigned long long)n_rows * (unsigned)nfft;
    hipLaunchKernelGGL(csd_finalize_kernel, dim3(row_finalize_grid(ctx, n_out)), dim3(256), 0, ctx->stream, partial, n_out, nfft, g.rows.nb,
                       ctx->scale * ctx->scale, d_saa, d_sbb, reinterpret_cast<float2*>(d_sab), d_msc);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
