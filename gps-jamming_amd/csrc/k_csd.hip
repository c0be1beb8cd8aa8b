// Cross-spectral density of a capture pair (gfx950): per bin the sums over the M short spectra of a row of |A|^2, |B|^2
// and B conj(A), and the magnitude-squared coherence
//   MSC = |Sab|^2 / (Saa Sbb)
// -- gj_csd_dev / gj_csd_rows / gj_csd_workspace of include/gpsjam.h, which states the definition and the sign.  Two
// antennas see the same jammer under independent receiver noise: MSC is about 1 / M under noise alone and
// (rho / (1 + rho))^2 in a bin of jammer-to-noise ratio rho, and the phase of Sab carries the delay of that band
// (gpsjam/coherence.py reads both).
//
// This is sk_kernel (k_skurt.hip) with two captures and four accumulators per bin, on the front end of stft_group.h:
//   * a transform group takes one BLOCK of a row, a run of up to kCsdMaxRun consecutive frame PAIRS.  Per pair it
//     transforms a's frame and keeps its 16 bins in registers, transforms b's frame through the same LDS buffer (the
//     front end's exchange ends with a barrier behind the gather, so the buffer is free again), and accumulates.  A bin
//     belongs to the same thread in both transforms: nothing is reduced across lanes;
//   * the sums run in LSB units (scale^2 is applied at the end);
//   * a block ends with one partial, float32[4][N] (Saa, Sbb, re, im), in the workspace; a second small launch adds a
//     row's partials in block order, scales, and evaluates MSC in double from the rounded float32 values.
// The partition is gj_sk_dev's: a function of M alone (csd_blocks below).  Determinism as there: a block's partial is
// computed by ONE group from that block's bytes alone, pair by pair in order; Saa's accumulator sees a's bins only and
// Sbb's b's only, so each depends on its own capture's bytes alone.
//
// A translation unit of its own with its own extern "C" entry points; no other source refers to it.
#include "stft_group.h"

#include <cmath>

namespace gj {

constexpr int kCsdMaxRun = 16;       // frame pairs per block at most (k_skurt.hip kSkMaxRun: the same rule)
constexpr int kCsdMaxFrames = 65536; // frames per row at most

// blocks of a row and frame pairs per block (the last block may be shorter, never empty)
struct CsdBlocks {
    unsigned nb, run;
};
inline CsdBlocks csd_blocks(int frames_per_row) {
    const unsigned M = (unsigned)frames_per_row;
    const unsigned nb = (M + kCsdMaxRun - 1) / kCsdMaxRun;
    return CsdBlocks{nb, (M + nb - 1) / nb};
}

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
    unsigned long long first_a, first_b, hop, n_units, nsteps, last_frame;
    unsigned frames_per_row, nb, run;
    float neg_off;   // -offset of the unpack convention
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
    const c2 koff = make_c2(g.neg_off, g.neg_off);

    // This group's block in workgroup step `step`, as sk_kernel's: its first frame and how many pairs it holds.  A group
    // behind the last block holds none; it walks the call's last block again so that every load stays inside both
    // captures, and every group of the grid makes g.run iterations per step (the barriers of the large sizes are
    // workgroup-wide).
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
    auto frame_at = [&](unsigned long long f) {   // a short block's spare iterations read the call's last frame
        return (f > g.last_frame ? g.last_frame : f) * g.hop;
    };
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
    for (; step < g.nsteps; step += gridDim.x) {
        const bool more = step + gridDim.x < g.nsteps;   // workgroup-uniform
        unsigned next_count = 0;
        const unsigned long long next_f0 = more ? block_of(step + gridDim.x, next_count) : 0ull;
        float saa[16], sbb[16], sre[16], sim[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) saa[s] = sbb[s] = sre[s] = sim[s] = 0.f;

        for (unsigned i = 0; i < g.run; ++i) {
            const bool within = i + 1 < g.run;
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

// bytes of partial sums for n_rows rows; 0 when the product does not fit a size_t
static size_t csd_workspace_bytes(int nfft, int frames_per_row, size_t n_rows) {
    size_t units = 0, bytes = 0;
    if (__builtin_mul_overflow(n_rows, (size_t)csd_blocks(frames_per_row).nb, &units)) return 0;
    if (__builtin_mul_overflow(units, (size_t)nfft * 4 * sizeof(float), &bytes)) return 0;
    return bytes;
}

// whole rows of one capture (gj_sk_rows' arithmetic)
static size_t csd_rows_of(size_t nbytes, size_t first, int nfft, size_t hop, int frames_per_row) {
    const size_t total = nbytes / 2;
    if (nfft < 1 || hop < 1 || frames_per_row < 1 || first > total || total - first < (size_t)nfft) return 0;
    return ((total - first - (size_t)nfft) / hop + 1) / (size_t)frames_per_row;
}

template <int N>
static void csd_launch(gj_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, CsdGeom g, float* partial) {
    constexpr unsigned long long B = kBlockPoints / N;
    g.nsteps = (g.n_units + B - 1) / B;
    const unsigned grid = stft_one_round_grid(ctx, CsdCfg<N>::min_waves, g.nsteps);
    hipLaunchKernelGGL(csd_kernel<N>, dim3(grid), dim3(kBlockThreads), 0, ctx->stream, d_a, d_b, g, ctx->d_twiddle, window_table(ctx, N),
                       partial);
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_csd_rows(size_t nbytes_a, size_t first_a, size_t nbytes_b, size_t first_b, int nfft, size_t hop, int frames_per_row) {
    const size_t ra = csd_rows_of(nbytes_a, first_a, nfft, hop, frames_per_row);
    const size_t rb = csd_rows_of(nbytes_b, first_b, nfft, hop, frames_per_row);
    return ra < rb ? ra : rb;
}

size_t gj_csd_workspace(gj_ctx* ctx, int nfft, int frames_per_row, size_t n_rows) {
    (void)ctx;
    if (!stft_nfft_ok(nfft) || frames_per_row < 2 || frames_per_row > kCsdMaxFrames) return 0;
    return csd_workspace_bytes(nfft, frames_per_row, n_rows);
}

int gj_csd_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b, size_t nbytes_b, size_t first_b,
               int nfft, size_t hop, int frames_per_row, size_t n_rows, float* d_saa, float* d_sbb, float* d_sab, float* d_msc) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (frames_per_row < 2) return fail(ctx, GJ_ERR_INVALID, "frames_per_row must be >= 2");
    if (frames_per_row > kCsdMaxFrames) return fail(ctx, GJ_ERR_UNSUPPORTED, "frames_per_row must be <= %d", kCsdMaxFrames);
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
    const size_t need = csd_workspace_bytes(nfft, frames_per_row, n_rows);
    if (!need) return fail(ctx, GJ_ERR_NOMEM, "the partial sums of %zu rows do not fit the address space", n_rows);
    int rc = ensure_workspace(ctx, need);
    if (rc) return rc;
    float* partial = reinterpret_cast<float*>(ctx->ws);
    const CsdBlocks blk = csd_blocks(frames_per_row);
    CsdGeom g;
    g.first_a = first_a;
    g.first_b = first_b;
    g.hop = hop;
    g.n_units = (unsigned long long)n_rows * blk.nb;
    g.nsteps = 0;
    g.last_frame = (unsigned long long)n_rows * (unsigned)frames_per_row - 1;
    g.frames_per_row = (unsigned)frames_per_row;
    g.nb = blk.nb;
    g.run = blk.run;
    g.neg_off = -0.5f * (float)ctx->off2;
    stft_dispatch(nfft, [&](auto n) { csd_launch<decltype(n)::value>(ctx, d_a, d_b, g, partial); });
    GJ_LAUNCH_CHECK(ctx);
    const unsigned long long n_out = (unsigned long long)n_rows * (unsigned)nfft;
    const unsigned long long want = (n_out + 255) / 256, cap = (unsigned long long)ctx->num_cus * 32;
    hipLaunchKernelGGL(csd_finalize_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, ctx->stream, partial, n_out, nfft, blk.nb,
                       ctx->scale * ctx->scale, d_saa, d_sbb, reinterpret_cast<float2*>(d_sab), d_msc);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
