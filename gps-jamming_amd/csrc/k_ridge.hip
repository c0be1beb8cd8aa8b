// Short-time spectral ridge (gfx950): per short frame the spectral peak, its bin, the power outside a guard band around
// it and the frame's total power -- gj_ridge_dev / gj_ridge_frames of include/gpsjam.h, which states the definition.
// The time series tells the four interferers of the reference's simulator apart (simulate/frontend/jammers/:
// cwJammer.py, chirpJammer.py, pulsedJammer.py, broadbandJammer.py; gpsjam/classify.py reads it).
//
// The transform is K2's (k_welch.hip): one 256-thread workgroup transforms 4096 points = 4096/N frames per step, every
// thread pulls its 16 samples straight from the uint8 stream, applies unpack and the periodic Hann window of K2's table
// and runs the register-resident Stockham passes of fft_core.h with LDS exchanges.  What differs:
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
#include "gj_common.h"

#include <climits>

namespace gj {

extern const float* window_table(gj_ctx* ctx, int n);   // api.hip: K2's periodic Hann tables

template <int N>
struct RidgeCfg {
    // as K2 (WelchCfg): three workgroups per CU from 32 points on, one LDS buffer with two syncs per exchange
    static constexpr int min_waves = N >= 32 ? 3 : 2;
    static constexpr bool xpose = N == 4096;       // the conflict-free exchange schedule of fft_core.h (X4096)
    // 16 and 32 points fetch the frame with 16-byte loads and pick the thread's samples out of the registers; from 64
    // points on that needs a run-time choice between registers and is slower than 2-byte loads (k_welch.hip, wide_load)
    static constexpr bool wide_load = N <= 32;
};

struct RidgeGeom {
    unsigned long long first_sample, hop, n_frames, nsteps;
    float neg_off;   // -offset of the unpack convention
    float scale2;    // scale^2: the transform runs on u8 - offset, the three powers are scaled at the end
    int guard;
};

// Reduction of `v` over each aligned group of G lanes (power of two, 1..64), result in every lane of the group: the
// DPP steps of group_sum_dpp_f (gj_common.h) inside a row of 16, shuffles across rows.  `op` must be commutative: lane
// pairs then compute op(a, b) and op(b, a) and stay bit-identical.
template <int G, typename Op>
__device__ __forceinline__ float group_reduce_f(float v, Op op) {
#define GJ_DPP_F(x, ctrl) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, 0xf, 0xf, false))
    if constexpr (G >= 2) v = op(v, GJ_DPP_F(v, 0xB1));     // quad_perm [1,0,3,2]
    if constexpr (G >= 4) v = op(v, GJ_DPP_F(v, 0x4E));     // quad_perm [2,3,0,1]
    if constexpr (G >= 8) v = op(v, GJ_DPP_F(v, 0x141));    // row_half_mirror
    if constexpr (G >= 16) v = op(v, GJ_DPP_F(v, 0x140));   // row_mirror
#undef GJ_DPP_F
    if constexpr (G >= 32) v = op(v, __shfl_xor(v, 16, 64));
    if constexpr (G >= 64) v = op(v, __shfl_xor(v, 32, 64));
    return v;
}
template <int G>
__device__ __forceinline__ int group_min_i(int v) {
#define GJ_DPP_I(x, ctrl) __builtin_amdgcn_update_dpp(0, x, ctrl, 0xf, 0xf, false)
    if constexpr (G >= 2) v = min(v, GJ_DPP_I(v, 0xB1));
    if constexpr (G >= 4) v = min(v, GJ_DPP_I(v, 0x4E));
    if constexpr (G >= 8) v = min(v, GJ_DPP_I(v, 0x141));
    if constexpr (G >= 16) v = min(v, GJ_DPP_I(v, 0x140));
#undef GJ_DPP_I
    if constexpr (G >= 32) v = min(v, __shfl_xor(v, 16, 64));
    if constexpr (G >= 64) v = min(v, __shfl_xor(v, 32, 64));
    return v;
}

// The exchange barrier, as K2's welch_exchange_sync: up to 1024 points a transform's N / 16 threads lie inside one wave,
// whose LDS instructions execute in issue order -- a wavefront fence keeps the compiler from reordering scatter and
// gather; larger transforms span waves and take the workgroup barrier.
template <int N>
__device__ __forceinline__ void ridge_exchange_sync() {
    if constexpr (N / 16 <= 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

template <int N, int PASS>
__device__ __forceinline__ void ridge_passes(c2 (&v)[16], cf* lds, int base, int jl, const c2 (&tw)[3][15], const InnerTw& ktw) {
    fft_pass<N, PASS, true>(v, tw[PASS], ktw);
    if constexpr (PASS + 1 < fft_npass(N)) {
        lds_scatter<N, PASS>(v, lds, base, jl);
        ridge_exchange_sync<N>();
        lds_gather<N>(v, lds, base, jl);
        ridge_exchange_sync<N>();
        ridge_passes<N, PASS + 1>(v, lds, base, jl, tw, ktw);
    }
}

// 4096 points: pass 0 in role jl0 = tid, passes 1 and 2 in role jl1 (fft_core.h, X4096)
__device__ __forceinline__ void ridge_passes_x4096(c2 (&v)[16], cf* lds, int tid, const c2 (&tw)[3][15], const InnerTw& ktw) {
    fft_pass<4096, 0, true>(v, tw[0], ktw);
    x4096_scatter<0>(v, lds, tid);
    __syncthreads();
    x4096_gather<0>(v, lds, tid);
    __syncthreads();
    fft_pass<4096, 1, true>(v, tw[1], ktw);
    x4096_scatter<1>(v, lds, tid);
    __syncthreads();
    x4096_gather<1>(v, lds, tid);
    __syncthreads();
    fft_pass<4096, 2, true>(v, tw[2], ktw);
}

template <int N>
__global__ __launch_bounds__(kBlockThreads, RidgeCfg<N>::min_waves) void ridge_kernel(const uint8_t* __restrict__ iq, RidgeGeom g,
                                                                                      const cf* __restrict__ twtab,
                                                                                      const float* __restrict__ wintab,
                                                                                      gj_ridge_frame* __restrict__ out) {
    using Cfg = RidgeCfg<N>;
    constexpr int TF = N / 16, B = kBlockPoints / N, NP = fft_npass(N);
    constexpr int WPF = (TF >= 64) ? TF / 64 : 1;   // waves per transform
    constexpr bool XP = Cfg::xpose;
    constexpr int SPAN = XP ? X4096::kSpan : lds_span(kBlockPoints);
    __shared__ cf lds0[NP > 1 ? SPAN : 1];
    // wave results of a transform group that spans waves (2048, 4096 points); one array per reduction, so that a wave
    // that is ahead never overwrites what a slower one still reads (the next step's writes lie behind the exchange
    // barriers of its transform)
    constexpr int RB = WPF > 1 ? B : 1;
    __shared__ float red_sum[RB][WPF], red_max[RB][WPF], red_sec[RB][WPF];
    __shared__ int red_bin[RB][WPF];
    // what the wave fence rests on (k_welch.hip): a transform group is an aligned fraction of ONE wave
    static_assert(TF > 64 || (64 % TF == 0 && WPF == 1 && kBlockThreads % 64 == 0 && B * TF == kBlockThreads),
                  "the wave-fence exchange needs a transform group inside one wave");
    const int tid = threadIdx.x;
    const int b = (TF >= 64) ? __builtin_amdgcn_readfirstlane(tid / TF) : tid / TF;
    const int jl0 = tid % TF;                    // butterfly of pass 0 (input index jl0 + TF s)
    const int jl = XP ? X4096::jl1(tid) : jl0;   // butterfly of the later passes = bins held at the end: jl + TF s

    const InnerTw ktw = inner_twiddles();
    c2 tw[3][15];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int k = 0; k < 15; ++k) tw[p][k] = make_c2(1.f, 0.f);
    if constexpr (NP > 1) load_twiddles<N, 1>(tw[1], twtab, jl);
    if constexpr (NP > 2) load_twiddles<N, 2>(tw[2], twtab, jl);

    c2 wp[8];   // (w[2i], w[2i+1]) share a register pair, op_sel picks the half
#pragma unroll
    for (int s = 0; s < 8; ++s) wp[s] = make_c2(wintab[jl0 + TF * (2 * s)], wintab[jl0 + TF * (2 * s + 1)]);
    const c2 koff = make_c2(g.neg_off, g.neg_off);

    const unsigned long long last = g.n_frames - 1;
    // a group without a frame (behind the last one) transforms the last frame again: every load stays inside the capture
    auto frame_base = [&](unsigned long long step) {
        unsigned long long f = step * B + (unsigned)b;
        if (f > last) f = last;
        return iq + 2ull * (g.first_sample + f * g.hop);
    };
    auto load_frame = [&](unsigned (&dst)[16], const uint8_t* base) {
        if constexpr (Cfg::wide_load) {
            // the whole frame (2 N bytes) in 16-byte loads; sample jl0 + TF s is one half of dword (jl0 + TF s) / 2.
            // The frame is only 2-byte aligned: global memory takes unaligned vector loads.
            struct __attribute__((packed, aligned(2))) Vec16 { unsigned x, y, z, w; };
            constexpr int NV = 2 * N / 16;
            const Vec16* src = reinterpret_cast<const Vec16*>(base);
            unsigned w[4 * NV];
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const Vec16 t = src[q];
                w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                if constexpr (TF == 1) dst[s] = (s & 1) ? (w[s >> 1] >> 16) : (w[s >> 1] & 0xffffu);
                else dst[s] = (w[s] >> (16u * (unsigned)jl0)) & 0xffffu;
            }
        } else {
            const uint8_t* p = base + 2 * jl0;
#pragma unroll
            for (int s = 0; s < 16; ++s) dst[s] = *reinterpret_cast<const uint16_t*>(p + 2 * TF * s);
        }
    };

    unsigned raw[16];   // the NEXT step's samples are fetched while the current ones are transformed
    unsigned long long step = blockIdx.x;   // the grid never exceeds nsteps
    load_frame(raw, frame_base(step));
    for (; step < g.nsteps; step += gridDim.x) {
        const unsigned long long f = step * B + (unsigned)b;
        const bool active = f <= last;
        c2 v[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const unsigned u = raw[s];
            const c2 x = cadd(make_c2((float)(u & 255u), (float)((u >> 8) & 255u)), koff);   // exact: u8 minus a multiple of 0.5
            v[s] = (s & 1) ? scale_hi(x, wp[s >> 1]) : scale_lo(x, wp[s >> 1]);
        }
        if (step + gridDim.x < g.nsteps) load_frame(raw, frame_base(step + gridDim.x));   // workgroup-uniform

        if constexpr (XP) ridge_passes_x4096(v, lds0, tid, tw, ktw);
        else ridge_passes<N, 0>(v, lds0, b * lds_span(N), jl, tw, ktw);

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
        constexpr int G = TF >= 64 ? 64 : TF;
        const auto add = [](float a, float c) { return a + c; };
        const auto fmx = [](float a, float c) { return fmaxf(a, c); };
        tot = group_reduce_f<G>(tot, add);
        float gmx = group_reduce_f<G>(mx, fmx);
        [[maybe_unused]] const int wv = (tid >> 6) % WPF;
        if constexpr (WPF > 1) {
            if ((tid & 63) == 0) { red_sum[b][wv] = tot; red_max[b][wv] = gmx; }
            __syncthreads();
            tot = red_sum[b][0]; gmx = red_max[b][0];
#pragma unroll
            for (int k = 1; k < WPF; ++k) { tot += red_sum[b][k]; gmx = fmaxf(gmx, red_max[b][k]); }
        }
        // smallest bin that attains the maximum: within a thread it is the thread's first such slot
        int bin = group_min_i<G>(mx == gmx ? jl + TF * ms : INT_MAX);
        if constexpr (WPF > 1) {
            if ((tid & 63) == 0) red_bin[b][wv] = bin;
            __syncthreads();
            bin = red_bin[b][0];
#pragma unroll
            for (int k = 1; k < WPF; ++k) bin = min(bin, red_bin[b][k]);
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
            if ((tid & 63) == 0) red_sec[b][wv] = sec;
            __syncthreads();
            sec = red_sec[b][0];
#pragma unroll
            for (int k = 1; k < WPF; ++k) sec = fmaxf(sec, red_sec[b][k]);
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
    constexpr unsigned long long B = kBlockPoints / N;
    g.nsteps = (g.n_frames + B - 1) / B;
    // one round of workgroups, each with the same number of steps (but for the last ones, one fewer)
    const unsigned long long slots = (unsigned long long)ctx->num_cus * RidgeCfg<N>::min_waves;
    const unsigned long long per_wg = (g.nsteps + slots - 1) / slots;
    const unsigned grid = (unsigned)((g.nsteps + per_wg - 1) / per_wg);
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
    if (nfft < 16 || nfft > 4096 || (nfft & (nfft - 1))) return fail(ctx, GJ_ERR_UNSUPPORTED, "nfft must be a power of two in [16, 4096]");
    if (!d_iq || !d_out) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (reinterpret_cast<uintptr_t>(d_iq) & 1) return fail(ctx, GJ_ERR_INVALID, "capture must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(ctx, GJ_ERR_INVALID, "records must be 4-byte aligned");
    if (hop < 1) return fail(ctx, GJ_ERR_INVALID, "hop must be >= 1");
    if (guard < 0 || 2 * (long long)guard + 1 >= nfft) return fail(ctx, GJ_ERR_INVALID, "guard must be >= 0 with 2 guard + 1 < nfft");
    const size_t fit = gj_ridge_frames(nbytes, first_sample, nfft, hop);
    if (n_frames == 0 || n_frames > fit)
        return fail(ctx, GJ_ERR_INVALID, "n_frames %zu: 1..%zu frames of %d points fit from sample %zu at hop %zu", n_frames, fit, nfft,
                    first_sample, hop);
    RidgeGeom g;
    g.first_sample = first_sample;
    g.hop = hop;
    g.n_frames = n_frames;
    g.nsteps = 0;
    g.neg_off = -0.5f * (float)ctx->off2;
    g.scale2 = (float)(ctx->scale * ctx->scale);
    g.guard = guard;
    switch (nfft) {
        case 16: ridge_launch<16>(ctx, d_iq, g, d_out); break;
        case 32: ridge_launch<32>(ctx, d_iq, g, d_out); break;
        case 64: ridge_launch<64>(ctx, d_iq, g, d_out); break;
        case 128: ridge_launch<128>(ctx, d_iq, g, d_out); break;
        case 256: ridge_launch<256>(ctx, d_iq, g, d_out); break;
        case 512: ridge_launch<512>(ctx, d_iq, g, d_out); break;
        case 1024: ridge_launch<1024>(ctx, d_iq, g, d_out); break;
        case 2048: ridge_launch<2048>(ctx, d_iq, g, d_out); break;
        default: ridge_launch<4096>(ctx, d_iq, g, d_out); break;
    }
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
