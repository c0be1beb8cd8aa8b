// The short-time transform front end of k_ridge.hip, k_excise.hip, k_skurt.hip, k_chirp.hip, k_excise_chirp.hip, k_csd.hip,
// k_cancel.hip and k_cancel2.hip (those eight include it through stft_frames.h, excise_stages.h or stft_rows.h).  The
// transform is K2's (k_welch.hip): one 256-thread workgroup holds 4096 / N transform groups of N / 16 threads,
// every thread pulls its 16 samples straight from the uint8 stream, applies unpack and the periodic Hann window of K2's
// table and runs the register-resident Stockham passes of fft_core.h with LDS exchanges.  Unlike K2's segments a frame may
// start at any sample, so it is only 2-byte aligned, and there is one LDS buffer with two barriers per exchange.
#pragma once
#include "gj_common.h"

#include <type_traits>

namespace gj {

extern const float* window_table(gj_ctx* ctx, int n);   // api.hip: K2's periodic Hann tables

// ---- the transform group ----------------------------------------------------------------------------------------------
template <int N>
struct StftShape {
    static constexpr int TF = N / 16;                       // threads per transform
    static constexpr int B = kBlockPoints / N;              // transforms per workgroup
    static constexpr int NP = fft_npass(N);
    static constexpr int WPF = (TF >= 64) ? TF / 64 : 1;    // waves per transform
    static constexpr int G = TF >= 64 ? 64 : TF;            // lanes of one wave that belong to the same transform
    // what the wave fence of stft_exchange_sync rests on (k_welch.hip): a transform group is an aligned fraction of ONE wave
    static_assert(TF > 64 || (64 % TF == 0 && WPF == 1 && kBlockThreads % 64 == 0 && B * TF == kBlockThreads),
                  "the wave-fence exchange needs a transform group inside one wave");
};

// A thread's roles.  XP: the conflict-free exchange schedule of fft_core.h (X4096), which changes the role after pass 0.
struct StftRoles {
    int b;     // transform group within the workgroup
    int jl0;   // butterfly of pass 0 (input index jl0 + TF s)
    int jl;    // butterfly of the later passes = bins held at the end: jl + TF s
};
template <int N, bool XP>
__device__ __forceinline__ StftRoles stft_roles(int tid) {
    constexpr int TF = StftShape<N>::TF;
    const int jl0 = tid % TF;
    return StftRoles{(TF >= 64) ? __builtin_amdgcn_readfirstlane(tid / TF) : tid / TF, jl0, XP ? X4096::jl1(tid) : jl0};
}

// The exchange barrier, as K2's welch_exchange_sync: up to 1024 points a transform's N / 16 threads lie inside one wave,
// whose LDS instructions execute in issue order -- a wavefront fence keeps the compiler from reordering scatter and
// gather; larger transforms span waves and take the workgroup barrier.
template <int N>
__device__ __forceinline__ void stft_exchange_sync() {
    if constexpr (N / 16 <= 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

template <int N, int PASS>
__device__ __forceinline__ void stft_passes(c2 (&v)[16], cf* lds, int base, int jl, const c2 (&tw)[3][15], const InnerTw& ktw) {
    fft_pass<N, PASS, true>(v, tw[PASS], ktw);
    if constexpr (PASS + 1 < fft_npass(N)) {
        lds_scatter<N, PASS>(v, lds, base, jl);
        stft_exchange_sync<N>();
        lds_gather<N>(v, lds, base, jl);
        stft_exchange_sync<N>();
        stft_passes<N, PASS + 1>(v, lds, base, jl, tw, ktw);
    }
}

// 4096 points: pass 0 in role jl0 = tid, passes 1 and 2 in role jl1 (fft_core.h, X4096)
__device__ __forceinline__ void stft_passes_x4096(c2 (&v)[16], cf* lds, int tid, const c2 (&tw)[3][15], const InnerTw& ktw) {
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

// the twiddle sets of the passes behind the first, for butterfly jl
template <int N>
__device__ __forceinline__ void stft_load_twiddles(c2 (&tw)[3][15], const cf* twtab, int jl) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int k = 0; k < 15; ++k) tw[p][k] = make_c2(1.f, 0.f);
    if constexpr (fft_npass(N) > 1) load_twiddles<N, 1>(tw[1], twtab, jl);
    if constexpr (fft_npass(N) > 2) load_twiddles<N, 2>(tw[2], twtab, jl);
}

// Pair s of the window of the thread's 16 input points: (w[2s], w[2s+1]) share a register pair, op_sel picks the half.
// One pair per call, the kernels fill their wp[8] themselves: filling the array in here made hipcc order the prologue's
// loads differently and changed sk_kernel's register count (profiles/NOTES_stft_group.md).
template <int N>
__device__ __forceinline__ c2 stft_window_pair(const float* wintab, int jl0, int s) {
    constexpr int TF = N / 16;
    return make_c2(wintab[jl0 + TF * (2 * s)], wintab[jl0 + TF * (2 * s + 1)]);
}

// The thread's samples jl0 + TF s of the frame at `base`, one uint16 (I, Q) each.  WIDE (N <= 32 only): the whole frame in
// 16-byte loads, the thread's samples picked out of the registers; from 64 points on that needs a run-time choice between
// registers and is slower than 2-byte loads (k_welch.hip, wide_load).
template <int N, bool WIDE>
__device__ __forceinline__ void stft_load_frame(unsigned (&dst)[16], const uint8_t* base, int jl0) {
    constexpr int TF = N / 16;
    if constexpr (WIDE) {
        static_assert(N <= 32, "the register pick below is written for one or two threads per frame");
        // 2 N bytes; sample jl0 + TF s is one half of dword (jl0 + TF s) / 2.  The frame is only 2-byte aligned: global
        // memory takes unaligned vector loads.
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
}

// unpack and window: v = (u8 + koff) * w, koff = -offset of the unpack convention in both halves
__device__ __forceinline__ void stft_unpack_window(c2 (&v)[16], const unsigned (&raw)[16], const c2 (&wp)[8], c2 koff) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const unsigned u = raw[s];
        const c2 x = cadd(make_c2((float)(u & 255u), (float)((u >> 8) & 255u)), koff);   // exact: u8 minus a multiple of 0.5
        v[s] = (s & 1) ? scale_hi(x, wp[s >> 1]) : scale_lo(x, wp[s >> 1]);
    }
}

// ---- reductions over a transform group --------------------------------------------------------------------------------
// Reduction of `v` over each aligned group of G lanes (power of two, 1..64), result in every lane of the group: the
// DPP steps of group_sum_dpp_f (gj_common.h) inside a row of 16, shuffles across rows.  `op` must be commutative: lane
// pairs then compute op(a, b) and op(b, a) and stay bit-identical.
template <int G, typename Op>
__device__ __forceinline__ int group_reduce_i(int v, Op op) {
#define GJ_DPP(x, ctrl) __builtin_amdgcn_update_dpp(0, x, ctrl, 0xf, 0xf, false)
    if constexpr (G >= 2) v = op(v, GJ_DPP(v, 0xB1));     // quad_perm [1,0,3,2]
    if constexpr (G >= 4) v = op(v, GJ_DPP(v, 0x4E));     // quad_perm [2,3,0,1]
    if constexpr (G >= 8) v = op(v, GJ_DPP(v, 0x141));    // row_half_mirror
    if constexpr (G >= 16) v = op(v, GJ_DPP(v, 0x140));   // row_mirror
#undef GJ_DPP
    if constexpr (G >= 32) v = op(v, __shfl_xor(v, 16, 64));
    if constexpr (G >= 64) v = op(v, __shfl_xor(v, 32, 64));
    return v;
}
template <int G>
__device__ __forceinline__ int group_min_i(int v) {
    return group_reduce_i<G>(v, [](int a, int c) { return min(a, c); });
}
// the same ladder on a float's bits
template <int G, typename Op>
__device__ __forceinline__ float group_reduce_f(float v, Op op) {
    return __int_as_float(group_reduce_i<G>(
        __float_as_int(v), [op](int a, int c) { return __float_as_int(op(__int_as_float(a), __int_as_float(c))); }));
}

// A transform group that spans waves (2048 and 4096 points) combines its waves' results through LDS, in wave order: lane 0
// of every wave posts into the group's row of the reduction's OWN array, the caller's __syncthreads() publishes, every
// lane folds.  One array per reduction and no barrier in here: a wave that is ahead must never overwrite what a slower
// one still reads, and the callers keep the number and the places of their barriers in sight.
template <int WPF, typename T>
__device__ __forceinline__ void waves_post(T (&row)[WPF], int tid, T v) {
    if ((tid & 63) == 0) row[(tid >> 6) % WPF] = v;
}
template <int WPF, typename T, typename Op>
__device__ __forceinline__ T waves_fold(const T (&row)[WPF], Op op) {
    T r = row[0];
#pragma unroll
    for (int k = 1; k < WPF; ++k) r = op(r, row[k]);
    return r;
}

// ---- host side --------------------------------------------------------------------------------------------------------
inline bool stft_nfft_ok(int nfft) { return nfft >= 16 && nfft <= 4096 && !(nfft & (nfft - 1)); }
inline int stft_check_nfft(gj_ctx* ctx, int nfft) {
    return stft_nfft_ok(nfft) ? GJ_OK : fail(ctx, GJ_ERR_UNSUPPORTED, "nfft must be a power of two in [16, 4096]");
}
inline int stft_check_capture(gj_ctx* ctx, const uint8_t* d_iq) {
    return (reinterpret_cast<uintptr_t>(d_iq) & 1) ? fail(ctx, GJ_ERR_INVALID, "capture must be 2-byte aligned") : GJ_OK;
}

// f(std::integral_constant<int, nfft>) for an nfft that passed stft_check_nfft
template <typename F>
inline void stft_dispatch(int nfft, F&& f) {
    switch (nfft) {
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 32: f(std::integral_constant<int, 32>{}); break;
        case 64: f(std::integral_constant<int, 64>{}); break;
        case 128: f(std::integral_constant<int, 128>{}); break;
        case 256: f(std::integral_constant<int, 256>{}); break;
        case 512: f(std::integral_constant<int, 512>{}); break;
        case 1024: f(std::integral_constant<int, 1024>{}); break;
        case 2048: f(std::integral_constant<int, 2048>{}); break;
        default: f(std::integral_constant<int, 4096>{}); break;
    }
}

// one round of workgroups, each with the same number of steps (but for the last ones, one fewer)
inline unsigned stft_one_round_grid(const gj_ctx* ctx, int min_waves, unsigned long long nsteps) {
    const unsigned long long slots = (unsigned long long)ctx->num_cus * min_waves;
    const unsigned long long per_wg = (nsteps + slots - 1) / slots;
    return (unsigned)((nsteps + per_wg - 1) / per_wg);
}

}   // namespace gj
