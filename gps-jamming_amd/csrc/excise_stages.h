// The device stages excise_kernel (k_excise.hip), excise_chirp_kernel (k_excise_chirp.hip), cancel_kernel (k_cancel.hip) and
// cancel2_kernel (k_cancel2.hip) share behind the front end of stft_group.h: their geometry, a group's run of frames, the
// excisors' mask on a bin, the cancellers' prediction on a bin, the group sums of a frame's record and the overlap-add of an
// output pair.  These fix the bits of records and output, so each stands once: "W = 0" and "rate 0" write gj_excise_dev's
// bytes because the kernels inline the same text.  Included through excise_host.h only.  No helper holds a barrier (as
// stft_group.h) or a loop over a thread's bins: one element per call, like stft_window_pair -- the loops written in here
// compiled to other registers and branches (profiles/NOTES_stages.md).
#pragma once
#include "stft_group.h"

namespace gj {

struct ExciseGeom {
    unsigned long long first_sample, n_frames, per_run;
    float offset;    // offset of the unpack convention
    float scale2;    // scale^2: the transform runs on u8 - offset, the powers are scaled to the units of gj_ridge_dev
};

// The run of group b of workgroup `block`, B groups to a workgroup: frames [first, end).  A kernel walks f = first - 1 ..
// end - 1: the first iteration primes the carry with the frame in front of the run and writes nothing, that frame's record
// and bytes belong to the run before.  Every group makes per_run + 1 iterations (the large sizes' barriers are workgroup-wide,
// a wave's lanes stay together for the DPP steps); a frame index outside the call is clamped, for whatever is read per frame,
// and writes nothing.  The group owns f when first <= f <= last (as a member function that test compiled to other branches).
struct ExciseRun {
    long long last, first, end;
    __device__ __forceinline__ ExciseRun(const ExciseGeom& g, unsigned block, int b, int B)
        : last((long long)g.n_frames - 1),
          first((long long)(((unsigned long long)block * B + (unsigned)b) * g.per_run)),
          end(first + (long long)g.per_run) {}
    __device__ __forceinline__ unsigned long long clamped(long long f) const {
        return (unsigned long long)(f < 0 ? 0 : (f > last ? last : f));
    }
};

// The two excisors' mask on one bin: power, strict compare, the thread's share of the three sums, conjugate for the way back
__device__ __forceinline__ void excise_mask_bin(c2& v, float thr, float scale2, float& tot, float& rem, float& cnt) {
    // no contraction here: the compiler otherwise fuses the scaling into the addition to `tot` (one rounding) but not into
    // the selected addition to `rem` (two), and the two sum differently rounded values -- removed must equal total, bit
    // for bit, when every bin is excised
#pragma clang fp contract(off)
    const float p = __builtin_fmaf(v.x, v.x, v.y * v.y) * scale2;
    const bool cut = p > thr;   // strict; false for a NaN threshold
    tot += p;
    rem += cut ? p : 0.f;
    cnt += cut ? 1.f : 0.f;     // at most 4096: exact in float
    v = cut ? make_c2(0.f, 0.f) : make_c2(v.x, -v.y);
}

// The cancellers' prediction on one bin (k_cancel.hip, k_cancel2.hip): W B with every product rounded on its own, never
// contracted: what a complex64 multiplication on the host computes, and exactly 0 for W = 0 and exactly B for W = (1, 0)
__device__ __forceinline__ c2 cancel_predict(c2 w, c2 b) {
#pragma clang fp contract(off)
    const float pr = w.x * b.x, qr = w.y * b.y, pi = w.x * b.y, qi = w.y * b.x;
    return make_c2(pr - qr, pi + qi);
}

// The sums of a frame's record over its transform group, in every lane: the lane ladders, then where the group spans waves
// (2048, 4096 points) the posts into the group's row of each sum's own LDS array, the kernel's __syncthreads(), the folds in
// wave order.  Below 2048 points the arrays are not touched and the kernels place no barrier.
template <int N>
struct GroupSum {
    float& v;
    float (&red)[StftShape<N>::WPF > 1 ? StftShape<N>::B : 1][StftShape<N>::WPF];   // the sum's own LDS array, a row per group
};
template <int N, typename... Sum>
__device__ __forceinline__ void group_sums_post(int b, int tid, const Sum&... s) {
    using S = StftShape<N>;
    const auto add = [](float a, float c) { return a + c; };
    ((s.v = group_reduce_f<S::G>(s.v, add)), ...);
    if constexpr (S::WPF > 1) (waves_post(s.red[b], tid, s.v), ...);
}
template <int N, typename... Sum>
__device__ __forceinline__ void group_sums_fold(int b, const Sum&... s) {
    const auto add = [](float a, float c) { return a + c; };
    if constexpr (StftShape<N>::WPF > 1) ((s.v = waves_fold(s.red[b], add)), ...);
}

// One output pair of the overlap-add.  Behind the second transform y_f = conj(v) / N at the output points jl + TF s; samples
// [f H, (f + 1) H) of the range are the previous frame's second half (carry) + this one's first, lo = v[s], rounded to
// nearest even, clamped to a byte and written to `dst` when `store`; hi = v[s + 8] becomes the carry.
template <int N>
__device__ __forceinline__ void excise_overlap_add(c2 lo, c2 hi, c2& carry, float offset, uint8_t* dst, bool store) {
    constexpr float inv_n = 1.0f / (float)N;
    const float yi = fmaf(lo.x, inv_n, carry.x) + offset;
    const float yq = fmaf(-lo.y, inv_n, carry.y) + offset;
    carry = make_c2(hi.x * inv_n, -hi.y * inv_n);
    if (store) {
        const unsigned ui = (unsigned)fminf(fmaxf(__builtin_rintf(yi), 0.f), 255.f);
        const unsigned uq = (unsigned)fminf(fmaxf(__builtin_rintf(yq), 0.f), 255.f);
        struct __attribute__((packed, aligned(1))) U16 { uint16_t v; };
        reinterpret_cast<U16*>(dst)->v = (uint16_t)(ui | (uq << 8));
    }
}

}   // namespace gj
