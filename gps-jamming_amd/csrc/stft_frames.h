// What ridge_kernel (k_ridge.hip) and chirp_kernel (k_chirp.hip) share besides the front end of stft_group.h (those two
// include this, nothing else does): the walk over frames at any hop and the host side of a call over n_frames frames.
// RidgeGeom is a prefix of ChirpGeom; both stay flat structs (nesting would move the kernel arguments behind it), so the
// helpers take the geometry as a template type.  The reduction of a spectrum to the ridge's four numbers is NOT in here: it
// stands in both kernels.  Stated once, cut at its three barriers, it made chirp_kernel at 2048 points 2.8 % slower
// (profiles/NOTES_stages.md).
#pragma once
#include "stft_group.h"

#include <climits>   // INT_MAX of the two kernels' reductions

namespace gj {

// Frame f starts at first_sample + f * hop, any hop.  A group without a frame (behind the last one) transforms the last
// frame again: every load stays inside the capture.
template <typename Geom>
__device__ __forceinline__ const uint8_t* frame_base(const uint8_t* iq, const Geom& g, unsigned long long f) {
    const unsigned long long last = g.n_frames - 1;
    if (f > last) f = last;
    return iq + 2ull * (g.first_sample + f * g.hop);
}

// the refusals gj_ridge_dev and gj_chirp_dev make in the same words, in the order both make them
inline int frames_check_buffers(gj_ctx* ctx, const uint8_t* d_iq, const void* d_out) {
    if (!d_iq || !d_out) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = stft_check_capture(ctx, d_iq)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(ctx, GJ_ERR_INVALID, "records must be 4-byte aligned");
    return GJ_OK;
}
inline int frames_check_geometry(gj_ctx* ctx, size_t nbytes, size_t first_sample, int nfft, size_t hop, size_t n_frames, int guard) {
    if (hop < 1) return fail(ctx, GJ_ERR_INVALID, "hop must be >= 1");
    if (guard < 0 || 2 * (long long)guard + 1 >= nfft) return fail(ctx, GJ_ERR_INVALID, "guard must be >= 0 with 2 guard + 1 < nfft");
    const size_t fit = gj_ridge_frames(nbytes, first_sample, nfft, hop);
    if (n_frames == 0 || n_frames > fit)
        return fail(ctx, GJ_ERR_INVALID, "n_frames %zu: 1..%zu frames of %d points fit from sample %zu at hop %zu", n_frames, fit, nfft,
                    first_sample, hop);
    return GJ_OK;
}
// the fields RidgeGeom and ChirpGeom share, of a call that has passed its checks; nsteps is the launch's to fill in
template <typename Geom>
inline Geom frames_geom(const gj_ctx* ctx, size_t first_sample, size_t hop, size_t n_frames, int guard) {
    Geom g{};
    g.first_sample = first_sample;
    g.hop = hop;
    g.n_frames = n_frames;
    g.nsteps = 0;
    g.neg_off = -0.5f * (float)ctx->off2;
    g.scale2 = (float)(ctx->scale * ctx->scale);
    g.guard = guard;
    return g;
}
// B frames to a step, one round of workgroups: fills in nsteps and returns the grid
template <int N, typename Geom>
inline unsigned frames_one_round(const gj_ctx* ctx, int min_waves, Geom& g) {
    constexpr unsigned long long B = kBlockPoints / N;
    g.nsteps = (g.n_frames + B - 1) / B;
    return stft_one_round_grid(ctx, min_waves, g.nsteps);
}

}   // namespace gj
