// The host side the two excisors, k_excise.hip and k_excise_chirp.hip, and the two cancellers, k_cancel.hip and k_cancel2.hip,
// share (those four include this, nothing else does): the geometry of a call, the refusals all four make in the same words,
// the run arithmetic of their launches and the copy of the edges no frame pair covers.  Their shared device stages,
// excise_stages.h, come in through here.  The transform kernels themselves stay apart, each in its own file.
#pragma once
#include "excise_stages.h"

namespace gj {

// the geometry of a call that has passed its checks; per_run is the launch's to fill in (excise_runs)
inline ExciseGeom excise_geom(const gj_ctx* ctx, size_t first_sample, size_t n_samples, int nfft) {
    ExciseGeom g;
    g.first_sample = first_sample;
    g.n_frames = gj_excise_frames(n_samples, nfft);
    g.per_run = 0;
    g.offset = 0.5f * (float)ctx->off2;
    g.scale2 = (float)(ctx->scale * ctx->scale);
    return g;
}

// the refusals the four entry points make in the same words, in the order all four make them
inline int excise_check_shape(gj_ctx* ctx, const float* d_threshold, const void* d_frames, size_t n_samples, int nfft) {
    if (reinterpret_cast<uintptr_t>(d_threshold) & 3) return fail(ctx, GJ_ERR_INVALID, "thresholds must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_frames) & 3) return fail(ctx, GJ_ERR_INVALID, "records must be 4-byte aligned");
    if (n_samples < (size_t)nfft) return fail(ctx, GJ_ERR_INVALID, "n_samples %zu is less than one frame of %d points", n_samples, nfft);
    return GJ_OK;
}

// One round of transform groups, B to a workgroup: runs of equal length, the length from the frame count alone -- at least
// min_run frames (but for short calls), which bounds the priming overhead.
struct ExciseRuns {
    unsigned long long per_run;
    unsigned grid;
};
inline ExciseRuns excise_runs(unsigned long long n_frames, unsigned long long B, int min_waves, int min_run, int num_cus) {
    const unsigned long long slots = (unsigned long long)num_cus * min_waves * B;
    unsigned long long per = (n_frames + slots - 1) / slots;
    if (per < (unsigned long long)min_run) per = min_run;
    if (per > n_frames) per = n_frames;
    const unsigned long long runs = (n_frames + per - 1) / per;
    return ExciseRuns{per, (unsigned)((runs + B - 1) / B)};
}

// the first half frame [0, n_head) and the tail [tail_first, n_bytes) come back as they went in.  Internal linkage: the
// library is built without relocatable device code, so each of the two translation units launches a copy of its own.
static __global__ __launch_bounds__(256) void excise_edges_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                                  unsigned long long n_head, unsigned long long tail_first,
                                                                  unsigned long long n_bytes) {
    const unsigned long long n_tail = n_bytes - tail_first;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_head + n_tail;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long at = i < n_head ? i : tail_first + (i - n_head);
        out[at] = src[at];
    }
}

// the second, small launch of both excisors, behind the transform kernel on the context's stream
static int excise_copy_edges(gj_ctx* ctx, const uint8_t* d_iq, const ExciseGeom& g, size_t n_samples, int nfft, uint8_t* d_out) {
    const unsigned long long h2 = (unsigned long long)nfft;   // bytes of half a frame
    const unsigned long long tail_first = g.n_frames * h2, n_bytes = 2ull * n_samples;
    const unsigned long long edge = h2 + (n_bytes - tail_first);   // < 3 nfft bytes
    hipLaunchKernelGGL(excise_edges_kernel, dim3((unsigned)((edge + 255) / 256)), dim3(256), 0, ctx->stream,
                       d_iq + 2 * g.first_sample, d_out, h2, tail_first, n_bytes);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // namespace gj
