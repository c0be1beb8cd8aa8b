// The row/block layer under the per-bin row sums of k_skurt.hip and k_csd.hip (those two include this, nothing else does),
// on the transform front end of stft_group.h.  A ROW is frames_per_row = M consecutive frames, a BLOCK a run of
// consecutive frames of one row, the unit of work of a transform group.  The kernels, their accumulators, their
// occupancy choices and their finalize formulas stay apart, each in its own file.
//
// THE PARTITION RULE: a row of M frames is cut into nb = ceil(M / kRowMaxRun) blocks of run = ceil(M / nb) frames, the
// last one shorter, never empty ((nb - 1) * run < M) -- row_blocks below.  It is a function of M alone, never of the
// transform length, the number of rows, the grid or the device.  A block's partial is computed by ONE group from that
// block's bytes alone, frame by frame in order, and a second launch (each file's finalize kernel) adds a row's partials
// in block order, so a row is bit-identical wherever it lies in a call and whatever else the call computes -- and the two
// kernels, which share this text, cut alike (gj_csd_dev's Saa is gj_sk_dev's S1 bit for bit).
#pragma once
#include "stft_group.h"

namespace gj {

constexpr int kRowMaxRun = 16;       // frames per block at most: at hop = N a block reads 32 N bytes per capture
constexpr int kRowMaxFrames = 65536; // frames per row at most

struct RowBlocks {
    unsigned nb, run;
};
inline RowBlocks row_blocks(int frames_per_row) {
    const unsigned M = (unsigned)frames_per_row;
    const unsigned nb = (M + kRowMaxRun - 1) / kRowMaxRun;
    return RowBlocks{nb, (M + nb - 1) / nb};
}

// what the kernels' parameter structs hold behind their start sample(s)
struct RowGeom {
    unsigned long long hop, n_units, nsteps, last_frame;   // n_units: blocks of the call; last_frame: its last frame
    unsigned frames_per_row, nb, run;
    float neg_off;   // -offset of the unpack convention
};

// ---- device side ------------------------------------------------------------------------------------------------------
// The block of group b (of B to a workgroup) in workgroup step `step`: its first frame and how many frames it holds.  A
// group behind the last block holds none; it walks the call's last block again so that every load stays inside the
// capture, and every group of the grid makes g.run iterations per step (the barriers of the large sizes are
// workgroup-wide).
template <int B>
__device__ __forceinline__ unsigned long long row_block_of(const RowGeom& g, unsigned long long step, int b, unsigned& count) {
    unsigned long long u = step * B + (unsigned)b;
    const bool valid = u < g.n_units;
    if (!valid) u = g.n_units - 1;
    const unsigned long long r = u / g.nb;
    const unsigned j = (unsigned)(u - r * g.nb);
    const unsigned rest = g.frames_per_row - j * g.run;
    count = valid ? (rest < g.run ? rest : g.run) : 0u;
    return r * g.frames_per_row + (unsigned long long)j * g.run;
}

// a short block's spare iterations read the call's last frame
__device__ __forceinline__ unsigned long long row_clamp_frame(const RowGeom& g, unsigned long long f) {
    return f > g.last_frame ? g.last_frame : f;
}

// ---- host side --------------------------------------------------------------------------------------------------------
// whole rows of one capture from sample `first` on; 0 when none fit
inline size_t row_fit(size_t nbytes, size_t first, int nfft, size_t hop, int frames_per_row) {
    const size_t total = nbytes / 2;
    if (nfft < 1 || hop < 1 || frames_per_row < 1 || first > total || total - first < (size_t)nfft) return 0;
    return ((total - first - (size_t)nfft) / hop + 1) / (size_t)frames_per_row;
}

// bytes of the partial sums, `planes` per block, of n_rows rows; 0 for a geometry the kernels refuse and when the product
// does not fit a size_t
inline size_t row_workspace_bytes(int planes, int nfft, int frames_per_row, size_t n_rows) {
    if (!stft_nfft_ok(nfft) || frames_per_row < 2 || frames_per_row > kRowMaxFrames) return 0;
    size_t units = 0, bytes = 0;
    if (__builtin_mul_overflow(n_rows, (size_t)row_blocks(frames_per_row).nb, &units)) return 0;
    if (__builtin_mul_overflow(units, (size_t)nfft * planes * sizeof(float), &bytes)) return 0;
    return bytes;
}

// the first refusals of both entry points, in their order
inline int row_check_shape(gj_ctx* ctx, int nfft, int frames_per_row) {
    if (int rc = stft_check_nfft(ctx, nfft)) return rc;
    if (frames_per_row < 2) return fail(ctx, GJ_ERR_INVALID, "frames_per_row must be >= 2");
    if (frames_per_row > kRowMaxFrames) return fail(ctx, GJ_ERR_UNSUPPORTED, "frames_per_row must be <= %d", kRowMaxFrames);
    return GJ_OK;
}

// the last ones: the context's workspace grown to the partial sums of a call that has passed its other checks
inline int row_workspace(gj_ctx* ctx, int planes, int nfft, int frames_per_row, size_t n_rows, float** partial) {
    const size_t need = row_workspace_bytes(planes, nfft, frames_per_row, n_rows);
    if (!need) return fail(ctx, GJ_ERR_NOMEM, "the partial sums of %zu rows do not fit the address space", n_rows);
    if (int rc = ensure_workspace(ctx, need)) return rc;
    *partial = reinterpret_cast<float*>(ctx->ws);
    return GJ_OK;
}

// the geometry of such a call; nsteps is the launch's to fill in (row_launch)
inline RowGeom row_geom(const gj_ctx* ctx, size_t hop, int frames_per_row, size_t n_rows) {
    const RowBlocks blk = row_blocks(frames_per_row);
    RowGeom g;
    g.hop = hop;
    g.n_units = (unsigned long long)n_rows * blk.nb;
    g.nsteps = 0;
    g.last_frame = (unsigned long long)n_rows * (unsigned)frames_per_row - 1;
    g.frames_per_row = (unsigned)frames_per_row;
    g.nb = blk.nb;
    g.run = blk.run;
    g.neg_off = -0.5f * (float)ctx->off2;
    return g;
}

// One round of workgroups over the call's blocks, kBlockPoints / N to a step: kernel(captures..., g, twiddles, window,
// partial), where Geom holds the RowGeom as `rows`.
template <int N, typename Kernel, typename Geom, typename... Capture>
inline void row_launch(gj_ctx* ctx, Kernel kernel, int min_waves, Geom g, float* partial, Capture... d_iq) {
    constexpr unsigned long long B = kBlockPoints / N;
    g.rows.nsteps = (g.rows.n_units + B - 1) / B;
    const unsigned grid = stft_one_round_grid(ctx, min_waves, g.rows.nsteps);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), 0, ctx->stream, d_iq..., g, ctx->d_twiddle, window_table(ctx, N), partial);
}

// the finalize launches' grid for n_out output cells, 256 to a workgroup
inline unsigned row_finalize_grid(const gj_ctx* ctx, unsigned long long n_out) {
    const unsigned long long want = (n_out + 255) / 256, cap = (unsigned long long)ctx->num_cus * 32;
    return (unsigned)(want < cap ? want : cap);
}

}   // namespace gj
