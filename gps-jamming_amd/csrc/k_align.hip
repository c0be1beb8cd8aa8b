// Pair alignment (gfx950): gj_align_dev / gj_align_blocks of include/gpsjam.h, which states the definition.  One uint8
// I/Q capture written from another along a linear time base (a 16-tap polyphase FIR at 256 sub-sample positions) and a
// linear phase (a 1024-entry turn), rounded once.  Integer arithmetic from the byte to the byte, and the position and
// the phase of an output sample are products of its index, not carried state: every byte and every record is the
// definition's whatever the tiling.
//
// A workgroup of four waves owns tiles of 4096 output samples, one record each.
//   0. once per workgroup: the tap table (8 KB) and the turn (2 KB) go to LDS;
//   1. per tile: the source samples its outputs read -- ONE contiguous span, at most 4127 samples, since pos_step lies
//      within 2^-8 of 1 -- are unpacked once into LDS as (uI, uQ) int16 pairs, zero outside the source.  The span starts
//      on a 16-byte boundary of the source's address, so a thread brings 8 samples with one 16-byte load where all 8
//      lie inside the source and sample by sample at its two ends;
//   2. per sample: thread tid owns outputs tid, tid + 256, .. of the tile, so a wave's 64 windows start at (nearly)
//      consecutive LDS words: no bank conflicts, and the row of taps is the same address for (nearly) all lanes.  16
//      words, 32 multiply-adds into int32; the turn's c and s; four 64-bit products; floor, offset, clamp; the two bytes
//      go to an LDS image of the tile's output;
//   3. the image leaves as 16-byte stores, a wave's 64 of them contiguous, where d_out is 16-byte aligned and the run is
//      whole, byte by byte otherwise;
//   4. the record, if asked for: power, clipped bytes and edge samples of the thread's outputs, a wave sum each, one LDS
//      word per wave and field, and thread 0 adds the four and stores the record: no atomics, no workspace.
//
// Widths.  |u| <= 255 and |tap| <= 32768: |y| <= 16 * 255 * 32768 = 133 693 440 < 2^31 at any table, partial sums
// included.  |z| <= 2 * 133 693 440 * 32768 < 2^43: int64.  n < 2^28 and pos_step <= 2^32 + 2^24: n * pos_step < 2^61, and
// with |pos0| < 2^60 the position stays inside int64.  A tile's power is at most 4096 * 2 * 255^2 = 532 684 800: uint32.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it.
#include "gj_common.h"

namespace gj {

constexpr int kAlignThreads = 256;
constexpr int kAlignWaves = kAlignThreads / 64;
constexpr int kAlignTile = GJ_ALIGN_BLOCK;
constexpr int kAlignRuns = kAlignTile / kAlignThreads;   // outputs per thread and tile
// k(last) - k(first) <= floor(frac + 4095 (1 + 2^-8)) <= 4111; 7 taps before, 8 behind; up to 7 samples of padding in
// front for the 16-byte boundary: 4111 + 16 + 7 = 4134 words, rounded up to whole 8-sample loads
constexpr int kAlignSpan = 4144;
constexpr long long kAlignHalfPhase = 1ll << 23;

static_assert(GJ_ALIGN_PHASES == 256 && GJ_ALIGN_TAPS == 16 && GJ_ALIGN_ROT_LEN == 1024, "the shifts below");
static_assert(sizeof(gj_align_params) == 32 && sizeof(gj_align_block) == 16, "the header's layout");
static_assert(((kAlignTile - 1ll) * ((1ll << 32) + GJ_ALIGN_MAX_DRIFT) + (1ll << 32) - 1) / (1ll << 32) + GJ_ALIGN_TAPS + 7 <= kAlignSpan,
              "a tile's source span fits the LDS buffer");
static_assert(kAlignSpan % 8 == 0, "whole 8-sample loads");
static_assert(16ll * 255 * 32768 < (1ll << 31), "y fits int32");
static_assert(4096ll * 2 * 255 * 255 < (1ll << 32), "a tile's power fits uint32");

struct AlignGeom {
    long long pos0;
    unsigned long long pos_step;
    unsigned rot_phase, rot_step;
    long long n_src;             // samples of the source
    unsigned long long n_out, n_tiles;
    int out_aligned;             // d_out is 16-byte aligned
};

// (uI, uQ) of one sample's two bytes, u = 2 byte - 255, as an int16 pair
__device__ __forceinline__ unsigned align_unpack(unsigned two_bytes) {
    const int ui = 2 * (int)(two_bytes & 0xffu) - 255, uq = 2 * (int)((two_bytes >> 8) & 0xffu) - 255;
    return ((unsigned)ui & 0xffffu) | ((unsigned)uq << 16);
}

__device__ __forceinline__ int align_lo(unsigned w) { return (int)(short)(w & 0xffffu); }
__device__ __forceinline__ int align_hi(unsigned w) { return (int)w >> 16; }

__global__ __launch_bounds__(kAlignThreads) void align_kernel(const uint8_t* __restrict__ iq, AlignGeom g,
                                                              const int16_t* __restrict__ taps, const int16_t* __restrict__ rot,
                                                              uint8_t* __restrict__ out, gj_align_block* __restrict__ blocks) {
    __shared__ __attribute__((aligned(16))) unsigned s_u[kAlignSpan];                          // (uI, uQ) per sample
    __shared__ __attribute__((aligned(16))) unsigned s_taps[GJ_ALIGN_PHASES * GJ_ALIGN_TAPS / 2];   // two taps per word
    __shared__ __attribute__((aligned(16))) unsigned s_rot[GJ_ALIGN_ROT_LEN / 2];
    __shared__ __attribute__((aligned(16))) unsigned short s_out[kAlignTile];                  // (I, Q) bytes per sample
    __shared__ unsigned sums[kAlignWaves][3];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- 0. the tables
    for (int i = tid; i < GJ_ALIGN_PHASES * GJ_ALIGN_TAPS / 2; i += kAlignThreads) s_taps[i] = reinterpret_cast<const unsigned*>(taps)[i];
    for (int i = tid; i < GJ_ALIGN_ROT_LEN / 2; i += kAlignThreads) s_rot[i] = reinterpret_cast<const unsigned*>(rot)[i];
    const short* const rot16 = reinterpret_cast<const short*>(s_rot);

    for (unsigned long long tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const unsigned long long n0 = tile * (unsigned long long)kAlignTile;
        const int nv = g.n_out - n0 >= (unsigned long long)kAlignTile ? kAlignTile : (int)(g.n_out - n0);   // outputs of this tile

        // ---- 1. the source span: words 0 .. need-1 of s_u hold samples kbase ..
        const long long k_first = (g.pos0 + (long long)(n0 * g.pos_step) + kAlignHalfPhase) >> 32;
        const long long k_last = (g.pos0 + (long long)((n0 + (unsigned)(nv - 1)) * g.pos_step) + kAlignHalfPhase) >> 32;
        const long long ks = k_first - 7;
        const long long kbase = ks - (long long)(((long long)(reinterpret_cast<uintptr_t>(iq) >> 1) + ks) & 7);
        long long need = k_last + 8 - kbase + 1;
        if (need > kAlignSpan) need = kAlignSpan;          // never: the entry point bounds pos_step
        __syncthreads();                                   // the tile before has read s_u and s_out, thread 0 its sums
        for (int c = tid; 8 * c < (int)need; c += kAlignThreads) {
            const long long kk = kbase + 8 * c;
            unsigned w[8];
            if (kk >= 0 && kk + 8 <= g.n_src) {
                const uint4 v = *reinterpret_cast<const uint4*>(iq + 2 * kk);
                w[0] = align_unpack(v.x), w[1] = align_unpack(v.x >> 16), w[2] = align_unpack(v.y), w[3] = align_unpack(v.y >> 16);
                w[4] = align_unpack(v.z), w[5] = align_unpack(v.z >> 16), w[6] = align_unpack(v.w), w[7] = align_unpack(v.w >> 16);
            } else {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const long long k = kk + s;
                    w[s] = (k >= 0 && k < g.n_src) ? align_unpack(*reinterpret_cast<const uint16_t*>(iq + 2 * k)) : 0u;
                }
            }
            reinterpret_cast<uint4*>(s_u)[2 * c] = uint4{w[0], w[1], w[2], w[3]};
            reinterpret_cast<uint4*>(s_u)[2 * c + 1] = uint4{w[4], w[5], w[6], w[7]};
        }
        __syncthreads();

        // ---- 2. the thread's outputs
        unsigned power = 0, clipped = 0, edge = 0;
#pragma unroll 2
        for (int r = 0; r < kAlignRuns; ++r) {
            const int t = tid + kAlignThreads * r;
            if (t < nv) {
                const unsigned long long n = n0 + (unsigned)t;
                const long long pos = g.pos0 + (long long)(n * g.pos_step) + kAlignHalfPhase;
                const long long k = pos >> 32;
                const unsigned p = (unsigned)pos >> 24;
                const unsigned* const win = s_u + (int)(k - 7 - kbase);
                const uint4 ta = reinterpret_cast<const uint4*>(s_taps)[2 * p], tb = reinterpret_cast<const uint4*>(s_taps)[2 * p + 1];
                const unsigned tw[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
                int yi = 0, yq = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned u0 = win[2 * j], u1 = win[2 * j + 1];
                    const int t0 = align_lo(tw[j]), t1 = align_hi(tw[j]);
                    yi += t0 * align_lo(u0) + t1 * align_lo(u1);
                    yq += t0 * align_hi(u0) + t1 * align_hi(u1);
                }
                const unsigned theta = g.rot_phase + (unsigned)n * g.rot_step;
                const unsigned i = ((theta + (1u << 21)) >> 22) & 1023u;
                const long long c = rot16[i], s = rot16[(i - 256u) & 1023u];
                const long long zi = (long long)yi * c - (long long)yq * s, zq = (long long)yi * s + (long long)yq * c;
                const long long wi = (zi >> 29) + 128, wq = (zq >> 29) + 128;                 // arithmetic shift: the floor
                const int bi = wi < 0 ? 0 : (wi > 255 ? 255 : (int)wi), bq = wq < 0 ? 0 : (wq > 255 ? 255 : (int)wq);
                s_out[t] = (unsigned short)(bi | (bq << 8));
                power += (unsigned)((2 * bi - 255) * (2 * bi - 255) + (2 * bq - 255) * (2 * bq - 255));
                clipped += (bi != wi ? 1u : 0u) + (bq != wq ? 1u : 0u);
                edge += (k - 7 < 0 || k + 8 >= g.n_src) ? 1u : 0u;
            }
        }
        if (blocks) {   // the same in every thread
            power = wave_sum_u32(power), clipped = wave_sum_u32(clipped), edge = wave_sum_u32(edge);
            if (lane == 0) sums[wave][0] = power, sums[wave][1] = clipped, sums[wave][2] = edge;
        }
        __syncthreads();

        // ---- 3. the tile's bytes: 16-byte run q holds outputs 8 q .. 8 q + 7
        uint8_t* const dst = out + 2 * n0;
#pragma unroll
        for (int h = 0; h < kAlignTile / 8 / kAlignThreads; ++h) {
            const int q = tid + kAlignThreads * h;
            if (8 * q + 8 <= nv && g.out_aligned)
                reinterpret_cast<uint4*>(dst)[q] = reinterpret_cast<const uint4*>(s_out)[q];
            else {   // the ragged end, or an output that is not 16-byte aligned
                const uint8_t* const img = reinterpret_cast<const uint8_t*>(s_out) + 16 * q;
                for (int b = 0; b < 16; ++b)
                    if (16 * q + b < 2 * nv) dst[16 * q + b] = img[b];
            }
        }

        // ---- 4. the tile's record
        if (blocks && tid == 0) {
            gj_align_block rec;
            rec.power_out = 0, rec.n_clipped = 0, rec.n_edge = 0;
#pragma unroll
            for (int w = 0; w < kAlignWaves; ++w) rec.power_out += sums[w][0], rec.n_clipped += (int32_t)sums[w][1], rec.n_edge += (int32_t)sums[w][2];
            blocks[tile] = rec;
        }
    }
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_align_blocks(size_t n_out) { return n_out / GJ_ALIGN_BLOCK + (n_out % GJ_ALIGN_BLOCK != 0); }

int gj_align_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, gj_align_params params, const int16_t* d_taps, const int16_t* d_rot,
                 size_t n_out, uint8_t* d_out, gj_align_block* d_blocks) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (!d_iq || !d_taps || !d_rot || !d_out) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (reinterpret_cast<uintptr_t>(d_iq) & 1) return fail(ctx, GJ_ERR_INVALID, "the capture must be 2-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_taps) | reinterpret_cast<uintptr_t>(d_rot)) & 3)
        return fail(ctx, GJ_ERR_INVALID, "the tables must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_blocks) & 7) return fail(ctx, GJ_ERR_INVALID, "records must be 8-byte aligned");
    if (params.reserved != 0) return fail(ctx, GJ_ERR_INVALID, "reserved must be 0");
    if (n_out < 1 || n_out > (size_t)GJ_ALIGN_MAX_SAMPLES) return fail(ctx, GJ_ERR_UNSUPPORTED, "n_out %zu outside 1 .. 2^28", n_out);
    const unsigned long long one = 1ull << 32;
    if (params.pos_step < one - GJ_ALIGN_MAX_DRIFT || params.pos_step > one + GJ_ALIGN_MAX_DRIFT)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "pos_step %llu is more than 2^24 from 2^32", (unsigned long long)params.pos_step);
    if (params.pos0 <= -(1ll << 60) || params.pos0 >= (1ll << 60)) return fail(ctx, GJ_ERR_UNSUPPORTED, "|pos0| must stay under 2^60");
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(d_iq), a1 = a0 + nbytes;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + 2 * n_out;
    if (o0 < a1 && a0 < o1) return fail(ctx, GJ_ERR_INVALID, "d_out overlaps the source");
    AlignGeom g;
    g.pos0 = params.pos0;
    g.pos_step = params.pos_step;
    g.rot_phase = params.rot_phase;
    g.rot_step = params.rot_step;
    g.n_src = (long long)(nbytes / 2);
    g.n_out = n_out;
    g.n_tiles = gj_align_blocks(n_out);
    g.out_aligned = (o0 & 15) == 0;
    // 37 KB of LDS per workgroup: four of them share a CU
    const unsigned long long slots = 4ull * (unsigned)(ctx->num_cus > 0 ? ctx->num_cus : 1);
    const unsigned grid = (unsigned)(g.n_tiles < slots ? g.n_tiles : slots);
    hipLaunchKernelGGL(align_kernel, dim3(grid), dim3(kAlignThreads), 0, ctx->stream, d_iq, g, d_taps, d_rot, d_out, d_blocks);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
