// Exact lag-window correlation of two uint8 I/Q ranges (gfx950): gj_xcorr_fine_dev / gj_fine_blocks of include/gpsjam.h,
// which states the definition.  The 2R + 1 lags around K5's integer answer as a direct time-domain sum: integer
// arithmetic throughout, so totals and block records are those of the definition whatever the tiling and the order.
//
// A workgroup of four waves owns tiles of two record blocks (8192 samples of a).  Per tile:
//   1. b's samples u0 .. u0 + 8192 + lags, u0 = tile start + lag_center - R, are loaded as 16-byte chunks (2-byte
//      aligned loads, first_b may be odd), unpacked to (2 I - o2, 2 Q - o2) as two int16 in one word, zero outside
//      [0, n), and staged ONCE in LDS: 33 KiB;
//   2. a wave owns half a block: every lane keeps 8 groups of 4 consecutive samples of a in registers, unpacked the
//      same way, once as (uI, uQ) and once as (-uQ, uI).  v_dot2_i32_i16 of b's word with the first is the real part's
//      term, with the second the imaginary part's.  Four lags run at a time: a lane reads the 7 words of b that its 4
//      samples meet under those 4 lags as two aligned LDS reads of 16 and 12 bytes (conflict-free: lanes are 16 bytes
//      apart) and spends 32 dot instructions on them; 2R + 1 is rounded up to a multiple of 4 and the surplus lags are dropped;
//   3. per lag group eight DPP wave reductions, one LDS word per wave and field;
//   4. behind a barrier, thread f < 2 (2R + 1) adds the two waves of each block: that is the block record, stored by
//      this one workgroup (plain 4-byte stores), and is added to a 64-bit sum the thread keeps over all its tiles.
// Totals: d_total is zeroed by a memset node in front of the launch, and every workgroup adds its 64-bit sums with one
// 64-bit atomic add per field when it has run out of tiles.  Integer sums commute: the total does not depend on which
// workgroup arrives when.  No workspace, no second launch.
//
// Widths.  |uI|, |uQ| <= 510 (offsets 0 and 255): int16.  One term is at most 2 * 510^2 = 520 200.  A lane's
// accumulator holds 32 terms (1.7e7), a wave's sum 2048 (1 065 369 600), a block's 4096: 2 130 739 200 < 2^31, the bound
// of the header; every partial sum of a block is bounded by the same figure, so int32 never wraps.  The 64-bit sums
// hold 2^63 / 520 200 > 1.7e13 samples.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it.
#include "gj_common.h"

namespace gj {

constexpr int kFineThreads = 256;
constexpr int kFineWaves = kFineThreads / 64;
constexpr int kFineTileBlocks = 2;
constexpr int kFineTile = kFineTileBlocks * GJ_FINE_BLOCK;          // samples of a that a workgroup owns at a time
constexpr int kFineWaveSamples = kFineTile / kFineWaves;            // 2048: half a record block
constexpr int kFineGroups = kFineWaveSamples / (64 * 4);            // 8 groups of 4 samples per lane
constexpr int kFineMaxLags = 2 * GJ_FINE_MAX_HALF + 1;              // 65
constexpr int kFineMaxLags4 = (kFineMaxLags + 3) / 4 * 4;           // 68
// words of b in LDS: sample p under lag index kk reads words p + kk .. p + kk + 7, p <= kFineTile - 4, kk <= 64
constexpr int kFineExtMax = (kFineTile + kFineMaxLags4 + 4 + 7) / 8 * 8;
constexpr int kFineStageIters = (kFineExtMax / 8 + kFineThreads - 1) / kFineThreads;

static_assert(GJ_FINE_BLOCK == 4096 && kFineWaves == 2 * kFineTileBlocks, "two waves per record block");
static_assert(kFineTile - 4 + (kFineMaxLags4 - 4) + 7 < kFineExtMax, "the last lag group's reads stay inside the staged words");
static_assert(2 * kFineMaxLags <= kFineThreads, "one thread per record field");
static_assert(4096ll * 2 * 510 * 510 < (1ll << 31), "a block record fits int32");

struct FineGeom {
    unsigned long long first_a, first_b, n_samples, n_tiles, n_blocks;
    long long lag_first;         // lag_center - R
    int n_lags;                  // 2R + 1
    int n_lags4;                 // rounded up to a multiple of 4
    int o2;                      // 2 * offset of the unpack convention
};

// a run of a capture that is only known to be 2-byte aligned; global memory takes unaligned vector loads
struct __attribute__((packed, aligned(2))) FineChunk16 {
    unsigned x, y, z, w;
};
struct __attribute__((packed, aligned(2))) FineChunk8 {
    unsigned x, y;
};

// bytes (I, Q) in the low half of `pair` -> (2 I - o2) in bits 0..15, (2 Q - o2) in bits 16..31
__device__ __forceinline__ unsigned fine_unpack(unsigned pair, int o2) {
    const int i = 2 * (int)(pair & 0xffu) - o2, q = 2 * (int)((pair >> 8) & 0xffu) - o2;
    return ((unsigned)i & 0xffffu) | ((unsigned)q << 16);
}

// S unpacked samples t .. t + S - 1 of the range that starts at src; zero where t + s lies outside [0, n): never a byte
// outside the range is read, and what is outside counts as the SAMPLE zero, not as the byte zero
template <int S, typename Chunk>
__device__ __forceinline__ void fine_load(unsigned (&dst)[S], const uint8_t* __restrict__ src, long long t, long long n, int o2) {
    unsigned raw[S / 2];
#pragma unroll
    for (int d = 0; d < S / 2; ++d) raw[d] = 0u;
#pragma unroll
    for (int s = 0; s < S; ++s) dst[s] = 0u;
    if (t >= 0 && t + S <= n) {
        const Chunk c = *reinterpret_cast<const Chunk*>(src + 2 * t);
        raw[0] = c.x, raw[1] = c.y;
        if constexpr (S == 8) raw[2] = c.z, raw[3] = c.w;
#pragma unroll
        for (int s = 0; s < S; ++s) dst[s] = fine_unpack(raw[s >> 1] >> (16 * (s & 1)), o2);
    } else if (t > -S && t < n) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const long long u = t + s;
            if (u >= 0 && u < n) dst[s] = fine_unpack((unsigned)*reinterpret_cast<const uint16_t*>(src + 2 * u), o2);
        }
    }
}

__device__ __forceinline__ int fine_dot2(unsigned b, unsigned a, int acc) {
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "v"(acc));
    return r;
}

__global__ __launch_bounds__(kFineThreads) void fine_kernel(const uint8_t* __restrict__ iq_a, const uint8_t* __restrict__ iq_b, FineGeom g,
                                                            unsigned long long* __restrict__ total, int32_t* __restrict__ blocks) {
    __shared__ __attribute__((aligned(16))) unsigned B[kFineExtMax];
    __shared__ int sums[kFineWaves][2 * kFineMaxLags4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* const src_a = iq_a + 2 * g.first_a;
    const uint8_t* const src_b = iq_b + 2 * g.first_b;
    const long long n = (long long)g.n_samples;
    const int n_chunks = (kFineTile + g.n_lags4 + 4 + 7) / 8;       // <= kFineExtMax / 8
    const int fields = 2 * g.n_lags;
    long long acc = 0;                                              // thread f < fields: field f over this workgroup's tiles

    for (unsigned long long tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const long long t0 = (long long)(tile * (unsigned long long)kFineTile);

        // ---- 1. b -> LDS
        const long long u0 = t0 + g.lag_first;
#pragma unroll
        for (int j = 0; j < kFineStageIters; ++j) {
            const int c = j * kFineThreads + tid;
            if (c < n_chunks) {
                unsigned w[8];
                fine_load<8, FineChunk16>(w, src_b, u0 + 8 * c, n, g.o2);
                uint4* dst = reinterpret_cast<uint4*>(B + 8 * c);
                dst[0] = uint4{w[0], w[1], w[2], w[3]};
                dst[1] = uint4{w[4], w[5], w[6], w[7]};
            }
        }

        // ---- 2. a -> registers: (uI, uQ) and (-uQ, uI)
        unsigned a_re[kFineGroups][4], a_im[kFineGroups][4];
        const int p0 = wave * kFineWaveSamples + 4 * lane;          // local sample of group 0
#pragma unroll
        for (int gr = 0; gr < kFineGroups; ++gr) {
            fine_load<4, FineChunk8>(a_re[gr], src_a, t0 + p0 + gr * 256, n, g.o2);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const unsigned v = a_re[gr][s];
                a_im[gr][s] = ((0u - (v >> 16)) & 0xffffu) | (v << 16);
            }
        }
        __syncthreads();

        // ---- 3. four lags at a time
        for (int kk = 0; kk < g.n_lags4; kk += 4) {
            int re[4] = {0, 0, 0, 0}, im[4] = {0, 0, 0, 0};
#pragma unroll
            for (int gr = 0; gr < kFineGroups; ++gr) {
                const uint4* src = reinterpret_cast<const uint4*>(B + p0 + gr * 256 + kk);
                const uint4 lo = src[0], hi = src[1];
                const unsigned bw[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        re[d] = fine_dot2(bw[s + d], a_re[gr][s], re[d]);
                        im[d] = fine_dot2(bw[s + d], a_im[gr][s], im[d]);
                    }
                }
            }
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int r = group_sum_dpp<64>(re[d]), i = group_sum_dpp<64>(im[d]);
                if (lane == 0) sums[wave][2 * (kk + d)] = r, sums[wave][2 * (kk + d) + 1] = i;
            }
        }
        __syncthreads();

        // ---- 4. records and the running 64-bit sums
        if (tid < fields) {
#pragma unroll
            for (int b = 0; b < kFineTileBlocks; ++b) {
                const unsigned long long block = tile * kFineTileBlocks + (unsigned)b;
                if (block < g.n_blocks) {
                    const int v = sums[2 * b][tid] + sums[2 * b + 1][tid];
                    if (blocks) blocks[block * (unsigned long long)fields + (unsigned)tid] = v;
                    acc += v;
                }
            }
        }
        // the next tile's B is written behind this tile's last read of it (the barrier above), and its sums behind the
        // barrier that follows its staging, which these reads of sums precede
    }
    if (tid < fields) atomicAdd(total + tid, (unsigned long long)acc);
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_fine_blocks(size_t n_samples) { return n_samples / GJ_FINE_BLOCK + (n_samples % GJ_FINE_BLOCK != 0); }

int gj_xcorr_fine_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b, size_t nbytes_b,
                      size_t first_b, size_t n_samples, int32_t lag_center, int half_width, int64_t* d_total, int32_t* d_blocks) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (half_width < 0 || half_width > GJ_FINE_MAX_HALF)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "half_width %d (0 .. %d)", half_width, GJ_FINE_MAX_HALF);
    if (!d_a || !d_b || !d_total) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 1)
        return fail(ctx, GJ_ERR_INVALID, "captures must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_total) & 7) return fail(ctx, GJ_ERR_INVALID, "totals must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_blocks) & 3) return fail(ctx, GJ_ERR_INVALID, "records must be 4-byte aligned");
    if (n_samples == 0) return fail(ctx, GJ_ERR_INVALID, "n_samples is 0");
    if (first_a > nbytes_a / 2 || n_samples > nbytes_a / 2 - first_a)
        return fail(ctx, GJ_ERR_INVALID, "samples %zu .. +%zu run past capture a's %zu", first_a, n_samples, nbytes_a / 2);
    if (first_b > nbytes_b / 2 || n_samples > nbytes_b / 2 - first_b)
        return fail(ctx, GJ_ERR_INVALID, "samples %zu .. +%zu run past capture b's %zu", first_b, n_samples, nbytes_b / 2);
    const long long c = lag_center;
    if ((c < 0 ? -c : c) + half_width > 2147483647ll)
        return fail(ctx, GJ_ERR_INVALID, "|lag_center| + half_width overflows int32");
    FineGeom g;
    g.first_a = first_a;
    g.first_b = first_b;
    g.n_samples = n_samples;
    g.n_tiles = (n_samples + kFineTile - 1) / kFineTile;
    g.n_blocks = gj_fine_blocks(n_samples);
    g.lag_first = c - half_width;
    g.n_lags = 2 * half_width + 1;
    g.n_lags4 = (g.n_lags + 3) / 4 * 4;
    g.o2 = ctx->off2;
    // every workgroup resident at once (four per CU) and the same number of tiles for each but the last few
    const unsigned long long slots = 4ull * (unsigned)(ctx->num_cus > 0 ? ctx->num_cus : 1);
    const unsigned long long per = (g.n_tiles + slots - 1) / slots;
    const unsigned grid = (unsigned)((g.n_tiles + per - 1) / per);
    GJ_HIP(ctx, hipMemsetAsync(d_total, 0, 16 * (size_t)g.n_lags, ctx->stream));
    hipLaunchKernelGGL(fine_kernel, dim3(grid), dim3(kFineThreads), 0, ctx->stream, d_a, d_b, g,
                       reinterpret_cast<unsigned long long*>(d_total), d_blocks);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
