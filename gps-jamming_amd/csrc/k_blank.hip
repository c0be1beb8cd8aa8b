// Time-domain pulse blanking (gfx950): a sliding-window power detector, a guard dilation and the blanked samples put
// to mid-level -- gj_blank_dev / gj_blank_blocks of include/gpsjam.h, which states the definition.  The blanker a
// receiver puts in front of its FFT excisor: a pulse shorter than a frame is spread over every bin of that frame, where
// the per-bin mask of k_excise.hip either wipes the frame or lets the pulse through.
//
// Everything is integer arithmetic, so bytes and records are those of the definition whatever the tiling.  A workgroup
// owns tiles of two record blocks (8192 samples) and walks a tile in five steps:
//   1. every thread loads 16-byte chunks (8 samples) of the tile and of its halo, lane after lane, and keeps them in
//      registers; e = 4 |x|^2 per sample, an inclusive prefix sum inside the chunk, a wave scan of the chunk totals and
//      one LDS step across waves and chunk rows give P[x] = sum of e up to x as uint32 in LDS.  e is at most 2 * 510^2 =
//      520 200 (offsets 0 and 255; 130 050 at 127.5), so over the 12 288 samples of a pass P reaches 6.4e9 and WRAPS
//      there (never at 127.5 or 128: 1.6e9).  A window sum is 1024 * 520 200 = 5.3e8 < 2^30 at most, so a difference
//      of two P is exact all the same;
//   2. a lane per sample: S = P[x - h + W - 1] - P[x - h - 1], D = S > T, and a ballot packs 64 D into one word;
//   3. an exclusive scan of the words' bit counts: the number of D in any interval is two look-ups, so the dilation by
//      `guard` costs the same whatever the guard; B again a lane per sample and a ballot per 64;
//   4. the chunks of step 1, still in registers, leave as they came or blanked by their byte of the B words: one 16-byte
//      store per chunk;
//   5. the two records: total and removed from step 4's e, n_blanked and n_rising from bit counts of the B words.
// No atomics, no second launch, no workspace: a record is written by the one workgroup that owns its block.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it.
#include <cmath>

#include "gj_common.h"

namespace gj {

constexpr int kBlankThreads = 256;
constexpr int kBlankWaves = kBlankThreads / 64;
constexpr int kBlankTileBlocks = 2;
constexpr int kBlankTile = kBlankTileBlocks * GJ_BLANK_BLOCK;   // samples a workgroup owns at a time
constexpr int kBlankMaxWindow = 1024, kBlankMaxGuard = 1024;
constexpr int kBlankIters = 6;                                  // 16-byte chunks per thread and tile
constexpr int kBlankExtMax = kBlankIters * kBlankThreads * 8;   // samples of P held in LDS
// D is needed from one sample in front of the tile's first (n_rising looks at B[t - 1]) minus the guard to the
// tile's last plus the guard
constexpr int kBlankDRowsMax = (kBlankMaxGuard + 1 + kBlankTile + kBlankMaxGuard + 63) / 64;
constexpr int kBlankBRows = kBlankTile / 64;

constexpr int round_up8(int v) { return (v + 7) / 8 * 8; }
static_assert(round_up8(kBlankMaxWindow / 2 + kBlankMaxGuard + 1) + kBlankTile +
                      round_up8(kBlankMaxWindow - 1 - kBlankMaxWindow / 2 + kBlankMaxGuard) <= kBlankExtMax,
              "tile and halos must fit the chunks of one pass");
static_assert(kBlankDRowsMax <= kBlankThreads && kBlankBRows <= kBlankThreads, "one thread per mask word");
static_assert(kBlankTileBlocks <= kBlankWaves && GJ_BLANK_BLOCK == 64 * 64, "one wave reduces the 64 B words of a record block");

struct BlankGeom {
    unsigned long long first_sample, n_samples, n_tiles, n_blocks;
    int window, guard;
    int halo_left, halo_right;   // samples of P in front of / behind the tile, multiples of 8
    int o2;                      // 2 * offset of the unpack convention
    unsigned T;                  // floor(4 W threshold), saturated: no window sum reaches 2^32 - 1
    unsigned blank_pair;         // bytes I Q I Q of two blanked samples, the first at an even index of the range
    int out_aligned;             // d_out is 16-byte aligned
};

// a 16-byte chunk of a capture that is only known to be 2-byte aligned (first_sample may be odd); global memory takes
// unaligned vector loads
struct __attribute__((packed, aligned(2))) BlankChunk {
    unsigned x, y, z, w;
};

// samples t .. t + 7 of the range, zero bytes where t + s lies outside [0, n): never a byte outside the range is read
__device__ __forceinline__ void blank_load(unsigned (&dst)[4], const uint8_t* __restrict__ src, long long t, long long n) {
    dst[0] = dst[1] = dst[2] = dst[3] = 0u;
    if (t >= 0 && t + 8 <= n) {
        const BlankChunk* p = reinterpret_cast<const BlankChunk*>(src + 2 * t);
        dst[0] = p->x, dst[1] = p->y, dst[2] = p->z, dst[3] = p->w;
    } else if (t > -8 && t < n) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const long long u = t + s;
            if (u >= 0 && u < n) dst[s >> 1] |= (unsigned)*reinterpret_cast<const uint16_t*>(src + 2 * u) << (16 * (s & 1));
        }
    }
}

// e = (2 I - o2)^2 + (2 Q - o2)^2 of sample s of a chunk
__device__ __forceinline__ unsigned blank_e(const unsigned (&raw)[4], int s, int o2) {
    const unsigned pair = raw[s >> 1] >> (16 * (s & 1));
    const int i = 2 * (int)(pair & 0xffu) - o2, q = 2 * (int)((pair >> 8) & 0xffu) - o2;
    return (unsigned)(i * i + q * q);
}

// inclusive sum over the lanes 0 .. lane of a wave
__device__ __forceinline__ unsigned wave_scan_u32(unsigned v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// The second bound is waves per SIMD.  A workgroup is kBlankWaves = 4 waves, one per SIMD, so 3 is also three workgroups
// per CU, which is what the 52 KiB of LDS admit; another kBlankThreads needs another figure here.
static_assert(kBlankWaves == 4, "__launch_bounds__ below reads 3 waves per SIMD as three workgroups per CU");
__global__ __launch_bounds__(kBlankThreads, 3) void blank_kernel(const uint8_t* __restrict__ iq, BlankGeom g, uint8_t* __restrict__ out,
                                                                 gj_blank_block* __restrict__ blocks) {
    // P[x], x = -1 .. kBlankExtMax - 1, with P[-1] = 0; a chunk's eight values start on a 16-byte boundary
    __shared__ __attribute__((aligned(16))) unsigned p_lds[4 + kBlankExtMax];
    __shared__ unsigned long long d_words[kBlankDRowsMax], b_words[kBlankBRows];
    __shared__ unsigned d_before[kBlankDRowsMax];          // D set in the words in front of this one
    __shared__ unsigned row_total[kBlankIters * kBlankWaves], wave_total[kBlankWaves];
    __shared__ unsigned sums[kBlankWaves][2 * kBlankTileBlocks];
    __shared__ unsigned b_prev;                            // B of the sample in front of the tile
    unsigned* const P = p_lds + 4;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* const src = iq + 2 * g.first_sample;
    const long long n = (long long)g.n_samples;
    const int W = g.window, G = g.guard, h = W / 2;
    const int n_chunks = (g.halo_left + kBlankTile + g.halo_right) / 8;
    const int d_left = G + 1;                              // D word bit y is sample t0 - d_left + y
    const int d_ext = d_left + kBlankTile + G;
    const int d_rows = (d_ext + 63) / 64;

    // D set among the bits 0 .. y of the D words; y = -1: none
    const auto d_upto = [&](int y) -> unsigned {
        if (y < 0) return 0u;
        return d_before[y >> 6] + (unsigned)__popcll(d_words[y >> 6] & (~0ull >> (63 - (y & 63))));
    };

    for (unsigned long long tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const long long t0 = (long long)(tile * (unsigned long long)kBlankTile);

        // ---- 1. chunks -> e -> P
        unsigned raw[kBlankIters][4], q[kBlankIters][8], before[kBlankIters];
#pragma unroll
        for (int j = 0; j < kBlankIters; ++j) {
            const int c = j * kBlankThreads + tid;
            const long long t = t0 - g.halo_left + 8 * c;
            blank_load(raw[j], src, t, c < n_chunks ? n : 0);
            // samples lo <= s < hi of the chunk lie in the range
            const int lo = t >= 0 ? 0 : (t <= -8 ? 8 : (int)-t);
            const int hi = c >= n_chunks || t >= n ? 0 : (n - t >= 8 ? 8 : (int)(n - t));
            unsigned run = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                run += s >= lo && s < hi ? blank_e(raw[j], s, g.o2) : 0u;
                q[j][s] = run;
            }
            const unsigned inc = wave_scan_u32(run, lane);
            before[j] = inc - run;
            if (lane == 63) row_total[j * kBlankWaves + wave] = inc;
        }
        __syncthreads();
        {
            unsigned carry = 0;
#pragma unroll
            for (int j = 0; j < kBlankIters; ++j) {
                unsigned base = carry + before[j];
#pragma unroll
                for (int w = 0; w < kBlankWaves; ++w) {
                    const unsigned v = row_total[j * kBlankWaves + w];
                    base += w < wave ? v : 0u;
                    carry += v;
                }
                uint4* dst = reinterpret_cast<uint4*>(P + 8 * (j * kBlankThreads + tid));
                dst[0] = uint4{base + q[j][0], base + q[j][1], base + q[j][2], base + q[j][3]};
                dst[1] = uint4{base + q[j][4], base + q[j][5], base + q[j][6], base + q[j][7]};
            }
            if (tid == 0) P[-1] = 0u;
        }
        __syncthreads();

        // ---- 2. D, a lane per sample, 64 to a word
        for (int r = wave; r < d_rows; r += kBlankWaves) {
            const int y = r * 64 + lane;
            const long long t = t0 - d_left + y;
            bool d = false;
            if (y < d_ext && t >= 0 && t < n) {
                const int x = y - d_left + g.halo_left;    // >= h: halo_left >= h + G + 1
                d = P[x - h + W - 1] - P[x - h - 1] > g.T;
            }
            const unsigned long long word = __ballot(d);
            if (lane == 0) d_words[r] = word;
        }
        __syncthreads();

        // ---- 3. D set in front of every word, then B
        {
            const unsigned cnt = tid < d_rows ? (unsigned)__popcll(d_words[tid]) : 0u;
            const unsigned inc = wave_scan_u32(cnt, lane);
            if (lane == 63) wave_total[wave] = inc;
            __syncthreads();
            unsigned base = inc - cnt;
#pragma unroll
            for (int w = 0; w < kBlankWaves; ++w) base += w < wave ? wave_total[w] : 0u;
            if (tid < d_rows) d_before[tid] = base;
        }
        __syncthreads();
        for (int r = wave; r < kBlankBRows; r += kBlankWaves) {
            const int k = r * 64 + lane;                   // sample t0 + k, bit y = k + d_left of the D words
            const int y = k + d_left;
            const bool b = t0 + k < n && d_upto(y + G) != d_upto(y - G - 1);   // y + G <= d_ext - 1
            const unsigned long long word = __ballot(b);
            if (lane == 0) b_words[r] = word;
        }
        if (tid == 0) b_prev = t0 > 0 && d_upto(2 * G) != 0u ? 1u : 0u;   // sample t0 - 1 is bit G
        __syncthreads();

        // ---- 4. the tile's chunks out
        unsigned tot0 = 0, tot1 = 0, rem0 = 0, rem1 = 0;
#pragma unroll
        for (int j = 0; j < kBlankIters; ++j) {
            const int k0 = 8 * (j * kBlankThreads + tid) - g.halo_left;   // a multiple of 8
            if (k0 < 0 || k0 >= kBlankTile || t0 + k0 >= n) continue;
            const long long t = t0 + k0;
            const int nv = n - t >= 8 ? 8 : (int)(n - t);
            const unsigned bits = reinterpret_cast<const uint8_t*>(b_words)[k0 >> 3];   // never set for a sample past n
            unsigned tot = 0, rem = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const unsigned e = s < nv ? blank_e(raw[j], s, g.o2) : 0u;
                tot += e;
                rem += (bits >> s) & 1u ? e : 0u;
            }
            const bool second = k0 >= GJ_BLANK_BLOCK;
            tot0 += second ? 0u : tot, rem0 += second ? 0u : rem;
            tot1 += second ? tot : 0u, rem1 += second ? rem : 0u;
            unsigned o[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned m = ((bits >> (2 * d)) & 1u ? 0x0000ffffu : 0u) | ((bits >> (2 * d + 1)) & 1u ? 0xffff0000u : 0u);
                o[d] = (raw[j][d] & ~m) | (g.blank_pair & m);
            }
            uint8_t* dst = out + 2 * t;
            if (nv == 8 && g.out_aligned) {
                *reinterpret_cast<uint4*>(dst) = uint4{o[0], o[1], o[2], o[3]};
            } else {   // the ragged end, or an output that is not 16-byte aligned
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (i < 2 * nv) dst[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
            }
        }

        // ---- 5. records: wave b holds the 64 B words of the tile's block b
        unsigned n_blanked = 0, n_rising = 0;
        if (tid < kBlankBRows) {
            const unsigned long long word = b_words[tid];
            const unsigned long long prev = tid == 0 ? (unsigned long long)b_prev : b_words[tid - 1] >> 63;
            n_blanked = (unsigned)__popcll(word);
            n_rising = (unsigned)__popcll(word & ~((word << 1) | prev));
        }
        n_blanked = wave_sum_u32(n_blanked);
        n_rising = wave_sum_u32(n_rising);
        tot0 = wave_sum_u32(tot0), tot1 = wave_sum_u32(tot1), rem0 = wave_sum_u32(rem0), rem1 = wave_sum_u32(rem1);
        if (lane == 0) sums[wave][0] = tot0, sums[wave][1] = tot1, sums[wave][2] = rem0, sums[wave][3] = rem1;
        __syncthreads();   // also the end of the tile: every LDS array is rewritten only behind a later barrier's wait
        const unsigned long long block = tile * kBlankTileBlocks + (unsigned)wave;
        if (blocks && lane == 0 && wave < kBlankTileBlocks && block < g.n_blocks) {
            unsigned total = 0, removed = 0;   // a block's sum of e fits at every offset: 4096 * 2 * 510^2 = 2 130 739 200 at most (offsets 0, 255)
#pragma unroll
            for (int w = 0; w < kBlankWaves; ++w) total += sums[w][wave], removed += sums[w][kBlankTileBlocks + wave];
            gj_blank_block rec;
            rec.total = total;
            rec.removed = removed;
            rec.n_blanked = (int32_t)n_blanked;
            rec.n_rising = (int32_t)n_rising;
            blocks[block] = rec;
        }
    }
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_blank_blocks(size_t n_samples) { return n_samples / GJ_BLANK_BLOCK + (n_samples % GJ_BLANK_BLOCK != 0); }

int gj_blank_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int window, int guard,
                 float threshold, uint8_t* d_out, gj_blank_block* d_blocks) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (window < 1 || window > kBlankMaxWindow) return fail(ctx, GJ_ERR_UNSUPPORTED, "window %d (1 .. %d)", window, kBlankMaxWindow);
    if (guard < 0 || guard > kBlankMaxGuard) return fail(ctx, GJ_ERR_UNSUPPORTED, "guard %d (0 .. %d)", guard, kBlankMaxGuard);
    if (!d_iq || !d_out) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (reinterpret_cast<uintptr_t>(d_iq) & 1) return fail(ctx, GJ_ERR_INVALID, "capture must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_blocks) & 7) return fail(ctx, GJ_ERR_INVALID, "records must be 8-byte aligned");
    if (!(threshold >= 0.f)) return fail(ctx, GJ_ERR_INVALID, "threshold must be a number >= 0");
    if (n_samples == 0) return fail(ctx, GJ_ERR_INVALID, "n_samples is 0");
    if (int rc = check_range_and_output(ctx, d_iq, nbytes, first_sample, n_samples, d_out)) return rc;
    BlankGeom g;
    g.first_sample = first_sample;
    g.n_samples = n_samples;
    g.n_tiles = (n_samples + kBlankTile - 1) / kBlankTile;
    g.n_blocks = gj_blank_blocks(n_samples);
    g.window = window;
    g.guard = guard;
    g.halo_left = round_up8(window / 2 + guard + 1);
    g.halo_right = round_up8(window - 1 - window / 2 + guard);
    g.o2 = ctx->off2;
    // exact in double: 4 W has 12 bits, a float 24.  +inf and everything from 2^32 - 1 on never blank
    const double t = std::floor(4.0 * (double)window * (double)threshold);
    g.T = t >= 4294967295.0 ? 0xffffffffu : (unsigned)t;
    {   // with an odd o2 the two nearest bytes alternate on the ABSOLUTE sample index; a chunk starts on an even t
        const unsigned odd = (unsigned)g.o2 & 1u, base = ((unsigned)g.o2 - odd) / 2, p = (unsigned)(first_sample & 1) & odd;
        const unsigned i0 = base + p, q0 = base + odd - p;   // I and Q of an even t; an odd t has them swapped
        g.blank_pair = i0 | (q0 << 8) | (q0 << 16) | (i0 << 24);
    }
    g.out_aligned = (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
    const unsigned grid = (unsigned)(g.n_tiles < (1ull << 20) ? g.n_tiles : (1ull << 20));   // longer ranges loop in the workgroup
    hipLaunchKernelGGL(blank_kernel, dim3(grid), dim3(kBlankThreads), 0, ctx->stream, d_iq, g, d_out, d_blocks);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
