// Counterfeit-signal subtraction (gfx950): gj_subtract_dev / gj_subtract_blocks of include/gpsjam.h, which states the
// definition.  The correlator bank (k_corr.hip) run backwards: the replica a c (C - jS) of every channel is rebuilt from
// its code, its carrier and one complex amplitude per block, the replicas are added up, brought down to LSB by a
// dithered floor and taken off the bytes.  Integer arithmetic from the amplitude to the byte, so every byte and every
// record is the definition's whatever the tiling.
//
// A workgroup of four waves owns tiles of 4096 samples, one record each, whatever B is.  Thread tid owns the 16
// consecutive samples 16 tid .. 16 tid + 15 of the tile; B is a multiple of 16 and a tile starts on a multiple of 16,
// so a thread's samples lie in ONE block: one amplitude pair per channel and thread.
//   0. once per workgroup: the channels are checked, kept in LDS and their code rows packed to sign bits (replica.h);
//   1. per tile: the thread's 32 bytes come from the capture ONCE (replica.h);
//   2. per channel: the amplitude pair of the thread's block, clamped; the first code phase by one 64-bit multiply and
//      a mod, the others by exact steps; the chip's sign picks +-a, and the table entry (C, S) at theta >> 28 turns
//      it: four multiply-adds into the sample's two accumulators.  Only tap 0 exists: no LDS code table, no barrier
//      per channel;
//   3. per sample and component: d (32768, or the hash of the absolute index), q = (R + d) >> 16 (arithmetic: the
//      floor), the byte less q, clamped; the 32 bytes leave as two 16-byte stores where d_out is 16-byte aligned and
//      the run is whole, byte by byte otherwise;
//   4. the record, if asked for: total, removed and n_clipped of the thread's samples, a wave sum each, one LDS word
//      per wave and field, and thread 0 adds the four and stores the record: no atomics, no workspace.
//
// Widths.  |a| <= 2^19 after the clamp and |C[i]| + |S[i]| <= 46: a channel adds at most 2^19 * 46 to |R|, 64 channels
// 1 543 503 872, and with d <= 65535 on top R + d <= 1 543 569 407 < 2^31: int32 is exact, partial sums included.  A
// tile's total is at most 4096 * 2 * 128^2 = 2^27 and its removed at most 4096 * 2 * 255^2 = 532 684 800: uint32.  The
// channel fields, the code phase and its widths: replica.h.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it.
#include "replica.h"

namespace gj {

constexpr int kSubWaves = kReplicaThreads / 64;

static_assert(kReplicaTile == GJ_SUB_BLOCK, "one record per tile");
static_assert(sizeof(gj_subtract_block) == 24, "the header's layout");
// |R| <= channels * max amplitude * max(|C| + |S|), and the dither adds less than 2^GJ_SUB_FRAC
static_assert((long long)GJ_CORR_MAX_CHANNELS * GJ_SUB_MAX_AMP * 46 + (1ll << GJ_SUB_FRAC) - 1 < (1ll << 31), "R + d fits int32");
static_assert(GJ_SUB_FRAC == 16, "d is the hash's upper half");
static_assert(4096ll * 2 * 255 * 255 < (1ll << 32), "a tile's sums fit uint32");

struct SubGeom {
    unsigned long long first_sample, n_samples, n_blocks, n_tiles;
    int block_samples;           // B
    int n_code_rows, n_channels;
    int dither;
    unsigned seed;
    int out_aligned;             // d_out is 16-byte aligned
};

__device__ __forceinline__ int sub_clamp_amp(int v) { return v < -GJ_SUB_MAX_AMP ? -GJ_SUB_MAX_AMP : (v > GJ_SUB_MAX_AMP ? GJ_SUB_MAX_AMP : v); }

// the header's d for component `comp` of absolute sample `sample`
__device__ __forceinline__ int sub_dither(unsigned long long sample, unsigned comp, unsigned seed) {
    const unsigned long long k = 2ull * sample + comp;
    unsigned v = (unsigned)k ^ ((unsigned)(k >> 32) * 0x9e3779b9u) ^ seed;
    v ^= v >> 16;
    v *= 0x7feb352du;
    v ^= v >> 15;
    v *= 0x846ca68bu;
    v ^= v >> 16;
    return (int)(v >> 16);
}

__global__ __launch_bounds__(kReplicaThreads) void subtract_kernel(const uint8_t* __restrict__ iq, SubGeom g,
                                                                   const int16_t* __restrict__ codes,
                                                                   const gj_corr_channel* __restrict__ channels,
                                                                   const int32_t* __restrict__ amp, uint8_t* __restrict__ out,
                                                                   gj_subtract_block* __restrict__ blocks) {
    __shared__ gj_corr_channel chan[GJ_CORR_MAX_CHANNELS];
    __shared__ unsigned code_bits[GJ_CORR_MAX_CHANNELS][32];         // bit c of word w: chip 32 w + c is -1
    __shared__ int2 mix[16];                                         // (C, S)
    __shared__ unsigned sums[kSubWaves][3];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- 0. channels: checked, kept, their code rows packed
    int bad = 0;
    if (tid < g.n_channels) {
        const gj_corr_channel c = channels[tid];
        bad = GJ_REPLICA_CHANNEL_BAD(c, g.n_code_rows);
        chan[tid] = c;
    }
    if (tid < 16) {
        constexpr int kCos[16] = GJ_CORR_COS_TABLE;
        int c = 0, s = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i == tid) c = kCos[i];
            if (((i + 4) & 15) == tid) s = kCos[i];                  // S[tid] = C[(tid - 4) & 15]
        }
        mix[tid] = int2{c, s};
    }
    if (__syncthreads_or(bad)) return;
    replica_pack_codes(codes, chan, code_bits, g.n_channels, wave, lane);
    __syncthreads();

    const long long n = (long long)g.n_samples;
    const uint8_t* const src = iq + 2 * g.first_sample;

    for (unsigned long long tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const long long t0 = (long long)(tile * (unsigned long long)kReplicaTile) + kReplicaRun * tid;   // this thread's first sample
        const int nv = t0 >= n ? 0 : (n - t0 >= kReplicaRun ? kReplicaRun : (int)(n - t0));             // its samples inside the range
        unsigned total = 0, removed = 0, clipped = 0;

        if (nv > 0) {
            // ---- 1. the thread's bytes
            unsigned raw[kReplicaRun / 2];
            if (nv == kReplicaRun)
                replica_load_run(src + 2 * t0, raw);
            else {
#pragma unroll
                for (int p = 0; p < kReplicaRun / 2; ++p) raw[p] = 0u;
#pragma unroll
                for (int s = 0; s < kReplicaRun; ++s)
                    if (s < nv) raw[s >> 1] |= (unsigned)*reinterpret_cast<const uint16_t*>(src + 2 * (t0 + s)) << (16 * (s & 1));
            }

            // ---- 2. the replicas of every channel, added up
            int ri[kReplicaRun], rq[kReplicaRun];
#pragma unroll
            for (int s = 0; s < kReplicaRun; ++s) ri[s] = rq[s] = 0;
            const unsigned long long block = (unsigned)t0 / (unsigned)g.block_samples;          // t0 < 2^28
            for (int ch = 0; ch < g.n_channels; ++ch) {
                const gj_corr_channel c = chan[ch];
                const int32_t* const a = amp + 2 * ((unsigned long long)ch * g.n_blocks + block);
                const int a_i = sub_clamp_amp(a[0]), a_q = sub_clamp_amp(a[1]);
                const unsigned* const bits = code_bits[ch];
                unsigned long long ph = replica_mod_period(c.code_phase + (unsigned long long)t0 * c.code_step);
                unsigned theta = c.carr_phase + (unsigned)t0 * c.carr_step;
#pragma unroll
                for (int s = 0; s < kReplicaRun; ++s) {
                    const bool neg = replica_chip_neg(bits, ph);
                    const int s_i = neg ? -a_i : a_i, s_q = neg ? -a_q : a_q;
                    const int2 m = mix[theta >> 28];
                    ri[s] += s_i * m.x + s_q * m.y;
                    rq[s] += s_q * m.x - s_i * m.y;
                    ph = replica_step(ph, c.code_step);
                    theta += c.carr_step;
                }
            }

            // ---- 3. down to LSB, off the bytes
            unsigned o[kReplicaRun / 2];
#pragma unroll
            for (int p = 0; p < kReplicaRun / 2; ++p) o[p] = 0u;
#pragma unroll
            for (int s = 0; s < kReplicaRun; ++s) {
                const unsigned long long sample = g.first_sample + (unsigned long long)t0 + (unsigned)s;
#pragma unroll
                for (int comp = 0; comp < 2; ++comp) {
                    const int shift = 16 * (s & 1) + 8 * comp;
                    const int in = (int)((raw[s >> 1] >> shift) & 0xffu);
                    const int d = g.dither ? sub_dither(sample, (unsigned)comp, g.seed) : 1 << (GJ_SUB_FRAC - 1);
                    const int q = ((comp ? rq[s] : ri[s]) + d) >> GJ_SUB_FRAC;               // arithmetic shift: the floor
                    const int want = in - q;
                    const int got = want < 0 ? 0 : (want > 255 ? 255 : want);
                    o[s >> 1] |= (unsigned)got << shift;
                    if (s < nv) {
                        total += (unsigned)((in - 128) * (in - 128));
                        removed += (unsigned)((in - got) * (in - got));
                        clipped += got != want ? 1u : 0u;
                    }
                }
            }
            uint8_t* const dst = out + 2 * t0;
            if (nv == kReplicaRun && g.out_aligned) {
                reinterpret_cast<uint4*>(dst)[0] = uint4{o[0], o[1], o[2], o[3]};
                reinterpret_cast<uint4*>(dst)[1] = uint4{o[4], o[5], o[6], o[7]};
            } else {   // the ragged end, or an output that is not 16-byte aligned
#pragma unroll
                for (int i = 0; i < 2 * kReplicaRun; ++i)
                    if (i < 2 * nv) dst[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
            }
        }

        // ---- 4. the tile's record
        if (blocks) {   // the same in every thread
            total = wave_sum_u32(total), removed = wave_sum_u32(removed), clipped = wave_sum_u32(clipped);
            if (lane == 0) sums[wave][0] = total, sums[wave][1] = removed, sums[wave][2] = clipped;
            __syncthreads();
            if (tid == 0) {
                gj_subtract_block rec;
                rec.total = 0, rec.removed = 0, rec.n_clipped = 0, rec.reserved = 0;
#pragma unroll
                for (int w = 0; w < kSubWaves; ++w) rec.total += sums[w][0], rec.removed += sums[w][1], rec.n_clipped += (int32_t)sums[w][2];
                blocks[tile] = rec;
            }
            __syncthreads();   // the next tile's sums are written behind thread 0's reads
        }
    }
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_subtract_blocks(size_t n_samples) { return n_samples / GJ_SUB_BLOCK + (n_samples % GJ_SUB_BLOCK != 0); }

int gj_subtract_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int block_samples,
                    const int16_t* d_codes, int n_code_rows, const gj_corr_channel* d_channels, int n_channels,
                    const int32_t* d_amp, int flags, uint32_t seed, uint8_t* d_out, gj_subtract_block* d_blocks) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (!d_iq || !d_codes || !d_channels || !d_amp || !d_out) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = replica_check_alignment(ctx, d_iq, d_codes, d_channels)) return rc;
    if (reinterpret_cast<uintptr_t>(d_amp) & 3) return fail(ctx, GJ_ERR_INVALID, "amplitudes must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_blocks) & 7) return fail(ctx, GJ_ERR_INVALID, "records must be 8-byte aligned");
    if (n_code_rows < 1) return fail(ctx, GJ_ERR_INVALID, "n_code_rows %d", n_code_rows);
    if (flags & ~GJ_SUB_DITHER) return fail(ctx, GJ_ERR_INVALID, "unknown flags 0x%x", (unsigned)flags);
    if (int rc = replica_check_block(ctx, block_samples)) return rc;
    if (int rc = replica_check_counts(ctx, n_channels, n_samples)) return rc;
    if (int rc = check_range_and_output(ctx, d_iq, nbytes, first_sample, n_samples, d_out)) return rc;
    SubGeom g;
    g.first_sample = first_sample;
    g.n_samples = n_samples;
    g.block_samples = block_samples;
    g.n_blocks = gj_corr_blocks(n_samples, block_samples);
    g.n_tiles = gj_subtract_blocks(n_samples);
    g.n_code_rows = n_code_rows;
    g.n_channels = n_channels;
    g.dither = (flags & GJ_SUB_DITHER) != 0;
    g.seed = seed;
    g.out_aligned = (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
    const unsigned grid = replica_grid(ctx, 4, g.n_tiles);   // the kernel's 124 registers allow four waves per SIMD
    hipLaunchKernelGGL(subtract_kernel, dim3(grid), dim3(kReplicaThreads), 0, ctx->stream, d_iq, g, d_codes, d_channels, d_amp,
                       d_out, d_blocks);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
