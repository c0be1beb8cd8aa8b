// Subtraction of TRACKED signals (gfx950): gj_subtract_track_dev of include/gpsjam.h, which states the definition.
// gj_subtract_dev (k_subtract.hip) with another source for the replica's NCOs: not one channel per call but one record
// per channel and EPOCH, as gj_track_dev wrote them, and one amplitude pair per epoch.  Stages 1, 3 and 4 below are
// k_subtract.hip's, statement for statement, so that d, q, the byte and the record are its own; they are repeated here
// and not shared, because that kernel's instructions are pinned (profiles/NOTES_replica.md) and a helper moves them.
//
// A workgroup of four waves owns tiles of 4096 samples; thread tid owns the 16 samples from 16 tid of the tile.
//   0. once per workgroup: the channel table is checked (code_row, start + E B <= n) and kept in LDS, the code rows
//      are packed to sign bits (replica.h);
//   1. per tile: the thread's 32 bytes, ONCE; and lane l of every wave places the TILE on channel l's epoch grid:
//      R0 = tile start - start[l], M0 = floor(R0 / B), U0 = R0 - M0 B -- the only division by B, one per lane and tile,
//      handed to the channel loop by v_readlane;
//   2. per channel: x = U0 + 16 tid < B + 4096 and m = M0 + floor(x / B) by one v_mul_hi with ceil(2^32 / B) (exact for
//      x B < 2^32), u = x mod B.  An epoch grid starts anywhere, so the run is cut at k = min(16, B - u): samples
//      0 .. k-1 belong to epoch m, samples k .. 15 to epoch m + 1 at u = 0; B >= 16, so there is no third.  An epoch
//      outside 0 .. E-1 or with a bad record is SILENT: amplitude 0, phase 0, step 0, which adds exactly nothing.
//      A segment costs its record's 24 bytes (every thread of an epoch reads the same ones), two amplitudes, and for
//      u > 0 one 64-bit multiply and a mod.  Where no lane of the WAVE is cut (k = 16 everywhere) the inner loop is
//      k_subtract.hip's; where one is, the wave runs the same loop with the segment swapped at s == k (eight selects per
//      sample).  A wave in which the channel is silent throughout skips it;
//   3. per sample and component: d, q = (R + d) >> 16, the byte less q, clamped, two 16-byte stores or byte by byte;
//   4. the record: wave sums, one LDS word per wave and field, thread 0 stores it.  No atomics, no workspace.
//
// Widths.  u < 4096 and code_step < 2^34: u code_step < 2^46, and with code_phase < 2^42 the sum is far below 2^63
// (replica_mod_period).  start + E B <= n <= 2^28 once the table is checked: R0, x and m fit int.  |R| is bounded as in
// k_subtract.hip: 64 channels, |a| <= 2^19, |C| + |S| <= 46.
//
// This is a translation unit of its own with its own extern "C" entry point: none of the other sources refers to it.
#include "replica.h"

namespace gj {

constexpr int kSubWaves = kReplicaThreads / 64;

static_assert(kReplicaTile == GJ_SUB_BLOCK, "one record per tile");
static_assert(sizeof(gj_subtract_block) == 24, "the header's layout");
static_assert(sizeof(gj_subtract_track_channel) == 8, "the header's layout");
static_assert(sizeof(gj_track_epoch) == 56 && offsetof(gj_track_epoch, carr_phase) == 24 && offsetof(gj_track_epoch, code_phase) == 32,
              "the four NCO fields are 24 bytes at offset 24");
static_assert((long long)GJ_CORR_MAX_CHANNELS * GJ_SUB_MAX_AMP * 46 + (1ll << GJ_SUB_FRAC) - 1 < (1ll << 31), "R + d fits int32");
static_assert(GJ_SUB_FRAC == 16, "d is the hash's upper half");
static_assert(4096ll * 2 * 255 * 255 < (1ll << 32), "a tile's sums fit uint32");
static_assert(GJ_CORR_MAX_CHANNELS == 64, "one lane of a wave per channel");
static_assert((long long)(GJ_CORR_MAX_BLOCK + kReplicaTile) * GJ_CORR_MAX_BLOCK < (1ll << 32), "x / B by one multiply");

struct SubTrackGeom {
    unsigned long long first_sample, n_samples, n_tiles;
    unsigned long long cover;    // E B
    int block_samples;           // B
    unsigned inv_block;          // floor(2^32 / B) + 1
    int n_epochs;                // E
    int n_code_rows, n_channels;
    int dither;
    unsigned seed;
    int out_aligned;             // d_out is 16-byte aligned
};

// one channel's NCOs and amplitudes along a piece of a thread's run
struct SubTrackSeg {
    unsigned long long ph, code_step;   // ph: reduced
    unsigned theta, carr_step;
    int a_i, a_q;
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

// The segment that starts u samples into epoch m of a channel whose records and amplitudes begin at rec and amp; silent
// (all zero) unless `live`, and where the record's code NCO is out of bounds.  m is only used where live.
__device__ __forceinline__ SubTrackSeg sub_track_segment(const gj_track_epoch* __restrict__ rec, const int32_t* __restrict__ amp,
                                                         bool live, int m, unsigned u) {
    SubTrackSeg s{0ull, 0ull, 0u, 0u, 0, 0};
    if (live) {
        const gj_track_epoch* const r = rec + m;
        const unsigned long long code_phase = r->code_phase, code_step = r->code_step;
        if (code_phase < kReplicaPeriod && code_step < GJ_CORR_MAX_CODE_STEP) {
            const unsigned carr_phase = r->carr_phase;
            s.code_step = code_step;
            s.carr_step = r->carr_step;
            s.ph = u ? replica_mod_period(code_phase + (unsigned long long)u * code_step) : code_phase;
            s.theta = carr_phase + u * s.carr_step;
            s.a_i = sub_clamp_amp(amp[2 * m]);
            s.a_q = sub_clamp_amp(amp[2 * m + 1]);
        }
    }
    return s;
}

// One channel's replica over a thread's run, added to the accumulators: k_subtract.hip's inner loop.  kCut: from
// sample k on the run continues with segment `next`.
template <bool kCut>
__device__ __forceinline__ void sub_track_add(int (&ri)[kReplicaRun], int (&rq)[kReplicaRun], const unsigned* bits, const int2* mix,
                                              SubTrackSeg g, const SubTrackSeg& next, int k) {
#pragma unroll
    for (int s = 0; s < kReplicaRun; ++s) {
        if (kCut && s > 0) {   // k >= 1.  Field by field: as `if (s == k) g = next` this becomes 15 branches and 202 registers
            const bool cut = s == k;
            g.ph = cut ? next.ph : g.ph, g.code_step = cut ? next.code_step : g.code_step;
            g.theta = cut ? next.theta : g.theta, g.carr_step = cut ? next.carr_step : g.carr_step;
            g.a_i = cut ? next.a_i : g.a_i, g.a_q = cut ? next.a_q : g.a_q;
        }
        const bool neg = replica_chip_neg(bits, g.ph);
        const int s_i = neg ? -g.a_i : g.a_i, s_q = neg ? -g.a_q : g.a_q;
        const int2 m = mix[g.theta >> 28];
        ri[s] += s_i * m.x + s_q * m.y;
        rq[s] += s_q * m.x - s_i * m.y;
        g.ph = replica_step(g.ph, g.code_step);
        g.theta += g.carr_step;
    }
}

__global__ __launch_bounds__(kReplicaThreads) void subtract_track_kernel(const uint8_t* __restrict__ iq, SubTrackGeom g,
                                                                         const int16_t* __restrict__ codes,
                                                                         const gj_subtract_track_channel* __restrict__ channels,
                                                                         const gj_track_epoch* __restrict__ epochs,
                                                                         const int32_t* __restrict__ amp, uint8_t* __restrict__ out,
                                                                         gj_subtract_block* __restrict__ blocks) {
    __shared__ gj_corr_channel chan[GJ_CORR_MAX_CHANNELS];          // code_row alone is used: what replica_pack_codes reads
    __shared__ int start[GJ_CORR_MAX_CHANNELS];
    __shared__ unsigned code_bits[GJ_CORR_MAX_CHANNELS][32];         // bit c of word w: chip 32 w + c is -1
    __shared__ int2 mix[16];                                         // (C, S)
    __shared__ unsigned sums[kSubWaves][3];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- 0. the channel table: checked, kept, the code rows packed
    int bad = 0;
    if (tid < g.n_channels) {
        const gj_subtract_track_channel c = channels[tid];
        bad = c.code_row < 0 || c.code_row >= g.n_code_rows || (unsigned long long)c.start + g.cover > g.n_samples;
        chan[tid] = gj_corr_channel{0ull, 0ull, 0u, 0u, c.code_row, 0};
        start[tid] = (int)c.start;                                   // < 2^28 where the table is good
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
    const int B = g.block_samples, E = g.n_epochs;
    const int my_start = lane < g.n_channels ? start[lane] : 0;      // lane l answers for channel l

    for (unsigned long long tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tile0 = (int)(tile * (unsigned long long)kReplicaTile);                               // < 2^28
        const long long t0 = (long long)tile0 + kReplicaRun * tid;                                      // this thread's first sample
        const int nv = t0 >= n ? 0 : (n - t0 >= kReplicaRun ? kReplicaRun : (int)(n - t0));             // its samples inside the range
        unsigned total = 0, removed = 0, clipped = 0;

        // the tile on channel `lane`'s epoch grid: floor and remainder of tile0 - start by B
        const int r0 = tile0 - my_start;
        const int my_m0 = r0 >= 0 ? (int)((unsigned)r0 / (unsigned)B) : -(int)(((unsigned)-r0 + (unsigned)B - 1u) / (unsigned)B);
        const int my_u0 = r0 - my_m0 * B;                            // 0 .. B-1

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

        // ---- 2. the replicas of every channel, added up.  EVERY thread walks the channels, those behind the range's end
        // too (their sums are never stored): v_readlane reads lane ch whatever EXEC says, so lane ch must have run the
        // lines above, and inside a branch on nv it has not where its own samples lie behind the end.
        int ri[kReplicaRun], rq[kReplicaRun];
#pragma unroll
        for (int s = 0; s < kReplicaRun; ++s) ri[s] = rq[s] = 0;
        for (int ch = 0; ch < g.n_channels; ++ch) {
            const int m0 = __builtin_amdgcn_readlane(my_m0, ch), u0 = __builtin_amdgcn_readlane(my_u0, ch);
            const unsigned x = (unsigned)u0 + (unsigned)(kReplicaRun * tid);
            const unsigned dm = __umulhi(x, g.inv_block);                                       // floor(x / B)
            const int m = m0 + (int)dm;
            const unsigned u = x - dm * (unsigned)B;
            const int k = (unsigned)B - u < (unsigned)kReplicaRun ? (int)((unsigned)B - u) : kReplicaRun;
            const bool live = m >= 0 && m < E;                                                  // samples 0 .. k-1
            const bool live_next = k < kReplicaRun && m + 1 >= 0 && m + 1 < E;                  // samples k .. 15
            if (!__any(live || live_next)) continue;                                            // silent for the whole wave
            const gj_track_epoch* const rec = epochs + (size_t)ch * (size_t)E;
            const int32_t* const a = amp + 2 * (size_t)ch * (size_t)E;
            const unsigned* const bits = code_bits[ch];
            const SubTrackSeg seg = sub_track_segment(rec, a, live, m, u);
            if (__any(k < kReplicaRun)) {
                const SubTrackSeg next = sub_track_segment(rec, a, live_next, m + 1, 0u);
                sub_track_add<true>(ri, rq, bits, mix, seg, next, k);
            } else
                sub_track_add<false>(ri, rq, bits, mix, seg, seg, kReplicaRun);
        }

        if (nv > 0) {
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

int gj_subtract_track_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int block_samples,
                          int n_epochs, const int16_t* d_codes, int n_code_rows, const gj_subtract_track_channel* d_channels,
                          int n_channels, const gj_track_epoch* d_epochs, const int32_t* d_amp, int flags, uint32_t seed,
                          uint8_t* d_out, gj_subtract_block* d_blocks) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (!d_iq || !d_codes || !d_channels || !d_epochs || !d_amp || !d_out) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if ((reinterpret_cast<uintptr_t>(d_iq) | reinterpret_cast<uintptr_t>(d_codes)) & 1)
        return fail(ctx, GJ_ERR_INVALID, "the capture and the codes must be 2-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_channels) | reinterpret_cast<uintptr_t>(d_epochs)) & 7)
        return fail(ctx, GJ_ERR_INVALID, "channels and epoch records must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_amp) & 3) return fail(ctx, GJ_ERR_INVALID, "amplitudes must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_blocks) & 7) return fail(ctx, GJ_ERR_INVALID, "records must be 8-byte aligned");
    if (n_code_rows < 1) return fail(ctx, GJ_ERR_INVALID, "n_code_rows %d", n_code_rows);
    if (flags & ~GJ_SUB_DITHER) return fail(ctx, GJ_ERR_INVALID, "unknown flags 0x%x", (unsigned)flags);
    if (int rc = replica_check_block(ctx, block_samples)) return rc;
    if (int rc = replica_check_counts(ctx, n_channels, n_samples)) return rc;
    if (n_epochs < 1) return fail(ctx, GJ_ERR_UNSUPPORTED, "n_epochs %d (at least 1)", n_epochs);
    const unsigned long long cover = (unsigned long long)n_epochs * (unsigned)block_samples;
    if (cover > n_samples) return fail(ctx, GJ_ERR_INVALID, "%d epochs of %d samples run past n_samples %zu", n_epochs, block_samples, n_samples);
    if (int rc = check_range_and_output(ctx, d_iq, nbytes, first_sample, n_samples, d_out)) return rc;
    SubTrackGeom g;
    g.first_sample = first_sample;
    g.n_samples = n_samples;
    g.n_tiles = gj_subtract_blocks(n_samples);
    g.cover = cover;
    g.block_samples = block_samples;
    g.inv_block = (unsigned)((1ull << 32) / (unsigned)block_samples) + 1u;
    g.n_epochs = n_epochs;
    g.n_code_rows = n_code_rows;
    g.n_channels = n_channels;
    g.dither = (flags & GJ_SUB_DITHER) != 0;
    g.seed = seed;
    g.out_aligned = (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
    const unsigned grid = replica_grid(ctx, 4, g.n_tiles);
    hipLaunchKernelGGL(subtract_track_kernel, dim3(grid), dim3(kReplicaThreads), 0, ctx->stream, d_iq, g, d_codes, d_channels, d_epochs,
                       d_amp, d_out, d_blocks);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
