// Correlator bank (gfx950): gj_corr_bank_dev / gj_corr_blocks of include/gpsjam.h, which states the definition.  Every
// channel and tap of a batch correlated over a whole range in one launch: integer arithmetic from the byte to the sum,
// so every record is the definition's whatever the tiling and the order.
//
// A workgroup of four waves owns tiles of k = floor(4096 / B) whole record blocks (k B <= 4096 samples).  Thread tid owns
// the 16 consecutive samples 16 tid .. 16 tid + 15 of the tile; B is a multiple of 16 and a tile starts on a block, so a
// thread's samples lie in ONE block.
//   0. once per workgroup: the channels are checked, kept in LDS and their code rows packed to sign bits (replica.h);
//   1. per tile: the thread's 32 bytes come from the capture ONCE (replica.h), are unpacked to (I - 128, Q - 128) as
//      two int16 in one word and stay in registers for every channel and tap: HBM traffic is one pass over the range
//      per call.  Samples past n_samples are the sample zero;
//   2. per channel: the resampled code of samples tile - 64 .. tile + 4096 + 64 is made once, as +-1 int16, in LDS: a
//      thread makes 18 consecutive entries, the first phase by one 64-bit multiply and a mod, the others by exact
//      steps (replica.h).  Every tap is then a whole-sample shift of these entries, the reference's code +- s[i] pointers;
//   3. the carrier: theta = carr_phase + t carr_step in uint32 (wraps as the definition's mod 2^32), the table entry
//      (C, -S), (S, C) as one 8-byte LDS read, wI and wQ by one v_dot2_i32_i16 each.  |w| <= 5888 is an int16, so two
//      samples' wI (and wQ) share a word;
//   4. per tap: nine LDS words of code (rows of 8 words are skewed by one word, so the lanes' reads, 8 words apart, fall
//      in different banks), shifted by 16 bits where the tap's first entry is odd, and 8 + 8 v_dot2_i32_i16: two
//      samples' w * c per instruction;
//   5. the threads of a block add up, tap by tap as the sums are made (eighteen sums kept to the end cost a wave per
//      SIMD in registers): a DPP reduction over the largest power of two G <= 64 that divides the B / 16
//      threads of a block, one LDS word per group and field, and behind a barrier one thread per record adds the
//      B / (16 G) group sums (2 for B = 2048, 4 for 4096) and stores the record: plain 4-byte stores, one workgroup per
//      record, no atomics, no workspace.
// Two barriers per channel: the code entries and the group sums are each written behind the barrier that follows their
// last read.
//
// Widths.  |I - 128|, |Q - 128| <= 128 and |C[i]| + |S[i]| <= 46: |w| <= 5888.  A thread's sum holds 16 terms (94 208), a
// record at most 4096: 24 117 248 < 2^31, the header's bound; every partial sum is bounded by the same figure.  The
// channel fields, the code phase and its widths: replica.h.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it
// but k_subtract.hip, which takes g.n_blocks from gj_corr_blocks.
#include "replica.h"

namespace gj {

constexpr int kCorrGuard = GJ_CORR_MAX_TAP_OFFSET;                   // code entries in front of the tile
constexpr int kCorrWordsPerThread = 9;                               // 18 code entries
constexpr int kCorrCodeWords = kReplicaThreads * kCorrWordsPerThread;  // 2304 words of two entries
constexpr int kCorrCodeLds = kCorrCodeWords + kCorrCodeWords / 8;    // rows of 8 words skewed by one word each
constexpr int kCorrFieldsMax = 2 * GJ_CORR_MAX_TAPS;

static_assert(GJ_CORR_MAX_BLOCK == kReplicaTile, "one full block per tile at the most");
// the last entry a tap reads: sample 4095 under offset +64, plus the odd shift's extra word
static_assert((kReplicaTile - 1 + 2 * kCorrGuard) / 2 + 1 < kCorrCodeWords, "every tap's reads stay inside the entries made");
static_assert(4096ll * 128 * 46 < (1ll << 31), "a record fits int32");
static_assert(64ull * GJ_CORR_MAX_CODE_STEP < kReplicaPeriod, "the guard's phase is less than one code period");

struct CorrGeom {
    unsigned long long n_samples, n_blocks, n_tiles;
    int block_samples;           // B
    int tile_blocks;             // k = 4096 / B
    int block_threads;           // B / 16
    int group;                   // G: largest power of two <= 64 that divides block_threads
    int n_code_rows, n_channels, n_taps;
    int tap[GJ_CORR_MAX_TAPS];
};

// bytes (I, Q) in the low half of `pair` -> I - 128 in bits 0..15, Q - 128 in bits 16..31
__device__ __forceinline__ unsigned corr_unpack(unsigned pair) {
    const int i = (int)(pair & 0xffu) - 128, q = (int)((pair >> 8) & 0xffu) - 128;
    return ((unsigned)i & 0xffffu) | ((unsigned)q << 16);
}

__device__ __forceinline__ int corr_dot2(unsigned a, unsigned b, int acc) {
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc));
    return r;
}

__device__ __forceinline__ int corr_code_slot(int word) { return word + (word >> 3); }

// the sum of v over each aligned group of G lanes, G a power of two up to 64 that is the same for the whole launch
__device__ __forceinline__ int corr_group_sum(int v, int G) {
    switch (G) {
        case 64: return group_sum_dpp<64>(v);
        case 32: return group_sum_dpp<32>(v);
        case 16: return group_sum_dpp<16>(v);
        case 8: return group_sum_dpp<8>(v);
        case 4: return group_sum_dpp<4>(v);
        case 2: return group_sum_dpp<2>(v);
        default: return v;
    }
}

__global__ __launch_bounds__(kReplicaThreads) void corr_bank_kernel(const uint8_t* __restrict__ iq, CorrGeom g,
                                                                    const int16_t* __restrict__ codes,
                                                                    const gj_corr_channel* __restrict__ channels,
                                                                    int32_t* __restrict__ out) {
    __shared__ gj_corr_channel chan[GJ_CORR_MAX_CHANNELS];
    __shared__ unsigned code_bits[GJ_CORR_MAX_CHANNELS][32];         // bit c of word w: chip 32 w + c is -1
    __shared__ unsigned code_lds[kCorrCodeLds];                      // two +-1 int16 entries per word, rows skewed
    __shared__ int sums[kReplicaThreads * kCorrFieldsMax];           // [group of threads][field]
    __shared__ uint2 mix[16];                                        // (C, -S), (S, C) as int16 pairs

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fields = 2 * g.n_taps;

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
        mix[tid] = uint2{((unsigned)c & 0xffffu) | ((unsigned)(-s) << 16), ((unsigned)s & 0xffffu) | ((unsigned)c << 16)};
    }
    if (__syncthreads_or(bad)) return;
    replica_pack_codes(codes, chan, code_bits, g.n_channels, wave, lane);
    __syncthreads();

    const int tile_samples = g.tile_blocks * g.block_samples;
    const int code_words = (tile_samples + 2 * kCorrGuard) / 2 + 2;  // entries 0 .. tile + 128 and the odd shift's word
    const long long n = (long long)g.n_samples;

    for (unsigned long long tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const unsigned long long t_tile = tile * (unsigned long long)tile_samples;
        const long long t0 = (long long)t_tile + kReplicaRun * tid; // this thread's first sample

        // ---- 1. the thread's samples
        unsigned x[kReplicaRun];
#pragma unroll
        for (int s = 0; s < kReplicaRun; ++s) x[s] = 0u;
        if (kReplicaRun * tid < tile_samples) {
            if (t0 + kReplicaRun <= n) {
                unsigned raw[kReplicaRun / 2];
                replica_load_run(iq + 2 * t0, raw);
#pragma unroll
                for (int s = 0; s < kReplicaRun; ++s) x[s] = corr_unpack(raw[s >> 1] >> (16 * (s & 1)));
            } else {
#pragma unroll
                for (int s = 0; s < kReplicaRun; ++s)
                    if (t0 + s < n) x[s] = corr_unpack((unsigned)*reinterpret_cast<const uint16_t*>(iq + 2 * (t0 + s)));
            }
        }

        for (int ch = 0; ch < g.n_channels; ++ch) {
            const gj_corr_channel c = chan[ch];

            // ---- 2. the resampled code: entry e is sample t_tile - 64 + e
            {
                // phase of entry 0: one period is added so that the guard's 64 steps can be taken off
                const unsigned long long at_tile = replica_mod_period(c.code_phase + t_tile * c.code_step);
                const unsigned long long entry0 = replica_mod_period(at_tile + kReplicaPeriod - (unsigned long long)kCorrGuard * c.code_step);
                const int w0 = kCorrWordsPerThread * tid;
                unsigned long long ph = replica_mod_period(entry0 + (unsigned long long)(2 * w0) * c.code_step);
#pragma unroll
                for (int k = 0; k < kCorrWordsPerThread; ++k) {
                    unsigned word = 0;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        word |= (replica_chip_neg(code_bits[ch], ph) ? 0xffffu : 1u) << (16 * h);
                        ph = replica_step(ph, c.code_step);
                    }
                    if (w0 + k < code_words) code_lds[corr_code_slot(w0 + k)] = word;
                }
            }
            __syncthreads();

            // ---- 3. the carrier
            unsigned wi[kReplicaRun / 2], wq[kReplicaRun / 2];
            {
                unsigned theta = c.carr_phase + (unsigned)t0 * c.carr_step;
#pragma unroll
                for (int p = 0; p < kReplicaRun / 2; ++p) {
                    int i2[2], q2[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint2 m = mix[theta >> 28];
                        i2[h] = corr_dot2(x[2 * p + h], m.x, 0);
                        q2[h] = corr_dot2(x[2 * p + h], m.y, 0);
                        theta += c.carr_step;
                    }
                    wi[p] = ((unsigned)i2[0] & 0xffffu) | ((unsigned)i2[1] << 16);
                    wq[p] = ((unsigned)q2[0] & 0xffffu) | ((unsigned)q2[1] << 16);
                }
            }

            // ---- 4. the taps, and 5. the block's threads add up: one LDS word per group of G threads and field
            const bool leader = (tid & (g.group - 1)) == 0;
            const int slot = (tid / g.group) * fields;
#pragma unroll
            for (int j = 0; j < GJ_CORR_MAX_TAPS; ++j) {
                if (j < g.n_taps) {
                    const int e0 = kReplicaRun * tid + kCorrGuard + g.tap[j];     // >= 0: |tap| <= 64
                    const int wb = e0 >> 1;
                    unsigned cw[kReplicaRun / 2 + 1];
#pragma unroll
                    for (int k = 0; k <= kReplicaRun / 2; ++k) cw[k] = code_lds[corr_code_slot(wb + k)];
                    if (e0 & 1) {
#pragma unroll
                        for (int k = 0; k < kReplicaRun / 2; ++k) cw[k] = (cw[k] >> 16) | (cw[k + 1] << 16);
                    }
                    int si = 0, sq = 0;
#pragma unroll
                    for (int p = 0; p < kReplicaRun / 2; ++p) {
                        si = corr_dot2(wi[p], cw[p], si);
                        sq = corr_dot2(wq[p], cw[p], sq);
                    }
                    si = corr_group_sum(si, g.group);
                    sq = corr_group_sum(sq, g.group);
                    if (leader) sums[slot + 2 * j] = si, sums[slot + 2 * j + 1] = sq;
                }
            }
            __syncthreads();
            const int groups_per_block = g.block_threads / g.group;
            for (int r = tid; r < g.tile_blocks * fields; r += kReplicaThreads) {
                const int b = r / fields, f = r - b * fields;
                const unsigned long long block = tile * (unsigned long long)g.tile_blocks + (unsigned)b;
                if (block < g.n_blocks) {
                    int v = 0;
                    for (int k = 0; k < groups_per_block; ++k) v += sums[(b * groups_per_block + k) * fields + f];
                    out[((unsigned long long)ch * g.n_blocks + block) * (unsigned)fields + (unsigned)f] = v;
                }
            }
            // the next channel's code entries are written behind this channel's last read of them (the barrier above),
            // and its group sums behind the barrier that follows its entries, which these reads of sums precede
        }
    }
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_corr_blocks(size_t n_samples, int block_samples) {
    if (block_samples < 1) return 0;
    return n_samples / (size_t)block_samples + (n_samples % (size_t)block_samples != 0);
}

int gj_corr_bank_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int block_samples,
                     const int16_t* d_codes, int n_code_rows, const gj_corr_channel* d_channels, int n_channels,
                     const int32_t* tap_offsets, int n_taps, int32_t* d_out) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (!d_iq || !d_codes || !d_channels || !tap_offsets || !d_out) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if (int rc = replica_check_alignment(ctx, d_iq, d_codes, d_channels)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(ctx, GJ_ERR_INVALID, "records must be 4-byte aligned");
    if (n_code_rows < 1) return fail(ctx, GJ_ERR_INVALID, "n_code_rows %d", n_code_rows);
    if (int rc = replica_check_block(ctx, block_samples)) return rc;
    if (n_taps < 1 || n_taps > GJ_CORR_MAX_TAPS) return fail(ctx, GJ_ERR_UNSUPPORTED, "n_taps %d (1 .. %d)", n_taps, GJ_CORR_MAX_TAPS);
    for (int j = 0; j < n_taps; ++j)
        if (tap_offsets[j] < -GJ_CORR_MAX_TAP_OFFSET || tap_offsets[j] > GJ_CORR_MAX_TAP_OFFSET)
            return fail(ctx, GJ_ERR_UNSUPPORTED, "tap offset %d (|d| <= %d)", (int)tap_offsets[j], GJ_CORR_MAX_TAP_OFFSET);
    if (int rc = replica_check_counts(ctx, n_channels, n_samples)) return rc;
    if (first_sample > nbytes / 2 || n_samples > nbytes / 2 - first_sample)
        return fail(ctx, GJ_ERR_INVALID, "samples %zu .. +%zu run past the capture's %zu", first_sample, n_samples, nbytes / 2);
    CorrGeom g;
    g.n_samples = n_samples;
    g.block_samples = block_samples;
    g.tile_blocks = kReplicaTile / block_samples;
    g.block_threads = block_samples / kReplicaRun;
    g.group = 1;
    while (g.group < 64 && g.block_threads % (2 * g.group) == 0) g.group *= 2;
    g.n_blocks = gj_corr_blocks(n_samples, block_samples);
    g.n_tiles = (g.n_blocks + (unsigned)g.tile_blocks - 1) / (unsigned)g.tile_blocks;
    g.n_code_rows = n_code_rows;
    g.n_channels = n_channels;
    g.n_taps = n_taps;
    for (int j = 0; j < GJ_CORR_MAX_TAPS; ++j) g.tap[j] = j < n_taps ? tap_offsets[j] : 0;
    const unsigned grid = replica_grid(ctx, 3, g.n_tiles);   // the kernel's registers allow three waves per SIMD
    hipLaunchKernelGGL(corr_bank_kernel, dim3(grid), dim3(kReplicaThreads), 0, ctx->stream, d_iq + 2 * first_sample, g, d_codes,
                       d_channels, d_out);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
