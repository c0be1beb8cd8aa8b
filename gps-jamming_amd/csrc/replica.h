// The replica layer under the correlator bank (k_corr.hip), the counterfeit-signal subtraction (k_subtract.hip), the
// tracking loops (k_track.hip) and the subtraction of tracked signals (k_subtract_track.hip): those four include this,
// nothing else does.  All walk the same local replica -- a code row resampled by a code NCO, times a 16-entry carrier
// table indexed by a carrier NCO -- the bank and the loops to multiply the capture with it, the subtractions to take it
// off.  What defines the replica stands here once; the
// kernels, their inner loops and their occupancy stay apart.
//
// A CHANNEL is a gj_corr_channel of include/gpsjam.h, good when reserved == 0, 0 <= code_row < n_code_rows,
// code_phase < 1023 * 2^32 (Q32.32 chips: less than one period) and code_step < GJ_CORR_MAX_CODE_STEP = 2^34.  An entry
// point cannot answer for device memory with a status, so every workgroup checks every channel itself
// (GJ_REPLICA_CHANNEL_BAD) and returns on a bad one before it reads a chip or writes anything.
//
// THE CODE PHASE of sample t is (code_phase + t code_step) mod 1023 * 2^32, its chip the upper word.  t < 2^28 and
// code_step < 2^34 give t code_step < 2^62; with code_phase < 2^42 the sum stays below 2^63.  Such an x is reduced as
// ((x >> 32) mod 1023) << 32 | low word (replica_mod_period): x >> 32 < 2^31, a 32-bit remainder by a constant.  From
// one sample to the next the phase is stepped exactly (replica_step): a reduced phase and a step are below two periods
// together, so one conditional subtraction reduces the sum.
//
// THE CARRIER of sample t is table entry (carr_phase + t carr_step) >> 28, in uint32, which wraps as the definition's
// mod 2^32: C = GJ_CORR_COS_TABLE, S[i] = C[(i - 4) & 15].
//
// Thread tid of kReplicaThreads owns the kReplicaRun consecutive samples from kReplicaRun * tid of its workgroup's tile;
// block sizes are multiples of the run, so they lie in ONE block.  Its 32 bytes come as two 16-byte loads that are
// 2-byte aligned, for first_sample may be odd.  Each kernel picks its own table entries and keeps its own inner loop.
#pragma once
#include "gj_common.h"

namespace gj {

constexpr int kReplicaThreads = 256;
constexpr int kReplicaRun = 16;                                      // samples of a thread
constexpr int kReplicaTile = kReplicaThreads * kReplicaRun;          // 4096
constexpr unsigned long long kReplicaPeriod = (unsigned long long)GJ_CORR_CODE_LEN << 32;

static_assert(sizeof(gj_corr_channel) == 32, "the header's layout");
static_assert(GJ_CORR_MAX_BLOCK % kReplicaRun == 0 && kReplicaTile % kReplicaRun == 0, "a thread's samples lie in one block");
static_assert(GJ_CORR_MAX_CODE_STEP < kReplicaPeriod, "a step passes the period once at the most");

// ---- device side ------------------------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(2))) ReplicaChunk16 {
    unsigned x, y, z, w;
};

// A thread's whole run at p: eight words of two samples (I, Q, I, Q) each.  A run at the ragged end is read two bytes at
// a time in each kernel: with that loop in a helper here both kernels came out in other instructions.
__device__ __forceinline__ void replica_load_run(const uint8_t* p, unsigned (&raw)[kReplicaRun / 2]) {
    const ReplicaChunk16 lo = *reinterpret_cast<const ReplicaChunk16*>(p);
    const ReplicaChunk16 hi = *reinterpret_cast<const ReplicaChunk16*>(p + 16);
    raw[0] = lo.x, raw[1] = lo.y, raw[2] = lo.z, raw[3] = lo.w, raw[4] = hi.x, raw[5] = hi.y, raw[6] = hi.z, raw[7] = hi.w;
}

// x mod 1023 * 2^32 for x < 2^63
__device__ __forceinline__ unsigned long long replica_mod_period(unsigned long long x) {
    return ((unsigned long long)((unsigned)(x >> 32) % (unsigned)GJ_CORR_CODE_LEN) << 32) | (x & 0xffffffffull);
}

// Any field of channel c outside its bounds.  A macro: as a function of any shape the chain of conditions is folded
// before it is inlined, and both kernels come out in other instructions (profiles/NOTES_replica.md).
#define GJ_REPLICA_CHANNEL_BAD(c, n_code_rows)                                                                       \
    ((c).reserved != 0 || (c).code_row < 0 || (c).code_row >= (n_code_rows) || (c).code_phase >= kReplicaPeriod || \
     (c).code_step >= GJ_CORR_MAX_CODE_STEP)

// The code row of every checked channel in `chan` packed to 1023 sign bits: bit c of code_bits[ch][w] says that chip
// 32 w + c is -1.  One ballot per 64 chips, the items dealt to the workgroup's waves: 8 KiB for 64 channels, whatever
// the number of rows.  The caller's barriers stand in front of it (chan) and behind it (code_bits).
__device__ __forceinline__ void replica_pack_codes(const int16_t* __restrict__ codes, const gj_corr_channel* chan,
                                                   unsigned (*code_bits)[32], int n_channels, int wave, int lane) {
    for (int item = wave; item < n_channels * 16; item += kReplicaThreads / 64) {
        const int ch = item >> 4, chip = (item & 15) * 64 + lane;
        const int v = chip < GJ_CORR_CODE_LEN ? (int)codes[(size_t)chan[ch].code_row * GJ_CORR_CODE_LEN + chip] : 0;
        const unsigned long long m = __ballot(v < 0);
        if (lane == 0) {
            code_bits[ch][2 * (item & 15)] = (unsigned)m;
            code_bits[ch][2 * (item & 15) + 1] = (unsigned)(m >> 32);
        }
    }
}

// 1 where the chip of the reduced phase ph is -1 in a channel's 32 sign words
__device__ __forceinline__ unsigned replica_chip_neg(const unsigned* bits, unsigned long long ph) {
    const unsigned chip = (unsigned)(ph >> 32);
    return (bits[chip >> 5] >> (chip & 31)) & 1u;
}

// the reduced phase of the next sample
__device__ __forceinline__ unsigned long long replica_step(unsigned long long ph, unsigned long long code_step) {
    ph += code_step;
    if (ph >= kReplicaPeriod) ph -= kReplicaPeriod;
    return ph;
}

// ---- host side --------------------------------------------------------------------------------------------------------
// The refusals both entry points make in the same words, in three pieces: each has checks of its own between them.
inline int replica_check_alignment(gj_ctx* ctx, const uint8_t* d_iq, const int16_t* d_codes, const gj_corr_channel* d_channels) {
    if ((reinterpret_cast<uintptr_t>(d_iq) | reinterpret_cast<uintptr_t>(d_codes)) & 1)
        return fail(ctx, GJ_ERR_INVALID, "the capture and the codes must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_channels) & 7) return fail(ctx, GJ_ERR_INVALID, "channels must be 8-byte aligned");
    return GJ_OK;
}
inline int replica_check_block(gj_ctx* ctx, int block_samples) {
    if (block_samples < 16 || block_samples > GJ_CORR_MAX_BLOCK || block_samples % 16)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "block_samples %d (a multiple of 16 in 16 .. %d)", block_samples, GJ_CORR_MAX_BLOCK);
    return GJ_OK;
}
inline int replica_check_counts(gj_ctx* ctx, int n_channels, size_t n_samples) {
    if (n_channels < 1 || n_channels > GJ_CORR_MAX_CHANNELS)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "n_channels %d (1 .. %d)", n_channels, GJ_CORR_MAX_CHANNELS);
    if (n_samples < 1 || n_samples > GJ_CORR_MAX_SAMPLES)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "n_samples %zu (1 .. %llu)", n_samples, (unsigned long long)GJ_CORR_MAX_SAMPLES);
    return GJ_OK;
}

// every workgroup resident at once, per_cu to a CU (what the kernel's registers allow), so that the code rows are packed
// once per slot and not once per tile
inline unsigned replica_grid(const gj_ctx* ctx, unsigned per_cu, unsigned long long n_tiles) {
    const unsigned long long slots = (unsigned long long)per_cu * (unsigned)(ctx->num_cus > 0 ? ctx->num_cus : 1);
    return (unsigned)(n_tiles < slots ? n_tiles : slots);
}

}   // namespace gj
