// Closed-loop tracking (gfx950): gj_track_dev of include/gpsjam.h, which states the definition.  Every channel runs its
// own DLL / FLL / PLL over n_epochs epochs of B samples in one launch: integer arithmetic from the byte to the loop
// state, so every record and every state is the definition's whatever the layout.
//
// One workgroup of four waves per channel; the loop is sequential per channel and the channels are independent.  Thread
// tid owns the 16 consecutive samples 16 tid .. 16 tid + 15 of the epoch (replica.h): B / 16 threads carry data, the
// others contribute zeros.  A channel's epochs never reach past n_samples (the channel check), so no run is ragged.
//   0. once: the state is read by every thread and checked (a bad channel returns before it reads a chip or writes
//      anything), the channel's one code row is packed to sign bits and the carrier table put into LDS;
//   1. per epoch, first the loads of the NEXT epoch's 32 bytes: their address is first_sample + start + (m + 1) B
//      whatever the loop does, so they are in flight while this epoch's chips, mixer and taps are made.  hipcc waits
//      for them where it copies them into the registers the next iteration reads, at the end of step 3 and in front
//      of the barrier, not behind the update (profiles/NOTES_track.md);
//   2. the chips as sign bits in a register.  spacing <= 8: ONE window t - d .. t + 15 + d, the first phase by one
//      64-bit multiply and a mod, the others by exact steps; the three taps are three 16-bit fields of it.  Wider
//      spacings: three windows of 16 with a first phase each (48 steps instead of up to 144);
//   3. the carrier as in k_corr.hip: theta in uint32, the table entry (C, -S), (S, C) as one 8-byte LDS read, wI and wQ
//      by one v_dot2_i32_i16 each; a tap's sum is sum(w) - 2 sum(w where the chip is -1);
//   4. six DPP wave sums (wave-uniform), 4 x 6 words to LDS, double-buffered on the epoch's parity: a wave writes
//      buffer m & 1 again only behind the barrier of epoch m + 1, which every wave reaches behind its reads of epoch m,
//      so ONE barrier per epoch suffices;
//   5. behind the barrier EVERY wave adds the four waves' sums and makes the discriminators, the filters and the update
//      redundantly: the state stays uniform in registers and needs no broadcast.  The three CORDICs are ONE instruction
//      stream, lanes 0, 1 and 2 turning P, E and L, and so are the epoch's two 64-bit divisions (lane 0 the code
//      discriminator, lane 1 the aiding's floor(carr_nco / aid_div), whose last value is kept along): left to itself
//      the compiler runs all of it on the scalar unit, three CORDICs and three divisions one after the other, behind
//      a branch per step (profiles/NOTES_track.md).  Thread 0 stores the record, and behind the last epoch the state.
//
// Widths.  The sums: k_corr.hip (|record| <= 24 117 248).  CORDIC: |x|, |y| < 2^25 2^8 1.65 sqrt 2 < 2^34 in int64.
// The filters: |e - e_prev| <= 2 sum A < 2^32, |e| < 2^31, |f| <= 2^30 and |gain| <= 2^30: the PLL sum is below
// 4.7e9 2^30 < 2^63 and |dn| < 2^31; |c| <= 2^16: |dc| < 2^24.  The code phase: replica.h (B code_step < 2^46).
//
// This is a translation unit of its own with its own extern "C" entry point: none of the other sources refers to it.
#include "replica.h"

namespace gj {

constexpr int kTrackNarrow = 8;                                      // spacings up to this use one chip window

static_assert(sizeof(gj_track_state) == 64 && sizeof(gj_track_params) == 32 && sizeof(gj_track_epoch) == 56, "the header's layout");
static_assert(16 + 2 * kTrackNarrow <= 32, "the narrow window fits one word");
static_assert((unsigned long long)GJ_CORR_MAX_TAP_OFFSET * GJ_CORR_MAX_CODE_STEP < kReplicaPeriod, "a tap's phase is less than one code period");
static_assert((unsigned long long)(GJ_CORR_MAX_BLOCK + GJ_CORR_MAX_TAP_OFFSET) * GJ_CORR_MAX_CODE_STEP + 2 * kReplicaPeriod < (1ull << 63),
              "a window's first phase is reduced by replica_mod_period");

struct TrackGeom {
    unsigned long long n_samples;
    int block_samples, n_epochs, n_code_rows;
    gj_track_params p;
};

// bytes (I, Q) in the low half of `pair` -> I - 128 in bits 0..15, Q - 128 in bits 16..31 (as k_corr.hip)
__device__ __forceinline__ unsigned track_unpack(unsigned pair) {
    const int i = (int)(pair & 0xffu) - 128, q = (int)((pair >> 8) & 0xffu) - 128;
    return ((unsigned)i & 0xffffu) | ((unsigned)q << 16);
}

__device__ __forceinline__ int track_dot2(unsigned a, unsigned b) {
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// sign bits of `count` consecutive chips from the reduced phase ph: bit i says that the chip of step i is -1
__device__ __forceinline__ unsigned track_chips(const unsigned* bits, unsigned long long ph, unsigned long long code_step, int count) {
    unsigned m = 0;
    for (int i = 0; i < count; ++i) {
        m |= replica_chip_neg(bits, ph) << i;
        ph = replica_step(ph, code_step);
    }
    return m;
}

// the phase of local sample s >= -GJ_CORR_MAX_TAP_OFFSET: one period is added so that a tap's steps can be taken off
__device__ __forceinline__ unsigned long long track_phase(const gj_corr_channel& c, int s) {
    return replica_mod_period(c.code_phase + kReplicaPeriod + (unsigned long long)(long long)s * c.code_step);
}

// (I, Q) -> angle in 2^-32 cycles and length, the header's CORDIC
__device__ __forceinline__ void track_cordic(int vi, int vq, int& angle, long long& length) {
    constexpr int kAtan[16] = GJ_TRACK_ATAN_TABLE;
    long long x = (long long)vi * 256, y = (long long)vq * 256;
    int z = 0;
    if (x < 0) x = -x, y = -y;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const long long xs = x >> k, ys = y >> k;
        if (y >= 0) x += ys, y -= xs, z += kAtan[k];
        else x -= ys, y += xs, z -= kAtan[k];
    }
    angle = (vi | vq) ? z : 0, length = x;                          // (0, 0): the steps alone would turn by the whole table
}

__device__ __forceinline__ long long track_readlane64(long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// floor(a / b) for b > 0
__device__ __forceinline__ long long track_floor_div(long long a, long long b) {
    long long q = a / b;
    if (a % b < 0) --q;
    return q;
}

__global__ __launch_bounds__(kReplicaThreads) void track_kernel(const uint8_t* __restrict__ iq, TrackGeom g,
                                                                const int16_t* __restrict__ codes, gj_track_state* states,
                                                                gj_track_epoch* __restrict__ out) {
    __shared__ gj_corr_channel chan[1];
    __shared__ unsigned code_bits[1][32];                            // bit c of word w: chip 32 w + c is -1
    __shared__ int sums[2][kReplicaThreads / 64][6];                 // [epoch parity][wave][E, P, L x I, Q]
    __shared__ uint2 mix[16];                                        // (C, -S), (S, C) as int16 pairs

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = g.block_samples, d = g.p.spacing;

    // ---- 0. the state: every thread reads and checks it; nothing is written before this
    gj_track_state S = states[blockIdx.x];
    if (GJ_REPLICA_CHANNEL_BAD(S.ch, g.n_code_rows) || S.reserved[0] != 0 || S.reserved[1] != 0 || (S.primed != 0 && S.primed != 1) ||
        (unsigned long long)S.start + (unsigned long long)g.n_epochs * (unsigned)B > g.n_samples)
        return;
    if (tid == 0) chan[0] = S.ch;
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
    __syncthreads();
    replica_pack_codes(codes, chan, code_bits, 1, wave, lane);
    __syncthreads();

    const bool active = kReplicaRun * tid < B;                       // this thread carries samples
    const int t0 = kReplicaRun * tid;
    const uint8_t* src = iq + 2 * ((size_t)S.start + (size_t)t0);    // this thread's run of epoch 0
    gj_track_epoch* rec = out + (size_t)blockIdx.x * (size_t)g.n_epochs;

    unsigned next[kReplicaRun / 2];
#pragma unroll
    for (int k = 0; k < kReplicaRun / 2; ++k) next[k] = 0u;
    if (active) replica_load_run(src, next);

    long long nco_div_prev = g.p.aid_div ? track_floor_div(S.carr_nco, g.p.aid_div) : 0;   // floor(carr_nco / aid_div), kept along

    for (int m = 0; m < g.n_epochs; ++m) {
        // ---- 1. this epoch's bytes, and the next epoch's loads
        unsigned raw[kReplicaRun / 2];
#pragma unroll
        for (int k = 0; k < kReplicaRun / 2; ++k) raw[k] = next[k];
        if (active && m + 1 < g.n_epochs) replica_load_run(src + 2 * (size_t)(m + 1) * (size_t)B, next);

        int s6[6] = {0, 0, 0, 0, 0, 0};
        if (active) {
            // ---- 2. the chips of the three taps
            unsigned early, prompt, late;
            if (d <= kTrackNarrow) {
                const unsigned w = track_chips(code_bits[0], track_phase(S.ch, t0 - d), S.ch.code_step, kReplicaRun + 2 * d);
                late = w & 0xffffu, prompt = (w >> d) & 0xffffu, early = (w >> (2 * d)) & 0xffffu;
            } else {
                early = track_chips(code_bits[0], track_phase(S.ch, t0 + d), S.ch.code_step, kReplicaRun);
                prompt = track_chips(code_bits[0], track_phase(S.ch, t0), S.ch.code_step, kReplicaRun);
                late = track_chips(code_bits[0], track_phase(S.ch, t0 - d), S.ch.code_step, kReplicaRun);
            }
            // ---- 3. the carrier and the taps: sum(w c) = sum(w) - 2 sum(w where c = -1)
            unsigned theta = S.ch.carr_phase + (unsigned)t0 * S.ch.carr_step;
            int ti = 0, tq = 0, n6[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < kReplicaRun; ++s) {
                const unsigned x = track_unpack(raw[s >> 1] >> (16 * (s & 1)));
                const uint2 mx = mix[theta >> 28];
                const int wi = track_dot2(x, mx.x), wq = track_dot2(x, mx.y);
                theta += S.ch.carr_step;
                ti += wi, tq += wq;
                const int me = -(int)((early >> s) & 1u), mp = -(int)((prompt >> s) & 1u), ml = -(int)((late >> s) & 1u);
                n6[0] += wi & me, n6[1] += wq & me;
                n6[2] += wi & mp, n6[3] += wq & mp;
                n6[4] += wi & ml, n6[5] += wq & ml;
            }
#pragma unroll
            for (int f = 0; f < 6; ++f) s6[f] = ((f & 1) ? tq : ti) - 2 * n6[f];
        }

        // ---- 4. the waves' sums
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            const int v = group_sum_dpp<64>(s6[f]);
            if (lane == 0) sums[m & 1][wave][f] = v;
        }
        __syncthreads();

        // ---- 5. every thread: the epoch's three sums, the discriminators, the filters and the update
        int r6[6];
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            int v = 0;
#pragma unroll
            for (int w = 0; w < kReplicaThreads / 64; ++w) v += sums[m & 1][w][f];
            r6[f] = v;
        }
        // lanes 0, 1 and 2 of every wave turn P, E and L in ONE instruction stream; the others repeat P
        const int which = lane < 3 ? lane : 0;
        int angle;
        long long length;
        track_cordic(which == 1 ? r6[0] : which == 2 ? r6[4] : r6[2], which == 1 ? r6[1] : which == 2 ? r6[5] : r6[3], angle, length);
        const int e = __builtin_amdgcn_readlane(angle, 0);
        const long long mE = track_readlane64(length, 1), mL = track_readlane64(length, 2);
        if (S.primed == 0) S.e_prev = e;
        const long long de = (long long)e - S.e_prev;
        long long f = de;
        if (f > (1ll << 30)) f = (1ll << 31) - f;
        else if (f < -(1ll << 30)) f = -(1ll << 31) - f;
        const long long dn = (g.p.pll_p * de + (long long)g.p.pll_i * e + g.p.fll * f) >> GJ_TRACK_PLL_SHIFT;
        const long long nco = (long long)((unsigned long long)S.carr_nco - (unsigned long long)dn);
        // the two divisions of an epoch likewise: lane 1 the aiding's floor(nco' / aid_div), the others the code discriminator
        const long long den = mE + mL;
        const long long quot = track_floor_div(lane == 1 ? nco : (mE - mL) * 65536, lane == 1 ? (g.p.aid_div ? g.p.aid_div : 1) : (den ? den : 1));
        const int c = den ? __builtin_amdgcn_readlane((int)quot, 0) : 0;
        const long long nco_div = track_readlane64(quot, 1);
        if (S.primed == 0) S.c_prev = c, S.primed = 1;
        const long long dc = (g.p.dll_p * ((long long)c - S.c_prev) + (long long)g.p.dll_i * c) >> GJ_TRACK_DLL_SHIFT;

        if (tid == 0) {
            gj_track_epoch r;
            r.early[0] = r6[0], r.early[1] = r6[1], r.prompt[0] = r6[2], r.prompt[1] = r6[3], r.late[0] = r6[4], r.late[1] = r6[5];
            r.carr_phase = S.ch.carr_phase, r.carr_step = S.ch.carr_step;
            r.code_phase = S.ch.code_phase, r.code_step = S.ch.code_step;
            r.e = e, r.c = c;
            rec[m] = r;
        }

        // advance with the old steps, then steer
        S.ch.code_phase = replica_mod_period(S.ch.code_phase + (unsigned long long)B * S.ch.code_step);
        S.ch.carr_phase += (unsigned)B * S.ch.carr_step;
        const long long aid = g.p.aid_div ? nco_div - nco_div_prev : 0;
        nco_div_prev = nco_div;
        S.ch.carr_step -= (unsigned)dn;
        long long step = (long long)S.ch.code_step + dc + aid;
        step = step < 0 ? 0 : step > (long long)(GJ_CORR_MAX_CODE_STEP - 1) ? (long long)(GJ_CORR_MAX_CODE_STEP - 1) : step;
        S.ch.code_step = (unsigned long long)step;
        S.carr_nco = nco, S.e_prev = e, S.c_prev = c;
    }

    if (tid == 0) {
        S.start += (unsigned)g.n_epochs * (unsigned)B;
        states[blockIdx.x] = S;
    }
}

}   // namespace gj

using namespace gj;

extern "C" {

int gj_track_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int block_samples,
                 int n_epochs, const int16_t* d_codes, int n_code_rows, gj_track_state* d_states, int n_channels,
                 gj_track_params params, gj_track_epoch* d_out) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (!d_iq || !d_codes || !d_states || !d_out) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if ((reinterpret_cast<uintptr_t>(d_iq) | reinterpret_cast<uintptr_t>(d_codes)) & 1)
        return fail(ctx, GJ_ERR_INVALID, "the capture and the codes must be 2-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_states) | reinterpret_cast<uintptr_t>(d_out)) & 7)
        return fail(ctx, GJ_ERR_INVALID, "states and records must be 8-byte aligned");
    if (n_code_rows < 1) return fail(ctx, GJ_ERR_INVALID, "n_code_rows %d", n_code_rows);
    if (params.reserved != 0) return fail(ctx, GJ_ERR_INVALID, "params.reserved must be 0");
    if (int rc = replica_check_block(ctx, block_samples)) return rc;
    if (n_epochs < 1 || n_epochs > GJ_TRACK_MAX_EPOCHS)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "n_epochs %d (1 .. %d)", n_epochs, GJ_TRACK_MAX_EPOCHS);
    if (n_channels < 1 || n_channels > GJ_TRACK_MAX_CHANNELS)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "n_channels %d (1 .. %d)", n_channels, GJ_TRACK_MAX_CHANNELS);
    if (n_samples < 1 || n_samples > GJ_CORR_MAX_SAMPLES)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "n_samples %zu (1 .. %llu)", n_samples, (unsigned long long)GJ_CORR_MAX_SAMPLES);
    if (params.spacing < 1 || params.spacing > GJ_CORR_MAX_TAP_OFFSET)
        return fail(ctx, GJ_ERR_UNSUPPORTED, "spacing %d (1 .. %d)", (int)params.spacing, GJ_CORR_MAX_TAP_OFFSET);
    if (params.aid_div < 0) return fail(ctx, GJ_ERR_UNSUPPORTED, "aid_div %d (>= 0)", (int)params.aid_div);
    for (int32_t gain : {params.pll_p, params.pll_i, params.fll, params.dll_p, params.dll_i})
        if (gain < -GJ_TRACK_MAX_GAIN || gain > GJ_TRACK_MAX_GAIN)
            return fail(ctx, GJ_ERR_UNSUPPORTED, "gain %d (|g| <= %d)", (int)gain, GJ_TRACK_MAX_GAIN);
    if ((unsigned long long)n_epochs * (unsigned)block_samples > n_samples)
        return fail(ctx, GJ_ERR_INVALID, "%d epochs of %d samples take more than the range's %zu", n_epochs, block_samples, n_samples);
    if (first_sample > nbytes / 2 || n_samples > nbytes / 2 - first_sample)
        return fail(ctx, GJ_ERR_INVALID, "samples %zu .. +%zu run past the capture's %zu", first_sample, n_samples, nbytes / 2);
    TrackGeom g;
    g.n_samples = n_samples;
    g.block_samples = block_samples;
    g.n_epochs = n_epochs;
    g.n_code_rows = n_code_rows;
    g.p = params;
    hipLaunchKernelGGL(track_kernel, dim3((unsigned)n_channels), dim3(kReplicaThreads), 0, ctx->stream, d_iq + 2 * first_sample, g,
                       d_codes, d_states, d_out);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
