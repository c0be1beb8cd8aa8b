// The de-chirp factors c_q[n] = exp(-i pi ((q n^2) mod 2 N^2) / N^2) of a thread's sixteen points n = jl + TF s, from
// exactly reduced integer phases and factored as k_chirp.hip factors them (its head has the argument):
//   q n^2 = q jl^2 + s (2 q jl TF) + s^2 (q TF^2)   (mod 2^32, of which 2 N^2 is a divisor)
//   c_q[jl + TF s] = (e8 d^(s - 8)) * k_s,   e8, d the thread's own, k_s a function of (q, s) alone.
// k_chirp.hip has ONE q per wave at a time and hands k_s round with v_readlane.  Here q belongs to a transform group,
// which may be a fraction of a wave (N <= 512), so k_s goes round the group's own lanes: the L = min(TF, 16) lanes that
// share a q evaluate 16 / L slots each and every lane fetches slot s from lane s mod L of its aligned set of L (a
// ds_bpermute; no LDS memory, no barrier).  A thread costs 2 + 16 / L sincospif: three from 256 points on.
// At q = 0 (and any multiple of 2 N^2) every phase is 0, every factor exactly (1, +0) and every product of them too.
//
// k_chirp.hip and k_excise_chirp.hip include this.  chirp_turn, the exact phase, serves both; chirp_factors is the
// excisor's, and k_chirp.hip keeps its wave-uniform hand-round of k_s and multiplies the data between the two parts
// (profiles/NOTES_excise_chirp.md).
#pragma once
#include "gj_common.h"

namespace gj {

// (cos, sin) of pi m / N^2 for a phase given modulo 2^32: the signed field of 2 log2(N) + 1 bits is m or m - 2 N^2,
// exact in a float, and m / N^2 an exact binary fraction.
template <int N>
__device__ __forceinline__ void chirp_turn(unsigned ph, float& cs, float& sn) {
    constexpr int PHASE_BITS = 2 * __builtin_ctz((unsigned)N) + 1;
    constexpr float INV_N2 = 1.0f / ((float)N * (float)N);
    const int m = (int)(ph << (32 - PHASE_BITS)) >> (32 - PHASE_BITS);
    sincospif((float)m * INV_N2, &sn, &cs);
}

// c[s] = c_q[jl + TF s], s = 0 .. 15.  `q` must be the same in every lane of the transform group (jl = 0 .. TF - 1, the
// group an aligned set of TF lanes, or whole waves); every lane of the wave must be active.
template <int N>
__device__ __forceinline__ void chirp_factors(c2 (&c)[16], unsigned q, int jl) {
    constexpr int TF = N / 16;
    constexpr int L = TF < 16 ? TF : 16;   // lanes that share the evaluation of k_s
    constexpr int K = 16 / L;              // slots each of them evaluates
    const unsigned uj = (unsigned)jl;
    const unsigned pj = q * (uj * uj), pd = q * (2u * uj * (unsigned)TF), pc = q * (unsigned)(TF * TF);
    float lcs[K], lsn[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const unsigned sl = (uj & (unsigned)(L - 1)) + (unsigned)(L * i);
        chirp_turn<N>(pc * (sl * sl), lcs[i], lsn[i]);
        lsn[i] = 0.f - lsn[i];   // the imaginary part; 0 - (+0) keeps rate 0 at (1, +0)
    }
    c2 k[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        if constexpr (L == 1) k[s] = make_c2(lcs[s], lsn[s]);
        else k[s] = make_c2(__shfl(lcs[s / L], s % L, L), __shfl(lsn[s / L], s % L, L));
    }
    if constexpr (TF == 1) {   // one thread per frame: jl = 0, n = s
#pragma unroll
        for (int s = 0; s < 16; ++s) c[s] = k[s];
    } else {
        float ecs, esn, dcs, dsn;
        chirp_turn<N>(pj + 8u * pd, ecs, esn);
        chirp_turn<N>(pd, dcs, dsn);
        const c2 e8 = make_c2(ecs, 0.f - esn), up = make_c2(dcs, 0.f - dsn), down = make_c2(dcs, dsn);
        c2 e = e8;
#pragma unroll
        for (int s = 8; s < 16; ++s) {
            c[s] = cmul(e, k[s]);
            e = cmul(e, up);
        }
        e = e8;
#pragma unroll
        for (int s = 7; s >= 0; --s) {
            e = cmul(e, down);
            c[s] = cmul(e, k[s]);
        }
    }
}

}   // namespace gj
