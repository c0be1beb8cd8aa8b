// K-peak search over the acquisition's power surfaces (gfx950): gj_acq_peaks_dev / gj_acq_peaks_workspace of
// include/gpsjam.h, which states the definition.  Comparisons only for the peaks, so every peak is the definition's
// whatever the tiling; the floor is a sum of doubles in a fixed order.
//
// A zone is a set of whole columns, so a column is all the picks need to know: its largest cell, the first row that
// holds it, and its sum.
//   1. peaks_columns_kernel, grid (PRN, tiles of 64 columns): a workgroup of four waves, wave w walks the rows w, w + 4,
//      ... of the tile; a lane owns one column, so a wave's load is 512 contiguous bytes and six of them are in flight
//      per lane.  The surface is read ONCE.  The four waves' (maximum, row, sum) meet in LDS: the larger value wins,
//      of equal values the smaller row -- the first row that attains the column's maximum.  One record per column goes
//      to the workspace: 20 bytes per column against 8 n_freq read.
//   2. peaks_pick_kernel, one workgroup per PRN: k passes over the PRN's column records (L2-resident: 40 KiB at 2048
//      columns).  A pass takes the columns no earlier peak excludes and reduces (value, flat index = row nsamp + column)
//      -- larger value, then smaller flat index: the first maximum in the surface's order -- over the lanes by
//      shuffles and over the waves through LDS.  A last pass adds the kept columns' sums.
// No atomics, no memset: every record of the workspace is written by launch 1 before launch 2 reads it.
//
// This is a translation unit of its own with its own extern "C" entry points: none of the other sources refers to it.
#include "gj_common.h"

namespace gj {

constexpr int kPeakCols = 64;                   // columns of a tile: one wave wide
constexpr int kPeakRowWaves = 4;                // waves of a workgroup, rows interleaved among them
constexpr int kPeakThreads = kPeakCols * kPeakRowWaves;
constexpr int kPeakUnroll = 6;                  // loads in flight per lane
constexpr int kPickThreads = 256;
constexpr int kPickWaves = kPickThreads / 64;
constexpr int kPickBatch = 8;                   // column records a thread loads at once: 2048 columns are one batch
constexpr int kPeakMinSamp = 8, kPeakMaxSamp = 65536, kPeakMaxFreq = 4096;
constexpr int kNoFlat = 0x7fffffff;

static_assert(sizeof(gj_acq_peak) == 16 && sizeof(gj_acq_floor) == 16, "the header's layout");
static_assert((long long)kPeakMaxFreq * kPeakMaxSamp < (long long)kNoFlat, "a flat index fits int32");

struct PeakWs {
    double* colmax;     // [n_prn][nsamp]
    double* colsum;     // [n_prn][nsamp]
    int* colrow;        // [n_prn][nsamp]
};

// (v, at) is better than (best, best_at): larger value, of equal values the smaller index
__device__ __forceinline__ bool peak_better(double v, int at, double best, int best_at) {
    return v > best || (v == best && at < best_at);
}

__global__ __launch_bounds__(kPeakThreads) void peaks_columns_kernel(const double* __restrict__ power, int n_freq, int nsamp,
                                                                     PeakWs ws) {
    __shared__ double s_max[kPeakRowWaves][kPeakCols], s_sum[kPeakRowWaves][kPeakCols];
    __shared__ int s_row[kPeakRowWaves][kPeakCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (int)blockIdx.y * kPeakCols + lane;
    const size_t prn = blockIdx.x;
    double m = -1.0, s = 0.0;                   // powers are >= 0: the first cell read replaces -1
    int r = 0;
    if (col < nsamp) {
        const double* p = power + prn * (size_t)n_freq * (size_t)nsamp + (size_t)col;
        int f = wave;
        for (; f + (kPeakUnroll - 1) * kPeakRowWaves < n_freq; f += kPeakUnroll * kPeakRowWaves) {
            double v[kPeakUnroll];
#pragma unroll
            for (int u = 0; u < kPeakUnroll; ++u) v[u] = p[(size_t)(f + u * kPeakRowWaves) * (size_t)nsamp];
#pragma unroll
            for (int u = 0; u < kPeakUnroll; ++u) {
                s += v[u];
                if (v[u] > m) m = v[u], r = f + u * kPeakRowWaves;   // rows ascend: the first that attains the maximum
            }
        }
        for (; f < n_freq; f += kPeakRowWaves) {
            const double v = p[(size_t)f * (size_t)nsamp];
            s += v;
            if (v > m) m = v, r = f;
        }
    }
    s_max[wave][lane] = m, s_sum[wave][lane] = s, s_row[wave][lane] = r;
    __syncthreads();
    if (wave == 0 && col < nsamp) {
#pragma unroll
        for (int w = 1; w < kPeakRowWaves; ++w) {
            const double mw = s_max[w][lane];
            const int rw = s_row[w][lane];
            if (peak_better(mw, rw, m, r)) m = mw, r = rw;
            s += s_sum[w][lane];
        }
        const size_t at = prn * (size_t)nsamp + (size_t)col;
        ws.colmax[at] = m, ws.colsum[at] = s, ws.colrow[at] = r;
    }
}

__global__ __launch_bounds__(kPickThreads) void peaks_pick_kernel(PeakWs ws, int n_freq, int nsamp, int k, int guard,
                                                                  gj_acq_peak* __restrict__ peaks, gj_acq_floor* __restrict__ floor) {
    __shared__ double w_val[kPickWaves];
    __shared__ int w_at[kPickWaves];
    __shared__ int s_code[GJ_ACQ_MAX_PEAKS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t prn = blockIdx.x;
    const double* colmax = ws.colmax + prn * (size_t)nsamp;
    const double* colsum = ws.colsum + prn * (size_t)nsamp;
    const int* colrow = ws.colrow + prn * (size_t)nsamp;

    // column i lies in the zone of one of the first `taken` peaks
    auto excluded = [&](int i, int taken) {
        bool out = false;
        for (int q = 0; q < taken; ++q) {
            int d = i - s_code[q];
            d = d < 0 ? -d : d;
            d = d < nsamp - d ? d : nsamp - d;
            out = out || d <= guard;
        }
        return out;
    };

    for (int j = 0; j < k; ++j) {
        double best = -2.0;                     // below every record, also one of a column that held no number
        int best_at = kNoFlat;
        for (int i0 = tid; i0 < nsamp; i0 += kPickBatch * kPickThreads) {
            // the batch's records first, zone or not: the loads go out together instead of one behind each zone test
            double v[kPickBatch];
            int row[kPickBatch];
#pragma unroll
            for (int u = 0; u < kPickBatch; ++u) {
                const int i = i0 + u * kPickThreads;
                v[u] = i < nsamp ? colmax[i] : -2.0;
                row[u] = i < nsamp ? colrow[i] : 0;
            }
#pragma unroll
            for (int u = 0; u < kPickBatch; ++u) {
                const int i = i0 + u * kPickThreads;
                const int at = row[u] * nsamp + i;
                if (i < nsamp && !excluded(i, j) && peak_better(v[u], at, best, best_at)) best = v[u], best_at = at;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off, 64);
            const int oat = __shfl_xor(best_at, off, 64);
            if (peak_better(ov, oat, best, best_at)) best = ov, best_at = oat;
        }
        if (lane == 0) w_val[wave] = best, w_at[wave] = best_at;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kPickWaves; ++w)
                if (peak_better(w_val[w], w_at[w], best, best_at)) best = w_val[w], best_at = w_at[w];
            // k (2 guard + 1) < nsamp leaves a column to every pick; one that held no number at all gives index -1
            const int code = best_at == kNoFlat ? -1 : best_at % nsamp, freq = best_at == kNoFlat ? -1 : best_at / nsamp;
            s_code[j] = code;
            gj_acq_peak rec;
            rec.power = best, rec.code_index = code, rec.freq_index = freq;
            peaks[prn * (size_t)k + (size_t)j] = rec;
        }
        __syncthreads();                        // s_code[j] for the next pass; w_val / w_at are free again
    }

    double sum = 0.0;
    int kept = 0;
    for (int i0 = tid; i0 < nsamp; i0 += kPickBatch * kPickThreads) {
        double v[kPickBatch];
#pragma unroll
        for (int u = 0; u < kPickBatch; ++u) {
            const int i = i0 + u * kPickThreads;
            v[u] = i < nsamp ? colsum[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kPickBatch; ++u) {
            const int i = i0 + u * kPickThreads;
            if (i < nsamp && !excluded(i, k)) sum += v[u], ++kept;
        }
    }
    sum = wave_sum_f64(sum);
    kept = (int)wave_sum_u32((unsigned)kept);
    if (lane == 0) w_val[wave] = sum, w_at[wave] = kept;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kPickWaves; ++w) sum += w_val[w], kept += w_at[w];
        gj_acq_floor rec;
        rec.mean_power = sum / ((double)n_freq * (double)kept);
        rec.kept_columns = kept, rec.reserved = 0;
        floor[prn] = rec;
    }
}

static bool peaks_shape_ok(int nsamp, int n_prn) { return nsamp >= kPeakMinSamp && nsamp <= kPeakMaxSamp && n_prn >= 1; }

static size_t peaks_workspace(int nsamp, int n_prn) {
    const size_t cols = (size_t)n_prn * (size_t)nsamp;
    return 2 * align_up(cols * sizeof(double), 256) + align_up(cols * sizeof(int), 256);
}

}   // namespace gj

using namespace gj;

extern "C" {

size_t gj_acq_peaks_workspace(gj_ctx*, int nsamp, int n_prn) { return peaks_shape_ok(nsamp, n_prn) ? peaks_workspace(nsamp, n_prn) : 0; }

int gj_acq_peaks_dev(gj_ctx* ctx, const double* d_power, int n_prn, int n_freq, int nsamp, int k, int guard, gj_acq_peak* d_peaks,
                     gj_acq_floor* d_floor) {
    if (!ctx) return GJ_ERR_INVALID;
    Guard lock(ctx);
    if (!d_power || !d_peaks || !d_floor) return fail(ctx, GJ_ERR_INVALID, "null buffer");
    if ((reinterpret_cast<uintptr_t>(d_power) | reinterpret_cast<uintptr_t>(d_peaks) | reinterpret_cast<uintptr_t>(d_floor)) & 7)
        return fail(ctx, GJ_ERR_INVALID, "the surface and the records must be 8-byte aligned");
    if (nsamp < kPeakMinSamp || nsamp > kPeakMaxSamp) return fail(ctx, GJ_ERR_UNSUPPORTED, "nsamp %d (%d .. %d)", nsamp, kPeakMinSamp, kPeakMaxSamp);
    if (n_freq < 1 || n_freq > kPeakMaxFreq) return fail(ctx, GJ_ERR_UNSUPPORTED, "n_freq %d (1 .. %d)", n_freq, kPeakMaxFreq);
    if (k < 1 || k > GJ_ACQ_MAX_PEAKS) return fail(ctx, GJ_ERR_UNSUPPORTED, "k %d (1 .. %d)", k, GJ_ACQ_MAX_PEAKS);
    if (n_prn < 1) return fail(ctx, GJ_ERR_INVALID, "n_prn %d", n_prn);
    if (guard < 0) return fail(ctx, GJ_ERR_INVALID, "guard %d", guard);
    if ((long long)k * (2ll * guard + 1) >= (long long)nsamp)
        return fail(ctx, GJ_ERR_INVALID, "%d zones of %lld columns leave none of %d", k, 2ll * guard + 1, nsamp);
    if (int rc = ensure_workspace(ctx, peaks_workspace(nsamp, n_prn))) return rc;
    const size_t cols = (size_t)n_prn * (size_t)nsamp;
    PeakWs ws;
    ws.colmax = reinterpret_cast<double*>(ctx->ws);
    ws.colsum = reinterpret_cast<double*>(ctx->ws + align_up(cols * sizeof(double), 256));
    ws.colrow = reinterpret_cast<int*>(ctx->ws + 2 * align_up(cols * sizeof(double), 256));
    hipLaunchKernelGGL(peaks_columns_kernel, dim3((unsigned)n_prn, (unsigned)((nsamp + kPeakCols - 1) / kPeakCols)), dim3(kPeakThreads), 0,
                       ctx->stream, d_power, n_freq, nsamp, ws);
    GJ_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(peaks_pick_kernel, dim3((unsigned)n_prn), dim3(kPickThreads), 0, ctx->stream, ws, n_freq, nsamp, k, guard, d_peaks,
                       d_floor);
    GJ_LAUNCH_CHECK(ctx);
    return GJ_OK;
}

}   // extern "C"
