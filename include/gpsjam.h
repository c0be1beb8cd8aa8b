/* gpsjam.h -- C-ABI of libgpsjam_hip.so: the MI355X (gfx950) implementation of the
 * jamming-detection DSP path of mfkiwl/GPS-JAMMING.
 *
 * The reference has no FFI for this path (it is numpy/scipy called from Python); the
 * entry points below are what its Python call sites bind through ctypes instead of
 * numpy/scipy.  Each one names the reference code it replaces (path:line relative to the
 * reference root).  INTEGRATION.md shows the ctypes stubs a maintainer adds.
 *
 * Conventions
 *  - every function returns GJ_OK (0) or a negative gj_status; gj_strerror() gives text,
 *    gj_last_error() the detailed message of the last failure on a context;
 *  - plain pointers and sizes only; the caller owns every buffer;
 *  - one opaque gj_ctx per GPU; different contexts are independent; the library may be entered
 *    from several host threads (the GUI's QThread, its HTTP handler thread, its triangulation
 *    thread).  The context's internal mutex is held only while work is ENQUEUED, never across a
 *    host-side wait, a file read or a staged copy, and it is a robust mutex: a caller that is
 *    killed inside a call (QThread.terminate(), GpsJammerApp/app/ui_mainwindow.py:818-826) does
 *    not block the next one.  Every "*_u8" / upload call works in buffers of its own (a "lane":
 *    device staging, pinned bounce buffers, events), so concurrent calls on one context never
 *    share a result area; kernels of all calls are ordered on the context's one stream.  The lane of
 *    a killed caller is taken back -- drained and emptied -- at the next lane check-out or
 *    gj_debug_counters call after its thread has ended (see "Diagnostics" below for exactly what);
 *  - "*_dev" functions take DEVICE pointers, enqueue on the context's stream and return
 *    without synchronising (results land in device memory; no host synchronisation, no
 *    allocation when the workspace has been reserved) -- this is what bench.py times;
 *  - "*_u8" functions take HOST buffers (numpy arrays), stage them to HBM, run the same
 *    kernels, copy the small results back and return synchronously, reporting the
 *    kernel-only time measured with HIP events on the context's stream.  Their input may also
 *    be a DEVICE pointer (a resident capture from gj_upload / gj_upload_file / gj_malloc, or
 *    an address inside one): it is then used in place and nothing is staged;
 *  - samples are interleaved unsigned 8-bit I,Q,I,Q,... (RTL-SDR, README.md:95); one
 *    "sample" = one I/Q pair = 2 bytes.
 */
#ifndef GPSJAM_H
#define GPSJAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GJ_VERSION 150 /* 0.1.5: no new entry points.  gj_amp_stats_* / gj_onset_* run the fused pass + tail (any alignment accepted; same bits as gj_capture_scan_dev); gj_set_stream orders the new stream behind the old one; gj_ingest_files leaves the context's fill-thread setting alone */

typedef struct gj_ctx gj_ctx;

typedef enum gj_status {
    GJ_OK = 0,
    GJ_ERR_INVALID = -1,     /* bad argument */
    GJ_ERR_HIP = -2,         /* a HIP runtime call failed (see gj_last_error) */
    GJ_ERR_NOMEM = -3,       /* device or host allocation failed */
    GJ_ERR_NODEVICE = -4,    /* no such GPU */
    GJ_ERR_UNSUPPORTED = -5, /* size / parameter outside what the kernels implement */
    GJ_ERR_CAPACITY = -6     /* caller's output buffer too small */
} gj_status;

/* ---------------------------------------------------------------- context ---------- */
int gj_version(void);
const char* gj_strerror(int status);
const char* gj_last_error(gj_ctx* ctx); /* of the CALLING THREAD's last failure (kept per thread) */
int gj_device_count(int* count);
int gj_create(int device_id, gj_ctx** out);
/* gj_destroy: idempotent on NULL.  Takes down the communicators made on the context (their handles stay valid for
 * gj_comm_destroy); a collective another thread is still enqueueing on one of them returns first.  No OTHER call on
 * the context may be in progress or start while it is being destroyed. */
int gj_destroy(gj_ctx* ctx);
/* external != 0: run on the caller's HIP stream `hip_stream` (e.g.
 * torch.cuda.current_stream().cuda_stream; NULL then means the legacy default stream);
 * external == 0: back to the context's own non-blocking stream.
 * ONE stream at a time per context: a context's kernels hand results between workgroups through arrival counters that
 * belong to the context, and its workspace is one arena, so two launches of one context must never be in flight on two
 * streams at once.  The switch itself sees to that -- the new stream is ordered behind everything the context has queued
 * on the old one (an event + a wait; skipped while either stream is being captured into a graph) -- and a caller who
 * wants two streams to run side by side uses two contexts (gpsjam/sharded.py, split.py, local.py do). */
int gj_set_stream(gj_ctx* ctx, void* hip_stream, int external);
int gj_synchronize(gj_ctx* ctx);
/* Unpack convention of the uint8 samples on this context: sample = (u8 - offset) * scale.  The
 * reference uses three: u - 127.5 (worker.py:222, checkIfJamming.py:15,
 * triangulateTDOA.py:34), (u - 127.5)/127.5 (triangulateRSSI.py:30, widmo_plot.py:39-40) and
 * (int8)(u - 128) (GpsJammerApp/backend/sdrrcv.c:104-106).  The default (127.5, 1/127.5)
 * reproduces the first two: `offset` is honoured by every kernel, `scale` by the kernels whose
 * reference normalises (K2 Welch, K3 amplitude); K1, K4, K5 work in LSB units like their
 * references.  offset must be a multiple of 0.5 in [0, 255] (sums stay exact integers).
 * gj_set_unpack(ctx, 128, 1/128.) gives the gnssdec convention; the acquisition search always
 * uses 128 as its reference does. */
int gj_set_unpack(gj_ctx* ctx, double offset, double scale);
int gj_get_unpack(gj_ctx* ctx, double* offset, double* scale);
int gj_device_info(gj_ctx* ctx, char* name, size_t name_cap, int* compute_units,
                   uint64_t* hbm_bytes);
/* Which physical GPU this context runs on, as text: "pci=<domain:bus:device.function> uuid=<hex> hip=<index>".
 * Ranks of a multi-GPU run exchange these so that the collecting rank can tell N GPUs from N ranks on one
 * (bench.py's `devices` list). */
int gj_device_identity(gj_ctx* ctx, char* out, size_t cap);
/* Pre-size the internal workspace so that later *_dev calls allocate nothing. */
int gj_reserve(gj_ctx* ctx, size_t workspace_bytes);
/* Diagnostics.  The hook is called, with NO internal lock held, right before every host-side wait of
 * the library (site: 1 event, 2 stream, 3 staged copy, 4 waiting for a free lane); tests park or end
 * a thread there to show that an abandoned caller blocks nobody.  Site 5 is the exception: it is
 * inside gj_debug_counters WITH the lock held, so that a test can end a thread as the mutex's owner
 * and watch the next caller recover it.  NULL removes the hook.  The counters:
 * lanes made, lanes in use, lanes taken back from callers whose thread had ended, and how often the
 * context mutex was found with a dead owner.
 *
 * What happens to a caller that is killed inside a call, and when: the calling thread holds its lane's
 * owner token -- a robust mutex -- from check-out to check-in.  The kernel marks that token "owner
 * died" while the thread exits, before the thread can be joined, so there is no interval in which a dead
 * caller looks alive and no thread id a later thread could inherit.  EVERY later lane check-out (any
 * "*_u8" / upload / ingest call, from any thread) and every gj_debug_counters call first sweeps all
 * lanes in use; a lane whose owner has ended is taken over by the sweeping thread, which -- holding
 * no lock -- waits for whatever the dead caller had queued (the context's streams, the lane's copy
 * stream and bounce-buffer events), frees everything the lane had grown to (device staging, pinned
 * buffers, events, copy stream, ingest workspace) and returns it to the pool.  Not covered: the
 * resident capture a killed gj_upload / gj_ingest had allocated but not yet handed out (that device
 * memory stays allocated until gj_destroy of the process' GPU context), and a kill in the middle of a
 * staged copy whose helper threads are still running. */
int gj_debug_set_wait_hook(gj_ctx* ctx, void (*hook)(void* arg, int site), void* arg);
int gj_debug_counters(gj_ctx* ctx, int* lanes, int* lanes_busy, int* lanes_reclaimed, int* owner_deaths);
/* Fault injection for tests.  GJ_INJECT_OWNER_ALIVE: the next `count` owner probes of a lane in use are
 * skipped, i.e. answer "its caller is alive" whatever the truth -- the wrong answer that round 4's
 * sampled probe gave inside the thread-exit window.  A test uses it to show that a lane missed once is
 * still taken back at the next check-out or counters call. */
#define GJ_INJECT_OWNER_ALIVE 1
/* GJ_INJECT_FILL_WORKSPACE: `count` is a byte, 0..255 (anything else is GJ_ERR_INVALID).  Enqueues ONE memset of that
 * byte over the whole of the context's current workspace arena, on the context's stream: behind everything already
 * queued there, in front of the next call.  Without an arena it does nothing.  It touches neither the tables, nor the
 * arrival counters, nor an arena that a growth has retired.  A test uses it to show that no kernel reads a workspace
 * word that its own call has not written: 0xFF makes such a float a NaN and such a counter or flag all-ones, 0x7F a
 * large finite float and a large positive int. */
#define GJ_INJECT_FILL_WORKSPACE 2
int gj_debug_inject(gj_ctx* ctx, int what, int count);

/* Stream-overlap probe.  Keeps the context's stream busy for `milliseconds` (0..100; more is refused) with ONE wave
 * that spins on the 100-MHz real-time counter: the chip stays free, the stream -- and the hardware queue the runtime
 * mapped it to -- does not.  A host that needs two streams to run side by side uses it to find out whether they share
 * a hardware queue (the HIP runtime deals streams over GPU_MAX_HW_QUEUES queues, four by default, and two streams on
 * one queue run one after the other): gpsjam/streams.py, which the pipelines of gpsjam/sharded.py, split.py and
 * local.py call at construction.  Enqueues only; never synchronises. */
int gj_probe_busy_dev(gj_ctx* ctx, float milliseconds);

/* device memory for callers that do not bring their own allocator (torch) */
int gj_malloc(gj_ctx* ctx, size_t bytes, void** dptr);
int gj_free(gj_ctx* ctx, void* dptr);
int gj_memcpy_h2d(gj_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int gj_memcpy_d2h(gj_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* Resident captures: one upload, then any number of *_dev calls on the returned device pointer
 * (free with gj_free).  The "*_u8" entry points below stage their input on EVERY call; a caller
 * that runs scan + PSD + RSSI on one file uploads it once with these.  gj_upload_file is the
 * reference's ingest (np.fromfile / f.read: GpsJammerApp/app/worker.py:209-217,
 * skrypty/triangulateRSSI.py:29, skrypty/triangulateTDOA.py:33) as file -> pinned bounce buffers
 * -> HBM; max_bytes = 0 reads to the end of the file. */
int gj_upload(gj_ctx* ctx, const uint8_t* host, size_t nbytes, void** dptr);
int gj_upload_file(gj_ctx* ctx, const char* path, size_t offset, size_t max_bytes, void** dptr,
                   size_t* nbytes_out);

/* Host threads that fill the pinned bounce buffers of ONE staged copy (gj_upload*, gj_ingest_*): 0 = by capture size (two
 * to eight: four for the reference's 10-s captures, eight from 64 MiB up -- starting and joining eight threads costs a
 * 41-MB capture more than they carry), 1..16 = that many.  For a host that brings in several files at once from threads
 * of its own (one lane per call) and wants them to share the cores.  GPSJAM_FILL_THREADS in the environment overrides
 * both. */
int gj_set_fill_threads(gj_ctx* ctx, int n);

/* HIP-event stopwatch on the context's stream (what bench.py's roofline uses) */
int gj_timer_start(gj_ctx* ctx);
int gj_timer_stop(gj_ctx* ctx, float* elapsed_ms); /* synchronises on the stop event */

/* ------------------------------------------------- K1: per-chunk power scan --------- */
/* Replaces the loop of GPSAnalysisThread.precalculate_power_profile
 * (GpsJammerApp/app/worker.py:216-230) and analyze_chunk_power
 * (GpsJammerApp/app/checkIfJamming.py:7-20, with GJ_CP_ODD_CHUNK_ZERO, eps = 0).
 * power[c] = mean over the I/Q pairs of chunk c of (I-127.5)^2+(Q-127.5)^2, + eps.
 * The ragged tail chunk is included; a trailing odd byte is dropped (worker.py:226);
 * a chunk without a complete pair gives NaN (numpy mean of empty) unless the flag below
 * is set.  The chunk sum is accumulated as an exact integer and rounded once. */
#define GJ_CP_ODD_CHUNK_ZERO 1 /* odd-sized or empty chunk -> 0.0 (checkIfJamming.py:12-13) */
size_t gj_chunk_count(size_t nbytes, size_t chunk_bytes);
int gj_chunk_power_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t chunk_bytes,
                       float eps, int flags, float* d_power /* [gj_chunk_count] */);
int gj_chunk_power_u8(gj_ctx* ctx, const uint8_t* iq, size_t nbytes, size_t chunk_bytes,
                      float eps, int flags, float* power, size_t power_cap, size_t* n_out,
                      float* kernel_ms);

/* Noise floor + threshold (worker.py:241-248): baseline = numpy.percentile(power, pct)
 * with numpy's float32 'linear' rule, 1.0 if <= 0; threshold = baseline * 10^(rise_db/10);
 * mask[c] = power[c] > threshold.  d_stats = {baseline, threshold, count_above}. */
int gj_power_threshold_dev(gj_ctx* ctx, const float* d_power, size_t n, float pct,
                           float rise_db, float* d_stats /* [3] */, uint8_t* d_mask /* [n] or NULL */);

/* ------------------------------------------------- K2: Welch PSD waterfall ---------- */
/* Replaces the chunk body of analyze_full_file (skrypty/widmo_plot.py:26-54) including
 * its scipy.signal.welch(x, fs, nperseg=N, return_onesided=False) call (:48):
 * per chunk of chunk_samples I/Q pairs: x = ((I-127.5) + j(Q-127.5))/127.5, periodic Hann,
 * 50 % overlap, per-segment mean removal, |FFT|^2 averaged over the segments,
 * scale 1/(fs*sum(w^2)); a trailing partial chunk is kept when it holds at least
 * nperseg samples (widmo_plot.py:31).  nperseg: power of two, 16..4096;
 * chunk_samples >= nperseg and chunk_samples + nperseg < 2^31 (a chunk is addressed with 32-bit
 * byte offsets; GJ_ERR_UNSUPPORTED otherwise -- the capture itself may be any length).
 * Output rows are float32[nperseg]; GJ_WELCH_SHIFT applies numpy.fft.fftshift (:51);
 * d_psd_db (optional) receives 10*log10(psd + 1e-15) (:52). */
#define GJ_WELCH_SHIFT 1
size_t gj_welch_rows(size_t nbytes, size_t chunk_samples, int nperseg);
int gj_welch_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t chunk_samples,
                 int nperseg, double fs, int flags, float* d_psd /* [rows*nperseg] */,
                 float* d_psd_db /* [rows*nperseg] or NULL */);
int gj_welch_u8(gj_ctx* ctx, const uint8_t* iq, size_t nbytes, size_t chunk_samples,
                int nperseg, double fs, int flags, float* psd, float* psd_db, size_t cap_floats,
                size_t* rows_out, float* kernel_ms);
/* n captures of ONE length (nbytes_each) in one transform launch + one finalize launch: the reference's deployment is
 * three antenna recordings of one length (GpsJammerApp/app/worker.py:97-101), and at 10-s captures a step's time is its
 * launch gaps and grid tails, not its bytes.  Each capture is planned, cut into workgroups and summed exactly as by
 * gj_welch_dev on its own, so d_psd[a] receives the same bits; d_psd[a] must be 16-byte aligned. */
int gj_welch_batch_dev(gj_ctx* ctx, const uint8_t* const* d_iq, int n_captures, size_t nbytes_each, size_t chunk_samples,
                       int nperseg, double fs, int flags, float* const* d_psd /* [n_captures] x [rows*nperseg] */);
/* Measurement: gj_welch_dev with HIP events around the transform launch and around the finalize launch (the sum over
 * the per-workgroup spectra, scaling, fftshift, dB), on the context's stream; synchronises and reports both.  bench.py
 * times K2 at nperseg 4096 and 1024 with it, interleaved, so that the two figures of one line come from the same
 * minute of the same box. */
int gj_welch_timed_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t chunk_samples, int nperseg, double fs,
                       int flags, float* d_psd, float* d_psd_db, float* kernel_ms, float* finalize_ms);
/* workspace bytes gj_welch_dev needs for this input (for gj_reserve) */
size_t gj_welch_workspace(gj_ctx* ctx, size_t nbytes, size_t chunk_samples, int nperseg);

/* ------------------------------------------------- short-time spectral ridge -------- */
/* Per short frame: where the spectral peak is and how much of the frame's power it holds -- the time series that tells
 * the reference simulator's four interferers apart (simulate/frontend/jammers/: cwJammer.py, chirpJammer.py,
 * pulsedJammer.py, broadbandJammer.py; gpsjam/classify.py reads it).  For frame f = 0 .. n_frames-1, with
 * s_f = first_sample + f*hop and N = nfft:
 *
 *   x[t]    = ((I_t - offset) + j(Q_t - offset)) * scale      K2's unpacking; honours gj_set_unpack
 *   w[n]    = 0.5 - 0.5 cos(2 pi n / N)                        periodic Hann, K2's table
 *   X_f[k]  = sum_{n<N} w[n] x[s_f + n] exp(-2 pi i k n / N)   NO mean removal, NO 1/(fs sum w^2) scaling
 *   P_f[k]  = |X_f[k]|^2
 *
 * (no mean removal: pulsedJammer.py's carrier sits at 0 Hz, and a detrend would erase it).
 * nfft: a power of two, 16..4096 (GJ_ERR_UNSUPPORTED otherwise).  hop >= 1, otherwise arbitrary (odd, larger than nfft,
 * not a divisor of it); first_sample may be odd; 0 <= guard and 2*guard + 1 < nfft.  n_frames == 0, a last frame that
 * runs past the capture, a null or odd d_iq, a d_out that is not 4-byte aligned: GJ_ERR_INVALID.  A refused call
 * enqueues nothing.  Needs no workspace.
 * Determinism: one transform group computes one frame and `total` is summed in an order that depends on nfft alone, so
 * frame f of a call is bit-identical to frame f-k of the same call started at first_sample + k*hop, and two identical
 * calls give identical bytes. */
typedef struct gj_ridge_frame {   /* 16 bytes */
    float total;      /* sum_k P_f[k] */
    float peak;       /* max_k P_f[k] */
    float second;     /* max P_f[k] over bins whose circular distance to peak_bin is > guard; 0 if none */
    int32_t peak_bin; /* 0..N-1 in FFT order (k >= N/2 is negative frequency); equal values: smallest k */
} gj_ridge_frame;
/* whole frames that fit: pure host arithmetic, no context; 0 for an impossible geometry (nfft < 1, hop < 1, no room) */
size_t gj_ridge_frames(size_t nbytes, size_t first_sample, int nfft, size_t hop);
int gj_ridge_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, int nfft, size_t hop,
                 size_t n_frames, int guard, gj_ridge_frame* d_out /* [n_frames] */);

/* ------------------------------------------------- chirp-rate search ---------------- */
/* The ridge behind a de-chirp, for every rate of a grid: a sweep that crosses many bins inside ONE frame does not
 * concentrate in any bin of that frame (gj_ridge_dev reads it as broadband); multiplied by the conjugate of a unit
 * chirp of the right rate it is a tone again, and the rate that concentrates it best is the sweep rate, measured inside
 * a frame instead of across frames (gpsjam/classify.py classify_swept reads the result).  For frame
 * f = 0 .. n_frames-1 at s_f = first_sample + f*hop, with N = nfft and q_r = rate_first + r*rate_step, r = 0 .. n_rates-1:
 *
 *   x[t], w[n]     exactly gj_ridge_dev's (unpack convention honoured, periodic Hann, no mean removal)
 *   m_r[n]  = (q_r * n^2) mod 2 N^2                                  exact integer arithmetic
 *   c_r[n]  = exp(-i pi m_r[n] / N^2)
 *   Y_fr[k] = sum_{n<N} w[n] x[s_f + n] c_r[n] exp(-2 pi i k n / N)
 *   P_fr[k] = |Y_fr[k]|^2                                            the units of gj_ridge_dev
 *   peak_fr = max_k P_fr[k]
 *
 * q counts bins per frame length: one unit is a sweep of fs/N Hz in N/fs seconds, fs^2 / N^2 Hz/s.  q > 0 de-chirps an
 * up-sweep.  At the matching q the peak bin is the sweep's frequency at the START of the frame; its frequency at the
 * frame's centre is bin + q/2 (in bins, modulo N).  Only integer q are searched.
 * Limits: nfft a power of two, 16..4096, and n_rates <= GJ_CHIRP_MAX_RATES (GJ_ERR_UNSUPPORTED otherwise);
 * n_rates >= 1, rate_step >= 1 and every |q_r| <= N^2 / 2 (beyond that the chirp's own frequency aliases); hop,
 * first_sample, guard, n_frames (gj_ridge_frames counts the frames that fit), d_iq and d_out as gj_ridge_dev; d_peaks
 * 4-byte aligned: GJ_ERR_INVALID otherwise.  A refused call enqueues nothing.  Needs no workspace; one launch on the
 * context's stream.
 * Determinism: one transform group computes all rates of one frame from that frame's bytes alone, and the rates are
 * independent of each other: c_r is evaluated from q_r's integer phase, nothing is carried from one rate to the next.
 * So d_peaks[f][r] is bit-identical to the `peak` of a call with the single rate q_r; frame f of a call is bit-identical
 * to frame f-k of the same call started at first_sample + k*hop; two identical calls give identical bytes; and a call
 * with the single rate 0 writes into the first 16 bytes of every record exactly the bytes gj_ridge_dev writes
 * (c_0 = (1, 0), and multiplying by it is exact). */
#define GJ_CHIRP_MAX_RATES 256
typedef struct gj_chirp_frame {   /* 24 bytes; the first four fields are gj_ridge_frame's, taken at rate_index */
    float total;        /* sum_k P_fr[k] */
    float peak;         /* max_k P_fr[k] = peak_fr */
    float second;       /* max P_fr[k] over bins whose circular distance to peak_bin is > guard; 0 if none */
    int32_t peak_bin;   /* 0..N-1 in FFT order; equal values: smallest k */
    int32_t rate_index; /* the r with the largest peak_fr; equal values: smallest r */
    int32_t reserved;   /* 0 */
} gj_chirp_frame;
int gj_chirp_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, int nfft, size_t hop,
                 size_t n_frames, int guard, int rate_first, int rate_step, int n_rates,
                 gj_chirp_frame* d_out /* [n_frames] */, float* d_peaks /* [n_frames][n_rates] or NULL */);

/* ------------------------------------------------- spectral kurtosis ---------------- */
/* Floor-free per-bin interference detection (Nita & Gary's estimator; gpsjam/kurtosis.py reads it): for every bin the
 * sums of P and of P^2 over the M = frames_per_row short spectra of a row.  Gaussian noise gives SK = 1 whatever its
 * level or the passband's shape, a steady carrier pulls its bin toward 0, anything intermittent (pulses, a chirp that
 * crosses the bin) pushes it above 1; the estimator's standard deviation under noise is 2 / sqrt(M).  Blind spots, by
 * construction: a Gaussian broadband jammer and a pulse train of exactly 50 % duty both have SK = 1.
 * With N = nfft, row r = 0 .. n_rows-1 holds the frames f = r*M + m, m = 0 .. M-1, at s_f = first_sample + f*hop:
 *
 *   x[t]     = (I_t - offset) + j(Q_t - offset)                  un-normalised; honours gj_set_unpack's offset
 *   w[n]     = 0.5 - 0.5 cos(2 pi n / N)                          periodic Hann, K2's table
 *   X_f[k]   = sum_{n<N} w[n] x[s_f + n] exp(-2 pi i k n / N)     no mean removal
 *   P_f[k]   = |X_f[k]|^2 * scale^2                               the units of gj_ridge_dev and gj_excise_dev
 *   S1[r][k] = sum_m P_f[k]          S2[r][k] = sum_m P_f[k]^2
 *   SK[r][k] = (M+1)/(M-1) * (M * S2 / S1^2 - 1)                  NaN where S1 == 0
 *
 * S1 / M is the mean of the very P_f[k] that gj_excise_dev compares with its threshold.
 * d_s1, d_s2: float32[n_rows][nfft] in FFT order; d_sk: the same shape, or NULL.  SK is evaluated in double from the
 * float32 values written to d_s1 and d_s2 and rounded once.
 * nfft: a power of two, 16..4096 (GJ_ERR_UNSUPPORTED otherwise).  hop >= 1, otherwise arbitrary (hop = nfft gives
 * independent frames); first_sample may be odd.  2 <= frames_per_row <= 65536 (below 2: GJ_ERR_INVALID, the estimator
 * is undefined; above: GJ_ERR_UNSUPPORTED).  n_rows == 0 or more rows than fit, a null or odd d_iq, a null d_s1 or
 * d_s2, an output that is not 4-byte aligned: GJ_ERR_INVALID.  A refused call enqueues nothing.  Enqueues on the
 * context's stream (two launches) and returns; allocates nothing when gj_sk_workspace bytes were reserved.
 * Determinism: a row is cut into blocks of at most 16 consecutive frames by a rule that depends on frames_per_row
 * alone; one transform group sums a block frame by frame in float32, and the blocks of a row are added in order.  So
 * row r of a call is bit-identical to row r-k of the same call started at first_sample + k*frames_per_row*hop and to
 * row r of a call with fewer rows, and two identical calls give identical bytes. */
/* whole rows that fit: pure host arithmetic, no context; 0 for an impossible geometry (nfft < 1, hop < 1,
 * frames_per_row < 1, no room) */
size_t gj_sk_rows(size_t nbytes, size_t first_sample, int nfft, size_t hop, int frames_per_row);
/* workspace bytes gj_sk_dev needs for the partial sums (for gj_reserve); 0 for parameters gj_sk_dev refuses */
size_t gj_sk_workspace(gj_ctx* ctx, int nfft, int frames_per_row, size_t n_rows);
int gj_sk_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, int nfft, size_t hop,
              int frames_per_row, size_t n_rows, float* d_s1 /* [n_rows*nfft] */, float* d_s2 /* [n_rows*nfft] */,
              float* d_sk /* [n_rows*nfft] or NULL */);

/* ------------------------------------------------- cross-spectral density ----------- */
/* The frequency-resolved question about a PAIR of captures (gpsjam/coherence.py reads it): which bins carry the same
 * source in both, and with what delay in each band.  Two antennas see the same jammer under independent receiver noise:
 * the magnitude-squared coherence is about 1/M under noise alone and (rho / (1 + rho))^2 in a bin of jammer-to-noise
 * ratio rho, also where the jammer lies below each receiver's noise floor and is Gaussian (the kurtosis's blind spot).
 * For Gaussian noise and independent frames P(MSC > g) = (1 - g)^(M-1) exactly (Carter): the detector needs no floor.
 * With N = nfft, M = frames_per_row, row r = 0 .. n_rows-1 holds the frames f = r*M + m, m = 0 .. M-1, at s_f = f*hop:
 *
 *   x_a[t]    = (I - offset) + j(Q - offset) of capture a at sample first_a + t     gj_set_unpack's offset; likewise x_b
 *   w[n]      = 0.5 - 0.5 cos(2 pi n / N)                          periodic Hann, K2's table; no mean removal
 *   A_f[k]    = sum_{n<N} w[n] x_a[s_f + n] exp(-2 pi i k n / N)   B_f[k] likewise from capture b at first_b
 *   Saa[r][k] = scale^2 sum_m |A_f[k]|^2     Sbb[r][k] = scale^2 sum_m |B_f[k]|^2      the units of gj_sk_dev's S1
 *   Sab[r][k] = scale^2 sum_m B_f[k] conj(A_f[k])
 *   MSC[r][k] = (re^2 + im^2) / (Saa Sbb)                          NaN where Saa Sbb == 0; not clamped
 *
 * Sign: if b is a delayed by D samples, arg Sab[k] = -2 pi k D / N with k signed, so D = -(N / 2 pi) d(arg)/dk, positive
 * when b is delayed: the convention of gj_xcorr_lags and gj_xcorr_fine_dev.
 * d_saa, d_sbb: float32[n_rows][nfft] in FFT order; d_sab: float32[n_rows][nfft][2], (re, im); d_msc: float32[n_rows][nfft]
 * or NULL.  MSC is evaluated in double from the float32 values written to the other three and rounded once; rounding may
 * carry it past 1.  The sums run in LSB units, scale^2 is applied once at the end.
 * nfft: a power of two, 16..4096 (GJ_ERR_UNSUPPORTED otherwise).  hop >= 1, otherwise arbitrary (hop >= nfft gives
 * independent frames); first_a and first_b may be odd and may differ; d_a == d_b and overlapping ranges are allowed.
 * 2 <= frames_per_row <= 65536 (below 2: GJ_ERR_INVALID, MSC is identically 1 at M = 1; above: GJ_ERR_UNSUPPORTED).
 * n_rows == 0 or more rows than gj_csd_rows, a null or odd d_a or d_b, a null d_saa, d_sbb or d_sab, a d_saa, d_sbb or
 * d_msc that is not 4-byte aligned, a d_sab that is not 8-byte aligned: GJ_ERR_INVALID.  A refused call enqueues
 * nothing.  Enqueues on the context's stream (two launches) and returns; allocates nothing when gj_csd_workspace bytes
 * were reserved.
 * Determinism: a row is cut into blocks by gj_sk_dev's rule -- ceil(M / 16) blocks of ceil(M / blocks) frames, the last
 * one shorter; one transform group sums a block frame by frame in float32, and the blocks of a row are added in order.
 * So row r of a call is bit-identical to row r-k of the call started k*M*hop samples later in both captures and to row r
 * of a call with fewer rows, two identical calls give identical bytes, d_msc == NULL changes no other bit, and Saa
 * depends on capture a's bytes alone (the same call against another b writes the same Saa), likewise Sbb on b's. */
/* whole rows that fit both captures: pure host arithmetic, no context; 0 for an impossible geometry */
size_t gj_csd_rows(size_t nbytes_a, size_t first_a, size_t nbytes_b, size_t first_b, int nfft, size_t hop,
                   int frames_per_row);
/* workspace bytes gj_csd_dev needs for the partial sums (for gj_reserve); 0 for parameters gj_csd_dev refuses and when
 * the product does not fit a size_t */
size_t gj_csd_workspace(gj_ctx* ctx, int nfft, int frames_per_row, size_t n_rows);
int gj_csd_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b, size_t nbytes_b,
               size_t first_b, int nfft, size_t hop, int frames_per_row, size_t n_rows, float* d_saa /* [n_rows*nfft] */,
               float* d_sbb /* [n_rows*nfft] */, float* d_sab /* [n_rows*nfft*2] */, float* d_msc /* [n_rows*nfft] or NULL */);

/* ------------------------------------------------- frequency-domain excision -------- */
/* The windowed 50 %-overlap FFT excisor of GPS receivers: a cleaned capture, uint8 I/Q again, with every bin above its
 * threshold taken out (the interferers of simulate/frontend/jammers/; gpsjam/mitigate.py builds the thresholds).  For a
 * range of n_samples I/Q pairs starting at first_sample, with N = nfft, h = N/2 and frames f = 0 .. F-1 at
 * s_f = first_sample + f*h:
 *
 *   F = gj_excise_frames(n_samples, nfft) = (n_samples - N) / h + 1   (0 if n_samples < N)
 *
 *   x[t]   = (I_t - offset) + j(Q_t - offset)          un-normalised; honours gj_set_unpack's offset
 *   w[n]   = 0.5 - 0.5 cos(2 pi n / N)                 K2's periodic Hann table
 *   X_f[k] = sum_n w[n] x[s_f + n] exp(-2 pi i k n / N)        no mean removal
 *   P_f[k] = |X_f[k]|^2 * scale^2                      the units of gj_ridge_dev
 *   M_f[k] = 0 if P_f[k] > thr[k] else 1               strict; thr = DEVICE float[N] in FFT order
 *   y_f    = IFFT_N(M_f * X_f)                         with the 1/N
 *   y[t]   = y_{f-1}[t - s_{f-1}] + y_f[t - s_f]       for t covered by two frames
 *
 * Periodic Hann at hop N/2 sums to exactly 1, so an all-ones mask gives y = x.
 * Output: d_out[2*n_samples] is range-relative, byte 0 is I of first_sample.  Samples [h, F*h) of the range receive
 * u = min(255, max(0, rint(fl32(y + offset)))) per component (rint: round half to even); the first half frame [0, h)
 * and everything from F*h to n_samples are copied from the input unchanged, so the cleaned capture has the length and
 * the byte coordinates of the original.  The call writes exactly 2*n_samples bytes.
 * Threshold values: +inf never excises, a negative value always does (a fixed notch), NaN never does.
 * d_frames (optional, may be NULL) receives one record per frame.
 * nfft: a power of two, 16..4096 (GJ_ERR_UNSUPPORTED otherwise).  GJ_ERR_INVALID: n_samples < nfft, a range that runs
 * past the capture, a null or odd d_iq, a null d_out or d_threshold, a d_threshold or d_frames that is not 4-byte
 * aligned, d_out[0, 2*n_samples) overlapping d_iq[0, nbytes) (frames read their neighbours: in place is wrong).
 * first_sample may be odd.  A refused call enqueues nothing.  Needs no workspace; enqueues and returns.
 * Determinism: an excised sample depends only on the bytes of the two frames that cover it and every sum runs in an
 * order fixed by nfft, so a call started k*h samples later reproduces the overlapping interior bytes and the records of
 * the shared frames bit for bit, and two identical calls give identical bytes. */
typedef struct gj_excise_frame {   /* 16 bytes */
    float total;       /* sum_k P_f[k] */
    float removed;     /* sum of P_f[k] over the excised bins */
    int32_t n_excised; /* bins with M_f[k] = 0 */
    int32_t reserved;  /* 0 */
} gj_excise_frame;
/* frames of the excisor: pure host arithmetic, no context */
size_t gj_excise_frames(size_t n_samples, int nfft);
int gj_excise_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int nfft,
                  const float* d_threshold /* [nfft] */, uint8_t* d_out /* [2*n_samples] */,
                  gj_excise_frame* d_frames /* [F] or NULL */);

/* ------------------------------------------------- chirp-domain excision ------------ */
/* De-chirp, notch, re-chirp: gj_excise_dev with every frame multiplied by the conjugate of a unit chirp of ITS OWN
 * rate in front of the transform and by the chirp itself behind the inverse.  A sweep that crosses hundreds of bins
 * inside one frame is a line of a few bins behind the de-chirp of its rate (gj_chirp_dev measures that rate), so the
 * mask removes the sweep and little else; gj_excise_dev sees it smeared and cuts nothing, or the signal with it.
 * With F, h, s_f, x, w, scale and the output rule exactly gj_excise_dev's, and c exactly gj_chirp_dev's:
 *
 *   q_f     = d_rate[f]                                 DEVICE int32[F]; any value, the phase is taken modulo 2 N^2
 *   c_f[n]  = exp(-i pi ((q_f n^2) mod 2 N^2) / N^2)      exact integer arithmetic
 *   X_f[k]  = sum_n w[n] x[s_f + n] c_f[n] exp(-2 pi i k n / N)
 *   P_f[k]  = |X_f[k]|^2 * scale^2
 *   M_f[k]  = 0 if P_f[k] > thr[k] else 1                strict; +inf, negative and NaN as gj_excise_dev
 *   y_f[n]  = conj(c_f[n]) * IFFT_N(M_f * X_f)[n]
 *   y[t]    = y_{f-1}[t - s_{f-1}] + y_f[t - s_f]
 *
 * |c| = 1, so an all-ones mask still gives y = x whatever the rates.  The records are gj_excise_frame, taken in the
 * de-chirped domain.  Edges, length and byte coordinates as gj_excise_dev: exactly 2*n_samples bytes are written.
 * One unit of q is fs^2 / N^2 Hz/s; only integer rates exist, and a frame has one rate.  A threshold that follows the
 * passband's shape is of little use here: the de-chirp smears that shape over the bins.
 * Refusals: those of gj_excise_dev, and a null d_rate or one that is not 4-byte aligned (GJ_ERR_INVALID).  No rate
 * VALUE is refused; the host never reads d_rate.  A refused call enqueues nothing.  Needs no workspace; enqueues on the
 * context's stream (two launches) and returns.
 * Determinism: a frame's spectrum, mask and re-chirped inverse depend on that frame's bytes and its own q_f alone, so
 * a call started k*h samples later with d_rate + k reproduces the overlapping interior bytes and the records of the
 * shared frames bit for bit; two identical calls give identical bytes; and with every q_f = 0, or any multiple of
 * 2 N^2, the call writes exactly the bytes and records of gj_excise_dev (every factor is then exactly (1, 0)). */
int gj_excise_chirp_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int nfft,
                        const int32_t* d_rate /* [F] */, const float* d_threshold /* [nfft] */,
                        uint8_t* d_out /* [2*n_samples] */, gj_excise_frame* d_frames /* [F] or NULL */);
/* The rates for gj_excise_chirp_dev out of a gj_chirp_dev scan, without a pass through the host.  Scan the same
 * first_sample at hop = nfft/2 over the grid (rate_first, rate_step, n_rates): frame f of the scan is frame f of the
 * excisor.  For f = 0 .. n_frames-1, with total, peak and rate_index the fields of d_scan[f]:
 *
 *   d_rate[f] = rate_first + rate_index * rate_step   if total > 0 and peak >= fl32(min_concentration * total)
 *             = 0                                     otherwise (also when a NaN is compared)
 *
 * fl32(.) is ONE float32 multiplication.  The sum is taken modulo 2^32.  Frames the search could not concentrate --
 * noise, a quiet lead-in, the frame that holds a saw-tooth's fly-back -- are thus excised as plain frames.
 * GJ_ERR_INVALID: a null or not 4-byte aligned d_scan or d_rate, n_frames == 0, rate_step < 1.  A refused call enqueues
 * nothing.  One launch on the context's stream. */
int gj_chirp_rates_dev(gj_ctx* ctx, const gj_chirp_frame* d_scan, size_t n_frames, int rate_first, int rate_step,
                       float min_concentration, int32_t* d_rate /* [n_frames] */);

/* ------------------------------------------------- two-antenna per-bin canceller ---- */
/* The frequency-domain sidelobe canceller (per-bin power inversion) of a receiver with two antennas: capture a's short
 * spectrum is predicted from capture b's with one complex weight per bin, the prediction is subtracted, and the rest
 * goes back to uint8 I/Q through the excisor's mask and overlap-add.  What is coherent between the antennas is removed,
 * a broadband Gaussian jammer included, which no threshold, de-chirp or blanker can touch; satellites arrive from other
 * directions with another inter-antenna phase and stay.  The MMSE weight is W[k] = conj(Sab[k]) / Sbb[k] of gj_csd_dev's
 * sums (gpsjam/coherence.py builds it).  With F, h = N/2, w, x (per capture), scale, the output rule and the copied edges
 * exactly gj_excise_dev's, F = gj_excise_frames(n_samples, nfft), and frames f = 0 .. F-1:
 *
 *   A_f[k]  = sum_n w[n] x_a[first_a + f*h + n] exp(-2 pi i k n / N)     B_f[k] likewise from capture b at first_b + f*h
 *   set(f)  = min(f / frames_per_set, n_sets - 1)                         integer division
 *   Y_f[k]  = A_f[k] - W[set(f)][k] * B_f[k]          every product of W * B rounded on its own, then the subtraction
 *   P_f[k]  = |Y_f[k]|^2 * scale^2
 *   M_f[k]  = 0 if P_f[k] > thr[k] else 1             strict; +inf never, negative always, NaN never, as gj_excise_dev
 *   y_f     = IFFT_N(M_f * Y_f)                       with the 1/N
 *   y[t]    = y_{f-1}[t - s_{f-1}] + y_f[t - s_f]     for t covered by two frames
 *
 * d_weights: DEVICE float32[n_sets][nfft][2], (re, im), FFT order; the host never reads it.  With every weight 0 the
 * call writes exactly the bytes of gj_excise_dev on capture a, and its total, removed and n_excised.
 * Output: d_out[2*n_samples], range-relative as gj_excise_dev's; the first half frame and everything from F*h on are
 * copied from capture a.  The call writes exactly 2*n_samples bytes.  d_frames (optional) receives one record per frame.
 * first_a and first_b may be odd and may differ; d_a == d_b is allowed.
 * Refusals: those of gj_excise_dev for each capture (nfft, n_samples < nfft, a range past either capture, a null or odd
 * d_a or d_b, a null d_out or d_threshold, a d_threshold or d_frames that is not 4-byte aligned, d_out overlapping either
 * capture), frames_per_set == 0 or n_sets == 0, a null d_weights or one that is not 8-byte aligned (GJ_ERR_INVALID but
 * for nfft: GJ_ERR_UNSUPPORTED).  A refused call enqueues nothing.  Needs no workspace; enqueues on the context's stream
 * (two launches: the transform kernel and the edge copy) and returns.
 * Determinism: an output sample depends only on the bytes of the two frame pairs that cover it and on their weight sets,
 * and every sum runs in an order fixed by nfft.  So a call started k*h samples later in both captures, with the sets
 * shifted alike, reproduces the overlapping interior bytes and the records of the shared frames bit for bit; two
 * identical calls give identical bytes; and d_frames == NULL changes no byte.
 * Limits: one auxiliary antenna gives one null per bin -- a signal whose inter-antenna phase is near the jammer's is
 * attenuated with it -- and capture a's receiver noise rises by up to 1 + |W|^2.  The pair must share a clock and be
 * aligned to well under nfft samples, as for gj_csd_dev. */
typedef struct gj_cancel_frame {   /* 16 bytes */
    float total_in;    /* sum_k |A_f[k]|^2 scale^2 */
    float total;       /* sum_k P_f[k], behind the cancellation */
    float removed;     /* sum of P_f[k] over the excised bins */
    int32_t n_excised; /* bins with M_f[k] = 0 */
} gj_cancel_frame;
int gj_cancel_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b, size_t nbytes_b,
                  size_t first_b, size_t n_samples, int nfft, const float* d_weights /* [n_sets][nfft][2] */,
                  size_t frames_per_set, size_t n_sets, const float* d_threshold /* [nfft] */,
                  uint8_t* d_out /* [2*n_samples] */, gj_cancel_frame* d_frames /* [F] or NULL */);

/* ------------------------------------------------- three-antenna per-bin canceller -- */
/* The multiple sidelobe canceller of a receiver with three antennas: gj_cancel_dev with two auxiliaries, two complex
 * weights per bin and so two nulls per bin.  Two Gaussian jammers from different directions in one band, of which a
 * single auxiliary can null only one, are removed together.  The MMSE weights solve, per bin, the 2 x 2 system
 *   W1 Sbb + W2 Sbc = conj(Sab),   W1 conj(Sbc) + W2 Scc = conj(Sac)
 * on gj_csd_dev's sums of the pairs (a,b), (a,c) and (b,c) (gpsjam/coherence.py, cancel_weights2).  Everything is
 * gj_cancel_dev's -- F, h, w, x, scale, set(f), the mask, the inverse transform, the overlap-add, the copied edges, the
 * record gj_cancel_frame with total_in capture a's power -- except:
 *
 *   C_f[k]  = sum_n w[n] x_c[first_c + f*h + n] exp(-2 pi i k n / N)      from capture c, as B_f from capture b
 *   Y_f[k]  = (A_f[k] - W1[set(f)][k] * B_f[k]) - W2[set(f)][k] * C_f[k]  every product of W1 * B and W2 * C rounded on
 *                                                                         its own, the two subtractions in this order
 *
 * d_weights: DEVICE float32[n_sets][2][nfft][2]: set s holds W1[s][k] at d_weights + s*4*nfft and W2[s][k] 2*nfft floats
 * further, both (re, im) in FFT order; 8-byte aligned; the host never reads it.
 * Bit-exact anchors: with every W2 = 0 the call writes the bytes and records of gj_cancel_dev(a, b, W1), whatever c
 * holds; with every W1 = 0 those of gj_cancel_dev(a, c, W2), whatever b holds; with both 0 those of gj_excise_dev on
 * capture a (total_in == total).
 * Output: d_out[2*n_samples], range-relative; the first half frame and everything from F*h on are copied from capture a.
 * The call writes exactly 2*n_samples bytes.  d_frames (optional) receives one record per frame.  first_a, first_b and
 * first_c may be odd and may all differ; d_a == d_b == d_c is allowed.
 * Refusals: those of gj_cancel_dev, applied to all three captures (nfft, n_samples < nfft, a range past any capture, a null
 * or odd d_a, d_b or d_c, a null d_out or d_threshold, a d_threshold or d_frames that is not 4-byte aligned, d_out
 * overlapping any of the three captures, frames_per_set == 0 or n_sets == 0, a null d_weights or one that is not 8-byte
 * aligned; GJ_ERR_INVALID but for nfft: GJ_ERR_UNSUPPORTED).  A refused call enqueues nothing.  Needs no workspace;
 * enqueues on the context's stream (two launches: the transform kernel and the edge copy) and returns.
 * Determinism: an output sample depends only on the bytes of the two frame triples that cover it and on their weight
 * sets, and every sum runs in an order fixed by nfft.  So a call started k*h samples later in all three captures, with the
 * sets shifted alike, reproduces the overlapping interior bytes and the records of the shared frames bit for bit; two
 * identical calls give identical bytes; and d_frames == NULL changes no byte.
 * Limits: two auxiliaries give two nulls per bin -- a signal whose steering vector lies near the plane of the two
 * jammers' is attenuated with them -- and capture a's receiver noise rises by up to 1 + |W1|^2 + |W2|^2.  The three
 * captures must share a clock and be aligned to well under nfft samples, as for gj_csd_dev. */
int gj_cancel2_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b, size_t nbytes_b,
                   size_t first_b, const uint8_t* d_c, size_t nbytes_c, size_t first_c, size_t n_samples, int nfft,
                   const float* d_weights /* [n_sets][2][nfft][2] */, size_t frames_per_set, size_t n_sets,
                   const float* d_threshold /* [nfft] */, uint8_t* d_out /* [2*n_samples] */,
                   gj_cancel_frame* d_frames /* [F] or NULL */);

/* ------------------------------------------------- time-domain pulse blanking ------- */
/* The pulse blanker a receiver puts in front of its FFT excisor: a cleaned capture, uint8 I/Q again, with every sample
 * near a window of excess power put to mid-level (simulate/frontend/jammers/pulsedJammer.py and every sweep that crosses
 * the band in a few samples; gpsjam/mitigate.py builds the threshold).  A pulse shorter than a frame is spread over every
 * bin of that frame: gj_excise_dev either wipes the frame or lets the pulse through.  For a range of n_samples I/Q
 * pairs, t = 0 .. n_samples-1 relative to the range (sample t of the range is sample first_sample + t of the capture),
 * with W = window, G = guard and o2 = 2*offset of gj_set_unpack (an integer):
 *
 *   e[t] = (2 I_t - o2)^2 + (2 Q_t - o2)^2            4 |x|^2 in LSB^2, an exact integer; 0 outside the range, even
 *                                                     where the capture has bytes there
 *   S[t] = sum of e[u], u = t - W/2 .. t - W/2 + W - 1     W/2 rounded down
 *   T    = floor(4 W threshold)                       in double, from the float32 threshold
 *   D[t] = S[t] > T                                   strict
 *   B[t] = OR of D[u] over |u - t| <= G, u inside the range
 *
 * threshold is a mean power per sample in LSB^2, the unit of gj_onset.noise_power.  +inf, or any T of 2^63 or more,
 * never blanks.  A result depends on the bytes of its range alone.
 * Output: d_out[2*n_samples] is range-relative, byte 0 is I of first_sample.  Where B[t] is false: the two input bytes,
 * unchanged.  Where B[t] is true and o2 is even: both bytes are o2/2.  Where B[t] is true and o2 is odd the mid-level is
 * not a byte and the two nearest bytes alternate on the ABSOLUTE sample index:
 *   I = (o2-1)/2 + ((first_sample + t) & 1),   Q = (o2-1)/2 + ((first_sample + t + 1) & 1)
 * so that a blanked stretch has mean `offset` exactly and the residue sits at +-fs/2.  The call writes exactly
 * 2*n_samples bytes; length and byte coordinates are the range's, as in gj_excise_dev.
 * d_blocks (optional, may be NULL) receives one record per GJ_BLANK_BLOCK samples of the range, the last one ragged.
 * Limits: 1 <= window <= 1024 and 0 <= guard <= 1024 (GJ_ERR_UNSUPPORTED otherwise), so that a window sum stays under
 * 2^30.  GJ_ERR_INVALID: n_samples == 0, a range that runs past the capture, a null or odd d_iq, a null d_out, a d_blocks
 * that is not 8-byte aligned, a NaN or negative threshold, d_out[0, 2*n_samples) overlapping d_iq[0, nbytes) (windows
 * read their neighbours: in place is wrong).  first_sample may be odd.  A refused call enqueues nothing.  Needs no
 * workspace; one launch on the context's stream, then the call returns.
 * Determinism: everything is integer arithmetic.  Two identical calls give identical bytes; a call on a sub-range
 * reproduces the bytes of the larger call wherever t is at least W/2 + G from the sub-range's start and at least W + G
 * from its end; and bytes and records equal those of the definition evaluated on the CPU, every one of them. */
#define GJ_BLANK_BLOCK 4096        /* samples per record */
typedef struct gj_blank_block {    /* 24 bytes, all exact integers */
    uint64_t total;     /* sum of e[t] over the block's samples */
    uint64_t removed;   /* sum of e[t] over its blanked samples */
    int32_t n_blanked;  /* blanked samples in the block */
    int32_t n_rising;   /* t in the block with B[t] and (t == 0 or !B[t-1]) */
} gj_blank_block;
/* records of the blanker: ceil(n_samples / GJ_BLANK_BLOCK); pure host arithmetic, no context */
size_t gj_blank_blocks(size_t n_samples);
int gj_blank_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int window,
                 int guard, float threshold, uint8_t* d_out /* [2*n_samples] */,
                 gj_blank_block* d_blocks /* [gj_blank_blocks(n_samples)] or NULL */);

/* raw-byte histogram of every `stride`-th byte (widmo_plot.py:35,85: stride 100,
 * 256 bins).  Strided per chunk exactly like raw_chunk[::100]. */
int gj_byte_histogram_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t chunk_samples,
                          int nperseg, int stride, uint64_t* d_hist /* [256] */);

/* ------------------------------------------------- K3: amplitude statistics --------- */
/* Replaces read_iq_data + np.abs + find_change_point + np.mean(amp[idx:])
 * (skrypty/triangulateRSSI.py:29-31,37-40,65-68): amp = |((I-127.5) + j(Q-127.5))/127.5|,
 * first index with amp > threshold, mean of amp from that index to the end. */
typedef struct gj_amp_stats {
    int64_t first_index; /* -1: nothing above the threshold (or empty input) */
    uint64_t count;      /* samples from first_index to the end */
    double sum;          /* sum of amp over those samples */
    float mean;          /* (float)(sum / count) -- the reference's avg_amplitude */
    float reserved;
} gj_amp_stats;
int gj_amp_stats_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, float threshold,
                     gj_amp_stats* d_out);
int gj_amp_stats_u8(gj_ctx* ctx, const uint8_t* iq, size_t nbytes, float threshold,
                    gj_amp_stats* out, float* kernel_ms);

/* ------------------------------------------------- K4: interference onset ----------- */
/* Replaces find_interference_start (skrypty/triangulateTDOA.py:37-49) on
 * z = (I-127.5) + j(Q-127.5): noise = mean |z|^2 over the first noise_samples
 * (1e-9 if 0), moving average of |z|^2 over `window` samples ('valid'), first index
 * above noise*factor, + window/2; -1 when none or the stream is shorter than
 * noise_samples + window.  Window sums are exact integers. window <= 8192. */
typedef struct gj_onset {
    int64_t start_index; /* -1 = not found */
    float noise_power;
    float threshold;
    /* Decision margins, relative to the threshold.  The window sums here are exact integers and
     * the noise mean is rounded once; the reference sums float32 |z|^2 (pairwise for the noise
     * mean, float64 inside np.convolve), so its threshold and moving averages differ from these in
     * the last ulps (~1e-7 relative).  See guard_index below for the exact statement of when the
     * index is the reference's by construction. */
    float margin_hit;    /* (moving average at the crossing - threshold) / threshold; 0 if not found */
    float margin_before; /* (threshold - largest moving average in front of the crossing) / threshold;
                          * positions the screening pass proved quiet enter with their upper bound, so
                          * this can under-state the true gap, never over-state it.  Not found: over the
                          * whole capture. */
    /* First index (+ window/2, like start_index) whose moving average exceeds threshold * (1 - 1e-6),
     * -1 if none.  In front of it every moving average is below the reference's threshold whatever
     * the reference's float32 rounding did, so the reference's own first crossing cannot lie before
     * it.  guard_index == start_index and margin_hit >= 1e-6: the index is the reference's by
     * construction.  Otherwise only the positions from guard_index on need the reference's
     * arithmetic (skrypty/triangulateTDOA.py evaluates it there, on the host). */
    int64_t guard_index;
} gj_onset;
int gj_onset_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, int noise_samples, int window,
                 float factor, gj_onset* d_out);
int gj_onset_u8(gj_ctx* ctx, const uint8_t* iq, size_t nbytes, int noise_samples, int window,
                float factor, gj_onset* out, float* kernel_ms);

/* ------------------------------------------------- fused stream scan ---------------- */
/* K1 + K3 + K4 in ONE pass over the capture (the three are pure streaming reductions over
 * the same bytes): identical results to gj_chunk_power_dev, gj_amp_stats_dev and gj_onset_dev
 * called one after the other.  The single pass is used when chunk_bytes is a multiple of
 * 65536 and the capture is 16-byte aligned; otherwise K1 runs alone and the pass delivers K3 + K4.
 * gj_amp_stats_dev and gj_onset_dev are themselves this pass (with the outputs nobody asked for
 * dropped): neither depends on the chunk size, so a capture gives the same K3 / K4 bits through
 * every entry point.  A capture that is not 16-byte aligned is first copied into the workspace
 * (one device-to-device copy; any alignment is accepted). */
int gj_stream_scan_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes,
                       size_t chunk_bytes, float eps, int flags, float* d_power,
                       float rssi_threshold, gj_amp_stats* d_amp,
                       int noise_samples, int window, float factor, gj_onset* d_onset);

/* The whole per-capture side chain in TWO launches: the fused pass above, then one "tail" launch whose workgroups take
 * roles -- noise-floor threshold of the power map (gj_power_threshold_dev: worker.py:241-248), amplitude totals
 * (triangulateRSSI.py:65-68), K4's screening + exact scan + record (triangulateTDOA.py:37-49) and the TDOA slot cut at that
 * onset (gj_tdoa_slot_dev with d_start = &d_onset->start_index) -- where gj_stream_scan_dev + gj_power_threshold_dev +
 * gj_tdoa_slot_dev were eight dependent launches.  At the reference's capture sizes (10 s = 41 MB) that chain, not the
 * bytes, was the step time.  Every result is the same bits as from the separate calls, except gj_onset.margin_before,
 * which is a bound (see gj_onset) and is now a function of the capture alone.  `extra` may be NULL (then this IS
 * gj_stream_scan_dev); a NULL d_stats / d_slot leaves that role out. */
typedef struct gj_scan_extra {
    float pct, rise_db;   /* noise floor: numpy.percentile(power, pct) * 10^(rise_db/10) */
    float* d_stats;       /* [3] {baseline, threshold, count_above} or NULL */
    uint8_t* d_mask;      /* [n_chunks] or NULL */
    size_t slice_samples; /* TDOA slot of slice_samples I/Q pairs ... */
    uint8_t* d_slot;      /* ... written here (gj_tdoa_slot_bytes, 16-byte aligned) or NULL */
} gj_scan_extra;
int gj_capture_scan_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t chunk_bytes, float eps, int flags,
                        float* d_power, float rssi_threshold, gj_amp_stats* d_amp, int noise_samples, int window,
                        float factor, gj_onset* d_onset, const gj_scan_extra* extra);

/* ------------------------------------------------- overlapped ingest ----------------- */
/* Overlapped ingest: upload a capture AND analyse it, with the kernels running on the pieces (1-16 MiB, by capture size) that have
 * landed in HBM while the rest is still on its way (the reference reads, then computes: worker.py:209-230,
 * triangulateRSSI.py:29-31, widmo_plot.py:26-54).  What is computed: with chunk_bytes != 0 the fused scan (K1 power
 * map, K3 amplitude statistics, K4 onset -- gj_stream_scan_dev), with nperseg != 0 the Welch waterfall (K2 --
 * gj_welch_dev).  Results are bit-identical to gj_upload* followed by those calls.  The capture stays resident:
 * *dptr is a device pointer like gj_upload's (free with gj_free), usable with every "*_dev" and "*_u8" entry point. */
typedef struct gj_ingest_plan {
    size_t chunk_bytes; /* K1 power chunks; 0: no scan (K3 and K4 are skipped too) */
    float eps;
    int power_flags; /* GJ_CP_* */
    float rssi_threshold; /* K3 */
    int noise_samples, window; /* K4 */
    float factor;
    size_t chunk_samples; /* K2 */
    int nperseg; /* 0: no PSD */
    int welch_flags; /* GJ_WELCH_* */
    double fs;
} gj_ingest_plan;
typedef struct gj_ingest_result {
    size_t nbytes, n_chunks, rows;
    gj_amp_stats amp;
    gj_onset onset;
    float upload_ms; /* wall clock until the last piece had been queued and its bounce buffer released */
    float total_ms;  /* wall clock of the whole call: results on the host */
} gj_ingest_result;
int gj_ingest_u8(gj_ctx* ctx, const uint8_t* host, size_t nbytes, const gj_ingest_plan* plan, float* power,
                 size_t power_cap, float* psd, float* psd_db, size_t psd_cap_floats, gj_ingest_result* result,
                 void** dptr);
int gj_ingest_file(gj_ctx* ctx, const char* path, size_t offset, size_t max_bytes, const gj_ingest_plan* plan,
                   float* power, size_t power_cap, float* psd, float* psd_db, size_t psd_cap_floats,
                   gj_ingest_result* result, void** dptr);

/* The recordings of a deployment brought in together: gj_ingest_file for every job, side by side (one host thread of the
 * library's own and one lane per file; the fill threads per file are lowered for the duration unless gj_set_fill_threads
 * fixed them).  The reference reads them one after the other (skrypty/triangulateRSSI.py:160-174, worker.py:586-600).
 * Every job gets its own status, result and device pointer (free each with gj_free); the return value is the first
 * non-zero status, with that file's message in gj_last_error.  Results are those of gj_ingest_file per file. */
typedef struct gj_ingest_job {
    const char* path;
    size_t offset, max_bytes; /* as gj_ingest_file */
    float* power;
    size_t power_cap;
    float* psd;
    float* psd_db; /* or NULL */
    size_t psd_cap_floats;
    gj_ingest_result result; /* out */
    void* dptr;              /* out */
    int status;              /* out */
} gj_ingest_job;
int gj_ingest_files(gj_ctx* ctx, gj_ingest_job* jobs, int n_jobs, const gj_ingest_plan* plan);

/* ------------------------------------------------- K5: TDOA cross-correlation ------- */
/* Replaces signal.correlate(sig1, sig0, 'full') + argmax|.| - (N-1)
 * (skrypty/triangulateTDOA.py:80-89) for every requested antenna pair.
 * d_iq[a] is antenna a's capture in HBM, nbytes[a] its length; the slice of antenna a is
 * the n_samples I/Q pairs starting at d_starts[a] (DEVICE array, e.g. written by
 * gj_onset_dev; a negative or out-of-range start marks the antenna invalid).
 * pairs = {i0,j0,i1,j1,...}: lag of antenna j relative to antenna i
 * (= correlate(slice_j, slice_i)), positive when j is delayed.  FFT length is the next
 * power of two >= 2*n_samples-1 (four-step, in HBM/L2).  Outputs (device):
 * lags[p] (INT32_MIN if an antenna of the pair is invalid), peaks[p] = max |c|. */
#define GJ_MAX_ANTENNAS 16
#define GJ_LAG_INVALID INT32_MIN
/* margins[p] (optional, may be NULL) = 1 - |c|_runner-up / |c|_peak, the relative gap between the
 * peak and the largest |c| at any other lag: the arg-max is taken over values that carry the
 * rounding of a complex64 FFT (~1e-6 of the peak, here as in scipy), so a margin of that order
 * means the reference's own choice between the two lags is decided by its rounding. */
int gj_xcorr_lags_dev(gj_ctx* ctx, const uint8_t* const* d_iq, const size_t* nbytes, int n_ant,
                      const int64_t* d_starts, size_t n_samples, const int32_t* pairs,
                      int n_pairs, int32_t* d_lags, float* d_peaks, float* d_margins);
int gj_xcorr_lags_u8(gj_ctx* ctx, const uint8_t* const* slices, int n_ant, size_t n_samples,
                     const int32_t* pairs, int n_pairs, int32_t* lags, float* peaks, float* margins,
                     float* kernel_ms);
size_t gj_xcorr_workspace(gj_ctx* ctx, int n_ant, size_t n_samples, int n_pairs);

/* TDOA slot = what one capture contributes to a multi-antenna solve, as ONE message:
 *   [int64 flag: 0 valid / -1 invalid][int64 start sample][2*n_samples bytes of I/Q], padded to a
 * multiple of 256 bytes (gj_tdoa_slot_bytes).  gj_tdoa_slot_dev cuts the n_samples I/Q pairs that
 * start at *d_start (DEVICE scalar, e.g. &gj_onset.start_index) out of a capture; an un-found
 * onset or a slice that runs off the end marks the slot invalid (the reference aborts there,
 * skrypty/triangulateTDOA.py:67-77).  gj_xcorr_slots_dev solves pairs over an array of n_ant
 * slots (slot a at d_slots + a*slot_stride), e.g. the receive buffer of gj_comm_allgather_dev:
 * pairs (i, j) of skrypty/triangulateTDOA.py:80-89 generalised to n_ant antennas.  Only the
 * slots the pairs name are transformed (at most GJ_MAX_ANTENNAS per call), so the pairs of a
 * many-antenna solve can be dealt over the ranks (gpsjam/sharded.py pairs_of_rank). */
#define GJ_SLOT_HEADER 16
size_t gj_tdoa_slot_bytes(size_t n_samples);
int gj_tdoa_slot_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, const int64_t* d_start,
                     size_t n_samples, uint8_t* d_slot);
int gj_xcorr_slots_dev(gj_ctx* ctx, const uint8_t* d_slots, size_t slot_stride, int n_ant,
                       size_t n_samples, const int32_t* pairs, int n_pairs, int32_t* d_lags,
                       float* d_peaks, float* d_margins);

/* ------------------------------------------------- cross-ambiguity search ------------ */
/* K5 for receivers that do NOT share a clock (one oscillator per dongle): the lag is searched together
 * with the frequency offset between the two receivers.  For a slice length n, L = gj_xcorr_fft_len(n) is
 * K5's FFT length (the power of two >= 2n-1, at least 65536) and one BIN is fs / L Hz.  For a pair (i, j)
 * and an integer bin b
 *     x_j^(b)[t] = x_j[t] * exp(-2 pi i b t / L),  t = 0 .. n-1 from the start of the slice
 *     c_b        = correlate(x_j^(b), x_i, 'full')      (skrypty/triangulateTDOA.py:86)
 * and the pair's result is the (b, m) with the largest |c_b[m]| over b = bin_first .. bin_first+n_bins-1,
 * lag = m - (n-1) as in K5.  Positive b: receiver j sees the source b*fs/L Hz higher than receiver i.
 * Ties: the larger value, then the earlier bin of the range, then the smaller m (numpy's first maximum
 * inside a bin, as K5).  x is K5's unpacking, (I - offset) + j(Q - offset), un-normalised.
 * The slice is zero-padded to L, so the rotation is an exact shift of the spectrum; every antenna is
 * transformed once per call and only product, inverse transform and arg-max repeat per (pair, bin).
 * With n_bins = 1, bin_first = 0 lag, peak and margin_lag equal gj_xcorr_lags_dev's bit for bit.
 *
 * Arguments as gj_xcorr_lags_dev / gj_xcorr_slots_dev / gj_xcorr_lags_u8.  n_bins >= 1 and every |b| < L/2,
 * else GJ_ERR_INVALID; more than GJ_CAF_MAX_BINS bins in one call: GJ_ERR_UNSUPPORTED.  Bins run in batches
 * of bins_per_launch (0 = a default sized to keep a batch's intermediate buffers in the Infinity Cache; a
 * request is clipped to what the arrival counters hold, 688 / n_pairs); the results do not depend on it.
 * d_bin_lags / d_bin_peaks (optional, [n_pairs][n_bins]) receive the best lag and its |c| of EVERY bin:
 * the ridge of the surface.  The *_dev calls enqueue and return; they allocate nothing when
 * gj_xcorr_caf_workspace bytes were reserved (gj_reserve), and a refused call enqueues nothing. */
#define GJ_CAF_MAX_BINS 4096
typedef struct gj_caf_result {
    int32_t lag;        /* GJ_LAG_INVALID if an antenna of the pair is invalid */
    int32_t bin;        /* the winning bin b */
    float peak;         /* max |c| over the searched surface */
    float margin_lag;   /* 1 - runner-up/peak among the OTHER lags of the winning bin (K5's margin) */
    float margin_bin;   /* 1 - (largest per-bin peak of any OTHER bin)/peak; 1 when n_bins == 1 */
    float reserved;
} gj_caf_result;
size_t gj_xcorr_fft_len(size_t n_samples); /* L; pure host arithmetic, no context (0 for n_samples 0) */
int gj_xcorr_caf_dev(gj_ctx* ctx, const uint8_t* const* d_iq, const size_t* nbytes, int n_ant,
                     const int64_t* d_starts, size_t n_samples, const int32_t* pairs, int n_pairs,
                     int bin_first, int n_bins, int bins_per_launch, gj_caf_result* d_out,
                     int32_t* d_bin_lags, float* d_bin_peaks);
int gj_xcorr_caf_slots_dev(gj_ctx* ctx, const uint8_t* d_slots, size_t slot_stride, int n_ant,
                           size_t n_samples, const int32_t* pairs, int n_pairs, int bin_first, int n_bins,
                           int bins_per_launch, gj_caf_result* d_out, int32_t* d_bin_lags,
                           float* d_bin_peaks);
int gj_xcorr_caf_u8(gj_ctx* ctx, const uint8_t* const* slices, int n_ant, size_t n_samples,
                    const int32_t* pairs, int n_pairs, int bin_first, int n_bins, gj_caf_result* out,
                    int32_t* bin_lags, float* bin_peaks, float* kernel_ms);
size_t gj_xcorr_caf_workspace(gj_ctx* ctx, int n_ant, size_t n_samples, int n_pairs, int n_bins,
                              int bins_per_launch);

/* ------------------------------------------------- fine TDOA: exact lag-window correlation ---- */
/* The correlation of two captures' ranges at the 2R + 1 lags around an integer lag (K5's answer), as a direct
 * time-domain sum over ANY number of samples, up to a whole capture: what a sub-sample delay estimate is made from
 * (gpsjam/tdoa.py does the float part, 65 complex numbers, on the host).  With R = half_width, n = n_samples,
 * o2 = 2*offset of gj_set_unpack (an integer) and u = 2*byte - o2 for I and Q:
 *
 *   xa[t] = sample first_a + t of capture a,  xb[t] = sample first_b + t of capture b,   t = 0 .. n-1;
 *           both are ZERO outside 0 .. n-1, even where the capture has bytes there
 *   for k = lag_center - R .. lag_center + R, in that order in the output:
 *   C4[k].re = sum_t  uI_b[t+k] uI_a[t] + uQ_b[t+k] uQ_a[t]
 *   C4[k].im = sum_t  uQ_b[t+k] uI_a[t] - uI_b[t+k] uQ_a[t]          t = 0 .. n-1,  0 <= t+k < n
 *
 * C4[k] = 4 * correlate(x_b, x_a, 'full')[k + n - 1] in K5's unpacking x = (I - offset) + j(Q - offset)
 * (skrypty/triangulateTDOA.py:86), K5's sign convention: the peak sits at a positive k when b is delayed.  Every value
 * is an exact integer.
 * d_total: int64[2R+1][2] (re, im).  d_blocks (optional, may be NULL): int32[gj_fine_blocks(n)][2R+1][2]; record m is
 * the same sum over t in [m*GJ_FINE_BLOCK, (m+1)*GJ_FINE_BLOCK) alone, the last block ragged.  A block sum is at most
 * 4096 * 2 * 510^2 = 2 130 739 200 < 2^31 in magnitude (offsets 0 and 255), so it fits; d_total is the sum of the block
 * records in 64 bits.  d_blocks = NULL changes no bit of d_total.
 * Determinism: integer addition, so the result does not depend on tiling or order; two calls give identical bits, and
 * the result depends on the bytes of the two ranges alone.
 * Allowed: d_a == d_b and overlapping ranges (the inputs are only read); odd first_a / first_b; a lag_center with no
 * overlap (|k| >= n gives zeros); n shorter than R.
 * GJ_ERR_INVALID: n_samples == 0, a range that runs past its capture, a null or odd d_a or d_b, a null d_total, a
 * d_total that is not 8-byte aligned, a d_blocks that is not 4-byte aligned, |lag_center| + R overflowing int32.
 * GJ_ERR_UNSUPPORTED: half_width outside 0 .. GJ_FINE_MAX_HALF.  A refused call enqueues nothing.
 * Enqueues on the context's stream (a memset of d_total and one launch, whose workgroups add their 64-bit sums to
 * d_total with atomic adds) and returns.  Needs no workspace: 0 bytes to gj_reserve, the call never allocates. */
#define GJ_FINE_BLOCK 4096          /* samples of a per block record */
#define GJ_FINE_MAX_HALF 32         /* half_width R: 0..32, 2R+1 <= 65 lags */
/* block records over n_samples: ceil(n_samples / GJ_FINE_BLOCK); pure host arithmetic, no context */
size_t gj_fine_blocks(size_t n_samples);
int gj_xcorr_fine_dev(gj_ctx* ctx, const uint8_t* d_a, size_t nbytes_a, size_t first_a, const uint8_t* d_b,
                      size_t nbytes_b, size_t first_b, size_t n_samples, int32_t lag_center, int half_width,
                      int64_t* d_total /* [2R+1][2]  re, im */,
                      int32_t* d_blocks /* [gj_fine_blocks(n_samples)][2R+1][2] or NULL */);

/* ------------------------------------------------- correlator bank: post-correlation I/Q ---- */
/* The reference's second hot loop (correlator, sdrcmn.c:707-740: mixcarr -> rescode -> dot_23 / dot_22) as a batch:
 * with code phase and Doppler known from the acquisition and the code rate tied to the Doppler, every block of every
 * channel is independent, so a whole capture is correlated in one launch, open loop.  Integer arithmetic from the byte
 * to the sum: gpsjam/postcorr.py makes Doppler, C/N0 and carrier phase of the prompt series on the host.
 *
 * For sample t = 0 .. n_samples-1 of the range (sample first_sample + t of the capture), I, Q = byte - 128 (the
 * acquisition's fixed unpacking, sdrrcv.c:104-106, WHATEVER gj_set_unpack says), and for channel ch:
 *
 *   carrier   theta = (carr_phase + t*carr_step) mod 2^32,   i = theta >> 28
 *             wI = C[i]*I - S[i]*Q,   wQ = S[i]*I + C[i]*Q,   S[i] = C[(i - 4) & 15]
 *             C = GJ_CORR_COS_TABLE: floor(cos(2 pi i / 16) * 32 + 0.5), the reference's SSE2 table (sdrcmn.c:629-630)
 *   code      for tap j, d = tap_offsets[j]:
 *             chip = floor((code_phase + (t + d)*code_step) / 2^32) mod 1023
 *             exact integers, mathematical floor and mod: a negative t + d is well defined
 *             c = d_codes[code_row][chip]; taps are whole-sample shifts of the resampled code (the reference's
 *             code +- s[i] pointers).  The chips are +-1: a value < 0 counts as -1, every other value as +1
 *   record    (ch, block m, tap j) = (sum wI*c, sum wQ*c) over t in [m*B, (m+1)*B), B = block_samples; last block ragged
 *
 * d_out: int32[n_channels][gj_corr_blocks(n_samples, B)][n_taps][2] (I, Q).  |w| <= 128*46 = 5888 (|C[i]| + |S[i]| <= 46),
 * so a record is at most 4096 * 5888 = 24 117 248 < 2.5e7 in magnitude: int32 never wraps.  Every value is an exact
 * integer: the result does not depend on tiling or order, two calls give identical bits, and it depends on the bytes
 * of the range alone.  A capture that holds code * exp(-2j pi f t) peaks at carr_step = +f / fs * 2^32.
 * Limits (GJ_ERR_UNSUPPORTED): block_samples a multiple of 16 in 16 .. GJ_CORR_MAX_BLOCK; n_taps 1 .. GJ_CORR_MAX_TAPS
 * (the reference's 1 + 2 corrn); |tap_offsets[j]| <= GJ_CORR_MAX_TAP_OFFSET; n_channels 1 .. GJ_CORR_MAX_CHANNELS;
 * n_samples 1 .. GJ_CORR_MAX_SAMPLES (t*code_step < 2^62).
 * GJ_ERR_INVALID: a null ctx, d_iq, d_codes, d_channels, tap_offsets or d_out; an odd d_iq or d_codes, a d_channels
 * that is not 8-byte aligned, a d_out that is not 4-byte aligned; n_code_rows < 1; a range that runs past the capture.
 * A refused call enqueues nothing.
 * The channel fields are in DEVICE memory, so the entry point cannot answer for them with a status.  They are checked
 * twice: Device.corr_bank (gpsjam/__init__.py) checks them on the host before it uploads them and raises
 * GJ_ERR_INVALID; and every workgroup of the kernel checks all of them before it reads a chip: if ANY channel has
 * reserved != 0, a code_row outside 0 .. n_code_rows-1, code_phase >= 1023 * 2^32 or code_step >= GJ_CORR_MAX_CODE_STEP,
 * the launch writes NOTHING (d_out is left as it was) and never reads outside d_codes.
 * One launch on the context's stream; no workspace, no memset, no atomics: 0 bytes to gj_reserve, the call never
 * allocates.  Each record is written by exactly one workgroup.  tap_offsets is a HOST array, read before the call returns. */
typedef struct gj_corr_channel {      /* 32 bytes */
    uint64_t code_phase;   /* Q32.32 chips at sample first_sample; < 1023 * 2^32 */
    uint64_t code_step;    /* Q32.32 chips per sample; < GJ_CORR_MAX_CODE_STEP */
    uint32_t carr_phase;   /* cycles * 2^32 at sample first_sample */
    uint32_t carr_step;    /* cycles * 2^32 per sample, modulo 2^32 (negative Doppler = two's complement) */
    int32_t code_row;      /* row of d_codes */
    int32_t reserved;      /* must be 0 */
} gj_corr_channel;
#define GJ_CORR_MAX_BLOCK 4096                  /* block_samples: a multiple of 16 in 16 .. 4096 */
#define GJ_CORR_MAX_TAPS 9
#define GJ_CORR_MAX_TAP_OFFSET 64
#define GJ_CORR_MAX_CHANNELS 64
#define GJ_CORR_MAX_SAMPLES (1ull << 28)
#define GJ_CORR_MAX_CODE_STEP (1ull << 34)      /* 4 chips per sample */
#define GJ_CORR_CODE_LEN 1023
#define GJ_CORR_COS_TABLE {32, 30, 23, 12, 0, -12, -23, -30, -32, -30, -23, -12, 0, 12, 23, 30}
/* block records over n_samples: ceil(n_samples / block_samples), 0 for block_samples < 1; pure host arithmetic */
size_t gj_corr_blocks(size_t n_samples, int block_samples);
int gj_corr_bank_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples,
                     int block_samples, const int16_t* d_codes /* [n_code_rows][1023], +-1 */, int n_code_rows,
                     const gj_corr_channel* d_channels, int n_channels,
                     const int32_t* tap_offsets /* HOST array [n_taps], samples */, int n_taps,
                     int32_t* d_out /* [n_channels][gj_corr_blocks][n_taps][2]  I, Q */);

/* ------------------------------------------------- counterfeit-signal subtraction ---- */
/* The correlator run backwards: the replicas of up to 64 channels, each with one complex amplitude per block, rebuilt
 * and subtracted from the capture: a cleaned capture, uint8 I/Q again (successive interference cancellation, open
 * loop).  The terms are the correlator bank's: gj_corr_channel, C = GJ_CORR_COS_TABLE with S[i] = C[(i - 4) & 15], the
 * chip rule at tap 0 (d = 0), I, Q = byte - 128 WHATEVER gj_set_unpack says, gj_corr_blocks.  gpsjam/postcorr.py
 * (amplitudes) makes the amplitudes from the bank's prompts; gpsjam/spoof.py (remove) joins the pieces.
 *
 * For sample t = 0 .. n_samples-1 of the range and block m = t / B, B = block_samples:
 *
 *   a(ch, m)  = clamp(d_amp[ch][m][0..1], -GJ_SUB_MAX_AMP, +GJ_SUB_MAX_AMP)        int32 pairs (aI, aQ)
 *   c, i      = the bank's chip (+-1) at tap 0 and its carrier index theta >> 28 of channel ch at sample t
 *   R_I       = sum over ch of c * (aI*C[i] + aQ*S[i])
 *   R_Q       = sum over ch of c * (aQ*C[i] - aI*S[i])         the replica a * c * (C - jS), scaled by 2^GJ_SUB_FRAC
 *   d         = 32768 without GJ_SUB_DITHER; with it, per component (comp = 0 for I, 1 for Q):
 *               k = 2*(first_sample + t) + comp  (uint64),   key = (uint32)k ^ ((uint32)(k >> 32) * 0x9e3779b9) ^ seed
 *               h: v ^= v>>16; v *= 0x7feb352d; v ^= v>>15; v *= 0x846ca68b; v ^= v>>16  (uint32),   d = h(key) >> 16
 *   q         = floor((R + d) / 65536)       mathematical floor: R may be negative
 *   out byte  = clamp(in byte - q, 0, 255)
 *
 * |R| <= 64 * 2^19 * 46 = 1 543 503 872 and d < 65536: R + d stays inside int32, every value is an exact integer, and the
 * bytes do not depend on tiling or order.  The bank's mixer turns the replica back: a sample that holds R / 2^16 alone
 * adds a (C[i]^2 + S[i]^2) / 2^16 to the channel's prompt, 1042.5 a / 2^16 in the mean over the table, so the amplitude
 * that takes a signal out is its own prompt sum over samples * 1042.5, times 2^16 (gpsjam.postcorr.amplitudes).
 * The dither.  A 40 dB-Hz signal is about one LSB and each of its components less than half of one: rounding to
 * nearest (d = 32768) then subtracts nothing at all.  With d uniform over 0 .. 65535 the expectation of q is R / 65536
 * exactly.  d is a function of the ABSOLUTE sample index (as the blanker's odd mid-level is), the component and the
 * seed: a call on a sub-range that starts at a block boundary m0*B, with the channels advanced by m0*B samples and
 * d_amp offset by m0 blocks, writes the bytes the larger call writes there.
 *
 * d_amp: int32[n_channels][gj_corr_blocks(n_samples, B)][2].  Amplitudes are not checked: the clamp is part of the
 * definition, so INT32_MIN is as good as -GJ_SUB_MAX_AMP.  d_out: 2*n_samples bytes, any alignment (two 16-byte stores per 16
 * samples where it is 16-byte aligned).  d_blocks (optional, may be NULL; the bytes are the same) receives one record per
 * GJ_SUB_BLOCK samples of the range, the last one ragged, whatever B is.
 *
 * Limits (GJ_ERR_UNSUPPORTED): block_samples a multiple of 16 in 16 .. GJ_CORR_MAX_BLOCK; n_channels
 * 1 .. GJ_CORR_MAX_CHANNELS; n_samples 1 .. GJ_CORR_MAX_SAMPLES (t*code_step < 2^62).
 * GJ_ERR_INVALID: a null ctx, d_iq, d_codes, d_channels, d_amp or d_out; an odd d_iq or d_codes, a d_channels
 * that is not 8-byte aligned, a d_amp that is not 4-byte aligned, a d_blocks that is not 8-byte aligned; n_code_rows < 1;
 * a flag bit other than GJ_SUB_DITHER; a range that runs past the capture; a d_out whose 2*n_samples bytes overlap
 * d_iq[0, nbytes) anywhere (in place included).  A refused call enqueues nothing.
 * The channel fields are in DEVICE memory, as the bank's: Device.subtract (gpsjam/__init__.py) checks them on the host
 * before it uploads them and raises GJ_ERR_INVALID; and every workgroup of the kernel checks all of them before it reads
 * a chip: if ANY channel has reserved != 0, a code_row outside 0 .. n_code_rows-1, code_phase >= 1023 * 2^32 or
 * code_step >= GJ_CORR_MAX_CODE_STEP, the launch writes NOTHING, neither a byte nor a record.
 * One launch on the context's stream; no workspace, no memset, no atomics: 0 bytes to gj_reserve, the call never
 * allocates.  Every byte and every record is written by exactly one workgroup. */
#define GJ_SUB_BLOCK 4096          /* samples per record */
#define GJ_SUB_FRAC 16             /* fraction bits of an amplitude */
#define GJ_SUB_MAX_AMP (1 << 19)   /* |aI|, |aQ| after the clamp: 8 LSB of replica per unit of the table */
#define GJ_SUB_DITHER 1            /* flags */
typedef struct gj_subtract_block { /* 24 bytes, all exact integers */
    uint64_t total;      /* sum of (I - 128)^2 + (Q - 128)^2 over the block's input samples */
    uint64_t removed;    /* sum of (in - out)^2 over both bytes of its samples, after the clamp */
    int32_t n_clipped;   /* bytes that the clamp to 0 .. 255 changed */
    int32_t reserved;    /* 0 */
} gj_subtract_block;
/* records of the subtraction: ceil(n_samples / GJ_SUB_BLOCK); pure host arithmetic, no context */
size_t gj_subtract_blocks(size_t n_samples);
int gj_subtract_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples,
                    int block_samples, const int16_t* d_codes /* [n_code_rows][1023], +-1 */, int n_code_rows,
                    const gj_corr_channel* d_channels, int n_channels,
                    const int32_t* d_amp /* [n_channels][gj_corr_blocks(n_samples, block_samples)][2]  aI, aQ */,
                    int flags, uint32_t seed, uint8_t* d_out /* [2*n_samples] */,
                    gj_subtract_block* d_blocks /* [gj_subtract_blocks(n_samples)] or NULL */);

/* ------------------------------------------------- closed-loop tracking: DLL / FLL / PLL per channel ---- */
/* The reference's receiver loop (sdrtracking -> correlator -> pll / dll, sdrtrk.c) for up to GJ_TRACK_MAX_CHANNELS
 * channels in one launch: every channel correlates one EPOCH of B = block_samples samples at early, prompt and late,
 * makes a carrier and a code discriminator of the three sums, filters them and steers its own carrier and code NCO
 * for the next epoch.  The loop is sequential per channel, the channels are independent: one workgroup each.  The
 * terms are the correlator bank's (gj_corr_channel, GJ_CORR_COS_TABLE, the chip rule, I, Q = byte - 128 WHATEVER
 * gj_set_unpack says); every step from the byte to the loop state is integer arithmetic.
 *
 * For channel ch with state S = d_states[ch] and epoch m = 0 .. n_epochs-1:
 *
 *   sums      (E, P, L) = the three records gj_corr_bank_dev defines for a call of n_samples = B that starts at sample
 *             first_sample + S.start + m*B, with the channel S.ch (as it stands NOW) and the taps (+d, 0, -d),
 *             d = params.spacing: local t = 0 .. B-1, the bank's carrier table, chip rule and unpacking
 *   cordic    (I, Q) -> (angle, length), in int64, A = GJ_TRACK_ATAN_TABLE:
 *             x = I * 2^8, y = Q * 2^8, z = 0;   if x < 0: (x, y) = (-x, -y)          the Costas fold
 *             for k = 0 .. 15:  if y >= 0: (x, y, z) <- (x + (y >> k), y - (x >> k), z + A[k])
 *                               else:      (x, y, z) <- (x - (y >> k), y + (x >> k), z - A[k])
 *             >> is arithmetic (floor), both updates use the OLD x and y.  angle = z in 2^-32 cycles, |z| <= sum A =
 *             1 191 629 338; length = x, about 421.6 |v|, below 2^34 for the bank's record bound.  I = Q = 0 gives
 *             angle 0 and length 0, a rule of its own (the steps would turn a zero vector by the whole table)
 *   discr.    e = angle(P);  mE = length(E), mL = length(L);
 *             c = floor((mE - mL) * 2^16 / (mE + mL)), 0 where mE + mL = 0     (|E| - |L|) / (|E| + |L|) in Q16,
 *                                                                              sdrtrk.c:99-100
 *             if S.primed == 0:  e_prev = e, c_prev = c, primed = 1
 *             f = e - e_prev;   f > 2^30: f = 2^31 - f;   f < -2^30: f = -2^31 - f
 *   filters   dn = floor((pll_p*(e - e_prev) + pll_i*e + fll*f) / 2^GJ_TRACK_PLL_SHIFT)       int64, mathematical floor;
 *             dc = floor((dll_p*(c - c_prev) + dll_i*c) / 2^GJ_TRACK_DLL_SHIFT)               |gain| <= 2^30: < 2^63
 *   record    d_out[ch][m] = E, P, L, the four NCO fields of S.ch as the sums were made with them, e, c
 *   advance   code_phase <- (code_phase + B*code_step) mod 1023 * 2^32;  carr_phase <- (carr_phase + B*carr_step) mod 2^32
 *             (with the OLD steps)
 *   steer     nco' = carr_nco - dn   (int64, wraps as two's complement);
 *             aid  = aid_div ? floor(nco' / aid_div) - floor(carr_nco / aid_div) : 0
 *             carr_step <- (carr_step - dn) mod 2^32;   code_step <- clamp(code_step + dc + aid, 0, GJ_CORR_MAX_CODE_STEP - 1)
 *             carr_nco <- nco';  e_prev <- e;  c_prev <- c
 *
 * After the last epoch S is written back with start advanced by n_epochs*B.  Signs: a replica that is late gives
 * c > 0 and (with positive dll gains) speeds the code up; a prompt whose angle grows lowers carr_step.
 *
 * Consequences.  Every value is an exact integer: the result does not depend on tiling or order, two calls give
 * identical bits, and it is a function of the bytes alone.  All gains 0 and aid_div 0 give, for start 0, the bits of
 * gj_corr_bank_dev with that constant channel, block_samples = B and taps (+d, 0, -d).  N epochs followed by M epochs
 * from the written-back states give the bits of N + M epochs.
 *
 * Limits (GJ_ERR_UNSUPPORTED): block_samples a multiple of 16 in 16 .. GJ_CORR_MAX_BLOCK; n_epochs 1 .. GJ_TRACK_MAX_EPOCHS
 * (the cap on how long one launch runs); n_channels 1 .. GJ_TRACK_MAX_CHANNELS; n_samples 1 .. GJ_CORR_MAX_SAMPLES;
 * spacing 1 .. GJ_CORR_MAX_TAP_OFFSET; aid_div >= 0; every gain within +-GJ_TRACK_MAX_GAIN.
 * GJ_ERR_INVALID: a null ctx, d_iq, d_codes, d_states or d_out; an odd d_iq or d_codes; a d_states or d_out that is
 * not 8-byte aligned; n_code_rows < 1; params.reserved != 0; n_epochs*B > n_samples; a range that runs past the
 * capture.  A refused call enqueues nothing.
 * The states are in DEVICE memory, as the bank's channels: Device.track (gpsjam/__init__.py) checks them on the host
 * before it uploads them and raises GJ_ERR_INVALID, and each workgroup checks ITS channel before it reads a chip.  A
 * channel is bad where its ch is (the bank's rule: reserved != 0, a code_row outside 0 .. n_code_rows-1, code_phase >=
 * 1023 * 2^32, code_step >= GJ_CORR_MAX_CODE_STEP), where a reserved word is not 0, where primed is neither 0 nor 1, or
 * where start + n_epochs*B > n_samples.  A bad channel writes NOTHING: its records and its state stay as they were.
 * The other channels run.
 * One launch on the context's stream; no workspace, no memset, no atomics: 0 bytes to gj_reserve, the call never
 * allocates.  Each record and each state is written by exactly one workgroup. */
typedef struct gj_track_state {   /* 64 bytes, DEVICE memory, in/out */
    gj_corr_channel ch;     /* the channel AT sample first_sample + start; the bank's bounds */
    int64_t  carr_nco;      /* what the loop has added to carr_step so far (for the aiding); 0 to begin */
    uint32_t start;         /* this channel's epoch 0 begins `start` samples after first_sample */
    int32_t  e_prev, c_prev;/* last epoch's discriminators; 0 to begin */
    int32_t  primed;        /* 0 to begin, 1 once e_prev / c_prev hold an epoch */
    int32_t  reserved[2];   /* 0 */
} gj_track_state;
typedef struct gj_track_params {  /* 32 bytes, by value */
    int32_t spacing;        /* d: early = tap +d, late = tap -d, whole samples, 1 .. GJ_CORR_MAX_TAP_OFFSET */
    int32_t aid_div;        /* carrier aiding: code_step follows carr_nco / aid_div (1540 for L1 C/A); 0 = none; >= 0 */
    int32_t pll_p, pll_i, fll, dll_p, dll_i;   /* |g| <= GJ_TRACK_MAX_GAIN */
    int32_t reserved;       /* 0 */
} gj_track_params;
typedef struct gj_track_epoch {   /* 56 bytes, all exact integers */
    int32_t  early[2], prompt[2], late[2];   /* I, Q */
    uint32_t carr_phase, carr_step;          /* the state the sums were made with, at the epoch's first sample */
    uint64_t code_phase, code_step;
    int32_t  e, c;                           /* the two discriminators of this epoch */
} gj_track_epoch;
#define GJ_TRACK_MAX_CHANNELS 4096
#define GJ_TRACK_MAX_EPOCHS (1 << 17)
#define GJ_TRACK_MAX_GAIN (1 << 30)
#define GJ_TRACK_PLL_SHIFT 32
#define GJ_TRACK_DLL_SHIFT 24
#define GJ_TRACK_ATAN_TABLE {536870912, 316933406, 167458907, 85004756, 42667331, 21354465, 10679838, 5340245, \
                             2670163, 1335087, 667544, 333772, 166886, 83443, 41722, 20861}  /* round(atan(2^-k) / 2pi * 2^32) */
int gj_track_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples, int block_samples,
                 int n_epochs, const int16_t* d_codes /* [n_code_rows][1023], +-1 */, int n_code_rows,
                 gj_track_state* d_states /* [n_channels], in/out */, int n_channels, gj_track_params params,
                 gj_track_epoch* d_out /* [n_channels][n_epochs] */);

/* ------------------------------------------------- subtraction of tracked signals ---- */
/* gj_subtract_dev with the replica's NCOs taken per EPOCH from the records gj_track_dev wrote, not from one channel per
 * call: a counterfeit signal followed by the loops is taken out over a whole capture, not over the tenth of a second
 * one Doppler and one code rate hold for.  The terms are the subtraction's and the bank's (GJ_CORR_COS_TABLE with
 * S[i] = C[(i - 4) & 15], the chip rule at tap 0, I, Q = byte - 128 WHATEVER gj_set_unpack says, GJ_SUB_*,
 * gj_subtract_block, gj_subtract_blocks).  gpsjam/track.py (amplitudes) makes the amplitudes from the records' own
 * prompts; gpsjam/spoof.py (remove_tracked) joins the pieces.
 *
 * For sample t = 0 .. n_samples-1 of the range and channel ch = d_channels[.], with B = block_samples, E = n_epochs:
 *
 *   r       = t - start                       the channel is SILENT at t if r < 0 or r >= E*B; otherwise
 *   m, u    = r div B, r mod B;   rec = d_epochs[ch][m]
 *             the channel is also silent at t if rec.code_phase >= 1023 * 2^32 or rec.code_step >= GJ_CORR_MAX_CODE_STEP
 *   chip    = ((rec.code_phase + u*rec.code_step) mod 1023 * 2^32) >> 32,   c = d_codes[code_row][chip] as +-1
 *   i       = ((rec.carr_phase + u*rec.carr_step) mod 2^32) >> 28
 *   a       = clamp(d_amp[ch][m][0..1], -GJ_SUB_MAX_AMP, +GJ_SUB_MAX_AMP)
 *   R_I, R_Q  gj_subtract_dev's sums, over the channels that are not silent at t
 *   d, q, the output byte and the gj_subtract_block records: gj_subtract_dev's, word for word; the dither is keyed on
 *   the ABSOLUTE sample first_sample + t.
 *
 * Only carr_phase, carr_step, code_phase and code_step of a record are read.  The records are device memory and far
 * too many for every workgroup to check, so a record out of bounds adds nothing: that is part of the definition, not
 * an error.  d_amp: int32[n_channels][n_epochs][2], not checked (the clamp is part of the definition).
 *
 * Consequences.  With records that are one constant channel advanced by m*B samples per epoch, start 0 and
 * n_samples = E*B, the call writes the bytes and the records of gj_subtract_dev with that channel and the same
 * amplitudes.  All amplitudes 0, or every channel silent everywhere, gives back the input bytes.  Every value is an
 * exact integer: the bytes do not depend on tiling or order, two calls give identical bits.  Widths: u < 4096 and
 * code_step < 2^34 give u*code_step < 2^46; R's bound is gj_subtract_dev's (64 channels at the most add up).  Samples
 * in front of a channel's start and behind its last whole epoch keep that channel's signal.
 *
 * Limits (GJ_ERR_UNSUPPORTED): gj_subtract_dev's (block_samples a multiple of 16 in 16 .. GJ_CORR_MAX_BLOCK, n_channels
 * 1 .. GJ_CORR_MAX_CHANNELS, n_samples 1 .. GJ_CORR_MAX_SAMPLES); n_epochs < 1.
 * GJ_ERR_INVALID: gj_subtract_dev's (a null ctx or buffer, d_epochs among them; an odd d_iq or d_codes; a d_amp that is
 * not 4-byte aligned, a d_blocks that is not 8-byte aligned; n_code_rows < 1; a flag bit other than GJ_SUB_DITHER; a
 * range that runs past the capture; a d_out that overlaps the capture); a d_channels or d_epochs that is not 8-byte
 * aligned; n_epochs*B > n_samples.  A refused call enqueues nothing.
 * The channel table is in DEVICE memory: Device.subtract_tracked (gpsjam/__init__.py) checks it on the host before it
 * uploads it and raises GJ_ERR_INVALID, and every workgroup checks all of it before it reads a chip: if ANY code_row
 * lies outside 0 .. n_code_rows-1 or ANY start + n_epochs*B > n_samples, the launch writes NOTHING, neither a byte nor
 * a record.
 * One launch on the context's stream; no workspace, no memset, no atomics: 0 bytes to gj_reserve, the call never
 * allocates.  Every byte and every record is written by exactly one workgroup. */
typedef struct gj_subtract_track_channel {   /* 8 bytes */
    uint32_t start;        /* this channel's epoch 0 begins `start` samples after first_sample (gj_track_state.start) */
    int32_t  code_row;     /* row of d_codes */
} gj_subtract_track_channel;
int gj_subtract_track_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t n_samples,
                          int block_samples, int n_epochs, const int16_t* d_codes /* [n_code_rows][1023], +-1 */,
                          int n_code_rows, const gj_subtract_track_channel* d_channels /* at most 64 */, int n_channels,
                          const gj_track_epoch* d_epochs /* [n_channels][n_epochs], as gj_track_dev wrote them */,
                          const int32_t* d_amp /* [n_channels][n_epochs][2]  aI, aQ */,
                          int flags, uint32_t seed, uint8_t* d_out /* [2*n_samples] */,
                          gj_subtract_block* d_blocks /* [gj_subtract_blocks(n_samples)] or NULL */);

/* ------------------------------------------------- pair alignment --------------------- */
/* One uint8 I/Q capture written from another along a linear time base and a linear phase: antenna b brought onto
 * antenna a's clock, for receivers that each run on a crystal of their own (the crystal sets the sample clock AND the
 * tuner: 1 ppm is a slip of 20 samples over 10 s and 1575 Hz at L1).  The capture is resampled by a polyphase FIR,
 * rotated, and rounded ONCE; every step from the byte to the byte is integer arithmetic.  gpsjam/align.py makes the
 * tables and the parameters (taps, rot_table, params), estimates lag, drift and offset of a pair (estimate) and joins
 * the pieces (to).
 *
 * I, Q are taken as u = 2*byte - 255 WHATEVER gj_set_unpack says, and u is ZERO outside samples 0 .. nbytes/2 - 1 of
 * the source.  With P = GJ_ALIGN_PHASES = 256, T = GJ_ALIGN_TAPS = 16, GJ_ALIGN_ROT_LEN = 1024, for n = 0 .. n_out-1:
 *
 *   pos   = pos0 + n*pos_step + 2^23          int64, Q31.32 source samples; mathematical floor below
 *   k     = floor(pos / 2^32),   p = (pos mod 2^32) >> 24
 *   yI    = sum_{j=0..15} taps[p][j] * uI[k - 7 + j]            (yQ likewise)    |y| <= 16*255*32768 < 2^31
 *   theta = (rot_phase + n*rot_step) mod 2^32,   i = ((theta + 2^21) >> 22) & 1023
 *   c = rot[i],  s = rot[(i - 256) & 1023]
 *   zI = yI*c - yQ*s,   zQ = yI*s + yQ*c                        int64: y times (c + js)
 *   out byte = clamp(floor(z / 2^29) + 128, 0, 255)
 *
 * taps (int16[256][16], unit gain 16384: row p interpolates at k + p/256, tap 7 on sample k) and rot (int16[1024],
 * 16384 cos(2 pi i / 1024)) are the CALLER's device tables, as d_codes is the bank's: the bytes depend on no libm.
 * Any int16 values are accepted: the widths above hold at the full range.  With row 0 of taps the delta at j = 7,
 * rot[0] = 16384, pos0 = 0, pos_step = 2^32 and rot_phase = rot_step = 0 the call is the identity, byte for byte:
 * z = u * 2^28 and floor((2b - 255) / 2) + 128 = b.  pos and theta are functions of n alone: a call on n = n1 ..
 * with pos0 + n1*pos_step and rot_phase + n1*rot_step in their places writes the bytes the larger call writes there.
 *
 * d_out: 2*n_out bytes, any alignment (16-byte stores where it is 16-byte aligned).  d_blocks (optional, may be NULL;
 * the bytes are the same) receives one record per GJ_ALIGN_BLOCK output samples, the last one ragged.
 *
 * Limits (GJ_ERR_UNSUPPORTED): |pos_step - 2^32| <= GJ_ALIGN_MAX_DRIFT = 2^24 (3900 ppm: no anti-alias stage is needed,
 * and the source span of GJ_ALIGN_BLOCK outputs is bounded); n_out 1 .. GJ_ALIGN_MAX_SAMPLES; |pos0| < 2^60.
 * GJ_ERR_INVALID: a null ctx, d_iq, d_taps, d_rot or d_out; an odd d_iq; a d_taps or d_rot that is not 4-byte aligned;
 * a d_blocks that is not 8-byte aligned; reserved != 0; a d_out whose 2*n_out bytes overlap d_iq[0, nbytes) anywhere.
 * A refused call enqueues nothing.  One launch on the context's stream; no workspace, no memset, no atomics: the call
 * never allocates.  Every byte and every record is written by exactly one workgroup. */
#define GJ_ALIGN_PHASES 256            /* rows of taps: sub-sample positions */
#define GJ_ALIGN_TAPS 16               /* taps per row */
#define GJ_ALIGN_ROT_LEN 1024          /* entries of rot: one turn */
#define GJ_ALIGN_BLOCK 4096            /* output samples per record */
#define GJ_ALIGN_MAX_DRIFT (1 << 24)   /* |pos_step - 2^32| */
#define GJ_ALIGN_MAX_SAMPLES (1 << 28) /* n_out */
typedef struct gj_align_params {       /* 32 bytes, passed by value */
    int64_t pos0;        /* source position of output sample 0, Q31.32 samples */
    uint64_t pos_step;   /* source samples per output sample, Q32.32 */
    uint32_t rot_phase;  /* phase of output sample 0, 2^32 per turn */
    uint32_t rot_step;   /* phase per output sample */
    uint64_t reserved;   /* 0 */
} gj_align_params;
typedef struct gj_align_block {        /* 16 bytes, all exact integers */
    uint64_t power_out;  /* sum of (2*out - 255)^2 over both bytes of the block's output samples */
    int32_t n_clipped;   /* bytes that the clamp to 0 .. 255 changed */
    int32_t n_edge;      /* samples with at least one tap outside the source */
} gj_align_block;
/* records of the alignment: ceil(n_out / GJ_ALIGN_BLOCK); pure host arithmetic, no context */
size_t gj_align_blocks(size_t n_out);
int gj_align_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, gj_align_params params,
                 const int16_t* d_taps /* [GJ_ALIGN_PHASES][GJ_ALIGN_TAPS] */, const int16_t* d_rot /* [GJ_ALIGN_ROT_LEN] */,
                 size_t n_out, uint8_t* d_out /* [2*n_out] */,
                 gj_align_block* d_blocks /* [gj_align_blocks(n_out)] or NULL */);

/* ------------------------------------------------- per-stream result vector ---------- */
/* What one rank sends to rank 0 (gpsjam/sharded.py):
 * double[40 + n_chunks + nperseg + 5*pair_capacity] =
 * header {  0 n_chunks, 1 baseline, 2 threshold, 3 n_above, 4 amp.first_index, 5 amp.count, 6 amp.mean,
 *           7 onset.start_index, 8 lag vs antenna 0 (0 on rank 0, GJ_LAG_INVALID elsewhere: the receiver
 *           fills it in from the pair table), 9 0, 10 onset.noise_power, 11 rows, 12 nperseg, 13 rank,
 *          14 n_pairs, 15 pair_capacity,
 *          16 onset.margin_hit, 17 onset.margin_before, 18 onset.guard_index, 19 onset.threshold -- the
 *             decision margins of K4 travel with the result, so the receiver knows when an onset was
 *             decided inside the rounding band (skrypty/triangulateTDOA.py:37-49),
 *          20 antenna, 21 part, 22 parts (1 = the stream is a whole capture), 23 first chunk, 24 first row,
 *          25 first sample of the part, 26 amp.sum, 27 amp tail, 28 tiles, 29 first tile, 30-31 reserved,
 *          32-35 the gj_onset record as it is (32 bytes), 36-39 the gj_amp_stats (gj_amp_part for a
 *          part) record as it is },
 * the float32 power map, the mean over the rows of the PSD waterfall, and the pairs THIS stream
 * solved as {i, j, lag, peak, margin} each (d_pairs = {i0,j0,i1,j1,...} and the outputs of
 * gj_xcorr_slots_dev, all DEVICE arrays), zero-padded to pair_capacity -- packed by one kernel
 * from device-resident outputs (no host synchronisation).  nperseg: power of two, 16..4096, as K2 takes it
 * (GJ_ERR_UNSUPPORTED otherwise, nothing is written); rows may be 0 (d_psd NULL): the spectrum is then zero. */
#define GJ_RESULT_HEADER 40
#define GJ_RESULT_PAIR_FIELDS 5
int gj_pack_result_dev(gj_ctx* ctx, size_t n_chunks, const float* d_power, const float* d_stats,
                       const gj_amp_stats* d_amp, const gj_onset* d_onset, const float* d_psd, size_t rows,
                       int nperseg, int rank, int n_pairs, int pair_capacity, const int32_t* d_pairs,
                       const int32_t* d_lags, const float* d_peaks, const float* d_margins, double* d_out);

/* gj_pack_result_dev for up to GJ_MAX_ANTENNAS captures in ONE launch.  `captures` is a HOST array of gj_combine_capture
 * (declared below) of which the fields n_chunks, rows, antenna (-> header field 13), n_pairs, pair_cap, d_power, d_stats,
 * d_amp, d_onset, d_psd and d_out are read; the pair arrays are shared (the capture with n_pairs > 0 carries them). */
struct gj_combine_capture;
int gj_pack_results_dev(gj_ctx* ctx, const struct gj_combine_capture* captures, int n_captures, int nperseg,
                        const int32_t* d_pairs, const int32_t* d_lags, const float* d_peaks, const float* d_margins);

/* ------------------------------------------------- one capture over several GPUs ------ */
/* "fewer files than GPUs => split one file into contiguous chunk ranges aligned to
 * 65 536 B / 1-s chunks".  The reference's deployment has THREE antennas (GpsJammerApp/app/worker.py:97-101,
 * 586-600; skrypty/triangulateRSSI.py:147-154); on an 8-GPU node each capture is cut into parts, one per GPU.
 * A part OWNS the capture bytes [own_first_byte, own_first_byte + own_bytes): a whole number of power chunks and
 * of PSD chunks (only the capture's last part may end ragged).  Its device buffer additionally holds
 *   - a HALO in front (whole 64-KiB tiles, >= window - 1 samples; none for the first part), so that K4 evaluates
 *     every window that ends inside the own range: the parts' position ranges then tile the capture,
 *   - a TAIL behind (>= the TDOA slice), so that a slice that starts in the own range can be cut here,
 * and every part but the first brings the capture's first 2*noise_samples bytes (d_noise) for K4's threshold --
 * each rank reads those few hundred KB itself, so K1-K4 need NO collective.  Results are in CAPTURE coordinates
 * and bit-identical to the unsplit run by construction: chunk powers and PSD rows are per-chunk quantities (the
 * Welch workgroup split is planned for the whole capture), amplitude sums travel as per-tile sums and are added
 * by the same code in the same order (gj_amp_combine_dev), window sums are exact integers. */
typedef struct gj_part_view {
    const uint8_t* d_buf;  /* DEVICE: capture bytes [buf_first_byte, buf_first_byte + buf_bytes), 16-byte aligned */
    size_t buf_bytes;
    size_t buf_first_byte;
    size_t own_first_byte; /* multiple of chunk_bytes and of 2*chunk_samples; own_first_byte - buf_first_byte = halo */
    size_t own_bytes;
    size_t total_bytes;    /* of the whole capture */
    const uint8_t* d_noise; /* DEVICE: the capture's first 2*noise_samples bytes (may be NULL for a first part
                             * whose own range holds them) */
} gj_part_view;
typedef struct gj_amp_part {
    int64_t first_index; /* capture coordinates; -1: nothing above the threshold in this part */
    uint64_t count;      /* own samples from first_index to the end of the own range */
    double sum;          /* of the amplitudes over those samples (this part alone) */
    double tail;         /* of the amplitudes from first_index to the end of ITS 64-KiB tile */
} gj_amp_part;
/* 64-KiB amplitude tiles of a range of nbytes (16 bytes each: double sum, int64 first) */
size_t gj_amp_tile_count(size_t nbytes);
/* K1 + K3 + K4 of one part in one pass (gj_stream_scan_dev for a part): d_power[own chunks], d_tiles[own tiles],
 * *d_amp, *d_onset (capture coordinates; duplicates of a crossing inside the halo are harmless: the combining
 * rank takes the smallest index). */
int gj_part_scan_dev(gj_ctx* ctx, const gj_part_view* part, size_t chunk_bytes, float eps, int flags, float* d_power,
                     float rssi_threshold, void* d_tiles, gj_amp_part* d_amp, int noise_samples, int window,
                     float factor, gj_onset* d_onset);
/* gj_part_scan_dev + gj_part_slot_dev (at &d_onset->start_index) in the same two launches as gj_capture_scan_dev */
int gj_part_capture_scan_dev(gj_ctx* ctx, const gj_part_view* part, size_t chunk_bytes, float eps, int flags, float* d_power,
                             float rssi_threshold, void* d_tiles, gj_amp_part* d_amp, int noise_samples, int window,
                             float factor, gj_onset* d_onset, const gj_scan_extra* extra);
/* K2 of the own range: rows [own_first_byte / (2 chunk_samples), ...) of the capture's waterfall */
int gj_part_welch_dev(gj_ctx* ctx, const gj_part_view* part, size_t chunk_samples, int nperseg, double fs, int flags,
                      float* d_psd, float* d_psd_db);
size_t gj_part_welch_workspace(gj_ctx* ctx, const gj_part_view* part, size_t chunk_samples, int nperseg);
/* TDOA slot cut from a part's buffer at the CAPTURE index *d_start (flag -2: valid in the capture but not held here) */
int gj_part_slot_dev(gj_ctx* ctx, const gj_part_view* part, const int64_t* d_start, size_t n_samples, uint8_t* d_slot);
/* Slots of the parts -> one slot per capture: group g = the slots d_members[d_offsets[g]] ...
 * d_members[d_offsets[g+1] - 1] (DEVICE int arrays, d_offsets has n_groups + 1 entries); its slot is the one cut
 * at the smallest start >= 0 (none: an invalid slot with start -1). */
int gj_slots_pick_dev(gj_ctx* ctx, const uint8_t* d_slots, size_t slot_stride, const int32_t* d_offsets,
                      const int32_t* d_members, int n_groups, uint8_t* d_out);
/* On the combining rank: the capture's amplitude statistics from ALL its tile sums (in tile order) and the parts'
 * first hits; its onset from the parts' onsets. */
int gj_amp_combine_dev(gj_ctx* ctx, const void* d_tiles, size_t n_tiles, const gj_amp_part* d_parts, int n_parts,
                       size_t total_bytes, gj_amp_stats* d_out);
int gj_onset_combine_dev(gj_ctx* ctx, const gj_onset* d_parts, int n_parts, gj_onset* d_out);
/* What a part sends to the combining rank: double[gj_part_result_len] = the 40-field header of
 * gj_pack_result_dev (part fields filled, records 32-39 = gj_onset, gj_amp_part), chunk_cap chunk powers,
 * tile_cap x (sum, first) tile records, pair_cap x {i, j, lag, peak, margin}, rows_cap x nperseg PSD values as
 * float32 (two per double slot).  The capacities are the largest over all parts, so every vector has one length. */
typedef struct gj_part_pack {
    int32_t rank, antenna, part, parts;
    uint64_t first_chunk, n_chunks, chunk_cap;
    uint64_t first_row, rows, rows_cap;
    uint64_t first_tile, n_tiles, tile_cap;
    int64_t first_sample;
    int32_t nperseg, n_pairs, pair_cap, reserved;
    const float* d_power;
    const gj_amp_part* d_amp;
    const gj_onset* d_onset;
    const void* d_tiles;
    const float* d_psd;
    const int32_t* d_pairs;
    const int32_t* d_lags;
    const float* d_peaks;
    const float* d_margins;
} gj_part_pack;
size_t gj_part_result_len(size_t chunk_cap, size_t tile_cap, size_t rows_cap, int nperseg, int pair_cap);
int gj_pack_part_dev(gj_ctx* ctx, const gj_part_pack* args, double* d_out);

/* The combining rank, every capture at once.  gj_amp_combine_dev / gj_onset_combine_dev / gj_power_threshold_dev /
 * gj_pack_result_dev finish ONE capture and want its arrays contiguous; with three antennas cut into ten parts that is
 * a chain of some forty small launches and copies on the combining rank -- the critical path once a rank's own K2 has
 * shrunk to 1/8.  gj_split_combine_dev does the same work in THREE launches whatever the number of antennas:
 *   1. assemble: every copy of `copies` (part vector -> capture-order array) in one grid;
 *   2. statistics: one workgroup per capture for the noise-floor threshold, one for amplitude totals + onset;
 *   3. pack: one grid row per capture (the layout of gj_pack_result_dev).
 * The kernels' bodies are those of the one-capture entry points (same code, same order, same bits).  The copy list and
 * the capture descriptors are static for a deployment: gj_combine_plan_create checks on the HOST that every copy
 * reads inside the gathered vectors (rows_bytes) and that every destination / array lies inside the caller's arena
 * (one device allocation holding all assembled arrays and result vectors), then keeps device copies of both. */
typedef struct gj_combine_copy {
    uint64_t src_byte;   /* offset of the first source element in the gathered part vectors */
    uint64_t dst;        /* DEVICE address of the first destination element (inside the arena) */
    uint64_t count;      /* elements */
    uint32_t src_stride; /* bytes between source elements (8 for a run of doubles, 40 for one field of the pair block) */
    uint32_t kind;       /* GJ_COPY_* */
} gj_combine_copy;
#define GJ_COPY_F64_F32 0 /* double -> float32 (chunk powers, pair peaks / margins) */
#define GJ_COPY_F64 1     /* 8-byte copy (amplitude tile records, gj_onset / gj_amp_part records) */
#define GJ_COPY_F32 2     /* 4-byte copy (PSD rows) */
#define GJ_COPY_F64_I32 3 /* double -> int32 (pair lags) */
typedef struct gj_combine_capture {
    uint64_t n_chunks, rows, n_tiles, total_bytes;
    int32_t n_parts, antenna;
    int32_t n_pairs, pair_cap; /* pairs this capture's vector carries (all of them on antenna 0, none elsewhere) */
    float* d_power;            /* [n_chunks]        assembled */
    float* d_stats;            /* [3]               written by step 2 */
    void* d_tiles;             /* [n_tiles] x 16 B  assembled */
    gj_amp_part* d_amp_parts;  /* [n_parts]         assembled */
    gj_onset* d_onset_parts;   /* [n_parts]         assembled */
    gj_amp_stats* d_amp;       /* written by step 2 */
    gj_onset* d_onset;         /* written by step 2 */
    float* d_psd;              /* [max(rows,1)][nperseg] assembled */
    double* d_out;             /* [40 + n_chunks + nperseg + 5 pair_cap] written by step 3 */
} gj_combine_capture;
typedef struct gj_combine_plan gj_combine_plan;
int gj_combine_plan_create(gj_ctx* ctx, const gj_combine_copy* copies, int n_copies, const gj_combine_capture* captures,
                           int n_captures, size_t rows_bytes, const void* d_arena, size_t arena_bytes, int nperseg,
                           float pct, float rise_db, const int32_t* d_pairs /* every solved pair, static */,
                           const int32_t* d_lags, const float* d_peaks, const float* d_margins /* assembled */,
                           gj_combine_plan** out);
/* The validation of gj_combine_plan_create alone (host arithmetic only; no context, no GPU): GJ_OK, or the status the
 * create call would return for these lists.  Bounds are taken by division, so a count or stride chosen to wrap a 64-bit
 * product is refused like any other out-of-range value. */
int gj_combine_plan_check(const gj_combine_copy* copies, int n_copies, const gj_combine_capture* captures, int n_captures,
                          size_t rows_bytes, const void* d_arena, size_t arena_bytes, int nperseg, int have_pairs);
int gj_split_combine_dev(gj_ctx* ctx, const gj_combine_plan* plan, const double* d_rows);
int gj_combine_plan_destroy(gj_ctx* ctx, gj_combine_plan* plan); /* idempotent on NULL; synchronises the context's stream */

/* ------------------------------------------------- GNSS acquisition search ----------- */
/* the reference receiver's parallel code-phase search, batched over every
 * PRN and Doppler bin.  Replaces, per call, what each of its channel threads does on its own:
 *   sdraqcuisition    GpsJammerApp/backend/sdracq.c:3-50    loop over `intg` steps, early stop
 *   pcorrelator       GpsJammerApp/backend/sdrcmn.c:742-773 per bin: mixcarr -> cpxcpx -> cpxconv
 *   mixcarr           sdrcmn.c:618-705 (the SSE2 form the reference's makefile builds)
 *   cpxconv           sdrcmn.c:124-147 FFT . conj(code FFT) . IFFT -> |.|^2 / m^2, accumulated
 *   checkacquisition  sdracq.c:52-84   peak, +-2 chip exclusion zone, peak ratio > threshold
 * Inputs (device memory): the capture as int8 = u8 - 128 (sdrrcv.c:104-106); step s of the search
 * reads the 2*nsamp samples from first_sample + s*nsamp; d_codes[p][nsamp] = the code of PRN p
 * resampled to the sampling rate (+-1, int16: rescode, sdrinit.c:439); d_phase[f][2*nsamp] = the
 * mixer's 4-bit phase index per sample for Doppler bin f, built on the host the way mixcarr
 * builds it (gpsjam/gnss.py).  nsamp: 512, 1024 or 2048 (FFT length 2*nsamp, sdrinit.c:402).
 * A PRN stops integrating at the first step whose peak ratio passes (results of that step are
 * kept); the others run all `intg` steps.  d_power (optional) receives the accumulated
 * correlation power double[n_prn][n_freq][nsamp] (the reference's `power` array). */
typedef struct gj_acq_result {
    double max_power;    /* maxP */
    double second_power; /* maxP2: largest power of the peak's Doppler row outside the exclusion zone */
    double mean_power;   /* meanP of that row outside the exclusion zone */
    double peak_ratio;   /* maxP / maxP2 (acq.peakr) */
    double cn0;          /* 10 log10(maxP / meanP / ctime) */
    int32_t code_index;  /* acq.acqcodei */
    int32_t freq_index;  /* acq.freqi */
    int32_t steps;       /* integration steps used, 1..intg */
    int32_t acquired;    /* peak_ratio > threshold */
} gj_acq_result;
int gj_acq_search_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, int nsamp,
                      int intg, const int16_t* d_codes, int n_prn, const uint8_t* d_phase, int n_freq,
                      int nsampchip, double ctime, float threshold, gj_acq_result* d_out /* [n_prn] */,
                      double* d_power /* [n_prn*n_freq*nsamp] or NULL */);
size_t gj_acq_workspace(gj_ctx* ctx, int nsamp, int n_freq, int n_prn, int intg, int with_power);
/* Acquisition series: n_epochs searches of a resident capture, epoch e at first_sample + e*stride_samples
 * (overlapping windows and stride 0 are allowed), d_out[e][p] = what gj_acq_search_dev(first_sample +
 * e*stride_samples) without d_power writes for PRN p, bit for bit.  The code spectra are transformed once per
 * call; the epochs run in batches of at most epochs_per_launch (0: 16; at most 4096), three launches per batch.
 * Arguments and limits as in gj_acq_search_dev, and n_epochs >= 1; the last epoch's window must lie in the
 * capture.  A refused call enqueues nothing.  The cn0 is the acquisition's 10 log10(maxP / meanP / ctime):
 * comparable between epochs of one capture, not with a tracking loop's C/N0. */
int gj_acq_series_dev(gj_ctx* ctx, const uint8_t* d_iq, size_t nbytes, size_t first_sample, size_t stride_samples,
                      int n_epochs, int epochs_per_launch, int nsamp, int intg, const int16_t* d_codes, int n_prn,
                      const uint8_t* d_phase, int n_freq, int nsampchip, double ctime, float threshold,
                      gj_acq_result* d_out /* [n_epochs][n_prn] */);
/* The workspace gj_acq_series_dev ensures for these arguments (reserve it first to capture the call in a graph);
 * 0 for arguments it would refuse by sign. */
size_t gj_acq_series_workspace(gj_ctx* ctx, int nsamp, int n_freq, int n_prn, int intg, int n_epochs,
                               int epochs_per_launch);
/* K-peak search: the k largest peaks of every PRN's power surface under successive column exclusion, and the floor
 * outside all of them.  checkacquisition (sdracq.c:52-84) keeps one peak per PRN; a second signal of the same PRN --
 * a counterfeit above the authentic one -- is a second peak of the same surface, at another code phase.
 *
 * d_power: double[n_prn][n_freq][nsamp], as gj_acq_search_dev writes it; cell (f, c) has the flat index f * nsamp + c.
 * For every PRN, j = 0 .. k - 1:
 *   peak j   = the cell of largest power among the columns (code indices) c not excluded by peaks 0 .. j - 1; of
 *              equal powers the smallest flat index wins (checkacquisition's first maximum, maxvd);
 *   excluded by a peak at code index c0 are the columns c with min(|c - c0|, nsamp - |c - c0|) <= guard, in EVERY
 *              Doppler row (a signal's Doppler sidelobes sit at its own code phase).  With guard = 2 * nsampchip these
 *              are the indices checkacquisition drops, its wrapped case included;
 *   floor    = the mean of the n_freq * kept_columns cells of the columns no peak excludes.
 * Powers are finite and >= 0 (what the search writes); on anything else the call still writes its own records only.
 * Peaks are exact (comparisons only); the floor is a sum of doubles in a fixed order, equal from call to call and
 * within n_freq * kept_columns * 2^-53 relative of any other order.
 *
 * Limits: nsamp 8 .. 65536 (any value), n_freq 1 .. 4096, k 1 .. GJ_ACQ_MAX_PEAKS (GJ_ERR_UNSUPPORTED); n_prn >= 1,
 * guard >= 0, k * (2 * guard + 1) < nsamp, no null pointer, all three buffers 8-byte aligned (GJ_ERR_INVALID).  A
 * refused call enqueues nothing.  Two launches on the context's stream, no atomics, no memset; allocates nothing when
 * gj_acq_peaks_workspace bytes were reserved (gj_reserve). */
#define GJ_ACQ_MAX_PEAKS 8
typedef struct gj_acq_peak {          /* 16 bytes */
    double power;
    int32_t code_index;
    int32_t freq_index;
} gj_acq_peak;
typedef struct gj_acq_floor {         /* 16 bytes */
    double mean_power;
    int32_t kept_columns;
    int32_t reserved;                 /* 0 */
} gj_acq_floor;
int gj_acq_peaks_dev(gj_ctx* ctx, const double* d_power, int n_prn, int n_freq, int nsamp, int k, int guard,
                     gj_acq_peak* d_peaks /* [n_prn][k] */, gj_acq_floor* d_floor /* [n_prn] */);
/* The workspace gj_acq_peaks_dev ensures for these arguments; 0 for arguments it would refuse. */
size_t gj_acq_peaks_workspace(gj_ctx* ctx, int nsamp, int n_prn);

/* ------------------------------------------------- collectives (RCCL over xGMI) ------- */
/* One communicator rank per GPU / process, for hosts without torch.distributed.  The path
 * shards by capture (file k -> GPU k) and has ONE exchange: TDOA slots and per-stream result
 * vectors travel to the solving rank (ncclGather, rccl.h:745).  The reference has no
 * equivalent (one process, numpy).  Rank 0 calls gj_comm_unique_id and ships the 128 bytes to
 * the other ranks by whatever means the host has (gpsjam/comm.py: one TCP socket on
 * MASTER_ADDR:MASTER_PORT); every rank then calls gj_comm_init_rank on ITS context.
 * Collectives are enqueued on the context's current stream (gj_set_stream) and do not
 * synchronise the host; buffers are device memory.  The context lock is NOT held across the RCCL
 * call (a communicator's first collective connects its peers inside the call and may wait for a
 * late rank): other threads keep using the context meanwhile; the order of collectives on one
 * communicator is the caller's.  gj_comm_destroy -- and gj_destroy of the communicator's context --
 * detach the communicator first (a call that starts afterwards answers GJ_ERR_INVALID) and wait for the
 * calls already in progress on it to return before RCCL's handle is destroyed; the two must not be
 * called concurrently with each other for the same context.  librccl is bound at run time
 * (GJ_ERR_UNSUPPORTED when it cannot be loaded). */
typedef struct gj_comm gj_comm;
#define GJ_COMM_ID_BYTES 128
int gj_comm_unique_id(void* id /* [GJ_COMM_ID_BYTES] */);
int gj_comm_init_rank(gj_ctx* ctx, const void* id, int rank, int n_ranks, gj_comm** out);
/* rank and size as the LIVE communicator reports them (ncclCommUserRank / ncclCommCount), not as passed at init;
 * -1 of 0 for a communicator whose context has been destroyed.  gj_comm_device: the HIP device it is bound to. */
int gj_comm_rank(gj_comm* comm, int* rank, int* n_ranks);
int gj_comm_device(gj_comm* comm, int* hip_device);
/* every rank sends `bytes` bytes; root receives n_ranks*bytes in rank order (d_recv may be NULL
 * elsewhere) */
int gj_comm_gather_dev(gj_comm* comm, const void* d_send, size_t bytes, void* d_recv, int root);
/* every rank sends `bytes` bytes and receives all n_ranks*bytes in rank order (ncclAllGather) */
int gj_comm_allgather_dev(gj_comm* comm, const void* d_send, size_t bytes, void* d_recv);
int gj_comm_bcast_dev(gj_comm* comm, void* d_buf, size_t bytes, int root);
int gj_comm_destroy(gj_comm* comm); /* idempotent on NULL; synchronises the context's stream */

/* ------------------------------------------------- synthetic captures --------------- */
/* Bit-identical to gpsjam/synth.py (integer-only counter-based generator that mirrors
 * the value distribution of simulate/frontend/weaken_gps.py + add_jammer_and_mix.py). */
typedef struct gj_synth_params {
    uint64_t key_noise;  /* per-antenna hash key */
    uint64_t key_common; /* common-source hash key */
    int64_t delay;       /* samples by which this antenna sees the source late */
    int64_t jam_start;   /* source-time sample range [start, end) of the burst */
    int64_t jam_end;
    int32_t noise_k; /* fixed-point gains, see synth.gain_k */
    int32_t jam_k;
    int32_t dc_i_q8; /* DC offsets in 1/256 LSB */
    int32_t dc_q_q8;
} gj_synth_params;
int gj_synth_u8_dev(gj_ctx* ctx, const gj_synth_params* params, int64_t first_sample,
                    size_t n_samples, uint8_t* d_out /* [2*n_samples] */);

#ifdef __cplusplus
}
#endif
#endif /* GPSJAM_H */
