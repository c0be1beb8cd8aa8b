"""K2 (gj_welch_dev) at all nine sizes against the float64 restatement of the Welch waterfall (tests/welch_restatement.py),
at the smallest geometries that reach every branch of the kernel: one segment per chunk (every row a single periodogram:
no averaging hides a butterfly), B - 1, B and B + 1 segments (B = 4096 / nperseg transform groups per workgroup: idle
groups, one exactly full step, one step and a segment; at 2048 points runs of 1, 2 and 3), an odd chunk_samples (chunks
1 and 3 start on an odd sample: 2-byte-aligned 16-byte segment loads at 16 and 32 points, trailing samples that belong
to no segment), and two shapes with several workgroups per chunk and uneven segment ranges, the larger with at least
five partial rows so that the finalize's four row lanes wrap.  Every capture is three full chunks and a ragged last one.

The measure is welch_restatement.errors (a bin's difference against the bin, its row's mean level or the floor of
test_extremes_gpu.test_extreme_k2_welch, whichever is largest); the tolerance is 4 x E32[nperseg][class], E32 the error
of the float32 restatement of K2's own form measured on the CPU over these very cases (tests/test_welch_host.py holds
each constant within a factor 2 of its measurement and shows that every defect it lists is further off than the
tolerance).  No tolerance comes from a GPU result."""
import numpy as np
import pytest

import welch_restatement as wr

pytestmark = pytest.mark.gpu

CASES = [(nperseg, shape, klass, name) for nperseg in wr.SIZES for klass in wr.CLASSES for shape, name in wr.cases_of(nperseg, klass)]


def _id(case):
    nperseg, shape, klass, name = case
    return f"{nperseg}-{shape}-{klass}" + (f"-{name.replace(' ', '_')}" if name else "")


def launch(dev, d_iq, nbytes, chunk, nperseg, rows, shift=True, want_db=False):
    d_psd = dev.alloc(4 * rows * nperseg)
    d_db = dev.alloc(4 * rows * nperseg) if want_db else None
    dev.welch_dev(d_iq, nbytes, chunk, nperseg, wr.FS, d_psd, d_db, shift=shift)
    dev.synchronize()
    psd = d_psd.download(np.float32).reshape(rows, nperseg)
    return (psd, d_db.download(np.float32).reshape(rows, nperseg)) if want_db else psd


def held(label, got_unshifted, truth, tol, one_segment):
    """The case error is within the tolerance; says where the largest error is."""
    assert got_unshifted.shape == truth.shape and np.all(np.isfinite(got_unshifted)) and np.all(got_unshifted >= 0)
    e = wr.errors(got_unshifted, truth)
    row, k = np.unravel_index(int(np.argmax(e)), e.shape)
    print(f"{label}: case error {e[row, k]:.3e} of tolerance {tol:.3e} (row {row} of {e.shape[0]}, bin {k}, "
          f"{'one segment per row' if one_segment else 'averaged rows'})")
    assert e[row, k] <= tol, label
    return float(e[row, k])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_k2_against_the_float64_welch(dev, case):
    nperseg, shape, klass, name = case
    chunk, samples, rows, nseg, _ = wr.geometry(nperseg, shape)
    tol = wr.tolerance(nperseg, klass)
    nbytes = 2 * samples
    raw = wr.capture(nperseg, shape, klass, name)                       # one sample longer than the geometry
    cap = dev.alloc(raw.size).upload(raw)
    assert dev.welch_rows(nbytes, chunk, nperseg) == rows
    if shape in wr.MIN_SPLIT:                                           # the shape reaches what it names on this device
        split = dev.welch_workspace(nbytes, chunk, nperseg) // (rows * nperseg * 4)
        print(f"nperseg {nperseg}, {shape}: {nseg} segments per chunk in {split} workgroups")
        assert split >= wr.MIN_SPLIT[shape]
    label = f"nperseg {nperseg}, {shape} ({nseg} segments), {klass}" + (f" {name}" if name else "")
    truth = wr.reference(nperseg, shape, klass, name)
    psd, db = launch(dev, cap, nbytes, chunk, nperseg, rows, want_db=True)
    held(label, np.fft.ifftshift(psd, axes=1), truth, tol, nseg == 1)
    again = launch(dev, cap, nbytes, chunk, nperseg, rows)
    assert again.tobytes() == psd.tobytes(), "a second launch gives the same bytes"
    if shape != "odd":
        return
    # the unshifted row is the same bits
    flat = launch(dev, cap, nbytes, chunk, nperseg, rows, shift=False)
    assert np.fft.fftshift(flat, axes=1).tobytes() == psd.tobytes()
    # the dB row: 10 log10(truth + 1e-15), the tolerance carried through the logarithm (for a bin at its row's level that
    # is tol * 10 / ln 10), plus two float32 spacings at the value
    den = wr.denominators(truth)
    hi = 10.0 * np.log10(truth + tol * den + 1e-15)
    lo = 10.0 * np.log10(np.maximum(truth - tol * den, 0.0) + 1e-15)
    want_db = 10.0 * np.log10(truth + 1e-15)
    slack = 2.0 * np.spacing(np.abs(want_db).astype(np.float32)).astype(np.float64)
    got_db = np.fft.ifftshift(db, axes=1).astype(np.float64)
    over = np.maximum(got_db - (hi + slack), (lo - slack) - got_db)
    print(f"{label}: dB row off by at most {np.max(np.abs(got_db - want_db)):.2e} dB, bound {np.max(hi - lo) / 2 + slack.max():.2e}")
    assert np.all(np.isfinite(got_db)) and over.max() <= 0.0, label
    # one sample later: a 2-byte-aligned base
    held(label + ", base + 2 bytes", launch(dev, cap.ptr + 2, nbytes, chunk, nperseg, rows, shift=False),
         wr.reference(nperseg, shape, klass, name, "base+2"), tol, False)
    # the other unpack convention
    try:
        dev.set_unpack(*wr.CONVENTIONS[1])
        other = launch(dev, cap, nbytes, chunk, nperseg, rows, shift=False)
    finally:
        dev.set_unpack(*wr.CONVENTIONS[0])
    held(label + ", unpack (128, 1/128)", other, wr.reference(nperseg, shape, klass, name, "unpack 128"), tol, False)
    assert launch(dev, cap, nbytes, chunk, nperseg, rows).tobytes() == psd.tobytes(), "the convention is restored"
    # two different captures in one launch: each gets the bytes of its own launch
    raw2 = wr.capture(nperseg, shape, "large_dc" if klass == "modest" else "modest")
    assert raw2.size == raw.size and not np.array_equal(raw2, raw)
    cap2 = dev.alloc(raw2.size).upload(raw2)
    alone2 = launch(dev, cap2, nbytes, chunk, nperseg, rows)
    outs = [dev.alloc(4 * rows * nperseg), dev.alloc(4 * rows * nperseg)]
    dev.welch_batch_dev([cap, cap2], nbytes, chunk, nperseg, wr.FS, outs)
    dev.synchronize()
    assert outs[0].download(np.float32).tobytes() == psd.tobytes()
    assert outs[1].download(np.float32).tobytes() == alone2.tobytes() != psd.tobytes()
