"""The acquisition series' bridge to the drop-in detector, on the CPU: gnss.telemetry() on a hand-made AcqSeries, and
those records replayed into an unmodified GPSAnalysisThread (GpsJammerApp/app/worker.py).  The expected events are worked
out by hand from check_jamming_conditions: F2 needs more than 40 C/N0 history entries and a C/N0 average more than 8 dB
below their median; an event is confirmed 2.5 s after its first flagged record (start_time = that record's time) and
closed 2.0 s after its first clean one (end_time = the closing record's time).

Epochs here are 256 000 samples apart at 2.048 MS/s: 0.125 s, so every elapsed time and difference is exact."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from gpsjam import gnss

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "gps-jamming_amd")
for p in (os.path.join(PKG, "skrypty"), os.path.join(PKG, "GpsJammerApp", "app")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS = 2.048e6
STRIDE = 256000
PRNS = [3, 7, 19]


def make_series(rows):
    """rows[e] = per-PRN C/N0, or None for a PRN not acquired at epoch e (its cn0 is then set to 60 dB-Hz, which must
    not leak into the telemetry)."""
    n = len(rows)
    acquired = np.array([[c is not None for c in r] for r in rows], bool)
    cn0 = np.array([[60.0 if c is None else c for c in r] for r in rows], np.float64)
    first = STRIDE * np.arange(n, dtype=np.int64)
    zi = np.zeros((n, len(PRNS)), np.int32)
    return gnss.AcqSeries(prns=list(PRNS), first_sample=first, elapsed_s=first / FS, acquired=acquired, cn0=cn0,
                          peak_ratio=np.where(acquired, 8.0, 1.5), code_index=zi, freq_index=zi + 35,
                          doppler_hz=np.zeros((n, len(PRNS))), steps=zi + 1)


CLEAN = [44.0, 45.0, 46.0]          # average 45
LOST = [None, None, None]           # average 0


def replay(series):
    import worker
    out = io.StringIO()
    with redirect_stdout(out):
        th = worker.GPSAnalysisThread([])
        for rec in gnss.telemetry(series):
            th.process_incoming_data(rec)
    return th, out.getvalue()


def test_telemetry_records():
    s = make_series([CLEAN, [36.0, None, 38.0], LOST])
    recs = list(gnss.telemetry(s))
    assert len(recs) == 3
    assert [r["elapsed_time"] for r in recs] == [0.0, 0.125, 0.25]
    assert [r["position"]["buffcnt"] for r in recs] == [0, 2 * STRIDE, 4 * STRIDE]     # bytes, not samples
    for r in recs:
        assert r["position"]["nsat"] == 0 and r["position"]["lat"] == r["position"]["lon"] == r["position"]["hgt"] == 0.0
    assert recs[0]["observations"] == [{"prn": 3, "snr": 44.0}, {"prn": 7, "snr": 45.0}, {"prn": 19, "snr": 46.0}]
    assert recs[1]["observations"] == [{"prn": 3, "snr": 36.0}, {"prn": 19, "snr": 38.0}]
    assert recs[2]["observations"] == []
    np.testing.assert_array_equal(s.cn0_avg(), [45.0, 37.0, 0.0])
    assert s.n_epochs == 3


def test_short_history_never_raises_f2():
    # 20 clean epochs, then 40 with nothing acquired: an average of 0 is not appended, so the history stays at 20 <= 40
    s = make_series([CLEAN] * 20 + [LOST] * 40 + [CLEAN] * 20)
    th, _ = replay(s)
    assert th.jamming_events == [] and not th.jamming_detected and len(th.cn0_history) == 40


@pytest.mark.parametrize("kind", ["drop_9db", "all_lost", "all_lost_with_short_gap"])
def test_replay_gives_the_predicted_event(kind):
    # epochs 0..47 clean (48 history entries, median 45); 48..79 jammed; 80..99 clean
    jam = {"drop_9db": [36.0, 36.0, None], "all_lost": LOST, "all_lost_with_short_gap": LOST}[kind]
    rows = [CLEAN] * 48 + [jam] * 32 + [CLEAN] * 20
    if kind == "all_lost_with_short_gap":
        rows[70:76] = [CLEAN] * 6              # 0.75 s clean inside the event: shorter than the 2 s clean time
    th, out = replay(make_series(rows))
    # first flagged record: epoch 48 (6.0 s) -> confirmed at epoch 68 (8.5 s); first clean record after the burst:
    # epoch 80 (10.0 s) -> closed at epoch 96 (12.0 s)
    assert th.jamming_events == [{"start_sample": 2 * 48 * STRIDE, "end_sample": 2 * 96 * STRIDE, "start_time": 6.0,
                                  "end_time": 12.0, "duration": 6.0}]
    assert out.count("Powód: Jakość/Integrity") == 1 and "Moc (Mapowana)" not in out
    assert not th.jamming_detected


def test_drop_of_7db_is_no_event():
    s = make_series([CLEAN] * 48 + [[38.0, 38.0, 38.0]] * 32 + [CLEAN] * 20)
    th, _ = replay(s)
    assert th.jamming_events == [] and not th.jamming_detected
