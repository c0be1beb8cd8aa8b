"""CPU side of the extreme-capture tests of the short-time kernels and the excisors (tests/extremes/test_round6_gpu.py):
the inputs of tests/extremes_inputs.py are what they are said to be, and everything the GPU tests take for granted about
them -- which frames have a tied peak bin or rate, how much room S2 has in float32 -- is computed here from the float64
restatements alone and printed.  No GPU call is made."""
import numpy as np

import chirp_restatement as cr
import excise_chirp_restatement as xr
import excise_restatement as er
import extremes_inputs as xi
import skurt_restatement as sr


def test_the_captures_are_the_recipes_at_2_to_the_15():
    for name in xi.NAMES:
        raw = xi.capture(name)
        assert raw.dtype == np.uint8 and raw.size == 2 * xi.SAMPLES and not raw.flags.writeable
        assert xi.capture(name) is raw
    assert set(np.unique(xi.capture("constant 255"))) == {255} and set(np.unique(xi.capture("constant 0"))) == {0}
    mid = xi.capture("constant 128/127")
    assert set(mid[0::2]) == {128} and set(mid[1::2]) == {127}
    ny = xi.capture("nyquist full scale")
    assert ny[:8].tolist() == [0, 255, 255, 0, 0, 255, 255, 0]
    assert len(np.unique(xi.capture("uniform bytes"))) == 256
    sat = xi.capture("saturated tone")
    assert np.mean((sat == 0) | (sat == 255)) > 0.5                       # clips hard
    burst = xi.capture("quiet then rail to rail")
    assert xi.RAIL_AT == 3 * xi.SAMPLES // 4 and set(np.unique(burst[2 * xi.RAIL_AT:])) == {0, 255}
    assert np.all(np.abs(burst[:2 * xi.RAIL_AT].astype(int) - 128) < 16)
    imp = xi.capture("one impulse")
    assert xi.IMPULSE_AT & 1 and abs(xi.IMPULSE_AT - xi.SAMPLES // 2) <= 1
    assert np.flatnonzero(imp != 128).tolist() == [2 * xi.IMPULSE_AT] and imp[2 * xi.IMPULSE_AT] == 255


def test_ridge_ties_are_where_they_must_be():
    """Constant and Nyquist captures: no tied frame (three bins, the middle one four times the others).  One impulse:
    under offset 128 exactly the frames that hold it (a flat spectrum; every other frame is without power), under
    127.5 none (the DC of 0.5 (1 + j) decides).  The captures of random draws: a few chance ties, under the cap."""
    worst = 0.0
    for name in xi.NAMES:
        counts = []
        for nfft in xi.RIDGE_NFFT:
            for hop in xi.hops(nfft):
                for offset, scale in xi.CONVENTIONS:
                    rec, margin = xi.ridge_reference(name, nfft, hop, offset, scale)
                    tied = xi.ridge_not_clear(name, nfft, hop, offset, scale)
                    what = (name, nfft, hop, offset)
                    if name in xi.RANDOM_NAMES:
                        worst = max(worst, tied.size / rec.size)
                        assert tied.size / rec.size <= xi.CHANCE_TIE_SHARE_CAP, what
                    elif name == "one impulse" and offset == 128.0:
                        assert np.array_equal(tied, xi.frames_with_the_impulse(nfft, hop, rec.size)) and tied.size >= 1, what
                        dead = np.ones(rec.size, bool)
                        dead[tied] = False
                        assert not rec["total"][dead].any() and np.all(rec["total"][tied] > 0), what
                    else:
                        assert tied.size == 0, what
                        assert name == "one impulse" or margin.min() > 0.7, what
                    if tied.size:
                        counts.append((nfft, hop, offset, tied.tolist()[:6]))
        print(f"ridge, {name}: frames that are not clear (nfft, hop, offset, frames) {counts}")
    print(f"ridge: largest share of chance ties {worst:.2e} (cap {xi.CHANCE_TIE_SHARE_CAP:.1e})")


def test_chirp_ties_are_where_they_must_be():
    """At the single rate 0 the ties are the ridge's.  At any other rate a constant, the Nyquist pattern and -- under
    offset 127.5, where every frame carries a DC -- the impulse capture have a spectrum that is symmetric in k, so EVERY
    frame ties bins k and -k exactly: those captures test the candidate rule and the values, not the choice.  The
    captures of random draws stay under the cap."""
    worst, where = 0.0, None
    for name in xi.NAMES:
        shares = {}
        for nfft in xi.CHIRP_NFFT:
            for hop in xi.hops(nfft):
                for rates in xi.chirp_rate_sets(nfft):
                    for offset, scale in xi.CONVENTIONS:
                        scan = xi.chirp_reference(name, nfft, hop, rates, offset, scale)
                        tied = xi.chirp_not_clear(name, nfft, hop, rates, offset, scale)
                        what = (name, nfft, hop, rates, offset)
                        share = tied.size / scan.records.size
                        shares[what[1:]] = tied.size
                        if rates == (0, 1, 1):
                            assert np.array_equal(tied, xi.ridge_not_clear(name, nfft, hop, offset, scale)), what
                            rec, _ = xi.ridge_reference(name, nfft, hop, offset, scale)
                            assert np.array_equal(scan.records["peak_bin"], rec["peak_bin"]) and np.array_equal(scan.records["peak"], rec["peak"])
                        if name in xi.RANDOM_NAMES:
                            if share > worst:
                                worst, where = share, (what, tied.size, scan.records.size)
                            assert share <= xi.CHANCE_TIE_SHARE_CAP, what
                        elif name == "one impulse" and offset == 128.0:
                            assert np.array_equal(tied, xi.frames_with_the_impulse(nfft, hop, scan.records.size)), what
                        # a tie of two RATES would make rate_index a matter of rounding on every frame: never structural
                        if name not in xi.RANDOM_NAMES and not (name == "one impulse" and offset == 128.0):
                            live = scan.records["peak"] > 0
                            assert name == "one impulse" or scan.rate_margin[live].min() >= cr.NEAR_TIE, what
        print(f"chirp, {name}: not clear in {sum(1 for v in shares.values() if v)} of {len(shares)} cases, {sum(shares.values())} frames in all")
    print(f"chirp: largest share of chance ties {worst:.2e} at {where} (measured {xi.CHANCE_TIE_SHARE_MEASURED:.1e}, cap {xi.CHANCE_TIE_SHARE_CAP:.1e})")
    assert worst <= xi.CHANCE_TIE_SHARE_MEASURED * 1.01


def test_kurtosis_cases_and_the_room_of_s2_in_float32():
    for nfft in xi.RIDGE_NFFT:
        ms = {m for _, m in xi.sk_cases(nfft)}
        assert {2, 5} <= ms, nfft
        assert (64 in ms) == (nfft <= 512), nfft                       # 63 hops and a frame inside 2^15 samples
    worst, where = 0.0, None
    for name in xi.NAMES:
        for nfft in xi.RIDGE_NFFT:
            for offset, scale in xi.CONVENTIONS:
                for hop, m in xi.sk_cases(nfft):
                    _, s2, _ = sr.sums_of(xi.frame_powers(name, nfft, hop, offset, scale), m)
                    if s2.max() > worst:
                        worst, where = float(s2.max()), (name, nfft, hop, m, offset)
    fmax = float(np.finfo(np.float32).max)
    lsb4 = 128.0 ** 4                                                   # the kernel accumulates in LSB units: P / scale^2
    print(f"kurtosis: largest S2 {worst:.3e} at {where}; in LSB units at most {worst * lsb4:.3e}; float32 holds {fmax:.3e}: "
          f"a factor of {fmax / (worst * lsb4):.1e} to spare")
    assert worst * lsb4 < fmax / 1e6


def test_excisor_identity_in_complex64():
    """Nothing notched (+inf): the complex64 restatement reproduces every byte of all eight captures under both
    conventions, for the plain excisor and for the chirp excisor at every rate of the identity runs, and every value
    is an integer to within 0.01 (the issue asks for 0.49 from every half-integer)."""
    worst, where = 0.0, None
    for name in xi.NAMES:
        raw = xi.capture(name)
        body = raw[2 * xi.FIRST:]
        for nfft in xi.CHIRP_NFFT:
            inf = np.full(nfft, np.inf, np.float32)
            nf = er.frames_loop(xi.SAMPLES - xi.FIRST, nfft)
            for offset, scale in xi.CONVENTIONS:
                runs = [("plain", er.excise(raw, inf, nfft, xi.FIRST, None, offset, scale, single=True))]
                runs += [(q, xr.excise_chirp(raw, inf, np.full(nf, q), nfft, xi.FIRST, None, offset, scale, single=True))
                         for q in xi.chirp_identity_rates(nfft)]
                for kind, got in runs:
                    assert got.out.tobytes() == body.tobytes(), (name, nfft, offset, kind)
                    assert not got.records["n_excised"].any()
                    dev = float(np.max(np.abs(got.value - np.rint(got.value))))
                    if dev > worst:
                        worst, where = dev, (name, nfft, offset, kind)
                    assert er.tie_distance(got.value).min() >= 0.49
    print(f"identity in complex64: every byte reproduced; the largest distance of a value from its integer is {worst:.2e} at {where}")
    assert worst < 0.01


def test_notch_cases_stay_inside_the_tie_share_cap_and_E_is_what_the_band_rests_on():
    e_worst, e_where, s_worst, s_where = 0.0, None, 0.0, None
    clipped = 0
    kinds = (("plain", xi.notch_cases(), xi.notch_reference, xi.NOTCH_128_ONLY, xi.NOTCH_NEVER),
             ("chirp", xi.chirp_notch_cases(), xi.chirp_notch_reference, xi.CHIRP_NOTCH_128_ONLY, xi.CHIRP_NOTCH_NEVER))
    for kind, cases, reference, only_128, never in kinds:
        for name, nfft, offset, scale in cases:
            w64, w32 = reference(name, nfft, offset, scale), reference(name, nfft, offset, scale, True)
            e = float(np.max(np.abs(w32.value - w64.value)))
            share = float(np.mean(er.tie_distance(w64.value) <= xi.TIE_BAND))
            clear = xi.frames_clear_of_the_threshold(w64, er.parity_threshold(nfft, scale))
            clipped += int(np.sum((w64.value < -0.5) | (w64.value > 255.5)))
            print(f"notch {kind}, {name}, {nfft} points, offset {offset}: E {e:.2e}, share in the band {share:.2e}, "
                  f"{int(w64.records['n_excised'].sum())} bins notched, {int(np.sum(~clear))} of {clear.size} frames have a bin within NEAR_TIE "
                  f"of the threshold")
            if e > e_worst:
                e_worst, e_where = e, (kind, name, nfft, offset)
            if share > s_worst:
                s_worst, s_where = share, (kind, name, nfft, offset)
            assert share <= xi.TIE_SHARE_CAP, (kind, name, nfft, offset, share)
            diff = np.abs(w32.out.astype(np.int16) - w64.out.astype(np.int16))
            assert diff.max() <= 1, (kind, name, nfft, offset)
            # outside the band the complex64 bytes are the float64 ones, wherever both notched the same bins
            same = np.array_equal(w32.records["n_excised"], w64.records["n_excised"])
            assert not same or not diff[w64.lo:w64.hi][er.tie_distance(w64.value) > xi.TIE_BAND].any(), (kind, name, nfft, offset)
        # every exclusion is justified: the excluded reference is over the cap
        for (name, nfft), reason in only_128.items():
            share = float(np.mean(er.tie_distance(reference(name, nfft, 127.5, 1.0 / 127.5).value) <= xi.TIE_BAND))
            assert share > xi.TIE_SHARE_CAP and reason, (kind, name, nfft, share)
            assert (name, nfft, 128.0, 1.0 / 128.0) in cases
        for (name, nfft), reason in never.items():
            for offset, scale in xi.CONVENTIONS:
                share = float(np.mean(er.tie_distance(reference(name, nfft, offset, scale).value) <= xi.TIE_BAND))
                assert share > xi.TIE_SHARE_CAP and reason, (kind, name, nfft, offset, share)
    print(f"notch: E = {e_worst:.3e} at {e_where} (E32_MEASURED {xi.E32_MEASURED:.3e}, E32 {xi.E32:.2e}, band {xi.TIE_BAND:.2e}); "
          f"largest share {s_worst:.2e} at {s_where} (cap {xi.TIE_SHARE_CAP:.2e})")
    assert e_worst <= xi.E32 and abs(e_worst - xi.E32_MEASURED) <= 0.01 * xi.E32_MEASURED
    # clipping: none of the cases above leaves [0, 255] before rounding; the clamp cases do, at both ends
    assert clipped == 0
    for nfft in xi.CLAMP_NFFT:
        w = xi.clamp_reference(nfft)
        assert w.value.max() > 255.5 and w.value.min() < -0.5, nfft
        share = float(np.mean(er.tie_distance(w.value) <= xi.TIE_BAND))
        print(f"clamp, {nfft} points: values {w.value.min():.1f} .. {w.value.max():.1f}, share in the band {share:.2e}")
        assert share <= xi.TIE_SHARE_CAP
