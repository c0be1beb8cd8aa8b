"""CPU side of the cancellers' extreme tests (tests/cancel_extremes/test_round6_gpu.py): everything the GPU file takes for
granted about the inputs of tests/cancel_extremes_inputs.py -- that the closed form is the definition, how far the
complex64 computation strays from float64 on full-scale inputs under |W| up to 4, that no power lies near its threshold,
which cases sit on rounding ties by construction -- is computed here from the restatements alone, printed, and held to
what the inputs module records.  No GPU call is made."""
import numpy as np

import cancel2_restatement as c2
import cancel_extremes_inputs as ce
import cancel_restatement as cr
import csd_restatement as cs
import excise_restatement as er
import extremes_inputs as xi
from gpsjam import _bands, coherence


def recorded_is_measured(recorded, measured, what):
    """A recorded figure is at least what is measured here and at most twice it."""
    assert measured <= recorded <= 2.0 * measured, (what, recorded, measured)


# ------------------------------------------------------------------------------------------- 1. constant weights
def test_the_closed_form_is_the_definition_and_the_clamp_decides_its_bytes():
    rails, e_worst = [], 0.0
    for nfft in ce.CLOSED_NFFT:
        rec_worst = 0.0
        for c, offset, scale in ce.CLOSED_CASES + ce.CLOSED_CASES2:
            what = (c, offset, nfft)
            value, out = ce.closed_value(c, offset, nfft), ce.closed_bytes(c, offset, nfft)
            (w64, d_f), (w32, _) = ce.closed_reference(c, offset, scale, nfft), ce.closed_reference(c, offset, scale, nfft, True)
            assert np.array_equal(value, np.rint(value)) and er.tie_distance(value).min() >= ce.CLOSED_TIE_MIN, what
            assert value.size == w64.value.size and np.max(np.abs(w64.value - value)) < 1e-9, what
            assert out.tobytes() == w64.out.tobytes() == w32.out.tobytes(), (what, "clip(rint(closed form)) is the restatement's bytes")
            assert not w64.cut.any() and np.all(d_f > 0) and np.all(w64.records["total_in"] > 0)
            low, high = float(np.mean(value < 0)), float(np.mean(value > 255))
            rails.append((low, high))
            assert min(low, high) >= ce.CLOSED_RAIL_SHARE_MIN, (what, low, high)
            e_worst = max(e_worst, float(np.max(np.abs(w32.value - value))))
            rec_worst = max(rec_worst, ce.record_ratio(w32.records, w64.records, d_f))
        print(f"closed form, {nfft} points: complex64 records within {rec_worst:.3e} of the float64 ones "
              f"(recorded {ce.CLOSED_REC32_MEASURED[nfft]:.3e}, tolerance {ce.closed_record_tol(nfft):.2e})")
        recorded_is_measured(ce.CLOSED_REC32_MEASURED[nfft], rec_worst, ("closed records", nfft))
    print(f"closed form: {100 * min(min(r) for r in rails):.0f} % to {100 * max(max(r) for r in rails):.0f} % of the values are clamped at "
          f"each end; the complex64 value is at most {e_worst:.1e} from the integer")
    assert e_worst < ce.CLOSED_TIE_MIN
    # the parity rule: c = 3 under 127.5 puts every value on a tie
    assert not er.tie_distance(ce.closed_value(3.0 + 0.0j, 127.5, 256)).any()
    # three equal sets are one set
    for cases, n_aux in ((ce.CLOSED_CASES, 1), (ce.CLOSED_CASES2, 2)):
        c, offset, scale = cases[ce.CLOSED_THREE_SETS]
        raws = ce.closed_captures()[:1 + n_aux]
        three = cr.cancel_aux(raws[0], ce.FIRSTS[0], ce.aux_of(raws), ce.closed_weights(c, 256, 3), None, 256, ce.CLOSED_SAMPLES,
                              ce.FRAMES_PER_SET, offset, scale)
        assert three.out.tobytes() == ce.closed_bytes(c, offset, 256).tobytes()
        assert three.records.tobytes() == ce.closed_reference(c, offset, scale, 256)[0].records.tobytes()


# ------------------------------------------------------------------------------ 2. extreme captures, |W| up to 4
def test_the_extreme_cases_are_what_the_issue_lists():
    assert len(ce.PAIRS) >= 9 and len(ce.TRIPLES) >= 5 and ce.EXTREME_NFFT == (16, 64, 1024, 4096)
    assert all(set(names) <= set(xi.NAMES) for names in ce.PAIRS + ce.TRIPLES)
    assert all(t[:2] in ce.PAIRS for t in ce.TRIPLES), "every triple is a pair with a third capture added"
    assert any(t[1] == t[2] for t in ce.TRIPLES) and any(t[0].startswith("constant") for t in ce.TRIPLES)
    assert ce.EXTREME_SAMPLES + max(ce.FIRSTS) == xi.SAMPLES
    for nfft in ce.EXTREME_NFFT:
        for n_aux in (1, 2):
            w = ce.extreme_weights(n_aux, nfft)
            assert w.dtype == np.complex64 and w.shape[0] == ce.extreme_sets(nfft) and w.shape[-1] == nfft
            mod = np.abs(w)
            assert 3.9 < mod.max() <= ce.W_MAX and np.mean(mod > 1.0) > 0.7 and abs(np.mean(np.angle(w))) < 0.1


def test_no_power_lies_near_its_threshold():
    for nfft in ce.EXTREME_NFFT:
        worst, where = np.inf, None
        for names, n, offset, scale, kind in ce.extreme_cases():
            if n != nfft or kind != "cut":
                continue
            what = (names, nfft, offset)
            share, recorded = ce.threshold_share(names, nfft, offset)
            thr = ce.extreme_threshold(names, nfft, offset, scale, kind)
            want, _ = ce.extreme_reference(names, nfft, offset, scale, kind)
            margin = er.threshold_margin(want.power, thr)
            assert share >= ce.THRESHOLD_FLOOR and np.all(thr >= ce.THRESHOLD_FLOOR * want.power.max()), what
            assert margin >= cr.NEAR_TIE and abs(margin - recorded) <= 0.01 * recorded, (what, margin, recorded)
            assert want.cut.any() and not want.cut.all(), (what, "the mask is neither empty nor full")
            # the margin is wide enough for complex64: its mask is the float64 one
            w32, _ = ce.extreme_reference(names, nfft, offset, scale, kind, True)
            assert np.array_equal(w32.cut, want.cut), what
            if margin < worst:
                worst, where = margin, what
        print(f"{nfft} points: smallest threshold margin {worst:.2e} at {where}")


def test_the_tie_band_the_record_tolerance_and_the_cases_under_the_cap():
    under, over_least = set(), np.inf
    silent = dead = clamped = 0
    for nfft in ce.EXTREME_NFFT:
        e_worst, e_where, r_worst, r_where, s_worst, s_where = 0.0, None, 0.0, None, 0.0, None
        for names, n, offset, scale, kind in ce.extreme_cases():
            if n != nfft:
                continue
            what = (names, nfft, offset, kind)
            (w64, d_f), (w32, _) = ce.extreme_reference(names, nfft, offset, scale, kind), ce.extreme_reference(names, nfft, offset, scale, kind, True)
            e = float(np.max(np.abs(w32.value - w64.value)))
            r = ce.record_ratio(w32.records, w64.records, d_f)
            if e > e_worst:
                e_worst, e_where = e, what
            if r > r_worst:
                r_worst, r_where = r, what
            share = ce.tie_share(w64.value, nfft)
            if share <= ce.TIE_SHARE_MAX:
                under.add(what)
                if share > s_worst:
                    s_worst, s_where = share, what
            else:
                over_least = min(over_least, share)
            assert ce.under_the_cap(names, nfft, offset, kind) == (share <= ce.TIE_SHARE_MAX), (what, share)
            # complex64 passes the GPU's own comparison
            diff = np.abs(w32.out.astype(np.int16) - w64.out.astype(np.int16))
            assert diff.max() <= 1 and not diff[w64.lo:w64.hi][er.tie_distance(w64.value) > ce.tie_band(nfft)].any(), what
            assert not ce.record_errors(w32.records, w64.records, d_f, ce.record_tol(nfft)), what
            assert np.array_equal(w32.records["n_excised"], w64.records["n_excised"]), what
            # frames without power: nothing comes of nothing
            quiet = w64.records["total_in"] == 0
            none = quiet & (d_f == 0)
            silent, dead = silent + int(quiet.sum()), dead + int(none.sum())
            assert not quiet.any() or (offset == 128.0 and names[0] == "one impulse"), what
            for rec in (w64.records, w32.records):
                assert not rec["total_in"][quiet].any() and not rec["total"][none].any() and not rec["removed"][none].any(), what
                assert not rec["n_excised"][none].any(), what
            h = nfft // 2
            for f in np.flatnonzero(none[:-1] & none[1:]):              # hop f + 1 is the sum of frames f and f + 1
                assert np.all(w64.out[2 * (f + 1) * h:2 * (f + 2) * h] == 128), what
            clamped += int(np.sum((w64.value < -0.5) | (w64.value > 255.5)))
        print(f"{nfft} points: |complex64 - float64| {e_worst:.3e} at {e_where} (recorded {ce.E32_MEASURED[nfft]:.3e}, band "
              f"{ce.tie_band(nfft):.2e}); records {r_worst:.3e} at {r_where} (recorded {ce.REC32_MEASURED[nfft]:.3e}, tolerance "
              f"{ce.record_tol(nfft):.2e}); largest share in the band of a case under the cap {s_worst:.2e} at {s_where}")
        recorded_is_measured(ce.E32_MEASURED[nfft], e_worst, ("E32", nfft))
        recorded_is_measured(ce.REC32_MEASURED[nfft], r_worst, ("records", nfft))
    listed = {(names, *case) for names, cases in ce.UNDER_THE_CAP.items() for case in cases}
    print(f"under the cap: {len(under)} of {len(ce.extreme_cases())} cases; the smallest share over it is {over_least:.2e}")
    print(f"{silent} frames without power in a, {dead} of them without any power at all; {clamped} values leave [0, 255] before rounding")
    assert under == listed, (sorted(under - listed), sorted(listed - under))
    assert silent > 0 and dead > 0 and clamped > 0
    # a band of half-width b holds 2 b of evenly spread values: with these bands no noise-like output can stay under the cap
    assert all(2.0 * ce.tie_band(nfft) > ce.TIE_SHARE_MAX for nfft in ce.EXTREME_NFFT)
    assert all(not any(n in xi.RANDOM_NAMES for n in names) or names == ("uniform bytes", "one impulse") for names in ce.UNDER_THE_CAP)


# ------------------------------------------------------------------------------ 3. past byte 2^32, 4. size_t's ends
def test_the_far_window_and_the_set_inputs():
    raw = ce.far_capture()
    assert raw.size == 2 * (ce.FIRSTS[2] + ce.FAR_SAMPLES) and 2 * ce.FAR_S0 + raw.size <= ce.FAR_BYTES
    assert 2 * ce.FAR_S0 == 2 ** 32 and raw.size % 2 == 0 and not raw.flags.writeable
    for n_aux, mod in ((1, cr), (2, c2)):
        for nfft in ce.FAR_NFFT:
            want = ce.far_reference(n_aux, nfft)
            margin = er.threshold_margin(want.power, ce.far_threshold(n_aux, nfft))
            share = float(np.mean(er.tie_distance(want.value) <= mod.TIE_BAND))
            print(f"far window, {n_aux} auxiliaries, {nfft} points: threshold margin {margin:.2e}, share in the parity band {share:.2e}")
            assert margin >= cr.NEAR_TIE and share <= cr.TIE_SHARE_MAX and want.cut.any() and not want.cut.all()
        nf = er.frames_loop(cr.PARITY_SAMPLES, ce.SET_NFFT)
        w = ce.per_frame_weights(n_aux, ce.SET_NFFT, nf, 3)
        assert w.shape[0] == nf + 3 and np.isnan(w[nf:].view(np.float32)).all() and np.isfinite(w[:nf].view(np.float32)).all()
        assert cr.set_of(nf, 1, nf + 3).max() == nf - 1, "set(f) <= F - 1: the sets behind the F-th are never read"
        assert len({w[f].tobytes() for f in range(nf)}) > 1
    # frames_per_set at size_t's end: every frame is in set 0
    assert max(min(f // (2 ** 64 - 1), 3 - 1) for f in range(255)) == 0 and cr.set_of(255, 1, 1).max() == 0


# ------------------------------------------------------------------------------ 5. one degenerate chain
def test_a_repeated_auxiliary_falls_back_to_one_weight():
    """cancel_weights2 on the sums of (a, b, b): det = 0 in every cell, every flagged cell falls back to b, W2 = 0."""
    a, b, _ = c2.parity_triple()
    nfft, m = 256, 16
    ab = cs.as_result(*(v.astype(t) for v, t in zip(cs.csd(a, b, nfft, nfft, m), (np.float32, np.float32, np.complex64, np.float32))), nfft, nfft, m)
    bb = cs.as_result(*(v.astype(t) for v, t in zip(cs.csd(b, b, nfft, nfft, m), (np.float32, np.float32, np.complex64, np.float32))), nfft, nfft, m)
    flagged = np.abs(_bands.signed_bins(nfft)) > 1
    w = coherence.cancel_weights2(coherence.SpectralMatrix(ab, ab, bb, (0, 0)), flagged)
    assert w.shape == (len(ab), 2, nfft) and len(ab) >= 8 and not w[:, 1].any()
    assert np.all(w[:, 0][:, flagged] != 0) and not w[:, 0][:, ~flagged].any()
    assert w[:, 0].tobytes() == coherence.cancel_weights(ab, coherence.Detection(flagged, 0.0, 1e-6)).tobytes()
