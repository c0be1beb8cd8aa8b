"""What the split rehearsals share (tests/test_split_gpu.py, tests/test_local_gpu.py): the scenarios, the established
single-GPU path they are held to, and the comparison, bit for bit."""
import numpy as np


def scenarios(big=False):
    """name -> (captures, parameters).  chunk_samples are chosen so that a unit (lcm of the power chunk and the PSD
    chunk) is small against the captures; G2 keeps the reference's 1-s chunk and therefore cannot be cut (one part,
    the other ranks idle: the empty-rank path)."""
    from golden import golden_inputs as gi
    from gpsjam.synth import StreamSpec, generate
    out = {}
    out["g1"] = ([gi.g1_stream()], dict(chunk_samples=32768, nperseg=256, slice_samples=1 << 12, rssi_threshold=0.0))
    out["g2"] = ([gi.g2_stream()], dict(chunk_samples=2048000, nperseg=4096, slice_samples=1 << 12, rssi_threshold=0.0))
    out["g3"] = (gi.g3_streams(), dict(chunk_samples=32768, nperseg=1024, slice_samples=1 << 12, rssi_threshold=0.1,
                                        noise_samples=20000))
    out["g4"] = (gi.g4_streams(), dict(chunk_samples=32768, nperseg=1024, slice_samples=1 << 19, rssi_threshold=0.0))
    n = 1_700_000
    syn = [generate(StreamSpec(seed=29, antenna=a, delay=d, jam_start=1_150_000, jam_end=1_600_000, jam_sigma=s), n)
           for a, (d, s) in enumerate(((0, 60.0), (5, 50.0), (-3, 55.0)))]
    syn[1] = syn[1][:-12345]                                       # captures of unequal, ragged length
    out["syn3"] = (syn, dict(chunk_samples=131072, nperseg=4096, slice_samples=1 << 15, rssi_threshold=0.05))
    if big:                                                         # 256 MiB, the reference's chunk sizes; made on the GPU
        spec = StreamSpec(seed=31, antenna=0, jam_start=70_000_000, jam_end=100_000_000, jam_sigma=60.0)
        out["big"] = ([(spec, 1 << 28)], dict(chunk_samples=2048000, nperseg=4096, slice_samples=1 << 19,
                                              rssi_threshold=0.0))
    return out


def _nbytes(src):
    return src[1] if isinstance(src, tuple) else int(src.size)


def _device_range(dev, src, b0, b1):
    """Capture bytes [b0, b1) in HBM: from a host array, or generated in place (bit-identical integer generator)."""
    import torch
    if isinstance(src, tuple):
        t = torch.zeros(b1 - b0, dtype=torch.uint8, device="cuda")
        dev.synth_dev(src[0], (b1 - b0) // 2, t, first_sample=b0 // 2)
        return t
    return torch.from_numpy(np.ascontiguousarray(src[b0:b1])).cuda()


def _collect(res, td, psd_rows):
    return dict(
        streams=[dict(power_map=r.power_map, baseline=r.baseline, threshold=r.threshold, n_above=r.n_above,
                      amp_first=r.amp_first, amp_count=r.amp_count, amp_mean=r.amp_mean, onset=r.onset,
                      onset_guard=r.onset_guard, onset_margin_hit=r.onset_margin_hit, noise_power=r.noise_power,
                      spec=r.mean_spectrum, psd=psd_rows[k]) for k, r in enumerate(res)],
        pairs=list(td.pairs), lags=list(td.lags), peaks=list(td.peaks), margins=list(td.margins))


def _single_gpu(dev, caps, kw):
    """The established single-GPU path on the whole captures: one AntennaStream per capture, then every pair over
    the slots they cut."""
    import torch
    from gpsjam import sharded
    res, slots, psd = [], [], []
    sl = kw["slice_samples"]
    for a, raw in enumerate(caps):
        st = sharded.AntennaStream(dev, _device_range(dev, raw, 0, _nbytes(raw)), nperseg=kw["nperseg"], chunk_samples=kw["chunk_samples"],
                                   slice_samples=sl, rssi_threshold=kw["rssi_threshold"],
                                   noise_samples=kw.get("noise_samples", 200000), rank=0, world_size=1)
        got = st.step()
        r, _ = got.unpack()
        res.append(r[0])
        slots.append(st.slots[0].clone())
        psd.append(st.psd[:st.rows].cpu().numpy().copy())
        st.close()
    pairs = sharded.all_pairs(len(caps))
    lags = peaks = margins = []
    if pairs:
        all_slots = torch.stack(slots).contiguous()
        d_l = torch.zeros(len(pairs), dtype=torch.int32, device="cuda")
        d_p = torch.zeros(len(pairs), dtype=torch.float32, device="cuda")
        d_m = torch.zeros(len(pairs), dtype=torch.float32, device="cuda")
        dev.xcorr_slots_dev(all_slots, all_slots.shape[1], len(caps), sl, pairs, d_l, d_p, d_m)
        torch.cuda.synchronize()
        lags, peaks, margins = d_l.tolist(), d_p.tolist(), d_m.tolist()
    td = type("TD", (), dict(pairs=pairs, lags=lags, peaks=peaks, margins=margins))
    return _collect(res, td, psd)


def _assert_identical(name, got, want):
    assert len(got["streams"]) == len(want["streams"])
    for a, (g, w) in enumerate(zip(got["streams"], want["streams"])):
        where = f"{name} antenna {a}"
        for key in ("power_map", "spec", "psd"):
            assert g[key].shape == w[key].shape, (where, key, g[key].shape, w[key].shape)
            assert g[key].tobytes() == w[key].tobytes(), (where, key, float(np.max(np.abs(g[key] - w[key]))))
        for key in ("baseline", "threshold", "n_above", "amp_first", "amp_count", "amp_mean", "onset", "onset_guard",
                    "onset_margin_hit", "noise_power"):
            assert g[key] == w[key], (where, key, g[key], w[key])
    assert got["pairs"] == want["pairs"] and got["lags"] == want["lags"], (name, got["lags"], want["lags"])
    assert got["peaks"] == want["peaks"] and got["margins"] == want["margins"], name
