"""The result vector (gj_pack_result_dev / gj_pack_results_dev, the last stage of gj_split_combine_dev) and the part
vector (gj_pack_part_dev) restated in numpy from the layouts in include/gpsjam.h -- test infrastructure, never imported
by the product.

    result: double[40 + n_chunks + nperseg + 5 pair_capacity] = header | float32 power map | mean spectrum | pair block
    part:   double[40 + chunk_cap + 2 tile_cap + 5 pair_cap + ceil(rows_cap nperseg / 2)]
            = header | chunk powers | (sum, first) tile records | pair block | PSD rows as float32, two per slot

Everything but the mean spectrum is a copy or an exact conversion and is compared as BYTES.  The mean spectrum is stated as
the float64 mean of the float32 rows; the kernel adds in float32 (16 row lanes, each a strided sum, then the 16 partial
sums, then one division) and is held to `spectrum_bound`, which is derived from that order and from nothing measured."""
import numpy as np

HEADER = 40
PAIR_FIELDS = 5
LAG_INVALID = -(1 << 31)
ONSET_T = np.dtype([("start", "<i8"), ("noise", "<f4"), ("thr", "<f4"), ("hit", "<f4"), ("before", "<f4"), ("guard", "<i8")])
AMP_T = np.dtype([("first", "<i8"), ("count", "<u8"), ("sum", "<f8"), ("mean", "<f4"), ("reserved", "<f4")])
AMP_PART_T = np.dtype([("first", "<i8"), ("count", "<u8"), ("sum", "<f8"), ("tail", "<f8")])
TILE_T = np.dtype([("sum", "<f8"), ("first", "<i8")])
assert ONSET_T.itemsize == AMP_T.itemsize == AMP_PART_T.itemsize == 32 and TILE_T.itemsize == 16

U = 2.0 ** -24     # unit roundoff of float32


def result_len(n_chunks: int, nperseg: int, pair_capacity: int) -> int:
    return HEADER + n_chunks + nperseg + PAIR_FIELDS * pair_capacity


def part_len(chunk_cap: int, tile_cap: int, rows_cap: int, nperseg: int, pair_cap: int) -> int:
    return HEADER + chunk_cap + 2 * tile_cap + PAIR_FIELDS * pair_cap + (rows_cap * nperseg + 1) // 2


def _record(rec, dtype) -> np.ndarray:
    """A 32-byte record as the four doubles the header carries as they are."""
    return np.frombuffer(np.asarray(rec, dtype).tobytes(), "<f8")


def _pair_block(n_pairs, pair_cap, pairs, lags, peaks, margins) -> np.ndarray:
    block = np.zeros((pair_cap, PAIR_FIELDS), np.float64)
    if n_pairs:
        pr = np.asarray(pairs, np.int32).reshape(-1, 2)[:n_pairs]
        block[:n_pairs, 0], block[:n_pairs, 1] = pr[:, 0], pr[:, 1]
        block[:n_pairs, 2] = np.asarray(lags, np.int32)[:n_pairs]
        block[:n_pairs, 3] = np.asarray(peaks, np.float32)[:n_pairs]
        block[:n_pairs, 4] = np.asarray(margins, np.float32)[:n_pairs]
    return block.reshape(-1)


def mean_spectrum(psd, rows: int, nperseg: int) -> np.ndarray:
    """The float64 mean over the float32 rows; zeros when there is no row."""
    if rows == 0:
        return np.zeros(nperseg, np.float64)
    return np.asarray(psd, np.float32).reshape(-1)[:rows * nperseg].reshape(rows, nperseg).astype(np.float64).mean(axis=0)


def kernel_order_spectrum(psd, rows: int, nperseg: int) -> np.ndarray:
    """The float32 order of the packing kernel: lane j adds rows j, j + 16, ... in turn, the 16 partial sums are added
    in lane order, the total is divided by float32(rows)."""
    if rows == 0:
        return np.zeros(nperseg, np.float32)
    p = np.asarray(psd, np.float32).reshape(-1)[:rows * nperseg].reshape(rows, nperseg)
    t = np.zeros(nperseg, np.float32)
    for j in range(16):
        s = np.zeros(nperseg, np.float32)
        for r in range(j, rows, 16):
            s = s + p[r]
        t = t + s
    return t / np.float32(rows)


def spectrum_bound(rows: int) -> float:
    """Relative bound on |kernel - float64 mean| per bin for non-negative rows: a lane's sum of m = ceil(rows / 16) terms is
    within (m - 1) u, the sum of the 16 partial sums within 15 u, the division within u; the two further u cover the
    higher-order terms: (1 + u)^(m + 15) <= 1 + (m + 17) u for every m below 8000.  u = 2^-24."""
    return (-(-rows // 16) + 17) * U


def spectrum_ratio(got, psd, rows: int, nperseg: int) -> float:
    """Largest |got - float64 mean| / (bound x mean) over the bins (0 when there is no row and got is all zero)."""
    want = mean_spectrum(psd, rows, nperseg)
    got = np.asarray(got, np.float64)
    if rows == 0:
        return 0.0 if not got.any() else np.inf
    assert np.all(want > 0)
    return float(np.max(np.abs(got - want) / (spectrum_bound(rows) * want)))


def pack_result(n_chunks, power, stats, amp, onset, psd, rows, nperseg, rank, n_pairs, pair_cap, pairs=None, lags=None,
                peaks=None, margins=None, spectrum=None) -> np.ndarray:
    """gj_pack_result_dev.  `amp` / `onset` are AMP_T / ONSET_T records; `spectrum` replaces the float64 mean (a caller
    that compares with another packer hands both the same one)."""
    amp, onset = np.asarray(amp, AMP_T).reshape(()), np.asarray(onset, ONSET_T).reshape(())
    stats = np.asarray(stats, np.float32)
    h = np.zeros(HEADER, np.float64)
    h[0] = n_chunks
    h[1:4] = stats[:3]
    h[4], h[5], h[6] = amp["first"], amp["count"], amp["mean"]
    h[7] = onset["start"]
    h[8] = 0.0 if rank == 0 else LAG_INVALID
    h[10] = onset["noise"]
    h[11], h[12], h[13], h[14], h[15] = rows, nperseg, rank, n_pairs, pair_cap
    h[16], h[17], h[18], h[19] = onset["hit"], onset["before"], onset["guard"], onset["thr"]
    h[20], h[22] = rank, 1.0
    h[26] = amp["sum"]
    h[32:36] = _record(onset, ONSET_T)
    h[36:40] = _record(amp, AMP_T)
    spec = mean_spectrum(psd, rows, nperseg) if spectrum is None else np.asarray(spectrum, np.float64)
    assert spec.shape == (nperseg,)
    out = np.concatenate([h, np.asarray(power, np.float32)[:n_chunks].astype(np.float64), spec,
                          _pair_block(n_pairs, pair_cap, pairs, lags, peaks, margins)])
    assert out.size == result_len(n_chunks, nperseg, pair_cap)
    return out


def pack_part(*, rank, antenna, part, parts, first_chunk, n_chunks, chunk_cap, first_row, rows, rows_cap, first_tile, n_tiles,
              tile_cap, first_sample, nperseg, n_pairs, pair_cap, power, amp, onset, tiles, psd, pairs=None, lags=None,
              peaks=None, margins=None) -> np.ndarray:
    """gj_pack_part_dev.  `amp` is an AMP_PART_T record, `tiles` TILE_T records; counts below their capacities leave
    zeros behind them."""
    amp, onset = np.asarray(amp, AMP_PART_T).reshape(()), np.asarray(onset, ONSET_T).reshape(())
    h = np.zeros(HEADER, np.float64)
    h[0] = n_chunks
    h[4], h[5] = amp["first"], amp["count"]
    h[7] = onset["start"]
    h[8] = LAG_INVALID
    h[10] = onset["noise"]
    h[11], h[12], h[13], h[14], h[15] = rows, nperseg, rank, n_pairs, pair_cap
    h[16], h[17], h[18], h[19] = onset["hit"], onset["before"], onset["guard"], onset["thr"]
    h[20], h[21], h[22], h[23], h[24], h[25] = antenna, part, parts, first_chunk, first_row, first_sample
    h[26], h[27], h[28], h[29] = amp["sum"], amp["tail"], n_tiles, first_tile
    h[32:36] = _record(onset, ONSET_T)
    h[36:40] = _record(amp, AMP_PART_T)
    pw = np.zeros(chunk_cap, np.float64)
    pw[:n_chunks] = np.asarray(power, np.float32)[:n_chunks]
    tl = np.zeros(2 * tile_cap, np.float64)
    tl[:2 * n_tiles] = np.frombuffer(np.asarray(tiles, TILE_T)[:n_tiles].tobytes(), "<f8")
    rf = np.zeros(2 * ((rows_cap * nperseg + 1) // 2), np.float32)
    if rows:
        rf[:rows * nperseg] = np.asarray(psd, np.float32).reshape(-1)[:rows * nperseg]
    out = np.concatenate([h, pw, tl, _pair_block(n_pairs, pair_cap, pairs, lags, peaks, margins),
                          np.frombuffer(rf.tobytes(), "<f8")])
    assert out.size == part_len(chunk_cap, tile_cap, rows_cap, nperseg, pair_cap)
    return out


# --------------------------------------------------------------------------------------- inputs
def records(seed: int, first_index=None):
    """An amplitude record, an onset record and an amplitude-part record with every field set to a value of its own."""
    rng = np.random.default_rng(31_000 + seed)
    first = int(rng.integers(0, 1 << 40)) if first_index is None else first_index
    amp = np.array((first, int(rng.integers(1, 1 << 41)), float(rng.uniform(1e3, 1e9)), rng.uniform(0.01, 1.2), 0.0), AMP_T)
    start = int(rng.integers(0, 1 << 40))
    onset = np.array((start, rng.uniform(1, 900), rng.uniform(50, 45000), rng.uniform(1e-7, 3), rng.uniform(1e-7, 1),
                      start - int(rng.integers(0, 3))), ONSET_T)
    part = np.array((first, int(rng.integers(1, 1 << 41)), float(rng.uniform(1e3, 1e9)), float(rng.uniform(0, 1e5))), AMP_PART_T)
    return amp, onset, part


def psd_rows(rows: int, nperseg: int, seed: int) -> np.ndarray:
    """Positive rows with a wide range: 10 ** uniform(-12, -3)."""
    rng = np.random.default_rng(32_000 + seed)
    return (10.0 ** rng.uniform(-12.0, -3.0, (max(rows, 1), nperseg))).astype(np.float32)[:rows]


def pair_table(n: int, seed: int):
    """(pairs int32[2n], lags int32[n], peaks float32[n], margins float32[n]); one lag is GJ_LAG_INVALID when n > 1."""
    rng = np.random.default_rng(33_000 + seed)
    pairs = rng.integers(0, 8, 2 * max(n, 1)).astype(np.int32)
    lags = rng.integers(-5000, 5000, max(n, 1)).astype(np.int32)
    if n > 1:
        lags[1] = LAG_INVALID
    return pairs, lags, rng.uniform(1, 1e9, max(n, 1)).astype(np.float32), rng.uniform(0, 1, max(n, 1)).astype(np.float32)


BASE = dict(nperseg=1024, rows=10, n_chunks=625, pair_cap=3, n_pairs=2, rank=0, first_index=None)


def result_cases():
    """name -> parameters: one factor varied at a time around BASE, then a dozen mixed cases."""
    out = {"base": dict(BASE)}
    for v in (16, 32, 64, 128, 4096):
        out[f"nperseg {v}"] = dict(BASE, nperseg=v)
    for v in (0, 1, 15, 16, 17, 31, 33, 263):
        out[f"rows {v}"] = dict(BASE, rows=v)
    for v in (1, 983, 984, 985, 262_150):            # 40 + 984 = 1024: one copy block exactly; 262 150: the blocks stride
        out[f"n_chunks {v}"] = dict(BASE, n_chunks=v)
    for cap, n in ((0, 0), (3, 0), (3, 3), (28, 28)):
        out[f"pairs {n} of {cap}"] = dict(BASE, pair_cap=cap, n_pairs=n)
    out["rank 2"] = dict(BASE, rank=2)
    out["nothing above the amplitude threshold"] = dict(BASE, first_index=-1)
    rng = np.random.default_rng(34_000)
    for k in range(12):
        cap = int(rng.choice([0, 1, 3, 28]))
        out[f"mixed {k}"] = dict(nperseg=int(rng.choice([16, 32, 64, 128, 256, 1024, 4096])),
                                 rows=int(rng.choice([0, 1, 15, 16, 17, 31, 33, 47, 263])),
                                 n_chunks=int(rng.choice([1, 2, 983, 984, 985, 625, 4097, 70_000])), pair_cap=cap,
                                 n_pairs=int(rng.integers(0, cap + 1)), rank=int(rng.choice([0, 1, 2, 7])),
                                 first_index=-1 if k % 4 == 3 else None)
    return out
