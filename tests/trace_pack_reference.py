"""The packed pad-trace rows (include/attpc_engine.h, "packed pad traces", format "for64-bitplane-v1") restated in
numpy: an encoder vectorised over the rows, a decoder written row by row straight from the definition, and the rows the
CPU and GPU tests share.  Integers throughout and a unique encoding: every comparison against the library is exact
equality of bytes."""
import numpy as np

NUM_TB = 512
BLOCK = 64
BLOCKS = NUM_TB // BLOCK
MAX_WIDTH = 12
FORMAT = "for64-bitplane-v1"


def bit_length(v):
    """bit_length of every entry of a non-negative integer array (0 -> 0)."""
    v = np.asarray(v, dtype=np.int64)
    out = np.zeros(v.shape, dtype=np.int64)
    for k in range(16):
        out += (v >> k) > 0
    return out


def encode(samples):
    """samples [R, 512] in 0 .. 4095 -> (row_start [R + 1] int64, packed uint8)."""
    s = np.asarray(samples).astype(np.int64).reshape(-1, BLOCKS, BLOCK)
    if s.size and (s.min() < 0 or s.max() > 4095):
        raise ValueError("sample outside 0 .. 4095")
    n = len(s)
    lowest = s.min(axis=2) if n else np.zeros((0, BLOCKS), dtype=np.int64)
    width = bit_length(s.max(axis=2) - lowest) if n else np.zeros((0, BLOCKS), dtype=np.int64)
    base = np.minimum(lowest, 4096 - (1 << width))  # the minimum, unless minimum + 2^w - 1 would pass 4095
    d = (s - base[:, :, None]).astype(np.uint64)
    shifts = np.arange(BLOCK, dtype=np.uint64)
    planes = np.zeros((n, BLOCKS, MAX_WIDTH), dtype=np.uint64)
    for k in range(MAX_WIDTH):
        planes[:, :, k] = np.bitwise_or.reduce(((d >> np.uint64(k)) & np.uint64(1)) << shifts, axis=2)
    used = np.arange(MAX_WIDTH)[None, None, :] < width[:, :, None]  # b ascending, then k ascending
    per_row = width.sum(axis=1)
    row_start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(16 + 8 * per_row, out=row_start[1:])
    words = np.zeros(int(row_start[-1]) // 8, dtype="<u8")
    first = row_start[:-1] // 8
    h = (base | (width << 12)).astype(np.uint64)
    for half in range(2):
        q = h[:, 4 * half:4 * half + 4]
        words[first + half] = q[:, 0] | (q[:, 1] << np.uint64(16)) | (q[:, 2] << np.uint64(32)) | (q[:, 3] << np.uint64(48))
    before = np.concatenate([[0], np.cumsum(per_row)[:-1]]) if n else np.zeros(0, dtype=np.int64)
    within = np.arange(int(per_row.sum())) - np.repeat(before, per_row)
    words[np.repeat(first + 2, per_row) + within] = planes[used]
    return row_start, words.view(np.uint8).copy()


def decode_row(record):
    """One record (uint8) -> its 512 samples; ValueError for anything the contract refuses."""
    record = np.asarray(record, dtype=np.uint8)
    if len(record) < 16 or len(record) % 8:
        raise ValueError("record size")
    h = record[:16].view("<u2").astype(np.int64)
    base, width = h & 0xfff, h >> 12
    if (width > MAX_WIDTH).any() or (base + (1 << width) - 1 > 4095).any() or len(record) != 16 + 8 * width.sum():
        raise ValueError("record header")
    words = record[16:].view("<u8")
    out = np.empty(NUM_TB, dtype=np.int16)
    at = 0
    shifts = np.arange(BLOCK, dtype=np.uint64)
    for b in range(BLOCKS):
        v = np.zeros(BLOCK, dtype=np.int64)
        for k in range(int(width[b])):
            v |= (((words[at] >> shifts) & np.uint64(1)).astype(np.int64)) << k
            at += 1
        out[BLOCK * b:BLOCK * (b + 1)] = base[b] + v
    return out


def decode(row_start, packed):
    row_start = np.asarray(row_start, dtype=np.int64)
    packed = np.asarray(packed, dtype=np.uint8)
    out = np.empty((len(row_start) - 1, NUM_TB), dtype=np.int16)
    if len(out) and ((np.diff(row_start) < 0).any() or (row_start % 8).any() or row_start[0] < 0 or row_start[-1] > len(packed)):
        raise ValueError("offsets")
    for r in range(len(out)):
        out[r] = decode_row(packed[row_start[r]:row_start[r + 1]])
    return out


def edge_rows():
    """The rows every encoder is held to: {name: [r, 512] int16}."""
    rows = {"zeros": np.zeros((1, NUM_TB)), "full": np.full((1, NUM_TB), 4095),
            "alternating": np.tile([0, 4095], (1, NUM_TB // 2)), "constant7": np.full((1, NUM_TB), 7)}
    steps = []
    for k in range(12):  # a block whose range is 2^k - 1 (width k) and one whose range is 2^k (width k + 1)
        row = np.full(NUM_TB, 100)
        row[BLOCK * 1 + 5] = 100 + (1 << k) - 1
        row[BLOCK * 2 + 63] = 100 + (1 << k)
        row[BLOCK * 5:BLOCK * 6] = 4095 - (1 << k)  # ... and the same step against the top of the range
        row[BLOCK * 5 + 1] = 4095
        steps.append(row)
    rows["width_steps"] = np.array(steps)
    single = np.zeros((4, NUM_TB))
    for i, j in enumerate((0, 63, 64, 511)):
        single[i, j] = 1 + 1000 * i
    rows["single"] = single
    return {name: np.ascontiguousarray(r, dtype=np.int16) for name, r in rows.items()}


def random_rows(n, seed=0, pedestal=300, sigma=5.0):
    """n rows of pedestal + rounded Gaussian noise + 1 .. 3 pulses, clamped to 0 .. 4095 (a few of them saturate)."""
    rng = np.random.default_rng(seed)
    j = np.arange(NUM_TB)
    rows = pedestal + np.rint(rng.normal(0.0, sigma, (n, NUM_TB))) if sigma > 0 else np.full((n, NUM_TB), float(pedestal))
    for r in range(n):
        for _ in range(int(rng.integers(1, 4))):
            t0, amp, tau = rng.integers(0, NUM_TB), rng.uniform(20, 6000), rng.uniform(3, 12)
            x = np.clip((j - t0) / tau, 0, None)
            rows[r] += np.rint(amp * x ** 3 * np.exp(3.0 - 3.0 * x))  # (peaks at amp, tau samples after t0)
    return np.clip(rows, 0, 4095).astype(np.int16)


def all_edge_rows():
    return np.concatenate(list(edge_rows().values()))
