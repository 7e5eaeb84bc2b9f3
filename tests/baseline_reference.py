"""The Fourier baseline of the trace rows restated in numpy (the contract is in include/attpc_engine.h, "Fourier
baseline", steps a to e): integers for the edge fix, the peak mask, the replacement and the result, ``numpy.fft`` for
the filter.  ``remove`` takes rows x [R,512] and the window scale and gives (y, baseline, mask); ``ambiguous`` names the
samples where a second implementation of the floating-point step may round the baseline the other way; ``rows`` is the
seeded generator of test rows the baseline tests share."""
import numpy as np

NUM_TB = 512
DELTA = 1.0e-6  # |baseline - half-integer| below which y may differ by 1 between implementations (contract, step h)


def edge_fixed(x) -> np.ndarray:
    """Step a: x [R,512] as int64 with x[0] = x[1] and x[511] = x[510]."""
    x = np.array(x, dtype=np.int64).reshape(-1, NUM_TB)
    x[:, 0] = x[:, 1]
    x[:, -1] = x[:, -2]
    return x


def peak_mask(x: np.ndarray) -> np.ndarray:
    """Step b on edge-fixed int64 rows: d = 512 x - S > 0 and 4 d^2 > 9 (512 Q - S^2)."""
    s = x.sum(axis=1, keepdims=True)
    q = (x * x).sum(axis=1, keepdims=True)
    d = NUM_TB * x - s
    return (d > 0) & (4 * d * d > 9 * (NUM_TB * q - s * s))


def replaced(x: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """Step c: b = x as f64, the masked samples replaced by (double)(sum of the others) / (double)(their number)."""
    b = x.astype(np.float64)
    rest = np.where(mask, 0, x).sum(axis=1).astype(np.float64)
    count = (~mask).sum(axis=1).astype(np.float64)
    mean = rest / count
    return np.where(mask, mean[:, None], b)


def window(scale: float) -> np.ndarray:
    """Step d's F [512]."""
    return np.fft.ifftshift(np.sinc(np.arange(-NUM_TB // 2, NUM_TB // 2) / float(scale)))


def remove(x, scale: float = 20.0):
    """Steps a to e -> (y [R,512] int16, baseline [R,512] f64, mask [R,512] bool)."""
    x = edge_fixed(x)
    mask = peak_mask(x)
    b = replaced(x, mask)
    baseline = np.real(np.fft.ifft(np.fft.fft(b, axis=1) * window(scale)[None, :], axis=1))
    y = np.clip(x - np.rint(baseline).astype(np.int64), -4095, 4095).astype(np.int16)
    return y, baseline, mask


def ambiguous(baseline: np.ndarray, delta: float = DELTA) -> np.ndarray:
    """Where the baseline lies within ``delta`` of a half-integer."""
    frac = baseline - np.floor(baseline)
    return np.abs(frac - 0.5) <= delta


def pulse_shape() -> np.ndarray:
    """A GET-like pulse exp(-3u) u^3 sin(u), u = t / 6.25, negative lobes clipped, scaled to a maximum of 1."""
    u = np.arange(NUM_TB) / 6.25
    shape = np.clip(np.exp(-3.0 * u) * u ** 3 * np.sin(u), 0.0, None)
    return shape / shape.max()


def rows(n: int, seed: int, pedestal: bool = True, noise: bool = True) -> np.ndarray:
    """``n`` test rows [n,512] int16 in 0 .. 4095: 0 to 3 pulses each, every pulse spread evenly over 1 to 60 buckets
    with a total amplitude of 30 to 6000, the summed signal clipped at 4095; a pedestal in 250 .. 450 (``pedestal``) and
    rounded Gaussian noise of sigma 5 (``noise``) on top, the whole clipped to 0 .. 4095."""
    rng = np.random.default_rng(seed)
    shape = pulse_shape()
    out = np.zeros((n, NUM_TB), dtype=np.int16)
    for i in range(n):
        arrivals = np.zeros(NUM_TB)
        for _ in range(int(rng.integers(0, 4))):
            start, spread = int(rng.integers(0, NUM_TB - 60)), int(rng.integers(1, 61))
            arrivals[start:start + spread] += float(rng.uniform(30.0, 6000.0)) / spread
        signal = np.minimum(np.convolve(arrivals, shape)[:NUM_TB], 4095.0)
        if pedestal:
            signal += int(rng.integers(250, 451))
        if noise:
            signal += np.rint(rng.normal(0.0, 5.0, NUM_TB))
        out[i] = np.clip(np.rint(signal), 0, 4095).astype(np.int16)
    return out


def mixed_rows(n: int, seed: int) -> np.ndarray:
    """``n`` rows, a quarter of each combination of pedestal and noise."""
    quarter = (n + 3) // 4
    parts = [rows(quarter, seed + 4 * i, pedestal=bool(i & 1), noise=bool(i & 2)) for i in range(4)]
    return np.concatenate(parts)[:n]
