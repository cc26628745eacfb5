"""Synthetic signals for the active-speech-level tests (tests/test_active_level_cpu.py, tests/test_active_level.py)."""
import numpy as np


def gated_bursts(n, fs, seed, amplitude=0.1, floor=1e-4, on=0.4):
    """Gaussian noise gated per second: `on` seconds at `amplitude`, the rest at `floor`; float32."""
    rng = np.random.default_rng(seed)
    gate = np.where((np.arange(n) % fs) < int(on * fs), amplitude, floor)
    return (gate * rng.standard_normal(n)).astype(np.float32)


def published_counts(x, fs):
    """The activity counts of the published asl_P56 loop (Hu & Loizou), transcribed literally: per sample and per threshold a
    hangover counter that is reset where the envelope reaches the threshold, counts while it is below I and starts expired.
    The envelope is metrics.p56_envelope (the published filter calls)."""
    from dcsnet import metrics
    q = metrics.p56_envelope(x, fs)
    I = int(np.ceil(fs * 0.2))
    c = [2.0 ** (j - 15) for j in range(15)]
    a = [0] * 15
    hang = [I] * 15
    for k in range(len(q)):
        for j in range(15):
            if q[k] >= c[j]:
                a[j] += 1
                hang[j] = 0
            elif hang[j] < I:
                a[j] += 1
                hang[j] += 1
            else:
                break
    return np.array(a, dtype=np.int64)
