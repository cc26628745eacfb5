"""What the GPU tests of the ragged measures share (tests/test_frame_measures_device.py, test_spectral_measures_device.py,
test_sdr_device.py, partly test_estoi_device.py and test_score_ragged.py): the flat buffer of a list of recordings, the AR(2)
signal pairs, and the comparison with a host contract by the rule of 2 float32 ulps + 1e-9 — and record(), the JSON record of
observed figures that every parity test writes.  A plain module, imported by name like tests/_plan_probe.py."""
import json
import os

import numpy as np
import torch
from scipy.signal import lfilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record(file_name, path, value):
    """Figures -> $DCS_PARITY_DIR/<file_name> (default parity_out/ in the repository, kept out of git): path = nested keys."""
    out = os.path.join(os.environ.get('DCS_PARITY_DIR') or os.path.join(ROOT, 'parity_out'), file_name)
    try:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        d = json.load(open(out)) if os.path.exists(out) else {}
        node = d
        for k in path[:-1]:
            node = node.setdefault(k, {})
        node[path[-1]] = value
        json.dump(d, open(out, 'w'), indent=1, sort_keys=True)
    except OSError:
        pass


def flat(recs, dev):
    """A list of 1-D arrays -> (the flat float32 device buffer, int64 offsets [n + 1] on the device)."""
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    buf = np.concatenate(recs) if off[-1] else np.zeros(0, np.float32)
    return torch.from_numpy(buf.astype(np.float32)).to(dev), torch.from_numpy(off).to(dev)


def ar_noise(L, snr_db, rng):
    """float64: (x, v), AR(2)-shaped noise and white noise snr_db below it."""
    x = lfilter([1.0], [1.0, -1.6, 0.8], rng.standard_normal(L + 200))[200:]
    v = rng.standard_normal(L)
    if L:
        v *= np.linalg.norm(x) / max(np.linalg.norm(v), 1e-30) * 10 ** (-snr_db / 20)
    return x, v


def ar_pair(L, snr_db, rng, zero_head=0):
    """float32: AR(2)-shaped noise as the clean signal, white noise added at snr_db; zero_head samples of both are exactly 0."""
    x, v = ar_noise(L, snr_db, rng)
    x, y = (0.1 * x).astype(np.float32), (0.1 * (x + v)).astype(np.float32)
    x[:zero_head], y[:zero_head] = 0.0, 0.0
    return x, y


def tied_pair(rng):
    """4800 samples of period 120 (the hop at 16 kHz): every frame is the same frame, every value ties."""
    x = np.tile(0.1 * rng.standard_normal(120), 40)
    y = x + np.tile(0.03 * rng.standard_normal(120), 40)
    return x.astype(np.float32), y.astype(np.float32)


def check_against_host(got, host, keys, tag, what, file_name):
    """got: {key: float32 [n] device tensor}; host: the host function's dict per recording.  Per key: 2 float32 ulps of the host
    value + 1e-9; NaN exactly where the host has NaN.  Prints and records (file_name, under (what, key)) the largest difference."""
    for k in keys:
        g = got[k].cpu().numpy()
        assert got[k].dtype == torch.float32 and g.shape == (len(host),)
        h = np.array([m[k] for m in host])
        assert np.array_equal(np.isnan(g), np.isnan(h)), (what, k, g, h)
        ok = ~np.isnan(h)
        diff = np.abs(g[ok].astype(np.float64) - h[ok])
        tol = 2.0 * np.spacing(np.abs(h[ok]).astype(np.float32)).astype(np.float64) + 1e-9
        worst = float(diff.max()) if ok.any() else 0.0
        ratio = float((diff / tol).max()) if ok.any() else 0.0
        print(f'[{tag}] {what} {k}: max |device - host| = {worst:.3e}, {ratio:.3f} of the tolerance')
        record(file_name, (what, k), {'max_abs_diff': worst, 'max_share_of_tolerance': ratio})
        assert (diff <= tol).all(), (what, k, g, h)
