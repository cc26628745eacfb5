"""ORACLE — TEST INFRASTRUCTURE ONLY. Never imported by the product path.

Host restatement of the fused dropout masks (dcs-net_amd/csrc/dcs_common.h: dcs_hash32, dcs_keep_scale), so that an fp64
oracle can drop exactly what the device dropped.  The mask is a pure function of (seed, element index):

    z    = seed + idx * 0x9E3779B97F4A7C15                      (uint64, wrapping)
    z    = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
    z    = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z    = z ^ (z >> 31)                                        — the splitmix64 output function
    u    = float32(z >> 40) * 2^-24                             — the top 24 bits of the high word: uniform in [0, 1)
    keep = 0 if u < float32(p) else 1 / (1 - p)

`idx` is the flat index of the REAL element of the channels-last tensor [B,H,W,C,2] (re and im are dropped independently),
and every kernel adds the device-side offset ops.SEED_STATE to its by-value seed: seed and state are separate arguments here
and their sum wraps mod 2^64 as it does on the device.  This is the project's own arithmetic; the reference draws its
masks from ATen's generator.
"""
import numpy as np
import torch

_M64 = (1 << 64) - 1
_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def hash64(seed, n, state=0, first=0):
    """The 64-bit hash of the indices first .. first + n - 1 (numpy uint64 [n]); seed + state wraps mod 2^64."""
    s = np.uint64((int(seed) + int(state)) & _M64)
    with np.errstate(over='ignore'):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(int(first) & _M64)) * _GAMMA + s
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return z


def uniform(seed, n, state=0, first=0):
    """dcs_keep_scale's uniform: float32 [n] in [0, 1), (hash32 >> 8) * 2^-24 — both steps exact in float32."""
    h24 = (hash64(seed, n, state, first) >> np.uint64(40)).astype(np.uint32)
    return h24.astype(np.float32) * np.float32(1.0 / 16777216.0)


def scale(p, wide=True):
    """1 / (1 - p): in fp64 (wide) or as the kernels form it, float32(1) / (float32(1) - float32(p))."""
    if wide:
        return 1.0 / (1.0 - float(p))
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_scale(seed, n, p, state=0, wide=True, first=0):
    """n values, each 0 or 1 / (1 - p): torch float64 (wide) or float32.  The threshold test is float32 either way."""
    dropped = uniform(seed, n, state, first) < np.float32(p)
    dt = np.float64 if wide else np.float32
    return torch.from_numpy(np.where(dropped, dt(0), dt(scale(p, wide))).astype(dt))


def keep_nchw(seed, shape_bchw, p, state=0, wide=True):
    """The mask of a channels-last activation [B,H,W,C,2] in the oracle's layout [B,C,H,W,2] (view_as_real of a complex
    [B,C,H,W] tensor).  The latent fc site is [B, seq, C, 2] on both sides: keep_scale(...).view(B, seq, C, 2)."""
    B, C, H, W = shape_bchw
    return keep_scale(seed, B * H * W * C * 2, p, state, wide).view(B, H, W, C, 2).permute(0, 3, 1, 2, 4).contiguous()


def keep_like(seed, shape_complex, p, state=0, wide=True):
    """The mask for view_as_real of an oracle tensor of complex shape [B,C,H,W] (a conv site) or [B, seq, C] (the fc site)."""
    shape = tuple(shape_complex)
    if len(shape) == 4:
        return keep_nchw(seed, shape, p, state, wide)
    n = 2
    for s in shape:
        n *= s
    return keep_scale(seed, n, p, state, wide).view(*shape, 2)
