"""numpy oracle of raw-frame conditioning (include/naf_hip.h A3), for tests/test_frames_cpu.py,
tests/test_hip_frames.py and tools/frames_host_check.py.  `condition` is the float32 restatement the kernel equals bit for bit
without the logarithm; `condition_loops` states the definition again one pixel at a time, with the quotient taken in float64 and
rounded once (for float32 operands that is the correctly rounded float32 quotient) and the median read off a sorted list.  With no bad
pixel `condition(..., log=False)` is tomopy's remove_outlier(normalize(raw, flat, dark), dif, size); neither scipy nor tomopy is
imported.  No GPU.
"""
import numpy as np

from _stripe_oracle import bits, equal_bits, key, unkey  # noqa: F401  (equal_bits is for the tests)

SIZES = (3, 5, 7)
BAD_KEY = np.uint32(0xffffffff)                # the window word of a bad pixel: the key of a NaN, above every finite float's
LOG, CLAMP_NONNEG = 1, 2
TILE_H, TILE_W = 16, 64                        # NAF_FRAMES_TILE_H, NAF_FRAMES_TILE_W


def transmission(raw, dark, flat, bad=None):
    """-> (t float32 [N, H, W], isbad bool [N, H, W]): steps 1 and 2."""
    raw = np.asarray(raw)
    assert raw.ndim == 3 and raw.dtype in (np.float32, np.uint16), (raw.shape, raw.dtype)
    dark, flat = np.asarray(dark, dtype=np.float32), np.asarray(flat, dtype=np.float32)
    with np.errstate(all="ignore"):
        den = flat - dark
        num = raw.astype(np.float32) - dark[None]
        t = num / den[None]
        isbad = ~(den > 0)[None] | ((t - t) != 0)
    if bad is not None:
        isbad = isbad | (np.asarray(bad) != 0)[None]
    return t.astype(np.float32), isbad


def window_words(t, isbad, size):
    """-> uint32 [N, H, W, size * size]: the words of every pixel's reflected window, a bad entry as BAD_KEY."""
    h = size // 2
    words = np.where(isbad, BAD_KEY, key(bits(t)))
    padded = np.pad(words, ((0, 0), (h, h), (h, h)), mode="symmetric")
    win = np.lib.stride_tricks.sliding_window_view(padded, (size, size), axis=(1, 2))
    return win.reshape(*t.shape, size * size)


def medians(t, isbad, size):
    """-> (m float32 [N, H, W], c int [N, H, W]): the lower median of every window's valid entries, 1.0 where there is none."""
    ranked = np.sort(window_words(t, isbad, size), axis=-1)                    # BAD_KEY sorts last
    c = (ranked != BAD_KEY).sum(axis=-1)
    rank = np.maximum(c - 1, 0) // 2
    m = unkey(np.take_along_axis(ranked, rank[..., None], axis=-1)[..., 0]).view(np.float32)
    return np.where(c == 0, np.float32(1.0), m).astype(np.float32), c


def tail(t, t_min, log, clamp):
    """Step 5 in float32, with numpy's logarithm: the kernel's equals it only up to the device's logf."""
    if not log:
        return t
    p = -np.log(np.maximum(t, np.float32(t_min)))
    if clamp:
        p = np.where(p > 0, p, np.float32(0.0))
    return p.astype(np.float32)


def repaired(raw, dark, flat, bad=None, size=3, dif=0.1):
    """-> (t' float32 [N, H, W], counts uint32 [N, 2], (t - m) float32 of the pixels that are not bad, -inf elsewhere)."""
    assert size in SIZES and size <= raw.shape[1] and size <= raw.shape[2], (raw.shape, size)
    t, isbad = transmission(raw, dark, flat, bad)
    m, _ = medians(t, isbad, size)
    with np.errstate(all="ignore"):
        excess = np.where(isbad, -np.inf, t - m).astype(np.float32)
    outlier = ~isbad & (excess > np.float32(dif))
    out = np.where(isbad | outlier, m, t).astype(np.float32)
    counts = np.stack([outlier.sum(axis=(1, 2)), isbad.sum(axis=(1, 2))], axis=1).astype(np.uint32)
    return out, counts, excess


def condition(raw, dark, flat, bad=None, size=3, dif=0.1, t_min=1e-5, log=False, clamp=False):
    """The definition, vectorised in float32 -> (out float32 [N, H, W], counts uint32 [N, 2])."""
    assert log or not clamp
    out, counts, _ = repaired(raw, dark, flat, bad, size, dif)
    return tail(out, t_min, log, clamp), counts


def log_reference(raw, dark, flat, bad=None, size=3, dif=0.1, t_min=1e-5, clamp=False):
    """-log in float64 of the oracle's float32 max(t', t_min) -> float64 [N, H, W]: what the LOG output is measured against."""
    out, _, _ = repaired(raw, dark, flat, bad, size, dif)
    p = -np.log(np.maximum(out, np.float32(t_min)).astype(np.float64))
    return np.maximum(p, 0.0) if clamp else p


def ulp_error(got, want64):
    """|got - want| in units of the last place of float32(want) -> float64 array."""
    want32 = np.abs(want64.astype(np.float32))
    ulp = np.spacing(np.maximum(want32, np.float32(np.finfo(np.float32).tiny))).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / ulp


def _key_int(b):
    return (~b) & 0xffffffff if b & 0x80000000 else b | 0x80000000


def _reflect_int(i, n):
    if i < 0:
        return -i - 1
    if i >= n:
        return 2 * n - 1 - i
    return i


def condition_loops(raw, dark, flat, bad=None, size=3, dif=0.1):
    """The definition without the logarithm, one pixel at a time -> (out, counts).  Shares nothing with `condition` but `bits`."""
    raw = np.asarray(raw)
    N, H, W = raw.shape
    h = size // 2
    out = np.zeros((N, H, W), dtype=np.float32)
    counts = np.zeros((N, 2), dtype=np.uint32)
    f32, f64 = np.float32, np.float64
    with np.errstate(all="ignore"):
        for i in range(N):
            t = np.zeros((H, W), dtype=np.float32)
            isbad = np.zeros((H, W), dtype=bool)
            for v in range(H):
                for u in range(W):
                    d, f, x = f64(f32(dark[v, u])), f64(f32(flat[v, u])), f64(f32(raw[i, v, u]))
                    den, num = f64(f32(f - d)), f64(f32(x - d))                  # sums of float32 round once from float64
                    t[v, u] = f32(num / den)
                    isbad[v, u] = (bad is not None and bad[v, u] != 0) or not den > 0 or not np.isfinite(t[v, u])
            tb = bits(t)
            for v in range(H):
                for u in range(W):
                    valid = []
                    for a in range(-h, h + 1):
                        for b in range(-h, h + 1):
                            vv, uu = _reflect_int(v + a, H), _reflect_int(u + b, W)
                            if not isbad[vv, uu]:
                                valid.append((_key_int(int(tb[vv, uu])), t[vv, uu]))
                    valid.sort(key=lambda e: e[0])
                    m = valid[(len(valid) - 1) // 2][1] if valid else f32(1.0)
                    if isbad[v, u]:
                        out[i, v, u] = m
                        counts[i, 1] += 1
                    elif f32(f64(t[v, u]) - f64(m)) > f32(dif):
                        out[i, v, u] = m
                        counts[i, 0] += 1
                    else:
                        out[i, v, u] = t[v, u]
    return out, counts


def special(shape, seed=0):
    """`frames` in float32 with what the bad test and the key must survive planted in it -> (raw, dark, flat): NaN, +-Inf and -0.0 in
    raw, raw == dark with dark = +-0 (t = +-0), flat == dark (den = 0), flat < dark (den < 0), and NaN and Inf in flat."""
    raw, dark, flat = frames(shape, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    pick = rng.random(raw.shape)
    for k, value in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0)):
        raw[(pick >= 0.03 * k) & (pick < 0.03 * (k + 1))] = value
    pick = rng.random(dark.shape)
    zero = (pick < 0.10)
    dark[zero] = np.where(rng.random(dark.shape) < 0.5, 0.0, -0.0)[zero].astype(np.float32)        # num = raw - +-0 keeps raw's sign
    flat[(pick >= 0.10) & (pick < 0.14)] = dark[(pick >= 0.10) & (pick < 0.14)]
    flat[(pick >= 0.14) & (pick < 0.18)] = dark[(pick >= 0.14) & (pick < 0.18)] - 7
    flat[(pick >= 0.18) & (pick < 0.20)] = np.nan
    flat[(pick >= 0.20) & (pick < 0.22)] = np.inf
    return raw, dark, flat


def frames(shape, seed=0, dtype=np.float32, zingers=0.02, dead=0.02):
    """A seeded test scan at `shape` = (N, H, W) -> (raw, dark, flat): counts of a smooth transmission under a flat of about 4000
    over a dark of about 100, all whole numbers below 65536 so that uint16 and float32 hold the same values; a fraction `zingers` of
    the samples is multiplied by 3 and a fraction `dead` of the detector pixels has flat == dark."""
    N, H, W = shape
    rng = np.random.default_rng(seed)
    dark = np.round(100 + 5 * rng.standard_normal((H, W)))
    flat = np.round(dark + 4000 + 200 * rng.standard_normal((H, W)))
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    trans = 0.55 + 0.4 * np.cos(0.31 * vv + 0.17 * uu + np.arange(N)[:, None, None])
    raw = np.round(dark + (flat - dark) * trans + 8 * rng.standard_normal(shape))
    raw = np.where(rng.random(shape) < zingers, np.minimum(raw * 3, 65535), raw)
    flat = np.where(rng.random((H, W)) < dead, dark, flat)
    return np.clip(raw, 0, 65535).astype(dtype), dark.astype(np.float32), flat.astype(np.float32)
