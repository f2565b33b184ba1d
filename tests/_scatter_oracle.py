"""Per-row float64 reference of the binned table-gradient scatter, with bounds derived from its record formats (not a test module).

The binned scatter (csrc/scatter_v2.h, scatter_binned.h, scatter_host.h) is driven through naf_levels_scatter with n_ranks blocks of
caller-chosen feature gradients and caller-chosen rays; nothing else of the training step is involved.  This module builds the inputs,
the reference and the bounds; tests/test_scatter_oracle_cpu.py validates them without a GPU, tests/test_hip_scatter_reference.py holds
the kernels to them.

EXACT COORDINATES.  The reference must put every point into the cell the kernel puts it in, so the rays are built such that
`o + d * z` (SrcRays::position) has ONE value in fp32 whatever the compiler contracts: bound = 0.5 (2 * bound = 1: the division is
the identity and `p + bound` is exact), d on a 2^-8 grid with |d| <= 1 (9 significant bits), z on a 2^-14 grid below 2 (15 bits), o
on a 2^-22 grid inside the volume.  d * z then has at most 24 significant bits (exact in fp32), and the sum lies on a 2^-22 grid below
4 (24 bits: exact).  Points that leave the volume take the clamp +-(bound - 1e-6f), restated here in fp32.  x01 * scale + 0.5
evaluated in float64 and rounded once to fp32 (hashgrid_ref.corners) is the kernels' fmaf.  positions() asserts the premise: the fp32
fused, fp32 unfused and float64 evaluations agree bit for bit.

REFERENCE (reference()), per table row and channel, from the gradient values as stored (bf16 / fp32 upcast, never re-rounded) and
the fp32 corner weights of hashgrid_ref.corners: s = sum w g in float64, a = sum |w g|, n = number of contributions,
p = sum |g| w_y w_z (the magnitude of the payload a pair record carries for both x-neighbour corners), and gmax = max |g| over the
levels of the call (the fixed-point scale of the reducers), E = floor(log2 gmax).

BOUNDS, |got - (prefill + s)| per element (u = 2^-24):

  all families, the fp32 part F = (n + 8) * 2^-23 * (a + |prefill|):
      the kernels' weights are products of the same fp32 factors in another order (<= 4 u relative against the reference's), the
      product with g (1 u), on merged levels up to four fused adds of a segmented scan (4 u of the run's magnitudes), a second
      product for single records (1 u), the conversion of the integer sum to fp32 (1 u), the `+=` into the table (1 u of
      |prefill| + a), and for spilled records or a split reducer up to n more fp32 atomic adds (n u of |prefill| + a):
      (n + 13) u (a + |prefill|) to first order, rounded up to (2 n + 16) u for the second-order terms.

  PairFx (scatter_v2.h, 8-byte records):
      payload  bf16(fl32(w_y w_z) g), round to nearest even.  bf16 has 8 significant bits: half an ulp is 2^-8 of the binade's
               lower end, so the relative error is <= 2^-8 (NOT 2^-9, the issue's reading: 2^-9 is the error relative to the
               binade's UPPER end; the numpy restatement leaves a 2^-9 bound at once), 2^-8 |w g| in either corner's row  -> 2^-8 a
               (singles round bf16(payload * w_x), merged runs round the bf16 of the run's sum: the same 2^-8 of the magnitudes)
      f_x      truncated to 15 bits, 0 <= f_x - f_q < 2^-15: the first corner gains, the second loses < 2^-15 |payload|   -> 2^-15 p
      products payload * f_q * 2^shift and payload * 2^shift - that: 8 x 15 bits, exact
      fixed    shift = kFixHead2 - E - 1 = 25 - E (at most 120), v_cvt_rpi = floor(v + 0.5): ROUNDS, half a quantum
               2^(E - 25) per converted value, one value per contribution and row                                          -> n 2^(E-26)
      sum      64-bit integers: exact
      bound_fx = (2^-8 a + 2^-15 p) (1 + 2^-7) + n 2^(E-26) + F        ((1 + 2^-7): products of the terms above)
      (the issue's reading had n 2^(E-24) for the conversion: the code rounds, so a quarter of that holds.)

  PairBF16 (scatter_binned.h):  values bf16(fl32(w g)) (merged: bf16 of the run's fp32 sum), to_fixed rounds to nearest with
      shift = kFixHead - E - 1 = 30 - E:   bound_bf16 = 2^-8 a (1 + 2^-7) + n 2^(E-31) + F
  PairF32:  values fl32(w g):             bound_f32  = n 2^(E-31) + F

TEETH.  A fault that moves one contribution of payload magnitude q = |g| w_y w_z and x weight w_x changes its row by w_x q.  It
leaves the bound whenever w_x q > 2 * bound (the faulted kernel's own rounding may use the bound once).  In a row with a <= p <= 2 q,
n <= 4, q >= 2^(E-8) and |prefill| <= q / 4:  2 * bound_fx <= q 2^-6 (1 + 2^-7)(1 + 2^-7) + q 2^-15 + q 2^-17 < 1.03 * 2^-6 q.
W_X_THRESHOLD = 1.05 * 2^-6 (a row the contribution has to itself, p = q, halves it to the 2^-7 the issue expected; with the correct
bf16 roundoff that is as tight as the record format allows).  test_scatter_oracle_cpu.py injects faults at the smallest w_x above it.
"""
import functools

import numpy as np

from oracle import hashgrid_ref

BOUND = np.float32(0.5)
LIM = np.float32(BOUND - np.float32(1e-6))            # SrcRays::position: lim = bound - 1e-6f in fp32
U23 = 2.0 ** -23
W_X_THRESHOLD = 1.05 * 2.0 ** -6
SENTINEL, GUARD_ROWS, PAD = -7.25, 64, 96
AXIS_LAST_LEVEL = 10


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def make_rays(kind, n_rays, S, seed):
    """-> rays float32 [n_rays, 8] (o, d, near, far), z float32 [n_rays, S] (explicit depths, non-decreasing along a ray).
    kind 'mixed': general rays inside the volume (ray 0 among them: coarse levels merge), every 5th parallel to an axis (every 10th along
    y or z with its x fixed), every 7th leaves the volume, every 11th so short that its samples share cells on coarse levels.
    kind 'axis_last': every ray parallel to y or z with x fixed in a cell 255 mod 256 of level AXIS_LAST_LEVEL (H = 16).
    kind 'runs': ray 0 is short (merging is on for every level below 2^16 cells per axis) and rays hold runs of 4, 16, 17 and S equal
    positions; the last ray is one run of S."""
    rng = np.random.default_rng(seed)
    q22, q8, q14 = 2.0 ** 22, 256.0, 2.0 ** 14
    o = np.round(rng.uniform(-0.45, 0.45, (n_rays, 3)) * q22) / q22
    e = rng.uniform(-0.45, 0.45, (n_rays, 3))
    d = np.clip(np.round((e - o) * q8), -256, 256) / q8
    step = np.maximum(1, (q14 - 1) // S)                                  # z = j * step * 2^-14 < 1
    jit = rng.integers(0, step, (n_rays, S))
    z = (np.arange(S)[None, :] * step + jit) / q14
    r = np.arange(n_rays)
    ax = (r % 5 == 1)
    axis = np.where(r % 10 == 1, 0, 1 + (r // 10) % 2)                    # x, or y / z with x fixed
    for i in np.nonzero(ax)[0]:
        keep = d[i, axis[i]] if d[i, axis[i]] != 0 else 0.5
        d[i] = 0.0
        d[i, axis[i]] = keep
    leave = (r % 7 == 3)
    z[leave] *= 2.0                                                       # still on the 2^-14 grid, below 2
    short = (r % 11 == 5)
    z[short] = (np.arange(S)[None, :] * rng.integers(1, 5, (int(short.sum()), 1)) + 4096) / q14
    if kind == "axis_last":
        scale, _ = hashgrid_ref.level_scale_res(AXIS_LAST_LEVEL, 16)
        cell = 255 + 256 * rng.integers(0, 64, n_rays)                    # the last x cell of a chunk (T = 2^14, 64 buckets: 256 rows each)
        x01 = np.ceil((cell + 0.25) / float(scale) * q22) / q22
        assert np.array_equal(np.floor(hashgrid_ref._fma32(x01.astype(np.float32), scale, np.float32(0.5))), cell)
        o[:, 0] = x01 - 0.5
        d[:, 0] = 0.0
        d[np.arange(n_rays), 1 + r % 2] = 0.0                             # parallel to z (even rays) or y
        d[(d == 0).all(1), 2] = 0.5
    elif kind == "runs":
        z[0] = (np.arange(S) + 4096) / q14
        for i in range(1, n_rays):
            run = (4, 16, 17, S)[i % 4] if i + 1 < n_rays else S
            z[i] = z[i, (np.arange(S) // run) * run]
    elif kind != "mixed":
        raise ValueError(kind)
    rays = np.concatenate([o, d, z.min(1, keepdims=True), z.max(1, keepdims=True)], 1).astype(np.float32)
    assert np.array_equal(rays[:, :6].astype(np.float64), np.concatenate([o, d], 1)) and float(z.max()) < 2.0
    return rays, z.astype(np.float32)


def positions(rays, z):
    """x01 float32 [n_rays * S, 3]: the points SrcRays::get hands the kernels.  Asserts that they do not depend on the contraction."""
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    z = z[:, :, None]
    unfused = ((d * z).astype(np.float32) + o).astype(np.float32)
    fused = (d.astype(np.float64) * z.astype(np.float64) + o.astype(np.float64)).astype(np.float32)          # one rounding: fmaf
    exact = d.astype(np.float64) * z.astype(np.float64) + o.astype(np.float64)
    assert np.array_equal(unfused.view(np.uint32), fused.view(np.uint32)), "o + d z depends on the contraction"
    assert np.array_equal(fused.astype(np.float64), exact), "o + d z is not exact in fp32"
    p = np.where(unfused < -LIM, -LIM, unfused)
    p = np.where(p > LIM, LIM, p).astype(np.float32)
    x01 = (p + BOUND).astype(np.float32)                                  # one fp32 add behind the clamp; (x / 1) is the identity
    inside = np.abs(unfused) <= LIM
    assert np.array_equal(x01[inside].astype(np.float64), exact[inside] + 0.5), "p + bound is not exact inside the volume"
    assert float(x01.min()) >= 0.0 and float(x01.max()) <= 1.0
    return x01.reshape(-1, 3)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
FAMILIES = ("fx", "fx_gather", "bf16", "f32")


def _case(name, family="fx", L=16, C=2, H=16, log2T=14, levels=None, n_rays=48, S=64, n_ranks=1, pad=PAD, flags=(), min_buckets=0,
          offsets="plain", rays="mixed", grad="normal", teeth=False):
    return dict(name=name, family=family, L=L, C=C, H=H, log2T=log2T, levels=levels or (0, L), n_rays=n_rays, S=S, n_ranks=n_ranks, pad=pad,
                flags=tuple(flags), min_buckets=min_buckets, offsets=offsets, rays=rays, grad=grad, teeth=teeth)


def _cases():
    out = []
    # families at the canonical shape (48 x 64 = 3T: whole tiles of the 1024-point plan), PairBF16 / PairF32 at their other shapes
    for fam in FAMILIES:
        out.append(_case(f"family-{fam}", fam, teeth=fam == "fx"))          # (the restatement is the same for both scatter_v2 routes)
    for L, C in ((8, 4), (4, 8), (32, 1)):
        out.append(_case(f"bf16-L{L}-C{C}", "bf16", L=L, C=C, H=1))
    out.append(_case("f32-C4", "f32", L=8, C=4, H=1))
    # tile edges, T = 1024 points: 2, T - 1, T, T + 1, 3 T + 17 points (n_rays x S splits where S does not divide the tile)
    for n_rays, S in ((1, 2), (33, 31), (16, 64), (25, 41), (1, 3089)):
        for fam in ("fx", "bf16"):
            out.append(_case(f"tile-{n_rays * S}-{fam}", fam, n_rays=n_rays, S=S))
    # ... and of the 2048-point tile of 128 buckets: T - 1 = 23 x 89, T, T + 1 = 3 x 683
    for n_rays, S in ((23, 89), (32, 64), (3, 683)):
        for fam in ("fx", "bf16"):
            out.append(_case(f"tile2048-{n_rays * S}-{fam}", fam, n_rays=n_rays, S=S, min_buckets=1))
    out.append(_case("ranks3-stride", "fx", n_rays=51, S=61, n_ranks=3, pad=4 * 61 + 2))       # 3111 points, 1037 per rank
    # level ranges at 64 buckets: split (64 nl < 256) and unsplit reducers, odd and even first levels
    for lv in ((0, 1), (15, 16), (5, 8), (12, 16)):
        for fam in ("fx", "fx_gather", "bf16"):
            out.append(_case(f"levels-{lv[0]}-{lv[1]}-{fam}", fam, levels=lv))
    # 1537 tiles: pass 1 takes all levels of the call per workgroup (the variant of large batches); two levels, a split reducer
    out.append(_case("many-tiles-fx", "fx", levels=(14, 16), n_rays=24577, S=64))
    # bucket plans
    for mb in (1, 2):
        for fam in ("fx", "bf16"):
            out.append(_case(f"buckets-{64 << mb}-{fam}", fam, min_buckets=mb, n_rays=71, S=64))
    for fam in ("fx", "bf16", "f32"):
        out.append(_case(f"log2T12-{fam}", fam, log2T=12, min_buckets=2))
    out.append(_case("log2T20-fx", "fx", log2T=20, n_rays=67, S=64, levels=(3, 9)))              # 128 buckets, 2048-point tile, start[] scan
    out.append(_case("log2T20-bf16", "bf16", log2T=20, n_rays=67, S=64, levels=(3, 9)))
    # level sizes that are no powers of two
    for fam in FAMILIES:
        out.append(_case(f"odd-sizes-{fam}", fam, offsets="odd"))
    # spill routes
    for fam in FAMILIES:
        out.append(_case(f"tiny-blocks-{fam}", fam, flags=("tiny",)))
    # ... and without the flag: every ray parallel to y or z, its x cell the last of a bucket's 256-row chunk on level AXIS_LAST_LEVEL --
    # all pairs of that level have their corners in two buckets, a tile emits twice its records there
    for fam in FAMILIES:
        out.append(_case(f"axis-last-{fam}", fam, rays="axis_last"))
    # merging
    for fam in ("fx", "bf16", "f32"):
        out.append(_case(f"runs-{fam}", fam, rays="runs", n_rays=37, S=64))
    # dynamic range
    for g in ("tiny_one", "zero", "chan0", "neg_level"):
        for fam in ("fx", "bf16"):
            out.append(_case(f"grad-{g}-{fam}", fam, grad=g))
    return {c["name"]: c for c in out}


CASES = _cases()


def offsets_of(case):
    offs = hashgrid_ref.level_offsets(case["L"], case["H"], case["log2T"], 3)
    if case["offsets"] == "odd":
        # level 0 keeps its dense 17^3; the rest are hashed behind a true modulo (12 288 = 3 * 2^12 and 16 383 among them), one is 2^14
        sizes = [4913, 10000, 16383, 777, 12288, 5001, 16384, 333] * 2
        sizes[0], sizes[8] = 4913, 9999
        assert max(sizes) <= 1 << case["log2T"] and len(sizes) == case["L"]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return offs


def _bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).astype(np.uint32)
    return r.view(np.float32)


def gradients(case, B):
    """The stored gradient values, float32 [B, L, C] (bf16 families: every value is a bf16)."""
    L, C = case["L"], case["C"]
    lb, le = case["levels"]
    rng = np.random.default_rng(sum(map(ord, case["name"])))
    g = rng.standard_normal((B, L, C)).astype(np.float32)
    kind = case["grad"]
    if kind == "tiny_one":
        g = (np.sign(g) * np.float32(2.0 ** -20)).astype(np.float32)
        g[B // 2, lb + (le - lb) // 2, 0] = 1.0
    elif kind == "zero":
        g[:] = 0.0
    elif kind == "chan0":
        g[:, :, 0] = 0.0
    elif kind == "neg_level":
        g[:, le - 1] = -np.abs(g[:, le - 1])
    elif kind != "normal":
        raise ValueError(kind)
    return g if case["family"] == "f32" else _bf16_round(g)


def _frac(x01, level, H):
    scale, _ = hashgrid_ref.level_scale_res(level, H)
    pos = hashgrid_ref._fma32(x01, scale, np.float32(0.5))
    return (pos - np.floor(pos)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """rays, depths, points, offsets, stored gradients and the prefill of a case (shared by every test; read-only)."""
    case = CASES[name]
    rays, z = make_rays(case["rays"], case["n_rays"], case["S"], seed=len(name) + case["n_rays"])
    x01 = positions(rays, z)
    offs = offsets_of(case)
    g = gradients(case, x01.shape[0])
    rng = np.random.default_rng(7)
    prefill = (rng.uniform(0.5, 1.0, (int(offs[-1]), case["C"])) * rng.choice([-1.0, 1.0], (int(offs[-1]), case["C"])) * 2.0 ** -12).astype(np.float32)
    for arr in (rays, z, x01, offs, g, prefill):
        arr.setflags(write=False)
    return rays, z, x01, offs, g, prefill


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict: s, a, n, p float64 [rows, C]; E (None when every gradient of the call is zero)."""
    case = CASES[name]
    _, _, x01, offs, g, _ = inputs(name)
    C, H = case["C"], case["H"]
    lb, le = case["levels"]
    rows_total = int(offs[-1])
    s, a, p = (np.zeros((rows_total, C)) for _ in range(3))
    n = np.zeros(rows_total)
    for lvl in range(lb, le):
        rows, w = hashgrid_ref.corners(x01, lvl, offs, H)
        fr = _frac(x01, lvl, H).astype(np.float64)
        wy, wz = np.stack([1 - fr[:, 1], fr[:, 1]], 1), np.stack([1 - fr[:, 2], fr[:, 2]], 1)
        gl = g[:, lvl].astype(np.float64)
        for c in range(8):
            t = w[:, c].astype(np.float64)[:, None] * gl
            pay = np.abs(gl) * (wy[:, (c >> 1) & 1] * wz[:, c >> 2])[:, None]
            for ch in range(C):
                s[:, ch] += np.bincount(rows[:, c], weights=t[:, ch], minlength=rows_total)
                a[:, ch] += np.bincount(rows[:, c], weights=np.abs(t[:, ch]), minlength=rows_total)
                p[:, ch] += np.bincount(rows[:, c], weights=pay[:, ch], minlength=rows_total)
            n += np.bincount(rows[:, c], minlength=rows_total)
    gmax = float(np.abs(g[:, lb:le]).max())
    ref = dict(s=s, a=a, p=p, n=np.repeat(n[:, None], C, axis=1), E=int(np.floor(np.log2(gmax))) if gmax > 0 else None)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def fx_shift(E):
    return 0 if E is None else min(25 - E, 120)


def _fp32_part(ref, prefill):
    return (ref["n"] + 8.0) * U23 * (ref["a"] + np.abs(prefill.astype(np.float64)))


def bound(family, ref, prefill):
    """Per element, see the module docstring."""
    n, a, p, E = ref["n"], ref["a"], ref["p"], ref["E"]
    F = _fp32_part(ref, prefill)
    if family in ("fx", "fx_gather"):
        quantum = 0.0 if E is None else 2.0 ** -fx_shift(E)
        return (2.0 ** -8 * a + 2.0 ** -15 * p) * (1 + 2.0 ** -7) + n * quantum / 2 + F
    quantum = 0.0 if E is None else 2.0 ** (E - 30)
    if family == "bf16":
        return 2.0 ** -8 * a * (1 + 2.0 ** -7) + n * quantum / 2 + F
    if family == "f32":
        return n * quantum / 2 + F
    raise ValueError(family)


def worst_use(got_rows, family, ref, prefill):
    """got_rows float32 [rows, C] -> (largest err / bound over the touched elements, number of elements outside the bound); untouched rows
    must equal the prefill bit for bit (asserted)."""
    hit = ref["n"] > 0
    assert np.array_equal(got_rows[~hit].view(np.uint32), prefill[~hit].view(np.uint32)), "a row no point touches has changed"
    err = np.abs(got_rows.astype(np.float64) - (ref["s"] + prefill.astype(np.float64)))
    b = bound(family, ref, prefill)
    if not hit.any():
        return 0.0, 0
    return float((err[hit] / b[hit]).max()), int((err[hit] > b[hit]).sum())


# ---- numpy restatement of the PairFx arithmetic (no binning) ------------------------------------------------------------------------
def fx_records(name):
    """One pair record per (point, level, k): dict of flat arrays -- level, point, row_a, row_b (absolute rows), pay float64 [N, C] (the
    bf16 payloads), fq (the 15-bit fraction as an integer), fx (the fp32 fraction), q float64 [N, C] = |g| w_y w_z."""
    case = CASES[name]
    _, _, x01, offs, g, _ = inputs(name)
    lb, le = case["levels"]
    out = {k: [] for k in ("level", "point", "row_a", "row_b", "pay", "fq", "fx", "q")}
    one = np.float32(1.0)
    for lvl in range(lb, le):
        rows, _ = hashgrid_ref.corners(x01, lvl, offs, case["H"])
        fr = _frac(x01, lvl, case["H"])
        wy, wz = [one - fr[:, 1], fr[:, 1]], [one - fr[:, 2], fr[:, 2]]
        fq = np.floor(fr[:, 0].astype(np.float64) * 32768.0).astype(np.int64)
        for k in range(4):
            wyz = (wy[k & 1] * wz[k >> 1]).astype(np.float32)
            pay = _bf16_round((wyz[:, None] * g[:, lvl]).astype(np.float32)).astype(np.float64)
            out["level"].append(np.full(len(fq), lvl)); out["point"].append(np.arange(len(fq)))
            out["row_a"].append(rows[:, 2 * k]); out["row_b"].append(rows[:, 2 * k + 1])
            out["pay"].append(pay); out["fq"].append(fq); out["fx"].append(fr[:, 0].astype(np.float64))
            out["q"].append(np.abs(g[:, lvl].astype(np.float64)) * wyz.astype(np.float64)[:, None])
    return {k: np.concatenate(v) for k, v in out.items()}


def fx_reduce(rec, E, prefill):
    """The reducer of scatter_v2.h on records `rec`: exact products, floor(v 2^shift + 0.5), integer sums, one rounding to fp32, `+=`."""
    rows_total, C = prefill.shape
    scale = 2.0 ** fx_shift(E)
    b = rec["pay"] * (rec["fq"] / 32768.0)[:, None]                        # exact in float64: 8 x 15 bits
    a = rec["pay"] - b                                                     # exact
    keep_b = rec.get("keep_b", 1.0)                                        # (fault injection: a second corner that never arrives)
    acc = np.zeros((rows_total, C))                                        # integers below 2^53: float64 sums them exactly
    for c in range(C):
        acc[:, c] = (np.bincount(rec["row_a"], weights=np.floor(a[:, c] * scale + 0.5), minlength=rows_total) +
                     np.bincount(rec["row_b"], weights=np.floor(b[:, c] * scale + 0.5) * keep_b, minlength=rows_total))
    sums = (acc / scale).astype(np.float32)                                # one rounding
    return (prefill + sums).astype(np.float32)
