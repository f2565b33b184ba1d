"""Float64 numpy restatement of the stand-alone ray-march operators (include/naf_hip.h R2, R4, R5, E2 and the running optical
depth of naf_render_forward_samples), written from the operations' definitions, plus a float32 rehearsal of each kernel's
arithmetic with a choice of summation order and a list of injectable faults.  tests/test_raymarch_oracle_cpu.py measures the
tolerances below from the two (never from a kernel) and shows that every fault lands outside them;
tests/test_hip_raymarch_reference.py holds the kernels to them.

Definitions (reference render.py:87-105, 113-126, 192-247, hashgrid.py:122-125):
  sample     t = linspace(0, 1, S) in fp32, z = near (1 - t) + far t, jittered inside its stratum [mid(s-1, s), mid(s, s+1)] by
             t_rand; pts = o + d z clamped to +-(bound - 1e-6).  fp32 throughout, in the kernel's op order: a bit-exact bar.
  integrate  acc[r] = sum_s sigma[r, s] dist[r, s], dist = (z[s+1] - z[s]) |d|, the last sample's distance 1e-10 |d|; the adjoint
             is grad_sigma[r, s] = grad_acc[r] dist[r, s].
  running_depth  tau[r, s] = sum_{s' <= s} sigma dist: a float64 cumulative sum.
  resample   w[s] = |sigma[s] - sigma[s-1]| / wmax (w[0] = 1e-10 / wmax), wmax = max(1e-10, the largest difference of the WHOLE
             call); pdf[i] = (w[i+1] + 1e-5) / total over the intervals i = 0 .. S-3, cdf[k] = sum_{i < k} pdf[i] at the S - 1 bin
             edges mid[k] = (z[k] + z[k+1]) / 2; a fine sample at u: k = #{cdf <= u} (right-sided search), below = max(k - 1, 0),
             above = min(k, S - 2), denom = cdf[above] - cdf[below], replaced by 1 where < 1e-5, t = (u - cdf[below]) / denom,
             depth = mid[below] + t (mid[above] - mid[below]); the row is the S coarse depths and the NF fine ones, sorted.
  normalize  out01 = (x + size) / (2 size) in fp32; flag = any x outside [-size, size] or NaN; min and max over the values that
             are not NaN (an input of NaN alone leaves the two words as the caller set them).

Decisions near a threshold.  A fine sample's depth is continuous in u across a cdf entry between two ordinary intervals, but
not next to an interval that takes the `denom < 1e-5` rule (there t is u - cdf[below], about 0, for the whole interval: the depth
jumps by a bin at its upper end), and `denom` against 1e-5 itself is a jump.  `resample` therefore returns, for every fine sample,
its admissible alternatives: the depths with each decision taken the other way wherever the float64 operand lies within DELTA of
the threshold (u against a cdf entry: the search index one lower or higher; denom against 1e-5: the other rule).  A sample is
UNDECIDED when an alternative differs from its depth by more than TOL_DEPTH -- alternatives that agree decide nothing.
`match_rows` accepts a kernel row that equals, within TOL_DEPTH, the sorted row of some combination of admissible depths; a ray
with more than three undecided samples is skipped.  The deterministic draw's u = 1.0 goes through the same
mechanism: it sits on the last cdf entry, both decisions give the last bin edge, so it is decided.

Tolerances: 8 x the worst float32-against-float64 figure of tests/test_raymarch_oracle_cpu.py over all its cases and three
summation orders (sequential, the kernel's 64-lane / tile shuffle tree with per-chunk carry, reversed), rounded up to one digit.
Measured there when the module was added (worst figure -> tolerance):
  cdf entries            1.4e-7 absolute in the kernel's order -> DELTA 2e-6.  Sequential and reversed sums err by up to 1.8e-6
                         (255 terms) and 2.7e-6 (a constant ray's 193 equal terms, which round the same way every time): 8 x that
                         would leave every ray of the S = 1 024 case undecided, so DELTA is taken from the kernel's order.  It
                         is the stricter choice: a smaller delta admits fewer alternatives.
  resampled depths       2.1e-7 m in the kernel's order, 7.3e-7 m reversed at S = 1 024 (8 x: 6e-6) -> TOL_DEPTH 3e-6 m, the cap
                         and the bar the suite already had: the figure above the cap belongs to a summation order the kernel
                         does not use, so the cap is kept rather than raised.
  weights                1.0e-7 of the largest    -> TOL_WEIGHT 9e-7    (cap 1e-6)
  integrals              1.1e-7 of sum|sigma dist| -> TOL_SUM 9e-7      (cap 2e-6)
  tau                    1.7e-7 of sum|sigma dist| of the prefix -> TOL_TAU 2e-6 (the cap)
  grad_sigma             1.6e-7 relative          -> TOL_GRAD  2e-6
grad_sigma is "one product" of grad_acc with dist, but dist = (z[s+1] - z[s]) |d| carries the roundings of |d| (three squares, two
sums, a square root) and of its own product, about 2.5 ulp in all before the last product: 8 x that is 2e-6, not a few ulp, and
no tighter figure would be a measurement.  The random sigma of the resampling cases is a walk with steps of 0.5 .. 1 times its
largest step and either sign: every interval then has a weight of at least half the largest and the depth's sensitivity to a cdf
error, (mid[above] - mid[below]) / denom, stays near the ray's length; with independent sigma some interval has a weight of a few
1e-3, a denom just above 1e-5, and turns a cdf error of 1e-7 into 1e-5 m of depth -- the conditioning of the operation at that
sample, not a property of the kernel."""
import itertools

import numpy as np

f32 = np.float32
EPS_PDF = float(f32(1e-5))          # the kernel's constants are fp32 literals
FLOOR_W = float(f32(1e-10))
LAST_DIST = float(f32(1e-10))

DELTA = 2e-6
TOL_DEPTH = 3e-6
TOL_WEIGHT = 9e-7
TOL_SUM = 9e-7
TOL_TAU = 2e-6
TOL_GRAD = 2e-6
CAPS = dict(depth=3e-6, weight=1e-6, sum=2e-6)


# ---- sampling: fp32, the kernel's op order -------------------------------------------------------------------------------------
def lin_t(S):
    """torch.linspace(0, 1, S) in fp32: i * step below S / 2, fma(-(S - 1 - i), step, 1) above (one step: [0])."""
    if S == 1:
        return np.zeros(1, f32)
    step = f32(1.0) / f32(S - 1)
    i = np.arange(S)
    low = i.astype(f32) * step
    high = (1.0 - (S - 1 - i).astype(np.float64) * np.float64(step)).astype(f32)      # exact in float64, rounded once: the fma
    return np.where(i < S // 2, low, high).astype(f32)


def sample(rays, t_rand, S, perturb, bound):
    """-> z [n, S], pts [n, S, 3], both fp32 and bit for bit what the kernel's op order gives."""
    rays = np.asarray(rays, f32)
    near, far = rays[:, 6:7], rays[:, 7:8]
    t = lin_t(S)[None, :]
    z = near * (f32(1.0) - t) + far * t
    if perturb:
        mids = f32(0.5) * (z[:, 1:] + z[:, :-1])
        lower = np.concatenate([z[:, :1], mids], 1)
        upper = np.concatenate([mids, z[:, -1:]], 1)
        z = lower + (upper - lower) * np.asarray(t_rand, f32)
    lim = f32(bound) - f32(1e-6)
    p = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    p = np.where(p < -lim, -lim, p)
    p = np.where(p > lim, lim, p)
    return z.astype(f32), p.astype(f32)


# ---- line integral, adjoint, running depth: float64 ----------------------------------------------------------------------------
def distances(z, rays):
    z, d = np.asarray(z, np.float64), np.asarray(rays, np.float64)[:, 3:6]
    dn = np.sqrt((d * d).sum(-1, keepdims=True))
    return np.concatenate([z[:, 1:] - z[:, :-1], np.full((z.shape[0], 1), LAST_DIST)], 1) * dn


def integrate(sigma, z, rays):
    """-> acc [n] and its scale sum_s |sigma dist| [n]."""
    term = np.asarray(sigma, np.float64) * distances(z, rays)
    return term.sum(-1), np.abs(term).sum(-1)


def sum_fraction(got, ref, scale, tol):
    """The worst |got - ref| / scale of the rays that carry weight, as a fraction of `tol` (NaN if any of them is NaN: the callers
    assert `< 1.0`, which a NaN fails)."""
    live = scale > 0
    err = np.abs(np.asarray(got, np.float64) - ref)[live] / scale[live]
    return float("nan") if np.isnan(err).any() else float(err.max()) / tol


def integrate_adjoint(grad_acc, z, rays):
    return np.asarray(grad_acc, np.float64)[:, None] * distances(z, rays)


def running_depth(sigma, z, rays):
    """-> tau [n, S] and the scale of each prefix, cumsum |sigma dist|."""
    term = np.asarray(sigma, np.float64) * distances(z, rays)
    return np.cumsum(term, -1), np.cumsum(np.abs(term), -1)


# ---- coarse -> fine resampling: float64 ------------------------------------------------------------------------------------------
def weights(sigma):
    """-> w [n, S] and wmax, the maximum over the whole call with its floor."""
    sg = np.asarray(sigma, np.float64)
    diff = np.abs(sg[:, 1:] - sg[:, :-1])
    wmax = max(FLOOR_W, float(diff.max()) if diff.size else 0.0)
    return np.concatenate([np.full((sg.shape[0], 1), FLOOR_W), diff], 1) / wmax, wmax


def _interp(cdf, mid, u, k, rule):
    """The depth of u with the search result k and the denom rule forced (True: denom := 1, False: as is, None: by value)."""
    M = cdf.shape[0]
    below, above = max(k - 1, 0), min(k, M - 1)
    denom = cdf[above] - cdf[below]
    if rule is None:
        rule = denom < EPS_PDF
    if rule:
        denom = 1.0
    if denom == 0.0:
        return None
    return mid[below] + (u - cdf[below]) / denom * (mid[above] - mid[below])


def resample(sigma, z, u, NF, det, delta=DELTA, tol=TOL_DEPTH):
    """-> dict(weights, wmax, pdf, cdf, mid, fine [n, NF], row [n, S + NF], alts: {(ray, j): [other admissible depths]}).
    `alts` holds the UNDECIDED samples only (module docstring); `cands` every admissible depth of every sample that has a decision
    within delta of its threshold, the agreeing ones included."""
    z = np.asarray(z, np.float64)
    n, S = z.shape
    w, wmax = weights(sigma)
    pw = w[:, 1:S - 1] + EPS_PDF
    pdf = pw / pw.sum(-1, keepdims=True)
    cdf = np.concatenate([np.zeros((n, 1)), np.cumsum(pdf, -1)], 1)            # [n, S - 1]
    mid = 0.5 * (z[:, 1:] + z[:, :-1])
    M = S - 1
    if det:
        u = np.broadcast_to(lin_t(NF).astype(np.float64), (n, NF))
    u = np.asarray(u, np.float64)
    fine = np.empty((n, NF))
    alts, cands = {}, {}
    for r in range(n):
        c, m = cdf[r], mid[r]
        k = np.searchsorted(c, u[r], side="right")
        below, above = np.maximum(k - 1, 0), np.minimum(k, M - 1)
        denom = c[above] - c[below]
        small = denom < EPS_PDF
        t = (u[r] - c[below]) / np.where(small, 1.0, denom)
        fine[r] = m[below] + t * (m[above] - m[below])
        # candidates: a cdf entry within delta of u, or a denom within delta of the threshold -- its own or, through the search
        # index, a neighbour's
        near_entry = np.abs(c[np.minimum(k, M - 1)] - u[r]) <= delta
        near_entry |= np.abs(c[np.maximum(k - 1, 0)] - u[r]) <= delta
        near_denom = np.abs(denom - EPS_PDF) <= delta
        for j in np.nonzero(near_entry | near_denom)[0]:
            ks = {int(k[j])}
            for kk in (int(k[j]) - 1, int(k[j]) + 1):
                # one lower undoes "cdf[k - 1] <= u", one higher takes "cdf[k] <= u": admissible when that entry is within delta
                idx = int(k[j]) - 1 if kk < k[j] else int(k[j])
                if 0 <= kk <= M and 0 <= idx < M and abs(c[idx] - u[r, j]) <= delta:
                    ks.add(kk)
            vals = []
            for kk in ks:
                b, a = max(kk - 1, 0), min(kk, M - 1)
                d = c[a] - c[b]
                rules = [None] if abs(d - EPS_PDF) > delta else [True, False]
                for rule in rules:
                    v = _interp(c, m, u[r, j], kk, rule)
                    if v is not None:
                        vals.append(v)
            cands[(r, int(j))] = vals
            other = [v for v in vals if abs(v - fine[r, j]) > tol]
            if other:
                alts[(r, int(j))] = other
    row = np.sort(np.concatenate([z, fine], 1), -1)
    return dict(weights=w, wmax=wmax, pdf=pdf, cdf=cdf, mid=mid, fine=fine, row=row, alts=alts, cands=cands, z=z)


def undecided_by_ray(res):
    per = {}
    for (r, j) in res["alts"]:
        per.setdefault(r, []).append(j)
    return per


def exclusion(res):
    """-> (fraction of rays skipped: more than three undecided samples; fraction with any undecided sample)."""
    per = undecided_by_ray(res)
    n = res["z"].shape[0]
    return sum(len(v) > 3 for v in per.values()) / n, len(per) / n


def match_rows(res, got, tol=TOL_DEPTH):
    """Compare the kernel's rows `got` [n, S + NF] with the oracle's.  -> dict(worst: largest |difference| of the rows that matched
    directly or through an alternative, skipped, through_alternative, failed: [(ray, difference)])."""
    got = np.asarray(got, np.float64)
    diff = np.abs(got - res["row"])
    diff = np.where(np.isnan(diff), np.inf, diff).max(-1)
    per = undecided_by_ray(res)
    out = dict(worst=0.0, skipped=0, through_alternative=0, failed=[])
    for r in range(got.shape[0]):
        if r in per and len(per[r]) > 3:
            out["skipped"] += 1
            continue
        best = diff[r]
        if best > tol and r in per:
            js = per[r]
            for combo in itertools.product(*[[res["fine"][r, j]] + res["alts"][(r, j)] for j in js]):
                fine = res["fine"][r].copy()
                fine[js] = combo
                d = np.abs(got[r] - np.sort(np.concatenate([res["z"][r], fine])))
                d = np.inf if np.isnan(d).any() else d.max()
                if d < best:
                    best = d
            if best <= tol:
                out["through_alternative"] += 1
        if best > tol:
            out["failed"].append((r, float(best)))
        else:
            out["worst"] = max(out["worst"], float(best))
    return out


def contains_coarse(got, z, chunk=128):
    """Every coarse depth appears in its row bit for bit, as often as it occurs (multiset)."""
    got, z = np.asarray(got, f32), np.asarray(z, f32)
    for a in range(0, got.shape[0], chunk):
        g, c = got[a:a + chunk], z[a:a + chunk]
        in_row = (g[:, :, None] == c[:, None, :]).sum(1)               # [rays, S]: occurrences of each coarse depth in the row
        in_z = (c[:, :, None] == c[:, None, :]).sum(1)
        if not (in_row >= in_z).all():
            return False
    return True


# ---- encoder range check ---------------------------------------------------------------------------------------------------------
def ordered_int(v):
    """The order-preserving int32 of an fp32 value: its bits, the lower 31 flipped for a negative one."""
    i = np.asarray(v, f32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF).astype(np.int64)


def unordered_float(i):
    i = int(i)
    i = i if i >= 0 else i ^ 0x7FFFFFFF
    return float(np.array([i & 0xFFFFFFFF], dtype=np.uint32).view(f32)[0])


INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def normalize(x, size):
    """-> out01 (fp32, bit-exact bar), flag, min, max; min / max are None for an input of NaN alone."""
    x = np.asarray(x, f32)
    s = f32(size)
    out01 = (x + s) / (f32(2.0) * s)
    flag = bool((~((x >= -s) & (x <= s))).any())
    real = x[~np.isnan(x)]
    if real.size == 0:
        return out01, flag, None, None
    return out01, flag, float(real.min()), float(real.max())


# =================================================================================================================================
# float32 rehearsals of the kernels' arithmetic.  order: "seq", "tree" (as the kernel sums) or "rev"; fault: one name of FAULTS.
# =================================================================================================================================
# "truncated" is the issue's "z_out truncated at P" read as a sort network one power of two short, so that the row ends at P / 2: P
# itself is never below S + NF, and a cut there could touch no row.
FAULTS = ("carry_dropped", "carry_lane62", "left_search", "no_eps", "last_in_total", "max_per_ray", "no_floor", "finite_pad",
          "sort_pair", "truncated", "last_dist_zero", "last_dist_prev", "tau_carry_w2", "tau_restart", "tail_dropped",
          "no_sign_fold", "nan_lost")


def _butterfly(part):
    """The xor-shuffle tree over 64 lanes: every lane ends with the same sum; lane 0's."""
    v = part.astype(f32)
    lanes = np.arange(v.shape[-1])
    off = v.shape[-1] // 2
    while off:
        v = v + v[..., lanes ^ off]
        off //= 2
    return v[..., 0]


def _lane_sum(term, order, lanes=64):
    """sum over the last axis in fp32: sequential, reversed, or lane-strided partials joined by the shuffle tree."""
    term = term.astype(f32)
    n, S = term.shape
    if order == "seq":
        return np.cumsum(term, -1, dtype=f32)[:, -1] if S else np.zeros(n, f32)
    if order == "rev":
        return np.cumsum(term[:, ::-1], -1, dtype=f32)[:, -1] if S else np.zeros(n, f32)
    pad = (-S) % lanes
    t = np.concatenate([term, np.zeros((n, pad), f32)], 1).reshape(n, -1, lanes)
    part = np.zeros((n, lanes), f32)
    for k in range(t.shape[1]):
        part = part + t[:, k]
    return _butterfly(part)


def _scan(term, order, W, fault=None):
    """Inclusive prefix sums of the last axis in fp32: sequential, each prefix summed backwards, or W-lane Hillis-Steele chunks
    with the carry of the chunk's last lane (the kernels' scan)."""
    term = term.astype(f32)
    n, S = term.shape
    if order == "seq":
        return np.cumsum(term, -1, dtype=f32)
    if order == "rev":
        out = np.empty_like(term)
        for k in range(S):
            out[:, k] = np.cumsum(term[:, k::-1], -1, dtype=f32)[:, -1]
        return out
    pad = (-S) % W
    t = np.concatenate([term, np.zeros((n, pad), f32)], 1)
    out = np.empty_like(t)
    carry = np.zeros(n, f32)
    for base in range(0, t.shape[1], W):
        v = t[:, base:base + W].copy()
        d = 1
        while d < W:
            v[:, d:] = v[:, d:] + v[:, :-d]
            d *= 2
        v = v + carry[:, None]
        out[:, base:base + W] = v
        carry = v[:, W - 1]
        if fault in ("carry_dropped", "tau_restart"):
            carry = np.zeros(n, f32)
        elif fault in ("carry_lane62", "tau_carry_w2"):
            carry = v[:, W - 2]
    return out[:, :S]


def distances_f32(z, rays, fault=None):
    z, d = np.asarray(z, f32), np.asarray(rays, f32)[:, 3:6]
    dn = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    n, S = z.shape
    last = np.full((n, 1), f32(1e-10))
    if fault == "last_dist_zero":
        last[:] = 0
    elif fault == "last_dist_prev" and S > 1:
        last = z[:, -1:] - z[:, -2:-1]
    return (np.concatenate([z[:, 1:] - z[:, :-1], last], 1) * dn).astype(f32)


def integrate_f32(sigma, z, rays, order="tree", fault=None):
    return _lane_sum(np.asarray(sigma, f32) * distances_f32(z, rays, fault), order)


def integrate_adjoint_f32(grad_acc, z, rays, fault=None):
    return np.asarray(grad_acc, f32)[:, None] * distances_f32(z, rays, fault)


def running_depth_f32(sigma, z, rays, order="tree", W=16, fault=None):
    return _scan(np.asarray(sigma, f32) * distances_f32(z, rays), order, W, fault)


def resample_f32(sigma, z, u, NF, det, order="tree", fault=None):
    """-> dict(weights, wmax, cdf, fine, row): the kernel's arithmetic, fp32 step by step."""
    sg, z = np.asarray(sigma, f32), np.asarray(z, f32)
    n, S = z.shape
    diff = np.abs(sg[:, 1:] - sg[:, :-1])
    floor = f32(0.0) if fault == "no_floor" else f32(1e-10)
    wmax = np.full((n, 1), max(floor, diff.max()), f32)
    if fault == "max_per_ray":
        wmax = np.maximum(floor, diff.max(-1, keepdims=True)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.concatenate([np.full((n, 1), f32(1e-10)), diff], 1) / wmax
        eps = f32(0.0) if fault == "no_eps" else f32(1e-5)
        pw = (w[:, 1:S - 1] + eps).astype(f32)
        tot_terms = (w[:, 1:] + eps).astype(f32) if fault == "last_in_total" else pw
        # the kernel's lanes hold sample s = interval s - 1: lane partials are strided by sample index
        total = _lane_sum(np.concatenate([np.zeros((n, 1), f32), tot_terms], 1), order)[:, None]
        pdf = (pw / total).astype(f32)
    cdf = np.concatenate([np.zeros((n, 1), f32), _scan(pdf, order, 64, fault)], 1)
    M = S - 1
    if det:
        u = np.broadcast_to(lin_t(NF), (n, NF))
    u = np.asarray(u, f32)
    fine = np.empty((n, NF), f32)
    for a in range(0, n, 256):
        c, uu = cdf[a:a + 256], u[a:a + 256]
        hit = (c[:, None, :] < uu[:, :, None]) if fault == "left_search" else (c[:, None, :] <= uu[:, :, None])
        k = hit.sum(-1)
        below, above = np.maximum(k - 1, 0), np.minimum(k, M - 1)
        c0, c1 = np.take_along_axis(c, below, 1), np.take_along_axis(c, above, 1)
        denom = c1 - c0
        denom = np.where(denom < f32(1e-5), f32(1.0), denom)
        t = (uu - c0) / denom
        mid = f32(0.5) * (z[a:a + 256, 1:] + z[a:a + 256, :-1])
        b0, b1 = np.take_along_axis(mid, below, 1), np.take_along_axis(mid, above, 1)
        fine[a:a + 256] = b0 + t * (b1 - b0)
    P = 2
    while P < S + NF:
        P *= 2
    pad = np.full((n, P - S - NF), f32(1.0) if fault == "finite_pad" else f32(np.inf))
    merged = np.sort(np.concatenate([z, fine, pad], 1), -1)
    if fault == "sort_pair":
        merged[:, [0, P // 2]] = merged[:, [P // 2, 0]]
    row = merged[:, :S + NF].copy()
    if fault == "truncated":
        row[:, P // 2:] = np.nan                                          # a network one power of two short: the rest never written
    return dict(weights=w.astype(f32), wmax=wmax, cdf=cdf, fine=fine, row=row)


def normalize_f32(x, size, fault=None):
    """-> flag, ordered-int min word, ordered-int max word as the kernel leaves them (caller's initial {0, INT32_MAX, INT32_MIN})."""
    x = np.asarray(x, f32)
    s = f32(size)
    real = x[~np.isnan(x)]
    flag = bool((~((x >= -s) & (x <= s))).any())
    if fault == "nan_lost":                                               # fminf / fmaxf drop a NaN: the range test never sees it
        flag = bool(((real < -s) | (real > s)).any())
    if real.size == 0:
        return flag, INT32_MAX, INT32_MIN
    if fault == "no_sign_fold":
        o = real.view(np.int32).astype(np.int64)
    else:
        o = ordered_int(real)
    return flag, int(o.min()), int(o.max())


def grid_tail_dropped(values, cap):
    """A grid-stride loop that never loops: elements past the grid's first trip keep the guard value."""
    out = np.array(values, dtype=np.float64).reshape(-1)
    out[cap:] = np.nan
    return out.reshape(np.shape(values))


# ---- the cases both test modules share -------------------------------------------------------------------------------------------
def make_rays(n, seed):
    """Rays with directions that are not unit vectors (cone-beam style) and per-ray near / far."""
    g = np.random.default_rng(seed)
    o = g.normal(size=(n, 3)) * 0.1
    d = g.normal(size=(n, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * (0.6 + 0.9 * g.random((n, 1)))
    near = 0.7 + 0.2 * g.random((n, 1))
    far = near + 0.2 + 0.3 * g.random((n, 1))
    return np.concatenate([o, d, near, far], 1).astype(f32)


def make_sigma(pattern, n, S, seed):
    g = np.random.default_rng(seed)
    if pattern == "walk":                                  # "random": module docstring, last paragraph
        step = (0.5 + 0.5 * g.random((n, S))) * np.where(g.random((n, S)) < 0.5, -1.0, 1.0)
        return (0.05 * np.cumsum(step, -1)).astype(f32)
    if pattern == "constant":
        return np.full((n, S), 0.37, f32)
    if pattern == "spike":
        sg = np.zeros((n, S), f32)
        sg[np.arange(n), g.integers(1, S - 1, n)] = 1.0
        return sg
    if pattern == "ramp":
        return (np.arange(S, dtype=f32)[None, :] * f32(0.03125) + np.arange(n, dtype=f32)[:, None] * f32(0.5)).astype(f32)
    if pattern == "one_constant":
        sg = make_sigma("walk", n, S, seed)
        sg[n // 2] = 0.25
        return sg
    if pattern == "max_last":                              # the call's maximum in the very last element and nowhere else
        sg = make_sigma("walk", n, S, seed)
        sg[-1, -1] = sg[-1, -2] + f32(1.0)                 # a step of 1.0; every other step is below 0.05
        return sg
    raise ValueError(pattern)


# (name, n, S, NF, sigma pattern, det): what each reaches is in tests/test_hip_raymarch_reference.py
RESAMPLE_CASES = [
    ("s3", 9, 3, 1, "walk", False), ("s4", 9, 4, 2, "walk", False),
    ("p_exact", 37, 64, 64, "walk", False), ("p_plus1", 37, 64, 65, "one_constant", False),
    ("one_chunk", 37, 66, 1, "ramp", False), ("first_carry", 37, 67, 61, "walk", False),
    ("first_carry_spike", 101, 67, 61, "spike", False), ("first_carry_constant", 5, 67, 61, "constant", False),
    ("p512", 19, 130, 127, "walk", False), ("three_chunks", 19, 195, 64, "one_constant", False),
    ("lds_64k", 5, 1024, 1024, "walk", False),
    ("second_ray", 32768 + 7, 3, 1, "walk", False), ("second_max_trip", 4100, 257, 3, "max_last", False),
    ("det1", 9, 67, 1, "walk", True), ("det2", 9, 67, 2, "ramp", True), ("det64", 9, 67, 64, "walk", True),
]


def resample_inputs(case):
    name, n, S, NF, pattern, det = case
    seed = sum(map(ord, name))
    g = np.random.default_rng(seed + 1)
    rays = make_rays(n, seed + 2)
    t_rand = g.random((n, S)).astype(f32)
    u = None if det else g.random((n, NF)).astype(f32)
    sigma = make_sigma(pattern, n, S, seed + 3)
    return rays, t_rand, sigma, u


INTEGRATE_S = (1, 2, 63, 64, 65, 129)


def integrate_inputs(n, S, seed=5):
    """Mixed-sign sigma (cancellation), one all-zero ray, non-unit directions; depths as the sampler gives them."""
    g = np.random.default_rng(seed + S)
    rays = make_rays(n, seed + 11)
    z = sample(rays, g.random((n, max(S, 2))).astype(f32), max(S, 2), True, 0.3)[0][:, :S]
    sigma = g.normal(size=(n, S)).astype(f32)
    sigma[n // 2] = 0.0
    grad = g.normal(size=n).astype(f32)
    return rays, np.ascontiguousarray(z), sigma, grad
