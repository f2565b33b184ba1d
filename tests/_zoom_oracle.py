"""Float64 numpy restatement of the volume resize (include/naf_hip.h, V1) -- not a test module.

scipy.ndimage.zoom(a, out / in, order=3, prefilter=False) with its defaults: output j of an axis with a inputs and b outputs
sits at x = j (a - 1) / (b - 1) (x = j for b = 1), the taps floor(x) - 1 .. floor(x) + 2 carry the cubic B-spline weights, a tap
outside [0, a - 1] is mirrored about the edge samples, and nothing is prefiltered.  The sum is separable, so a dense [b, a] tap
matrix per axis applied with tensordot is the whole definition; no scipy is needed."""
import numpy as np

# the nine shape pairs the definition was checked on against scipy 1.15.3 (tests/golden/zoom_scipy.npz)
GOLDEN_PAIRS = [((5, 6, 7), (9, 4, 13)), ((8, 8, 8), (16, 16, 16)), ((12, 9, 10), (7, 9, 5)), ((3, 4, 2), (6, 3, 5)),
                ((8, 1, 5), (4, 3, 1)), ((1, 1, 1), (3, 2, 4)), ((2, 2, 2), (5, 1, 7)), ((6, 6, 6), (6, 6, 9)),
                ((40, 3, 17), (5, 8, 17))]


def mirror(i, a):
    """Whole-sample symmetric mirror of tap index i on an axis of a samples."""
    if a == 1:
        return 0
    p = 2 * (a - 1)
    i = i % p                      # Python's modulo is non-negative for p > 0
    return p - i if i >= a else i


def weights(t):
    """Cubic B-spline weights of the taps f - 1 .. f + 2 at fraction t."""
    return np.array([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6])


def taps(a, b, j):
    """(mirrored tap indices [4], weights [4]) of output j of an axis with a inputs and b outputs."""
    r = np.float64(a - 1) / np.float64(b - 1) if b > 1 else np.float64(1.0)
    x = np.float64(j) * r
    f = int(np.floor(x))
    return [mirror(f - 1 + k, a) for k in range(4)], weights(x - f)


def tap_matrix(a, b):
    """Dense [b, a] float64 matrix of one axis (mirrored taps that coincide add up)."""
    m = np.zeros((b, a), dtype=np.float64)
    for j in range(b):
        idx, w = taps(a, b, j)
        for i, v in zip(idx, w):
            m[j, i] += v
    return m


def support(a, b, j):
    """The set of input indices output j reads (zero-weight taps included)."""
    return set(taps(a, b, j)[0])


def zoom(vol, out_shape):
    """The definition: float64 [b1, b2, b3] from a [a1, a2, a3] volume."""
    v = np.asarray(vol, dtype=np.float64)
    for axis in range(3):
        m = tap_matrix(v.shape[axis], int(out_shape[axis]))
        v = np.moveaxis(np.tensordot(m, v, axes=([1], [axis])), 0, axis)
    return v


def zoom_at(vol, out_shape, idx):
    """One output voxel of zoom(vol, out_shape), from its 64 taps: for spot checks of outputs too large to form."""
    v = np.asarray(vol)
    t = [taps(v.shape[k], int(out_shape[k]), int(idx[k])) for k in range(3)]
    block = v[np.ix_(t[0][0], t[1][0], t[2][0])].astype(np.float64)
    return float(np.einsum("i,j,k,ijk->", t[0][1], t[1][1], t[2][1], block))


def inputs(shape, seed):
    """The golden inputs: uniform in [0.5, 1.5], float32."""
    return (0.5 + np.random.default_rng(seed).random(shape)).astype(np.float32)
