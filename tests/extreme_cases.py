"""Helper of the extreme-value tests (no test here): the rows and queries at the edges of what the engines claim to
serve, shared by the GPU tests (tests/test_extreme_values.py, tests/test_side_searches_extreme.py) and the CPU model of the
side searches (tests/test_side_extreme_model.py).  A seed or a generator in, arrays out; nothing here needs a GPU or the
package.  The filters bound rows whose sumsq is 0 or lies in (1e-24, 1e30) (norm_ok, k_misc.hip)."""
import numpy as np

POS_NAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
N_I8, BLOCK0, NBLOCK = 16384, 1000, 256
# binary16 storage: the largest half, the last float that still rounds to it, the first that rounds to Inf (both signs), the
# smallest subnormal half, a tie that rounds to zero, one that rounds up to it, a float far below it, and -0
F16_EDGE = np.array([65504.0, 65519.996, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 1e-8, -0.0],
                    dtype=np.float32)


def _scaled(rng, n, d, sumsq_lo, sumsq_hi):
    """n random directions with |x|^2 log-uniform in [sumsq_lo, sumsq_hi]"""
    g = rng.standard_normal((n, d))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    s2 = np.exp(rng.uniform(np.log(sumsq_lo), np.log(sumsq_hi), n))
    return (g * np.sqrt(s2)[:, None]).astype(np.float32)


def _kind_rows(kind, rng, n, d):
    if kind == "a_lo":
        return _scaled(rng, n, d, 2e-24, 4e-24)      # just inside the band's low edge
    if kind == "a_hi":
        return _scaled(rng, n, d, 2.5e29, 5e29)      # just inside the high edge
    if kind == "b_lo":
        return _scaled(rng, n, d, 2e-25, 5e-25)      # just outside
    if kind == "b_hi":
        return _scaled(rng, n, d, 2e30, 4e30)
    if kind == "c":                                  # products and sums are fp32 subnormals
        return (rng.standard_normal((n, d)) * 1e-21).astype(np.float32)
    if kind == "d":                                  # finite rows whose L2 distances overflow to +Inf
        return (rng.standard_normal((n, d)) * 1e19).astype(np.float32)
    if kind == "e":                                  # sumsq overflows, every component finite (cosine: a zero row)
        return (np.sign(rng.standard_normal((n, d))) * rng.uniform(1e37, 3e37, (n, d))).astype(np.float32)
    if kind == "f":
        return np.zeros((n, d), np.float32)
    if kind == "g":                                  # one non-finite component: +NaN, -NaN, +Inf, -Inf
        X = rng.standard_normal((n, d)).astype(np.float32)
        for i in range(n):
            X[i, (i * 7) % d] = (POS_NAN, NEG_NAN, np.inf, -np.inf)[i % 4]
        return X
    raise ValueError(kind)


KINDS = ["a_lo", "a_hi", "b_lo", "b_hi", "c", "d", "e", "f", "g"]
SAFE = {"a_lo", "a_hi", "f"}   # rows the filters still bound


def _ladder(kind, d, seed, n=N_I8):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    B = _kind_rows(kind, rng, NBLOCK, d)
    X[BLOCK0:BLOCK0 + NBLOCK] = B
    Q = rng.standard_normal((20, d)).astype(np.float32)
    near = B[[0, 1, 2, 3, 5]].copy()
    near[4] *= np.float32(1.0001)
    Q = np.concatenate([Q, near, np.zeros((1, d), np.float32)])
    return X, Q


def _odd_queries(rng, d):
    def band(s2):
        g = rng.standard_normal(d)
        return (g / np.linalg.norm(g) * np.sqrt(s2)).astype(np.float32)
    out = [np.zeros(d, np.float32)]
    for v in (POS_NAN, NEG_NAN, np.inf, -np.inf):
        q = rng.standard_normal(d).astype(np.float32)
        q[3] = v
        out.append(q)
    out += [band(2e-24), band(5e-25), band(5e29), band(2e30)]
    q = rng.standard_normal(d).astype(np.float32)
    q[0] = 1e15
    out.append(q)
    out.append((rng.standard_normal(d) * 1e-21).astype(np.float32))
    return out


ODD_AT = [0, 1, 2, 63, 64, 127, 128, 129, 200, 255, 256]
