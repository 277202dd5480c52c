"""numpy restatement of the virtual Brownian tree (csrc/lrnde_sde_tree.hpp, include/lrnde.h) — a test helper,
not a test.

nfine = 2^L; z (nfine, ...) float32 standard normals, z[n] = normal n of each column; span = t2 - t0 in float32.  Every
operation is one float32 operation:
    W[0] = 0,  W[nfine] = sT z[0],  sT = f32(sqrt(f64(span)))
    level l = 1..L, node j = 0..2^(l-1)-1:  a = j 2^(L-l+1), b = a + 2^(L-l+1), mid = a + 2^(L-l), n = 2^(l-1) + j
    W[mid] = (0.5 (W[a] + W[b])) + (s_l z[n]),  s_l = f32(0.5 sqrt(f64(span) 2^-(l-1)))
`build` fills the whole array, `descend` computes one index by the descent from (0, nfine): L - ctz(k) levels."""
import numpy as np

f32 = np.float32


def scale_top(span):
    return f32(np.sqrt(np.float64(f32(span))))


def scale_level(span, l):
    return f32(0.5 * np.sqrt(np.float64(f32(span)) * 2.0 ** -(l - 1)))


def build(z, L, span):
    """(2^L + 1, ...) float32: the array of the definition, from z (at least 2^L rows)"""
    z = np.asarray(z, dtype=f32)
    nfine = 1 << L
    assert z.shape[0] >= nfine
    W = np.zeros((nfine + 1,) + z.shape[1:], f32)
    W[nfine] = scale_top(span) * z[0]
    for l in range(1, L + 1):
        step = 1 << (L - l + 1)
        half = step >> 1
        sl = scale_level(span, l)
        j = np.arange(1 << (l - 1))
        a = j * step
        mean = f32(0.5) * (W[a] + W[a + step])          # one float32 add, one float32 multiply
        W[a + half] = mean + sl * z[(1 << (l - 1)) + j]  # one multiply, one add
    return W


def descend(z, L, span, k):
    """W[k] alone, computing only the midpoints on the way down"""
    z = np.asarray(z, dtype=f32)
    nfine = 1 << L
    assert 0 <= k <= nfine
    wa = np.zeros(z.shape[1:], f32)
    if k == 0:
        return wa
    wb = (scale_top(span) * z[0]).astype(f32)
    a, b = 0, nfine
    if k == nfine:
        return wb
    for l in range(1, L + 1):
        mid = (a + b) >> 1
        n = (1 << (l - 1)) + (a >> (L - l + 1))
        wm = (f32(0.5) * (wa + wb) + scale_level(span, l) * z[n]).astype(f32)
        if mid == k:
            return wm
        if k < mid:
            b, wb = mid, wm
        else:
            a, wa = mid, wm
    raise AssertionError("unreachable")


def levels_of(k, L):
    """levels a query for k descends (0 for the two ends)"""
    if k == 0 or k == (1 << L):
        return 0
    return L - ((k & -k).bit_length() - 1)
