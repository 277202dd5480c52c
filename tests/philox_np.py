"""numpy restatement of lrnde_sde_draw_noise (csrc/lrnde_noise.hpp) — a test helper, not a test.

Philox-4x32-10 (Salmon et al., SC'11) with the mulhi / mullo in uint64 arithmetic; normal j of column c = b*D + d in
stream s is word (j & 3) of the block at counter (j >> 2, c, s, 0), key (seed & 0xffffffff, seed >> 32), through
Box-Muller in float64 on the pairs (x0, x1), (x2, x3), rounded once to float32."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of uint32 words, key: 2; broadcast; returns the 4 output words as uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK for v in key)
    for r in range(10):
        if r:
            k0 = (k0 + W0) & _MASK
            k1 = (k1 + W1) & _MASK
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
    return [v.astype(np.uint32) for v in c]


def _u01(x):
    return ((x >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def _box_muller(a, b):
    r = np.sqrt(-2.0 * np.log(_u01(a)))
    th = 6.283185307179586 * _u01(b)
    return (r * np.cos(th)).astype(np.float32), (r * np.sin(th)).astype(np.float32)


def normals(seed, stream, nsteps, ncols):
    """(nsteps, ncols) float32 standard normals of lrnde_sde_draw_noise (the unscaled z)"""
    seed = int(seed)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    nq = (nsteps + 3) // 4
    q = np.arange(nq, dtype=np.uint64)[:, None]
    col = np.arange(ncols, dtype=np.uint64)[None, :]
    x = philox4x32_10((q, col, np.uint64(stream), np.uint64(0)), key)
    z0, z1 = _box_muller(x[0], x[1])
    z2, z3 = _box_muller(x[2], x[3])
    z = np.stack([z0, z1, z2, z3], axis=1).reshape(4 * nq, ncols)
    return z[:nsteps]


def increments(seed, stream, nsteps, B, D, scale):
    """cumulative = 0: (nsteps, B, D) = f32(z) * f32(scale)"""
    return (normals(seed, stream, nsteps, B * D) * np.float32(scale)).reshape(nsteps, B, D)


def path(seed, stream, nsteps, B, D, scale):
    """cumulative = 1: (nsteps + 1, B, D), row 0 zero, then the sequential float32 running sum of the increments"""
    inc = increments(seed, stream, nsteps, B, D, scale)
    return np.concatenate([np.zeros((1, B, D), np.float32), np.cumsum(inc, axis=0, dtype=np.float32)], axis=0)
