"""The numpy restatement of the device noise generator (tests/philox_np.py) against the Random123 known-answer vectors for
philox4x32-10, and the properties of its normals that need no GPU."""
import numpy as np

import philox_np as PX

# (counter, key, output) — Random123's kat_vectors for philox4x32_10
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_restatement_reproduces_the_random123_vectors():
    for ctr, key, want in KAT:
        got = tuple(int(v) for v in PX.philox4x32_10(ctr, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])


def test_restatement_normals_are_independent_of_batch_and_length_and_look_normal():
    seed = 0x0123456789ABCDEF
    a = PX.increments(seed, 0, 13, 7, 5, 1.0)
    b = PX.increments(seed, 0, 9, 3, 5, 1.0)
    assert np.array_equal(a[:9, :3], b)
    assert not np.array_equal(PX.increments(seed, 1, 9, 3, 5, 1.0), b)
    assert not np.array_equal(PX.increments(seed + 1, 0, 9, 3, 5, 1.0), b)
    W = PX.path(seed, 0, 13, 7, 5, 0.25)
    assert not W[0].any() and np.array_equal(W[1:], np.cumsum(PX.increments(seed, 0, 13, 7, 5, 0.25), axis=0, dtype=np.float32))
    z = PX.normals(7, 2, 512, 512).astype(np.float64).ravel()
    n = z.size
    assert abs(z.mean()) < 6 / np.sqrt(n) and abs(z.var() - 1) < 6 * np.sqrt(2 / n)
