"""tests/philox_ref.py, the host reference of the in-kernel latent draws, pinned to the published known answers of Random123
(kat_vectors, philox4x32 with 10 rounds: counter / key -> output) and to its own documented layout."""
import numpy as np

import common as C  # noqa: F401  (sets sys.path)
import philox_ref as P

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_known_answers():
    for ctr, key, out in KAT:
        got = tuple(int(v[0]) for v in P.philox4x32_10(ctr, key))
        assert got == out, (["%08x" % v for v in got], ["%08x" % v for v in out])


def test_known_answers_vectorised():
    """All three vectors in one call: the arrays broadcast, nothing leaks from one lane to the next."""
    ctr = [np.array([k[0][i] for k in KAT]) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT]) for i in range(2)]
    got = P.philox4x32_10(ctr, key)
    for n, (_, _, out) in enumerate(KAT):
        assert tuple(int(v[n]) for v in got) == out


def test_key_words_and_uniforms():
    k0, k1 = 0x8123456789abcdef, 0x0fedcba987654321
    assert P.key_words(k0, k1) == (0x89abcdef ^ 0x0fedcba9, 0x81234567 ^ 0x87654321)
    assert P.key_words(k0 - 2 ** 64, k1) == P.key_words(k0, k1)          # torch holds the words as signed int64
    u = P.uniform(np.array([0, 1, 2 ** 32 - 1], dtype=np.uint64))
    assert u[0] == 2.0 ** -33 and u[1] == 1.5 * 2.0 ** -32 and u[2] == 1.0 - 2.0 ** -33


def test_draw_layout():
    """Element 4 q + e of image b takes normal e of quad (b % rows_per_key) nquad + q; the last quad of 315 elements gives three."""
    B, ppi, Ch, site = 4, 63, 5, 5
    keys = [(11, -7), (2 ** 62 + 5, 3)]
    nquad = (ppi * Ch + 3) // 4
    assert nquad == 79 and ppi * Ch == 4 * 78 + 3
    e = P.normals(B, ppi, Ch, keys, rows_per_key=2, site=site).reshape(B, -1)
    assert e.shape == (B, 315) and np.isfinite(e).all()
    for b, q in ((0, 0), (1, 78), (3, 40)):
        gq = (b % 2) * nquad + q
        w = [int(v[0]) for v in P.philox4x32_10((gq, 0, site, 0x7467), P.key_words(*keys[b // 2]))]
        u = [(x + 0.5) * 2.0 ** -32 for x in w]
        r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
        want = [r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r1 * np.cos(2 * np.pi * u[3]), r1 * np.sin(2 * np.pi * u[3])]
        n = min(4, 315 - 4 * q)
        assert np.array_equal(e[b, 4 * q:4 * q + n], np.array(want[:n])), (b, q)
    # a member restarts the counter: with the same key, rows 0 and 2 draw the same numbers; another key or site does not
    same = P.normals(4, ppi, Ch, [keys[0], keys[0]], rows_per_key=2, site=site)
    assert np.array_equal(same[0], same[2]) and not np.array_equal(same[0], same[1])
    assert not np.array_equal(P.normals(2, ppi, Ch, [keys[0]], site=0), P.normals(2, ppi, Ch, [keys[0]], site=1))
    shifted = P.normals(2, ppi, Ch, [keys[0]], site=site, gq_shift=np.ones((2, nquad), dtype=np.int64))
    assert np.array_equal(shifted.reshape(2, -1)[0, :4 * 77], P.normals(2, ppi, Ch, [keys[0]], site=site).reshape(2, -1)[0, 4:4 * 78])
