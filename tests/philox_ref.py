"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library) in
vectorised integer numpy, and the documented use gauss_sample_kernel (tmg_glue.hip) makes of it.  Host reference of the tests: no
code of the library.

  counter = (gq lo, gq hi, site, 0x7467), key = (k0.lo ^ k1.hi, k0.hi ^ k1.lo) of the two 64-bit words (k0, k1) of the key's row
  gq = (b % rows_per_key) nquad + q,  nquad = ceil(ppi Ch / 4): the counter restarts at every key
  element 4 q + e of image b, in flat (pixel, channel) order, takes normal e of quad q
  uniforms u = (x + 0.5) 2^-32 (exact in fp64); Box-Muller r = sqrt(-2 ln u1) with cos / sin of 2 pi u2: the words (x, y) of the
  quad give normals 0 (cos) and 1 (sin), the words (z, w) normals 2 and 3."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TAG = 0x7467


def _u64(v):
    return np.atleast_1d(np.asarray(v, dtype=np.uint64))


def philox4x32_10(ctr, key):
    """ctr: four, key: two arrays (or ints) of 32-bit words, broadcast against each other -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (_u64(c) for c in ctr)
    k0, k1 = (_u64(k) for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2               # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def key_words(k0, k1):
    """The 32-bit key pair of a key row (k0, k1): Python ints, signed (as torch's int64 holds them) or unsigned."""
    k0, k1 = int(k0) & (2 ** 64 - 1), int(k1) & (2 ** 64 - 1)
    return (k0 & 0xFFFFFFFF) ^ (k1 >> 32), (k0 >> 32) ^ (k1 & 0xFFFFFFFF)


def uniform(x):
    return (x.astype(np.float64) + 0.5) * 2.0 ** -32


def box_muller(u1, u2, use_sin):
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    return r * np.where(use_sin, np.sin(a), np.cos(a))


def draw_uniforms(B, ppi, Ch, keys, rows_per_key, site, gq_shift=None):
    """The uniforms behind every latent of a [B, ppi, Ch] draw: (u1, u2, use_sin), each [B, ppi * Ch] (fp64, fp64, bool).
    keys: [B / rows_per_key] rows (k0, k1).  gq_shift: optional int array [B, nquad] added to the counters (the sensitivity test)."""
    total = ppi * Ch
    nquad = (total + 3) // 4
    assert B % rows_per_key == 0 and len(keys) == B // rows_per_key
    q = np.arange(nquad, dtype=np.uint64)
    u1 = np.empty((B, 4 * nquad))
    u2 = np.empty((B, 4 * nquad))
    for b in range(B):
        gq = np.uint64(b % rows_per_key) * np.uint64(nquad) + q
        if gq_shift is not None:
            gq = (gq.astype(np.int64) + np.asarray(gq_shift[b], dtype=np.int64)).astype(np.uint64)
        x, y, z, w = philox4x32_10((gq & MASK, gq >> S32, site, TAG), key_words(*keys[b // rows_per_key]))
        ux, uy, uz, uw = uniform(x), uniform(y), uniform(z), uniform(w)
        u1[b] = np.stack((ux, ux, uz, uz), 1).reshape(-1)
        u2[b] = np.stack((uy, uy, uw, uw), 1).reshape(-1)
    use_sin = np.tile(np.array([False, True, False, True]), nquad)[None, :].repeat(B, 0)
    return u1[:, :total], u2[:, :total], use_sin[:, :total]


def normals(B, ppi, Ch, keys, rows_per_key=None, site=0, gq_shift=None):
    """fp64 latents [B, ppi, Ch] of a draw."""
    u1, u2, sn = draw_uniforms(B, ppi, Ch, keys, B if rows_per_key is None else rows_per_key, site, gq_shift)
    return box_muller(u1, u2, sn).reshape(B, ppi, Ch)
