"""numpy twin of csrc/rng.h for the tests that feed the library the very bits its Philox mode draws (not collected by pytest):
Philox4x32-10, the keep-bits of one nn.Dropout(0.5) call, the per-row uniforms, and the explicit icz_rng arrays of a whole BUTD
rollout / XE pass built from a seed."""
import numpy as np

RNG_EMB, RNG_ATT, RNG_OUT, RNG_UNIFORM = 1, 2, 3, 4       # csrc/rng.h: RngStream
RNG_SS_GATE, RNG_SS_DRAW = 5, 6                           # the gate and the draw of scheduled sampling (ss_select_kernel)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """numpy twin of csrc/rng.h (Philox4x32-10): uint32 arrays in, four uint32 arrays out."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(0xFFFFFFFF), p1 >> np.uint64(32), p1 & np.uint64(0xFFFFFFFF)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def _keep_bits(seed, stream, step, n):
    """keep flags of elements 0..n-1 of one dropout call: bit (idx & 31) of word (idx >> 5) & 3 of the Philox block idx >> 7."""
    idx = np.arange(n, dtype=np.uint64)
    g = idx >> np.uint64(7)
    gu = np.unique(g)
    r = _philox4x32_10(gu & np.uint64(0xFFFFFFFF), gu >> np.uint64(32), np.full(gu.shape, step), np.full(gu.shape, stream),
                       seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(r, 1)[g.astype(np.int64), ((idx >> np.uint64(5)) & np.uint64(3)).astype(np.int64)]
    return ((words >> (idx & np.uint64(31))) & np.uint64(1)).astype(np.uint8)


def _uniforms(seed, T, B, stream=RNG_UNIFORM):
    """rng_uniform of csrc/rng.h for steps 0..T-1 and rows 0..B-1: counter (row, 0, step, stream), the top 24 bits of word 0 -> [T, B] fp32"""
    rows = np.arange(B, dtype=np.uint64)
    return np.stack([(_philox4x32_10(rows, np.zeros(B), np.full(B, t), np.full(B, stream), seed & 0xFFFFFFFF, seed >> 32)[0] >> np.uint64(8))
                     .astype(np.float32) / np.float32(16777216.0) for t in range(T)])


def butd_rng_arrays(seed, T, B, R, E, A, H):
    """What the BUTD handle draws in Philox mode from `seed` for B rows x T steps, as the explicit arrays of make_rng: uniforms [T, B] fp32,
    embedding / attention / output keep-masks [T, B, E] / [T, B, R, A] / [T, B, H] uint8 (element index = position in the step's array)."""
    em = np.stack([_keep_bits(seed, RNG_EMB, t, B * E).reshape(B, E) for t in range(T)])
    am = np.stack([_keep_bits(seed, RNG_ATT, t, B * R * A).reshape(B, R, A) for t in range(T)])
    om = np.stack([_keep_bits(seed, RNG_OUT, t, B * H).reshape(B, H) for t in range(T)])
    return _uniforms(seed, T, B), em, am, om
