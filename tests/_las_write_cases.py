"""The cases of the LAS encoder's tests: synthetic score tensors with the edges planted first, and the smallest shapes at which the
kernel can still go wrong.  A workgroup takes tiles of 256 output records, composes them in LDS and stores them 16 bytes at a time,
so T_out = 1, 255, 256, 257, 513 (one short, exact, one over, two tiles and one) and once 2^20 + 3 (more tiles than workgroups, a
tail whose byte count is no multiple of 16); every format at its least length; odd source lengths; every mask that gives another
alignment of the appended bytes (0, four bytes, two bytes only, 18, all 38)."""
import struct

import numpy as np

import _las_cases as C

CODES = (3, 2, 4, 5)
MASKS = (0, 0x001, 0x200, 0x2AA, 0x3FF)
NAN_PAYLOAD = struct.unpack("<f", struct.pack("<I", 0x7FC12345))[0]     # a quiet NaN that is not the default one
NEG_NAN = struct.unpack("<f", struct.pack("<I", 0xFFC00001))[0]

# (p_low, p_soil, p_medium, p_high, hits): exact ties in every pair of classes (the pair above the other two), all four equal, a NaN
# on a scored point in every position, -0.0 against 0.0, hits of 0, 1, 65535, 65536
_TIE = [(0.4, 0.4, 0.1, 0.1), (0.4, 0.1, 0.4, 0.1), (0.4, 0.1, 0.1, 0.4), (0.1, 0.4, 0.4, 0.1), (0.1, 0.4, 0.1, 0.4), (0.1, 0.1, 0.4, 0.4),
        (0.25, 0.25, 0.25, 0.25), (0.0, -0.0, 0.0, -0.0), (-0.0, 0.0, -0.0, 0.0)]
_NAN = [(np.nan, 0.2, 0.3, 0.1), (0.5, np.nan, 0.3, 0.1), (0.1, 0.2, np.nan, 0.3), (0.1, 0.2, 0.3, np.nan), (np.nan, np.nan, np.nan, 0.1),
        (np.nan, np.nan, np.nan, np.nan), (NAN_PAYLOAD, 0.7, 0.1, 0.1), (0.3, NEG_NAN, 0.6, 0.1)]
_PLAIN = [(0.7, 0.1, 0.1, 0.1), (0.1, 0.7, 0.1, 0.1), (0.1, 0.1, 0.7, 0.1), (0.1, 0.1, 0.1, 0.7)]
PLANTED_P = _TIE + _NAN + _PLAIN
PLANTED_HITS = [0, 1, 65535, 65536, 2, 70000, 2 ** 31 - 1, 0, 3]


def make_scores(S, seed=0):
    """-> (scores (8,S) fp32, weight (S) fp32, hits (S) int32): the planted rows first -- each probability row once with every
    planted hits value --, then seeded random ones of which a quarter is unscored (hits 0, NaN scores, weight 0, as
    sn2_points_finalize leaves them) and a tenth ties two classes."""
    rng = np.random.default_rng(5000 + seed)
    scores = rng.random((8, S), dtype=np.float32)
    weight = (rng.random(S, dtype=np.float32) * 3).astype(np.float32)
    hits = rng.integers(1, 9, size=S).astype(np.int32)
    tie = rng.random(S) < 0.1
    a, b = rng.integers(0, 4, size=S), rng.integers(0, 4, size=S)
    cols = np.arange(S)
    scores[4 + b[tie], cols[tie]] = scores[4 + a[tie], cols[tie]]
    un = rng.random(S) < 0.25
    scores[:, un] = np.nan
    weight[un] = 0.0
    hits[un] = 0
    n = 0
    for p in PLANTED_P:
        for h in PLANTED_HITS:
            if n >= S:
                break
            scores[4:8, n] = p
            scores[0:4, n] = (-0.0, NAN_PAYLOAD, 1.0, 0.5)
            weight[n] = -0.0 if h == 0 else 1.25
            hits[n] = h
            n += 1
    return scores, weight, hits


# (name, format, source record length or None = the least, T_out, field mask)
SHAPE_CASES = [(f"fmt{f}_least", f, None, 257, 0x3FF) for f in (0, 1, 2, 3, 6, 7, 8, 10)] + [
    ("fmt8_T1", 8, None, 1, 0x3FF), ("fmt8_T255", 8, None, 255, 0x2AA), ("fmt8_T256", 8, None, 256, 0x001),
    ("fmt8_T513", 8, None, 513, 0x200), ("fmt8_L39", 8, 39, 257, 0x3FF), ("fmt8_L41", 8, 41, 513, 0x2AA), ("fmt6_L33", 6, 33, 257, 0x200),
    ("fmt1_L33_T1", 1, 33, 1, 0x001),
] + [(f"fmt8_L39_mask{m:03x}", 8, 39, 257, m) for m in MASKS] + [(f"fmt3_mask{m:03x}", 3, None, 513, m) for m in MASKS]
SHAPE_IDS = [c[0] for c in SHAPE_CASES]


def source(fmt, L, T, seed=0):
    """(fields, T * L bytes) of T source records: the decoder's edge fields, the extra bytes a byte ramp that differs per record"""
    import _las_ref as R
    f = C.make_fields(T, seed)
    L = R.LAYOUTS[fmt][1] if L is None else L
    b = np.frombuffer(R.pack_records(f, fmt, L), dtype=np.uint8).reshape(T, L).copy()
    least = R.LAYOUTS[fmt][1]
    if L > least:
        b[:, least:] = (np.arange(T)[:, None] * 7 + np.arange(L - least)[None, :] * 13 + 1) % 251
    return f, b.tobytes()
