"""The cases of the LAS decoder's tests: the smallest shapes at which the kernel can still go wrong.  A workgroup takes 256
records and stages them with 16-byte loads, so T = 1, 255, 256, 257 (one short, exact, one over) and 2^20 + 3 (4097 workgroups, a
tail whose byte count is no multiple of 16); every format at its least record length; odd lengths (nothing aligned); the longest
staged length (128) and one beyond it (131: the field-by-field form).  The field values plant the edges first and fill up with
seeded random ones."""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# Lambert-93 centimetres: x about 650 km, y about 6 860 km
EDGE_XYZ = [I32_MIN, I32_MAX, 0, -1, 1, -123456789, 65012345, 686012345, 68601234 * 10 + 7, 99, -100, 100, 50, -50, I32_MIN + 1, I32_MAX - 1]
EDGE_U16 = [0, 32768, 65535, 1, 32767, 255, 256, 65534]
EDGE_RETURNS = [0x00, 0xFF, 0x5A, 0xA5, 0x07, 0x38, 0x0F, 0xF0, 0x11, 0x12]
EDGE_CLASS = [0, 255, 2, 5, 0x80, 0x1F, 0xE0, 17]

# (name, format, record length or None = the least, T)
CASES = [(f"fmt{f}_least", f, None, 257) for f in (0, 1, 2, 3, 6, 7, 8, 10)] + [
    ("fmt8_T1", 8, None, 1), ("fmt8_T255", 8, None, 255), ("fmt8_T256", 8, None, 256), ("fmt8_T2p20_3", 8, None, 2 ** 20 + 3),
    ("fmt8_L39", 8, 39, 257), ("fmt8_L41", 8, 41, 513), ("fmt6_L33", 6, 33, 257),
    ("fmt7_L128", 7, 128, 257), ("fmt6_L131", 6, 131, 257), ("fmt4_least", 4, None, 255), ("fmt5_L65", 5, 65, 257), ("fmt9_least", 9, None, 256),
]
CASE_IDS = [c[0] for c in CASES]

# origins of the two modes: raw integer units (Lambert-93 centimetres) and metres
ORIGIN_RAW = (65000000, 686000000, -1234)
ORIGIN_M = (650000.0, 6860000.0, -12.5)
SCALE, OFFSET = (0.01, 0.001, 0.0025), (600000.0, 6800000.0, -100.25)


def _cycle(edges, T, rng, lo, hi, dtype, shift):
    """the edge values from position `shift` on, cycled over the first 4 * len(edges) records, then random ones"""
    out = rng.integers(lo, hi, size=T, endpoint=True, dtype=np.int64)
    n = min(T, 4 * len(edges))
    out[:n] = [edges[(i + shift) % len(edges)] for i in range(n)]
    return out.astype(dtype)


def make_fields(T, seed=0):
    """name -> (T) array for every field a format can hold.  The edge lists have different lengths and different shifts, so
    their combinations vary from record to record; half of the random coordinates are Lambert-93 centimetres."""
    rng = np.random.default_rng(1000 + seed)
    f = {k: _cycle(EDGE_XYZ, T, rng, I32_MIN, I32_MAX, np.int32, s) for k, s in (("X", 0), ("Y", 5), ("Z", 11))}
    lam = np.arange(T) % 2 == 1
    lam[:4 * len(EDGE_XYZ)] = False
    f["X"][lam] = rng.integers(10000000, 125000000, size=int(lam.sum()))
    f["Y"][lam] = rng.integers(600000000, 720000000, size=int(lam.sum()))
    f["Z"][lam] = rng.integers(-5000, 480000, size=int(lam.sum()))
    for k, s in (("intensity", 0), ("red", 1), ("green", 2), ("blue", 3), ("nir", 4)):
        f[k] = _cycle(EDGE_U16, T, rng, 0, 65535, np.uint16, s)
    f["returns"] = _cycle(EDGE_RETURNS, T, rng, 0, 255, np.uint8, 0)
    f["classification"] = _cycle(EDGE_CLASS, T, rng, 0, 255, np.uint8, 3)
    f["flags"] = _cycle([0xFF, 0x00, 0x3C], T, rng, 0, 255, np.uint8, 0)
    f["gps_time"] = rng.random(T) * 1e9
    f["user_data"] = _cycle([0xFF, 0x00], T, rng, 0, 255, np.uint8, 1)
    f["point_source_id"] = _cycle([65535, 0], T, rng, 0, 65535, np.uint16, 0)
    return f
