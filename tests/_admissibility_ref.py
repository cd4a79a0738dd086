"""The admissibility band (include/strata_hip.h, "Admissibility band") restated in numpy.

A restatement of the header's rule, NOT a fixture from the reference: the reference builds the band with rasterio `sieve` /
`shapes`, a shapely buffer and `geometry_mask` (`inference/geotiff_raster.py:149-196`), none of which is available to this
project's tests, so the stated rule is the yardstick.  Everything is integer logic and one fp32 comparison: the device must give
the same bytes.

The algorithms differ from the kernels' on purpose: the labelling is a minimum propagation with pointer jumping (the kernels:
union-find), the walk is pointer doubling with the big-enough regions as fixed points (the kernels: one walk per region with
Brent's repeat detection).  `wrong=` switches in ONE deliberate misreading of the rule; tests/test_admissibility_host.py shows that
each of them changes a planted canvas, i.e. that the canvases can tell the readings apart.
"""
import numpy as np

WRONG = ("conn8", "cascade", "tie_largest_id", "tie_le", "edge_one", "invalid_targets", "fill_holes")
NAN32 = np.float32(np.nan)


def parse(art):
    """rows of '.', '#', 'x' -> (H,W) fp32 hard band: 0, 1, NaN"""
    rows = [r for r in art.strip("\n").split("\n")]
    assert len({len(r) for r in rows}) == 1, [len(r) for r in rows]
    m = {".": 0.0, "#": 1.0, "x": np.nan}
    return np.array([[m[c] for c in r] for r in rows], dtype=np.float32)


def bands_from_hard(hard, seed=0):
    """(H,W) hard band -> (5,H,W) fp32 as the finalisation leaves them: random scores and weights, NaN together with the hard band"""
    rng = np.random.default_rng(seed)
    H, W = hard.shape
    b = rng.random((5, H, W), dtype=np.float32)
    b[1] = np.where(rng.random((H, W)) < 0.5, b[1], np.float32(0.5) * b[0])      # Vm_soft below Vb about half of the time
    b[3] = hard
    b[:, np.isnan(hard)] = np.nan
    return b


def random_hard(H, W, density, nan_fraction, seed):
    rng = np.random.default_rng(seed)
    hard = (rng.random((H, W)) < density).astype(np.float32)
    hard[rng.random((H, W)) < nan_fraction] = np.nan
    return hard


def _pairs(H, W, conn8):
    """index pairs (a, b) of adjacent pixels, each unordered pair once"""
    idx = np.arange(H * W).reshape(H, W)
    out = [(idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])]
    if conn8:
        out += [(idx[:-1, :-1], idx[1:, 1:]), (idx[:-1, 1:], idx[1:, :-1])]
    return np.concatenate([a.reshape(-1) for a, _ in out]), np.concatenate([b.reshape(-1) for _, b in out])


def label_regions(part, val, conn8=False):
    """part (H,W) bool: the pixels that take part; val (H,W) int: regions are connected components of equal val ->
    (H,W) int64 label = the smallest row-major pixel index of the pixel's region, -1 where not part"""
    H, W = part.shape
    P = H * W
    a, b = _pairs(H, W, conn8)
    pf, vf = part.reshape(-1), val.reshape(-1)
    keep = pf[a] & pf[b] & (vf[a] == vf[b])
    a, b = a[keep], b[keep]
    lab = np.arange(P, dtype=np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        np.minimum.at(new, b, lab[a])
        while True:                                   # pointer jumping: a label is a pixel of the same region
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(pf, lab, -1).reshape(H, W)


def scipy_partition(valid, h):
    """an independent labelling for the partition check only: scipy.ndimage.label, 4-connected, per value -> (H,W) int, 0 = invalid"""
    from scipy import ndimage
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    l1, n1 = ndimage.label(valid & (h == 1), structure=cross)
    l0, n0 = ndimage.label(valid & (h == 0), structure=cross)
    return np.where(l1 > 0, l1, np.where(l0 > 0, n1 + l0, 0))


def same_partition(lab_a, lab_b, none_a, none_b):
    """do two labellings cut the pixels into the same sets?  none_x: the label that means "no region" """
    a, b = lab_a.reshape(-1), lab_b.reshape(-1)
    if not np.array_equal(a == none_a, b == none_b):
        return False
    a, b = a[a != none_a], b[b != none_b]
    pairs = np.unique(np.stack([a, b]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


def _cascade(lab, val, size, nb_a, nb_b, s):
    """WRONG on purpose: regions in id order, each small one merged into its largest CURRENT neighbour, whose size then grows"""
    ids = [int(r) for r in np.unique(lab[lab >= 0])]
    adj = {r: set() for r in ids}
    for x, y in zip(nb_a.tolist(), nb_b.tolist()):
        adj[x].add(y)
    cur = {r: int(size[r]) for r in ids}
    value = {r: int(val.reshape(-1)[r]) for r in ids}
    owner = {r: r for r in ids}
    for r in ids:
        if cur[r] >= s or not adj[r]:
            continue
        b = max(adj[r], key=lambda n: (cur[n], -n))
        cur[b] += cur[r]
        for n in adj[r]:
            adj[n].discard(r)
            if n != b:
                adj[n].add(b)
                adj[b].add(n)
        for k, o in owner.items():
            if o == r:
                owner[k] = b
    S = np.zeros(lab.size, dtype=np.int64)
    for r in ids:
        S[r] = value[owner[r]] & 1
    return S


def admissibility(bands5, s, wrong=None):
    """bands5 (5,H,W) fp32 -> dict: bands6 (6,H,W) fp32, stats (4) int64 = regions, small regions, pixels with S != h, valid
    inaccessible pixels; and the intermediate fields label (H,W) (-1 invalid), size, target (per pixel: the region its region's walk
    found, -1 when the walk failed or never started), steps (per pixel: the number of steps of its region's successful walk, 0
    otherwise), S, Hp, inacc."""
    assert wrong is None or wrong in WRONG
    bands5 = np.asarray(bands5, dtype=np.float32)
    _, H, W = bands5.shape
    P = H * W
    hard = bands5[3]
    valid = ~np.isnan(hard)
    h = (np.nan_to_num(hard, nan=0.0) > 0).astype(np.int64)
    conn8 = wrong == "conn8"
    # the invalid pixels take part in the labelling only under the misreading that lets them be merge targets (value 2, bit 1)
    part = np.ones_like(valid) if wrong == "invalid_targets" else valid
    val = np.where(valid, h, 2)
    lab = label_regions(part, val, conn8)
    lf, pf = lab.reshape(-1), part.reshape(-1)
    size = np.bincount(lf[pf], minlength=P).astype(np.int64)
    roots = np.flatnonzero((lf == np.arange(P)) & pf)
    bit = (val.reshape(-1) != 0).astype(np.int64)                           # a region's bit, read at its root
    small = np.zeros(P, dtype=bool)
    small[roots] = (size[roots] < s) & (val.reshape(-1)[roots] != 2)

    # neighbours: every ordered pair (region, neighbouring region)
    a, b = _pairs(H, W, conn8)
    keep = pf[a] & pf[b] & (lf[a] != lf[b])
    ra, rb = lf[a][keep], lf[b][keep]
    nb_a, nb_b = np.concatenate([ra, rb]), np.concatenate([rb, ra])

    if wrong == "cascade":
        S_root = _cascade(lf, val, size, nb_a, nb_b, s)
        target = np.full(P, -1, dtype=np.int64)
        steps = np.zeros(P, dtype=np.int64)
    else:
        # big(R): the neighbour of largest size, ties to the smallest id
        from_small = small[nb_a]
        ka, kb = nb_a[from_small], nb_b[from_small]
        tie = kb if wrong == "tie_largest_id" else (P - 1 - kb)
        key = size[kb] * P + tie                                            # size first, then the tie; > 0 whenever there is one
        best = np.zeros(P, dtype=np.int64)
        np.maximum.at(best, ka, key + 1)
        has_big = best > 0
        big = np.where(has_big, (best - 1) % P if wrong == "tie_largest_id" else P - 1 - (best - 1) % P, -1)
        # the walk by pointer doubling: a region of size >= s and a small region without a big stay where they are; after 2^k >=
        # (small regions + 1) steps a walk that has not come to rest has met a region twice
        step = np.arange(P, dtype=np.int64)
        go = small & has_big
        step[go] = big[go]
        nsteps = np.where(go, 1, 0).astype(np.int64)                        # moves made so far (a region at rest makes none)
        at = step.copy()
        k, n_small = 0, int(small.sum())
        while (1 << k) < n_small + 1:
            nsteps = nsteps + nsteps[at]
            at = at[at]
            k += 1
        found = small & (~small[at]) & (at != np.arange(P))
        target = np.where(found, at, -1)
        steps = np.where(found, nsteps, 0)
        S_root = np.where(found, bit[np.maximum(target, 0)], bit)
    S = np.where(valid, S_root[np.maximum(lab, 0)], 0)
    Hp = np.where(valid, S if wrong == "fill_holes" else np.minimum(h, S), 1)

    pad = np.full((H + 4, W + 4), 1 if wrong == "edge_one" else 0, dtype=np.int64)
    pad[2:H + 2, 2:W + 2] = Hp
    inacc = np.ones((H, W), dtype=bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            d = max(2 * abs(dx) - 1, 0) ** 2 + max(2 * abs(dy) - 1, 0) ** 2
            if (d <= 9) if wrong == "tie_le" else (d < 9):
                inacc &= pad[2 + dy:2 + dy + H, 2 + dx:2 + dx + W] == 1

    vb, vms = bands5[0], bands5[1]
    with np.errstate(invalid="ignore"):
        adm = np.where(vb > vms, vb, vms).astype(np.float32)
    adm = np.where(inacc, np.float32(0.0), adm)
    adm = np.where(valid, adm, NAN32).astype(np.float32)
    bands6 = np.stack([bands5[0], bands5[1], bands5[2], bands5[3], adm, bands5[4]]).astype(np.float32)
    vroots = roots[val.reshape(-1)[roots] != 2]
    stats = np.array([len(vroots), int(small.sum()), int((valid & (S != h)).sum()), int((valid & inacc).sum())], dtype=np.int64)
    per_pixel = lambda arr: np.where(valid, arr[np.maximum(lab, 0)], -1 if arr is target else 0)
    return dict(bands6=bands6, stats=stats, label=np.where(valid, lab, -1), size=size, target=per_pixel(target), steps=per_pixel(steps),
                S=S, Hp=Hp, inacc=inacc, valid=valid, h=h)


def tie_decided(bands5, s):
    """the number of pixels whose inaccessibility the tie rule decides: inaccessible with `<`, not with `<=`"""
    a, b = admissibility(bands5, s), admissibility(bands5, s, wrong="tie_le")
    return int((a["valid"] & a["inacc"] & ~b["inacc"]).sum())
