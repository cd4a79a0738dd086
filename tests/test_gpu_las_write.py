"""The LAS encoder on the device (csrc/las_write.hip, las.py) against the tests' own numpy restatement (tests/_las_write_ref.py),
bytes against bytes: every shape case with planted scores, guard bytes behind the destination, poison behind the source and outside
the score columns; both kernel forms; point_index in every flavour; the statistics over two launches; the round trip through the
decoder; the file-level entry points on hand-written files; and one run of the network's own per-point scores into a file."""
import struct

import numpy as np
import pytest
import torch

import _las_cases as C
import _las_ref as R
import _las_write_cases as WC
import _las_write_ref as W
from stratanet2_vegetation_coverage_maps_amd import _lib
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd import las, parcel
from stratanet2_vegetation_coverage_maps_amd.inference import PointScoreResult

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, PATTERN = 64, 0x5C
COL0, SLACK = 5, 7                        # score columns in front of and behind the range


def header_of(fmt, L, T):
    return las.LasHeader((1, 4), fmt, L, 375, T, C.SCALE, C.OFFSET, (0.0,) * 3, (0.0,) * 3, 375)


def dev_source(recs, poison=0xEE):
    """the source block on the device, followed by 4096 poisoned bytes the encoder must not read: the view ends with the block"""
    a = np.concatenate([np.frombuffer(recs, dtype=np.uint8), np.full(4096, poison, dtype=np.uint8)])
    return torch.from_numpy(a).to(DEV)[:len(recs)]


def dev_scores(s, w, h):
    return PointScoreResult(torch.from_numpy(s).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(h).to(DEV))


def poisoned_scores(T, seed):
    """scores over COL0 + T + SLACK columns whose columns outside [COL0, COL0 + T) hold values that would show: hits 9, a winning
    high-vegetation probability, weight 1e30"""
    s, w, h = WC.make_scores(COL0 + T + SLACK, seed)
    s, w, h = np.roll(s, COL0, axis=1), np.roll(w, COL0), np.roll(h, COL0)       # the planted columns start at COL0
    for sl in (slice(0, COL0), slice(COL0 + T, None)):
        s[:, sl], w[sl], h[sl] = 9.0, 1e30, 9
    return s, w, h


def run(raw, fmt, L, T_src, res, *, form=0, guard=True, **kw):
    """las.encode into a destination followed by GUARD pattern bytes -> (bytes, read stats); the guard must keep its pattern"""
    mask = ops.las_field_mask(kw.get("fields", ()))
    n_out = kw.get("n_out") or (len(kw["point_index"]) if kw.get("point_index") is not None else T_src)
    n = n_out * (L + ops.las_extra_bytes(mask))
    out = torch.full((max(n, 16) + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    try:
        assert _lib.load().sn2_debug_las_encode_form(form) == 0
        got, stats = las.encode(raw, header_of(fmt, L, T_src), res, out=out[:max(n, 16)], **kw)
    finally:
        assert _lib.load().sn2_debug_las_encode_form(0) == 0
    host = out.cpu().numpy()
    assert got.data_ptr() == out.data_ptr() and got.numel() == n
    assert (host[max(n, 16):] == PATTERN).all(), "bytes behind the destination were written"
    if n < 16:
        assert (host[n:16] == PATTERN).all(), "bytes behind the last record were written"
    return host[:n].tobytes(), stats.read()


def fields_of(mask):
    return tuple(W.FIELD_NAMES[k] for k in range(10) if mask >> k & 1)


def same_bytes(got, want, L_dst, what):
    assert len(got) == len(want), what
    if got != want:
        a, b = (np.frombuffer(x, dtype=np.uint8).reshape(-1, L_dst) for x in (got, want))
        rec = int(np.argwhere((a != b).any(axis=1))[0, 0])
        at = int(np.argwhere(a[rec] != b[rec])[0, 0])
        raise AssertionError(f"{what}: {int((a != b).any(axis=1).sum())} records differ, first record {rec} at byte {at}: "
                             f"{a[rec].tobytes().hex()} != {b[rec].tobytes().hex()}")


def same_stats(got, want, what):
    assert (got.mins, got.maxs, list(got.by_return), got.n_bad, got.n_scored) == (
        want["mins"], want["maxs"], want["by_return"], want["n_bad"], want["n_scored"]), what


@pytest.mark.parametrize("name,fmt,L,T,mask", WC.SHAPE_CASES, ids=WC.SHAPE_IDS)
def test_every_shape_both_forms_bytes_and_stats(name, fmt, L, T, mask):
    L = R.LAYOUTS[fmt][1] if L is None else L
    _, recs = WC.source(fmt, L, T, seed=fmt)
    s, w, h = poisoned_scores(T, seed=T)
    unscored = -1 if T % 2 else 7
    want, want_stats = W.encode_ref(recs, fmt, L, T, s, w, h, col0=COL0, mask=mask, class_codes=WC.CODES, unscored=unscored)
    raw, res = dev_source(recs), dev_scores(s, w, h)
    assert ops.las_encode_stage_max() >= L + 38
    for form in (0, 1):
        got, stats = run(raw, fmt, L, T, res, form=form, col0=COL0, fields=fields_of(mask), classify=True, unscored=unscored)
        same_bytes(got, want, L + W.extra_bytes(mask), f"{name} form {form}")
        same_stats(stats, want_stats, f"{name} form {form}")
    # class_mode 0: the class bytes stay, the fields are the same
    want0, _ = W.encode_ref(recs, fmt, L, T, s, w, h, col0=COL0, mask=mask)
    same_bytes(run(raw, fmt, L, T, res, col0=COL0, fields=fields_of(mask))[0], want0, L + W.extra_bytes(mask), f"{name} unclassified")


@pytest.mark.parametrize("fmt,L,gathered", [(8, 38, False), (8, 38, True), (6, 60, False)], ids=["identity", "gathered", "long_source"])
def test_a_million_records_once(fmt, L, gathered):
    """more tiles than workgroups: every workgroup walks several tiles and loads each one tile ahead -- in the identity form with
    few and with many 16-byte chunks per lane, and in the gathered form"""
    T = 2 ** 20 + 3
    _, recs = WC.source(fmt, L, T, seed=1)
    s, w, h = WC.make_scores(T, seed=2)
    index = np.random.default_rng(3).permutation(T).astype(np.int32) if gathered else None
    want, want_stats = W.encode_ref(recs, fmt, L, T, s, w, h, point_index=index, mask=0x3FF, class_codes=WC.CODES)
    got, stats = run(dev_source(recs), fmt, L, T, dev_scores(s, w, h), fields="all", classify=True,
                     point_index=None if index is None else torch.from_numpy(index).to(DEV))
    same_bytes(got, want, L + 38, "2^20 + 3 records")
    same_stats(stats, want_stats, "2^20 + 3 records")
    assert stats.n_scored > T // 2 and sum(stats.by_return) > 0


def test_each_side_of_the_staged_length():
    """L_dst at sn2_las_encode_stage_max() and one above, with and without appended bytes, identity and gathered; the staged ones
    again in the forced direct form"""
    M = ops.las_encode_stage_max()
    T = 513
    rng = np.random.default_rng(3)
    perm = rng.permutation(T).astype(np.int32)
    s, w, h = WC.make_scores(T, seed=4)
    res = dev_scores(s, w, h)
    for L, mask in ((M - 38, 0x3FF), (M - 37, 0x3FF), (M, 0), (M + 1, 0), (M - 2, 0x200), (M - 1, 0x200)):
        _, recs = WC.source(6, L, T, seed=L)
        raw = dev_source(recs)
        for index in (None, perm):
            want, want_stats = W.encode_ref(recs, 6, L, T, s, w, h, point_index=index, mask=mask, class_codes=WC.CODES, unscored=0)
            pi = None if index is None else torch.from_numpy(index).to(DEV)
            for form in ((0, 1) if L + W.extra_bytes(mask) <= M else (0,)):
                got, stats = run(raw, 6, L, T, res, form=form, point_index=pi, fields=fields_of(mask), classify=True, unscored=0)
                same_bytes(got, want, L + W.extra_bytes(mask), f"L {L} mask {mask:#x} gathered {index is not None} form {form}")
                same_stats(stats, want_stats, f"L {L} mask {mask:#x}")


@pytest.mark.parametrize("fmt,L", [(8, 39), (1, 28)])
def test_point_index_in_every_flavour(fmt, L):
    T_src = 300
    _, recs = WC.source(fmt, L, T_src, seed=9)
    rng = np.random.default_rng(10)
    planted = rng.integers(0, T_src, size=257)
    planted[[0, 100, 255, 256]] = [-1, T_src, -2 ** 31, 2 ** 31 - 1]
    flavours = {"identity": np.arange(T_src), "permutation": rng.permutation(T_src), "repeats": rng.integers(0, T_src, size=700),
                "subset": np.sort(rng.choice(T_src, size=100, replace=False)), "planted": planted}
    raw = dev_source(recs)
    for name, index in flavours.items():
        index = index.astype(np.int32)
        T_out = len(index)
        s, w, h = poisoned_scores(T_out, seed=T_out)
        res = dev_scores(s, w, h)
        want, want_stats = W.encode_ref(recs, fmt, L, T_src, s, w, h, point_index=index, col0=COL0, mask=0x2AA, class_codes=WC.CODES)
        assert want_stats["n_bad"] == (4 if name == "planted" else 0)
        for form in (0, 1):
            got, stats = run(raw, fmt, L, T_src, res, form=form, point_index=torch.from_numpy(index).to(DEV), col0=COL0,
                             fields=fields_of(0x2AA), classify=True)
            same_bytes(got, want, L + 18, f"{name} form {form}")
            same_stats(stats, want_stats, f"{name} form {form}")
    # without scores: a pure gather, and a pure copy
    index = flavours["repeats"].astype(np.int32)
    got, stats = run(raw, fmt, L, T_src, None, point_index=torch.from_numpy(index).to(DEV))
    want, want_stats = W.encode_ref(recs, fmt, L, T_src, point_index=index)
    same_bytes(got, want, L, "gather without scores")
    same_stats(stats, want_stats, "gather without scores")
    assert run(raw, fmt, L, T_src, None)[0] == recs
    # n_out below the index's length
    got, _ = run(raw, fmt, L, T_src, None, point_index=torch.from_numpy(index).to(DEV), n_out=99)
    assert got == W.encode_ref(recs, fmt, L, T_src, point_index=index, n_out=99)[0]


def test_stats_over_two_launches_equal_one_launch_over_both():
    Ta, Tb = 300, 257
    _, ra = WC.source(8, 39, Ta, seed=20)
    _, rb = WC.source(8, 39, Tb, seed=21)
    s, w, h = WC.make_scores(Ta + Tb, seed=22)
    res = dev_scores(s, w, h)
    both = las.encode(dev_source(ra + rb), header_of(8, 39, Ta + Tb), res, fields="all", classify=True)[1]
    acc = ops.LasEncodeStats(DEV)
    las.encode(dev_source(ra), header_of(8, 39, Ta), res, fields="all", classify=True, stats=acc)
    out_b, acc2 = las.encode(dev_source(rb), header_of(8, 39, Tb), res, col0=Ta, fields="all", classify=True, stats=acc)
    assert acc2 is acc and acc.buf.cpu().numpy().tobytes() == both.buf.cpu().numpy().tobytes()
    want, want_stats = W.encode_ref(ra + rb, 8, 39, Ta + Tb, s, w, h, mask=0x3FF, class_codes=WC.CODES)
    same_stats(acc.read(), want_stats, "two launches")
    assert out_b.cpu().numpy().tobytes() == want[Ta * 77:]
    fresh = ops.LasEncodeStats(DEV).read()
    assert (fresh.mins, fresh.maxs, sum(fresh.by_return), fresh.n_bad, fresh.n_scored) == (None, None, 0, 0, 0)


@pytest.mark.parametrize("fmt,L,mask", [(8, 38, 0x3FF), (3, 37, 0x2AA), (6, 33, 0x200), (0, 20, 0x001)])
def test_decoding_the_written_block_gives_the_source_cloud(fmt, L, mask):
    T_src, T_out = 600, 777
    _, recs = WC.source(fmt, L, T_src, seed=30)
    index = np.random.default_rng(31).integers(0, T_src, size=T_out).astype(np.int32)
    s, w, h = WC.make_scores(T_out, seed=32)
    raw = dev_source(recs)
    got, _ = las.encode(raw, header_of(fmt, L, T_src), dev_scores(s, w, h), point_index=torch.from_numpy(index).to(DEV),
                        fields=fields_of(mask), classify=True, unscored=1)
    src_cloud, src_cls = las.decode(raw, header_of(fmt, L, T_src), "header", C.ORIGIN_M, classification=True)
    cloud, cls = las.decode(got, header_of(fmt, L + W.extra_bytes(mask), T_out), "header", C.ORIGIN_M, classification=True)
    assert cloud.cpu().numpy().tobytes() == src_cloud[:, torch.from_numpy(index.astype(np.int64)).to(DEV)].cpu().numpy().tobytes()
    code = np.where(h > 0, np.asarray(WC.CODES)[W.best_class(s[4:8])], 1)
    old = src_cls.cpu().numpy()[index]
    want_cls = code if fmt >= 6 else (old & 0xE0) | code
    assert np.array_equal(cls.cpu().numpy(), want_cls.astype(np.uint8))
    assert (h > 0).any() and (h == 0).any()


# ---- files
def tile_fields(rng, T, x0=0):
    return {"X": rng.integers(0, 6000, T) + x0, "Y": rng.integers(0, 4000, T), "Z": rng.integers(0, 3000, T),
            "intensity": rng.integers(0, 60000, T), "returns": rng.integers(0, 256, T), "flags": rng.integers(0, 256, T),
            "classification": rng.choice(np.array([1, 2, 5, 66]), T), "gps_time": rng.random(T) * 1e6,
            "red": rng.integers(0, 65536, T), "green": rng.integers(0, 65536, T), "blue": rng.integers(0, 65536, T),
            "nir": rng.integers(0, 65536, T)}


def test_write_scored_of_a_hand_written_file(tmp_path):
    T = 1000
    rng = np.random.default_rng(40)
    blob = R.write_las(tile_fields(rng, T), 8, 41, (1, 4), scale=C.SCALE, offset=C.OFFSET, legacy_count=0, pad_after_header=54)
    src, dst = tmp_path / "src.las", tmp_path / "dst.las"
    src.write_bytes(blob)
    s, w, h = WC.make_scores(T, seed=41)
    stats = las.write_scored(str(src), str(dst), dev_scores(s, w, h), fields="all", classify=True)
    out = dst.read_bytes()
    f = W.parse_frame(out)
    fmt, L, _, off, _, _ = R.parse(blob)
    want, want_stats = W.encode_ref(blob[off:], fmt, L, T, s, w, h, mask=0x3FF, class_codes=WC.CODES)
    same_bytes(f["points"], want, 79, "write_scored")
    same_stats(stats, want_stats, "write_scored")
    assert (f["L"], f["count"], f["legacy_count"], f["n_vlr"], f["padding"]) == (79, T, 0, 1, bytes(54))
    assert f["offset_to_points"] == 375 + 54 + 11 * 192 + 54 and len(out) == f["offset_to_points"] + T * 79
    assert f["by_return"] == want_stats["by_return"]
    for a in range(3):
        assert f["mins"][a] == want_stats["mins"][a] * C.SCALE[a] + C.OFFSET[a] and f["maxs"][a] == want_stats["maxs"][a] * C.SCALE[a] + C.OFFSET[a]
    assert [x[0] for x in W.extra_bytes_fields(out)] == ["undocumented"] + W.FIELD_NAMES
    # read_header accepts the file and it decodes to the source's cloud bit for bit
    assert las.read_header(str(dst)).n_points == T
    for coords in ("reference", "header"):
        assert las.load_las(str(dst), DEV, coords).cpu().numpy().tobytes() == las.load_las(str(src), DEV, coords).cpu().numpy().tobytes()
    # a PointScores-like object with finalize() is taken too; no field and no class: the records as they were
    class Lazy:
        def finalize(self):
            return dev_scores(s, w, h)
    las.write_scored(str(src), str(dst), Lazy())
    assert W.parse_frame(dst.read_bytes())["points"] == blob[off:] and len(dst.read_bytes()) == len(blob)


def test_write_parcels_through_a_tiny_cut(tmp_path):
    rng = np.random.default_rng(50)
    paths, blobs = [], []
    for j, T in enumerate((1500, 1100)):
        b = R.write_las(tile_fields(rng, T, x0=6000 * j), 8, 39, (1, 4), legacy_count=0)
        p = tmp_path / f"tile{j}.las"
        p.write_bytes(b)
        paths.append(str(p))
        blobs.append(b)
    # two rectangles: one inside tile 0, one across both tiles; a third one far away gets no point
    shapes = [[np.array([[5.0, 5.0], [25.0, 5.0], [25.0, 25.0], [5.0, 25.0]])], [np.array([[50.0, 10.0], [75.0, 10.0], [75.0, 30.0], [50.0, 30.0]])],
              [np.array([[500.0, 500.0], [510.0, 500.0], [510.0, 510.0]])]]
    cut = las.load_parcels(paths, shapes, buffer_m=2.0)
    assert cut.clouds.K == 2 and cut.parcel_index.tolist() == [0, 1] and cut.counts[2] == 0
    T_cut = int(cut.clouds.point_start[-1])
    s, w, h = WC.make_scores(T_cut, seed=51)
    res = dev_scores(s, w, h)
    dsts = [str(tmp_path / f"parcel{k}.las") for k in range(2)]
    stats = las.write_parcels(paths, cut, dsts, res, fields=("p_high_veg", "hits"), classify=True, unscored=1)
    records = b"".join(b[375:] for b in blobs)
    index = cut.point_index.cpu().numpy()
    assert index.max() >= 1500                                             # the second parcel takes points of the second tile
    for k in range(2):
        p0, p1 = (int(v) for v in cut.clouds.point_start[k:k + 2])
        want, want_stats = W.encode_ref(records, 8, 39, 2600, s, w, h, point_index=index[p0:p1], col0=p0, mask=0x280,
                                        class_codes=WC.CODES, unscored=1)
        out = open(dsts[k], "rb").read()
        f = W.parse_frame(out)
        same_bytes(f["points"], want, 45, f"parcel {k}")
        same_stats(stats[k], want_stats, f"parcel {k}")
        assert (f["count"], f["L"], f["n_vlr"]) == (p1 - p0, 45, 1)
        assert W.extra_bytes_fields(out) == [("undocumented", 0, 1, 38), ("p_high_veg", 9, 4, 39), ("hits", 3, 2, 43)]
        # the file is the parcel's cloud, with the tile's exact integer coordinates
        assert las.load_las(dsts[k], DEV).cpu().numpy().tobytes() == cut.clouds.cloud(k).cpu().numpy().tobytes()
    # no scores: a pure gather into files
    las.write_parcels(paths, cut, dsts)
    assert W.parse_frame(open(dsts[1], "rb").read())["points"] == W.encode_ref(records, 8, 39, 2600, point_index=index[p0:p1])[0]
    # tiles that differ are named
    odd = tmp_path / "odd.las"
    odd.write_bytes(R.write_las(tile_fields(rng, 10), 8, 39, (1, 4), scale=(0.001, 0.01, 0.01)))
    with pytest.raises(ValueError, match="odd.las.*scale"):
        las.write_parcels([paths[0], str(odd)], cut, dsts)
    with pytest.raises(ValueError, match="paths"):
        las.write_parcels(paths, cut, dsts[:1])
    # an index outside the tiles read is an error after the read
    with pytest.raises(ValueError, match="outside"):
        las.write_parcels(paths[:1], cut, dsts)


def test_the_networks_scores_into_a_file_and_back(tmp_path):
    from stratanet2_vegetation_coverage_maps_amd import PointNet2
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel
    a = make_args(cuda=0, subsample_size=1024)
    cloud = make_parcel(30, 30, density=32.0, seed=10, plant=False, x0=650000.0)
    f = {k: np.round(cloud[i].astype(np.float64) * 100).astype(np.int32) for i, k in enumerate("XYZ")}
    for i, k in ((3, "red"), (4, "green"), (5, "blue"), (6, "nir"), (7, "intensity")):
        f[k] = np.clip(np.round(cloud[i]), 0, 65535).astype(np.uint16)
    f["returns"] = (np.clip(cloud[8], 0, 15).astype(np.uint8) | (np.clip(cloud[9], 0, 15).astype(np.uint8) << 4))
    f["classification"] = np.full(cloud.shape[1], 1, dtype=np.uint8)
    src, dst = tmp_path / "parcel.las", tmp_path / "scored.las"
    blob = R.write_las(f, 8, None, (1, 4), legacy_count=0)
    src.write_bytes(blob)
    on_dev = las.load_las(str(src), DEV)
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    mos, plots, scores = parcel.predict_parcel_cloud(model, on_dev, a, batch_size=64, points=True, sampler="device", seed=20250117,
                                                     fps_start=0)
    res = scores.finalize()
    stats = las.write_scored(str(src), str(dst), scores, fields="all", classify=True)
    s, w, h = res.scores.cpu().numpy(), res.weight.cpu().numpy(), res.hits.cpu().numpy()
    T = cloud.shape[1]
    assert (h > 0).any() and (h == 0).any(), "the cloud must hold scored and unscored points"
    assert stats.n_scored == int((h > 0).sum()) and stats.n_bad == 0
    out = dst.read_bytes()
    want, _ = W.encode_ref(blob[375:], 8, 38, T, s, w, h, mask=0x3FF, class_codes=WC.CODES)
    same_bytes(W.parse_frame(out)["points"], want, 76, "the network's scores")
    rec = np.frombuffer(W.parse_frame(out)["points"], dtype=W.out_dtype(8, 38, 0x3FF))
    assert set(rec["classification"][h > 0].tolist()) <= set(WC.CODES) and (rec["classification"][h == 0] == 1).all()
    assert np.array_equal(rec["x_hits"], np.minimum(h, 65535)) and rec["x_p_high_veg"].tobytes() == s[7].tobytes()
    assert las.load_las(str(dst), DEV).cpu().numpy().tobytes() == on_dev.cpu().numpy().tobytes()
