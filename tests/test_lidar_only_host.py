"""Four point features (LiDAR-only plots: n_input_feats = 6), the host side: argument checks and route rules of the library, the
model's constructor and state dict, and the test helper against the oracle.  No device: every library call below returns from
its argument checks (fake pointers, never dereferenced) or is host arithmetic."""
import ctypes
from ctypes import byref

import pytest
import torch

from _lidar_only_ref import init_state_dict, lidar_args, lidar_batch, train_ref
from oracle import network
from stratanet2_vegetation_coverage_maps_amd import PointNet2, _lib
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd.point_net2_3sa import PointNet2ThreeSA
from stratanet2_vegetation_coverage_maps_amd.synthetic import LIDAR_ROWS, make_args

FAKE = 0x1000
EINVAL, ELIMIT = -1, -2


def test_binding_version_and_the_new_names():
    assert _lib.SN2_VERSION == 102 and _lib.load().sn2_version() == 102
    assert _lib.NET_CLOUD10 == _lib.CONSTANTS["SN2_NET_CLOUD10"] == 512
    assert "sn2_pack_rows_feat" in _lib.SIGNATURES
    assert LIDAR_ROWS == (0, 1, 2, 7, 8, 9)


def test_pack_rows_feat_table_and_error_codes():
    """The (C, F) table of sn2_pack_rows_feat: every pair outside it is SN2_ELIMIT, null or non-positive arguments SN2_EINVAL --
    before any launch (no device here: an accepted pair would launch, so the accepted ones are told apart from the refused ones
    by NOT getting SN2_ELIMIT from the check, with a null stream argument left out: tests/test_gpu_lidar_only.py runs them)."""
    fn = _lib.load().sn2_pack_rows_feat
    accepted = {(10, 8), (6, 4), (10, 4)}
    for C in (1, 4, 5, 6, 7, 8, 10, 12):
        for F in (1, 2, 3, 4, 6, 8, 10):
            if (C, F) not in accepted:
                assert fn(FAKE, FAKE, 2, C, 100, F, FAKE, None) == ELIMIT, (C, F)
    for args in ((None, FAKE, 2, 6, 100, 4, FAKE), (FAKE, None, 2, 6, 100, 4, FAKE), (FAKE, FAKE, 2, 6, 100, 4, None),
                 (FAKE, FAKE, 0, 6, 100, 4, FAKE), (FAKE, FAKE, 2, 0, 100, 4, FAKE), (FAKE, FAKE, 2, 6, 0, 4, FAKE),
                 (FAKE, FAKE, 2, 6, 100, 0, FAKE), (FAKE, FAKE, -1, 10, 100, 8, FAKE), (FAKE, FAKE, 2, 10, -5, 4, FAKE)):
        assert fn(*args, None) == EINVAL, args
    # sn2_pack_rows itself is what it was: ten rows or SN2_ELIMIT
    assert _lib.load().sn2_pack_rows(FAKE, FAKE, 2, 6, 100, FAKE, None) == ELIMIT


def test_source_side_rule_with_four_skip_columns():
    """sn2_fp_source_side(R, 4, force): cb = 4 passes the width test (a multiple of four, at most 16), so the rule is the row
    count's -- above SN2_STAT_SLOTS * 64 rows, or forced."""
    lib = _lib.load()
    for R in (1, 65536):
        assert lib.sn2_fp_source_side(R, 4, 0) == 0 and lib.sn2_fp_source_side(R, 4, 1) == 1
        assert ops.fp_source_side(R, 4) is False and ops.fp_source_side(R, 4, True) is True
    for R in (65537, 72003, 524288):
        assert lib.sn2_fp_source_side(R, 4, 0) == 1 and lib.sn2_fp_source_side(R, 4, 1) == 1
        assert ops.fp_source_side(R, 4) is True
    assert lib.sn2_fp_source_side(10 ** 6, 4, 0) == lib.sn2_fp_source_side(10 ** 6, 8, 0) == 1


def _model_shell(sa1_cin, fp1_cin):
    m = _lib.NetModel()
    for L, (ci, co) in zip([m.sa1[0], m.sa1[1], m.sa2, m.sa3, m.fp3, m.fp2, m.fp1],
                           [(sa1_cin, 16), (16, 16), (19, 32), (35, 64), (96, 64), (80, 34), (fp1_cin, 34)]):
        L.cin, L.cout = ci, co
    m.n_flat, m.max_neighbors, m.source_side, m.fuse_eval_head = 14997, 2000, 1, 1
    return m


def _dims(B, N, M1, M2):
    d = _lib.NetDims()
    d.B, d.N, d.M1, d.M2, d.cap1, d.cap2 = B, N, M1, M2, min(2000, N), min(2000, M1)
    return d


def test_check_dims_and_the_smaller_rows0():
    """check_dims through sn2_net_geo_carve: SA1 / FP1 input widths 7 / 38 and 11 / 42 are the two models; 7 / 42, 11 / 38 and
    9 / 40 are none.  The four-feature arena holds rows0 as (B*N, 8): 16 bytes per point less than the eight-feature one, and
    nothing else moves."""
    lib = _lib.load()
    B, N, M1, M2 = 16, 32768, 1024, 256
    d = _dims(B, N, M1, M2)
    sz = ctypes.c_size_t()
    sizes = {}
    for sa1, fp1, want in ((7, 38, 0), (11, 42, 0), (7, 42, ELIMIT), (11, 38, ELIMIT), (9, 40, ELIMIT), (3, 34, ELIMIT), (15, 46, ELIMIT)):
        g = _lib.NetGeo()
        m = _model_shell(sa1, fp1)
        assert lib.sn2_net_geo_carve(byref(m), byref(d), None, byref(g), byref(sz)) == want, (sa1, fp1)
        a, b = _lib.NetAct(), _lib.NetBwd()
        s2, s3 = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.sn2_net_act_carve(byref(m), byref(d), 1, None, byref(a), byref(s2)) == want
        assert lib.sn2_net_bwd_carve(byref(m), byref(d), None, None, byref(b), byref(s2), byref(s3)) == want
        if want == 0:
            sizes[sa1] = (sz.value, g.rows0 or 0, g.p2_pix)
    pad = lambda n: (n + 255) // 256 * 256          # noqa: E731
    assert sizes[11][0] - sizes[7][0] == pad(B * N * 12 * 4) - pad(B * N * 8 * 4)
    assert sizes[11][1] == sizes[7][1]               # rows0 is the arena's last table: everything in front keeps its offset


def test_constructor_names_the_supported_feature_counts():
    for n in (8, 4, 7, 12):
        with pytest.raises(ValueError, match=r"\{4, 8\}"):
            PointNet2(make_args(n_input_feats=n))
    with pytest.raises(ValueError):
        PointNet2(make_args(n_class=3))
    # the three-level variant stays at eight features
    with pytest.raises(ValueError, match=r"\{8\}"):
        PointNet2ThreeSA(make_args(n_input_feats=6, ratio3=0.25, r3=4.0))
    assert PointNet2(make_args(n_input_feats=6)).n_input_feats == 4 and PointNet2(make_args()).n_input_feats == 8


def test_state_dict_has_the_reference_keys_and_no_silent_slicing():
    m4 = PointNet2(make_args(n_input_feats=6))
    sd4, sd8 = init_state_dict(4, 3), network.init_state_dict(3)
    assert list(m4.state_dict()) == list(sd4) == list(sd8)
    assert tuple(m4.state_dict()["sa1_module.conv.local_nn.0.0.weight"].shape) == (16, 7)
    assert tuple(m4.state_dict()["fp1_module.nn.0.0.weight"].shape) == (34, 38)
    other = {"sa1_module.conv.local_nn.0.0.weight", "fp1_module.nn.0.0.weight"}
    assert all(sd4[k].shape == sd8[k].shape for k in sd4 if k not in other)
    m4.load_state_dict(sd4)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m4.load_state_dict(sd8)
    with pytest.raises(RuntimeError, match="size mismatch"):
        PointNet2(make_args()).load_state_dict(sd4)
    # the helper at F = 8 is the oracle's own initialisation (same construction order, same generator)
    sd8h = init_state_dict(8, 3)
    assert all(torch.equal(sd8h[k], sd8[k]) for k in sd8)
    # same construction order as the model's: same default weights from the same seed
    torch.manual_seed(3)
    fresh = PointNet2(make_args(n_input_feats=6)).state_dict()
    assert all(torch.equal(fresh[k], sd4[k]) for k in sd4)


def test_forward_refuses_other_row_counts_on_the_host():
    """The shape check comes after the device check, so on a CPU model the device error must NOT hide a wrong shape's message on a
    GPU machine: here only the accepted row counts are read off the model (tests/test_gpu_lidar_only.py raises the errors)."""
    assert PointNet2(make_args(n_input_feats=6))._cloud_rows() == (6, 10)
    assert PointNet2(make_args())._cloud_rows() == (10,)


def test_helper_state_dict_runs_a_four_feature_oracle_step():
    """A six-row cloud through the oracle unchanged (`cloud[:, 2:]` whatever its width): one fp64 training step at 2 x 400 points,
    every parameter with a finite gradient of its own shape, outputs the fp32 run reproduces."""
    B, N, ratio1 = 2, 400, 0.1
    ref = train_ref(B, N, ratio1, 3)
    sd = init_state_dict(4, 3)
    assert set(ref["grads"]) == set(network.param_keys(sd))
    for k, g in ref["grads"].items():
        assert g.shape == sd[k].shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    assert ref["cov"].shape == (B * N, 4) and bool(torch.isfinite(ref["cov"]).all())
    six, ten = lidar_batch(B, N)
    assert six["cloud"].shape == (B, 6, N) and ten["cloud"].shape == (B, 10, N)
    assert bool(torch.isnan(ten["cloud"][:, 3:7]).all()) and torch.equal(ten["cloud"][:, list(LIDAR_ROWS)], six["cloud"])
    from oracle import check
    r32 = check.train_step(sd, six, lidar_args(N, ratio1), fps_start=six["fps_start"], dtype=torch.float32)
    assert float((r32["cov"].double() - ref["cov"]).abs().max()) < 1e-4
