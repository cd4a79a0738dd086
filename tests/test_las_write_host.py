"""The LAS encoder without a device: six records typed out by hand, byte by byte, pin the tests' own restatement of the rule
(tests/_las_write_ref.py: `encode_ref`, which the GPU tests hold the kernel to) AND the library's own statement of it
(csrc/las_write_rules.h: `las_compose`, the function the kernels run per lane, compiled here for the host into a small program);
each deliberately wrong restatement differs from both on the planted cases; las.patch_header on files of `_las_ref.write_las` in
versions 1.2 and 1.4 against the tests' own frame parser and hand-computed offsets; the argument checks of sn2_las_encode return
their codes before any device work."""
import ctypes
import os
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import _las_cases as C
import _las_ref as R
import _las_write_cases as WC
import _las_write_ref as W
from conftest import ROOT


def hx(s):
    return bytes.fromhex(s)


# ---- the library's rule on the CPU: las_compose of csrc/las_write_rules.h behind a file interface
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "las_write_rules.h"
template <class T> static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) exit(3);
    return v;
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    // format, L_src, mask, class_mode, four codes, unscored, T_src, T_out, has_index, has_scores, col0, stride
    const std::vector<long long> h = take<long long>(f, 15);
    const int format = (int)h[0], L_src = (int)h[1], codes[4] = {(int)h[4], (int)h[5], (int)h[6], (int)h[7]};
    const long long T_src = h[9], T_out = h[10];
    const size_t col0 = (size_t)h[13], stride = (size_t)h[14];
    const std::vector<uint32_t> src = take<uint32_t>(f, ((size_t)T_src * L_src + 3) / 4);       // 4-byte aligned
    const std::vector<int> index = take<int>(f, h[11] ? (size_t)T_out : 0);
    const std::vector<float> scores = take<float>(f, h[12] ? 8 * stride : 0), weight = take<float>(f, h[12] ? stride : 0);
    const std::vector<int> hits = take<int>(f, h[12] ? stride : 0);
    fclose(f);
    las_write_rule R = {format, L_src, las_write_extra_bytes((unsigned)h[2]), (unsigned)h[2], (int)h[3], las_write_pack_codes(codes), (int)h[8]};
    las_score_cols S = {h[12] ? scores.data() : nullptr, h[12] ? weight.data() : nullptr, h[12] ? hits.data() : nullptr, stride};
    const int L_dst = L_src + R.E;
    std::vector<uint8_t> out((size_t)T_out * L_dst + 4, 0xCD);
    const las_guarded_words words{(const uint8_t*)src.data(), (size_t)T_src * L_src};
    for (long long i = 0; i < T_out; ++i) {
        const long long s = h[11] ? index[i] : i;
        const bool have = s >= 0 && s < T_src;
        las_compose(words, have ? (size_t)s * L_src : 0, have, las_byte_stream{out.data(), 0}, (size_t)i * L_dst, R,
                    las_load_scores(S, col0 + (size_t)i, R));
    }
    for (int k = 0; k < 4; ++k)
        if (out[(size_t)T_out * L_dst + k] != 0xCD) return 4;                                   // wrote behind the block
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 1, (size_t)T_out * L_dst, f);
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def composer(tmp_path_factory):
    """encode_ref's signature over the library's las_compose: the driver above compiled for the host with the header of the tree"""
    d = tmp_path_factory.mktemp("compose")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "stratanet2_vegetation_coverage_maps_amd", "csrc"),
                           str(d / "driver.cpp"), "-o", exe])

    def encode(records, fmt, L_src, T_src, scores=None, weight=None, hits=None, point_index=None, n_out=None, col0=0, mask=0,
               class_codes=None, unscored=-1):
        T_out = n_out if n_out is not None else (len(point_index) if point_index is not None else T_src)
        stride = 0 if scores is None else scores.shape[1]
        head = [fmt, L_src, mask, 0 if class_codes is None else 1, *(class_codes or (0, 0, 0, 0)), unscored, T_src, T_out,
                int(point_index is not None), int(scores is not None), col0, stride]
        blob = np.asarray(head, dtype=np.int64).tobytes() + bytes(records[:T_src * L_src]) + bytes(-(T_src * L_src) % 4)
        if point_index is not None:
            blob += np.asarray(point_index, dtype=np.int32)[:T_out].tobytes()
        if scores is not None:
            blob += np.ascontiguousarray(scores, dtype=np.float32).tobytes() + weight.astype(np.float32).tobytes() + hits.astype(np.int32).tobytes()
        (d / "in.bin").write_bytes(blob)
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        return (d / "out.bin").read_bytes()
    return encode


def both(composer, *a, **kw):
    """the restatement's bytes, after checking that the library's rule gives the same"""
    got, stats = W.encode_ref(*a, **kw)
    assert composer(*a, **kw) == got, "las_compose and the restatement differ"
    return got, stats


def cols(p, hits, cov=(0.5, 0.0, 0.0, 0.0), weight=1.25):
    """one score column: scores (8,1), weight (1), hits (1)"""
    s = np.array(list(cov) + list(p), dtype=np.float32).reshape(8, 1)
    return s, np.array([weight], dtype=np.float32), np.array([hits], dtype=np.int32)


# ---- six hand-written records: the source bytes, the call, the bytes that must come out
# 1. legacy (format 1, 28 bytes) with the three flag bits set: byte 15 = 0xe5 = flags 0xe0 | class 5.  bare soil wins -> code 2:
#    byte 15 = 0xe0 | 2 = 0xe2.  Mask 0x201: cov_low_veg = 0.5 = 0x3f000000, then hits = 3 as uint16.
LEGACY_IN = hx("7902e003 b9b7e328 37750000  0100 5a e5 fb ee 0900  000000000000f83f")
LEGACY_OUT = hx("7902e003 b9b7e328 37750000  0100 5a e2 fb ee 0900  000000000000f83f  0000003f 0300")
# 2. extended (format 8, 38 bytes): byte 15 = 0xff is the flag byte and stays, byte 16 = 5 is the class.  low vegetation and bare
#    soil tie at 0.4 -> the lower index, low vegetation -> code 3.  Mask 0x100: weight = 1.25 = 0x3fa00000.
EXT_IN = hx("7902e003 b9b7e328 00000080  ffff 5a ff 05 ee 48f4 0102  000000000000f83f  0000 0080 ffff  0201")
EXT_OUT = hx("7902e003 b9b7e328 00000080  ffff 5a ff 03 ee 48f4 0102  000000000000f83f  0000 0080 ffff  0201  0000a03f")
# 3. odd L (format 6, 30 bytes + the file's own three extra bytes a1 b2 c3 = 33): p = 0.1, 0.2, NaN, 0.3 -> the NaN never wins,
#    high vegetation -> code 5.  Mask 0x202: cov_bare_soil = the NaN 0x7fc12345 bit for bit, hits = 65536 -> 0xffff.  39 bytes.
ODD_IN = hx("ffffffff ffffff7f 39300000  0080 a5 00 ff 00 0700 ffff  00000000000000c0  a1b2c3")
ODD_OUT = hx("ffffffff ffffff7f 39300000  0080 a5 00 05 00 0700 ffff  00000000000000c0  a1b2c3  4523c17f ffff")
# 4. unscored, kept (format 8, hits = 0, unscored = -1): the class byte 5 stays; mask 0x080: p_high_veg = the default NaN 0x7fc00000
KEPT_OUT = hx("7902e003 b9b7e328 00000080  ffff 5a ff 05 ee 48f4 0102  000000000000f83f  0000 0080 ffff  0201  0000c07f")
# 5. unscored, coded (format 0, 20 bytes, byte 15 = 0xa5, unscored = 1): byte 15 = 0xa0 | 1 = 0xa1; no extra bytes
CODED_IN = hx("00000080 9cffffff ffffff7f  ffff ff a5 7f 00 ffff")
CODED_OUT = hx("00000080 9cffffff ffffff7f  ffff ff a1 7f 00 ffff")
# 6. bad index (point_index = -1 and = T_src): 34 zero bytes each, n_bad = 2, nothing else counted


def test_hand_written_records_pin_the_restatement_and_the_librarys_rule(composer):
    s, w, h = cols((0.1, 0.7, 0.1, 0.1), 3)
    got, st = both(composer, LEGACY_IN, 1, 28, 1, s, w, h, mask=0x201, class_codes=WC.CODES)
    assert len(LEGACY_OUT) == 34 and got == LEGACY_OUT
    assert st["mins"] == st["maxs"] == (65012345, 686012345, 30007) and st["n_scored"] == 1 and st["n_bad"] == 0
    assert st["by_return"] == [0, 1] + [0] * 13                              # byte 14 = 0x5a: return number 0b010 in a legacy record
    s, w, h = cols((0.4, 0.4, 0.1, 0.1), 1)
    got, st = both(composer, EXT_IN, 8, 38, 1, s, w, h, mask=0x100, class_codes=WC.CODES)
    assert len(EXT_OUT) == 42 and got == EXT_OUT
    assert st["by_return"] == [0] * 9 + [1] + [0] * 5                        # 0x5a: return number 0xa in an extended record
    s, w, h = cols((0.1, 0.2, np.nan, 0.3), 65536, cov=(0.0, WC.NAN_PAYLOAD, 0.0, 0.0))
    got, st = both(composer, ODD_IN, 6, 33, 1, s, w, h, mask=0x202, class_codes=WC.CODES)
    assert len(ODD_OUT) == 39 and got == ODD_OUT
    assert st["mins"] == (-1, 2 ** 31 - 1, 12345)
    s, w, h = cols((np.nan,) * 4, 0, cov=(np.nan,) * 4, weight=0.0)
    got, st = both(composer, EXT_IN, 8, 38, 1, s, w, h, mask=0x080, class_codes=WC.CODES, unscored=-1)
    assert got == KEPT_OUT and st["n_scored"] == 0
    got, _ = both(composer, CODED_IN, 0, 20, 1, s, w, h, mask=0, class_codes=WC.CODES, unscored=1)
    assert got == CODED_OUT
    s, w, h = (np.repeat(a, 2, axis=-1) for a in cols((0.1, 0.7, 0.1, 0.1), 3))
    got, st = both(composer, LEGACY_IN, 1, 28, 1, s, w, h, point_index=[-1, 1], mask=0x201, class_codes=WC.CODES)
    assert got == bytes(68) and st == dict(mins=None, maxs=None, by_return=[0] * 15, n_bad=2, n_scored=0)
    # class_mode 0 leaves the field alone whatever the scores say
    s, w, h = cols((0.1, 0.7, 0.1, 0.1), 3)
    assert both(composer, LEGACY_IN, 1, 28, 1, s, w, h, mask=0x201)[0] == LEGACY_IN + LEGACY_OUT[28:]
    # a gather: record 1, record 0, record 1 of two
    two = LEGACY_IN + LEGACY_OUT[:28]
    assert both(composer, two, 1, 28, 2, point_index=[1, 0, 1])[0] == LEGACY_OUT[:28] + LEGACY_IN + LEGACY_OUT[:28]


# ---- planted wrong restatements: each must differ from the rule on the planted columns, or the cases would not notice the bug
PLANTED = len(WC.PLANTED_P) * len(WC.PLANTED_HITS)


@pytest.mark.parametrize("wrong,fmt,L,unscored", [("ties_last", 8, 38, -1), ("ge", 8, 38, -1), ("flags_cleared", 1, 28, -1),
                                                  ("class_at_15", 8, 38, -1), ("extras_first", 8, 41, -1), ("hits_wrap", 8, 38, -1),
                                                  ("unscored_zero", 8, 38, -1), ("unscored_zero", 3, 34, 1)])
def test_planted_wrong_restatement_differs(wrong, fmt, L, unscored, composer):
    T = PLANTED
    _, recs = WC.source(fmt, L, T, seed=3)
    s, w, h = WC.make_scores(T, seed=1)
    kw = dict(mask=0x3FF, class_codes=WC.CODES, unscored=unscored)
    right, _ = both(composer, recs, fmt, L, T, s, w, h, **kw)
    bad, _ = W.encode_ref(recs, fmt, L, T, s, w, h, wrong=wrong, **kw)
    assert len(right) == len(bad) == T * (L + 38)
    a, b = (np.frombuffer(x, dtype=np.uint8).reshape(T, L + 38) for x in (right, bad))
    assert (a != b).any(axis=1).sum() >= 1, wrong
    assert wrong in W.WRONG


def test_the_two_tie_mistakes_are_different_mistakes(composer):
    p = np.array([[np.nan, 0.4, 0.1], [0.2, 0.4, 0.1], [0.3, 0.1, 0.4], [0.1, 0.1, np.nan]], dtype=np.float32)
    assert W.best_class(p).tolist() == [0, 0, 2]                             # the rule as written: p[0] is where the search starts
    # the library's rule on the same three points: codes 10..13 name the winner in byte 16 of a format-6 record
    out = composer(bytes(90), 6, 30, 3, np.concatenate([np.zeros((4, 3), np.float32), p]), np.zeros(3, np.float32),
                   np.ones(3, np.int32), class_codes=(10, 11, 12, 13))
    assert [out[16], out[46], out[76]] == [10, 10, 12]
    assert W.best_class(p, "ge").tolist() == [0, 1, 2]
    assert W.best_class(p, "ties_last").tolist() == [2, 1, 3]                # and here a NaN in the last place wins


def test_cases_hold_the_edges_the_issue_names(composer):
    s, w, h = WC.make_scores(PLANTED + 500)
    # on all of them, gathered with planted bad indices, the library's rule is the restatement
    _, recs = WC.source(8, 41, 300, seed=5)
    index = np.random.default_rng(6).integers(-3, 303, size=PLANTED + 500)
    both(composer, recs, 8, 41, 300, s, w, h, point_index=index, mask=0x3FF, class_codes=WC.CODES, unscored=9)
    both(composer, recs, 3, 41, 300, s, w, h, point_index=index, mask=0x2AA, class_codes=WC.CODES)
    p = s[4:8, :PLANTED]
    for i in range(4):
        for j in range(i + 1, 4):
            others = [k for k in range(4) if k not in (i, j)]
            assert ((p[i] == p[j]) & (p[i] > p[others[0]]) & (p[i] > p[others[1]])).any(), (i, j)
    assert (np.isnan(p).any(axis=0) & (h[:PLANTED] > 0)).any()
    assert {0, 1, 65535, 65536} <= set(h.tolist())
    bits = s.view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0x7FC12345).any() and (bits == 0xFFC00001).any()
    assert (h[PLANTED:] == 0).any() and (h[PLANTED:] > 0).any()
    assert {c[3] for c in WC.SHAPE_CASES} >= {1, 255, 256, 257, 513}
    assert {(c[1], c[2]) for c in WC.SHAPE_CASES} >= {(f, None) for f in (0, 1, 2, 3, 6, 7, 8, 10)} | {(8, 39), (8, 41), (6, 33)}
    assert {c[4] for c in WC.SHAPE_CASES} >= set(WC.MASKS)
    assert [W.extra_bytes(m) for m in WC.MASKS] == [0, 4, 2, 18, 38]


# ---- las.patch_header
def vlr(user, rid, payload, description=b""):
    """a VLR typed from table 4: reserved u16, user id char[16], record id u16, length after header u16, description char[32]"""
    return struct.pack("<H16sHH32s", 0, user, rid, len(payload), description) + payload


def descriptor(data_type, name, options=0):
    d = bytearray(192)
    d[2], d[3] = data_type, options
    d[4:4 + len(name)] = name
    return bytes(d)


def with_frame(blob, vlrs=(), evlr=None, pad=0):
    """a file of write_las (no VLRs) -> the same with `vlrs` and `pad` zero bytes between header and points, and an EVLR behind them"""
    hs, off = struct.unpack_from("<HI", blob, 94)
    assert off == hs
    mid = b"".join(vlrs) + bytes(pad)
    head = bytearray(blob[:hs])
    struct.pack_into("<II", head, 96, hs + len(mid), len(vlrs))
    out = bytes(head) + mid + blob[hs:]
    if evlr is not None:
        out = bytearray(out + evlr)
        struct.pack_into("<QI", out, 235, len(out) - len(evlr), 1)
    return bytes(out)


STATS = SimpleNamespace(mins=(-5, 10, 7), maxs=(100, 2000, 7), by_return=(4, 2, 1, 0, 0, 0, 0) + (0,) * 8, n_bad=0, n_scored=5)
CRS = vlr(b"LASF_Projection", 2112, b"PROJCS[...]")          # 54 + 11 = 65 bytes
EVLR = struct.pack("<H16sHQ32s", 0, b"someone", 7, 5, b"") + b"hello"


def check_extents(f):
    for a in range(3):
        assert f["maxs"][a] == STATS.maxs[a] * C.SCALE[a] + C.OFFSET[a] and f["mins"][a] == STATS.mins[a] * C.SCALE[a] + C.OFFSET[a]


def test_patch_header_1_2_without_and_with_a_vlr_block():
    from stratanet2_vegetation_coverage_maps_amd import las
    plain = R.write_las(C.make_fields(7, 1), 3, None, (1, 2), scale=C.SCALE, offset=C.OFFSET)
    # no VLR, no field: nothing but the count, the by-return counts and the extents changes
    head, tail = las.patch_header(plain, 5, 0, STATS)
    assert len(head) == 227 and tail == b""
    f = W.parse_frame(head + bytes(5 * 34))
    assert (f["offset_to_points"], f["n_vlr"], f["L"], f["legacy_count"], f["legacy_by_return"]) == (227, 0, 34, 5, [4, 2, 1, 0, 0])
    check_extents(f)
    changed = [i for i in range(227) if head[i] != plain[i]]
    assert set(changed) <= set(range(107, 131)) | set(range(179, 227))
    # no VLR, all fields: one new VLR of 54 + 10 * 192 bytes
    head, _ = las.patch_header(plain, 7, 0x3FF, STATS)
    assert len(head) == 227 + 54 + 1920
    f = W.parse_frame(head + bytes(7 * 72))
    assert (f["offset_to_points"], f["n_vlr"], f["L"], f["legacy_count"]) == (2201, 1, 72, 7)
    assert W.extra_bytes_fields(head + bytes(7 * 72)) == [(n, 3 if n == "hits" else 9, 2 if n == "hits" else 4, 34 + 4 * k)
                                                           for k, n in enumerate(W.FIELD_NAMES)]
    # a CRS VLR and 9 bytes of padding in front: both verbatim, ours behind the CRS
    blob = with_frame(plain, [CRS], pad=9)
    head, _ = las.patch_header(blob, 7, 0x201, STATS)
    f = W.parse_frame(head + bytes(7 * 40))
    assert (f["offset_to_points"], f["n_vlr"], f["L"]) == (227 + 65 + 54 + 384 + 9, 2, 40)
    assert f["vlrs"][0][:3] == (b"LASF_Projection", 2112, b"PROJCS[...]") and head[227:227 + 65] == CRS and f["padding"] == bytes(9)
    assert f["vlrs"][1][0] == b"LASF_Spec" and f["vlrs"][1][1] == 4 and f["vlrs"][1][3] == 292
    assert W.extra_bytes_fields(head + bytes(7 * 40)) == [("cov_low_veg", 9, 4, 34), ("hits", 3, 2, 38)]
    h = las.read_header(head + bytes(7 * 40))
    assert (h.n_points, h.record_length, h.offset_to_points, h.point_format) == (7, 40, 739, 3)
    # the file of the source's length is accepted too when nothing is appended
    assert las.read_header(las.patch_header(blob, 7, 0, STATS)[0] + bytes(7 * 34)).offset_to_points == 227 + 65 + 9


def test_patch_header_1_4_prior_extra_bytes_undocumented_bytes_and_an_evlr():
    from stratanet2_vegetation_coverage_maps_amd import las
    # format 8 with 3 + 4 of the file's own extra bytes: L = 45.  A prior Extra Bytes VLR documents the LAST four (one uint32) only
    # after an explicit 3-byte type-0 entry; a second file documents nothing.
    src = R.write_las(C.make_fields(6, 2), 8, 45, (1, 4), scale=C.SCALE, offset=C.OFFSET, legacy_count=0)
    prior = vlr(b"LASF_Spec", 4, descriptor(0, b"pad", 3) + descriptor(5, b"mine"), b"Extra Bytes")          # 54 + 384 = 438 bytes
    blob = with_frame(src, [CRS, prior], evlr=EVLR)
    head, tail = las.patch_header(blob, 4, 0x300, STATS)
    assert tail == EVLR
    out = head + bytes(4 * 51) + tail
    f = W.parse_frame(out)
    # 375 + 65 + (438 + 2 * 192) = 1262: the prior VLR grew in place, no VLR was added
    assert (f["offset_to_points"], f["n_vlr"], f["L"], f["legacy_count"], f["count64"]) == (1262, 2, 51, 0, 4)
    assert f["legacy_by_return"] == [0] * 5 and f["by_return"] == list(STATS.by_return)
    assert (f["first_evlr"], f["n_evlr"], f["evlrs"]) == (1262 + 4 * 51, 1, EVLR)
    assert W.extra_bytes_fields(out) == [("pad", 0, 3, 38), ("mine", 5, 4, 41), ("weight", 9, 4, 45), ("hits", 3, 2, 49)]
    check_extents(f)
    assert las.read_header(out).n_points == 4 and las.read_header(out).record_length == 51
    # undocumented: 7 bytes no descriptor covers -> a type-0 entry of 7 bytes first, ours at byte 45
    blob = with_frame(src, [CRS])
    head, tail = las.patch_header(blob, 6, 0x001, STATS)
    out = head + bytes(6 * 49)
    assert tail == b"" and W.parse_frame(out)["offset_to_points"] == 375 + 65 + 54 + 2 * 192 and W.parse_frame(out)["first_evlr"] == 0
    assert W.extra_bytes_fields(out) == [("undocumented", 0, 7, 38), ("cov_low_veg", 9, 4, 45)]
    # a prior VLR that covers part: 3 of 7 bytes documented -> the other 4 undocumented behind them
    blob = with_frame(src, [vlr(b"LASF_Spec", 4, descriptor(0, b"pad", 3))])
    out = las.patch_header(blob, 6, 0x200, STATS)[0] + bytes(6 * 47)
    assert W.extra_bytes_fields(out) == [("pad", 0, 3, 38), ("undocumented", 0, 4, 41), ("hits", 3, 2, 45)]
    # descriptors that cover more than the record holds are refused
    with pytest.raises(ValueError, match="cover"):
        las.patch_header(with_frame(src, [vlr(b"LASF_Spec", 4, descriptor(10, b"wide"))]), 6, 0x200, STATS)
    # a 1.4 file whose legacy count is set keeps a legacy count
    legacy = R.write_las(C.make_fields(6, 2), 1, None, (1, 4), scale=C.SCALE, offset=C.OFFSET)
    f = W.parse_frame(las.patch_header(legacy, 3, 0, STATS)[0] + bytes(3 * 28))
    assert (f["legacy_count"], f["count64"], f["legacy_by_return"]) == (3, 3, [4, 2, 1, 0, 0])
    # no statistics: zero extents and counts
    f = W.parse_frame(las.patch_header(legacy, 3, 0)[0] + bytes(3 * 28))
    assert f["maxs"] == f["mins"] == (0.0, 0.0, 0.0) and f["by_return"] == [0] * 15


def test_field_names_and_masks():
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    from stratanet2_vegetation_coverage_maps_amd import las
    assert list(las.FIELDS) == W.FIELD_NAMES and las.DEFAULT_CLASS_CODES == WC.CODES
    assert ops.las_field_mask("all") == 0x3FF and ops.las_field_mask(()) == 0 and ops.las_field_mask(("hits", "cov_low_veg")) == 0x201
    assert [ops.las_extra_bytes(m) for m in WC.MASKS] == [W.extra_bytes(m) for m in WC.MASKS]
    with pytest.raises(ValueError, match="fields"):
        ops.las_field_mask(("hit",))


# ---- the C ABI
def test_las_write_is_part_of_the_build():
    from stratanet2_vegetation_coverage_maps_amd import _build, _lib
    assert "las_write.hip" in _build.SOURCES and "las_write_rules.h" in _build.HEADERS
    assert {"sn2_las_encode", "sn2_las_encode_stage_max", "sn2_debug_las_encode_form"} <= set(_lib.SIGNATURES)
    assert _lib.SN2_LAS_STATS_BYTES == 160 == struct.calcsize("<3i3i15QQQ")
    assert 67 < _lib.load().sn2_las_encode_stage_max() <= 65535


def test_encode_argument_checks_return_before_any_device_work():
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    fake = 0x10000                                            # 16-byte aligned, never dereferenced: every call fails a check first
    good_codes = (ctypes.c_int * 4)(3, 2, 4, 5)

    def call(src=fake, src_bytes=38 * 100, fmt=8, L=38, T_src=100, index=None, T_out=100, scores=fake, weight=fake, hits=fake,
             stride=100, col0=0, mask=0x3FF, mode=1, codes=good_codes, unscored=-1, dst=fake, dst_bytes=76 * 100, stats=fake):
        return lib.sn2_las_encode(src, src_bytes, fmt, L, T_src, index, T_out, scores, weight, hits, stride, col0, mask, mode, codes,
                                  unscored, dst, dst_bytes, stats, None)
    EINVAL, ELIMIT = -1, -2
    assert call(src=None) == EINVAL and call(dst=None) == EINVAL and call(stats=None) == EINVAL
    assert call(scores=None) == EINVAL and call(weight=None) == EINVAL and call(hits=None) == EINVAL
    assert call(scores=None, weight=None, hits=None, mask=1, mode=0, dst_bytes=10 ** 6) == EINVAL          # a field needs the scores
    assert call(scores=None, weight=None, hits=None, mask=0, mode=1, dst_bytes=10 ** 6) == EINVAL          # and so does a class
    assert call(mode=1, codes=None) == EINVAL
    assert call(T_out=0) == EINVAL and call(T_out=-3) == EINVAL and call(T_src=0) == EINVAL and call(T_src=-1, index=fake) == EINVAL
    assert call(fmt=0x80 | 8) == EINVAL and call(fmt=0x40 | 8) == EINVAL                                    # LAZ
    assert call(fmt=11) == EINVAL and call(fmt=-1) == EINVAL
    for fmt, least in R.LAYOUTS.items():
        assert call(fmt=fmt, L=least[1] - 1, src_bytes=10 ** 6, dst_bytes=10 ** 6, codes=(ctypes.c_int * 4)(1, 2, 3, 4)) == EINVAL, fmt
    assert call(L=65536, src_bytes=10 ** 8, dst_bytes=10 ** 8) == EINVAL
    assert call(L=65535 - 37, src_bytes=10 ** 8, dst_bytes=10 ** 8) == EINVAL                              # L_dst = 65536
    assert call(src_bytes=38 * 100 - 1) == EINVAL and call(dst_bytes=76 * 100 - 1) == EINVAL
    assert call(mask=0x200, dst_bytes=40 * 100 - 1) == EINVAL
    assert call(src=fake + 8) == EINVAL and call(dst=fake + 4) == EINVAL and call(stats=fake + 4) == EINVAL
    assert call(col0=-1) == EINVAL and call(col0=1) == EINVAL and call(stride=99) == EINVAL
    assert call(T_out=101, dst_bytes=10 ** 6, stride=101) == EINVAL                                         # no index: record 100 of 100
    assert call(mask=0x400) == EINVAL and call(mask=-1) == EINVAL and call(mode=2) == EINVAL and call(mode=-1) == EINVAL
    for bad in ((256, 2, 4, 5), (3, -1, 4, 5), (3, 2, 4, 1000)):
        assert call(codes=(ctypes.c_int * 4)(*bad)) == EINVAL, bad
    assert call(unscored=256) == EINVAL and call(unscored=-2) == EINVAL
    assert call(fmt=3, L=34, src_bytes=34 * 100, codes=(ctypes.c_int * 4)(3, 2, 4, 32)) == EINVAL          # legacy: five bits
    assert call(fmt=3, L=34, src_bytes=34 * 100, unscored=32) == EINVAL
    assert call(T_out=2 ** 31, index=fake, dst_bytes=76 * 2 ** 31, stride=2 ** 31) == ELIMIT
    assert call(T_src=2 ** 31, src_bytes=38 * 2 ** 31, index=fake) == ELIMIT
    assert lib.sn2_debug_las_encode_form(2) == EINVAL and lib.sn2_debug_las_encode_form(0) == 0
