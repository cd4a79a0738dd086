"""The rule of the LAS encoder (include/strata_hip.h, "LAS point records, written") in numpy, over the packed structured dtypes of
tests/_las_ref.py, and a reader of a written file's frame -- header, VLRs, the Extra Bytes VLR, EVLRs -- written from the ASPRS
LAS 1.4 specification (tables 3, 4, 24-26) a second time.  Nothing here shares code with csrc/las_write.hip, csrc/las_write_rules.h
or las.py's header writer.  `encode_ref(..., wrong=...)` states the rule wrongly on purpose, one planted mistake at a time."""
import struct

import numpy as np

import _las_ref as R

FIELD_NAMES = ["cov_low_veg", "cov_bare_soil", "cov_medium_veg", "cov_high_veg", "p_low_veg", "p_bare_soil", "p_medium_veg",
               "p_high_veg", "weight", "hits"]
WRONG = ("ties_last", "ge", "flags_cleared", "class_at_15", "extras_first", "hits_wrap", "unscored_zero")


def extra_bytes(mask):
    return sum(2 if k == 9 else 4 for k in range(10) if mask >> k & 1)


def out_dtype(fmt, L_src, mask, extras_at=None):
    """the source format's fields at their offsets, then the appended fields at L_src (or at `extras_at`)"""
    fields, _ = R.LAYOUTS[fmt]
    names, formats, offsets = [f[0] for f in fields], [f[1] for f in fields], [f[2] for f in fields]
    at = L_src if extras_at is None else extras_at
    for k in range(10):
        if mask >> k & 1:
            names.append("x_" + FIELD_NAMES[k])
            formats.append("<u2" if k == 9 else "<u4")
            offsets.append(at)
            at += 2 if k == 9 else 4
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": L_src + extra_bytes(mask)})


def best_class(p, wrong=None):
    """p (4,T) fp32 -> (T) index of the largest, strictly: ties to the lowest index, a NaN never wins"""
    T = p.shape[1]
    cols = np.arange(T)
    if wrong == "ties_last":                                   # from the last class down
        best = np.full(T, 3)
        for k in (2, 1, 0):
            with np.errstate(invalid="ignore"):
                best[p[k] > p[best, cols]] = k
        return best
    best = np.zeros(T, dtype=np.int64)
    for k in (1, 2, 3):
        with np.errstate(invalid="ignore"):
            best[(p[k] >= p[best, cols]) if wrong == "ge" else (p[k] > p[best, cols])] = k
    return best


def encode_ref(records, fmt, L_src, T_src, scores=None, weight=None, hits=None, point_index=None, n_out=None, col0=0, mask=0,
               class_codes=None, unscored=-1, wrong=None):
    """records: bytes that start at the first source record; scores (8,S) fp32, weight (S) fp32, hits (S) int32 numpy or None.
    -> (T_out * L_dst bytes, stats: dict(mins, maxs, by_return (15), n_bad, n_scored))"""
    srcb = np.frombuffer(records, dtype=np.uint8, count=T_src * L_src).reshape(T_src, L_src)
    idx = np.arange(T_src, dtype=np.int64) if point_index is None else np.asarray(point_index, dtype=np.int64)
    T_out = len(idx) if n_out is None else n_out
    idx = idx[:T_out]
    good = (idx >= 0) & (idx < T_src)
    E = extra_bytes(mask)
    L_dst = L_src + E
    least = R.LAYOUTS[fmt][1]
    extras_at = least if wrong == "extras_first" else None
    out = np.zeros(T_out, dtype=out_dtype(fmt, L_src, mask, extras_at))
    ob = out.view(np.uint8).reshape(T_out, L_dst)
    if wrong == "extras_first":                                # the source's own extra bytes pushed behind the new ones
        ob[good, :least] = srcb[idx[good], :least]
        ob[good, least + E:] = srcb[idx[good], least:]
    else:
        ob[good, :L_src] = srcb[idx[good]]
    cols = slice(col0, col0 + T_out)
    h = np.zeros(T_out, dtype=np.int64) if hits is None else hits[cols].astype(np.int64)
    scored = (h > 0) & good
    if class_codes is not None:
        best = best_class(scores[4:8, cols], wrong)
        code = np.asarray(class_codes, dtype=np.int64)[best]
        code = np.where(h > 0, code, 0 if wrong == "unscored_zero" else unscored)
        write = good & (code >= 0)
        if fmt >= 6:
            name = "flags" if wrong == "class_at_15" else "classification"            # byte 15 of an extended record: its flags
            out[name][write] = code[write]
        else:
            keep = 0 if wrong == "flags_cleared" else 0xE0
            out["classification"][write] = (out["classification"][write] & keep) | code[write]
    for k in range(10):
        if not mask >> k & 1:
            continue
        if k < 8:
            v = scores[k, cols].view(np.uint32)
        elif k == 8:
            v = weight[cols].view(np.uint32)
        else:
            v = (h & 0xFFFF) if wrong == "hits_wrap" else np.clip(h, 0, 65535)
        out["x_" + FIELD_NAMES[k]][good] = v[good]
    g = out[good]
    stats = dict(mins=None, maxs=None, by_return=[0] * 15, n_bad=int((~good).sum()), n_scored=int(scored.sum()))
    if len(g):
        stats["mins"] = tuple(int(g[k].min()) for k in "XYZ")
        stats["maxs"] = tuple(int(g[k].max()) for k in "XYZ")
        r = g["returns"].astype(np.int64) & (15 if fmt >= 6 else 7)
        stats["by_return"] = [int((r == b + 1).sum()) for b in range(15)]
    return out.tobytes(), stats


# ---- the frame of a file, read back (LAS 1.4 R15: table 3 the public header, table 4 the VLR header, 24-26 the Extra Bytes)
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 2, 5: 4, 6: 4, 7: 8, 8: 8, 9: 4, 10: 8}


def parse_frame(blob):
    """-> dict: the header's patched fields, the VLRs as (user id, record id, payload, byte offset), the bytes between the last
    VLR and the points, the EVLR bytes"""
    minor = blob[25]
    hs, off, n_vlr = struct.unpack_from("<HII", blob, 94)
    fmt, L, legacy = struct.unpack_from("<BHI", blob, 104)
    f = dict(minor=minor, header_size=hs, offset_to_points=off, n_vlr=n_vlr, fmt=fmt, L=L, legacy_count=legacy,
             legacy_by_return=list(struct.unpack_from("<5I", blob, 111)), scale=struct.unpack_from("<3d", blob, 131),
             offset=struct.unpack_from("<3d", blob, 155))
    e = struct.unpack_from("<6d", blob, 179)
    f["maxs"], f["mins"] = (e[0], e[2], e[4]), (e[1], e[3], e[5])
    f["count"] = legacy
    f["first_evlr"], f["n_evlr"], f["by_return"] = 0, 0, None
    if minor >= 4:
        f["first_evlr"], f["n_evlr"] = struct.unpack_from("<QI", blob, 235)
        f["count64"] = struct.unpack_from("<Q", blob, 247)[0]
        f["by_return"] = list(struct.unpack_from("<15Q", blob, 255))
        if legacy == 0:
            f["count"] = f["count64"]
    at, vlrs = hs, []
    for _ in range(n_vlr):
        user = blob[at + 2:at + 18].split(b"\0")[0]
        rid, n = struct.unpack_from("<HH", blob, at + 18)
        vlrs.append((user, rid, blob[at + 54:at + 54 + n], at))
        at += 54 + n
    assert at <= off
    f["vlrs"], f["padding"] = vlrs, blob[at:off]
    f["points"] = blob[off:off + f["count"] * L]
    f["evlrs"] = blob[f["first_evlr"]:] if f["n_evlr"] else b""
    return f


def extra_bytes_fields(blob):
    """the descriptors of the file's Extra Bytes VLR (LASF_Spec, 4) -> [(name, data type, size in bytes, byte offset in the record)],
    the first of them right behind the format's own fields"""
    f = parse_frame(blob)
    own = [v for v in f["vlrs"] if v[0] == b"LASF_Spec" and v[1] == 4]
    assert len(own) <= 1
    out, at = [], R.LAYOUTS[f["fmt"]][1]
    if own:
        payload = own[0][2]
        assert len(payload) % 192 == 0
        for i in range(0, len(payload), 192):
            d = payload[i:i + 192]
            t, options = d[2], d[3]
            size = options if t == 0 else TYPE_SIZE[t]
            out.append((d[4:36].split(b"\0")[0].decode(), t, size, at))
            at += size
    return out
