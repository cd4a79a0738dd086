"""The inverted 3-NN index built in a given order of the target rows (sn2_interp_index_ordered, csrc/interp_index.hip), against a
host construction in numpy from the same 3-NN table: whatever order the rows are walked in -- their own, a random one, the one
the grid search of sn2_three_nn_xy leaves in its workspace -- and whichever way the table is read (a gather through the order,
or the search's sorted copy), every source's list holds the same (row, normalised weight) entries, and cnt / off / the item
table / the chunk table are what tests/test_gpu_geometry.py::test_inverted_index_and_its_chunk_table asks of them.

Weights are compared BIT FOR BIT: inv_fill_kernel writes w_j * (1 / ((w0 + w1) + w2)) in float32, a correctly rounded division
and one multiplication with nothing to contract, and numpy's float32 arithmetic rounds each of those steps the same way."""
import numpy as np
import pytest
import torch

from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

pytestmark = pytest.mark.gpu

F32 = np.float32


def _host_lists(idx, w, B, R, S, row_perm=None):
    """-> (cnt (B*S), entries (n,3) int64 sorted rows of (global source, listed row, weight bits)) from the table alone."""
    idx, w = idx.reshape(B, R, 3), w.reshape(B, R, 3).astype(F32)
    inv = F32(1.0) / ((w[..., 0] + w[..., 1]) + w[..., 2])
    wn = (w * inv[..., None]).astype(F32)
    listed = w != 0
    listed[..., 0] = True
    b, r, j = np.nonzero(listed)
    src = b * S + idx[b, r, j]
    row = r if row_perm is None else row_perm.reshape(B, R)[b, r]
    ent = np.stack([src.astype(np.int64), row.astype(np.int64), wn[b, r, j].view(np.int32).astype(np.int64)], 1)
    return np.bincount(src, minlength=B * S), ent[np.lexsort((ent[:, 2], ent[:, 1], ent[:, 0]))]


def _check_index(ws, cnt_want, ent_want, B, R, S):
    words = ws.cpu().view(torch.int32).numpy()
    SL = (R + 2047) // 2048
    o_off = B * SL * S
    o_cnt = o_off + B * S
    o_row = o_cnt + B * S
    o_w = o_row + 3 * B * R
    o_items = (o_w + 3 * B * R + 3) // 4 * 4
    CM = ops.interp_chunks(R, S)
    o_chunks = o_items + 4 * B * S
    assert o_chunks + 4 * B * CM <= ops.interp_ws_words(B, R, S)
    off, cnt = words[o_off:o_off + B * S], words[o_cnt:o_cnt + B * S]
    inv_row, inv_w = words[o_row:o_row + 3 * B * R], words[o_w:o_w + 3 * B * R]
    items = words[o_items:o_items + 4 * B * S].reshape(B, S, 4)
    chunks = words[o_chunks:o_chunks + 4 * B * CM].reshape(B, CM, 4)
    assert np.array_equal(cnt, cnt_want)
    # off: per plot the exclusive scan of cnt behind the plot's 3 R places
    c2 = cnt.reshape(B, S).astype(np.int64)
    assert np.array_equal(off.reshape(B, S), np.arange(B)[:, None] * 3 * R + np.cumsum(c2, 1) - c2)
    # the lists: the used places of plot b are [3 R b, 3 R b + sum cnt), source after source
    got = []
    for b in range(B):
        n = int(c2[b].sum())
        pl = slice(3 * R * b, 3 * R * b + n)
        got.append(np.stack([np.repeat(np.arange(b * S, (b + 1) * S), c2[b]), inv_row[pl].astype(np.int64), inv_w[pl].astype(np.int64)], 1))
    got = np.concatenate(got)
    got = got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))]
    assert got.shape == ent_want.shape
    bad = np.nonzero((got != ent_want).any(1))[0]
    assert bad.size == 0, f"{bad.size} list entries differ, first: got {got[bad[0]]} want {ent_want[bad[0]]}"
    # item and chunk tables
    for b in range(B):
        assert sorted(items[b, :, 0].tolist()) == list(range(b * S, (b + 1) * S))
        first = 0
        for k in range(S):
            sid, o, n, f = items[b, k]
            assert o == off[sid] and n == cnt[sid] and f == first
            nch = (n + 62) // 63
            for c in range(nch):
                assert chunks[b, first + c].tolist() == [sid, o + 63 * c, min(63, n - 63 * c), b]
            first += nch
        assert not chunks[b, first:].any()
    return cnt


def _perms(g, B, R):
    return torch.stack([torch.randperm(R, generator=g) for _ in range(B)]).int().view(-1)


@pytest.mark.parametrize("B,R,S", [(2, 300, 1),            # every lane of every wave on one cursor, a multi-chunk list
                                   (3, 2049, 100),         # second slice of one row, two-dimensional grid
                                   (8, 2049, 128),         # XCD placement, one plot per XCD
                                   (16, 2560, 128),        # XCD placement, two plots per XCD
                                   (1, 3000, 1025)])       # the scans cross a round of 1024 sources
def test_ordered_index_equals_the_host_lists(B, R, S):
    g = torch.Generator().manual_seed(B * 1000 + S)
    top = S - S // 5 if S > 4 else S
    idx = (torch.rand(B * R, 3, generator=g) ** 3 * top).long().clamp_(0, S - 1).int()
    w = torch.rand(B * R, 3, generator=g) + 0.1
    w[::7, 2] = 0.0
    pos = torch.rand(B * S, 4, generator=g).cuda()
    ident = torch.arange(R, dtype=torch.int32).repeat(B)
    order, row_perm = _perms(g, B, R), _perms(g, B, R)
    rows_of = (torch.arange(B).repeat_interleave(R) * R + order.long())          # global row of every position
    table = (idx[rows_of].contiguous().cuda(), w[rows_of].contiguous().cuda())
    knn = (idx.cuda(), w.cuda())
    plain = _host_lists(idx.numpy(), w.numpy(), B, R, S)
    permuted = _host_lists(idx.numpy(), w.numpy(), B, R, S, row_perm.numpy())
    variants = [("identity order", dict(row_order=ident.cuda()), plain),
                ("random order, gather", dict(row_order=order.cuda()), plain),
                ("random order, sorted table", dict(row_order=order.cuda(), sorted_table=table), plain),
                ("random order, gather, row_perm", dict(row_order=order.cuda(), row_perm=row_perm.cuda()), permuted),
                ("random order, sorted table, row_perm", dict(row_order=order.cuda(), sorted_table=table, row_perm=row_perm.cuda()), permuted)]
    for what, kw, (cnt_want, ent_want) in variants:
        ws = ops.interp_index(knn, B, R, S, src_pos=pos, **kw)
        torch.cuda.synchronize()
        cnt = _check_index(ws, cnt_want, ent_want, B, R, S)
    assert S == 1 or (cnt.max() > 4 * 63 and (cnt == 0).any())


def test_index_in_the_order_the_grid_search_leaves():
    """Through the search: B = 8, S = 128, T = 2304 (the smallest shapes of the grid route), half of every plot's targets in one
    cell of the source grid.  The order in the workspace is a permutation per plot, the sorted copy is the table in that order
    bit for bit, and the index built from either equals the host's."""
    B, S, T = 8, 128, 2304
    assert ops.three_nn_uses_grid(S, T)
    g = torch.Generator().manual_seed(7)
    src = torch.rand(B, 3, S, generator=g)
    dst = torch.rand(B, 3, T, generator=g)
    dst[:, :2, T // 2:] = 0.41 + 0.18 * dst[:, :2, T // 2:]         # G = 5 cells of ~0.2 a side: inside the middle cell
    ws = torch.empty(ops.three_nn_ws_words(B, S, T), dtype=torch.int32, device="cuda")
    idx, w = ops.three_nn(src.cuda(), dst.cuda(), 3, ws=ws, sorted_copy=True)
    order, si, sw = ops.three_nn_order(ws, B, S, T)
    torch.cuda.synchronize()
    o = order.cpu().view(B, T).long()
    assert torch.equal(o.sort(1).values, torch.arange(T).expand(B, T))
    rows_of = (torch.arange(B)[:, None] * T + o).view(-1)
    assert torch.equal(si.cpu(), idx.cpu()[rows_of])
    assert torch.equal(sw.cpu().view(torch.int32), w.cpu()[rows_of].view(torch.int32))
    # the full scan's table is the same table
    idx_f, w_f = ops.three_nn(src.cuda(), dst.cuda(), 3, grid=False)
    assert torch.equal(idx_f, idx) and torch.equal(w_f, w)
    pos = torch.cat([src.permute(0, 2, 1).reshape(B * S, 3), torch.zeros(B * S, 1)], 1).contiguous().cuda()
    cnt_want, ent_want = _host_lists(idx.cpu().numpy(), w.cpu().numpy(), B, T, S)
    for kw in (dict(row_order=order, sorted_table=(si, sw)), dict(row_order=order)):
        inv = ops.interp_index((idx, w), B, T, S, src_pos=pos, **kw)
        torch.cuda.synchronize()
        _check_index(inv, cnt_want, ent_want, B, T, S)
