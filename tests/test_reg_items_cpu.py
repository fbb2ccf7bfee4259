"""RegTerm.items (pkc/engine.py), the host side of the regulariser kernels: the row-slice items it
cuts the cost_l1 / cost_l2 / cost_gl blocks into, against torch.chunk (utils.py:49-54: the blocks of
cost_gl are torch.chunk(p, nblk, 1) x torch.chunk(., nblk, 0), in that order)."""
import pytest
import torch

from pkc.engine import RegTerm

ROWS = [1, 2, 3, 5, 7, 8, 9, 10, 16, 33, 48, 100]
COLS = [2, 3, 5, 7, 9, 10, 11, 32, 40, 1030, 5000]
NBLK = [1, 2, 3, 4, 5, 7, 16]


def _check(p2d, items, bstart, blocks, p, g):
    """items / bstart describe `blocks` (2-D tensors, in order) of the flattened parameter p2d."""
    assert len(bstart) - 1 == len(blocks)
    assert bstart[0] == 0 and bstart[-1] == len(items)
    for b, blk in enumerate(blocks):
        lo, hi = bstart[b], bstart[b + 1]
        assert lo < hi, "block %d has no item" % b
        parts = []
        for ip, ig, ld, r0, r1, c0, c1, ib in items[lo:hi]:
            assert ip is p and ig is g and ib == b
            assert ld == p2d.shape[1]
            assert 0 <= r0 < r1 <= p2d.shape[0] and 0 <= c0 < c1 <= p2d.shape[1]
            assert (r1 - r0) * (c1 - c0) <= max(4096, c1 - c0)
            parts.append(p2d[r0:r1, c0:c1])
        assert torch.equal(torch.cat(parts, 0), blk), "block %d" % b


@pytest.mark.parametrize("nblk", NBLK)
def test_gl_items_are_the_torch_chunk_blocks(nblk):
    for R in ROWS:
        for Cc in COLS:
            p = torch.arange(R * Cc, dtype=torch.float32).view(R, Cc)
            g = torch.zeros(1)
            items, bstart = RegTerm("cost_gl", 0.5, nblk, [p]).items({id(p): g})
            blocks = [blk for col in torch.chunk(p, nblk, 1) for blk in torch.chunk(col, nblk, 0)]
            _check(p, items, bstart, blocks, p, g)


@pytest.mark.parametrize("op", ["cost_l1", "cost_l2"])
def test_l1_l2_one_block_per_parameter(op):
    params = [torch.arange(R * Cc, dtype=torch.float32).view(R, Cc) + 1000 * i
              for i, (R, Cc) in enumerate([(300, 1030), (5, 5000), (1, 2), (48, 40), (100, 11)])]
    grads = {id(p): torch.zeros(1) for p in params}
    items, bstart = RegTerm(op, 1e-3, None, params).items(grads)
    assert len(bstart) - 1 == len(params)
    for b, p in enumerate(params):
        sub = items[bstart[b]:bstart[b + 1]]
        rows = torch.cat([it[0][it[3]:it[4], it[5]:it[6]] for it in sub], 0)
        assert torch.equal(rows, p)
        assert all(it[0] is p and it[1] is grads[id(p)] and it[7] == b and it[2] == p.shape[1]
                   and (it[4] - it[3]) * (it[6] - it[5]) <= max(4096, it[6] - it[5]) for it in sub)
    # 300 x 1030: 3 rows per item, one block of 100 items; 5 x 5000: a row per item (per = 1)
    assert bstart[1] - bstart[0] == 100
    assert bstart[2] - bstart[1] == 5


def test_3d_parameter_flattens_to_rows_by_rest():
    p = torch.arange(4 * 3 * 5, dtype=torch.float32).view(4, 3, 5)
    g = torch.zeros(1)
    for op in ("cost_l1", "cost_l2"):
        items, bstart = RegTerm(op, 1.0, None, [p]).items({id(p): g})
        assert bstart == [0, len(items)]
        flat = p.reshape(4, 15)
        rows = torch.cat([flat[r0:r1, c0:c1] for _, _, _, r0, r1, c0, c1, _ in items], 0)
        assert torch.equal(rows, flat)
        assert all(it[0] is p and it[1] is g and it[2] == 15 and it[7] == 0 for it in items)
    big = torch.zeros(3, 70, 100)                 # 7000 per row: wider than 4096, a row per item
    items, bstart = RegTerm("cost_l2", 1.0, None, [big]).items({})
    assert [(it[3], it[4], it[5], it[6]) for it in items] == [(r, r + 1, 0, 7000) for r in range(3)]
    assert all(it[2] == 7000 for it in items)


def test_parameter_missing_from_grads_gives_no_gradient_buffer():
    a, b = torch.ones(9, 10), torch.ones(100, 70)
    gb = torch.zeros(100, 70)
    for op, nblk in (("cost_l1", None), ("cost_l2", None), ("cost_gl", 4)):
        items, bstart = RegTerm(op, 1.0, nblk, [a, b]).items({id(b): gb})
        assert all(it[1] is None for it in items if it[0] is a)
        assert all(it[1] is gb for it in items if it[0] is b)
        assert any(it[0] is a for it in items) and any(it[0] is b for it in items)
        # blocks in parameter order: every item of a comes before every item of b
        first_b = min(i for i, it in enumerate(items) if it[0] is b)
        assert all(it[0] is a for it in items[:first_b])
        assert [it[7] for it in items] == sorted(it[7] for it in items)
        assert bstart[-1] == len(items)
    # cost_gl with nblk = 4 on 9 x 10: chunks of 3 -> 3 row chunks x 4 column chunks (3, 3, 3, 1)
    items, bstart = RegTerm("cost_gl", 1.0, 4, [a]).items({})
    assert len(bstart) - 1 == len(torch.chunk(a, 4, 0)) * len(torch.chunk(a, 4, 1)) == 12
