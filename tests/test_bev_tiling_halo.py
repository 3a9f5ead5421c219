"""BEV tiling with a halo (bev_tiling.halo_tables): the needed-panel tables of a tile, built on the host.  No GPU."""
import pytest
import torch

from bevformer_amd import bev_tiling
from bevformer_amd import synthetic as S

DEFAULT_H = 16      # the halo the GPU tests (tests/test_bev_tiling_halo_gpu.py) run with


def _tile_cells(bev_h, bev_w, world, rank, layout):
    if layout == "rows":
        h0, h1 = bev_tiling.row_blocks(bev_h, world)[rank]
        return torch.arange(h0 * bev_w, h1 * bev_w)
    q0, q1 = bev_tiling.query_blocks(bev_h * bev_w, world)[rank]
    return bev_tiling.sector_order(bev_h, bev_w, S.PC_RANGE, "cpu")[3][q0:q1]


@pytest.mark.parametrize("layout", ["rows", "sectors"])
@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("name", ["base", "tiny", "micro4"])
def test_every_cell_within_the_halo_lies_in_a_marked_panel(name, world, layout):
    """For every rank: each cell within ``H`` cells (in both grid directions) of a tile cell lies in a panel marked in BOTH
    tables; the projection's table contains the flag's table and, around every marked panel, the ``bev_w + 1`` rows the
    sampling kernel's zero-coefficient taps reach (cyclically).  At base size, G = 8 and the default H the marked share is
    below 1 — the share is what the rank still projects; it is printed.  ``tiny`` (50 x 50 = 2,500 cells = 39.06 panels) is the
    grid whose last panel is partial: the padded tail, the cyclic wrap over it, and (H = 3) panels left unmarked at G = 8;
    ``micro4`` (120 cells, two panels) is the degenerate end: everything marked."""
    w = S.WORKLOADS[name]
    bev_h, bev_w = w["bev_h"], w["bev_w"]
    Q, P = bev_h * bev_w, bev_tiling.HALO_PANEL_ROWS
    H = {"base": DEFAULT_H, "tiny": 3, "micro4": 2}[name]
    shares = []
    for rank in range(world):
        cells = _tile_cells(bev_h, bev_w, world, rank, layout)
        tables = bev_tiling.halo_tables(bev_h, bev_w, cells, H)
        assert tables.dtype == torch.int32 and tuple(tables.shape) == (2, (Q + P - 1) // P)
        need, proj = tables[0].bool(), tables[1].bool()
        # brute force, independent of the builder's pooling: the cells within H of a tile cell
        cy, cx = cells // bev_w, cells % bev_w
        near = torch.zeros(bev_h, bev_w, dtype=torch.bool)
        for dy in range(-H, H + 1):
            y = cy + dy
            for dx in range(-H, H + 1):
                x = cx + dx
                ok = (y >= 0) & (y < bev_h) & (x >= 0) & (x < bev_w)
                near[y[ok], x[ok]] = True
        near_cells = near.view(-1).nonzero().squeeze(1)
        assert need[near_cells // P].all()
        # ... and no panel is marked without such a cell in it (the table is exactly the panels of the dilated tile)
        want_need = torch.zeros_like(need)
        want_need[near_cells // P] = True
        assert torch.equal(need, want_need)
        assert (proj | ~need).all()                                           # need is a subset of proj
        rows = need.repeat_interleave(P)[:Q].nonzero().squeeze(1)
        for d in (-(bev_w + 1), -1, 1, bev_w + 1):
            assert proj[((rows + d) % Q) // P].all()
        # brute force of the projection table too: the panels with a row within bev_w + 1 (cyclically) of a needed panel's row
        reach = torch.zeros(Q, dtype=torch.bool)
        for d in range(-(bev_w + 1), bev_w + 2):
            reach[(rows + d) % Q] = True
        want_proj = torch.zeros_like(proj)
        want_proj[reach.nonzero().squeeze(1) // P] = True
        assert torch.equal(proj, want_proj)
        shares.append((need.float().mean().item(), proj.float().mean().item()))
    flag_share = sum(s[0] for s in shares) / world
    proj_share = sum(s[1] for s in shares) / world
    print(f"{name} {layout} G={world} H={H}: marked share of the panels, mean over ranks: flag table {flag_share:.3f}, "
          f"projection table {proj_share:.3f}; per rank (projection) {[round(s[1], 3) for s in shares]}")
    if name in ("base", "tiny") and world == 8:
        assert all(s[1] < 1.0 for s in shares)


def test_halo_zero_marks_the_tile_and_enable_reads_the_mode():
    """H = 0 marks exactly the panels of the tile's own cells; ``enable_bev_tiling`` takes its default from
    ``modes.tile_halo`` and rejects a negative halo."""
    import bevformer_amd
    from bevformer_amd import ops
    cells = torch.arange(128, 256)
    t = bev_tiling.halo_tables(20, 32, cells, 0)
    assert t[0].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0]
    assert t[1].tolist() == [0, 1, 1, 1, 1, 0, 0, 0, 0, 0]                 # + 33 rows either side
    enc = bevformer_amd.build_transformer_layer_sequence(S.encoder_cfg("micro4")).eval()
    bev_tiling.enable_bev_tiling(enc, simulate=(0, 2))
    assert enc.bev_tiling.halo == ops.modes().tile_halo
    with ops.using(tile_halo=5):
        bev_tiling.enable_bev_tiling(enc, simulate=(0, 2))
        assert enc.bev_tiling.halo == 5
    bev_tiling.enable_bev_tiling(enc, simulate=(0, 2), halo=3)
    assert enc.bev_tiling.halo == 3 and enc.bev_tiling.stats == {"frames": 0, "halo_misses": 0}
    with pytest.raises(ValueError):
        bev_tiling.enable_bev_tiling(enc, simulate=(0, 2), halo=-1)
