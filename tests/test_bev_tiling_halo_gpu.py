"""BEV tiling with a halo on the GPU: the row-panel projection over a needed-panel table
(``bevmsda_linear_panel_rows2_masked_f32``), the out-of-band flag of TemporalSelfAttention's sampling kernel
(``bevmsda_fused_forward_halo_f32``) and the schedule's fallback (bev_tiling.tiled_forward)."""
import functools

import pytest
import torch

from bevformer_amd import bev_tiling, ops
from bevformer_amd import synthetic as S
from bevformer_amd.ops import gemm as G

from helpers import build_pair, oracle_encoder_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAME, WORLD, RANK = "base", 8, 3
# The halo of these tests, in cells.  Reasoned, not fitted: the stock TemporalSelfAttention bias puts point p of head h at
# (p + 1) cells along the head's direction, at most 4 cells per axis; the trained-like offset weights (N(0, 0.01) over 512 inputs
# of unit scale) add a fraction of a cell; the frame's ego-motion shift is 2.5 m / 0.512 m = 4.9 cells; a bilinear footprint
# adds one more.  That is below 12 cells; 16 leaves a margin, and the CPU oracle measures the real figure before any GPU run.
HALO = 16
BIAS_SCALE = 16.0   # the "miss" case: offsets of up to 64 cells


class TapRecorder:
    """``msda=`` stand-in for the oracle (tests/helpers.py): evaluates the operator and, for TemporalSelfAttention's calls
    (2 value entries, one level, row i = grid cell ``cells[i]``), records the live taps — bilinear coefficient and attention
    weight both non-zero, inside the grid — as their largest Chebyshev distance from the query's own cell and as the set of
    grid cells they touch."""

    def __init__(self, cells, bev_h, bev_w):
        self.cells, self.h, self.w = cells, bev_h, bev_w
        self.max_dist = 0
        self.touched = torch.zeros(bev_h * bev_w, dtype=torch.bool)

    def __call__(self, value, shapes, loc, att):
        from oracle import bevformer_cpu as O
        out = O.msda_gridsample(value, shapes, loc, att)
        if value.shape[0] == 2 and shapes.shape[0] == 1 and loc.shape[1] == self.cells.numel():
            H, W = self.h, self.w
            x = loc[..., 0].float() * W - 0.5                       # (2, R, M, 1, P)
            y = loc[..., 1].float() * H - 0.5
            x0, y0 = x.floor(), y.floor()
            fx, fy = x - x0, y - y0
            cy = (self.cells // W).view(1, -1, 1, 1, 1)
            cx = (self.cells % W).view(1, -1, 1, 1, 1)
            for dy, wy in ((0, 1 - fy), (1, fy)):
                for dx, wx in ((0, 1 - fx), (1, fx)):
                    ty, tx = (y0 + dy).long(), (x0 + dx).long()
                    live = (wy * wx * att.float() != 0) & (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
                    if live.any():
                        d = torch.maximum((ty - cy).abs(), (tx - cx).abs())[live]
                        self.max_dist = max(self.max_dist, int(d.max()))
                        self.touched[(ty * W + tx)[live]] = True
        return out


def _rank_cells(layout, rank=RANK, world=WORLD):
    w = S.WORKLOADS[NAME]
    if layout == "rows":
        h0, h1 = bev_tiling.row_blocks(w["bev_h"], world)[rank]
        return torch.arange(h0 * w["bev_w"], h1 * w["bev_w"])
    q0, q1 = bev_tiling.query_blocks(w["bev_h"] * w["bev_w"], world)[rank]
    return bev_tiling.sector_order(w["bev_h"], w["bev_w"], S.PC_RANGE, "cpu")[3][q0:q1]


def _scaled(sd, scale):
    return {k: (v * scale if k.endswith("attentions.0.sampling_offsets.bias") else v.clone()) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _oracle_taps(layout, scale, rank=RANK):
    """The reference arithmetic alone (CPU oracle, the rank's rows through all six layers): (largest distance of a live tap
    from its query's cell, does a live tap touch a panel outside the flag's table)."""
    torch.set_num_threads(16)
    w = S.WORKLOADS[NAME]
    _, sd = build_pair(NAME)
    sd = _scaled(sd, scale)
    q, f, kw = S.make_inputs(NAME, seed=0, temporal=True)
    cells = _rank_cells(layout, rank)
    rec = TapRecorder(cells, w["bev_h"], w["bev_w"])
    with torch.no_grad():
        oracle_encoder_rows(sd, q, f, cells, pc_range=S.PC_RANGE, msda=rec, **kw)
    need = bev_tiling.halo_tables(w["bev_h"], w["bev_w"], cells, HALO)[0].bool()
    outside = bool((~need[rec.touched.nonzero().squeeze(1) // bev_tiling.HALO_PANEL_ROWS]).any())
    return rec.max_dist, outside


def _encoder(scale=1.0):
    enc, sd = build_pair(NAME, device=DEV)
    if scale != 1.0:
        enc.load_state_dict(_scaled(sd, scale))
    return enc


@pytest.fixture
def poison():
    """Unwritten rows of a partial projection hold NaN (ops/gemm.py test hook): a read of one shows in the output."""
    G._SEGMENT_POISON["on"], G._SEGMENT_POISON["launches"] = True, 0
    yield G._SEGMENT_POISON
    G._SEGMENT_POISON["on"] = False


# ------------------------------------------------------------------------------------------------ 1. the projection alone
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_masked_projection_equals_the_unmasked_rows_and_leaves_the_rest(out_dtype):
    """Base TSA shapes (2 x 40,000 rows, K = 256, 6 x 256 grouped columns: the role-split shape) over a random table of
    64-row panels, the output pre-filled with a sentinel: needed panels of BOTH row blocks are bit-equal to
    ``bevmsda_linear_panel_rows2_f32``, unneeded ones still hold the sentinel; an all-ones table equals the unmasked launch
    everywhere.  Also a shape of the 64-row panel kernel (a rank-sized call) with a table entry of 128 rows, and the 128-row
    panel kernel (``gemm_kernel="panel128"``) over 64-row entries, whose panels span two entries and straddle the split."""
    import ctypes
    from bevformer_amd import _lib
    g = torch.Generator().manual_seed(11)
    import contextlib
    for Q, groups, rows, kern, bm in ((40000, 6, 64, None, 64), (5000, 6, 128, None, 64), (40000, 6, 64, "panel128", 128)):
        forced = ops.using(gemm_kernel=kern) if kern else contextlib.nullcontext()
        N, K = groups * 256, 256
        lo = torch.randn(Q, K, generator=g).to(DEV)
        hi = torch.randn(Q, K, generator=g).to(DEV)
        wgt = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
        bias = torch.randn(N, generator=g).to(DEV)
        with torch.no_grad(), forced:
            want = ops.linear_rows2(lo, hi, wgt, bias, groups=groups, out_dtype=out_dtype)
            assert want is not None and not getattr(want, "_bevmsda_partial", False)
            n = (Q + rows - 1) // rows
            ones = torch.ones(n, dtype=torch.int32, device=DEV)
            full = ops.linear_rows2(lo, hi, wgt, bias, groups=groups, out_dtype=out_dtype, need=(ones, rows))
            assert full._bevmsda_partial and torch.equal(full, want)
            table = (torch.rand(n, generator=g) < 0.4).to(torch.int32)
            table[0], table[-1] = 1, 0
            # the sentinel: the C entry point on a pre-filled output (ops.linear_rows2 allocates its own)
            blob = ops.panel_weight(wgt)
            y = torch.full((groups, 2 * Q, 256), -7.0, dtype=out_dtype, device=DEV)
            desc = _lib.LinearDesc(M=2 * Q, ldx0=K, lda0=0, ldx1=0, lda1=0, ldw=K, ldy=256, N=N, K0=K, K1=0, relu=0,
                                   precision=0 if ops.gemm_mode() == "split" else 1, group_cols=256,
                                   out_bf16=int(out_dtype == torch.bfloat16))
            desc.reserved[2] = 2 if kern == "panel128" else 0          # (the forced 128-row shape; else the library's rule)
            tdev = table.to(DEV)
            rc = _lib.load().bevmsda_linear_panel_rows2_masked_f32(
                lo.data_ptr(), hi.data_ptr(), Q, blob.data_ptr(), bias.data_ptr(), ctypes.byref(desc), tdev.data_ptr(), rows, n,
                y.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
            torch.cuda.synchronize()
        # every row of a needed entry is computed, and so is every row that shares a workgroup's ``bm``-row panel (global rows
        # [bm p, bm p + bm)) with one: at 40,000 rows per block and 64-row entries a panel is exactly one entry; at 5,000 rows
        # the panels of the second block straddle its 128-row entries, and one panel straddles the split
        row_need = table.bool().repeat_interleave(rows)[:Q]
        both = torch.cat([row_need, row_need]).to(DEV)
        assert torch.equal(y[:, both], want[:, both])
        padded = torch.zeros(((2 * Q + bm - 1) // bm) * bm, dtype=torch.bool, device=DEV)
        padded[:2 * Q] = both
        computed = padded.view(-1, bm).any(1).repeat_interleave(bm)[:2 * Q]
        assert torch.equal(y[:, computed], want[:, computed])
        assert (y[:, ~computed] == -7.0).all()
        assert 0 < int((~computed).sum()) < 2 * Q
    # what the masked entry point does not take: the unmasked launch runs and the result is complete
    with torch.no_grad(), ops.using(gemm_kernel="panelr1"):
        full = ops.linear_rows2(lo, hi, wgt, bias, groups=groups, out_dtype=out_dtype, need=(ones, rows))
        assert full is not None and not getattr(full, "_bevmsda_partial", False)


# --------------------------------------------------------------------------------------- 3. clear flag, exact result
@pytest.mark.parametrize("rank", [0, 3, 7])
@pytest.mark.parametrize("layout", ["rows", "sectors"])
def test_halo_frame_equals_the_full_projection_bit_for_bit_with_a_clear_flag(layout, rank, poison):
    """Ranks 0, 3 and 7 (as the existing base-size tiled test) of a simulated 8-GPU job at base size, with history and the frame's non-zero ego-motion shift, the weights of
    the existing base-size tiled test: the rank's rows with ``halo = 16`` are bit-equal to its rows without, the flag is
    clear, no miss is counted — with unwritten rows poisoned with NaN.
    Condition (CPU oracle, before the GPU runs): the largest distance of a live tap from its query's cell, over the six
    layers, is below the halo.  Measured with the oracle: 10 cells (rows, ranks 0 and 7) or 11 cells (rows rank 3; sectors, every rank) — printed by this test.
    The edge ranks are the ones whose zero-coefficient taps leave the grid's row range: rank 0's taps one row above the
    current-BEV entry land in the history entry's last rows, rank 7's one row below the history entry in the current
    entry's first — memory the cyclic margin of the projection's table must have written, or the poison shows."""
    dist, outside = _oracle_taps(layout, 1.0, rank)
    print(f"{layout} rank {rank}: largest live-tap distance from the query's cell (CPU oracle): {dist} cells; halo {HALO}")
    assert dist < HALO and not outside
    enc = _encoder()
    q, f, kw = S.make_inputs(NAME, seed=0, temporal=True, device=DEV)
    assert float(kw["shift"].abs().max()) > 0
    mine = _rank_cells(layout, rank).to(DEV)
    with torch.no_grad():
        bev_tiling.enable_bev_tiling(enc, simulate=(rank, WORLD), layout=layout, halo=0)
        want = enc(q, f, f, **kw)
        plain = poison["launches"]                             # (the camera segments)
        bev_tiling.enable_bev_tiling(enc, simulate=(rank, WORLD), layout=layout, halo=HALO)
        got = enc(q, f, f, **kw)
        stats = dict(enc.bev_tiling.stats)
        missed = bev_tiling.halo_missed(enc)
        bev_tiling.disable_bev_tiling(enc)
    assert poison["launches"] == 2 * plain + 1                 # (the same again + the masked TSA value projection)
    assert torch.isfinite(got[:, mine]).all()
    assert torch.equal(got[:, mine], want[:, mine])
    assert not missed and stats == {"frames": 1, "halo_misses": 0}


# ------------------------------------------------------------------------------------------ 4. set flag, still right
@pytest.mark.parametrize("layout", ["rows", "sectors"])
def test_a_missed_halo_raises_the_flag_and_the_frame_is_recomputed(layout, poison):
    """The same frame with TemporalSelfAttention's ``sampling_offsets.bias`` scaled by 16 (offsets of up to 64 cells): the CPU
    oracle confirms live taps in panels outside the table (up to 70 cells from their query's cell); the flag is set, one miss is counted and the returned grid is
    the halo-off result bit for bit (the second pass runs the full projection)."""
    dist, outside = _oracle_taps(layout, BIAS_SCALE)
    print(f"{layout}, bias x {BIAS_SCALE}: largest live-tap distance (CPU oracle): {dist} cells; halo {HALO}")
    assert dist > HALO and outside
    enc = _encoder(BIAS_SCALE)
    q, f, kw = S.make_inputs(NAME, seed=0, temporal=True, device=DEV)
    with torch.no_grad():
        bev_tiling.enable_bev_tiling(enc, simulate=(RANK, WORLD), layout=layout, halo=0)
        want = enc(q, f, f, **kw)
        bev_tiling.enable_bev_tiling(enc, simulate=(RANK, WORLD), layout=layout, halo=HALO)
        got = enc(q, f, f, **kw)
        stats = dict(enc.bev_tiling.stats)
        missed = bev_tiling.halo_missed(enc)
        bev_tiling.disable_bev_tiling(enc)
    assert missed and stats == {"frames": 1, "halo_misses": 1}
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------- 5. capture
@pytest.mark.parametrize("scale,expect", [(1.0, False), (BIAS_SCALE, True)])
def test_captured_halo_frame_replays_and_reports_its_flag(scale, expect):
    """One tiled frame with the halo captured in a ``torch.cuda.graph``: nothing is read during capture or replay; the replay
    equals the eager frame and ``halo_missed`` is False — with the weights of the miss case it is True (the owner of the
    graph then replays the graph captured without the halo)."""
    layout = "sectors"
    enc = _encoder(scale)
    q, f, kw = S.make_inputs(NAME, seed=0, temporal=True, device=DEV)
    mine = _rank_cells(layout).to(DEV)
    with torch.no_grad():
        bev_tiling.enable_bev_tiling(enc, simulate=(RANK, WORLD), layout=layout, halo=0)
        want = enc(q, f, f, **kw)
        bev_tiling.enable_bev_tiling(enc, simulate=(RANK, WORLD), layout=layout, halo=HALO)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc(q, f, f, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        frames = enc.bev_tiling.stats["frames"]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = enc(q, f, f, **kw)
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        assert enc.bev_tiling.stats["frames"] == frames          # (captured frames read nothing and count nothing)
        assert bev_tiling.halo_missed(enc) is expect
        if not expect:
            assert torch.equal(out[:, mine], want[:, mine])
        bev_tiling.disable_bev_tiling(enc)
