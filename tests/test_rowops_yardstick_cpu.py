"""CPU: the float64 yardsticks of tests/rowops_yardstick.py against torch's own float64 evaluation, and every premise the
exact GPU cases (tests/test_mha_exact_gpu.py, tests/test_rowops_exact_gpu.py) rest on, asserted for the shipped inputs by the
reference alone: selection gaps, lattice sums below 2^24, E32 > 0 wherever a bound is a multiple of it, and the one-pass
variance counterexample."""
import pytest
import torch
import torch.nn.functional as F

import rowops_yardstick as Y


# ---------------------------------------------------------------------------------------------------------------------
# yardsticks against torch float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(1, 256), (5, 512), (37, 1024)])
def test_forward_yardstick_is_torch_float64_layer_norm(rows, C):
    g = torch.Generator().manual_seed(rows)
    z = torch.randn(rows, C, generator=g) * 3 + 10
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    want = F.layer_norm(z.double(), (C,), gamma.double(), beta.double(), 1e-5)
    torch.testing.assert_close(Y.ln_forward64(z, gamma, beta, 1e-5), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("rows,C", [(1, 256), (5, 512), (300, 256)])
def test_backward_yardstick_is_torch_float64_autograd(rows, C):
    gen, x, res, gamma, beta = Y.bwd_operands(rows, C)
    g = torch.randn(rows, C, generator=gen)
    gx, gr, dg, db = Y.ln_autograd(x, res, gamma, beta, g, Y.BWD_EPS, torch.float64)
    assert gx is gr or torch.equal(gx, gr)
    got = Y.ln_backward64(x + res, gamma, g, Y.BWD_EPS)
    for a, b in zip(got[:3], (gx, dg, db)):
        torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-11)


def test_attention_yardstick_is_softmax_of_the_scores():
    q, k, v, want, e32 = Y.wide_case(33, 257, 3, 8.0)
    p = Y.scores64(q, k).softmax(-1)
    out = (p @ Y.heads(v, torch.float64)).permute(2, 0, 1, 3).reshape(q.shape)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# ops.mha: premises
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Y.WINNER_MAPS)
def test_selection_gaps(kind):
    """Every shipped case: the winner is ``w``, it leads every other key by >= 128 in the logit (exp(-104) is already 0 in
    float32), every logit is an exact multiple of the scale and reaches the range where exp overflows without a max."""
    for nq, nk, bs in Y.MHA_SHAPES:
        q, k, v, w, want = Y.selection_case(kind, nq, nk, bs)
        s = Y.scores64(q, k)                                                  # (bs, H, nq, nk)
        assert torch.equal(s.argmax(-1), w.permute(1, 2, 0)), (nq, nk, bs)
        raw = s / Y.MHA_SCALE
        assert torch.equal(raw, raw.round()) and torch.equal(raw.float().double(), raw)
        if nk > 1:
            top = s.topk(2, -1).values
            assert (top[..., 0] - top[..., 1]).min().item() >= 128.0, (nq, nk, bs)
        assert s.max().item() > 900.0                                       # exp(905) overflows float32 without a max
        assert 0 <= int(w.min()) and int(w.max()) < nk
        if kind == "tail" and nk >= 32:
            assert (w >= (nk - 1) // 32 * 32).any()                           # winners inside the last (partial) key block
            if nq >= 31:                                                      # ... and on both lane halves (tile rows 4..7 mod 8)
                assert ((w % 32) % 8 >= 4).any() and ((w % 32) % 8 < 4).any()
        heads_differ = (w[:, :, 0] != w[:, :, 1]).any() if nk > 1 else True
        assert heads_differ and (bs == 1 or nk == 1 or (w[:, 0] != w[:, 1]).any())


@pytest.mark.parametrize("nq,nk,bs", [(33, 1, 1), (33, 33, 1), (33, 257, 3), (40, 513, 2)])
@pytest.mark.parametrize("kind", Y.WINNER_MAPS)
def test_selection_is_exact_for_torch_softmax_in_both_precisions(kind, nq, nk, bs):
    q, k, v, w, want = Y.selection_case(kind, nq, nk, bs)
    assert torch.equal(Y.sdpa(q, k, v, torch.float32), want)
    assert torch.equal(Y.sdpa(q, k, v, torch.float64).float(), want)


def test_uniform_cases_are_exact():
    for nq, nk, bs in Y.MHA_SHAPES:
        q, k, v, want = Y.uniform_case(nq, nk, bs)
        assert torch.equal(k, k[:1].expand_as(k))
        assert torch.equal(v, v.round()) and v.abs().max().item() <= 4 and v.abs().sum(0).max().item() < 2 ** 24
        if nk & (nk - 1) == 0:
            assert torch.equal(want.float().double(), want)               # the quotient itself is a float32


def test_wide_logit_yardsticks_are_not_vacuous():
    for nq, nk, bs in Y.MHA_WIDE:
        for gain in Y.MHA_GAINS:
            q, k, v, want, e32 = Y.wide_case(nq, nk, bs, gain)
            std = Y.scores64(q, k).std().item()
            print(f"\nwide nq={nq} nk={nk} bs={bs} gain={gain:g}: logit std {std:.2f}, E32 {e32:.3e}")
            assert e32 > 0 and 0.8 * gain < std < 1.25 * gain


# ---------------------------------------------------------------------------------------------------------------------
# add_layernorm forward: premises
# ---------------------------------------------------------------------------------------------------------------------
def _forward_cases():
    for family in Y.LN_FAMILIES:
        for C in Y.LN_WIDTHS:
            for rows in Y.LN_ROWS:
                for with_res in (False, True):
                    case = Y.ln_forward_case(family, rows, C, with_res)
                    if case is not None:
                        yield family, rows, C, with_res, case


def test_forward_yardsticks_are_not_vacuous():
    n = 0
    for family, rows, C, with_res, c in _forward_cases():
        assert c["e32"] > 0, (family, rows, C, with_res)
        assert torch.isfinite(c["want"]).all()
        n += 1
    assert n == (4 * 2 + 1) * len(Y.LN_WIDTHS) * len(Y.LN_ROWS)


def test_one_pass_variance_breaks_the_bound_on_the_offset_rows():
    """The inputs discriminate: E[z^2] - mean^2 in float32 misses the bound, FACTOR x max(E32, E_mean), on EVERY offset
    case (by 6 x the bound where it comes closest; it misses FACTOR x E32 alone all the more)."""
    for family, rows, C, with_res, c in _forward_cases():
        if not family.startswith("offset"):
            continue
        err = (Y.ln_one_pass32(c["z"], c["gamma"], c["beta"], c["eps"]).double() - c["want"]).abs().max().item()
        assert err > Y.FACTOR * c["yard"] >= Y.FACTOR * c["e32"], (family, rows, C, with_res, err, c["yard"])


def test_the_mean_rounding_term_of_the_forward_bound():
    """E_mean (``Y.ln_e_mean``): 2^-24 |mean| gamma / sqrt(var + eps) by the float64 statement alone.  Centred rows: below E32, the
    bound there is FACTOR x E32.  Offset rows: E32 — torch's own luck with each row's mean — lies below it or near it, and
    torch's evaluation with ONLY its mean replaced by the float32 next to it already costs more than E32."""
    for family, rows, C, with_res, c in _forward_cases():
        assert c["yard"] == max(c["e32"], c["e_mean"])
        if family in ("cancelling", "eps_zero"):
            assert c["e_mean"] < c["e32"] and c["yard"] == c["e32"], (family, rows, C, with_res)
    c = Y.ln_forward_case("offset_1", 1, 512, True)
    z = c["z"].double()
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + c["eps"])
    m32 = mean.float()
    assert ((m32.double() - mean).abs() < 0.1 * Y.ulp32(mean)).all()                       # torch's luck with this row: 0.09 ulp
    nxt = torch.nextafter(m32, torch.where(m32.double() < mean, m32 + 1, m32 - 1)).double()  # the float32 on the other side
    err = ((z - nxt) * rstd * c["gamma"].double() + c["beta"].double() - c["want"]).abs().max().item()
    assert Y.FACTOR * c["e32"] < err <= Y.FACTOR * c["yard"]


def test_tiny_variance_rows_sit_below_eps():
    for rows in Y.LN_ROWS:
        c = Y.ln_forward_case("tiny_variance", rows, 256, False)
        var = c["z"].double().var(-1, unbiased=False)
        assert (var < 0.01 * c["eps"]).all() and (var > 0).all()
    assert Y.ln_forward_case("eps_zero", 3, 256, False)["eps"] == 0.0


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("C", Y.LN_WIDTHS)
def test_constant_rows_are_exact(C, with_res):
    x, res, gamma, beta = Y.ln_constant_case(C, with_res)
    z = Y.add32(x, res)
    want = torch.tensor(Y.LN_CONSTANTS, dtype=torch.float64)
    assert torch.equal(z.double(), want[:, None].expand(-1, C))
    assert torch.equal((want * C).float().double(), want * C)                  # the row sum is a float32 in any order
    assert torch.equal(Y.ln_forward64(z, gamma, beta, 1e-5), beta.double()[None].expand(len(want), C))


# ---------------------------------------------------------------------------------------------------------------------
# add_layernorm backward: premises
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", Y.BWD_WIDTHS)
@pytest.mark.parametrize("rows", Y.BWD_ROWS)
def test_backward_yardsticks_are_not_vacuous(rows, C):
    """E32 > 0 per output — but for grad beta of ONE row, which is g itself in any precision: the GPU test asks equality there."""
    for kind in ("randn", "two") if rows in (5, 8197) else ("randn",):
        e = Y.bwd_case(rows, C, kind)["e32"]
        print(f"\nbackward rows={rows} C={C} {kind}: E32 gx {e['gx']:.3e} dgamma {e['dgamma']:.3e} dbeta {e['dbeta']:.3e}")
        assert e["gx"] > 0 and e["dgamma"] > 0
        assert e["dbeta"] > 0 if rows > 1 else e["dbeta"] == 0


@pytest.mark.parametrize("C", Y.BWD_WIDTHS)
def test_backward_lattice_sums_stay_below_2_24(C):
    for rows in Y.BWD_ROWS:
        x, res, gamma, g, want = Y.bwd_lattice_case(rows, C)
        assert torch.equal(g, g.round()) and g.abs().max().item() <= 2
        assert g.abs().sum(0).max().item() < 2 ** 24
        assert torch.equal(want.float().double(), want)
        assert rows < 100 or (want != 0).any()


@pytest.mark.parametrize("C", Y.BWD_WIDTHS)
def test_backward_live_row_yardsticks(C):
    assert Y.live_rows() == (0, 8196, 8191, 8192)
    for r in Y.live_rows():
        c = Y.bwd_live_row_case(C, r)
        assert c["e32"]["gx"] > 0 and c["e32"]["dgamma"] > 0
        live = torch.zeros(Y.BWD_LIVE_ROWS, dtype=torch.bool)
        live[r] = True
        assert (c["want"][0][~live] == 0).all() and (c["want"][0][r] != 0).any()
        assert torch.equal(c["want"][2], c["g"][r].double())
        torch.testing.assert_close(c["want"][1], c["g"][r].double() * c["xhat_r"], rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# gather_mean, cast_rows_bf16: premises
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,J,R,C", Y.GATHER_SHAPES)
def test_gather_cases(Q, J, R, C):
    for seed in (0, 1):
        idx = Y.gather_index(Q, J, R, seed)
        assert idx.dtype == torch.int32 and int(idx.min()) >= -1 and int(idx.max()) < R
        if Q >= 2:
            assert (idx[-1] == -1).all()
        if J >= 3:
            assert idx[0, 0] >= 0 and idx[0, 1] == -1 and idx[0, 2] >= 0
        if J >= 2 and Q >= 2:
            assert idx[1, 0] == idx[1, 1] >= 0
    if Q == 65:
        assert (Q * C // 4) % 256 != 0                                             # a partial last workgroup
    rows, idx, scale = Y.gather_case(Q, J, R, C, exact=True)
    want = Y.gather_mean32(rows.double(), idx, scale.double())
    assert torch.equal(Y.gather_mean32(rows, idx, scale).double(), want)           # exact: float32 == float64
    assert torch.equal(torch.log2(scale), torch.log2(scale).round())
    rows, idx, scale = Y.gather_case(Q, J, R, C, exact=False)
    torch.testing.assert_close(Y.gather_mean32(rows, idx, scale).double(), Y.gather_mean32(rows.double(), idx, scale.double()),
                               rtol=1e-6, atol=1e-6)


def _bf16_bits(pattern):
    t = torch.tensor([pattern if pattern < 1 << 31 else pattern - (1 << 32)], dtype=torch.int32).view(torch.float32)
    return int(t.to(torch.bfloat16).view(torch.int16)) & 0xFFFF


def test_cast_patterns_and_the_reference_rounding():
    """torch's float32 -> bfloat16 on the CPU rounds to nearest even: pinned on the chosen patterns by hand."""
    assert _bf16_bits(0x3F808000) == 0x3F80 and _bf16_bits(0x3F818000) == 0x3F82          # ties, down and up to even
    assert _bf16_bits(0x3F807FFF) == 0x3F80 and _bf16_bits(0x3F808001) == 0x3F81          # just below / above a tie
    assert _bf16_bits(0x3F7FFFFF) == 0x3F80                                               # carry into the exponent
    assert _bf16_bits(0x7F7FFFFF) == 0x7F80 and _bf16_bits(0xFF7FFFFF) == 0xFF80          # largest finite -> inf
    assert _bf16_bits(0x00000000) == 0x0000 and _bf16_bits(0x80000000) == 0x8000
    assert _bf16_bits(0x007FFFFF) == 0x0080 and _bf16_bits(0x00008000) == 0x0000 and _bf16_bits(0x00018000) == 0x0002
    for R, C in [(33, 8), (33, 264)]:
        a, nan = Y.cast_case(R, C)
        bits = a.view(torch.int32).flatten()
        for p in Y.BF16_PATTERNS + Y.BF16_NANS:
            assert (bits == (p if p < 1 << 31 else p - (1 << 32))).sum().item() >= 2, hex(p)
        assert nan.sum().item() >= 2 * len(Y.BF16_NANS) and torch.equal(nan, torch.isnan(a))
        for scale in (1.0, 0.5):
            assert torch.equal(torch.isnan(a * scale), nan)
        assert Y.rows_written(None, R) == R and Y.rows_written(R + 5, R) == R and Y.rows_written(-3, R) == 0
