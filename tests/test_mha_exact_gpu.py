"""GPU: ``ops.mha`` (csrc/mha_d32.h) where its online softmax has to work: one-hot selections with logits up to +-905
(output == a V row, bit for bit), uniform weights over identical keys (masked tail keys weigh nothing), peaked softmaxes at
logit standard deviations 8 and 30 (float64 yardstick), and NaN queries (they poison their own outputs only).  Inputs and
references: tests/rowops_yardstick.py; their premises: tests/test_rowops_yardstick_cpu.py."""
import pytest
import torch

import rowops_yardstick as Y
from bevformer_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _mha(q, k, v, shape):
    """``ops.mha`` on CPU operands; at ``Y.MHA_STRIDED`` q and k are the column blocks of one (nk, bs, 512) tensor and v has
    a padded row stride (read in place)."""
    if shape == Y.MHA_STRIDED:
        nq, nk, bs = shape
        qk = torch.full((nk, bs, 512), 7.0, device=DEV)
        qk[:nq, :, :256] = q.to(DEV)
        qk[..., 256:] = k.to(DEV)
        vpad = torch.full((nk, bs, 320), -7.0, device=DEV)
        vpad[..., :256] = v.to(DEV)
        qd, kd, vd = qk[:nq, :, :256], qk[..., 256:], vpad[..., :256]
        assert not qd.is_contiguous() and not kd.is_contiguous() and not vd.is_contiguous()
    else:
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    out = ops.mha(qd, kd, vd, Y.HEADS)
    assert out is not None and out.shape == q.shape and out.dtype == torch.float32 and out.is_contiguous()
    return out.cpu()


@pytest.mark.parametrize("kind", Y.WINNER_MAPS)
@pytest.mark.parametrize("nq,nk,bs", Y.MHA_SHAPES)
def test_mha_selects_a_value_row_bit_for_bit(nq, nk, bs, kind):
    """p is exactly 1 at the winner and 0 elsewhere in every block and every wavefront: out[i, b, head h] EQUALS
    v[w(i, b, h), b, head h].  Fails on a wrong pairing of a probability register with its V row, a wrong wavefront merge, a
    missing max subtraction (exp(905) = inf), a wrong stride, a head or batch mix-up."""
    q, k, v, w, want = Y.selection_case(kind, nq, nk, bs)
    got = _mha(q, k, v, (nq, nk, bs))
    bad = (got != want).any(-1).nonzero()
    assert torch.equal(got, want), f"{bad.shape[0]} (query, batch) rows differ, first {bad[:4].tolist()}"


@pytest.mark.parametrize("nq,nk,bs", Y.MHA_SHAPES)
def test_mha_uniform_weights_count_every_real_key_once(nq, nk, bs):
    """Identical keys: p = 1 for every real key, l = nk and the unnormalised O are exact integers, the merge factors 1.  One
    division is the only rounding: EQUAL to sum(V) / nk at a power-of-two nk, within 1 float32 ulp of the float64 quotient
    otherwise.  A masked tail key that leaks, or a key counted twice, moves the result by about 1 / nk."""
    q, k, v, want = Y.uniform_case(nq, nk, bs)
    got = _mha(q, k, v, (nq, nk, bs)).double()
    if nk & (nk - 1) == 0:
        assert torch.equal(got, want)
    else:
        over = ((got - want).abs() / Y.ulp32(want)).max().item()
        assert over <= 1.0, f"{over:.3f} ulp from the float64 quotient"


@pytest.mark.parametrize("gain", Y.MHA_GAINS)
@pytest.mark.parametrize("nq,nk,bs", Y.MHA_WIDE)
def test_mha_peaked_softmax_matches_float64_attention(nq, nk, bs, gain):
    """tests/test_mha_gpu.py's check at logit standard deviations 8 and 30: max abs error <= 4 x E32, E32 = torch's float32 SDPA
    on the CPU against float64 on the same inputs.  The factor holds at these scales; measured on an MI355X:
      nq=33 nk=257 bs=3 gain=8:  max abs error 5.573e-06, E32 8.533e-06, ratio 0.65
      nq=33 nk=257 bs=3 gain=30: max abs error 2.072e-05, E32 1.811e-05, ratio 1.14
      nq=37 nk=900 bs=1 gain=8:  max abs error 6.760e-06, E32 6.107e-06, ratio 1.11
      nq=37 nk=900 bs=1 gain=30: max abs error 2.203e-05, E32 1.438e-05, ratio 1.53
    """
    q, k, v, want, e32 = Y.wide_case(nq, nk, bs, gain)
    got = _mha(q, k, v, (nq, nk, bs))
    err = (got.double() - want).abs().max().item()
    print(f"\nmha wide nq={nq} nk={nk} bs={bs} gain={gain:g}: max abs error {err:.3e}, E32 {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= Y.FACTOR * e32, f"max abs error {err:.3e} > 4 x E32 = {Y.FACTOR * e32:.3e}"


@pytest.mark.parametrize("head", [None, 5])
@pytest.mark.parametrize("nq,nk,bs", [(33, 257, 3), (31, 33, 1)])
def test_mha_nan_queries_poison_only_themselves(nq, nk, bs, head):
    """NaN in all of query row r (``head``: only in that head's 32 columns), r = 0 and r = nq - 1 — the row the tail lanes of
    the last query block compute again: exactly those outputs are NaN, every other output is equal to the clean run's."""
    g = torch.Generator().manual_seed(nq + nk)
    q, k, v = torch.randn(nq, bs, 256, generator=g), torch.randn(nk, bs, 256, generator=g), torch.randn(nk, bs, 256, generator=g)
    clean = _mha(q, k, v, (nq, nk, bs))
    assert torch.isfinite(clean).all()
    cols = slice(0, 256) if head is None else slice(32 * head, 32 * head + 32)
    for r in (0, nq - 1):
        qn = q.clone()
        qn[r, :, cols] = float("nan")
        got = _mha(qn, k, v, (nq, nk, bs))
        want_nan = torch.zeros(nq, bs, 256, dtype=torch.bool)
        want_nan[r, :, cols] = True
        assert torch.equal(torch.isnan(got), want_nan), f"row {r}"
        assert torch.equal(got[~want_nan], clean[~want_nan]), f"row {r}"
