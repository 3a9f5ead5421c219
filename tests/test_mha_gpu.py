"""GPU: ``ops.mha`` (csrc/mha_d32.h, the decoder's self-attention core) against
``torch.nn.functional.scaled_dot_product_attention`` evaluated in float64 on the CPU.

Bound: max abs error <= 4 x E32, E32 = the error of the SAME torch call in float32 on the CPU against float64, computed
here — a yardstick made of the reference alone.  The factor 4 covers the different summation order of an online softmax
over key blocks merged across wavefronts.  Both numbers are printed (``pytest -s``; copied to profiles/r7/decoder_ab.txt)."""
import pytest
import torch
import torch.nn.functional as F

from bevformer_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADS = 8


def _sdpa(q, k, v, dtype):
    """(n, bs, E) operands -> (nq, bs, E), per (batch, head) attention in ``dtype`` on the CPU."""
    def heads(t):
        n, bs, E = t.shape
        return t.to(dtype).view(n, bs, HEADS, E // HEADS).permute(1, 2, 0, 3)
    o = F.scaled_dot_product_attention(heads(q), heads(k), heads(v))
    return o.permute(2, 0, 1, 3).reshape(q.shape)


def _operands(nq, bs, seed, E=256):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(nq, bs, E, generator=g) for _ in range(3)]


def _check(got, q, k, v, what):
    want = _sdpa(q, k, v, torch.float64)
    e32 = (_sdpa(q, k, v, torch.float32).double() - want).abs().max().item()
    err = (got.cpu().double() - want).abs().max().item()
    print(f"\nmha {what}: max abs error {err:.3e}, E32 {e32:.3e}, bound 4 x E32 = {4 * e32:.3e}")
    assert err <= 4 * e32, f"{what}: max abs error {err:.3e} > 4 x E32 = {4 * e32:.3e}"


@pytest.mark.parametrize("nq,bs", [(900, 1), (37, 2), (1, 1), (129, 3), (1024, 1)])
def test_mha_matches_float64_attention(nq, bs):
    q, k, v = _operands(nq, bs, seed=nq + bs)
    got = ops.mha(q.to(DEV), k.to(DEV), v.to(DEV), HEADS)
    assert got is not None and got.shape == (nq, bs, 256) and got.dtype == torch.float32
    _check(got, q, k, v, f"nq={nq} bs={bs}")


def test_mha_reads_column_blocks_of_a_merged_projection_in_place():
    """q and k as the two column blocks of one (nq, bs, 512) tensor, v with a padded row stride: no copies needed, and
    the same bound."""
    nq, bs = 129, 3
    q, k, v = _operands(nq, bs, seed=11)
    qk = torch.cat([q, k], -1).to(DEV)
    vpad = torch.zeros(nq, bs, 320, device=DEV)
    vpad[..., :256] = v.to(DEV)
    qd, kd, vd = qk[..., :256], qk[..., 256:], vpad[..., :256]
    assert not qd.is_contiguous() and not kd.is_contiguous() and not vd.is_contiguous()
    got = ops.mha(qd, kd, vd, HEADS)
    assert got is not None and got.is_contiguous()
    _check(got, q, k, v, "column blocks nq=129 bs=3")
    assert torch.equal(got, ops.mha(qd.contiguous(), kd.contiguous(), vd.contiguous(), HEADS))


def test_mha_keys_and_queries_of_different_counts():
    g = torch.Generator().manual_seed(3)
    q = torch.randn(45, 2, 256, generator=g)
    k, v = torch.randn(301, 2, 256, generator=g), torch.randn(301, 2, 256, generator=g)
    got = ops.mha(q.to(DEV), k.to(DEV), v.to(DEV), HEADS)
    _check(got, q, k, v, "nq=45 nk=301 bs=2")


def test_mha_declines_what_it_does_not_cover():
    q, k, v = (t.to(DEV) for t in _operands(10, 1, seed=0, E=512))
    assert ops.mha(q, k, v, HEADS) is None                      # head width 64
    q, k, v = _operands(10, 1, seed=0)
    assert ops.mha(q, k, v, HEADS) is None                      # CPU tensors
    qd = q.to(DEV).requires_grad_(True)
    assert ops.mha(qd, k.to(DEV), v.to(DEV), HEADS) is None     # a gradient is wanted
    with torch.no_grad():
        assert ops.mha(qd, k.to(DEV), v.to(DEV), HEADS) is not None
    assert ops.mha(q.to(DEV).double(), k.to(DEV).double(), v.to(DEV).double(), HEADS) is None


def test_mha_records_its_tag_with_the_gemm_timer():
    import contextlib
    seen = []

    @contextlib.contextmanager
    def cb(tag, flops, nbytes):
        seen.append((tag, flops, nbytes))
        yield

    q, k, v = (t.to(DEV) for t in _operands(64, 1, seed=1))
    ops.set_gemm_timer(cb)
    try:
        ops.mha(q, k, v, HEADS)
    finally:
        ops.set_gemm_timer(None)
    assert [s[0] for s in seen] == ["dec_mha"]
    assert seen[0][1] == 4.0 * 8 * 64 * 64 * 32
