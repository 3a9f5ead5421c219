"""GPU: ``ops.head_branches`` / ``ops.reg_refine`` (csrc/head_branch.h) against the float64 yardstick (tests/head_yardstick.py).

Bound: error against the float64 yardstick <= 3 x E_parent, E_parent = the error of the switch-off module path
(``BEVFormerHead.predictions``: the branches' Linear layers through the GEMM of the same mode, the reference's statements in
torch) on the same inputs; 3 = the project's standing factor for re-associated fp32 sums."""
import copy
import functools
import types

import pytest
import torch

from bevformer_amd import ops
from bevformer_amd.modules.head import BEVFormerHead

import head_yardstick as Y

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PC = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
SHAPES = [(1, 37, 2, 10, 10), (6, 37, 1, 8, 3), (2, 64, 2, 10, 10), (6, 900, 1, 10, 10)]


@functools.lru_cache(maxsize=None)
def _case(L, nq, bs, code, nc, shared=False):
    g = torch.Generator().manual_seed(11 + L + nq)
    hs = torch.randn(L, nq, bs, 256, generator=g)
    refs = torch.rand(L, bs, nq, 3, generator=g) * 0.9 + 0.05
    refs[0, 0, 0] = 0.0             # the clamps of inverse_sigmoid
    refs[0, 0, 1] = 1.0
    refs[0, 0, 2] = 1e-6
    cls, reg = Y.make_branches(L, code, nc, shared, seed=3)
    want = Y.head_outputs(hs.double(), refs.double(), [Y.branch_params(b) for b in cls], [Y.branch_params(b) for b in reg], PC)
    return hs, refs, cls, reg, want


def _parent(hs, refs, cls, reg, pc=PC):
    stub = types.SimpleNamespace(cls_branches=cls, reg_branches=reg, pc_range=pc)
    L = hs.shape[0]
    inter = torch.cat([refs[1:], refs[-1:]], 0)      # predictions() reads init_reference and inter_references[:L - 1]
    with torch.no_grad(), ops.using(head_fused=False):
        return BEVFormerHead.predictions(stub, hs, refs[0], inter)


def _err(got, want):
    return (got.detach().double().cpu() - want).abs().max().item()


# (every shape in both GEMM modes; the base-size case once)
CASES = [(s, m) for s in SHAPES for m in ("split", "bf16") if not (s[1] == 900 and m == "bf16")]


@pytest.mark.parametrize("shape,mode", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_head_branches_within_three_times_the_parent_error(shape, mode):
    hs, refs, cls, reg, want = _case(*shape)
    cls, reg = copy.deepcopy(cls).to(DEV), copy.deepcopy(reg).to(DEV)
    hd, rd = hs.to(DEV), refs.to(DEV)
    with torch.no_grad(), ops.using(gemm=mode):
        parent = _parent(hd, rd, cls, reg)
        got = ops.head_branches(hd, rd, cls, reg, PC)
        again = ops.head_branches(hd, rd, cls, reg, PC)
    assert got is not None
    L, nq, bs, code, nc = shape
    assert tuple(got[0].shape) == (L, bs, nq, nc) and tuple(got[1].shape) == (L, bs, nq, code)
    for name, i in (("cls", 0), ("box", 1)):
        e_parent, e_fused = _err(parent[i], want[i]), _err(got[i], want[i])
        print(f"\nhead_branches {shape} {mode} {name}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  (bound {3 * e_parent:.3e})")
        assert e_fused <= 3 * e_parent, f"{name}: fused error {e_fused:.3e} > 3 x E_parent = {3 * e_parent:.3e}"
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), "two runs are not bit-equal"


def test_shared_and_cloned_branches_give_equal_results():
    hs, refs, cls, reg, _ = _case(2, 37, 2, 10, 10, True)
    assert cls[0] is cls[1]
    cls, reg = copy.deepcopy(cls).to(DEV), copy.deepcopy(reg).to(DEV)
    assert cls[0] is cls[1] and reg[0] is reg[1]
    cls_c = torch.nn.ModuleList([copy.deepcopy(cls[0]) for _ in range(2)])
    reg_c = torch.nn.ModuleList([copy.deepcopy(reg[0]) for _ in range(2)])
    with torch.no_grad():
        a = ops.head_branches(hs.to(DEV), refs.to(DEV), cls, reg, PC)
        b = ops.head_branches(hs.to(DEV), refs.to(DEV), cls_c, reg_c, PC)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_refine_is_bit_equal_to_the_head_modes_sigmoid_columns(mode):
    hs, refs, cls, reg, _ = _case(6, 37, 1, 8, 3)
    cls, reg = copy.deepcopy(cls).to(DEV), copy.deepcopy(reg).to(DEV)
    hd, rd = hs.to(DEV), refs.to(DEV)
    with torch.no_grad(), ops.using(gemm=mode):
        _, box = ops.head_branches(hd, rd, cls, reg, (0, 0, 0, 1, 1, 1))
        for l in (0, 3, 5):
            new_ref = ops.reg_refine(hd[l], rd[l], reg[l])
            assert new_ref is not None and tuple(new_ref.shape) == (1, 37, 3)
            assert torch.equal(new_ref, box[l][..., [0, 1, 4]])


@pytest.mark.parametrize("case", ["double", "cpu", "requires_grad", "native"])
def test_uncovered_calls_return_none(case):
    hs, refs, cls, reg, _ = _case(1, 37, 2, 10, 10)
    cls, reg = copy.deepcopy(cls).to(DEV), copy.deepcopy(reg).to(DEV)
    hd, rd, mode, grad = hs.to(DEV), refs.to(DEV), "split", False
    if case == "double":
        hd, rd, cls, reg = hd.double(), rd.double(), cls.double(), reg.double()
    elif case == "cpu":
        hd, rd, cls, reg = hs, refs, cls.cpu(), reg.cpu()
    elif case == "requires_grad":
        hd, grad = hd.clone().requires_grad_(True), True
    else:
        mode = "native"
    with torch.set_grad_enabled(grad), ops.using(gemm=mode):
        assert ops.head_branches(hd, rd, cls, reg, PC) is None
        assert ops.reg_refine(hd[0], rd[0], reg[0]) is None
