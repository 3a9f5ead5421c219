"""No GPU: ``bevmsda_match_cost_grouped_f32`` and ``bevmsda_det_loss_grouped_f32`` validate every argument before any launch,
in the order of the existing descriptor calls, and answer a bad call with a code of ``bevmsda_error_string``'s table
(include/bevmsda.h).  Pointers are fake: no kernel runs.  The two entry points were ADDED to ABI version 7; the number did
not move."""
import ctypes
import re

import pytest

from bevformer_amd import _lib, build

OK, NULLP, SHAPE, LARGE, MISAL = 0, -1, -2, -3, -4
fake = ctypes.c_void_p(0x1000)
odd = ctypes.c_void_p(0x1002)


@pytest.fixture(scope="module")
def lib():
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _desc(**kw):
    base = dict(L=2, bs=2, groups=3, nq=37, cls_out=10, code_size=10, gmax=8, cost_cls_weight=2.0, cost_reg_weight=0.25,
                cost_alpha=0.25, cost_gamma=2.0, cost_eps=1e-12, loss_alpha=0.25, loss_gamma=2.0, loss_cls_weight=2.0,
                loss_box_weight=0.25)
    base.update(kw)
    return ctypes.byref(_lib.GroupLossDesc(**base))


# a bad shape is named before a size, a size before an empty problem, an empty problem before the pointers
BAD_DESCS = [(dict(L=-1), SHAPE), (dict(bs=-1), SHAPE), (dict(nq=-1), SHAPE), (dict(gmax=-1), SHAPE), (dict(groups=0), SHAPE),
             (dict(groups=-2), SHAPE), (dict(code_size=7), SHAPE), (dict(code_size=9), SHAPE), (dict(cls_out=0), SHAPE),
             (dict(cls_out=33), SHAPE), (dict(nq=2049), LARGE), (dict(gmax=513), LARGE), (dict(L=300, bs=300, groups=1), LARGE),
             (dict(L=6, bs=993, groups=11), LARGE),             # 65,538 problems: one past the grid limit of 65,535
             (dict(groups=0, nq=2049), SHAPE), (dict(nq=2049, L=0), LARGE)]


def test_the_symbols_are_bound_and_the_version_did_not_move():
    assert _lib.ABI_VERSION == 7
    header = open(build.PUBLIC_HEADER).read()
    assert re.search(r"#define BEVMSDA_ABI_VERSION 7\b", header)
    for name in ("bevmsda_match_cost_grouped_f32", "bevmsda_det_loss_grouped_f32"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header)
    assert re.search(r"typedef struct bevmsda_group_loss_desc \{\s*int32_t L, bs, groups, nq, cls_out, code_size, gmax;", header)
    d = _lib.GroupLossDesc
    assert d.cost_cls_weight.offset == 32 and ctypes.sizeof(d) == 32 + 9 * 8 + 16      # seven int32 and a pad, nine doubles


def test_match_cost_grouped_rejects_bad_arguments(lib):
    f = lib.bevmsda_match_cost_grouped_f32
    names = ("cls", "box", "gt", "label", "count", "cost")

    def call(d, **kw):
        a = {n: fake for n in names}
        a.update(kw)
        return f(a["cls"], a["box"], a["gt"], a["label"], a["count"], d, a["cost"], None)
    assert f(fake, fake, fake, fake, fake, None, fake, None) == NULLP
    for kw, code in BAD_DESCS:
        assert call(_desc(**kw)) == code, kw
    assert call(_desc(L=6, bs=993, groups=11), cls=None) == LARGE            # (before the pointers are looked at)
    for kw in (dict(L=0), dict(bs=0), dict(nq=0), dict(gmax=0)):
        assert call(_desc(**kw)) == OK, kw                          # empty: a no-op
        assert call(_desc(**kw), cls=None, cost=None) == OK, kw
    for n in names:
        assert call(_desc(), **{n: None}) == NULLP, n
        assert call(_desc(), **{n: odd}) == MISAL, n


def test_det_loss_grouped_rejects_bad_arguments(lib):
    f = lib.bevmsda_det_loss_grouped_f32
    names = ("cls", "box", "gt", "label", "count", "assigned", "code_weights", "factors", "group_losses", "losses", "grad_cls",
             "grad_box")

    def call(d, **kw):
        a = {n: fake for n in names}
        a.update(kw)
        return f(a["cls"], a["box"], a["gt"], a["label"], a["count"], a["assigned"], a["code_weights"], a["factors"], d,
                 a["group_losses"], a["losses"], a["grad_cls"], a["grad_box"], None)
    assert f(*([fake] * 8), None, fake, fake, fake, fake, None) == NULLP
    for kw, code in BAD_DESCS:
        assert call(_desc(**kw)) == code, kw
    for kw in (dict(L=0), dict(bs=0), dict(nq=0)):
        assert call(_desc(**kw)) == OK, kw
        assert call(_desc(**kw), cls=None, losses=None) == OK, kw
    for n in names:
        assert call(_desc(), **{n: None}) == NULLP, n
        assert call(_desc(), **{n: odd}) == MISAL, n
    # without gt rows the packed boxes and labels are not read
    assert call(_desc(gmax=0), factors=None) == NULLP
