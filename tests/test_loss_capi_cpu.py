"""No GPU: ``bevmsda_match_cost_f32``, ``bevmsda_lsap_f32`` and ``bevmsda_det_loss_f32`` validate every argument before any
launch and answer a bad call with a code of ``bevmsda_error_string``'s table (include/bevmsda.h).  Pointers are fake: no
kernel runs.  The three entry points were ADDED to ABI version 6; the number did not move."""
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
    base = dict(L=2, bs=2, nq=37, cls_out=10, code_size=10, gmax=8, cost_cls_weight=2.0, cost_reg_weight=0.25, cost_alpha=0.25,
                cost_gamma=2.0, cost_eps=1e-12, loss_alpha=0.25, loss_gamma=2.0, loss_cls_weight=2.0, loss_box_weight=0.25)
    base.update(kw)
    return ctypes.byref(_lib.LossDesc(**base))


BAD_DESCS = [(dict(L=-1), SHAPE), (dict(bs=-1), SHAPE), (dict(nq=-1), SHAPE), (dict(gmax=-1), SHAPE), (dict(code_size=7), SHAPE),
             (dict(code_size=9), SHAPE), (dict(cls_out=0), SHAPE), (dict(cls_out=33), SHAPE), (dict(nq=2049), LARGE),
             (dict(gmax=513), LARGE), (dict(L=300, bs=300), LARGE)]


def test_abi_version_and_the_symbols_are_bound():
    assert _lib.ABI_VERSION == 7
    header = open(build.PUBLIC_HEADER).read()
    assert re.search(r"#define BEVMSDA_ABI_VERSION 7\b", header)
    for name in ("bevmsda_match_cost_f32", "bevmsda_lsap_f32", "bevmsda_det_loss_f32"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header)


def test_match_cost_rejects_bad_arguments(lib):
    f = lib.bevmsda_match_cost_f32
    names = ("cls", "box", "gt", "label", "count", "cost")

    def call(d, **kw):
        a = {n: fake for n in names}
        a.update(kw)
        return f(a["cls"], a["box"], a["gt"], a["label"], a["count"], d, a["cost"], None)
    assert f(fake, fake, fake, fake, fake, None, fake, None) == NULLP
    for kw, code in BAD_DESCS:
        assert call(_desc(**kw)) == code, kw
    for kw in (dict(L=0), dict(bs=0), dict(nq=0), dict(gmax=0)):
        assert call(_desc(**kw)) == OK, kw                          # empty: a no-op
        assert call(_desc(**kw), cls=None, cost=None) == OK, kw
    for n in names:
        assert call(_desc(), **{n: None}) == NULLP, n
        assert call(_desc(), **{n: odd}) == MISAL, n


def test_lsap_rejects_bad_arguments(lib):
    f = lib.bevmsda_lsap_f32
    names = ("cost", "count", "match", "assigned", "status")

    def call(P=4, gmax=8, nq=37, **kw):
        a = {n: fake for n in names}
        a.update(kw)
        return f(a["cost"], a["count"], P, gmax, nq, a["match"], a["assigned"], a["status"], None)
    assert call(P=-1) == SHAPE
    assert call(gmax=-1) == SHAPE
    assert call(nq=-1) == SHAPE
    assert call(nq=2049) == LARGE
    assert call(gmax=513) == LARGE
    assert call(P=0) == OK
    assert call(P=0, cost=None, count=None, match=None, assigned=None, status=None) == OK
    for n in names:
        assert call(**{n: None}) == NULLP, n
        assert call(**{n: odd}) == MISAL, n


def test_det_loss_rejects_bad_arguments(lib):
    f = lib.bevmsda_det_loss_f32
    names = ("cls", "box", "gt", "label", "count", "assigned", "code_weights", "factors", "losses", "grad_cls", "grad_box")

    def call(d, **kw):
        a = {n: fake for n in names}
        a.update(kw)
        return f(a["cls"], a["box"], a["gt"], a["label"], a["count"], a["assigned"], a["code_weights"], a["factors"], d,
                 a["losses"], a["grad_cls"], a["grad_box"], None)
    assert f(*([fake] * 8), None, fake, fake, fake, None) == NULLP
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
