"""No GPU: ``bevmsda_head_branches_f32`` and ``bevmsda_nms_free_decode_f32`` validate every argument before any launch and
answer a bad call with a code of ``bevmsda_error_string``'s table (include/bevmsda.h).  Pointers are fake: no kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT = 0, -1, -2, -3, -4, -6
fake = ctypes.c_void_p(0x1000)
odd = ctypes.c_void_p(0x1004)
odd2 = ctypes.c_void_p(0x1002)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _branch(**kw):
    base = {n: 0x1000 for n in ("w1", "w2", "w3", "b1", "b2", "b3", "gamma1", "beta1", "gamma2", "beta2")}
    base.update(kw)
    return (_lib.HeadBranch * 1)(_lib.HeadBranch(eps1=1e-5, eps2=1e-5, **base))


def _hdesc(**kw):
    base = dict(ld_x=256, ld_layer=37 * 2 * 256, mode=0, L=1, nq=37, bs=2, code_size=10, cls_out=10, precision=0, layer_stride=1)
    base.update(kw)
    return ctypes.byref(_lib.HeadDesc(**base))


def test_abi_version_and_signatures():
    assert _lib.ABI_VERSION == 7
    assert "bevmsda_head_branches_f32" in _lib.SIGNATURES and "bevmsda_nms_free_decode_f32" in _lib.SIGNATURES


def test_head_branches_rejects_bad_arguments(lib):
    f = lib.bevmsda_head_branches_f32
    reg, cls = _branch(), _branch()
    call = lambda d, x=fake, ref=fake, r=reg, c=cls, ob=fake, oc=fake: f(x, ref, r, c, d, ob, oc, None)
    assert f(fake, fake, reg, cls, None, fake, fake, None) == NULLP                  # no descriptor
    assert call(_hdesc(mode=2)) == OPT
    assert call(_hdesc(precision=2)) == OPT
    assert call(_hdesc(layer_stride=3)) == OPT
    assert call(_hdesc(nq=-1)) == SHAPE
    assert call(_hdesc(bs=-1)) == SHAPE
    assert call(_hdesc(L=-1)) == SHAPE
    assert call(_hdesc(L=9)) == SHAPE                                                 # over BEVMSDA_HEAD_MAX_LAYERS
    assert call(_hdesc(mode=1, L=2)) == SHAPE                                         # refine: one layer
    assert call(_hdesc(code_size=7)) == SHAPE
    assert call(_hdesc(code_size=9)) == SHAPE
    assert call(_hdesc(cls_out=0)) == SHAPE
    assert call(_hdesc(cls_out=33)) == SHAPE
    assert call(_hdesc(nq=5000, bs=5000)) == LARGE                                    # over 2^24 rows
    assert call(_hdesc(nq=0)) == OK                                                   # empty: no-op
    assert call(_hdesc(L=0)) == OK
    assert call(_hdesc(), x=None) == NULLP
    assert call(_hdesc(), ref=None) == NULLP
    assert call(_hdesc(), r=None) == NULLP
    assert call(_hdesc(), c=None) == NULLP
    assert call(_hdesc(), ob=None) == NULLP
    assert call(_hdesc(), oc=None) == NULLP
    assert call(_hdesc(ld_x=128)) == SHAPE
    assert call(_hdesc(ld_x=258)) == MISAL                                            # rows not on 16 bytes
    assert call(_hdesc(), x=odd) == MISAL
    assert call(_hdesc(), ref=odd2) == MISAL
    assert call(_hdesc(), r=_branch(w2=None)) == NULLP
    assert call(_hdesc(), r=_branch(b3=None)) == NULLP
    assert call(_hdesc(), c=_branch(gamma1=None)) == NULLP
    assert call(_hdesc(), r=_branch(w1=0x1004)) == MISAL
    assert call(_hdesc(), c=_branch(beta2=0x1004)) == MISAL


def _ddesc(**kw):
    base = dict(bs=1, nq=37, num_classes=10, code_size=10, max_num=300, n_ladder=0)
    base.update(kw)
    return ctypes.byref(_lib.DecodeDesc(**base))


def test_nms_free_decode_rejects_bad_arguments(lib):
    f = lib.bevmsda_nms_free_decode_f32
    call = lambda d, cls=fake, box=fake, s=fake, l=fake, b=fake, k=fake, c=fake: f(cls, box, d, s, l, b, k, c, None)
    assert f(fake, fake, None, fake, fake, fake, fake, fake, None) == NULLP
    assert call(_ddesc(nq=-1)) == SHAPE
    assert call(_ddesc(max_num=-1)) == SHAPE
    assert call(_ddesc(n_ladder=-1)) == SHAPE
    assert call(_ddesc(code_size=7)) == SHAPE
    assert call(_ddesc(max_num=371)) == SHAPE                                         # max_num > nq * C
    assert call(_ddesc(nq=2000, max_num=300)) == LARGE                                # 20,000 scores
    assert call(_ddesc(nq=900, max_num=1025)) == LARGE
    assert call(_ddesc(n_ladder=65)) == LARGE
    assert call(_ddesc(bs=70000)) == LARGE
    assert call(_ddesc(bs=0)) == OK
    for name in ("cls", "box", "s", "l", "b", "k", "c"):
        assert call(_ddesc(), **{name: None}) == NULLP, name
    assert call(_ddesc(), cls=odd2) == MISAL
    assert call(_ddesc(), l=odd) == MISAL                                             # int64 labels on 8 bytes
    assert call(_ddesc(), c=odd2) == MISAL


def test_error_strings_cover_the_codes(lib):
    for code in (OK, NULLP, SHAPE, LARGE, MISAL, OPT):
        assert lib.bevmsda_error_string(code)
