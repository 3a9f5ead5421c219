"""No GPU: ``bevmsda_deform_conv_f32`` validates every argument before any launch and answers a bad call with a code of
``bevmsda_error_string``'s table, in the order include/bevmsda.h documents.  Pointers are fake: no kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
X, OFFS, BIAS, Y, WP, BN = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000    # far apart: nothing overlaps by accident
fake = ctypes.c_void_p(WP)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _desc(bn=None, **kw):
    base = dict(x=X, ld_x=64, offs=OFFS, ld_offs=32, bias=BIAS, eps=1e-5, n_img=2, H=6, W=10, c_in=64, c_out=128, stride=1, relu=0,
                precision=0)
    base.update(kw)
    d = _lib.DeformConvDesc(**base)
    for i, v in enumerate(bn or ()):
        d.bn[i] = v
    return ctypes.byref(d)


def _call(lib, d, w=fake, y=Y, ld_y=128):
    return lib.bevmsda_deform_conv_f32(d, w, ctypes.c_void_p(y) if y is not None else None, ld_y, None)


def test_signature_is_listed_and_the_abi_version_stays():
    assert _lib.ABI_VERSION == 7
    assert "bevmsda_deform_conv_f32" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.DeformConvDesc) == 5 * 8 + 4 * 8 + 4 + 8 * 4 + 3 * 4
    assert _lib.DeformConvDesc.eps.offset == 72 and _lib.DeformConvDesc.n_img.offset == 76


def test_deform_conv_rejects_bad_arguments_in_the_documented_order(lib):
    call = lambda d, **kw: _call(lib, d, **kw)
    bn = [BN, BN + 0x1000, BN + 0x2000, BN + 0x3000]
    assert lib.bevmsda_deform_conv_f32(None, fake, ctypes.c_void_p(Y), 128, None) == NULLP      # no descriptor
    # options come first, whatever else is wrong
    for bad in (dict(stride=0), dict(stride=3), dict(precision=2), dict(precision=-1)):
        assert call(_desc(H=-1, **bad)) == OPT, bad
    assert call(_desc(bn=bn, H=-1)) == OPT                              # bias and BatchNorm both given
    assert call(_desc(bn=bn[:3], bias=0, H=-1)) == OPT                  # some but not all of the four vectors
    for name in ("n_img", "H", "W", "c_in", "c_out"):
        assert call(_desc(**{name: -1})) == SHAPE, name
    assert call(_desc(n_img=5000, H=100, W=100)) == LARGE              # over 2^24 rows
    assert call(_desc(n_img=1, H=1 << 13, W=(1 << 11) + 1)) == LARGE
    assert call(_desc(c_in=65536 + 32, ld_x=65536 + 32)) == LARGE
    assert call(_desc(c_out=65536 + 32), ld_y=65536 + 32) == LARGE
    for name in ("n_img", "H", "W", "c_out"):                          # the empty problem: no-op, whatever the pointers
        assert call(_desc(**{name: 0}), w=None, y=None) == OK, name
    assert call(_desc(c_in=0)) == SHAPE
    assert call(_desc(c_in=48, ld_x=48)) == UNSUP                      # channel counts off the kernel's granularity
    assert call(_desc(c_out=100), ld_y=100) == UNSUP
    assert call(_desc(x=0)) == NULLP
    assert call(_desc(offs=0)) == NULLP
    assert call(_desc(), w=None) == NULLP
    assert call(_desc(), y=None) == NULLP
    assert call(_desc(ld_x=32)) == SHAPE                               # strides below the width
    assert call(_desc(), ld_y=64) == SHAPE
    assert call(_desc(ld_offs=28)) == SHAPE                            # the offset matrix has 32 columns
    assert call(_desc(ld_offs=27)) == SHAPE
    assert call(_desc(ld_x=66, x=X + 4)) == MISAL                      # rows not on 16 bytes come before pointers
    assert call(_desc(), ld_y=130) == MISAL
    assert call(_desc(ld_offs=34)) == MISAL
    assert call(_desc(x=X + 4)) == MISAL                               # pointers off 16 bytes
    assert call(_desc(offs=OFFS + 8)) == MISAL
    assert call(_desc(bias=BIAS + 8)) == MISAL
    assert call(_desc(bias=0, bn=bn[:2] + [bn[2] + 4, bn[3]])) == MISAL
    assert call(_desc(), w=ctypes.c_void_p(WP + 4)) == MISAL
    assert call(_desc(), y=Y + 4) == MISAL
    # y overlapping x or offs: x spans 120 rows of 64 floats, offs 120 rows of 32, y 120 rows of 128
    assert call(_desc(), y=X) == OPT
    assert call(_desc(), y=X + 119 * 64 * 4 + 63 * 4 - 12) == OPT      # y starts on x's last 16 bytes
    assert call(_desc(), y=OFFS) == OPT
    assert call(_desc(), y=OFFS + (119 * 32 + 28) * 4) == OPT
    assert call(_desc(offs=Y + 119 * 128 * 4 + 127 * 4 - 12)) == OPT   # offs starts on y's last 16 bytes
    assert call(_desc(stride=2), y=OFFS + (14 * 32 + 28) * 4) == OPT   # stride 2: 2 * 3 * 5 = 30 output rows
