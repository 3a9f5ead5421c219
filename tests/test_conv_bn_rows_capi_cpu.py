"""No GPU: ``bevmsda_conv_bn_rows_f32`` validates every argument before any launch and answers a bad call with a code of
``bevmsda_error_string``'s table, in the order include/bevmsda.h documents.  Pointers are fake: no kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
X, RES, Y, WP, BN = 0x100000, 0x200000, 0x400000, 0x500000, 0x600000    # far apart: nothing overlaps by accident
BNS = [BN, BN + 0x1000, BN + 0x2000, BN + 0x3000]
fake = ctypes.c_void_p(WP)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _desc(bn=BNS, **kw):
    base = dict(x=X, ld_x=64, res=0, ld_res=0, eps=1e-5, n_img=2, H=6, W=10, c_in=64, c_out=128, taps=1, stride=1, relu=0,
                precision=0)
    base.update(kw)
    d = _lib.ConvBnRowsDesc(**base)
    for i, v in enumerate(bn):
        d.bn[i] = v
    return ctypes.byref(d)


def _call(lib, d, w=fake, y=Y, ld_y=128):
    return lib.bevmsda_conv_bn_rows_f32(d, w, ctypes.c_void_p(y) if y is not None else None, ld_y, None)


def test_signature_is_listed_and_the_abi_version_stays():
    assert _lib.ABI_VERSION == 7
    assert "bevmsda_conv_bn_rows_f32" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.ConvBnRowsDesc) == 4 * 8 + 4 * 8 + 4 + 9 * 4 + 2 * 4
    assert _lib.ConvBnRowsDesc.eps.offset == 64 and _lib.ConvBnRowsDesc.n_img.offset == 68


def test_header_declares_the_entry_point_and_its_descriptor():
    from bevformer_amd import build
    text = open(build.PUBLIC_HEADER).read()
    assert "int bevmsda_conv_bn_rows_f32(const bevmsda_conv_bn_rows_desc *desc, const uint16_t *wpack, float *y, int64_t ld_y, void *stream);" in text
    assert "#define BEVMSDA_ABI_VERSION 7" in text


def test_conv_bn_rows_rejects_bad_arguments_in_the_documented_order(lib):
    call = lambda d, **kw: _call(lib, d, **kw)
    assert lib.bevmsda_conv_bn_rows_f32(None, fake, ctypes.c_void_p(Y), 128, None) == NULLP      # 1. no descriptor
    # 2. options come first, whatever else is wrong
    for bad in (dict(taps=0), dict(taps=3), dict(taps=25), dict(stride=0), dict(stride=3), dict(precision=2), dict(precision=-1)):
        assert call(_desc(H=-1, **bad)) == OPT, bad
    for name in ("n_img", "H", "W", "c_in", "c_out"):                  # 3. a negative size
        assert call(_desc(**{name: -1})) == SHAPE, name
    assert call(_desc(n_img=5000, H=100, W=100)) == LARGE              # 4. over 2^24 input rows
    assert call(_desc(n_img=1, H=1 << 13, W=(1 << 11) + 1)) == LARGE
    assert call(_desc(n_img=5000, H=100, W=100, stride=2)) == LARGE    # (INPUT rows: the stride does not help)
    assert call(_desc(c_in=65536 + 32, ld_x=65536 + 32)) == LARGE
    assert call(_desc(c_out=65536 + 32), ld_y=65536 + 32) == LARGE
    for name in ("n_img", "H", "W", "c_out"):                          # 5. the empty problem: no-op, whatever the pointers
        assert call(_desc(bn=[0, 0, 0, 0], x=0, **{name: 0}), w=None, y=None) == OK, name
    assert call(_desc(c_in=0)) == SHAPE                                # 6.
    assert call(_desc(c_in=48, ld_x=48)) == UNSUP                      # 7. channel counts off the kernel's granularity
    assert call(_desc(c_out=100), ld_y=100) == UNSUP
    assert call(_desc(c_in=48, x=0)) == UNSUP                          # (before the pointers)
    assert call(_desc(x=0)) == NULLP                                   # 8.
    assert call(_desc(), w=None) == NULLP
    assert call(_desc(), y=None) == NULLP
    for i in range(4):
        assert call(_desc(bn=[0 if j == i else v for j, v in enumerate(BNS)])) == NULLP, i
    assert call(_desc(x=0, ld_x=32)) == NULLP                          # (before the strides)
    assert call(_desc(ld_x=32)) == SHAPE                               # 9. strides below the width
    assert call(_desc(), ld_y=64) == SHAPE
    assert call(_desc(res=RES, ld_res=64)) == SHAPE
    assert call(_desc(ld_x=32, x=X + 4)) == SHAPE                      # (before the alignment)
    assert call(_desc(ld_x=66)) == MISAL                               # 10. rows not on 16 bytes
    assert call(_desc(), ld_y=130) == MISAL
    assert call(_desc(res=RES, ld_res=130)) == MISAL
    assert call(_desc(x=X + 4)) == MISAL                               # pointers off 16 bytes
    assert call(_desc(res=RES + 8, ld_res=128)) == MISAL
    for i in range(4):
        assert call(_desc(bn=[v + 4 if j == i else v for j, v in enumerate(BNS)])) == MISAL, i
    assert call(_desc(), w=ctypes.c_void_p(WP + 4)) == MISAL
    assert call(_desc(), y=Y + 4) == MISAL
    assert call(_desc(x=X + 4), y=X) == MISAL                          # (before the overlap)
    # 11. y overlapping x or res: x spans 120 rows of 64 floats, res and y 120 rows of 128
    assert call(_desc(), y=X) == OPT
    assert call(_desc(), y=X + 119 * 64 * 4 + 63 * 4 - 12) == OPT      # y starts on x's last 16 bytes
    assert call(_desc(res=RES, ld_res=128), y=RES) == OPT
    assert call(_desc(res=RES, ld_res=128), y=RES + (119 * 128 + 124) * 4) == OPT
    assert call(_desc(res=Y + (119 * 128 + 124) * 4, ld_res=128)) == OPT       # res starts on y's last 16 bytes
    # stride 2: 2 * 3 * 5 = 30 output rows of res and y, for both tap counts (the 1 x 1 stride-2 form is an option here)
    for taps in (1, 9):
        assert call(_desc(taps=taps, stride=2, res=RES, ld_res=128), y=RES + (29 * 128 + 124) * 4) == OPT, taps
