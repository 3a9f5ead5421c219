"""No GPU: ``bevmsda_conv_rows_f32`` and ``bevmsda_flatten_rows_f32`` validate every argument before any launch and answer a
bad call with a code of ``bevmsda_error_string``'s table, in the order include/bevmsda.h documents.  Pointers are fake: no
kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
X, RES, BIAS, Y, WP = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000     # far apart: nothing overlaps by accident
fake = ctypes.c_void_p(WP)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _desc(**kw):
    base = dict(x=X, ld_x=64, n_img=2, H=6, W=10, c_in=64, c_out=128, taps=9, stride=1, relu_in=0, bias=BIAS, res=RES,
                ld_res=128, res_mode=1, precision=0)
    base.update(kw)
    return ctypes.byref(_lib.ConvRowsDesc(**base))


def _call(lib, d, w=fake, y=Y, ld_y=128):
    return lib.bevmsda_conv_rows_f32(d, w, ctypes.c_void_p(y) if y is not None else None, ld_y, None)


def test_signatures_are_listed_and_the_abi_version_stays():
    assert _lib.ABI_VERSION == 7
    assert "bevmsda_conv_rows_f32" in _lib.SIGNATURES and "bevmsda_flatten_rows_f32" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.ConvRowsDesc) == 5 * 8 + 10 * 4 + 4 * 4


def test_conv_rows_rejects_bad_arguments_in_the_documented_order(lib):
    call = lambda d, **kw: _call(lib, d, **kw)
    assert lib.bevmsda_conv_rows_f32(None, fake, ctypes.c_void_p(Y), 128, None) == NULLP      # no descriptor
    # options come first, whatever else is wrong
    for bad in (dict(taps=3), dict(taps=0), dict(stride=0), dict(stride=3), dict(taps=1, stride=2), dict(res_mode=3),
                dict(res_mode=-1), dict(precision=2), dict(precision=-1)):
        assert call(_desc(H=-1, **bad)) == OPT, bad
    for name in ("n_img", "H", "W", "c_in", "c_out"):
        assert call(_desc(**{name: -1})) == SHAPE, name
    assert call(_desc(n_img=5000, H=100, W=100)) == LARGE              # over 2^24 rows
    assert call(_desc(n_img=1, H=1 << 13, W=(1 << 11) + 1)) == LARGE
    assert call(_desc(c_in=65536 + 32, ld_x=65536 + 32)) == LARGE
    for name in ("n_img", "H", "W", "c_out"):                          # the empty problem: no-op, whatever the pointers
        assert call(_desc(**{name: 0}), w=None, y=None) == OK, name
    assert call(_desc(c_in=0)) == SHAPE
    assert call(_desc(c_in=48, ld_x=48)) == UNSUP                      # channel counts off the kernel's granularity
    assert call(_desc(c_out=100, ld_res=100), ld_y=100) == UNSUP
    assert call(_desc(res_mode=2, H=5, W=10, x=0)) == SHAPE            # upsampled residual onto an odd map, before the pointers
    assert call(_desc(res_mode=2, H=6, W=9, x=0)) == SHAPE
    assert call(_desc(res_mode=2, stride=2, H=6, W=12, x=0)) == SHAPE  # (the OUTPUT map is 3 x 6)
    assert call(_desc(x=0)) == NULLP
    assert call(_desc(), w=None) == NULLP
    assert call(_desc(), y=None) == NULLP
    assert call(_desc(res=0)) == NULLP
    assert call(_desc(res=0, res_mode=0, ld_res=0), y=None) == NULLP   # (res is not looked at without a res_mode: y is what is missing)
    assert call(_desc(ld_x=32)) == SHAPE                               # strides below the width
    assert call(_desc(), ld_y=64) == SHAPE
    assert call(_desc(ld_res=64)) == SHAPE
    assert call(_desc(ld_x=66, x=X + 4)) == MISAL                      # rows not on 16 bytes come before pointers
    assert call(_desc(), ld_y=130) == MISAL
    assert call(_desc(ld_res=130)) == MISAL
    assert call(_desc(x=X + 4)) == MISAL                               # pointers off 16 bytes
    assert call(_desc(res=RES + 4)) == MISAL
    assert call(_desc(bias=BIAS + 8)) == MISAL
    assert call(_desc(), w=ctypes.c_void_p(WP + 4)) == MISAL
    assert call(_desc(), y=Y + 4) == MISAL
    # y overlapping x or res: x spans 2 * 6 * 10 rows of 64 floats, y and res 120 rows of 128 floats
    assert call(_desc(), y=X) == OPT
    assert call(_desc(), y=X + 119 * 64 * 4 + 63 * 4 - 12) == OPT      # y starts on x's last 16 bytes
    assert call(_desc(x=Y + 119 * 128 * 4 + 127 * 4 - 12)) == OPT      # x starts on y's last 16 bytes
    assert call(_desc(), y=RES) == OPT
    assert call(_desc(res_mode=2), y=RES + (30 * 128 - 4) * 4) == OPT  # the coarse map is 2 * 3 * 5 rows
    assert call(_desc(ld_x=128, x=Y + 64 * 4), ld_y=256) == OPT        # interleaved columns of one buffer still overlap


def test_flatten_rows_rejects_bad_arguments(lib):
    f = lib.bevmsda_flatten_rows_f32
    p = lambda v: ctypes.c_void_p(v)
    assert f(p(X), 256, None, None, p(Y), 1, 6, 256, 10, 5, 0, None) == SHAPE          # s0 + hw > S
    assert f(p(X), 256, None, None, p(Y), -1, 6, 256, 10, 10, 0, None) == SHAPE
    assert f(p(X), 256, None, None, p(Y), 1, 6, 0, 10, 10, 0, None) == SHAPE
    assert f(p(X), 256, None, None, p(Y), 1, 6, 6, 10, 10, 0, None) == UNSUP            # C % 4
    for name, args in (("bs", (0, 6, 256, 10)), ("Nc", (1, 0, 256, 10)), ("hw", (1, 6, 256, 0))):
        assert f(None, 256, None, None, None, *args, 10, 0, None) == OK, name            # empty: no-op
    assert f(None, 256, None, None, p(Y), 1, 6, 256, 10, 10, 0, None) == NULLP
    assert f(p(X), 256, None, None, None, 1, 6, 256, 10, 10, 0, None) == NULLP
    assert f(p(X), 128, None, None, p(Y), 1, 6, 256, 10, 10, 0, None) == SHAPE          # row stride below the width
    assert f(p(X), 258, None, None, p(Y), 1, 6, 256, 10, 10, 0, None) == MISAL
    assert f(p(X + 4), 256, None, None, p(Y), 1, 6, 256, 10, 10, 0, None) == MISAL
    assert f(p(X), 256, p(BIAS + 4), None, p(Y), 1, 6, 256, 10, 10, 0, None) == MISAL
    assert f(p(X), 256, None, p(BIAS + 4), p(Y), 1, 6, 256, 10, 10, 0, None) == MISAL
    assert f(p(X), 256, None, None, p(Y + 8), 1, 6, 256, 10, 10, 0, None) == MISAL
