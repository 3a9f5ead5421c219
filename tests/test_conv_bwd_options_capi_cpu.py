"""No GPU: the options of ``bevmsda_conv_dgrad_rows_f32`` (``add_mode``, ``add_after_mask``) and ``bevmsda_conv_wgrad_rows_f32``
(``relu_x``, ``dbias``) live in the descriptors' former reserved words; their argument checks answer with a code of
``bevmsda_error_string``'s table where include/bevmsda.h documents them, and a descriptor with every new field zero answers as
before.  Pointers are fake: no kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
# far apart: nothing overlaps by accident
G, YM, X, ADD, NM, DX, DW, WP, DB = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000, 0x900000
fake = ctypes.c_void_p(WP)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _dgrad(**kw):
    base = dict(g=G, ld_g=128, eps=1e-5, next_eps=1e-5, n_img=2, H=6, W=10, c_in=64, c_out=128, taps=1, stride=1, precision=0)
    base.update(kw)
    return ctypes.byref(_lib.ConvDgradRowsDesc(**base))


def _wgrad(**kw):
    base = dict(g=G, ld_g=128, x=X, ld_x=64, eps=1e-5, n_img=2, H=6, W=10, c_in=64, c_out=128, taps=1, stride=1, precision=0)
    base.update(kw)
    return ctypes.byref(_lib.ConvWgradRowsDesc(**base))


def test_the_new_fields_sit_in_the_reserved_words():
    assert _lib.ABI_VERSION == 7
    D, Wg = _lib.ConvDgradRowsDesc, _lib.ConvWgradRowsDesc
    assert ctypes.sizeof(D) == 12 * 8 + 2 * 4 + 8 * 4 + 2 * 4 and ctypes.sizeof(Wg) == 8 * 8 + 4 + 8 * 4 + 3 * 4
    assert D.precision.offset == 132 and D.add_mode.offset == 136 and D.add_after_mask.offset == 140
    assert Wg.precision.offset == 96 and Wg.relu_x.offset == 100 and Wg.dbias.offset == 104
    assert (_lib.CONV_ADD_SAME, _lib.CONV_ADD_POOL2) == (0, 1)


def test_header_documents_the_fields():
    from bevformer_amd import build
    text = open(build.PUBLIC_HEADER).read()
    for word in ("int32_t add_mode;", "int32_t add_after_mask;", "int32_t relu_x;", "float *dbias;", "#define BEVMSDA_CONV_ADD_POOL2 1",
                 "#define BEVMSDA_ABI_VERSION 7"):
        assert word in text, word


def test_dgrad_options_are_checked_in_the_documented_order(lib):
    def call(d, w=fake, dx=DX, ld_dx=64):
        return lib.bevmsda_conv_dgrad_rows_f32(d, w, ctypes.c_void_p(dx) if dx is not None else None, ld_dx, None)
    mask = dict(next_mask=NM, ld_next_mask=64)
    add = dict(add=ADD, ld_add=64)
    # every new field zero: as before
    assert call(_dgrad(g=0)) == NULLP and call(_dgrad(H=-1)) == SHAPE and call(_dgrad(n_img=0, g=0), w=None, dx=None) == OK
    assert call(_dgrad(add=DX, ld_add=128)) == OPT
    # 1. values other than 0 / 1: with the options, before the shape
    for bad in (dict(add_mode=2), dict(add_mode=-1), dict(add_after_mask=2), dict(add_after_mask=-1)):
        assert call(_dgrad(H=-1, **add, **mask, **bad)) == OPT, bad
    # 2. an add option without add
    assert call(_dgrad(H=-1, add_mode=1)) == OPT
    assert call(_dgrad(H=-1, add_after_mask=1, **mask)) == OPT
    # 3. add_after_mask without next_mask
    assert call(_dgrad(H=-1, add_after_mask=1, **add)) == OPT
    # (valid combinations get past the options: the negative size answers)
    assert call(_dgrad(H=-1, add_mode=1, **add)) == SHAPE
    assert call(_dgrad(H=-1, add_mode=1, add_after_mask=1, **add, **mask)) == SHAPE
    # 4. POOL2: the fine map's rows are bounded too.  (g = NULL: a call that passes the bound answers NULL_POINTER, none launches)
    assert call(_dgrad(g=0, n_img=1, H=1 << 11, W=1 << 11, add_mode=1, **add)) == NULLP       # exactly 2^24 fine rows
    assert call(_dgrad(g=0, n_img=1, H=(1 << 11) + 1, W=1 << 11, add_mode=1, **add)) == LARGE
    assert call(_dgrad(g=0, n_img=1, H=(1 << 11) + 1, W=1 << 11, **add)) == NULLP             # (the same rows without POOL2)
    assert call(_dgrad(g=0, n_img=0, H=(1 << 11) + 1, W=1 << 11, add_mode=1, **add)) == OK    # (n_img = 0: empty)
    assert call(_dgrad(g=0, n_img=5000, H=100, W=100, add_mode=1, **add)) == LARGE
    # the later stages are unchanged by the options
    assert call(_dgrad(add_mode=1, c_in=48, **add), ld_dx=48) == UNSUP
    assert call(_dgrad(add_mode=1, g=0, **add)) == NULLP
    assert call(_dgrad(add_mode=1, add=ADD, ld_add=32)) == SHAPE
    assert call(_dgrad(add_mode=1, add=ADD, ld_add=66)) == MISAL
    assert call(_dgrad(add_mode=1, add=ADD + 4, ld_add=64)) == MISAL
    # 5. POOL2: add (4 * 120 fine rows) may not overlap dx (120 rows) at all
    assert call(_dgrad(add_mode=1, add=DX, ld_add=64)) == OPT                                 # add IS dx: not in this mode
    assert call(_dgrad(add_mode=1, add=DX - (479 * 64 + 60) * 4, ld_add=64)) == OPT           # add's last 16 bytes are dx's first
    assert call(_dgrad(add_mode=1, add=DX + (119 * 64 + 60) * 4, ld_add=64)) == OPT           # add starts on dx's last 16 bytes
    # rows 120 .. 479 of the fine map lie beyond the coarse extent: only POOL2 sees the overlap
    assert call(_dgrad(add_mode=1, add=DX - 200 * 64 * 4, ld_add=64)) == OPT


def test_wgrad_options_are_checked_in_the_documented_order(lib):
    def call(d, dw=DW):
        return lib.bevmsda_conv_wgrad_rows_f32(d, ctypes.c_void_p(dw) if dw is not None else None, None)
    # every new field zero: as before
    assert call(_wgrad(g=0)) == NULLP and call(_wgrad(H=-1)) == SHAPE and call(_wgrad(n_img=0, g=0, x=0), dw=None) == OK
    assert call(_wgrad(), dw=G) == OPT
    # 1. relu_x other than 0 / 1: with the options, before the shape
    assert call(_wgrad(H=-1, relu_x=2)) == OPT and call(_wgrad(H=-1, relu_x=-1)) == OPT
    assert call(_wgrad(H=-1, relu_x=1)) == SHAPE
    assert call(_wgrad(n_img=0, relu_x=1, dbias=DB + 2, g=0, x=0), dw=None) == OK             # the empty problem: whatever the pointers
    assert call(_wgrad(relu_x=1, dbias=DB, g=0)) == NULLP
    # 2. dbias off 4 bytes, with dw's alignment: after the strides, before the overlaps
    assert call(_wgrad(dbias=DB + 2)) == MISAL
    assert call(_wgrad(dbias=DB + 2, ld_x=32)) == SHAPE
    assert call(_wgrad(dbias=G + 2), dw=G) == MISAL
    # 3. dbias (128 floats) overlapping g (120 rows of 128), x (120 rows of 64), y or dw (128 x 64)
    assert call(_wgrad(dbias=G)) == OPT
    assert call(_wgrad(dbias=G + (119 * 128 + 127) * 4)) == OPT                               # starts on g's last float
    assert call(_wgrad(dbias=G - 127 * 4)) == OPT                                             # ends on g's first float
    assert call(_wgrad(dbias=X + (119 * 64 + 63) * 4)) == OPT
    assert call(_wgrad(dbias=YM, y=YM, ld_y=128)) == OPT
    assert call(_wgrad(dbias=DW)) == OPT
    assert call(_wgrad(dbias=DW + (128 * 64 - 1) * 4)) == OPT                                 # starts on dw's last float
    assert call(_wgrad(dbias=DW - 127 * 4)) == OPT
