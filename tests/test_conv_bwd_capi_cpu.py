"""No GPU: ``bevmsda_conv_dgrad_rows_f32``, ``bevmsda_conv_wgrad_rows_f32``, ``bevmsda_conv_gz_rows_f32`` and the input gradient's
weight-image pair validate every argument before any launch and answer a bad call with a code of ``bevmsda_error_string``'s
table, in the order include/bevmsda.h documents.  Pointers are fake: no kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
# far apart: nothing overlaps by accident
G, YM, X, ADD, NM, DX, DW, WP, V = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000, 0x900000
GA, VA, NGA, NVA = V, V + 0x1000, V + 0x2000, V + 0x3000
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


def test_signatures_are_listed_and_the_abi_version_stays():
    assert _lib.ABI_VERSION == 7
    for name in ("bevmsda_conv_dgrad_rows_f32", "bevmsda_conv_wgrad_rows_f32", "bevmsda_conv_gz_rows_f32",
                 "bevmsda_conv_dgrad_packed_bytes", "bevmsda_conv_dgrad_pack_weight_f32"):
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.ConvDgradRowsDesc) == 12 * 8 + 2 * 4 + 8 * 4 + 2 * 4
    assert _lib.ConvDgradRowsDesc.eps.offset == 96 and _lib.ConvDgradRowsDesc.n_img.offset == 104
    assert ctypes.sizeof(_lib.ConvWgradRowsDesc) == 8 * 8 + 4 + 8 * 4 + 3 * 4
    assert _lib.ConvWgradRowsDesc.eps.offset == 64 and _lib.ConvWgradRowsDesc.n_img.offset == 68


def test_header_declares_the_entry_points():
    from bevformer_amd import build
    text = open(build.PUBLIC_HEADER).read()
    assert "int bevmsda_conv_wgrad_rows_f32(const bevmsda_conv_wgrad_rows_desc *desc, float *dw, void *stream);" in text
    assert "int bevmsda_conv_dgrad_rows_f32(const bevmsda_conv_dgrad_rows_desc *desc, const uint16_t *wpack, float *dx, int64_t ld_dx," in text
    assert "#define BEVMSDA_ABI_VERSION 7" in text


def test_dgrad_weight_image_size_and_pack_checks(lib):
    size = lib.bevmsda_conv_dgrad_packed_bytes
    assert size(128, 64, 1) == 1 * 4 * 2 * 128 * 40 * 2            # rows = c_in padded to 128, K = taps * c_out in chunks of 32
    assert size(64, 160, 9) == 2 * 18 * 2 * 128 * 40 * 2
    assert size(48, 64, 1) == 0 and size(64, 64, 4) == 0 and size(0, 64, 1) == 0
    pack = lib.bevmsda_conv_dgrad_pack_weight_f32
    blob = ctypes.c_void_p(DX)
    assert pack(fake, 64, 64, 4, blob, None) == OPT
    assert pack(fake, -1, 64, 1, blob, None) == SHAPE
    assert pack(None, 0, 64, 1, None, None) == OK
    assert pack(fake, 48, 64, 1, blob, None) == UNSUP and pack(fake, 64, 48, 9, blob, None) == UNSUP
    assert pack(None, 64, 64, 1, blob, None) == NULLP and pack(fake, 64, 64, 1, None, None) == NULLP
    assert pack(ctypes.c_void_p(WP + 2), 64, 64, 1, blob, None) == MISAL
    assert pack(fake, 64, 64, 1, ctypes.c_void_p(DX + 8), None) == MISAL


def test_dgrad_rejects_bad_arguments_in_the_documented_order(lib):
    def call(d, w=fake, dx=DX, ld_dx=64):
        return lib.bevmsda_conv_dgrad_rows_f32(d, w, ctypes.c_void_p(dx) if dx is not None else None, ld_dx, None)
    assert lib.bevmsda_conv_dgrad_rows_f32(None, fake, ctypes.c_void_p(DX), 64, None) == NULLP       # 1. no descriptor
    # 2. options come first, whatever else is wrong
    for bad in (dict(taps=0), dict(taps=3), dict(taps=25), dict(stride=0), dict(stride=3), dict(precision=2), dict(precision=-1),
                dict(gamma=GA), dict(var=VA), dict(next_mask=NM, ld_next_mask=64, next_gamma=NGA),
                dict(next_gamma=NGA, next_var=NVA)):
        assert call(_dgrad(H=-1, **bad)) == OPT, bad
    for name in ("n_img", "H", "W", "c_in", "c_out"):                  # 3. a negative size
        assert call(_dgrad(**{name: -1})) == SHAPE, name
    assert call(_dgrad(n_img=5000, H=100, W=100)) == LARGE             # 4. over 2^24 input rows
    assert call(_dgrad(n_img=5000, H=100, W=100, stride=2)) == LARGE
    assert call(_dgrad(c_in=65536 + 32), ld_dx=65536 + 32) == LARGE
    assert call(_dgrad(c_out=65536 + 32, ld_g=65536 + 32)) == LARGE
    for name in ("n_img", "H", "W", "c_in"):                           # 5. the empty problem: no-op, whatever the pointers
        assert call(_dgrad(g=0, **{name: 0}), w=None, dx=None) == OK, name
    assert call(_dgrad(c_out=0)) == SHAPE                              # 6.
    assert call(_dgrad(c_in=48), ld_dx=48) == UNSUP                    # 7. channel counts off the kernel's granularity
    assert call(_dgrad(c_out=100, ld_g=100)) == UNSUP
    assert call(_dgrad(c_in=48, g=0)) == UNSUP                         # (before the pointers)
    assert call(_dgrad(g=0)) == NULLP                                  # 8.
    assert call(_dgrad(), w=None) == NULLP
    assert call(_dgrad(), dx=None) == NULLP
    assert call(_dgrad(g=0, ld_g=64)) == NULLP                         # (before the strides)
    assert call(_dgrad(ld_g=64)) == SHAPE                              # 9. strides below the width
    assert call(_dgrad(), ld_dx=32) == SHAPE
    assert call(_dgrad(y=YM, ld_y=64)) == SHAPE
    assert call(_dgrad(add=ADD, ld_add=32)) == SHAPE
    assert call(_dgrad(next_mask=NM, ld_next_mask=32)) == SHAPE
    assert call(_dgrad(ld_g=64, g=G + 4)) == SHAPE                     # (before the alignment)
    assert call(_dgrad(ld_g=130)) == MISAL                             # 10. rows not on 16 bytes
    assert call(_dgrad(), ld_dx=66) == MISAL
    assert call(_dgrad(y=YM, ld_y=130)) == MISAL
    assert call(_dgrad(add=ADD, ld_add=66)) == MISAL
    assert call(_dgrad(next_mask=NM, ld_next_mask=66)) == MISAL
    for bad in (dict(g=G + 4), dict(y=YM + 8, ld_y=128), dict(gamma=GA + 4, var=VA), dict(gamma=GA, var=VA + 4),
                dict(add=ADD + 4, ld_add=64), dict(next_mask=NM + 4, ld_next_mask=64),
                dict(next_mask=NM, ld_next_mask=64, next_gamma=NGA + 4, next_var=NVA),
                dict(next_mask=NM, ld_next_mask=64, next_gamma=NGA, next_var=NVA + 8)):
        assert call(_dgrad(**bad)) == MISAL, bad
    assert call(_dgrad(), w=ctypes.c_void_p(WP + 4)) == MISAL
    assert call(_dgrad(), dx=DX + 4) == MISAL
    assert call(_dgrad(g=G + 4), dx=G) == MISAL                        # (before the overlap)
    # 11. dx (120 rows of 64 floats) overlapping g (120 rows of 128), y, next_mask, or add other than exactly
    assert call(_dgrad(), dx=G) == OPT
    assert call(_dgrad(), dx=G + (119 * 128 + 124) * 4) == OPT         # dx starts on g's last 16 bytes
    assert call(_dgrad(y=DX + (119 * 64 + 60) * 4, ld_y=128)) == OPT   # y starts on dx's last 16 bytes
    assert call(_dgrad(next_mask=DX, ld_next_mask=64)) == OPT
    assert call(_dgrad(add=DX + 64 * 4, ld_add=64)) == OPT             # add one row into dx
    assert call(_dgrad(add=DX, ld_add=128)) == OPT                     # add at dx with another stride
    # stride 2: g has 2 * 3 * 5 = 30 rows
    for taps in (1, 9):
        assert call(_dgrad(taps=taps, stride=2), dx=G + (29 * 128 + 124) * 4) == OPT, taps


def test_wgrad_rejects_bad_arguments_in_the_documented_order(lib):
    def call(d, dw=DW):
        return lib.bevmsda_conv_wgrad_rows_f32(d, ctypes.c_void_p(dw) if dw is not None else None, None)
    assert lib.bevmsda_conv_wgrad_rows_f32(None, ctypes.c_void_p(DW), None) == NULLP
    for bad in (dict(taps=0), dict(taps=4), dict(stride=0), dict(stride=4), dict(precision=2), dict(gamma=GA), dict(var=VA)):
        assert call(_wgrad(H=-1, **bad)) == OPT, bad
    for name in ("n_img", "H", "W", "c_in", "c_out"):
        assert call(_wgrad(**{name: -1})) == SHAPE, name
    assert call(_wgrad(n_img=5000, H=100, W=100)) == LARGE
    assert call(_wgrad(n_img=1, H=1 << 13, W=(1 << 11) + 1, stride=2)) == LARGE
    assert call(_wgrad(c_in=65536 + 32, ld_x=65536 + 32)) == LARGE
    for name in ("n_img", "H", "W", "c_in", "c_out"):                  # the empty problem: nothing to add
        assert call(_wgrad(g=0, x=0, **{name: 0}), dw=None) == OK, name
    assert call(_wgrad(c_in=48, ld_x=48)) == UNSUP
    assert call(_wgrad(c_out=100, g=0)) == UNSUP                       # (before the pointers)
    assert call(_wgrad(g=0)) == NULLP
    assert call(_wgrad(x=0)) == NULLP
    assert call(_wgrad(), dw=None) == NULLP
    assert call(_wgrad(x=0, ld_x=32)) == NULLP                         # (before the strides)
    assert call(_wgrad(ld_x=32)) == SHAPE
    assert call(_wgrad(ld_g=64)) == SHAPE
    assert call(_wgrad(y=YM, ld_y=64)) == SHAPE
    assert call(_wgrad(ld_x=32, x=X + 4)) == SHAPE                     # (before the alignment)
    assert call(_wgrad(ld_x=66)) == MISAL
    assert call(_wgrad(ld_g=130)) == MISAL
    assert call(_wgrad(y=YM, ld_y=130)) == MISAL
    for bad in (dict(g=G + 4), dict(x=X + 8), dict(y=YM + 4, ld_y=128), dict(gamma=GA + 4, var=VA), dict(gamma=GA, var=VA + 4)):
        assert call(_wgrad(**bad)) == MISAL, bad
    assert call(_wgrad(), dw=DW + 2) == MISAL                          # dw: 4 bytes (atomics on single floats)
    assert call(_wgrad(x=X + 4), dw=X) == MISAL                        # (before the overlap)
    # dw (128 x 64 floats) overlapping g, x or y
    assert call(_wgrad(), dw=G) == OPT
    assert call(_wgrad(), dw=X + (119 * 64 + 63) * 4) == OPT           # dw starts on x's last float
    assert call(_wgrad(y=DW + (128 * 64 - 4) * 4, ld_y=128)) == OPT    # y starts on dw's last 16 bytes


def test_gz_rejects_bad_arguments_in_the_documented_order(lib):
    def call(g=G, ld_g=64, y=YM, ld_y=64, gamma=GA, var=VA, M=100, C=64, gz=DX, ld_gz=64):
        p = lambda v: ctypes.c_void_p(v) if v else None
        return lib.bevmsda_conv_gz_rows_f32(p(g), ld_g, p(y), ld_y, p(gamma), p(var), 1e-5, M, C, p(gz), ld_gz, None)
    assert call(gamma=0, M=-1) == OPT and call(var=0, C=48) == OPT
    assert call(M=-1) == SHAPE and call(C=-1) == SHAPE
    assert call(M=(1 << 24) + 1) == LARGE and call(C=65536 + 32, ld_g=1 << 17, ld_gz=1 << 17, ld_y=1 << 17) == LARGE
    assert call(M=0, g=0, gz=0) == OK and call(C=0, g=0, gz=0) == OK
    assert call(C=48, g=0) == UNSUP
    assert call(g=0) == NULLP and call(gz=0) == NULLP
    assert call(ld_g=32) == SHAPE and call(ld_gz=32) == SHAPE and call(ld_y=32) == SHAPE
    assert call(ld_g=66) == MISAL and call(ld_gz=66) == MISAL and call(ld_y=66) == MISAL
    assert call(g=G + 4) == MISAL and call(gz=DX + 4) == MISAL and call(y=YM + 4) == MISAL
    assert call(gamma=GA + 4) == MISAL and call(var=VA + 8) == MISAL
    assert call(gz=G + 64 * 4) == OPT                                  # one row into g
    assert call(gz=G, ld_g=128, ld_gz=64) == OPT                       # at g with another stride
    assert call(gz=YM) == OPT
