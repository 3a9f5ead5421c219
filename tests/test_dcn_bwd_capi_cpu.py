"""No GPU: ``bevmsda_deform_conv_dgrad_f32``, ``bevmsda_deform_conv_wgrad_f32`` and the input gradient's weight-image pair
(``bevmsda_deform_dgrad_packed_bytes`` / ``bevmsda_deform_dgrad_pack_weight_f32``) validate every argument before any launch and
answer a bad call with a code of ``bevmsda_error_string``'s table, in the order include/bevmsda.h documents.  Pointers are fake:
no kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
# far apart: nothing overlaps by accident
G, YM, X, OFF, DX, DOFF, DW, WP, V = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000, 0x900000
GA, VA = V, V + 0x1000
fake = ctypes.c_void_p(WP)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _dgrad(**kw):
    base = dict(g=G, ld_g=128, x=X, ld_x=64, offs=OFF, ld_offs=32, dx=DX, ld_dx=64, doffs=DOFF, ld_doffs=32, eps=1e-5, n_img=2, H=6,
                W=10, c_in=64, c_out=128, stride=1, precision=0, need_dx=1, need_doffs=1)
    base.update(kw)
    return ctypes.byref(_lib.DeformConvDgradDesc(**base))


def _wgrad(**kw):
    base = dict(g=G, ld_g=128, x=X, ld_x=64, offs=OFF, ld_offs=32, eps=1e-5, n_img=2, H=6, W=10, c_in=64, c_out=128, stride=1,
                precision=0)
    base.update(kw)
    return ctypes.byref(_lib.DeformConvWgradDesc(**base))


def test_signatures_are_listed_and_the_abi_version_stays():
    assert _lib.ABI_VERSION == 7
    for name in ("bevmsda_deform_conv_dgrad_f32", "bevmsda_deform_conv_wgrad_f32", "bevmsda_deform_dgrad_packed_bytes",
                 "bevmsda_deform_dgrad_pack_weight_f32"):
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.DeformConvDgradDesc) == 14 * 8 + 4 + 9 * 4 + 2 * 4
    assert _lib.DeformConvDgradDesc.eps.offset == 112 and _lib.DeformConvDgradDesc.n_img.offset == 116
    assert _lib.DeformConvDgradDesc.need_doffs.offset == 148
    assert ctypes.sizeof(_lib.DeformConvWgradDesc) == 10 * 8 + 4 + 7 * 4 + 2 * 4
    assert _lib.DeformConvWgradDesc.eps.offset == 80 and _lib.DeformConvWgradDesc.n_img.offset == 84


def test_header_declares_the_entry_points_and_the_library_exports_them(lib):
    from bevformer_amd import build
    text = open(build.PUBLIC_HEADER).read()
    assert "int bevmsda_deform_conv_dgrad_f32(const bevmsda_deform_conv_dgrad_desc *desc, const uint16_t *wpack, void *stream);" in text
    assert "int bevmsda_deform_conv_wgrad_f32(const bevmsda_deform_conv_wgrad_desc *desc, float *dw, void *stream);" in text
    assert "int bevmsda_deform_dgrad_pack_weight_f32(const float *w, int32_t c_out, int32_t c_in, uint16_t *blob, void *stream);" in text
    assert "#define BEVMSDA_ABI_VERSION 7" in text
    for name in ("bevmsda_deform_conv_dgrad_f32", "bevmsda_deform_conv_wgrad_f32", "bevmsda_deform_dgrad_packed_bytes",
                 "bevmsda_deform_dgrad_pack_weight_f32"):
        assert getattr(lib, name) is not None


def test_weight_image_size_and_pack_checks(lib):
    size = lib.bevmsda_deform_dgrad_packed_bytes
    assert size(128, 64, ) == 5 * 4 * 2 * 128 * 40 * 2             # rows = 9 c_in padded to 128 (576 -> 640), K = c_out in chunks of 32
    assert size(64, 256) == 18 * 2 * 2 * 128 * 40 * 2
    assert size(48, 64) == 0 and size(64, 48) == 0 and size(0, 64) == 0 and size(64, -32) == 0
    pack = lib.bevmsda_deform_dgrad_pack_weight_f32
    blob = ctypes.c_void_p(DX)
    assert pack(fake, -1, 64, blob, None) == SHAPE and pack(fake, 64, -1, blob, None) == SHAPE
    assert pack(fake, 65536 + 32, 64, blob, None) == LARGE
    assert pack(None, 0, 64, None, None) == OK and pack(None, 64, 0, None, None) == OK
    assert pack(fake, 48, 64, blob, None) == UNSUP and pack(fake, 64, 48, blob, None) == UNSUP
    assert pack(None, 64, 64, blob, None) == NULLP and pack(fake, 64, 64, None, None) == NULLP
    assert pack(ctypes.c_void_p(WP + 2), 64, 64, blob, None) == MISAL
    assert pack(fake, 64, 64, ctypes.c_void_p(DX + 8), None) == MISAL


def test_dgrad_rejects_bad_arguments_in_the_documented_order(lib):
    def call(d, w=fake):
        return lib.bevmsda_deform_conv_dgrad_f32(d, w, None)
    assert lib.bevmsda_deform_conv_dgrad_f32(None, fake, None) == NULLP                               # 1. no descriptor
    for bad in (dict(stride=0), dict(stride=3), dict(precision=2), dict(precision=-1), dict(gamma=GA), dict(var=VA)):
        assert call(_dgrad(H=-1, **bad)) == OPT, bad                   # 2. options come first, whatever else is wrong
    for name in ("n_img", "H", "W", "c_in", "c_out"):                  # 3. a negative size
        assert call(_dgrad(**{name: -1})) == SHAPE, name
    assert call(_dgrad(n_img=5000, H=100, W=100)) == LARGE             # 4. over 2^24 input rows
    assert call(_dgrad(n_img=5000, H=100, W=100, stride=2)) == LARGE
    assert call(_dgrad(c_in=65536 + 32, ld_x=65536 + 32, ld_dx=65536 + 32)) == LARGE
    assert call(_dgrad(c_out=65536 + 32, ld_g=65536 + 32)) == LARGE
    for name in ("n_img", "H", "W", "c_in", "c_out"):                  # 5. the empty problem: no-op, whatever the pointers
        assert call(_dgrad(g=0, x=0, offs=0, dx=0, doffs=0, **{name: 0}), w=None) == OK, name
    assert call(_dgrad(g=0, need_dx=0, need_doffs=0), w=None) == OK    # (nothing asked for)
    assert call(_dgrad(c_in=48, ld_x=48, ld_dx=48)) == UNSUP           # 6. channel counts off the kernel's granularity
    assert call(_dgrad(c_out=100, ld_g=100)) == UNSUP
    assert call(_dgrad(c_in=48, g=0)) == UNSUP                         # (before the pointers)
    for name in ("g", "x", "offs", "dx", "doffs"):                     # 7.
        assert call(_dgrad(**{name: 0})) == NULLP, name
    assert call(_dgrad(), w=None) == NULLP
    assert call(_dgrad(g=0, ld_g=64)) == NULLP                         # (before the strides)
    for bad in (dict(ld_g=64), dict(ld_x=32), dict(ld_offs=28), dict(ld_dx=32), dict(ld_doffs=28), dict(y=YM, ld_y=64)):
        assert call(_dgrad(**bad)) == SHAPE, bad                       # 8. strides below the width; ld_offs, ld_doffs >= 32
    assert call(_dgrad(ld_g=64, g=G + 4)) == SHAPE                     # (before the alignment)
    for bad in (dict(ld_g=130), dict(ld_x=66), dict(ld_offs=34), dict(ld_dx=66), dict(ld_doffs=34), dict(y=YM, ld_y=130)):
        assert call(_dgrad(**bad)) == MISAL, bad                       # 9. rows not on 16 bytes
    for bad in (dict(g=G + 4), dict(x=X + 8), dict(offs=OFF + 4), dict(dx=DX + 4), dict(doffs=DOFF + 8), dict(y=YM + 4, ld_y=128),
                dict(gamma=GA + 4, var=VA), dict(gamma=GA, var=VA + 4)):
        assert call(_dgrad(**bad)) == MISAL, bad
    assert call(_dgrad(), w=ctypes.c_void_p(WP + 4)) == MISAL
    assert call(_dgrad(g=G + 4, dx=G)) == MISAL                        # (before the overlap)
    # 10. dx (120 rows of 64 floats) or doffs (120 rows of 32) overlapping g (120 rows of 128), y, x, offs or one another
    assert call(_dgrad(dx=G)) == OPT and call(_dgrad(doffs=G)) == OPT
    assert call(_dgrad(dx=G + (119 * 128 + 124) * 4)) == OPT           # dx starts on g's last 16 bytes
    assert call(_dgrad(dx=X)) == OPT and call(_dgrad(doffs=X + (119 * 64 + 60) * 4)) == OPT
    assert call(_dgrad(dx=OFF)) == OPT and call(_dgrad(doffs=OFF + (119 * 32 + 28) * 4)) == OPT
    assert call(_dgrad(y=DX + (119 * 64 + 60) * 4, ld_y=128)) == OPT   # y starts on dx's last 16 bytes
    assert call(_dgrad(y=DOFF, ld_y=128)) == OPT
    assert call(_dgrad(doffs=DX + (119 * 64 + 60) * 4)) == OPT         # doffs starts on dx's last 16 bytes
    # stride 2: g and doffs have 2 * 3 * 5 = 30 rows
    assert call(_dgrad(stride=2, dx=G + (29 * 128 + 124) * 4)) == OPT
    assert call(_dgrad(stride=2, dx=DOFF + (29 * 32 + 28) * 4)) == OPT
    # a part that is left out is not looked at: its pointer may be NULL, misaligned or overlapping
    assert call(_dgrad(c_in=48, ld_x=48, need_dx=0, dx=0)) == UNSUP    # (reaches the granularity check, not NULLP)
    assert call(_dgrad(ld_dx=2, need_dx=0, dx=G + 4, y=YM, ld_y=64)) == SHAPE      # (only y's stride is wrong)
    assert call(_dgrad(ld_doffs=2, need_doffs=0, doffs=X + 4, ld_g=130)) == MISAL  # (only g's stride is wrong)


def test_wgrad_rejects_bad_arguments_in_the_documented_order(lib):
    def call(d, dw=DW):
        return lib.bevmsda_deform_conv_wgrad_f32(d, ctypes.c_void_p(dw) if dw is not None else None, None)
    assert lib.bevmsda_deform_conv_wgrad_f32(None, ctypes.c_void_p(DW), None) == NULLP
    for bad in (dict(stride=0), dict(stride=4), dict(precision=2), dict(gamma=GA), dict(var=VA)):
        assert call(_wgrad(H=-1, **bad)) == OPT, bad
    for name in ("n_img", "H", "W", "c_in", "c_out"):
        assert call(_wgrad(**{name: -1})) == SHAPE, name
    assert call(_wgrad(n_img=5000, H=100, W=100)) == LARGE
    assert call(_wgrad(n_img=1, H=1 << 13, W=(1 << 11) + 1, stride=2)) == LARGE
    assert call(_wgrad(c_in=65536 + 32, ld_x=65536 + 32)) == LARGE
    for name in ("n_img", "H", "W", "c_in", "c_out"):                  # the empty problem: nothing to add
        assert call(_wgrad(g=0, x=0, offs=0, **{name: 0}), dw=None) == OK, name
    assert call(_wgrad(c_in=48, ld_x=48)) == UNSUP
    assert call(_wgrad(c_out=100, g=0)) == UNSUP                       # (before the pointers)
    for name in ("g", "x", "offs"):
        assert call(_wgrad(**{name: 0})) == NULLP, name
    assert call(_wgrad(), dw=None) == NULLP
    assert call(_wgrad(x=0, ld_x=32)) == NULLP                         # (before the strides)
    for bad in (dict(ld_x=32), dict(ld_g=64), dict(ld_offs=28), dict(y=YM, ld_y=64)):
        assert call(_wgrad(**bad)) == SHAPE, bad
    assert call(_wgrad(ld_x=32, x=X + 4)) == SHAPE                     # (before the alignment)
    for bad in (dict(ld_x=66), dict(ld_g=130), dict(ld_offs=34), dict(y=YM, ld_y=130)):
        assert call(_wgrad(**bad)) == MISAL, bad
    for bad in (dict(g=G + 4), dict(x=X + 8), dict(offs=OFF + 4), dict(y=YM + 4, ld_y=128), dict(gamma=GA + 4, var=VA),
                dict(gamma=GA, var=VA + 4)):
        assert call(_wgrad(**bad)) == MISAL, bad
    assert call(_wgrad(), dw=DW + 2) == MISAL                          # dw: 4 bytes (atomics on single floats)
    assert call(_wgrad(x=X + 4), dw=X) == MISAL                        # (before the overlap)
    # dw (128 x 64 x 9 floats) overlapping g, x, offs or y
    assert call(_wgrad(), dw=G) == OPT
    assert call(_wgrad(), dw=X + (119 * 64 + 63) * 4) == OPT           # dw starts on x's last float
    assert call(_wgrad(), dw=OFF + (119 * 32 + 31) * 4) == OPT         # dw starts on offs's last float
    assert call(_wgrad(y=DW + (9 * 128 * 64 - 4) * 4, ld_y=128)) == OPT     # y starts on dw's last 16 bytes
