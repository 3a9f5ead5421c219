"""No GPU: the ``bevmsda_conv3x3_*`` entry points validate every argument before any launch and answer a bad call with a code
of ``bevmsda_error_string``'s table (include/bevmsda.h).  Pointers are fake: no kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
fake = ctypes.c_void_p(0x1000)
odd = ctypes.c_void_p(0x1004)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _desc(segs=(0x1000, 0x2000), ld_seg=None, **kw):
    base = dict(bs=2, H=6, W=11, nseg=len(segs), c_seg=32, c_out=128, relu=1, precision=0, eps=1e-5, ld_y=128, ld_res=128,
                res=0x3000, gamma=0x4000, beta=0x5000, mean=0x6000, var=0x7000)
    base.update(kw)
    d = _lib.Conv3x3Desc(**base)
    for i, p in enumerate(segs[:8]):
        d.seg[i] = p
        d.ld_seg[i] = (ld_seg[i] if ld_seg is not None else base["c_seg"])
    return ctypes.byref(d)


def test_signatures_are_listed_and_the_abi_version_stays():
    assert _lib.ABI_VERSION == 7
    for name in ("bevmsda_conv3x3_packed_bytes", "bevmsda_conv3x3_pack_weight_f32", "bevmsda_conv3x3_bn_f32"):
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.Conv3x3Desc) == 8 * 8 + 8 * 8 + 3 * 8 + 4 * 8 + 8 * 4 + 4 + 3 * 4


def test_conv3x3_bn_rejects_bad_arguments(lib):
    f = lib.bevmsda_conv3x3_bn_f32
    call = lambda d, w=fake, y=fake: f(d, w, y, None)
    assert f(None, fake, fake, None) == NULLP                          # no descriptor
    assert call(_desc(precision=2)) == OPT
    assert call(_desc(precision=-1)) == OPT
    for name in ("bs", "H", "W", "c_seg", "c_out"):
        assert call(_desc(**{name: -1})) == SHAPE, name
    assert call(_desc(nseg=-1)) == SHAPE
    assert call(_desc(nseg=9)) == SHAPE                                # more than 8 segments
    assert call(_desc(bs=5000, H=100, W=100)) == LARGE                 # over 2^24 rows
    assert call(_desc(bs=1, H=1 << 13, W=(1 << 11) + 1)) == LARGE
    for name in ("bs", "H", "W", "c_out"):                             # the empty problem: no-op, whatever the pointers
        assert call(_desc(**{name: 0}), w=None, y=None) == OK, name
    assert call(_desc(nseg=0)) == SHAPE
    assert call(_desc(c_seg=0)) == SHAPE
    assert call(_desc(c_seg=48, ld_seg=(48, 48))) == UNSUP             # channel counts off the kernel's granularity
    assert call(_desc(c_out=100, ld_y=100, ld_res=100)) == UNSUP
    assert call(_desc(), w=None) == NULLP
    assert call(_desc(), y=None) == NULLP
    for name in ("gamma", "beta", "mean", "var"):
        assert call(_desc(**{name: None})) == NULLP, name
    assert call(_desc(segs=(0x1000, 0))) == NULLP
    assert call(_desc(ld_y=64)) == SHAPE                               # strides below the width
    assert call(_desc(ld_res=64)) == SHAPE
    assert call(_desc(ld_seg=(32, 16))) == SHAPE
    assert call(_desc(ld_y=130)) == MISAL                              # rows not on 16 bytes
    assert call(_desc(ld_res=130)) == MISAL
    assert call(_desc(ld_seg=(32, 34))) == MISAL
    assert call(_desc(segs=(0x1000, 0x2004))) == MISAL                 # pointers off 16 bytes
    assert call(_desc(res=0x3004)) == MISAL
    for name in ("gamma", "beta", "mean", "var"):
        assert call(_desc(**{name: 0x4004})) == MISAL, name
    assert call(_desc(), w=odd) == MISAL
    assert call(_desc(), y=odd) == MISAL


def test_pack_weight_rejects_bad_arguments(lib):
    f = lib.bevmsda_conv3x3_pack_weight_f32
    assert f(fake, -1, 32, fake, None) == SHAPE
    assert f(fake, 128, -32, fake, None) == SHAPE
    assert f(None, 0, 32, None, None) == OK                            # empty: no-op
    assert f(None, 128, 0, None, None) == OK
    assert f(fake, 128, 48, fake, None) == UNSUP
    assert f(fake, 100, 32, fake, None) == UNSUP
    assert f(None, 128, 32, fake, None) == NULLP
    assert f(fake, 128, 32, None, None) == NULLP
    assert f(ctypes.c_void_p(0x1002), 128, 32, fake, None) == MISAL
    assert f(fake, 128, 32, odd, None) == MISAL


def test_packed_bytes_matches_the_pack_kernels_layout(lib):
    """The image is ``bevmsda_linear_pack_weight_f32``'s over the (c_out, 9 c_in) matrix: per 128-row tile and 32-deep chunk
    two planes (hi, lo) of 128 rows x (32 + 8 pad) bf16."""
    f = lib.bevmsda_conv3x3_packed_bytes
    chunk = 2 * 128 * 40 * 2
    for c_out, c_in in ((128, 32), (256, 64), (512, 512), (512, 2048), (160, 96)):
        want = -(-c_out // 128) * (9 * c_in // 32) * chunk
        assert f(c_out, c_in) == want
        assert f(c_out, c_in) == lib.bevmsda_linear_packed_bytes(c_out, 9 * c_in)
    assert f(128, 48) == 0 and f(0, 32) == 0 and f(128, 0) == 0 and f(-1, 32) == 0


def test_error_strings_cover_the_codes(lib):
    for code in (OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP):
        assert lib.bevmsda_error_string(code)
