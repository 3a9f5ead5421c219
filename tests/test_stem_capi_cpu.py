"""No GPU: ``bevmsda_stem_f32`` and its weight-image entry points validate every argument before any launch and answer a bad call
with a code of ``bevmsda_error_string``'s table, in the order include/bevmsda.h documents.  Pointers are fake, so every call here
is one that a check refuses or an empty problem: no kernel runs."""
import ctypes

import pytest

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
X, Y, WP, BN = 0x100000, 0x400000, 0x500000, 0x600000    # far apart: nothing overlaps by accident
BNS = [BN, BN + 0x1000, BN + 0x2000, BN + 0x3000]
fake = ctypes.c_void_p(WP)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _desc(bn=BNS, **kw):
    # (2, 3, 10, 20) dense: Hc x Wc = 5 x 10, Hp x Wp = 3 x 5
    base = dict(x=X, ld_img=600, ld_ch=200, ld_row=20, eps=1e-5, n_img=2, H=10, W=20, c_in=3, c_out=64, pool=1, precision=0)
    base.update(kw)
    d = _lib.StemDesc(**base)
    for i, v in enumerate(bn):
        d.bn[i] = v
    return ctypes.byref(d)


def _call(lib, d, w=fake, y=Y, ld_y=64):
    return lib.bevmsda_stem_f32(d, w, ctypes.c_void_p(y) if y is not None else None, ld_y, None)


def test_signatures_are_listed_and_the_abi_version_stays():
    assert _lib.ABI_VERSION == 7
    for name in ("bevmsda_stem_packed_bytes", "bevmsda_stem_pack_weight_f32", "bevmsda_stem_f32"):
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.StemDesc) == 4 * 8 + 4 * 8 + 4 + 7 * 4 + 2 * 4 == 104
    D = _lib.StemDesc
    assert (D.x.offset, D.ld_img.offset, D.ld_ch.offset, D.ld_row.offset, D.bn.offset) == (0, 8, 16, 24, 32)
    assert (D.eps.offset, D.n_img.offset, D.H.offset, D.W.offset, D.c_in.offset, D.c_out.offset, D.pool.offset,
            D.precision.offset, D.reserved.offset) == (64, 68, 72, 76, 80, 84, 88, 92, 96)


def test_header_declares_the_entry_points_and_the_descriptor():
    from bevformer_amd import build
    text = open(build.PUBLIC_HEADER).read()
    assert "int64_t bevmsda_stem_packed_bytes(int32_t c_out, int32_t c_in);" in text
    assert "int bevmsda_stem_pack_weight_f32(const float *w, int32_t c_out, int32_t c_in, uint16_t *out, void *stream);" in text
    assert "int bevmsda_stem_f32(const bevmsda_stem_desc *desc, const uint16_t *wpack, float *y, int64_t ld_y, void *stream);" in text
    assert "} bevmsda_stem_desc;" in text
    assert "#define BEVMSDA_ABI_VERSION 7" in text


def test_packed_bytes_is_the_documented_formula(lib):
    assert lib.bevmsda_stem_packed_bytes(64, 3) == 2 * 11 * 64 * 16 * 2          # planes x k-steps x columns x 16 k x 2 bytes
    assert lib.bevmsda_stem_packed_bytes(64, 4) == 0
    assert lib.bevmsda_stem_packed_bytes(32, 3) == 0


def test_pack_weight_rejects_bad_arguments(lib):
    pack = lambda w, N, C, out: lib.bevmsda_stem_pack_weight_f32(w, N, C, out, None)
    w, out = ctypes.c_void_p(X), ctypes.c_void_p(WP)
    assert pack(w, -1, 3, out) == SHAPE and pack(w, 64, -1, out) == SHAPE
    assert pack(None, 0, 3, None) == OK and pack(None, 64, 0, None) == OK
    assert pack(w, 64, 4, out) == UNSUP and pack(w, 32, 3, out) == UNSUP and pack(None, 32, 3, None) == UNSUP
    assert pack(None, 64, 3, out) == NULLP and pack(w, 64, 3, None) == NULLP
    assert pack(ctypes.c_void_p(X + 2), 64, 3, out) == MISAL and pack(w, 64, 3, ctypes.c_void_p(WP + 8)) == MISAL


def test_stem_rejects_bad_arguments_in_the_documented_order(lib):
    call = lambda d, **kw: _call(lib, d, **kw)
    assert lib.bevmsda_stem_f32(None, fake, ctypes.c_void_p(Y), 64, None) == NULLP     # 1. no descriptor
    for bad in (dict(pool=2), dict(pool=-1), dict(precision=2), dict(precision=-1)):    # 2. options first, whatever else is wrong
        assert call(_desc(H=-1, **bad)) == OPT, bad
    for name in ("n_img", "H", "W", "c_in", "c_out"):                  # 3. a negative size
        assert call(_desc(**{name: -1})) == SHAPE, name
    assert call(_desc(n_img=-1, c_in=4)) == SHAPE                      # (before the channel counts)
    assert call(_desc(n_img=1, H=1 << 13, W=(1 << 13) + 2)) == LARGE   # 4. 2^12 x (2^12 + 1) conv pixels
    assert call(_desc(n_img=5000, H=200, W=200)) == LARGE              # 5000 x 100 x 100
    assert call(_desc(n_img=5000, H=200, W=200, pool=0)) == LARGE
    assert call(_desc(n_img=5000, H=200, W=200, c_in=4)) == LARGE      # (before the channel counts)
    for name in ("n_img", "H", "W", "c_out"):                          # 5. the empty problem: no-op, whatever the pointers
        assert call(_desc(bn=[0, 0, 0, 0], x=0, **{name: 0}), w=None, y=None) == OK, name
    assert call(_desc(n_img=0, c_in=4)) == OK                          # (before the channel counts)
    for bad in (dict(c_in=4), dict(c_in=0), dict(c_in=1), dict(c_out=32), dict(c_out=128)):        # 6. not 3 -> 64 channels
        assert call(_desc(**bad), ld_y=128) == UNSUP, bad
    assert call(_desc(c_in=4, x=0)) == UNSUP                           # (before the pointers)
    assert call(_desc(x=0)) == NULLP                                   # 7.
    assert call(_desc(), w=None) == NULLP
    assert call(_desc(), y=None) == NULLP
    for i in range(4):
        assert call(_desc(bn=[0 if j == i else v for j, v in enumerate(BNS)])) == NULLP, i
    assert call(_desc(x=0, ld_row=19)) == NULLP                        # (before the strides)
    assert call(_desc(ld_row=19)) == SHAPE                             # 8. a row stride below the width
    assert call(_desc(ld_ch=199)) == SHAPE                             # channels that overlap: 9 x 20 + 20 = 200
    assert call(_desc(ld_row=30, ld_ch=289)) == SHAPE                  # 9 x 30 + 20 = 290
    assert call(_desc(ld_img=599)) == SHAPE                            # images that overlap: 2 x 200 + 200
    assert call(_desc(ld_ch=300, ld_img=799)) == SHAPE                 # 2 x 300 + 200
    assert call(_desc(ld_ch=0)) == SHAPE and call(_desc(ld_img=0)) == SHAPE
    assert call(_desc(), ld_y=60) == SHAPE
    assert call(_desc(ld_row=19, x=X + 2)) == SHAPE                    # (before the alignment)
    assert call(_desc(ld_row=30, ld_ch=290, ld_img=900), y=X) == OPT   # (a crop's strides pass: the call gets as far as the overlap)
    assert call(_desc(), ld_y=66) == MISAL                             # 9. rows of y not on 16 bytes
    assert call(_desc(), y=Y + 4) == MISAL
    assert call(_desc(), w=ctypes.c_void_p(WP + 8)) == MISAL
    for i in range(4):
        assert call(_desc(bn=[v + 4 if j == i else v for j, v in enumerate(BNS)])) == MISAL, i
    assert call(_desc(x=X + 2)) == MISAL                               # x: 4 bytes
    assert call(_desc(x=X + 4), y=X + 16, ld_y=68) == OPT              # ... are enough, and 4 floats for ld_y: as far as the overlap
    assert call(_desc(x=X + 2), y=X) == MISAL                          # (before the overlap)
    # 10. y overlapping x: x spans 1200 floats; pooled y 30 rows of 64, un-pooled 100 rows
    assert call(_desc(), y=X) == OPT
    assert call(_desc(), y=X + 1196 * 4) == OPT                        # y starts on x's last 16 bytes
    assert call(_desc(x=Y + (29 * 64 + 60) * 4)) == OPT                # x starts on y's last 16 bytes
    assert call(_desc(pool=0, x=Y + 30 * 64 * 4)) == OPT               # the un-pooled rows reach further
    assert call(_desc(pool=0, x=Y + (99 * 64 + 60) * 4)) == OPT
    assert call(_desc(ld_img=100000), y=X + 100000 * 4) == OPT         # the second image of a strided batch
