"""No GPU: ``bevmsda_mha_d32_f32`` validates its arguments before any device work (error codes of include/bevmsda.h), so a
bad call is a return value, never a launch.  Pointers are fake but non-NULL where a check must get past the NULL test; no
kernel runs here (style of tests/test_capi_symbols.py)."""
import ctypes

import pytest

OK, NULLP, SHAPE, LARGE, MISAL, UNSUP = 0, -1, -2, -3, -4, -7


@pytest.fixture(scope="module")
def mha():
    from bevformer_amd import _lib, build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH).bevmsda_mha_d32_f32


def _call(fn, q=0x1000, k=0x2000, v=0x3000, out=0x4000, ldq=512, ldk=512, ldv=256, ldo=256, nq=900, nk=900, bs=1, heads=8,
          D=32, scale=0.17677669):
    p = lambda a: ctypes.c_void_p(a) if a else None
    return fn(p(q), ldq, p(k), ldk, p(v), ldv, nq, nk, bs, heads, D, scale, p(out), ldo, None)


def test_entry_point_is_bound_and_declared():
    from bevformer_amd import _lib
    assert "bevmsda_mha_d32_f32" in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 4


def test_null_pointers(mha):
    for name in ("q", "k", "v", "out"):
        assert _call(mha, **{name: 0}) == NULLP, name


def test_shapes(mha):
    for name in ("nq", "nk", "bs", "heads", "D"):
        assert _call(mha, **{name: -1}) == SHAPE, name
    assert _call(mha, nk=0) == SHAPE                                  # queries, but nothing to attend to
    for name in ("ldq", "ldk", "ldv", "ldo"):
        assert _call(mha, **{name: 128}) == SHAPE, name               # narrower than heads * 32
    # empty problems are no-ops whatever the pointers
    for name in ("nq", "bs", "heads"):
        assert _call(mha, q=0, k=0, v=0, out=0, **{name: 0}) == OK, name


def test_unsupported(mha):
    for D in (64, 16, 0, 33):
        assert _call(mha, D=D) == UNSUP, D
    assert _call(mha, D=64, q=0) == UNSUP                             # decided before the pointers are looked at
    for name in ("ldq", "ldk", "ldv", "ldo"):
        assert _call(mha, **{name: 514}) == UNSUP, name               # rows not 16-byte aligned


def test_misaligned_and_too_large(mha):
    for name in ("q", "k", "v", "out"):
        assert _call(mha, **{name: 0x1004}) == MISAL, name
    assert _call(mha, bs=65536) == LARGE
    assert _call(mha, heads=65536, ldq=1 << 22, ldk=1 << 22, ldv=1 << 22, ldo=1 << 22) == LARGE
