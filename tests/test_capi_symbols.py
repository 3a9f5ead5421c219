"""The C-ABI library loads on a machine without a GPU and exports every entry
point include/bevmsda.h declares, with the ABI version the host expects.  No
compute call is made here (that is the `-m gpu` suite)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bevmsda.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(bevmsda_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib_path():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return build.LIB_PATH


def test_header_declares_the_operator_pair():
    names = _declared()
    for want in ("bevmsda_forward_f32", "bevmsda_backward_f32", "bevmsda_forward_bf16",
                 "bevmsda_backward_bf16", "bevmsda_abi_version", "bevmsda_error_string"):
        assert want in names


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for name in _declared():
        assert hasattr(lib, name), f"{name} declared in include/bevmsda.h but not exported"
    from bevformer_amd import _lib
    assert lib.bevmsda_abi_version() == _lib.ABI_VERSION
    # host binding table and header agree (nothing bound that is not declared, and vice versa)
    assert sorted(_lib.SIGNATURES) == [n for n in _declared()]


def test_exports_are_plain_c_names(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in _declared():
        assert name in exported


def test_error_strings_and_host_argument_checks_without_gpu(lib_path):
    lib = ctypes.CDLL(lib_path)
    lib.bevmsda_error_string.restype = ctypes.c_char_p
    assert lib.bevmsda_error_string(0) == b"ok"
    for code in range(-1, -10, -1):
        assert lib.bevmsda_error_string(code)  # never NULL
    # argument validation happens before any device work: negative dims are
    # rejected and an all-empty problem is a no-op, with no GPU present
    from bevformer_amd import _lib
    h = _lib.load(lib_path)
    assert h.bevmsda_forward_f32(None, None, None, None, None, -1, 0, 8, 32, 1, 0, 4, None, None) \
        == -2
    assert h.bevmsda_forward_f32(None, None, None, None, None, 0, 0, 8, 32, 1, 0, 4, None, None) \
        == 0


def test_row_panel_knob_range_without_gpu(lib_path):
    """``desc.reserved[3]`` of the row-panel entry point: shapes 1 and 2 take 0 only (the prefetch-depth, epilogue, phase-skew
    and one-wavefront-per-SIMD knobs are retired), shape 3 takes its knobs 0 .. 4, and there is no shape 4.  A rejected
    value is a return code before any launch: the pointers are fake."""
    from bevformer_amd import _lib
    h = _lib.load(lib_path)
    OPT = -6
    fake = ctypes.c_void_p(0x1000)                # 16-byte aligned, never dereferenced

    def call(shape, knob):
        d = _lib.LinearDesc(M=64, ldx0=256, ldw=256, ldy=256, N=256, K0=256, K1=0)
        d.reserved[2], d.reserved[3] = shape, knob
        return h.bevmsda_linear_panel_f32(fake, None, None, None, None, None, fake, None, ctypes.byref(d), None, fake, None)

    for knob in (2, 6, 33, 36, 64, 70, 97, 98):
        assert call(1, knob) == OPT, knob
        assert call(2, knob) == OPT, knob
        assert call(0, knob) == OPT, knob         # (the shape rule picks 1 or 2 here)
    assert call(3, 5) == OPT
    assert call(3, -1) == OPT
    assert call(4, 0) == OPT


def test_fused_sampling_knob_range_without_gpu(lib_path):
    """``bevmsda_fused_desc.reserved`` of the fused sampling entry points (ABI version 7): [5] takes 0 or 1, [0] and [4] take 0,
    [3] is the row-count hint of the ``_rows_`` entry points and 0 elsewhere — the retired kernel-body, register-budget,
    LDS-pad and grid-shape knobs are ``BEVMSDA_ERR_BAD_OPTION`` on every entry point, before any launch: the pointers are fake.
    The descriptors are valid TemporalSelfAttention / SpatialCrossAttention shapes whose row count is one past what the launch
    geometry takes, so an ACCEPTED option comes back as ``BEVMSDA_ERR_TOO_LARGE`` (a check behind the option checks), never
    as a launch."""
    from bevformer_amd import _lib
    h = _lib.load(lib_path)
    BIG, OPT = -3, -6
    fake = ctypes.c_void_p(0x1000)                # 16-byte aligned, never dereferenced
    shapes = {"tsa": dict(L=1, P=4, K=2, A=1, ref_mode=1, off_head=16, off_k=8, lg_head=8, lg_k=4, vmul=2, vadd=1),
              "sca": dict(L=4, P=8, K=1, A=4, ref_mode=0, off_head=64, off_k=0, lg_head=32, lg_k=0, vmul=1, vadd=0)}
    STATIC_ROWS, DYN_ROWS = (1 << 33) - 8, 1 << 27   # (2^31 - 2 logical blocks; the device-row-count form's capacity bound)

    def call(entry, shape, **reserved):
        dyn = "_rows_" in entry
        d = _lib.FusedDesc(R=DYN_ROWS if dyn else STATIC_ROWS, proj_row=512, N=2, S=1024, M=8, D=32, Q=1024, **shapes[shape])
        for i, v in reserved.items():
            d.reserved[int(i[1:])] = v
        head = [fake] * 8
        if entry == "bevmsda_fused_forward_halo_f32":
            return getattr(h, entry)(*head, ctypes.byref(d), fake, 4, 64, fake, fake, None)
        if entry == "bevmsda_fused_forward_rows_save_f32":
            return getattr(h, entry)(*head, fake, ctypes.byref(d), fake, fake, fake, None)
        if dyn:
            return getattr(h, entry)(*head, fake, ctypes.byref(d), fake, None)
        return getattr(h, entry)(*head, ctypes.byref(d), fake, None)

    cases = [("bevmsda_fused_forward_f32", "tsa"), ("bevmsda_fused_forward_f32", "sca"),
             ("bevmsda_fused_forward_bf16", "tsa"), ("bevmsda_fused_forward_bf16", "sca"),
             ("bevmsda_fused_forward_halo_f32", "tsa"),
             ("bevmsda_fused_forward_rows_f32", "tsa"), ("bevmsda_fused_forward_rows_f32", "sca"),
             ("bevmsda_fused_forward_rows_save_f32", "sca")]
    for entry, shape in cases:
        assert call(entry, shape) == BIG, (entry, shape)          # the descriptor itself passes every option check
        assert call(entry, shape, r5=1) == BIG, (entry, shape)    # generic bodies: still an option
        for v in (2, 3, 4, 5, -1, 6):
            assert call(entry, shape, r5=v) == OPT, (entry, shape, v)
        for v in (4, 8):
            assert call(entry, shape, r0=v) == OPT, (entry, shape, v)
        for v in (1, 54, 64):
            assert call(entry, shape, r4=v) == OPT, (entry, shape, v)
        if "_rows_" not in entry:
            assert call(entry, shape, r3=(8 << 16) | 16) == OPT, (entry, shape)
    assert call("bevmsda_fused_forward_rows_f32", "sca", r3=7) == BIG            # the hint: not rejected as an option
    assert call("bevmsda_fused_forward_rows_f32", "tsa", r3=7) == BIG


def test_fused_spec_outside_its_range_fails_loudly(monkeypatch):
    """``BEVMSDA_FUSED_SPEC`` / ``modes.fused_spec`` take 0 and 1; a retired value raises instead of running the default, and the
    retired register-budget and LDS-pad modes are unknown names."""
    from bevformer_amd import modes
    monkeypatch.setenv("BEVMSDA_FUSED_SPEC", "4")
    with pytest.raises(ValueError, match="BEVMSDA_FUSED_SPEC"):
        modes.Modes()
    monkeypatch.setenv("BEVMSDA_FUSED_SPEC", "1")
    assert modes.Modes().fused_spec == 1
    monkeypatch.delenv("BEVMSDA_FUSED_SPEC")
    assert modes.Modes().fused_spec == 0
    for name in ("fused_wpe", "fused_lds_pad_kb"):
        with pytest.raises(AttributeError):
            with modes.using(**{name: 4}):
                pass


def test_projection_and_prologue_argument_checks_without_gpu(lib_path):
    """The entry points added for the projections and the encoder's caller validate their
    arguments before any device work (error codes of include/bevmsda.h), so a bad call is a
    return value, never a launch.  Pointers are fake but non-NULL where a check must get past
    the NULL test; no kernel runs in this test."""
    from bevformer_amd import _lib
    h = _lib.load(lib_path)
    OK, NULLP, SHAPE, MISAL, OPT, UNSUP = 0, -1, -2, -4, -6, -7
    fake = ctypes.c_void_p(0x1000)                # 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(0x1004)

    def desc(**kw):
        base = dict(M=8, ldx0=64, ldw=64, ldy=128, N=128, K0=64, K1=0)
        base.update(kw)
        return ctypes.byref(_lib.LinearDesc(**base))

    lin = h.bevmsda_linear_f32
    assert lin(fake, None, None, None, fake, None, None, fake, None) == NULLP          # no descriptor
    assert lin(fake, None, None, None, None, None, desc(), fake, None) == NULLP        # no weight
    assert lin(fake, None, None, None, fake, None, desc(M=-1), fake, None) == SHAPE
    assert lin(fake, None, None, None, fake, None, desc(M=0), fake, None) == OK        # empty: no-op
    assert lin(fake, None, None, None, fake, None, desc(K0=48), fake, None) == UNSUP   # K % 32
    assert lin(fake, None, None, None, fake, None, desc(ldx0=66), fake, None) == UNSUP
    assert lin(fake, None, None, None, fake, None, desc(ldx0=32), fake, None) == SHAPE  # ld < K
    assert lin(odd, None, None, None, fake, None, desc(), fake, None) == MISAL
    assert lin(fake, None, None, None, fake, None, desc(precision=7), fake, None) == OPT
    assert lin(fake, None, None, None, fake, None, desc(K1=32), fake, None) == NULLP   # x1 missing
    assert lin(fake, None, None, None, fake, None, desc(group_cols=96), fake, None) == UNSUP
    assert lin(fake, None, None, None, fake, None, desc(variant=1 + 12), fake, None) == OPT   # packed variant, fp32 weight
    assert h.bevmsda_linear_packed_f32(fake, None, None, None, None, None, desc(), fake, None) == NULLP
    assert h.bevmsda_linear_packed_f32(fake, None, None, None, fake, None, desc(variant=1 + 2), fake, None) == OPT
    assert h.bevmsda_linear_gather_packed_f32(fake, 64, None, fake, fake, None, desc(), fake, None) == NULLP
    assert h.bevmsda_linear_gather_packed_f32(fake, 64, fake, fake, fake, None, desc(K1=32), fake, None) == SHAPE

    assert h.bevmsda_linear_packed_bytes(256, 256) == 2 * 8 * 2 * 128 * 40 * 2
    assert h.bevmsda_linear_packed_bytes(130, 64) == 2 * 2 * 2 * 128 * 40 * 2          # N padded to 256
    assert h.bevmsda_linear_packed_bytes(256, 48) == 0
    assert h.bevmsda_linear_pack_weight_f32(fake, 64, 0, 64, fake, None) == SHAPE
    assert h.bevmsda_linear_pack_weight_f32(fake, 64, 8, 48, fake, None) == UNSUP
    assert h.bevmsda_linear_pack_weight_f32(None, 64, 8, 64, fake, None) == NULLP

    theta = (ctypes.c_float * 6)(1, 0, 0, 0, 1, 0)
    rot = h.bevmsda_rotate_bev_f32
    assert rot(fake, 256, fake, 256, 4, 4, 256, theta, None) == OPT                     # in place
    assert rot(fake, 256, ctypes.c_void_p(0x2000), 256, 4, 4, 100, theta, None) == UNSUP
    assert rot(fake, 128, ctypes.c_void_p(0x2000), 256, 4, 4, 256, theta, None) == SHAPE
    assert rot(fake, 256, ctypes.c_void_p(0x2000), 256, 0, 4, 256, theta, None) == OK
    assert rot(None, 256, ctypes.c_void_p(0x2000), 256, 4, 4, 256, theta, None) == NULLP
    fl = h.bevmsda_flatten_feats_f32
    assert fl(fake, None, None, fake, 1, 6, 256, 10, 5, 0, None) == SHAPE               # s0 + hw > S
    assert fl(fake, None, None, fake, 1, 6, 100, 10, 10, 0, None) == UNSUP
    assert fl(fake, None, None, fake, 0, 6, 256, 10, 10, 0, None) == OK
    assert fl(None, None, None, fake, 1, 6, 256, 10, 10, 0, None) == NULLP
