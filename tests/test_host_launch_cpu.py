"""The host layer's shared pieces, without a GPU: the one image cache (``ops.images._image``), the return-code classification
behind the one launch tail (``ops._declined``) and the row-panel launch shape (``ops._panel_launch_shape``)."""
import pytest
import torch

from bevformer_amd import _lib, modes, ops
from bevformer_amd.ops import images


@pytest.fixture
def not_capturing(monkeypatch):
    """No device here: the capture test of ``_cached_image`` answers "no" without asking the runtime."""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)


class _Counter:
    def __init__(self, result=True):
        self.calls, self.result = 0, result

    def __call__(self, weight):
        self.calls += 1
        return object() if self.result else None


def test_image_is_built_once_and_rebuilt_after_a_write(not_capturing):
    w = torch.nn.Parameter(torch.randn(8, 4))
    build = _Counter()
    key = lambda: (ops._ver(w), w.data_ptr())
    first = images._image(w, "_bevmsda_pack", key(), build)
    assert images._image(w, "_bevmsda_pack", key(), build) is first and build.calls == 1
    assert w._bevmsda_pack == (key(), first) and w._bevmsda_pack[1] is first        # the (key, payload) layout
    with torch.no_grad():
        w.add_(1)
    second = images._image(w, "_bevmsda_pack", key(), build)
    assert second is not first and build.calls == 2 and w._bevmsda_pack[1] is second
    assert images._image(w, "_bevmsda_pack", key(), build) is second and build.calls == 2


def test_image_that_is_not_covered_caches_nothing(not_capturing):
    w = torch.randn(8, 4)
    build = _Counter(result=False)
    assert images._image(w, "_bevmsda_panel", ("k",), build) is None
    assert not hasattr(w, "_bevmsda_panel") and build.calls == 1
    assert images._image(w, "_bevmsda_panel", ("k",), build) is None and build.calls == 2


def test_image_attribute_must_be_registered(not_capturing):
    w = torch.randn(8, 4)
    with pytest.raises(AssertionError):
        images._image(w, "_bevmsda_new", ("k",), _Counter())
    assert not hasattr(w, "_bevmsda_new")


def test_clear_weight_caches_knows_every_registered_attribute():
    lin = torch.nn.Linear(8, 4)
    for name in images.IMAGE_ATTRS:
        setattr(lin.weight, name, ("k", torch.zeros(1)))
    holder = torch.nn.Module()
    holder.lin = lin
    assert len(set(images.IMAGE_ATTRS)) == len(images.IMAGE_ATTRS) >= 6
    assert ops.clear_weight_caches(holder) == len(images.IMAGE_ATTRS)
    assert not any(hasattr(lin.weight, name) for name in images.IMAGE_ATTRS)


def test_return_code_classification():
    assert ops._declined(0, "probe") is False
    assert ops._declined(_lib.ERR_UNSUPPORTED, "probe") is True
    assert ops._declined(_lib.ERR_MISALIGNED, "probe") is True
    with pytest.raises(RuntimeError, match="probe launch failed"):
        ops._declined(_lib.ERR_TOO_LARGE, "probe launch")
    assert ops._declined(_lib.ERR_TOO_LARGE, "probe", also_declined=(_lib.ERR_TOO_LARGE,)) is True
    other = next(c for c in range(-1, -20, -1) if c not in (_lib.ERR_UNSUPPORTED, _lib.ERR_MISALIGNED, _lib.ERR_TOO_LARGE))
    with pytest.raises(RuntimeError, match="probe launch failed"):
        ops._declined(other, "probe launch", also_declined=(_lib.ERR_TOO_LARGE,))
    # a call with no other path: nothing is declined, zero still passes
    assert ops._declined(0, "probe", required=True) is False
    for code in (_lib.ERR_UNSUPPORTED, _lib.ERR_MISALIGNED):
        with pytest.raises(RuntimeError, match="must-succeed failed"):
            ops._declined(code, "must-succeed", required=True)


# (desc.reserved[2], desc.reserved[3]) of a row-panel launch at K = 256, read off the code before ``_panel_launch_shape`` existed
# (``_panel_shape`` + the decode in ``_panel_call``; ``linear_rows2``'s copy agreed with the plain column wherever both apply):
# per kernel name one row per form, and in a row (M, N) = (64, 256), (64, 1024), (1 << 16, 256), (1 << 16, 1024), (1 << 17, 256), (1 << 17, 1024)
PANEL_LAUNCH_SHAPES = {
    None:       [(1, 0), (1, 0), (1, 0), (3, 0), (2, 0), (3, 0),     # plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (2, 0), (2, 0),     # not plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)],    # not plain, LayerNorm
    "first":    [(1, 0), (1, 0), (1, 0), (3, 0), (2, 0), (3, 0),     # plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (2, 0), (2, 0),     # not plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)],    # not plain, LayerNorm
    "first64":  [(1, 0), (1, 0), (1, 0), (3, 0), (2, 0), (3, 0),     # plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (2, 0), (2, 0),     # not plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)],    # not plain, LayerNorm
    "pipe":     [(1, 0), (1, 0), (1, 0), (3, 0), (2, 0), (3, 0),     # plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (2, 0), (2, 0),     # not plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)],    # not plain, LayerNorm
    "panel":    [(1, 0), (1, 0), (1, 0), (3, 0), (2, 0), (3, 0),     # plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (2, 0), (2, 0),     # not plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)],    # not plain, LayerNorm
    "panel64":  [(1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0),     # plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0),     # not plain
                 (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)],    # not plain, LayerNorm
    "panel128": [(2, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0),     # plain
                 (2, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0),     # not plain
                 (2, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0)],    # not plain, LayerNorm
    "panelr":   [(3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0),     # plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0),     # not plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0)],    # not plain, LayerNorm
    "panelr1":  [(3, 1), (3, 1), (3, 1), (3, 1), (3, 1), (3, 1),     # plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0),     # not plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0)],    # not plain, LayerNorm
    "panelr2":  [(3, 2), (3, 2), (3, 2), (3, 2), (3, 2), (3, 2),     # plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0),     # not plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0)],    # not plain, LayerNorm
    "panelr3":  [(3, 3), (3, 3), (3, 3), (3, 3), (3, 3), (3, 3),     # plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0),     # not plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0)],    # not plain, LayerNorm
    "panelr4":  [(3, 4), (3, 4), (3, 4), (3, 4), (3, 4), (3, 4),     # plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0),     # not plain
                 (3, 0), (3, 0), (3, 0), (3, 0), (3, 0), (3, 0)],    # not plain, LayerNorm
}


def test_panel_launch_shape_is_the_recorded_table():
    assert set(PANEL_LAUNCH_SHAPES) == set(modes.GEMM_KERNELS)
    for kern, want in PANEL_LAUNCH_SHAPES.items():
        got = [ops._panel_launch_shape(kern, M, N, 256, plain=plain, ln=ln)
               for plain, ln in ((True, False), (False, False), (False, True))
               for M in (64, 1 << 16, 1 << 17) for N in (256, 1024)]
        assert got == want, kern
        # ``linear_rows2`` passes neither ``plain`` nor ``ln``: the plain column
        assert [ops._panel_launch_shape(kern, M, N, 256) for M in (64, 1 << 16, 1 << 17) for N in (256, 1024)] == want[:6], kern
