"""Which row-panel shape a launch asks for (``ops._panel_shape``, the ``desc.reserved[2]`` the library receives) and the
agreement of that rule with the library's own default for shape 0 (csrc/bevmsda_linear.hip)."""
import os
import re

from bevformer_amd import ops
from bevformer_amd.ops.gemm import _panel_shape


def test_hoisted_value_projections_take_the_role_split_panels():
    assert _panel_shape("", 184950, 1536, 256) == 3          # camera values
    assert _panel_shape("", 80000, 1536, 256) == 3           # BEV values (rows2)
    assert _panel_shape("", 40000, 1536, 256) == 1           # a tile's rows: today's 64-row panels
    assert _panel_shape("", 184950, 1536, 512, plain=False) == 2
    assert _panel_shape("", 184950, 256, 256, plain=False, ln=True) == 1
    assert _panel_shape("", 184950, 768, 256) == 2           # N below panel_min_cols
    assert _panel_shape("panel128", 184950, 1536, 256) == 2
    assert _panel_shape("panel64", 80000, 1536, 256) == 1
    assert _panel_shape("panelr", 5000, 256, 256) == 3


def test_role_split_thresholds_match_the_library():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bevformer_amd", "csrc", "bevmsda_linear.hip")).read()
    assert int(re.search(r"kPanelRolesMinRows\s*=\s*(\d+)", src).group(1)) == ops.KERNEL_SELECTION["panel_roles_rows"][0]
    assert int(re.search(r"kPanelRolesMinCols\s*=\s*(\d+)", src).group(1)) == ops.KERNEL_SELECTION["panel_min_cols"][0]
