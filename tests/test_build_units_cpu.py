"""The translation units of libbevmsda.so (bevformer_amd/build.py): what each was compiled from, as the compiler itself
listed it next to the object, and the staleness rule that reads those lists (no GPU)."""
import os

import pytest

from bevformer_amd import build


@pytest.fixture(scope="module")
def deps():
    """unit -> the base names of the files it was compiled from"""
    build.build_library()
    out = {}
    for src in build.sources():
        files = build.dependencies(src)
        assert files, f"no dependency list next to the object of {src}"
        assert files[0] == os.path.join(build.CSRC, src)
        out[src] = {os.path.basename(f) for f in files}
    return out


def test_a_unit_is_compiled_from_the_headers_of_its_own_kernel_family(deps):
    optim = deps["bevmsda_optim.hip"]
    assert {"optim.h", "scalar_ops.h", "capi_checks.h", "bevmsda.h"} <= optim
    assert not optim & {"linear_chain.h", "conv_mfma.h", "msda_d32.h"}
    assert {"conv_mfma.h", "linear_mfma.h"} <= deps["bevmsda_conv.hip"]
    assert "bevmsda_capi.hip" in deps["bevmsda_capi_backward.hip"]
    assert "bevmsda.h" in deps["bevmsda_plan.hip"]


def test_every_header_is_compiled_into_some_unit_and_the_shared_checks_hold_no_kernel(deps):
    headers = {f for f in os.listdir(build.CSRC) if f.endswith(".h")}
    used = set().union(*deps.values())
    assert headers <= used, f"headers no unit includes: {sorted(headers - used)}"
    assert "__global__" not in open(os.path.join(build.CSRC, "capi_checks.h")).read()
    # the one kernel that is no template and sat in a shared header: its host stub may exist once in the library
    assert [u for u, d in deps.items() if "linear_pack_multi.h" in d] == ["bevmsda_linear.hip"]


def test_the_dependency_list_follows_the_tree_when_it_is_copied_or_moved(tmp_path):
    """The repository's own files are recorded relative to csrc/, whatever path the compiler was given."""
    d = tmp_path / "unit.d"
    header = os.path.join(build.CSRC, "..", "..", "include", "bevmsda.h")
    d.write_text(f"unit.o: {os.path.join(build.CSRC, 'a.hip')} \\\n  {header} \\\n  /opt/x\\ y/z.h optim.h\n")
    build._keep_relative(str(d))
    assert build._prerequisites(str(d)) == ["a.hip", os.path.join("..", "..", "include", "bevmsda.h"), "/opt/x y/z.h",
                                            "optim.h"]


def test_staleness_is_decided_per_unit_from_its_own_dependencies():
    units = {"a.hip": ("a.o", ["a.hip", "shared.h", "a_only.h"]),
             "b.hip": ("b.o", ["b.hip", "shared.h"]),
             "c.hip": ("c.o", ["c.hip", "b.hip"])}
    fresh = {"a.hip": 1.0, "b.hip": 1.0, "c.hip": 1.0, "shared.h": 2.0, "a_only.h": 2.0, "a.o": 5.0, "b.o": 5.0, "c.o": 5.0}

    def stale(changed=()):
        return sorted(build._stale_objects(units, {**fresh, **dict(changed)}.get))

    assert stale() == []
    assert stale({"a_only.h": 6.0}) == ["a.hip"]                     # a header of one unit: that unit alone
    assert stale({"shared.h": 6.0}) == ["a.hip", "b.hip"]
    assert stale({"b.hip": 6.0}) == ["b.hip", "c.hip"]               # a source that another source includes
    assert stale({"a.o": None}) == ["a.hip"]                         # no object
    assert stale({"a_only.h": None}) == ["a.hip"]                    # a dependency that is gone
    assert stale({"a_only.h": 5.0}) == []                            # as old as the object: not newer
    units["b.hip"] = ("b.o", None)                                   # no dependency list (an object of an older build)
    assert stale() == ["b.hip"]


def test_the_compile_pool_is_capped():
    assert build.MAX_WORKERS == 16
