"""No GPU: the four optimizer entry points validate every argument before any launch and answer a bad call with a code of
``bevmsda_error_string``'s table (include/bevmsda.h).  Pointers are fake: no kernel runs.  The entry points were ADDED to ABI
version 6; the number did not move."""
import ctypes
import re

import pytest

from bevformer_amd import _lib, build

OK, NULLP, SHAPE, LARGE, MISAL, OPT = 0, -1, -2, -3, -4, -6
fake = ctypes.c_void_p(0x1000)
off4 = ctypes.c_void_p(0x1004)          # 4-byte aligned only
off2 = ctypes.c_void_p(0x1002)
NAMES = ("bevmsda_optim_job_blocks", "bevmsda_optim_workspace_bytes", "bevmsda_optim_grad_norm_f32", "bevmsda_optim_adamw_f32")


@pytest.fixture(scope="module")
def lib():
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def test_abi_version_and_the_symbols_are_bound():
    assert _lib.ABI_VERSION == 7
    header = open(build.PUBLIC_HEADER).read()
    assert re.search(r"#define BEVMSDA_ABI_VERSION 7\b", header)
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(r"\bint(64_t)? %s\(" % name, header), name
    assert "bevmsda_optim_job" in header and "bevmsda_optim_group" in header
    assert ctypes.sizeof(_lib.OptimJob) == 56 and ctypes.sizeof(_lib.OptimGroup) == 40


def test_sizes(lib):
    assert lib.bevmsda_optim_job_blocks(0) == 0 and lib.bevmsda_optim_job_blocks(1) == 1
    assert lib.bevmsda_optim_job_blocks(4096) == 1 and lib.bevmsda_optim_job_blocks(4097) == 2
    assert lib.bevmsda_optim_job_blocks(-5) == -1
    assert lib.bevmsda_optim_workspace_bytes(-1) == -1 and lib.bevmsda_optim_workspace_bytes(0) == 8
    assert lib.bevmsda_optim_workspace_bytes(1000) == 8000


def test_grad_norm_rejects_bad_arguments(lib):
    f = lib.bevmsda_optim_grad_norm_f32

    def call(jobs=fake, njobs=3, blocks=5, max_norm=35.0, flags=1, workspace=fake, scalars=fake):
        return f(jobs, njobs, blocks, max_norm, flags, workspace, scalars, None)
    assert call(njobs=-1) == SHAPE
    assert call(blocks=-1) == SHAPE
    assert call(blocks=1 << 30) == LARGE
    assert call(flags=4) == OPT
    assert call(flags=-1) == OPT
    assert call(max_norm=-1.0) == OPT
    assert call(max_norm=float("nan")) == OPT
    assert call(max_norm=-1.0, flags=2, njobs=0) == OK                   # (max_norm is not read without the clip bit)
    assert call(njobs=0) == OK
    assert call(njobs=0, jobs=None, workspace=None, scalars=None) == OK
    for n in ("jobs", "workspace", "scalars"):
        assert call(**{n: None}) == NULLP, n
    assert call(jobs=off4) == MISAL
    assert call(workspace=off4) == MISAL
    assert call(scalars=off2) == MISAL


def test_adamw_rejects_bad_arguments(lib):
    f = lib.bevmsda_optim_adamw_f32

    def call(jobs=fake, njobs=3, blocks=5, groups=fake, ngroups=2, scalars=fake):
        return f(jobs, njobs, blocks, groups, ngroups, scalars, None)
    assert call(njobs=-1) == SHAPE
    assert call(blocks=-1) == SHAPE
    assert call(ngroups=-1) == SHAPE
    assert call(blocks=1 << 30) == LARGE
    assert call(njobs=0) == OK
    assert call(njobs=0, jobs=None, groups=None, scalars=None) == OK
    for n in ("jobs", "groups", "scalars"):
        assert call(**{n: None}) == NULLP, n
    assert call(ngroups=0) == NULLP                                      # jobs without a group to read
    assert call(jobs=off4) == MISAL
    assert call(groups=off4) == MISAL
    assert call(scalars=off2) == MISAL
    assert call(blocks=0) == OK                                          # every job empty: nothing to update
