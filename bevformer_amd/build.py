"""Builds ``lib/libbevmsda.so`` (HIP kernels + C ABI) for gfx950 with hipcc.

The library is compiled in-tree so that it travels with the repo snapshot to
the GPU box; there is no JIT and no torch C++ extension involved — the shared
object has a plain C ABI (include/bevmsda.h) and is loaded with ctypes.
Every ``csrc/*.hip`` file is one translation unit; they are compiled in
parallel into ``lib/obj/*.o`` (only the stale ones) and linked into one
shared object.  A unit is stale when a file it was compiled from — the
compiler's own list, ``lib/obj/*.d`` — is newer than its object.  The list
names the repository's files relative to ``csrc/``, so a built tree can be
copied or moved and its objects stay current.
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
OBJ_DIR = os.path.join(LIB_DIR, "obj")
LIB_PATH = os.path.join(LIB_DIR, "libbevmsda.so")
PUBLIC_HEADER = os.path.join(HERE, "..", "include", "bevmsda.h")
ARCH = "gfx950"
FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         "-Wno-pass-failed"]


# per-source additions to FLAGS
EXTRA_FLAGS = {}
MAX_WORKERS = 16


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _obj(src):
    return os.path.join(OBJ_DIR, os.path.splitext(src)[0] + ".o")


def _dep(src):
    return os.path.join(OBJ_DIR, os.path.splitext(src)[0] + ".d")


def _prerequisites(path):
    """The right-hand side of the Makefile rule in ``path``, as the compiler or ``_keep_relative`` wrote it."""
    text = open(path).read()
    rule = text.replace("\\\n", " ").partition(":")[2].replace("\\ ", "\0").split()     # ("\ " = a blank inside a path)
    return [w.replace("\0", " ") for w in rule]


def _keep_relative(path):
    """Rewrite the rule in ``path`` with the repository's own files relative to ``csrc/`` (the compiler wrote them as
    it was given the source: absolute), so that the list still names this tree's files after the tree was copied,
    moved or reached by another path.  Files outside the repository (the toolchain's headers) stay absolute."""
    root = os.path.dirname(HERE) + os.sep
    words = [os.path.relpath(w, CSRC) if os.path.isabs(w) and os.path.normpath(w).startswith(root) else w
             for w in _prerequisites(path)]
    with open(path, "w") as f:
        f.write("unit.o: " + " \\\n  ".join(w.replace(" ", "\\ ") for w in words) + "\n")


def dependencies(src):
    """The files ``src`` was last compiled from (its own path first), as absolute paths, read from the Makefile rule
    next to the object; ``None`` when there is none."""
    try:
        rule = _prerequisites(_dep(src))
    except OSError:
        return None
    return [os.path.normpath(os.path.join(CSRC, w)) for w in rule]


def _mtime(path):
    try:
        return os.path.getmtime(path)
    except OSError:
        return None


def _stale_objects(units=None, mtime=_mtime):
    """The sources to compile.  ``units`` maps a source to ``(object, dependencies or None)`` and ``mtime`` a path to its
    modification time (``None``: no such file), so that the rule can be evaluated on a made-up tree: a unit is stale when
    its object or its dependency list is missing, or when a dependency is newer than the object or gone."""
    if units is None:
        units = {s: (_obj(s), dependencies(s)) for s in sources()}
    out = []
    for src, (obj, deps) in units.items():
        built = mtime(obj)
        if built is None or not deps or any(mtime(f) is None or mtime(f) > built for f in deps):
            out.append(src)
    return out


def is_stale():
    if _stale_objects():
        return True
    linked = _mtime(LIB_PATH)
    return linked is None or any(_mtime(_obj(s)) > linked for s in sources())


def build_library(force=False, verbose=False):
    """Compile every HIP source (stale ones only unless ``force``) and link one shared object.
    Returns its path."""
    if not force and not is_stale():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libbevmsda.so")
    os.makedirs(OBJ_DIR, exist_ok=True)
    todo = sources() if force else _stale_objects()

    def compile_one(src):
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-MD", "-MF", _dep(src) + ".tmp"]
        cmd += ["-c", os.path.join(CSRC, src), "-o", _obj(src) + ".tmp"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=CSRC)
        _keep_relative(_dep(src) + ".tmp")
        os.replace(_dep(src) + ".tmp", _dep(src))
        os.replace(_obj(src) + ".tmp", _obj(src))

    with ThreadPoolExecutor(max_workers=max(1, min(len(todo), MAX_WORKERS, os.cpu_count() or 1))) as ex:
        list(ex.map(compile_one, todo))
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB_PATH + ".tmp"]
    cmd += [_obj(s) for s in sources()]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    import sys
    print(build_library(force="--force" in sys.argv, verbose=True))
