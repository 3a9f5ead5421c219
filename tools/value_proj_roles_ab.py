"""A/B of the hoisted value projections by row-panel shape on the GPU box: today's shapes (128-row panels for the camera
values, 64-row for the BEV values) against the role-split panels (csrc/linear_roles.h) and its knobs, interleaved rounds
in one process, median and minimum of the per-round times; every output compared bit for bit with the first shape's.

    python tools/value_proj_roles_ab.py [--rounds 7] [--iters 10] [--modes split]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bevformer_amd import ops  # noqa: E402
from kbench import timeit  # noqa: E402

DEV = "cuda:0"
KERNELS = ("panel128", "panel64", "panelr", "panelr1", "panelr2", "panelr3", "panelr4")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--modes", default="split")
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    w = torch.randn(1536, 256, device=DEV, generator=g) * 0.05
    b = torch.randn(1536, device=DEV, generator=g)
    cam = torch.randn(184950, 256, device=DEV, generator=g)
    hist = torch.randn(40000, 256, device=DEV, generator=g)
    cur = torch.randn(40000, 256, device=DEV, generator=g)
    cases = [("sca_value_proj", lambda: ops.linear(cam, w, b, groups=6)),
             ("tsa_value_proj (rows2)", lambda: ops.linear_rows2(hist, cur, w, b, groups=6))]
    for mode in args.modes.split(","):
        ops.set_gemm_mode(mode)
        print(f"mode {mode}: {'shape':24s}" + "".join(f"{k:>18s}" for k in KERNELS) + "   (us: median / min over rounds)")
        for name, fn in cases:
            ts = {k: [] for k in KERNELS}
            ref = None
            same = True
            with torch.no_grad():
                for r in range(args.rounds):
                    for k in KERNELS:
                        ops.set_gemm_kernel(k)
                        if r == 0:
                            y = fn()
                            ref = y if ref is None else ref
                            same = same and torch.equal(y, ref)
                            del y
                        ts[k].append(timeit(fn, args.iters)[0] * 1e6)
            ops.set_gemm_kernel(None)
            print(f"   {name:24s}" + "".join(f"{med(ts[k]):9.1f} /{min(ts[k]):7.1f}" for k in KERNELS)
                  + f"   bit-identical: {same}")


if __name__ == "__main__":
    main()
