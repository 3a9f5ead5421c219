"""The backbone's deformable convolution alone (conv2 + bn2 + ReLU of a stage-3 / stage-4 bottleneck of the reference's
ResNet-101) at the sizes the base config runs, 6 cameras at 928 x 1600: ``stage3`` = 256 -> 256 at 58 x 100, ``stage4`` = 512 -> 512
at 29 x 50; ``tiny`` = 512 -> 512 at 15 x 25 (the last stage at the tiny config's image size).  Arms, each captured as a HIP graph:

    module        the module path: ModulatedDeformConv2dPack.forward_torch (torch gathers + einsum) + BatchNorm + ReLU, NCHW
    fast_split    modes.dcn_fused: ops.dcn on a channels-last input, GEMM mode split (offset launch + deformable launch)
    fast_bf16     ... GEMM mode bf16 (the offset launch stays in split precision)
    offsets       the offset launch alone (ops.dcn_offsets)
    floor_split   ops.conv_rows at the same 3 x 3 shape, split: the plain convolution without the gather — the floor
    floor_bf16    ... bf16

One fresh child process per shape with its own timeout.  A child times the arms in interleaved windows (device events around
many replays), so that a drift of the box shows as spread between the windows of ONE arm instead of as a difference between
arms; it also compares the outputs.  Speed is reported, not gated: no vendor DCN exists here to compare against, and the switch
stays off by default whatever comes out.  GPU box.

    python tools/dcn_ab.py [--windows 4] [--steps 10] [--out profiles/r15/dcn_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
# name -> (n_img, H, W, channels)
SHAPES = {"stage3": (6, 58, 100, 256), "stage4": (6, 29, 50, 512), "tiny": (6, 15, 25, 512)}
ARMS = ("module", "fast_split", "fast_bf16", "offsets", "floor_split", "floor_bf16")


def child(name, windows, steps):
    import torch

    sys.path.insert(0, ROOT)
    from bevformer_amd import ops
    from bevformer_amd.modules import ModulatedDeformConv2dPack

    dev = torch.device("cuda:0")
    n_img, H, W, C = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    pack = ModulatedDeformConv2dPack(C, C, 3, padding=1, bias=False)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():       # offsets of about a pixel, masks around 1/2: a trained pack's regime, not the zero initialisation
        pack.weight.copy_(torch.randn(pack.weight.shape, generator=g) / (9 * C) ** 0.5)
        pack.conv_offset.weight.copy_(torch.randn(pack.conv_offset.weight.shape, generator=g) / (9 * C) ** 0.5)
        pack.conv_offset.bias.copy_(torch.randn(27, generator=g) * 0.5)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.2), bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    pack, bn = pack.to(dev).eval(), bn.to(dev).eval()
    x = torch.randn(n_img, C, H, W, generator=g).to(dev)
    x_cl = x.contiguous(memory_format=torch.channels_last)
    rows = ops.rows_of_map(x_cl)

    def fast(mode):
        def fn():
            with ops.using(gemm=mode):
                return ops.dcn(pack, x_cl, bn, relu=True)
        return fn

    def floor(mode):
        def fn():
            with ops.using(gemm=mode):
                return ops.conv_rows(rows, n_img, (H, W), pack.weight, None)
        return fn

    fns = {"module": lambda: torch.relu(bn(pack.forward_torch(x))), "fast_split": fast("split"), "fast_bf16": fast("bf16"),
           "offsets": lambda: ops.dcn_offsets(rows, n_img, (H, W), pack.conv_offset, 1),
           "floor_split": floor("split"), "floor_bf16": floor("bf16")}

    def capture(fn):
        for _ in range(3):
            assert fn() is not None, "the fast path does not cover this shape"
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        return graph, out

    def timed(graph, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            graph.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / n          # us per step

    M = n_img * H * W
    out = dict(shape=name, gflop=2.0 * M * C * 9 * C / 1e9, offsets_gflop=2.0 * M * 32 * 9 * C / 1e9,
               mbytes=4.0 * (M * C + 9 * C * C + 32 * M + M * C) / 1e6)
    with torch.no_grad(), ops.using(gemm="split"):
        assert ops.dcn_reject(pack, x_cl, bn) is None
        graphs = {arm: capture(fns[arm]) for arm in ARMS}
        times = {arm: [] for arm in ARMS}
        for _ in range(windows):
            for arm in ARMS:
                times[arm].append(timed(graphs[arm][0], steps))
        out["us"] = times
        ref = graphs["module"][1]
        out["out_abs_max"] = float(ref.abs().max().item())
        out["diff_split"] = float((graphs["fast_split"][1] - ref).abs().max().item())
        out["diff_bf16"] = float((graphs["fast_bf16"][1] - ref).abs().max().item())
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "dcn_ab.txt"))
    ap.add_argument("--child", metavar="SHAPE")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.windows, args.steps)
    lines = ["DCNv2 conv2 + bn2 + ReLU alone, 6 cameras: module path (torch gathers + einsum, NCHW) vs modes.dcn_fused (offset launch + "
             "deformable MFMA launch on channel-last rows) vs ops.conv_rows at the same 3 x 3 shape (the floor: no gather); every "
             "arm a replayed HIP graph",
             f"per shape: one fresh process, {args.windows} interleaved windows of {args.steps} replays per arm (us per step); TFLOP/s = "
             "the 3 x 3 convolution's FLOPs from the shape over the WHOLE step's time (for the fast arms that includes the offset "
             "launch; end to end, not a kernel's share of peak)", ""]
    for name in SHAPES:
        env = {k: v for k, v in os.environ.items() if k not in ("BEVMSDA_DCN_FUSED", "BEVMSDA_GEMM")}
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--windows", str(args.windows),
                                "--steps", str(args.steps)], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            print(f"{name}: timed out after {CHILD_TIMEOUT} s — stopping", flush=True)
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{name}: exit code {p.returncode} — stopping\n{p.stderr[-2000:]}", flush=True)
            return 1
        r = json.loads(line[-1][7:])
        n_img, H, W, C = SHAPES[name]
        first = len(lines)
        lines.append(f"{name}: {n_img} x {H} x {W}, {C} -> {C}: {r['gflop']:.2f} GFLOP (+ {r['offsets_gflop']:.2f} for the offsets), "
                     f"{r['mbytes']:.1f} MB algorithmic")
        for arm in ARMS:
            v = r["us"][arm]
            gf = r["offsets_gflop"] if arm == "offsets" else r["gflop"]
            lines.append(f"{name:6s} {arm:11s}: median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}  "
                         f"spread {max(v) - min(v):7.1f}  TFLOP/s {gf / statistics.median(v) * 1e3:6.1f}")
        med = {arm: statistics.median(r["us"][arm]) for arm in ARMS}
        spread = max(max(v) - min(v) for v in r["us"].values())
        for mode in ("split", "bf16"):
            lines.append(f"{name:6s} {mode:5s}: module / fast = x{med['module'] / med['fast_' + mode]:.2f}; fast - offsets = "
                         f"{med['fast_' + mode] - med['offsets']:.1f} us against the floor's {med['floor_' + mode]:.1f} us "
                         f"(x{(med['fast_' + mode] - med['offsets']) / med['floor_' + mode]:.2f}: what the gather costs); largest spread "
                         f"between windows of one arm {spread:.1f} us")
        lines.append(f"{name:6s} outputs: max |fast - module| split {r['diff_split']:.3e}, bf16 {r['diff_bf16']:.3e} at max |output| "
                     f"{r['out_abs_max']:.3f}")
        lines.append("")
        print("\n".join(lines[first:]), flush=True)
        text = "\n".join(lines) + "\n"          # (written after every child: a later child's trouble keeps what was measured)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
