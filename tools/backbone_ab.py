"""The backbone's bottlenecks under ``modes.backbone_fused`` against the module path, 6 cameras, at the sizes the reference
configs run.  Shapes: one steady block (no downsample) of each stage of the base backbone at 928 x 1600 — ``stage1`` = 256 -> 64 ->
256 at 232 x 400, ``stage2`` = 512 -> 128 -> 512 at 116 x 200, ``stage3`` = 1024 -> 256 -> 1024 at 58 x 100 and ``stage4`` = 2048 -> 512
-> 2048 at 29 x 50, the last two with a DCNv2 ``conv2`` —, the whole base backbone (``base``: ResNet-101, caffe style, DCNv2 in
stages 3 and 4) and the whole tiny backbone (``tiny``: ResNet-50, pytorch style, 480 x 800).  Arms, each captured as a HIP graph:

    module_nchw   the module path (``modes.backbone_fused`` and ``modes.dcn_fused`` off) on a contiguous NCHW input
    module_cl     the module path on a ``torch.channels_last`` input
    fast_split    modes.backbone_fused, GEMM mode split (a block: on a channels-last input, as inside a stage; a backbone: the
                  image as it comes, NCHW — the stem is torch's)
    fast_bf16     ... GEMM mode bf16 (a pack's offset launch stays in split precision)

and, per block, every launch of the fast path on its own in both modes (``conv1``, ``conv2`` or ``offsets`` + ``deform``,
``conv3`` with the residual): what the half-used column tile of the 64-wide stage-1 ``conv1`` / ``conv2`` costs shows there as
TFLOP/s against the same launches of the wider stages.

One fresh child process per shape with its own timeout.  A child times the arms in interleaved windows (device events around
many replays), so that a drift of the box shows as spread between the windows of ONE arm instead of as a difference between
arms; it also compares the outputs.  Speed is reported, not gated, and the switch stays off by default whatever comes out.
GPU box.

    python tools/backbone_ab.py [--windows 4] [--steps 10] [--net-steps 2] [--out profiles/r17/backbone_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 400
N_IMG = 6
DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)
# name -> (H, W, inplanes, planes, dcn)
BLOCKS = {"stage1": (232, 400, 256, 64, False), "stage2": (116, 200, 512, 128, False), "stage3": (58, 100, 1024, 256, True),
          "stage4": (29, 50, 2048, 512, True)}
# name -> (H, W, ResNet arguments)
NETS = {"base": (928, 1600, dict(depth=101, style="caffe", out_indices=(1, 2, 3), dcn=DCN, stage_with_dcn=(False, False, True, True))),
        "tiny": (480, 800, dict(depth=50, style="pytorch", out_indices=(3,)))}
ARMS = ("module_nchw", "module_cl", "fast_split", "fast_bf16")


def _randomize(module, g):
    """A trained network's regime, not the initialisation: affine norms with running statistics, offsets of about a pixel."""
    import torch
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5), m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.2), m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
            if hasattr(m, "conv_offset"):
                w = m.conv_offset.weight
                w.copy_(torch.randn(w.shape, generator=g) / (9 * w.shape[1]) ** 0.5)
                m.conv_offset.bias.copy_(torch.randn(27, generator=g) * 0.5)
    return module


def child(name, windows, steps):
    import torch

    sys.path.insert(0, ROOT)
    from bevformer_amd import ops
    from bevformer_amd.modules import Bottleneck, ResNet

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    is_block = name in BLOCKS
    if is_block:
        H, W, inplanes, planes, dcn = BLOCKS[name]
        mod = Bottleneck(inplanes, planes, style="caffe", dcn=DCN if dcn else None)
        with torch.no_grad():
            for m in mod.modules():
                w = getattr(m, "weight", None)
                if torch.is_tensor(w) and w.dim() == 4:
                    w.copy_(torch.randn(w.shape, generator=g) / w[0].numel() ** 0.5)
        x = torch.randn(N_IMG, inplanes, H, W, generator=g).to(dev)
    else:
        H, W, kw = NETS[name]
        mod = ResNet(**kw)
        x = torch.randn(N_IMG, 3, H, W, generator=g).to(dev)
    mod = _randomize(mod, g).to(dev).eval()
    x_cl = x.contiguous(memory_format=torch.channels_last)
    first = (lambda o: o) if is_block else (lambda o: o[-1])

    def module(inp):
        def fn():
            with ops.using(gemm="split", backbone_fused=False, dcn_fused=False):
                return first(mod(inp))
        return fn

    def fast(mode):
        def fn():
            with ops.using(gemm=mode, backbone_fused=True):
                return first(mod(x_cl if is_block else x))
        return fn

    fns = {"module_nchw": module(x), "module_cl": module(x_cl), "fast_split": fast("split"), "fast_bf16": fast("bf16")}
    arms = list(ARMS)
    flops = {}
    if is_block:        # every launch of the fast path on its own: its inputs are made once, outside the graphs
        rows = ops.rows_of_map(x_cl)
        hw = (H, W)
        with torch.no_grad(), ops.using(gemm="split"):
            o1 = ops.conv_bn_rows(rows, N_IMG, hw, mod.conv1.weight, mod.bn1, relu=True)
            if dcn:
                offs = ops.dcn_offsets(o1, N_IMG, hw, mod.conv2.conv_offset, 1)
                o2 = ops.deform_conv_rows(o1, N_IMG, hw, offs, mod.conv2.weight, bn=mod.bn2, relu=True)
            else:
                o2 = ops.conv_bn_rows(o1, N_IMG, hw, mod.conv2.weight, mod.bn2, relu=True)
        M = N_IMG * H * W
        parts = {"conv1": (lambda: ops.conv_bn_rows(rows, N_IMG, hw, mod.conv1.weight, mod.bn1, relu=True), 2.0 * M * inplanes * planes),
                 "conv3": (lambda: ops.conv_bn_rows(o2, N_IMG, hw, mod.conv3.weight, mod.bn3, relu=True, res=rows), 2.0 * M * inplanes * planes)}
        if dcn:
            parts["offsets"] = (lambda: ops.dcn_offsets(o1, N_IMG, hw, mod.conv2.conv_offset, 1), 2.0 * M * 32 * 9 * planes)
            parts["deform"] = (lambda: ops.deform_conv_rows(o1, N_IMG, hw, offs, mod.conv2.weight, bn=mod.bn2, relu=True), 2.0 * M * 9 * planes * planes)
        else:
            parts["conv2"] = (lambda: ops.conv_bn_rows(o1, N_IMG, hw, mod.conv2.weight, mod.bn2, relu=True), 2.0 * M * 9 * planes * planes)
        for part in ("conv1", "conv2", "offsets", "deform", "conv3"):
            if part not in parts:
                continue
            for mode in ("split", "bf16"):
                def fn(call=parts[part][0], mode=mode):
                    with ops.using(gemm=mode):
                        return call()
                fns[f"{part}_{mode}"] = fn
                flops[f"{part}_{mode}"] = parts[part][1]
                arms.append(f"{part}_{mode}")

    def capture(fn):
        for _ in range(2):
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

    out = dict(shape=name, arms=arms, flops=flops)
    with torch.no_grad():
        blocks = [m for m in mod.modules() if isinstance(m, Bottleneck)]
        with ops.using(gemm="split"):
            out["covered"] = sum(ops.bottleneck_reject(b) is None for b in blocks)
        out["blocks"] = len(blocks)
        launches = []
        ops.set_gemm_timer(lambda tag, fl, nb: (launches.append((tag, fl, nb)), _Null())[1])
        try:
            fns["fast_split"]()
        finally:
            ops.set_gemm_timer(None)
        out["launches"] = len(launches)
        out["gflop"] = sum(l[1] for l in launches) / 1e9
        out["mbytes"] = sum(l[2] for l in launches) / 1e6
        graphs = {arm: capture(fns[arm]) for arm in arms}
        times = {arm: [] for arm in arms}
        for _ in range(windows):
            for arm in arms:
                times[arm].append(timed(graphs[arm][0], steps))
        out["us"] = times
        ref = graphs["module_nchw"][1]
        out["out_abs_max"] = float(ref.abs().max().item())
        out["diff_cl"] = float((graphs["module_cl"][1] - ref).abs().max().item())
        out["diff_split"] = float((graphs["fast_split"][1] - ref).abs().max().item())
        out["diff_bf16"] = float((graphs["fast_bf16"][1] - ref).abs().max().item())
    print("RESULT " + json.dumps(out), flush=True)


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--net-steps", type=int, default=2, help="replays per window for the whole backbones")
    ap.add_argument("--shapes", default=",".join(list(BLOCKS) + list(NETS)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "backbone_ab.txt"))
    ap.add_argument("--child", metavar="SHAPE")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.windows, args.steps)
    lines = ["ResNet bottlenecks, 6 cameras: the module path (torch convolution + BatchNorm + ReLU launches, DCNv2 as torch gathers + "
             "einsum) on an NCHW and on a channels-last input vs modes.backbone_fused (conv + BatchNorm + residual + ReLU per launch "
             "on channel-last rows) in split and in bf16; every arm a replayed HIP graph",
             f"per shape: one fresh process, {args.windows} interleaved windows of {args.steps} replays per arm ({args.net_steps} for a "
             "whole backbone), us per step; GFLOP and MB are the fast path's algorithmic figures as its launches report them (the "
             "stem and the max pooling, on torch in every arm, are not counted); TFLOP/s = those FLOPs over the WHOLE step's time",
             ""]
    for name in args.shapes.split(","):
        env = {k: v for k, v in os.environ.items() if k not in ("BEVMSDA_BACKBONE_FUSED", "BEVMSDA_DCN_FUSED", "BEVMSDA_GEMM")}
        steps = args.steps if name in BLOCKS else args.net_steps
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--windows", str(args.windows),
                                "--steps", str(steps)], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            print(f"{name}: timed out after {CHILD_TIMEOUT} s — stopping", flush=True)
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{name}: exit code {p.returncode} — stopping\n{p.stderr[-2000:]}", flush=True)
            return 1
        r = json.loads(line[-1][7:])
        first = len(lines)
        if name in BLOCKS:
            H, W, inplanes, planes, dcn = BLOCKS[name]
            what = f"{N_IMG} x {H} x {W}, {inplanes} -> {planes} -> {inplanes}" + (", DCNv2 conv2" if dcn else "")
        else:
            H, W, kw = NETS[name]
            what = f"{N_IMG} x 3 x {H} x {W}, ResNet-{kw['depth']} {kw['style']}"
        lines.append(f"{name}: {what}: {r['covered']} of {r['blocks']} blocks covered, {r['launches']} launches, {r['gflop']:.2f} GFLOP, "
                     f"{r['mbytes']:.1f} MB algorithmic")
        med = {arm: statistics.median(r["us"][arm]) for arm in r["arms"]}
        for arm in r["arms"]:
            v = r["us"][arm]
            gf = r["flops"].get(arm, r["gflop"] * 1e9) / 1e9
            lines.append(f"{name:6s} {arm:13s}: median {med[arm]:10.1f}  min {min(v):10.1f}  max {max(v):10.1f}  "
                         f"spread {max(v) - min(v):8.1f}  TFLOP/s {gf / med[arm] * 1e3:6.1f}")
        spread = max(max(v) - min(v) for v in r["us"].values())
        best = min(med["module_nchw"], med["module_cl"])
        for mode in ("split", "bf16"):
            f = med["fast_" + mode]
            verdict = "the fast path LOSES" if f > best else "the fast path wins"
            lines.append(f"{name:6s} {mode:5s}: module_nchw / fast = x{med['module_nchw'] / f:.2f}, module_cl / fast = x{med['module_cl'] / f:.2f} "
                         f"({verdict} against the better module arm)")
        if name in BLOCKS:
            for mode in ("split", "bf16"):
                parts = [a for a in r["arms"] if a.endswith("_" + mode) and a not in ARMS]
                lines.append(f"{name:6s} {mode:5s}: launches alone " + " + ".join(f"{a.rsplit('_', 1)[0]} {med[a]:.1f}" for a in parts)
                             + f" = {sum(med[a] for a in parts):.1f} us against the block's {med['fast_' + mode]:.1f} us")
        lines.append(f"{name:6s} largest spread between windows of one arm {spread:.1f} us; outputs: max |module_cl - module_nchw| "
                     f"{r['diff_cl']:.3e}, max |fast - module_nchw| split {r['diff_split']:.3e}, bf16 {r['diff_bf16']:.3e} at max |output| "
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
