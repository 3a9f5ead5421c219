"""The bevformerv2 backbone — ResNet-50, caffe style, nothing frozen, every BatchNorm in ``train()`` mode (batch statistics,
trainable affine parameters: ``norm_eval=False``, ``SyncBN`` on one rank) —, forward + backward under ``modes.backbone_train`` +
``modes.bn_train`` against the module path, 6 cameras at the config's image size (1600 x 640 after its crop).  Shapes: the whole
backbone (``v2``) and one steady block (no downsample) of each stage at that size — ``stage1`` = 256 -> 64 -> 256 at 160 x 400,
``stage2`` = 512 -> 128 -> 512 at 80 x 200, ``stage3`` = 1024 -> 256 -> 1024 at 40 x 100, ``stage4`` = 2048 -> 512 -> 2048 at
20 x 50.  Arms, each ONE forward + backward captured as a HIP graph on one stream:

    module        the module path at the same commit (every switch off)
    fast_split    modes.backbone_train + modes.bn_train, GEMM mode split
    fast_bf16     ... GEMM mode bf16

and, per block, the BatchNorm launches of its widest norm on their own (``bn3_stats``, ``bn3_apply`` with the residual and the ReLU,
``bn3_bwd`` = the backward's reduce + apply with the identity's gradient written) with their algorithmic bytes.  One fresh child process per shape with its own timeout; interleaved windows (device events around
many replays), so a drift of the machine shows as spread between the windows of ONE arm.  Speed is reported, not gated; the switch
stays off by default.  Needs a GPU.

    python tools/bn_train_ab.py [--windows 4] [--steps 10] [--net-steps 2] [--shapes ...] [--out profiles/r22/bn_train_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 400
N_IMG = 6
H_IMG, W_IMG = 640, 1600
# name -> (H, W, inplanes, planes)
BLOCKS = {"stage1": (160, 400, 256, 64), "stage2": (80, 200, 512, 128), "stage3": (40, 100, 1024, 256), "stage4": (20, 50, 2048, 512)}
NET = dict(depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=-1, norm_cfg=dict(type="SyncBN"), norm_eval=False, style="caffe")
ARMS = ("module", "fast_split", "fast_bf16")


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _randomize(module, g):
    import torch
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5), m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
            w = getattr(m, "weight", None)
            if torch.is_tensor(w) and w.dim() == 4:
                w.copy_(torch.randn(w.shape, generator=g) / w[0].numel() ** 0.5)
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
        H, W, inplanes, planes = BLOCKS[name]
        mod = Bottleneck(inplanes, planes, style="caffe", norm_cfg=dict(type="SyncBN"))
        x = torch.randn(N_IMG, inplanes, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
    else:
        mod = ResNet(**NET)
        x = torch.randn(N_IMG, 3, H_IMG, W_IMG, generator=g).to(dev)
    mod = _randomize(mod, g).to(dev).train()
    params = [p for p in mod.parameters() if p.requires_grad]
    wrt = ([x] if is_block else []) + params
    with torch.no_grad():
        probe = mod(x)
    gos = [torch.randn(o.shape, generator=g).to(dev) for o in ([probe] if is_block else probe)]

    def step(**modes):
        def fn():
            with ops.using(**modes):
                out = mod(x)
                outs = [out] if is_block else list(out)
                return torch.autograd.grad(sum((o * go).sum() for o, go in zip(outs, gos)), wrt)
        return fn

    off = dict(backbone_train=False, bn_train=False, backbone_fused=False, stem_fused=False, dcn_fused=False)
    fns = {"module": step(gemm="split", **off), "fast_split": step(gemm="split", backbone_train=True, bn_train=True),
           "fast_bf16": step(gemm="bf16", backbone_train=True, bn_train=True)}
    arms, nbytes = list(ARMS), {}
    if is_block:        # the four BatchNorm launches of bn3 on their own: inputs made once, outside the graphs
        M, C = N_IMG * H * W, 4 * planes
        z, go, res = (torch.randn(M, C, generator=g).to(dev) for _ in range(3))
        with torch.no_grad():
            mean, var = ops.bn_stats_rows(z)
            y = ops.bn_apply_rows(z, mean, var, mod.bn3, relu=True, res=res)
        parts = {"stats": lambda: ops.bn_stats_rows(z, mod.bn3),
                 "apply": lambda: ops.bn_apply_rows(z, mean, var, mod.bn3, relu=True, res=res),
                 "bwd": lambda: ops.bn_rows_backward(go, y, z, mean, var, mod.bn3, relu=True, gy_out=True)}
        for part, call in parts.items():
            rec = []
            ops.set_gemm_timer(lambda tag, fl, nb: (rec.append(nb), _Null())[1])
            try:
                with torch.no_grad():
                    assert call() is not None, part
            finally:
                ops.set_gemm_timer(None)

            def fn(call=call):
                with torch.no_grad():
                    return call()
            arm = "bn3_" + part
            fns[arm], nbytes[arm] = fn, sum(rec)
            arms.append(arm)

    def capture(fn):
        for _ in range(2):
            assert fn() is not None
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

    out = dict(shape=name, arms=arms, nbytes=nbytes)
    blocks = [m for m in mod.modules() if isinstance(m, Bottleneck)]
    with ops.using(gemm="split", backbone_train=True):
        out["covered_without"] = sum(ops.bottleneck_train_reject(b) is None for b in blocks)
        with ops.using(bn_train=True):
            out["covered"] = sum(ops.bottleneck_train_reject(b) is None for b in blocks)
    out["blocks"] = len(blocks)
    launches = []
    ops.set_gemm_timer(lambda tag, fl, nb: (launches.append((tag, fl, nb)), _Null())[1])
    try:
        fns["fast_split"]()
    finally:
        ops.set_gemm_timer(None)
    out["launches"] = len(launches)
    out["bn_launches"] = sum(1 for l in launches if l[0].endswith(("_stats", "_apply", "_reduce")))
    graphs = {arm: capture(fns[arm]) for arm in arms}
    times = {arm: [] for arm in arms}
    for _ in range(windows):
        for arm in arms:
            times[arm].append(timed(graphs[arm][0], steps))
    out["us"] = times
    ref = graphs["module"][1]
    rel = lambda a, b: float(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item())
    for mode in ("split", "bf16"):
        out["diff_" + mode] = max(rel(a, b) for a, b in zip(graphs["fast_" + mode][1], ref))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--net-steps", type=int, default=2, help="replays per window for the whole backbone")
    ap.add_argument("--shapes", default=",".join(list(BLOCKS) + ["v2"]))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "bn_train_ab.txt"))
    ap.add_argument("--child", metavar="SHAPE")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.windows, args.steps)
    lines = ["ResNet-50 bottlenecks with BatchNorms in train() mode (batch statistics, trainable affine parameters: the bevformerv2 backbone), "
             f"{N_IMG} cameras at {W_IMG} x {H_IMG}, ONE forward + backward: the module path (torch convolution + batch_norm + ReLU and their "
             "autograd) vs modes.backbone_train + modes.bn_train (one autograd Function per block: raw convolution, statistics, apply per "
             "convolution forward; reduce, apply, weight gradient, input gradient per convolution backward) in split and in bf16; every arm a "
             "replayed HIP graph",
             f"per shape: one fresh process, {args.windows} interleaved windows of {args.steps} replays per arm ({args.net_steps} for the "
             "whole backbone), us per step; MB per launch are algorithmic bytes as the launches report them",
             ""]
    for name in args.shapes.split(","):
        env = {k: v for k, v in os.environ.items() if not k.startswith("BEVMSDA_")}
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
            H, W, inplanes, planes = BLOCKS[name]
            what = f"{N_IMG} x {H} x {W}, {inplanes} -> {planes} -> {4 * planes}"
        else:
            what = f"{N_IMG} x 3 x {H_IMG} x {W_IMG}, ResNet-50 caffe, SyncBN, norm_eval=False"
        lines.append(f"{name}: {what}: {r['covered']} of {r['blocks']} blocks covered ({r['covered_without']} without bn_train), "
                     f"{r['launches']} launches per step of which {r['bn_launches']} BatchNorm")
        med = {arm: statistics.median(r["us"][arm]) for arm in r["arms"]}
        for arm in r["arms"]:
            v = r["us"][arm]
            tail = f"  MB {r['nbytes'][arm] / 1e6:8.2f}  GB/s {r['nbytes'][arm] / med[arm] / 1e3:7.1f}" if arm in r["nbytes"] else ""
            lines.append(f"{name:8s} {arm:16s}: median {med[arm]:10.1f}  min {min(v):10.1f}  max {max(v):10.1f}  spread {max(v) - min(v):8.1f}{tail}")
        for mode in ("split", "bf16"):
            f = med["fast_" + mode]
            verdict = "the fast path LOSES" if f > med["module"] else "the fast path wins"
            lines.append(f"{name:8s} {mode:5s}: module / fast = x{med['module'] / f:.2f} ({verdict})")
        lines.append(f"{name:8s} max |fast - module| / max |module|, worst gradient: split {r['diff_split']:.3e}, bf16 {r['diff_bf16']:.3e} "
                     "(random inputs: ReLU inputs within the forward's rounding of zero take the other side)")
        lines.append("")
        print("\n".join(lines[first:]), flush=True)
        text = "\n".join(lines) + "\n"          # (written after every child: a later child's trouble keeps what was measured)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
