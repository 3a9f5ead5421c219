"""Backbone forward + backward under ``modes.backbone_train`` against the module path, 6 cameras, frozen BatchNorms
(``norm_eval=True``, ``requires_grad=False`` norms, ``frozen_stages=1``) as the reference training configs set them.  Shapes: steady
blocks (no downsample) of the trainable stages with a plain ``conv2`` — ``stage2_base`` = 512 -> 128 -> 512 at 116 x 200 (base,
928 x 1600) and ``stage2`` / ``stage3`` / ``stage4`` of the tiny backbone at 480 x 800 (60 x 100, 30 x 50, 15 x 25) —, the first block of
tiny's stage 3 (``stage3_first``: stride 2 on ``conv2`` with a downsample: the strided input gradients), the whole tiny backbone
(``tiny``: ResNet-50, pytorch style) and the whole base backbone (``base``: ResNet-101, caffe style, DCNv2 in stages 3 and 4 — those
stay on the module path unless ``modes.dcn_train`` is on).  DCN blocks at the base shapes, caffe style (the stride on ``conv1``):
``dcn_stage3`` = 1024 -> 256 -> 1024 at 58 x 100, ``dcn_stage4`` = 2048 -> 512 -> 2048 at 29 x 50 and the strided first block of each
(``dcn_stage3_first`` from 116 x 200, ``dcn_stage4_first`` from 58 x 100, with a downsample).  Arms, each ONE forward + backward
captured as a HIP graph on one stream:

    module        the module path (every switch off)
    fast_split    modes.backbone_train, GEMM mode split (a DCN block: the module path — the commit before modes.dcn_train)
    fast_bf16     ... GEMM mode bf16
    dcn_split     modes.backbone_train + modes.dcn_train, GEMM mode split (shapes with a DCNv2 conv2 only)
    dcn_bf16      ... GEMM mode bf16

and, per block, every backward launch on its own in both modes (``mask``; per convolution ``<conv>_wgrad`` and ``<conv>_dgrad``; for a
DCN block ``dcn_dgrad`` — the deformable input + offset gradient, atomics into buffers that are not re-zeroed between replays —,
``dcn_wgrad`` and ``conv_offset``'s ``dcn_offset_wgrad`` / ``dcn_offset_dgrad``) with its algorithmic FLOPs and bytes as the launch
reports them.  The strided 3 x 3 input gradient is the plain gather form
(csrc/conv_bwd_rows.h): ``stage3_first``'s ``conv2_dgrad`` against ``stage3``'s shows what the staged zeros of the dead taps cost
per useful FLOP; the form that tiles one parity class is not built, so there is no second form to time.

One fresh child process per shape with its own timeout; interleaved windows (device events around many replays), so a drift of
the box shows as spread between the windows of ONE arm.  Speed is reported, not gated; the switch stays off by default.  GPU box.

    python tools/backbone_train_ab.py [--windows 4] [--steps 10] [--net-steps 2] [--shapes ...] [--out profiles/r19/backbone_train_ab.txt]
    python tools/backbone_train_ab.py --shapes dcn_stage3,dcn_stage4,dcn_stage3_first,dcn_stage4_first,base --out profiles/r20/dcn_train_ab.txt"""
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
FROZEN_BN = dict(type="BN", requires_grad=False)
# name -> (H, W, inplanes, planes, stride)
BLOCKS = {"stage2_base": (116, 200, 512, 128, 1), "stage2": (60, 100, 512, 128, 1), "stage3": (30, 50, 1024, 256, 1),
          "stage4": (15, 25, 2048, 512, 1), "stage3_first": (60, 100, 512, 256, 2)}
# DCN blocks (caffe style): name -> (H, W, inplanes, planes, stride)
DCN_BLOCKS = {"dcn_stage3": (58, 100, 1024, 256, 1), "dcn_stage4": (29, 50, 2048, 512, 1),
              "dcn_stage3_first": (116, 200, 512, 256, 2), "dcn_stage4_first": (58, 100, 1024, 512, 2)}
NET_KW = dict(frozen_stages=1, norm_eval=True, norm_cfg=FROZEN_BN)
# name -> (H, W, ResNet arguments)
NETS = {"tiny": (480, 800, dict(depth=50, style="pytorch", out_indices=(3,), **NET_KW)),
        "base": (928, 1600, dict(depth=101, style="caffe", out_indices=(1, 2, 3), dcn=DCN, stage_with_dcn=(False, False, True, True), **NET_KW))}
ARMS = ("module", "fast_split", "fast_bf16")
DCN_ARMS = ("dcn_split", "dcn_bf16")


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _randomize(module, g):
    """A trained network's regime, not the initialisation: affine norms with running statistics, offsets of about a pixel."""
    import torch
    with torch.no_grad():
        for name, m in module.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5), m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.2), m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
            w = getattr(m, "weight", None)
            if torch.is_tensor(w) and w.dim() == 4 and not name.endswith("conv_offset"):
                w.copy_(torch.randn(w.shape, generator=g) / w[0].numel() ** 0.5)
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
    is_dcn_block = name in DCN_BLOCKS
    is_block = name in BLOCKS or is_dcn_block
    if is_block:
        H, W, inplanes, planes, stride = (DCN_BLOCKS if is_dcn_block else BLOCKS)[name]
        ds = None
        if stride != 1 or inplanes != 4 * planes:
            ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(4 * planes))
            for p in ds[1].parameters():
                p.requires_grad = False
        mod = Bottleneck(inplanes, planes, stride=stride, style="caffe" if is_dcn_block else "pytorch", downsample=ds,
                         norm_cfg=FROZEN_BN, dcn=DCN if is_dcn_block else None)
        x = torch.randn(N_IMG, inplanes, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
    else:
        H, W, kw = NETS[name]
        mod = ResNet(**kw)
        x = torch.randn(N_IMG, 3, H, W, generator=g).to(dev)
    has_dcn = is_dcn_block or (not is_block and kw.get("dcn") is not None)
    mod = _randomize(mod, g).to(dev)
    mod = mod.eval() if is_block else mod.train()
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

    off = dict(backbone_train=False, backbone_fused=False, stem_fused=False, dcn_fused=False)
    fns = {"module": step(gemm="split", **off), "fast_split": step(gemm="split", backbone_train=True),
           "fast_bf16": step(gemm="bf16", backbone_train=True)}
    arms, flops, nbytes = list(ARMS), {}, {}
    if has_dcn:
        fns["dcn_split"] = step(gemm="split", backbone_train=True, dcn_train=True)
        fns["dcn_bf16"] = step(gemm="bf16", backbone_train=True, dcn_train=True)
        arms += list(DCN_ARMS)
    if is_block:        # every backward launch on its own: its inputs are made once, outside the graphs
        rows, hw = ops.rows_of_map(x.detach()), (H, W)
        with torch.no_grad(), ops.using(gemm="split"):
            o1, hw1, offs, o2, hw2 = ops.backbone._block_inner(ops, mod, rows, N_IMG, hw)
            go_rows = ops.rows_of_map(gos[0])
            gid = ops.conv_gz_rows(go_rows, ops.rows_of_map(probe))
            gz2 = torch.randn_like(o2)
            gz1 = torch.randn_like(o1)
        convs = {"conv3": (gid, o2, hw2, mod.conv3, mod.bn3, dict(next_mask=o2, next_bn=mod.bn2))}
        if not is_dcn_block:
            convs["conv2"] = (gz2, o1, hw1, mod.conv2, None, dict(next_mask=o1, next_bn=mod.bn1))
        convs["conv1"] = (gz1, rows, hw, mod.conv1, None, dict(add=gid) if mod.downsample is None else {})
        if mod.downsample is not None:
            convs["downsample"] = (gid, rows, hw, mod.downsample[0], mod.downsample[1], {})
        parts = {"mask": lambda: ops.conv_gz_rows(go_rows, ops.rows_of_map(probe))}
        for cname, (gg, xin, chw, conv, bn, extra) in convs.items():
            parts[cname + "_wgrad"] = lambda gg=gg, xin=xin, chw=chw, conv=conv, bn=bn: ops.conv_bn_rows_backward(
                gg, None, xin, N_IMG, chw, conv.weight, bn, stride=conv.stride[0], need_dx=False)
            parts[cname + "_dgrad"] = lambda gg=gg, xin=xin, chw=chw, conv=conv, bn=bn, extra=extra: ops.conv_bn_rows_backward(
                gg, None, xin, N_IMG, chw, conv.weight, bn, stride=conv.stride[0], need_dw=False, **extra)
        if is_dcn_block:
            s2 = mod.conv2.stride[0]
            dx1, doffs = torch.zeros_like(o1), torch.zeros(offs.shape[0], 32, device=dev)
            dw2 = torch.zeros_like(mod.conv2.weight)
            w32 = ops.dcn_offset_padded_weight(mod.conv2.conv_offset.weight)
            goffs = torch.randn(offs.shape[0], 32, generator=g).to(dev)
            goffs[:, 27:] = 0
            parts["dcn_dgrad"] = lambda: ops.deform_conv_rows_backward(gz2, None, o1, N_IMG, hw1, offs, mod.conv2.weight, None, stride=s2,
                                                                       need_dw=False, dx_out=dx1, doffs_out=doffs)
            parts["dcn_wgrad"] = lambda: ops.deform_conv_rows_backward(gz2, None, o1, N_IMG, hw1, offs, mod.conv2.weight, None, stride=s2,
                                                                       need_dx=False, need_doffs=False, dw_out=dw2)
            parts["dcn_offset_wgrad"] = lambda: ops.conv_bn_rows_backward(goffs, None, o1, N_IMG, hw1, w32, None, stride=s2, need_dx=False)
            parts["dcn_offset_dgrad"] = lambda: ops.conv_bn_rows_backward(goffs, None, o1, N_IMG, hw1, w32, None, stride=s2, need_dw=False,
                                                                          add=gz1, next_mask=o1, next_bn=mod.bn1)
        for part, call in parts.items():
            rec = []
            ops.set_gemm_timer(lambda tag, fl, nb: (rec.append((fl, nb)), _Null())[1])
            try:
                with torch.no_grad(), ops.using(gemm="split"):
                    assert call() is not None, part
            finally:
                ops.set_gemm_timer(None)
            for mode in ("split", "bf16"):
                def fn(call=call, mode=mode):
                    with torch.no_grad(), ops.using(gemm=mode):
                        return call()
                arm = f"{part}_{mode}"
                fns[arm], flops[arm], nbytes[arm] = fn, rec[0][0], rec[0][1]
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

    out = dict(shape=name, arms=arms, flops=flops, nbytes=nbytes)
    blocks = [m for m in mod.modules() if isinstance(m, Bottleneck)]
    with ops.using(gemm="split"):
        out["covered"] = sum(any(p.requires_grad for p in b.parameters()) and ops.bottleneck_train_reject(b) is None for b in blocks)
        out["trainable"] = sum(any(p.requires_grad for p in b.parameters()) for b in blocks)
        with ops.using(dcn_train=True):
            out["covered_dcn"] = sum(any(p.requires_grad for p in b.parameters()) and ops.bottleneck_train_reject(b) is None
                                     for b in blocks)
    out["blocks"] = len(blocks)
    launches = []
    ops.set_gemm_timer(lambda tag, fl, nb: (launches.append((tag, fl, nb)), _Null())[1])
    try:
        fns["dcn_split" if has_dcn else "fast_split"]()
    finally:
        ops.set_gemm_timer(None)
    bwd = [l for l in launches if l[0].endswith(("_wgrad", "_dgrad", "_mask"))]
    out["launches"], out["backward_launches"] = len(launches), len(bwd)
    out["gflop"] = sum(l[1] for l in launches) / 1e9
    graphs = {arm: capture(fns[arm]) for arm in arms}
    times = {arm: [] for arm in arms}
    for _ in range(windows):
        for arm in arms:
            times[arm].append(timed(graphs[arm][0], steps))
    out["us"] = times
    ref = graphs["module"][1]
    rel = lambda a, b: float(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item())
    nx = 1 if is_block else 0       # the input's gradient comes first: per pixel, so one ReLU on the other side of its kink shows whole
    for mode in ("split", "bf16"):
        got = graphs["fast_" + mode][1]
        out["diff_dw_" + mode] = max(rel(a, b) for a, b in zip(got[nx:], ref[nx:]))
        out["diff_dx_" + mode] = rel(got[0], ref[0]) if nx else None
        if has_dcn:
            got = graphs["dcn_" + mode][1]
            out["dcn_diff_dw_" + mode] = max(rel(a, b) for a, b in zip(got[nx:], ref[nx:]))
            out["dcn_diff_dx_" + mode] = rel(got[0], ref[0]) if nx else None
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--net-steps", type=int, default=2, help="replays per window for the whole backbones")
    ap.add_argument("--shapes", default=",".join(list(BLOCKS) + list(DCN_BLOCKS) + list(NETS)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "backbone_train_ab.txt"))
    ap.add_argument("--child", metavar="SHAPE")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.windows, args.steps)
    lines = ["ResNet bottlenecks with frozen BatchNorms, 6 cameras, ONE forward + backward: the module path (torch convolution + BatchNorm + "
             "ReLU and their autograd) vs modes.backbone_train (one autograd Function per block: conv + BatchNorm + residual + ReLU per "
             "launch forward; one mask launch, then a weight-gradient and an input-gradient launch per convolution backward) in split "
             "and in bf16; every arm a replayed HIP graph",
             f"per shape: one fresh process, {args.windows} interleaved windows of {args.steps} replays per arm ({args.net_steps} for a "
             "whole backbone), us per step; GFLOP and MB per launch are algorithmic figures as the launch reports them",
             "the strided 3 x 3 input gradient is the plain gather form (dead taps stage zeros); the parity-class form is not built",
             ""]
    for name in args.shapes.split(","):
        env = {k: v for k, v in os.environ.items() if not k.startswith("BEVMSDA_")}
        steps = args.steps if name in BLOCKS or name in DCN_BLOCKS else args.net_steps
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
        if name in BLOCKS or name in DCN_BLOCKS:
            H, W, inplanes, planes, stride = (BLOCKS if name in BLOCKS else DCN_BLOCKS)[name]
            what = f"{N_IMG} x {H} x {W}, {inplanes} -> {planes} -> {4 * planes}, stride {stride}" + (", DCNv2 conv2, caffe" if name in DCN_BLOCKS else "")
        else:
            H, W, kw = NETS[name]
            what = f"{N_IMG} x 3 x {H} x {W}, ResNet-{kw['depth']} {kw['style']}"
        dcn_arms = "dcn_split" in r["arms"]
        cov = f"{r['covered']} of {r['trainable']} trainable blocks covered" + (f", {r['covered_dcn']} with dcn_train" if dcn_arms else "")
        lines.append(f"{name}: {what}: {cov} ({r['blocks']} blocks), {r['launches']} "
                     f"launches per step of which {r['backward_launches']} backward, {r['gflop']:.2f} GFLOP algorithmic")
        med = {arm: statistics.median(r["us"][arm]) for arm in r["arms"]}
        for arm in r["arms"]:
            v = r["us"][arm]
            tail = ""
            if arm in r["flops"]:
                tail = f"  GFLOP {r['flops'][arm] / 1e9:8.3f}  MB {r['nbytes'][arm] / 1e6:8.2f}  TFLOP/s {r['flops'][arm] / med[arm] / 1e6:6.1f}  " \
                       f"GB/s {r['nbytes'][arm] / med[arm] / 1e3:7.1f}"
            lines.append(f"{name:12s} {arm:24s}: median {med[arm]:10.1f}  min {min(v):10.1f}  max {max(v):10.1f}  spread {max(v) - min(v):8.1f}{tail}")
        for mode in ("split", "bf16"):
            f = med["fast_" + mode]
            verdict = "the fast path LOSES" if f > med["module"] else "the fast path wins"
            lines.append(f"{name:12s} {mode:5s}: module / fast = x{med['module'] / f:.2f} ({verdict})")
            if dcn_arms:
                d = med["dcn_" + mode]
                verdict = "dcn_train LOSES" if d > f else "dcn_train wins"
                lines.append(f"{name:12s} {mode:5s}: module / dcn = x{med['module'] / d:.2f}, fast (dcn_train off) / dcn = x{f / d:.2f} ({verdict})")
        if dcn_arms:
            ddx = "" if r["dcn_diff_dx_split"] is None else f"; input gradient split {r['dcn_diff_dx_split']:.3e}, bf16 {r['dcn_diff_dx_bf16']:.3e}"
            lines.append(f"{name:12s} dcn_train: max |dcn - module| / max |module|, worst weight gradient: split {r['dcn_diff_dw_split']:.3e}, bf16 "
                         f"{r['dcn_diff_dw_bf16']:.3e}{ddx}")
        dx = "" if r["diff_dx_split"] is None else f"; input gradient split {r['diff_dx_split']:.3e}, bf16 {r['diff_dx_bf16']:.3e}"
        lines.append(f"{name:12s} max |fast - module| / max |module|, worst weight gradient: split {r['diff_dw_split']:.3e}, bf16 "
                     f"{r['diff_dw_bf16']:.3e}{dx} (random inputs: ReLU inputs within the forward's rounding of zero take the other side)")
        lines.append("")
        print("\n".join(lines[first:]), flush=True)
        text = "\n".join(lines) + "\n"          # (written after every child: a later child's trouble keeps what was measured)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
