"""BEVFormerV2's temporal fusion alone at the sizes the configs run: the module path (permute to NCHW + contiguous per frame,
``ResNetFusion.forward``: cat, MIOpen convolutions, BatchNorm, permute back, Linear + LayerNorm) against the fast path
(``modes.bevfusion_fused``: ``ops.resnet_fusion`` on the channel-last convolution kernel straight from the frames' rows), in both
GEMM modes.  Workloads: ``t2`` = 2 frames x 256 -> 512, three blocks, 200 x 200, bs 1 (no downsample); ``t8first`` = the first
block of the t8 config, 8 frames x 256 -> 512 with its downsample convolution (plus the output projection), 200 x 200, bs 1.
Every (workload, mode) is a fresh child process with its own timeout.  A child captures BOTH paths as HIP graphs and times
them in alternating windows (off / on / off / on ...: device events around many replays), so that a drift of the box shows
as spread between the windows of ONE path instead of as a difference between the two; it also compares the two outputs.
Speed is reported, not gated: the switch stays off by default whatever comes out.  GPU box.

    python tools/fusion_ab.py [--windows 4] [--steps 10] [--out profiles/r13/fusion_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
WORKLOADS = {  # name: (frames, channels per frame, inter_channels, blocks, H, W)
    "t2": (2, 256, 512, 3, 200, 200),
    "t8first": (8, 256, 512, 1, 200, 200),
}


def conv_flops(frames, c, inter, blocks, H, W):
    """FLOPs of the 3 x 3 convolutions of the workload (2 per multiply-add), from the shapes."""
    cin = frames * c
    per = lambda ci, co: 2.0 * H * W * 9 * ci * co
    total = per(cin, inter) + per(inter, inter) + (per(cin, inter) if cin != inter else 0.0)
    return total + (blocks - 1) * 2 * per(inter, inter)


def child(name, mode, windows, steps):
    import torch

    sys.path.insert(0, ROOT)
    from bevformer_amd import ops
    from bevformer_amd.modules.transformer import ResNetFusion

    frames, c, inter, blocks, H, W = WORKLOADS[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    fusion = ResNetFusion(frames * c, 256, inter, blocks)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in fusion.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0, (9 * m.in_channels) ** -0.5, generator=g)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
    fusion = fusion.to(dev).eval()
    rows = [torch.randn(1, H * W, c, generator=g).to(dev) for _ in range(frames)]

    def module_path():
        maps = [x.reshape(x.shape[0], H, W, x.shape[-1]).permute(0, 3, 1, 2).contiguous() for x in rows]
        return fusion(maps)

    def fast_path():
        return fusion.forward_rows(rows, H, W)

    def capture(fn):
        for _ in range(3):
            fn()
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

    out = dict(workload=name, mode=mode, conv_gflop=conv_flops(*WORKLOADS[name]) / 1e9)
    with torch.no_grad(), ops.using(gemm=mode):
        g_off, y_off = capture(module_path)
        with ops.using(bevfusion_fused=True):
            why = ops.fusion_reject(fusion, rows)
            if why is not None:
                raise RuntimeError(f"the fast path does not cover this workload: {why}")
            g_on, y_on = capture(fast_path)
        off, on = [], []
        for _ in range(windows):
            off.append(timed(g_off, steps))
            on.append(timed(g_on, steps))
        out["off_us"], out["on_us"] = off, on
        out["max_abs_diff"] = float((y_on - y_off).abs().max().item())
        out["out_abs_max"] = float(y_off.abs().max().item())
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "fusion_ab.txt"))
    ap.add_argument("--child", nargs=2, metavar=("WORKLOAD", "MODE"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.windows, args.steps)
    lines = ["ResNetFusion alone, bs 1, 200 x 200 BEV grid: module path (permute + contiguous per frame, MIOpen convolutions) vs "
             "modes.bevfusion_fused (channel-last convolution kernel, frames read in place); both as replayed HIP graphs",
             f"per (workload, GEMM mode): one fresh process, {args.windows} alternating windows of {args.steps} replays per path "
             "(us per step); conv TFLOP/s = the convolutions' FLOPs from the shapes over the WHOLE step's time (end to end, "
             "not a kernel's share of peak)", ""]
    for name in WORKLOADS:
        for mode in ("split", "bf16"):
            env = {k: v for k, v in os.environ.items() if k not in ("BEVMSDA_BEVFUSION_FUSED", "BEVMSDA_GEMM")}
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, mode, "--windows", str(args.windows),
                                    "--steps", str(args.steps)], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                print(f"{name} {mode}: timed out after {CHILD_TIMEOUT} s — stopping", flush=True)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{name} {mode}: exit code {p.returncode} — stopping\n{p.stderr[-2000:]}", flush=True)
                return 1
            r = json.loads(line[-1][7:])
            for key, label in (("off_us", "module path"), ("on_us", "fast path  ")):
                v = r[key]
                lines.append(f"{name:8s} {mode:5s} {label}: median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}  "
                             f"spread {max(v) - min(v):7.1f}  conv TFLOP/s {r['conv_gflop'] / statistics.median(v) * 1e3:6.1f}")
            gain = statistics.median(r["off_us"]) - statistics.median(r["on_us"])
            spread = max(max(r[k]) - min(r[k]) for k in ("off_us", "on_us"))
            lines.append(f"{name:8s} {mode:5s} off - on = {gain:.1f} us (medians), x{statistics.median(r['off_us']) / statistics.median(r['on_us']):.2f}; "
                         f"largest spread between windows of one path {spread:.1f} us -> "
                         + ("the fast path is ahead by more than the spread" if gain > spread
                            else "the fast path is NOT ahead by more than the spread"))
            lines.append(f"{name:8s} {mode:5s} outputs: max |fast - module| {r['max_abs_diff']:.3e} at max |output| {r['out_abs_max']:.3f}")
            lines.append("")
            print("\n".join(lines[-5:]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
