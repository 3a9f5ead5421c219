"""The backbone's stem under ``modes.stem_fused`` against the module path, 6 cameras, at the sizes the reference configs run:
``base`` (6 x 3 x 928 x 1600) and ``tiny`` (6 x 3 x 480 x 800).  Stem arms (``stem_base``, ``stem_tiny``), each captured as a HIP graph:

    module_nchw   today's four launches (conv1, bn1, relu, maxpool) on the NCHW batch plus the channels-last copy the first
                  block of ``backbone_fused`` pays (``rows_of_map``)
    fast_split    ``ops.stem``: one launch, GEMM mode split; its output IS the channel-last rows
    fast_bf16     ... GEMM mode bf16

Whole-backbone arms (``net_base``: ResNet-101, caffe style, DCNv2 in stages 3 and 4; ``net_tiny``: ResNet-50, pytorch style), GEMM
mode split: ``backbone_fused`` with the stem on torch, ``backbone_fused`` + ``stem_fused``.

One fresh child process per shape with its own timeout.  A child times the arms in interleaved windows (device events around
many replays), so that a drift of the box shows as spread between the windows of ONE arm instead of as a difference between
arms; it also compares the outputs.  GB/s and TFLOP/s are ALGORITHMIC: the image in, the pooled rows out and the weight; the
convolution's products.  Speed is reported, not gated, and the switch stays off by default whatever comes out.  GPU box.

    python tools/stem_ab.py [--windows 4] [--steps 10] [--net-steps 2] [--out profiles/r18/stem_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from backbone_ab import N_IMG, NETS, _randomize  # noqa: E402

CHILD_TIMEOUT = 400
SIZES = {"base": (928, 1600), "tiny": (480, 800)}
SHAPES = ("stem_base", "stem_tiny", "net_base", "net_tiny")
STEM_ARMS = ("module_nchw", "fast_split", "fast_bf16")
NET_ARMS = ("backbone_fused", "backbone_fused+stem_fused")


def child(name, windows, steps):
    import torch

    sys.path.insert(0, ROOT)
    from bevformer_amd import ops
    from bevformer_amd.modules import ResNet

    kind, size = name.split("_")
    H, W = SIZES[size]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    kw = NETS[size][2] if kind == "net" else dict(depth=50, num_stages=1, out_indices=(0,))
    net = _randomize(ResNet(**kw), g).to(dev).eval()
    x = torch.randn(N_IMG, 3, H, W, generator=g).to(dev)

    if kind == "stem":
        def module():
            return ops.rows_of_map(net.maxpool(net.relu(net.bn1(net.conv1(x)))))

        def fast(mode):
            def fn():
                with ops.using(gemm=mode):
                    return ops.rows_of_map(ops.stem(net, x))
            return fn
        fns = {"module_nchw": module, "fast_split": fast("split"), "fast_bf16": fast("bf16")}
    else:
        def arm(stem):
            def fn():
                with ops.using(gemm="split", backbone_fused=True, stem_fused=stem):
                    return net(x)[-1]
            return fn
        fns = {"backbone_fused": arm(False), "backbone_fused+stem_fused": arm(True)}
    arms = list(fns)

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

    out = dict(shape=name, arms=arms)
    with torch.no_grad():
        with ops.using(gemm="split"):
            assert ops.stem_reject(net, x) is None
        launches = []
        ops.set_gemm_timer(lambda tag, fl, nb: (launches.append((tag, fl, nb)), _Null())[1])
        try:
            with ops.using(gemm="split"):
                ops.stem(net, x)
        finally:
            ops.set_gemm_timer(None)
        assert len(launches) == 1, launches         # the stem is ONE launch
        out["gflop"], out["mbytes"] = launches[0][1] / 1e9, launches[0][2] / 1e6
        graphs = {a: capture(fns[a]) for a in arms}
        times = {a: [] for a in arms}
        for _ in range(windows):
            for a in arms:
                times[a].append(timed(graphs[a][0], steps))
        out["us"] = times
        ref = graphs[arms[0]][1]
        out["out_abs_max"] = float(ref.abs().max().item())
        out["diff"] = {a: float((graphs[a][1] - ref).abs().max().item()) for a in arms[1:]}
        out["view"] = bool(ops.rows_of_map(ops.stem(net, x)).data_ptr() == ops.stem(net, x).data_ptr()) if kind == "stem" else None
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
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "stem_ab.txt"))
    ap.add_argument("--child", metavar="SHAPE")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.windows, args.steps)
    lines = ["ResNet stem, 6 cameras: the module path (conv1, bn1, relu, maxpool as four torch launches on the NCHW batch + the "
             "channels-last copy the first fused bottleneck pays) vs modes.stem_fused (ONE launch: 7 x 7 stride-2 convolution + "
             "BatchNorm + ReLU + 3 x 3 max pooling, NCHW in, channel-last rows out) in split and in bf16; then the whole backbone "
             "under modes.backbone_fused with the stem on torch and with modes.stem_fused; every arm a replayed HIP graph",
             f"per shape: one fresh process, {args.windows} interleaved windows of {args.steps} replays per arm ({args.net_steps} for a "
             "whole backbone), us per step; GFLOP and MB are the stem's algorithmic figures as its launch reports them (image in, "
             "pooled rows out, weight; the convolution's products): GB/s and TFLOP/s = those over the arm's time",
             ""]
    for name in args.shapes.split(","):
        env = {k: v for k, v in os.environ.items()
               if k not in ("BEVMSDA_BACKBONE_FUSED", "BEVMSDA_DCN_FUSED", "BEVMSDA_STEM_FUSED", "BEVMSDA_GEMM")}
        kind, size = name.split("_")
        steps = args.steps if kind == "stem" else args.net_steps
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
        H, W = SIZES[size]
        what = "the stem alone" if kind == "stem" else f"ResNet-{NETS[size][2]['depth']} {NETS[size][2]['style']}"
        lines.append(f"{name}: {N_IMG} x 3 x {H} x {W}, {what}; the stem: {r['gflop']:.2f} GFLOP, {r['mbytes']:.1f} MB algorithmic")
        med = {a: statistics.median(r["us"][a]) for a in r["arms"]}
        for a in r["arms"]:
            v = r["us"][a]
            tail = f"  GB/s {r['mbytes'] / med[a] * 1e3:7.1f}  TFLOP/s {r['gflop'] / med[a] * 1e3:6.2f}" if kind == "stem" else ""
            lines.append(f"{name:9s} {a:26s}: median {med[a]:10.1f}  min {min(v):10.1f}  max {max(v):10.1f}  "
                         f"spread {max(v) - min(v):8.1f}{tail}")
        spread = max(max(v) - min(v) for v in r["us"].values())
        ref = r["arms"][0]
        for a in r["arms"][1:]:
            verdict = "LOSES" if med[a] > med[ref] else "wins"
            lines.append(f"{name:9s} {ref} / {a} = x{med[ref] / med[a]:.2f} ({a} {verdict}: {med[ref] - med[a]:+.1f} us); "
                         f"max |{a} - {ref}| {r['diff'][a]:.3e} at max |output| {r['out_abs_max']:.3f}")
        if kind == "stem":
            floor_b, floor_f = r["mbytes"] / 8e6 * 1e6, r["gflop"] / 2.5e6 * 1e6        # 8 TB/s; 2.5 PFLOP/s dense bf16
            lines.append(f"{name:9s} floors: {floor_b:.1f} us at 8 TB/s, {floor_f:.1f} us ({3 * floor_f:.1f} us for split's three products) at "
                         f"2.5 PFLOP/s; rows_of_map of the fast arm is a view: {r['view']}")
        lines.append(f"{name:9s} largest spread between windows of one arm {spread:.1f} us")
        lines.append("")
        print("\n".join(lines[first:]), flush=True)
        text = "\n".join(lines) + "\n"          # (written after every child: a later child's trouble keeps what was measured)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
