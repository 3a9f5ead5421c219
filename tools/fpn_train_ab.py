"""The image neck alone, forward + backward, under ``modes.fpn_train`` against the module path, 6 cameras.  Shapes: ``base`` =
512 / 1024 / 2048 -> 256 at 116 x 200 with ``num_outs`` 4 (bevformer_base.py's neck on the 928 x 1600 image) and ``tiny`` = 2048 -> 256
at 15 x 25 with ``num_outs`` 1.  The inputs are dense channel-last and need a gradient, as a backbone on rows hands them over.  Arms,
each ONE forward + backward captured as a HIP graph on one stream:

    module        the module path (torch convolutions, interpolate, adds and their autograd; every switch off)
    fast_split    modes.fpn_train, GEMM mode split
    fast_bf16     ... GEMM mode bf16

and every backward launch of the fast path on its own in both modes (``extra<j>`` / ``out<i>`` / ``lateral<i>`` x ``_wgrad`` /
``_dgrad``, with the epilogue the neck's backward gives it) with its algorithmic FLOPs and bytes as the launch reports them.  The
weight-gradient launches accumulate into buffers that are not re-zeroed between replays.

One fresh child process per shape with its own timeout; interleaved windows (device events around many replays), so a drift of
the box shows as spread between the windows of ONE arm.  Speed is reported, not gated; the switch stays off by default.  GPU box.

    python tools/fpn_train_ab.py [--windows 4] [--steps 10] [--shapes base,tiny] [--out profiles/r21/fpn_train_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 400
N_IMG = 6
SHAPES = ("base", "tiny")
ARMS = ("module", "fast_split", "fast_bf16")


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def child(name, windows, steps):
    import torch

    sys.path.insert(0, ROOT)
    import bevformer_amd
    from bevformer_amd import ops, synthetic as S

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    neck = bevformer_amd.build_neck(S.neck_cfg(name))
    with torch.no_grad():           # a trained neck's regime: every level O(1)
        for m in neck.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight[0].numel() ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    neck = neck.to(dev)
    xs = [x.requires_grad_() for x in S.make_neck_inputs(name, n_img=N_IMG, seed=1, device=dev, channels_last=True)]
    params = list(neck.parameters())
    wrt = xs + params
    with torch.no_grad():
        probe = neck(xs)
    gos = [torch.randn(o.shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for o in probe]

    def step(**modes):
        def fn():
            with ops.using(**modes):
                outs = neck(xs)
                return torch.autograd.grad(sum((o * go).sum() for o, go in zip(outs, gos)), wrt)
        return fn

    fns = {"module": step(gemm="split", fpn_train=False, fpn_fused=False), "fast_split": step(gemm="split", fpn_train=True),
           "fast_bf16": step(gemm="bf16", fpn_train=True)}
    arms, flops, nbytes = list(ARMS), {}, {}

    # every backward launch on its own: its operands are made once, outside the graphs
    lat, outs, extras, start, end = ops.neck._plan(neck)
    n, ne = len(lat), len(extras)
    with torch.no_grad(), ops.using(gemm="split"):
        xrows, laterals, rows, hws = ops.neck._fpn_rows(ops, neck, [x.detach() for x in xs])
    grow = [ops.rows_of_map(go) for go in gos]
    glat = [torch.randn_like(l) for l in laterals]
    parts = {}

    def add_part(label, conv, gz, x, hw, wkw, dkw):
        dw, db = torch.zeros_like(conv.weight), torch.zeros_like(conv.bias)
        parts[label + "_wgrad"] = lambda: ops.conv_bn_rows_backward(gz, None, x, N_IMG, hw, conv.weight, None, need_dx=False, dw_out=dw,
                                                                    db_out=db, **wkw)
        if dkw is not None:
            parts[label + "_dgrad"] = lambda: ops.conv_bn_rows_backward(gz, None, x, N_IMG, hw, conv.weight, None, need_dw=False, **dkw)

    for j in range(ne - 1, -1, -1):
        relu_in = bool(j > 0 and neck.relu_before_extra_convs)
        mask = dict(next_mask=rows[n - 1 + j], add_after_mask=True) if relu_in else {}
        add_part(f"extra{j}", extras[j], grow[n + j], rows[n - 1 + j], hws[n - 1 + j], dict(stride=2, relu_x=relu_in),
                 dict(stride=2, add=grow[n - 1 + j], **mask))
    for i in range(n):
        add_part(f"out{i}", outs[i], grow[i], laterals[i], hws[i], {}, dict(add=glat[i - 1], add_pool2=True) if i else {})
    for i in range(n):
        add_part(f"lateral{i}", lat[i], glat[i], xrows[i], hws[i], {}, {})
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

    def timed(graph, k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(k):
            graph.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / k          # us per step

    out = dict(shape=name, arms=arms, flops=flops, nbytes=nbytes)
    with ops.using(gemm="split"):
        out["reject"] = ops.fpn_train_reject(neck, xs)
    launches = []
    ops.set_gemm_timer(lambda tag, fl, nb: (launches.append((tag, fl, nb)), _Null())[1])
    try:
        fns["fast_split"]()
    finally:
        ops.set_gemm_timer(None)
    bwd = [l for l in launches if l[0].endswith(("_wgrad", "_dgrad"))]
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
    for mode in ("split", "bf16"):
        got = graphs["fast_" + mode][1]
        out["diff_dx_" + mode] = max(rel(a, b) for a, b in zip(got[:len(xs)], ref[:len(xs)]))
        out["diff_dw_" + mode] = max(rel(a, b) for a, b in zip(got[len(xs):], ref[len(xs):]))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "fpn_train_ab.txt"))
    ap.add_argument("--child", metavar="SHAPE")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.windows, args.steps)
    sys.path.insert(0, ROOT)
    from bevformer_amd import synthetic as S
    lines = ["FPN, 6 cameras, dense channel-last inputs that need a gradient, ONE forward + backward: the module path (torch convolutions, "
             "interpolate, adds and their autograd) vs modes.fpn_train (one autograd Function for the neck: ops.fpn's launches forward; a "
             "weight-gradient launch with the bias gradient in it and an input-gradient launch per convolution backward) in split and in "
             "bf16; every arm a replayed HIP graph",
             f"per shape: one fresh process, {args.windows} interleaved windows of {args.steps} replays per arm, us per step; GFLOP and MB per "
             "launch are algorithmic figures as the launch reports them",
             ""]
    for name in args.shapes.split(","):
        env = {k: v for k, v in os.environ.items() if not k.startswith("BEVMSDA_")}
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
        first = len(lines)
        cin, num_outs, (H, W) = S.NECKS[name]
        lines.append(f"{name}: {N_IMG} x {' / '.join(str(c) for c in cin)} -> {S.EMBED_DIMS} at {H} x {W}, num_outs {num_outs}: "
                     f"fpn_train_reject = {r['reject']}, {r['launches']} launches per step of which {r['backward_launches']} backward, "
                     f"{r['gflop']:.2f} GFLOP algorithmic")
        med = {arm: statistics.median(r["us"][arm]) for arm in r["arms"]}
        for arm in r["arms"]:
            v = r["us"][arm]
            tail = ""
            if arm in r["flops"]:
                tail = f"  GFLOP {r['flops'][arm] / 1e9:8.3f}  MB {r['nbytes'][arm] / 1e6:8.2f}  TFLOP/s {r['flops'][arm] / med[arm] / 1e6:6.1f}  " \
                       f"GB/s {r['nbytes'][arm] / med[arm] / 1e3:7.1f}"
            lines.append(f"{name:6s} {arm:24s}: median {med[arm]:10.1f}  min {min(v):10.1f}  max {max(v):10.1f}  spread {max(v) - min(v):8.1f}{tail}")
        for mode in ("split", "bf16"):
            f = med["fast_" + mode]
            verdict = "the fast path LOSES" if f > med["module"] else "the fast path wins"
            lines.append(f"{name:6s} {mode:5s}: module / fast = x{med['module'] / f:.2f} ({verdict})")
        lines.append(f"{name:6s} max |fast - module| / max |module|: worst input gradient split {r['diff_dx_split']:.3e}, bf16 "
                     f"{r['diff_dx_bf16']:.3e}; worst parameter gradient split {r['diff_dw_split']:.3e}, bf16 {r['diff_dw_bf16']:.3e} "
                     "(random inputs: a ReLU input within the forward's rounding of zero takes the other side)")
        lines.append("")
        print("\n".join(lines[first:]), flush=True)
        text = "\n".join(lines) + "\n"          # (written after every child: a later child's trouble keeps what was measured)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
