"""The image neck alone at the sizes the configs run: the module path (``FPN.forward_torch``: MIOpen convolutions on NCHW maps,
``interpolate``, adds) against the fast path (``modes.fpn_fused``: ``ops.fpn`` on the channel-last row convolution kernel), in
both GEMM modes.  Workloads: ``base`` = 6 cameras, 512 / 1024 / 2048 channels at 116 x 200, 58 x 100, 29 x 50 -> 4 levels of 256;
``tiny`` = 6 cameras, 2048 channels at 15 x 25 -> 1 level of 256.  Arms, each captured as a HIP graph:

    module        the module path on NCHW inputs
    fast_nchw     the fast path on NCHW inputs (one channels-last copy per level inside the graph)
    fast_cl       the fast path on inputs that are dense in torch.channels_last (read in place)
    module+flat   module path + ops.flatten_feats (contiguous + transposing kernel)
    fast+flat     fast path on channels-last inputs + ops.flatten_feats on its views (the row kernel, no transpose)

Every (workload, mode) is a fresh child process with its own timeout.  A child times the arms in interleaved windows (device
events around many replays), so that a drift of the box shows as spread between the windows of ONE arm instead of as a
difference between arms; it also compares the outputs.  Speed is reported, not gated: the switch stays off by default
whatever comes out.  GPU box.

    python tools/fpn_ab.py [--windows 4] [--steps 10] [--out profiles/r14/fpn_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
WORKLOADS = ("base", "tiny")
ARMS = ("module", "fast_nchw", "fast_cl", "module+flat", "fast+flat")


def neck_flops(in_channels, out_c, num_outs, n_img, hw):
    """FLOPs of the neck's convolutions (2 per multiply-add), from the shapes."""
    total, (h, w) = 0.0, hw
    sizes = []
    for c in in_channels:
        sizes.append((h, w))
        total += 2.0 * n_img * h * w * (c * out_c + 9 * out_c * out_c)
        h, w = h // 2, w // 2
    h, w = sizes[-1]
    for _ in range(num_outs - len(in_channels)):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        total += 2.0 * n_img * h * w * 9 * out_c * out_c
    return total


def child(name, mode, windows, steps):
    import torch

    sys.path.insert(0, ROOT)
    import bevformer_amd
    from bevformer_amd import ops, synthetic as S

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    neck = bevformer_amd.build_neck(S.neck_cfg(name)).to(dev).eval()
    nchw = S.make_neck_inputs(name, device=dev)
    cl = [x.contiguous(memory_format=torch.channels_last) for x in nchw]
    g = torch.Generator().manual_seed(1)
    n_lvl = S.NECKS[name][1]
    cams_embeds = torch.randn(S.NUM_CAMS, S.EMBED_DIMS, generator=g).to(dev)
    level_embeds = torch.randn(n_lvl, S.EMBED_DIMS, generator=g).to(dev)

    def flat(levels):
        return ops.flatten_feats([o.view(1, S.NUM_CAMS, *o.shape[1:]) for o in levels], cams_embeds, level_embeds)[0]

    fns = {"module": lambda: neck.forward_torch(nchw), "fast_nchw": lambda: neck(nchw), "fast_cl": lambda: neck(cl),
           "module+flat": lambda: flat(neck.forward_torch(nchw)), "fast+flat": lambda: flat(neck(cl))}

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

    in_c, num_outs, hw = S.NECKS[name]
    out = dict(workload=name, mode=mode, conv_gflop=neck_flops(in_c, S.EMBED_DIMS, num_outs, S.NUM_CAMS, hw) / 1e9)
    with torch.no_grad(), ops.using(gemm=mode):
        graphs = {}
        for arm in ARMS:
            with ops.using(fpn_fused=arm.startswith("fast")):
                if arm.startswith("fast"):
                    why = ops.fpn_reject(neck, nchw)
                    if why is not None:
                        raise RuntimeError(f"the fast path does not cover this workload: {why}")
                graphs[arm] = capture(fns[arm])
        times = {arm: [] for arm in ARMS}
        for _ in range(windows):
            for arm in ARMS:
                times[arm].append(timed(graphs[arm][0], steps))
        out["us"] = times
        ref = graphs["module"][1]
        out["max_abs_diff"] = max(float((a - b).abs().max().item()) for a, b in zip(graphs["fast_cl"][1], ref))
        out["nchw_vs_cl_equal"] = all(bool(torch.equal(a, b)) for a, b in zip(graphs["fast_nchw"][1], graphs["fast_cl"][1]))
        out["out_abs_max"] = max(float(t.abs().max().item()) for t in ref)
        out["flat_max_abs_diff"] = float((graphs["fast+flat"][1] - graphs["module+flat"][1]).abs().max().item())
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "fpn_ab.txt"))
    ap.add_argument("--child", nargs=2, metavar=("WORKLOAD", "MODE"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.windows, args.steps)
    lines = ["FPN alone, 6 cameras: module path (MIOpen convolutions on NCHW maps) vs modes.fpn_fused (channel-last row convolution "
             "kernel); every arm a replayed HIP graph",
             f"per (workload, GEMM mode): one fresh process, {args.windows} interleaved windows of {args.steps} replays per arm "
             "(us per step); conv TFLOP/s = the convolutions' FLOPs from the shapes over the WHOLE step's time (end to end, "
             "not a kernel's share of peak)", ""]
    for name in WORKLOADS:
        for mode in ("split", "bf16"):
            env = {k: v for k, v in os.environ.items() if k not in ("BEVMSDA_FPN_FUSED", "BEVMSDA_GEMM")}
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
            first = len(lines)
            for arm in ARMS:
                v = r["us"][arm]
                lines.append(f"{name:5s} {mode:5s} {arm:12s}: median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}  "
                             f"spread {max(v) - min(v):7.1f}  conv TFLOP/s {r['conv_gflop'] / statistics.median(v) * 1e3:6.1f}")
            med = {arm: statistics.median(r["us"][arm]) for arm in ARMS}
            spread = max(max(v) - min(v) for v in r["us"].values())
            for a, b in (("module", "fast_nchw"), ("module", "fast_cl"), ("module+flat", "fast+flat")):
                gain = med[a] - med[b]
                lines.append(f"{name:5s} {mode:5s} {a} - {b} = {gain:.1f} us (medians), x{med[a] / med[b]:.2f}; largest spread between "
                             f"windows of one arm {spread:.1f} us -> the fast arm is " + ("" if gain > spread else "NOT ")
                             + "ahead by more than the spread")
            lines.append(f"{name:5s} {mode:5s} outputs: max |fast - module| {r['max_abs_diff']:.3e} at max |output| {r['out_abs_max']:.3f}; "
                         f"NCHW and channels-last inputs bit-equal: {r['nchw_vs_cl_equal']}; flattened max |fast - module| "
                         f"{r['flat_max_abs_diff']:.3e}")
            lines.append("")
            print("\n".join(lines[first:]), flush=True)
            text = "\n".join(lines) + "\n"          # (written after every child: a later child's trouble keeps what was measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
