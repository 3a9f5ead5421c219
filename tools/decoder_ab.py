"""The detection decoder alone at base size (900 queries, 200 x 200 BEV, 6 layers, bs = 1) with ``modes.decoder_fused`` off
and on.  Every run is a fresh child process with its own timeout; the two settings alternate (off / on / off / on ...), so
that a drift of the box shows as spread between the runs of ONE setting instead of as a difference between the two.  A child
times the step eagerly and as a replayed HIP graph (device events around many steps), collects per-tag kernel times through
the ``ops`` timer hooks in a pass of its own, and counts the kernels of one replayed step with the torch profiler (in a pass
of its own as well).  GPU box.

    python tools/decoder_ab.py [--pairs 4] [--out profiles/r7/decoder_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240


def child(fused, steps):
    import contextlib

    import torch

    sys.path.insert(0, ROOT)
    import bevformer_amd
    from bevformer_amd import ops
    from bevformer_amd import synthetic as S

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    dec = bevformer_amd.build_transformer_layer_sequence(S.reference_decoder_cfg(6)).eval()
    dec.load_state_dict(S.trained_like_({k: v.clone() for k, v in dec.state_dict().items()}, seed=7))
    dec = dec.to(dev)
    reg = torch.nn.ModuleList([torch.nn.Linear(256, 10) for _ in range(6)]).to(dev)
    q, qp, v, ref, shapes, start = S.make_decoder_inputs(200, 200, num_query=900, bs=1, seed=4, device=dev)
    kw = dict(query=q, key=None, value=v, query_pos=qp, reference_points=ref, reg_branches=reg, spatial_shapes=shapes,
              level_start_index=start)

    def timed(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / n          # us per step

    out = dict(fused=fused)
    with torch.no_grad(), ops.using(decoder_fused=fused):
        step = lambda: dec(**kw)
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        out["eager_us"] = [timed(step, steps) for _ in range(3)]

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            res = step()
        for _ in range(10):
            graph.replay()
        torch.cuda.synchronize()
        out["graph_us"] = [timed(graph.replay, 4 * steps) for _ in range(3)]
        out["checksum"] = float(res[0].double().abs().sum().item())

        # per-tag kernel times, eager, in a pass of its own (event brackets around every launch of the package)
        events = []

        def bracket(tag):
            @contextlib.contextmanager
            def ctx():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                yield
                e.record()
                events.append((tag, s, e))
            return ctx()
        ops.set_gemm_timer(lambda tag, flops, nbytes: bracket(tag))
        ops.set_kernel_timer(lambda tag, nbytes: bracket(tag))
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        ops.set_gemm_timer(None)
        ops.set_kernel_timer(None)
        tags = {}
        for tag, s, e in events:
            a = tags.setdefault(tag, [0.0, 0])
            a[0] += s.elapsed_time(e) * 1e3
            a[1] += 1
        out["tags"] = {t: dict(us=a[0] / a[1], per_step=a[1] / 20) for t, a in tags.items()}

        # kernels of one replayed step (the profiler's first windows may come back empty: a few attempts, two replays each)
        out["replay_launches"] = None
        try:
            from torch.profiler import ProfilerActivity, profile
            for _ in range(4):
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    graph.replay()
                    graph.replay()
                    torch.cuda.synchronize()
                n = sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA"))
                if n:
                    out["replay_launches"] = n / 2
                    break
        except Exception as exc:       # noqa: BLE001
            out["replay_launches_error"] = repr(exc)[:200]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "decoder_ab.txt"))
    ap.add_argument("--child", choices=("off", "on"))
    ap.add_argument("--notes", default=None, help="a text file appended to the report (e.g. the accuracy figures of the tests)")
    args = ap.parse_args()
    if args.child:
        return child(args.child == "on", args.steps)
    runs = []
    for i in range(2 * args.pairs):
        setting = "on" if i % 2 else "off"
        env = {k: v for k, v in os.environ.items() if k != "BEVMSDA_DECODER_FUSED"}
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting, "--steps", str(args.steps)],
                               env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            print(f"run {i} ({setting}): timed out after {CHILD_TIMEOUT} s — stopping", flush=True)
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"run {i} ({setting}): exit code {p.returncode} — stopping\n{p.stderr[-2000:]}", flush=True)
            return 1
        runs.append(json.loads(line[-1][7:]))
        r = runs[-1]
        print(f"run {i} {setting:3s}: eager {min(r['eager_us']):8.1f} us  graph {min(r['graph_us']):8.1f} us  "
              f"launches/replay {r['replay_launches']}", flush=True)

    lines = ["decoder alone, base size (900 queries, 200 x 200 BEV, 6 layers, bs = 1, reg_branches), split GEMM mode",
             f"{args.pairs} alternating pairs of fresh processes; per run: best of 3 windows of {args.steps} eager / "
             f"{4 * args.steps} replayed steps (us per step)", ""]
    lines.append(f"{'run':>3s} {'switch':>6s} {'eager us':>10s} {'graph us':>10s} {'launches/replay':>16s} {'checksum':>16s}")
    for i, r in enumerate(runs):
        lines.append(f"{i:3d} {'on' if r['fused'] else 'off':>6s} {min(r['eager_us']):10.1f} {min(r['graph_us']):10.1f} "
                     f"{str(r['replay_launches']):>16s} {r['checksum']:16.6f}")
    lines.append("")
    summary = {}
    for name, sel in (("off", False), ("on", True)):
        for key in ("eager_us", "graph_us"):
            vals = [min(r[key]) for r in runs if r["fused"] == sel]
            summary[(name, key)] = vals
            lines.append(f"switch {name:3s} {key:9s}: median {statistics.median(vals):8.1f}  min {min(vals):8.1f}  max {max(vals):8.1f}  "
                         f"spread (max - min) {max(vals) - min(vals):6.1f}")
    off, on = summary[("off", "graph_us")], summary[("on", "graph_us")]
    gain = statistics.median(off) - statistics.median(on)
    spread = max(off) - min(off)
    lines.append("")
    lines.append(f"replayed step: off - on = {gain:.1f} us (medians); spread between repeated switch-off runs {spread:.1f} us -> "
                 + ("the fused step is faster by more than the spread" if gain > spread
                    else "NOT faster by more than the spread: the switch stays experimental"))
    lines.append("")
    for name, sel in (("off", False), ("on", True)):
        r = [x for x in runs if x["fused"] == sel][-1]
        lines.append(f"per-tag kernel times, eager, switch {name} (last run; us per launch x launches per step):")
        tot = 0.0
        for tag, t in sorted(r["tags"].items(), key=lambda kv: -kv[1]["us"] * kv[1]["per_step"]):
            lines.append(f"    {tag:28s} {t['us']:8.1f} x {t['per_step']:4.1f}")
            tot += t["us"] * t["per_step"]
        lines.append(f"    {'sum of the package kernels':28s} {tot:8.1f}")
        lines.append("")
    if args.notes and os.path.exists(args.notes):
        lines.append(open(args.notes).read().rstrip())
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
