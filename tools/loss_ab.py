"""The detection loss at base size (6 layers x 900 queries, bs = 1, 10 classes, code_size 10) with G in {8, 64, 256} gt
boxes: the module path (``BEVFormerHead.loss_single``'s statements: torch + scipy, one host round trip per layer) eagerly, and
the device path (``ops.detection_loss``: three launches) eagerly and as a replayed HIP graph, forward + backward.  The
module path cannot be captured — it reads the cost matrix back — so it has no replayed figure.  Every run is a fresh child
process with its own timeout and the tool stops at the first failure.  Speed is reported, not gated: the switch stays off
by default whatever comes out; what is gated is parity and capturability (tests/test_loss_fused_gpu.py).  GPU box.

    python tools/loss_ab.py [--steps 20] [--out profiles/r9/loss_ab.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
COUNTS = (8, 64, 256)


def child(G, fused, steps):
    import torch

    sys.path.insert(0, ROOT)
    import bevformer_amd
    from bevformer_amd import ops
    from bevformer_amd import synthetic as S

    dev = torch.device("cuda:0")
    L, nq = 6, 900
    torch.manual_seed(0)
    head = bevformer_amd.build_head(S.head_cfg("micro", num_query=nq, decoder_layers=2, max_num=300, train=True)).to(dev)
    g = torch.Generator().manual_seed(3)
    cls = (torch.randn(L, 1, nq, 10, generator=g) * 2 - 3).to(dev).requires_grad_(True)
    box = torch.randn(L, 1, nq, 10, generator=g)
    box[..., 0:2] = (torch.rand(L, 1, nq, 2, generator=g) * 2 - 1) * 51.2
    box = box.to(dev).requires_grad_(True)
    gts, labels = S.make_gt(5, (G,), device=dev)
    packed = ops.pack_gt(gts, labels, dev)
    cw = head.code_weights.detach()
    params = ops.head_loss_params(head)

    def step():
        if fused:
            losses = ops.detection_loss(cls, box, *packed, cw, params=params)
            return torch.autograd.grad(losses.sum(), (cls, box)) + (losses,)
        per = [head.loss_single(cls[i], box[i], gts, labels) for i in range(L)]
        total = sum(a.sum() + b.sum() for a, b in per)
        return torch.autograd.grad(total, (cls, box)) + (torch.stack([torch.stack([a.reshape(()), b.reshape(())]) for a, b in per]),)

    def timed(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / n          # us per step

    out = dict(G=G, fused=fused)
    for _ in range(3):
        res = step()
    torch.cuda.synchronize()
    out["eager_us"] = [timed(step, steps) for _ in range(3)]
    out["losses"] = res[2].detach().double().cpu().flatten().tolist()
    if fused:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        out["graph_us"] = [timed(graph.replay, steps) for _ in range(3)]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "loss_ab.txt"))
    ap.add_argument("--child", nargs=2, metavar=("G", "ARM"))
    args = ap.parse_args()
    if args.child:
        return child(int(args.child[0]), args.child[1] == "fused", args.steps)
    lines = ["detection loss, forward + backward, L = 6, nq = 900, bs = 1, 10 classes, code_size 10 (us per step; best of 3 windows of "
             f"{args.steps} steps; one fresh process per line)", ""]
    for G in COUNTS:
        got = {}
        for arm in ("module", "fused"):
            env = {k: v for k, v in os.environ.items() if k != "BEVMSDA_LOSS_FUSED"}
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(G), arm, "--steps", str(args.steps)],
                                   env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                print(f"G {G} {arm}: timed out after {CHILD_TIMEOUT} s — stopping", flush=True)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"G {G} {arm}: exit code {p.returncode} — stopping\n{p.stderr[-2000:]}", flush=True)
                return 1
            r = got[arm] = json.loads(line[-1][7:])
            graph = f"{min(r['graph_us']):10.1f}" if "graph_us" in r else "         —"
            lines.append(f"G {G:4d}  {arm:6s}  eager {min(r['eager_us']):10.1f}  replayed {graph}")
            print(lines[-1], flush=True)
        worst = max(abs(a - b) / max(abs(b), 1e-30) for a, b in zip(got["fused"]["losses"], got["module"]["losses"]))
        lines.append(f"G {G:4d}  losses, fused against module: worst relative difference {worst:.2e}")
        lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
