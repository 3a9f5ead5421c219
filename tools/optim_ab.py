"""The optimizer step on the parameter list of a base-size encoder + decoder + head (``synthetic.head_cfg('base')``): gradient
clipping at max_norm 35 + AdamW (lr 2e-4, weight decay 0.01), three ways, each eagerly and as a replayed HIP graph over
static gradients:

  foreach   ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.AdamW(foreach=True, capturable=True)``
  fused     ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.AdamW(fused=True, capturable=True)``
  hip       ``bevformer_amd.optim.AdamW2`` (csrc/optim.h: two launches)

Beside the times, the achieved bytes/s of ``hip`` on its algorithmic bytes — 4 read per element by the norm launch, 16 read +
12 written by the update — next to the chip's measured 6.29 TB/s copy rate.  Every run is a fresh child process with its own
timeout and the tool stops at the first failure.  Speed is reported, not gated; what is gated is parity and capturability
(tests/test_optim_gpu.py).  GPU box.

    python tools/optim_ab.py [--steps 20] [--out profiles/r10/optim_ab.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
ARMS = ("foreach", "fused", "hip")
COPY_RATE = 6.29e12


def child(arm, steps):
    import torch

    sys.path.insert(0, ROOT)
    import bevformer_amd
    from bevformer_amd import synthetic as S
    from bevformer_amd.optim import AdamW2

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    head = bevformer_amd.build_head(S.head_cfg("base")).to(dev)
    params = [p for p in head.parameters() if p.requires_grad]
    g = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=dev)
    clip = dict(max_norm=35, norm_type=2)
    if arm == "hip":
        opt = AdamW2(params, lr=2e-4, weight_decay=0.01, grad_clip=clip)
        step = opt.step
    else:
        opt = torch.optim.AdamW(params, lr=2e-4, weight_decay=0.01, capturable=True, **{arm: True})

        def step():
            torch.nn.utils.clip_grad_norm_(params, **clip)
            opt.step()

    def timed(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / n          # us per step

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    out = dict(arm=arm, tensors=len(params), elements=sum(p.numel() for p in params))
    out["eager_us"] = [timed(step, steps) for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "optim_ab.txt"))
    ap.add_argument("--child", metavar="ARM")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps)
    lines = ["clip_grad_norm_(35) + AdamW on the parameters of a base-size encoder + decoder + head (us per step; best of 3 windows "
             f"of {args.steps} steps; one fresh process per line)", ""]
    for arm in ARMS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm, "--steps", str(args.steps)],
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            print(f"{arm}: timed out after {CHILD_TIMEOUT} s — stopping", flush=True)
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{arm}: exit code {p.returncode} — stopping\n{p.stderr[-2000:]}", flush=True)
            return 1
        r = json.loads(line[-1][7:])
        if arm == ARMS[0]:
            lines[0] += f"; {r['tensors']} tensors, {r['elements']:,} elements"
        lines.append(f"{arm:8s} eager {min(r['eager_us']):10.1f}  replayed {min(r['graph_us']):10.1f}")
        if arm == "hip":
            rate = 32.0 * r["elements"] / (min(r["graph_us"]) * 1e-6)
            lines.append(f"hip, replayed: {rate / 1e12:.2f} TB/s on 32 algorithmic bytes per element (norm 4 read; update 16 read + 12 "
                         f"written) = {100 * rate / COPY_RATE:.0f} % of the measured {COPY_RATE / 1e12:.2f} TB/s copy rate")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
