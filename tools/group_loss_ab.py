"""``BEVFormerHead_GroupDETR.loss`` at the shape of the bevformerv2 configs — 6 decoder layers, one sample, 11 groups of 900
queries, 40 gt boxes: 66 matching problems — forward and backward to the predictions' gradients, two ways:

  module    the modules of the head (``loss_fused`` off): per problem the assigner's torch costs, a device-to-host copy, scipy,
            and the torch losses.  It reads device values on the host, so it cannot be captured; eager only
  fused     ``ops.detection_loss(groups=11)`` (csrc/det_cost.h, match_lsap.h, det_loss.h: four launches, no host read), eagerly
            and as a replayed HIP graph

Both arms run in ONE child process on the same seeded inputs, in alternating windows (module, fused eager, fused replayed,
module, ...), so that a drift of the shared machine falls on all of them; each line reports the best window and the spread
of the windows.  The arms' losses are compared first (rtol 1e-4, the bound of tests/test_group_loss_gpu.py for the two paths).
The child has its own timeout and the tool stops at the first failure.  Speed is reported, not gated; what is gated is parity
and capturability (tests/test_group_loss_gpu.py).  GPU box.

    python tools/group_loss_ab.py [--rounds 5] [--out profiles/r12/group_loss_ab.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 400
L, BS, G, N, NGT = 6, 1, 11, 900, 40
STEPS = {"module": 2, "fused_eager": 50, "fused_graph": 200}        # steps per window: each window is > 0.1 s of work or 2 steps


def child(rounds):
    import torch

    sys.path.insert(0, ROOT)
    import bevformer_amd
    from bevformer_amd import ops, synthetic as S

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    head = bevformer_amd.build_head(S.head_cfg("micro", num_query=N, decoder_layers=L, max_num=20, train=True, group_detr=G)).to(dev)
    # predictions in the head's output format: logits N(-2, 1.5), centres inside the base pc_range, log sizes, (sin, cos), velocities
    g = torch.Generator().manual_seed(100 + N + G)
    cls = torch.randn(L, BS, G * N, 10, generator=g) * 1.5 - 2.0
    box = torch.randn(L, BS, G * N, 10, generator=g)
    box[..., 0:2] = (torch.rand(L, BS, G * N, 2, generator=g) * 2 - 1) * 51.2
    box[..., 4] = torch.rand(L, BS, G * N, generator=g) * 8 - 5
    gts, labels = S.make_gt(200 + N + G, (NGT,) * BS)
    cls, box = cls.to(dev).requires_grad_(True), box.to(dev).requires_grad_(True)
    gts, labels = [g.to(dev) for g in gts], [x.to(dev) for x in labels]
    preds = {"all_cls_scores": cls, "all_bbox_preds": box, "enc_cls_scores": None, "enc_bbox_preds": None}
    assert head.loss_fused_reject(preds, gts) is None

    def head_step(fused):
        with ops.using(loss_fused=fused):
            d = head.loss(gts, labels, preds)
        total = sum(v.sum() for v in d.values())
        grads = torch.autograd.grad(total, (cls, box))
        return d, grads

    # the captured form: what a captured training step holds — packed gt in static buffers, the four launches, the backward.
    # Its leaves are made INSIDE the step: ``cls`` and ``box`` have been used on the default stream above, their gradient
    # accumulators belong to that stream, and a backward onto them inside a capture would make the default stream wait on a
    # captured event (torch warns about exactly this), which the HIP runtime does not survive.
    gt, label, count = ops.pack_gt(gts, labels, dev)
    cw, params = head.code_weights.detach(), ops.head_loss_params(head)

    def fused_core():
        c, b = cls.detach().requires_grad_(True), box.detach().requires_grad_(True)
        losses = ops.detection_loss(c, b, gt, label, count, cw, params=params, groups=G)
        return losses, torch.autograd.grad(losses.sum(), (c, b))

    def timed(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / n          # us per step

    md, mg = head_step(False)
    fd, fg = head_step(True)
    for k in md:
        torch.testing.assert_close(fd[k].reshape(()), md[k].reshape(()), rtol=1e-4, atol=1e-6)
    for a, b in zip(fg, mg):
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-6)
    losses, (gc, _) = fused_core()
    core = (losses.detach(), gc)
    del losses
    assert torch.equal(core[0][-1, 0], fd["loss_cls"].detach().reshape(())) and torch.equal(core[1], fg[0])
    print("STAGE the two paths agree; capturing", flush=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused_core()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fused_core()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static[0], core[0]) and torch.equal(static[1][0], core[1])
    print("STAGE the replay equals the eager run; timing", flush=True)

    arms = {"module": lambda: head_step(False), "fused_eager": lambda: head_step(True), "fused_graph": graph.replay}
    for fn in arms.values():                        # warm-up of every arm
        fn()
    out = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            out[name].append(timed(fn, STEPS[name]))
            print(f"STAGE {name} {out[name][-1]:.1f} us", flush=True)
    out["loss_cls"] = float(fd["loss_cls"])
    out["max_rel_loss_diff"] = max(abs(float(fd[k]) - float(md[k])) / abs(float(md[k])) for k in md)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "group_loss_ab.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.rounds)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds)],
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        print(f"timed out after {CHILD_TIMEOUT} s — stopping", flush=True)
        return 1
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"exit code {p.returncode} — stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
        return 1
    r = json.loads(line[-1][7:])
    lines = [f"BEVFormerHead_GroupDETR.loss, forward + backward to the predictions: L = {L}, bs = {BS}, {G} groups of {N} queries, "
             f"{NGT} gt ({L * BS * G} matching problems); us per step; best and (min .. max) of {args.rounds} windows, the arms "
             "alternating in one process",
             f"the two paths' losses agree to {r['max_rel_loss_diff']:.1e} relative (loss_cls {r['loss_cls']:.4f})", ""]
    for name, label in (("module", "module, eager"), ("fused_eager", "fused, eager"), ("fused_graph", "fused, replayed")):
        t = r[name]
        lines.append(f"{label:16s} {min(t):12.1f}   ({min(t):.1f} .. {max(t):.1f}; windows of {STEPS[name]} steps)")
    lines.append("module, replayed          n/a   (the module path reads device values on the host: not capturable)")
    lines.append(f"module / fused: eager {min(r['module']) / min(r['fused_eager']):.1f} x, "
                 f"eager module / replayed fused {min(r['module']) / min(r['fused_graph']):.1f} x")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
