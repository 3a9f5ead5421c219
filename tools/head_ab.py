"""The detection head alone at base size (6 layers x 900 queries, bs = 1: branch chains of every layer, reference-point
arithmetic and the NMS-free decode of the last layer) and the decoder at base size (``decoder_fused`` on, stock three-Linear
reg branches), each with ``modes.head_fused`` off and on.  Every run is a fresh child process with its own timeout; the two
settings alternate (off / on / off / on ...), so that a drift of the box shows as spread between the runs of ONE setting
instead of as a difference between the two.  A child times its step as a replayed HIP graph (device events around many
replays) and eagerly.  Speed is reported, not gated: the switch stays off by default whatever comes out.  GPU box.

    python tools/head_ab.py [--pairs 3] [--out profiles/r8/head_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 180


def _branches(L, seed):
    import copy

    import torch
    nn = torch.nn
    torch.manual_seed(seed)
    cls = nn.Sequential(nn.Linear(256, 256), nn.LayerNorm(256), nn.ReLU(inplace=True), nn.Linear(256, 256), nn.LayerNorm(256),
                        nn.ReLU(inplace=True), nn.Linear(256, 10))
    reg = nn.Sequential(nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 10))
    return (nn.ModuleList([copy.deepcopy(cls) for _ in range(L)]).eval(), nn.ModuleList([copy.deepcopy(reg) for _ in range(L)]).eval())


def child(what, fused, steps):
    import types

    import torch

    sys.path.insert(0, ROOT)
    import bevformer_amd
    from bevformer_amd import ops
    from bevformer_amd import synthetic as S
    from bevformer_amd.modules.head import BEVFormerHead, NMSFreeCoder

    dev = torch.device("cuda:0")
    cls, reg = _branches(6, 1)
    cls, reg = cls.to(dev), reg.to(dev)
    g = torch.Generator().manual_seed(2)
    if what == "head":
        hs = torch.randn(6, 900, 1, 256, generator=g).to(dev)
        init_ref = (torch.rand(1, 900, 3, generator=g) * 0.9 + 0.05).to(dev)
        inter = (torch.rand(6, 1, 900, 3, generator=g) * 0.9 + 0.05).to(dev)
        coder = NMSFreeCoder(S.PC_RANGE, post_center_range=S.POST_CENTER_RANGE, max_num=300, num_classes=10)
        stub = types.SimpleNamespace(cls_branches=cls, reg_branches=reg, pc_range=S.PC_RANGE,
                                     head_fused_reject=lambda hs=None: None)
        range_t = torch.tensor(S.POST_CENTER_RANGE, device=dev)

        def step():
            c, b = BEVFormerHead.predictions(stub, hs, init_ref, inter)
            if fused:
                return coder.decode_padded(dict(all_cls_scores=c, all_bbox_preds=b))
            # the reference's decode_single up to its boolean slice (the slice synchronises: outside the timed step in both arms)
            scores, idx = c[-1][0].sigmoid().view(-1).topk(300)
            from bevformer_amd.modules.head import denormalize_bbox
            boxes = denormalize_bbox(b[-1][0][idx // 10])
            keep = (boxes[..., :3] >= range_t[:3]).all(1) & (boxes[..., :3] <= range_t[3:]).all(1)
            return scores, idx % 10, boxes, keep
    else:
        torch.manual_seed(0)
        dec = bevformer_amd.build_transformer_layer_sequence(S.reference_decoder_cfg(6)).eval()
        dec.load_state_dict(S.trained_like_({k: v.clone() for k, v in dec.state_dict().items()}, seed=7))
        dec = dec.to(dev)
        q, qp, v, ref, shapes, start = S.make_decoder_inputs(200, 200, num_query=900, bs=1, seed=4, device=dev)
        kw = dict(query=q, key=None, value=v, query_pos=qp, reference_points=ref, reg_branches=reg, spatial_shapes=shapes,
                  level_start_index=start)
        step = lambda: dec(**kw)

    def timed(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / n          # us per step

    out = dict(what=what, fused=fused)
    with torch.no_grad(), ops.using(decoder_fused=True, head_fused=fused):
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
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8", "head_ab.txt"))
    ap.add_argument("--child", nargs=2, metavar=("WHAT", "SWITCH"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1] == "on", args.steps)
    lines = ["head alone (6 x 900 rows, bs = 1: branch chains + reference arithmetic + decode of the last layer) and the decoder "
             "(base size, decoder_fused on, stock reg branches), modes.head_fused off / on, split GEMM mode",
             f"{args.pairs} alternating pairs of fresh processes per workload; per run: best of 3 windows of {args.steps} eager / "
             f"{4 * args.steps} replayed steps (us per step)", ""]
    for what in ("head", "decoder"):
        runs = []
        for i in range(2 * args.pairs):
            setting = "on" if i % 2 else "off"
            env = {k: v for k, v in os.environ.items() if k not in ("BEVMSDA_HEAD_FUSED", "BEVMSDA_DECODER_FUSED")}
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, setting, "--steps", str(args.steps)],
                                   env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                print(f"{what} run {i} ({setting}): timed out after {CHILD_TIMEOUT} s — stopping", flush=True)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{what} run {i} ({setting}): exit code {p.returncode} — stopping\n{p.stderr[-2000:]}", flush=True)
                return 1
            runs.append(json.loads(line[-1][7:]))
            r = runs[-1]
            print(f"{what} run {i} {setting:3s}: eager {min(r['eager_us']):8.1f} us  graph {min(r['graph_us']):8.1f} us", flush=True)
            lines.append(f"{what:8s} run {i} switch {setting:3s}  eager {min(r['eager_us']):9.1f}  graph {min(r['graph_us']):9.1f}  "
                         f"checksum {r['checksum']:.6f}")
        lines.append("")
        med = {}
        for name, sel in (("off", False), ("on", True)):
            for key in ("eager_us", "graph_us"):
                vals = [min(r[key]) for r in runs if r["fused"] == sel]
                med[(name, key)] = vals
                lines.append(f"{what:8s} switch {name:3s} {key:9s}: median {statistics.median(vals):8.1f}  min {min(vals):8.1f}  "
                             f"max {max(vals):8.1f}  spread (max - min) {max(vals) - min(vals):6.1f}")
        off, on = med[("off", "graph_us")], med[("on", "graph_us")]
        gain, spread = statistics.median(off) - statistics.median(on), max(off) - min(off)
        lines.append(f"{what:8s} replayed step: off - on = {gain:.1f} us (medians); spread between repeated switch-off runs "
                     f"{spread:.1f} us -> " + ("the fused form is ahead by more than the spread" if gain > spread
                                               else "the fused form is NOT ahead by more than the spread"))
        lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
