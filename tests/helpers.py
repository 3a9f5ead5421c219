"""Shared test helpers (tests may use oracle/; the product package may not)."""
import contextlib
import functools

import torch

from bevformer_amd import ops
from oracle import bevformer_cpu as O


def _oracle_msda(value, shapes, start, loc, attn, im2col_step=64, tag=None):
    return O.msda_gridsample(value, shapes, loc, attn)


def _oracle_msda_ragged(value, shapes, start, loc, attn, row_batch, tag=None, msda=None):
    """Ragged batch through the oracle: one call per value-batch entry.  ``msda``: the operator's statement (default: the
    grid_sample form; ``c_oracle_msda`` for gradients by the operator's own convention)."""
    msda = msda or O.msda_gridsample
    R, M = loc.shape[:2]
    out = value.new_zeros(R, M * value.shape[-1])
    for n in range(value.shape[0]):
        sel = (row_batch == n).nonzero().squeeze(-1)
        if sel.numel():
            out[sel] = msda(value[n:n + 1], shapes, loc[sel][None], attn[sel][None])[0]
    return out


def _oracle_msda_fused(value, shapes, start, proj, n_off, ref, row_batch, *, M, L, P, K, off_head,
                       off_k, lg_head, lg_k, ref_mode, vmul, vadd, Q=0, row_src=None, tag=None, msda=None, **_lds):
    """CPU statement of the fused entry point's contract (include/bevmsda.h,
    ``bevmsda_fused_forward_*``) out of torch ops + the oracle operator: what the
    kernel must compute for a given descriptor."""
    if row_src is not None:                 # one projection row per BEV query, shared by its rows
        proj = proj[row_src.long()]
    R = proj.shape[0]
    D = value.shape[-1]
    A = ref.shape[-2]
    ref = ref.reshape(R, K, A, 2)
    norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(proj.dtype)            # (L,2) = (W,H)
    m = torch.arange(M)[:, None]
    lp = torch.arange(L * P)[None, :]
    base = row_batch.long() if row_batch is not None else torch.arange(R) // Q
    out = value.new_zeros(R, M * D)
    for k in range(K):
        col_lg = n_off + m * lg_head + k * lg_k + lp                                 # (M, L*P)
        att = proj[:, col_lg].softmax(-1).view(R, M, L, P)
        col_off = (m * off_head + k * off_k + lp * 2)[..., None] + torch.arange(2)   # (M, L*P, 2)
        off = proj[:, col_off].view(R, M, L, P, 2)
        if ref_mode == 0:
            rp = ref[:, k][:, torch.arange(P) % A]                                   # (R,P,2)
            loc = rp[:, None, None, :, :] + off / norm[None, None, :, None, :]
        else:
            loc = ref[:, k][:, None, :, None, :] + off / norm[None, None, :, None, :]
        n = (base * vmul + k * vadd).to(torch.int32)
        out = out + _oracle_msda_ragged(value, shapes, start, loc, att, n, msda=msda)
    return out / K


def _oracle_gather_mean(rows, idx, scale):
    """Contract of ``bevmsda_gather_mean_f32`` in torch ops."""
    Qn, J = idx.shape
    out = rows.new_zeros(Qn, rows.shape[1])
    for j in range(J):
        sel = idx[:, j].long()
        ok = sel >= 0
        out[ok] += rows[sel[ok]]
    return out * scale.reshape(-1, 1)


def _oracle_rotate_bev(prev_bev, angles_deg, center, bev_h, bev_w):
    out = prev_bev.clone()
    for i in range(prev_bev.shape[1]):
        img = prev_bev[:, i].reshape(bev_h, bev_w, -1).permute(2, 0, 1)
        out[:, i] = O.rotate_nearest(img, angles_deg[i], center).permute(1, 2, 0).reshape(bev_h * bev_w, -1)
    return out


def kernel_rotation_index(h, w, angle_deg, center, device, device_pose=False):
    """The source-pixel map (h*w,) int64 (-1 = zero fill) the product's rotate kernel applies for this pose, read
    off an index image; ``device_pose`` takes the GraphedBevHistory route (angle in a device tensor, matrix from
    ``ops.rotation_theta_device``)."""
    img = (torch.arange(h * w, dtype=torch.float32) + 1).view(-1, 1, 1).expand(-1, 1, 256).contiguous().to(device)
    ang = torch.tensor([angle_deg], dtype=torch.float64, device=device) if device_pose else [float(angle_deg)]
    return ops.rotate_bev(img, ang, center, h, w)[:, 0, 0].round().long().cpu() - 1


def _oracle_flatten_feats(mlvl_feats, cams_embeds, level_embeds):
    """Contract of ``bevmsda_flatten_feats_f32`` in torch ops (transformer.py:165-184)."""
    flat, shapes = [], []
    for lvl, feat in enumerate(mlvl_feats):
        h, w = feat.shape[3:]
        feat = feat.flatten(3).permute(1, 0, 3, 2)
        if cams_embeds is not None:
            feat = feat + cams_embeds[:, None, None, :]
        feat = feat + level_embeds[None, None, lvl:lvl + 1, :]
        shapes.append((h, w))
        flat.append(feat)
    out = torch.cat(flat, 2).permute(0, 2, 1, 3).contiguous()
    ss = torch.as_tensor(shapes, dtype=torch.long)
    return out, ss, torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))


@contextlib.contextmanager
def oracle_ops():
    """Route the package's operator calls through the CPU oracle so that the
    HOST logic of the modules (ragged rows, merged GEMMs, geometry, plans,
    tiling) can be parity-tested without a GPU.  Test-only: the product path
    itself has no CPU implementation."""
    saved = (ops.msda, ops.msda_ragged, ops.msda_fused, ops.gather_mean, ops.rotate_bev,
             ops.flatten_feats)
    ops.msda, ops.msda_ragged, ops.msda_fused, ops.gather_mean, ops.rotate_bev, ops.flatten_feats = \
        _oracle_msda, _oracle_msda_ragged, _oracle_msda_fused, _oracle_gather_mean, \
        _oracle_rotate_bev, _oracle_flatten_feats
    try:
        yield
    finally:
        (ops.msda, ops.msda_ragged, ops.msda_fused, ops.gather_mean, ops.rotate_bev,
         ops.flatten_feats) = saved


def build_pair(name, seed=3, device="cpu"):
    """(product encoder, reference-keyed state_dict with 'trained-like' weights)."""
    import bevformer_amd
    from bevformer_amd import synthetic as S
    torch.manual_seed(0)
    enc = bevformer_amd.build_transformer_layer_sequence(S.encoder_cfg(name)).eval()
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    S.trained_like_(sd, seed=seed)
    enc.load_state_dict(sd)
    return enc.to(device), sd


def build_transformer_pair(name, seed=3, device="cpu"):
    """(product PerceptionTransformer, its state_dict with trained-like encoder weights and
    N(0,1)-scale embeddings / can-bus MLP)."""
    import bevformer_amd
    from bevformer_amd import synthetic as S
    torch.manual_seed(0)
    t = bevformer_amd.build_transformer(S.transformer_cfg(name)).eval()
    t.init_weights()
    sd = {k: v.clone() for k, v in t.state_dict().items()}
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    S.trained_like_(enc, seed=seed)
    for k, v in enc.items():
        sd["encoder." + k] = v
    t.load_state_dict(sd)
    return t.to(device), sd


def split_transformer_sd(sd):
    """-> (transformer-own parameters, encoder state_dict without the prefix)."""
    own = {k: v for k, v in sd.items() if not k.startswith(("encoder.", "decoder."))}
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    return own, enc


# ---------------------------------------------------------------------------------------------------------------------
# The oracle on a SUBSET of BEV queries, and the edge-adjacent sampling points of a frame
# ---------------------------------------------------------------------------------------------------------------------
def _tsa_rows(sd, pre, query, value, hist_rows, bev_pos, ref_2d, bev_h, bev_w, msda, num_heads=8, num_points=4):
    """``O.temporal_self_attention`` (temporal_self_attention.py:177-272) for the query rows ``query`` (bs, R, C) of a
    grid whose value tensor ``value`` (bs * 2, Q, C) is complete; ``hist_rows`` = value[:bs] at the same rows (the first
    half of the projection's input).  The only change against the oracle function: the rows of the concatenation."""
    bs, R, C = query.shape
    identity = query
    query = query + bev_pos
    shapes = torch.tensor([[bev_h, bev_w]])
    q2 = torch.cat([hist_rows, query], -1)
    v = O._lin(sd, pre + "value_proj", value).reshape(bs * 2, value.shape[1], num_heads, -1)
    off = O._lin(sd, pre + "sampling_offsets", q2).view(bs, R, num_heads, 2, 1, num_points, 2)
    att = O._lin(sd, pre + "attention_weights", q2).view(bs, R, num_heads, 2, num_points)
    att = att.softmax(-1).view(bs, R, num_heads, 2, 1, num_points)
    att = att.permute(0, 3, 1, 2, 4, 5).reshape(bs * 2, R, num_heads, 1, num_points).contiguous()
    off = off.permute(0, 3, 1, 2, 4, 5, 6).reshape(bs * 2, R, num_heads, 1, num_points, 2)
    norm = torch.stack([shapes[..., 1], shapes[..., 0]], -1)
    loc = ref_2d[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    out = msda(v, shapes, loc, att)
    out = out.permute(1, 2, 0).view(R, C, bs, 2).mean(-1).permute(2, 0, 1)
    return O._lin(sd, pre + "output_proj", out) + identity


def oracle_encoder_rows(sd, bev_query, feats, rows, *, bev_h, bev_w, bev_pos, spatial_shapes, prev_bev, shift, img_metas,
                        pc_range, msda=None, num_points_in_pillar=4, **_):
    """Rows ``rows`` (1-D long tensor of BEV query ids) of ``O.encoder_forward`` WITH a history BEV, out of the oracle's own
    pieces: every per-query operation of a layer is row-wise, the only cross-query reads are the sampling values
    (camera features; [history, layer-0 queries]), which stay complete.  Pinned against the full oracle on the CPU
    (tests/test_oracle.py::test_oracle_rows_helper_equals_the_full_oracle).  Any dtype (float64 for the gradient checks)."""
    msda = msda or O.msda_gridsample
    num_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    bs = bev_query.size(1)
    dt = bev_query.dtype
    # the geometry in float32 whatever ``dt``: the reference computes it in float32 (encoder.py:86, @force_fp32), and a
    # float64 projection would decide borderline visibility tests differently from every float32 implementation
    g = torch.float32
    ref_3d = O.pillar_points(bev_h, bev_w, pc_range[5] - pc_range[2], num_points_in_pillar, bs, g)
    ref_2d = O.bev_grid_points(bev_h, bev_w, bs, g)
    ref_cam, bev_mask = O.project_to_cameras(ref_3d, pc_range, img_metas)
    shifted = (ref_2d.clone() + shift.to(g)[:, None, None, :]).to(dt)
    ref_2d, ref_cam = ref_2d.to(dt), ref_cam.to(dt)
    x_full = bev_query.permute(1, 0, 2)
    pos = bev_pos.permute(1, 0, 2)[:, rows]
    Q = x_full.shape[1]
    prev = torch.stack([prev_bev.permute(1, 0, 2), x_full], 1).reshape(bs * 2, Q, -1)
    hybrid = torch.stack([shifted, ref_2d], 1).reshape(bs * 2, Q, 1, 2)[:, rows]
    hist_rows = prev[:bs][:, rows]
    ref_cam, bev_mask = ref_cam[:, :, rows], bev_mask[:, :, rows]
    x = x_full[:, rows]
    for i in range(num_layers):
        pre = f"layers.{i}."
        x = _tsa_rows(sd, pre + "attentions.0.", x, prev, hist_rows, pos, hybrid, bev_h, bev_w, msda)
        x = O.layer_norm(sd, pre + "norms.0", x)
        x = O.spatial_cross_attention(sd, pre + "attentions.1.", x, feats, ref_cam, bev_mask, spatial_shapes, msda=msda)
        x = O.layer_norm(sd, pre + "norms.1", x)
        h = O._lin(sd, pre + "ffns.0.layers.0.0", x)           # O.ffn, with the pre-activations shown to the recorder
        if hasattr(msda, "preactivations"):
            msda.preactivations(h)
        x = x + O._lin(sd, pre + "ffns.0.layers.1", torch.relu(h))
        x = O.layer_norm(sd, pre + "norms.2", x)
    return x


class EdgeRecorder:
    """An ``msda=`` stand-in for the oracle that evaluates the operator and REMEMBERS which BEV queries own a sampling point
    within ``eps`` pixels of a pixel boundary (x = loc_x * W - 0.5 within eps of an integer, or y): bilinear sampling is
    piecewise linear in the location, so such a point takes the slope of one cell in one evaluation and of its neighbour
    in another when round-off moves it across — a comparison of gradients means something on the OTHER queries.
    ``cam_rows[i]`` = the BEV query of every row of camera i's rebatch (``bev_mask[i][0].sum(-1).nonzero()``: the
    oracle's own list); calls with 2 * bs value entries are TemporalSelfAttention's (row = query)."""

    def __init__(self, num_queries, cam_rows, eps=1e-4, query_ids=None, relu_eps=0.0):
        self.fragile = torch.zeros(num_queries, dtype=torch.bool)
        self.cam_rows, self.eps, self.relu_eps = cam_rows, eps, relu_eps
        self.query_ids = query_ids          # rows of a subset evaluation -> BEV query ids (None: identity)

    def preactivations(self, h):
        """The FFN's ReLU is the other kink of a layer: rows with a pre-activation within ``relu_eps`` of zero."""
        if self.relu_eps:
            near = (h.detach().abs() < self.relu_eps).any(-1).any(0)
            ids = torch.arange(near.shape[0]) if self.query_ids is None else self.query_ids
            self.fragile[ids[near]] = True

    def __call__(self, value, shapes, loc, att):
        out = O.msda_gridsample(value, shapes, loc, att)
        with torch.no_grad():
            wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(loc.dtype)           # (L, 2) = (W, H)
            px = loc.detach() * wh[None, None, None, :, None, :] - 0.5
            fr = px - px.floor()
            near = (torch.minimum(fr, 1 - fr) < self.eps).any(-1).flatten(2).any(-1)    # (N, rows)
            if value.shape[0] == len(self.cam_rows):                                    # SCA: one value entry per camera
                for i, ids in enumerate(self.cam_rows):
                    self.fragile[ids[near[i, :len(ids)]]] = True
            else:
                ids = torch.arange(near.shape[1]) if self.query_ids is None else self.query_ids
                self.fragile[ids[near.any(0)]] = True
        return out


def camera_rows(name, rows=None):
    """The BEV query of every row of the oracle's per-camera rebatch for workload ``name`` (spatial_cross_attention.py:136-141),
    optionally for a subset evaluation over queries ``rows`` (ids are then BEV query ids of the subset's rows)."""
    from bevformer_amd import synthetic as S
    w = S.WORKLOADS[name]
    ref_3d = O.pillar_points(w["bev_h"], w["bev_w"], S.PC_RANGE[5] - S.PC_RANGE[2], 4, 1, torch.float32)
    _, bev_mask = O.project_to_cameras(ref_3d, S.PC_RANGE, S.make_img_metas(name))
    if rows is not None:
        bev_mask = bev_mask[:, :, rows]
    out = []
    for m in bev_mask:
        local = m[0].sum(-1).nonzero().squeeze(-1)
        out.append(local if rows is None else rows[local])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# A reference-only yardstick for bf16 error: the oracle with bf16 roundings, against the oracle without
# ---------------------------------------------------------------------------------------------------------------------
def _bf16_ste(t):
    """Round to bf16, straight through for autograd (the emulated oracle stays differentiable)."""
    return t + (t.bfloat16().float() - t).detach()


@contextlib.contextmanager
def oracle_bf16(gemm, storage):
    """``oracle.bevformer_cpu`` with the roundings bf16 arithmetic legitimately performs, and nothing of the product:
    ``gemm``    every Linear layer of the encoder (``O._lin``) takes both operands rounded to bf16; products are summed in
                fp32 and the bias is added in fp32 (``gemm="bf16"``: one bf16 MFMA per product, fp32 accumulator).  The
                can-bus MLP of ``get_bev_features`` calls ``F.linear`` itself and stays fp32, as the product's
                ``nn.Sequential`` does (modules/transformer.py: ``self.can_bus_mlp(can_bus)``);
    ``storage`` the projected value tensor that enters the sampling operator is rounded to bf16
                (``value_storage=torch.bfloat16``: the value projection's epilogue writes bf16).
    Dropout, LayerNorm, softmax and the sampling arithmetic stay fp32.  The oracle's file is untouched: its functions
    look ``_lin`` and ``encoder_forward`` up in the module at call time."""
    real_lin, real_enc = O._lin, O.encoder_forward

    def lin(sd, key, x):
        return torch.nn.functional.linear(_bf16_ste(x), _bf16_ste(sd[key + ".weight"]), sd[key + ".bias"])

    def rounded_values(msda):
        def call(value, shapes, loc, att):
            return msda(_bf16_ste(value), shapes, loc, att)
        return call

    def encoder_forward(*a, msda=O.msda_gridsample, **k):
        return real_enc(*a, msda=rounded_values(msda), **k)

    if gemm:
        O._lin = lin
    if storage:
        O.encoder_forward = encoder_forward
    try:
        yield
    finally:
        O._lin, O.encoder_forward = real_lin, real_enc


def output_errors(got, want):
    """(max abs, 1 - cosine) of two outputs; the cosine in float64 (in fp32 it came out as 1.0003 for these tensors)."""
    a, b = got.detach().double().flatten().cpu(), want.detach().double().flatten().cpu()
    cos = torch.dot(a, b) / (a.norm() * b.norm())
    return (a - b).abs().max().item(), (1.0 - cos).item()


def gradient_errors(got, want):
    """{tensor: (relative L2 error, max error / largest entry of the reference tensor)}."""
    out = {}
    for k, b in want.items():
        a, b = got[k].detach().double().cpu(), b.detach().double().cpu()
        out[k] = (((a - b).norm() / (b.norm() + 1e-30)).item(), ((a - b).abs().max() / (b.abs().max() + 1e-30)).item())
    return out


def row_block_ratio(got, want, block=64):
    """Per-row max abs error of two (1, Q, C) outputs -> (worst 64-row-aligned block's mean row error) / (mean row error
    over all rows): a wrong partial panel or a mis-addressed row segment stands out here even when every element of it is
    'within bf16 noise'."""
    rows = (got.detach().double() - want.detach().double()).abs().amax(-1).flatten().cpu()
    n = rows.numel() // block * block
    blocks = [rows[:n].view(-1, block).mean(1)]
    if n < rows.numel():
        blocks.append(rows[n:].mean().reshape(1))
    return (torch.cat(blocks).max() / rows.mean()).item()


def oracle_training_step(name, gemm=False, storage=False, dropout_scales=None, gout_seed=5):
    """Output and gradients (BEV queries, camera features, every parameter) of workload ``name`` with a history BEV through
    autograd of the oracle, plain (fp32) or under ``oracle_bf16(gemm, storage)`` -> (output, {tensor: gradient})."""
    from bevformer_amd import synthetic as S
    torch.set_num_threads(16)
    _, sd = build_pair(name)
    q, f, kw = S.make_inputs(name, seed=0, temporal=True)
    gout = torch.randn(1, q.shape[0], 256, generator=torch.Generator().manual_seed(gout_seed))
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    qc, fc = q.clone().requires_grad_(True), f.clone().requires_grad_(True)
    with oracle_bf16(gemm, storage):
        out = O.encoder_forward(leaves, qc, fc, pc_range=S.PC_RANGE, dropout_scales=dropout_scales, **kw)
        out.backward(gout)
    grads = {"bev_query": qc.grad, "feat": fc.grad, **{k: v.grad for k, v in leaves.items() if v.grad is not None}}
    return out.detach(), grads


def oracle_forward(name, gemm=False, storage=False, temporal=True):
    from bevformer_amd import synthetic as S
    torch.set_num_threads(16)
    _, sd = build_pair(name)
    q, f, kw = S.make_inputs(name, seed=0, temporal=temporal)
    with torch.no_grad(), oracle_bf16(gemm, storage):
        return O.encoder_forward(sd, q, f, pc_range=S.PC_RANGE, **kw)


def E_ref(emulated, plain):
    """The bf16 yardstick: the error of the EMULATED oracle (``oracle_bf16``) against the plain fp32 oracle on the same
    inputs and weights, in the metrics the GPU tests use.  ``emulated`` / ``plain``: outputs -> dict(max_abs, one_minus_cos,
    block_ratio), or (output, gradients) pairs of ``oracle_training_step`` -> the same plus l2 / max_ratio (worst tensor)
    and ``per_tensor``.  It holds everything bf16 legitimately costs — the slope flips at pixel boundaries that
    bf16-perturbed offsets cause included — and nothing of the product."""
    grads = isinstance(emulated, tuple)
    out_e, out_p = (emulated[0], plain[0]) if grads else (emulated, plain)
    mx, omc = output_errors(out_e, out_p)
    res = dict(max_abs=mx, one_minus_cos=omc, block_ratio=row_block_ratio(out_e, out_p))
    if grads:
        per = gradient_errors(emulated[1], plain[1])
        res.update(per_tensor=per, l2=max(v[0] for v in per.values()), max_ratio=max(v[1] for v in per.values()))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# The bench's four-frame scene (BASELINE configs[4], ``queue4_bf16``), restated
# ---------------------------------------------------------------------------------------------------------------------
def queue_scene(name, frames=4):
    """DELIBERATE DUPLICATE of bench.py's ``make_queue_step`` scene (bench.py is a yardstick and is not edited or
    imported by tests): ``frames`` frames of ONE scene over the same camera features, absolute can-bus poses advancing
    by (2.0, 0.5) m and 4 degrees per frame -> (mlvl_feats, bev_queries, kwargs without img_metas / prev_bev, [metas])."""
    import copy
    import numpy as np
    from bevformer_amd import synthetic as S
    mlvl, bq, kw = S.make_transformer_inputs(name, seed=0, temporal=False)
    kw.pop("prev_bev")
    metas = []
    for i in range(frames):
        m = copy.deepcopy(kw["img_metas"])
        m[0]["scene_token"] = "bench-scene"
        m[0]["can_bus"][:3] = np.array([2.0 * (i + 1), 0.5 * (i + 1), 0.0])
        m[0]["can_bus"][-1] = 4.0 * (i + 1)
        metas.append(m)
    return mlvl, bq, {k: v for k, v in kw.items() if k != "img_metas"}, metas


def queue_oracle(name, sd, scene, rotate_fn=None):
    """DELIBERATE DUPLICATE of bench.py's ``queue_oracle``, returning EVERY frame: the scene through
    ``O.get_bev_features`` under the restated ``forward_test`` state machine (detectors/bevformer.py:236-269).
    ``rotate_fn``: the history rotation (default: the oracle's own nearest-neighbour map)."""
    import copy
    from bevformer_amd import synthetic as S
    torch.set_num_threads(16)
    mlvl, bq, rest, metas = scene
    own, enc = split_transformer_sd({k: v.detach().float().cpu() for k, v in sd.items()})
    w = S.WORKLOADS[name]
    rest = dict(rest)
    bev_h, bev_w = rest.pop("bev_h"), rest.pop("bev_w")
    extra = {} if rotate_fn is None else dict(rotate_fn=rotate_fn)

    def fn(f, m, p):
        return O.get_bev_features(own, enc, f, bq, bev_h, bev_w, img_metas=m, prev_bev=p, pc_range=S.PC_RANGE,
                                  rotate_center=(w["bev_w"] // 2, w["bev_h"] // 2), **extra, **rest)
    info = {"prev_bev": None, "scene_token": None, "prev_pos": 0, "prev_angle": 0}
    out = []
    with torch.no_grad():
        for m in metas:
            out.append(O.forward_test_step(info, fn, mlvl, copy.deepcopy(m)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Exact-arithmetic sampling cases: every point on the quarter-pixel lattice, the map borders included
# ---------------------------------------------------------------------------------------------------------------------
# quanta of the operator's results on a lattice case: bilinear weights are multiples of 1/16, attention weights
# of 1/64, value / grad_out integers, level sides powers of two
LATTICE_QUANTA = dict(out=2.0 ** -10, grad_value=2.0 ** -10, grad_loc=2.0 ** -8, grad_attn=2.0 ** -4)

LATTICE_CASES = {
    # name: level shapes (H, W) — powers of two —, N, Q, M, D, P.  N = 2: the right / bottom neighbour of batch entry 0's last pixel
    # is real memory of entry 1.  Q: every lattice point of every level occurs at least twice (N * Q * M * P slots per level
    # >= twice its lattice: ``poison_locations`` may take one occurrence away),
    # N * Q = 300 rows = partial last workgroups of the 64- / 128- / 256-row grad_value kernel and a batch boundary inside one.
    "d32_p8": dict(shapes=[(8, 16), (4, 8), (2, 4), (1, 2)], N=2, Q=150, M=8, D=32, P=8),     # the D = 32 bodies, 8 points
    "d32_p4": dict(shapes=[(8, 16)], N=2, Q=150, M=8, D=32, P=4),                             # ... 4 points, one level
    "d32_grid": dict(shapes=[(32, 32)], N=2, Q=1024, M=8, D=32, P=4),                         # ... rows = the level's own grid
                                                                                              # (grad_value kernel: grid tiles)
    "generic_d8": dict(shapes=[(4, 8), (1, 1)], N=2, Q=101, M=3, D=8, P=3),                   # generic kernels, a 1 x 1 level
    "generic_d64": dict(shapes=[(4, 4), (2, 8)], N=2, Q=31, M=2, D=64, P=5),                  # generic kernels, 16 lanes per row
}


def lattice_points(H, W):
    """All (px, py) of the quarter-pixel lattice {-1.25, -1, ..., side, side + 0.25}^2 of an H x W level, float64 (n, 2)."""
    xs = torch.arange(-5, 4 * W + 2, dtype=torch.float64) / 4
    ys = torch.arange(-5, 4 * H + 2, dtype=torch.float64) / 4
    return torch.cartesian_prod(xs, ys)


def lattice_locations(shapes, slots, gen):
    """(slots, L, 2) float64 normalised locations ``(px + 0.5) / W``: per level the shuffled full lattice, repeated (each
    repeat shuffled again) to fill ``slots``."""
    loc = torch.empty(slots, len(shapes), 2, dtype=torch.float64)
    for l, (H, W) in enumerate(shapes):
        assert H & (H - 1) == 0 and W & (W - 1) == 0, "power-of-two sides: loc * W - 0.5 is then exact in fp32"
        pts = lattice_points(H, W)
        n = pts.shape[0]
        assert n <= slots, f"level {H}x{W}: {n} lattice points do not fit {slots} slots"
        idx = torch.cat([torch.randperm(n, generator=gen) for _ in range(-(-slots // n))])[:slots]
        loc[:, l] = (pts[idx] + 0.5) / torch.tensor([W, H], dtype=torch.float64)
    return loc


def make_lattice_case(shapes, N, Q, M, D, P, seed=0):
    """-> (value, shapes, level_start, loc, attn, grad_out) of an exact-arithmetic case: every product and partial sum of the
    operator and of its backward is a dyadic number of few bits, so the result does not depend on the summation order, on
    FMA contraction or on the order of atomics — kernels are compared with the oracle by ``torch.equal``."""
    gen = torch.Generator().manual_seed(seed)
    L = len(shapes)
    sh = torch.tensor(shapes, dtype=torch.long)
    start = torch.cat([sh.new_zeros(1), sh.prod(1).cumsum(0)[:-1]])
    S = int(sh.prod(1).sum())
    loc = lattice_locations(shapes, N * Q * M * P, gen).view(N, Q, M, P, L, 2).permute(0, 1, 2, 4, 3, 5).contiguous()
    loc32 = loc.float()
    assert torch.equal(loc32.double(), loc)
    value = torch.randint(-4, 5, (N, S, M, D), generator=gen).float()
    attn = torch.randint(0, 9, (N, Q, M, L, P), generator=gen).float() / 64
    gout = torch.randint(-2, 3, (N, Q, M * D), generator=gen).float()
    return value, sh, start, loc32, attn, gout


NONFINITE = (float("nan"), float("inf"), float("-inf"), 1e30, -1e30)


def poison_locations(loc, seed=0):
    """In place: 15 points of ``loc`` (..., 2) get NaN, +inf, -inf, 1e30, -1e30 in x only, in y only and in both — the first
    and the last point among them.  -> their flat point indices."""
    flat = loc.view(-1, 2)
    n = flat.shape[0]
    gen = torch.Generator().manual_seed(seed)
    idx = torch.cat([torch.tensor([0, n - 1]), 1 + torch.randperm(n - 2, generator=gen)[:13]])
    for i, p in enumerate(idx.tolist()):
        bad, where = NONFINITE[i % 5], i // 5
        if where in (0, 2):
            flat[p, 0] = bad
        if where in (1, 2):
            flat[p, 1] = bad
    return idx


def pixel_coordinates(sh, loc, dtype):
    """``loc * (W, H) - 0.5`` formed in ``dtype`` from the fp32 locations (N, Q, M, L, P, 2), as the kernels (fp32) and the C
    oracle (double) form them."""
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1).to(dtype)
    return loc.to(dtype) * wh[None, None, None, :, None, :] - 0.5


class _COracleMSDA(torch.autograd.Function):
    """The C oracle (oracle/msda_ref.c) under autograd: its forward and ITS backward — at a pixel centre or edge the location
    gradient is the slope of the floor cell, and a point outside (-1, W) x (-1, H) has none, which autograd through
    ``grid_sample`` does not reproduce."""

    @staticmethod
    def forward(ctx, value, shapes, loc, attn):
        from oracle import msda_c
        start = torch.cat([shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]])
        ctx.save_for_backward(value, shapes, start, loc, attn)
        return msda_c.forward(value, shapes, start, loc, attn)

    @staticmethod
    def backward(ctx, g):
        from oracle import msda_c
        gv, gl, ga = msda_c.backward(*ctx.saved_tensors, g)
        return gv, None, gl, ga


def c_oracle_msda(value, shapes, loc, attn):
    return _COracleMSDA.apply(value, shapes, loc, attn)


def make_lattice_fused_case(kind, seed=0, exact_softmax=False):
    """The fused entry point's operands (``_oracle_msda_fused``'s arguments) with every sampling location on the quarter-pixel
    lattice: dyadic reference points (multiples of 1/4) and offsets that are multiples of 1/4 px, so ``ref + off / (W, H)`` is
    exact.  ``kind``: "sca" (pillar anchors, ragged rows that share projection rows through ``row_src``) or "tsa" (two queue
    entries averaged).  Three rows have every point outside (-1, W) x (-1, H).  ``exact_softmax``: logits in {0, -200} with
    a power-of-two count of zeros per softmax — the weights are then exactly 0 or 1 / count and the whole call is exact.
    -> (value, shapes, start, proj, n_off, ref, row_batch, kwargs, grad_out)"""
    gen = torch.Generator().manual_seed(seed)
    M, D = 8, 32
    if kind == "sca":
        shapes, P, K, A, N, Rb, extra = [(8, 16), (4, 8), (2, 4), (1, 2)], 8, 1, 4, 2, 131, 42
    else:
        shapes, P, K, A, N, Rb, extra = [(8, 16)], 4, 2, 1, 4, 134, 0
    L = len(shapes)
    sh = torch.tensor(shapes, dtype=torch.long)
    start = torch.cat([sh.new_zeros(1), sh.prod(1).cumsum(0)[:-1]])
    S = int(sh.prod(1).sum())
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1).double()                                        # (L, 2) = (W, H)
    n_in = Rb - 3
    loc = lattice_locations(shapes, n_in * M * K * P, gen).view(n_in, M, K, P, L, 2).permute(0, 1, 2, 4, 3, 5)
    # three rows outside every map: x from {-1.25, -1, W, W + 0.25}, y anywhere on the lattice
    ox = torch.stack([torch.tensor([-1.25, -1.0, float(W), W + 0.25])[torch.randint(0, 4, (3, M, K, P), generator=gen)]
                      for H, W in shapes], 3)
    oy = torch.stack([(torch.randint(-5, 4 * H + 2, (3, M, K, P), generator=gen) / 4) for H, W in shapes], 3)
    outside = (torch.stack([ox, oy], -1).double() + 0.5) / wh[None, None, None, :, None, :]
    order = torch.cat([torch.tensor([n_in]), torch.arange(0, n_in // 2), torch.tensor([n_in + 1]),
                       torch.arange(n_in // 2, n_in), torch.tensor([n_in + 2])])              # outside rows first, middle, last
    loc = torch.cat([loc, outside])[order].contiguous()                                        # (Rb, M, K, L, P, 2)
    quarters = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)
    if kind == "sca":
        ref_b = quarters[torch.randint(0, 3, (Rb, 1, A, 2), generator=gen)]
        rp = ref_b[:, 0][:, torch.arange(P) % A]                                               # (Rb, P, 2)
        off = (loc[:, :, 0] - rp[:, None, None, :, :]) * wh[None, None, :, None, :]            # (Rb, M, L, P, 2)
        R = Rb + extra
        row_src = torch.cat([torch.arange(Rb), torch.randint(0, Rb, (extra,), generator=gen)]).to(torch.int32)
        ref = torch.cat([ref_b, quarters[torch.randint(0, 3, (extra, 1, A, 2), generator=gen)]])
        row_batch = torch.randint(0, N, (R,), generator=gen, dtype=torch.int32).sort()[0]
        kw = dict(M=M, L=L, P=P, K=K, Q=0, off_head=L * P * 2, off_k=0, lg_head=L * P, lg_k=0, ref_mode=0, vmul=1, vadd=0,
                  row_src=row_src)
    else:
        ref = quarters[torch.randint(0, 3, (Rb, K, L, 2), generator=gen)]
        off = (loc - ref[:, None, :, :, None, :]) * wh[None, None, None, :, None, :]           # (Rb, M, K, L, P, 2)
        R, row_batch = Rb, None
        kw = dict(M=M, L=L, P=P, K=K, Q=Rb // 2, off_head=K * L * P * 2, off_k=L * P * 2, lg_head=K * L * P, lg_k=L * P,
                  ref_mode=1, vmul=2, vadd=1)
    assert torch.equal(off * 4, (off * 4).round()), "offsets are multiples of a quarter pixel"
    n_off = M * K * L * P * 2
    G, LP = Rb * M * K, L * P
    if exact_softmax:
        rank = torch.rand(G, LP, generator=gen).argsort(-1).argsort(-1)
        count = LP >> torch.randint(0, 3, (G, 1), generator=gen)
        logits = torch.where(rank < count, 0.0, -200.0)
    else:
        logits = torch.randn(G, LP, generator=gen)
    proj = torch.cat([off.reshape(Rb, n_off).float(), logits.reshape(Rb, M * K * LP).float()], 1).contiguous()
    value = torch.randint(-4, 5, (N, S, M, D), generator=gen).float()
    gout = torch.randint(-2, 3, (R, M * D), generator=gen).float()
    return value, sh, start, proj, n_off, ref.float().contiguous(), row_batch, kw, gout


def fused_lattice_locations(sh, proj, n_off, ref, *, M, L, P, K, ref_mode, row_src=None, **_):
    """(R, K, M, L, P, 2) fp32 sampling locations of a fused case, by the contract's expression in fp32."""
    rows = proj if row_src is None else proj[row_src.long()]
    R = rows.shape[0]
    off = rows[:, :n_off].reshape(R, M, K, L, P, 2).permute(0, 2, 1, 3, 4, 5)
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1).float()
    ref = ref.reshape(R, K, -1, 2)
    A = ref.shape[2]
    if ref_mode == 0:
        rp = ref[:, :, torch.arange(P) % A]                                                    # (R, K, P, 2)
        return rp[:, :, None, None, :, :] + off / wh[None, None, None, :, None, :]
    return ref[:, :, None, :, None, :] + off / wh[None, None, None, :, None, :]


def _with_oracle(value, sh, start, loc, attn, gout):
    from oracle import msda_c
    gv, gl, ga = msda_c.backward(value, sh, start, loc, attn, gout)
    return dict(value=value, shapes=sh, start=start, loc=loc, attn=attn, grad_out=gout,
                out=msda_c.forward(value, sh, start, loc, attn), grad_value=gv, grad_loc=gl, grad_attn=ga)


@functools.lru_cache(maxsize=None)
def lattice_reference(name):
    """Operands and C-oracle results of ``LATTICE_CASES[name]``, computed once per process and shared (read-only)."""
    return _with_oracle(*make_lattice_case(**LATTICE_CASES[name], seed=1 + sorted(LATTICE_CASES).index(name)))


NONFINITE_CASES = ("d32_p8", "generic_d8")


@functools.lru_cache(maxsize=None)
def nonfinite_reference(name):
    """``lattice_reference(name)``'s case with 15 NaN / inf / 1e30 locations (``poison_locations``) -> the same dict + "bad"
    (flat point indices)."""
    value, sh, start, loc, attn, gout = make_lattice_case(**LATTICE_CASES[name], seed=11 + sorted(LATTICE_CASES).index(name))
    bad = poison_locations(loc, seed=5)
    return dict(_with_oracle(value, sh, start, loc, attn, gout), bad=bad)


@functools.lru_cache(maxsize=None)
def fused_lattice_reference(kind, exact_softmax):
    """A fused lattice case, its contract's result and — through the C oracle's backward — its gradients w.r.t. value / proj."""
    value, sh, start, proj, n_off, ref, rb, kw, gout = make_lattice_fused_case(kind, seed=7, exact_softmax=exact_softmax)
    v, pj = value.clone().requires_grad_(True), proj.clone().requires_grad_(True)
    out = _oracle_msda_fused(v, sh, start, pj, n_off, ref, rb, msda=c_oracle_msda, **kw)
    out.backward(gout)
    loc = fused_lattice_locations(sh, proj, n_off, ref, **kw)
    px = pixel_coordinates(sh, loc.permute(1, 0, 2, 3, 4, 5), torch.float32)                   # (K, R, M, L, P, 2)
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1).float()
    zero_rows = ((px <= -1) | (px >= wh[None, None, None, :, None, :])).any(-1).permute(1, 0, 2, 3, 4).flatten(1).all(1)
    return dict(value=value, shapes=sh, start=start, proj=proj, n_off=n_off, ref=ref, row_batch=rb, kw=kw, grad_out=gout,
                out=out.detach(), grad_value=v.grad, grad_proj=pj.grad, loc=loc, zero_rows=zero_rows.nonzero().flatten())
