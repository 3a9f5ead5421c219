"""No GPU: the switch of the decoder fast path (``modes.decoder_fused``) and its eligibility predicate
(``DetectionTransformerDecoder.fused_reject`` / ``decoder.fused_layer_reject``) on CPU-built modules.  The predicate
decides the device of the tensors LAST, so on the CPU the stock decoder with good arguments is turned down for exactly
that reason and every other condition shows with a reason of its own."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import bevformer_amd
from bevformer_amd import modes, ops
from bevformer_amd import synthetic as S
from bevformer_amd.modules.decoder import fused_layer_reject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ONLY = "not CUDA fp32 tensors"


def _stock(num_layers=2):
    return bevformer_amd.build_transformer_layer_sequence(S.reference_decoder_cfg(num_layers)).eval()


def _call(seed=0, nq=37, bs=2):
    q, qp, v, ref, shapes, start = S.make_decoder_inputs(12, 10, num_query=nq, bs=bs, seed=seed)
    return dict(query=q, key=None, value=v, query_pos=qp, reference_points=ref, spatial_shapes=shapes,
                level_start_index=start)


def _why(dec, **changes):
    kw = _call()
    kw.update(changes)
    with torch.no_grad():
        return dec.fused_reject(**kw)


def test_switch_is_off_by_default_and_follows_the_environment():
    env = {k: v for k, v in os.environ.items() if k != "BEVMSDA_DECODER_FUSED"}
    code = "from bevformer_amd import modes; print(modes.Modes().decoder_fused, modes.current().decoder_fused)"
    for value, want in ((None, "False False"), ("1", "True True"), ("0", "False False")):
        e = dict(env, **({"BEVMSDA_DECODER_FUSED": value} if value is not None else {}))
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want, (value, out.stdout, out.stderr)


def test_using_turns_it_on_for_the_calling_thread_only():
    before = ops.modes().decoder_fused
    with ops.using(decoder_fused=True):
        assert ops.modes().decoder_fused is True
        seen = []
        import threading
        t = threading.Thread(target=lambda: seen.append(modes.current().decoder_fused))
        t.start()
        t.join()
        assert seen == [before]
    assert ops.modes().decoder_fused == before


def test_stock_decoder_is_accepted_up_to_the_device():
    dec = _stock()
    assert all(fused_layer_reject(layer) is None for layer in dec.layers)
    assert _why(dec) == DEVICE_ONLY
    assert _why(dec, query_pos=None) == DEVICE_ONLY
    assert _why(dec, attn_masks=[None, None]) == DEVICE_ONLY
    assert _why(dec, img_metas=[{}], cls_branches=None) == DEVICE_ONLY          # what PerceptionTransformer passes along


def test_switch_on_leaves_a_cpu_call_on_the_module_path():
    """The predicate turns CPU tensors down, so the call reaches the modules — whose sampling has no CPU path."""
    dec = _stock()
    with torch.no_grad(), ops.using(decoder_fused=True), pytest.raises(RuntimeError, match="no CPU path"):
        dec(**_call())


def test_layer_variants_outside_the_conditions_are_rejected():
    assert fused_layer_reject(bevformer_amd.build_transformer_layer_sequence(S.decoder_cfg(2)).layers[0]) == "operation order"
    assert _why(bevformer_amd.build_transformer_layer_sequence(S.decoder_cfg(2)).eval()) == "operation order"

    def variant(edit, **cfg_changes):
        cfg = S.reference_decoder_cfg(1)
        cfg["transformerlayers"].update(cfg_changes)
        layer = bevformer_amd.build_transformer_layer_sequence(cfg).eval().layers[0]
        if edit is not None:
            edit(layer)
        return fused_layer_reject(layer)

    assert variant(None) is None
    assert "FFN" in variant(None, ffn_num_fcs=3)                                  # three-layer FFN
    assert "FFN" in variant(None, feedforward_channels=1024)
    attn = S.reference_decoder_cfg(1)["transformerlayers"]["attn_cfgs"]
    a4 = copy.deepcopy(attn)
    a4[0]["num_heads"] = 4
    assert "self-attention" in variant(None, attn_cfgs=a4)
    a2 = copy.deepcopy(attn)
    a2[1]["num_levels"] = 2
    assert "cross-attention" in variant(None, attn_cfgs=a2)
    ah = copy.deepcopy(attn)
    ah[1]["num_heads"] = 4
    assert "cross-attention" in variant(None, attn_cfgs=ah)
    assert variant(None, operation_order=("self_attn", "norm", "ffn", "norm", "cross_attn", "norm")) == "operation order"

    def no_mha(layer):
        layer.attentions[0].attn = nn.Identity()
    assert "nn.MultiheadAttention" in variant(no_mha)

    def batch_first(layer):
        layer.attentions[0].batch_first = True
    assert "self-attention" in variant(batch_first)

    def add_bias_kv(layer):
        layer.attentions[0].attn = nn.MultiheadAttention(256, 8, add_bias_kv=True)
    assert "self-attention" in variant(add_bias_kv)

    def other_cross(layer):
        layer.attentions[1] = copy.deepcopy(layer.attentions[0])
    assert "cross-attention" in variant(other_cross)

    def gelu(layer):
        layer.ffns[0].layers[0][1] = nn.GELU()
    assert "FFN" in variant(gelu)

    def no_identity(layer):
        layer.ffns[0].add_identity = False
    assert "FFN" in variant(no_identity)

    def group_norm(layer):
        layer.norms[1] = nn.GroupNorm(8, 256)
    assert "norms" in variant(group_norm)

    def no_affine(layer):
        layer.norms[2] = nn.LayerNorm(256, elementwise_affine=False)
    assert "norms" in variant(no_affine)


def test_one_odd_layer_among_stock_ones_rejects_the_call():
    dec = _stock(3)
    dec.layers[2].norms[0] = nn.LayerNorm(256, elementwise_affine=False)
    assert "norms" in _why(dec)


def test_call_arguments_outside_the_conditions_are_rejected():
    dec = _stock()
    kw = _call()
    assert dec.fused_reject(**kw) == "gradient mode is on"                        # (no torch.no_grad() here)
    dec.train()
    assert _why(dec) == "train() mode"
    dec.eval()
    dec.layers[1].train()
    assert _why(dec) == "train() mode"
    dec.eval()
    with ops.using(gemm="native"):
        assert "GEMM mode" in _why(dec)
    for mode in ("split", "bf16"):
        with ops.using(gemm=mode):
            assert _why(dec) == DEVICE_ONLY
    nq, bs = kw["query"].shape[:2]
    assert _why(dec, attn_masks=[torch.zeros(nq, nq, dtype=torch.bool), None]) == "attention mask"
    assert _why(dec, attn_masks=torch.zeros(nq, nq, dtype=torch.bool)) == "attention mask"
    assert _why(dec, key_padding_mask=torch.zeros(bs, 120, dtype=torch.bool)) == "key-padding mask"
    assert _why(dec, query_key_padding_mask=torch.zeros(bs, nq, dtype=torch.bool)) == "key-padding mask"
    ref = kw["reference_points"]
    assert "reference points" in _why(dec, reference_points=ref[..., :2])
    assert "reference points" in _why(dec, reference_points=torch.cat([ref, ref[..., :1]], -1))      # box-shaped
    assert "reference points" in _why(dec, reference_points=None)
    with torch.no_grad():
        assert dec.fused_reject(kw["query"], None, kw["value"], **{k: v for k, v in kw.items() if k not in ("query", "key", "value")}) \
            == "positional key / value"
    assert _why(dec, value=None) == "operand shapes"
    assert _why(dec, value=kw["value"][:, :1]) == "operand shapes"
    assert _why(dec, query_pos=kw["query_pos"][:5]) == "operand shapes"
    two = torch.tensor([[12, 10], [6, 5]])
    assert _why(dec, spatial_shapes=two, level_start_index=torch.tensor([0, 120])) == "not one BEV level"
    assert _why(dec, spatial_shapes=None) == "not one BEV level"
    assert _why(dec, query=kw["query"].double(), query_pos=kw["query_pos"].double()) == DEVICE_ONLY
