"""GPU: ``bench.py --dump-outputs`` writes what the last timed step computed.  With a static rig every step computes the
same frame, so the dump of the replayed HIP graph (whose output and gradients live in the graph's memory pool) must
equal the dump of eager launches: forward output bit-equal, gradients to the atomic-accumulation tolerance of
tests/test_encoder_gpu.py (2e-3 of each tensor's max).  Two runs with the same arguments dump the same forward output."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _dump(tmp_path, name, *extra):
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "2", "--warmup", "1",
           "--static-rig", "--dump-outputs", str(out), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(os.listdir(out))
    assert files and all(f.endswith(".npy") for f in files)
    return {f[:-4]: np.load(out / f) for f in files}


def test_forward_dump_of_the_graph_equals_eager_and_repeats(tmp_path):
    a = _dump(tmp_path, "graph_a")
    b = _dump(tmp_path, "graph_b")
    e = _dump(tmp_path, "eager", "--graph", "off")
    assert list(a) == list(b) == list(e) == ["bev_embed"]
    assert a["bev_embed"].dtype == np.float32 and a["bev_embed"].shape == (1, 50 * 50, 256)
    assert np.isfinite(a["bev_embed"]).all() and np.abs(a["bev_embed"]).max() > 0
    assert np.array_equal(a["bev_embed"], b["bev_embed"])
    assert np.array_equal(a["bev_embed"], e["bev_embed"])


def test_backward_dump_of_the_graph_equals_eager(tmp_path):
    g = _dump(tmp_path, "graph", "--backward")
    e = _dump(tmp_path, "eager", "--backward", "--graph", "off")
    assert list(g) == list(e)
    assert {"bev_embed", "grad_bev_query", "grad_feats"} <= set(g)
    assert any(k.startswith("grad.") for k in g)
    assert np.array_equal(g["bev_embed"], e["bev_embed"])
    for k in g:
        assert g[k].dtype == np.float32 and g[k].shape == e[k].shape, k
        assert np.isfinite(g[k]).all(), k
        scale = np.abs(e[k]).max()
        assert np.abs(g[k] - e[k]).max() <= 2e-3 * scale + 1e-7, (k, np.abs(g[k] - e[k]).max(), scale)
    assert np.abs(g["grad_bev_query"]).max() > 0 and np.abs(g["grad_feats"]).max() > 0
