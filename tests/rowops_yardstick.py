"""Float64 yardsticks and shared inputs of the decoder's attention core (csrc/mha_d32.h) and of the row helpers
(csrc/rowops.h): plain statements of each operation on float64 CPU tensors, the yardstick ``E32`` (torch's OWN float32 CPU
evaluation against the float64 statement, on the same inputs: nothing of a kernel enters it), and the inputs of the exact
cases, whose premises tests/test_rowops_yardstick_cpu.py asserts by the reference alone.

Bound of every toleranced comparison: max abs error <= ``FACTOR`` x E32, the project's factor for a float32 reduction
in another order (tests/test_mha_gpu.py).  One exception, explained at ``ln_forward_case``: the LayerNorm forward multiplies
max(E32, E_mean), E_mean the cost of rounding a row's mean to float32."""
import functools
import math

import torch
import torch.nn.functional as F

FACTOR = 4.0

# ---------------------------------------------------------------------------------------------------------------------
# ops.mha
# ---------------------------------------------------------------------------------------------------------------------
HEADS, HEAD_DIM, EMBED = 8, 32, 256
MHA_SCALE = 1.0 / math.sqrt(HEAD_DIM)
CODE_BITS = 10                      # key j carries the +-1 binary code of j in the first 10 dimensions of every head
Q_GAIN = 512.0                      # winner's score - any other score >= 2 * 512 / sqrt(32) = 181: exp(-181) == 0 in float32

MHA_GRID = [(nq, nk, 1) for nq in (1, 31, 32, 33) for nk in (1, 16, 31, 32, 33, 255, 256, 257, 513)]
MHA_BATCHED = (33, 257, 3)
MHA_STRIDED = (40, 513, 2)          # q and k as the column blocks of one (n, bs, 512) tensor, v at a padded row stride
MHA_SHAPES = MHA_GRID + [MHA_BATCHED, MHA_STRIDED]
MHA_WIDE = [(33, 257, 3), (37, 900, 1)]
MHA_GAINS = (8.0, 30.0)
WINNER_MAPS = ("stride", "tail")


def heads(t, dtype=None):
    """(n, bs, E) -> (bs, HEADS, n, 32)"""
    n, bs, E = t.shape
    return (t if dtype is None else t.to(dtype)).view(n, bs, HEADS, E // HEADS).permute(1, 2, 0, 3)


def sdpa(q, k, v, dtype):
    """(n, bs, E) operands -> (nq, bs, E): per (batch, head) attention in ``dtype`` on the CPU (tests/test_mha_gpu.py's)."""
    o = F.scaled_dot_product_attention(heads(q, dtype), heads(k, dtype), heads(v, dtype))
    return o.permute(2, 0, 1, 3).reshape(q.shape)


def mha_e32(q, k, v):
    """-> (float64 attention, E32)"""
    want = sdpa(q, k, v, torch.float64)
    return want, (sdpa(q, k, v, torch.float32).double() - want).abs().max().item()


def key_code(n):
    """(n, CODE_BITS) of +-1: bit d of j set -> +1"""
    j = torch.arange(n)[:, None]
    return (((j >> torch.arange(CODE_BITS)[None, :]) & 1) * 2 - 1).float()


def winners(kind, nq, nk, bs):
    """(nq, bs, HEADS) long: the key every (query, batch entry, head) selects.  "stride": (7 i + 3) mod nk, "tail":
    nk - 1 - (i mod min(nk, 32)) — the last, partial key block and both lane halves —, each shifted per head and per batch
    entry so that a head or batch mix-up selects another row."""
    i = torch.arange(nq)[:, None, None]
    b = torch.arange(bs)[None, :, None]
    h = torch.arange(HEADS)[None, None, :]
    if kind == "stride":
        return (7 * i + 3 + 5 * h + 11 * b) % nk
    assert kind == "tail"
    return nk - 1 - (i + 3 * h + 7 * b) % min(nk, 32)


@functools.lru_cache(maxsize=None)
def selection_case(kind, nq, nk, bs):
    """-> (q, k, v, w, want): softmax(q k^T / sqrt(32)) is exactly one-hot at ``w``, ``want[i, b, head h] = v[w[i, b, h], b,
    head h]``.  Key j of (batch b, head h) is ``code(j) * sign[b, h]`` (a fixed +-1 pattern per (b, h)), query i is
    ``512 * code(w) * sign[b, h]``: with the right pairing of q and k the signs cancel and every score is 512 * (10 - 2 *
    Hamming distance of the codes), an exact integer."""
    assert nk <= 1 << CODE_BITS
    g = torch.Generator().manual_seed(1000 * nq + nk + bs + WINNER_MAPS.index(kind))
    sign = (torch.randint(0, 2, (bs, HEADS, CODE_BITS), generator=g) * 2 - 1).float()
    w = winners(kind, nq, nk, bs)
    code = key_code(max(nk, 1))
    k = torch.zeros(nk, bs, HEADS, HEAD_DIM)
    k[..., :CODE_BITS] = code[:, None, None, :] * sign[None]
    q = torch.zeros(nq, bs, HEADS, HEAD_DIM)
    q[..., :CODE_BITS] = Q_GAIN * code[w] * sign[None]
    v = torch.randn(nk, bs, HEADS, HEAD_DIM, generator=g)
    b = torch.arange(bs)[None, :, None]
    h = torch.arange(HEADS)[None, None, :]
    want = v[w, b, h]                                                   # (nq, bs, HEADS, 32)
    return q.view(nq, bs, EMBED), k.view(nk, bs, EMBED), v.view(nk, bs, EMBED), w, want.reshape(nq, bs, EMBED)


def scores64(q, k):
    """(bs, HEADS, nq, nk) float64 logits ``q k^T / sqrt(32)``"""
    return heads(q, torch.float64) @ heads(k, torch.float64).transpose(-1, -2) * MHA_SCALE


@functools.lru_cache(maxsize=None)
def uniform_case(nq, nk, bs):
    """-> (q, k, v, want64): all keys of a (batch, head) are one randn row, so every score of a query is the same float and
    every real key weighs exactly 1; v integers in {-4..4}: ``want64 = sum(v) / nk`` in float64, (nq, bs, E)."""
    g = torch.Generator().manual_seed(7000 + 1000 * nq + nk + bs)
    q = torch.randn(nq, bs, EMBED, generator=g)
    k = torch.randn(1, bs, EMBED, generator=g).expand(nk, bs, EMBED).contiguous()
    v = torch.randint(-4, 5, (nk, bs, EMBED), generator=g).float()
    want = (v.double().sum(0) / nk)[None].expand(nq, bs, EMBED).contiguous()
    return q, k, v, want


@functools.lru_cache(maxsize=None)
def wide_case(nq, nk, bs, gain):
    """randn operands with q times ``gain`` (logit standard deviation = gain) -> (q, k, v, float64 attention, E32)"""
    g = torch.Generator().manual_seed(9000 + nq + nk + bs)
    q = torch.randn(nq, bs, EMBED, generator=g) * gain
    k, v = torch.randn(nk, bs, EMBED, generator=g), torch.randn(nk, bs, EMBED, generator=g)
    return (q, k, v) + mha_e32(q, k, v)


def ulp32(x):
    """Spacing of float32 at |x| (float64 tensor in, float64 out; normal range)."""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x.abs().clamp_min(2.0 ** -126))[1] - 24)


# ---------------------------------------------------------------------------------------------------------------------
# add_layernorm, forward
# ---------------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (256, 512, 1024)
LN_ROWS = (1, 2, 3, 5, 9)
LN_FAMILIES = ("offset_1000", "offset_1", "cancelling", "tiny_variance", "eps_zero")
LN_CONSTANTS = (0.0, 1.0, -3.0, 2.0 ** -20)


def add32(x, res):
    """The kernel's contract for the sum: one float32 add."""
    return x if res is None else x + res


def ln_forward64(z, gamma, beta, eps):
    """LayerNorm over the last dimension of float32 ``z``, every step in float64."""
    z, gamma, beta = z.double(), gamma.double(), beta.double()
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + eps) * gamma + beta


def ln_one_pass32(z, gamma, beta, eps):
    """What a ONE-pass kernel would compute: var = E[z^2] - mean^2 in float32 (clamped at 0, the kindest reading).  The
    offset families must break the bound with it (tests/test_rowops_yardstick_cpu.py): they tell the two apart."""
    mean = z.mean(-1, keepdim=True)
    var = ((z * z).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
    return (z - mean) * torch.rsqrt(var + eps) * gamma + beta


def ln_e32(z, gamma, beta, eps, want):
    return (F.layer_norm(z, (z.shape[-1],), gamma, beta, eps).double() - want).abs().max().item()


def ln_e_mean(z, gamma, eps):
    """What rounding the row mean to float32 costs in the output, by the number format alone: the nearest float32 to the
    mean is up to 2^-24 |mean| away, ``out = (z - mean) * rstd * gamma + beta`` moves by ``gamma * rstd`` times that, the same
    amount in every column of the row.  Next to nothing for rows centred on 0 and the WHOLE error of a float32 LayerNorm
    for rows with |mean| >> sigma (1e-4 at mean 1000, sigma 1).  It is ONE number per row, somewhere between 0 and this
    value by the luck of that row's mean, for torch's float32 evaluation as for a kernel: E32 of a few rows is then a draw,
    not a scale (see ``ln_forward_case``)."""
    z = z.double()
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + eps)
    return (2.0 ** -24 * mean.abs() * rstd).max().item() * gamma.double().abs().max().item()


@functools.lru_cache(maxsize=None)
def ln_forward_case(family, rows, C, with_res):
    """-> dict(x, res, gamma, beta, eps, z, want, e32, e_mean, yard); ``None`` for a family that needs ``res`` when there is none.

    ``yard = max(E32, E_mean)`` is what the bound multiplies.  With E32 alone, 2 of the 135 cases miss 4 x E32 on an MI355X:
    offset_1 C=512 rows=1 with res (error 6.44e-5, E32 6.37e-6) and tiny_variance C=512 rows=1 (9.34e-6, 4.53e-7).  Cause,
    reproduced on the CPU by summing in the kernel's order: the kernel's mean (a float32 tree sum, then * 1/C) is the float32
    NEXT to the nearest one there (0.91 and 1.05 ulp off), torch's is the nearest (0.09 and 0.05 ulp off, by luck of the row:
    up to 0.5), and sigma is 1e-3 / 3e-3 of the mean, so that one ulp IS the error (6.44e-5 and 9.34e-6 with everything
    else in float64).  Nothing is wrong with either; a single row's E32 is a draw of one number in [0, E_mean].  E_mean comes
    from the number format alone (``ln_e_mean``); FACTOR x E_mean = 2 ulp of the mean.  Where rows are centred (cancelling,
    eps_zero) E_mean < E32 and the bound is 4 x E32 as before; a one-pass variance misses the bound on every case of the
    offset families, by 6 x where it comes closest (tests/test_rowops_yardstick_cpu.py asserts both)."""
    g = torch.Generator().manual_seed(100 * rows + C + 7 * LN_FAMILIES.index(family) + int(with_res))
    rn = lambda *s: torch.randn(*s, generator=g)
    eps = 1e-5
    res = rn(rows, C) if with_res else None
    if family == "offset_1000":
        x = rn(rows, C) + 1000.0
    elif family == "offset_1":
        x = rn(rows, C) * 1e-3 + 1.0
        res = res * 1e-3 if with_res else None
    elif family == "cancelling":
        if not with_res:
            return None
        x = rn(rows, C) * 3 + 0.5
        res = -x + 1e-3 * rn(rows, C)
    elif family == "tiny_variance":                    # row standard deviation 1e-4: the variance (1e-8) is far below eps
        x = rn(rows, C) * 1e-4 + 0.25
        res = res * 1e-5 if with_res else None
    else:
        assert family == "eps_zero"
        x, eps = rn(rows, C), 0.0
    gamma, beta = rn(C) * 0.3 + 1.0, rn(C) * 0.2
    z = add32(x, res)
    want = ln_forward64(z, gamma, beta, eps)
    e32, e_mean = ln_e32(z, gamma, beta, eps, want), ln_e_mean(z, gamma, eps)
    return dict(x=x, res=res, gamma=gamma, beta=beta, eps=eps, z=z, want=want, e32=e32, e_mean=e_mean, yard=max(e32, e_mean))


@functools.lru_cache(maxsize=None)
def ln_constant_case(C, with_res):
    """Rows equal to a constant c: the sum (C c) and the mean are exact in float32, z - mean is 0 and the output IS beta.
    With ``res`` the constant is split as (c - r) + r, r small integers: both addends and their sum exact.
    -> (x, res, gamma, beta): one row per constant of LN_CONSTANTS."""
    g = torch.Generator().manual_seed(C + int(with_res))
    z = torch.tensor(LN_CONSTANTS, dtype=torch.float64)[:, None].expand(-1, C)
    res = torch.randint(-4, 5, (len(LN_CONSTANTS), C), generator=g).double() if with_res else None
    x = z - res if with_res else z
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    return x.float().contiguous(), None if res is None else res.float(), gamma, beta


# ---------------------------------------------------------------------------------------------------------------------
# add_layernorm, backward
# ---------------------------------------------------------------------------------------------------------------------
BWD_WIDTHS = (256, 512)
BWD_ROWS = (1, 3, 5, 8192, 8193, 8197, 16389)      # 8192 rows: the last count at which every wavefront has one row
BWD_LIVE_ROWS = 8197
BWD_EPS = 1e-5


def ln_backward64(z, gamma, g, eps):
    """Gradients of ``y = LayerNorm(z) * gamma + beta`` for the incoming ``g``, written out in float64:
    -> (grad z, grad gamma, grad beta, xhat)."""
    z, gamma, g = z.double(), gamma.double(), g.double()
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (z - mean) * rstd
    gg = g * gamma
    gz = rstd * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))
    return gz, (g * xhat).sum(0), g.sum(0), xhat


def ln_autograd(x, res, gamma, beta, g, eps, dtype):
    """torch's own add + LayerNorm under autograd on the CPU in ``dtype`` -> (grad x, grad res, grad gamma, grad beta).
    In float64 the sum is still the float32 one (the kernel's contract)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)           # (never the caller's tensor: cases are shared)
    if dtype == torch.float32:
        x, res = leaf(x), leaf(res)
        z = x + res
    else:
        z = x = res = leaf(x.detach() + res.detach())
    gamma, beta = leaf(gamma), leaf(beta)
    F.layer_norm(z, (z.shape[-1],), gamma, beta, eps).backward(g.to(dtype))
    return x.grad, res.grad, gamma.grad, beta.grad


def bwd_errors32(x, res, gamma, beta, g, eps, want):
    """E32 per output: torch float32 autograd on the CPU against the float64 statement -> dict(gx, dgamma, dbeta)."""
    gx, gr, dg, db = ln_autograd(x, res, gamma, beta, g, eps, torch.float32)
    assert torch.equal(gx, gr)
    return dict(gx=(gx.double() - want[0]).abs().max().item(), dgamma=(dg.double() - want[1]).abs().max().item(),
                dbeta=(db.double() - want[2]).abs().max().item())


def bwd_operands(rows, C, seed=0):
    g = torch.Generator().manual_seed(rows + C + seed)
    x = torch.randn(rows, C, generator=g) * 2 + 0.5
    res = torch.randn(rows, C, generator=g)
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    return g, x, res, gamma, beta


@functools.lru_cache(maxsize=2)
def bwd_case(rows, C, kind="randn"):
    """-> dict(x, res, gamma, beta, g, g2, want=(gx, dgamma, dbeta) float64, e32=dict).  ``kind``: "randn" | "two" (the
    gradient arrives as g + g2, summed in float32 by torch: ``g`` is then that sum's first addend)."""
    gen, x, res, gamma, beta = bwd_operands(rows, C)
    g = torch.randn(rows, C, generator=gen)
    g2 = torch.randn(rows, C, generator=gen) * 0.5 if kind == "two" else None
    gsum = g if g2 is None else g + g2
    want = ln_backward64(x + res, gamma, gsum, BWD_EPS)[:3]
    return dict(x=x, res=res, gamma=gamma, beta=beta, g=g, g2=g2, gsum=gsum, want=want,
                e32=bwd_errors32(x, res, gamma, beta, gsum, BWD_EPS, want))


def bwd_lattice_case(rows, C):
    """``g`` integers in {-2..2}: every column sum of g stays below 2^24 in magnitude, so it is exact in float32 in any order.
    -> (x, res, gamma, g, float64 column sum of g)"""
    gen, x, res, gamma, _ = bwd_operands(rows, C, seed=1)
    g = torch.randint(-2, 3, (rows, C), generator=gen).float()
    return x, res, gamma, g, g.double().sum(0)


@functools.lru_cache(maxsize=2)
def bwd_live_row_case(C, r):
    """rows = BWD_LIVE_ROWS, ``g`` zero except row ``r`` -> as ``bwd_case`` + xhat64 of row r."""
    rows = BWD_LIVE_ROWS
    gen, x, res, gamma, beta = bwd_operands(rows, C, seed=2)
    g = torch.zeros(rows, C)
    g[r] = torch.randn(C, generator=gen)
    gz, dg, db, xhat = ln_backward64(x + res, gamma, g, BWD_EPS)
    want = (gz, dg, db)
    return dict(x=x, res=res, gamma=gamma, beta=beta, g=g, want=want, xhat_r=xhat[r],
                e32=bwd_errors32(x, res, gamma, beta, g, BWD_EPS, want))


def live_rows(rows=BWD_LIVE_ROWS):
    return (0, rows - 1, 8191, 8192)


# ---------------------------------------------------------------------------------------------------------------------
# gather_mean, rows_from_slots, cast_rows_bf16
# ---------------------------------------------------------------------------------------------------------------------
GATHER_SHAPES = [(1, 1, 1, 4), (3, 2, 5, 36), (65, 3, 40, 256), (50, 6, 90, 64)]     # (Q, J, R, C)


def gather_index(Q, J, R, seed=0):
    """(Q, J) int32 row ids, -1 = empty, with — wherever Q and J leave room — a query whose ids are all -1 (the last), a -1
    between two live ids (query 0, J >= 3) and the same row twice in one query (query 1 of J >= 2, or query 0 of a J = 2
    table)."""
    g = torch.Generator().manual_seed(Q + J + R + seed)
    idx = torch.randint(-1, R, (Q, J), generator=g, dtype=torch.int32)
    if J >= 3:
        idx[0, :3] = torch.tensor([R - 1, -1, 0], dtype=torch.int32)
    if J >= 2 and Q >= 2:
        idx[1, :2] = R // 2
    if Q >= 2:
        idx[-1] = -1
    return idx


def gather_mean32(rows, idx, scale):
    """The kernel's own order in float32 on the CPU: the J rows added in ascending j, one multiply."""
    out = torch.zeros(idx.shape[0], rows.shape[1], dtype=rows.dtype)
    for j in range(idx.shape[1]):
        sel = idx[:, j].long()
        ok = sel >= 0
        out[ok] = out[ok] + rows[sel[ok]]
    return out * scale.to(rows.dtype)[:, None]


def gather_case(Q, J, R, C, exact, seed=0):
    """-> (rows, idx, scale).  ``exact``: integer rows in {-8..8} and power-of-two scales — no rounding anywhere."""
    g = torch.Generator().manual_seed(Q * J + C + seed)
    idx = gather_index(Q, J, R, seed)
    if exact:
        rows = torch.randint(-8, 9, (R, C), generator=g).float()
        scale = torch.ldexp(torch.ones(Q), -torch.randint(0, 4, (Q,), generator=g))
    else:
        rows, scale = torch.randn(R, C, generator=g), torch.rand(Q, generator=g) + 0.1
    return rows, idx, scale


def device_counts(R):
    """Row counts tried: none (the host's R holds), and device-side counts around R, above it and negative."""
    return (None, 0, 1, R - 1, R, R + 5, -3)


def rows_written(count, R):
    """How many leading rows a kernel with a device-side row count writes."""
    return R if count is None else max(0, min(count, R))


# float32 bit patterns of the bf16 cast: ties to even both ways, just below / above a tie, a carry into the exponent, the
# largest finite value (rounds to inf), zeros, infinities, denormals
BF16_PATTERNS = (0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x3F7FFFFF, 0x7F7FFFFF, 0xFF7FFFFF,
                 0x7F7F8000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x00008000, 0x00018000,
                 0x007FFFFF, 0x807FFFFF, 0x00400000, 0xBF808000, 0xBF818000)
BF16_NANS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF)


def cast_case(R, C):
    """(R, C) float32: randn with the chosen bit patterns scattered over it -> (matrix, mask of the NaN entries)."""
    g = torch.Generator().manual_seed(R + C)
    a = torch.randn(R, C, generator=g)
    bits = torch.tensor(BF16_PATTERNS + BF16_NANS, dtype=torch.int64)
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    n = bits.numel()
    assert R * C >= 3 * n
    # three copies: the first entries, the last entries, and random places in between
    pos = torch.cat([torch.arange(n), R * C - 1 - torch.arange(n), n + torch.randperm(R * C - 2 * n, generator=g)[:n]])
    flat = a.view(-1).view(torch.int32)
    flat[pos] = bits.repeat(3)
    return a, torch.isnan(a)
