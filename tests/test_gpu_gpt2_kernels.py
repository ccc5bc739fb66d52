"""The GPT-2 trial kernels (csrc/hip/transformer.hip) against the fp64 oracle of
tests/gpt2_kernel_oracle.py, row by row, at the shapes where their loops, tails and path switches
sit: the second row of a LayerNorm-backward wave and its second grid-stride iteration, the first
element counts at which the flat kernels loop, both fused cross-entropy widths and the two-pass
fallback, an argmax tie across waves, attention with an odd number of query blocks, forced and
avoided online-softmax rescales. Truth (fp64) and reference arm (fp32) are computed on the GPU."""
import pytest
import torch

import gpt2_kernel_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SEED = (3 << 32) | 77  # both Philox key words in use


@pytest.fixture(scope="module")
def hip():
    from katib_amd.ops.transformer import HipOps

    return HipOps()


def _gen(seed=3):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


def _check(name, got, ref, truth, row=O.ROW):
    assert got.dtype == ref.dtype, (name, got.dtype, ref.dtype)
    return O.assert_rows_close(got, ref, truth, margin=O.margin_for(name), row=row, what=name)


def _col(x):
    return x.reshape(-1, 1)


# ============================================================================== LayerNorm
def _ln_inputs(M, D, big_mean=False, seed=3):
    g = _gen(seed)
    x = _randn(g, M, D) * (0.5 if big_mean else 2.0) + (300.0 if big_mean else 0.5)
    r = _randn(g, M, D).to(BF16)
    gamma = (1 + 0.1 * _randn(g, D)).to(BF16)
    beta = (0.1 * _randn(g, D)).to(BF16)
    dy = _randn(g, M, D).to(BF16)
    G0 = _randn(g, M, D)
    return x, r, gamma, beta, dy, G0


def _ln_check_fwd(name, got, x, r, gamma, beta, keep=None, scale=1.0):
    ref, tru = (arm.ln_fwd(x, r, gamma, beta, keep=keep, scale=scale) for arm in (O.REF, O.TRUTH))
    M = x.shape[0]
    _check(name + " xin", got[0], ref[0], tru[0], row=x.shape[1])
    _check(name + " y", got[1], ref[1], tru[1], row=x.shape[1])
    _check(name + " mean", got[2], ref[2], tru[2])
    _check(name + " rstd", got[3], ref[3], tru[3])
    assert got[2].shape == (M,) and got[3].shape == (M,)


def _ln_run_bwd(hip, dy, xin, mean, rstd, gamma, G0, accumulate, dbias, drop=None):
    M, D = xin.shape
    G = G0.clone()
    dr = torch.full((M, D), 7.0, device=DEV, dtype=BF16)
    dg, db, dbi = (torch.full((D,), 7.0, device=DEV, dtype=BF16) for _ in range(3))
    hip.ln_bwd(dy, xin, mean, rstd, gamma, G, dr, dg, db, accumulate=accumulate, dbias=dbi if dbias else None, drop=drop)
    return {"G": G, "dr": dr, "dgamma": dg, "dbeta": db, "dbias": dbi if dbias else None}


def _ln_check_bwd(name, got, dy, xin, mean, rstd, gamma, G0, accumulate, keep=None, scale=1.0):
    D = xin.shape[1]
    ref, tru = (arm.ln_bwd(dy, xin, mean, rstd, gamma, G0, accumulate=accumulate, keep=keep, scale=scale)
                for arm in (O.REF, O.TRUTH))
    for k in ("G", "dr"):
        _check("%s %s" % (name, k), got[k], ref[k], tru[k], row=D)
    for k in ("dgamma", "dbeta", "dbias"):
        if got[k] is not None:
            _check("%s %s" % (name, k), got[k], ref[k], tru[k], row=64)


# M = 1029: the second row of a wave (row0 + 1024) is valid for 5 rows only; 2051: a second
# grid-stride iteration (rows 2048..) with 3 rows; D = 2048 with dbias: red[0] reused in LDS
LN_CASES = [(256, 1), (256, 5), (256, 1029), (256, 2051), (768, 2051), (2048, 5), (2048, 1029)]


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("D,M", LN_CASES)
def test_layernorm(hip, D, M, residual):
    x, r, gamma, beta, dy, G0 = _ln_inputs(M, D)
    r = r if residual else None
    got = hip.ln_fwd(x, r, gamma, beta)
    if residual:
        assert torch.equal(got[0], x + r.float())  # one fp32 add
    else:
        assert got[0] is x
    _ln_check_fwd("ln_fwd", got, x, r, gamma, beta)
    xin, _, mean, rstd = got
    for accumulate in (True, False):
        for dbias in (False, True):
            out = _ln_run_bwd(hip, dy, xin, mean, rstd, gamma, G0, accumulate, dbias)
            _ln_check_bwd("ln_bwd", out, dy, xin, mean, rstd, gamma, G0, accumulate)


def test_layernorm_large_mean(hip):
    """Rows of mean 300 and standard deviation 0.5: a one-pass variance E[x^2] - mu^2 loses them."""
    M, D = 1029, 256
    x, r, gamma, beta, dy, G0 = _ln_inputs(M, D, big_mean=True)
    got = hip.ln_fwd(x, None, gamma, beta)
    _ln_check_fwd("ln_fwd mean300", got, x, None, gamma, beta)
    _, _, mean, rstd = got
    out = _ln_run_bwd(hip, dy, x, mean, rstd, gamma, G0, True, True)
    _ln_check_bwd("ln_bwd mean300", out, dy, x, mean, rstd, gamma, G0, True)


def test_layernorm_bwd_partials(hip):
    """D = 2048 through the binding: asking for the bias-gradient partials (which reuse red[0] after a
    barrier) leaves the dgamma / dbeta partials bit for bit what they are without them, writes every
    partial row, and ln_reduce of the partials is what HipOps.ln_bwd returns."""
    M, D = 1029, 2048
    x, r, gamma, beta, dy, G0 = _ln_inputs(M, D)
    xin, _, mean, rstd = hip.ln_fwd(x, r, gamma, beta)
    nb = hip.k.ln_bwd_blocks(M)
    assert nb == 256
    parts = []
    for want in (False, True):
        part = torch.full((3, nb, D), float("nan"), device=DEV)
        G, dr = G0.clone(), torch.empty(M, D, device=DEV, dtype=BF16)
        hip.k.ln_bwd(dy, xin, mean, rstd, gamma, G, G, dr, part[0], part[1], part[2] if want else None)
        parts.append((part, G, dr))
    (p0, Ga, dra), (p1, Gb, drb) = parts
    assert torch.equal(p0[:2], p1[:2]) and torch.equal(Ga, Gb) and torch.equal(dra, drb)
    assert bool(torch.isfinite(p1).all()) and bool(torch.isnan(p0[2]).all())
    ref, tru = (arm.ln_bwd(dy, xin, mean, rstd, gamma, G0) for arm in (O.REF, O.TRUTH))
    for k, name in enumerate(("dgamma", "dbeta", "dbias")):
        _check("ln_bwd partials " + name, p1[k].sum(0).to(BF16), ref[name], tru[name], row=64)
    dg, db, dbi = (torch.empty(D, device=DEV, dtype=BF16) for _ in range(3))
    hip.k.ln_reduce(p1[0], p1[1], dg, db, p1[2], dbi)
    out = _ln_run_bwd(hip, dy, xin, mean, rstd, gamma, G0, True, True)
    assert torch.equal(dg, out["dgamma"]) and torch.equal(db, out["dbeta"]) and torch.equal(dbi, out["dbias"])


@pytest.mark.parametrize("third", [False, True])
@pytest.mark.parametrize("nblk", [1, 15, 16, 17, 256])
def test_ln_reduce(hip, nblk, third):
    D = 256
    g = _gen(nblk)
    part = _randn(g, 3, nblk, D)
    out = [torch.full((D,), 7.0, device=DEV, dtype=BF16) for _ in range(3)]
    hip.k.ln_reduce(part[0], part[1], out[0], out[1], part[2] if third else None, out[2] if third else None)
    for k in range(3 if third else 2):
        _check("ln_reduce", out[k], O.REF.ln_reduce(part[k]), O.TRUTH.ln_reduce(part[k]), row=64)
    if not third:
        assert bool((out[2] == 7.0).all())


def test_layernorm_dropout_rows_past_1024(hip):
    """ln_fwd_drop / ln_bwd_drop at M = 2051: the mask on rows from 1024 upwards (the second row of a
    backward wave and its second iteration) is the oracle's, element for element."""
    from katib_amd.ops.transformer import Drop, dropout_mask, dropout_scale

    M, D, p, site, step = 2051, 256, 0.5, 5, 3
    drop = Drop(p, site, SEED, torch.full((1,), float(step), device=DEV))
    keep, scale = dropout_mask(M, D, p, site, SEED, step, DEV), dropout_scale(p)
    g = _gen(9)
    x = _randn(g, M, D) * 2 + 0.5
    r = (torch.rand(M, D, device=DEV, generator=g) + 0.5).to(BF16)  # never 0
    gamma = (1 + 0.1 * _randn(g, D)).to(BF16)
    beta = (0.1 * _randn(g, D)).to(BF16)
    dy = (0.1 * _randn(g, M, D)).to(BF16)
    sign = torch.where(torch.rand(M, D, device=DEV, generator=g) < 0.5, -1.0, 1.0)
    G0 = sign * (3.0 + torch.rand(M, D, device=DEV, generator=g))  # |G0 + dx| > 1: dr != 0 wherever it is kept
    got = hip.ln_fwd(x, r, gamma, beta, drop=drop)
    assert torch.equal(got[0] == x, ~keep)
    _ln_check_fwd("ln_fwd_drop", got, x, r, gamma, beta, keep=keep, scale=scale)
    xin, _, mean, rstd = got
    out = _ln_run_bwd(hip, dy, xin, mean, rstd, gamma, G0, True, True, drop=drop)
    assert torch.equal(out["dr"] == 0, ~keep)
    assert torch.equal((out["dr"] == 0)[1024:], ~keep[1024:]) and not bool(keep[1024:].all())
    _ln_check_bwd("ln_bwd_drop", out, dy, xin, mean, rstd, gamma, G0, True, keep=keep, scale=scale)


# (256, 5): the tail row of a workgroup; (256, 1029): the half-valid second row of a backward wave;
# (2048, 5): the widest instantiation
@pytest.mark.parametrize("D,M", [(256, 5), (256, 1029), (2048, 5)])
def test_layernorm_drop_p0_is_plain(hip, D, M):
    """The two branches of each LayerNorm template compute the same thing: at p = 0 (thr = 0 keeps
    every element, scale = 1.0f, and t + 1.0 * r, 1.0 * o round as t + r, o, fused or not) the
    dropped entry points, called straight through the binding, give the plain ones' bits."""
    x, r, gamma, beta, dy, G0 = _ln_inputs(M, D)
    step = torch.full((1,), 3.0, device=DEV)
    nb = hip.k.ln_bwd_blocks(M)

    def run(drop):  # outputs start as NaN, which equals nothing: an element left unwritten fails below
        tail = (0.0, 5, SEED, step) if drop else ()
        nan = float("nan")
        xo, y = torch.full_like(x, nan), torch.full((M, D), nan, device=DEV, dtype=BF16)
        mean, rstd = torch.full((M,), nan, device=DEV), torch.full((M,), nan, device=DEV)
        (hip.k.ln_fwd_drop if drop else hip.k.ln_fwd)(x, r, xo, gamma, beta, y, mean, rstd, 1e-5, *tail)
        G, dr = G0.clone(), torch.full((M, D), nan, device=DEV, dtype=BF16)
        part = torch.full((3, nb, D), nan, device=DEV)
        (hip.k.ln_bwd_drop if drop else hip.k.ln_bwd)(dy, xo, mean, rstd, gamma, G, G, dr, part[0], part[1], part[2],
                                                      *tail)
        return {"xo": xo, "y": y, "mean": mean, "rstd": rstd, "dx": G, "dr": dr, "part_g": part[0],
                "part_b": part[1], "part_r": part[2]}

    plain, dropped = run(False), run(True)
    assert torch.equal(plain["xo"], x + r.float())
    for k in plain:
        assert torch.equal(dropped[k], plain[k]), k


# ============================================================================== GELU
def test_gelu_first_looping_size(hip):
    """n = 8 * 256 * 4096 + 40: grid_for caps at 4096 workgroups of 256 threads x 8 elements, so the
    last 40 elements are the first a thread reaches in a second iteration; the special values sit at
    both ends."""
    n = 8 * 256 * 4096 + 40
    g = _gen(4)
    u = (torch.rand(n, device=DEV, generator=g) * 24 - 12).to(BF16)
    special = torch.tensor([0.0, -0.0, 3.0, -3.0, 8.0, -8.0, O.bf16_near(2.99), O.bf16_near(-2.99), O.bf16_near(3.01),
                            O.bf16_near(-3.01), O.bf16_near(7.99), O.bf16_near(-7.99), O.bf16_near(8.03),
                            O.bf16_near(-8.03), 12.0, -12.0], device=DEV).to(BF16)
    u[:16] = special
    u[n - 16:] = special
    dy = _randn(g, n).to(BF16)
    yh, dh = hip.gelu_fwd(u), hip.gelu_bwd(u, dy)
    _check("gelu_fwd", yh, O.REF.gelu_fwd(u), O.TRUTH.gelu_fwd(u))
    _check("gelu_bwd", dh, O.REF.gelu_bwd(u, dy), O.TRUTH.gelu_bwd(u, dy))
    assert float(yh[0]) == 0.0 and float(yh[1]) == 0.0 and float(yh[n - 16]) == 0.0


# ============================================================================== cross-entropy
# 16384: xent_fused switches from 4 to 13 vectors per thread above it; 53248: the last width it takes,
# wider rows go to xent_fwd + xent_bwd
XENT_CASES = [(1, 8), (8, 8), (16373, 16384), (16384, 16384), (16385, 16392), (53248, 53248), (53249, 53256)]
GSCALE = 0.7


def _xent_rows(V, Vp, extra=0):
    """Row 0: random x 3; 1: all equal; 2: one logit +60 (the target), the rest -60; 3: the target at
    column 0; 4: the target at V - 1. Pad columns +100."""
    g = _gen(V)
    N = 5 + extra
    logits = (_randn(g, N, Vp) * 3).to(BF16)
    tgt = torch.randint(0, V, (N,), device=DEV, generator=g)
    logits[1] = 1.5
    hot = (2 * V) // 3
    logits[2] = -60.0
    logits[2, hot] = 60.0
    tgt[2], tgt[3], tgt[4] = hot, 0, V - 1
    logits[:, V:] = 100.0
    return logits, tgt


def _xent_check(name, V, logits, tgt, loss, lse, grad):
    """Every check runs; the failures are reported together."""
    (lr, sr), (lt, st) = (arm.xent_fwd(logits, tgt, V) for arm in (O.REF, O.TRUTH))
    gr, gt = O.REF.xent_bwd(logits, tgt, GSCALE, V), O.TRUTH.xent_bwd(logits, tgt, GSCALE, V)
    failed = []
    for what, args, row in ((" loss", (_col(loss), _col(lr), _col(lt)), 1), (" lse", (_col(lse), _col(sr), _col(st)), 1),
                            (" grad", (grad, gr, gt), logits.shape[1])):
        try:
            _check(name + what, *args, row=row)
        except AssertionError as e:
            failed.append(str(e))
    if V < logits.shape[1] and float(grad[:, V:].abs().max()) != 0.0:
        failed.append("pad columns of the gradient are not 0")
    if V == 1 and float(loss.abs().max()) != 0.0:
        failed.append("V = 1: loss %r is not exactly 0" % loss.tolist())
    if V == 1 and float(grad.abs().max()) != 0.0:
        failed.append("V = 1: gradient %r is not exactly 0" % grad[:, 0].tolist())
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("V,Vp", XENT_CASES)
def test_cross_entropy_two_pass(hip, V, Vp):
    logits, tgt = _xent_rows(V, Vp)
    gs = torch.full((1,), GSCALE, device=DEV)
    loss, lse = hip.xent_fwd(logits, tgt, V)
    grad = hip.xent_bwd(logits.clone(), tgt, lse, gs, V)
    _xent_check("xent_fwd/bwd", V, logits, tgt, loss, lse, grad)


@pytest.mark.parametrize("V,Vp", XENT_CASES)
def test_cross_entropy_train(hip, V, Vp):
    logits, tgt = _xent_rows(V, Vp)
    gs = torch.full((1,), GSCALE, device=DEV)
    work = logits.clone()
    loss, lse, grad = hip.xent_train(work, tgt, gs, V)
    assert grad is work
    _xent_check("xent_train", V, logits, tgt, loss, lse, grad)
    # the fused kernel takes rows up to 53248 wide and refuses the next width
    probe = logits.clone()
    fused = hip.k.xent_fused(probe, tgt, torch.empty_like(loss), torch.empty_like(lse), gs, 1.0 / logits.shape[0], V)
    assert fused == (Vp <= 53248)
    assert fused or torch.equal(probe, logits)


@pytest.mark.parametrize("V,Vp", [(2408, 2408)] + [c for c in XENT_CASES if c[0] >= 2408])
def test_cross_entropy_eval(hip, V, Vp):
    """Rows 5 and 6 tie their maximum between column 561 (thread 70, wave 1) and column 2400 (thread
    44 of wave 0, in its second pass): the lower index sits in the later wave, so the merge across
    waves has to compare indices. The target is 561 in row 5 (a hit) and 2400 in row 6 (a miss)."""
    logits, tgt = _xent_rows(V, Vp, extra=2)
    logits[5:7, 561] = 40.0
    logits[5:7, 2400] = 40.0
    tgt[5], tgt[6] = 561, 2400
    tgt[0] = logits[0, :V].float().argmax()  # and an ordinary hit
    N = logits.shape[0]
    out = torch.empty((2, 8), device=DEV)
    hip.k.xent_eval(logits, tgt, out[0, :N], out[1, :N], V)
    (lr, hr), (lt, ht) = (arm.xent_eval(logits, tgt, V) for arm in (O.REF, O.TRUTH))
    _check("xent_eval loss", _col(out[0, :N]), _col(lr), _col(lt))
    assert torch.equal(out[1, :N].double(), ht), (out[1, :N], ht)
    assert ht[5] == 1 and ht[6] == 0 and ht[0] == 1 and ht[2] == 1
    s_loss, s_hit = hip.xent_eval(logits, tgt, V)
    assert float(s_hit) == float(ht.sum())
    assert abs(float(s_loss) - float(lt.sum())) <= 1e-5 * float(lt.sum())


# ============================================================================== attention
# T = 384: an odd number of 128-query blocks, 6 key tiles; B * H = 6 and 3 are no multiples of 8
ATTN_CASES = [(1, 128, 1), (3, 256, 2), (1, 384, 3)]


def _attn_check(name, hip, qkv, do, B, T, H, drop=None, keep=None, scale=1.0):
    oh, lh = hip.attn_fwd(qkv, B, T, H, drop=drop)
    (orf, lr), (ot, lt) = (arm.attn_fwd(qkv, B, T, H, keep=keep, scale=scale) for arm in (O.REF, O.TRUTH))
    _check(name + " o", O.head_rows(oh, B, T, H), O.head_rows(orf, B, T, H), O.head_rows(ot, B, T, H))
    _check(name + " lse", _col(lh), _col(lr), _col(lt))
    # the kernels' own o and lse, as in training; o is an input of the contract, so both arms get the same one
    dh = hip.attn_bwd(qkv, oh, do, lh, B, T, H, drop=drop)
    dr = O.REF.attn_bwd(qkv, oh, do, B, T, H, keep=keep, scale=scale)
    dt = O.TRUTH.attn_bwd(qkv, oh, do, B, T, H, keep=keep, scale=scale)
    for part in range(3):
        _check("%s d%s" % (name, "qkv"[part]), *(O.head_rows(z, B, T, H, part) for z in (dh, dr, dt)))
    return oh, lh, dh


@pytest.mark.parametrize("B,T,H", ATTN_CASES)
def test_attention(hip, B, T, H):
    g = _gen(B * T + H)
    qkv = _randn(g, B * T, 3 * H * 64).to(BF16)
    do = _randn(g, B * T, H * 64).to(BF16)
    oh, _, _ = _attn_check("attn", hip, qkv, do, B, T, H)
    # one key: p = 1 and 1 / l = 1, so the first output row is v[b, 0] bit for bit
    v0 = qkv.view(B, T, 3, H, 64)[:, 0, 2]
    assert torch.equal(oh.view(B, T, H, 64)[:, 0], v0)


@pytest.mark.parametrize("B,T,H", ATTN_CASES)
def test_attention_dropout(hip, B, T, H):
    from katib_amd.ops.transformer import Drop, attn_dropout_mask, attn_dropout_scale

    p, site, step = 0.5, 2 * H + 1, 4
    drop = Drop(p, site, SEED, torch.full((1,), float(step), device=DEV))
    keep, scale = attn_dropout_mask(B, H, T, p, site, SEED, step, DEV), attn_dropout_scale(p)
    g = _gen(B * T + H + 1)
    qkv = _randn(g, B * T, 3 * H * 64).to(BF16)
    do = _randn(g, B * T, H * 64).to(BF16)
    oh, lh, _ = _attn_check("attn_drop", hip, qkv, do, B, T, H, drop=drop, keep=keep, scale=scale)
    assert torch.equal(lh, hip.attn_fwd(qkv, B, T, H)[1])  # lse is that of the undropped softmax
    # a query row all of whose visible keys are dropped is exactly zero
    causal = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    dead = ~(keep & causal).any(-1)  # [B, H, T]
    assert bool(dead.any())  # at step 4 every case has one (row 0 of some head: its only key is dropped)
    assert float(oh.view(B, T, H, 64).permute(0, 2, 1, 3)[dead].abs().max()) == 0.0


def _rescale_case(late):
    """One query row (200) attends almost only to one key whose score, 2 * 2 * 64 / 8 = 32 (46 in log2
    units), is far over kLazy = 8 above the others'. late: the key is 190, in tile 2, so the running
    maximum jumps after two tiles and the accumulators are rescaled; else the key is 5, in tile 0, and
    every later tile stays below the lazy threshold."""
    B, T, H = 1, 256, 1
    g = _gen(11)
    x = _randn(g, B * T, 3 * 64) * 0.5
    x[200, :64] = 2.0
    x[190 if late else 5, 64:128] = 2.0
    return x.to(BF16), _randn(g, B * T, 64).to(BF16), B, T, H


@pytest.mark.parametrize("late", [True, False])
def test_attention_forced_rescale(hip, late):
    qkv, do, B, T, H = _rescale_case(late)
    _, lh, _ = _attn_check("attn rescale " + ("late" if late else "early"), hip, qkv, do, B, T, H)
    assert float(lh[0, 0, 200]) > 40.0


def test_attention_near_one_hot(hip):
    B, T, H = 1, 256, 2
    g = _gen(13)
    x = _randn(g, B * T, 3, H, 64)
    x[:, :2] *= 4.0  # q and k: scores ~ N(0, 16^2 / ...) - each row is close to one key
    _attn_check("attn one-hot", hip, x.view(B * T, 3 * H * 64).to(BF16), _randn(g, B * T, H * 64).to(BF16), B, T, H)


# ============================================================================== AdamW and the sums
ADAM = dict(b1=0.9, b2=0.95, eps=1e-8, wd=0.1, max_norm=1.0)


def _adamw_grad(g, n, mode):
    """"exact": values in {0, +-0.5, +-1}, norm 1450 - their squares sum exactly in fp32 in any order
    (every partial sum is a multiple of 0.25 below 2^24 * 0.25), so the clip coefficient does not
    depend on the order in which grad_sumsq's atomics land. "generic": normal values, norm 2048.
    "unclipped": normal values of norm 0.2."""
    if mode == "exact":
        return (torch.randint(-2, 3, (n,), device=DEV, generator=g).float() * 0.5).to(BF16)
    return (_randn(g, n) * (1.0 if mode == "generic" else 1e-4)).to(BF16)


@pytest.mark.parametrize("mode", ["exact", "generic", "unclipped"])
def test_adamw_first_looping_size(hip, mode):
    """n = 4 * 256 * 4096 + 104: the last 104 elements are reached in a second grid-stride iteration.
    Three steps through HipOps.adamw (zero, grad_sumsq, adamw).

    With generic clipped gradients the fp32 sum of 4 M squares moves by about 1e-6 of itself with the
    order of grad_sumsq's atomics, the clip coefficient by half of that, and m and v follow: v reached
    4.1 times the reference arm's error in one run and 2.2 in another. p does not: m / sqrt(v) is
    invariant under a scale of the gradient. So that case holds p to the checker, and m and v, element
    by element, to the bound of the sum itself: delta = (1 + 2^-24)^L - 1 with L = 8 (one iteration of
    8 elements per thread: 2049 workgroups x 256 threads cover n / 8 vectors) + 6 (wave tree) + 3 (LDS)
    + 2049 (serial atomics), 1.2e-4. v, a sum of non-negative terms g^2 clip^2, is within delta of
    itself; m, a sum of terms g clip of either sign, within delta / 2 of the same sum over |g|; both
    plus 8 ulp for the three steps' own fp32 roundings (at most 3 per step and 4 in the coefficient).
    The "exact" case holds m and v to the checker with the clip active."""
    n = 4 * 256 * 4096 + 104
    g = _gen(5)
    p0 = _randn(g, n)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    w16 = torch.empty(n, device=DEV, dtype=BF16)
    lr, step, ss = torch.full((1,), 1e-2, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ref, tru = (p0, m.clone(), v.clone()), (p0, m.clone(), v.clone())
    mabs = (p0, m.clone(), v.clone())  # the truth's m over |g|: the same clip, no cancellation
    for t in (1, 2, 3):
        gr = _adamw_grad(g, n, mode)
        want = float(O.TRUTH.grad_sumsq(gr))
        assert (want < 0.1) if mode == "unclipped" else (want > 1e6)
        step += 1
        hip.adamw(p, gr, m, v, w16, lr, step, ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], ADAM["max_norm"], ss)
        ref = O.REF.adamw(ref[0], gr, ref[1], ref[2], lr, t, **ADAM)[:3]
        tru = O.TRUTH.adamw(tru[0], gr, tru[1], tru[2], lr, t, **ADAM)[:3]
        mabs = O.TRUTH.adamw(mabs[0], gr.abs(), mabs[1], mabs[2], lr, t, **ADAM)[:3]
        if mode == "exact":
            assert float(ss) == want  # exact, and zeroed before each step
        else:
            assert abs(float(ss) - want) <= 1e-3 * want
    _check("adamw p " + mode, p, ref[0], tru[0])
    if mode == "generic":
        delta = (1 + 2.0 ** -24) ** (8 + 6 + 3 + 2049) - 1
        em = ((m.double() - tru[1]).abs() / mabs[1].clamp_min(1e-300)).max()
        ev = ((v.double() - tru[2]).abs() / tru[2].clamp_min(1e-300)).max()
        print("adamw generic: m err %.3e (bound %.3e), v err %.3e (bound %.3e)"
              % (float(em), delta / 2 + 2.0 ** -20, float(ev), delta + 2.0 ** -20))
        assert float(em) <= delta / 2 + 2.0 ** -20 and float(ev) <= delta + 2.0 ** -20
    else:
        _check("adamw m " + mode, m, ref[1], tru[1])
        _check("adamw v " + mode, v, ref[2], tru[2])
    assert torch.equal(w16, p.to(BF16))


def test_grad_sumsq_bound_and_accumulation(hip):
    """n = 8 * 256 * 4096 + 40 against fp64. Every term is non-negative, so whatever the order, the
    relative error is at most (1 + 2^-24)^L - 1 with L the longest chain of additions a term passes:
    a thread runs at most 2 iterations (4096 workgroups x 256 threads x 8 elements < n) of 8 elements,
    each one addition (squares of bf16 values are exact in fp32): 16; the wave tree: 6; the LDS sum
    (sh0 + sh1) + (sh2 + sh3): counted as 3; one atomic per workgroup, serial in the worst case: 4096.
    The kernel adds to what is there (HipOps.adamw zeroes it first): a second call doubles the value
    through a chain of 8192 atomics."""
    n = 8 * 256 * 4096 + 40
    gr = _randn(_gen(6), n).to(BF16)
    want = float(O.TRUTH.grad_sumsq(gr))
    ss = torch.zeros(1, device=DEV)
    hip.k.grad_sumsq(gr, ss)
    one = float(ss)
    hip.k.grad_sumsq(gr, ss)
    two = float(ss)
    u = 2.0 ** -24
    for got, target, chain in ((one, want, 16 + 6 + 3 + 4096), (two, 2 * want, 16 + 6 + 3 + 8192)):
        bound = (1 + u) ** chain - 1
        print("grad_sumsq rel err %.3e, bound %.3e" % (abs(got - target) / target, bound))
        assert abs(got - target) <= bound * target, (got, target, bound)


@pytest.mark.parametrize("R", [1, 2, 9])  # 9: a remainder after the unroll of 8
def test_reduce_rows(hip, R):
    n = 260
    part = _randn(_gen(R), R, n)
    out = torch.full((n,), 7.0, device=DEV, dtype=BF16)
    hip.k.reduce_rows(part, out)
    _check("reduce_rows", out, O.REF.reduce_rows(part), O.TRUTH.reduce_rows(part))


# one row and one column vector; the row-group tail; 17 column vectors (the second column block is
# mostly idle); many chunks with a ragged last one
@pytest.mark.parametrize("M,N", [(1, 8), (17, 8), (1000, 136), (4099, 2056)])
def test_colsum(hip, M, N):
    x = _randn(_gen(M), M, N).to(BF16)
    out = torch.full((N,), 7.0, device=DEV, dtype=BF16)
    hip.colsum(x, out)
    _check("colsum", out, O.REF.colsum(x), O.TRUTH.colsum(x))
