"""The ENAS child's head kernels (``csrc/hip/enas_head.hip``) against ``ops.enas_head.reference`` in
fp64 on the same bf16-rounded inputs, per row and within 4 times the error of ``reference`` in fp32
(at least one ulp), at the smallest shapes at which each path can go wrong; the keep pattern and the
hits exactly. The one CPU test anchors the oracle to torch's own ``cross_entropy``."""
import pytest
import torch
import torch.nn.functional as F

import gpt2_kernel_oracle as O

gpu = pytest.mark.gpu
SEED, SITE, STEP, G = 0x1234567890AB, 3, 5, 0.75
SHAPES = [(2, 1, 1, 8, 10),                        # a 1x1 map
          (3, 4, 4, 64, 10),                       # vector path
          (2, 5, 3, 24, 10),                       # three chunks do not divide 256; odd, non-square map
          (2, 2, 2, 3, 10), (2, 4, 4, 67, 10),     # element path, padded mask row
          (2, 2, 2, 2056, 3),                      # 257 chunks: the chunk loop, several weight workgroups
          (257, 1, 1, 8, 10),                      # batch loops of the sum kernel and of the dl tile
          (2, 2, 2, 8, 1), (2, 2, 2, 8, 64)]       # the ends of K


def _inputs(B, H, W, C, K, dev):
    gen = torch.Generator().manual_seed(B * 1000 + C + K)
    x = (torch.rand(B, C, H, W, generator=gen) + 0.25) * (torch.randint(0, 2, (B, C, 1, 1), generator=gen) * 2 - 1)
    x = x.to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)  # no zeros, no zero mean
    w = (torch.randn(K, C, generator=gen) * 0.3).to(dev)
    b = torch.randn(K, generator=gen).to(dev)
    return x, w, b, torch.randint(0, K, (B,), generator=gen).to(dev)


def _arm(x, w, b, y, p, dtype, train=True):
    """``reference`` in ``dtype`` with its gradients for the upstream gradient G -> (parts, dl, dx, dW, db)."""
    from katib_amd.ops.enas_head import Drop, reference

    x, w, b = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    r = reference(x, w, b, y, Drop(p, SITE, SEED, STEP), train)
    dl, = torch.autograd.grad(r.loss, r.logits, retain_graph=True)
    return (r, dl) + torch.autograd.grad(r.loss * G, (x, w, b))


def _check(got, ref, truth, what, row=O.ROW):
    O.assert_rows_close(got, ref, truth, row=row, what=what)


@gpu
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_against_fp64(shape, p):
    from katib_amd.ops import enas_head as hh

    dev = torch.device("cuda", 0)
    B, H, W, C, K = shape
    x, w, b, y = _inputs(*shape, dev)
    step, stats = torch.tensor([STEP], dtype=torch.int32, device=dev), torch.tensor([1.0, 2.0], device=dev)
    assert hh.supported(x, K)
    got = hh.forward_parts(x, w, b, y, hh.Drop(p, SITE, SEED, step), stats)
    dx, dw, db = hh.backward_parts(got, w, torch.tensor([G], device=dev), H, W, p)
    (t, tdl, tdx, tdw, tdb), (r, rdl, rdx, rdw, rdb) = _arm(x, w, b, y, p, torch.float64), _arm(x, w, b, y, p, torch.float32)
    assert torch.equal(got.keep.bool(), t.keep) and torch.equal(got.feat != 0, t.keep)
    if K > 1:  # one class: softmax = 1, every gradient is zero
        assert torch.equal(dx != 0, t.keep[:, :, None, None].expand_as(dx))
    assert torch.equal(got.hit_b, (got.logits.argmax(1) == y).float())
    for name, g_, r_, t_ in (("feat", got.feat, r.feat, t.feat), ("logits", got.logits, r.logits, t.logits),
                             ("dl", got.dl, rdl, tdl), ("dx", dx.flatten(1), rdx.flatten(1), tdx.flatten(1)),
                             ("loss_b", got.loss_b[None], r.loss_b[None], t.loss_b[None]),
                             ("loss", got.loss.view(1, 1), r.loss.view(1, 1), t.loss.view(1, 1)),
                             ("db", db[None], rdb[None], tdb[None])):
        _check(g_, r_, t_, name)
    _check(dw.reshape(-1), rdw.reshape(-1), tdw.reshape(-1), "dW", row=64)
    assert int(step) == STEP + 1 and float(got.hits) == float(got.hit_b.sum())
    assert torch.equal(stats, torch.stack([1.0 + got.loss, 2.0 + got.hits]))
    if shape == SHAPES[2]:  # evaluation: no draw, sums, the counter untouched
        ls, hits = hh.head_eval(x, w, b, y)
        te, re = _arm(x, w, b, y, p, torch.float64, False)[0], _arm(x, w, b, y, p, torch.float32, False)[0]
        _check(ls.view(1, 1), re.loss.view(1, 1), te.loss.view(1, 1), "eval loss")
        own = hh.forward_parts(x, w, b, y, train=False)
        assert int(step) == STEP + 1 and float(hits) == float((own.logits.argmax(1) == y).sum())


@gpu
def test_equal_logits_hit_class_zero():
    from katib_amd.ops import enas_head as hh

    dev = torch.device("cuda", 0)
    x, w, b, _ = _inputs(3, 2, 2, 8, 10, dev)
    y = torch.tensor([0, 4, 0], device=dev)
    got = hh.forward_parts(x, torch.zeros_like(w), torch.full_like(b, 0.5), y)
    assert torch.equal(got.hit_b, (y == 0).float()) and float(got.hits) == 2.0


def _grads(x, w, b, y, step, p=0.4, xg=True, wg=True):
    from katib_amd.ops import enas_head as hh

    step.fill_(STEP)
    x, w, b = x.detach().requires_grad_(xg), w.detach().requires_grad_(wg), b.detach().requires_grad_(True)
    loss = hh.head_loss(x, w, b, y, hh.Drop(p, SITE, SEED, step))
    loss.backward()
    return loss.detach(), x.grad, w.grad, b.grad


@gpu
def test_bits_and_skipped_gradients():
    from katib_amd.ops import enas_head as hh

    dev = torch.device("cuda", 0)
    x, w, b, y = _inputs(3, 4, 4, 64, 10, dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    full = _grads(x, w, b, y, step)
    assert all(torch.equal(a, c) for a, c in zip(full, _grads(x, w, b, y, step)))  # two runs from one state
    nox, now = _grads(x, w, b, y, step, xg=False), _grads(x, w, b, y, step, wg=False)
    assert nox[1] is None and all(torch.equal(nox[i], full[i]) for i in (0, 2, 3))
    assert now[2] is None and all(torch.equal(now[i], full[i]) for i in (0, 1, 3))
    whole = hh.forward_parts(x, w, b, y)  # p = 0: a row does not depend on the batch it sits in
    one = torch.ones(1, device=dev)  # three uneven pixel segments per sample write what one segment writes
    assert torch.equal(hh.backward_parts(whole, w, one, 4, 4, 0.0, segs=3)[0], hh.backward_parts(whole, w, one, 4, 4, 0.0)[0])
    for i in range(3):
        alone = hh.forward_parts(x[i:i + 1].contiguous(memory_format=torch.channels_last), w, b, y[i:i + 1])
        assert torch.equal(alone.logits[0], whole.logits[i]) and torch.equal(alone.loss_b[0], whole.loss_b[i])


@gpu
def test_counter_under_replay():
    from katib_amd.ops import enas_head as hh
    from katib_amd.ops.transformer import dropout_mask
    from katib_amd.utils.graphcheck import capture

    dev = torch.device("cuda", 0)
    B, H, W, C, K = 4, 3, 3, 24, 10
    x, w, b, y = _inputs(B, H, W, C, K, dev)
    x.requires_grad_(True)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    drop = hh.Drop(0.4, SITE, SEED, step)
    torch.autograd.grad(hh.head_loss(x, w, b, y, drop), x)  # eager warm-up: counts as the step it is
    assert int(step) == 1
    step.fill_(STEP)
    graph = torch.cuda.CUDAGraph()
    with capture(graph):
        dx, = torch.autograd.grad(hh.head_loss(x, w, b, y, drop), x)
    for s in (STEP, STEP + 1):
        graph.replay()
        keep = dropout_mask(B, C, 0.4, SITE, SEED, s, dev)
        assert torch.equal(dx != 0, keep[:, :, None, None].expand_as(dx)), s
    hh.head_eval(x.detach(), w, b, y)
    assert int(step) == STEP + 2


EMB = {"0": {"opt_type": "convolution", "filter_size": "3", "num_filter": "32", "stride": "1"},
       "1": {"opt_type": "reduction", "reduction_type": "max_pooling", "pool_size": 2}}
NN_CONFIG = {"num_layers": 2, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": EMB}
ARCH = [[0], [1, 0]]


@gpu
def test_child_trainer_head_hip():
    from katib_amd.ops.enas_head import reference
    from katib_amd.workloads.enas_child import ChildTrainer

    out = {}
    for head in ("module", "hip"):
        tr = ChildTrainer(ARCH, NN_CONFIG, num_train=256, num_valid=64, batch_size=32, capture=False, seed=5, head=head)
        tr.model.drop.p = 0.0
        idx = torch.arange(32, device=tr.dev)
        if head == "module":  # the truth, from the weights before the step
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                feats = tr.model.features(tr.tx.index_select(0, idx))
            fc = tr.model.fc
            wt = fc.weight.detach().double().requires_grad_(True)
            tl = reference(feats.double(), wt, fc.bias.detach().double(), tr.ty.index_select(0, idx)).loss
            tg, = torch.autograd.grad(tl, wt)
        tr.step(idx)
        out[head] = (tr.acc_buf[0].detach().view(1, 1).clone(), tr.model.fc.weight.grad.clone())
    _check(out["hip"][0], out["module"][0], tl.detach().view(1, 1), "step loss")
    _check(out["hip"][1].reshape(-1), out["module"][1].reshape(-1), tg.reshape(-1), "fc.weight.grad", row=64)
    tr = ChildTrainer(ARCH, NN_CONFIG, num_train=256, num_valid=64, batch_size=32, capture=True, seed=5, head="hip")
    for s in range(tr.step_fn.warmup + 3):
        tr.step(torch.arange(32, device=tr.dev) + 32 * (s % 8))
    assert tr.step_fn.graph is not None and int(tr.step_t) == tr.step_fn.warmup + 3
    vl, va = tr.validate()
    assert bool(torch.isfinite(torch.cat([tr.acc_buf.cpu(), torch.tensor([vl, va])])).all()) and 0.0 <= va <= 1.0


def test_reference_is_cross_entropy_of_the_pooled_linear():
    from katib_amd.ops.enas_head import reference

    gen = torch.Generator().manual_seed(0)
    x, w, b = (torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_(True) for s in ((5, 7, 3, 2), (4, 7), (4,)))
    y = torch.randint(0, 4, (5,), generator=gen)
    r = reference(x, w, b, y)
    logits = F.linear(F.avg_pool2d(x, (3, 2)).flatten(1), w, b)
    want = F.cross_entropy(logits, y)
    assert abs(float(r.loss - want)) <= 1e-12 and torch.equal(r.hit_b, (logits.argmax(1) == y).double())
    for a, c in zip(torch.autograd.grad(r.loss, (x, w, b)), torch.autograd.grad(want, (x, w, b))):
        assert float((a - c).abs().max()) <= 1e-12
