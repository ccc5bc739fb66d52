"""The ENAS child's convolution Functions (``ops/conv.py`` ``_ConvFn``, ``ops/dwconv.py`` ``_DwFn``,
``ops/enas_sepconv.py`` ``_SepFn``) serve a plain call and a call over the ``prep`` records of
``ops.enas_optim.ChildAdam`` from one body each. Held here, at the smallest shapes that take every branch:
the sequence of kernel bindings of a forward + backward on every path, written out; that the prepared path
reads and writes the optimizer's own buffers; that the two paths agree bit for bit where no atomics are
involved; the error of a layer with a record that is about to leave the HIP kernels; and, on the CPU, the
shared 'same' geometry against the formula."""
import pytest
import torch

gpu = pytest.mark.gpu

CONV = {"opt_type": "convolution", "num_filter": 8, "filter_size": 3, "stride": 1}
DW = {"opt_type": "depthwise_convolution", "filter_size": 3, "stride": 2, "depth_multiplier": 2}
SEP = {"opt_type": "separable_convolution", "num_filter": 16, "filter_size": 3, "stride": 1, "depth_multiplier": 1}
# op -> (Op config, input channels, map size)
OPS = {"conv8": (CONV, 8, 5), "conv3": (CONV, 3, 5), "dw": (DW, 8, 5), "sep": (SEP, 8, 8)}
# case -> (over prep records, x wants a gradient, the weights want one)
CASES = {"plain": (False, True, True), "plain-w-frozen": (False, True, False), "plain-x-none": (False, False, True),
         "prep": (True, True, True), "prep-x-none": (True, False, True)}

# What a forward + backward calls on the extension: (binding, its tensor arguments in order, "-" for an absent
# bias). Obtained by running record() below - this same body, through the ops' public functions - on the parent
# commit of the change that merged the plain and the prepared Functions; not taken from the code under test.
BIAS8, BIAS16, BIAS_SEP = ("channel_sum", "bf16[50,8] f32[8]"), ("channel_sum", "bf16[18,16] f32[16]"), (
    "channel_sum", "bf16[128,16] f32[16]")
ROWS, PLAN = ("dw_wgrad_rows", ""), ("sep_plan", "")
# convolution, Cin = 8 and Cin = 3 alike (3 channels are padded to 8 around the kernels); image [K][R][S][C8]
C_FWD = ("conv_fwd", "bf16[2,5,5,8] bf16[8,3,3,8] bf16[2,5,5,8]")
C_DGRAD = ("conv_dgrad", "bf16[2,5,5,8] bf16[8,3,3,8] bf16[2,5,5,8]")
C_WGRAD = ("conv_wgrad", "bf16[2,5,5,8] bf16[2,5,5,8] f32[8,72]")
CP_FWD = ("conv_fwd", "bf16[2,5,5,8] bf16[576] bf16[2,5,5,8]")  # the optimizer's images are flat
CP_DGRAD = ("conv_dgrad", "bf16[2,5,5,8] bf16[576] bf16[2,5,5,8]")
# depthwise: the optimizer's image and partials have the plain path's shapes
D_FWD = ("dw_fwd", "bf16[2,5,5,8] f32[9,16] f32[16] bf16[2,3,3,16]")
D_DGRAD = ("dw_dgrad", "bf16[2,3,3,16] f32[9,16] bf16[2,5,5,8]")
D_WGRAD = ("dw_wgrad", "bf16[2,5,5,8] bf16[2,3,3,16] f32[6,16,9]")
# fused separable
S_FWD = ("sep_fwd", "bf16[2,8,8,8] f32[9,8] bf16[16,8] f32[16] bf16[2,8,8,16]")
S_BWD = ("sep_bwd_pw", "bf16[2,8,8,8] f32[9,8] bf16[8,16] bf16[2,8,8,16] bf16[2,8,8,8] f32[16,8]")
SP_FWD = ("sep_fwd", "bf16[2,8,8,8] f32[9,8] bf16[128] f32[16] bf16[2,8,8,16]")
SP_BWD = ("sep_bwd_pw", "bf16[2,8,8,8] f32[9,8] bf16[128] bf16[2,8,8,16] bf16[2,8,8,8] f32[16,8]")
S_DGRAD = ("dw_dgrad", "bf16[2,8,8,8] f32[9,8] bf16[2,8,8,8]")
S_WGRAD = ("dw_wgrad", "bf16[2,8,8,8] bf16[2,8,8,8] f32[16,8,9]")
EXPECTED = {
    ("conv8", "plain"): [C_FWD, BIAS8, C_DGRAD, C_WGRAD],
    ("conv8", "plain-w-frozen"): [C_FWD, BIAS8, C_DGRAD],
    ("conv8", "plain-x-none"): [C_FWD, BIAS8, C_WGRAD],
    ("conv8", "prep"): [CP_FWD, BIAS8, CP_DGRAD, C_WGRAD],
    ("conv8", "prep-x-none"): [CP_FWD, BIAS8, C_WGRAD],
    ("conv3", "plain"): [C_FWD, BIAS8, C_DGRAD, C_WGRAD],
    ("conv3", "plain-w-frozen"): [C_FWD, BIAS8, C_DGRAD],
    ("conv3", "plain-x-none"): [C_FWD, BIAS8, C_WGRAD],
    ("dw", "plain"): [D_FWD, D_DGRAD, ROWS, D_WGRAD, BIAS16],
    ("dw", "plain-w-frozen"): [D_FWD, D_DGRAD, BIAS16],
    ("dw", "plain-x-none"): [D_FWD, ROWS, D_WGRAD, BIAS16],
    ("dw", "prep"): [D_FWD, D_DGRAD, ROWS, D_WGRAD, BIAS16],
    ("dw", "prep-x-none"): [D_FWD, ROWS, D_WGRAD, BIAS16],
    ("sep", "plain"): [PLAN, S_FWD, S_BWD, S_DGRAD, ROWS, S_WGRAD, BIAS_SEP],
    ("sep", "plain-w-frozen"): [PLAN, S_FWD, S_BWD, S_DGRAD, ROWS, BIAS_SEP],
    ("sep", "plain-x-none"): [PLAN, S_FWD, S_BWD, ROWS, S_WGRAD, BIAS_SEP],
    ("sep", "prep"): [PLAN, SP_FWD, SP_BWD, S_DGRAD, ROWS, S_WGRAD, BIAS_SEP],
    ("sep", "prep-x-none"): [PLAN, SP_FWD, SP_BWD, ROWS, S_WGRAD, BIAS_SEP],
}


def _sig(a):
    if a is None:
        return "-"
    return "%s[%s]" % ({torch.bfloat16: "bf16", torch.float32: "f32"}.get(a.dtype, str(a.dtype)),
                       ",".join(map(str, a.shape)))


class Recorder:
    """Replaces every binding of the extension by a wrapper that notes the call and still makes it."""

    def __init__(self, monkeypatch, k):
        self.calls = []
        for name in dir(k):
            fn = getattr(k, name)
            if not name.startswith("_") and callable(fn):
                monkeypatch.setattr(k, name, lambda *a, _n=name, _f=fn, **kw: self._call(_n, _f, a, kw))

    def _call(self, name, fn, a, kw):
        self.calls.append((name, [t for t in a if t is None or torch.is_tensor(t)]))
        return fn(*a, **kw)

    def sequence(self):
        return [(n, " ".join(_sig(t) for t in ts)) for n, ts in self.calls]

    def tensors(self, name):
        got = [ts for n, ts in self.calls if n == name]
        assert len(got) == 1, (name, len(got))
        return got[0]


def _setup(op_name, prepared):
    """A bare Op with seeded weights (under ChildAdam when ``prepared``), its input and output gradient."""
    from katib_amd.ops.enas_optim import ChildAdam
    from katib_amd.workloads.enas_child import Op

    cfg, cin, hw = OPS[op_name]
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    op = Op(cfg, cin, hw, sep="fused").to(dev)
    gen = torch.Generator().manual_seed(cin * 100 + hw)
    x = torch.randn(2, cin, hw, hw, generator=gen).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, op.cout, op.hw, op.hw, generator=gen).to(dev).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    opt = ChildAdam(op) if prepared else None
    return op, opt, x, gy


def _call(op_name, op, x):
    """The op's convolution through the public function of its module, with the layers' records where they have one."""
    from katib_amd.ops import conv as hconv, dwconv as hdw, enas_sepconv as hs

    first = op.body[0]
    if op_name == "sep":
        pw = op.body[1]
        return hs.separable_same(x, first.conv.weight, pw.weight, pw.bias, first.s,
                                 getattr(first, "prep", None), getattr(pw, "prep", None))
    fn = hdw.depthwise_same if op_name == "dw" else hconv.same_conv2d
    return fn(x, first.conv.weight, first.conv.bias, first.s, getattr(first, "prep", None))


def _weights(op_name, op):
    first = op.body[0]
    return [first.conv.weight] + ([op.body[1].weight] if op_name == "sep" else [])


def record(monkeypatch, op_name, case):
    """One forward + backward under the recorder -> (recorder, op, optimizer, x, y)."""
    from katib_amd.ops import conv as hconv

    prepared, xg, wg = CASES[case]
    op, opt, x, gy = _setup(op_name, prepared)
    for w in _weights(op_name, op):
        w.requires_grad_(wg)
    x.requires_grad_(xg)
    torch.cuda.synchronize()
    rec = Recorder(monkeypatch, hconv.kernels())
    y = _call(op_name, op, x)
    y.backward(gy)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return rec, op, opt, x, y


PAIRS = [(o, c) for o in OPS for c in CASES if not (o == "conv3" and CASES[c][0])]


@gpu
@pytest.mark.parametrize("op_name,case", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_launch_sequence_is_the_parents(monkeypatch, op_name, case):
    rec, op, opt, x, y = record(monkeypatch, op_name, case)
    got = rec.sequence()
    print(op_name, case, got)
    assert got == EXPECTED[(op_name, case)]
    assert (x.grad is not None) == CASES[case][1]
    if not CASES[case][0]:
        for w in _weights(op_name, op):
            assert (w.grad is not None) == CASES[case][2]
        return
    # the prepared arms: the optimizer's buffers themselves, and no gradient on the masters
    assert all(w.grad is None for w in _weights(op_name, op))
    first = op.body[0].prep
    if op_name == "conv8":
        assert rec.tensors("conv_fwd")[1].data_ptr() == first.wk.data_ptr()
        assert rec.tensors("conv_wgrad")[2].data_ptr() == first.g.data_ptr()
        if CASES[case][1]:
            assert rec.tensors("conv_dgrad")[1].data_ptr() == first.wt.data_ptr()
        return
    rows = rec.tensors("dw_wgrad")[2].shape[0]
    assert first.rows == rows and rec.tensors("dw_wgrad")[2].data_ptr() == first.partials(rows).data_ptr()
    if CASES[case][1]:
        assert rec.tensors("dw_dgrad")[1].data_ptr() == first.img.data_ptr()
    if op_name == "dw":
        assert rec.tensors("dw_fwd")[1].data_ptr() == first.img.data_ptr()
    else:
        pw = op.body[1].prep
        fwd, bwd = rec.tensors("sep_fwd"), rec.tensors("sep_bwd_pw")
        assert fwd[1].data_ptr() == first.img.data_ptr() and fwd[2].data_ptr() == pw.wk.data_ptr()
        assert bwd[1].data_ptr() == first.img.data_ptr() and bwd[2].data_ptr() == pw.wt.data_ptr()
        assert bwd[5].data_ptr() == pw.g.data_ptr()


@gpu
@pytest.mark.parametrize("op_name", ["conv8", "dw"])
def test_plain_and_prepared_agree(monkeypatch, op_name):
    """Same weights, same input: y and gx bit for bit (neither kernel uses atomics for them), and for the
    convolution the optimizer's accumulator against the plain weight gradient."""
    _, plain_op, _, xa, ya = record(monkeypatch, op_name, "plain")
    _, prep_op, opt, xb, yb = record(monkeypatch, op_name, "prep")
    assert torch.equal(plain_op.body[0].conv.weight, prep_op.body[0].conv.weight) and torch.equal(xa, xb)
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    if op_name == "conv8":
        assert torch.equal(opt.grads()["body.0.conv.weight"], plain_op.body[0].conv.weight.grad)


@gpu
def test_a_layer_with_a_record_does_not_fall_back():
    """A layer whose gradient buffers ChildAdam holds must not take the torch fallback, where autograd would
    fill the master's .grad and the optimizer read its own zero accumulator."""
    op, opt, x, _ = _setup("conv8", True)
    with pytest.raises(RuntimeError, match="ChildAdam"):
        op(x.cpu().float())
    bare = _setup("conv8", False)[0]
    with pytest.raises(Exception) as err:  # torch's own complaint about a CPU input to GPU weights
        bare(x.cpu().float())
    assert "ChildAdam" not in str(err.value)


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_same_geometry(k, s):
    from katib_amd.ops.conv import same_geometry

    for size in range(1, 10):
        out = (size + s - 1) // s
        total = max((out - 1) * s + k - size, 0)
        assert same_geometry(size, k, s) == (total // 2, total - total // 2, out), (size, k, s)
