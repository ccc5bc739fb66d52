"""graphcheck.capture: Python's cyclic garbage collector never runs inside a HIP-graph capture.

Stale garbage (a trainer in a reference cycle with its captured step keeps its CUDAGraph alive
until a collection) is collected before the capture begins, the collector is off while it runs
and back in its earlier state afterwards - so no object of earlier work is destroyed by a
capturing thread. The package captures only through this helper."""
import gc
import os
import re
import weakref

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Node:
    pass


def _cycle():
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    return weakref.ref(a)


@pytest.mark.gpu
def test_capture_collects_before_and_keeps_the_collector_off_inside():
    from katib_amd.utils.graphcheck import capture

    dev = torch.device("cuda", 0)
    x = torch.ones(64, device=dev)
    torch.cuda.synchronize()
    assert gc.isenabled()
    gc.collect()
    gc.disable()  # (so that only the helper can have collected the cycle below)
    try:
        stale = _cycle()
        assert stale() is not None
        gc.enable()
        g = torch.cuda.CUDAGraph()
        with capture(g):
            assert stale() is None  # collected before the capture began
            assert not gc.isenabled()
            inside = _cycle()
            y = x * 2 + 1
        assert gc.isenabled()
        assert inside() is not None  # nothing was collected while capturing
        gc.collect()
        assert inside() is None
    finally:
        gc.enable()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(x, 3.0))


@pytest.mark.gpu
def test_capture_restores_a_disabled_collector_and_survives_an_error():
    from katib_amd.utils.graphcheck import capture

    x = torch.ones(8, device="cuda:0")
    torch.cuda.synchronize()
    gc.disable()
    try:
        with capture(torch.cuda.CUDAGraph()):
            x + 1
        assert not gc.isenabled()  # it was off before: it stays off
    finally:
        gc.enable()
    with pytest.raises(ValueError):
        with capture(torch.cuda.CUDAGraph()):
            x + 1
            raise ValueError("inside the capture")
    assert gc.isenabled()
    torch.cuda.synchronize()


def test_the_package_captures_only_through_the_helper():
    pat = re.compile(r"torch\.cuda\.graph\(|\.capture_begin\(")
    hits = []
    for base, _, files in os.walk(os.path.join(ROOT, "katib_amd")):
        for f in files:
            if f.endswith(".py"):
                p = os.path.join(base, f)
                for i, line in enumerate(open(p, encoding="utf-8"), 1):
                    if pat.search(line) and not line.lstrip().startswith("#"):
                        hits.append("%s:%d" % (os.path.relpath(p, ROOT), i))
    assert hits == ["katib_amd/utils/graphcheck.py:%d" % n for n in _helper_lines()], hits


def _helper_lines():
    p = os.path.join(ROOT, "katib_amd", "utils", "graphcheck.py")
    return [i for i, line in enumerate(open(p, encoding="utf-8"), 1) if "with torch.cuda.graph(graph" in line]
