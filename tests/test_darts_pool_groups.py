"""Which edges of a DARTS cell share their pooling (hip_darts.pool_groups): the plan itself, on the
static cell description - no tensors, no GPU. The forward pools each (state, stride) group once;
the backward forms the state's gradient from the group's live edges (hip_darts.live_edges) in one
pool_bwd_multi entry."""
import pytest

ALL = ["max_pooling_3x3", "avg_pooling_3x3", "skip_connection", "separable_convolution_3x3",
       "separable_convolution_5x5", "dilated_convolution_3x3", "dilated_convolution_5x5"]


def _cells(nodes, prims=ALL):
    from katib_amd.models.darts import DartsLayout, DartsNetwork
    from katib_amd.ops import hip_darts as hd

    layout = DartsLayout(prims, init_channels=4, num_layers=2, num_nodes=nodes, stem_multiplier=1)
    net = DartsNetwork(layout)
    return hd, net._cell_spec(hd, 0), net._cell_spec(hd, 1)  # (normal, reduction)


def _expected(nodes, red):
    """State s (0, 1 = the preprocessed inputs, 2 + j = node j) is read by edge s of every node that
    comes after it; the inputs of a reduction cell are read with stride 2."""
    exp = {}
    for s in range(2 + nodes - 1):
        members = [(i, s) for i in range(nodes) if s < 2 + i]
        exp[(s, 2 if red and s < 2 else 1)] = members
    return exp


@pytest.mark.parametrize("nodes", [3, 4])
def test_normal_cell_groups(nodes):
    hd, normal, _ = _cells(nodes)
    g = hd.pool_groups(normal)
    assert g == _expected(nodes, False)
    sizes = sorted(len(v) for v in g.values())
    # 3 nodes: 9 edges over 4 states (3, 3, 2, 1); 4 nodes: 14 edges over 5 states (4, 4, 3, 2, 1)
    assert sizes == ([1, 2, 3, 3] if nodes == 3 else [1, 2, 3, 4, 4])
    assert sum(sizes) == sum(len(n) for n in normal.nodes)
    assert max(sizes) <= hd.POOL_SHARE  # one entry per state in both configurations
    assert hd.pool_groups(normal) == g and list(hd.pool_groups(normal)) == list(g)  # pure, stable order


@pytest.mark.parametrize("nodes", [3, 4])
def test_reduction_cell_separates_strides(nodes):
    hd, _, red = _cells(nodes)
    g = hd.pool_groups(red)
    assert g == _expected(nodes, True)
    assert {k for k in g if k[1] == 2} == {(0, 2), (1, 2)}  # s0 / s1: stride 2
    assert all(k[1] == 1 for k in g if k[0] >= 2)  # node states: stride 1
    for (src, stride), members in g.items():
        for i, k in members:
            es, _, _, s, _ = red.nodes[i][k]
            assert s == src and es.stride == stride


def test_live_masks_from_needed_grads_with_detached_weights():
    """The architect's finite-difference passes: weights detached, d(alpha) only. The preprocessed
    inputs need no gradient, so the edges reading them are not live and their groups vanish; the
    node states keep theirs. With the cell's first input needed, its group comes back."""
    hd, normal, red = _cells(3)
    for spec in (normal, red):
        need = hd.needed_grads(spec, False, False, lambda n: False, True)
        assert need == [False, False, True, True, True]
        live = hd.live_edges(spec, need, lambda n: False)
        assert live == [[False, False], [False, False, True], [False, False, True, True]]
        assert hd.pool_groups(spec, live) == {(2, 1): [(1, 2), (2, 2)], (3, 1): [(2, 3)]}
        need = hd.needed_grads(spec, True, False, lambda n: False, True)
        live = hd.live_edges(spec, need, lambda n: False)
        g = hd.pool_groups(spec, live)
        s = 2 if spec is red else 1
        assert g[(0, s)] == [(0, 0), (1, 0), (2, 0)] and (1, s) not in g
    # a parameter of one edge keeps that edge live although its source state needs no gradient
    name = normal.nodes[1][0][1][0]
    need = hd.needed_grads(normal, False, False, lambda n: n == name, False)
    live = hd.live_edges(normal, need, lambda n: n == name)
    assert live == [[False, False], [True, False, False], [False, False, False, True]]
    assert hd.pool_groups(normal, live) == {(0, 1): [(1, 0)], (3, 1): [(2, 3)]}
    # a node that needs no gradient has no live edge
    need = [True, True, False, True, True]
    assert hd.live_edges(normal, need, lambda n: True)[0] == [False, False]
    # all weights and inputs: every edge
    need = hd.needed_grads(normal, True, True, lambda n: True, True)
    assert hd.pool_groups(normal, hd.live_edges(normal, need, lambda n: True)) == hd.pool_groups(normal)


def test_state_read_only_by_none_edges_has_no_group():
    """A state all of whose readers are ``none`` edges gets no entry (its gradient is the caller's
    to zero-fill); groups of mixed edges keep their non-``none`` members only."""
    hd, normal, _ = _cells(3)
    none = hd.EdgeSpec(["none"], 1, [], {})
    nodes = [[(none if src == 1 else es, pn, bn, src, row) for es, pn, bn, src, row in node] for node in normal.nodes]
    spec = hd.CellSpec(normal.pre0, normal.pre1, nodes, normal.C)
    g = hd.pool_groups(spec)
    assert all(k[0] != 1 for k in g)
    assert g[(0, 1)] == [(0, 0), (1, 0), (2, 0)] and g[(2, 1)] == [(1, 2), (2, 2)]
    # only node 2's edge from state 0 is `none`
    nodes = [[(none if (src == 0 and i == 2) else es, pn, bn, src, row) for es, pn, bn, src, row in node]
             for i, node in enumerate(normal.nodes)]
    g = hd.pool_groups(hd.CellSpec(normal.pre0, normal.pre1, nodes, normal.C))
    assert g[(0, 1)] == [(0, 0), (1, 0)]
