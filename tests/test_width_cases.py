"""The cases of width_cases.py on the CPU: each width case puts its node_dim / edge_dim where its name says in the operand image's
slot formula, each layout is what its role says, and every forward case is well conditioned -- the float32 oracle is within a
quarter of the 1e-5 forward bar of the float64 restatement, so that the bar, applied to the GPU, tests the kernel and not the
conditioning of the case.  Seeds and weights were fixed here, under this condition, not by looking at GPU results."""
import numpy as np
import pytest
import torch

import width_cases as wc
from conftest import BOUNDS, STATS
from oracle import epd_oracle as orc
from oracle import torch_epd


def test_slot_formula_covers_every_feature_once():
    for n_ks in (wc.NODE_KS, wc.EDGE_KS):
        f = sorted(int(wc.slot_feature(ks, kg, j)) for ks in range(n_ks) for kg in range(2) for j in range(8))
        assert f == list(range(16 * n_ks))
    # the four runs of 4 inside a k-group, in feature order
    assert [(kg, j) for f in (0, 4, 8, 12) for kg in range(2) for j in range(8) if wc.slot_feature(0, kg, j) == f] == [(0, 0), (1, 0), (0, 4), (1, 4)]
    assert wc.NODE_KS * 16 == wc.NODE_CAP and wc.EDGE_CAP <= wc.EDGE_KS * 16


@pytest.mark.parametrize("name", list(wc.WIDTHS))
def test_width_case_is_where_its_name_says(name):
    wc.check_width_case(name)


def test_width_cases_cover_the_issue_list():
    assert sorted(d for d, _ in wc.WIDTHS.values()) == sorted([(22, 4, 3), (1, 1, 1), (4, 2, 2), (8, 8, 4), (16, 3, 1), (17, 5, 2), (31, 7, 4), (32, 8, 4)])
    assert {wc.WIDTHS[k][0][0] for k in wc.WIDTHS} >= {1, 17, 32} and {wc.WIDTHS[k][0][1] for k in wc.WIDTHS} >= {1, 8}


@pytest.mark.parametrize("kind", list(wc.GRAPHS))
def test_graph_inputs_are_in_their_regime(kind):
    n, ei = wc.graph(kind)
    assert n == wc.GRAPHS[kind][0] and ei.dtype == np.int64 and 0 <= ei.min() and ei.max() < n
    deg = np.bincount(ei[1], minlength=n) + np.bincount(ei[0], minlength=n)
    assert deg[wc.ISOLATED] == 0 and (np.delete(deg, wc.ISOLATED) > 0).all()
    assert ei.shape[1] % 32 != 0 and ei.shape[1] > 128                 # more than one block, the last one partial
    if kind == "ragged":
        assert np.bincount(ei[1], minlength=n).max() <= 3                # almost only self edges
    else:
        assert np.bincount(ei[1], minlength=n).max() >= 20
    for name in wc.WIDTHS:
        nodes, ea, ei2 = wc.inputs(name, kind)
        assert nodes.dtype == np.float32 and nodes.shape == (n, wc.WIDTHS[name][0][0]) and ea.shape == (ei.shape[1], wc.WIDTHS[name][0][1])
        assert not nodes[wc.ZERO_ROW].any() and not ea[wc.ZERO_ROW].any()
        mx = np.abs(nodes).max(axis=1)
        assert mx[list(wc.SMALL_ROWS)].max() < 1e-2 and mx[list(wc.LARGE_ROWS)].min() > 30.0   # the per-row scale differs by 2^12 and more
        assert np.isfinite(nodes).all() and np.isfinite(ea).all()


@pytest.mark.parametrize("hidden", (wc.HIDDEN,) + wc.OTHER_HIDDEN)
@pytest.mark.parametrize("name", list(wc.WIDTHS))
def test_forward_case_is_well_conditioned(name, hidden):
    """|float32 oracle - float64 restatement| <= 0.25 * 1e-5 * max |ref|: a quarter of the forward bar."""
    for kind in ("dense", "ragged") if (hidden == wc.HIDDEN and name in wc.RAGGED) else ("dense",):
        nodes, ea, ei = wc.inputs(name, kind)
        p = wc.params(name, hidden)
        p64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}
        ref = torch_epd.epd_forward(p64, torch.tensor(nodes, dtype=torch.float64), torch.tensor(ea, dtype=torch.float64),
                                    torch.tensor(ei), wc.NUM_LAYERS, wc.M_STEPS).numpy()
        out = wc.forward_reference(name, hidden, kind)
        assert out.shape == (nodes.shape[0], wc.WIDTHS[name][0][2])
        err, scale = np.abs(out - ref).max(), np.abs(ref).max()
        print(f"{name} h{hidden} {kind}: |f32 - f64| = {err:.3e}, max |ref| = {scale:.3e}, ratio to the bar = {err / (1e-5 * scale):.3f}")
        assert scale > 1e-3                                              # above the floor the GPU test passes to assert_forward_close
        assert err <= 0.25 * 1e-5 * scale, (name, hidden, kind, err, scale)


@pytest.mark.parametrize("name", list(wc.WIDTHS))
def test_input_gradient_case_is_well_conditioned(name):
    """The encoder's input gradients are held to 2e-4 of the tensor's maximum with no allowance for a ReLU whose sign differs between
    two float32-accurate evaluations (one such unit moves a whole row of the gradient, here by up to 3 % of the maximum).  So the
    case must have none: plain PyTorch float32 is within a quarter of that bar of float64 autograd."""
    _, _, dx, dea = wc.input_gradient_reference(name)
    dx32, dea32 = wc.input_gradient_float32(name)
    for g32, g64 in ((dx32, dx), (dea32, dea)):
        err, scale = np.abs(g32 - g64).max(), np.abs(g64).max()
        print(f"{name}: |f32 - f64| = {err:.3e}, max |ref| = {scale:.3e}, ratio to the bar = {err / (2e-4 * scale):.4f}")
        assert g32.shape == g64.shape and scale > 0
        assert err <= 0.25 * 2e-4 * scale, (name, err, scale)


@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_layout_case_is_in_its_regime(name):
    L = wc.LAYOUTS[name]
    assert L.node_dim == wc.LAYOUT_NODE_DIM[name] <= wc.NODE_CAP
    assert L.payload == wc.LAYOUT_PAYLOAD[name]
    assert 2 <= L.k <= 64 and L.cart + 3 <= L.D and 0 <= L.mat < L.D and L.ctrl + 3 <= L.D
    obs = wc.scene_in_layout(name)
    assert obs.dtype == np.float32 and obs.shape == (L.k, wc.SCENE_N, L.D) and np.isfinite(obs).all()
    rigid = wc.rigid_rows(obs, L)
    assert rigid.sum() == round(0.1 * wc.SCENE_N) and (obs[:, :, L.mat] == obs[-1, :, L.mat]).all()
    assert (obs[-1, list(wc.OTHER_MATERIAL_ROWS), L.mat] == 2.0).all() and not rigid[list(wc.OTHER_MATERIAL_ROWS)].any()
    pos = obs[:, :, L.cart:L.cart + 3]
    assert 0.1 < pos.min() and pos.max() < 0.9
    vel = pos[1:] - pos[:-1]
    for t in range(1, vel.shape[0]):
        assert (vel[t] != vel[t - 1]).any(axis=1).mean() > 0.99          # velocities differ between frames
    for c in L.payload:                                                  # payload differs per frame: a missed shift shows
        assert all((obs[t, :, c] != obs[t + 1, :, c]).mean() > 0.99 for t in range(L.k - 1))
    if L.ctrl >= 0:
        assert (obs[-1, rigid, L.ctrl:L.ctrl + 3] != 0).all()            # the overwrite of state_pre has something to replace
    traj = wc.drift_trajectory(obs, L, 2, 5)
    assert traj.shape == (2, rigid.sum(), 3) and (traj[0] != pos[-1][rigid]).any(axis=1).all()
    # the same scene in every layout: the last frame's positions, so the same graph
    assert np.array_equal(pos[-1], wc.scene_in_layout("default")[-1, :, 2:5])
    s, _ = orc.get_connectivity(pos[-1], wc.R, 20)
    assert s.shape[0] > 10 * wc.SCENE_N


def test_restated_state_update_is_the_oracles_rollout_step():
    """state_pre / state_post of width_cases.py against one step of orc.rollout (with and without control columns, with a target and
    past the trajectory's end), the prediction held at zero."""
    for name in ("moved", "no_control"):
        L = wc.LAYOUTS[name]
        obs = wc.scene_in_layout(name)
        traj = wc.drift_trajectory(obs, L, 1, 6)
        zero = lambda n, ea, ei: np.zeros((n.shape[0], 3), np.float32)
        nxt = orc.get_position_from_prediction(STATS, L.cart_idx, np.zeros((obs.shape[1], 3), np.float32), obs)
        for steps_of_traj in (1, 0):
            ref, rec = orc.rollout(None, obs, traj[:steps_of_traj], 1, STATS, BOUNDS, wc.R, L.cart_idx, [L.mat], L.ctrl_idx, record=True, forward_fn=zero)
            target = traj[0] if steps_of_traj else None
            pre = wc.state_pre(obs, L, target) if L.ctrl >= 0 else np.array(obs)
            assert np.array_equal(pre[-1], rec[0])
            assert np.array_equal(wc.state_post(pre, L, nxt, target), ref)
