"""CPU: every case of tests/ragged_rollout_cases.py is in the regime it was built for, measured on the oracle's radius graphs of
the first window -- so that the GPU test (test_gpu_ragged_rollout.py) compares what it claims to compare."""
import numpy as np
import pytest

import ragged_cases as rgc
import ragged_rollout_cases as rrc


@pytest.mark.parametrize("name", sorted(rrc.CASES))
def test_case_is_in_its_regime(name):
    c = rrc.case(name)
    c.check()
    props = c.measure()
    print(f"\n[ragged rollout cases] {name}: sizes {props['sizes']} edges {props['edges']} (mod 128: {props['edges_mod_group']}) "
          f"rigid {props['rigid']} boundaries mod 16 {props['boundaries_mod_16']} mod 256 {props['boundaries_mod_256']} "
          f"largest in-degree {[int(d.max()) for d in props['indeg']]}")
    # a shared block plan would put the tail of one scene and the head of the next into one group
    if len(c.sizes) > 1:
        assert all(props["edges_mod_group"]), props["edges"]


def test_the_cases_cover_what_the_batch_can_get_wrong():
    p = {name: rrc.case(name).measure() for name in rrc.CASES}
    assert 0 in p["mixed"]["boundaries_mod_16"] and any(p["mixed"]["boundaries_mod_16"])          # on and off the 16-query edge
    assert 0 in p["mixed"]["boundaries_mod_256"] and any(p["mixed"]["boundaries_mod_256"])        # on and off the 256-row edge
    assert 0 in p["mixed"]["rigid"]                                                               # a scene without rigid rows
    assert 1 in p["single_row"]["sizes"]
    assert len(set(p["equal"]["sizes"])) == 1 and p["one"]["n_graphs"] == 1
    assert rrc.case("clump").max_nb == 160
    # both sides of the clump's boundary hold segments longer than a group: head partials and stitch entries at the boundary
    d0, d1 = p["clump"]["indeg"]
    assert (d0[-rrc.CLUMP:] > rrc.GROUP_EDGES).all() and (d1[:rrc.CLUMP] > rrc.GROUP_EDGES).all()
    assert d0[-1] > rrc.GROUP_EDGES and d1[0] > rrc.GROUP_EDGES                                   # the two rows AT the boundary
    for name, model in rrc.FORWARD:
        assert name in rrc.CASES and model in rrc.MODELS
    assert {m for c, m in rrc.FORWARD if c == "mixed"} == set(rrc.MODELS)                          # every kernel family and f16


def test_batch_arrays_are_the_scenes_side_by_side():
    c = rrc.case("mixed")
    w, f, tr = c.window(), c.frames(), c.trajectory()
    assert w.shape == (rrc.L.k, sum(c.sizes), rrc.L.D) and f.shape == (rrc.STEPS, sum(c.sizes), rrc.L.D)
    for g, s in enumerate(c.scenes):
        assert np.array_equal(w[:, c.rows(g)], s.window()) and np.array_equal(f[:, c.rows(g)], s.frames())
    # global ranks: the poses of scene g's rigid rows follow those of the scenes before it
    counts = [int(s.rigid.sum()) for s in c.scenes]
    assert tr.shape == (rrc.STEPS, sum(counts), 3)
    at = np.r_[0, np.cumsum(counts)]
    for g, t in enumerate(c.trajectories()):
        assert t.shape[1] == counts[g] and np.array_equal(tr[:, at[g]:at[g + 1]], t)
    # the first frame a recorded step reads is the window's last one, and the recording's control is the way to the next frame
    s = c.scenes[0]
    assert np.array_equal(s.frames()[0], s.window()[-1])
    k = rrc.L.k
    assert np.array_equal(s.sim[k - 1][s.rigid][:, rrc.L.ctrl_idx], s.sim[k][s.rigid][:, rrc.L.cart_idx] - s.sim[k - 1][s.rigid][:, rrc.L.cart_idx])


def test_clump_stays_inside_one_radius_over_the_steps():
    c = rrc.case("clump")
    for s, rows in ((c.scenes[0], slice(-rrc.CLUMP, None)), (c.scenes[1], slice(0, rrc.CLUMP))):
        for t in range(rrc.T_FRAMES):
            p = s.sim[t][rows][:, rrc.L.cart_idx].astype(np.float64)
            assert np.linalg.norm(p - p.mean(axis=0), axis=1).max() < rrc.R / 2          # any two of them within one radius


def test_refusal_tables():
    sizes = rrc.case("mixed").sizes
    r = rrc.refusals(sizes)
    good = [int(v) for v in rgc.offsets(sizes)]
    assert r["nodes_per_graph"][:2] == (good, sizes[0]) and r["workspace"] == (good, 0, 1)
    assert r["offsets_start"][0][0] != 0 and r["offsets_start"][0][1:] == good[1:]
    e = r["empty_graph"][0]
    assert any(a == b for a, b in zip(e, e[1:])) and len(e) == len(good) + 1
    assert len(r["too_many_graphs"][0]) - 1 == rgc.GM_RAGGED_MAX_GRAPHS + 1


# ------------------------------------------------------------------------------------------ the loss of a ragged batch
@pytest.mark.parametrize("mask", ["none", "rigid", "rigid_material", "empty"])
@pytest.mark.parametrize("frame_dim", [8, 5])
def test_ragged_loss_restatement_is_autograd_per_sample(mask, frame_dim):
    """losses[g] and the gradient slabs against float64 autograd through L1Loss(reduction='sum') on graph g's counted rows alone."""
    import torch
    import train_rollout_cases as trc
    b = rrc.loss_batch(6, frame_dim, mask)
    cart = trc.LOSS_CART
    losses, counts, d_rec, d_fin = rrc.rollout_l1_restated_ragged(b["windows"], b["final"], b["frames"], b["sizes"], cart, b["rank"],
                                                                    b["material_col"], b["pos_scale"])
    off = rgc.offsets(b["sizes"])
    steps, k = b["windows"].shape[:2]
    scale = (1.0, 1.0, 1.0) if b["pos_scale"] is None else b["pos_scale"]
    assert len(losses) == len(b["sizes"]) and d_rec.shape == (steps,) + b["final"].shape[1:] and d_fin.shape == b["final"].shape
    for g, p in enumerate(b["parts"]):
        rows = slice(int(off[g]), int(off[g + 1]))
        counted = trc.counted_rows(p["windows"], p["rank"], p["material_col"])
        assert counts[g] == counted.sum()
        if mask == "empty":
            assert counts[g] == 0 and np.isnan(losses[g]) and not d_rec[:, rows].any() and not d_fin[:, rows].any()
            continue
        assert 0 < counts[g] < p["windows"].shape[2] or mask == "none"
        w = torch.tensor(p["windows"].astype(np.float64), requires_grad=True)
        f = torch.tensor(p["final"].astype(np.float64), requires_grad=True)
        total = 0.0
        for t in range(steps):
            pred = (w[t + 1][-1] if t + 1 < steps else f[-1])[:, cart:cart + 3]
            gt = torch.tensor(p["frames"][t][:, cart:cart + 3].astype(np.float64))
            for c in range(3):
                total = total + torch.nn.L1Loss(reduction="sum")(pred[counted, c], gt[counted, c]) / scale[c]
        total = total / (steps * int(counts[g]))
        total.backward()
        assert abs(losses[g] - float(total.detach())) <= 1e-6 * abs(float(total.detach()))    # float32 differences against float64 ones
        # record t + 1 IS the predicted frame of step t < steps - 1: its gradient is autograd's on the window's last frame
        for t in range(steps - 1):
            want = w.grad[t + 1][-1].numpy()
            assert np.abs(d_rec[t + 1][rows] - want).max() <= 1e-6 * np.abs(want).max()
        want = f.grad[-1].numpy()
        sign0 = np.zeros_like(want, bool)
        sign0[p["windows"].shape[2] // 2, cart + 2] = True                        # the one exactly equal element: sign(0) = 0
        assert np.abs(np.where(sign0, 0.0, d_fin[-1][rows] - want)).max() <= 1e-6 * np.abs(want).max() and d_fin[-1][rows][sign0] == 0
        assert not d_rec[0][rows].any() and not d_fin[:-1, rows].any()
    total, bad = rrc.batch_loss(losses)
    assert bad == (len(b["sizes"]) if mask == "empty" else 0) and (np.isnan(total) if mask == "empty" else total == (losses[0] + losses[1]) + losses[2])


def test_ragged_loss_batch_has_global_ranks_and_its_own_regime():
    import train_step_cases as tsc
    b = rrc.loss_batch(6, 8, "rigid")
    rigid = b["rank"][b["rank"] >= 0]
    assert np.array_equal(rigid, np.arange(len(rigid))) and len(rigid) > 3
    assert [tsc.loss_regime(n)[0] for n in b["sizes"]] == [2, 1, 1] and all(n % tsc.LOSS_WG for n in b["sizes"])
    assert rrc.case(rrc.SWEEP_CASE).sizes == (130, 1, 77)


def test_loss_shapes_are_in_the_regimes_they_were_built_for():
    import train_rollout_cases as trc
    import train_step_cases as tsc
    tail, cap = rrc.LOSS_SHAPES["tail"], rrc.LOSS_SHAPES["cap"]
    # tail: one row; past one pass of the capped grid, the second pass one full workgroup and one with a single row; one full workgroup
    assert [tsc.loss_regime(n) for n in tail] == [(1, 1), (tsc.LOSS_GRID_MAX, 2), (1, 1)] and tail[0] == 1 and tail[2] == tsc.LOSS_WG
    assert tail[1] - tsc.LOSS_GRID_MAX * tsc.LOSS_WG == tsc.LOSS_WG + 1
    # cap: the table is full, and a binary search over it reaches every depth up to log2 of the cap
    from gnn_manip_amd import _lib
    assert len(cap) == rgc.GM_RAGGED_MAX_GRAPHS == _lib.RAGGED_MAX_GRAPHS == 64 and set(cap) == {1, 2, 3, 5} and sum(cap) < tsc.LOSS_WG
    for name in rrc.LOSS_SHAPES:
        for mask in rrc.LOSS_SHAPE_MASKS:
            b = rrc.loss_shape(name, 6, 8, mask)
            assert b["sizes"] == rrc.LOSS_SHAPES[name] and b["windows"].shape[:2] == (rrc.LOSS_STEPS, 6)
            counts = [int(trc.counted_rows(p["windows"], p["rank"], p["material_col"]).sum()) for p in b["parts"]]
            empty = rrc.LOSS_CAP_EMPTY if (name, mask) == ("cap", "rigid_material") else ()
            assert all((c == 0) == (g in empty) for g, c in enumerate(counts)), (name, mask, counts)
            if mask == "none":
                assert counts == list(b["sizes"]) and b["rank"] is None
            else:
                rigid = b["rank"][b["rank"] >= 0]
                assert np.array_equal(rigid, np.arange(len(rigid))) and len(rigid) > 3          # ranks are global
                assert all(p["pos_scale"] == b["pos_scale"] for p in b["parts"])
    assert {cap[g] for g in rrc.LOSS_CAP_EMPTY} == set(cap) and {0, len(cap) - 1} <= set(rrc.LOSS_CAP_EMPTY)
    assert np.allclose(rrc.loss_rtol(2, [1, 33025]), [2.0 ** -52, 66050 * 2.0 ** -53], rtol=0, atol=0)
