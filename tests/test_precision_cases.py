"""CPU: the cases of the fp16 single-product mode (precision_cases.py) are what their names say, and the bar of the tight GPU check
(test_gpu_precision.py, part A) means something at every one of them.

The bar is 3 g per case and output, g = the distance (rms over all elements, relative to the rms of the output) between the
restatement accumulated in float32 and in float64.  It separates the mode's contract from its neighbours only if 3 g is well below
the restatement's distance to them, so this asserts, per case and output, 3 g <= half the distance to
  * the exact float64 forward (a library that ignores the switch sits there),
  * the variant with only the weights rounded, and the one with only the inputs rounded (a library that drops the rounding of
    one operand -- or keeps one of the two cross products -- sits at or near these)."""
import numpy as np
import pytest

import precision_cases as pc


def test_fp16_rounding_is_to_nearest_even():
    # 2049 and 2051 lie halfway between fp16 neighbours (spacing 2 from 2048): ties go to the even mantissa
    assert pc.r16(np.float32(2049.0)) == 2048.0 and pc.r16(np.float32(2051.0)) == 2052.0
    assert pc.r16(np.float32(1.0 + 2.0 ** -11)) == 1.0 and pc.r16(np.float32(1.0 + 3 * 2.0 ** -11)) == 1.0 + 2.0 ** -9
    assert np.isinf(pc.r16(np.float32(65520.0))) and pc.r16(np.float32(65519.0)) == 65504.0   # the mode's range ends where fp16's does


def test_centring_gives_zero_mean_outputs_before_the_rounding():
    p = pc.a_params(128, 2)
    w, b = pc.centred(p["encoder.phi_node.4.weight"], p["encoder.phi_node.4.bias"])
    assert w.dtype == np.float32 and abs(w.astype(np.float64).sum(axis=0)).max() < 1e-5 and abs(float(b.astype(np.float64).sum())) < 1e-5


def test_the_restatement_without_rounding_is_the_oracle():
    """Neither operand rounded, float64: the model of oracle/torch_epd.py (the centred Linear + mean-square LayerNorm is the
    LayerNorm)."""
    name, hidden, nl, ms, _, _ = pc.HM_CASES[0]
    params, (nodes, ea, ei) = pc.hm_params(name), pc.hm_case(name)
    import torch
    from oracle import torch_epd
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
    ref = torch_epd.epd_forward(p, torch.tensor(nodes, dtype=torch.float64), torch.tensor(ea, dtype=torch.float64), torch.tensor(ei), nl, ms)
    assert pc.max_err(pc.exact(pc.epd_forward, params, nodes, ea, ei, nl, ms), ref.numpy()) < 1e-6


@pytest.mark.parametrize("hidden,nl", pc.A_CASES)
def test_the_bar_of_check_a_separates_the_contract_from_its_neighbours(hidden, nl):
    r64, g = pc.a_reference(hidden, nl)
    ex = pc.a_restate(hidden, nl, round_w=False, round_x=False)
    w_only = pc.a_restate(hidden, nl, round_x=False)
    x_only = pc.a_restate(hidden, nl, round_w=False)
    for name in pc.A_OUTPUTS:
        bar = 3 * g[name]
        d = {"exact": pc.rel_rms(r64[name], ex[name]), "weights only": pc.rel_rms(r64[name], w_only[name]),
             "inputs only": pc.rel_rms(r64[name], x_only[name])}
        print(f"hidden {hidden} layers {nl} {name}: g = {g[name]:.2e}, 3 g = {bar:.2e}, distances " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        assert g[name] > 0, name   # the two accumulations differ: the bar is not vacuous
        for k, v in d.items():
            assert bar <= 0.5 * v, (hidden, nl, name, k, bar, v)


def test_whole_forward_cases_are_where_their_names_put_them():
    for name, n, e, hub in pc.SYS_GRAPHS:
        nodes, ea, ei = pc.sys_case(name)
        assert nodes.shape == (n, pc.NODE_DIM) and ea.shape == (e, pc.EDGE_DIM) and ei.shape == (2, e)
        assert int(ei.min()) >= 0 and int(ei.max()) < n
        if hub:
            assert int((ei[1] == n // 2).sum()) >= hub > 128   # the hub's segment crosses groups of 4 x 32 edges
    assert [e for _, n, e, _ in pc.SYS_GRAPHS if n == 40] == [1, 33, 129, 4 * 128 + 1]
    blocks = lambda n: -(-n // 32)
    cus = 256
    for name, hidden, nl, ms, n, e in pc.HM_CASES:
        small_blocks = 4 if hidden == 128 else (4 * 8 * 32 // hidden)   # launch_node_h (csrc/hmlp.hip)
        four = blocks(n) >= small_blocks * cus
        assert four == (name == "four_block"), name
    n = next(c for c in pc.HM_CASES if c[0] == "four_block")[4]
    assert 4 * cus <= blocks(n) < 4 * cus + 16   # just past the switch


def test_whole_forward_restatement_sits_at_the_modes_precision():
    """The restatement's error against float64 is at fp16's scale, three orders of magnitude above the float32 parity bar -- the
    envelope of check B (err / 4 .. 4 err) therefore excludes a library that ignores the switch."""
    name, hidden, nl, ms, _, _ = pc.HM_CASES[2]
    ref, err = pc.hm_reference(name)
    print(f"{name}: err(restatement) = {err:.2e}")
    assert 4e-5 < err / 4 and err < 2e-2
