"""CPU: the C-ABI library loads and exports every symbol include/gnn_manip_hip.h declares."""
import os
import re

from conftest import ROOT


def test_library_exports_every_declared_symbol():
    from gnn_manip_amd import _lib
    from gnn_manip_amd.build import build
    build()
    header = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gm_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    handle = _lib.lib()
    for name in declared:
        assert hasattr(handle, name), name
    assert handle.gm_abi_version() == 7


def test_workspace_queries_and_host_side_errors():
    import ctypes as C
    from gnn_manip_amd import _lib
    L = _lib.lib()
    assert L.gm_graph_workspace_bytes(1000, 20) > 1000 * 20 * 4
    assert L.gm_csr_workspace_bytes(1000, 20000) > 3 * 20000 * 4
    d = _lib.ModelDesc(25, 4, 3, 128, 2, 10, 1e-5)
    assert L.gm_model_num_tensors(C.byref(d)) == 182  # 182 tensors
    assert L.gm_forward_workspace_bytes(C.byref(d), 1000, 20000) >= (1000 * 4 + 20000) * 128 * 4
    # argument validation happens before any device call
    bad = _lib.ModelDesc(25, 4, 3, 128, 1, 10, 1e-5)
    out = C.c_void_p()
    arr = (C.c_void_p * 1)()
    rc = L.gm_model_create(C.byref(bad), arr, 1, 0, None, C.byref(out))
    assert rc == -1 and b"num_layers must be at least 2" in L.gm_last_error()
    rc = L.gm_radius_graph_build(None, 3, 10, -1.0, 20, None, 0, None)
    assert rc == -1


def test_model_create_refuses_an_eps_that_is_not_positive():
    """ln_eps = 0, negative or NaN (which fails `> 0` like any comparison) is refused before any pointer is read or device call made."""
    import ctypes as C
    from gnn_manip_amd import _lib
    L = _lib.lib()
    arr = (C.c_void_p * 1)()
    for eps in (0.0, -0.0, -1e-5, float("-inf"), float("nan")):
        out = C.c_void_p()
        rc = L.gm_model_create(C.byref(_lib.ModelDesc(25, 4, 3, 128, 2, 10, eps)), arr, 1, 0, None, C.byref(out))
        assert rc == -1 and b"ln_eps must be > 0" in L.gm_last_error() and not out.value, eps


def test_product_modules_reject_cpu_tensors():
    import pytest
    import torch
    from gnn_manip_amd import EncProcDecGNN, get_connectivity
    with pytest.raises(RuntimeError):
        get_connectivity(torch.zeros(4, 3), 0.015)
    m = EncProcDecGNN(25, 4, 3, 128, 2, 2)
    with pytest.raises(RuntimeError), torch.no_grad():
        m.forward(torch.zeros(4, 25), torch.zeros(4, 4), torch.zeros(2, 4, dtype=torch.long))


def test_state_dict_layout_matches_reference_fixture(golden):
    import torch
    from gnn_manip_amd import EncProcDecGNN
    g7 = golden("g7_epd_wiring.npz")
    m = EncProcDecGNN(25, 4, 3, 128, 2, 10)
    assert sorted(m.state_dict().keys()) == list(g7["h128.keys"])
    assert sum(p.numel() for p in m.parameters()) == 1591299
    m3 = EncProcDecGNN(25, 4, 3, 64, 3, 2)
    assert sorted(m3.state_dict().keys()) == list(g7["h64_l3_m2.keys"])


# (hidden_size, num_layers, m_steps), (n, e) -> gm_train_tape_bytes, gm_train_backward_workspace_bytes, gm_block_tape_bytes of the
# GraphIndependent and of the InteractionNetwork, gm_block_backward_workspace_bytes: the training tape and workspace layouts
TRAIN_BYTES = {
    ((64, 2, 1), (1, 0)): (7168, 73345792, 1280, 4608, 73345792),
    ((64, 2, 1), (300, 4000)): (9651456, 77980416, 3388672, 3902720, 77980416),
    ((64, 5, 10), (1, 0)): (32512, 77033728, 2048, 5376, 73715968),
    ((64, 5, 10), (300, 4000)): (88446720, 84969216, 6794240, 7308288, 81651456),
    ((128, 2, 10), (1, 0)): (38144, 84514048, 2048, 6144, 76551424),
    ((128, 2, 10), (300, 4000)): (101020672, 93779712, 6759936, 7504384, 85817088),
    ((128, 5, 2), (1, 0)): (19712, 79503616, 3584, 7680, 78029056),
    ((128, 5, 2), (300, 4000)): (49008128, 95371008, 13571072, 14315520, 93896448),
    ((256, 2, 2), (1, 0)): (22784, 88762624, 3584, 9216, 85223680),
    ((256, 2, 2), (300, 4000)): (55862272, 107290368, 13502208, 14707456, 103751424),
    ((256, 5, 1), (1, 0)): (26368, 91128064, 6656, 12288, 91128064),
    ((256, 5, 1), (300, 4000)): (65845248, 122859264, 27124736, 28329984, 122859264),
}


def test_training_tape_and_workspace_sizes_are_pinned():
    import ctypes as C
    from gnn_manip_amd import _lib
    L = _lib.lib()
    for ((hidden, num_layers, m_steps), (n, e)), want in TRAIN_BYTES.items():
        d = C.byref(_lib.ModelDesc(25, 4, 3, hidden, num_layers, m_steps, 1e-5))
        got = (L.gm_train_tape_bytes(d, n, e), L.gm_train_backward_workspace_bytes(d, n, e), L.gm_block_tape_bytes(d, 0, n, e),
               L.gm_block_tape_bytes(d, 1, n, e), L.gm_block_backward_workspace_bytes(d, n, e))
        assert got == want, (hidden, num_layers, m_steps, n, e, got)


def test_training_entry_points_reject_a_null_model():
    """Every other argument null or zero: the null model is what each one reports, before any device call."""
    import ctypes as C
    from gnn_manip_amd import _lib
    L = _lib.lib()
    for name in ("gm_epd_forward_train", "gm_epd_backward", "gm_graph_independent_forward_train", "gm_graph_independent_backward",
                 "gm_interaction_network_forward_train", "gm_interaction_network_backward"):
        args = [None if t is C.c_void_p else 0 for t in _lib.PROTOTYPES[name][1]]
        assert getattr(L, name)(*args) == -1, name   # GM_ERR_INVALID_ARGUMENT
        assert L.gm_last_error() == f"{name}: null model".encode()
