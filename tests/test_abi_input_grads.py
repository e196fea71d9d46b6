"""CPU: the entry points of the differentiable rollout step are declared in include/gnn_manip_hip.h, bound in _lib.py and exported
by the built library; the new workspace queries answer without a device."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = ("gm_epd_backward_inputs", "gm_train_backward_inputs_workspace_bytes", "gm_edge_features_backward",
               "gm_edge_features_backward_workspace_bytes", "gm_node_features_backward", "gm_integrate_backward")


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbol_is_declared_bound_and_exported(name):
    from gnn_manip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, header), "not declared in the header"
    assert name in _lib.PROTOTYPES, "not bound in _lib.py"
    assert hasattr(_lib.lib(), name), "not exported by the library"


def test_abi_version_is_unchanged_and_the_queries_answer():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    assert L.gm_abi_version() == 7
    d = C.byref(_lib.ModelDesc(25, 4, 3, 128, 2, 10, 1e-5))
    # the encoders' slots of the backward workspace are laid out with their transposed W1 images: the existing query covers them
    assert L.gm_train_backward_inputs_workspace_bytes(d, 300, 4000) >= L.gm_train_backward_workspace_bytes(d, 300, 4000) > 0
    # [2, E] int64 + two destination sorts + [E, 3] float per-edge gradients
    assert L.gm_edge_features_backward_workspace_bytes(300, 4000) >= 2 * 4000 * 8 + 2 * L.gm_csr_workspace_bytes(300, 4000) + 4000 * 12


def test_new_entry_points_check_their_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    args = [None if t is C.c_void_p else 0 for t in _lib.PROTOTYPES["gm_epd_backward_inputs"][1]]
    assert L.gm_epd_backward_inputs(*args) == -1
    assert L.gm_last_error() == b"gm_epd_backward_inputs: null model"
    assert L.gm_node_features_backward(None, 5, None, None, None, None) == -1
    assert L.gm_integrate_backward(None, 5, None, None, None, None) == -1
    assert L.gm_edge_features_backward(None, 3, None, None, 5, 7, 0.015, None, None, None, 0, None) == -1
