"""CPU: the entry points of the differentiable rollout are declared in include/gnn_manip_hip.h, bound in _lib.py and exported by
the built library; they refuse their arguments before any device call."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = ("gm_epd_backward_inputs_only", "gm_rigid_transform_backward")


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbol_is_declared_bound_and_exported(name):
    from gnn_manip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, header), "not declared in the header"
    assert name in _lib.PROTOTYPES, "not bound in _lib.py"
    assert hasattr(_lib.lib(), name), "not exported by the library"


def test_abi_version_is_unchanged():
    from gnn_manip_amd import _lib
    assert _lib.lib().gm_abi_version() == 7


def test_inputs_only_takes_the_inputs_signature_without_grads():
    from gnn_manip_amd import _lib
    full, only = _lib.PROTOTYPES["gm_epd_backward_inputs"][1], _lib.PROTOTYPES["gm_epd_backward_inputs_only"][1]
    assert only == full[:8] + full[9:]          # argument 8 of gm_epd_backward_inputs is `grads`


def test_new_entry_points_check_their_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    args = [None if t is C.c_void_p else 0 for t in _lib.PROTOTYPES["gm_epd_backward_inputs_only"][1]]
    # both outputs NULL: nothing to compute, refused whatever else is passed
    assert L.gm_epd_backward_inputs_only(*args) == -1
    assert L.gm_last_error() == b"gm_epd_backward_inputs_only: d_nodes and d_edge_attr are both null"
    fake = C.c_void_p(64)   # never dereferenced: the null model is reported first
    args[8] = fake
    assert L.gm_epd_backward_inputs_only(*args) == -1
    assert L.gm_last_error() == b"gm_epd_backward_inputs_only: null model"
    t3 = (C.c_float * 3)(0.5, 0.5, 0.4)
    assert L.gm_rigid_transform_backward(None, 5, None, 2, C.byref(t3), None, None, None) == -1      # no output
    assert L.gm_last_error() == b"gm_rigid_transform_backward: null pointer"
    assert L.gm_rigid_transform_backward(None, 5, None, 2, None, None, None, None) == -1             # no ty_init
    assert L.gm_rigid_transform_backward(None, -1, None, 2, C.byref(t3), None, None, None) == -1
    assert L.gm_rigid_transform_backward(None, 5, None, 0, C.byref(t3), None, None, None) == 0       # no steps: nothing to write
