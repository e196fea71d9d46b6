"""CPU: gm_model_set_precision is declared in include/gnn_manip_hip.h, bound in _lib.py and exported by the built library; it is a
pure addition to ABI version 7, rejects a null model and unknown values without touching a device, and the Python switch rejects
unknown names."""
import os
import re

import pytest

from conftest import ROOT

NAME = "gm_model_set_precision"


def _header():
    return open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()


def test_symbol_is_declared_bound_and_exported():
    from gnn_manip_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gm_model\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;" % NAME, code), "not declared in the header"
    assert re.search(r"\bGM_PRECISION_F32\s*=\s*0\b", code) and re.search(r"\bGM_PRECISION_F16\s*=\s*1\b", code)
    res, args = _lib.PROTOTYPES[NAME]
    assert res is _lib._i32 and args == [_lib._vp, _lib._i32]
    assert hasattr(_lib.lib(), NAME), "not exported by the library"


def test_header_documents_the_mode():
    h = _header()
    assert "Numeric domain of the fp16 mode" in h
    doc = h[h.index("int gm_model_set_node_fusion"):h.index("int %s" % NAME)]
    for word in ("GM_PRECISION_F16", "gm_rollout_step", "training", "GM_ERR_INVALID_ARGUMENT"):
        assert word in doc, word


def test_abi_version_is_unchanged():
    from gnn_manip_amd import _lib
    assert _lib.lib().gm_abi_version() == 7


@pytest.mark.parametrize("value", [0, 1, 2, -1])
def test_null_model_is_rejected_with_a_message(value):
    from gnn_manip_amd import _lib
    L = _lib.lib()
    assert L.gm_model_set_precision(None, value) == -1   # GM_ERR_INVALID_ARGUMENT
    assert b"gm_model_set_precision" in L.gm_last_error()


def test_python_switch_checks_the_name_and_defaults_to_f32():
    from gnn_manip_amd import EncProcDecGNN
    m = EncProcDecGNN(25, 4, 3, 64, 2, 1)
    assert m.precision == m.encoder.precision == m.processor[0].precision == "f32"
    for bad in ("bf16", "F16", 1, None):
        with pytest.raises(ValueError):
            m.set_precision(bad)
        with pytest.raises(ValueError):
            m.encoder.set_precision(bad)
        with pytest.raises(ValueError):
            m.processor[0].set_precision(bad)
    assert m.precision == "f32"
    m.set_precision("f16")   # no handle yet: remembered, applied when the handle is created
    assert m.precision == m.encoder.precision == m.processor[0].precision == "f16"
    m.processor[0].set_precision("f32")
    assert (m.precision, m.processor[0].precision) == ("f16", "f32")
