"""CPU: the bindings of the training-step entry points (gm_l1_loss, gm_trainer_*, gm_train_step and their workspace queries):
declared in include/gnn_manip_hip.h, bound in _lib.py with the signatures the header states, exported by the built library -- an
addition to ABI 7 -- and refusing null or absurd arguments before any device call, with a message that starts with their name."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
import train_step_cases as sc

NEW_SYMBOLS = ("gm_l1_loss_workspace_bytes", "gm_l1_loss", "gm_trainer_create", "gm_trainer_destroy", "gm_train_step_workspace_bytes",
               "gm_train_step", "gm_trainer_record", "gm_trainer_export", "gm_trainer_import")
FAKE = C.c_void_p(4096)          # a pointer that is only ever compared with NULL: every call below is refused before it is read


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    """The ctypes type _lib.py uses for a C parameter declaration: the descriptor is typed, an array of tensor pointers or a
    returned handle is a pointer to void*, every other pointer is void*."""
    from gnn_manip_amd import _lib
    decl = " ".join(decl.split())
    if "*" in decl:
        if decl.startswith("const gm_model_desc"):
            return _lib._MD
        if decl.count("*") == 2:
            return C.POINTER(C.c_void_p)
        return C.c_void_p
    return {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}[decl.rsplit(" ", 1)[0]]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbol_is_declared_bound_and_exported(name):
    from gnn_manip_amd import _lib
    assert re.search(r"\b%s\s*\(" % name, _header()), "not declared in the header"
    assert name in _lib.PROTOTYPES, "not bound in _lib.py"
    assert hasattr(_lib.lib(), name), "not exported by the library"
    assert _lib.lib().gm_abi_version() == 7


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_binding_has_the_headers_signature(name):
    from gnn_manip_amd import _lib
    ret, params = re.search(r"\b(int|size_t|void)\s+%s\s*\(([^)]*)\)\s*;" % name, _header()).groups()
    want = [_ctype(p) for p in params.split(",")]
    res, args = _lib.PROTOTYPES[name]
    assert res is {"int": C.c_int, "size_t": C.c_size_t, "void": None}[ret]
    assert args == want, (name, args, want)


def test_header_constants_are_the_packages():
    from gnn_manip_amd import train
    for name, value in (("PARAMS", train.PARAMS), ("EXP_AVG", train.EXP_AVG), ("EXP_AVG_SQ", train.EXP_AVG_SQ), ("GRADS", train.GRADS)):
        assert re.search(r"#define\s+GM_TRAINER_%s\s+%d\b" % (name, value), _header()), name
    assert len({train.PARAMS, train.EXP_AVG, train.EXP_AVG_SQ, train.GRADS}) == 4


def _loss(L, pred=FAKE, target=FAKE, n=10, od=3, nodes=FAKE, node_dim=6, mask_col=-1, loss=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.gm_l1_loss_workspace_bytes(max(n, 1), max(od, 1))
    return L.gm_l1_loss(pred, target, n, od, nodes, node_dim, mask_col, loss, None, None, ws, ws_bytes, None)


def test_l1_loss_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    for kw in (dict(pred=None), dict(target=None), dict(loss=None), dict(ws=None)):
        assert _loss(L, **kw) == -1 and err() == "gm_l1_loss: null pointer", kw
    for kw in (dict(n=0), dict(n=-5), dict(od=0)):
        assert _loss(L, **kw) == -1 and err().startswith("gm_l1_loss: sizes out of range"), kw
    for col in (6, 7, 1 << 20):
        assert _loss(L, mask_col=col) == -1 and err() == "gm_l1_loss: mask_col=%d outside the 6 node columns" % col
    assert _loss(L, nodes=None, mask_col=2) == -1 and err() == "gm_l1_loss: null nodes with mask_col=2"
    need = L.gm_l1_loss_workspace_bytes(10, 3)
    assert need > 0 and _loss(L, ws_bytes=need - 1) == -4 and err() == "gm_l1_loss: workspace %d < %d" % (need - 1, need)
    assert L.gm_l1_loss_workspace_bytes(0, 3) == 0 and L.gm_l1_loss_workspace_bytes(10, 0) == 0
    # the partials of a full grid and the finish's 24-byte state fit
    assert need >= sc.LOSS_GRID_MAX * 16 + 24 and need == L.gm_l1_loss_workspace_bytes(1 << 30, 4)


def test_trainer_entry_points_refuse_null_handles_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    out = C.c_void_p()
    assert L.gm_trainer_create(None, 0.9, 0.999, 1e-8, None, C.byref(out)) == -1 and err() == "gm_trainer_create: null model"
    assert out.value is None
    assert L.gm_train_step(None, FAKE, 10, FAKE, FAKE, 20, FAKE, -1, 1e-3, None, FAKE, 1 << 30, None) == -1 and err() == "gm_train_step: null trainer"
    assert L.gm_trainer_record(None, FAKE, None) == -1 and err() == "gm_trainer_record: null trainer"
    arr = (C.c_void_p * 2)(4096, 4096)
    assert L.gm_trainer_export(None, 1, arr, 2, None) == -1 and err() == "gm_trainer_export: null trainer"
    assert L.gm_trainer_import(None, 1, arr, 2, 0, None) == -1 and err() == "gm_trainer_import: null trainer"
    L.gm_trainer_destroy(None)                                   # like gm_model_destroy: nothing to do
    # the step's workspace: the tape, the backward's workspace and two [N, out_dim] arrays
    d = _lib.ModelDesc(*sc.SMALL, 1e-5)
    need = L.gm_train_step_workspace_bytes(C.byref(d), 300, 4000)
    assert need >= L.gm_train_tape_bytes(C.byref(d), 300, 4000) + L.gm_train_backward_workspace_bytes(C.byref(d), 300, 4000) + 2 * 300 * 3 * 4
    assert L.gm_train_step_workspace_bytes(None, 300, 4000) == 0 and L.gm_train_step_workspace_bytes(C.byref(d), 0, 10) == 0
    assert L.gm_train_step_workspace_bytes(C.byref(d), 300, -1) == 0


def test_python_surface():
    import inspect
    import gnn_manip_amd
    from gnn_manip_amd.train import Trainer
    assert gnn_manip_amd.Trainer is Trainer
    sig = inspect.signature(Trainer.__init__).parameters
    assert list(sig) == ["self", "model", "lr", "betas", "eps", "sand_only", "material_col"]
    assert (sig["lr"].default, sig["betas"].default, sig["eps"].default, sig["sand_only"].default, sig["material_col"].default) \
        == (1e-4, (0.9, 0.999), 1e-8, False, None)
    for name in ("step", "evaluate", "fit_epoch", "eval_epoch", "sync_module", "state_dict", "load_state_dict", "record", "status"):
        assert callable(getattr(Trainer, name)), name
    assert "autograd" in Trainer.__doc__ and "64 / 128 / 256" in Trainer.__doc__
    # a hidden size the training kernels are not instantiated for: refused by name, before anything touches a device
    model = gnn_manip_amd.EncProcDecGNN(25, 4, 3, 100, 2, 2)
    with pytest.raises(ValueError, match="64, 128 and 256"):
        Trainer(model)
