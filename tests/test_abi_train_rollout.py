"""CPU: the bindings of the rollout-training entry points (gm_rollout_l1_loss, gm_train_rollout_step and their workspace queries):
declared in include/gnn_manip_hip.h, bound in _lib.py with the signatures the header states, exported by the built library -- an
addition to ABI 7 -- and refusing null or absurd arguments before any device call, with a message that starts with their name."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import BOUNDS, CART, CTRL, MAT, ROOT, STATS
import train_step_cases as sc

NEW_SYMBOLS = ("gm_rollout_l1_loss_workspace_bytes", "gm_rollout_l1_loss", "gm_train_rollout_step_workspace_bytes", "gm_train_rollout_step")
FAKE = C.c_void_p(4096)          # a pointer that is only ever compared with NULL: every call below is refused before it is read


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    """The ctypes type _lib.py uses for a C parameter declaration: the two descriptors are typed, every other pointer is void*."""
    from gnn_manip_amd import _lib
    decl = " ".join(decl.split())
    if "*" in decl:
        if decl.startswith("const gm_model_desc"):
            return _lib._MD
        if decl.startswith("const gm_feature_desc"):
            return _lib._FD
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


def _fdesc(k=6, data_dim=8, control=True):
    from gnn_manip_amd.graph import make_feature_desc
    return make_feature_desc(0.015, STATS, BOUNDS, CART, MAT, CTRL if control else None, k, data_dim)


def _loss(L, windows=FAKE, final=FAKE, frames=FAKE, frame_dim=8, steps=3, n=10, fd=None, rank=FAKE, col=-1, scale=None, loss=FAKE,
          d_records=None, d_final=None, ws=FAKE, ws_bytes=None):
    fd = _fdesc() if fd is None else fd
    if ws_bytes is None:
        ws_bytes = L.gm_rollout_l1_loss_workspace_bytes(max(n, 1), min(max(steps, 1), 32768))
    return L.gm_rollout_l1_loss(windows, final, frames, frame_dim, steps, n, C.byref(fd) if fd else None, rank, col, scale, loss, None,
                                d_records, d_final, ws, ws_bytes, None)


def test_rollout_l1_loss_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    for kw in (dict(windows=None), dict(final=None), dict(frames=None), dict(loss=None), dict(ws=None)):
        assert _loss(L, **kw) == -1 and err() == "gm_rollout_l1_loss: null pointer", kw
    for steps in (0, -1, 32769):
        assert _loss(L, steps=steps) == -1 and err().startswith("gm_rollout_l1_loss: steps=%d outside 1..32768" % steps)
    for n in (0, -5):
        assert _loss(L, n=n) == -1 and err().startswith("gm_rollout_l1_loss: sizes out of range"), n
    for frame_dim in (4, 6, 7, 9, 0):
        assert _loss(L, frame_dim=frame_dim) == -1 and err().startswith("gm_rollout_l1_loss: frame_dim=%d is neither" % frame_dim)
    assert _loss(L, frame_dim=5, col=8) == -1 and err().startswith("gm_rollout_l1_loss: material_col=8")      # data_dim - 3 passes that check
    for col in (8, 9, 1 << 20):
        assert _loss(L, col=col) == -1 and err() == "gm_rollout_l1_loss: material_col=%d outside the 8 state columns" % col
    for bad in ((1.0, 0.0, 1.0), (1.0, 1.0, float("nan"))):
        assert _loss(L, scale=(C.c_double * 3)(*bad)) == -1 and "pos_scale" in err()
    assert _loss(L, d_records=FAKE) == -1 and err() == "gm_rollout_l1_loss: d_records and d_final go together"
    assert _loss(L, d_final=FAKE) == -1 and err() == "gm_rollout_l1_loss: d_records and d_final go together"
    need = L.gm_rollout_l1_loss_workspace_bytes(10, 3)
    assert need > 0 and _loss(L, ws_bytes=need - 1) == -4 and err() == "gm_rollout_l1_loss: workspace %d < %d" % (need - 1, need)
    assert L.gm_rollout_l1_loss_workspace_bytes(0, 3) == 0 and L.gm_rollout_l1_loss_workspace_bytes(10, 0) == 0
    # three sums and a count per workgroup of a full grid and the finish's 24-byte state fit, whatever the sizes
    assert need >= sc.LOSS_GRID_MAX * 32 + 24 and need == L.gm_rollout_l1_loss_workspace_bytes(1 << 30, 32768)


def test_train_rollout_step_refuses_a_null_trainer_and_sizes_its_workspace():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    fd = _fdesc()
    assert L.gm_train_rollout_step(None, FAKE, 400, C.byref(fd), 20, FAKE, 40, FAKE, 8, 4, -1, None, 1e-3, 1, None, FAKE, 1 << 40, None) == -1
    assert err() == "gm_train_rollout_step: null trainer"
    d = _lib.ModelDesc(*sc.SMALL, 1e-5)
    q = lambda n=400, nr=40, k_nb=20, steps=4: L.gm_train_rollout_step_workspace_bytes(C.byref(d), C.byref(fd), n, nr, k_nb, steps)
    window = 6 * 400 * 8 * 4
    parts = (L.gm_rollout_workspace_bytes(C.byref(d), 400, 20) + L.gm_rollout_backward_workspace_bytes(C.byref(d), C.byref(fd), 400, 20)
             + 5 * window + 4 * 400 * 8 * 4 + 2 * window + 4 * 40 * 3 * 4 + L.gm_rollout_l1_loss_workspace_bytes(400, 4))
    assert parts <= q() <= parts + 8 * 256                        # the parts, each on 256 bytes
    assert q(steps=8) - q() >= 4 * (window + 400 * 8 * 4)         # a window and a record per further step
    for kw in (dict(n=0), dict(nr=-1), dict(nr=401), dict(k_nb=0), dict(steps=0), dict(steps=32769)):
        assert q(**kw) == 0, kw
    assert L.gm_train_rollout_step_workspace_bytes(None, C.byref(fd), 400, 40, 20, 4) == 0
    assert L.gm_train_rollout_step_workspace_bytes(C.byref(d), None, 400, 40, 20, 4) == 0


def test_python_surface():
    import gnn_manip_amd
    from gnn_manip_amd.dataset import CoffeeDataset
    from gnn_manip_amd.train import Trainer
    for name in ("step_rollout", "evaluate_rollout"):
        sig = inspect.signature(getattr(Trainer, name)).parameters
        assert list(sig)[:7] == ["self", "engine", "obs0", "frames", "steps", "pos_scale", "loss_out"], name
        assert all(sig[p].default is None for p in list(sig)[4:]), name
    sig = inspect.signature(Trainer.fit_rollout_epoch).parameters
    assert list(sig)[:6] == ["self", "dataset", "engine", "steps", "starts", "seed"] and sig["starts"].default is None and sig["seed"].default == 0
    sig = inspect.signature(CoffeeDataset.rollout_sample).parameters
    assert list(sig) == ["self", "idx", "steps", "seed", "stream"] and (sig["seed"].default, sig["stream"].default) == (0, 0)
    assert "synchronises" in Trainer.step_rollout.__doc__ and "never synchronises" in Trainer.evaluate_rollout.__doc__
    assert gnn_manip_amd.Trainer is Trainer
