"""include/x2g_train.h: its binding table and the guarded update's argument checks, all made on the host before any
launch (no GPU needed)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EWORKSPACE = 0, 1001, 1003


def test_binding_table():
    from x2gnn import _lib

    names = {"x2g_optimizer_guard_workspace", "x2g_clip_adam_ema_guard"}
    assert set(_lib.TRAIN_SIGNATURES) == names == set(_lib.TRAIN_RESTYPES)
    for table in (_lib.SIGNATURES, _lib.STAGED_SIGNATURES, _lib.MULTI_SIGNATURES, _lib.CONV_SIGNATURES,
                  _lib.ATOMCTX_SIGNATURES):
        assert not names & set(table)
    P = ctypes.c_void_p
    assert _lib.TRAIN_SIGNATURES["x2g_clip_adam_ema_guard"] == [P, P, P, P, P, ctypes.c_int64, P, ctypes.c_int, P, P,
                                                                ctypes.c_size_t, P]
    assert _lib.TRAIN_RESTYPES["x2g_optimizer_guard_workspace"] is ctypes.c_size_t
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.TRAIN_SIGNATURES[n]
    # the unguarded entry's signature with the guard words in front of the workspace
    ex = _lib.SIGNATURES["x2g_clip_adam_ema_ex"]
    assert _lib.TRAIN_SIGNATURES["x2g_clip_adam_ema_guard"] == ex[:8] + [P] + ex[8:]


def test_the_header_declares_functions_only_and_leaves_the_abi_alone():
    from x2gnn import _lib

    with open(os.path.join(ROOT, "include", "x2g_train.h")) as f:
        sig, res, structs, consts = _lib.parse_header(f.read())
    assert not structs and not consts
    assert "x2g_clip_adam_ema_guard" not in _lib.SIGNATURES and _lib.CONSTS["OPT_ZERO_GRADS"] == 1


def test_workspace_holds_the_partials_and_the_four_tentative_scalars():
    from x2gnn import _lib

    lib = _lib.load()
    assert lib.x2g_optimizer_guard_workspace(0) == 0 and lib.x2g_optimizer_guard_workspace(-3) == 0
    for n in (1, 5, 1 << 33):
        assert lib.x2g_optimizer_guard_workspace(n) == lib.x2g_optimizer_workspace(n) + 16


A, ODD8, ODD16 = 0x10000, 0x10004, 0x10008  # never dereferenced: every case below is refused before a launch


def args(**kw):
    v = dict(params=A, grads=A, m=A, v=A, ema=A, n=64, sc=A, flags=0, guard=A, ws=A, ws_bytes=4096, stream=None)
    v.update(kw)
    return [v[k] for k in ("params", "grads", "m", "v", "ema", "n", "sc", "flags", "guard", "ws", "ws_bytes", "stream")]


@pytest.mark.parametrize("kw,want", [
    (dict(n=0), OK), (dict(n=0, params=None, grads=None, m=None, v=None, ws=None), OK),
    (dict(n=-1), EINVAL), (dict(sc=None), EINVAL), (dict(flags=2), EINVAL), (dict(flags=-1), EINVAL),
    (dict(params=None), EINVAL), (dict(grads=None), EINVAL), (dict(m=None), EINVAL), (dict(v=None), EINVAL),
    (dict(grads=ODD16), EINVAL), (dict(grads=ODD8), EINVAL),
    (dict(ws=None), EWORKSPACE), (dict(ws_bytes=1024), EWORKSPACE), (dict(ws_bytes=1039), EWORKSPACE),
    (dict(guard=None), EINVAL), (dict(guard=ODD8), EINVAL), (dict(n=0, guard=None), EINVAL),
])
def test_argument_validation_without_gpu(kw, want):
    from x2gnn import _lib

    assert _lib.load().x2g_clip_adam_ema_guard(*args(**kw)) == want


@pytest.mark.parametrize("kw", [dict(n=-1), dict(sc=None), dict(flags=2), dict(params=None), dict(grads=ODD8),
                                dict(ws=None), dict(ws_bytes=1023), dict(n=0)])
def test_the_statuses_follow_the_unguarded_entry(kw):
    from x2gnn import _lib

    lib = _lib.load()
    a = args(**kw)
    assert lib.x2g_clip_adam_ema_guard(*a) == lib.x2g_clip_adam_ema_ex(*(a[:8] + a[9:]))
