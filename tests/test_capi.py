"""C-ABI library: loads without a GPU, exports every symbol include/*.h declares, rejects bad inputs before
touching the device, and the product path refuses to run without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from instantsfm_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions(only=None):
    names = set()
    for h in sorted(os.listdir(os.path.join(REPO, "include"))):
        if h.endswith(".h") and (only is None or h in only):
            txt = open(os.path.join(REPO, "include", h)).read()
            txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
            names |= set(re.findall(r"\b(insfm_[a-z_]+)\s*\(", txt))
    return sorted(names - {"insfm_ba_allreduce_fn"})


def test_header_declares_expected_api():
    fns = header_functions()
    for name in ("insfm_ba_create", "insfm_ba_step", "insfm_ba_cost", "insfm_ba_destroy", "insfm_ba_last_error",
                 "insfm_gp_create", "insfm_gp_step", "insfm_gp_cost"):
        assert name in fns


def test_library_exports_every_header_symbol():
    L = _capi.load()
    for name in header_functions():
        assert hasattr(L, name), name
    assert set(header_functions()) == set(_capi.SYMBOLS)


def test_product_header_is_free_of_debug_entry_points():
    """insfm_ba.h is the product ABI; introspection, timing probes and the partitioned-CG prototype live in
    insfm_ba_debug.h."""
    assert set(_capi.SYMBOLS) == set(_capi.PUBLIC_SYMBOLS) | set(_capi.DEBUG_SYMBOLS)
    assert not set(_capi.PUBLIC_SYMBOLS) & set(_capi.DEBUG_SYMBOLS)
    other = set(header_functions(only=("insfm_passes.h", "insfm_tracks.h")))  # (their own headers, same library)
    ba = {n for n in _capi.PUBLIC_SYMBOLS if not n.startswith("insfm_gp_")} - other
    assert set(header_functions(only=("insfm_ba.h",))) == ba
    assert "debug" not in open(os.path.join(REPO, "include", "insfm_ba.h")).read()
    assert set(header_functions(only=("insfm_ba_debug.h",))) == set(_capi.DEBUG_SYMBOLS)
    public = set(header_functions(only=("insfm_ba.h", "insfm_gp.h", "insfm_passes.h", "insfm_tracks.h")))
    assert public == set(_capi.PUBLIC_SYMBOLS)


def test_struct_layout_matches_header():
    # field order/size of insfm_ba_desc as the C compiler sees it
    d = _capi.default_desc()
    assert d.huber_delta == 1.0 and d.tr_radius == 1e4 and d.tr_max == 1e10 and d.tr_down == 1 / 16
    assert d.max_rejects == 30 and abs(d.pcg_tol - 1e-5) < 1e-20 and d.world_size == 1 and d.cam_model == 2


def _create(desc, uv, cam, pt, pp):
    L = _capi.load()
    h = ctypes.c_void_p()
    rc = L.insfm_ba_create(ctypes.byref(desc), uv.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                           cam.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), pt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                           pp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, ctypes.byref(h))
    msg = L.insfm_ba_last_error(h).decode() if h.value else ""
    if h.value:
        L.insfm_ba_destroy(h)
    return rc, msg


@pytest.mark.parametrize("case", ["model7", "model10", "not_track_major", "cam_oob", "pt_oob", "bad_rank",
                                  "schur_variant"])
def test_create_rejects_bad_inputs_without_gpu(case):
    d = _capi.default_desc()
    uv = np.zeros((4, 2))
    cam = np.array([0, 1, 0, 1], np.int32)
    pt = np.array([0, 0, 1, 1], np.int32)
    pp = np.zeros((2, 2))
    d.n_cams, d.n_points, d.n_obs = 2, 2, 4
    if case == "model7":
        d.cam_model = 7
    elif case == "model10":
        d.cam_model = 10
    elif case == "not_track_major":
        pt = np.array([1, 0, 1, 0], np.int32)
    elif case == "cam_oob":
        cam = np.array([0, 2, 0, 1], np.int32)
    elif case == "pt_oob":
        pt = np.array([0, 0, 1, 5], np.int32)
    elif case == "bad_rank":
        d.world_size, d.rank = 2, 3
    elif case == "schur_variant":  # the round-2/3 Schur variants 1-3 were removed
        d.schur_variant = 3
    rc, msg = _create(d, uv, cam, pt, pp)
    assert rc == _capi.INSFM_BA_EINVAL, (rc, msg)
    assert msg


def test_gp_default_desc_is_torchgp():
    d = _capi.gp_default_desc()
    assert d.huber_delta == 0.1 and d.tr_radius == 1e3 and d.tr_max == 1e8 and d.tr_down == 1 / 16
    assert d.max_rejects == 30 and abs(d.pcg_tol - 1e-5) < 1e-20


@pytest.mark.parametrize("case", ["not_track_major", "cam_oob", "null_factor"])
def test_gp_create_rejects_bad_inputs_without_gpu(case):
    L = _capi.load()
    d = _capi.gp_default_desc()
    d.n_cams, d.n_points, d.n_obs = 2, 2, 4
    t = np.zeros((4, 3))
    cam = np.array([0, 1, 0, 1], np.int32)
    pt = np.array([0, 0, 1, 1], np.int32)
    fc = np.ones(2)
    if case == "not_track_major":
        pt = np.array([1, 0, 1, 0], np.int32)
    elif case == "cam_oob":
        cam = np.array([0, 2, 0, 1], np.int32)
    h = ctypes.c_void_p()
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int32)
    rc = L.insfm_gp_create(ctypes.byref(d), t.ctypes.data_as(dp), cam.ctypes.data_as(ip), pt.ctypes.data_as(ip),
                           None if case == "null_factor" else fc.ctypes.data_as(dp), None, None, ctypes.byref(h))
    msg = L.insfm_ba_last_error(h).decode() if h.value else ""
    if h.value:
        L.insfm_ba_destroy(h)
    assert rc == _capi.INSFM_BA_EINVAL, (rc, msg)
    assert msg


def test_no_cpu_fallback():
    from instantsfm_amd.engine import BundleAdjuster
    with pytest.raises(RuntimeError):
        BundleAdjuster(2, np.zeros((4, 2)), [0, 1, 0, 1], [0, 0, 1, 1], np.zeros((2, 2)), 2, 2, device="cpu")
    from instantsfm_amd.engine import GlobalPositioner
    with pytest.raises(RuntimeError):
        GlobalPositioner(np.zeros((4, 3)), [0, 1, 0, 1], [0, 0, 1, 1], np.ones(2), None, 2, 2, device="cpu")


def test_product_path_does_not_import_oracle():
    for root, _, files in os.walk(os.path.join(REPO, "instantsfm_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(root, f)).read()
                assert "oracle" not in re.sub(r"#.*|//.*", "", src).replace("oracle's", ""), f


def test_library_built_from_this_tree(monkeypatch):
    """insfm_build_info() carries the hash of the sources the library was compiled from (instantsfm_amd/build.py); the
    loader compares it with the tree and refuses a stale or foreign binary."""
    from instantsfm_amd import _capi
    from instantsfm_amd import build as b
    L = _capi.load()
    info = _capi.build_info(L)
    assert info.startswith(f"src={b.source_hash()} arch=gfx950"), info
    monkeypatch.setattr(b, "source_hash", lambda: "0000000000000000")
    with pytest.raises(RuntimeError, match="built from other sources"):
        _capi._check_provenance(L, _capi.LIB_PATH)
