"""C-ABI of the folded layer's grouped weight products (bgnn_fold_weights_fwd / _bwd, ABI 17): the
header declares them, the library exports them, the Python binding agrees on the version and the
argument counts, and every argument check answers BGNN_E_ARG with its message before anything
touches a device (no GPU here: the pointers below are never dereferenced)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
NAMES = ("bgnn_fold_weights_supported", "bgnn_fold_weights_ws_bytes", "bgnn_fold_weights_fwd",
         "bgnn_fold_weights_bwd")


def test_header_library_and_binding_agree():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 17
    lib = _lib.load()
    assert lib.bgnn_abi_version() == _lib.ABI_VERSION
    for name in NAMES:
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert decl, name
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name


def test_supported_shapes_and_workspace_query():
    from bgnn import _lib

    for H, K in [(64, 32), (128, 128), (80, 48), (512, 128)]:
        assert _lib.query("bgnn_fold_weights_supported", H, K) == 1, (H, K)
    assert _lib.query("bgnn_fold_weights_supported", 0, 128) == 0
    assert _lib.query("bgnn_fold_weights_supported", 512, 0) == 0
    assert _lib.query("bgnn_fold_weights_ws_bytes", 0, 128) == 0
    # K = 2H = 1024 is deep enough for the planner to split dW_in and db_in along K
    assert _lib.query("bgnn_fold_weights_ws_bytes", 512, 128) >= (512 * 128 + 512) * 4 * 2
    assert _lib.query("bgnn_fold_weights_ws_bytes", 64, 32) == 0


def _fwd(H=512, K=128, wcat=P, ld_wcat=None, w_in=P, ld_win=None, b_in=P, famax=P, wf=P, ld_wf=None, bf=P, wf_t=P,
         ld_wft=None, w_amax=P):
    from bgnn import _lib

    return _lib.call("bgnn_fold_weights_fwd", H, K, wcat, H if ld_wcat is None else ld_wcat, w_in,
                     K if ld_win is None else ld_win, b_in, famax, wf, K if ld_wf is None else ld_wf, bf, wf_t,
                     2 * H if ld_wft is None else ld_wft, w_amax, None)


def _bwd(H=512, K=128, dwf=P, ld_dwf=None, dbf=P, wcat=P, ld_wcat=None, w_in=P, ld_win=None, b_in=P, famax=P,
         dwcat=P, ld_dwcat=None, dw_in=P, ld_dwin=None, db_in=P, ws=P, ws_bytes=None):
    from bgnn import _lib

    if ws_bytes is None:
        ws_bytes = _lib.query("bgnn_fold_weights_ws_bytes", H, K)
    return _lib.call("bgnn_fold_weights_bwd", H, K, dwf, K if ld_dwf is None else ld_dwf, dbf, wcat,
                     H if ld_wcat is None else ld_wcat, w_in, K if ld_win is None else ld_win, b_in, famax, dwcat,
                     H if ld_dwcat is None else ld_dwcat, dw_in, K if ld_dwin is None else ld_dwin, db_in, ws,
                     ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(wcat=None), "null pointer"),
    (dict(w_in=None), "null pointer"),
    (dict(b_in=None), "null pointer"),
    (dict(famax=None), "null pointer"),
    (dict(wf=None), "null pointer"),
    (dict(bf=None), "null pointer"),
    (dict(w_amax=None), "null pointer"),
    (dict(K=0), "must be positive"),
    (dict(H=0), "must be positive"),
    (dict(H=-4), "must be positive"),
    (dict(ld_wcat=511), "leading dimension"),
    (dict(ld_win=127), "leading dimension"),
    (dict(ld_wf=64), "leading dimension"),
    (dict(ld_wft=1023), "leading dimension"),
    (dict(H=8192, K=128), "unsupported"),
])
def test_forward_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _fwd(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


@pytest.mark.parametrize("kw,msg", [
    (dict(dwf=None), "null pointer"),
    (dict(dbf=None), "null pointer"),
    (dict(wcat=None), "null pointer"),
    (dict(w_in=None), "null pointer"),
    (dict(b_in=None), "null pointer"),
    (dict(famax=None), "null pointer"),
    (dict(dwcat=None), "null pointer"),
    (dict(dw_in=None), "null pointer"),
    (dict(db_in=None), "null pointer"),
    (dict(K=0), "must be positive"),
    (dict(H=0), "must be positive"),
    (dict(ld_dwf=127), "leading dimension"),
    (dict(ld_dwcat=500), "leading dimension"),
    (dict(ld_dwin=100), "leading dimension"),
    (dict(H=8192, K=128), "unsupported"),
    (dict(ws_bytes=16), "workspace"),
    (dict(ws=None), "workspace"),
])
def test_backward_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _bwd(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


@pytest.mark.parametrize("H,K,product", [
    (1024, 128, (2048, 128, 1024, 0, 0)),   # Wf = Wcat W_in: K = H = 1024 is split along K by the planner
    (64, 1024, (128, 64, 1024, 0, 1)),      # dWcat = dWf W_in^T: K = K_in = 1024 is split
])
def test_supported_tells_what_the_entry_points_accept(H, K, product):
    """A shape whose forward products or dWcat the planner splits along K is not taken (their
    epilogues carry max|Wf|, Wf^T and the outer-product add): the query says so, which sends
    bgnn/fused.py to the GEMM chain, and both entry points refuse it before any launch."""
    from bgnn import _lib

    assert _lib.query("bgnn_gemm_ws_bytes", *product) > 256   # slabs beyond the operand-max head: split-K
    assert _lib.query("bgnn_fold_weights_supported", H, K) == 0
    assert _lib.query("bgnn_fold_weights_ws_bytes", H, K) == 0
    for call in (_fwd, lambda **kw: _bwd(ws_bytes=1 << 30, **kw)):
        with pytest.raises(_lib.BgnnError, match="unsupported") as e:
            call(H=H, K=K)
        assert e.value.code == 1001


def test_supported_and_entry_points_agree_over_a_shape_sweep():
    """Wherever the query answers 0, both entry points refuse the shape (before any launch: there
    is no device here)."""
    from bgnn import _lib

    for H in (4, 64, 80, 256, 512, 1024, 1536, 2048):
        for K in (1, 32, 128, 512, 1024):
            if not _lib.query("bgnn_fold_weights_supported", H, K):
                for call in (_fwd, lambda **kw: _bwd(ws_bytes=1 << 30, **kw)):
                    with pytest.raises(_lib.BgnnError, match="unsupported"):
                        call(H=H, K=K)
