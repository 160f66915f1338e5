"""C-ABI of the extended per-graph losses: bgnn_graph_loss_ex / bgnn_force_scale and their workspace
queries (additive to ABI 22). The header declares them, the library exports them with the same
argument counts as bgnn._lib's table, and every argument check answers BGNN_E_ARG before anything
touches a device (no GPU here: the pointers below are never dereferenced)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # an aligned non-NULL "pointer"
ENTRIES = {
    "bgnn_graph_loss_ex_ws_bytes": ("size_t", 3),
    "bgnn_graph_loss_ex": ("int", 19),
    "bgnn_force_scale_ws_bytes": ("size_t", 1),
    "bgnn_force_scale": ("int", 11),
}


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION
    lib = _lib.load()
    assert lib.bgnn_abi_version() == _lib.ABI_VERSION
    for name, (ret, n_args) in ENTRIES.items():
        decl = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (ret, name), text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name


def test_public_names():
    import bgnn
    from bgnn import losses

    for name in ("ScaledGraphMAELoss", "ScaledGraphMSELoss", "ScaledGraphRELoss", "get_loss_function"):
        assert getattr(bgnn, name) is getattr(losses, name) and name in bgnn.__all__
    assert losses.FUSED_CRITERIA <= {"graph_mixed", "graph_max_rel", "graph_mae_scaled", "graph_mse_scaled",
                                     "graph_rel_scaled"}


def _loss(pred=P, target=P, N=100, C=3, rowptr=P, col=P, B=4, kind=4, eps=1e-8, mult=1.0, scale=None, center=None,
          q=0.2, mult_dev=None, loss=P, dpred=P, ws=P, ws_bytes=1 << 20):
    from bgnn import _lib

    return _lib.call("bgnn_graph_loss_ex", pred, target, N, C, rowptr, col, B, kind, eps, mult, scale, center, q,
                     mult_dev, loss, dpred, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(kind=6), "kind 6 unknown"),
    (dict(kind=-1), "kind -1 unknown"),
    (dict(C=0), "C=0 unsupported"),
    (dict(C=9), "C=9 unsupported"),
    (dict(N=0), "must be in"),
    (dict(B=0), "must be in"),
    (dict(N=2 ** 30, C=8), "must be in"),
    (dict(q=-0.1), "outside"),
    (dict(q=1.5), "outside"),
    (dict(q=float("nan")), "outside"),
    (dict(pred=None), "null pointer"),
    (dict(target=None), "null pointer"),
    (dict(rowptr=None), "null pointer"),
    (dict(col=None), "null pointer"),
    (dict(loss=None), "null pointer"),
    (dict(ws=None), "workspace too small"),
    (dict(ws=P + 4), "not 8-byte aligned"),
    (dict(ws_bytes=0), "workspace too small"),
])
def test_graph_loss_ex_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _loss(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


def test_graph_loss_ex_workspace():
    from bgnn import _lib

    for N, C, B in ((100, 3, 4), (3000, 3, 300), (80656, 2, 16), (10 ** 7, 8, 1)):
        n = _lib.query("bgnn_graph_loss_ex_ws_bytes", N, C, B)
        # two sums per (graph, segment-block) and one value per graph, on bgnn_graph_loss's segmentation
        assert n == 2 * _lib.query("bgnn_graph_loss_ws_bytes", N, C, B) + 8 * B
        for kind in range(6):
            with pytest.raises(_lib.BgnnError, match="workspace too small"):
                _loss(N=N, C=C, B=B, kind=kind, ws_bytes=n - 1)
    assert _lib.query("bgnn_graph_loss_ex_ws_bytes", 100, 3, 0) == 0


def _force(x=P, N=100, ldx=16, c0=3, nc=2, flag_col=15, min_scale=0.1, out=P, ws=P, ws_bytes=1 << 20):
    from bgnn import _lib

    return _lib.call("bgnn_force_scale", x, N, ldx, c0, nc, flag_col, min_scale, out, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(N=0), "N must be in"),
    (dict(N=2 ** 31), "N must be in"),
    (dict(nc=0), "columns"),
    (dict(nc=9), "columns"),
    (dict(c0=-1), "columns"),
    (dict(c0=15, nc=2), "columns"),
    (dict(flag_col=16), "flag column 16 outside"),
    (dict(x=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(ws=None), "workspace too small"),
    (dict(ws=P + 4), "not 8-byte aligned"),
    (dict(ws_bytes=0), "workspace too small"),
])
def test_force_scale_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _force(**kw)
    assert e.value.code == 1001


def test_force_scale_workspace():
    from bgnn import _lib

    assert _lib.query("bgnn_force_scale_ws_bytes", 0) == 0
    assert _lib.query("bgnn_force_scale_ws_bytes", 1) == 8
    assert _lib.query("bgnn_force_scale_ws_bytes", 257) == 16
    assert _lib.query("bgnn_force_scale_ws_bytes", 10 ** 7) == 256 * 8
    for N in (1, 257, 80656):
        n = _lib.query("bgnn_force_scale_ws_bytes", N)
        with pytest.raises(_lib.BgnnError, match="workspace too small"):
            _force(N=N, ws_bytes=n - 1)
