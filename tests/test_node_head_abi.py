"""C-ABI of the node-level head (ABI 21): the decoder tail kernel's entries (bgnn_head2_*) and the
per-graph loss (bgnn_graph_loss). The header declares them, the library exports them with the same
argument counts as bgnn._lib's table, and every argument check answers BGNN_E_ARG before anything
touches a device (no GPU here: the pointers below are never dereferenced)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
ENTRIES = {
    "bgnn_head2_supported": ("int", 3),
    "bgnn_head2_geometry": ("int", 1),
    "bgnn_head2_fwd": ("int", 11),
    "bgnn_head2_bwd_ws_bytes": ("size_t", 3),
    "bgnn_head2_bwd": ("int", 17),
    "bgnn_graph_loss_ws_bytes": ("size_t", 3),
    "bgnn_graph_loss": ("int", 17),
}


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 21
    lib = _lib.load()
    assert lib.bgnn_abi_version() == _lib.ABI_VERSION
    for name, (ret, n_args) in ENTRIES.items():
        decl = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (ret, name), text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name


def test_exported_names():
    import bgnn

    assert callable(bgnn.node_head) and bgnn.fused.FUSED_NODE_HEAD is True
    assert bgnn.losses.FUSED_GRAPH_LOSS is True
    s = bgnn.ColumnScaler([1.0, 2.0], [3.0, 4.0])
    import torch
    v = torch.tensor([[1.0, 1.0], [0.0, -1.0]])
    assert torch.equal(s.denormalize(v), v * torch.tensor([3.0, 4.0]) + torch.tensor([1.0, 2.0]))
    assert torch.allclose(s.normalize(s.denormalize(v)), v)
    assert torch.equal(s.denormalize_displacement(v), s.denormalize(v))
    assert torch.equal(s.denormalize_gp_stresses(v), s.denormalize(v))


@pytest.mark.parametrize("D0,D1,C,ok", [(64, 64, 1, 1), (64, 64, 8, 1), (128, 64, 1, 1), (128, 64, 3, 1),
                                        (128, 64, 8, 1), (96, 64, 3, 0), (256, 64, 3, 0), (32, 64, 3, 0),
                                        (128, 64, 9, 0), (128, 64, 0, 0), (64, 128, 3, 0), (64, 32, 2, 0)])
def test_head2_supported(D0, D1, C, ok):
    from bgnn import _lib

    assert _lib.query("bgnn_head2_supported", D0, D1, C) == ok


def test_head2_geometry_and_workspace():
    from bgnn import _lib

    rows, fwd, bwd = (_lib.query("bgnn_head2_geometry", i) for i in range(3))
    assert rows > 0 and fwd > 0 and bwd > 0
    assert _lib.query("bgnn_head2_geometry", 3) == -1
    part = lambda D0, C: (64 * D0 + 64 + 64 * C + C + 3) // 4 * 4 * 4   # noqa: E731  (bytes per slot)
    for D0, C in ((64, 1), (128, 3), (128, 8)):
        one = _lib.query("bgnn_head2_bwd_ws_bytes", 1, D0, C)
        assert one % part(D0, C) == 0
        groups = one // part(D0, C) - 1
        # one slot per workgroup: grows with the tiles up to the backward's grid, then stays
        assert _lib.query("bgnn_head2_bwd_ws_bytes", rows * 5, D0, C) == (5 + groups) * part(D0, C)
        assert (_lib.query("bgnn_head2_bwd_ws_bytes", rows * bwd * 3, D0, C)
                == _lib.query("bgnn_head2_bwd_ws_bytes", rows * bwd, D0, C) == (bwd + groups) * part(D0, C))
    assert _lib.query("bgnn_head2_bwd_ws_bytes", 100, 96, 3) == 0


def _fwd(x=P, N=100, D0=128, D1=64, C=3, W1=P, b1=P, W2=P, b2=P, y=P):
    from bgnn import _lib

    return _lib.call("bgnn_head2_fwd", x, N, D0, D1, C, W1, b1, W2, b2, y, None)


def _bwd(x=P, N=100, D0=128, D1=64, C=3, W1=P, b1=P, W2=P, dy=P, dx=P, dW1=P, db1=P, dW2=P, db2=P, ws=P,
         ws_bytes=1 << 30):
    from bgnn import _lib

    return _lib.call("bgnn_head2_bwd", x, N, D0, D1, C, W1, b1, W2, dy, dx, dW1, db1, dW2, db2, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(D0=96), "shape 96x64x3 not built"),
    (dict(C=9), "shape 128x64x9 not built"),
    (dict(D1=128), "shape 128x128x3 not built"),
    (dict(N=-1), "N < 0"),
    (dict(x=None), "null pointer"),
    (dict(W1=None), "null pointer"),
    (dict(W2=None), "null pointer"),
    (dict(y=None), "null pointer"),
    (dict(x=P + 4), "x must be 16-byte aligned"),
])
def test_head2_fwd_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _fwd(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


@pytest.mark.parametrize("kw,msg", [
    (dict(D0=96), "shape 96x64x3 not built"),
    (dict(C=0), "shape 128x64x0 not built"),
    (dict(N=-1), "N < 0"),
    (dict(dW1=None), "null gradient output"),
    (dict(db2=None), "null gradient output"),
    (dict(x=None), "null pointer"),
    (dict(dy=None), "null pointer"),
    (dict(dx=None), "null pointer"),
    (dict(x=P + 8), "x and dx must be 16-byte aligned"),
    (dict(dx=P + 4), "x and dx must be 16-byte aligned"),
    (dict(ws=None), "workspace too small"),
    (dict(ws_bytes=1024), "workspace too small"),
    (dict(ws=P + 4), "workspace too small or not 16-byte aligned"),
])
def test_head2_bwd_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _bwd(**kw)
    assert e.value.code == 1001


def test_head2_no_rows_forward_is_a_no_op():
    assert _fwd(N=0) == 0
    assert _fwd(N=0, x=None, y=None) == 0


def _loss(pred=P, target=P, N=100, C=3, rowptr=P, col=P, B=4, kind=0, eps=0.1, mult=10000.0, scale=None,
          center=None, loss=P, dpred=P, ws=P, ws_bytes=1 << 20):
    from bgnn import _lib

    return _lib.call("bgnn_graph_loss", pred, target, N, C, rowptr, col, B, kind, eps, mult, scale, center, loss,
                     dpred, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(kind=3), "kind 3 unknown"),
    (dict(kind=-1), "kind -1 unknown"),
    (dict(C=0), "C=0 unsupported"),
    (dict(C=9), "C=9 unsupported"),
    (dict(N=0), "N and B must be"),
    (dict(B=0), "N and B must be"),
    (dict(pred=None), "null pointer"),
    (dict(target=None), "null pointer"),
    (dict(rowptr=None), "null pointer"),
    (dict(col=None), "null pointer"),
    (dict(loss=None), "null pointer"),
    (dict(ws=None), "workspace too small"),
    (dict(ws_bytes=24), "workspace too small"),
    (dict(ws=P + 4), "not 8-byte aligned"),
])
def test_graph_loss_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _loss(**kw)
    assert e.value.code == 1001


def test_graph_loss_workspace():
    from bgnn import _lib

    # one double per (graph, segment-block); a graph's elements split into blocks of about 2048
    assert _lib.query("bgnn_graph_loss_ws_bytes", 3000, 3, 300) == 300 * 8
    assert _lib.query("bgnn_graph_loss_ws_bytes", 80656, 2, 16) == 16 * 5 * 8
    assert _lib.query("bgnn_graph_loss_ws_bytes", 10 ** 7, 8, 1) == 64 * 8
    assert _lib.query("bgnn_graph_loss_ws_bytes", 100, 3, 0) == 0
