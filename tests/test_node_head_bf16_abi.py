"""C-ABI of the node-level decoder tail on bf16 rows (bgnn_head2_fwd_bf16, additive to ABI 22): the
header declares it, the library exports it with the argument count of bgnn._lib's table, the ABI
version stays 22 on all three sides, and every argument check answers BGNN_E_ARG before anything
touches a device (no GPU here: the pointers below are never dereferenced). evaluate_nodes carries
the two keywords of the bf16 decoder path."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
NAME = "bgnn_head2_fwd_bf16"
N_ARGS = 12


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == 22
    assert _lib.ABI_VERSION == 22
    lib = _lib.load()
    assert lib.bgnn_abi_version() == 22
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, text)
    assert decl, NAME
    assert len(decl.group(1).split(",")) == N_ARGS
    assert hasattr(lib, NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == N_ARGS


def _fwd(x=P, ldx=128, N=100, D0=128, D1=64, C=3, W1=P, b1=P, W2=P, b2=P, y=P):
    from bgnn import _lib

    return _lib.call(NAME, x, ldx, N, D0, D1, C, W1, b1, W2, b2, y, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(D0=96, ldx=96), "shape 96x64x3 not built"),
    (dict(D0=256, ldx=256), "shape 256x64x3 not built"),
    (dict(C=9), "shape 128x64x9 not built"),
    (dict(C=0), "shape 128x64x0 not built"),
    (dict(D1=128), "shape 128x128x3 not built"),
    (dict(N=-1), "N < 0"),
    (dict(x=None), "null pointer"),
    (dict(W1=None), "null pointer"),
    (dict(W2=None), "null pointer"),
    (dict(y=None), "null pointer"),
    (dict(x=P + 2), "x must be 16-byte aligned"),
    (dict(x=P + 8), "x must be 16-byte aligned"),
    (dict(ldx=120), "ldx=120 must be >= D0 and a multiple of 8"),
    (dict(D0=64, ldx=56), "ldx=56 must be >= D0 and a multiple of 8"),
    (dict(ldx=132), "ldx=132 must be >= D0 and a multiple of 8"),
    (dict(ldx=0), "ldx=0 must be >= D0 and a multiple of 8"),
])
def test_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _fwd(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG
    assert "head2_bf16" in str(e.value)


def test_no_rows_is_a_no_op():
    assert _fwd(N=0) == 0
    assert _fwd(N=0, x=None, y=None) == 0


def test_driver_and_package_surface():
    import bgnn

    params = inspect.signature(bgnn.evaluate_nodes).parameters
    assert params["bf16"].default is None
    assert params["return_predictions"].default is False
    assert callable(bgnn.node_head_bf16) and bgnn.node_head_bf16 is bgnn.fused.node_head_bf16
    model = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=1, prediction_type="static_disp",
                         model_name="GraphSage_addAggr")
    assert model.infer_bf16 is False and model.infer_bf16_decoder is False
