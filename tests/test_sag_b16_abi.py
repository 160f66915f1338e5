"""C-ABI of SAGPooling on bf16 rows (bgnn_sag_score_bf16 and bgnn_gather_scale_bf16, additive to
ABI 22): the header declares both, the library exports them with the argument counts of
bgnn._lib's table, the ABI version stays 22 on all three sides, and every argument check answers
BGNN_E_ARG before anything touches a device (no GPU here: the pointers below are never
dereferenced; the CSR descriptor is a host struct). The model carries the infer_bf16_sag flag, off
by default, and both inference drivers the bf16_sag keyword."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
ENTRIES = {"bgnn_sag_score_bf16": 12, "bgnn_gather_scale_bf16": 10}
E_ARG = 1001   # BGNN_E_ARG


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == 22
    assert _lib.ABI_VERSION == 22
    lib = _lib.load()
    assert lib.bgnn_abi_version() == 22
    for name, n_args in ENTRIES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args


def _csr(n_rows=100, rowptr=P, col=P, n_heavy=0, heavy_row=None, chunk=64):
    from bgnn import _lib

    return _lib.CsrStruct(rowptr=rowptr, col=col, heavy_row=heavy_row, n_rows=n_rows, nnz=10, n_heavy=n_heavy,
                          n_chunks=0, chunk=chunk)


def _score(csr="default", csr_rows=None, x=P, ldx=64, N=100, H=64, w_l=P, w_r=P, bias=P, sgn=1.0, score=P, ws=P):
    from bgnn import _lib

    if csr == "default":
        csr = _csr(N if csr_rows is None else csr_rows)
    ref = ctypes.byref(csr) if csr is not None else None
    return _lib.call("bgnn_sag_score_bf16", ref, x, ldx, N, H, w_l, w_r, bias, sgn, score, ws, None)


def _gather(x=P, ldx=64, H=64, perm=P, score=P, K=50, m=1.0, out=P, ldo=64):
    from bgnn import _lib

    return _lib.call("bgnn_gather_scale_bf16", x, ldx, H, perm, score, K, m, out, ldo, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(H=68, ldx=72), "H=68 unsupported"),
    (dict(H=0), "H=0 unsupported"),
    (dict(H=4, ldx=8), "H=4 unsupported"),
    (dict(H=520, ldx=520), "H=520 unsupported"),
    (dict(ldx=56), "ldx=56 must be >= H and a multiple of 8"),
    (dict(ldx=68), "ldx=68 must be >= H and a multiple of 8"),
    (dict(ldx=0), "ldx=0 must be >= H and a multiple of 8"),
    (dict(x=P + 2), "x must be 16-byte aligned"),
    (dict(x=P + 8), "x must be 16-byte aligned"),
    (dict(x=None), "null x"),
    (dict(w_l=None), "null w_l / w_r / score / ws"),
    (dict(w_r=None), "null w_l / w_r / score / ws"),
    (dict(score=None), "null w_l / w_r / score / ws"),
    (dict(ws=None), "null w_l / w_r / score / ws"),
    (dict(N=-1), "N < 0"),
    (dict(csr=None), "null csr"),
    (dict(csr_rows=99), "the CSR has 99 rows, x 100"),
])
def test_score_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=re.escape(msg)) as e:
        _score(**kw)
    assert e.value.code == E_ARG
    assert "sag_score_bf16" in str(e.value)


def test_score_heavy_rows_need_the_plan():
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match="heavy rows need the CSR's chunk plan") as e:
        _score(csr=_csr(100, n_heavy=2, heavy_row=None))
    assert e.value.code == E_ARG
    with pytest.raises(_lib.BgnnError, match="null csr") as e:
        _score(csr=_csr(100, rowptr=None))
    assert e.value.code == E_ARG


@pytest.mark.parametrize("kw,msg", [
    (dict(H=68, ldx=72, ldo=72), "H=68 unsupported"),
    (dict(H=0), "H=0 unsupported"),
    (dict(H=520, ldx=520, ldo=520), "H=520 unsupported"),
    (dict(ldx=56), "ldx=56 must be >= H and a multiple of 8"),
    (dict(ldx=68), "ldx=68 must be >= H and a multiple of 8"),
    (dict(ldo=56), "ldo=56 must be >= H and a multiple of 8"),
    (dict(ldo=100), "ldo=100 must be >= H and a multiple of 8"),
    (dict(x=P + 4), "x must be 16-byte aligned"),
    (dict(out=P + 8), "out must be 16-byte aligned"),
    (dict(x=None), "null x"),
    (dict(out=None), "null out"),
    (dict(perm=None), "null perm / score"),
    (dict(score=None), "null perm / score"),
    (dict(K=-1), "K < 0"),
])
def test_gather_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=re.escape(msg)) as e:
        _gather(**kw)
    assert e.value.code == E_ARG
    assert "gather_scale_bf16" in str(e.value)


def test_no_rows_is_a_no_op():
    assert _score(N=0) == 0
    assert _score(N=0, csr=None, x=None, score=None, ws=None) == 0
    assert _gather(K=0) == 0
    assert _gather(K=0, x=None, out=None, perm=None) == 0


def test_flag_drivers_and_package_surface():
    import bgnn

    model = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=2, model_name="GraphSAGE_SAG")
    assert model.infer_bf16_sag is False and model.infer_bf16 is False
    for fn in (bgnn.evaluate, bgnn.evaluate_nodes):
        params = inspect.signature(fn).parameters
        assert params["bf16_sag"].default is None
        assert params["bf16"].default is None
    for name in ("sag_score_bf16", "gather_scale_bf16", "sag_pool_bf16"):
        assert callable(getattr(bgnn, name)) and getattr(bgnn, name) is getattr(bgnn.pool, name)
    # off by default, and the flag alone (infer_bf16 off) does not turn the path on
    import torch
    x = torch.zeros(4, 16)
    model.eval()
    model.infer_bf16_sag = True
    with torch.no_grad():
        assert model._sag_bf16_on(x) is False
