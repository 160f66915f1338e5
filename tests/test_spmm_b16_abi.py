"""C-ABI of the bf16 aggregation and its transpose (bgnn_spmm_fwd_bf16 / bgnn_spmm_bwd_bf16, ABI 15):
the header declares them, the library exports them, and every argument check answers BGNN_E_ARG
with its message before anything touches a device (no GPU here: the pointers below are never
dereferenced)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
NAMES = {"fwd": ("bgnn_spmm_fwd_bf16", 10), "bwd": ("bgnn_spmm_bwd_bf16", 11)}


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 15
    lib = _lib.load()
    for name, n_args in NAMES.values():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args


def _csr(n_chunks=0, n_heavy=0, **kw):
    from bgnn import _lib

    f = dict(rowptr=P, col=P, heavy_row=P, heavy_chunk0=P, chunk_heavy=P, n_rows=100, nnz=800, n_heavy=n_heavy,
             n_chunks=n_chunks, chunk=64)
    f.update(kw)
    return _lib.CsrStruct(**f)


def _call(which, csr=None, x=P, ldx=64, H=64, reduce=0, out=P, ldo=64, out_f32=0, partial=None, null_csr=False,
          fwd_rowptr=P):
    from bgnn import _lib

    c = _csr() if csr is None else csr
    ref = None if null_csr else ctypes.byref(c)
    if which == "fwd":
        return _lib.call("bgnn_spmm_fwd_bf16", ref, x, ldx, H, reduce, out, ldo, out_f32, partial, None)
    return _lib.call("bgnn_spmm_bwd_bf16", ref, fwd_rowptr, x, ldx, H, reduce, out, ldo, out_f32, partial, None)


CHECKS = [
    (dict(H=68, ldx=72, ldo=72), "H=68 unsupported"),
    (dict(H=520, ldx=520, ldo=520), "H=520 unsupported"),
    (dict(H=0), "H=0 unsupported"),
    (dict(reduce=2), "reduce must be sum/mean"),
    (dict(reduce=-1), "reduce must be sum/mean"),
    (dict(null_csr=True), "null csr"),
    (dict(x=None), "null (x|g) / (out|gx)"),
    (dict(out=None), "null (x|g) / (out|gx)"),
    (dict(ldx=68), "ld(x|g) must be >= H and a multiple of 8"),
    (dict(ldx=56), "ld(x|g) must be >= H and a multiple of 8"),
    (dict(ldo=68), "ld(o|gx) must be >= H and a multiple of 8"),
    (dict(ldo=56), "ld(o|gx) must be >= H"),
    (dict(ldo=66, out_f32=1), "ld(o|gx) must be .* multiple of 4"),
    (dict(x=P + 8), "must be 16-byte aligned"),
    (dict(out=P + 2), "must be 16-byte aligned"),
    (dict(csr="heavy", partial=P + 4), "must be 16-byte aligned"),
    (dict(csr="heavy"), "partial scratch required"),
    (dict(csr="no_plan", partial=P), "heavy rows need the CSR's chunk plan"),
]


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("kw,msg", CHECKS)
def test_argument_checks(which, kw, msg):
    from bgnn import _lib

    if kw.get("csr") == "heavy":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1))
    elif kw.get("csr") == "no_plan":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1, chunk_heavy=None))
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _call(which, **kw)
    assert e.value.code == 1001   # BGNN_E_ARG


def test_mean_backward_needs_the_forward_rowptr():
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match="MEAN needs fwd_rowptr") as e:
        _call("bwd", reduce=1, fwd_rowptr=None)
    assert e.value.code == 1001


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_f32_out_takes_ld_multiple_of_4_and_empty_graph_is_a_no_op(which):
    """ldo = 68 is refused for a bf16 output (above) and accepted for an f32 one; with no rows the
    call returns before any launch (a SUM backward needs no fwd_rowptr)."""
    from bgnn import _lib

    c = _lib.CsrStruct(rowptr=P, col=P, n_rows=0, nnz=0, chunk=64)
    assert _call(which, csr=c, ldo=68, out_f32=1, fwd_rowptr=None) == 0
