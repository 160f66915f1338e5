"""C-ABI of the bf16 max aggregation and the dense SAGE row tail (bgnn_spmm_max_bf16 /
bgnn_sage_tail_bf16, ABI 16): the header declares them, the library exports them, and every
argument check answers BGNN_E_ARG with its message before anything touches a device (no GPU here:
the pointers below are never dereferenced)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
NAMES = {"bgnn_spmm_max_bf16": 9, "bgnn_sage_tail_bf16": 13}


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 16
    lib = _lib.load()
    assert lib.bgnn_abi_version() == _lib.ABI_VERSION
    for name, n_args in NAMES.items():
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


def _max(csr=None, x=P, ldx=64, H=64, out=P, ldo=64, arg=None, partial=None, null_csr=False):
    from bgnn import _lib

    c = _csr() if csr is None else csr
    return _lib.call("bgnn_spmm_max_bf16", None if null_csr else ctypes.byref(c), x, ldx, H, out, ldo, arg, partial,
                     None)


MAX_CHECKS = [
    (dict(null_csr=True), "null csr"),
    (dict(csr="no_rowptr"), "null csr"),
    (dict(x=None), "null x / out"),
    (dict(out=None), "null x / out"),
    (dict(H=68, ldx=72, ldo=72), "H=68 unsupported"),
    (dict(H=520, ldx=520, ldo=520), "H=520 unsupported"),
    (dict(H=0), "H=0 unsupported"),
    (dict(H=4, ldx=8, ldo=8), "H=4 unsupported"),
    (dict(ldx=68), "ldx must be >= H and a multiple of 8"),
    (dict(ldx=56), "ldx must be >= H and a multiple of 8"),
    (dict(ldo=68), "ldo must be >= H and a multiple of 8"),
    (dict(ldo=56), "ldo must be >= H and a multiple of 8"),
    (dict(x=P + 8), "must be 16-byte aligned"),
    (dict(out=P + 2), "must be 16-byte aligned"),
    (dict(arg=P + 4), "must be 16-byte aligned"),
    (dict(csr="heavy", partial=P + 4), "must be 16-byte aligned"),
    (dict(csr="heavy"), "partial scratch required for heavy rows"),
    (dict(csr="heavy", arg=P), "partial scratch required for heavy rows"),
    (dict(csr="no_plan", partial=P), "heavy rows need the CSR's chunk plan"),
    (dict(csr="chunk255", arg=P), r"chunk must be in \[1, 254\]"),
]


@pytest.mark.parametrize("kw,msg", MAX_CHECKS)
def test_max_argument_checks(kw, msg):
    from bgnn import _lib

    csr = kw.get("csr")
    if csr == "heavy":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1))
    elif csr == "no_plan":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1, chunk_heavy=None))
    elif csr == "chunk255":
        kw = dict(kw, csr=_csr(chunk=255))
    elif csr == "no_rowptr":
        kw = dict(kw, csr=_csr(rowptr=None))
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _max(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


def test_max_empty_graph_is_a_no_op():
    """With no rows the call returns before any launch, with or without the argmax state, and a
    strided pair of planes (ldx = ldo = 2H) passes the checks."""
    from bgnn import _lib

    c = _lib.CsrStruct(rowptr=P, col=P, n_rows=0, nnz=0, chunk=64)
    assert _max(csr=c) == 0
    assert _max(csr=c, arg=P) == 0
    assert _max(csr=c, x=P + 128, ldx=128, ldo=128) == 0


def _tail(y=P, ldy=64, bias=P, scale=P, shift=P, x_prev=P, ldx=64, n_rows=100, H=64, out=P, ldo=64, out_f32=0):
    from bgnn import _lib

    return _lib.call("bgnn_sage_tail_bf16", y, ldy, bias, scale, shift, x_prev, ldx, n_rows, H, out, ldo, out_f32,
                     None)


TAIL_CHECKS = [
    (dict(y=None), "null y / out"),
    (dict(out=None), "null y / out"),
    (dict(H=68, ldy=72, ldx=72, ldo=72), "H=68 unsupported"),
    (dict(H=520, ldy=520, ldx=520, ldo=520), "H=520 unsupported"),
    (dict(H=0), "H=0 unsupported"),
    (dict(ldy=68), "ldy must be >= H and a multiple of 8"),
    (dict(ldy=56), "ldy must be >= H and a multiple of 8"),
    (dict(ldx=68), "ldx must be >= H and a multiple of 8"),
    (dict(ldo=68), "ldo must be >= H and a multiple of 8"),
    (dict(ldo=56), "ldo must be >= H"),
    (dict(ldo=66, out_f32=1), "ldo must be .* multiple of 4"),
    (dict(scale=None), "scale and shift go together"),
    (dict(shift=None), "scale and shift go together"),
    (dict(y=P + 8), "must be 16-byte aligned"),
    (dict(x_prev=P + 2), "must be 16-byte aligned"),
    (dict(out=P + 4), "must be 16-byte aligned"),
]


@pytest.mark.parametrize("kw,msg", TAIL_CHECKS)
def test_tail_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _tail(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


def test_tail_f32_out_takes_ld_multiple_of_4_and_no_rows_is_a_no_op():
    """ldo = 68 is refused for a bf16 out (above) and accepted for an f32 out; an unused ldx is not
    checked; with no rows the call returns before any launch."""
    assert _tail(n_rows=0, ldo=68, out_f32=1) == 0
    assert _tail(n_rows=0, x_prev=None, ldx=0, scale=None, shift=None, bias=None) == 0
