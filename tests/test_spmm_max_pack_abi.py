"""C-ABI of the max layer's pack gather (bgnn_spmm_max_pack_bf16, ABI 20): the header declares it,
the library exports it, and every argument check answers BGNN_E_ARG with its message before
anything touches a device (no GPU here: the pointers below are never dereferenced)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
NAME, N_ARGS = "bgnn_spmm_max_pack_bf16", 9


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 20
    lib = _lib.load()
    assert lib.bgnn_abi_version() == _lib.ABI_VERSION
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, text)
    assert decl, NAME
    assert len(decl.group(1).split(",")) == N_ARGS
    assert hasattr(lib, NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == N_ARGS


def _csr(n_chunks=0, n_heavy=0, **kw):
    from bgnn import _lib

    f = dict(rowptr=P, col=P, heavy_row=P, heavy_chunk0=P, chunk_heavy=P, n_rows=100, nnz=800, n_heavy=n_heavy,
             n_chunks=n_chunks, chunk=64)
    f.update(kw)
    return _lib.CsrStruct(**f)


def _pack(csr=None, x=P, ldx=64, H=64, out=P, ldo=128, arg=P, partial=None, null_csr=False):
    from bgnn import _lib

    c = _csr() if csr is None else csr
    return _lib.call(NAME, None if null_csr else ctypes.byref(c), x, ldx, H, out, ldo, arg, partial, None)


CHECKS = [
    (dict(null_csr=True), "null csr"),
    (dict(csr="no_rowptr"), "null csr"),
    (dict(x=None), "null x / out"),
    (dict(out=None), "null x / out"),
    (dict(arg=None), "null arg"),
    (dict(H=68, ldx=68, ldo=136), "H=68 unsupported"),
    (dict(H=520, ldx=520, ldo=1040), "H=520 unsupported"),
    (dict(H=0), "H=0 unsupported"),
    (dict(H=4, ldx=8, ldo=8), "H=4 unsupported"),
    (dict(ldx=60), "ldx must be >= H and a multiple of 4"),
    (dict(ldx=66), "ldx must be >= H and a multiple of 4"),
    (dict(ldo=120), "ldo must be >= 2H and a multiple of 8"),
    (dict(ldo=132), "ldo must be >= 2H and a multiple of 8"),
    (dict(x=P + 8), "must be 16-byte aligned"),
    (dict(out=P + 2), "must be 16-byte aligned"),
    (dict(arg=P + 4), "must be 16-byte aligned"),
    (dict(csr="heavy", partial=P + 4), "must be 16-byte aligned"),
    (dict(csr="heavy"), "partial scratch required for heavy rows"),
    (dict(csr="no_plan", partial=P), "heavy rows need the CSR's chunk plan"),
    (dict(csr="chunk255"), r"chunk must be in \[1, 254\]"),
    (dict(csr="chunk0"), r"chunk must be in \[1, 254\]"),
]


@pytest.mark.parametrize("kw,msg", CHECKS)
def test_argument_checks(kw, msg):
    from bgnn import _lib

    csr = kw.get("csr")
    if csr == "heavy":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1))
    elif csr == "no_plan":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1, chunk_heavy=None))
    elif csr == "chunk255":
        kw = dict(kw, csr=_csr(chunk=255))
    elif csr == "chunk0":
        kw = dict(kw, csr=_csr(chunk=0))
    elif csr == "no_rowptr":
        kw = dict(kw, csr=_csr(rowptr=None))
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _pack(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


def test_empty_graph_is_a_no_op():
    """With no rows the call returns before any launch; ldx a multiple of 4 (not of 8) and an out
    wider than 2H pass the checks."""
    from bgnn import _lib

    c = _lib.CsrStruct(rowptr=P, col=P, n_rows=0, nnz=0, chunk=64)
    assert _pack(csr=c) == 0
    assert _pack(csr=c, ldx=68, ldo=136) == 0
    assert _pack(csr=c, x=P + 16, out=P + 256) == 0
