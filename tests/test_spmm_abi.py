"""C-ABI of the f32 aggregation entry points with the plain epilogue (bgnn_spmm_fwd, bgnn_spmm_bwd,
bgnn_spmm_bwd_add, bgnn_spmm_bwd_max, bgnn_spmm_max_arg_bytes): the header declares them, the library
exports them, and every argument check answers BGNN_E_ARG with its message before anything touches a
device (no GPU here: the pointers below are never dereferenced) -- the checks the entry points
always had, and the ones for operands a kernel would otherwise dereference as NULL: x / out / g / gx
with rows, col with entries, a pointer of the chunk plan with chunks, a negative row count, an
addend without its ld. A CSR without rows returns BGNN_OK without a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
NAMES = {"bgnn_spmm_fwd": 10, "bgnn_spmm_bwd": 13, "bgnn_spmm_bwd_add": 14, "bgnn_spmm_bwd_max": 15}
E_ARG = 1001


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, n_args in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args
    decl = re.search(r"\bsize_t\s+bgnn_spmm_max_arg_bytes\s*\(([^)]*)\)", text)
    assert decl and len(decl.group(1).split(",")) == 3 == len(_lib.SIGNATURES["bgnn_spmm_max_arg_bytes"][1])
    assert hasattr(lib, "bgnn_spmm_max_arg_bytes")


def test_max_arg_bytes_layout():
    """a byte plane [rows, H], heavy_of int32 [rows], arg_h int32 [n_heavy, H], each 256-byte aligned;
    0 for an argument out of range"""
    from bgnn import _lib

    q = lambda *a: _lib.query("bgnn_spmm_max_arg_bytes", *a)   # noqa: E731
    assert q(1003, 512, 2) == (1003 * 512 + 255) // 256 * 256 + (1003 * 4 + 255) // 256 * 256 + 2 * 512 * 4
    assert q(0, 8, 0) == 0 and q(1, 1, 0) == 512
    assert q(-1, 8, 0) == 0 and q(1, 0, 0) == 0 and q(1, 8, -1) == 0


def _csr(kind=None, **kw):
    from bgnn import _lib

    f = dict(rowptr=P, col=P, heavy_row=P, heavy_chunk0=P, chunk_heavy=P, n_rows=100, nnz=800, n_heavy=0, n_chunks=0,
             chunk=64)
    if kind is not None and kind.startswith("heavy"):
        f.update(n_chunks=3, n_heavy=1)
    f.update({"no_rowptr": dict(rowptr=None), "neg_rows": dict(n_rows=-1), "no_col": dict(col=None),
              "heavy_no_row": dict(heavy_row=None), "heavy_no_chunk0": dict(heavy_chunk0=None),
              "heavy_no_owner": dict(chunk_heavy=None), "chunk255": dict(chunk=255), "chunk0": dict(chunk=0),
              "ranges": dict(ranges=P), "empty": dict(n_rows=0, nnz=0, col=None)}.get(kind, {}))
    f.update(kw)
    return _lib.CsrStruct(**f)


def _ref(csr):
    return None if csr == "null" else ctypes.byref(_csr(csr))


def _fwd(csr=None, x=P, ldx=64, H=64, reduce=0, out=P, ldo=64, arg=None, partial=None):
    from bgnn import _lib

    return _lib.call("bgnn_spmm_fwd", _ref(csr), x, ldx, H, reduce, out, ldo, arg, partial, None)


def _bwd(csr=None, perm_t=P, frp=P, g=P, ldg=64, H=64, reduce=0, gx=P, ldgx=64, partial=None, amax=None, heavy_done=0):
    from bgnn import _lib

    return _lib.call("bgnn_spmm_bwd", _ref(csr), perm_t, frp, g, ldg, H, reduce, gx, ldgx, partial, amax, heavy_done, None)


def _add(csr=None, perm_t=P, frp=P, g=P, ldg=64, H=64, reduce=0, addend=P, ld_add=64, gx=P, ldgx=64, partial=None,
         amax=None):
    from bgnn import _lib

    return _lib.call("bgnn_spmm_bwd_add", _ref(csr), perm_t, frp, g, ldg, H, reduce, addend, ld_add, gx, ldgx, partial,
                     amax, None)


def _max(csr=None, perm_t=P, frp=P, fwd_rows=100, g=P, ldg=64, H=64, arg=P, addend=None, ld_add=0, gx=P, ldgx=64,
         partial=None, amax=None):
    from bgnn import _lib

    return _lib.call("bgnn_spmm_bwd_max", _ref(csr), perm_t, frp, fwd_rows, g, ldg, H, arg, addend, ld_add, gx, ldgx,
                     partial, amax, None)


# the checks every transpose shares (spmm_bwd_impl), in the order they run
SHARED_BWD = [
    (dict(csr="null"), "spmm_bwd: null csr"),
    (dict(csr="no_rowptr"), "spmm_bwd: null csr"),
    (dict(H=0), "spmm_bwd: bad H/ld"),
    (dict(ldg=56), "spmm_bwd: bad H/ld"),
    (dict(ldgx=56), "spmm_bwd: bad H/ld"),
    (dict(csr="heavy"), "spmm_bwd: partial scratch required"),
    (dict(csr="neg_rows"), "spmm_bwd: negative n_rows"),
    (dict(g=None), "spmm_bwd: null g / gx"),
    (dict(gx=None), "spmm_bwd: null g / gx"),
    (dict(csr="no_col"), "spmm_bwd: null col"),
    (dict(csr="heavy_no_row", partial=P), "spmm_bwd: heavy rows need the CSR's chunk plan"),
    (dict(csr="heavy_no_chunk0", partial=P), "spmm_bwd: heavy rows need the CSR's chunk plan"),
    (dict(csr="heavy_no_owner", partial=P), "spmm_bwd: heavy rows need the CSR's chunk plan"),
]

CHECKS = [
    (_fwd, dict(csr="null"), "spmm_fwd: null csr"),
    (_fwd, dict(csr="no_rowptr"), "spmm_fwd: null csr"),
    (_fwd, dict(H=0), "spmm_fwd: bad H/ld"),
    (_fwd, dict(H=-4), "spmm_fwd: bad H/ld"),
    (_fwd, dict(ldx=56), "spmm_fwd: bad H/ld"),
    (_fwd, dict(ldo=56), "spmm_fwd: bad H/ld"),
    (_fwd, dict(reduce=3), "spmm_fwd: bad reduce 3"),
    (_fwd, dict(reduce=-1), "spmm_fwd: bad reduce -1"),
    (_fwd, dict(csr="heavy"), "spmm_fwd: partial scratch required for heavy rows"),
    (_fwd, dict(csr="neg_rows"), "spmm_fwd: negative n_rows"),
    (_fwd, dict(x=None), "spmm_fwd: null x / out"),
    (_fwd, dict(out=None), "spmm_fwd: null x / out"),
    (_fwd, dict(csr="no_col"), "spmm_fwd: null col"),
    (_fwd, dict(csr="heavy_no_row", partial=P), "spmm_fwd: heavy rows need the CSR's chunk plan"),
    (_fwd, dict(csr="heavy_no_chunk0", partial=P), "spmm_fwd: heavy rows need the CSR's chunk plan"),
    (_fwd, dict(csr="heavy_no_owner", partial=P), "spmm_fwd: heavy rows need the CSR's chunk plan"),
    (_fwd, dict(csr="chunk255", reduce=2, arg=P), r"chunk must be in \[1, 254\] for the compact argmax \(got 255\)"),
    (_fwd, dict(csr="chunk0", reduce=2, arg=P), r"chunk must be in \[1, 254\] for the compact argmax \(got 0\)"),
    (_bwd, dict(reduce=2), "spmm_bwd: max aggregation takes bgnn_spmm_bwd_max"),
    (_bwd, dict(heavy_done=1), "spmm_bwd: heavy_done needs the CSR's ranges"),
    (_bwd, dict(csr="null", heavy_done=1), "spmm_bwd: heavy_done needs the CSR's ranges"),
    (_bwd, dict(reduce=1, frp=None), r"spmm_bwd\(mean\): fwd_rowptr required"),
    (_add, dict(reduce=2), "spmm_bwd_add: max aggregation takes bgnn_spmm_bwd_max"),
    (_add, dict(ld_add=0), "spmm_bwd: bad ld_add"),          # an addend whose ld was not given
    (_add, dict(ld_add=56), "spmm_bwd: bad ld_add"),
    (_add, dict(reduce=1, frp=None), r"spmm_bwd\(mean\): fwd_rowptr required"),
    (_max, dict(perm_t=None), "spmm_bwd_max: perm_t, fwd_rowptr and arg required"),
    (_max, dict(frp=None), "spmm_bwd_max: perm_t, fwd_rowptr and arg required"),
    (_max, dict(arg=None), "spmm_bwd_max: perm_t, fwd_rowptr and arg required"),
    (_max, dict(fwd_rows=-1), "spmm_bwd_max: perm_t, fwd_rowptr and arg required"),
    (_max, dict(addend=P, ld_add=0), "spmm_bwd: bad ld_add"),
] + [(fn, kw, msg) for fn in (_bwd, _add, _max) for kw, msg in SHARED_BWD]


@pytest.mark.parametrize("i", range(len(CHECKS)), ids=[f"{c[0].__name__[1:]}-{'-'.join(f'{k}={v}' for k, v in c[1].items())}"
                                                        for c in CHECKS])
def test_argument_checks(i):
    from bgnn import _lib

    fn, kw, msg = CHECKS[i]
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        fn(**kw)
    assert e.value.code == E_ARG


def test_no_rows_is_a_no_op():
    """n_rows == 0: BGNN_OK before any launch, whatever the operands (NULL x / out / col included)"""
    for reduce in (0, 1, 2):
        assert _fwd(csr="empty", reduce=reduce, x=None, out=None) == 0
    assert _fwd(csr="empty", reduce=2, arg=P) == 0
    for reduce in (0, 1):
        assert _bwd(csr="empty", reduce=reduce, g=None, gx=None) == 0
        assert _add(csr="empty", reduce=reduce, g=None, gx=None) == 0
    assert _max(csr="empty", fwd_rows=0, g=None, gx=None) == 0
