"""C-ABI of bgnn_sage_apply_pool and bgnn_pool_grad_scale (ABI 18): the header declares them, the
library exports them, the Python binding agrees on the version and the argument counts, and every
argument check answers BGNN_E_ARG with its message before anything touches a device (no GPU here:
the pointers below are never dereferenced, and every call in this file is one the library rejects
before a launch, or returns from before one)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
Q = P + 4  # a misaligned one
NAMES = ("bgnn_sage_apply_pool", "bgnn_pool_grad_scale")


def test_header_library_and_binding_agree():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 18
    lib = _lib.load()
    assert lib.bgnn_abi_version() == _lib.ABI_VERSION
    for name in NAMES:
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert decl, name
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
    assert len(_lib.SIGNATURES["bgnn_sage_apply_pool"][1]) == 16
    assert len(_lib.SIGNATURES["bgnn_pool_grad_scale"][1]) == 6


def _csr(**kw):
    from bgnn import _lib

    f = dict(rowptr=P, col=P, heavy_row=P, heavy_chunk0=P, chunk_heavy=P, n_rows=3, nnz=100, n_heavy=0, n_chunks=0,
             chunk=64)
    f.update(kw)
    return _lib.CsrStruct(**f)


def pool_(o=P, scale=P, shift=P, x_prev=P, skip=1, p=0.1, seed=7, n_rows=100, H=64, x_next=P, amax=P, csr=None,
          null_csr=False, reduce=1, partial=None, pooled=P):
    c = _csr(**(csr or {}))   # (byref keeps the struct alive)
    return ("bgnn_sage_apply_pool", o, scale, shift, x_prev, skip, p, seed, n_rows, H, x_next, amax,
            None if null_csr else ctypes.byref(c), reduce, partial, pooled, None)


def scale_(g=P, rowptr=P, segments=3, H=64, out=P):
    return ("bgnn_pool_grad_scale", g, rowptr, segments, H, out, None)


HEAVY = dict(n_chunks=2, n_heavy=1)
CHECKS = [
    (pool_(o=None), "sage_apply_pool: null o"),
    (pool_(n_rows=-1), "sage_apply_pool: negative n_rows"),
    (pool_(H=66), "sage_apply_pool: H must be a multiple of 4"),
    (pool_(H=0), "sage_apply_pool: H must be a multiple of 4"),
    (pool_(p=1.0), "dropout p must be in \\[0, 1\\)"),
    (pool_(p=-0.5), "dropout p must be in \\[0, 1\\)"),
    (pool_(p=float("nan")), "dropout p must be in \\[0, 1\\)"),
    (pool_(scale=None), "scale/shift must both be set or NULL"),
    (pool_(shift=None), "scale/shift must both be set or NULL"),
    (pool_(x_prev=None), "skip requires x_prev"),
    (pool_(o=Q), "sage_apply_pool: pointers must be 16-byte aligned"),
    (pool_(x_next=Q), "sage_apply_pool: pointers must be 16-byte aligned"),
    (pool_(x_prev=Q, skip=0), "sage_apply_pool: pointers must be 16-byte aligned"),
    (pool_(scale=Q), "sage_apply_pool: pointers must be 16-byte aligned"),
    (pool_(shift=Q), "sage_apply_pool: pointers must be 16-byte aligned"),
    (pool_(null_csr=True), "sage_apply_pool: null pool csr"),
    (pool_(csr=dict(rowptr=None)), "sage_apply_pool: null pool csr"),
    (pool_(reduce=2), "sage_apply_pool: reduce must be sum/mean"),
    (pool_(reduce=-1), "sage_apply_pool: reduce must be sum/mean"),
    (pool_(csr=dict(n_rows=-1)), "sage_apply_pool: negative segment count"),
    (pool_(csr=dict(nnz=99)), "the pool must list each of the n_rows rows once"),
    (pool_(csr=dict(nnz=101)), "the pool must list each of the n_rows rows once"),
    (pool_(csr=dict(col=None)), "sage_apply_pool: null col"),
    (pool_(pooled=None), "sage_apply_pool: null pooled"),
    (pool_(csr=HEAVY), "heavy segments need partial and the CSR's chunk plan"),
    (pool_(csr=dict(HEAVY, chunk=0), partial=P), "heavy segments need partial and the CSR's chunk plan"),
    (pool_(csr=dict(HEAVY, heavy_row=None), partial=P), "heavy segments need partial and the CSR's chunk plan"),
    (pool_(csr=dict(HEAVY, heavy_chunk0=None), partial=P), "heavy segments need partial and the CSR's chunk plan"),
    (pool_(csr=dict(HEAVY, chunk_heavy=None), partial=P), "heavy segments need partial and the CSR's chunk plan"),
    (pool_(csr=HEAVY, partial=Q), "partial / pooled must be 16-byte aligned"),
    (pool_(pooled=Q), "partial / pooled must be 16-byte aligned"),
    (scale_(segments=-1), "pool_grad_scale: bad sizes"),
    (scale_(H=0), "pool_grad_scale: bad sizes"),
    (scale_(g=None), "pool_grad_scale: null pointer"),
    (scale_(rowptr=None), "pool_grad_scale: null pointer"),
    (scale_(out=None), "pool_grad_scale: null pointer"),
]


@pytest.mark.parametrize("i", range(len(CHECKS)), ids=[f"{c[0][0][5:]}-{i}" for i, c in enumerate(CHECKS)])
def test_argument_checks(i):
    from bgnn import _lib

    args, msg = CHECKS[i]
    name, args = args[0], args[1:]
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _lib.call(name, *args)
    assert e.value.code == 1001, f"{name}: {e.value}"   # BGNN_E_ARG; a HIP code means the call reached a launch


def test_without_rows_nothing_is_launched():
    """n_rows == 0 (an empty pool) and segments == 0 return before any launch, also with NULL data."""
    from bgnn import _lib

    name, *args = pool_(n_rows=0, o=None, x_next=None, csr=dict(nnz=0, col=None))
    assert _lib.call(name, *args) == 0
    name, *args = scale_(segments=0, g=None, rowptr=None, out=None)
    assert _lib.call(name, *args) == 0


def test_stale_argument_count_is_refused():
    from bgnn import _lib

    name, *args = pool_()
    with pytest.raises(TypeError, match="takes 16 arguments"):
        _lib.call(name, *args[:-1])
