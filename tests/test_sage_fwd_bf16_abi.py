"""C-ABI of the bf16 training aggregation (bgnn_sage_fwd_bf16 / bgnn_sage_fwd_bf16_slots, ABI 19):
the header declares both, the library exports them, and every argument check answers BGNN_E_ARG with
its message before anything touches a device (no GPU here: the pointers below are never
dereferenced)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+bgnn_sage_fwd_bf16\s*\(", text)
    assert re.search(r"\bint32_t\s+bgnn_sage_fwd_bf16_slots\s*\(", text)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 19
    lib = _lib.load()
    assert hasattr(lib, "bgnn_sage_fwd_bf16") and hasattr(lib, "bgnn_sage_fwd_bf16_slots")
    assert len(_lib.SIGNATURES["bgnn_sage_fwd_bf16"][1]) == 11
    assert len(_lib.SIGNATURES["bgnn_sage_fwd_bf16_slots"][1]) == 1


def _csr(n_chunks=0, n_heavy=0, **kw):
    from bgnn import _lib

    f = dict(rowptr=P, col=P, heavy_row=P, heavy_chunk0=P, chunk_heavy=P, n_rows=100, nnz=800, n_heavy=n_heavy,
             n_chunks=n_chunks, chunk=64)
    f.update(kw)
    return _lib.CsrStruct(**f)


def _call(csr=None, z=P, ldz=128, bias=P, H=64, reduce=0, o=P, nrm=P, bn_partial=P, partial=None, null_csr=False):
    from bgnn import _lib

    c = _csr() if csr is None else csr
    ref = None if null_csr else ctypes.byref(c)
    return _lib.call("bgnn_sage_fwd_bf16", ref, z, ldz, bias, H, reduce, o, nrm, bn_partial, partial, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(H=68, ldz=136), "H=68 unsupported"),
    (dict(H=520, ldz=1040), "H=520 unsupported"),
    (dict(reduce=2), "reduce must be sum/mean"),
    (dict(reduce=-1), "reduce must be sum/mean"),
    (dict(null_csr=True), "null csr"),
    (dict(z=None), "null z / o"),
    (dict(o=None), "null z / o"),
    (dict(nrm=None), "null nrm"),
    (dict(ldz=120), "ldz must be >= 2H"),
    (dict(ldz=132), "ldz must be >= 2H and a multiple of 8"),
    (dict(z=P + 8), "must be 16-byte aligned"),
    (dict(o=P + 4), "must be 16-byte aligned"),
    (dict(bias=P + 4), "must be 16-byte aligned"),
    (dict(bn_partial=P + 8), "must be 16-byte aligned"),
    (dict(csr="heavy", partial=P + 4), "must be 16-byte aligned"),
    (dict(csr="heavy"), "partial scratch required"),
    (dict(csr="no_plan", partial=P), "heavy rows need the CSR's chunk plan"),
])
def test_argument_checks(kw, msg):
    from bgnn import _lib

    if kw.get("csr") == "heavy":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1))
    elif kw.get("csr") == "no_plan":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1, chunk_heavy=None))
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _call(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


def test_slots_of_a_null_csr_and_empty_graph_is_a_no_op():
    """With no rows the call returns before any launch (NULL bias and statistics are legal); the
    slot query refuses a NULL CSR with -1, as bgnn_sage_fwd_slots does."""
    from bgnn import _lib

    c = _lib.CsrStruct(rowptr=P, col=P, n_rows=0, nnz=0, chunk=64)
    assert _call(csr=c) == 0
    assert _call(csr=c, bias=None, bn_partial=None) == 0
    assert _lib.load().bgnn_sage_fwd_bf16_slots(None) == -1
    # 100 rows without a group plan: one row per wave, 25 blocks of 4 waves rounded up to whole XCD sets of 8;
    # a CSR with chunks adds one slot per heavy row
    assert _lib.query("bgnn_sage_fwd_bf16_slots", ctypes.byref(_csr())) == 32
    assert _lib.query("bgnn_sage_fwd_bf16_slots", ctypes.byref(_csr(n_chunks=3, n_heavy=2))) == 34
