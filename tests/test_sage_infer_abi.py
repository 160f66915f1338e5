"""C-ABI of the bf16 inference layer (bgnn_sage_infer_bf16, ABI 14): the header declares it, the
library exports it, and every argument check answers BGNN_E_ARG with its message before anything
touches a device (no GPU here: the pointers below are never dereferenced)."""
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
    assert re.search(r"\bint\s+bgnn_sage_infer_bf16\s*\(", text)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 14
    lib = _lib.load()
    assert hasattr(lib, "bgnn_sage_infer_bf16")
    assert len(_lib.SIGNATURES["bgnn_sage_infer_bf16"][1]) == 15


def _csr(n_chunks=0, n_heavy=0):
    from bgnn import _lib

    return _lib.CsrStruct(rowptr=P, col=P, heavy_row=P, heavy_chunk0=P, chunk_heavy=P, n_rows=100, nnz=800,
                          n_heavy=n_heavy, n_chunks=n_chunks, chunk=64)


def _call(csr=None, z=P, ldz=128, bias=P, scale=P, shift=P, x_prev=P, ldx=64, H=64, reduce=0, out=P, ldo=64,
          out_f32=0, partial=None, null_csr=False):
    from bgnn import _lib

    c = _csr() if csr is None else csr
    ref = None if null_csr else ctypes.byref(c)
    return _lib.call("bgnn_sage_infer_bf16", ref, z, ldz, bias, scale, shift, x_prev, ldx, H, reduce, out, ldo,
                     out_f32, partial, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(H=68, ldz=136, ldx=72, ldo=72), "H=68 unsupported"),
    (dict(H=520, ldz=1040, ldx=520, ldo=520), "H=520 unsupported"),
    (dict(reduce=2), "reduce must be sum/mean"),
    (dict(reduce=-1), "reduce must be sum/mean"),
    (dict(null_csr=True), "null csr"),
    (dict(z=None), "null z / out"),
    (dict(out=None), "null z / out"),
    (dict(ldz=132), "ldz must be"),
    (dict(ldx=68), "ldx must be"),
    (dict(ldo=68), "ldo must be"),
    (dict(ldo=66, out_f32=1), "ldo must be .* multiple of 4"),
    (dict(scale=None), "scale and shift go together"),
    (dict(shift=None), "scale and shift go together"),
    (dict(csr="heavy"), "partial scratch required"),
])
def test_argument_checks(kw, msg):
    from bgnn import _lib

    if kw.get("csr") == "heavy":
        kw = dict(kw, csr=_csr(n_chunks=3, n_heavy=1))
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _call(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


def test_f32_out_takes_ld_multiple_of_4_and_empty_graph_is_a_no_op():
    """ldo = 68 is refused for a bf16 out (above) and accepted for an f32 out; with no rows the call
    returns before any launch."""
    from bgnn import _lib

    c = _lib.CsrStruct(rowptr=P, col=P, n_rows=0, nnz=0, chunk=64)
    assert _call(csr=c, ldo=68, out_f32=1) == 0
