"""C-ABI of the bf16-storage GEMM entry points and the bf16 helpers of csrc/elem.hip: every argument
check of bgnn_gemm_bf16, bgnn_gemm_gather_add_bf16, bgnn_gemm_bf16_dropadd, bgnn_gemm_b16_variant,
bgnn_add_dropout_bf16, bgnn_add_dropped_bf16, bgnn_segment_sum_bf16 and bgnn_segment_bcast_bf16
answers BGNN_E_ARG before anything touches a device (no GPU here: the pointers below are never
dereferenced), among them the NULL A / B / C checks of the two bf16 GEMM entry points; M == 0 or
N == 0 (n == 0, n_rows == 0) stays BGNN_OK without a launch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
ENTRIES = {"bgnn_gemm_bf16": 19, "bgnn_gemm_gather_add_bf16": 21, "bgnn_gemm_bf16_dropadd": 14, "bgnn_gemm_b16_variant": 1,
           "bgnn_add_dropout_bf16": 7, "bgnn_add_dropped_bf16": 7, "bgnn_segment_sum_bf16": 10,
           "bgnn_segment_bcast_bf16": 10}


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, n_args in ENTRIES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name


def test_header_matches_the_code():
    text = " ".join(open(HEADER).read().replace(" * ", " ").split())
    assert "Every other value is BGNN_E_ARG (ABI 12 removed the fixed forms 1-14)" in text
    assert "13 = variant 11" not in text and "1-14 = fixed" not in text
    assert "correctly rounded f32 reciprocal of max(deg, 1) -- a product, two roundings, not a division" in text
    assert "when M, N > 0 and C is NULL, or K > 0 too and A or B is NULL" in text
    assert "a kept element is pinned only to |out - (a + w ik)| <= 2^-8 |a + w ik| + 2^-23 (|a| + |w ik|)" in text


def _raises(name, args, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _lib.call(name, *args)
    assert e.value.code == 1001   # BGNN_E_ARG


def _ok(name, args):
    from bgnn import _lib

    assert _lib.call(name, *args) == 0


def _gemm(ta=0, tb=1, M=100, N=64, K=64, alpha=1.0, A=P, lda=None, B=P, ldb=None, beta=0.0, C=P, ldc=None, bias=None,
          relu=0, storage=7, ws=None, ws_bytes=0):
    lda = (M if ta else K) if lda is None else lda
    ldb = (K if tb else N) if ldb is None else ldb
    return "bgnn_gemm_bf16", (ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, N if ldc is None else ldc, bias, relu,
                              storage, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(storage=8), "storage flags must be in \\[0, 8\\)"),
    (dict(storage=-1), "storage flags must be in \\[0, 8\\)"),
    (dict(storage=2), "storage 2 with ta=0 tb=1 is not built"),
    (dict(storage=6), "storage 6 with ta=0 tb=1 is not built"),
    (dict(ta=1, tb=0, storage=4), "storage 4 with ta=1 tb=0 is not built"),
    (dict(ta=1, tb=0, storage=7), "storage 7 with ta=1 tb=0 is not built"),
    (dict(ta=0, tb=0, storage=1), "storage 1 with ta=0 tb=0 is not built"),
    (dict(ta=1, tb=1, storage=3), "storage 3 with ta=1 tb=1 is not built"),
    (dict(A=None), "null A / B / C"), (dict(B=None), "null A / B / C"), (dict(C=None), "null A / B / C"),
    (dict(A=None, storage=0), "null A / B / C"), (dict(C=None, K=0), "null A / B / C"),
    (dict(A=None, ta=1, tb=0, storage=3), "null A / B / C"),
    (dict(ta=2, storage=0), "bad transpose flags"),
    (dict(beta=0.5, storage=4), "beta 0 for a bf16 C"), (dict(beta=0.5, storage=7), "beta 0 for a bf16 C"),
    (dict(M=-1), "negative size"), (dict(N=-1), "negative size"), (dict(K=-1), "negative size"),
    (dict(lda=63), "bad lda"), (dict(ta=1, tb=0, storage=3, lda=99), "bad lda"),
    (dict(ldb=63), "bad ldb"), (dict(ta=1, tb=0, storage=3, ldb=63), "bad ldb"),
    (dict(ldc=63), "bad ldc"),
])
def test_gemm_bf16_argument_checks(kw, msg):
    _raises(*_gemm(**kw), msg)


def test_gemm_bf16_empty_is_a_no_op():
    """M == 0 or N == 0: BGNN_OK, nothing launched, whatever the pointers"""
    for kw in (dict(M=0), dict(N=0), dict(M=0, A=None, B=None, C=None), dict(N=0, A=None, B=None, C=None, ldb=64),
               dict(M=0, N=0, K=0, A=None, B=None, C=None)):
        _ok(*_gemm(**kw))


def _gather(M=100, N=64, K=64, A=P, lda=None, B=P, ldb=None, C=P, ldc=None, bias=None, relu=0, add0=P, idx0=P, ld0=None,
            add1=None, idx1=None, ld1=0, storage=7):
    return "bgnn_gemm_gather_add_bf16", (M, N, K, A, K if lda is None else lda, B, K if ldb is None else ldb, C,
                                         N if ldc is None else ldc, bias, relu, add0, idx0, N if ld0 is None else ld0,
                                         add1, idx1, ld1, storage, None, 0, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(storage=2), "storage must be one of 0, 1, 3, 4, 5, 7"), (dict(storage=6), "storage must be one of"),
    (dict(storage=8), "storage must be one of"), (dict(storage=-1), "storage must be one of"),
    (dict(A=None), "null A / B / C"), (dict(B=None), "null A / B / C"), (dict(C=None), "null A / B / C"),
    (dict(C=None, K=0), "null A / B / C"), (dict(B=None, storage=0), "null A / B / C"),
    (dict(M=-1), "negative size"), (dict(N=-1), "negative size"), (dict(K=-1), "negative size"),
    (dict(add0=None), "add0/idx0/ld0 required"), (dict(idx0=None), "add0/idx0/ld0 required"),
    (dict(ld0=63), "add0/idx0/ld0 required"),
    (dict(add1=P, idx1=None, ld1=64), "bad add1/idx1/ld1"), (dict(add1=P, idx1=P, ld1=63), "bad add1/idx1/ld1"),
    (dict(lda=63), "bad lda"), (dict(ldb=63), "bad ldb"), (dict(ldc=63), "bad ldc"),
])
def test_gemm_gather_add_bf16_argument_checks(kw, msg):
    _raises(*_gather(**kw), msg)


def test_gemm_gather_add_bf16_empty_is_a_no_op():
    for kw in (dict(M=0), dict(N=0, ld0=0), dict(M=0, A=None, B=None, C=None)):
        _ok(*_gather(**kw))


def _dropadd(M=100, N=256, K=64, A=P, lda=None, B=P, ldb=None, C=P, ldc=None, src=P, ld_src=None, p=0.1, seed=7):
    return "bgnn_gemm_bf16_dropadd", (M, N, K, A, K if lda is None else lda, B, K if ldb is None else ldb, C,
                                      N if ldc is None else ldc, src, N if ld_src is None else ld_src, p, seed, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(M=-1), "negative size"), (dict(N=-8), "negative size"), (dict(K=-64), "negative size"),
    (dict(p=1.0), "p must be in \\[0, 1\\)"), (dict(p=-0.25), "p must be in \\[0, 1\\)"),
    (dict(ldc=264), "need ldc == ld_src == N"), (dict(ld_src=264), "need ldc == ld_src == N"),
    (dict(lda=56), "need ldc == ld_src == N"), (dict(ldb=56), "need ldc == ld_src == N"),
    (dict(A=None), "null pointer or N % 8 != 0"), (dict(B=None), "null pointer or N % 8 != 0"),
    (dict(C=None), "null pointer or N % 8 != 0"), (dict(src=None), "null pointer or N % 8 != 0"),
    (dict(N=100), "null pointer or N % 8 != 0"),
])
def test_gemm_bf16_dropadd_argument_checks(kw, msg):
    _raises(*_dropadd(**kw), msg)


def test_gemm_bf16_dropadd_empty_is_a_no_op():
    for kw in (dict(M=0), dict(N=0), dict(M=0, A=None, B=None, C=None, src=None)):
        _ok(*_dropadd(**kw))


def test_gemm_b16_variant_takes_minus_one_or_zero():
    try:
        for v in (-2, 1, 2, 11, 13, 14, 15, 100):
            _raises("bgnn_gemm_b16_variant", (v,), "must be -1 \\(off\\) or 0")
        _ok("bgnn_gemm_b16_variant", (-1,))
    finally:
        _ok("bgnn_gemm_b16_variant", (0,))


def _elem(name, a=P, b=P, n=64, p=0.1, seed=3, out=P):
    return name, (a, b, n, p, seed, out, None)


ELEM_BAD = [
    (dict(n=-8), "n must be a multiple of 8"), (dict(n=12), "n must be a multiple of 8"), (dict(n=4), "n must be a multiple of 8"),
    (dict(p=1.0), "p must be in \\[0, 1\\)"), (dict(p=-0.5), "p must be in \\[0, 1\\)"),
    (dict(a=None), "16-byte aligned a / b / out required"), (dict(out=None), "16-byte aligned a / b / out required"),
    (dict(a=P + 8), "16-byte aligned a / b / out required"), (dict(out=P + 2), "16-byte aligned a / b / out required"),
    (dict(b=P + 4), "16-byte aligned a / b / out required"),
]


@pytest.mark.parametrize("kw,msg", ELEM_BAD)
def test_add_dropout_bf16_argument_checks(kw, msg):
    _raises(*_elem("bgnn_add_dropout_bf16", **kw), "add_dropout_bf16: " + msg)


@pytest.mark.parametrize("kw,msg", ELEM_BAD + [(dict(b=None), "16-byte aligned a / b / out required")])
def test_add_dropped_bf16_argument_checks(kw, msg):
    _raises(*_elem("bgnn_add_dropped_bf16", **kw), "add_dropped_bf16: " + msg)


def test_elem_bf16_no_elements_is_a_no_op():
    for name in ("bgnn_add_dropout_bf16", "bgnn_add_dropped_bf16"):
        _ok(*_elem(name, n=0))
        _ok(*_elem(name, n=0, a=None, b=None, out=None))


def _seg(name, rowptr=P, col=P, n_rows=10, v=P, ldv=64, H=64, mean=1, out=P, ldo=64):
    return name, (rowptr, col, n_rows, v, ldv, H, mean, out, ldo, None)


SEG_BAD = [
    (dict(rowptr=None), "null pointer"), (dict(col=None), "null pointer"), (dict(v=None), "null pointer"),
    (dict(out=None), "null pointer"), (dict(n_rows=-1), "null pointer or n_rows < 0"),
    (dict(rowptr=None, n_rows=0), "null pointer"),
    (dict(H=0), "H must be a multiple of 8 up to 512"), (dict(H=12), "H must be a multiple of 8 up to 512"),
    (dict(H=520, ldv=520, ldo=520), "H must be a multiple of 8 up to 512"),
    (dict(ldv=56), "H must be a multiple of 8 up to 512"), (dict(ldo=56), "H must be a multiple of 8 up to 512"),
    (dict(v=P + 8), "16-byte aligned"), (dict(out=P + 8), "16-byte aligned"),
]


@pytest.mark.parametrize("kw,msg", SEG_BAD + [(dict(ldv=68), "rows 16-B aligned"), (dict(ldo=66), "rows 16-B aligned"),
                                              (dict(v=P + 2), "16-byte aligned x / out"), (dict(out=P + 4), "16-byte aligned x / out")])
def test_segment_sum_bf16_argument_checks(kw, msg):
    _raises(*_seg("bgnn_segment_sum_bf16", **kw), "segment_sum_bf16: .*" + msg)


@pytest.mark.parametrize("kw,msg", SEG_BAD + [(dict(ldv=66), "rows 16-B aligned"), (dict(ldo=68), "rows 16-B aligned"),
                                              (dict(v=P + 4), "16-byte aligned g / out"), (dict(out=P + 2), "16-byte aligned g / out")])
def test_segment_bcast_bf16_argument_checks(kw, msg):
    _raises(*_seg("bgnn_segment_bcast_bf16", **kw), "segment_bcast_bf16: .*" + msg)


def test_segment_bf16_no_rows_is_a_no_op():
    for name in ("bgnn_segment_sum_bf16", "bgnn_segment_bcast_bf16"):
        _ok(*_seg(name, n_rows=0))
        _ok(*_seg(name, n_rows=0, col=None, v=None, out=None))
