"""C-ABI of the dense VALU kernels and the per-module BatchNorm (csrc/mlp.hip, csrc/bn.hip): every
argument check of bgnn_mlp2_fwd / _bwd, bgnn_small_linear_fwd / _bwd, bgnn_linear_bwd_prep_bf16 and
bgnn_bn_stats / _apply / _bwd_stats / _bwd_dx answers BGNN_E_ARG before anything touches a device
(no GPU here: the pointers below are never dereferenced). Among them the 16-byte alignment of every
array a kernel reads or writes in float4: mean / invstd / gamma / sums of bgnn_bn_bwd_dx and h / dh /
ws of bgnn_mlp2_bwd, as their siblings (bn_bwd_stats, head2_bwd, linear_bwd_prep) always required.
(bgnn_head2_*: tests/test_node_head_abi.py.)"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a 16-byte aligned non-NULL "pointer"
ENTRIES = {
    "bgnn_mlp2_supported": ("int", 3), "bgnn_mlp2_fwd": ("int", 12), "bgnn_mlp2_bwd_ws_bytes": ("size_t", 1),
    "bgnn_mlp2_bwd": ("int", 17), "bgnn_small_linear_fwd": ("int", 9), "bgnn_small_linear_bwd": ("int", 11),
    "bgnn_linear_bwd_prep_slots": ("int32_t", 1), "bgnn_linear_bwd_prep_bf16": ("int", 7),
    "bgnn_bn_slots": ("int32_t", 2), "bgnn_bn_stats": ("int", 5), "bgnn_bn_apply": ("int", 7),
    "bgnn_bn_bwd_stats": ("int", 8), "bgnn_bn_bwd_dx": ("int", 10),
}


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, (ret, n_args) in ENTRIES.items():
        decl = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (ret, name), text)
        assert decl, name
        args = decl.group(1).strip()
        assert (0 if args == "void" else len(args.split(","))) == len(_lib.SIGNATURES[name][1]), name
        assert args == "void" or len(args.split(",")) == n_args, name
        assert hasattr(lib, name), name


def test_header_states_the_alignment():
    text = " ".join(open(HEADER).read().split())
    assert "h (both entries), dh and ws (bgnn_mlp2_bwd_ws_bytes(N) bytes) 16-byte aligned" in text.replace(" * ", " ")
    assert "mean, invstd, gamma and sums [2, C] are read in 16-byte vectors" in text.replace(" * ", " ")


def _raises(name, args, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _lib.call(name, *args)
    assert e.value.code == 1001   # BGNN_E_ARG


def _mlp2_fwd(x=P, N=100, F=16, D1=64, D2=128, W1=P, b1=P, W2=P, b2=P, h=P, amax=None):
    return "bgnn_mlp2_fwd", (x, N, F, D1, D2, W1, b1, W2, b2, h, amax, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(F=32), "shape 32x64x128 not built"),
    (dict(D1=128), "shape 16x128x128 not built"),
    (dict(D2=64), "shape 16x64x64 not built"),
    (dict(N=-1), "N < 0"),
    (dict(x=None), "null pointer"),
    (dict(W1=None), "null pointer"),
    (dict(W2=None), "null pointer"),
    (dict(h=None), "null pointer"),
    (dict(h=P + 4), "h must be 16-byte aligned"),
])
def test_mlp2_fwd_argument_checks(kw, msg):
    _raises(*_mlp2_fwd(**kw), msg)


def test_mlp2_no_rows_forward_is_a_no_op():
    from bgnn import _lib

    assert _lib.call(*_mlp2_fwd(N=0)[0:1], *_mlp2_fwd(N=0, x=None, h=None)[1]) == 0


def _mlp2_bwd(x=P, N=100, F=16, D1=64, D2=128, W1=P, b1=P, W2=P, h=P, dh=P, dW1=P, db1=P, dW2=P, db2=P, ws=P,
              ws_bytes=1 << 30):
    return "bgnn_mlp2_bwd", (x, N, F, D1, D2, W1, b1, W2, h, dh, dW1, db1, dW2, db2, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(F=8), "shape 8x64x128 not built"),
    (dict(N=-1), "N < 0"),
    (dict(dW1=None), "null gradient output"),
    (dict(db1=None), "null gradient output"),
    (dict(dW2=None), "null gradient output"),
    (dict(db2=None), "null gradient output"),
    (dict(x=None), "null pointer"),
    (dict(W1=None), "null pointer"),
    (dict(W2=None), "null pointer"),
    (dict(h=None), "null pointer"),
    (dict(dh=None), "null pointer"),
    (dict(h=P + 4), "h and dh must be 16-byte aligned"),
    (dict(dh=P + 8), "h and dh must be 16-byte aligned"),
    (dict(ws=None), "workspace too small"),
    (dict(ws=P + 4), "workspace too small or not 16-byte aligned"),
    (dict(ws=P + 12), "workspace too small or not 16-byte aligned"),
    (dict(ws_bytes=1024), "workspace too small"),
])
def test_mlp2_bwd_argument_checks(kw, msg):
    _raises(*_mlp2_bwd(**kw), msg)


def test_mlp2_workspace():
    from bgnn import _lib

    part = (128 * 64 + 128 + 64 * 16 + 64) * 4   # bytes per slot: [dW2 | db2 | dW1 | db1]
    one = _lib.query("bgnn_mlp2_bwd_ws_bytes", 1)
    assert one % part == 0 and part % 16 == 0
    groups = one // part - 1
    assert groups == 16
    assert _lib.query("bgnn_mlp2_bwd_ws_bytes", 0) == one
    assert _lib.query("bgnn_mlp2_bwd_ws_bytes", 64 * 17) == (17 + groups) * part
    assert _lib.query("bgnn_mlp2_bwd_ws_bytes", 64 * 256 + 65) == _lib.query("bgnn_mlp2_bwd_ws_bytes", 64 * 256) \
        == (256 + groups) * part
    # the last byte short
    _raises(*_mlp2_bwd(N=64 * 17, ws_bytes=(17 + groups) * part - 1), "workspace too small")


def _sl_fwd(x=P, B=3, K=64, W=P, bias=P, N=5, relu=1, y=P):
    return "bgnn_small_linear_fwd", (x, B, K, W, bias, N, relu, y, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(x=None), "bad args"), (dict(W=None), "bad args"), (dict(y=None), "bad args"), (dict(B=-1), "bad args"),
    (dict(K=0), "bad args"), (dict(N=0), "bad args"),
    (dict(K=6), "K % 4 == 0 and 16-B aligned x, W"),
    (dict(x=P + 4), "K % 4 == 0 and 16-B aligned x, W"),
    (dict(W=P + 8), "K % 4 == 0 and 16-B aligned x, W"),
])
def test_small_linear_fwd_argument_checks(kw, msg):
    _raises(*_sl_fwd(**kw), msg)


def test_small_linear_fwd_no_rows_is_a_no_op():
    from bgnn import _lib

    assert _lib.call(*_sl_fwd(B=0)[0:1], *_sl_fwd(B=0)[1]) == 0


def _sl_bwd(gy=P, y=P, x=P, B=3, K=64, W=P, N=5, dx=P, dW=P, db=P):
    return "bgnn_small_linear_bwd", (gy, y, x, B, K, W, N, dx, dW, db, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(gy=None), "bad args"), (dict(x=None), "bad args"), (dict(W=None), "bad args"), (dict(dW=None), "bad args"),
    (dict(B=-1), "bad args"), (dict(K=-4), "bad args"), (dict(N=0), "bad args"),
    (dict(K=10), "K % 4 == 0 and 16-B aligned x, W, dW, dx"),
    (dict(x=P + 4), "16-B aligned x, W, dW, dx"),
    (dict(W=P + 4), "16-B aligned x, W, dW, dx"),
    (dict(dW=P + 8), "16-B aligned x, W, dW, dx"),
    (dict(dx=P + 12), "16-B aligned x, W, dW, dx"),
])
def test_small_linear_bwd_argument_checks(kw, msg):
    _raises(*_sl_bwd(**kw), msg)


def _prep16(g=P, y=P, N=100, C=64, g_out=P, partial=P):
    return "bgnn_linear_bwd_prep_bf16", (g, y, N, C, g_out, partial, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(g=None), "null pointer or negative size"),
    (dict(partial=None), "null pointer or negative size"),
    (dict(N=-1), "null pointer or negative size"),
    (dict(g_out=None), "a ReLU mask needs g_out"),
    (dict(C=4), "C = 4 must be 8 \\* a power of two"),
    (dict(C=12), "C = 12 must be 8"),
    (dict(C=24), "C = 24 must be 8"),
    (dict(C=4096), "C = 4096 must be 8"),
    (dict(g=P + 8), "pointers must be 16-B aligned"),
    (dict(y=P + 2), "pointers must be 16-B aligned"),
    (dict(g_out=P + 4), "pointers must be 16-B aligned"),
    (dict(partial=P + 4), "pointers must be 16-B aligned"),
])
def test_linear_bwd_prep_bf16_argument_checks(kw, msg):
    _raises(*_prep16(**kw), msg)


def test_bn_slots():
    from bgnn import _lib

    assert _lib.query("bgnn_linear_bwd_prep_slots") == 512
    for C, rpi in ((4, 256), (8, 128), (64, 16), (512, 2), (1024, 1)):
        for n, want in ((0, 1), (1, 1), (rpi, 1), (rpi + 1, 2), (1024 * rpi, 1024), (1024 * rpi + 1, 1024)):
            assert _lib.query("bgnn_bn_slots", n, C) == want, (C, n)
    for C in (0, 2, 6, 12, 2048):
        assert _lib.query("bgnn_bn_slots", 10, C) == -1
    assert _lib.query("bgnn_bn_slots", -1, 64) == -1


BAD_C = [(dict(C=0), "C=0 unsupported"), (dict(C=6), "C=6 unsupported"), (dict(C=12), "C=12 unsupported"),
         (dict(C=2048), "C=2048 unsupported")]


def _bn_stats(x=P, n=10, C=64, partial=P):
    return "bgnn_bn_stats", (x, n, C, partial, None)


@pytest.mark.parametrize("kw,msg", BAD_C + [(dict(x=None), "16-byte aligned x / partial"),
                                            (dict(partial=None), "16-byte aligned x / partial"),
                                            (dict(x=P + 4), "16-byte aligned x / partial"),
                                            (dict(partial=P + 8), "16-byte aligned x / partial")])
def test_bn_stats_argument_checks(kw, msg):
    _raises(*_bn_stats(**kw), msg)


def _bn_apply(x=P, n=10, C=64, scale=P, shift=P, y=P):
    return "bgnn_bn_apply", (x, n, C, scale, shift, y, None)


@pytest.mark.parametrize("kw,msg", BAD_C + [(dict(**{k: v}), "16-byte aligned pointers required")
                                            for k in ("x", "scale", "shift", "y") for v in (None, P + 4)])
def test_bn_apply_argument_checks(kw, msg):
    _raises(*_bn_apply(**kw), msg)


def _bn_bwd_stats(g=P, x=P, mean=P, invstd=P, n=10, C=64, partial=P):
    return "bgnn_bn_bwd_stats", (g, x, mean, invstd, n, C, partial, None)


@pytest.mark.parametrize("kw,msg", BAD_C + [(dict(**{k: v}), "16-byte aligned pointers required")
                                            for k in ("g", "x", "mean", "invstd", "partial") for v in (None, P + 4)])
def test_bn_bwd_stats_argument_checks(kw, msg):
    _raises(*_bn_bwd_stats(**kw), msg)


def _bn_bwd_dx(g=P, x=P, mean=P, invstd=P, gamma=P, sums=P, n=10, C=64, dx=P):
    return "bgnn_bn_bwd_dx", (g, x, mean, invstd, gamma, sums, n, C, dx, None)


@pytest.mark.parametrize("kw,msg", BAD_C + [(dict(**{k: None}), "16-byte aligned g / x / dx required")
                                            for k in ("g", "x", "mean", "invstd", "sums", "dx")] + [
    (dict(g=P + 4), "16-byte aligned g / x / dx required"),
    (dict(x=P + 8), "16-byte aligned g / x / dx required"),
    (dict(dx=P + 12), "16-byte aligned g / x / dx required"),
    (dict(mean=P + 4), "16-byte aligned mean / invstd / gamma / sums required"),
    (dict(invstd=P + 8), "16-byte aligned mean / invstd / gamma / sums required"),
    (dict(gamma=P + 4), "16-byte aligned mean / invstd / gamma / sums required"),
    (dict(sums=P + 12), "16-byte aligned mean / invstd / gamma / sums required"),
    (dict(gamma=None, sums=P + 4), "16-byte aligned mean / invstd / gamma / sums required"),
])
def test_bn_bwd_dx_argument_checks(kw, msg):
    _raises(*_bn_bwd_dx(**kw), msg)


def test_bn_no_rows_are_no_ops():
    """no launch without rows (bgnn_bn_bwd_stats launches: its one slot of zeros is a GPU test)"""
    from bgnn import _lib

    for name, args in (_bn_stats(n=0), _bn_apply(n=0), _bn_bwd_dx(n=0), _bn_bwd_dx(n=0, gamma=None)):
        assert _lib.call(name, *args) == 0
