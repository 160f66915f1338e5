"""GPU: the node-level decoder tail on bf16 rows (bgnn_head2_fwd_bf16) and bgnn.fused.node_head_bf16.

The kernel widens each bf16 exactly into the f32 tile bgnn_head2_fwd computes on, so its output has
the bits of bgnn_head2_fwd on x.float(): that is asserted with torch.equal, next to the fp64 bound
tests/test_gpu_node_head.py puts on y (rtol = atol = 1e-5), a strided read beside a NaN plane, and
run-to-run determinism. node_head_bf16 at the h = 512 decoder shape is bounded against a torch
restatement of its rounding points (test_node_head_bf16_h512)."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from bgnn import _lib, fused
from bgnn.graph import _stream

pytestmark = pytest.mark.gpu


def _rows():
    """1, around one tile, 1003, and the N at which one workgroup of the forward's persistent grid
    takes a second tile, with a short final tile."""
    rows, fwd = _lib.query("bgnn_head2_geometry", 0), _lib.query("bgnn_head2_geometry", 1)
    return [1, rows - 1, rows, rows + 1, 1003, rows * fwd + rows + 1]


@functools.lru_cache(maxsize=None)
def _case(D0, C, N):
    """(x bf16 [N, D0] with many exact zeros, W1, b1, W2, b2) on the host, and y in fp64 from the
    same bf16 rows; built once per case."""
    g = torch.Generator().manual_seed(1000 * D0 + 10 * C + N % 997)
    x = torch.randn(N, D0, generator=g).clamp_min(0).bfloat16()
    k1, k2 = D0 ** -0.5, 64 ** -0.5   # nn.Linear's initial ranges
    W1 = (torch.rand(64, D0, generator=g) * 2 - 1) * k1
    b1 = (torch.rand(64, generator=g) * 2 - 1) * k1
    W2 = (torch.rand(C, 64, generator=g) * 2 - 1) * k2
    b2 = (torch.rand(C, generator=g) * 2 - 1) * k2
    y64 = torch.relu(x.double() @ W1.double().t() + b1.double()) @ W2.double().t() + b2.double()
    return x, W1, b1, W2, b2, y64


def _run16(x, W1, b1, W2, b2, y=None):
    """bgnn_head2_fwd_bf16 on the bf16 [N, D0] view x (any row stride)."""
    N, D0 = x.shape
    C = W2.size(0)
    if y is None:
        y = torch.empty(N, C, dtype=torch.float32, device=x.device)
    _lib.call("bgnn_head2_fwd_bf16", x.data_ptr(), x.stride(0), N, D0, 64, C, W1.data_ptr(), b1.data_ptr(),
              W2.data_ptr(), b2.data_ptr(), y.data_ptr(), _stream())
    return y


def _run32(x, W1, b1, W2, b2):
    N, D0 = x.shape
    C = W2.size(0)
    y = torch.empty(N, C, dtype=torch.float32, device=x.device)
    _lib.call("bgnn_head2_fwd", x.data_ptr(), N, D0, 64, C, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
              b2.data_ptr(), y.data_ptr(), _stream())
    return y


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("D0", [64, 128])
def test_kernel_bits_fp64_strided_deterministic(dev, D0, C):
    for N in _rows():
        x, W1, b1, W2, b2, y64 = _case(D0, C, N)
        x, W1, b1, W2, b2 = (t.to(dev) for t in (x, W1, b1, W2, b2))
        y = _run16(x, W1, b1, W2, b2)
        # the bits of the f32 entry on the widened rows
        assert torch.equal(y, _run32(x.float(), W1, b1, W2, b2)), (D0, C, N)
        # fp64 of the same bf16 inputs, at the f32 kernel's forward bound
        err = float((y.double().cpu() - y64).abs().max())
        print(f"D0={D0} C={C} N={N}: max |y - fp64| {err:.3e}")
        torch.testing.assert_close(y.double().cpu(), y64, rtol=1e-5, atol=1e-5)
        # plane 1 of an [N, 2 D0] buffer whose plane 0 is NaN, into a NaN-filled y
        buf = torch.full((N, 2 * D0), float("nan"), dtype=torch.bfloat16, device=dev)
        buf[:, D0:] = x
        ys = _run16(buf[:, D0:], W1, b1, W2, b2, torch.full((N, C), float("nan"), device=dev))
        assert bool(torch.isfinite(ys).all()) and torch.equal(ys, y), (D0, C, N)
        # the same bits on a second run
        assert torch.equal(_run16(x, W1, b1, W2, b2), y), (D0, C, N)


@pytest.mark.parametrize("nb1,nb2", [(1, 0), (0, 1), (1, 1)])
def test_kernel_null_biases(dev, nb1, nb2):
    """b1 / b2 = NULL (zeros, as the header allows): the bits of bgnn_head2_fwd with the same NULLs, and
    of both entries given zero vectors"""
    D0, C, N = 128, 5, _rows()[3]
    x, W1, b1, W2, b2, _ = _case(D0, C, N)
    x, W1, b1, W2, b2 = (t.to(dev) for t in (x, W1, b1, W2, b2))
    z1, z2 = torch.zeros_like(b1), torch.zeros_like(b2)

    def call(name, xx, head, p1, p2):
        y = torch.full((N, C), float("nan"), device=dev)
        _lib.call(name, xx.data_ptr(), *head, N, D0, 64, C, W1.data_ptr(), p1, W2.data_ptr(), p2, y.data_ptr(), _stream())
        return y

    p1, p2 = (None if nb1 else b1.data_ptr()), (None if nb2 else b2.data_ptr())
    q1, q2 = (z1 if nb1 else b1).data_ptr(), (z2 if nb2 else b2).data_ptr()
    y = call("bgnn_head2_fwd_bf16", x, (x.stride(0),), p1, p2)
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, call("bgnn_head2_fwd", x.float(), (), p1, p2))
    assert torch.equal(y, call("bgnn_head2_fwd_bf16", x, (x.stride(0),), q1, q2))
    b1d, b2d = (z1 if nb1 else b1).double().cpu(), (z2 if nb2 else b2).double().cpu()
    y64 = torch.relu(x.double().cpu() @ W1.double().cpu().t() + b1d) @ W2.double().cpu().t() + b2d
    torch.testing.assert_close(y.double().cpu(), y64, rtol=1e-5, atol=1e-5)


def _h512_decoder(dev, C=3):
    torch.manual_seed(5)
    seq = torch.nn.Sequential(torch.nn.Linear(512, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64), torch.nn.ReLU(),
                              torch.nn.Linear(64, C)).to(dev)
    with torch.no_grad():   # a front bias that bf16 holds exactly: torch's bf16 Linear rounds none of it
        seq[0].bias.copy_(seq[0].bias.bfloat16().float())
    return seq


def test_node_head_bf16_h512(dev, monkeypatch):
    """Linear(512,128).ReLU.Linear(128,64).ReLU.Linear(64,3) at N = 1003 against a torch restatement:
    F.linear on the bf16 rows, the bf16 weight and the (bf16-exact) bias with a bf16 output, ReLU,
    widened, then the f32 tail evaluated in fp64.

    Bound. Both sides compute the hidden row as h = bf16(ReLU(s)), s an f32-accumulated sum of the
    same 512 bf16 products (each exact in f32) plus the same bias; the two s differ only by the
    order of accumulation, |s_o - s_t| <= eps = 2 (K - 1) 2^-24 max_row sum_k |x_k| |w_k| (the
    standard bound of a K-term f32 sum, once per side; computed from the data below). Rounding to
    bf16 (nearest) moves a value by at most 2^-9 of itself, ReLU is 1-Lipschitz and commutes with
    the rounding, so |h_o - h_t| <= 2^-9 (|ReLU s_o| + |ReLU s_t|) + eps <= 2^-8 |h_t| (1 + 2^-8) +
    eps (1 + 2^-9). The test asserts eps (1 + 2^-9) + 2^-16 max |h_t| <= 1e-4, which makes that
    dh = 2^-8 |h_t| + 1e-4: one bf16 rounding of the hidden row. The tail is the same f32 function
    on both sides: through Linear(128,64) (|dv| <= |W2| dh), ReLU (1-Lipschitz) and Linear(64,C),
    |dy| <= |W3| (|W2| dh), plus the f32 tail kernel's own bound against fp64, 1e-5 |y| + 1e-5
    (tests/test_gpu_node_head.py)."""
    seq = _h512_decoder(dev)
    g = torch.Generator().manual_seed(12)
    x = (0.1 * torch.randn(1003, 512, generator=g)).clamp_min(0).bfloat16().to(dev)
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a)), orig(name, *a))[1])
    out = fused.node_head_bf16(seq, x)
    assert out is not None and out.dtype == torch.float32 and tuple(out.shape) == (1003, 3)
    assert not out.requires_grad
    names = [c[0] for c in calls]
    assert names.count("bgnn_gemm_bf16") == 1 and names.count("bgnn_head2_fwd_bf16") == 1
    assert "bgnn_head2_fwd" not in names and "bgnn_gemm_f32_scaled" not in names
    gemm = [a for n, a in calls if n == "bgnn_gemm_bf16"][0]
    assert gemm[-4] == 7   # storage: bf16 A, bf16 weight, bf16 output
    with torch.no_grad():
        l0, l1, l2 = seq[0], seq[2], seq[4]
        w16 = l0.weight.bfloat16()
        h_t = torch.relu(F.linear(x, w16, l0.bias.bfloat16()))
        assert h_t.dtype == torch.bfloat16
        h64 = h_t.double()
        y_t = torch.relu(h64 @ l1.weight.double().t() + l1.bias.double()) @ l2.weight.double().t() + l2.bias.double()
        eps = 2 * 511 * 2.0 ** -24 * float((x.double() @ w16.double().abs().t()).max())
        assert eps * (1 + 2.0 ** -9) + 2.0 ** -16 * float(h64.max()) <= 1e-4, eps
        dh = 2.0 ** -8 * h64 + 1e-4
        bound = (dh @ l1.weight.double().abs().t()) @ l2.weight.double().abs().t() + 1e-5 * y_t.abs() + 1e-5
        err = (out.double() - y_t).abs()
    print(f"node_head_bf16 h512: eps {eps:.3e}, max err {float(err.max()):.3e}, "
          f"max err / bound {float((err / bound).max()):.3f}, min bound {float(bound.min()):.3e}")
    assert bool((err <= bound).all()), float((err / bound).max())


def test_front_weight_cache_follows_the_weights(dev):
    seq = _h512_decoder(dev)
    x = torch.randn(64, 512, device=dev).bfloat16()
    fused.node_head_bf16(seq, x)
    w0 = fused.head_front_weight(seq[0])
    assert w0.dtype == torch.bfloat16 and torch.equal(w0, seq[0].weight.detach().bfloat16())
    a = fused.node_head_bf16(seq, x)
    assert fused.head_front_weight(seq[0]) is w0   # the same object on a second call
    with torch.no_grad():
        seq[0].weight.mul_(2.0)
    b = fused.node_head_bf16(seq, x)
    w1 = fused.head_front_weight(seq[0])
    assert w1 is not w0 and torch.equal(w1, seq[0].weight.detach().bfloat16())
    assert not torch.equal(a, b)


def test_two_linears_read_strided_rows_in_place(dev):
    """h = 64 / 128: the tail reads the layer rows where they are (a column plane of a wider
    buffer: the max loop's [agg | x] layout)."""
    for D0 in (64, 128):
        torch.manual_seed(D0)
        seq = torch.nn.Sequential(torch.nn.Linear(D0, 64), torch.nn.ReLU(), torch.nn.Linear(64, 2)).to(dev)
        buf = torch.randn(1003, 2 * D0, device=dev).bfloat16()
        x = buf[:, D0:]
        out = fused.node_head_bf16(seq, x)
        assert out is not None
        assert torch.equal(out, fused.node_head_bf16(seq, x.contiguous()))
        with torch.no_grad():
            assert torch.equal(out, fused.node_head(seq, x.float()))


def test_node_head_bf16_declines(dev):
    lin, relu = torch.nn.Linear, torch.nn.ReLU
    ok = torch.nn.Sequential(lin(128, 64), relu(), lin(64, 3)).to(dev)
    x = torch.randn(40, 128, device=dev).bfloat16()
    assert fused.node_head_bf16(ok, x) is not None
    assert fused.node_head_bf16(ok, x.float()) is None                        # f32 x
    assert fused.node_head_bf16(ok, x.cpu()) is None                          # CPU x
    assert fused.node_head_bf16(torch.nn.Sequential(lin(128, 64), torch.nn.Tanh(), lin(64, 3)).to(dev), x) is None
    assert fused.node_head_bf16(torch.nn.Sequential(lin(128, 64), relu(), lin(64, 3, bias=False)).to(dev), x) is None
    assert fused.node_head_bf16(torch.nn.Sequential(lin(96, 64), relu(), lin(64, 3)).to(dev),
                                torch.randn(40, 96, device=dev).bfloat16()) is None          # D0 = 96
    assert fused.node_head_bf16(torch.nn.Sequential(lin(128, 64), relu(), lin(64, 9)).to(dev), x) is None   # C = 9
    assert fused.node_head_bf16(ok, x[:0]) is None                            # N = 0
    assert fused.node_head_bf16(ok, torch.randn(40, 64, device=dev).bfloat16()) is None      # other width
    assert fused.node_head_bf16(ok, torch.randn(128, 40, device=dev).bfloat16().t()) is None  # column stride
    assert fused.node_head_bf16(ok, torch.randn(40, 132, device=dev).bfloat16()[:, 4:]) is None   # row alignment
    assert fused.node_head_bf16(copy.deepcopy(ok).to(torch.bfloat16), x) is None
    # node_head keeps declining bf16 rows
    assert fused.node_head(ok, x) is None
