"""The node-level decoder's tail kernel (bgnn_head2_fwd / _bwd through bgnn.fused.node_head) against
an fp64 torch run of the same nn.Sequential: y, dx and the four parameter gradients, at the bounds
of the sibling kernels' tests (tests/test_gpu_fused.py:259-263, 315-317); the backward is
bit-identical on a second run."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _geometry():
    from bgnn import _lib
    return tuple(_lib.query("bgnn_head2_geometry", i) for i in range(3))


def _rows():
    """1, around one tile, 1000, and one N at which a workgroup of the forward's (and so of the
    backward's smaller) persistent grid takes a second tile, with a ragged last tile."""
    tile, fwd, bwd = _geometry()
    return [1, tile - 1, tile, tile + 1, 1000, tile * max(fwd, bwd) + tile + 1]


def _check(dev, seq, x, spy_tail=True):
    """seq through node_head on x against fp64; returns nothing, asserts."""
    from bgnn import _lib, fused
    calls = []
    orig = _lib.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)

    params = list(seq.parameters())
    _lib.call = spy
    try:
        out = fused.node_head(seq, x)
        assert out is not None
        gy = torch.randn_like(out)
        grads = torch.autograd.grad(out, [x] + params, gy)
        again = torch.autograd.grad(fused.node_head(seq, x), [x] + params, gy)
    finally:
        _lib.call = orig
    assert calls.count("bgnn_head2_fwd") == 2 and calls.count("bgnn_head2_bwd") == 2
    for g, g2 in zip(grads, again):   # deterministic
        assert torch.equal(g, g2)
    seq64 = copy.deepcopy(seq).double()
    x64 = x.detach().double().requires_grad_(True)
    out64 = seq64(x64)
    grads64 = torch.autograd.grad(out64, [x64] + list(seq64.parameters()), gy.double())
    assert out.shape == out64.shape
    torch.testing.assert_close(out.double(), out64, rtol=1e-5, atol=1e-5)
    for g, g64 in zip(grads, grads64):
        assert g.shape == g64.shape
        err = (g.double() - g64).abs().max().item()
        assert err <= 1e-5 * g64.abs().max().item() + 1e-6, (tuple(g.shape), err)


@pytest.mark.parametrize("C", [1, 3, 6, 8])
@pytest.mark.parametrize("D0", [64, 128])
def test_head2_matches_fp64(dev, D0, C):
    """Linear(D0,64).ReLU.Linear(64,C): the whole decoder at h <= 128. Inputs with many exact zeros
    (the ReLU'd layer output the decoder reads)."""
    for N in _rows():
        torch.manual_seed(N + D0 + C)
        seq = torch.nn.Sequential(torch.nn.Linear(D0, 64), torch.nn.ReLU(), torch.nn.Linear(64, C)).to(dev)
        x = torch.randn(N, D0, device=dev).clamp_min(0).requires_grad_(True)
        _check(dev, seq, x)


def test_head2_h512_decoder(dev):
    """Linear(512,128).ReLU.Linear(128,64).ReLU.Linear(64,C): the first Linear on the bgnn GEMM, the
    tail kernel on the rest."""
    torch.manual_seed(5)
    seq = torch.nn.Sequential(torch.nn.Linear(512, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64), torch.nn.ReLU(),
                              torch.nn.Linear(64, 2)).to(dev)
    x = torch.randn(1500, 512, device=dev).clamp_min(0).requires_grad_(True)
    _check(dev, seq, x)


def test_head2_unaligned_rows_and_empty(dev):
    """dy arrives as a non-contiguous view (made contiguous inside); no rows: None (torch modules)."""
    from bgnn import fused
    torch.manual_seed(9)
    seq = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 3)).to(dev)
    x = torch.randn(77, 64, device=dev, requires_grad=True)
    out = fused.node_head(seq, x)
    gy = torch.randn(3, 77, device=dev).t()
    gx, = torch.autograd.grad(out, [x], gy)
    x64 = x.detach().double().requires_grad_(True)
    gx64, = torch.autograd.grad(copy.deepcopy(seq).double()(x64), [x64], gy.double())
    assert (gx.double() - gx64).abs().max().item() <= 1e-5 * gx64.abs().max().item() + 1e-6
    assert fused.node_head(seq, torch.zeros(0, 64, device=dev)) is None


def test_node_head_declines(dev):
    """Shapes and inputs outside the kernel return None (the caller runs the torch modules)."""
    from bgnn import fused
    lin = torch.nn.Linear
    relu = torch.nn.ReLU
    ok = torch.nn.Sequential(lin(128, 64), relu(), lin(64, 3)).to(dev)
    x = torch.randn(40, 128, device=dev)
    assert fused.node_head(ok, x) is not None
    assert fused.node_head(torch.nn.Sequential(lin(96, 64), relu(), lin(64, 3)).to(dev),
                           torch.randn(40, 96, device=dev)) is None
    assert fused.node_head(torch.nn.Sequential(lin(128, 64), relu(), lin(64, 9)).to(dev), x) is None
    assert fused.node_head(torch.nn.Sequential(lin(128, 32), relu(), lin(32, 3)).to(dev), x) is None
    assert fused.node_head(torch.nn.Sequential(lin(128, 64), torch.nn.Tanh(), lin(64, 3)).to(dev), x) is None
    assert fused.node_head(torch.nn.Sequential(lin(128, 64), relu(), lin(64, 3, bias=False)).to(dev), x) is None
    assert fused.node_head(ok, x.to(torch.bfloat16)) is None
    assert fused.node_head(ok, x.cpu()) is None
    assert fused.node_head(copy.deepcopy(ok).to(torch.bfloat16), x) is None
    old = fused.FUSED_NODE_HEAD
    fused.FUSED_NODE_HEAD = False
    try:
        assert fused.node_head(ok, x) is None
    finally:
        fused.FUSED_NODE_HEAD = old


def test_model_with_hooked_decoder_takes_torch(dev):
    """BuckGNN's node-level return: a decoder with a hook runs as a module (the hook fires), without
    one the tail kernel runs from 1024 rows on; both agree."""
    import bgnn
    from bgnn import _lib, synthetic
    torch.manual_seed(2)
    batch = synthetic.make_batch(19, 3, super_node=False).to(dev)
    assert batch.x.size(0) >= 1024
    model = bgnn.BuckGNN(batch.x.size(1), batch.edge_attr.size(1), hidden_channels=64, num_layers=2,
                         prediction_type="static_disp", dropout_rate=0.0,
                         model_name="GraphSage_addAggr").to(dev).eval()
    calls = []
    orig = _lib.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)

    _lib.call = spy
    try:
        with torch.no_grad():
            a, _ = model(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
            n_fused = calls.count("bgnn_head2_fwd")
            seen = []
            h = model.decoder.register_forward_hook(lambda m, i, o: seen.append(o.shape))
            b, _ = model(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
            h.remove()
    finally:
        _lib.call = orig
    assert n_fused == 1 and calls.count("bgnn_head2_fwd") == 1 and len(seen) == 1
    assert a.shape == b.shape == (batch.x.size(0), 2)
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
