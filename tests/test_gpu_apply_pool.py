"""GPU: bgnn_sage_apply_pool (the last SAGE layer's apply pass with the segment pool of x_next summed
on the fly, csrc/sage.hip) against the two kernels it replaces, bgnn_sage_apply followed by the
segment reduce of the stored x_next, bit for bit; and bgnn_pool_grad_scale against the torch
expression it replaces.

Segments of 1, 5, 63, 64, 65, 128, 200 and 1100 rows and an empty one in the middle, chunk 64: light
and heavy segments, the chunk boundary from both sides, ragged last chunks, and 18 chunks in one
segment (more than the combine's 16 runs). Once with the rows in segment order (col = identity) and
once with the node order shuffled."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [1, 5, 63, 64, 0, 65, 128, 200, 1100]
N = sum(LENGTHS)
_cache = {}


def _segments(dev, shuffled: bool):
    from bgnn.graph import SegmentIndex

    key = ("seg", shuffled)
    if key not in _cache:
        batch = torch.repeat_interleave(torch.arange(len(LENGTHS)), torch.tensor(LENGTHS))
        if shuffled:
            batch = batch[torch.randperm(N, generator=torch.Generator().manual_seed(5))]
        seg = SegmentIndex.build(batch.to(dev), len(LENGTHS))
        assert seg.fwd.plan.chunk == 64 and seg.fwd.plan.n_heavy == 4 and seg.fwd.plan.n_chunks == 2 + 2 + 4 + 18
        assert shuffled != bool(torch.equal(seg.fwd.col[:N].cpu(), torch.arange(N, dtype=torch.int32)))
        _cache[key] = seg
    return _cache[key]


def _inputs(dev, H: int, bn: bool):
    key = ("in", H, bn)
    if key not in _cache:
        g = torch.Generator().manual_seed(H + bn)
        o = torch.randn(N, H, generator=g)
        o = (o / o.norm(dim=1, keepdim=True)).to(dev)
        x_prev = torch.randn(N, H, generator=g).abs().to(dev)
        scale = (torch.rand(H, generator=g) * 20 + 5).to(dev) if bn else None
        shift = (torch.randn(H, generator=g) * 0.2).to(dev) if bn else None
        _cache[key] = (o, x_prev, scale, shift)
    return _cache[key]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _apply(o, x_prev, scale, shift, skip, p, seed):
    """The reference side: bgnn_sage_apply -> (x_next, max|x_next|)."""
    from bgnn import _lib
    from bgnn.graph import _stream

    x = torch.empty_like(o)
    amax = torch.zeros(1, dtype=torch.float32, device=o.device)
    _lib.call("bgnn_sage_apply", o.data_ptr(), _ptr(scale), _ptr(shift), x_prev.data_ptr(), skip, p, seed, o.size(0),
              o.size(1), x.data_ptr(), amax.data_ptr(), None, None, _stream())
    return x, amax


def _apply_pool(o, x_prev, scale, shift, skip, p, seed, seg, reduce, x_next):
    from bgnn import _lib
    from bgnn.graph import _stream

    H = o.size(1)
    pooled = torch.full((seg.num_rows, H), float("nan"), dtype=torch.float32, device=o.device)
    part = torch.full((seg.fwd.plan.n_chunks * H,), float("nan"), dtype=torch.float32, device=o.device)
    amax = torch.zeros(1, dtype=torch.float32, device=o.device)
    _lib.call("bgnn_sage_apply_pool", o.data_ptr(), _ptr(scale), _ptr(shift), x_prev.data_ptr(), skip, p, seed,
              o.size(0), H, _ptr(x_next), amax.data_ptr(), seg.fwd.ref(), reduce, part.data_ptr(), pooled.data_ptr(),
              _stream())
    return pooled, amax


@pytest.mark.parametrize("shuffled", [False, True], ids=["ordered", "shuffled"])
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("bn", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H", [64, 512])
def test_pool_matches_apply_then_segment_reduce(dev, H, p, bn, skip, shuffled):
    _check(dev, H, p, bn, skip, shuffled)


@pytest.mark.parametrize("H", [640, 1024])
def test_pool_rows_wider_than_two_tiles(dev, H):
    """Rows of 3 and 4 column tiles of 64 float4s: four tiles per block, one of them past the row
    at H = 640."""
    _check(dev, H, 0.1, True, 1, True)


def _check(dev, H, p, bn, skip, shuffled):
    from bgnn.ops import segment_reduce

    seg = _segments(dev, shuffled)
    o, x_prev, scale, shift = _inputs(dev, H, bn)
    seed = 1234567 + H
    x_ref, amax_ref = _apply(o, x_prev, scale, shift, skip, p, seed)
    assert p == 0.0 or 0.05 < float((x_ref == 0).float().mean())   # (the mask is on)
    for reduce, name in ((1, "mean"), (0, "sum")):
        ref = segment_reduce(x_ref, seg, name)
        assert not bool(ref[4].any())   # the empty segment
        # with x_next requested: the same rows, the same maximum, the same pool
        x = torch.full_like(o, float("nan"))
        pooled, amax = _apply_pool(o, x_prev, scale, shift, skip, p, seed, seg, reduce, x)
        assert torch.equal(pooled, ref), name
        assert torch.equal(x, x_ref), name
        assert torch.equal(amax, amax_ref) and float(amax) > 0, name
        # without: the same pool and maximum, and nothing of size [N, H] written (a decoy stays NaN)
        decoy = torch.full_like(o, float("nan"))
        pooled2, amax2 = _apply_pool(o, x_prev, scale, shift, skip, p, seed, seg, reduce, None)
        assert torch.equal(pooled2, ref), name
        assert torch.equal(amax2, amax_ref), name
        assert bool(torch.isnan(decoy).all())
        # run to run
        pooled3, _ = _apply_pool(o, x_prev, scale, shift, skip, p, seed, seg, reduce, None)
        assert torch.equal(pooled3, pooled2), name


@pytest.mark.parametrize("shuffled", [False, True], ids=["ordered", "shuffled"])
@pytest.mark.parametrize("H", [64, 512])
def test_pool_against_fp64(dev, H, shuffled):
    """The mean pool against an fp64 evaluation of relu(o * scale + shift) + x_prev and its segment
    means (no dropout: the mask is the library's own hash). Every term is >= 0, so nothing cancels:
    a segment's f32 sum is a chain of at most 64 adds per chunk plus the combine tree, about
    sqrt(64 / 3) u / sqrt(3) = 1.6e-7 relative (u = 2^-24) at one sigma, under 6e-7 over a row's
    512 columns, and the rounded 1 / count and its product add at most 2 u = 1.2e-7: within 1e-6 of
    the row's largest value."""
    seg = _segments(dev, shuffled)
    o, x_prev, scale, shift = _inputs(dev, H, True)
    pooled, _ = _apply_pool(o, x_prev, scale, shift, 1, 0.0, 1, seg, 1, None)
    x64 = torch.relu(o.double() * scale.double() + shift.double()) + x_prev.double()
    ref = torch.zeros(len(LENGTHS), H, dtype=torch.float64, device=dev).index_add_(0, seg.index, x64)
    ref /= torch.tensor(LENGTHS, dtype=torch.float64, device=dev).clamp_min(1).unsqueeze(1)
    err = (pooled.double() - ref).abs().amax(dim=1)
    bound = 1e-6 * ref.abs().amax(dim=1)
    print("fp64: max relative error per segment", (err / ref.abs().amax(dim=1).clamp_min(1e-300)).tolist())
    assert bool((err <= bound).all())
    assert float(ref.abs().max()) > 0.1


@pytest.mark.parametrize("H", [4, 64, 512])
def test_pool_grad_scale_matches_torch(dev, H):
    """gp = g_pool / max(count, 1): the bits of the torch expression, the empty segment included."""
    from bgnn import _lib
    from bgnn.graph import _stream

    seg = _segments(dev, False)
    g = torch.randn(len(LENGTHS), H, generator=torch.Generator().manual_seed(H)).to(dev)
    ref = g / seg.fwd.degree().clamp_min(1).to(g.dtype).unsqueeze(1)
    out = torch.full_like(g, float("nan"))
    _lib.call("bgnn_pool_grad_scale", g.data_ptr(), seg.fwd.rowptr.data_ptr(), g.size(0), H, out.data_ptr(), _stream())
    assert torch.equal(out, ref)
    assert torch.equal(out[4], g[4])   # count 0 divides by 1
