"""GPU: the max layer's pack gather (bgnn_spmm_max_pack_bf16): a = [bf16(max agg of x) | bf16(x)] from
f32 rows, with the argmax state of the f32 kernel.

Everything is compared bit for bit, nothing has a tolerance. The yardstick is bgnn_spmm_fwd(MAX) on the
same f32 rows (itself checked against fp64 in tests/test_gpu_spmm_matrix.py): rounding is monotone, so
plane 0 must equal its output rounded to bf16; plane 1 must equal x rounded to bf16; the decoded
argmax positions and the light rows' state bytes must equal the f32 kernel's. Structure cases are
those of tests/test_gpu_spmm_max_b16.py (the hand graph: in-degree 64 / 65 / 700, duplicated edges,
isolated rows, a short last group; a GraphStore batch with 3 super nodes). Inputs:
  randn   plain values
  ties    relu of small integers: ties everywhere, the first edge in CSR order must win
  near    1 + k 2^-20, k < 4096: every value rounds to 1.0 in bf16 and (almost) none tie in f32 --
          a gather over the rounded rows takes each row's first edge, the f32 argmax does not; the
          test first checks that bgnn_spmm_max_bf16 on the rounded rows does disagree
  inf     columns of all -inf and scattered NaN: value -inf, offset 0 (the row's first edge)"""
import functools

import pytest
import torch

from bgnn import ops
from test_gpu_spmm_max_b16 import bits, graph_case

pytestmark = pytest.mark.gpu

HS = [8, 64, 200, 264, 512]   # lanes outside H (8, 64, 200), a row crossing the 256-column half (264, 512)
INF_COLS = (0, 5)


@functools.lru_cache(maxsize=None)
def rows_f32(n, H, inp):
    g = torch.Generator().manual_seed(11 + 7 * H + n)
    if inp == "randn":
        return torch.randn(n, H, generator=g)
    if inp == "ties":
        return torch.relu(torch.randint(-3, 4, (n, H), generator=g).float())
    if inp == "near":
        x = 1.0 + torch.randint(0, 4096, (n, H), generator=g).float() * 2.0 ** -20
        assert bool((x.bfloat16().float() == 1.0).all()) and int(torch.unique(x).numel()) > 2048
        return x
    x = torch.randn(n, H, generator=g)
    x[torch.rand(n, H, generator=g) < 0.05] = float("nan")
    for c in INF_COLS:
        x[:, c] = float("-inf")
    return x


def run_pack(csr, x, n, ldo=None):
    """(buffer [n + 1, ldo] pre-filled with a sentinel, arg) after one launch on the buffer's first n rows."""
    H = x.size(1)
    buf = torch.full((n + 1, ldo or 2 * H), -7.0, dtype=torch.bfloat16, device=x.device)
    out, arg = ops.spmm_max_pack_bf16(csr, x, n, out=buf[:n])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    return buf, arg


def check_against_f32_kernel(csr, x, n, buf, arg):
    H = x.size(1)
    xc = x.contiguous()
    ref_out, ref_arg = ops.spmm_fwd(csr, xc, 2, n, want_arg=True)
    assert torch.equal(bits(buf[:n, :H]), bits(ref_out.bfloat16()))       # plane 0
    assert torch.equal(bits(buf[:n, H:2 * H]), bits(xc.bfloat16()))       # plane 1
    assert bool((buf[:n, 2 * H:] == -7.0).all()) and bool((buf[n] == -7.0).all())   # padding, the row behind
    pos = ops.max_arg_positions(csr, arg, n, H)
    ref_pos = ops.max_arg_positions(csr, ref_arg, n, H)
    assert torch.equal(pos, ref_pos)
    deg = csr.degree()
    light, heavy, empty = (deg > 0) & (deg <= csr.plan.chunk), deg > csr.plan.chunk, deg == 0
    assert int(light.sum()) > 0 and int(heavy.sum()) == csr.plan.n_heavy > 0
    a8, r8 = arg[:n * H].view(n, H), ref_arg[:n * H].view(n, H)
    assert torch.equal(a8[light], r8[light])
    assert bool((a8[heavy] == 255).all()) and bool((a8[empty] == 0).all())
    assert bool((buf[:n, :H][empty] == 0).all())
    # the state contract: every offset in [0, deg)
    rp = csr.rowptr.long()
    off = pos - rp[:-1].view(-1, 1)
    assert bool(((off >= 0) & (off < deg.view(-1, 1)))[~empty].all())
    return ref_out, pos, ref_pos


@pytest.mark.parametrize("inp", ["randn", "ties"])
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("kind", ["hand", "store"])
def test_planes_and_state_equal_the_f32_kernel(dev, kind, H, inp):
    _, n, csr, _ = graph_case(kind, dev)
    x = rows_f32(n, H, inp).to(dev)
    buf, arg = run_pack(csr, x, n)
    check_against_f32_kernel(csr, x, n, buf, arg)


@pytest.mark.parametrize("H", [64, 264, 512])
@pytest.mark.parametrize("kind", ["hand", "store"])
def test_argmax_is_the_f32_one(dev, kind, H):
    """Every neighbour ties after rounding and (almost) none before: the state must be the f32 kernel's,
    which a gather over the rounded rows does not give."""
    _, n, csr, _ = graph_case(kind, dev)
    x = rows_f32(n, H, "near").to(dev)
    _, b16_arg = ops.spmm_max_bf16(csr, x.bfloat16(), n, want_arg=True)
    buf, arg = run_pack(csr, x, n)
    _, pos, ref_pos = check_against_f32_kernel(csr, x, n, buf, arg)
    b16_pos = ops.max_arg_positions(csr, b16_arg, n, H)
    differ = float((b16_pos != ref_pos).float().mean())
    assert differ > 0.1, differ   # the case discriminates: the rounded rows' argmax is another one
    deg = csr.degree()
    assert bool((buf[:n, :H][deg > 0] == 1.0).all())


@pytest.mark.parametrize("H", [8, 200, 512])
@pytest.mark.parametrize("kind", ["hand", "store"])
def test_columns_without_a_winner(dev, kind, H):
    """Columns of all -inf give -inf with offset 0 (the row's first edge), NaN never wins, and the
    state is valid for the backward as it stands."""
    _, n, csr, _ = graph_case(kind, dev)
    x = rows_f32(n, H, "inf").to(dev)
    buf, arg = run_pack(csr, x, n)
    ref_out, pos, _ = check_against_f32_kernel(csr, x, n, buf, arg)
    deg = csr.degree()
    rp = csr.rowptr.long()
    some = deg > 0
    for c in INF_COLS:
        assert bool((buf[:n, c][some] == float("-inf")).all())
        assert torch.equal(pos[:, c][some], rp[:-1][some])
    assert not bool(torch.isnan(buf[:n, :H]).any())
    assert bool(torch.isnan(buf[:n, H:2 * H]).any())


@pytest.mark.parametrize("H", [8, 264, 512])
@pytest.mark.parametrize("kind", ["hand", "store"])
def test_padded_rows_on_both_sides(dev, kind, H):
    """ldx = H + 4 (a multiple of 4, not of 8) and ldo = 2H + 8: the source padding holds values that
    would win every maximum, the destination padding a sentinel that must survive."""
    _, n, csr, _ = graph_case(kind, dev)
    xb = torch.full((n, H + 4), 1e30, device=dev)
    xb[:, :H] = rows_f32(n, H, "randn").to(dev)
    x = xb[:, :H]
    assert x.stride(0) == H + 4
    buf, arg = run_pack(csr, x, n, ldo=2 * H + 8)
    assert buf.stride(0) == 2 * H + 8
    check_against_f32_kernel(csr, x, n, buf, arg)


@pytest.mark.parametrize("kind", ["hand", "store"])
def test_two_launches_give_equal_bits(dev, kind):
    _, n, csr, _ = graph_case(kind, dev)
    x = rows_f32(n, 512, "ties").to(dev)
    a, arg_a = run_pack(csr, x, n)
    b, arg_b = run_pack(csr, x, n)
    assert torch.equal(bits(a), bits(b))
    assert torch.equal(ops.max_arg_positions(csr, arg_a, n, 512), ops.max_arg_positions(csr, arg_b, n, 512))
    m = n * 512
    assert torch.equal(arg_a[:m], arg_b[:m])


def test_wrapper_checks(dev):
    _, n, csr, _ = graph_case("hand", dev)
    x = torch.zeros(n, 64, device=dev)
    with pytest.raises(ValueError, match="x must be float32"):
        ops.spmm_max_pack_bf16(csr, x.bfloat16(), n)
    with pytest.raises(ValueError, match="out must be bfloat16"):
        ops.spmm_max_pack_bf16(csr, x, n, out=torch.zeros(n, 64, dtype=torch.bfloat16, device=dev))
    a, arg = ops.spmm_max_pack_bf16(csr, x, n)
    assert a.shape == (n, 128) and a.dtype == torch.bfloat16 and arg.dtype == torch.uint8
