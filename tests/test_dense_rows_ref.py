"""CPU: the references of tests/dense_rows_ref.py are right and their bounds have teeth.

- Every reference and its gradients agree with torch fp64 autograd of the same nn.Sequential /
  BatchNorm1d to 1e-12 relative.
- An f32 host evaluation (plain torch f32, row sums in the slot / group structure the bound describes;
  once in the natural order and once with rows and inner dimensions permuted) stays inside every bound.
- The dyadic hidden layers are bit-equal between f32 and fp64, and hold exact zeros.
- Every mutation leaves the true result by more than 8 x the bound, at the shapes at which
  tests/test_gpu_dense_matrix.py runs the branch it breaks.
- The cycled case lists reach every value of every axis."""
import pytest
import torch

import dense_rows_ref as R
from sage_rows_ref import D, away, ratio

TEETH = 8.0


def close(a, b, what):
    a, b = a.to(D), b.to(D)
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-30), what


def geometry():
    from bgnn import _lib
    return _lib.query("bgnn_head2_geometry", 0), _lib.query("bgnn_head2_geometry", 1), _lib.query("bgnn_head2_geometry", 2)


def enc(N, grid=1, tag=0):
    return R.two_layer_inputs(N, R.MLP_F, R.MLP_D1, R.MLP_D2, grid, tag=tag)


def head(N, D0, C, grid=1):
    T, _fwd, bwd = geometry()
    return R.two_layer_inputs(N, D0, R.HEAD_D1, C, grid, T=T, cap=bwd)


# ----------------------------------------------------------------------------- references vs autograd
def _seq(d, relu_out, b1=True, b2=True):
    W1, W2 = d["W1"], d["W2"]
    l1 = torch.nn.Linear(W1.size(1), W1.size(0), bias=b1).double()
    l2 = torch.nn.Linear(W2.size(1), W2.size(0), bias=b2).double()
    with torch.no_grad():
        l1.weight.copy_(W1)
        l2.weight.copy_(W2)
        if b1:
            l1.bias.copy_(d["b1"])
        if b2:
            l2.bias.copy_(d["b2"])
    mods = [l1, torch.nn.ReLU(), l2] + ([torch.nn.ReLU()] if relu_out else [])
    return torch.nn.Sequential(*mods), l1, l2


@pytest.mark.parametrize("b1,b2", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_mlp2_references_agree_with_autograd(b1, b2):
    d = enc(131)
    seq, l1, l2 = _seq(d, True, b1, b2)
    out = seq(d["x"].double())
    ref, _ = R.mlp2_fwd_ref(d["x"], d["W1"], d["b1"] if b1 else None, d["W2"], d["b2"] if b2 else None)
    close(ref, out.detach(), "h")
    (out * d["g"].double()).sum().backward()
    r = R.mlp2_bwd_ref(d["x"], d["W1"], d["b1"] if b1 else None, d["W2"], out.detach(), d["g"])
    close(r["dW1"][0], l1.weight.grad, "dW1")
    close(r["dW2"][0], l2.weight.grad, "dW2")
    if b1:
        close(r["db1"][0], l1.bias.grad, "db1")
    if b2:
        close(r["db2"][0], l2.bias.grad, "db2")


@pytest.mark.parametrize("D0,C", [(64, 1), (128, 5), (64, 8)])
@pytest.mark.parametrize("b1,b2", [(1, 1), (0, 0)])
def test_head2_references_agree_with_autograd(D0, C, b1, b2):
    T, _f, bwd = geometry()
    d = head(77, D0, C)
    seq, l1, l2 = _seq(d, False, b1, b2)
    x = d["x"].double().requires_grad_(True)
    out = seq(x)
    close(R.head2_fwd_ref(d["x"], d["W1"], d["b1"] if b1 else None, d["W2"], d["b2"] if b2 else None)[0], out.detach(), "y")
    (out * d["g"].double()).sum().backward()
    r = R.head2_bwd_ref(d["x"], d["W1"], d["b1"] if b1 else None, d["W2"], d["g"], T, bwd)
    close(r["dx"][0], x.grad, "dx")
    close(r["dW1"][0], l1.weight.grad, "dW1")
    close(r["dW2"][0], l2.weight.grad, "dW2")
    if b1:
        close(r["db1"][0], l1.bias.grad, "db1")
    if b2:
        close(r["db2"][0], l2.bias.grad, "db2")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("B,K,N", [(3, 252, 65), (200, 64, 3), (1, 4, 1)])
def test_small_linear_references_agree_with_autograd(B, K, N, relu):
    d = R.small_linear_inputs(B, K, N)
    lin = torch.nn.Linear(K, N).double()
    with torch.no_grad():
        lin.weight.copy_(d["W"])
        lin.bias.copy_(d["bias"])
    x = d["x"].double().requires_grad_(True)
    out = torch.relu(lin(x)) if relu else lin(x)
    close(R.small_linear_fwd_ref(d["x"], d["W"], d["bias"], relu)[0], out.detach(), "y")
    (out * d["gy"].double()).sum().backward()
    r = R.small_linear_bwd_ref(d["gy"], out.detach() if relu else None, d["x"], d["W"])
    close(r["dW"][0], lin.weight.grad, "dW")
    close(r["db"][0], lin.bias.grad, "db")
    close(r["dx"][0], x.grad, "dx")


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("affine", [1, 0])
def test_bn_references_agree_with_autograd(kind, affine):
    n, C = 37, 8
    d = R.bn_inputs(n, C, kind)
    bn = torch.nn.BatchNorm1d(C, eps=1e-5, affine=bool(affine)).double().train()
    beta = torch.linspace(-1, 1, C, dtype=D)
    if affine:
        with torch.no_grad():
            bn.weight.copy_(d["gamma"])
            bn.bias.copy_(beta)
    x = d["x"].double().requires_grad_(True)
    y = bn(x)
    (y * d["g"].double()).sum().backward()
    (s0, _), (s1, _) = R.bn_stats_ref(d["x"])
    mean = d["x"][0].double() + s0 / n
    var = s1 / n - (s0 / n) ** 2
    close(mean, d["x"].double().mean(0), "mean from the shifted sums")
    # (the variance is a difference of two sums: compared at the size of its terms)
    assert float((var - d["x"].double().var(0, unbiased=False)).abs().max()) <= 1e-12 * float((s1 / n).max())
    var = d["x"].double().var(0, unbiased=False)
    invstd = 1.0 / (var + 1e-5).sqrt()
    gam = d["gamma"].double() if affine else torch.ones(C, dtype=D)
    scale = gam * invstd
    shift = (beta if affine else 0) - mean * scale
    close(R.bn_apply_ref(d["x"].double(), scale, shift)[0], y.detach(), "y")
    (g0, _), (g1, _) = R.bn_bwd_stats_ref(d["g"], d["x"].double(), mean, invstd)
    if affine:
        close(g0, bn.bias.grad, "dbeta")
        close(g1, bn.weight.grad, "dgamma")
    dx, _ = R.bn_bwd_dx_ref(d["g"], d["x"].double(), mean, invstd, gam if affine else None, torch.stack([g0, g1]))
    assert float((dx - x.grad).abs().max()) <= 1e-11 * float(dx.abs().max())   # (x = 1e3 + ...: x - mean loses 3 digits)


def test_prep_bf16_reference_is_threshold_backward():
    g, y = R.prep_bf16_inputs(257, 16)
    yy = y.clone().requires_grad_(True)
    torch.relu(yy).backward(g)
    go, s, _ = R.prep_bf16_ref(g, y)
    assert go.dtype == torch.bfloat16 and torch.equal(go.view(torch.int16), yy.grad.view(torch.int16))
    close(s, go.double().sum(0), "column sums")
    assert torch.equal(R.prep_bf16_ref(g, None)[0].view(torch.int16), g.view(torch.int16))


# ----------------------------------------------------------------------------- the inputs
def test_dyadic_hidden_layers_are_exact_and_hold_zeros():
    T, _f, bwd = geometry()
    for d in [enc(n) for n in R.MLP_BWD_NS] + [head(n, D0, 5) for n in R.head_ns(T, bwd) for D0 in (64, 128)]:
        x, W1, b1 = d["x"], d["W1"], d["b1"]
        assert R.is_dyadic_hidden(x, W1, b1)
        pre64 = x.double() @ W1.double().t() + b1.double()
        perm = torch.randperm(x.size(1), generator=torch.Generator().manual_seed(1))
        seq = b1.clone().expand(x.size(0), -1).clone()
        for f in perm.tolist():                       # one term at a time, in a permuted order
            seq = seq + x[:, f:f + 1] * W1[:, f].unsqueeze(0)
        for pre32 in (x @ W1.t() + b1, x[:, perm] @ W1[:, perm].t() + b1, seq):
            assert pre32.dtype == torch.float32 and torch.equal(pre32.double(), pre64)
        if d["zero_rows"]:
            z = pre64[d["zero_rows"]]
            assert int((z == 0).sum()) >= 3 * len(d["zero_rows"])
            assert bool((d["g"][d["zero_rows"]].abs() > 0).all())   # non-zero upstream gradients there
    assert not R.is_dyadic_hidden(enc(65, grid=0)["x"], enc(65, grid=0)["W1"], None)


def test_mask_arrays():
    for h in (enc(65)["h"], R.small_linear_inputs(200, 64, 65)["y"], R.prep_bf16_inputs(257, 16)[1].float()):
        z = h == 0
        assert 0.35 < float(z.float().mean()) < 0.65
        assert bool(torch.signbit(h[z]).any()) and not bool(torch.signbit(h[z]).all())   # -0.0 and +0.0
        assert bool((h[~z] >= 0.5).all())            # positive normal numbers, no denormals


def test_case_lists_reach_every_value():
    assert {c[0] for c in R.MLP_FWD_CASES} == set(R.MLP_FWD_NS)
    for k, vals in enumerate(((0, 1, 2, 3), (0, 1), (0, 1, 2), (0, 1))):
        assert {c[1][k] for c in R.MLP_FWD_CASES} == set(vals)
    for k, vals in enumerate(((1, 3, 200), (4, 64, 252, 256, 260, 1024), (1, 3, 64, 65))):
        assert {s[k] for s in R.SL_SHAPES} == set(vals)
    assert {c[1] for c in R.SL_FWD_CASES} == {(1, 0), (1, 1), (0, 0), (0, 1)}
    for k in range(3):
        assert {c[1][k] for c in R.SL_BWD_CASES} == {0, 1}
    assert {c[1] for c in R.HEAD_CASES} == set(range(6)) and {c[2] for c in R.HEAD_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c[0] for c in R.HEAD_CASES} == set(R.HEAD_SHAPES)
    assert {c[0][0] for c in R.BN_CASES} == set(R.BN_CS)
    assert {c[1] for c in R.BN_CASES} == {0, 1} == {c[2] for c in R.BN_CASES}
    assert R.bn_rows_list(1024) == [1, 2, 1025] and R.bn_rows_list(4) == [1, 2, 255, 256, 257, 262145]
    assert R.tile_partition(64 * 17, 64, 256) == (17, 64) and R.tile_partition(64 * 256 + 65, 64, 256) == (256, 128)
    assert R.tile_partition(0, 64, 256) == (1, 0) and R.bn_slots(262145, 4) == (1024, 257, 256)


# ----------------------------------------------------------------------------- f32 host evaluations
def slot_sums_f32(terms, slot, slots):
    """f32 row sums in the structure of the bound: the rows of a slot in sequence, the slots of a group
    in sequence, the 16 groups in sequence"""
    part = torch.zeros((slots,) + terms.shape[1:]).index_add_(0, slot, terms)
    per = -(-slots // R.SUM_GROUPS)
    tmp = torch.zeros((R.SUM_GROUPS,) + terms.shape[1:]).index_add_(0, torch.arange(slots) // per, part)
    s = tmp[0]
    for k in range(1, R.SUM_GROUPS):
        s = s + tmp[k]
    return s


def inside(got, ref_bound, what, f32=True):
    """f32=False: f32 slot sums added in fp64, as the GPU matrix adds the slots it reads"""
    ref, bound = ref_bound
    assert got.dtype == (torch.float32 if f32 else D)
    r = ratio((got.to(D) - ref).abs(), bound)
    assert r <= 1.0, f"{what}: f32 host evaluation at {r:.3f} of the bound"
    return r


def f32_two_layer_bwd(x, W1, b1, W2, g2, T, cap, permute):
    N = x.size(0)
    q = torch.Generator().manual_seed(5)
    rows = torch.randperm(N, generator=q) if permute else torch.arange(N)
    pc = torch.randperm(W2.size(0), generator=q) if permute else torch.arange(W2.size(0))
    pk = torch.randperm(W1.size(0), generator=q) if permute else torch.arange(W1.size(0))
    slots, _ = R.tile_partition(N, T, cap)
    slot = (rows // T) % slots
    x, g2 = x[rows], g2[rows]
    h1 = torch.relu(x @ W1.t() + (b1 if b1 is not None else 0))
    g1 = torch.where(h1 > 0, g2[:, pc] @ W2[pc], torch.zeros(()))
    out = dict(dW2=slot_sums_f32(g2.unsqueeze(2) * h1.unsqueeze(1), slot, slots), db2=slot_sums_f32(g2, slot, slots),
               dW1=slot_sums_f32(g1.unsqueeze(2) * x.unsqueeze(1), slot, slots), db1=slot_sums_f32(g1, slot, slots))
    dx = torch.empty_like(x)
    dx[:] = g1[:, pk] @ W1[pk]
    out["dx"] = torch.empty_like(dx)
    out["dx"][rows] = dx
    return out


@pytest.mark.parametrize("permute", [0, 1])
def test_f32_two_layer_evaluations_stay_inside_the_bounds(permute):
    T, _f, bwd = geometry()
    q = torch.Generator().manual_seed(9)
    worst = {}
    # forward: dyadic and randn-scale inputs
    cases = [(enc(65, g), True) for g in (0, 1)] + [(head(33, D0, 5, g), False) for g in (0, 1) for D0 in (64, 128)]
    for d, relu_out in cases:
        x, W1, b1, W2, b2 = (d[k] for k in ("x", "W1", "b1", "W2", "b2"))
        p0 = torch.randperm(x.size(1), generator=q) if permute else torch.arange(x.size(1))
        p1 = torch.randperm(W1.size(0), generator=q) if permute else torch.arange(W1.size(0))
        h1 = torch.relu(x[:, p0] @ W1[:, p0].t() + b1)
        y = h1[:, p1] @ W2[:, p1].t() + b2
        worst["fwd"] = max(worst.get("fwd", 0), inside(torch.relu(y) if relu_out else y,
                                                      R.two_layer_fwd_ref(x, W1, b1, W2, b2, relu_out), "forward"))
    # backward
    for N in (65, 64 * 17):
        d = enc(N)
        g2 = torch.where(d["h"] > 0, d["g"], torch.zeros(()))
        got = f32_two_layer_bwd(d["x"], d["W1"], d["b1"], d["W2"], g2, R.KT, R.MLP_BLOCKS, permute)
        ref = R.mlp2_bwd_ref(d["x"], d["W1"], d["b1"], d["W2"], d["h"], d["g"])
        for k in ref:
            worst[k] = max(worst.get(k, 0), inside(got[k], ref[k], f"mlp2_bwd N={N} {k}"))
    for N, D0, C in ((33, 128, 5), (T * 17, 64, 8)):
        d = head(N, D0, C)
        got = f32_two_layer_bwd(d["x"], d["W1"], d["b1"], d["W2"], d["g"], T, bwd, permute)
        ref = R.head2_bwd_ref(d["x"], d["W1"], d["b1"], d["W2"], d["g"], T, bwd)
        for k in ref:
            worst[k] = max(worst.get(k, 0), inside(got[k], ref[k], f"head2_bwd N={N} {k}"))
    print("largest f32 err / bound:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("permute", [0, 1])
def test_f32_small_linear_prep_and_bn_stay_inside_the_bounds(permute):
    q = torch.Generator().manual_seed(10)
    for B, K, N in ((3, 252, 65), (200, 1024, 3), (200, 64, 64)):
        d = R.small_linear_inputs(B, K, N)
        pk = torch.randperm(K, generator=q) if permute else torch.arange(K)
        pb = torch.randperm(B, generator=q) if permute else torch.arange(B)
        pn = torch.randperm(N, generator=q) if permute else torch.arange(N)
        x, W, bias, gy, y = (d[k] for k in ("x", "W", "bias", "gy", "y"))
        inside(torch.relu(x[:, pk] @ W[:, pk].t() + bias), R.small_linear_fwd_ref(x, W, bias, 1), "small_linear_fwd")
        g = torch.where(y > 0, gy, torch.zeros(()))
        ref = R.small_linear_bwd_ref(gy, y, x, W)
        dW, db = torch.zeros(N, K), torch.zeros(N)
        for b in pb.tolist():   # one thread adds the B rows in order
            dW = dW + g[b].unsqueeze(1) * x[b].unsqueeze(0)
            db = db + g[b]
        inside(dW, ref["dW"], "small_linear dW")
        inside(db, ref["db"], "small_linear db")
        inside(g[:, pn] @ W[pn], ref["dx"], "small_linear dx")
    for n, C in ((257, 16), (5000, 8)):
        g, y = R.prep_bf16_inputs(n, C)
        go, s, bound = R.prep_bf16_ref(g, y)
        rows = torch.randperm(n, generator=q) if permute else torch.arange(n)
        Rr = R.prep_bf16_rows_per_slot(n, C)
        part = torch.zeros(-(-n // Rr), C).index_add_(0, torch.arange(n) // Rr, go.float()[rows])
        inside(part.double().sum(0), (s, bound), "prep_bf16 column sums", f32=False)
    for (C, n), kind in (((8, 257), 0), ((64, 100), 1), ((4, 1000), 1)):
        d = R.bn_inputs(n, C, kind)
        x, g = d["x"], d["g"]
        slots, rpb, _ = R.bn_slots(n, C)
        rows = torch.randperm(n, generator=q) if permute else torch.arange(n)
        slot = rows // rpb
        dd = x[rows] - x[0]
        a, b = R.bn_stats_ref(x)
        xh = (x[rows] - d["mean"]) * d["invstd"]
        a2, b2 = R.bn_bwd_stats_ref(g, x, d["mean"], d["invstd"])
        for terms, (s, bound), nm in ((dd, a, "sum x - k"), (dd * dd, b, "sum (x - k)^2"), (g[rows], a2, "sum g"),
                                      (g[rows] * xh, b2, "sum g xhat")):
            part = torch.zeros(slots, C).index_add_(0, slot, terms)
            inside(part.double().sum(0), (s, bound), f"bn {nm} C={C} n={n}", f32=False)
        inside(x * d["scale"] + d["shift"], R.bn_apply_ref(x, d["scale"], d["shift"]), "bn_apply")
        ga = d["gamma"] * d["invstd"]
        invn = torch.tensor(1.0) / torch.tensor(float(n))
        xh = (x - d["mean"]) * d["invstd"]
        dx = ga * g - ga * d["sums"][0] * invn - xh * (ga * d["sums"][1] * invn)
        inside(dx, R.bn_bwd_dx_ref(g, x, d["mean"], d["invstd"], d["gamma"], d["sums"]), "bn_bwd_dx")


# ----------------------------------------------------------------------------- mutations
def shows(true, mutated):
    """the largest distance of a mutated result from the true one, in bounds, over the outputs"""
    if not isinstance(true, dict):
        true, mutated = {"": true}, {"": mutated}
    return max(away(mutated[k][0], true[k][0], true[k][1]) for k in true)


def _mlp_bwd(N, nb=0):
    d = enc(N)
    return lambda m=None: R.mlp2_bwd_ref(d["x"], d["W1"], None if nb else d["b1"], d["W2"], d["h"], d["g"], m)


def _mlp_fwd(N, grid):
    d = enc(N, grid)
    return lambda m=None: R.mlp2_fwd_ref(d["x"], d["W1"], d["b1"], d["W2"], d["b2"], m)


def _head_bwd(N, D0, C):
    T, _f, bwd = geometry()
    d = head(N, D0, C)
    return lambda m=None: R.head2_bwd_ref(d["x"], d["W1"], d["b1"], d["W2"], d["g"], T, bwd, m)


def _head_fwd(N, D0, C, grid):
    d = head(N, D0, C, grid)
    return lambda m=None: R.head2_fwd_ref(d["x"], d["W1"], d["b1"], d["W2"], d["b2"], m)


def _sl_fwd(B, K, N):
    d = R.small_linear_inputs(B, K, N)
    return lambda m=None: R.small_linear_fwd_ref(d["x"], d["W"], d["bias"], 0, m)


def _sl_bwd(B, K, N):
    d = R.small_linear_inputs(B, K, N)
    return lambda m=None: R.small_linear_bwd_ref(d["gy"], d["y"], d["x"], d["W"], m)


def _prep(n, C):
    g, y = R.prep_bf16_inputs(n, C)

    def f(m=None):
        go, s, bound = R.prep_bf16_ref(g, y, m)
        return {"sums": (s, bound), "g_out": (go.double(), torch.zeros(n, C, dtype=D))}
    return f


def _bn(C, n, kind, which):
    d = R.bn_inputs(n, C, kind)

    def f(m=None):
        if which == "stats":
            a, b = R.bn_stats_ref(d["x"], m)
        elif which == "bwd_stats":
            a, b = R.bn_bwd_stats_ref(d["g"], d["x"], d["mean"], d["invstd"], m)
        else:
            return R.bn_bwd_dx_ref(d["g"], d["x"], d["mean"], d["invstd"], d["gamma"], d["sums"], m)
        return {"s0": a, "s1": b}
    return f


def mutation_cases():
    T, fwd, bwd = geometry()
    big, hbig = 64 * 256 + 65, T * bwd + T + 1
    out = []
    for N in (1, 63, 65, big):
        out.append(("mlp2_bwd", N, _mlp_bwd, (N,), ("drop_last_row", "mask_ge_h", "no_b1")))
    for N in (65, 64 * 17, big):
        out.append(("mlp2_bwd", N, _mlp_bwd, (N,), ("skip_last_slot", "skip_group_slot", "mask_ge_h1", "w2_last_row")))
    out.append(("mlp2_bwd", big, _mlp_bwd, (big,), ("drop_second_tile_row",)))
    for g in (0, 1):
        out.append(("mlp2_fwd", 65, _mlp_fwd, (65, g), ("no_b1", "no_b2", "w2_last_row")))
    for D0 in (64, 128):
        for C in (1, 2, 4, 5, 7, 8):
            for N in (1, T + 1, T * 17, hbig):
                muts = ("drop_last_row", "no_b1", "w2_last_row") + (("cg4_col",) if C > 4 else ()) + \
                    (("skip_last_slot", "skip_group_slot", "mask_ge_h1") if N > T else ()) + \
                    (("drop_second_tile_row",) if N == hbig else ())
                if N in (T + 1, hbig) or C == 5:
                    out.append(("head2_bwd", (N, D0, C), _head_bwd, (N, D0, C), muts))
            out.append(("head2_fwd", (T + 1, D0, C), _head_fwd, (T + 1, D0, C, C % 2), ("no_b1", "no_b2", "w2_last_row")))
    for B, K, N in R.SL_SHAPES:
        tail = ("lane_tail",) if (K // 4) % 64 else ()
        out.append(("small_linear_fwd", (B, K, N), _sl_fwd, (B, K, N), ("no_bias",) + tail))
        y = R.small_linear_inputs(B, K, N)["y"]   # (B = N = 1: the one element of y is either masked or not)
        out.append(("small_linear_bwd", (B, K, N), _sl_bwd, (B, K, N),
                    (("drop_last_row",) if bool((y[B - 1] > 0).any()) else ()) +
                    (("mask_ge_y",) if bool((y == 0).any()) else ())))
    for (n, C), _y in R.PREP16_CASES[::2]:
        y = R.prep_bf16_inputs(n, C)[1]
        out.append(("prep_bf16", (n, C), _prep, (n, C),
                    (("drop_last_row",) if bool((y[n - 1] > 0).any()) else ()) +
                    (("mask_ge_y",) if bool((y == 0).any()) else ())))
    for (C, n), kind, _g in R.BN_CASES:
        out.append(("bn_stats", (C, n, kind), _bn, (C, n, kind, "stats"),
                    (("unshifted_var", "drop_last_row") if n > 1 else ()) +
                    (("skip_last_slot",) if n > 256 // (C // 4) else ())))
        out.append(("bn_bwd_stats", (C, n, kind), _bn, (C, n, kind, "bwd_stats"),
                    ("drop_last_row",) + (("skip_last_slot",) if n > 256 // (C // 4) else ())))
        # (1 / (n - 1) differs from 1 / n by 1 / n of two of the three terms: it is shown at the smaller shapes)
        out.append(("bn_bwd_dx", (C, n, kind), _bn, (C, n, kind, "dx"),
                    ("sums_swapped",) + (("n_minus_1",) if 1 < n <= 4096 else ())))
    return out


def test_every_mutation_leaves_the_bound():
    seen = set()
    for name, shape, make, args, muts in mutation_cases():
        f = make(*args)
        true = f()
        assert shows(true, f()) == 0.0
        for m in muts:
            assert m in R.MUTATIONS
            far = shows(true, f(m))
            assert far > TEETH, f"{name} {shape}: mutation {m} stays at {far:.2f} bounds"
            seen.add(m)
    # the amax fold (exact values)
    out = torch.tensor([0.5, -2.0])
    big = float(torch.tensor(3.0e30, dtype=torch.float32))
    assert R.amax_ref(3.0e30, out) == big != R.amax_ref(3.0e30, out, "amax_not_accumulated")
    assert R.amax_ref(0.0, out) == 2.0
    seen.add("amax_not_accumulated")
    assert seen == set(R.MUTATIONS), set(R.MUTATIONS) - seen
