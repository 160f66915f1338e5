"""GPU: bf16 mixed-precision training of GraphSage_maxAggr on the fused layer loop
(BuckGNN.sage_bf16 = "all"): aggregate-first, the maximum and its argmax from the f32 rows, the
operands of every N-row product rounded to bf16, the two terms of y = agg W_l^T + x W_r^T stored as
bf16, everything else f32.

The yardstick is, as in tests/test_gpu_sage_bf16_train.py, a torch restatement of autocast's
arithmetic with autograd, run beside the code under test: per layer the f32 first-argmax segment max
of x (oracle.pyg_ref.sage_aggregate), F.linear(agg.bfloat16(), W_l.bfloat16()) and
F.linear(x.bfloat16(), W_r.bfloat16()) with their bf16 outputs, then f32 bias, normalize, BatchNorm,
ReLU and skip. Errors are relative L2 against fp64, and for every quantity
    e_on <= 1.5 * e_torch + e_off
(1.5: the project's margin for bf16 paths, tests/test_gpu_sage_infer.py; e_off: the f32-accurate
path's own error on the same case, measured here).

Argmax flips: from layer 1 on each run's x carries its own rounding error, so a run, the restatement
and fp64 may order two near-equal neighbours differently, and each such place routes one gradient
element to another source. As tests/test_gpu_fullsize.py does, every run's per-layer argmax is
captured (bgnn: a spy on the transform function and ops.max_arg_positions; the restatement: its own
first-argmax edge ids), each disagreement with fp64's first argmax is first checked to be a near tie
-- fp64 margin at most twice the largest |x_run - x_fp64| of that layer's input, a condition, not a
tolerance (_ForcedMax) -- and the fp64 backward is then evaluated along that run's own choices. At
layer level the input is one f32 tensor for every run (f32 -> fp64 is exact), so no flip is possible
and the positions must equal the f32 layer's exactly."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bgnn import _lib, fused, ops
from oracle import buckgnn_ref as R
from oracle import pyg_ref
from test_gpu_fullsize import _ForcedMax
from test_gpu_sage_bf16_train import _trainable, batch_host, rel, run_model, state
from test_gpu_spmm_max_b16 import N_HAND, graph_case

pytestmark = pytest.mark.gpu

NAME = "GraphSage_maxAggr"
TRANSFORMS = ("_max_transform", "_max_transform_bf16")


# ----------------------------------------------------------------------------- argmax capture
def csr_perm(ei):
    """forward-CSR position -> edge id (the CSR is a stable sort of edge_index by target)"""
    return torch.from_numpy(np.argsort(ei[1].numpy(), kind="stable"))


def spy_transforms(mp, ei, seen):
    """Record (function name, layer input x, argmax as edge ids; E: none) of every max transform."""
    perm, E = csr_perm(ei), ei.size(1)
    for fn in TRANSFORMS:
        def spy(x, w_l, w_r, graph, *a, _real=getattr(fused, fn), _fn=fn, **k):
            res = _real(x, w_l, w_r, graph, *a, **k)
            pos = ops.max_arg_positions(graph.fwd, res[2], x.size(0), x.size(1)).cpu()
            seen.append((_fn, x.detach().cpu(), torch.where(pos >= 0, perm[pos.clamp_min(0)], torch.full_like(pos, E))))
            return res
        mp.setattr(fused, fn, spy)


def first_argmax(x, ei):
    """The restatement's choice: per (row, column) the first edge (in edge_index order) that attains
    the row's maximum, as oracle.pyg_ref._ScatterMaxFirst picks it; E for an empty row. On the host."""
    x, E = x.detach().cpu(), ei.size(1)
    src = x.index_select(0, ei[0])
    idx = ei[1].view(-1, 1).expand_as(src)
    out = src.new_zeros(x.shape).scatter_reduce_(0, idx, src, reduce="amax", include_self=False)
    pos = torch.arange(E).view(-1, 1).expand_as(src)
    hit = src == out.index_select(0, ei[1])
    first = torch.full(out.shape, E, dtype=torch.long)
    first.scatter_reduce_(0, idx, torch.where(hit, pos, torch.full_like(pos, E)), reduce="amin", include_self=True)
    return first


def oracle_along(monkeypatch, captures, run):
    """run() -- an fp64 forward + backward on the host -- with the backward of its k-th max
    aggregation forced along captures[k] = (that layer's input as the run under test saw it, its
    argmax edge ids), after _ForcedMax has checked that every disagreement is a near tie.
    Returns (run(), [(flips, largest fp64 margin, allowance)] per layer)."""
    flips, layer = [], [0]

    def forced(x, edge_index, aggr):
        assert aggr == "max"
        xg, eid = captures[layer[0]]
        layer[0] += 1
        tol = 2.0 * float((xg.double() - x.detach()).abs().max())
        return _ForcedMax.apply(x.index_select(0, edge_index[0]), edge_index[1], x.size(0), eid, tol, flips)
    with monkeypatch.context() as mp:
        mp.setattr(pyg_ref, "sage_aggregate", forced)
        mp.setattr(R, "sage_aggregate", forced)
        out = run()
    assert layer[0] == len(captures) == len(flips)
    return out, flips


def check_bound(tag, rows):
    """rows: (quantity, e_on, e_torch, e_off). e_on <= 1.5 * e_torch + e_off for each, after printing."""
    ratio = lambda r: r[1] / (1.5 * r[2] + r[3] + 1e-300)   # noqa: E731
    worst = max(rows, key=ratio)
    print(f"{tag}: {rows[0][0]} on {rows[0][1]:.3e} torch {rows[0][2]:.3e} off {rows[0][3]:.3e}; largest e_on / bound "
          f"{ratio(worst):.3f} at {worst[0]} (on {worst[1]:.3e} torch {worst[2]:.3e} off {worst[3]:.3e})")
    for k, e_on, e_t, e_off in rows:
        assert e_on <= 1.5 * e_t + e_off, (tag, k, e_on, e_t, e_off)


# ----------------------------------------------------------------------------- layer level
@functools.lru_cache(maxsize=None)
def layer_case(H):
    """One layer's input, parameters and output gradient on the host (f32)."""
    g = torch.Generator().manual_seed(100 + H)
    n = N_HAND
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return dict(x=r(n, H), w_l=r(H, H) / H ** 0.5, b_l=0.1 * r(H), w_r=r(H, H) / H ** 0.5, gamma=1.0 + 0.1 * r(H),
                beta=0.1 * r(H), G=r(n, H))


PARAMS = ("x", "w_l", "b_l", "w_r", "gamma", "beta")


def layer_torch(case, ei, skip, bf16):
    """The layer in torch with autograd: fp64 (bf16 False; on the tensors' device in their dtype) or
    autocast's arithmetic on f32 tensors (bf16 True). Returns {x_next, d<param>...}."""
    t = {k: v.clone().requires_grad_(k in PARAMS) for k, v in case.items()}
    x = t["x"]
    agg = pyg_ref.sage_aggregate(x, ei, "max")
    if bf16:
        h = (F.linear(agg.bfloat16(), t["w_l"].bfloat16()).float() + F.linear(x.bfloat16(), t["w_r"].bfloat16()).float()
             + t["b_l"])
    else:
        h = F.linear(agg, t["w_l"], t["b_l"]) + F.linear(x, t["w_r"])
    o = F.batch_norm(F.normalize(h, p=2.0, dim=-1), None, None, t["gamma"], t["beta"], True, 0.1, 1e-5)
    xn = torch.relu(o) + x if skip else torch.relu(o)
    (xn * t["G"]).sum().backward()
    return dict({"x_next": xn.detach()}, **{"d" + k: t[k].grad for k in PARAMS})


def layer_bgnn(dev, case, graph, skip, bf16):
    t = {k: v.to(dev).clone().requires_grad_(k in PARAMS) for k, v in case.items()}
    H = t["x"].size(1)
    bn = torch.nn.BatchNorm1d(H).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(t["gamma"])
        bn.bias.copy_(t["beta"])
    t["gamma"], t["beta"] = bn.weight, bn.bias
    xn = fused.sage_layer(t["x"], t["w_l"], t["b_l"], t["w_r"], bn, graph, 2, skip, 0.0, True, 0, bf16=bf16)
    (xn * t["G"]).sum().backward()
    torch.cuda.synchronize()
    return dict({"x_next": xn.detach()}, **{"d" + k: t[k].grad for k in PARAMS})


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("H", [24, 64, 512])   # (24: 2H % 64 != 0, the forward product's f32-weight storage)
def test_layer_within_autocast_class(dev, monkeypatch, H, skip):
    ei, n, _, graph = graph_case("hand", dev)
    case = layer_case(H)
    seen = []
    with monkeypatch.context() as mp:
        spy_transforms(mp, ei, seen)
        on = layer_bgnn(dev, case, graph, skip, True)
        off = layer_bgnn(dev, case, graph, skip, False)
    assert [s[0] for s in seen] == ["_max_transform_bf16", "_max_transform"]
    assert torch.equal(seen[0][2], seen[1][2])                       # the f32 layer's argmax, exactly
    assert torch.equal(seen[0][2], first_argmax(case["x"], ei))     # which is fp64's: no flip is possible
    tor = layer_torch({k: v.to(dev) for k, v in case.items()}, ei.to(dev), skip, True)
    ref = layer_torch({k: v.double() for k, v in case.items()}, ei, skip, False)
    assert not torch.equal(on["x_next"], off["x_next"])
    rows = [(k, rel(on[k], ref[k]), rel(tor[k], ref[k]), rel(off[k], ref[k])) for k in ref]
    assert all(bool(torch.isfinite(v).all()) for v in on.values())
    check_bound(f"layer H={H} skip={skip}", rows)


def test_layer_refuses_a_folded_transform_and_a_pool(dev):
    H = 64
    _, n, _, graph = graph_case("hand", dev)
    x = torch.zeros(n, H, device=dev)
    w, b = torch.zeros(H, H, device=dev), torch.zeros(H, device=dev)
    with pytest.raises(ValueError, match="no folded input transform"):
        fused.sage_layer(x[:, :16].contiguous(), w, b, w, None, graph, 2, False, 0.0, True, 0,
                         w_in=torch.zeros(H, 16, device=dev), b_in=b, bf16=True)
    with pytest.raises(ValueError, match="fused mean pool is for sum / mean"):
        fused.sage_layer(x, w, b, w, None, graph, 2, False, 0.0, True, 0, pool=object(), bf16=True)
    with pytest.raises(ValueError, match="bf16 needs H % 8 == 0"):
        fused.sage_layer(x[:, :60].contiguous(), w[:60, :60].contiguous(), b[:60].contiguous(),
                         w[:60, :60].contiguous(), None, graph, 2, False, 0.0, True, 0, bf16=True)


# ----------------------------------------------------------------------------- model level
def model_bgnn(dev, monkeypatch, h, flag, super_node=False, training=True):
    """(prediction, gradients, per-layer (x, argmax edge ids)) of one step of the bgnn model."""
    seen = []
    with monkeypatch.context() as mp:
        spy_transforms(mp, batch_host(super_node).edge_index, seen)
        pred, grads = run_model(dev, NAME, h, flag, super_node, training)
    assert [s[0] for s in seen] == [TRANSFORMS[1 if flag == "all" else 0]] * 6
    return pred, grads, [s[1:] for s in seen]


def model_torch(dev, h, super_node=False, training=True, L=6):
    """Autocast's arithmetic, restated in torch with autograd (the module docstring)."""
    hb = batch_host(super_node)
    b = hb.to(dev)
    st = {k: v.to(dev).clone().requires_grad_(_trainable(k, v)) for k, v in state(NAME, h).items()}
    attr, aggr, use_bn = R.SAGE[NAME]
    assert aggr == "max" and use_bn
    x = R._mlp(st, "node_encoder", b.x)
    captures = []
    for i in range(L):
        pre = f"{attr}.{i}"
        captures.append((x.detach().cpu(), first_argmax(x, hb.edge_index)))
        agg = pyg_ref.sage_aggregate(x, b.edge_index, "max")
        zl = F.linear(agg.bfloat16(), st[pre + ".lin_l.weight"].bfloat16())
        zr = F.linear(x.bfloat16(), st[pre + ".lin_r.weight"].bfloat16())
        o = F.normalize(zl.float() + zr.float() + st[pre + ".lin_l.bias"], p=2.0, dim=-1)
        q = f"batch_norms.{i}"
        o = F.batch_norm(o, st[q + ".running_mean"].clone(), st[q + ".running_var"].clone(), st[q + ".weight"],
                         st[q + ".bias"], training, 0.1, 1e-5)
        y = torch.relu(o)
        x = y + x if 0 < i < L - 1 else y
    cnt = torch.bincount(b.batch, minlength=b.num_graphs).clamp_min(1).float().unsqueeze(1)
    pooled = torch.zeros(b.num_graphs, h, device=dev).index_add(0, b.batch, x) / cnt
    pred = R._mlp(st, "decoder", pooled).squeeze()
    R.relative_error_loss(pred, b.y).backward()
    return pred.detach(), {k: v.grad for k, v in st.items() if v.grad is not None}, captures


def model_fp64(h, super_node, training):
    b = batch_host(super_node)
    st = {k: v.double().clone().requires_grad_(_trainable(k, v)) for k, v in state(NAME, h).items()}
    pred = R.forward(st, NAME, b.x.double(), b.edge_index, b.batch, training, "mean", 0.0)
    R.relative_error_loss(pred, b.y.double()).backward()
    return pred.detach(), {k: v.grad for k, v in st.items() if v.grad is not None}


def check_model(dev, monkeypatch, tag, h, super_node=False, training=True):
    runs = {"on": model_bgnn(dev, monkeypatch, h, "all", super_node, training),
            "off": model_bgnn(dev, monkeypatch, h, False, super_node, training),
            "torch": model_torch(dev, h, super_node, training)}
    assert not torch.equal(runs["on"][0], runs["off"][0])   # the flag does something
    # layer 0 reads the f32 encoder's output in both bgnn runs: the same argmax, whatever the mode
    assert torch.equal(runs["on"][2][0][1], runs["off"][2][0][1])
    err = {}
    for name, (pred, grads, captures) in runs.items():
        (p_x, g_x), flips = oracle_along(monkeypatch, captures, lambda: model_fp64(h, super_node, training))
        print(f"{tag}: {name}: argmax flips per layer (count, largest fp64 margin, allowance): {flips}")
        assert set(g_x) <= set(grads) and (name == "torch" or set(g_x) == set(grads))
        assert bool(torch.isfinite(pred).all()) and all(bool(torch.isfinite(grads[k]).all()) for k in g_x)
        err[name] = dict({"prediction": rel(pred, p_x)}, **{k: rel(grads[k], g_x[k]) for k in g_x})
        cat = lambda g: torch.cat([g[k].double().cpu().flatten() for k in sorted(g_x)])   # noqa: E731
        print(f"{tag}: {name}: whole-gradient rel L2 {rel(cat(grads), cat(g_x)):.3e}")
    check_bound(tag, [(k, err["on"][k], err["torch"][k], err["off"][k]) for k in err["on"]])


@pytest.mark.parametrize("h", [64, 512])
def test_training_step_within_autocast_class(dev, monkeypatch, h):
    """Measured (MI355X): h = 64, the largest e_on / bound is 0.78 (batch_norms.2.weight; the
    prediction on 3.27e-3, torch 3.20e-3, off 1.3e-7); h = 512, 0.98, the prediction (on 8.58e-4,
    torch 5.84e-4, off 1.9e-7; whole gradient on 1.42e-2, torch 1.43e-2, off 1.6e-4). The prediction
    is four numbers behind a mean pool over 576 nodes in which the per-node errors cancel to about a
    tenth, so it is the quantity with the least room: a mode that rounded y = [agg | x] [W_l | W_r]^T
    once, where the restatement rounds z_l and z_r and adds them, missed the bound here (9.97e-4,
    1.14 x) with features as accurate as the restatement's, which is why the layer rounds the two
    terms apart."""
    check_model(dev, monkeypatch, f"{NAME} h={h}", h)


def test_training_step_with_super_nodes(dev, monkeypatch):
    """Heavy rows (chunk + combine) in every layer's gather."""
    check_model(dev, monkeypatch, f"{NAME} h=64 super", 64, super_node=True)


def test_eval_mode_with_grad(dev, monkeypatch):
    """eval() with autograd on: BatchNorm's running statistics, no batch sums (bn_partial = NULL)."""
    check_model(dev, monkeypatch, f"{NAME} h=64 eval", 64, training=False)


# ----------------------------------------------------------------------------- plumbing
@pytest.fixture
def lib_calls(monkeypatch):
    calls = []
    real = _lib.call

    def counted(name, *a):
        calls.append((name, a))
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", counted)
    return calls


def test_launches(dev, lib_calls):
    """Under "all" the max model gathers with the pack kernel and takes the bf16 row epilogue, six
    times each, and neither the f32 MAX gather nor the f32 row epilogue. (bgnn_spmm_fwd itself is
    still launched once: the mean pool in front of the decoder, reduce = MEAN.)"""
    def names():
        return [c[0] for c in lib_calls]

    def gathers():   # the reduce argument of every bgnn_spmm_fwd launch
        return [c[1][4] for c in lib_calls if c[0] == "bgnn_spmm_fwd"]
    run_model(dev, NAME, 64, "all", calls=lib_calls)
    assert names().count("bgnn_spmm_max_pack_bf16") == 6 and names().count("bgnn_sage_fwd_bf16") == 6
    assert names().count("bgnn_sage_fwd") == 0 and gathers() == [1]
    for flag in (False, True):   # True keeps its meaning: a max model stays f32
        run_model(dev, NAME, 64, flag, calls=lib_calls)
        assert names().count("bgnn_spmm_max_pack_bf16") == 0 and names().count("bgnn_sage_fwd_bf16") == 0
        assert names().count("bgnn_sage_fwd") == 6 and gathers() == [2] * 6 + [1]
    run_model(dev, "GraphSage_addAggr", 64, "all", calls=lib_calls)
    assert names().count("bgnn_sage_fwd_bf16") == 6 and names().count("bgnn_sage_fwd") == 0
    assert names().count("bgnn_spmm_max_pack_bf16") == 0


def test_all_equals_true_on_a_sum_model(dev):
    """"all" is truthy: a sum model behaves under it exactly as under True."""
    a = run_model(dev, "GraphSage_addAggr", 64, "all", seed=3)
    b = run_model(dev, "GraphSage_addAggr", 64, True, seed=3)
    assert torch.equal(a[0], b[0]) and set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("case", ["h60", "sag", "unfused"])
def test_fallbacks_are_bit_identical(dev, lib_calls, case):
    """Outside the mode (rows that are no whole bf16 vectors, the SAG loops, the per-module path)
    "all" changes nothing: the same train-mode forward bit for bit, and on the fused max layer
    (h = 60) the same gradients."""
    name = "GraphSAGE_SAG" if case == "sag" else NAME
    h = 60 if case == "h60" else 64
    back = case == "h60"
    runs = [run_model(dev, name, h, flag, seed=11, use_fused=case != "unfused", backward=back)
            for flag in (False, "all")]
    called = {c[0] for c in lib_calls}
    assert "bgnn_sage_fwd_bf16" not in called and "bgnn_spmm_max_pack_bf16" not in called
    assert torch.equal(runs[0][0], runs[1][0])
    if back:
        assert runs[0][1] and set(runs[0][1]) == set(runs[1][1])
        for k in runs[0][1]:
            assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_same_seed_same_bits(dev):
    """Two steps from the same state and dropout seed, with super nodes: predictions and all
    gradients equal."""
    a = run_model(dev, NAME, 64, "all", super_node=True, p=0.1, seed=5)
    b = run_model(dev, NAME, 64, "all", super_node=True, p=0.1, seed=5)
    assert torch.equal(a[0], b[0]) and set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
