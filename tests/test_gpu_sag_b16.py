"""GPU: GraphSAGE_SAG on bf16 rows (BuckGNN.infer_bf16_sag).

Kernel level: bgnn_sag_score_bf16 against the formula of include/bgnn.h in fp64 on the same bf16
rows, with the bound that f32 accumulation gives (score_fp64), on the hand-built graph of
tests/test_gpu_sage_infer.py (isolated rows, duplicated edges, in-degree 64 and 65, a row of 11
chunks, a short last row group); bgnn_gather_scale_bf16 bit for bit against torch's own f32 products
and bf16 rounding. Model level: the path against an fp64 restatement of the SAG forward that takes
the path's node selection, with torch's bf16 arithmetic at the same rounding points as the
yardstick; the selection itself against the fp64 scores of the path's own rows, outside the band the
scorer's bound leaves open. Fall-backs: every case outside the path is bit-identical to the flag
being off. Drivers: the bf16_sag keyword."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import bgnn
from bgnn import _lib, fused, pool
from bgnn.data import Batch
from bgnn.graph import Graph
from test_gpu_sage_infer import N_HAND, hand_edges, model_graphs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # f32 unit roundoff
SEED = 80        # the model tests' weight seed, chosen on the CPU (test_selection_follows_the_fp64_scores)


# ----------------------------------------------------------------------------- the scorer in fp64
def score_fp64(xb, w_l, w_r, b, sgn, ei):
    """(score, bound) of include/bgnn.h's formula in fp64 on the bf16 rows xb (CPU tensors).
    bound: f32 accumulation of n terms is off by at most n * 2^-24 of the sum of magnitudes -- a
    row's dot product is H terms (a rounded product, then 7 in-lane adds and the butterfly), the
    neighbour sum deg more, bias and s_r two -- and tanh has slope <= 1 and |tanh| <= 1 (tanhf's own
    error within the 4 ulps of 1 that end the bound):
        |score - score64| <= (H + deg_i + 4) 2^-24 A_i + 4 2^-24,
        A_i = sum_k |x_ik w_r,k| + |b| + sum_e sum_k |x_{col e,k} w_l,k|."""
    x = xb.double()
    n, H = x.shape
    w_l, w_r = w_l.double().view(-1), w_r.double().view(-1)
    b = 0.0 if b is None else float(b)
    src, dst = ei
    attn = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, (x @ w_l)[src]) + b + x @ w_r
    A = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, (x.abs() @ w_l.abs())[src]) + abs(b) + x.abs() @ w_r.abs()
    deg = torch.bincount(dst, minlength=n).double()
    return torch.tanh(sgn * attn), (H + deg + 4) * U * A + 4 * U, attn


@functools.lru_cache(maxsize=None)
def score_inputs(H):
    """bf16 rows [N_HAND, H + 8] (the wide buffer of the ldx > H case; its first H columns are the
    rows), w_l, w_r and the bias; weights small enough that the 700-edge row stays off tanh's
    plateau (asserted in the test)."""
    g = torch.Generator().manual_seed(4000 + H)
    wide = torch.randn(N_HAND, H + 8, generator=g).bfloat16()
    s = 0.05 / math.sqrt(H)
    return wide, s * torch.randn(H, generator=g), s * torch.randn(H, generator=g), torch.tensor([0.1])


@functools.lru_cache(maxsize=None)
def hand_graph():
    return Graph.build(hand_edges().cuda(), N_HAND)


class _Scorer:
    """What pool.sag_score_bf16 reads of SAGPooling's scorer."""

    def __init__(self, w_l, w_r, b):
        self.lin_l = torch.nn.Linear(w_l.numel(), 1, bias=b is not None)
        self.lin_r = torch.nn.Linear(w_l.numel(), 1, bias=False)
        with torch.no_grad():
            self.lin_l.weight.copy_(w_l.view(1, -1))
            self.lin_r.weight.copy_(w_r.view(1, -1))
            if b is not None:
                self.lin_l.bias.copy_(b)
        self.lin_l.cuda()
        self.lin_r.cuda()


def check_score(dev, H, with_bias, sgn, wide):
    g = hand_graph()
    f = g.fwd
    assert f.plan.chunk == 64 and f.plan.n_heavy == 2 and f.plan.n_chunks == 2 + 11
    buf, w_l, w_r, b = score_inputs(H)
    b = b if with_bias else None
    xb = buf[:, :H]
    x_dev = buf.to(dev)[:, :H] if wide else xb.contiguous().to(dev)
    assert x_dev.stride(0) == (H + 8 if wide else H)
    conv = _Scorer(w_l, w_r, b)
    select = torch.tensor([[0.37 * sgn]], device=dev)
    ref, bound, attn = score_fp64(xb, w_l, w_r, b, sgn, hand_edges())
    # the rows the case is about are off tanh's plateau: their errors are not hidden by its slope
    assert float(attn[[10, 11, 500]].abs().max()) < 3.0
    out = pool.sag_score_bf16(x_dev, conv, select, g)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (N_HAND,)
    err = (out.cpu().double() - ref).abs()
    print(f"H={H} bias={with_bias} sgn={sgn} wide={wide}: max err / bound {float((err / bound).max()):.3f}, "
          f"max err {float(err.max()):.3e}, heavy rows {float(err[500]):.2e} / {float(bound[500]):.2e}")
    assert bool(torch.isfinite(out).all())
    assert bool((err <= bound).all()), (int((err > bound).sum()), float((err / bound).max()))
    again = pool.sag_score_bf16(x_dev, conv, select, g)
    assert torch.equal(out, again)


@pytest.mark.parametrize("sgn", [1.0, -1.0])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("H", [8, 72, 512])
def test_score_matches_fp64(dev, H, with_bias, sgn):
    check_score(dev, H, with_bias, sgn, wide=False)


def test_score_on_a_column_view(dev):
    """x a column view of a wider buffer (ldx = H + 8)."""
    check_score(dev, 72, True, 1.0, wide=True)


def test_sign_follows_the_weight(dev):
    """sign(select.weight) is cached per weight version, not per call."""
    buf, w_l, w_r, b = score_inputs(8)
    conv = _Scorer(w_l, w_r, b)
    x = buf[:, :8].contiguous().to(dev)
    w = torch.tensor([[0.5]], device=dev)
    s0 = pool.sag_score_bf16(x, conv, w, hand_graph())
    key = conv._bgnn_sag_sign
    assert torch.equal(pool.sag_score_bf16(x, conv, w, hand_graph()), s0) and conv._bgnn_sag_sign is key
    w.mul_(-1.0)
    s1 = pool.sag_score_bf16(x, conv, w, hand_graph())
    assert conv._bgnn_sag_sign is not key and conv._bgnn_sag_sign[1] == -1.0
    ref = score_fp64(buf[:, :8], w_l, w_r, b, -1.0, hand_edges())
    assert bool(((s1.cpu().double() - ref[0]).abs() <= ref[1]).all())


# ----------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("m", [1.0, 0.5])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("K", [1, N_HAND])
@pytest.mark.parametrize("H", [8, 72, 512])
def test_gather_scale_is_torchs_bits(dev, H, K, wide, m):
    """Two f32 roundings and one bf16 rounding, as torch's own expression: the same bits."""
    g = torch.Generator().manual_seed(5000 + H + K)
    buf = torch.randn(N_HAND, H + 8, generator=g).bfloat16().to(dev)
    x = buf[:, :H] if wide else buf[:, :H].contiguous()
    score = torch.tanh(torch.randn(N_HAND, generator=g)).to(dev)
    perm = (torch.randperm(N_HAND, generator=g) if K == N_HAND else torch.tensor([N_HAND - 1])).to(dev)
    out = pool.gather_scale_bf16(x, score, perm, m)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (K, H)
    ref = ((x.float()[perm] * score[perm, None]) * m).bfloat16()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(out.view(torch.int16), pool.gather_scale_bf16(x, score, perm, m).view(torch.int16))


# ----------------------------------------------------------------------------- model level
def make_model(name, h, L, dev, seed=SEED):
    from recipe import make_weights
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, h, L, "mean", model_name=name)
    sd = model.state_dict()
    w = make_weights({k: tuple(v.shape) for k, v in sd.items()}, seed)   # non-trivial running statistics
    sd = {k: torch.from_numpy(w[k]) if k in w else sd[k] for k in sd}
    model.load_state_dict(sd)
    return (model.to(dev).eval() if dev is not None else model.eval()), sd


def _bn(sd, key, o):
    return F.batch_norm(o, sd[key + ".running_mean"], sd[key + ".running_var"], sd[key + ".weight"], sd[key + ".bias"],
                        False, 0.1, 1e-5)


def _sage_loop(sd, part, n_layers, x, ei, first_skip, bf16, last_f32):
    """One of GraphSAGE_SAG's layer loops (Models/BuckGNN.py:494-501, :505-511; eval: dropout is the
    identity). bf16=False: the oracle's layer arithmetic in x's dtype. bf16=True: the path's
    rounding points in torch -- bf16 x and weights, F.linear with a bf16 output, f32 aggregation and
    tail, the skip from the bf16 x, one bf16 rounding per layer (none on the last with last_f32)."""
    from oracle import buckgnn_ref as R
    src, dst = ei
    for i in range(n_layers):
        pre = f"sage_layers_{part}.{i}"
        if bf16:
            xb = x.bfloat16()
            zl = F.linear(xb, sd[pre + ".lin_l.weight"].bfloat16()).float()
            zr = F.linear(xb, sd[pre + ".lin_r.weight"].bfloat16()).float()
            agg = torch.zeros_like(zl).index_add_(0, dst, zl[src])
            o = F.normalize(agg + zr + sd[pre + ".lin_l.bias"], p=2.0, dim=-1)
            identity = xb.float()
        else:
            o = R.sage_conv(sd, pre, x, ei, "add")
            identity = x
        y = torch.relu(_bn(sd, f"batch_norms_{part}.{i}", o))
        if first_skip or i > 0:
            y = y + identity
        x = y if (not bf16 or (last_f32 and i == n_layers - 1)) else y.bfloat16().float()
    return x


def _score(sd, x, ei, bf16):
    """SAGPooling's score from the rows x: the oracle's expression (aggregate, lin_l + lin_r, the
    select weight), or with bf16 the path's (transform first, the sign of the select weight)."""
    from oracle import pyg_ref as P
    w = sd["pool.select.weight"]
    if not bf16:
        attn = F.linear(P.sage_aggregate(x, ei, "add"), sd["pool.gnn.lin_l.weight"], sd["pool.gnn.lin_l.bias"]) + \
            F.linear(x, sd["pool.gnn.lin_r.weight"])
        return torch.tanh((attn * w).sum(-1) / w.norm(p=2, dim=-1))
    s_l, s_r = x @ sd["pool.gnn.lin_l.weight"].view(-1), x @ sd["pool.gnn.lin_r.weight"].view(-1)
    attn = torch.zeros_like(s_l).index_add_(0, ei[1], s_l[ei[0]]) + sd["pool.gnn.lin_l.bias"] + s_r
    return torch.tanh(torch.sign(w.view(())) * attn)


def sag_forward_given_perm(sd, x, ei, batch, perm, L, bf16):
    """The GraphSAGE_SAG eval forward with mean pooling (oracle.buckgnn_ref.sag_forward) with the
    node selection `perm` given instead of computed. bf16=False: the oracle's arithmetic in x's
    dtype (fp64 in the tests). bf16=True: torch arithmetic with the bf16 path's rounding points."""
    from oracle import buckgnn_ref as R
    n1 = L // 2
    x = R._mlp(sd, "node_encoder", x)
    x = _sage_loop(sd, 1, n1, x, ei, False, bf16, False)
    if bf16:
        x = x.bfloat16().float()   # (an empty loop 1: the encoder's output, rounded once)
    score = _score(sd, x, ei, bf16)
    x = x[perm] * score[perm].view(-1, 1)
    if bf16:
        x = x.bfloat16().float()
    new_id = torch.full((score.numel(),), -1, dtype=torch.long, device=perm.device)
    new_id[perm] = torch.arange(perm.numel(), dtype=torch.long, device=perm.device)
    ei2 = new_id[ei]   # PyG's filter_adj: both ends kept, edge_index order, relabelled
    ei2 = ei2[:, (ei2 >= 0).all(0)]
    batch2 = batch[perm]
    x = _sage_loop(sd, 2, L - n1, x, ei2, True, bf16, True)
    B = int(batch.max()) + 1
    cnt = torch.bincount(batch2, minlength=B).clamp_min(1).to(x.dtype).unsqueeze(1)
    pooled = torch.zeros(B, x.size(1), dtype=x.dtype, device=x.device).index_add_(0, batch2, x) / cnt
    return R._mlp(sd, "decoder", pooled).squeeze()


def rel(a, r):
    return float((a.double().cpu() - r).norm() / r.norm())


def host_batches():
    gs = model_graphs()
    return [Batch.from_data_list(gs[0:4]), Batch.from_data_list(gs[4:6])]


class Spies:
    """What a forward of the path did: sage_infer_layer calls, the libbgnn entry points by name,
    topk_select's perm and the scorer's input rows and output."""

    def __init__(self, monkeypatch):
        self.layers, self.entries, self.perms, self.scored = [], [], [], []
        real_layer, real_call, real_topk, real_score = fused.sage_infer_layer, _lib.call, pool.topk_select, pool.sag_score_bf16

        def layer(*a, **k):
            self.layers.append(1)
            return real_layer(*a, **k)

        def call(name, *a):
            self.entries.append(name)
            return real_call(name, *a)

        def topk(*a, **k):
            out = real_topk(*a, **k)
            self.perms.append(out[0])
            return out

        def score(x, *a, **k):
            out = real_score(x, *a, **k)
            self.scored.append((x.clone(), out.clone()))
            return out
        monkeypatch.setattr(fused, "sage_infer_layer", layer)
        monkeypatch.setattr(_lib, "call", call)
        monkeypatch.setattr(pool, "topk_select", topk)
        monkeypatch.setattr(pool, "sag_score_bf16", score)

    def clear(self):
        for v in (self.layers, self.entries, self.perms, self.scored):
            v.clear()


@pytest.fixture
def spies(monkeypatch):
    return Spies(monkeypatch)


def run_path(model, b):
    model.infer_bf16, model.infer_bf16_sag = True, True
    try:
        with torch.no_grad():
            return model(b.x, b.edge_index, b.edge_attr, b.batch)[0]
    finally:
        model.infer_bf16, model.infer_bf16_sag = False, False


@pytest.mark.parametrize("h,L", [(64, 6), (64, 2), (64, 1), (512, 6)])
def test_model_bf16_close_to_fp64(dev, spies, h, L):
    model, sd = make_model("GraphSAGE_SAG", h, L, dev)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    sdd = {k: v.to(dev) for k, v in sd.items()}
    ref, ours, tor = [], [], []
    for hb in host_batches():
        b = hb.to(dev)
        spies.clear()
        ours.append(run_path(model, b))
        assert len(spies.layers) == L                      # every layer of both loops on the bf16 layer
        assert "bgnn_gather_scale" not in spies.entries    # the f32 gather did not run
        assert spies.entries.count("bgnn_sag_score_bf16") == 1 and spies.entries.count("bgnn_gather_scale_bf16") == 1
        perm = spies.perms[0]
        assert len(spies.perms) == 1 and perm.numel() == int(sum(math.ceil(0.5 * n) for n in torch.bincount(hb.batch)))
        ref.append(sag_forward_given_perm(sd64, hb.x.double(), hb.edge_index, hb.batch, perm.cpu(), L, False))
        tor.append(sag_forward_given_perm(sdd, b.x, b.edge_index, b.batch, perm, L, True))
    ref = torch.cat(ref)
    r_ours, r_torch = rel(torch.cat(ours), ref), rel(torch.cat(tor), ref)
    print(f"GraphSAGE_SAG h={h} L={L}: rel L2 vs the fp64 restatement at the path's selection: bf16 path "
          f"{r_ours:.3e}, torch bf16 {r_torch:.3e}")
    assert bool(torch.isfinite(torch.cat(ours)).all())
    assert r_ours <= 1.5 * r_torch + 1e-4, (r_ours, r_torch)


def band_counts(score64, bound, batch, kept):
    """Per graph: (nodes inside the band around the cut score, nodes outside it whose fp64 side of
    the cut disagrees with `kept`). The cut score is the mean of the last kept and the first
    dropped score in fp64 order; a node is inside the band when its fp64 score is within its own
    scorer bound of the cut. kept: bool [N], or None to count the band only."""
    out = []
    for g in range(int(batch.max()) + 1):
        idx = torch.nonzero(batch == g).flatten()
        s = score64[idx]
        k = int((0.5 * torch.tensor(float(idx.numel()))).ceil())   # PyG: in the score dtype (f32)
        if k >= idx.numel():
            out.append((0, 0 if kept is None else int((~kept[idx]).sum())))
            continue
        top = torch.sort(s, descending=True, stable=True)[0]
        cut = 0.5 * (top[k - 1] + top[k])
        clear = (s - cut).abs() > bound[idx]
        wrong = 0 if kept is None else int(((s > cut) != kept[idx])[clear].sum())
        out.append((int((~clear).sum()), wrong))
    return out


def restated_band_counts(seed, h=64, L=6):
    """The band's node counts per graph from the restatement alone, on the CPU (how SEED was
    chosen): loop 1 with the bf16 rounding points in torch, the fp64 scores of those rows."""
    from oracle import buckgnn_ref as R
    _, sd = make_model("GraphSAGE_SAG", h, L, None, seed)
    counts = []
    for hb in host_batches():
        x = _sage_loop(sd, 1, L // 2, R._mlp(sd, "node_encoder", hb.x), hb.edge_index, False, True, False)
        s64, bound, _ = score_fp64(x.bfloat16(), sd["pool.gnn.lin_l.weight"], sd["pool.gnn.lin_r.weight"],
                                   sd["pool.gnn.lin_l.bias"], float(torch.sign(sd["pool.select.weight"])), hb.edge_index)
        counts += [c for c, _ in band_counts(s64, bound, hb.batch, None)]
    return counts


def test_selection_follows_the_fp64_scores(dev, spies):
    """The path's selection against the fp64 scores of the rows it scored (h = 64, 6 layers): every
    node whose fp64 score is further from its graph's cut score than the scorer's bound is kept or
    dropped as fp64 says; the nodes inside that band are left out, at most 2 per graph. SEED is
    the first weight seed from 77 on for which the restatement alone, on the CPU
    (restated_band_counts), has no node inside the band: 0 in each of the 6 graphs with SEED = 80
    (and 8 to 18 per graph inside a band 100 times as wide, so a node or two may enter on other
    arithmetic; seeds 77 and 78 have 7 to 95 nodes per graph inside the band, seed 79 up to 2).
    On the MI355X the path's own rows give 0 in each graph as well."""
    L, h = 6, 64
    model, sd = make_model("GraphSAGE_SAG", h, L, dev)
    for hb in host_batches():
        b = hb.to(dev)
        spies.clear()
        run_path(model, b)
        (x16, score), perm = spies.scored[0], spies.perms[0].cpu()
        assert x16.dtype == torch.bfloat16 and tuple(x16.shape) == (hb.num_nodes, h)
        s64, bound, _ = score_fp64(x16.cpu(), sd["pool.gnn.lin_l.weight"], sd["pool.gnn.lin_r.weight"],
                                   sd["pool.gnn.lin_l.bias"], float(torch.sign(sd["pool.select.weight"])), hb.edge_index)
        # the scorer inside the model, on the model's graph (super nodes: heavy rows)
        assert bool(((score.cpu().double() - s64).abs() <= bound).all())
        kept = torch.zeros(hb.num_nodes, dtype=torch.bool)
        kept[perm] = True
        counts = band_counts(s64, bound, hb.batch, kept)
        print("nodes inside the band / misplaced outside it, per graph:", counts)
        assert all(c <= 2 for c, _ in counts), counts
        assert all(w == 0 for _, w in counts), counts


# ----------------------------------------------------------------------------- fall-backs
def _fallback_model(case, dev):
    name, h = "GraphSAGE_SAG", 64
    if case == "eagnn_sag":
        name = "EAGNN_SAG"
    elif case == "addaggr":
        name = "GraphSage_addAggr"
    elif case == "h68":
        h = 68
    torch.manual_seed(3)
    model = bgnn.BuckGNN(16, 5, h, 6, "mean", model_name=name).to(dev)
    if case == "bn_no_running_stats":
        model.batch_norms_2[1] = torch.nn.BatchNorm1d(h, track_running_stats=False).to(dev)
    return model.train() if case == "train" else model.eval()


@pytest.mark.parametrize("case", ["flag_off", "infer_bf16_off", "train", "grad", "h68", "bn_no_running_stats",
                                  "eagnn_sag", "addaggr"])
def test_fallbacks_are_bit_identical(dev, spies, case):
    """Outside the path the flag changes nothing: the f32 path's bits and no bf16 layer. (addaggr:
    the model's own bf16 path, with infer_bf16_sag on and off.)"""
    b = Batch.from_data_list(model_graphs()[0:4]).to(dev)
    base = (True, False) if case == "addaggr" else (False, False)
    flagged = {"flag_off": (True, False), "infer_bf16_off": (False, True)}.get(case, (True, True))
    preds, layers = [], []
    for infer, sag in (base, flagged):
        model = _fallback_model(case, dev)   # the same weights both times (seeded)
        model.infer_bf16, model.infer_bf16_sag = infer, sag
        torch.manual_seed(11)   # the train-mode dropout seeds
        spies.clear()
        with torch.set_grad_enabled(case in ("train", "grad")):
            preds.append(model(b.x, b.edge_index, b.edge_attr, b.batch)[0].detach())
        layers.append(len(spies.layers))
        assert "bgnn_sag_score_bf16" not in spies.entries and "bgnn_gather_scale_bf16" not in spies.entries
    assert layers == ([6, 6] if case == "addaggr" else [0, 0])
    assert torch.equal(preds[0], preds[1])


# ----------------------------------------------------------------------------- drivers
def test_drivers_set_and_restore_the_flag(dev, spies):
    model, _ = make_model("GraphSAGE_SAG", 64, 6, dev)
    batches = host_batches()
    ours = torch.cat([run_path(model, hb.to(dev)) for hb in batches])
    scaler = bgnn.EigenvalueScaler(2.0, 0.75)
    spies.clear()
    r = bgnn.evaluate(model, batches, scaler, device=dev, bf16=True, bf16_sag=True)
    assert model.infer_bf16 is False and model.infer_bf16_sag is False
    assert len(spies.layers) == 12
    torch.testing.assert_close(r["predictions"], scaler.denormalize_eigenvalue(ours), rtol=0, atol=0)
    # bf16 alone leaves a SAG model on the f32 path; bf16_sag=None leaves the flag alone
    spies.clear()
    f32 = bgnn.evaluate(model, batches, scaler, device=dev, bf16=True)
    assert not spies.layers and model.infer_bf16_sag is False
    assert torch.equal(f32["predictions"], bgnn.evaluate(model, batches, scaler, device=dev)["predictions"])
    model.infer_bf16_sag = True
    r2 = bgnn.evaluate(model, batches[:1], scaler, device=dev, bf16=True)
    assert model.infer_bf16_sag is True and model.infer_bf16 is False and len(spies.layers) == 6
    assert torch.equal(r2["predictions"], r["predictions"][:batches[0].num_graphs])
    spies.clear()
    bgnn.evaluate(model, batches[:1], scaler, device=dev, bf16=True, bf16_sag=False)
    assert model.infer_bf16_sag is True and not spies.layers
