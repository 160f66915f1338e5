"""GPU: the readout index of a super-node batch (bgnn_readout_index, graph.Readout) and the model
routes on it (buckgnn.FUSED_READOUT): the last fused sum / mean layer pools the 2B segments
[real nodes | super node] per graph inside its apply pass, and every super-node / MLP readout is a
view of that pool. The yardstick throughout is the route without it (FUSED_READOUT = False: mask,
nonzero, gather and a segment pool on the stored rows), bit for bit."""
import glob
import os

import numpy as np
import pytest
import torch

import bgnn
from bgnn import _lib, buckgnn, graph as G, synthetic as S
from bgnn.ops import segment_reduce

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MODES = ("mean_no_super", "supernode_only", "supernode_with_pooling", "mlp_no_super", "mlp")
MODELS = ("GraphSage_addAggr", "GraphSage_meanAggr", "GraphSage_addAggr_Shared")
# real segments of 1 row, exactly chunk = 64 rows (light) and 129 rows (heavy: three chunks, the
# last with one row)
SIZES = (2, 65, 130)


def _index(sizes, dev):
    """(batch vector, ptr) of graphs with these node counts, on the device."""
    n = np.asarray(sizes, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(n)])
    batch = torch.from_numpy(np.repeat(np.arange(n.size), n)).to(dev)
    return batch, torch.from_numpy(ptr).to(dev), n, ptr


def _expected(n, ptr):
    B, N = n.size, int(ptr[-1])
    rowptr2 = np.empty(2 * B + 1, dtype=np.int32)
    rowptr2[0::2], rowptr2[1::2] = ptr, ptr[1:] - 1
    is_super = np.zeros(N, dtype=bool)
    is_super[ptr[1:] - 1] = True
    b = np.repeat(np.arange(B), n)
    real = np.nonzero(~is_super)[0]
    return dict(rowptr2=rowptr2, seg_of_row=2 * b + is_super, real_index=real, real_batch=b[real],
                real_rowptr=(ptr - np.arange(B + 1)).astype(np.int32))


@pytest.fixture
def spy(monkeypatch):
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    return calls


# ------------------------------------------------------------------------------ 1. index kernel
@pytest.mark.parametrize("sizes", [(2,), (65,), (130,), SIZES, (130, 2, 65), (1, 130, 1)],
                         ids=lambda s: "-".join(map(str, s)))
def test_index_kernel_matches_numpy(dev, sizes):
    batch, ptr, n, ptr_h = _index(sizes, dev)
    want = _expected(n, ptr_h)
    runs = []
    for _ in range(2):
        ro = G.build_readout(batch, ptr, n)
        got = dict(rowptr2=ro.seg.fwd.rowptr, seg_of_row=ro.seg.index, real_index=ro.real_index,
                   real_batch=ro.real_batch, real_rowptr=ro.real_seg.fwd.rowptr)
        for k, v in got.items():
            assert v.dtype == (torch.int32 if "rowptr" in k else torch.int64), k
            assert torch.equal(v.cpu(), torch.from_numpy(np.asarray(want[k])).to(v.dtype)), k
        runs.append(got)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    # the structures around the tables: the sizes, the plans from the host counts, the registration
    B, N = n.size, int(ptr_h[-1])
    assert (ro.seg.n, ro.seg.num_rows, ro.seg.fwd.n_rows, ro.seg.fwd.nnz) == (N, 2 * B, 2 * B, N)
    heavy = [int(d) for d in np.diff(want["rowptr2"]) if d > 64]
    assert ro.seg.fwd.plan.n_heavy == len(heavy) and ro.seg.fwd.plan.n_chunks == sum((d + 63) // 64 for d in heavy)
    assert ro.real_seg.fwd.plan.n_heavy == len(heavy) and (ro.real_seg.n, ro.real_seg.num_rows) == (N - B, B)
    if heavy:
        hr = np.nonzero(np.diff(want["rowptr2"]) > 64)[0]
        assert ro.seg.fwd.plan.heavy_row.cpu().tolist() == hr.tolist()
        assert ro.real_seg.fwd.plan.heavy_row.cpu().tolist() == (hr // 2).tolist()
        c0 = np.concatenate([[0], np.cumsum([(d + 63) // 64 for d in heavy])])
        for plan in (ro.seg.fwd.plan, ro.real_seg.fwd.plan):
            assert plan.heavy_chunk0.cpu().tolist() == c0.tolist()
            assert plan.chunk_heavy.cpu().tolist() == np.repeat(np.arange(len(heavy)), np.diff(c0)).tolist()
    assert G.readout_for(batch) is ro
    assert G._index_cache.peek(ro.real_batch, ("batch",)) is ro.real_seg
    assert torch.equal(ro.seg.bwd.col[:N].cpu(), torch.from_numpy(want["seg_of_row"]).int())


def test_register_readout_reads_ptr_once_per_batch(dev, spy):
    batch, ptr, n, _ = _index(SIZES, dev)
    ro = bgnn.register_readout(batch, ptr)
    assert bgnn.register_readout(batch, ptr) is ro is bgnn.readout_for(batch)
    assert spy.count("bgnn_readout_index") == 1
    assert bgnn.readout_for(batch.clone()) is None and bgnn.readout_for(None) is None
    with pytest.raises(ValueError, match="at least its super node"):
        G.build_readout(batch, ptr, [2, 0, 195])


def test_store_batch_carries_the_same_index(dev, spy):
    """GraphStore.batch (plans inside its one upload, cached arange) against build_readout on the
    same counts: the same tables and the same plans, from one bgnn_readout_index launch."""
    graphs = [S.make_mesh_graph(n, 10 + i, super_node=True) for i, n in enumerate((12, 5, 9))]
    store = bgnn.GraphStore(graphs, device=dev)
    assert store.super_nodes
    del spy[:]
    b = store.batch([2, 0, 1])
    # (bgnn_heavy_plan twice: the graph's two CSRs, whose super-node rows are heavy; none for the segments)
    assert spy.count("bgnn_readout_index") == 1 and spy.count("bgnn_heavy_plan") == 2
    assert "bgnn_index_csr_build" not in spy
    ro = bgnn.readout_for(b.batch)
    n = np.array([82, 145, 26])
    assert torch.equal(b.ptr.cpu(), torch.from_numpy(np.concatenate([[0], np.cumsum(n)])))
    want = G.build_readout(b.batch.clone(), b.ptr, n)
    for got_s, want_s in ((ro.seg, want.seg), (ro.real_seg, want.real_seg)):
        assert (got_s.n, got_s.num_rows) == (want_s.n, want_s.num_rows)
        assert torch.equal(got_s.fwd.rowptr, want_s.fwd.rowptr) and torch.equal(got_s.index, want_s.index)
        assert torch.equal(got_s.fwd.col[:got_s.n], want_s.fwd.col[:got_s.n])
        assert torch.equal(got_s.bwd.col[:got_s.n], want_s.bwd.col[:got_s.n])
        gp, wp = got_s.fwd.plan, want_s.fwd.plan
        assert (gp.n_heavy, gp.n_chunks, gp.chunk) == (wp.n_heavy, wp.n_chunks, wp.chunk) == (2, 5, 64)
        for k in ("heavy_row", "heavy_chunk0", "chunk_heavy"):
            assert torch.equal(getattr(gp, k), getattr(wp, k)), k
    assert torch.equal(ro.real_index, want.real_index) and torch.equal(ro.real_batch, want.real_batch)
    assert G._index_cache.peek(ro.real_batch, ("batch",)) is ro.real_seg


# ------------------------------------------------------------------------------ 2. pool pass
@pytest.fixture(scope="module")
def pool_case(dev):
    batch, ptr, n, ptr_h = _index(SIZES, dev)
    ro = G.build_readout(batch, ptr, n)
    sup = torch.from_numpy(ptr_h[1:] - 1).to(dev)
    return ro, sup, int(ptr_h[-1])


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("H", [64, 200, 512])
def test_pool_pass_on_the_readout_index(dev, pool_case, H, skip, p, bn):
    """bgnn_sage_apply_pool over the 2B-segment CSR (singleton and light segments beside a heavy
    one) against bgnn_sage_apply, then index_select / segment_reduce on the stored rows."""
    ro, sup, N = pool_case
    g = torch.Generator(device="cpu").manual_seed(H + 2 * skip + int(10 * p) + 7 * bn)
    o = torch.randn(N, H, generator=g).to(dev)
    x_prev = torch.randn(N, H, generator=g).to(dev)
    scale = (torch.rand(H, generator=g) + 0.5).to(dev) if bn else None
    shift = torch.randn(H, generator=g).to(dev) if bn else None
    s = torch.cuda.current_stream().cuda_stream
    pt = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    x_ref = torch.empty(N, H, device=dev)
    amax_ref = torch.zeros(1, device=dev)
    _lib.call("bgnn_sage_apply", o.data_ptr(), pt(scale), pt(shift), x_prev.data_ptr(), skip, p, 1234, N, H,
              x_ref.data_ptr(), amax_ref.data_ptr(), None, None, s)
    want = torch.empty(2 * sup.numel(), H, device=dev)
    want[0::2] = segment_reduce(x_ref.index_select(0, ro.real_index), ro.real_seg, "mean")
    want[1::2] = x_ref.index_select(0, sup)
    nch = ro.seg.fwd.plan.n_chunks
    assert nch == 3
    for need_x in (True, False):
        part = torch.empty(nch * H, device=dev)
        pooled = torch.full((2 * sup.numel(), H), float("nan"), device=dev)
        x_next = torch.empty(N, H, device=dev) if need_x else None
        amax = torch.zeros(1, device=dev) if need_x else None
        _lib.call("bgnn_sage_apply_pool", o.data_ptr(), pt(scale), pt(shift), x_prev.data_ptr(), skip, p, 1234, N, H,
                  pt(x_next), pt(amax), ro.seg.fwd.ref(), 1, part.data_ptr(), pooled.data_ptr(), s)
        assert torch.equal(pooled, want)
        if need_x:
            assert torch.equal(x_next, x_ref) and torch.equal(amax, amax_ref)


def test_pool_pass_with_an_empty_real_segment(dev):
    """A graph that is only its super node: an empty real segment, whose mean is 0."""
    batch, ptr, n, ptr_h = _index((1, 130, 1), dev)
    ro = G.build_readout(batch, ptr, n)
    N, H = int(ptr_h[-1]), 64
    o = torch.randn(N, H, generator=torch.Generator().manual_seed(3)).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    x_ref = torch.empty(N, H, device=dev)
    amax = torch.zeros(1, device=dev)
    _lib.call("bgnn_sage_apply", o.data_ptr(), None, None, o.data_ptr(), 0, 0.0, 1, N, H, x_ref.data_ptr(),
              amax.data_ptr(), None, None, s)
    part = torch.empty(ro.seg.fwd.plan.n_chunks * H, device=dev)
    pooled = torch.full((6, H), float("nan"), device=dev)
    _lib.call("bgnn_sage_apply_pool", o.data_ptr(), None, None, o.data_ptr(), 0, 0.0, 1, N, H, None, None,
              ro.seg.fwd.ref(), 1, part.data_ptr(), pooled.data_ptr(), s)
    want = torch.empty(6, H, device=dev)
    want[0::2] = segment_reduce(x_ref.index_select(0, ro.real_index), ro.real_seg, "mean")
    want[1::2] = x_ref[torch.tensor([0, 130, 131], device=dev)]
    assert torch.equal(pooled, want)
    assert not pooled[0].any() and not pooled[4].any() and bool(pooled[2].any())


# ------------------------------------------------------------------------------ 3. model parity
def _store(dev, ns, super_node=True, y_nodes=0):
    graphs = [S.make_mesh_graph(n, 10 + i, super_node=super_node) for i, n in enumerate(ns)]
    if y_nodes:   # node-level targets: one row per real node
        for i, d in enumerate(graphs):
            d.y = torch.randn(d.num_nodes - (1 if super_node else 0), y_nodes,
                              generator=torch.Generator().manual_seed(50 + i))
    return bgnn.GraphStore(graphs, device=dev)


def _model(name, mode, h, dev, L=3, ptype="buckling"):
    torch.manual_seed(0)
    m = bgnn.BuckGNN(16, 5, hidden_channels=h, num_layers=L, pooling_layer=mode, prediction_type=ptype,
                     dropout_rate=0.1, model_name=name).to(dev)
    return m, {k: v.clone() for k, v in m.state_dict().items()}


def _run(model, sd, b, train, on, monkeypatch, crit=None):
    """One forward (+ backward in train mode) from the state sd under torch.manual_seed: the
    prediction, every parameter gradient and the buffers afterwards."""
    monkeypatch.setattr(buckgnn, "FUSED_READOUT", on)
    model.load_state_dict(sd)
    model.train(train)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(7)
    if not train:
        with torch.no_grad():
            pred, ob = model(b.x, b.edge_index, b.edge_attr, b.batch)
        return pred.clone(), ob, {}, {}
    pred, ob = model(b.x, b.edge_index, b.edge_attr, b.batch)
    loss = bgnn.RelativeErrorLoss()(pred, b.y) if crit is None else crit(pred, b.y, ob, None)
    loss.backward()
    grads = {k: None if p.grad is None else p.grad.clone() for k, p in model.named_parameters()}
    return pred.detach().clone(), ob, grads, {k: v.clone() for k, v in model.named_buffers()}


def _assert_same(a, b):
    assert a[0].shape == b[0].shape and torch.equal(a[0], b[0]), "prediction"
    assert torch.equal(a[1], b[1]), "returned batch vector"
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert (a[2][k] is None) == (b[2][k] is None), k
        assert a[2][k] is None or torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.fixture(scope="module")
def small_store(dev):
    return _store(dev, (5, 7, 12))   # 26, 50 and 145 nodes: the last real segment is heavy


@pytest.fixture
def small_batch(small_store):
    """A fresh batch per test: its readout index lives in the identity cache of the batch vector."""
    return small_store, small_store.batch([0, 1, 2])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", MODELS)
def test_model_equals_the_route_without_the_readout(dev, monkeypatch, spy, small_batch, name, mode):
    _, b = small_batch
    assert (bgnn.readout_for(b.batch) is not None)
    model, sd = _model(name, mode, 64, dev)
    for train in (True, False):
        del spy[:]
        on = _run(model, sd, b, train, True, monkeypatch)
        assert spy.count("bgnn_sage_apply_pool") == 1 and spy.count("bgnn_index_csr_build") == 0, spy
        del spy[:]
        off = _run(model, sd, b, train, False, monkeypatch)
        assert spy.count("bgnn_sage_apply_pool") == 0
        _assert_same(on, off)
    assert any(g is not None for g in on[2].values()) or not on[2]


@pytest.mark.parametrize("mode", MODES)
def test_model_equals_the_route_without_the_readout_h512(dev, monkeypatch, spy, mode):
    """Two n = 24 meshes (1,154 rows) at h = 512: the fused, folded encoder in front."""
    store = _store(dev, (24, 24))
    b = store.batch([0, 1])
    assert b.x.size(0) >= 1024
    model, sd = _model("GraphSage_addAggr", mode, 512, dev)
    for train in (True, False):
        del spy[:]
        on = _run(model, sd, b, train, True, monkeypatch)
        assert spy.count("bgnn_sage_apply_pool") == 1
        off = _run(model, sd, b, train, False, monkeypatch)
        _assert_same(on, off)


def test_node_head_equals_the_route_without_the_readout(dev, monkeypatch):
    """static_stress with a super-node pooling: the real nodes by index_select on the readout index
    and the cached real-node batch vector, against the boolean-mask filter."""
    store = _store(dev, (5, 7, 12), y_nodes=3)
    b = store.batch([0, 1, 2])
    ro = bgnn.readout_for(b.batch)
    model, sd = _model("GraphSage_addAggr", "supernode_only", 64, dev, ptype="static_stress")
    crit = bgnn.GraphRelativeError()
    for train in (True, False):
        on = _run(model, sd, b, train, True, monkeypatch, crit)
        assert on[1] is ro.real_batch
        off = _run(model, sd, b, train, False, monkeypatch, crit)
        assert off[1] is not ro.real_batch
        _assert_same(on, off)


# ------------------------------------------------------------------------------ 4. launch record
def _step_models(dev):
    """(model, criterion, batch) of every route: the five buckling readouts and a static_stress
    super-node model, each on a fresh store batch."""
    out = []
    store = _store(dev, (5, 7, 12))
    for mode in MODES:
        m, _ = _model("GraphSage_addAggr", mode, 64, dev)
        out.append((mode, m, bgnn.RelativeErrorLoss(), store))
    m, _ = _model("GraphSage_addAggr", "supernode_only", 64, dev, ptype="static_stress")
    out.append(("static_stress", m, bgnn.GraphRelativeError(), _store(dev, (5, 7, 12), y_nodes=3)))
    return out


def test_launch_record_of_a_train_step(dev, spy):
    """One bgnn.train_step on a store batch: the last layer pools in its apply pass (the node-level
    head has no pool: L plain apply passes), and nothing sorts or builds a graph structure."""
    L = 3
    for tag, model, crit, store in _step_models(dev):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        model.train()
        b = store.batch([0, 1, 2])
        del spy[:]
        bgnn.train_step(model, b, opt, crit)
        torch.cuda.synchronize()
        pools = 0 if tag == "static_stress" else 1
        assert spy.count("bgnn_sage_apply_pool") == pools, (tag, spy)
        assert spy.count("bgnn_sage_apply") == L - pools, (tag, spy)
        assert "bgnn_index_csr_build" not in spy and "bgnn_graph_build" not in spy, (tag, spy)


# ------------------------------------------------------------------------------ 5. no host sync
def test_a_train_step_does_not_synchronise(dev):
    prev = torch.cuda.get_sync_debug_mode()
    probe = torch.ones(1, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raised = False
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this build")
    for tag, model, crit, store in _step_models(dev):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        model.train()
        bgnn.train_step(model, store.batch([0, 1, 2]), opt, crit)   # (lazy initialisations, outside the check)
        b = store.batch([2, 0, 1])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = bgnn.train_step(model, b, opt, crit, sync_metrics=False)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        assert bool(torch.isfinite(loss)), tag


# ------------------------------------------------------------------------------ 6. goldens
def _ptr_of(batch_h):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(batch_h))]))


@pytest.mark.parametrize("case", ["add_super_nosuper_h64", "add_super_only_h64", "add_super_withpool_h64"])
def test_buckling_goldens_through_register_readout(dev, spy, case):
    """The reference's own vectors (tests/test_gpu_model.py and its tolerances) on the readout route."""
    from recipe import meta_from_array
    from test_gpu_model import build
    z = np.load(os.path.join(GOLDEN, case + ".npz"))
    meta = meta_from_array(z["meta"])
    model = build(meta, dev, True)
    captured = {}
    model.decoder.register_forward_pre_hook(lambda mod, inp: captured.__setitem__("pooled", inp[0].detach()))
    x, ei, ea, batch = (torch.from_numpy(z[k]).to(dev) for k in ("x", "edge_index", "edge_attr", "batch"))
    y = torch.from_numpy(z["y"]).to(dev)
    bgnn.register_readout(batch, _ptr_of(z["batch"]).to(dev))
    model.train()
    pred, _ = model(x, ei, ea, batch)
    assert spy.count("bgnn_sage_apply_pool") == 1
    loss = bgnn.RelativeErrorLoss()(pred, y)
    loss.backward()
    tol = dict(rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(pred.detach().cpu().numpy().reshape(-1), z["pred_train"], **tol)
    np.testing.assert_allclose(loss.item(), float(z["loss_train"]), **tol)
    np.testing.assert_allclose(captured["pooled"].cpu().numpy(), z["pooled_train"], **tol)
    params = dict(model.named_parameters())
    n_grads = 0
    for k in z.files:
        if k.startswith("grad/"):
            assert params[k[5:]].grad is not None, k
            np.testing.assert_allclose(params[k[5:]].grad.cpu().numpy(), z[k], rtol=1e-3, atol=2e-5, err_msg=k)
            n_grads += 1
    assert n_grads > 0
    for k, p in params.items():
        if ("grad/" + k) not in z.files and ("gradsum/" + k) not in z.files:
            assert p.grad is None, k
    sd = model.state_dict()
    for k in z.files:
        if k.startswith("state/"):
            np.testing.assert_allclose(sd[k[6:]].cpu().numpy(), z[k], rtol=1e-5, atol=1e-6, err_msg=k)
    model.eval()
    with torch.no_grad():
        pe, _ = model(x, ei, ea, batch)
    np.testing.assert_allclose(pe.cpu().numpy().reshape(-1), z["pred_eval"], **tol)
    np.testing.assert_allclose(captured["pooled"].cpu().numpy(), z["pooled_eval"], **tol)


def test_node_head_golden_through_register_readout(dev):
    """tests/test_node_heads_golden.py's super-node fixture and tolerances on the readout route."""
    from recipe import meta_from_array
    from test_node_heads_golden import TOL, _model as golden_model
    (path,) = glob.glob(os.path.join(GOLDEN, "heads", "node_stress_super_h64.npz"))
    z = np.load(path)
    meta = meta_from_array(z["meta"])
    model = golden_model(meta).to(dev)
    args = [torch.from_numpy(z[k]).to(dev) for k in ("x", "edge_index", "edge_attr", "batch")]
    y = torch.from_numpy(z["y"]).to(dev)
    ro = bgnn.register_readout(args[3], _ptr_of(z["batch"]).to(dev))
    model.train()
    pred, out_batch = model(*args)
    assert out_batch is ro.real_batch
    assert torch.equal(out_batch.cpu(), torch.from_numpy(z["out_batch"]))
    np.testing.assert_allclose(pred.detach().cpu().numpy(), z["pred_train"], **TOL)
    loss = bgnn.GraphRelativeError()(pred, y, out_batch, None)
    np.testing.assert_allclose(loss.item(), float(z["loss_train"]), **TOL)
    loss.backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    model.eval()
    with torch.no_grad():
        pe, _ = model(*args)
    np.testing.assert_allclose(pe.cpu().numpy(), z["pred_eval"], **TOL)


# ------------------------------------------------------------------------------ 7. negative cases
def test_a_store_without_super_nodes_registers_nothing(dev, monkeypatch, spy):
    store = _store(dev, (5, 7), super_node=False)
    assert not store.super_nodes
    b = store.batch([0, 1])
    assert bgnn.readout_for(b.batch) is None and "bgnn_readout_index" not in spy
    model, sd = _model("GraphSage_addAggr", "supernode_with_pooling", 64, dev)
    on = _run(model, sd, b, True, True, monkeypatch)
    assert spy.count("bgnn_sage_apply_pool") == 0
    _assert_same(on, _run(model, sd, b, True, False, monkeypatch))
    # one graph whose flag column marks a second node: no super-node store either
    graphs = [S.make_mesh_graph(5, 1, super_node=True), S.make_mesh_graph(5, 2, super_node=True)]
    graphs[1].x[3, -1] = 1.0
    assert not bgnn.GraphStore(graphs, device=dev).super_nodes


def test_hybrid_still_raises(dev, small_batch):
    _, b = small_batch
    model, _ = _model("GraphSage_addAggr", "hybrid", 64, dev)
    with pytest.raises(AttributeError, match="hybrid_pooling"):
        model(b.x, b.edge_index, b.edge_attr, b.batch)


def test_mean_on_a_super_node_batch_is_unchanged(dev, monkeypatch, spy, small_batch):
    _, b = small_batch
    model, sd = _model("GraphSage_addAggr", "mean", 64, dev)
    on = _run(model, sd, b, True, True, monkeypatch)
    n_pool = spy.count("bgnn_sage_apply_pool")
    off = _run(model, sd, b, True, False, monkeypatch)
    assert n_pool == 1 and spy.count("bgnn_sage_apply_pool") == 2   # FUSED_POOL's route, both times
    _assert_same(on, off)
