"""Node-level prediction types against the REFERENCE's own model (tests/golden/heads/node_*.npz, made
by tests/golden/make_golden_node_heads.py from Models/BuckGNN.py and Utils/Losses.py): the
node-level prediction in train and eval mode, the batch vector returned with it (real nodes only
under a "super" pooling) and the GraphRelativeError loss.

CPU: the oracle route the GPU tests use as their yardstick (oracle.buckgnn_ref.forward(...,
return_nodes=True) then _mlp(sd, "decoder", nodes)) is pinned to the reference. GPU: bgnn.BuckGNN on
both layer loops (these fixtures have < 1,024 nodes: the torch decoder) at the bounds of
tests/test_gpu_model.py:70-72 (rtol = atol = 1e-4)."""
import glob
import os

import numpy as np
import pytest
import torch

import bgnn
from recipe import make_weights, meta_from_array

FILES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "heads", "node_*.npz")))
TOL = dict(rtol=1e-4, atol=1e-4)


def _model(meta):
    m = bgnn.BuckGNN(16, 5, hidden_channels=meta["hidden"], num_layers=meta["num_layers"],
                     pooling_layer=meta["pooling"], prediction_type=meta["prediction_type"], dropout_rate=0.0,
                     model_name=meta["model_name"])
    sd = m.state_dict()
    w = make_weights({k: tuple(v.shape) for k, v in sd.items()}, meta["weight_seed"])
    m.load_state_dict({k: torch.from_numpy(w[k]) if k in w else sd[k] for k in sd})
    return m


def test_fixtures_present():
    assert len(FILES) == 2
    for p in FILES:
        assert os.path.getsize(p) < 64 << 10


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_oracle_route_matches_reference(path):
    from oracle import buckgnn_ref as R
    z = np.load(path)
    meta = meta_from_array(z["meta"])
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in _model(meta).state_dict().items()}
    x = torch.from_numpy(z["x"])
    batch = torch.from_numpy(z["batch"])
    real = x[:, -1] == 0 if "super" in meta["pooling"] else torch.ones(x.size(0), dtype=torch.bool)
    assert torch.equal(batch[real], torch.from_numpy(z["out_batch"]))
    for training, key in ((True, "pred_train"), (False, "pred_eval")):
        _, nodes = R.forward(sd, meta["model_name"], x.double(), torch.from_numpy(z["edge_index"]), batch, training,
                             meta["pooling"], 0.0, num_layers=meta["num_layers"], return_nodes=True)
        pred = R._mlp(sd, "decoder", nodes[real])
        assert pred.shape == z[key].shape
        np.testing.assert_allclose(pred.numpy(), z[key], **TOL)
        if training:
            loss = bgnn.GraphRelativeError()(pred.float(), torch.from_numpy(z["y"]), batch[real], None)
            np.testing.assert_allclose(loss.item(), float(z["loss_train"]), **TOL)
    # the loss class on the reference's own prediction: the reference's own loss
    loss = bgnn.GraphRelativeError()(torch.from_numpy(z["pred_train"]), torch.from_numpy(z["y"]),
                                     torch.from_numpy(z["out_batch"]), None)
    assert loss.item() == pytest.approx(float(z["loss_train"]), rel=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("fused_path", [True, False], ids=["fused", "per_op"])
@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_model_matches_reference_golden(dev, path, fused_path):
    z = np.load(path)
    meta = meta_from_array(z["meta"])
    model = _model(meta).to(dev)
    model.use_fused = fused_path
    args = [torch.from_numpy(z[k]).to(dev) for k in ("x", "edge_index", "edge_attr", "batch")]
    y = torch.from_numpy(z["y"]).to(dev)
    model.train()
    pred, out_batch = model(*args)
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
