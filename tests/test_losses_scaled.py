"""The eight criterion(pred, target, batch, x) classes of bgnn.losses against the reference's own
(tests/golden/heads/losses_scaled.npz, made by tests/golden/make_golden_losses_scaled.py from
Utils/Losses.py:303-695): values and autograd gradients with respect to pred, with and without a
batch vector, the force-scaled ones with the forces on, off, and small enough that min_scale wins;
and bgnn.get_loss_function over every name of the reference's table. CPU tensors: the torch routes."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "heads", "losses_scaled.npz")
TAGS = ("s3", "d3", "v1", "m3")
NAMES = {"rel": "GraphRelativeError", "mixed": "GraphMixedError", "mse": "GraphMSELoss", "mae": "GraphMAELoss",
         "maxc": "GraphMaxComponentRelativeError", "mae_scaled": "ScaledGraphMAELoss",
         "mse_scaled": "ScaledGraphMSELoss", "rel_scaled": "ScaledGraphRELoss"}
SCALED = ("mae_scaled", "mse_scaled", "rel_scaled")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _variants(name):
    return (("", {}), ("_noforce", {"force_scaling": False})) if name in SCALED else (("", {}),)


@pytest.mark.parametrize("name", list(NAMES))
@pytest.mark.parametrize("tag", TAGS)
def test_values_and_gradients_match_the_reference(gold, tag, name):
    from bgnn import losses
    p, t, b, x = (torch.from_numpy(gold[f"{tag}_{k}"]) for k in ("pred", "target", "batch", "x"))
    n = 0
    for suffix, kw in _variants(name):
        mod = getattr(losses, NAMES[name])(**kw)
        for bsuffix, bv in (("", b), ("_nobatch", None)):
            key = f"{tag}_{name}{suffix}{bsuffix}"
            pr = p.clone().requires_grad_(True)
            v = mod(pr, t, bv, x)
            g, = torch.autograd.grad(v, pr)
            assert v.item() == pytest.approx(float(gold[key]), rel=2e-5), key
            want = gold[key + "_grad"]
            assert g.shape == want.shape
            np.testing.assert_allclose(g.numpy(), want, rtol=2e-5, atol=0, err_msg=key)
            n += 1
    assert n == (4 if name in SCALED else 2)


def test_min_scale_wins_in_the_small_force_case(gold):
    """m3's total force is below min_scale = 0.1 (the clamp decides the value); the others' is above."""
    from bgnn import losses
    mod = losses.ScaledGraphMAELoss()
    for tag in TAGS:
        total = float(mod.compute_total_force(torch.from_numpy(gold[f"{tag}_x"])))
        assert (total < 0.1) == (tag == "m3"), (tag, total)
    p, t, b, x = (torch.from_numpy(gold[f"m3_{k}"]) for k in ("pred", "target", "batch", "x"))
    for name in SCALED:
        on = float(gold[f"m3_{name}"])
        off = float(gold[f"m3_{name}_noforce"])
        assert on == pytest.approx(0.1 * off, rel=1e-5)
        assert getattr(losses, NAMES[name])(min_scale=0.5)(p, t, b, x).item() == pytest.approx(0.5 * off, rel=2e-5)


@pytest.mark.parametrize("name", SCALED)
def test_force_scaling_needs_x(gold, name):
    from bgnn import losses
    p, t, b = (torch.from_numpy(gold[f"s3_{k}"]) for k in ("pred", "target", "batch"))
    cls = getattr(losses, NAMES[name])
    for bv in (b, None):
        with pytest.raises(ValueError, match="needs the node features x"):
            cls()(p, t, bv, None)
        assert torch.isfinite(cls(force_scaling=False)(p, t, bv, None))
    assert cls().force_scaling is True and cls().min_scale == 0.1


def test_scaled_mse_without_a_batch_vector_is_the_mae(gold):
    """The reference's quirk: ScaledGraphMSELoss without a batch vector returns mean |p - t| * scale."""
    from bgnn import losses
    p, t, x = (torch.from_numpy(gold[f"d3_{k}"]) for k in ("pred", "target", "x"))
    assert losses.ScaledGraphMSELoss()(p, t, None, x).item() == pytest.approx(
        losses.ScaledGraphMAELoss()(p, t, None, x).item(), rel=1e-7)
    assert float(gold["d3_mse_scaled_nobatch"]) == pytest.approx(float(gold["d3_mae_scaled_nobatch"]), rel=1e-7)


def test_get_loss_function():
    import bgnn
    from bgnn import losses
    table = {"graph_rel": losses.GraphRelativeError, "graph_mae": losses.GraphMAELoss, "graph_mse": losses.GraphMSELoss,
             "graph_mixed": losses.GraphMixedError, "graph_max_rel": losses.GraphMaxComponentRelativeError,
             "graph_rel_scaled": losses.ScaledGraphRELoss, "graph_mae_scaled": losses.ScaledGraphMAELoss,
             "graph_mse_scaled": losses.ScaledGraphMSELoss, "relative_error": bgnn.RelativeErrorLoss,
             "mse": torch.nn.MSELoss}
    for name, cls in table.items():
        assert type(bgnn.get_loss_function(name)) is cls, name
    assert type(bgnn.get_loss_function("graph_mae", allValues=[1.0], use_z_coord=True, use_rotations=True)) \
        is losses.GraphMAELoss
    for name in ("static_mixed", "static_mse", "static_relative", "static_stress", "static_mae", "log_cosh",
                 "eigenvalue", "order_preserving", "focal", "mape", "mae", "rse", "rrse", "rrse1", "msle",
                 "focal_rrse", "focal_mape"):
        with pytest.raises(NotImplementedError, match=name):
            bgnn.get_loss_function(name)
    with pytest.raises(ValueError, match="Unknown loss function: no_such_loss"):
        bgnn.get_loss_function("no_such_loss")
