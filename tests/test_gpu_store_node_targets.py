"""GraphStore batches of graphs with a node-level target y (one row per real node: with a super node
y has one row fewer than x, so the store does not class it as a per-node tensor): the batch must
equal host collation (Batch.from_data_list), the graph-order concatenation train_step's node-level
losses expect."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _graphs(super_node, sizes, C=3):
    from bgnn import synthetic
    out = []
    for i, n in enumerate(sizes):
        d = synthetic.make_mesh_graph(n, 60 + i, super_node=super_node)
        n_real = d.x.size(0) - (1 if super_node else 0)
        g = torch.Generator().manual_seed(i)
        d.y = torch.randn(n_real, C, generator=g)
        out.append(d)
    return out


@pytest.mark.parametrize("sizes", [[4, 6, 5, 3], [5, 5, 5]], ids=["ragged", "equal"])
@pytest.mark.parametrize("super_node", [False, True])
def test_store_batch_of_node_targets_equals_host_collation(dev, super_node, sizes):
    import bgnn
    graphs = _graphs(super_node, sizes)
    store = bgnn.GraphStore(graphs, device=dev)
    for ids in ([0, 1, 2], [2, 0], list(range(len(sizes)))[::-1], [1]):
        got = store.batch(ids)
        want = bgnn.Batch.from_data_list([graphs[i] for i in ids])
        assert got.y.device.type == "cuda"
        assert torch.equal(got.y.cpu(), want.y)
        assert torch.equal(got.x.cpu(), want.x)
        assert torch.equal(got.batch.cpu(), want.batch)
        n_real = int((want.x[:, -1] == 0).sum()) if super_node else want.x.size(0)
        assert got.y.shape == (n_real, 3)
