"""C-ABI of the static heads' metric table (ABI 22): bgnn_graph_metrics / bgnn_graph_metrics_ws_bytes.
The header declares them, the library exports them with the same argument counts as bgnn._lib's
table, every argument check answers BGNN_E_ARG before anything touches a device (no GPU here: the
pointers below are never dereferenced), and bgnn.losses.METRIC_KEYS mirrors the column order with the
key set of the reference's own stress_errors (tests/golden/heads/metrics.npz)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # an aligned non-NULL "pointer"
ENTRIES = {
    "bgnn_graph_metrics_ws_bytes": ("size_t", 3),
    "bgnn_graph_metrics": ("int", 15),
}


def test_header_declares_and_library_exports():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 22
    assert int(re.search(r"#define\s+BGNN_GRAPH_METRICS_COLS\s+(\d+)", text).group(1)) == 30
    lib = _lib.load()
    assert lib.bgnn_abi_version() == 22
    for name, (ret, n_args) in ENTRIES.items():
        decl = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (ret, name), text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name


def _call(pred=P, target=P, N=100, C=3, rowptr=P, col=P, B=4, mode=0, threshold=0.2, scale=None, center=None, out=P,
          ws=P, ws_bytes=1 << 20):
    from bgnn import _lib

    return _lib.call("bgnn_graph_metrics", pred, target, N, C, rowptr, col, B, mode, threshold, scale, center, out,
                     ws, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(C=0), "C=0 unsupported"),
    (dict(C=9), "C=9 unsupported"),
    (dict(mode=2), "mode 2 unknown"),
    (dict(mode=-1), "mode -1 unknown"),
    (dict(mode=0, C=2), "mode 0 needs C >= 3"),
    (dict(mode=1, C=1), "mode 1 needs C >= 2"),
    (dict(N=0), "must be in"),
    (dict(B=0), "must be in"),
    (dict(N=2 ** 30, C=8), "must be in"),
    (dict(pred=None), "null pointer"),
    (dict(target=None), "null pointer"),
    (dict(rowptr=None), "null pointer"),
    (dict(col=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(out=P + 4), "out must be 8-byte aligned"),
    (dict(ws=None), "workspace too small"),
    (dict(ws=P + 4), "not 8-byte aligned"),
    (dict(ws_bytes=0), "workspace too small"),
])
def test_argument_checks(kw, msg):
    from bgnn import _lib

    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _call(**kw)
    assert e.value.code == 1001   # BGNN_E_ARG


def test_workspace_query():
    from bgnn import _lib

    for N, C, B in ((100, 3, 4), (80656, 2, 16), (10 ** 7, 8, 1)):
        n = _lib.query("bgnn_graph_metrics_ws_bytes", N, C, B)
        assert n > 0 and n % 8 == 0
        with pytest.raises(_lib.BgnnError, match="workspace too small"):
            _call(N=N, C=C, B=B, mode=1, ws_bytes=n - 1)
    assert _lib.query("bgnn_graph_metrics_ws_bytes", 100, 3, 0) == 0


def test_metric_keys_mirror_the_reference():
    import bgnn
    from bgnn import losses

    gold = np.load(os.path.join(ROOT, "tests", "golden", "heads", "metrics.npz"))
    seen = set()
    for tag in ("stress", "disp"):
        kind = str(gold[f"{tag}_kind"])
        seen.add(kind)
        keys = losses.METRIC_KEYS[kind]
        assert len(keys) == 28 == len(set(keys))
        assert sorted(keys) == [str(k) for k in gold[f"{tag}_keys"]]
    assert seen == set(losses.METRIC_KEYS) == {"static_stress", "static_disp"}
    assert losses.GRAPH_METRICS_COLS == 30 and losses.FUSED_STRESS_ERRORS in (True, False)
    assert bgnn.StressErrorMeter is losses.StressErrorMeter and callable(bgnn.evaluate_nodes)
    assert bgnn.graph_metrics is losses.graph_metrics


def test_meter_defaults_and_cpu_path():
    """The meter's thresholds are the reference's; on CPU tensors it runs the torch stress_errors."""
    import torch
    from bgnn import losses

    assert losses.StressErrorMeter("static_disp").threshold == 1e-4
    assert losses.StressErrorMeter("static_stress").threshold == 0.2
    with pytest.raises(ValueError):
        losses.StressErrorMeter("buckling")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "heads", "metrics.npz"))
    p, t, b = (torch.from_numpy(gold[f"stress_{k}"]) for k in ("pred", "target", "batch"))
    assert losses.graph_metrics(p, t, b, "static_stress", 0.2) is None   # CPU tensors: declined
    m = losses.StressErrorMeter("static_stress")
    assert all(np.isnan(v) for v in m.compute().values())
    m.update(p, t, b)
    m.update(p, t, b)
    assert m.counts == (2 * (int(b.max()) + 1), 2)
    want = losses.stress_errors(p, t, b, "static_stress", 0.2)
    per_batch, per_graph = m.compute("batch"), m.compute("graph")
    for k in losses.METRIC_KEYS["static_stress"]:
        assert per_batch[k] == pytest.approx(want[k], rel=1e-12)
        assert per_graph[k] == pytest.approx(want[k] / (int(b.max()) + 1), rel=1e-12)
    m.reset()
    assert m.counts == (0, 0)
