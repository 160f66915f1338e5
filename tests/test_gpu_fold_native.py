"""GPU: the folded layer's grouped weight products (csrc/fold.hip, bgnn_fold_weights_fwd / _bwd)
against the chain of bgnn GEMMs, max passes and torch launches they replace (bgnn/fused.py,
SageLayerFn with w_in, FOLD_NATIVE off), run on the same device tensors. The two are the same
arithmetic -- the operand scales, the f16 piece split, the 32x32x16 MFMA order, the K ranges of the
planner's split and the epilogue -- so every output and every maxima slot must agree bit for bit
(compared as int32, so that an Inf - Inf NaN of the 1e30 inputs must agree too). Outputs sit in
NaN-filled windows of guarded buffers whose guard pattern must survive."""
import pytest
import torch

from bgnn import _lib, fused
from bgnn.graph import _stream

pytestmark = pytest.mark.gpu

PATTERN = 0x4B1D5EED   # guard bit pattern (tests/test_gpu_gemm_matrix.py)
GUARD = 64             # guard elements before and after a window (a multiple of 4: 16-B aligned windows)
SHAPES = [(64, 32), (128, 128), (80, 48), (512, 128)]
# name -> (scale of Wcat, dWf, dbf; scale of W_in, b_in; b_in zeroed)
INPUTS = {
    "random": (1.0, 1.0, False),
    "b_in_zero": (1.0, 1.0, True),      # zero maximum -> unit scale, bf = 0
    "tiny": (1e-30, 1e-30, False),
    "huge": (1e30, 1e30, False),
    "huge_tiny": (1e30, 1e-30, False),  # the two unscales meet: the one-multiply / two-multiply paths
}


class Window:
    """A rows x cols f32 window (row stride ld) inside a guarded flat buffer, pre-filled with NaN."""

    def __init__(self, rows, cols, ld, dev, off=0):
        n = (rows - 1) * ld + cols
        g = GUARD + off   # off elements further: a window base that is not 16-B aligned
        self.flat = torch.full((n + 2 * GUARD + off,), PATTERN, dtype=torch.int32, device=dev)
        self.view = self.flat.view(torch.float32)[g:g + n].as_strided((rows, cols), (ld, 1))
        self.mask = torch.ones(n + 2 * GUARD + off, dtype=torch.bool, device=dev)
        self.mask[g:g + n].as_strided((rows, cols), (ld, 1)).fill_(False)
        self.view.fill_(float("nan"))

    def assert_guard(self, label):
        assert bool((self.flat[self.mask] == PATTERN).all()), f"{label}: guard overwritten"


def operand(rows, cols, ld, scale, gen, dev, off=0):
    buf = torch.randn(rows * ld + off, generator=gen, dtype=torch.float32).to(dev) * scale
    return buf[off:].view(rows, ld)[:, :cols]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b, label):
    assert torch.equal(bits(a), bits(b)), f"{label}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ"


def chain_fwd(wcat, w_in, b_in, fs, w_amax, wf, bf, wf_t):
    """SageLayerFn.forward's folded block on the bgnn GEMMs."""
    H = w_in.size(0)
    fused.absmax(wcat, fs[0:1], accumulate=True)
    fused.absmax(w_in, fs[1:2], accumulate=True)
    fused.absmax(b_in.view(1, -1), fs[2:3], accumulate=True)
    fused.gemm(wcat, w_in, trans_a=False, trans_b=False, out=wf, a_amax=fs[0:1], b_amax=fs[1:2])
    fused.gemm(wcat, b_in.view(H, 1), trans_a=False, trans_b=False, out=bf.view(-1, 1), a_amax=fs[0:1],
               b_amax=fs[2:3])
    fused.absmax(wf, w_amax, accumulate=True)
    wf_t.copy_(wf.t())


def chain_bwd(dwf, db2, wcat, w_in, b_in, fs, dw, dw_in, db_in):
    """SageLayerFn.backward's folded block on the bgnn GEMMs and torch's outer / add_."""
    dbf = db2.view(-1)
    fused.absmax(db2, fs[4:5], accumulate=True)
    fused.gemm(dwf, w_in, trans_a=False, trans_b=True, out=dw, a_amax=fs[3:4], b_amax=fs[1:2])
    dw.add_(torch.outer(dbf, b_in))
    fused.gemm(wcat, dwf, trans_a=True, trans_b=False, out=dw_in, a_amax=fs[0:1], b_amax=fs[3:4])
    fused.gemm(wcat, dbf.view(-1, 1), trans_a=True, trans_b=False, out=db_in.view(-1, 1), a_amax=fs[0:1],
               b_amax=fs[4:5])


# (leading-dimension pad, base offset in elements): the last keeps ld % 4 == 0 on 4-byte-offset
# bases, so every 16-byte path falls back on the pointer's alignment alone
@pytest.mark.parametrize("pad,off", [(0, 0), (12, 0), (3, 0), (12, 1)], ids=["dense", "ld", "ld_odd", "unaligned"])
@pytest.mark.parametrize("kind", list(INPUTS))
@pytest.mark.parametrize("H,K", SHAPES)
def test_native_fold_matches_gemm_chain(dev, H, K, kind, pad, off):
    s_out, s_in, zero_b = INPUTS[kind]
    gen = torch.Generator().manual_seed(1000 * H + K)
    wcat = operand(2 * H, H, H + pad, s_out, gen, dev, off)
    w_in = operand(H, K, K + pad, s_in, gen, dev, off)
    b_in = (torch.zeros(H + off, device=dev) if zero_b else
            torch.randn(H + off, generator=gen, dtype=torch.float32).to(dev) * s_in)[off:]
    dwf = operand(2 * H, K, K + pad, s_out, gen, dev, off)
    db2 = (torch.randn(2 * H + off, generator=gen, dtype=torch.float32).to(dev) * s_out)[off:].view(2, H)
    assert _lib.query("bgnn_fold_weights_supported", H, K) == 1
    label = f"H={H} K_in={K} {kind} pad={pad} off={off}"

    def outputs():
        return {"wf": Window(2 * H, K, K + pad, dev, off), "bf": Window(1, 2 * H, 2 * H, dev, off),
                "wf_t": Window(K, 2 * H, 2 * H + pad, dev, off), "dw": Window(2 * H, H, H + pad, dev, off),
                "dw_in": Window(H, K, K + pad, dev, off), "db_in": Window(1, H, H, dev, off)}

    ref, got = outputs(), outputs()
    fs_r = torch.zeros(5, device=dev)
    fs_n = torch.zeros(5, device=dev)
    wa_r = torch.zeros(1, device=dev)
    wa_n = torch.zeros(1, device=dev)
    # max|dWf| comes from the weight-gradient GEMM's epilogue in the layer: given here
    fused.absmax(dwf, fs_r[3:4], accumulate=True)
    fs_n[3:4].copy_(fs_r[3:4])

    chain_fwd(wcat, w_in, b_in, fs_r, wa_r, ref["wf"].view, ref["bf"].view.view(-1), ref["wf_t"].view)
    chain_bwd(dwf, db2, wcat, w_in, b_in, fs_r, ref["dw"].view, ref["dw_in"].view, ref["db_in"].view.view(-1))

    s = _stream()
    g = {k: w.view for k, w in got.items()}
    _lib.call("bgnn_fold_weights_fwd", H, K, wcat.data_ptr(), wcat.stride(0), w_in.data_ptr(), w_in.stride(0),
              b_in.data_ptr(), fs_n.data_ptr(), g["wf"].data_ptr(), g["wf"].stride(0), g["bf"].data_ptr(),
              g["wf_t"].data_ptr(), g["wf_t"].stride(0), wa_n.data_ptr(), s)
    ws_bytes = _lib.query("bgnn_fold_weights_ws_bytes", H, K)
    ws = Window(1, max(ws_bytes // 4, 1), max(ws_bytes // 4, 1), dev, off)
    _lib.call("bgnn_fold_weights_bwd", H, K, dwf.data_ptr(), dwf.stride(0), db2.data_ptr(), wcat.data_ptr(),
              wcat.stride(0), w_in.data_ptr(), w_in.stride(0), b_in.data_ptr(), fs_n.data_ptr(), g["dw"].data_ptr(),
              g["dw"].stride(0), g["dw_in"].data_ptr(), g["dw_in"].stride(0), g["db_in"].data_ptr(),
              ws.view.data_ptr() if ws_bytes else None, ws_bytes, s)
    torch.cuda.synchronize()

    if H == 512:   # the real shape runs the planner's split-K plan for dW_in and db_in
        assert ws_bytes > 0
    for k in ref:
        same_bits(got[k].view, ref[k].view, f"{label} {k}")
        got[k].assert_guard(f"{label} {k}")
        ref[k].assert_guard(f"{label} {k} (chain)")
    ws.assert_guard(f"{label} workspace")
    same_bits(fs_n, fs_r, f"{label} fold_amax")
    same_bits(wa_n, wa_r, f"{label} max|Wf|")
    if zero_b:
        assert float(fs_n[2]) == 0.0 and not bool(got["bf"].view.any())
    if kind == "random":   # the check is not NaN == NaN throughout
        assert all(bool(torch.isfinite(w.view).all()) for w in got.values())
